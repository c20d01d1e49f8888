"""siggan_g_latent_grad (Engine.g_latent_grad): the eval-mode Generator forward, the per-image reconstruction loss
mean((G(z) - t)^2) and its gradient with respect to z.

The gradient is held to the oracle in fp64 on the device's own sign decisions (the README parity contract's "HIP =
oracle(HIP's decisions)", 1e-4 of max|dz_ref|), the decisions to the fp64 run's own wherever that run is not borderline, the
loss to numpy fp64 on the device's own images, the images to g_forward bit for bit.  The final conv carries a gain so that the
images span the range and saturate in places; the targets are the bytes of G at another z, so x - t is far from the
quantisation floor.  One case per path: ragged GEMM rows (batch 3), one sample, 128x128 (five blocks, F = 8192), latent 50
(the generic fc kernels in the forward, a ragged second k pass in dz), LeakyReLU(0.2)."""
import ctypes as C

import numpy as np
import pytest
import torch

from common import I, SEED
from latentcommon import oracle_latent_grad, oracle_sd64

pytestmark = pytest.mark.gpu

GAIN = {64: 32.0, 128: 16.0}       # the oracle on the CPU: 6-20 % of the bytes at 255 and a minimum of 0-41 (64x64), all 256 values (128x128)
CASES = [(64, 100, 3, 0.0), (64, 100, 1, 0.0), (128, 128, 2, 0.0), (64, 50, 2, 0.0), (64, 100, 2, 0.2)]


def _engine(size, latent, batch, slope, dtype="f32"):
    from hipcommon import load_engine_state
    from signature_gan_amd.engine import Engine
    kw = dict(g_activation="leaky_relu", g_leaky_slope=slope) if slope else {}
    eng = load_engine_state(Engine(latent_dim=latent, image_size=size, max_batch=batch, device="cuda:0", seed=0, dtype=dtype, **kw),
                            size, latent, False)
    v = eng.views("g")
    v["final_conv.0.weight"].mul_(GAIN[size]); v["final_conv.0.bias"].mul_(GAIN[size])
    eng.params_changed()
    return eng


def compute_case(case):
    """Everything the tests of one case compare, computed once and brought to the CPU (also what
    profiles/projection_parity_margins.py records)."""
    from hipcommon import hip_signs_g
    from signature_gan_amd import _lib
    size, latent, batch, slope = case
    eng = _engine(size, latent, batch, slope)
    z = torch.from_numpy(I.gen_z(batch, latent, SEED["z"]))
    z_t = torch.from_numpy(I.gen_z(batch, latent, SEED["z"] + 1))
    t_u8 = eng.g_generate_u8(z_t.cuda())
    lut = torch.from_numpy(_lib.dequant_table())
    t_f32 = lut[t_u8.cpu().long()].unsqueeze(1).contiguous()
    want_img = eng.g_forward(z.cuda(), training=False).cpu()
    dz, loss, img = eng.g_latent_grad(z.cuda(), t_u8, want_images=True)
    signs = hip_signs_g(eng, size, batch)
    dz_f, loss_f = eng.g_latent_grad(z.cuda(), t_f32.cuda())
    dz_2, loss_2 = eng.g_latent_grad(z.cuda(), t_u8)
    out = {"case": case, "dz": dz.cpu(), "loss": loss.cpu(), "img": img.cpu(), "want_img": want_img, "signs": signs,
           "dz_f": dz_f.cpu(), "loss_f": loss_f.cpu(), "dz_2": dz_2.cpu(), "loss_2": loss_2.cpu(), "t_u8": t_u8.cpu().numpy()}
    eng.close()
    rec = []
    out["dz_ref"], out["loss_ref"] = oracle_latent_grad(oracle_sd64(size, latent, GAIN[size]), z, t_f32[:, 0].double(), size, signs, slope, rec)
    out["rec"], out["t64"] = rec, t_f32[:, 0].double().numpy()
    return out


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"s{c[0]}-z{c[1]}-b{c[2]}-slope{c[3]:g}")
def run(request):
    return compute_case(request.param)


def test_gradient_is_the_oracles_on_the_devices_decisions(run):
    ref = run["dz_ref"]
    err = float((run["dz"].double() - ref).abs().max()) / float(ref.abs().max())
    print(f"{run['case']}: max|dz - dz_ref| / max|dz_ref| = {err:.3e}  (max|dz_ref| {float(ref.abs().max()):.3e})")
    assert run["dz"].shape == ref.shape and float(ref.abs().max()) > 0
    assert err <= 1e-4, err


def test_decisions_differ_only_where_fp64_is_borderline(run):
    from hipcommon import count_sign_flips
    n = count_sign_flips(run["signs"], run["rec"])       # asserts |pre| <= 1e-5 of its layer's max|pre| wherever the signs differ
    print(f"{run['case']}: {n} borderline decisions of {sum(x.numel() for x in run['rec'])}")


def test_loss_is_the_mean_square_of_the_devices_images(run):
    size = run["case"][0]
    x = run["img"][:, 0].double().numpy()
    want = ((x - run["t64"]) ** 2).mean(axis=(1, 2))
    rel = np.abs(run["loss"].double().numpy() - want) / want
    print(f"{run['case']}: loss {run['loss'].numpy()}, rel err {rel.max():.3e}")
    assert (want > 1e-4).all()                           # the targets are other images, not the quantised own
    assert rel.max() <= size * size * 2.0 ** -24, rel
    # (the fp64 oracle's loss differs by its images' ~1e-6 only: the two references agree)
    assert np.allclose(want, run["loss_ref"].numpy(), rtol=1e-3)


def test_images_are_g_forwards(run):
    assert torch.equal(run["img"], run["want_img"])
    u8 = run["t_u8"]
    assert len(np.unique(u8)) >= 32 and u8.min() < 64 and u8.max() == 255          # the gain spans the range and saturates its top


def test_byte_and_fp32_targets_give_the_same_bits(run):
    assert torch.equal(run["dz"], run["dz_f"]) and torch.equal(run["loss"], run["loss_f"])


def test_two_calls_give_the_same_bits(run):
    assert torch.equal(run["dz"], run["dz_2"]) and torch.equal(run["loss"], run["loss_2"])


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_training_state_is_untouched(graph):
    """train_step; g_latent_grad; train_step leaves exactly what two train_steps leave."""
    from hipcommon import assert_same_state, cuda, full_state, make_engine
    size, latent, batch = 64, 100, 4
    real = [cuda(I.gen_real(batch, size, SEED["real"] + i)) for i in range(2)]
    zs = [cuda(I.gen_z(batch, latent, SEED["z"] + 10 + i)) for i in range(5)]
    states = []
    for with_call in (False, True):
        eng = make_engine(size, latent, batch, warm=True)
        if graph:
            eng.set_mode(graph=True)
        eng.train_step(real[0], zs[0], None, zs[1])
        if with_call:
            t_u8 = torch.randint(0, 256, (batch, size, size), dtype=torch.uint8, generator=torch.Generator().manual_seed(5)).cuda()
            eng.g_latent_grad(zs[4], t_u8)
        eng.train_step(real[1], zs[2], None, zs[3])
        torch.cuda.synchronize()
        states.append(full_state(eng))
        eng.close()
    assert_same_state(states[0], states[1], "a training step after g_latent_grad")


def _raw_call(eng, z, t_u8, t_f32, dz, loss, batch):
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    return eng.lib.siggan_g_latent_grad(eng._h, p(z), batch, p(t_u8), p(t_f32), p(dz), p(loss), None, eng._stream())


def test_refusals_enqueue_nothing():
    from signature_gan_amd import _lib
    size, latent, batch = 64, 100, 2
    z = torch.from_numpy(I.gen_z(4, latent, SEED["z"])).cuda()
    t_u8 = torch.zeros(4, size, size, dtype=torch.uint8, device="cuda")
    t_f32 = torch.zeros(4, 1, size, size, dtype=torch.float32, device="cuda")

    def refused(eng, *args):
        dz = torch.full((4, latent), 7.0, device="cuda")
        loss = torch.full((4,), 7.0, device="cuda")
        rc = _raw_call(eng, *args[:3], dz, loss, args[3])
        torch.cuda.synchronize()
        assert rc == -1, (rc, eng.lib.siggan_last_error())                 # SIGGAN_E_INVALID
        with pytest.raises(ValueError):
            _lib.check(rc)
        assert bool((dz == 7.0).all()) and bool((loss == 7.0).all())       # nothing ran

    eng = _engine(size, latent, batch, 0.0)
    refused(eng, z, t_u8, t_f32, batch)                                    # both targets
    refused(eng, z, None, None, batch)                                     # neither
    refused(eng, z, t_u8, None, batch + 1)                                 # beyond the context's maximum
    refused(eng, z, t_u8, None, 0)
    assert _raw_call(eng, z, t_u8, None, None, torch.empty(4, device="cuda"), batch) == -1      # null dz
    assert _raw_call(eng, z, t_u8, None, torch.empty(4, latent, device="cuda"), None, batch) == -1
    with pytest.raises(ValueError):
        eng.g_latent_grad(z[:batch], t_u8[:batch].float())                 # fp32 targets are (B, 1, S, S)
    with pytest.raises(ValueError):
        eng.g_latent_grad(z[:batch, :50], t_u8[:batch])
    dz, loss = eng.g_latent_grad(z[:batch], t_u8[:batch])                  # the context still works
    assert bool(torch.isfinite(dz).all()) and bool((loss > 0).all())
    eng.close()
    eng16 = _engine(size, latent, batch, 0.0, dtype="bf16")
    refused(eng16, z, t_u8, None, batch)                                   # a 16-bit context
    with pytest.raises(ValueError):
        eng16.g_latent_grad(z[:batch], t_u8[:batch])
    eng16.close()
