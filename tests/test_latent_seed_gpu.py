"""siggan_g_latent_objective_grad_seeded (Engine.g_latent_objective_grad(image_grad=...)): the latent objective's gradient plus
J_G(z)^T of a caller-supplied image-space gradient.

A zero seed gives the unseeded call's bits; with all weights 0 the call is linear in the seed (a power-of-two scaling is exact)
and dz is held to the existing fp64 oracle on the device's own sign decisions at the README contract's 1e-4 of max|dz_ref| --
oracle_objective yields J_G^T seed when it is handed the fp64 target t = x64 - (S^2 / 2) seed with the weights (1, 0, 0), x64 its
own image on those decisions; with the weights (1, 1, 1) the seed's share of dz is the seed-only dz; training state is untouched.
Cases: the 64x64 cases of objectivecommon.CASES."""
import ctypes as C

import pytest
import torch

from common import I, O, SEED
from latentcommon import oracle_sd64
from objectivecommon import CASES, GAIN, WEIGHTS, lut_f32, objective_engine, oracle_d_sd64, oracle_objective

pytestmark = pytest.mark.gpu
CASES64 = [c for c in CASES if c[0] == 64]
ONES = (1.0, 1.0, 1.0)
ZERO = (0.0, 0.0, 0.0)


def make_seed(batch, size, k=0):
    g = torch.Generator().manual_seed(90 + k)
    return (torch.randn(batch, 1, size, size, generator=g) / float(size * size)).contiguous()


def compute_case(case):
    from hipcommon import hip_signs_g
    size, latent, batch, slope, sn = case
    eng = objective_engine(size, latent, batch, slope, sn)
    z = torch.from_numpy(I.gen_z(batch, latent, SEED["z"]))
    zc = z.cuda()
    t_u8 = eng.g_generate_u8(torch.from_numpy(I.gen_z(batch, latent, SEED["z"] + 1)).cuda())
    seed = make_seed(batch, size)
    sc, zero = seed.cuda(), torch.zeros_like(seed).cuda()
    cpu = lambda ts: tuple(t.cpu() for t in ts)
    kw = dict(want_terms=True, want_images=True)
    out = {"case": case, "z": z, "seed": seed}
    uv = {k: v.cpu().clone() for k, v in eng.sn_views().items()} if sn else None
    out["want_img"] = eng.g_forward(zc, training=False).cpu()
    frozen = lambda: {**{k: v.clone() for k, v in eng.bn_views().items()}, **({k: v.clone() for k, v in eng.sn_views().items()} if sn else {})}
    before = frozen()
    for w in WEIGHTS:
        t = t_u8 if w[0] else None
        out["plain", w] = cpu(eng.g_latent_objective_grad(zc, t, *w, want_probs=w[1] > 0, **kw))
        out["zero", w] = cpu(eng.g_latent_objective_grad(zc, t, *w, want_probs=w[1] > 0, image_grad=zero, **kw))
    out["plain", ONES] = cpu(eng.g_latent_objective_grad(zc, t_u8, *ONES, want_probs=True, **kw))
    out["seeded", ONES] = cpu(eng.g_latent_objective_grad(zc, t_u8, *ONES, want_probs=True, image_grad=sc, **kw))
    out["seed2"] = cpu(eng.g_latent_objective_grad(zc, None, *ZERO, image_grad=2.0 * sc, **kw))
    out["seed1"] = cpu(eng.g_latent_objective_grad(zc, None, *ZERO, image_grad=sc, **kw))
    out["signs_g"] = hip_signs_g(eng, size, batch)
    out["again"] = cpu(eng.g_latent_objective_grad(zc, None, *ZERO, image_grad=sc, **kw))
    out["squeezed"] = cpu(eng.g_latent_objective_grad(zc, None, *ZERO, image_grad=sc[:, 0], **kw))
    after = frozen()
    out["frozen"] = [(k, torch.equal(before[k], after[k])) for k in before]
    eng.close()
    g64 = oracle_sd64(size, latent, GAIN[size])
    with torch.no_grad():
        x64 = O.g_forward(g64, z.double(), False, size, signs=out["signs_g"], slope=slope)[:, 0]
    t64 = x64 - (size * size / 2.0) * seed[:, 0].double()
    _, grads, _ = oracle_objective(g64, oracle_d_sd64(size, uv), z, t64, size, out["signs_g"], None, slope)
    out["dz_ref"] = grads[0]
    return out


@pytest.fixture(scope="module", params=CASES64, ids=lambda c: f"s{c[0]}-z{c[1]}-b{c[2]}-slope{c[3]:g}{'-sn' if c[4] else ''}")
def run(request):
    return compute_case(request.param)


def test_a_zero_seed_gives_the_unseeded_bits(run):
    for w in WEIGHTS:
        for name, a, b in zip(("dz", "objective", "terms", "probs/images", "images"), run["plain", w], run["zero", w]):
            assert torch.equal(a, b), (w, name)


def test_doubling_the_seed_doubles_dz_bit_for_bit(run):
    dz1, dz2 = run["seed1"][0], run["seed2"][0]
    assert float(dz1.abs().max()) > 0
    assert torch.equal(2.0 * dz1, dz2)
    for a, b in zip(run["seed1"], run["again"]):                           # two calls on equal inputs: equal bits
        assert torch.equal(a, b)
    for a, b in zip(run["seed1"], run["squeezed"]):                        # (B, S, S) is the same memory
        assert torch.equal(a, b)


def test_seed_only_objective_and_terms_are_zero(run):
    dz, obj, terms, img = run["seed1"]
    assert not obj.any() and not terms.any()
    assert torch.equal(img, run["want_img"])


def test_seed_only_dz_is_the_oracles_vjp_on_the_devices_decisions(run):
    ref = run["dz_ref"]
    scale = float(ref.abs().max())
    err = float((run["seed1"][0].double() - ref).abs().max()) / scale
    print(f"{run['case']}: max|dz - J^T seed| / max|J^T seed| = {err:.3e}  (max {scale:.3e})")
    assert scale > 0 and err <= 1e-4


def test_the_seeds_share_of_a_full_objective_is_the_seed_only_dz(run):
    ref = run["dz_ref"]
    scale = float(ref.abs().max())
    share = run["seeded", ONES][0].double() - run["plain", ONES][0].double()
    err = float((share - ref).abs().max()) / scale
    print(f"{run['case']}: max|(dz_seeded - dz_unseeded) - J^T seed| / max|J^T seed| = {err:.3e}  "
          f"(max|dz_unseeded| {float(run['plain', ONES][0].abs().max()):.3e})")
    assert err <= 1e-4
    for a, b in zip(run["seeded", ONES][1:], run["plain", ONES][1:]):      # objective, terms, probs, images never see the seed
        assert torch.equal(a, b)


def test_images_are_the_eval_forward(run):
    for key in (("seeded", ONES), ("zero", WEIGHTS[0]), "seed1", "seed2"):
        assert torch.equal(run[key][-1], run["want_img"]), key


def test_batchnorm_buffers_and_u_v_do_not_move(run):
    assert run["frozen"] and all(same for _, same in run["frozen"]), run["frozen"]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_training_state_is_untouched(graph):
    """train_step; a seeded call with all three weights; train_step leaves exactly what two train_steps leave."""
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
            eng.g_latent_objective_grad(zs[4], t_u8, *ONES, want_terms=True, want_probs=True, image_grad=make_seed(batch, size).cuda())
        eng.train_step(real[1], zs[2], None, zs[3])
        torch.cuda.synchronize()
        states.append(full_state(eng))
        eng.close()
    assert_same_state(states[0], states[1], "a training step after the seeded g_latent_objective_grad")


def test_refusals_enqueue_nothing():
    from signature_gan_amd import _lib
    size, latent, batch = 64, 100, 2
    eng = objective_engine(size, latent, batch)
    z = torch.from_numpy(I.gen_z(batch, latent, SEED["z"])).cuda()
    pool = torch.zeros(batch * size * size + 4, dtype=torch.float32, device="cuda")
    seed = pool[:batch * size * size]
    t_u8 = torch.zeros(batch, size, size, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def refused(w, g, tu=None, b=batch, rc_want=-1):
        dz, obj = torch.full((batch, latent), 7.0, device="cuda"), torch.full((batch,), 7.0, device="cuda")
        wp = C.byref(_lib.LatentObjective(*w)) if w is not None else None
        rc = eng.lib.siggan_g_latent_objective_grad_seeded(eng._h, p(z), b, p(tu), None, wp, p(g), p(dz), p(obj), None, None, None,
                                                           eng._stream())
        torch.cuda.synchronize()
        assert rc == rc_want, (rc, eng.lib.siggan_last_error())
        assert bool((dz == 7.0).all()) and bool((obj == 7.0).all())        # nothing ran

    refused(ZERO, None)                                                    # a null seed: use the unseeded call
    refused(ZERO, pool[1:1 + batch * size * size])                         # misaligned
    refused((-1.0, 0.0, 0.0), seed)
    refused((0.0, float("nan"), 0.0), seed)
    refused((1.0, 0.0, 0.0), seed)                                         # recon_weight > 0 without a target
    refused(ZERO, seed, tu=t_u8)                                           # a target but recon_weight 0
    refused(None, seed)
    refused(ZERO, seed, b=batch + 1)
    with pytest.raises(ValueError):
        eng.g_latent_objective_grad(z, realism_weight=0.0, image_grad=torch.zeros(batch, 1, 32, 32, device="cuda"))
    with pytest.raises(ValueError):
        eng.g_latent_objective_grad(z, realism_weight=0.0, image_grad=torch.zeros(batch, 1, size, size))     # on the CPU
    with pytest.raises(ValueError):
        eng.g_latent_objective_grad(z, realism_weight=0.0)                  # all weights 0 without a seed: still refused
    eng.step_begin(torch.from_numpy(I.gen_real(batch, size, SEED["real"])).cuda(), z)
    refused(ZERO, seed, rc_want=-2)                                        # between step_begin and its g_grads
    eng.d_apply(); eng.g_compute_grads(batch); eng.g_apply()
    dz, obj = eng.g_latent_objective_grad(z, realism_weight=0.0, image_grad=seed.view(batch, 1, size, size))
    assert bool(torch.isfinite(dz).all()) and not obj.any()                # a zero seed, zero weights: dz = 0 and objective 0
    assert not dz.any()
    eng.close()
