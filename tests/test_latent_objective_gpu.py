"""siggan_g_latent_objective_grad (Engine.g_latent_objective_grad): the gradient with respect to z of
w_r * mean((G(z) - t)^2) + w_d * -max(log D(G(z)), -100) + w_p * 0.5 * mean(z^2) through the eval-mode Generator and the eval-mode
Discriminator.

The gradient is held to the oracle in fp64 on the device's own sign decisions in BOTH networks (the README parity contract's
"HIP = oracle(HIP's decisions)", 1e-4 of max|dz_ref|), the decisions to the fp64 run's own wherever that run is not
borderline, the terms to fp64 on the device's own probabilities / z, the bit contracts of include/siggan.h one by one.  Cases:
those of test_latent_grad_gpu plus one on a spectral-norm context; the state is the cold synthetic one with that test's final-conv
gain, where no prediction saturates (the test asserts |logit| < 6 on the device); the spectral-norm case runs on u, v after eight
power iterations (objectivecommon.objective_engine says why), read back from the context for the oracle."""
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch

from common import I, SEED
from latentcommon import oracle_sd64
from objectivecommon import (CASES, GAIN, WEIGHTS, combine, hip_signs_d_rows, lut_f32, objective_engine, oracle_d_sd64,
                             oracle_objective)

pytestmark = pytest.mark.gpu
ALL3 = WEIGHTS[1]


def compute_case(case, z_seed=None, extra=None):
    """Everything the tests of one case compare, computed once and brought to the CPU (also what
    profiles/latent_objective_parity_margins.py records).  ``z_seed``: the seed of z (default SEED["z"]; the targets are the
    bytes of G at SEED["z"] + 1 either way).  ``extra(eng, out, zc, t_u8)``: further calls on the same engine, after the ones
    here, adding to ``out`` (test_eval_grad_batches_gpu.py)."""
    from hipcommon import hip_signs_g
    size, latent, batch, slope, sn = case
    eng = objective_engine(size, latent, batch, slope, sn)
    z = torch.from_numpy(I.gen_z(batch, latent, SEED["z"] if z_seed is None else z_seed))
    zc = z.cuda()
    t_u8 = eng.g_generate_u8(torch.from_numpy(I.gen_z(batch, latent, SEED["z"] + 1)).cuda())
    t_f32 = lut_f32(t_u8)
    cpu = lambda ts: tuple(t.cpu() for t in ts)
    out = {"case": case, "z": z, "t64": t_f32[:, 0].double()}
    uv = {k: v.cpu().clone() for k, v in eng.sn_views().items()} if sn else None
    out["want_img"] = eng.g_forward(zc, training=False).cpu()
    out["latent_grad"] = cpu(eng.g_latent_grad(zc, t_u8, want_images=True))                   # dz, loss, images
    frozen = lambda: {**{k: v.clone() for k, v in eng.bn_views().items()}, **({k: v.clone() for k, v in eng.sn_views().items()} if sn else {})}
    before = frozen()
    for w in WEIGHTS:
        out[w] = cpu(eng.g_latent_objective_grad(zc, t_u8 if w[0] else None, *w, want_terms=True, want_probs=w[1] > 0, want_images=True))
        if w == ALL3:
            out["signs_g"], out["signs_d"] = hip_signs_g(eng, size, batch), hip_signs_d_rows(eng, size, batch)
            out["f32"] = cpu(eng.g_latent_objective_grad(zc, t_f32.cuda(), *w, want_terms=True, want_probs=True, want_images=True))
            out["again"] = cpu(eng.g_latent_objective_grad(zc, t_u8, *w, want_terms=True, want_probs=True, want_images=True))
    after = frozen()
    out["frozen"] = [(k, torch.equal(before[k], after[k])) for k in before]
    out["d_forward"] = eng.d_forward(out[ALL3][4].cuda(), training=False).cpu().reshape(-1)
    if extra is not None:
        extra(eng, out, zc, t_u8)
    eng.close()
    rec_g, rec_d = [], []
    t0 = time.perf_counter()
    out["terms_ref"], out["grads_ref"], out["logit_ref"] = oracle_objective(
        oracle_sd64(size, latent, GAIN[size]), oracle_d_sd64(size, uv), z, out["t64"], size, out["signs_g"], out["signs_d"], slope,
        rec_g, rec_d)
    out["oracle_seconds"] = time.perf_counter() - t0
    out["rec_g"], out["rec_d"] = rec_g, rec_d
    return out


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"s{c[0]}-z{c[1]}-b{c[2]}-slope{c[3]:g}{'-sn' if c[4] else ''}")
def run(request):
    return compute_case(request.param)


def grad_margins(run):
    """{weights: (max|dz - dz_ref| / max|dz_ref|, max|dz_ref|)}"""
    out = {}
    for w in WEIGHTS:
        ref = combine(w, run["grads_ref"])
        out[w] = (float((run[w][0].double() - ref).abs().max()) / float(ref.abs().max()), float(ref.abs().max()))
    return out


def test_gradient_is_the_oracles_on_the_devices_decisions(run):
    m = grad_margins(run)
    for w, (err, scale) in m.items():
        print(f"{run['case']} {w}: max|dz - dz_ref| / max|dz_ref| = {err:.3e}  (max|dz_ref| {scale:.3e})")
    p = run[ALL3][3].double()
    logit = torch.log(p) - torch.log1p(-p)
    print(f"{run['case']}: device logits {logit.numpy()}, oracle {run['logit_ref'].numpy()}")
    assert float(logit.abs().max()) < 6.0                # no prediction saturates: the realism gradient is not vacuous
    for w, (err, scale) in m.items():
        assert scale > 0 and err <= 1e-4, (w, err)


def test_decisions_differ_only_where_fp64_is_borderline(run):
    from hipcommon import count_sign_flips
    for net in ("g", "d"):
        n = count_sign_flips(run["signs_" + net], run["rec_" + net])
        print(f"{run['case']} {net}: {n} borderline decisions of {sum(x.numel() for x in run['rec_' + net])}")


def test_reconstruction_alone_is_g_latent_grad_bit_for_bit(run):
    dz, obj, terms, img = run[(1.0, 0.0, 0.0)]
    want_dz, want_loss, want_img = run["latent_grad"]
    assert torch.equal(dz, want_dz) and torch.equal(obj, want_loss) and torch.equal(img, want_img)
    assert torch.equal(terms[0], want_loss) and not terms[1:].any()


def test_images_and_probabilities_are_the_forward_passes(run):
    for w in WEIGHTS:
        assert torch.equal(run[w][-1], run["want_img"]), w
    assert torch.equal(run[ALL3][3], run["d_forward"])
    assert torch.equal(run[WEIGHTS[0]][3], run["d_forward"])          # (the images are the same, so are the scores)


def test_byte_and_fp32_targets_give_the_same_bits(run):
    for a, b in zip(run[ALL3], run["f32"]):
        assert torch.equal(a, b)


def test_two_calls_give_the_same_bits(run):
    for a, b in zip(run[ALL3], run["again"]):
        assert torch.equal(a, b)


def test_batchnorm_buffers_and_u_v_do_not_move(run):
    assert run["frozen"] and all(same for _, same in run["frozen"]), run["frozen"]


def term_margins(run):
    """{weights: (realism, prior, objective relative errors)} against fp64 on the device's own probabilities, z and terms."""
    out = {}
    for w in WEIGHTS:
        terms, obj = run[w][2].double().numpy(), run[w][1].double().numpy()
        rel = lambda got, want: float(np.max(np.abs(got - want) / np.abs(want)))
        e_real = rel(terms[1], -np.log(run[w][3].double().numpy())) if w[1] else 0.0
        e_prior = rel(terms[2], 0.5 * (run["z"].double().numpy() ** 2).mean(axis=1)) if w[2] else 0.0
        out[w] = (e_real, e_prior, rel(obj, combine(w, terms)))
    return out


def test_terms(run):
    latent = run["case"][1]
    want_loss = run["latent_grad"][1]
    for w, (e_real, e_prior, e_obj) in term_margins(run).items():
        terms = run[w][2]
        print(f"{run['case']} {w}: terms {terms.numpy().tolist()}  rel err realism {e_real:.2e} prior {e_prior:.2e} objective {e_obj:.2e}")
        assert tuple(terms.shape) == (3, run["case"][2])
        if w[0]:
            assert torch.equal(terms[0], want_loss)                   # the recon term: g_latent_grad's loss bits
        for i in range(3):
            assert w[i] or not terms[i].any()                         # a term whose weight is 0 is written as 0
        assert e_real <= 2.0 ** -22 and e_prior <= latent * 2.0 ** -24 and e_obj <= 2.0 ** -22, (w, e_real, e_prior, e_obj)
    # (the fp64 oracle's terms differ by its images' / logits' ~1e-6 only: the two references agree)
    assert np.allclose(run[ALL3][2].double().numpy(), run["terms_ref"].numpy(), rtol=1e-3)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_training_state_is_untouched(graph):
    """train_step; g_latent_objective_grad with all three weights; train_step leaves exactly what two train_steps leave."""
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
            eng.g_latent_objective_grad(zs[4], t_u8, *ALL3, want_terms=True, want_probs=True)
        eng.train_step(real[1], zs[2], None, zs[3])
        torch.cuda.synchronize()
        states.append(full_state(eng))
        eng.close()
    assert_same_state(states[0], states[1], "a training step after g_latent_objective_grad")


def _raw_call(eng, z, t_u8, t_f32, w, dz, obj, batch, terms=None, probs=None, img=None):
    from signature_gan_amd import _lib
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    wp = C.byref(_lib.LatentObjective(*w)) if w is not None else None
    return eng.lib.siggan_g_latent_objective_grad(eng._h, p(z), batch, p(t_u8), p(t_f32), wp, p(dz), p(obj), p(terms), p(probs), p(img),
                                                  eng._stream())


def test_refusals_enqueue_nothing():
    from signature_gan_amd import _lib
    size, latent, batch = 64, 100, 2
    z = torch.from_numpy(I.gen_z(4, latent, SEED["z"])).cuda()
    t_u8 = torch.zeros(4, size, size, dtype=torch.uint8, device="cuda")
    t_f32 = torch.zeros(4, 1, size, size, dtype=torch.float32, device="cuda")
    pool = torch.zeros(4 * size * size + 4, dtype=torch.float32, device="cuda")

    def refused(eng, z_, tu, tf, w, b, want_probs=False, img=None, rc_want=-1):
        dz = torch.full((4, latent), 7.0, device="cuda")
        obj = torch.full((4,), 7.0, device="cuda")
        terms = torch.full((3, 4), 7.0, device="cuda")
        probs = torch.full((4,), 7.0, device="cuda")
        rc = _raw_call(eng, z_, tu, tf, w, dz, obj, b, terms, probs if want_probs else None, img)
        torch.cuda.synchronize()
        assert rc == rc_want, (rc, eng.lib.siggan_last_error())
        if rc == -1:
            with pytest.raises(ValueError):
                _lib.check(rc)
        for t in (dz, obj, terms, probs):
            assert bool((t == 7.0).all())                                  # nothing ran

    eng = objective_engine(size, latent, batch)
    for w in ((-1.0, 1.0, 0.0), (0.0, -0.5, 0.0), (0.0, 1.0, -1.0), (math.nan, 1.0, 0.0), (0.0, math.inf, 0.0), (0.0, 1.0, math.nan)):
        refused(eng, z, t_u8 if w[0] > 0 else None, None, w, batch)        # a negative or non-finite weight
    refused(eng, z, None, None, (0.0, 0.0, 0.0), batch)                    # all three weights 0
    refused(eng, z, None, None, (1.0, 1.0, 0.0), batch)                    # recon_weight > 0 without a target
    refused(eng, z, t_u8, t_f32, (1.0, 1.0, 0.0), batch)                   # ... with both
    refused(eng, z, t_u8, None, (0.0, 1.0, 0.0), batch)                    # recon_weight == 0 with a target
    refused(eng, z, None, t_f32, (0.0, 1.0, 0.5), batch)
    refused(eng, z, t_u8, None, (1.0, 0.0, 0.0), batch, want_probs=True)   # probs without the realism term
    refused(eng, z, None, None, (0.0, 0.0, 1.0), batch, want_probs=True)
    u8_pool = torch.zeros(4 * size * size + 4, dtype=torch.uint8, device="cuda")
    refused(eng, z, u8_pool[1:1 + batch * size * size], None, (1.0, 1.0, 0.0), batch)          # the alignment rules of g_latent_grad
    refused(eng, z, None, pool[1:1 + batch * size * size], (1.0, 1.0, 0.0), batch)
    refused(eng, z, None, None, (0.0, 1.0, 0.0), batch, img=pool[1:1 + batch * size * size])
    refused(eng, z, None, None, (0.0, 1.0, 0.0), batch + 1)                # beyond the context's maximum
    refused(eng, z, None, None, (0.0, 1.0, 0.0), 0)
    refused(eng, z, None, None, None, batch)                               # null weights
    ok = torch.empty(4, latent, device="cuda")
    assert _raw_call(eng, z, None, None, (0.0, 1.0, 0.0), None, torch.empty(4, device="cuda"), batch) == -1     # null dz
    assert _raw_call(eng, z, None, None, (0.0, 1.0, 0.0), ok, None, batch) == -1
    assert _raw_call(eng, None, None, None, (0.0, 1.0, 0.0), ok, torch.empty(4, device="cuda"), batch) == -1
    with pytest.raises(ValueError):
        eng.g_latent_objective_grad(z[:batch], t_u8[:batch].float(), recon_weight=1.0)          # fp32 targets are (B, 1, S, S)
    with pytest.raises(ValueError):
        eng.g_latent_objective_grad(z[:batch, :50])
    with pytest.raises(ValueError):
        eng.g_latent_objective_grad(z[:batch], realism_weight=0.0, prior_weight=1.0, want_probs=True)
    # between siggan_step_begin and its siggan_g_grads: SIGGAN_E_STATE
    eng.step_begin(torch.from_numpy(I.gen_real(batch, size, SEED["real"])).cuda(), z[:batch])
    refused(eng, z, None, None, (0.0, 1.0, 0.0), batch, rc_want=-2)
    eng.d_apply(); eng.g_compute_grads(batch); eng.g_apply()               # ... and accepted again once the step is complete
    assert bool(torch.isfinite(eng.g_latent_objective_grad(z[:batch])[0]).all())
    eng.close()
    eng = objective_engine(size, latent, batch)                            # the context works after refusals
    refused(eng, z, None, None, (0.0, 0.0, 0.0), batch)
    dz, obj, probs = eng.g_latent_objective_grad(z[:batch], want_probs=True)
    assert bool(torch.isfinite(dz).all()) and bool((obj > 0).all()) and bool(((probs > 0) & (probs < 1)).all())
    dz_p, obj_p, terms_p = eng.g_latent_objective_grad(z[:batch], realism_weight=0.0, prior_weight=2.0, want_terms=True)   # the prior alone
    assert torch.allclose(dz_p, 2.0 * z[:batch] / latent, rtol=1e-6, atol=0) and torch.allclose(obj_p, 2.0 * terms_p[2], rtol=1e-6)
    eng.close()
    eng16 = objective_engine(size, latent, batch, dtype="bf16")
    refused(eng16, z, None, None, (0.0, 1.0, 0.0), batch)                  # a 16-bit context
    with pytest.raises(ValueError):
        eng16.g_latent_objective_grad(z[:batch])
    eng16.close()
