"""siggan_g_param_grad (Engine.g_param_grad): the gradient with respect to the Generator's PARAMETERS of
w_r * mean((G(z) - t)^2) + w_d * -max(log D(G(z)), -100), summed over the batch, through the eval-mode Generator (BatchNorm =
the affine of its running statistics) and the eval-mode Discriminator; and siggan_op_anchor.

Every parameter tensor is held to the oracle in fp64 on the device's own sign decisions in both networks, per tensor:
max|d - ref| <= 1e-4 * max|ref| -- the project's gradient bound, applied per tensor as the README's contract does (torch fp32
against fp64 on shared decisions and targets deviates at most 3.9e-6 of a tensor's max over these cases, and no tensor's max|ref|
is below 3e-4, so the bound is neither vacuous nor within rounding).  Cases, final-conv gain and targets: those of
test_latent_grad_gpu / test_latent_objective_gpu -- the smallest shapes that reach ragged GEMM rows, one sample, five blocks, the
generic fc path and LeakyReLU -- plus the spectral-norm Discriminator for the realism term alone, plus the batches adapt_generator
runs, 9 and 64 images (PARAM_BATCH_CASES; worst tensor there 7.5e-6 and 5.5e-6, no tensor's max|ref| below 1.5e-3)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from adaptcommon import BOUND, PARAM_WEIGHTS, combine, n_blocks, oracle_param_grads, param_keys, split_arena, tensor_margins
from common import I, SEED
from latentcommon import oracle_sd64
from objectivecommon import BATCH_CASES, CASES, GAIN, hip_signs_d_rows, lut_f32, objective_engine, oracle_d_sd64

pytestmark = pytest.mark.gpu
BOTH = PARAM_WEIGHTS[2]
# the gamma-edge entries.  Block 2's zeroed channel is 8, the one whose synthetic beta is largest (+0.219): with gamma = 0 the
# pre-activation IS beta, so a channel with beta <= 0 is dead under ReLU and its dgamma is 0 whatever the kernel does
EDGE = {"upsample_blocks.1.block.1.weight": dict(zero=8, negate=7), "fc.1.weight": dict(zero=11)}
EDGE_BIAS = ("fc.1.bias", 11, 0.1)                      # ... and the bias that keeps the zeroed fc feature active under ReLU


def apply_edge(sd, scale=None):
    """Zero / negate the EDGE entries of a state dict of tensors (views of an engine's arena, or the oracle's) in place."""
    for k, e in EDGE.items():
        sd[k][e["zero"]] = 0.0
        if "negate" in e:
            sd[k][e["negate"]] = -sd[k][e["negate"]]
    sd[EDGE_BIAS[0]][EDGE_BIAS[1]] = EDGE_BIAS[2]


def compute_case(case, edge=False, weights=None):
    """Everything the tests of one case compare, computed once and brought to the CPU (also what
    profiles/param_grad_parity_margins.py records)."""
    from hipcommon import hip_signs_g
    size, latent, batch, slope, sn = case
    weights = weights or ([PARAM_WEIGHTS[1]] if sn else PARAM_WEIGHTS)
    eng = objective_engine(size, latent, batch, slope, sn)
    g64 = oracle_sd64(size, latent, GAIN[size])
    if edge:
        apply_edge(eng.views("g")); eng.params_changed()
        apply_edge(g64)
    z = torch.from_numpy(I.gen_z(batch, latent, SEED["z"]))
    zc = z.cuda()
    t_u8 = eng.g_generate_u8(torch.from_numpy(I.gen_z(batch, latent, SEED["z"] + 1)).cuda())
    t_f32 = lut_f32(t_u8)
    out = {"case": case, "z": z, "t64": t_f32[:, 0].double(), "weights": weights, "keys": param_keys(latent, size)}
    uv = {k: v.cpu().clone() for k, v in eng.sn_views().items()} if sn else None
    out["want_img"] = eng.g_forward(zc, training=False).cpu()
    frozen = lambda: {**{k: v.clone() for k, v in eng.bn_views().items()}, **({k: v.clone() for k, v in eng.sn_views().items()} if sn else {}),
                      "g_params": eng.g_params.clone(), "g_grads": eng.g_grads.clone()}
    before = frozen()

    def call(w, target):
        res = eng.g_param_grad(zc, target if w[0] else None, w[0], w[1], want_terms=True, want_probs=w[1] > 0, want_images=True)
        return {"dparams": split_arena(eng, res[0]), "flat": res[0].cpu(), "objective": res[1].cpu(), "terms": res[2].cpu(),
                "probs": res[3].cpu() if w[1] > 0 else None, "images": res[-1].cpu()}

    for w in weights:
        out[w] = call(w, t_u8)
        lo = eng.g_latent_objective_grad(zc, t_u8 if w[0] else None, w[0], w[1], 0.0, want_terms=True, want_probs=w[1] > 0, want_images=True)
        out[("latent", w)] = tuple(t.cpu() for t in lo)
    last = weights[-1]
    out["again"] = call(last, t_u8)
    out["signs_g"] = hip_signs_g(eng, size, batch)
    out["signs_d"] = hip_signs_d_rows(eng, size, batch) if last[1] > 0 else None
    if last[0] > 0:
        out["f32"] = call(last, t_f32.cuda())
    after = frozen()
    out["frozen"] = [(k, torch.equal(before[k], after[k])) for k in before]
    eng.close()
    need_d = any(w[1] > 0 for w in weights)
    rec_g, rec_d = [], []
    out["g_recon"], out["g_real"], out["terms_ref"], out["logit_ref"] = oracle_param_grads(
        g64, oracle_d_sd64(size, uv) if need_d else None, z, out["t64"], size, latent, out["signs_g"], out["signs_d"], slope, rec_g, rec_d)
    out["rec_g"], out["rec_d"] = rec_g, rec_d
    return out


def margins(run):
    """{weights: {key: (max|d - ref| / max|ref|, max|ref|)}}"""
    return {w: tensor_margins(run[w]["dparams"], combine(w, run["g_recon"], run["g_real"])) for w in run["weights"]}


def check_bound(run):
    worst = 0.0
    for w, m in margins(run).items():
        for k, (err, scale) in m.items():
            print(f"{run['case']} {w} {k}: max|d - ref| / max|ref| = {err:.3e}  (max|ref| {scale:.3e})")
            worst = max(worst, err)
    for w, m in margins(run).items():
        for k, (err, scale) in m.items():
            assert scale > 0, (w, k)
            assert err <= BOUND, (w, k, err)
    return worst


# ... and the batches adapt_generator runs (chunks of max_batch, 64 by default): 9 images -- k_bn_eval_bwd on block 1 in two
# chunks, the second 64 rows, every input-gradient GEMM still slab-split with other counts than at 3 -- and 64, where the
# table-free EPI_LRELU_BWD runs inside k_gconv<128,32> (l = 4, 512 workgroups) and the two-quad k_gconv<64,64> (l = 3), and
# k_part_sum's lanes add up to 16 chunks each (512 chunks in block 4).  evalpaths restates the launchers; the GEMMs are pinned
# through the profile by test_the_batch_cases_make_their_launches.
PARAM_BATCH_CASES = [c for c, _ in BATCH_CASES if c[:3] in ((64, 100, 9), (64, 100, 64))]


@pytest.fixture(scope="module", params=CASES + PARAM_BATCH_CASES,
                ids=lambda c: f"s{c[0]}-z{c[1]}-b{c[2]}-slope{c[3]:g}{'-sn' if c[4] else ''}")
def run(request):
    return compute_case(request.param)


def test_every_tensor_is_the_oracles_on_the_devices_decisions(run):
    check_bound(run)
    if run["weights"][-1][1] > 0:
        p = run[run["weights"][-1]]["probs"].double()
        assert float((torch.log(p) - torch.log1p(-p)).abs().max()) < 6.0          # no prediction saturates: the realism gradient is not vacuous


def test_decisions_differ_only_where_fp64_is_borderline(run):
    from hipcommon import count_sign_flips
    for net in ("g", "d"):
        if run["signs_" + net] is not None:
            n = count_sign_flips(run["signs_" + net], run["rec_" + net])
            print(f"{run['case']} {net}: {n} borderline decisions of {sum(x.numel() for x in run['rec_' + net])}")


def test_objective_terms_probs_and_images(run):
    """Against siggan_g_latent_objective_grad at the same inputs: the forward here keeps the pre-BatchNorm tensors (raw GEMM, then
    the affine as a launch of its own) -- where its images are the folded forward's bits, so is everything derived from them;
    otherwise the images are within the README's 1e-3 and the difference is printed.  The loss is held to numpy fp64 on the
    call's own images."""
    size = run["case"][0]
    for w in run["weights"]:
        got, lat = run[w], run[("latent", w)]
        img = got["images"]
        diff = float((img - run["want_img"]).abs().max())
        same = torch.equal(img, run["want_img"])
        print(f"{run['case']} {w}: images vs g_forward max|diff| {diff:.3e} (bit-equal: {same})")
        assert diff <= 1e-3 * float(run["want_img"].abs().max())
        assert tuple(got["terms"].shape) == (3, run["case"][2]) and not got["terms"][2].any()       # the prior row is 0
        if same:
            assert torch.equal(got["objective"], lat[1]) and torch.equal(got["terms"], lat[2])
            if w[1] > 0:
                assert torch.equal(got["probs"], lat[3])
        else:
            assert torch.allclose(got["objective"], lat[1], rtol=1e-3) and torch.allclose(got["terms"], lat[2], rtol=1e-3, atol=1e-6)
        if w[0] > 0:
            want = ((img[:, 0].double().numpy() - run["t64"].numpy()) ** 2).mean(axis=(1, 2))
            rel = float(np.max(np.abs(got["terms"][0].double().numpy() - want) / want))
            print(f"{run['case']} {w}: loss rel err against fp64 on the call's own images {rel:.2e}")
            assert rel <= size * size * 2.0 ** -24
        else:
            assert not got["terms"][0].any()
        if w[1] > 0:
            want = -np.log(got["probs"].double().numpy())
            assert float(np.max(np.abs(got["terms"][1].double().numpy() - want) / want)) <= 2.0 ** -22
        obj = w[0] * got["terms"][0].double() + w[1] * got["terms"][1].double()
        assert float(((got["objective"].double() - obj).abs() / obj.abs()).max()) <= 2.0 ** -22


def test_byte_and_fp32_targets_give_the_same_bits(run):
    if "f32" not in run:
        assert run["weights"] == [PARAM_WEIGHTS[1]]         # (the spectral-norm case runs the realism term alone: no target to compare)
        return
    a, b = run[run["weights"][-1]], run["f32"]
    assert torch.equal(a["flat"], b["flat"]) and torch.equal(a["objective"], b["objective"]) and torch.equal(a["images"], b["images"])


def test_two_calls_give_the_same_bits(run):
    a, b = run[run["weights"][-1]], run["again"]
    assert torch.equal(a["flat"], b["flat"]) and torch.equal(a["objective"], b["objective"]) and torch.equal(a["terms"], b["terms"])


def test_parameters_gradient_arena_batchnorm_buffers_and_u_v_do_not_move(run):
    assert run["frozen"] and all(same for _, same in run["frozen"]), run["frozen"]


def test_gamma_of_zero_and_of_negative_sign():
    """One BatchNorm channel of block 2 with gamma exactly 0 and one negated; one fc feature with gamma 0 and beta 0.1 (active
    under ReLU): dgamma there does not vanish (the oracle's is at least 1 % of its tensor's largest) and the bound holds."""
    run = compute_case(CASES[0], edge=True, weights=[PARAM_WEIGHTS[0], BOTH])
    for w in run["weights"]:
        ref = combine(w, run["g_recon"], run["g_real"])
        for k, e in EDGE.items():
            frac = abs(float(ref[k][e["zero"]])) / float(ref[k].abs().max())
            print(f"{w} {k}[{e['zero']}] (gamma = 0): oracle dgamma {float(ref[k][e['zero']]):.3e} = {frac:.1%} of the tensor's max, "
                  f"device {float(run[w]['dparams'][k][e['zero']]):.3e}")
            assert frac >= 0.01
    check_bound(run)


def expected_gemms(size, first_layer, with_d):
    lg = n_blocks(size)
    nb = lg - max(first_layer, 1) + 1 if first_layer <= lg else 0
    nd = lg - first_layer if first_layer <= lg else 0
    return lg + nb + nd + (2 * (lg - 1) if with_d else 0)          # (Ld == Lg at both sizes)


def test_first_layer_freezes_a_prefix_and_shortens_the_chain():
    size, latent, batch = 64, 100, 2
    eng = objective_engine(size, latent, batch)
    lg = eng.g_layers
    zc = torch.from_numpy(I.gen_z(batch, latent, SEED["z"])).cuda()
    t_u8 = eng.g_generate_u8(torch.from_numpy(I.gen_z(batch, latent, SEED["z"] + 1)).cuda())
    full = {w: eng.g_param_grad(zc, t_u8 if w[0] else None, w[0], w[1])[0].clone() for w in (PARAM_WEIGHTS[0], BOTH)}
    assert all(bool(v.any()) for v in full.values())
    counts = []
    for fl in range(lg + 2):
        off, num = eng.layer_span(fl)
        assert off + num == eng.g_params.numel()
        for w, want in full.items():
            d = torch.full_like(eng.g_params, 7.0)
            eng.g_param_grad(zc, t_u8 if w[0] else None, w[0], w[1], first_layer=fl, dparams_out=d)
            assert torch.equal(d[off:], want[off:]), (fl, w)                                    # trainable spans: the full call's bits
            assert not d[:off].any(), (fl, w)                                                   # frozen spans: exactly 0
        eng.prof_enable(True)
        eng.g_param_grad(zc, t_u8, 1.0, 0.0, first_layer=fl)
        n = len(eng.prof_launches())
        eng.prof_enable(False)
        counts.append(n)
        assert n == expected_gemms(size, fl, False), (fl, n)
    print(f"implicit-GEMM + weight-gradient launches by first_layer: {counts}")
    assert counts == sorted(counts, reverse=True) and counts[-1] == lg                          # Lg + 1: the forward's GEMMs only
    eng.prof_enable(True)
    eng.g_param_grad(zc, t_u8, *BOTH)
    assert len(eng.prof_launches()) == expected_gemms(size, 0, True)
    eng.prof_enable(False)
    eng.close()


@pytest.mark.parametrize("case", PARAM_BATCH_CASES, ids=lambda c: f"b{c[2]}")
def test_the_batch_cases_make_their_launches(case):
    """One g_param_grad with both weights on an engine of its own makes the input-gradient GEMMs evalpaths restates for the
    batch -- tile, rows, channels, slab count, in-workgroup split; test_eval_paths_cpu.py writes them out per case -- in both
    chains, and as many GEMM and weight-gradient launches as expected_gemms counts."""
    import evalpaths
    size, latent, batch, slope, sn = case
    eng = objective_engine(size, latent, batch, slope, sn)
    zc = torch.from_numpy(I.gen_z(batch, latent, SEED["z"])).cuda()
    t_u8 = eng.g_generate_u8(torch.from_numpy(I.gen_z(batch, latent, SEED["z"] + 1)).cuda())
    eng.prof_enable(True)
    try:
        eng.g_param_grad(zc, t_u8, *BOTH)
        torch.cuda.synchronize()
        launches = eng.prof_launches()
    finally:
        eng.prof_enable(False)
        eng.close()
    keys = ("kernel", "form", "epi", "M", "Ci", "Co", "slabs", "kq")
    for want in evalpaths.g_chain(size, batch) + evalpaths.d_chain(size, batch):
        assert [l for l in launches if all(l[k] == want[k] for k in keys)], (want, [{k: l[k] for k in keys} for l in launches if l["M"] >= 0])
    assert len(launches) == expected_gemms(size, 0, True)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_training_state_is_untouched(graph):
    """train_step; g_param_grad with both weights; train_step leaves exactly what two train_steps leave."""
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
            bn = {k: v.clone() for k, v in eng.bn_views().items()}
            d = eng.g_param_grad(zs[4], t_u8, *BOTH, want_terms=True, want_probs=True)[0]
            assert bool(torch.isfinite(d).all()) and bool(d.any())
            assert all(torch.equal(v, eng.bn_views()[k]) for k, v in bn.items())              # running tensors and counters
        eng.train_step(real[1], zs[2], None, zs[3])
        torch.cuda.synchronize()
        states.append(full_state(eng))
        eng.close()
    assert_same_state(states[0], states[1], "a training step after g_param_grad")


def _raw_call(eng, z, t_u8, t_f32, w, fl, d, obj, batch, terms=None, probs=None, img=None):
    from signature_gan_amd import _lib
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    wp = C.byref(_lib.LatentObjective(*w)) if w is not None else None
    return eng.lib.siggan_g_param_grad(eng._h, p(z), batch, p(t_u8), p(t_f32), wp, fl, p(d), p(obj), p(terms), p(probs), p(img),
                                       eng._stream())


def test_refusals_enqueue_nothing():
    from signature_gan_amd import _lib
    size, latent, batch = 64, 100, 2
    z = torch.from_numpy(I.gen_z(4, latent, SEED["z"])).cuda()
    t_u8 = torch.zeros(4, size, size, dtype=torch.uint8, device="cuda")
    t_f32 = torch.zeros(4, 1, size, size, dtype=torch.float32, device="cuda")

    def refused(eng, tu, tf, w, b, fl=0, want_probs=False, null_d=False, rc_want=-1, shift=0):
        d = torch.full((eng.g_params.numel() + 4,), 7.0, device="cuda")
        obj = torch.full((4,), 7.0, device="cuda")
        terms = torch.full((3, 4), 7.0, device="cuda")
        probs = torch.full((4,), 7.0, device="cuda")
        rc = _raw_call(eng, z, tu, tf, w, fl, None if null_d else d[shift:], obj, b, terms, probs if want_probs else None)
        torch.cuda.synchronize()
        assert rc == rc_want, (rc, eng.lib.siggan_last_error())
        if rc == -1:
            with pytest.raises(ValueError):
                _lib.check(rc)
        for t in (d, obj, terms, probs):
            assert bool((t == 7.0).all())                                  # nothing ran

    eng = objective_engine(size, latent, batch)
    lg = eng.g_layers
    refused(eng, t_u8, None, (1.0, 0.0, 0.5), batch)                       # the prior does not depend on the parameters
    refused(eng, None, None, (0.0, 1.0, 1.0), batch)
    for w in ((-1.0, 1.0, 0.0), (0.0, -0.5, 0.0), (math.nan, 1.0, 0.0), (0.0, math.inf, 0.0)):
        refused(eng, t_u8 if w[0] > 0 else None, None, w, batch)           # a negative or non-finite weight
    refused(eng, None, None, (0.0, 0.0, 0.0), batch)                       # both weights 0
    refused(eng, None, None, (1.0, 1.0, 0.0), batch)                       # recon_weight > 0 without a target
    refused(eng, t_u8, t_f32, (1.0, 1.0, 0.0), batch)                      # ... with both
    refused(eng, t_u8, None, (0.0, 1.0, 0.0), batch)                       # recon_weight == 0 with a target
    refused(eng, t_u8, None, (1.0, 0.0, 0.0), batch, want_probs=True)      # probs without the realism term
    refused(eng, t_u8, None, (1.0, 0.0, 0.0), batch, fl=-1)                # first_layer out of range
    refused(eng, t_u8, None, (1.0, 0.0, 0.0), batch, fl=lg + 2)
    refused(eng, t_u8, None, (1.0, 0.0, 0.0), batch, null_d=True)          # null dparams
    refused(eng, t_u8, None, (1.0, 0.0, 0.0), batch, shift=1)              # ... misaligned
    refused(eng, t_u8, None, (1.0, 0.0, 0.0), batch + 1)                   # beyond the context's maximum
    refused(eng, t_u8, None, None, batch)                                  # null weights
    for bad in (dict(first_layer=lg + 2), dict(first_layer=-1), dict(recon_weight=0.0), dict(want_probs=True)):
        with pytest.raises(ValueError):
            eng.g_param_grad(z[:batch], t_u8[:batch], **bad)
    # between siggan_step_begin and its siggan_g_grads: SIGGAN_E_STATE
    eng.step_begin(torch.from_numpy(I.gen_real(batch, size, SEED["real"])).cuda(), z[:batch])
    refused(eng, t_u8, None, (1.0, 0.0, 0.0), batch, rc_want=-2)
    eng.d_apply(); eng.g_compute_grads(batch); eng.g_apply()               # ... and accepted again once the step is complete
    assert bool(torch.isfinite(eng.g_param_grad(z[:batch], t_u8[:batch])[0]).all())
    eng.close()
    eng16 = objective_engine(size, latent, batch, dtype="bf16")
    refused(eng16, t_u8, None, (1.0, 0.0, 0.0), batch)                     # a 16-bit context
    with pytest.raises(ValueError):
        eng16.g_param_grad(z[:batch], t_u8[:batch])
    eng16.close()


@pytest.mark.parametrize("n", [1, 5, 4099])
@pytest.mark.parametrize("weight", [0.0, 0.3])
def test_op_anchor_is_numpys_float32_expression(n, weight):
    from hipcommon import make_engine
    eng = make_engine(64, 100, 2)
    rng = np.random.default_rng(n)
    g, p, p0 = (rng.standard_normal(n + 1).astype(np.float32) for _ in range(3))
    for shift in (0, 1):                                                   # float4 path, and the one-element path of a misaligned view
        gd, pd, qd = (torch.from_numpy(a).cuda()[shift:shift + n] for a in (g, p, p0))
        want = g[shift:shift + n] + np.float32(weight) * (p[shift:shift + n] - p0[shift:shift + n])
        eng.op_anchor(gd, pd, qd, weight)
        assert np.array_equal(gd.cpu().numpy(), want), (n, weight, shift)
    for bad in (-1.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            eng.op_anchor(gd, pd, qd, bad)
    eng.close()
