"""The eval-mode gradient calls at the batches their callers run: siggan_g_latent_grad, siggan_g_latent_objective_grad and its
seeded form on objectivecommon.BATCH_CASES (9, 13, 64 and 256 images at 64x64, 64 again at latent 512, 12 at 128x128), where
the parity tests of test_latent_grad_gpu / test_latent_objective_gpu / test_latent_seed_gpu stop at 3.  (siggan_g_param_grad runs its two batch cases
in test_param_grad_gpu.)

Per case, on one engine: dz of all three weight sets and of one seeded call against the fp64 oracle on the device's own decisions
in both networks -- 1e-4 of max|dz_ref| over the batch as before AND per image (max_k|dz - dz_ref| <= 1e-4 max_k|dz_ref| of that
row: row scales differ several-fold inside these batches, and the README's contract holds each image, the B = 1 case already
does); torch's own fp32 on the same decisions and targets runs alongside and its per-row deviation is printed -- a row that misses
while torch fp32 is itself above 1e-4 / 32 there would be an ill-conditioned z, any other miss is a kernel finding; the sign
decisions; the bit contracts of test_latent_objective_gpu rerun through its own test functions; and ROTATION: the same call with
z, targets and seed rolled by one row returns every output rolled by one row, bit for bit -- a roll by one moves every image
across the 4-image (k_obj_fin_tiles), 8-image (k_fc_dz) and GEMM row-tile boundaries, and no per-image sum's order involves the
row index.  One test per case pins the launches the case exists for through the library's launch profile against evalpaths'
restatement of the launchers; one test runs several sizes on one context."""
import time

import pytest
import torch

import evalpaths
import test_latent_objective_gpu as T
from common import I, O, SEED
from latentcommon import oracle_latent_grad, oracle_sd64
from objectivecommon import BATCH_CASES, GAIN, WEIGHTS, combine, objective_engine, oracle_d_sd64, oracle_objective
from test_latent_seed_gpu import make_seed

pytestmark = pytest.mark.gpu
ALL3 = T.ALL3
BOUND = 1e-4                       # the README's gradient contract
ILL = BOUND / 32                   # torch fp32's own deviation above which a row's z counts as ill-conditioned
KW = dict(want_terms=True, want_probs=True, want_images=True)
NAMES = ("dz", "objective", "terms", "probs", "images")
_id = lambda cz: f"s{cz[0][0]}-z{cz[0][1]}-b{cz[0][2]}-slope{cz[0][3]:g}"


def roll(t):
    """An output rolled by one image: terms are (3, B), everything else has the batch first."""
    return t.roll(1, 1) if t.dim() == 2 and t.shape[0] == 3 else t.roll(1, 0)


def compute_case(case, z_seed):
    """test_latent_objective_gpu.compute_case at this z plus, on the same engine, the seeded call with all three weights, the
    rolled calls, and on the CPU the seed's oracle (test_latent_seed_gpu's: J_G^T seed as the reconstruction gradient at the
    fp64 target x64 - (S^2 / 2) seed on the device's decisions) and torch fp32 (also what profiles/eval_grad_batch_margins.py
    records)."""
    size, latent, batch, slope, sn = case
    seed = make_seed(batch, size)

    def extra(eng, out, zc, t_u8):
        cpu = lambda ts: tuple(t.cpu() for t in ts)
        sc = seed.cuda()
        out["seeded"] = cpu(eng.g_latent_objective_grad(zc, t_u8, *ALL3, image_grad=sc, **KW))
        out["rolled"] = cpu(eng.g_latent_objective_grad(zc.roll(1, 0).contiguous(), t_u8.roll(1, 0).contiguous(), *ALL3, **KW))
        out["rolled_seeded"] = cpu(eng.g_latent_objective_grad(zc.roll(1, 0).contiguous(), t_u8.roll(1, 0).contiguous(), *ALL3,
                                                               image_grad=sc.roll(1, 0).contiguous(), **KW))
        out["rolled_latent_grad"] = cpu(eng.g_latent_grad(zc.roll(1, 0).contiguous(), t_u8.roll(1, 0).contiguous(), want_images=True))

    w0 = time.perf_counter()
    run = T.compute_case(case, z_seed, extra)
    run["seed"] = seed
    g64 = oracle_sd64(size, latent, GAIN[size])
    w1 = time.perf_counter()
    with torch.no_grad():
        x64 = O.g_forward(g64, run["z"].double(), False, size, signs=run["signs_g"], slope=slope)[:, 0]
    run["jt_seed_ref"] = oracle_latent_grad(g64, run["z"], x64 - (size * size / 2.0) * seed[:, 0].double(), size, run["signs_g"], slope)[0]
    w2 = time.perf_counter()
    f32 = lambda sd: {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}
    run["grads_f32"] = oracle_objective(f32(g64), f32(oracle_d_sd64(size)), run["z"], run["t64"].float(), size, run["signs_g"],
                                        run["signs_d"], slope, dtype=torch.float32)[1].double()
    run["seconds"] = {"oracle_fp64": run["oracle_seconds"], "seed_oracle_fp64": w2 - w1, "torch_fp32": time.perf_counter() - w2,
                      "fixture": time.perf_counter() - w0}
    print(f"{case}: seconds {run['seconds']}")
    return run


@pytest.fixture(scope="module", params=BATCH_CASES, ids=_id)
def run(request):
    return compute_case(*request.param)


def row_margins(run):
    """{call: dict(batch=max|dz - ref| / max|ref| over the batch, row=the worst per-row ratio, at=its row, torch_f32=torch
    fp32's per-row ratio on that row, torch_f32_worst=its worst over the rows, scale_spread=largest / smallest row scale)}
    for the three weight sets, g_latent_grad and the seeded call."""
    def one(dz, ref, ref32):
        err, scale = (dz.double() - ref).abs().amax(dim=1), ref.abs().amax(dim=1)
        per_row, f32_row = err / scale, (ref32 - ref).abs().amax(dim=1) / scale if ref32 is not None else None
        at = int(per_row.argmax())
        return dict(batch=float(err.max() / scale.max()), row=float(per_row[at]), at=at,
                    torch_f32=float(f32_row[at]) if f32_row is not None else None,
                    torch_f32_worst=float(f32_row.max()) if f32_row is not None else None,
                    scale_spread=float(scale.max() / scale.min()), min_scale=float(scale.min()))
    out = {w: one(run[w][0], combine(w, run["grads_ref"]), combine(w, run["grads_f32"])) for w in WEIGHTS}
    out["latent_grad"] = one(run["latent_grad"][0], run["grads_ref"][0], run["grads_f32"][0])
    out["seeded"] = one(run["seeded"][0], combine(ALL3, run["grads_ref"]) + run["jt_seed_ref"], None)
    return out


def test_gradient_is_the_oracles_batch_wide_and_on_every_row(run):
    m = row_margins(run)
    for call, r in m.items():
        print(f"{run['case']} {call}: batch-wide {r['batch']:.3e}; worst row {r['at']}: {r['row']:.3e} of its own max|dz_ref| "
              f"(torch fp32 there {r['torch_f32']}, worst {r['torch_f32_worst']}); row scales spread {r['scale_spread']:.1f}x, "
              f"smallest {r['min_scale']:.3e}")
    p = run[ALL3][3].double()
    logit = torch.log(p) - torch.log1p(-p)
    print(f"{run['case']}: max|logit| device {float(logit.abs().max()):.3f}, oracle {float(run['logit_ref'].abs().max()):.3f}")
    assert float(logit.abs().max()) < 6.0                # no prediction saturates: the realism gradient is not vacuous
    for call, r in m.items():
        assert r["min_scale"] > 0, call
        assert r["batch"] <= BOUND, (call, r)
        assert r["row"] <= BOUND, (call, r, "ill-conditioned z" if (r["torch_f32"] or 0.0) > ILL else "a kernel finding")


def test_the_bit_contracts_and_terms_of_the_small_batches_hold(run):
    """test_latent_objective_gpu's own checks on this run: the oracle bound batch-wide, the sign decisions, reconstruction alone =
    g_latent_grad, images = g_forward, probabilities = d_forward, byte = fp32 targets, two calls alike, BatchNorm buffers
    untouched, the term bounds."""
    for check in (T.test_gradient_is_the_oracles_on_the_devices_decisions, T.test_decisions_differ_only_where_fp64_is_borderline,
                  T.test_reconstruction_alone_is_g_latent_grad_bit_for_bit, T.test_images_and_probabilities_are_the_forward_passes,
                  T.test_byte_and_fp32_targets_give_the_same_bits, T.test_two_calls_give_the_same_bits,
                  T.test_batchnorm_buffers_and_u_v_do_not_move, T.test_terms):
        check(run)


def test_the_seed_changes_dz_alone(run):
    for name, a, b in zip(NAMES[1:], run["seeded"][1:], run[ALL3][1:]):
        assert torch.equal(a, b), name
    assert not torch.equal(run["seeded"][0], run[ALL3][0])


def test_rolling_the_inputs_by_one_image_rolls_every_output_bit_for_bit(run):
    bad = []
    calls = [("all three", NAMES, run[ALL3], run["rolled"]), ("seeded", NAMES, run["seeded"], run["rolled_seeded"]),
             ("g_latent_grad", ("dz", "loss", "images"), run["latent_grad"], run["rolled_latent_grad"])]
    for call, names, plain, rolled in calls:
        for name, a, b in zip(names, plain, rolled):
            if not torch.equal(roll(a), b):
                d = (roll(a).double() - b.double()).abs()
                rows = d.any(dim=0) if name == "terms" else d.reshape(d.shape[0], -1).any(dim=1)
                bad.append((call, name, f"max|diff| {float(d.max()):.3e}", "rows (after the roll)", rows.nonzero().reshape(-1).tolist()[:16]))
    assert not bad, bad


# ---- the launches each case exists for -----------------------------------------------------------------------------------------
def _profiled(eng, call):
    eng.prof_enable(True)
    try:
        call()
        torch.cuda.synchronize()
        return [l for l in eng.prof_launches() if l["M"] >= 0]
    finally:
        eng.prof_enable(False)


def _assert_launched(launches, want, what):
    keys = ("kernel", "form", "epi", "M", "Ci", "Co", "slabs", "kq")
    for w in want:
        hit = [l for l in launches if all(l[k] == w[k] for k in keys)]
        assert hit, (f"{what}: no launch {({k: w[k] for k in keys})}; the GEMM launches were "
                     f"{[{k: l[k] for k in keys} for l in launches]}")


@pytest.mark.parametrize("case,z_seed", BATCH_CASES, ids=[_id(c) for c in BATCH_CASES])
def test_each_case_makes_the_launches_it_exists_for(case, z_seed):
    """One all-three-weights call on an engine of its own (profiling is process-wide: off again before the next test) makes
    every implicit GEMM evalpaths restates for it -- the Generator's input-gradient chain (form 0, EPI_LRELU_BWD for l >= 2) and
    the Discriminator's (form 1) with tile, rows, channels, slab count and in-workgroup split, as test_eval_paths_cpu.py pins
    them per case -- and nothing the restatement does not know: 2 Lg + 2 Ld - 2 GEMM launches with the two forwards.  The
    profile records implicit GEMMs only: launch_fc_dz's nsplit -- 64, 64, 64, 128, 64 and, halved once, 32 at (64, 512, 64),
    where a k_fc_dz workgroup walks two feature chunks -- and the workgroup counts of k_obj_fin_tiles and k_bn_eval_bwd are
    evalpaths' arithmetic, pinned by the CPU test against the sources, not read back from the device; what holds those kernels
    on the device is the per-row, roll and one-context tests above."""
    size, latent, batch, slope, sn = case
    eng = objective_engine(size, latent, batch, slope, sn)
    try:
        zc = torch.from_numpy(I.gen_z(batch, latent, z_seed)).cuda()
        t_u8 = eng.g_generate_u8(torch.from_numpy(I.gen_z(batch, latent, SEED["z"] + 1)).cuda())
        launches = _profiled(eng, lambda: eng.g_latent_objective_grad(zc, t_u8, *ALL3))
        _assert_launched(launches, evalpaths.g_chain(size, batch) + evalpaths.d_chain(size, batch), f"{case} latent objective")
        lg, ld = len(evalpaths.G_CHAIN[size]) - 1, len(evalpaths.D_CHAIN[size]) - 1
        assert len(launches) == 2 * lg + 2 * (ld - 1), [(l["kernel"], l["form"], l["epi"], l["M"]) for l in launches]
    finally:
        eng.close()


# ---- one context, several sizes ------------------------------------------------------------------------------------------------
def test_one_context_serves_9_then_64_then_9_images():
    """On an engine with max_batch 64: all three weights at B = 9, B = 64 and B = 9 again -- the first and the third results are
    the same bits (nothing of the larger call stays behind in lg_tab, partial or g_da), both are a max_batch-9 engine's, and
    the B = 64 result is a fresh engine's.  A raw C call at B = 9 writes nothing past row 9 of dz, objective, probs and images
    nor past the 3 x 9 floats of terms (buffers for 64 rows, pre-filled with 7)."""
    size, latent = 64, 100
    z = {b: torch.from_numpy(I.gen_z(b, latent, SEED["z"])).cuda() for b in (9, 64)}
    zt = {b: torch.from_numpy(I.gen_z(b, latent, SEED["z"] + 1)).cuda() for b in (9, 64)}
    fresh = {}
    for b in (9, 64):
        eng = objective_engine(size, latent, b)
        t_u8 = eng.g_generate_u8(zt[b])
        fresh[b] = tuple(t.clone() for t in eng.g_latent_objective_grad(z[b], t_u8, *ALL3, **KW))
        eng.close()
    eng = objective_engine(size, latent, 64)
    t = {b: eng.g_generate_u8(zt[b]).clone() for b in (9, 64)}
    got = [tuple(x.clone() for x in eng.g_latent_objective_grad(z[b], t[b], *ALL3, **KW)) for b in (9, 64, 9)]
    for name, a, b, f in zip(NAMES, got[0], got[2], fresh[9]):
        assert torch.equal(a, b), f"{name}: B = 9 after B = 64 differs from B = 9 before it"
        assert torch.equal(a, f), f"{name}: B = 9 on a max_batch-64 context differs from a max_batch-9 context's"
    for name, a, f in zip(NAMES, got[1], fresh[64]):
        assert torch.equal(a, f), f"{name}: B = 64 after B = 9 differs from a fresh context's"
    full = lambda *shape: torch.full(shape, 7.0, device="cuda")
    dz, obj, terms, probs, img = full(64, latent), full(64), full(3 * 64), full(64), full(64, 1, size, size)
    rc = T._raw_call(eng, z[9], t[9], None, ALL3, dz, obj, 9, terms, probs, img)
    torch.cuda.synchronize()
    assert rc == 0, eng.lib.siggan_last_error()
    for name, buf, want in zip(NAMES, (dz, obj, terms, probs, img), got[0]):
        n = want.numel()
        assert torch.equal(buf.reshape(-1)[:n], want.reshape(-1)), name
        assert bool((buf.reshape(-1)[n:] == 7.0).all()), f"{name}: written past the 9 images"
    eng.close()
