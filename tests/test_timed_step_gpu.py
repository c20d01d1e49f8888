"""The timed training step held to the oracle directly, at the workloads bench.py reports (common.TIMED).

bench.py times one code path: DataParallelStep.step(real, next_real=real) on an engine built by init_reference(seed=0), fresh
Adam state, overlap mode, library RNG.  It is not the path the other parity tests take (d_step / g_step with injected z and
masks): the G step's training forward runs beside the D backward (siggan_step_begin), z and the dropout tables are drawn on
the device, the D update runs the pending G step's first Discriminator block in B * S/4 rider workgroups (k_adam_pack; fp32
contexts), and the next step's D(real) forward with its dropout tables drawn ahead runs beside the Generator backward
(siggan_stage_real).  Here that loop runs four steps -- step 0 with no staged batch, steps 1-3 on a staged batch and an
already-updated network -- making DataParallelStep.step's ABI calls with read points between them, and every half-step is
compared with the oracle run from the engine's own state before it (as test_three_step_sequence does), given the noise the
library drew and the HIP path's sign decisions.  One assertion shows the read points did not change the path: the final state
equals an uninstrumented dp.step loop's, bit for bit.

The same check runs at common.BATCH_EDGES, batches that reach launcher paths no benchmark record does (one step at the
largest), and one test pins the GEMM tile each added workload exists for (common.COVERS) through the library's profiler."""
import copy
import resource
import time

import pytest
import torch

from common import BATCH_EDGES, COVERS, DK, GK, TIMED, O, assert_close
from hipcommon import (assert_same_state, bench_setup, count_sign_flips, debug_scalar, full_state, grad_scales, hip_d_masks,
                       hip_signs_d, hip_signs_g, oracle_state_of)
from signature_gan_amd import _lib
from test_engine_gpu import MARGINS, _Half, _close_halves, _dump_margins, _scale_close
from test_narrow_gpu import SIGN_DIST, SIGN_FRAC, TOL_FP32, TOL_Q, assert_narrow_row, compare_d_half, compare_g_half

pytestmark = pytest.mark.gpu
STEPS = 4
# per workload: the worst deviation of each kind over the four steps, and the largest fraction of its tolerance any check
# used -- recorded with the other parity margins (test_engine_gpu.MARGINS, under "timed_step/...") for the measurement record


def _metrics(eng, keys):
    m = eng.metrics.cpu()
    return {k: float(m[_lib.METRIC_INDEX[k]]) for k in keys}


def _worst_tensor(got, want, names, scale):
    """name of the gradient tensor furthest from the oracle's, relative to its comparison scale (for the margins record)"""
    return max(names, key=lambda k: float((got[k] - want[k]).abs().max()) / scale[k])


def _metric_frac(got, want, keys, rt=2e-4, at=2e-6):
    """largest |got - want| as a fraction of assert_close's tolerance"""
    return max(abs(got[k] - want[k]) / (at + rt * abs(want[k])) for k in keys)


def _fp32_d_half(eng, size, real, z, masks, signs, state, m):
    g_sd, d_sd, _, d_opt = copy.deepcopy(state)
    init_d, init_opt = state[1], state[3]
    rec = []
    om, og = O.d_step(g_sd, d_sd, d_opt, real, z, masks[: len(masks) // 2], masks[len(masks) // 2:], size, signs=signs, record=rec)
    m["sign_flips"] = max(m["sign_flips"], count_sign_flips(signs, rec, keep=masks))
    met = _metrics(eng, DK)
    for k in DK:
        assert_close(met[k], om[k], 2e-4, 2e-6, f"D metric {k} vs oracle(HIP signs) from the engine's state")
    m["metric_frac"] = max(m["metric_frac"], _metric_frac(met, om, DK))
    names = list(eng.views("d", "grads"))
    mine, scale = _Half.of_engine(eng, "d", met), grad_scales(og, names)
    worst = _close_halves(mine, _Half.of_oracle(om, og, d_sd, d_opt), names, scale, init_d, init_opt, 1e-4,
                          "D half vs oracle(HIP signs)")
    if worst >= m["d_grad"]:
        m["d_grad"], m["d_grad_worst_tensor"] = worst, _worst_tensor(mine.g, og, names, scale)


def _fp32_g_half(eng, size, z, signs, state, m):
    g_sd, d_sd, g_opt, _ = copy.deepcopy(state)
    init_g, init_opt = state[0], state[2]
    rec = []
    om, og = O.g_step(g_sd, d_sd, g_opt, z, size, signs=signs, record=rec)
    m["sign_flips"] = max(m["sign_flips"], count_sign_flips(signs, rec))
    met = _metrics(eng, GK)
    for k in GK:
        assert_close(met[k], om[k], 2e-4, 2e-6, f"G metric {k} vs oracle(HIP signs) from the engine's state")
    m["metric_frac"] = max(m["metric_frac"], _metric_frac(met, om, GK))
    names = list(eng.views("g", "grads"))
    mine, scale = _Half.of_engine(eng, "g", met), grad_scales(og, names)
    worst = _close_halves(mine, _Half.of_oracle(om, og, g_sd, g_opt), names, scale, init_g, init_opt, 1e-4,
                          "G half vs oracle(HIP signs)")
    if worst >= m["g_grad"]:
        m["g_grad"], m["g_grad_worst_tensor"] = worst, _worst_tensor(mine.g, og, names, scale)
    for k, t in eng.bn_views().items():
        if "num_batches" in k:
            assert int(t) == int(g_sd[k]), k
            continue
        got, want = t.float().cpu(), g_sd[k].float()
        _scale_close(got.numpy(), want.numpy(), f"BatchNorm buffer {k} vs oracle")
        m["bn"] = max(m["bn"], float((got - want).abs().max()) / (float(want.abs().max()) + 1e-30))


def _tol_fp32(dtype, row):
    """TOL_FP32, except for the BatchNorm running statistics: at least 1.6 x (TOL_FP32's margin over what it was set from)
    the distance of the storage-rounding oracle's own statistics from the fp32 oracle's in this very step.

    TOL_FP32["bn"] was measured on the synthetic warm state of test_narrow_steps.  From init_reference's weights (N(0, 0.02),
    zero biases) the batch means of every pre-BatchNorm layer are near-cancelling sums, so a running mean after a few updates
    is ~1e-2 -- and 16-bit storage of the values summed moves it by ~2e-3 (bf16) / ~3e-4 (fp16) of that: measured for the
    oracle alone (oracle.Quant vs fp32, no HIP code involved), which the HIP path matches to TOL_Q["bn"].  The fp32 bar on
    these buffers thus measures the storage type, not the kernels; the kernels are held by the TOL_Q comparison."""
    return dict(TOL_FP32[dtype], bn=max(TOL_FP32[dtype]["bn"], 1.6 * row["bn_q_oracle_vs_fp32"]))


# Sign decisions the HIP path and the storage-rounding oracle take differently: bounded for both 16-bit types at the coarser
# type's SIGN_FRAC / SIGN_DIST.  fp16 was measured at 1.7e-3 of a layer's elements, up to 4.1e-3 of its largest |x| from zero
# (D step 0, 128x128 batch 32, from init_reference) -- over the 8e-4 / 2.5e-3 set on test_narrow_steps' synthetic state,
# where the layers' largest pre-activations stand further above the bulk.  The gradients those decisions feed still agree with
# the storage-rounding oracle at TOL_Q (the arithmetic check), with a wide margin.
TIMED_SIGN_BOUNDS = (SIGN_FRAC["bf16"], SIGN_DIST["bf16"])


@pytest.mark.parametrize("dtype,size,latent,batch", TIMED)
def test_timed_step_vs_oracle(dtype, size, latent, batch):
    _timed_vs_oracle(dtype, size, latent, batch, STEPS)


@pytest.mark.parametrize("dtype,size,latent,batch,steps", BATCH_EDGES)
def test_batch_edge_step_vs_oracle(dtype, size, latent, batch, steps):
    """The same check at the batches of common.BATCH_EDGES, whose paths (tile, fallback, fc kernel, rider count) no benchmark
    record reaches; records the row's wall time with its margins, and the peak host memory of the whole test process so far
    (ru_maxrss: an upper bound for the row's own, which depends on what ran before it in the process)."""
    t0 = time.perf_counter()
    m = _timed_vs_oracle(dtype, size, latent, batch, steps)
    m["wall_s"] = round(time.perf_counter() - t0, 1)
    m["process_peak_rss_gb"] = round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20, 2)
    MARGINS[f"timed_step/{dtype}/s{size}_b{batch}"] = m
    _dump_margins()


def _timed_vs_oracle(dtype, size, latent, batch, steps):
    eng, dp, real = bench_setup(dtype, size, latent, batch)
    hp, real_c = dp.hp, real.cpu()
    assert eng._mode == 2 and dp.transport == "host"       # overlap on, no graph (pre_real is off under graph mode)
    # the riders run at fp32 only: the 16-bit contexts measured faster with the first block as a launch of its own, and
    # fp16 has no one-launch update at all (its overflow guard) -- step.hip apply_common
    ride = batch if dtype == "f32" else 0
    m = dict(rode=ride, riders=ride * (size // 4))
    m.update(dict(sign_flips=0, metric_frac=0.0, d_grad=0.0, g_grad=0.0, bn=0.0) if dtype == "f32" else dict(narrow=[]))
    for s in range(steps):
        where = f"{dtype} s{size} b{batch} step {s}"
        before = oracle_state_of(eng, size, latent)
        # ---- D half: DataParallelStep.step's calls, world 1 (the all-reduce of the host transport is a no-op) ----
        eng.step_begin(real, None, None, None, hp["ls"])
        z = eng.debug_tensor("z", 0, (batch, latent)).cpu()
        masks = hip_d_masks(eng, size, batch)
        signs_d = hip_signs_d(eng, size, batch, 2)        # before d_apply: its riders overwrite rows [B, 2B) of block 1
        eng.d_apply(hp["lr_d"], hp["beta1"], hp["beta2"], clip=hp["clip"], grad_scale=1.0, sync=False)
        if dtype == "f32":
            try:
                _fp32_d_half(eng, size, real_c, z, masks, signs_d, before, m)
            except AssertionError as e:
                raise AssertionError(f"{where}, D half: {e}") from e
        else:
            row = compare_d_half(eng, dtype, size, real_c, z, masks, signs_d, _metrics(eng, DK),
                                 lambda: copy.deepcopy(before), {})
        # ---- G half: the oracle starts from the updated D and the Generator as it was before the step (the pipelined
        # training forward has already moved the engine's BatchNorm running statistics) ----
        after_d = oracle_state_of(eng, size, latent)
        g_state = (before[0], after_d[1], before[2], after_d[3])
        eng.stage_real(real)
        eng.g_compute_grads(batch)
        z_g = eng.debug_tensor("z_g", 0, (batch, latent)).cpu()
        signs_g = hip_signs_g(eng, size, batch) + hip_signs_d(eng, size, batch, 1)
        rode, pre_real = debug_scalar(eng, "rode"), debug_scalar(eng, "pre_real")
        eng.g_apply(hp["lr_g"], hp["beta1"], hp["beta2"], clip=hp["clip"], grad_scale=1.0, sync=False)
        # rows [B, 2B) of block 1 came from k_adam_pack's riders (not a fallback forward), and the next step's D(real)
        # forward was started beside the Generator backward: on every step, step 0 included
        assert rode == ride, f"{where}: the G step's first Discriminator block: rode {rode}, expected {ride}"
        assert pre_real == batch, f"{where}: the staged D(real) forward did not run beside the Generator backward"
        if dtype == "f32":
            try:
                _fp32_g_half(eng, size, z_g, signs_g, g_state, m)
            except AssertionError as e:
                raise AssertionError(f"{where}, G half: {e}") from e
        else:
            compare_g_half(eng, dtype, size, z_g, signs_g, _metrics(eng, GK), lambda: copy.deepcopy(g_state), row)
            m["narrow"].append(row)
            MARGINS[f"timed_step/{dtype}/s{size}_b{batch}"] = m
            _dump_margins()
            assert_narrow_row(row, dtype, tol_fp32=_tol_fp32(dtype, row), sign_bounds=TIMED_SIGN_BOUNDS)
    torch.cuda.synchronize()
    assert debug_scalar(eng, "ride_late") == 0.0
    instrumented = full_state(eng)
    eng.close()

    eng, dp, real = bench_setup(dtype, size, latent, batch)
    for _ in range(steps):
        dp.step(real, next_real=real)
    torch.cuda.synchronize()
    assert debug_scalar(eng, "ride_late") == 0.0
    assert_same_state(instrumented, full_state(eng), "the instrumented loop vs dp.step")
    eng.close()

    if dtype == "f32":
        m["worst_fraction_of_tolerance"] = max(m["d_grad"] / 1e-4, m["g_grad"] / 1e-4, m["metric_frac"], m["bn"] / 2e-4)
    else:
        fr = lambda r: {"fp32": _tol_fp32(dtype, r), "q": TOL_Q[dtype]}
        m["worst_fraction_of_tolerance"] = max(
            r[f"{net}_{kind}_vs_{tag}"] / fr(r)[tag][kind] for r in m["narrow"] for tag in ("fp32", "q") for net in ("d", "g")
            for kind in ("metric", "grad_t", "grad_all"))
        m["worst_fraction_of_tolerance"] = max(m["worst_fraction_of_tolerance"],
                                               max(r[f"bn_vs_{tag}"] / fr(r)[tag]["bn"] for r in m["narrow"] for tag in ("fp32", "q")))
        m["worst_fraction_of_tolerance"] = max(m["worst_fraction_of_tolerance"],
                                               max(r[f"{net}_sign_{k}"] / b for r in m["narrow"] for net in ("d", "g")
                                                   for k, b in zip(("frac", "dist"), TIMED_SIGN_BOUNDS)))
        m["worst_fraction_of_tolerance_fp32_bn_at_TOL_FP32"] = max(r["bn_vs_fp32"] / TOL_FP32[dtype]["bn"] for r in m["narrow"])
    MARGINS[f"timed_step/{dtype}/s{size}_b{batch}"] = m
    _dump_margins()
    return m


@pytest.mark.parametrize("dtype,size,latent,batch", list(COVERS))
def test_added_workloads_reach_their_launches(dtype, size, latent, batch):
    """Each workload added to TIMED / BATCH_EDGES for a launcher path makes, in one timed step, the launches common.COVERS
    lists for it: the tile, form, epilogue and GEMM shape, read per launch from the library's profile.  Profiling is
    process-wide and turns the riders off: this engine is its own, and the profiler is off again before the next test."""
    eng, dp, real = bench_setup(dtype, size, latent, batch)
    eng.prof_enable(True)
    try:
        dp.step(real, next_real=real)
        torch.cuda.synchronize()
        launches = eng.prof_launches()
    finally:
        eng.prof_enable(False)
        eng.close()
    seen = sorted({tuple(sorted(l.items())) for l in launches if l["M"] >= 0})
    for want in COVERS[(dtype, size, latent, batch)]:
        hit = [l for l in launches if all(l[k] == v for k, v in want.items())]
        assert hit, (f"{dtype} s{size} b{batch} no longer makes the launch it exists for: {want}; "
                     f"its GEMM launches were {[dict(t) for t in seen]}")
    if batch <= 256:
        # (the fallback belongs to the b1025 row alone: below it every statistics epilogue fits its carve)
        assert not [l for l in launches if l["epi_req"] == "bn_bwd_stats" and l["epi"] != "bn_bwd_stats"]
