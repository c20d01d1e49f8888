#!/usr/bin/env python3
"""Headline benchmark: signature images/sec for one G+D train step (n_critic = 1).

    python bench.py --gpus N --steps K --warmup W [--dtype f32|bf16|f16] [--size 64|128] [--batch B] [--latent Z]
                    [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Default workload (BASELINE.json configs[1], the configuration the metric is quoted on): reference conv G/D, 64x64x1,
z = 100, batch 64 PER GPU, fp32, dropout 0.25 active in the D step, label smoothing 0.9, Adam lr 2e-4 betas (0.5, 0.999),
clipping off; the real batch is synthetic U[-1,1] resident in HBM, z and the dropout masks are drawn by the library's RNG
inside the step, weights are random-init from the reference's init distribution.  The other flags select the per-GPU
workloads of the other BASELINE configs (tracked lines under profiles/, not the driver's line): --batch 128 (configs[3]),
--dtype bf16 (configs[2]: bf16 storage / MFMA operands, fp32 masters), --size 128 --latent 128 --batch 32 --dtype f16
(configs[4]).

A "step" = siggan_step_begin / d_apply / g_grads / g_apply through the C ABI.  With N > 1 every rank runs the step on its
own shard (weak scaling, per-replica BatchNorm) and the two flat gradient buckets are sum-all-reduced over RCCL INSIDE the
library (siggan_comm_init; torch.distributed only carries the 128-byte id and the timing barrier).

Timing: W warm-up steps, then ONE block of EXACTLY K timed steps, bracketed by a barrier + torch.cuda.synchronize() on both
sides and reduced with MAX over ranks; `ms_per_step` / `value` are that block.  A plain run does nothing else: set up, warm
up, time the K steps, write the outputs (--dump-outputs) and print the line.

--dump-outputs DIR: after the timed block, rank 0 writes what a caller of the step holds after its last step -- the 16
training metrics and the updated G / D weights and G BatchNorm buffers -- as DIR/<name>.npy in float32 (under 64 MB; a
larger set is cut to a fixed, seeded sample).  Inputs are seeded: the same arguments give the same inputs in every run.

--full adds, after the dump, everything the headline does not need (each leg can still be skipped by its --no-* flag):
  timing       -- `--blocks` - 1 (default 10 - 1) further blocks of K steps: median / p10 / p90 over all blocks
  roofline     -- the dominant MFMA kernel: algorithmic FLOPs per launch / its mean launch duration, measured live with HIP
                  events stamped by the launch itself (hipExtLaunchKernelGGL) over a second, instrumented pass of K steps run
                  one kernel at a time; `peak` is derived from the device (compute units x clock x FLOP/clk/CU of the dtype's
                  MFMA); `hbm` gives the same kernel's algorithmic bytes / duration against 8 TB/s.  `traffic` (HBM bytes per
                  launch from PMC counters) comes from a committed rocprofv3 pass and is labelled with its file
  secondary    -- generation throughput (G eval forward) on the same engine and batch
  cpu_baseline -- the oracle's same step (torch CPU, fp32) timed on the host cores of the same box in the same run (rank 0, at
                  every N); `cores` = the threads used, `host` = the box's physical cores / logical CPUs / this job's share
Without --full these objects are null.

Parity contract of what is measured here (tests/test_engine_gpu.py through the C ABI; numbers of the round's final binary in
profiles/r04_parity_margins.json, the attribution in profiles/r03_flip_attribution.txt): against the reference run's fixtures
the north star's 1e-3 holds for losses, predictions, generated images and BatchNorm buffers in every case, and for gradients /
Adam moments / weights wherever the HIP path takes the same (Leaky)ReLU sign decisions as the reference run did.  Where a
pre-activation lies within 1e-5 of its layer's scale of zero and the two fp32 implementations land on different sides (1-12
such elements per step out of ~1e7; the reference re-run with another thread count does the same to itself), the gradients
differ by exactly what those decisions produce: HIP = oracle(HIP's decisions) to 1e-4 of each tensor's scale (worst 7e-5),
oracle(reference's decisions) = reference to 1e-4, and HIP - reference = the difference of the two oracle runs to 1e-3
(residual <= 7e-5).  In round 3's record 18 of 42 step rows met the strict bound directly and 24 went through that chain; the
largest raw deviation was 1.27e-2 on final_conv.0.bias (one scalar, a near-cancelling sum over 524 288 pixels, 12 decisions).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# algorithmic work per image per G+D step: 8*D_fwd + 4*G_fwd (conv / convT / linear MACs x 2), SURVEY 8(d)
FLOP_PER_IMAGE = {(64, 100): 1975.8e6, (128, 128): 9240.2e6}
FLOP_PER_CLK_PER_CU = {"f32": 256, "bf16": 4096, "f16": 4096}   # MI355X_MICROARCH.md: 64 (f32) / 1024 (16-bit) FLOP/clk/SIMD x 4
HBM_PEAK_GBPS = 8000.0                                          # MI355X_MICROARCH.md: HBM3E 8 TB/s (spec)


def flop_per_image(size, latent):
    if (size, latent) in FLOP_PER_IMAGE:
        return FLOP_PER_IMAGE[(size, latent)]
    base = FLOP_PER_IMAGE[(64, 100)] if size == 64 else FLOP_PER_IMAGE[(128, 128)]
    z0, feat = (100, 4096) if size == 64 else (128, 8192)
    return base + 4 * 2 * feat * (latent - z0)                  # only the fc GEMM depends on the latent size (4 x G_fwd)


def host_cores():
    """(physical cores, logical CPUs, CPUs this process may run on) of the box: /proc/cpuinfo's distinct (physical id, core id)
    pairs -- the north star asks for the core count to be stated beside the CPU number."""
    phys = set()
    try:
        pid = cid = None
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("physical id"):
                    pid = line.split(":")[1].strip()
                elif line.startswith("core id"):
                    cid = line.split(":")[1].strip()
                elif not line.strip():
                    if pid is not None and cid is not None:
                        phys.add((pid, cid))
                    pid = cid = None
        if pid is not None and cid is not None:
            phys.add((pid, cid))
    except OSError:
        pass
    try:
        share = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        share = os.cpu_count() or 1
    return len(phys) or None, os.cpu_count() or 1, share


def cpu_baseline(threads, size, latent, batch, budget_s=12.0):
    """The oracle (kind "port") on the host cores: same step, same shapes, fp32."""
    import torch
    for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from common import I, O, oracle_states
    torch.set_num_threads(threads)
    g_sd, d_sd, g_opt, d_opt = oracle_states(size, latent, warm=False)
    real = torch.from_numpy(I.gen_real(batch, size, 22))
    chans = list(O.D_CHAIN[size])
    gen = torch.Generator().manual_seed(3)

    def one():
        z1, z2 = torch.randn(batch, latent, generator=gen), torch.randn(batch, latent, generator=gen)
        masks = [(torch.rand(batch, c, generator=gen) < 0.75).float() for c in chans * 2]
        O.d_step(g_sd, d_sd, d_opt, real, z1, masks[:len(chans)], masks[len(chans):], size)
        O.g_step(g_sd, d_sd, g_opt, z2, size)

    one(); one()
    n, t0 = 0, time.perf_counter()
    while True:
        one(); n += 1
        dt = time.perf_counter() - t0
        if dt >= budget_s or n >= 64:
            break
    return batch * n / dt, n


DUMP_LIMIT_BYTES = 60_000_000                     # --dump-outputs: under 64 MB in all, .npy headers included


def dump_outputs(out_dir, arrays):
    """arrays: name -> tensor.  Written as out_dir/<name>.npy in float32.  If they hold more than DUMP_LIMIT_BYTES in all,
    every array above 64 K elements is cut to the same fraction of its (flattened) elements, at sorted indices drawn from
    a fixed seed, so that two builds still compare element for element."""
    import numpy as np
    small = 1 << 16
    host = {k: v.detach().float().cpu().numpy().reshape(-1) for k, v in arrays.items()}
    fixed = sum(a.nbytes for a in host.values() if a.size <= small)
    large = sum(a.nbytes for a in host.values() if a.size > small)
    frac = min(1.0, (DUMP_LIMIT_BYTES - fixed) / large) if large else 1.0
    os.makedirs(out_dir, exist_ok=True)
    for k, a in host.items():
        if frac < 1.0 and a.size > small:
            keep = max(1, int(a.size * frac))
            a = a[np.sort(np.random.default_rng(1234).choice(a.size, keep, replace=False))]
        np.save(os.path.join(out_dir, f"{k}.npy"), np.ascontiguousarray(a, dtype=np.float32))


def step_outputs(m):
    """What a caller of the train step holds after it: metrics, updated weights, G BatchNorm running statistics."""
    return {"metrics": m.metrics, "g_params": m.g_params, "d_params": m.d_params,
            "g_bn_running_mean": m.g_bn_mean, "g_bn_running_var": m.g_bn_var}


def bench_mlp(args):
    """BASELINE.json configs[0] as worded (fully-connected G/D, 28x28, batch 32): a BUILD-DEFINED extension with no reference
    model -- parity unpinned (include/siggan_mlp.h).  Same timing protocol; the CPU leg times the extension's own oracle."""
    import torch
    import signature_gan_amd  # noqa: F401
    from signature_gan_amd.mlp_gan import MLPGAN
    size, batch, hidden = args.size, args.batch, (256, 512)
    torch.cuda.set_device(0)
    m = MLPGAN(latent_dim=100, image_size=size, hidden=hidden, max_batch=batch, device="cuda:0", seed=2)
    real = (torch.rand(batch, 1, size, size, generator=torch.Generator().manual_seed(1)) * 2 - 1).cuda()
    for _ in range(args.warmup):
        m.train_step(real, sync=False)

    def timed_block():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            m.train_step(real, sync=False)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    dt = timed_block()
    met = m.metrics.cpu()
    assert torch.isfinite(met).all()
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, step_outputs(m))
    blocks = [dt]
    if args.full:
        blocks += [timed_block() for _ in range(max(1, args.blocks) - 1)]
    dims = [100, *hidden, size * size]
    fwd = sum(2 * a * b for a, b in zip(dims[:-1], dims[1:]))            # G forward = D forward (mirror) FLOP per image, + the 1-wide head
    flop_img = 8 * (fwd - 2 * 100 * hidden[0] + 2 * hidden[0]) + 4 * fwd   # 8 x D_fwd + 4 x G_fwd, as for the conv model
    cpu = None
    if args.full and not args.no_cpu:
        from oracle import mlp_oracle as M
        from oracle.siggan_oracle import AdamState
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        g_sd = {k: v.cpu().clone() for k, v in m.views("g").items()}
        g_sd.update({k: v.cpu().clone() for k, v in m.bn_views().items()})
        d_sd = {k: v.cpu().clone() for k, v in m.views("d").items()}
        g_opt, d_opt = AdamState(list(m.g_spans), g_sd), AdamState(list(m.d_spans), d_sd)
        rc, n, t0 = real.cpu(), 0, time.perf_counter()
        while time.perf_counter() - t0 < 8.0:
            M.d_step(g_sd, d_sd, d_opt, rc, torch.randn(batch, 100), hidden, size)
            M.g_step(g_sd, d_sd, g_opt, torch.randn(batch, 100), hidden, size)
            n += 1
        cpu = {"value": round(batch * n / (time.perf_counter() - t0), 1), "unit": "images/s", "cores": torch.get_num_threads(), "kind": "port",
               "sample": f"{n} G+D steps of the same workload by oracle/mlp_oracle.py (torch CPU; the extension's own restatement: parity unpinned)"}
    cus, khz, _ = __import__("signature_gan_amd.engine", fromlist=["Engine"]).Engine.device_info(0)
    peak = cus * khz * 1e3 * FLOP_PER_CLK_PER_CU["f32"] / 1e12
    imgs = batch * args.steps
    print(json.dumps({
        "metric": f"signature images/sec (MLP G+D train step, bs{batch} {size}x{size} z=100)", "value": round(imgs / dt, 1), "unit": "images/s",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * dt / args.steps, 4), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"configs[0] as worded: fully-connected G 100-256-512-{size * size} / mirror D, {size}x{size}x1, batch {batch}, fp32 -- "
                               "BUILD-DEFINED extension, the reference has no such model: PARITY UNPINNED", "global_batch": batch, "parallelism": "dp1"},
        "timing": timing_summary(blocks, args.steps),
        "achieved_tflops_whole_step": round(imgs / dt * flop_img / 1e12, 4),
        "frac_of_mfma_peak_whole_step": round(imgs / dt * flop_img / 1e12 / peak, 6),
        "roofline": None, "note": "launch-bound: ~0.4 GFLOP per step spread over ~45 launches; no kernel of this path is near any roofline",
        "final_metrics": {"d_loss": round(float(met[0]), 4), "g_loss": round(float(met[8]), 4)}, "cpu_baseline": cpu}), flush=True)
    m.close()


def launch_ranks(n, argv):
    """`python bench.py --gpus N` with N > 1 and no launcher around it (no WORLD_SIZE in the environment): this process
    becomes the launcher.  It starts N children -- the same command line, one rank each, RANK / LOCAL_RANK / WORLD_SIZE /
    MASTER_ADDR / MASTER_PORT set as torch.distributed.run would set them -- relays rank 0's stdout (the ONE JSON line),
    sends the other ranks' stdout to stderr, and exits with the worst child's code.  It never imports torch and never
    touches HIP: a process that has initialised the GPU must not be the parent of the ranks' rendezvous, and must never
    exec.  If a rank dies, the others (which would wait in a collective for ever) are terminated by PID."""
    import socket
    import subprocess
    with socket.socket() as sk:                                  # a free rendezvous port on the loopback interface
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=os.environ.get("MASTER_PORT", str(port)))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")        # dmabuf IPC: what RCCL needs between processes on this pool
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env,
                                      stdout=None if r == 0 else sys.stderr))
    worst, live = 0, set(range(n))
    while live:
        for r in sorted(live):
            rc = procs[r].poll()
            if rc is None:
                continue
            live.discard(r)
            if rc != 0:
                worst = worst or rc
                print(f"[bench] rank {r} exited with code {rc}; stopping the other ranks", file=sys.stderr, flush=True)
                for q in live:
                    procs[q].terminate()
        if live:
            time.sleep(0.05)
    return worst


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, max(0, int(round(q * (len(xs) - 1)))))]


def timing_summary(block_s, steps):
    """block_s[0] is the headline block (`ms_per_step`); --full adds the spread over all blocks."""
    out = {"blocks": len(block_s), "steps_per_block": steps, "headline": "block 1"}
    if len(block_s) > 1:
        out.update({"ms_per_step_median": round(1e3 * statistics.median(block_s) / steps, 4),
                    "ms_per_step_p10": round(1e3 * pct(block_s, 0.1) / steps, 4),
                    "ms_per_step_p90": round(1e3 * pct(block_s, 0.9) / steps, 4)})
    return out


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=10,
                    help="with --full: blocks of --steps steps in all, the headline block included (median / p10 / p90 over them)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline: further timing blocks, the roofline pass, generation throughput and the CPU "
                         "baseline (each still skippable by its --no-* flag)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's metrics, weights and BatchNorm buffers to DIR/<name>.npy (float32)")
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16", "f16"])
    ap.add_argument("--model", default="conv", choices=["conv", "mlp"],
                    help="conv: the reference's G/D (default, the headline). mlp: the fully-connected extension (configs[0], parity unpinned)")
    ap.add_argument("--size", type=int, default=None, help="64 | 128 (conv); any (mlp, default 28)")
    ap.add_argument("--latent", type=int, default=None)
    ap.add_argument("--batch", type=int, default=64, help="batch PER GPU")
    ap.add_argument("--no-cpu", action="store_true", help="--full: skip the CPU baseline leg")
    ap.add_argument("--no-roofline", action="store_true", help="--full: skip the instrumented pass")
    ap.add_argument("--no-secondary", action="store_true", help="--full: skip the generation-throughput pass (the `secondary` object)")
    ap.add_argument("--serialize", action="store_true",
                    help="run every pass with side-lane overlap OFF (one kernel at a time): the mode the roofline "
                         "pass always uses, and the one to profile with rocprofv3 so per-kernel durations agree")
    ap.add_argument("--dist", action="store_true",
                    help="initialise torch.distributed (nccl) and the library's RCCL communicator even at world size 1")
    ap.add_argument("--metrics-readback", default="late", choices=["late", "none"],
                    help="late (default): every timed step's metrics are copied to pinned host memory asynchronously and read "
                         "one step late, as the drop-in trainer does (SURVEY 8b: one read-back per step); none: never read")
    ap.add_argument("--host-allreduce", action="store_true",
                    help="N > 1: reduce the gradient buckets with torch.distributed between the step halves instead of the "
                         "library's own communicator (fallback / comparison)")
    args = ap.parse_args(argv)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and args.model == "conv":
        return launch_ranks(args.gpus, argv)                     # before anything imports torch or touches the GPU
    if args.model == "mlp":
        args.size = args.size or 28
        return bench_mlp(args)
    args.size = args.size or 64
    if args.size not in (64, 128):
        ap.error("--size must be 64 or 128 for the conv model")
    size, batch, dtype = args.size, args.batch, args.dtype
    latent = args.latent if args.latent is not None else (100 if size == 64 else 128)

    import torch
    import torch.distributed as dist
    import signature_gan_amd  # noqa: F401
    from signature_gan_amd.dp import DataParallelStep, env_rank, init_library_comm
    from signature_gan_amd.engine import Engine

    rank, world, local = env_rank()
    grouped = args.gpus > 1 or world > 1 or args.dist
    if grouped:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        # SIGGAN_DIST_BACKEND=gloo: rehearsal of the multi-rank path on a box with fewer GPUs than ranks (ranks then
        # share devices round-robin and the buckets go through torch.distributed; RCCL refuses two ranks on one GPU).
        backend = os.environ.get("SIGGAN_DIST_BACKEND", "nccl")
        local = local % torch.cuda.device_count() if backend != "nccl" else local
        torch.cuda.set_device(local)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
            args.host_allreduce = True
    else:
        torch.cuda.set_device(0)
        local = 0
    dev = torch.device("cuda", local)

    eng = Engine(latent_dim=latent, image_size=size, max_batch=batch, device=str(dev), seed=2 + rank, dtype=dtype)
    eng.init_reference(seed=0)                                  # identical initial weights on every rank
    if args.serialize:
        eng.set_mode(graph=False, overlap=False)
    transport = "host" if (args.host_allreduce or not grouped) else "lib"
    comm_note = None
    if transport == "lib":
        # the library's own RCCL communicator; if ANY rank fails to create it, every rank falls back to reducing the two
        # gradient arenas with torch.distributed between the step halves (same arithmetic), and the line says so
        ok = 1
        try:
            if os.environ.get("SIGGAN_BENCH_FORCE_COMM_FAILURE"):  # rehearsal hook for the fallback below
                raise RuntimeError("forced by SIGGAN_BENCH_FORCE_COMM_FAILURE")
            init_library_comm(eng)
        except Exception as exc:                                 # noqa: BLE001 -- reported in the JSON line
            ok, comm_note = 0, f"{type(exc).__name__}: {exc}"
        if world > 1:
            flag = torch.tensor([ok], dtype=torch.int32, device=dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            ok = int(flag.item())
        if not ok:
            if eng.comm_world > 0:
                eng.comm_destroy()
            transport, comm_note = "host", comm_note or "another rank failed to create the library communicator"
            print(f"[bench] rank {rank}: library RCCL communicator unavailable ({comm_note}); using torch.distributed",
                  file=sys.stderr, flush=True)
    dp = DataParallelStep(eng, transport=transport)
    dp.sync_initial_state()
    gen = torch.Generator(device="cpu").manual_seed(1 + rank)
    real = (torch.rand(batch, 1, size, size, generator=gen) * 2 - 1).to(dev)

    def barrier():
        torch.cuda.synchronize(dev)
        if grouped:
            dist.barrier()
        torch.cuda.synchronize(dev)

    # The loop hands each step the batch of the step after it as well (a prefetching loader has it):
    # that batch's D(real) forward then runs beside this step's Generator backward (siggan_stage_real).
    # Every step still does one D(real) forward -- for its successor instead of for itself.
    # One metrics read-back per step, as GANTrainer.train does it here: asynchronous copy of the 16 floats into
    # pinned host memory behind the step, read on the host one step late (so the host is never more than a step ahead).
    late = args.metrics_readback == "late"
    host_m = [torch.empty(eng.metrics.numel(), dtype=torch.float32).pin_memory() for _ in range(2)]
    host_ev = [torch.cuda.Event(), torch.cuda.Event()]
    seen = {"n": 0, "d_loss": 0.0, "g_loss": 0.0}

    def step(i):
        dp.step(real, next_real=real)
        if late:
            host_m[i & 1].copy_(eng.metrics, non_blocking=True)
            host_ev[i & 1].record()
            if i > 0:
                host_ev[(i - 1) & 1].synchronize()
                seen["n"] += 1; seen["d_loss"] += float(host_m[(i - 1) & 1][0]); seen["g_loss"] += float(host_m[(i - 1) & 1][8])

    def timed_block():
        barrier()
        t0 = time.perf_counter()
        for i in range(args.steps):
            step(i)
        barrier()
        dt = time.perf_counter() - t0
        if grouped and world > 1:
            t = torch.tensor([dt], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt

    for i in range(args.warmup):
        step(i)
    dt = timed_block()                                          # the headline: exactly --steps timed steps
    m = eng.metrics.cpu()
    assert torch.isfinite(m).all(), "non-finite training metrics"
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, step_outputs(eng))
    block_s = [dt]
    if args.full:
        block_s += [timed_block() for _ in range(max(1, args.blocks) - 1)]

    cus, khz, hbm_bytes = Engine.device_info(local)
    peak = cus * khz * 1e3 * FLOP_PER_CLK_PER_CU[dtype] / 1e12          # TFLOP/s, dense, for this dtype's MFMA
    fpi = flop_per_image(size, latent)

    roofline = None
    if rank == 0 and args.full and not args.no_roofline:
        # one kernel at a time: a launch's event-bracketed time is then the kernel's own duration
        # (with overlap on, two MFMA kernels share the chip and each looks proportionally longer)
        eng.set_mode(graph=False, overlap=False)
        eng.prof_enable(True)
        for _ in range(args.steps):
            if world == 1:
                dp.step(real, next_real=real)
            else:
                eng.d_compute_grads(real); eng.g_compute_grads(batch)       # local kernels only: no collective on one rank alone
        recs = eng.prof_read()
        eng.prof_enable(False)
        eng.set_mode(graph=False, overlap=not args.serialize)
        top = max(recs, key=lambda r: r["ms"])
        ach = top["flops"] / (top["ms"] * 1e-3) / 1e12
        gbps = top["bytes"] / (top["ms"] * 1e-3) / 1e9
        traffic, traffic_src, step_bytes = None, None, None   # HBM bytes from the committed PMC passes (separate rocprofv3 runs)
        tag = "" if (dtype, size, batch) == ("f32", 64, 64) else f"_{dtype}_s{size}_b{batch}"
        tfile = next((t for t in (os.path.join("profiles", f"r{r:02d}_pmc_traffic{tag}.json") for r in (4, 3))
                      if os.path.exists(os.path.join(ROOT, t))), os.path.join("profiles", f"r04_pmc_traffic{tag}.json"))
        try:
            with open(os.path.join(ROOT, tfile)) as f:
                tj = json.load(f)
            traffic = tj["per_launch_bytes"][top["name"]]["total"]
            step_bytes = tj.get("per_step_bytes_all_library_kernels")
            traffic_src = {"file": tfile, "commit": tj.get("commit"), "note": "separate rocprofv3 --pmc passes of this workload, "
                           "FETCH_SIZE doubled per MI355X_MICROARCH.md; not measured in this run"}
        except (OSError, KeyError, ValueError):
            pass
        fam_ms, fam_fl = sum(r["ms"] for r in recs), sum(r["flops"] for r in recs)
        roofline = {
            "bound": "mfma", "kernel": top["name"] + ("" if dtype == "f32" else f" [{dtype} operands]"),
            "achieved": round(ach, 3), "peak": round(peak, 1), "unit": "TFLOP/s", "frac": round(ach / peak, 4),
            "peak_from": {"compute_units": cus, "clock_mhz": khz / 1e3, "flop_per_clk_per_cu": FLOP_PER_CLK_PER_CU[dtype]},
            "traffic": traffic, "traffic_source": traffic_src,
            "launches_per_step": top["launches"] / args.steps,
            "avg_launch_us": round(1e3 * top["ms"] / top["launches"], 2),
            "gflop_per_launch": round(top["flops"] / top["launches"] / 1e9, 4),
            "hbm": {"algorithmic_mb_per_launch": round(top["bytes"] / top["launches"] / 1e6, 3), "achieved": round(gbps, 1),
                    "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(gbps / HBM_PEAK_GBPS, 4)},
            # whole step: HBM bytes of ALL kernels of one step (same PMC passes) over this run's step time
            "hbm_whole_step": None if not step_bytes else {
                "mb_per_step": round(step_bytes / 1e6, 1), "achieved": round(step_bytes / (dt / args.steps) / 1e9, 1),
                "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(step_bytes / (dt / args.steps) / 1e9 / HBM_PEAK_GBPS, 4)},
            "mfma_family": {"ms_per_step": round(fam_ms / args.steps, 4),
                            "achieved": round(fam_fl / (fam_ms * 1e-3) / 1e12, 3),
                            "kernels": {r["name"]: {"launches_per_step": r["launches"] / args.steps,
                                                    "ms_per_step": round(r["ms"] / args.steps, 4),
                                                    "tflops": round(r["flops"] / (r["ms"] * 1e-3) / 1e12, 2),
                                                    "algorithmic_gbps": round(r["bytes"] / (r["ms"] * 1e-3) / 1e9, 1)} for r in recs}},
        }
    secondary = None
    if rank == 0 and args.full and not args.no_roofline and not args.no_secondary:
        # generation throughput (Generator.forward in eval mode, vanilla_gan_model.py:338-371) beside the headline,
        # same engine / weights / batch; MFMA kernels stamped one at a time as above (profiles/secondary.py has the wider table)
        gflop = {64: 87.06e6, 128: 414.19e6}[size] + 2 * (4096 if size == 64 else 8192) * (latent - (100 if size == 64 else 128))
        zgen = torch.randn(batch, latent, device=dev)
        for _ in range(10):
            eng.g_forward(zgen, training=False)
        torch.cuda.synchronize(dev); t0 = time.perf_counter()
        for _ in range(100):
            eng.g_forward(zgen, training=False)
        torch.cuda.synchronize(dev); tg = (time.perf_counter() - t0) / 100
        eng.set_mode(graph=False, overlap=False)
        eng.prof_enable(True)
        for _ in range(50):
            eng.g_forward(zgen, training=False)
        grecs = eng.prof_read()
        eng.prof_enable(False)
        eng.set_mode(graph=False, overlap=not args.serialize)
        secondary = {"generation": {"metric": f"generated images/sec (G eval forward, bs{batch} {size}x{size})", "value": round(batch / tg, 0),
                                    "us_per_batch": round(tg * 1e6, 1), "tflops": round(gflop * batch / tg / 1e12, 1),
                                    "frac_of_mfma_peak": round(gflop * batch / tg / 1e12 / peak, 4),
                                    "mfma_kernels_per_batch": {r["name"]: {"launches": r["launches"] / 50, "us": round(1e3 * r["ms"] / 50, 2),
                                                                           "tflops": round(r["flops"] / (r["ms"] * 1e-3) / 1e12, 1)} for r in grecs},
                                    "mfma_us_per_batch": round(sum(1e3 * r["ms"] for r in grecs) / 50, 1)}}
    cpu = None
    if rank == 0 and args.full and not args.no_cpu:
        # At every N, on rank 0, while the other ranks wait in the barrier below (their GPUs are idle: nothing is timed any
        # more).  Two thread counts -- this job's CPU share (16 per GPU on the pool's boxes) and 8, the survey container's
        # count; torch's oneDNN convs do not always scale past 8: the faster one is the baseline, the other is quoted in `sample`
        phys, logical, share = host_cores()
        runs = []
        for threads in sorted({min(16, share), min(8, share)}, reverse=True):
            v, n = cpu_baseline(threads, size, latent, batch, budget_s=10.0)
            runs.append((v, threads, n))
        (v, threads, n), rest = max(runs), [r for r in runs if r != max(runs)]
        other = "; ".join(f"{round(r[0], 1)} images/s with {r[1]} threads ({r[2]} steps)" for r in rest)
        cpu = {"value": round(v, 1), "unit": "images/s", "cores": threads, "kind": "port",
               "host": {"physical_cores": phys, "logical_cpus": logical, "cpus_usable_by_this_job": share},
               "sample": f"{n} G+D steps of the same workload (batch {batch}, {size}x{size}, fp32) by oracle/siggan_oracle.py "
                         f"on torch CPU with {threads} threads" + (f"; {other}" if other else "")}
    if grouped:
        dist.barrier()

    if rank == 0:
        imgs = batch * world * args.steps
        cfg_name = {("f32", 64, 64): "configs[1]", ("f32", 64, 128): "configs[3]", ("bf16", 64, 64): "configs[2] per-GPU shard",
                    ("f16", 128, 32): "configs[4] per-GPU shard"}.get((dtype, size, batch), "custom")
        out = {
            "metric": f"signature images/sec (G+D train step, bs{batch} {size}x{size} z={latent})",
            "value": round(imgs / dt, 1), "unit": "images/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1e3 * dt / args.steps, 4), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": dtype, "data": "synthetic",
            "config": {"workload": f"{cfg_name}: reference conv G/D {size}x{size}x1, z={latent}, batch {batch} per GPU, {dtype}, n_critic=1",
                       "global_batch": batch * world, "parallelism": f"dp{world}",
                       "metrics_readback": ("one per step, read one step late from pinned host memory (async copy + event), "
                                            f"{seen['n']} read in this run") if late else "none",
                       "gradient_allreduce": None if world == 1 and not grouped else
                       ("library RCCL (siggan_comm_init)" if transport == "lib" else "torch.distributed between the step halves"
                        + (f" (fallback: {comm_note})" if comm_note else ""))},
            "timing": timing_summary(block_s, args.steps),
            "achieved_tflops_whole_step": round(imgs / dt * fpi / 1e12, 3),
            "frac_of_mfma_peak_whole_step": round(imgs / dt * fpi / 1e12 / (peak * world), 4),
            "final_metrics": {"d_loss": round(float(m[0]), 4), "g_loss": round(float(m[8]), 4)},
            "roofline": roofline, "cpu_baseline": cpu, "secondary": secondary,
        }
        if dtype == "f32":
            out["frac_of_fp32_mfma_peak_whole_step"] = out["frac_of_mfma_peak_whole_step"]
        print(json.dumps(out), flush=True)
    if grouped:
        dist.destroy_process_group()
    eng.close()


if __name__ == "__main__":
    sys.exit(main() or 0)
