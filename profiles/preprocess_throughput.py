#!/usr/bin/env python3
"""Scans per second of preprocess.preprocess_scans on the MI355X, beside the host time Pillow needs to decode the same
files -- the bound a user of preprocess_signatures.preprocess_batch will actually see.

    python profiles/preprocess_throughput.py --height 512 --width 256 [--out profiles/preprocess_throughput.json]
    python profiles/preprocess_throughput.py --height 1024 --width 1024

One run measures 2048 synthetic scans of one size and merges its figures into the JSON under "<height>x<width>", so each
size runs under a time limit of its own.  The scans are DISTINCT pen-stroke scans (tests/preprocesscommon.pen_scan: PIL
polylines on noisy paper with specks) repeated to 2048; they go through the device in chunks of CHUNK scans, one
ScanBatch each (the chunk preprocess_signatures uses is at most 2^28 pixels).  Per size:
  "device"        preprocess_scans at 64 and at 128, pool resident: device events around all chunks, ROUNDS rounds after
                  WARMUP; scans per second from the median
  "pack_upload"   pack_scans of every chunk (host copy into the pool, upload, workspace allocation): a host clock around
                  work that ends in a synchronise
  "pillow_decode" Image.open(...).convert('L') into numpy for DECODE_FILES of the same scans written as PNG to a temporary
                  folder, ONE host thread, file cache warm: files per second
  "denoise_copy"  the floor of the first kernel alone: a device copy of the pool
No pass / fail threshold.  The device results of the distinct scans are checked against the numpy restatement.  Needs the
GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import preprocesscommon as PC  # noqa: E402
import signature_gan_amd  # noqa: E402,F401
from signature_gan_amd import preprocess  # noqa: E402

SCANS, DISTINCT, WARMUP, ROUNDS, DECODE_FILES, CHUNK_PIXELS = 2048, 8, 2, 5, 64, 1 << 28


def spread(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "samples": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preprocess_throughput.json"))
    ap.add_argument("--height", type=int, required=True)
    ap.add_argument("--width", type=int, required=True)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    h, w = a.height, a.width
    distinct = [PC.pen_scan(h, w, 900 + i, min_ink=0.06) for i in range(DISTINCT)]
    chunk = max(1, min(SCANS, CHUNK_PIXELS // (h * w)))
    chunks = [[distinct[(c + i) % DISTINCT] for i in range(min(chunk, SCANS - c))] for c in range(0, SCANS, chunk)]

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    pack_times = []
    for _ in range(2):
        t, batches = clock(lambda: [preprocess.pack_scans(c, dev) for c in chunks])
        pack_times.append(t)
    res = {"device_name": torch.cuda.get_device_name(0), "height": h, "width": w, "scans": SCANS, "distinct_scans": DISTINCT,
           "chunk_scans": chunk, "chunks": len(chunks), "warmup_rounds": WARMUP, "host_threads": 1,
           "workspace_bytes_per_chunk": int(batches[0].workspace.numel()), "pack_upload": spread(pack_times),
           "pack_upload_scans_per_s": SCANS / statistics.median(pack_times)}

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    for T in (64, 128):
        outs = [torch.empty((b.n, T, T), dtype=torch.uint8, device=dev) for b in batches]
        stats = [torch.empty((b.n, 13), dtype=torch.int32, device=dev) for b in batches]

        def run_all():
            for b, o, s in zip(batches, outs, stats):
                preprocess.preprocess_scans(b, T, out=o, stats=s)

        for _ in range(WARMUP):
            events(run_all)
        times = [events(run_all) for _ in range(ROUNDS)]
        want = [PC.restate(x, T) for x in distinct]
        o, s = outs[0].cpu().numpy(), stats[0].cpu().numpy()
        ok = all(np.array_equal(o[i], want[i % DISTINCT]["out"]) and np.array_equal(s[i], want[i % DISTINCT]["stats"])
                 for i in range(min(len(o), 2 * DISTINCT)))
        res[f"device_{T}"] = {**spread(times), "scans_per_s": SCANS / statistics.median(times),
                              "us_per_scan": 1e6 * statistics.median(times) / SCANS, "equals_restatement": bool(ok),
                              "status_nonzero": int((s[:, 0] != 0).sum())}
        print(T, json.dumps(res[f"device_{T}"]), flush=True)
    copies = [torch.empty_like(b.pool) for b in batches]
    copy_times = [events(lambda: [c.copy_(b.pool) for b, c in zip(batches, copies)]) for _ in range(WARMUP + ROUNDS)][WARMUP:]
    res["denoise_copy"] = spread(copy_times)

    with tempfile.TemporaryDirectory() as tmp:
        files = []
        for i in range(DECODE_FILES):
            files.append(os.path.join(tmp, f"scan_{i:04d}.png"))
            Image.fromarray(distinct[i % DISTINCT], mode="L").save(files[-1], "PNG")
        decode = lambda: [np.asarray(Image.open(f).convert("L"), dtype=np.uint8) for f in files]      # noqa: E731
        decode()
        dts = []
        for _ in range(3):
            t0 = time.perf_counter()
            decode()
            dts.append(time.perf_counter() - t0)
        res["pillow_decode"] = {**spread(dts), "files": DECODE_FILES, "files_per_s": DECODE_FILES / statistics.median(dts),
                                "png_bytes_mean": float(np.mean([os.path.getsize(f) for f in files]))}
    res["device_64_over_pillow_decode"] = res["device_64"]["scans_per_s"] / res["pillow_decode"]["files_per_s"]
    print(json.dumps(res["pillow_decode"]), flush=True)
    merged = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            merged = json.load(f)
    merged[f"{h}x{w}"] = res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(merged, f, indent=2, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
