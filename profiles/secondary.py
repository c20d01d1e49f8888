#!/usr/bin/env python3
"""Secondary figures ("generation throughput reported as a secondary figure"): tracked so that every
number the record quotes is one command away.

    python profiles/secondary.py [--out profiles/r04_secondary.json] [--no-trainer]
    python profiles/secondary.py --export [--out profiles/r05_export.json] [--export-shapes 64x64] [--export-images 8192]

  * generation -- Generator.forward in eval mode (siggan_g_forward; reference: utils/inference.py:136-194,
    vanilla_gan_model.py:338-371) at several batch sizes / both image sizes: us per batch, images/s, achieved TFLOP/s on
    87.06 / 414.19 MFLOP per image, and the per-kernel breakdown of the batch-64 case (MFMA launches stamped with
    hipExtLaunchKernelGGL events, one kernel at a time)
  * trainer -- GANTrainer.train end to end (reference: train_vanilla_gan_signatures.py:486-635) on a folder of synthetic PNGs:
    decode cache + device loader with augmentation + pipelined step with the next batch staged + metrics read one step late +
    tqdm / logs; images/s over whole epochs
  * export (--export, a run of its own) -- generation as its callers use it: z on the device -> uint8 bytes in host memory,
    images/s over 8192 images per shape.  Path A is the fp32 route (siggan_g_forward, 4 bytes per pixel to the host, numpy's
    (x + 1) * 127.5 / clip / truncate on one CPU thread: utils/inference.tensor_to_uint8); path B the byte route
    (siggan_g_generate_u8, 1 byte per pixel through the pinned buffer: utils/inference.generate_uint8's steps).  The two
    alternate, 5 repeats each after a warm-up, host clock, synchronised.  "stats_only": the counters alone (12 bytes per
    image reach the host, no image copy) -- what the evaluation tool needs of a sample
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
G_FLOP = {64: 87.06e6, 128: 414.19e6}


def generation(torch, Engine):
    rows = []
    for B, S, Z in ((64, 64, 100), (256, 64, 100), (1024, 64, 100), (64, 128, 128), (256, 128, 128)):
        eng = Engine(latent_dim=Z, image_size=S, max_batch=B, device="cuda:0", seed=1)
        eng.init_reference(0)
        z = torch.randn(B, Z, device="cuda:0")
        for _ in range(10):
            eng.g_forward(z, training=False)
        torch.cuda.synchronize(); t0 = time.perf_counter(); n = 200
        for _ in range(n):
            eng.g_forward(z, training=False)
        torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / n
        row = {"image_size": S, "latent": Z, "batch": B, "us_per_batch": round(dt * 1e6, 1), "images_per_s": round(B / dt, 0),
               "tflops": round(G_FLOP[S] * B / dt / 1e12, 1)}
        if B == 64:
            eng.set_mode(graph=False, overlap=False)
            eng.prof_enable(True)
            for _ in range(50):
                eng.g_forward(z, training=False)
            recs = eng.prof_read()
            eng.prof_enable(False)
            row["mfma_kernels_per_batch"] = {r["name"]: {"launches": r["launches"] / 50, "us": round(1e3 * r["ms"] / 50, 2),
                                                         "tflops": round(r["flops"] / (r["ms"] * 1e-3) / 1e12, 1)} for r in recs}
            row["mfma_us_per_batch"] = round(sum(1e3 * r["ms"] for r in recs) / 50, 1)
        rows.append(row)
        eng.close()
    return rows


def export(torch, Engine, shapes, images):
    import statistics
    from signature_gan_amd.utils.inference import _to_host_u8, tensor_to_uint8
    latent = {64: 100, 128: 128}
    rows = []
    for B, S in shapes:
        Z, nb = latent[S], max(1, images // B)
        eng = Engine(latent_dim=Z, image_size=S, max_batch=B, device="cuda:0", seed=1)
        eng.init_reference(0)
        z = torch.randn(B, Z, device="cuda:0")

        def path_a():
            return sum(int(tensor_to_uint8(eng.g_forward(z, training=False)).shape[0]) for _ in range(nb))

        def path_b():
            return sum(int(_to_host_u8(eng.g_generate_u8(z)).shape[0]) for _ in range(nb))

        def stats_only():
            st = [eng.g_generate_u8(z, threshold=0.5)[1] for _ in range(nb)]
            return int(torch.cat(st).cpu().shape[0])

        def timed(fn):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            n = fn()
            torch.cuda.synchronize()
            return n / (time.perf_counter() - t0)

        assert (tensor_to_uint8(eng.g_forward(z, training=False)) == _to_host_u8(eng.g_generate_u8(z))).all()
        for fn in (path_a, path_b, stats_only):            # warm-up: allocator, pinned buffer, weight packs
            fn()
        rates = {"a": [], "b": [], "stats": []}
        for _ in range(5):                                 # A and B alternate, so drift hits both alike
            rates["a"].append(timed(path_a)); rates["b"].append(timed(path_b)); rates["stats"].append(timed(stats_only))
        fmt = lambda v: {"median": round(statistics.median(v), 0), "min": round(min(v), 0), "max": round(max(v), 0)}
        rows.append({"image_size": S, "latent": Z, "batch": B, "images": nb * B,
                     "a_fp32_forward_plus_host_quantise_images_per_s": fmt(rates["a"]),
                     "b_uint8_kernel_plus_pinned_copy_images_per_s": fmt(rates["b"]),
                     "stats_only_images_per_s": fmt(rates["stats"]),
                     "b_over_a_median": round(statistics.median(rates["b"]) / statistics.median(rates["a"]), 2)})
        eng.close()
    return rows


def trainer(torch):
    import numpy as np
    from PIL import Image
    from signature_gan_amd.data_loader_signatures import create_data_loader
    from signature_gan_amd.train_vanilla_gan_signatures import GANTrainer, TrainingConfig
    d, run = tempfile.mkdtemp(), tempfile.mkdtemp()
    rng, n, epochs = np.random.default_rng(0), 6400, 10
    for i in range(n):
        Image.fromarray(rng.integers(0, 256, (72, 96), dtype=np.uint8), "L").save(os.path.join(d, f"s{i:05d}.png"))
    cfg = TrainingConfig(data_dir=d, epochs=epochs, batch_size=64, checkpoint_dir=run + "/ck", sample_dir=run + "/s", log_dir=run + "/l",
                         checkpoint_interval=100, sample_interval=100)
    tr = GANTrainer(cfg, device="cuda")
    t0 = time.perf_counter()
    loader = create_data_loader(d, batch_size=64, num_workers=4, image_size=64, device="cuda")
    t_load = time.perf_counter() - t0
    t0 = time.perf_counter()
    tr.train(data_loader=loader)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"images": n, "epochs": epochs, "steps_per_epoch": n // 64, "loader_build_s": round(t_load, 2), "train_s": round(dt, 2),
            "images_per_s_end_to_end": round(epochs * (n // 64) * 64 / dt, 0),
            "includes": "decode cache + device loader with augmentation + pipelined step (next batch staged) + metrics read one step late + tqdm / logs"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-trainer", action="store_true")
    ap.add_argument("--export", action="store_true", help="run the export leg alone (z on the device -> uint8 on the host)")
    ap.add_argument("--export-shapes", default="64x64,256x64,64x128", help="BATCHxSIZE,... of the export leg")
    ap.add_argument("--export-images", type=int, default=8192, help="images per timed repeat of the export leg")
    a = ap.parse_args()
    import torch
    import signature_gan_amd  # noqa: F401
    from signature_gan_amd.engine import Engine
    if a.export:
        shapes = [tuple(int(v) for v in item.split("x")) for item in a.export_shapes.split(",")]
        out = {"what": "export leg: images/s from z on the device to uint8 bytes in host memory, 1 x MI355X, fp32",
               "command": "python profiles/secondary.py --export", "export": export(torch, Engine, shapes, a.export_images)}
    else:
        out = {"what": "secondary figures, 1 x MI355X, fp32", "command": "python profiles/secondary.py",
               "generation": generation(torch, Engine)}
        if not a.no_trainer:
            out["trainer"] = trainer(torch)
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
