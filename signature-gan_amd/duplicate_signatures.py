"""Duplicate a folder of signatures: ``python -m signature_gan_amd.duplicate_signatures IN OUT [--copies 8] ...``.

Every image file of IN (grayscale, all of one size: 1 <= H <= 128, W a multiple of 4 in 4..128) yields ``--copies`` smooth
random warps of itself (warp.duplicate_u8: one HIP launch for the whole folder), written as ``<stem>_dupNN.png`` beside a
``duplicates.json`` that records per copy its source, draw id, affine draws, largest displacement and ink pixels before and
after.  It needs no GAN checkpoint: this is the training-free baseline beside ``generate_signatures --adapt``.  On request the
record also holds, per copy against its source, ``dtw_paired`` (--dtw [BAND]), ``ssim_paired`` (--ssim) and the verifier's
``embedding_distance`` / ``verifier_score`` (--verifier_checkpoint CKPT): the keys of generate_signatures' identity records.
Whether the copies help a verifier trained on them is not measured."""
import argparse
import json
from pathlib import Path
from typing import List, Optional

import numpy as np
import torch
from PIL import Image

from .warp import AFFINE_DRAWS, WarpSpec, draw_affine, duplicate_u8

EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff")
INK_BELOW = 128


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Smooth random warps of every signature of a folder (no checkpoint needed)")
    p.add_argument("input_dir", metavar="IN")
    p.add_argument("output_dir", metavar="OUT")
    p.add_argument("--copies", type=int, default=8, help="Variants per signature (default: 8)")
    p.add_argument("--amplitude", metavar="PX", type=float, default=2.0, help="Largest control displacement in pixels, at most 0.4 cells (default: 2)")
    p.add_argument("--cell", metavar="C", type=int, default=16, help="Pixels between control points: 8, 16 or 32 (default: 16)")
    p.add_argument("--rotate", metavar="DEG", type=float, default=0.0, help="Rotation within +-DEG degrees (default: 0)")
    p.add_argument("--slant", metavar="S", type=float, default=0.0, help="Slant within +-S pixels of x per pixel of y (default: 0)")
    p.add_argument("--scale", metavar="R", type=float, default=0.0, help="Scale within 1 +- R (default: 0)")
    p.add_argument("--shift", metavar="PX", type=float, default=0.0, help="Shift within +-PX pixels per axis (default: 0)")
    p.add_argument("--seed", metavar="N", type=int, default=0)
    p.add_argument("--verifier_checkpoint", metavar="CKPT", default=None, help="Record the verifier's embedding_distance / verifier_score against the source")
    p.add_argument("--dtw", metavar="BAND", type=int, nargs="?", const=-1, default=None, help="Record dtw_paired against the source (BAND columns; default W // 8)")
    p.add_argument("--ssim", action="store_true", help="Record ssim_paired against the source")
    p.add_argument("--device", default="cuda")
    return p


def load_folder(folder: Path):
    """(files, uint8 (N, H, W)); SystemExit with one line when the folder is empty or the sizes differ."""
    files = sorted(f for f in folder.iterdir() if f.suffix.lower() in EXTENSIONS)
    if not files:
        raise SystemExit(f"error: no image files in {folder}")
    images = [np.asarray(Image.open(f).convert("L"), dtype=np.uint8) for f in files]
    for f, a in zip(files, images):
        if a.shape != images[0].shape:
            raise SystemExit(f"error: {f.name} is {a.shape[1]}x{a.shape[0]} but {files[0].name} is {images[0].shape[1]}x{images[0].shape[0]}: "
                             "all inputs must share one size")
    return files, np.stack(images)


def verifier_records(checkpoint: str, copies_u8: torch.Tensor, sources_u8: torch.Tensor) -> List[dict]:
    """[{embedding_distance, verifier_score}]: copy i against source i (generate_signatures.identity_report's keys)."""
    from .signature_verifier_eval import load_model
    model, _ = load_model(checkpoint, copies_u8.device)
    model.eval()
    out = []
    for i in range(0, copies_u8.shape[0], model.max_images):
        e, r = model.embed_resized(copies_u8[i:i + model.max_images]), model.embed_resized(sources_u8[i:i + model.max_images])
        dist, score = (e - r).norm(dim=1).cpu(), model.compare(e, r).reshape(-1).cpu()
        out += [{"embedding_distance": float(d), "verifier_score": float(s)} for d, s in zip(dist, score)]
    return out


def main(argv: Optional[List[str]] = None) -> int:
    args = build_parser().parse_args(argv)
    try:
        spec = WarpSpec(cell=args.cell, amplitude=(args.amplitude, args.amplitude), rotate_deg=args.rotate, slant=args.slant, scale=args.scale,
                        shift_px=args.shift).check()
        if args.copies < 1:
            raise ValueError(f"copies = {args.copies} < 1")
    except ValueError as e:
        raise SystemExit(f"error: {e}")
    files, images = load_folder(Path(args.input_dir))
    n, h, w = images.shape
    device = torch.device(args.device)
    src = torch.from_numpy(images).to(device)
    try:
        out, field = duplicate_u8(src, args.copies, spec, args.seed, return_field=True)
    except ValueError as e:                                         # a size the warp does not take
        raise SystemExit(f"error: {e}")
    total = n * args.copies
    source_of = np.repeat(np.arange(n), args.copies)
    sources = src[torch.from_numpy(source_of).to(device)].contiguous()
    _, draws = draw_affine(spec, total, args.seed, (h, w))
    largest = field.abs().amax(dim=(1, 2, 3)).cpu().numpy()
    ink_before = (sources < INK_BELOW).sum(dim=(1, 2)).cpu().numpy()
    ink_after = (out < INK_BELOW).sum(dim=(1, 2)).cpu().numpy()
    extra = {}
    if args.dtw is not None:
        from .dtw import dtw_paired
        extra["dtw_paired"] = [int(v) for v in dtw_paired(out, sources, None if args.dtw < 0 else args.dtw).cpu().numpy()]
    if args.ssim:
        from .ssim import ssim_paired
        extra["ssim_paired"] = [float(v) for v in ssim_paired(out, sources).cpu().numpy()]
    identity = verifier_records(args.verifier_checkpoint, out, sources) if args.verifier_checkpoint else None

    out_dir = Path(args.output_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    host = out.cpu().numpy()
    records = []
    for r in range(total):
        i, k = divmod(r, args.copies)
        name = f"{files[i].stem}_dup{k:02d}.png"
        Image.fromarray(host[r], mode="L").save(out_dir / name)
        rec = {"file": name, "source": files[i].name, "draw_id": r, "affine": {d: float(draws[d][r]) for d in AFFINE_DRAWS},
               "max_displacement_px": float(largest[r]) / 256.0, "ink_pixels_source": int(ink_before[r]), "ink_pixels": int(ink_after[r])}
        rec.update({key: values[r] for key, values in extra.items()})
        if identity is not None:
            rec.update(identity[r])
        records.append(rec)
    report = {"input_dir": str(args.input_dir), "copies": args.copies, "seed": args.seed, "size": [h, w], "cell": spec.cell,
              "amplitude_px": args.amplitude, "rotate_deg": args.rotate, "slant": args.slant, "scale": args.scale, "shift_px": args.shift,
              "ink_below": INK_BELOW, "duplicates": records}
    with open(out_dir / "duplicates.json", "w") as f:
        json.dump(report, f, indent=2)
    print(f"Wrote {total} duplicates of {n} signatures to: {out_dir}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
