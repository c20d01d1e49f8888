"""Drop-in for the reference's ``generate_signatures.py`` CLI: checkpoint in -> PNG files out, with the
Generator forward on the MI355X HIP engine (``siggan_g_forward``).  Flags, file naming
(``<prefix>_%06d.png``) and the ``--seed`` semantics follow generate_signatures.py:50-249.

``--filter_by_realism`` adds the reference app's realism filter (app_vanilla_gan_signatures.py:1065-1385) to the CLI: oversample,
score every image with the checkpoint's Discriminator, keep the best ``--n_samples`` -- on the device
(utils.inference.generate_signatures_filtered).  ``--noise_scale`` and ``--threshold`` / ``--transparent`` (the app's
post-processing) also apply to a plain run.  Without the new flags, files and stdout are what they were.

``--project PATH`` and ``--morph [A B]`` go the other way, from images to latent vectors (utils.inference.project_signatures:
Adam on z around the library's eval-mode dL/dz), and build the app's second generation tab, "Morphing"
(app_vanilla_gan_signatures.py:1631-1717), on it: ``--project`` reconstructs every image of a file or directory, ``--morph A B``
projects two images and writes the strip of frames between them, ``--morph`` alone morphs between two random endpoints."""
import argparse
import json
import os
import sys
from typing import Any, Dict, Optional

import numpy as np
import torch

from .utils.inference import (generate_signatures_batch, generate_signatures_filtered, load_discriminator, load_generator,
                              load_target_images, morph_sequence, morph_strip, process_images, project_signatures)


def generate_signatures(generator, n_samples: int, output_dir: str, batch_size: int = 64,
                        device: torch.device = torch.device("cuda"), seed: Optional[int] = None,
                        prefix: str = "signature", noise_scale: float = 1.0, threshold: Optional[int] = None,
                        transparent: bool = False) -> None:
    os.makedirs(output_dir, exist_ok=True)
    print(f"Output directory: {output_dir}")
    print(f"Generating {n_samples} signatures...")
    images = generate_signatures_batch(generator=generator, n_samples=n_samples, latent_dim=generator.latent_dim,
                                       device=device, seed=seed, batch_size=batch_size, noise_scale=noise_scale)
    if threshold is not None:
        images = process_images(images, threshold=threshold, make_transparent=transparent)
    print(f"Saving {len(images)} images...")
    for i, img in enumerate(images):
        img.save(os.path.join(output_dir, f"{prefix}_{i + 1:06d}.png"), "PNG")
    print("\nGeneration complete!")
    print(f"Generated {len(images)} signatures saved to: {output_dir}")


def generate_filtered(generator, discriminator, n_samples: int, output_dir: str, batch_size: int = 64,
                      device: torch.device = torch.device("cuda"), seed: Optional[int] = None, prefix: str = "signature",
                      oversampling_ratio: float = 2.0, threshold: Optional[int] = None, transparent: bool = False,
                      noise_scale: float = 1.0) -> None:
    """The best ``n_samples`` of int(n_samples * oversampling_ratio) generated signatures by the Discriminator's score, written
    in rank order under the usual names, plus ``<prefix>_scores.json``: [{file, score}, ...] in the same order."""
    os.makedirs(output_dir, exist_ok=True)
    print(f"Output directory: {output_dir}")
    print(f"Generating {int(n_samples * oversampling_ratio)} signatures, keeping the {n_samples} most realistic...")
    images, scores = generate_signatures_filtered(generator, discriminator, n_samples, generator.latent_dim, device, seed=seed,
                                                  batch_size=batch_size, oversampling_ratio=oversampling_ratio,
                                                  noise_scale=noise_scale, threshold=threshold)
    if threshold is not None:
        images = process_images(images, threshold=threshold, make_transparent=transparent)
    print(f"Saving {len(images)} images...")
    records = []
    for i, (img, score) in enumerate(zip(images, scores)):
        name = f"{prefix}_{i + 1:06d}.png"
        img.save(os.path.join(output_dir, name), "PNG")
        records.append({"file": name, "score": score})
    with open(os.path.join(output_dir, f"{prefix}_scores.json"), "w") as f:
        json.dump(records, f, indent=2)
    print("\nGeneration complete!")
    print(f"Generated {len(images)} signatures saved to: {output_dir}")
    if scores:
        print(f"Realism scores: best {scores[0]:.4f}, worst kept {scores[-1]:.4f}")


def run_projection(generator, path: str, output_dir: str, prefix: str = "signature", steps: int = 200, lr: float = 0.05,
                   restarts: int = 1, seed: Optional[int] = None) -> None:
    """Reconstructions of the image file / the images of the directory ``path``: ``<prefix>_projection_%06d.png`` each, and
    ``<prefix>_projection.json``: [{file, reconstruction, loss, z}, ...] in the same order."""
    from PIL import Image
    os.makedirs(output_dir, exist_ok=True)
    files, targets = load_target_images(path, generator.output_size)
    print(f"Projecting {len(files)} images into the latent space ({steps} steps, {restarts} restart(s))...")
    z, recon, loss, _ = project_signatures(generator, targets, steps=steps, lr=lr, seed=seed, restarts=restarts)
    z, loss = z.cpu(), loss.cpu()
    records = []
    for i, name in enumerate(files):
        out = f"{prefix}_projection_{i + 1:06d}.png"
        Image.fromarray(recon[i], mode="L").save(os.path.join(output_dir, out), "PNG")
        records.append({"file": name, "reconstruction": out, "loss": float(loss[i]), "z": [float(v) for v in z[i]]})
    with open(os.path.join(output_dir, f"{prefix}_projection.json"), "w") as f:
        json.dump(records, f, indent=2)
    print(f"Reconstruction loss (mean squared error in [-1, 1]): best {float(loss.min()):.3e}, worst {float(loss.max()):.3e}")
    print(f"Saved {len(files)} reconstructions to: {output_dir}")


def run_morph(generator, endpoints, output_dir: str, device: torch.device, prefix: str = "signature", n_frames: int = 10,
              seed: Optional[int] = None, threshold: Optional[int] = None, transparent: bool = False, steps: int = 200,
              lr: float = 0.05, restarts: int = 1) -> None:
    """``<prefix>_morph.png``: the strip of ``n_frames`` frames between two latent endpoints -- the projections of the two image
    files in ``endpoints`` (then ``<prefix>_morph.json`` holds their files, losses and z vectors), or two N(0, 1) draws seeded
    by ``seed`` when ``endpoints`` is empty."""
    os.makedirs(output_dir, exist_ok=True)
    if endpoints:
        files, targets = [], []
        for p in endpoints:
            f, t = load_target_images(p, generator.output_size)
            if len(f) != 1:
                raise ValueError(f"--morph takes two image files, {p} holds {len(f)} images")
            files += f; targets.append(t[0])
        z, _, loss, _ = project_signatures(generator, np.stack(targets), steps=steps, lr=lr, seed=seed, restarts=restarts)
        with open(os.path.join(output_dir, f"{prefix}_morph.json"), "w") as f:
            json.dump({"files": files, "losses": [float(v) for v in loss.cpu()], "z": [[float(v) for v in row] for row in z.cpu()]},
                      f, indent=2)
        print(f"Projected the endpoints: losses {float(loss[0]):.3e}, {float(loss[1]):.3e}")
    else:
        if seed is not None:
            torch.manual_seed(seed)
            if torch.cuda.is_available():
                torch.cuda.manual_seed_all(seed)
        z = torch.cat([torch.randn(1, generator.latent_dim, device=device), torch.randn(1, generator.latent_dim, device=device)])
    frames = morph_sequence(generator, z[0:1], z[1:2], n_frames)
    morph_strip(frames, threshold=threshold, make_transparent=transparent).save(os.path.join(output_dir, f"{prefix}_morph.png"), "PNG")
    print(f"Saved a morph strip of {n_frames} frames to: {os.path.join(output_dir, prefix + '_morph.png')}")


def get_checkpoint_info(checkpoint_path: str) -> Dict[str, Any]:
    if not os.path.exists(checkpoint_path):
        return {"error": f"Checkpoint not found: {checkpoint_path}"}
    ck = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
    info: Dict[str, Any] = {"path": checkpoint_path, "type": type(ck).__name__}
    if isinstance(ck, dict):
        info["keys"] = list(ck.keys())
        for k in ("epoch", "config", "g_loss", "d_loss"):
            if k in ck:
                info[k] = ck[k]
    return info


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description="Generate synthetic signatures (MI355X HIP engine)",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--checkpoint", type=str, required=True, help="Path to the generator checkpoint file")
    p.add_argument("--n_samples", type=int, default=100, help="Number of signatures to generate")
    p.add_argument("--output_dir", type=str, default="./generated_signatures", help="Output directory")
    p.add_argument("--batch_size", type=int, default=64, help="Batch size for generation")
    p.add_argument("--seed", type=int, default=None, help="Random seed for reproducibility (optional)")
    p.add_argument("--prefix", type=str, default="signature", help="Filename prefix for generated images")
    p.add_argument("--device", type=str, default="auto", help="Device to use for inference")
    p.add_argument("--info", action="store_true", help="Display checkpoint information and exit")
    p.add_argument("--filter_by_realism", action="store_true",
                   help="Oversample, score with the checkpoint's Discriminator and keep the n_samples most realistic")
    p.add_argument("--oversampling_ratio", type=float, default=2.0, help="Signatures generated per signature kept (>= 1.0)")
    p.add_argument("--threshold", type=int, default=None, help="Binarise before scoring and saving: pixel < THRESHOLD -> 0, else 255")
    p.add_argument("--transparent", action="store_true", help="With --threshold: save RGBA with the white background transparent")
    p.add_argument("--noise_scale", type=float, default=1.0, help="Scale of the latent noise")
    p.add_argument("--morph", type=str, nargs="*", default=None, metavar="IMAGE",
                   help="Write <prefix>_morph.png, a strip of frames between two latent endpoints: the projections of two image "
                        "files, or two random draws (from --seed) when no files are given")
    p.add_argument("--morph_frames", type=int, default=10, help="Frames of the morph strip")
    p.add_argument("--project", type=str, default=None, metavar="PATH",
                   help="Project an image file, or every image of a directory, into the latent space; write the reconstructions "
                        "and <prefix>_projection.json")
    p.add_argument("--project_steps", type=int, default=200, help="Adam iterations of a projection")
    p.add_argument("--project_lr", type=float, default=0.05, help="Adam learning rate of a projection")
    p.add_argument("--project_restarts", type=int, default=1, help="Random starts per image (the lowest final loss is kept)")
    a = p.parse_args(argv)
    if a.morph is not None and len(a.morph) not in (0, 2):
        p.error("--morph takes no image files (random endpoints) or exactly two")
    if a.morph_frames < 2:
        p.error("--morph_frames must be >= 2")
    if a.project_steps < 1 or a.project_restarts < 1 or not a.project_lr > 0:
        p.error("--project_steps and --project_restarts must be >= 1, --project_lr > 0")
    if a.oversampling_ratio < 1.0:
        p.error("--oversampling_ratio must be >= 1.0")
    if a.threshold is not None and not 0 <= a.threshold <= 255:
        p.error("--threshold must be a byte value (0..255)")
    if not a.filter_by_realism and a.oversampling_ratio != 2.0:
        p.error("--oversampling_ratio needs --filter_by_realism")
    if a.transparent and a.threshold is None:
        p.error("--transparent needs --threshold")
    return a


def main(argv=None) -> None:
    a = parse_args(argv)
    device = torch.device("cuda" if a.device == "auto" else a.device)
    print(f"Using device: {device}")
    if a.info:
        print("\nCheckpoint Information:")
        for k, v in get_checkpoint_info(a.checkpoint).items():
            print(f"  {k}: {v}")
        return
    generator, _ = load_generator(a.checkpoint, device)
    if a.project is not None or a.morph is not None:
        if a.project is not None:
            run_projection(generator, a.project, a.output_dir, a.prefix, a.project_steps, a.project_lr, a.project_restarts, a.seed)
        if a.morph is not None:
            run_morph(generator, a.morph, a.output_dir, device, a.prefix, a.morph_frames, a.seed, a.threshold, a.transparent,
                      a.project_steps, a.project_lr, a.project_restarts)
        return
    if a.filter_by_realism:
        discriminator = load_discriminator(a.checkpoint, device, image_size=generator.output_size)
        if discriminator is None:
            sys.exit(f"error: {a.checkpoint} holds no discriminator_state_dict: --filter_by_realism needs the Discriminator's "
                     "weights (a full training checkpoint, not a generator-only export)")
        generate_filtered(generator, discriminator, a.n_samples, a.output_dir, a.batch_size, device, a.seed, a.prefix,
                          a.oversampling_ratio, a.threshold, a.transparent, a.noise_scale)
    else:
        generate_signatures(generator, a.n_samples, a.output_dir, a.batch_size, device, a.seed, a.prefix, a.noise_scale,
                            a.threshold, a.transparent)
    print("\n" + "=" * 50 + "\nGeneration Summary:")
    print(f"  Checkpoint: {a.checkpoint}\n  Samples generated: {a.n_samples}\n  Output directory: {a.output_dir}")
    print(f"  Seed: {a.seed if a.seed is not None else 'Random'}\n  Device: {device}\n" + "=" * 50)


if __name__ == "__main__":
    main()
