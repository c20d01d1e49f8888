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
projects two images and writes the strip of frames between them, ``--morph`` alone morphs between two random endpoints.

``--refine_by_realism`` is the filter's counterpart that discards nothing: every latent vector is moved up the Discriminator's
score for a few Adam steps (utils.inference.generate_signatures_refined) and ``<prefix>_refine.json`` records each image's score
before and after.  ``--project_realism_weight`` / ``--project_prior_weight`` add the same terms to a projection.

``--adapt PATH`` changes the model instead of the latent vectors (utils.inference.adapt_generator: the images of PATH are
projected to pivots, then Adam runs on the Generator's weights around the library's eval-mode dL/dtheta); ``--n_samples``
signatures are then generated at z = pivot[i mod N] + S * randn with S = ``--adapt_sigma`` (default 0.25 * ``--noise_scale``),
``<prefix>_adapt.json`` records each target's loss before and after, and ``--adapt_save CKPT`` keeps the adapted weights.

``--despeckle [MIN_AREA]`` cleans every generated signature on the device before it is written (components.despeckle_u8): an
ink component (byte < ``--threshold``, 128 without it; 8-connected) of fewer than MIN_AREA pixels becomes white, every other
byte stays.  It applies to the plain run, ``--filter_by_realism`` (the pool is cleaned before it is scored, so a score belongs
to the file it stands beside), ``--refine_by_realism`` and ``--adapt``; projections and morph strips are left alone.  What
was removed is recorded as ``despeckle: {min_area, threshold, connectivity, removed_components, removed_pixels}``: in
``<prefix>_despeckle.json`` for a plain run, as a key of ``<prefix>_adapt.json``, and in ``<prefix>_scores.json`` /
``<prefix>_refine.json``, which then are ``{"despeckle": {...}, "records": [...]}`` instead of the bare list.

``--pen_width W`` (1..9; the plain run only) redraws every generated signature at one pen width on the device before it is
written (strokes.restroke_u8): the image is thinned to its centre line (ink is byte < ``--threshold``, 128 without it) and the
line is drawn again, ink 0 on paper 255, with a disc of squared radius (W - 1)^2 // 4.  ``--despeckle`` given as well runs
first.  ``<prefix>_pen_width.json`` records W, the radius, the threshold and the mean pen width along the centre line before
and after.

``--filter_by_realism --diverse`` (with ``--verifier_checkpoint``) selects for diversity instead of taking the top of the
ranking (utils.inference.generate_signatures_diverse): among the ``--diverse_keep_ratio`` most realistic signatures of the pool
it picks, greedily, those that lie farthest apart in the Siamese verifier's embedding space (utils.diverse.select_diverse, on
the device).  ``--diverse_real_dir DIR --diverse_memorisation_ratio R`` bars near copies of the real signatures in DIR,
``--diverse_existing_dir DIR`` keeps the picks away from a synthetic set that exists already, ``--diverse_min_separation S``
stops the run once nothing new is at least S away from what is kept -- fewer than ``--n_samples`` files may then be written.
The files are in pick order, ``<prefix>_scores.json`` is the filter's, and ``<prefix>_diverse.json`` is the report: every pick's
pool index, score and gain, and the nearest-neighbour distances inside this selection beside those of the plain top-n.  Whether
a verifier trained on such a set is more accurate is not measured.

``--edit`` changes the shape of every generated signature before it is written (utils.inference.generate_signatures_edited: Adam
on z around the ink moments' gradient, shape.shape_grad, on the device): ``--edit_slant_delta D`` adds D to the slant (the shear
coefficient; NEGATIVE leans to the right, because the image's v axis points down), ``--edit_size_scale R`` makes the signature R
times as large in the frame, ``--edit_boldness_scale R`` multiplies its ink mass, ``--edit_shift DX DY`` moves its centre (in
units of the image side, DY downwards); ``--edit_keep W`` weighs staying the same signature.  The latent vectors are the ones
the plain run draws for the same ``--seed``, so the two runs' files pair up.  ``<prefix>_edit.json`` records, per file, the
features before, the targets, the features after and the objective before and after.  Whether an edit reaches its target
depends on the checkpoint, and whether edited signatures help a verifier's training is not measured.

``--adapt PATH --adapt_preprocess`` and ``--project PATH --project_preprocess`` take raw scans: every file goes through
preprocess_signatures.preprocess_single_image at the checkpoint's size (denoise, validate, crop, area resize, centre, CLAHE on
the device) instead of the plain decode-and-resize, the preprocessed targets are written as ``<prefix>_target_%06d.png`` and
named in the JSON report; a scan that preprocessing rejects ends the run with an error."""
import argparse
import json
import os
import sys
from typing import Any, Dict, Optional

import numpy as np
import torch

from .utils.inference import (Despeckle, PenWidth, generate_signatures_batch, generate_signatures_diverse, generate_signatures_filtered,
                              generate_signatures_edited, generate_signatures_refined,
                              load_discriminator, load_generator, load_target_images, morph_sequence, morph_strip, process_images,
                              project_signatures)


def generate_signatures(generator, n_samples: int, output_dir: str, batch_size: int = 64,
                        device: torch.device = torch.device("cuda"), seed: Optional[int] = None,
                        prefix: str = "signature", noise_scale: float = 1.0, threshold: Optional[int] = None,
                        transparent: bool = False, despeckle: Optional[Despeckle] = None,
                        pen_width: Optional[PenWidth] = None) -> None:
    os.makedirs(output_dir, exist_ok=True)
    print(f"Output directory: {output_dir}")
    print(f"Generating {n_samples} signatures...")
    images = generate_signatures_batch(generator=generator, n_samples=n_samples, latent_dim=generator.latent_dim,
                                       device=device, seed=seed, batch_size=batch_size, noise_scale=noise_scale,
                                       **with_despeckle(despeckle), **with_pen_width(pen_width))
    if threshold is not None:
        images = process_images(images, threshold=threshold, make_transparent=transparent)
    print(f"Saving {len(images)} images...")
    for i, img in enumerate(images):
        img.save(os.path.join(output_dir, f"{prefix}_{i + 1:06d}.png"), "PNG")
    if despeckle is not None:
        with open(os.path.join(output_dir, f"{prefix}_despeckle.json"), "w") as f:
            json.dump({"despeckle": despeckle.report()}, f, indent=2)
        print_despeckle(despeckle)
    if pen_width is not None:
        r = pen_width.report()
        with open(os.path.join(output_dir, f"{prefix}_pen_width.json"), "w") as f:
            json.dump(r, f, indent=2)
        print(f"Pen width: redrawn at {r['pen_width']} px (radius^2 {r['radius2']}); mean width along the centre line "
              f"{r['mean_width_before']} before, {r['mean_width_after']} after")
    print("\nGeneration complete!")
    print(f"Generated {len(images)} signatures saved to: {output_dir}")


def with_despeckle(despeckle: Optional[Despeckle]) -> Dict[str, Any]:
    """The keyword a generation call gets: none at all without --despeckle, so such a call is what it was."""
    return {} if despeckle is None else {"despeckle": despeckle}


def with_pen_width(pen_width: Optional[PenWidth]) -> Dict[str, Any]:
    """Likewise for --pen_width."""
    return {} if pen_width is None else {"pen_width": pen_width}


def print_despeckle(despeckle: Despeckle) -> None:
    r = despeckle.report()
    print(f"Despeckle: removed {r['removed_components']} components ({r['removed_pixels']} pixels) smaller than {r['min_area']} pixels")


def records_json(records, despeckle: Optional[Despeckle]):
    """What <prefix>_scores.json / <prefix>_refine.json hold: the bare list, or with --despeckle the list beside its report."""
    return records if despeckle is None else {"despeckle": despeckle.report(), "records": records}


def generate_filtered(generator, discriminator, n_samples: int, output_dir: str, batch_size: int = 64,
                      device: torch.device = torch.device("cuda"), seed: Optional[int] = None, prefix: str = "signature",
                      oversampling_ratio: float = 2.0, threshold: Optional[int] = None, transparent: bool = False,
                      noise_scale: float = 1.0, despeckle: Optional[Despeckle] = None) -> None:
    """The best ``n_samples`` of int(n_samples * oversampling_ratio) generated signatures by the Discriminator's score, written
    in rank order under the usual names, plus ``<prefix>_scores.json``: [{file, score}, ...] in the same order."""
    os.makedirs(output_dir, exist_ok=True)
    print(f"Output directory: {output_dir}")
    print(f"Generating {int(n_samples * oversampling_ratio)} signatures, keeping the {n_samples} most realistic...")
    images, scores = generate_signatures_filtered(generator, discriminator, n_samples, generator.latent_dim, device, seed=seed,
                                                  batch_size=batch_size, oversampling_ratio=oversampling_ratio,
                                                  noise_scale=noise_scale, threshold=threshold, **with_despeckle(despeckle))
    if threshold is not None:
        images = process_images(images, threshold=threshold, make_transparent=transparent)
    print(f"Saving {len(images)} images...")
    records = []
    for i, (img, score) in enumerate(zip(images, scores)):
        name = f"{prefix}_{i + 1:06d}.png"
        img.save(os.path.join(output_dir, name), "PNG")
        records.append({"file": name, "score": score})
    with open(os.path.join(output_dir, f"{prefix}_scores.json"), "w") as f:
        json.dump(records_json(records, despeckle), f, indent=2)
    if despeckle is not None:
        print_despeckle(despeckle)
    print("\nGeneration complete!")
    print(f"Generated {len(images)} signatures saved to: {output_dir}")
    if scores:
        print(f"Realism scores: best {scores[0]:.4f}, worst kept {scores[-1]:.4f}")


def generate_diverse(generator, discriminator, verifier, n_samples: int, output_dir: str, batch_size: int = 64,
                     device: torch.device = torch.device("cuda"), seed: Optional[int] = None, prefix: str = "signature",
                     oversampling_ratio: float = 2.0, threshold: Optional[int] = None, transparent: bool = False,
                     noise_scale: float = 1.0, despeckle: Optional[Despeckle] = None, keep_ratio: float = 0.5,
                     real_dir: Optional[str] = None, memorisation_ratio: Optional[float] = None, existing_dir: Optional[str] = None,
                     min_separation: float = 0.0) -> None:
    """Up to ``n_samples`` of int(n_samples * oversampling_ratio) generated signatures, chosen for diversity among the
    ``keep_ratio`` most realistic (utils.inference.generate_signatures_diverse), written in pick order under the usual names,
    plus ``<prefix>_scores.json`` as generate_filtered writes it and ``<prefix>_diverse.json``, the selection's report."""
    os.makedirs(output_dir, exist_ok=True)
    print(f"Output directory: {output_dir}")
    print(f"Generating {int(n_samples * oversampling_ratio)} signatures, selecting up to {n_samples} for diversity...")
    size = generator.output_size
    real = load_target_images(real_dir, size)[1] if real_dir is not None else None
    existing = load_target_images(existing_dir, size)[1] if existing_dir is not None else None
    images, scores, report = generate_signatures_diverse(
        generator, discriminator, verifier, n_samples, generator.latent_dim, device, seed=seed, batch_size=batch_size,
        oversampling_ratio=oversampling_ratio, keep_ratio=keep_ratio, noise_scale=noise_scale, threshold=threshold, real_u8=real,
        memorisation_ratio=memorisation_ratio, existing_u8=existing, min_separation=min_separation, verifier_resize=size != 64,
        **with_despeckle(despeckle))
    if threshold is not None:
        images = process_images(images, threshold=threshold, make_transparent=transparent)
    print(f"Saving {len(images)} images...")
    records = []
    for i, (img, score) in enumerate(zip(images, scores)):
        name = f"{prefix}_{i + 1:06d}.png"
        img.save(os.path.join(output_dir, name), "PNG")
        records.append({"file": name, "score": score})
        report["picks"][i]["file"] = name
    with open(os.path.join(output_dir, f"{prefix}_scores.json"), "w") as f:
        json.dump(records_json(records, despeckle), f, indent=2)
    with open(os.path.join(output_dir, f"{prefix}_diverse.json"), "w") as f:
        json.dump(report, f, indent=2)
    if despeckle is not None:
        print_despeckle(despeckle)
    print("\nGeneration complete!")
    print(f"Generated {len(images)} signatures saved to: {output_dir}")
    if len(images) < n_samples:
        print(f"Selected {len(images)} of the {n_samples} signatures asked for (stopped by: {report['stopped_by']})")
    d, t = report["diverse"], report["top_n"]
    if d["min_nn_distance"] is not None and t["min_nn_distance"] is not None:
        print(f"Nearest-neighbour distance inside the selection: min {d['min_nn_distance']:.4f}, mean {d['mean_nn_distance']:.4f} "
              f"(top-n by realism: min {t['min_nn_distance']:.4f}, mean {t['mean_nn_distance']:.4f})")
    if d["mean_realism"] is not None and t["mean_realism"] is not None:
        print(f"Mean realism: {d['mean_realism']:.4f} (top-n by realism: {t['mean_realism']:.4f})")


def generate_refined(generator, discriminator, n_samples: int, output_dir: str, batch_size: int = 64,
                     device: torch.device = torch.device("cuda"), seed: Optional[int] = None, prefix: str = "signature",
                     steps: int = 20, lr: float = 0.02, prior_weight: float = 0.0, threshold: Optional[int] = None,
                     transparent: bool = False, noise_scale: float = 1.0, despeckle: Optional[Despeckle] = None) -> None:
    """``n_samples`` generated signatures whose latent vectors were refined by the Discriminator's score, written in generation
    order under the usual names, plus ``<prefix>_refine.json``: [{file, before, after}, ...] in the same order."""
    os.makedirs(output_dir, exist_ok=True)
    print(f"Output directory: {output_dir}")
    print(f"Generating {n_samples} signatures, refining each for {steps} steps by the Discriminator's score...")
    images, after, before = generate_signatures_refined(generator, discriminator, n_samples, generator.latent_dim, device, seed=seed,
                                                        batch_size=batch_size, noise_scale=noise_scale, steps=steps, lr=lr,
                                                        prior_weight=prior_weight, threshold=threshold, **with_despeckle(despeckle))
    if threshold is not None:
        images = process_images(images, threshold=threshold, make_transparent=transparent)
    print(f"Saving {len(images)} images...")
    records = []
    for i, (img, b, a) in enumerate(zip(images, before, after)):
        name = f"{prefix}_{i + 1:06d}.png"
        img.save(os.path.join(output_dir, name), "PNG")
        records.append({"file": name, "before": b, "after": a})
    with open(os.path.join(output_dir, f"{prefix}_refine.json"), "w") as f:
        json.dump(records_json(records, despeckle), f, indent=2)
    if despeckle is not None:
        print_despeckle(despeckle)
    print("\nGeneration complete!")
    print(f"Generated {len(images)} signatures saved to: {output_dir}")
    if after:
        print(f"Realism scores: mean {sum(before) / len(before):.4f} before, {sum(after) / len(after):.4f} after")


def generate_edited(generator, discriminator, n_samples: int, output_dir: str, batch_size: int = 64,
                    device: torch.device = torch.device("cuda"), seed: Optional[int] = None, prefix: str = "signature",
                    threshold: Optional[int] = None, transparent: bool = False, noise_scale: float = 1.0,
                    edit: Optional[Dict[str, Any]] = None) -> None:
    """``n_samples`` generated signatures whose latent vectors were edited (``edit``: utils.inference.edit_latents' keyword
    arguments), written in generation order under the usual names, plus ``<prefix>_edit.json``: {edit: the settings, records:
    [{file, before, targets, after, objective_before, objective_after}, ...]} in the same order."""
    os.makedirs(output_dir, exist_ok=True)
    print(f"Output directory: {output_dir}")
    print(f"Generating {n_samples} signatures, editing each for {edit['steps']} steps...")
    images, records = generate_signatures_edited(generator, n_samples, generator.latent_dim, device, seed=seed, batch_size=batch_size,
                                                 noise_scale=noise_scale, threshold=threshold, discriminator=discriminator, **edit)
    if threshold is not None:
        images = process_images(images, threshold=threshold, make_transparent=transparent)
    print(f"Saving {len(images)} images...")
    for i, (img, rec) in enumerate(zip(images, records)):
        name = f"{prefix}_{i + 1:06d}.png"
        img.save(os.path.join(output_dir, name), "PNG")
        records[i] = {"file": name, **rec}
    with open(os.path.join(output_dir, f"{prefix}_edit.json"), "w") as f:
        json.dump({"edit": {k: (list(v) if isinstance(v, tuple) else v) for k, v in edit.items()}, "records": records}, f, indent=2)
    print("\nGeneration complete!")
    print(f"Generated {len(images)} signatures saved to: {output_dir}")
    for name in sorted({k for r in records for k in r["targets"]}):
        mean = lambda key: sum(r[key][name] for r in records) / len(records)              # noqa: E731
        print(f"  {name}: mean {mean('before'):.5f} before, {mean('after'):.5f} after (target {mean('targets'):.5f})")


def run_projection(generator, path: str, output_dir: str, prefix: str = "signature", steps: int = 200, lr: float = 0.05,
                   restarts: int = 1, seed: Optional[int] = None, discriminator=None, realism_weight: float = 0.0,
                   prior_weight: float = 0.0, verifier=None, identity_weight: float = 0.0,
                   identity_score_weight: float = 0.0, verifier_resize: bool = False, project_ssim: bool = False,
                   preprocess: bool = False) -> None:
    """Reconstructions of the image file / the images of the directory ``path``: ``<prefix>_projection_%06d.png`` each, and
    ``<prefix>_projection.json``: [{file, reconstruction, loss, z}, ...] in the same order; with ``realism_weight`` > 0 every
    record also holds ``realism``, the Discriminator's score of the reconstruction.  With a ``verifier`` every record holds
    ``identity``: {embedding_distance, verifier_score} of G(z) against the target at the returned z, and
    ``identity_pixel_only``: the same two numbers for the projection without the identity term (what the term bought).
    ``verifier_resize``: the verifier reads targets and reconstructions through the device resize to 64x64 (a 128x128 Generator).
    ``project_ssim``: every record also holds ``ssim``, the structural similarity (ssim.ssim_paired) of the target's bytes and
    the reconstruction's bytes as written.  ``preprocess``: the files are raw scans; every target goes through
    load_preprocessed_targets instead of the plain load, is written as ``<prefix>_target_%06d.png`` and named in its record
    under ``preprocessed_target``."""
    from PIL import Image
    os.makedirs(output_dir, exist_ok=True)
    files, targets = load_preprocessed_targets(path, generator.output_size) if preprocess else load_target_images(path, generator.output_size)
    target_names = save_preprocessed_targets(targets, output_dir, prefix) if preprocess else None
    print(f"Projecting {len(files)} images into the latent space ({steps} steps, {restarts} restart(s))...")
    kw = dict(steps=steps, lr=lr, seed=seed, restarts=restarts, discriminator=discriminator, realism_weight=realism_weight,
              prior_weight=prior_weight)
    z, recon, loss, _ = project_signatures(generator, targets, verifier=verifier, identity_weight=identity_weight,
                                           identity_score_weight=identity_score_weight, verifier_resize=verifier_resize, **kw)
    identity = pixel_only = None
    if verifier is not None:
        identity = identity_report(generator, verifier, targets, z, verifier_resize)
        pixel_only = identity
        if identity_weight > 0 or identity_score_weight > 0:
            pixel_only = identity_report(generator, verifier, targets, project_signatures(generator, targets, **kw)[0], verifier_resize)
    realism = None
    if realism_weight > 0:
        mb = generator._require_engine().max_batch
        realism = torch.cat([discriminator.score_u8(torch.from_numpy(recon[i:i + mb]).to(z.device)) for i in range(0, len(recon), mb)]).cpu()
    similarity = None
    if project_ssim:
        from .ssim import ssim_paired
        similarity = ssim_paired(torch.as_tensor(targets).to(z.device).contiguous(),
                                 torch.from_numpy(recon).to(z.device).contiguous()).cpu()
    z, loss = z.cpu(), loss.cpu()
    records = []
    for i, name in enumerate(files):
        out = f"{prefix}_projection_{i + 1:06d}.png"
        Image.fromarray(recon[i], mode="L").save(os.path.join(output_dir, out), "PNG")
        records.append({"file": name, "reconstruction": out, "loss": float(loss[i]), "z": [float(v) for v in z[i]]})
        if realism is not None:
            records[-1]["realism"] = float(realism[i])
        if identity is not None:
            records[-1]["identity"] = identity[i]
            records[-1]["identity_pixel_only"] = pixel_only[i]
        if similarity is not None:
            records[-1]["ssim"] = float(similarity[i])
        if target_names is not None:
            records[-1]["preprocessed_target"] = target_names[i]
    with open(os.path.join(output_dir, f"{prefix}_projection.json"), "w") as f:
        json.dump(records, f, indent=2)
    print(f"Reconstruction loss (mean squared error in [-1, 1]): best {float(loss.min()):.3e}, worst {float(loss.max()):.3e}")
    print(f"Saved {len(files)} reconstructions to: {output_dir}")


def identity_report(generator, verifier, targets_u8, z, resize: bool = False):
    """[{embedding_distance, verifier_score}, ...]: the verifier's view of G(z[i]) against target i -- the Euclidean distance of
    the two unit embeddings and the head's similarity -- on the fp32 images of the eval-mode Generator.  ``resize``: both go
    through the device resize to 64x64 first (SiameseNetwork.embed_resized)."""
    embed_f32, embed_u8 = (verifier.embed_resized,) * 2 if resize else (verifier.forward_one, verifier.embed_u8)
    eng = generator._require_engine()
    t = torch.as_tensor(targets_u8).to(z.device).contiguous()
    step = min(eng.max_batch, verifier.max_images)
    out = []
    for i in range(0, z.shape[0], step):
        e = embed_f32(eng.g_forward(z[i:i + step].contiguous(), training=False))
        r = embed_u8(t[i:i + step])
        dist, score = (e - r).norm(dim=1).cpu(), verifier.compare(e, r).reshape(-1).cpu()
        out += [{"embedding_distance": float(d), "verifier_score": float(s)} for d, s in zip(dist, score)]
    return out


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


def run_adapt(generator, path: str, output_dir: str, device: torch.device, n_samples: int, prefix: str = "signature",
              steps: int = 100, lr: float = 1e-4, first_layer: int = 0, anchor_weight: float = 0.0, discriminator=None,
              realism_weight: float = 0.0, sigma: float = 0.25, save: Optional[str] = None, seed: Optional[int] = None,
              project_steps: int = 200, project_lr: float = 0.05, project_restarts: int = 1, threshold: Optional[int] = None,
              transparent: bool = False, config: Optional[Dict[str, Any]] = None, despeckle: Optional[Despeckle] = None,
              preprocess: bool = False) -> None:
    """Adapt the Generator to the image file / the images of the directory ``path`` (utils.inference.adapt_generator: project
    them to pivots, then Adam on the weights of layers >= ``first_layer``), then write ``n_samples`` signatures
    ``<prefix>_%06d.png`` generated at z = pivot[i mod N] + sigma * randn (seeded by ``seed``) and ``<prefix>_adapt.json``:
    {steps, lr, first_layer, anchor_weight, realism_weight, sigma, trainable: [keys], targets: [{file, loss_before,
    loss_after}, ...]}.  ``save``: also a checkpoint {generator_state_dict, config} of the adapted weights that
    load_generator reads back.  ``preprocess``: the files are raw scans; every target goes through load_preprocessed_targets
    instead of the plain load, is written as ``<prefix>_target_%06d.png`` and named in its entry of ``targets`` under
    ``preprocessed_target``, and the report says ``preprocess: true``."""
    from PIL import Image
    from .utils.inference import adapt_generator, generate_uint8
    os.makedirs(output_dir, exist_ok=True)
    files, targets = load_preprocessed_targets(path, generator.output_size) if preprocess else load_target_images(path, generator.output_size)
    target_names = save_preprocessed_targets(targets, output_dir, prefix) if preprocess else None
    print(f"Adapting the Generator to {len(files)} signatures ({steps} steps, lr {lr:g}, layers >= {first_layer})...")
    res = adapt_generator(generator, targets, steps=steps, lr=lr, first_layer=first_layer, anchor_weight=anchor_weight,
                          discriminator=discriminator, realism_weight=realism_weight, seed=seed,
                          project_kwargs=dict(steps=project_steps, lr=project_lr, restarts=project_restarts))
    before, after = res["loss_before"].cpu(), res["loss_after"].cpu()
    gen = None if seed is None else torch.Generator().manual_seed(int(seed))
    pivots, n = res["z"], len(files)
    images, mb = [], generator._require_engine().max_batch
    for i0 in range(0, n_samples, mb):
        idx = torch.arange(i0, min(i0 + mb, n_samples)) % n
        noise = torch.randn(len(idx), generator.latent_dim, generator=gen).to(device)
        images += [Image.fromarray(arr, mode="L") for arr in generate_uint8(generator, (pivots[idx.to(device)] + sigma * noise).contiguous(),
                                                                              **with_despeckle(despeckle))]
    if threshold is not None:
        images = process_images(images, threshold=threshold, make_transparent=transparent)
    for i, img in enumerate(images):
        img.save(os.path.join(output_dir, f"{prefix}_{i + 1:06d}.png"), "PNG")
    report = {"steps": steps, "lr": lr, "first_layer": first_layer, "anchor_weight": anchor_weight, "realism_weight": realism_weight,
              "sigma": sigma, "trainable": res["trainable"],
              "targets": [{"file": f, "loss_before": float(before[i]), "loss_after": float(after[i])} for i, f in enumerate(files)]}
    if despeckle is not None:
        report["despeckle"] = despeckle.report()
        print_despeckle(despeckle)
    if target_names is not None:
        report["preprocess"] = True
        for entry, name in zip(report["targets"], target_names):
            entry["preprocessed_target"] = name
    with open(os.path.join(output_dir, f"{prefix}_adapt.json"), "w") as f:
        json.dump(report, f, indent=2)
    if save:
        cfg = dict(config or {})
        cfg.update(latent_dim=generator.latent_dim, image_size=generator.output_size, image_channels=generator.output_channels)
        torch.save({"generator_state_dict": {k: v.detach().cpu().clone() for k, v in generator.state_dict().items()}, "config": cfg}, save)
        print(f"Saved the adapted Generator to: {save}")
    print(f"Objective per target: mean {float(before.mean()):.3e} before, {float(after.mean()):.3e} after")
    print(f"Saved {len(images)} signatures to: {output_dir}")


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


LATER_DEFAULTS = dict(refine_by_realism=False, refine_steps=20, refine_lr=0.02, refine_prior=0.0, project_realism_weight=0.0,
                      project_prior_weight=0.0)


def opt(a: argparse.Namespace, name: str):
    """A flag of LATER_DEFAULTS: its value on the command line, else its default."""
    return getattr(a, name, LATER_DEFAULTS[name])


# the adaptation flags, added later still and kept out of the namespace the same way (adapt_sigma None: 0.25 * --noise_scale)
ADAPT_DEFAULTS = dict(adapt=None, adapt_steps=100, adapt_lr=1e-4, adapt_first_layer=0, adapt_anchor=0.0, adapt_realism_weight=0.0,
                      adapt_sigma=None, adapt_save=None)


# the identity flags of a projection, kept out of the namespace the same way
IDENTITY_DEFAULTS = dict(verifier_checkpoint=None, project_identity_weight=0.0, project_identity_score_weight=0.0,
                         project_identity_resize=False)


# --despeckle, kept out of the namespace the same way: absent = off, "auto" = components.default_min_area, else MIN_AREA
DESPECKLE_DEFAULTS = dict(despeckle=None)


def despeckle_opt(a: argparse.Namespace) -> Optional[Despeckle]:
    """The Despeckle of a command line with --despeckle (its ink threshold is --threshold, 128 without it), else None."""
    v = getattr(a, "despeckle", DESPECKLE_DEFAULTS["despeckle"])
    if v is None:
        return None
    return Despeckle(None if v == "auto" else v, 128 if a.threshold is None else a.threshold)


# --pen_width, kept out of the namespace the same way: absent = off
PEN_WIDTH_DEFAULTS = dict(pen_width=None)


def pen_width_opt(a: argparse.Namespace) -> Optional[PenWidth]:
    """The PenWidth of a command line with --pen_width (its ink threshold is --threshold, 128 without it), else None."""
    v = getattr(a, "pen_width", PEN_WIDTH_DEFAULTS["pen_width"])
    if v is None:
        return None
    return PenWidth(v, 128 if a.threshold is None else a.threshold)


# --project_ssim, kept out of the namespace the same way
PROJECT_SSIM_DEFAULTS = dict(project_ssim=False)


def project_ssim_opt(a: argparse.Namespace) -> bool:
    return getattr(a, "project_ssim", PROJECT_SSIM_DEFAULTS["project_ssim"])


# --adapt_preprocess / --project_preprocess, kept out of the namespace the same way
PREPROCESS_DEFAULTS = dict(adapt_preprocess=False, project_preprocess=False)


def preprocess_opt(a: argparse.Namespace, name: str) -> bool:
    """A flag of PREPROCESS_DEFAULTS: its value on the command line, else its default."""
    return getattr(a, name, PREPROCESS_DEFAULTS[name])


def load_preprocessed_targets(path: str, image_size: int, device=None):
    """load_target_images for raw scans: the same files in the same order, each through
    preprocess_signatures.preprocess_single_image at the checkpoint's size (denoise, validate, crop, resize, centre, CLAHE on
    the device) instead of the plain decode-and-resize.  A scan that preprocessing rejects raises: a target cannot be dropped
    silently."""
    from pathlib import Path
    from .data_loader_signatures import SignatureDataset
    from .preprocess_signatures import preprocess_single_image
    p = Path(path)
    if not p.exists():
        raise FileNotFoundError(f"no such image file or directory: {path}")
    ds = SignatureDataset(p if p.is_dir() else p.parent)
    if not p.is_dir():
        ds.image_paths = [p]
    if len(ds) == 0:
        raise ValueError(f"No images found in {path}")
    names, out = [], []
    for i in range(len(ds)):
        f = ds.get_image_path(i)
        arr = preprocess_single_image(f, (image_size, image_size), normalize=False, device=device)
        if arr is None:
            raise ValueError(f"preprocessing rejected {f}: unreadable, outside 16..1024 pixels a side, blank, or degenerate")
        names.append(os.path.basename(str(f))); out.append(arr)
    return names, np.stack(out)


def save_preprocessed_targets(targets, output_dir: str, prefix: str):
    """``<prefix>_target_%06d.png`` per preprocessed target; returns the names."""
    from PIL import Image
    names = [f"{prefix}_target_{i + 1:06d}.png" for i in range(len(targets))]
    for name, t in zip(names, targets):
        Image.fromarray(t, mode="L").save(os.path.join(output_dir, name), "PNG")
    return names


# the --diverse flags, kept out of the namespace the same way
DIVERSE_DEFAULTS = dict(diverse=False, diverse_keep_ratio=0.5, diverse_real_dir=None, diverse_memorisation_ratio=None,
                        diverse_existing_dir=None, diverse_min_separation=0.0)


def diverse_opt(a: argparse.Namespace, name: str):
    """A flag of DIVERSE_DEFAULTS: its value on the command line, else its default."""
    return getattr(a, name, DIVERSE_DEFAULTS[name])


# the --edit flags, kept out of the namespace the same way
EDIT_DEFAULTS = dict(edit=False, edit_slant_delta=0.0, edit_size_scale=1.0, edit_boldness_scale=1.0, edit_shift=(0.0, 0.0),
                     edit_steps=30, edit_lr=0.02, edit_keep=1.0, edit_realism_weight=0.0)


def edit_opt(a: argparse.Namespace, name: str):
    """A flag of EDIT_DEFAULTS: its value on the command line, else its default."""
    return getattr(a, name, EDIT_DEFAULTS[name])


def edit_kwargs(a: argparse.Namespace) -> Dict[str, Any]:
    """utils.inference.edit_latents' keyword arguments of a command line with --edit."""
    return dict(slant_delta=edit_opt(a, "edit_slant_delta"), size_scale=edit_opt(a, "edit_size_scale"),
                boldness_scale=edit_opt(a, "edit_boldness_scale"), shift=tuple(edit_opt(a, "edit_shift")),
                steps=edit_opt(a, "edit_steps"), lr=edit_opt(a, "edit_lr"), keep_weight=edit_opt(a, "edit_keep"),
                realism_weight=edit_opt(a, "edit_realism_weight"))


def identity_opt(a: argparse.Namespace, name: str):
    """A flag of IDENTITY_DEFAULTS: its value on the command line, else its default."""
    return getattr(a, name, IDENTITY_DEFAULTS[name])


def adapt_opt(a: argparse.Namespace, name: str):
    """A flag of ADAPT_DEFAULTS: its value on the command line, else its default."""
    return getattr(a, name, ADAPT_DEFAULTS[name])


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
    # (the refinement flags appear in the namespace only when given -- LATER_DEFAULTS holds their defaults, opt() reads them --
    #  so the namespace of a command line without them is what it was before they existed)
    later = dict(default=argparse.SUPPRESS)
    p.add_argument("--refine_by_realism", action="store_true", **later,
                   help="Refine every latent vector by the checkpoint's Discriminator's score (Adam on z) before generating; "
                        "write <prefix>_refine.json with each image's score before and after")
    p.add_argument("--refine_steps", type=int, **later, help="Adam iterations of a refinement (default: 20)")
    p.add_argument("--refine_lr", type=float, **later, help="Adam learning rate of a refinement (default: 0.02)")
    p.add_argument("--refine_prior", type=float, **later, help="Weight of the prior term 0.5 * mean(z^2) of a refinement (default: 0)")
    p.add_argument("--project_realism_weight", type=float, **later,
                   help="With --project: weight of -log D(G(z)) beside the pixel error; needs the checkpoint's Discriminator (default: 0)")
    p.add_argument("--project_prior_weight", type=float, **later,
                   help="With --project: weight of the prior term 0.5 * mean(z^2) (default: 0)")
    p.add_argument("--verifier_checkpoint", type=str, metavar="CKPT", **later,
                   help="With --project: the Siamese verifier's checkpoint; <prefix>_projection.json then records the verifier's "
                        "embedding distance and score of every reconstruction against its target")
    p.add_argument("--project_identity_weight", type=float, **later,
                   help="With --project and --verifier_checkpoint: weight of 0.5 * |e(G(z)) - e(target)|^2 beside the pixel error (default: 0)")
    p.add_argument("--project_identity_score_weight", type=float, **later,
                   help="With --project and --verifier_checkpoint: weight of -log verifier_score(G(z), target) (default: 0)")
    p.add_argument("--project_identity_resize", action="store_true", **later,
                   help="With --project and --verifier_checkpoint: the verifier reads targets and G(z) through the device resize to "
                        "64x64 (Pillow's antialiased bilinear filter), so a 128x128 Generator can be used (default: off)")
    p.add_argument("--adapt", type=str, metavar="PATH", **later,
                   help="Adapt the Generator's weights to an image file, or the images of a directory (pivotal tuning: project, then "
                        "Adam on the weights), generate n_samples signatures near the pivots and write <prefix>_adapt.json")
    p.add_argument("--adapt_steps", type=int, **later, help="Adam iterations of an adaptation (default: 100)")
    p.add_argument("--adapt_lr", type=float, **later, help="Adam learning rate of an adaptation (default: 1e-4)")
    p.add_argument("--adapt_first_layer", type=int, **later,
                   help="First trained layer: 0 fc, 1..L the upsample blocks, L+1 the final conv; the layers below stay frozen (default: 0)")
    p.add_argument("--adapt_anchor", type=float, **later, help="Weight of the pull 0.5 * |theta - theta0|^2 back to the checkpoint (default: 0)")
    p.add_argument("--adapt_realism_weight", type=float, **later,
                   help="Weight of -log D(G(z)) beside the pixel error; needs the checkpoint's Discriminator (default: 0)")
    p.add_argument("--adapt_sigma", type=float, **later,
                   help="Signatures are generated at z = pivot[i mod N] + SIGMA * randn (default: 0.25 * noise_scale)")
    p.add_argument("--adapt_save", type=str, metavar="CKPT", **later, help="Also save the adapted Generator as a checkpoint")
    p.add_argument("--despeckle", nargs="?", type=lambda v: v if v == "auto" else int(v), const="auto", metavar="MIN_AREA", **later,
                   help="Remove ink components of fewer than MIN_AREA pixels from every generated signature before it is scored and "
                        "written (MIN_AREA omitted: max(2, round(0.001 * H * W))); ink is byte < --threshold, 128 without it "
                        "(default: off)")
    p.add_argument("--project_ssim", action="store_true", **later,
                   help="With --project: record every reconstruction's structural similarity (SSIM, 11-tap Gaussian window, computed "
                        "on the device) to its target in <prefix>_projection.json (default: off)")
    p.add_argument("--adapt_preprocess", action="store_true", **later,
                   help="With --adapt: the files are raw scans; send each through the device preprocessing (denoise, validate, crop, "
                        "resize, centre, CLAHE) at the checkpoint's size instead of the plain load (default: off)")
    p.add_argument("--project_preprocess", action="store_true", **later,
                   help="With --project: the same for the images to project (default: off)")
    p.add_argument("--pen_width", type=int, metavar="W", **later,
                   help="Redraw every generated signature at pen width W (1..9) before it is written: thinned to its centre line "
                        "and drawn again with a disc of squared radius (W - 1)^2 // 4, on the device; ink is byte < --threshold, "
                        "128 without it; after --despeckle when both are given; the plain run only (default: off)")
    p.add_argument("--diverse", action="store_true", **later,
                   help="With --filter_by_realism and --verifier_checkpoint: select for diversity -- greedily the signatures "
                        "farthest apart in the verifier's embedding space, among the most realistic of the pool -- instead of "
                        "keeping the top of the ranking; write <prefix>_diverse.json (default: off)")
    p.add_argument("--diverse_keep_ratio", type=float, metavar="R", **later,
                   help="With --diverse: the fraction of the pool, best realism first, that may be selected (default: 0.5)")
    p.add_argument("--diverse_real_dir", type=str, metavar="DIR", **later,
                   help="With --diverse and --diverse_memorisation_ratio: real signatures the selection must not copy")
    p.add_argument("--diverse_memorisation_ratio", type=float, metavar="R", **later,
                   help="With --diverse_real_dir: a candidate closer to a real signature than R times the real set's median "
                        "nearest-neighbour distance is not selected")
    p.add_argument("--diverse_existing_dir", type=str, metavar="DIR", **later,
                   help="With --diverse: a synthetic set that exists already; the selection keeps away from it too")
    p.add_argument("--diverse_min_separation", type=float, metavar="S", **later,
                   help="With --diverse: stop once no candidate is at least S (embedding distance) from everything kept; fewer "
                        "than n_samples may then be written (default: 0)")
    p.add_argument("--edit", action="store_true", **later,
                   help="Edit the shape of every generated signature (Adam on z around the ink moments' gradient, on the device) "
                        "before it is written; the latent vectors are the plain run's for the same --seed; write "
                        "<prefix>_edit.json (default: off)")
    p.add_argument("--edit_slant_delta", type=float, metavar="D", **later,
                   help="With --edit: add D to the slant, the shear coefficient sxy / syy; NEGATIVE leans to the right (default: 0)")
    p.add_argument("--edit_size_scale", type=float, metavar="R", **later,
                   help="With --edit: make the signature R times as large in the frame (its spread R^2 times) (default: 1)")
    p.add_argument("--edit_boldness_scale", type=float, metavar="R", **later,
                   help="With --edit: multiply the signature's ink mass by R (default: 1)")
    p.add_argument("--edit_shift", type=float, nargs=2, metavar=("DX", "DY"), **later,
                   help="With --edit: move the ink's centre by (DX, DY) in units of the image side, DY downwards (default: 0 0)")
    p.add_argument("--edit_steps", type=int, **later, help="Adam iterations of an edit (default: 30)")
    p.add_argument("--edit_lr", type=float, **later, help="Adam learning rate of an edit (default: 0.02)")
    p.add_argument("--edit_keep", type=float, metavar="W", **later,
                   help="With --edit: weight of staying the same signature, mean((G(z) - G(z0))^2) (default: 1)")
    p.add_argument("--edit_realism_weight", type=float, metavar="W", **later,
                   help="With --edit: weight of -log D(G(z)); needs the checkpoint's Discriminator (default: 0)")
    a = p.parse_args(argv)
    if edit_opt(a, "edit"):
        for flag, on in (("filter_by_realism", a.filter_by_realism), ("refine_by_realism", opt(a, "refine_by_realism")),
                         ("adapt", adapt_opt(a, "adapt") is not None), ("project", a.project is not None), ("morph", a.morph is not None),
                         ("pen_width", hasattr(a, "pen_width")), ("despeckle", hasattr(a, "despeckle"))):
            if on:
                p.error(f"--edit edits the plain generation run only; it cannot be combined with --{flag}")
        from .utils.inference import check_edit
        try:
            check_edit(**edit_kwargs(a), has_discriminator=True)
        except ValueError as e:
            p.error(f"--edit: {e}")
    elif any(hasattr(a, k) for k in EDIT_DEFAULTS):
        p.error("the --edit_* flags need --edit")
    if diverse_opt(a, "diverse"):
        if not a.filter_by_realism:
            p.error("--diverse needs --filter_by_realism")
        if identity_opt(a, "verifier_checkpoint") is None:
            p.error("--diverse needs --verifier_checkpoint")
        for flag, on in (("refine_by_realism", opt(a, "refine_by_realism")), ("adapt", adapt_opt(a, "adapt") is not None),
                         ("project", a.project is not None), ("morph", a.morph is not None), ("pen_width", hasattr(a, "pen_width"))):
            if on:
                p.error(f"--diverse cannot be combined with --{flag}")
        if any(hasattr(a, k) for k in IDENTITY_DEFAULTS if k != "verifier_checkpoint"):
            p.error("the --project_identity_* flags need --project")
        if (diverse_opt(a, "diverse_real_dir") is None) != (diverse_opt(a, "diverse_memorisation_ratio") is None):
            p.error("--diverse_real_dir and --diverse_memorisation_ratio need each other")
        ratio = diverse_opt(a, "diverse_memorisation_ratio")
        if not 0.0 < diverse_opt(a, "diverse_keep_ratio") <= 1.0 or not diverse_opt(a, "diverse_min_separation") >= 0 or (
                ratio is not None and not ratio >= 0):
            p.error("--diverse_keep_ratio must be in (0, 1], --diverse_min_separation and --diverse_memorisation_ratio >= 0")
    elif any(hasattr(a, k) for k in DIVERSE_DEFAULTS):
        p.error("the --diverse_* flags need --diverse")
    if hasattr(a, "pen_width"):
        if not 1 <= a.pen_width <= 9:
            p.error("--pen_width W must be in 1..9")
        for flag, on in (("filter_by_realism", a.filter_by_realism), ("refine_by_realism", opt(a, "refine_by_realism")),
                         ("adapt", adapt_opt(a, "adapt") is not None), ("project", a.project is not None), ("morph", a.morph is not None)):
            if on:
                p.error(f"--pen_width redraws the plain generation run only; it cannot be combined with --{flag}")
        if a.threshold is not None and not 1 <= a.threshold <= 255:
            p.error("--pen_width needs --threshold in 1..255")
    if hasattr(a, "project_ssim") and a.project is None:
        p.error("--project_ssim needs --project")
    if hasattr(a, "project_preprocess") and a.project is None:
        p.error("--project_preprocess needs --project")
    if hasattr(a, "adapt_preprocess") and adapt_opt(a, "adapt") is None:
        p.error("--adapt_preprocess needs --adapt")
    if hasattr(a, "despeckle"):
        if a.project is not None or a.morph is not None:
            p.error("--despeckle cleans generated signatures; projections and morph strips are left alone")
        if a.despeckle != "auto" and a.despeckle < 1:
            p.error("--despeckle MIN_AREA must be >= 1")
        if a.threshold is not None and not 1 <= a.threshold <= 255:
            p.error("--despeckle needs --threshold in 1..255")
    if adapt_opt(a, "adapt") is not None:
        for flag in ("filter_by_realism", "project", "morph"):
            if getattr(a, flag) not in (None, False):
                p.error(f"--adapt and --{flag} are mutually exclusive")
        if opt(a, "refine_by_realism"):
            p.error("--adapt and --refine_by_realism are mutually exclusive")
        sigma = adapt_opt(a, "adapt_sigma")
        if (adapt_opt(a, "adapt_steps") < 1 or not adapt_opt(a, "adapt_lr") > 0 or adapt_opt(a, "adapt_first_layer") < 0
                or not adapt_opt(a, "adapt_anchor") >= 0 or not adapt_opt(a, "adapt_realism_weight") >= 0
                or (sigma is not None and not sigma >= 0)):
            p.error("--adapt_steps must be >= 1, --adapt_lr > 0, --adapt_first_layer, --adapt_anchor, --adapt_realism_weight and "
                    "--adapt_sigma >= 0")
    elif any(hasattr(a, k) for k in ADAPT_DEFAULTS):
        p.error("the --adapt_* flags need --adapt")
    if opt(a, "refine_by_realism"):
        for flag in ("filter_by_realism", "project", "morph"):
            if getattr(a, flag) not in (None, False):
                p.error(f"--refine_by_realism and --{flag} are mutually exclusive")
    elif any(hasattr(a, k) for k in ("refine_steps", "refine_lr", "refine_prior")):
        p.error("--refine_steps, --refine_lr and --refine_prior need --refine_by_realism")
    if opt(a, "refine_steps") < 1 or not opt(a, "refine_lr") > 0 or not opt(a, "refine_prior") >= 0:
        p.error("--refine_steps must be >= 1, --refine_lr > 0, --refine_prior >= 0")
    if not opt(a, "project_realism_weight") >= 0 or not opt(a, "project_prior_weight") >= 0:
        p.error("--project_realism_weight and --project_prior_weight must be >= 0")
    if a.project is None and (hasattr(a, "project_realism_weight") or hasattr(a, "project_prior_weight")):
        p.error("--project_realism_weight and --project_prior_weight need --project")
    if a.project is None and not diverse_opt(a, "diverse") and any(hasattr(a, k) for k in IDENTITY_DEFAULTS):
        p.error("--verifier_checkpoint, --project_identity_weight and --project_identity_score_weight need --project")
    w_i = (identity_opt(a, "project_identity_weight"), identity_opt(a, "project_identity_score_weight"))
    if not w_i[0] >= 0 or not w_i[1] >= 0:
        p.error("--project_identity_weight and --project_identity_score_weight must be >= 0")
    if (w_i[0] > 0 or w_i[1] > 0) and identity_opt(a, "verifier_checkpoint") is None:
        p.error("--project_identity_weight and --project_identity_score_weight need --verifier_checkpoint")
    if identity_opt(a, "project_identity_resize") and identity_opt(a, "verifier_checkpoint") is None:
        p.error("--project_identity_resize needs --verifier_checkpoint")
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
    if adapt_opt(a, "adapt") is not None:
        from .utils.inference import load_generator_and_config
        generator, _, config = load_generator_and_config(a.checkpoint, device)
    else:
        generator, _ = load_generator(a.checkpoint, device)

    def need_discriminator(flag):
        discriminator = load_discriminator(a.checkpoint, device, image_size=generator.output_size)
        if discriminator is None:
            sys.exit(f"error: {a.checkpoint} holds no discriminator_state_dict: {flag} needs the Discriminator's "
                     "weights (a full training checkpoint, not a generator-only export)")
        return discriminator

    if adapt_opt(a, "adapt") is not None:
        w_d, sigma = adapt_opt(a, "adapt_realism_weight"), adapt_opt(a, "adapt_sigma")
        run_adapt(generator, adapt_opt(a, "adapt"), a.output_dir, device, a.n_samples, a.prefix, adapt_opt(a, "adapt_steps"),
                  adapt_opt(a, "adapt_lr"), adapt_opt(a, "adapt_first_layer"), adapt_opt(a, "adapt_anchor"),
                  need_discriminator("--adapt_realism_weight") if w_d > 0 else None, w_d,
                  0.25 * a.noise_scale if sigma is None else sigma, adapt_opt(a, "adapt_save"), a.seed, a.project_steps,
                  a.project_lr, a.project_restarts, a.threshold, a.transparent, config, **with_despeckle(despeckle_opt(a)),
                  **({"preprocess": True} if preprocess_opt(a, "adapt_preprocess") else {}))
        return
    if a.project is not None or a.morph is not None:
        if a.project is not None:
            w_d, w_p = opt(a, "project_realism_weight"), opt(a, "project_prior_weight")
            discriminator = need_discriminator("--project_realism_weight") if w_d > 0 else None
            verifier = None
            if identity_opt(a, "verifier_checkpoint") is not None:
                from .signature_verifier_eval import load_model
                verifier = load_model(identity_opt(a, "verifier_checkpoint"), device)[0]
            run_projection(generator, a.project, a.output_dir, a.prefix, a.project_steps, a.project_lr, a.project_restarts, a.seed,
                           discriminator, w_d, w_p, verifier, identity_opt(a, "project_identity_weight"),
                           identity_opt(a, "project_identity_score_weight"), identity_opt(a, "project_identity_resize"),
                           project_ssim_opt(a), **({"preprocess": True} if preprocess_opt(a, "project_preprocess") else {}))
        if a.morph is not None:
            run_morph(generator, a.morph, a.output_dir, device, a.prefix, a.morph_frames, a.seed, a.threshold, a.transparent,
                      a.project_steps, a.project_lr, a.project_restarts)
        return
    if edit_opt(a, "edit"):
        kw = edit_kwargs(a)
        generate_edited(generator, need_discriminator("--edit_realism_weight") if kw["realism_weight"] > 0 else None, a.n_samples,
                        a.output_dir, a.batch_size, device, a.seed, a.prefix, a.threshold, a.transparent, a.noise_scale, kw)
    elif opt(a, "refine_by_realism"):
        generate_refined(generator, need_discriminator("--refine_by_realism"), a.n_samples, a.output_dir, a.batch_size, device, a.seed,
                         a.prefix, opt(a, "refine_steps"), opt(a, "refine_lr"), opt(a, "refine_prior"), a.threshold, a.transparent,
                         a.noise_scale, **with_despeckle(despeckle_opt(a)))
    elif a.filter_by_realism and diverse_opt(a, "diverse"):
        from .signature_verifier_eval import load_model
        discriminator = need_discriminator("--diverse")
        verifier = load_model(identity_opt(a, "verifier_checkpoint"), device)[0]
        generate_diverse(generator, discriminator, verifier, a.n_samples, a.output_dir, a.batch_size, device, a.seed, a.prefix,
                         a.oversampling_ratio, a.threshold, a.transparent, a.noise_scale, despeckle_opt(a),
                         diverse_opt(a, "diverse_keep_ratio"), diverse_opt(a, "diverse_real_dir"),
                         diverse_opt(a, "diverse_memorisation_ratio"), diverse_opt(a, "diverse_existing_dir"),
                         diverse_opt(a, "diverse_min_separation"))
    elif a.filter_by_realism:
        discriminator = need_discriminator("--filter_by_realism")
        generate_filtered(generator, discriminator, a.n_samples, a.output_dir, a.batch_size, device, a.seed, a.prefix,
                          a.oversampling_ratio, a.threshold, a.transparent, a.noise_scale, **with_despeckle(despeckle_opt(a)))
    else:
        generate_signatures(generator, a.n_samples, a.output_dir, a.batch_size, device, a.seed, a.prefix, a.noise_scale,
                            a.threshold, a.transparent, **with_despeckle(despeckle_opt(a)), **with_pen_width(pen_width_opt(a)))
    print("\n" + "=" * 50 + "\nGeneration Summary:")
    print(f"  Checkpoint: {a.checkpoint}\n  Samples generated: {a.n_samples}\n  Output directory: {a.output_dir}")
    print(f"  Seed: {a.seed if a.seed is not None else 'Random'}\n  Device: {device}\n" + "=" * 50)


if __name__ == "__main__":
    main()
