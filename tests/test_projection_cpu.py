"""Host side of latent-space projection and morphing (no GPU): the blend is the reference app's expression bit for bit, the
strip is laid out as the app lays it out (a Pillow restatement of app_vanilla_gan_signatures.py:1706-1712), the CLI takes the
new flags and keeps every existing default, the batch / restart plan and the starts are what the documentation says, and the
new entry point is declared, listed and exported."""
import os
import re

import numpy as np
import pytest
import torch

from common import ROOT

import signature_gan_amd  # noqa: F401
from signature_gan_amd import _lib
from signature_gan_amd.generate_signatures import parse_args
from signature_gan_amd.utils.inference import (morph_blend, morph_strip, process_images, projection_plan, projection_starts)


@pytest.mark.parametrize("n_frames", [2, 5, 10, 30])
def test_blend_is_the_apps_expression(n_frames):
    gen = torch.Generator().manual_seed(3)
    z1, z2 = torch.randn(1, 100, generator=gen), torch.randn(1, 100, generator=gen)
    got = morph_blend(z1, z2, n_frames)
    assert got.shape == (n_frames, 100) and got.dtype == torch.float32
    for i in range(n_frames):
        a = i / (n_frames - 1)
        z_interp = (1 - a) * z1 + a * z2                                  # app_vanilla_gan_signatures.py:1696-1697
        assert torch.equal(got[i:i + 1], z_interp), i
    assert torch.equal(got[0], z1[0]) and torch.equal(got[-1], z2[0])     # a = 0 and a = 1 are exact
    assert torch.equal(morph_blend(z1[0], z2[0], n_frames), got)          # (latent,) endpoints too
    with pytest.raises(ValueError):
        morph_blend(z1, z2, 1)
    with pytest.raises(ValueError):
        morph_blend(z1, z2[:, :50], n_frames)


def _app_strip(frames, apply_threshold, threshold_value, make_transparent):
    """app_vanilla_gan_signatures.py:1699-1712 from `frame = Image.fromarray(...)` on, restated with Pillow."""
    from PIL import Image
    out = []
    for arr in frames:
        frame = Image.fromarray(arr)
        if apply_threshold:
            frame = process_images([frame], threshold=threshold_value, make_transparent=make_transparent)[0]
        out.append(frame)
    n_frames = len(out)
    strip_width = out[0].width * n_frames
    strip = Image.new('RGBA' if make_transparent else 'L', (strip_width, out[0].height), (255, 255, 255, 0) if make_transparent else 255)
    for i, frame in enumerate(out):
        if frame.mode != strip.mode:
            frame = frame.convert(strip.mode)
        strip.paste(frame, (i * out[0].width, 0))
    return strip


@pytest.mark.parametrize("transparent", [False, True], ids=["L", "RGBA"])
@pytest.mark.parametrize("threshold", [None, 127, 200])
def test_strip_layout_is_the_apps(threshold, transparent):
    from PIL import Image
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, size=(7, 12, 9), dtype=np.uint8)          # seven frames, 9 wide and 12 high
    want = _app_strip(frames, threshold is not None, threshold, transparent)
    got = morph_strip(frames, threshold=threshold, make_transparent=transparent)
    assert got.mode == want.mode == ("RGBA" if transparent else "L")
    assert got.size == want.size == (9 * 7, 12)
    assert np.array_equal(np.array(got), np.array(want))
    if threshold is None and not transparent:                               # the plain strip is the frames side by side
        assert np.array_equal(np.array(got), np.concatenate(list(frames), axis=1))
    if threshold is not None and transparent:                               # ink opaque black, paper transparent white
        px = np.array(got)
        ink = np.concatenate(list(frames), axis=1) < threshold
        assert (px[ink] == (0, 0, 0, 255)).all() and (px[~ink] == (255, 255, 255, 0)).all()
    pil = [Image.fromarray(f, mode="L") for f in frames]                    # PIL frames are taken as they are
    assert np.array_equal(np.array(morph_strip(pil, threshold=threshold, make_transparent=transparent)), np.array(want))
    with pytest.raises(ValueError):
        morph_strip([])


def test_cli_takes_the_new_flags_and_keeps_the_defaults():
    a = vars(parse_args(["--checkpoint", "g.pt"]))
    before = dict(checkpoint="g.pt", n_samples=100, output_dir="./generated_signatures", batch_size=64, seed=None,
                  prefix="signature", device="auto", info=False, filter_by_realism=False, oversampling_ratio=2.0, threshold=None,
                  transparent=False, noise_scale=1.0)
    assert {k: a[k] for k in before} == before
    new = {k: v for k, v in a.items() if k not in before}
    assert new == dict(morph=None, morph_frames=10, project=None, project_steps=200, project_lr=0.05, project_restarts=1)
    assert parse_args(["--checkpoint", "g.pt", "--morph"]).morph == []
    a = parse_args(["--checkpoint", "g.pt", "--morph", "a.png", "b.png", "--morph_frames", "5", "--project", "dir",
                    "--project_steps", "40", "--project_lr", "0.02", "--project_restarts", "3"])
    assert (a.morph, a.morph_frames, a.project) == (["a.png", "b.png"], 5, "dir")
    assert (a.project_steps, a.project_lr, a.project_restarts) == (40, 0.02, 3)
    for bad in (["--morph", "a.png"], ["--morph", "a", "b", "c"], ["--morph_frames", "1"], ["--project_steps", "0"],
                ["--project_restarts", "0"], ["--project_lr", "0"]):
        with pytest.raises(SystemExit):
            parse_args(["--checkpoint", "g.pt"] + bad)


def test_plan_walks_every_restart_through_the_same_chunks():
    assert projection_plan(5, 1, 2) == [(0, 0, 2), (0, 2, 2), (0, 4, 1)]
    assert projection_plan(5, 2, 2) == [(0, 0, 2), (0, 2, 2), (0, 4, 1), (1, 0, 2), (1, 2, 2), (1, 4, 1)]
    assert projection_plan(3, 2, 64) == [(0, 0, 3), (1, 0, 3)]
    assert projection_plan(0, 2, 4) == []
    for n, r, mb in ((7, 3, 4), (64, 1, 64), (65, 2, 64)):
        plan = projection_plan(n, r, mb)
        seen = sorted((rr, t) for rr, t0, b in plan for t in range(t0, t0 + b))
        assert seen == [(rr, t) for rr in range(r) for t in range(n)]       # every candidate exactly once
        assert all(1 <= b <= mb for _, _, b in plan)
        assert [c[1:] for c in plan if c[0] == 0] * r == [c[1:] for c in plan]
    for bad in ((3, 0, 4), (3, 1, 0), (-1, 1, 4)):
        with pytest.raises(ValueError):
            projection_plan(*bad)


def test_starts_are_seeded_per_restart():
    z0 = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    assert torch.equal(projection_starts(2, 3, 0, z0=z0, seed=4), z0)       # restart 0 starts where the caller says
    a = projection_starts(2, 3, 1, z0=z0, seed=4)
    assert torch.equal(a, torch.randn(2, 3, generator=torch.Generator().manual_seed(5)))
    assert torch.equal(a, projection_starts(2, 3, 0, seed=5))               # restart r of seed s = restart 0 of seed s + r
    assert not torch.equal(a, projection_starts(2, 3, 2, seed=4))
    with pytest.raises(ValueError):
        projection_starts(2, 3, 0, z0=z0[:1])


def test_entry_point_is_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "siggan.h")).read()
    decl = re.search(r"int siggan_g_latent_grad\(([^)]*)\)", header)
    assert decl and decl.group(1).count(",") == 8                           # nine parameters
    assert "siggan_g_latent_grad" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "siggan_g_latent_grad")
    assert len(lib.siggan_g_latent_grad.argtypes) == 9
    assert lib.siggan_g_latent_grad(None, None, 1, None, None, None, None, None, None) == -1      # a null context: refused
    with pytest.raises(ValueError):
        _lib.check(-1)
