"""preprocess_signatures' command line and generate_signatures' --adapt_preprocess on the MI355X, on a temporary folder of
files the test writes with Pillow: grayscale, RGB and RGBA PNGs, a JPEG, an upper-case extension, a text file named .png, a
blank page and a scan that is too small.  The yardstick is the numpy restatement (preprocesscommon.restate) on the bytes
Pillow decodes; every comparison of pixels is exact."""
import json

import numpy as np
import pytest
import torch
from PIL import Image

import preprocesscommon as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    src = tmp_path_factory.mktemp("scans")
    gray = PC.pen_scan(90, 140, 41)
    Image.fromarray(gray, mode="L").save(src / "b_gray.png")
    rgb = np.stack([gray, np.minimum(gray.astype(np.int64) + 20, 255).astype(np.uint8), gray // 2 + 100], axis=-1)
    Image.fromarray(rgb, mode="RGB").save(src / "c_rgb.png")
    rgba = np.concatenate([rgb[:, ::-1], np.full(gray.shape + (1,), 255, np.uint8)], axis=-1)
    Image.fromarray(np.ascontiguousarray(rgba), mode="RGBA").save(src / "d_rgba.png")
    Image.fromarray(PC.pen_scan(120, 100, 42), mode="L").save(src / "e_photo.jpg", quality=90)
    Image.fromarray(PC.pen_scan(33, 47, 43), mode="L").save(src / "a_UPPER.PNG")
    (src / "f_text.png").write_text("this is not an image\n")
    Image.fromarray(np.full((70, 50), 251, np.uint8), mode="L").save(src / "g_blank.png")
    Image.fromarray(np.full((10, 40), 0, np.uint8), mode="L").save(src / "h_small.png")
    (src / "notes.txt").write_text("ignored\n")
    return src


GOOD = ["a_UPPER.PNG", "b_gray.png", "c_rgb.png", "d_rgba.png", "e_photo.jpg"]


def decoded(folder, name):
    return np.asarray(Image.open(folder / name).convert("L"), dtype=np.uint8)


def summary(success, fail, failed):
    text = "\n" + "=" * 50 + "\nPreprocessing Complete\n" + "=" * 50 + f"\nSuccessfully processed: {success}\nFailed: {fail}\n"
    if failed:
        text += "\nFailed files:\n" + "".join(f"  - {f}\n" for f in failed)
    return text


def test_the_command_line_writes_what_the_device_api_computes(folder, tmp_path, capsys):
    from signature_gan_amd import preprocess, preprocess_signatures as ps
    out = tmp_path / "out"
    ps.main([str(folder), str(out)])
    failed = [str(folder / n) for n in ("f_text.png", "g_blank.png", "h_small.png")]
    assert capsys.readouterr().out == summary(5, 3, failed)
    assert sorted(p.name for p in out.iterdir()) == sorted(n.rsplit(".", 1)[0] + "_processed.png" for n in GOOD)
    scans = [decoded(folder, n) for n in GOOD]
    made, stats = preprocess.preprocess_scans(preprocess.pack_scans(scans, "cuda:0"), 64)
    made = made.cpu().numpy()
    for i, n in enumerate(GOOD):
        im = Image.open(out / (n.rsplit(".", 1)[0] + "_processed.png"))
        assert im.mode == "L" and im.size == (64, 64)
        assert np.array_equal(np.asarray(im), made[i]) and np.array_equal(made[i], PC.restate(scans[i], 64)["out"]), n
    assert decoded(folder, "c_rgb.png").tolist() != decoded(folder, "b_gray.png").tolist()                    # colour went through 'L'
    # the function returns the tuple the summary printed
    assert ps.preprocess_batch(folder, tmp_path / "again") == (5, 3, failed)
    assert sorted(p.name for p in (tmp_path / "again").iterdir()) == sorted(p.name for p in out.iterdir())
    # one file: None for the three bad ones, floats in [-1, 1] or bytes for a good one
    for n in ("f_text.png", "g_blank.png", "h_small.png"):
        assert ps.preprocess_single_image(folder / n) is None
    x = ps.preprocess_single_image(folder / "b_gray.png")
    u = ps.preprocess_single_image(folder / "b_gray.png", normalize=False)
    assert x.dtype == np.float32 and x.shape == (64, 64) and -1.0 <= x.min() < x.max() <= 1.0
    assert u.dtype == np.uint8 and np.array_equal(u, made[1]) and np.array_equal(x, ps.normalize_pixels(u))
    assert ps.save_preprocessed_image(x, tmp_path / "deep" / "x.png") and np.array_equal(np.asarray(Image.open(tmp_path / "deep" / "x.png")),
                                                                                       ps.denormalize_pixels(x))


def test_no_validate_keeps_the_blank_page_and_the_other_flags_reach_the_kernels(folder, tmp_path, capsys):
    from signature_gan_amd import preprocess_signatures as ps
    failed = [str(folder / n) for n in ("f_text.png", "h_small.png")]
    ps.main([str(folder), str(tmp_path / "nv"), "--no-validate"])
    assert capsys.readouterr().out == summary(6, 2, failed)
    blank = np.asarray(Image.open(tmp_path / "nv" / "g_blank_processed.png"))
    assert np.array_equal(blank, PC.restate(decoded(folder, "g_blank.png"), 64)["out"])
    ps.main([str(folder), str(tmp_path / "big"), "--size", "128"])
    assert capsys.readouterr().out == summary(5, 3, [str(folder / n) for n in ("f_text.png", "g_blank.png", "h_small.png")])
    for n in GOOD:
        im = np.asarray(Image.open(tmp_path / "big" / (n.rsplit(".", 1)[0] + "_processed.png")))
        assert im.shape == (128, 128) and np.array_equal(im, PC.restate(decoded(folder, n), 128)["out"]), n
    ps.main([str(folder), str(tmp_path / "bare"), "--no-crop", "--no-center", "--no-denoise"])
    capsys.readouterr()
    im = np.asarray(Image.open(tmp_path / "bare" / "b_gray_processed.png"))
    assert np.array_equal(im, PC.restate(decoded(folder, "b_gray.png"), 64, denoise_on=False, crop=False, center=False)["out"])
    with pytest.raises(SystemExit) as e:
        ps.main([str(folder), str(tmp_path / "bin"), "--binarize"])
    assert "not implemented here" in str(e.value.code) and not (tmp_path / "bin").exists()


def test_adapt_preprocess_runs_on_raw_scans_and_records_the_preprocessed_targets(tmp_path):
    from signature_gan_amd import generate_signatures as cli
    from signature_gan_amd.generator_vanilla_gan import Generator
    torch.manual_seed(11)
    g = Generator(latent_dim=100, output_size=64).to("cuda").eval()
    ck = tmp_path / "gan.pt"
    torch.save({"epoch": 1, "generator_state_dict": {k: v.detach().cpu().clone() for k, v in g.state_dict().items()},
                "config": {"latent_dim": 100, "image_size": 64}}, ck)
    src = tmp_path / "raw"
    src.mkdir()
    scans = [PC.pen_scan(h, w, 50 + i) for i, (h, w) in enumerate([(80, 150), (200, 160), (64, 64)])]
    for i, a in enumerate(scans):
        Image.fromarray(a, mode="L").save(src / f"scan_{i}.png")
    out = tmp_path / "out"
    cli.main(["--checkpoint", str(ck), "--output_dir", str(out), "--seed", "3", "--n_samples", "2", "--adapt", str(src), "--adapt_preprocess",
              "--adapt_steps", "2", "--project_steps", "4"])
    rep = json.load(open(out / "signature_adapt.json"))
    assert rep["preprocess"] is True and [t["file"] for t in rep["targets"]] == ["scan_0.png", "scan_1.png", "scan_2.png"]
    for i, t in enumerate(rep["targets"]):
        assert t["preprocessed_target"] == f"signature_target_{i + 1:06d}.png"
        assert np.array_equal(np.asarray(Image.open(out / t["preprocessed_target"])), PC.restate(scans[i], 64)["out"])
    assert len(sorted(out.glob("signature_0*.png"))) == 2
    # --project_preprocess: the same targets, named in every record
    cli.main(["--checkpoint", str(ck), "--output_dir", str(tmp_path / "proj"), "--seed", "3", "--project", str(src / "scan_1.png"),
              "--project_preprocess", "--project_steps", "3"])
    rec = json.load(open(tmp_path / "proj" / "signature_projection.json"))
    assert len(rec) == 1 and rec[0]["file"] == "scan_1.png" and rec[0]["preprocessed_target"] == "signature_target_000001.png"
    assert np.array_equal(np.asarray(Image.open(tmp_path / "proj" / "signature_target_000001.png")), PC.restate(scans[1], 64)["out"])
    # a blank page among the targets ends the run
    Image.fromarray(np.full((64, 64), 250, np.uint8), mode="L").save(src / "scan_3.png")
    with pytest.raises(ValueError, match="preprocessing rejected"):
        cli.main(["--checkpoint", str(ck), "--output_dir", str(tmp_path / "bad"), "--adapt", str(src), "--adapt_preprocess"])
