"""Host side of realism-filtered generation (the reference app's "Filter by Realism"): the batch plan, the binarisation and
post-processing, the dequantisation table the Discriminator's byte-reading first block uses, checkpoint loading, the CLI
flags and the new exports.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import signature_gan_amd  # noqa: F401  (import shim)
from signature_gan_amd import _lib
from signature_gan_amd.utils import inference as inf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_filter_plan_follows_the_reference_arithmetic():
    assert inf.filter_plan(7, 1.5, 4, 11) == (10, [(4, 11), (4, 12), (2, 13)])              # int(10.5), ragged last batch
    assert inf.filter_plan(5, 2.5, 32, 0) == (12, [(12, 0)])                                 # int(12.5), one short batch
    assert inf.filter_plan(3, 1.5, 2, None) == (4, [(2, None), (2, None)])                   # int(4.5), no seed
    assert inf.filter_plan(10, 2.5, 8, 3) == (25, [(8, 3), (8, 4), (8, 5), (1, 6)])
    assert inf.filter_plan(0, 2.0, 8, 3) == (0, [])
    with pytest.raises(ValueError):
        inf.filter_plan(4, 2.0, 0, None)


def _all_bytes_image():
    from PIL import Image
    return Image.fromarray(np.arange(256, dtype=np.uint8).reshape(16, 16))


@pytest.mark.parametrize("thr", [1, 127, 128, 255])
def test_binarize_uint8_is_pillows_point_route(thr):
    img = _all_bytes_image()
    want = np.array(img.point(lambda x: 0 if x < thr else 255, mode="1").convert("L"))
    assert set(np.unique(want)) <= {0, 255} and int((want == 0).sum()) == thr
    got = inf.binarize_uint8(np.array(img), thr)
    assert got.dtype == np.uint8 and np.array_equal(got, want)


@pytest.mark.parametrize("thr", [1, 127, 128, 255])
def test_process_images_modes_and_alpha(thr):
    img = _all_bytes_image()
    want = inf.binarize_uint8(np.array(img), thr)
    plain, = inf.process_images([img], threshold=thr)
    assert plain.mode == "1" and np.array_equal(np.array(plain.convert("L")), want)
    rgba, = inf.process_images([img], threshold=thr, make_transparent=True)
    assert rgba.mode == "RGBA"
    a = np.array(rgba)
    ink = want == 0
    assert (a[ink] == (0, 0, 0, 255)).all() and (a[~ink] == (255, 255, 255, 0)).all()
    assert np.array_equal(np.array(rgba.convert("L")), want)             # what the reference scores after post-processing
    assert inf.process_images([], threshold=thr) == []
    # the default threshold is the app's
    assert np.array_equal(np.array(inf.process_images([img])[0].convert("L")), inf.binarize_uint8(np.array(img), 127))


def test_dequantisation_table_is_the_torch_cpu_expression():
    table = _lib.dequant_table()
    want = (torch.from_numpy(np.arange(256, dtype=np.uint8)).float() / 127.5 - 1.0).numpy()
    assert table.dtype == np.float32 and table.shape == (256,)
    assert np.array_equal(table.view(np.uint32), want.view(np.uint32))
    assert table[0] == -1.0 and table[255] == 1.0
    # the shortcut the table exists to avoid really differs (so the comparison above can fail)
    shortcut = np.arange(256, dtype=np.float32) * np.float32(1.0 / 127.5) - np.float32(1.0)
    assert (shortcut != want).sum() > 50
    assert np.array_equal(inf.dequantize_uint8(np.arange(256, dtype=np.uint8).reshape(1, 16, 16)).numpy().reshape(-1), want)
    assert _lib.load().siggan_dequant_table(None) == -1


def test_cli_defaults_leave_the_filter_off():
    from signature_gan_amd.generate_signatures import parse_args
    a = parse_args(["--checkpoint", "g.pth"])
    assert (a.filter_by_realism, a.oversampling_ratio, a.threshold, a.transparent, a.noise_scale) == (False, 2.0, None, False, 1.0)
    a = parse_args(["--checkpoint", "g.pth", "--filter_by_realism", "--oversampling_ratio", "1.5", "--threshold", "127",
                    "--transparent", "--noise_scale", "0.8"])
    assert (a.filter_by_realism, a.oversampling_ratio, a.threshold, a.transparent, a.noise_scale) == (True, 1.5, 127, True, 0.8)
    for bad in (["--filter_by_realism", "--oversampling_ratio", "0.5"], ["--oversampling_ratio", "3"],
                ["--filter_by_realism", "--threshold", "256"], ["--transparent"]):
        with pytest.raises(SystemExit):
            parse_args(["--checkpoint", "g.pth"] + bad)


def test_load_discriminator_returns_none_without_discriminator_weights(tmp_path):
    from signature_gan_amd.generator_vanilla_gan import Generator
    g = Generator(latent_dim=16, output_size=64)
    p = tmp_path / "generator_only.pth"
    torch.save({"generator_state_dict": g.state_dict(), "config": {"latent_dim": 16, "image_size": 64}}, p)
    assert inf.load_discriminator(str(p), torch.device("cpu")) is None
    q = tmp_path / "bare.pth"
    torch.save(g.state_dict(), q)                                        # a dict, but of tensors: no discriminator either
    assert inf.load_discriminator(str(q), torch.device("cpu")) is None
    r = tmp_path / "not_a_dict.pth"
    torch.save([torch.zeros(2)], r)
    assert inf.load_discriminator(str(r), torch.device("cpu")) is None
    with pytest.raises(FileNotFoundError):                               # other errors propagate
        inf.load_discriminator(str(tmp_path / "missing.pth"), torch.device("cpu"))


@pytest.mark.parametrize("sn", [False, True])
def test_load_discriminator_builds_the_checkpoints_network(tmp_path, sn):
    from signature_gan_amd.discriminator_vanilla_gan import Discriminator
    d = Discriminator(input_size=64, use_spectral_norm=sn)
    p = tmp_path / "full.pth"
    torch.save({"discriminator_state_dict": d.state_dict()}, p)
    got = inf.load_discriminator(str(p), torch.device("cpu"))
    assert isinstance(got, Discriminator) and not got.training and got.use_spectral_norm == sn
    for k, v in d.state_dict().items():
        assert torch.equal(got.state_dict()[k], v)
    with pytest.raises(RuntimeError):                                    # eval-mode only, and there is no CPU path
        got.train().score_u8(torch.zeros(1, 64, 64, dtype=torch.uint8))


def test_new_symbols_are_exported_and_the_abi_stays_4():
    lib = _lib.load()
    assert lib.siggan_abi_version() == 4 and _lib.ABI_VERSION == 4
    for name in ("siggan_d_score_u8", "siggan_dequant_table") + _lib.SELECT_EXPORTS:
        assert hasattr(lib, name), name
    assert set(_lib.SELECT_EXPORTS) == {"siggan_select_topk", "siggan_gather_u8"}
    header = open(os.path.join(ROOT, "include", "siggan_select.h")).read()
    for name in _lib.SELECT_EXPORTS:
        assert f"int {name}(" in header
    assert f"#define SIGGAN_SELECT_MAX {_lib.SELECT_MAX}" in header
    # refusals that need no device: null tensors
    assert lib.siggan_select_topk(0, None, 4, 2, None, None) == -1
    assert lib.siggan_gather_u8(0, None, 4, 64, None, 2, -1, None, None) == -1
    assert lib.siggan_d_score_u8(None, None, 1, -1, None, None, None) == -1
    assert b"null" in lib.siggan_last_error()
