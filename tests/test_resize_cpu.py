"""CPU-only checks of the device resize (include/siggan_resize.h): the numpy restatement of Pillow's antialiased bilinear
filter (resizecommon) equals Pillow byte for byte, the library's host-side coefficient table equals the restatement
exactly, every refusal happens before a device is touched, the existing 64x64 refusals stand when the new option is off,
and the new entry points are declared, listed and exported."""
import os
import re

import numpy as np
import pytest
import torch

from common import ROOT

import resizecommon as RC
import signature_gan_amd  # noqa: F401
from signature_gan_amd import _lib, resize
from signature_gan_amd.generate_signatures import parse_args
from signature_gan_amd.generator_vanilla_gan import Generator
from signature_gan_amd.signature_verifier_eval import SiameseNetwork
from signature_gan_amd.utils import inference

SHAPES = [(128, 128), (64, 64), (96, 150), (40, 50), (65, 127), (256, 256), (300, 77), (64, 128), (128, 64), (1, 1), (33, 200)]
AXES = [(128, 64), (150, 64), (50, 64), (127, 64), (64, 64), (1, 64)]


@pytest.mark.parametrize("kind", ["random", "binary", "ruled"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_is_pillow(shape, kind):
    a = RC.contents(kind, (2,) + shape, seed=shape[0] * 1000 + shape[1])
    want = RC.pillow_resize(a)
    got = RC.resize_u8_ref(a)
    assert want.shape == got.shape == (2, 64, 64) and want.dtype == got.dtype == np.uint8
    assert int((want != got).sum()) == 0


def test_restatement_is_pillow_at_other_output_sizes():
    """What the GPU tests use beyond 64x64: one output row off a tall image, an upscale, the largest output."""
    for shape, size in (((1024, 80), (1, 64)), ((20, 30), (64, 48)), ((300, 260), (128, 128)), ((64, 64), (64, 32))):
        a = RC.contents("random", (1,) + shape, seed=7)
        assert np.array_equal(RC.resize_u8_ref(a, size), RC.pillow_resize(a, size)), (shape, size)


@pytest.mark.parametrize("n_in,n_out", AXES, ids=lambda v: str(v))
def test_library_table_is_the_restatement(n_in, n_out):
    bounds, kk, kf = resize.coefficient_table(n_in, n_out)
    want_bounds, w = RC.coefficients(n_in, n_out)
    assert kk.shape == kf.shape == w.shape == (n_out, RC.ksize(n_in, n_out))
    assert np.array_equal(bounds, want_bounds)
    assert np.array_equal(kk, RC.quantise(w))
    assert kf.dtype == np.float32 and np.array_equal(kf, w.astype(np.float32))
    # every window lies inside the input, its weights sum to one in fixed point up to a rounding per tap
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= n_in).all() and (bounds[:, 1] >= 1).all()
    assert (np.abs(kk.sum(axis=1) - (1 << RC.PRECISION_BITS)) <= kk.shape[1]).all()


def test_table_refusals_need_no_device():
    lib = _lib.load()
    for n_in, n_out in ((0, 64), (1025, 64), (128, 0), (128, 129), (-1, 64)):
        assert lib.siggan_resize_ksize(n_in, n_out) == _lib.E_ARG
        assert lib.siggan_resize_table(n_in, n_out, None, None, None) == _lib.E_ARG
        assert b"outside" in lib.siggan_last_error()
        with pytest.raises(ValueError, match="outside"):
            resize.coefficient_table(n_in, n_out)
    assert lib.siggan_resize_ksize(1024, 1) == 2049 and lib.siggan_resize_ksize(1, 128) == 3
    assert lib.siggan_resize_table(128, 64, None, None, None) == 0          # every buffer is optional
    for fn in (lib.siggan_resize_u8, lib.siggan_resize_f32, lib.siggan_resize_f32_adjoint):
        assert fn(None, None, 1, 128, 128, None, 64, 64, None) == _lib.E_ARG   # a null context: refused


def test_python_refusals_happen_before_the_library():
    u8, f32 = torch.zeros(2, 128, 128, dtype=torch.uint8), torch.zeros(2, 128, 128)
    for fn, good, bad in ((resize.resize_u8, u8, f32), (resize.resize_f32, f32, u8)):
        with pytest.raises(ValueError, match="must be torch"):
            fn(bad)                                                          # a wrong dtype
        with pytest.raises(ValueError, match="no CPU path"):
            fn(good)                                                         # a CPU tensor with everything else in order
        for size in (0, 129, (64, 0), (129, 64), 64.0, (64,), True):
            with pytest.raises(ValueError, match="size"):
                fn(good, size)
        for shape in ((2, 0, 128), (2, 128, 1025), (2, 1025, 8), (128, 128), (2, 3, 128, 128)):
            with pytest.raises(ValueError, match="images"):
                fn(torch.zeros(shape, dtype=good.dtype))
        with pytest.raises(ValueError, match="tensor"):
            fn(np.zeros((2, 128, 128)))
    with pytest.raises(ValueError, match="in_hw"):
        resize.resize_f32_adjoint(torch.zeros(2, 64, 64), 1025)
    with pytest.raises(ValueError, match="in_hw"):
        resize.resize_f32_adjoint(torch.zeros(2, 64, 64), 0)
    with pytest.raises(ValueError, match="grad"):
        resize.resize_f32_adjoint(torch.zeros(2, 129, 64), 128)              # the gradient is of an output: <= 128
    with pytest.raises(ValueError, match="must be torch.float32"):
        resize.resize_f32_adjoint(torch.zeros(2, 64, 64, dtype=torch.float64), 128)
    with pytest.raises(ValueError, match="no CPU path"):
        resize.resize_f32_adjoint(torch.zeros(2, 64, 64), 128)
    assert not resize._CONTEXTS                                              # no context was ever created


def test_non_contiguous_input_is_refused_after_the_device_check():
    """Layout is the last refusal: on the CPU a strided tensor is refused for its device like any other, on the device it is
    refused as non-contiguous by all three calls (the GPU file checks that)."""
    strided = torch.zeros(2, 128, 256, dtype=torch.uint8)[:, :, ::2]
    assert not strided.is_contiguous()
    with pytest.raises(ValueError, match="no CPU path"):
        resize.resize_u8(strided)
    meta = torch.zeros(2, 128, 256, device="meta")[:, :, ::2]
    with pytest.raises(ValueError, match="no CPU path"):
        resize.resize_f32(meta)


def test_verifier_entry_points_refuse_without_a_device():
    model = SiameseNetwork(embedding_dim=40, max_images=4).eval()
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.embed_resized(torch.zeros(2, 128, 128, dtype=torch.uint8))
    with pytest.raises(ValueError):
        model.input_grad_resized(torch.zeros(2, 1, 128, 128), torch.zeros(2, 40), embed_weight=-1.0)
    with pytest.raises(ValueError):
        model.input_grad_resized(torch.zeros(2, 1, 128, 128, dtype=torch.float64), torch.zeros(2, 40))
    with pytest.raises(ValueError):
        model.input_grad_resized(torch.zeros(2, 128, 128), torch.zeros(2, 40))       # (N, 1, H, W) only
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.input_grad_resized(torch.zeros(2, 1, 128, 128), torch.zeros(2, 40))
    with pytest.raises(ValueError):                                          # 64x64: input_grad's own refusals
        model.input_grad_resized(torch.zeros(5, 1, 64, 64), torch.zeros(5, 40))
    assert model._ctx is None and not resize._CONTEXTS


def test_projection_keeps_its_64x64_refusal_without_the_option():
    g128 = Generator(100, 128).eval()
    verifier = SiameseNetwork(embedding_dim=40).eval()
    t = np.zeros((1, 128, 128), dtype=np.uint8)
    with pytest.raises(ValueError, match="64x64"):
        inference.project_signatures(g128, t, steps=1, verifier=verifier, identity_weight=1.0, verifier_resize=False)
    with pytest.raises(ValueError, match="64x64"):
        inference.project_signatures(g128, t, steps=1, verifier=verifier, identity_weight=1.0)
    with pytest.raises(ValueError, match="64x64"):
        inference.check_identity_projection(g128, verifier, 1.0, 0.0)
    assert inference.check_identity_projection(g128, verifier, 1.0, 0.5, verifier_resize=True) == (1.0, 0.5)
    # the other refusals do not depend on the option
    with pytest.raises(ValueError, match="eval"):
        inference.check_identity_projection(g128, SiameseNetwork(embedding_dim=40), 1.0, 0.0, verifier_resize=True)
    with pytest.raises(ValueError, match="need the verifier"):
        inference.check_identity_projection(g128, None, 1.0, 0.0, verifier_resize=True)
    assert g128._engine is None and verifier._ctx is None


def test_cli_takes_the_resize_flag_and_keeps_the_namespace():
    base = ["--checkpoint", "g.pt", "--project", "dir"]
    assert "project_identity_resize" not in vars(parse_args(base))
    a = parse_args(base + ["--verifier_checkpoint", "v.pth", "--project_identity_resize"])
    assert a.project_identity_resize is True
    for bad in (["--checkpoint", "g.pt", "--project_identity_resize"], base + ["--project_identity_resize"]):
        with pytest.raises(SystemExit):
            parse_args(bad)


def test_evaluate_no_longer_refuses_a_128_generator():
    from signature_gan_amd import evaluate_vanilla_gan_signatures as cli
    v = cli.VerifierFeatures("missing.pth", torch.device("cpu"), 128)
    assert v.input_resize == "pillow_bilinear_128_to_64" and "64x64" not in (v.error or "")
    assert "Checkpoint not found" in v.error and v.sink() is None           # the load failed, and only that is recorded
    assert cli.VerifierFeatures("missing.pth", torch.device("cpu"), 64).input_resize is None


def test_entry_points_are_declared_listed_and_exported():
    h = open(os.path.join(ROOT, "include", "siggan_resize.h")).read()
    gh = open(os.path.join(ROOT, "include", "siggan.h")).read()
    assert "#define SIGGAN_ABI_VERSION 4" in gh and _lib.ABI_VERSION == 4     # new symbols only
    declared = set(re.findall(r"\b(?:int|int32_t)\s+(siggan_resize\w*)\s*\(", h))
    assert declared == set(_lib.RESIZE_EXPORTS)
    assert not set(_lib.RESIZE_EXPORTS) & set(_lib.EXPORTS)
    lib = _lib.load()
    for name in _lib.RESIZE_EXPORTS:
        fn = getattr(lib, name)
        decl = re.search(r"\b" + name + r"\(([^;]*)\);", h)
        assert decl and len(decl.group(1).split(",")) == len(fn.argtypes), name
    assert f"#define SIGGAN_RESIZE_MAX_IN  {_lib.RESIZE_MAX_IN}" in h and f"#define SIGGAN_RESIZE_MAX_OUT {_lib.RESIZE_MAX_OUT}" in h
    mk = open(os.path.join(ROOT, "signature-gan_amd", "csrc", "Makefile")).read()
    # the source is listed; its headers, siggan_resize.h among them, are tracked through the compiler's dependency files
    assert "resize.hip" in mk and "-MMD" in mk and "-include $(OBJ:.o=.d)" in mk
    dep = os.path.join(ROOT, "signature-gan_amd", "csrc", "resize.d")       # written beside the object by the build that made the library
    assert os.path.exists(dep), "resize.d is missing: the library was not built by csrc/Makefile"
    assert "siggan_resize.h" in open(dep).read()
