"""The wrappers' shared calling convention (signature_gan_amd/_call.py) and the symbol registry (_lib.GROUPS), without a
device: every helper's refusals word for word and in their order, the order the two check_arguments keep around them, and
ALL_EXPORTS."""
import re

import numpy as np
import pytest
import torch

import signature_gan_amd  # noqa: F401
from signature_gan_amd import _call, _lib, components, resize, shape, ssim, strokes
from signature_gan_amd.utils import diverse, neighbors, twosample

NO_CPU = "a ROCm device ('cuda:N'); there is no CPU path"


def refusal(fn, *args, **kwargs) -> str:
    with pytest.raises(ValueError) as e:
        fn(*args, **kwargs)
    return str(e.value)


def u8(*shape):
    return torch.zeros(shape, dtype=torch.uint8)


def test_ptr_is_null_for_none_and_the_address_otherwise():
    t = torch.zeros(4)
    assert _call.ptr(None).value is None and _call.ptr(t).value == t.data_ptr()


def test_as_int_takes_integers_only():
    assert _call.as_int(3, "k") == 3 and _call.as_int(np.int64(5), "k") == 5 and type(_call.as_int(np.int32(5), "k")) is int
    assert refusal(_call.as_int, True, "fill") == "fill must be an integer, got True"
    assert refusal(_call.as_int, 1.0, "threshold") == "threshold must be an integer, got 1.0"
    assert refusal(_call.as_int, "3", "pen width") == "pen width must be an integer, got '3'"


def test_check_u8_images_refuses_in_order_type_dtype_rank_sizes():
    chk = _call.check_u8_images
    assert chk(u8(2, 8, 12)) == (2, 8, 12) and chk(u8(3, 1, 128, 128)) == (3, 128, 128) and chk(u8(0, 1, 4)) == (0, 1, 4)
    assert refusal(chk, [1], "images") == "images must be a tensor, got list"
    assert refusal(chk, None, "a", kinds="a tensor or an SsimSet") == "a must be a tensor or an SsimSet, got NoneType"
    assert refusal(chk, torch.zeros(2, 3, 5), "images") == "images must be torch.uint8, got torch.float32"       # dtype before rank
    assert refusal(chk, u8(2, 2, 3, 5), "b") == "b must be (N, H, W) or (N, 1, H, W), got (2, 2, 3, 5)"          # rank before sizes
    assert refusal(chk, u8(8, 8), "images") == "images must be (N, H, W) or (N, 1, H, W), got (8, 8)"
    assert refusal(chk, u8(0, 200, 5), "images", allow_empty=False) == "images holds no image"                   # emptiness first
    assert refusal(chk, u8(1, 200, 5), "images") == "height = 200 outside [1, 128]"                              # height before width
    assert refusal(chk, u8(1, 10, 16), "images", 11, 12, 128) == "height = 10 outside [11, 128]"
    assert refusal(chk, u8(1, 8, 6), "images") == "width = 6 must be a multiple of 4 in [4, 128]"
    assert refusal(chk, u8(1, 8, 132), "images", max_size=128) == "width = 132 must be a multiple of 4 in [4, 128]"
    assert refusal(chk, u8(1, 11, 8), "images", 11, 12, 128) == "width = 8 must be a multiple of 4 in [12, 128]"
    assert chk(u8(1, 8, 24)[:, :, ::2]) == (1, 8, 12)                        # layout and device are not its business


def test_check_resident_refuses_the_device_before_the_layout():
    strided = u8(2, 8, 16)[:, :, ::2]
    assert not strided.is_contiguous()
    assert refusal(_call.check_resident, strided, "images") == f"images must live on {NO_CPU}"
    assert refusal(_call.check_resident, u8(2, 8, 8), "byte images") == f"byte images must live on {NO_CPU}"

    class OnDevice:                                                          # the layout branch without a device: a stand-in
        device = torch.device("cuda", 0)

        def is_contiguous(self):
            return False
    assert refusal(_call.check_resident, OnDevice(), "grad") == "grad must be contiguous"


def test_check_rows_refuses_in_order_residence_dtype_and_sizes_layout():
    chk = _call.check_rows
    rows = torch.zeros(5, 3)
    assert refusal(chk, "q", [[1.0]], torch.float32, "(n, dim)") == f"q must be a tensor on {NO_CPU}"
    assert refusal(chk, "q", rows.double()[:, ::2], torch.float32, "(n, dim)") == f"q must be a tensor on {NO_CPU}"     # residence first
    cpu = torch.device("cpu")                                                # as `device`, a CPU tensor passes the residence check
    assert refusal(chk, "labels", rows, torch.uint8, "(5, cols)", shape=(5, None), device=torch.device("meta"),
                   where="x's device cuda:0") == "labels must be a tensor on x's device cuda:0"
    assert refusal(chk, "x", rows.double()[:, ::2], torch.float32, "(n, dim)", device=cpu) == \
        "x must be float32 (n, dim), got torch.float64 (5, 2)"                                                          # dtype before layout
    assert refusal(chk, "x", torch.zeros(5), torch.float32, "(n, dim)", device=cpu) == "x must be float32 (n, dim), got torch.float32 (5,)"
    assert refusal(chk, "labels", torch.zeros(4, 2, dtype=torch.uint8), torch.uint8, "(5, cols)", shape=(5, None), device=cpu) == \
        "labels must be uint8 (5, cols), got torch.uint8 (4, 2)"
    assert refusal(chk, "features", rows, torch.float32, "(n, 4)", shape=(None, 4), device=cpu) == \
        "features must be float32 (n, 4), got torch.float32 (5, 3)"
    assert refusal(chk, "scores", torch.zeros(0), torch.float32, "(n >= 1,)", shape=(None,), min_rows=1, device=cpu) == \
        "scores must be float32 (n >= 1,), got torch.float32 (0,)"
    assert refusal(chk, "x", torch.zeros(5, 6)[:, ::2], torch.float32, "(n, dim)", device=cpu) == "x must be contiguous"
    chk("x", torch.zeros(5, 6)[:, ::2], torch.float32, "(n, dim)", device=cpu, contiguous=False)
    chk("x", rows, torch.float32, "(n, dim)", device=cpu)
    chk("scores", torch.zeros(1), torch.float32, "(n >= 1,)", shape=(None,), min_rows=1, device=cpu)


def test_check_vector_out_and_stats_have_one_message_each():
    cpu = torch.device("cpu")
    _call.check_vector("radius2", torch.zeros(3, dtype=torch.float64), torch.float64, 3, cpu)
    for bad in (None, torch.zeros(3), torch.zeros(4, dtype=torch.float64), torch.zeros(6, dtype=torch.float64)[::2],
                torch.zeros(3, dtype=torch.float64, device="meta")):
        assert refusal(_call.check_vector, "radius2", bad, torch.float64, 3, cpu) == "radius2 must be a contiguous float64 (3,) tensor on cpu"
    assert refusal(_call.check_vector, "eligible", torch.zeros(3), torch.uint8, 3, cpu) == "eligible must be a contiguous uint8 (3,) tensor on cpu"

    x = u8(2, 4, 8)
    assert _call.check_out_u8(x, x) is x
    new = _call.check_out_u8(None, x)
    assert new.shape == x.shape and new.dtype == torch.uint8 and new.data_ptr() != x.data_ptr()
    assert _call.check_out_u8(u8(64), x).numel() == 64                       # any shape of the same element count
    for bad in ([0], torch.zeros(2, 4, 8), u8(2, 4, 4), u8(2, 4, 16)[:, :, ::2], torch.zeros(2, 4, 8, dtype=torch.uint8, device="meta")):
        assert refusal(_call.check_out_u8, bad, x) == "out must be a contiguous torch.uint8 tensor of 64 elements on cpu"
    big = u8(128)
    assert refusal(_call.check_out_u8, big[32:96], big[:64]) == "out overlaps the input without being the input"
    assert refusal(_call.check_out_u8, big[:64], big[32:96]) == "out overlaps the input without being the input"
    _call.check_out_u8(big[64:], big[:64])                                   # adjacent is not overlapping

    _call.check_stats(None, 2, 9, cpu)
    _call.check_stats(torch.zeros(2, 9, dtype=torch.int32), 2, 9, cpu)
    for bad in ([0], torch.zeros(2, 9), torch.zeros(9, 2, dtype=torch.int32), torch.zeros(2, 18, dtype=torch.int32)[:, ::2],
                torch.zeros(2, 9, dtype=torch.int32, device="meta")):
        assert refusal(_call.check_stats, bad, 2, 9, cpu) == "stats must be a contiguous torch.int32 tensor (2, 9) on cpu"
    assert refusal(_call.check_stats, torch.zeros(2, 9, dtype=torch.int32), 2, 23, cpu) == "stats must be a contiguous torch.int32 tensor (2, 23) on cpu"


def test_check_arguments_refuse_a_bad_parameter_before_a_cpu_resident_tensor():
    img = u8(2, 8, 8)                                                        # well-formed, but on the CPU
    assert refusal(components.check_arguments, img, 128, 8, None) == f"images must live on {NO_CPU}"
    assert refusal(components.check_arguments, img, 0, 8, None) == "threshold = 0 outside [1, 255]"
    assert refusal(components.check_arguments, img, 128, 6, None) == "connectivity must be 4 or 8, got 6"
    assert refusal(components.check_arguments, img, 128, 8, 0) == "min_area = 0 < 1"
    assert refusal(components.check_arguments, img, 128, 8, None, 100) == "fill = 100 outside [threshold = 128, 255]: a cleaned pixel must not be ink"
    assert refusal(components.check_arguments, img, 128.0, 8, None) == "threshold must be an integer, got 128.0"
    assert refusal(components.check_arguments, u8(2, 8, 6), 0, 8, None) == "width = 6 must be a multiple of 4 in [4, 128]"     # sizes before parameters
    assert refusal(strokes.check_arguments, img, 128) == f"images must live on {NO_CPU}"
    assert refusal(strokes.check_arguments, img, 256) == "threshold = 256 outside [1, 255]"
    assert refusal(strokes.check_arguments, img, 128, 37) == "radius2 = 37 outside [0, 36]"
    assert refusal(strokes.check_arguments, img, 128, 0, 128) == "ink = 128 outside [0, threshold - 1 = 127]: a redrawn stroke must be ink"
    assert refusal(strokes.check_arguments, img, 128, 0, 0, 127) == "fill = 127 outside [threshold = 128, 255]: the paper must not be ink"
    assert refusal(strokes.check_arguments, img, 128, True) == "radius2 must be an integer, got True"
    assert refusal(strokes.check_arguments, u8(2, 200, 8), 0) == "height = 200 outside [1, 128]"


def test_every_wrapper_keeps_its_own_wording():
    img = u8(2, 16, 16)
    assert refusal(ssim.check_images, None) == "images must be a tensor or an SsimSet, got NoneType"
    assert refusal(ssim.check_images, u8(0, 16, 16), "b") == "b holds no image"
    assert refusal(ssim.check_images, u8(1, 10, 16)) == "height = 10 outside [11, 128]"
    assert refusal(ssim.check_images, img, "a") == f"a must live on {NO_CPU}"
    assert refusal(shape.shape_sums_u8, u8(2, 64, 64)) == f"byte images must live on {NO_CPU}"
    assert refusal(shape.shape_features, torch.zeros(2, 64, 32)) == "images must be square with a side in (64, 128), got 64 x 32"
    assert refusal(resize.check_images, torch.zeros(1, 8, 8), torch.float32, "grad", 128) == f"grad must live on {NO_CPU}"
    assert refusal(resize.check_images, torch.zeros(1, 8, 2000), torch.float32, "grad", 128) == "grad is 8 x 2000: sizes outside [1, 128]"
    rows = torch.zeros(4, 3)
    assert refusal(neighbors.knn, rows, rows, 1) == f"q must be a tensor on {NO_CPU}"
    assert refusal(diverse.select_diverse, rows, 2) == f"q must be a tensor on {NO_CPU}"
    assert refusal(diverse.eligibility, rows[0], 0.5) == f"scores must be a tensor on {NO_CPU}"
    assert refusal(twosample.kernel_forms, rows, torch.zeros(4, 1, dtype=torch.uint8)) == f"x must be a tensor on {NO_CPU}"
    assert refusal(twosample.kid, rows, rows) == f"real_emb must be a tensor on {NO_CPU}"


def test_all_exports_is_the_groups_in_order_without_duplicates():
    by_name = [_lib.EXPORTS, _lib.VERIFIER_EXPORTS, _lib.VERIFIER_GRAD_EXPORTS, _lib.VERIFIER_PAIRS_EXPORTS, _lib.VERIFIER_TOPK_EXPORTS,
               _lib.VERIFIER_TRAIN_EXPORTS, _lib.VERIFIER_DATA_EXPORTS, _lib.MOMENTS_EXPORTS, _lib.SELECT_EXPORTS, _lib.NEIGHBORS_EXPORTS,
               _lib.RESIZE_EXPORTS, _lib.COMPONENTS_EXPORTS, _lib.SSIM_EXPORTS, _lib.STROKES_EXPORTS, _lib.DIVERSE_EXPORTS, _lib.SHAPE_EXPORTS,
               _lib.TWOSAMPLE_EXPORTS, _lib.DTW_EXPORTS]
    assert [tuple(g) for g in _lib.GROUPS] == [tuple(e) for e in by_name]
    assert _lib.ALL_EXPORTS == tuple(name for e in by_name for name in e)
    assert len(set(_lib.ALL_EXPORTS)) == len(_lib.ALL_EXPORTS) == sum(len(e) for e in by_name)
    assert len(_lib.EXPORTS) == 64 and _lib.ALL_EXPORTS[0] == "siggan_abi_version" and _lib.ALL_EXPORTS[-1] == "siggan_dtw_pairs"
    # every *_EXPORTS tuple the module defines is a group: none can be forgotten
    named = {n for n in vars(_lib) if re.fullmatch(r"[A-Z_]*EXPORTS", n) and n != "ALL_EXPORTS"}
    assert len(named) == len(_lib.GROUPS) and {id(getattr(_lib, n)) for n in named} == {id(e) for e in by_name}
    lib = _lib.load()
    for name in _lib.ALL_EXPORTS:
        assert getattr(lib, name).argtypes is not None, name
