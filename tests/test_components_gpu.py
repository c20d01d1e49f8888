"""siggan_components_u8 on the MI355X (include/siggan_components.h, components.py) against scipy.ndimage.label.

Every comparison is exact equality of integers and bytes; there is no tolerance.  The shapes are the smallest at which the
kernel can go wrong: one row, a width of one word, widths that are no multiple of 64, one and two mask words per row, more
rows than threads per row, and 128 x 128 where the slot numbers and the areas fill their halves of the label word.  Every
case family of componentscommon.families stands at every batch index (all rotations of the family list) at batch 1, 3, 70."""
import ctypes as C

import numpy as np
import pytest
import torch

import componentscommon as CC

import signature_gan_amd  # noqa: F401
from signature_gan_amd import _lib, components

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THRESHOLD = 128
_CASES = {}


def cases(h, w, conn):
    """(names, images, [yardstick triple per image]) at the default min_area, computed once."""
    key = (h, w, conn)
    if key not in _CASES:
        fam = CC.families(h, w, THRESHOLD)
        names, images = list(fam), list(fam.values())
        for im in images:
            im.setflags(write=False)
        ma = CC.default_min_area(h, w)
        _CASES[key] = (names, images, [CC.yardstick(im, THRESHOLD, conn, ma, 255) for im in images])
    return _CASES[key]


def raw(x, conn, min_area, fill=255, threshold=THRESHOLD, stats=True, root=True, clean=True, in_place=False, poison=None):
    """One launch through the C ABI -> (rc, stats, root, clean) with None for the outputs not asked for."""
    n, h, w = x.shape
    mk = (lambda shape, dt: torch.empty(shape, dtype=dt, device=x.device)) if poison is None else \
        (lambda shape, dt: torch.full(shape, poison, dtype=dt, device=x.device))
    s = mk((n, 9), torch.int32) if stats else None
    r = mk((n, h, w), torch.int32) if root else None
    c = (x if in_place else mk((n, h, w), torch.uint8)) if clean else None
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)            # noqa: E731
    rc = _lib.load().siggan_components_u8(0, p(x), n, h, w, threshold, conn, min_area, fill, p(s), p(r), p(c),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, s, r, c


def host(t):
    return None if t is None else t.cpu().numpy()


@pytest.mark.parametrize("conn", [8, 4])
@pytest.mark.parametrize("shape", CC.GPU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stats_root_and_clean_equal_scipy_at_every_batch_index(shape, conn):
    h, w = shape
    names, images, want = cases(h, w, conn)
    ma, f = CC.default_min_area(h, w), len(images)
    for batch in (1, 3, 70):
        for rot in range(f):
            x = torch.from_numpy(CC.rotated_batch(images, batch, rot)).to(DEV)
            rc, s, r, c = raw(x, conn, ma)
            assert rc == 0, _lib.load().siggan_last_error()
            s, r, c = host(s), host(r), host(c)
            assert (s[:, CC.COMPONENTS] >= 0).all(), "the kernel's safety bound was hit"
            for i in range(batch):
                ws, wr, wc = want[(i + rot) % f]
                name = names[(i + rot) % f]
                assert np.array_equal(s[i], ws), (name, batch, i, s[i], ws)
                assert np.array_equal(r[i], wr), (name, batch, i, int((r[i] != wr).sum()))
                assert np.array_equal(c[i], wc), (name, batch, i, int((c[i] != wc).sum()))


@pytest.mark.parametrize("conn", [8, 4])
@pytest.mark.parametrize("shape", [(5, 12), (64, 64), (128, 128)], ids=lambda s: "x".join(map(str, s)))
def test_each_output_alone_in_place_and_twice(shape, conn):
    h, w = shape
    names, images, want = cases(h, w, conn)
    ma = CC.default_min_area(h, w)
    x = torch.from_numpy(np.stack(images)).to(DEV)
    rc, s, r, c = raw(x, conn, ma)
    assert rc == 0
    # the Python layer launches each output alone (the other two pointers null)
    assert torch.equal(components.component_stats(x, THRESHOLD, conn), s)
    assert torch.equal(components.component_roots(x, THRESHOLD, conn), r)
    assert torch.equal(components.despeckle_u8(x, THRESHOLD, conn), c)
    for only in ("stats", "root", "clean"):
        rc1, s1, r1, c1 = raw(x, conn, ma, stats=only == "stats", root=only == "root", clean=only == "clean")
        assert rc1 == 0
        got, ref = {"stats": (s1, s), "root": (r1, r), "clean": (c1, c)}[only]
        assert torch.equal(got, ref), only
    # a second run: identical bits
    rc2, s2, r2, c2 = raw(x, conn, ma)
    assert rc2 == 0 and torch.equal(s2, s) and torch.equal(r2, r) and torch.equal(c2, c)
    # (N, 1, H, W) keeps its rank; stats from the cleaning launch
    st = torch.zeros((len(images), 9), dtype=torch.int32, device=DEV)
    four = components.despeckle_u8(x[:, None], THRESHOLD, conn, stats=st)
    assert four.shape == (len(images), 1, h, w) and torch.equal(four[:, 0], c) and torch.equal(st, s)
    # in place equals out of place, and the input of the out-of-place call is untouched
    assert torch.equal(x.cpu(), torch.from_numpy(np.stack(images)))
    y = x.clone()
    assert components.despeckle_u8(y, THRESHOLD, conn, out=y) is y and torch.equal(y, c)
    # another fill value
    rc3, _, _, c3 = raw(x, conn, ma, fill=THRESHOLD, stats=False, root=False)
    assert rc3 == 0
    for i, im in enumerate(images):
        assert np.array_equal(host(c3)[i], CC.yardstick(im, THRESHOLD, conn, ma, THRESHOLD)[2]), names[i]


@pytest.mark.parametrize("conn", [8, 4])
@pytest.mark.parametrize("shape", [(8, 8), (64, 64), (128, 128)], ids=lambda s: "x".join(map(str, s)))
def test_properties_of_the_cleaned_image(shape, conn):
    h, w = shape
    _, images, _ = cases(h, w, conn)
    x = torch.from_numpy(np.stack(images)).to(DEV)
    for ma in (1, 2, CC.default_min_area(h, w), 9, h * w + 1):
        before = host(components.component_stats(x, THRESHOLD, conn, ma))
        clean = components.despeckle_u8(x, THRESHOLD, conn, ma)
        after = host(components.component_stats(clean, THRESHOLD, conn, ma))
        assert (before[:, CC.COMPONENTS] >= 0).all() and (after[:, CC.COMPONENTS] >= 0).all()
        assert (after[:, CC.SMALL_COMPONENTS] == 0).all() and (after[:, CC.SMALL_INK] == 0).all()
        assert np.array_equal(after[:, CC.COMPONENTS], before[:, CC.COMPONENTS] - before[:, CC.SMALL_COMPONENTS])
        assert np.array_equal(after[:, CC.INK], before[:, CC.INK] - before[:, CC.SMALL_INK])
        assert np.array_equal(after[:, CC.X0:], before[:, CC.X0:])
        kept = before[:, CC.COMPONENTS] > before[:, CC.SMALL_COMPONENTS]
        assert np.array_equal(after[kept, CC.LARGEST], before[kept, CC.LARGEST]) and (after[~kept, CC.LARGEST] == 0).all()
        assert torch.equal(components.despeckle_u8(clean, THRESHOLD, conn, ma), clean)         # a second cleaning changes no byte
        if ma == 1:
            assert torch.equal(clean, x)                                                       # nothing is smaller than one pixel
        if ma == h * w + 1:
            assert (host(clean) >= THRESHOLD).all() and (after[:, CC.X0:] == -1).all()          # everything is small


def test_other_thresholds():
    h, w = 64, 64
    img = CC.families(h, w, 128)["strokes"]
    x = torch.from_numpy(np.stack([img, 255 - img])).to(DEV)
    for thr in (1, 40, 200, 255):
        rc, s, r, c = raw(x, 8, 4, fill=255, threshold=thr)
        assert rc == 0
        for i in range(2):
            ws, wr, wc = CC.yardstick(host(x)[i], thr, 8, 4, 255)
            assert np.array_equal(host(s)[i], ws) and np.array_equal(host(r)[i], wr) and np.array_equal(host(c)[i], wc)


REFUSALS = [dict(batch=0), dict(batch=-1), dict(h=0), dict(h=129), dict(w=0), dict(w=2), dict(w=6), dict(w=132), dict(threshold=0),
            dict(threshold=256), dict(conn=6), dict(conn=0), dict(min_area=0), dict(fill=127), dict(fill=256), dict(outputs=()),
            dict(offset="u8"), dict(offset="stats"), dict(offset="root"), dict(offset="clean"), dict(null_input=True)]


@pytest.mark.parametrize("bad", REFUSALS, ids=lambda d: "-".join(f"{k}_{v}" for k, v in d.items()))
def test_refusals_return_invalid_and_leave_the_outputs_untouched(bad):
    lib = _lib.load()
    n, h, w = 2, 8, 8
    src = torch.zeros(n * h * w + 8, dtype=torch.uint8, device=DEV)
    stats = torch.full((n * 9 * 4 + 8,), 0x5a, dtype=torch.uint8, device=DEV)
    root = torch.full((n * h * w * 4 + 8,), 0x5a, dtype=torch.uint8, device=DEV)
    clean = torch.full((n * h * w + 8,), 0x5a, dtype=torch.uint8, device=DEV)
    off = bad.get("offset")
    ptrs = {"u8": src.data_ptr() + (1 if off == "u8" else 0), "stats": stats.data_ptr() + (2 if off == "stats" else 0),
            "root": root.data_ptr() + (2 if off == "root" else 0), "clean": clean.data_ptr() + (1 if off == "clean" else 0)}
    outputs = bad.get("outputs", ("stats", "root", "clean"))
    p = lambda k: C.c_void_p(ptrs[k] if (k == "u8" or k in outputs) else None)     # noqa: E731
    u8 = C.c_void_p(None) if bad.get("null_input") else p("u8")
    rc = lib.siggan_components_u8(0, u8, bad.get("batch", n), bad.get("h", h), bad.get("w", w), bad.get("threshold", 128),
                                  bad.get("conn", 8), bad.get("min_area", 4), bad.get("fill", 255), p("stats"), p("root"), p("clean"),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == _lib.E_ARG and lib.siggan_last_error()
    for t in (stats, root, clean):
        assert bool((t == 0x5a).all())
    with pytest.raises(ValueError):
        _lib.check(rc)


def test_python_layer_refuses_on_the_device_too():
    x = torch.zeros((2, 8, 8), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        components.despeckle_u8(x, 128, 8, 4, fill=127)                          # fill < threshold: the pixel would stay ink
    with pytest.raises(ValueError):
        components.component_stats(x[:, :, ::2])                                 # not contiguous
    with pytest.raises(ValueError):
        components.despeckle_u8(x, out=x.view(-1)[4:].clone()[:-4])              # wrong element count
    big = torch.zeros(2 * 64 + 4, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        components.despeckle_u8(big[:128].view(2, 8, 8), out=big[4:132].view(2, 8, 8))       # overlaps without being the input
    assert components.component_stats(x[:0]).shape == (0, 9)
