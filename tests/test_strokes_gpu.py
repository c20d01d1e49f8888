"""siggan_strokes_u8 on the MI355X (include/siggan_strokes.h, strokes.py) against the numpy restatement of
tests/strokescommon.py.

Every comparison is exact equality of integers and bytes; there is no tolerance.  The shapes are the smallest at which the
kernel can go wrong: one and two rows, a width of one word, widths that are no multiple of 64, 64 x 68 -- the first width that
needs a row's second mask word --, fewer pixels than threads, 127 x 124 and the full 128 x 128.  tests/test_strokes_cpu.py
shows that the reference alone has the properties asked for here (fixed point in one pass, 65 passes for the full image,
component counts kept)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import strokescommon as SC

import signature_gan_amd  # noqa: F401
from signature_gan_amd import _lib, components, strokes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, SENTINEL = 64, 0xA5
ALL = ("stats", "d2", "skel", "redraw")


class Outputs:
    """The four outputs of one launch, each inside a byte buffer with GUARD sentinel bytes on both sides."""

    def __init__(self, n, h, w, which=ALL, redraw_into=None):
        self.bufs, self.views = {}, {}
        for name, (shape, dt) in {"stats": ((n, 23), torch.int32), "d2": ((n, h, w), torch.int16), "skel": ((n, h, w), torch.uint8),
                                  "redraw": ((n, h, w), torch.uint8)}.items():
            if name not in which:
                continue
            if name == "redraw" and redraw_into is not None:
                self.views[name] = redraw_into
                continue
            size = int(np.prod(shape)) * torch.empty(0, dtype=dt).element_size()
            buf = torch.full((size + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
            self.bufs[name] = buf
            self.views[name] = buf[GUARD:GUARD + size].view(dt).view(shape)

    def ptr(self, name):
        return C.c_void_p(self.views[name].data_ptr() if name in self.views else None)

    def guards_intact(self):
        return all(bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all()) for b in self.bufs.values())

    def untouched(self):
        return all(bool((b == SENTINEL).all()) for b in self.bufs.values())

    def host(self, name):
        return self.views[name].cpu().numpy() if name in self.views else None


def launch(x, threshold=128, radius2=0, ink=0, fill=255, which=ALL, in_place=False):
    """One launch through the C ABI on the current stream -> Outputs (rc asserted 0)."""
    n, h, w = x.shape
    out = Outputs(n, h, w, which, redraw_into=x if in_place else None)
    rc = _lib.load().siggan_strokes_u8(0, C.c_void_p(x.data_ptr()), n, h, w, threshold, radius2, ink, fill, out.ptr("stats"), out.ptr("d2"),
                                       out.ptr("skel"), out.ptr("redraw"), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.load().siggan_last_error()
    return out


def check(out, images, names, threshold=128, radius2=0, ink=0, fill=255):
    assert out.guards_intact()
    got = {k: out.host(k) for k in ALL}
    for i, (name, img) in enumerate(zip(names, images)):
        want = dict(zip(ALL, SC.reference(img, threshold, radius2, ink, fill)))
        for k in ALL:
            if got[k] is not None:
                assert got[k][i].dtype == want[k].dtype
                assert np.array_equal(got[k][i], want[k]), (name, k, got[k][i] if k == "stats" else int((got[k][i] != want[k]).sum()), want["stats"])


@pytest.mark.parametrize("shape", SC.GPU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_output_equals_the_restatement_on_random_fillings(shape):
    fam = SC.fills(*shape)
    names, images = list(fam), list(fam.values())
    x = torch.from_numpy(np.stack(images)).to(DEV)
    check(launch(x, radius2=2), images, names, radius2=2)
    assert torch.equal(x.cpu(), torch.from_numpy(np.stack(images)))              # the input is untouched
    # the Python layer launches each output alone
    want = [SC.reference(im, 128, 2) for im in images]
    assert np.array_equal(strokes.stroke_stats(x).cpu().numpy(), np.stack([r[0] for r in want]))
    assert np.array_equal(strokes.distance_map(x).cpu().numpy(), np.stack([r[1] for r in want]))
    assert np.array_equal(strokes.skeleton_u8(x).cpu().numpy(), np.stack([r[2] for r in want]))
    four = strokes.restroke_u8(x[:, None], 2)
    assert four.shape == (len(images), 1) + shape and np.array_equal(four[:, 0].cpu().numpy(), np.stack([r[3] for r in want]))


@pytest.mark.parametrize("shape", [(5, 12), (64, 64), (128, 128)], ids=lambda s: "x".join(map(str, s)))
def test_edge_images(shape):
    fam = SC.edges(*shape)
    names, images = list(fam), list(fam.values())
    x = torch.from_numpy(np.stack(images)).to(DEV)
    out = launch(x, radius2=1)
    check(out, images, names, radius2=1)
    stats = dict(zip(names, out.host("stats")))
    assert stats["no_ink"].tolist() == [0, 0, 0, 0, 1, 0, 0] + [0] * 16
    assert stats["block_2x2"][SC.SKELETON] == 1 and stats["corner_se"][SC.SKELETON] == 1
    assert (out.host("stats")[:, SC.PASSES] >= 1).all()
    if shape == (128, 128):
        assert stats["all_ink"][SC.PASSES] == 65 == SC.reference(fam["all_ink"])[0][SC.PASSES]     # the one test of the loop bound
        assert stats["all_ink"][SC.INK] == 128 * 128 and stats["all_ink"][SC.D2_MAX] == 4096
    # bytes on both sides of other thresholds, and the two extreme thresholds on a grey ramp
    for thr in (1, 77, 255):
        both = [SC.edges(*shape, threshold=thr)["threshold_bytes"], fam["grey_ramp"]]
        check(launch(torch.from_numpy(np.stack(both)).to(DEV), threshold=thr, radius2=4, ink=0, fill=thr),
              both, ["threshold_bytes", "grey_ramp"], threshold=thr, radius2=4, ink=0, fill=thr)


def test_a_batch_equals_each_image_alone_in_any_order_on_any_stream_and_twice():
    batch = SC.mixed_batch(64, 64, 37)
    x = torch.from_numpy(batch).to(DEV)
    whole = launch(x, radius2=2)
    check(whole, list(batch), [f"mixed_{i}" for i in range(37)], radius2=2)
    for i in range(37):
        one = launch(x[i:i + 1].contiguous(), radius2=2)
        assert all(torch.equal(one.views[k][0], whole.views[k][i]) for k in ALL), i
    perm = np.random.default_rng(3).permutation(37)
    shuffled = launch(torch.from_numpy(batch[perm]).to(DEV), radius2=2)
    index = torch.from_numpy(perm).to(DEV)
    assert all(torch.equal(shuffled.views[k], whole.views[k][index]) for k in ALL)
    again = launch(x, radius2=2)
    assert all(torch.equal(again.views[k], whole.views[k]) for k in ALL)         # bit-equal from run to run
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = launch(x, radius2=2)
        stats = strokes.stroke_stats(x)
    side.synchronize()
    assert all(torch.equal(other.views[k], whole.views[k]) for k in ALL) and torch.equal(stats, whole.views["stats"])


@pytest.mark.parametrize("shape", [(5, 12), (64, 68), (128, 128)], ids=lambda s: "x".join(map(str, s)))
def test_every_combination_of_outputs_gives_the_same_bits(shape):
    images = list(SC.fills(*shape).values())[::2] + [SC.edges(*shape)["checkerboard"]]
    x = torch.from_numpy(np.stack(images)).to(DEV)
    keep = x.clone()
    whole = launch(x, radius2=4, ink=9, fill=200)
    check(whole, images, list(range(len(images))), radius2=4, ink=9, fill=200)
    for r in range(1, 4):
        for which in itertools.combinations(ALL, r):
            part = launch(x, radius2=4, ink=9, fill=200, which=which)
            assert part.guards_intact() and set(part.views) == set(which)
            assert all(torch.equal(part.views[k], whole.views[k]) for k in which), which
            assert torch.equal(x, keep), which
    for which in (("redraw",), ALL):                                              # in place: the redraw lands in the input
        y = x.clone()
        part = launch(y, radius2=4, ink=9, fill=200, which=which, in_place=True)
        assert part.guards_intact() and torch.equal(y, whole.views["redraw"])
        assert all(torch.equal(part.views[k], whole.views[k]) for k in which if k != "redraw")
    y = x.clone()
    st = torch.zeros((len(images), 23), dtype=torch.int32, device=DEV)
    assert strokes.restroke_u8(y, 4, ink=9, fill=200, out=y, stats=st) is y
    assert torch.equal(y, whole.views["redraw"]) and torch.equal(st, whole.views["stats"])


@pytest.mark.parametrize("shape", [(5, 12), (64, 68), (128, 128)], ids=lambda s: "x".join(map(str, s)))
def test_every_radius_equals_the_disc_dilation(shape):
    fam = {**SC.fills(*shape), **{k: v for k, v in SC.edges(*shape).items() if k in ("corner_nw", "corner_se", "line_east", "checkerboard")}}
    names, images = list(fam), list(fam.values())
    x = torch.from_numpy(np.stack(images)).to(DEV)
    for radius2 in SC.RADII2:
        check(launch(x, radius2=radius2, which=("redraw",)), images, names, radius2=radius2)
    skel = strokes.skeleton_u8(x)
    assert torch.equal(strokes.restroke_u8(x, 0) == 0, skel == 1)                # radius 0 is the skeleton itself


@pytest.mark.parametrize("shape", SC.GPU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_a_redraw_at_radius_0_is_a_fixed_point_and_keeps_the_components(shape):
    images = list(SC.fills(*shape).values()) + list(SC.edges(*shape).values())[:12]
    x = torch.from_numpy(np.stack(images)).to(DEV)
    before = strokes.stroke_stats(x).cpu().numpy()
    thin = strokes.restroke_u8(x, 0)
    after = strokes.stroke_stats(thin).cpu().numpy()
    assert torch.equal(strokes.skeleton_u8(thin), strokes.skeleton_u8(x))
    assert np.array_equal(after[:, SC.INK], before[:, SC.SKELETON]) and np.array_equal(after[:, SC.INK], after[:, SC.SKELETON])
    assert (after[:, SC.PASSES] == 1).all()
    assert torch.equal(strokes.restroke_u8(thin, 0), thin)
    count = lambda t: components.component_stats(t, 128, 8, 1).cpu().numpy()[:, components.COMPONENTS]      # noqa: E731
    assert np.array_equal(count(x), count(thin))
    assert np.array_equal(count(x), [SC.components8(im < 128) for im in images])


REFUSALS = [dict(batch=0), dict(batch=-1), dict(h=0), dict(h=129), dict(w=0), dict(w=2), dict(w=6), dict(w=132), dict(threshold=0),
            dict(threshold=256), dict(radius2=-1), dict(radius2=37), dict(ink=-1), dict(ink=128), dict(fill=127), dict(fill=256), dict(outputs=()),
            dict(offset="u8"), dict(offset="stats"), dict(offset="d2"), dict(offset="skel"), dict(offset="redraw"), dict(null_input=True)]


@pytest.mark.parametrize("bad", REFUSALS, ids=lambda d: "-".join(f"{k}_{v}" for k, v in d.items()))
def test_refusals_return_invalid_and_leave_the_outputs_untouched(bad):
    lib = _lib.load()
    n, h, w = 2, 8, 8
    src = torch.zeros(n * h * w + 8, dtype=torch.uint8, device=DEV)
    out = Outputs(n, h, w)
    off = bad.get("offset")
    step = {"u8": 1, "stats": 2, "d2": 1, "skel": 1, "redraw": 2}
    outputs = bad.get("outputs", ALL)
    p = lambda k: C.c_void_p(out.views[k].data_ptr() + (step[k] if off == k else 0)) if k in outputs else C.c_void_p(None)     # noqa: E731
    u8 = C.c_void_p(None) if bad.get("null_input") else C.c_void_p(src.data_ptr() + (step["u8"] if off == "u8" else 0))
    rc = lib.siggan_strokes_u8(0, u8, bad.get("batch", n), bad.get("h", h), bad.get("w", w), bad.get("threshold", 128), bad.get("radius2", 1),
                               bad.get("ink", 0), bad.get("fill", 255), p("stats"), p("d2"), p("skel"), p("redraw"),
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == _lib.E_ARG and lib.siggan_last_error()
    assert out.untouched()
    with pytest.raises(ValueError):
        _lib.check(rc)


def test_python_layer_refuses_on_the_device_too():
    x = torch.zeros((2, 8, 8), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        strokes.restroke_u8(x, 0, fill=127)                                      # fill < threshold: the paper would be ink
    with pytest.raises(ValueError):
        strokes.stroke_stats(x[:, :, ::2])                                       # not contiguous
    with pytest.raises(ValueError):
        strokes.restroke_u8(x, 0, out=x.view(-1)[4:].clone()[:-4])               # wrong element count
    with pytest.raises(ValueError):
        strokes.restroke_u8(x, 0, stats=torch.zeros((2, 9), dtype=torch.int32, device=DEV))
    big = torch.zeros(2 * 64 + 4, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        strokes.restroke_u8(big[:128].view(2, 8, 8), 0, out=big[4:132].view(2, 8, 8))        # overlaps without being the input
    assert strokes.stroke_stats(x[:0]).shape == (0, 23) and strokes.restroke_u8(x[:0], 0).shape == (0, 8, 8)
