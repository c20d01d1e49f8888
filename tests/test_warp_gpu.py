"""siggan_warp_u8 on the MI355X against the numpy restatement (tests/warpcommon.py): bytes and field equal, bit for bit.
Everything is integer arithmetic, so every comparison is ==.  The launches go through the C ABI with parameter rows the
test writes (every image of a launch has its own draw id, amplitudes and base map) and through the package (warp.warp_u8,
warp.duplicate_u8)."""
import itertools

import numpy as np
import pytest
import torch

import warpcommon as W

from signature_gan_amd import _call, _lib, warp

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NS = (1, 3, 5)
GUARD = 0xA5


def amps(c):
    return (0, 1, W.max_amp(c))


def launch(src, rows, c, fill, seed, index=None, ctrl=None, want_field=True, guard=64):
    """One siggan_warp_u8 call on device copies of the numpy arguments; out (and field) sit between guard bytes, which are
    checked here.  Returns (out uint8 (n, h, w), field int32 (n, 2, h, w) or None) as numpy."""
    n, (n_src, h, w) = len(rows), src.shape
    src_t = src if isinstance(src, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(src)).to(DEV)
    rows_t = torch.from_numpy(np.ascontiguousarray(rows, np.int32)).to(DEV)
    index_t = torch.from_numpy(np.asarray(index, np.int32)).to(DEV) if index is not None else None
    ctrl_t = torch.from_numpy(np.ascontiguousarray(ctrl, np.int16)).to(DEV) if ctrl is not None else None
    buf = torch.full((2 * guard + n * h * w,), GUARD, dtype=torch.uint8, device=DEV)
    out = buf[guard:guard + n * h * w]
    fbuf = torch.full((2 * guard + 2 * n * h * w,), -7, dtype=torch.int32, device=DEV) if want_field else None
    field = fbuf[guard:guard + 2 * n * h * w] if want_field else None
    _lib.check(_lib.load().siggan_warp_u8(DEV.index, _call.ptr(src_t), n_src, _call.ptr(index_t), _call.ptr(rows_t), _call.ptr(ctrl_t),
                                          _call.ptr(out), _call.ptr(field), n, h, w, c, fill, seed, _call.stream(DEV)))
    host = buf.cpu().numpy()
    assert (host[:guard] == GUARD).all() and (host[guard + n * h * w:] == GUARD).all(), "the guard bytes around out"
    if want_field:
        fhost = fbuf.cpu().numpy()
        assert (fhost[:guard] == -7).all() and (fhost[guard + 2 * n * h * w:] == -7).all(), "the guard words around field"
        return host[guard:guard + n * h * w].reshape(n, h, w), fhost[guard:-guard].reshape(n, 2, h, w)
    return host[guard:guard + n * h * w].reshape(n, h, w), None


def restated(src, rows, c, fill, seed, index=None, ctrl=None):
    """The restatement of the same launch, image by image from its parameter row."""
    n = len(rows)
    idx = np.arange(n) if index is None else np.clip(np.asarray(index, np.int64), 0, len(src) - 1)
    u = np.asarray(rows, np.int32).view(np.uint32).astype(np.uint64)
    outs, fields = [], []
    for i in range(n):
        o, f = W.warp_one(src[idx[i]], seed, int(u[i, 0] | (u[i, 1] << np.uint64(32))), (int(rows[i][2]), int(rows[i][3])),
                          [int(v) for v in rows[i][4:10]], c, fill, None if ctrl is None else ctrl[i])
        outs.append(o)
        fields.append(f)
    return np.stack(outs), np.stack(fields).astype(np.int32)


def make_rows(n, c, h, w, draw_id, k):
    """Parameter rows of a launch: image i draws with id draw_id + i (wrapping at 2^64), amplitudes and base map cycling with
    i + k through {0, 1, max} and {identity, tilted}."""
    a = amps(c)
    ids = np.array([(draw_id + i) % (1 << 64) for i in range(n)], np.uint64)
    aff = np.array([(W.IDENTITY, W.tilted_affine(h, w))[(i + k // 4) % 2] for i in range(n)], np.int64)
    rows = warp.param_rows(ids, (0, 0), aff)
    rows[:, 2] = [a[(i + k) % 3] for i in range(n)]
    rows[:, 3] = [a[(i + k + 1) % 3] for i in range(n)]
    return rows


def indexes(n, n_src):
    """NULL; repeats; out of range on both sides (must clamp)."""
    rep = [(i // 2) % n_src for i in range(n)]
    far = [(-1, n_src, -(1 << 31), (1 << 31) - 1, n_src - 1)[i % 5] for i in range(n)]
    return (None, rep, far)


@pytest.mark.parametrize("h,w,c", W.SHAPES)
def test_bytes_and_field_equal_the_restatement(h, w, c):
    src = W.contents(h, w, seed=h + w + c)
    for k, (n, mode, (seed, draw_id)) in enumerate(itertools.product(NS, range(3), W.DRAWS)):
        rows = make_rows(n, c, h, w, draw_id, k)
        index = indexes(n, len(src))[mode]
        s = src[:n] if index is None else src
        fill = (255, 0)[(k // 2) % 2]
        out, field = launch(s, rows, c, fill, seed, index)
        want, want_field = restated(s, rows, c, fill, seed, index)
        assert np.array_equal(field, want_field), (k, n, mode, seed, draw_id)
        assert np.array_equal(out, want), (k, n, mode, seed, draw_id)


@pytest.mark.parametrize("h,w,c", [(40, 68, 16), (64, 64, 8)])
def test_every_amplitude_base_map_and_fill_on_every_content(h, w, c):
    src = W.contents(h, w, seed=5)
    ids = np.arange(100, 105, dtype=np.uint64)
    seen_outside = False
    for amp, aff, fill in itertools.product(amps(c), (W.IDENTITY, W.tilted_affine(h, w)), (0, 255)):
        rows = warp.param_rows(ids, (amp, amp), np.array([aff] * 5, np.int64))
        out, field = launch(src, rows, c, fill, 77)
        want, want_field = restated(src, rows, c, fill, 77)
        assert np.array_equal(field, want_field) and np.array_equal(out, want), (amp, aff, fill)
        assert np.abs(field).max() <= amp
        if amp == 0 and aff == W.IDENTITY:
            assert np.array_equal(out, src), "zero amplitude and the identity: a copy"
        if aff != W.IDENTITY:
            seen_outside |= bool((out[0] == fill).any() and fill == 0)    # paper (255) turned to the fill where taps fall outside
    assert seen_outside


@pytest.mark.parametrize("h,w,c", [(3, 4, 8), (5, 12, 16), (1, 4, 32), (7, 128, 32)])
def test_sizes_whose_images_are_not_16_byte_multiples(h, w, c):
    """h * w not a multiple of 16: the image is staged with dword loads; and a source that begins 4 bytes into its buffer."""
    src = np.random.default_rng(h * w).integers(0, 256, (4, h, w), dtype=np.uint8)
    rows = make_rows(4, c, h, w, 11, 1)
    rows[:, 2:4] = W.max_amp(c)
    out, field = launch(src, rows, c, 255, 3)
    want, want_field = restated(src, rows, c, 255, 3)
    assert np.array_equal(field, want_field) and np.array_equal(out, want)
    shifted = torch.zeros(4 + src.size, dtype=torch.uint8, device=DEV)
    shifted[4:] = torch.from_numpy(src.reshape(-1)).to(DEV)
    out2, _ = launch(shifted[4:].view(4, h, w), rows, c, 255, 3)
    assert np.array_equal(out2, want)


@pytest.mark.parametrize("h,w,c", [(8, 8, 8), (40, 68, 16), (128, 128, 32)])
def test_a_control_grid_handed_in(h, w, c):
    src = W.contents(h, w, seed=2)
    gy, gx = W.grid(h, w, c)
    amp = (W.max_amp(c), W.max_amp(c) // 3)
    ids = np.array([7, (1 << 32) - 1, 1 << 32, 9, 10], np.uint64)
    rows = warp.param_rows(ids, amp, np.array([W.IDENTITY] * 5, np.int64))
    drawn, drawn_field = launch(src, rows, c, 255, 9)
    ctrl = np.stack([W.control_points(9, int(d), amp, h, w, c) for d in ids]).astype(np.int16)
    rows0 = rows.copy()
    rows0[:, :4] = 0                                                 # with ctrl the draw id and the amplitudes are not read
    given, given_field = launch(src, rows0, c, 255, 1234, ctrl=ctrl)
    assert np.array_equal(given, drawn) and np.array_equal(given_field, drawn_field), "ctrl given against drawn"
    wild = np.random.default_rng(c).integers(-32768, 32768, (5, 2, gy, gx)).astype(np.int16)   # beyond +-8192: clamped
    wild[0, :, 0, 0], wild[1, :, -1, -1] = -32768, 32767
    rows0[:, 4:10] = W.tilted_affine(h, w)
    out, field = launch(src, rows0, c, 0, 0, ctrl=wild)
    want, want_field = restated(src, rows0, c, 0, 0, ctrl=wild)
    assert np.array_equal(field, want_field) and np.array_equal(out, want)
    assert np.abs(field).max() <= W.MAX_CTRL


def test_an_image_does_not_depend_on_its_place_and_runs_repeat():
    h, w, c = 64, 64, 16
    src = W.contents(h, w, seed=8)
    spec = warp.WarpSpec(cell=c, amplitude=(6.0, 3.0), rotate_deg=4, slant=0.1, scale=0.05, shift_px=2, fill=255)
    src_t = torch.from_numpy(src).to(DEV)
    ids = [5, (1 << 32) - 1, 1 << 32, (1 << 63) + 1, 0]
    big, big_field = warp.warp_u8(src_t, spec, (1 << 32) + 7, draw_ids=ids, return_field=True)
    again = warp.warp_u8(src_t, spec, (1 << 32) + 7, draw_ids=ids)
    assert torch.equal(big, again), "two runs give equal bits"
    for i in (0, 2, 4):
        alone, alone_field = warp.warp_u8(src_t[i:i + 1], spec, (1 << 32) + 7, draw_ids=[ids[i]], return_field=True)
        assert torch.equal(alone[0], big[i]) and torch.equal(alone_field[0], big_field[i])
    moved = warp.warp_u8(src_t, spec, (1 << 32) + 7, draw_ids=[ids[3], ids[1]], index=[3, 1])
    assert torch.equal(moved[0], big[3]) and torch.equal(moved[1], big[1])
    # the package's path equals the restatement too: its rows, its affine draws
    aff, _ = warp.draw_affine(spec, 5, (1 << 32) + 7, (h, w), ids)
    want, want_field = W.warp_batch(src, (1 << 32) + 7, ids, spec.amplitude_q8(), aff, c, 255)
    assert np.array_equal(big.cpu().numpy(), want) and np.array_equal(big_field.cpu().numpy(), want_field)
    assert len({bytes(a.tobytes()) for a in want}) == 5 and not np.array_equal(want[4], src[4])


def test_duplicate_u8_layout():
    h, w, c = 40, 68, 8
    src = W.contents(h, w, seed=4)[2:5]
    spec = warp.WarpSpec(cell=c, amplitude=(3.0, 2.0), fill=255)
    out, field = warp.duplicate_u8(torch.from_numpy(src).to(DEV), 3, spec, 21, first_id=(1 << 32) - 4, return_field=True)
    assert out.shape == (9, h, w) and field.shape == (9, 2, h, w)
    ids = [(1 << 32) - 4 + r for r in range(9)]
    want, want_field = W.warp_batch(src, 21, ids, spec.amplitude_q8(), [W.IDENTITY] * 9, c, 255, index=np.repeat(np.arange(3), 3))
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(field.cpu().numpy(), want_field)
    own = torch.full((9, h, w), 7, dtype=torch.uint8, device=DEV)
    assert warp.warp_u8(torch.from_numpy(src).to(DEV), spec, 21, draw_ids=ids, index=np.repeat(np.arange(3), 3), out=own) is own
    assert np.array_equal(own.cpu().numpy(), want)


def test_offsets_past_two_to_the_31():
    """More than 2^31 bytes of output: the last images of the launch are as right as the first."""
    h = w = 128
    n = (1 << 17) + 3
    src = W.contents(h, w, seed=6)
    index = np.zeros(n, np.int32)
    index[-3:] = (4, 2, 9)
    ids = np.arange(n, dtype=np.uint64)
    rows = warp.param_rows(ids, (W.max_amp(32), W.max_amp(32)), np.array([W.IDENTITY], np.int64).repeat(n, 0))
    out = torch.empty((n, h, w), dtype=torch.uint8, device=DEV)
    src_t, rows_t, index_t = torch.from_numpy(src).to(DEV), torch.from_numpy(rows).to(DEV), torch.from_numpy(index).to(DEV)
    _lib.check(_lib.load().siggan_warp_u8(DEV.index, _call.ptr(src_t), 5, _call.ptr(index_t), _call.ptr(rows_t), None, _call.ptr(out), None,
                                          n, h, w, 32, 255, 1, _call.stream(DEV)))
    pick = [0, 1, n - 3, n - 2, n - 1]
    want, _ = restated(src, rows[pick], 32, 255, 1, index[pick])
    assert np.array_equal(out[pick].cpu().numpy(), want)


def test_refusals_launch_nothing():
    spec = warp.WarpSpec()
    buf = torch.full((4, 64, 64), 9, dtype=torch.uint8, device=DEV)
    src, out = buf[:2], buf[2:]

    def refused(text, *args, **kw):
        with pytest.raises(ValueError) as e:
            warp.warp_u8(*args, **kw)
        assert str(e.value) == text
        assert bool((buf == 9).all()), "a refused call wrote"

    refused("out overlaps the images", src, spec, 0, out=buf[1:3])
    refused("out overlaps the images", buf[1:3], spec, 0, out=src)
    refused(f"out must be a contiguous torch.uint8 tensor (2, 64, 64) on {DEV}", src, spec, 0, out=buf[2:3])
    refused(f"out must be a contiguous torch.uint8 tensor (2, 64, 64) on {DEV}", src, spec, 0, out=out.cpu())
    refused("amplitude y = 1639 / 256 px outside [0, 1638 / 256] (0.4 cells of 16 px)", src, warp.WarpSpec(amplitude=(0, 1639 / 256)), 0, out=out)
    refused("cell must be one of (8, 16, 32), got 64", src, warp.WarpSpec(cell=64), 0, out=out)
    refused("width = 6 must be a multiple of 4 in [4, 128]", torch.zeros((1, 8, 6), dtype=torch.uint8, device=DEV), spec, 0)
    refused("images holds no image", src[:0], spec, 0, out=out)
    refused("images must be contiguous", buf[:, :, ::2][:2], spec, 0)
    gy, gx = W.grid(64, 64, 16)
    refused(f"ctrl must be int16 (2, 2, {gy}, {gx}), got torch.int16 (2, 2, {gy}, {gx + 1})", src, spec, 0,
            ctrl=torch.zeros((2, 2, gy, gx + 1), dtype=torch.int16, device=DEV), out=out)
    refused(f"ctrl must be a tensor on {DEV}", src, spec, 0, ctrl=torch.zeros((2, 2, gy, gx), dtype=torch.int16), out=out)
    # the C side on device pointers: the overlap, a bad cell, size and n
    lib = _lib.load()
    rows = torch.zeros((2, 12), dtype=torch.int32, device=DEV)
    for kw in (dict(out=buf[1:3]), dict(cell=12), dict(h=129), dict(w=66), dict(n=0), dict(n=(1 << 20) + 1), dict(fill=300)):
        a = dict(out=out, cell=16, h=64, w=64, n=2, fill=255)
        a.update(kw)
        rc = lib.siggan_warp_u8(DEV.index, _call.ptr(src), 2, None, _call.ptr(rows), None, _call.ptr(a["out"]), None, a["n"], a["h"], a["w"],
                                a["cell"], a["fill"], 0, _call.stream(DEV))
        assert rc == _lib.E_ARG, kw
    torch.cuda.synchronize()
    assert bool((buf == 9).all())
    assert torch.equal(warp.warp_u8(src, warp.WarpSpec(amplitude=0.0), 0, out=out), src), "and a sound call still runs"
