"""siggan_preprocess_u8 on the MI355X (include/siggan_preprocess.h, preprocess.py) against the numpy / scipy restatement of
tests/preprocesscommon.py.

Every comparison is exact equality of bytes and integers; there is no tolerance.  One ragged batch holds every scan of
preprocesscommon.world() back to back: 16 x 16 up to 1024 x 1024, odd widths (so offsets are unaligned and tiles partial),
the 1024 x 16 and 16 x 1024 strips, the comb and the spiral at 300 x 300 and the other planted cases.  The restatement of a
configuration is computed once and shared."""
import ctypes as C

import numpy as np
import pytest
import torch

import preprocesscommon as PC

import signature_gan_amd  # noqa: F401
from signature_gan_amd import _lib, preprocess

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_BATCH = []


def world_batch():
    if not _BATCH:
        _BATCH.append(preprocess.pack_scans([a for _, a in PC.world()], DEV))
    return _BATCH[0]


def run(batch, T=64, poison=None, **flags):
    """One call -> (out, stats, [denoised scan], canvas) on the host."""
    mk = (lambda shape, dt: torch.empty(shape, dtype=dt, device=DEV)) if poison is None else \
        (lambda shape, dt: torch.full(shape, poison, dtype=dt, device=DEV))
    den, canvas = mk((batch.total_pixels,), torch.uint8), mk((batch.n, T, T), torch.uint8)
    out, stats = preprocess.preprocess_scans(batch, T, denoised=den, canvas=canvas, **flags)
    return out.cpu().numpy(), stats.cpu().numpy(), [batch.scan(i, den).cpu().numpy() for i in range(batch.n)], canvas.cpu().numpy()


def flags_of(cfg):
    return {"denoise" if k == "denoise_on" else k: v for k, v in cfg.items()}


def compare(got, want, names, what):
    out, stats, den, canvas = got
    assert not (stats[:, PC.STATUS] & PC.OVERFLOW).any(), "the labelling's safety bound was hit"
    for i, (name, w) in enumerate(zip(names, want)):
        assert np.array_equal(stats[i], w["stats"]), (what, name, stats[i].tolist(), w["stats"].tolist())
        assert np.array_equal(den[i], w["denoised"]), (what, name, int((den[i] != w["denoised"]).sum()))
        assert np.array_equal(canvas[i], w["canvas"]), (what, name, int((canvas[i] != w["canvas"]).sum()))
        assert np.array_equal(out[i], w["out"]), (what, name, int((out[i] != w["out"]).sum()))


@pytest.mark.parametrize("T", [64, 128])
def test_out_stats_denoised_and_canvas_equal_the_restatement(T):
    names = [n for n, _ in PC.world()]
    compare(run(world_batch(), T), PC.expected(T), names, f"T = {T}")


OFF = [dict(denoise_on=False), dict(crop=False), dict(center=False), dict(equalize=False),
       dict(denoise_on=False, crop=False, center=False, equalize=False)]


@pytest.mark.parametrize("cfg", OFF, ids=lambda c: "no_" + "_".join(k.replace("_on", "") for k in c))
def test_each_stage_off_alone_and_all_four_off(cfg):
    names = [n for n, _ in PC.world()]
    compare(run(world_batch(), 64, **flags_of(cfg)), PC.expected(64, **cfg), names, str(cfg))
    if len(cfg) == 4:
        compare(run(world_batch(), 128, **flags_of(cfg)), PC.expected(128, **cfg), names, f"T = 128, {cfg}")


def test_other_margins_and_min_pixels():
    scans = dict(PC.world())
    picks = ["specks", "pen_96x61", "corner_br", "threshold"]
    for margin, mp in ((0, None), (64, None), (5, 1), (5, 10), (5, 12), (3, 40)):
        b = preprocess.pack_scans([scans[n] for n in picks], DEV, min_pixels=mp)
        want = [PC.restate(scans[n], 64, denoise_on=False, margin=margin, min_px=mp) for n in picks]
        compare(run(b, 64, denoise=False, margin=margin), want, picks, f"margin {margin}, min_pixels {mp}")


def test_a_scan_alone_gives_the_bytes_it_gives_in_the_batch():
    both = {T: run(world_batch(), T) for T in (64, 128)}
    for i, (name, a) in enumerate(PC.world()):
        single = preprocess.pack_scans([a], DEV)
        for T in (64, 128):
            out, stats, den, canvas = run(single, T)
            o, s, d, c = both[T]
            assert np.array_equal(out[0], o[i]) and np.array_equal(stats[0], s[i]) and np.array_equal(den[0], d[i]) and \
                np.array_equal(canvas[0], c[i]), (name, T)


def test_two_runs_a_dirty_workspace_and_a_reused_batch_give_equal_bytes():
    b = world_batch()
    first = run(b, 64)
    second = run(b, 64, poison=0x5a)
    b.workspace.fill_(0xff)
    third = run(b, 64)
    b.workspace.copy_(torch.from_numpy(np.random.RandomState(5).randint(0, 256, b.workspace.numel(), dtype=np.uint8)))
    run(b, 128)                                      # another target in between, on the same batch
    fourth = run(b, 64, crop=True)
    for other in (second, third, fourth):
        assert np.array_equal(first[0], other[0]) and np.array_equal(first[1], other[1]) and np.array_equal(first[3], other[3])
        assert all(np.array_equal(x, y) for x, y in zip(first[2], other[2]))
    assert np.array_equal(b.pool.cpu().numpy(), np.concatenate([a.reshape(-1) for _, a in PC.world()]))        # the input is untouched


def test_out_and_stats_supplied_by_the_caller():
    b = world_batch()
    want_out, want_stats = preprocess.preprocess_scans(b, 128)
    out = torch.full((b.n, 128, 128), 7, dtype=torch.uint8, device=DEV)
    stats = torch.full((b.n, 13), -7, dtype=torch.int32, device=DEV)
    got_out, got_stats = preprocess.preprocess_scans(b, 128, out=out, stats=stats)
    assert got_out is out and got_stats is stats and torch.equal(out, want_out) and torch.equal(stats, want_stats)
    # without denoised= / canvas= the result is the same
    compare((want_out.cpu().numpy(), want_stats.cpu().numpy()) + run(b, 128)[2:], PC.expected(128), [n for n, _ in PC.world()], "no taps")
    v = preprocess.validity(want_stats, b.geom_host)
    assert np.array_equal(v, preprocess.validity(want_stats.cpu().numpy(), b.geom))
    assert np.array_equal(v, [PC.is_valid(int(r["stats"][PC.WHITE]), a.size) for (_, a), r in zip(PC.world(), PC.expected(128))])


def test_a_pool_with_gaps_and_denoised_bytes_between_scans_untouched():
    scans = [a for n, a in PC.world() if n in ("pen_17x23", "pen_65x130", "diagonal", "texture")]
    gaps = [3, 1, 70, 9]
    geom, parts, off = [], [], 0
    for a, g in zip(scans, gaps):
        parts.append(np.full(g, 0xa5, np.uint8)); off += g
        geom.append((off, a.shape[0], a.shape[1], PC.min_pixels(*a.shape)))
        parts.append(a.reshape(-1)); off += a.size
    parts.append(np.full(5, 0xa5, np.uint8)); off += 5
    gh = torch.tensor(geom, dtype=torch.int64)
    b = preprocess.ScanBatch(torch.from_numpy(np.concatenate(parts)).to(DEV), gh.to(DEV), gh,
                             torch.empty(preprocess.workspace_bytes(off, len(scans)), dtype=torch.uint8, device=DEV))
    got = run(b, 64, poison=0x3c)
    compare(got, [PC.restate(a, 64) for a in scans], ["17x23", "65x130", "diagonal", "texture"], "gaps")
    den = torch.full((off,), 0x3c, dtype=torch.uint8, device=DEV)
    preprocess.preprocess_scans(b, 64, denoised=den)
    den = den.cpu().numpy()
    inside = np.zeros(off, dtype=bool)
    for o, h, w, _ in geom:
        inside[o:o + h * w] = True
    assert (den[~inside] == 0x3c).all() and int((~inside).sum()) == sum(gaps) + 5


def test_refusals_on_the_device_leave_the_outputs_untouched():
    b = preprocess.pack_scans([np.zeros((16, 16), np.uint8), np.full((20, 16), 255, np.uint8)], DEV)
    out = torch.full((2, 64, 64), 0x5a, dtype=torch.uint8, device=DEV)
    stats = torch.full((2, 13), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
    for kw, words in [(dict(out=out[:1]), "out must be a contiguous torch.uint8 tensor \\(2, 64, 64\\)"),
                      (dict(out=out.cpu()), "out must be a contiguous torch.uint8 tensor"),
                      (dict(stats=stats.float()), "stats must be a contiguous torch.int32 tensor \\(2, 13\\)"),
                      (dict(canvas=torch.zeros((2, 128, 128), dtype=torch.uint8, device=DEV)), "canvas must be"),
                      (dict(denoised=torch.zeros(16 * 16 + 20 * 16 + 1, dtype=torch.uint8, device=DEV)), "denoised must be"),
                      (dict(out=torch.zeros((2, 64, 128), dtype=torch.uint8, device=DEV)[:, :, ::2]), "out must be a contiguous")]:
        with pytest.raises(ValueError, match=words):
            preprocess.preprocess_scans(b, 64, **kw)
    lib = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())           # noqa: E731
    bad_geom = b.geom_host.clone()
    bad_geom[1, 0] = 255                             # overlaps scan 0 by one byte
    for geom_host, opt, ws_bytes in ((bad_geom, (64, 1, 1, 1, 1, 5), b.workspace.numel()), (b.geom_host, (32, 1, 1, 1, 1, 5), b.workspace.numel()),
                                     (b.geom_host, (64, 1, 1, 1, 1, 5), b.workspace.numel() - 1)):
        rc = lib.siggan_preprocess_u8(0, p(b.pool), b.total_pixels, p(geom_host), p(b.geom), 2, _lib.PreprocessOptions(*opt), p(out), p(stats),
                                      None, None, p(b.workspace), ws_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == _lib.E_ARG and lib.siggan_last_error()
        with pytest.raises(ValueError):
            _lib.check(rc)
    assert bool((out == 0x5a).all()) and bool((stats == 0x5a5a5a5a).all())
    got, st = preprocess.preprocess_scans(b, 64, out=out, stats=stats)               # and the same tensors are then filled
    st = st.cpu().numpy()
    assert st[0, PC.WHITE] == 0 and st[1, PC.WHITE] == 320 and st[1, PC.STATUS] == PC.NO_BBOX and st[0, PC.KEPT] == 1
