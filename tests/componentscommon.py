"""Connected components of byte images, three times over, and the images they are tried on.

``yardstick``  scipy.ndimage.label (structure ones((3, 3)) for 8-connectivity, the default cross for 4), areas from bincount,
               boxes from find_objects, its labels mapped to "smallest linear index of the component".
``flood``      an independent restatement: a plain stack flood fill over pixels, nothing shared with scipy or the kernel.
``emulate``    the kernel's own method (csrc/components.hip) with its data structures: one 128-bit mask per row, run slots
               y * (w / 2) + (x >> 1), one word per slot that holds the link and, for a root, the area in its high half, joins
               by atomic min towards the smaller slot, then one pass that replaces links by roots and adds the areas.  The 512 threads run in LOCK STEP: every tick each live thread performs
               one LDS access (a read of lab[], an atomic min, a store), in thread order, in reverse order or in an order
               shuffled anew every tick -- the result must not depend on it.  It counts what the kernel bounds: the longest
               chain a find walked and the most retries a join needed.

All three return (stats (9,) int32, root (h, w) int32, clean (h, w) uint8) in the layout of include/siggan_components.h.
``families`` generates the cases the issue lists, for any height 1..128 and width 4..128 (a multiple of 4)."""
import random

import numpy as np
from PIL import Image, ImageDraw, ImageFilter
from scipy import ndimage

INK, COMPONENTS, LARGEST, SMALL_COMPONENTS, SMALL_INK, X0, Y0, X1, Y1, COUNT = range(10)
THREADS = 512
GPU_SHAPES = [(1, 4), (5, 12), (8, 8), (64, 64), (128, 64), (64, 128), (128, 128)]


def default_min_area(h, w):
    return max(2, int(round(0.001 * h * w)))


# ---------------------------------------------------------------------------------------------------------- yardstick
def _finish(img, lbl_root, areas_of_root, min_area, fill):
    """stats / clean from a root map and {root: area}."""
    h, w = img.shape
    stats = np.zeros(COUNT, dtype=np.int32)
    stats[X0:] = -1
    clean = img.copy()
    areas = np.array(sorted(areas_of_root.values()), dtype=np.int64)
    stats[INK] = int(areas.sum())
    stats[COMPONENTS] = len(areas)
    stats[LARGEST] = int(areas.max()) if len(areas) else 0
    stats[SMALL_COMPONENTS] = int((areas < min_area).sum())
    stats[SMALL_INK] = int(areas[areas < min_area].sum())
    small_roots = np.array([r for r, a in areas_of_root.items() if a < min_area], dtype=np.int64)
    small = np.isin(lbl_root, small_roots)
    kept = (lbl_root >= 0) & ~small
    if kept.any():
        ys, xs = np.nonzero(kept)
        stats[X0], stats[Y0], stats[X1], stats[Y1] = xs.min(), ys.min(), xs.max(), ys.max()
    clean[small] = fill
    return stats, lbl_root.astype(np.int32), clean


def yardstick(img, threshold=128, connectivity=8, min_area=1, fill=255):
    h, w = img.shape
    ink = img < threshold
    lbl, n = ndimage.label(ink, structure=np.ones((3, 3), dtype=int) if connectivity == 8 else None)
    stats = np.zeros(COUNT, dtype=np.int32)
    stats[X0:] = -1
    root = np.full((h, w), -1, dtype=np.int32)
    clean = img.copy()
    if n == 0:
        return stats, root, clean
    areas = np.bincount(lbl.ravel(), minlength=n + 1)[1:]
    first = np.asarray(ndimage.minimum(np.arange(h * w).reshape(h, w), lbl, index=np.arange(1, n + 1))).astype(np.int64)
    root = np.where(lbl > 0, first[np.maximum(lbl, 1) - 1], -1).astype(np.int32)
    small = areas < min_area
    stats[INK], stats[COMPONENTS], stats[LARGEST] = areas.sum(), n, areas.max()
    stats[SMALL_COMPONENTS], stats[SMALL_INK] = small.sum(), areas[small].sum()
    boxes = [b for b, s in zip(ndimage.find_objects(lbl), small) if not s]
    if boxes:
        stats[X0], stats[Y0] = min(b[1].start for b in boxes), min(b[0].start for b in boxes)
        stats[X1], stats[Y1] = max(b[1].stop for b in boxes) - 1, max(b[0].stop for b in boxes) - 1
    clean[(lbl > 0) & small[np.maximum(lbl, 1) - 1]] = fill
    return stats, root, clean


def flood(img, threshold=128, connectivity=8, min_area=1, fill=255):
    h, w = img.shape
    ink = (img < threshold).tolist()
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    root = [[-1] * w for _ in range(h)]
    areas = {}
    for y in range(h):
        for x in range(w):
            if not ink[y][x] or root[y][x] >= 0:
                continue
            r = y * w + x                     # raster order: the first pixel met is the component's smallest linear index
            root[y][x] = r
            stack, area = [(y, x)], 0
            while stack:
                cy, cx = stack.pop()
                area += 1
                for dy, dx in steps:
                    ny, nx = cy + dy, cx + dx
                    if 0 <= ny < h and 0 <= nx < w and ink[ny][nx] and root[ny][nx] < 0:
                        root[ny][nx] = r
                        stack.append((ny, nx))
            areas[r] = area
    return _finish(img, np.array(root, dtype=np.int64).reshape(h, w), areas, min_area, fill)


# ---------------------------------------------------------------------------------------------------------- emulation
def _ctz(v):
    return (v & -v).bit_length() - 1


def _below(n):
    return (1 << max(n, 0)) - 1


def _starts(m):
    return m & ~(m << 1)


def _run_end(m, s, w):
    e = s
    while e < w and (m >> e) & 1:
        e += 1
    return e


def emulate(img, threshold=128, connectivity=8, min_area=1, fill=255, order="forward"):
    """-> (stats, root, clean, info); info: runs, nodes, find_steps (longest chain walked), retries (most retries of one
    join), ticks (lock-step rounds of the join phase), bound_hit."""
    h, w = img.shape
    assert 1 <= h <= 128 and 4 <= w <= 128 and w % 4 == 0
    wh, c8 = w // 2, 1 if connectivity == 8 else 0
    nodes = h * wh
    masks = [sum(1 << x for x in np.nonzero(row < threshold)[0].tolist()) for row in img]        # the ballots
    lab = list(range(nodes))
    info = {"runs": 0, "nodes": nodes, "find_steps": 0, "retries": 0, "ticks": 0, "bound_hit": False}

    def start_of(slot):
        y, k = divmod(slot, wh)
        two = (_starts(masks[y]) >> (2 * k)) & 3
        return (y, None) if not two else (y, 2 * k + (0 if two & 1 else 1))

    def find(x):
        steps = 0
        while True:
            yield                                               # one LDS read
            p = lab[x] & 0xffff                                 # (the high half holds an area once the second phase runs)
            if p == x:
                info["find_steps"] = max(info["find_steps"], steps)
                return x
            if steps >= nodes:
                info["bound_hit"] = True
                return x
            x = p
            steps += 1

    def join(a, b):
        tries = 0
        while True:
            a0, b0 = a, b
            a = yield from find(a)
            b = yield from find(b)
            if a != a0:
                yield                                           # LDS atomic min: the start of the chain now points at its root
                lab[a0] = min(lab[a0], a)
            if b != b0:
                yield
                lab[b0] = min(lab[b0], b)
            if a == b or info["bound_hit"]:
                break
            if a < b:
                a, b = b, a
            yield                                               # the LDS atomic min
            old = lab[a]
            lab[a] = min(old, b)
            if old == a:
                break
            if tries >= 2 * nodes:
                info["bound_hit"] = True
                break
            tries += 1
            a = old
        info["retries"] = max(info["retries"], tries)

    def join_thread(tid):
        for slot in range(wh + tid, nodes, THREADS):
            y, s = start_of(slot)
            if s is None:
                continue
            m, up = masks[y], masks[y - 1]
            e = _run_end(m, s, w)
            touch = up & _below(e + c8) & ~_below(s - c8)
            while touch:
                b = _ctz(touch)
                us = (_starts(up) & _below(b + 1)).bit_length() - 1
                yield from join(slot, (y - 1) * wh + (us >> 1))
                touch &= ~_below(_run_end(up, b, w))

    def flatten_thread(tid):
        for slot in range(tid, nodes, THREADS):
            y, s = start_of(slot)
            if s is None:
                continue
            r = yield from find(slot)
            if r != slot:
                yield                                           # the store
                lab[slot] = r
            yield                                               # the LDS atomic add: the run's length into the root's high half
            lab[r] += (_run_end(masks[y], s, w) - s) << 16

    def lock_step(make, count_ticks):
        live = [make(t) for t in range(THREADS)]
        rng = random.Random(order) if order not in ("forward", "reverse") else None
        while live:
            if order == "reverse":
                seq = live[::-1]
            elif rng is not None:
                seq = live[:]
                rng.shuffle(seq)
            else:
                seq = live
            done = set()
            for g in seq:
                try:
                    next(g)
                except StopIteration:
                    done.add(id(g))
            live = [g for g in live if id(g) not in done]
            if count_ticks:
                info["ticks"] += 1

    lock_step(join_thread, True)
    lock_step(flatten_thread, False)

    stats = np.zeros(COUNT, dtype=np.int32)
    stats[X0:] = -1
    root = np.full((h, w), -1, dtype=np.int32)
    clean = img.copy()
    if info["bound_hit"]:
        stats[COMPONENTS] = -1
        return stats, root, clean, info
    runs = []
    for slot in range(nodes):
        y, s = start_of(slot)
        if s is not None:
            runs.append((slot, y, s, _run_end(masks[y], s, w)))
    info["runs"] = len(runs)
    x0 = y0 = 1 << 30
    x1 = y1 = -1
    for slot, y, s, e in runs:
        r = lab[slot] & 0xffff
        area = lab[r] >> 16
        stats[INK] += e - s
        if r == slot:
            stats[COMPONENTS] += 1
            stats[LARGEST] = max(stats[LARGEST], area)
            if area < min_area:
                stats[SMALL_COMPONENTS] += 1
                stats[SMALL_INK] += area
        if area >= min_area:
            x0, x1, y0, y1 = min(x0, s), max(x1, e - 1), min(y0, y), max(y1, y)
        ry, rs = start_of(r)
        root[y, s:e] = ry * w + rs
        if area < min_area:
            clean[y, s:e] = fill
    if x1 >= 0:
        stats[X0], stats[Y0], stats[X1], stats[Y1] = x0, y0, x1, y1
    return stats, root, clean, info


# -------------------------------------------------------------------------------------------------------------- cases
def render(ink, threshold, seed):
    """A bool ink mask as bytes: ink anywhere in [0, threshold), background anywhere in [threshold, 255]."""
    rng = np.random.default_rng(seed)
    lo = rng.integers(0, threshold, ink.shape)
    hi = rng.integers(threshold, 256, ink.shape)
    return np.where(ink, lo, hi).astype(np.uint8)


def _spiral(h, w):
    g = np.zeros((h, w), dtype=bool)
    y = x = 0
    dy, dx = 0, 1
    g[0, 0] = True

    def free(cy, cx, ddy, ddx):
        ny, nx = cy + ddy, cx + ddx
        if not (0 <= ny < h and 0 <= nx < w) or g[ny, nx]:
            return False
        my, mx = ny + ddy, nx + ddx                              # keep a one-pixel gap to the previous turn of the spiral
        if 0 <= my < h and 0 <= mx < w and g[my, mx]:
            return False
        return True

    turns = 0
    while turns < 2:
        if free(y, x, dy, dx):
            y, x = y + dy, x + dx
            g[y, x] = True
            turns = 0
        else:
            dy, dx = dx, -dy
            turns += 1
    return g


def _blob(n, width):
    """n pixels filling rows of `width` from the left: one 4-connected component."""
    rows = (n + width - 1) // width
    g = np.zeros((rows, width), dtype=bool)
    g.ravel()[:n] = True
    return g


def _strokes(h, w, seed):
    rng = np.random.default_rng(seed)
    scale = 4
    im = Image.new("L", (w * scale, h * scale), 255)
    d = ImageDraw.Draw(im)
    for _ in range(3):
        pts = [(int(rng.integers(0, w * scale)), int(rng.integers(0, h * scale))) for _ in range(5)]
        d.line(pts, fill=0, width=int(rng.integers(2, 7)))
    for _ in range(6):                                           # specks
        px, py = int(rng.integers(0, w * scale)), int(rng.integers(0, h * scale))
        d.ellipse([px, py, px + 3, py + 3], fill=int(rng.integers(0, 100)))
    im = im.filter(ImageFilter.GaussianBlur(2.0)).resize((w, h), Image.BILINEAR)
    return np.asarray(im, dtype=np.uint8).copy()


def families(h, w, threshold=128, min_area=None, seed=0):
    """{name: uint8 (h, w)} -- every family of the issue's list at this shape."""
    min_area = default_min_area(h, w) if min_area is None else min_area
    yy, xx = np.mgrid[0:h, 0:w]
    z = lambda: np.zeros((h, w), dtype=bool)                     # noqa: E731
    out = {}
    out["empty"] = z()
    out["full"] = ~z()
    g = z(); g[0, 0] = g[0, w - 1] = g[h - 1, 0] = g[h - 1, w - 1] = True
    out["corners"] = g
    g = z(); g[0, 0] = True; g[min(1, h - 1), 1] = True
    out["diagonal_pair"] = g
    out["checkerboard"] = (yy + xx) % 2 == 0
    g = z(); g[0::2] = True
    for y in range(1, h, 2):
        g[y, w - 1 if (y >> 1) % 2 == 0 else 0] = True
    out["serpentine"] = g
    g = z(); g[:, 0::2] = True
    for x in range(1, w, 2):
        g[h - 1 if (x >> 1) % 2 == 0 else 0, x] = True
    out["serpentine_columns"] = g
    out["spiral"] = _spiral(h, w)
    g = z(); g[:, 0::2] = True; g[:h - 1, 1::2] = False; g[h - 1] = True
    out["comb"] = g
    g = z()                                                      # a U, a ring and an arch side by side
    a, b, c = 0, w // 3, 2 * w // 3
    g[:, a] = True; g[:, max(b - 2, a)] = True; g[h - 1, a:max(b - 1, a + 1)] = True
    g[0, b:c - 1] = g[h - 1, b:c - 1] = True; g[:, b] = True; g[:, max(c - 2, b)] = True
    g[:, c] = True; g[:, w - 1] = True; g[0, c:] = True
    if h >= 4:                                                   # children on both arms before they meet
        g[1:h - 1:2, a + 1:max(b - 2, a + 1):2] = True
    out["u_ring_arch"] = g
    g = z(); mid = min(64, w // 2)
    rows = [(0, mid - 4, mid), (2, mid, mid + 4), (4, mid - 2, mid + 2), (6, 0, w), (8, mid - 1, mid), (10, mid, mid + 1), (11, mid - 1, mid + 1),
            (13, mid - 1, mid), (14, mid, mid + 1)]
    for y, s, e in rows:
        if y < h:
            g[y, max(s, 0):min(e, w)] = True
    out["word_border"] = g
    g = z(); g[h // 2] = True; g[:, w // 2] = True
    if h >= 8 and w >= 8:
        g[1, 1] = g[h - 2, w - 2] = g[1, w - 2] = True
    out["borders"] = g
    rng = np.random.default_rng(seed + 17 * h + w)
    for p in (0.1, 0.3, 0.5, 0.6):
        out[f"noise_{p}"] = rng.random((h, w)) < p
    g = z(); y = 0                                               # components of min_area - 1, min_area, min_area + 1 pixels
    for n in (min_area - 1, min_area, min_area + 1):
        if n < 1:
            continue
        blob = _blob(n, max(1, min(w // 2, 5)))
        if y + blob.shape[0] <= h:
            g[y:y + blob.shape[0], 1:1 + blob.shape[1]] |= blob[:, :w - 1]
            y += blob.shape[0] + 1
    out["around_min_area"] = g
    imgs = {k: render(v, threshold, seed + i) for i, (k, v) in enumerate(out.items())}
    imgs["strokes"] = _strokes(h, w, seed + 5)
    imgs["strokes_2"] = _strokes(h, w, seed + 6)
    return imgs


def rotated_batch(images, batch, rotation):
    """(batch, h, w): image i is images[(i + rotation) % len(images)] -- over all rotations every image stands at every index."""
    return np.stack([images[(i + rotation) % len(images)] for i in range(batch)])
