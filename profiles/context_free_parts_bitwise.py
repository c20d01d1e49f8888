"""Bit-for-bit comparison of two builds of the library over the context-free ops whose kernels are built from shared parts
(csrc/rows_f64.h, csrc/ink_rows.h): neighbors, twosample, components, strokes and moments.

    python profiles/context_free_parts_bitwise.py --parent PARENT.so [--new NEW.so] [--out FILE.json]

Each build runs in a fresh process of its own (the library is loaded once per process, through SIGGAN_LIB_PATH).  Every
output is recorded as its sha256; a call the library or the wrapper refuses is recorded by its message, which must be equal
too, and the entry points' own refusals are provoked one by one through the C ABI (they need no launch).  The requirement is
that every recorded value is equal.

  neighbors   (nq, nr, dim) in NEIGHBOR_SHAPES x k in 1, 3, 8, 16 x exclude_self x rows 16-byte aligned / 4 bytes past it:
              dist2 and index; ball_count per shape and layout
  twosample   n in 2, 17, 33, 70 x cols in 1, 3, 4, 257 x dim in 1, 20, 128 x rbf and poly degree 1..3, with and without diag
  components  (h, w) in IMAGE_SHAPES, two seeded random images, an all-ink and an all-paper one; connectivity 4 and 8: stats,
              roots, the cleaned copy out of place and in place
  strokes     the same images: stats, d2, skeleton, the redraw at radius2 0 and 36 out of place and in place
  moments     one update of 7 rows at dim 20 and at dim 33, then read"""
import argparse, ctypes as C, hashlib, json, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEIGHBOR_SHAPES = [(1, 1, 1), (17, 33, 3), (16, 64, 16), (33, 130, 20), (40, 200, 128)]
IMAGE_SHAPES = [(1, 4), (5, 8), (64, 64), (65, 68), (128, 128)]


def child(out_path):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import signature_gan_amd  # noqa: F401
    from signature_gan_amd import _lib, components, strokes
    from signature_gan_amd.utils import frechet, neighbors, twosample

    dev = torch.device("cuda:0")
    res = {}

    def sha(t):
        if isinstance(t, (tuple, list)):
            return [sha(v) for v in t]
        if isinstance(t, np.ndarray):
            return hashlib.sha256(np.ascontiguousarray(t).tobytes()).hexdigest()
        return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()

    def record(key, fn):
        try:
            res[key] = sha(fn())
        except Exception as e:                                       # refused: the message is the result
            res[key] = f"refused ({type(e).__name__}): {e}"

    def place(rows, offset):
        flat = torch.empty(rows.size + 1, dtype=torch.float32, device=dev)
        t = (flat[1:] if offset else flat[:-1]).view(rows.shape)
        t.copy_(torch.from_numpy(rows))
        assert t.data_ptr() % 16 == (4 if offset else 0)
        return t

    # ---- neighbors
    for nq, nr, dim in NEIGHBOR_SHAPES:
        rng = np.random.default_rng([1, nq, nr, dim])
        q, r = rng.standard_normal((nq, dim)).astype(np.float32), rng.standard_normal((nr, dim)).astype(np.float32)
        r[::7] = q[(np.arange(0, nr, 7) // 7) % nq]                  # some references are copies of queries: d2 = 0.0
        radius2 = torch.from_numpy(rng.uniform(0.5, 2.0, nr) * dim).to(dev)
        for offset in (False, True):
            qd, rd = place(q, offset), place(r, offset)
            tag = f"neighbors/{nq}x{nr}x{dim}/{'offset' if offset else 'aligned'}"
            for k in (1, 3, 8, 16):
                for excl in (False, True):
                    record(f"{tag}/k{k}/{'exclude_self' if excl else 'all'}", lambda: neighbors.knn(qd, rd, k, exclude_self=excl))
            record(f"{tag}/ball_count", lambda: neighbors.ball_count(qd, rd, radius2))

    # ---- twosample
    for n in (2, 17, 33, 70):
        for dim in (1, 20, 128):
            rng = np.random.default_rng([2, n, dim])
            rows = rng.standard_normal((n, dim)).astype(np.float32) / np.sqrt(dim)
            if n > 16:
                rows[n - 1] = rows[0]                                # a copy in another tile: k = 1.0 under the RBF kernel
            for offset in (False, True):
                x = place(rows, offset)
                for cols in (1, 3, 4, 257):
                    labels = torch.from_numpy(np.random.default_rng([3, n, cols]).integers(0, 3, (n, cols)).astype(np.uint8)).to(dev)
                    for kind, degree in (("rbf", 3), ("poly", 1), ("poly", 2), ("poly", 3)):
                        for diag in (False, True):
                            record(f"twosample/n{n}/dim{dim}/{'offset' if offset else 'aligned'}/cols{cols}/{kind}{degree if kind == 'poly' else ''}"
                                   f"/{'diag' if diag else 'forms'}",
                                   lambda: twosample.kernel_forms(x, labels, kind=kind, gamma=0.75, coef0=1.0, degree=degree, want_diag=diag))

    # ---- components and strokes
    for h, w in IMAGE_SHAPES:
        rng = np.random.default_rng([4, h, w])
        img = np.stack([rng.integers(0, 256, (h, w)), np.where(rng.random((h, w)) < 0.55, 40, 220), np.zeros((h, w)), np.full((h, w), 255)])
        u8 = torch.from_numpy(img.astype(np.uint8)).to(dev)
        for conn in (4, 8):
            tag = f"components/{h}x{w}/conn{conn}"
            record(f"{tag}/stats", lambda: components.component_stats(u8, 128, conn, 3))
            record(f"{tag}/stats_default_min_area", lambda: components.component_stats(u8, 128, conn))
            record(f"{tag}/roots", lambda: components.component_roots(u8, 128, conn))
            stats = torch.zeros(4, 9, dtype=torch.int32, device=dev)
            record(f"{tag}/clean", lambda: (components.despeckle_u8(u8, 128, conn, 3, 200, stats=stats), stats))
            mine = u8.clone()
            record(f"{tag}/clean_in_place", lambda: components.despeckle_u8(mine, 128, conn, 3, 200, out=mine))
        tag = f"strokes/{h}x{w}"
        record(f"{tag}/stats", lambda: strokes.stroke_stats(u8, 128))
        record(f"{tag}/d2", lambda: strokes.distance_map(u8, 128))
        record(f"{tag}/skeleton", lambda: strokes.skeleton_u8(u8, 128))
        for radius2 in (0, 36):
            stats = torch.zeros(4, strokes.COUNT, dtype=torch.int32, device=dev)
            record(f"{tag}/redraw{radius2}", lambda: (strokes.restroke_u8(u8, radius2, 128, 10, 240, stats=stats), stats))
            mine = u8.clone()
            record(f"{tag}/redraw{radius2}_in_place", lambda: strokes.restroke_u8(mine, radius2, 128, 10, 240, out=mine))

    # ---- moments
    for dim in (20, 33):
        m = frechet.FeatureMoments(dim, dev)
        m.update(torch.from_numpy(np.random.default_rng([5, dim]).standard_normal((7, dim)).astype(np.float32)).to(dev))
        n, s, g = m.read()
        res[f"moments/dim{dim}"] = [int(n), sha(s), sha(g)]
        m.close()

    # ---- the entry points' refusals, one by one (nothing is launched; p is a valid 4-byte aligned address)
    lib = _lib.load()
    buf = torch.zeros(64, dtype=torch.int32, device=dev)
    p, odd = buf.data_ptr(), buf.data_ptr() + 1

    def refuse(key, fn, *args):
        rc = fn(0, *args, None)
        res["refusal/" + key] = [int(rc), lib.siggan_last_error().decode() if rc else ""]

    cc = dict(u8=p, batch=1, h=8, w=8, thr=128, conn=8, area=1, fill=255, stats=p, root=None, clean=None)
    for name, change in [("null_image", dict(u8=None)), ("no_output", dict(stats=None)), ("both", dict(u8=None, stats=None)), ("batch", dict(batch=0)),
                         ("height_low", dict(h=0)), ("height_high", dict(h=129)), ("width_low", dict(w=0)), ("width_odd", dict(w=6)),
                         ("width_high", dict(w=132)), ("threshold_low", dict(thr=0)), ("threshold_high", dict(thr=256)),
                         ("connectivity", dict(conn=6)), ("min_area", dict(area=0)), ("fill_low", dict(fill=127)), ("fill_high", dict(fill=256)),
                         ("threshold_before_fill", dict(thr=0, fill=-1)), ("connectivity_before_fill", dict(conn=5, fill=0)),
                         ("fill_before_alignment", dict(fill=0, u8=odd)),
                         ("unaligned_u8", dict(u8=odd)), ("unaligned_stats", dict(stats=odd)), ("unaligned_root", dict(root=odd)),
                         ("unaligned_clean", dict(clean=odd))]:
        refuse("components/" + name, lib.siggan_components_u8, *dict(cc, **change).values())
    sk = dict(u8=p, batch=1, h=8, w=8, thr=128, radius2=0, ink=0, fill=255, stats=p, d2=None, skel=None, redraw=None)
    for name, change in [("null_image", dict(u8=None)), ("no_output", dict(stats=None)), ("batch", dict(batch=-1)), ("height_high", dict(h=129)),
                         ("width_odd", dict(w=10)), ("threshold_high", dict(thr=256)), ("radius2", dict(radius2=37)), ("ink", dict(ink=128)),
                         ("fill_low", dict(fill=127)), ("radius2_before_fill", dict(radius2=-1, fill=0)), ("ink_before_fill", dict(ink=200, fill=0)),
                         ("fill_before_alignment", dict(fill=0, stats=odd)), ("unaligned_u8", dict(u8=odd)), ("unaligned_skel", dict(skel=odd)),
                         ("unaligned_redraw", dict(redraw=odd)), ("unaligned_d2", dict(d2=odd)), ("alignment_before_d2", dict(d2=odd, stats=odd))]:
        refuse("strokes/" + name, lib.siggan_strokes_u8, *dict(sk, **change).values())
    torch.cuda.synchronize()
    with open(out_path, "w") as f:
        json.dump(res, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--new", default=os.path.join(ROOT, "signature-gan_amd", "libsiggan_hip.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "context_free_parts_bitwise.json"))
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    got = {}
    for name, path in (("parent", a.parent), ("new", a.new)):
        tmp = a.out + "." + name + ".tmp"
        env = dict(os.environ, SIGGAN_LIB_PATH=os.path.abspath(path))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tmp], env=env, capture_output=True, text=True, timeout=400)
        if p.returncode != 0:
            print(name, "FAILED", p.returncode, p.stderr[-2000:], flush=True)
            return 1
        got[name] = json.load(open(tmp))
        os.remove(tmp)
    different = sorted(k for k in set(got["parent"]) | set(got["new"]) if got["parent"].get(k) != got["new"].get(k))
    ops = sorted({k.split("/")[0] for k in got["parent"]})
    result = {
        "what": "every output of the context-free ops built from csrc/rows_f64.h and csrc/ink_rows.h, the parent commit's library against "
                "this commit's: sha256 of every output tensor, the text of every refusal",
        "not_run": "all five ops whose source or headers changed are run, although the device code of twosample, components, strokes and moments is "
                   "the parent's instruction for instruction (context_free_parts_resources.md): their host code changed.  Object files "
                   "cannot decide it -- two compilations of one unchanged source already differ byte for byte (the offload bundle "
                   "carries an id of its own).  ssim, shape, resize, select and diverse are not run: their sources did not change and "
                   "their dependency files (*.d) name neither rows_f64.h nor ink_rows.h",
        "values_per_build": {op: sum(1 for k in got["parent"] if k.split("/")[0] == op) for op in ops},
        "refused_calls": sum(1 for v in got["parent"].values() if isinstance(v, str) and v.startswith("refused")),
        "all_equal": not different,
        "different": different,
        "values": got["parent"] if not different else got,
    }
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: result[k] for k in ("values_per_build", "refused_calls", "all_equal", "different")}), flush=True)
    return 0 if not different else 1


if __name__ == "__main__":
    sys.exit(main())
