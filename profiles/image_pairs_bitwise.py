"""Bit-for-bit comparison of two builds of the library over the two ops built on the pair scaffold (csrc/image_pairs.h,
csrc/pair_plan.h): ssim and dtw.

    python profiles/image_pairs_bitwise.py --parent PARENT.so [--new NEW.so] [--out FILE.json]

Each build runs in a fresh process of its own (the library is loaded once per process, through SIGGAN_LIB_PATH).  Every
output is recorded as its sha256; a call the library or the wrapper refuses is recorded by its message, which must be equal
too, and the entry points' own refusals are provoked one by one through the C ABI (they need no launch).  The requirement is
that every recorded value is equal.

  ssim   (h, w) in SSIM_SHAPES x (na, nb) in BATCHES: the prepared maps of both sets; matrix, best and matrix_and_best in ALL and
         in SAME_SET, paired over the first min(na, nb) of both
  dtw    (h, w) in DTW_SHAPES x band in 0, the default, w - 1 x (na, nb) in BATCHES: the profiles, then the same routes

The images are seeded noise and thresholded noise with copies planted in both sets (b[1] = b[nb - 1] = a[0], a[na - 1] = a[0]
where the set is that long), so rows tie at the best value inside a split and across splits."""
import argparse, hashlib, json, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SSIM_SHAPES = [(11, 12), (16, 16), (40, 52), (64, 128), (128, 128)]
DTW_SHAPES = [(1, 4), (7, 12), (64, 64), (33, 68), (128, 128)]
BATCHES = [(1, 1), (5, 7), (17, 33), (3, 70)]


def child(out_path):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import signature_gan_amd  # noqa: F401
    from signature_gan_amd import _lib, dtw, ssim

    dev = torch.device("cuda:0")
    res = {}

    def sha(t):
        if isinstance(t, (tuple, list)):
            return [sha(v) for v in t]
        return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()

    def record(key, fn):
        try:
            res[key] = sha(fn())
        except Exception as e:                                       # refused: the message is the result
            res[key] = f"refused ({type(e).__name__}): {e}"

    def images(tag, h, w, na, nb):
        rng = np.random.default_rng([tag, h, w, na, nb])
        def some(n):
            x = rng.integers(0, 256, (n, h, w))
            x[1::2] = np.where(x[1::2] < 90, 30, 230)                # every second image: ink on paper
            return x.astype(np.uint8)
        a, b = some(na), some(nb)
        a[na - 1] = a[0]
        b[min(1, nb - 1)] = a[0]
        b[nb - 1] = a[0]
        return torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)

    def routes(tag, a, b, n_pairs, matrix, paired, best, both, first, **kw):
        record(f"{tag}/all/matrix", lambda: matrix(a, b, **kw))
        record(f"{tag}/all/best", lambda: best(a, b, **kw))
        record(f"{tag}/all/matrix_and_best", lambda: both(a, b, **kw))
        record(f"{tag}/same_set/matrix", lambda: matrix(a, **kw))
        record(f"{tag}/same_set/best", lambda: best(a, **kw))
        record(f"{tag}/same_set/matrix_and_best", lambda: both(a, **kw))
        record(f"{tag}/same_set_of_b/matrix_and_best", lambda: both(b, **kw))
        record(f"{tag}/paired", lambda: paired(first(a, n_pairs), first(b, n_pairs), **kw))

    for h, w in SSIM_SHAPES:
        for na, nb in BATCHES:
            ua, ub = images(1, h, w, na, nb)
            tag = f"ssim/{h}x{w}/{na}x{nb}"
            a, b = ssim.SsimSet(ua), ssim.SsimSet(ub)
            res[f"{tag}/maps"] = sha((a.maps, b.maps))
            routes(tag, a, b, min(na, nb), ssim.ssim_matrix, ssim.ssim_paired, ssim.ssim_best, ssim.ssim_matrix_and_best,
                   lambda s, n: ssim.SsimSet(s.u8[:n]))
    for h, w in DTW_SHAPES:
        for na, nb in BATCHES:
            ua, ub = images(2, h, w, na, nb)
            a, b = dtw.DtwSet(ua), dtw.DtwSet(ub)
            res[f"dtw/{h}x{w}/{na}x{nb}/profiles"] = sha((a.profiles, b.profiles))
            for band in sorted({0, dtw.default_band(w), w - 1}):
                routes(f"dtw/{h}x{w}/band{band}/{na}x{nb}", a, b, min(na, nb), dtw.dtw_matrix, dtw.dtw_paired, dtw.dtw_best,
                       dtw.dtw_matrix_and_best, lambda s, n: s.first(n), band=band)

    # ---- the entry points' refusals, one by one (nothing is launched; p is a valid 4-byte aligned address)
    lib = _lib.load()
    buf = torch.zeros(64, dtype=torch.int32, device=dev)
    p, odd, other = buf.data_ptr(), buf.data_ptr() + 2, buf.data_ptr() + 64

    def refuse(key, fn, *args):
        rc = fn(0, *args, None)
        res["refusal/" + key] = [int(rc), lib.siggan_last_error().decode() if rc else ""]

    sp = dict(a_u8=p, a_maps=p, na=2, b_u8=p, b_maps=p, nb=2, h=16, w=16, mode=_lib.SSIM_ALL, matrix=p, best=None, index=None)
    same, paired = dict(mode=_lib.SSIM_SAME_SET), dict(mode=_lib.SSIM_PAIRED)
    for name, change in [("na", dict(na=0)), ("nb", dict(nb=-1)), ("height_low", dict(h=10)), ("height_high", dict(h=129)), ("width_low", dict(w=8)),
                         ("width_odd", dict(w=14)), ("width_high", dict(w=132)), ("mode_low", dict(mode=-1)), ("mode_high", dict(mode=3)),
                         ("no_output", dict(matrix=None)), ("null_a_u8", dict(a_u8=None)), ("null_a_maps", dict(a_maps=None)),
                         ("null_b_u8", dict(b_u8=None)), ("null_b_maps", dict(b_maps=None)), ("same_set_nb", dict(same, nb=3)),
                         ("same_set_foreign_u8", dict(same, b_u8=other)), ("same_set_foreign_maps", dict(same, b_maps=other)),
                         ("same_set_null_b_is_no_refusal_but_alignment", dict(same, b_u8=None, b_maps=None, matrix=odd)),
                         ("paired_nb", dict(paired, nb=3)), ("paired_best", dict(paired, best=p)), ("paired_index", dict(paired, index=p)),
                         ("unaligned_a_u8", dict(a_u8=odd)), ("unaligned_a_maps", dict(a_maps=odd)), ("unaligned_b_u8", dict(b_u8=odd)),
                         ("unaligned_b_maps", dict(b_maps=odd)), ("unaligned_matrix", dict(matrix=odd)), ("unaligned_best", dict(best=odd)),
                         ("unaligned_index", dict(index=odd)),
                         # the order: an argument list wrong in several ways names the first
                         ("counts_before_size", dict(na=0, h=10)), ("size_before_mode", dict(w=14, mode=7)), ("mode_before_no_output", dict(mode=7, matrix=None)),
                         ("no_output_before_null_a", dict(matrix=None, a_u8=None)), ("null_a_before_same_set", dict(same, a_maps=None, nb=3)),
                         ("same_set_before_null_b", dict(same, nb=3, b_u8=None)), ("null_b_before_paired", dict(paired, b_u8=None, nb=3)),
                         ("paired_before_alignment", dict(paired, best=p, a_u8=odd))]:
        refuse("ssim_pairs/" + name, lib.siggan_ssim_pairs, *dict(sp, **change).values())
    pr = dict(u8=p, n=1, h=16, w=16, maps=p)
    for name, change in [("n", dict(n=0)), ("height", dict(h=10)), ("width", dict(w=18)), ("null_u8", dict(u8=None)), ("null_maps", dict(maps=None)),
                         ("unaligned_u8", dict(u8=odd)), ("unaligned_maps", dict(maps=odd)), ("null_before_alignment", dict(u8=None, maps=odd))]:
        refuse("ssim_prepare/" + name, lib.siggan_ssim_prepare_u8, *dict(pr, **change).values())
    for name, args in [("n", (0, 64, 64)), ("height", (1, 129, 64)), ("width", (1, 64, 130))]:
        rc = lib.siggan_ssim_maps_bytes(*args)
        res["refusal/ssim_maps_bytes/" + name] = [int(rc), lib.siggan_last_error().decode()]
    res["refusal/ssim_window/null"] = [int(lib.siggan_ssim_window(None)), lib.siggan_last_error().decode()]

    dp = dict(a=p, na=2, b=p, nb=2, w=16, band=2, mode=_lib.DTW_ALL, matrix=p, best=None, index=None)
    same, paired = dict(mode=_lib.DTW_SAME_SET), dict(mode=_lib.DTW_PAIRED)
    for name, change in [("na", dict(na=0)), ("nb", dict(nb=-1)), ("width_low", dict(w=0)), ("width_odd", dict(w=6)), ("width_high", dict(w=132)),
                         ("band_low", dict(band=-1)), ("band_high", dict(band=16)), ("mode_low", dict(mode=-1)), ("mode_high", dict(mode=3)),
                         ("no_output", dict(matrix=None)), ("null_a", dict(a=None)), ("null_b", dict(b=None)), ("same_set_nb", dict(same, nb=3)),
                         ("same_set_foreign", dict(same, b=other)), ("same_set_null_b_is_no_refusal_but_alignment", dict(same, b=None, matrix=odd)),
                         ("paired_nb", dict(paired, nb=3)), ("paired_best", dict(paired, best=p)), ("paired_index", dict(paired, index=p)),
                         ("unaligned_a", dict(a=odd)), ("unaligned_b", dict(b=odd)), ("unaligned_matrix", dict(matrix=odd)),
                         ("unaligned_best", dict(best=odd)), ("unaligned_index", dict(index=odd)),
                         ("counts_before_width", dict(na=0, w=6)), ("width_before_band", dict(w=6, band=-1)), ("band_before_mode", dict(band=16, mode=7)),
                         ("mode_before_no_output", dict(mode=7, matrix=None)), ("no_output_before_null_a", dict(matrix=None, a=None)),
                         ("null_a_before_same_set", dict(same, a=None, nb=3)), ("same_set_before_null_b", dict(same, nb=3, b=None)),
                         ("null_b_before_paired", dict(paired, b=None, nb=3)), ("paired_before_alignment", dict(paired, best=p, a=odd))]:
        refuse("dtw_pairs/" + name, lib.siggan_dtw_pairs, *dict(dp, **change).values())
    df = dict(u8=p, n=1, h=16, w=16, thr=128, prof=p)
    for name, change in [("null_u8", dict(u8=None)), ("null_profiles", dict(prof=None)), ("n", dict(n=0)), ("height_low", dict(h=0)),
                         ("height_high", dict(h=129)), ("width", dict(w=18)), ("threshold_low", dict(thr=0)), ("threshold_high", dict(thr=256)),
                         ("unaligned_u8", dict(u8=odd)), ("unaligned_profiles", dict(prof=odd))]:
        refuse("dtw_profiles/" + name, lib.siggan_dtw_profiles_u8, *dict(df, **change).values())
    torch.cuda.synchronize()
    with open(out_path, "w") as f:
        json.dump(res, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--new", default=os.path.join(ROOT, "signature-gan_amd", "libsiggan_hip.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_pairs_bitwise.json"))
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
    groups = sorted({k.split("/")[0] for k in got["parent"]})
    result = {
        "what": "every output of ssim and dtw, the two ops built on csrc/image_pairs.h and csrc/pair_plan.h, the parent commit's library "
                "against this commit's, both through this commit's Python wrappers: sha256 of every output tensor, the text of every refusal",
        "values_per_build": {g: sum(1 for k in got["parent"] if k.split("/")[0] == g) for g in groups},
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
