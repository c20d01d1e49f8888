#!/usr/bin/env python3
"""Time of the per-row top-k lists (siggan_verifier_pairs_topk) on the MI355X against the row-maxima call they grew out of and
against the route they replace.

    python profiles/pairs_topk_throughput.py [--parent_lib PATH] [--out profiles/pairs_topk_throughput.json]

n unit-norm rows of dim 128, n / 16 writers, a SiameseNetwork(128) with torch's default initialisation (seeded); one set against
itself (same_set), n = 4096 and n = 16384, all n^2 ordered pairs scored by every route:
  "topk_k1" / "topk_k4" / "topk_k16"   ONE siggan_verifier_pairs_topk call (PAIR_TOPK_CHUNK raised to n): both classes, the
                     genuine list lowest-first -- the tile kernel's LIST instantiation plus the merge kernel
  "topk_k16_chunked" SiameseNetwork.pair_topk as shipped at n = 16384: four chunks of 4096 queries, each as three calls (the rows
                     before, the chunk's own rows with same_set, the rows after) merged by two torch sorts
  "best"             the existing SiameseNetwork.pairs(want_best=True) of THIS build (its instantiations compile from unchanged
                     expressions; profiles/pairs_topk_resources.md)
  "best_parent"      the same call on a second model whose context lives in --parent_lib, a build of the parent commit loaded
                     beside this build's library (it lacks the new symbols, so it is bound by hand); absent without --parent_lib
  "matrix_topk"      score_matrix + two masked torch.topk(k = 16): the (n, n) matrix is written and read back three times
Device events around each call; WARMUP calls, then CALLS windows alternating between the routes; medians with min and max.
Needs the GPU; there is no fallback."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import signature_gan_amd  # noqa: E402,F401
from signature_gan_amd import _lib  # noqa: E402
from signature_gan_amd import signature_verifier_eval as SV  # noqa: E402

DIM = 128
WARMUP, CALLS = 3, 10
SIZES = (4096, 16384)


def unit_rows(n, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(n, DIM, generator=g, dtype=torch.float64)
    return (x / x.norm(dim=1, keepdim=True)).float().to(dev).contiguous()


def spread(ts):
    return {"median_ms": 1e3 * statistics.median(ts), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts), "calls": len(ts)}


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, out


def matrix_topk(model, e, ids, k):
    s = model.score_matrix(e, e)
    genuine = ids[:, None] == ids[None, :]
    eye = torch.eye(e.shape[0], dtype=torch.bool, device=e.device)
    imp = torch.topk(torch.where(genuine | eye, float("-inf"), s), k, dim=1)
    gen = torch.topk(torch.where(~genuine | eye, float("inf"), s), k, dim=1, largest=False)
    return imp, gen


def measure(routes):
    last, times = {}, {name: [] for name in routes}
    for name, fn in routes.items():
        for _ in range(WARMUP):
            last[name] = events(fn)[1]
    for _ in range(CALLS):
        for name, fn in routes.items():
            times[name].append(events(fn)[0])
    return last, times


def setup(n, dev):
    return unit_rows(n, n, dev), (torch.arange(n, device=dev) // 16).to(torch.int32)


def new_model(dev):
    torch.manual_seed(5)
    return SV.SiameseNetwork(DIM, max_images=4).to(dev).eval()


def parent_model(path, dev):
    """A model whose HIP context is created in the library at ``path`` (an older build of the same ABI: the symbols it has are
    given this build's signatures); this build's library stays the one every other context uses."""
    lib = C.CDLL(os.path.abspath(path))
    for table in (_lib._SIGNATURES, _lib._VERIFIER_SIGNATURES, _lib._VERIFIER_PAIRS_SIGNATURES):
        for name, (res, args) in table.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    assert lib.siggan_abi_version() == _lib.ABI_VERSION
    ours = _lib.load()
    _lib._lib = lib
    try:
        model = new_model(dev)
        assert model._context().lib is lib
    finally:
        _lib._lib = ours
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs_topk_throughput.json"))
    ap.add_argument("--parent_lib", default=None, help="libsiggan_hip.so built from the parent commit")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    dev = torch.device("cuda:0")
    model = new_model(dev)
    parent = parent_model(a.parent_lib, dev) if a.parent_lib else None
    out = {"device_name": torch.cuda.get_device_name(0), "dim": DIM, "warmup": WARMUP, "sizes": {}}
    for n in SIZES:
        e, ids = setup(n, dev)
        SV.PAIR_TOPK_CHUNK = n                                   # one call per list: the kernels, not the chunking
        routes = {f"topk_k{k}": (lambda k=k: model.pair_topk(e, ids, e, ids, k, same_set=True)) for k in (1, 4, 16)}
        routes["best"] = lambda: model.pairs(e, ids, e, ids, same_set=True, want_best=True)
        if parent is not None:
            routes["best_parent"] = lambda: parent.pairs(e, ids, e, ids, same_set=True, want_best=True)
        routes["matrix_topk"] = lambda: matrix_topk(model, e, ids, 16)
        last, times = measure(routes)
        res = {"n": n, "ordered_pairs": n * n}
        for name in routes:
            res[name] = spread(times[name])
        if n > 4096:
            SV.PAIR_TOPK_CHUNK = 4096
            _, t = measure({"topk_k16_chunked": lambda: model.pair_topk(e, ids, e, ids, 16, same_set=True)})
            res["topk_k16_chunked"] = spread(t["topk_k16_chunked"])
        if parent is not None:
            res["topk_k1_over_best_parent"] = res["topk_k1"]["median_ms"] / res["best_parent"]["median_ms"]
            res["best_over_best_parent"] = res["best"]["median_ms"] / res["best_parent"]["median_ms"]
            res["best_parent_equals_best"] = all(bool(torch.equal(last["best"][k_], last["best_parent"][k_])) for k_ in last["best"])
        res["topk_k1_over_best"] = res["topk_k1"]["median_ms"] / res["best"]["median_ms"]
        res["topk_k16_over_best"] = res["topk_k16"]["median_ms"] / res["best"]["median_ms"]
        res["matrix_topk_over_topk_k16"] = res["matrix_topk"]["median_ms"] / res["topk_k16"]["median_ms"]
        # what was timed is the right thing: k = 1 impostors are the row maxima; k = 16 impostors are torch.topk's values
        res["k1_impostor_equals_best"] = bool(torch.equal(last["topk_k1"]["impostor_index"][:, 0], last["best"]["best_impostor_index"]))
        res["k16_impostor_scores_equal_matrix_topk"] = bool(torch.equal(last["topk_k16"]["impostor_score"], last["matrix_topk"][0].values))
        out["sizes"][str(n)] = res
        del e, last
        torch.cuda.empty_cache()
    SV.PAIR_TOPK_CHUNK = 4096
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=2)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
