"""Speed of two builds of the library on kernels whose ISA is not the parent's (context_free_parts_resources.md), with the
ops' own throughput scripts at their own shapes: neighbors and strokes.

    python profiles/context_free_parts_speed.py --parent PARENT.so --op neighbors            [--runs 5] [--out FILE.json]
    python profiles/context_free_parts_speed.py --parent PARENT.so --op strokes --size 128 --batch 1024

One run is one fresh process of neighbors_throughput.py / strokes_throughput.py with SIGGAN_LIB_PATH set; parent and new take
turns.  A figure is that run's median (the scripts' own warm-up and call counts).  The yardstick is the parent's own
[min, max] span over its runs of this session; `inside` says whether the new build's median over its runs lies in it.  The
result is appended under `measured` -> op (and shape) in the JSON, one entry per pass, and the derived fields (`what`, `how`,
`outside_the_parent_span`, `slow_side`, `sides_per_pass`) are rewritten from all of `measured`.  Passes measured in separate
sessions are joined with

    python profiles/context_free_parts_speed.py --merge PASS1.json PASS2.json ... [--out FILE.json]

Whatever a file holds under `notes_written_by_hand` is kept as it is: nothing here produces it."""
import argparse, json, os, statistics, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = {
    "neighbors": lambda a: (["neighbors_throughput.py"], lambda d: {"knn_ms": d["knn"]["median_ms"], "manifold_ms": d["manifold"]["median_ms"]}),
    "strokes": lambda a: (["strokes_throughput.py", "--size", str(a.size), "--batch", str(a.batch)],
                          lambda d: {f"{inp}/{route}_us": v[route]["median_us"] for inp, v in d[f"s{a.size}_b{a.batch}"]["inputs"].items()
                                     for route in ("stats", "all")}),
}


def write(path, measured, notes):
    """The file: the passes, what follows from them, and the hand-written notes untouched."""
    outside, sides = [], {}
    for name, passes in measured.items():
        for i, ps in enumerate(passes):
            for fig, r in ps["figures"].items():
                sides.setdefault(f"{name}: {fig}", []).append(r["side"])
                if not r["inside"]:
                    outside.append({"what": name, "figure": fig, "pass": i + 1, "parent_span": r["parent_span"], "new_median": r["new_median"],
                                    "side": r["side"]})
    out = {"what": "Time of two builds of the library, the parent commit's and another, with the ops' own throughput scripts at their own "
                   "shapes: the builds alternately in one session, each run a fresh process through SIGGAN_LIB_PATH.",
           "how": "profiles/context_free_parts_speed.py; a figure is one run's median (neighbors_throughput.py: 20 calls; strokes_throughput.py: "
                  "10 samples of 10 calls per input); the yardstick is the parent's own [min, max] span over its runs of that pass; a list under "
                  "a name in `measured` holds the passes in order",
           "outside_the_parent_span": outside, "slow_side": [o for o in outside if o["side"] == "above"],
           "sides_per_pass": {k: v for k, v in sides.items() if set(v) != {"inside"}}}
    if notes:
        out["notes_written_by_hand"] = notes
    out["measured"] = measured
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge", nargs="+", help="join the passes of these files, in order, instead of measuring")
    ap.add_argument("--parent")
    ap.add_argument("--new", default=os.path.join(ROOT, "signature-gan_amd", "libsiggan_hip.so"))
    ap.add_argument("--op", choices=sorted(OPS))
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "context_free_parts_speed.json"))
    a = ap.parse_args()
    if a.merge:
        measured, notes = {}, None
        for path in a.merge:
            d = json.load(open(path))
            notes = d.get("notes_written_by_hand", notes)
            for name, passes in d["measured"].items():
                measured.setdefault(name, []).extend(passes)
        write(a.out, measured, notes)
        return 0
    if not a.parent or not a.op:
        ap.error("--parent and --op are needed to measure")
    cmd, figures = OPS[a.op](a)
    runs = {"parent": [], "new": []}
    for i in range(a.runs):
        for build, path in (("parent", a.parent), ("new", a.new)):
            with tempfile.TemporaryDirectory() as tmp:
                out = os.path.join(tmp, "run.json")
                p = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", cmd[0]), *cmd[1:], "--out", out],
                                   env=dict(os.environ, SIGGAN_LIB_PATH=os.path.abspath(path)), capture_output=True, text=True, timeout=600)
                if p.returncode != 0:
                    print(build, "FAILED", p.returncode, p.stderr[-2000:], flush=True)
                    return 1
                runs[build].append(figures(json.load(open(out))))
            print(i, build, json.dumps(runs[build][-1]), flush=True)
    rows = {}
    for key in runs["parent"][0]:
        par, new = [r[key] for r in runs["parent"]], [r[key] for r in runs["new"]]
        span, med = [min(par), max(par)], statistics.median(new)
        rows[key] = {"parent": par, "new": new, "parent_median": statistics.median(par), "parent_span": span, "new_median": med,
                     "inside": span[0] <= med <= span[1], "side": "inside" if span[0] <= med <= span[1] else ("below" if med < span[0] else "above")}
    merged = json.load(open(a.out)) if os.path.exists(a.out) else {}
    name = a.op if a.op == "neighbors" else f"{a.op}/s{a.size}_b{a.batch}"
    merged.setdefault("measured", {}).setdefault(name, []).append({"runs_per_build": a.runs, "figures": rows})
    write(a.out, merged["measured"], merged.get("notes_written_by_hand"))
    print(json.dumps({k: (v["parent_span"], v["new_median"], v["side"]) for k, v in rows.items()}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
