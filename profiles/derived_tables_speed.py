"""Step time of two builds of the library at every timed shape (tests/common.py TIMED), run alternately in one session.

    python profiles/derived_tables_speed.py --parent PARENT.so [--new NEW.so] [--reps 5] [--only f16,128,128,64] [--out FILE.json]

Each run is a fresh `bench.py --gpus 1 --full --no-cpu --no-roofline --blocks 5 --steps 100 --warmup 20` process with the
build named by SIGGAN_LIB_PATH; its figure is the median ms/step over the five blocks.  Per shape: parent, new, parent, new,
... --reps times each.  The yardstick is the parent's own run-to-run span [min, max] of that session; `inside` says whether
the median of the new build's runs lies in it."""
import argparse, json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--new", default=os.path.join(ROOT, "signature-gan_amd", "libsiggan_hip.so"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", help="one shape: dtype,size,latent,batch")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "derived_tables_speed.json"))
    a = ap.parse_args()
    from common import TIMED
    builds = {"parent": os.path.abspath(a.parent), "new": os.path.abspath(a.new)}
    shapes = []
    only = a.only and tuple(int(v) if v.isdigit() else v for v in a.only.split(","))
    for dtype, size, latent, batch in ([only] if only else TIMED):
        runs = {"parent": [], "new": []}
        for _ in range(a.reps):
            for name, path in builds.items():
                cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--full", "--no-cpu", "--no-roofline", "--blocks", "5",
                       "--steps", "100", "--warmup", "20", "--dtype", dtype, "--size", str(size), "--latent", str(latent), "--batch", str(batch)]
                p = subprocess.run(cmd, env=dict(os.environ, SIGGAN_LIB_PATH=path), capture_output=True, text=True, timeout=300)
                if p.returncode != 0:
                    print(name, dtype, size, batch, "FAILED", p.returncode, p.stderr[-1500:], flush=True)
                    return 1
                runs[name].append(json.loads(p.stdout.strip().splitlines()[-1])["timing"]["ms_per_step_median"])
        lo, hi = min(runs["parent"]), max(runs["parent"])
        row = {"dtype": dtype, "size": size, "latent": latent, "batch": batch, "runs_ms_per_step": runs,
               "parent_median": statistics.median(runs["parent"]), "parent_span": [lo, hi],
               "new_median": statistics.median(runs["new"]), "inside": lo <= statistics.median(runs["new"]) <= hi,
               "new_runs_outside_span": [v for v in runs["new"] if not lo <= v <= hi]}
        shapes.append(row)
        print(json.dumps(row), flush=True)
        with open(a.out, "w") as f:
            json.dump({"what": __doc__.split("\n")[0], "reps": a.reps, "shapes": shapes}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
