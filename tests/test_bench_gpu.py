"""bench.py's plain run on the MI355X: exactly --steps timed steps, the headline keys, no --full legs, and the outputs of
the last timed step written by --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from common import ROOT

pytestmark = pytest.mark.gpu


def test_plain_bench_times_its_steps_and_dumps_the_last_step(tmp_path):
    out_dir = tmp_path / "outputs"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                          "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert run.returncode == 0, run.stderr[-4000:]
    line = json.loads(run.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["unit"] == "images/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 5 and line["timing"]["blocks"] == 1 and line["timing"]["steps_per_block"] == 5
    assert line["value"] == pytest.approx(64 * 1e3 / line["ms_per_step"], rel=1e-3)
    assert line["roofline"] is None and line["secondary"] is None and line["cpu_baseline"] is None
    got = {p.stem: np.load(p) for p in out_dir.glob("*.npy")}
    assert set(got) == {"metrics", "g_params", "d_params", "g_bn_running_mean", "g_bn_running_var"}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert sum(os.path.getsize(p) for p in out_dir.glob("*.npy")) < 64e6
    assert got["metrics"].shape == (16,)
    assert got["metrics"][0] == pytest.approx(line["final_metrics"]["d_loss"], abs=1e-4)
    assert got["metrics"][8] == pytest.approx(line["final_metrics"]["g_loss"], abs=1e-4)
