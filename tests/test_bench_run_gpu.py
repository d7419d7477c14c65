"""A plain `bench.py` run end to end on the MI355X (small batch): one strict-JSON line with the headline fields only, and
`--dump-outputs` writes the last timed step's results as finite float64 arrays that agree with the line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "256",
                        "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    line = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert "roofline" not in line and "cpu_baseline" not in line
    xd, solved, inst = (np.load(tmp_path / (nm + ".npy")) for nm in ("xd", "solved", "instance"))
    assert xd.dtype == np.float64 and xd.shape[0] == 256 and np.isfinite(xd[solved > 0]).all()
    assert np.array_equal(inst, np.arange(256))
    for f in tmp_path.iterdir():
        a = np.load(f)
        assert a.dtype == np.float64 and np.isfinite(a).all(), f.name
    assert int((solved == 0).sum()) == line["failed_instances"]
    # the line's iteration count is what the dumped history says was executed
    assert int(np.load(tmp_path / "hist_active.npy").sum()) == line["scp_iterations_executed_per_step"]
