"""The ONE stdout line of bench.py (a 23.9 KB line left BENCH_r05.json unparsed): built from canned records, it must be
short, strict JSON, and carry the contract's fields plus `roofline` and `cpu_baseline`."""
import glob
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _fail(c):
    raise AssertionError("non-JSON constant %r in the bench line" % c)


CANNED = sorted(glob.glob(os.path.join(ROOT, "profiles", "r0[3-9]_final_bench.json")) + glob.glob(os.path.join(ROOT, "profiles", "r0[6-9]_final_bench_records.json")))
# (since round 6 `rNN_final_bench.json` IS the compact line bench.py printed; the full record it was cut from is `rNN_final_bench_records.json`)
FULL = [p for p in CANNED if "parity" in json.load(open(p)).get("config", {}) and "residual" in json.load(open(p))]


@pytest.mark.parametrize("path", CANNED, ids=[os.path.basename(p) for p in CANNED])
def test_line_from_a_committed_full_record_is_short_strict_json(path):
    m = _bench()
    out = json.load(open(path))
    if "roofline" not in out:          # (a committed compact line: nothing to rebuild it from)
        pytest.skip("compact record")
    txt = m.compact_line(out, "bench_records.json")
    assert "\n" not in txt and len(txt) < 6000, len(txt)
    assert len(txt) <= m.LINE_BYTES_MAX
    line = json.loads(txt, parse_constant=_fail)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["value"] == pytest.approx(out["value"], rel=1e-6)
    assert "workload" in line["config"] and "model" not in line["config"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in line["roofline"], k
    assert line["roofline"]["frac"] == pytest.approx(out["roofline"]["frac"], rel=1e-4)
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in line["cpu_baseline"], k


def test_non_finite_numbers_and_oversized_records_do_not_break_the_line():
    m = _bench()
    out = json.load(open(FULL[-1]))
    out["roofline"]["traffic"] = float("nan")
    out["residual"]["ipm_max_gap"] = float("inf")
    out["value_to_convergence"] = float("nan")
    out["config"]["parity"]["teacher_forced"] = {"case_%03d" % i: {"optimal_value_rel_diff_max": 1e-7} for i in range(400)}
    txt = m.compact_line(out, None)
    assert len(txt) <= m.LINE_BYTES_MAX
    line = json.loads(txt, parse_constant=_fail)
    assert line["roofline"]["traffic"] is None and "cpu_baseline" in line and "roofline" in line
    # the side file's cleaner maps non-finite numbers to null too
    import numpy as np
    rec = {"a": np.float64("nan"), "b": [np.int64(3), float("inf")], "c": np.arange(3)}
    import tempfile
    old = m.ROOT
    with tempfile.TemporaryDirectory() as d:
        m.ROOT = d
        try:
            assert m.write_records(rec) == "bench_records.json"
            assert json.load(open(os.path.join(d, "bench_records.json")), parse_constant=_fail) == {"a": None, "b": [3, None], "c": [0, 1, 2]}
        finally:
            m.ROOT = old


def test_line_of_a_plain_run_is_the_headline_only():
    """without `--full` the run measures the headline figure only: its line carries the contract's fields and no empty sections"""
    m = _bench()
    out = {"metric": "SCP iterations/sec (batched PTR, N=100 nodes)", "value": 28618.642123456, "unit": "SCP iterations/s", "n_gpus": 1,
           "steps": 20, "warmup": 5, "ms_per_step": 2132.84061234, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "f64", "data": "synthetic", "config": {"workload": "rocket_landing PTR", "global_batch": 4096, "solver_opts": {}},
           "scp_iterations_executed_per_step": 61039, "failed_instances": 0}
    line = json.loads(m.compact_line(out), parse_constant=_fail)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "failed_instances", "scp_iterations_executed_per_step"):
        assert k in line, k
    assert line["value"] == pytest.approx(out["value"], rel=1e-7) and line["ms_per_step"] == pytest.approx(out["ms_per_step"], rel=1e-7)
    for k in ("roofline", "roofline_discretize", "cpu_baseline", "residual", "parity", "records"):
        assert k not in line, k


def _fake_batch(pkg, B, N, nx, nu, iters, seed):
    rng = np.random.default_rng(seed)
    status = ["SCP_SOLVED" if rng.uniform() < 0.9 else "SCP_FAILED (x)" for _ in range(B)]
    sol = pkg.PTR.SCPSolutionBatch(status=status, algo="test", iterations=rng.integers(1, iters + 1, B), cost=rng.standard_normal(B),
                                   J=rng.standard_normal(B), td=np.linspace(0.0, 1.0, N), xd=rng.standard_normal((B, N, nx)),
                                   ud=rng.standard_normal((B, N, nu)), p=rng.standard_normal((B, 1)), J_aug=rng.standard_normal(B),
                                   feas=rng.uniform(size=B) < 0.5, defect=rng.standard_normal((B, N - 1, nx)))
    hist = pkg.PTR.SCPHistoryBatch(**{f: rng.standard_normal((iters, B)) for f in pkg.PTR.SCPHistoryBatch.__dataclass_fields__})
    hist.improv_rel[0] = np.nan                       # as the device reports it: no improvement before the first iteration
    sol.cost[[s != "SCP_SOLVED" for s in status]] = np.inf
    sol.J[0] = -np.inf
    return sol, hist


def test_dump_outputs_float64_within_budget_and_a_fixed_sample(pkg, tmp_path):
    """`--dump-outputs`: one float64 .npy of finite numbers per result array, the whole batch when it fits the budget, otherwise the
    same seeded sample of problems (with their Monte-Carlo indices) in every run"""
    m = _bench()
    sol, hist = _fake_batch(pkg, 64, 10, 7, 4, 15, 0)
    total = m.dump_outputs(str(tmp_path / "all"), sol, hist, offset=100)
    assert total == sum(f.stat().st_size for f in (tmp_path / "all").iterdir())
    xd = np.load(tmp_path / "all" / "xd.npy")
    assert xd.dtype == np.float64 and np.array_equal(xd, sol.xd)
    assert np.array_equal(np.load(tmp_path / "all" / "instance.npy"), 100 + np.arange(64))
    assert np.array_equal(np.load(tmp_path / "all" / "hist_J.npy"), hist.J.T)
    assert np.array_equal(np.load(tmp_path / "all" / "solved.npy"), [s == "SCP_SOLVED" for s in sol.status])
    for f in (tmp_path / "all").iterdir():
        a = np.load(f)
        assert a.dtype == np.float64 and np.isfinite(a).all(), f.name
    # non-finite entries are written as 0 beside a code array that restores them
    for nm, ref in (("hist_improv_rel", hist.improv_rel.T), ("cost", sol.cost), ("J", sol.J)):
        a, code = np.load(tmp_path / "all" / (nm + ".npy")), np.load(tmp_path / "all" / (nm + "_nonfinite.npy"))
        back = np.select([code == 1, code == 2, code == 3], [np.nan, np.inf, -np.inf], a)
        assert np.array_equal(back, ref, equal_nan=True), nm
    assert not (tmp_path / "all" / "xd_nonfinite.npy").exists()
    budget = total // 3
    small = [m.dump_outputs(str(tmp_path / d), sol, hist, budget=budget) for d in ("s1", "s2")]
    assert max(small) <= budget
    inst = np.load(tmp_path / "s1" / "instance.npy")
    assert 0 < inst.size < 64 and np.all(np.diff(inst) > 0)
    assert np.array_equal(inst, np.load(tmp_path / "s2" / "instance.npy"))
    assert np.array_equal(np.load(tmp_path / "s1" / "xd.npy"), sol.xd[inst.astype(int)])
