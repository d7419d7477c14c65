"""oracle/cpu_ptr.cpp (the C++/OpenMP restatement of the structured PTR iteration: bench.py's CPU baseline and the sibling the
device results are compared with at the headline size, tests/test_config_size_gpu.py) pinned against the LITERAL loop of
oracle/ptr_ref.py -- every subproblem a literal conic program solved by oracle/ipm.py -- on the first instances of the headline
Monte-Carlo batch (rocket landing, N = 100, Nsub = 15, 15 iterations; tests/golden/ptr_outcomes_rocket_landing_N100.npz), and
pinned TIGHTLY against its own recorded results on three small batches (tests/golden/cpu_twin_pins.npz), so that an edit of the twin
which changes what it computes shows on a CPU in seconds."""
import os

import numpy as np
import pytest

import bench
from oracle import cpu_ptr
from oracle.models import MODELS
from tests.golden.make_cpu_twin_pins import CASES, run_case


def test_structured_port_equals_the_literal_loop_on_headline_instances():
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "ptr_outcomes_rocket_landing_N100.npz"))
    nb = 64
    mdl = MODELS["rocket_landing"]()
    r = cpu_ptr.solve_batch("rocket_landing", int(g["N"]), int(g["Nsub"]), int(g["iter_max"]), bench.mc_pp(mdl, nb, 0), threads=0,
                            want_hist=True)

    class Sol:
        pass
    sol = Sol()
    sol.status = ["SCP_SOLVED" if r["hist"][b, :, 5].max() <= 1 else "SCP_FAILED" for b in range(nb)]
    sol.feas = r["stats"][:, 2] > 0
    sol.J_aug = r["hist"][:, -1, 0]
    sol.p = r["p"]
    o = bench.oracle_outcomes_ptr("rocket_landing", int(g["N"]), int(g["Nsub"]), int(g["iter_max"]), 0, sol)     # what bench.py reports
    assert o["instances"] == nb and o["same_status"] == 1.0 and o["same_feasibility_flag"] == 1.0
    assert o["converged_in_both"] >= 55
    # measured on the first 256 instances: median 5.7e-9, maximum 9.4e-7 (costs), 5e-4 s (final time)
    assert o["J_aug_rel_diff_max"] <= 2e-6 and o["tf_abs_diff_max_s"] <= 2e-3
    # the oracle's batch statistics themselves (all 256): every subproblem OPTIMAL, 93.75 % dynamically feasible after 15 iterations
    assert g["ipm_all_optimal"].all() and (g["status"] == 0).all() and abs(g["feas"].mean() - 0.9375) < 1e-12


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_twin_results_are_pinned(case):
    """The twin computes what it computed when tests/golden/cpu_twin_pins.npz was recorded (tests/golden/make_cpu_twin_pins.py: the
    build before the twin was reduced to the shipped algorithm).  Iteration counts, statuses and the batch statistics are integers and
    must be equal; the floats agree to 1e-9 of the array's largest magnitude -- three decades below the 2e-6 of the test above, far above
    last-bit libm differences between hosts.  The twin is single-threaded per problem: the thread count must not change a bit."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "cpu_twin_pins.npz"))
    model = case[0]
    r = run_case(*case, threads=1)
    want = {k: g["%s_%s" % (model, k)] for k in r}
    assert np.array_equal(r["hist"][..., 4], want["hist"][..., 4])      # IPM iterations per solve, all attempts
    assert np.array_equal(r["hist"][..., 5], want["hist"][..., 5])      # status per solve
    assert np.array_equal(r["stats"], want["stats"])                    # (IPM iterations, worst status, feasible) per problem
    for k, a, b in [(k, r[k], want[k]) for k in ("xd", "ud", "p")] + [("hist[%d]" % c, r["hist"][..., c], want["hist"][..., c]) for c in range(4)]:
        assert a.shape == b.shape
        if b.size:
            err = np.abs(a - b).max() / np.abs(b).max()
            print("%s %s: %.3e" % (model, k, err))
            assert err <= 1e-9, k
    r4 = run_case(*case, threads=4)
    for k in r:
        assert np.array_equal(r[k], r4[k]), k
