"""Results of the CPU twin of K3 (oracle/cpu_ptr.cpp through oracle/cpu_ptr.py) on three small batches, one per model: the fixture
tests/test_cpu_port_cpu.py::test_twin_results_are_pinned compares every later build of the twin with.  Inputs are the first
instances of bench.py's Monte-Carlo batch (bench.mc_pp(model, B, 0)) at the default weights; each case runs on ONE thread with
the per-iteration history.  The rocket case needs a full run: its solves start cold, then from level 0 (PTR iterations 1-4), 1 (5-6), 2 (6)
and from the very fine level 3 only from iteration 6 or 7 on, so that only the second half of the run has started from all four levels.

Record it with the build the twin is to stay equal to, BEFORE oracle/cpu_ptr.cpp is edited:

    make -C oracle && python tests/golden/make_cpu_twin_pins.py        # ~5 s
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

# (model, N, Nsub, PTR iterations, batch)
CASES = [("rocket_landing", 100, 15, 15, 8), ("quadrotor", 30, 10, 10, 4), ("double_integrator", 20, 10, 6, 4)]


def run_case(model, N, Nsub, iters, B, threads=1):
    import bench
    from oracle import cpu_ptr
    from oracle.models import MODELS
    r = cpu_ptr.solve_batch(model, N, Nsub, iters, bench.mc_pp(MODELS[model](), B, 0), threads=threads, want_hist=True)
    return dict(xd=r["xd"], ud=r["ud"], p=r["p"], hist=r["hist"], stats=r["stats"][:, :3].copy())


def main():
    out = {}
    for model, N, Nsub, iters, B in CASES:
        r = run_case(model, N, Nsub, iters, B)
        for k, v in r.items():
            out["%s_%s" % (model, k)] = v
        h = r["hist"]
        print("%-18s IPM iterations per solve %5.1f (first) %5.1f (later), worst status %d, feasible %d / %d" % (
            model, h[:, 0, 4].mean(), h[:, 1:, 4].mean(), int(h[:, :, 5].max()), int(r["stats"][:, 2].sum()), B))
    np.savez_compressed(os.path.join(HERE, "cpu_twin_pins.npz"), **out)


if __name__ == "__main__":
    main()
