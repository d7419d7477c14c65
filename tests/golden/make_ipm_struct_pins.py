"""Results of the numpy statement of K3's reduced Newton system (oracle/ipm_struct.py::solve with its default arguments) on six PTR
subproblems: the fixture tests/test_oracle_ipm.py::test_structured_solver_reproduces_its_pins compares every later version of the
solver with.  The problems are the first two subproblems of quadrotor N = 10, double_integrator N = 12 and rocket_landing N = 10,
built as test_reduced_structured_solver_equals_literal_program builds them (nominal parameters, the model's guess, second reference =
discretised solution of the literal program on the first).  Rocket landing has two second-order cones per node, hinge rows and a
free parameter together.

Record it with the solver the file is to stay equal to, BEFORE oracle/ipm_struct.py is edited:

    python tests/golden/make_ipm_struct_pins.py [OUT.npz]        # ~10 s; default tests/golden/ipm_struct_pins.npz

Statuses and iteration counts (15, 19, 14, 16, 76, 22) are compared exactly, arrays and scalars to the relative tolerance PIN_RTOL
(rel_diff below: largest difference over the array's largest magnitude).  On one machine two versions of the solver that take the
same arithmetic path write the same bytes.  PIN_RTOL covers the BLAS / LAPACK differences between machines and is measured, not
chosen: the unedited solver was recorded on the development machine and on the CPU of a GPU machine (numpy 2.2.6, scipy 1.15.3 on
both).  The largest rel_diff between the two recordings over all recorded floats was MEASURED_MACHINE_DIFF = 0.0 -- the two files
hold the same bytes -- so that PIN_RTOL = max(100 x 0.0, 1e-12) = 1e-12, its floor.  On both machines the solver reduced to the
shipped algorithm wrote the bytes of the unedited one.
"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

# (model, N); two successive subproblems each
CASES = [("quadrotor", 10), ("double_integrator", 12), ("rocket_landing", 10)]
FLOATS = ("pcost", "gap", "pres", "dres", "z", "p")
STATUS = ("OPTIMAL", "ALMOST_OPTIMAL", "ITERATION_LIMIT", "NUMERICAL_ERROR")

MEASURED_MACHINE_DIFF = 0.0
PIN_RTOL = max(100 * MEASURED_MACHINE_DIFF, 1e-12)


@functools.lru_cache(maxsize=None)
def solved(model, N):
    """The two successive subproblems of one model as (stage problem, solution of the literal program, scaling, result of
    ipm_struct.solve); computed once per process and shared by the tests that read it."""
    from oracle import ipm_struct, ptr_ref
    from oracle.models import MODELS
    mdl = MODELS[model]()
    pars = ptr_ref.PTRParameters(N, 8, 3, 1e3, 0.1, 0, 0, 1e-3)
    scale = ptr_ref.Scaling(*mdl.bbox())
    pp = mdl.nominal_pp()
    x, u, p = mdl.guess(N, pp)
    ref = ptr_ref.discretize(mdl, pars, scale, x, u, p)
    out = []
    for it in range(2):
        sub = ptr_ref.solve_subproblem(mdl, pars, scale, ref, pp)
        P = ipm_struct.build_stage_problem(mdl, pars, scale, ref, pp)
        out.append((P, sub, scale, ipm_struct.solve(P)))
        ref = ptr_ref.discretize(mdl, pars, scale, sub["x"], sub["u"], sub["p"])
    return tuple(out)


def pins(model, it, r):
    """What is recorded of one result."""
    key = "%s_%d_" % (model, it)
    out = {key + "status": np.int64(STATUS.index(r["status"])),
           key + "iters": np.int64(r["iters"]),                                # of the returned (best) iterate
           key + "iters_total": np.int64(r.get("iters_total", r["iters"]))}    # of the whole solve
    for f in FLOATS:
        out[key + f] = np.asarray(r[f], float)
    return out


def rel_diff(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    if a.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def main():
    from oracle import ipm_struct
    out = {}
    for model, N in CASES:
        for it, (P, sub, scale, r) in enumerate(solved(model, N)):
            out.update(pins(model, it, r))
            ua = ipm_struct.unpack(P, r["z"], r["p"])[1]
            print("%-18s %d  %-14s %3d iterations  cost - literal %.1e (rel)  input - literal %.1e (scaled)" % (
                model, it, r["status"], r["iters"],
                abs(r["pcost"] + P.cost_const - sub["J_aug"]) / max(1.0, abs(sub["J_aug"])),
                np.abs((ua - sub["u"]) / scale.Su).max()))
    np.savez_compressed(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ipm_struct_pins.npz"), **out)


if __name__ == "__main__":
    main()
