"""K3 without its declared zeros and mirrored halves (csrc/ipm2_kernel.hpp) on the GPU: the reductions over the parameter column
skip the rows whose coefficient is a declared zero and no C0 exists (models without Kp), H0 is the packed lower triangle, a
cone's scalings are the packed lower triangles of W and W^-1.  tests/test_sparse_stage_gpu.py and tests/test_k3_records_gpu.py
cover the pattern check, the short horizons, both kernel variants and the three models on cold solves; here are the two
paths they leave out:

* the refinement forced on from the first iteration on the quadrotor (one cone, np = 1) and the double integrator (no cone,
  np = 0, dense pattern): the only path that reads the W block of a cone's scalings outside the combined-direction pass and
  that calls G' more than once per Newton solve (the rocket at N = 9: tests/test_k3_records_gpu.py);
* three PTR iterations on ONE handle: the second and the third launch start warm from snapshots in the workspace the first
  launch left behind.

Every device solve is compared with the oracle's literal conic program about the same reference at the tolerances of those
files -- 5e-6 relative on J_aug, 2e-3 on the scaled inputs -- and must end OPTIMAL or ALMOST_OPTIMAL; the two kernel variants
must agree to 1e-7.  The oracle solves every instance listed (checked on the CPU).
"""
import functools

import numpy as np
import pytest

import test_k3_records_gpu
from test_k3_records_gpu import _solve_and_compare      # (itself built on test_sparse_stage_gpu's _oracle_solutions, at that file's NSUB and B)
from test_sparse_stage_gpu import _mc_pp

pytestmark = pytest.mark.gpu

NSUB, B = 6, 3
assert (test_k3_records_gpu.NSUB, test_k3_records_gpu.B) == (NSUB, B)   # the refinement test runs at the helper's sizes: the same


@pytest.mark.parametrize("model", ["quadrotor", "double_integrator"])
def test_refinement_forced_on_one_cone_and_no_cone(pkg, orc, model):
    # nref steps of iterative refinement in every Newton solve from the first iteration on (ref_gap above any gap, ref_tol 0: no early exit)
    _solve_and_compare(pkg, model, 4, dict(nref=2, ref_gap=1e300, ref_tol=0.0))


@functools.lru_cache(maxsize=None)
def _oracle_sub(model, N, x, u, p, pp):
    """The literal program about one reference (given as bytes: hashable; the first one is shared by the kernel variants), solved by
    the oracle."""
    from oracle import ptr_ref
    from oracle.models import MODELS
    mdl = MODELS[model]()
    opars = ptr_ref.PTRParameters(N, NSUB, 15, 1e3, 0.1, 0, 0, 1e-3)
    scale = ptr_ref.Scaling(*mdl.bbox())
    x = np.frombuffer(x).reshape(N, mdl.nx).copy(); u = np.frombuffer(u).reshape(N, mdl.nu).copy()
    p = np.frombuffer(p).copy(); pp = np.frombuffer(pp).copy()
    ref = ptr_ref.discretize(mdl, opars, scale, x, u, p)
    return ptr_ref.solve_subproblem(mdl, opars, scale, ref, pp), scale


def _ptr_run(pkg, model, N, iters, wpe, pp):
    traj = pkg.TrajectoryProblem(model)
    pars = pkg.PTR.Parameters(N=N, Nsub=NSUB, iter_max=iters, wvc=1e3, wtr=0.1, eps_abs=0.0, eps_rel=0.0, solver_opts=dict(wpe=wpe))
    pbm = pkg.PTR.create(pars, traj, batch_capacity=B)
    sol, h = pkg.PTR.solve(pbm, pp)
    pbm.close()
    return sol, h


@pytest.mark.parametrize("model", ["rocket_landing", "quadrotor"])
def test_three_ptr_iterations_on_one_handle(pkg, orc, model):
    N = 5
    traj = pkg.TrajectoryProblem(model)
    pp = _mc_pp(traj.mdl, model, B, spread=0.05)
    pp[0] = traj.mdl.nominal_pp()
    final = {}
    for wpe in (1, 2):
        # the run under test: three iterations on one handle.  Runs of one and two iterations on handles of their own give the
        # references of its second and third subproblem (the loop is deterministic: their histories are its first rows, bit for bit)
        runs = {it: _ptr_run(pkg, model, N, it, wpe, pp) for it in (1, 2, 3)}
        sol3, h3 = runs[3]
        assert (sol3.iterations == 3).all(), sol3.iterations
        assert np.isin(h3.solver_status[:3], (0, 1)).all(), (wpe, h3.solver_status[:3])
        for it in (1, 2):
            assert np.array_equal(runs[it][1].J_aug[:it], h3.J_aug[:it]), (wpe, it)
        for b in range(B):
            x, u, p = traj.guess(N, pp[b])
            for it in (1, 2, 3):
                sub, scale = _oracle_sub(model, N, np.ascontiguousarray(x, dtype=np.float64).tobytes(),
                                         np.ascontiguousarray(u, dtype=np.float64).tobytes(),
                                         np.ascontiguousarray(np.atleast_1d(p), dtype=np.float64).tobytes(), pp[b].tobytes())
                assert sub["status"] in ("OPTIMAL", "ALMOST_OPTIMAL"), (wpe, b, it, sub["status"])
                sol = runs[it][0]
                dj = abs(h3.J_aug[it - 1, b] - sub["J_aug"]) / max(1.0, abs(sub["J_aug"]))
                du = np.abs((sol.ud[b] - sub["u"]) / scale.Su).max()
                print("%s wpe=%d b=%d iteration %d: dJ_aug %.2e  du %.2e  IPM iterations %d" % (model, wpe, b, it, dj, du, h3.solver_iters[it - 1, b]))
                assert dj <= 5e-6, (wpe, b, it, h3.J_aug[it - 1, b], sub["J_aug"])
                assert du <= 2e-3, (wpe, b, it, du)
                x, u, p = sol.xd[b], sol.ud[b], sol.p[b]      # the next subproblem's reference
        final[wpe] = sol3
    np.testing.assert_allclose(final[1].xd, final[2].xd, rtol=0, atol=1e-7)
    np.testing.assert_allclose(final[1].ud, final[2].ud, rtol=0, atol=1e-7)
    np.testing.assert_allclose(final[1].J_aug, final[2].J_aug, rtol=1e-8)
