"""K3's factor records and the column view of the compact stage record (csrc/ipm2_kernel.hpp) on the GPU.

* A chain sweep loads exactly the part of a node's factor record it uses, PD = 3 nodes ahead, with the two boundary nodes
  peeled off: the horizons with 0 ... 5 interior nodes cover no interior record, a tail shorter than one pipeline round,
  exactly one round, and one round plus tails of 1 and 2.
* G' and the right-hand-side pass give a lane one column of Kl and find its slots through the transposed view of the
  pattern (StagePat::col_entry: all rows for G', the linear and cone rows for the right-hand sides), as many slots per
  column as the longest column has.  The column lists are MIRRORED here from the documented rows (PATTERNS of
  tests/test_sparse_stage_gpu.py), not read from the library.
* The refinement path calls G' once per step: one solve with the refinement forced on from the first iteration.

Every device solve is compared with the oracle's literal conic program at the tolerances of
tests/test_sparse_stage_gpu.py::test_item_indexing_edge_horizons_both_kernel_variants and must end OPTIMAL or
ALMOST_OPTIMAL; the two kernel variants must agree to 1e-7.
"""
import numpy as np
import pytest

from test_sparse_stage_gpu import PATTERNS, _mc_pp, _oracle_solutions, _stage_blocks

pytestmark = pytest.mark.gpu

NSUB, B = 6, 3
# slots per column the kernel is built for (StagePat::col_width(0): all rows, col_width(ns): rows behind the hinge rows): the longest column
# of the model's pattern -- rocket: r_z in the four glide-slope rows, xi in both thrust bounds, the pointing row and its
# cone; quadrotor: sigma in both bounds, the tilt row and its cone
BUILT_WIDTH = {"rocket_landing": dict(all=4, lin_cone=4, ns=2), "quadrotor": dict(all=4, lin_cone=4, ns=2)}


def _solve_and_compare(pkg, model, N, solver_opts, variants=(1, 2)):
    pp, refs, subs, scale = _oracle_solutions(model, N, NSUB, B)
    assert all(s["status"] in ("OPTIMAL", "ALMOST_OPTIMAL") for s in subs), [s["status"] for s in subs]
    xd = np.stack([r.xd for r in refs]); ud = np.stack([r.ud for r in refs]); p = np.stack([np.atleast_1d(r.p) for r in refs])
    got = {}
    for wpe in variants:
        traj = pkg.TrajectoryProblem(model)
        pars = pkg.PTR.Parameters(N=N, Nsub=NSUB, iter_max=15, wvc=1e3, wtr=0.1, eps_abs=0.0, eps_rel=0.0,
                                  solver_opts=dict(solver_opts, wpe=wpe))
        pbm = pkg.PTR.create(pars, traj, batch_capacity=B)
        g = pkg.PTR.solve_subproblem_(pbm, xd, ud, p, pp)
        pbm.close()
        assert np.isin(g["status"], (0, 1)).all(), (wpe, g["status"], g["info"])
        for b in range(B):
            sub = subs[b]
            dj = abs(g["J_aug"][b] - sub["J_aug"]) / max(1.0, abs(sub["J_aug"]))
            du = np.abs((g["u"][b] - sub["u"]) / scale.Su).max()
            print("%s N=%d wpe=%d b=%d: dJ_aug %.2e  du %.2e" % (model, N, wpe, b, dj, du))
            assert dj <= 5e-6, (wpe, b, g["J_aug"][b], sub["J_aug"])
            assert du <= 2e-3, (wpe, b, du)
        got[wpe] = g
    if len(variants) == 2:
        np.testing.assert_allclose(got[1]["x"], got[2]["x"], rtol=0, atol=1e-7)
        np.testing.assert_allclose(got[1]["u"], got[2]["u"], rtol=0, atol=1e-7)
        np.testing.assert_allclose(got[1]["J_aug"], got[2]["J_aug"], rtol=1e-8)


# N - 2 interior nodes: 0 (both records boundary records), 1, 2 (tails shorter than a round), 3 (one round), 4, 5 (a round and
# a tail).  The oracle solves the literal program of every instance listed, the rocket's N = 2 included (checked on the CPU).
@pytest.mark.parametrize("model,N", [(m, n) for m in ("rocket_landing", "quadrotor", "double_integrator") for n in range(2, 8)])
def test_sweep_pipeline_edges_both_kernel_variants(pkg, orc, model, N):
    _solve_and_compare(pkg, model, N, {})


def _columns(rows, lo):
    """column -> rows >= lo that hold it, ascending: the order of the transposed view"""
    nz = 1 + max(j for cols in rows for j in cols)
    return {j: [r for r, cols in enumerate(rows) if r >= lo and j in cols] for j in range(nz)}


@pytest.mark.parametrize("model", ["rocket_landing", "quadrotor"])
def test_column_view_width_and_longest_column_on_the_assembled_slab(pkg, model):
    rows, built = PATTERNS[model]["kl"], BUILT_WIDTH[model]
    views = {"all": _columns(rows, 0), "lin_cone": _columns(rows, built["ns"])}
    for name, cols in views.items():
        assert max(len(v) for v in cols.values()) <= built[name], (name, cols)
        # every declared slot is in exactly one column list
        assert sum(len(v) for v in cols.values()) == sum(len(c) for r, c in enumerate(rows) if name == "all" or r >= built["ns"])
    N = 6
    traj = pkg.TrajectoryProblem(model)
    pars = pkg.PTR.Parameters(N=N, Nsub=NSUB, iter_max=3, wvc=1e3, wtr=0.1, eps_abs=0.0, eps_rel=0.0)
    pbm = pkg.PTR.create(pars, traj, batch_capacity=B)
    pp = _mc_pp(traj.mdl, model, B)
    xs, us, ps = zip(*[traj.guess(N, pp[b]) for b in range(B)])
    g = pkg.PTR.solve_subproblem_(pbm, np.stack(xs), np.stack(us), np.stack(ps), pp)
    assert np.isin(g["status"], (0, 1)).all(), (g["status"], g["info"])
    assert pbm.info.ns == built["ns"]
    _, Kl, _ = _stage_blocks(pbm.info, N, pkg.PTR.debug_stage_problem(pbm, 0))
    pbm.close()
    # the longest column is full -- every slot non-zero -- at some interior node: the column view is not tested on short columns alone
    for name, cols in views.items():
        longest = [j for j, v in cols.items() if len(v) == built[name]]
        assert longest, (name, cols)
        full = [j for j in longest if any((Kl[k, cols[j], j] != 0.0).all() for k in range(1, N - 1))]
        assert full, (name, longest, [Kl[1, cols[j], j] for j in longest])


def test_refinement_path_forced_on(pkg, orc):
    # nref steps of iterative refinement in every Newton solve from the first iteration on (ref_gap above any gap, ref_tol 0: no
    # early exit): G' runs once per step
    _solve_and_compare(pkg, "rocket_landing", 9, dict(nref=2, ref_gap=1e300, ref_tol=0.0))
