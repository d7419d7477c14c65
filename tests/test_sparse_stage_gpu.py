"""K3's compact stage record (csrc/ipm2_kernel.hpp: StagePat) on the GPU.

The node-parallel passes of the structured IPM do not read the structural part of a stage record: the identity x-block
of E and the entries of Kl / Kp outside the pattern a model declares (models/*.hpp: kl_width, kl_col, has_kp).  Here

* the declared patterns are checked against the slab K2 assembles -- the pattern is MIRRORED below from the rows the
  model files document (s_eval / lin_rows / soc_rows), not read from the library;
* the horizons at which the new item indexing changes shape (one batch of 128 items, a clamped tail, counts just under
  a batch) are solved with both kernel variants and compared with the oracle's literal conic program;
* every solve must end OPTIMAL / ALMOST_OPTIMAL: the in-kernel pattern check ends a solve NUMERR.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# rows [hinge | linear | cone]: the columns of z = (x, u) a row can touch; None = no statement (dense default).
# rocket_landing (nx 7, nu 4): x = [r(3) v(3) ln m], u = [a(3) xi]
#   thrust bounds (ln m, xi) x 2 | glide slope (r_x, r_z) x 2, (r_y, r_z) x 2, ln m, pointing (a_z, xi) | ||v|| <= v_max:
#   constant, v_x, v_y, v_z | ||a|| <= xi: xi, a_x, a_y, a_z
# quadrotor (nx 6, nu 4): x = [r(3) v(3)], u = [a(3) sigma]
#   obstacles (r) x 2 | sigma >= u_min, sigma <= u_max, tilt (a_z, sigma) | ||a|| <= sigma: sigma, a_x, a_y, a_z
PATTERNS = {
    "rocket_landing": dict(kl=[{6, 10}, {6, 10}, {0, 2}, {0, 2}, {1, 2}, {1, 2}, {6}, {9, 10},
                               set(), {3}, {4}, {5}, {10}, {7}, {8}, {9}], kp=False),
    "quadrotor": dict(kl=[{0, 1, 2}, {0, 1, 2}, {9}, {9}, {8, 9}, {9}, {6}, {7}, {8}], kp=False),
    "double_integrator": dict(kl=None, kp=True),
}


def _stage_blocks(info, N, slab):
    """E, Kl, Kp of every node (all N of them) -- the slicing of tests/test_subproblem_gpu.py::_slab_views."""
    nx, nu, np_ = info.nx, info.nu, info.np
    nz, npa = nx + nu, max(np_, 1)
    ml = info.ns + info.nl + 4 * info.nsoc
    sizes = [("Qd", nz), ("q", nz), ("zref", nz), ("ttr", 1), ("cd", nx), ("om", nx), ("hw", max(info.ns, 1)), ("cl", ml),
             ("D", nx * nz), ("E", nx * nz), ("Fp", nx * npa), ("Kl", ml * nz), ("Kp", ml * npa)]
    SR = (sum(n for _, n in sizes) + 1) & ~1
    st = slab[:N * SR].reshape(N, SR)
    off, o = {}, 0
    for nm, n in sizes:
        off[nm] = (o, n)
        o += n
    cut = lambda nm, sh: st[:, off[nm][0]:off[nm][0] + off[nm][1]].reshape((N,) + sh)
    return cut("E", (nx, nz)), cut("Kl", (ml, nz)), cut("Kp", (ml, npa))


def _mc_pp(mdl, name, B, spread=0.1):
    out = []
    for b in range(B):
        rng = np.random.default_rng(100 + b)
        q = mdl.nominal_pp().copy()
        if name == "quadrotor":
            q[6:9] = q[6:9] * (1 + spread * rng.uniform(-1, 1, 3))      # r0 = 0: the goal position carries the spread
        else:
            q = q * (1 + spread * rng.uniform(-1, 1, q.size))
        out.append(q)
    return np.stack(out)


@pytest.mark.parametrize("model", ["rocket_landing", "quadrotor", "double_integrator", "oscillator"])
def test_declared_pattern_holds_on_the_assembled_slab(pkg, model):
    N, Nsub, B = 6, 6, 3
    traj = pkg.TrajectoryProblem(model)
    pars = pkg.PTR.Parameters(N=N, Nsub=Nsub, iter_max=3, wvc=1e3, wtr=0.1, eps_abs=0.0, eps_rel=0.0)
    pbm = pkg.PTR.create(pars, traj, batch_capacity=B)
    if model == "oscillator":
        # K3 does not serve this model (models/oscillator.hpp: structured = false -- node parameters): its subproblems go
        # through the generic conic solver and no stage-form slab exists whose pattern could be wrong
        assert not pbm.info.structured
        pbm.close()
        return
    assert pbm.info.structured
    pp = _mc_pp(traj.mdl, model, B)
    rng = np.random.default_rng(7)
    xs, us, ps = [], [], []
    for b in range(B):
        x, u, p = traj.guess(N, pp[b])
        xs.append(x + 0.02 * rng.standard_normal(x.shape) * (1 + np.abs(x))); us.append(u + 0.02 * rng.standard_normal(u.shape))
        ps.append(p)
    g = pkg.PTR.solve_subproblem_(pbm, np.stack(xs), np.stack(us), np.stack(ps), pp)
    assert np.isin(g["status"], (0, 1)).all(), (g["status"], g["info"])
    pat = PATTERNS[model]
    nx = pbm.info.nx
    for b in range(B):
        E, Kl, Kp = _stage_blocks(pbm.info, N, pkg.PTR.debug_stage_problem(pbm, b))
        for k in range(N):      # the last node included: the rocket's lin_rows switch to placeholder rows there
            want = np.eye(nx) if k < N - 1 else np.zeros((nx, nx))
            assert np.array_equal(E[k][:, :nx], want), (b, k)
            if pat["kl"] is not None:
                assert len(pat["kl"]) == Kl.shape[1]
                for r, cols in enumerate(pat["kl"]):
                    outside = [j for j in range(Kl.shape[2]) if j not in cols]
                    assert (Kl[k, r, outside] == 0.0).all(), (b, k, r, Kl[k, r])
            if not pat["kp"]:
                assert (Kp[k] == 0.0).all(), (b, k)
        if model == "rocket_landing":
            # the pattern is not vacuous: every declared slot is used at some interior node (the quadrotor's nominal obstacles
            # are cylinders -- their z column is declared because obstacles are data, and is zero here)
            for r, cols in enumerate(pat["kl"]):
                for j in cols:
                    assert (Kl[:N - 1, r, j] != 0.0).any(), (r, j)
    pbm.close()


@functools.lru_cache(maxsize=None)
def _oracle_solutions(model, N, Nsub, B):
    """The literal conic program of each of the B instances, solved once by the oracle (shared by the kernel variants)."""
    from oracle import ptr_ref
    from oracle.models import MODELS
    mdl = MODELS[model]()
    opars = ptr_ref.PTRParameters(N, Nsub, 15, 1e3, 0.1, 0, 0, 1e-3)
    scale = ptr_ref.Scaling(*mdl.bbox())
    pp = _mc_pp(mdl, model, B, spread=0.05)
    pp[0] = mdl.nominal_pp()
    refs, subs = [], []
    for b in range(B):
        x, u, p = mdl.guess(N, pp[b])
        ref = ptr_ref.discretize(mdl, opars, scale, x, u, p)
        refs.append(ref)
        subs.append(ptr_ref.solve_subproblem(mdl, opars, scale, ref, pp[b]))
    return pp, refs, subs, scale


# rocket (nx 7, nz 11, ml 16): N = 3 first / one middle / last node, every item count far below one 128-item batch;
# N = 9: N ml = 144, one full batch and a clamped tail; N = 17: N nz = 187 and N nx = 119, just under a batch.
# quadrotor: the second declared pattern (three slots per row).
@pytest.mark.parametrize("model,N", [("rocket_landing", 3), ("rocket_landing", 9), ("rocket_landing", 17),
                                     ("quadrotor", 3), ("quadrotor", 9)])
def test_item_indexing_edge_horizons_both_kernel_variants(pkg, orc, model, N):
    Nsub, B = 6, 3
    pp, refs, subs, scale = _oracle_solutions(model, N, Nsub, B)
    xd = np.stack([r.xd for r in refs]); ud = np.stack([r.ud for r in refs]); p = np.stack([np.atleast_1d(r.p) for r in refs])
    got = {}
    for wpe in (1, 2):
        traj = pkg.TrajectoryProblem(model)
        pars = pkg.PTR.Parameters(N=N, Nsub=Nsub, iter_max=15, wvc=1e3, wtr=0.1, eps_abs=0.0, eps_rel=0.0, solver_opts=dict(wpe=wpe))
        pbm = pkg.PTR.create(pars, traj, batch_capacity=B)
        g = pkg.PTR.solve_subproblem_(pbm, xd, ud, p, pp)
        pbm.close()
        assert np.isin(g["status"], (0, 1)).all(), (wpe, g["status"], g["info"])
        for b in range(B):      # the tolerances of tests/test_subproblem_gpu.py::test_smallest_horizons
            sub = subs[b]
            assert abs(g["J_aug"][b] - sub["J_aug"]) <= 5e-6 * max(1.0, abs(sub["J_aug"])), (wpe, b, g["J_aug"][b], sub["J_aug"])
            du = np.abs((g["u"][b] - sub["u"]) / scale.Su).max()
            assert du <= 2e-3, (wpe, b, du)
        got[wpe] = g
    # the two register budgets run the same algorithm (tests/test_ptr_gpu.py::test_large_batch_kernel_variant_matches_small_batch)
    np.testing.assert_allclose(got[1]["x"], got[2]["x"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(got[1]["u"], got[2]["u"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(got[1]["J_aug"], got[2]["J_aug"], rtol=1e-8)
