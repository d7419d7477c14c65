"""Oscillator with actuator deadband on the device: discretize! and the device guess against the numpy restatement
(oracle/models.py, oracle/discretize_ref.py), teacher-forced subproblems and the warm-started PTR homotopy against the oracle's fixture
(tests/golden/oscillator_outcomes_n12.npz), the device-resident continuation against a host restart, model constants changed
after create, and the refusals."""
import ctypes
import os

import numpy as np
import pytest

from oracle import discretize_ref, models

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oscillator_outcomes_n12.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def make(pkg, N, Nsub, cap, kappa1=1.0, method=None, iter_max=10):
    """PTR problem with the parameters of oscillator/tests.jl:24-57"""
    traj = pkg.TrajectoryProblem("oscillator", kappa1=kappa1)
    pars = pkg.PTR.Parameters(N=N, Nsub=Nsub, iter_max=iter_max, disc_method=pkg.FOH if method is None else method, wvc=1e2, wtr=1e-3,
                              eps_abs=-np.inf, eps_rel=1e-3 / 100, feas_tol=5e-3)
    return pkg.PTR.create(pars, traj, batch_capacity=cap)


@pytest.mark.parametrize("method,N,Nsub,B", [("foh", 6, 5, 3), ("impulse", 6, 5, 3), ("foh", 30, 10, 1)])
def test_discretize_against_the_restatement(pkg, method, N, Nsub, B):
    pbm = make(pkg, N, Nsub, B, method=pkg.IMPULSE if method == "impulse" else pkg.FOH)
    mdl = models.Oscillator(N)
    rng = np.random.default_rng(5)
    xs, us, ps = [], [], []
    for b in range(B):
        x, u, p = mdl.guess(N, models.INSTANCES[b])
        xs.append(x + 0.1 * rng.standard_normal(x.shape)); us.append(0.3 * rng.uniform(-1, 1, u.shape)); ps.append(p)
    ref = pkg.SubproblemSolutionBatch(np.stack(xs), np.stack(us), np.stack(ps), pbm)
    pkg.discretize_(ref, pbm)
    assert ref.dyn.F.shape[2] == 0
    for b in range(B):
        o = discretize_ref.discretize_arrays(mdl, N, Nsub, ref.xd[b], ref.ud[b], ref.p[b], pbm.scale.iSx, pbm.pars.feas_tol, method)
        for nm, got in (("A", ref.dyn.A[b]), ("Bm", ref.dyn.B[0][b]), ("Bp", ref.dyn.B[1][b]), ("E", ref.dyn.E[b])):
            err = np.abs(np.swapaxes(got, 1, 2) - o[nm]).max() / max(1.0, np.abs(o[nm]).max())
            assert err < 1e-10, (nm, b, err)
        for nm, got in (("r", ref.dyn.r[b]), ("defect", ref.defect[b])):
            err = np.abs(got - o[nm]).max() / max(1.0, np.abs(o[nm]).max())
            assert err < 1e-10, (nm, b, err)
        assert bool(ref.feas[b]) == o["feas"]
    pbm.close()


def test_device_guess_against_the_restatement(pkg):
    N = 12
    pbm = make(pkg, N, 10, len(models.INSTANCES))
    xd, ud, p = pkg.device_guess(pbm, models.INSTANCES)
    assert pkg.device_guess_failures(pbm) == 0
    mdl = models.Oscillator(N)
    for b, pp in enumerate(models.INSTANCES):
        x, u, pn = mdl.guess(N, pp)
        assert np.abs(xd[b] - x).max() < 1e-10 and np.abs(ud[b] - u).max() == 0.0 and np.abs(p[b] - pn).max() < 1e-10
    pbm.close()


@pytest.mark.parametrize("stage", [0, 1, 2])
def test_teacher_forced_subproblems(pkg, gold, stage):
    """the oracle's reference trajectories of the first subproblem of every stage (5 instances x 3 kappa1) through
    solve_subproblem!: same optimal value"""
    N, Nsub = int(gold["N"]), int(gold["Nsub"])
    pbm = make(pkg, N, Nsub, 5, kappa1=float(gold["kappa"][stage]))
    g = pkg.PTR.solve_subproblem_(pbm, gold["ref_x"][:, stage], gold["ref_u"][:, stage], gold["ref_p"][:, stage], pp=gold["pp"])
    want = gold["J_aug_first"][:, stage]
    rel = np.abs(g["pcost"] - want) / np.abs(want)
    print("teacher-forced stage %d: status %s, relative error of J_aug %s" % (stage, g["status"].tolist(), rel.tolist()))
    assert (g["status"] <= 1).all()
    assert rel.max() <= 1e-6
    pbm.close()


def test_homotopy_loop_on_a_batch_across_a_wavefront(pkg, gold):
    B = 67
    idx = np.arange(B) % 5
    pbm = make(pkg, int(gold["N"]), int(gold["Nsub"]), B)
    sol, hist, summ = pkg.PTR.solve_homotopy(pbm, "kappa1", gold["kappa"], pp=gold["pp"][idx])
    print("homotopy B = 67: iterations per stage (first five instances) %s, oracle %s" % (summ["iterations"][:, :5].T.tolist(), gold["iterations"].tolist()))
    assert (summ["status"] == 0).all()                      # the reference's own assertion (oscillator/tests.jl:81), at every stage
    assert all(st == "SCP_SOLVED" for st in sol.status)
    assert sol.feas.all()
    mdl = models.Oscillator(int(gold["N"]), float(gold["kappa"][-1]))
    smax = max(mdl.s(0.0, k + 1, sol.xd[b, k], sol.ud[b, k], sol.p[b]).max() for b in range(B) for k in range(mdl.N))
    print("largest deadband violation max(s, 0) at the last kappa1: %.3e" % max(smax, 0.0))
    assert max(smax, 0.0) <= 1e-6
    want = gold["J"][idx, -1]
    rel = np.abs(sol.J - want) / np.abs(want)
    print("final J, relative to the oracle's: max %.3e" % rel.max())
    assert rel.max() <= 1e-4
    np.testing.assert_array_equal(summ["J"][-1], sol.J)
    for i in range(5):                                      # copies of one instance agree
        for s in range(3):
            assert np.unique(summ["status"][s, idx == i]).size == 1 and np.unique(summ["iterations"][s, idx == i]).size == 1
    assert pbm.traj.mdl.kappa1 == float(gold["kappa"][-1]) and pbm.traj.mdl.par()[5] == float(gold["kappa"][-1])
    pbm.close()


def test_continue_equals_a_host_restart(pkg, gold):
    """stage 2 by scp_ptr_generic_continue == stage 2 by get_host + a fresh init_host with those arrays as warm start on a
    second handle created at the same kappa1: bit for bit"""
    N, Nsub, B = int(gold["N"]), int(gold["Nsub"]), 7
    pp = gold["pp"][np.arange(B) % 5]
    k0, k1 = float(gold["kappa"][0]), float(gold["kappa"][1])
    pbm = make(pkg, N, Nsub, B)
    sols, hists, summ = pkg.PTR.solve_homotopy(pbm, "kappa1", [k0, k1], pp=pp, keep=True)
    pb2 = make(pkg, N, Nsub, B, kappa1=k1)
    s2, h2 = pkg.PTR.solve(pb2, pp, warm=(sols[0].xd, sols[0].ud, sols[0].p))
    c = sols[1]
    for nm in ("xd", "ud", "p", "iterations", "cost", "J", "J_aug", "feas", "defect"):
        np.testing.assert_array_equal(getattr(c, nm), getattr(s2, nm), err_msg=nm)
    assert c.status == s2.status
    for nm in ("J", "J_aug", "deviation", "solver_iters", "solver_status"):
        np.testing.assert_array_equal(getattr(hists[1], nm), getattr(h2, nm), err_msg=nm)
    np.testing.assert_array_equal(summ["iterations"][1], s2.iterations)
    # the continued run is a run: iterate / get_host afterwards as after init (nothing is active any more)
    na = ctypes.c_int(-1)
    sub = pkg.PTR._generic_sub(pbm)
    assert pkg._lib.lib().scp_ptr_generic_iterate(sub._h, ctypes.byref(na)) == 0
    pbm.close(); pb2.close()


def test_continue_with_new_parameters(pkg, gold):
    """a non-NULL `pars`: the continued stage runs under a LARGER iter_max (its history is reallocated) with eps_rel = 0, so that it runs past the old capacity, and
    equals a host restart on a handle created with those parameters, bit for bit"""
    N, Nsub, B = int(gold["N"]), int(gold["Nsub"]), 5
    pp, k0, k1 = gold["pp"], float(gold["kappa"][0]), float(gold["kappa"][1])
    L = pkg._lib.lib()
    pbm = make(pkg, N, Nsub, B, kappa1=k0, iter_max=6)
    s1, _ = pkg.PTR.solve(pbm, pp)
    sub = pkg.PTR._generic_sub(pbm)
    pbm.set_model_par(kappa1=k1)
    pbm.pars.iter_max, pbm.pars.eps_rel = 13, 0.0
    cp = pkg.PTR._generic_params(pbm, sub)
    assert L.scp_ptr_generic_continue(sub._h, ctypes.byref(cp)) == 0
    r = pkg.generic.iterate_and_read(pbm, sub, L.scp_ptr_generic_iterate, L.scp_ptr_generic_get_host, B, (B, 4), pkg._lib.HIST_WIDTH)
    c, hc = pkg.PTR._result(pbm, "PTR", r)
    pb2 = make(pkg, N, Nsub, B, kappa1=k1, iter_max=13)
    pb2.pars.eps_rel = 0.0
    s2, h2 = pkg.PTR.solve(pb2, pp, warm=(s1.xd, s1.ud, s1.p))
    print("continue with new parameters: iterations %s (first stage %s)" % (c.iterations.tolist(), s1.iterations.tolist()))
    assert c.iterations.max() > 6                                    # rows of the history beyond the first stage's capacity were written
    for nm in ("xd", "ud", "p", "iterations", "cost", "J", "feas", "defect"):
        np.testing.assert_array_equal(getattr(c, nm), getattr(s2, nm), err_msg=nm)
    assert c.status == s2.status and hc.J_aug.shape == (13, B)
    np.testing.assert_array_equal(hc.J_aug, h2.J_aug)
    cp.iter_max = 0                                                  # refused like init refuses it; the run is untouched
    assert L.scp_ptr_generic_continue(sub._h, ctypes.byref(cp)) == 1
    pbm.close(); pb2.close()


def test_continue_before_any_iteration(pkg, gold):
    """continue straight after init: no solution exists yet, the reference (the guess) stays, and the run equals a plain solve"""
    N, Nsub, B = int(gold["N"]), int(gold["Nsub"]), 5
    pp, L = gold["pp"], pkg._lib.lib()
    pbm = make(pkg, N, Nsub, B, kappa1=float(gold["kappa"][0]))
    sub = pkg.PTR._generic_sub(pbm)
    cp = pkg.PTR._generic_params(pbm, sub)
    xd, ud, p = pkg.generic.stack_guesses(pbm, pp)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.scp_ptr_generic_init_host(sub._h, B, ctypes.byref(cp), vp(xd), vp(ud), vp(p), vp(pp)) == 0
    assert L.scp_ptr_generic_continue(sub._h, None) == 0
    rc, g = pkg.generic.read_result(pbm, B, L.scp_ptr_generic_get_host, sub._h, (B, 4), pkg._lib.HIST_WIDTH)
    assert rc == 0
    np.testing.assert_array_equal(g.xd, xd); np.testing.assert_array_equal(g.p, p)      # get_host before the first iteration: the reference
    r = pkg.generic.iterate_and_read(pbm, sub, L.scp_ptr_generic_iterate, L.scp_ptr_generic_get_host, B, (B, 4), pkg._lib.HIST_WIDTH)
    pb2 = make(pkg, N, Nsub, B, kappa1=float(gold["kappa"][0]))
    s2, _ = pkg.PTR.solve(pb2, pp, warm=(xd, ud, p))
    for nm in ("xd", "ud", "p", "iterations"):
        np.testing.assert_array_equal(getattr(r, nm), getattr(s2, nm), err_msg=nm)
    np.testing.assert_array_equal(r.cost[:, 3], s2.J_aug)
    pbm.close(); pb2.close()


def test_set_model_par(pkg, gold):
    N, Nsub = int(gold["N"]), int(gold["Nsub"])
    k0, k1 = float(gold["kappa"][0]), float(gold["kappa"][1])
    args = (gold["ref_x"][:, 1], gold["ref_u"][:, 1], gold["ref_p"][:, 1])
    pa, pb = make(pkg, N, Nsub, 5, kappa1=k0), make(pkg, N, Nsub, 5, kappa1=k1)
    assert pa.mutable_model_par() == ("kappa1",)
    pa.set_model_par(kappa1=k1)
    ga, gb = (pkg.PTR.solve_subproblem_(p_, *args, pp=gold["pp"]) for p_ in (pa, pb))
    for nm in ("x", "u", "p", "pcost", "status", "iters"):
        np.testing.assert_array_equal(ga[nm], gb[nm], err_msg=nm)
    # a constant frozen into the handle: refused, nothing changes
    with pytest.raises(pkg._lib.ScpError) as e:
        pa.set_model_par(a_max=0.2)
    assert e.value.code == 1 and "frozen" in str(e.value)
    assert pa.traj.mdl.a_max == 0.3 and pa._par[3] == 0.3
    with pytest.raises(pkg._lib.ScpError):
        pa.set_model_par(kappa=1.0)
    # a second problem on the same TrajectoryProblem keeps the constants its handle was created with
    pc = pkg.PTR.create(pb.pars, pb.traj, batch_capacity=1)
    pc.set_model_par(kappa1=k0)
    assert pc.traj.mdl.par()[5] == k0 and pb.traj.mdl.par()[5] == k1 and pb._par[5] == k1
    pc.close()
    g2 = pkg.PTR.solve_subproblem_(pa, *args, pp=gold["pp"])
    for nm in ("x", "u", "p", "pcost"):
        np.testing.assert_array_equal(g2[nm], gb[nm], err_msg=nm)
    pa.close(); pb.close()


def test_refusals(pkg, gold):
    L = pkg._lib.lib()
    N, Nsub = int(gold["N"]), int(gold["Nsub"])
    pbm = make(pkg, N, Nsub, 2)
    sub = pkg.PTR._generic_sub(pbm)
    assert L.scp_ptr_generic_continue(sub._h, None) == 1            # no run owns the handle
    assert b"continue" in L.scp_sub_last_error(sub._h)
    # both audits: an X row reads the node's own slack
    x, u, p = pbm.traj.guess(N)
    sol = pkg.SubproblemSolutionBatch(x[None], u[None], p[None], pbm)
    for fn in (pkg.audit, pkg.audit_intervals):
        with pytest.raises(pkg._lib.ScpError) as e:
            fn(sol, pbm)
        assert e.value.code == 7
    # a name the model does not mark mutable, and a problem on the structured fast path
    with pytest.raises(pkg._lib.ScpError) as e:
        pkg.PTR.solve_homotopy(pbm, "a_max", [0.3, 0.2])
    assert e.value.code == 1
    pbm.close()
    di = pkg.PTR.create(pkg.PTR.Parameters(N=8, Nsub=5, iter_max=2), pkg.TrajectoryProblem("double_integrator"), batch_capacity=1)
    with pytest.raises(pkg._lib.ScpError) as e:
        pkg.PTR.solve_homotopy(di, "g", [0.1, 0.2])
    assert e.value.code == 7
    pkg.PTR.solve(di)                                               # a structured-path run owns the handle
    sub = pkg.PTR._generic_sub(di)
    assert L.scp_ptr_generic_continue(sub._h, None) == 1
    di.close()


def test_reference_configuration(pkg, gold):
    """oscillator/tests.jl:22-93: N = 30, Nsub = 10, ten stages; the nominal instance plus seven of r0 in [0.15, 1]"""
    pp = np.array([[1.0, 0.0]] + [[r0, 0.0] for r0 in np.linspace(0.15, 1.0, 7)])
    pbm = make(pkg, 30, 10, len(pp))
    sol, hist, summ = pkg.PTR.solve_homotopy(pbm, "kappa1", gold["kappa30"], pp=pp)
    print("N = 30: iterations per stage of the nominal instance %s, oracle %s" % (summ["iterations"][:, 0].tolist(), gold["iterations30"].tolist()))
    assert (summ["status"] == 0).all()
    rel = abs(sol.J[0] - gold["J30"][-1]) / abs(gold["J30"][-1])
    print("nominal J %.6f (oracle %.6f), relative %.3e" % (sol.J[0], gold["J30"][-1], rel))
    assert rel <= 1e-4
    np.testing.assert_array_equal(summ["iterations"][:, 0], summ["iterations"][:, -1])      # the last instance is a copy of the nominal one
    pbm.close()
