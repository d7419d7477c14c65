"""The interval-parallel audit on the device (-m gpu): scp_audit_intervals_batch_host against the CPU reference of
tests/audit_intervals_util.py (four models under FOH, two under IMPULSE), a problem that spans more than one wavefront, the
independence of the batch, masking and the non-finite flag, scp_audit_intervals_resident against the host variant bit for bit
behind a structured PTR run (FOH and IMPULSE) and behind an SCvx loop, and the refusals."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import audit_intervals_util as aiu
import audit_util as au

pytestmark = pytest.mark.gpu

N, NSUB, B = 8, 3, 67          # 469 threads: waves straddle the problem boundaries and the last wave is partial
OK, BAD, TOO_LARGE, UNSUPPORTED = 0, 1, 6, 7


def _handle(pkg, name, method=aiu.FOH, n=N, nsub=NSUB, cap=B, **kw):
    traj = pkg.TrajectoryProblem(name)
    return pkg.PTR.create(pkg.PTR.Parameters(N=n, Nsub=nsub, iter_max=3, disc_method=pkg.FOH if method == aiu.FOH else pkg.IMPULSE, **kw),
                          traj, batch_capacity=cap)


def _batch(orc, name, method, res, Sx, seed0, n=N, b=B):
    """b different instances (case, reference) at `res`, shared over the session"""
    pairs = [aiu.reference(orc, name, method, n, seed0 + i, res, Sx=Sx) for i in range(b)]
    cases, refs = [c for c, _ in pairs], [r for _, r in pairs]
    xd, ud, p, pp = (np.ascontiguousarray(np.stack([c[i] for c in cases])) for i in range(4))
    return SimpleNamespace(xd=xd, ud=ud, p=p), pp, refs


def _raw(pkg, pbm, sol, pp, res, viol_tol, B_=None, intervals=True):
    b, n = sol.xd.shape[0], sol.xd.shape[1]
    out, rec = np.full((b, aiu.W), 77.0), np.full((b, n - 1, aiu.WI), 78.0)
    sec = ctypes.c_double(-1.0)
    rc = pkg._lib.lib().scp_audit_intervals_batch_host(pbm.handle, b if B_ is None else B_, au.vp(sol.xd), au.vp(sol.ud),
                                                       au.vp(sol.p) if pbm.np else None, au.vp(pp), res, float(viol_tol), au.vp(out),
                                                       au.vp(rec) if intervals else None, ctypes.byref(sec))
    return rc, out, rec, sec.value


@pytest.mark.parametrize("name,method", aiu.CASES)
def test_batch_interval_audit_matches_reference(pkg, orc, name, method):
    pbm = _handle(pkg, name, method)
    for res in aiu.res_values(N):
        sol, pp, refs = _batch(orc, name, method, res, pbm.scale.Sx, 2000)
        tol = au.choose_viol_tol(refs)
        a = pkg.audit_intervals(sol, pbm, pp=pp, res=res, viol_tol=tol)
        assert a.raw.shape == (B, aiu.W) and a.intervals.shape == (B, N - 1, aiu.WI) and a.seconds > 0.0 and a.sub == refs[0].sub
        for b in range(B):
            refs[b].check(a.raw[b], a.intervals[b], tol, "%s/%d res=%d b=%d" % (name, method, res, b))
        assert np.array_equal(a.defect, a.raw[:, 8]) and np.array_equal(a.worst_interval, a.raw[:, 12].astype(int))
    pbm.close()


@pytest.mark.parametrize("method", [aiu.FOH, aiu.IMPULSE])
def test_a_problem_wider_than_a_wavefront(pkg, orc, method):
    """N = 66: the 65 intervals of one problem span two wavefronts, and the summary is still the ORDERED fold of its records"""
    name, n, b, res = "double_integrator", 66, 3, 2
    pbm = _handle(pkg, name, method, n=n, cap=b)
    sol, pp, refs = _batch(orc, name, method, res, pbm.scale.Sx, 3000, n=n, b=b)
    tol = au.choose_viol_tol(refs)
    a = pkg.audit_intervals(sol, pbm, pp=pp, res=res, viol_tol=tol)
    for i in range(b):
        refs[i].check(a.raw[i], a.intervals[i], tol, "N=66 b=%d" % i)
        assert a.raw[i].tobytes() == aiu.fold(a.intervals[i], a.raw[i, 6], False, 2).tobytes()
    pbm.close()


@pytest.mark.parametrize("name,method", [("quadrotor", aiu.FOH), ("quadrotor", aiu.IMPULSE), ("starship", aiu.FOH)])
def test_results_do_not_depend_on_the_batch(pkg, orc, name, method):
    """instance b of the batch of 67, audited alone at B = 1: identical bits for the summary and the interval records"""
    res = aiu.res_values(N)[2]
    pbm = _handle(pkg, name, method)
    sol, pp, refs = _batch(orc, name, method, res, pbm.scale.Sx, 2000)
    rc, out, rec, _ = _raw(pkg, pbm, sol, pp, res, 0.0)
    assert rc == OK
    for b in (0, 9, 63, 64, 66):
        one = SimpleNamespace(xd=np.ascontiguousarray(sol.xd[b:b + 1]), ud=np.ascontiguousarray(sol.ud[b:b + 1]), p=np.ascontiguousarray(sol.p[b:b + 1]))
        rc, o1, r1, _ = _raw(pkg, pbm, one, np.ascontiguousarray(pp[b:b + 1]), res, 0.0)
        assert rc == OK and o1[0].tobytes() == out[b].tobytes() and r1[0].tobytes() == rec[b].tobytes(), b
        assert out[b].tobytes() == aiu.fold(rec[b], out[b, 6], np.isfinite(refs[b].summary[6]), refs[b].sub).tobytes()
    pbm.close()


@pytest.mark.parametrize("method", [aiu.FOH, aiu.IMPULSE])
def test_masking_and_the_nonfinite_flag(pkg, orc, method):
    name, res = "quadrotor", aiu.res_values(N)[2]
    pbm = _handle(pkg, name, method)
    sol, pp, refs = _batch(orc, name, method, res, pbm.scale.Sx, 2000)
    tol = au.choose_viol_tol(refs)
    xd = sol.xd.copy(); xd[5, 3, 1] = np.nan             # node 4 of instance 5: the intervals 3 and 4 read it
    status = ["SCP_SOLVED"] * B
    status[9] = "SCP_FAILED (NUMERICAL_ERROR)"
    bad = SimpleNamespace(xd=xd, ud=sol.ud, p=sol.p, status=status)
    a = pkg.audit_intervals(bad, pbm, pp=pp, res=res, viol_tol=tol)
    assert a.nonfinite[5] == 1.0 and np.array_equal(np.nonzero(a.intervals[5, :, 9])[0] + 1, [3, 4])
    assert np.isnan(a.raw[9]).all() and np.isnan(a.intervals[9]).all() and a.skipped[9] and a.skipped.sum() == 1
    assert a.worst_interval[9] == -1 and (np.delete(a.worst_interval, 9) >= 1).all()
    for b in range(B):
        if b not in (5, 9):
            refs[b].check(a.raw[b], a.intervals[b], tol, "b=%d" % b)
    s = a.summary(tol_con=1e-6, tol_bc=1e-3)
    assert s["total"] == B and s["skipped"] == 1 and s["nonfinite"] == 1
    a2 = pkg.audit_intervals(bad, pbm, pp=pp, res=res, viol_tol=tol, intervals=False)
    assert a2.intervals is None and a2.raw.tobytes() == a.raw.tobytes()
    pbm.close()


def _get(pkg, pbm, get_host, handle, b):
    rc, r = pkg.generic.read_result(pbm, b, get_host, handle, (b, 4) if get_host is pkg._lib.lib().scp_ptr_get_host else (2, b),
                                    pkg._lib.HIST_WIDTH)
    assert rc == OK
    return r


def _resident(pkg, pbm, res, viol_tol, cap, n, intervals=True):
    out, rec = np.full((cap, aiu.W), 55.0), np.full((cap, n - 1, aiu.WI), 56.0)
    sec = ctypes.c_double(-1.0)
    rc = pkg._lib.lib().scp_audit_intervals_resident(pbm.handle, res, float(viol_tol), au.vp(out), au.vp(rec) if intervals else None,
                                                     ctypes.byref(sec))
    return rc, out, rec, sec.value


def _resident_equals_host(pkg, pbm, get_host, handle, pp, b, res):
    """scp_audit_intervals_resident == scp_audit_intervals_batch_host on what get_host returns, bit for bit on the solved instances
    and NaN on the others; the run's buffers are left alone"""
    n = pbm.pars.N
    r0 = _get(pkg, pbm, get_host, handle, b)
    rc, res_out, res_rec, sec = _resident(pkg, pbm, res, 0.0, b, n)
    assert rc == OK and sec > 0.0
    rc, only, _, _ = _resident(pkg, pbm, res, 0.0, b, n, intervals=False)
    assert rc == OK and only.tobytes() == res_out.tobytes()
    r1 = _get(pkg, pbm, get_host, handle, b)
    for k in ("xd", "ud", "p", "status", "iterations", "cost", "feas", "defect", "hist"):
        assert np.array_equal(getattr(r0, k), getattr(r1, k), equal_nan=True), k
    rc, host_out, host_rec, _ = _raw(pkg, pbm, r0, pp, res, 0.0)
    assert rc == OK
    ok = r0.status == 0
    print("solved %d of %d" % (ok.sum(), b))
    if ok.any():
        print("worst s / lin / soc / bc / defect of the solved: %s" % np.max(res_out[ok][:, [0, 2, 4, 7, 8]], axis=0))
    assert res_out[ok].tobytes() == host_out[ok].tobytes() and res_rec[ok].tobytes() == host_rec[ok].tobytes()
    assert np.isnan(res_out[~ok]).all() and np.isnan(res_rec[~ok]).all()
    return r0, res_out, res_rec


@pytest.mark.parametrize("method", [aiu.FOH, aiu.IMPULSE])
def test_resident_equals_host_behind_a_structured_ptr_run(pkg, method):
    """FOH: at least one instance is solved after three iterations.  IMPULSE: whether any is solved is not known; the count is
    printed, the solved ones are compared and none is required"""
    name, res = "quadrotor", 2 * 5 * (N - 1)
    traj = pkg.TrajectoryProblem(name)
    rng = np.random.default_rng(3)
    pp = np.ascontiguousarray(np.stack([traj.mdl.nominal_pp() * (1 + 0.03 * rng.uniform(-1, 1, 12)) for _ in range(B)]))
    pbm = _handle(pkg, name, method, nsub=5)
    assert pkg.PTR.upload(pbm, pp) == B
    for _ in range(3):
        pkg.PTR.iterate(pbm)
    r0, out, rec = _resident_equals_host(pkg, pbm, pkg._lib.lib().scp_ptr_get_host, pbm.handle, pp, B, res)
    if method == aiu.FOH:
        assert (r0.status == 0).any()
    a = pkg.audit_intervals_resident(pbm)                 # the Python entry point: res = 2 Nsub (N - 1), B = the batch PTR.upload started
    assert len(a) == B and a.res == res and a.sub == 10 and a.raw.tobytes() == out.tobytes() and a.intervals.tobytes() == rec.tobytes()
    assert pkg.audit_intervals_resident(pbm, intervals=False).intervals is None
    pbm.close()


def test_resident_equals_host_behind_an_scvx_loop(pkg):
    """the pp of the SUBPROBLEM handle is the one read"""
    n, nsub, b = 12, 8, 5          # the quadrotor SCvx case of tests/test_template_cpu.py
    traj = pkg.TrajectoryProblem("quadrotor")
    pars = pkg.SCvx.Parameters(N=n, Nsub=nsub, iter_max=3, lam=30.0, rho_0=0.0, rho_1=0.1, rho_2=0.7, beta_sh=2.0, beta_gr=2.0,
                               eta_init=1.0, eta_lb=1e-3, eta_ub=10.0, eps_abs=1e-4, eps_rel=1e-3)
    pbm = pkg.SCvx.create(pars, traj, batch_capacity=8)
    rng = np.random.default_rng(4)
    pp = np.ascontiguousarray(np.stack([traj.mdl.nominal_pp() * (1 + 0.05 * rng.uniform(-1, 1, 12)) for _ in range(b)]))
    g = [traj.guess(n, pp[i]) for i in range(b)]
    xd, ud, p = (np.ascontiguousarray(np.stack([gi[j] for gi in g]), np.float64) for j in range(3))
    L = pkg._lib.lib()
    cp = pars.c_struct()
    assert L.scp_scvx_init_host(pbm.sub._h, None, b, ctypes.byref(cp), au.vp(xd), au.vp(ud), au.vp(p), au.vp(pp)) == OK
    res = 2 * nsub * (n - 1)
    r0, _, _ = _resident_equals_host(pkg, pbm, L.scp_scvx_get_host, pbm.sub._h, pp, b, res)
    assert np.array_equal(r0.xd, xd)
    na = ctypes.c_int(-1)
    for _ in range(2):
        assert L.scp_scvx_iterate(pbm.sub._h, ctypes.byref(na)) == OK
    r1, out1, _ = _resident_equals_host(pkg, pbm, L.scp_scvx_get_host, pbm.sub._h, pp, b, res)
    ok = r1.status == 0
    assert ok.any()
    # the terminal condition reads pp[6:12] (r_f, v_f): a record computed with another target position differs.  (Other instances'
    # pp would not do: v_f = 0 in all of them, and the residual of a flown last interval can be largest in the velocity.)
    far = pp.copy(); far[:, 6:9] += 10.0
    rc, other, _, _ = _raw(pkg, pbm, r1, far, res, 0.0)
    assert rc == OK and (other[ok][:, 7] != out1[ok][:, 7]).all()
    pbm.close()


def test_refusals(pkg):
    L = pkg._lib.lib()
    out, rec = np.zeros((4, aiu.W)), np.zeros((4, N - 1, aiu.WI))
    sec = ctypes.c_double(0.0)
    # the free-flyer: node parameters
    traj = pkg.TrajectoryProblem("freeflyer")
    pbm = pkg.PTR.create(pkg.PTR.Parameters(N=N, Nsub=NSUB, iter_max=1), traj, batch_capacity=2)
    x, u, p = traj.guess(N, traj.mdl.nominal_pp())
    sol = SimpleNamespace(xd=np.ascontiguousarray(x[None]), ud=np.ascontiguousarray(u[None]), p=np.ascontiguousarray(p[None]))
    pp = np.ascontiguousarray(traj.mdl.nominal_pp()[None])
    assert _raw(pkg, pbm, sol, pp, 8, 0.0)[0] == UNSUPPORTED and b"node parameters" in L.scp_last_error(pbm.handle)
    assert L.scp_audit_intervals_resident(pbm.handle, 8, 0.0, au.vp(out), au.vp(rec), ctypes.byref(sec)) == UNSUPPORTED
    with pytest.raises(pkg._lib.ScpError) as e:
        pkg.audit_intervals(sol, pbm, pp=pp, res=8)
    assert e.value.code == UNSUPPORTED
    pbm.close()
    # a handle nobody runs on, and bad arguments
    traj = pkg.TrajectoryProblem("quadrotor")
    x, u, p = traj.guess(N, traj.mdl.nominal_pp())
    sol = SimpleNamespace(xd=np.ascontiguousarray(x[None]), ud=np.ascontiguousarray(u[None]), p=np.ascontiguousarray(p[None]))
    pp = np.ascontiguousarray(traj.mdl.nominal_pp()[None])
    for method in (aiu.FOH, aiu.IMPULSE):
        pbm = _handle(pkg, "quadrotor", method, cap=2)
        assert L.scp_audit_intervals_resident(pbm.handle, 8, 0.0, au.vp(out), au.vp(rec), ctypes.byref(sec)) == BAD       # RUN_NONE
        assert b"no run" in L.scp_last_error(pbm.handle)
        assert _raw(pkg, pbm, sol, pp, 1, 0.0)[0] == BAD                                                                # res = 1
        assert L.scp_audit_intervals_resident(pbm.handle, 1, 0.0, au.vp(out), au.vp(rec), ctypes.byref(sec)) == BAD
        args = (au.vp(sol.xd), au.vp(sol.ud))
        assert L.scp_audit_intervals_batch_host(pbm.handle, 1, *args, au.vp(sol.p), au.vp(pp), 8, 0.0, None, au.vp(rec), None) == BAD
        assert L.scp_audit_intervals_batch_host(pbm.handle, 1, *args, None, au.vp(pp), 8, 0.0, au.vp(out), au.vp(rec), None) == BAD
        assert L.scp_audit_intervals_batch_host(pbm.handle, 1, *args, au.vp(sol.p), None, 8, 0.0, au.vp(out), au.vp(rec), None) == BAD
        big = SimpleNamespace(xd=np.repeat(sol.xd, 3, 0), ud=np.repeat(sol.ud, 3, 0), p=np.repeat(sol.p, 3, 0))
        assert _raw(pkg, pbm, big, np.repeat(pp, 3, 0), 8, 0.0)[0] == TOO_LARGE
        rc, o, r, _ = _raw(pkg, pbm, sol, pp, 8, 0.0)
        assert rc == OK and np.isfinite(o[0, [1, 3, 5, 7, 8, 9, 10, 11]]).all() and o[0, 11] == 0.0 and o[0, 13] == 1.0 and o[0, 14] == 2.0
        assert np.isfinite(r[0][:, 6:]).all()
        pbm.close()
