"""The continuous-time audit on the device (-m gpu): scp_audit_batch_host against the CPU reference of tests/audit_util.py for the
four supported models, masking and the non-finite flag, scp_audit_resident against scp_audit_batch_host bit for bit behind a
structured PTR run and behind an SCvx loop, and the refusals."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import audit_util as au

pytestmark = pytest.mark.gpu

N, NSUB, B = 8, 3, 67          # one full wavefront plus a partial one: an indexing error in b shows only past 64
OK, BAD, UNSUPPORTED = 0, 1, 7


def _handle(pkg, name, n=N, nsub=NSUB, cap=B, **kw):
    traj = pkg.TrajectoryProblem(name)
    return pkg.PTR.create(pkg.PTR.Parameters(N=n, Nsub=nsub, iter_max=3, **kw), traj, batch_capacity=cap)


def _batch(orc, name, res, Sx, seed0):
    """B different instances (case, reference) at `res`, shared over the session"""
    pairs = [au.reference(orc, name, N, seed0 + b, res, Sx=Sx) for b in range(B)]
    cases, refs = [c for c, _ in pairs], [r for _, r in pairs]
    xd, ud, p, pp = (np.ascontiguousarray(np.stack([c[i] for c in cases])) for i in range(4))
    return SimpleNamespace(xd=xd, ud=ud, p=p), pp, refs


def _raw(pkg, pbm, sol, pp, res, viol_tol, B_=None):
    out = np.full((sol.xd.shape[0], au.W), 77.0)
    sec = ctypes.c_double(-1.0)
    rc = pkg._lib.lib().scp_audit_batch_host(pbm.handle, sol.xd.shape[0] if B_ is None else B_, au.vp(sol.xd), au.vp(sol.ud),
                                             au.vp(sol.p) if pbm.np else None, au.vp(pp), res, float(viol_tol), au.vp(out), ctypes.byref(sec))
    return rc, out, sec.value


@pytest.mark.parametrize("name", au.AUDIT_MODELS)
def test_batch_audit_matches_reference(pkg, orc, name):
    pbm = _handle(pkg, name)
    for res in au.res_values(N):
        sol, pp, refs = _batch(orc, name, res, pbm.scale.Sx, 1000)
        tol = au.choose_viol_tol(refs)
        a = pkg.audit(sol, pbm, pp=pp, res=res, viol_tol=tol)
        assert a.raw.shape == (B, au.W) and a.seconds > 0.0
        for b in range(B):
            refs[b].check(a.raw[b], tol, "%s res=%d b=%d" % (name, res, b))
        assert np.array_equal(a.s_max, a.raw[:, 0]) and np.array_equal(a.cost, a.raw[:, 9])
        # the integration is propagate's own, bit for bit: the drift (one subtraction, one division) of its last sample is the record's
        tc, xc = pkg.propagate(sol, pbm, res=res)
        assert np.array_equal(np.abs((xc[:, -1] - sol.xd[:, -1]) / pbm.scale.Sx).max(axis=1), a.drift)
    pbm.close()


def test_masking_and_the_nonfinite_flag(pkg, orc):
    name, res = "quadrotor", au.res_values(N)[2]
    pbm = _handle(pkg, name)
    sol, pp, refs = _batch(orc, name, res, pbm.scale.Sx, 1000)
    tol = au.choose_viol_tol(refs)
    xd = sol.xd.copy(); xd[5, 0, 1] = np.nan
    status = ["SCP_SOLVED"] * B
    status[9] = "SCP_FAILED (NUMERICAL_ERROR)"
    a = pkg.audit(SimpleNamespace(xd=xd, ud=sol.ud, p=sol.p, status=status), pbm, pp=pp, res=res, viol_tol=tol)
    assert a.nonfinite[5] == 1.0
    assert np.isnan(a.raw[9]).all() and a.skipped[9] and a.skipped.sum() == 1
    for b in range(B):
        if b not in (5, 9):
            refs[b].check(a.raw[b], tol, "b=%d" % b)
    s = a.summary(tol_con=1e-6, tol_bc=1e-3)
    assert s["total"] == B and s["skipped"] == 1 and s["nonfinite"] == 1
    assert s["constraints_pass"] + s["constraints_fail"] == B - 2
    pbm.close()


def _get(pkg, pbm, get_host, handle, b):
    rc, r = pkg.generic.read_result(pbm, b, get_host, handle, (b, 4) if get_host is pkg._lib.lib().scp_ptr_get_host else (2, b),
                                    pkg._lib.HIST_WIDTH)
    assert rc == OK
    return r


def _resident(pkg, pbm, res, viol_tol, cap):
    out = np.full((cap, au.W), 55.0)
    sec = ctypes.c_double(-1.0)
    rc = pkg._lib.lib().scp_audit_resident(pbm.handle, res, float(viol_tol), au.vp(out), ctypes.byref(sec))
    return rc, out, sec.value


def _resident_equals_host(pkg, pbm, get_host, handle, pp, b, res):
    """scp_audit_resident == scp_audit_batch_host on what get_host returns, bit for bit; the run's buffers are left alone"""
    r0 = _get(pkg, pbm, get_host, handle, b)
    rc, res_rec, sec = _resident(pkg, pbm, res, 0.0, b)
    assert rc == OK and sec > 0.0
    r1 = _get(pkg, pbm, get_host, handle, b)
    for k in ("xd", "ud", "p", "status", "iterations", "cost", "feas", "defect", "hist"):
        assert np.array_equal(getattr(r0, k), getattr(r1, k), equal_nan=True), k
    rc, host_rec, _ = _raw(pkg, pbm, r0, pp, res, 0.0)
    assert rc == OK
    ok = r0.status == 0
    print("solved %d of %d; worst s / lin / soc / bc / drift of the solved: %s" % (ok.sum(), b, np.nanmax(res_rec[:, [0, 2, 4, 7, 8]], axis=0)))
    assert res_rec[ok].tobytes() == host_rec[ok].tobytes()
    assert np.isnan(res_rec[~ok]).all()
    return r0, res_rec


def test_resident_equals_host_behind_a_structured_ptr_run(pkg):
    name, res = "quadrotor", 2 * 5 * (N - 1)
    traj = pkg.TrajectoryProblem(name)
    rng = np.random.default_rng(3)
    pp = np.ascontiguousarray(np.stack([traj.mdl.nominal_pp() * (1 + 0.03 * rng.uniform(-1, 1, 12)) for _ in range(B)]))
    L = pkg._lib.lib()
    pbm = _handle(pkg, name, nsub=5)
    assert pkg.PTR.upload(pbm, pp) == B
    for _ in range(3):
        pkg.PTR.iterate(pbm)
    r0, rec = _resident_equals_host(pkg, pbm, L.scp_ptr_get_host, pbm.handle, pp, B, res)
    assert (r0.status == 0).any()
    a = pkg.audit_resident(pbm)                       # the Python entry point: res = 2 Nsub (N - 1), B = the batch PTR.upload started
    assert len(a) == B and a.res == res and a.raw.tobytes() == rec.tobytes()
    pbm.close()
    # failed instances (the subproblem solver stops at its iteration limit of 2): their records are NaN
    pbm = _handle(pkg, name, nsub=5, solver_opts={"maxit": 2})
    assert pkg.PTR.upload(pbm, pp) == B
    pkg.PTR.iterate(pbm)
    r0 = _get(pkg, pbm, L.scp_ptr_get_host, pbm.handle, B)
    assert (r0.status != 0).any()
    rc, rec, _ = _resident(pkg, pbm, res, 0.0, B)
    assert rc == OK and np.isnan(rec[r0.status != 0]).all() and not np.isnan(rec[r0.status == 0]).any()
    pbm.close()


def test_resident_equals_host_behind_an_scvx_loop(pkg):
    """the pp of the SUBPROBLEM handle is the one read (the problem handle's own pp buffer was never written)"""
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
    # before the first iteration get_host returns the reference (the guess): the audit flies that
    r0, rec0 = _resident_equals_host(pkg, pbm, L.scp_scvx_get_host, pbm.sub._h, pp, b, res)
    assert np.array_equal(r0.xd, xd)
    na = ctypes.c_int(-1)
    for _ in range(2):
        assert L.scp_scvx_iterate(pbm.sub._h, ctypes.byref(na)) == OK
    # the host call above staged its input in the solution buffers; the loop has written them again since
    r1, rec1 = _resident_equals_host(pkg, pbm, L.scp_scvx_get_host, pbm.sub._h, pp, b, res)
    ok = r1.status == 0
    assert ok.any()
    # the terminal condition reads pp[6:12] (r_f, v_f): a record computed with another pp differs
    rc, other, _ = _raw(pkg, pbm, r1, np.ascontiguousarray(pp[::-1]), res, 0.0)
    assert rc == OK and not np.array_equal(other[ok][:, 7], rec1[ok][:, 7])
    pbm.close()


def test_refusals(pkg):
    L = pkg._lib.lib()
    out = np.zeros((4, au.W))
    sec = ctypes.c_double(0.0)
    # the free-flyer: node parameters
    traj = pkg.TrajectoryProblem("freeflyer")
    pbm = pkg.PTR.create(pkg.PTR.Parameters(N=N, Nsub=NSUB, iter_max=1), traj, batch_capacity=2)
    x, u, p = traj.guess(N, traj.mdl.nominal_pp())
    sol = SimpleNamespace(xd=np.ascontiguousarray(x[None]), ud=np.ascontiguousarray(u[None]), p=np.ascontiguousarray(p[None]))
    pp = np.ascontiguousarray(traj.mdl.nominal_pp()[None])
    rc, _, _ = _raw(pkg, pbm, sol, pp, 8, 0.0)
    assert rc == UNSUPPORTED and b"node parameters" in L.scp_last_error(pbm.handle)
    assert L.scp_audit_resident(pbm.handle, 8, 0.0, au.vp(out), ctypes.byref(sec)) == UNSUPPORTED
    with pytest.raises(pkg._lib.ScpError) as e:
        pkg.audit(sol, pbm, pp=pp, res=8)
    assert e.value.code == UNSUPPORTED
    pbm.close()
    # an IMPULSE handle
    traj = pkg.TrajectoryProblem("quadrotor")
    pbm = pkg.PTR.create(pkg.PTR.Parameters(N=N, Nsub=NSUB, iter_max=1, disc_method=pkg.IMPULSE), traj, batch_capacity=2)
    x, u, p = traj.guess(N, traj.mdl.nominal_pp())
    sol = SimpleNamespace(xd=np.ascontiguousarray(x[None]), ud=np.ascontiguousarray(u[None]), p=np.ascontiguousarray(p[None]))
    pp = np.ascontiguousarray(traj.mdl.nominal_pp()[None])
    rc, _, _ = _raw(pkg, pbm, sol, pp, 8, 0.0)
    assert rc == UNSUPPORTED and b"FOH" in L.scp_last_error(pbm.handle)
    pbm.close()
    # a FOH handle nobody runs on, and bad arguments
    pbm = _handle(pkg, "quadrotor", cap=2)
    assert L.scp_audit_resident(pbm.handle, 8, 0.0, au.vp(out), ctypes.byref(sec)) == BAD           # RUN_NONE
    assert b"no run" in L.scp_last_error(pbm.handle)
    assert _raw(pkg, pbm, sol, pp, 1, 0.0)[0] == BAD                                                # res = 1
    assert L.scp_audit_resident(pbm.handle, 1, 0.0, au.vp(out), ctypes.byref(sec)) == BAD
    assert L.scp_audit_batch_host(pbm.handle, 1, au.vp(sol.xd), au.vp(sol.ud), au.vp(sol.p), au.vp(pp), 8, 0.0, None, None) == BAD
    assert L.scp_audit_batch_host(pbm.handle, 1, au.vp(sol.xd), au.vp(sol.ud), None, au.vp(pp), 8, 0.0, au.vp(out), None) == BAD
    assert L.scp_audit_batch_host(pbm.handle, 1, au.vp(sol.xd), au.vp(sol.ud), au.vp(sol.p), None, 8, 0.0, au.vp(out), None) == BAD
    big = SimpleNamespace(xd=np.repeat(sol.xd, 3, 0), ud=np.repeat(sol.ud, 3, 0), p=np.repeat(sol.p, 3, 0))
    assert _raw(pkg, pbm, big, np.repeat(pp, 3, 0), 8, 0.0)[0] == 6                                  # SCP_ERR_BATCH_TOO_LARGE
    rc, rec, _ = _raw(pkg, pbm, sol, pp, 8, 0.0)
    assert rc == OK and np.isfinite(rec[0, [1, 3, 5, 7, 8, 9, 10, 11]]).all() and rec[0, 11] == 0.0
    pbm.close()
