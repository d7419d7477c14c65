"""The dispersed-flight audit on the device (-m gpu): scp_audit_dispersed_batch_host against the CPU reference of
tests/audit_dispersed_util.py (four models, with and without a truth model), the launch geometry (a problem's flights across two
wavefronts, every flight against the same flight alone, the ordered fold, SCP_DISP_SHARED, flights = NULL), the resident variant
against the host variant bit for bit behind a structured PTR run, and the refusals."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import audit_dispersed_util as adu
import audit_util as au

pytestmark = pytest.mark.gpu

N, NSUB, B, D = 5, 3, 3, adu.D3
OK, BAD, TOO_LARGE, UNSUPPORTED = 0, 1, 6, 7
SHARED = 1


def _handle(pkg, name, n=N, nsub=NSUB, cap=B, **kw):
    return pkg.PTR.create(pkg.PTR.Parameters(N=n, Nsub=nsub, iter_max=3, **kw), pkg.TrajectoryProblem(name), batch_capacity=cap)


def _raw(pkg, pbm, sol, pp, res, viol_tol, d, dx0, gain, bias, flags=0, par_true=None, flights=True, B_=None):
    b = sol.xd.shape[0]
    out, rec = np.full((b, au.W), 77.0), np.full((b, d, au.W), 78.0)
    sec = ctypes.c_double(-1.0)
    rc = pkg._lib.lib().scp_audit_dispersed_batch_host(pbm.handle, b if B_ is None else B_, au.vp(sol.xd), au.vp(sol.ud),
                                                       au.vp(sol.p) if pbm.np else None, au.vp(pp), res, float(viol_tol), d, au.vp(dx0),
                                                       au.vp(gain), au.vp(bias), flags, au.vp(par_true), au.vp(out),
                                                       au.vp(rec) if flights else None, ctypes.byref(sec))
    return rc, out, rec, sec.value


def _batch(orc, name, res, Sx):
    """B distinct cases with their own three flights each: the case of the CPU tests first, shared with them over the session"""
    seeds = [adu.SEEDS[name] + N] + [2000 + i for i in range(1, B)]
    trip = [adu.reference(orc, name, N, s, res, disp_seed=1000 + N + i, Sx=Sx) for i, s in enumerate(seeds)]
    xd, ud, p, pp = (np.ascontiguousarray(np.stack([t[0][i] for t in trip])) for i in range(4))
    disp = tuple(np.ascontiguousarray(np.stack([t[1][i] for t in trip])) for i in range(3))        # [B, D, n]
    return SimpleNamespace(xd=xd, ud=ud, p=p), pp, disp, [t[2] for t in trip]


@pytest.mark.parametrize("name", au.AUDIT_MODELS)
def test_batch_flights_match_reference(pkg, orc, name):
    pbm = _handle(pkg, name)
    for res in au.res_values(N):
        sol, pp, disp, refs = _batch(orc, name, res, pbm.scale.Sx)
        tol = au.choose_viol_tol([r for rb in refs for r in rb])
        a = pkg.audit_dispersed(sol, pbm, *disp, pp=pp, res=res, viol_tol=tol, flights=True)
        assert a.raw.shape == (B, au.W) and a.flights.shape == (B, D, au.W) and a.D == D and a.seconds > 0.0 and not a.skipped.any()
        for b in range(B):
            for d in range(D):
                refs[b][d].check(a.flights[b, d], tol, "%s res=%d b=%d d=%d" % (name, res, b, d + 1))
            assert a.raw[b].tobytes() == adu.fold(a.flights[b]).tobytes(), (b, a.raw[b], adu.fold(a.flights[b]))
        assert np.array_equal(a.flight_batch(1).raw, a.flights[1]) and np.array_equal(a.cost_max, a.raw[:, 15])
    pbm.close()


@pytest.mark.parametrize("name", ["quadrotor", "rocket_landing"])
def test_truth_model_on_the_device(pkg, orc, name):
    res = au.res_values(N)[2]
    pbm = _handle(pkg, name)
    sol, pp, disp, nominal = _batch(orc, name, res, pbm.scale.Sx)
    blob, tr = adu.truth(pkg, orc, name, N)
    refs = [adu.flight_references(orc, name, N, (sol.xd[b], sol.ud[b], sol.p[b], pp[b]), pbm.scale.Sx, res, *(a[b] for a in disp), truth=tr)
            for b in range(B)]
    tol = au.choose_viol_tol([r for rb in refs for r in rb])
    rc, out, rec, _ = _raw(pkg, pbm, sol, pp, res, tol, D, *disp, par_true=blob)
    assert rc == OK
    for b in range(B):
        for d in range(D):
            refs[b][d].check(rec[b, d], tol, "%s truth b=%d d=%d" % (name, b, d + 1))
        assert out[b].tobytes() == adu.fold(rec[b]).tobytes()
    # the Python entry point builds the same blob from a dict of overrides and from a model instance; the handle keeps its constants
    over = dict(g=9.81 * 1.05) if name == "quadrotor" else dict(g=blob[0:3], alpha=blob[6], rho_max=blob[10])
    for model in (over, pkg.REGISTRY[name](**over)):
        a = pkg.audit_dispersed(sol, pbm, *disp, model=model, pp=pp, res=res, viol_tol=tol, flights=True)
        assert a.raw.tobytes() == out.tobytes() and a.flights.tobytes() == rec.tobytes()
    rc, out0, rec0, _ = _raw(pkg, pbm, sol, pp, res, tol, D, *disp)
    assert rc == OK and (rec0[:, :, 9] != rec[:, :, 9]).all()
    rc, same, rsame, _ = _raw(pkg, pbm, sol, pp, res, tol, D, *disp, par_true=au.model_blob(pkg, name, N))
    assert rc == OK and same.tobytes() == out0.tobytes() and rsame.tobytes() == rec0.tobytes()
    pbm.close()


def test_geometry(pkg, orc):
    """B = 5, D = 13: 65 threads, the flights of the last problem straddle two wavefronts"""
    name, b, d, res = "quadrotor", 5, 13, au.res_values(N)[2]
    pbm = _handle(pkg, name, cap=b)
    cases = [au.make_case(name, N, 3000 + i) for i in range(b)]
    xd, ud, p, pp = (np.ascontiguousarray(np.stack([c[i] for c in cases])) for i in range(4))
    sol = SimpleNamespace(xd=xd, ud=ud, p=p)
    rng = np.random.default_rng(7)
    ub = np.asarray(au.oracle_model(name, N).bbox()[1], float)
    dx0 = 0.01 * pbm.scale.Sx * rng.standard_normal((b, d, 6))
    gain = 1.0 + 0.02 * rng.standard_normal((b, d, 4))
    bias = 0.01 * (ub[:, 1] - ub[:, 0]) * rng.standard_normal((b, d, 4))
    dx0[:, 0], gain[:, 0], bias[:, 0] = 0.0, 1.0, 0.0
    rc, out, rec, sec = _raw(pkg, pbm, sol, pp, res, 0.0, d, dx0, gain, bias)
    assert rc == OK and sec > 0.0 and (rec[:, :, 11] == 0.0).all() and not rec[:, :, 12:].any()
    for i in range(b):
        one = SimpleNamespace(xd=xd[i:i + 1].copy(), ud=ud[i:i + 1].copy(), p=p[i:i + 1].copy())
        for j in range(d):
            rc, o1, r1, _ = _raw(pkg, pbm, one, pp[i:i + 1].copy(), res, 0.0, 1, dx0[i, j].copy(), gain[i, j].copy(), bias[i, j].copy())
            assert rc == OK and r1[0, 0].tobytes() == rec[i, j].tobytes(), (i, j)
            assert o1[0].tobytes() == adu.fold(rec[i, j:j + 1]).tobytes()
        assert out[i].tobytes() == adu.fold(rec[i]).tobytes(), i
    rc, only, _, _ = _raw(pkg, pbm, sol, pp, res, 0.0, d, dx0, gain, bias, flights=False)
    assert rc == OK and only.tobytes() == out.tobytes()
    # SCP_DISP_SHARED == the same [D, .] arrays tiled over the batch
    tile = lambda a: np.ascontiguousarray(np.tile(a[None], (b, 1, 1)))      # noqa: E731
    rc, out_t, rec_t, _ = _raw(pkg, pbm, sol, pp, res, 0.0, d, tile(dx0[2]), tile(gain[2]), tile(bias[2]))
    assert rc == OK
    rc, out_s, rec_s, _ = _raw(pkg, pbm, sol, pp, res, 0.0, d, dx0[2].copy(), gain[2].copy(), bias[2].copy(), flags=SHARED)
    assert rc == OK and out_s.tobytes() == out_t.tobytes() and rec_s.tobytes() == rec_t.tobytes()
    a = pkg.audit_dispersed(sol, pbm, dx0[2], gain[2], bias[2], shared=True, pp=pp, res=res, flights=True)
    assert a.raw.tobytes() == out_t.tobytes() and a.flights.tobytes() == rec_t.tobytes()
    # NULL arrays are 0 / 1 / 0, and a failed problem is masked by the Python wrapper
    rc, out_n, rec_n, _ = _raw(pkg, pbm, sol, pp, res, 0.0, 2, None, None, None)
    assert rc == OK and rec_n[:, 0].tobytes() == rec[:, 0].tobytes() and rec_n[:, 1].tobytes() == rec[:, 0].tobytes()
    sol.status = ["SCP_SOLVED"] * b
    sol.status[3] = "SCP_FAILED (NUMERICAL_ERROR)"
    a = pkg.audit_dispersed(sol, pbm, dx0, gain, bias, pp=pp, res=res, flights=True)
    assert list(a.skipped) == [False, False, False, True, False] and np.isnan(a.flights[3]).all() and np.isnan(a.raw[3]).all()
    assert np.delete(a.raw, 3, 0).tobytes() == np.delete(out, 3, 0).tobytes()
    pbm.close()


def _get(pkg, pbm, b):
    rc, r = pkg.generic.read_result(pbm, b, pkg._lib.lib().scp_ptr_get_host, pbm.handle, (b, 4), pkg._lib.HIST_WIDTH)
    assert rc == OK
    return r


def test_resident_equals_host_behind_a_structured_ptr_run(pkg):
    name, n, b, d = "quadrotor", 8, 4, 3
    res = 2 * 5 * (n - 1)
    traj = pkg.TrajectoryProblem(name)
    rng = np.random.default_rng(3)
    pp = np.ascontiguousarray(np.stack([traj.mdl.nominal_pp() * (1 + 0.03 * rng.uniform(-1, 1, 12)) for _ in range(b)]))
    pbm = pkg.PTR.create(pkg.PTR.Parameters(N=n, Nsub=5, iter_max=2), traj, batch_capacity=b)
    assert pkg.PTR.upload(pbm, pp) == b
    for _ in range(2):
        pkg.PTR.iterate(pbm)
    dx0 = 0.01 * pbm.scale.Sx * rng.standard_normal((b, d, 6))
    gain = 1.0 + 0.02 * rng.standard_normal((b, d, 4))
    bias = 0.1 * rng.standard_normal((b, d, 4))
    r0 = _get(pkg, pbm, b)
    out, rec = np.full((b, au.W), 55.0), np.full((b, d, au.W), 56.0)
    sec = ctypes.c_double(-1.0)
    L = pkg._lib.lib()
    assert L.scp_audit_dispersed_resident(pbm.handle, res, 0.0, d, au.vp(dx0), au.vp(gain), au.vp(bias), 0, None, au.vp(out), au.vp(rec),
                                          ctypes.byref(sec)) == OK and sec.value > 0.0
    only = np.full((b, au.W), 57.0)
    assert L.scp_audit_dispersed_resident(pbm.handle, res, 0.0, d, au.vp(dx0), au.vp(gain), au.vp(bias), 0, None, au.vp(only), None, None) == OK
    assert only.tobytes() == out.tobytes()
    a = pkg.audit_dispersed_resident(pbm, dx0, gain, bias, flights=True)      # res = 2 Nsub (N - 1), B = the batch PTR.upload started
    assert len(a) == b and a.res == res and a.D == d and a.raw.tobytes() == out.tobytes() and a.flights.tobytes() == rec.tobytes()
    r1 = _get(pkg, pbm, b)
    for k in ("xd", "ud", "p", "status", "iterations", "cost", "feas", "defect", "hist"):
        assert np.array_equal(getattr(r0, k), getattr(r1, k), equal_nan=True), k
    rc, host_out, host_rec, _ = _raw(pkg, pbm, r0, pp, res, 0.0, d, dx0, gain, bias)
    assert rc == OK
    ok = r0.status == 0
    print("solved %d of %d" % (ok.sum(), b))
    assert out[ok].tobytes() == host_out[ok].tobytes() and rec[ok].tobytes() == host_rec[ok].tobytes()
    assert np.isnan(out[~ok]).all() and np.isnan(rec[~ok]).all() and list(a.skipped) == list(~ok)
    assert not np.isnan(host_out[:, 10:15]).any()
    pbm.close()
    # failed instances (the subproblem solver stops at its iteration limit of 2): their summary and all their flights are NaN
    pbm = pkg.PTR.create(pkg.PTR.Parameters(N=n, Nsub=5, iter_max=2, solver_opts={"maxit": 2}), traj, batch_capacity=b)
    assert pkg.PTR.upload(pbm, pp) == b
    pkg.PTR.iterate(pbm)
    bad = _get(pkg, pbm, b).status != 0
    print("failed %d of %d" % (bad.sum(), b))
    assert bad.any()
    a = pkg.audit_dispersed_resident(pbm, dx0, gain, bias, flights=True)
    assert np.isnan(a.raw[bad]).all() and np.isnan(a.flights[bad]).all() and not np.isnan(a.raw[~bad][:, 10:15]).any()
    assert list(a.skipped) == list(bad)
    pbm.close()


def test_refusals(pkg):
    L = pkg._lib.lib()
    one = np.zeros((1, 1, 16))
    # an IMPULSE handle and the free-flyer (node parameters): refused with a text
    for name, kw, text in (("quadrotor", dict(disc_method=pkg.IMPULSE), b"FOH handles only"), ("freeflyer", {}, b"node parameters")):
        traj = pkg.TrajectoryProblem(name)
        pbm = pkg.PTR.create(pkg.PTR.Parameters(N=N, Nsub=NSUB, iter_max=1, **kw), traj, batch_capacity=2)
        x, u, p = traj.guess(N, traj.mdl.nominal_pp())
        sol = SimpleNamespace(xd=np.ascontiguousarray(x[None]), ud=np.ascontiguousarray(u[None]), p=np.ascontiguousarray(p[None]))
        pp = np.ascontiguousarray(traj.mdl.nominal_pp()[None])
        assert _raw(pkg, pbm, sol, pp, 8, 0.0, 1, None, None, None)[0] == UNSUPPORTED and text in L.scp_last_error(pbm.handle)
        assert L.scp_audit_dispersed_resident(pbm.handle, 8, 0.0, 1, None, None, None, 0, None, au.vp(one), None, None) == UNSUPPORTED
        with pytest.raises(pkg._lib.ScpError) as e:
            pkg.audit_dispersed(sol, pbm, pp=pp, res=8)
        assert e.value.code == UNSUPPORTED
        pbm.close()
    # bad arguments, a batch above the capacity, and the handle stays usable
    traj = pkg.TrajectoryProblem("quadrotor")
    pbm = _handle(pkg, "quadrotor", cap=2)
    x, u, p = traj.guess(N, traj.mdl.nominal_pp())
    sol = SimpleNamespace(xd=np.ascontiguousarray(x[None]), ud=np.ascontiguousarray(u[None]), p=np.ascontiguousarray(p[None]))
    pp = np.ascontiguousarray(traj.mdl.nominal_pp()[None])
    assert L.scp_audit_dispersed_resident(pbm.handle, 8, 0.0, 1, None, None, None, 0, None, au.vp(one), None, None) == BAD      # RUN_NONE
    assert b"no run" in L.scp_last_error(pbm.handle)
    assert _raw(pkg, pbm, sol, pp, 8, 0.0, 0, None, None, None)[0] == BAD                               # D = 0
    assert _raw(pkg, pbm, sol, pp, 1, 0.0, 1, None, None, None)[0] == BAD                               # res = 1
    assert _raw(pkg, pbm, sol, pp, 8, 0.0, 1, None, None, None, flags=2)[0] == BAD                      # an unknown flag bit
    args = (au.vp(sol.xd), au.vp(sol.ud))
    tail = (8, 0.0, 1, None, None, None, 0, None)
    assert L.scp_audit_dispersed_batch_host(pbm.handle, 1, *args, au.vp(sol.p), au.vp(pp), *tail, None, None, None) == BAD      # NULL summary
    assert L.scp_audit_dispersed_batch_host(pbm.handle, 1, *args, None, au.vp(pp), *tail, au.vp(one), None, None) == BAD
    assert L.scp_audit_dispersed_batch_host(pbm.handle, 1, *args, au.vp(sol.p), None, *tail, au.vp(one), None, None) == BAD
    big = SimpleNamespace(xd=np.repeat(sol.xd, 3, 0), ud=np.repeat(sol.ud, 3, 0), p=np.repeat(sol.p, 3, 0))
    assert _raw(pkg, pbm, big, np.repeat(pp, 3, 0), 8, 0.0, 1, None, None, None)[0] == TOO_LARGE
    assert b"batch_capacity" in L.scp_last_error(pbm.handle)
    rc, o, r, _ = _raw(pkg, pbm, sol, pp, 8, 0.0, 2, None, None, None)
    assert rc == OK and o[0, 11] == 0.0 and o[0, 13] == 2.0 and o[0, 14] == 2.0 and np.isfinite(o[0, [7, 8, 9, 15]]).all()
    assert r[0, 0].tobytes() == r[0, 1].tobytes() and r[0, 0, 11] == 0.0
    # more flights than the buffers were built for: they are rebuilt
    rc, o5, r5, _ = _raw(pkg, pbm, sol, pp, 8, 0.0, 5, None, None, None)
    assert rc == OK and o5[0, 14] == 5.0 and all(r5[0, j].tobytes() == r[0, 0].tobytes() for j in range(5))
    pbm.close()
