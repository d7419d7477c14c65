"""The Monte-Carlo audit on the device (-m gpu): scp_audit_montecarlo_batch_host against the CPU reference of
tests/montecarlo_util.py, the launch geometry (whole wavefronts per problem, padded lanes, more than one wavefront) against the
host twin, batch independence bit for bit, the resident variant behind a structured PTR run, and the refusals."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import audit_tracking_util as atu
import audit_util as au
import montecarlo_util as mu

pytestmark = pytest.mark.gpu

OK, BAD, TOO_LARGE, UNSUPPORTED = 0, 1, 6, 7
FIRST3 = au.AUDIT_MODELS[:3]
FLIGHT_CASES = [(n, N, 3, 4) for n in FIRST3 for N in (2, 5)] + [("starship", atu.STARSHIP["N"], 2, atu.STARSHIP["steps"])]
SEED = 2026


def _handle(pkg, name, N, cap, **kw):
    nsub = atu.STARSHIP["Nsub"] if name == "starship" else atu.NSUB
    kw.setdefault("Nsub", nsub)
    return pkg.PTR.create(pkg.PTR.Parameters(N=N, iter_max=3, **kw), pkg.TrajectoryProblem(name), batch_capacity=cap)


def _fly(pkg, pbm, xd, ud, p, pp, K, steps, viol_tol, D, seed, sig, moments=True, flights=True, B_=None, summary=True, stat=True):
    """K in the library's layout [B, N-1, nx, nu] or None"""
    b, N = xd.shape[0], xd.shape[1]
    out, st = np.full((b, au.W), 77.0), np.full((b, mu.SW), 79.0)
    mom, rec = np.full((b, N, 1 + 2 * pbm.nx + pbm.nu), 80.0), np.full((b, max(D, 1), au.W), 78.0)
    sec = ctypes.c_double(-1.0)
    rc = pkg._lib.lib().scp_audit_montecarlo_batch_host(pbm.handle, b if B_ is None else B_, au.vp(xd), au.vp(ud), au.vp(p) if pbm.np else None,
                                                        au.vp(pp), au.vp(K), steps, float(viol_tol), D, seed, au.vp(sig[0]), au.vp(sig[1]),
                                                        au.vp(sig[2]), au.vp(out) if summary else None, au.vp(st) if stat else None,
                                                        au.vp(mom) if moments else None, au.vp(rec) if flights else None, ctypes.byref(sec))
    return rc, out, st, mom, rec, sec.value


def _twin(pkg, name, N, case, Sx, Su, K, steps, viol_tol, D, seed, sig):
    """the host twin on ONE problem; K in the math layout [N-1, nu, nx]"""
    xd, ud, p, pp = case
    nx, nu = xd.shape[1], ud.shape[1]
    out, st, mom, rec = np.zeros(au.W), np.zeros(mu.SW), np.zeros((N, 1 + 2 * nx + nu)), np.zeros((D, au.W))
    rc = pkg._lib.lib().scp_model_audit_montecarlo_host(pkg.models.MODEL_IDS[name], au.vp(au.model_blob(pkg, name, N)), N, au.vp(xd), au.vp(ud),
                                                        au.vp(p) if p.size else None, au.vp(pp), au.vp(Sx), au.vp(Su), au.vp(atu.to_lib(K)), steps,
                                                        float(viol_tol), D, seed, au.vp(sig[0]), au.vp(sig[1]), au.vp(sig[2]), au.vp(out),
                                                        au.vp(st), au.vp(mom), au.vp(rec))
    assert rc == OK
    return out, st, mom, rec


def _gains(orc, name, N, s, cases):
    return [atu.riccati(*atu.oracle_dynamics(orc, name, N, s["Nsub"], *c[:3], s["Sx"]), *s["weights"])[0] for c in cases]


def _close(got, ref):
    """non-finite entries exactly, the others to RTOL max(1, |ref|)"""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    fin = np.isfinite(ref)
    return np.array_equal(got[~fin], ref[~fin], equal_nan=True) and (np.abs(got[fin] - ref[fin]) <= au.RTOL * np.maximum(1.0, np.abs(ref[fin]))).all()


@pytest.mark.parametrize("name,N,D,steps", FLIGHT_CASES)
def test_device_matches_reference(pkg, orc, name, N, D, steps):
    """B = 3 different problems (the Starship: its one configuration three times), the gains GIVEN (the reference's own)"""
    B = 3
    s = atu.setup(orc, name, N)
    cases, xd, ud, p, pp = atu.batch(orc, name, N, B)
    pbm = _handle(pkg, name, N, B)
    Sx, Su, sig = pbm.scale.Sx, pbm.scale.Su, mu.sigmas(s)
    Ks = _gains(orc, name, N, s, cases)
    refs = [mu.references(orc, name, N, steps, D, SEED, case=cases[b], K=Ks[b], Sx=Sx, Su=Su, key=("gpu", b if name != "starship" else 0))
            for b in range(B)]
    tol = au.choose_viol_tol([r for rb, _ in refs for r in rb])
    rc, out, st, mom, rec, sec = _fly(pkg, pbm, xd, ud, p, pp, atu.to_lib(np.stack(Ks)), steps, tol, D, SEED, sig)
    assert rc == OK and sec > 0.0
    for b in range(B):
        for d in range(D):
            refs[b][0][d].check_tracking(rec[b, d], tol, "%s b=%d d=%d" % (name, b, d + 1))
        mu.check_moments(mom[b], refs[b][1], "%s b=%d" % (name, b))
        mu.check_stat(st[b], refs[b][1], Sx, D, "%s b=%d" % (name, b))
        want = atu.fold(rec[b])
        want[13] = 4.0
        assert out[b].tobytes() == want.tobytes()
    pbm.close()


def test_geometry_against_the_host_twin(pkg, orc):
    """D = 2 (62 padded lanes), 64 (a full wavefront), 65 and 130 (a second and a third wavefront, partly filled): flights, moments
    and stat to RTOL against the host twin; a flight depends on d only"""
    name, N, steps, B = "rocket_landing", 5, 4, 2
    s = atu.setup(orc, name, N)
    cases, xd, ud, p, pp = atu.batch(orc, name, N, B)
    pbm = _handle(pkg, name, N, B)
    Sx, Su, sig = pbm.scale.Sx, pbm.scale.Su, mu.sigmas(s)
    Ks = _gains(orc, name, N, s, cases)
    recs = {}
    for D in (2, 64, 65, 130):
        rc, out, st, mom, rec, _ = _fly(pkg, pbm, xd, ud, p, pp, atu.to_lib(np.stack(Ks)), steps, 0.0, D, SEED, sig)
        assert rc == OK and (rec[:, :, 11] == 0.0).all() and (mom[:, :, 0] == D).all() and (st[:, 7] == D).all()
        recs[D] = rec
        for b in range(B):
            hout, hst, hmom, hrec = _twin(pkg, name, N, cases[b], Sx, Su, Ks[b], steps, 0.0, D, SEED, sig)
            assert _close(mom[b], hmom), (D, b)
            assert _close(st[b, [0, 3, 5]], hst[[0, 3, 5]]) and st[b, 7] == hst[7], (D, b, st[b], hst)
            assert _close(rec[b][:, [0, 2, 4, 6, 7, 8, 9, 12, 14]], hrec[:, [0, 2, 4, 6, 7, 8, 9, 12, 14]]), (D, b)
            want = atu.fold(rec[b])
            want[13] = 4.0
            assert out[b].tobytes() == want.tobytes() and out[b, 14] == D
    assert recs[130][:, :64].tobytes() == recs[64].tobytes() and recs[65][:, :64].tobytes() == recs[64].tobytes()
    assert recs[130][:, :65].tobytes() == recs[65].tobytes() and recs[64][:, :2].tobytes() == recs[2].tobytes()
    pbm.close()


def test_batch_independence(pkg, orc):
    """problem c alone (B = 1) and as entry 3 of B = 5: summary, stat, moments and flights byte for byte"""
    name, N, steps, D, B = "quadrotor", 5, 2, 70, 5
    s = atu.setup(orc, name, N)
    cases, xd, ud, p, pp = atu.batch(orc, name, N, B)
    pbm = _handle(pkg, name, N, B)
    sig = mu.sigmas(s)
    K = atu.to_lib(np.stack(_gains(orc, name, N, s, cases)))
    rc, out, st, mom, rec, _ = _fly(pkg, pbm, xd, ud, p, pp, K, steps, 0.0, D, SEED, sig)
    assert rc == OK and (rec[:, :, 11] == 0.0).all()
    one = [a[2:3].copy() for a in (xd, ud, p, pp, K)]
    rc, o1, s1, m1, r1, _ = _fly(pkg, pbm, *one, steps, 0.0, D, SEED, sig)
    assert rc == OK
    for a, b in ((o1, out), (s1, st), (m1, mom), (r1, rec)):
        assert a[0].tobytes() == b[2].tobytes()
    # the optional outputs change nothing; another seed does; the Python entry point gives the same bits
    rc, o2, s2, _, _, _ = _fly(pkg, pbm, xd, ud, p, pp, K, steps, 0.0, D, SEED, sig, moments=False, flights=False)
    assert rc == OK and o2.tobytes() == out.tobytes() and s2.tobytes() == st.tobytes()
    rc, o3, s3, m3, _, _ = _fly(pkg, pbm, xd, ud, p, pp, K, steps, 0.0, D, SEED + 2 ** 32, sig)
    assert rc == OK and (m3[:, :, 1] != mom[:, :, 1]).all()
    sol = SimpleNamespace(xd=xd, ud=ud, p=p)
    a = pkg.audit_montecarlo(sol, pbm, K.transpose(0, 1, 3, 2), steps, *sig, D, SEED, flights=True, pp=pp)
    assert a.raw.tobytes() == out.tobytes() and a.stat.tobytes() == st.tobytes() and a.moments.tobytes() == mom.tobytes()
    assert a.flights.tobytes() == rec.tobytes() and a.seconds > 0.0 and a.D == D and a.steps == steps and np.array_equal(a.n_min, st[:, 7])
    cov = pkg.audit_covariance(sol, pbm, K.transpose(0, 1, 3, 2), *sig, per_node=True, pp=pp)
    c = a.compare(cov)
    # D = 70: five standard errors of a sample sigma are 5 / sqrt(2 * 69) = 0.43; the bounds below lie outside 1 +- 0.43 on either side
    print("std / sig over the batch: min %.3f max %.3f" % (c.ratio_min.min(), c.ratio_max.max()))
    assert c.ratio.shape == (B, N, pbm.nx) and (c.ratio_min > 0.5).all() and (c.ratio_max < 2.0).all()
    sol.status = ["SCP_SOLVED"] * B
    sol.status[3] = "SCP_FAILED (NUMERICAL_ERROR)"
    a = pkg.audit_montecarlo(sol, pbm, K.transpose(0, 1, 3, 2), steps, *sig, D, SEED, pp=pp)
    assert list(a.skipped) == [False, False, False, True, False] and np.isnan(a.stat[3]).all() and np.isnan(a.moments[3]).all()
    pbm.close()


def _get(pkg, pbm, b):
    rc, r = pkg.generic.read_result(pbm, b, pkg._lib.lib().scp_ptr_get_host, pbm.handle, (b, 4), pkg._lib.HIST_WIDTH)
    assert rc == OK
    return r


def test_resident_equals_host_behind_a_structured_ptr_run(pkg):
    name, n, b, D, steps = "rocket_landing", 8, 4, 66, 3
    traj = pkg.TrajectoryProblem(name)
    rng = np.random.default_rng(3)
    npp = traj.mdl.nominal_pp().size
    pp = np.ascontiguousarray(np.stack([traj.mdl.nominal_pp() * (1 + 0.03 * rng.uniform(-1, 1, npp)) for _ in range(b)]))

    def run(iters, **kw):
        pbm = pkg.PTR.create(pkg.PTR.Parameters(N=n, Nsub=5, **kw), traj, batch_capacity=b)
        assert pkg.PTR.upload(pbm, pp) == b
        for _ in range(iters):
            pkg.PTR.iterate(pbm)
        return pbm

    pbm = run(10, iter_max=15)
    sig = (0.01 * pbm.scale.Sx, 0.01 * pbm.scale.Su, 0.002 * pbm.scale.Sx)
    r0 = _get(pkg, pbm, b)
    g = pkg.lqr_gains_resident(pbm)
    a = pkg.audit_montecarlo_resident(pbm, None, steps, *sig, D, SEED, flights=True)
    assert len(a) == b and a.D == D and a.seconds > 0.0
    r1 = _get(pkg, pbm, b)
    for k in ("xd", "ud", "p", "status", "iterations", "cost", "feas", "defect", "hist"):
        assert np.array_equal(getattr(r0, k), getattr(r1, k), equal_nan=True), k
    ok = r0.status == 0
    print("solved %d of %d" % (ok.sum(), b))
    assert ok.any()
    # a further iteration of the run is what it would have been without the calls
    twin = run(10, iter_max=15)
    for h in (pbm, twin):
        pkg.PTR.iterate(h)
    r2, t2 = _get(pkg, pbm, b), _get(pkg, twin, b)
    for k in ("xd", "ud", "p", "status", "cost"):
        assert np.array_equal(getattr(r2, k), getattr(t2, k), equal_nan=True), k
    twin.close()
    # the host variant on what get_host returned, with the gains of the resident call
    h = pkg.audit_montecarlo(SimpleNamespace(xd=r0.xd, ud=r0.ud, p=r0.p), pbm, g, steps, *sig, D, SEED, flights=True, pp=pp)
    for x, y in ((h.raw, a.raw), (h.stat, a.stat), (h.moments, a.moments), (h.flights, a.flights)):
        assert x[ok].tobytes() == y[ok].tobytes()
        assert np.isnan(y[~ok]).all()
    assert list(a.skipped) == list(~ok) and (a.n[ok] == D).all()
    pbm.close()
    # failed instances (the subproblem solver stops at its iteration limit of 2): NaN in everything of theirs
    pbm = run(1, iter_max=2, solver_opts={"maxit": 2})
    bad = _get(pkg, pbm, b).status != 0
    print("failed %d of %d" % (bad.sum(), b))
    assert bad.any()
    pkg.lqr_gains_resident(pbm)
    a = pkg.audit_montecarlo_resident(pbm, None, steps, *sig, D, SEED, flights=True)
    for y in (a.raw, a.stat, a.moments, a.flights):
        assert np.isnan(y[bad]).all()
    assert list(a.skipped) == list(bad)
    pbm.close()


def test_refusals(pkg, orc):
    L = pkg._lib.lib()
    one, st8, N = np.zeros((1, 16)), np.zeros((1, 8)), 5
    for name, kw, text in (("quadrotor", dict(disc_method=pkg.IMPULSE), b"FOH handles only"), ("freeflyer", {}, b"node parameters"),
                           ("oscillator", {}, b"node parameters")):
        traj = pkg.TrajectoryProblem(name)
        pbm = pkg.PTR.create(pkg.PTR.Parameters(N=N, Nsub=3, iter_max=1, **kw), traj, batch_capacity=2)
        xd, ud, p, pp = np.zeros((1, N, pbm.nx)), np.zeros((1, N, pbm.nu)), np.zeros((1, 64 * N)), np.zeros((1, 64))      # refused unread
        K = np.zeros((1, N - 1, pbm.nx, pbm.nu))
        sig = (np.ones(pbm.nx), np.ones(pbm.nu), np.ones(pbm.nx))
        assert _fly(pkg, pbm, xd, ud, p, pp, K, 2, 0.0, 2, 0, sig)[0] == UNSUPPORTED and text in L.scp_last_error(pbm.handle)
        assert L.scp_audit_montecarlo_resident(pbm.handle, au.vp(K), 2, 0.0, 2, 0, au.vp(sig[0]), au.vp(sig[1]), au.vp(sig[2]), au.vp(one),
                                               au.vp(st8), None, None, None) == UNSUPPORTED
        with pytest.raises(pkg._lib.ScpError) as e:
            pkg.audit_montecarlo(SimpleNamespace(xd=xd, ud=ud, p=p), pbm, K.transpose(0, 1, 3, 2), 2, *sig, 2, pp=pp)
        assert e.value.code == UNSUPPORTED
        pbm.close()
    name = "quadrotor"
    s = atu.setup(orc, name, N)
    xd, ud, p, pp = (np.ascontiguousarray(a[None]) for a in s["case"])
    K = atu.to_lib(s["K"][None])
    sig = mu.sigmas(s)
    pbm = _handle(pkg, name, N, cap=2)
    assert L.scp_audit_montecarlo_resident(pbm.handle, au.vp(K), 2, 0.0, 2, 0, au.vp(sig[0]), au.vp(sig[1]), au.vp(sig[2]), au.vp(one), au.vp(st8),
                                           None, None, None) == BAD and b"no run" in L.scp_last_error(pbm.handle)      # RUN_NONE
    with pytest.raises(pkg._lib.ScpError):
        pkg.audit_montecarlo_resident(pbm, None, 2, *sig, 2)
    # no resident gains; then gains made for another B
    assert _fly(pkg, pbm, xd, ud, p, pp, None, 2, 0.0, 2, 0, sig)[0] == BAD and b"holds no gains" in L.scp_last_error(pbm.handle)
    rep = lambda a, n: np.repeat(a, n, 0)      # noqa: E731
    pkg.lqr_gains(SimpleNamespace(xd=rep(xd, 2), ud=rep(ud, 2), p=rep(p, 2)), pbm, *s["weights"])
    assert _fly(pkg, pbm, xd, ud, p, pp, None, 2, 0.0, 2, 0, sig)[0] == BAD and b"made for B = 2" in L.scp_last_error(pbm.handle)
    rc, o2, _, _, r2, _ = _fly(pkg, pbm, rep(xd, 2), rep(ud, 2), rep(p, 2), rep(pp, 2), None, 2, 0.0, 2, 0, sig)
    assert rc == OK and o2[0].tobytes() == o2[1].tobytes() and o2[0, 13] == 4.0 and o2[0, 14] == 2.0 and (r2[:, :, 11] == 0.0).all()
    assert _fly(pkg, pbm, xd, ud, p, pp, K, 2, 0.0, 1, 0, sig)[0] == BAD                                # D < 2
    assert _fly(pkg, pbm, xd, ud, p, pp, K, 0, 0.0, 2, 0, sig)[0] == BAD and b"steps" in L.scp_last_error(pbm.handle)
    assert _fly(pkg, pbm, xd, ud, p, pp, K, 2, 0.0, 2, 0, sig, summary=False)[0] == BAD
    assert _fly(pkg, pbm, xd, ud, p, pp, K, 2, 0.0, 2, 0, sig, stat=False)[0] == BAD
    for i in range(3):
        for spoil in (lambda a: -a, lambda a: a * np.nan, lambda a: None):
            bad = list(sig)
            bad[i] = spoil(bad[i])
            assert _fly(pkg, pbm, xd, ud, p, pp, K, 2, 0.0, 2, 0, bad)[0] == BAD, i
    assert _fly(pkg, pbm, rep(xd, 3), rep(ud, 3), rep(p, 3), rep(pp, 3), rep(K, 3), 2, 0.0, 2, 0, sig)[0] == TOO_LARGE
    assert b"batch_capacity" in L.scp_last_error(pbm.handle)
    # the handle stays usable
    rc, o, st, mom, r, _ = _fly(pkg, pbm, xd, ud, p, pp, K, 1, 0.0, 2, 0, sig)
    assert rc == OK and o[0, 11] == 0.0 and o[0, 13] == 4.0 and st[0, 7] == 2.0 and (mom[0, :, 0] == 2.0).all()
    pbm.close()
