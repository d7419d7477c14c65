"""The LQR gains and the closed-loop tracking audit on the device (-m gpu): scp_lqr_gains_batch_host against the reference chain
(oracle discretize!, numpy Riccati) and against the host twin on the device's own discretisation, the launch geometry of both
kernels bit for bit, scp_audit_tracking_batch_host against the CPU reference of tests/audit_tracking_util.py (four models, truth
models), the two sources of the gains, the resident variants behind a structured PTR run, and the refusals."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import audit_dispersed_util as adu
import audit_tracking_util as atu
import audit_util as au

pytestmark = pytest.mark.gpu

B = 5
OK, BAD, TOO_LARGE, UNSUPPORTED = 0, 1, 6, 7
SHARED = 1
FIRST3 = au.AUDIT_MODELS[:3]


def _handle(pkg, name, N, cap=B, **kw):
    nsub = atu.STARSHIP["Nsub"] if name == "starship" else atu.NSUB
    kw.setdefault("Nsub", nsub)
    return pkg.PTR.create(pkg.PTR.Parameters(N=N, iter_max=3, **kw), pkg.TrajectoryProblem(name), batch_capacity=cap)


def _gains(pkg, pbm, xd, ud, p, w, want_K=True, B_=None):
    b, N = xd.shape[0], xd.shape[1]
    K, info = np.full((b, N - 1, pbm.nx, pbm.nu), 66.0), np.full((b, 4), 67.0)
    sec = ctypes.c_double(-1.0)
    rc = pkg._lib.lib().scp_lqr_gains_batch_host(pbm.handle, b if B_ is None else B_, au.vp(xd), au.vp(ud), au.vp(p) if pbm.np else None,
                                                 au.vp(w[0]), au.vp(w[1]), au.vp(w[2]), au.vp(K) if want_K else None, au.vp(info),
                                                 ctypes.byref(sec))
    return rc, K, info, sec.value


def _fly(pkg, pbm, xd, ud, p, pp, K, steps, viol_tol, d, dx0, gain, bias, flags=0, par_true=None, flights=True, B_=None):
    """K in the library's layout [B, N-1, nx, nu] or None"""
    b = xd.shape[0]
    out, rec = np.full((b, au.W), 77.0), np.full((b, max(d, 1), au.W), 78.0)
    sec = ctypes.c_double(-1.0)
    rc = pkg._lib.lib().scp_audit_tracking_batch_host(pbm.handle, b if B_ is None else B_, au.vp(xd), au.vp(ud), au.vp(p) if pbm.np else None,
                                                      au.vp(pp), au.vp(K), steps, float(viol_tol), d, au.vp(dx0), au.vp(gain), au.vp(bias),
                                                      flags, au.vp(par_true), au.vp(out), au.vp(rec) if flights else None, ctypes.byref(sec))
    return rc, out, rec, sec.value


@pytest.mark.parametrize("name,N", [(n, N) for n in FIRST3 for N in (2, 9)] + [("starship", 9)])
def test_device_gains(pkg, orc, name, N):
    """the chain discretize! + Riccati on the device against oracle discretize! + numpy Riccati, within 10 x what a 1e-10 relative
    change of A, B-, B+ (the parity discretize! is held to) does to the reference's K; the device's Riccati alone against the host
    twin fed the device's own discretisation"""
    s = atu.setup(orc, name, N)
    cases, xd, ud, p, pp = atu.batch(orc, name, N, B)
    pbm = _handle(pkg, name, N)
    rc, K, info, sec = _gains(pkg, pbm, xd, ud, p, s["weights"])
    assert rc == OK and sec > 0.0 and (info[:, 0] == 0.0).all() and (info[:, 3] == 0.0).all()
    rng = np.random.default_rng(5)
    for b in range(B):
        dyn = atu.oracle_dynamics(orc, name, N, s["Nsub"], *cases[b][:3], s["Sx"])
        Kref, iref = atu.riccati(*dyn, *s["weights"])
        Kpert, ipert = atu.riccati(*(a * (1.0 + 1e-10 * rng.uniform(-1, 1, a.shape)) for a in dyn), *s["weights"])
        floor = au.RTOL * max(1.0, np.abs(Kref).max())
        tol = max(10.0 * np.abs(Kpert - Kref).max(), floor)
        err = np.abs(np.swapaxes(K[b], -1, -2) - Kref).max()
        print("%s N=%d b=%d max|K| %.3e sensitivity %.3e tol %.3e err %.3e" % (name, N, b, np.abs(Kref).max(), np.abs(Kpert - Kref).max(), tol, err))
        assert err <= tol, (b, err, tol)
        tol_tr = max(10.0 * abs(ipert[2] - iref[2]), au.RTOL * abs(iref[2]))      # the trace of P by the same rule
        assert abs(info[b, 1] - iref[1]) <= tol and abs(info[b, 2] - iref[2]) <= tol_tr, (b, info[b], iref, tol, tol_tr)
    # the device Riccati alone
    A, Bm, Bp = (np.zeros((B, N - 1, c, pbm.nx)) for c in (pbm.nx, pbm.nu, pbm.nu))
    assert pkg._lib.lib().scp_discretize_batch_host(pbm.handle, B, au.vp(xd), au.vp(ud), au.vp(p) if pbm.np else None, au.vp(A), au.vp(Bm),
                                                    au.vp(Bp), None, None, None, None, None, None) == OK
    for b in range(B):
        Kh, ih = np.zeros((N - 1, pbm.nx, pbm.nu)), np.zeros(4)
        assert pkg._lib.lib().scp_lqr_gains_host(pbm.nx, pbm.nu, N, au.vp(A[b]), au.vp(Bm[b]), au.vp(Bp[b]), *(au.vp(a) for a in s["weights"]),
                                                 au.vp(Kh), au.vp(ih)) == OK
        tol = au.RTOL * max(1.0, np.abs(Kh).max())
        assert np.abs(K[b] - Kh).max() <= tol, (b, np.abs(K[b] - Kh).max(), tol)
        assert ih[0] == 0.0 and abs(info[b, 1] - ih[1]) <= tol and abs(info[b, 2] - ih[2]) <= au.RTOL * abs(ih[2])
    # the Python entry point: the same bits, K[B, N-1, nu, nx]
    g = pkg.lqr_gains(SimpleNamespace(xd=xd, ud=ud, p=p), pbm, *s["weights"])
    assert g.K.shape == (B, N - 1, pbm.nu, pbm.nx) and g.raw.tobytes() == K.tobytes() and g.info.tobytes() == info.tobytes()
    assert not g.failed.any() and np.array_equal(g.k_max, info[:, 1]) and np.array_equal(g.trace_p, info[:, 2]) and g.seconds > 0.0
    pbm.close()


@pytest.mark.parametrize("name", ["double_integrator", "rocket_landing"])
def test_gain_geometry(pkg, orc, name):
    """a problem's K and info: alone, in a batch of 5, in the reversed batch, and in a batch of 67 (two wavefronts of one problem
    each, or five packed wavefronts of 16 double integrators) -- bit for bit; a failing neighbour changes nothing"""
    N = 5
    s = atu.setup(orc, name, N)
    _, xd, ud, p, _ = atu.batch(orc, name, N, B)
    pbm = _handle(pkg, name, N, cap=67)
    w = s["weights"]
    rc, K5, i5, _ = _gains(pkg, pbm, xd, ud, p, w)
    assert rc == OK and (i5[:, 0] == 0.0).all()
    for b in range(B):
        rc, K1, i1, _ = _gains(pkg, pbm, xd[b:b + 1].copy(), ud[b:b + 1].copy(), p[b:b + 1].copy(), w)
        assert rc == OK and K1[0].tobytes() == K5[b].tobytes() and i1[0].tobytes() == i5[b].tobytes(), b
    rc, Kr, ir, _ = _gains(pkg, pbm, xd[::-1].copy(), ud[::-1].copy(), p[::-1].copy(), w)
    assert rc == OK and Kr[::-1].tobytes() == K5.tobytes() and ir[::-1].tobytes() == i5.tobytes()
    idx = np.arange(67) % B
    x67, u67, p67 = xd[idx].copy(), ud[idx].copy(), p[idx].copy()
    fails = name != "double_integrator"                     # (the double integrator has no parameter to spoil)
    if fails:
        p67[33] = np.nan                                    # one problem that fails: its time dilation enters every A, B-, B+
    rc, K67, i67, _ = _gains(pkg, pbm, x67, u67, p67, w)
    assert rc == OK
    if fails:
        assert i67[33, 0] == 1.0 and np.isnan(K67[33]).all() and np.isnan(i67[33, 1:3]).all()
    keep = np.arange(67) != (33 if fails else -1)
    assert K67[keep].tobytes() == K5[idx][keep].tobytes() and i67[keep].tobytes() == i5[idx][keep].tobytes()
    pbm.close()


def test_flight_geometry(pkg, orc):
    """B = 5, D = 13: 65 threads, the flights of the last problem straddle two wavefronts; every flight equals the same flight
    alone (B = 1, D = 1) bit for bit, and SCP_DISP_SHARED equals the tiled arrays"""
    name, N, d, steps = "quadrotor", 5, 13, 2
    s = atu.setup(orc, name, N)
    _, xd, ud, p, pp = atu.batch(orc, name, N, B)
    pbm = _handle(pkg, name, N)
    rc, K, info, _ = _gains(pkg, pbm, xd, ud, p, s["weights"])
    assert rc == OK
    rng = np.random.default_rng(7)
    dx0 = 0.01 * pbm.scale.Sx * rng.standard_normal((B, d, 6))
    gain = 1.0 + 0.02 * rng.standard_normal((B, d, 4))
    bias = 0.01 * s["Su"] * rng.standard_normal((B, d, 4))
    rc, out, rec, sec = _fly(pkg, pbm, xd, ud, p, pp, K, steps, 0.0, d, dx0, gain, bias)
    assert rc == OK and sec > 0.0 and (rec[:, :, 11] == 0.0).all() and (rec[:, :, 12] > 0.0).all()
    for i in range(B):
        one = [a[i:i + 1].copy() for a in (xd, ud, p, pp, K)]
        for j in range(d):
            rc, o1, r1, _ = _fly(pkg, pbm, *one, steps, 0.0, 1, dx0[i, j].copy(), gain[i, j].copy(), bias[i, j].copy())
            assert rc == OK and r1[0, 0].tobytes() == rec[i, j].tobytes(), (i, j)
            assert o1[0].tobytes() == atu.fold(rec[i, j:j + 1]).tobytes()
        assert out[i].tobytes() == atu.fold(rec[i]).tobytes(), i
    rc, only, _, _ = _fly(pkg, pbm, xd, ud, p, pp, K, steps, 0.0, d, dx0, gain, bias, flights=False)
    assert rc == OK and only.tobytes() == out.tobytes()
    tile = lambda a: np.ascontiguousarray(np.tile(a[None], (B, 1, 1)))      # noqa: E731
    rc, out_t, rec_t, _ = _fly(pkg, pbm, xd, ud, p, pp, K, steps, 0.0, d, tile(dx0[2]), tile(gain[2]), tile(bias[2]))
    assert rc == OK
    rc, out_s, rec_s, _ = _fly(pkg, pbm, xd, ud, p, pp, K, steps, 0.0, d, dx0[2].copy(), gain[2].copy(), bias[2].copy(), flags=SHARED)
    assert rc == OK and out_s.tobytes() == out_t.tobytes() and rec_s.tobytes() == rec_t.tobytes()
    # the Python entry point: gains as a GainBatch, as an array, and failed problems masked
    sol = SimpleNamespace(xd=xd, ud=ud, p=p)
    g = pkg.lqr_gains(sol, pbm, *s["weights"])
    for gains in (g, g.K, None):
        a = pkg.audit_tracking(sol, pbm, gains, steps, dx0[2], gain[2], bias[2], shared=True, pp=pp, flights=True)
        assert a.raw.tobytes() == out_t.tobytes() and a.flights.tobytes() == rec_t.tobytes() and a.steps == steps and a.res == steps * (N - 1) + 1
    assert np.array_equal(a.effort, rec_t[:, :, 12]) and np.array_equal(a.track_node, rec_t[:, :, 15])
    sol.status = ["SCP_SOLVED"] * B
    sol.status[3] = "SCP_FAILED (NUMERICAL_ERROR)"
    a = pkg.audit_tracking(sol, pbm, g, steps, dx0, gain, bias, pp=pp, flights=True)
    assert list(a.skipped) == [False, False, False, True, False] and np.isnan(a.flights[3]).all()
    assert np.delete(a.raw, 3, 0).tobytes() == np.delete(out, 3, 0).tobytes()
    assert pkg.audit_tracking(sol, pbm, g, pp=pp).steps == 2 * atu.NSUB      # ceil((2 Nsub (N-1) - 1) / (N-1))
    pbm.close()


@pytest.mark.parametrize("name,truth", [(n, False) for n in au.AUDIT_MODELS] + [("quadrotor", True), ("rocket_landing", True)])
def test_device_flights_match_reference(pkg, orc, name, truth):
    """B = 5 problems, D = 4 flights, the gains GIVEN (the reference's own, per problem); a truth model on the quadrotor and the rocket"""
    N, steps = (atu.STARSHIP["N"], atu.STARSHIP["steps"]) if name == "starship" else (5, 4)
    s = atu.setup(orc, name, N)
    cases, xd, ud, p, pp = atu.batch(orc, name, N, B)
    pbm = _handle(pkg, name, N)
    Sx, Su = pbm.scale.Sx, pbm.scale.Su
    Ks = [atu.riccati(*atu.oracle_dynamics(orc, name, N, s["Nsub"], *c[:3], s["Sx"]), *s["weights"])[0] for c in cases]
    blob, tr = adu.truth(pkg, orc, name, N) if truth else (None, None)
    refs = [atu.references(orc, name, N, steps, K=Ks[b], Sx=Sx, Su=Su, truth=tr, case=cases[b], key=("gpu", b if name != "starship" else 0))
            for b in range(B)]
    tol = au.choose_viol_tol([r for rb in refs for r in rb])
    disp = tuple(np.ascontiguousarray(np.tile(a[None], (B, 1, 1))) for a in s["disp"])
    rc, out, rec, sec = _fly(pkg, pbm, xd, ud, p, pp, atu.to_lib(np.stack(Ks)), steps, tol, 4, *disp, par_true=blob)
    assert rc == OK and sec > 0.0
    for b in range(B):
        for d in range(4):
            refs[b][d].check_tracking(rec[b, d], tol, "%s truth=%s b=%d d=%d" % (name, truth, b, d + 1))
        assert out[b].tobytes() == atu.fold(rec[b]).tobytes()
    pbm.close()


def test_gain_sources(pkg, orc):
    """K = NULL after scp_lqr_gains_batch_host gives the bits of passing the returned K; without gains, or with gains made for
    another B, it is refused; gains that are passed leave the resident ones alone"""
    name, N, steps = "rocket_landing", 5, 2
    s = atu.setup(orc, name, N)
    _, xd, ud, p, pp = atu.batch(orc, name, N, B)
    pbm = _handle(pkg, name, N)
    L = pkg._lib.lib()
    disp = tuple(np.ascontiguousarray(np.tile(a[None], (B, 1, 1))) for a in s["disp"])
    assert _fly(pkg, pbm, xd, ud, p, pp, None, steps, 0.0, 4, *disp)[0] == BAD and b"holds no gains" in L.scp_last_error(pbm.handle)
    rc, K, info, _ = _gains(pkg, pbm, xd, ud, p, s["weights"])
    assert rc == OK
    rc, out, rec, _ = _fly(pkg, pbm, xd, ud, p, pp, K, steps, 0.0, 4, *disp)
    assert rc == OK and (rec[:, :, 11] == 0.0).all()
    rc, out0, rec0, _ = _fly(pkg, pbm, xd, ud, p, pp, None, steps, 0.0, 4, *disp)
    assert rc == OK and out0.tobytes() == out.tobytes() and rec0.tobytes() == rec.tobytes()
    # other gains, passed: another flight; the resident ones are still there afterwards
    rc, outz, recz, _ = _fly(pkg, pbm, xd, ud, p, pp, np.zeros_like(K), steps, 0.0, 4, *disp)
    assert rc == OK and (recz[:, :, 12] == 0.0).all() and (recz[:, 1:, 8] != rec[:, 1:, 8]).all()
    rc, out1, rec1, _ = _fly(pkg, pbm, xd, ud, p, pp, None, steps, 0.0, 4, *disp)
    assert rc == OK and out1.tobytes() == out.tobytes() and rec1.tobytes() == rec.tobytes()
    # gains kept on the device only (K = NULL in the gains call), and gains for another B
    rc, _, info2, _ = _gains(pkg, pbm, xd, ud, p, s["weights"], want_K=False)
    assert rc == OK and info2.tobytes() == info.tobytes()
    rc, out2, rec2, _ = _fly(pkg, pbm, xd, ud, p, pp, None, steps, 0.0, 4, *disp)
    assert rc == OK and rec2.tobytes() == rec.tobytes()
    rc, _, _, _ = _gains(pkg, pbm, xd[:3].copy(), ud[:3].copy(), p[:3].copy(), s["weights"])
    assert rc == OK
    assert _fly(pkg, pbm, xd, ud, p, pp, None, steps, 0.0, 4, *disp)[0] == BAD and b"made for B = 3" in L.scp_last_error(pbm.handle)
    rc, out3, rec3, _ = _fly(pkg, pbm, xd[:3].copy(), ud[:3].copy(), p[:3].copy(), pp[:3].copy(), None, steps, 0.0, 4, *(a[:3].copy() for a in disp))
    assert rc == OK and rec3.tobytes() == rec[:3].tobytes()
    pbm.close()


def _get(pkg, pbm, b):
    rc, r = pkg.generic.read_result(pbm, b, pkg._lib.lib().scp_ptr_get_host, pbm.handle, (b, 4), pkg._lib.HIST_WIDTH)
    assert rc == OK
    return r


def test_resident_equals_host_behind_a_structured_ptr_run(pkg):
    name, n, b, d, steps = "rocket_landing", 8, 4, 3, 3
    traj = pkg.TrajectoryProblem(name)
    rng = np.random.default_rng(3)
    npp = traj.mdl.nominal_pp().size
    pp = np.ascontiguousarray(np.stack([traj.mdl.nominal_pp() * (1 + 0.03 * rng.uniform(-1, 1, npp)) for _ in range(b)]))
    L = pkg._lib.lib()

    def run(iters, **kw):
        pbm = pkg.PTR.create(pkg.PTR.Parameters(N=n, Nsub=5, **kw), traj, batch_capacity=b)
        assert pkg.PTR.upload(pbm, pp) == b
        for _ in range(iters):
            pkg.PTR.iterate(pbm)
        return pbm

    pbm = run(10, iter_max=15)
    w = atu.weights(pbm.scale.Sx, pbm.scale.Su)
    dx0 = 0.01 * pbm.scale.Sx * rng.standard_normal((b, d, pbm.nx))
    gain = 1.0 + 0.02 * rng.standard_normal((b, d, pbm.nu))
    bias = 0.01 * pbm.scale.Su * rng.standard_normal((b, d, pbm.nu))
    r0 = _get(pkg, pbm, b)
    K, info = np.full((b, n - 1, pbm.nx, pbm.nu), 44.0), np.full((b, 4), 45.0)
    sec = ctypes.c_double(-1.0)
    assert L.scp_lqr_gains_resident(pbm.handle, au.vp(w[0]), au.vp(w[1]), au.vp(w[2]), au.vp(K), au.vp(info), ctypes.byref(sec)) == OK and sec.value > 0.0
    out, rec = np.full((b, au.W), 55.0), np.full((b, d, au.W), 56.0)
    assert L.scp_audit_tracking_resident(pbm.handle, None, steps, 0.0, d, au.vp(dx0), au.vp(gain), au.vp(bias), 0, None, au.vp(out), au.vp(rec),
                                         ctypes.byref(sec)) == OK and sec.value > 0.0
    g = pkg.lqr_gains_resident(pbm)                         # Bryson's rule from the handle's scaling: the same weights
    assert g.raw.tobytes() == K.tobytes() and g.info.tobytes() == info.tobytes()
    a = pkg.audit_tracking_resident(pbm, None, steps, dx0, gain, bias, flights=True)
    assert len(a) == b and a.D == d and a.raw.tobytes() == out.tobytes() and a.flights.tobytes() == rec.tobytes()
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
    # the host variants on what get_host returned
    rc, Kh, ih, _ = _gains(pkg, pbm, r0.xd, r0.ud, r0.p, w)
    assert rc == OK and Kh[ok].tobytes() == K[ok].tobytes() and ih[ok].tobytes() == info[ok].tobytes()
    rc, oh, rh, _ = _fly(pkg, pbm, r0.xd, r0.ud, r0.p, pp, Kh, steps, 0.0, d, dx0, gain, bias)
    assert rc == OK and oh[ok].tobytes() == out[ok].tobytes() and rh[ok].tobytes() == rec[ok].tobytes()
    assert np.isnan(K[~ok]).all() and np.isnan(info[~ok]).all() and np.isnan(out[~ok]).all() and np.isnan(rec[~ok]).all()
    assert list(a.skipped) == list(~ok) and list(g.skipped) == list(~ok)
    pbm.close()
    # failed instances (the subproblem solver stops at its iteration limit of 2): NaN in everything of theirs
    pbm = run(1, iter_max=2, solver_opts={"maxit": 2})
    bad = _get(pkg, pbm, b).status != 0
    print("failed %d of %d" % (bad.sum(), b))
    assert bad.any()
    g = pkg.lqr_gains_resident(pbm)
    a = pkg.audit_tracking_resident(pbm, None, steps, dx0, gain, bias, flights=True)
    assert np.isnan(g.raw[bad]).all() and np.isnan(g.info[bad]).all() and np.isnan(a.raw[bad]).all() and np.isnan(a.flights[bad]).all()
    assert list(a.skipped) == list(bad) and list(g.skipped) == list(bad)
    pbm.close()


def test_refusals(pkg, orc):
    L = pkg._lib.lib()
    one, i4, N = np.zeros((1, 1, 16)), np.zeros((1, 4)), 5
    for name, kw, text in (("quadrotor", dict(disc_method=pkg.IMPULSE), b"FOH handles only"), ("freeflyer", {}, b"node parameters"),
                           ("oscillator", {}, b"node parameters")):
        traj = pkg.TrajectoryProblem(name)
        pbm = pkg.PTR.create(pkg.PTR.Parameters(N=N, Nsub=3, iter_max=1, **kw), traj, batch_capacity=2)
        xd, ud, p, pp = np.zeros((1, N, pbm.nx)), np.zeros((1, N, pbm.nu)), np.zeros((1, 64 * N)), np.zeros((1, 64))      # refused unread
        K = np.zeros((1, N - 1, pbm.nx, pbm.nu))
        w = (np.ones(pbm.nx), np.ones(pbm.nu), np.ones(pbm.nx))
        assert _gains(pkg, pbm, xd, ud, p, w)[0] == UNSUPPORTED and text in L.scp_last_error(pbm.handle)
        assert L.scp_lqr_gains_resident(pbm.handle, au.vp(w[0]), au.vp(w[1]), au.vp(w[2]), None, au.vp(i4), None) == UNSUPPORTED
        assert _fly(pkg, pbm, xd, ud, p, pp, K, 2, 0.0, 1, None, None, None)[0] == UNSUPPORTED and text in L.scp_last_error(pbm.handle)
        assert L.scp_audit_tracking_resident(pbm.handle, au.vp(K), 2, 0.0, 1, None, None, None, 0, None, au.vp(one), None, None) == UNSUPPORTED
        with pytest.raises(pkg._lib.ScpError) as e:
            pkg.audit_tracking(SimpleNamespace(xd=xd, ud=ud, p=p), pbm, K.transpose(0, 1, 3, 2), 2, pp=pp)
        assert e.value.code == UNSUPPORTED
        pbm.close()
    name = "quadrotor"
    s = atu.setup(orc, name, N)
    xd, ud, p, pp = (np.ascontiguousarray(a[None]) for a in s["case"])
    K = atu.to_lib(s["K"][None])
    pbm = _handle(pkg, name, N, cap=2)
    w = s["weights"]
    assert L.scp_lqr_gains_resident(pbm.handle, au.vp(w[0]), au.vp(w[1]), au.vp(w[2]), None, au.vp(i4), None) == BAD      # RUN_NONE
    assert b"no run" in L.scp_last_error(pbm.handle)
    assert L.scp_audit_tracking_resident(pbm.handle, au.vp(K), 2, 0.0, 1, None, None, None, 0, None, au.vp(one), None, None) == BAD
    assert b"no run" in L.scp_last_error(pbm.handle)
    for bad in ((-w[0], w[1], w[2]), (w[0], 0.0 * w[1], w[2]), (w[0], w[1], np.nan * w[2]), (None, w[1], w[2])):
        assert _gains(pkg, pbm, xd, ud, p, bad)[0] == BAD
    assert L.scp_lqr_gains_batch_host(pbm.handle, 1, au.vp(xd), au.vp(ud), au.vp(p), au.vp(w[0]), au.vp(w[1]), au.vp(w[2]), None, None, None) == BAD
    assert _fly(pkg, pbm, xd, ud, p, pp, K, 0, 0.0, 1, None, None, None)[0] == BAD and b"steps" in L.scp_last_error(pbm.handle)
    assert _fly(pkg, pbm, xd, ud, p, pp, K, 2, 0.0, 0, None, None, None)[0] == BAD                      # D = 0
    assert _fly(pkg, pbm, xd, ud, p, pp, K, 2, 0.0, 1, None, None, None, flags=2)[0] == BAD             # an unknown flag bit
    args = (au.vp(xd), au.vp(ud))
    tail = (au.vp(K), 2, 0.0, 1, None, None, None, 0, None)
    assert L.scp_audit_tracking_batch_host(pbm.handle, 1, *args, au.vp(p), au.vp(pp), *tail, None, None, None) == BAD      # NULL summary
    assert L.scp_audit_tracking_batch_host(pbm.handle, 1, *args, None, au.vp(pp), *tail, au.vp(one), None, None) == BAD
    assert L.scp_audit_tracking_batch_host(pbm.handle, 1, *args, au.vp(p), None, *tail, au.vp(one), None, None) == BAD
    rep = lambda a: np.repeat(a, 3, 0)      # noqa: E731
    assert _fly(pkg, pbm, rep(xd), rep(ud), rep(p), rep(pp), rep(K), 2, 0.0, 1, None, None, None)[0] == TOO_LARGE
    assert _gains(pkg, pbm, rep(xd), rep(ud), rep(p), w)[0] == TOO_LARGE and b"batch_capacity" in L.scp_last_error(pbm.handle)
    # the handle stays usable; steps = 1 is the smallest grid
    rc, o, r, _ = _fly(pkg, pbm, xd, ud, p, pp, K, 1, 0.0, 2, None, None, None)
    assert rc == OK and o[0, 11] == 0.0 and o[0, 13] == 3.0 and o[0, 14] == 2.0 and r[0, 0].tobytes() == r[0, 1].tobytes()
    assert r[0, 0, 12] >= 0.0 and 1.0 <= r[0, 0, 13] <= N - 1 and 1.0 <= r[0, 0, 15] <= N
    pbm.close()
