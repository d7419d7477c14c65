"""The closed-loop covariance audit on the device (-m gpu): scp_audit_covariance_batch_host against the numpy reference of
tests/covariance_util.py (four models, gains passed and resident, with and without the optional outputs), the launch geometry of
the chain bit for bit, the resident variant behind a structured PTR run and behind an SCvx loop, the refusals, and a sanity link to
the sampling audit scp_audit_tracking_batch_host."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import audit_tracking_util as atu
import audit_util as au
import covariance_util as cu

pytestmark = pytest.mark.gpu

B = 3
OK, BAD, TOO_LARGE, UNSUPPORTED = 0, 1, 6, 7


def _handle(pkg, name, N, cap=B, **kw):
    nsub = atu.STARSHIP["Nsub"] if name == "starship" else atu.NSUB
    kw.setdefault("Nsub", nsub)
    return pkg.PTR.create(pkg.PTR.Parameters(N=N, iter_max=3, **kw), pkg.TrajectoryProblem(name), batch_capacity=cap)


def _gains(pkg, pbm, xd, ud, p, w):
    b, N = xd.shape[0], xd.shape[1]
    K, info = np.full((b, N - 1, pbm.nx, pbm.nu), 66.0), np.full((b, 4), 67.0)
    rc = pkg._lib.lib().scp_lqr_gains_batch_host(pbm.handle, b, au.vp(xd), au.vp(ud), au.vp(p) if pbm.np else None, au.vp(w[0]), au.vp(w[1]),
                                                 au.vp(w[2]), au.vp(K), au.vp(info), None)
    assert rc == OK and (info[:, 0] == 0.0).all()
    return K


def _cov(pkg, pbm, xd, ud, p, pp, K, sig, nsig=cu.NSIG, want=(True, True), B_=None, summary=True):
    """K in the library's layout [B, N-1, nx, nu] or None; sig = (sig0, sigu, sigw)"""
    b, N = xd.shape[0], xd.shape[1]
    out, s, nodes = np.full((b, cu.W), 81.0), np.full((b, N, pbm.nx), 82.0), np.full((b, N, cu.NW), 83.0)
    sec = ctypes.c_double(-1.0)
    rc = pkg._lib.lib().scp_audit_covariance_batch_host(pbm.handle, b if B_ is None else B_, au.vp(xd), au.vp(ud), au.vp(p) if pbm.np else None,
                                                        au.vp(pp), au.vp(K), au.vp(sig[0]), au.vp(sig[1]), au.vp(sig[2]), float(nsig),
                                                        au.vp(out) if summary else None, au.vp(s) if want[0] else None,
                                                        au.vp(nodes) if want[1] else None, ctypes.byref(sec))
    return rc, out, s, nodes, sec.value


def _resident(pkg, pbm, K, sig, cap, N, nsig=cu.NSIG, want=(True, True)):
    out, s, nodes = np.full((cap, cu.W), 84.0), np.full((cap, N, pbm.nx), 85.0), np.full((cap, N, cu.NW), 86.0)
    sec = ctypes.c_double(-1.0)
    rc = pkg._lib.lib().scp_audit_covariance_resident(pbm.handle, au.vp(K), au.vp(sig[0]), au.vp(sig[1]), au.vp(sig[2]), float(nsig), au.vp(out),
                                                      au.vp(s) if want[0] else None, au.vp(nodes) if want[1] else None, ctypes.byref(sec))
    return rc, out, s, nodes, sec.value


def _inputs(pbm):
    return 0.01 * pbm.scale.Sx, 0.01 * pbm.scale.Su, 1e-3 * pbm.scale.Sx


@pytest.mark.parametrize("name,N", [(n, N) for n in au.AUDIT_MODELS[:3] for N in (2, 5)] + [("starship", atu.STARSHIP["N"])])
def test_device_matches_reference(pkg, orc, name, N):
    """B = 3 problems against the numpy reference over the oracle's discretize!, the gains GIVEN (the reference's own, per problem);
    the summary bit for bit whether or not the optional outputs are asked for; the gains resident = the same gains passed"""
    s = atu.setup(orc, name, N)
    cases, xd, ud, p, pp = atu.batch(orc, name, N, B)
    pbm = _handle(pkg, name, N)
    Sx, Su = pbm.scale.Sx, pbm.scale.Su
    sig = _inputs(pbm)
    Ks, refs = [], []
    for b in range(B):
        dyn = atu.oracle_dynamics(orc, name, N, s["Nsub"], *cases[b][:3], s["Sx"])
        K = atu.riccati(*dyn, *s["weights"])[0]
        rows = cu.oracle_rows(name, N, *cases[b][:3], K)
        Hf = np.asarray(au.oracle_model(name, N).Hf(cases[b][0][-1], cases[b][2], cases[b][3]), float).reshape(-1, pbm.nx)
        Ks.append(K)
        refs.append(cu.Reference(dyn, K, rows, Hf, Sx, Su, *sig))
    Kl = atu.to_lib(np.stack(Ks))
    rc, out, sg, nodes, sec = _cov(pkg, pbm, xd, ud, p, pp, Kl, sig)
    assert rc == OK and sec > 0.0
    made = skipped = 0
    for b in range(B):
        m, k = refs[b].check(out[b], sg[b], nodes[b], "%s N=%d b=%d" % (name, N, b))
        made, skipped = made + m, skipped + k
    print("index comparisons", made, "skipped", skipped)
    assert skipped <= cu.SKIP_CAP * (made + skipped)
    for want in ((False, False), (True, False), (False, True)):
        rc, only, s1, n1, _ = _cov(pkg, pbm, xd, ud, p, pp, Kl, sig, want=want)
        assert rc == OK and only.tobytes() == out.tobytes()
        assert (s1.tobytes() == sg.tobytes()) if want[0] else (s1 == 82.0).all()
        assert (n1.tobytes() == nodes.tobytes()) if want[1] else (n1 == 83.0).all()
    # the gains the device made, resident and passed: the same bits, and the Python entry point
    Kd = _gains(pkg, pbm, xd, ud, p, s["weights"])
    rc, o_res, s_res, n_res, _ = _cov(pkg, pbm, xd, ud, p, pp, None, sig)
    assert rc == OK and (o_res[:, 0] == 0.0).all()
    rc, o_pas, s_pas, n_pas, _ = _cov(pkg, pbm, xd, ud, p, pp, Kd, sig)
    assert rc == OK and o_pas.tobytes() == o_res.tobytes() and s_pas.tobytes() == s_res.tobytes() and n_pas.tobytes() == n_res.tobytes()
    sol = SimpleNamespace(xd=xd, ud=ud, p=p)
    for gains in (None, np.swapaxes(Kd, -1, -2)):
        a = pkg.audit_covariance(sol, pbm, gains, *sig, nsig=cu.NSIG, per_node=True, pp=pp)
        assert a.raw.tobytes() == o_res.tobytes() and a.sig.tobytes() == s_res.tobytes() and a.nodes.tobytes() == n_res.tobytes() and a.seconds > 0.0
    a = pkg.audit_covariance(sol, pbm, None, sig[0], nsig=cu.NSIG, pp=pp)          # sigu, sigw default to zeros
    rc, o_zero, _, _, _ = _cov(pkg, pbm, xd, ud, p, pp, None, (sig[0], 0.0 * sig[1], 0.0 * sig[2]), want=(False, False))
    assert rc == OK and a.raw.tobytes() == o_zero.tobytes() and a.sig is None and a.nodes is None
    sol.status = ["SCP_SOLVED", "SCP_FAILED (NUMERICAL_ERROR)", "SCP_SOLVED"]
    a = pkg.audit_covariance(sol, pbm, None, *sig, per_node=True, pp=pp)
    assert list(a.skipped) == [False, True, False] and np.isnan(a.sig[1]).all() and np.isnan(a.nodes[1]).all()
    assert np.delete(a.raw, 1, 0).tobytes() == np.delete(o_res, 1, 0).tobytes()
    pbm.close()


@pytest.mark.parametrize("name,sizes", [("double_integrator", (1, 15, 16, 17, 33)), ("quadrotor", (1, 2, 5))])
def test_geometry(pkg, orc, name, sizes):
    """a problem's record, sig and nodes: alone, at every position of batches of one lane-group, a full wavefront of 16 double
    integrators, a partial second block and more than two blocks (the quadrotor: one problem per wavefront), and in the reversed
    batch -- bit for bit"""
    N, nb = 5, 5
    s = atu.setup(orc, name, N)
    _, xd, ud, p, pp = atu.batch(orc, name, N, nb)
    pbm = _handle(pkg, name, N, cap=max(sizes))
    sig = _inputs(pbm)
    K = _gains(pkg, pbm, xd, ud, p, s["weights"])
    alone = []
    for b in range(nb):
        rc, o, sg, nd, _ = _cov(pkg, pbm, *(a[b:b + 1].copy() for a in (xd, ud, p, pp, K)), sig)
        assert rc == OK and o[0, 0] == 0.0
        alone.append((o[0].tobytes(), sg[0].tobytes(), nd[0].tobytes()))
    assert len(set(alone)) == nb                             # five different problems
    for size in sizes:
        idx = (np.arange(size) * 3 + 1) % nb                # every problem at many positions
        for order in (idx, idx[::-1]):
            rc, o, sg, nd, _ = _cov(pkg, pbm, *(a[order].copy() for a in (xd, ud, p, pp, K)), sig)
            assert rc == OK
            for i, b in enumerate(order):
                assert (o[i].tobytes(), sg[i].tobytes(), nd[i].tobytes()) == alone[b], (size, i, b)
    pbm.close()


def _get(pkg, pbm, b):
    rc, r = pkg.generic.read_result(pbm, b, pkg._lib.lib().scp_ptr_get_host, pbm.handle, (b, 4), pkg._lib.HIST_WIDTH)
    assert rc == OK
    return r


def test_resident_equals_host_behind_a_structured_ptr_run(pkg):
    name, n, b = "rocket_landing", 8, 4
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
    sig = _inputs(pbm)
    r0 = _get(pkg, pbm, b)
    g = pkg.lqr_gains_resident(pbm)
    a = pkg.audit_covariance_resident(pbm, None, *sig, per_node=True)
    rc, out, sg, nd, sec = _resident(pkg, pbm, None, sig, b, n)
    assert rc == OK and sec > 0.0 and a.raw.tobytes() == out.tobytes() and a.sig.tobytes() == sg.tobytes() and a.nodes.tobytes() == nd.tobytes()
    rc, only, _, _, _ = _resident(pkg, pbm, None, sig, b, n, want=(False, False))
    assert rc == OK and only.tobytes() == out.tobytes()
    r1 = _get(pkg, pbm, b)
    for k in ("xd", "ud", "p", "status", "iterations", "cost", "feas", "defect", "hist"):
        assert np.asarray(getattr(r0, k)).tobytes() == np.asarray(getattr(r1, k)).tobytes(), k
    ok = r0.status == 0
    print("solved %d of %d" % (ok.sum(), b))
    assert ok.any() and (out[ok, 0] == 0.0).all()
    assert np.isnan(out[~ok]).all() and np.isnan(sg[~ok]).all() and np.isnan(nd[~ok]).all() and list(a.skipped) == list(~ok)
    # the host variant on what get_host returned, with the gains the resident call made
    h = pkg.audit_covariance(SimpleNamespace(xd=r0.xd, ud=r0.ud, p=r0.p), pbm, g, *sig, per_node=True, pp=pp)
    assert h.raw[ok].tobytes() == out[ok].tobytes() and h.sig[ok].tobytes() == sg[ok].tobytes() and h.nodes[ok].tobytes() == nd[ok].tobytes()
    pbm.close()
    # failed instances (iter_max = 3, the subproblem solver stops at its iteration limit of 2): NaN in everything of theirs
    pbm = run(1, iter_max=3, solver_opts={"maxit": 2})
    r0 = _get(pkg, pbm, b)
    bad = r0.status != 0
    print("unsolved %d of %d" % (bad.sum(), b))
    assert bad.any()
    pkg.lqr_gains_resident(pbm)
    a = pkg.audit_covariance_resident(pbm, None, *sig, per_node=True)
    assert np.isnan(a.raw[bad]).all() and np.isnan(a.sig[bad]).all() and np.isnan(a.nodes[bad]).all() and list(a.skipped) == list(bad)
    r1 = _get(pkg, pbm, b)
    for k in ("xd", "ud", "p", "status", "iterations", "cost", "feas", "defect", "hist"):
        assert np.asarray(getattr(r0, k)).tobytes() == np.asarray(getattr(r1, k)).tobytes(), k
    pbm.close()


def test_resident_behind_an_scvx_loop(pkg):
    """the loop's own solution and the SUBPROBLEM handle's pp are what the resident call reads"""
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
    na = ctypes.c_int(-1)
    for _ in range(2):
        assert L.scp_scvx_iterate(pbm.sub._h, ctypes.byref(na)) == OK

    def get():
        rc, r = pkg.generic.read_result(pbm, b, L.scp_scvx_get_host, pbm.sub._h, (2, b), pkg._lib.HIST_WIDTH)
        assert rc == OK
        return r

    r0 = get()
    ok = r0.status == 0
    assert ok.any()
    sig = _inputs(pbm)
    w = atu.weights(pbm.scale.Sx, pbm.scale.Su)
    K, info = np.full((8, n - 1, pbm.nx, pbm.nu), 44.0), np.full((8, 4), 45.0)
    assert L.scp_lqr_gains_resident(pbm.handle, au.vp(w[0]), au.vp(w[1]), au.vp(w[2]), au.vp(K), au.vp(info), None) == OK
    rc, out, sg, nd, sec = _resident(pkg, pbm, None, sig, 8, n)
    assert rc == OK and sec > 0.0 and (out[:b][ok, 0] == 0.0).all() and np.isnan(out[:b][~ok]).all()
    r1 = get()
    for k in ("xd", "ud", "p", "status", "cost"):
        assert np.asarray(getattr(r0, k)).tobytes() == np.asarray(getattr(r1, k)).tobytes(), k
    rc, oh, sh, nh, _ = _cov(pkg, pbm, r0.xd, r0.ud, r0.p, pp, K[:b].copy(), sig)
    assert rc == OK and oh[ok].tobytes() == out[:b][ok].tobytes() and sh[ok].tobytes() == sg[:b][ok].tobytes() and nh[ok].tobytes() == nd[:b][ok].tobytes()
    # and in the reversed batch
    rc, other, _, _, _ = _cov(pkg, pbm, r0.xd[::-1].copy(), r0.ud[::-1].copy(), r0.p[::-1].copy(), pp[::-1].copy(), K[:b][::-1].copy(), sig)
    assert rc == OK and other[::-1][ok].tobytes() == oh[ok].tobytes()
    pbm.close()


def test_refusals(pkg, orc):
    L = pkg._lib.lib()
    N = 5
    for name, kw, text in (("quadrotor", dict(disc_method=pkg.IMPULSE), b"FOH handles only"), ("freeflyer", {}, b"node parameters")):
        traj = pkg.TrajectoryProblem(name)
        pbm = pkg.PTR.create(pkg.PTR.Parameters(N=N, Nsub=3, iter_max=1, **kw), traj, batch_capacity=2)
        xd, ud, p, pp = np.zeros((1, N, pbm.nx)), np.zeros((1, N, pbm.nu)), np.zeros((1, 64 * N)), np.zeros((1, 64))      # refused unread
        K = np.zeros((1, N - 1, pbm.nx, pbm.nu))
        sig = (np.ones(pbm.nx), np.ones(pbm.nu), np.ones(pbm.nx))
        assert _cov(pkg, pbm, xd, ud, p, pp, K, sig)[0] == UNSUPPORTED and text in L.scp_last_error(pbm.handle)
        assert _resident(pkg, pbm, K, sig, 2, N)[0] == UNSUPPORTED and text in L.scp_last_error(pbm.handle)
        with pytest.raises(pkg._lib.ScpError) as e:
            pkg.audit_covariance(SimpleNamespace(xd=xd, ud=ud, p=p), pbm, K.transpose(0, 1, 3, 2), *sig, pp=pp)
        assert e.value.code == UNSUPPORTED and text.decode() in str(e.value)
        if name == "freeflyer":                              # the model-level twin refuses the model, whatever the arrays hold
            ff = np.ones(16 * 16 * N)
            assert L.scp_model_covariance_rows_host(pkg.models.MODEL_IDS[name], au.vp(np.ones(64)), N, au.vp(ff), au.vp(ff), au.vp(ff), au.vp(ff),
                                                    au.vp(ff), au.vp(ff), au.vp(ff)) == UNSUPPORTED
        pbm.close()
    name = "quadrotor"
    s = atu.setup(orc, name, N)
    xd, ud, p, pp = (np.ascontiguousarray(a[None]) for a in s["case"])
    K = atu.to_lib(s["K"][None])
    pbm = _handle(pkg, name, N, cap=2)
    sig = _inputs(pbm)
    assert _cov(pkg, pbm, xd, ud, p, pp, None, sig)[0] == BAD and b"holds no gains" in L.scp_last_error(pbm.handle)
    assert _resident(pkg, pbm, K, sig, 2, N)[0] == BAD and b"no run" in L.scp_last_error(pbm.handle)            # RUN_NONE
    with pytest.raises(pkg._lib.ScpError):
        pkg.audit_covariance_resident(pbm, None, *sig)
    for bad in ((-sig[0], sig[1], sig[2]), (sig[0], -sig[1], sig[2]), (sig[0], sig[1], np.nan * sig[2]), (None, sig[1], sig[2]),
                (sig[0], None, sig[2]), (sig[0], sig[1], None)):
        assert _cov(pkg, pbm, xd, ud, p, pp, K, bad)[0] == BAD and b"sig0" in L.scp_last_error(pbm.handle)
    for nsig in (0.0, -2.0, np.nan, np.inf):
        assert _cov(pkg, pbm, xd, ud, p, pp, K, sig, nsig=nsig)[0] == BAD
    assert _cov(pkg, pbm, xd, ud, p, pp, K, sig, summary=False)[0] == BAD
    assert L.scp_audit_covariance_batch_host(pbm.handle, 1, au.vp(xd), au.vp(ud), None, au.vp(pp), au.vp(K), au.vp(sig[0]), au.vp(sig[1]),
                                             au.vp(sig[2]), 3.0, au.vp(np.zeros(16)), None, None, None) == BAD       # the model has a p
    rep = lambda a: np.repeat(a, 3, 0)      # noqa: E731
    assert _cov(pkg, pbm, rep(xd), rep(ud), rep(p), rep(pp), rep(K), sig)[0] == TOO_LARGE and b"batch_capacity" in L.scp_last_error(pbm.handle)
    # gains made for another B
    _gains(pkg, pbm, rep(xd)[:2].copy(), rep(ud)[:2].copy(), rep(p)[:2].copy(), s["weights"])
    assert _cov(pkg, pbm, xd, ud, p, pp, None, sig)[0] == BAD and b"made for B = 2" in L.scp_last_error(pbm.handle)
    # the handle stays usable
    rc, out, _, _, _ = _cov(pkg, pbm, xd, ud, p, pp, K, sig)
    assert rc == OK and out[0, 0] == 0.0 and out[0, 15] == 0.0
    pbm.close()


def test_sanity_link_to_the_tracking_audit(pkg, orc):
    """not a gate on statistics: on the double integrator (linear dynamics, so the flight IS the linear propagation) with
    sigu = sigw = 0, one closed-loop flight from dx0 = eps e_i at steps = Nsub tracks within (1 + 1e-3) of
    max_k |A_cl(k-1) ... A_cl(1) e_i eps|_inf / Sx, computed from the device's own discretisation and gains"""
    name, N = "double_integrator", 5
    s = atu.setup(orc, name, N)
    xd, ud, p, pp = (np.ascontiguousarray(a[None]) for a in s["case"])
    pbm = _handle(pkg, name, N, cap=1)
    Sx = pbm.scale.Sx
    K = _gains(pkg, pbm, xd, ud, p, s["weights"])
    A, Bm, Bp = (np.zeros((1, N - 1, c, pbm.nx)) for c in (pbm.nx, pbm.nu, pbm.nu))
    assert pkg._lib.lib().scp_discretize_batch_host(pbm.handle, 1, au.vp(xd), au.vp(ud), None, au.vp(A), au.vp(Bm), au.vp(Bp), None, None, None,
                                                    None, None, None) == OK
    eps = 0.01 * Sx
    dx0 = np.ascontiguousarray(np.diag(eps)[None])          # [1, D = nx, nx]
    a = pkg.audit_tracking(SimpleNamespace(xd=xd, ud=ud, p=p), pbm, np.swapaxes(K, -1, -2), steps=atu.NSUB, dx0=dx0, pp=pp, flights=True)
    for i in range(pbm.nx):
        e, bound = dx0[0, i].copy(), 0.0
        for k in range(N):
            bound = max(bound, np.abs(e / Sx).max())
            if k < N - 1:
                Phi, Gam = A[0, k].T, (Bm[0, k] + Bp[0, k]).T
                e = (Phi - Gam @ K[0, k].T) @ e
        print("state", i, "flight", a.track_err[0, i], "linear", bound)
        assert a.track_err[0, i] <= (1.0 + 1e-3) * bound
        # and the covariance of that single direction is its square: sigma from sig0 = eps e_i alone
        sig0 = np.zeros(pbm.nx); sig0[i] = eps[i]
        rc, out, sg, _, _ = _cov(pkg, pbm, xd, ud, p, pp, K, (sig0, np.zeros(pbm.nu), np.zeros(pbm.nx)))
        assert rc == OK and abs(out[0, 1] - bound) <= 1e-9 * max(1.0, bound)
    pbm.close()
