"""The closed-loop covariance audit on the host (scp_covariance_host and scp_model_covariance_rows_host: the bodies the device
kernels run, csrc/cov_kernel.hpp) against the numpy reference of tests/covariance_util.py: the chain fed the oracle's dynamics,
gains and rows, the row pre-pass against the oracle's closures, a closed form on the double integrator, failure reporting, and the
error codes and exported names that need no device."""
import ctypes

import numpy as np
import pytest

import audit_tracking_util as atu
import audit_util as au
import covariance_util as cu

BAD, UNKNOWN, UNSUPPORTED = 1, 2, 7
FIRST3 = au.AUDIT_MODELS[:3]
CASES = [(n, N) for n in FIRST3 for N in (2, 5, 9)] + [("starship", 9)]


def _chain(pkg, dyn, K, nrow, T, Hf, Sx, Su, sig0, sigu, sigw, nsig=cu.NSIG, dims=None, N=None, want=(True, True), summary=True):
    """K[N-1, nu, nx] in the math layout, T the row table [N, nrow, nx+1], Hf[ntc, nx]"""
    A, Bm, Bp = dyn
    nx, nu = (A.shape[1], Bm.shape[1]) if dims is None else dims
    N = A.shape[0] + 1 if N is None else N
    out, sig, nodes = np.full(cu.W, 91.0), np.full((max(N, 1), nx), 92.0), np.full((max(N, 1), cu.NW), 93.0)
    Hf = np.asarray(Hf, float)
    nrow = None if nrow is None else np.ascontiguousarray(nrow, np.int32)
    rc = pkg._lib.lib().scp_covariance_host(nx, nu, N, au.vp(A), au.vp(Bm), au.vp(Bp), au.vp(None if K is None else atu.to_lib(K)),
                                            None if nrow is None else nrow.ctypes.data, au.vp(T),
                                            Hf.shape[0], au.vp(np.ascontiguousarray(Hf.T)), au.vp(Sx), au.vp(Su), au.vp(sig0), au.vp(sigu),
                                            au.vp(sigw), float(nsig), au.vp(out) if summary else None, au.vp(sig) if want[0] else None,
                                            au.vp(nodes) if want[1] else None)
    return rc, out, sig, nodes


def _rows(pkg, name, N, case, K, want=True):
    xd, ud, p, pp = case
    nx = xd.shape[1]
    info = pkg._lib.ScpModelInfo()
    assert pkg._lib.lib().scp_model_query(pkg.models.MODEL_IDS[name], ctypes.byref(info)) == 0
    nrow = (info.ns, info.nl, info.nsoc)
    T, Hf = np.full((N, sum(nrow), nx + 1), 94.0), np.full((nx, info.ntc), 95.0)
    rc = pkg._lib.lib().scp_model_covariance_rows_host(pkg.models.MODEL_IDS[name], au.vp(au.model_blob(pkg, name, N)), N, au.vp(xd), au.vp(ud),
                                                       au.vp(p) if p.size else None, au.vp(pp), au.vp(None if K is None else atu.to_lib(K)),
                                                       au.vp(T) if want else None, au.vp(Hf))
    return rc, nrow, T, Hf.T


@pytest.mark.parametrize("name,N", CASES)
def test_chain_matches_reference(pkg, orc, name, N):
    """scp_covariance_host fed the oracle's A, B-, B+, the reference K and the reference rows (N = 2: the single step)"""
    s, rows, Hf, ref = cu.reference(orc, name, N)
    nrow, T = cu.table(rows, s["Sx"].size)
    rc, out, sig, nodes = _chain(pkg, s["dyn"], s["K"], nrow, T, Hf, s["Sx"], s["Su"], *cu.inputs(s))
    assert rc == 0
    made, skipped = ref.check(out, sig, nodes, "%s N=%d" % (name, N))
    print("index comparisons", made, "skipped", skipped)
    assert skipped <= cu.SKIP_CAP * (made + skipped)
    # the optional outputs change nothing
    rc, only, _, _ = _chain(pkg, s["dyn"], s["K"], nrow, T, Hf, s["Sx"], s["Su"], *cu.inputs(s), want=(False, False))
    assert rc == 0 and only.tobytes() == out.tobytes()


@pytest.mark.parametrize("name,N", CASES)
def test_rows_match_the_oracle_closures(pkg, orc, name, N):
    """scp_model_covariance_rows_host against the rows built from the oracle's closures: value and gradient per family, rows sorted
    by value within a family at each node; Hf"""
    s, rows, Hf, _ = cu.reference(orc, name, N)
    rc, nrow, T, Hg = _rows(pkg, name, N, s["case"], s["K"])
    assert rc == 0
    nx = s["Sx"].size
    assert [rows[0][f][0].size for f in range(3)] == list(nrow)
    for k in range(N):
        r0 = 0
        for f in range(3):
            v, g = rows[k][f]
            got = T[k, r0:r0 + nrow[f]]
            r0 += nrow[f]
            if not v.size:
                continue
            o_ref, o_got = np.argsort(v, kind="stable"), np.argsort(got[:, nx], kind="stable")
            tol_v = au.RTOL * max(1.0, np.abs(v).max())
            tol_g = au.RTOL * max(1.0, np.abs(g).max())
            assert np.abs(got[o_got, nx] - v[o_ref]).max() <= tol_v, (name, k, f, got[o_got, nx], v[o_ref])
            # rows of equal value may come in either order: compare each with the nearest reference row of its value
            for i in o_got:
                same = np.abs(v - got[i, nx]) <= tol_v
                assert min(np.abs(g[j] - got[i, :nx]).max() for j in np.nonzero(same)[0]) <= tol_g, (name, k, f, i)
    assert np.abs(Hg - Hf).max() <= au.RTOL


def test_closed_form_on_the_double_integrator(pkg, orc):
    """K = 0, sigu = sigw = 0: Sigma_k = Phi(k,1) diag(sig0^2) Phi(k,1)' from the product of the A_k; rows with a zero gradient
    (the input rows) have margins +-Inf by the sign of their value"""
    name, N = "double_integrator", 9
    s, _, Hf, _ = cu.reference(orc, name, N)
    K0 = np.zeros_like(s["K"])
    rc, nrow, T, Hg = _rows(pkg, name, N, s["case"], K0)
    assert rc == 0
    sig0 = cu.inputs(s)[0]
    zu, zx = np.zeros(1), np.zeros(2)
    rc, out, sig, nodes = _chain(pkg, s["dyn"], K0, nrow, T, Hg, s["Sx"], s["Su"], sig0, zu, zx)
    assert rc == 0 and out[0] == 0.0
    Phi, want = np.eye(2), []
    for k in range(N):
        S = Phi @ np.diag(sig0 ** 2) @ Phi.T
        want.append(np.sqrt(np.diag(S)))
        if k < N - 1:
            Phi = s["dyn"][0][k].T @ Phi
    want = np.array(want)
    assert np.abs(sig - want).max() <= au.RTOL * max(1.0, np.abs(want).max())
    assert out[4] == 0.0 and (nodes[:-1, 1] == 0.0).all() and np.isnan(nodes[-1, 1])
    assert abs(out[13] - ((want[-1] / s["Sx"]) ** 2).sum()) <= au.RTOL * max(1.0, out[13])
    # the rows: every row whose gradient over the state is zero has an infinite margin of the sign of -v
    zero = ~T[:, :, :2].any(axis=2)
    assert zero.any()
    nx = 2
    r0 = 0
    for f in range(3):
        blk, zf = T[:, r0:r0 + nrow[f]], zero[:, r0:r0 + nrow[f]]
        r0 += nrow[f]
        if nrow[f] and zf.all():
            v = blk[:, :, nx]
            want_min = np.where((v > 0.0).any(axis=1), -np.inf, np.inf)
            assert np.array_equal(nodes[:, 2 + f], want_min), (f, nodes[:, 2 + f], want_min)
            assert out[6 + 2 * f] == want_min.min()
    # a second statement of the same rule with rows made by hand: v = -1, 0, +2 with g = 0
    Th = np.zeros((N, 3, 3)); Th[:, 0, 2], Th[:, 2, 2] = -1.0, 2.0
    rc, o2, _, n2 = _chain(pkg, s["dyn"], K0, (1, 1, 1), Th, Hg, s["Sx"], s["Su"], sig0, zu, zx)
    assert rc == 0 and o2[6] == np.inf and o2[7] == 0.0 and o2[8] == np.inf and o2[9] == 0.0 and o2[10] == -np.inf and o2[11] == 1.0
    assert o2[14] == N and (n2[:, 4] == -np.inf).all()


def test_failures_are_reported(pkg, orc):
    """a NaN in A at an interior interval: [0] = 1 and the rest NaN, no abort; the next call is not touched"""
    name, N = "rocket_landing", 5
    s, rows, Hf, ref = cu.reference(orc, name, N)
    nrow, T = cu.table(rows, s["Sx"].size)
    for arr, val in ((0, np.nan), (1, np.inf)):
        dyn = [a.copy() for a in s["dyn"]]
        dyn[arr][2, 1, 3] = val
        rc, out, sig, nodes = _chain(pkg, dyn, s["K"], nrow, T, Hf, s["Sx"], s["Su"], *cu.inputs(s))
        assert rc == 0 and out[0] == 1.0 and np.isnan(out[1:]).all(), (arr, val, out)
    Kbad = s["K"].copy(); Kbad[0, 0, 0] = np.nan
    rc, out, _, _ = _chain(pkg, s["dyn"], Kbad, nrow, T, Hf, s["Sx"], s["Su"], *cu.inputs(s))
    assert rc == 0 and out[0] == 1.0 and np.isnan(out[1:]).all()
    Tbad = T.copy(); Tbad[3, 1, -1] = np.nan
    rc, out, _, _ = _chain(pkg, s["dyn"], s["K"], nrow, Tbad, Hf, s["Sx"], s["Su"], *cu.inputs(s))
    assert rc == 0 and out[0] == 1.0 and np.isnan(out[1:]).all()
    rc, out, sig, nodes = _chain(pkg, s["dyn"], s["K"], nrow, T, Hf, s["Sx"], s["Su"], *cu.inputs(s))
    assert rc == 0 and out[0] == 0.0
    ref.check(out, sig, nodes, "after the failures")


def test_error_codes(pkg, orc):
    name, N = "double_integrator", 5
    s, rows, Hf, _ = cu.reference(orc, name, N)
    nrow, T = cu.table(rows, 2)
    sig0, sigu, sigw = cu.inputs(s)
    base = (s["dyn"], s["K"], nrow, T, Hf, s["Sx"], s["Su"])
    assert _chain(pkg, *base, sig0, sigu, sigw)[0] == 0
    for bad in ((-sig0, sigu, sigw), (sig0, -sigu, sigw), (sig0, sigu, -sigw), (sig0 * np.nan, sigu, sigw), (sig0, sigu * np.inf, sigw),
                (sig0, sigu, sigw * np.nan), (None, sigu, sigw), (sig0, None, sigw), (sig0, sigu, None)):
        assert _chain(pkg, *base, *bad)[0] == BAD
    for nsig in (0.0, -1.0, np.nan, np.inf):
        assert _chain(pkg, *base, sig0, sigu, sigw, nsig=nsig)[0] == BAD
    assert _chain(pkg, *base, 0.0 * sig0, 0.0 * sigu, 0.0 * sigw)[0] == 0            # zero dispersions are allowed
    assert _chain(pkg, *base, sig0, sigu, sigw, summary=False)[0] == BAD
    assert _chain(pkg, *base, sig0, sigu, sigw, N=1)[0] == BAD
    assert _chain(pkg, s["dyn"], None, nrow, T, Hf, s["Sx"], s["Su"], sig0, sigu, sigw)[0] == BAD
    assert _chain(pkg, s["dyn"], s["K"], nrow, None, Hf, s["Sx"], s["Su"], sig0, sigu, sigw)[0] == BAD      # rows are announced
    assert _chain(pkg, s["dyn"], s["K"], (0, 0, 0), None, Hf, s["Sx"], s["Su"], sig0, sigu, sigw)[0] == 0   # no rows at all
    assert _chain(pkg, s["dyn"], s["K"], (1, -1, 0), T, Hf, s["Sx"], s["Su"], sig0, sigu, sigw)[0] == BAD
    assert _chain(pkg, s["dyn"], s["K"], None, T, Hf, s["Sx"], s["Su"], sig0, sigu, sigw)[0] == BAD
    big = np.ones((4, 13 * 13))
    for dims in ((13, 6), (2, 2), (6, 3), (3, 1)):                                   # the free-flyer's and other pairs
        assert _chain(pkg, (big, big, big), big[:, :78].reshape(4, 6, 13), (0, 0, 0), None, np.zeros((0, 13)), np.ones(13), np.ones(13),
                      np.ones(13), np.ones(13), np.ones(13), dims=dims, N=5)[0] == UNSUPPORTED
    # the pre-pass
    K = s["K"]
    assert _rows(pkg, name, N, s["case"], K)[0] == 0
    assert _rows(pkg, name, N, s["case"], None)[0] == BAD                            # the host twin has no resident gains
    assert _rows(pkg, name, N, s["case"], K, want=False)[0] == BAD
    q = atu.setup(orc, "quadrotor", 5)
    xd, ud, p, pp = q["case"]
    assert _rows(pkg, "quadrotor", 5, (xd, ud, np.zeros(0), pp), q["K"])[0] == BAD   # the model has a p
    L = pkg._lib.lib()
    ff = np.ones(16 * 16 * N)
    assert L.scp_model_covariance_rows_host(42, au.vp(ff), N, au.vp(ff), au.vp(ff), au.vp(ff), au.vp(ff), au.vp(ff), au.vp(ff), au.vp(ff)) == UNKNOWN
    for other in ("freeflyer", "oscillator"):                                        # refused whatever the arrays hold
        assert L.scp_model_covariance_rows_host(pkg.models.MODEL_IDS[other], au.vp(np.ones(64)), N, au.vp(ff), au.vp(ff), au.vp(ff), au.vp(ff),
                                                au.vp(ff), au.vp(ff), au.vp(ff)) == UNSUPPORTED


def test_names_are_exported(pkg):
    for nm in ("audit_covariance", "audit_covariance_resident", "CovarianceAuditBatch"):
        assert callable(getattr(pkg, nm))
    for nm in ("scp_audit_covariance_batch_host", "scp_audit_covariance_resident", "scp_model_covariance_rows_host", "scp_covariance_host"):
        assert nm in pkg._lib.EXPORTS and hasattr(pkg._lib.lib(), nm)
    raw = np.arange(32.0).reshape(2, 16)
    raw[1] = np.nan; raw[0, 0] = 0.0
    sig, nodes = np.arange(2 * 3 * 4.0).reshape(2, 3, 4), np.arange(2 * 3 * 8.0).reshape(2, 3, 8)
    a = pkg.CovarianceAuditBatch(raw, nsig=3.0, sig=sig, nodes=nodes)
    assert len(a) == 2 and list(a.failed) == [False, False] and list(a.skipped) == [False, True] and a.nsig == 3.0
    assert a.sigma_max[0] == 1.0 and a.sigma_node[0] == 2.0 and a.sigma_state[0] == 3.0 and a.effort[0] == 4.0 and a.effort_node[0] == 5.0
    assert a.margin_s[0] == 6.0 and a.margin_s_node[0] == 7.0 and a.margin_lin[0] == 8.0 and a.margin_lin_node[0] == 9.0
    assert a.margin_soc[0] == 10.0 and a.margin_soc_node[0] == 11.0 and a.terminal_sigma[0] == 12.0 and a.trace_final[0] == 13.0
    assert a.n_below[0] == 14.0 and a.sig.shape == (2, 3, 4) and a.nodes.shape == (2, 3, 8) and a.seconds == 0.0
    b = pkg.CovarianceAuditBatch(raw, 2.0)
    assert b.sig is None and b.nodes is None
    raw[0, 0] = 1.0
    assert list(pkg.CovarianceAuditBatch(raw, 2.0).failed) == [True, False]
