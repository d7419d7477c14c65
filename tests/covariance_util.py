"""CPU reference of the closed-loop covariance audit (include/scp_mi355x.h, scp_audit_covariance_*), shared by
tests/test_audit_covariance_cpu.py and tests/test_audit_covariance_gpu.py.  It takes nothing from the code under test: plain
matrix products over the oracle's `discretize!` (audit_tracking_util.oracle_dynamics), the numpy Riccati gains of
audit_tracking_util, and the rows of the closures of oracle/models.py (s / C / D, X / U without the parameter-only rows as in
audit_util._sample, Hf).

Cases: audit_tracking_util.setup (flown trajectories, Bryson gains, Sx, Su).  Inputs: sig0 = 0.01 Sx, sigu = 0.01 Su,
sigw = 1e-3 Sx, all strictly positive, so that every Sigma_k is positive definite and no row variance sits at roundoff: the
reference asserts that every row with a non-zero gradient has a variance above 1e-12 |g|^2 max diag Sigma (a row whose gradient
is exactly zero -- the rocket's terminal stand-in rows -- has the variance exactly 0 on both sides and a margin of +-Inf by sign).

Tolerance: audit_util.RTOL applied as in test_gain_parity: absolute error <= RTOL max(1, max |reference|) per quantity (a summary
field, the sig array, a column of the node records), +-Inf compared exactly.  A node or state index is compared only when the
reference's runner-up is separated from the winner by more than twice that tolerance; `check` returns how many index comparisons
were made and how many were skipped, and the tests cap the skipped share at 25 %."""
import numpy as np

import audit_tracking_util as atu
import audit_util as au
from oracle.models import linrange

W, NW = 16, 8      # SCP_COV_WIDTH, SCP_COV_NODE_WIDTH
NSIG = 3.0
SKIP_CAP = 0.25


def inputs(s):
    """(sig0, sigu, sigw) of a setup() dict"""
    return 0.01 * s["Sx"], 0.01 * s["Su"], 1e-3 * s["Sx"]


def oracle_rows(name, N, xd, ud, p, K):
    """per node (0-based) and family (s, linear, cone): [(v, g_x[nx], g_u[nu])] at the nominal node, and g = g_x - g_u K_k (g_x at
    node N) as rows[k][f] = (v[n], g[n, nx]); K[N-1, nu, nx] in the math layout"""
    mdl = au.oracle_model(name, N)
    tgrid = linrange(0.0, 1.0, N)
    nx, nu = xd.shape[1], ud.shape[1]
    out = []
    for k in range(N):
        t, x, u = tgrid[k], xd[k], ud[k]
        fam = [[], [], []]
        s = np.asarray(mdl.s(t, k + 1, x, u, p), float)
        if s.size:
            C, D = np.asarray(mdl.C(t, k + 1, x, u, p), float), np.asarray(mdl.D(t, k + 1, x, u, p), float)
            fam[0] = [(s[i], C[i], D[i]) for i in range(s.size)]
        for v, rows, is_x in ((x, mdl.X(t, k + 1), True), (u, mdl.U(t, k + 1), False)):
            for kind, M, Mp, m0 in rows:
                z = M @ v + (Mp @ p if p.size else 0.0) + m0
                pad = (lambda g: (g, np.zeros(nu))) if is_x else (lambda g: (np.zeros(nx), g))
                if kind == "NONPOS":
                    for i in range(M.shape[0]):
                        if not M[i].any() and Mp[i].any():
                            continue                      # parameter-only: not part of this audit
                        fam[1].append((z[i],) + pad(M[i]))
                else:
                    assert kind == "SOC" and M.shape[0] == 4
                    nrm = np.linalg.norm(z[1:])
                    g = (z[1:] / nrm) @ M[1:] - M[0] if nrm != 0.0 else -M[0]
                    fam[2].append((nrm - z[0],) + pad(g))
        node = []
        for f in range(3):
            v = np.array([r[0] for r in fam[f]], float)
            gx = np.array([r[1] for r in fam[f]], float).reshape(len(fam[f]), nx)
            gu = np.array([r[2] for r in fam[f]], float).reshape(len(fam[f]), nu)
            node.append((v, gx - gu @ K[k] if k < N - 1 else gx))
        out.append(node)
    return out


def table(rows, nx):
    """oracle_rows -> (nrow[3], the library's table [N, nrow, nx+1]) in the reference's own row order"""
    nrow = [rows[0][f][0].size for f in range(3)]
    T = np.zeros((len(rows), sum(nrow), nx + 1))
    for k, node in enumerate(rows):
        r = 0
        for v, g in node:
            T[k, r:r + v.size, :nx], T[k, r:r + v.size, nx] = g, v
            r += v.size
    return np.array(nrow, dtype=np.int32), T


def _winner(vals, largest):
    """(value, flat index of the first winner, gap to the runner-up) of a finite-or-Inf array"""
    v = np.asarray(vals, float).ravel()
    key = -v if largest else v
    order = np.argsort(key, kind="stable")
    with np.errstate(invalid="ignore"):
        gap = abs(v[order[1]] - v[order[0]]) if v.size > 1 else np.inf
    return v[order[0]], int(order[0]), (0.0 if np.isnan(gap) else gap)


class Reference:
    """the covariance audit of ONE problem in numpy.  dyn = (A, Bm, Bp) in memory order (audit_tracking_util.oracle_dynamics),
    K[N-1, nu, nx], rows = oracle_rows(...), Hf[ntc, nx]"""

    def __init__(self, dyn, K, rows, Hf, Sx, Su, sig0, sigu, sigw, nsig=NSIG, strict=True):
        A, Bm, Bp = dyn
        N, nx, nu = A.shape[0] + 1, A.shape[1], Bm.shape[1]
        self.N, self.nx, self.nsig = N, nx, nsig
        Sig = [np.diag(np.asarray(sig0, float) ** 2)]
        for k in range(N - 1):
            Phi, Gam = A[k].T, (Bm[k] + Bp[k]).T
            Acl = Phi - Gam @ K[k]
            S = Acl @ Sig[k] @ Acl.T + Gam @ np.diag(np.asarray(sigu, float) ** 2) @ Gam.T + np.diag(np.asarray(sigw, float) ** 2)
            Sig.append(0.5 * (S + S.T))
        self.Sigma = Sig
        self.sig = np.array([np.sqrt(np.maximum(np.diag(S), 0.0)) for S in Sig])
        self.effort = np.array([np.sqrt(np.maximum(np.diag(K[k] @ Sig[k] @ K[k].T), 0.0)) / Su for k in range(N - 1)])
        self.margin = [[None] * 3 for _ in range(N)]       # [k][f] -> margins of the rows
        node_min = np.full((N, 3), np.inf)
        n_below = 0
        for k in range(N):
            for f in range(3):
                v, g = rows[k][f]
                var = np.maximum(np.einsum("ri,ij,rj->r", g, Sig[k], g), 0.0) if v.size else np.zeros(0)
                nz = (g * g).sum(axis=1) > 0.0 if v.size else np.zeros(0, bool)
                if strict:
                    floor = 1e-12 * (g * g).sum(axis=1) * np.diag(Sig[k]).max() if v.size else np.zeros(0)
                    assert (var[nz] > floor[nz]).all(), ("a row variance sits at roundoff: change the case", k, f, var, floor)
                    assert (var[~nz] == 0.0).all()
                with np.errstate(divide="ignore", invalid="ignore"):
                    m = np.where(var > 0.0, -v / np.sqrt(var), np.where(v <= 0.0, np.inf, -np.inf))
                self.margin[k][f] = m
                if m.size:
                    node_min[k, f] = m.min()
                n_below += int((m < nsig).sum())
        self.node_min = node_min
        self.tau = np.sqrt(np.maximum(np.diag(Hf @ Sig[-1] @ Hf.T), 0.0)) if Hf.size else np.zeros(0)
        iS = np.diag(1.0 / Sx)
        self.trace = np.array([np.trace(iS @ S @ iS) for S in Sig])
        self.ssc = self.sig / Sx[None, :]
        self.nodes = np.zeros((N, NW))
        self.nodes[:, 0] = self.ssc.max(axis=1)
        self.nodes[:-1, 1], self.nodes[-1, 1] = self.effort.max(axis=1), np.nan
        self.nodes[:, 2:5] = node_min
        self.nodes[:, 5] = self.trace
        rec = np.zeros(W)
        rec[1], i, self.gap_sigma = _winner(self.ssc, True)
        rec[2], rec[3] = i // nx + 1, i % nx + 1
        rec[4], i, self.gap_effort = _winner(self.nodes[:-1, 1], True)
        rec[5] = i + 1
        self.gap_margin = [0.0] * 3
        for f in range(3):
            rec[6 + 2 * f], i, self.gap_margin[f] = _winner(node_min[:, f], False)
            rec[7 + 2 * f] = i + 1 if rec[6 + 2 * f] < np.inf else 0
        rec[12] = self.tau.max() if self.tau.size else 0.0
        rec[13] = self.trace[-1]
        rec[14] = n_below
        self.rec = rec
        assert np.isfinite(self.sig).all() and np.isfinite(self.effort).all() and np.isfinite(self.trace).all()

    @staticmethod
    def _close(got, ref, tag):
        got, ref = np.asarray(got, float), np.asarray(ref, float)
        assert got.shape == ref.shape, (tag, got.shape, ref.shape)
        fin = np.isfinite(ref)
        assert np.array_equal(got[~fin], ref[~fin], equal_nan=True), (tag, "non-finite entries", got[~fin], ref[~fin])
        tol = au.RTOL * max(1.0, np.abs(ref[fin]).max() if fin.any() else 0.0)
        err = np.abs(got[fin] - ref[fin]).max() if fin.any() else 0.0
        assert err <= tol, (tag, err, tol)
        return tol

    def check(self, summary, sig=None, nodes=None, tag=""):
        """assert that the outputs of the code under test agree with this reference -> (index comparisons made, skipped)"""
        got = np.asarray(summary, float)
        assert got.shape == (W,), (tag, got.shape)
        print("%s ref %s\n%s got %s" % (tag, np.array2string(self.rec, precision=12), tag, np.array2string(got, precision=12)))
        assert got[0] == 0.0 and got[15] == 0.0, (tag, got)
        made = skipped = 0

        def index(fields, gap, tol):
            nonlocal made, skipped
            if gap > 2.0 * tol:
                made += 1
                for i in fields:
                    assert got[i] == self.rec[i], (tag, "index", i, got[i], self.rec[i])
            else:
                skipped += 1
                for i in fields:
                    assert got[i] == int(got[i]) and 1 <= got[i] <= (self.nx if i == 3 else self.N), (tag, "index", i, got[i])

        index((2, 3), self.gap_sigma, self._close(got[1], self.rec[1], tag + " [1]"))
        index((5,), self.gap_effort, self._close(got[4], self.rec[4], tag + " [4]"))
        for f in range(3):
            tol = self._close(got[6 + 2 * f], self.rec[6 + 2 * f], tag + " [%d]" % (6 + 2 * f))
            if self.rec[6 + 2 * f] == np.inf:
                assert got[7 + 2 * f] == 0.0, (tag, 7 + 2 * f, got)
            else:
                index((7 + 2 * f,), self.gap_margin[f], tol)
        for i in (12, 13):
            self._close(got[i], self.rec[i], tag + " [%d]" % i)
        # the count: exact unless a margin lies within its tolerance of nsig (then either side is accepted for that pair)
        allm = np.concatenate([m for node in self.margin for m in node if m is not None and m.size] or [np.zeros(0)])
        fin = allm[np.isfinite(allm)]
        tol = au.RTOL * max(1.0, np.abs(fin).max() if fin.size else 0.0)
        near = int((np.abs(fin - self.nsig) <= tol).sum())
        assert abs(got[14] - self.rec[14]) <= near, (tag, "n_below", got[14], self.rec[14], near)
        if sig is not None:
            self._close(np.asarray(sig, float).reshape(self.N, self.nx), self.sig, tag + " sig")
        if nodes is not None:
            nodes = np.asarray(nodes, float).reshape(self.N, NW)
            for c in range(6):
                self._close(nodes[:, c], self.nodes[:, c], tag + " nodes[%d]" % c)
            assert not nodes[:, 6:].any(), (tag, nodes[:, 6:])
        return made, skipped


_cache = {}


def reference(orc, name, N, case=None, dyn=None, K=None, key=None):
    """(setup dict, oracle rows, Hf, Reference) of audit_tracking_util.setup(name, N) -- or of another `case` of that model with its
    own dynamics and gains, cached under `key` -- at inputs(s) and NSIG, computed once per session"""
    ck = (name, N, key)
    if ck not in _cache:
        s = atu.setup(orc, name, N)
        xd, ud, p, pp = s["case"] if case is None else case
        dyn = s["dyn"] if dyn is None else dyn
        K = s["K"] if K is None else K
        rows = oracle_rows(name, N, xd, ud, p, K)
        Hf = np.asarray(au.oracle_model(name, N).Hf(xd[-1], p, pp), float).reshape(-1, xd.shape[1])
        _cache[ck] = (s, rows, Hf, Reference(dyn, K, rows, Hf, s["Sx"], s["Su"], *inputs(s)))
    return _cache[ck]
