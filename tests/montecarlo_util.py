"""CPU reference of the Monte-Carlo audit (include/scp_mi355x.h, scp_audit_montecarlo_*), shared by
tests/test_audit_montecarlo_cpu.py and tests/test_audit_montecarlo_gpu.py.  It takes nothing from the code under test:

  generator  Philox4x32-10 in plain Python integers (also element-wise over numpy uint64 arrays), checked against the Random123
             known answers by the CPU tests; uniforms and Box-Muller normals by the header's formulas in numpy
  flights    audit_tracking_util.TrackingReference's sample-and-hold RK4 flight over the oracle's dynamics with the three noise
             sources of the header, recording e = x - xd[:, k] and du / Su at every node
  moments    numpy over the flights: count, mean, std(ddof=1), rms
  linear     for models RK4 integrates exactly: e_{k+1} = A_k e_k + Gam_k (-K_k e_k + sigu xiu_k) + sigw xiw_{k+1} over the oracle's
             discretize!

Cases, gains and scalings are audit_tracking_util.setup's; sig0 = 0.01 Sx, sigu = 0.01 Su, sigw = 0.002 Sx.
Tolerances: audit_util's for the flight records (check_tracking); moments and stat values au.RTOL max(1, |ref|); an index of stat
must be a place where the reference's own value is within that tolerance of its extreme."""
import numpy as np

import audit_tracking_util as atu
import audit_util as au
from oracle.models import linrange

W, SW = 16, 8      # SCP_AUDIT_WIDTH, SCP_MC_STAT_WIDTH
M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox4x32-10: ctr = 4 words, key = 2 words (Python ints, or numpy uint64 arrays holding 32-bit values) -> 4 words"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def words(seed, kind, k, d, n):
    """the 4 ceil(n / 2) output words of the draw (seed, kind, k, d); d 1-based"""
    out = []
    for q in range((n + 1) // 2):
        out += philox4x32_10((q, k, d - 1, kind), (seed & M32, seed >> 32))
    return np.array(out, dtype=np.uint64)


def normals_from_words(w, n):
    """the first n normals behind the output words w[4 npairs]: Box-Muller on the header's uniforms"""
    w = np.asarray(w, dtype=np.uint64).reshape(-1, 4)
    hi = [(w[:, j] >> np.uint64(5)).astype(np.float64) for j in (0, 2)]
    lo = [(w[:, j] >> np.uint64(6)).astype(np.float64) for j in (1, 3)]
    u1 = (hi[0] * 2.0 ** 26 + lo[0] + 0.5) * 2.0 ** -53
    u2 = (hi[1] * 2.0 ** 26 + lo[1] + 0.5) * 2.0 ** -53
    assert (u1 > 0.0).all() and (u1 < 1.0).all() and (u2 > 0.0).all() and (u2 < 1.0).all()
    rho = np.sqrt(-2.0 * np.log(u1))
    z = np.stack([rho * np.cos(2.0 * np.pi * u2), rho * np.sin(2.0 * np.pi * u2)], axis=1).reshape(-1)
    return z[:n]


def normals(seed, kind, k, d, n):
    return normals_from_words(words(seed, kind, k, d, n), n)


def normals_many(seed, kind, k, D, n):
    """[D, n]: the draw (seed, kind, k, d) of the flights d = 1 .. D at once (uint64 arrays through the same Philox)"""
    d = np.arange(D, dtype=np.uint64)
    cols = []
    for q in range((n + 1) // 2):
        full = lambda v: np.full(D, v, dtype=np.uint64)      # noqa: E731
        w = philox4x32_10((full(q), full(k), d, full(kind)), (full(seed & M32), full(seed >> 32)))
        cols.append(np.stack(w, axis=1))
    w = np.stack(cols, axis=1).reshape(D, -1)
    return normals_from_words(w.reshape(-1), D * 2 * len(cols)).reshape(D, -1)[:, :n]


def sigmas(s):
    """(sig0, sigu, sigw) of a setup() dict"""
    return 0.01 * s["Sx"], 0.01 * s["Su"], 0.002 * s["Sx"]


class NoisyReference(atu.TrackingReference):
    """ONE noisy closed-loop flight d (1-based) on the CPU in the form check_tracking reads, with the node errors e[N, nx] and the
    scaled hold updates dus[N-1, nu]"""

    def __init__(self, orc, name, N, xd, ud, p, pp, Sx, Su, K, steps, seed, d, sig0, sigu, sigw):
        par, mdl = orc.default_params(name), au.oracle_model(name, N)
        res = steps * (N - 1) + 1
        self.name, self.res = name, res
        tgrid = linrange(0.0, 1.0, N)
        tc = np.array([(1 - j / (res - 1)) * 0.0 + (j / (res - 1)) * 1.0 for j in range(res)])
        self.tc = tc
        ct = mdl.cost_terms()
        nx, nu = xd.shape[1], ud.shape[1]
        x, du, wk = xd[0] + sig0 * normals(seed, 0, 0, d, nx), np.zeros(nu), np.zeros(nu)
        self.effort, self.track = np.zeros(N - 1), np.zeros(N)
        self.e, self.dus = np.zeros((N, nx)), np.zeros((N - 1, nu))

        def flown(t):
            return (au._input(tgrid, ud, t) + du) + wk

        def f(t, xs):
            return orc.model_eval(name, par, t, N, xs, flown(t), p)[0]

        fam, scale, gam, par_max = np.full((res, 3), -np.inf), np.ones((res, 3)), np.zeros(res), -np.inf

        def sample(j):
            nonlocal par_max
            t = tc[j]
            k = max(int(np.sum(tgrid <= t)), 1)
            fam[j], scale[j], pm, gam[j] = au._sample(name, mdl, ct, t, k, x, flown(t), p)
            par_max = max(par_max, pm)

        def node(k):
            nonlocal du, wk
            e = x - xd[k - 1]
            self.e[k - 1] = e
            self.track[k - 1] = np.abs(e / Sx).max()
            if k < N:
                du = -(K[k - 1] @ e)
                self.dus[k - 1] = du / Su
                self.effort[k - 1] = np.abs(du / Su).max()
                wk = sigu * normals(seed, 1, k, d, nu)

        node(1)
        sample(0)
        for j in range(res - 1):
            if j > 0 and j % steps == 0:
                node(j // steps + 1)
            t, h = tc[j], tc[j + 1] - tc[j]
            k1 = f(t, x)
            k2 = f(t + h / 2, x + h / 2 * k1)
            k3 = f(t + h / 2, x + h / 2 * k2)
            k4 = f(t + h, x + h * k3)
            x = x + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
            if (j + 1) % steps == 0:
                x = x + sigw * normals(seed, 2, (j + 1) // steps + 1, d, nx)
            sample(j + 1)
        node(N)
        self.fam, self.scale = fam, scale
        rec = np.zeros(W)
        for i in range(3):
            if np.isfinite(fam[:, i]).any():
                j = int(np.argmax(fam[:, i]))
                rec[2 * i], rec[2 * i + 1] = fam[j, i], tc[j]
            else:
                rec[2 * i], rec[2 * i + 1] = -np.inf, 0.0
        rec[6] = par_max
        rec[7] = np.abs(mdl.gtc(x, p, pp)).max()
        rec[8] = np.abs((x - xd[-1]) / Sx).max()
        phi = ct["tx"] @ x + (ct["tp"] @ p + ct["Qp"] @ (p * p) if p.size else 0.0)
        rec[9] = phi + sum(0.5 * (tc[j + 1] - tc[j]) * (gam[j + 1] + gam[j]) for j in range(res - 1))
        rec[12], rec[13] = self.effort.max(), float(np.argmax(self.effort) + 1)
        rec[14], rec[15] = self.track.max(), float(np.argmax(self.track) + 1)
        self.worst = fam.max(axis=1)
        self.rec = rec
        assert np.isfinite(rec[[7, 8, 9, 12, 14]]).all() and np.isfinite(self.worst).all(), (name, N, steps, "the reference is not finite")


def moments(E, U):
    """E[D, N, nx] node errors and U[D, N-1, nu] scaled hold updates of D flights -> the library's node records [N, 1 + 2 nx + nu]"""
    D, N, nx = E.shape
    nu = U.shape[2]
    out = np.full((N, 1 + 2 * nx + nu), np.nan)
    out[:, 0] = D
    out[:, 1:1 + nx] = E.mean(axis=0)
    out[:, 1 + nx:1 + 2 * nx] = E.std(axis=0, ddof=1)
    out[:-1, 1 + 2 * nx:] = np.sqrt((U * U).mean(axis=0))
    return out


def check_moments(got, ref, tag=""):
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (tag, "NaN pattern", got, ref)
    tol = au.RTOL * np.maximum(1.0, np.abs(ref[~nan]))
    err = np.abs(got[~nan] - ref[~nan])
    print("%s moments: max err / tol %.3e" % (tag, (err / tol).max()))
    assert (err <= tol).all(), (tag, err.max())


def check_stat(got, mom, Sx, D, tag=""):
    """stat[8] of the code under test against the reference node records mom[N, NV]"""
    got = np.asarray(got, float)
    assert got.shape == (SW,), (tag, got.shape)
    N, nx = mom.shape[0], Sx.size
    s, m, r = mom[:, 1 + nx:1 + 2 * nx] / Sx, np.abs(mom[:, 1:1 + nx]) / Sx, mom[:-1, 1 + 2 * nx:]
    print("%s stat ref %s %s %s got %s" % (tag, s.max(), m.max(), r.max(), got))
    for i, arr, idx in ((0, s, (1, 2)), (3, m, (4,)), (5, r, (6,))):
        tol = au.RTOL * max(1.0, arr.max())
        assert abs(got[i] - arr.max()) <= tol, (tag, i, got[i], arr.max(), tol)
        k = got[idx[0]]
        assert k == int(k) and 1 <= k <= arr.shape[0], (tag, idx, k)
        if len(idx) == 2:
            j = got[idx[1]]
            assert j == int(j) and 1 <= j <= arr.shape[1], (tag, idx, j)
            assert abs(arr[int(k) - 1, int(j) - 1] - arr.max()) <= tol, (tag, idx, k, j)
        else:
            assert abs(arr[int(k) - 1].max() - arr.max()) <= tol, (tag, idx, k)
    assert got[7] == float(D), (tag, got[7])


_cache = {}


def references(orc, name, N, steps, D, seed, case=None, K=None, Sx=None, Su=None, key=None):
    """[NoisyReference of flight d = 1 .. D] of atu.setup(name, N) (or of `case` with gains K, cached under `key`), and their node
    records"""
    s = atu.setup(orc, name, N)
    ck = (name, N, steps, D, seed, key, None if Sx is None else Sx.tobytes(), None if Su is None else Su.tobytes())
    if ck not in _cache:
        sx, su = s["Sx"] if Sx is None else Sx, s["Su"] if Su is None else Su
        sig = sigmas(s)
        refs = [NoisyReference(orc, name, N, *(s["case"] if case is None else case), sx, su, s["K"] if K is None else K, steps, seed, d, *sig)
                for d in range(1, D + 1)]
        mom = moments(np.stack([r.e for r in refs]), np.stack([r.dus for r in refs]))
        _cache[ck] = (refs, mom)
    return _cache[ck]


def linear_errors(dyn, K, D, seed, sig0, sigu, sigw):
    """E[D, N, nx] and U[D, N-1, nu] unscaled du of the linear recursion over memory-order blocks dyn = (A, Bm, Bp), K[N-1, nu, nx]"""
    A, Bm, Bp = dyn
    N, nx, nu = A.shape[0] + 1, A.shape[1], Bm.shape[1]
    E, U = np.zeros((D, N, nx)), np.zeros((D, N - 1, nu))
    E[:, 0] = sig0 * normals_many(seed, 0, 0, D, nx)
    for k in range(N - 1):
        Phi, Gam = A[k].T, (Bm[k] + Bp[k]).T
        U[:, k] = -(E[:, k] @ K[k].T)
        flown = U[:, k] + sigu * normals_many(seed, 1, k + 1, D, nu)
        E[:, k + 1] = E[:, k] @ Phi.T + flown @ Gam.T + sigw * normals_many(seed, 2, k + 2, D, nx)
    return E, U
