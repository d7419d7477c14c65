"""CPU reference of the continuous-time audit (include/scp_mi355x.h, scp_audit_*), shared by tests/test_audit_cpu.py and
tests/test_audit_gpu.py.  It takes nothing from the code under test: xc comes from the oracle's `propagate`
(oracle/scp_oracle.c), everything else from the closures of oracle/models.py (s, X, U, gtc, cost_terms).

Row families.  The oracle lists the parameter-only rows (the t_f bounds) inside X / U; the library keeps them apart
(record 6).  A NONPOS row whose state / input matrix is zero and whose parameter matrix is not is parameter-only here;
every other NONPOS row is a "linear row" (record 2), every SOC a cone (record 4).

Tolerances: `propagate` is held to 1e-10 relative; an audited maximum is a row applied
to xc whose terms may be far larger than its value, so a value is compared with 1e-9 * max(1, largest absolute term
entering that row at the reference's arg-max sample); records 7-9 with 1e-9 * max(1, |ref|).  Reported times are not
compared with the reference's arg-max (the guesses contain exact ties): the reference's own sample value AT the
reported time must be within the same tolerance of the reference maximum.  viol_tol is chosen from the reference so
that no sample's worst value lies within 1e-6 relative of it; the counts must then be equal."""
import ctypes
import math

import numpy as np

from oracle.models import MODELS, linrange

W = 16      # SCP_AUDIT_WIDTH
AUDIT_MODELS = ("double_integrator", "quadrotor", "rocket_landing", "starship")
RTOL = 1e-9


def oracle_model(name, N):
    return MODELS[name](N) if name in ("starship", "oscillator") else MODELS[name]()


def state_scale(mdl):
    """diag(Sx) by the rule of scp.jl:479-511 from the model's bounding box"""
    w = np.asarray(mdl.bbox()[0], float)
    w = w[:, 1] - w[:, 0]
    return np.where(w < math.sqrt(np.finfo(float).eps), 1.0, w)


def res_values(N):
    """2: the smallest; 4 (N - 1) + 1: samples exactly on the grid nodes (tests k_j there); 2 * 3 * (N - 1): the reference's rule at Nsub = 3"""
    return (2, 4 * (N - 1) + 1, 2 * 3 * (N - 1))


def make_case(name, N, seed):
    """the model's guess plus a fixed-seed perturbation, about a perturbed pp: (xd[N,nx], ud[N,nu], p[np], pp)"""
    mdl = oracle_model(name, N)
    rng = np.random.default_rng(seed)
    pp = mdl.nominal_pp() * (1.0 + 0.1 * rng.uniform(-1, 1, size=mdl.nominal_pp().size))
    x, u, p = mdl.guess(N, pp)
    Sx = state_scale(mdl)
    ub = np.asarray(mdl.bbox()[1], float)
    x = x + 0.03 * Sx[None, :] * rng.standard_normal(x.shape)
    u = u + 0.03 * (ub[:, 1] - ub[:, 0])[None, :] * rng.standard_normal(u.shape)
    p = np.asarray(p, float) * (1.0 + 0.05 * rng.uniform(-1, 1, size=np.asarray(p).shape))
    return np.ascontiguousarray(x), np.ascontiguousarray(u), np.ascontiguousarray(p), np.ascontiguousarray(pp)


def _input(tgrid, ud, t):
    """linterp(ud, t_grid)(t) (helper.jl:84-118): bin = number of grid points strictly below t, at least 1"""
    t = min(max(t, tgrid[0]), tgrid[-1])
    k = min(max(int(np.sum(tgrid < t)), 1), tgrid.size - 1)
    c = (tgrid[k] - t) / (tgrid[k] - tgrid[k - 1])
    return c * ud[k - 1] + (1.0 - c) * ud[k]


def _s_terms(name, mdl, x, u, p):
    """per row of s: the largest absolute term entering it"""
    if name == "double_integrator":
        return [max(1.0, u[0] ** 2)]
    if name == "quadrotor":
        return [max(1.0, np.linalg.norm(H @ x[0:3]), np.linalg.norm(H @ c)) for H, c in zip(mdl.obs_H, mdl.obs_c)]
    if name == "rocket_landing":
        rmin, rmax = mdl.thrust_limits()
        return [max(rmin * math.exp(-x[6]), abs(u[3])), max(rmax * math.exp(-x[6]), abs(u[3]))]
    assert name == "starship"
    a = max(abs(u[1]), abs(x[7]), abs(u[2]) * mdl.rate_delay)
    b = max(abs(u[2]), mdl.deltadot_max)
    pw = [max(abs(p[2 + i]), abs(x[i])) for i in range(8)]
    th = max(abs(x[4]), mdl.theta_max2)
    return [a, a, b, b, max(np.linalg.norm(x[0:2]) * math.cos(mdl.gamma_gs), abs(x[1]))] + pw + pw + [th, th]


def _sample(name, mdl, ct, t, k, x, u, p):
    """(values of the three sampled families, their term scales, parameter-only maximum, Gamma) at one sample"""
    fam, scale, par_max = np.full(3, -np.inf), np.ones(3), -np.inf
    s = mdl.s(t, k, x, u, p)
    if len(s):
        i = int(np.argmax(s))
        fam[0], scale[0] = s[i], max(1.0, _s_terms(name, mdl, x, u, p)[i])
    for v, rows in ((x, mdl.X(t, k)), (u, mdl.U(t, k))):
        for kind, M, Mp, m0 in rows:
            terms = [np.abs(M * v[None, :]), np.abs(Mp * p[None, :]) if p.size else np.zeros((M.shape[0], 0)), np.abs(m0)[:, None]]
            tmax = np.concatenate(terms, axis=1).max(axis=1)
            z = M @ v + (Mp @ p if p.size else 0.0) + m0
            if kind == "NONPOS":
                for i in range(M.shape[0]):
                    if not M[i].any() and Mp[i].any():
                        par_max = max(par_max, z[i])
                    elif z[i] > fam[1]:
                        fam[1], scale[1] = z[i], max(1.0, tmax[i])
            else:
                assert kind == "SOC" and M.shape[0] == 4
                q = np.linalg.norm(z[1:]) - z[0]
                if q > fam[2]:
                    fam[2], scale[2] = q, max(1.0, tmax.max())
    return fam, scale, par_max, ct["Qu"] @ (u * u) + ct["lu"] @ u + ct["lx"] @ x


class Reference:
    """the audit of ONE problem on the CPU: per-sample values of the three sampled families, their term scales, and the record"""

    def __init__(self, orc, name, N, xd, ud, p, pp, Sx, res, par=None, mdl=None):
        # a truth model: `par` the C oracle's parameter vector, `mdl` the oracle model instance with the same constants overridden
        par = orc.default_params(name) if par is None else par
        mdl = oracle_model(name, N) if mdl is None else mdl
        self.name, self.res = name, res
        tc, xc = orc.propagate(name, par, N, xd, ud, p, res=res)
        tgrid = linrange(0.0, 1.0, N)
        self.tc = tc
        fam = np.full((res, 3), -np.inf)          # s, linear rows, cones
        scale = np.ones((res, 3))                 # largest absolute term of the row that attains the sample's maximum
        par_max, gam = -np.inf, np.zeros(res)
        ct = mdl.cost_terms()
        for j in range(res):
            t = tc[j]
            k = max(int(np.sum(tgrid <= t)), 1)   # 1-based index of the last grid node <= t
            fam[j], scale[j], pm, gam[j] = _sample(name, mdl, ct, t, k, xc[j], _input(tgrid, ud, t), p)
            par_max = max(par_max, pm)            # parameter-only rows: the same at every sample
        self.fam, self.scale = fam, scale
        rec = np.zeros(W)
        for f in range(3):
            if np.isfinite(fam[:, f]).any():
                j = int(np.argmax(fam[:, f]))     # first maximum
                rec[2 * f], rec[2 * f + 1] = fam[j, f], tc[j]
            else:
                rec[2 * f], rec[2 * f + 1] = -np.inf, 0.0
        rec[6] = par_max
        xf = xc[-1]
        rec[7] = np.abs(mdl.gtc(xf, p, pp)).max()
        rec[8] = np.abs((xf - xd[-1]) / Sx).max()
        phi = ct["tx"] @ xf + (ct["tp"] @ p + ct["Qp"] @ (p * p) if p.size else 0.0)
        rec[9] = phi + sum(0.5 * (tc[j + 1] - tc[j]) * (gam[j + 1] + gam[j]) for j in range(res - 1))
        self.worst = fam.max(axis=1)              # per sample: the worst value of the three sampled families
        self.rec = rec

    def check(self, got, viol_tol, tag=""):
        """assert that the record `got` of the code under test, computed with `viol_tol`, agrees with this reference"""
        got = np.asarray(got, float)
        assert got.shape == (W,), (tag, got.shape)
        print("%s ref %s\n%s got %s" % (tag, np.array2string(self.rec[:12], precision=15), tag, np.array2string(got[:12], precision=15)))
        for f in range(3):
            vref, v, t = self.rec[2 * f], got[2 * f], got[2 * f + 1]
            if not np.isfinite(vref):
                assert v == -np.inf and t == 0.0, (tag, f, v, t)
                continue
            jr = int(np.argmax(self.fam[:, f]))
            tol = RTOL * self.scale[jr, f]
            assert abs(v - vref) <= tol, (tag, "family", f, v, vref, tol)
            j = np.nonzero(self.tc == t)[0]
            assert j.size == 1, (tag, "family", f, "reported time is not a sample time", t)
            assert abs(self.fam[j[0], f] - vref) <= tol, (tag, "family", f, "time", t, self.fam[j[0], f], vref, tol)
        if np.isfinite(self.rec[6]):
            assert abs(got[6] - self.rec[6]) <= RTOL * max(1.0, abs(self.rec[6])), (tag, 6, got[6], self.rec[6])
        else:
            assert got[6] == -np.inf, (tag, 6, got[6])
        for i in (7, 8, 9):
            assert abs(got[i] - self.rec[i]) <= RTOL * max(1.0, abs(self.rec[i])), (tag, i, got[i], self.rec[i])
        assert (np.abs(self.worst - viol_tol) > 1e-6 * max(1.0, abs(viol_tol))).all(), (tag, "viol_tol too close to a sample", viol_tol)
        n_viol = float((self.worst > viol_tol).sum())
        assert got[10] == n_viol, (tag, "n_viol", got[10], n_viol, viol_tol)
        assert got[11] == 0.0 and not got[12:].any(), (tag, got[11:])


def choose_viol_tol(refs):
    """a viol_tol for one call over `refs`: the middle of the widest gap between the samples' worst values (beyond the largest
    when they all tie), so that no sample of any instance lies within 1e-6 relative of it"""
    w = np.sort(np.concatenate([r.worst for r in refs]))
    w = w[np.isfinite(w)]
    gaps = np.diff(w)
    if gaps.size and gaps.max() > 4e-6 * max(1.0, np.abs(w).max()):
        g = int(np.argmax(gaps))
        return 0.5 * (w[g] + w[g + 1])
    return w[-1] + 1.0


_cache = {}


def reference(orc, name, N, seed, res, Sx=None):
    """(case, Reference) for make_case(name, N, seed) at `res`: computed once per session and shared"""
    key = (name, N, seed, res)
    if key not in _cache:
        case = make_case(name, N, seed)
        sx = state_scale(oracle_model(name, N)) if Sx is None else np.asarray(Sx, float)
        _cache[key] = (case, Reference(orc, name, N, *case, sx, res), sx)
    case, ref, sx = _cache[key]
    assert Sx is None or np.array_equal(sx, Sx)
    return case, ref


def model_blob(pkg, name, N):
    """parameter blob of the compiled model at its defaults (the constants of oracle/models.py)"""
    mdl = pkg.REGISTRY[name]()
    if name == "starship":
        mdl.N = N
    return np.ascontiguousarray(mdl.par(), float)


def vp(a):
    return None if a is None else np.ascontiguousarray(a, float).ctypes.data_as(ctypes.c_void_p)
