"""CPU reference of the dispersed-flight audit (include/scp_mi355x.h, scp_audit_dispersed_*), shared by
tests/test_audit_dispersed_cpu.py and tests/test_audit_dispersed_gpu.py.  It takes nothing from the code under test.

Flight d of a problem is audit_util.Reference on transformed nodes: xd' = xd with dx0 added to row 0 only, ud' = ud * gain + bias.
The first-order hold is linear, so holding the transformed nodes is the transformed hold, and the reference's record 8 is already
measured against the untouched last row.  With a truth model the same loop runs over the C oracle's `propagate` with the changed
parameter vector (oracle.default_params layout) and an oracle model instance with the same constants overridden.

The fold is a numpy loop over the flight records the code under test returned, compared bit for bit.  Tolerances: audit_util's
(RTOL, choose_viol_tol over all flights of a call, equal counts); nothing new."""
import numpy as np

import audit_util as au

W = au.W
D3 = 3
SEEDS = {"double_integrator": 11, "quadrotor": 12, "rocket_landing": 13, "starship": 14}      # those of tests/test_audit_cpu.py


def dispersions(name, N, rng):
    """the three flights of the recipe as (dx0[3,nx], ugain[3,nu], ubias[3,nu]): flight 1 undispersed, flight 2 with
    dx0 = 0.01 Sx N(0,1) only, flight 3 with a dx0 of its own plus ugain = 1 + 0.02 N(0,1) and ubias = 0.01 (box width) N(0,1)"""
    mdl = au.oracle_model(name, N)
    Sx = au.state_scale(mdl)
    ub = np.asarray(mdl.bbox()[1], float)
    wu = ub[:, 1] - ub[:, 0]
    dx0, gain, bias = np.zeros((D3, Sx.size)), np.ones((D3, wu.size)), np.zeros((D3, wu.size))
    dx0[1] = 0.01 * Sx * rng.standard_normal(Sx.size)
    dx0[2] = 0.01 * Sx * rng.standard_normal(Sx.size)
    gain[2] = 1.0 + 0.02 * rng.standard_normal(wu.size)
    bias[2] = 0.01 * wu * rng.standard_normal(wu.size)
    return dx0, gain, bias


def flight_references(orc, name, N, case, Sx, res, dx0, gain, bias, truth=None):
    """one Reference per flight of ONE problem; truth = (C-oracle parameter vector, oracle model instance) or None"""
    xd, ud, p, pp = case
    refs = []
    for d in range(dx0.shape[0]):
        x = xd.copy(); x[0] += dx0[d]
        u = ud * gain[d][None, :] + bias[d][None, :]
        refs.append(au.Reference(orc, name, N, x, u, p, pp, Sx, res, *(truth or ())))
        assert np.isfinite(refs[-1].rec[[7, 8, 9]]).all() and np.isfinite(refs[-1].worst).all(), (name, N, res, d, "the reference is not finite")
    return refs


def fold(R):
    """the ordered fold of the flight records R[D, 16] of one problem, operation by operation as the header states it"""
    R = np.asarray(R, float)
    S = np.zeros(W)
    v, dv = [-np.inf] * 3, [0.0] * 3
    par_max, bc, dbc, drift, total, cmax, n_viol, n_bad, m = -np.inf, -np.inf, 0.0, -np.inf, 0.0, -np.inf, 0.0, 0.0, 0
    for d in range(R.shape[0]):
        r = R[d]
        if r[11] != 0.0:
            n_bad += 1.0
            continue
        for f in range(3):
            if r[2 * f] > v[f]:
                v[f], dv[f] = r[2 * f], float(d + 1)
        if m == 0:
            par_max = r[6]
        if r[7] > bc:
            bc, dbc = r[7], float(d + 1)
        if r[8] > drift:
            drift = r[8]
        total = total + r[9]
        if r[9] > cmax:
            cmax = r[9]
        if r[10] > 0.0:
            n_viol += 1.0
        m += 1
    S[0:6] = [v[0], dv[0], v[1], dv[1], v[2], dv[2]]
    S[6] = par_max
    S[7], S[8], S[9], S[15] = (bc, drift, total / m, cmax) if m else (np.nan,) * 4
    S[10], S[11], S[12], S[13], S[14] = n_viol, n_bad, dbc, 2.0, float(R.shape[0])
    return S


_cache = {}


def reference(orc, name, N, seed, res, disp_seed=None, Sx=None):
    """(case, (dx0, gain, bias), [Reference per flight]) for audit_util.make_case(name, N, seed) at `res` with the recipe's three
    flights drawn from default_rng(disp_seed) (1000 + N when None): computed once per session and shared"""
    disp_seed = 1000 + N if disp_seed is None else disp_seed
    key = (name, N, seed, res, disp_seed)
    if key not in _cache:
        case = au.make_case(name, N, seed)
        sx = au.state_scale(au.oracle_model(name, N)) if Sx is None else np.asarray(Sx, float)
        disp = dispersions(name, N, np.random.default_rng(disp_seed))
        _cache[key] = (case, disp, flight_references(orc, name, N, case, sx, res, *disp), sx)
    case, disp, refs, sx = _cache[key]
    assert Sx is None or np.array_equal(sx, Sx)
    return case, disp, refs


def truth(pkg, orc, name, N):
    """a truth model of `name` three ways: (blob of the compiled model, (C-oracle parameter vector, oracle model instance))"""
    mdl = au.oracle_model(name, N)
    par = orc.default_params(name).copy()
    if name == "quadrotor":
        g = 9.81 * 1.05
        par[0] = g
        mdl.g = g                                            # the oracle model's running cost reads it too
        blob = pkg.REGISTRY[name](g=g).par()
    else:
        assert name == "rocket_landing"
        rmin, rmax = mdl.thrust_limits()
        gv, alpha, rmax = np.array([0.0, 0.0, -3.7114 * 1.08]), par[6] * 1.1, 0.9 * rmax
        par[0:3], par[6] = gv, alpha
        mdl.thrust_limits = lambda: (rmin, rmax)             # the rows of s follow the truth model too
        blob = pkg.REGISTRY[name](g=gv, alpha=alpha, rho_max=rmax).par()
    return np.ascontiguousarray(blob, float), (par, mdl)
