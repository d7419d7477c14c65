"""Oscillator with actuator deadband (test/examples/oscillator), CPU side: the compiled model's closures evaluated on the host
through the C ABI against the numpy restatement of oracle/models.py, the restatement itself against the C oracle on a
model both know, the node-parameter running cost, the PTR template with no terminal condition against the oracle's literal
program, the mutable-constant mask, the homotopy schedule and the committed fixture."""
import ctypes
import math
import os

import numpy as np
import pytest

from oracle import conic_host, discretize_ref, models, ptr_ref
from oracle.models import MODELS
from template_util import make_src, template_matrices

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oscillator_outcomes_n12.npz")
OSC = 5
KAPPAS = [4.595, 2.1e3, 4.595e8]


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_model_query(pkg):
    info = pkg._lib.ScpModelInfo()
    assert pkg._lib.lib().scp_model_query(OSC, ctypes.byref(info)) == 0
    assert (info.nx, info.nu, info.np, info.np_node, info.npF) == (2, 4, 0, 1, 0)
    assert (info.ns, info.nic, info.ntc, info.nsoc, info.ng, info.nl) == (2, 2, 0, 0, 0, 10)
    assert (info.npp, info.npar, info.structured, info.has_subproblem, info.s_input_free, info.linf_groups) == (2, 9, 0, 1, 0, 0)
    m = pkg.REGISTRY["oscillator"]()
    np.testing.assert_array_equal(m.par(), models.Oscillator(5).par())      # defaults of parameters.jl:69-115, kappa1 = r_nrml = 1
    np.testing.assert_array_equal(m.nominal_pp(), [1.0, 0.0])
    assert pkg.TrajectoryProblem("oscillator", kappa1=3.0).mdl.par()[5] == 3.0


@pytest.mark.parametrize("method", ["foh", "impulse"])
def test_numpy_discretisation_agrees_with_the_c_oracle_on_the_double_integrator(orc, method):
    """keeps the restatement of derivs_foh / derivs_impulse honest: both know the double integrator"""
    N, Nsub = 5, 4
    g, T = orc.default_params("double_integrator")

    class DI:
        nx, nu = 2, 1

        def f(self, t, k, x, u, p):
            return np.array([0.0, u[0]]) if k < 0 else T * np.array([x[1], u[0] - g])

        def A(self, t, k, x, u, p):
            return T * np.array([[0.0, 1.0], [0.0, 0.0]])

        def B(self, t, k, x, u, p):
            return np.array([[0.0], [1.0]]) * (1.0 if k < 0 else T)

        def F(self, t, k, x, u, p):
            return np.zeros((2, 0))
    rng = np.random.default_rng(3)
    x, u, p = rng.standard_normal((N, 2)), rng.standard_normal((N, 1)), np.zeros(0)
    iSx = np.array([0.5, 2.0])
    mine = discretize_ref.discretize_arrays(DI(), N, Nsub, x, u, p, iSx, 1e-3, method)
    o = orc.discretize("double_integrator", np.array([g, T]), N, Nsub, x[None], u[None], p[None], iSx, 1e-3, method=method)
    for nm in ("A", "Bm", "Bp", "E"):
        ref = np.swapaxes(o[nm][0], 1, 2)
        assert np.abs(mine[nm] - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), nm
    for nm in ("r", "defect"):
        assert np.abs(mine[nm] - o[nm][0]).max() <= 1e-12 * max(1.0, np.abs(o[nm][0]).max()), nm
    assert bool(o["feas"][0]) == mine["feas"]


def _eval(pkg, par, N, k, x, u, p):
    f, A, B = np.zeros(2), np.zeros((2, 2)), np.zeros((4, 2))
    s, C, D, G = np.zeros(2), np.zeros((2, 2)), np.zeros((2, 4)), np.zeros((2, 1))
    q, nq = np.zeros(8), ctypes.c_int(0)
    rc = pkg._lib.lib().scp_model_eval_host(OSC, _vp(par), N, k, _vp(x), _vp(u), _vp(p), _vp(f), _vp(A), _vp(B), None, _vp(s), _vp(C),
                                            _vp(D), _vp(G), _vp(q), ctypes.byref(nq))
    assert rc == 0
    return dict(f=f, A=A.T, B=B.T, s=s, C=C, D=D, G=G, q=q[:nq.value])


def _points(mdl, N):
    rng = np.random.default_rng(11)
    db, am = mdl.a_db, mdl.a_max
    ars = [0.0, db, -db, db * (1 + 1e-6), db * (1 - 1e-6), -db * (1 + 1e-6), -db * (1 - 1e-6), am, -am] + list(rng.uniform(-am, am, 8))
    for ar in ars:
        u = np.array([rng.uniform(-am, am), ar, rng.uniform(0, am), rng.uniform(0, 2 * am)])
        yield rng.integers(1, N + 1), rng.standard_normal(2), u, np.abs(rng.standard_normal(N))


@pytest.mark.parametrize("kappa", KAPPAS)
def test_compiled_closures_against_the_restatement(pkg, kappa):
    N = 7
    mdl = models.Oscillator(N, kappa)
    par = mdl.par()
    for k, x, u, p in _points(mdl, N):
        k = int(k)
        got = _eval(pkg, par, N, k, x, u, p)
        t = k / (N - 1)
        want = dict(f=mdl.f(t, k, x, u, p), A=mdl.A(t, k, x, u, p), B=mdl.B(t, k, x, u, p), s=mdl.s(t, k, x, u, p),
                    C=mdl.C(t, k, x, u, p), D=mdl.D(t, k, x, u, p), G=np.zeros((2, 1)))
        for nm, w in want.items():
            assert np.isfinite(got[nm]).all(), (nm, kappa, u)
            assert np.abs(got[nm] - w).max() <= 1e-12 * max(1.0, np.abs(w).max()), (nm, kappa, u, got[nm], w)
        # the cone indicators of X: +-r - l1r_k
        np.testing.assert_allclose(np.sort(got["q"]), np.sort([x[0] - p[k - 1], -x[0] - p[k - 1]]), rtol=0, atol=1e-15)


@pytest.mark.parametrize("kappa", [4.595, 35.6])
def test_jacobian_of_the_deadband_against_central_differences(pkg, kappa):
    N = 7
    mdl = models.Oscillator(N, kappa)
    par, h = mdl.par(), 1e-6
    for k, x, u, p in _points(mdl, N):
        D = _eval(pkg, par, N, int(k), x, u, p)["D"]
        for j in range(4):
            e = np.zeros(4); e[j] = h
            fd = (_eval(pkg, par, N, int(k), x, u + e, p)["s"] - _eval(pkg, par, N, int(k), x, u - e, p)["s"]) / (2 * h)
            assert np.abs(D[:, j] - fd).max() <= 1e-6 * max(1.0, np.abs(fd).max()), (kappa, u, j, D[:, j], fd)


def test_rows_and_cost_against_the_restatement(pkg):
    N = 5
    pm = pkg.REGISTRY["oscillator"]()
    mr = pkg.subproblem.ModelRows(pm, N)
    mdl = models.Oscillator(N)
    for k in (1, 3, N):
        L, Lp, l, Mm, m = mr.rows(N, k)
        assert Mm.shape[0] == 0 and L.shape == (10, 6) and Lp.shape == (10, N)
        want = [(np.concatenate([np.zeros(2), M[0]]), Mp[0], m0[0]) for _, M, Mp, m0 in mdl.U(0.0, k)] + \
               [(np.concatenate([M[0], np.zeros(4)]), Mp[0], m0[0]) for _, M, Mp, m0 in mdl.X(0.0, k)]
        for i, (Lw, Lpw, lw) in enumerate(want):
            np.testing.assert_array_equal(L[i], Lw); np.testing.assert_array_equal(Lp[i], Lpw); assert l[i] == lw
    ct, cw = mr.cost_terms(N), mdl.cost_terms()
    # the node parameter sits in the RUNNING cost: node k's coefficient carries the trapezoid weight
    np.testing.assert_allclose(ct["tp"], np.array([1 / 8, 1 / 4, 1 / 4, 1 / 4, 1 / 8]) / mdl.r_nrml, rtol=0, atol=1e-16)
    for nm in ("Qu", "lu", "lx", "tx", "tp", "Qp"):
        np.testing.assert_allclose(ct[nm], cw[nm], rtol=0, atol=1e-16)
    assert mr.state_indicators(N) == 2


def test_freeflyer_node_cost_terms_are_still_tiled(pkg):
    N = 4
    mr = pkg.subproblem.ModelRows(pkg.REGISTRY["freeflyer"](), N)
    ct = mr.cost_terms(N)
    np.testing.assert_array_equal(ct["tp"], np.concatenate([[0.0], np.full(6 * N, -1e-4)]))
    np.testing.assert_array_equal(ct["Qp"][1:], np.zeros(6 * N))


@pytest.mark.parametrize("kappa", [models.KAPPA3[0], models.KAPPA3[2]])
def test_ptr_template_without_a_terminal_condition_equals_the_oracles_program(pkg, orc, kappa):
    """in the manner of tests/test_template_cpu.py: the product's template (ntc = 0: empty vtc, Pf[1] >= ||[]||_1, zero-row
    sources Hf / Kf / lf; the node parameter in the running cost) about the guess, solved by the host build of the conic solver,
    against the oracle's literal program"""
    N, Nsub = 6, 5
    mdl = models.Oscillator(N, kappa)
    pm = pkg.REGISTRY["oscillator"](kappa1=kappa)
    mr = pkg.subproblem.ModelRows(pm)
    scale = ptr_ref.Scaling(*mdl.bbox())
    pars = ptr_ref.reference_pars(N, Nsub)
    pp = np.array([0.7, 0.2])
    x, u, p = mdl.guess(N, pp)
    ref = ptr_ref.discretize(mdl, pars, scale, x, u, p)
    o = ptr_ref.solve_subproblem(mdl, pars, scale, ref, pp)
    T = pkg.subproblem.build_ptr(mr, N, scale, pars.wvc, pars.wtr, np.inf)
    assert T.variables["vtc"].size == 0 and T.variables["vic"].size == 2
    assert T.n == o["sizes"]["n"] and T.p == o["sizes"]["p"]
    v, G, A, P = template_matrices(T, make_src(T, mdl, ref, pp))
    r = conic_host.solve(v["c"], G, v["h"], T.l, T.q, A, v["b"], P=P)
    assert r["status"] in (0, 1)
    assert abs(r["pcost"] + T.cost_const - o["J_aug"]) <= 1e-6 * max(1.0, abs(o["J_aug"]))
    assert abs(r["x"][T.variables["Pf"]][1]) <= 1e-6      # the penalty of the empty terminal condition


def test_mutable_constants(pkg):
    L = pkg._lib.lib()
    for mid, npar in ((0, 2), (1, 19), (2, 17), (3, 25), (4, 61), (OSC, 9)):
        info = pkg._lib.ScpModelInfo()
        assert L.scp_model_query(mid, ctypes.byref(info)) == 0 and info.npar == npar
        mask = (ctypes.c_int * npar)(*([7] * npar))
        assert L.scp_model_par_mutable(mid, mask) == 0
        assert list(mask) == ([int(i == 5) for i in range(9)] if mid == OSC else [0] * npar)
    assert L.scp_model_par_mutable(99, (ctypes.c_int * 4)()) == 2
    assert L.scp_model_par_mutable(OSC, None) == 1
    assert L.scp_problem_set_model_par(None, None) == 1
    assert L.scp_ptr_generic_continue(None, None) == 1
    assert pkg.REGISTRY["oscillator"].PAR_NAMES[5] == "kappa1"


def test_audits_refuse_the_oscillator(pkg):
    L = pkg._lib.lib()
    one = np.ones(64)
    par = models.Oscillator(5).par()
    assert L.scp_model_audit_host(OSC, _vp(par), 5, _vp(one), _vp(one), _vp(one), _vp(one), _vp(one), 4, 0.0, _vp(one)) == 7
    assert L.scp_model_audit_intervals_host(OSC, _vp(par), 5, 0, _vp(one), _vp(one), _vp(one), _vp(one), _vp(one), 4, 0.0, _vp(one),
                                            _vp(one)) == 7


def test_homotopy_schedule(pkg):
    h = pkg.Homotopy(1e-8)
    assert h(0) == pytest.approx(math.log(99.0), rel=1e-15)
    assert h(1) == pytest.approx(1e8 * math.log(99.0), rel=1e-14)
    assert h(0.5) == pytest.approx(1e4 * math.log(99.0), rel=1e-14)
    assert pkg.Homotopy(1e-3, delta_max=0.5, eps=0.1)(1) == pytest.approx(math.log(9.0) / 1e-3, rel=1e-14)
    np.testing.assert_allclose([h(x) for x in np.linspace(0, 1, 10)], models.KAPPA10, rtol=1e-13)


def test_guess_is_the_free_response(pkg):
    """the Python model's guess and the restatement's against the closed form of the underdamped free response.  RK4 at 999 steps
    is exact to 1e-10 here; what remains is the reference's LINEAR sampling between the 1000 grid points (definition.jl:95-97):
    at most (1/999)^2 / 8 * max |d2x / dtau2| <= 1.25e-7 * tf^2 * 2 (|r0| + |v0|) = 2.5e-5 (|r0| + |v0|); asserted at twice that"""
    pm, N = pkg.REGISTRY["oscillator"](), 12
    wd = pm.w0 * math.sqrt(1.0 - pm.zeta ** 2)
    t = pm.tf * np.arange(N) / (N - 1)
    for pp in models.INSTANCES:
        r0, v0 = pp
        a, b = r0, (v0 + pm.zeta * pm.w0 * r0) / wd
        e = np.exp(-pm.zeta * pm.w0 * t)
        r = e * (a * np.cos(wd * t) + b * np.sin(wd * t))
        v = -pm.zeta * pm.w0 * r + e * wd * (-a * np.sin(wd * t) + b * np.cos(wd * t))
        for mdl in (pm, models.Oscillator(N)):
            x, u, p = mdl.guess(N, pp)
            assert np.abs(x - np.stack([r, v], axis=1)).max() <= 5e-5 * (abs(r0) + abs(v0))
            np.testing.assert_array_equal(x[0], pp)
            np.testing.assert_array_equal(p, np.abs(x[:, 0]))
            assert u.shape == (N, 4) and not u.any()


def test_generator_reproduces_the_committed_fixture():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_oscillator_outcomes", os.path.join(os.path.dirname(GOLDEN), "make_oscillator_outcomes.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    d, g = gen.compute(), np.load(GOLDEN)
    for nm in ("status", "iterations", "status30", "iterations30"):
        np.testing.assert_array_equal(d[nm], g[nm])
    assert (g["status"] == 0).all() and (g["status30"] == 0).all()      # the reference's own assertion (tests.jl:81), every stage
    for nm in ("J", "J30", "J_aug_first"):
        assert np.abs(d[nm] - g[nm]).max() <= 1e-6 * np.maximum(1.0, np.abs(g[nm])).max(), nm
    assert abs(g["J30"][-1] - 0.128624) < 5e-6
