"""The program families of tests/conic_families.py on the HOST build of the conic solver (oracle/conic_host) and on the independent
oracle (oracle/ipm.py), where there is no GPU: every fact that tests/test_conic_geometry_gpu.py expects of the device kernel in
every launch geometry is pinned here first -- intended statuses, iteration counts, extended-precision certificates, closed forms.

Also pinned, as a known LIMIT: the unbounded members of the mixed family are certified for seed 34 only (see
test_unbounded_members_are_never_mistaken_for_solved)."""
import collections

import numpy as np
import pytest

import conic_families as cf


@pytest.fixture(scope="module", autouse=True)
def _build(orc):
    return orc


def _certified(fam, r):
    bad = {t: cf.certify(fam, r, t) for t in range(fam.B)}
    return {t: v for t, v in bad.items() if v}


def test_mixed_family_statuses_iterations_and_oracle_costs():
    fam, r = cf.family("mixed"), cf.host("mixed")
    assert (fam.n, fam.p, fam.l, fam.q) == (15, 2, 11, [4, 3, 5, 1, 2]) and fam.B == 70
    assert collections.Counter(fam.kind.tolist()) == {0: 50, 4: 10, 5: 10}
    assert np.array_equal(r["status"], fam.kind)
    feas = fam.kind == cf.OPTIMAL
    # members of one wave finish at different iterations: that is what the family is for
    assert sorted(collections.Counter(r["iters"][feas].tolist()).items()) == [(9, 1), (10, 9), (11, 16), (12, 11), (13, 8), (14, 4), (15, 1)]
    assert set(r["iters"][fam.kind == cf.INFEASIBLE]) == {5, 6, 7} and set(r["iters"][fam.kind == cf.DUAL_INFEASIBLE]) == {5}
    assert r["dyn_regs"].max() == 0
    st, pc = cf.oracle_costs("mixed")
    assert all(s == "OPTIMAL" for s, k in zip(st, fam.kind) if k == cf.OPTIMAL)
    assert np.all(np.abs(r["pcost"][feas] - pc[feas]) <= 1e-8 * np.maximum(1.0, np.abs(pc[feas])))
    assert _certified(fam, r) == {}


def test_mixed_family_at_an_iteration_cap_of_eight():
    """what the ladder of further attempts sees (Engine::launch): the certificate members are finished -- with the bits of the uncapped
    run -- and of the feasible members 36 end ITERATION_LIMIT, 14 ALMOST_OPTIMAL, at every regularisation of the ladder"""
    fam, full = cf.family("mixed"), cf.host("mixed")
    for reg in (-1.0, 1e-7, 1e-6):
        r = cf.host("mixed", "seq", 8, reg)
        assert collections.Counter(r["status"].tolist()) == {2: 36, 1: 14, 4: 10, 5: 10}
        assert np.array_equal(r["status"][fam.kind != 0], fam.kind[fam.kind != 0])
    r = cf.host("mixed", "seq", 8, -1.0)
    assert all(cf.same_bits(r, t, full, t) == [] for t in np.nonzero(fam.kind)[0])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_unbounded_members_are_never_mistaken_for_solved(seed):
    """A LIMIT, pinned so that it is known (the seed of the mixed family was not a free choice).  Of seeds 1 .. 40 the host build
    gives every feasible and every infeasible member its intended status, but certifies all ten unbounded members (min -v, v >= 0)
    for seed 34 only: elsewhere most of them end NUMERICAL_ERROR after 26 to 67 iterations, and the oracle ends them
    NUMERICAL_ERROR or ITERATION_LIMIT.  A ray is reported once the iterates have diverged far enough for |Gx + s| / (-c'x) to fall
    under 1e-8, and an infeasible-start method without the self-dual embedding is not sure to get that far -- the same class of limit
    as the exponential cone that has to be entered against its curvature (tests/test_oracle_exp_cone.py).  Asserted: what the
    solver then says is never a solution and never the wrong certificate."""
    fam = cf.mixed(seed)
    r = cf._solve_host(fam, "seq")
    assert np.array_equal(r["status"][fam.kind != cf.DUAL_INFEASIBLE], fam.kind[fam.kind != cf.DUAL_INFEASIBLE])
    unb = r["status"][fam.kind == cf.DUAL_INFEASIBLE]
    assert unb.size == 10 and not np.isin(unb, (cf.OPTIMAL, cf.ALMOST_OPTIMAL, cf.INFEASIBLE)).any()
    assert (unb != cf.DUAL_INFEASIBLE).any()          # (should a later solver certify them all, this pin and its text go)
    assert all(cf.certify(fam, r, t) == [] for t in np.nonzero(r["status"] != cf.NUMERICAL_ERROR)[0])   # what IS claimed holds


def test_chain_family_in_both_elimination_orders():
    fam = cf.family("chain")
    seq, nd = cf.host("chain", "seq"), cf.host("chain", "nd")
    assert (fam.n, fam.B) == (241, 20) and seq["stats"][2] == 1011
    assert fam.G[:, fam.n - 1].nnz + fam.A[:, fam.n - 1].nnz == 143          # the global variable: a KKT row over KK_LONG = 64 terms
    assert seq["stats"][7] > 128 and nd["stats"][7] > 128                    # factor rows over LONG_ITEM = 128 terms: chunked
    assert seq["stats"][4] == 0 and seq["stats"][5] == 145 and nd["stats"][4] == 6 and nd["stats"][5] == 22
    for r in (seq, nd):
        assert (r["status"] == 0).all()
        assert sorted(collections.Counter(r["iters"].tolist()).items()) == [(9, 13), (10, 6), (11, 1)]
        assert r["dyn_regs"].max() == 0
        assert _certified(fam, r) == {}
    assert np.all(np.abs(nd["pcost"] - seq["pcost"]) <= 1e-8 * np.maximum(1.0, np.abs(seq["pcost"])))


def test_softplus_family_has_the_logit_optimum():
    fam, r = cf.family("softplus"), cf.host("softplus")
    assert (r["status"] == 0).all() and set(r["iters"]) == {18, 19, 20}
    assert np.abs(r["x"][:, 0] - fam.f_star).max() <= 2e-6 and np.abs(r["pcost"] - fam.value).max() <= 1e-7
    assert np.allclose(fam.value, -(-fam.t * np.log(-fam.t) + (1 + fam.t) * np.log(1 + fam.t)), rtol=0, atol=1e-12)   # binary entropy of -t
    assert _certified(fam, r) == {}


def test_certify_rejects_what_is_not_certified():
    """the checker itself: a solution pushed off its constraints, a cone vector outside its (degenerate) cone, a status swapped"""
    fam, r = cf.family("mixed"), cf.host("mixed")
    bent = {k: np.array(r[k]) for k in cf.RESULT_KEYS}
    bent["x"][0] += 1e-5                            # primal and dual residual no longer hold, reported numbers no longer match
    assert any(s.startswith("pres") for s in cf.certify(fam, bent, 0)) and any(s.startswith("reported") for s in cf.certify(fam, bent, 0))
    o1 = fam.l + 4 + 3 + 5                       # Q^1: the ray s >= 0
    bent["s"][1, o1] = -1e-13
    assert any("Q^1" in s for s in cf.certify(fam, bent, 1))
    bent["z"][2, o1 + 1 + 1] = 2.0 * abs(bent["z"][2, o1 + 1]) + 1.0        # Q^2: |z_1| <= z_0
    assert any("Q^2" in s for s in cf.certify(fam, bent, 2))
    bent["status"][3], bent["status"][5] = cf.DUAL_INFEASIBLE, cf.INFEASIBLE
    assert cf.certify(fam, bent, 3) and cf.certify(fam, bent, 5)
