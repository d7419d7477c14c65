"""Generic conic solver on the MI355X (-m gpu) in EVERY launch geometry: the eight instantiations conic_ipm_kernel<MAXW, SUB>
(MAXW = 16 | 8 by the waves of a workgroup, SUB = 1 | 4 | 16 | 64 sub-workers per wave, i.e. 64 | 16 | 4 | 1 problems per wave) and two odd
worker counts, forced at small batch sizes through SCP_CONIC_SUB / SCP_CONIC_WAVES / SCP_CONIC_ORDER (read by the engine at every
scp_conic_create).  The program families and their independent references are tests/conic_families.py (pinned on the host build
in tests/test_conic_families_cpu.py):

  a. every geometry against references it shares nothing with: intended statuses, iteration counts of the host build +- 1, costs of
     oracle/ipm.py / closed forms, extended-precision certificates recomputed from the returned x, y, z, s;
  b. batch independence bit for bit where problems share a wave and every control decision is taken for the whole workgroup;
  c. finished members frozen next to the members that the ladder of further attempts re-solves;
  d. shared against per-problem input arrays;
  and the refusal of a sub-worker count for which there is no kernel."""
import numpy as np
import pytest

import conic_families as cf

pytestmark = pytest.mark.gpu

GEOMETRIES = [(sub, waves) for sub in (1, 4, 16, 64) for waves in (16, 8)] + [(4, 3), (64, 3)]
SHARED_WAVE = [g for g in GEOMETRIES if g[0] < 64]
COST_TOL = 1e-8       # both sides stop at a gap of 1e-8 (tests/test_conic_gpu.py::test_random_socps_match_oracle_ipm)


@pytest.fixture(scope="module", autouse=True)
def _references(orc):
    return orc


def batch(pkg, monkeypatch, fam, sub, waves, order=None, capacity=None):
    monkeypatch.setenv("SCP_CONIC_SUB", str(sub))
    monkeypatch.setenv("SCP_CONIC_WAVES", str(waves))
    if order is None:
        monkeypatch.delenv("SCP_CONIC_ORDER", raising=False)
    else:
        monkeypatch.setenv("SCP_CONIC_ORDER", order)
    prog = cf.device_batch(pkg, fam, capacity)
    assert prog.stats()["waves"] == waves
    return prog


def check_against_references(fam, r, ref):
    """(a) for one solved batch; returns (largest iteration difference to the host build, largest relative cost difference to `ref`)"""
    host = cf.host(fam.name, "nd" if ref == "host nd" else "seq")
    assert np.array_equal(r["status"], fam.kind), (r["status"], fam.kind)
    dit = np.abs(r["iters"].astype(int) - host["iters"])
    opt = fam.kind == cf.OPTIMAL
    dcost = 0.0
    if fam.name == "softplus":
        ferr, verr = np.abs(r["x"][:, 0] - fam.f_star).max(), np.abs(r["pcost"] - fam.value).max()
        print("  softplus: |f - f*| %.3e, value error %.3e" % (ferr, verr))
        assert ferr <= 2e-6 and verr <= 1e-7
    else:
        pc = cf.oracle_costs(fam.name)[1] if ref == "oracle" else host["pcost"]
        rel = np.abs(r["pcost"][opt] - pc[opt]) / np.maximum(1.0, np.abs(pc[opt]))
        dcost = rel.max()
    print("  %s vs %s: iteration difference %d, relative cost difference %.3e" % (fam.name, ref, dit.max(), dcost))
    assert dit.max() <= 1, (dit, r["iters"], host["iters"])
    assert dcost <= COST_TOL
    bad = {t: v for t, v in ((t, cf.certify(fam, r, t)) for t in range(fam.B)) if v}
    assert bad == {}
    return int(dit.max()), float(dcost)


CASES = [("mixed", None, "oracle"), ("softplus", None, "closed form"), ("chain", "seq", "host seq"), ("chain", "nd", "host nd")]


@pytest.mark.parametrize("name,order,ref", CASES, ids=["mixed", "softplus", "chain-seq", "chain-nd"])
@pytest.mark.parametrize("sub,waves", GEOMETRIES)
def test_every_geometry_against_independent_references(pkg, monkeypatch, sub, waves, name, order, ref):
    fam = cf.family(name)
    prog = batch(pkg, monkeypatch, fam, sub, waves, order)
    r = cf.device_solve(prog, fam)
    st = prog.stats()
    prog.close()
    print("SUB %d WAVES %d" % (sub, waves))
    if order is not None:
        assert (st["nd_depth"] > 0) if order == "nd" else (st["nd_depth"] == 0)
    assert st["fallback_solves"] == 0        # (every member ends OPTIMAL or with a certificate: nothing for the ladder of further attempts)
    check_against_references(fam, r, ref)


def independence_cases():
    return [(g, nm) for g in SHARED_WAVE for nm in ("mixed", "softplus")] + [((64, 16), "mixed")]


@pytest.mark.parametrize("geometry,name", independence_cases(), ids=lambda v: v if isinstance(v, str) else "%d-%d" % v)
def test_batch_independence_bit_for_bit(pkg, monkeypatch, geometry, name):
    """a member's x, y, z, s, status, iteration count and info entries do not depend on its lane, its workgroup or its neighbours:
    the batch, the batch in reversed order (same handle: the buffers of the other lanes hold the previous run) and single members
    next to 63 padding lanes (a fresh handle)"""
    fam = cf.family(name)
    host = cf.host(name)
    feas = fam.kind == cf.OPTIMAL
    slowest = int(np.argmax(np.where(feas, host["iters"], -1))), int(np.argmin(np.where(feas, host["iters"], 1000)))
    alone = sorted({0, 3, 5} | set(slowest))       # 3: infeasible, 5: unbounded (mixed family)
    prog = batch(pkg, monkeypatch, fam, *geometry)
    fwd = cf.device_solve(prog, fam)
    rev = cf.device_solve(prog, fam, members=np.arange(fam.B)[::-1])
    prog.close()
    one = batch(pkg, monkeypatch, fam, *geometry, capacity=1)
    singles = {t: cf.device_solve(one, fam, members=[t]) for t in alone}
    one.close()
    assert np.array_equal(fwd["status"], fam.kind)
    assert len(set(fwd["iters"][feas])) >= 2          # members of one wave do finish at different iterations
    diff = {t: cf.same_bits(fwd, t, rev, fam.B - 1 - t) for t in range(fam.B)}
    assert {t: v for t, v in diff.items() if v} == {}, "batch against reversed batch"
    diff = {t: cf.same_bits(fwd, t, singles[t], 0) for t in alone}
    assert {t: v for t, v in diff.items() if v} == {}, "batch against single members"


@pytest.mark.parametrize("sub,waves", [(1, 16), (4, 16), (16, 8), (64, 16)])
def test_finished_members_stay_frozen_next_to_resolved_ones(pkg, monkeypatch, sub, waves):
    """max_iter = 8: the 20 certificate members are finished, most feasible members end ITERATION_LIMIT and are re-solved twice by the
    ladder of Engine::launch under its `active` mask (at a cap of 8 they cannot do better) -- in the waves of the finished ones"""
    fam = cf.family("mixed")
    prog = batch(pkg, monkeypatch, fam, sub, waves)
    full = cf.device_solve(prog, fam)
    assert prog.stats()["fallback_solves"] == 0
    capped = cf.device_solve(prog, fam, max_iter=8)
    st = prog.stats()
    prog.close()
    cert = np.nonzero(fam.kind != cf.OPTIMAL)[0]
    assert np.array_equal(full["status"], fam.kind) and np.array_equal(capped["status"][cert], fam.kind[cert])
    diff = {t: cf.same_bits(capped, t, full, t) for t in cert}
    assert {t: v for t, v in diff.items() if v} == {}
    feas = capped["status"][fam.kind == cf.OPTIMAL]
    print("SUB %d WAVES %d cap 8: ALMOST_OPTIMAL %d, ITERATION_LIMIT %d, fallback solves %d" %
          (sub, waves, (feas == 1).sum(), (feas == 2).sum(), st["fallback_solves"]))
    assert np.isin(feas, (cf.ALMOST_OPTIMAL, cf.ITERATION_LIMIT)).all()
    assert st["fallback_solves"] > 0 and st["fallback_solves"] >= (feas == cf.ITERATION_LIMIT).sum()


def test_shared_and_per_problem_inputs_give_the_same_bits(pkg, monkeypatch):
    """70 chain programs (the 20 members repeated: one more than a 64 x 64 tile of the transposes, ragged in both directions) with
    h, Gx, Ax, Px as shared arrays against the same values passed per problem"""
    fam = cf.family("chain")
    B = 70
    idx = np.arange(B) % fam.B
    prog = batch(pkg, monkeypatch, fam, 4, 16, "nd", capacity=B)
    tile = lambda v: np.ascontiguousarray(np.tile(v, (B, 1)))
    per = prog.solve(fam.c[idx], fam.h[idx], b=fam.b[idx], Gx=tile(fam.G.data), Ax=tile(fam.A.data), Px=tile(fam.P.data))
    shr = prog.solve(fam.c[idx], fam.h[0], b=fam.b[idx], Gx=fam.G.data, Ax=fam.A.data, Px=fam.P.data, shared=("h", "Gx", "Ax", "Px"))
    prog.close()
    assert np.array_equal(fam.h, np.tile(fam.h[0], (fam.B, 1)))
    assert (per["status"] == 0).all()
    diff = {t: cf.same_bits(per, t, shr, t) for t in range(B)}
    assert {t: v for t, v in diff.items() if v} == {}, "shared against per-problem arrays"
    diff = {t: cf.same_bits(per, t, per, t - fam.B) for t in range(fam.B, B)}
    assert {t: v for t, v in diff.items() if v} == {}, "same data in another lane / workgroup"
    host = cf.host("chain", "nd")
    assert np.all(np.abs(per["pcost"] - host["pcost"][idx]) <= COST_TOL * np.maximum(1.0, np.abs(host["pcost"][idx])))


@pytest.mark.parametrize("sub", [2, 3, 8, 32, 65, 128])
def test_a_sub_worker_count_without_a_kernel_is_refused_at_create(pkg, monkeypatch, sub):
    """launch_one has SUB = 1, 4, 16, 64 only: SCP_CONIC_SUB = 2 used to run the SUB = 64 kernel on a grid sized for 32 problems
    per workgroup, solve one problem in 32 and report nothing"""
    fam = cf.family("softplus")
    monkeypatch.setenv("SCP_CONIC_SUB", str(sub))
    with pytest.raises(pkg._lib.ScpError) as e:
        cf.device_batch(pkg, fam)
    assert e.value.code == 1          # SCP_ERR_BAD_ARGUMENT
