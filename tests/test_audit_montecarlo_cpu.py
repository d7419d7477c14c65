"""The Monte-Carlo audit on the host (scp_model_audit_montecarlo_host and scp_mc_draws_host: the bodies the device kernels run,
csrc/audit_kernel.hpp, csrc/mc_kernel.hpp and csrc/mc_rng.hpp) against the CPU reference of tests/montecarlo_util.py: the
generator, the noisy flights and their moments, exactness on a linear model, agreement with the covariance audit, zero sigmas =
the tracking audit, the tree and its padding, failure reporting, and the error codes and exported names that need no device."""
import ctypes

import numpy as np
import pytest

import audit_tracking_util as atu
import audit_util as au
import montecarlo_util as mu

BAD, UNKNOWN, UNSUPPORTED = 1, 2, 7
FIRST3 = au.AUDIT_MODELS[:3]
FLIGHT_CASES = [(n, N, 3, 4) for n in FIRST3 for N in (2, 5)] + [("starship", atu.STARSHIP["N"], 2, atu.STARSHIP["steps"])]
SEED = 2026


def _draws(pkg, seed, kind, k, d, n, want_words=True):
    z, w = np.full(max(n, 1), 7.0), np.zeros(4 * ((max(n, 1) + 1) // 2), dtype=np.uint32)
    rc = pkg._lib.lib().scp_mc_draws_host(seed, kind, k, d, n, au.vp(z), w.ctypes.data if want_words else None)
    return rc, z, w


def _fly(pkg, name, N, s, K, steps, viol_tol, D, seed, sig, moments=True, flights=True, summary=True, stat=True, Su=None):
    xd, ud, p, pp = s["case"]
    nx, nu = xd.shape[1], ud.shape[1]
    out, st = np.full(au.W, 123.0), np.full(mu.SW, 125.0)
    mom, rec = np.full((N, 1 + 2 * nx + nu), 126.0), np.full((max(D, 1), au.W), 124.0)
    rc = pkg._lib.lib().scp_model_audit_montecarlo_host(pkg.models.MODEL_IDS[name], au.vp(au.model_blob(pkg, name, N)), N, au.vp(xd), au.vp(ud),
                                                        au.vp(p) if p.size else None, au.vp(pp), au.vp(s["Sx"]), au.vp(s["Su"] if Su is None else Su),
                                                        au.vp(None if K is None else atu.to_lib(K)), steps, float(viol_tol), D, seed,
                                                        au.vp(sig[0]), au.vp(sig[1]), au.vp(sig[2]), au.vp(out) if summary else None,
                                                        au.vp(st) if stat else None, au.vp(mom) if moments else None,
                                                        au.vp(rec) if flights else None)
    return rc, out, st, mom, rec


def test_generator_known_answers_and_draws(pkg):
    """the util's Philox against the Random123 known answers; the library's words against the util's; its normals to a few ulp"""
    kat = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
    for ctr, key, want in kat:
        assert tuple(mu.philox4x32_10(ctr, key)) == want
        got = mu.philox4x32_10(tuple(np.full(3, c, np.uint64) for c in ctr), tuple(np.full(3, k, np.uint64) for k in key))
        assert all((g == w).all() for g, w in zip(got, want))                       # the array form used by normals_many
    rc, z, w = _draws(pkg, 0, 0, 0, 1, 2)
    assert rc == 0 and tuple(int(v) for v in w) == kat[0][2]
    for seed, kind, k, d, n in ((0, 0, 0, 1, 2), (2026, 1, 3, 2, 4), (2 ** 32 + 5, 2, 9, 65, 7), (2 ** 63 + 12345, 1, 1, 4096, 3),
                                (0xA4093822299F31D0, 0, 0, 130, 8), (1, 2, 2, 1, 1)):
        rc, z, w = _draws(pkg, seed, kind, k, d, n)
        assert rc == 0
        wr = mu.words(seed, kind, k, d, n)
        assert np.array_equal(w.astype(np.uint64), wr), (seed, kind, k, d, n)
        zr = mu.normals(seed, kind, k, d, n)
        assert zr.shape == (n,) and (np.abs(z - zr) <= 1e-14 * np.maximum(1.0, np.abs(zr))).all(), (z, zr)
        rc, z2, _ = _draws(pkg, seed, kind, k, d, n, want_words=False)
        assert rc == 0 and z2.tobytes() == z.tobytes()
        assert np.array_equal(mu.normals_many(seed, kind, k, d, n)[d - 1], zr)
    for bad in ((0, 3, 0, 1, 2), (0, -1, 0, 1, 2), (0, 0, -1, 1, 2), (0, 0, 0, 0, 2), (0, 0, 0, 1, 0)):
        assert _draws(pkg, *bad)[0] == BAD
    assert pkg._lib.lib().scp_mc_draws_host(0, 0, 0, 1, 2, None, None) == BAD


@pytest.mark.parametrize("name,N,D,steps", FLIGHT_CASES)
def test_host_twin_matches_reference(pkg, orc, name, N, D, steps):
    """every flight record, the node records and stat against the numpy flights; the summary is the dispersed fold marked 4.0"""
    s = atu.setup(orc, name, N)
    refs, mom_ref = mu.references(orc, name, N, steps, D, SEED)
    tol = au.choose_viol_tol(refs)
    rc, out, st, mom, rec = _fly(pkg, name, N, s, s["K"], steps, tol, D, SEED, mu.sigmas(s))
    assert rc == 0
    for d, ref in enumerate(refs):
        ref.check_tracking(rec[d], tol, "%s N=%d d=%d" % (name, N, d + 1))
    mu.check_moments(mom, mom_ref, "%s N=%d" % (name, N))
    mu.check_stat(st, mom_ref, s["Sx"], D, "%s N=%d" % (name, N))
    want = atu.fold(rec)
    want[13] = 4.0
    assert out.tobytes() == want.tobytes() and out[14] == float(D) and out[11] == 0.0
    rc, only, st2, _, _ = _fly(pkg, name, N, s, s["K"], steps, tol, D, SEED, mu.sigmas(s), moments=False, flights=False)
    assert rc == 0 and only.tobytes() == out.tobytes() and st2.tobytes() == st.tobytes()


def _linear_setup(orc):
    s = atu.setup(orc, "double_integrator", 9)
    return s, mu.sigmas(s)


def test_linear_exactness(pkg, orc):
    """RK4 is exact for the double integrator under a first-order hold: every flight's node errors obey the linear recursion
    over the oracle's A, B-, B+ with the util's draws (a wrong counter layout, a kick in the wrong place or a disturbance that
    misses the stage times all break this)"""
    name, N, D, steps = "double_integrator", 9, 64, 2
    s, sig = _linear_setup(orc)
    E, U = mu.linear_errors(s["dyn"], s["K"], D, SEED, *sig)
    ref = mu.moments(E, U / s["Su"])
    rc, out, st, mom, rec = _fly(pkg, name, N, s, s["K"], steps, 0.0, D, SEED, sig)
    assert rc == 0 and (rec[:, 11] == 0.0).all()
    nx = 2
    got, want = mom.copy(), ref.copy()
    for a in (got, want):                                   # compare in units of Sx
        a[:, 1:1 + nx] /= s["Sx"]
        a[:, 1 + nx:1 + 2 * nx] /= s["Sx"]
    mu.check_moments(got, want, "linear")
    mu.check_stat(st, ref, s["Sx"], D, "linear")
    # the flights' own [14]: the largest scaled node error of each flight
    track = np.abs(E / s["Sx"]).max(axis=(1, 2))
    assert (np.abs(rec[:, 14] - track) <= au.RTOL * np.maximum(1.0, track)).all()


def test_agreement_with_the_covariance_audit(pkg, orc):
    """D = 4096 on the double integrator: at every (k, i) with sig > 0, |std / sig - 1| <= 5 / sqrt(2 (D - 1)) and
    |mean| <= 5 sig / sqrt(D): five standard errors of a Gaussian sample's sigma and mean, over 18 comparisons.  seed = 2026 was
    confirmed first with the util's linear recursion alone (the first block below, independent of the code under test)."""
    name, N, D, steps = "double_integrator", 9, 4096, 1
    s, sig = _linear_setup(orc)
    nx, nu = 2, 1
    A, Bm, Bp = s["dyn"]
    out, csig = np.zeros(16), np.zeros((N, nx))
    nrow = np.zeros(3, np.int32)
    rc = pkg._lib.lib().scp_covariance_host(nx, nu, N, au.vp(A), au.vp(Bm), au.vp(Bp), au.vp(atu.to_lib(s["K"])), nrow.ctypes.data, None, 0, None,
                                            au.vp(s["Sx"]), au.vp(s["Su"]), au.vp(sig[0]), au.vp(sig[1]), au.vp(sig[2]), 3.0, au.vp(out),
                                            au.vp(csig), None)
    assert rc == 0 and out[0] == 0.0 and (csig > 0.0).all()
    b_std, b_mean = 5.0 / np.sqrt(2.0 * (D - 1)), 5.0 * csig / np.sqrt(D)
    E, U = mu.linear_errors(s["dyn"], s["K"], D, SEED, *sig)
    lin = mu.moments(E, U / s["Su"])
    print("util alone: max |std/sig - 1| %.4f of %.4f, max |mean| / bound %.3f" % (
        np.abs(lin[:, 1 + nx:1 + 2 * nx] / csig - 1).max(), b_std, (np.abs(lin[:, 1:1 + nx]) / b_mean).max()))
    assert (np.abs(lin[:, 1 + nx:1 + 2 * nx] / csig - 1.0) <= b_std).all() and (np.abs(lin[:, 1:1 + nx]) <= b_mean).all(), "the seed itself"
    rc, _, st, mom, _ = _fly(pkg, name, N, s, s["K"], steps, 0.0, D, SEED, sig, flights=False)
    assert rc == 0 and (mom[:, 0] == D).all() and st[7] == D
    ratio = mom[:, 1 + nx:1 + 2 * nx] / csig
    print("twin: max |std/sig - 1| %.4f of %.4f, max |mean| / bound %.3f" % (np.abs(ratio - 1).max(), b_std, (np.abs(mom[:, 1:1 + nx]) / b_mean).max()))
    assert (np.abs(ratio - 1.0) <= b_std).all()
    assert (np.abs(mom[:, 1:1 + nx]) <= b_mean).all()
    # the Python comparison of the two audits gives the same figures
    a = pkg.MonteCarloAuditBatch(np.zeros((1, 16)), st[None], nx, steps, steps * (N - 1) + 1, 0.0, D, SEED, mom[None])
    c = a.compare(pkg.CovarianceAuditBatch(out[None], 3.0, sig=csig[None]))
    assert np.array_equal(c.ratio[0], ratio) and c.ratio_max[0] == ratio.max() and c.ratio_min[0] == ratio.min()
    assert (c.z_mean <= 5.0).all()


@pytest.mark.parametrize("name", au.AUDIT_MODELS)
def test_zero_sigmas_are_the_tracking_flight(pkg, orc, name):
    """all sigmas zero: the flight records are those of scp_model_audit_tracking_host with dx0 = 0, gain 1, bias 0, bit for bit"""
    N, steps = (atu.STARSHIP["N"], atu.STARSHIP["steps"]) if name == "starship" else (5, 4)
    s = atu.setup(orc, name, N)
    xd, ud, p, pp = s["case"]
    nx, nu = xd.shape[1], ud.shape[1]
    zero = (np.zeros(nx), np.zeros(nu), np.zeros(nx))
    rc, out, st, mom, rec = _fly(pkg, name, N, s, s["K"], steps, 0.0, 2, SEED, zero)
    assert rc == 0
    tsum, trec = np.zeros(au.W), np.zeros((2, au.W))
    assert pkg._lib.lib().scp_model_audit_tracking_host(pkg.models.MODEL_IDS[name], au.vp(au.model_blob(pkg, name, N)), None, N, au.vp(xd),
                                                        au.vp(ud), au.vp(p) if p.size else None, au.vp(pp), au.vp(s["Sx"]), au.vp(s["Su"]),
                                                        au.vp(atu.to_lib(s["K"])), steps, 0.0, 2, au.vp(np.zeros((2, nx))), au.vp(np.ones((2, nu))),
                                                        au.vp(np.zeros((2, nu))), au.vp(tsum), au.vp(trec)) == 0
    assert rec.tobytes() == trec.tobytes(), (rec, trec)
    tsum[13] = 4.0
    assert out.tobytes() == tsum.tobytes()
    assert (mom[:, 0] == 2.0).all() and (mom[:, 1 + nx:1 + 2 * nx] == 0.0).all()      # two identical flights: no spread


def test_tree_and_padding(pkg, orc):
    """D = 65 and 130 (a second and a third, partly filled wavefront): a flight depends on d only, every flight counts at every node,
    and the moments are numpy's over the flights' own node errors, recomputed by the reference at D = 65"""
    name, N, steps = "rocket_landing", 5, 4
    s = atu.setup(orc, name, N)
    sig = mu.sigmas(s)
    rc, o64, st64, m64, r64 = _fly(pkg, name, N, s, s["K"], steps, 0.0, 64, SEED, sig)
    assert rc == 0
    for D in (65, 130):
        rc, out, st, mom, rec = _fly(pkg, name, N, s, s["K"], steps, 0.0, D, SEED, sig)
        assert rc == 0 and rec[:64].tobytes() == r64.tobytes() and (mom[:, 0] == D).all() and st[7] == D and out[14] == D
        if D == 65:
            refs, mom_ref = mu.references(orc, name, N, steps, D, SEED)
            mu.check_moments(mom, mom_ref, "D=65")
            mu.check_stat(st, mom_ref, s["Sx"], D, "D=65")
            assert (np.abs(rec[:, 14] - [r.rec[14] for r in refs]) <= au.RTOL).all()


def test_failures_are_reported(pkg, orc):
    """a NaN in K at an interior node: no abort, every flight flagged, n_k = 0 from that node on with NaN moments, stat[7] = 0;
    the next call is untouched"""
    name, N, steps, D = "quadrotor", 5, 2, 3
    s = atu.setup(orc, name, N)
    sig = mu.sigmas(s)
    rc, out0, st0, mom0, rec0 = _fly(pkg, name, N, s, s["K"], steps, 0.0, D, SEED, sig)
    assert rc == 0 and out0[11] == 0.0
    K = s["K"].copy()
    K[2, 1, 3] = np.nan                                     # node 3 of 5
    rc, out, st, mom, rec = _fly(pkg, name, N, s, K, steps, 0.0, D, SEED, sig)
    assert rc == 0 and (rec[:, 11] == 1.0).all() and out[11] == float(D) and out[13] == 4.0
    assert (mom[:2, 0] == D).all() and mom[:2].tobytes() == mom0[:2].tobytes()
    assert (mom[2:, 0] == 0.0).all() and np.isnan(mom[2:, 1:]).all() and st[7] == 0.0
    rc, out1, st1, mom1, rec1 = _fly(pkg, name, N, s, s["K"], steps, 0.0, D, SEED, sig)
    assert rc == 0 and all(a.tobytes() == b.tobytes() for a, b in ((out1, out0), (st1, st0), (mom1, mom0), (rec1, rec0)))


def test_error_codes_and_exports(pkg, orc):
    name, N = "quadrotor", 5
    s = atu.setup(orc, name, N)
    K, sig = s["K"], mu.sigmas(s)
    assert _fly(pkg, name, N, s, K, 1, 0.0, 2, 0, sig)[0] == 0
    assert _fly(pkg, name, N, s, K, 1, 0.0, 1, 0, sig)[0] == BAD                     # D < 2
    assert _fly(pkg, name, N, s, K, 1, 0.0, 0, 0, sig)[0] == BAD
    assert _fly(pkg, name, N, s, K, 0, 0.0, 2, 0, sig)[0] == BAD                     # steps < 1
    assert _fly(pkg, name, N, s, None, 1, 0.0, 2, 0, sig)[0] == BAD                  # the host twin has no resident gains
    assert _fly(pkg, name, N, s, K, 1, 0.0, 2, 0, sig, summary=False)[0] == BAD
    assert _fly(pkg, name, N, s, K, 1, 0.0, 2, 0, sig, stat=False)[0] == BAD
    for i in range(3):
        for spoil in (lambda a: -a, lambda a: a * np.nan, lambda a: a + np.inf, lambda a: None):
            bad = list(sig)
            bad[i] = spoil(bad[i])
            assert _fly(pkg, name, N, s, K, 1, 0.0, 2, 0, bad)[0] == BAD, i
    xd, ud, p, pp = s["case"]
    assert _fly(pkg, name, N, dict(s, case=(xd, ud, np.zeros(0), pp)), K, 1, 0.0, 2, 0, sig)[0] == BAD      # the model has a p
    L = pkg._lib.lib()
    out, st = np.zeros(au.W), np.zeros(mu.SW)
    args = (N, au.vp(xd), au.vp(ud), au.vp(p), au.vp(pp), au.vp(s["Sx"]), au.vp(s["Su"]), au.vp(atu.to_lib(K)), 1, 0.0, 2, 0,
            au.vp(sig[0]), au.vp(sig[1]), au.vp(sig[2]), au.vp(out), au.vp(st), None, None)
    par = au.model_blob(pkg, name, N)
    assert L.scp_model_audit_montecarlo_host(pkg.models.MODEL_IDS[name], au.vp(par), *args) == 0
    assert L.scp_model_audit_montecarlo_host(42, au.vp(par), *args) == UNKNOWN
    ff = np.ones(16 * 16 * N)
    for other in ("freeflyer", "oscillator"):
        assert L.scp_model_audit_montecarlo_host(pkg.models.MODEL_IDS[other], au.vp(np.ones(64)), N, au.vp(ff), au.vp(ff), au.vp(ff), au.vp(ff),
                                                 au.vp(np.ones(16)), au.vp(np.ones(16)), au.vp(ff), 1, 0.0, 2, 0, au.vp(ff), au.vp(ff), au.vp(ff),
                                                 au.vp(out), au.vp(st), None, None) == UNSUPPORTED
    for nm in ("audit_montecarlo", "audit_montecarlo_resident", "MonteCarloAuditBatch"):
        assert callable(getattr(pkg, nm))
    for nm in ("scp_audit_montecarlo_batch_host", "scp_audit_montecarlo_resident", "scp_model_audit_montecarlo_host", "scp_mc_draws_host"):
        assert nm in pkg._lib.EXPORTS and hasattr(L, nm)
    # the batch object from raw arrays: B = 2, N = 3, nx = 2, nu = 1
    raw, stat = np.arange(32.0).reshape(2, 16), np.arange(16.0).reshape(2, 8)
    mom = np.arange(2 * 3 * 6.0).reshape(2, 3, 6) + 1.0
    fl = np.arange(2 * 4 * 16.0).reshape(2, 4, 16)
    a = pkg.MonteCarloAuditBatch(raw, stat, 2, steps=4, res=9, viol_tol=0.5, D=4, seed=7, moments=mom, flights=fl)
    assert isinstance(a, pkg.TrackingAuditBatch) and len(a) == 2 and a.steps == 4 and a.D == 4 and a.seed == 7 and a.seconds == 0.0
    assert a.drift[0] == 8.0 and a.effort[1, 2] == fl[1, 2, 12]
    assert a.std_max[1] == 8.0 and a.std_node[0] == 1.0 and a.std_state[0] == 2.0 and a.mean_max[0] == 3.0 and a.mean_node[0] == 4.0
    assert a.effort_rms_max[0] == 5.0 and a.effort_rms_node[0] == 6.0 and a.n_min[1] == 15.0
    assert a.n.shape == (2, 3) and a.mean.shape == (2, 3, 2) and a.std.shape == (2, 3, 2) and a.effort_rms.shape == (2, 3, 1)
    assert a.n[1, 2] == mom[1, 2, 0] and a.mean[0, 1, 1] == mom[0, 1, 2] and a.std[1, 0, 0] == mom[1, 0, 3] and a.effort_rms[0, 2, 0] == mom[0, 2, 5]
    sig_lin = a.std / 2.0
    sig_lin[0, 0, 0] = 0.0
    c = a.compare(pkg.CovarianceAuditBatch(np.zeros((2, 16)), 3.0, sig=sig_lin))
    assert np.isnan(c.ratio[0, 0, 0]) and np.isnan(c.z_mean[0, 0, 0]) and (c.ratio[1] == 2.0).all() and list(c.ratio_max) == [2.0, 2.0]
    assert list(c.ratio_min) == [2.0, 2.0] and c.z_mean[1, 2, 1] == abs(mom[1, 2, 2]) / (sig_lin[1, 2, 1] / np.sqrt(mom[1, 2, 0]))
    with pytest.raises(ValueError):
        a.compare(pkg.CovarianceAuditBatch(np.zeros((2, 16)), 3.0, sig=sig_lin[:, :2]))
    with pytest.raises(ValueError):
        a.compare(pkg.CovarianceAuditBatch(np.zeros((2, 16)), 3.0))
    b = pkg.MonteCarloAuditBatch(raw, stat, 2, 4, 9, 0.0, 4)
    assert b.moments is None and b.n is None and b.std is None and b.flights is None and b.effort is None
    with pytest.raises(ValueError):
        b.compare(pkg.CovarianceAuditBatch(np.zeros((2, 16)), 3.0, sig=sig_lin))
