"""Which models and which (nx, nu) pairs the audit family accepts, asked of the library alone: every host twin of the audit kernel
units (audit_api, lqr_api, cov_api, mc_api) refuses exactly the models with node parameters (scp_model_query: np_node > 0) and the
dimension pairs of no auditable model, and reports an unknown id as such.  Tiny arrays of the documented sizes, N = 2; no device."""
import ctypes

import numpy as np
import pytest

import audit_util as au

OK, UNKNOWN, UNSUPPORTED = 0, 2, 7
N, D = 2, 2
IDS = range(6)


def _info(pkg, mid):
    info = pkg._lib.ScpModelInfo()
    assert pkg._lib.lib().scp_model_query(mid, ctypes.byref(info)) == OK
    return info


def _ones(*shape):
    return np.ones(shape)


def _chains(pkg, nx, nu):
    """(rc of scp_lqr_gains_host, rc of scp_covariance_host) on an identity discretisation without rows"""
    L = pkg._lib.lib()
    A = np.ascontiguousarray(np.eye(nx).reshape(1, nx, nx).repeat(N - 1, 0))
    Bm, Bp, K = _ones(N - 1, nu, nx) * 0.1, _ones(N - 1, nu, nx) * 0.1, np.zeros((N - 1, nx, nu))
    info, none = np.zeros(8), np.zeros(3, np.int32)
    gains = L.scp_lqr_gains_host(nx, nu, N, au.vp(A), au.vp(Bm), au.vp(Bp), au.vp(_ones(nx)), au.vp(_ones(nu)), au.vp(_ones(nx)), au.vp(K),
                                 au.vp(info))
    summary = np.zeros(64)
    cov = L.scp_covariance_host(nx, nu, N, au.vp(A), au.vp(Bm), au.vp(Bp), au.vp(np.zeros((N - 1, nx, nu))), none.ctypes.data, None, 0, None,
                                au.vp(_ones(nx)), au.vp(_ones(nu)), au.vp(_ones(nx) * 0.01), au.vp(_ones(nu) * 0.01), au.vp(_ones(nx) * 0.01),
                                3.0, au.vp(summary), None, None)
    return gains, cov


def _model_twins(pkg, mid, info):
    """{entry point: rc} of the six model-level host twins on a constant trajectory of the model's sizes"""
    L = pkg._lib.lib()
    nx, nu, nrow = info.nx, info.nu, info.ns + info.nl + info.nsoc
    names = {v: k for k, v in pkg.models.MODEL_IDS.items()}
    par = au.vp(au.model_blob(pkg, names[mid], N)) if mid in names else au.vp(_ones(64))
    xd, ud, p, pp = _ones(N, nx), _ones(N, nu), _ones(info.np + info.np_node * N + 1), _ones(info.npp + 1)
    Sx, Su, K = _ones(nx), _ones(nu), np.zeros((N - 1, nx, nu))
    rec, sig = np.zeros(64), [au.vp(_ones(nx) * 0.01), au.vp(_ones(nu) * 0.01), au.vp(_ones(nx) * 0.01)]
    args = (au.vp(xd), au.vp(ud), au.vp(p), au.vp(pp))
    return {
        "audit": L.scp_model_audit_host(mid, par, N, *args, au.vp(Sx), 2, 0.0, au.vp(rec)),
        "intervals": L.scp_model_audit_intervals_host(mid, par, N, 0, *args, au.vp(Sx), 2, 0.0, au.vp(rec), None),
        "dispersed": L.scp_model_audit_dispersed_host(mid, par, None, N, *args, au.vp(Sx), 2, 0.0, D, None, None, None, au.vp(rec), None),
        "tracking": L.scp_model_audit_tracking_host(mid, par, None, N, *args, au.vp(Sx), au.vp(Su), au.vp(K), 1, 0.0, D, None, None, None,
                                                    au.vp(rec), None),
        "covariance rows": L.scp_model_covariance_rows_host(mid, par, N, *args, au.vp(K), au.vp(np.zeros((N, nrow + 1, nx + 1))),
                                                            au.vp(np.zeros((info.ntc + 1, nx)))),
        "montecarlo": L.scp_model_audit_montecarlo_host(mid, par, N, *args, au.vp(Sx), au.vp(Su), au.vp(K), 1, 0.0, D, 7, *sig, au.vp(rec),
                                                        au.vp(np.zeros(64)), None, None),
    }


@pytest.mark.parametrize("mid", IDS)
def test_node_parameters_decide(pkg, mid):
    """the chains by the model's (nx, nu) and the six model-level twins: SCP_OK without node parameters, SCP_ERR_UNSUPPORTED with"""
    info = _info(pkg, mid)
    want = OK if info.np_node == 0 else UNSUPPORTED
    assert _chains(pkg, info.nx, info.nu) == (want, want)
    assert _model_twins(pkg, mid, info) == dict.fromkeys(("audit", "intervals", "dispersed", "tracking", "covariance rows", "montecarlo"), want)


@pytest.mark.parametrize("mid", (-1, 6))
def test_unknown_model(pkg, mid):
    info = _info(pkg, 1)      # sizes of any model: the refusal touches no array
    assert _model_twins(pkg, mid, info) == dict.fromkeys(("audit", "intervals", "dispersed", "tracking", "covariance rows", "montecarlo"), UNKNOWN)


def test_dimension_pair_of_no_model(pkg):
    assert all((m.nx, m.nu) != (3, 2) for m in (_info(pkg, i) for i in IDS))
    assert _chains(pkg, 3, 2) == (UNSUPPORTED, UNSUPPORTED)
