"""The audit family on a solved batch (include/scp_mi355x.h, scp_audit_* and scp_lqr_gains_*): the continuous-time audit, its
interval-parallel and dispersed variants, LQR gains with the closed-loop tracking audit, the covariance and the Monte-Carlo audit.
Every audit comes as a pair: `name(sol, pbm, ...)` for a batch given on the host and `name_resident(pbm, ...)` for the batch a run
left in the handle.  The two differ only in where the batch comes from (`_host_batch`, `_resident_batch`) and in what happens to
the rows afterwards (`_finish`).  Array convention as in scp.py."""
import collections
import ctypes

import numpy as np

from . import _lib
from .scp import _ptr

AUDIT_WIDTH = 16      # SCP_AUDIT_WIDTH
_AUDIT_FIELDS = ("s_max", "t_s", "lin_max", "t_lin", "soc_max", "t_soc", "par_max", "bc_tc", "drift", "cost", "n_viol", "nonfinite")

# The batch of one call: the entry point of the library that takes it, its size, the rows the output arrays need, the leading
# arguments after the handle (a pointer made by `_ptr` keeps its array alive) and, for a host batch, the solution it was made from.
_Batch = collections.namedtuple("_Batch", "entry B rows lead sol")


def _host_batch(entry, sol, pbm, pp=None, with_pp=True):
    """`sol` (xd[B,N,nx], ud[B,N,nu], p[B,np]) and pp[B,npp] (None = the nominal problem for all) as the arguments B, xd, ud, p
    and, unless with_pp is False, pp of a *_batch_host entry point; NULL where the model has no p or no pp"""
    xd, ud, p = (np.ascontiguousarray(a, dtype=np.float64) for a in (sol.xd, sol.ud, sol.p))
    B = xd.shape[0]
    lead = [B, _ptr(xd), _ptr(ud), _ptr(p) if pbm.np > 0 else None]
    if with_pp:
        pp = np.ascontiguousarray(np.tile(pbm.traj.mdl.nominal_pp()[None], (B, 1)) if pp is None else pp, dtype=np.float64)
        assert pp.shape[0] == B
        lead.append(_ptr(pp) if pbm.info.npp > 0 else None)
    return _Batch(entry, B, B, lead, sol)


def _resident_batch(entry, pbm):
    """the batch the run started through this package left in the handle (`pbm.resident_B`), refused in the name of `entry`.
    The library writes the records of ITS batch, at most batch_capacity of them: room for all, whatever this module believes"""
    B = getattr(pbm, "resident_B", None)
    if B is None:
        raise _lib.ScpError(1, "%s: no run has been started on this problem" % entry[len("scp_"):])
    return _Batch(entry, B, max(pbm.batch_capacity, B), [], None)


def _call(pbm, batch, *args):
    """the batch's entry point on the problem's handle: the batch, then `args`; its last argument, the device seconds, is returned"""
    sec = ctypes.c_double(0.0)
    _lib.check(getattr(_lib.lib(), batch.entry)(pbm.handle, *batch.lead, *args, ctypes.byref(sec)), pbm.handle)
    return sec.value


def _mask_failed(sol, *arrays):
    """NaN in the rows of the problems whose `sol.status` is not SCP_SOLVED (as in `continuous_time`); None entries are ignored"""
    status = getattr(sol, "status", None)
    if status is not None:
        bad = ~np.array([str(st).startswith("SCP_SOLVED") for st in status])
        for a in arrays:
            if a is not None:
                a[bad] = np.nan


def _finish(batch, *arrays):
    """the output arrays of a call as they are returned: a host batch masked by its status, a resident one cut to its B rows"""
    if batch.sol is None:
        return tuple(None if a is None else a[:batch.B].copy() for a in arrays)
    _mask_failed(batch.sol, *arrays)
    return arrays


class AuditBatch:
    """The records of the continuous-time audit (scp_audit_batch_host / scp_audit_resident, include/scp_mi355x.h) of a batch as
    named arrays [B]: s_max / lin_max / soc_max = the worst value over the samples of the non-convex constraints s, of the linear
    rows and of the second-order cones of X and U (t_s / t_lin / t_soc: the sample time where it is attained), par_max = the
    parameter-only rows, bc_tc = the open-loop residual of the terminal condition, drift = the scaled distance of the flown end
    point from the discrete one, cost = the cost flown, n_viol = samples above viol_tol, nonfinite = 1 where something was not
    finite.  Problems that were skipped (failed) hold NaN everywhere.  `raw` is the [B, 16] array itself."""

    def __init__(self, raw, res, viol_tol):
        self.raw = np.ascontiguousarray(raw, dtype=np.float64).reshape(-1, AUDIT_WIDTH)
        self.res, self.viol_tol = int(res), float(viol_tol)
        for j, name in enumerate(_AUDIT_FIELDS):
            setattr(self, name, self.raw[:, j])

    def __len__(self):
        return self.raw.shape[0]

    @property
    def skipped(self):
        return np.isnan(self.raw[:, 12])

    def summary(self, tol_con, tol_bc):
        """counts of instances per criterion: constraints (all four families <= tol_con over the whole flight), arrival
        (bc_tc <= tol_bc), both, and the instances that were skipped or not finite"""
        live = ~self.skipped & (self.nonfinite == 0)
        with np.errstate(invalid="ignore"):
            con = live & (np.maximum.reduce([self.s_max, self.lin_max, self.soc_max, self.par_max]) <= tol_con)
            bc = live & (self.bc_tc <= tol_bc)
        n = len(self)
        return dict(total=n, skipped=int(self.skipped.sum()), nonfinite=int((~self.skipped & (self.nonfinite != 0)).sum()),
                    constraints_pass=int(con.sum()), constraints_fail=int((live & ~con).sum()),
                    arrival_pass=int(bc.sum()), arrival_fail=int((live & ~bc).sum()),
                    all_pass=int((con & bc).sum()), any_fail=int((live & ~(con & bc)).sum()))


def _audit_res(pbm, res):
    return 2 * pbm.pars.Nsub * (pbm.pars.N - 1) if res is None else int(res)      # the rule of SCPSolution(history), scp.jl:227


def _audit(pbm, batch, res, viol_tol):
    res = _audit_res(pbm, res)
    out = np.zeros((batch.rows, AUDIT_WIDTH))
    sec = _call(pbm, batch, res, float(viol_tol), _ptr(out))
    a = AuditBatch(*_finish(batch, out), res, viol_tol)
    a.seconds = sec
    return a


def audit(sol, pbm, pp=None, res=None, viol_tol=0.0):
    """Continuous-time audit of the batch solution `sol` (xd[B,N,nx], ud[B,N,nu], p[B,np]; pp[B,npp] the per-problem data,
    None = the nominal problem) on the device, fused into the propagation (scp_audit_batch_host): no sample of xc comes back.
    The C entry point takes no mask: every trajectory given is flown, and the records of failed problems (a `status` that is
    not SCP_SOLVED, as in `continuous_time`) are set to NaN HERE, after the call -- drop them from `sol` beforehand to save
    their time (`audit_resident` skips them in the kernel).  Like `propagate` the call stages its input in the handle's
    solution buffers.  Returns an AuditBatch."""
    return _audit(pbm, _host_batch("scp_audit_batch_host", sol, pbm, pp), res, viol_tol)


def audit_resident(pbm, res=None, viol_tol=0.0):
    """The same for the batch RESIDENT in the handle after (or during) a run of any loop family (scp_audit_resident): the
    trajectories that run's get_host would return, its own pp, failed problems skipped by the kernel; 16 doubles per problem
    come back and the run is left untouched.  The batch size is the one the run was started with through this package
    (PTR.upload / PTR.solve, SCvx.solve, GuSTO.solve: `pbm.resident_B`).  Returns an AuditBatch."""
    return _audit(pbm, _resident_batch("scp_audit_resident", pbm), res, viol_tol)


AUDIT_INTERVAL_WIDTH = 16      # SCP_AUDIT_INTERVAL_WIDTH


class IntervalAuditBatch(AuditBatch):
    """The interval-parallel (multiple-shooting) audit of a batch (scp_audit_intervals_batch_host / scp_audit_intervals_resident):
    every interval flown from its own node.  An AuditBatch of the summary records -- there `drift` holds the LARGEST per-interval
    defect, also available as `defect` -- plus `intervals` [B, N-1, 16], the per-interval records (None when they were not
    asked for), `worst_interval` [B] = the 1-based interval of the largest defect (-1 for skipped problems) and `sub`, the
    samples per interval."""

    def __init__(self, raw, res, viol_tol, sub, intervals=None):
        super().__init__(raw, res, viol_tol)
        self.sub = int(sub)
        self.intervals = None if intervals is None else np.ascontiguousarray(intervals, dtype=np.float64)
        self.defect = self.raw[:, 8]
        self.worst_interval = np.where(np.isnan(self.raw[:, 12]), -1.0, self.raw[:, 12]).astype(np.int64)


def _interval_sub(N, res):
    return max(2, -(-int(res) // (N - 1)))


def _audit_intervals(pbm, batch, res, viol_tol, intervals):
    N = pbm.pars.N
    res = _audit_res(pbm, res)
    out = np.zeros((batch.rows, AUDIT_WIDTH))
    recs = np.zeros((batch.rows, N - 1, AUDIT_INTERVAL_WIDTH)) if intervals else None
    sec = _call(pbm, batch, res, float(viol_tol), _ptr(out), _ptr(recs))
    out, recs = _finish(batch, out, recs)
    a = IntervalAuditBatch(out, res, viol_tol, _interval_sub(N, res), recs)
    a.seconds = sec
    return a


def audit_intervals(sol, pbm, pp=None, res=None, viol_tol=0.0, intervals=True):
    """Interval-parallel audit of the batch solution `sol` (scp_audit_intervals_batch_host): like `audit`, but every interval
    restarts from its own node (FOH and IMPULSE handles), one device thread per (problem, interval).  `intervals=False` leaves
    the per-interval records on the device (128 (N-1) bytes per problem).  `sol.status` masks as in `audit`.  Returns an
    IntervalAuditBatch."""
    return _audit_intervals(pbm, _host_batch("scp_audit_intervals_batch_host", sol, pbm, pp), res, viol_tol, intervals)


def audit_intervals_resident(pbm, res=None, viol_tol=0.0, intervals=True):
    """The same for the batch RESIDENT in the handle (scp_audit_intervals_resident): the trajectories the owning run's get_host
    would return, its own pp, failed problems skipped by the kernels; the run is left untouched.  Returns an
    IntervalAuditBatch."""
    return _audit_intervals(pbm, _resident_batch("scp_audit_intervals_resident", pbm), res, viol_tol, intervals)


DISP_SHARED = 1      # SCP_DISP_SHARED
_DISPERSED_FIELDS = ("s_max", "flight_s", "lin_max", "flight_lin", "soc_max", "flight_soc", "par_max", "bc_tc", "drift", "cost_mean",
                     "n_violating", "n_nonfinite", "flight_bc")


class DispersedAuditBatch:
    """The dispersed-flight audit of a batch (scp_audit_dispersed_batch_host / scp_audit_dispersed_resident, include/scp_mi355x.h):
    every problem flown `D` times off-nominal.  Named views [B] of the summary records: s_max / lin_max / soc_max = the worst
    value over the counted flights (flight_s / flight_lin / flight_soc: the 1-based flight attaining it, 0 when no value is finite),
    par_max, bc_tc and drift = the largest over the flights (flight_bc: the flight of bc_tc), cost_mean and cost_max,
    n_violating = flights with samples above viol_tol, n_nonfinite = flights that were not finite (they take no part in any other
    field).  Skipped (failed) problems hold NaN everywhere.  `raw` is the [B, 16] array itself; `flights` [B, D, 16] holds the
    single-shooting record of every flight when they were asked for, else None."""

    def __init__(self, raw, res, viol_tol, D, flights=None):
        self.raw = np.ascontiguousarray(raw, dtype=np.float64).reshape(-1, AUDIT_WIDTH)
        self.res, self.viol_tol, self.D = int(res), float(viol_tol), int(D)
        for j, name in enumerate(_DISPERSED_FIELDS):
            setattr(self, name, self.raw[:, j])
        self.cost_max = self.raw[:, 15]
        self.flights = None if flights is None else np.ascontiguousarray(flights, dtype=np.float64).reshape(len(self), self.D, AUDIT_WIDTH)
        self.seconds = 0.0

    def __len__(self):
        return self.raw.shape[0]

    @property
    def skipped(self):
        return np.isnan(self.raw[:, 13])

    def flight_batch(self, b):
        """the D flights of problem b as an AuditBatch (needs flights=True)"""
        if self.flights is None:
            raise ValueError("the flight records were not asked for (flights=True)")
        return AuditBatch(self.flights[b], self.res, self.viol_tol)


def _dispersed_args(pbm, B, dx0, ugain, ubias, shared, model):
    """the three dispersion arrays as [B, D, n] ([D, n] when shared) C arrays (None stays None), D, the flags and par_true"""
    arrs, D = [], None
    for a, n in ((dx0, pbm.nx), (ugain, pbm.nu), (ubias, pbm.nu)):
        if a is not None:
            a = np.ascontiguousarray(a, dtype=np.float64)
            want = (a.shape[-2] if a.ndim >= 2 else 0, n) if shared else (B, a.shape[-2] if a.ndim >= 2 else 0, n)
            if a.shape != want:
                raise ValueError("dispersion array of shape %s, expected %s" % (a.shape, "[D, %d]" % n if shared else "[%d, D, %d]" % (B, n)))
            if D is not None and a.shape[-2] != D:
                raise ValueError("the dispersion arrays disagree on the number of flights")
            D = a.shape[-2]
        arrs.append(a)
    par_true = None
    if model is not None:
        mdl = pbm.traj.mdl
        true = type(mdl)(**{**mdl.opts, **model}) if isinstance(model, dict) else model
        if type(true) is not type(mdl):
            raise ValueError("the truth model is a %s, the problem's model a %s" % (type(true).__name__, type(mdl).__name__))
        if hasattr(true, "bind"):
            true.bind(pbm.pars)      # models whose constraints depend on the grid (Starship: phase-switch node)
        par_true = np.ascontiguousarray(true.par(), dtype=np.float64)
        assert par_true.size == pbm.info.npar
    return arrs, (1 if D is None else D), (DISP_SHARED if shared else 0), par_true


def _audit_flights(pbm, batch, lead, viol_tol, disp, flights):
    """The call of a D-flight audit (dispersed, tracking): `lead` holds the arguments between the batch and viol_tol, `disp` those
    of `_dispersed_args` after B.  Returns summary [B, 16], the flight records [B, D, 16] or None, D and the device seconds."""
    (dx0, ugain, ubias), D, flags, par_true = _dispersed_args(pbm, batch.B, *disp)
    out = np.zeros((batch.rows, AUDIT_WIDTH))
    recs = np.zeros((batch.rows, D, AUDIT_WIDTH)) if flights else None
    sec = _call(pbm, batch, *lead, float(viol_tol), D, _ptr(dx0), _ptr(ugain), _ptr(ubias), flags, _ptr(par_true), _ptr(out),
                _ptr(recs))
    out, recs = _finish(batch, out, recs)
    return out, recs, D, sec


def _audit_dispersed(pbm, batch, disp, res, viol_tol, flights):
    res = _audit_res(pbm, res)
    out, recs, D, sec = _audit_flights(pbm, batch, (res,), viol_tol, disp, flights)
    a = DispersedAuditBatch(out, res, viol_tol, D, recs)
    a.seconds = sec
    return a


def audit_dispersed(sol, pbm, dx0=None, ugain=None, ubias=None, shared=False, model=None, pp=None, res=None, viol_tol=0.0, flights=False):
    """Dispersed-flight audit of the batch solution `sol` (scp_audit_dispersed_batch_host): every problem is flown D times by the
    single-shooting audit, flight d starting at xd[:, 0] + dx0[b, d] (physical units) and flying ugain[b, d] * u(t) + ubias[b, d]
    -- arrays [B, D, nx] and [B, D, nu], or [D, .] with shared=True (every problem flies the same dispersions); None = 0, 1, 0,
    and D = 1 when all three are None.  `model` = the truth model the flights are flown with: a model instance of the problem's
    kind or a dict of constant overrides (None: the problem's own constants).  flights=True also returns the record of every
    flight.  `sol.status` masks as in `audit`.  Returns a DispersedAuditBatch."""
    return _audit_dispersed(pbm, _host_batch("scp_audit_dispersed_batch_host", sol, pbm, pp), (dx0, ugain, ubias, shared, model), res,
                            viol_tol, flights)


def audit_dispersed_resident(pbm, dx0=None, ugain=None, ubias=None, shared=False, model=None, res=None, viol_tol=0.0, flights=False):
    """The same for the batch RESIDENT in the handle (scp_audit_dispersed_resident): the trajectories the owning run's get_host
    would return, its own pp, failed problems skipped by the kernels; the run is left untouched.  Returns a
    DispersedAuditBatch."""
    return _audit_dispersed(pbm, _resident_batch("scp_audit_dispersed_resident", pbm),
                            (dx0, ugain, ubias, shared, model), res, viol_tol, flights)


LQR_INFO_WIDTH = 4      # SCP_LQR_INFO_WIDTH


class GainBatch:
    """Time-varying LQR gains of a batch (scp_lqr_gains_batch_host / scp_lqr_gains_resident, include/scp_mi355x.h): `K`
    [B, N-1, nu, nx], the hold of interval k is du = -K[b, k] (x - xd[b, k]); `failed` [B] = a pivot <= 0 or a non-finite value
    (the K of that problem is NaN), `k_max` = the largest |K| entry, `trace_p` = the trace of the cost-to-go at the first node.
    Skipped (failed SCP) problems hold NaN everywhere.  `raw` [B, N-1, nx, nu] is the library's own layout, `info` [B, 4]."""

    def __init__(self, raw, info, qx, ru, qf):
        self.raw = np.ascontiguousarray(raw, dtype=np.float64)
        assert self.raw.ndim == 4
        self.K = self.raw.transpose(0, 1, 3, 2)
        self.info = np.ascontiguousarray(info, dtype=np.float64).reshape(-1, LQR_INFO_WIDTH)
        assert self.info.shape[0] == self.raw.shape[0]
        self.qx, self.ru, self.qf = (np.asarray(a, dtype=np.float64) for a in (qx, ru, qf))
        self.k_max, self.trace_p = self.info[:, 1], self.info[:, 2]
        self.seconds = 0.0

    def __len__(self):
        return self.raw.shape[0]

    @property
    def failed(self):
        return self.info[:, 0] == 1.0

    @property
    def skipped(self):
        return np.isnan(self.info[:, 0])


def _lqr_weights(pbm, qx, ru, qf):
    """Bryson's rule from the handle's scaling where a weight is None: qx = 1 / Sx^2, ru = 1 / Su^2, qf = 10 / Sx^2"""
    qx = 1.0 / pbm.scale.Sx ** 2 if qx is None else qx
    ru = 1.0 / pbm.scale.Su ** 2 if ru is None else ru
    qf = 10.0 / pbm.scale.Sx ** 2 if qf is None else qf
    qx, ru, qf = (np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (qx, ru, qf))
    if qx.size != pbm.nx or qf.size != pbm.nx or ru.size != pbm.nu:
        raise ValueError("qx and qf hold nx = %d weights, ru nu = %d" % (pbm.nx, pbm.nu))
    return qx, ru, qf


def _lqr_gains(pbm, batch, qx, ru, qf):
    qx, ru, qf = _lqr_weights(pbm, qx, ru, qf)
    raw, info = np.zeros((batch.rows, pbm.pars.N - 1, pbm.nx, pbm.nu)), np.zeros((batch.rows, LQR_INFO_WIDTH))
    sec = _call(pbm, batch, _ptr(qx), _ptr(ru), _ptr(qf), _ptr(raw), _ptr(info))
    g = GainBatch(*_finish(batch, raw, info), qx, ru, qf)
    g.seconds = sec
    return g


def lqr_gains(sol, pbm, qx=None, ru=None, qf=None):
    """Sample-and-hold LQR tracking gains about the batch solution `sol` (scp_lqr_gains_batch_host): discretize! about it and the
    discrete Riccati recursion on the device.  qx[nx], ru[nu], qf[nx] weigh state, input and final state in physical units
    (None: Bryson's rule from the problem's scaling).  The gains also stay resident in the handle for `audit_tracking`.
    `sol.status` masks as in `audit`.  Returns a GainBatch."""
    return _lqr_gains(pbm, _host_batch("scp_lqr_gains_batch_host", sol, pbm, with_pp=False), qx, ru, qf)


def lqr_gains_resident(pbm, qx=None, ru=None, qf=None):
    """The same about the batch RESIDENT in the handle (scp_lqr_gains_resident): the trajectories the owning run's get_host would
    return, failed problems NaN; the run is left untouched.  Returns a GainBatch."""
    return _lqr_gains(pbm, _resident_batch("scp_lqr_gains_resident", pbm), qx, ru, qf)


class TrackingAuditBatch(DispersedAuditBatch):
    """The closed-loop tracking audit of a batch (scp_audit_tracking_batch_host / scp_audit_tracking_resident): a
    DispersedAuditBatch whose flights were flown with `steps` RK4 steps per interval under sample-and-hold feedback.  Where the
    flight records are present, views [B, D] of them: `effort` = the largest ||Su^-1 du||_inf over the hold updates and
    `effort_node` the 1-based node of it, `track_err` = the largest ||Sx^-1 (x(t_k) - xd[:, k])||_inf over the nodes and
    `track_node` its node; None otherwise."""

    def __init__(self, raw, steps, res, viol_tol, D, flights=None):
        super().__init__(raw, res, viol_tol, D, flights)
        self.steps = int(steps)
        views = ("effort", "effort_node", "track_err", "track_node")
        for j, name in enumerate(views):
            setattr(self, name, None if self.flights is None else self.flights[:, :, 12 + j])


def _tracking_steps(pbm, steps):
    N = pbm.pars.N
    steps = -(-(_audit_res(pbm, None) - 1) // (N - 1)) if steps is None else int(steps)
    return steps, steps * (N - 1) + 1


def _tracking_gains(pbm, B, gains):
    """None (the gains resident in the handle), a GainBatch or an array [B, N-1, nu, nx] -> the library's layout or None"""
    if gains is None:
        return None
    K = gains.K if isinstance(gains, GainBatch) else np.asarray(gains, dtype=np.float64)
    if K.shape != (B, pbm.pars.N - 1, pbm.nu, pbm.nx):
        raise ValueError("gains of shape %s, expected %s" % (K.shape, (B, pbm.pars.N - 1, pbm.nu, pbm.nx)))
    return np.ascontiguousarray(K.transpose(0, 1, 3, 2))


def _audit_tracking(pbm, batch, gains, steps, res, disp, viol_tol, flights):
    out, recs, D, sec = _audit_flights(pbm, batch, (_ptr(_tracking_gains(pbm, batch.B, gains)), steps), viol_tol, disp, flights)
    a = TrackingAuditBatch(out, steps, res, viol_tol, D, recs)
    a.seconds = sec
    return a


def audit_tracking(sol, pbm, gains=None, steps=None, dx0=None, ugain=None, ubias=None, shared=False, model=None, pp=None, viol_tol=0.0,
                   flights=False):
    """Closed-loop tracking audit of the batch solution `sol` (scp_audit_tracking_batch_host): `audit_dispersed` with the loop
    closed.  `gains` = a GainBatch, an array [B, N-1, nu, nx], or None for the gains the last `lqr_gains` call on this problem left
    in the handle; `steps` = RK4 steps per interval (None: ceil((default res - 1) / (N - 1))).  At every node k the hold
    du = -K_k (x - xd[:, k]) is renewed; the flown input is ugain * (u(t) + du) + ubias.  The other arguments are those of
    `audit_dispersed`.  Returns a TrackingAuditBatch."""
    return _audit_tracking(pbm, _host_batch("scp_audit_tracking_batch_host", sol, pbm, pp), gains, *_tracking_steps(pbm, steps),
                           (dx0, ugain, ubias, shared, model), viol_tol, flights)


def audit_tracking_resident(pbm, gains=None, steps=None, dx0=None, ugain=None, ubias=None, shared=False, model=None, viol_tol=0.0,
                            flights=False):
    """The same for the batch RESIDENT in the handle (scp_audit_tracking_resident), with `gains` None = those of the last
    `lqr_gains_resident`; the run is left untouched.  Returns a TrackingAuditBatch."""
    return _audit_tracking(pbm, _resident_batch("scp_audit_tracking_resident", pbm), gains,
                           *_tracking_steps(pbm, steps), (dx0, ugain, ubias, shared, model), viol_tol, flights)


COV_WIDTH, COV_NODE_WIDTH = 16, 8      # SCP_COV_WIDTH, SCP_COV_NODE_WIDTH
_COV_FIELDS = (None, "sigma_max", "sigma_node", "sigma_state", "effort", "effort_node", "margin_s", "margin_s_node", "margin_lin",
               "margin_lin_node", "margin_soc", "margin_soc_node", "terminal_sigma", "trace_final", "n_below")


class CovarianceAuditBatch:
    """The closed-loop covariance audit of a batch (scp_audit_covariance_batch_host / scp_audit_covariance_resident,
    include/scp_mi355x.h).  Named views [B] of the summary records: sigma_max = the largest state 1-sigma in units of Sx with its
    1-based sigma_node and sigma_state, effort = the largest 1-sigma feedback effort in units of Su and effort_node, margin_s /
    margin_lin / margin_soc = the smallest distance of a row of that family from its boundary in sigmas and margin_*_node
    (+Inf and 0 without rows), terminal_sigma = the largest 1-sigma of the terminal conditions, trace_final =
    trace(Sx^-1 Sigma_N Sx^-1), n_below = the (node, row) pairs with a margin below `nsig`.  `failed` [B] = something was not
    finite (the other fields are NaN); skipped (failed SCP) problems hold NaN everywhere.  `raw` is the [B, 16] array itself;
    `sig` [B, N, nx] and `nodes` [B, N, 8] hold the state 1-sigma values and the per-node records when they were asked for, else
    None."""

    def __init__(self, raw, nsig, sig=None, nodes=None):
        self.raw = np.ascontiguousarray(raw, dtype=np.float64).reshape(-1, COV_WIDTH)
        self.nsig = float(nsig)
        for j, name in enumerate(_COV_FIELDS):
            if name is not None:
                setattr(self, name, self.raw[:, j])
        self.sig = None if sig is None else np.ascontiguousarray(sig, dtype=np.float64)
        self.nodes = None if nodes is None else np.ascontiguousarray(nodes, dtype=np.float64).reshape(len(self), -1, COV_NODE_WIDTH)
        self.seconds = 0.0

    def __len__(self):
        return self.raw.shape[0]

    @property
    def failed(self):
        return self.raw[:, 0] == 1.0

    @property
    def skipped(self):
        return np.isnan(self.raw[:, 0])


def _cov_sigmas(pbm, sig0, sigu, sigw):
    """sig0 is required; sigu and sigw default to zeros"""
    if sig0 is None:
        raise ValueError("sig0, the initial 1-sigma of every state, is required")
    sigu = np.zeros(pbm.nu) if sigu is None else sigu
    sigw = np.zeros(pbm.nx) if sigw is None else sigw
    sig0, sigu, sigw = (np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (sig0, sigu, sigw))
    if sig0.size != pbm.nx or sigw.size != pbm.nx or sigu.size != pbm.nu:
        raise ValueError("sig0 and sigw hold nx = %d values, sigu nu = %d" % (pbm.nx, pbm.nu))
    return sig0, sigu, sigw


def _audit_covariance(pbm, batch, gains, sig0, sigu, sigw, nsig, per_node):
    N = pbm.pars.N
    sig0, sigu, sigw = _cov_sigmas(pbm, sig0, sigu, sigw)
    K = _tracking_gains(pbm, batch.B, gains)
    out = np.zeros((batch.rows, COV_WIDTH))
    sig = np.zeros((batch.rows, N, pbm.nx)) if per_node else None
    nodes = np.zeros((batch.rows, N, COV_NODE_WIDTH)) if per_node else None
    sec = _call(pbm, batch, _ptr(K), _ptr(sig0), _ptr(sigu), _ptr(sigw), float(nsig), _ptr(out), _ptr(sig), _ptr(nodes))
    out, sig, nodes = _finish(batch, out, sig, nodes)
    a = CovarianceAuditBatch(out, nsig, sig, nodes)
    a.seconds = sec
    return a


def audit_covariance(sol, pbm, gains=None, sig0=None, sigu=None, sigw=None, nsig=3.0, per_node=False, pp=None):
    """Closed-loop covariance audit of the batch solution `sol` (scp_audit_covariance_batch_host): discretize! about it, then the
    covariance recursion Sigma_{k+1} = A_cl Sigma_k A_cl' + Gam diag(sigu^2) Gam' + diag(sigw^2) with A_cl = A_k - Gam K_k on the
    device, from Sigma_1 = diag(sig0^2).  `gains` = a GainBatch, an array [B, N-1, nu, nx], or None for the gains the last
    `lqr_gains` call on this problem left in the handle; sig0[nx], sigu[nu], sigw[nx] in physical units (sigu, sigw: None = 0);
    `nsig` = the sigma level of n_below.  per_node=True also returns `sig` and `nodes`.  `sol.status` masks as in `audit`.
    Returns a CovarianceAuditBatch."""
    return _audit_covariance(pbm, _host_batch("scp_audit_covariance_batch_host", sol, pbm, pp), gains, sig0, sigu, sigw, nsig, per_node)


def audit_covariance_resident(pbm, gains=None, sig0=None, sigu=None, sigw=None, nsig=3.0, per_node=False):
    """The same for the batch RESIDENT in the handle (scp_audit_covariance_resident), with `gains` None = those of the last
    `lqr_gains_resident`; failed problems NaN; the run is left untouched.  Returns a CovarianceAuditBatch."""
    return _audit_covariance(pbm, _resident_batch("scp_audit_covariance_resident", pbm), gains, sig0, sigu,
                             sigw, nsig, per_node)


MC_STAT_WIDTH = 8      # SCP_MC_STAT_WIDTH
_MC_STAT_FIELDS = ("std_max", "std_node", "std_state", "mean_max", "mean_node", "effort_rms_max", "effort_rms_node", "n_min")


class MonteCarloAuditBatch(TrackingAuditBatch):
    """The Monte-Carlo audit of a batch (scp_audit_montecarlo_batch_host / scp_audit_montecarlo_resident, include/scp_mi355x.h):
    a TrackingAuditBatch whose `D` flights were flown under the noise model of the covariance audit, drawn from `seed`.  Named
    views [B] of `stat` [B, 8]: std_max = the largest sample standard deviation of a node error in units of Sx with its 1-based
    std_node and std_state, mean_max = the largest |sample mean| in units of Sx and mean_node, effort_rms_max = the largest rms
    feedback effort in units of Su and effort_rms_node, n_min = the fewest flights counted at a node.  Where the node records were
    asked for: `n` [B, N] the flights counted, `mean` and `std` [B, N, nx] of the node errors x(t_k) - xd[:, k], `effort_rms`
    [B, N, nu] (NaN at the last node); `moments` [B, N, 1 + 2 nx + nu] is the array itself; None otherwise.  Skipped (failed)
    problems hold NaN everywhere."""

    def __init__(self, raw, stat, nx, steps, res, viol_tol, D, seed=0, moments=None, flights=None):
        super().__init__(raw, steps, res, viol_tol, D, flights)
        self.stat = np.ascontiguousarray(stat, dtype=np.float64).reshape(-1, MC_STAT_WIDTH)
        assert self.stat.shape[0] == len(self)
        self.seed, nx = int(seed), int(nx)
        for j, name in enumerate(_MC_STAT_FIELDS):
            setattr(self, name, self.stat[:, j])
        self.moments = None if moments is None else np.ascontiguousarray(moments, dtype=np.float64)
        self.n = self.mean = self.std = self.effort_rms = None
        if self.moments is not None:
            assert self.moments.ndim == 3 and self.moments.shape[0] == len(self) and self.moments.shape[2] > 1 + 2 * nx
            self.n, self.mean = self.moments[:, :, 0], self.moments[:, :, 1:1 + nx]
            self.std, self.effort_rms = self.moments[:, :, 1 + nx:1 + 2 * nx], self.moments[:, :, 1 + 2 * nx:]

    def compare(self, cov):
        """Against the linear prediction: `cov` = a CovarianceAuditBatch of the same batch, made with per_node=True and the same
        sigmas and gains.  Returns an object with ratio [B, N, nx] = std / cov.sig (NaN where cov.sig == 0), ratio_max and
        ratio_min [B] over the nodes and states, and z_mean [B, N, nx] = |mean| / (cov.sig / sqrt(n)), the sample mean in
        standard errors of the prediction.  ValueError when the node records of either side are missing or the shapes differ."""
        from types import SimpleNamespace
        sig = getattr(cov, "sig", None)
        if self.moments is None or sig is None:
            raise ValueError("compare needs the node records of both audits (moments=True here, per_node=True there)")
        sig = np.asarray(sig, dtype=np.float64)
        if sig.shape != self.std.shape:
            raise ValueError("cov.sig of shape %s, the Monte-Carlo moments of shape %s" % (sig.shape, self.std.shape))
        with np.errstate(divide="ignore", invalid="ignore"):
            pos = sig > 0.0
            ratio = np.where(pos, self.std / np.where(pos, sig, 1.0), np.nan)
            z_mean = np.where(pos, np.abs(self.mean) / (np.where(pos, sig, 1.0) / np.sqrt(self.n)[:, :, None]), np.nan)
            flat = ratio.reshape(len(self), -1)
            some = np.isfinite(flat).any(axis=1)
            ratio_max = np.where(some, np.nanmax(np.where(np.isfinite(flat), flat, -np.inf), axis=1), np.nan)
            ratio_min = np.where(some, np.nanmin(np.where(np.isfinite(flat), flat, np.inf), axis=1), np.nan)
        return SimpleNamespace(ratio=ratio, ratio_max=ratio_max, ratio_min=ratio_min, z_mean=z_mean)


def _audit_montecarlo(pbm, batch, gains, steps, sig0, sigu, sigw, D, seed, viol_tol, moments, flights):
    N, D = pbm.pars.N, int(D)
    steps, res = _tracking_steps(pbm, steps)
    sig0, sigu, sigw = _cov_sigmas(pbm, sig0, sigu, sigw)
    K = _tracking_gains(pbm, batch.B, gains)
    out, stat = np.zeros((batch.rows, AUDIT_WIDTH)), np.zeros((batch.rows, MC_STAT_WIDTH))
    mom = np.zeros((batch.rows, N, 1 + 2 * pbm.nx + pbm.nu)) if moments else None
    recs = np.zeros((batch.rows, max(D, 1), AUDIT_WIDTH)) if flights else None
    sec = _call(pbm, batch, _ptr(K), steps, float(viol_tol), D, int(seed), _ptr(sig0), _ptr(sigu), _ptr(sigw), _ptr(out),
                _ptr(stat), _ptr(mom), _ptr(recs))
    out, stat, mom, recs = _finish(batch, out, stat, mom, recs)
    a = MonteCarloAuditBatch(out, stat, pbm.nx, steps, res, viol_tol, D, seed, mom, recs)
    a.seconds = sec
    return a


def audit_montecarlo(sol, pbm, gains=None, steps=None, sig0=None, sigu=None, sigw=None, D=64, seed=0, viol_tol=0.0, moments=True,
                     flights=False, pp=None):
    """Monte-Carlo audit of the batch solution `sol` (scp_audit_montecarlo_batch_host): `D` >= 2 closed-loop flights per problem
    through the nonlinear dynamics under the noise model of `audit_covariance` -- initial state xd[:, 0] + sig0 * xi, an input
    disturbance sigu * xi held over each interval, a state kick sigw * xi on arrival at each node -- drawn on the device from
    `seed` (every problem sees the same draws), and the per-node sample moments of the tracking error, reduced on the device.
    `gains` and `steps` as in `audit_tracking`; sig0[nx], sigu[nu], sigw[nx] as in `audit_covariance`.  moments=True also returns
    the node records, flights=True the record of every flight.  `sol.status` masks as in `audit`.  Returns a
    MonteCarloAuditBatch; its `compare(cov)` sets the moments next to the covariance audit's prediction."""
    return _audit_montecarlo(pbm, _host_batch("scp_audit_montecarlo_batch_host", sol, pbm, pp), gains, steps, sig0, sigu, sigw, D, seed,
                             viol_tol, moments, flights)


def audit_montecarlo_resident(pbm, gains=None, steps=None, sig0=None, sigu=None, sigw=None, D=64, seed=0, viol_tol=0.0, moments=True,
                              flights=False):
    """The same for the batch RESIDENT in the handle (scp_audit_montecarlo_resident), with `gains` None = those of the last
    `lqr_gains_resident`; failed problems NaN; the run is left untouched.  Returns a MonteCarloAuditBatch."""
    return _audit_montecarlo(pbm, _resident_batch("scp_audit_montecarlo_resident", pbm), gains, steps, sig0,
                             sigu, sigw, D, seed, viol_tol, moments, flights)
