// The handle-level entry points of the audit family (include/scp_mi355x.h): scp_audit_*_batch_host, scp_audit_*_resident and
// scp_lqr_gains_*.  Host code only: the kernels live in audit_api.hip, lqr_api.hip, cov_api.hip and mc_api.hip, behind their
// launch functions.  Every entry point is begin (its refusals) -> source (where the batch comes from) -> run (its work between
// the handle's two events, the copies, the device seconds).
#include <algorithm>
#include <initializer_list>
#include <string>
#include <vector>

#include "scp_handle.hpp"
#include "audit_kernel.hpp"
#include "lqr_kernel.hpp"
#include "cov_kernel.hpp"
#include "mc_kernel.hpp"

using namespace scp;

// ------------------------------------------------------------------------------------------
// the buffers outside h->allocs: each group is one list of slots, which reserves and releases it
// ------------------------------------------------------------------------------------------

struct Slot { void** p; size_t bytes; };
template <class T>
static Slot slot(T*& p, size_t bytes) { return {(void**)&p, bytes}; }

static void release(const std::vector<Slot>& slots)
{
    for (const Slot& s : slots) {
        if (*s.p) (void)hipFree(*s.p);
        *s.p = nullptr;
    }
}

// what the slots hold is freed, then all of them are allocated or none
static int reserve(scp_problem* h, const std::vector<Slot>& slots, const std::string& what)
{
    release(slots);
    for (const Slot& s : slots)
        if (hipMalloc(s.p, s.bytes) != hipSuccess) {
            (void)hipGetLastError();
            release(slots);
            h->err = what + " could not be allocated";
            return SCP_ERR_ALLOC;
        }
    return SCP_OK;
}

// the flight records and the staged dispersions for D flights of every problem the handle can hold
static std::vector<Slot> flight_slots(scp_problem* h, int D)
{
    scp_problem::Audit& A = h->audit;
    const size_t n = (size_t)D * (size_t)h->cap * sizeof(double);
    return {slot(A.flights, SCP_AUDIT_WIDTH * n), slot(A.dx0, (size_t)h->info.nx * n), slot(A.ugain, (size_t)h->info.nu * n),
            slot(A.ubias, (size_t)h->info.nu * n)};
}
// the buffers of h->lqr but Kin, and Kin, for every problem the handle can hold
static std::vector<Slot> lqr_slots(scp_problem* h)
{
    scp_problem::Lqr& q = h->lqr;
    const size_t nx = h->info.nx, nu = h->info.nu, npF = h->info.npF > 0 ? h->info.npF : 1, M = h->N - 1, cap = h->cap, D = sizeof(double);
    return {slot(q.dyn.A, nx * nx * M * cap * D), slot(q.dyn.Bm, nx * nu * M * cap * D), slot(q.dyn.Bp, nx * nu * M * cap * D),
            slot(q.dyn.F, nx * npF * M * cap * D), slot(q.dyn.r, nx * M * cap * D), slot(q.dyn.E, nx * nx * M * cap * D),
            slot(q.dyn.defect, nx * M * cap * D), slot(q.feas, cap * sizeof(int)), slot(q.info, SCP_LQR_INFO_WIDTH * cap * D),
            slot(q.w, (2 * nx + nu) * D), slot(q.K, nu * nx * M * cap * D)};
}
static std::vector<Slot> kin_slots(scp_problem* h)
{
    return {slot(h->lqr.Kin, sizeof(double) * h->info.nu * h->info.nx * (size_t)(h->N - 1) * (size_t)h->cap)};
}
static std::vector<Slot> cov_slots(scp_problem* h)
{
    scp_problem::Cov& c = h->cov;
    const size_t nx = h->info.nx, nu = h->info.nu, nrow = (size_t)h->info.ns + h->info.nl + h->info.nsoc, ntc = h->info.ntc, N = h->N,
                 cap = h->cap, D = sizeof(double);
    return {slot(c.rows, std::max<size_t>((nx + 1) * nrow * N * cap, 1) * D), slot(c.Hf, std::max<size_t>(ntc * nx * cap, 1) * D),
            slot(c.rec, SCP_COV_WIDTH * cap * D), slot(c.sig, nx * N * cap * D), slot(c.nodes, SCP_COV_NODE_WIDTH * N * cap * D),
            slot(c.w, (2 * nx + nu) * D)};
}
// the buffers of h->mc for W wavefronts per problem
static std::vector<Slot> mc_slots(scp_problem* h, int W)
{
    scp_problem::Mc& c = h->mc;
    const size_t nx = h->info.nx, nu = h->info.nu, nv = 1 + 2 * nx + nu, N = h->N, cap = h->cap, D = sizeof(double);
    return {slot(c.part, nv * N * (size_t)W * cap * D), slot(c.moments, nv * N * cap * D), slot(c.stat, SCP_MC_STAT_WIDTH * cap * D),
            slot(c.w, (2 * nx + nu) * D)};
}

void scp::audit_release(scp_problem* h)
{
    for (const auto& slots : {flight_slots(h, 0), lqr_slots(h), kin_slots(h), cov_slots(h), mc_slots(h, 0)}) release(slots);
}

// grows with D
static int flights_reserve(scp_problem* h, int D)
{
    if (D <= h->audit.disp_D) return SCP_OK;
    h->audit.disp_D = 0;
    TRY(reserve(h, flight_slots(h, D), "audit: the buffers of " + std::to_string(D) + " flights per problem"));
    h->audit.disp_D = D;
    return SCP_OK;
}
static int lqr_reserve(scp_problem* h)
{
    return h->lqr.K ? (int)SCP_OK : reserve(h, lqr_slots(h), "lqr: the discretisation and gain buffers");
}
static int cov_reserve(scp_problem* h)
{
    return h->cov.rows ? (int)SCP_OK : reserve(h, cov_slots(h), "audit: the row table and the records of the covariance audit");
}
// grows with W
static int mc_reserve(scp_problem* h, int W)
{
    if (W <= h->mc.W) return SCP_OK;
    h->mc.W = 0;
    TRY(reserve(h, mc_slots(h, W), "audit: the partial sums and the records of the Monte-Carlo audit"));
    h->mc.W = W;
    return SCP_OK;
}

// ------------------------------------------------------------------------------------------
// what the entry points share: the refusals, the batch source, the timed run, the packed triple
// ------------------------------------------------------------------------------------------

// what every audit entry point refuses, and the O(B) buffers of the call; the interval audit flies IMPULSE handles too
static int audit_begin(scp_problem* h, int res, const double* audit, bool foh_only = true)
{
    if (!h) return SCP_ERR_BAD_ARGUMENT;
    if (foh_only && h->method != SCP_FOH) { h->err = "audit: FOH handles only (an IMPULSE solution has no continuous input to fly)"; return SCP_ERR_UNSUPPORTED; }
    if (h->info.np_node > 0) {
        h->err = "audit: models with node parameters are not supported (a row of X at node k reads that node's own slack; between the nodes there is none)";
        return SCP_ERR_UNSUPPORTED;
    }
    if (res < 2 || !audit) { h->err = "audit: res >= 2 and an output array are required"; return SCP_ERR_BAD_ARGUMENT; }
    HIP_TRY(h, hipSetDevice(h->device));
    if (!h->audit.rec) TRY(dalloc(h, &h->audit.rec, (size_t)SCP_AUDIT_WIDTH * h->cap));
    if (!h->audit.mask) TRY(dalloc(h, &h->audit.mask, (size_t)h->cap));
    if (!h->audit.pp) TRY(dalloc(h, &h->audit.pp, (size_t)(h->info.npp > 0 ? h->info.npp : 1) * h->cap));
    return SCP_OK;
}

// the batch an entry point works on: its size, its trajectories, its pp and the instances to skip (nullptr: none)
struct AuditSource { int B; Traj tr; const double* d_pp; const int* mask; };

// from host arrays: trajectories into the solution buffers; with `with_pp`, pp into the audit's own buffer (the run's pp is left
// alone).  `who` prefixes the refusal ("audit", "lqr")
static int source_host(scp_problem* h, const char* who, int B, const double* xd, const double* ud, const double* p, bool with_pp,
                       const double* pp, AuditSource* src)
{
    if (B < 1 || !xd || !ud || (h->npt > 0 && !p) || (with_pp && h->info.npp > 0 && !pp)) { h->err = std::string(who) + ": missing input"; return SCP_ERR_BAD_ARGUMENT; }
    if (B > h->cap) { h->err = "batch size exceeds batch_capacity"; return SCP_ERR_BATCH_TOO_LARGE; }
    TRY(upload_traj(h, B, xd, ud, p, h->traj.sol_xd, h->traj.sol_ud, h->traj.sol_p));
    if (with_pp && h->info.npp > 0)
        HIP_TRY(h, hipMemcpyAsync(h->audit.pp, pp, sizeof(double) * h->info.npp * (size_t)B, hipMemcpyHostToDevice, h->stream));
    *src = {B, traj_sol(h), with_pp ? h->audit.pp : nullptr, nullptr};
    return SCP_OK;
}

// from the resident run: what the owning run's get_host returns (structured PTR: the last solution; the generic loops: the
// reference until the first iteration), that run's pp, and in h->audit.mask its solved instances.  `entry` names the caller
static int source_resident(scp_problem* h, const char* entry, AuditSource* src)
{
    const scp_sub* s = h->run.sub;
    if (h->run.kind == RUN_NONE || (h->run.kind != RUN_PTR && !s)) {
        h->err = std::string(entry) + ": no run owns the handle's trajectory buffers; start one with its init";
        return SCP_ERR_BAD_ARGUMENT;
    }
    const SubRun r = h->run.kind == RUN_PTR ? SubRun{h->ptr.B, true, h->ptr.d_pp, h->ptr.scp_status} : sub_run(s);
    *src = {r.B, r.iterated ? traj_sol(h) : traj_ref(h), r.d_pp, h->audit.mask};
    if (audit_mask_from_status(r.status, h->audit.mask, src->B, h->stream) != SCP_OK) {
        h->err = "audit: kernel launch failed";
        return SCP_ERR_HIP;
    }
    return SCP_OK;
}

// a launch function's return value, with the text of its failure
static int launched(scp_problem* h, int rc, const char* failed = "audit: kernel launch failed")
{
    if (rc != SCP_OK) h->err = failed;
    return rc;
}

// `enqueue` (which leaves its own h->err) between the handle's two events, every output with a destination to the host, the sync,
// the device seconds
struct Output { void* dst; const void* src; size_t bytes; };
template <class Enqueue>
static int timed_run(scp_problem* h, Enqueue&& enqueue, std::initializer_list<Output> outputs, double* seconds)
{
    HIP_TRY(h, hipEventRecord(h->timing.ev0, h->stream));
    TRY(enqueue());
    HIP_TRY(h, hipEventRecord(h->timing.ev1, h->stream));
    for (const Output& o : outputs)
        if (o.dst) HIP_TRY(h, hipMemcpyAsync(o.dst, o.src, o.bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    stamps_collect(h);
    return elapsed_out(h, seconds);
}

// dev = a [nx], b [nu], c [nx] through `host`, which the handle owns: the copy may outlive the call that enqueued it
static int upload_triple(scp_problem* h, std::vector<double>& host, double* dev, const double* a, const double* b, const double* c)
{
    const size_t nx = h->info.nx, nu = h->info.nu;
    host.clear();      // (the capacity stays: the storage does not move after the first call)
    host.insert(host.end(), a, a + nx); host.insert(host.end(), b, b + nu); host.insert(host.end(), c, c + nx);
    HIP_TRY(h, hipMemcpyAsync(dev, host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice, h->stream));
    return SCP_OK;
}

// ------------------------------------------------------------------------------------------
// single-shooting and interval-parallel audit (audit_kernel.hpp)
// ------------------------------------------------------------------------------------------

static int audit_run(scp_problem* h, const AuditSource& s, int res, double viol_tol, double* audit, double* seconds)
{
    AuditArgs a;
    a.B = s.B; a.N = h->N; a.res = res; a.viol_tol = viol_tol; a.xd = s.tr.xd; a.ud = s.tr.ud; a.p = s.tr.p; a.pp = s.d_pp; a.Sx = h->d_Sx;
    a.mask = s.mask; a.audit = h->audit.rec;
    return timed_run(h, [&] { return launched(h, audit_launch(h->model_id, h->par.data(), a, h->stream)); },
                     {{audit, h->audit.rec, sizeof(double) * SCP_AUDIT_WIDTH * (size_t)s.B}}, seconds);
}

extern "C" int scp_audit_batch_host(scp_handle h, int B, const double* xd, const double* ud, const double* p, const double* pp,
                                    int res, double viol_tol, double* audit, double* seconds)
{
    AuditSource src;
    TRY(audit_begin(h, res, audit));
    TRY(source_host(h, "audit", B, xd, ud, p, true, pp, &src));
    return audit_run(h, src, res, viol_tol, audit, seconds);
}

extern "C" int scp_audit_resident(scp_handle h, int res, double viol_tol, double* audit, double* seconds)
{
    AuditSource src;
    TRY(audit_begin(h, res, audit));
    TRY(source_resident(h, "scp_audit_resident", &src));
    return audit_run(h, src, res, viol_tol, audit, seconds);
}

// the flight kernel and the ordered fold
static int audit_intervals_run(scp_problem* h, const AuditSource& s, int res, double viol_tol, double* audit, double* intervals,
                               double* seconds)
{
    const size_t nrec = (size_t)SCP_AUDIT_INTERVAL_WIDTH * (h->N - 1);
    if (!h->audit.intervals) TRY(dalloc(h, &h->audit.intervals, nrec * h->cap));
    AuditIntervalArgs a;
    a.B = s.B; a.N = h->N; a.sub = audit_interval_sub(h->N, res); a.viol_tol = viol_tol; a.xd = s.tr.xd; a.ud = s.tr.ud; a.p = s.tr.p;
    a.pp = s.d_pp; a.Sx = h->d_Sx; a.mask = s.mask; a.intervals = h->audit.intervals; a.audit = h->audit.rec;
    return timed_run(h, [&] {
        const int rc = audit_intervals_launch(h->model_id, h->par.data(), (int)h->method, a, h->stream);
        return launched(h, rc, rc == SCP_ERR_HIP ? "audit: kernel launch failed" : "audit: IMPULSE handle of a model without an impulsive-input form");
    }, {{audit, h->audit.rec, sizeof(double) * SCP_AUDIT_WIDTH * (size_t)s.B}, {intervals, h->audit.intervals, sizeof(double) * nrec * (size_t)s.B}},
                     seconds);
}

extern "C" int scp_audit_intervals_batch_host(scp_handle h, int B, const double* xd, const double* ud, const double* p,
                                              const double* pp, int res, double viol_tol, double* audit, double* intervals,
                                              double* seconds)
{
    AuditSource src;
    TRY(audit_begin(h, res, audit, false));
    TRY(source_host(h, "audit", B, xd, ud, p, true, pp, &src));
    return audit_intervals_run(h, src, res, viol_tol, audit, intervals, seconds);
}

extern "C" int scp_audit_intervals_resident(scp_handle h, int res, double viol_tol, double* audit, double* intervals, double* seconds)
{
    AuditSource src;
    TRY(audit_begin(h, res, audit, false));
    TRY(source_resident(h, "scp_audit_intervals_resident", &src));
    return audit_intervals_run(h, src, res, viol_tol, audit, intervals, seconds);
}

// ------------------------------------------------------------------------------------------
// dispersed-flight audit: D off-nominal flights per problem and their ordered fold (audit_kernel.hpp)
// ------------------------------------------------------------------------------------------

static int audit_dispersed_begin(scp_problem* h, int res, int D, unsigned flags, const double* summary)
{
    TRY(audit_begin(h, res, summary));
    if (D < 1 || (flags & ~SCP_DISP_SHARED) != 0u) { h->err = "audit: D >= 1 and no flag bit but SCP_DISP_SHARED are required"; return SCP_ERR_BAD_ARGUMENT; }
    return SCP_OK;
}

// the caller's dispersions of a D-flight audit (dispersed, tracking) and its outputs
struct Flights {
    int D;
    const double *dx0, *ugain, *ubias;
    unsigned flags;
    const double* par_true;   // the truth model: the blob the flights are flown with (NULL: the handle's); taken as given
    double *summary, *flights;
};

// The run of a D-flight audit: the dispersions to the device, then `launch` -- the two kernels of the audit, given the model blob,
// the staged arrays (nullptr where the caller passed none) and the shared flag -- timed
template <class Launch>
static int audit_flights_run(scp_problem* h, const AuditSource& s, const Flights& f, double* seconds, Launch&& launch)
{
    TRY(flights_reserve(h, f.D));
    const bool shared = (f.flags & SCP_DISP_SHARED) != 0u;
    const size_t cols = shared ? (size_t)f.D : (size_t)f.D * (size_t)s.B;
    if (f.dx0) HIP_TRY(h, hipMemcpyAsync(h->audit.dx0, f.dx0, sizeof(double) * h->info.nx * cols, hipMemcpyHostToDevice, h->stream));
    if (f.ugain) HIP_TRY(h, hipMemcpyAsync(h->audit.ugain, f.ugain, sizeof(double) * h->info.nu * cols, hipMemcpyHostToDevice, h->stream));
    if (f.ubias) HIP_TRY(h, hipMemcpyAsync(h->audit.ubias, f.ubias, sizeof(double) * h->info.nu * cols, hipMemcpyHostToDevice, h->stream));
    return timed_run(h, [&] {
        return launched(h, launch(f.par_true ? f.par_true : h->par.data(), shared ? 1 : 0, f.dx0 ? h->audit.dx0 : nullptr,
                                  f.ugain ? h->audit.ugain : nullptr, f.ubias ? h->audit.ubias : nullptr));
    }, {{f.summary, h->audit.rec, sizeof(double) * SCP_AUDIT_WIDTH * (size_t)s.B},
        {f.flights, h->audit.flights, sizeof(double) * SCP_AUDIT_WIDTH * (size_t)f.D * (size_t)s.B}}, seconds);
}

static int audit_dispersed_run(scp_problem* h, const AuditSource& s, int res, double viol_tol, const Flights& f, double* seconds)
{
    return audit_flights_run(h, s, f, seconds, [&](const double* par, int shared, const double* d_dx0, const double* d_ugain, const double* d_ubias) {
        AuditDispersedArgs a;
        a.B = s.B; a.N = h->N; a.res = res; a.D = f.D; a.shared = shared; a.viol_tol = viol_tol; a.xd = s.tr.xd; a.ud = s.tr.ud; a.p = s.tr.p;
        a.pp = s.d_pp; a.Sx = h->d_Sx; a.dx0 = d_dx0; a.ugain = d_ugain; a.ubias = d_ubias; a.mask = s.mask; a.flights = h->audit.flights;
        a.audit = h->audit.rec;
        return audit_dispersed_launch(h->model_id, par, a, h->stream);
    });
}

extern "C" int scp_audit_dispersed_batch_host(scp_handle h, int B, const double* xd, const double* ud, const double* p, const double* pp,
                                              int res, double viol_tol, int D, const double* dx0, const double* ugain,
                                              const double* ubias, unsigned flags, const double* par_true, double* summary,
                                              double* flights, double* seconds)
{
    AuditSource src;
    TRY(audit_dispersed_begin(h, res, D, flags, summary));
    TRY(source_host(h, "audit", B, xd, ud, p, true, pp, &src));
    return audit_dispersed_run(h, src, res, viol_tol, {D, dx0, ugain, ubias, flags, par_true, summary, flights}, seconds);
}

extern "C" int scp_audit_dispersed_resident(scp_handle h, int res, double viol_tol, int D, const double* dx0, const double* ugain,
                                            const double* ubias, unsigned flags, const double* par_true, double* summary,
                                            double* flights, double* seconds)
{
    AuditSource src;
    TRY(audit_dispersed_begin(h, res, D, flags, summary));
    TRY(source_resident(h, "scp_audit_dispersed_resident", &src));
    return audit_dispersed_run(h, src, res, viol_tol, {D, dx0, ugain, ubias, flags, par_true, summary, flights}, seconds);
}

// ------------------------------------------------------------------------------------------
// LQR gains on the discretisation (lqr_kernel.hpp) and the closed-loop tracking audit
// ------------------------------------------------------------------------------------------

// what both gains entry points refuse (the audit's refusals, and the weights), and the buffers of the call
static int lqr_begin(scp_problem* h, const double* qx, const double* ru, const double* qf, const double* info)
{
    TRY(audit_begin(h, 2, info));
    if (!lqr_weights_ok(h->info.nx, h->info.nu, qx, ru, qf)) {
        h->err = "lqr: qx >= 0, qf >= 0 and ru > 0, all finite, are required";
        return SCP_ERR_BAD_ARGUMENT;
    }
    return lqr_reserve(h);
}

// discretize! about the batch into the buffers of h->lqr and the Riccati kernel; the gains are resident once the stream has drained
static int lqr_run(scp_problem* h, const AuditSource& s, const double* qx, const double* ru, const double* qf, double* K, double* info,
                   double* seconds)
{
    scp_problem::Lqr& q = h->lqr;
    const size_t nx = h->info.nx, nu = h->info.nu;
    q.B = 0;
    TRY(upload_triple(h, q.w_host, q.w, qx, ru, qf));
    LqrArgs a;
    a.B = s.B; a.N = h->N; a.A = q.dyn.A; a.Bm = q.dyn.Bm; a.Bp = q.dyn.Bp; a.qx = q.w; a.ru = q.w + nx; a.qf = q.w + nx + nu; a.mask = s.mask;
    a.K = q.K; a.info = q.info;
    TRY(timed_run(h, [&] {
        TRY(discretize_dev(h, s.B, s.tr.xd, s.tr.ud, s.tr.p, q.dyn, q.feas, s.mask));
        return launched(h, lqr_launch((int)nx, (int)nu, a, h->stream), "lqr: kernel launch failed");
    }, {{info, q.info, sizeof(double) * SCP_LQR_INFO_WIDTH * (size_t)s.B}, {K, q.K, sizeof(double) * nu * nx * (size_t)(h->N - 1) * (size_t)s.B}},
                  seconds));
    q.B = s.B;
    return SCP_OK;
}

extern "C" int scp_lqr_gains_batch_host(scp_handle h, int B, const double* xd, const double* ud, const double* p, const double* qx,
                                        const double* ru, const double* qf, double* K, double* info, double* seconds)
{
    AuditSource src;
    TRY(lqr_begin(h, qx, ru, qf, info));
    TRY(source_host(h, "lqr", B, xd, ud, p, false, nullptr, &src));
    return lqr_run(h, src, qx, ru, qf, K, info, seconds);
}

extern "C" int scp_lqr_gains_resident(scp_handle h, const double* qx, const double* ru, const double* qf, double* K, double* info,
                                      double* seconds)
{
    AuditSource src;
    TRY(lqr_begin(h, qx, ru, qf, info));
    TRY(source_resident(h, "scp_lqr_gains_resident", &src));
    return lqr_run(h, src, qx, ru, qf, K, info, seconds);
}

static int audit_tracking_begin(scp_problem* h, int steps, int D, unsigned flags, const double* summary)
{
    TRY(audit_dispersed_begin(h, 2, D, flags, summary));
    if (steps < 1) { h->err = "audit: steps >= 1 is required"; return SCP_ERR_BAD_ARGUMENT; }
    return SCP_OK;
}

// the gains of the call on the device: the caller's, staged, or the resident ones when they were made for this B
static int audit_tracking_gains(scp_problem* h, int B, const double* K, const double** d_K)
{
    if (K) {
        if (!h->lqr.Kin) TRY(reserve(h, kin_slots(h), "audit: the buffer of the gains passed by the caller"));
        HIP_TRY(h, hipMemcpyAsync(h->lqr.Kin, K, sizeof(double) * h->info.nu * h->info.nx * (size_t)(h->N - 1) * (size_t)B, hipMemcpyHostToDevice, h->stream));
        *d_K = h->lqr.Kin;
        return SCP_OK;
    }
    if (h->lqr.B == 0) { h->err = "audit: K is NULL and the handle holds no gains; call scp_lqr_gains_batch_host or scp_lqr_gains_resident first"; return SCP_ERR_BAD_ARGUMENT; }
    if (h->lqr.B != B) {
        h->err = "audit: K is NULL and the resident gains were made for B = " + std::to_string(h->lqr.B) + ", not " + std::to_string(B);
        return SCP_ERR_BAD_ARGUMENT;
    }
    *d_K = h->lqr.K;
    return SCP_OK;
}

static int audit_tracking_run(scp_problem* h, const AuditSource& s, const double* K, int steps, double viol_tol, const Flights& f,
                              double* seconds)
{
    const double* d_K = nullptr;
    TRY(audit_tracking_gains(h, s.B, K, &d_K));
    return audit_flights_run(h, s, f, seconds, [&](const double* par, int shared, const double* d_dx0, const double* d_ugain, const double* d_ubias) {
        AuditTrackingArgs a;
        a.B = s.B; a.N = h->N; a.steps = steps; a.D = f.D; a.shared = shared; a.viol_tol = viol_tol; a.xd = s.tr.xd; a.ud = s.tr.ud; a.p = s.tr.p;
        a.pp = s.d_pp; a.Sx = h->d_Sx; a.Su = h->d_Su; a.K = d_K; a.dx0 = d_dx0; a.ugain = d_ugain; a.ubias = d_ubias; a.mask = s.mask;
        a.flights = h->audit.flights; a.audit = h->audit.rec;
        return audit_tracking_launch(h->model_id, par, a, h->stream);
    });
}

extern "C" int scp_audit_tracking_batch_host(scp_handle h, int B, const double* xd, const double* ud, const double* p, const double* pp,
                                             const double* K, int steps, double viol_tol, int D, const double* dx0, const double* ugain,
                                             const double* ubias, unsigned flags, const double* par_true, double* summary,
                                             double* flights, double* seconds)
{
    AuditSource src;
    TRY(audit_tracking_begin(h, steps, D, flags, summary));
    TRY(source_host(h, "audit", B, xd, ud, p, true, pp, &src));
    return audit_tracking_run(h, src, K, steps, viol_tol, {D, dx0, ugain, ubias, flags, par_true, summary, flights}, seconds);
}

extern "C" int scp_audit_tracking_resident(scp_handle h, const double* K, int steps, double viol_tol, int D, const double* dx0,
                                           const double* ugain, const double* ubias, unsigned flags, const double* par_true,
                                           double* summary, double* flights, double* seconds)
{
    AuditSource src;
    TRY(audit_tracking_begin(h, steps, D, flags, summary));
    TRY(source_resident(h, "scp_audit_tracking_resident", &src));
    return audit_tracking_run(h, src, K, steps, viol_tol, {D, dx0, ugain, ubias, flags, par_true, summary, flights}, seconds);
}

// ------------------------------------------------------------------------------------------
// closed-loop covariance audit (cov_kernel.hpp)
// ------------------------------------------------------------------------------------------

// the dispersions of the covariance and the Monte-Carlo audit
struct Sigmas { const double *sig0, *sigu, *sigw; };

// what both covariance entry points refuse (the audit's refusals, and the dispersions), and the buffers of the call
static int cov_begin(scp_problem* h, const Sigmas& g, double nsig, const double* summary)
{
    TRY(audit_begin(h, 2, summary));
    if (!(nsig > 0.0) || !__builtin_isfinite(nsig) || !audit_sigmas_ok(h->info.nx, h->info.nu, g.sig0, g.sigu, g.sigw)) {
        h->err = "audit: sig0 >= 0, sigu >= 0, sigw >= 0, all finite, and a finite nsig > 0 are required";
        return SCP_ERR_BAD_ARGUMENT;
    }
    TRY(lqr_reserve(h));
    return cov_reserve(h);
}

// discretize! about the batch into the buffers of h->lqr, the row pre-pass and the chain
static int cov_run(scp_problem* h, const AuditSource& s, const double* K, const Sigmas& g, double nsig, double* summary, double* sig,
                   double* nodes, double* seconds)
{
    scp_problem::Lqr& q = h->lqr;
    scp_problem::Cov& c = h->cov;
    const size_t nx = h->info.nx, nu = h->info.nu, N = h->N;
    const double* d_K = nullptr;
    TRY(audit_tracking_gains(h, s.B, K, &d_K));
    TRY(upload_triple(h, c.w_host, c.w, g.sig0, g.sigu, g.sigw));
    CovArgs a;
    a.B = s.B; a.N = h->N; a.nrow[0] = h->info.ns; a.nrow[1] = h->info.nl; a.nrow[2] = h->info.nsoc; a.ntc = h->info.ntc; a.nsig = nsig;
    a.xd = s.tr.xd; a.ud = s.tr.ud; a.p = s.tr.p; a.pp = s.d_pp; a.A = q.dyn.A; a.Bm = q.dyn.Bm; a.Bp = q.dyn.Bp; a.K = d_K;
    a.Sx = h->d_Sx; a.Su = h->d_Su; a.sig0 = c.w; a.sigu = c.w + nx; a.sigw = c.w + nx + nu; a.mask = s.mask;
    a.rows = c.rows; a.Hf = c.Hf; a.summary = c.rec; a.sig = sig ? c.sig : nullptr; a.nodes = nodes ? c.nodes : nullptr;
    return timed_run(h, [&] {
        TRY(discretize_dev(h, s.B, s.tr.xd, s.tr.ud, s.tr.p, q.dyn, q.feas, s.mask));
        return launched(h, cov_launch(h->model_id, h->par.data(), a, h->stream));
    }, {{summary, c.rec, sizeof(double) * SCP_COV_WIDTH * (size_t)s.B}, {sig, c.sig, sizeof(double) * nx * N * (size_t)s.B},
        {nodes, c.nodes, sizeof(double) * SCP_COV_NODE_WIDTH * N * (size_t)s.B}}, seconds);
}

extern "C" int scp_audit_covariance_batch_host(scp_handle h, int B, const double* xd, const double* ud, const double* p, const double* pp,
                                               const double* K, const double* sig0, const double* sigu, const double* sigw, double nsig,
                                               double* summary, double* sig, double* nodes, double* seconds)
{
    AuditSource src;
    TRY(cov_begin(h, {sig0, sigu, sigw}, nsig, summary));
    TRY(source_host(h, "audit", B, xd, ud, p, true, pp, &src));
    return cov_run(h, src, K, {sig0, sigu, sigw}, nsig, summary, sig, nodes, seconds);
}

extern "C" int scp_audit_covariance_resident(scp_handle h, const double* K, const double* sig0, const double* sigu, const double* sigw,
                                             double nsig, double* summary, double* sig, double* nodes, double* seconds)
{
    AuditSource src;
    TRY(cov_begin(h, {sig0, sigu, sigw}, nsig, summary));
    TRY(source_resident(h, "scp_audit_covariance_resident", &src));
    return cov_run(h, src, K, {sig0, sigu, sigw}, nsig, summary, sig, nodes, seconds);
}

// ------------------------------------------------------------------------------------------
// Monte-Carlo audit (mc_kernel.hpp)
// ------------------------------------------------------------------------------------------

// what both Monte-Carlo entry points refuse (the tracking audit's refusals, D < 2, the dispersions, a NULL stat)
static int mc_begin(scp_problem* h, int steps, int D, const Sigmas& g, const double* summary, const double* stat)
{
    TRY(audit_tracking_begin(h, steps, D, 0u, summary));
    if (D < 2 || !stat) { h->err = "audit: D >= 2 flights and the stat array are required"; return SCP_ERR_BAD_ARGUMENT; }
    if (!audit_sigmas_ok(h->info.nx, h->info.nu, g.sig0, g.sigu, g.sigw)) {
        h->err = "audit: sig0 >= 0, sigu >= 0, sigw >= 0, all finite, are required";
        return SCP_ERR_BAD_ARGUMENT;
    }
    return SCP_OK;
}

// the three kernels
static int mc_run(scp_problem* h, const AuditSource& s, const double* K, int steps, double viol_tol, int D, uint64_t seed, const Sigmas& g,
                  double* summary, double* stat, double* moments, double* flights, double* seconds)
{
    scp_problem::Mc& c = h->mc;
    const size_t nx = h->info.nx, nu = h->info.nu, nv = 1 + 2 * nx + nu, N = h->N;
    const int W = (D + 63) / 64;
    const double* d_K = nullptr;
    TRY(audit_tracking_gains(h, s.B, K, &d_K));
    TRY(flights_reserve(h, D));
    TRY(mc_reserve(h, W));
    TRY(upload_triple(h, c.w_host, c.w, g.sig0, g.sigu, g.sigw));
    McArgs a;
    a.B = s.B; a.N = h->N; a.steps = steps; a.D = D; a.W = W; a.seed = seed; a.viol_tol = viol_tol; a.xd = s.tr.xd; a.ud = s.tr.ud; a.p = s.tr.p;
    a.pp = s.d_pp; a.Sx = h->d_Sx; a.Su = h->d_Su; a.K = d_K; a.sig0 = c.w; a.sigu = c.w + nx; a.sigw = c.w + nx + nu; a.mask = s.mask;
    a.flights = h->audit.flights; a.audit = h->audit.rec; a.part = c.part; a.moments = c.moments; a.stat = c.stat;
    return timed_run(h, [&] { return launched(h, mc_launch(h->model_id, h->par.data(), a, h->stream)); },
                     {{summary, h->audit.rec, sizeof(double) * SCP_AUDIT_WIDTH * (size_t)s.B}, {stat, c.stat, sizeof(double) * SCP_MC_STAT_WIDTH * (size_t)s.B},
                      {moments, c.moments, sizeof(double) * nv * N * (size_t)s.B},
                      {flights, h->audit.flights, sizeof(double) * SCP_AUDIT_WIDTH * (size_t)D * (size_t)s.B}}, seconds);
}

extern "C" int scp_audit_montecarlo_batch_host(scp_handle h, int B, const double* xd, const double* ud, const double* p, const double* pp,
                                               const double* K, int steps, double viol_tol, int D, uint64_t seed, const double* sig0,
                                               const double* sigu, const double* sigw, double* summary, double* stat, double* moments,
                                               double* flights, double* seconds)
{
    AuditSource src;
    TRY(mc_begin(h, steps, D, {sig0, sigu, sigw}, summary, stat));
    TRY(source_host(h, "audit", B, xd, ud, p, true, pp, &src));
    return mc_run(h, src, K, steps, viol_tol, D, seed, {sig0, sigu, sigw}, summary, stat, moments, flights, seconds);
}

extern "C" int scp_audit_montecarlo_resident(scp_handle h, const double* K, int steps, double viol_tol, int D, uint64_t seed,
                                             const double* sig0, const double* sigu, const double* sigw, double* summary, double* stat,
                                             double* moments, double* flights, double* seconds)
{
    AuditSource src;
    TRY(mc_begin(h, steps, D, {sig0, sigu, sigw}, summary, stat));
    TRY(source_resident(h, "scp_audit_montecarlo_resident", &src));
    return mc_run(h, src, K, steps, viol_tol, D, seed, {sig0, sigu, sigw}, summary, stat, moments, flights, seconds);
}
