// C-ABI implementation (include/scp_mi355x.h) of the MI355X-native SCP inner loop: model queries, the handle's life cycle and
// services (scp_handle.hpp), discretize! and propagate (K1), the handle-level continuous-time audit.
// gfx950 only: no CUDA shims, no dual paths.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "scp_handle.hpp"
#include "audit_kernel.hpp"
#include "lqr_kernel.hpp"
#include "cov_kernel.hpp"
#include "mc_kernel.hpp"
#include "discretize_kernel.hpp"

using namespace scp;

// The one check of every entry point that continues a run (iterate, poll, restart, get_host): is the run theirs?
int scp::check_run(scp_problem* h, RunKind kind, const scp_sub* sub, const char* who)
{
    if (!h) return SCP_ERR_BAD_ARGUMENT;
    if (h->run.kind == kind && h->run.sub == sub) return SCP_OK;
    static const char* const names[] = {"no run", "a structured PTR run", "an SCvx loop", "a GuSTO loop", "a generic PTR loop"};
    h->err = std::string(who) + " of " + names[kind] + ": the handle's trajectory buffers belong to " + names[h->run.kind] +
             (h->run.kind == kind ? " of another subproblem handle" : "") + "; start the run with its init";
    return SCP_ERR_BAD_ARGUMENT;
}

template <class M>
static void fill_info(scp_model_info* i)
{
    std::memset(i, 0, sizeof(*i));
    i->nx = M::nx; i->nu = M::nu; i->np = M::np; i->npF = M::npF;
    for (int j = 0; j < M::npF && j < 8; j++) i->Fcols[j] = M::Fcol(j);
    i->ns = M::ns; i->nic = M::nic; i->ntc = M::ntc; i->npar = M::npar; i->npp = M::npp;
    i->nl = M::nl; i->nsoc = M::nsoc; i->ng = M::ng;
    i->structured = M::structured ? 1 : 0;
    i->has_subproblem = M::has_subproblem ? 1 : 0;
    i->np_node = M::np_node;
    i->global_rows_in_X = M::global_rows_in_X ? 1 : 0;
    i->linf_groups = M::linf_groups; i->linf_rows = M::linf_rows;
    i->s_input_free = M::s_input_free ? 1 : 0;
}

extern "C" int scp_model_query(int model_id, scp_model_info* info)
{
    if (!info) return SCP_ERR_BAD_ARGUMENT;
    return with_model(model_id, [&](auto m) { fill_info<decltype(m)>(info); return (int)SCP_OK; });
}

// Host-side evaluation of the compiled model's convex sets and cost (the X / U / cost closures of TrajectoryProblem).
extern "C" int scp_model_rows(int model_id, const double* model_par, int N, int k, double* L, double* Lp, double* l,
                              double* Mm, double* m, double* Lg, double* lg, double* cost)
{
    if (!model_par || N < 2 || k < 1 || k > N) return SCP_ERR_BAD_ARGUMENT;
    return with_model(model_id, [&](auto mt) {
        using M = decltype(mt);
        constexpr int nx = M::nx, nu = M::nu, np = M::np, npa = np > 0 ? np : 1, nz = nx + nu, npc = np_compact<M>(),
                      npca = npc > 0 ? npc : 1;
        const typename M::Params P = M::make_params(model_par);
        const double t = (1.0 - (double)(k - 1) / (double)(N - 1)) * 0.0 + ((double)(k - 1) / (double)(N - 1)) * 1.0;
        if constexpr (M::nl > 0) {
            double Lb[M::nl * nz], Lpb[M::nl * npca], lb[M::nl];
            for (int i = 0; i < M::nl * npca; i++) Lpb[i] = 0.0;
            M::lin_rows(P, t, k, Lb, Lpb, lb);
            if (L) std::memcpy(L, Lb, sizeof(Lb));
            if (Lp) for (int i = 0; i < M::nl; i++) for (int j = 0; j < npc; j++) Lp[i * npc + j] = Lpb[i * npca + j];
            if (l) std::memcpy(l, lb, sizeof(lb));
        }
        if constexpr (M::nsoc > 0) {
            double Mb[M::nsoc * 4 * nz], mb[M::nsoc * 4];
            M::soc_rows(P, t, k, Mb, mb);
            if (Mm) std::memcpy(Mm, Mb, sizeof(Mb));
            if (m) std::memcpy(m, mb, sizeof(mb));
        }
        if constexpr (M::ng > 0) {
            double Lgb[M::ng * npa], lgb[M::ng];
            M::glin_rows(P, Lgb, lgb);
            if (Lg) for (int i = 0; i < M::ng; i++) for (int j = 0; j < np; j++) Lg[i * np + j] = Lgb[i * npa + j];
            if (lg) std::memcpy(lg, lgb, sizeof(lgb));
        }
        if (cost) {
            double Qu[nu], lu[nu], lx[nx], tx[nx], tp[npca], Qp[npca];
            for (int i = 0; i < npca; i++) { tp[i] = 0.0; Qp[i] = 0.0; }
            M::cost_terms(P, Qu, lu, lx, tx, tp, Qp);
            double* c = cost;
            for (int i = 0; i < nu; i++) *c++ = Qu[i];
            for (int i = 0; i < nu; i++) *c++ = lu[i];
            for (int i = 0; i < nx; i++) *c++ = lx[i];
            for (int i = 0; i < nx; i++) *c++ = tx[i];
            for (int i = 0; i < npc; i++) *c++ = tp[i];
            for (int i = 0; i < npc; i++) *c++ = Qp[i];
        }
        return (int)SCP_OK;
    });
}

// number of cone indicators of the convex state set X per node (GuSTO's soft penalties, gusto.jl:883-934): what
// scp_gusto_init_host expects as nst - ns
extern "C" int scp_model_state_indicators(int model_id, const double* model_par, int N, int* nq)
{
    if (!model_par || N < 2 || !nq) return SCP_ERR_BAD_ARGUMENT;
    return with_model(model_id, [&](auto mt) {
        using M = decltype(mt);
        *nq = count_x_indicators<M>(M::make_params(model_par), N);
        return (int)SCP_OK;
    });
}

// Host-side evaluation of the compiled model's closures at one point -- the counterpart of calling traj.f/A/B/F
// (problem.jl:432-450), traj.s/C/D/G (:560-600) and the cone indicators of X from Julia: lets a maintainer (and the CPU
// tests) check a compiled model against the closures it replaces without a GPU.
extern "C" int scp_model_eval_host(int model_id, const double* model_par, int N, int k, const double* x, const double* u,
                                   const double* p, double* f, double* A, double* B, double* F, double* s, double* C, double* D,
                                   double* G, double* q, int* nq)
{
    if (!model_par || N < 2 || k < 1 || k > N || !x || !u) return SCP_ERR_BAD_ARGUMENT;
    return with_model(model_id, [&](auto mt) {
        using M = decltype(mt);
        constexpr int nx = M::nx, nu = M::nu, npF = M::npF, npFa = npF > 0 ? npF : 1, ns = M::ns, nsa = ns > 0 ? ns : 1,
                      npc = np_compact<M>(), npca = npc > 0 ? npc : 1;
        if (np_total<M>(N) > 0 && !p) return (int)SCP_ERR_BAD_ARGUMENT;
        const typename M::Params P = M::make_params(model_par);
        const double t = (1.0 - (double)(k - 1) / (double)(N - 1)) * 0.0 + ((double)(k - 1) / (double)(N - 1)) * 1.0;
        double xs[nx], us[nu];
        for (int i = 0; i < nx; i++) xs[i] = x[i];
        for (int i = 0; i < nu; i++) us[i] = u[i];
        if (f || A || B || F) {
            double fb[nx], Ab[nx * nx], Bb[nx * nu], Fb[nx * npFa];
            M::dyn(P, t, k, xs, us, p, fb, Ab, Bb, Fb);
            if (f) std::memcpy(f, fb, sizeof(fb));
            if (A) std::memcpy(A, Ab, sizeof(Ab));
            if (B) std::memcpy(B, Bb, sizeof(Bb));
            if (F && npF > 0) std::memcpy(F, Fb, sizeof(double) * nx * npF);
        }
        if constexpr (ns > 0) {
            if (s || C || D || G) {
                double sb[nsa], Cb[nsa * nx], Db[nsa * nu], Gb[nsa * npca];
                for (int i = 0; i < nsa * npca; i++) Gb[i] = 0.0;
                M::s_eval(P, t, k, x, u, p, sb, Cb, Db, Gb);
                if (s) std::memcpy(s, sb, sizeof(double) * ns);
                if (C) std::memcpy(C, Cb, sizeof(double) * ns * nx);
                if (D) std::memcpy(D, Db, sizeof(double) * ns * nu);
                if (G) for (int i = 0; i < ns; i++) for (int j = 0; j < npc; j++) G[i * npc + j] = Gb[i * npca + j];
            }
        }
        int n = 0;
        for_each_x_indicator<M>(P, t, k, x, p, N, [&](double v) { if (q) q[n] = v; n++; });
        if (nq) *nq = n;
        return (int)SCP_OK;
    });
}

// Which entries of a model's parameter blob may change after scp_problem_create (M::par_mutable, model_common.hpp)
extern "C" int scp_model_par_mutable(int model_id, int* mask)
{
    if (!mask) return SCP_ERR_BAD_ARGUMENT;
    return with_model(model_id, [&](auto m) {
        using M = decltype(m);
        for (int i = 0; i < M::npar; i++) mask[i] = M::par_mutable(i) ? 1 : 0;
        return (int)SCP_OK;
    });
}

extern "C" const char* scp_last_error(scp_handle h) { return h ? h->err.c_str() : "null handle"; }

int scp::stamp_begin(scp_problem* h, int kind)
{
    scp_problem::Timing::Stamp st;
    if (!h->timing.stamps_free.empty()) { st = h->timing.stamps_free.back(); h->timing.stamps_free.pop_back(); }
    else { HIP_TRY(h, hipEventCreate(&st.a)); HIP_TRY(h, hipEventCreate(&st.b)); }
    st.kind = kind;
    HIP_TRY(h, hipEventRecord(st.a, h->stream));
    h->timing.stamps_pending.push_back(st);
    return SCP_OK;
}
int scp::stamp_end(scp_problem* h)
{
    HIP_TRY(h, hipEventRecord(h->timing.stamps_pending.back().b, h->stream));
    return SCP_OK;
}
// a finished stamp: its time into the totals of its kernel, its events back to the free list
static void stamp_fold(scp_problem* h, const scp_problem::Timing::Stamp& st)
{
    float ms = 0;
    if (hipEventElapsedTime(&ms, st.a, st.b) == hipSuccess) { h->timing.t_kernel[st.kind] += ms * 1e-3; h->timing.n_kernel[st.kind] += 1; }
    h->timing.stamps_free.push_back(st);
}
// call after a stream synchronise
void scp::stamps_collect(scp_problem* h)
{
    for (auto& st : h->timing.stamps_pending) stamp_fold(h, st);
    h->timing.stamps_pending.clear();
}

// without waiting: the stamps at the head of the list whose end event has completed (scp_ptr_poll_iteration)
void scp::stamps_collect_ready(scp_problem* h)
{
    size_t n = 0;
    while (n < h->timing.stamps_pending.size() && hipEventQuery(h->timing.stamps_pending[n].b) == hipSuccess) stamp_fold(h, h->timing.stamps_pending[n++]);
    h->timing.stamps_pending.erase(h->timing.stamps_pending.begin(), h->timing.stamps_pending.begin() + (long)n);
}

extern "C" int scp_get_kernel_timing(scp_handle h, double seconds[4], long launches[4], int reset)
{
    if (!h) return SCP_ERR_BAD_ARGUMENT;
    for (int i = 0; i < 4; i++) {
        if (seconds) seconds[i] = h->timing.t_kernel[i];
        if (launches) launches[i] = h->timing.n_kernel[i];
        if (reset) { h->timing.t_kernel[i] = 0; h->timing.n_kernel[i] = 0; }
    }
    return SCP_OK;
}

// *seconds = device time between the handle's ev0 and ev1 (recorded on its stream, which has been synchronised since)
int scp::elapsed_out(scp_problem* h, double* seconds)
{
    if (!seconds) return SCP_OK;
    float ms = 0;
    HIP_TRY(h, hipEventElapsedTime(&ms, h->timing.ev0, h->timing.ev1));
    *seconds = ms * 1e-3;
    return SCP_OK;
}

static int alloc_dyn(scp_problem* h, DynBuf& d)
{
    const size_t nx = h->info.nx, nu = h->info.nu, npF = h->info.npF > 0 ? h->info.npF : 1, M = h->N - 1, B = h->cap;
    TRY(dalloc(h, &d.A, nx * nx * M * B)); TRY(dalloc(h, &d.Bm, nx * nu * M * B)); TRY(dalloc(h, &d.Bp, nx * nu * M * B));
    TRY(dalloc(h, &d.F, nx * npF * M * B)); TRY(dalloc(h, &d.r, nx * M * B)); TRY(dalloc(h, &d.E, nx * nx * M * B));
    TRY(dalloc(h, &d.defect, nx * M * B));
    return SCP_OK;
}

extern "C" int scp_problem_create(const scp_problem_desc* d, scp_handle* out)
{
    if (!d || !out) return SCP_ERR_BAD_ARGUMENT;
    *out = nullptr;
    scp_model_info info;
    int rc = scp_model_query(d->model_id, &info);
    if (rc) return rc;
    if (d->N < 2 || d->Nsub < 2 || d->batch_capacity < 1) return SCP_ERR_BAD_ARGUMENT;
    if (d->disc_method != SCP_FOH && d->disc_method != SCP_IMPULSE) return SCP_ERR_BAD_ARGUMENT;
    if (d->disc_method == SCP_IMPULSE) {   // the model must define its impulse response (f, B evaluated with k < 0)
        const int rci = with_model(d->model_id, [&](auto mt) { return decltype(mt)::has_impulse ? (int)SCP_OK : (int)SCP_ERR_UNSUPPORTED; });
        if (rci != SCP_OK) return rci;
    }
    if (!d->model_par || !d->scale.Sx || !d->scale.cx || !d->scale.Su || !d->scale.cu) return SCP_ERR_BAD_ARGUMENT;
    const int npt = info.np + info.np_node * d->N;
    if (npt > 0 && (!d->scale.Sp || !d->scale.cp)) return SCP_ERR_BAD_ARGUMENT;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SCP_ERR_NO_DEVICE;
    if (d->device < 0 || d->device >= ndev) return SCP_ERR_NO_DEVICE;
    scp_problem* h = new (std::nothrow) scp_problem();
    if (!h) return SCP_ERR_ALLOC;
    h->model_id = d->model_id; h->info = info; h->N = d->N; h->Nsub = d->Nsub; h->method = d->disc_method;
    h->cap = d->batch_capacity; h->device = d->device; h->feas_tol = d->feas_tol; h->npt = npt;
    h->par.assign(d->model_par, d->model_par + info.npar);
    h->Sx.assign(d->scale.Sx, d->scale.Sx + info.nx); h->cx.assign(d->scale.cx, d->scale.cx + info.nx);
    h->Su.assign(d->scale.Su, d->scale.Su + info.nu); h->cu.assign(d->scale.cu, d->scale.cu + info.nu);
    if (npt > 0) {
        h->Sp.assign(d->scale.Sp, d->scale.Sp + npt); h->cp.assign(d->scale.cp, d->scale.cp + npt);
    }
    *out = h;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    {
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, h->device) == hipSuccess && ncu > 0) h->num_cus = ncu;
    }
    HIP_TRY(h, hipEventCreate(&h->timing.ev0));
    HIP_TRY(h, hipEventCreate(&h->timing.ev1));
    const size_t nx = info.nx, nu = info.nu, np = npt > 0 ? npt : 1;
    const size_t B = h->cap, N = h->N;
    TRY(dalloc(h, &h->traj.ref_xd, nx * N * B)); TRY(dalloc(h, &h->traj.ref_ud, nu * N * B)); TRY(dalloc(h, &h->traj.ref_p, np * B));
    TRY(dalloc(h, &h->traj.sol_xd, nx * N * B)); TRY(dalloc(h, &h->traj.sol_ud, nu * N * B)); TRY(dalloc(h, &h->traj.sol_p, np * B));
    TRY(alloc_dyn(h, h->traj.ref_dyn)); TRY(alloc_dyn(h, h->traj.sol_dyn));
    TRY(dalloc(h, &h->traj.d_feas_new, B)); TRY(dalloc(h, &h->traj.d_feas, B));
    TRY(dalloc(h, &h->d_iSx, nx)); TRY(dalloc(h, &h->d_Sx, nx)); TRY(dalloc(h, &h->d_cx, nx));
    TRY(dalloc(h, &h->d_Su, nu)); TRY(dalloc(h, &h->d_cu, nu)); TRY(dalloc(h, &h->d_Sp, np)); TRY(dalloc(h, &h->d_cp, np));
    std::vector<double> iSx(nx);
    for (size_t i = 0; i < nx; i++) iSx[i] = 1.0 / h->Sx[i];  // iSx = inv(Sx), scp.jl:492-493
    const size_t D = sizeof(double);
    HIP_TRY(h, hipMemcpy(h->d_iSx, iSx.data(), nx * D, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->d_Sx, h->Sx.data(), nx * D, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->d_cx, h->cx.data(), nx * D, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->d_Su, h->Su.data(), nu * D, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->d_cu, h->cu.data(), nu * D, hipMemcpyHostToDevice));
    if (npt > 0) {
        HIP_TRY(h, hipMemcpy(h->d_Sp, h->Sp.data(), (size_t)npt * D, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->d_cp, h->cp.data(), (size_t)npt * D, hipMemcpyHostToDevice));
    }
    return SCP_OK;
}

// Replace the handle's copy of the model constants.  Every kernel takes M::Params BY VALUE at its launch (make_params(h->par)),
// so the change applies to the launches enqueued after this call and is ordered with the handle's stream by construction: no
// synchronisation, nothing on the device to update.  Only the entries the model marks mutable may differ.
extern "C" int scp_problem_set_model_par(scp_handle h, const double* model_par)
{
    if (!h) return SCP_ERR_BAD_ARGUMENT;
    if (!model_par) { h->err = "scp_problem_set_model_par: model_par is required"; return SCP_ERR_BAD_ARGUMENT; }
    std::vector<int> mask((size_t)h->info.npar, 0);
    TRY(scp_model_par_mutable(h->model_id, mask.data()));
    for (int i = 0; i < h->info.npar; i++)
        if (!mask[i] && std::memcmp(&model_par[i], &h->par[i], sizeof(double)) != 0) {
            h->err = "scp_problem_set_model_par: entry " + std::to_string(i) + " of the model parameter blob is frozen into the handle "
                     "(host formulation, scaling or cost constant); only the entries scp_model_par_mutable marks may change";
            return SCP_ERR_BAD_ARGUMENT;
        }
    h->par.assign(model_par, model_par + h->info.npar);
    return SCP_OK;
}

// every device buffer of h->lqr
static std::vector<void*> lqr_buffers(scp_problem* h)
{
    scp_problem::Lqr& q = h->lqr;
    return {q.dyn.A, q.dyn.Bm, q.dyn.Bp, q.dyn.F, q.dyn.r, q.dyn.E, q.dyn.defect, q.feas, q.K, q.Kin, q.info, q.w};
}

extern "C" int scp_problem_destroy(scp_handle h)
{
    if (!h) return SCP_ERR_BAD_ARGUMENT;
    (void)hipSetDevice(h->device);
    if (h->guess.sg) starship_guess_free(h->guess.sg);
    for (void* p : h->allocs) (void)hipFree(p);
    for (double* p : {h->audit.flights, h->audit.dx0, h->audit.ugain, h->audit.ubias})
        if (p) (void)hipFree(p);
    for (void* p : lqr_buffers(h))
        if (p) (void)hipFree(p);
    for (double* p : {h->cov.rows, h->cov.Hf, h->cov.rec, h->cov.sig, h->cov.nodes, h->cov.w})
        if (p) (void)hipFree(p);
    for (double* p : {h->mc.part, h->mc.moments, h->mc.stat, h->mc.w})
        if (p) (void)hipFree(p);
    for (auto& st : h->timing.stamps_free) { (void)hipEventDestroy(st.a); (void)hipEventDestroy(st.b); }
    for (auto& st : h->timing.stamps_pending) { (void)hipEventDestroy(st.a); (void)hipEventDestroy(st.b); }
    if (h->timing.ev0) (void)hipEventDestroy(h->timing.ev0);
    if (h->timing.ev1) (void)hipEventDestroy(h->timing.ev1);
    for (hipEvent_t e : h->ptr.na_ev) (void)hipEventDestroy(e);
    if (h->ptr.na_ring) (void)hipHostFree(h->ptr.na_ring);
    if (h->ptr.na_dev) (void)hipFree(h->ptr.na_dev);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return SCP_OK;
}

extern "C" int scp_set_stream_priority(scp_handle h, int level)
{
    if (!h) return SCP_ERR_BAD_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    int least = 0, greatest = 0;      // numerically: greatest priority <= least priority
    HIP_TRY(h, hipDeviceGetStreamPriorityRange(&least, &greatest));
    int pr = -level;                  // level > 0 = higher priority = numerically lower
    pr = std::max(greatest, std::min(least, pr));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    stamps_collect(h);
    hipStream_t ns = nullptr;
    HIP_TRY(h, hipStreamCreateWithPriority(&ns, hipStreamNonBlocking, pr));
    (void)hipStreamDestroy(h->stream);
    h->stream = ns;
    return SCP_OK;
}

extern "C" int scp_sync(scp_handle h)
{
    if (!h) return SCP_ERR_BAD_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    stamps_collect(h);
    return SCP_OK;
}

// ------------------------------------------------------------------------------------------
// discretize!
// ------------------------------------------------------------------------------------------

int scp::discretize_dev(scp_problem* h, int B, const double* xd, const double* ud, const double* p, const DynBuf& d,
                          int* feas, const int* mask)
{
    DiscArgs a;
    a.B = B; a.N = h->N; a.Nsub = h->Nsub;
    a.xd = xd; a.ud = ud; a.p = p; a.iSx = h->d_iSx; a.feas_tol = h->feas_tol;
    a.A = d.A; a.Bm = d.Bm; a.Bp = d.Bp; a.F = d.F; a.r = d.r; a.E = d.E; a.defect = d.defect; a.feas = feas; a.mask = mask;
    HIP_TRY(h, hipMemsetAsync(feas, 0xff, (size_t)B * sizeof(int), h->stream));  // ref.feas = true (:179); non-zero == true
    return with_model(h->model_id, [&](auto m) -> int {
        using M = decltype(m);
        using L = DiscLayout<M>;
        const long groups = (long)a.B * (a.N - 1);
        const int blocks = (int)((groups + L::GROUPS_PER_BLOCK - 1) / L::GROUPS_PER_BLOCK);
        typename M::Params P = M::make_params(h->par.data());
        TRY(stamp_begin(h, 0));
        const double rk4_step = 1.0 / ((double)(a.N - 1) * (double)(a.Nsub - 1));
        if (h->disc.bits == 32) {     // fp32 arithmetic (tolerance-check variant; FOH, models with M::has_fp32)
            if constexpr (M::has_fp32) {
                hipLaunchKernelGGL((discretize_foh_kernel<M, false, float>), dim3(blocks), dim3(256), 0, h->stream, a, P);
            } else {
                return (int)SCP_ERR_UNSUPPORTED;
            }
        } else if (h->method == SCP_IMPULSE) {
            hipLaunchKernelGGL((discretize_foh_kernel<M, true>), dim3(blocks), dim3(256), 0, h->stream, a, P);
        } else if (M::const_jacobian && !h->disc.reference_form && rk4_step <= M::var_form_max_step) {
            // variational form (K1v): thread per (problem, interval, column), blockIdx.y = column
            const unsigned gx = (unsigned)((groups + 255) / 256);
            hipLaunchKernelGGL((discretize_foh_var_kernel<M, false>), dim3(gx, 2 * M::nx + 2 * M::nu), dim3(256), 0, h->stream, a, P);
            hipLaunchKernelGGL((discretize_foh_var_kernel<M, true>), dim3(gx, M::npF + 1), dim3(256), 0, h->stream, a, P);
        } else if (!M::const_jacobian && M::var_form_max_phys_step > 0.0) {
            // state-dependent Jacobians: per problem the variational form (K1x) where it meets the reference formulation to
            // 1e-10 (physical RK4 step below the model's bound), the reference form (K1) elsewhere
            if (!h->disc.d_mvar) { TRY(dalloc(h, &h->disc.d_mvar, 2 * (size_t)h->cap)); }
            int* mvar = h->disc.d_mvar; int* mref = h->disc.d_mvar + h->cap;
            hipLaunchKernelGGL(disc_split_kernel<M>, dim3((a.B + 255) / 256), dim3(256), 0, h->stream, a.B, a.N, a.Nsub, a.p, a.mask, P,
                               h->disc.reference_form ? 1 : 0, mvar, mref);
            DiscArgs av = a; av.mask = mvar;
            const unsigned gx = (unsigned)((groups + 255) / 256);
            hipLaunchKernelGGL((discretize_foh_varx_kernel<M, R_PHI>), dim3(gx, M::nx), dim3(256), 0, h->stream, av, P);
            hipLaunchKernelGGL((discretize_foh_varx_kernel<M, R_BM>), dim3(gx, M::nu), dim3(256), 0, h->stream, av, P);
            hipLaunchKernelGGL((discretize_foh_varx_kernel<M, R_BP>), dim3(gx, M::nu), dim3(256), 0, h->stream, av, P);
            if (M::npF > 0) hipLaunchKernelGGL((discretize_foh_varx_kernel<M, R_F>), dim3(gx, M::npF), dim3(256), 0, h->stream, av, P);
            hipLaunchKernelGGL((discretize_foh_varx_kernel<M, R_R>), dim3(gx, 1), dim3(256), 0, h->stream, av, P);
            hipLaunchKernelGGL((discretize_foh_varx_kernel<M, R_E>), dim3(gx, M::nx), dim3(256), 0, h->stream, av, P);
            DiscArgs ar = a; ar.mask = mref;
            hipLaunchKernelGGL(discretize_foh_kernel<M>, dim3(blocks), dim3(256), 0, h->stream, ar, P);
        } else {
            hipLaunchKernelGGL(discretize_foh_kernel<M>, dim3(blocks), dim3(256), 0, h->stream, a, P);
        }
        TRY(stamp_end(h));
        HIP_TRY(h, hipGetLastError());
        return (int)SCP_OK;
    });
}

extern "C" int scp_set_discretize_precision(scp_handle h, int bits)
{
    if (!h || (bits != 32 && bits != 64)) return SCP_ERR_BAD_ARGUMENT;
    if (bits == 32) {
        const bool ok = with_model(h->model_id, [&](auto m) -> int { return decltype(m)::has_fp32 ? 1 : 0; }) == 1;
        if (!ok || h->method != SCP_FOH) { h->err = "fp32 discretize!: FOH and models with an fp32 evaluation only (starship)"; return SCP_ERR_UNSUPPORTED; }
    }
    h->disc.bits = bits;
    return SCP_OK;
}

extern "C" int scp_discretize_batch_dev(scp_handle h, int B, const double* xd, const double* ud, const double* p,
                                        double* A, double* Bm, double* Bp, double* F, double* r, double* E,
                                        double* defect, int32_t* feas)
{
    if (!h || B < 1 || !xd || !ud || !A || !Bm || !Bp || !F || !r || !E || !defect || !feas) return SCP_ERR_BAD_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    DynBuf d;
    d.A = A; d.Bm = Bm; d.Bp = Bp; d.F = F; d.r = r; d.E = E; d.defect = defect;
    return discretize_dev(h, B, xd, ud, p, d, feas, nullptr);
}

int scp::copy_dyn_out(scp_problem* h, int B, const DynBuf& d, double* A, double* Bm, double* Bp, double* F, double* r,
                        double* E, double* defect)
{
    const size_t nx = h->info.nx, nu = h->info.nu, npF = h->info.npF, M = h->N - 1, D = sizeof(double), b = B;
    if (A) HIP_TRY(h, hipMemcpyAsync(A, d.A, nx * nx * M * b * D, hipMemcpyDeviceToHost, h->stream));
    if (Bm) HIP_TRY(h, hipMemcpyAsync(Bm, d.Bm, nx * nu * M * b * D, hipMemcpyDeviceToHost, h->stream));
    if (Bp) HIP_TRY(h, hipMemcpyAsync(Bp, d.Bp, nx * nu * M * b * D, hipMemcpyDeviceToHost, h->stream));
    if (F && npF > 0) HIP_TRY(h, hipMemcpyAsync(F, d.F, nx * npF * M * b * D, hipMemcpyDeviceToHost, h->stream));
    if (r) HIP_TRY(h, hipMemcpyAsync(r, d.r, nx * M * b * D, hipMemcpyDeviceToHost, h->stream));
    if (E) HIP_TRY(h, hipMemcpyAsync(E, d.E, nx * nx * M * b * D, hipMemcpyDeviceToHost, h->stream));
    if (defect) HIP_TRY(h, hipMemcpyAsync(defect, d.defect, nx * M * b * D, hipMemcpyDeviceToHost, h->stream));
    return SCP_OK;
}

int scp::upload_traj(scp_problem* h, int B, const double* xd, const double* ud, const double* p, double* dxd,
                       double* dud, double* dp)
{
    const size_t nx = h->info.nx, nu = h->info.nu, np = h->npt, N = h->N, D = sizeof(double), b = B;
    HIP_TRY(h, hipMemcpyAsync(dxd, xd, nx * N * b * D, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(dud, ud, nu * N * b * D, hipMemcpyHostToDevice, h->stream));
    if (np > 0) HIP_TRY(h, hipMemcpyAsync(dp, p, np * b * D, hipMemcpyHostToDevice, h->stream));
    return SCP_OK;
}

// the opposite direction: the last solution (h->traj.sol_*) or the reference (h->traj.ref_*) and its defects; any pointer may be NULL
int scp::download_traj(scp_problem* h, int B, bool from_sol, double* xd, double* ud, double* p, double* defect)
{
    const size_t nx = h->info.nx, nu = h->info.nu, np = h->npt, N = h->N, D = sizeof(double), b = B;
    if (xd) HIP_TRY(h, hipMemcpyAsync(xd, from_sol ? h->traj.sol_xd : h->traj.ref_xd, nx * N * b * D, hipMemcpyDeviceToHost, h->stream));
    if (ud) HIP_TRY(h, hipMemcpyAsync(ud, from_sol ? h->traj.sol_ud : h->traj.ref_ud, nu * N * b * D, hipMemcpyDeviceToHost, h->stream));
    if (p && np > 0) HIP_TRY(h, hipMemcpyAsync(p, from_sol ? h->traj.sol_p : h->traj.ref_p, np * b * D, hipMemcpyDeviceToHost, h->stream));
    if (defect)
        HIP_TRY(h, hipMemcpyAsync(defect, (from_sol ? h->traj.sol_dyn : h->traj.ref_dyn).defect, nx * (N - 1) * b * D, hipMemcpyDeviceToHost, h->stream));
    return SCP_OK;
}

int scp::feas_out(scp_problem* h, int B, const int* dfeas, uint8_t* feas)
{
    std::vector<int> hf(B);
    HIP_TRY(h, hipMemcpyAsync(hf.data(), dfeas, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    stamps_collect(h);
    if (feas)
        for (int i = 0; i < B; i++) feas[i] = hf[i] != 0;
    return SCP_OK;
}

// active[0 .. B) = 1 for a run that starts; waits for the stream (the source is on this stack frame)
int scp::set_active_all(scp_problem* h, int* active, int B)
{
    std::vector<int> ones(B, 1);
    HIP_TRY(h, hipMemcpyAsync(active, ones.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    stamps_collect(h);
    return SCP_OK;
}

__global__ void merge_feas_kernel(int B, const int* active, const int* fnew, int* feas)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B && (active == nullptr || active[b])) feas[b] = fnew[b];
}
// feas <- the flags of the launch for its active problems (a null `active`: for all): d_feas keeps every problem's LAST solution's
int scp::merge_feas_dev(scp_problem* h, int B, const int* active)
{
    hipLaunchKernelGGL(merge_feas_kernel, dim3((B + 255) / 256), dim3(256), 0, h->stream, B, active, h->traj.d_feas_new, h->traj.d_feas);
    HIP_TRY(h, hipGetLastError());
    return SCP_OK;
}

extern "C" int scp_discretize_batch_host(scp_handle h, int B, const double* xd, const double* ud, const double* p,
                                         double* A, double* Bm, double* Bp, double* F, double* r, double* E,
                                         double* defect, uint8_t* feas, double* seconds)
{
    if (!h || B < 1 || !xd || !ud) return SCP_ERR_BAD_ARGUMENT;
    if (B > h->cap) return SCP_ERR_BATCH_TOO_LARGE;
    if (h->npt > 0 && !p) return SCP_ERR_BAD_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    TRY(upload_traj(h, B, xd, ud, p, h->traj.sol_xd, h->traj.sol_ud, h->traj.sol_p));
    HIP_TRY(h, hipEventRecord(h->timing.ev0, h->stream));
    TRY(discretize_dev(h, B, h->traj.sol_xd, h->traj.sol_ud, h->traj.sol_p, h->traj.sol_dyn, h->traj.d_feas_new, nullptr));
    HIP_TRY(h, hipEventRecord(h->timing.ev1, h->stream));
    TRY(copy_dyn_out(h, B, h->traj.sol_dyn, A, Bm, Bp, F, r, E, defect));
    TRY(feas_out(h, B, h->traj.d_feas_new, feas));
    return elapsed_out(h, seconds);
}

extern "C" int scp_propagate_batch_host(scp_handle h, int B, const double* xd, const double* ud, const double* p, int res,
                                        double* xc)
{
    if (!h || B < 1 || !xd || !ud || !xc || res < 2) return SCP_ERR_BAD_ARGUMENT;
    if (B > h->cap) return SCP_ERR_BATCH_TOO_LARGE;
    if (h->npt > 0 && !p) return SCP_ERR_BAD_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    TRY(upload_traj(h, B, xd, ud, p, h->traj.sol_xd, h->traj.sol_ud, h->traj.sol_p));
    double* d_xc = nullptr;   // result buffer of this call only (post-processing path, not resident)
    const bool imp = h->method == SCP_IMPULSE;
    const int sub = (res + (h->N - 1) - 1) / (h->N - 1);                  // IMPULSE: subres = ceil(res / (N - 1))  (:544)
    const size_t nsamp = imp ? 1 + (size_t)(h->N - 1) * sub : (size_t)res;
    const size_t n = (size_t)h->info.nx * nsamp * (size_t)B;
    HIP_TRY(h, hipMalloc(&d_xc, n * sizeof(double)));
    PropArgs a;
    a.B = B; a.N = h->N; a.res = res; a.xd = h->traj.sol_xd; a.ud = h->traj.sol_ud; a.p = h->traj.sol_p; a.xc = d_xc;
    PropImpArgs ai;
    ai.B = B; ai.N = h->N; ai.sub = sub; ai.xd = h->traj.sol_xd; ai.ud = h->traj.sol_ud; ai.p = h->traj.sol_p; ai.xc = d_xc;
    int rc = with_model(h->model_id, [&](auto m) -> int {
        using M = decltype(m);
        typename M::Params P = M::make_params(h->par.data());
        if (imp) {
            const long tot = (long)B * (h->N - 1);
            hipLaunchKernelGGL(propagate_impulse_kernel<M>, dim3((unsigned)((tot + 63) / 64)), dim3(64), 0, h->stream, ai, P);
        } else {
            hipLaunchKernelGGL(propagate_foh_kernel<M>, dim3((B + 63) / 64), dim3(64), 0, h->stream, a, P);
        }
        return (int)SCP_OK;
    });
    hipError_t e = hipGetLastError();
    if (rc == SCP_OK && e == hipSuccess) e = hipMemcpyAsync(xc, d_xc, n * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (rc == SCP_OK && e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void)hipFree(d_xc);
    if (rc != SCP_OK) return rc;
    HIP_TRY(h, e);
    return SCP_OK;
}

// ------------------------------------------------------------------------------------------
// continuous-time audit (audit_kernel.hpp; the kernels live in audit_api.hip)
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

// the kernel between the handle's two events, the records to the host, the device time
static int audit_run(scp_problem* h, int B, const Traj& tr, const double* d_pp, const int* mask, int res, double viol_tol,
                     double* audit, double* seconds)
{
    AuditArgs a;
    a.B = B; a.N = h->N; a.res = res; a.viol_tol = viol_tol; a.xd = tr.xd; a.ud = tr.ud; a.p = tr.p; a.pp = d_pp; a.Sx = h->d_Sx;
    a.mask = mask; a.audit = h->audit.rec;
    HIP_TRY(h, hipEventRecord(h->timing.ev0, h->stream));
    const int rc = audit_launch(h->model_id, h->par.data(), a, h->stream);
    if (rc != SCP_OK) { h->err = "audit: kernel launch failed"; return rc; }
    HIP_TRY(h, hipEventRecord(h->timing.ev1, h->stream));
    HIP_TRY(h, hipMemcpyAsync(audit, h->audit.rec, sizeof(double) * SCP_AUDIT_WIDTH * (size_t)B, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    stamps_collect(h);
    return elapsed_out(h, seconds);
}

// the host variants' input: trajectories into the solution buffers, pp into the audit's own buffer (the run's pp is left alone)
static int audit_stage_host(scp_problem* h, int B, const double* xd, const double* ud, const double* p, const double* pp)
{
    if (B < 1 || !xd || !ud || (h->npt > 0 && !p) || (h->info.npp > 0 && !pp)) { h->err = "audit: missing input"; return SCP_ERR_BAD_ARGUMENT; }
    if (B > h->cap) { h->err = "batch size exceeds batch_capacity"; return SCP_ERR_BATCH_TOO_LARGE; }
    TRY(upload_traj(h, B, xd, ud, p, h->traj.sol_xd, h->traj.sol_ud, h->traj.sol_p));
    if (h->info.npp > 0)
        HIP_TRY(h, hipMemcpyAsync(h->audit.pp, pp, sizeof(double) * h->info.npp * (size_t)B, hipMemcpyHostToDevice, h->stream));
    return SCP_OK;
}

extern "C" int scp_audit_batch_host(scp_handle h, int B, const double* xd, const double* ud, const double* p, const double* pp,
                                    int res, double viol_tol, double* audit, double* seconds)
{
    TRY(audit_begin(h, res, audit));
    TRY(audit_stage_host(h, B, xd, ud, p, pp));
    return audit_run(h, B, traj_sol(h), h->audit.pp, nullptr, res, viol_tol, audit, seconds);
}

// the batch a resident audit flies: what the owning run's get_host returns (structured PTR: the last solution; the generic loops:
// the reference until the first iteration), that run's pp, and in h->audit.mask its solved instances
struct AuditSource { int B; Traj tr; const double* d_pp; };
static int audit_resident_source(scp_problem* h, const char* no_run, AuditSource* src)
{
    const scp_sub* s = h->run.sub;
    if (h->run.kind == RUN_NONE || (h->run.kind != RUN_PTR && !s)) { h->err = no_run; return SCP_ERR_BAD_ARGUMENT; }
    const SubRun r = h->run.kind == RUN_PTR ? SubRun{h->ptr.B, true, h->ptr.d_pp, h->ptr.scp_status} : sub_run(s);
    src->B = r.B;
    src->tr = r.iterated ? traj_sol(h) : traj_ref(h);
    src->d_pp = r.d_pp;
    if (audit_mask_from_status(r.status, h->audit.mask, src->B, h->stream) != SCP_OK) {
        h->err = "audit: kernel launch failed";
        return SCP_ERR_HIP;
    }
    return SCP_OK;
}

extern "C" int scp_audit_resident(scp_handle h, int res, double viol_tol, double* audit, double* seconds)
{
    TRY(audit_begin(h, res, audit));
    AuditSource src;
    TRY(audit_resident_source(h, "scp_audit_resident: no run owns the handle's trajectory buffers; start one with its init", &src));
    return audit_run(h, src.B, src.tr, src.d_pp, h->audit.mask, res, viol_tol, audit, seconds);
}

// interval-parallel audit: the flight kernel and the ordered fold between the handle's two events, then the copies
static int audit_intervals_run(scp_problem* h, int B, const Traj& tr, const double* d_pp, const int* mask, int res, double viol_tol,
                               double* audit, double* intervals, double* seconds)
{
    const size_t nrec = (size_t)SCP_AUDIT_INTERVAL_WIDTH * (h->N - 1);
    if (!h->audit.intervals) TRY(dalloc(h, &h->audit.intervals, nrec * h->cap));
    AuditIntervalArgs a;
    a.B = B; a.N = h->N; a.sub = audit_interval_sub(h->N, res); a.viol_tol = viol_tol; a.xd = tr.xd; a.ud = tr.ud; a.p = tr.p;
    a.pp = d_pp; a.Sx = h->d_Sx; a.mask = mask; a.intervals = h->audit.intervals; a.audit = h->audit.rec;
    HIP_TRY(h, hipEventRecord(h->timing.ev0, h->stream));
    const int rc = audit_intervals_launch(h->model_id, h->par.data(), (int)h->method, a, h->stream);
    if (rc != SCP_OK) {
        h->err = rc == SCP_ERR_HIP ? "audit: kernel launch failed" : "audit: IMPULSE handle of a model without an impulsive-input form";
        return rc;
    }
    HIP_TRY(h, hipEventRecord(h->timing.ev1, h->stream));
    HIP_TRY(h, hipMemcpyAsync(audit, h->audit.rec, sizeof(double) * SCP_AUDIT_WIDTH * (size_t)B, hipMemcpyDeviceToHost, h->stream));
    if (intervals)
        HIP_TRY(h, hipMemcpyAsync(intervals, h->audit.intervals, sizeof(double) * nrec * (size_t)B, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    stamps_collect(h);
    return elapsed_out(h, seconds);
}

extern "C" int scp_audit_intervals_batch_host(scp_handle h, int B, const double* xd, const double* ud, const double* p,
                                              const double* pp, int res, double viol_tol, double* audit, double* intervals,
                                              double* seconds)
{
    TRY(audit_begin(h, res, audit, false));
    TRY(audit_stage_host(h, B, xd, ud, p, pp));
    return audit_intervals_run(h, B, traj_sol(h), h->audit.pp, nullptr, res, viol_tol, audit, intervals, seconds);
}

extern "C" int scp_audit_intervals_resident(scp_handle h, int res, double viol_tol, double* audit, double* intervals, double* seconds)
{
    TRY(audit_begin(h, res, audit, false));
    AuditSource src;
    TRY(audit_resident_source(h, "scp_audit_intervals_resident: no run owns the handle's trajectory buffers; start one with its init", &src));
    return audit_intervals_run(h, src.B, src.tr, src.d_pp, h->audit.mask, res, viol_tol, audit, intervals, seconds);
}

// dispersed-flight audit: D off-nominal flights per problem and their ordered fold (audit_kernel.hpp)
static int audit_dispersed_begin(scp_problem* h, int res, int D, unsigned flags, const double* summary)
{
    TRY(audit_begin(h, res, summary));
    if (D < 1 || (flags & ~SCP_DISP_SHARED) != 0u) { h->err = "audit: D >= 1 and no flag bit but SCP_DISP_SHARED are required"; return SCP_ERR_BAD_ARGUMENT; }
    return SCP_OK;
}

// the flight records and the staged dispersions for D flights of every problem the handle can hold
static int audit_dispersed_reserve(scp_problem* h, int D)
{
    scp_problem::Audit& A = h->audit;
    if (D <= A.disp_D) return SCP_OK;
    for (double** p : {&A.flights, &A.dx0, &A.ugain, &A.ubias}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    A.disp_D = 0;
    const size_t n = (size_t)D * (size_t)h->cap * sizeof(double);
    if (hipMalloc((void**)&A.flights, SCP_AUDIT_WIDTH * n) != hipSuccess || hipMalloc((void**)&A.dx0, (size_t)h->info.nx * n) != hipSuccess ||
        hipMalloc((void**)&A.ugain, (size_t)h->info.nu * n) != hipSuccess || hipMalloc((void**)&A.ubias, (size_t)h->info.nu * n) != hipSuccess) {
        (void)hipGetLastError();
        for (double** p : {&A.flights, &A.dx0, &A.ugain, &A.ubias}) {
            if (*p) (void)hipFree(*p);
            *p = nullptr;
        }
        h->err = "audit: the buffers of " + std::to_string(D) + " flights per problem could not be allocated";
        return SCP_ERR_ALLOC;
    }
    A.disp_D = D;
    return SCP_OK;
}

// The run of a D-flight audit (dispersed, tracking): the dispersions to the device, `launch` -- the two kernels of the audit, given
// the staged arrays (nullptr where the caller passed none) and the shared flag -- between the handle's two events, then the copies.
template <class Launch>
static int audit_flights_run(scp_problem* h, int B, int D, const double* dx0, const double* ugain, const double* ubias, unsigned flags,
                             double* summary, double* flights, double* seconds, Launch&& launch)
{
    TRY(audit_dispersed_reserve(h, D));
    const bool shared = (flags & SCP_DISP_SHARED) != 0u;
    const size_t cols = shared ? (size_t)D : (size_t)D * (size_t)B;
    if (dx0) HIP_TRY(h, hipMemcpyAsync(h->audit.dx0, dx0, sizeof(double) * h->info.nx * cols, hipMemcpyHostToDevice, h->stream));
    if (ugain) HIP_TRY(h, hipMemcpyAsync(h->audit.ugain, ugain, sizeof(double) * h->info.nu * cols, hipMemcpyHostToDevice, h->stream));
    if (ubias) HIP_TRY(h, hipMemcpyAsync(h->audit.ubias, ubias, sizeof(double) * h->info.nu * cols, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipEventRecord(h->timing.ev0, h->stream));
    const int rc = launch(shared ? 1 : 0, dx0 ? h->audit.dx0 : nullptr, ugain ? h->audit.ugain : nullptr, ubias ? h->audit.ubias : nullptr);
    if (rc != SCP_OK) { h->err = "audit: kernel launch failed"; return rc; }
    HIP_TRY(h, hipEventRecord(h->timing.ev1, h->stream));
    HIP_TRY(h, hipMemcpyAsync(summary, h->audit.rec, sizeof(double) * SCP_AUDIT_WIDTH * (size_t)B, hipMemcpyDeviceToHost, h->stream));
    if (flights)
        HIP_TRY(h, hipMemcpyAsync(flights, h->audit.flights, sizeof(double) * SCP_AUDIT_WIDTH * (size_t)D * (size_t)B, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    stamps_collect(h);
    return elapsed_out(h, seconds);
}

static int audit_dispersed_run(scp_problem* h, int B, const Traj& tr, const double* d_pp, const int* mask, int res, double viol_tol,
                               int D, const double* dx0, const double* ugain, const double* ubias, unsigned flags,
                               const double* par_true, double* summary, double* flights, double* seconds)
{
    return audit_flights_run(h, B, D, dx0, ugain, ubias, flags, summary, flights, seconds,
                             [&](int shared, const double* d_dx0, const double* d_ugain, const double* d_ubias) {
        AuditDispersedArgs a;
        a.B = B; a.N = h->N; a.res = res; a.D = D; a.shared = shared; a.viol_tol = viol_tol; a.xd = tr.xd; a.ud = tr.ud; a.p = tr.p;
        a.pp = d_pp; a.Sx = h->d_Sx; a.dx0 = d_dx0; a.ugain = d_ugain; a.ubias = d_ubias; a.mask = mask; a.flights = h->audit.flights;
        a.audit = h->audit.rec;
        // the truth model: the blob the flights are flown with; like the handle's own it is taken as given
        return audit_dispersed_launch(h->model_id, par_true ? par_true : h->par.data(), a, h->stream);
    });
}

extern "C" int scp_audit_dispersed_batch_host(scp_handle h, int B, const double* xd, const double* ud, const double* p, const double* pp,
                                              int res, double viol_tol, int D, const double* dx0, const double* ugain,
                                              const double* ubias, unsigned flags, const double* par_true, double* summary,
                                              double* flights, double* seconds)
{
    TRY(audit_dispersed_begin(h, res, D, flags, summary));
    TRY(audit_stage_host(h, B, xd, ud, p, pp));
    return audit_dispersed_run(h, B, traj_sol(h), h->audit.pp, nullptr, res, viol_tol, D, dx0, ugain, ubias, flags, par_true, summary,
                               flights, seconds);
}

extern "C" int scp_audit_dispersed_resident(scp_handle h, int res, double viol_tol, int D, const double* dx0, const double* ugain,
                                            const double* ubias, unsigned flags, const double* par_true, double* summary,
                                            double* flights, double* seconds)
{
    TRY(audit_dispersed_begin(h, res, D, flags, summary));
    AuditSource src;
    TRY(audit_resident_source(h, "scp_audit_dispersed_resident: no run owns the handle's trajectory buffers; start one with its init", &src));
    return audit_dispersed_run(h, src.B, src.tr, src.d_pp, h->audit.mask, res, viol_tol, D, dx0, ugain, ubias, flags, par_true, summary,
                               flights, seconds);
}

// ------------------------------------------------------------------------------------------
// LQR gains on the discretisation (lqr_kernel.hpp; the kernels live in lqr_api.hip) and the closed-loop tracking audit
// ------------------------------------------------------------------------------------------

// the buffers of h->lqr but Kin for every problem the handle can hold: all or none
static int lqr_reserve(scp_problem* h)
{
    scp_problem::Lqr& q = h->lqr;
    if (q.K) return SCP_OK;
    const size_t nx = h->info.nx, nu = h->info.nu, npF = h->info.npF > 0 ? h->info.npF : 1, M = h->N - 1, cap = h->cap, D = sizeof(double);
    const bool ok = hipMalloc((void**)&q.dyn.A, nx * nx * M * cap * D) == hipSuccess && hipMalloc((void**)&q.dyn.Bm, nx * nu * M * cap * D) == hipSuccess &&
                    hipMalloc((void**)&q.dyn.Bp, nx * nu * M * cap * D) == hipSuccess && hipMalloc((void**)&q.dyn.F, nx * npF * M * cap * D) == hipSuccess &&
                    hipMalloc((void**)&q.dyn.r, nx * M * cap * D) == hipSuccess && hipMalloc((void**)&q.dyn.E, nx * nx * M * cap * D) == hipSuccess &&
                    hipMalloc((void**)&q.dyn.defect, nx * M * cap * D) == hipSuccess && hipMalloc((void**)&q.feas, cap * sizeof(int)) == hipSuccess &&
                    hipMalloc((void**)&q.info, SCP_LQR_INFO_WIDTH * cap * D) == hipSuccess &&
                    hipMalloc((void**)&q.w, (2 * nx + nu) * D) == hipSuccess && hipMalloc((void**)&q.K, nu * nx * M * cap * D) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        for (void** p : {(void**)&q.dyn.A, (void**)&q.dyn.Bm, (void**)&q.dyn.Bp, (void**)&q.dyn.F, (void**)&q.dyn.r, (void**)&q.dyn.E,
                         (void**)&q.dyn.defect, (void**)&q.feas, (void**)&q.info, (void**)&q.w, (void**)&q.K}) {
            if (*p) (void)hipFree(*p);
            *p = nullptr;
        }
        h->err = "lqr: the discretisation and gain buffers could not be allocated";
        return SCP_ERR_ALLOC;
    }
    return SCP_OK;
}

// what both gains entry points refuse (the audit's refusals, and the weights)
static int lqr_begin(scp_problem* h, const double* qx, const double* ru, const double* qf, const double* info)
{
    TRY(audit_begin(h, 2, info));
    if (!lqr_weights_ok(h->info.nx, h->info.nu, qx, ru, qf)) {
        h->err = "lqr: qx >= 0, qf >= 0 and ru > 0, all finite, are required";
        return SCP_ERR_BAD_ARGUMENT;
    }
    return lqr_reserve(h);
}

// discretize! about `tr` into the buffers of h->lqr and the Riccati kernel between the handle's two events, then the copies
static int lqr_run(scp_problem* h, int B, const Traj& tr, const int* mask, const double* qx, const double* ru, const double* qf,
                   double* K, double* info, double* seconds)
{
    scp_problem::Lqr& q = h->lqr;
    const size_t nx = h->info.nx, nu = h->info.nu;
    q.B = 0;
    std::vector<double> w(2 * nx + nu);
    std::copy(qx, qx + nx, w.begin()); std::copy(ru, ru + nu, w.begin() + nx); std::copy(qf, qf + nx, w.begin() + nx + nu);
    HIP_TRY(h, hipMemcpyAsync(q.w, w.data(), sizeof(double) * w.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipEventRecord(h->timing.ev0, h->stream));
    TRY(discretize_dev(h, B, tr.xd, tr.ud, tr.p, q.dyn, q.feas, mask));
    LqrArgs a;
    a.B = B; a.N = h->N; a.A = q.dyn.A; a.Bm = q.dyn.Bm; a.Bp = q.dyn.Bp; a.qx = q.w; a.ru = q.w + nx; a.qf = q.w + nx + nu; a.mask = mask;
    a.K = q.K; a.info = q.info;
    const int rc = lqr_launch((int)nx, (int)nu, a, h->stream);
    if (rc != SCP_OK) { h->err = "lqr: kernel launch failed"; return rc; }
    HIP_TRY(h, hipEventRecord(h->timing.ev1, h->stream));
    HIP_TRY(h, hipMemcpyAsync(info, q.info, sizeof(double) * SCP_LQR_INFO_WIDTH * (size_t)B, hipMemcpyDeviceToHost, h->stream));
    if (K) HIP_TRY(h, hipMemcpyAsync(K, q.K, sizeof(double) * nu * nx * (size_t)(h->N - 1) * (size_t)B, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));      // w is on this stack frame
    stamps_collect(h);
    q.B = B;
    return elapsed_out(h, seconds);
}

extern "C" int scp_lqr_gains_batch_host(scp_handle h, int B, const double* xd, const double* ud, const double* p, const double* qx,
                                        const double* ru, const double* qf, double* K, double* info, double* seconds)
{
    TRY(lqr_begin(h, qx, ru, qf, info));
    if (B < 1 || !xd || !ud || (h->npt > 0 && !p)) { h->err = "lqr: missing input"; return SCP_ERR_BAD_ARGUMENT; }
    if (B > h->cap) { h->err = "batch size exceeds batch_capacity"; return SCP_ERR_BATCH_TOO_LARGE; }
    TRY(upload_traj(h, B, xd, ud, p, h->traj.sol_xd, h->traj.sol_ud, h->traj.sol_p));
    return lqr_run(h, B, traj_sol(h), nullptr, qx, ru, qf, K, info, seconds);
}

extern "C" int scp_lqr_gains_resident(scp_handle h, const double* qx, const double* ru, const double* qf, double* K, double* info,
                                      double* seconds)
{
    TRY(lqr_begin(h, qx, ru, qf, info));
    AuditSource src;
    TRY(audit_resident_source(h, "scp_lqr_gains_resident: no run owns the handle's trajectory buffers; start one with its init", &src));
    return lqr_run(h, src.B, src.tr, h->audit.mask, qx, ru, qf, K, info, seconds);
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
        if (!h->lqr.Kin && hipMalloc((void**)&h->lqr.Kin, sizeof(double) * h->info.nu * h->info.nx * (size_t)(h->N - 1) * (size_t)h->cap) != hipSuccess) {
            (void)hipGetLastError();
            h->lqr.Kin = nullptr;
            h->err = "audit: the buffer of the gains passed by the caller could not be allocated";
            return SCP_ERR_ALLOC;
        }
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

static int audit_tracking_run(scp_problem* h, int B, const Traj& tr, const double* d_pp, const int* mask, const double* K, int steps,
                              double viol_tol, int D, const double* dx0, const double* ugain, const double* ubias, unsigned flags,
                              const double* par_true, double* summary, double* flights, double* seconds)
{
    const double* d_K = nullptr;
    TRY(audit_tracking_gains(h, B, K, &d_K));
    return audit_flights_run(h, B, D, dx0, ugain, ubias, flags, summary, flights, seconds,
                             [&](int shared, const double* d_dx0, const double* d_ugain, const double* d_ubias) {
        AuditTrackingArgs a;
        a.B = B; a.N = h->N; a.steps = steps; a.D = D; a.shared = shared; a.viol_tol = viol_tol; a.xd = tr.xd; a.ud = tr.ud; a.p = tr.p;
        a.pp = d_pp; a.Sx = h->d_Sx; a.Su = h->d_Su; a.K = d_K; a.dx0 = d_dx0; a.ugain = d_ugain; a.ubias = d_ubias; a.mask = mask;
        a.flights = h->audit.flights; a.audit = h->audit.rec;
        return audit_tracking_launch(h->model_id, par_true ? par_true : h->par.data(), a, h->stream);
    });
}

extern "C" int scp_audit_tracking_batch_host(scp_handle h, int B, const double* xd, const double* ud, const double* p, const double* pp,
                                             const double* K, int steps, double viol_tol, int D, const double* dx0, const double* ugain,
                                             const double* ubias, unsigned flags, const double* par_true, double* summary,
                                             double* flights, double* seconds)
{
    TRY(audit_tracking_begin(h, steps, D, flags, summary));
    TRY(audit_stage_host(h, B, xd, ud, p, pp));
    return audit_tracking_run(h, B, traj_sol(h), h->audit.pp, nullptr, K, steps, viol_tol, D, dx0, ugain, ubias, flags, par_true, summary,
                              flights, seconds);
}

extern "C" int scp_audit_tracking_resident(scp_handle h, const double* K, int steps, double viol_tol, int D, const double* dx0,
                                           const double* ugain, const double* ubias, unsigned flags, const double* par_true,
                                           double* summary, double* flights, double* seconds)
{
    TRY(audit_tracking_begin(h, steps, D, flags, summary));
    AuditSource src;
    TRY(audit_resident_source(h, "scp_audit_tracking_resident: no run owns the handle's trajectory buffers; start one with its init", &src));
    return audit_tracking_run(h, src.B, src.tr, src.d_pp, h->audit.mask, K, steps, viol_tol, D, dx0, ugain, ubias, flags, par_true, summary,
                              flights, seconds);
}

// ------------------------------------------------------------------------------------------
// closed-loop covariance audit (cov_kernel.hpp; the kernels live in cov_api.hip)
// ------------------------------------------------------------------------------------------

// the buffers of h->cov for every problem the handle can hold: all or none
static int cov_reserve(scp_problem* h)
{
    scp_problem::Cov& c = h->cov;
    if (c.rows) return SCP_OK;
    const size_t nx = h->info.nx, nu = h->info.nu, nrow = (size_t)h->info.ns + h->info.nl + h->info.nsoc, ntc = h->info.ntc, N = h->N,
                 cap = h->cap, D = sizeof(double);
    const bool ok = hipMalloc((void**)&c.rows, std::max<size_t>((nx + 1) * nrow * N * cap, 1) * D) == hipSuccess &&
                    hipMalloc((void**)&c.Hf, std::max<size_t>(ntc * nx * cap, 1) * D) == hipSuccess &&
                    hipMalloc((void**)&c.rec, SCP_COV_WIDTH * cap * D) == hipSuccess && hipMalloc((void**)&c.sig, nx * N * cap * D) == hipSuccess &&
                    hipMalloc((void**)&c.nodes, SCP_COV_NODE_WIDTH * N * cap * D) == hipSuccess && hipMalloc((void**)&c.w, (2 * nx + nu) * D) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        for (double** p : {&c.rows, &c.Hf, &c.rec, &c.sig, &c.nodes, &c.w}) {
            if (*p) (void)hipFree(*p);
            *p = nullptr;
        }
        h->err = "audit: the row table and the records of the covariance audit could not be allocated";
        return SCP_ERR_ALLOC;
    }
    return SCP_OK;
}

// what both covariance entry points refuse (the audit's refusals, and the dispersions), and the buffers of the call
static int cov_begin(scp_problem* h, const double* sig0, const double* sigu, const double* sigw, double nsig, const double* summary)
{
    TRY(audit_begin(h, 2, summary));
    if (!cov_sigmas_ok(h->info.nx, h->info.nu, sig0, sigu, sigw, nsig)) {
        h->err = "audit: sig0 >= 0, sigu >= 0, sigw >= 0, all finite, and a finite nsig > 0 are required";
        return SCP_ERR_BAD_ARGUMENT;
    }
    TRY(lqr_reserve(h));
    return cov_reserve(h);
}

// discretize! about `tr` into the buffers of h->lqr, the row pre-pass and the chain between the handle's two events, then the copies
static int cov_run(scp_problem* h, int B, const Traj& tr, const double* d_pp, const int* mask, const double* K, const double* sig0,
                   const double* sigu, const double* sigw, double nsig, double* summary, double* sig, double* nodes, double* seconds)
{
    scp_problem::Lqr& q = h->lqr;
    scp_problem::Cov& c = h->cov;
    const size_t nx = h->info.nx, nu = h->info.nu, N = h->N;
    const double* d_K = nullptr;
    TRY(audit_tracking_gains(h, B, K, &d_K));
    std::vector<double> w(2 * nx + nu);
    std::copy(sig0, sig0 + nx, w.begin()); std::copy(sigu, sigu + nu, w.begin() + nx); std::copy(sigw, sigw + nx, w.begin() + nx + nu);
    HIP_TRY(h, hipMemcpyAsync(c.w, w.data(), sizeof(double) * w.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipEventRecord(h->timing.ev0, h->stream));
    TRY(discretize_dev(h, B, tr.xd, tr.ud, tr.p, q.dyn, q.feas, mask));
    CovArgs a;
    a.B = B; a.N = h->N; a.nrow[0] = h->info.ns; a.nrow[1] = h->info.nl; a.nrow[2] = h->info.nsoc; a.ntc = h->info.ntc; a.nsig = nsig;
    a.xd = tr.xd; a.ud = tr.ud; a.p = tr.p; a.pp = d_pp; a.A = q.dyn.A; a.Bm = q.dyn.Bm; a.Bp = q.dyn.Bp; a.K = d_K;
    a.Sx = h->d_Sx; a.Su = h->d_Su; a.sig0 = c.w; a.sigu = c.w + nx; a.sigw = c.w + nx + nu; a.mask = mask;
    a.rows = c.rows; a.Hf = c.Hf; a.summary = c.rec; a.sig = sig ? c.sig : nullptr; a.nodes = nodes ? c.nodes : nullptr;
    const int rc = cov_launch(h->model_id, h->par.data(), a, h->stream);
    if (rc != SCP_OK) { h->err = "audit: kernel launch failed"; return rc; }
    HIP_TRY(h, hipEventRecord(h->timing.ev1, h->stream));
    HIP_TRY(h, hipMemcpyAsync(summary, c.rec, sizeof(double) * SCP_COV_WIDTH * (size_t)B, hipMemcpyDeviceToHost, h->stream));
    if (sig) HIP_TRY(h, hipMemcpyAsync(sig, c.sig, sizeof(double) * nx * N * (size_t)B, hipMemcpyDeviceToHost, h->stream));
    if (nodes) HIP_TRY(h, hipMemcpyAsync(nodes, c.nodes, sizeof(double) * SCP_COV_NODE_WIDTH * N * (size_t)B, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));      // w is on this stack frame
    stamps_collect(h);
    return elapsed_out(h, seconds);
}

extern "C" int scp_audit_covariance_batch_host(scp_handle h, int B, const double* xd, const double* ud, const double* p, const double* pp,
                                               const double* K, const double* sig0, const double* sigu, const double* sigw, double nsig,
                                               double* summary, double* sig, double* nodes, double* seconds)
{
    TRY(cov_begin(h, sig0, sigu, sigw, nsig, summary));
    TRY(audit_stage_host(h, B, xd, ud, p, pp));
    return cov_run(h, B, traj_sol(h), h->audit.pp, nullptr, K, sig0, sigu, sigw, nsig, summary, sig, nodes, seconds);
}

extern "C" int scp_audit_covariance_resident(scp_handle h, const double* K, const double* sig0, const double* sigu, const double* sigw,
                                             double nsig, double* summary, double* sig, double* nodes, double* seconds)
{
    TRY(cov_begin(h, sig0, sigu, sigw, nsig, summary));
    AuditSource src;
    TRY(audit_resident_source(h, "scp_audit_covariance_resident: no run owns the handle's trajectory buffers; start one with its init", &src));
    return cov_run(h, src.B, src.tr, src.d_pp, h->audit.mask, K, sig0, sigu, sigw, nsig, summary, sig, nodes, seconds);
}

// ------------------------------------------------------------------------------------------
// Monte-Carlo audit (mc_kernel.hpp; the kernels live in mc_api.hip)
// ------------------------------------------------------------------------------------------

// the buffers of h->mc for W wavefronts per problem and every problem the handle can hold: all or none
static int mc_reserve(scp_problem* h, int W)
{
    scp_problem::Mc& c = h->mc;
    if (W <= c.W) return SCP_OK;
    for (double** p : {&c.part, &c.moments, &c.stat, &c.w}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    c.W = 0;
    const size_t nx = h->info.nx, nu = h->info.nu, nv = 1 + 2 * nx + nu, N = h->N, cap = h->cap, D = sizeof(double);
    const bool ok = hipMalloc((void**)&c.part, nv * N * (size_t)W * cap * D) == hipSuccess && hipMalloc((void**)&c.moments, nv * N * cap * D) == hipSuccess &&
                    hipMalloc((void**)&c.stat, SCP_MC_STAT_WIDTH * cap * D) == hipSuccess && hipMalloc((void**)&c.w, (2 * nx + nu) * D) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        for (double** p : {&c.part, &c.moments, &c.stat, &c.w}) {
            if (*p) (void)hipFree(*p);
            *p = nullptr;
        }
        h->err = "audit: the partial sums and the records of the Monte-Carlo audit could not be allocated";
        return SCP_ERR_ALLOC;
    }
    c.W = W;
    return SCP_OK;
}

// what both Monte-Carlo entry points refuse (the tracking audit's refusals, D < 2, the dispersions, a NULL stat)
static int mc_begin(scp_problem* h, int steps, int D, const double* sig0, const double* sigu, const double* sigw, const double* summary,
                    const double* stat)
{
    TRY(audit_tracking_begin(h, steps, D, 0u, summary));
    if (D < 2 || !stat) { h->err = "audit: D >= 2 flights and the stat array are required"; return SCP_ERR_BAD_ARGUMENT; }
    if (!mc_sigmas_ok(h->info.nx, h->info.nu, sig0, sigu, sigw)) {
        h->err = "audit: sig0 >= 0, sigu >= 0, sigw >= 0, all finite, are required";
        return SCP_ERR_BAD_ARGUMENT;
    }
    return SCP_OK;
}

// the three kernels between the handle's two events, then the copies
static int mc_run(scp_problem* h, int B, const Traj& tr, const double* d_pp, const int* mask, const double* K, int steps, double viol_tol,
                  int D, uint64_t seed, const double* sig0, const double* sigu, const double* sigw, double* summary, double* stat,
                  double* moments, double* flights, double* seconds)
{
    scp_problem::Mc& c = h->mc;
    const size_t nx = h->info.nx, nu = h->info.nu, nv = 1 + 2 * nx + nu, N = h->N;
    const int W = (D + 63) / 64;
    const double* d_K = nullptr;
    TRY(audit_tracking_gains(h, B, K, &d_K));
    TRY(audit_dispersed_reserve(h, D));
    TRY(mc_reserve(h, W));
    std::vector<double> w(2 * nx + nu);
    std::copy(sig0, sig0 + nx, w.begin()); std::copy(sigu, sigu + nu, w.begin() + nx); std::copy(sigw, sigw + nx, w.begin() + nx + nu);
    HIP_TRY(h, hipMemcpyAsync(c.w, w.data(), sizeof(double) * w.size(), hipMemcpyHostToDevice, h->stream));
    McArgs a;
    a.B = B; a.N = h->N; a.steps = steps; a.D = D; a.W = W; a.seed = seed; a.viol_tol = viol_tol; a.xd = tr.xd; a.ud = tr.ud; a.p = tr.p;
    a.pp = d_pp; a.Sx = h->d_Sx; a.Su = h->d_Su; a.K = d_K; a.sig0 = c.w; a.sigu = c.w + nx; a.sigw = c.w + nx + nu; a.mask = mask;
    a.flights = h->audit.flights; a.audit = h->audit.rec; a.part = c.part; a.moments = c.moments; a.stat = c.stat;
    HIP_TRY(h, hipEventRecord(h->timing.ev0, h->stream));
    const int rc = mc_launch(h->model_id, h->par.data(), a, h->stream);
    if (rc != SCP_OK) { h->err = "audit: kernel launch failed"; return rc; }
    HIP_TRY(h, hipEventRecord(h->timing.ev1, h->stream));
    HIP_TRY(h, hipMemcpyAsync(summary, h->audit.rec, sizeof(double) * SCP_AUDIT_WIDTH * (size_t)B, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(stat, c.stat, sizeof(double) * SCP_MC_STAT_WIDTH * (size_t)B, hipMemcpyDeviceToHost, h->stream));
    if (moments) HIP_TRY(h, hipMemcpyAsync(moments, c.moments, sizeof(double) * nv * N * (size_t)B, hipMemcpyDeviceToHost, h->stream));
    if (flights)
        HIP_TRY(h, hipMemcpyAsync(flights, h->audit.flights, sizeof(double) * SCP_AUDIT_WIDTH * (size_t)D * (size_t)B, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));      // w is on this stack frame
    stamps_collect(h);
    return elapsed_out(h, seconds);
}

extern "C" int scp_audit_montecarlo_batch_host(scp_handle h, int B, const double* xd, const double* ud, const double* p, const double* pp,
                                               const double* K, int steps, double viol_tol, int D, uint64_t seed, const double* sig0,
                                               const double* sigu, const double* sigw, double* summary, double* stat, double* moments,
                                               double* flights, double* seconds)
{
    TRY(mc_begin(h, steps, D, sig0, sigu, sigw, summary, stat));
    TRY(audit_stage_host(h, B, xd, ud, p, pp));
    return mc_run(h, B, traj_sol(h), h->audit.pp, nullptr, K, steps, viol_tol, D, seed, sig0, sigu, sigw, summary, stat, moments, flights,
                  seconds);
}

extern "C" int scp_audit_montecarlo_resident(scp_handle h, const double* K, int steps, double viol_tol, int D, uint64_t seed,
                                             const double* sig0, const double* sigu, const double* sigw, double* summary, double* stat,
                                             double* moments, double* flights, double* seconds)
{
    TRY(mc_begin(h, steps, D, sig0, sigu, sigw, summary, stat));
    AuditSource src;
    TRY(audit_resident_source(h, "scp_audit_montecarlo_resident: no run owns the handle's trajectory buffers; start one with its init", &src));
    return mc_run(h, src.B, src.tr, src.d_pp, h->audit.mask, K, steps, viol_tol, D, seed, sig0, sigu, sigw, summary, stat, moments, flights,
                  seconds);
}
