// C-ABI implementation (include/scp_mi355x.h) of the MI355X-native SCP inner loop: model queries, the handle's life cycle and
// services (scp_handle.hpp), discretize! and propagate (K1).  The handle-level audit entry points stand in audit_entry.hip.
// gfx950 only: no CUDA shims, no dual paths.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "scp_handle.hpp"
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

extern "C" int scp_problem_destroy(scp_handle h)
{
    if (!h) return SCP_ERR_BAD_ARGUMENT;
    (void)hipSetDevice(h->device);
    if (h->guess.sg) starship_guess_free(h->guess.sg);
    for (void* p : h->allocs) (void)hipFree(p);
    audit_release(h);
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
            if constexpr (M::has_impulse) {
                hipLaunchKernelGGL((discretize_foh_kernel<M, true>), dim3(blocks), dim3(256), 0, h->stream, a, P);
            } else {
                return (int)SCP_ERR_UNSUPPORTED;   // (scp_problem_create rejects IMPULSE for these models)
            }
        } else if (DiscForms<M>::k1v && !h->disc.reference_form && rk4_step <= M::var_form_max_step) {
            // variational form (K1v): thread per (problem, interval, column), blockIdx.y = column
            if constexpr (DiscForms<M>::k1v) {
                const unsigned gx = (unsigned)((groups + 255) / 256);
                hipLaunchKernelGGL((discretize_foh_var_kernel<M, false>), dim3(gx, 2 * M::nx + 2 * M::nu), dim3(256), 0, h->stream, a, P);
                hipLaunchKernelGGL((discretize_foh_var_kernel<M, true>), dim3(gx, M::npF + 1), dim3(256), 0, h->stream, a, P);
            }
        } else if constexpr (DiscForms<M>::k1x) {
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
            if constexpr (M::has_impulse) {
                const long tot = (long)B * (h->N - 1);
                hipLaunchKernelGGL(propagate_impulse_kernel<M>, dim3((unsigned)((tot + 63) / 64)), dim3(64), 0, h->stream, ai, P);
            } else {
                return (int)SCP_ERR_UNSUPPORTED;   // (scp_problem_create rejects IMPULSE for these models)
            }
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
