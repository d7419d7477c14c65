// The initial guesses of the C-ABI library (include/scp_mi355x.h): traj.guess(N) of every compiled model on the device and the
// reference's own Starship guess (starship_guess.hpp).  Owns h->guess (scp_handle.hpp).  A unit of its own because the Starship guess
// solves its descent programs with the conic engine: next to K3 every change of the conic solver's headers would rebuild K3.
#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "scp_handle.hpp"
#include "guess_kernel.hpp"
#include "starship_guess.hpp"

using namespace scp;

// traj.guess(N) of the handle's model on the device (ptr_guess_kernel: the model's own straight-line rule)
int scp::guess_dev(scp_problem* h, const GuessArgs& g)
{
    TRY(with_model(h->model_id, [&](auto m) -> int {
        using M = decltype(m);
        const long n = (long)g.B * g.N;
        hipLaunchKernelGGL(ptr_guess_kernel<M>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, g, M::make_params(h->par.data()));
        return (int)SCP_OK;
    }));
    HIP_TRY(h, hipGetLastError());
    return SCP_OK;
}

// ---- the reference's Starship guess on the device (starship_guess.hpp): flip simulation -> batched descent programs -> reconstruction ----
struct StarshipGuessState {
    scp::conic::Engine eng;
    scp::SgPattern pat;
    int chunk = 0;                       // instances per conic launch
    std::vector<void*> allocs;
    int *a_kind = nullptr, *a_i = nullptr, *a_j = nullptr, *g_kind = nullptr, *b_kind = nullptr, *b_i = nullptr, *h_kind = nullptr;
    int *a_row = nullptr, *g_row = nullptr, *gs_kind = nullptr;
    double *g_val = nullptr, *h_val = nullptr, *lti = nullptr, *gs_val = nullptr;
    double *xs = nullptr, *t1 = nullptr;
    int *ok1 = nullptr, *active = nullptr, *fail = nullptr;
    double Su[2], cu[2];
    int n1 = 0, N2 = 0, id_sw = 0;
};
void scp::starship_guess_free(StarshipGuessState* g)
{
    if (!g) return;
    g->eng.destroy();
    for (void* p : g->allocs) (void)hipFree(p);
    delete g;
}
template <class T>
static int sg_upload(scp_problem* h, StarshipGuessState* g, T** dst, const std::vector<T>& v)
{
    void* d = nullptr;
    HIP_TRY(h, hipMalloc(&d, std::max<size_t>(v.size(), 1) * sizeof(T)));
    g->allocs.push_back(d);
    if (!v.empty()) HIP_TRY(h, hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *dst = (T*)d;
    return SCP_OK;
}
static int starship_guess_dev(scp_problem* h, int B, const double* d_pp, double* d_xd, double* d_ud, double* d_p)
{
    using namespace scp;
    const Starship::Params K = Starship::make_params(h->par.data());
    const int N = h->N;
    if (!h->guess.sg) {
        // built into a local object and published in h->guess.sg only after EVERY step succeeded: a half-built state (chunk = 0, null
        // device arrays, engine not created) must never be seen by the next call on this handle
        StarshipGuessState* g = new (std::nothrow) StarshipGuessState;
        if (!g) return SCP_ERR_ALLOC;
        struct Guard { StarshipGuessState* g; ~Guard() { if (g) starship_guess_free(g); } } guard{g};
        // grid split (definition.jl:108-113): id1 = {k: tau_k <= tau_s}, id2 = id1[end] .. N
        int n1 = 0;
        for (int k = 0; k < N; k++) { const double t = (double)k / (double)(N - 1); if ((1.0 - t) * 0.0 + t * 1.0 <= K.tau_s) n1 = k + 1; }
        if (n1 < 2 || n1 >= N) { h->err = "starship guess: the grid has no node on both sides of tau_s"; return SCP_ERR_BAD_ARGUMENT; }
        g->n1 = n1; g->id_sw = n1 - 1; g->N2 = N - g->id_sw;
        const double Tmax_x = K.T_max1 * std::sin(K.theta_max2);
        sg_scale(-Tmax_x, Tmax_x, g->Su[0], g->cu[0]); sg_scale(K.T_min1, K.T_max1, g->Su[1], g->cu[1]);
        g->pat = sg_build_pattern(g->N2, g->Su, g->cu, K.T_min1, K.T_max1, K.theta_max2);
        // FOH models of the candidate durations: one normalised interval of the phase-2 grid
        auto tau = [&](int k) { const double t = (double)k / (double)(N - 1); return (1.0 - t) * 0.0 + t * 1.0; };
        const double dtn = (tau(g->id_sw + 1) - tau(g->id_sw)) - (tau(g->id_sw) - tau(g->id_sw));
        std::vector<double> lti((size_t)SG_NCAND * 36);
        for (int c = 0; c < SG_NCAND; c++) {
            double o[36];
            sg_descent_lti(dtn, (10.0 + c) / (1.0 - K.tau_s), K.m, K.g0, o);
            std::copy(o, o + 36, lti.begin() + (size_t)c * 36);
        }
        g->chunk = std::min(h->cap, 256);
        const conic::Csc Pm = conic::make_csc(g->pat.n, g->pat.n, nullptr, nullptr);   // no quadratic cost
        int rc = g->eng.create(g->pat.n, g->pat.p, g->pat.m, g->pat.l, g->pat.q, Pm, g->pat.A, g->pat.G, nullptr, g->chunk * SG_NCAND, h->device);
        if (rc != SCP_OK) { h->err = "starship guess: " + g->eng.err; return rc; }
        TRY(sg_upload(h, g, &g->a_kind, g->pat.a_kind)); TRY(sg_upload(h, g, &g->a_i, g->pat.a_i)); TRY(sg_upload(h, g, &g->a_j, g->pat.a_j));
        TRY(sg_upload(h, g, &g->g_kind, g->pat.g_kind)); TRY(sg_upload(h, g, &g->g_val, g->pat.g_val));
        TRY(sg_upload(h, g, &g->b_kind, g->pat.b_kind)); TRY(sg_upload(h, g, &g->b_i, g->pat.b_i));
        TRY(sg_upload(h, g, &g->h_kind, g->pat.h_kind)); TRY(sg_upload(h, g, &g->h_val, g->pat.h_val));
        TRY(sg_upload(h, g, &g->lti, lti));
        TRY(sg_upload(h, g, &g->a_row, g->pat.A.i)); TRY(sg_upload(h, g, &g->g_row, g->pat.G.i));
        TRY(sg_upload(h, g, &g->gs_kind, g->pat.gs_kind)); TRY(sg_upload(h, g, &g->gs_val, g->pat.gs_val));
        TRY(sg_upload(h, g, &g->xs, std::vector<double>((size_t)8 * h->cap, 0.0))); TRY(sg_upload(h, g, &g->t1, std::vector<double>((size_t)h->cap, 0.0)));
        TRY(sg_upload(h, g, &g->ok1, std::vector<int>((size_t)h->cap, 0))); TRY(sg_upload(h, g, &g->fail, std::vector<int>((size_t)h->cap, 0)));
        TRY(sg_upload(h, g, &g->active, std::vector<int>((size_t)g->chunk * SG_NCAND, 0)));
        if (g->chunk <= 0) { h->err = "starship guess: empty batch capacity"; return SCP_ERR_BAD_ARGUMENT; }
        h->guess.sg = g;
        guard.g = nullptr;
    }
    StarshipGuessState* g = h->guess.sg;
    SgDev a;
    a.B = B; a.N = N; a.n1 = g->n1; a.N2 = g->N2; a.id_sw = g->id_sw; a.pp = d_pp; a.xd = d_xd; a.ud = d_ud; a.p = d_p;
    a.xs = g->xs; a.t1 = g->t1; a.ok1 = g->ok1;
    hipLaunchKernelGGL(starship_flip_kernel, dim3((B + 63) / 64), dim3(64), 0, h->stream, a, K);
    HIP_TRY(h, hipGetLastError());
    SgProg P;
    P.n = g->pat.n; P.p = g->pat.p; P.m = g->pat.m; P.l = g->pat.l; P.nnzA = g->pat.A.nnz(); P.nnzG = g->pat.G.nnz(); P.N2 = g->N2;
    P.a_kind = g->a_kind; P.a_i = g->a_i; P.a_j = g->a_j; P.g_kind = g->g_kind; P.g_val = g->g_val; P.b_kind = g->b_kind; P.b_i = g->b_i;
    P.h_kind = g->h_kind; P.h_val = g->h_val; P.lti = g->lti;
    P.a_row = g->a_row; P.g_row = g->g_row; P.gs_kind = g->gs_kind; P.gs_val = g->gs_val;
    P.Su[0] = g->Su[0]; P.Su[1] = g->Su[1]; P.cu[0] = g->cu[0]; P.cu[1] = g->cu[1]; P.vf[0] = K.vf_x; P.vf[1] = K.vf_y;
    conic::Opts o = conic::default_opts();
    o.nref = 30;      // feasibility programs (zero cost, variables held by equality rows only) need more refinement steps (models.py)
    for (int b0 = 0; b0 < B; b0 += g->chunk) {
        const int nb = std::min(g->chunk, B - b0);
        SgFill f;
        f.B = nb; f.BS = g->eng.BS; f.xs = g->xs + (size_t)8 * b0; f.ok1 = g->ok1 + b0;
        f.c = g->eng.c; f.b = g->eng.b; f.h = g->eng.h; f.Gx = g->eng.Gx; f.Ax = g->eng.Ax; f.active = g->active;
        const long nt = (long)nb * SG_NCAND;
        hipLaunchKernelGGL(starship_descent_fill_kernel, dim3((unsigned)((nt + 63) / 64)), dim3(64), 0, h->stream, f, P);
        HIP_TRY(h, hipGetLastError());
        int rc = g->eng.launch(h->stream, (int)nt, o, 0u, g->active);
        if (rc != SCP_OK) { h->err = "starship guess: " + g->eng.err; return rc; }
        SgRec r;
        r.B = nb; r.N = N; r.n1 = g->n1; r.N2 = g->N2; r.id_sw = g->id_sw; r.BS = g->eng.BS; r.z = g->eng.x; r.status = g->eng.status;
        r.xs = g->xs + (size_t)8 * b0; r.t1 = g->t1 + b0; r.ok1 = g->ok1 + b0;
        r.xd = d_xd + (size_t)b0 * N * 8; r.ud = d_ud + (size_t)b0 * N * 3; r.p = d_p + (size_t)b0 * 10; r.fail = g->fail + b0;
        r.Su[0] = g->Su[0]; r.Su[1] = g->Su[1]; r.cu[0] = g->cu[0]; r.cu[1] = g->cu[1]; r.tau_s = K.tau_s; r.alpha_e = K.alpha_e;
        hipLaunchKernelGGL(starship_reconstruct_kernel, dim3((nb + 63) / 64), dim3(64), 0, h->stream, r);
        HIP_TRY(h, hipGetLastError());
    }
    // instances without a reference guess (no velocity crossing / no feasible descent duration: the reference raises an error,
    // definition.jl:163-167, 415-419) get the straight-line guess and are counted (scp_guess_failures)
    std::vector<int> fail(B);
    HIP_TRY(h, hipMemcpyAsync(fail.data(), g->fail, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    int nf = 0;
    for (int b = 0; b < B; b++) nf += fail[b] != 0;
    h->guess.failures = nf;
    if (nf > 0) {
        GuessArgs ga;
        ga.B = B; ga.N = N; ga.pp = d_pp; ga.xd = d_xd; ga.ud = d_ud; ga.p = d_p; ga.only = g->fail;
        hipLaunchKernelGGL(ptr_guess_kernel<Starship>, dim3((unsigned)(((long)B * N + 255) / 256)), dim3(256), 0, h->stream, ga, K);
        HIP_TRY(h, hipGetLastError());
    }
    return SCP_OK;
}

extern "C" int scp_guess_failures(scp_handle h) { return h ? h->guess.failures : -1; }

// traj.guess(N) of the compiled model for a Monte-Carlo batch, evaluated on the device for ANY registered model (the
// structured ones also have scp_ptr_init_guess_host, which keeps the guesses resident for a PTR run)
extern "C" int scp_guess_batch_host(scp_handle h, int B, const double* pp, double* xd, double* ud, double* p)
{
    if (!h || B < 1 || !xd || !ud) return SCP_ERR_BAD_ARGUMENT;
    if (B > h->cap) return SCP_ERR_BATCH_TOO_LARGE;
    if ((h->info.npp > 0 && !pp) || (h->npt > 0 && !p)) return SCP_ERR_BAD_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    // a pure query: its own scratch, so that a resident PTR / SCvx / GuSTO run (d_pp, sol_*) is left untouched
    const size_t nx = h->info.nx, nu = h->info.nu, np = h->npt, npp = h->info.npp, N = h->N, D = sizeof(double), b = B;
    if (!h->guess.q_pp) {
        TRY(dalloc(h, &h->guess.q_pp, (npp > 0 ? npp : 1) * (size_t)h->cap)); TRY(dalloc(h, &h->guess.q_xd, nx * N * h->cap));
        TRY(dalloc(h, &h->guess.q_ud, nu * N * h->cap)); TRY(dalloc(h, &h->guess.q_p, (np > 0 ? np : 1) * (size_t)h->cap));
    }
    if (npp > 0) HIP_TRY(h, hipMemcpyAsync(h->guess.q_pp, pp, npp * b * D, hipMemcpyHostToDevice, h->stream));
    GuessArgs g;
    g.B = B; g.N = h->N; g.pp = h->guess.q_pp; g.xd = h->guess.q_xd; g.ud = h->guess.q_ud; g.p = h->guess.q_p;
    h->guess.failures = 0;
    // Starship: the reference's own guess, bang-bang flip + convex terminal descent per instance (starship_guess.hpp)
    if (h->model_id == Starship::id) TRY(starship_guess_dev(h, B, h->guess.q_pp, h->guess.q_xd, h->guess.q_ud, h->guess.q_p));
    else TRY(guess_dev(h, g));
    HIP_TRY(h, hipMemcpyAsync(xd, h->guess.q_xd, nx * N * b * D, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(ud, h->guess.q_ud, nu * N * b * D, hipMemcpyDeviceToHost, h->stream));
    if (np > 0) HIP_TRY(h, hipMemcpyAsync(p, h->guess.q_p, np * b * D, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SCP_OK;
}
