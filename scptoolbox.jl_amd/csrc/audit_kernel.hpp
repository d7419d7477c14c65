// Continuous-time audit of a solved batch: fly every solution open loop through the NONLINEAR dynamics (the propagation
// of SCPSolution(history), src/solvers/scp.jl:196-245: xc = propagate(last_sol, pbm; res)) and reduce, on the fly, what a
// user inspects afterwards -- the worst value of every constraint family BETWEEN the grid nodes, the open-loop terminal
// miss and the cost actually flown -- to one record of SCP_AUDIT_WIDTH doubles per problem (include/scp_mi355x.h).
//
// One body, audit_one<M>, serves the kernel and the host twin (scp_model_audit_host).  The state after each RK4 step is
// consumed in registers: nothing of size res * B exists anywhere.  The integration repeats propagate_foh_kernel
// (discretize_kernel.hpp) expression by expression -- same sample times, same interval search of the input
// interpolation, same stage order, M::action behind every step.
//
// The row matrices of the convex sets depend on (t, k) only.  They are built per sample by the model's own lin_rows /
// soc_rows into local arrays that are read with COMPILE-TIME indices only (every loop below is fully unrolled), so the
// arrays are promoted to registers and the time loop runs without scratch ("Continuous-time audit", has the
// compiler's resource report of the four instantiations).  Products with the structural zeros stay in the code -- 0 * NaN
// must remain NaN -- as plain FMAs.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/scp_mi355x.h"
#include "models/model_common.hpp"

namespace scp {

struct AuditArgs {
    int B, N, res;
    double viol_tol;
    const double* xd;   // [nx,N,B]
    const double* ud;   // [nu,N,B]
    const double* p;    // [np,B]
    const double* pp;   // [npp,B]
    const double* Sx;   // [nx] diagonal of the state scaling
    const int* mask;    // optional [B]: problems with mask[b] == 0 are skipped, their record is NaN
    double* audit;      // [SCP_AUDIT_WIDTH,B]
};

// audit_api.hip: launch audit_foh_kernel<M> of the model on `stream` (SCP_ERR_UNSUPPORTED for models with node parameters);
// mask[b] = (status[b] == 0), the "solved" code of every loop family
int audit_launch(int model_id, const double* model_par, const AuditArgs& a, hipStream_t stream);
int audit_mask_from_status(const int* status, int* mask, int B, hipStream_t stream);

// Julia LinRange(a,b,n)[j] (0-based j): the `linrange` of discretize_kernel.hpp, callable from the host twin too
SCP_DEV double audit_linrange(double a, double b, int n, int j)
{
    const double tt = (double)j / (double)(n - 1);
    return (1.0 - tt) * a + tt * b;
}

// xd[nx,N], ud[nu,N], p[np], pp[npp], Sx[nx] of ONE problem -> out[SCP_AUDIT_WIDTH]
template <class M>
SCP_DEV void audit_one(const typename M::Params& par, int N, int res, double viol_tol, const double* xd, const double* ub,
                       const double* pb, const double* pp, const double* Sx, double* out)
{
    static_assert(M::np_node == 0, "a row of node k would read that node's own parameters: undefined between the nodes");
    constexpr int nx = M::nx, nu = M::nu, nz = nx + nu, np = M::np, npa = np > 0 ? np : 1, npF = M::npF, npFa = npF > 0 ? npF : 1;
    constexpr int ns = M::ns, nsa = ns > 0 ? ns : 1, nl = M::nl, nla = nl > 0 ? nl : 1, nsoc = M::nsoc, nsoca = nsoc > 0 ? nsoc : 1;
    constexpr int ng = M::ng, nga = ng > 0 ? ng : 1, ntc = M::ntc, ntca = ntc > 0 ? ntc : 1;
    const double ninf = -INFINITY;

    double x[nx];
#pragma unroll
    for (int i = 0; i < nx; i++) x[i] = xd[i];
    // u(t) and f(t, x): propagate_foh_kernel's own
    auto input = [&](double t, double (&u)[nu]) {
        const double g0 = audit_linrange(0.0, 1.0, N, 0), g1 = audit_linrange(0.0, 1.0, N, N - 1);
        t = fmax(g0, fmin(g1, t));
        int k = (int)floor(t * (N - 1));
        k = k < 0 ? 0 : (k > N ? N : k);
        while (k < N && t > audit_linrange(0.0, 1.0, N, k)) k++;
        while (k > 0 && !(t > audit_linrange(0.0, 1.0, N, k - 1))) k--;
        if (k == 0) k = 1;
        const double ta = audit_linrange(0.0, 1.0, N, k - 1), tb = audit_linrange(0.0, 1.0, N, k);
        const double c = (tb - t) / (tb - ta);
#pragma unroll
        for (int i = 0; i < nu; i++) u[i] = c * ub[(long)(k - 1) * nu + i] + (1.0 - c) * ub[(long)k * nu + i];
    };
    auto f = [&](double t, const double (&xs)[nx], double (&fx)[nx]) {
        double u[nu], Am[nx * nx], Bmat[nx * nu], Fc[nx * npFa];
        input(t, u);
        M::dyn(par, t, N, xs, u, pb, fx, Am, Bmat, Fc);   // only f survives dead-code elimination
    };

    double Qu[nu], lu[nu], lx[nx], tx[nx], ctp[npa], cQp[npa];
#pragma unroll
    for (int i = 0; i < npa; i++) { ctp[i] = 0.0; cQp[i] = 0.0; }
    M::cost_terms(par, Qu, lu, lx, tx, ctp, cQp);

    double s_max = ninf, t_s = 0.0, l_max = ninf, t_l = 0.0, c_max = ninf, t_c = 0.0;
    double n_viol = 0.0, gam_prev = 0.0, cost_int = 0.0;
    bool bad = false;

    // everything that is evaluated AT a sample (t, x): returns the running cost Gamma there
    auto sample = [&](double t) -> double {
        // 1-based index of the last grid node <= t, decided against the exact grid values (N at t = 1)
        int k = (int)floor(t * (N - 1)) + 1;
        k = k < 1 ? 1 : (k > N ? N : k);
        while (k < N && !(audit_linrange(0.0, 1.0, N, k) > t)) k++;
        while (k > 1 && audit_linrange(0.0, 1.0, N, k - 1) > t) k--;
        double z[nz], u[nu];
        input(t, u);
#pragma unroll
        for (int i = 0; i < nx; i++) z[i] = x[i];
#pragma unroll
        for (int i = 0; i < nu; i++) z[nx + i] = u[i];
#pragma unroll
        for (int i = 0; i < nz; i++) bad = bad || !__builtin_isfinite(z[i]);
        double vs = ninf, vl = ninf, vc = ninf;
        if constexpr (ns > 0) {
            double s[nsa], C[nsa * nx], Dm[nsa * nu], G[nsa * npa];
            M::s_eval(par, t, k, x, u, pb, s, C, Dm, G);       // only s survives dead-code elimination
#pragma unroll
            for (int i = 0; i < ns; i++) { bad = bad || !__builtin_isfinite(s[i]); vs = s[i] > vs ? s[i] : vs; }
        }
        if constexpr (nl > 0) {
            double L[nla * nz], Lp[nla * npa], l[nla];
#pragma unroll
            for (int i = 0; i < nl * npa; i++) Lp[i] = 0.0;
            M::lin_rows(par, t, k, L, Lp, l);
#pragma unroll
            for (int i = 0; i < nl; i++) {
                double a = l[i];
#pragma unroll
                for (int j = 0; j < nz; j++) a += L[i * nz + j] * z[j];
#pragma unroll
                for (int j = 0; j < np; j++) a += Lp[i * npa + j] * pb[j];
                bad = bad || !__builtin_isfinite(a);
                vl = a > vl ? a : vl;
            }
        }
        if constexpr (nsoc > 0) {
            double Mm[nsoca * 4 * nz], m[nsoca * 4];
            M::soc_rows(par, t, k, Mm, m);
#pragma unroll
            for (int c = 0; c < nsoc; c++) {
                double w[4];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    double a = m[4 * c + r];
#pragma unroll
                    for (int j = 0; j < nz; j++) a += Mm[(4 * c + r) * nz + j] * z[j];
                    w[r] = a;
                }
                const double q = sqrt(w[1] * w[1] + w[2] * w[2] + w[3] * w[3]) - w[0];
                bad = bad || !__builtin_isfinite(q);
                vc = q > vc ? q : vc;
            }
        }
        if (vs > s_max) { s_max = vs; t_s = t; }      // strict: on ties the first sample wins
        if (vl > l_max) { l_max = vl; t_l = t; }
        if (vc > c_max) { c_max = vc; t_c = t; }
        if (vs > viol_tol || vl > viol_tol || vc > viol_tol) n_viol += 1.0;
        double gam = 0.0;
#pragma unroll
        for (int i = 0; i < nu; i++) gam += Qu[i] * u[i] * u[i] + lu[i] * u[i];
#pragma unroll
        for (int i = 0; i < nx; i++) gam += lx[i] * x[i];
        return gam;
    };

    gam_prev = sample(audit_linrange(0.0, 1.0, res, 0));
    for (int j = 1; j < res; j++) {
        const double t = audit_linrange(0.0, 1.0, res, j - 1), tp = audit_linrange(0.0, 1.0, res, j), h = tp - t;
        double k1[nx], k2[nx], k3[nx], k4[nx], tmp[nx];
        f(t, x, k1);
#pragma unroll
        for (int i = 0; i < nx; i++) tmp[i] = x[i] + h / 2 * k1[i];
        f(t + h / 2, tmp, k2);
#pragma unroll
        for (int i = 0; i < nx; i++) tmp[i] = x[i] + h / 2 * k2[i];
        f(t + h / 2, tmp, k3);
#pragma unroll
        for (int i = 0; i < nx; i++) tmp[i] = x[i] + h * k3[i];
        f(t + h, tmp, k4);
#pragma unroll
        for (int i = 0; i < nx; i++) x[i] = x[i] + h / 6 * (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]);
        M::action(x);
        const double gam = sample(tp);
        cost_int += 0.5 * h * (gam + gam_prev);          // trapz over tc (helper.jl:560-568), normalised time like the discrete J
        gam_prev = gam;
    }

    // ---- quantities of the end point and of the parameters alone ----
    double par_max = ninf;
    if constexpr (ng > 0) {
        double Lg[nga * npa], lg[nga];
        M::glin_rows(par, Lg, lg);
#pragma unroll
        for (int i = 0; i < ng; i++) {
            double a = lg[i];
#pragma unroll
            for (int j = 0; j < np; j++) a += Lg[i * np + j] * pb[j];
            par_max = a > par_max ? a : par_max;
        }
    }
    double bc = 0.0;
    if constexpr (ntc > 0) {
        double g[ntca], H[ntca * nx], K[ntca * npa];
        M::bc_tc(par, x, pb, pp, g, H, K);               // only g survives dead-code elimination
#pragma unroll
        for (int i = 0; i < ntc; i++) bc = fmax(bc, fabs(g[i]));
        // fmax drops a NaN operand: the flag below must see it
#pragma unroll
        for (int i = 0; i < ntc; i++) bad = bad || !__builtin_isfinite(g[i]);
    }
    double drift = 0.0;
#pragma unroll
    for (int i = 0; i < nx; i++) {
        const double d = (x[i] - xd[(long)(N - 1) * nx + i]) / Sx[i];
        bad = bad || !__builtin_isfinite(d);
        drift = fmax(drift, fabs(d));
    }
    double phi = 0.0;
#pragma unroll
    for (int i = 0; i < nx; i++) phi += tx[i] * x[i];
#pragma unroll
    for (int j = 0; j < np; j++) phi += ctp[j] * pb[j] + cQp[j] * pb[j] * pb[j];
    const double cost = phi + cost_int;
    bad = bad || !__builtin_isfinite(cost) || (ng > 0 && !__builtin_isfinite(par_max));

    out[0] = s_max; out[1] = t_s; out[2] = l_max; out[3] = t_l; out[4] = c_max; out[5] = t_c;
    out[6] = par_max; out[7] = bc; out[8] = drift; out[9] = cost; out[10] = n_viol; out[11] = bad ? 1.0 : 0.0;
#pragma unroll
    for (int i = 12; i < SCP_AUDIT_WIDTH; i++) out[i] = 0.0;
}

// one thread per problem, blocks of one wavefront, like propagate_foh_kernel: serial in time, independent across the batch
template <class M>
__global__ __launch_bounds__(64) void audit_foh_kernel(AuditArgs a, typename M::Params par)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    double* out = a.audit + (long)b * SCP_AUDIT_WIDTH;
    if (a.mask != nullptr && a.mask[b] == 0) {
#pragma unroll
        for (int i = 0; i < SCP_AUDIT_WIDTH; i++) out[i] = NAN;
        return;
    }
    audit_one<M>(par, a.N, a.res, a.viol_tol, a.xd + (long)b * a.N * M::nx, a.ud + (long)b * a.N * M::nu,
                 a.p + (long)b * np_total<M>(a.N), a.pp + (long)b * M::npp, a.Sx, out);
}

}  // namespace scp
