// Continuous-time audit of a solved batch: fly every solution open loop through the NONLINEAR dynamics (the propagation
// of SCPSolution(history), src/solvers/scp.jl:196-245: xc = propagate(last_sol, pbm; res)) and reduce, on the fly, what a
// user inspects afterwards -- the worst value of every constraint family BETWEEN the grid nodes, the open-loop terminal
// miss and the cost actually flown -- to one record of SCP_AUDIT_WIDTH doubles per problem (include/scp_mi355x.h).
//
// One body, audit_flight_one<M, MODE>, serves the flight kernels and their host twins (scp_model_audit_host and its kin).  The
// state after each RK4 step is consumed in registers: nothing of size res * B exists anywhere.  The integration repeats propagate_foh_kernel
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
#include "mc_rng.hpp"
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

// what the samples of one flight (audit_flight_one) or of one interval (audit_interval_one) accumulate
struct AuditAcc {
    double s_max = -INFINITY, t_s = 0.0, l_max = -INFINITY, t_l = 0.0, c_max = -INFINITY, t_c = 0.0, n_viol = 0.0;
    bool bad = false;
};

// Everything that is evaluated AT a sample: the three row families of z = [x; u] with the model functions called at (t, k),
// folded into `acc`; returns the running cost Gamma(x, u) there.  The one body of both audits.
template <class M>
SCP_DEV double audit_sample(const typename M::Params& par, double t, int k, const double (&x)[M::nx], const double (&u)[M::nu],
                            const double* pb, double viol_tol, const double (&Qu)[M::nu], const double (&lu)[M::nu],
                            const double (&lx)[M::nx], AuditAcc& acc)
{
    constexpr int nx = M::nx, nu = M::nu, nz = nx + nu, np = M::np, npa = np > 0 ? np : 1;
    constexpr int ns = M::ns, nsa = ns > 0 ? ns : 1, nl = M::nl, nla = nl > 0 ? nl : 1, nsoc = M::nsoc, nsoca = nsoc > 0 ? nsoc : 1;
    const double ninf = -INFINITY;
    bool bad = acc.bad;
    double z[nz];
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
    acc.bad = bad;
    if (vs > acc.s_max) { acc.s_max = vs; acc.t_s = t; }      // strict: on ties the first sample wins
    if (vl > acc.l_max) { acc.l_max = vl; acc.t_l = t; }
    if (vc > acc.c_max) { acc.c_max = vc; acc.t_c = t; }
    if (vs > viol_tol || vl > viol_tol || vc > viol_tol) acc.n_viol += 1.0;
    double gam = 0.0;
#pragma unroll
    for (int i = 0; i < nu; i++) gam += Qu[i] * u[i] * u[i] + lu[i] * u[i];
#pragma unroll
    for (int i = 0; i < nx; i++) gam += lx[i] * x[i];
    return gam;
}

// max_i (Lg p + lg)_i, the parameter-only rows (-Inf without rows)
template <class M>
SCP_DEV double audit_par_max(const typename M::Params& par, const double* pb)
{
    constexpr int np = M::np, npa = np > 0 ? np : 1, ng = M::ng, nga = ng > 0 ? ng : 1;
    double par_max = -INFINITY;
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
    return par_max;
}

// ||g_tc(x, p, pp)||_inf of a flown end state
template <class M>
SCP_DEV double audit_bc_tc(const typename M::Params& par, const double (&x)[M::nx], const double* pb, const double* pp, bool& bad)
{
    constexpr int nx = M::nx, np = M::np, npa = np > 0 ? np : 1, ntc = M::ntc, ntca = ntc > 0 ? ntc : 1;
    double bc = 0.0;
    if constexpr (ntc > 0) {
        double g[ntca], H[ntca * nx], K[ntca * npa];
        M::bc_tc(par, x, pb, pp, g, H, K);               // only g survives dead-code elimination
#pragma unroll
        for (int i = 0; i < ntc; i++) bc = fmax(bc, fabs(g[i]));
        // fmax drops a NaN operand: the flag must see it
#pragma unroll
        for (int i = 0; i < ntc; i++) bad = bad || !__builtin_isfinite(g[i]);
    }
    return bc;
}

// the terminal cost phi(x, p) of a flown end state
template <class M>
SCP_DEV double audit_phi(const double (&x)[M::nx], const double* pb, const double (&tx)[M::nx], const double (&ctp)[M::np > 0 ? M::np : 1],
                         const double (&cQp)[M::np > 0 ? M::np : 1])
{
    double phi = 0.0;
#pragma unroll
    for (int i = 0; i < M::nx; i++) phi += tx[i] * x[i];
#pragma unroll
    for (int j = 0; j < M::np; j++) phi += ctp[j] * pb[j] + cQp[j] * pb[j] * pb[j];
    return phi;
}

// ------------------------------------------------------------------------------------------------
// ONE flight of ONE problem, the body of the single-shooting, the dispersed, the tracking and the Monte-Carlo audit, on the device
// and in the host twins.The flight starts at the first node and takes res - 1 RK4 steps over LinRange(0, 1, res); the input is the
// first-order hold of ud with propagate_foh_kernel's clamp and interval search, stage times included.  The state is sampled
// before the first and after every step: the sample at time t is audited with the model functions of the last grid node <= t,
// decided against the exact grid values (the k_j rule), and the running cost is integrated by the trapezoidal rule over the
// samples.  The end point gives g_tc, the drift against xd[:,N] (the UNDISPERSED one in every mode) and phi.
//   nominal    x(0) = xd[:,1], u(t) = u_foh(t); out[12..15] = 0
//   dispersed  x(0) = xd[:,1] + dx0 (physical units), u'(t) = gain o u_foh(t) + bias at every time; the dynamics, the row
//              families, the cones and Gamma all see u': the flight is audited as flown.  `par` is the truth model's where the
//              call gives one (dynamics, s, rows, cost and g_tc); p and pp are not dispersed.  out[12..15] = 0
//   tracking   the dispersed flight with the loop closed by sample-and-hold gains Kg[nu,nx,N-1] at the node rate.  The caller
//              gives the RK4 steps per interval, the samples are res = steps (N-1) + 1, so that every step lies inside one interval
//              and node k is sample (k-1) steps by integer arithmetic.  Hold update at node k < N, before the step that leaves
//              it: du = -K_k (x - xd[:,k]); commanded input u_foh(t) + du, flown input gain o (u_foh(t) + du) + bias.  A sample
//              at a node is audited with the hold that was in force over the step that ended there.  out[12], [13] the largest
//              ||Su^-1 du||_inf over the hold updates and its node, [14], [15] the largest ||Sx^-1 (x(t_k) - xd[:,k])||_inf
//              over the nodes 1 .. N and its node (strict >: the first wins).  With K = 0 it is the dispersed flight.
//   montecarlo the tracking flight with gain = 1, bias = 0 under the disturbance model of the covariance audit (cov_kernel.hpp),
//              drawn inside the flight by mc_rng.hpp for flight mc.d: x(0) = xd[:,1] + sig0 o xi0; at node k < N, after the hold
//              update, w_k = sigu o xiu_k is drawn and the flown input is (u_foh(t) + du) + w_k over the whole interval, stage
//              times included (dynamics, U rows, cones and Gamma see it; the effort is measured on du alone); after the last RK4
//              step of interval k and BEFORE that sample is audited x += sigw o xiw_{k+1}, then M::action(x): the sample at node
//              k+1 and the node's tracking error see the kicked state.  Linearised, this is the Sigma recursion of
//              scp_audit_covariance_*: Gam = B- + B+ is the response to an input offset held over the interval.  At every node
//              mc.node(k, N, e, du / Su, finite) receives the node error -- on the device the cross-flight reduction
//              (mc_kernel.hpp) -- so every lane of a wavefront must reach it: the loops below have uniform trip counts.
// Only these places -- the initial state, one expression of `input`, the `node` calls with the draws, the kick and out[12..15] --
// stand behind `if constexpr`; what a mode does not use (ug, ubs, du, wk, effort .. k_track, node, mc) is dead there, and every
// kernel's machine code is what its own copy of this body gave ("One flight body").  Do NOT merge further: sharing the RK4 step with
// audit_interval_one, one argument struct for the dispersed and the tracking kernel, or one body with the interval audit
// each changes the register allocation of kernels that sit at their VGPR limit (measured, same place).
// ------------------------------------------------------------------------------------------------
enum class AuditFlight { nominal, dispersed, tracking, montecarlo };
struct AuditNoNoise {};      // the `mc` of the three deterministic modes

// xd[nx,N], ud[nu,N], p[np], pp[npp], Sx[nx] -> out[SCP_AUDIT_WIDTH]; dispersed and tracking: dx0[nx], gain[nu], bias[nu], each
// may be nullptr; tracking: Su[nu], Kg[nu,nx,N-1]; montecarlo: those two and mc = {seed, d, sig0[nx], sigu[nu], sigw[nx], node(...)}
template <class M, AuditFlight MODE, class Mc = AuditNoNoise>
SCP_DEV void audit_flight_one(const typename M::Params& par, int N, int res_or_steps, double viol_tol, const double* xd,
                              const double* ub, const double* pb, const double* pp, const double* Sx, double* out, const double* dx0 = nullptr,
                              const double* gain = nullptr, const double* bias = nullptr, const double* Su = nullptr,
                              const double* Kg = nullptr, Mc&& mc = Mc{})
{
    static_assert(M::np_node == 0, "a row of node k would read that node's own parameters: undefined between the nodes");
    constexpr int nx = M::nx, nu = M::nu, np = M::np, npa = np > 0 ? np : 1, npF = M::npF, npFa = npF > 0 ? npF : 1, ng = M::ng;
    constexpr bool noisy = MODE == AuditFlight::montecarlo, tracking = MODE == AuditFlight::tracking || noisy;
    const int steps = res_or_steps, res = tracking ? steps * (N - 1) + 1 : res_or_steps;

    double x[nx], ug[nu], ubs[nu], du[nu], wk[nu];
    if constexpr (noisy) {
        double xi[nx];
        mc_normals<nx>(mc.seed, 0, 0, mc.d, xi);
#pragma unroll
        for (int i = 0; i < nx; i++) x[i] = xd[i] + mc.sig0[i] * xi[i];
    } else {
#pragma unroll
        for (int i = 0; i < nx; i++) {
            if constexpr (MODE == AuditFlight::nominal) x[i] = xd[i];
            else x[i] = xd[i] + (dx0 != nullptr ? dx0[i] : 0.0);
        }
    }
#pragma unroll
    for (int i = 0; i < nu; i++) { ug[i] = gain != nullptr ? gain[i] : 1.0; ubs[i] = bias != nullptr ? bias[i] : 0.0; du[i] = 0.0; wk[i] = 0.0; }
    // u(t) and f(t, x): propagate_foh_kernel's own, then the mode's feedback, gain and bias
    auto input = [&](double t, double (&u)[nu]) {
        const double g0 = linrange(0.0, 1.0, N, 0), g1 = linrange(0.0, 1.0, N, N - 1);
        t = fmax(g0, fmin(g1, t));
        int k = (int)floor(t * (N - 1));
        k = k < 0 ? 0 : (k > N ? N : k);
        while (k < N && t > linrange(0.0, 1.0, N, k)) k++;
        while (k > 0 && !(t > linrange(0.0, 1.0, N, k - 1))) k--;
        if (k == 0) k = 1;
        const double ta = linrange(0.0, 1.0, N, k - 1), tb = linrange(0.0, 1.0, N, k);
        const double c = (tb - t) / (tb - ta);
#pragma unroll
        for (int i = 0; i < nu; i++) {
            if constexpr (MODE == AuditFlight::nominal) u[i] = c * ub[(long)(k - 1) * nu + i] + (1.0 - c) * ub[(long)k * nu + i];
            else if constexpr (MODE == AuditFlight::dispersed) u[i] = ug[i] * (c * ub[(long)(k - 1) * nu + i] + (1.0 - c) * ub[(long)k * nu + i]) + ubs[i];
            else if constexpr (noisy) u[i] = ((c * ub[(long)(k - 1) * nu + i] + (1.0 - c) * ub[(long)k * nu + i]) + du[i]) + wk[i];
            else u[i] = ug[i] * ((c * ub[(long)(k - 1) * nu + i] + (1.0 - c) * ub[(long)k * nu + i]) + du[i]) + ubs[i];
        }
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

    AuditAcc acc;
    double gam_prev = 0.0, cost_int = 0.0;
    double effort = -INFINITY, k_effort = 0.0, track = -INFINITY, k_track = 0.0;

    // everything that is evaluated AT a sample (t, x): returns the running cost Gamma there
    auto sample = [&](double t) -> double {
        // 1-based index of the last grid node <= t, decided against the exact grid values (N at t = 1)
        int k = (int)floor(t * (N - 1)) + 1;
        k = k < 1 ? 1 : (k > N ? N : k);
        while (k < N && !(linrange(0.0, 1.0, N, k) > t)) k++;
        while (k > 1 && linrange(0.0, 1.0, N, k - 1) > t) k--;
        double u[nu];
        input(t, u);
        return audit_sample<M>(par, t, k, x, u, pb, viol_tol, Qu, lu, lx, acc);
    };
    // tracking, at node k (1-based): the tracking error of the state as it is, and for k < N the new hold from it
    [[maybe_unused]] auto node = [&](int k) {
        const double* xk = xd + (long)(k - 1) * nx;
        double e[nx], terr = 0.0;
        [[maybe_unused]] double dus[nu];
        [[maybe_unused]] bool fin = true;      // montecarlo: e and du / Su of this node are all finite
#pragma unroll
        for (int i = 0; i < nx; i++) {
            e[i] = x[i] - xk[i];
            const double d = e[i] / Sx[i];
            acc.bad = acc.bad || !__builtin_isfinite(d);
            if constexpr (noisy) fin = fin && __builtin_isfinite(e[i]);
            terr = fmax(terr, fabs(d));
        }
        if constexpr (noisy) {
#pragma unroll
            for (int a = 0; a < nu; a++) dus[a] = 0.0;
        }
        if (terr > track) { track = terr; k_track = (double)k; }
        if (k < N) {
            const double* Kk = Kg + (long)(k - 1) * nu * nx;
            double eff = 0.0;
#pragma unroll
            for (int a = 0; a < nu; a++) {
                double s = 0.0;
#pragma unroll
                for (int i = 0; i < nx; i++) s += Kk[a + nu * i] * e[i];
                du[a] = -s;
                const double d = du[a] / Su[a];
                acc.bad = acc.bad || !__builtin_isfinite(d);
                if constexpr (noisy) { dus[a] = d; fin = fin && __builtin_isfinite(d); }
                eff = fmax(eff, fabs(d));
            }
            if (eff > effort) { effort = eff; k_effort = (double)k; }
        }
        if constexpr (noisy) {
            mc.node(k, N, e, dus, fin);
            if (k < N) {
                double xi[nu];
                mc_normals<nu>(mc.seed, 1, k, mc.d, xi);
#pragma unroll
                for (int a = 0; a < nu; a++) wk[a] = mc.sigu[a] * xi[a];
            }
        }
    };

    if constexpr (tracking) node(1);
    gam_prev = sample(linrange(0.0, 1.0, res, 0));
    for (int j = 1; j < res; j++) {
        if constexpr (tracking) {
            if (j > 1 && (j - 1) % steps == 0) node((j - 1) / steps + 1);
        }
        const double t = linrange(0.0, 1.0, res, j - 1), tp = linrange(0.0, 1.0, res, j), h = tp - t;
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
        if constexpr (noisy) {
            if (j % steps == 0) {                         // the step that arrives at node j / steps + 1
                double xi[nx];
                mc_normals<nx>(mc.seed, 2, j / steps + 1, mc.d, xi);
#pragma unroll
                for (int i = 0; i < nx; i++) x[i] += mc.sigw[i] * xi[i];
                M::action(x);
            }
        }
        const double gam = sample(tp);
        cost_int += 0.5 * h * (gam + gam_prev);          // trapz over tc (helper.jl:560-568), normalised time like the discrete J
        gam_prev = gam;
    }
    if constexpr (tracking) node(N);

    // ---- quantities of the end point and of the parameters alone ----
    const double par_max = audit_par_max<M>(par, pb);
    const double bc = audit_bc_tc<M>(par, x, pb, pp, acc.bad);
    double drift = 0.0;
#pragma unroll
    for (int i = 0; i < nx; i++) {
        const double d = (x[i] - xd[(long)(N - 1) * nx + i]) / Sx[i];
        acc.bad = acc.bad || !__builtin_isfinite(d);
        drift = fmax(drift, fabs(d));
    }
    const double phi = audit_phi<M>(x, pb, tx, ctp, cQp);
    const double cost = phi + cost_int;
    acc.bad = acc.bad || !__builtin_isfinite(cost) || (ng > 0 && !__builtin_isfinite(par_max));

    out[0] = acc.s_max; out[1] = acc.t_s; out[2] = acc.l_max; out[3] = acc.t_l; out[4] = acc.c_max; out[5] = acc.t_c;
    out[6] = par_max; out[7] = bc; out[8] = drift; out[9] = cost; out[10] = acc.n_viol; out[11] = acc.bad ? 1.0 : 0.0;
    if constexpr (tracking) {
        out[12] = effort; out[13] = k_effort; out[14] = track; out[15] = k_track;
    } else {
#pragma unroll
        for (int i = 12; i < SCP_AUDIT_WIDTH; i++) out[i] = 0.0;
    }
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
    audit_flight_one<M, AuditFlight::nominal>(par, a.N, a.res, a.viol_tol, a.xd + (long)b * a.N * M::nx, a.ud + (long)b * a.N * M::nu,
                                              a.p + (long)b * np_total<M>(a.N), a.pp + (long)b * M::npp, a.Sx, out);
}

// ------------------------------------------------------------------------------------------------
// Interval-parallel audit (multiple shooting; scp_audit_intervals_*): every interval k = 1 .. N-1 is flown from ITS OWN node
// over LinRange(t_k, t_{k+1}, sub), sub = max(2, ceil(res / (N - 1))), and reduced to one record of SCP_AUDIT_INTERVAL_WIDTH
// doubles; the records of a problem are then folded IN INTERVAL ORDER into the summary record, so that neither output
// depends on the batch size, on the place of a problem in the batch or on the launch geometry.
//   FOH      x0 = xd[:,k], u(t) = the first-order hold of ud[:,k], ud[:,k+1] alone (t clamped to the interval): no search
//   IMPULSE  x0 = xd[:,k] + M::impulse(t_k, k, xd[:,k], ud[:,k], p) as in propagate_impulse_kernel, the dynamics coast with
//            u = 0, and the row families and Gamma see z = [x; ud[:,k]], the impulse that opened the interval
// The model functions get the node index k at every sample but the last, which is node k+1 (decided by index).
// ------------------------------------------------------------------------------------------------
struct AuditIntervalArgs {
    int B, N, sub;
    double viol_tol;
    const double* xd;   // [nx,N,B]
    const double* ud;   // [nu,N,B]
    const double* p;    // [np,B]
    const double* pp;   // [npp,B]
    const double* Sx;   // [nx]
    const int* mask;    // optional [B]: problems with mask[b] == 0 are skipped, all their records are NaN
    double* intervals;  // [SCP_AUDIT_INTERVAL_WIDTH,N-1,B]
    double* audit;      // [SCP_AUDIT_WIDTH,B]
};

// audit_api.hip: audit_interval_kernel<M, IMP> then audit_interval_fold_kernel<M> on `stream`
int audit_intervals_launch(int model_id, const double* model_par, int disc_method, const AuditIntervalArgs& a, hipStream_t stream);

SCP_DEV int audit_interval_sub(int N, int res)
{
    const int sub = (res + (N - 1) - 1) / (N - 1);        // the reference's subres (discretization.jl:544) ...
    return sub < 2 ? 2 : sub;                             // ... but at least one step per interval
}

// interval k0 (0-based) of ONE problem: xd[nx,N], ud[nu,N], p[np], pp[npp], Sx[nx] -> rec[SCP_AUDIT_INTERVAL_WIDTH]
template <class M, bool IMP>
SCP_DEV void audit_interval_one(const typename M::Params& par, int N, int sub, int k0, double viol_tol, const double* xd,
                                const double* ud, const double* pb, const double* pp, const double* Sx, double* rec)
{
    static_assert(M::np_node == 0, "a row of node k would read that node's own parameters: undefined between the nodes");
    static_assert(!IMP || M::has_impulse, "the model has no impulsive-input form");
    constexpr int nx = M::nx, nu = M::nu, np = M::np, npa = np > 0 ? np : 1, npF = M::npF, npFa = npF > 0 ? npF : 1;
    const double t0 = linrange(0.0, 1.0, N, k0), t1 = linrange(0.0, 1.0, N, k0 + 1);

    double x[nx], ua[nu], ub[nu];
#pragma unroll
    for (int i = 0; i < nx; i++) x[i] = xd[(long)k0 * nx + i];
#pragma unroll
    for (int i = 0; i < nu; i++) { ua[i] = ud[(long)k0 * nu + i]; ub[i] = IMP ? 0.0 : ud[(long)(k0 + 1) * nu + i]; }
    if constexpr (IMP) {
        double dx[nx], Bi[nx * nu];
        M::impulse(par, t0, k0 + 1, x, ua, pb, dx, Bi);
#pragma unroll
        for (int i = 0; i < nx; i++) x[i] += dx[i];
    }
    // the input the dynamics see, and the input the rows and the running cost see
    auto input = [&](double t, double (&u)[nu]) {
        if constexpr (IMP) {
#pragma unroll
            for (int i = 0; i < nu; i++) u[i] = 0.0;
        } else {
            t = fmax(t0, fmin(t1, t));
            const double c = (t1 - t) / (t1 - t0);
#pragma unroll
            for (int i = 0; i < nu; i++) u[i] = c * ua[i] + (1.0 - c) * ub[i];
        }
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

    AuditAcc acc;
    auto sample = [&](double t, int k) -> double {
        double u[nu];
        if constexpr (IMP) {
#pragma unroll
            for (int i = 0; i < nu; i++) u[i] = ua[i];
        } else {
            input(t, u);
        }
        return audit_sample<M>(par, t, k, x, u, pb, viol_tol, Qu, lu, lx, acc);
    };

    double gam_prev = sample(linrange(t0, t1, sub, 0), k0 + 1), cost_int = 0.0;
    for (int j = 1; j < sub; j++) {
        const double t = linrange(t0, t1, sub, j - 1), tp = linrange(t0, t1, sub, j), h = tp - t;
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
        const double gam = sample(tp, j == sub - 1 ? k0 + 2 : k0 + 1);
        cost_int += 0.5 * h * (gam + gam_prev);
        gam_prev = gam;
    }

    double defect = 0.0;
#pragma unroll
    for (int i = 0; i < nx; i++) {
        const double d = (x[i] - xd[(long)(k0 + 1) * nx + i]) / Sx[i];
        acc.bad = acc.bad || !__builtin_isfinite(d);
        defect = fmax(defect, fabs(d));
    }
    double bc = 0.0, phi = 0.0;
    if (k0 == N - 2) {                                    // the end of the horizon: the last interval carries it
        bc = audit_bc_tc<M>(par, x, pb, pp, acc.bad);
        phi = audit_phi<M>(x, pb, tx, ctp, cQp);
    }
    acc.bad = acc.bad || !__builtin_isfinite(cost_int) || !__builtin_isfinite(phi);

    rec[0] = acc.s_max; rec[1] = acc.t_s; rec[2] = acc.l_max; rec[3] = acc.t_l; rec[4] = acc.c_max; rec[5] = acc.t_c;
    rec[6] = defect; rec[7] = cost_int; rec[8] = acc.n_viol; rec[9] = acc.bad ? 1.0 : 0.0; rec[10] = bc; rec[11] = phi;
#pragma unroll
    for (int i = 12; i < SCP_AUDIT_INTERVAL_WIDTH; i++) rec[i] = 0.0;
}

// The ordered fold of the N-1 interval records recs[SCP_AUDIT_INTERVAL_WIDTH, N-1] of ONE problem into out[SCP_AUDIT_WIDTH]
// (the layout of the single-shooting record).  Strict comparisons: the earliest interval wins a tie.  The cost is
// phi + (((I_1 + I_2) + ...) + I_{N-1}); the flag also covers a non-finite par_max where the model has such rows.
SCP_DEV void audit_interval_fold(int N, int sub, const double* recs, double par_max, bool has_par_rows, double* out)
{
    double vmax[3] = {-INFINITY, -INFINITY, -INFINITY}, tmax[3] = {0.0, 0.0, 0.0};
    double dmax = -INFINITY, kmax = 0.0, integral = 0.0, n_viol = 0.0;
    bool bad = has_par_rows && !__builtin_isfinite(par_max);
    for (int k = 0; k < N - 1; k++) {
        const double* r = recs + (long)k * SCP_AUDIT_INTERVAL_WIDTH;
#pragma unroll
        for (int f = 0; f < 3; f++)
            if (r[2 * f] > vmax[f]) { vmax[f] = r[2 * f]; tmax[f] = r[2 * f + 1]; }
        if (r[6] > dmax) { dmax = r[6]; kmax = (double)(k + 1); }
        integral += r[7];
        n_viol += r[8];
        bad = bad || r[9] != 0.0;
    }
    const double* last = recs + (long)(N - 2) * SCP_AUDIT_INTERVAL_WIDTH;
    const double cost = last[11] + integral;
    bad = bad || !__builtin_isfinite(cost);
    out[0] = vmax[0]; out[1] = tmax[0]; out[2] = vmax[1]; out[3] = tmax[1]; out[4] = vmax[2]; out[5] = tmax[2];
    out[6] = par_max; out[7] = last[10]; out[8] = dmax; out[9] = cost; out[10] = n_viol; out[11] = bad ? 1.0 : 0.0;
    out[12] = kmax; out[13] = 1.0; out[14] = (double)sub; out[15] = 0.0;
}

// one thread per (problem, interval), gid = b (N-1) + k0, blocks of one wavefront like propagate_impulse_kernel: neighbouring
// lanes fly neighbouring intervals of the same problem, all with the same trip count
template <class M, bool IMP>
__global__ __launch_bounds__(64) void audit_interval_kernel(AuditIntervalArgs a, typename M::Params par)
{
    const long gid = (long)blockIdx.x * 64 + threadIdx.x;
    if (gid >= (long)a.B * (a.N - 1)) return;
    const int b = (int)(gid / (a.N - 1)), k0 = (int)(gid % (a.N - 1));
    double* rec = a.intervals + gid * SCP_AUDIT_INTERVAL_WIDTH;
    if (a.mask != nullptr && a.mask[b] == 0) {
#pragma unroll
        for (int i = 0; i < SCP_AUDIT_INTERVAL_WIDTH; i++) rec[i] = NAN;
        return;
    }
    audit_interval_one<M, IMP>(par, a.N, a.sub, k0, a.viol_tol, a.xd + (long)b * a.N * M::nx, a.ud + (long)b * a.N * M::nu,
                               a.p + (long)b * np_total<M>(a.N), a.pp + (long)b * M::npp, a.Sx, rec);
}

// one thread per problem: its N-1 records in interval order -> the summary record
template <class M>
__global__ __launch_bounds__(64) void audit_interval_fold_kernel(AuditIntervalArgs a, typename M::Params par)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    double* out = a.audit + (long)b * SCP_AUDIT_WIDTH;
    if (a.mask != nullptr && a.mask[b] == 0) {
#pragma unroll
        for (int i = 0; i < SCP_AUDIT_WIDTH; i++) out[i] = NAN;
        return;
    }
    audit_interval_fold(a.N, a.sub, a.intervals + (long)b * (a.N - 1) * SCP_AUDIT_INTERVAL_WIDTH,
                        audit_par_max<M>(par, a.p + (long)b * np_total<M>(a.N)), M::ng > 0, out);
}

// ------------------------------------------------------------------------------------------------
// Dispersed-flight audit (scp_audit_dispersed_*): every problem is flown D times OFF-nominal, audit_flight_one's dispersed mode
// with column d = 1 .. D of dx0 / ugain / ubias.  One record per flight in the single-shooting layout; the records of a problem
// are then folded IN FLIGHT ORDER into its summary, so that neither output depends on the batch size, on the place of a problem
// in the batch or on the launch geometry.
// ------------------------------------------------------------------------------------------------
struct AuditDispersedArgs {
    int B, N, res, D;
    int shared;          // 1: dx0 / ugain / ubias carry no batch dimension ([., D]) and every problem flies the same D dispersions
    double viol_tol;
    const double* xd;    // [nx,N,B]
    const double* ud;    // [nu,N,B]
    const double* p;     // [np,B]
    const double* pp;    // [npp,B]
    const double* Sx;    // [nx]
    const double* dx0;   // [nx,D,B] or [nx,D]; nullptr = 0
    const double* ugain; // [nu,D,B] or [nu,D]; nullptr = 1
    const double* ubias; // [nu,D,B] or [nu,D]; nullptr = 0
    const int* mask;     // optional [B]: problems with mask[b] == 0 are skipped, their summary and flight records are NaN
    double* flights;     // [SCP_AUDIT_WIDTH,D,B]
    double* audit;       // [SCP_AUDIT_WIDTH,B]
};

// audit_api.hip: audit_dispersed_kernel<M> then audit_dispersed_fold_kernel (no model enters the fold: it lives there) on `stream`; model_par is the blob the flights fly with
int audit_dispersed_launch(int model_id, const double* model_par, const AuditDispersedArgs& a, hipStream_t stream);

// The ordered fold of the D flight records recs[SCP_AUDIT_WIDTH, D] of ONE problem into out[SCP_AUDIT_WIDTH].  A flight whose
// record [11] != 0 is counted in [11] and takes no part in any other field.  Strict comparisons from -Inf: the first flight wins
// a tie.  [6] is that of the first counted flight (-Inf when none is counted); the mean cost is (((c_1 + c_2) + ...) + c_m) / m.
// `marker` is what [13] holds: 2.0 for the dispersed audit, 3.0 for the tracking audit.
SCP_DEV void audit_dispersed_fold(int D, const double* recs, double* out, double marker = 2.0)
{
    double vmax[3] = {-INFINITY, -INFINITY, -INFINITY}, dmax[3] = {0.0, 0.0, 0.0};
    double par_max = -INFINITY, bc = -INFINITY, dbc = 0.0, drift = -INFINITY, sum = 0.0, cmax = -INFINITY, n_viol = 0.0, n_bad = 0.0;
    int m = 0;
    for (int d = 0; d < D; d++) {
        const double* r = recs + (long)d * SCP_AUDIT_WIDTH;
        if (r[11] != 0.0) { n_bad += 1.0; continue; }
#pragma unroll
        for (int f = 0; f < 3; f++)
            if (r[2 * f] > vmax[f]) { vmax[f] = r[2 * f]; dmax[f] = (double)(d + 1); }
        if (m == 0) par_max = r[6];
        if (r[7] > bc) { bc = r[7]; dbc = (double)(d + 1); }
        if (r[8] > drift) drift = r[8];
        sum += r[9];
        if (r[9] > cmax) cmax = r[9];
        if (r[10] > 0.0) n_viol += 1.0;
        m++;
    }
    out[0] = vmax[0]; out[1] = dmax[0]; out[2] = vmax[1]; out[3] = dmax[1]; out[4] = vmax[2]; out[5] = dmax[2];
    out[6] = par_max; out[7] = m > 0 ? bc : NAN; out[8] = m > 0 ? drift : NAN; out[9] = m > 0 ? sum / (double)m : NAN;
    out[10] = n_viol; out[11] = n_bad; out[12] = dbc; out[13] = marker; out[14] = (double)D; out[15] = m > 0 ? cmax : NAN;
}

// the record of a skipped problem (mask[b] == 0): W NaNs
template <int W>
SCP_DEV void nan_record(double* out)
{
#pragma unroll
    for (int i = 0; i < W; i++) out[i] = NAN;
}

// the disturbance model of the covariance and Monte-Carlo audits: sig0[nx], sigu[nu], sigw[nx] all present, finite and >= 0
inline bool audit_sigmas_ok(int nx, int nu, const double* sig0, const double* sigu, const double* sigw)
{
    if (!sig0 || !sigu || !sigw) return false;
    for (int i = 0; i < nx; i++)
        if (!__builtin_isfinite(sig0[i]) || sig0[i] < 0.0 || !__builtin_isfinite(sigw[i]) || sigw[i] < 0.0) return false;
    for (int i = 0; i < nu; i++)
        if (!__builtin_isfinite(sigu[i]) || sigu[i] < 0.0) return false;
    return true;
}

// one thread per (problem, flight), gid = b D + (d - 1), blocks of one wavefront: the mapping of audit_interval_kernel.
// Neighbouring lanes fly the same problem, so their ud loads hit the same addresses and the trip count is uniform.
template <class M>
__global__ __launch_bounds__(64) void audit_dispersed_kernel(AuditDispersedArgs a, typename M::Params par)
{
    const long gid = (long)blockIdx.x * 64 + threadIdx.x;
    if (gid >= (long)a.B * a.D) return;
    const int b = (int)(gid / a.D);
    double* rec = a.flights + gid * SCP_AUDIT_WIDTH;
    if (a.mask != nullptr && a.mask[b] == 0) {
#pragma unroll
        for (int i = 0; i < SCP_AUDIT_WIDTH; i++) rec[i] = NAN;
        return;
    }
    const long col = a.shared ? gid % a.D : gid;          // the flight's column of the dispersion arrays
    audit_flight_one<M, AuditFlight::dispersed>(par, a.N, a.res, a.viol_tol, a.xd + (long)b * a.N * M::nx, a.ud + (long)b * a.N * M::nu,
                                                a.p + (long)b * np_total<M>(a.N), a.pp + (long)b * M::npp, a.Sx, rec,
                                                a.dx0 != nullptr ? a.dx0 + col * M::nx : nullptr,
                                                a.ugain != nullptr ? a.ugain + col * M::nu : nullptr,
                                                a.ubias != nullptr ? a.ubias + col * M::nu : nullptr);
}

// ------------------------------------------------------------------------------------------------
// Closed-loop tracking audit (scp_audit_tracking_*): the dispersed audit with audit_flight_one's tracking mode, the gains
// K[nu,nx,N-1] of every problem from lqr_kernel.hpp or any others; the fold is the dispersed one, marked 3.0.
// ------------------------------------------------------------------------------------------------
struct AuditTrackingArgs {
    int B, N, steps, D;
    int shared;          // as AuditDispersedArgs
    double viol_tol;
    const double* xd;    // [nx,N,B]
    const double* ud;    // [nu,N,B]
    const double* p;     // [np,B]
    const double* pp;    // [npp,B]
    const double* Sx;    // [nx]
    const double* Su;    // [nu]
    const double* K;     // [nu,nx,N-1,B]
    const double* dx0;   // [nx,D,B] or [nx,D]; nullptr = 0
    const double* ugain; // [nu,D,B] or [nu,D]; nullptr = 1
    const double* ubias; // [nu,D,B] or [nu,D]; nullptr = 0
    const int* mask;     // optional [B]
    double* flights;     // [SCP_AUDIT_WIDTH,D,B]
    double* audit;       // [SCP_AUDIT_WIDTH,B]
};

// audit_api.hip: audit_tracking_kernel<M> then audit_tracking_fold_kernel on `stream`; model_par is the blob the flights fly with
int audit_tracking_launch(int model_id, const double* model_par, const AuditTrackingArgs& a, hipStream_t stream);

// one thread per (problem, flight), gid = b D + (d - 1): the mapping of audit_dispersed_kernel
template <class M>
__global__ __launch_bounds__(64) void audit_tracking_kernel(AuditTrackingArgs a, typename M::Params par)
{
    const long gid = (long)blockIdx.x * 64 + threadIdx.x;
    if (gid >= (long)a.B * a.D) return;
    const int b = (int)(gid / a.D);
    double* rec = a.flights + gid * SCP_AUDIT_WIDTH;
    if (a.mask != nullptr && a.mask[b] == 0) {
#pragma unroll
        for (int i = 0; i < SCP_AUDIT_WIDTH; i++) rec[i] = NAN;
        return;
    }
    const long col = a.shared ? gid % a.D : gid;          // the flight's column of the dispersion arrays
    audit_flight_one<M, AuditFlight::tracking>(par, a.N, a.steps, a.viol_tol, a.xd + (long)b * a.N * M::nx, a.ud + (long)b * a.N * M::nu,
                                               a.p + (long)b * np_total<M>(a.N), a.pp + (long)b * M::npp, a.Sx, rec,
                                               a.dx0 != nullptr ? a.dx0 + col * M::nx : nullptr,
                                               a.ugain != nullptr ? a.ugain + col * M::nu : nullptr,
                                               a.ubias != nullptr ? a.ubias + col * M::nu : nullptr, a.Su,
                                               a.K + (long)b * (a.N - 1) * M::nu * M::nx);
}

}  // namespace scp