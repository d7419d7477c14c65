// What the stand-alone sanitizer checks of the audit family share (tools/*_host_check.cpp, built and run by tools/Makefile): the
// table of the auditable models with the numbers each program feeds them, the trajectory and the synthetic discretisation they fly,
// the gains, the arrays of the calls that must be refused, and the count of failures with its last line.  Each program keeps its
// own calls, expectations and printed lines.  Host code only: not a pytest, not loaded into Python.
#pragma once
#include <cmath>
#include <cstdio>
#include <vector>

#include "../include/scp_mi355x.h"

static const double d2r = 3.14159265358979323846 / 180.0;

struct Model {
    const char* name;
    int id, nx, nu, np, npp;
    int nrow[3], ntc;      // (ns, nl, nsoc) and ntc of the model header: were they out of date, the sanitizer would see the covariance pre-pass overrun `rows`
    std::vector<double> par, par_true;      // the model blob; a truth blob for the dispersed flights (empty: none is flown)
    std::vector<double> x0, xf, u, p, pp, Sx, Su;
};

// the four auditable models (csrc/models/registry.hpp), indexed by model id.  The truth models: heavier gravity, a thirstier engine
// and less thrust for the rocket; heavier gravity for the quadrotor
inline const std::vector<Model>& models()
{
    static const std::vector<Model> m = {
        {"double_integrator", SCP_MODEL_DOUBLE_INTEGRATOR, 2, 1, 0, 4, {1, 2, 0}, 2, {0.1, 10.0}, {}, {0, 0}, {47, 0}, {1.5}, {}, {0, 0, 47, 0},
         {47, 9.4}, {4}},
        {"quadrotor", SCP_MODEL_QUADROTOR, 6, 4, 1, 12, {2, 3, 1}, 6,
         {9.81, 0.6, 23.2, 60 * d2r, 0.0, 2.5, 0.0, 2, 2, 0, 1, 2, 0, 1.5, 1.5, 0, 2, 5, 0},
         {10.3, 0.6, 23.2, 60 * d2r, 0.0, 2.5, 0.0, 2, 2, 0, 1, 2, 0, 1.5, 1.5, 0, 2, 5, 0},
         {0, 0, 0, 0, 0, 0}, {2.5, 6, 0, 0, 0, 0}, {0.1, -0.2, 9.81, 9.9}, {1.25}, {0, 0, 0, 0, 0, 0, 2.5, 6, 0, 0, 0, 0},
         {1, 1, 1, 1, 1, 1}, {46, 46, 46, 23}},
        {"rocket_landing", SCP_MODEL_ROCKET_LANDING, 7, 4, 1, 6, {2, 6, 2}, 6,
         {0, 0, -3.7114, 6.1e-5, 0, 3.5e-5, 5.1e-4, 1505, 1905, 4972, 13258, 86 * d2r, 40 * d2r, 138.9, 40, 120, 1},
         {0, 0, -4.0, 6.1e-5, 0, 3.5e-5, 5.6e-4, 1505, 1905, 4972, 12000, 86 * d2r, 40 * d2r, 138.9, 40, 120, 1},
         {2000, 0, 1500, 80, 30, -75, std::log(1905.0)}, {0, 0, 0, 0, 0, 0, std::log(1505.0)}, {0.1, 0.1, 3.7, 3.9}, {75},
         {2000, 0, 1500, 80, 30, -75}, {5000, 5000, 2500, 278, 278, 278, 0.24}, {14, 14, 7, 7}},
        {"starship", SCP_MODEL_STARSHIP, 8, 3, 10, 5, {23, 5, 0}, 6,
         {9, 100, 9.81, 120e3, 0.4, 0.45, 2.5e7, 0.2, 880e3, 2210e3, 2640e3, 6630e3, -3.1e-4, 10 * d2r, 20 * d2r, 0.05, 0, 40, 0.5,
          27 * d2r, 15 * d2r, 0, -0.1, 0.3, 10e3},
         {}, {100, 600, 0, -85, 90 * d2r, 0, 0, 0}, {0, 0, 0, -0.1, 0, 0, -3e3, 0}, {2.7e6, 0.02, 0.01},
         {1.0, 1.0, 50, 300, 0, -42, 0.8, 0, -1500, 0}, {100, 600, 0, -85, 90 * d2r}, {200, 600, 20, 85, 1.6, 0.35, 1e3, 0.35},
         {5750e3, 20 * d2r, 40 * d2r}},
    };
    return m;
}

// the straight line from x0 to xf on N nodes, under the model's input with a ripple of 5 %: xd[nx,N], ud[nu,N]
inline void straight_line(const Model& c, int N, std::vector<double>& xd, std::vector<double>& ud)
{
    xd.assign((size_t)c.nx * N, 0.0);
    ud.assign((size_t)c.nu * N, 0.0);
    for (int k = 0; k < N; k++) {
        const double t = (double)k / (N - 1);
        for (int i = 0; i < c.nx; i++) xd[(size_t)k * c.nx + i] = (1 - t) * c.x0[i] + t * c.xf[i];
        for (int i = 0; i < c.nu; i++) ud[(size_t)k * c.nu + i] = c.u[i] * (1.0 + 0.05 * std::sin(3.0 * k + i));
    }
}

// a discretisation that looks like one: A = I + h (a few couplings), B-, B+ = h / 2 (a few entries); [.,.,N-1] column-major.
// cross: every input also enters one more row of B-, weakly
inline void make_dyn(int nx, int nu, int N, std::vector<double>& A, std::vector<double>& Bm, std::vector<double>& Bp, bool cross = true)
{
    const double h = 1.0 / (N - 1);
    A.assign((size_t)nx * nx * (N - 1), 0.0);
    Bm.assign((size_t)nx * nu * (N - 1), 0.0);
    Bp.assign((size_t)nx * nu * (N - 1), 0.0);
    for (int k = 0; k < N - 1; k++) {
        double* a = A.data() + (size_t)k * nx * nx;
        for (int i = 0; i < nx; i++) a[i + nx * i] = 1.0;
        for (int i = 0; i + nx / 2 < nx; i++) a[i + nx * (i + nx / 2)] = h * (1.0 + 0.1 * k);      // position rows read the velocities
        for (int c = 0; c < nu; c++) {
            const int i = nx / 2 + c % (nx - nx / 2);
            Bm[(size_t)k * nx * nu + i + nx * c] = 0.5 * h * (1.0 + 0.05 * c);
            Bp[(size_t)k * nx * nu + i + nx * c] = 0.5 * h * (1.0 - 0.05 * c);
            if (cross) Bm[(size_t)k * nx * nu + c % nx + nx * c] += 0.1 * h * h;
        }
    }
}

// gains by Bryson's rule on a discretisation (scp_lqr_gains_host, csrc/lqr_api.hip): small, finite, K[nu,nx,N-1] of the documented size
inline bool gains(int nx, int nu, int N, const std::vector<double>& A, const std::vector<double>& Bm, const std::vector<double>& Bp,
                  const std::vector<double>& Sx, const std::vector<double>& Su, std::vector<double>& K)
{
    std::vector<double> qx(nx), ru(nu), qf(nx), info(SCP_LQR_INFO_WIDTH);
    for (int i = 0; i < nx; i++) { qx[i] = 1.0 / (Sx[i] * Sx[i]); qf[i] = 10.0 * qx[i]; }
    for (int i = 0; i < nu; i++) ru[i] = 1.0 / (Su[i] * Su[i]);
    K.assign((size_t)nu * nx * (N - 1), -5.0);
    return scp_lqr_gains_host(nx, nu, N, A.data(), Bm.data(), Bp.data(), qx.data(), ru.data(), qf.data(), K.data(), info.data()) == SCP_OK &&
           info[0] == 0.0;
}

// the arrays of the calls that must be refused before they read anything: one = 1.0 throughout, neg = one with a first entry of -1.0
static double one[64], neg[8];
static const bool dummies_filled = [] {
    for (double& v : one) v = 1.0;
    for (double& v : neg) v = 1.0;
    neg[0] = -1.0;
    return true;
}();

// the calls that did not return what they should; the last line and the exit status of a program
static int bad = 0;
inline int verdict()
{
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
