// The generator of the Monte-Carlo audit (scp_audit_montecarlo_*): Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random
// numbers: as easy as 1, 2, 3", SC'11; the Random123 known-answer vectors are in tests/test_audit_montecarlo_cpu.py) as a pure
// function of a counter, and standard normals from it by Box-Muller.  Plain integer C++, one body for the kernels and the host twins.
//
//   key      the low and the high 32 bits of the caller's uint64 seed
//   counter  (c0, c1, c2, c3) = (pair index q, node k, flight d - 1, kind)
//   kind     0  the initial-state draw (k = 0)
//            1  the input disturbance of the interval LEAVING node k = 1 .. N-1
//            2  the state noise on ARRIVAL at node k = 2 .. N
//   uniforms from the output words r0 .. r3: u1 = ((r0 >> 5) 2^26 + (r1 >> 6) + 0.5) 2^-53, u2 the same from r2, r3: 53 random bits
//            at the centre of their cell, so both lie strictly inside (0, 1) and the logarithm never sees 0
//   normals  rho = sqrt(-2 ln u1):  z_{2q} = rho cos(2 pi u2),  z_{2q+1} = rho sin(2 pi u2)
//   indexing component i of a vector is element i % 2 of pair q = i / 2
//
// A draw depends on (seed, kind, k, d, i) and on NOTHING else: not on the problem b, not on B, D or the launch geometry.  Every
// problem of a batch therefore sees the same disturbances.  These common random numbers are the right default for ranking the
// problems of a batch against each other (the sampling error is shared and cancels in the comparison), and they make a problem's
// result independent of the batch it is audited in.
#pragma once
#include <math.h>
#include <stdint.h>

#include "models/model_common.hpp"

namespace scp {

SCP_DEV void mc_philox4x32_10(const uint32_t (&ctr)[4], uint32_t key0, uint32_t key1, uint32_t (&out)[4])
{
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ key0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ key1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        key0 += 0x9E3779B9u; key1 += 0xBB67AE85u;       // the Weyl sequence of the key
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

SCP_DEV double mc_uniform(uint32_t hi, uint32_t lo)
{
    return ((double)(hi >> 5) * 67108864.0 + (double)(lo >> 6) + 0.5) * (1.0 / 9007199254740992.0);
}

// pair q of the draw (seed, kind, k, d): z[0] = z_{2q}, z[1] = z_{2q+1}; d is the 1-based flight
SCP_DEV void mc_normal_pair(uint64_t seed, int kind, int k, int d, int q, double (&z)[2], uint32_t (&words)[4])
{
    const uint32_t ctr[4] = {(uint32_t)q, (uint32_t)k, (uint32_t)(d - 1), (uint32_t)kind};
    mc_philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32), words);
    const double u1 = mc_uniform(words[0], words[1]), u2 = mc_uniform(words[2], words[3]);
    const double rho = sqrt(-2.0 * log(u1)), phi = 6.283185307179586476925286766559 * u2;
    z[0] = rho * cos(phi);
    z[1] = rho * sin(phi);
}

// the n normals of the draw (seed, kind, k, d), n a compile-time size: every index below is one, so z stays in registers
template <int n>
SCP_DEV void mc_normals(uint64_t seed, int kind, int k, int d, double (&z)[n])
{
#pragma unroll
    for (int q = 0; q < (n + 1) / 2; q++) {
        double pair[2];
        uint32_t words[4];
        mc_normal_pair(seed, kind, k, d, q, pair, words);
        z[2 * q] = pair[0];
        if (2 * q + 1 < n) z[2 * q + 1] = pair[1];
    }
}

}  // namespace scp
