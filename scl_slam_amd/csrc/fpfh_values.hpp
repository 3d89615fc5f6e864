// fpfh_values.hpp -- the FPFH histogram value of a bin count in closed form, on the host and the device (fpfh.hip, scl_fpfh_values).
//
// PCL adds hist_incr to a float bin once per vote (hist_f1(row, h) += hist_incr).  The float left after `count` such additions from
// 0 depends on the count only, but it is a chain of up to N dependent roundings.  Here it is computed one binade at a time, exactly:
// in units of v = ulp(hist_incr) every partial sum is an integer S; inside a binade [2^p, 2^(p+1)) of spacing U (U = 1 below 2^24
// units) every step adds the same multiple of U -- m U when the remainder r = I mod U is below U / 2, (m + 1) U above it, and on a
// tie (r = U / 2) m U or (m + 1) U so that S / U stays even, which is constant once S / U is even -- as long as the exact sum stays
// below the binade's top.  The first step of a binade (and a tie step from an odd S / U) is rounded one by one.
// tests/test_fpfh_checker.py compares every count 0 .. N with the plain loop at N up to 240 000.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SCL_FPFH_HD __host__ __device__
#else
#define SCL_FPFH_HD
#endif

namespace scl {

// X (an integer in units of v, X < 2^62) rounded to the float grid: 24 significant bits, ties to even
SCL_FPFH_HD inline uint64_t fpfh_round_units(uint64_t X)
{
    const int p = 63 - __builtin_clzll(X | 1ull);
    if (p <= 23) return X;
    const int sh = p - 23;
    const uint64_t U = 1ull << sh, rem = X & (U - 1), half = U >> 1;
    uint64_t q = X >> sh;
    if (rem > half || (rem == half && (q & 1ull))) ++q;
    return q << sh;
}

SCL_FPFH_HD inline float fpfh_value(uint32_t count, float inc)
{
    if (count == 0) return 0.0f;
    uint32_t bits;
    memcpy(&bits, &inc, sizeof bits);
    const int E = (int)((bits >> 23) & 0xffu);
    if (!(inc > 0.0f) || E == 0 || E == 255) {               // not a positive normal float: the plain loop
        float s = 0.0f;
        for (uint32_t i = 0; i < count; ++i) s += inc;
        return s;
    }
    const uint64_t I = (uint64_t)((bits & 0x7fffffu) | 0x800000u);
    uint64_t S = 0;
    uint32_t k = 0;
    while (k < count) {
        S = fpfh_round_units(S + I);                          // one step, rounded on its own
        if (++k == count) break;
        const int p = 63 - __builtin_clzll(S);
        const int sh = p > 23 ? p - 23 : 0;
        const uint64_t U = 1ull << sh, T = p > 23 ? (1ull << (p + 1)) : (1ull << 24);
        const uint64_t m = I >> sh, r = I & (U - 1);
        uint64_t st;
        if (2 * r < U) st = m * U;
        else if (2 * r > U) st = (m + 1) * U;
        else {                                                // tie: constant only from an even S / U on
            if ((S >> sh) & 1ull) continue;
            st = (m & 1ull) ? (m + 1) * U : m * U;
        }
        if (st == 0) break;                                   // hist_incr below half an ulp of the sum: it never moves again
        if (S + I >= T) continue;                             // the next step leaves the binade
        uint64_t n = (T - I - S + st - 1) / st;               // steps j with S + j st + I < T
        if (n > (uint64_t)(count - k)) n = count - k;
        S += n * st;
        k += (uint32_t)n;
    }
    // S has at most 24 significant bits: exact in float, then scaled by the power of two v
    return (float)__builtin_ldexp((double)S, E - 150);
}

}  // namespace scl
