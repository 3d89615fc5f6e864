// pgo_blocks.hpp -- the 6 x 6 pieces pgo.hip and pgo_condensed.hip share: Cholesky of a symmetric block given by its upper triangle
// (se3::tri), and the two triangular solves with its factor.  Device code.
#pragma once

#include <hip/hip_runtime.h>

#include "se3_device.hpp"

namespace scl {
namespace pgo_blocks {

using se3::tri;

constexpr int kFacW = 55;          // the first of the 36 planes of W = A_i^T A_j in a linearised factor's 91 planes (pgo.hip)

// S (upper triangle, 21) = L L^T, column by column (scl_loop_covariance's order); false where a pivot is not > 0
__device__ inline bool chol6(const double *S, double *L)
{
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double s = S[tri(c, c)];
#pragma unroll
        for (int k = 0; k < c; ++k) s -= L[tri(k, c)] * L[tri(k, c)];
        if (!(s > 0.0)) ok = false;
        const double p = sqrt(s);
        L[tri(c, c)] = p;
#pragma unroll
        for (int rr = c + 1; rr < 6; ++rr) {
            double v = S[tri(c, rr)];
#pragma unroll
            for (int k = 0; k < c; ++k) v -= L[tri(k, rr)] * L[tri(k, c)];
            L[tri(c, rr)] = v / p;
        }
    }
    return ok;
}

// the same operations; false where a pivot is not above 2^-43 of its diagonal entry (scl_loop_covariance's rule)
__device__ inline bool chol6_checked(const double *S, double *L)
{
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double s = S[tri(c, c)];
#pragma unroll
        for (int k = 0; k < c; ++k) s -= L[tri(k, c)] * L[tri(k, c)];
        if (!(s > S[tri(c, c)] * 0x1p-43)) ok = false;
        const double p = sqrt(s);
        L[tri(c, c)] = p;
#pragma unroll
        for (int rr = c + 1; rr < 6; ++rr) {
            double v = S[tri(c, rr)];
#pragma unroll
            for (int k = 0; k < c; ++k) v -= L[tri(k, rr)] * L[tri(k, c)];
            L[tri(c, rr)] = v / p;
        }
    }
    return ok;
}

// v <- L^-1 v
__device__ inline void forward6(const double *L, double *v)
{
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double s = v[a];
#pragma unroll
        for (int k = 0; k < a; ++k) s -= L[tri(k, a)] * v[k];
        v[a] = s / L[tri(a, a)];
    }
}

// v <- L^-T v
__device__ inline void backward6(const double *L, double *v)
{
#pragma unroll
    for (int a = 5; a >= 0; --a) {
        double s = v[a];
#pragma unroll
        for (int k = a + 1; k < 6; ++k) s -= L[tri(a, k)] * v[k];
        v[a] = s / L[tri(a, a)];
    }
}

}  // namespace pgo_blocks
}  // namespace scl
