// m2dp.hip -- the M2DP descriptor on the GPU (include/scl_m2dp.h; reference m2dp_descriptor, include/descriptor.h:1803-2040).
// Numerics contract: DESIGN.md section 4 "M2DP".  Per launch group of up to 16 scans (copied in once, resident until the
// signatures are in the database):
//
//   m2dp_moments_kernel    fp64 sums of x, y, z and their products; 32 fixed parts per scan, each a fixed-order block
//                          reduction (the same cloud gives the same bits in any batch); flags non-finite coordinates;
//   m2dp_frame_kernel      one wave per scan: the parts summed in order, mean and covariance, 3 x 3 cyclic Jacobi in fp64,
//                          axes by descending eigenvalue, axis 2 = axis0 x axis1, rounded to float (signs still open);
//   m2dp_project_kernel    the float projection E^T (p - mean) of every point on the unsigned axes (sequential 3-term dots):
//                          the fp64 sums of the cubed coordinates along axes 0 and 1 (the sign rule) and maxRho =
//                          max sqrtf(x*x + x*x + z*z) as an order-free integer max (the quirk of D.h:1836-1839);
//   m2dp_hist_kernel       the signs applied to the frame, every point projected again on the signed axes, then 64 planes x
//                          the points of a part: pcx / pcy / rho in fp64 in the reference's order, theta by
//                          atan2 with an exact decision near the edges, votes into a 64 x 128 integer histogram in LDS
//                          (lane l visits plane (j + l) & 63 at step j: the 64 lanes of a wave never hit the same word),
//                          merged into the scan's global counts by integer atomics (order-free, exact);
//   m2dp_signature_kernel  one workgroup per scan: G = C C^T of the counts (exact integers in fp64), G^(2^16) by repeated
//                          squaring, four power steps through C, u and v = C^T u / |C^T u|, written as floats straight into
//                          the database slot (A = C / n has the same singular vectors).
// The database, the keyframe registry, make_and_save_many and the 1-NN detection (nn_l2_kernel<192>): plugin_host.hpp.
#include "scl_m2dp.h"

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstring>
#include <algorithm>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "device_common.hpp"
#include "plugin_host.hpp"

using namespace scl;

namespace {

constexpr int kGroup = SCL_M2DP_MAX_GROUP;
constexpr int kParts = 32;                 // blocks per scan of the moment / projection / histogram passes
constexpr int kThreads = 256;
constexpr int kBins = SCL_M2DP_ROWS * SCL_M2DP_COLS;   // 8192
constexpr int kHistStride = 129;           // LDS row stride of the histogram: lane l's plane row shifts its bank by l
constexpr int kSquarings = 16;
constexpr int kPowerSteps = 4;
// Theta guard: the device's atan2 (ocml, fp64) is within a few ulp of the true angle (< 1e-15 rad on [-pi, pi]); an angle
// farther than kThetaGuard from every edge is on the same side of it as glibc's atan2 (< 1 ulp).  Inside the band the edge is
// settled exactly (theta_below_edge).
constexpr double kThetaGuard = 1.0e-10;

// For every edge t_i of thetaList (D.h:1866-1870): the midpoint m_i between t_i and the next double below it and
// (cos m_i, sin m_i) as double-double pairs.  A correctly rounded atan2(pcy, pcx) is < t_i exactly when the true angle is
// < m_i, i.e. when pcy * cos(m_i) - pcx * sin(m_i) < 0 (for angles near m_i).  Edge 8 (t = 0): below exactly when pcy < 0.
// Generated at 70 decimal digits by tests/m2dp_checker.py:theta_edge_constants (tests/test_m2dp_checker.py compares).
__constant__ double c_edge_cs[17][4] = {
    {-0x1.0000000000000p+0, 0x1.9be6b7272cbaep-108, 0x1.cb3b399d7ce7ap-54, 0x1.4a22090a2b399p-108},    // t_0  = -pi
    {-0x1.d906bcf328d47p-1, 0x1.c7bda591e0c68p-55, -0x1.87de2a6aea961p-2, 0x1.7d9048d417083p-58},
    {-0x1.6a09e667f3bcdp-1, -0x1.934d46945349bp-55, -0x1.6a09e667f3bccp-1, 0x1.0ef3c90a9fd48p-55},
    {-0x1.87de2a6aea963p-2, -0x1.9241792bde5dap-56, -0x1.d906bcf328d46p-1, -0x1.484edcbf3431bp-58},
    {-0x1.cb3b399d747f2p-55, -0x1.f1976b7ed8fbcp-110, -0x1.0000000000000p+0, 0x1.9be6b7271da59p-110},  // t_4  = -pi/2
    {0x1.87de2a6aea962p-2, -0x1.0ed78e6a0f0cdp-56, -0x1.d906bcf328d46p-1, -0x1.8884dad161a87p-55},
    {0x1.6a09e667f3bccp-1, 0x1.9fcfde4d02749p-55, -0x1.6a09e667f3bcdp-1, 0x1.1b7660c34eff4p-55},
    {0x1.d906bcf328d46p-1, 0x1.db3f4267a5c72p-57, -0x1.87de2a6aea963p-2, -0x1.abbb254107cccp-60},
    {0x1.0000000000000p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0},                                               // t_8  = 0
    {0x1.d906bcf328d46p-1, 0x1.3abee5cf5ebcep-55, 0x1.87de2a6aea962p-2, 0x1.a2b8e1b6fb501p-58},
    {0x1.6a09e667f3bcdp-1, 0x1.cf8eac73a7b86p-57, 0x1.6a09e667f3bccp-1, 0x1.075d26cc98726p-59},
    {0x1.87de2a6aea96dp-2, -0x1.6c6baf3c7649fp-57, 0x1.d906bcf328d44p-1, 0x1.653f713f8886cp-57},
    {0x1.8d313198a2e03p-53, 0x1.c1cd129024e08p-107, 0x1.0000000000000p+0, -0x1.3420cea3b79acp-106},   // t_12 = pi/2
    {-0x1.87de2a6aea967p-2, -0x1.69dd83149401cp-58, 0x1.d906bcf328d45p-1, 0x1.194d86c211599p-55},
    {-0x1.6a09e667f3bcbp-1, 0x1.bd01ecab4a9cep-55, 0x1.6a09e667f3bcfp-1, -0x1.bea495cb01ee8p-55},
    {-0x1.d906bcf328d43p-1, -0x1.f9510716ca855p-55, 0x1.87de2a6aea970p-2, -0x1.3e8c73cfeb380p-56},
    {-0x1.0000000000000p+0, 0x1.3420cea3b79acp-104, 0x1.8d313198a2e03p-52, 0x1.c1cd129024e06p-106},  // t_16 = pi
};

struct M2Scan {
    unsigned long long byte_off;    // first byte of the scan in the group's point buffer
    int n;
    int slot;                       // database row that receives the signature
};

// frame record (float): mean[3], axis0[3], axis1[3], axis2[3]
constexpr int kFrame = 12;

__device__ __forceinline__ void part_range(int n, int part, long long &lo, long long &hi)
{
    lo = (long long)n * part / kParts;
    hi = (long long)n * (part + 1) / kParts;
}

// fixed-order tree reduction of `k` doubles per thread over the block; result in red[j * kThreads] for thread 0
template <int K>
__device__ __forceinline__ void block_sum_fixed(double (&v)[K], double *red)
{
    const int t = threadIdx.x;
    for (int j = 0; j < K; ++j) red[j * kThreads + t] = v[j];
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1) {
        if (t < off)
            for (int j = 0; j < K; ++j) red[j * kThreads + t] += red[j * kThreads + t + off];
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void m2dp_moments_kernel(const unsigned char *pts, const M2Scan *scans, int stride,
                                                                double *part, int *bad)
{
    __shared__ double red[9 * kThreads];
    const M2Scan sc = scans[blockIdx.y];
    long long lo, hi;
    part_range(sc.n, blockIdx.x, lo, hi);
    double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool nonfinite = false;
    for (long long i = lo + threadIdx.x; i < hi; i += kThreads) {
        const float *f = reinterpret_cast<const float *>(pts + sc.byte_off + (unsigned long long)i * (unsigned long long)stride);
        const float x = f[0], y = f[1], z = f[2];
        nonfinite |= !(isfinite(x) && isfinite(y) && isfinite(z));
        const double dx = x, dy = y, dz = z;
        s[0] += dx; s[1] += dy; s[2] += dz;
        s[3] += dx * dx; s[4] += dx * dy; s[5] += dx * dz; s[6] += dy * dy; s[7] += dy * dz; s[8] += dz * dz;
    }
    if (nonfinite) atomicOr(&bad[blockIdx.y], 1);
    block_sum_fixed<9>(s, red);
    if (threadIdx.x == 0)
        for (int j = 0; j < 9; ++j) part[((size_t)blockIdx.y * kParts + blockIdx.x) * 9 + j] = red[j * kThreads];
}

__global__ __launch_bounds__(64) void m2dp_frame_kernel(const M2Scan *scans, const double *part, float *framef)
{
    if (threadIdx.x != 0) return;
    const int g = blockIdx.x;
    const double n = (double)scans[g].n;
    double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = 0; b < kParts; ++b)
        for (int j = 0; j < 9; ++j) S[j] += part[((size_t)g * kParts + b) * 9 + j];
    const double m[3] = {S[0] / n, S[1] / n, S[2] / n};
    double a[3][3];
    a[0][0] = S[3] / n - m[0] * m[0]; a[0][1] = S[4] / n - m[0] * m[1]; a[0][2] = S[5] / n - m[0] * m[2];
    a[1][1] = S[6] / n - m[1] * m[1]; a[1][2] = S[7] / n - m[1] * m[2]; a[2][2] = S[8] / n - m[2] * m[2];
    a[1][0] = a[0][1]; a[2][0] = a[0][2]; a[2][1] = a[1][2];
    double v[3][3];
    jacobi3(a, v);
    int ord[3] = {0, 1, 2};                                       // descending eigenvalue, ties by index
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (a[ord[j]][ord[j]] > a[ord[i]][ord[i]]) { const int t = ord[i]; ord[i] = ord[j]; ord[j] = t; }
    const double a0[3] = {v[0][ord[0]], v[1][ord[0]], v[2][ord[0]]};
    const double a1[3] = {v[0][ord[1]], v[1][ord[1]], v[2][ord[1]]};
    const double a2[3] = {a0[1] * a1[2] - a0[2] * a1[1], a0[2] * a1[0] - a0[0] * a1[2], a0[0] * a1[1] - a0[1] * a1[0]};
    float *f = framef + (size_t)g * kFrame;
    for (int k = 0; k < 3; ++k) { f[k] = (float)m[k]; f[3 + k] = (float)a0[k]; f[6 + k] = (float)a1[k]; f[9 + k] = (float)a2[k]; }
}

__global__ __launch_bounds__(kThreads) void m2dp_project_kernel(const unsigned char *pts, const M2Scan *scans, int stride,
                                                                const float *framef, double *cube, unsigned int *max_rho)
{
    __shared__ double red[2 * kThreads];
    const M2Scan sc = scans[blockIdx.y];
    const float *f = framef + (size_t)blockIdx.y * kFrame;
    const float mx = f[0], my = f[1], mz = f[2];
    const float e00 = f[3], e01 = f[4], e02 = f[5], e10 = f[6], e11 = f[7], e12 = f[8], e20 = f[9], e21 = f[10], e22 = f[11];
    long long lo, hi;
    part_range(sc.n, blockIdx.x, lo, hi);
    double c3[2] = {0.0, 0.0};
    float rmax = 0.0f;
    for (long long i = lo + threadIdx.x; i < hi; i += kThreads) {
        const float *p = reinterpret_cast<const float *>(pts + sc.byte_off + (unsigned long long)i * (unsigned long long)stride);
        const float d0 = p[0] - mx, d1 = p[1] - my, d2 = p[2] - mz;
        const float c0 = (e00 * d0 + e01 * d1) + e02 * d2;
        const float c1 = (e10 * d0 + e11 * d1) + e12 * d2;
        const float c2 = (e20 * d0 + e21 * d1) + e22 * d2;
        const double q0 = c0, q1 = c1;
        c3[0] += q0 * q0 * q0; c3[1] += q1 * q1 * q1;
        rmax = fmaxf(rmax, sqrtf((c0 * c0 + c0 * c0) + c2 * c2));   // D.h:1836-1839: x twice, y absent
    }
    // non-negative floats order like their bit patterns: the max is order-free
    for (int off = 32; off > 0; off >>= 1) rmax = fmaxf(rmax, __shfl_xor(rmax, off));
    if ((threadIdx.x & 63) == 0) atomicMax(&max_rho[blockIdx.y], __float_as_uint(rmax));
    block_sum_fixed<2>(c3, red);
    if (threadIdx.x == 0) {
        cube[((size_t)blockIdx.y * kParts + blockIdx.x) * 2 + 0] = red[0];
        cube[((size_t)blockIdx.y * kParts + blockIdx.x) * 2 + 1] = red[kThreads];
    }
}

// Is glibc's atan2(pcy, pcx) < t_e?  Exact for an angle near edge e: the sign of pcy * cos(m_e) - pcx * sin(m_e) in
// double-double (the products split exactly by fma; p1 - p2 is exact near the edge, where the two are within a factor 2).
__device__ __forceinline__ bool theta_below_edge(double pcx, double pcy, int e)
{
    if (e == 0) return false;                                     // atan2 >= -M_PI = t_0
    const double ch = c_edge_cs[e][0], cl = c_edge_cs[e][1], sh = c_edge_cs[e][2], sl = c_edge_cs[e][3];
    const double p1 = pcy * ch, e1 = fma(pcy, ch, -p1);
    const double p2 = pcx * sh, e2 = fma(pcx, sh, -p2);
    const double hi = p1 - p2;
    const double lo = ((e1 - e2) + pcy * cl) - pcx * sl;
    return hi + lo < 0.0 || (hi + lo == 0.0 && (hi < 0.0 || (hi == 0.0 && lo < 0.0)));
}

struct HistShared {
    unsigned int hist[SCL_M2DP_ROWS * kHistStride];
    double pl[6][SCL_M2DP_ROWS];                                  // px0, px1, px2, py0, py1, py2 per plane
    double tl[17];
    double rl[9];
    float fr[kFrame];                                             // the signed float frame
};

__global__ __launch_bounds__(kThreads) void m2dp_hist_kernel(const unsigned char *pts, const M2Scan *scans, int stride, const double *cube,
                                                             const unsigned int *max_rho, const double *planes, const double *theta_list,
                                                             const float *framef, float *frame_out, unsigned int *counts,
                                                             unsigned long long *exact_hits)
{
    __shared__ HistShared sh;
    const int g = blockIdx.y, t = threadIdx.x;
    const M2Scan sc = scans[g];
    for (int i = t; i < SCL_M2DP_ROWS * kHistStride; i += kThreads) sh.hist[i] = 0u;
    for (int i = t; i < 6 * SCL_M2DP_ROWS; i += kThreads) sh.pl[i / SCL_M2DP_ROWS][i % SCL_M2DP_ROWS] = planes[i];
    if (t < 17) sh.tl[t] = theta_list[t];
    if (t == 0) {
        double s0 = 0.0, s1 = 0.0;                                // the parts in order: the same signs in every block
        for (int b = 0; b < kParts; ++b) { s0 += cube[((size_t)g * kParts + b) * 2]; s1 += cube[((size_t)g * kParts + b) * 2 + 1]; }
        const float g0 = s0 >= 0.0 ? 1.0f : -1.0f, g1 = s1 >= 0.0 ? 1.0f : -1.0f;
        const float *f = framef + (size_t)g * kFrame;             // axis 2 = axis0 x axis1 follows both flips
        for (int k = 0; k < 3; ++k) { sh.fr[k] = f[k]; sh.fr[3 + k] = f[3 + k] * g0; sh.fr[6 + k] = f[6 + k] * g1; sh.fr[9 + k] = f[9 + k] * (g0 * g1); }
        const double mr = (double)__uint_as_float(max_rho[g]);
        for (int i = 0; i <= SCL_M2DP_NUM_R; ++i) {               // D.h:1872-1880
            const double r = (double)i * sqrt(mr) / SCL_M2DP_NUM_R;
            sh.rl[i] = r * r;
        }
        sh.rl[SCL_M2DP_NUM_R] = sh.rl[SCL_M2DP_NUM_R] + 0.001;
        if (blockIdx.x == 0)
            for (int k = 0; k < kFrame; ++k) frame_out[(size_t)g * kFrame + k] = sh.fr[k];
    }
    __syncthreads();
    const float mx = sh.fr[0], my = sh.fr[1], mz = sh.fr[2];
    const float e00 = sh.fr[3], e01 = sh.fr[4], e02 = sh.fr[5], e10 = sh.fr[6], e11 = sh.fr[7], e12 = sh.fr[8];
    const float e20 = sh.fr[9], e21 = sh.fr[10], e22 = sh.fr[11];
    const int lane = t & 63;
    long long lo, hi;
    part_range(sc.n, blockIdx.x, lo, hi);
    unsigned int exact = 0;
    for (long long i = lo + t; i < hi; i += kThreads) {
        // the projection with the SIGNED axes (negating an unsigned projection afterwards would turn its +0 into -0, and
        // atan2(+-0, x < 0) is +-pi: one is dropped, the other counts in bin 0)
        const float *q = reinterpret_cast<const float *>(pts + sc.byte_off + (unsigned long long)i * (unsigned long long)stride);
        const float d0 = q[0] - mx, d1 = q[1] - my, d2 = q[2] - mz;
        const double x = (double)((e00 * d0 + e01 * d1) + e02 * d2);
        const double y = (double)((e10 * d0 + e11 * d1) + e12 * d2);
        const double z = -(double)((e20 * d0 + e21 * d1) + e22 * d2);                          // cloudPca row, D.h:1831-1833
        for (int j = 0; j < SCL_M2DP_ROWS; ++j) {
            const int p = (j + lane) & 63;
            const double pcx = (x * sh.pl[0][p] + y * sh.pl[1][p]) + z * sh.pl[2][p];
            const double pcy = (x * sh.pl[3][p] + y * sh.pl[4][p]) + z * sh.pl[5][p];
            const double rho = sqrt(pcx * pcx + pcy * pcy);           // D.h:1942-1946
            int rb = 0;                                               // first j with rho < rhoList[j], minus 1
#pragma unroll
            for (int k = 1; k <= SCL_M2DP_NUM_R; ++k) rb += sh.rl[k] <= rho ? 1 : 0;
            const double th = atan2(pcy, pcx);
            int tb = (int)floor((th + 3.141592653589793) * (16.0 / 6.283185307179586));
            tb = tb < 0 ? 0 : (tb > 16 ? 16 : tb);
            if (tb >= 1 && th < sh.tl[tb]) --tb;
            if (tb < 16 && th >= sh.tl[tb + 1]) ++tb;
            // tb = first i with th < thetaList[i], minus 1 (16: th >= thetaList[16], dropped)
            const bool near_lo = fabs(th - sh.tl[tb]) <= kThetaGuard;
            const bool near_hi = tb < 16 && fabs(th - sh.tl[tb + 1]) <= kThetaGuard;
            if (near_lo | near_hi) {
                const int e = near_lo ? tb : tb + 1;
                tb = theta_below_edge(pcx, pcy, e) ? e - 1 : e;
                ++exact;
            }
            if (rb < SCL_M2DP_NUM_R && tb < SCL_M2DP_NUM_T)          // D.h:1974-1977
                atomicAdd(&sh.hist[p * kHistStride + rb * SCL_M2DP_NUM_T + tb], 1u);
        }
    }
    if (exact) atomicAdd(exact_hits, (unsigned long long)exact);
    __syncthreads();
    for (int i = t; i < kBins; i += kThreads) {
        const unsigned int v = sh.hist[(i >> 7) * kHistStride + (i & 127)];
        if (v) atomicAdd(&counts[(size_t)g * kBins + i], v);
    }
}

__device__ __forceinline__ double block_max_abs(double v, double *red)
{
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(kThreads) void m2dp_signature_kernel(const M2Scan *scans, const unsigned int *counts, float *db)
{
    __shared__ double G[SCL_M2DP_ROWS * SCL_M2DP_ROWS];            // first the counts (uint32 view), then G
    __shared__ double u[SCL_M2DP_ROWS], w[SCL_M2DP_COLS], red[4], nrm;
    const int g = blockIdx.x, t = threadIdx.x;
    const unsigned int *C = counts + (size_t)g * kBins;
    unsigned int *Cl = reinterpret_cast<unsigned int *>(G);
    for (int i = t; i < kBins; i += kThreads) Cl[i] = C[i];
    __syncthreads();
    const int r0 = t >> 6, col = t & 63;                           // entries (r0 + 4 r, col), r = 0..15
    double acc[16];
    for (int r = 0; r < 16; ++r) {
        const int row = r0 + 4 * r;
        double s = 0.0;
        for (int k = 0; k < SCL_M2DP_COLS; ++k) s += (double)Cl[row * SCL_M2DP_COLS + k] * (double)Cl[col * SCL_M2DP_COLS + k];
        acc[r] = s;
    }
    __syncthreads();
    for (int r = 0; r < 16; ++r) G[(r0 + 4 * r) * SCL_M2DP_ROWS + col] = acc[r];
    __syncthreads();
    // G^(2^kSquarings), rescaled by a power of two after every squaring (exact, keeps the entries in range)
    for (int it = 0; it < kSquarings; ++it) {
        double mx = 0.0;
        for (int r = 0; r < 16; ++r) {
            const int row = r0 + 4 * r;
            double s = 0.0;
            for (int k = 0; k < SCL_M2DP_ROWS; ++k) s += G[row * SCL_M2DP_ROWS + k] * G[k * SCL_M2DP_ROWS + col];
            acc[r] = s; mx = fmax(mx, fabs(s));
        }
        mx = block_max_abs(mx, red);                                // (also the barrier before G is overwritten)
        int ex = 0;
        if (mx > 0.0) (void)frexp(mx, &ex);
        for (int r = 0; r < 16; ++r) G[(r0 + 4 * r) * SCL_M2DP_ROWS + col] = ldexp(acc[r], -ex);
        __syncthreads();
    }
    if (t < SCL_M2DP_ROWS) {                                        // u = P 1
        double s = 0.0;
        for (int k = 0; k < SCL_M2DP_ROWS; ++k) s += G[t * SCL_M2DP_ROWS + k];
        u[t] = s;
    }
    __syncthreads();
    auto normalize_u = [&]() {
        if (t == 0) { double s = 0.0; for (int k = 0; k < SCL_M2DP_ROWS; ++k) s += u[k] * u[k]; nrm = sqrt(s); }
        __syncthreads();
        if (t < SCL_M2DP_ROWS) u[t] = nrm > 0.0 ? u[t] / nrm : 0.0;
        __syncthreads();
    };
    normalize_u();
    for (int it = 0; it <= kPowerSteps; ++it) {
        if (t < SCL_M2DP_COLS) {                                    // w = C^T u
            double s = 0.0;
            for (int i = 0; i < SCL_M2DP_ROWS; ++i) s += (double)C[(size_t)i * SCL_M2DP_COLS + t] * u[i];
            w[t] = s;
        }
        __syncthreads();
        if (it == kPowerSteps) break;
        if (t < SCL_M2DP_ROWS) {                                    // u = C w
            double s = 0.0;
            for (int k = 0; k < SCL_M2DP_COLS; ++k) s += (double)C[(size_t)t * SCL_M2DP_COLS + k] * w[k];
            u[t] = s;
        }
        __syncthreads();
        normalize_u();
    }
    if (t == 0) {
        double s = 0.0, su = 0.0;
        for (int k = 0; k < SCL_M2DP_COLS; ++k) s += w[k] * w[k];
        for (int k = 0; k < SCL_M2DP_ROWS; ++k) su += u[k];
        nrm = su < 0.0 ? -sqrt(s) : sqrt(s);                        // the Perron sign: sum(u) >= 0
        red[0] = su < 0.0 ? -1.0 : 1.0;
    }
    __syncthreads();
    float *o = db + (size_t)scans[g].slot * SCL_M2DP_DIM;
    if (t < SCL_M2DP_ROWS) o[t] = (float)(u[t] * red[0]);
    if (t < SCL_M2DP_COLS) o[SCL_M2DP_ROWS + t] = (float)(nrm != 0.0 ? w[t] / nrm : 0.0);
}

}  // namespace

struct __attribute__((visibility("hidden"))) scl_m2dp : scl::VectorPlugin<SCL_M2DP_DIM> {
    static constexpr int kGroup = ::kGroup;
    scl_m2dp_config cfg;
    // the launch group's workspace
    unsigned char *d_pts = nullptr; size_t pts_cap = 0;
    M2Scan *d_scans = nullptr;
    double *d_part = nullptr, *d_cube = nullptr, *d_planes = nullptr, *d_theta = nullptr;
    float *d_framef = nullptr, *d_frame_out = nullptr;
    unsigned int *d_max_rho = nullptr, *d_counts = nullptr;
    int *d_bad = nullptr;
    unsigned long long *d_exact = nullptr;
    unsigned long long decisions = 0;

    static int check_layout(scl_m2dp *h, const void *points, int n_points, int stride);
    static int run_group_locked(scl_m2dp *h, const void *const *clouds, const int *n_points, int stride, int G, int slot0, int *any_bad,
                                uint32_t *counts_out = nullptr, float *frame_out = nullptr, float *max_rho_out = nullptr);
};

int scl_m2dp::check_layout(scl_m2dp *h, const void *points, int n_points, int stride)
{
    if (stride < 12 || (stride & 3)) return fail(h, SCL_ERR_INVALID_ARG, "bad point layout (stride_bytes >= 12, multiple of 4)");
    if (n_points < 3) return fail(h, SCL_ERR_INVALID_ARG, "M2DP needs at least 3 points (PCA)");
    if (!points) return fail(h, SCL_ERR_INVALID_ARG, "null point pointer");
    return SCL_OK;
}

// One launch group (G <= 16 clouds): signatures into database rows slot0 .. slot0 + G - 1 (capacity ensured by the caller).
// *any_bad = 1 if a cloud has a non-finite coordinate.  counts_out / frame_out / max_rho_out: the test hook (G == 1).
int scl_m2dp::run_group_locked(scl_m2dp *h, const void *const *clouds, const int *n_points, int stride, int G, int slot0, int *any_bad,
                                uint32_t *counts_out, float *frame_out, float *max_rho_out)
{
    M2Scan scans[kGroup];
    unsigned long long bytes = 0;
    for (int g = 0; g < G; ++g) {
        scans[g].byte_off = bytes; scans[g].n = n_points[g]; scans[g].slot = slot0 + g;
        bytes += (unsigned long long)n_points[g] * (unsigned long long)stride;
    }
    if (bytes > h->pts_cap) {
        h->pts_cap = 0;
        const size_t c = bytes + bytes / 4 + 4096;
        int rc = dev_regrow(h, &h->d_pts, c);
        if (rc) return rc;
        h->pts_cap = c;
    }
    for (int g = 0; g < G; ++g)
        SCL_HIP(h, hipMemcpyAsync(h->d_pts + scans[g].byte_off, clouds[g], (size_t)n_points[g] * stride, hipMemcpyHostToDevice, h->stream));
    SCL_HIP(h, hipMemcpyAsync(h->d_scans, scans, sizeof(M2Scan) * G, hipMemcpyHostToDevice, h->stream));
    SCL_HIP(h, hipMemsetAsync(h->d_bad, 0, sizeof(int) * G, h->stream));
    SCL_HIP(h, hipMemsetAsync(h->d_max_rho, 0, sizeof(unsigned int) * G, h->stream));
    SCL_HIP(h, hipMemsetAsync(h->d_counts, 0, sizeof(unsigned int) * kBins * G, h->stream));
    SCL_HIP(h, hipEventRecord(h->ev0, h->stream));
    hipLaunchKernelGGL(m2dp_moments_kernel, dim3(kParts, G), dim3(kThreads), 0, h->stream, h->d_pts, h->d_scans, stride, h->d_part, h->d_bad);
    hipLaunchKernelGGL(m2dp_frame_kernel, dim3(G), dim3(64), 0, h->stream, h->d_scans, h->d_part, h->d_framef);
    hipLaunchKernelGGL(m2dp_project_kernel, dim3(kParts, G), dim3(kThreads), 0, h->stream, h->d_pts, h->d_scans, stride, h->d_framef,
                       h->d_cube, h->d_max_rho);
    hipLaunchKernelGGL(m2dp_hist_kernel, dim3(kParts, G), dim3(kThreads), 0, h->stream, h->d_pts, h->d_scans, stride, h->d_cube, h->d_max_rho,
                       h->d_planes, h->d_theta, h->d_framef, h->d_frame_out, h->d_counts, h->d_exact);
    hipLaunchKernelGGL(m2dp_signature_kernel, dim3(G), dim3(kThreads), 0, h->stream, h->d_scans, h->d_counts, h->db.d_db);
    SCL_HIP(h, hipGetLastError());
    SCL_HIP(h, hipEventRecord(h->ev1, h->stream));
    int bad[kGroup];
    SCL_HIP(h, hipMemcpyAsync(bad, h->d_bad, sizeof(int) * G, hipMemcpyDeviceToHost, h->stream));
    if (counts_out) SCL_HIP(h, hipMemcpyAsync(counts_out, h->d_counts, sizeof(unsigned int) * kBins, hipMemcpyDeviceToHost, h->stream));
    if (frame_out) SCL_HIP(h, hipMemcpyAsync(frame_out, h->d_frame_out, sizeof(float) * kFrame, hipMemcpyDeviceToHost, h->stream));
    unsigned int mr = 0;
    if (max_rho_out) SCL_HIP(h, hipMemcpyAsync(&mr, h->d_max_rho, sizeof(unsigned int), hipMemcpyDeviceToHost, h->stream));
    SCL_HIP(h, hipStreamSynchronize(h->stream));
    if (max_rho_out) std::memcpy(max_rho_out, &mr, sizeof(float));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) h->kernel_us += 1000.0 * (double)ms;
    *any_bad = 0;
    for (int g = 0; g < G; ++g) {
        if (bad[g]) *any_bad = 1;
        h->decisions += (unsigned long long)n_points[g] * SCL_M2DP_ROWS;
    }
    return SCL_OK;
}

extern "C" {

int scl_m2dp_default_config(scl_m2dp_config *c)
{
    if (!c) return SCL_ERR_INVALID_ARG;
    c->device = 0; c->dist_thres = 0.3; c->num_exclude_recent = 30; c->robot_num = 1; c->this_id = 0;
    return SCL_OK;
}

int scl_m2dp_create(const scl_m2dp_config *cfg, scl_m2dp **out)
{
    if (!cfg || !out) return SCL_ERR_INVALID_ARG;
    *out = nullptr;
    scl_m2dp *h = nullptr;
    int rc = open_plugin(cfg, &h);
    if (rc) return rc;
    auto bail = [&](int code) { scl_m2dp_destroy(h); return code; };
    if ((rc = dev_alloc(h, &h->d_scans, kGroup)) || (rc = dev_alloc(h, &h->d_part, (size_t)kGroup * kParts * 9)) ||
        (rc = dev_alloc(h, &h->d_cube, (size_t)kGroup * kParts * 2)) || (rc = dev_alloc(h, &h->d_planes, 6 * SCL_M2DP_ROWS)) ||
        (rc = dev_alloc(h, &h->d_theta, 17)) || (rc = dev_alloc(h, &h->d_framef, (size_t)kGroup * kFrame)) ||
        (rc = dev_alloc(h, &h->d_frame_out, (size_t)kGroup * kFrame)) || (rc = dev_alloc(h, &h->d_max_rho, kGroup)) ||
        (rc = dev_alloc(h, &h->d_counts, (size_t)kGroup * kBins)) || (rc = dev_alloc(h, &h->d_bad, kGroup)) ||
        (rc = dev_alloc(h, &h->d_exact, 1)))
        return bail(rc);
    // the planes with the host's libm, as the reference computes them (D.h:1808-1818, 1885-1906; Eigen's cross product)
    std::vector<double> pl(6 * SCL_M2DP_ROWS);
    for (int i = 0; i < SCL_M2DP_NUM_P; ++i) {
        const double azm = -M_PI_2 + i * M_PI / (SCL_M2DP_NUM_P - 1);
        for (int j = 0; j < SCL_M2DP_NUM_Q; ++j) {
            const double elv = j * M_PI_2 / (SCL_M2DP_NUM_Q - 1);
            const double n0 = 1.0 * std::cos(elv) * std::cos(azm), n1 = 1.0 * std::cos(elv) * std::sin(azm), n2 = 1.0 * std::sin(elv);
            const double hh = n0;                                  // [1, 0, 0] . vecN
            const double p0 = 1.0 - hh * n0, p1 = 0.0 - hh * n1, p2 = 0.0 - hh * n2;
            const int r = i * SCL_M2DP_NUM_Q + j;
            pl[0 * SCL_M2DP_ROWS + r] = p0; pl[1 * SCL_M2DP_ROWS + r] = p1; pl[2 * SCL_M2DP_ROWS + r] = p2;
            pl[3 * SCL_M2DP_ROWS + r] = n1 * p2 - n2 * p1; pl[4 * SCL_M2DP_ROWS + r] = n2 * p0 - n0 * p2; pl[5 * SCL_M2DP_ROWS + r] = n0 * p1 - n1 * p0;
        }
    }
    double tl[17];
    for (int i = 0; i <= SCL_M2DP_NUM_T; ++i) tl[i] = -M_PI + i * 2 * M_PI / SCL_M2DP_NUM_T;    // D.h:1866-1870
    if (hipMemcpy(h->d_planes, pl.data(), sizeof(double) * pl.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_theta, tl, sizeof(tl), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(h->d_exact, 0, sizeof(unsigned long long)) != hipSuccess)
        return bail(SCL_ERR_HIP);
    *out = h;
    return SCL_OK;
}

int scl_m2dp_destroy(scl_m2dp *h)
{
    if (!h) return SCL_OK;
    return close_plugin(h, {h->d_pts, h->d_scans, h->d_part, h->d_cube, h->d_planes, h->d_theta, h->d_framef, h->d_frame_out, h->d_max_rho,
                            h->d_counts, h->d_bad, h->d_exact});
}

int scl_m2dp_signature_matrix(scl_m2dp *h, const void *points, int n_points, int stride_bytes, uint32_t *counts,
                              float *mean, float *axes, float *max_rho)
{
    if (!h) return SCL_ERR_INVALID_ARG;
    Entered<scl_m2dp> in(h);
    int rc = scl_m2dp::check_layout(h, points, n_points, stride_bytes), bad = 0;
    if (rc) return rc;
    if ((rc = h->db.grow(h, h->reg.n + 1))) return rc;
    float fr[kFrame], mr = 0.0f;
    std::vector<uint32_t> c(kBins);
    if ((rc = scl_m2dp::run_group_locked(h, &points, &n_points, stride_bytes, 1, h->reg.n, &bad, c.data(), fr, &mr))) return rc;
    if (bad) return fail(h, SCL_ERR_INVALID_ARG, "non-finite coordinate");
    if (counts) std::memcpy(counts, c.data(), sizeof(uint32_t) * kBins);
    if (mean) std::memcpy(mean, fr, sizeof(float) * 3);
    if (axes) std::memcpy(axes, fr + 3, sizeof(float) * 9);
    if (max_rho) *max_rho = mr;
    return SCL_OK;
}

int scl_m2dp_stats(const scl_m2dp *h, unsigned long long *decisions, unsigned long long *exact, double *kernel_us)
{
    if (!h) return SCL_ERR_INVALID_ARG;
    Entered<scl_m2dp> in(h);
    unsigned long long e = 0;
    SCL_HIP(h, hipMemcpy(&e, h->d_exact, sizeof(e), hipMemcpyDeviceToHost));
    if (decisions) *decisions = h->decisions;
    if (exact) *exact = e;
    if (kernel_us) *kernel_us = h->kernel_us;
    return SCL_OK;
}

}  // extern "C"

SCL_VECTOR_PLUGIN_ENTRY_POINTS(scl_m2dp)
