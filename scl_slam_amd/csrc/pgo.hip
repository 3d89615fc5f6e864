// pgo.hip -- the pose-graph solve (contract: include/scl_engine.h "POSE-GRAPH SOLVE"): SE(3) between factors and priors, Levenberg-
// Marquardt on the host around a launch chain with no grid-wide barrier, the linear solve by block-Jacobi PCG on the device.  All fp64.
//
//   pgo_prep_kernel        once per call, one thread per pose and per factor: quaternions normalised, Z^-1 (a prior: Z), cov = L L^T
//   pgo_linearise_kernel   one thread per factor: E, r, D(E), A = L^-1 J; stores chi2, A_i^T y, A_j^T y, A_i^T A_i, A_j^T A_j, W = A_i^T A_j
//                          as 91 planes of n_factors + n_priors doubles
//   pgo_assemble_kernel    one gather per pose over its incident (factor, side) list: g, the diagonal block, the cost's partial sums
//   pgo_finish_kernel      one block: the cost, |g|_inf and |delta|_inf of an LM iteration -> the record the host reads
//   pgo_pcg_init_kernel    the damped blocks' Cholesky factors, x = 0, r = -g, z = M^-1 r, the partial sums of r . z
//   pgo_pcg_a_kernel       beta and the convergence test from the partial sums, p = z + beta p (a neighbour's p is formed from its z and
//                          its old p, so no launch lies between the new p and the operator), q = (H + lambda diag H) p, partials of p . q
//   pgo_pcg_b_kernel       alpha from the partial sums, x += alpha p, r -= alpha q, z = M^-1 r, the partial sums of r . z
//   pgo_retract_kernel     X <- X (+) delta into the trial poses, the partial maxima of |delta|
//   pgo_apply_kernel       y = (H + lambda diag H) x for scl_pgo_hessian_apply: the operator of pgo_pcg_a_kernel on a vector from the host
//
// A pose of kPgoLongRow incident factors or more is gathered by the wave of the thread that owns it (gather_rows).  No atomics on floats;
// the one flag, set at convergence, turns the PCG launches queued behind it into returns.
#include "pgo.hpp"
#include "pgo_blocks.hpp"
#include "pgo_graph.hpp"
#include "se3_device.hpp"

#include <cmath>
#include <cstring>
#include <vector>

namespace scl {

namespace {

using namespace se3;
using pgo_blocks::chol6;
using pgo_blocks::forward6;
using pgo_blocks::backward6;

constexpr int kPrepStride = 28;    // q, t of Z^-1 (a prior: of Z) (7); L, cov = L L^T, L[tri(c, r)] = L_rc for r >= c (21)
constexpr int kPrepL = 7;
// the planes of a linearised factor
constexpr int kFacChi2 = 0, kFacGi = 1, kFacGj = 7, kFacHii = 13, kFacHjj = 34, kFacW = 55, kFacPlanes = 91;
static_assert(kFacW == pgo_blocks::kFacW, "pgo_condensed.hip reads W from these planes");
constexpr int kBlock = 256;
constexpr int kCgBlock = 32;       // PCG iterations queued between two reads of the flag

// ---- reductions of a fixed shape ----------------------------------------------------------------------------------------------------------

__device__ inline double block_sum(double v, double *s)
{
    const int tid = (int)threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if (tid < o) s[tid] = s[tid] + s[tid + o];
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}

__device__ inline double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }       // a NaN, once taken, stays

__device__ inline double block_max(double v, double *s)
{
    const int tid = (int)threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if (tid < o) s[tid] = nan_max(s[tid], s[tid + o]);
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}

// the sum of a list of per-block partial sums, the same in every thread of every workgroup that takes it
__device__ inline double list_sum(const double *part, int nb, double *s)
{
    double v = 0.0;
    for (int k = (int)threadIdx.x; k < nb; k += kBlock) v = v + part[k];
    return block_sum(v, s);
}

__device__ inline double list_max(const double *part, int nb, double *s)
{
    double v = 0.0;
    for (int k = (int)threadIdx.x; k < nb; k += kBlock) v = nan_max(v, part[k]);
    return block_max(v, s);
}

// acc[0 .. NV) = the sum of f's contributions over the incident list of pose p, in list order.  Every lane of the wave must call it (p >= n:
// an empty row).  A row below kPgoLongRow entries is summed by its own thread, one entry after the other; a longer one by the whole wave:
// lane l takes the entries l, l + 64, ... in that order and a butterfly adds the 64 lanes.
template <int NV, class F>
__device__ inline void gather_rows(const int *row_ptr, const int *entries, int p, int n, F f, double *acc)
{
    int beg = 0, deg = 0;
    if (p < n) { beg = row_ptr[p]; deg = row_ptr[p + 1] - beg; }
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.0;
    if (deg < kPgoLongRow)
        for (int e = 0; e < deg; ++e) f(entries[beg + e], acc);
    const int lane = (int)(threadIdx.x & 63u);
    for (unsigned long long longs = __ballot(deg >= kPgoLongRow); longs; longs &= longs - 1ull) {
        const int owner = __builtin_ctzll(longs);
        const int b = __shfl(beg, owner, 64), d = __shfl(deg, owner, 64);
        double part[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) part[v] = 0.0;
        for (int e = lane; e < d; e += 64) f(entries[b + e], part);
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) part[v] = part[v] + __shfl_xor(part[v], o, 64);
        if (lane == owner) {
#pragma unroll
            for (int v = 0; v < NV; ++v) acc[v] = part[v];
        }
    }
}

// ---- 6 x 6 pieces ---------------------------------------------------------------------------------------------------------------------------

// chol6, forward6, backward6: pgo_blocks.hpp

// out = (D + lambda diag(D)) v for the symmetric D given by its upper triangle
__device__ inline void damped_times(const double *D, double lambda, const double *v, double *out)
{
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < 6; ++b) s += (a <= b ? D[tri(a, b)] : D[tri(b, a)]) * v[b];
        out[a] = s + lambda * D[tri(a, a)] * v[a];
    }
}

// ---- prep ---------------------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void pgo_prep_kernel(const double *poses, int n, const double *z, const double *cov, const int *fi, int M,
                                                           double *X, double *prep)
{
    int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t < n) {
        double o[7];
        normalise_pose(poses + 7 * (size_t)t, o);
        for (int k = 0; k < 7; ++k) X[kPoseStride * (size_t)t + k] = o[k];
        X[kPoseStride * (size_t)t + 7] = 0.0;
        return;
    }
    t -= n;
    if (t >= M) return;
    double Z[7], S[21], L[21];
    normalise_pose(z + 7 * (size_t)t, Z);
    double *o = prep + kPrepStride * (size_t)t;
    if (fi[t] >= 0) {
        double qi[4], ti[3];
        qconj(Z, qi);
        qrot(qi, Z + 4, ti);
        for (int k = 0; k < 4; ++k) o[k] = qi[k];
        for (int k = 0; k < 3; ++k) o[4 + k] = -ti[k];
    } else {
        for (int k = 0; k < 7; ++k) o[k] = Z[k];
    }
    const double *c = cov + 36 * (size_t)t;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) S[tri(a, b)] = c[6 * a + b];
    (void)chol6(S, L);                                     // the host refused every covariance this would fail on
    for (int k = 0; k < 21; ++k) o[kPrepL + k] = L[k];
}

// ---- linearise ------------------------------------------------------------------------------------------------------------------------------

// J <- L^-1 J, column by column
__device__ inline void whiten(const double *L, double *J)
{
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double col[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) col[a] = J[6 * a + c];
        forward6(L, col);
#pragma unroll
        for (int a = 0; a < 6; ++a) J[6 * a + c] = col[a];
    }
}

__global__ __launch_bounds__(kBlock) void pgo_linearise_kernel(const double *X, const double *prep, const int *fi, const int *fj, int M, double *fac)
{
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= M) return;
    const int i = fi[k], j = fj[k];
    const double *P = prep + kPrepStride * (size_t)k;
    const double *Xj = X + kPoseStride * (size_t)j;
    double qE[4], tE[3], Rh[9], Bh[9];
    if (i >= 0) {
        const double *Xi = X + kPoseStride * (size_t)i;
        double qh[4], th[3], qhi[4], thi[3];
        relative_pose(Xi, Xj, qh, th);                     // h = X_i^-1 X_j
        compose(P, P + 4, qh, th, qE, tE);                 // E = Z^-1 h
        relative_pose(Xj, Xi, qhi, thi);                   // h^-1
        adjoint_blocks(qhi, thi, Rh, Bh);
    } else {
        relative_pose(P, Xj, qE, tE);                      // E = Z^-1 X
    }
    double r[6], qp[4], nv;
    qlog(qE, r, qp, &nv);
    r[3] = tE[0]; r[4] = tE[1]; r[5] = tE[2];
    // Jr^-1(w) = I + 1/2 [w]x + c [w]x^2, [w]x^2 = w w^T - (w . w) I
    const double theta = nv == 0.0 ? 0.0 : 2.0 * atan2(nv, qp[3]);
    const double t2 = theta * theta;
    const double cc = theta < 0.05 ? 1.0 / 12.0 + t2 / 720.0 + t2 * t2 / 30240.0 + t2 * t2 * t2 / 1209600.0
                                   : 1.0 / t2 - qp[3] / (2.0 * theta * nv);
    const double ww = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    double Jri[9], RE[9];
    Jri[0] = 1.0 + cc * (r[0] * r[0] - ww); Jri[1] = -0.5 * r[2] + cc * (r[0] * r[1]); Jri[2] = 0.5 * r[1] + cc * (r[0] * r[2]);
    Jri[3] = 0.5 * r[2] + cc * (r[1] * r[0]); Jri[4] = 1.0 + cc * (r[1] * r[1] - ww); Jri[5] = -0.5 * r[0] + cc * (r[1] * r[2]);
    Jri[6] = -0.5 * r[1] + cc * (r[2] * r[0]); Jri[7] = 0.5 * r[0] + cc * (r[2] * r[1]); Jri[8] = 1.0 + cc * (r[2] * r[2] - ww);
    qmat(qE, RE);
    double L[21];
#pragma unroll
    for (int a = 0; a < 21; ++a) L[a] = P[kPrepL + a];
    double Aj[36];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            Aj[6 * a + b] = Jri[3 * a + b]; Aj[6 * a + 3 + b] = 0.0;
            Aj[6 * (3 + a) + b] = 0.0;      Aj[6 * (3 + a) + 3 + b] = RE[3 * a + b];
        }
    whiten(L, Aj);
    forward6(L, r);                                        // y = L^-1 r
    const size_t MM = (size_t)M;
    double *o = fac + k;
    o[kFacChi2 * MM] = r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3] + r[4] * r[4] + r[5] * r[5];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < 6; ++m) s += Aj[6 * m + a] * r[m];
        o[(kFacGj + a) * MM] = s;
#pragma unroll
        for (int b = a; b < 6; ++b) {
            double h = 0.0;
#pragma unroll
            for (int m = 0; m < 6; ++m) h += Aj[6 * m + a] * Aj[6 * m + b];
            o[(kFacHjj + tri(a, b)) * MM] = h;
        }
    }
    if (i < 0) return;                                     // a prior has no i side: the gathers never read those planes of it
    // J_i = -D(E) Ad(h^-1) = -[[Jr^-1 R', 0], [R_E B', R_E R']]
    double Ai[36], T1[9], T2[9], T3[9];
    mm(Jri, Rh, T1); mm(RE, Bh, T2); mm(RE, Rh, T3);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            Ai[6 * a + b] = -T1[3 * a + b];       Ai[6 * a + 3 + b] = 0.0;
            Ai[6 * (3 + a) + b] = -T2[3 * a + b]; Ai[6 * (3 + a) + 3 + b] = -T3[3 * a + b];
        }
    whiten(L, Ai);
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < 6; ++m) s += Ai[6 * m + a] * r[m];
        o[(kFacGi + a) * MM] = s;
#pragma unroll
        for (int b = a; b < 6; ++b) {
            double h = 0.0;
#pragma unroll
            for (int m = 0; m < 6; ++m) h += Ai[6 * m + a] * Ai[6 * m + b];
            o[(kFacHii + tri(a, b)) * MM] = h;
        }
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            double w = 0.0;
#pragma unroll
            for (int m = 0; m < 6; ++m) w += Ai[6 * m + a] * Aj[6 * m + b];
            o[(kFacW + 6 * a + b) * MM] = w;
        }
    }
}

// ---- assemble -------------------------------------------------------------------------------------------------------------------------------

struct AssembleEntry {
    const double *fac; size_t M;
    // acc: g (6), the diagonal block's upper triangle (21), the chi2 of the factors whose j side (a prior's only side) the pose is
    __device__ void operator()(int entry, double *acc) const
    {
        const int k = entry >> 1, side = entry & 1;
        const double *o = fac + k;
        const int g0 = side ? kFacGj : kFacGi, h0 = side ? kFacHjj : kFacHii;
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[a] = acc[a] + o[(g0 + a) * M];
#pragma unroll
        for (int a = 0; a < 21; ++a) acc[6 + a] = acc[6 + a] + o[(h0 + a) * M];
        if (side) acc[27] = acc[27] + o[kFacChi2 * M];
    }
};

__global__ __launch_bounds__(kBlock) void pgo_assemble_kernel(const double *fac, int M, const int *row_ptr, const int *entries, int n,
                                                               double *g, double *D, double *part_cost, double *part_gmax)
{
    __shared__ double s[kBlock];
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    double acc[28];
    gather_rows<28>(row_ptr, entries, p, n, AssembleEntry{fac, (size_t)M}, acc);
    double gm = 0.0;
    if (p < n) {
        for (int a = 0; a < 6; ++a) { g[6 * (size_t)p + a] = acc[a]; gm = nan_max(gm, fabs(acc[a])); }
        for (int a = 0; a < 21; ++a) D[21 * (size_t)p + a] = acc[6 + a];
    }
    const double c = block_sum(p < n ? acc[27] : 0.0, s);
    const double m = block_max(gm, s);
    if (threadIdx.x == 0) { part_cost[blockIdx.x] = c; part_gmax[blockIdx.x] = m; }
}

__global__ __launch_bounds__(kBlock) void pgo_finish_kernel(const double *part_cost, const double *part_gmax, const double *part_step, int nb,
                                                             PgoRecord *rec)
{
    __shared__ double s[kBlock];
    const double c = list_sum(part_cost, nb, s), m = list_max(part_gmax, nb, s);
    const double st = part_step ? list_max(part_step, nb, s) : 0.0;
    if (threadIdx.x == 0) { rec->cost = 0.5 * c; rec->gmax = m; rec->step = st; }
}

// ---- the operator ------------------------------------------------------------------------------------------------------------------------------

// the off-diagonal part of a row: entry (k, side 0) adds W_k v(f_j[k]), entry (k, side 1) adds W_k^T v(f_i[k]); a prior adds nothing
template <class Vec>
struct OperatorEntry {
    const double *fac; size_t M; const int *fi; const int *fj; Vec vec;
    __device__ void operator()(int entry, double *acc) const
    {
        const int k = entry >> 1, side = entry & 1;
        const int other = side ? fi[k] : fj[k];
        if (other < 0) return;
        double v[6];
        vec(other, v);
        const double *W = fac + kFacW * M + k;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            double s = 0.0;
#pragma unroll
            for (int b = 0; b < 6; ++b) s += (side ? W[(6 * b + a) * M] : W[(6 * a + b) * M]) * v[b];
            acc[a] = acc[a] + s;
        }
    }
};

struct PlainVec {
    const double *x;
    __device__ void operator()(int pose, double *v) const { for (int a = 0; a < 6; ++a) v[a] = x[6 * (size_t)pose + a]; }
};

// p = z + beta p_old of the PCG iteration (p = z at its first)
struct DirectionVec {
    const double *z; const double *p_old; double beta; bool first;
    __device__ void operator()(int pose, double *v) const
    {
        for (int a = 0; a < 6; ++a) {
            const double zz = z[6 * (size_t)pose + a];
            v[a] = first ? zz : zz + beta * p_old[6 * (size_t)pose + a];
        }
    }
};

__global__ __launch_bounds__(kBlock) void pgo_apply_kernel(const double *fac, int M, const int *fi, const int *fj, const int *row_ptr,
                                                            const int *entries, int n, const double *D, double lambda, const double *x, double *y)
{
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    double acc[6];
    const PlainVec vec{x};
    gather_rows<6>(row_ptr, entries, p, n, OperatorEntry<PlainVec>{fac, (size_t)M, fi, fj, vec}, acc);
    if (p >= n) return;
    double v[6], d[6];
    vec(p, v);
    damped_times(D + 21 * (size_t)p, lambda, v, d);
    for (int a = 0; a < 6; ++a) y[6 * (size_t)p + a] = d[a] + acc[a];
}

// ---- PCG ----------------------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void pgo_pcg_init_kernel(const double *g, const double *D, double lambda, int n, double *Lblk,
                                                               double *x, double *r, double *z, double *part_rz, PgoRecord *rec)
{
    __shared__ double s[kBlock];
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    double rz = 0.0;
    if (p < n) {
        double S[21], L[21], v[6];
        for (int a = 0; a < 21; ++a) S[a] = D[21 * (size_t)p + a];
#pragma unroll
        for (int a = 0; a < 6; ++a) S[tri(a, a)] = S[tri(a, a)] + lambda * S[tri(a, a)];
        (void)chol6(S, L);
        for (int a = 0; a < 21; ++a) Lblk[21 * (size_t)p + a] = L[a];
        for (int a = 0; a < 6; ++a) { v[a] = -g[6 * (size_t)p + a]; r[6 * (size_t)p + a] = v[a]; x[6 * (size_t)p + a] = 0.0; }
        double w[6];
        for (int a = 0; a < 6; ++a) w[a] = v[a];
        forward6(L, w); backward6(L, w);
        for (int a = 0; a < 6; ++a) { z[6 * (size_t)p + a] = w[a]; rz += v[a] * w[a]; }
    }
    const double t = block_sum(rz, s);
    if (threadIdx.x == 0) {
        part_rz[blockIdx.x] = t;
        if (blockIdx.x == 0) { rec->flag = 0; rec->cg = 0; rec->rz0 = 0.0; }
    }
}

// iteration t: part_rz_new holds the partial sums of the current r . z, part_rz_old those of the iteration before (t > 0)
__global__ __launch_bounds__(kBlock) void pgo_pcg_a_kernel(int t, const double *fac, int M, const int *fi, const int *fj, const int *row_ptr,
                                                            const int *entries, int n, int nb, const double *D, double lambda, double tol2,
                                                            const double *z, const double *p_old, double *p_new, double *q,
                                                            const double *part_rz_new, const double *part_rz_old, double *part_pq, PgoRecord *rec)
{
    __shared__ double s[kBlock];
    // The flag may be set by workgroup 0 of this very launch -- every workgroup comes to the same decision below, so either value read
    // here ends the same way --; one thread reads it, so that a workgroup does not split over it in front of a barrier.
    __shared__ int flag;
    if (threadIdx.x == 0) flag = __atomic_load_n(&rec->flag, __ATOMIC_RELAXED);
    __syncthreads();
    if (flag) return;
    const double rz_new = list_sum(part_rz_new, nb, s);
    const double rz0 = t == 0 ? rz_new : rec->rz0;
    if (rz_new <= tol2 * rz0) {                            // converged (rz0 == 0: nothing to solve)
        if (blockIdx.x == 0 && threadIdx.x == 0) __atomic_store_n(&rec->flag, 1, __ATOMIC_RELAXED);
        return;
    }
    double beta = 0.0;
    if (t > 0) beta = rz_new / list_sum(part_rz_old, nb, s);
    if (blockIdx.x == 0 && threadIdx.x == 0) { rec->cg = t + 1; if (t == 0) rec->rz0 = rz_new; }
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const DirectionVec vec{z, p_old, beta, t == 0};
    double acc[6];
    gather_rows<6>(row_ptr, entries, p, n, OperatorEntry<DirectionVec>{fac, (size_t)M, fi, fj, vec}, acc);
    double pq = 0.0;
    if (p < n) {
        double v[6], d[6];
        vec(p, v);
        damped_times(D + 21 * (size_t)p, lambda, v, d);
        for (int a = 0; a < 6; ++a) {
            const double qa = d[a] + acc[a];
            p_new[6 * (size_t)p + a] = v[a];
            q[6 * (size_t)p + a] = qa;
            pq += v[a] * qa;
        }
    }
    const double tot = block_sum(pq, s);
    if (threadIdx.x == 0) part_pq[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kBlock) void pgo_pcg_b_kernel(int n, int nb, const double *Lblk, const double *pv, const double *q, double *x, double *r,
                                                            double *z, const double *part_rz, const double *part_pq, double *part_rz_next,
                                                            const PgoRecord *rec)
{
    __shared__ double s[kBlock];
    if (rec->flag) return;                                 // written by the launch before this one, or earlier
    const double rz = list_sum(part_rz, nb, s);
    const double alpha = rz / list_sum(part_pq, nb, s);
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    double rzn = 0.0;
    if (p < n) {
        double L[21], v[6], w[6];
        for (int a = 0; a < 21; ++a) L[a] = Lblk[21 * (size_t)p + a];
        for (int a = 0; a < 6; ++a) {
            const size_t o = 6 * (size_t)p + a;
            x[o] = x[o] + alpha * pv[o];
            v[a] = r[o] - alpha * q[o];
            r[o] = v[a];
            w[a] = v[a];
        }
        forward6(L, w); backward6(L, w);
        for (int a = 0; a < 6; ++a) { z[6 * (size_t)p + a] = w[a]; rzn += v[a] * w[a]; }
    }
    const double tot = block_sum(rzn, s);
    if (threadIdx.x == 0) part_rz_next[blockIdx.x] = tot;
}

// ---- retract, output ----------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void pgo_retract_kernel(const double *X, const double *delta, int n, double *Xt, double *part_step)
{
    __shared__ double s[kBlock];
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    double step = 0.0;
    if (p < n) {
        const double *P = X + kPoseStride * (size_t)p;
        double d[6];
        for (int a = 0; a < 6; ++a) { d[a] = delta[6 * (size_t)p + a]; step = nan_max(step, fabs(d[a])); }
        const double th = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        const double k = th < 1e-4 ? 0.5 - th * th / 48.0 : sin(0.5 * th) / th;
        const double dq[4] = {k * d[0], k * d[1], k * d[2], cos(0.5 * th)};
        double qn[4], rv[3];
        qmul(P, dq, qn);
        const double nn = sqrt(qn[0] * qn[0] + qn[1] * qn[1] + qn[2] * qn[2] + qn[3] * qn[3]);
        qrot(P, d + 3, rv);
        double *O = Xt + kPoseStride * (size_t)p;
        for (int a = 0; a < 4; ++a) O[a] = qn[a] / nn;
        for (int a = 0; a < 3; ++a) O[4 + a] = P[4 + a] + rv[a];
        O[7] = 0.0;
    }
    const double m = block_max(step, s);
    if (threadIdx.x == 0) part_step[blockIdx.x] = m;
}

__global__ __launch_bounds__(kBlock) void pgo_output_kernel(const double *X, int n, double *out)
{
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= n) return;
    const double *P = X + kPoseStride * (size_t)p;
    const double sg = P[3] < 0.0 ? -1.0 : 1.0;
    double *o = out + 7 * (size_t)p;
    o[0] = P[4]; o[1] = P[5]; o[2] = P[6];
    o[3] = sg * P[0]; o[4] = sg * P[1]; o[5] = sg * P[2]; o[6] = sg * P[3];
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------

#define PGO_HIP(call)                                                                                  \
    do {                                                                                               \
        const hipError_t e__ = (call);                                                                 \
        if (e__ != hipSuccess) {                                                                       \
            if (err) *err = std::string("pgo: ") + #call + ": " + hipGetErrorString(e__);              \
            return e__ == hipErrorOutOfMemory ? SCL_ERR_NOMEM : SCL_ERR_HIP;                           \
        }                                                                                              \
    } while (0)

using WS = PgoWorkspace;

int ensure(WS *ws, int k, size_t bytes, std::string *err)
{
    if (bytes <= ws->cap[k]) return SCL_OK;
    if (ws->buf[k]) { (void)hipFree(ws->buf[k]); ws->buf[k] = nullptr; ws->cap[k] = 0; }
    PGO_HIP(hipMalloc(&ws->buf[k], bytes));
    ws->cap[k] = bytes;
    return SCL_OK;
}

template <class T> T *at(WS *ws, int k) { return static_cast<T *>(ws->buf[k]); }

bool finite_all(const double *p, size_t n)
{
    for (size_t k = 0; k < n; ++k) if (!std::isfinite(p[k])) return false;
    return true;
}

bool quaternions_ok(const double *poses, int n)
{
    for (int k = 0; k < n; ++k) {
        const double *q = poses + 7 * (size_t)k + 3;
        const double s = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
        if (!(s >= 0.25 && s <= 4.0)) return false;
    }
    return true;
}

// 0, 1 (a non-finite entry of the upper triangle) or 2 (a pivot not above 2^-43 of its diagonal entry: scl_loop_covariance's rule)
int covariances_bad(const double *cov, int n)
{
    for (int i = 0; i < n; ++i) {
        const double *S = cov + 36 * (size_t)i;
        for (int a = 0; a < 6; ++a)
            for (int b = a; b < 6; ++b) if (!std::isfinite(S[6 * a + b])) return 1;
        double L[6][6] = {{0.0}};
        for (int c = 0; c < 6; ++c) {
            double s = S[6 * c + c];
            for (int k = 0; k < c; ++k) s -= L[c][k] * L[c][k];
            if (!(s > std::ldexp(S[6 * c + c], -43))) return 2;
            L[c][c] = std::sqrt(s);
            for (int r = c + 1; r < 6; ++r) {
                double v = S[6 * c + r];
                for (int k = 0; k < c; ++k) v -= L[r][k] * L[c][k];
                L[r][c] = v / L[c][c];
            }
        }
    }
    return 0;
}

using Graph = PgoGraph;

// inputs to the device, the incidence lists, the prep launch: X0 holds the normalised poses afterwards
int setup(WS *ws, hipStream_t stream, const PgoInputs &in, bool timing, Graph *gr, std::string *err)
{
    const int n = in.n_poses, F = in.n_factors, Pn = in.n_priors, M = F + Pn, nb = (n + kBlock - 1) / kBlock;
    *gr = Graph{n, M, nb, timing, 0.f, 0.f};
    if (timing) ws->linearize_ms = ws->solve_ms = 0.0;      // an untimed call leaves the last timed call's figures
    const size_t nn = (size_t)n, MM = (size_t)M;
    std::vector<int> fi(MM), fj(MM), row_ptr, entries;
    for (int k = 0; k < F; ++k) { fi[(size_t)k] = in.f_i[k]; fj[(size_t)k] = in.f_j[k]; }
    for (int m = 0; m < Pn; ++m) { fi[(size_t)(F + m)] = -1; fj[(size_t)(F + m)] = in.p_idx[m]; }
    pgo_incidence(n, in.f_i, in.f_j, F, in.p_idx, Pn, &row_ptr, &entries);
    int rc;
    const size_t vec = sizeof(double) * 6 * nn, part = sizeof(double) * (size_t)nb;
    const struct { int k; size_t bytes; } need[] = {
        {WS::B_POSES_IN, sizeof(double) * 7 * nn}, {WS::B_Z_IN, sizeof(double) * 7 * MM}, {WS::B_COV_IN, sizeof(double) * 36 * MM},
        {WS::B_FI, sizeof(int) * MM}, {WS::B_FJ, sizeof(int) * MM}, {WS::B_ROWPTR, sizeof(int) * (nn + 1)}, {WS::B_ENTRIES, sizeof(int) * entries.size()},
        {WS::B_X0, sizeof(double) * kPoseStride * nn}, {WS::B_X1, sizeof(double) * kPoseStride * nn}, {WS::B_FPREP, sizeof(double) * kPrepStride * MM},
        {WS::B_FAC0, sizeof(double) * kFacPlanes * MM}, {WS::B_FAC1, sizeof(double) * kFacPlanes * MM}, {WS::B_G0, vec}, {WS::B_G1, vec},
        {WS::B_D0, sizeof(double) * 21 * nn}, {WS::B_D1, sizeof(double) * 21 * nn}, {WS::B_LBLK, sizeof(double) * 21 * nn},
        {WS::B_VX, vec}, {WS::B_VR, vec}, {WS::B_VZ, vec}, {WS::B_VQ, vec}, {WS::B_VP0, vec}, {WS::B_VP1, vec},
        {WS::B_PART_COST, part}, {WS::B_PART_GMAX, part}, {WS::B_PART_RZ0, part}, {WS::B_PART_RZ1, part}, {WS::B_PART_PQ, part}, {WS::B_PART_STEP, part},
        {WS::B_REC, sizeof(PgoRecord)}, {WS::B_XIN, vec}, {WS::B_POSES_OUT, sizeof(double) * 7 * nn}};
    for (const auto &b : need)
        if ((rc = ensure(ws, b.k, b.bytes, err))) return rc;
    if (timing)
        for (hipEvent_t &ev : ws->ev)
            if (!ev) PGO_HIP(hipEventCreate(&ev));
    PGO_HIP(hipMemcpyAsync(ws->buf[WS::B_POSES_IN], in.poses, sizeof(double) * 7 * nn, hipMemcpyHostToDevice, stream));
    if (F > 0) {
        PGO_HIP(hipMemcpyAsync(ws->buf[WS::B_Z_IN], in.f_z, sizeof(double) * 7 * (size_t)F, hipMemcpyHostToDevice, stream));
        PGO_HIP(hipMemcpyAsync(ws->buf[WS::B_COV_IN], in.f_cov, sizeof(double) * 36 * (size_t)F, hipMemcpyHostToDevice, stream));
    }
    PGO_HIP(hipMemcpyAsync(at<double>(ws, WS::B_Z_IN) + 7 * (size_t)F, in.p_z, sizeof(double) * 7 * (size_t)Pn, hipMemcpyHostToDevice, stream));
    PGO_HIP(hipMemcpyAsync(at<double>(ws, WS::B_COV_IN) + 36 * (size_t)F, in.p_cov, sizeof(double) * 36 * (size_t)Pn, hipMemcpyHostToDevice, stream));
    PGO_HIP(hipMemcpyAsync(ws->buf[WS::B_FI], fi.data(), sizeof(int) * MM, hipMemcpyHostToDevice, stream));
    PGO_HIP(hipMemcpyAsync(ws->buf[WS::B_FJ], fj.data(), sizeof(int) * MM, hipMemcpyHostToDevice, stream));
    PGO_HIP(hipMemcpyAsync(ws->buf[WS::B_ROWPTR], row_ptr.data(), sizeof(int) * (nn + 1), hipMemcpyHostToDevice, stream));
    PGO_HIP(hipMemcpyAsync(ws->buf[WS::B_ENTRIES], entries.data(), sizeof(int) * entries.size(), hipMemcpyHostToDevice, stream));
    PGO_HIP(hipStreamSynchronize(stream));                 // the vectors above and the caller's arrays are pageable: nothing of them is read after this
    pgo_prep_kernel<<<dim3((unsigned)((nn + MM + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream>>>(
        at<double>(ws, WS::B_POSES_IN), n, at<double>(ws, WS::B_Z_IN), at<double>(ws, WS::B_COV_IN), at<int>(ws, WS::B_FI), M,
        at<double>(ws, WS::B_X0), at<double>(ws, WS::B_FPREP));
    PGO_HIP(hipGetLastError());
    return SCL_OK;
}

// the poses of side `b` linearised and assembled, the record written (part_step: with the step's norm of the retraction before it)
int enqueue_linearise(WS *ws, hipStream_t stream, const Graph &gr, int b, bool with_step, std::string *err)
{
    if (gr.timing) PGO_HIP(hipEventRecord(ws->ev[0], stream));
    pgo_linearise_kernel<<<dim3((unsigned)((gr.M + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream>>>(
        at<double>(ws, b ? WS::B_X1 : WS::B_X0), at<double>(ws, WS::B_FPREP), at<int>(ws, WS::B_FI), at<int>(ws, WS::B_FJ), gr.M,
        at<double>(ws, b ? WS::B_FAC1 : WS::B_FAC0));
    pgo_assemble_kernel<<<dim3((unsigned)gr.nb), dim3(kBlock), 0, stream>>>(
        at<double>(ws, b ? WS::B_FAC1 : WS::B_FAC0), gr.M, at<int>(ws, WS::B_ROWPTR), at<int>(ws, WS::B_ENTRIES), gr.n,
        at<double>(ws, b ? WS::B_G1 : WS::B_G0), at<double>(ws, b ? WS::B_D1 : WS::B_D0), at<double>(ws, WS::B_PART_COST), at<double>(ws, WS::B_PART_GMAX));
    pgo_finish_kernel<<<dim3(1), dim3(kBlock), 0, stream>>>(at<double>(ws, WS::B_PART_COST), at<double>(ws, WS::B_PART_GMAX),
                                                            with_step ? at<double>(ws, WS::B_PART_STEP) : nullptr, gr.nb, at<PgoRecord>(ws, WS::B_REC));
    PGO_HIP(hipGetLastError());
    if (gr.timing) PGO_HIP(hipEventRecord(ws->ev[1], stream));
    return SCL_OK;
}

int read_record(WS *ws, hipStream_t stream, PgoRecord *rec, std::string *err)
{
    PGO_HIP(hipMemcpyAsync(rec, ws->buf[WS::B_REC], sizeof *rec, hipMemcpyDeviceToHost, stream));
    PGO_HIP(hipStreamSynchronize(stream));
    return SCL_OK;
}

int add_timing(WS *ws, Graph *gr, bool lin, bool solve, std::string *err)
{
    float ms = 0.f;
    if (!gr->timing) return SCL_OK;
    if (lin) { PGO_HIP(hipEventElapsedTime(&ms, ws->ev[0], ws->ev[1])); gr->lin_ms += ms; }
    if (solve) { PGO_HIP(hipEventElapsedTime(&ms, ws->ev[2], ws->ev[3])); gr->solve_ms += ms; }
    ws->linearize_ms = gr->lin_ms; ws->solve_ms = gr->solve_ms;
    return SCL_OK;
}

// the damped system of side b solved into B_VX and the poses of side b retracted into side 1 - b; reads the flag once per kCgBlock iterations
int enqueue_solve(WS *ws, hipStream_t stream, const Graph &gr, int b, double lambda, const scl_pgo_params &prm, std::string *err)
{
    const dim3 grid((unsigned)gr.nb), block(kBlock);
    const double *g = at<double>(ws, b ? WS::B_G1 : WS::B_G0), *D = at<double>(ws, b ? WS::B_D1 : WS::B_D0);
    const double *fac = at<double>(ws, b ? WS::B_FAC1 : WS::B_FAC0);
    PgoRecord *rec = at<PgoRecord>(ws, WS::B_REC);
    double *part_rz[2] = {at<double>(ws, WS::B_PART_RZ0), at<double>(ws, WS::B_PART_RZ1)};
    double *pv[2] = {at<double>(ws, WS::B_VP0), at<double>(ws, WS::B_VP1)};
    if (gr.timing) PGO_HIP(hipEventRecord(ws->ev[2], stream));
    pgo_pcg_init_kernel<<<grid, block, 0, stream>>>(g, D, lambda, gr.n, at<double>(ws, WS::B_LBLK), at<double>(ws, WS::B_VX), at<double>(ws, WS::B_VR),
                                                    at<double>(ws, WS::B_VZ), part_rz[0], rec);
    const double tol2 = prm.cg_tolerance * prm.cg_tolerance;
    for (int t = 0; t < prm.cg_max_iterations; ++t) {
        pgo_pcg_a_kernel<<<grid, block, 0, stream>>>(t, fac, gr.M, at<int>(ws, WS::B_FI), at<int>(ws, WS::B_FJ), at<int>(ws, WS::B_ROWPTR),
                                                     at<int>(ws, WS::B_ENTRIES), gr.n, gr.nb, D, lambda, tol2, at<double>(ws, WS::B_VZ), pv[(t + 1) & 1],
                                                     pv[t & 1], at<double>(ws, WS::B_VQ), part_rz[t & 1], part_rz[(t + 1) & 1],
                                                     at<double>(ws, WS::B_PART_PQ), rec);
        pgo_pcg_b_kernel<<<grid, block, 0, stream>>>(gr.n, gr.nb, at<double>(ws, WS::B_LBLK), pv[t & 1], at<double>(ws, WS::B_VQ), at<double>(ws, WS::B_VX),
                                                     at<double>(ws, WS::B_VR), at<double>(ws, WS::B_VZ), part_rz[t & 1], at<double>(ws, WS::B_PART_PQ),
                                                     part_rz[(t + 1) & 1], rec);
        if ((t + 1) % kCgBlock == 0 && t + 1 < prm.cg_max_iterations) {
            PgoRecord h;
            PGO_HIP(hipGetLastError());
            const int rc = read_record(ws, stream, &h, err);
            if (rc) return rc;
            if (h.flag) break;
        }
    }
    pgo_retract_kernel<<<grid, block, 0, stream>>>(at<double>(ws, b ? WS::B_X1 : WS::B_X0), at<double>(ws, WS::B_VX), gr.n,
                                                   at<double>(ws, b ? WS::B_X0 : WS::B_X1), at<double>(ws, WS::B_PART_STEP));
    PGO_HIP(hipGetLastError());
    if (gr.timing) PGO_HIP(hipEventRecord(ws->ev[3], stream));
    return SCL_OK;
}

}  // namespace

void pgo_workspace_free(PgoWorkspace *ws)
{
    for (int k = 0; k < PgoWorkspace::B_COUNT; ++k) {
        if (ws->buf[k]) (void)hipFree(ws->buf[k]);
        ws->buf[k] = nullptr; ws->cap[k] = 0;
    }
    for (hipEvent_t &ev : ws->ev) { if (ev) (void)hipEventDestroy(ev); ev = nullptr; }
    for (hipEvent_t &ev : ws->ev_c) { if (ev) (void)hipEventDestroy(ev); ev = nullptr; }
}

void pgo_default_params(scl_pgo_params *p)
{
    p->max_iterations = 50;
    p->lambda_initial = 1e-5; p->lambda_factor = 10.0; p->lambda_max = 1e10;
    p->relative_cost_tolerance = 1e-10; p->step_tolerance = 1e-10;
    p->cg_tolerance = 1e-8; p->cg_max_iterations = 500;
}

const char *pgo_params_bad(const scl_pgo_params &p)
{
    const double d[6] = {p.lambda_initial, p.lambda_factor, p.lambda_max, p.relative_cost_tolerance, p.step_tolerance, p.cg_tolerance};
    for (double v : d) if (!std::isfinite(v) || !(v > 0.0)) return "a params field that is not finite and positive";
    if (p.max_iterations < 1 || p.cg_max_iterations < 1) return "a params field that is not finite and positive";
    if (!(p.lambda_factor > 1.0)) return "lambda_factor <= 1";
    return nullptr;
}

const char *pgo_inputs_bad(const PgoInputs &in)
{
    if (in.n_poses < 0 || in.n_factors < 0 || in.n_priors < 0) return "a negative count";
    if (in.n_poses == 0) return "no pose";
    if (in.n_poses > SCL_PGO_MAX_POSES) return "more than 1048576 poses";
    if (in.n_factors > SCL_PGO_MAX_FACTORS) return "more than 4194304 factors";
    if (in.n_priors > in.n_poses) return "more priors than poses";
    if (!in.poses) return "poses == NULL";
    if (in.n_factors > 0 && (!in.f_i || !in.f_j || !in.f_z || !in.f_cov)) return "a factor array is NULL";
    if (in.n_priors > 0 && (!in.p_idx || !in.p_z || !in.p_cov)) return "a prior array is NULL";
    if (!finite_all(in.poses, 7 * (size_t)in.n_poses) || !finite_all(in.f_z, 7 * (size_t)in.n_factors) || !finite_all(in.p_z, 7 * (size_t)in.n_priors))
        return "a non-finite pose";
    if (!quaternions_ok(in.poses, in.n_poses) || !quaternions_ok(in.f_z, in.n_factors) || !quaternions_ok(in.p_z, in.n_priors))
        return "a quaternion's squared norm outside [0.25, 4]";
    const int cf = covariances_bad(in.f_cov, in.n_factors), cp = cf ? 0 : covariances_bad(in.p_cov, in.n_priors);
    if (cf == 1 || cp == 1) return "a non-finite covariance";
    if (cf == 2 || cp == 2) return "a covariance with a pivot not above 2^-43 of its diagonal entry";
    // the indices' range, f_i == f_j and the components' priors: pgo_graph.hpp, which nothing above needed
    return pgo_graph_bad(in.n_poses, in.f_i, in.f_j, in.n_factors, in.p_idx, in.n_priors);
}

int pgo_linearize(PgoWorkspace *ws, hipStream_t stream, const PgoInputs &in, double *cost, double *gradient, double *diag, double *chi2,
                  bool timing, std::string *err)
{
    Graph gr;
    int rc;
    if ((rc = setup(ws, stream, in, timing, &gr, err)) || (rc = enqueue_linearise(ws, stream, gr, 0, false, err))) return rc;
    const size_t nn = (size_t)gr.n;
    std::vector<double> g(gradient ? 6 * nn : 0), D(diag ? 21 * nn : 0), c2(chi2 ? (size_t)gr.M : 0);
    if (gradient) PGO_HIP(hipMemcpyAsync(g.data(), ws->buf[WS::B_G0], sizeof(double) * 6 * nn, hipMemcpyDeviceToHost, stream));
    if (diag) PGO_HIP(hipMemcpyAsync(D.data(), ws->buf[WS::B_D0], sizeof(double) * 21 * nn, hipMemcpyDeviceToHost, stream));
    if (chi2) PGO_HIP(hipMemcpyAsync(c2.data(), ws->buf[WS::B_FAC0], sizeof(double) * (size_t)gr.M, hipMemcpyDeviceToHost, stream));
    PgoRecord rec;
    if ((rc = read_record(ws, stream, &rec, err)) || (rc = add_timing(ws, &gr, true, false, err))) return rc;
    // into the caller's arrays only once the whole call has run
    if (cost) *cost = rec.cost;
    if (gradient) std::memcpy(gradient, g.data(), sizeof(double) * 6 * nn);
    if (chi2) std::memcpy(chi2, c2.data(), sizeof(double) * (size_t)gr.M);
    if (diag)
        for (size_t p = 0; p < nn; ++p)
            for (int a = 0; a < 6; ++a)
                for (int b = 0; b < 6; ++b) diag[36 * p + 6 * (size_t)a + (size_t)b] = D[21 * p + (size_t)(a <= b ? tri(a, b) : tri(b, a))];
    return SCL_OK;
}

int pgo_hessian_apply(PgoWorkspace *ws, hipStream_t stream, const PgoInputs &in, double lambda, const double *x, double *y, bool timing,
                      std::string *err)
{
    Graph gr;
    int rc;
    if ((rc = setup(ws, stream, in, timing, &gr, err))) return rc;
    const size_t nn = (size_t)gr.n;
    PGO_HIP(hipMemcpyAsync(ws->buf[WS::B_XIN], x, sizeof(double) * 6 * nn, hipMemcpyHostToDevice, stream));
    PGO_HIP(hipStreamSynchronize(stream));
    if ((rc = enqueue_linearise(ws, stream, gr, 0, false, err))) return rc;
    if (gr.timing) PGO_HIP(hipEventRecord(ws->ev[2], stream));
    pgo_apply_kernel<<<dim3((unsigned)gr.nb), dim3(kBlock), 0, stream>>>(at<double>(ws, WS::B_FAC0), gr.M, at<int>(ws, WS::B_FI), at<int>(ws, WS::B_FJ),
                                                                         at<int>(ws, WS::B_ROWPTR), at<int>(ws, WS::B_ENTRIES), gr.n, at<double>(ws, WS::B_D0),
                                                                         lambda, at<double>(ws, WS::B_XIN), at<double>(ws, WS::B_VQ));
    PGO_HIP(hipGetLastError());
    if (gr.timing) PGO_HIP(hipEventRecord(ws->ev[3], stream));
    std::vector<double> out(6 * nn);
    PGO_HIP(hipMemcpyAsync(out.data(), ws->buf[WS::B_VQ], sizeof(double) * 6 * nn, hipMemcpyDeviceToHost, stream));
    PGO_HIP(hipStreamSynchronize(stream));
    if ((rc = add_timing(ws, &gr, true, true, err))) return rc;
    std::memcpy(y, out.data(), sizeof(double) * 6 * nn);
    return SCL_OK;
}

int pgo_setup(PgoWorkspace *ws, hipStream_t stream, const PgoInputs &in, bool timing, PgoGraph *gr, std::string *err)
{
    return setup(ws, stream, in, timing, gr, err);
}

int pgo_enqueue_linearise(PgoWorkspace *ws, hipStream_t stream, const PgoGraph &gr, int b, bool with_step, std::string *err)
{
    return enqueue_linearise(ws, stream, gr, b, with_step, err);
}

int pgo_read_record(PgoWorkspace *ws, hipStream_t stream, PgoRecord *rec, std::string *err) { return read_record(ws, stream, rec, err); }

int pgo_add_timing(PgoWorkspace *ws, PgoGraph *gr, bool lin, bool solve, std::string *err) { return add_timing(ws, gr, lin, solve, err); }

int pgo_ensure(PgoWorkspace *ws, int k, size_t bytes, std::string *err) { return ensure(ws, k, bytes, err); }

int pgo_enqueue_retract(PgoWorkspace *ws, hipStream_t stream, const PgoGraph &gr, int b, std::string *err)
{
    pgo_retract_kernel<<<dim3((unsigned)gr.nb), dim3(kBlock), 0, stream>>>(at<double>(ws, b ? WS::B_X1 : WS::B_X0), at<double>(ws, WS::B_VX), gr.n,
                                                                           at<double>(ws, b ? WS::B_X0 : WS::B_X1), at<double>(ws, WS::B_PART_STEP));
    PGO_HIP(hipGetLastError());
    return SCL_OK;
}

int pgo_optimize(PgoWorkspace *ws, hipStream_t stream, const PgoInputs &in, const scl_pgo_params &prm, double *poses_out,
                 scl_pgo_result *result, double *chi2, bool timing, std::string *err)
{
    const PgoSolveFn pcg = [&prm](PgoWorkspace *w, hipStream_t st, const PgoGraph &gr, int b, double lambda, std::string *e) {
        return enqueue_solve(w, st, gr, b, lambda, prm, e);
    };
    return pgo_lm(ws, stream, in, prm, pcg, false, poses_out, result, chi2, nullptr, timing, err);
}

int pgo_lm(PgoWorkspace *ws, hipStream_t stream, const PgoInputs &in, const scl_pgo_params &prm, const PgoSolveFn &solve, bool direct,
           double *poses_out, scl_pgo_result *result, double *chi2, int *failed_factorisations, bool timing, std::string *err)
{
    Graph gr;
    int rc;
    PgoRecord rec;
    if ((rc = setup(ws, stream, in, timing, &gr, err)) || (rc = enqueue_linearise(ws, stream, gr, 0, false, err)) ||
        (rc = read_record(ws, stream, &rec, err)) || (rc = add_timing(ws, &gr, true, false, err)))
        return rc;
    scl_pgo_result res;
    std::memset(&res, 0, sizeof res);
    int cur = 0, failed = 0;
    double cost = rec.cost, gmax = rec.gmax, lambda = prm.lambda_initial;
    res.initial_cost = cost;
    for (;;) {
        if ((rc = solve(ws, stream, gr, cur, lambda, err)) || (rc = enqueue_linearise(ws, stream, gr, 1 - cur, true, err)) ||
            (rc = read_record(ws, stream, &rec, err)) || (rc = add_timing(ws, &gr, true, true, err)))
            return rc;
        ++res.iterations;
        if (!direct) res.cg_iterations += rec.cg;
        bool stop_cost = false;
        if (direct && rec.fail) {                              // a failed pivot: no step was taken
            ++res.rejected; ++failed;
            lambda *= prm.lambda_factor;
            if (res.iterations >= prm.max_iterations) { res.stop_reason = SCL_PGO_STOP_ITERATIONS; break; }
            if (lambda > prm.lambda_max) { res.stop_reason = SCL_PGO_STOP_LAMBDA; break; }
            continue;
        }
        if (rec.cost < cost) {
            stop_cost = cost - rec.cost <= prm.relative_cost_tolerance * cost;
            cost = rec.cost; gmax = rec.gmax; cur = 1 - cur;
            ++res.accepted;
            lambda /= prm.lambda_factor;
        } else {
            ++res.rejected;
            lambda *= prm.lambda_factor;
        }
        if (stop_cost) { res.stop_reason = SCL_PGO_STOP_COST; break; }
        if (rec.step <= prm.step_tolerance) { res.stop_reason = SCL_PGO_STOP_STEP; break; }
        if (res.iterations >= prm.max_iterations) { res.stop_reason = SCL_PGO_STOP_ITERATIONS; break; }
        if (lambda > prm.lambda_max) { res.stop_reason = SCL_PGO_STOP_LAMBDA; break; }
    }
    res.final_cost = cost; res.final_lambda = lambda; res.gradient_max = gmax;
    const size_t nn = (size_t)gr.n;
    pgo_output_kernel<<<dim3((unsigned)gr.nb), dim3(kBlock), 0, stream>>>(at<double>(ws, cur ? WS::B_X1 : WS::B_X0), gr.n, at<double>(ws, WS::B_POSES_OUT));
    PGO_HIP(hipGetLastError());
    std::vector<double> out(7 * nn), c2(chi2 ? (size_t)gr.M : 0);
    PGO_HIP(hipMemcpyAsync(out.data(), ws->buf[WS::B_POSES_OUT], sizeof(double) * 7 * nn, hipMemcpyDeviceToHost, stream));
    if (chi2) PGO_HIP(hipMemcpyAsync(c2.data(), ws->buf[cur ? WS::B_FAC1 : WS::B_FAC0], sizeof(double) * (size_t)gr.M, hipMemcpyDeviceToHost, stream));
    PGO_HIP(hipStreamSynchronize(stream));
    std::memcpy(poses_out, out.data(), sizeof(double) * 7 * nn);
    if (chi2) std::memcpy(chi2, c2.data(), sizeof(double) * (size_t)gr.M);
    *result = res;
    if (failed_factorisations) *failed_factorisations = failed;
    return SCL_OK;
}

}  // namespace scl
