// pgo_condensed.hip -- the condensed direct step of the pose-graph solve (contract: include/scl_engine.h "POSE-GRAPH SOLVE, CONDENSED
// DIRECT STEP"): (H + lambda diag H) delta = -g solved exactly.  Every run of interior poses (a segment) is eliminated by block cyclic
// reduction over its path, what that leaves on the path's two ends is added into a dense matrix S over the junctions, S is factored by a
// blocked Cholesky, and the interior is recovered level by level.  The linearisation, assembly, finish and retraction are pgo.hip's,
// and so is the LM loop (pgo_lm).  All fp64, no atomics on floats.  Plan: pgo_condense_plan.hpp (host).
//
//   cond_setup_kernel         one thread per path node: the damped diagonal block and -g of an interior pose (zeros on a path's ends),
//                             the coupling (node, next node) from the W planes
//   cond_eliminate_kernel     one level, one thread per eliminated node m with neighbours l, r: D_m = L L^T, P = L^-1 U_l^T, Q = L^-1 U_m,
//                             w = L^-1 b_m; the contributions -P^T P, -P^T w (to l) and -Q^T Q, -Q^T w (to r) into m's own slots, the new
//                             coupling U_l = -P^T Q.  L, P, Q, w stay in the node for the way back.  Segments of all lengths share it.
//   cond_absorb_kernel        the level's survivors take the slot of the node eliminated on their left, then of the one on their right
//   cond_gather_kernel        one thread per entry of a (junction, junction) block of S: its sources in the plan's order
//   cond_rhs_kernel           the junctions' right-hand side, the original diagonal of S, the padding of S to a multiple of 32
//   cond_chol_panel_kernel    panel p: every workgroup factors the 32 x 32 diagonal block in LDS (the first one stores it), then solves
//                             64 rows of the column below it
//   cond_chol_update_kernel   the trailing update, a 32 x 32 tile per wave on v_mfma_f64_16x16x4_f64
//   cond_tri_solve_kernel     L y = b and L^T x = y, one workgroup, panel by panel
//   cond_scatter_kernel       delta of the junctions; the paths' ends take theirs
//   cond_back_kernel          one level back: x_m = L^-T (w - P x_l - Q x_r)
// What the first three stages leave -- L, P, Q of every node, the factor of S -- is also what pgo_marginals.hip solves many columns on
// (pgo_condensed_factor: the same launches up to the factorisation).
#include "pgo.hpp"
#include "pgo_blocks.hpp"
#include "pgo_condense_plan.hpp"

#include <cstring>
#include <vector>

namespace scl {

namespace {

using namespace pgo_blocks;

constexpr int kNodeBlock = 64;     // the per-node kernels hold two 6 x 6 blocks and a factor in registers
constexpr int kNB = 32;            // the panel width of the dense Cholesky
constexpr int kSolveThreads = 512;
typedef double double4_t __attribute__((ext_vector_type(4)));

// symmetric block given by its upper triangle
__device__ inline double sym(const double *T, int a, int b) { return a <= b ? T[tri(a, b)] : T[tri(b, a)]; }

// node_kind[i] >= 0: the pose of an interior node; < 0: an end of a path, -1 - its junction
__global__ __launch_bounds__(kNodeBlock) void cond_setup_kernel(int n_nodes, const int *node_kind, const int *node_coupling, const double *g,
                                                                 const double *D, double lambda, const double *fac, int M, double *ND,
                                                                 double *NBv, double *NU, PgoRecord *rec)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i == 0) { rec->fail = 0; rec->cg = 0; }
    if (i >= n_nodes) return;
    const int pose = node_kind[i];
    double *d = ND + 21 * (size_t)i, *b = NBv + 6 * (size_t)i;
    if (pose >= 0) {
        for (int a = 0; a < 21; ++a) d[a] = D[21 * (size_t)pose + a];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const double v = D[21 * (size_t)pose + tri(a, a)];
            d[tri(a, a)] = v + lambda * v;
            b[a] = -g[6 * (size_t)pose + a];
        }
    } else {
        for (int a = 0; a < 21; ++a) d[a] = 0.0;
        for (int a = 0; a < 6; ++a) b[a] = 0.0;
    }
    const int c = node_coupling[i];
    if (c < 0) return;
    const double *W = fac + (size_t)kFacW * (size_t)M + (c >> 1);
    double *U = NU + 36 * (size_t)i;
    for (int a = 0; a < 6; ++a)
        for (int bb = 0; bb < 6; ++bb) U[6 * a + bb] = (c & 1) ? W[(size_t)(6 * bb + a) * (size_t)M] : W[(size_t)(6 * a + bb) * (size_t)M];
}

__global__ __launch_bounds__(kNodeBlock) void cond_eliminate_kernel(const int *elim, int count, double *ND, double *NBv, double *NU, double *NP,
                                                                     double *NCL, double *NCR, PgoRecord *rec)
{
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= count) return;
    const int m = elim[3 * e], l = elim[3 * e + 1];
    double S[21], L[21], PT[36], Q[36], w[6];
#pragma unroll
    for (int a = 0; a < 21; ++a) S[a] = ND[21 * (size_t)m + a];
    if (!chol6_checked(S, L)) rec->fail = 1;               // the same word from every thread that fails
#pragma unroll
    for (int a = 0; a < 21; ++a) ND[21 * (size_t)m + a] = L[a];
    // PT[c][.] = column c of P = L^-1 U_l^T, i.e. L^-1 applied to row c of U_l; Q = L^-1 U_m column by column
#pragma unroll
    for (int a = 0; a < 36; ++a) { PT[a] = NU[36 * (size_t)l + a]; Q[a] = NU[36 * (size_t)m + a]; }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        forward6(L, PT + 6 * c);
        double col[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) col[a] = Q[6 * a + c];
        forward6(L, col);
#pragma unroll
        for (int a = 0; a < 6; ++a) Q[6 * a + c] = col[a];
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) w[a] = NBv[6 * (size_t)m + a];
    forward6(L, w);
    double *cl = NCL + 27 * (size_t)m, *cr = NCR + 27 * (size_t)m, *U = NU + 36 * (size_t)l;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
#pragma unroll
        for (int d = c; d < 6; ++d) {
            double sl = 0.0, sr = 0.0;
#pragma unroll
            for (int a = 0; a < 6; ++a) { sl += PT[6 * c + a] * PT[6 * d + a]; sr += Q[6 * a + c] * Q[6 * a + d]; }
            cl[tri(c, d)] = -sl; cr[tri(c, d)] = -sr;
        }
        double gl = 0.0, gr = 0.0;
#pragma unroll
        for (int a = 0; a < 6; ++a) { gl += PT[6 * c + a] * w[a]; gr += Q[6 * a + c] * w[a]; }
        cl[21 + c] = -gl; cr[21 + c] = -gr;
#pragma unroll
        for (int d = 0; d < 6; ++d) {
            double u = 0.0;
#pragma unroll
            for (int a = 0; a < 6; ++a) u += PT[6 * c + a] * Q[6 * a + d];
            U[6 * c + d] = -u;
        }
    }
#pragma unroll
    for (int a = 0; a < 36; ++a) { NP[36 * (size_t)m + a] = PT[a]; NU[36 * (size_t)m + a] = Q[a]; }
#pragma unroll
    for (int a = 0; a < 6; ++a) NBv[6 * (size_t)m + a] = w[a];
}

__global__ __launch_bounds__(256) void cond_absorb_kernel(const int *absorb, int count, double *ND, double *NBv, const double *NCL, const double *NCR)
{
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= count) return;
    const int s = absorb[3 * e], le = absorb[3 * e + 1], re = absorb[3 * e + 2];
    double *d = ND + 21 * (size_t)s, *b = NBv + 6 * (size_t)s;
    if (le >= 0) {                                         // the node eliminated on the left gave this one its right contribution
        const double *c = NCR + 27 * (size_t)le;
        for (int a = 0; a < 21; ++a) d[a] = d[a] + c[a];
        for (int a = 0; a < 6; ++a) b[a] = b[a] + c[21 + a];
    }
    if (re >= 0) {
        const double *c = NCL + 27 * (size_t)re;
        for (int a = 0; a < 21; ++a) d[a] = d[a] + c[a];
        for (int a = 0; a < 6; ++a) b[a] = b[a] + c[21 + a];
    }
}

__global__ __launch_bounds__(256) void cond_gather_kernel(int n_blocks, const int *block_ptr, const int *block_rc, const int *src, const double *D,
                                                           double lambda, const double *fac, int M, const double *ND, const double *NU,
                                                           double *S, int ld)
{
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= 36 * n_blocks) return;
    const int blk = t / 36, a = (t % 36) / 6, c = t % 6;
    double v = 0.0;
    for (int s = block_ptr[blk]; s < block_ptr[blk + 1]; ++s) {
        const int kind = src[2 * s], idx = src[2 * s + 1];
        double term;
        if (kind == kSrcDiag) {
            term = sym(D + 21 * (size_t)idx, a, c);
            if (a == c) term = term + lambda * term;
        } else if (kind == kSrcW || kind == kSrcWT) {
            const double *W = fac + (size_t)kFacW * (size_t)M + idx;
            term = kind == kSrcW ? W[(size_t)(6 * a + c) * (size_t)M] : W[(size_t)(6 * c + a) * (size_t)M];
        } else if (kind == kSrcEnd) {
            term = sym(ND + 21 * (size_t)idx, a, c);
        } else {
            term = NU[36 * (size_t)idx + 6 * c + a];
        }
        v = v + term;
    }
    S[(size_t)(6 * block_rc[2 * blk] + a) * (size_t)ld + (size_t)(6 * block_rc[2 * blk + 1] + c)] = v;
}

// row i < 6 n_junctions: b_i = -g + the ends' updates, and the diagonal entry of S as assembled (the pivot rule's reference); the rows
// behind them pad S with the identity
__global__ __launch_bounds__(256) void cond_rhs_kernel(int n_rows, int ld, const int *jpose, const int *rhs_ptr, const int *rhs_src, const double *g,
                                                        const double *NBv, double *S, double *diag0, double *rhs)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= ld) return;
    if (i >= n_rows) { S[(size_t)i * (size_t)ld + i] = 1.0; diag0[i] = 1.0; rhs[i] = 0.0; return; }
    const int j = i / 6, a = i % 6;
    double v = -g[6 * (size_t)jpose[j] + a];
    for (int s = rhs_ptr[j]; s < rhs_ptr[j + 1]; ++s) v = v + NBv[6 * (size_t)rhs_src[s] + a];
    rhs[i] = v;
    diag0[i] = S[(size_t)i * (size_t)ld + i];
}

// Panel p of the lower triangle of S (row-major, ld a multiple of kNB).  The factored diagonal block goes to Ldiag + 1024 p and S keeps
// the block as it was, so that the workgroups of this launch all read the same; the column below becomes L in place.
__global__ __launch_bounds__(64) void cond_chol_panel_kernel(double *S, int ld, int p, const double *diag0, double *Ldiag, PgoRecord *rec)
{
    __shared__ double L[kNB][kNB + 1];
    const int tid = (int)threadIdx.x, c0 = p * kNB;
    for (int e = tid; e < kNB * kNB; e += 64) {
        const int r = e / kNB, c = e % kNB;
        L[r][c] = c <= r ? S[(size_t)(c0 + r) * (size_t)ld + (size_t)(c0 + c)] : 0.0;
    }
    __syncthreads();
    for (int c = 0; c < kNB; ++c) {
        double s = 0.0;
        if (tid >= c && tid < kNB) {
            s = L[tid][c];
            for (int k = 0; k < c; ++k) s -= L[tid][k] * L[c][k];
        }
        if (tid == c) {
            if (!(s > diag0[c0 + c] * 0x1p-43) && blockIdx.x == 0) rec->fail = 1;
            L[c][c] = sqrt(s);
        }
        __syncthreads();
        if (tid > c && tid < kNB) L[tid][c] = s / L[c][c];
        __syncthreads();
    }
    if (blockIdx.x == 0)
        for (int e = tid; e < kNB * kNB; e += 64) Ldiag[(size_t)p * (kNB * kNB) + e] = L[e / kNB][e % kNB];
    const int r = c0 + kNB + (int)blockIdx.x * 64 + tid;
    if (r >= ld) return;
    double *row = S + (size_t)r * (size_t)ld + c0;
    double x[kNB];
#pragma unroll
    for (int c = 0; c < kNB; ++c) x[c] = row[c];
#pragma unroll
    for (int c = 0; c < kNB; ++c) {
        double s = x[c];
#pragma unroll
        for (int k = 0; k < c; ++k) s -= x[k] * L[c][k];
        x[c] = s / L[c][c];
    }
#pragma unroll
    for (int c = 0; c < kNB; ++c) row[c] = x[c];
}

// Tile (I, J), J <= I, of the matrix behind panel p: C -= L_I L_J^T with the two 32 x 32 pieces of the panel's column.  A wave per
// tile; v_mfma_f64_16x16x4_f64 takes A[row lane & 15][k = lane >> 4] and B[k = lane >> 4][col lane & 15] and leaves
// D[row (lane >> 4) + 4 v][col lane & 15] in its v-th result.
__global__ __launch_bounds__(64) void cond_chol_update_kernel(double *S, int ld, int p)
{
    const int I = (int)blockIdx.y, J = (int)blockIdx.x;
    if (J > I) return;
    const int lane = (int)threadIdx.x, r16 = lane & 15, k4 = lane >> 4;
    const size_t row0 = (size_t)(p + 1 + I) * kNB, col0 = (size_t)(p + 1 + J) * kNB, k0 = (size_t)p * kNB, LD = (size_t)ld;
    double a[2][8], b[2][8];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            a[h][kk] = S[(row0 + 16 * h + r16) * LD + k0 + 4 * kk + k4];
            b[h][kk] = S[(col0 + 16 * h + r16) * LD + k0 + 4 * kk + k4];
        }
#pragma unroll
    for (int ib = 0; ib < 2; ++ib)
#pragma unroll
        for (int jb = 0; jb < 2; ++jb) {
            double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ib][kk], b[jb][kk], acc, 0, 0, 0);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                double *c = S + (row0 + 16 * ib + k4 + 4 * v) * LD + col0 + 16 * jb + r16;
                *c = *c - acc[v];
            }
        }
}

// y <- L^-T L^-1 y for the factor the two kernels above left (Ldiag: the diagonal blocks, S: the rest), one workgroup
__global__ __launch_bounds__(kSolveThreads) void cond_tri_solve_kernel(const double *S, int ld, const double *Ldiag, double *y)
{
    __shared__ double xp[kNB];
    const int tid = (int)threadIdx.x, T = ld / kNB, r = tid & (kNB - 1);
    const size_t LD = (size_t)ld;
    for (int p = 0; p < T; ++p) {
        if (tid < 64) {                                    // the first wave: lane r holds row r of the diagonal block
            double row[kNB];
#pragma unroll
            for (int k = 0; k < kNB; ++k) row[k] = Ldiag[(size_t)p * (kNB * kNB) + r * kNB + k];
            double x = y[p * kNB + r];
#pragma unroll
            for (int c = 0; c < kNB; ++c) {
                const double v = __shfl(x / row[c], c, 64);
                if (r > c) x -= row[c] * v;
                else if (r == c) x = v;
            }
            if (tid < kNB) { xp[r] = x; y[p * kNB + r] = x; }
        }
        __syncthreads();
        for (int q = (p + 1) * kNB + tid; q < ld; q += kSolveThreads) {
            const double *Lq = S + (size_t)q * LD + (size_t)p * kNB;
            double s = y[q];
#pragma unroll
            for (int k = 0; k < kNB; ++k) s -= Lq[k] * xp[k];
            y[q] = s;
        }
        __syncthreads();
    }
    for (int p = T - 1; p >= 0; --p) {
        if (tid < 64) {                                    // lane r holds column r of the diagonal block
            double col[kNB];
#pragma unroll
            for (int k = 0; k < kNB; ++k) col[k] = Ldiag[(size_t)p * (kNB * kNB) + k * kNB + r];
            double x = y[p * kNB + r];
#pragma unroll
            for (int c = kNB - 1; c >= 0; --c) {
                const double v = __shfl(x / col[c], c, 64);
                if (r < c) x -= col[c] * v;
                else if (r == c) x = v;
            }
            if (tid < kNB) { xp[r] = x; y[p * kNB + r] = x; }
        }
        __syncthreads();
        for (int q = tid; q < p * kNB; q += kSolveThreads) {
            double s = y[q];
#pragma unroll
            for (int k = 0; k < kNB; ++k) s -= S[(size_t)(p * kNB + k) * LD + q] * xp[k];
            y[q] = s;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void cond_scatter_kernel(int n_junctions, const int *jpose, int n_nodes, const int *node_kind, const double *x,
                                                            double *delta, double *NX)
{
    int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t < n_junctions) {
        for (int a = 0; a < 6; ++a) delta[6 * (size_t)jpose[t] + a] = x[6 * (size_t)t + a];
        return;
    }
    t -= n_junctions;
    if (t >= n_nodes || node_kind[t] >= 0) return;
    const int j = -1 - node_kind[t];
    for (int a = 0; a < 6; ++a) NX[6 * (size_t)t + a] = x[6 * (size_t)j + a];
}

__global__ __launch_bounds__(kNodeBlock) void cond_back_kernel(const int *elim, int count, const int *node_kind, const double *ND, const double *NBv,
                                                                const double *NU, const double *NP, double *NX, double *delta)
{
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= count) return;
    const int m = elim[3 * e], l = elim[3 * e + 1], r = elim[3 * e + 2];
    double L[21], v[6], xl[6], xr[6];
#pragma unroll
    for (int a = 0; a < 21; ++a) L[a] = ND[21 * (size_t)m + a];
#pragma unroll
    for (int a = 0; a < 6; ++a) { v[a] = NBv[6 * (size_t)m + a]; xl[a] = NX[6 * (size_t)l + a]; xr[a] = NX[6 * (size_t)r + a]; }
    const double *PT = NP + 36 * (size_t)m, *Q = NU + 36 * (size_t)m;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) s += PT[6 * c + a] * xl[c];
        v[a] = v[a] - s;
        s = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) s += Q[6 * a + c] * xr[c];
        v[a] = v[a] - s;
    }
    backward6(L, v);
    const int pose = node_kind[m];
#pragma unroll
    for (int a = 0; a < 6; ++a) { NX[6 * (size_t)m + a] = v[a]; delta[6 * (size_t)pose + a] = v[a]; }
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
template <class T> T *at(WS *ws, int k) { return static_cast<T *>(ws->buf[k]); }

using Condensed = PgoCondensed;

int upload(WS *ws, hipStream_t stream, int k, const std::vector<int> &v, std::string *err)
{
    const int rc = pgo_ensure(ws, k, sizeof(int) * v.size(), err);
    if (rc) return rc;
    if (!v.empty()) PGO_HIP(hipMemcpyAsync(ws->buf[k], v.data(), sizeof(int) * v.size(), hipMemcpyHostToDevice, stream));
    return SCL_OK;
}

// the plan to the device and the buffers of a step; after pgo_setup, whose buffers the step reads
int prepare(WS *ws, hipStream_t stream, const PgoInputs &in, bool timing, Condensed *C, std::string *err)
{
    PgoCondensePlan P;
    pgo_condense_plan(in.n_poses, in.f_i, in.f_j, in.n_factors, in.p_idx, in.n_priors, &P);
    C->n_nodes = P.n_nodes; C->n_junctions = P.n_junctions; C->n_levels = P.n_levels;
    C->n_blocks = (int)P.block_rc.size() / 2;
    C->n_rows = 6 * P.n_junctions;
    C->ld = (C->n_rows + kNB - 1) / kNB * kNB;
    C->level_ptr = P.level_ptr; C->absorb_ptr = P.absorb_ptr;
    std::vector<int> node_kind((size_t)P.n_nodes);
    for (int s = 0; s < P.n_segments; ++s) {
        const int n0 = P.seg_node0[(size_t)s], n1 = P.seg_node0[(size_t)s + 1] - 1;
        for (int i = n0; i <= n1; ++i)
            node_kind[(size_t)i] = (i == n0 || i == n1) ? -1 - P.junction_of[(size_t)P.node_pose[(size_t)i]] : P.node_pose[(size_t)i];
    }
    int rc;
    if ((rc = upload(ws, stream, WS::B_C_NODE_POSE, node_kind, err)) || (rc = upload(ws, stream, WS::B_C_NODE_COUPLING, P.node_coupling, err)) ||
        (rc = upload(ws, stream, WS::B_C_ELIM, P.elim, err)) || (rc = upload(ws, stream, WS::B_C_ABSORB, P.absorb, err)) ||
        (rc = upload(ws, stream, WS::B_C_BLOCK_PTR, P.block_ptr, err)) || (rc = upload(ws, stream, WS::B_C_BLOCK_RC, P.block_rc, err)) ||
        (rc = upload(ws, stream, WS::B_C_SRC, P.src, err)) || (rc = upload(ws, stream, WS::B_C_RHS_PTR, P.rhs_ptr, err)) ||
        (rc = upload(ws, stream, WS::B_C_RHS_SRC, P.rhs_src, err)) || (rc = upload(ws, stream, WS::B_C_JPOSE, P.junction_pose, err)))
        return rc;
    const size_t nn = (size_t)P.n_nodes, ld = (size_t)C->ld;
    const struct { int k; size_t bytes; } need[] = {
        {WS::B_C_ND, sizeof(double) * 21 * nn}, {WS::B_C_NB, sizeof(double) * 6 * nn}, {WS::B_C_NU, sizeof(double) * 36 * nn},
        {WS::B_C_NP, sizeof(double) * 36 * nn}, {WS::B_C_NCL, sizeof(double) * 27 * nn}, {WS::B_C_NCR, sizeof(double) * 27 * nn},
        {WS::B_C_NX, sizeof(double) * 6 * nn}, {WS::B_C_S, sizeof(double) * ld * ld}, {WS::B_C_LDIAG, sizeof(double) * ld * kNB},
        {WS::B_C_DIAG0, sizeof(double) * ld}, {WS::B_C_RHS, sizeof(double) * ld}};
    for (const auto &b : need)
        if ((rc = pgo_ensure(ws, b.k, b.bytes, err))) return rc;
    if (timing) {
        for (hipEvent_t &ev : ws->ev_c)
            if (!ev) PGO_HIP(hipEventCreate(&ev));
        for (double &m : ws->condensed_ms) m = 0.0;
    }
    PGO_HIP(hipStreamSynchronize(stream));                 // the plan's vectors are pageable: nothing of them is read after this
    return SCL_OK;
}

// the events of the last timed step into the call's sums; the stream has been waited for since
int collect(WS *ws, Condensed *C, std::string *err)
{
    if (!C->pending) return SCL_OK;
    for (int k = 0; k < 4; ++k) {
        float ms = 0.f;
        PGO_HIP(hipEventElapsedTime(&ms, ws->ev_c[k], ws->ev_c[k + 1]));
        C->ms[k] += ms;
        ws->condensed_ms[k] = C->ms[k];
    }
    C->pending = false;
    return SCL_OK;
}

inline unsigned blocks_for(int count, int block) { return (unsigned)((count > 0 ? count : 1) + block - 1) / (unsigned)block; }

// the first three stages of a step on side b: elimination, assembly of S, factorisation
int enqueue_factor(WS *ws, hipStream_t stream, const PgoGraph &gr, Condensed *C, int b, double lambda, std::string *err)
{
    int rc;
    if ((rc = collect(ws, C, err))) return rc;
    const double *g = at<double>(ws, b ? WS::B_G1 : WS::B_G0), *D = at<double>(ws, b ? WS::B_D1 : WS::B_D0);
    const double *fac = at<double>(ws, b ? WS::B_FAC1 : WS::B_FAC0);
    PgoRecord *rec = at<PgoRecord>(ws, WS::B_REC);
    const int *node_kind = at<int>(ws, WS::B_C_NODE_POSE), *elim = at<int>(ws, WS::B_C_ELIM), *absorb = at<int>(ws, WS::B_C_ABSORB);
    double *ND = at<double>(ws, WS::B_C_ND), *NBv = at<double>(ws, WS::B_C_NB), *NU = at<double>(ws, WS::B_C_NU), *NP = at<double>(ws, WS::B_C_NP);
    double *NCL = at<double>(ws, WS::B_C_NCL), *NCR = at<double>(ws, WS::B_C_NCR);
    double *S = at<double>(ws, WS::B_C_S), *Ldiag = at<double>(ws, WS::B_C_LDIAG), *diag0 = at<double>(ws, WS::B_C_DIAG0), *rhs = at<double>(ws, WS::B_C_RHS);
    const int ld = C->ld, T = ld / kNB;
    if (gr.timing) PGO_HIP(hipEventRecord(ws->ev_c[0], stream));
    cond_setup_kernel<<<dim3(blocks_for(C->n_nodes, kNodeBlock)), dim3(kNodeBlock), 0, stream>>>(
        C->n_nodes, node_kind, at<int>(ws, WS::B_C_NODE_COUPLING), g, D, lambda, fac, gr.M, ND, NBv, NU, rec);
    for (int l = 0; l < C->n_levels; ++l) {
        const int e0 = C->level_ptr[(size_t)l], ne = C->level_ptr[(size_t)l + 1] - e0;
        const int a0 = C->absorb_ptr[(size_t)l], na = C->absorb_ptr[(size_t)l + 1] - a0;
        cond_eliminate_kernel<<<dim3(blocks_for(ne, kNodeBlock)), dim3(kNodeBlock), 0, stream>>>(elim + 3 * (size_t)e0, ne, ND, NBv, NU, NP, NCL, NCR, rec);
        cond_absorb_kernel<<<dim3(blocks_for(na, 256)), dim3(256), 0, stream>>>(absorb + 3 * (size_t)a0, na, ND, NBv, NCL, NCR);
    }
    PGO_HIP(hipGetLastError());
    if (gr.timing) PGO_HIP(hipEventRecord(ws->ev_c[1], stream));
    PGO_HIP(hipMemsetAsync(S, 0, sizeof(double) * (size_t)ld * (size_t)ld, stream));
    cond_gather_kernel<<<dim3(blocks_for(36 * C->n_blocks, 256)), dim3(256), 0, stream>>>(
        C->n_blocks, at<int>(ws, WS::B_C_BLOCK_PTR), at<int>(ws, WS::B_C_BLOCK_RC), at<int>(ws, WS::B_C_SRC), D, lambda, fac, gr.M, ND, NU, S, ld);
    cond_rhs_kernel<<<dim3(blocks_for(ld, 256)), dim3(256), 0, stream>>>(C->n_rows, ld, at<int>(ws, WS::B_C_JPOSE), at<int>(ws, WS::B_C_RHS_PTR),
                                                                         at<int>(ws, WS::B_C_RHS_SRC), g, NBv, S, diag0, rhs);
    PGO_HIP(hipGetLastError());
    if (gr.timing) PGO_HIP(hipEventRecord(ws->ev_c[2], stream));
    for (int p = 0; p < T; ++p) {
        const int below = ld - (p + 1) * kNB;
        cond_chol_panel_kernel<<<dim3(blocks_for(below, 64)), dim3(64), 0, stream>>>(S, ld, p, diag0, Ldiag, rec);
        if (below > 0) cond_chol_update_kernel<<<dim3((unsigned)(below / kNB), (unsigned)(below / kNB)), dim3(64), 0, stream>>>(S, ld, p);
    }
    PGO_HIP(hipGetLastError());
    if (gr.timing) PGO_HIP(hipEventRecord(ws->ev_c[3], stream));
    return SCL_OK;
}

// the damped system of side b solved into B_VX
int enqueue_step(WS *ws, hipStream_t stream, const PgoGraph &gr, Condensed *C, int b, double lambda, std::string *err)
{
    int rc;
    if ((rc = enqueue_factor(ws, stream, gr, C, b, lambda, err))) return rc;
    const int *node_kind = at<int>(ws, WS::B_C_NODE_POSE), *elim = at<int>(ws, WS::B_C_ELIM);
    const double *ND = at<double>(ws, WS::B_C_ND), *NBv = at<double>(ws, WS::B_C_NB), *NU = at<double>(ws, WS::B_C_NU), *NP = at<double>(ws, WS::B_C_NP);
    double *NX = at<double>(ws, WS::B_C_NX), *rhs = at<double>(ws, WS::B_C_RHS), *delta = at<double>(ws, WS::B_VX);
    cond_tri_solve_kernel<<<dim3(1), dim3(kSolveThreads), 0, stream>>>(at<double>(ws, WS::B_C_S), C->ld, at<double>(ws, WS::B_C_LDIAG), rhs);
    cond_scatter_kernel<<<dim3(blocks_for(C->n_junctions + C->n_nodes, 256)), dim3(256), 0, stream>>>(C->n_junctions, at<int>(ws, WS::B_C_JPOSE), C->n_nodes,
                                                                                                     node_kind, rhs, delta, NX);
    for (int l = C->n_levels - 1; l >= 0; --l) {
        const int e0 = C->level_ptr[(size_t)l], ne = C->level_ptr[(size_t)l + 1] - e0;
        cond_back_kernel<<<dim3(blocks_for(ne, kNodeBlock)), dim3(kNodeBlock), 0, stream>>>(elim + 3 * (size_t)e0, ne, node_kind, ND, NBv, NU, NP, NX, delta);
    }
    PGO_HIP(hipGetLastError());
    if (gr.timing) { PGO_HIP(hipEventRecord(ws->ev_c[4], stream)); C->pending = true; }
    return SCL_OK;
}

}  // namespace

const char *pgo_condensed_bad(const PgoInputs &in)
{
    int nj = 0, ns = 0, longest = 0;
    pgo_count_junctions(in.n_poses, in.f_i, in.f_j, in.n_factors, in.p_idx, in.n_priors, &nj, &ns, &longest);
    return nj > SCL_PGO_MAX_JUNCTIONS ? "more than 1024 junctions" : nullptr;
}

int pgo_solve_condensed(PgoWorkspace *ws, hipStream_t stream, const PgoInputs &in, double lambda, double *delta, bool timing, std::string *err)
{
    PgoGraph gr;
    Condensed C;
    int rc;
    if ((rc = pgo_setup(ws, stream, in, timing, &gr, err)) || (rc = prepare(ws, stream, in, timing, &C, err)) ||
        (rc = pgo_enqueue_linearise(ws, stream, gr, 0, false, err)))
        return rc;
    if (gr.timing) PGO_HIP(hipEventRecord(ws->ev[2], stream));
    if ((rc = enqueue_step(ws, stream, gr, &C, 0, lambda, err))) return rc;
    if (gr.timing) PGO_HIP(hipEventRecord(ws->ev[3], stream));
    const size_t nn = (size_t)gr.n;
    std::vector<double> out(6 * nn);
    PGO_HIP(hipMemcpyAsync(out.data(), ws->buf[WS::B_VX], sizeof(double) * 6 * nn, hipMemcpyDeviceToHost, stream));
    PgoRecord rec;
    if ((rc = pgo_read_record(ws, stream, &rec, err)) || (rc = pgo_add_timing(ws, &gr, true, true, err)) || (rc = collect(ws, &C, err))) return rc;
    if (rec.fail) {
        if (err) *err = "pgo_solve_condensed: a pivot not above 2^-43 of its diagonal entry";
        return SCL_ERR_NUMERIC;
    }
    std::memcpy(delta, out.data(), sizeof(double) * 6 * nn);
    return SCL_OK;
}

int pgo_condensed_factor(PgoWorkspace *ws, hipStream_t stream, const PgoInputs &in, double lambda, bool timing, PgoGraph *gr, PgoCondensed *C,
                         std::string *err)
{
    int rc;
    if ((rc = pgo_setup(ws, stream, in, timing, gr, err)) || (rc = prepare(ws, stream, in, timing, C, err)) ||
        (rc = pgo_enqueue_linearise(ws, stream, *gr, 0, false, err)))
        return rc;
    if (gr->timing) PGO_HIP(hipEventRecord(ws->ev[2], stream));
    return enqueue_factor(ws, stream, *gr, C, 0, lambda, err);
}

int pgo_condensed_finish(PgoWorkspace *ws, hipStream_t stream, PgoGraph *gr, PgoCondensed *C, std::string *err)
{
    if (gr->timing) {
        PGO_HIP(hipEventRecord(ws->ev_c[4], stream));
        PGO_HIP(hipEventRecord(ws->ev[3], stream));
        C->pending = true;
    }
    PGO_HIP(hipStreamSynchronize(stream));
    int rc;
    if ((rc = pgo_add_timing(ws, gr, true, true, err))) return rc;
    return collect(ws, C, err);
}

int pgo_optimize_condensed(PgoWorkspace *ws, hipStream_t stream, const PgoInputs &in, const scl_pgo_params &params, double *poses_out,
                           scl_pgo_result *result, double *chi2, int *failed_factorisations, bool timing, std::string *err)
{
    Condensed C;
    bool prepared = false;
    const PgoSolveFn direct = [&](PgoWorkspace *w, hipStream_t st, const PgoGraph &gr, int b, double lambda, std::string *e) -> int {
        int rc;
        if (!prepared) {                                   // behind pgo_lm's setup, once per call
            if ((rc = prepare(w, st, in, gr.timing, &C, e))) return rc;
            prepared = true;
        }
        std::string *err = e;
        if (gr.timing) PGO_HIP(hipEventRecord(w->ev[2], st));
        if ((rc = enqueue_step(w, st, gr, &C, b, lambda, e)) || (rc = pgo_enqueue_retract(w, st, gr, b, e))) return rc;
        if (gr.timing) PGO_HIP(hipEventRecord(w->ev[3], st));
        return (int)SCL_OK;
    };
    const int rc = pgo_lm(ws, stream, in, params, direct, true, poses_out, result, chi2, failed_factorisations, timing, err);
    if (rc) return rc;
    return collect(ws, &C, err);
}

}  // namespace scl
