// pgo_marginals.hip -- many right-hand sides on the factorisation the condensed direct step keeps, and the marginal covariances built on
// them (contract: include/scl_engine.h "POSE-GRAPH SOLVE, MANY RIGHT-HAND SIDES AND MARGINAL COVARIANCES").  The linearisation, the
// elimination and the blocked Cholesky of S are pgo_condensed.hip's launches (pgo_condensed_factor); what they leave -- L, P, Q of every
// eliminated node, the factor of S -- is read here and never written.  A column's arithmetic is one fixed sequence that depends on the
// graph and on the column alone: every kernel below gives a thread or a lane of an MFMA one column, and no result of a column reads
// another column's data.  Columns run in groups (pgo_marginal_plan.hpp).  All fp64, no atomics.
//
// Layouts.  A group's columns: X[column][6 n_poses], the right-hand sides on the way in, the solutions on the way out.  Node arrays:
// [column][node][6], so that the lanes of a wave read consecutive nodes of one column.  The junctions' dense right-hand sides: tiles of
// 16 columns, [tile][row < ld][16].
//
//   marg_setup_kernel     a thread per (node, column): b of an interior pose from X, zeros on a path's ends
//   marg_forward_kernel   one level, a thread per (eliminated node, column): w = L^-1 b_m, -P^T w into the node's left slot, -Q^T w into
//                         its right slot, w stays for the way back
//   marg_absorb_kernel    the level's survivors take left, then right (cond_absorb_kernel's order)
//   marg_rhs_kernel       the junctions' right-hand sides in cond_rhs_kernel's order, into the tiles; zero rows and columns pad them
//   marg_trsm_kernel      L Y = B, then L^T X = Y: a workgroup owns a tile of 16 columns through all panels of both sweeps
//   marg_scatter_kernel   x of the junctions into X; the paths' ends take theirs
//   marg_back_kernel      one level back: x_m = L^-T (w - P x_l - Q x_r)
//   marg_unit_kernel      the unit columns of the queried poses
//   marg_keep_kernel      the rows of the queried poses out of a group's solutions
//   marg_pick_kernel      a thread per query: Sigma_ij, h, Ad(h^-1), rel
#include "pgo.hpp"
#include "pgo_blocks.hpp"
#include "pgo_marginal_plan.hpp"

#include <cstring>
#include <vector>

namespace scl {

namespace {

using namespace pgo_blocks;

constexpr int kNodeBlock = 64;
constexpr int kNB = 32;            // the panel width of the factor of S (pgo_condensed.hip)
constexpr int kTrsmThreads = 512;  // 16 columns x 32 rows of a panel in the diagonal solve; 8 waves share the row tiles of the update
typedef double double4_t __attribute__((ext_vector_type(4)));
static_assert(kTrsmThreads == kMargTile * kNB, "a thread per (row of the panel, column of the tile)");

__global__ __launch_bounds__(256) void marg_setup_kernel(int n_nodes, const int *node_kind, size_t n6, const double *X, double *NBv)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const size_t c = blockIdx.y;
    if (i >= n_nodes) return;
    const int pose = node_kind[i];
    double *b = NBv + 6 * (c * (size_t)n_nodes + (size_t)i);
#pragma unroll
    for (int a = 0; a < 6; ++a) b[a] = pose >= 0 ? X[c * n6 + 6 * (size_t)pose + a] : 0.0;
}

__global__ __launch_bounds__(kNodeBlock) void marg_forward_kernel(const int *elim, int count, int n_nodes, const double *ND, const double *NU,
                                                                   const double *NP, double *NBv, double *NL, double *NR)
{
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= count) return;
    const int m = elim[3 * e];
    const size_t at = 6 * ((size_t)blockIdx.y * (size_t)n_nodes + (size_t)m);
    double L[21], w[6];
#pragma unroll
    for (int a = 0; a < 21; ++a) L[a] = ND[21 * (size_t)m + a];
#pragma unroll
    for (int a = 0; a < 6; ++a) w[a] = NBv[at + a];
    forward6(L, w);
    const double *PT = NP + 36 * (size_t)m, *Q = NU + 36 * (size_t)m;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double gl = 0.0, gr = 0.0;
#pragma unroll
        for (int a = 0; a < 6; ++a) { gl += PT[6 * c + a] * w[a]; gr += Q[6 * a + c] * w[a]; }
        NL[at + c] = -gl; NR[at + c] = -gr;
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) NBv[at + a] = w[a];
}

__global__ __launch_bounds__(256) void marg_absorb_kernel(const int *absorb, int count, int n_nodes, double *NBv, const double *NL, const double *NR)
{
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= count) return;
    const int s = absorb[3 * e], le = absorb[3 * e + 1], re = absorb[3 * e + 2];
    const size_t col = (size_t)blockIdx.y * (size_t)n_nodes;
    double *b = NBv + 6 * (col + (size_t)s);
    if (le >= 0) {                                         // the node eliminated on the left gave this one its right contribution
        const double *c = NR + 6 * (col + (size_t)le);
        for (int a = 0; a < 6; ++a) b[a] = b[a] + c[a];
    }
    if (re >= 0) {
        const double *c = NL + 6 * (col + (size_t)re);
        for (int a = 0; a < 6; ++a) b[a] = b[a] + c[a];
    }
}

// row i of column c (blockIdx.y, over whole tiles): the column's own entry at the junction's pose, then the ends' updates; the rows
// behind 6 n_junctions and the columns behind n_cols are zeros
__global__ __launch_bounds__(256) void marg_rhs_kernel(int n_rows, int ld, int n_cols, int n_nodes, size_t n6, const int *jpose, const int *rhs_ptr,
                                                        const int *rhs_src, const double *X, const double *NBv, double *tiles)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const size_t c = blockIdx.y;
    if (i >= ld) return;
    double v = 0.0;
    if (i < n_rows && c < (size_t)n_cols) {
        const int j = i / 6, a = i % 6;
        v = X[c * n6 + 6 * (size_t)jpose[j] + a];
        for (int s = rhs_ptr[j]; s < rhs_ptr[j + 1]; ++s) v = v + NBv[6 * (c * (size_t)n_nodes + (size_t)rhs_src[s]) + a];
    }
    tiles[((c / kMargTile) * (size_t)ld + (size_t)i) * kMargTile + c % kMargTile] = v;
}

// Y <- L^-T L^-1 Y for the tile blockIdx.x ([row < ld][16]) and the factor pgo_condensed.hip left (Ldiag: the diagonal blocks, S: the
// rest, row-major lower triangle).  Per panel of 32: thread (r, col) = (tid & 31, tid >> 5) solves the diagonal block against the tile's
// 32 x 16 -- column by column of the block, c ascending (descending in the transposed sweep), the pivot's value handed round within the
// 32 lanes that share a column of the tile --, then the eight waves share the 16-row tiles below (above) the panel:
// v_mfma_f64_16x16x4_f64 with A[row lane & 15][k = lane >> 4] from L's panel column, B[k = lane >> 4][col lane & 15] from the solved
// 32 x 16 in LDS, eight of them in ascending k, D[row (lane >> 4) + 4 v][col lane & 15].  Entry (row, col) of D is a sum over k of
// products with column col of B alone: no lane's result depends on another column, and a zero column stays out of its neighbours.
__global__ __launch_bounds__(kTrsmThreads) void marg_trsm_kernel(const double *S, int ld, const double *Ldiag, double *tiles)
{
    __shared__ double Xs[kNB][kMargTile + 1];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, T = ld / kNB;
    const int r = tid & (kNB - 1), col = tid >> 5, r16 = lane & 15, k4 = lane >> 4;
    const size_t LD = (size_t)ld;
    double *Y = tiles + (size_t)blockIdx.x * LD * kMargTile;
    for (int p = 0; p < T; ++p) {
        {
            double row[kNB];                               // row r of the diagonal block
#pragma unroll
            for (int k = 0; k < kNB; ++k) row[k] = Ldiag[(size_t)p * (kNB * kNB) + r * kNB + k];
            double *y = Y + ((size_t)p * kNB + r) * kMargTile + col;
            double x = *y;
#pragma unroll
            for (int c = 0; c < kNB; ++c) {
                const double v = __shfl(x / row[c], c, kNB);
                if (r > c) x -= row[c] * v;
                else if (r == c) x = v;
            }
            Xs[r][col] = x; *y = x;
        }
        __syncthreads();
        double b[8];
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) b[kk] = Xs[4 * kk + k4][r16];
        for (int t = 2 * (p + 1) + wave; t < 2 * T; t += kTrsmThreads / 64) {
            const double *Lr = S + ((size_t)16 * t + r16) * LD + (size_t)p * kNB + k4;
            double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Lr[4 * kk], b[kk], acc, 0, 0, 0);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                double *y = Y + ((size_t)16 * t + k4 + 4 * v) * kMargTile + r16;
                *y = *y - acc[v];
            }
        }
        __syncthreads();
    }
    for (int p = T - 1; p >= 0; --p) {
        {
            double cl[kNB];                                // column r of the diagonal block
#pragma unroll
            for (int k = 0; k < kNB; ++k) cl[k] = Ldiag[(size_t)p * (kNB * kNB) + k * kNB + r];
            double *y = Y + ((size_t)p * kNB + r) * kMargTile + col;
            double x = *y;
#pragma unroll
            for (int c = kNB - 1; c >= 0; --c) {
                const double v = __shfl(x / cl[c], c, kNB);
                if (r < c) x -= cl[c] * v;
                else if (r == c) x = v;
            }
            Xs[r][col] = x; *y = x;
        }
        __syncthreads();
        double b[8];
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) b[kk] = Xs[4 * kk + k4][r16];
        for (int t = wave; t < 2 * p; t += kTrsmThreads / 64) {
            // A = the transpose of L's rows of the panel: A[row][k] = L[32 p + k][16 t + row]
            const double *Lc = S + ((size_t)p * kNB + k4) * LD + (size_t)16 * t + r16;
            double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Lc[(size_t)(4 * kk) * LD], b[kk], acc, 0, 0, 0);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                double *y = Y + ((size_t)16 * t + k4 + 4 * v) * kMargTile + r16;
                *y = *y - acc[v];
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void marg_scatter_kernel(int n_junctions, const int *jpose, int n_nodes, const int *node_kind, int ld, size_t n6,
                                                            const double *tiles, double *X, double *NBv)
{
    int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const size_t c = blockIdx.y;
    const double *x = tiles + (c / kMargTile) * (size_t)ld * kMargTile + c % kMargTile;
    if (t < n_junctions) {
        for (int a = 0; a < 6; ++a) X[c * n6 + 6 * (size_t)jpose[t] + a] = x[(6 * (size_t)t + a) * kMargTile];
        return;
    }
    t -= n_junctions;
    if (t >= n_nodes || node_kind[t] >= 0) return;
    const int j = -1 - node_kind[t];
    for (int a = 0; a < 6; ++a) NBv[6 * (c * (size_t)n_nodes + (size_t)t) + a] = x[(6 * (size_t)j + a) * kMargTile];
}

__global__ __launch_bounds__(kNodeBlock) void marg_back_kernel(const int *elim, int count, int n_nodes, const int *node_kind, size_t n6, const double *ND,
                                                                const double *NU, const double *NP, double *NBv, double *X)
{
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= count) return;
    const int m = elim[3 * e], l = elim[3 * e + 1], r = elim[3 * e + 2];
    const size_t c = blockIdx.y, col = c * (size_t)n_nodes;
    double L[21], v[6], xl[6], xr[6];
#pragma unroll
    for (int a = 0; a < 21; ++a) L[a] = ND[21 * (size_t)m + a];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        v[a] = NBv[6 * (col + (size_t)m) + a]; xl[a] = NBv[6 * (col + (size_t)l) + a]; xr[a] = NBv[6 * (col + (size_t)r) + a];
    }
    const double *PT = NP + 36 * (size_t)m, *Q = NU + 36 * (size_t)m;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) s += PT[6 * k + a] * xl[k];
        v[a] = v[a] - s;
        s = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) s += Q[6 * a + k] * xr[k];
        v[a] = v[a] - s;
    }
    backward6(L, v);
    const int pose = node_kind[m];
#pragma unroll
    for (int a = 0; a < 6; ++a) { NBv[6 * (col + (size_t)m) + a] = v[a]; X[c * n6 + 6 * (size_t)pose + a] = v[a]; }
}

// column c of the group is unit column first + c of the queried poses: entry (first + c) % 6 of pose sel[(first + c) / 6]; X is zeros
__global__ __launch_bounds__(256) void marg_unit_kernel(int first, int n_cols, const int *sel, size_t n6, double *X)
{
    const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (c >= n_cols) return;
    const int u = first + c;
    X[(size_t)c * n6 + 6 * (size_t)sel[u / 6] + u % 6] = 1.0;
}

// kept[row 6 u + a][first + c] = x_c at entry a of pose sel[u]
__global__ __launch_bounds__(256) void marg_keep_kernel(int n_sel_rows, const int *sel, int first, int n_cols, int n_total, size_t n6, const double *X,
                                                         double *kept)
{
    const int row = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const size_t c = blockIdx.y;
    if (row >= n_sel_rows || c >= (size_t)n_cols) return;
    kept[(size_t)row * (size_t)n_total + (size_t)first + c] = X[c * n6 + 6 * (size_t)sel[row / 6] + row % 6];
}

// Query k: poses i, j at positions ui, uj of the selection.  Sigma_ij = the rows of i in the columns of j.  rel = Sigma_jj - A Sigma_ij -
// (A Sigma_ij)^T + A Sigma_ii A^T with A = Ad(h^-1), h^-1 = X_j^-1 X_i formed as the linearisation forms it; upper triangle, mirrored.
__global__ __launch_bounds__(64) void marg_pick_kernel(int n_queries, const int *query, int n_total, const double *kept, const double *poses,
                                                        double *blocks, double *rel)
{
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= n_queries) return;
    const int i = query[4 * k], j = query[4 * k + 1], ui = query[4 * k + 2], uj = query[4 * k + 3];
    const size_t NT = (size_t)n_total;
    if (blocks) {
        double *o = blocks + 36 * (size_t)k;
        for (int a = 0; a < 6; ++a)
            for (int b = 0; b < 6; ++b) {
                const int ra = (i == j && a > b) ? b : a, cb = (i == j && a > b) ? a : b;
                o[6 * a + b] = kept[(size_t)(6 * ui + ra) * NT + (size_t)(6 * uj + cb)];
            }
    }
    if (!rel) return;
    double *o = rel + 36 * (size_t)k;
    if (i == j) {
        for (int a = 0; a < 36; ++a) o[a] = 0.0;
        return;
    }
    double qh[4], th[3], R[9], B[9], A[36], Sij[36], Sii[36], Sjj[36], M[36], Tm[36];
    se3::relative_pose(poses + se3::kPoseStride * (size_t)j, poses + se3::kPoseStride * (size_t)i, qh, th);
    se3::adjoint_blocks(qh, th, R, B);
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            A[6 * a + b] = R[3 * a + b];       A[6 * a + 3 + b] = 0.0;
            A[6 * (3 + a) + b] = B[3 * a + b]; A[6 * (3 + a) + 3 + b] = R[3 * a + b];
        }
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) {
            const int lo = a < b ? a : b, hi = a < b ? b : a;
            Sij[6 * a + b] = kept[(size_t)(6 * ui + a) * NT + (size_t)(6 * uj + b)];
            Sii[6 * a + b] = kept[(size_t)(6 * ui + lo) * NT + (size_t)(6 * ui + hi)];
            Sjj[6 * a + b] = kept[(size_t)(6 * uj + lo) * NT + (size_t)(6 * uj + hi)];
        }
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) {
            double m = 0.0, t = 0.0;
            for (int c = 0; c < 6; ++c) { m += A[6 * a + c] * Sij[6 * c + b]; t += A[6 * a + c] * Sii[6 * c + b]; }
            M[6 * a + b] = m; Tm[6 * a + b] = t;
        }
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) {
            double n = 0.0;
            for (int c = 0; c < 6; ++c) n += Tm[6 * a + c] * A[6 * b + c];
            const double v = ((Sjj[6 * a + b] - M[6 * a + b]) - M[6 * b + a]) + n;
            o[6 * a + b] = v; o[6 * b + a] = v;
        }
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

inline unsigned blocks_for(int count, int block) { return (unsigned)((count > 0 ? count : 1) + block - 1) / (unsigned)block; }

// the buffers of a group of `group` columns
int ensure_group(WS *ws, const PgoCondensed &C, int n_poses, int group, std::string *err)
{
    const size_t g = (size_t)group, nodes = sizeof(double) * 6 * (size_t)(C.n_nodes > 0 ? C.n_nodes : 1) * g;
    const size_t n_tiles = (g + kMargTile - 1) / kMargTile;
    const struct { int k; size_t bytes; } need[] = {
        {WS::B_M_X, sizeof(double) * 6 * (size_t)n_poses * g}, {WS::B_M_NB, nodes}, {WS::B_M_NL, nodes}, {WS::B_M_NR, nodes},
        {WS::B_M_TILES, sizeof(double) * n_tiles * (size_t)C.ld * kMargTile}};
    for (const auto &b : need)
        if (const int rc = pgo_ensure(ws, b.k, b.bytes, err)) return rc;
    return SCL_OK;
}

// the n_cols columns in B_M_X solved in place: forward over the levels, the junctions' system, the way back
int enqueue_group(WS *ws, hipStream_t stream, const PgoCondensed &C, int n_poses, int n_cols, std::string *err)
{
    const int *node_kind = at<int>(ws, WS::B_C_NODE_POSE), *elim = at<int>(ws, WS::B_C_ELIM), *absorb = at<int>(ws, WS::B_C_ABSORB);
    const int *jpose = at<int>(ws, WS::B_C_JPOSE);
    const double *ND = at<double>(ws, WS::B_C_ND), *NU = at<double>(ws, WS::B_C_NU), *NP = at<double>(ws, WS::B_C_NP);
    double *X = at<double>(ws, WS::B_M_X), *NBv = at<double>(ws, WS::B_M_NB), *NL = at<double>(ws, WS::B_M_NL), *NR = at<double>(ws, WS::B_M_NR);
    double *tiles = at<double>(ws, WS::B_M_TILES);
    const size_t n6 = 6 * (size_t)n_poses;
    const unsigned cols = (unsigned)n_cols, n_tiles = (cols + kMargTile - 1) / kMargTile;
    if (C.n_nodes > 0)
        marg_setup_kernel<<<dim3(blocks_for(C.n_nodes, 256), cols), dim3(256), 0, stream>>>(C.n_nodes, node_kind, n6, X, NBv);
    for (int l = 0; l < C.n_levels; ++l) {
        const int e0 = C.level_ptr[(size_t)l], ne = C.level_ptr[(size_t)l + 1] - e0;
        const int a0 = C.absorb_ptr[(size_t)l], na = C.absorb_ptr[(size_t)l + 1] - a0;
        marg_forward_kernel<<<dim3(blocks_for(ne, kNodeBlock), cols), dim3(kNodeBlock), 0, stream>>>(elim + 3 * (size_t)e0, ne, C.n_nodes, ND, NU, NP, NBv, NL, NR);
        marg_absorb_kernel<<<dim3(blocks_for(na, 256), cols), dim3(256), 0, stream>>>(absorb + 3 * (size_t)a0, na, C.n_nodes, NBv, NL, NR);
    }
    marg_rhs_kernel<<<dim3(blocks_for(C.ld, 256), n_tiles * kMargTile), dim3(256), 0, stream>>>(
        C.n_rows, C.ld, n_cols, C.n_nodes, n6, jpose, at<int>(ws, WS::B_C_RHS_PTR), at<int>(ws, WS::B_C_RHS_SRC), X, NBv, tiles);
    marg_trsm_kernel<<<dim3(n_tiles), dim3(kTrsmThreads), 0, stream>>>(at<double>(ws, WS::B_C_S), C.ld, at<double>(ws, WS::B_C_LDIAG), tiles);
    marg_scatter_kernel<<<dim3(blocks_for(C.n_junctions + C.n_nodes, 256), cols), dim3(256), 0, stream>>>(C.n_junctions, jpose, C.n_nodes, node_kind, C.ld,
                                                                                                         n6, tiles, X, NBv);
    for (int l = C.n_levels - 1; l >= 0; --l) {
        const int e0 = C.level_ptr[(size_t)l], ne = C.level_ptr[(size_t)l + 1] - e0;
        marg_back_kernel<<<dim3(blocks_for(ne, kNodeBlock), cols), dim3(kNodeBlock), 0, stream>>>(elim + 3 * (size_t)e0, ne, C.n_nodes, node_kind, n6, ND, NU, NP,
                                                                                                  NBv, X);
    }
    PGO_HIP(hipGetLastError());
    return SCL_OK;
}

// the factorisation at lambda; SCL_ERR_NUMERIC where a pivot failed in it
int factor(WS *ws, hipStream_t stream, const PgoInputs &in, double lambda, bool timing, PgoGraph *gr, PgoCondensed *C, const char *name, std::string *err)
{
    int rc;
    PgoRecord rec;
    if ((rc = pgo_condensed_factor(ws, stream, in, lambda, timing, gr, C, err)) || (rc = pgo_read_record(ws, stream, &rec, err))) return rc;
    if (rec.fail) {
        if ((rc = pgo_condensed_finish(ws, stream, gr, C, err))) return rc;
        if (err) *err = std::string(name) + ": a pivot not above 2^-43 of its diagonal entry";
        return SCL_ERR_NUMERIC;
    }
    return SCL_OK;
}

}  // namespace

int pgo_solve_condensed_many(PgoWorkspace *ws, hipStream_t stream, const PgoInputs &in, double lambda, const double *rhs, int n_rhs, double *x,
                             bool timing, std::string *err)
{
    PgoGraph gr;
    PgoCondensed C;
    int rc;
    if ((rc = factor(ws, stream, in, lambda, timing, &gr, &C, "pgo_solve_condensed_many", err))) return rc;
    const int group = std::min(pgo_marginal_group_columns(in.n_poses, C.n_nodes), n_rhs);
    if ((rc = ensure_group(ws, C, in.n_poses, group, err))) return rc;
    const size_t n6 = 6 * (size_t)in.n_poses;
    for (int g = 0;; ++g) {
        int first, count;
        pgo_marginal_group(n_rhs, group, g, &first, &count);
        if (count <= 0) break;
        const size_t bytes = sizeof(double) * n6 * (size_t)count;
        PGO_HIP(hipMemcpyAsync(ws->buf[WS::B_M_X], rhs + n6 * (size_t)first, bytes, hipMemcpyHostToDevice, stream));
        PGO_HIP(hipStreamSynchronize(stream));             // the caller's array is pageable, and x may be it
        if ((rc = enqueue_group(ws, stream, C, in.n_poses, count, err))) return rc;
        PGO_HIP(hipMemcpyAsync(x + n6 * (size_t)first, ws->buf[WS::B_M_X], bytes, hipMemcpyDeviceToHost, stream));
        PGO_HIP(hipStreamSynchronize(stream));
    }
    return pgo_condensed_finish(ws, stream, &gr, &C, err);
}

int pgo_marginals(PgoWorkspace *ws, hipStream_t stream, const PgoInputs &in, const int *q_i, const int *q_j, int n_queries, double *blocks,
                  double *rel, bool timing, std::string *err)
{
    std::vector<int> sel, ui, uj;
    if (const char *bad = pgo_marginal_select(q_i, q_j, n_queries, in.n_poses, &sel, &ui, &uj)) {
        if (err) *err = std::string("pgo_marginals: ") + bad;
        return SCL_ERR_INVALID_ARG;
    }
    PgoGraph gr;
    PgoCondensed C;
    int rc;
    if ((rc = factor(ws, stream, in, 0.0, timing, &gr, &C, "pgo_marginals", err))) return rc;
    const int n_total = 6 * (int)sel.size();
    const int group = std::min(pgo_marginal_group_columns(in.n_poses, C.n_nodes), n_total);
    const size_t nq = (size_t)n_queries, out_bytes = sizeof(double) * 36 * nq;
    std::vector<int> query(4 * nq);
    for (size_t k = 0; k < nq; ++k) { query[4 * k] = q_i[k]; query[4 * k + 1] = q_j[k]; query[4 * k + 2] = ui[k]; query[4 * k + 3] = uj[k]; }
    if ((rc = ensure_group(ws, C, in.n_poses, group, err)) || (rc = pgo_ensure(ws, WS::B_M_SEL, sizeof(int) * sel.size(), err)) ||
        (rc = pgo_ensure(ws, WS::B_M_QUERY, sizeof(int) * query.size(), err)) ||
        (rc = pgo_ensure(ws, WS::B_M_KEPT, sizeof(double) * (size_t)n_total * (size_t)n_total, err)) ||
        (rc = pgo_ensure(ws, WS::B_M_BLOCKS, out_bytes, err)) || (rc = pgo_ensure(ws, WS::B_M_REL, out_bytes, err)))
        return rc;
    PGO_HIP(hipMemcpyAsync(ws->buf[WS::B_M_SEL], sel.data(), sizeof(int) * sel.size(), hipMemcpyHostToDevice, stream));
    PGO_HIP(hipMemcpyAsync(ws->buf[WS::B_M_QUERY], query.data(), sizeof(int) * query.size(), hipMemcpyHostToDevice, stream));
    PGO_HIP(hipStreamSynchronize(stream));                 // the two vectors are pageable
    const size_t n6 = 6 * (size_t)in.n_poses;
    for (int g = 0;; ++g) {
        int first, count;
        pgo_marginal_group(n_total, group, g, &first, &count);
        if (count <= 0) break;
        PGO_HIP(hipMemsetAsync(ws->buf[WS::B_M_X], 0, sizeof(double) * n6 * (size_t)count, stream));
        marg_unit_kernel<<<dim3(blocks_for(count, 256)), dim3(256), 0, stream>>>(first, count, at<int>(ws, WS::B_M_SEL), n6, at<double>(ws, WS::B_M_X));
        if ((rc = enqueue_group(ws, stream, C, in.n_poses, count, err))) return rc;
        marg_keep_kernel<<<dim3(blocks_for(n_total, 256), (unsigned)count), dim3(256), 0, stream>>>(n_total, at<int>(ws, WS::B_M_SEL), first, count, n_total, n6,
                                                                                                   at<double>(ws, WS::B_M_X), at<double>(ws, WS::B_M_KEPT));
    }
    marg_pick_kernel<<<dim3(blocks_for(n_queries, 64)), dim3(64), 0, stream>>>(n_queries, at<int>(ws, WS::B_M_QUERY), n_total, at<double>(ws, WS::B_M_KEPT),
                                                                                at<double>(ws, WS::B_X0), blocks ? at<double>(ws, WS::B_M_BLOCKS) : nullptr,
                                                                                rel ? at<double>(ws, WS::B_M_REL) : nullptr);
    PGO_HIP(hipGetLastError());
    std::vector<double> ob(blocks ? 36 * nq : 0), orl(rel ? 36 * nq : 0);
    if (blocks) PGO_HIP(hipMemcpyAsync(ob.data(), ws->buf[WS::B_M_BLOCKS], out_bytes, hipMemcpyDeviceToHost, stream));
    if (rel) PGO_HIP(hipMemcpyAsync(orl.data(), ws->buf[WS::B_M_REL], out_bytes, hipMemcpyDeviceToHost, stream));
    if ((rc = pgo_condensed_finish(ws, stream, &gr, &C, err))) return rc;
    if (blocks) std::memcpy(blocks, ob.data(), out_bytes);
    if (rel) std::memcpy(rel, orl.data(), out_bytes);
    return SCL_OK;
}

}  // namespace scl
