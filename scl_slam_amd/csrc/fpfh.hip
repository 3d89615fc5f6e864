// fpfh.hip -- the FPFH descriptor on the GPU (include/scl_fpfh.h; reference fpfh_descriptor, include/descriptor.h:253-460).
// Numerics contract: DESIGN.md section 4 "FPFH".  Per launch group of up to 16 scans (copied in once, resident until the
// descriptors are in the database):
//
//   fpfh_grid_kernel     one workgroup per scan: bounding box (float min / max), non-finite flag, and the cell size h of a uniform
//                        grid with at most 2 N cells (the smallest h by bisection: an outlier coarsens the grid, never overflows it);
//   fpfh_key_kernel      every point's cell (fp64: floor((x - min) / h)) as the sort key, the point as a float4 in input order;
//   sort_pairs_u64_segmented (device_sort.hip): the points of every scan ordered by cell;
//   fpfh_cells_kernel    cell starts from the sorted keys (empty cells included), the points gathered in cell order;
//   fpfh_knn_kernel      one lane per point, points taken in cell order: the 10 smallest (d2, index) keys in registers, shells of
//                        cells searched outward until the 10th d2 is below a conservative bound on every unvisited cell; then the
//                        normal in the same lane (fp64 scatter in (d2, index) order, jacobi3, PCL's float flip), written in input order;
//   fpfh_spfh_kernel     the N - 2 pairs (last point, j): PCL's pair features in float, three bins, counted per wave by ballots
//                        and popcounts, one global atomic per bin per workgroup;
//   fpfh_finish_kernel   counts -> the floats of PCL's sequential `+=` (fpfh_values.hpp), straight into the database slot.
// The database, the keyframe registry, make_and_save_many and the 1-NN detection (nn_l2_kernel<33>): plugin_host.hpp.
#include "scl_fpfh.h"

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
#include "device_sort.hpp"
#include "fpfh_values.hpp"
#include "plugin_host.hpp"

using namespace scl;

namespace {

constexpr int kGroup = SCL_FPFH_MAX_GROUP;
constexpr int kK = SCL_FPFH_K;
constexpr int kDim = SCL_FPFH_DIM;
constexpr int kCounts = 34;                 // 33 bins + skipped pairs
constexpr int kThreads = 256;
constexpr int kGridThreads = 1024;
constexpr int kSpfhBlocks = 32;             // workgroups per scan of the pair kernel
constexpr int kCellsPerPoint = 2;           // grid budget

struct FpScan {
    unsigned long long byte_off;            // first byte of the scan in the group's point buffer
    int n;
    int slot;                               // database row that receives the descriptor
    int pt_off;                             // first element of the scan in the group's per-point arrays
    int cell_off;                           // first cell start of the scan
    int cell_cap;                           // cells the grid may use (the start array has cell_cap + 1 entries)
    int pad;
};

struct FpGrid {
    double ox, oy, oz, h;
    int dx, dy, dz, cells;
};

__device__ __forceinline__ const float *point_at(const unsigned char *pts, const FpScan &sc, int stride, int i)
{
    return reinterpret_cast<const float *>(pts + sc.byte_off + (unsigned long long)i * (unsigned long long)stride);
}

__device__ __forceinline__ double grid_cells(double ex, double ey, double ez, double h)
{
    return (floor(ex / h) + 1.0) * (floor(ey / h) + 1.0) * (floor(ez / h) + 1.0);
}

__global__ __launch_bounds__(kGridThreads) void fpfh_grid_kernel(const unsigned char *pts, const FpScan *scans, int stride, FpGrid *grids,
                                                                 int *bad)
{
    __shared__ float red[6][kGridThreads / 64];
    __shared__ int nonfinite;
    const FpScan sc = scans[blockIdx.x];
    const int t = threadIdx.x;
    if (t == 0) nonfinite = 0;
    __syncthreads();
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    bool nf = false;
    for (int i = t; i < sc.n; i += kGridThreads) {
        const float *p = point_at(pts, sc, stride, i);
        const float x = p[0], y = p[1], z = p[2];
        nf |= !(isfinite(x) && isfinite(y) && isfinite(z));
        mn[0] = fminf(mn[0], x); mn[1] = fminf(mn[1], y); mn[2] = fminf(mn[2], z);
        mx[0] = fmaxf(mx[0], x); mx[1] = fmaxf(mx[1], y); mx[2] = fmaxf(mx[2], z);
    }
    if (nf) atomicOr(&nonfinite, 1);
    for (int off = 32; off > 0; off >>= 1)
        for (int a = 0; a < 3; ++a) { mn[a] = fminf(mn[a], __shfl_xor(mn[a], off)); mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], off)); }
    if ((t & 63) == 0)
        for (int a = 0; a < 3; ++a) { red[a][t >> 6] = mn[a]; red[3 + a][t >> 6] = mx[a]; }
    __syncthreads();
    if (t != 0) return;
    for (int w = 1; w < kGridThreads / 64; ++w)
        for (int a = 0; a < 3; ++a) { red[a][0] = fminf(red[a][0], red[a][w]); red[3 + a][0] = fmaxf(red[3 + a][0], red[3 + a][w]); }
    if (nonfinite) bad[blockIdx.x] = 1;
    FpGrid g;
    g.ox = (double)red[0][0]; g.oy = (double)red[1][0]; g.oz = (double)red[2][0];
    const double ex = nonfinite ? 0.0 : (double)red[3][0] - g.ox, ey = nonfinite ? 0.0 : (double)red[4][0] - g.oy,
                 ez = nonfinite ? 0.0 : (double)red[5][0] - g.oz;
    const double emax = fmax(ex, fmax(ey, ez));
    double h = 1.0;
    if (emax > 0.0) {                                             // the smallest h (to 2^-60 relative) with at most cell_cap cells
        double lo = 0.0, hi = emax * 2.0;
        for (int it = 0; it < 80; ++it) {
            const double mid = 0.5 * (lo + hi);
            if (mid <= lo || mid >= hi) break;
            if (grid_cells(ex, ey, ez, mid) <= (double)sc.cell_cap) hi = mid;
            else lo = mid;
        }
        h = hi;
    }
    g.h = h;
    g.dx = (int)floor(ex / h) + 1; g.dy = (int)floor(ey / h) + 1; g.dz = (int)floor(ez / h) + 1;
    g.cells = g.dx * g.dy * g.dz;
    grids[blockIdx.x] = g;
}

__device__ __forceinline__ int cell_coord(float x, double o, double h, int d)
{
    const int c = (int)floor(((double)x - o) / h);
    return c < 0 ? 0 : (c >= d ? d - 1 : c);
}

__global__ __launch_bounds__(kThreads) void fpfh_key_kernel(const unsigned char *pts, const FpScan *scans, int stride, const FpGrid *grids,
                                                            const int *bad, unsigned long long *keys, unsigned int *vals, float4 *pos)
{
    const FpScan sc = scans[blockIdx.y];
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= sc.n) return;
    const FpGrid g = grids[blockIdx.y];
    const float *p = point_at(pts, sc, stride, i);
    const float x = p[0], y = p[1], z = p[2];
    unsigned long long key = 0;
    if (!bad[blockIdx.y]) {
        const int cx = cell_coord(x, g.ox, g.h, g.dx), cy = cell_coord(y, g.oy, g.h, g.dy), cz = cell_coord(z, g.oz, g.h, g.dz);
        key = ((unsigned long long)cz * (unsigned long long)g.dy + (unsigned long long)cy) * (unsigned long long)g.dx + (unsigned long long)cx;
    }
    keys[sc.pt_off + i] = key;
    vals[sc.pt_off + i] = (unsigned int)i;
    pos[sc.pt_off + i] = make_float4(x, y, z, 0.0f);
}

__global__ __launch_bounds__(kThreads) void fpfh_cells_kernel(const FpScan *scans, const FpGrid *grids, const unsigned long long *keys,
                                                              const unsigned int *vals, const float4 *pos, int *starts, float4 *sp)
{
    const FpScan sc = scans[blockIdx.y];
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= sc.n) return;
    const int cells = grids[blockIdx.y].cells;
    int *st = starts + sc.cell_off;
    const long long k = (long long)keys[sc.pt_off + i];
    const long long prev = i > 0 ? (long long)keys[sc.pt_off + i - 1] : -1;
    for (long long c = prev + 1; c <= k; ++c) st[c] = i;
    if (i == sc.n - 1)
        for (long long c = k + 1; c <= cells; ++c) st[c] = sc.n;
    const unsigned int o = vals[sc.pt_off + i];
    float4 p = pos[sc.pt_off + o];
    p.w = __uint_as_float(o);
    sp[sc.pt_off + i] = p;
}

// insert (d2 bits, index) into the ascending top-K in registers (unrolled: static indices only)
__device__ __forceinline__ void topk_insert(unsigned long long (&best)[kK], unsigned long long key)
{
    if (key >= best[kK - 1]) return;
    best[kK - 1] = key;
#pragma unroll
    for (int j = kK - 1; j > 0; --j) {
        const unsigned long long a = best[j - 1], b = best[j];
        const bool sw = b < a;
        best[j - 1] = sw ? b : a; best[j] = sw ? a : b;
    }
}

__global__ __launch_bounds__(kThreads) void fpfh_knn_kernel(const FpScan *scans, const FpGrid *grids, const int *starts, const float4 *sp,
                                                            const float4 *pos, const int *bad, float4 *normals, int *nbr_idx, float *nbr_d2,
                                                            unsigned long long *candidates)
{
    const FpScan sc = scans[blockIdx.y];
    const int i = blockIdx.x * kThreads + threadIdx.x;
    unsigned long long evals = 0;
    if (i < sc.n && !bad[blockIdx.y]) {
        const FpGrid g = grids[blockIdx.y];
        const int *st = starts + sc.cell_off;
        const float4 *cp = sp + sc.pt_off;
        const float4 q = cp[i];
        const int k = sc.n < kK ? sc.n : kK;
        const int cx = cell_coord(q.x, g.ox, g.h, g.dx), cy = cell_coord(q.y, g.oy, g.h, g.dy), cz = cell_coord(q.z, g.oz, g.h, g.dz);
        const int rmax = max(max(max(cx, g.dx - 1 - cx), max(cy, g.dy - 1 - cy)), max(cz, g.dz - 1 - cz));
        unsigned long long best[kK];
#pragma unroll
        for (int j = 0; j < kK; ++j) best[j] = ~0ull;
        for (int r = 0;; ++r) {
            const int z0 = max(cz - r, 0), z1 = min(cz + r, g.dz - 1), y0 = max(cy - r, 0), y1 = min(cy + r, g.dy - 1);
            for (int z = z0; z <= z1; ++z)
                for (int y = y0; y <= y1; ++y) {
                    const bool face = (z == cz - r) || (z == cz + r) || (y == cy - r) || (y == cy + r);
                    // a face row: every cell of [cx - r, cx + r]; an inner row: only its two ends
                    for (int side = 0; side < (face ? 1 : 2); ++side) {
                        int x0, x1;
                        if (face) { x0 = max(cx - r, 0); x1 = min(cx + r, g.dx - 1); }
                        else { x0 = x1 = side == 0 ? cx - r : cx + r; if (x0 < 0 || x0 >= g.dx) continue; }
                        const int row = (z * g.dy + y) * g.dx;
                        const int a = st[row + x0], b = st[row + x1 + 1];
                        evals += (unsigned long long)(b - a);
                        for (int j = a; j < b; ++j) {
                            const float4 c = cp[j];
                            const float dx = c.x - q.x, dy = c.y - q.y, dz = c.z - q.z;
                            const float d2 = (dx * dx + dy * dy) + dz * dz;
                            topk_insert(best, ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)__float_as_uint(c.w));
                        }
                    }
                }
            if (r >= rmax) break;
            // every unvisited point lies in a cell >= r + 1 cells away along some axis: its distance is >= (r - 0.001) h (the cell
            // coordinates are fp64 and off by far less than 1e-3 cell); its float d2 >= (1 - 1e-6) of the true square
            if (r >= 1) {
                unsigned long long kth = best[0];
#pragma unroll
                for (int j = 1; j < kK; ++j) kth = j == k - 1 ? best[j] : kth;
                if (kth != ~0ull) {
                    const double bnd = ((double)r - 0.001) * g.h;
                    if ((double)__uint_as_float((unsigned int)(kth >> 32)) < bnd * bnd * (1.0 - 1e-5) - 1e-36) break;
                }
            }
        }
        const int orig = (int)__float_as_uint(q.w);
        const float4 *ip = pos + sc.pt_off;
        // the normal: fp64 mean and scatter in (d2, index) order, Jacobi, the smallest eigenvalue's column (ties: lowest)
        double sx = 0.0, sy = 0.0, sz = 0.0;
#pragma unroll
        for (int j = 0; j < kK; ++j)
            if (j < k) { const float4 p = ip[(unsigned int)best[j]]; sx += (double)p.x; sy += (double)p.y; sz += (double)p.z; }
        const double mx = sx / (double)k, my = sy / (double)k, mz = sz / (double)k;
        double c00 = 0, c01 = 0, c02 = 0, c11 = 0, c12 = 0, c22 = 0;
#pragma unroll
        for (int j = 0; j < kK; ++j)
            if (j < k) {
                const float4 p = ip[(unsigned int)best[j]];
                const double dx = (double)p.x - mx, dy = (double)p.y - my, dz = (double)p.z - mz;
                c00 += dx * dx; c01 += dx * dy; c02 += dx * dz; c11 += dy * dy; c12 += dy * dz; c22 += dz * dz;
            }
        double a[3][3] = {{c00, c01, c02}, {c01, c11, c12}, {c02, c12, c22}}, v[3][3];
        jacobi3(a, v);
        int m = 0;
        if (a[1][1] < a[m][m]) m = 1;
        if (a[2][2] < a[m][m]) m = 2;
        float nx = (float)v[0][m], ny = (float)v[1][m], nz = (float)v[2][m];
        const float vx = 0.0f - q.x, vy = 0.0f - q.y, vz = 0.0f - q.z;
        if ((vx * nx + vy * ny) + vz * nz < 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
        normals[sc.pt_off + orig] = make_float4(nx, ny, nz, 0.0f);
        if (nbr_idx) {
#pragma unroll
            for (int j = 0; j < kK; ++j)
                if (j < k) {
                    nbr_idx[(size_t)orig * k + j] = (int)(unsigned int)best[j];
                    nbr_d2[(size_t)orig * k + j] = __uint_as_float((unsigned int)(best[j] >> 32));
                }
        }
    }
    for (int off = 32; off > 0; off >>= 1) evals += __shfl_xor(evals, off);
    if ((threadIdx.x & 63) == 0 && evals) atomicAdd(candidates, evals);
}

// Eigen's Vector4f dot with lane 3 = +0: (a0*b0 + a2*b2) + (a1*b1 + 0)
__device__ __forceinline__ float dot4(float a0, float a1, float a2, float b0, float b1, float b2)
{
    return (a0 * b0 + a2 * b2) + (a1 * b1 + 0.0f);
}

__device__ __forceinline__ int clamp_bin(double t)
{
    if (t != t) return 0;
    const double fl = floor(t);
    return fl < 0.0 ? 0 : (fl >= 11.0 ? 10 : (int)fl);
}

// PCL's computePairFeatures(p_last, n_last, p_j, n_j) and the three bins; false when the pair is skipped
__device__ __forceinline__ bool pair_bins(float4 p1, float4 n1, float4 p2, float4 n2, int &b1, int &b2, int &b3)
{
    float d0 = p2.x - p1.x, d1 = p2.y - p1.y, d2 = p2.z - p1.z;
    const float f4 = sqrtf(dot4(d0, d1, d2, d0, d1, d2));
    if (f4 == 0.0f) return false;
    const float a1 = dot4(n1.x, n1.y, n1.z, d0, d1, d2) / f4, a2 = dot4(n2.x, n2.y, n2.z, d0, d1, d2) / f4;
    const bool sw = acosf_glibc(fabsf(a1)) > acosf_glibc(fabsf(a2));
    const float u0 = sw ? n2.x : n1.x, u1 = sw ? n2.y : n1.y, u2 = sw ? n2.z : n1.z;
    const float m0 = sw ? n1.x : n2.x, m1 = sw ? n1.y : n2.y, m2 = sw ? n1.z : n2.z;
    if (sw) { d0 = -d0; d1 = -d1; d2 = -d2; }
    const float f3 = sw ? -a2 : a1;
    float v0 = d1 * u2 - d2 * u1, v1 = d2 * u0 - d0 * u2, v2 = d0 * u1 - d1 * u0;
    const float vn = sqrtf(dot4(v0, v1, v2, v0, v1, v2));
    if (vn == 0.0f) return false;
    v0 = v0 / vn; v1 = v1 / vn; v2 = v2 / vn;
    const float w0 = u1 * v2 - u2 * v1, w1 = u2 * v0 - u0 * v2, w2 = u0 * v1 - u1 * v0;
    const float f2 = dot4(v0, v1, v2, m0, m1, m2);
    const float f1 = iris_atan2f(dot4(w0, w1, w2, m0, m1, m2), dot4(u0, u1, u2, m0, m1, m2));
    const float d_pi = 1.0f / (2.0f * 3.14159265358979323846f);
    b1 = clamp_bin(11.0 * (((double)f1 + 3.14159265358979323846) * (double)d_pi));
    b2 = clamp_bin(11.0 * (((double)f2 + 1.0) * 0.5));
    b3 = clamp_bin(11.0 * (((double)f3 + 1.0) * 0.5));
    return true;
}

__global__ __launch_bounds__(kThreads) void fpfh_spfh_kernel(const FpScan *scans, const float4 *pos, const float4 *normals, const int *bad,
                                                             unsigned int *counts)
{
    __shared__ unsigned int cs[kCounts];
    const FpScan sc = scans[blockIdx.y];
    const int t = threadIdx.x, lane = t & 63;
    if (t < kCounts) cs[t] = 0u;
    __syncthreads();
    if (bad[blockIdx.y]) return;
    const int pairs = sc.n - 1;                                       // j = 0 .. n - 2
    const float4 pl = pos[sc.pt_off + sc.n - 1], nl = normals[sc.pt_off + sc.n - 1];
    unsigned int c[kCounts];
#pragma unroll
    for (int b = 0; b < kCounts; ++b) c[b] = 0u;
    const int wave = blockIdx.x * (kThreads / 64) + (t >> 6), waves = gridDim.x * (kThreads / 64);
    for (int base = wave * 64; base < pairs; base += waves * 64) {  // wave-uniform trip count: the ballots see converged waves
        const int j = base + lane;
        int b1 = -1, b2 = -1, b3 = -1;
        bool skip = false;
        if (j < pairs) skip = !pair_bins(pl, nl, pos[sc.pt_off + j], normals[sc.pt_off + j], b1, b2, b3);
#pragma unroll
        for (int b = 0; b < SCL_FPFH_BINS; ++b) {
            c[b] += (unsigned int)__popcll(__ballot(b1 == b));
            c[SCL_FPFH_BINS + b] += (unsigned int)__popcll(__ballot(b2 == b));
            c[2 * SCL_FPFH_BINS + b] += (unsigned int)__popcll(__ballot(b3 == b));
        }
        c[kCounts - 1] += (unsigned int)__popcll(__ballot(skip));
    }
    if (lane == 0)
#pragma unroll
        for (int b = 0; b < kCounts; ++b)
            if (c[b]) atomicAdd(&cs[b], c[b]);
    __syncthreads();
    if (t < kCounts && cs[t]) atomicAdd(&counts[(size_t)blockIdx.y * kCounts + t], cs[t]);
}

__global__ __launch_bounds__(64) void fpfh_finish_kernel(const FpScan *scans, const int *bad, const unsigned int *counts, float *db)
{
    const FpScan sc = scans[blockIdx.x];
    const int t = threadIdx.x;
    if (t >= kDim || bad[blockIdx.x]) return;
    const float inc = 100.0f / (float)(long long)(sc.n - 2);         // hist_incr = 100.0f / (float)(indices.size() - 1)
    db[(size_t)sc.slot * kDim + t] = scl::fpfh_value(counts[(size_t)blockIdx.x * kCounts + t], inc);
}

__device__ __forceinline__ unsigned long long mix64(unsigned long long z)
{
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// 2^24 inputs per block index: 4096 workgroups x 256 lanes x 16 consecutive bit patterns
__global__ __launch_bounds__(kThreads) void fpfh_acosf_blocks_kernel(int first_block, unsigned long long *sums)
{
    const unsigned int blk = (unsigned int)(first_block + (int)blockIdx.y);
    const unsigned int base = (blk << 24) | ((blockIdx.x * kThreads + threadIdx.x) * 16u);
    unsigned long long h = 0;
    for (unsigned int i = 0; i < 16; ++i) {
        const unsigned int bits = base + i;
        const float r = acosf_glibc(__uint_as_float(bits));
        const unsigned int ur = r != r ? 0x7fc00000u : __float_as_uint(r);
        h += mix64(((unsigned long long)bits << 32) | ur);
    }
    for (int off = 32; off > 0; off >>= 1) h += __shfl_xor(h, off);
    if ((threadIdx.x & 63) == 0) atomicAdd(&sums[blockIdx.y], h);
}

}  // namespace

struct __attribute__((visibility("hidden"))) scl_fpfh : scl::VectorPlugin<kDim> {
    static constexpr int kGroup = ::kGroup;
    scl_fpfh_config cfg;
    // the launch group's workspace (per point, per cell, per scan)
    unsigned char *d_pts = nullptr; size_t pts_cap = 0;
    size_t pt_cap = 0, cell_cap = 0, sort_cap = 0;
    float4 *d_pos = nullptr, *d_sp = nullptr, *d_normals = nullptr;
    unsigned long long *d_keys0 = nullptr, *d_keys1 = nullptr;
    unsigned int *d_vals0 = nullptr, *d_vals1 = nullptr;
    void *d_sort = nullptr;
    int *d_starts = nullptr;
    FpScan *d_scans = nullptr;
    FpGrid *d_grids = nullptr;
    int *d_bad = nullptr;
    unsigned int *d_counts = nullptr;
    unsigned long long *d_cand = nullptr;
    int *d_nbr = nullptr; float *d_nbr_d2 = nullptr; size_t nbr_cap = 0;
    unsigned long long points = 0;

    int report_dims() const { return cfg.report_dims; }
    bool inter_snapshot() const { return cfg.inter_mode == 0; }
    int snapshot_period() const { return cfg.tree_making_period; }
    int reported_distance(int a, int b, float d2, float *dist);
    static int check_layout(scl_fpfh *h, const void *points, int n_points, int stride);
    static int run_group_locked(scl_fpfh *h, const void *const *clouds, const int *n_points, int stride, int G, int slot0, int *any_bad,
                                bool want_nbr = false);
};

int scl_fpfh::check_layout(scl_fpfh *h, const void *points, int n_points, int stride)
{
    if (stride < 12 || (stride & 3)) return fail(h, SCL_ERR_INVALID_ARG, "bad point layout (stride_bytes >= 12, multiple of 4)");
    if (n_points < 3) return fail(h, SCL_ERR_INVALID_ARG, "FPFH needs at least 3 points (N - 2 pairs)");
    if (n_points > (1 << 28)) return fail(h, SCL_ERR_INVALID_ARG, "FPFH: more than 2^28 points in one cloud");
    if (!points) return fail(h, SCL_ERR_INVALID_ARG, "null point pointer");
    return SCL_OK;
}

// the workspace for a group of `pts` points, `cells` cell starts and `bytes` bytes of input
static int reserve(scl_fpfh *h, size_t pts, size_t cells, size_t bytes)
{
    int rc;
    if (bytes > h->pts_cap) {
        const size_t c = bytes + bytes / 4 + 4096;
        if ((rc = dev_regrow(h, &h->d_pts, c))) return rc;
        h->pts_cap = c;
    }
    if (pts > h->pt_cap) {
        const size_t c = pts + pts / 4 + 1024;
        if ((rc = dev_regrow(h, &h->d_pos, c)) || (rc = dev_regrow(h, &h->d_sp, c)) || (rc = dev_regrow(h, &h->d_normals, c)) ||
            (rc = dev_regrow(h, &h->d_keys0, c)) || (rc = dev_regrow(h, &h->d_keys1, c)) || (rc = dev_regrow(h, &h->d_vals0, c)) ||
            (rc = dev_regrow(h, &h->d_vals1, c)))
            return rc;
        h->pt_cap = c;
    }
    const size_t sb = scl::sort_scratch_bytes(h->pt_cap, kGroup);
    if (sb > h->sort_cap) {
        unsigned char *p = nullptr;
        if ((rc = dev_alloc(h, &p, sb))) return rc;
        if (h->d_sort) (void)hipFree(h->d_sort);
        h->d_sort = p; h->sort_cap = sb;
    }
    if (cells > h->cell_cap) {
        const size_t c = cells + cells / 4 + 1024;
        if ((rc = dev_regrow(h, &h->d_starts, c))) return rc;
        h->cell_cap = c;
    }
    return SCL_OK;
}

// One launch group (G <= 16 clouds): descriptors into database rows slot0 .. slot0 + G - 1 (capacity ensured by the caller).
// *any_bad = 1 if a cloud has a non-finite coordinate.  want_nbr: the neighbour hook (G == 1, d_nbr / d_nbr_d2 sized by the caller).
int scl_fpfh::run_group_locked(scl_fpfh *h, const void *const *clouds, const int *n_points, int stride, int G, int slot0, int *any_bad,
                                bool want_nbr)
{
    FpScan scans[kGroup];
    unsigned long long bytes = 0;
    size_t pts = 0, cells = 0;
    int max_n = 0, max_cap = 1;
    scl::SortSegments seg{};
    seg.nseg = G;
    for (int g = 0; g < G; ++g) {
        scans[g].byte_off = bytes; scans[g].n = n_points[g]; scans[g].slot = slot0 + g;
        scans[g].pt_off = (int)pts; scans[g].cell_off = (int)cells; scans[g].cell_cap = kCellsPerPoint * n_points[g]; scans[g].pad = 0;
        seg.off[g] = (int)pts;
        bytes += (unsigned long long)n_points[g] * (unsigned long long)stride;
        pts += (size_t)n_points[g];
        cells += (size_t)scans[g].cell_cap + 1;
        max_n = std::max(max_n, n_points[g]); max_cap = std::max(max_cap, scans[g].cell_cap);
    }
    seg.off[G] = (int)pts;
    if (pts > (size_t)1 << 30 || cells > (size_t)1 << 31) return fail(h, SCL_ERR_INVALID_ARG, "FPFH: launch group too large");
    int rc = reserve(h, pts, cells, bytes);
    if (rc) return rc;
    int bits = 1;
    while (bits < 40 && ((unsigned long long)1 << bits) <= (unsigned long long)max_cap) ++bits;
    for (int g = 0; g < G; ++g)
        SCL_HIP(h, hipMemcpyAsync(h->d_pts + scans[g].byte_off, clouds[g], (size_t)n_points[g] * stride, hipMemcpyHostToDevice, h->stream));
    SCL_HIP(h, hipMemcpyAsync(h->d_scans, scans, sizeof(FpScan) * G, hipMemcpyHostToDevice, h->stream));
    SCL_HIP(h, hipMemsetAsync(h->d_bad, 0, sizeof(int) * G, h->stream));
    SCL_HIP(h, hipMemsetAsync(h->d_counts, 0, sizeof(unsigned int) * kCounts * G, h->stream));
    SCL_HIP(h, hipEventRecord(h->ev0, h->stream));
    const dim3 pgrid((unsigned)((max_n + kThreads - 1) / kThreads), (unsigned)G);
    hipLaunchKernelGGL(fpfh_grid_kernel, dim3(G), dim3(kGridThreads), 0, h->stream, h->d_pts, h->d_scans, stride, h->d_grids, h->d_bad);
    hipLaunchKernelGGL(fpfh_key_kernel, pgrid, dim3(kThreads), 0, h->stream, h->d_pts, h->d_scans, stride, h->d_grids, h->d_bad, h->d_keys0,
                       h->d_vals0, h->d_pos);
    SCL_HIP(h, scl::sort_pairs_u64_segmented(h->d_sort, h->d_keys0, h->d_keys1, h->d_vals0, h->d_vals1, seg, bits, h->stream));
    hipLaunchKernelGGL(fpfh_cells_kernel, pgrid, dim3(kThreads), 0, h->stream, h->d_scans, h->d_grids, h->d_keys1, h->d_vals1, h->d_pos,
                       h->d_starts, h->d_sp);
    hipLaunchKernelGGL(fpfh_knn_kernel, pgrid, dim3(kThreads), 0, h->stream, h->d_scans, h->d_grids, h->d_starts, h->d_sp, h->d_pos, h->d_bad,
                       h->d_normals, want_nbr ? h->d_nbr : nullptr, want_nbr ? h->d_nbr_d2 : nullptr, h->d_cand);
    hipLaunchKernelGGL(fpfh_spfh_kernel, dim3(kSpfhBlocks, G), dim3(kThreads), 0, h->stream, h->d_scans, h->d_pos, h->d_normals, h->d_bad,
                       h->d_counts);
    hipLaunchKernelGGL(fpfh_finish_kernel, dim3(G), dim3(64), 0, h->stream, h->d_scans, h->d_bad, h->d_counts, h->db.d_db);
    SCL_HIP(h, hipGetLastError());
    SCL_HIP(h, hipEventRecord(h->ev1, h->stream));
    int bad[kGroup];
    SCL_HIP(h, hipMemcpyAsync(bad, h->d_bad, sizeof(int) * G, hipMemcpyDeviceToHost, h->stream));
    SCL_HIP(h, hipStreamSynchronize(h->stream));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) h->kernel_us += 1000.0 * (double)ms;
    *any_bad = 0;
    for (int g = 0; g < G; ++g) {
        if (bad[g]) *any_bad = 1;
        h->points += (unsigned long long)n_points[g];
    }
    return SCL_OK;
}

// the reported distance between keys a and b: sqrtf of the squared L2 over the first report_dims floats, nanoflann's order
int scl_fpfh::reported_distance(int a, int b, float, float *dist)
{
    float va[kDim], vb[kDim];
    SCL_HIP(this, hipMemcpyAsync(va, db.row(a), sizeof va, hipMemcpyDeviceToHost, stream));
    SCL_HIP(this, hipMemcpyAsync(vb, db.row(b), sizeof vb, hipMemcpyDeviceToHost, stream));
    SCL_HIP(this, hipStreamSynchronize(stream));
    const int D = cfg.report_dims;
    float s = 0.0f;
    int k = 0;
    for (; k + 4 <= D; k += 4) {
        const float d0 = va[k] - vb[k], d1 = va[k + 1] - vb[k + 1], d2 = va[k + 2] - vb[k + 2], d3 = va[k + 3] - vb[k + 3];
        s += ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
    }
    for (; k < D; ++k) { const float d = va[k] - vb[k]; s += d * d; }
    *dist = sqrtf(s);
    return SCL_OK;
}

extern "C" {

int scl_fpfh_default_config(scl_fpfh_config *c)
{
    if (!c) return SCL_ERR_INVALID_ARG;
    c->device = 0; c->dist_thres = 100.0; c->num_exclude_recent = 30; c->tree_making_period = 10; c->report_dims = 21;
    c->inter_mode = 0; c->robot_num = 1; c->this_id = 0;
    return SCL_OK;
}

int scl_fpfh_create(const scl_fpfh_config *cfg, scl_fpfh **out)
{
    if (!cfg || !out) return SCL_ERR_INVALID_ARG;
    *out = nullptr;
    if (cfg->tree_making_period < 1 || cfg->report_dims < 1 || cfg->report_dims > kDim || (cfg->inter_mode != 0 && cfg->inter_mode != 1))
        return SCL_ERR_INVALID_ARG;
    scl_fpfh *h = nullptr;
    int rc = open_plugin(cfg, &h);
    if (rc) return rc;
    auto bail = [&](int code) { scl_fpfh_destroy(h); return code; };
    if ((rc = dev_alloc(h, &h->d_scans, kGroup)) || (rc = dev_alloc(h, &h->d_grids, kGroup)) || (rc = dev_alloc(h, &h->d_bad, kGroup)) ||
        (rc = dev_alloc(h, &h->d_counts, (size_t)kGroup * kCounts)) || (rc = dev_alloc(h, &h->d_cand, 1)))
        return bail(rc);
    if (hipMemset(h->d_cand, 0, sizeof(unsigned long long)) != hipSuccess) return bail(SCL_ERR_HIP);
    *out = h;
    return SCL_OK;
}

int scl_fpfh_destroy(scl_fpfh *h)
{
    if (!h) return SCL_OK;
    return close_plugin(h, {h->d_pts, h->d_pos, h->d_sp, h->d_normals, h->d_keys0, h->d_keys1, h->d_vals0, h->d_vals1, h->d_sort, h->d_starts,
                            h->d_scans, h->d_grids, h->d_bad, h->d_counts, h->d_cand, h->d_nbr, h->d_nbr_d2});
}

int scl_fpfh_neighbors(scl_fpfh *h, const void *points, int n_points, int stride_bytes, int32_t *idx, float *d2)
{
    if (!h) return SCL_ERR_INVALID_ARG;
    Entered<scl_fpfh> in(h);
    int rc = scl_fpfh::check_layout(h, points, n_points, stride_bytes), bad = 0;
    if (rc) return rc;
    if ((rc = h->db.grow(h, h->reg.n + 1))) return rc;
    if ((size_t)n_points * kK > h->nbr_cap) {
        const size_t c = (size_t)n_points * kK;
        if ((rc = dev_regrow(h, &h->d_nbr, c)) || (rc = dev_regrow(h, &h->d_nbr_d2, c))) return rc;
        h->nbr_cap = c;
    }
    if ((rc = scl_fpfh::run_group_locked(h, &points, &n_points, stride_bytes, 1, h->reg.n, &bad, true))) return rc;     // row n: scratch
    if (bad) return fail(h, SCL_ERR_INVALID_ARG, "non-finite coordinate");
    const size_t cnt = (size_t)n_points * (size_t)std::min(n_points, kK);
    if (idx) SCL_HIP(h, hipMemcpyAsync(idx, h->d_nbr, sizeof(int) * cnt, hipMemcpyDeviceToHost, h->stream));
    if (d2) SCL_HIP(h, hipMemcpyAsync(d2, h->d_nbr_d2, sizeof(float) * cnt, hipMemcpyDeviceToHost, h->stream));
    SCL_HIP(h, hipStreamSynchronize(h->stream));
    return SCL_OK;
}

int scl_fpfh_normals(scl_fpfh *h, const void *points, int n_points, int stride_bytes, float *normals)
{
    if (!h) return SCL_ERR_INVALID_ARG;
    Entered<scl_fpfh> in(h);
    int rc = run_single_locked(h, points, n_points, stride_bytes);
    if (rc) return rc;
    if (normals) {
        std::vector<float4> nv((size_t)n_points);
        SCL_HIP(h, hipMemcpyAsync(nv.data(), h->d_normals, sizeof(float4) * (size_t)n_points, hipMemcpyDeviceToHost, h->stream));
        SCL_HIP(h, hipStreamSynchronize(h->stream));
        for (int i = 0; i < n_points; ++i) { normals[3 * i] = nv[(size_t)i].x; normals[3 * i + 1] = nv[(size_t)i].y; normals[3 * i + 2] = nv[(size_t)i].z; }
    }
    return SCL_OK;
}

int scl_fpfh_counts(scl_fpfh *h, const void *points, int n_points, int stride_bytes, uint32_t *counts, uint32_t *skipped)
{
    if (!h) return SCL_ERR_INVALID_ARG;
    Entered<scl_fpfh> in(h);
    int rc = run_single_locked(h, points, n_points, stride_bytes);
    if (rc) return rc;
    uint32_t c[kCounts];
    SCL_HIP(h, hipMemcpyAsync(c, h->d_counts, sizeof c, hipMemcpyDeviceToHost, h->stream));
    SCL_HIP(h, hipStreamSynchronize(h->stream));
    if (counts) std::memcpy(counts, c, sizeof(uint32_t) * kDim);
    if (skipped) *skipped = c[kCounts - 1];
    return SCL_OK;
}

int scl_fpfh_values(const uint32_t *counts, int n, float hist_incr, float *out)
{
    if (n < 0 || (n > 0 && (!counts || !out))) return SCL_ERR_INVALID_ARG;
    for (int i = 0; i < n; ++i) out[i] = scl::fpfh_value(counts[i], hist_incr);
    return SCL_OK;
}

int scl_fpfh_acosf_blocks(scl_fpfh *h, int first_block, int n_blocks, uint64_t *checksums)
{
    if (!h || !checksums || first_block < 0 || n_blocks < 1 || first_block + n_blocks > 256) return SCL_ERR_INVALID_ARG;
    Entered<scl_fpfh> in(h);
    unsigned long long *d = nullptr;
    int rc = dev_alloc(h, &d, (size_t)n_blocks);
    if (rc) return rc;
    hipError_t he = hipMemsetAsync(d, 0, sizeof(unsigned long long) * (size_t)n_blocks, h->stream);
    if (he == hipSuccess) {
        hipLaunchKernelGGL(fpfh_acosf_blocks_kernel, dim3((1u << 24) / (kThreads * 16), (unsigned)n_blocks), dim3(kThreads), 0, h->stream,
                           first_block, d);
        he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipMemcpyAsync(checksums, d, sizeof(uint64_t) * (size_t)n_blocks, hipMemcpyDeviceToHost, h->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(h->stream);
    (void)hipFree(d);
    SCL_HIP(h, he);
    return SCL_OK;
}

int scl_fpfh_stats(const scl_fpfh *h, unsigned long long *points, unsigned long long *candidates, double *kernel_us)
{
    if (!h) return SCL_ERR_INVALID_ARG;
    Entered<scl_fpfh> in(h);
    unsigned long long c = 0;
    SCL_HIP(h, hipMemcpy(&c, h->d_cand, sizeof(c), hipMemcpyDeviceToHost));
    if (points) *points = h->points;
    if (candidates) *candidates = c;
    if (kernel_us) *kernel_us = h->kernel_us;
    return SCL_OK;
}

}  // extern "C"

SCL_VECTOR_PLUGIN_ENTRY_POINTS(scl_fpfh)
