// grsd.hip -- the GRSD descriptor on the GPU (include/scl_grsd.h; reference grsd_descriptor, include/descriptor.h:38-196).
// Numerics contract: DESIGN.md section 4 "GRSD": every stage is independent of traversal order.  Per launch group of up to 16
// scans (copied in once, resident until the descriptors are in the database):
//
//   grsd_bbox_kernel     one workgroup per scan: bounding box, non-finite flag, pcl::VoxelGrid's min_b / div_b for the leaf
//                        (= grsd_radius) and the int32 check of the voxel index range;
//   grsd_key_kernel      every point's voxel index (fp32: floor(p * 1/leaf) - min_b, x fastest) under the scan number as the sort key;
//   sort_pairs_u64_segmented (device_sort.hip): the points of every scan ordered by voxel, a voxel's points in input order;
//   grsd_heads_kernel    voxel heads flagged, the points gathered in voxel order; prefix_sum_i32 numbers the voxels of the group;
//   grsd_voxels_kernel   one thread per voxel: the fp32 centroid sums in input order, the voxel's index and point range;
//   grsd_normals_kernel  one lane per point, points taken in voxel order: the neighbours within ne_radius found in the rows of voxels
//                        the search box touches (a row's points are contiguous; its ends by bisection of the sorted voxel indices),
//                        the scatter as exact int64 sums, jacobi3, PCL's float flip;
//   grsd_rsd_kernel      one wave per voxel: the neighbour nearest to the centroid by a wave reduction of (d2, index) keys, then the
//                        angle to every valid neighbour normal, min / max per distance bin as unsigned integers (shuffles), the two
//                        radii and the class in lane 0;
//   grsd_trans_kernel    one thread per voxel: its 26 neighbour cells looked up by bisection, 6 x 6 counters per scan in LDS, then
//                        global atomics;
//   grsd_finish_kernel   counters -> the 21 floats, straight into the database slot.
// The database, the keyframe registry, make_and_save_many and the 1-NN detection (nn_l2_kernel<21>): plugin_host.hpp.
#include "scl_grsd.h"

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
#include "plugin_host.hpp"

using namespace scl;

namespace {

constexpr int kGroup = SCL_GRSD_MAX_GROUP;
constexpr int kDim = SCL_GRSD_DIM;
constexpr int kT = SCL_GRSD_CLASSES * SCL_GRSD_CLASSES;
constexpr int kThreads = 256;
constexpr int kBoxThreads = 1024;
constexpr int kVoxelBlocks = 2048;           // workgroups of the per-voxel kernels (they stride over the group's voxels)
constexpr int kBins = 5;                     // nr_subdiv
constexpr unsigned int kUnset = 0xffffffffu;

struct GrScan {
    unsigned long long byte_off;             // first byte of the scan in the group's point buffer
    int n;
    int slot;                                // database row that receives the descriptor
    int pt_off;                              // first element of the scan in the group's per-point arrays
    int pad;
};

struct GrGrid {
    int minb[3];
    int divb[3];
    int vox_first, vox_last;                 // the scan's voxels [vox_first, vox_last) among the group's
};

struct GrParams {
    float inv_leaf;                          // 1.0f / (float)grsd_radius
    float ne_r2, ne_rw;                      // (float)(ne_radius^2); a radius slightly above ne_radius for the search box
    float rsd_r2, rsd_rw;
    double max_dist;                         // grsd_radius
};

__device__ __forceinline__ const float *point_at(const unsigned char *pts, const GrScan &sc, int stride, int i)
{
    return reinterpret_cast<const float *>(pts + sc.byte_off + (unsigned long long)i * (unsigned long long)stride);
}

__global__ __launch_bounds__(kBoxThreads) void grsd_bbox_kernel(const unsigned char *pts, const GrScan *scans, int stride, float inv,
                                                                GrGrid *grids, int *bad)
{
    __shared__ float red[6][kBoxThreads / 64];
    __shared__ int nonfinite;
    const GrScan sc = scans[blockIdx.x];
    const int t = threadIdx.x;
    if (t == 0) nonfinite = 0;
    __syncthreads();
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    bool nf = false;
    for (int i = t; i < sc.n; i += kBoxThreads) {
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
    for (int w = 1; w < kBoxThreads / 64; ++w)
        for (int a = 0; a < 3; ++a) { red[a][0] = fminf(red[a][0], red[a][w]); red[3 + a][0] = fmaxf(red[3 + a][0], red[3 + a][w]); }
    GrGrid g;
    bool big = false;
    long long div[3];
    for (int a = 0; a < 3; ++a) {                                          // as voxel.hip's vox_setup_kernel_body
        const float lo = nonfinite ? 0.f : floorf(red[a][0] * inv), hi = nonfinite ? 0.f : floorf(red[3 + a][0] * inv);
        const bool in_range = lo >= -2147483648.f && hi <= 2147483520.f;
        big |= !in_range;
        const long long mb = in_range ? (long long)lo : 0;
        div[a] = in_range ? (long long)hi - mb + 1 : 1;
        big |= div[a] > 2147483647LL;
        g.minb[a] = (int)mb; g.divb[a] = big ? 1 : (int)div[a];
    }
    if (!big) {
        const long long xy = div[0] * div[1];
        big = xy > 2147483647LL || xy * div[2] > 2147483647LL;
    }
    g.vox_first = 0; g.vox_last = 0;
    grids[blockIdx.x] = g;
    bad[blockIdx.x] = nonfinite ? 1 : (big ? 2 : 0);
}

__device__ __forceinline__ unsigned int voxel_of(float x, float y, float z, float inv, const GrGrid &g)
{
    const long long i0 = (long long)floorf(x * inv) - g.minb[0], i1 = (long long)floorf(y * inv) - g.minb[1],
                    i2 = (long long)floorf(z * inv) - g.minb[2];
    return (unsigned int)(i0 + i1 * g.divb[0] + i2 * (long long)g.divb[0] * g.divb[1]);
}

__global__ __launch_bounds__(kThreads) void grsd_key_kernel(const unsigned char *pts, const GrScan *scans, int stride, float inv,
                                                            const GrGrid *grids, const int *bad, unsigned long long *keys, unsigned int *vals,
                                                            float4 *pos)
{
    const GrScan sc = scans[blockIdx.y];
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= sc.n) return;
    const float *p = point_at(pts, sc, stride, i);
    const float x = p[0], y = p[1], z = p[2];
    const unsigned int vox = bad[blockIdx.y] ? 0u : voxel_of(x, y, z, inv, grids[blockIdx.y]);
    keys[sc.pt_off + i] = ((unsigned long long)blockIdx.y << 32) | vox;
    vals[sc.pt_off + i] = (unsigned int)i;
    pos[sc.pt_off + i] = make_float4(x, y, z, 0.0f);
}

// i runs over the sorted points of the whole group
__global__ __launch_bounds__(kThreads) void grsd_heads_kernel(const GrScan *scans, const unsigned long long *keys, const unsigned int *vals,
                                                              const float4 *pos, int total, int *head, float4 *sp)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const unsigned long long k = keys[i];
    head[i] = (i == 0 || keys[i - 1] != k) ? 1 : 0;
    const unsigned int o = vals[i];
    float4 p = pos[scans[(int)(k >> 32)].pt_off + o];
    p.w = __uint_as_float(o);
    sp[i] = p;
}

// one thread per voxel (the thread of its head): the centroid as fp32 sums in input order (the sort is stable), as voxel.hip
__global__ __launch_bounds__(kThreads) void grsd_voxels_kernel(const GrScan *scans, const unsigned long long *keys, const float4 *sp,
                                                               const int *head, const int *vid, int total, float4 *cent, unsigned int *vkey,
                                                               int *vstart, int *vend, int *vscan, GrGrid *grids, int *n_voxels)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= total || !head[i]) return;
    const unsigned long long k = keys[i];
    const int s = (int)(k >> 32), v = vid[i];
    float sx = 0.f, sy = 0.f, sz = 0.f;
    int b = i;
    while (b < total && keys[b] == k) {
        const float4 p = sp[b];
        sx += p.x; sy += p.y; sz += p.z;
        ++b;
    }
    const float cnt = (float)(b - i);
    cent[v] = make_float4(sx / cnt, sy / cnt, sz / cnt, 0.0f);
    vkey[v] = (unsigned int)k; vstart[v] = i; vend[v] = b; vscan[v] = s;
    const GrScan sc = scans[s];
    if (i == sc.pt_off) grids[s].vox_first = v;
    if (b == sc.pt_off + sc.n) grids[s].vox_last = v + 1;
    if (b == total) *n_voxels = v + 1;
}

// first voxel of [a, b) whose index is >= key
__device__ __forceinline__ int lower_bound(const unsigned int *vkey, int a, int b, unsigned int key)
{
    while (a < b) {
        const int m = (a + b) >> 1;
        if (vkey[m] < key) a = m + 1; else b = m;
    }
    return a;
}

// The cells a search box of half-width rw around coordinate c touches along one axis: a float at or below c - rw (at or above
// c + rw) through the voxel rule floor(x * inv) - min_b, which is monotone in x: every point within rw of c has its cell in
// [lo, hi].  Clamped to the grid (a box outside it keeps one cell, whose points then fail the distance test).
__device__ __forceinline__ void cell_range(float c, float rw, float inv, int minb, int divb, int &lo, int &hi)
{
    const float a = nextafterf(c - rw, -INFINITY), b = nextafterf(c + rw, INFINITY);
    const double fa = (double)floorf(a * inv) - (double)minb, fb = (double)floorf(b * inv) - (double)minb, top = (double)(divb - 1);
    lo = (int)fmin(fmax(fa, 0.0), top);
    hi = (int)fmin(fmax(fb, 0.0), top);
}

// the sorted points [*a, *b) of the row of cells x0 .. x1 at (y, z)
__device__ __forceinline__ void row_points(const GrGrid &g, const unsigned int *vkey, const int *vstart, const int *vend, int x0, int x1, int y,
                                           int z, int &a, int &b)
{
    const unsigned int base = (unsigned int)(((long long)z * g.divb[1] + y) * g.divb[0]);
    const int va = lower_bound(vkey, g.vox_first, g.vox_last, base + (unsigned int)x0);
    const int vb = lower_bound(vkey, va, g.vox_last, base + (unsigned int)x1 + 1u);
    a = b = 0;
    if (va < vb) { a = vstart[va]; b = vend[vb - 1]; }
}

__global__ __launch_bounds__(kThreads) void grsd_normals_kernel(const GrScan *scans, const GrGrid *grids, const int *bad, GrParams prm,
                                                                const float4 *sp, const unsigned int *vkey, const int *vstart,
                                                                const int *vend, float4 *normals, float4 *nsp)
{
    const GrScan sc = scans[blockIdx.y];
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= sc.n || bad[blockIdx.y]) return;
    const GrGrid g = grids[blockIdx.y];
    const float4 q = sp[sc.pt_off + i];
    int x0, x1, y0, y1, z0, z1;
    cell_range(q.x, prm.ne_rw, prm.inv_leaf, g.minb[0], g.divb[0], x0, x1);
    cell_range(q.y, prm.ne_rw, prm.inv_leaf, g.minb[1], g.divb[1], y0, y1);
    cell_range(q.z, prm.ne_rw, prm.inv_leaf, g.minb[2], g.divb[2], z0, z1);
    long long n = 0, s0 = 0, s1 = 0, s2 = 0, s00 = 0, s01 = 0, s02 = 0, s11 = 0, s12 = 0, s22 = 0;
    for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y) {
            int a, b;
            row_points(g, vkey, vstart, vend, x0, x1, y, z, a, b);
            for (int j = a; j < b; ++j) {
                const float4 c = sp[j];
                const float dx = c.x - q.x, dy = c.y - q.y, dz = c.z - q.z;
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                if (!(d2 < prm.ne_r2)) continue;
                const long long qa = (long long)rint((double)dx * 1048576.0), qb = (long long)rint((double)dy * 1048576.0),
                                qc = (long long)rint((double)dz * 1048576.0);
                n += 1; s0 += qa; s1 += qb; s2 += qc;
                s00 += qa * qa; s01 += qa * qb; s02 += qa * qc; s11 += qb * qb; s12 += qb * qc; s22 += qc * qc;
            }
        }
    float4 out = make_float4(__int_as_float(0x7fc00000), __int_as_float(0x7fc00000), __int_as_float(0x7fc00000), 0.0f);
    if (n >= 3) {
        const double dn = (double)n, m0 = (double)s0, m1 = (double)s1, m2 = (double)s2;
        const double c00 = (double)s00 - m0 * m0 / dn, c01 = (double)s01 - m0 * m1 / dn, c02 = (double)s02 - m0 * m2 / dn,
                     c11 = (double)s11 - m1 * m1 / dn, c12 = (double)s12 - m1 * m2 / dn, c22 = (double)s22 - m2 * m2 / dn;
        double a[3][3] = {{c00, c01, c02}, {c01, c11, c12}, {c02, c12, c22}}, v[3][3];
        jacobi3(a, v);
        int m = 0;
        if (a[1][1] < a[m][m]) m = 1;
        if (a[2][2] < a[m][m]) m = 2;
        float nx = (float)v[0][m], ny = (float)v[1][m], nz = (float)v[2][m];
        const float vx = 0.0f - q.x, vy = 0.0f - q.y, vz = 0.0f - q.z;
        if ((vx * nx + vy * ny) + vz * nz < 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
        out = make_float4(nx, ny, nz, 1.0f);
    }
    normals[sc.pt_off + (int)__float_as_uint(q.w)] = out;
    nsp[sc.pt_off + i] = out;
}

__device__ __forceinline__ unsigned int wave_min_u32(unsigned int v)
{
    for (int off = 32; off > 0; off >>= 1) v = min(v, (unsigned int)__shfl_xor((int)v, off));
    return v;
}

__device__ __forceinline__ unsigned int wave_max_u32(unsigned int v)
{
    for (int off = 32; off > 0; off >>= 1) v = max(v, (unsigned int)__shfl_xor((int)v, off));
    return v;
}

// PCL's getSimpleType on the float radii (thresholds as doubles): 0 noise, 1 plane, 2 cylinder, 3 sphere, 4 edge
__device__ __forceinline__ int simple_type(float r_min, float r_max)
{
    if ((double)r_min > 0.1) return 1;
    if ((double)r_max > 0.175) return 2;
    if ((double)r_min < 0.015) return 0;
    if ((double)(r_max - r_min) < 0.05) return 3;
    return 4;
}

// one wave per voxel, the waves stride over the voxels of the whole group
__global__ __launch_bounds__(kThreads) void grsd_rsd_kernel(const GrGrid *grids, const int *bad, GrParams prm, const int *n_voxels,
                                                            const float4 *sp, const float4 *nsp, const float4 *cent, const int *vscan,
                                                            const unsigned int *vkey, const int *vstart, const int *vend, float *r_min,
                                                            float *r_max, int *cls)
{
    const int lane = threadIdx.x & 63, waves = gridDim.x * (kThreads / 64), total = *n_voxels;
    for (int v = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); v < total; v += waves) {
        const int s = vscan[v];
        if (bad[s]) continue;
        const GrGrid g = grids[s];
        const float4 c = cent[v];
        int x0, x1, y0, y1, z0, z1;
        cell_range(c.x, prm.rsd_rw, prm.inv_leaf, g.minb[0], g.divb[0], x0, x1);
        cell_range(c.y, prm.rsd_rw, prm.inv_leaf, g.minb[1], g.divb[1], y0, y1);
        cell_range(c.z, prm.rsd_rw, prm.inv_leaf, g.minb[2], g.divb[2], z0, z1);
        // pass 1: the neighbour count and the smallest (d2, index) key
        unsigned long long best = ~0ull;
        int count = 0, at = -1;
        for (int z = z0; z <= z1; ++z)
            for (int y = y0; y <= y1; ++y) {
                int a, b;
                row_points(g, vkey, vstart, vend, x0, x1, y, z, a, b);
                for (int j = a + lane; j < b; j += 64) {
                    const float4 p = sp[j];
                    const float dx = p.x - c.x, dy = p.y - c.y, dz = p.z - c.z;
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    if (!(d2 < prm.rsd_r2)) continue;
                    count += 1;
                    const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)__float_as_uint(p.w);
                    if (key < best) { best = key; at = j; }
                }
            }
        unsigned long long nearest = best;
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(nearest, off);
            nearest = o < nearest ? o : nearest;
            count += __shfl_xor(count, off);
        }
        // the keys are distinct (the index): one lane holds the nearest neighbour's sorted position
        at = (best == nearest) ? at : -1;
        for (int off = 32; off > 0; off >>= 1) at = max(at, __shfl_xor(at, off));
        // pass 2: the angles.  Bin 0 starts at (0, 0), bins 1 .. 4 unset
        unsigned int mn[kBins], mx[kBins];
#pragma unroll
        for (int k = 0; k < kBins; ++k) { mn[k] = k == 0 ? 0u : kUnset; mx[k] = 0u; }
        float4 ref = make_float4(0.f, 0.f, 0.f, 0.f);
        if (count >= 2) ref = nsp[at];
        if (count >= 2 && ref.w != 0.0f) {
            const float pi = __int_as_float(0x40490fdb), pio2 = __int_as_float(0x3fc90fdb);
            for (int z = z0; z <= z1; ++z)
                for (int y = y0; y <= y1; ++y) {
                    int a, b;
                    row_points(g, vkey, vstart, vend, x0, x1, y, z, a, b);
                    for (int j = a + lane; j < b; j += 64) {
                        const float4 p = sp[j];
                        const float dx = p.x - c.x, dy = p.y - c.y, dz = p.z - c.z;
                        const float d2 = (dx * dx + dy * dy) + dz * dz;
                        if (!(d2 < prm.rsd_r2)) continue;
                        const float4 nj = nsp[j];
                        if (nj.w == 0.0f) continue;
                        float cosine = (ref.x * nj.x + ref.y * nj.y) + ref.z * nj.z;
                        cosine = cosine > 1.0f ? 1.0f : (cosine < -1.0f ? -1.0f : cosine);
                        float angle = acosf_glibc(cosine);
                        if (angle > pio2) angle = pi - angle;
                        const double dist = sqrt((double)d2);
                        int bin = (int)floor(5.0 * dist / prm.max_dist);
                        bin = bin > kBins - 1 ? kBins - 1 : bin;
                        const unsigned int ab = __float_as_uint(angle);
#pragma unroll
                        for (int k = 0; k < kBins; ++k)
                            if (bin == k) { mn[k] = min(mn[k], ab); mx[k] = max(mx[k], ab); }
                    }
                }
        }
#pragma unroll
        for (int k = 0; k < kBins; ++k) { mn[k] = wave_min_u32(mn[k]); mx[k] = wave_max_u32(mx[k]); }
        if (lane != 0) continue;
        float rmin = 0.0f, rmax = 0.0f;
        if (count >= 2) {
            double amin = 0.0, amin_d = 0.0, amax = 0.0, amax_d = 0.0;
#pragma unroll
            for (int k = 0; k < kBins; ++k) {
                if (mn[k] == kUnset) continue;
                const double f = ((double)k + 0.5) * prm.max_dist / 5.0;
                const double pmin = (double)__uint_as_float(mn[k]), pmax = (double)__uint_as_float(mx[k]);
                amin += pmin * pmin; amin_d += pmin * f;
                amax += pmax * pmax; amax_d += pmax * f;
            }
            const double plane_radius = 0.2;
            const double ra = amin == 0.0 ? plane_radius : fmin(amin_d / amin, plane_radius);
            const double rb = amax == 0.0 ? plane_radius : fmin(amax_d / amax, plane_radius);
            float fa = (float)ra, fb = (float)rb;
            fa = (float)((double)fa * 1.1); fb = (float)((double)fb * 1.1);
            rmin = fa < fb ? fa : fb; rmax = fa < fb ? fb : fa;
        }
        r_min[v] = rmin; r_max[v] = rmax; cls[v] = simple_type(rmin, rmax);
    }
}

__global__ __launch_bounds__(kThreads) void grsd_trans_kernel(const GrGrid *grids, const int *bad, float inv, const int *n_voxels,
                                                              const float4 *cent, const int *vscan, const unsigned int *vkey, const int *cls,
                                                              unsigned int *counters)
{
    __shared__ unsigned int ts[kGroup * kT];
    for (int t = threadIdx.x; t < kGroup * kT; t += kThreads) ts[t] = 0u;
    __syncthreads();
    const int total = *n_voxels;
    for (int v = blockIdx.x * kThreads + threadIdx.x; v < total; v += gridDim.x * kThreads) {
        const int s = vscan[v];
        if (bad[s]) continue;
        const GrGrid g = grids[s];
        const float4 c = cent[v];
        // PCL's getNeighborCentroidIndices: the cell of the centroid itself, displaced by the 26 offsets
        const long long cx = (long long)floorf(c.x * inv) - g.minb[0], cy = (long long)floorf(c.y * inv) - g.minb[1],
                        cz = (long long)floorf(c.z * inv) - g.minb[2];
        const int mine = cls[v];
        for (int o = 0; o < 27; ++o) {
            if (o == 13) continue;
            const long long x = cx + (o % 3 - 1), y = cy + (o / 3 % 3 - 1), z = cz + (o / 9 - 1);
            int other = 5;
            if (x >= 0 && x < g.divb[0] && y >= 0 && y < g.divb[1] && z >= 0 && z < g.divb[2]) {
                const unsigned int key = (unsigned int)(x + y * g.divb[0] + z * (long long)g.divb[0] * g.divb[1]);
                const int at = lower_bound(vkey, g.vox_first, g.vox_last, key);
                if (at < g.vox_last && vkey[at] == key) other = cls[at];
            }
            atomicAdd(&ts[s * kT + mine * SCL_GRSD_CLASSES + other], 1u);
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < kGroup * kT; t += kThreads)
        if (ts[t]) atomicAdd(&counters[t], ts[t]);
}

__global__ __launch_bounds__(64) void grsd_finish_kernel(const GrScan *scans, const int *bad, const unsigned int *counters, float *db)
{
    const GrScan sc = scans[blockIdx.x];
    if (bad[blockIdx.x] || threadIdx.x != 0) return;
    const unsigned int *T = counters + (size_t)blockIdx.x * kT;
    int k = 0;
    for (int i = 0; i < SCL_GRSD_CLASSES; ++i)
        for (int j = i; j < SCL_GRSD_CLASSES; ++j)
            db[(size_t)sc.slot * kDim + k++] = (float)(T[i * SCL_GRSD_CLASSES + j] + T[j * SCL_GRSD_CLASSES + i]);
}

}  // namespace

struct __attribute__((visibility("hidden"))) scl_grsd : scl::VectorPlugin<kDim> {
    static constexpr int kGroup = ::kGroup;
    scl_grsd_config cfg;
    GrParams prm;
    // the launch group's workspace (per point -- a group has at most as many voxels as points -- and per scan)
    unsigned char *d_pts = nullptr; size_t pts_cap = 0;
    size_t pt_cap = 0, sort_cap = 0;
    float4 *d_pos = nullptr, *d_sp = nullptr, *d_normals = nullptr, *d_nsp = nullptr, *d_cent = nullptr;
    unsigned long long *d_keys0 = nullptr, *d_keys1 = nullptr;
    unsigned int *d_vals0 = nullptr, *d_vals1 = nullptr, *d_vkey = nullptr;
    int *d_head = nullptr, *d_vid = nullptr, *d_vstart = nullptr, *d_vend = nullptr, *d_vscan = nullptr, *d_cls = nullptr;
    float *d_rmin = nullptr, *d_rmax = nullptr;
    void *d_sort = nullptr;
    GrScan *d_scans = nullptr;
    GrGrid *d_grids = nullptr;
    int *d_bad = nullptr, *d_nvox = nullptr;
    unsigned int *d_T = nullptr;
    int last_voxels = 0;                     // voxels of the last launch group (the hooks read one cloud's)
    unsigned long long points = 0, voxels = 0;

    bool inter_snapshot() const { return cfg.inter_mode == 0; }
    int snapshot_period() const { return cfg.tree_making_period; }
    const char *bad_cloud(int bad) const
    {
        return bad == 2 ? "GRSD: the voxel index range of the cloud overflows int32: nothing of the call was stored"
                        : "non-finite coordinate: nothing of the call was stored";
    }
    static int check_layout(scl_grsd *h, const void *points, int n_points, int stride);
    static int run_group_locked(scl_grsd *h, const void *const *clouds, const int *n_points, int stride, int G, int slot0, int *any_bad);
};

int scl_grsd::check_layout(scl_grsd *h, const void *points, int n_points, int stride)
{
    if (stride < 12 || (stride & 3)) return fail(h, SCL_ERR_INVALID_ARG, "bad point layout (stride_bytes >= 12, multiple of 4)");
    if (n_points < 1) return fail(h, SCL_ERR_INVALID_ARG, "GRSD needs at least 1 point");
    if (n_points > SCL_GRSD_MAX_POINTS) return fail(h, SCL_ERR_INVALID_ARG, "GRSD: more than 2^22 points in one cloud");
    if (!points) return fail(h, SCL_ERR_INVALID_ARG, "null point pointer");
    return SCL_OK;
}

// the workspace for a group of `pts` points and `bytes` bytes of input
static int reserve(scl_grsd *h, size_t pts, size_t bytes)
{
    int rc;
    if (bytes > h->pts_cap) {
        const size_t c = bytes + bytes / 4 + 4096;
        if ((rc = dev_regrow(h, &h->d_pts, c))) return rc;
        h->pts_cap = c;
    }
    if (pts > h->pt_cap) {
        const size_t c = pts + pts / 4 + 1024;
        h->pt_cap = 0;
        if ((rc = dev_regrow(h, &h->d_pos, c)) || (rc = dev_regrow(h, &h->d_sp, c)) || (rc = dev_regrow(h, &h->d_normals, c)) ||
            (rc = dev_regrow(h, &h->d_nsp, c)) || (rc = dev_regrow(h, &h->d_cent, c)) || (rc = dev_regrow(h, &h->d_keys0, c)) ||
            (rc = dev_regrow(h, &h->d_keys1, c)) || (rc = dev_regrow(h, &h->d_vals0, c)) || (rc = dev_regrow(h, &h->d_vals1, c)) ||
            (rc = dev_regrow(h, &h->d_vkey, c)) || (rc = dev_regrow(h, &h->d_head, c)) || (rc = dev_regrow(h, &h->d_vid, c)) ||
            (rc = dev_regrow(h, &h->d_vstart, c)) || (rc = dev_regrow(h, &h->d_vend, c)) || (rc = dev_regrow(h, &h->d_vscan, c)) ||
            (rc = dev_regrow(h, &h->d_cls, c)) || (rc = dev_regrow(h, &h->d_rmin, c)) || (rc = dev_regrow(h, &h->d_rmax, c)))
            return rc;
        h->pt_cap = c;
    }
    const size_t sb = std::max(scl::sort_scratch_bytes(h->pt_cap, kGroup), scl::scan_scratch_bytes(h->pt_cap)) + 256;
    if (sb > h->sort_cap) {
        unsigned char *p = nullptr;
        if ((rc = dev_alloc(h, &p, sb))) return rc;
        if (h->d_sort) (void)hipFree(h->d_sort);
        h->d_sort = p; h->sort_cap = sb;
    }
    return SCL_OK;
}

// One launch group (G <= 16 clouds): descriptors into database rows slot0 .. slot0 + G - 1 (capacity ensured by the caller).
// *any_bad = 1 if a cloud has a non-finite coordinate, 2 if its voxel index range overflows int32.
int scl_grsd::run_group_locked(scl_grsd *h, const void *const *clouds, const int *n_points, int stride, int G, int slot0, int *any_bad)
{
    GrScan scans[kGroup];
    unsigned long long bytes = 0;
    size_t pts = 0;
    int max_n = 0;
    scl::SortSegments seg{};
    unsigned int seg_hi[scl::kSortMaxSegments];
    seg.nseg = G;
    for (int g = 0; g < G; ++g) {
        scans[g].byte_off = bytes; scans[g].n = n_points[g]; scans[g].slot = slot0 + g; scans[g].pt_off = (int)pts; scans[g].pad = 0;
        seg.off[g] = (int)pts; seg_hi[g] = (unsigned int)g;
        bytes += (unsigned long long)n_points[g] * (unsigned long long)stride;
        pts += (size_t)n_points[g];
        max_n = std::max(max_n, n_points[g]);
    }
    seg.off[G] = (int)pts;
    int rc = reserve(h, pts, bytes);
    if (rc) return rc;
    const int total = (int)pts;
    for (int g = 0; g < G; ++g)
        SCL_HIP(h, hipMemcpyAsync(h->d_pts + scans[g].byte_off, clouds[g], (size_t)n_points[g] * stride, hipMemcpyHostToDevice, h->stream));
    SCL_HIP(h, hipMemcpyAsync(h->d_scans, scans, sizeof(GrScan) * G, hipMemcpyHostToDevice, h->stream));
    SCL_HIP(h, hipMemsetAsync(h->d_T, 0, sizeof(unsigned int) * kT * kGroup, h->stream));
    SCL_HIP(h, hipMemsetAsync(h->d_nvox, 0, sizeof(int), h->stream));
    SCL_HIP(h, hipEventRecord(h->ev0, h->stream));
    const GrParams prm = h->prm;
    const dim3 pgrid((unsigned)((max_n + kThreads - 1) / kThreads), (unsigned)G), tgrid((unsigned)((total + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(grsd_bbox_kernel, dim3(G), dim3(kBoxThreads), 0, h->stream, h->d_pts, h->d_scans, stride, prm.inv_leaf, h->d_grids, h->d_bad);
    hipLaunchKernelGGL(grsd_key_kernel, pgrid, dim3(kThreads), 0, h->stream, h->d_pts, h->d_scans, stride, prm.inv_leaf, h->d_grids, h->d_bad,
                       h->d_keys0, h->d_vals0, h->d_pos);
    SCL_HIP(h, scl::sort_pairs_u64_segmented(h->d_sort, h->d_keys0, h->d_keys1, h->d_vals0, h->d_vals1, seg, 32, h->stream, seg_hi));
    hipLaunchKernelGGL(grsd_heads_kernel, tgrid, dim3(kThreads), 0, h->stream, h->d_scans, h->d_keys1, h->d_vals1, h->d_pos, total, h->d_head,
                       h->d_sp);
    SCL_HIP(h, scl::prefix_sum_i32(h->d_sort, h->d_head, h->d_vid, total, false, h->stream));
    hipLaunchKernelGGL(grsd_voxels_kernel, tgrid, dim3(kThreads), 0, h->stream, h->d_scans, h->d_keys1, h->d_sp, h->d_head, h->d_vid, total,
                       h->d_cent, h->d_vkey, h->d_vstart, h->d_vend, h->d_vscan, h->d_grids, h->d_nvox);
    hipLaunchKernelGGL(grsd_normals_kernel, pgrid, dim3(kThreads), 0, h->stream, h->d_scans, h->d_grids, h->d_bad, prm, h->d_sp, h->d_vkey,
                       h->d_vstart, h->d_vend, h->d_normals, h->d_nsp);
    const int vblocks = std::min(kVoxelBlocks, (total + kThreads / 64 - 1) / (kThreads / 64));
    hipLaunchKernelGGL(grsd_rsd_kernel, dim3((unsigned)vblocks), dim3(kThreads), 0, h->stream, h->d_grids, h->d_bad, prm, h->d_nvox, h->d_sp,
                       h->d_nsp, h->d_cent, h->d_vscan, h->d_vkey, h->d_vstart, h->d_vend, h->d_rmin, h->d_rmax, h->d_cls);
    const int tblocks = std::min(kVoxelBlocks, (total + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(grsd_trans_kernel, dim3((unsigned)tblocks), dim3(kThreads), 0, h->stream, h->d_grids, h->d_bad, prm.inv_leaf, h->d_nvox,
                       h->d_cent, h->d_vscan, h->d_vkey, h->d_cls, h->d_T);
    hipLaunchKernelGGL(grsd_finish_kernel, dim3(G), dim3(64), 0, h->stream, h->d_scans, h->d_bad, h->d_T, h->db.d_db);
    SCL_HIP(h, hipGetLastError());
    SCL_HIP(h, hipEventRecord(h->ev1, h->stream));
    int bad[kGroup], nvox = 0;
    SCL_HIP(h, hipMemcpyAsync(bad, h->d_bad, sizeof(int) * G, hipMemcpyDeviceToHost, h->stream));
    SCL_HIP(h, hipMemcpyAsync(&nvox, h->d_nvox, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    SCL_HIP(h, hipStreamSynchronize(h->stream));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) h->kernel_us += 1000.0 * (double)ms;
    *any_bad = 0;
    for (int g = 0; g < G; ++g) {
        if (bad[g]) *any_bad = std::max(*any_bad, bad[g]);
        h->points += (unsigned long long)n_points[g];
    }
    h->last_voxels = nvox;
    if (!*any_bad) h->voxels += (unsigned long long)nvox;
    return SCL_OK;
}

extern "C" {

int scl_grsd_default_config(scl_grsd_config *c)
{
    if (!c) return SCL_ERR_INVALID_ARG;
    c->device = 0; c->ne_radius = 0.5; c->grsd_radius = 2.0; c->dist_thres = 160.0; c->num_exclude_recent = 30; c->tree_making_period = 10;
    c->inter_mode = 0; c->robot_num = 1; c->this_id = 0;
    return SCL_OK;
}

int scl_grsd_create(const scl_grsd_config *cfg, scl_grsd **out)
{
    if (!cfg || !out) return SCL_ERR_INVALID_ARG;
    *out = nullptr;
    // ne_radius <= 1: |q| <= 2^20 (1 + 2^-23) + 1/2 per axis, a product below 2^40.1, a sum over 2^22 points below 2^62.1 (scl_grsd.h)
    if (cfg->tree_making_period < 1 || (cfg->inter_mode != 0 && cfg->inter_mode != 1) || !(cfg->ne_radius > 0.0 && cfg->ne_radius <= 1.0) ||
        !(cfg->grsd_radius > 0.0 && cfg->grsd_radius <= 1.0e6) || !((float)cfg->grsd_radius > 0.0f) ||
        !((float)(cfg->ne_radius * cfg->ne_radius) > 0.0f))
        return SCL_ERR_INVALID_ARG;
    scl_grsd *h = nullptr;
    int rc = open_plugin(cfg, &h);
    if (rc) return rc;
    h->prm.inv_leaf = 1.0f / (float)cfg->grsd_radius;
    h->prm.ne_r2 = (float)(cfg->ne_radius * cfg->ne_radius); h->prm.ne_rw = (float)(cfg->ne_radius * 1.00001);
    h->prm.rsd_r2 = (float)(cfg->grsd_radius * cfg->grsd_radius); h->prm.rsd_rw = (float)(cfg->grsd_radius * 1.00001);
    h->prm.max_dist = cfg->grsd_radius;
    if ((rc = dev_alloc(h, &h->d_scans, kGroup)) || (rc = dev_alloc(h, &h->d_grids, kGroup)) || (rc = dev_alloc(h, &h->d_bad, kGroup)) ||
        (rc = dev_alloc(h, &h->d_T, (size_t)kGroup * kT)) || (rc = dev_alloc(h, &h->d_nvox, 1))) {
        scl_grsd_destroy(h);
        return rc;
    }
    *out = h;
    return SCL_OK;
}

int scl_grsd_destroy(scl_grsd *h)
{
    if (!h) return SCL_OK;
    return close_plugin(h, {h->d_pts, h->d_pos, h->d_sp, h->d_normals, h->d_nsp, h->d_cent, h->d_keys0, h->d_keys1, h->d_vals0, h->d_vals1,
                            h->d_vkey, h->d_head, h->d_vid, h->d_vstart, h->d_vend, h->d_vscan, h->d_cls, h->d_rmin, h->d_rmax, h->d_sort,
                            h->d_scans, h->d_grids, h->d_bad, h->d_nvox, h->d_T});
}

int scl_grsd_normals(scl_grsd *h, const void *points, int n_points, int stride_bytes, float *normals, uint8_t *valid)
{
    if (!h) return SCL_ERR_INVALID_ARG;
    Entered<scl_grsd> in(h);
    int rc = run_single_locked(h, points, n_points, stride_bytes);
    if (rc) return rc;
    std::vector<float4> nv((size_t)n_points);
    SCL_HIP(h, hipMemcpyAsync(nv.data(), h->d_normals, sizeof(float4) * (size_t)n_points, hipMemcpyDeviceToHost, h->stream));
    SCL_HIP(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < n_points; ++i) {
        if (normals) { normals[3 * i] = nv[(size_t)i].x; normals[3 * i + 1] = nv[(size_t)i].y; normals[3 * i + 2] = nv[(size_t)i].z; }
        if (valid) valid[i] = nv[(size_t)i].w != 0.0f ? 1 : 0;
    }
    return SCL_OK;
}

int scl_grsd_voxels(scl_grsd *h, const void *points, int n_points, int stride_bytes, int *n_voxels, float *centroids, float *r_min,
                    float *r_max, int32_t *classes)
{
    if (!h) return SCL_ERR_INVALID_ARG;
    Entered<scl_grsd> in(h);
    int rc = run_single_locked(h, points, n_points, stride_bytes);
    if (rc) return rc;
    const size_t nv = (size_t)h->last_voxels;
    if (n_voxels) *n_voxels = (int)nv;
    std::vector<float4> cv(nv);
    SCL_HIP(h, hipMemcpyAsync(cv.data(), h->d_cent, sizeof(float4) * nv, hipMemcpyDeviceToHost, h->stream));
    if (r_min) SCL_HIP(h, hipMemcpyAsync(r_min, h->d_rmin, sizeof(float) * nv, hipMemcpyDeviceToHost, h->stream));
    if (r_max) SCL_HIP(h, hipMemcpyAsync(r_max, h->d_rmax, sizeof(float) * nv, hipMemcpyDeviceToHost, h->stream));
    if (classes) SCL_HIP(h, hipMemcpyAsync(classes, h->d_cls, sizeof(int) * nv, hipMemcpyDeviceToHost, h->stream));
    SCL_HIP(h, hipStreamSynchronize(h->stream));
    if (centroids)
        for (size_t v = 0; v < nv; ++v) { centroids[3 * v] = cv[v].x; centroids[3 * v + 1] = cv[v].y; centroids[3 * v + 2] = cv[v].z; }
    return SCL_OK;
}

int scl_grsd_transitions(scl_grsd *h, const void *points, int n_points, int stride_bytes, uint32_t *counters)
{
    if (!h) return SCL_ERR_INVALID_ARG;
    Entered<scl_grsd> in(h);
    int rc = run_single_locked(h, points, n_points, stride_bytes);
    if (rc) return rc;
    if (counters) {
        SCL_HIP(h, hipMemcpyAsync(counters, h->d_T, sizeof(uint32_t) * kT, hipMemcpyDeviceToHost, h->stream));
        SCL_HIP(h, hipStreamSynchronize(h->stream));
    }
    return SCL_OK;
}

int scl_grsd_stats(const scl_grsd *h, unsigned long long *points, unsigned long long *voxels, double *kernel_us)
{
    if (!h) return SCL_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (points) *points = h->points;
    if (voxels) *voxels = h->voxels;
    if (kernel_us) *kernel_us = h->kernel_us;
    return SCL_OK;
}

}  // extern "C"

SCL_VECTOR_PLUGIN_ENTRY_POINTS(scl_grsd)
