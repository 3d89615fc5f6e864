// plugin_host.hpp -- the host layer the descriptor plugins share (iris.hip, m2dp.hip, fpfh.hip, grsd.hip; engine.hip and sharded_front.hip
// take the error helpers): the HIP-check macro and error helpers, the keyframe registry behind the get_size / get_index / local_to_global
// entry points and the inter-detection candidate rule, and for the vector plugins (M2DP, FPFH, GRSD) everything but their kernels: the
// float-row database, the 1-NN search with its batched and k-nearest forms, the handle base (scl::VectorPlugin), the C entry points as
// function templates and the macro that defines the extern "C" functions from them.  No descriptor logic lives here.
//
// Every helper that touches a handle assumes its lock is held (the `_locked` convention; std::mutex is not recursive), except
// the entry points, which take it once.  A handle provides `mutable std::mutex mu`, `mutable std::string last_error`,
// `hipStream_t stream` and `scl::KeyframeRegistry reg`; a vector plugin's derives from scl::VectorPlugin<DIM> and adds `cfg`.
// Included from .hip files only (the search kernels are device code).  Everything here has internal linkage (the unnamed namespace)
// and the vector plugins' handles are marked hidden: the library exports its C ABI and nothing of this layer.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "nn_plan.hpp"
#include "scl_engine.h"
#include "scl_plugin_batch.h"

// a failed HIP call: its text and the runtime's message into h->last_error, SCL_ERR_NOMEM / SCL_ERR_HIP returned
#define SCL_HIP(h_, call)                                                              \
    do {                                                                               \
        hipError_t err__ = (call);                                                     \
        if (err__ != hipSuccess) {                                                     \
            (h_)->last_error = std::string(#call) + ": " + hipGetErrorString(err__);   \
            return err__ == hipErrorOutOfMemory ? SCL_ERR_NOMEM : SCL_ERR_HIP;         \
        }                                                                              \
    } while (0)

namespace scl {
namespace {

template <class H> int fail(const H *h, int code, const char *msg)
{
    if (h) h->last_error = msg;
    return code;
}

template <class H, class T> int dev_alloc(H *h, T **p, size_t count)
{
    void *q = nullptr;
    SCL_HIP(h, hipMalloc(&q, sizeof(T) * (count ? count : 1)));
    *p = static_cast<T *>(q);
    return SCL_OK;
}

// *p freed (if any) and allocated again for `count` elements: nothing is copied
template <class H, class T> int dev_regrow(H *h, T **p, size_t count)
{
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    return dev_alloc(h, p, count);
}

// room for `need` elements (of `per` Ts each) in *p, whose capacity is *cap: past it the buffer is allocated again for need + need / 2
// + 256 elements, nothing copied.  The capacity is zero while the pointer is invalid
template <class H, class T> int dev_reserve(H *h, T **p, size_t *cap, size_t need, size_t per = 1)
{
    if (need <= *cap) return SCL_OK;
    *cap = 0;
    const size_t c = need + need / 2 + 256;
    int rc = dev_regrow(h, p, per * c);
    if (rc) return rc;
    *cap = c;
    return SCL_OK;
}

// ---- keyframe registry (the reference's plugin layer, D.h:501-509, 1055-1057): global key -> (robot, index), and per robot
// the global keys of its keyframes in arrival order
struct KeyframeRegistry {
    int robot_num = 0, n = 0;
    std::vector<int8_t> robots;
    std::vector<int> indexs;
    std::vector<std::vector<int>> local2global;

    void init(int robot_count)
    {
        robot_num = robot_count;
        local2global.resize((size_t)robot_count);
    }
    bool robot_ok(int robot) const { return robot >= 0 && robot < robot_num; }
    const std::vector<int> &keys_of(int robot) const { return local2global[(size_t)robot]; }
    void commit(int8_t robot, int index)
    {
        local2global[(size_t)robot].push_back(n);
        robots.push_back(robot); indexs.push_back(index); n++;
    }
    // The inter-detection search set of key `cur` (newLocal2Global, D.h:1167-1195): a keyframe of this robot searches every
    // other robot's, a keyframe of another robot searches this robot's.  In the reference's concatenation order, NOT sorted:
    // Iris's tie-breaking depends on it; the vector plugins sort the list themselves.
    std::vector<int> inter_candidates(int cur, int this_id) const
    {
        if (robots[(size_t)cur] != this_id) return local2global[(size_t)this_id];
        std::vector<int> list;
        for (int i = 0; i < robot_num; ++i)
            if (i != this_id) list.insert(list.end(), local2global[(size_t)i].begin(), local2global[(size_t)i].end());
        return list;
    }
};

template <class H> int check_robot(const H *h, int robot, int code)
{
    return h->reg.robot_ok(robot) ? SCL_OK : fail(h, code, "robot id outside [0, robot_num)");
}

// the registry's C entry points (scl_*_get_size, _get_size_of, _get_index, _local_to_global): one lock each
template <class H> int get_size(const H *h)
{
    if (!h) return SCL_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    return h->reg.n;
}

template <class H> int get_size_of(const H *h, int id)
{
    if (!h) return SCL_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (id == -1) return h->reg.n;                                            // D.h:1262-1265
    if (int rc = check_robot(h, id, SCL_ERR_OUT_OF_RANGE)) return rc;
    return (int)h->reg.keys_of(id).size();                                    // D.h:1268
}

template <class H> int get_index(const H *h, int key, int8_t *robot, int *index)
{
    if (!h || !robot || !index) return SCL_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (key < 0 || key >= h->reg.n) return fail(h, SCL_ERR_OUT_OF_RANGE, "key out of range");
    *robot = h->reg.robots[(size_t)key]; *index = h->reg.indexs[(size_t)key];
    return SCL_OK;
}

template <class H> int local_to_global(const H *h, int robot, int local, int *key)
{
    if (!h || !key) return SCL_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = check_robot(h, robot, SCL_ERR_OUT_OF_RANGE)) return rc;
    const std::vector<int> &l2g = h->reg.keys_of(robot);
    if (local < 0 || local >= (int)l2g.size()) return fail(h, SCL_ERR_OUT_OF_RANGE, "local index out of range");
    *key = l2g[(size_t)local];
    return SCL_OK;
}

// ---- the vector plugins' database: one row of DIM floats per key, rows [0, reg.n) live
template <int DIM> struct FloatRows {
    static constexpr int kDim = DIM;
    float *d_db = nullptr;
    int cap = 0;

    float *row(int key) const { return d_db + (size_t)key * DIM; }
    // room for `need` rows: the capacity starts at 256 and doubles, the live rows are copied on the stream, which is synchronised
    template <class H> int grow(H *h, int need)
    {
        if (need <= cap) return SCL_OK;
        int ncap = cap > 0 ? cap : 256;
        while (ncap < need) ncap *= 2;
        float *nd = nullptr;
        int rc = dev_alloc(h, &nd, (size_t)ncap * DIM);
        if (rc) return rc;
        if (h->reg.n > 0) SCL_HIP(h, hipMemcpyAsync(nd, d_db, sizeof(float) * DIM * h->reg.n, hipMemcpyDeviceToDevice, h->stream));
        SCL_HIP(h, hipStreamSynchronize(h->stream));
        if (d_db) (void)hipFree(d_db);
        d_db = nd; cap = ncap;
        return SCL_OK;
    }
    // one row from the host (capacity ensured by the caller)
    template <class H> int write(H *h, int key, const float *values)
    {
        SCL_HIP(h, hipMemcpyAsync(row(key), values, sizeof(float) * DIM, hipMemcpyHostToDevice, h->stream));
        SCL_HIP(h, hipStreamSynchronize(h->stream));
        return SCL_OK;
    }
    // rows key .. key + count - 1 to the host
    template <class H> int read(H *h, int key, int count, float *values)
    {
        SCL_HIP(h, hipMemcpyAsync(values, row(key), sizeof(float) * DIM * (size_t)count, hipMemcpyDeviceToHost, h->stream));
        SCL_HIP(h, hipStreamSynchronize(h->stream));
        return SCL_OK;
    }
};

// make_and_save_many of a vector plugin: every cloud (H::check_layout) and robot id validated first, then launch groups of up to
// H::kGroup clouds into rows n .. n + count - 1 (H::run_group_locked); the first group with an invalid cloud ends the call, and
// nothing of the call is committed
template <class H>
int make_and_save_many_locked(H *h, const void *const *clouds, const int *n_points, int stride, const int8_t *robots,
                              const int *indexs, int count, float *out_values)
{
    for (int i = 0; i < count; ++i) {
        int rc = H::check_layout(h, clouds[i], n_points[i], stride);
        if (rc) return rc;
        if ((rc = check_robot(h, robots[i], SCL_ERR_INVALID_ARG))) return rc;
    }
    if (count == 0) return SCL_OK;
    int rc = h->db.grow(h, h->reg.n + count);
    if (rc) return rc;
    for (int s = 0; s < count; s += H::kGroup) {
        const int G = std::min((int)H::kGroup, count - s);
        int bad = 0;
        if ((rc = H::run_group_locked(h, clouds + s, n_points + s, stride, G, h->reg.n + s, &bad))) return rc;
        if (bad) return fail(h, SCL_ERR_INVALID_ARG, "non-finite coordinate: nothing of the call was stored");
    }
    if (out_values && (rc = h->db.read(h, h->reg.n, count, out_values))) return rc;
    for (int i = 0; i < count; ++i) h->reg.commit(robots[i], indexs[i]);
    return SCL_OK;
}

// one cloud through the chain into row reg.n (scratch, not committed): make and the test hooks
template <class H> int run_single_locked(H *h, const void *points, int n_points, int stride)
{
    int rc = H::check_layout(h, points, n_points, stride), bad = 0;
    if (rc) return rc;
    if ((rc = h->db.grow(h, h->reg.n + 1))) return rc;
    if ((rc = H::run_group_locked(h, &points, &n_points, stride, 1, h->reg.n, &bad))) return rc;
    if (bad) return fail(h, SCL_ERR_INVALID_ARG, h->bad_cloud(bad));
    return SCL_OK;
}

// ---- 1-NN: squared L2 in nanoflann's float order (L2_Adaptor: groups of four, ((d0*d0 + d1*d1) + d2*d2) + d3*d3, then the
// tail one element at a time) between row qkey and rows list[0 .. n) (list == nullptr: rows 0 .. n - 1); the (distance bits,
// position) keys reduced by a 64-bit atomic min: ties go to the lowest position.  A NaN sum (a non-finite row from the wire)
// has a bit pattern above +inf's, so it loses to every other sum, as in nanoflann's result set (dist < worst)
constexpr int kNnThreads = 256;

template <int DIM>
__global__ __launch_bounds__(kNnThreads) void nn_l2_kernel(const float *db, const int *list, int n, int qkey, unsigned long long *best)
{
    __shared__ alignas(16) float q[DIM];                               // read through float4 * below when DIM % 4 == 0
    for (int i = threadIdx.x; i < DIM; i += kNnThreads) q[i] = db[(size_t)qkey * DIM + i];
    __syncthreads();
    const int i = blockIdx.x * kNnThreads + threadIdx.x;
    unsigned long long key = ~0ull;
    if (i < n) {
        const float *c = db + (size_t)(list ? list[i] : i) * DIM;
        float s = 0.0f;
        if constexpr (DIM % 4 == 0) {                                  // rows of whole float4s
            const float4 *a4 = reinterpret_cast<const float4 *>(q), *c4 = reinterpret_cast<const float4 *>(c);
            for (int k = 0; k < DIM / 4; ++k) {
                const float4 x = a4[k], y = c4[k];
                const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
                s += ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
            }
        } else {
            for (int k = 0; k < DIM / 4 * 4; k += 4) {
                const float d0 = q[k] - c[k], d1 = q[k + 1] - c[k + 1], d2 = q[k + 2] - c[k + 2], d3 = q[k + 3] - c[k + 3];
                s += ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
            }
            for (int k = DIM / 4 * 4; k < DIM; ++k) {
                const float d = q[k] - c[k];
                s += d * d;
            }
        }
        key = ((unsigned long long)__float_as_uint(s) << 32) | (unsigned int)i;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(key, off);
        key = o < key ? o : key;
    }
    if ((threadIdx.x & 63) == 0 && key != ~0ull) atomicMin(best, key);
}

// the nearest of `list` (n global keys; nullptr: keys 0 .. n - 1) to key `q`: its position in the list (-1 if n <= 0) and
// the squared distance (+inf if n <= 0)
template <class H> int nearest_locked(H *h, int q, const int *list, int n, int *pos, float *d2)
{
    constexpr int DIM = decltype(h->db)::kDim;
    *pos = -1; *d2 = INFINITY;
    if (n <= 0) return SCL_OK;
    if (list)
        if (int rc = dev_reserve(h, &h->d_list, &h->list_cap, (size_t)n)) return rc;
    if (list) SCL_HIP(h, hipMemcpyAsync(h->d_list, list, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    SCL_HIP(h, hipMemsetAsync(h->d_best, 0xff, sizeof(unsigned long long), h->stream));
    hipLaunchKernelGGL(nn_l2_kernel<DIM>, dim3((unsigned)((n + kNnThreads - 1) / kNnThreads)), dim3(kNnThreads), 0, h->stream, h->db.d_db,
                       list ? h->d_list : nullptr, n, q, h->d_best);
    SCL_HIP(h, hipGetLastError());
    unsigned long long best = ~0ull;
    SCL_HIP(h, hipMemcpyAsync(&best, h->d_best, sizeof(best), hipMemcpyDeviceToHost, h->stream));
    SCL_HIP(h, hipStreamSynchronize(h->stream));
    if (best == ~0ull) return fail(h, SCL_ERR_HIP, "nearest neighbour: no key reduced");
    const unsigned int bits = (unsigned int)(best >> 32);
    std::memcpy(d2, &bits, sizeof(float));
    *pos = (int)(best & 0xffffffffu);
    return SCL_OK;
}

// ---- batched 1-NN: one launch scores up to SCL_PLUGIN_DETECT_GROUP queries against one shared candidate list, the database rows
// read once per launch.  Query q (row qkey[q]) searches the prefix list[0 .. limit[q]) -- every search set the plugins use is a
// prefix of one list: intra = this robot's keys [0, cur - num_exclude_recent), the reference's inter mode = keys [0, snap_n), M2DP's
// inter rule = a whole sorted list -- and best[q] receives the same (distance bits, position) key as nn_l2_kernel's.
//
// A workgroup is one wave and owns a tile of 64 candidates, one per lane.  Their rows go through LDS in chunks of kChunk floats
// (coalesced loads: consecutive lanes read consecutive floats of a row), the group's query rows are staged once.  A lane then reads
// its candidate's values once per chunk and every query value as a broadcast, and keeps the 16 running sums in registers: per
// (candidate, query) pair the sum over k stays in one lane, in nn_l2_kernel's order (the chunks are whole groups of four; the
// tail exists only where a row is one chunk).  The row pitch in LDS is odd: lane l reads dword l * pitch + k, bank (l * pitch + k)
// % 32 for ds_read_b32, distinct over a 32-lane half (a pitch of 192 would put every lane on one bank).
constexpr int kDetectGroup = SCL_PLUGIN_DETECT_GROUP;
constexpr int kManyTile = 64;

template <int DIM> struct NnManyShape {
    static constexpr int kChunk = DIM <= 64 ? DIM : 32;
    static constexpr int kPitch = kChunk | 1;
    static_assert(DIM % kChunk == 0 && (kChunk % 4 == 0 || kChunk == DIM), "a chunk is whole groups of four, or the whole row");
};

// The body the 1-NN and the k-NN tile kernels share, so that both form the same floats: lane t's sums s[q] between candidate
// blockIdx.x * kManyTile + t of the list and the group's queries.  Returns lim[] in LDS for the epilogue: limit[q], 0 for an absent query
template <int DIM>
__device__ __forceinline__ const int *nn_tile_sums(const float *db, const int *list, int n, const int *qkey, const int *limit, int nq,
                                                   float (&s)[kDetectGroup])
{
    constexpr int KC = NnManyShape<DIM>::kChunk, P = NnManyShape<DIM>::kPitch;
    __shared__ alignas(16) float qs[kDetectGroup * DIM];               // rows of absent queries (q >= nq): zeros, their sums unused
    __shared__ float cs[kManyTile * P];
    __shared__ int ks[kManyTile], lim[kDetectGroup];
    const int t = threadIdx.x, base = blockIdx.x * kManyTile, i = base + t;
    const int rows = min(kManyTile, n - base);
    for (int e = t; e < kDetectGroup * DIM; e += kManyTile) {
        const int q = e / DIM;
        qs[e] = q < nq ? db[(size_t)qkey[q] * DIM + (e - q * DIM)] : 0.0f;
    }
    if (t < kDetectGroup) lim[t] = t < nq ? limit[t] : 0;
    if (t < rows) ks[t] = list ? list[i] : i;
#pragma unroll
    for (int q = 0; q < kDetectGroup; ++q) s[q] = 0.0f;
    for (int k0 = 0; k0 < DIM; k0 += KC) {
        __syncthreads();                                               // ks / qs written; the previous chunk read
        for (int e = t; e < rows * KC; e += kManyTile) {
            const int c = e / KC, k = e - c * KC;
            cs[c * P + k] = db[(size_t)ks[c] * DIM + k0 + k];
        }
        __syncthreads();
        if (t < rows) {
            const float *c = cs + t * P;
#pragma unroll
            for (int k = 0; k + 4 <= KC; k += 4) {
                const float c0 = c[k], c1 = c[k + 1], c2 = c[k + 2], c3 = c[k + 3];
#pragma unroll
                for (int q = 0; q < kDetectGroup; ++q) {
                    const float *a = qs + q * DIM + k0 + k;
                    const float d0 = a[0] - c0, d1 = a[1] - c1, d2 = a[2] - c2, d3 = a[3] - c3;
                    s[q] += ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
                }
            }
#pragma unroll
            for (int k = KC / 4 * 4; k < KC; ++k) {
                const float ck = c[k];
#pragma unroll
                for (int q = 0; q < kDetectGroup; ++q) {
                    const float d = qs[q * DIM + k0 + k] - ck;
                    s[q] += d * d;
                }
            }
        }
    }
    return lim;
}

template <int DIM>
__global__ __launch_bounds__(kManyTile) void nn_l2_many_kernel(const float *db, const int *list, int n, const int *qkey, const int *limit,
                                                               int nq, unsigned long long *best)
{
    float s[kDetectGroup];
    const int *lim = nn_tile_sums<DIM>(db, list, n, qkey, limit, nq, s);
    const int t = threadIdx.x, i = blockIdx.x * kManyTile + t;
#pragma unroll
    for (int q = 0; q < kDetectGroup; ++q) {
        unsigned long long key = i < lim[q] ? ((unsigned long long)__float_as_uint(s[q]) << 32) | (unsigned int)i : ~0ull;   // lim[q] <= n
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(key, off);
            key = o < key ? o : key;
        }
        if (t == 0 && key != ~0ull) atomicMin(best + q, key);
    }
}

// What a search reports for the candidate at position `pos` of a query's list (list_off: where the list starts in `list`, -1 for
// keys 0 .. n - 1): its global key into *key, and sqrtf of the squared distance between its row and the query's row `a` (in global
// memory or in LDS) over the first report_dims floats, in nanoflann's order
template <int DIM>
__device__ __forceinline__ float nn_reported(const float *db, const int *list, int list_off, int pos, const float *a, int report_dims, int *key)
{
    *key = list_off < 0 ? pos : list[list_off + pos];
    const float *c = db + (size_t)*key * DIM;
    float s = 0.0f;
    int k = 0;
    for (; k + 4 <= report_dims; k += 4) {
        const float d0 = a[k] - c[k], d1 = a[k + 1] - c[k + 1], d2 = a[k + 2] - c[k + 2], d3 = a[k + 3] - c[k + 3];
        s += ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
    }
    for (; k < report_dims; ++k) {
        const float d = a[k] - c[k];
        s += d * d;
    }
    return sqrtf(s);
}

// what a batched search answers per query: the winner's position in its list and its global key (-1, -1: nothing reduced, an empty
// prefix), the 1-NN's squared distance (+inf then) and the reported distance (+inf then)
struct NnManyResult {
    int pos, key;
    float d2, dist;
};

// the finishing step, one thread per query of the whole call: best[q] -> NnManyResult without the host in between
template <int DIM>
__global__ __launch_bounds__(kNnThreads) void nn_finish_many_kernel(const float *db, const int *list, const int *qkey, const int *list_off,
                                                                    const unsigned long long *best, int count,
                                                                    int report_dims, NnManyResult *res)
{
    const int q = blockIdx.x * kNnThreads + threadIdx.x;
    if (q >= count) return;
    NnManyResult r = {-1, -1, INFINITY, INFINITY};
    const unsigned long long b = best[q];
    if (b != ~0ull) {
        r.pos = (int)(b & 0xffffffffu);
        r.d2 = __uint_as_float((unsigned int)(b >> 32));
        r.dist = nn_reported<DIM>(db, list, list_off[q], r.pos, db + (size_t)qkey[q] * DIM, report_dims, &r.key);
    }
    res[q] = r;
}

// ---- batched k-NN (the candidate lists, SCL_PLUGIN_TOPK_API): the sums of nn_l2_many_kernel -- both kernels call nn_tile_sums, so
// bit for bit the same floats -- but instead of the atomic min every wave emits, per query, the min(k, valid) smallest
// (sum bits << 32 | position) keys of its tile in ascending order into part[(q * tiles + tile) * k + j]; unused slots are ~0ull.  Valid: position < limit[q] and the sum not NaN (nanoflann's KNNResultSet admits dist < worst only; +inf
// is a distance like any other).  A tile at or past limit[q] writes nothing for q: the merge reads the tiles below the limit only.
//
// The selection is a bitonic sorting network over the wave's 64 keys, one per lane, through __shfl_xor: 21 compare-exchange stages
// whatever k is, against 6 shuffle steps per listed entry for k rounds of wave-min with knock-out (192 at k = 32), and the sorted
// order falls out of it.  The keys of a tile are distinct (the position is part of them) apart from the ~0ull fillers, which are
// interchangeable, so the network's result does not depend on anything but the keys: no atomics, no workgroup order.
constexpr int kTopkMax = SCL_PLUGIN_TOPK_MAX;
static_assert(kTopkMax <= kManyTile, "a wave lists at most one key per lane");

__device__ __forceinline__ unsigned long long wave_sort_ascending(unsigned long long key, int lane)
{
#pragma unroll
    for (int k2 = 2; k2 <= kManyTile; k2 <<= 1)
#pragma unroll
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            const unsigned long long o = __shfl_xor(key, j);
            const bool keep_min = ((lane & j) == 0) == ((lane & k2) == 0);        // k2 == 64: every pair ascending
            key = (o < key) == keep_min ? o : key;
        }
    return key;
}

template <int DIM>
__global__ __launch_bounds__(kManyTile) void nn_l2_topk_kernel(const float *db, const int *list, int n, const int *qkey, const int *limit,
                                                               int nq, int k, unsigned long long *part)
{
    float s[kDetectGroup];
    const int *lim = nn_tile_sums<DIM>(db, list, n, qkey, limit, nq, s);
    const int t = threadIdx.x, base = blockIdx.x * kManyTile, i = base + t;
#pragma unroll
    for (int q = 0; q < kDetectGroup; ++q) {
        if (base >= lim[q]) continue;                              // the same for every lane (lim[q] <= n; absent queries: 0)
        const bool valid = i < lim[q] && s[q] == s[q];
        unsigned long long key = valid ? ((unsigned long long)__float_as_uint(s[q]) << 32) | (unsigned int)i : ~0ull;
        key = wave_sort_ascending(key, t);
        if (t < k) part[((size_t)q * gridDim.x + blockIdx.x) * (size_t)k + t] = key;
    }
}

// one listed candidate of a query: its position in the query's list and its global key (-1, -1: the slot is unused) and the
// reported distance (+inf for an unused slot)
struct NnTopkEntry {
    int pos, key;
    float dist;
};

// the merge and the finishing step, one workgroup per query of the whole call: the query's (tiles below its limit) * k partial keys,
// which start at part[part_row[q] * k], go through LDS in rounds of up to kTopkMergeCap - k keys beside the k best so far, each
// round one bitonic sort of the next power of two; then one thread per listed entry does what nn_finish_many_kernel does for the
// winner and writes res[q * k + j]
constexpr int kTopkMergeCap = 2048;

template <int DIM>
__global__ __launch_bounds__(kNnThreads) void nn_topk_merge_kernel(const float *db, const int *list, const int *qkey, const int *list_off,
                                                                   const int *limit, const int *part_row, const unsigned long long *part,
                                                                   int k, int report_dims, NnTopkEntry *res)
{
    __shared__ unsigned long long buf[kTopkMergeCap];
    __shared__ float a[DIM];
    const int q = blockIdx.x, t = threadIdx.x;
    for (int e = t; e < DIM; e += kNnThreads) a[e] = db[(size_t)qkey[q] * DIM + e];
    if (t < k) buf[t] = ~0ull;
    const size_t total = (size_t)((limit[q] + kManyTile - 1) / kManyTile) * (size_t)k;
    const unsigned long long *src = part + (size_t)part_row[q] * (size_t)k;
    for (size_t done = 0; done < total;) {
        const int chunk = total - done < (size_t)(kTopkMergeCap - k) ? (int)(total - done) : kTopkMergeCap - k;
        int m = 2;
        while (m < k + chunk) m <<= 1;                                 // <= kTopkMergeCap
        for (int e = t; e < m - k; e += kNnThreads) buf[k + e] = e < chunk ? src[done + e] : ~0ull;
        __syncthreads();
        for (int k2 = 2; k2 <= m; k2 <<= 1)
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                for (int e = t; e < m / 2; e += kNnThreads) {
                    const int lo = ((e & ~(j - 1)) << 1) | (e & (j - 1)), hi = lo | j;
                    const unsigned long long x = buf[lo], y = buf[hi];
                    if ((x > y) == ((lo & k2) == 0)) { buf[lo] = y; buf[hi] = x; }
                }
                __syncthreads();
            }
        done += (size_t)chunk;
    }
    __syncthreads();                                                   // total == 0: buf[0 .. k) and a[] written
    if (t >= k) return;
    NnTopkEntry r = {-1, -1, INFINITY};
    const unsigned long long b = buf[t];
    if (b != ~0ull) {
        r.pos = (int)(b & 0xffffffffu);
        r.dist = nn_reported<DIM>(db, list, list_off[q], r.pos, a, report_dims, &r.key);
    }
    res[(size_t)q * (size_t)k + t] = r;
}

// the work buffers of a batched search on a handle (`many` with R = NnManyResult for the 1-NN form, `topk` with R = NnTopkEntry for
// the candidate lists; the lists share d_list): they grow like d_list
template <class R> struct NnWork {
    int *d_q = nullptr;                          // the plan's table: qkey | limit | list_off [| part_row], `count` elements each
    unsigned long long *d_keys = nullptr;        // 1-NN: best[query]; k-NN: the partial lists [query][tile][k], group after group
    R *d_res = nullptr;                          // 1-NN: [query]; k-NN: [query][k]
    size_t q_cap = 0, keys_cap = 0, res_cap = 0;
    void release()
    {
        for (void *p : {(void *)d_q, (void *)d_keys, (void *)d_res})
            if (p) (void)hipFree(p);
        d_q = nullptr; d_keys = nullptr; d_res = nullptr; q_cap = keys_cap = res_cap = 0;
    }
};

// ---- what every vector plugin's handle holds: scl_m2dp, scl_fpfh and scl_grsd derive from it and add `cfg` (device, dist_thres,
// num_exclude_recent, robot_num, this_id and the plugin's own fields), their workspace and their counters.  The plugin's rules are
// members of the derived handle; the ones below are the defaults, hidden by a plugin that differs:
//   report_dims()           the floats a reported distance is taken over (FPFH: cfg.report_dims);
//   inter_snapshot()        detect_inter is the reference's (every key below a snapshot taken each snapshot_period() calls), not
//                           M2DP's rule (the sorted keys of the other robots) -- FPFH and GRSD: cfg.inter_mode == 0;
//   reported_distance()     the distance a single detection reports for the winner (FPFH: over report_dims floats, on the host);
//   bad_cloud()             the message of a single cloud the kernels flagged;
// and the launch group has no default: static int check_layout(H *, points, n_points, stride), static int run_group_locked(H *,
// clouds, n_points, stride, G, slot0, &any_bad) and kGroup, the clouds of one group.
template <int DIM> struct VectorPlugin {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;                 // around a launch group's kernels: kernel_us
    mutable std::mutex mu;
    mutable std::string last_error;
    KeyframeRegistry reg;
    FloatRows<DIM> db;
    unsigned long long *d_best = nullptr;
    int *d_list = nullptr; size_t list_cap = 0;
    NnWork<NnManyResult> many;                               // the batched detections' work buffers
    NnWork<NnTopkEntry> topk;                                // the candidate lists' work buffers
    double kernel_us = 0.0;
    // the reference's inter detection state: the call counter and the snapshot [0, snap_n) taken at the last rebuild
    int tree_counter = 0, snap_n = 0;

    int report_dims() const { return DIM; }
    bool inter_snapshot() const { return false; }
    int snapshot_period() const { return 1; }
    int reported_distance(int, int, float d2, float *dist) { *dist = sqrtf(d2); return SCL_OK; }
    const char *bad_cloud(int) const { return "non-finite coordinate"; }
};

// ---- the driver of a batched search.  `count` queries in one call: query i is row qkey[i] against the prefix [0, limit[i]) of
// lists[which[i]] (limit[i] <= its n).  k == 0 with R = NnManyResult: the nearest, out[i]; k >= 1 with R = NnTopkEntry: the k nearest,
// out[i * k + j] the j-th by (squared distance bits, position), an unused slot (fewer than k candidates with a non-NaN distance) as
// NnTopkEntry says; both in the caller's order.  The queries are grouped by list (nn_plan.hpp) and run in groups of 16 back to back
// on the stream -- nn_l2_many_kernel into best[], or nn_l2_topk_kernel into the partial lists -- then the finishing or the merge
// kernel over all queries; ONE device-to-host copy and ONE synchronisation for the whole call
template <class H, class R>
int nearest_batch_locked(H *h, NnWork<R> &w, const int *qkey, const int *limit, const int *which, const NnList lists[2], int count, int k,
                         int report_dims, R *out)
{
    constexpr int DIM = decltype(h->db)::kDim;
    constexpr bool kOne = std::is_same<R, NnManyResult>::value;        // k == 0
    if (count <= 0) return SCL_OK;
    NnPlan p;
    if (!nn_plan<kDetectGroup, kManyTile>(qkey, limit, which, lists, count, k, &p))
        return fail(h, SCL_ERR_NOMEM, "candidate lists: the partial lists pass 2^31 rows");
    const size_t per = kOne ? 1 : (size_t)k, n_keys = kOne ? (size_t)count : p.rows * per, n_res = (size_t)count * per;
    int rc;
    if ((rc = dev_reserve(h, &h->d_list, &h->list_cap, p.keys)) || (rc = dev_reserve(h, &w.d_q, &w.q_cap, (size_t)count, (size_t)p.cols)) ||
        (rc = dev_reserve(h, &w.d_keys, &w.keys_cap, n_keys)) || (rc = dev_reserve(h, &w.d_res, &w.res_cap, n_res)))
        return rc;
    for (int l = 0; l < 2; ++l)
        if (p.off[l] >= 0)
            SCL_HIP(h, hipMemcpyAsync(h->d_list + p.off[l], lists[l].keys, sizeof(int) * (size_t)p.used[l], hipMemcpyHostToDevice, h->stream));
    SCL_HIP(h, hipMemcpyAsync(w.d_q, p.table.data(), sizeof(int) * p.table.size(), hipMemcpyHostToDevice, h->stream));
    if (kOne) SCL_HIP(h, hipMemsetAsync(w.d_keys, 0xff, sizeof(unsigned long long) * (size_t)count, h->stream));
    const int *d_qkey = w.d_q, *d_limit = w.d_q + count, *d_off = w.d_q + 2 * (size_t)count, *d_row = w.d_q + 3 * (size_t)count;
    for (const NnGroup &g : p.groups) {
        if (g.n <= 0) continue;                                        // every prefix empty: best stays unset, the merge reads no tile
        const int *d_keys_of_list = p.off[g.list] >= 0 ? h->d_list + p.off[g.list] : nullptr;
        if constexpr (kOne)
            hipLaunchKernelGGL(nn_l2_many_kernel<DIM>, dim3((unsigned)g.tiles), dim3(kManyTile), 0, h->stream, h->db.d_db, d_keys_of_list, g.n,
                               d_qkey + g.first, d_limit + g.first, g.G, w.d_keys + g.first);
        else
            hipLaunchKernelGGL(nn_l2_topk_kernel<DIM>, dim3((unsigned)g.tiles), dim3(kManyTile), 0, h->stream, h->db.d_db, d_keys_of_list, g.n,
                               d_qkey + g.first, d_limit + g.first, g.G, k, w.d_keys + (size_t)p.table[3 * (size_t)count + g.first] * per);
    }
    if constexpr (kOne)
        hipLaunchKernelGGL(nn_finish_many_kernel<DIM>, dim3((unsigned)((count + kNnThreads - 1) / kNnThreads)), dim3(kNnThreads), 0, h->stream,
                           h->db.d_db, h->d_list, d_qkey, d_off, w.d_keys, count, report_dims, w.d_res);
    else
        hipLaunchKernelGGL(nn_topk_merge_kernel<DIM>, dim3((unsigned)count), dim3(kNnThreads), 0, h->stream, h->db.d_db, h->d_list, d_qkey, d_off,
                           d_limit, d_row, w.d_keys, k, report_dims, w.d_res);
    SCL_HIP(h, hipGetLastError());
    std::vector<R> res(n_res);
    SCL_HIP(h, hipMemcpyAsync(res.data(), w.d_res, sizeof(R) * n_res, hipMemcpyDeviceToHost, h->stream));
    SCL_HIP(h, hipStreamSynchronize(h->stream));
    for (int j = 0; j < count; ++j) std::copy_n(res.begin() + (size_t)j * per, per, out + (size_t)p.order[(size_t)j] * per);
    return SCL_OK;
}

template <class H>
int nearest_many_locked(H *h, const int *qkey, const int *limit, const int *which, const NnList lists[2], int count, int report_dims,
                        NnManyResult *out)
{
    return nearest_batch_locked(h, h->many, qkey, limit, which, lists, count, 0, report_dims, out);
}

template <class H>
int nearest_topk_many_locked(H *h, const int *qkey, const int *limit, const int *which, const NnList lists[2], int count, int k,
                             int report_dims, NnTopkEntry *out)
{
    return nearest_batch_locked(h, h->topk, qkey, limit, which, lists, count, k, report_dims, out);
}

// ---- the search sets of the detections, each rule written once: the single calls, the batched calls and the candidate lists all
// take theirs from search_sets_locked.  Query i is row qkey[i] against the prefix [0, limit[i]) of lists[which[i]]
struct NnSearch {
    std::vector<int> qkey, limit, which, others;
    NnList lists[2] = {{nullptr, 0}, {nullptr, 0}};
    bool too_few = false;                        // the snapshot rule before num_exclude_recent + 1 keyframes: nothing is searched
    int tree_counter = 0, snap_n = 0;            // the handle's snapshot state after these queries: commit_search_locked
};

// detect_intra: the keyframes of this robot before cur - num_exclude_recent
template <class H> int intra_sets_locked(const H *h, const std::string &call, const int *curs, int count, NnSearch *s)
{
    const std::vector<int> &mine = h->reg.keys_of(h->cfg.this_id);
    for (int i = 0; i < count; ++i)
        if (curs[i] < 0 || curs[i] >= (int)mine.size()) return fail(h, SCL_ERR_OUT_OF_RANGE, (call + ": no such keyframe of this robot").c_str());
    for (int i = 0; i < count; ++i) {
        s->qkey[(size_t)i] = mine[(size_t)curs[i]];
        s->limit[(size_t)i] = std::max(0, curs[i] - h->cfg.num_exclude_recent);
    }
    s->lists[0] = {mine.data(), (int)mine.size()};                     // ascending keys: position = local index
    return SCL_OK;
}

// detect_inter by M2DP's rule (inter_mode 1 of FPFH and GRSD): a keyframe of this robot searches the sorted keys of every other
// robot, a received keyframe searches this robot's
template <class H> void inter_lists_sets_locked(const H *h, const int *curs, int count, NnSearch *s)
{
    const std::vector<int> &mine = h->reg.keys_of(h->cfg.this_id);
    for (int r = 0; r < h->reg.robot_num; ++r)
        if (r != h->cfg.this_id) s->others.insert(s->others.end(), h->reg.keys_of(r).begin(), h->reg.keys_of(r).end());
    std::sort(s->others.begin(), s->others.end());                     // ties go to the lowest key
    s->lists[0] = {s->others.data(), (int)s->others.size()};
    s->lists[1] = {mine.data(), (int)mine.size()};
    for (int i = 0; i < count; ++i) {
        s->which[(size_t)i] = h->reg.robots[(size_t)curs[i]] == h->cfg.this_id ? 0 : 1;
        s->limit[(size_t)i] = s->lists[s->which[(size_t)i]].n;
    }
}

// detect_inter of the reference (inter_mode 0 of FPFH and GRSD; FPFH: D.h:381-428, GRSD: D.h:116-167), the handle's tree_counter
// and snap_n walked as `count` single calls in order would: before num_exclude_recent + 1 keyframes nothing is searched and the
// counter stays; else the snapshot [0, snap_n) is retaken when tree_counter % tree_making_period == 0 and the counter advances
template <class H> void inter_snapshot_sets_locked(const H *h, int count, NnSearch *s)
{
    if ((s->too_few = h->reg.n < h->cfg.num_exclude_recent + 1)) return;
    for (int i = 0; i < count; ++i) {
        if (s->tree_counter % h->snapshot_period() == 0) s->snap_n = h->reg.n - h->cfg.num_exclude_recent;
        s->tree_counter += 1;
        s->limit[(size_t)i] = s->snap_n;
    }
    s->lists[0] = {nullptr, h->reg.n};
}

// the search sets of `call` (detect_intra / detect_inter, or their _topk forms: the messages' prefix) for curs[0 .. count): every
// cur is validated before anything runs
template <class H> int search_sets_locked(const H *h, bool intra, const std::string &call, const int *curs, int count, NnSearch *s)
{
    s->qkey = std::vector<int>((size_t)count);
    std::copy_n(curs, count, s->qkey.begin());                         // inter: a cur is a global key
    s->limit.assign((size_t)count, 0);
    s->which.assign((size_t)count, 0);
    s->tree_counter = h->tree_counter; s->snap_n = h->snap_n;
    if (intra) return intra_sets_locked(h, call, curs, count, s);
    for (int i = 0; i < count; ++i)
        if (curs[i] < 0 || curs[i] >= h->reg.n) return fail(h, SCL_ERR_OUT_OF_RANGE, (call + ": key out of range").c_str());
    if (h->inter_snapshot()) inter_snapshot_sets_locked(h, count, s);
    else inter_lists_sets_locked(h, curs, count, s);
    return SCL_OK;
}

// the snapshot rule's state after the queries of `s`; the other rules leave it as it was
template <class H> void commit_search_locked(H *h, const NnSearch &s) { h->tree_counter = s.tree_counter; h->snap_n = s.snap_n; }

// the detections' answers from the search results, as the single calls give them: nothing searched -> (-1, +inf); every distance
// NaN -> (-1, that NaN); else the reported distance, and the loop (the position for intra, the key for inter) when it is below
// dist_thres, compared in double.  dists may be null
template <class H> void report_many(const H *h, const NnManyResult *res, int count, bool local_ids, int *loop_ids, float *dists)
{
    for (int i = 0; i < count; ++i) {
        const NnManyResult &r = res[i];
        int loop = -1;
        float d = INFINITY;
        if (r.pos >= 0) {
            if (std::isnan(r.d2)) d = r.d2;
            else {
                d = r.dist;
                if ((double)d < h->cfg.dist_thres) loop = local_ids ? r.pos : r.key;
            }
        }
        loop_ids[i] = loop;
        if (dists) dists[i] = d;
    }
}

// detect_intra / detect_inter for curs[0 .. count) in one batched search.  The snapshot rule's state is committed on success only;
// where it searches nothing it answers (-1, 0)
template <class H> int detect_many_locked(H *h, bool intra, const int *curs, int count, int *loop_ids, float *dists)
{
    NnSearch s;
    int rc = search_sets_locked(h, intra, intra ? "detect_intra" : "detect_inter", curs, count, &s);
    if (rc) return rc;
    if (s.too_few) {
        for (int i = 0; i < count; ++i) { loop_ids[i] = -1; if (dists) dists[i] = 0.0f; }
        return SCL_OK;
    }
    std::vector<NnManyResult> res((size_t)count);
    if ((rc = nearest_many_locked(h, s.qkey.data(), s.limit.data(), s.which.data(), s.lists, count, h->report_dims(), res.data()))) return rc;
    commit_search_locked(h, s);
    report_many(h, res.data(), count, intra, loop_ids, dists);
    return SCL_OK;
}

// the lists from the search results: the listed candidates first (the position for intra, the key for inter; the reported distance),
// then (-1, +inf) up to k; dist_thres is not applied.  cand_dists and n_found may be null
inline void report_topk(const NnTopkEntry *res, int count, int k, bool local_ids, int *cand_ids, float *cand_dists, int *n_found)
{
    for (int i = 0; i < count; ++i) {
        int found = 0;
        for (int j = 0; j < k; ++j) {
            const NnTopkEntry &r = res[(size_t)i * k + j];
            found += r.pos >= 0;
            cand_ids[(size_t)i * k + j] = local_ids ? r.pos : r.key;
            if (cand_dists) cand_dists[(size_t)i * k + j] = r.pos >= 0 ? r.dist : INFINITY;
        }
        if (n_found) n_found[i] = found;
    }
}

// the candidate lists of detect_intra / detect_inter for curs[0 .. count): the search sets of detect_many_locked, a bad k refused
// before curs is looked at.  The snapshot rule's state is committed on success only; where it searches nothing every list is empty
template <class H>
int detect_topk_locked(H *h, bool intra, const int *curs, int count, int k, int *cand_ids, float *cand_dists, int *n_found)
{
    const std::string call = intra ? "detect_intra_topk" : "detect_inter_topk";
    if (k < 1 || k > kTopkMax) return fail(h, SCL_ERR_INVALID_ARG, (call + ": k outside [1, SCL_PLUGIN_TOPK_MAX]").c_str());
    NnSearch s;
    int rc = search_sets_locked(h, intra, call, curs, count, &s);
    if (rc) return rc;
    std::vector<NnTopkEntry> res((size_t)count * k);
    if (s.too_few) std::fill(res.begin(), res.end(), NnTopkEntry{-1, -1, INFINITY});
    else {
        if ((rc = nearest_topk_many_locked(h, s.qkey.data(), s.limit.data(), s.which.data(), s.lists, count, k, h->report_dims(), res.data()))) return rc;
        commit_search_locked(h, s);
    }
    report_topk(res.data(), count, k, intra, cand_ids, cand_dists, n_found);
    return SCL_OK;
}

// save_from_wire for `count` rows: every robot id validated, the database grown once, the rows copied in one transfer, then committed
template <class H> int save_from_wire_many_locked(H *h, const float *values, const int8_t *robots, const int *indexs, int count)
{
    constexpr int DIM = decltype(h->db)::kDim;
    for (int i = 0; i < count; ++i)
        if (int rc = check_robot(h, robots[i], SCL_ERR_INVALID_ARG)) return rc;
    if (count == 0) return SCL_OK;
    int rc = h->db.grow(h, h->reg.n + count);
    if (rc) return rc;
    SCL_HIP(h, hipMemcpyAsync(h->db.row(h->reg.n), values, sizeof(float) * DIM * (size_t)count, hipMemcpyHostToDevice, h->stream));
    SCL_HIP(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < count; ++i) h->reg.commit(robots[i], indexs[i]);
    return SCL_OK;
}

// make_and_save_many, then on the same stream the intra detection of every new keyframe of this robot; entries of other robots
// answer (-1, +inf).  An invalid cloud: nothing stored, nothing detected, the outputs untouched
template <class H>
int make_save_and_detect_locked(H *h, const void *const *clouds, const int *n_points, int stride, const int8_t *robots, const int *indexs,
                                int count, int *loop_ids, float *dists, float *out_values)
{
    const int first = (int)h->reg.keys_of(h->cfg.this_id).size();
    int rc = make_and_save_many_locked(h, clouds, n_points, stride, robots, indexs, count, out_values);
    if (rc) return rc;
    std::vector<int> curs, at;
    for (int i = 0; i < count; ++i)
        if (robots[i] == h->cfg.this_id) { curs.push_back(first + (int)curs.size()); at.push_back(i); }
    std::vector<int> loops(curs.size());
    std::vector<float> ds(curs.size());
    if ((rc = detect_many_locked(h, true, curs.data(), (int)curs.size(), loops.data(), ds.data()))) return rc;
    for (int i = 0; i < count; ++i) { loop_ids[i] = -1; if (dists) dists[i] = INFINITY; }
    for (size_t j = 0; j < at.size(); ++j) { loop_ids[at[j]] = loops[j]; if (dists) dists[at[j]] = ds[j]; }
    return SCL_OK;
}

// ---- the vector plugins' C entry points, written once: SCL_VECTOR_PLUGIN_ENTRY_POINTS(scl_X) below forwards scl_X_<name> to
// <name> here.  Each is the argument check, the handle's lock with its device made current, and the body

// a call on a handle: its lock held and its device current for the scope
template <class H> struct Entered {
    std::lock_guard<std::mutex> lk;
    explicit Entered(const H *h) : lk(h->mu) { (void)hipSetDevice(h->device); }
};

// the common half of destroy: the stream drained, the plugin's own device buffers (`own`) and the base's freed, the handle deleted
template <class H> int close_plugin(H *h, std::initializer_list<void *> own)
{
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (void *p : own)
        if (p) (void)hipFree(p);
    for (void *p : {(void *)h->db.d_db, (void *)h->d_best, (void *)h->d_list})
        if (p) (void)hipFree(p);
    h->many.release();
    h->topk.release();
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return SCL_OK;
}

// the common half of create, after the plugin's own config checks: the shared checks, the device, then a new handle with its config,
// registry, stream, events, d_best and a database of one row.  On an error nothing is left behind
template <class H, class C> int open_plugin(const C *cfg, H **out)
{
    *out = nullptr;
    if (cfg->robot_num < 1 || cfg->robot_num > 127 || cfg->this_id < 0 || cfg->this_id >= cfg->robot_num || cfg->num_exclude_recent < 0 ||
        !(cfg->dist_thres == cfg->dist_thres))
        return SCL_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SCL_ERR_NO_DEVICE;
    if (cfg->device < 0 || cfg->device >= ndev) return SCL_ERR_INVALID_ARG;
    H *h = new (std::nothrow) H();
    if (!h) return SCL_ERR_NOMEM;
    h->cfg = *cfg; h->device = cfg->device;
    h->reg.init(cfg->robot_num);
    int rc = SCL_OK;
    if (hipSetDevice(h->device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess)
        rc = SCL_ERR_HIP;
    else if (!(rc = dev_alloc(h, &h->d_best, 1)))
        rc = h->db.grow(h, 1);
    if (rc) { close_plugin(h, {}); return rc; }
    *out = h;
    return SCL_OK;
}

template <class H> const char *last_error(const H *h) { return h ? h->last_error.c_str() : "null handle"; }

template <class H> int make(H *h, const void *points, int n_points, int stride, float *out_values)
{
    if (!h || !out_values) return SCL_ERR_INVALID_ARG;
    Entered<H> in(h);
    int rc = run_single_locked(h, points, n_points, stride);
    return rc ? rc : h->db.read(h, h->reg.n, 1, out_values);
}

template <class H>
int make_and_save_many(H *h, const void *const *clouds, const int *n_points, int stride, const int8_t *robots, const int *indexs, int count,
                       float *out_values)
{
    if (!h || count < 0 || (count > 0 && (!clouds || !n_points || !robots || !indexs))) return SCL_ERR_INVALID_ARG;
    Entered<H> in(h);
    return make_and_save_many_locked(h, clouds, n_points, stride, robots, indexs, count, out_values);
}

template <class H> int save_from_wire(H *h, const float *values, int8_t robot, int index)
{
    if (!h || !values) return SCL_ERR_INVALID_ARG;
    Entered<H> in(h);
    int rc;
    if ((rc = check_robot(h, robot, SCL_ERR_INVALID_ARG)) || (rc = h->db.grow(h, h->reg.n + 1)) || (rc = h->db.write(h, h->reg.n, values))) return rc;
    h->reg.commit(robot, index);
    return SCL_OK;
}

template <class H> int save_from_wire_many(H *h, const float *values, const int8_t *robots, const int *indexs, int count)
{
    if (!h || count < 0 || (count > 0 && (!values || !robots || !indexs))) return SCL_ERR_INVALID_ARG;
    Entered<H> in(h);
    return save_from_wire_many_locked(h, values, robots, indexs, count);
}

template <class H> int get_signature(H *h, int key, float *values)
{
    if (!h || !values) return SCL_ERR_INVALID_ARG;
    Entered<H> in(h);
    if (key < 0 || key >= h->reg.n) return fail(h, SCL_ERR_OUT_OF_RANGE, "key out of range");
    return h->db.read(h, key, 1, values);
}

// a single detection's answer by report_many's rule.  *loop_id = -1 and *dist = +inf on entry (nothing searched); the winner of row
// `q` is row `key` at squared distance d2 and would be reported as `loop`: a NaN d2 -> (-1, that NaN), else the reported distance,
// and the loop when it is below dist_thres, compared in double
template <class H> int report_one_locked(H *h, int q, int key, int loop, float d2, int *loop_id, float *dist)
{
    if (std::isnan(d2)) { if (dist) *dist = d2; return SCL_OK; }          // every distance NaN: nothing is nearest
    float d;
    int rc = h->reported_distance(q, key, d2, &d);
    if (rc) return rc;
    if (dist) *dist = d;
    if ((double)d < h->cfg.dist_thres) *loop_id = loop;
    return SCL_OK;
}

// detect_intra / detect_inter of one keyframe: the search set of search_sets_locked for it, searched by nn_l2_kernel.  The snapshot
// rule's counter advances before the search, as the reference's does
template <class H> int detect_one(H *h, bool intra, int cur, int *loop_id, float *dist)
{
    if (!h || !loop_id) return SCL_ERR_INVALID_ARG;
    Entered<H> in(h);
    *loop_id = -1;
    if (dist) *dist = INFINITY;
    NnSearch s;
    int rc = search_sets_locked(h, intra, intra ? "detect_intra" : "detect_inter", &cur, 1, &s);
    if (rc) return rc;
    if (s.too_few) { if (dist) *dist = 0.0f; return SCL_OK; }
    commit_search_locked(h, s);
    const NnList &list = s.lists[s.which[0]];
    int pos;
    float d2;
    if ((rc = nearest_locked(h, s.qkey[0], list.keys, s.limit[0], &pos, &d2)) || pos < 0) return rc;
    const int key = list.keys ? list.keys[pos] : pos;
    return report_one_locked(h, s.qkey[0], key, intra ? pos : key, d2, loop_id, dist);
}

template <class H> int detect_many(H *h, bool intra, const int *curs, int count, int *loop_ids, float *dists)
{
    if (!h || count < 0 || (count > 0 && (!curs || !loop_ids))) return SCL_ERR_INVALID_ARG;
    Entered<H> in(h);
    return detect_many_locked(h, intra, curs, count, loop_ids, dists);
}

template <class H> int detect_topk(H *h, bool intra, const int *curs, int count, int k, int *cand_ids, float *cand_dists, int *n_found)
{
    if (!h || count < 0 || (count > 0 && (!curs || !cand_ids))) return SCL_ERR_INVALID_ARG;
    Entered<H> in(h);
    return detect_topk_locked(h, intra, curs, count, k, cand_ids, cand_dists, n_found);
}

template <class H>
int make_save_and_detect(H *h, const void *const *clouds, const int *n_points, int stride, const int8_t *robots, const int *indexs, int count,
                         int *loop_ids, float *dists, float *out_values)
{
    if (!h || count < 0 || (count > 0 && (!clouds || !n_points || !robots || !indexs || !loop_ids))) return SCL_ERR_INVALID_ARG;
    Entered<H> in(h);
    return make_save_and_detect_locked(h, clouds, n_points, stride, robots, indexs, count, loop_ids, dists, out_values);
}

}  // namespace
}  // namespace scl

// The extern "C" definitions of a vector plugin whose handle type and prefix are P, the counterpart of the declarations in scl_P.h
// and of SCL_PLUGIN_BATCH_API / SCL_PLUGIN_TOPK_API: every one a forward to its template above.  default_config, create, destroy,
// stats and the test hooks stay in the plugin's own file
#define SCL_VECTOR_PLUGIN_ENTRY_POINTS(P)                                                                                              \
    extern "C" {                                                                                                                       \
    const char *P##_last_error(const P *h) { return scl::last_error(h); }                                                              \
    int P##_make(P *h, const void *points, int n_points, int stride_bytes, float *out_values)                                          \
    { return scl::make(h, points, n_points, stride_bytes, out_values); }                                                               \
    int P##_make_and_save_many(P *h, const void *const *clouds, const int *n_points, int stride_bytes, const int8_t *robots,           \
                               const int *indexs, int count, float *out_values)                                                        \
    { return scl::make_and_save_many(h, clouds, n_points, stride_bytes, robots, indexs, count, out_values); }                          \
    int P##_make_and_save(P *h, const void *points, int n_points, int stride_bytes, int8_t robot, int index, float *out_values)        \
    { return scl::make_and_save_many(h, &points, &n_points, stride_bytes, &robot, &index, 1, out_values); }                            \
    int P##_save_from_wire(P *h, const float *values, int8_t robot, int index)                                                         \
    { return scl::save_from_wire(h, values, robot, index); }                                                                           \
    int P##_save_from_wire_many(P *h, const float *values, const int8_t *robots, const int *indexs, int count)                         \
    { return scl::save_from_wire_many(h, values, robots, indexs, count); }                                                             \
    int P##_get_size(const P *h) { return scl::get_size(h); }                                                                          \
    int P##_get_size_of(const P *h, int id) { return scl::get_size_of(h, id); }                                                        \
    int P##_get_index(const P *h, int key, int8_t *robot, int *index) { return scl::get_index(h, key, robot, index); }                 \
    int P##_local_to_global(const P *h, int robot, int local, int *key) { return scl::local_to_global(h, robot, local, key); }         \
    int P##_get_signature(P *h, int key, float *values) { return scl::get_signature(h, key, values); }                                 \
    int P##_detect_intra(P *h, int cur, int *loop_id, float *dist) { return scl::detect_one(h, true, cur, loop_id, dist); }                 \
    int P##_detect_inter(P *h, int cur, int *loop_id, float *dist) { return scl::detect_one(h, false, cur, loop_id, dist); }                \
    int P##_detect_intra_many(P *h, const int *curs, int count, int *loop_ids, float *dists)                                           \
    { return scl::detect_many(h, true, curs, count, loop_ids, dists); }                                                                 \
    int P##_detect_inter_many(P *h, const int *curs, int count, int *loop_ids, float *dists)                                           \
    { return scl::detect_many(h, false, curs, count, loop_ids, dists); }                                                                \
    int P##_detect_intra_topk(P *h, const int *curs, int count, int k, int *cand_ids, float *cand_dists, int *n_found)                 \
    { return scl::detect_topk(h, true, curs, count, k, cand_ids, cand_dists, n_found); }                                                \
    int P##_detect_inter_topk(P *h, const int *curs, int count, int k, int *cand_ids, float *cand_dists, int *n_found)                 \
    { return scl::detect_topk(h, false, curs, count, k, cand_ids, cand_dists, n_found); }                                               \
    int P##_make_save_and_detect(P *h, const void *const *clouds, const int *n_points, int stride_bytes, const int8_t *robots,         \
                                 const int *indexs, int count, int *loop_ids, float *dists, float *out_values)                         \
    { return scl::make_save_and_detect(h, clouds, n_points, stride_bytes, robots, indexs, count, loop_ids, dists, out_values); }       \
    }
