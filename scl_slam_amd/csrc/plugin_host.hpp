// plugin_host.hpp -- the host layer the descriptor plugins share (iris.hip, m2dp.hip, fpfh.hip, grsd.hip; engine.hip and sharded_front.hip
// take the error helpers): the HIP-check macro and error helpers, the keyframe registry behind the get_size / get_index / local_to_global
// entry points and the inter-detection candidate rule, and for the vector plugins (M2DP, FPFH, GRSD) the float-row database, the
// make_and_save_many driver and the 1-NN search.  No descriptor logic lives here.
//
// Every helper that touches a handle assumes its lock is held (the `_locked` convention; std::mutex is not recursive), except
// the registry's C entry points below, which take it once.  A handle provides `mutable std::mutex mu`, `mutable std::string
// last_error`, `hipStream_t stream` and `scl::KeyframeRegistry reg`; a vector plugin's also `scl::FloatRows<DIM> db`,
// `int *d_list`, `size_t list_cap` and `unsigned long long *d_best` (one element).
// Included from .hip files only (nn_l2_kernel is device code).  Everything here has internal linkage (the unnamed namespace): the
// library exports its C ABI and nothing of this layer.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "scl_engine.h"

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

// make_and_save_many of a vector plugin: every cloud (check(h, points, n_points, stride)) and robot id validated first, then
// launch groups of up to max_group clouds into rows n .. n + count - 1 (run(clouds, n_points, G, slot0, &bad)); the first
// group with a non-finite coordinate ends the call, and nothing of the call is committed
template <class H, class Check, class Run>
int make_and_save_many_locked(H *h, const void *const *clouds, const int *n_points, int stride, const int8_t *robots,
                              const int *indexs, int count, float *out_values, int max_group, Check check, Run run)
{
    for (int i = 0; i < count; ++i) {
        int rc = check(h, clouds[i], n_points[i], stride);
        if (rc) return rc;
        if ((rc = check_robot(h, robots[i], SCL_ERR_INVALID_ARG))) return rc;
    }
    if (count == 0) return SCL_OK;
    int rc = h->db.grow(h, h->reg.n + count);
    if (rc) return rc;
    for (int s = 0; s < count; s += max_group) {
        const int G = std::min(max_group, count - s);
        int bad = 0;
        if ((rc = run(clouds + s, n_points + s, G, h->reg.n + s, &bad))) return rc;
        if (bad) return fail(h, SCL_ERR_INVALID_ARG, "non-finite coordinate: nothing of the call was stored");
    }
    if (out_values && (rc = h->db.read(h, h->reg.n, count, out_values))) return rc;
    for (int i = 0; i < count; ++i) h->reg.commit(robots[i], indexs[i]);
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
    if (list && (size_t)n > h->list_cap) {
        h->list_cap = 0;
        const size_t c = (size_t)n + (size_t)n / 2 + 256;
        int rc = dev_regrow(h, &h->d_list, c);
        if (rc) return rc;
        h->list_cap = c;
    }
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

}  // namespace
}  // namespace scl
