// global_map.hip -- the persistent global voxel map (include/scl_engine.h "GLOBAL MAP"): an open-addressing hash table of voxels keyed by
// 63-bit lattice coordinates, filled from the on-device keyframe store at fp64 poses.  A voxel's state is four unsigned 64-bit integers
// (count and the sums of the points' 20-bit fractions per axis), changed by integer atomic adds only: exact, order independent and
// exactly invertible, so a keyframe is taken out at its old pose by adding the two's complement of what it added.
//
//   map_prepare_kernel     one thread per job: the pose normalised by se3::normalise_pose
//   map_points_kernel<0>   reserve pass: one thread per point, key found or inserted (64-bit compare-and-swap on the key word); a probe
//                          that runs out of steps, or an insert beyond the load bound, raises bit 63 of the control word; successful
//                          inserts count in its low bits
//   map_points_kernel<1>   add pass: the same point again, its key looked up, four 64-bit atomic adds
//   map_rehash_kernel      one thread per slot of the old table: voxels with n != 0 re-inserted into the new one
//   map_count / compact / key_hi / records kernels: the extraction -- occupied slots (inside the box) compacted, ordered by key with two
//                          stable passes of device_sort.hip (low 32 bits, then the high 31), written as 16-byte records
//
// A slot is one 64-byte line: key, n, Sx, Sy, Sz and three unused words, so the compare-and-swap and the four adds of a point go to
// one line.  The host-only plan (capacity rule, diff of a call, launch groups) is global_map_plan.hpp; the C entry points are at the end.
#include "scl_engine.h"

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "device_sort.hpp"
#include "engine_internal.hpp"
#include "global_map.hpp"
#include "global_map_plan.hpp"
#include "plugin_host.hpp"
#include "se3_device.hpp"

namespace scl {

namespace {

using gmap::kEmptyKey;

struct alignas(64) MapSlot { unsigned long long key, n, sx, sy, sz, pad[3]; };
static_assert(sizeof(MapSlot) == 64, "a slot is one 64-byte line");

struct MapJobDev { const unsigned char *cloud; int n; int sign; double raw[7]; double q[4]; double t[3]; };
struct MapBox { double lo[3], hi[3]; int on; };

enum { C_RESERVE = 0, C_SKIPPED, C_MISS, C_COUNT, C_POS, C_WORDS = 8 };
constexpr unsigned long long kFullBit = 1ULL << 63;
enum { B_JOBS = 0, B_OFFSETS, B_KEYS_A, B_KEYS_B, B_VALS_A, B_VALS_B, B_SCRATCH, B_RECORDS, B_COUNT };
static_assert(B_COUNT <= (int)(sizeof(GlobalMap::buf) / sizeof(void *)), "GlobalMap::buf holds every buffer");

__global__ void map_init_kernel(MapSlot *table, unsigned long long capacity)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= capacity) return;
    MapSlot s{};
    s.key = kEmptyKey;
    table[i] = s;
}

__global__ void map_prepare_kernel(MapJobDev *jobs, int n_jobs)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_jobs) return;
    double o[7];
    se3::normalise_pose(jobs[j].raw, o);
    for (int k = 0; k < 4; ++k) jobs[j].q[k] = o[k];
    for (int k = 0; k < 3; ++k) jobs[j].t[k] = o[4 + k];
}

// the voxel of a stored point under a job's pose: false = skipped (a coordinate not finite after the move, or outside the lattice)
__device__ inline bool voxel_of(const MapJobDev &jb, const float *p, double inv, unsigned long long *key, unsigned long long f[3])
{
    const double v[3] = {(double)p[0], (double)p[1], (double)p[2]};
    double r[3];
    se3::qrot(jb.q, v, r);
    unsigned long long k = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double s = (r[a] + jb.t[a]) * inv;
        const double fl = floor(s);
        if (!(fl >= -1048576.0 && fl < 1048576.0)) return false;          // NaN and the infinities fail it too
        f[a] = (unsigned long long)(unsigned int)floor((s - fl) * 1048576.0);
        k |= (unsigned long long)((long long)fl + gmap::kCoordBias) << (gmap::kCoordBits * a);
    }
    *key = k;
    return true;
}

// One atomic add per wave for a 0 / 1 of every lane: the lane's position in the count (what the counter held before it, plus the set
// lanes below it).  Every insert, kept voxel or compacted record counted on its own made the single counter word the slowest thing in
// its kernel (8.7 M returning adds to one address: 20 ms; DESIGN.md section 4, Global map).  The lanes that call it together form
// the group; which lanes those are changes no result.
__device__ inline unsigned long long wave_count(unsigned long long *counter, bool flag)
{
    const unsigned long long m = __ballot(flag);
    if (m == 0) return 0;
    const int lane = (int)(threadIdx.x & 63), leader = __ffsll((long long)m) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(m));
    base = __shfl(base, leader);
    return base + (unsigned long long)__popcll(m & ((1ULL << lane) - 1ULL));
}

// The slot of `key`, inserted where INSERT says so and the probe meets an empty slot first (*inserted says whether this lane put it
// there); -1: not there within `limit` steps.  A key never moves or leaves, so a stale read can only show an empty slot where there is
// a key by now, and the compare-and-swap settles that.
template <bool INSERT>
__device__ inline long long find_slot(MapSlot *table, unsigned long long mask, int limit, unsigned long long key, bool *inserted)
{
    unsigned long long s = gmap::hash_key(key) & mask;
    for (int step = 0; step < limit; ++step) {
        const unsigned long long k = table[s].key;
        if (k == key) return (long long)s;
        if (k == kEmptyKey) {
            if (!INSERT) return -1;
            const unsigned long long old = atomicCAS(&table[s].key, kEmptyKey, key);
            if (old == kEmptyKey) { *inserted = true; return (long long)s; }
            if (old == key) return (long long)s;
        }
        s = (s + 1) & mask;
    }
    return -1;
}

// A reserve pass's bookkeeping for the lanes that are still here: inserts counted in the control word's low bits; the flag raised by a
// probe that ran out of steps and by the insert that takes the table past its load bound (`room` inserts were left), so that a pass
// into a table that is too small ends early -- its blocks leave when they see the flag -- and never fills the table to the brim.
__device__ inline void reserve_account(unsigned long long *ctl, bool inserted, bool failed, unsigned long long room)
{
    const unsigned long long before = wave_count(&ctl[C_RESERVE], inserted) & ~kFullBit;
    if (failed || (inserted && before >= room)) atomicOr(&ctl[C_RESERVE], kFullBit);
}

template <bool ADD>
__global__ __launch_bounds__(256) void map_points_kernel(const MapJobDev *jobs, const int *offsets, int n_jobs, int n_total, int stride, double inv,
                                                         MapSlot *table, unsigned long long mask, int limit, unsigned long long *ctl, unsigned long long room)
{
    __shared__ int s_off[gmap::kMaxJobs + 1];
    for (int j = threadIdx.x; j <= n_jobs; j += blockDim.x) s_off[j] = j < n_jobs ? offsets[j] : n_total;
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_total) return;
    if (!ADD && (__hip_atomic_load(&ctl[C_RESERVE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kFullBit)) return;   // the table is full: the pass will be run again
    int a = 0, b = n_jobs;                                             // the last job whose offset is <= i (empty jobs share an offset with the next)
    while (b - a > 1) { const int m = (a + b) >> 1; if (s_off[m] <= i) a = m; else b = m; }
    const MapJobDev &jb = jobs[a];
    const float *p = reinterpret_cast<const float *>(jb.cloud + (size_t)(i - s_off[a]) * (size_t)stride);
    unsigned long long key = 0, f[3];
    const unsigned long long sg = jb.sign < 0 ? ~0ULL : 1ULL;          // subtraction = adding the two's complement
    const bool placed = voxel_of(jb, p, inv, &key, f);
    bool inserted = false;
    const long long s = placed ? find_slot<!ADD>(table, mask, limit, key, &inserted) : -1;
    if (!ADD) {
        reserve_account(ctl, inserted, placed && s < 0, room);
        return;
    }
    if (!placed) { atomicAdd(&ctl[C_SKIPPED], sg); return; }
    if (s < 0) { atomicAdd(&ctl[C_MISS], 1ULL); return; }              // cannot happen behind a reserve pass that raised no flag; reported, not dropped
    MapSlot *v = table + s;
    atomicAdd(&v->n, sg);
    atomicAdd(&v->sx, sg * f[0]);
    atomicAdd(&v->sy, sg * f[1]);
    atomicAdd(&v->sz, sg * f[2]);
}

__global__ void map_rehash_kernel(const MapSlot *old_table, unsigned long long old_capacity, MapSlot *table, unsigned long long mask, int limit,
                                  unsigned long long *ctl)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= old_capacity) return;
    const MapSlot o = old_table[i];
    const bool live = o.key != kEmptyKey && o.n != 0;                  // an emptied voxel is not part of the map: it is dropped here
    bool inserted = false;
    const long long s = live ? find_slot<true>(table, mask, limit, o.key, &inserted) : -1;
    reserve_account(ctl, inserted, live && s < 0, ~0ULL);
    if (s < 0) return;
    MapSlot *v = table + s;                                            // the new slot holds zeros and is this key's alone
    atomicAdd(&v->n, o.n); atomicAdd(&v->sx, o.sx); atomicAdd(&v->sy, o.sy); atomicAdd(&v->sz, o.sz);
}

// part of the map (and inside the box): the centroid in double, before it is narrowed
__device__ inline bool slot_kept(const MapSlot &s, const MapBox &box, double leaf, double c[3])
{
    if (s.key == kEmptyKey || s.n == 0) return false;
    const double den = (double)s.n * 1048576.0;
    const unsigned long long sum[3] = {s.sx, s.sy, s.sz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const long long ca = (long long)((s.key >> (gmap::kCoordBits * a)) & ((1ULL << gmap::kCoordBits) - 1)) - gmap::kCoordBias;
        c[a] = ((double)ca + (double)sum[a] / den) * leaf;
        if (box.on && !(c[a] >= box.lo[a] && c[a] <= box.hi[a])) return false;
    }
    return true;
}

__global__ void map_count_kernel(const MapSlot *table, unsigned long long capacity, MapBox box, double leaf, unsigned long long *ctl)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= capacity) return;
    double c[3];
    (void)wave_count(&ctl[C_COUNT], slot_kept(table[i], box, leaf, c));
}

__global__ void map_compact_kernel(const MapSlot *table, unsigned long long capacity, MapBox box, double leaf, unsigned long long *ctl,
                                   unsigned int *key_lo, unsigned int *slot, unsigned long long room)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= capacity) return;
    double c[3];
    const MapSlot s = table[i];
    const bool kept = slot_kept(s, box, leaf, c);
    const unsigned long long pos = wave_count(&ctl[C_POS], kept);
    if (!kept || pos >= room) return;                                  // (pos >= room: the count kernel saw the same table, never taken)
    key_lo[pos] = (unsigned int)s.key;
    slot[pos] = (unsigned int)i;
}

__global__ void map_key_hi_kernel(const MapSlot *table, const unsigned int *slot, unsigned int *key_hi, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) key_hi[i] = (unsigned int)(table[slot[i]].key >> 32);
}

__global__ void map_records_kernel(const MapSlot *table, const unsigned int *slot, int n, double leaf, uint4 *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const MapSlot s = table[slot[i]];
    MapBox none{};
    double c[3] = {0.0, 0.0, 0.0};
    (void)slot_kept(s, none, leaf, c);
    uint4 r;
    r.x = __float_as_uint((float)c[0]); r.y = __float_as_uint((float)c[1]); r.z = __float_as_uint((float)c[2]);
    r.w = s.n > 0xffffffffULL ? 0xffffffffu : (unsigned int)s.n;
    out[i] = r;
}

#define MAP_HIP(call)                                                                                  \
    do {                                                                                               \
        const hipError_t e__ = (call);                                                                 \
        if (e__ != hipSuccess) {                                                                       \
            if (err) *err = std::string("map: ") + #call + ": " + hipGetErrorString(e__);              \
            return e__ == hipErrorOutOfMemory ? SCL_ERR_NOMEM : SCL_ERR_HIP;                           \
        }                                                                                              \
    } while (0)

int map_fail(std::string *err, int code, const char *msg)
{
    if (err) *err = std::string("map: ") + msg;
    return code;
}

int mensure(GlobalMap *m, int k, size_t bytes, std::string *err)
{
    if (bytes <= m->cap[k]) return SCL_OK;
    if (m->buf[k]) { (void)hipFree(m->buf[k]); m->buf[k] = nullptr; m->cap[k] = 0; }
    const size_t want = bytes + bytes / 2 + 256;
    MAP_HIP(hipMalloc(&m->buf[k], want));
    m->cap[k] = want;
    return SCL_OK;
}

inline unsigned int blocks_for(unsigned long long n) { return (unsigned int)((n + 255) / 256); }

int table_alloc(unsigned long long capacity, hipStream_t stream, void **out, std::string *err)
{
    if (capacity > gmap::kMaxSlots) return map_fail(err, SCL_ERR_NOMEM, "the table would exceed 2^31 slots");
    void *t = nullptr;
    MAP_HIP(hipMalloc(&t, (size_t)capacity * sizeof(MapSlot)));
    hipLaunchKernelGGL(map_init_kernel, dim3(blocks_for(capacity)), dim3(256), 0, stream, static_cast<MapSlot *>(t), capacity);
    *out = t;
    return SCL_OK;
}

int controls(GlobalMap *m, std::string *err)
{
    if (!m->d_ctl) MAP_HIP(hipMalloc(reinterpret_cast<void **>(&m->d_ctl), C_WORDS * sizeof(unsigned long long)));
    if (!m->h_ctl) MAP_HIP(hipHostMalloc(reinterpret_cast<void **>(&m->h_ctl), C_WORDS * sizeof(unsigned long long)));
    for (auto &ev : m->ev) if (!ev) MAP_HIP(hipEventCreate(&ev));
    return SCL_OK;
}

// the control words on the host, the stream waited for
int read_controls(GlobalMap *m, hipStream_t stream, std::string *err)
{
    MAP_HIP(hipGetLastError());
    MAP_HIP(hipMemcpyAsync(m->h_ctl, m->d_ctl, C_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    MAP_HIP(hipStreamSynchronize(stream));
    return SCL_OK;
}

// A larger table with the occupied voxels of the old one; the old one is let go only when the new one holds them all
int map_grow(GlobalMap *m, hipStream_t stream, bool timing, std::string *err)
{
    if (timing) MAP_HIP(hipEventRecord(m->ev[2], stream));
    unsigned long long cap = gmap::grown_capacity(m->capacity, m->used_slots);
    for (;;) {
        void *t = nullptr;
        if (int rc = table_alloc(cap, stream, &t, err)) return rc;
        hipError_t e = hipMemsetAsync(m->d_ctl + C_RESERVE, 0, sizeof(unsigned long long), stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(map_rehash_kernel, dim3(blocks_for(m->capacity)), dim3(256), 0, stream, static_cast<const MapSlot *>(m->table), m->capacity,
                               static_cast<MapSlot *>(t), cap - 1, gmap::probe_limit(cap), m->d_ctl);
        }
        const int rc = e == hipSuccess ? read_controls(m, stream, err) : map_fail(err, SCL_ERR_HIP, hipGetErrorString(e));
        if (rc) { (void)hipFree(t); return rc; }
        if (m->h_ctl[C_RESERVE] & kFullBit) { (void)hipFree(t); cap *= 2; continue; }
        (void)hipFree(m->table);
        m->table = t; m->capacity = cap; m->used_slots = m->h_ctl[C_RESERVE]; ++m->growths;
        break;
    }
    if (timing) {
        float ms = 0.0f;
        MAP_HIP(hipEventRecord(m->ev[3], stream));
        MAP_HIP(hipEventSynchronize(m->ev[3]));
        MAP_HIP(hipEventElapsedTime(&ms, m->ev[2], m->ev[3]));
        m->ms[1] += (double)ms;
    }
    return SCL_OK;
}

MapBox make_box(const double *box)
{
    MapBox b{};
    if (box) { for (int a = 0; a < 3; ++a) { b.lo[a] = box[a]; b.hi[a] = box[3 + a]; } b.on = 1; }
    return b;
}

}  // namespace

void map_free(GlobalMap *m)
{
    if (m->table) (void)hipFree(m->table);
    if (m->d_ctl) (void)hipFree(m->d_ctl);
    if (m->h_ctl) (void)hipHostFree(m->h_ctl);
    for (auto &b : m->buf) if (b) (void)hipFree(b);
    for (auto &ev : m->ev) if (ev) (void)hipEventDestroy(ev);
    const unsigned long long hook = m->next_start_slots;
    *m = GlobalMap{};
    m->next_start_slots = hook;
}

int map_reset(GlobalMap *m, hipStream_t stream, float leaf, std::string *err)
{
    if (int rc = controls(m, err)) return rc;
    const unsigned long long cap = gmap::start_capacity(m->next_start_slots);
    void *t = nullptr;
    if (int rc = table_alloc(cap, stream, &t, err)) return rc;
    MAP_HIP(hipGetLastError());
    MAP_HIP(hipStreamSynchronize(stream));
    if (m->table) (void)hipFree(m->table);
    m->table = t; m->capacity = cap; m->used_slots = 0;
    m->points_added = m->points_skipped = m->growths = 0;
    m->entries.clear();
    m->leaf = leaf; m->exists = true;
    m->ms[0] = m->ms[1] = m->ms[2] = 0.0;
    return SCL_OK;
}

int map_apply(GlobalMap *m, hipStream_t stream, const MapPass *passes, int n_passes, int stride, bool timing, std::string *err)
{
    m->ms[0] = m->ms[1] = 0.0;
    if (n_passes <= 0) return SCL_OK;
    const double inv = 1.0 / (double)m->leaf;
    std::vector<int> counts((size_t)n_passes), first, offsets;
    for (int j = 0; j < n_passes; ++j) counts[(size_t)j] = passes[j].n;
    gmap::plan_groups(counts.data(), n_passes, &first, &offsets);
    if (timing) MAP_HIP(hipEventRecord(m->ev[0], stream));
    MAP_HIP(hipMemsetAsync(m->d_ctl, 0, C_WORDS * sizeof(unsigned long long), stream));
    std::vector<MapJobDev> jobs;
    long long signed_points = 0;
    for (size_t g = 0; g + 1 < first.size(); ++g) {
        const int j0 = first[g], nj = first[g + 1] - j0;
        const long long total = (long long)offsets[(size_t)(j0 + nj - 1)] + counts[(size_t)(j0 + nj - 1)];
        for (int j = j0; j < j0 + nj; ++j) signed_points += (long long)passes[j].sign * passes[j].n;
        if (total == 0) continue;
        if (total > (long long)INT_MAX) return map_fail(err, SCL_ERR_INVALID_ARG, "a launch group exceeds 2^31 - 1 points");
        jobs.assign((size_t)nj, MapJobDev{});
        for (int j = 0; j < nj; ++j) {
            MapJobDev &d = jobs[(size_t)j];
            d.cloud = passes[j0 + j].cloud; d.n = passes[j0 + j].n; d.sign = passes[j0 + j].sign;
            std::memcpy(d.raw, passes[j0 + j].pose, sizeof d.raw);
        }
        if (int rc = mensure(m, B_JOBS, sizeof(MapJobDev) * (size_t)nj, err)) return rc;
        if (int rc = mensure(m, B_OFFSETS, sizeof(int) * (size_t)nj, err)) return rc;
        MAP_HIP(hipMemcpyAsync(m->buf[B_JOBS], jobs.data(), sizeof(MapJobDev) * (size_t)nj, hipMemcpyHostToDevice, stream));
        MAP_HIP(hipMemcpyAsync(m->buf[B_OFFSETS], offsets.data() + j0, sizeof(int) * (size_t)nj, hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(map_prepare_kernel, dim3(blocks_for((unsigned long long)nj)), dim3(256), 0, stream, static_cast<MapJobDev *>(m->buf[B_JOBS]), nj);
        const dim3 grid(blocks_for((unsigned long long)total));
        for (;;) {                                                     // phase 1: every key of the group gets its slot; repeated on a larger table as needed
            MAP_HIP(hipMemsetAsync(m->d_ctl + C_RESERVE, 0, sizeof(unsigned long long), stream));
            hipLaunchKernelGGL(map_points_kernel<false>, grid, dim3(256), 0, stream, static_cast<const MapJobDev *>(m->buf[B_JOBS]),
                               static_cast<const int *>(m->buf[B_OFFSETS]), nj, (int)total, stride, inv, static_cast<MapSlot *>(m->table), m->capacity - 1,
                               gmap::probe_limit(m->capacity), m->d_ctl, gmap::room(m->used_slots, m->capacity));
            if (int rc = read_controls(m, stream, err)) return rc;
            const unsigned long long word = m->h_ctl[C_RESERVE];
            m->used_slots += word & ~kFullBit;
            if (!(word & kFullBit) && !gmap::over_load(m->used_slots, m->capacity)) break;
            if (int rc = map_grow(m, stream, timing, err)) return rc;
        }
        // phase 2: the adds
        hipLaunchKernelGGL(map_points_kernel<true>, grid, dim3(256), 0, stream, static_cast<const MapJobDev *>(m->buf[B_JOBS]),
                           static_cast<const int *>(m->buf[B_OFFSETS]), nj, (int)total, stride, inv, static_cast<MapSlot *>(m->table), m->capacity - 1,
                           gmap::probe_limit(m->capacity), m->d_ctl, ~0ULL);
        MAP_HIP(hipGetLastError());
        MAP_HIP(hipStreamSynchronize(stream));                         // `jobs` is reused by the next group
    }
    if (timing) MAP_HIP(hipEventRecord(m->ev[1], stream));
    if (int rc = read_controls(m, stream, err)) return rc;
    if (m->h_ctl[C_MISS]) return map_fail(err, SCL_ERR_HIP, "a reserved key was not found by the add pass");
    const unsigned long long skipped = m->h_ctl[C_SKIPPED];            // two's complement of the net change
    m->points_skipped += skipped;
    m->points_added += (unsigned long long)signed_points - skipped;
    if (timing) {
        float ms = 0.0f;
        MAP_HIP(hipEventElapsedTime(&ms, m->ev[0], m->ev[1]));
        m->ms[0] = (double)ms - m->ms[1];
    }
    return SCL_OK;
}

int map_count(GlobalMap *m, hipStream_t stream, unsigned long long *occupied, std::string *err)
{
    MAP_HIP(hipMemsetAsync(m->d_ctl + C_COUNT, 0, 2 * sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(map_count_kernel, dim3(blocks_for(m->capacity)), dim3(256), 0, stream, static_cast<const MapSlot *>(m->table), m->capacity, make_box(nullptr),
                       (double)m->leaf, m->d_ctl);
    if (int rc = read_controls(m, stream, err)) return rc;
    *occupied = m->h_ctl[C_COUNT];
    return SCL_OK;
}

int map_extract(GlobalMap *m, hipStream_t stream, const double *box, void *out, int out_capacity, int *n_out, bool timing, std::string *err)
{
    m->ms[2] = 0.0;
    const MapBox bx = make_box(box);
    const MapSlot *table = static_cast<const MapSlot *>(m->table);
    const double leaf = (double)m->leaf;
    if (timing) MAP_HIP(hipEventRecord(m->ev[0], stream));
    MAP_HIP(hipMemsetAsync(m->d_ctl + C_COUNT, 0, 2 * sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(map_count_kernel, dim3(blocks_for(m->capacity)), dim3(256), 0, stream, table, m->capacity, bx, leaf, m->d_ctl);
    if (int rc = read_controls(m, stream, err)) return rc;
    const unsigned long long count = m->h_ctl[C_COUNT];
    if (count > (unsigned long long)INT_MAX) return map_fail(err, SCL_ERR_OUT_OF_RANGE, "more than 2^31 - 1 voxels: extract a box");
    if (out && count > (unsigned long long)(out_capacity > 0 ? out_capacity : 0)) return map_fail(err, SCL_ERR_INVALID_ARG, "map_extract: output capacity too small");
    const int n = (int)count;
    if (out && n > 0) {
        const size_t words = sizeof(unsigned int) * (size_t)n;
        for (int k : {B_KEYS_A, B_KEYS_B, B_VALS_A, B_VALS_B}) if (int rc = mensure(m, k, words, err)) return rc;
        if (int rc = mensure(m, B_SCRATCH, sort_scratch_bytes((size_t)n, 1), err)) return rc;
        if (int rc = mensure(m, B_RECORDS, 16 * (size_t)n, err)) return rc;
        unsigned int *ka = static_cast<unsigned int *>(m->buf[B_KEYS_A]), *kb = static_cast<unsigned int *>(m->buf[B_KEYS_B]);
        unsigned int *va = static_cast<unsigned int *>(m->buf[B_VALS_A]), *vb = static_cast<unsigned int *>(m->buf[B_VALS_B]);
        hipLaunchKernelGGL(map_compact_kernel, dim3(blocks_for(m->capacity)), dim3(256), 0, stream, table, m->capacity, bx, leaf, m->d_ctl, ka, va, count);
        // ascending key: the low 32 bits, then -- stable -- the high 31
        MAP_HIP(sort_pairs_u32(m->buf[B_SCRATCH], ka, kb, va, vb, n, 32, stream));
        hipLaunchKernelGGL(map_key_hi_kernel, dim3(blocks_for(count)), dim3(256), 0, stream, table, (const unsigned int *)vb, ka, n);
        MAP_HIP(sort_pairs_u32(m->buf[B_SCRATCH], ka, kb, vb, va, n, 31, stream));
        hipLaunchKernelGGL(map_records_kernel, dim3(blocks_for(count)), dim3(256), 0, stream, table, (const unsigned int *)va, n, leaf,
                           static_cast<uint4 *>(m->buf[B_RECORDS]));
        MAP_HIP(hipGetLastError());
        MAP_HIP(hipMemcpyAsync(out, m->buf[B_RECORDS], 16 * (size_t)n, hipMemcpyDeviceToHost, stream));
    }
    if (timing) MAP_HIP(hipEventRecord(m->ev[1], stream));
    MAP_HIP(hipStreamSynchronize(stream));
    if (timing) {
        float ms = 0.0f;
        MAP_HIP(hipEventElapsedTime(&ms, m->ev[0], m->ev[1]));
        m->ms[2] = (double)ms;
    }
    *n_out = n;
    return SCL_OK;
}

}  // namespace scl

/* ---- the C entry points (include/scl_engine.h "GLOBAL MAP") ------------------------------------------------------------------- */

using namespace scl;

namespace {

// the primary shard does the work; its message goes to the handle the caller holds
template <class Call> int map_call(scl_engine *e, Call call)
{
    if (!e) return SCL_ERR_INVALID_ARG;
    if (e->front) {
        scl_engine *p = front_primary(e);
        const int rc = map_call(p, call);
        if (rc) e->last_error = scl_last_error(p);
        return rc;
    }
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    return call(e);
}

// the listed keyframes' clouds in the store: nullptr, or what is wrong
const char *listed_clouds(const scl_engine *e, const int *robots, const int *indices, int n, std::vector<const scl_engine::StoredCloud *> *out,
                          std::vector<uint64_t> *generations)
{
    for (int i = 0; i < n; ++i) {
        const int r = robots[i], x = indices[i];
        if (r < 0 || x < 0 || (size_t)r >= e->kf.size() || (size_t)x >= e->kf[(size_t)r].size() || e->kf[(size_t)r][(size_t)x].n < 0)
            return "a listed keyframe is not in the store";
        out->push_back(&e->kf[(size_t)r][(size_t)x]);
        generations->push_back(e->kf[(size_t)r][(size_t)x].generation);
    }
    return nullptr;
}

int apply_jobs(scl_engine *e, const std::vector<gmap::Job> &jobs, const std::vector<const scl_engine::StoredCloud *> &clouds)
{
    std::vector<MapPass> passes;
    passes.reserve(jobs.size());
    for (const gmap::Job &j : jobs) {
        const auto *c = clouds[(size_t)j.item];
        MapPass p{c->d, c->n, j.sign, {0}};
        std::memcpy(p.pose, j.pose, sizeof p.pose);
        passes.push_back(p);
    }
    std::string err;
    const int rc = map_apply(&e->gmap, e->stream, passes.data(), (int)passes.size(), e->kf_stride ? e->kf_stride : 16, e->prof_on == 1, &err);
    if (rc) {                                                          // a device failure half way: what the groups before it added stays added
        e->gmap.exists = false;
        e->last_error = err + " (the map is no longer valid: scl_map_reset)";
    }
    return rc;
}

}  // namespace

int scl_map_reset(scl_engine *e, float leaf)
{
    return map_call(e, [&](scl_engine *pe) {
        if (!std::isfinite(leaf) || !(leaf > 0.0f)) return fail(pe, SCL_ERR_INVALID_ARG, "map_reset: leaf must be finite and > 0");
        std::string err;
        const int rc = map_reset(&pe->gmap, pe->stream, leaf, &err);
        if (rc) pe->last_error = err;
        return rc;
    });
}

int scl_map_set_keyframes(scl_engine *e, const int *robots, const int *indices, const double *poses, int n)
{
    return map_call(e, [&](scl_engine *pe) {
        if (n < 0) return fail(pe, SCL_ERR_INVALID_ARG, "map_set_keyframes: n < 0");
        if (n > 0 && (!robots || !indices || !poses)) return fail(pe, SCL_ERR_INVALID_ARG, "map_set_keyframes: robots, indices or poses is NULL");
        if (!pe->gmap.exists) return fail(pe, SCL_ERR_INVALID_ARG, "map_set_keyframes: no map yet (scl_map_reset)");
        std::vector<const scl_engine::StoredCloud *> clouds; std::vector<uint64_t> gens;
        if (const char *bad = listed_clouds(pe, robots, indices, n, &clouds, &gens)) return fail(pe, SCL_ERR_INVALID_ARG, (std::string("map_set_keyframes: ") + bad).c_str());
        std::vector<int> actions; std::vector<gmap::Job> jobs;
        if (const char *bad = gmap::plan_set(pe->gmap.entries, robots, indices, poses, gens.data(), n, &actions, &jobs))
            return fail(pe, SCL_ERR_INVALID_ARG, (std::string("map_set_keyframes: ") + bad).c_str());
        if (int rc = apply_jobs(pe, jobs, clouds)) return rc;
        for (int i = 0; i < n; ++i) {
            if (actions[(size_t)i] == gmap::kSkip) continue;
            gmap::Entry en{};
            std::memcpy(en.pose, poses + 7 * (size_t)i, sizeof en.pose);
            en.generation = gens[(size_t)i];
            pe->gmap.entries[{robots[i], indices[i]}] = en;
        }
        return (int)SCL_OK;
    });
}

int scl_map_remove_keyframes(scl_engine *e, const int *robots, const int *indices, int n)
{
    return map_call(e, [&](scl_engine *pe) {
        if (n < 0) return fail(pe, SCL_ERR_INVALID_ARG, "map_remove_keyframes: n < 0");
        if (n > 0 && (!robots || !indices)) return fail(pe, SCL_ERR_INVALID_ARG, "map_remove_keyframes: robots or indices is NULL");
        if (!pe->gmap.exists) return fail(pe, SCL_ERR_INVALID_ARG, "map_remove_keyframes: no map yet (scl_map_reset)");
        std::vector<const scl_engine::StoredCloud *> clouds; std::vector<uint64_t> gens;
        if (const char *bad = listed_clouds(pe, robots, indices, n, &clouds, &gens)) return fail(pe, SCL_ERR_INVALID_ARG, (std::string("map_remove_keyframes: ") + bad).c_str());
        std::vector<gmap::Job> jobs;
        if (const char *bad = gmap::plan_remove(pe->gmap.entries, robots, indices, gens.data(), n, &jobs))
            return fail(pe, SCL_ERR_INVALID_ARG, (std::string("map_remove_keyframes: ") + bad).c_str());
        if (int rc = apply_jobs(pe, jobs, clouds)) return rc;
        for (int i = 0; i < n; ++i) pe->gmap.entries.erase({robots[i], indices[i]});
        return (int)SCL_OK;
    });
}

int scl_map_extract(scl_engine *e, const double *box, void *out, int out_capacity, int *n_out)
{
    return map_call(e, [&](scl_engine *pe) {
        if (!n_out) return fail(pe, SCL_ERR_INVALID_ARG, "map_extract: n_out is NULL");
        if (!pe->gmap.exists) return fail(pe, SCL_ERR_INVALID_ARG, "map_extract: no map yet (scl_map_reset)");
        if (out && out_capacity < 0) return fail(pe, SCL_ERR_INVALID_ARG, "map_extract: out_capacity < 0");
        if (box) for (int k = 0; k < 6; ++k) if (std::isnan(box[k])) return fail(pe, SCL_ERR_INVALID_ARG, "map_extract: the box holds a NaN");
        std::string err;
        const int rc = map_extract(&pe->gmap, pe->stream, box, out, out_capacity, n_out, pe->prof_on == 1, &err);
        if (rc) pe->last_error = err;
        return rc;
    });
}

int scl_map_stats(scl_engine *e, struct scl_map_stats *out)
{
    return map_call(e, [&](scl_engine *pe) {
        if (!out) return fail(pe, SCL_ERR_INVALID_ARG, "map_stats: out is NULL");
        if (!pe->gmap.exists) return fail(pe, SCL_ERR_INVALID_ARG, "map_stats: no map yet (scl_map_reset)");
        std::string err;
        unsigned long long occupied = 0;
        const int rc = map_count(&pe->gmap, pe->stream, &occupied, &err);
        if (rc) { pe->last_error = err; return rc; }
        out->keyframes = (uint64_t)pe->gmap.entries.size();
        out->points_added = pe->gmap.points_added; out->points_skipped = pe->gmap.points_skipped;
        out->occupied_voxels = occupied; out->capacity = pe->gmap.capacity; out->growths = pe->gmap.growths;
        return (int)SCL_OK;
    });
}

int scl_map_last_timing(scl_engine *e, double ms[3])
{
    return map_call(e, [&](scl_engine *pe) {
        if (!ms) return fail(pe, SCL_ERR_INVALID_ARG, "map_last_timing: ms is NULL");
        for (int k = 0; k < 3; ++k) ms[k] = pe->gmap.ms[k];
        return (int)SCL_OK;
    });
}

int scl_selftest_map_capacity(scl_engine *e, uint64_t slots)
{
    return map_call(e, [&](scl_engine *pe) {
        if (slots > gmap::kMaxSlots) return fail(pe, SCL_ERR_INVALID_ARG, "selftest_map_capacity: more than 2^31 slots");
        pe->gmap.next_start_slots = slots;
        return (int)SCL_OK;
    });
}
