// sc_rank.hip -- the selection behind scl_sc_search / scl_sc_search_range / scl_sc_search_intra / _inter: the k smallest entries of
// each row of a finished group of the exact distance matrix (sc_distance.hip, sc_matrix.hip, sc_masked.hip write the rows; nothing
// here computes a distance).
//
// A row holds, per keyframe of the group's range, distanceBtnScanContext (descriptor.h:1538-1569) in fp64 and its shift.  The list of a
// row is its k smallest entries in ascending (distance compared as doubles, position) order among the positions [plo, phi) of the
// row's own query that are listable: distance < 1e7, argmin_kernel's rule (sc_distance.hip), which NaN fails by itself.  The robot-aware
// searches (scl_sc_search_intra / _inter) add a rule per row on the (robot, index) of the entry's database slot (kernels.hpp: ScRankRule),
// applied where the entry becomes a key: an entry that fails its row's rule is a filler like an unlistable one, so rows of different
// rules share a launch and the merge knows nothing of rules.  Without the slot arrays no entry is filtered.
//
//   * The key of an entry is the pair (u64 image of the distance, u32 position).  The image keeps the order of the doubles: sign bit
//     set -> every bit flipped, otherwise -> the sign bit set; -0.0 is keyed as +0.0, since the two compare equal and the position
//     must decide between them.  An entry that is not listable is a filler (~0, ~0): it sorts behind every key, and every listable
//     distance is below 1e7, so no key is a filler's.  Keys are distinct apart from the fillers, which are interchangeable: the
//     result depends on nothing but the row -- no atomics, no workgroup or wave order.
//   * sc_rank_tile_kernel: a wave takes 64 consecutive positions of a row, sorts its keys with a bitonic network through __shfl_xor
//     (21 compare-exchange stages, plugin_host.hpp: wave_sort_ascending) and emits the tile's k smallest into part[row][tile][k].
//     Tiles outside the row's own range write nothing and are not read.
//   * sc_rank_merge_kernel: one workgroup per row folds the tiles' lists through LDS in rounds of up to kRankMergeCap - k keys beside
//     the k best so far, each round one bitonic sort of the next power of two (plugin_host.hpp: nn_topk_merge_kernel), and writes the
//     (distance, id, shift) records: the distance is the row's own double (its bits, not the key's), the id the database slot.
#include "device_common.hpp"
#include "kernels.hpp"

namespace scl {

namespace {

constexpr int kRankTile = 64;                  // positions per wave
constexpr int kRankTileWaves = 4;              // waves (= tiles) per workgroup of the tile kernel
constexpr int kRankMergeThreads = 256;
constexpr int kRankMergeCap = 2048;            // keys the merge sorts at once (24 KB of LDS)
constexpr unsigned long long kRankNoKey = ~0ull;
constexpr unsigned int kRankNoPos = ~0u;
static_assert(kMaxScreenBatch <= 16 && kMaxQueryBatch <= 16, "ScRankArgs holds the ranges of 16 rows");
static_assert(kScRankMaxK <= kRankTile && 2 * kScRankMaxK <= kRankMergeCap, "a wave lists at most one key per lane");

__device__ __forceinline__ unsigned long long rank_key(double d)
{
    unsigned long long b = (unsigned long long)__double_as_longlong(d);
    if ((b << 1) == 0) b = 0;                                              // -0.0 == 0.0
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ bool rank_less(unsigned long long ak, unsigned int ap, unsigned long long bk, unsigned int bp)
{
    return ak < bk || (ak == bk && ap < bp);
}

__global__ __launch_bounds__(kRankTileWaves * kRankTile) void sc_rank_tile_kernel(ScRankArgs a)
{
    const int lane = threadIdx.x & (kRankTile - 1), r = blockIdx.y;
    const int tile = blockIdx.x * kRankTileWaves + (threadIdx.x >> 6);     // the same for every lane of a wave
    const int plo = a.plo[r], phi = a.phi[r];
    if (tile >= a.tiles || plo >= phi || tile < plo / kRankTile || tile > (phi - 1) / kRankTile) return;
    const int p = tile * kRankTile + lane;
    unsigned long long key = kRankNoKey;
    unsigned int pos = kRankNoPos;
    if (p >= plo && p < phi) {                                             // (phi <= n: inside the row)
        const double d = a.dist[(size_t)r * a.row_stride + (size_t)p];
        bool listable = d < kBigDist;
        if (a.meta_robot && (a.rule[r].flags & kScRuleActive)) {           // the row's rule on (robot, index) of slot base + p
            const ScRankRule rule = a.rule[r];
            const size_t s = (size_t)a.base + (size_t)p;
            listable = listable && (((int)a.meta_robot[s] == rule.robot) != ((rule.flags & kScRuleNotEqual) != 0));
            if (rule.flags & kScRuleIndex) listable = listable && a.meta_index[s] < rule.bound;
        }
        if (listable) { key = rank_key(d); pos = (unsigned int)p; }
    }
#pragma unroll
    for (int k2 = 2; k2 <= kRankTile; k2 <<= 1)
#pragma unroll
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            const unsigned long long ok = __shfl_xor(key, j);
            const unsigned int op = __shfl_xor(pos, j);
            const bool keep_min = ((lane & j) == 0) == ((lane & k2) == 0);  // k2 == 64: every pair ascending
            if (rank_less(ok, op, key, pos) == keep_min) { key = ok; pos = op; }
        }
    if (lane < a.k) {
        const size_t o = ((size_t)r * (size_t)a.tiles + (size_t)tile) * (size_t)a.k + (size_t)lane;
        a.part_key[o] = key; a.part_pos[o] = pos;
    }
}

__global__ __launch_bounds__(kRankMergeThreads) void sc_rank_merge_kernel(ScRankArgs a)
{
    __shared__ unsigned long long kbuf[kRankMergeCap];
    __shared__ unsigned int pbuf[kRankMergeCap];
    const int r = blockIdx.x, t = threadIdx.x, k = a.k;
    const int plo = a.plo[r], phi = a.phi[r];
    const int tile_lo = plo < phi ? plo / kRankTile : 0, tile_hi = plo < phi ? (phi - 1) / kRankTile + 1 : 0;
    if (t < k) { kbuf[t] = kRankNoKey; pbuf[t] = kRankNoPos; }
    const size_t total = (size_t)(tile_hi - tile_lo) * (size_t)k;
    const size_t src = ((size_t)r * (size_t)a.tiles + (size_t)tile_lo) * (size_t)k;
    for (size_t done = 0; done < total;) {
        const int chunk = total - done < (size_t)(kRankMergeCap - k) ? (int)(total - done) : kRankMergeCap - k;
        int m = 2;
        while (m < k + chunk) m <<= 1;                                     // <= kRankMergeCap
        for (int e = t; e < m - k; e += kRankMergeThreads) {
            kbuf[k + e] = e < chunk ? a.part_key[src + done + (size_t)e] : kRankNoKey;
            pbuf[k + e] = e < chunk ? a.part_pos[src + done + (size_t)e] : kRankNoPos;
        }
        __syncthreads();
        for (int k2 = 2; k2 <= m; k2 <<= 1)
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                for (int e = t; e < m / 2; e += kRankMergeThreads) {
                    const int lo = ((e & ~(j - 1)) << 1) | (e & (j - 1)), hi = lo | j;
                    const unsigned long long xk = kbuf[lo], yk = kbuf[hi];
                    const unsigned int xp = pbuf[lo], yp = pbuf[hi];
                    if (rank_less(yk, yp, xk, xp) == ((lo & k2) == 0)) { kbuf[lo] = yk; pbuf[lo] = yp; kbuf[hi] = xk; pbuf[hi] = xp; }
                }
                __syncthreads();
            }
        done += (size_t)chunk;
    }
    __syncthreads();                                                       // total == 0: the fillers of kbuf / pbuf [0, k) written
    if (t >= k) return;
    ScRankRecord rec = {kBigDist, -1, 0};                                  // the engine's "no winner" values
    const unsigned int p = pbuf[t];
    if (p != kRankNoPos) {
        const size_t o = (size_t)r * a.row_stride + (size_t)p;
        rec.dist = a.dist[o]; rec.id = a.base + (int)p; rec.shift = a.shift[o];
    }
    a.out[(size_t)r * (size_t)k + (size_t)t] = rec;
}

}  // namespace

size_t sc_rank_part_entries(int rows, int n, int k)
{
    return (size_t)rows * (size_t)((n + kRankTile - 1) / kRankTile) * (size_t)k;
}

hipError_t launch_sc_rank(const ScRankArgs &args, hipStream_t stream)
{
    if (args.rows < 1 || args.rows > kMaxScreenBatch || args.k < 1 || args.k > kScRankMaxK || args.n < 0 || !args.out) return hipErrorInvalidValue;
    if (args.n > 0 && (!args.dist || !args.shift || !args.part_key || !args.part_pos || args.row_stride < (unsigned long long)args.n)) return hipErrorInvalidValue;
    for (int r = 0; r < args.rows; ++r)
        if (args.plo[r] < 0 || args.phi[r] > args.n || args.phi[r] < args.plo[r]) return hipErrorInvalidValue;
    if ((args.meta_robot != nullptr) != (args.meta_index != nullptr)) return hipErrorInvalidValue;
    ScRankArgs a = args;
    a.tiles = (a.n + kRankTile - 1) / kRankTile;
    if (a.tiles > 0) {
        hipLaunchKernelGGL(sc_rank_tile_kernel, dim3((unsigned)((a.tiles + kRankTileWaves - 1) / kRankTileWaves), (unsigned)a.rows),
                           dim3(kRankTileWaves * kRankTile), 0, stream, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(sc_rank_merge_kernel, dim3((unsigned)a.rows), dim3(kRankMergeThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace scl
