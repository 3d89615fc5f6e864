// grid_limits.hpp -- which descriptor grids (num_ring R x num_sector S) the engine takes, host code only (no HIP): every limit a kernel
// of the descriptor front end or of the plain search puts on R and S is written here once, by arithmetic, so that scl_create refuses
// a grid BEFORE it touches the device (a grid it accepts never fails at a launch for its size), the launch sites take their limits
// from here instead of repeating them, and tests/cpp/grid_limits_check.cpp sweeps all 256 x 1024 grids under ASan / UBSan without a
// GPU.  Internal linkage: the library exports nothing of it.
//
// The limits and where they come from:
//   R <= 256                the ring-key scan's query (ringkey_topk.hip), scl_create's old range
//   S >= 2                  make_sc.hip's index splits divide by S with one multiply-high by ceil(2^32 / S), which is 2^32 = 0 in 32
//                           bits at S = 1 (a one-sector descriptor has no shift to search either)
//   S <= 224                kmask holds seven words of sector bits (words 0..6; word 6 holds the bound E instead up to 192 sectors)
//   fastdiv operands < 2^16 the multiply-high is exact for n, d < 2^16: R * S, ceil(R / 4) * S, S * RGH, the chunk-major image's
//                           entries and the alignment image's P * CP are the largest indices split
//   scatter LDS             a private R x S tile of ints per workgroup, within the 160 KB a workgroup may have
//   ingest LDS              ingest_lds_bytes(R, S) of dynamic LDS plus the kernel's static LDS, within the same 160 KB; the fused
//                           launch (front_fused_kernel) takes the larger of the two and has the same static LDS
//   launch_fast             the specialised exact kernels (sc_distance.hip: RG = 5 / W = 7, 16 / 13, 20 / 19) stage
//                           sc_fast_plan().fixed + G * per_group bytes; a grid on which not even G = 1 fits goes to the generic
//                           kernel (sc_fast_plan().G == 0), whose 48 S bytes always fit -- so no accepted grid is refused for them
#pragma once

#include <cstddef>
#include <cstdint>

namespace scl {
namespace {

constexpr size_t kLdsPerWorkgroup = 160 * 1024;     // gfx950: LDS a workgroup may have (static + dynamic)
// .group_segment_fixed_size of ingest_kernel and of front_fused_kernel in the gfx950 code object's metadata (the scratch of
// __syncthreads_or's reduction); make_sc_batch_scatter_kernel has none.  launch_ingest / launch_front_fused compare it with
// what the loaded kernel reports (hipFuncGetAttributes) before they raise the dynamic limit, so a compiler that changes it is noticed.
constexpr size_t kIngestStaticLds = 256;
constexpr size_t kScFastStaticLds = 0;              // sc_distance_kernel<RG, W, MAXT>, all three instances: none, same source
constexpr int kGridMaxRing = 256;
constexpr int kGridMaxSector = 224;                 // sector bits of kmask: 7 words
constexpr int kGridMaskBoundSectors = 192;          // up to here word 6 of kmask holds the bound E, beyond it sector bits
constexpr int kFastdivLimit = 1 << 16;

constexpr size_t scatter_lds_bytes(int R, int S) { return sizeof(int) * (size_t)R * (size_t)S; }
constexpr size_t ingest_lds_bytes(int R, int S)
{
    return sizeof(float) * ((size_t)R * (size_t)(S + 1) + (size_t)S + 2) + sizeof(double) * 3 * (size_t)S;
}

// the index splits of ingest_body (make_sc.hip): the largest operand + 1 and the divisor of each; n: how many there are on this grid
struct GridFastdiv { int64_t operands; int64_t divisor; };
constexpr int kGridFastdivs = 6;
inline int grid_fastdivs(int R, int S, GridFastdiv out[kGridFastdivs])
{
    const int64_t RG = (R + 3) / 4, RGH = ((RG * 8 + 63) / 64) * 8;                  // kernels.hpp: hdesc_sector
    const int64_t P = S % 8 == 0 ? 8 : (S % 4 == 0 ? 4 : 0), CP = ((S + 8 + 31) / 32) * 32;   // halign_P, halign_CP
    int n = 0;
    out[n++] = {(int64_t)R * S, S};                                                  // cells -> (ring, sector)
    out[n++] = {RG * S, S};                                                          // tiled copy -> (ring group, sector)
    out[n++] = {(int64_t)S * RGH, RGH};                                              // screening copy -> (sector, ring group)
    if (RGH % 8 == 0) out[n++] = {(RGH / 8) * 4 * (S + 16), S + 16};                 // chunk-major image (hdesc2_elems / 2)
    if (P) { out[n++] = {P * CP, CP}; out[n++] = {CP + S, S}; }                      // alignment image, and its (k - rho) mod S
    return n;
}

enum GridLimit {
    kGridOk = 0,
    kGridRange,             // outside 1..256 x 1..1024: what scl_create always refused (SCL_ERR_INVALID_ARG)
    kGridOneSector,         // S = 1
    kGridSectorMask,        // S > 224
    kGridFastdivRange,      // an index split's operand reaches 2^16 or its divisor is below 2
    kGridScatterLds,        // the scatter's tile does not fit a workgroup's LDS
    kGridIngestLds,         // the ingest's staging does not fit a workgroup's LDS
};

// the plan of launch_fast<RG, W, MAXT> at S sectors: G candidates per workgroup; G = 0: does not fit, the generic kernel scores the grid
struct ScFastPlan { size_t fixed, per_group; int G; };
inline ScFastPlan sc_fast_plan(int RG, int W, int MAXT, int S)
{
    ScFastPlan p{};
    const int QS = S + W - 1, NW = (S + 63) / 64;
    p.fixed = (size_t)(RG * 4 * QS + 2 * S) * sizeof(double);
    p.per_group = (size_t)(4 * S + W * S + 8) * sizeof(double);
    const size_t room = kLdsPerWorkgroup - kScFastStaticLds;
    if (p.fixed + p.per_group > room) return p;                 // (never `room - fixed` first: it wraps when fixed is the larger)
    size_t G = (room - p.fixed) / p.per_group;
    const size_t max_g_threads = (size_t)(MAXT / (NW * 64));
    if (G > max_g_threads) G = max_g_threads;
    if (G > 8) G = 8;
    p.G = (int)G;
    return p;
}

// which specialised exact kernel launch_sc_distance takes on (R, S, SR) when the grid has no wave program: 0 none (generic), else
// the RG of launch_fast<5, 7, 512>, <16, 13, 512>, <20, 19, 256> -- only where its plan fits
inline int sc_fast_branch(int R, int S, int SR)
{
    const int RG = (R + 3) / 4, W = 2 * SR + 1;
    if (RG == 5 && W == 7 && S >= W) return sc_fast_plan(5, 7, 512, S).G >= 1 ? 5 : 0;
    if (RG == 16 && W == 13 && S >= W) return sc_fast_plan(16, 13, 512, S).G >= 1 ? 16 : 0;
    if (RG == 20 && W == 19 && S >= W && S <= 180) return sc_fast_plan(20, 19, 256, S).G >= 1 ? 20 : 0;
    return 0;
}

// the first limit the grid violates.  SR (the searched shifts either side, from search_ratio) selects the exact kernel only: the
// specialised ones are taken where they fit and the generic one otherwise (sc_fast_branch), so no SR refuses a grid.
inline GridLimit grid_limit(int R, int S, int SR)
{
    (void)SR;
    if (R < 1 || R > kGridMaxRing || S < 1 || S > 1024) return kGridRange;
    if (S < 2) return kGridOneSector;
    if (S > kGridMaxSector) return kGridSectorMask;
    GridFastdiv fd[kGridFastdivs];
    const int n = grid_fastdivs(R, S, fd);
    for (int i = 0; i < n; ++i)
        if (fd[i].operands > kFastdivLimit || fd[i].divisor < 2 || fd[i].divisor >= kFastdivLimit) return kGridFastdivRange;
    if (scatter_lds_bytes(R, S) > kLdsPerWorkgroup) return kGridScatterLds;
    if (ingest_lds_bytes(R, S) + kIngestStaticLds > kLdsPerWorkgroup) return kGridIngestLds;
    return kGridOk;
}

inline bool grid_supported(int R, int S, int SR) { return grid_limit(R, S, SR) == kGridOk; }

inline const char *grid_limit_text(GridLimit l)
{
    switch (l) {
    case kGridOk: return "supported";
    case kGridRange: return "num_ring outside 1..256 or num_sector outside 1..1024";
    case kGridOneSector: return "num_sector = 1: a one-sector descriptor has no shift to search";
    case kGridSectorMask: return "num_sector > 224: the sector masks hold 224 bits";
    case kGridFastdivRange: return "num_ring * num_sector too large for the ingest's index arithmetic";
    case kGridScatterLds: return "num_ring * num_sector too large for the descriptor scatter's LDS tile";
    case kGridIngestLds: return "num_ring * (num_sector + 1) too large for the ingest's LDS";
    }
    return "unknown";
}

}  // namespace
}  // namespace scl
