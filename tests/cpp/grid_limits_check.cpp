// grid_limits_check -- the grid contract (scl_slam_amd/csrc/grid_limits.hpp: grid_limit, sc_fast_plan, sc_fast_branch) on its own,
// without a GPU and under ASan + UBSan (tests/test_grid_limits.py runs it).  Over ALL 256 x 1024 grids of scl_create's old range the
// predicate is compared with conditions restated here from the kernels (make_sc.hip, sc_distance.hip), not from the header:
//   (a) an accepted grid satisfies every one of them: the bytes of the scatter's and of the ingest's launch (the ingest's counted
//       by walking its LDS layout as ingest_body lays it out) within a workgroup's 160 KB with the kernels' static LDS, every sector
//       in kmask's seven words and in one workgroup's threads, every index split's operand below 2^16 and divisor at least 2, and
//       for every search ratio's SR the specialised exact kernel either fits with G >= 1 or is not taken;
//   (b) a refused grid violates at least one of them -- so the predicate refuses nothing it need not, the boundary included;
//   (c) the multiply-high split itself is exact for every divisor 2 .. 2^16 - 1 at the operands where a quotient changes.
// The literals the Python tests and the documents quote (Rmax = 174 at 224 sectors, 154 sectors at 256 rings) are asserted too.
// Exit status 0 and "grid_limits_check: ok", or the first failed check and 1.
#include "grid_limits.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>

namespace {

int g_R, g_S, g_SR;                              // what a failed check prints

#define CHECK(cond)                                                                                                      \
    do {                                                                                                                 \
        if (!(cond)) {                                                                                                   \
            std::fprintf(stderr, "grid_limits_check: %s:%d: %s  (R %d, S %d, SR %d)\n", __FILE__, __LINE__, #cond, g_R, g_S, g_SR); \
            std::exit(1);                                                                                                \
        }                                                                                                                \
    } while (0)

constexpr int64_t kCap = 160 * 1024;             // LDS of a workgroup
constexpr int64_t kStatic = 256;                 // ingest_kernel, front_fused_kernel: .group_segment_fixed_size of the code object

// the end of ingest_body's LDS layout in bytes: sv [R][S + 1] floats, siv [S] floats, then (8-byte aligned) svk, sdd, snorm [S] doubles
int64_t ingest_layout_end(int64_t R, int64_t S)
{
    const int64_t LS = S + 1;
    const int64_t siv_end = R * LS + S;                                  // floats
    const int64_t svk_at = (R * LS + S + 1) & ~(int64_t)1;               // floats: where the doubles begin
    if (svk_at < siv_end) return INT64_MAX;                              // (the doubles would overlap siv)
    return 4 * svk_at + 8 * 3 * S;
}

// fastdiv as make_sc.hip has it, in plain integers
uint32_t magic(uint32_t d) { return 0xffffffffu / d + 1u; }
uint32_t fastdiv(uint32_t n, uint32_t m) { return (uint32_t)(((uint64_t)n * m) >> 32); }

struct Split { int64_t count, divisor; };        // indices 0 .. count - 1 are split by divisor
int splits(int64_t R, int64_t S, Split out[8])
{
    const int64_t RG = (R + 3) / 4, RGH = ((RG * 8 + 63) / 64) * 8;
    const int64_t P = S % 8 == 0 ? 8 : (S % 4 == 0 ? 4 : 0), CP = ((S + 8 + 31) / 32) * 32;
    int n = 0;
    out[n++] = {R * S, S};
    out[n++] = {RG * S, S};
    out[n++] = {S * RGH, RGH};
    if (RGH % 8 == 0) out[n++] = {(RGH / 8) * 8 * (S + 16) / 2, S + 16};
    if (P) { out[n++] = {P * CP, CP}; out[n++] = {(CP - 1) + S + 1, S}; }
    return n;
}

// every condition an accepted grid must satisfy, restated; the first that fails (0: none)
int violated(int R, int S)
{
    if (R < 1 || R > 256 || S < 1 || S > 1024) return 1;
    if ((S + 31) / 32 > 7) return 2;                                     // kmask words 0..6
    if (S >= 256) return 3;                                              // thread c of 256 looks at column c
    if (4 * (int64_t)R * S > kCap) return 4;                             // scatter: no static LDS
    const int64_t dyn = (int64_t)scl::ingest_lds_bytes(R, S);
    if (ingest_layout_end(R, S) > dyn) return 5;                         // the launch's bytes cover the layout
    if (dyn + kStatic > kCap) return 6;
    const int64_t fused = dyn > 4 * (int64_t)R * S ? dyn : 4 * (int64_t)R * S;
    if (fused + kStatic > kCap) return 7;
    Split sp[8];
    const int n = splits(R, S, sp);
    for (int i = 0; i < n; ++i)
        if (sp[i].divisor < 2 || sp[i].divisor >= 65536 || sp[i].count > 65536) return 8;
    return 0;
}

void check_fast_plans(int R, int S)
{
    static const int tmpl[3][3] = {{5, 7, 512}, {16, 13, 512}, {20, 19, 256}};
    for (int SR = 0; SR <= S; ++SR) {
        g_SR = SR;
        const int fast = scl::sc_fast_branch(R, S, SR);
        const int RG = (R + 3) / 4, W = 2 * SR + 1;
        if (!fast) continue;
        CHECK(fast == RG);
        int t = -1;
        for (int k = 0; k < 3; ++k) if (tmpl[k][0] == fast) t = k;
        CHECK(t >= 0 && tmpl[t][1] == W && S >= W);
        const scl::ScFastPlan p = scl::sc_fast_plan(tmpl[t][0], tmpl[t][1], tmpl[t][2], S);
        CHECK(p.G >= 1 && p.G <= 8);
        const int64_t QS = S + W - 1, NW = (S + 63) / 64;
        CHECK((int64_t)p.fixed == (RG * 4 * QS + 2 * S) * 8 && (int64_t)p.per_group == (4 * (int64_t)S + (int64_t)W * S + 8) * 8);
        CHECK((int64_t)p.fixed + p.G * (int64_t)p.per_group <= kCap);
        CHECK(p.G * NW * 64 <= tmpl[t][2]);
    }
    g_SR = -1;
}

}  // namespace

int main()
{
    // (c) the split is exact wherever a quotient changes, for every divisor the kernels can meet
    for (uint32_t d = 2; d < 65536; ++d) {
        const uint32_t m = magic(d);
        for (uint32_t q = 0; q * d < 65536; ++q) {
            g_R = (int)d; g_S = (int)q; g_SR = -1;
            CHECK(fastdiv(q * d, m) == q);
            if (q * d + d - 1 < 65536) CHECK(fastdiv(q * d + d - 1, m) == q);
        }
        CHECK(fastdiv(65535, m) == 65535 / d);
    }
    CHECK(magic(1) == 0);                                                // why S = 1 is refused: every index would split to row 0

    long accepted = 0;
    for (int R = 0; R <= 257; ++R)
        for (int S = 0; S <= 1025; ++S) {
            g_R = R; g_S = S; g_SR = -1;
            const scl::GridLimit l = scl::grid_limit(R, S, 0);
            const int v = violated(R, S);
            if (R < 1 || R > 256 || S < 1 || S > 1024) { CHECK(l == scl::kGridRange && v == 1); continue; }
            CHECK(l != scl::kGridRange);
            if (S == 1) { CHECK(l == scl::kGridOneSector); continue; }   // divisor 1: violated() says so too
            CHECK((l == scl::kGridOk) == (v == 0));                       // (a) and (b)
            if (l != scl::kGridOk) continue;
            ++accepted;
            // the operands the header lists are the ones restated here
            scl::GridFastdiv fd[scl::kGridFastdivs];
            Split sp[8];
            const int n = scl::grid_fastdivs(R, S, fd), m = splits(R, S, sp);
            CHECK(n == m);
            for (int i = 0; i < n; ++i) CHECK(fd[i].operands == sp[i].count && fd[i].divisor == sp[i].divisor);
            for (int SR = 0; SR <= S; SR += 7) CHECK(scl::grid_supported(R, S, SR));   // no SR refuses an accepted grid
            check_fast_plans(R, S);
        }
    g_R = g_S = g_SR = -1;
    CHECK(violated(1, 1) == 8);

    // the plans the dispatch never reaches on an accepted grid, but must not wrap on: S up to 1024
    for (int S = 1; S <= 1024; ++S) {
        g_S = S;
        static const int tmpl[3][3] = {{5, 7, 512}, {16, 13, 512}, {20, 19, 256}};
        for (const auto &t : tmpl) {
            const scl::ScFastPlan p = scl::sc_fast_plan(t[0], t[1], t[2], S);
            CHECK(p.G >= 0 && p.G <= 8);
            if (p.G) CHECK((int64_t)p.fixed + p.G * (int64_t)p.per_group <= kCap && p.G * ((S + 63) / 64) * 64 <= t[2]);
        }
    }
    CHECK(scl::sc_fast_plan(16, 13, 512, 512).G == 0);                  // fixed alone exceeds the LDS: the difference used to wrap
    CHECK(scl::sc_fast_plan(5, 7, 512, 577).G == 0);                    // ten waves per candidate: none fits 512 threads
    // the plans of the three baseline grids are what they were (G before the few-candidates halving)
    CHECK(scl::sc_fast_plan(5, 7, 512, 60).G == 8 && scl::sc_fast_plan(16, 13, 512, 120).G == 4 && scl::sc_fast_plan(20, 19, 256, 180).G == 1);

    // the literals the tests and the documents quote
    g_S = 224;
    CHECK(scl::grid_supported(174, 224, 11) && scl::grid_limit(175, 224, 11) == scl::kGridIngestLds);
    CHECK(scl::grid_supported(256, 154, 8) && !scl::grid_supported(256, 155, 8));
    CHECK(scl::grid_limit(16, 225, 11) == scl::kGridSectorMask && scl::grid_limit(20, 1024, 51) == scl::kGridSectorMask);
    CHECK(scl::grid_limit(256, 224, 11) == scl::kGridScatterLds &&scl::grid_limit(1, 1, 0) == scl::kGridOneSector);
    CHECK(scl::grid_supported(1, 2, 0) && scl::grid_supported(20, 60, 3) && scl::grid_supported(64, 120, 6) && scl::grid_supported(80, 180, 9));
    CHECK(scl::grid_supported(256, 40, 2) && scl::grid_supported(16, 224, 11) && scl::grid_supported(33, 193, 10));
    std::printf("grid_limits_check: ok (%ld of %d grids accepted)\n", accepted, 256 * 1024);
    return 0;
}
