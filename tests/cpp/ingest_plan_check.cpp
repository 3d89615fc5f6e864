// ingest_plan_check -- two pieces of the ingest host layer on their own, without a GPU and under ASan + UBSan (tests/test_ingest_plan.py
// runs it):
//   1. the copy plan of a group of clouds of the points pipeline (scl_slam_amd/csrc/ingest_plan.hpp: plan_group_copy) over enumerated
//      layouts of synthetic addresses, which are never dereferenced.  Every result is checked two ways:
//        (a) against restated_group_bytes below: the lambda that stood in the pipeline before the plan was taken out of it, on integers;
//        (b) against check_invariants, which does not mention that lambda: what any plan must satisfy for the copies to be right.
//   2. the table of the database's arrays (scl_slam_amd/csrc/db_arrays.hpp) against the sizes and offsets the engine's growth was
//      written with before the table, for the grids 20 x 60, 64 x 120, 80 x 180 and 1 x 1 with their row widths as numbers.
// Exit status 0 and "ingest_plan_check: ok", or the first failed check and 1.
#include "db_arrays.hpp"
#include "ingest_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace {

constexpr int G = 16;                            // kMaxScBatch: clouds of a group at most

std::string g_case;                              // what a failed check prints

#define CHECK(cond)                                                                                             \
    do {                                                                                                        \
        if (!(cond)) {                                                                                          \
            std::fprintf(stderr, "ingest_plan_check: %s:%d: %s  (%s)\n", __FILE__, __LINE__, #cond, g_case.c_str()); \
            std::exit(1);                                                                                       \
        }                                                                                                       \
    } while (0)

struct Call { std::vector<uintptr_t> addr; std::vector<int> n; int stride; };

// ---- (a) the pipeline's lambda as it stood, its pointers as integers ----------------------------------------------------------------
size_t restated_group_bytes(const Call &c, int g, size_t *off, bool *merged_out)
{
    const int n_scans = (int)c.n.size();
    const int i0 = g * G, i1 = (g + 1) * G < n_scans ? (g + 1) * G : n_scans;
    bool merged = i1 - i0 >= 2;
    const uintptr_t base = c.addr[(size_t)i0];
    uintptr_t end = base;
    for (int i = i0; merged && i < i1; ++i) {
        const uintptr_t p = c.addr[(size_t)i];
        const size_t bytes = (size_t)c.n[(size_t)i] * (size_t)c.stride;
        if (!p || bytes == 0 || p < end || (size_t)(p - end) >= 4096 || ((size_t)(p - base) & 15)) merged = false;
        else end = p + bytes;
    }
    if (merged_out) *merged_out = merged;
    if (merged) {
        for (int i = i0; off && i < i1; ++i) off[i - i0] = (size_t)(c.addr[(size_t)i] - base);
        return (size_t)(end - base) + 16;
    }
    size_t at = 0;
    for (int i = i0; i < i1; ++i) {
        if (off) off[i - i0] = at;
        at += (((size_t)c.n[(size_t)i] * (size_t)c.stride + 16) + 255) & ~(size_t)255;
    }
    return at;
}

// ---- (b) what a plan must satisfy, whatever code made it ----------------------------------------------------------------------------
void check_invariants(const Call &c, int i0, int i1, const scl::GroupCopyPlan &p)
{
    const int m = i1 - i0;
    auto bytes = [&](int j) { return (size_t)c.n[(size_t)(i0 + j)] * (size_t)c.stride; };
    auto addr = [&](int j) { return c.addr[(size_t)(i0 + j)]; };
    // merged exactly when: two clouds at least, none empty or null, ascending addresses with gaps below a page, distances from the
    // first a multiple of 16
    bool want = m >= 2;
    for (int j = 0; j < m; ++j) want = want && addr(j) != 0 && bytes(j) != 0;
    for (int j = 1; want && j < m; ++j) {
        const uintptr_t prev_end = addr(j - 1) + bytes(j - 1);
        want = addr(j) >= prev_end && addr(j) - prev_end < 4096 && (addr(j) - addr(0)) % 16 == 0;
    }
    CHECK(p.merged == want);
    if (p.merged) {
        for (int j = 0; j < m; ++j) CHECK(p.off[j] == (size_t)(addr(j) - addr(0)));
        CHECK(p.span == (size_t)(addr(m - 1) + bytes(m - 1) - addr(0)) + 16);
        return;
    }
    CHECK(p.off[0] == 0);
    for (int j = 0; j < m; ++j) {
        CHECK(p.off[j] % 256 == 0);
        const size_t limit = j + 1 < m ? p.off[j + 1] : p.span;             // the clouds do not overlap, and each has 16 bytes behind it
        CHECK(p.off[j] + bytes(j) + 16 <= limit);
    }
    CHECK(p.span == p.off[m - 1] + ((bytes(m - 1) + 16 + 255) / 256) * 256);
}

long long g_groups = 0, g_merged = 0;

void check_call(const Call &c)
{
    const int n_scans = (int)c.n.size();
    for (int g = 0; g * G < n_scans; ++g) {
        const int i0 = g * G, i1 = (g + 1) * G < n_scans ? (g + 1) * G : n_scans;
        const scl::GroupCopyPlan p = scl::plan_group_copy(c.addr.data(), c.n.data(), c.stride, i0, i1);
        size_t off[G];
        bool merged = false;
        const size_t span = restated_group_bytes(c, g, off, &merged);
        CHECK(p.merged == merged && p.span == span);
        CHECK(span == restated_group_bytes(c, g, nullptr, nullptr));         // (the lambda's `need` form)
        for (int j = 0; j < i1 - i0; ++j) CHECK(p.off[j] == off[j]);
        check_invariants(c, i0, i1, p);
        ++g_groups; g_merged += p.merged;
    }
}

// what is done to one cloud of a layout
enum Defect { kNone, kLower, kOverlap, kMisaligned, kEmpty, kNullEmpty, kDefects };
const char *const kDefectName[kDefects] = {"none", "lower", "overlap", "misaligned", "empty", "null+empty"};

void plan_checks()
{
    const int totals[] = {1, 2, 15, 16, 20, 33};                            // groups of 1, 2, 15, 16; calls whose last group is partial (4, 1)
    const int strides[] = {12, 16, 32};
    const int counts[][3] = {{2000, 2000, 2000}, {1000, 1999, 4}, {1, 1, 1}, {0, 0, 0}, {2048, 0, 1024}, {1001, 1000, 1000}};
    const size_t gaps[] = {0, 16, 4080, 4095, 4096, 8192};
    for (int total : totals)
        for (int stride : strides)
            for (const auto &cnt : counts)
                for (size_t gap : gaps)
                    for (int defect = 0; defect < kDefects; ++defect) {
                        const int places[] = {0, 1, total / 2, total - 1};
                        for (int at : places) {
                            if (at >= total || (defect == kNone && at != 0)) continue;
                            Call c;
                            c.stride = stride;
                            uintptr_t next = (uintptr_t)0x7f0000001000ull;   // (a page boundary: never dereferenced)
                            for (int i = 0; i < total; ++i) {
                                int n = cnt[i % 3];
                                uintptr_t a = next;
                                if (i == at) {
                                    if (defect == kLower && i > 0) a = c.addr[(size_t)(i - 1)] - 4096;
                                    if (defect == kOverlap && i > 0) a = c.addr[(size_t)(i - 1)] + ((size_t)c.n[(size_t)(i - 1)] * (size_t)stride) / 2 / 16 * 16;
                                    if (defect == kMisaligned) a += 4;
                                    if (defect == kEmpty) n = 0;
                                    if (defect == kNullEmpty) { n = 0; a = 0; }
                                }
                                c.addr.push_back(a);
                                c.n.push_back(n);
                                if (a) next = a + (size_t)n * (size_t)stride + gap;
                            }
                            g_case = "clouds " + std::to_string(total) + ", stride " + std::to_string(stride) + ", counts " + std::to_string(cnt[0]) + "/" +
                                     std::to_string(cnt[1]) + "/" + std::to_string(cnt[2]) + ", gap " + std::to_string(gap) + ", " + kDefectName[defect] + " at " + std::to_string(at);
                            check_call(c);
                        }
                    }
    CHECK(g_merged > 0 && g_merged < g_groups);                               // both answers were seen
}

// ---- 2. the table of the database's arrays ------------------------------------------------------------------------------------------
struct F4 { float v[4]; };
struct U2 { unsigned v[2]; };

struct Grid { const char *name; size_t RG, S, R4, hstride, hkw, halign; };  // the row widths of a grid (kernels.hpp's formulas, worked out)

void table_checks()
{
    using namespace scl;
    const Grid grids[] = {
        {"20x60",  5,  60,  20, 1120, 136, 1552},
        {"64x120", 16, 120, 64, 4144, 264, 4112},
        {"80x180", 20, 180, 80, 9088, 392, 3088},
        {"1x1",    1,  1,   4,  176,  72,  0},
    };
    for (const Grid &g : grids)
        for (size_t cap : {(size_t)1, (size_t)8, (size_t)4096})
            for (size_t st : {(size_t)76, (size_t)76 + 512}) {
                g_case = std::string(g.name) + ", cap " + std::to_string(cap) + ", stage rows " + std::to_string(st);
                const DbShape sh{g.RG * g.S, g.S, g.R4, g.hstride, 8, g.hkw, g.halign, g.RG};
                const size_t nst = cap + st, tile = g.RG * g.S;
                // the allocations as the growth spelled them out: elements x sizeof
                const size_t want_bytes[kDbArrayCount] = {16 * tile * nst, 8 * g.S * nst, 8 * g.S * nst, 4 * g.R4 * nst, 8 * g.hstride * nst,
                                                          4 * 8 * nst, 2 * g.hkw * nst, g.halign * cap, 16 * g.RG * cap};
                const size_t want_row[kDbArrayCount] = {16 * tile, 8 * g.S, 8 * g.S, 4 * g.R4, 8 * g.hstride, 32, 2 * g.hkw, g.halign, 16};
                const bool want_staged[kDbArrayCount] = {true, true, true, true, true, true, true, false, false};
                for (int id = 0; id < kDbArrayCount; ++id) {
                    const DbArrayInfo &t = kDbArrays[id];
                    CHECK(db_array_bytes(t, sh, cap, st) == want_bytes[id]);
                    CHECK(db_array_present(t, sh) == (want_bytes[id] != 0));
                    CHECK(t.staged == want_staged[id]);                       // a staging-row copy skips the alignment images and the tiled ring key
                    CHECK(t.slot_major == (id != kDbRkey4));
                    for (size_t s : {(size_t)0, (size_t)1, cap - 1}) CHECK(db_row_offset(t, sh, s) == want_row[id] * s);
                    if (t.staged)
                        for (size_t j : {(size_t)0, (size_t)1, st - 1}) {
                            CHECK(db_row_offset(t, sh, cap + j) == want_row[id] * (cap + j));
                            CHECK(db_row_offset(t, sh, cap + j) + db_row_bytes(t, sh) <= db_array_bytes(t, sh, cap, st));
                        }
                }
                CHECK(!db_array_present(kDbArrays[kDbHalign], sh) == (g.halign == 0));
            }
    // the struct of pointers: the table's id reaches the member of that name
    DbArraysOf<F4, U2> a;
    alignas(16) static unsigned char mem[kDbArrayCount][16];
    for (int id = 0; id < kDbArrayCount; ++id) { CHECK(a.at(id) == nullptr); a.set(id, mem[id]); }
    for (int id = 0; id < kDbArrayCount; ++id) CHECK(a.at(id) == mem[id]);
    CHECK((void *)a.d_desc == mem[kDbDesc] && (void *)a.d_vkey == mem[kDbVkey] && (void *)a.d_norm == mem[kDbNorm] && (void *)a.d_rkey == mem[kDbRkey]);
    CHECK((void *)a.d_hdesc == mem[kDbHdesc] && (void *)a.d_kmask == mem[kDbKmask] && (void *)a.d_hkey == mem[kDbHkey]);
    CHECK((void *)a.d_halign == mem[kDbHalign] && (void *)a.d_rkey4 == mem[kDbRkey4]);
}

}  // namespace

int main()
{
    plan_checks();
    table_checks();
    std::printf("ingest_plan_check: %lld groups, %lld of them merged\n", g_groups, g_merged);
    std::printf("ingest_plan_check: ok\n");
    return 0;
}
