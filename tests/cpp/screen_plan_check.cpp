// screen_plan_check -- the launch schedule of a chunk of the screened stream form (scl_slam_amd/csrc/screen_plan.hpp: plan_chunk) on
// its own, without a GPU and under ASan + UBSan (tests/test_screen_plan.py runs it).  Over pairs in {0, 1}, spl in 1..16, every list
// length of the chunk, the lengths of the next chunk's list at which something changes, and every aligned_in that a chunk in front can
// leave, the plan is checked two ways:
//   (a) against restated_loop below: the loop that stood in the stream's submit before the plan was taken out of it, as plain integer
//       code -- the unit list and next_aligned must be equal;
//   (b) against check_invariants, which does not mention that loop: what any schedule must satisfy for the stream to be right.
// Exit status 0 and "screen_plan_check: ok", or the first failed check and 1.
#include "screen_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

namespace {

using scl::PlanGroup;
using scl::PlanUnit;

constexpr int kChunk = 128;                      // scans of a chunk at most (scl_engine::kScreenSets / 2)
constexpr int kBatch = 16;                       // kMaxScreenBatch: scans of a full launch group, the most a launch takes

struct Case { int pairs, spl, cur_m, nxt_m, aligned_in; };
Case g_case;                                     // what a failed check prints

#define CHECK(cond)                                                                                                              \
    do {                                                                                                                         \
        if (!(cond)) {                                                                                                           \
            std::fprintf(stderr, "screen_plan_check: %s:%d: %s  (pairs %d, spl %d, cur_m %d, nxt_m %d, aligned_in %d)\n", __FILE__, \
                         __LINE__, #cond, g_case.pairs, g_case.spl, g_case.cur_m, g_case.nxt_m, g_case.aligned_in);               \
            std::exit(1);                                                                                                        \
        }                                                                                                                        \
    } while (0)

// ---- (a) the loop as it stood in the stream's submit, its HIP calls replaced by a record of what they were given -----------------
struct Issued {
    int g0_off, g0_nq, g1_off, g1_nq;            // the products launch: launch_screen_group(g0) or launch_screen_pair_group(g0, g1)
    int n0_off, n0_nq, n1_off, n1_nq;            // the `next` groups handed to it (nq == 0: a null pointer)
    bool align0, align1;
    int waited;                                  // > 0: the wait in front of it was asked for, reach - cur.m scans into the next chunk
};

int restated_loop(int cur_m, int nxt_m, int spl, bool pairs, int k_aligned, std::vector<Issued> *out)
{
    struct G { int off, nq; };                   // (off: cur's list at its own offsets, nxt's behind them)
    auto group_at = [&](int off) {
        G g{0, 0};
        if (off < cur_m) {
            g = G{off, cur_m - off < spl ? cur_m - off : spl};
        } else if (nxt_m > 0 && off - cur_m < nxt_m) {
            const int o = off - cur_m;
            g = G{cur_m + o, nxt_m - o < spl ? nxt_m - o : spl};
        }
        return g;
    };
    auto pair_at = [&](int off) { return pairs && group_at(off).nq == kBatch && group_at(off + kBatch).nq == kBatch &&
                                         (off + 2 * kBatch <= cur_m || off >= cur_m); };
    out->clear();
    int aligned_to = k_aligned;
    for (int g = 0; g < cur_m;) {
        const bool pair = pair_at(g);
        const G g0 = group_at(g), g1 = pair ? group_at(g + g0.nq) : G{0, 0};
        const int end = g + g0.nq + g1.nq;
        G n0{0, 0}, n1 = n0;
        if (end >= aligned_to) {
            n0 = group_at(end);
            if (pair && pair_at(end)) n1 = group_at(end + n0.nq);
        }
        const int reach = end + n0.nq + n1.nq;
        int waited = 0;
        if (reach > cur_m && n0.nq > 0) waited = reach - cur_m;
        const bool align0 = g >= aligned_to, align1 = pair && g + g0.nq >= aligned_to;
        out->push_back({g0.off, g0.nq, g1.off, g1.nq, n0.off, n0.nq, n1.off, n1.nq, align0, align1, waited});
        if (reach > aligned_to) aligned_to = reach;
        g = end;
    }
    return aligned_to > cur_m ? aligned_to - cur_m : 0;
}

bool same(const PlanGroup &p, int off, int nq) { return p.nq == nq && (nq == 0 || p.off == off); }

// ---- (b) what a schedule must satisfy, whatever loop made it ---------------------------------------------------------------------
void check_invariants(const Case &c, const PlanUnit *u, int n_units, int next_aligned)
{
    const int all_m = c.cur_m + c.nxt_m;
    CHECK(n_units <= c.cur_m && n_units <= kChunk);
    // a group is scans of ONE list, a launch's worth at most
    auto one_list = [&](const PlanGroup &g) { return g.nq == 0 || (g.off >= 0 && g.nq <= c.spl && (g.off + g.nq <= c.cur_m || (g.off >= c.cur_m && g.off + g.nq <= all_m))); };
    std::vector<int> products_in((size_t)all_m, -1), aligned((size_t)all_m, 0), aligned_in_unit((size_t)all_m, -1);
    for (int s = 0; s < c.aligned_in; ++s) aligned[(size_t)s] = 1;        // (by the chunk before: in front of every launch of this one)
    int pos = 0;
    for (int i = 0; i < n_units; ++i) {
        const PlanUnit &p = u[i];
        CHECK(one_list(p.g0) && one_list(p.g1) && one_list(p.n0) && one_list(p.n1));
        // the products tile [0, cur_m) in ascending order: each scan in exactly one launch, none of the next chunk's in any
        CHECK(p.g0.nq > 0 && p.g0.off == pos);
        CHECK(p.g0.nq == std::min(c.spl, c.cur_m - pos));                    // (a short launch costs the same pass over the database)
        pos += p.g0.nq;
        if (p.g1.nq > 0) {                                                   // a pair: two groups of exactly 16, adjacent, both in this chunk
            CHECK(c.pairs && p.g0.nq == kBatch && p.g1.nq == kBatch && p.g1.off == pos && pos + kBatch <= c.cur_m);
            pos += p.g1.nq;
        }
        CHECK(pos <= c.cur_m);
        for (const PlanGroup *g : {&p.g0, &p.g1})
            for (int s = g->off; s < g->off + g->nq; ++s) { CHECK(products_in[(size_t)s] < 0); products_in[(size_t)s] = i; }
        CHECK(p.align1 ? p.g1.nq > 0 : true);
        // n1 only behind a pair, and only with both full: the two tails align the pair that follows
        if (p.n1.nq > 0) CHECK(p.g1.nq > 0 && p.n0.nq == kBatch && p.n1.nq == kBatch && p.n1.off == p.n0.off + kBatch);
        if (p.n0.nq > 0) CHECK(p.n0.off == pos);                             // (what a tail aligns begins right behind the unit)
        // who is aligned where: a group of its own in front of its products (same unit), a tail's behind them
        auto count = [&](const PlanGroup &g) { for (int s = g.off; s < g.off + g.nq; ++s) { ++aligned[(size_t)s]; aligned_in_unit[(size_t)s] = i; } };
        if (p.align0) count(p.g0);
        if (p.align1) count(p.g1);
        count(p.n0); count(p.n1);
        const int reach = std::max(p.n0.nq > 0 ? p.n0.off + p.n0.nq : 0, p.n1.nq > 0 ? p.n1.off + p.n1.nq : 0);
        CHECK((p.over > 0) == (reach > c.cur_m));                            // the wait: exactly when a tail writes the next chunk's sets,
        if (p.over > 0) CHECK(p.over == reach - c.cur_m);                    // and how far (the wide grid's choice of event rests on it)
    }
    CHECK(pos == c.cur_m);
    for (int s = 0; s < c.cur_m; ++s) {
        CHECK(products_in[(size_t)s] >= 0 && aligned[(size_t)s] == 1);       // every scan aligned exactly once ...
        const int i = aligned_in_unit[(size_t)s];                            // ... never after its products: its own launch in front of them
        if (i >= 0) CHECK(i < products_in[(size_t)s] || (i == products_in[(size_t)s] && (u[i].g0.off <= s && s < u[i].g0.off + u[i].g0.nq ? u[i].align0 : u[i].align1)));
    }
    for (int s = c.cur_m; s < all_m; ++s) {                                  // the next chunk: no products, its aligned scans a prefix
        CHECK(products_in[(size_t)s] < 0);
        CHECK(aligned[(size_t)s] == (s - c.cur_m < next_aligned ? 1 : 0));
    }
    CHECK(next_aligned >= 0 && next_aligned <= c.nxt_m);
}

std::vector<int> list_lengths(int spl, int chn)
{
    std::set<int> s;
    for (int v : {0, 1, spl - 1, spl, spl + 1, 15, 16, 17, 31, 32, 33, 48, chn})
        if (v >= 0 && v <= chn) s.insert(v);
    return std::vector<int>(s.begin(), s.end());
}

}  // namespace

int main()
{
    long long cases = 0, units_total = 0;
    int most_units = 0;
    std::vector<Issued> want, scratch;
    PlanUnit units[kChunk];
    for (int pairs = 0; pairs <= 1; ++pairs)
        for (int spl = 1; spl <= kBatch; ++spl) {
            const int chn = (kChunk / spl) * spl;
            const std::vector<int> lens = list_lengths(spl, chn);
            for (int cur_m = 0; cur_m <= chn; ++cur_m) {
                // every aligned_in a chunk in front can leave: a chunk of each of those lengths planned in front of this one -- itself
                // the call's first (nothing aligned for it) or behind a chunk of each of those lengths
                std::set<int> aligned_ins{0};
                for (int prev_m : lens) {
                    std::set<int> prev_ins{0};
                    for (int first_m : lens) prev_ins.insert(restated_loop(first_m, prev_m, spl, pairs != 0, 0, &scratch));
                    for (int a : prev_ins) {
                        g_case = {pairs, spl, prev_m, cur_m, a};
                        const int left = restated_loop(prev_m, cur_m, spl, pairs != 0, a, &scratch);
                        int left_plan = -1;
                        (void)scl::plan_chunk(prev_m, cur_m, spl, pairs != 0, a, units, &left_plan);
                        CHECK(left_plan == left && left <= cur_m);
                        aligned_ins.insert(left);
                    }
                }
                for (int nxt_m : lens)
                    for (int aligned_in : aligned_ins) {
                        const Case c{pairs, spl, cur_m, nxt_m, aligned_in};
                        g_case = c;
                        int next_aligned = -1;
                        const int n_units = scl::plan_chunk(cur_m, nxt_m, spl, pairs != 0, aligned_in, units, &next_aligned);
                        // (a)
                        const int want_next = restated_loop(cur_m, nxt_m, spl, pairs != 0, aligned_in, &want);
                        CHECK(n_units == (int)want.size() && next_aligned == want_next);
                        for (int i = 0; i < n_units; ++i) {
                            const Issued &w = want[(size_t)i];
                            const PlanUnit &p = units[i];
                            CHECK(same(p.g0, w.g0_off, w.g0_nq) && same(p.g1, w.g1_off, w.g1_nq));
                            CHECK(same(p.n0, w.n0_off, w.n0_nq) && same(p.n1, w.n1_off, w.n1_nq));
                            CHECK(p.align0 == w.align0 && p.align1 == w.align1 && p.over == w.waited);
                        }
                        // (b)
                        check_invariants(c, units, n_units, next_aligned);
                        ++cases; units_total += n_units; most_units = std::max(most_units, n_units);
                    }
            }
        }
    std::printf("screen_plan_check: %lld cases, %lld units, at most %d units per chunk\n", cases, units_total, most_units);
    std::printf("screen_plan_check: ok\n");
    return 0;
}
