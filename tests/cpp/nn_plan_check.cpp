// nn_plan_check -- the plan of the vector plugins' batched search (scl_slam_amd/csrc/nn_plan.hpp) on its own, without a GPU and
// under ASan + UBSan (tests/test_nn_plan.py runs it): the grouping, the list offsets, a group's own prefix, the partial lists' rows
// and the 2^31 guard, which no GPU test can allocate its way to.  The plan only does arithmetic: nothing here is sized by a limit.
// Exit status 0 and "nn_plan_check: ok", or the first failed check and 1.
#include "nn_plan.hpp"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

constexpr int kGroup = 16, kTile = 64;

#define CHECK(cond)                                                                                \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            std::fprintf(stderr, "nn_plan_check: %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            std::exit(1);                                                                          \
        }                                                                                          \
    } while (0)

struct Call {
    std::vector<int> qkey, limit, which;
    scl::NnList lists[2];
    int k;
};

const int kSomeKeys[1] = {0};                    // a list with keys: the plan looks at the pointer only

// what every plan must satisfy, whatever the call; returns the plan
scl::NnPlan checked_plan(const Call &c)
{
    const int count = (int)c.qkey.size();
    scl::NnPlan p;
    CHECK((scl::nn_plan<kGroup, kTile>(c.qkey.data(), c.limit.data(), c.which.data(), c.lists, count, c.k, &p)));
    // order: a permutation, list 0's queries first, stable within each list
    CHECK((int)p.order.size() == count);
    std::vector<int> seen((size_t)count, 0);
    for (int j = 0; j < count; ++j) {
        const int i = p.order[(size_t)j];
        CHECK(i >= 0 && i < count && !seen[(size_t)i]++);
        CHECK(c.which[(size_t)i] == (j < p.seg[1] ? 0 : 1));
        if (j > 0 && j != p.seg[1]) CHECK(p.order[(size_t)j - 1] < i);
    }
    CHECK(p.seg[0] == 0 && p.seg[2] == count);
    // used, off, keys
    size_t keys = 0;
    for (int l = 0; l < 2; ++l) {
        int used = 0;
        for (int i = 0; i < count; ++i)
            if (c.which[(size_t)i] == l) used = std::max(used, c.limit[(size_t)i]);
        CHECK(p.used[l] == used);
        if (c.lists[l].keys && used > 0) { CHECK(p.off[l] == (int)keys); keys += (size_t)used; }
        else CHECK(p.off[l] == -1);
    }
    CHECK(p.keys == keys);
    // the table, in the grouped order
    CHECK(p.cols == (c.k > 0 ? 4 : 3) && p.table.size() == (size_t)p.cols * (size_t)count);
    for (int j = 0; j < count; ++j) {
        const int i = p.order[(size_t)j];
        CHECK(p.table[(size_t)j] == c.qkey[(size_t)i]);
        CHECK(p.table[(size_t)count + j] == c.limit[(size_t)i]);
        CHECK(p.table[2 * (size_t)count + j] == p.off[c.which[(size_t)i]]);
    }
    // the groups tile [0, count), none mixes lists, each has its own longest prefix; the partial rows are the running sum
    int next = 0;
    size_t rows = 0;
    for (const scl::NnGroup &g : p.groups) {
        CHECK(g.first == next && g.G >= 1 && g.G <= kGroup);
        CHECK(g.list == 0 || g.list == 1);
        CHECK(g.first >= p.seg[g.list] && g.first + g.G <= p.seg[g.list + 1]);
        CHECK(g.G == kGroup || g.first + g.G == p.seg[g.list + 1]);     // only a list's last group is short
        int n = 0;
        for (int j = g.first; j < g.first + g.G; ++j) n = std::max(n, p.table[(size_t)count + j]);
        CHECK(g.n == n);
        CHECK((size_t)g.tiles == ((size_t)n + kTile - 1) / kTile);
        if (c.k > 0) {
            for (int j = g.first; j < g.first + g.G; ++j)
                CHECK((size_t)p.table[3 * (size_t)count + j] == rows + (size_t)(j - g.first) * (size_t)g.tiles);
            rows += (size_t)g.G * (size_t)g.tiles;
        }
        next += g.G;
    }
    CHECK(next == count);
    CHECK(p.rows == rows);
    return p;
}

Call make_call(int count, int which_rule, int k)                  // which_rule 0: all list 0, 1: all list 1, 2: alternating from 0
{
    Call c;
    c.k = k;
    c.lists[0] = {kSomeKeys, 1000};
    c.lists[1] = {kSomeKeys, 1000};
    for (int i = 0; i < count; ++i) {
        c.qkey.push_back(5000 + 7 * i);
        c.limit.push_back((i * 37) % 1001);
        c.which.push_back(which_rule == 2 ? i & 1 : which_rule);
    }
    return c;
}

void group_sizes()
{
    for (int k : {0, 1, 10})
        for (int count : {1, 15, 16, 17, 33})
            for (int rule : {0, 1, 2}) {
                const scl::NnPlan p = checked_plan(make_call(count, rule, k));
                const int n0 = rule == 0 ? count : rule == 1 ? 0 : (count + 1) / 2, n1 = count - n0;
                CHECK(p.seg[1] == n0);
                CHECK((int)p.groups.size() == (n0 + kGroup - 1) / kGroup + (n1 + kGroup - 1) / kGroup);
            }
}

void list_offsets()
{
    Call c = make_call(17, 2, 0);
    scl::NnPlan p = checked_plan(c);
    CHECK(p.off[0] == 0 && p.off[1] == p.used[0] && p.keys == (size_t)p.used[0] + (size_t)p.used[1]);
    c.lists[0].keys = nullptr;                                     // keys 0 .. n - 1: nothing to upload, list 1 moves to the front
    p = checked_plan(c);
    CHECK(p.off[0] == -1 && p.off[1] == 0 && p.keys == (size_t)p.used[1]);
    c = make_call(17, 2, 4);
    for (int i = 1; i < 17; i += 2) c.limit[(size_t)i] = 0;        // no query of list 1 reaches a candidate
    p = checked_plan(c);
    CHECK(p.used[1] == 0 && p.off[1] == -1 && p.keys == (size_t)p.used[0]);
    for (const scl::NnGroup &g : p.groups)
        if (g.list == 1) CHECK(g.n == 0 && g.tiles == 0);
}

void group_prefix()
{
    Call c = make_call(33, 0, 0);
    for (int i = 0; i < 33; ++i) c.limit[(size_t)i] = i < 16 ? 0 : i < 32 ? 100 + i : 7;
    const scl::NnPlan p = checked_plan(c);
    CHECK(p.groups.size() == 3);
    CHECK(p.groups[0].n == 0 && p.groups[0].tiles == 0);           // every prefix empty: no launch
    CHECK(p.groups[1].n == 131 && p.groups[1].tiles == 3);         // its own longest prefix,
    CHECK(p.groups[2].n == 7 && p.groups[2].tiles == 1);           // not the call's
    CHECK(p.used[0] == 131);
}

void partial_rows()
{
    Call c = make_call(18, 0, 5);
    for (int i = 0; i < 18; ++i) c.limit[(size_t)i] = i < 16 ? 64 : 65;
    const scl::NnPlan p = checked_plan(c);
    CHECK(p.groups.size() == 2 && p.groups[0].tiles == 1 && p.groups[1].tiles == 2);
    CHECK(p.rows == 16 * 1 + 2 * 2);
    CHECK(p.table[3 * 18 + 15] == 15 && p.table[3 * 18 + 16] == 16 && p.table[3 * 18 + 17] == 18);
    c.k = 0;                                                       // the 1-NN form has no partial lists
    CHECK(checked_plan(c).rows == 0);
}

void guard()
{
    Call c = make_call(63, 0, 1);
    c.lists[0].n = INT_MAX;
    for (int &l : c.limit) l = INT_MAX;                            // 2^25 tiles each
    scl::NnPlan p = checked_plan(c);
    CHECK(p.rows == 2113929216u && p.rows == (size_t)63 << 25);
    CHECK(p.table[3 * 63 + 62] == 62 << 25);                       // the last query's first row still fits an int
    c = make_call(64, 0, 1);
    c.lists[0].n = INT_MAX;
    for (int &l : c.limit) l = INT_MAX;
    CHECK(!(scl::nn_plan<kGroup, kTile>(c.qkey.data(), c.limit.data(), c.which.data(), c.lists, 64, c.k, &p)));   // 64 * 2^25 = 2^31
    c.k = 0;                                                       // the 1-NN form keeps no partial lists: nothing to refuse
    checked_plan(c);
}

void empty_call()
{
    Call c = make_call(0, 0, 3);
    scl::NnPlan p = checked_plan(c);
    CHECK(p.order.empty() && p.table.empty() && p.groups.empty() && p.keys == 0 && p.rows == 0);
    CHECK((scl::nn_plan<kGroup, kTile>(nullptr, nullptr, nullptr, c.lists, 0, 0, &p)));
    CHECK(p.groups.empty());
}

}  // namespace

int main()
{
    group_sizes();
    list_offsets();
    group_prefix();
    partial_rows();
    guard();
    empty_call();
    std::puts("nn_plan_check: ok");
    return 0;
}
