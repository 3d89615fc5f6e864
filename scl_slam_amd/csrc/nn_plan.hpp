// nn_plan.hpp -- the PLAN of a batched nearest-neighbour search of the vector plugins, host code only (no HIP): what
// plugin_host.hpp's driver allocates, uploads and launches is decided here from the queries alone, by arithmetic, so that
// tests/cpp/nn_plan_check.cpp can run it under ASan / UBSan and past sizes no test could allocate.  Internal linkage, as everything
// of the plugins' host layer: the library exports nothing of it.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace scl {
namespace {

// a candidate list of a batched search: n global keys, keys == nullptr for keys 0 .. n - 1
struct NnList {
    const int *keys;
    int n;
};

// one launch: queries [first, first + G) of the grouped order, all of list `list`, against the prefix [0, n) of it -- n the longest
// of the group's own limits, `tiles` tiles of candidates.  n == 0 (every prefix of the group empty): nothing is launched
struct NnGroup {
    int list, first, G, n, tiles;
};

struct NnPlan {
    std::vector<int> order;              // grouped position j holds the caller's query order[j]: list 0's queries first, stable
    int seg[3] = {0, 0, 0};              // list l's queries are [seg[l], seg[l + 1]) of the grouped order
    int used[2] = {0, 0};                // the longest prefix of list l that a query reaches
    int off[2] = {-1, -1};               // where that prefix goes in the device list; -1: nothing uploaded (no keys, or nothing reached)
    size_t keys = 0;                     // the device list's ints: the uploaded prefixes one after the other
    int cols = 3;                        // the table's columns, `count` ints each, in the grouped order:
    std::vector<int> table;              //   qkey | limit | list_off [| part_row, for k > 0]
    std::vector<NnGroup> groups;
    size_t rows = 0;                     // k > 0: the partial lists' rows, [query][tile] group after group; part_row: a query's first
};

// The plan of `count` queries, query i being row qkey[i] against the prefix [0, limit[i]) of lists[which[i]] (0 <= limit[i] <= its
// n), in launch groups of up to GROUP queries over tiles of TILE candidates; k == 0 for the 1-NN form, else the length of the lists.
// False: the partial lists pass 2^31 rows (k > 0 only; part_row is an int) -- found by arithmetic, before anything is sized by it
template <int GROUP, int TILE>
bool nn_plan(const int *qkey, const int *limit, const int *which, const NnList lists[2], int count, int k, NnPlan *p)
{
    *p = NnPlan();
    p->cols = k > 0 ? 4 : 3;
    if (count <= 0) return true;
    p->seg[2] = count;
    for (int i = 0; i < count; ++i) {
        p->seg[1] += which[i] == 0;
        p->used[which[i]] = std::max(p->used[which[i]], limit[i]);
    }
    p->order.resize((size_t)count);
    for (int i = 0, a = 0, b = p->seg[1]; i < count; ++i) p->order[(size_t)(which[i] == 0 ? a++ : b++)] = i;
    for (int l = 0; l < 2; ++l)
        if (lists[l].keys && p->used[l] > 0) { p->off[l] = (int)p->keys; p->keys += (size_t)p->used[l]; }
    p->table.resize((size_t)p->cols * (size_t)count);
    int *t_qkey = p->table.data(), *t_limit = t_qkey + count, *t_off = t_limit + count;
    for (int j = 0; j < count; ++j) {
        const int i = p->order[(size_t)j];
        t_qkey[j] = qkey[i]; t_limit[j] = limit[i]; t_off[j] = p->off[which[i]];
    }
    for (int l = 0; l < 2; ++l)
        for (int s = p->seg[l]; s < p->seg[l + 1]; s += GROUP) {
            const int G = std::min(GROUP, p->seg[l + 1] - s);
            int n = 0;
            for (int j = s; j < s + G; ++j) n = std::max(n, t_limit[j]);
            const size_t tiles = ((size_t)n + TILE - 1) / TILE;
            if (k > 0) {                                               // a group's partials: [query][tile][k] over the tiles of n
                if (p->rows + (size_t)G * tiles > (size_t)INT32_MAX) return false;
                for (int j = s; j < s + G; ++j) t_off[count + j] = (int)(p->rows + (size_t)(j - s) * tiles);
                p->rows += (size_t)G * tiles;
            }
            p->groups.push_back({l, s, G, n, (int)tiles});
        }
    return true;
}

}  // namespace
}  // namespace scl
