// pgo_marginal_plan.hpp -- the host-only plan of the many-column solve and of the marginals of the pose-graph solve (contract:
// include/scl_engine.h "POSE-GRAPH SOLVE, MANY RIGHT-HAND SIDES AND MARGINAL COVARIANCES"): how many columns run in one group, and
// which poses a list of queries names.  Pure functions.  No HIP in here, so that tests/cpp/pgo_marginal_plan_check.cpp can run them
// without a GPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

namespace scl {

constexpr int kMargTile = 16;                              // columns of one workgroup of the dense triangular solves
constexpr int kMargMinGroup = 6;                           // one pose's unit columns
constexpr int kMargMaxColumns = 1536;                      // SCL_PGO_MAX_RHS
constexpr int kMargMaxPoses = 256;                         // SCL_PGO_MAX_MARGINAL_POSES
constexpr size_t kMargBudgetBytes = (size_t)256 << 20;     // of a group's per-column arrays
constexpr int kMargNodeDoubles = 18;                       // per path node and column: b / w / x (6), the left slot (6), the right slot (6)

// bytes of one column in a group: its row of the solution and its share of the node arrays
inline size_t pgo_marginal_column_bytes(int n_poses, int n_nodes)
{
    return sizeof(double) * ((size_t)6 * (size_t)n_poses + (size_t)kMargNodeDoubles * (size_t)n_nodes);
}

// Columns per group: as many as the budget holds, never fewer than 6 nor more than 1536; from 16 on a multiple of 16, so that only a
// group's last tile can be a partial one.  By the contract's core rule the figure cannot change a bit of any column.
inline int pgo_marginal_group_columns(int n_poses, int n_nodes)
{
    size_t c = kMargBudgetBytes / pgo_marginal_column_bytes(n_poses, n_nodes);
    if (c > (size_t)kMargMaxColumns) c = (size_t)kMargMaxColumns;
    if (c >= (size_t)kMargTile) c -= c % (size_t)kMargTile;
    if (c < (size_t)kMargMinGroup) c = (size_t)kMargMinGroup;
    return (int)c;
}

// group g of n_columns columns in groups of `group`: its first column and its count (0 behind the last group)
inline void pgo_marginal_group(int n_columns, int group, int g, int *first, int *count)
{
    const long long f = (long long)g * group;
    *first = f < n_columns ? (int)f : n_columns;
    *count = std::min(group, n_columns - *first);
}

// The distinct poses named by q_i and q_j in ascending order (sel), and for every query the positions of its two poses in sel.
// nullptr, or what is wrong: nothing is written then.
inline const char *pgo_marginal_select(const int *q_i, const int *q_j, int n_queries, int n_poses, std::vector<int> *sel,
                                       std::vector<int> *u_i, std::vector<int> *u_j)
{
    if (!q_i || !q_j) return "q_i or q_j is NULL";
    for (int k = 0; k < n_queries; ++k)
        if (q_i[k] < 0 || q_i[k] >= n_poses || q_j[k] < 0 || q_j[k] >= n_poses) return "a query index out of range";
    std::vector<int> all;
    all.reserve(2 * (size_t)n_queries);
    for (int k = 0; k < n_queries; ++k) { all.push_back(q_i[k]); all.push_back(q_j[k]); }
    std::sort(all.begin(), all.end());
    all.erase(std::unique(all.begin(), all.end()), all.end());
    if (all.size() > (size_t)kMargMaxPoses) return "more than 256 distinct query poses";
    std::vector<int> ui((size_t)n_queries), uj((size_t)n_queries);
    for (int k = 0; k < n_queries; ++k) {
        ui[(size_t)k] = (int)(std::lower_bound(all.begin(), all.end(), q_i[k]) - all.begin());
        uj[(size_t)k] = (int)(std::lower_bound(all.begin(), all.end(), q_j[k]) - all.begin());
    }
    sel->swap(all); u_i->swap(ui); u_j->swap(uj);
    return nullptr;
}

}  // namespace scl
