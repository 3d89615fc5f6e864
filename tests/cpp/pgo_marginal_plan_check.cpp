// pgo_marginal_plan_check -- the host-only plan of the many-column solve and the marginals (scl_slam_amd/csrc/pgo_marginal_plan.hpp) as
// a program of its own, built with ASan + UBSan (Makefile).  Reads requests from standard input until it ends:
//     group n_poses n_nodes n_columns          -> "group <columns per group> <n_groups> first:count ..."
//     select n_poses n_queries  q_i q_j (pairs) -> "select <n_sel> sel ... | u_i:u_j ..." or "refused <why>"
// The checks a plan must pass whatever the request -- the groups tile [0, n_columns) in order, a group's arrays stay within the budget
// unless the group is the minimum of 6, every position names the query's pose, a refusal writes nothing -- are made here and end the
// program with status 3.  tests/test_pgo_marginals_abi.py holds the figures to the rule restated in Python.
#include <cstdio>
#include <cstring>
#include <vector>

#include "pgo_marginal_plan.hpp"

static int fail(const char *what)
{
    std::printf("plan broken: %s\n", what);
    return 3;
}

int main()
{
    char word[16];
    while (std::scanf("%15s", word) == 1) {
        if (!std::strcmp(word, "group")) {
            int n, nodes, cols;
            if (std::scanf("%d %d %d", &n, &nodes, &cols) != 3 || n < 1 || nodes < 0 || cols < 1 || cols > scl::kMargMaxColumns) return 2;
            const int group = scl::pgo_marginal_group_columns(n, nodes);
            if (group < scl::kMargMinGroup || group > scl::kMargMaxColumns) return fail("group out of range");
            if (group >= scl::kMargTile && group % scl::kMargTile) return fail("a group of 16 or more that is no multiple of 16");
            if (group > scl::kMargMinGroup && (size_t)group * scl::pgo_marginal_column_bytes(n, nodes) > scl::kMargBudgetBytes)
                return fail("a group above the minimum that exceeds the budget");
            std::vector<int> firsts, counts;
            int next = 0;
            for (int g = 0;; ++g) {
                int first, count;
                scl::pgo_marginal_group(cols, group, g, &first, &count);
                if (count <= 0) break;
                if (first != next || count > group) return fail("groups do not tile the columns");
                next = first + count;
                firsts.push_back(first); counts.push_back(count);
            }
            if (next != cols) return fail("groups do not cover the columns");
            std::printf("group %d %zu", group, firsts.size());
            for (size_t g = 0; g < firsts.size(); ++g) std::printf(" %d:%d", firsts[g], counts[g]);
            std::printf("\n");
        } else if (!std::strcmp(word, "select")) {
            int n, nq;
            if (std::scanf("%d %d", &n, &nq) != 2 || n < 1 || nq < 0 || nq > (1 << 20)) return 2;
            std::vector<int> qi((size_t)nq), qj((size_t)nq);
            for (int k = 0; k < nq; ++k)
                if (std::scanf("%d %d", &qi[(size_t)k], &qj[(size_t)k]) != 2) return 2;
            std::vector<int> sel = {-7}, ui = {-7}, uj = {-7};
            const char *bad = scl::pgo_marginal_select(qi.data(), qj.data(), nq, n, &sel, &ui, &uj);
            if (bad) {
                if (sel != std::vector<int>{-7} || ui != std::vector<int>{-7} || uj != std::vector<int>{-7}) return fail("a refusal wrote");
                std::printf("refused %s\n", bad);
                continue;
            }
            if ((int)ui.size() != nq || (int)uj.size() != nq || (int)sel.size() > scl::kMargMaxPoses) return fail("sizes");
            for (size_t s = 1; s < sel.size(); ++s)
                if (sel[s - 1] >= sel[s]) return fail("selection not ascending");
            for (int k = 0; k < nq; ++k) {
                const int a = ui[(size_t)k], b = uj[(size_t)k];
                if (a < 0 || a >= (int)sel.size() || b < 0 || b >= (int)sel.size()) return fail("a position out of range");
                if (sel[(size_t)a] != qi[(size_t)k] || sel[(size_t)b] != qj[(size_t)k]) return fail("a position names another pose");
            }
            std::printf("select %zu", sel.size());
            for (int v : sel) std::printf(" %d", v);
            std::printf(" |");
            for (int k = 0; k < nq; ++k) std::printf(" %d:%d", ui[(size_t)k], uj[(size_t)k]);
            std::printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
