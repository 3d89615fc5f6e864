// pgo_graph_check -- the host-only graph work of the pose-graph solve (scl_slam_amd/csrc/pgo_graph.hpp) as a program of its own, built
// with ASan + UBSan (Makefile).  Reads graphs from standard input until it ends:
//     n_poses n_factors n_priors   f_i f_j (n_factors pairs)   p_idx (n_priors)
// and answers each with one line "bad: <what pgo_graph_bad says>" or "ok", and for an accepted graph a line "row_ptr ..." and a line
// "entries ..." of pgo_incidence.  tests/test_pgo_abi.py holds the answers to its own union-find and counting sort.
#include <cstdio>
#include <vector>

#include "pgo_graph.hpp"

int main()
{
    int n, F, P;
    while (std::scanf("%d %d %d", &n, &F, &P) == 3) {
        if (n < 1 || F < 0 || P < 0 || n > (1 << 22) || F > (1 << 23) || P > (1 << 22)) return 2;
        std::vector<int> fi((size_t)F), fj((size_t)F), pi((size_t)P);
        for (int k = 0; k < F; ++k)
            if (std::scanf("%d %d", &fi[(size_t)k], &fj[(size_t)k]) != 2) return 2;
        for (int m = 0; m < P; ++m)
            if (std::scanf("%d", &pi[(size_t)m]) != 1) return 2;
        if (const char *bad = scl::pgo_graph_bad(n, fi.data(), fj.data(), F, pi.data(), P)) {
            std::printf("bad: %s\n", bad);
            continue;
        }
        std::vector<int> row_ptr, entries;
        scl::pgo_incidence(n, fi.data(), fj.data(), F, pi.data(), P, &row_ptr, &entries);
        std::printf("ok\nrow_ptr");
        for (int v : row_ptr) std::printf(" %d", v);
        std::printf("\nentries");
        for (int v : entries) std::printf(" %d", v);
        std::printf("\n");
    }
    return 0;
}
