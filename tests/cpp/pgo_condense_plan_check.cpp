// pgo_condense_plan_check -- the host-only plan of the condensed direct step (scl_slam_amd/csrc/pgo_condense_plan.hpp) as a program of
// its own, built with ASan + UBSan (Makefile).  Reads graphs from standard input until it ends:
//     n_poses n_factors n_priors   f_i f_j (n_factors pairs)   p_idx (n_priors)
// and answers each (indices in range: the caller's business) with the lines
//     counts <n_junctions> <n_segments> <longest_segment> <n_levels> <n_nodes>     (pgo_count_junctions must agree, or "counts differ")
//     junctions ...            the junctions' poses
//     segments a b ...         pairs
//     couplings ...            node_coupling of every node
//     level <l> m l r ...      per level the eliminated nodes with their neighbours, as path positions p:s (position p of segment s)
//     absorb <l> s le re ...   per level the survivors with the eliminated node on their left and right (-1: none), the same way
//     block r c kind:index ... per block of S
//     rhs j node ...           per junction with an end node
// The checks a plan must pass whatever the graph -- every index in range, every node eliminated exactly once, no node written twice in a
// level -- are made here and end the program with status 3.  tests/test_pgo_condensed_abi.py holds the rest to tests/pgo_condensed_cases.py.
#include <cstdio>
#include <string>
#include <vector>

#include "pgo_condense_plan.hpp"

static int fail(const char *what)
{
    std::printf("plan broken: %s\n", what);
    return 3;
}

int main()
{
    int n, F, Pn;
    while (std::scanf("%d %d %d", &n, &F, &Pn) == 3) {
        if (n < 1 || F < 0 || Pn < 0 || n > (1 << 22) || F > (1 << 23) || Pn > (1 << 22)) return 2;
        std::vector<int> fi((size_t)F), fj((size_t)F), pi((size_t)Pn);
        for (int k = 0; k < F; ++k)
            if (std::scanf("%d %d", &fi[(size_t)k], &fj[(size_t)k]) != 2) return 2;
        for (int m = 0; m < Pn; ++m)
            if (std::scanf("%d", &pi[(size_t)m]) != 1) return 2;
        scl::PgoCondensePlan P;
        scl::pgo_condense_plan(n, fi.data(), fj.data(), F, pi.data(), Pn, &P);
        int nj = -1, ns = -1, longest = -1;
        scl::pgo_count_junctions(n, fi.data(), fj.data(), F, pi.data(), Pn, &nj, &ns, &longest);
        if (nj != P.n_junctions || ns != P.n_segments || longest != P.longest_segment) return fail("counts differ");
        // the path position p:s of a node
        std::vector<int> seg_of((size_t)P.n_nodes);
        for (int s = 0; s < P.n_segments; ++s)
            for (int i = P.seg_node0[(size_t)s]; i < P.seg_node0[(size_t)s + 1]; ++i) seg_of[(size_t)i] = s;
        auto name = [&](int node) {
            if (node < 0) return std::string("-1");
            const int s = seg_of[(size_t)node];
            return std::to_string(node - P.seg_node0[(size_t)s]) + ":" + std::to_string(s);
        };
        auto in_nodes = [&](int v) { return v >= 0 && v < P.n_nodes; };
        std::vector<int> eliminated((size_t)P.n_nodes, 0);
        if ((int)P.level_ptr.size() != P.n_levels + 1 || (int)P.absorb_ptr.size() != P.n_levels + 1) return fail("level pointers");
        if ((int)P.node_pose.size() != P.n_nodes || (int)P.node_coupling.size() != P.n_nodes) return fail("node arrays");
        std::printf("counts %d %d %d %d %d\njunctions", P.n_junctions, P.n_segments, P.longest_segment, P.n_levels, P.n_nodes);
        for (int v : P.junction_pose) std::printf(" %d", v);
        std::printf("\nsegments");
        for (int s = 0; s < P.n_segments; ++s) std::printf(" %d %d", P.seg_first[(size_t)s], P.seg_last[(size_t)s]);
        std::printf("\ncouplings");
        for (int i = 0; i < P.n_nodes; ++i) {
            const int c = P.node_coupling[(size_t)i];
            if (c >= 2 * F) return fail("a coupling's factor");
            if (c >= 0) {
                const int k = c >> 1, lo = (c & 1) ? fj[(size_t)k] : fi[(size_t)k], hi = (c & 1) ? fi[(size_t)k] : fj[(size_t)k];
                if (lo != P.node_pose[(size_t)i] || hi != lo + 1) return fail("a coupling's poses");
            }
            std::printf(" %d", c);
        }
        std::printf("\n");
        for (int l = 0; l < P.n_levels; ++l) {
            std::vector<int> written((size_t)P.n_nodes, 0);
            std::printf("level %d", l);
            for (int e = P.level_ptr[(size_t)l]; e < P.level_ptr[(size_t)l + 1]; ++e) {
                const int m = P.elim[3 * (size_t)e], lf = P.elim[3 * (size_t)e + 1], r = P.elim[3 * (size_t)e + 2];
                if (!in_nodes(m) || !in_nodes(lf) || !in_nodes(r)) return fail("an eliminated node out of range");
                if (eliminated[(size_t)m]++ || eliminated[(size_t)lf] || eliminated[(size_t)r]) return fail("a node eliminated twice, or a neighbour that is gone");
                if (P.junction_of[(size_t)P.node_pose[(size_t)m]] >= 0) return fail("an end eliminated");
                // the launch writes node m and the coupling of its left neighbour: each once per level
                if (written[(size_t)m]++ || written[(size_t)lf]++) return fail("a node written twice in a level");
                std::printf(" %s %s %s", name(m).c_str(), name(lf).c_str(), name(r).c_str());
            }
            std::printf("\nabsorb %d", l);
            std::vector<int> absorbed((size_t)P.n_nodes, 0);
            for (int e = P.absorb_ptr[(size_t)l]; e < P.absorb_ptr[(size_t)l + 1]; ++e) {
                const int s = P.absorb[3 * (size_t)e], le = P.absorb[3 * (size_t)e + 1], re = P.absorb[3 * (size_t)e + 2];
                if (!in_nodes(s) || le >= P.n_nodes || re >= P.n_nodes || le < -1 || re < -1) return fail("an absorb entry out of range");
                if (eliminated[(size_t)s] || absorbed[(size_t)s]++) return fail("a survivor that is gone, or listed twice");
                std::printf(" %s %s %s", name(s).c_str(), name(le).c_str(), name(re).c_str());
            }
            std::printf("\n");
        }
        for (int i = 0; i < P.n_nodes; ++i)
            if (eliminated[(size_t)i] != (P.junction_of[(size_t)P.node_pose[(size_t)i]] < 0 ? 1 : 0)) return fail("an interior node never eliminated");
        const int nb = (int)P.block_rc.size() / 2;
        if ((int)P.block_ptr.size() != nb + 1) return fail("block pointers");
        for (int b = 0; b < nb; ++b) {
            const int r = P.block_rc[2 * (size_t)b], c = P.block_rc[2 * (size_t)b + 1];
            if (r < 0 || r >= P.n_junctions || c < 0 || c > r) return fail("a block outside the lower triangle");
            std::printf("block %d %d", r, c);
            for (int s = P.block_ptr[(size_t)b]; s < P.block_ptr[(size_t)b + 1]; ++s) {
                const int kind = P.src[2 * (size_t)s], idx = P.src[2 * (size_t)s + 1];
                const int limit = kind == scl::kSrcDiag ? n : (kind == scl::kSrcW || kind == scl::kSrcWT) ? F : P.n_nodes;
                if (idx < 0 || idx >= limit) return fail("a source out of range");
                if (kind == scl::kSrcEnd || kind == scl::kSrcCouplingT) std::printf(" %d:%s", kind, name(idx).c_str());
                else std::printf(" %d:%d", kind, idx);
            }
            std::printf("\n");
        }
        if ((int)P.rhs_ptr.size() != P.n_junctions + 1) return fail("rhs pointers");
        for (int j = 0; j < P.n_junctions; ++j) {
            if (P.rhs_ptr[(size_t)j] == P.rhs_ptr[(size_t)j + 1]) continue;
            std::printf("rhs %d", j);
            for (int s = P.rhs_ptr[(size_t)j]; s < P.rhs_ptr[(size_t)j + 1]; ++s) {
                if (!in_nodes(P.rhs_src[(size_t)s])) return fail("an rhs source out of range");
                std::printf(" %s", name(P.rhs_src[(size_t)s]).c_str());
            }
            std::printf("\n");
        }
        std::printf("end\n");
    }
    return 0;
}
