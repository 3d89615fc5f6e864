// pgo_condense_plan.hpp -- the host-only plan of the condensed direct step of the pose-graph solve (contract: include/scl_engine.h
// "POSE-GRAPH SOLVE, CONDENSED DIRECT STEP"): which poses are interior and which are junctions, the segments, each segment's level
// schedule of block cyclic reduction, the junction numbering and the list of (junction, junction) blocks of S with their sources in
// the order they are added.  A pure function of the index arrays.  No HIP in here, so that tests/cpp/pgo_condense_plan_check.cpp can
// run it without a GPU.
#pragma once

#include <algorithm>
#include <vector>

#include "pgo_graph.hpp"

namespace scl {

// the sources of a block of S (PgoCondensePlan::src holds pairs kind, index)
enum { kSrcDiag = 0,       // the damped diagonal block of pose `index`
       kSrcW = 1,          // W of factor `index` as it is: the block's row is the junction of f_i
       kSrcWT = 2,         // W of factor `index` transposed: the block's row is the junction of f_j
       kSrcEnd = 3,        // the diagonal update left on end node `index` of a segment's path
       kSrcCouplingT = 4   // the coupling (left end, right end) left on node `index`, the first of a segment's path, transposed
};

struct PgoCondensePlan {
    int n_poses = 0, n_junctions = 0, n_segments = 0, longest_segment = 0, n_levels = 0, n_nodes = 0;
    std::vector<int> junction_of;      // pose -> its junction number, -1: interior
    std::vector<int> junction_pose;    // junction -> pose, ascending
    std::vector<int> seg_first, seg_last;   // the interior poses a..b of a segment, segments in ascending a
    // A segment's path [a - 1, a..b, b + 1] is b - a + 3 nodes; the paths lie one behind the other: node seg_node0[s] + t is pose a - 1 + t.
    std::vector<int> seg_node0;        // n_segments + 1
    std::vector<int> node_pose;        // n_nodes
    std::vector<int> node_coupling;    // n_nodes: 2 k + t, factor k joins the node's pose p with p + 1, t = 1: f_j[k] == p (W^T is the block
                                       // (p, p + 1)); -1 for the last node of a path
    // level l eliminates the nodes elim[3 e], e in [level_ptr[l], level_ptr[l + 1]), with the neighbours elim[3 e + 1] (left) and
    // elim[3 e + 2] (right); afterwards node absorb[3 e] takes the contribution of the eliminated node absorb[3 e + 1] on its left (-1:
    // none) and then of absorb[3 e + 2] on its right, e in [absorb_ptr[l], absorb_ptr[l + 1])
    std::vector<int> level_ptr, elim, absorb_ptr, absorb;
    // S: block b is (row junction block_rc[2 b], column junction block_rc[2 b + 1]), row >= column, blocks sorted by (row, column); its
    // sources src[2 s], src[2 s + 1] for s in [block_ptr[b], block_ptr[b + 1]) in the order of the contract
    std::vector<int> block_ptr, block_rc, src;
    // the right-hand side of junction j: -g of its pose, then the end nodes rhs_src[rhs_ptr[j] .. rhs_ptr[j + 1]) in ascending segment
    std::vector<int> rhs_ptr, rhs_src;
};

// The order in which a path of m nodes (both ends included, m >= 2) is reduced: level by level, every second survivor between the ends.
// f(level, position of the eliminated node, of its left and of its right neighbour).  Returns the number of levels.
template <class F>
inline int pgo_path_levels(int m, F f)
{
    std::vector<int> alive((size_t)m);
    for (int t = 0; t < m; ++t) alive[(size_t)t] = t;
    int level = 0;
    while (alive.size() > 2) {
        std::vector<int> next;
        const size_t cnt = alive.size();
        for (size_t p = 0; p < cnt; ++p) {
            if ((p & 1) && p + 1 < cnt) f(level, alive[p], alive[p - 1], alive[p + 1]);
            else next.push_back(alive[p]);
        }
        alive.swap(next);
        ++level;
    }
    return level;
}

// interior[k] = 1 where pose k's incident list is exactly two between factors, one to k - 1 and one to k + 1; toward[2 k], toward[2 k + 1]:
// the coupling codes (2 factor + t, as node_coupling) of (k - 1, k) and of (k, k + 1) for an interior k.  Indices must be in range.
inline void pgo_classify(int n_poses, const int *f_i, const int *f_j, int n_factors, const int *p_idx, int n_priors,
                         std::vector<char> *interior, std::vector<int> *toward)
{
    std::vector<int> row_ptr, entries;
    pgo_incidence(n_poses, f_i, f_j, n_factors, p_idx, n_priors, &row_ptr, &entries);
    interior->assign((size_t)n_poses, 0);
    toward->assign(2 * (size_t)n_poses, -1);
    for (int k = 0; k < n_poses; ++k) {
        const int beg = row_ptr[(size_t)k];
        if (row_ptr[(size_t)k + 1] - beg != 2) continue;
        int prev = -1, next = -1;
        bool ok = true;
        for (int e = 0; e < 2; ++e) {
            const int f = entries[(size_t)(beg + e)] >> 1, side = entries[(size_t)(beg + e)] & 1;
            if (f >= n_factors) { ok = false; break; }              // a prior
            const int other = side ? f_i[f] : f_j[f];
            // the block (lower pose, higher pose) is W where f_i is the lower pose, W^T otherwise
            if (other == k - 1 && prev < 0) prev = 2 * f + (side ? 0 : 1);
            else if (other == k + 1 && next < 0) next = 2 * f + (side ? 1 : 0);
            else ok = false;
        }
        if (ok && prev >= 0 && next >= 0) {
            (*interior)[(size_t)k] = 1;
            (*toward)[2 * (size_t)k] = prev; (*toward)[2 * (size_t)k + 1] = next;
        }
    }
}

// the counts alone (scl_pgo_count_junctions)
inline void pgo_count_junctions(int n_poses, const int *f_i, const int *f_j, int n_factors, const int *p_idx, int n_priors,
                                int *n_junctions, int *n_segments, int *longest_segment)
{
    std::vector<char> interior;
    std::vector<int> toward;
    pgo_classify(n_poses, f_i, f_j, n_factors, p_idx, n_priors, &interior, &toward);
    int nj = 0, ns = 0, longest = 0, run = 0;
    for (int k = 0; k < n_poses; ++k) {
        if (interior[(size_t)k]) { if (run++ == 0) ++ns; longest = std::max(longest, run); }
        else { ++nj; run = 0; }
    }
    *n_junctions = nj; *n_segments = ns; *longest_segment = longest;
}

inline void pgo_condense_plan(int n_poses, const int *f_i, const int *f_j, int n_factors, const int *p_idx, int n_priors, PgoCondensePlan *out)
{
    PgoCondensePlan &P = *out;
    P = PgoCondensePlan();
    P.n_poses = n_poses;
    std::vector<char> interior;
    std::vector<int> toward;
    pgo_classify(n_poses, f_i, f_j, n_factors, p_idx, n_priors, &interior, &toward);
    P.junction_of.assign((size_t)n_poses, -1);
    for (int k = 0; k < n_poses; ++k)
        if (!interior[(size_t)k]) { P.junction_of[(size_t)k] = (int)P.junction_pose.size(); P.junction_pose.push_back(k); }
    P.n_junctions = (int)P.junction_pose.size();
    // segments and their paths
    P.seg_node0.push_back(0);
    for (int k = 0; k < n_poses;) {
        if (!interior[(size_t)k]) { ++k; continue; }
        int b = k;
        while (interior[(size_t)b + 1]) ++b;                         // an interior pose has a pose behind it
        P.seg_first.push_back(k); P.seg_last.push_back(b);
        P.longest_segment = std::max(P.longest_segment, b - k + 1);
        for (int p = k - 1; p <= b + 1; ++p) {
            P.node_pose.push_back(p);
            P.node_coupling.push_back(p == b + 1 ? -1 : (p == k - 1 ? toward[2 * (size_t)k] : toward[2 * (size_t)p + 1]));
        }
        P.seg_node0.push_back((int)P.node_pose.size());
        k = b + 1;
    }
    P.n_segments = (int)P.seg_first.size();
    P.n_nodes = (int)P.node_pose.size();
    // the level schedule: every segment's own order, the segments of a level one behind the other
    std::vector<std::vector<int>> lev_elim, lev_absorb;
    for (int s = 0; s < P.n_segments; ++s) {
        const int n0 = P.seg_node0[(size_t)s], m = P.seg_node0[(size_t)s + 1] - n0;
        std::vector<std::vector<int>> mine;                          // per level: eliminated node, left, right (path positions)
        const int levels = pgo_path_levels(m, [&](int l, int node, int left, int right) {
            if ((int)mine.size() <= l) mine.resize((size_t)l + 1);
            mine[(size_t)l].insert(mine[(size_t)l].end(), {node, left, right});
        });
        if ((int)lev_elim.size() < levels) { lev_elim.resize((size_t)levels); lev_absorb.resize((size_t)levels); }
        for (int l = 0; l < levels; ++l) {
            const std::vector<int> &e = mine[(size_t)l];
            std::vector<int> &E = lev_elim[(size_t)l], &A = lev_absorb[(size_t)l];
            for (size_t q = 0; q < e.size(); q += 3) {
                E.insert(E.end(), {n0 + e[q], n0 + e[q + 1], n0 + e[q + 2]});
                // the survivor on the left of this node: its left contribution is the node eliminated before it, if that one's right is it
                const bool shared = q >= 3 && e[q - 1] == e[q + 1];
                if (shared) A[A.size() - 1] = n0 + e[q];              // the entry of the survivor between the two
                else A.insert(A.end(), {n0 + e[q + 1], -1, n0 + e[q]});
                A.insert(A.end(), {n0 + e[q + 2], n0 + e[q], -1});
            }
        }
    }
    P.n_levels = (int)lev_elim.size();
    P.level_ptr.push_back(0); P.absorb_ptr.push_back(0);
    for (int l = 0; l < P.n_levels; ++l) {
        P.elim.insert(P.elim.end(), lev_elim[(size_t)l].begin(), lev_elim[(size_t)l].end());
        P.absorb.insert(P.absorb.end(), lev_absorb[(size_t)l].begin(), lev_absorb[(size_t)l].end());
        P.level_ptr.push_back((int)P.elim.size() / 3); P.absorb_ptr.push_back((int)P.absorb.size() / 3);
    }
    // the blocks of S.  Candidates (row, column, order key, kind, index) sorted by (row, column, key): the key puts the diagonal first,
    // then the factors by number, then the segments by number.
    struct Cand { int row, col; long long key; int kind, index; };
    std::vector<Cand> cand;
    for (int j = 0; j < P.n_junctions; ++j) cand.push_back({j, j, -1, kSrcDiag, P.junction_pose[(size_t)j]});
    for (int k = 0; k < n_factors; ++k) {
        const int a = P.junction_of[(size_t)f_i[k]], b = P.junction_of[(size_t)f_j[k]];
        if (a < 0 || b < 0) continue;
        if (a > b) cand.push_back({a, b, (long long)k, kSrcW, k});
        else cand.push_back({b, a, (long long)k, kSrcWT, k});
    }
    std::vector<std::vector<int>> rhs((size_t)P.n_junctions);
    for (int s = 0; s < P.n_segments; ++s) {
        const int n0 = P.seg_node0[(size_t)s], n1 = P.seg_node0[(size_t)s + 1] - 1;
        const int ja = P.junction_of[(size_t)P.node_pose[(size_t)n0]], jb = P.junction_of[(size_t)P.node_pose[(size_t)n1]];
        const long long key = (long long)n_factors + s;
        cand.push_back({ja, ja, key, kSrcEnd, n0});
        cand.push_back({jb, jb, key, kSrcEnd, n1});
        cand.push_back({jb, ja, key, kSrcCouplingT, n0});
        rhs[(size_t)ja].push_back(n0); rhs[(size_t)jb].push_back(n1);
    }
    std::stable_sort(cand.begin(), cand.end(), [](const Cand &x, const Cand &y) {
        if (x.row != y.row) return x.row < y.row;
        if (x.col != y.col) return x.col < y.col;
        return x.key < y.key;
    });
    for (size_t c = 0; c < cand.size(); ++c) {
        if (c == 0 || cand[c].row != cand[c - 1].row || cand[c].col != cand[c - 1].col) {
            P.block_ptr.push_back((int)c);
            P.block_rc.push_back(cand[c].row); P.block_rc.push_back(cand[c].col);
        }
        P.src.push_back(cand[c].kind); P.src.push_back(cand[c].index);
    }
    P.block_ptr.push_back((int)cand.size());
    P.rhs_ptr.push_back(0);
    for (int j = 0; j < P.n_junctions; ++j) {
        P.rhs_src.insert(P.rhs_src.end(), rhs[(size_t)j].begin(), rhs[(size_t)j].end());
        P.rhs_ptr.push_back((int)P.rhs_src.size());
    }
}

}  // namespace scl
