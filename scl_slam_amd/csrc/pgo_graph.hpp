// pgo_graph.hpp -- the host-only graph work of the pose-graph solve (contract: include/scl_engine.h "POSE-GRAPH SOLVE"): the check that
// every connected component holds a prior, and the pose -> incident (factor, side) lists the device gathers over.  No HIP in here, so
// that tests/cpp/pgo_graph_check.cpp can run it without a GPU.
#pragma once

#include <numeric>
#include <vector>

namespace scl {

// nullptr, or what is wrong with the indices: one out of range, f_i == f_j, or a connected component without a prior (union-find over
// the between factors, by size with path halving)
inline const char *pgo_graph_bad(int n_poses, const int *f_i, const int *f_j, int n_factors, const int *p_idx, int n_priors)
{
    for (int k = 0; k < n_factors; ++k) {
        if (f_i[k] < 0 || f_i[k] >= n_poses || f_j[k] < 0 || f_j[k] >= n_poses) return "a factor's pose index out of range";
        if (f_i[k] == f_j[k]) return "a factor between a pose and itself";
    }
    for (int m = 0; m < n_priors; ++m)
        if (p_idx[m] < 0 || p_idx[m] >= n_poses) return "a prior's pose index out of range";
    std::vector<int> parent((size_t)n_poses), size((size_t)n_poses, 1);
    std::iota(parent.begin(), parent.end(), 0);
    auto find = [&](int v) {
        while (parent[(size_t)v] != v) { parent[(size_t)v] = parent[(size_t)parent[(size_t)v]]; v = parent[(size_t)v]; }
        return v;
    };
    for (int k = 0; k < n_factors; ++k) {
        int a = find(f_i[k]), b = find(f_j[k]);
        if (a == b) continue;
        if (size[(size_t)a] < size[(size_t)b]) { const int t = a; a = b; b = t; }
        parent[(size_t)b] = a; size[(size_t)a] += size[(size_t)b];
    }
    std::vector<char> anchored((size_t)n_poses, 0);
    for (int m = 0; m < n_priors; ++m) anchored[(size_t)find(p_idx[m])] = 1;
    for (int v = 0; v < n_poses; ++v)
        if (!anchored[(size_t)find(v)]) return "a connected component without a prior";
    return nullptr;
}

// Factors are numbered between factors first, then priors (prior m is factor n_factors + m).  Entry 2 k + side says that the pose is
// side 0 (i) or 1 (j; a prior's only side) of factor k.  row_ptr (n_poses + 1) and entries (2 n_factors + n_priors) by a counting sort
// by pose, which is stable: every pose's list is in ascending factor number.
inline void pgo_incidence(int n_poses, const int *f_i, const int *f_j, int n_factors, const int *p_idx, int n_priors,
                          std::vector<int> *row_ptr, std::vector<int> *entries)
{
    row_ptr->assign((size_t)n_poses + 1, 0);
    for (int k = 0; k < n_factors; ++k) { ++(*row_ptr)[(size_t)f_i[k] + 1]; ++(*row_ptr)[(size_t)f_j[k] + 1]; }
    for (int m = 0; m < n_priors; ++m) ++(*row_ptr)[(size_t)p_idx[m] + 1];
    for (int v = 0; v < n_poses; ++v) (*row_ptr)[(size_t)v + 1] += (*row_ptr)[(size_t)v];
    entries->assign((size_t)(*row_ptr)[(size_t)n_poses], 0);
    std::vector<int> fill(row_ptr->begin(), row_ptr->end() - 1);
    for (int k = 0; k < n_factors; ++k) {
        (*entries)[(size_t)fill[(size_t)f_i[k]]++] = 2 * k;
        (*entries)[(size_t)fill[(size_t)f_j[k]]++] = 2 * k + 1;
    }
    for (int m = 0; m < n_priors; ++m) (*entries)[(size_t)fill[(size_t)p_idx[m]]++] = 2 * (n_factors + m) + 1;
}

}  // namespace scl
