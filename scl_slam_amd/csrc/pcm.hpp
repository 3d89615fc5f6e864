// pcm.hpp -- pairwise consistency of loop closures on the GPU (host-side interface used by engine.hip; contract:
// include/scl_engine.h "PAIRWISE CONSISTENCY OF LOOP CLOSURES").
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "scl_engine.h"

namespace scl {

constexpr int kPcmMaxLoops = 4096;             // W = 64 words of adjacency per row: one word per lane of the clique kernel's wave

// Grow-only.  Nothing a call reads was left by an earlier one: the inputs are copied in, and every word of the n x W adjacency, every
// degree, every entry of the n x n matrix, every seed's record and the result are written by the call's own kernels before they are read.
struct PcmWorkspace {
    enum { B_POSES_A = 0, B_POSES_B, B_IDX_A, B_IDX_B, B_Z, B_COV, B_ODOM, B_PREP_A, B_PREP_B, B_LOOPS, B_UPPER, B_ADJ, B_DEGREE, B_D2,
           B_SETS, B_SIZES, B_BEST, B_RESULT, B_COUNT };
    void *buf[B_COUNT] = {nullptr};
    size_t cap[B_COUNT] = {0};
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // timed calls (timing != 0): around the matrix kernels, around the clique kernels
    double pairs_ms = 0.0, clique_ms = 0.0;                    // of the last timed call (0: that stage did not run)
};

void pcm_workspace_free(PcmWorkspace *ws);

struct PcmInputs {
    const double *poses_a; int n_a; const double *poses_b; int n_b;
    const int *idx_a; const int *idx_b; const double *z; const double *cov; int n_loops;
    const double *odom_var; double threshold;
};

// nullptr, or what is wrong with the arguments (checked on the host before anything runs)
const char *pcm_inputs_bad(const PcmInputs &in);
const char *pcm_graph_bad(const uint64_t *adj, int n);

// The matrix and the graph (d2, adj, degree: each may be nullptr), then -- members != nullptr -- the clique of that graph without the graph
// leaving the device.  n_loops >= 1, arguments checked by the caller.  Waits for the stream before it returns.
int pcm_consistency(PcmWorkspace *ws, hipStream_t stream, const PcmInputs &in, double *d2, uint64_t *adj, int *degree,
                    int *members, int *n_members, int *seed, bool timing, std::string *err);
// the clique of a graph from the host (n >= 1, checked by the caller)
int pcm_max_clique(PcmWorkspace *ws, hipStream_t stream, const uint64_t *adj, int n, int *members, int *n_members, int *seed,
                   bool timing, std::string *err);

}  // namespace scl
