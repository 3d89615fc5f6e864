// pgo.hpp -- the pose-graph solve on the GPU (host-side interface used by engine.hip; contract: include/scl_engine.h "POSE-GRAPH SOLVE").
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "scl_engine.h"

namespace scl {

constexpr int kPgoLongRow = 64;                // a pose with this many incident factors or more is summed by a wave, not by one thread

// Grow-only.  Nothing a call reads was left by an earlier one: the inputs are copied in, and every kernel's inputs are written by the
// kernels queued in front of it in the same call.
struct PgoWorkspace {
    enum { B_POSES_IN = 0, B_Z_IN, B_COV_IN, B_FI, B_FJ, B_ROWPTR, B_ENTRIES, B_X0, B_X1, B_FPREP, B_FAC0, B_FAC1, B_G0, B_G1, B_D0, B_D1,
           B_LBLK, B_VX, B_VR, B_VZ, B_VQ, B_VP0, B_VP1, B_PART_COST, B_PART_GMAX, B_PART_RZ0, B_PART_RZ1, B_PART_PQ, B_PART_STEP, B_REC,
           B_XIN, B_POSES_OUT, B_COUNT };
    void *buf[B_COUNT] = {nullptr};
    size_t cap[B_COUNT] = {0};
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // timed calls: around a linearisation + assembly, around a solve + retraction
    double linearize_ms = 0.0, solve_ms = 0.0;                 // of the last timed call
};

void pgo_workspace_free(PgoWorkspace *ws);

struct PgoInputs {
    const double *poses; int n_poses;
    const int *f_i; const int *f_j; const double *f_z; const double *f_cov; int n_factors;
    const int *p_idx; const double *p_z; const double *p_cov; int n_priors;
};

// nullptr, or what is wrong with the arguments (checked on the host before anything runs)
const char *pgo_inputs_bad(const PgoInputs &in);
const char *pgo_params_bad(const scl_pgo_params &p);
void pgo_default_params(scl_pgo_params *p);

// Arguments checked by the caller; each waits for the stream before it returns.
int pgo_linearize(PgoWorkspace *ws, hipStream_t stream, const PgoInputs &in, double *cost, double *gradient, double *diag, double *chi2,
                  bool timing, std::string *err);
int pgo_hessian_apply(PgoWorkspace *ws, hipStream_t stream, const PgoInputs &in, double lambda, const double *x, double *y, bool timing,
                      std::string *err);
int pgo_optimize(PgoWorkspace *ws, hipStream_t stream, const PgoInputs &in, const scl_pgo_params &params, double *poses_out,
                 scl_pgo_result *result, double *chi2, bool timing, std::string *err);

}  // namespace scl
