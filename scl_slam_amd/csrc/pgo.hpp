// pgo.hpp -- the pose-graph solve on the GPU (host-side interface used by engine.hip; contract: include/scl_engine.h "POSE-GRAPH SOLVE").
#pragma once

#include <hip/hip_runtime.h>

#include <functional>
#include <string>
#include <vector>

#include "scl_engine.h"

namespace scl {

constexpr int kPgoLongRow = 64;                // a pose with this many incident factors or more is summed by a wave, not by one thread

// Grow-only.  Nothing a call reads was left by an earlier one: the inputs are copied in, and every kernel's inputs are written by the
// kernels queued in front of it in the same call.
struct PgoWorkspace {
    enum { B_POSES_IN = 0, B_Z_IN, B_COV_IN, B_FI, B_FJ, B_ROWPTR, B_ENTRIES, B_X0, B_X1, B_FPREP, B_FAC0, B_FAC1, B_G0, B_G1, B_D0, B_D1,
           B_LBLK, B_VX, B_VR, B_VZ, B_VQ, B_VP0, B_VP1, B_PART_COST, B_PART_GMAX, B_PART_RZ0, B_PART_RZ1, B_PART_PQ, B_PART_STEP, B_REC,
           B_XIN, B_POSES_OUT,
           // the condensed direct step (pgo_condensed.hip): the plan's arrays, the paths' nodes, the dense system
           B_C_NODE_POSE, B_C_NODE_COUPLING, B_C_ELIM, B_C_ABSORB, B_C_BLOCK_PTR, B_C_BLOCK_RC, B_C_SRC, B_C_RHS_PTR, B_C_RHS_SRC, B_C_JPOSE,
           B_C_ND, B_C_NB, B_C_NU, B_C_NP, B_C_NCL, B_C_NCR, B_C_NX, B_C_S, B_C_LDIAG, B_C_DIAG0, B_C_RHS,
           // the many-column solve on the kept factor (pgo_marginals.hip): a group's columns, its node arrays, its tiles of the dense
           // right-hand sides; the marginals' query arrays, kept rows and outputs
           B_M_X, B_M_NB, B_M_NL, B_M_NR, B_M_TILES, B_M_SEL, B_M_QUERY, B_M_KEPT, B_M_BLOCKS, B_M_REL,
           B_COUNT };
    void *buf[B_COUNT] = {nullptr};
    size_t cap[B_COUNT] = {0};
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // timed calls: around a linearisation + assembly, around a solve + retraction
    double linearize_ms = 0.0, solve_ms = 0.0;                 // of the last timed call
    hipEvent_t ev_c[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // a timed condensed step: its four stages lie between them
    double condensed_ms[4] = {0.0, 0.0, 0.0, 0.0};             // of the last timed condensed call: elimination, assembly, factorisation,
                                                               // solves + back-substitution, each summed over the call's steps
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

// ---- what pgo.hip shares with pgo_condensed.hip: the LM loop around a solve given to it, and the launches around that solve ----------

// the record the host reads once per LM iteration (B_REC).  fail: written by the condensed step alone, a pivot that failed in it
struct PgoRecord {
    double cost, gmax, step, rz0;
    int flag, cg, fail, pad;
};

// what one call keeps between its launches
struct PgoGraph {
    int n, M, nb;
    bool timing;
    float lin_ms, solve_ms;
};

// The damped system of side b solved into B_VX and the poses of side b retracted into side 1 - b (pgo_enqueue_retract), between the
// events ev[2] and ev[3] of a timed call.
using PgoSolveFn = std::function<int(PgoWorkspace *, hipStream_t, const PgoGraph &, int b, double lambda, std::string *err)>;

// The contract's Levenberg-Marquardt loop.  direct: the solve is exact, so cg_iterations stays 0, and a record with fail set makes
// the iteration a rejected step that counts in *failed_factorisations (may be NULL).
int pgo_lm(PgoWorkspace *ws, hipStream_t stream, const PgoInputs &in, const scl_pgo_params &params, const PgoSolveFn &solve, bool direct,
           double *poses_out, scl_pgo_result *result, double *chi2, int *failed_factorisations, bool timing, std::string *err);

int pgo_setup(PgoWorkspace *ws, hipStream_t stream, const PgoInputs &in, bool timing, PgoGraph *gr, std::string *err);
int pgo_enqueue_linearise(PgoWorkspace *ws, hipStream_t stream, const PgoGraph &gr, int b, bool with_step, std::string *err);
int pgo_enqueue_retract(PgoWorkspace *ws, hipStream_t stream, const PgoGraph &gr, int b, std::string *err);
int pgo_read_record(PgoWorkspace *ws, hipStream_t stream, PgoRecord *rec, std::string *err);
int pgo_add_timing(PgoWorkspace *ws, PgoGraph *gr, bool lin, bool solve, std::string *err);
int pgo_ensure(PgoWorkspace *ws, int k, size_t bytes, std::string *err);

// ---- pgo_condensed.hip ----------------------------------------------------------------------------------------------------------------

// the plan's shape, kept on the host between the launches of a call
struct PgoCondensed {
    int n_nodes = 0, n_junctions = 0, n_blocks = 0, n_levels = 0, n_rows = 0, ld = 0;
    std::vector<int> level_ptr, absorb_ptr;
    double ms[4] = {0.0, 0.0, 0.0, 0.0};
    bool pending = false;                                  // a timed step whose events have not been read
};

// nullptr, or why the condensed step refuses the graph (more than SCL_PGO_MAX_JUNCTIONS junctions); the indices are in range
const char *pgo_condensed_bad(const PgoInputs &in);
// one exact step (H + lambda diag H) delta = -g at in.poses; SCL_ERR_NUMERIC on a failed pivot, nothing written
int pgo_solve_condensed(PgoWorkspace *ws, hipStream_t stream, const PgoInputs &in, double lambda, double *delta, bool timing, std::string *err);
int pgo_optimize_condensed(PgoWorkspace *ws, hipStream_t stream, const PgoInputs &in, const scl_pgo_params &params, double *poses_out,
                           scl_pgo_result *result, double *chi2, int *failed_factorisations, bool timing, std::string *err);
// What pgo_marginals.hip takes from the step.  pgo_condensed_factor: setup, plan, one linearisation at in.poses, the elimination,
// the assembly and the factorisation of S at lambda -- the step's own launches up to the event ev_c[3]; L, P, Q of every node and the
// factor of S stay in the workspace.  pgo_condensed_finish: behind the caller's launches, the events ev_c[4] and ev[3], a wait for the
// stream, the call's timing.
int pgo_condensed_factor(PgoWorkspace *ws, hipStream_t stream, const PgoInputs &in, double lambda, bool timing, PgoGraph *gr, PgoCondensed *C,
                         std::string *err);
int pgo_condensed_finish(PgoWorkspace *ws, hipStream_t stream, PgoGraph *gr, PgoCondensed *C, std::string *err);

// ---- pgo_marginals.hip ----------------------------------------------------------------------------------------------------------------

// (H + lambda diag H) x_c = rhs_c for n_rhs columns of 6 n_poses on one factorisation; x may alias rhs
int pgo_solve_condensed_many(PgoWorkspace *ws, hipStream_t stream, const PgoInputs &in, double lambda, const double *rhs, int n_rhs, double *x,
                             bool timing, std::string *err);
// the blocks of H^-1 and the relative-pose covariances of n_queries pairs; the queries are checked by the caller (pgo_marginal_plan.hpp)
int pgo_marginals(PgoWorkspace *ws, hipStream_t stream, const PgoInputs &in, const int *q_i, const int *q_j, int n_queries, double *blocks,
                  double *rel, bool timing, std::string *err);

}  // namespace scl
