// registration.hip -- host side of every registration entry point of the C ABI (include/scl_engine.h): single and batched ICP, the
// correspondence / SVD / RANSAC / verification wrappers, the voxel filter, submaps and the pose helpers, the on-device keyframe store
// and every *_from_store, *_guess and *_eval* call.  No kernel lives here (icp.hip, voxel.hip); the engine object, its locks and the
// sharded front's hooks are engine_internal.hpp's.  What the batched store forms share is written once: the windows of a list of
// candidates and a round's slice of them (candidate_windows.hpp), the received cloud (stage_received), a round's host targets
// (stage_host_targets), the live candidates of a round with their results' way back (LiveCandidates), the clears, and the scaffold
// of the guessed ICP and the scoring forms (store_form).
#include "scl_engine.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "candidate_windows.hpp"
#include "engine_internal.hpp"
#include "plugin_host.hpp"

using namespace scl;

namespace {

// the frame of the calls that wrap one function of icp.hip / voxel.hip: the primary shard, its lock and its device around
// call(e, &err) -> status, the message kept where it failed
template <class Call> int on_primary(scl_engine *e, Call call)
{
    if (e->front) e = front_primary(e);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    std::string err;
    const int rc = call(e, &err);
    if (rc) e->last_error = err;
    return rc;
}

}  // namespace

/* ---- geometric verification -------------------------------------------------- */

int scl_icp_default_params(scl_icp_params *p)
{
    if (!p) return SCL_ERR_INVALID_ARG;
    p->max_iterations = 50;               /* DM.h:1110 */
    p->max_correspondence_dist = 100.0;   /* DM.h:1109 */
    p->transformation_epsilon = 1e-6;     /* DM.h:1111 */
    p->euclidean_fitness_epsilon = 1e-6;  /* DM.h:1112 */
    p->estimator = 0;
    p->normal_radius = 1.0;
    return SCL_OK;
}

int scl_icp_align(scl_engine *e, const void *src, int n_src, const void *tgt, int n_tgt,
                  int stride_bytes, const scl_icp_params *p,
                  float T[16], float *fitness, int *converged, int *iterations)
{
    if (!e || !src || !tgt || !p || !T) return SCL_ERR_INVALID_ARG;
    return on_primary(e, [&](scl_engine *pe, std::string *err) {
        return icp_align(&pe->icp_ws, pe->stream, pe->num_cu, src, n_src, tgt, n_tgt, stride_bytes, *p, T, fitness, converged, iterations, err);
    });
}

namespace {
int icp_align_batch_host(scl_engine *e, const void *src, int n_src, const void *const *tgts, const int *n_tgts,
                         int n_targets, int stride_bytes, const float *guesses, const scl_icp_params *p,
                         float *T, float *fitness, int *converged, int *iterations);
}  // namespace

int scl_icp_align_batch(scl_engine *e, const void *src, int n_src, const void *const *tgts, const int *n_tgts,
                        int n_targets, int stride_bytes, const scl_icp_params *p,
                        float *T, float *fitness, int *converged, int *iterations)
{
    if (!e || !src || !p || !T || n_targets < 0 || (n_targets > 0 && (!tgts || !n_tgts))) return SCL_ERR_INVALID_ARG;
    if (e->front) return front_icp_align_batch(e, src, n_src, tgts, n_tgts, n_targets, stride_bytes, nullptr, p, T, nullptr, fitness, converged, iterations);
    return icp_align_batch_host(e, src, n_src, tgts, n_tgts, n_targets, stride_bytes, nullptr, p, T, fitness, converged, iterations);
}

namespace {

// scl_icp_align_batch (guesses == nullptr) and, on one engine, scl_icp_align_batch_guess (guesses = the call's n x 16, checked by the
// caller; T then receives every alignment's own transform, from the moved source)
int icp_align_batch_host(scl_engine *e, const void *src, int n_src, const void *const *tgts, const int *n_tgts,
                         int n_targets, int stride_bytes, const float *guesses, const scl_icp_params *p,
                         float *T, float *fitness, int *converged, int *iterations)
{
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    const int lanes = n_targets < scl_engine::kIcpLanes ? n_targets : scl_engine::kIcpLanes;
    for (int l = 0; l < lanes; ++l) {
        if (!e->icp_lane_stream[l]) SCL_HIP(e, hipStreamCreateWithFlags(&e->icp_lane_stream[l], hipStreamNonBlocking));
        if (!e->ev_lane[l]) SCL_HIP(e, hipEventCreateWithFlags(&e->ev_lane[l], hipEventDisableTiming));
    }
    if (n_src < 0 || stride_bytes < 12 || (stride_bytes & 3)) return fail(e, SCL_ERR_INVALID_ARG, "icp_align_batch: bad cloud layout");
    for (int c = 0; c < n_targets; ++c)
        if ((!tgts[c] && n_tgts[c] > 0) || n_tgts[c] < 0) return fail(e, SCL_ERR_INVALID_ARG, "icp_align_batch: bad target");
    // the source crosses PCIe once; every alignment's working cloud is made from it on the device
    int rc0 = eng_ensure_points(e, (size_t)n_src * stride_bytes + 16);
    if (rc0) return rc0;
    if (n_src) SCL_HIP(e, hipMemcpyAsync(e->d_points, src, (size_t)n_src * stride_bytes, hipMemcpyHostToDevice, e->stream));
    SCL_HIP(e, hipStreamSynchronize(e->stream));
    for (int first = 0; first < n_targets; first += scl_engine::kIcpBatch) {
        const int m = n_targets - first < scl_engine::kIcpBatch ? n_targets - first : scl_engine::kIcpBatch;
        // stage the targets and build their search grids (normals): independent per candidate, issued from a few host
        // threads onto the lane streams, so that one candidate's kernels run under another's PCIe copy (the batched chain of
        // scl_loop_icp_batch_from_store behind ALL the copies was measured slower here: 8.3 against 8.1 ms, 6.2 against 5.1 point to plane)
        std::atomic<int> next{0};
        std::atomic<int> first_rc{SCL_OK};
        std::string errs[scl_engine::kIcpLanes];
        auto worker = [&](int l) {
            (void)hipSetDevice(e->device);
            hipStream_t st = e->icp_lane_stream[l];
            for (;;) {
                const int c = next.fetch_add(1);
                if (c >= m) break;
                IcpWorkspace *ws = &e->icp_batch_ws[c];
                int rc = icp_stage_cloud_host(ws, st, true, tgts[first + c], n_tgts[first + c], stride_bytes, &errs[l]);
                if (!rc) rc = icp_batch_prepare(ws, st, e->d_points, n_src, n_tgts[first + c], stride_bytes, *p, &errs[l]);
                if (rc) { int ok = SCL_OK; first_rc.compare_exchange_strong(ok, rc); }
            }
            (void)hipEventRecord(e->ev_lane[l], st);
        };
        const int nl = m < lanes ? m : lanes;
        std::vector<std::thread> pool;
        for (int l = 1; l < nl; ++l) pool.emplace_back(worker, l);
        worker(0);
        for (auto &t : pool) t.join();
        int rc = first_rc.load();
        if (rc) { for (auto &msg : errs) if (!msg.empty()) { e->last_error = msg; break; } (void)hipDeviceSynchronize(); return rc; }
        for (int l = 0; l < nl; ++l) SCL_HIP(e, hipStreamWaitEvent(e->stream, e->ev_lane[l], 0));
        IcpWorkspace *wss[scl_engine::kIcpBatch];
        for (int c = 0; c < m; ++c) wss[c] = &e->icp_batch_ws[c];
        std::string err;
        float g12[12 * scl_engine::kIcpBatch];                          // rows 0 .. 2 of the round's guesses
        if (guesses) for (int c = 0; c < m; ++c) std::memcpy(g12 + 12 * (size_t)c, guesses + 16 * (size_t)(first + c), 12 * sizeof(float));
        rc = icp_batch_run(wss, m, &e->icp_batch_ctl, e->stream, e->d_points, n_src, stride_bytes, *p, guesses ? g12 : nullptr, T + 16 * (size_t)first,
                           fitness ? fitness + first : nullptr, converged ? converged + first : nullptr,
                           iterations ? iterations + first : nullptr, &err);
        if (rc) { e->last_error = err; return rc; }
    }
    return SCL_OK;
}

}  // namespace

int scl_nn_correspondences(scl_engine *e, const void *src, int n_src, const void *tgt, int n_tgt,
                           int stride_bytes, int *nn_index, float *nn_dist2)
{
    if (!e || !src || !tgt || !nn_index) return SCL_ERR_INVALID_ARG;
    return on_primary(e, [&](scl_engine *pe, std::string *err) {
        return icp_nn_correspondences(&pe->icp_ws, pe->stream, pe->num_cu, src, n_src, tgt, n_tgt, stride_bytes, nullptr, nn_index, nn_dist2, err);
    });
}

void scl_debug_icp_tile_stats(unsigned long long out[16], int reset) { icp_tile_stats(out, reset != 0); }

int scl_nn_correspondences_moved(scl_engine *e, const void *src, int n_src, const void *tgt, int n_tgt,
                                 int stride_bytes, const float T[16], int *nn_index, float *nn_dist2)
{
    if (!e || !src || !tgt || !nn_index || !T) return SCL_ERR_INVALID_ARG;
    return on_primary(e, [&](scl_engine *pe, std::string *err) {
        return icp_nn_correspondences(&pe->icp_ws, pe->stream, pe->num_cu, src, n_src, tgt, n_tgt, stride_bytes, T, nn_index, nn_dist2, err);
    });
}

int scl_rigid_svd(scl_engine *e, const void *src, int n_src, const void *tgt, int n_tgt,
                  int stride_bytes, const int *src_index, const int *tgt_index, int n_corr, float T[16])
{
    if (!e || !src || !tgt || !src_index || !tgt_index || !T) return SCL_ERR_INVALID_ARG;
    return on_primary(e, [&](scl_engine *pe, std::string *err) {
        return icp_rigid_svd(&pe->icp_ws, pe->stream, pe->num_cu, src, n_src, tgt, n_tgt, stride_bytes, src_index, tgt_index, n_corr, T, err);
    });
}

int scl_ransac_correspondences(scl_engine *e, const void *src, int n_src, const void *tgt, int n_tgt,
                               int stride_bytes, const int *src_index, const int *tgt_index, int n_corr,
                               int max_iterations, double inlier_threshold, uint64_t seed,
                               int *inlier_mask, int *n_inliers, int *best_hypothesis, float T_model[16])
{
    if (!e || !src || !tgt || !src_index || !tgt_index) return SCL_ERR_INVALID_ARG;
    return on_primary(e, [&](scl_engine *pe, std::string *err) {
        return icp_ransac(&pe->icp_ws, pe->stream, src, n_src, tgt, n_tgt, stride_bytes, src_index, tgt_index, n_corr,
                          max_iterations, inlier_threshold, (unsigned long long)seed, inlier_mask, n_inliers, best_hypothesis, T_model, err);
    });
}

int scl_geometric_verification(scl_engine *e, const void *src, int n_src, const void *tgt, int n_tgt,
                               int stride_bytes, int ransac_iterations, double inlier_threshold,
                               double inlier_ratio, uint64_t seed, float T[16], int *success,
                               int *n_correspondences, int *n_inliers)
{
    if (!e || !src || !tgt || !T) return SCL_ERR_INVALID_ARG;
    return on_primary(e, [&](scl_engine *pe, std::string *err) {
        return icp_geometric_verification(&pe->icp_ws, pe->stream, pe->num_cu, src, n_src, tgt, n_tgt, stride_bytes, ransac_iterations, inlier_threshold,
                                          inlier_ratio, (unsigned long long)seed, T, success, n_correspondences, n_inliers, err);
    });
}

int scl_voxel_grid(scl_engine *e, const void *points, int n_points, int stride_bytes, float leaf,
                   void *out, int out_capacity, int *n_out)
{
    if (!e || (!points && n_points > 0) || !out || !n_out) return SCL_ERR_INVALID_ARG;
    return on_primary(e, [&](scl_engine *pe, std::string *err) {
        return voxel_grid(&pe->vox_ws, pe->stream, points, n_points, stride_bytes, leaf, out, out_capacity, n_out, err);
    });
}

int scl_pose_to_matrix(float x, float y, float z, float roll, float pitch, float yaw, float T[16])
{
    if (!T) return SCL_ERR_INVALID_ARG;
    const float A = std::cos(yaw), B = std::sin(yaw), C = std::cos(pitch), D = std::sin(pitch), E = std::cos(roll), F = std::sin(roll);
    const float DE = D * E, DF = D * F;
    T[0] = A * C; T[1] = A * DF - B * E; T[2] = B * F + A * DE; T[3] = x;
    T[4] = B * C; T[5] = A * E + B * DF; T[6] = B * DE - A * F; T[7] = y;
    T[8] = -D;    T[9] = C * F;          T[10] = C * E;         T[11] = z;
    T[12] = 0.f;  T[13] = 0.f;           T[14] = 0.f;           T[15] = 1.f;
    return SCL_OK;
}

int scl_loop_guess_from_shift(int shift, int num_sector, const float pose_cur[6], const float pose_pre[6], float G[16])
{
    if (!pose_cur || !pose_pre || !G || num_sector < 1) return SCL_ERR_INVALID_ARG;
    for (int k = 0; k < 6; ++k) if (!std::isfinite(pose_cur[k]) || !std::isfinite(pose_pre[k])) return SCL_ERR_INVALID_ARG;
    auto pose_matrix = [](const float p[6], double R[9], double t[3]) {      /* scl_pose_to_matrix's entries, in double */
        const double A = std::cos((double)p[5]), B = std::sin((double)p[5]), C = std::cos((double)p[4]), D = std::sin((double)p[4]);
        const double E = std::cos((double)p[3]), F = std::sin((double)p[3]);
        R[0] = A * C; R[1] = A * D * F - B * E; R[2] = B * F + A * D * E;
        R[3] = B * C; R[4] = A * E + B * D * F; R[5] = B * D * E - A * F;
        R[6] = -D;    R[7] = C * F;             R[8] = C * E;
        t[0] = (double)p[0]; t[1] = (double)p[1]; t[2] = (double)p[2];
    };
    double Rc[9], tc[3], Rp[9], tp[3];
    pose_matrix(pose_cur, Rc, tc);
    pose_matrix(pose_pre, Rp, tp);
    /* the candidate's columns shifted right by `shift` look like the query (D.h:1376-1378, 1559): the query turns by -shift sectors */
    const int sh = ((shift % num_sector) + num_sector) % num_sector;
    const double yaw = -(double)sh * 6.283185307179586476925286766559 / (double)num_sector;
    const double cz = std::cos(yaw), sz = std::sin(yaw);
    const double Rz[9] = {cz, -sz, 0.0, sz, cz, 0.0, 0.0, 0.0, 1.0};
    double A[9], R[9], t[3];                                                 /* A = Rp * Rz, R = A * Rc^T, t = tp - R * tc */
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) A[3 * r + c] = (Rp[3 * r] * Rz[c] + Rp[3 * r + 1] * Rz[3 + c]) + Rp[3 * r + 2] * Rz[6 + c];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[3 * r + c] = (A[3 * r] * Rc[3 * c] + A[3 * r + 1] * Rc[3 * c + 1]) + A[3 * r + 2] * Rc[3 * c + 2];
    for (int r = 0; r < 3; ++r) t[r] = tp[r] - ((R[3 * r] * tc[0] + R[3 * r + 1] * tc[1]) + R[3 * r + 2] * tc[2]);
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) G[4 * r + c] = (float)R[3 * r + c]; G[4 * r + 3] = (float)t[r]; }
    G[12] = 0.f; G[13] = 0.f; G[14] = 0.f; G[15] = 1.f;
    return SCL_OK;
}

int scl_assemble_submap(scl_engine *e, const void *const *clouds, const int *counts, const float *transforms,
                        int n_clouds, int stride_bytes, float leaf, void *out, int out_capacity, int *n_out)
{
    if (!e || (n_clouds > 0 && (!clouds || !counts || !transforms)) || !out || !n_out) return SCL_ERR_INVALID_ARG;
    return on_primary(e, [&](scl_engine *pe, std::string *err) {
        return assemble_submap(&pe->vox_ws, pe->stream, clouds, counts, transforms, n_clouds, stride_bytes, leaf, out, out_capacity, n_out, err);
    });
}

int scl_transform_cloud(scl_engine *e, const void *in, int n, int stride_bytes, const float T[16], void *out)
{
    if (!e || !in || !out || !T) return SCL_ERR_INVALID_ARG;
    return on_primary(e, [&](scl_engine *pe, std::string *err) { return icp_transform_cloud(&pe->icp_ws, pe->stream, in, n, stride_bytes, T, out, err); });
}

/* ---- on-device keyframe store ------------------------------------------------ */

namespace {

constexpr size_t kKfSlabBytes = (size_t)256 << 20;         // 256 MiB slabs: ~100 keyframes of 100 k points each

int kf_alloc(scl_engine *e, size_t bytes, unsigned char **out)
{
    bytes = (bytes + 255) & ~(size_t)255;
    if (e->kf_slabs.empty() || e->kf_slab_used + bytes > e->kf_slab_cap) {
        const size_t cap = bytes > kKfSlabBytes ? bytes : kKfSlabBytes;
        void *slab = nullptr;
        if (hipMalloc(&slab, cap) != hipSuccess) return fail(e, SCL_ERR_NOMEM, "keyframe store: hipMalloc failed");
        e->kf_slabs.push_back(slab);
        e->kf_slab_used = 0;
        e->kf_slab_cap = cap;
    }
    *out = static_cast<unsigned char *>(e->kf_slabs.back()) + e->kf_slab_used;
    e->kf_slab_used += bytes;
    return SCL_OK;
}

// keyframes key-search_num .. key+search_num that exist in the store (DM.h:1168-1176), as one more window of w; poses[i] belongs to
// keyframe key - search_num + i.  The one function that reads the store; a refused window leaves w as it was
int kf_window(scl_engine *e, int robot, int key, int search_num, const float *poses, CandidateWindows *w)
{
    if (robot < 0 || search_num < 0 || !poses) return fail(e, SCL_ERR_INVALID_ARG, "keyframe window: bad arguments");
    std::vector<const void *> clouds; std::vector<int> counts; std::vector<float> T;
    if ((size_t)robot < e->kf.size()) {
        const auto &arr = e->kf[robot];
        for (int i = -search_num; i <= search_num; ++i) {
            const long long k = (long long)key + i;
            if (k < 0 || k >= (long long)arr.size()) continue;         // DM.h:1171-1174
            const auto &c = arr[(size_t)k];
            if (c.n < 0) return fail(e, SCL_ERR_INVALID_ARG, "keyframe window: a keyframe inside the window was never stored");
            clouds.push_back(c.d);
            counts.push_back(c.n);
            const float *m = poses + 16 * (size_t)(i + search_num);
            T.insert(T.end(), m, m + 16);
        }
    }
    w->add(clouds.data(), counts.data(), T.data(), (int)clouds.size());
    return SCL_OK;
}

// the windows of candidates 0 .. n - 1 (loopFindNearKeyframes(pre, historyKeyframeSearchNum), DM.h:1107 / 1202), each with its own
// 2 * search_num + 1 poses: the one collection loop of the batched store forms
int kf_windows(scl_engine *e, int robot, int n, const int *keys, int search_num, const float *poses, CandidateWindows *w)
{
    const int win = 2 * search_num + 1;
    for (int c = 0; c < n; ++c)
        if (int rc = kf_window(e, robot, keys[c], search_num, poses + (size_t)c * win * 16, w)) return rc;
    return SCL_OK;
}

// the submaps of a round's windows, every step of the voxel filter one launch over all of them (voxel.hip, assemble_submaps_batch);
// they stay in the filter's workspace and are read there until the round is over
int round_submaps(scl_engine *e, const CandidateWindows::Round &r, int stride, float leaf, const void **d_sub, int *n_sub)
{
    std::string err;
    const int rc = assemble_submaps_batch(&e->vox_ws, e->stream, r.clouds.data(), r.counts.data(), r.poses.data(), r.first.data(), r.jobs, stride, leaf,
                                          d_sub, n_sub, &err);
    if (rc) e->last_error = err;
    return rc;
}

// The received cloud: downSizeFilterICP (DM.h:1199-1201) with src_leaf, once per call; what is left (*ns points) is placed as the
// source of ws -- icp_batch_ctl, the single verification: icp_ws -- and stays on the device (a guess or a transform moves the
// filtered cloud, per candidate)
int stage_received(scl_engine *e, IcpWorkspace *ws, const void *src, int n_src, int stride, float src_leaf, int *ns)
{
    std::string err;
    const void *d_res = nullptr;
    int rc = voxel_grid_to_device(&e->vox_ws, e->stream, src, n_src, stride, src_leaf, &d_res, ns, &err);
    if (!rc) rc = icp_stage_cloud(ws, e->stream, false, d_res, *ns, stride, &err);
    if (rc) e->last_error = err;
    return rc;
}

// a round's host targets (m of them, at most kIcpBatch), target c placed in icp_batch_ws[c] and found at d_tgts[c]; none is gated, and one
// without a point is not staged
int stage_host_targets(scl_engine *e, const void *const *tgts, const int *n_tgts, int m, int stride, const void **d_tgts, bool *gated)
{
    std::string err;
    for (int c = 0; c < m; ++c) {
        gated[c] = false; d_tgts[c] = nullptr;
        if (n_tgts[c] < 1) continue;
        const int rc = icp_stage_cloud_host(&e->icp_batch_ws[c], e->stream, true, tgts[c], n_tgts[c], stride, &err);
        if (rc) { e->last_error = err; return rc; }
        d_tgts[c] = icp_staged_cloud(&e->icp_batch_ws[c], true);
    }
    return SCL_OK;
}

// The candidates of one round (at most kIcpBatch) that go on to a batch function of icp.hip, as that function takes them: live
// candidate j is candidate c of the round (its workspace: icp_batch_ws[c]) and entry which[j] of the call's outputs.  Who is live is
// the call site's rule; the results come back through which[].
struct LiveCandidates {
    scl_engine *e;
    IcpWorkspace *wss[scl_engine::kIcpBatch]; int which[scl_engine::kIcpBatch];
    const void *tg[scl_engine::kIcpBatch]; int tn[scl_engine::kIcpBatch];
    float rows[12 * scl_engine::kIcpBatch];                             // rows 0 .. 2 of the live candidates' guesses or transforms
    int live = 0;
    explicit LiveCandidates(scl_engine *engine) : e(engine) {}
    void add(int c, int global_index, const void *d_tgt, int n_tgt, const float *T16 /* nullptr: none */)
    {
        if (T16) std::memcpy(rows + 12 * (size_t)live, T16, 12 * sizeof(float));
        wss[live] = &e->icp_batch_ws[c]; which[live] = global_index; tg[live] = d_tgt; tn[live] = n_tgt; ++live;
    }
    // a round's results, `per` values for each live candidate, into the call's array (nullptr: not asked for)
    template <class V> void scatter(const V *round_values, V *out, int per = 1) const
    {
        if (out) for (int j = 0; j < live; ++j) std::memcpy(out + (size_t)per * which[j], round_values + (size_t)per * j, (size_t)per * sizeof(V));
    }
};

// the ICP forms' outputs before anything is known: identity (T_icp too, where there is one) and zeros
void icp_clear(int n, float *T, float *T_icp, float *fitness, int *converged, int *iterations, int *n_tgts)
{
    for (int c = 0; c < n; ++c) {
        for (int i = 0; i < 16; ++i) T[16 * (size_t)c + i] = (i % 5 == 0) ? 1.0f : 0.0f;
        if (T_icp) std::memcpy(T_icp + 16 * (size_t)c, T + 16 * (size_t)c, 16 * sizeof(float));
        if (fitness) fitness[c] = 0.0f;
        if (converged) converged[c] = 0;
        if (iterations) iterations[c] = 0;
        if (n_tgts) n_tgts[c] = 0;
    }
}

// One round (at most kIcpBatch candidates, entries first .. first + m - 1 of the outputs) of a batched ICP from the store: the search
// grids (+ normals) of the candidates behind the size gate (DM.h:1108), their submaps read where the filter left them -- one launch per
// step over all of them (icp.hip, icp_batch_prepare_all), on the engine's stream -- then icp_batch_run, with the live candidates' guesses
// where the call has guesses (nullptr: the unguessed form, which launches no move).  T receives every alignment's own transform; a gated
// candidate keeps what the caller wrote
int icp_round(scl_engine *e, int first, int m, const void *d_src, int ns, const void *const *d_tgts, const int *n_tgts, const bool *gated, int stride,
              const float *guesses /* nullptr, or the call's n x 16 */, const scl_icp_params &p, float *T, float *fitness, int *converged, int *iterations)
{
    LiveCandidates lc(e);
    for (int c = 0; c < m; ++c)
        if (!gated[c]) lc.add(c, first + c, d_tgts[c], n_tgts[c], guesses ? guesses + 16 * (size_t)(first + c) : nullptr);
    if (lc.live == 0) return SCL_OK;
    std::string err;
    int rc = icp_batch_prepare_all(lc.wss, lc.live, &e->icp_batch_ctl, e->stream, ns, lc.tg, lc.tn, stride, p, &err);
    if (rc) { e->last_error = err; return rc; }
    float Tl[16 * scl_engine::kIcpBatch], fl[scl_engine::kIcpBatch]; int cl[scl_engine::kIcpBatch], il[scl_engine::kIcpBatch];
    rc = icp_batch_run(lc.wss, lc.live, &e->icp_batch_ctl, e->stream, d_src, ns, stride, p, guesses ? lc.rows : nullptr, Tl, fl, cl, il, &err);
    if (rc) { e->last_error = err; return rc; }
    lc.scatter(Tl, T, 16); lc.scatter(fl, fitness); lc.scatter(cl, converged); lc.scatter(il, iterations);
    return SCL_OK;
}

}  // namespace

int scl_keyframe_put(scl_engine *e, int robot, int index, const void *points, int n_points, int stride_bytes)
{
    if (!e || robot < 0 || index < 0 || n_points < 0 || (!points && n_points > 0)) return SCL_ERR_INVALID_ARG;
    if (e->front) e = front_primary(e);
    std::lock_guard<std::mutex> lk(e->mu);
    if (stride_bytes < 12 || (stride_bytes & 3)) return fail(e, SCL_ERR_INVALID_ARG, "keyframe_put: bad stride");
    if (e->kf_stride == 0) e->kf_stride = stride_bytes;
    if (stride_bytes != e->kf_stride) return fail(e, SCL_ERR_INVALID_ARG, "keyframe_put: stride differs from the store's");
    (void)hipSetDevice(e->device);
    if ((size_t)robot >= e->kf.size()) e->kf.resize((size_t)robot + 1);
    auto &arr = e->kf[robot];
    if ((size_t)index >= arr.size()) arr.resize((size_t)index + 1);
    auto &c = arr[(size_t)index];
    const size_t bytes = (size_t)n_points * stride_bytes;
    if (bytes > c.cap_bytes) {                                         // replacing with a larger cloud: old space is retired
        unsigned char *d = nullptr;
        int rc = kf_alloc(e, bytes, &d);
        if (rc) return rc;
        c.d = d; c.cap_bytes = (bytes + 255) & ~(size_t)255;
    }
    if (bytes) {
        SCL_HIP(e, hipMemcpyAsync(c.d, points, bytes, hipMemcpyHostToDevice, e->stream));
        SCL_HIP(e, hipStreamSynchronize(e->stream));                   // the caller's buffer is free on return
    }
    c.n = n_points;
    ++c.generation;
    return SCL_OK;
}

int scl_keyframe_count(const scl_engine *e, int robot)
{
    if (!e || robot < 0) return SCL_ERR_INVALID_ARG;
    if (e->front) e = front_primary(e);
    std::lock_guard<std::mutex> lk(e->mu);
    return (size_t)robot < e->kf.size() ? (int)e->kf[robot].size() : 0;
}

int scl_keyframe_get(scl_engine *e, int robot, int index, void *out, int out_capacity, int *n_points)
{
    if (!e || robot < 0 || index < 0 || !n_points) return SCL_ERR_INVALID_ARG;
    if (e->front) e = front_primary(e);
    std::lock_guard<std::mutex> lk(e->mu);
    if ((size_t)robot >= e->kf.size() || (size_t)index >= e->kf[robot].size() || e->kf[robot][index].n < 0)
        return fail(e, SCL_ERR_INVALID_ARG, "keyframe_get: no such keyframe");
    const auto &c = e->kf[robot][index];
    *n_points = c.n;
    if (!out) return SCL_OK;
    if (c.n > out_capacity) return fail(e, SCL_ERR_INVALID_ARG, "keyframe_get: output capacity too small");
    (void)hipSetDevice(e->device);
    if (c.n) {
        SCL_HIP(e, hipMemcpyAsync(out, c.d, (size_t)c.n * e->kf_stride, hipMemcpyDeviceToHost, e->stream));
        SCL_HIP(e, hipStreamSynchronize(e->stream));
    }
    return SCL_OK;
}

int scl_submap_from_store(scl_engine *e, int robot, int key, int search_num, const float *poses, float leaf,
                          void *out, int out_capacity, int *n_out)
{
    if (!e || !out || !n_out) return SCL_ERR_INVALID_ARG;
    if (e->front) e = front_primary(e);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    CandidateWindows w;
    int rc = kf_window(e, robot, key, search_num, poses, &w);
    if (rc) return rc;
    std::string err;
    rc = assemble_submap_ex(&e->vox_ws, e->stream, w.clouds.data(), w.counts.data(), w.poses.data(), w.entries(),
                            e->kf_stride ? e->kf_stride : 16, leaf, true, out, out_capacity, nullptr, n_out, &err);
    if (rc) e->last_error = err;
    return rc;
}

int scl_loop_icp_from_store(scl_engine *e, int robot, int key_cur, const float *pose_cur,
                            int key_pre, int search_num, const float *poses_pre, float leaf,
                            const scl_icp_params *p, int min_src_points, int min_tgt_points,
                            float T[16], float *fitness, int *converged, int *iterations, int *n_src, int *n_tgt)
{
    if (!e || !pose_cur || !poses_pre || !p || !T) return SCL_ERR_INVALID_ARG;
    if (e->front) e = front_primary(e);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    const int stride = e->kf_stride ? e->kf_stride : 16;
    CandidateWindows cur, pre;
    std::string err;
    int ns = 0, nt = 0;
    const void *d_res = nullptr;
    // source: loopFindNearKeyframes(cur, 0), DM.h:1105
    int rc = kf_window(e, robot, key_cur, 0, pose_cur, &cur);
    if (rc) return rc;
    rc = assemble_submap_ex(&e->vox_ws, e->stream, cur.clouds.data(), cur.counts.data(), cur.poses.data(), cur.entries(), stride, leaf,
                            true, nullptr, 0, &d_res, &ns, &err);
    if (!rc) rc = icp_stage_cloud(&e->icp_ws, e->stream, false, d_res, ns, stride, &err);
    if (rc) { e->last_error = err; return rc; }
    // target: loopFindNearKeyframes(pre, historyKeyframeSearchNum), DM.h:1107
    rc = kf_window(e, robot, key_pre, search_num, poses_pre, &pre);
    if (rc) return rc;
    rc = assemble_submap_ex(&e->vox_ws, e->stream, pre.clouds.data(), pre.counts.data(), pre.poses.data(), pre.entries(), stride, leaf,
                            true, nullptr, 0, &d_res, &nt, &err);
    if (!rc) rc = icp_stage_cloud(&e->icp_ws, e->stream, true, d_res, nt, stride, &err);
    if (rc) { e->last_error = err; return rc; }
    if (n_src) *n_src = ns;
    if (n_tgt) *n_tgt = nt;
    if (converged) *converged = 0;
    if (iterations) *iterations = 0;
    if (fitness) *fitness = 0.0f;
    for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0f : 0.0f;
    if (ns < min_src_points || nt < min_tgt_points) return SCL_OK;    // DM.h:1108-1111: too small, no alignment attempted
    rc = icp_align_staged(&e->icp_ws, e->stream, ns, nt, stride, *p, T, fitness, converged, iterations, &err);
    if (rc) e->last_error = err;
    return rc;
}

int scl_loop_icp_batch_from_store(scl_engine *e, int robot, int key_cur, const float *pose_cur,
                                  int n_candidates, const int *keys_pre, int search_num, const float *poses_pre, float leaf,
                                  const scl_icp_params *p, int min_src_points, int min_tgt_points,
                                  float *T, float *fitness, int *converged, int *iterations, int *n_src, int *n_tgts)
{
    if (!e || !pose_cur || !p || !T || n_candidates < 0 || (n_candidates > 0 && (!keys_pre || !poses_pre))) return SCL_ERR_INVALID_ARG;
    if (e->front) e = front_primary(e);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    const int stride = e->kf_stride ? e->kf_stride : 16;
    const int win = 2 * search_num + 1;
    icp_clear(n_candidates, T, nullptr, fitness, converged, iterations, n_tgts);
    if (n_src) *n_src = 0;
    int rc = SCL_OK;
    CandidateWindows lead;
    if ((rc = kf_window(e, robot, key_cur, 0, pose_cur, &lead))) return rc;
    for (int first = 0; first < n_candidates || first == 0; first += scl_engine::kIcpBatch) {
        const int m = n_candidates - first < scl_engine::kIcpBatch ? n_candidates - first : scl_engine::kIcpBatch;
        // The submaps of a round -- the scan's own (loopFindNearKeyframes(cur, 0), DM.h:1105) in front, then the candidates'
        // (loopFindNearKeyframes(pre, historyKeyframeSearchNum), DM.h:1107) -- are assembled and filtered TOGETHER: every step of the
        // voxel filter is one launch over all of them (voxel.hip, assemble_submaps_batch), where each used to be a chain of ~20 short
        // launches on its lane.  (The scan's submap is redone per round of kIcpBatch candidates: rounds beyond the first are rare.)
        // This form reads a round's windows when the round begins, not all of them first as the guessed form does: a keyframe that was
        // never stored fails the call in its own round, behind the answers of the rounds before (docs/HISTORY.md)
        CandidateWindows cand;
        if ((rc = kf_windows(e, robot, m, keys_pre + first, search_num, poses_pre + (size_t)first * win * 16, &cand))) return rc;
        const void *d_sub[scl_engine::kIcpBatch + 1]; int n_sub[scl_engine::kIcpBatch + 1];
        if ((rc = round_submaps(e, cand.round(0, m, &lead), stride, leaf, d_sub, n_sub))) return rc;
        const int ns = n_sub[0];
        if (n_src) *n_src = ns;
        if (m <= 0) break;
        bool gated[scl_engine::kIcpBatch];
        for (int c = 0; c < m; ++c) {
            if (n_tgts) n_tgts[first + c] = n_sub[c + 1];
            gated[c] = ns < min_src_points || n_sub[c + 1] < min_tgt_points;   // DM.h:1108
        }
        if ((rc = icp_round(e, first, m, d_sub[0], ns, d_sub + 1, n_sub + 1, gated, stride, nullptr, *p, T, fitness, converged, iterations))) return rc;
    }
    return SCL_OK;
}

/* test hook: the submaps of voxel.hip's batched filter themselves -- scl_loop_icp_batch_from_store shows only their sizes and the ICP
 * result behind them.  Job j = the window of keys[j] with search_nums[j] (the production call: 0 for job 0), all jobs in ONE
 * assemble_submaps_batch call on the engine's own workspace and stream, the results copied back to back into `out` */
int scl_selftest_submaps_batch(scl_engine *e, int robot, int n_jobs, const int *keys, const int *search_nums, const float *poses,
                               float leaf, void *out, int out_capacity, int *n_out)
{
    if (!e || n_jobs < 0 || out_capacity < 0 || (out_capacity > 0 && !out) || (n_jobs > 0 && (!keys || !search_nums || !poses || !n_out))) return SCL_ERR_INVALID_ARG;
    if (e->front) e = front_primary(e);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    const int stride = e->kf_stride ? e->kf_stride : 16;
    CandidateWindows w;
    int rc = SCL_OK;
    size_t pose_off = 0;
    for (int j = 0; j < n_jobs; ++j) {
        if ((rc = kf_window(e, robot, keys[j], search_nums[j], poses + 16 * pose_off, &w))) return rc;
        pose_off += 2 * (size_t)search_nums[j] + 1;
    }
    std::vector<const void *> d_sub((size_t)n_jobs + 1); std::vector<int> n_sub((size_t)n_jobs + 1);
    if ((rc = round_submaps(e, w.round(0, n_jobs), stride, leaf, d_sub.data(), n_sub.data()))) return rc;
    size_t total = 0;
    for (int j = 0; j < n_jobs; ++j) total += (size_t)n_sub[(size_t)j];
    if (total > (size_t)out_capacity) return fail(e, SCL_ERR_INVALID_ARG, "selftest_submaps_batch: output capacity too small");
    size_t off = 0;
    for (int j = 0; j < n_jobs; ++j) {
        n_out[j] = n_sub[(size_t)j];
        if (n_sub[(size_t)j]) SCL_HIP(e, hipMemcpyAsync(static_cast<unsigned char *>(out) + off * stride, d_sub[(size_t)j], (size_t)n_sub[(size_t)j] * stride, hipMemcpyDeviceToHost, e->stream));
        off += (size_t)n_sub[(size_t)j];
    }
    SCL_HIP(e, hipStreamSynchronize(e->stream));
    return SCL_OK;
}

int scl_geometric_verification_from_store(scl_engine *e, const void *src, int n_src, int stride_bytes, float src_leaf,
                                          int robot, int key_pre, int search_num, const float *poses_pre, float leaf,
                                          int min_src_points, int min_tgt_points,
                                          int ransac_iterations, double inlier_threshold, double inlier_ratio, uint64_t seed,
                                          float T[16], int *success, int *n_src_filtered, int *n_tgt,
                                          int *n_correspondences, int *n_inliers)
{
    if (!e || (!src && n_src > 0) || !poses_pre || !T) return SCL_ERR_INVALID_ARG;
    if (e->front) e = front_primary(e);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    const int stride = e->kf_stride ? e->kf_stride : stride_bytes;
    if (stride != stride_bytes) return fail(e, SCL_ERR_INVALID_ARG, "geometric_verification_from_store: stride differs from the store's");
    std::string err;
    int ns = 0, nt = 0, rc;
    const void *d_res = nullptr;
    if ((rc = stage_received(e, &e->icp_ws, src, n_src, stride, src_leaf, &ns))) return rc;
    // submap around the matched keyframe (DM.h:1202) from the keyframe store
    CandidateWindows w;
    rc = kf_window(e, robot, key_pre, search_num, poses_pre, &w);
    if (rc) return rc;
    rc = assemble_submap_ex(&e->vox_ws, e->stream, w.clouds.data(), w.counts.data(), w.poses.data(), w.entries(), stride, leaf,
                            true, nullptr, 0, &d_res, &nt, &err);
    if (!rc) rc = icp_stage_cloud(&e->icp_ws, e->stream, true, d_res, nt, stride, &err);
    if (rc) { e->last_error = err; return rc; }
    if (n_src_filtered) *n_src_filtered = ns;
    if (n_tgt) *n_tgt = nt;
    for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0f : 0.0f;
    if (success) *success = 0;
    if (n_correspondences) *n_correspondences = 0;
    if (n_inliers) *n_inliers = 0;
    if (ns < min_src_points || nt < min_tgt_points) return SCL_OK;    // DM.h:1204: clouds too small
    rc = icp_geometric_verification_staged(&e->icp_ws, e->stream, ns, nt, stride, ransac_iterations, inlier_threshold,
                                           inlier_ratio, (unsigned long long)seed, T, success, n_correspondences, n_inliers, &err);
    if (rc) e->last_error = err;
    return rc;
}

/* ---- geometric verification of one received scan against k candidates ----------- */

namespace {

// one round (at most kIcpBatch candidates, entries first .. first + m - 1 of the outputs) of a verification batch: the source
// staged in icp_batch_ctl, target c on the device at d_tgts[c]; a candidate that is gated or has no point keeps what the caller
// wrote (identity, zeros), the others go through icp_geometric_verification_batch in one chain
int verification_round(scl_engine *e, int first, int m, int ns, const void *const *d_tgts, const int *n_tgts, const bool *gated, int stride,
                       const float *guesses /* nullptr, or the call's n x 16 */, int ransac_iterations, double inlier_threshold, double inlier_ratio, uint64_t seed,
                       float *T, int *success, int *n_correspondences, int *n_inliers)
{
    LiveCandidates lc(e);
    for (int c = 0; c < m; ++c) {
        if (gated[c] || ns < 1 || n_tgts[c] < 1) continue;                  // (no pair at all: scl_geometric_verification's early answer)
        lc.add(c, first + c, d_tgts[c], n_tgts[c], guesses ? guesses + 16 * (size_t)(first + c) : nullptr);
    }
    const int live = lc.live;
    if (live == 0) return SCL_OK;
    float Tl[16 * scl_engine::kIcpBatch]; int ok[scl_engine::kIcpBatch], nc[scl_engine::kIcpBatch], ni[scl_engine::kIcpBatch];
    std::string err;
    int rc = icp_geometric_verification_batch(lc.wss, live, &e->icp_batch_ctl, e->stream, ns, lc.tg, lc.tn, stride, guesses ? lc.rows : nullptr, ransac_iterations,
                                              inlier_threshold, inlier_ratio, (unsigned long long)seed, Tl, ok, nc, ni, &err);
    if (rc) { e->last_error = err; return rc; }
    lc.scatter(Tl, T, 16); lc.scatter(ok, success); lc.scatter(nc, n_correspondences); lc.scatter(ni, n_inliers);
    return SCL_OK;
}

void verification_clear(int n, float *T, int *success, int *n_tgts, int *n_correspondences, int *n_inliers)
{
    for (int c = 0; c < n; ++c) {
        for (int i = 0; i < 16; ++i) T[16 * (size_t)c + i] = (i % 5 == 0) ? 1.0f : 0.0f;
        if (success) success[c] = 0;
        if (n_tgts) n_tgts[c] = 0;
        if (n_correspondences) n_correspondences[c] = 0;
        if (n_inliers) n_inliers[c] = 0;
    }
}

// the guessed calls' last checks (after everything the unguessed calls refuse) -> nullptr or the message
const char *verification_guesses_bad(const float *guesses, int n)
{
    if (n > 0 && !guesses) return "guesses is NULL";
    for (size_t k = 0; k < 16 * (size_t)n; ++k)
        if ((k & 15) < 12 && !std::isfinite(guesses[k])) return "a guess has a non-finite entry in its first three rows";
    return nullptr;
}

// T[c] = T_fit[c] * G_c with G_c's last row taken as (0, 0, 0, 1): the whole motion received cloud -> candidate.  Every entry in double,
// ((a0 b0 + a1 b1) + a2 b2) + a3 b3, rounded once; no contraction (an fma would round differently).  T may be T_fit's own storage.
void verification_compose(int n, const float *T_fit, const float *guesses, const char *skip, float *T)
{
#pragma clang fp contract(off)
    for (int c = 0; c < n; ++c) {
        const float *A = T_fit + 16 * (size_t)c, *G = guesses + 16 * (size_t)c;
        float out[16];
        for (int r = 0; r < 4; ++r)
            for (int k = 0; k < 4; ++k) {
                const double a0 = A[4 * r], a1 = A[4 * r + 1], a2 = A[4 * r + 2], a3 = A[4 * r + 3];
                const double b0 = G[k], b1 = G[4 + k], b2 = G[8 + k], b3 = k == 3 ? 1.0 : 0.0;
                const double p0 = a0 * b0, p1 = a1 * b1, p2 = a2 * b2, p3 = a3 * b3;
                out[4 * r + k] = (float)(((p0 + p1) + p2) + p3);
            }
        std::memcpy(T + 16 * (size_t)c, skip && skip[c] ? A : out, sizeof out);
    }
}

int verification_batch_host(scl_engine *e, const void *src, int n_src,
                            const void *const *tgts, const int *n_tgts, int n_targets, int stride_bytes, const float *guesses, bool guessed,
                            int ransac_iterations, double inlier_threshold, double inlier_ratio, uint64_t seed,
                            float *T, float *T_fit, int *success, int *n_correspondences, int *n_inliers);
int verification_batch_store(scl_engine *e, const void *src, int n_src, int stride_bytes, float src_leaf,
                             int robot, int n_candidates, const int *keys_pre, int search_num, const float *poses_pre, float leaf,
                             const float *guesses, bool guessed, int min_src_points, int min_tgt_points,
                             int ransac_iterations, double inlier_threshold, double inlier_ratio, uint64_t seed,
                             float *T, float *T_fit, int *success, int *n_src_filtered, int *n_tgts,
                             int *n_correspondences, int *n_inliers);

}  // namespace

int scl_geometric_verification_batch(scl_engine *e, const void *src, int n_src,
                                     const void *const *tgts, const int *n_tgts, int n_targets, int stride_bytes,
                                     int ransac_iterations, double inlier_threshold, double inlier_ratio, uint64_t seed,
                                     float *T, int *success, int *n_correspondences, int *n_inliers)
{
    return verification_batch_host(e, src, n_src, tgts, n_tgts, n_targets, stride_bytes, nullptr, false, ransac_iterations, inlier_threshold,
                                   inlier_ratio, seed, T, nullptr, success, n_correspondences, n_inliers);
}

int scl_geometric_verification_batch_guess(scl_engine *e, const void *src, int n_src,
                                           const void *const *tgts, const int *n_tgts, int n_targets, int stride_bytes,
                                           const float *guesses,
                                           int ransac_iterations, double inlier_threshold, double inlier_ratio, uint64_t seed,
                                           float *T, float *T_fit, int *success, int *n_correspondences, int *n_inliers)
{
    return verification_batch_host(e, src, n_src, tgts, n_tgts, n_targets, stride_bytes, guesses, true, ransac_iterations, inlier_threshold,
                                   inlier_ratio, seed, T, T_fit, success, n_correspondences, n_inliers);
}

int scl_geometric_verification_batch_from_store(scl_engine *e, const void *src, int n_src, int stride_bytes, float src_leaf,
                                                int robot, int n_candidates, const int *keys_pre, int search_num, const float *poses_pre, float leaf,
                                                int min_src_points, int min_tgt_points,
                                                int ransac_iterations, double inlier_threshold, double inlier_ratio, uint64_t seed,
                                                float *T, int *success, int *n_src_filtered, int *n_tgts,
                                                int *n_correspondences, int *n_inliers)
{
    return verification_batch_store(e, src, n_src, stride_bytes, src_leaf, robot, n_candidates, keys_pre, search_num, poses_pre, leaf, nullptr, false,
                                    min_src_points, min_tgt_points, ransac_iterations, inlier_threshold, inlier_ratio, seed,
                                    T, nullptr, success, n_src_filtered, n_tgts, n_correspondences, n_inliers);
}

int scl_geometric_verification_batch_from_store_guess(scl_engine *e, const void *src, int n_src, int stride_bytes, float src_leaf,
                                                      int robot, int n_candidates, const int *keys_pre, int search_num, const float *poses_pre, float leaf,
                                                      const float *guesses,
                                                      int min_src_points, int min_tgt_points,
                                                      int ransac_iterations, double inlier_threshold, double inlier_ratio, uint64_t seed,
                                                      float *T, float *T_fit, int *success, int *n_src_filtered, int *n_tgts,
                                                      int *n_correspondences, int *n_inliers)
{
    return verification_batch_store(e, src, n_src, stride_bytes, src_leaf, robot, n_candidates, keys_pre, search_num, poses_pre, leaf, guesses, true,
                                    min_src_points, min_tgt_points, ransac_iterations, inlier_threshold, inlier_ratio, seed,
                                    T, T_fit, success, n_src_filtered, n_tgts, n_correspondences, n_inliers);
}

namespace {

// scl_geometric_verification_batch (guessed == false: guesses and T_fit are not looked at) and scl_geometric_verification_batch_guess
int verification_batch_host(scl_engine *e, const void *src, int n_src,
                            const void *const *tgts, const int *n_tgts, int n_targets, int stride_bytes, const float *guesses, bool guessed,
                            int ransac_iterations, double inlier_threshold, double inlier_ratio, uint64_t seed,
                            float *T, float *T_fit, int *success, int *n_correspondences, int *n_inliers)
{
    if (!e || n_targets < 0 || (!src && n_src > 0) || (n_targets > 0 && (!tgts || !n_tgts || !T))) return SCL_ERR_INVALID_ARG;
    if (e->front) e = front_primary(e);
    std::lock_guard<std::mutex> lk(e->mu);
    if (n_src < 0 || stride_bytes < 12 || (stride_bytes & 3)) return fail(e, SCL_ERR_INVALID_ARG, "geometric_verification_batch: bad cloud layout");
    for (int c = 0; c < n_targets; ++c)
        if (n_tgts[c] < 0 || (!tgts[c] && n_tgts[c] > 0)) return fail(e, SCL_ERR_INVALID_ARG, "geometric_verification_batch: bad target");
    if (n_src >= 3 && (ransac_iterations < 1 || ransac_iterations > (1 << 20))) return fail(e, SCL_ERR_INVALID_ARG, "ransac iterations out of range");
    if (guessed) if (const char *bad = verification_guesses_bad(guesses, n_targets)) return fail(e, SCL_ERR_INVALID_ARG, (std::string("geometric_verification_batch_guess: ") + bad).c_str());
    if (n_targets == 0) return SCL_OK;
    (void)hipSetDevice(e->device);
    verification_clear(n_targets, T, success, nullptr, n_correspondences, n_inliers);
    std::string err;
    int rc = SCL_OK;
    if (n_src >= 1) rc = icp_stage_cloud_host(&e->icp_batch_ctl, e->stream, false, src, n_src, stride_bytes, &err);   // once per call (none: no pair at all)
    if (rc) { e->last_error = err; return rc; }
    for (int first = 0; n_src >= 1 && first < n_targets; first += scl_engine::kIcpBatch) {
        const int m = n_targets - first < scl_engine::kIcpBatch ? n_targets - first : scl_engine::kIcpBatch;
        const void *d_tgts[scl_engine::kIcpBatch]; bool gated[scl_engine::kIcpBatch];
        if ((rc = stage_host_targets(e, tgts + first, n_tgts + first, m, stride_bytes, d_tgts, gated))) return rc;
        rc = verification_round(e, first, m, n_src, d_tgts, n_tgts + first, gated, stride_bytes, guessed ? guesses : nullptr, ransac_iterations,
                                inlier_threshold, inlier_ratio, seed, T, success, n_correspondences, n_inliers);
        if (rc) return rc;
    }
    if (guessed) {                                                         // the chain answered the fits: T = fit * guess, on the host
        if (T_fit) std::memcpy(T_fit, T, sizeof(float) * 16 * (size_t)n_targets);
        verification_compose(n_targets, T, guesses, nullptr, T);
    }
    return SCL_OK;
}

// scl_geometric_verification_batch_from_store (guessed == false) and scl_geometric_verification_batch_from_store_guess
int verification_batch_store(scl_engine *e, const void *src, int n_src, int stride_bytes, float src_leaf,
                             int robot, int n_candidates, const int *keys_pre, int search_num, const float *poses_pre, float leaf,
                             const float *guesses, bool guessed, int min_src_points, int min_tgt_points,
                             int ransac_iterations, double inlier_threshold, double inlier_ratio, uint64_t seed,
                             float *T, float *T_fit, int *success, int *n_src_filtered, int *n_tgts,
                             int *n_correspondences, int *n_inliers)
{
    if (!e || n_candidates < 0 || (!src && n_src > 0) || (n_candidates > 0 && (!keys_pre || !poses_pre || !T))) return SCL_ERR_INVALID_ARG;
    if (e->front) e = front_primary(e);
    std::lock_guard<std::mutex> lk(e->mu);
    const int stride = e->kf_stride ? e->kf_stride : stride_bytes;
    if (stride != stride_bytes) return fail(e, SCL_ERR_INVALID_ARG, "geometric_verification_batch_from_store: stride differs from the store's");
    if (n_src < 0 || stride < 12 || (stride & 3) || !(src_leaf > 0.f) || !(leaf > 0.f)) return fail(e, SCL_ERR_INVALID_ARG, "geometric_verification_batch_from_store: bad arguments");
    // (the received cloud's size before the filter: what is left of it is known only after something has run)
    if (n_src >= 3 && (ransac_iterations < 1 || ransac_iterations > (1 << 20))) return fail(e, SCL_ERR_INVALID_ARG, "ransac iterations out of range");
    // every candidate's window (DM.h:1202) before anything runs: an unstored keyframe inside one fails the call with no output written
    CandidateWindows cand;
    int rc;
    if ((rc = kf_windows(e, robot, n_candidates, keys_pre, search_num, poses_pre, &cand))) return rc;
    if (guessed) if (const char *bad = verification_guesses_bad(guesses, n_candidates)) return fail(e, SCL_ERR_INVALID_ARG, (std::string("geometric_verification_batch_from_store_guess: ") + bad).c_str());
    (void)hipSetDevice(e->device);
    int ns = 0;
    std::vector<char> gated_all((size_t)n_candidates + 1, 0);
    if ((rc = stage_received(e, &e->icp_batch_ctl, src, n_src, stride, src_leaf, &ns))) return rc;
    if (n_src_filtered) *n_src_filtered = ns;
    verification_clear(n_candidates, T, success, n_tgts, n_correspondences, n_inliers);
    for (int first = 0; first < n_candidates; first += scl_engine::kIcpBatch) {
        const int m = n_candidates - first < scl_engine::kIcpBatch ? n_candidates - first : scl_engine::kIcpBatch;
        const void *d_sub[scl_engine::kIcpBatch]; int n_sub[scl_engine::kIcpBatch]; bool gated[scl_engine::kIcpBatch];
        if ((rc = round_submaps(e, cand.round(first, m), stride, leaf, d_sub, n_sub))) return rc;
        for (int c = 0; c < m; ++c) {
            if (n_tgts) n_tgts[first + c] = n_sub[c];
            gated_all[(size_t)(first + c)] = gated[c] = ns < min_src_points || n_sub[c] < min_tgt_points;   // DM.h:1204: clouds too small
        }
        rc = verification_round(e, first, m, ns, d_sub, n_sub, gated, stride, guessed ? guesses : nullptr, ransac_iterations, inlier_threshold,
                                inlier_ratio, seed, T, success, n_correspondences, n_inliers);
        if (rc) return rc;
    }
    if (guessed) {                                                         // (a gated candidate keeps T = T_fit = identity)
        if (T_fit) std::memcpy(T_fit, T, sizeof(float) * 16 * (size_t)n_candidates);
        verification_compose(n_candidates, T, guesses, gated_all.data(), T);
    }
    return SCL_OK;
}

}  // namespace

/* ---- the batched ICP with one initial guess per candidate ------------------------ */

namespace {

// What the batched store forms with a guess or a transform per candidate are called with, whatever they compute: the source -- received
// == true: src, filtered once with src_leaf and placed in icp_batch_ctl as the guessed verification places it; received == false:
// submap(key_cur, 0), assembled in front of every round's candidates as the unguessed loop ICP does -- the candidates' windows and
// the size gate.  n_src_out receives the source's size behind the filter, n_tgts the submaps'
struct StoreCall {
    bool received; const void *src; int n_src, stride_bytes; float src_leaf;
    int robot, key_cur; const float *pose_cur;
    int n_candidates; const int *keys_pre; int search_num; const float *poses_pre; float leaf;
    int min_src_points, min_tgt_points;
    int *n_src_out, *n_tgts;
};

// The scaffold of those forms (the guessed ICP: icp_batch_store_guess, the scoring: eval_batch_store), in the order every one of them
// keeps: the arguments they share (`name` in front of every message), every window, the form's own last checks (last_checks() ->
// nullptr or the message), the source, then the rounds of kIcpBatch candidates: the round's submaps, the outputs cleared once behind
// the first round's (clear()), n_tgts and the size gate, and the form's round body(e, first, m, d_src, ns, d_tgts, n_tgts, gated, stride).
// (The verification from the store is not built on it: it checks its RANSAC count before the windows, names two calls in its messages
// and clears before the first round's submaps; it uses the pieces.)
template <class LastChecks, class Clear, class RoundBody>
int store_form(scl_engine *e, const StoreCall &a, const char *name, LastChecks last_checks, Clear clear, RoundBody body)
{
    if (!e || a.n_candidates < 0 || (a.n_candidates > 0 && (!a.keys_pre || !a.poses_pre))) return SCL_ERR_INVALID_ARG;
    if (a.received ? (!a.src && a.n_src > 0) : !a.pose_cur) return SCL_ERR_INVALID_ARG;
    if (e->front) e = front_primary(e);
    std::lock_guard<std::mutex> lk(e->mu);
    auto refuse = [&](const char *what) { return fail(e, SCL_ERR_INVALID_ARG, (std::string(name) + what).c_str()); };
    const int stride = e->kf_stride ? e->kf_stride : (a.received ? a.stride_bytes : 16);
    if (a.received) {
        if (stride != a.stride_bytes) return refuse("stride differs from the store's");
        if (a.n_src < 0 || stride < 12 || (stride & 3) || !(a.src_leaf > 0.f)) return refuse("bad arguments");
    }
    if (!(a.leaf > 0.f)) return refuse("bad arguments");
    // every window before anything runs: an unstored keyframe inside one fails the call with no output written
    CandidateWindows lead, cand;
    int rc;
    if (!a.received && (rc = kf_window(e, a.robot, a.key_cur, 0, a.pose_cur, &lead))) return rc;   // loopFindNearKeyframes(cur, 0), DM.h:1105
    if ((rc = kf_windows(e, a.robot, a.n_candidates, a.keys_pre, a.search_num, a.poses_pre, &cand))) return rc;
    if (const char *bad = last_checks()) return refuse(bad);
    (void)hipSetDevice(e->device);
    int ns = 0;
    const void *d_src = nullptr;
    if (a.received) {
        if ((rc = stage_received(e, &e->icp_batch_ctl, a.src, a.n_src, stride, a.src_leaf, &ns))) return rc;
        d_src = icp_staged_cloud(&e->icp_batch_ctl, false);
        if (a.n_src_out) *a.n_src_out = ns;
    }
    const int L = a.received ? 0 : 1;                                      // the loop forms' source is job 0 of every round, redone per round
    bool cleared = false;
    for (int first = 0; first < a.n_candidates || (first == 0 && L); first += scl_engine::kIcpBatch) {
        const int m = a.n_candidates - first < scl_engine::kIcpBatch ? a.n_candidates - first : scl_engine::kIcpBatch;
        const void *d_sub[scl_engine::kIcpBatch + 1]; int n_sub[scl_engine::kIcpBatch + 1]; bool gated[scl_engine::kIcpBatch];
        if ((rc = round_submaps(e, cand.round(first, m, L ? &lead : nullptr), stride, a.leaf, d_sub, n_sub))) return rc;
        if (L) { ns = n_sub[0]; d_src = d_sub[0]; if (a.n_src_out) *a.n_src_out = ns; }
        if (!cleared) { clear(); cleared = true; }
        if (m <= 0) break;
        for (int c = 0; c < m; ++c) {
            if (a.n_tgts) a.n_tgts[first + c] = n_sub[c + L];
            gated[c] = ns < a.min_src_points || n_sub[c + L] < a.min_tgt_points;   // DM.h:1108 / 1204: the unmoved sizes
        }
        if ((rc = body(e, first, m, d_src, ns, d_sub + L, n_sub + L, gated, stride))) return rc;
    }
    return SCL_OK;
}

// scl_loop_icp_batch_from_store_guess and scl_icp_align_batch_from_store_guess.  A round: icp_round with the live candidates' guesses
int icp_batch_store_guess(scl_engine *e, const StoreCall &a, const float *guesses, const scl_icp_params *p,
                          float *T, float *T_icp, float *fitness, int *converged, int *iterations)
{
    if (!p || !T) return SCL_ERR_INVALID_ARG;
    const int n = a.n_candidates > 0 ? a.n_candidates : 0;
    std::vector<float> own;                                                // the alignments' own transforms, where the caller does not ask for them
    float *Ti = T_icp;
    if (!Ti) { own.resize(16 * (size_t)n + 16); Ti = own.data(); }
    std::vector<char> gated_all((size_t)n + 1, 0);
    const int rc = store_form(e, a, a.received ? "icp_align_batch_from_store_guess: " : "loop_icp_batch_from_store_guess: ",
        [&]() -> const char * {
            if (a.n_candidates > 0) if (const char *bad = icp_params_bad(*p)) return bad;
            return verification_guesses_bad(guesses, a.n_candidates);
        },
        [&] { icp_clear(a.n_candidates, T, Ti, fitness, converged, iterations, a.n_tgts); },
        [&](scl_engine *pe, int first, int m, const void *d_src, int ns, const void *const *d_tgts, const int *n_tgts, const bool *gated, int stride) {
            for (int c = 0; c < m; ++c) gated_all[(size_t)(first + c)] = gated[c];
            return icp_round(pe, first, m, d_src, ns, d_tgts, n_tgts, gated, stride, guesses, *p, Ti, fitness, converged, iterations);
        });
    if (rc) return rc;
    if (a.n_candidates > 0) verification_compose(a.n_candidates, Ti, guesses, gated_all.data(), T);   // T = T_icp * G; a gated candidate keeps the identity
    return SCL_OK;
}

}  // namespace

int scl_icp_align_batch_guess(scl_engine *e, const void *src, int n_src, const void *const *tgts, const int *n_tgts,
                              int n_targets, int stride_bytes, const float *guesses, const scl_icp_params *p,
                              float *T, float *T_icp, float *fitness, int *converged, int *iterations)
{
    if (!e || !src || !p || !T || n_targets < 0 || (n_targets > 0 && (!tgts || !n_tgts))) return SCL_ERR_INVALID_ARG;
    {   // everything the unguessed call refuses, then the guesses: before anything runs (on a sharded engine: before any shard does)
        std::lock_guard<std::mutex> lk(e->mu);
        if (n_src < 0 || stride_bytes < 12 || (stride_bytes & 3)) return fail(e, SCL_ERR_INVALID_ARG, "icp_align_batch_guess: bad cloud layout");
        for (int c = 0; c < n_targets; ++c)
            if ((!tgts[c] && n_tgts[c] > 0) || n_tgts[c] < 0) return fail(e, SCL_ERR_INVALID_ARG, "icp_align_batch_guess: bad target");
        if (n_targets > 0) if (const char *bad = icp_params_bad(*p)) return fail(e, SCL_ERR_INVALID_ARG, (std::string("icp_align_batch_guess: ") + bad).c_str());
        if (const char *bad = verification_guesses_bad(guesses, n_targets)) return fail(e, SCL_ERR_INVALID_ARG, (std::string("icp_align_batch_guess: ") + bad).c_str());
    }
    if (n_targets == 0) return SCL_OK;
    std::vector<float> own;
    float *Ti = T_icp;
    if (!Ti) { own.resize(16 * (size_t)n_targets); Ti = own.data(); }
    const int rc = e->front ? front_icp_align_batch(e, src, n_src, tgts, n_tgts, n_targets, stride_bytes, guesses, p, T, Ti, fitness, converged, iterations)
                            : icp_align_batch_host(e, src, n_src, tgts, n_tgts, n_targets, stride_bytes, guesses, p, Ti, fitness, converged, iterations);
    if (rc) return rc;
    if (!e->front) verification_compose(n_targets, Ti, guesses, nullptr, T);   // (the shards composed their own entries)
    return SCL_OK;
}

int scl_loop_icp_batch_from_store_guess(scl_engine *e, int robot, int key_cur, const float *pose_cur,
                                        int n_candidates, const int *keys_pre, int search_num, const float *poses_pre, float leaf,
                                        const float *guesses, const scl_icp_params *p, int min_src_points, int min_tgt_points,
                                        float *T, float *T_icp, float *fitness, int *converged, int *iterations, int *n_src, int *n_tgts)
{
    const StoreCall a = {false, nullptr, 0, 0, 0.f, robot, key_cur, pose_cur, n_candidates, keys_pre, search_num, poses_pre, leaf,
                         min_src_points, min_tgt_points, n_src, n_tgts};
    return icp_batch_store_guess(e, a, guesses, p, T, T_icp, fitness, converged, iterations);
}

int scl_icp_align_batch_from_store_guess(scl_engine *e, const void *src, int n_src, int stride_bytes, float src_leaf,
                                         int robot, int n_candidates, const int *keys_pre, int search_num, const float *poses_pre, float leaf,
                                         const float *guesses, const scl_icp_params *p, int min_src_points, int min_tgt_points,
                                         float *T, float *T_icp, float *fitness, int *converged, int *iterations, int *n_src_filtered, int *n_tgts)
{
    const StoreCall a = {true, src, n_src, stride_bytes, src_leaf, robot, 0, nullptr, n_candidates, keys_pre, search_num, poses_pre, leaf,
                         min_src_points, min_tgt_points, n_src_filtered, n_tgts};
    return icp_batch_store_guess(e, a, guesses, p, T, T_icp, fitness, converged, iterations);
}

/* ---- batched registration scoring: overlap, RMSE and information matrix ----------- */

namespace {

// the plane forms' own arguments (nullptr: the point-to-point forms): the normals' radius, and n_planar and sums (29 per candidate)
// where the point forms have moments
struct EvalPlane { double normal_radius; int *n_planar; double *sums; };

// what the scoring calls refuse last, behind their own cloud and window checks -> nullptr or the message
const char *eval_args_bad(const float *transforms, int n, double max_dist, const int *n_valid, const int *n_inliers, const double *moments,
                          const EvalPlane *pl = nullptr)
{
    if (!std::isfinite(max_dist) || max_dist < 0.0) return "max_dist must be finite and >= 0";
    if (pl && !(pl->normal_radius > 0.0)) return "normal_radius must be > 0";                      // the ICP's parameter check (icp_params_bad)
    if (n > 0 && !n_valid && !n_inliers && !moments && !(pl && (pl->n_planar || pl->sums))) return "no output asked for";
    if (n > 0 && !transforms) return "transforms is NULL";
    for (size_t k = 0; k < 16 * (size_t)n; ++k)
        if ((k & 15) < 12 && !std::isfinite(transforms[k])) return "a transform has a non-finite entry in its first three rows";
    return nullptr;
}

void eval_clear(int n, int *n_valid, int *n_inliers, double *moments, int *n_tgts, const EvalPlane *pl = nullptr)
{
    for (int c = 0; c < n; ++c) {
        if (n_valid) n_valid[c] = 0;
        if (n_inliers) n_inliers[c] = 0;
        if (n_tgts) n_tgts[c] = 0;
        if (pl && pl->n_planar) pl->n_planar[c] = 0;
    }
    if (moments) for (size_t k = 0; k < 10 * (size_t)n; ++k) moments[k] = 0.0;
    if (pl && pl->sums) for (size_t k = 0; k < 29 * (size_t)n; ++k) pl->sums[k] = 0.0;
}

// one round (at most kIcpBatch candidates, entries first .. first + m - 1 of the outputs): the source on the device at d_src, target c
// at d_tgts[c]; a candidate that is gated or has no pair to find keeps the zeros the caller wrote
int eval_round(scl_engine *e, int first, int m, const void *d_src, int ns, const void *const *d_tgts, const int *n_tgts, const bool *gated,
               int stride, const float *transforms, double max_dist, int *n_valid, int *n_inliers, double *moments, const EvalPlane *pl = nullptr)
{
    LiveCandidates lc(e);
    for (int c = 0; c < m; ++c) {
        if (gated[c] || ns < 1 || n_tgts[c] < 1) continue;
        lc.add(c, first + c, d_tgts[c], n_tgts[c], transforms + 16 * (size_t)(first + c));
    }
    const int live = lc.live;
    if (live == 0) return SCL_OK;
    int nv[scl_engine::kIcpBatch], ni[scl_engine::kIcpBatch], np[scl_engine::kIcpBatch]; double mo[29 * scl_engine::kIcpBatch];
    std::string err;
    const float maxd2 = (float)(max_dist * max_dist);                    // ICP's rejection rule (icp.hip, icp_batch_run)
    int rc = pl ? icp_registration_eval_plane_batch(lc.wss, live, &e->icp_batch_ctl, e->stream, d_src, ns, lc.tg, lc.tn, stride, lc.rows, maxd2, pl->normal_radius,
                                                    nv, ni, np, mo, &err)
                : icp_registration_eval_batch(lc.wss, live, &e->icp_batch_ctl, e->stream, d_src, ns, lc.tg, lc.tn, stride, lc.rows, maxd2, nv, ni, mo, &err);
    if (rc) { e->last_error = err; return rc; }
    lc.scatter(nv, n_valid); lc.scatter(ni, n_inliers); lc.scatter(mo, moments, 10);
    if (pl) { lc.scatter(np, pl->n_planar); lc.scatter(mo, pl->sums, 29); }
    return SCL_OK;
}

// scl_loop_eval_batch_from_store, scl_registration_eval_batch_from_store and their plane forms (pl != nullptr): store_form with
// eval_round as the round
int eval_batch_store(scl_engine *e, const StoreCall &a, const float *transforms, double max_dist,
                     int *n_valid, int *n_inliers, double *moments, const EvalPlane *pl = nullptr)
{
    const char *const name = pl ? (a.received ? "registration_eval_plane_batch_from_store: " : "loop_eval_plane_batch_from_store: ")
                                : (a.received ? "registration_eval_batch_from_store: " : "loop_eval_batch_from_store: ");
    return store_form(e, a, name,
        [&] { return eval_args_bad(transforms, a.n_candidates, max_dist, n_valid, n_inliers, moments, pl); },
        [&] { eval_clear(a.n_candidates, n_valid, n_inliers, moments, a.n_tgts, pl); },
        [&](scl_engine *pe, int first, int m, const void *d_src, int ns, const void *const *d_tgts, const int *n_tgts, const bool *gated, int stride) {
            return eval_round(pe, first, m, d_src, ns, d_tgts, n_tgts, gated, stride, transforms, max_dist, n_valid, n_inliers, moments, pl);
        });
}

// scl_registration_eval_batch (pl == nullptr) and scl_registration_eval_plane_batch: host clouds
int eval_batch_host(scl_engine *e, const void *src, int n_src, const void *const *tgts, const int *n_tgts,
                    int n_targets, int stride_bytes, const float *transforms, double max_dist,
                    int *n_valid, int *n_inliers, double *moments, const EvalPlane *pl)
{
    const std::string name = pl ? "registration_eval_plane_batch: " : "registration_eval_batch: ";
    if (!e || n_targets < 0 || (!src && n_src > 0) || (n_targets > 0 && (!tgts || !n_tgts))) return SCL_ERR_INVALID_ARG;
    if (e->front) e = front_primary(e);
    std::lock_guard<std::mutex> lk(e->mu);
    if (n_src < 0 || stride_bytes < 12 || (stride_bytes & 3)) return fail(e, SCL_ERR_INVALID_ARG, (name + "bad cloud layout").c_str());
    for (int c = 0; c < n_targets; ++c)
        if (n_tgts[c] < 0 || (!tgts[c] && n_tgts[c] > 0)) return fail(e, SCL_ERR_INVALID_ARG, (name + "bad target").c_str());
    if (const char *bad = eval_args_bad(transforms, n_targets, max_dist, n_valid, n_inliers, moments, pl)) return fail(e, SCL_ERR_INVALID_ARG, (name + bad).c_str());
    if (n_targets == 0) return SCL_OK;
    (void)hipSetDevice(e->device);
    eval_clear(n_targets, n_valid, n_inliers, moments, nullptr, pl);
    std::string err;
    int rc = SCL_OK;
    if (n_src >= 1) rc = icp_stage_cloud_host(&e->icp_batch_ctl, e->stream, false, src, n_src, stride_bytes, &err);   // once per call (none: no pair at all)
    if (rc) { e->last_error = err; return rc; }
    for (int first = 0; n_src >= 1 && first < n_targets; first += scl_engine::kIcpBatch) {
        const int m = n_targets - first < scl_engine::kIcpBatch ? n_targets - first : scl_engine::kIcpBatch;
        const void *d_tgts[scl_engine::kIcpBatch]; bool gated[scl_engine::kIcpBatch];
        if ((rc = stage_host_targets(e, tgts + first, n_tgts + first, m, stride_bytes, d_tgts, gated))) return rc;
        rc = eval_round(e, first, m, icp_staged_cloud(&e->icp_batch_ctl, false), n_src, d_tgts, n_tgts + first, gated, stride_bytes, transforms, max_dist,
                        n_valid, n_inliers, moments, pl);
        if (rc) return rc;
    }
    return SCL_OK;
}

}  // namespace

int scl_registration_eval_batch(scl_engine *e, const void *src, int n_src, const void *const *tgts, const int *n_tgts,
                                int n_targets, int stride_bytes, const float *transforms, double max_dist,
                                int *n_valid, int *n_inliers, double *moments)
{
    return eval_batch_host(e, src, n_src, tgts, n_tgts, n_targets, stride_bytes, transforms, max_dist, n_valid, n_inliers, moments, nullptr);
}

int scl_registration_eval_batch_from_store(scl_engine *e, const void *src, int n_src, int stride_bytes, float src_leaf,
                                           int robot, int n_candidates, const int *keys_pre, int search_num, const float *poses_pre, float leaf,
                                           const float *transforms, int min_src_points, int min_tgt_points, double max_dist,
                                           int *n_valid, int *n_inliers, double *moments, int *n_src_filtered, int *n_tgts)
{
    const StoreCall a = {true, src, n_src, stride_bytes, src_leaf, robot, 0, nullptr, n_candidates, keys_pre, search_num, poses_pre, leaf,
                         min_src_points, min_tgt_points, n_src_filtered, n_tgts};
    return eval_batch_store(e, a, transforms, max_dist, n_valid, n_inliers, moments);
}

int scl_loop_eval_batch_from_store(scl_engine *e, int robot, int key_cur, const float *pose_cur,
                                   int n_candidates, const int *keys_pre, int search_num, const float *poses_pre, float leaf,
                                   const float *transforms, int min_src_points, int min_tgt_points, double max_dist,
                                   int *n_valid, int *n_inliers, double *moments, int *n_src, int *n_tgts)
{
    const StoreCall a = {false, nullptr, 0, 0, 0.f, robot, key_cur, pose_cur, n_candidates, keys_pre, search_num, poses_pre, leaf,
                         min_src_points, min_tgt_points, n_src, n_tgts};
    return eval_batch_store(e, a, transforms, max_dist, n_valid, n_inliers, moments);
}

int scl_registration_information(int n_inliers, const double moments[10], double info[36])
{
    if (!moments || !info || n_inliers < 0) return SCL_ERR_INVALID_ARG;
    const double m = (double)n_inliers;
    const double Sx = moments[0], Sy = moments[1], Sz = moments[2], Sxx = moments[3], Syy = moments[4], Szz = moments[5];
    const double Sxy = moments[6], Sxz = moments[7], Syz = moments[8];
    const double out[36] = {Syy + Szz, -Sxy, -Sxz, 0.0, -Sz, Sy,
                            -Sxy, Sxx + Szz, -Syz, Sz, 0.0, -Sx,
                            -Sxz, -Syz, Sxx + Syy, -Sy, Sx, 0.0,
                            0.0, Sz, -Sy, m, 0.0, 0.0,
                            -Sz, 0.0, Sx, 0.0, m, 0.0,
                            Sy, -Sx, 0.0, 0.0, 0.0, m};
    std::memcpy(info, out, sizeof out);
    return SCL_OK;
}

/* ---- point-to-plane registration scoring: normals, plane Hessian, residuals ------ */

int scl_target_normals(scl_engine *e, const void *tgt, int n_tgt, int stride_bytes, double radius, float *normals)
{
    if (!e || n_tgt < 0 || (n_tgt > 0 && (!tgt || !normals))) return SCL_ERR_INVALID_ARG;
    return on_primary(e, [&](scl_engine *pe, std::string *err) { return icp_target_normals(&pe->icp_ws, pe->stream, tgt, n_tgt, stride_bytes, radius, normals, err); });
}

int scl_registration_eval_plane_batch(scl_engine *e, const void *src, int n_src, const void *const *tgts, const int *n_tgts,
                                      int n_targets, int stride_bytes, const float *transforms, double max_dist, double normal_radius,
                                      int *n_valid, int *n_inliers, int *n_planar, double *sums)
{
    const EvalPlane pl = {normal_radius, n_planar, sums};
    return eval_batch_host(e, src, n_src, tgts, n_tgts, n_targets, stride_bytes, transforms, max_dist, n_valid, n_inliers, nullptr, &pl);
}

int scl_registration_eval_plane_batch_from_store(scl_engine *e, const void *src, int n_src, int stride_bytes, float src_leaf,
                                                 int robot, int n_candidates, const int *keys_pre, int search_num, const float *poses_pre, float leaf,
                                                 const float *transforms, int min_src_points, int min_tgt_points, double max_dist, double normal_radius,
                                                 int *n_valid, int *n_inliers, int *n_planar, double *sums, int *n_src_filtered, int *n_tgts)
{
    const EvalPlane pl = {normal_radius, n_planar, sums};
    const StoreCall a = {true, src, n_src, stride_bytes, src_leaf, robot, 0, nullptr, n_candidates, keys_pre, search_num, poses_pre, leaf,
                         min_src_points, min_tgt_points, n_src_filtered, n_tgts};
    return eval_batch_store(e, a, transforms, max_dist, n_valid, n_inliers, nullptr, &pl);
}

int scl_loop_eval_plane_batch_from_store(scl_engine *e, int robot, int key_cur, const float *pose_cur,
                                         int n_candidates, const int *keys_pre, int search_num, const float *poses_pre, float leaf,
                                         const float *transforms, int min_src_points, int min_tgt_points, double max_dist, double normal_radius,
                                         int *n_valid, int *n_inliers, int *n_planar, double *sums, int *n_src, int *n_tgts)
{
    const EvalPlane pl = {normal_radius, n_planar, sums};
    const StoreCall a = {false, nullptr, 0, 0, 0.f, robot, key_cur, pose_cur, n_candidates, keys_pre, search_num, poses_pre, leaf,
                         min_src_points, min_tgt_points, n_src, n_tgts};
    return eval_batch_store(e, a, transforms, max_dist, n_valid, n_inliers, nullptr, &pl);
}

int scl_registration_information_plane(const double sums[29], double info[36], double grad[6])
{
    if (!sums || !info) return SCL_ERR_INVALID_ARG;
    int t = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) { info[6 * a + b] = sums[t]; info[6 * b + a] = sums[t]; ++t; }
    if (grad) for (int a = 0; a < 6; ++a) grad[a] = sums[21 + a];
    return SCL_OK;
}

