/*
 * scl_plugin_batch.h -- the batch forms of the float-row descriptor plugins (scl_m2dp.h, scl_fpfh.h, scl_grsd.h): one text for
 * the four calls every one of them declares.  SCL_PLUGIN_BATCH_API(scl_X) declares, for the plugin whose handle type and prefix
 * are scl_X and whose descriptor is DIM floats:
 *
 *   int scl_X_detect_intra_many(scl_X *h, const int *curs, int count, int *loop_ids, float *dists);     curs, loop_ids: LOCAL
 *   int scl_X_detect_inter_many(scl_X *h, const int *curs, int count, int *loop_ids, float *dists);     curs, loop_ids: GLOBAL
 *   int scl_X_save_from_wire_many(scl_X *h, const float *values, const int8_t *robots, const int *indexs, int count);
 *   int scl_X_make_save_and_detect(scl_X *h, const void *const *clouds, const int *n_points, int stride_bytes,
 *                                  const int8_t *robots, const int *indexs, int count,
 *                                  int *loop_ids, float *dists, float *out_values);
 *
 * Each answers, element by element and bit for bit, what the same single calls made in array order answer, and leaves the handle
 * in the same state (for inter_mode 0 of FPFH and GRSD that includes the call counter and the snapshot, committed only when the
 * call succeeds).  A call of any `count` runs in launch groups of SCL_PLUGIN_DETECT_GROUP queries, each group reading the candidate
 * rows once, and waits for the device once.  count == 0 is SCL_OK; dists may be NULL.
 *   * detect_*_many: every cur is validated first; one out of range anywhere returns SCL_ERR_OUT_OF_RANGE with nothing run, no
 *     output written and no state changed.
 *   * save_from_wire_many: `count` save_from_wire calls in one; values holds count * DIM floats; every robot id is validated
 *     first (a bad one stores nothing), the rows go to the device in one transfer.
 *   * make_save_and_detect: make_and_save_many followed, in the same call and on the same stream, by detect_intra of every new
 *     keyframe whose robots[i] is this_id (loop_ids LOCAL); entries of other robots answer loop -1, distance +inf.  If a cloud is
 *     invalid nothing is stored, nothing is detected and the outputs are untouched.  out_values (count * DIM floats) may be NULL.
 */
#ifndef SCL_PLUGIN_BATCH_H
#define SCL_PLUGIN_BATCH_H

#include <stdint.h>

#define SCL_PLUGIN_DETECT_GROUP 16   /* queries per launch of the batched 1-NN search */

#define SCL_PLUGIN_BATCH_API(X)                                                                                             \
    int X##_detect_intra_many(X *h, const int *curs, int count, int *loop_ids, float *dists);                               \
    int X##_detect_inter_many(X *h, const int *curs, int count, int *loop_ids, float *dists);                               \
    int X##_save_from_wire_many(X *h, const float *values, const int8_t *robots, const int *indexs, int count);             \
    int X##_make_save_and_detect(X *h, const void *const *clouds, const int *n_points, int stride_bytes,                    \
                                 const int8_t *robots, const int *indexs, int count, int *loop_ids, float *dists,           \
                                 float *out_values)

/*
 * THE CANDIDATE LISTS.  SCL_PLUGIN_TOPK_API(scl_X) declares the k nearest instead of the nearest, for a verifier (ICP, RANSAC) or
 * for rank statistics:
 *
 *   int scl_X_detect_intra_topk(scl_X *h, const int *curs, int count, int k, int *cand_ids, float *cand_dists, int *n_found);
 *   int scl_X_detect_inter_topk(scl_X *h, const int *curs, int count, int k, int *cand_ids, float *cand_dists, int *n_found);
 *
 * cand_ids and cand_dists hold count * k elements, row i for curs[i]; n_found holds count elements; cand_dists and n_found may be
 * NULL.  Query i searches exactly the set scl_X_detect_intra_many / scl_X_detect_inter_many searches for curs[i]: intra this
 * robot's keyframes [0, cur - num_exclude_recent), curs and ids LOCAL; inter by the plugin's rule (the snapshot for inter_mode 0 of
 * FPFH and GRSD, else the sorted lists), curs and ids GLOBAL.
 *   * Ranking: the squared L2 over the whole row in nanoflann's float order -- the sums of the 1-NN, bit for bit -- ascending by
 *     (float bits of the sum, position in the searched list): ties go to the lowest position.  A candidate whose sum is NaN is never
 *     listed (nanoflann's KNNResultSet admits dist < worst only); a sum of +inf is a candidate like any other.
 *   * n_found[i] = min(k, candidates with a non-NaN sum); entries j >= n_found[i] are id -1, distance +inf.
 *   * cand_dists: the plugin's reported distance of every listed candidate (sqrtf of the squared L2 over the floats the detections
 *     report, in nanoflann's order).  dist_thres is NOT applied: the list is for the verifier to judge.
 *   * When n_found[i] > 0, entry 0 is what the _many form finds before its threshold (id and distance bits); where the _many form
 *     reports a loop, the loop is cand_ids[i * k].
 *   * The handle is left exactly as the _many form with the same curs leaves it: for inter_mode 0 of FPFH and GRSD, below
 *     num_exclude_recent + 1 keyframes every n_found is 0 and the call counter stays; otherwise the counter and the snapshot walk
 *     per query and are committed only when the call succeeds.
 *   * k < 1 or k > SCL_PLUGIN_TOPK_MAX: SCL_ERR_INVALID_ARG.  A cur out of range anywhere: SCL_ERR_OUT_OF_RANGE with nothing run, no
 *     output written and no state changed.  count == 0 is SCL_OK.
 * A call of any `count` runs in launch groups of SCL_PLUGIN_DETECT_GROUP queries, each group reading the candidate rows once whatever
 * k is, and waits for the device once.
 */
#define SCL_PLUGIN_TOPK_MAX 32       /* the longest candidate list */

#define SCL_PLUGIN_TOPK_API(X)                                                                                              \
    int X##_detect_intra_topk(X *h, const int *curs, int count, int k, int *cand_ids, float *cand_dists, int *n_found);     \
    int X##_detect_inter_topk(X *h, const int *curs, int count, int k, int *cand_ids, float *cand_dists, int *n_found)

#endif /* SCL_PLUGIN_BATCH_H */
