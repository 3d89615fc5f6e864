/*
 * scl_m2dp.h -- C ABI of the M2DP descriptor (He, Wang, Zhang: "M2DP: a novel 3D point cloud descriptor and its application in
 * loop closure detection", IROS 2016): the third descriptor of the reference's run-time switch (class m2dp_descriptor,
 * include/descriptor.h:1803-2040; selected by descriptorType, distributedMapping.h:156-182, built at DM.h:412).
 *
 * On the GPU, per launch group of up to 16 scans: the PCA frame of the cloud (pca.project, D.h:1824-1825), the projected cloud
 * cloudPca and the maxRho quirk (D.h:1828-1840), the 64 x 128 signature matrix A of 64 planes x (16 theta x 8 rho) bins
 * (GetSignatureMatrix, D.h:1862-1932), its top singular pair (JacobiSVD, D.h:1850-1859) as the 192-float signature [u, v], and a
 * brute-force 1-NN detection over the stored signatures.  The numerics contract is DESIGN.md section 4 "M2DP"; in short:
 *   * the frame is computed in fp64 (fixed-order reduction, 3 x 3 Jacobi eigen-solver), axes sorted by descending eigenvalue,
 *     axes 0 and 1 flipped so that the sum of the cubed projected coordinates along each is >= 0 and axis 2 = axis0 x axis1 (a
 *     documented departure: PCL's signs are whatever Eigen returns; this makes the descriptor rotation invariant), then rounded
 *     to float as PCL holds it; every point is projected in float;
 *   * maxRho = max sqrtf(x*x + x*x + z*z) -- x twice, y absent, as the reference writes it (D.h:1836-1839);
 *   * the bins of every (point, plane) equal those of a restatement with glibc's atan2 and a correctly rounded sqrt;
 *   * the signature is the top singular pair of A with sum(u) >= 0 (the Perron pair: u, v >= 0), each double rounded to float.
 *
 * The reference's class is incomplete: detectIntraLoopClosureID / detectInterLoopClosureID have empty bodies (D.h:1998-2006),
 * and saveDescriptorAndKey reads 128 of the 192 floats makeAndSaveDescriptorAndKey emits (D.h:1989-1995).  Here:
 *   * detection follows the reference's other global-vector descriptors (GRSD / FPFH detectInterLoopClosureID, D.h:116-167,
 *     381-432): nearest neighbour by squared L2 in nanoflann's float order, the newest keyframes excluded, a threshold on the
 *     distance; the multi-robot bookkeeping (per-robot lists, local <-> global keys) is the one scl_iris.h ships;
 *   * save_from_wire takes all 192 floats; the reference's 128-float read truncates its own message and is not reproduced.
 * dist_thres = 0.3 is a PLACEHOLDER that no one has validated on real data: the reference gives none.
 * Conventions as in scl_engine.h (status codes, point clouds as pointer / count / stride, no CPU fallback).
 */
#ifndef SCL_M2DP_H
#define SCL_M2DP_H

#include <stdint.h>

#include "scl_engine.h"
#include "scl_plugin_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the grid is fixed, as the reference's Eigen::Matrix<double, 64, 128> A (D.h:2018-2021, 2028) */
#define SCL_M2DP_NUM_T 16      /* theta bins  */
#define SCL_M2DP_NUM_R 8       /* rho bins    */
#define SCL_M2DP_NUM_P 4       /* azimuths    */
#define SCL_M2DP_NUM_Q 16      /* elevations  */
#define SCL_M2DP_ROWS 64       /* planes: row = azimuth * 16 + elevation                    */
#define SCL_M2DP_COLS 128      /* bins: column = rho_bin * 16 + theta_bin (hist's column-major index) */
#define SCL_M2DP_DIM 192       /* signature: u (64) then v (128)                             */
#define SCL_M2DP_MAX_GROUP 16  /* scans per launch group of scl_m2dp_make_and_save_many      */

typedef struct scl_m2dp scl_m2dp;

typedef struct scl_m2dp_config {
    int    device;
    double dist_thres;          /* 0.3: loop accepted when dist < dist_thres.  A PLACEHOLDER, not validated on real data  */
    int    num_exclude_recent;  /* 30: newest keyframes of this robot kept out of intra detection (GRSD / FPFH, D.h:187, 452) */
    int    robot_num;           /* 1  */
    int    this_id;             /* 0  */
} scl_m2dp_config;

int  scl_m2dp_default_config(scl_m2dp_config *cfg);
int  scl_m2dp_create(const scl_m2dp_config *cfg, scl_m2dp **out);
int  scl_m2dp_destroy(scl_m2dp *h);
const char *scl_m2dp_last_error(const scl_m2dp *h);

/* the signature of one cloud (D.h:1820-1863): 192 floats [u, v].  Nothing is stored.  n_points < 3 or a non-finite x / y / z
 * -> SCL_ERR_INVALID_ARG (PCL's PCA throws on the first). */
int  scl_m2dp_make(scl_m2dp *h, const void *points, int n_points, int stride_bytes, float *out_values);
/* makeAndSaveDescriptorAndKey, D.h:1820-1863: the signature is built and appended; out_values (192 floats) may be NULL */
int  scl_m2dp_make_and_save(scl_m2dp *h, const void *points, int n_points, int stride_bytes, int8_t robot, int index, float *out_values);
/* `count` clouds (clouds[i], n_points[i], one stride), appended in order as robots[i] / indexs[i]; built in launch groups of
 * up to SCL_M2DP_MAX_GROUP scans, the signatures written on the device straight into the database.  out_values (count * 192
 * floats) may be NULL.  If any cloud is invalid, SCL_ERR_INVALID_ARG and nothing of the call is stored. */
int  scl_m2dp_make_and_save_many(scl_m2dp *h, const void *const *clouds, const int *n_points, int stride_bytes,
                                 const int8_t *robots, const int *indexs, int count, float *out_values);
/* saveDescriptorAndKey(const float*), D.h:1989-1995, but all 192 floats as emitted above (the reference reads 128).  The
 * values are not checked.  In the detections a NaN squared distance (a row holding a NaN, or inf - inf) never beats another
 * one, as in nanoflann's result set; when every candidate's is NaN (the query row itself holds a NaN) nothing is found:
 * *loop_id = -1 and *dist = NaN.  A row with an infinity is at distance +inf from every finite row. */
int  scl_m2dp_save_from_wire(scl_m2dp *h, const float *values, int8_t robot, int index);

/* getSize(idIn): id = -1 -> keyframes of all robots, else those of robot `id` */
int  scl_m2dp_get_size(const scl_m2dp *h);
int  scl_m2dp_get_size_of(const scl_m2dp *h, int id);
/* getIndex(key), D.h:2008-2011: global key -> (robot, index) */
int  scl_m2dp_get_index(const scl_m2dp *h, int key, int8_t *robot, int *index);
/* global key of robot `robot`'s local keyframe `local` */
int  scl_m2dp_local_to_global(const scl_m2dp *h, int robot, int local, int *key);
/* the stored 192 floats of keyframe `key` */
int  scl_m2dp_get_signature(scl_m2dp *h, int key, float *values);

/* detectIntraLoopClosureID(cur): cur = LOCAL index among this_id's keyframes; the nearest signature among this robot's
 * keyframes [0, cur - num_exclude_recent) (squared L2 in float: groups of four d0*d0 + d1*d1 + d2*d2 + d3*d3 added to the
 * running sum, nanoflann's order; ties to the lowest key); *dist = sqrtf of that sum (+inf if the set is empty);
 * *loop_id = LOCAL index of the nearest if dist < dist_thres, else -1. */
int  scl_m2dp_detect_intra(scl_m2dp *h, int cur, int *loop_id, float *dist);
/* detectInterLoopClosureID(cur): cur = GLOBAL key; a keyframe of this robot is searched among all other robots' keyframes,
 * a received one among this robot's (as scl_iris_detect_inter); *loop_id = GLOBAL key or -1. */
int  scl_m2dp_detect_inter(scl_m2dp *h, int cur, int *loop_id, float *dist);

/* THE BATCH FORMS (scl_plugin_batch.h has the rules): scl_m2dp_detect_intra_many, scl_m2dp_detect_inter_many,
 * scl_m2dp_save_from_wire_many and scl_m2dp_make_save_and_detect -- what the single calls in array order answer, bit for bit,
 * 16 queries per launch and one wait for the device per call */
SCL_PLUGIN_BATCH_API(scl_m2dp);

/* THE CANDIDATE LISTS (scl_plugin_batch.h has the rules): scl_m2dp_detect_intra_topk and scl_m2dp_detect_inter_topk -- the k <=
 * SCL_PLUGIN_TOPK_MAX nearest of the set the _many form searches, without dist_thres; the reported distance is over all 192 floats, so it rises with the rank */
SCL_PLUGIN_TOPK_API(scl_m2dp);

/* TEST HOOK: for one cloud, the 64 x 128 integer counts of A (row-major: plane row, bin column; A = counts / n_points), the
 * float frame (mean[3], axes[9]: axis k = axes[3k .. 3k+2], signs applied) and maxRho.  Any output may be NULL. */
int  scl_m2dp_signature_matrix(scl_m2dp *h, const void *points, int n_points, int stride_bytes, uint32_t *counts,
                               float *mean, float *axes, float *max_rho);
/* TEST / BENCH HOOK, totals since creation: (point, plane) decisions made, decisions that took the exact theta-edge path, and
 * the device time of the launch groups' kernel chains in microseconds (events around the chain, copies excluded).  Any output
 * may be NULL. */
int  scl_m2dp_stats(const scl_m2dp *h, unsigned long long *decisions, unsigned long long *exact, double *kernel_us);

#ifdef __cplusplus
}
#endif
#endif /* SCL_M2DP_H */
