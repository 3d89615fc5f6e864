/*
 * scl_fpfh.h -- C ABI of the FPFH descriptor plugin (Rusu, Blodow, Beetz: "Fast Point Feature Histograms (FPFH) for 3D
 * registration", ICRA 2009): the fifth descriptor of the reference's run-time switch (class fpfh_descriptor,
 * include/descriptor.h:253-460; selected by descriptorType, distributedMapping.h:99, 402-421).
 *
 * What the reference computes per keyframe (the voxel-filtered cloud, N points): normals by PCA over each point's 10 nearest
 * points, flipped towards the origin; then the SPFH of the LAST point only against the points [0, N - 2] -- three 11-bin
 * histograms of PCL's pair features, every vote adding 100 / (N - 2) -- as the 33-float descriptor.  On the GPU, per launch group
 * of up to 16 scans: a uniform grid per scan (cells sorted by the segmented radix sort), a fused 10-NN search + normal per point,
 * the pair features of the N - 2 pairs counted into integer bins, and the counts turned into the floats PCL's sequential `+=`
 * leaves, written straight into the database.  The numerics contract is DESIGN.md section 4 "FPFH"; in short:
 *   * neighbours: the min(10, N) points with the smallest (d2, index), d2 = (dx*dx + dy*dy) + dz*dz in float (exact; FLANN's tie
 *     order is not pinned);
 *   * normals: fp64 mean and scatter in (d2, index) order, a cyclic Jacobi eigensolver, the smallest eigenvalue's vector rounded
 *     to float, then PCL's float viewpoint flip.  A DEPARTURE: PCL's float covariance and closed-form eigen33 agree only to
 *     ~1e-6, so normals are not bit-comparable with the reference's binaries;
 *   * pair features: PCL's computePairFeatures in Eigen's Vector4f operation order, glibc's acosf and atan2f restated;
 *   * values: exactly the floats of count sequential `+= 100.0f / (float)(N - 2)` additions.
 *
 * The reference's class is incomplete: detectIntraLoopClosureID has an empty body (D.h:376-379) and the inter detection's distance
 * is taken over 21 of the 33 floats (save() maps 21, D.h:302, 415-416).  Here:
 *   * detect_inter with inter_mode 0 is the reference's: nothing before num_exclude_recent + 1 keyframes (result (-1, 0)); every
 *     tree_making_period-th call the search set becomes the global keys [0, size - num_exclude_recent) of ALL robots (a stale
 *     snapshot between rebuilds; the query may be in it); the 1-NN in 33 dimensions; the distance reported over the first
 *     report_dims (21) floats; a loop when it is < dist_thres (100);
 *   * inter_mode 1 is scl_m2dp_detect_inter's: other robots' keyframes for one of this robot, this robot's for a received one;
 *   * detect_intra works: this robot's keyframes [0, cur - num_exclude_recent);
 *   * the 1-NN is exact (brute force, ties to the lowest key; nanoflann's tie order depends on its tree and is not pinned).
 * Conventions as in scl_engine.h (status codes, point clouds as pointer / count / stride, no CPU fallback).
 */
#ifndef SCL_FPFH_H
#define SCL_FPFH_H

#include <stdint.h>

#include "scl_engine.h"
#include "scl_plugin_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SCL_FPFH_BINS 11        /* bins per feature (nr_subdiv, D.h:338)                          */
#define SCL_FPFH_DIM 33         /* descriptor: hist_f1, hist_f2, hist_f3                          */
#define SCL_FPFH_K 10           /* neighbours of the normal estimation (setKSearch(10), D.h:319)   */
#define SCL_FPFH_MAX_GROUP 16   /* scans per launch group of scl_fpfh_make_and_save_many          */

typedef struct scl_fpfh scl_fpfh;

typedef struct scl_fpfh_config {
    int    device;
    double dist_thres;          /* 100: a loop when dist < dist_thres (D.h:420)                                 */
    int    num_exclude_recent;  /* 30 (D.h:453)                                                                 */
    int    tree_making_period;  /* 10: the inter search set is rebuilt every 10th call (D.h:455, 394-401)        */
    int    report_dims;         /* 21: the reported distance is over the first 21 floats (D.h:302); 1 .. 33       */
    int    inter_mode;          /* 0: the reference's inter detection; 1: as scl_m2dp_detect_inter              */
    int    robot_num;           /* 1 */
    int    this_id;             /* 0 */
} scl_fpfh_config;

int  scl_fpfh_default_config(scl_fpfh_config *cfg);
int  scl_fpfh_create(const scl_fpfh_config *cfg, scl_fpfh **out);
int  scl_fpfh_destroy(scl_fpfh *h);
const char *scl_fpfh_last_error(const scl_fpfh *h);

/* the descriptor of one cloud (D.h:308-365): 33 floats.  Nothing is stored.  n_points < 3 or a non-finite x / y / z ->
 * SCL_ERR_INVALID_ARG. */
int  scl_fpfh_make(scl_fpfh *h, const void *points, int n_points, int stride_bytes, float *out_values);
/* makeAndSaveDescriptorAndKey: built and appended; out_values (33 floats) may be NULL */
int  scl_fpfh_make_and_save(scl_fpfh *h, const void *points, int n_points, int stride_bytes, int8_t robot, int index, float *out_values);
/* `count` clouds appended in order as robots[i] / indexs[i], built in launch groups of up to SCL_FPFH_MAX_GROUP scans, written
 * on the device straight into the database; out_values (count * 33 floats) may be NULL.  If any cloud is invalid,
 * SCL_ERR_INVALID_ARG and nothing of the call is stored. */
int  scl_fpfh_make_and_save_many(scl_fpfh *h, const void *const *clouds, const int *n_points, int stride_bytes,
                                 const int8_t *robots, const int *indexs, int count, float *out_values);
/* saveDescriptorAndKey(const float*), D.h:367-374: all 33 floats.  The values are not checked.  In the detections a NaN 33-D
 * squared distance (a row holding a NaN, or inf - inf) never beats another one, as in nanoflann's result set; when every
 * candidate's is NaN (the query row itself holds a NaN, in any of the 33 floats) nothing is found: *loop_id = -1 and
 * *dist = NaN, whatever report_dims is. */
int  scl_fpfh_save_from_wire(scl_fpfh *h, const float *values, int8_t robot, int index);

int  scl_fpfh_get_size(const scl_fpfh *h);
/* id = -1 -> keyframes of all robots, else those of robot `id` */
int  scl_fpfh_get_size_of(const scl_fpfh *h, int id);
/* getIndex(key): global key -> (robot, index) */
int  scl_fpfh_get_index(const scl_fpfh *h, int key, int8_t *robot, int *index);
int  scl_fpfh_local_to_global(const scl_fpfh *h, int robot, int local, int *key);
int  scl_fpfh_get_signature(scl_fpfh *h, int key, float *values);

/* cur = LOCAL index among this_id's keyframes; the nearest (33-D squared L2 in nanoflann's float order: groups of four
 * d0*d0 + d1*d1 + d2*d2 + d3*d3 added to the running sum, then the 33rd term; ties to the lowest key) among this robot's
 * keyframes [0, cur - num_exclude_recent); *dist = sqrtf of the same sum over the first report_dims floats (+inf, loop -1 if
 * the range is empty); *loop_id = LOCAL index of the nearest if dist < dist_thres, else -1. */
int  scl_fpfh_detect_intra(scl_fpfh *h, int cur, int *loop_id, float *dist);
/* cur = GLOBAL key; inter_mode 0: the reference's semantics above (*dist = 0 before num_exclude_recent + 1 keyframes);
 * inter_mode 1: as scl_m2dp_detect_inter.  *loop_id = GLOBAL key or -1. */
int  scl_fpfh_detect_inter(scl_fpfh *h, int cur, int *loop_id, float *dist);

/* THE BATCH FORMS (scl_plugin_batch.h has the rules): scl_fpfh_detect_intra_many, scl_fpfh_detect_inter_many,
 * scl_fpfh_save_from_wire_many and scl_fpfh_make_save_and_detect -- what the single calls in array order answer, bit for bit,
 * 16 queries per launch and one wait for the device per call */
SCL_PLUGIN_BATCH_API(scl_fpfh);

/* THE CANDIDATE LISTS (scl_plugin_batch.h has the rules): scl_fpfh_detect_intra_topk and scl_fpfh_detect_inter_topk -- the k <=
 * SCL_PLUGIN_TOPK_MAX nearest of the set the _many form searches, without dist_thres; the ranking is over all 33 floats but the reported
 * distance over report_dims (21) of them, so cand_dists need NOT be monotone in the rank */
SCL_PLUGIN_TOPK_API(scl_fpfh);

/* TEST HOOKS (one cloud each; any output may be NULL):
 * neighbours: n_points x min(10, n_points) int32 indices and float d2, in (d2, index) order, rows in input order */
int  scl_fpfh_neighbors(scl_fpfh *h, const void *points, int n_points, int stride_bytes, int32_t *idx, float *d2);
/* normals: n_points x 3 floats in input order */
int  scl_fpfh_normals(scl_fpfh *h, const void *points, int n_points, int stride_bytes, float *normals);
/* the 33 integer bin counts of the SPFH and the number of skipped pairs */
int  scl_fpfh_counts(scl_fpfh *h, const void *points, int n_points, int stride_bytes, uint32_t *counts, uint32_t *skipped);
/* the closed form on the host (no handle, no device): out[i] = the float after counts[i] sequential `+= hist_incr` from 0 */
int  scl_fpfh_values(const uint32_t *counts, int n, float hist_incr, float *out);
/* the device's acosf over the float bit patterns of blocks [first_block, first_block + n_blocks) of 2^24: one checksum per
 * block as tests/golden/acosf_blocks.json */
int  scl_fpfh_acosf_blocks(scl_fpfh *h, int first_block, int n_blocks, uint64_t *checksums);
/* totals since creation: points described, candidate distances evaluated by the neighbour search, device microseconds of the
 * launch groups' kernel chains (events around the chain, copies excluded) */
int  scl_fpfh_stats(const scl_fpfh *h, unsigned long long *points, unsigned long long *candidates, double *kernel_us);

#ifdef __cplusplus
}
#endif
#endif /* SCL_FPFH_H */
