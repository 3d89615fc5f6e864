/*
 * scl_grsd.h -- C ABI of the GRSD descriptor plugin (Marton, Pangercic, Blodow, Beetz: "Combined 2D-3D categorization and
 * classification for multimodal perception systems", IJRR 2011; the global radius-based surface descriptor): the last descriptor of
 * the reference's run-time switch (class grsd_descriptor, include/descriptor.h:38-196; selected by descriptorType,
 * distributedMapping.h:99, 402-421).
 *
 * What the reference computes per keyframe: normals of the whole cloud by a radius search (neRadius = 0.5 m), then
 * pcl::GRSDEstimation with a search radius of 2.0 m -- the cloud down-sampled by a VoxelGrid of leaf 2.0 m, for every voxel
 * centroid the minimum and maximum local curvature radius over the input points within 2.0 m (RSD), one of five surface classes per
 * voxel, and the 6 x 6 matrix of class transitions between every voxel and its 26 neighbour cells (class 5 = empty), whose
 * symmetrised upper triangle is the 21-float descriptor.  On the GPU, per launch group of up to 16 scans: the points of every scan
 * sorted by voxel (one grid on the voxel lattice serves both radius searches), a normal per point, a centroid per voxel, one wave
 * per voxel for the RSD, the transitions counted in integers, the 21 floats written straight into the database.  The numerics
 * contract is DESIGN.md section 4 "GRSD"; every stage is independent of traversal order.  In short:
 *   * neighbours of a point / centroid: every input point with float d2 = (dx*dx + dy*dy) + dz*dz STRICTLY below (float)(r * r)
 *     (FLANN's boundary convention is not pinned), the point itself included;
 *   * normals: fewer than 3 neighbours -> a NaN triple, flagged invalid; else the scatter from exact int64 sums of the neighbours'
 *     offsets in units of 2^-20 m, a cyclic Jacobi eigensolver in fp64, the smallest eigenvalue's vector rounded to float, PCL's
 *     float viewpoint flip.  A DEPARTURE from PCL's float covariance: normals are not bit-comparable with the reference's binaries;
 *   * voxels: pcl::VoxelGrid as scl_voxel_grid (floor(p * 1/leaf) - min_b in fp32, x fastest, fp32 centroid sums in input order,
 *     ascending voxel index); a voxel index range beyond int32 is SCL_ERR_INVALID_ARG;
 *   * RSD: angles between the normal of the neighbour nearest to the centroid and every valid neighbour normal by glibc's float
 *     acosf (PCL: double acos, a departure of ~1e-7 rad), folded into [0, pi/2], min / max per distance bin (5 bins), radii in fp64;
 *   * classes by PCL's getSimpleType; the histogram out[k++] = T[i][j] + T[j][i], i = 0..5, j = i..5.
 *
 * The reference's class is incomplete: detectIntraLoopClosureID has an empty body (D.h:111-114).  Here:
 *   * detect_inter with inter_mode 0 is the reference's (D.h:116-167): nothing before num_exclude_recent + 1 keyframes (result
 *     (-1, 0)); every tree_making_period-th call the search set becomes the global keys [0, size - num_exclude_recent) of ALL robots
 *     (a stale snapshot between rebuilds; the query may be in it); the 1-NN over the 21 floats; *dist = sqrtf of that squared
 *     distance; a loop when it is < dist_thres (160);
 *   * inter_mode 1 is scl_m2dp_detect_inter's: other robots' keyframes for one of this robot, this robot's for a received one;
 *   * detect_intra works: this robot's keyframes [0, cur - num_exclude_recent);
 *   * the 1-NN is exact (brute force, ties to the lowest key; nanoflann's tie order depends on its tree and is not pinned).
 * Conventions as in scl_engine.h (status codes, point clouds as pointer / count / stride, no CPU fallback).
 */
#ifndef SCL_GRSD_H
#define SCL_GRSD_H

#include <stdint.h>

#include "scl_engine.h"
#include "scl_plugin_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SCL_GRSD_DIM 21          /* descriptor: the upper triangle of the symmetrised 6 x 6 transition matrix */
#define SCL_GRSD_CLASSES 6       /* noise, plane, cylinder, sphere, edge, empty                                */
#define SCL_GRSD_MAX_GROUP 16    /* scans per launch group of scl_grsd_make_and_save_many                      */
#define SCL_GRSD_MAX_POINTS (1 << 22)   /* points per cloud                                                    */

typedef struct scl_grsd scl_grsd;

typedef struct scl_grsd_config {
    int    device;
    double ne_radius;           /* 0.5: radius of the normal estimation (D.h:186); 0 < ne_radius <= 1: the int64 sums of the
                                 * scatter hold |q| <= 2^20 per axis, q*q <= 2^40, over 2^22 points <= 2^62                 */
    double grsd_radius;         /* 2.0: voxel leaf and RSD search radius (setRadiusSearch(2.0), D.h:89); 0 < r <= 1e6       */
    double dist_thres;          /* 160: a loop when dist < dist_thres (D.h:155)                                            */
    int    num_exclude_recent;  /* 30 (D.h:187)                                                                            */
    int    tree_making_period;  /* 10: the inter search set is rebuilt every 10th call (D.h:189, 129-137)                  */
    int    inter_mode;          /* 0: the reference's inter detection; 1: as scl_m2dp_detect_inter                         */
    int    robot_num;           /* 1 */
    int    this_id;             /* 0 */
} scl_grsd_config;

int  scl_grsd_default_config(scl_grsd_config *cfg);
int  scl_grsd_create(const scl_grsd_config *cfg, scl_grsd **out);
int  scl_grsd_destroy(scl_grsd *h);
const char *scl_grsd_last_error(const scl_grsd *h);

/* the descriptor of one cloud (D.h:57-100): 21 floats.  Nothing is stored.  n_points < 1, more than SCL_GRSD_MAX_POINTS, a
 * non-finite x / y / z or a voxel index range beyond int32 -> SCL_ERR_INVALID_ARG. */
int  scl_grsd_make(scl_grsd *h, const void *points, int n_points, int stride_bytes, float *out_values);
/* makeAndSaveDescriptorAndKey: built and appended; out_values (21 floats) may be NULL */
int  scl_grsd_make_and_save(scl_grsd *h, const void *points, int n_points, int stride_bytes, int8_t robot, int index, float *out_values);
/* `count` clouds appended in order as robots[i] / indexs[i], built in launch groups of up to SCL_GRSD_MAX_GROUP scans, written
 * on the device straight into the database; out_values (count * 21 floats) may be NULL.  If any cloud is invalid,
 * SCL_ERR_INVALID_ARG and nothing of the call is stored. */
int  scl_grsd_make_and_save_many(scl_grsd *h, const void *const *clouds, const int *n_points, int stride_bytes,
                                 const int8_t *robots, const int *indexs, int count, float *out_values);
/* saveDescriptorAndKey(const float*), D.h:102-109: 21 floats.  The values are not checked.  In the detections a NaN squared
 * distance (a row holding a NaN, or inf - inf) never beats another one, as in nanoflann's result set; when every candidate's is
 * NaN (the query row itself holds a NaN) nothing is found: *loop_id = -1 and *dist = NaN. */
int  scl_grsd_save_from_wire(scl_grsd *h, const float *values, int8_t robot, int index);

int  scl_grsd_get_size(const scl_grsd *h);
/* id = -1 -> keyframes of all robots, else those of robot `id` */
int  scl_grsd_get_size_of(const scl_grsd *h, int id);
/* getIndex(key): global key -> (robot, index) */
int  scl_grsd_get_index(const scl_grsd *h, int key, int8_t *robot, int *index);
int  scl_grsd_local_to_global(const scl_grsd *h, int robot, int local, int *key);
int  scl_grsd_get_signature(scl_grsd *h, int key, float *values);

/* cur = LOCAL index among this_id's keyframes; the nearest (21-D squared L2 in nanoflann's float order: groups of four
 * ((d0*d0 + d1*d1) + d2*d2) + d3*d3 added to the running sum, then the 21st term; ties to the lowest key) among this robot's
 * keyframes [0, cur - num_exclude_recent); *dist = sqrtf of that sum (+inf, loop -1 if the range is empty); *loop_id = LOCAL
 * index of the nearest if dist < dist_thres, else -1. */
int  scl_grsd_detect_intra(scl_grsd *h, int cur, int *loop_id, float *dist);
/* cur = GLOBAL key; inter_mode 0: the reference's semantics above (*dist = 0 before num_exclude_recent + 1 keyframes);
 * inter_mode 1: as scl_m2dp_detect_inter.  *loop_id = GLOBAL key or -1. */
int  scl_grsd_detect_inter(scl_grsd *h, int cur, int *loop_id, float *dist);

/* THE BATCH FORMS (scl_plugin_batch.h has the rules): scl_grsd_detect_intra_many, scl_grsd_detect_inter_many,
 * scl_grsd_save_from_wire_many and scl_grsd_make_save_and_detect -- what the single calls in array order answer, bit for bit,
 * 16 queries per launch and one wait for the device per call */
SCL_PLUGIN_BATCH_API(scl_grsd);

/* THE CANDIDATE LISTS (scl_plugin_batch.h has the rules): scl_grsd_detect_intra_topk and scl_grsd_detect_inter_topk -- the k <=
 * SCL_PLUGIN_TOPK_MAX nearest of the set the _many form searches, without dist_thres; the reported distance is over all 21 floats, so it rises with the rank */
SCL_PLUGIN_TOPK_API(scl_grsd);

/* TEST HOOKS (one cloud each; any output may be NULL):
 * normals: n_points x 3 floats in input order (NaN triples where invalid) and n_points validity flags (1 / 0) */
int  scl_grsd_normals(scl_grsd *h, const void *points, int n_points, int stride_bytes, float *normals, uint8_t *valid);
/* voxels in ascending voxel index: *n_voxels, and per voxel the centroid (3 floats), r_min, r_max and the class; every array
 * has room for n_points voxels */
int  scl_grsd_voxels(scl_grsd *h, const void *points, int n_points, int stride_bytes, int *n_voxels, float *centroids,
                     float *r_min, float *r_max, int32_t *classes);
/* the 36 transition counters T[class][neighbour's class], row-major */
int  scl_grsd_transitions(scl_grsd *h, const void *points, int n_points, int stride_bytes, uint32_t *counters);
/* totals since creation: points described, voxels classified, device microseconds of the launch groups' kernel chains (events
 * around the chain, copies excluded) */
int  scl_grsd_stats(const scl_grsd *h, unsigned long long *points, unsigned long long *voxels, double *kernel_us);

#ifdef __cplusplus
}
#endif
#endif /* SCL_GRSD_H */
