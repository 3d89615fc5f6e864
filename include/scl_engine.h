/*
 * scl_engine.h -- C ABI of the MI355X-native Scan Context loop-closure engine.
 *
 * This is the drop-in boundary for ONE path of thisparticle/scl_slam (ROS
 * package dlc_slam): Scan Context place recognition + geometric verification.
 * Plain pointers and sizes only; no C++/torch types; never throws.
 *
 * Each entry point names the reference interface it replaces
 *   D.h  = include/descriptor.h          (class scan_descriptor, D.h:21-36;
 *                                          scan_context_descriptor, D.h:1304-1801)
 *   DM.h = include/distributedMapping.h  (loop-closure driver)
 * A header-only C++ adapter with the reference's six virtuals lives in
 * include/scl/scan_context_hip_descriptor.hpp; INTEGRATION.md shows the
 * one-line change at DM.h:404.
 *
 * Conventions
 *   - every function returns an scl_status (0 = ok, < 0 = error);
 *   - "values" is the wire format of msg/global_descriptor.msg:8 `float32[]
 *     values`: R*S floats, ROW-major (ring-major), D.h:1446-1455 / 1576-1582;
 *   - point clouds are (base pointer, count, stride_bytes) with x,y,z as three
 *     consecutive floats at the start of each record (pcl::PointXYZI: stride 32);
 *   - "no loop" is loop_id == -1 exactly as D.h:1615,1678;
 *   - an engine is internally synchronised: append and detect may be called
 *     from different threads (the reference calls detect* without mtxSC,
 *     DM.h:1078,1280, while save() runs under it, DM.h:1001-1003).
 *   - all compute runs on the GPU; there is no CPU fallback.  Without a HIP
 *     device scl_create fails with SCL_ERR_NO_DEVICE.
 */
#ifndef SCL_ENGINE_H
#define SCL_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct scl_engine scl_engine;

typedef enum scl_status {
    SCL_OK               =  0,
    SCL_ERR_INVALID_ARG  = -1,
    SCL_ERR_NO_DEVICE    = -2,
    SCL_ERR_HIP          = -3,
    SCL_ERR_OUT_OF_RANGE = -4,
    SCL_ERR_NOMEM        = -5,
    SCL_ERR_UNSUPPORTED  = -6,
    SCL_ERR_NUMERIC      = -7     /* a factorisation met a pivot it refuses (scl_pgo_solve_condensed) */
} scl_status;

/* Constructor arguments of scan_context_descriptor, D.h:1307-1316 (same
 * defaults), plus engine-side knobs. */
typedef struct scl_config {
    /* The grid: 1 <= num_ring <= 256, 2 <= num_sector <= 224 (the sector masks hold 224 bits; one sector has no shift to search), and
     * 900-odd bytes of on-chip memory per ring at 224 sectors: 4 * (num_ring * (num_sector + 1) + num_sector + 2) + 24 * num_sector
     * + 256 <= 163840 bytes -- 174 rings at 224 sectors, all 256 rings up to 154 sectors.  scl_create answers SCL_ERR_INVALID_ARG
     * outside 1..256 x 1..1024 and SCL_ERR_UNSUPPORTED for any other grid beyond these limits, before it touches the device; a
     * grid it accepts is bit-exact against the reference through the descriptor front end and the plain search. */
    int    num_ring;            /* PC_NUM_RING              = 20   */
    int    num_sector;          /* PC_NUM_SECTOR            = 60   */
    int    num_candidates;      /* NUM_CANDIDATES_FROM_TREE = 3    */
    double dist_thres;          /* SC_DIST_THRES            = 0.14 */
    double lidar_height;        /* LIDAR_HEIGHT             = 1.65 */
    double max_radius;          /* PC_MAX_RADIUS            = 80.0 */
    int    num_exclude_recent;  /* NUM_EXCLUDE_RECENT       = 100  */
    int    tree_making_period;  /* TREE_MAKING_PERIOD_      = 10   */
    double search_ratio;        /* SEARCH_RATIO             = 0.1  */
    float  knn_exclude_eps;     /* 0 = nanoflann semantics (D.h:1716); FLT_EPSILON =
                                   libnabo self-match exclusion (D.h:1642)          */
    int    device;              /* HIP device ordinal                     = 0    */
    int    initial_capacity;    /* keyframe slots preallocated (grows x2) = 4096 */
} scl_config;

/* Accumulated device time per kernel family, measured with HIP events on the
 * engine's own stream while profiling is enabled (scl_profile_enable). */
typedef struct scl_profile {
    double   sc_distance_ms;   uint64_t sc_distance_launches;  uint64_t sc_distance_pairs;
    double   ringkey_topk_ms;  uint64_t ringkey_topk_launches;
    double   argmin_ms;        uint64_t argmin_launches;
    double   make_sc_ms;       uint64_t make_sc_launches;      uint64_t make_sc_points;
    double   ingest_ms;        uint64_t ingest_launches;
    double   icp_nn_ms;        uint64_t icp_nn_launches;
    double   icp_reduce_ms;    uint64_t icp_reduce_launches;
} scl_profile;

const char *scl_status_string(int status);
const char *scl_last_error(const scl_engine *e);       /* detail of the last failure */
int  scl_abi_version(void);

int  scl_default_config(scl_config *cfg);
int  scl_create(const scl_config *cfg, scl_engine **out);     /* ctor, D.h:1307-1344 */
int  scl_destroy(scl_engine *e);
/* The same constructor for ONE keyframe database sharded over the GPUs of a node (BASELINE configs[3]): one
 * process, one engine state per entry of devices[], keyframe g on shard g % n_devices; every entry point of this
 * header works on the returned engine exactly as on a one-GPU engine (same results, bit for bit: the search
 * range of D.h:1627 is applied on global indices, ties go to the lowest global index).  Scoring needs no
 * exchange; the per-shard winners of the full-DB mode are reduced with two RCCL min all-reduces on packed 64-bit
 * keys (exchange = 2; needs every shard on its own device), or on the host from pinned memory (exchange = 1);
 * exchange = 0 picks RCCL when n_devices > 1 and the devices are distinct, else the host merge.  The same device
 * may be listed more than once (several shards on one GPU: rehearsal of the multi-GPU path on a one-GPU box).
 * The collective library is librccl unless the environment names another one (SCL_RCCL_LIB=/path/to/lib: a newer RCCL build, or
 * the stand-in the tests link -- tests/cpp/mock_rccl.cpp, the ranks' element-wise minimum formed on the host --, which is how the
 * G > 1 control flow of exchange = 2 runs on a one-GPU box: RCCL itself refuses two ranks on one device).
 * With more than one shard every shard also keeps the query-side rows of the newest 1024 keyframes of each OTHER shard (copied
 * device to device when a keyframe is appended: 66 KB per keyframe at 64x120, n_devices x 1024 rows per shard), so that searching
 * for a recent keyframe -- what detection does -- moves nothing between the devices; older keyframes are copied when asked for.
 * Geometric verification of one scan's candidates (scl_icp_align_batch) is spread over the shards by candidate;
 * other geometry calls and the keyframe store live on devices[0].  cfg->device is ignored. */
int  scl_create_sharded(const scl_config *cfg, const int *devices, int n_devices, int exchange, scl_engine **out);
/* number of shards (1 for scl_create) and the exchange in use (0 none, 1 host merge, 2 min all-reduces through the collective library); either may be NULL */
int  scl_shard_info(const scl_engine *e, int *n_shards, int *exchange);

/* ---- the six virtuals of scan_descriptor (D.h:21-36) ----------------------- */

/* makeAndSaveDescriptorAndKey, D.h:25 / 1604-1611 (called at DM.h:1002).
 * out_values (R*S floats, may be NULL) receives the vector the reference returns. */
int  scl_make_and_save(scl_engine *e, const void *points, int n_points, int stride_bytes,
                       int8_t robot, int index, float *out_values);
/* saveDescriptorAndKey, D.h:27 / 1572-1585 (called at DM.h:627). */
int  scl_save_from_wire(scl_engine *e, const float *values, int8_t robot, int index);
/* detectIntraLoopClosureID, D.h:29 / 1613-1674 (called at DM.h:1078).
 * shift = ring shift as float (D.h:1665); dist (may be NULL) = the float-narrowed
 * running minimum of D.h:1655 widened back to double. */
int  scl_detect_intra(scl_engine *e, int cur, int *loop_id, float *shift, double *dist);
/* detectInterLoopClosureID, D.h:31 / 1676-1756 (called at DM.h:1280);
 * yaw_rad as D.h:1752.  Latent defects of the reference are repaired, see DESIGN.md. */
int  scl_detect_inter(scl_engine *e, int cur, int *loop_id, float *yaw_rad, double *dist);
/* getIndex, D.h:33 / 1758-1761 */
int  scl_get_index(const scl_engine *e, int key, int8_t *robot, int *index);
/* getSize, D.h:35 / 1763-1766: returns the size (>= 0) or a negative status. */
int  scl_get_size(const scl_engine *e, int id);

/* ---- bulk / building-block entry points ----------------------------------- */

/* makeDescriptors (DM.h:996-1002) in one call: pcl::VoxelGrid with leaf `leaf` (descriptLeafSize) on the raw scan,
 * then makeAndSaveDescriptorAndKey on the filtered cloud, which stays on the device.  *n_filtered (optional) =
 * points after the filter.  Same descriptor, key and database state as scl_voxel_grid + scl_make_and_save. */
int  scl_make_and_save_filtered(scl_engine *e, const void *points, int n_points, int stride_bytes, float leaf,
                                int8_t robot, int index, float *out_values, int *n_filtered);
/* makeDescriptors for a BATCH of keyframes (DM.h:988-1025 runs once per keyframe; a robot team's keyframes arrive together, and a
 * map that is loaded or replayed arrives all at once): `count` clouds -> `count` descriptors appended in order, as `count` calls of
 * scl_make_and_save would (same descriptors, keys and database state, bit for bit).  Groups of up to 16 scans cost two kernel
 * launches each (one scatter over all the clouds, one ingest that writes every array of their slots); a group's clouds travel to
 * the device while the group before is processed -- by DMA when the buffers are pinned (scl_host_alloc / scl_host_register).
 * robots / indexs may be NULL (robot 0, index = slot); out_values may be NULL, else count x R*S floats (the wire format of
 * global_descriptor.values, D.h:1446-1456, per scan). */
int  scl_make_and_save_many(scl_engine *e, const void *const *clouds, const int *n_points, int count, int stride_bytes,
                            const int8_t *robots, const int *indexs, float *out_values);
/* The per-incoming-scan pipeline from raw points in one call: for scan i, makeAndSaveDescriptorAndKey (DM.h:1002; keyframe
 * key_i = size before the call + i) and then the full-database detection of that keyframe over [0, key_i - NUM_EXCLUDE_RECENT)
 * (D.h:1627; scl_detect_full's rule): nn_idx[i] = arg-min keyframe (-1: empty range), shift[i], dist[i] = its fp64 SC distance --
 * what scl_make_and_save + scl_detect_full_range give scan by scan, bit for bit.  Same grouping and copy overlap as
 * scl_make_and_save_many; the caller applies the threshold (dist < dist_thres, D.h:1662). */
int  scl_stream_from_points(scl_engine *e, const void *const *clouds, const int *n_points, int n_scans, int stride_bytes,
                            const int8_t *robots, const int *indexs, int *nn_idx, int *shift, double *dist, float *out_values);
/* The same for keyframes whose clouds are already in the on-device keyframe store (scl_keyframe_put, DM.h:674): keyframes
 * first_index .. first_index + count - 1 of `robot` get their descriptors built from the stored clouds and are appended as
 * (robot, index); then each is searched for over [0, key - NUM_EXCLUDE_RECENT).  Nothing crosses PCIe but the results (and the
 * descriptor values when out_values is given): the path's rate with its inputs resident in HBM.  Same results as
 * scl_stream_from_points on the same clouds. */
int  scl_stream_from_store(scl_engine *e, int robot, int first_index, int count, int *nn_idx, int *shift, double *dist, float *out_values);
/* Pinned host memory for point clouds: a cloud handed over from such a buffer goes to the device by DMA, without the runtime's
 * staging copy, and overlaps the kernels of the scans before it.  scl_host_alloc buffers are freed by scl_host_free or with the
 * engine; scl_host_register pins memory the caller owns (e.g. a pcl::PointCloud's points) until scl_host_unregister. */
int  scl_host_alloc(scl_engine *e, size_t bytes, void **out);
int  scl_host_free(scl_engine *e, void *p);
int  scl_host_register(scl_engine *e, void *p, size_t bytes);
int  scl_host_unregister(scl_engine *e, void *p);
/* makeScancontext only (D.h:1404-1461), nothing is stored. */
int  scl_make_descriptor(scl_engine *e, const void *points, int n_points, int stride_bytes,
                         float *out_values);
/* count descriptors at once; robots/indexs may be NULL (robot 0, index = slot). */
int  scl_save_bulk(scl_engine *e, const float *values, int count,
                   const int8_t *robots, const int *indexs);
/* read back: descriptor in wire format, ring key (D.h:1463-1475, R floats),
 * sector key (D.h:1477-1489, S doubles) */
int  scl_get_descriptor(const scl_engine *e, int key, float *values);
int  scl_get_ringkey(const scl_engine *e, int key, float *ringkey);
int  scl_get_sectorkey(const scl_engine *e, int key, double *sectorkey);

/* `count` descriptors first .. first+count-1 in wire format (count * R*S floats) */
int  scl_get_descriptors(const scl_engine *e, int first, int count, float *values);
/* Reverse of getIndex (D.h:1758-1761): the database key of keyframe `index` of robot `robot`, or -1 (*key) when it
 * is not in the database -- the index mapping of performInterLoopClosure, DM.h:1281-1284. */
int  scl_find_key(const scl_engine *e, int8_t robot, int index, int *key);
/* The whole keyframe database as a flat file: header {magic, version, R, S, N}, float32[N][R*S] descriptors in
 * wire order (D.h:1446-1455), then N x {int32 robot, int32 index} (the map of D.h:1758-1761).  Keys, norms and the
 * tiled layouts are derived data and are rebuilt on load.  load appends to the engine's database (an empty one-GPU engine
 * reproduces the dumped one exactly: same keys, same detections -- the header's reserved words carry the counter and range
 * of detectInterLoopClosureID's periodic tree, D.h:1691-1703; a sharded engine restarts that period); the grid must match.
 * load checks the file's length against its header before sizing anything by it and fails with SCL_ERR_INVALID_ARG /
 * SCL_ERR_NOMEM, never by an exception; a load that fails midway (I/O error, device memory) leaves the keyframes appended
 * so far in the database: *n_loaded says how many. */
int  scl_db_dump_file(scl_engine *e, const char *path);
int  scl_db_load_file(scl_engine *e, const char *path, int *n_loaded);

/* Stage an external query descriptor (wire format) that is NOT stored in the DB;
 * afterwards pass SCL_QUERY_STAGED as `query`.  Used by the sharded (multi-GPU)
 * driver, where the query keyframe may live on another rank. */
#define SCL_QUERY_STAGED (-1)
int  scl_stage_query(scl_engine *e, const float *values);

/* Exact k nearest ring keys among DB slots [lo, hi): replaces both KD-trees
 * (libnabo D.h:1631-1642, nanoflann D.h:1699-1716).  Squared L2 in fp32 with
 * nanoflann's accumulation order (nanoflann.hpp:383-408); ascending distance,
 * ties -> lower index; unfilled slots idx = -1, d2 = FLT_MAX.
 * Returns the number found in *found (may be NULL). */
int  scl_ringkey_topk(scl_engine *e, int query, int lo, int hi, int k,
                      int *idx, float *d2, int *found);
/* distanceBtnScanContext (D.h:1538-1569) of `query` against cand[0..n)
 * (cand == NULL: slots 0..n-1).  dist[i] is bit-identical to the fp64 value of
 * the sequential CPU evaluation; shift[i] the arg-min ring shift. */
int  scl_sc_distance_batch(scl_engine *e, int query, const int *cand, int n,
                           double *dist, int *shift);
/* The distance MATRIX of north_star ("the column-shifted SC distance matrix over the keyframe database"): row r =
 * distanceBtnScanContext (D.h:1538-1569) of keyframe queries[r] (or a staged query, -1 - slot) against the keyframes
 * lo .. hi-1; dist / shift are nq x (hi - lo), row-major.  Every entry is the exact fp64 evaluation (bit-identical to the
 * sequential CPU evaluation, as scl_sc_distance_batch).  On the screened grids (64x120, 80x180) the screening pass first tells,
 * per pair, which of the 2 SR + 1 shifts can still hold the minimum (a guaranteed bound: DESIGN.md section 4), and the fp64
 * arithmetic of the reference is then carried out at those shifts only -- the result is the same number; the environment switch
 * SCL_MATRIX_PLAIN=1 evaluates every shift of every pair.  Several rows share a launch and a launch's results travel to the
 * host while the next one runs. */
int  scl_sc_distance_matrix(scl_engine *e, const int *queries, int nq, int lo, int hi, double *dist, int *shift);
/*
 * THE RANKED SEARCH.  scl_detect_full* reports the one arg-min of a scan's search set and scl_topk_with_distance ranks by RING KEY
 * (the reference's pre-selection) before it scores; these two calls score a query against its WHOLE search set with the distance
 * that decides and return the k best, ranked, for a verifier that takes several candidates (scl_loop_icp_batch_from_store's
 * keys_pre; BASELINE C3: 25 ICP verifications per query) or for rank statistics.  Shape and conventions are those of
 * scl_iris_search_* (scl_iris.h) and SCL_PLUGIN_TOPK_API (scl_plugin_batch.h): cand_ids, cand_shifts and cand_dists hold
 * n_queries * k elements, row i for query i; n_found holds n_queries elements; cand_shifts, cand_dists and n_found may be NULL;
 * n_queries == 0 is SCL_OK.
 *   * Search set of query i.  scl_sc_search_range: keyframe queries[i] (or a staged query, -1 - slot, as scl_sc_distance_matrix
 *     takes it) against the keyframes lo[i] .. hi[i]-1.  scl_sc_search: the set of scl_detect_full, keyframe curs[i] against
 *     [0, curs[i] - num_exclude_recent) (D.h:1627; empty when that is <= 0).  ids are database slots, which are global keys; the
 *     query itself is listed like any other keyframe when it lies in its range.
 *   * Score of a pair: distanceBtnScanContext (D.h:1538-1569) with its arg-min shift -- bit for bit the fp64 value and the shift
 *     of scl_sc_distance_matrix and scl_sc_distance_batch (the same kernels produce it; the screened grids evaluate the open
 *     shifts only, as there).
 *   * The list: the k smallest scores in ascending (distance compared as doubles with <, position in the range) order -- equal
 *     distances go to the lower keyframe, by value and not by bit pattern (-0.0 ties with 0.0).  A pair is listed only if its
 *     distance is < 10000000.0, the rule of the engine's arg-min: an empty descriptor scores exactly 10000000.0 and is never listed,
 *     NaN is never listed.  n_found[i] = min(k, listable pairs); entries j >= n_found[i] are id -1, shift 0, distance 10000000.0,
 *     the engine's "no winner" values.
 *   * No threshold, no loop decision: the caller applies dist_thres.  The result does not depend on num_candidates, dist_thres,
 *     knn_exclude_eps or tree_making_period, and the calls change nothing a later call can see (the periodic tree's counter of
 *     scl_detect_inter included).
 *   * k < 1 or k > SCL_SC_SEARCH_MAX or a NULL required pointer: SCL_ERR_INVALID_ARG.  A query out of range (for scl_sc_search
 *     every cur < 0 too): SCL_ERR_OUT_OF_RANGE; a staged slot that holds nothing: SCL_ERR_INVALID_ARG; a range with lo < 0,
 *     hi > size or hi < lo: SCL_ERR_OUT_OF_RANGE -- the matrix's rule, not the clipping of scl_detect_full_range.  All of it before
 *     anything runs: no output written, no state changed.
 * The rows come from the distance matrix's own launches, queries in call order in groups of 4 (16 on the screened grids); the
 * selection of a group runs on the device behind its rows, and rows x k records travel to the host instead of 12 bytes per pair.
 * A group's matrix runs over the union [min lo, max hi) of its queries' ranges and each list is cut from its own range: widely
 * different ranges in one group cost the union.  The host waits for the device once per call.  On a scl_create_sharded engine
 * every query runs once per shard over the shard's slots of its range and the shards' lists are merged on the host by (distance,
 * global key), whatever the exchange: the same lists, bit for bit.
 */
#define SCL_SC_SEARCH_MAX 32     /* the longest list; = SCL_PLUGIN_TOPK_MAX, SCL_IRIS_SEARCH_MAX */

int  scl_sc_search_range(scl_engine *e, const int *queries, const int *lo, const int *hi, int n_queries, int k,
                         int *cand_ids, int *cand_shifts, double *cand_dists, int *n_found);
int  scl_sc_search(scl_engine *e, const int *curs, int count, int k,
                   int *cand_ids, int *cand_shifts, double *cand_dists, int *n_found);
/*
 * THE RANKED SEARCH PER ROBOT.  The database is one slot sequence for the whole team (the own robot's keyframes and every received
 * one, DM.h:627 and DM.h:1002), and once two robots' keyframes interleave no slot range is "this robot's older keyframes" or "that
 * robot's keyframes".  These two calls are scl_sc_search over search sets defined by the VALUE of each keyframe's (robot, index), the
 * pair scl_get_index returns (robot 0 and index = slot for keyframes saved without them).  Output shape, optional pointers, k,
 * count == 0, the score of a pair, the order, the < 10000000.0 rule and the fillers behind n_found are scl_sc_search's; ids are
 * global slots, and equal distances go to the lower slot among the eligible ones.  curs[i] is a database key; let (r_i, x_i) be its
 * robot and index.
 *   * scl_sc_search_intra: every slot s with robot[s] == r_i and index[s] < x_i - num_exclude_recent (D.h:1627 on the robot's own
 *     keyframe numbering, the rule of scl_iris_search_intra; the bound is formed in 64 bits).  Slot order plays no part: a keyframe
 *     that arrived out of order, a duplicate (robot, index) and a slot behind curs[i] are judged by the rule like any other.  With
 *     num_exclude_recent >= 0 the query is never in its own set.  In a one-robot database with index = slot the lists are
 *     scl_sc_search's, bit for bit.
 *   * scl_sc_search_inter, robot_pre == SCL_SC_ANY_OTHER_ROBOT: every slot with robot[s] != r_i.  No index rule: other robots'
 *     keyframes are not temporal neighbours.  A keyframe stored with a negative robot id counts as another robot here.
 *   * scl_sc_search_inter, robot_pre in 0 .. 127: every slot with robot[s] == robot_pre -- the list to hand to
 *     scl_geometric_verification_batch_from_store*(robot = robot_pre) once scl_get_index has turned the ids into that robot's keys.
 *     A negative robot id cannot be named.
 *   * Errors, all before anything runs (no output written, no state changed): those of scl_sc_search -- a NULL required pointer,
 *     count < 0, k outside [1, SCL_SC_SEARCH_MAX]: SCL_ERR_INVALID_ARG; a cur < 0 or >= size: SCL_ERR_OUT_OF_RANGE --, and
 *     robot_pre < -1 or > 127, or robot_pre == r_i for any i (the intra set without its recency rule: a mistake):
 *     SCL_ERR_INVALID_ARG.
 *   * Not offered: staged (unsaved) queries -- the reference saves a received descriptor before it searches for it, DM.h:625-628.
 * Like scl_sc_search the calls leave nothing a later call can see and do not depend on num_candidates, dist_thres, knn_exclude_eps or
 * tree_making_period.  The rule is applied in the selection on the device, which reads a copy of (robot, index) per slot that a search
 * brings up to date before its first launch.  A query's matrix runs over [its first eligible slot, its last eligible slot + 1) --
 * a team map loaded in per-robot blocks does not score the other blocks --; inside that span ineligible keyframes are scored and then
 * dropped.  On a scl_create_sharded engine: the same lists, bit for bit.
 */
#define SCL_SC_ANY_OTHER_ROBOT (-1)
int  scl_sc_search_intra(scl_engine *e, const int *curs, int count, int k,
                         int *cand_ids, int *cand_shifts, double *cand_dists, int *n_found);
int  scl_sc_search_inter(scl_engine *e, const int *curs, int count, int robot_pre, int k,
                         int *cand_ids, int *cand_shifts, double *cand_dists, int *n_found);
/* BASELINE "full-DB" mode: ring-key top-k AND the shifted SC distance against
 * every eligible slot [0, hi) with hi = cur - num_exclude_recent (D.h:1627), then
 * the global arg-min (ties -> lowest slot).  nn_idx/shift/dist describe the best
 * slot; loop_id = nn_idx iff dist < dist_thres else -1.
 * With query == SCL_QUERY_STAGED, `hi` is given explicitly via scl_detect_full_range. */
int  scl_detect_full(scl_engine *e, int cur, int *loop_id, int *nn_idx, int *shift, double *dist);
int  scl_detect_full_range(scl_engine *e, int query, int lo, int hi,
                           int *nn_idx, int *shift, double *dist);
/* Pipelined form of scl_detect_full_range for streams of scans: submit enqueues the pass and returns a
 * ticket at once (up to 8 may be in flight, results are collected in any order); collect blocks until
 * that pass has finished.  scl_detect_full_range == submit + collect. */
int  scl_detect_full_submit(scl_engine *e, int query, int lo, int hi, int *ticket);
/* Several keyframes of the database as queries in ONE launch (scans of several robots arriving together,
 * or a backlog): query i = keyframe queries[i] against [lo[i], hi[i]); tickets[i] is collected like a
 * ticket of scl_detect_full_submit.  Up to 4 queries share a launch (more are split); staged queries
 * (SCL_QUERY_STAGED) and grids without the fused kernel fall back to one launch per query. */
int  scl_detect_full_submit_many(scl_engine *e, const int *queries, const int *lo, const int *hi, int n_queries, int *tickets);
/* A backlog of n_queries scans in one call: the submit / collect pipeline of the two calls above run natively
 * (scans_per_launch queries per kernel launch, launches_in_flight launches enqueued ahead), results in
 * submission order.  Blocks until the last scan is done; no other pass may be in flight.
 * scans_per_launch is the size of a launch GROUP (the unit of alignment, finishing and buffer sets), not a promise of
 * one pass over the database per group: on the 64x120 grid two consecutive full groups (16 scans each) of a chunk may
 * share one pass -- one products launch with two scan sets -- with results bit-identical to separate launches
 * (SCL_SCREEN_PAIR=0 keeps every group's pass to itself). */
int  scl_detect_full_stream(scl_engine *e, const int *queries, const int *lo, const int *hi, int n_queries,
                            int scans_per_launch, int launches_in_flight, int *nn_idx, int *shift, double *dist);
int  scl_detect_full_collect(scl_engine *e, int ticket, int *nn_idx, int *shift, double *dist);
/* Diagnostic view of the screening pass behind the full-DB mode on the 64x120 grid (scl_slam_amd/csrc/sc_screen.hip):
 * approx[i] = the reduced-precision (fp16 matrix-core) evaluation of distanceBtnScanContext (D.h:1538-1569) of
 * `query` against slot lo + i -- the reference's own alignment, its 13 shifts -- guaranteed within *eps of the fp64
 * value (-inf: the keyframe is always scored exactly); survivors[0 .. *n_survivors) = the slots (ascending) that can
 * still hold the minimum and are re-scored by the exact fp64 kernel.  The full-DB entry points return the exact
 * winner; this call exists so that tests can check the bound on the hardware.  survivors (n entries), n_survivors
 * and eps may be NULL.  SCL_ERR_UNSUPPORTED on other grids. */
int  scl_screen_distances(scl_engine *e, int query, int lo, int hi, float *approx, int *survivors, int *n_survivors, float *eps);
/* ... of up to 16 scans in ONE screening launch (the stream form's batch: the products' second form, every column of its matrix
 * products): approx[i * n + k] = scan queries[i] against slot lo + k, n = the clipped range's length.  No survivor lists. */
int  scl_screen_distances_many(scl_engine *e, const int *queries, int n_queries, int lo, int hi, float *approx, float *eps);
/* The ring-key top-k (num_candidates entries) computed as part of the last scl_detect_full[_range]. */
int  scl_get_last_topk(scl_engine *e, int k, int *idx, float *d2);
/* Reference-faithful candidates for the sharded driver: local ring-key top-k in
 * [lo,hi) plus the SC distance/shift of each (one device pass, no host round trip). */
int  scl_topk_with_distance(scl_engine *e, int query, int lo, int hi, int k,
                            int *idx, float *d2, double *dist, int *shift, int *found);

/* ---- geometric verification (PCL objects inlined at DM.h:1108-1121, 1211-1230) */

/* Coordinates far from the origin.  The clouds of this section are in world frames, so they may lie kilometres out, where a float32
 * coordinate has a quantum of 1.2e-4 m (2 km) to 4.9e-4 m (8 km).  Two promises hold there.  The searches are exact for any finite
 * float32 input: scl_nn_correspondences[_moved], the search inside the ICP loops (in memory and by tiles), scl_target_normals' radius
 * search, scl_voxel_grid's voxel indices and with them scl_assemble_submap answer what brute force over the same float32 numbers
 * answers -- indices, distance bits and ties (lowest index) included; RANSAC's hypotheses are formed in double and its mask, count
 * and winning hypothesis are the restatement's.  The transforms are as accurate as float32 coordinates allow: T is returned in
 * float, so a rotation rounded to 2^-24 is carried over the distance from the origin as a lever (5e-4 m at 8 km, per increment of
 * an ICP loop), and an alignment 8 km out is reproduced to a centimetre or two (measured 5 to 7 mm, held to 18 to 29 mm), not to the
 * 1e-5 it is held to near the origin.  The stop criteria feel the same quantum: with the default transformation epsilon (1e-6 on
 * the squared translation, i.e. 1 mm) an alignment that stops after 6 iterations near the origin needs 21 to 40 at 8 km, where one
 * increment cannot be smaller than the lever's rounding.  The measured bars per distance are in tests/offset_cases.py (ICP) and
 * tests/test_verification_cases.py (the rigid fit); tests/test_gpu_registration_offsets.py holds the kernels to both promises at 0,
 * 500, 2 000 and 8 000 m.  Callers that need more than that should subtract a common origin before the call. */

typedef struct scl_icp_params {
    int    max_iterations;            /* icp.setMaximumIterations(50)        DM.h:1110 */
    double max_correspondence_dist;   /* icp.setMaxCorrespondenceDistance(100) DM.h:1109 */
    double transformation_epsilon;    /* icp.setTransformationEpsilon(1e-6)  DM.h:1111 */
    double euclidean_fitness_epsilon; /* icp.setEuclideanFitnessEpsilon(1e-6) DM.h:1112 */
    int    estimator;                 /* 0 = point-to-point SVD (reference, DM.h:1108), 1 = point-to-plane LLS
                                         (BASELINE configs[2]; target normals by PCA within normal_radius) */
    double normal_radius;             /* neighbourhood radius of the target normals, metres (1.0) */
} scl_icp_params;

int  scl_icp_default_params(scl_icp_params *p);
/* pcl::IterativeClosestPoint::align + getFitnessScore, DM.h:1108-1121.
 * T = 4x4 row-major final transformation (source -> target). */
int  scl_icp_align(scl_engine *e, const void *src, int n_src, const void *tgt, int n_tgt,
                   int stride_bytes, const scl_icp_params *p,
                   float T[16], float *fitness, int *converged, int *iterations);
/* The same alignment for the n_targets loop candidates of one scan (BASELINE configs[2]: ICP on the
 * top-25 candidates): one source against tgts[c] (n_tgts[c] points), up to four alignments in flight on
 * internal streams.  T: n_targets x 16 floats; fitness / converged / iterations: n_targets entries
 * (each may be NULL).  Per-candidate results are those of scl_icp_align. */
int  scl_icp_align_batch(scl_engine *e, const void *src, int n_src, const void *const *tgts, const int *n_tgts,
                         int n_targets, int stride_bytes, const scl_icp_params *p,
                         float *T, float *fitness, int *converged, int *iterations);
/* CorrespondenceEstimation::determineCorrespondences, DM.h:1211-1215:
 * exact 1-NN of every source point in the target (ties -> lowest target index). */
int  scl_nn_correspondences(scl_engine *e, const void *src, int n_src, const void *tgt, int n_tgt,
                            int stride_bytes, int *nn_index, float *nn_dist2);
/* The correspondences of the source moved by T (row-major 4x4, DM.h:247-249 arithmetic), searched from those of the
 * unmoved source: the warm neighbour search of an ICP iteration (pcl::IterativeClosestPoint's loop body, DM.h:1119) on
 * its own.  Results equal scl_nn_correspondences on the moved cloud. */
int  scl_nn_correspondences_moved(scl_engine *e, const void *src, int n_src, const void *tgt, int n_tgt,
                                  int stride_bytes, const float T[16], int *nn_index, float *nn_dist2);
/* TransformationEstimationSVD::estimateRigidTransformation, DM.h:1228-1230,
 * over correspondence pairs (src_index[i], tgt_index[i]). */
int  scl_rigid_svd(scl_engine *e, const void *src, int n_src, const void *tgt, int n_tgt,
                   int stride_bytes, const int *src_index, const int *tgt_index, int n_corr,
                   float T[16]);
/* CorrespondenceRejectorSampleConsensus::getCorrespondences, DM.h:1218-1225 (ransacMaxIter DM.h:187,
 * ransacOutlierTreshold DM.h:188).  Deterministic: hypothesis h draws its 3 correspondences from a
 * counter-based generator of (seed, h); every one of max_iterations hypotheses is scored; best = most
 * inliers, ties -> lowest h.  inlier_mask[n_corr] (0/1), T_model = the winning 3-point model (may be NULL). */
int  scl_ransac_correspondences(scl_engine *e, const void *src, int n_src, const void *tgt, int n_tgt,
                                int stride_bytes, const int *src_index, const int *tgt_index, int n_corr,
                                int max_iterations, double inlier_threshold, uint64_t seed,
                                int *inlier_mask, int *n_inliers, int *best_hypothesis, float T_model[16]);
/* The compute core of geometricVerificationService, DM.h:1211-1243: NN correspondences -> RANSAC ->
 * SVD transform on the inliers -> gate `inliers >= inlier_ratio * correspondences` (inlierTreshold DM.h:189).
 * Only a source point whose search found a neighbour is a correspondence (one with a NaN or infinite coordinate finds
 * none): they are kept in source order, *n_correspondences is their count, and RANSAC samples from, scores and gates
 * on that count.  Fewer than three: T = identity, *success = 0, the count reported. */
int  scl_geometric_verification(scl_engine *e, const void *src, int n_src, const void *tgt, int n_tgt,
                                int stride_bytes, int ransac_iterations, double inlier_threshold,
                                double inlier_ratio, uint64_t seed, float T[16], int *success,
                                int *n_correspondences, int *n_inliers);
/* pcl::VoxelGrid::filter with one leaf size (DM.h:501,503; DM.h:996-998, 1183-1185, 1200-1201): one point
 * per occupied voxel = centroid of x, y, z and intensity, ascending voxel index.  out must hold out_capacity
 * records (n_points always suffices).  When the voxel index range overflows int32 the input is returned
 * unchanged, as PCL does. */
int  scl_voxel_grid(scl_engine *e, const void *points, int n_points, int stride_bytes, float leaf,
                    void *out, int out_capacity, int *n_out);
/* pcl::getTransformation(x, y, z, roll, pitch, yaw) (DM.h:223,241) as a row-major 4x4; host-side helper */
int  scl_pose_to_matrix(float x, float y, float z, float roll, float pitch, float yaw, float T[16]);
/* pcl::getTranslationAndEulerAngles (DM.h:1133, 1139): roll = atan2(R21, R22), pitch = asin(-R20), yaw = atan2(R10, R00) */
int  scl_matrix_to_pose(const float T[16], float *x, float *y, float *z, float *roll, float *pitch, float *yaw);
/* The tail of the ICP block, DM.h:1130-1141 (and DM.h:1249-1259 with the SVD transform): tfCorrect = T_icp * tfWrong
 * (pose_cur = x, y, z, roll, pitch, yaw of the current keyframe, float like Affine3f), poseFrom = its Euler pose,
 * poseTo = pose_pre, result = poseFrom.between(poseTo) in double: between_xyz_q = translation x, y, z and the unit
 * quaternion x, y, z, w (w >= 0) -- the fields of loop_info.betPose / poseBetween --, between_rpy (optional) =
 * roll, pitch, yaw of the same rotation. */
int  scl_loop_pose_between(const float T_icp[16], const float pose_cur[6], const float pose_pre[6], double between_xyz_q[7], double between_rpy[3]);
/* The initial guess of an inter-robot verification from a Scan Context match; host-side helper, no engine.  shift = the ring shift
 * the search reported for (query = the received keyframe, candidate) -- scl_sc_search's cand_shifts --, num_sector = the grid's,
 * pose_cur / pose_pre = x, y, z, roll, pitch, yaw of the received keyframe in its robot's world frame (the received cloud is in that
 * frame, DM.h:1333) and of the candidate keyframe in the other robot's.  G = M(pose_pre) * Rz(yaw) * M(pose_cur)^-1, M the matrix of
 * scl_pose_to_matrix, M^-1 the rigid inverse [R^T | -R^T t]: the received cloud back in its sensor frame, turned by the descriptor's
 * yaw, placed at the candidate keyframe's pose.  distanceBtnScanContext shifts the CANDIDATE's columns right by `shift` (D.h:1376-1378,
 * 1559), so the query turns by yaw = -shift * 2 pi / num_sector (shift taken modulo num_sector).  Built in double from the float
 * inputs, rounded to float once.  The shift resolves the yaw to half a sector only.  num_sector < 1, a NULL pointer or a non-finite
 * pose: SCL_ERR_INVALID_ARG. */
int  scl_loop_guess_from_shift(int shift, int num_sector, const float pose_cur[6], const float pose_pre[6], float G[16]);
/* loopFindNearKeyframes, DM.h:1163-1186: concatenation of transformPointCloud(cloud_i, T_i) (DM.h:234-253)
 * followed by the voxel filter.  transforms = n_clouds row-major 4x4 matrices. */
int  scl_assemble_submap(scl_engine *e, const void *const *clouds, const int *counts, const float *transforms,
                         int n_clouds, int stride_bytes, float leaf, void *out, int out_capacity, int *n_out);
/* paramsServer::transformPointCloud, DM.h:234-253 (xyz transformed, rest copied) */
int  scl_transform_cloud(scl_engine *e, const void *in, int n, int stride_bytes,
                         const float T[16], void *out);

/* ---- on-device keyframe store ------------------------------------------------
 * robots[id].keyFrameArray (DM.h:86; filled at DM.h:983-985) kept resident in HBM, so that submap
 * assembly and the ICP of a loop candidate move only poses across PCIe, not clouds.
 * Records have one stride per engine (fixed by the first put).  Keyframes are dense per robot
 * (index = position in keyFrameArray); putting an existing index replaces that cloud. */
int  scl_keyframe_put(scl_engine *e, int robot, int index, const void *points, int n_points, int stride_bytes);
/* keyFrameArray.size() of one robot (highest stored index + 1) */
int  scl_keyframe_count(const scl_engine *e, int robot);
/* read one stored cloud back (out may be NULL to query the size only) */
int  scl_keyframe_get(scl_engine *e, int robot, int index, void *out, int out_capacity, int *n_points);
/* loopFindNearKeyframes(nearKeyframes, key, searchNum), DM.h:1163-1186, from the store: keyframes
 * key-searchNum .. key+searchNum that exist, each moved by its pose, concatenated in index order and
 * voxel-filtered with `leaf`.  poses: (2*search_num+1) row-major 4x4 matrices, poses[i] belonging to
 * keyframe key-search_num+i (entries of keyframes outside [0, count) are ignored). */
int  scl_submap_from_store(scl_engine *e, int robot, int key, int search_num, const float *poses, float leaf,
                           void *out, int out_capacity, int *n_out);
/* performIntraLoopClosure stage 2, DM.h:1104-1121, entirely on the device: source = submap(key_cur, 0),
 * target = submap(key_pre, search_num), size gate (DM.h:1108: fewer than min_src_points / min_tgt_points
 * -> no alignment, *converged = 0, T = identity), then scl_icp_align's alignment. */
int  scl_loop_icp_from_store(scl_engine *e, int robot, int key_cur, const float *pose_cur,
                             int key_pre, int search_num, const float *poses_pre, float leaf,
                             const scl_icp_params *p, int min_src_points, int min_tgt_points,
                             float T[16], float *fitness, int *converged, int *iterations, int *n_src, int *n_tgt);
/* The same stage for the n_candidates loop candidates of ONE scan (BASELINE configs[2]: ICP on the top-25 candidates):
 * the source submap is built once, every candidate's target submap comes from the store (keys_pre[c], its window of
 * 2 * search_num + 1 poses at poses_pre + c * (2 * search_num + 1) * 16), and the ICP loops of all candidates run fused
 * -- every loop step is one launch for the whole batch.  Outputs are per candidate (T: n_candidates x 16); candidates
 * that fail the size gate keep T = identity, converged = 0.  Per-candidate results equal scl_loop_icp_from_store's. */
int  scl_loop_icp_batch_from_store(scl_engine *e, int robot, int key_cur, const float *pose_cur,
                                   int n_candidates, const int *keys_pre, int search_num, const float *poses_pre, float leaf,
                                   const scl_icp_params *p, int min_src_points, int min_tgt_points,
                                   float *T, float *fitness, int *converged, int *iterations, int *n_src, int *n_tgts);

/* geometricVerificationService (DM.h:1189-1268) with the submap taken from the keyframe store: voxel filter of
 * the received cloud (src_leaf), submap(key_pre, search_num) from stored keyframes (leaf), size gate
 * (DM.h:1204), then exactly scl_geometric_verification's correspondences -> RANSAC -> SVD -> inlier gate;
 * no cloud but the received one crosses PCIe. */
int  scl_geometric_verification_from_store(scl_engine *e, const void *src, int n_src, int stride_bytes, float src_leaf,
                                           int robot, int key_pre, int search_num, const float *poses_pre, float leaf,
                                           int min_src_points, int min_tgt_points,
                                           int ransac_iterations, double inlier_threshold, double inlier_ratio, uint64_t seed,
                                           float T[16], int *success, int *n_src_filtered, int *n_tgt,
                                           int *n_correspondences, int *n_inliers);

/*
 * THE BATCHED VERIFICATION.  scl_sc_search, scl_iris_search_* and scl_X_detect_*_topk hand a robot up to 32 ranked candidates per
 * query; scl_loop_icp_batch_from_store verifies such a list on the intra-robot side.  These two calls are the inter-robot side:
 * geometricVerificationService (DM.h:1189-1268) for ONE received scan against n candidates, where scl_geometric_verification and
 * scl_geometric_verification_from_store take one candidate per call (about fifteen short launches, three waits of the host, and
 * the received cloud filtered and uploaded again every time).
 *   * Arguments.  scl_geometric_verification_batch: tgts[c] / n_tgts[c] = candidate c's cloud on the host, every cloud with the
 *     source's stride.  scl_geometric_verification_batch_from_store: candidate c = submap(keys_pre[c], search_num) from the
 *     keyframe store, its window of 2 * search_num + 1 poses at poses_pre + c * (2 * search_num + 1) * 16 (the layout of
 *     scl_loop_icp_batch_from_store).  One seed serves every candidate.
 *   * Outputs.  T: n x 16 floats; success, n_correspondences, n_inliers and n_tgts: n entries each, any of them may be NULL;
 *     n_src_filtered: one int (may be NULL).  Entry c is, bit for bit, what the single call answers for candidate c with the same
 *     arguments -- T, success, the pair count and the inlier count; the size gate (a gated candidate keeps T = identity, success
 *     0, counts 0, its n_tgts reported), fewer than three pairs and fewer than three inliers included.
 *   * Errors.  A NULL required pointer, n < 0, a bad stride, a stride other than the store's, a NULL target with points,
 *     ransac_iterations outside 1 .. 2^20 when n_src >= 3 (the received cloud's size BEFORE its filter in the store form), a key
 *     whose window holds a keyframe that was never stored: the status the single call returns, before anything runs, no output
 *     written.  n == 0 is SCL_OK; the store form still filters the received cloud and reports n_src_filtered.
 *   * How it runs.  Candidates go in rounds of 32.  The received cloud is filtered and placed on the device once per call.  A
 *     round is one chain on the engine's stream -- submaps (the batched voxel filter), search grids, one cold neighbour search,
 *     pairs, RANSAC scoring / pick / mask, masked covariance, solve -- every step one launch over all candidates of the round, a
 *     candidate's pair count staying on the device; the host waits once per round behind the submaps' sizes.  On a
 *     scl_create_sharded engine the calls run on the shard that owns the keyframe store, like the other store calls.
 */
int  scl_geometric_verification_batch(scl_engine *e, const void *src, int n_src,
                                      const void *const *tgts, const int *n_tgts, int n_targets, int stride_bytes,
                                      int ransac_iterations, double inlier_threshold, double inlier_ratio, uint64_t seed,
                                      float *T, int *success, int *n_correspondences, int *n_inliers);
int  scl_geometric_verification_batch_from_store(scl_engine *e, const void *src, int n_src, int stride_bytes, float src_leaf,
                                                 int robot, int n_candidates, const int *keys_pre, int search_num, const float *poses_pre, float leaf,
                                                 int min_src_points, int min_tgt_points,
                                                 int ransac_iterations, double inlier_threshold, double inlier_ratio, uint64_t seed,
                                                 float *T, int *success, int *n_src_filtered, int *n_tgts,
                                                 int *n_correspondences, int *n_inliers);

/*
 * THE BATCHED VERIFICATION WITH INITIAL GUESSES.  Nearest-neighbour pairs mean something only between clouds that are nearly aligned,
 * and two robots' world frames are not: the ranked search reports a ring shift per candidate (scl_loop_guess_from_shift turns it and
 * the two keyframe poses into a motion), and these two calls take one such motion per candidate.
 *   * Arguments.  Those of the pair above, and guesses: n x 16 floats, candidate c's G_c = guesses + 16 * c, a row-major 4x4 whose
 *     first three rows are read (the last is taken as 0, 0, 0, 1).  Candidate c's source is the received cloud moved by G_c with the
 *     arithmetic of scl_transform_cloud (DM.h:247-249); fields other than x, y, z play no part.  In the store form the received cloud
 *     is voxel-filtered FIRST, once, with src_leaf, and the filtered cloud is moved per candidate.
 *   * Outputs.  T_fit (n x 16, may be NULL), success, n_correspondences, n_inliers: entry c is, bit for bit, what
 *     scl_geometric_verification answers for (scl_transform_cloud(src, G_c), tgts[c]) with the same arguments -- in the store form
 *     for (scl_transform_cloud(scl_voxel_grid(src, src_leaf), G_c), scl_submap_from_store(keys_pre[c], ...)) behind the size gate of
 *     the store form above, which looks at the filtered size (no guess changes it); a gated candidate keeps T = T_fit = identity,
 *     success 0, counts 0, its n_tgts reported.  T (n x 16, required): the whole motion received cloud -> candidate, T_fit[c] * G_c,
 *     every entry formed on the host in double as ((a0 b0 + a1 b1) + a2 b2) + a3 b3 and rounded to float once; where T_fit[c] is the
 *     identity because there were fewer than three pairs or inliers, T[c] is G_c with the last row 0, 0, 0, 1.  The other optional
 *     outputs as above.
 *   * Errors.  Whatever the pair above refuses, with the same status; then guesses == NULL with n > 0, or a non-finite entry in the
 *     first three rows of any guess: SCL_ERR_INVALID_ARG.  All before anything runs, no output written.  n == 0 is SCL_OK (guesses
 *     may then be NULL); the store form still reports n_src_filtered.
 *   * How it runs.  The chain of the pair above on the engine's stream, one wait per round, with one more launch per round: a
 *     (blocks, candidates) grid writes every candidate's moved source as a float4 cloud, which the cold search and the RANSAC / mask /
 *     covariance steps of that candidate read in place of the shared one.  Memory: 16 bytes x n_src per candidate of a round (at
 *     most 32), in the candidates' grow-only workspaces; a later call without guesses does not read them.  Sharded engines: as above.
 */
int  scl_geometric_verification_batch_guess(scl_engine *e, const void *src, int n_src,
                                            const void *const *tgts, const int *n_tgts, int n_targets, int stride_bytes,
                                            const float *guesses,
                                            int ransac_iterations, double inlier_threshold, double inlier_ratio, uint64_t seed,
                                            float *T, float *T_fit, int *success, int *n_correspondences, int *n_inliers);
int  scl_geometric_verification_batch_from_store_guess(scl_engine *e, const void *src, int n_src, int stride_bytes, float src_leaf,
                                                       int robot, int n_candidates, const int *keys_pre, int search_num, const float *poses_pre, float leaf,
                                                       const float *guesses,
                                                       int min_src_points, int min_tgt_points,
                                                       int ransac_iterations, double inlier_threshold, double inlier_ratio, uint64_t seed,
                                                       float *T, float *T_fit, int *success, int *n_src_filtered, int *n_tgts,
                                                       int *n_correspondences, int *n_inliers);

/*
 * THE BATCHED ICP WITH INITIAL GUESSES.  pcl::IterativeClosestPoint::align takes a `guess`; the reference aligns every loop candidate
 * from the identity (DM.h:1107-1121) and drops the yaw Scan Context reported, so a loop entered from the opposite direction starts
 * 180 degrees off; and its inter-robot verification ends at RANSAC + SVD with a constant noise on the factor, where its own comment
 * asks for the fitness score (DM.h:1361).  These three calls are the batched ICP with one initial guess per candidate.
 *   * Arguments.  Those of the unguessed call, and guesses: n x 16 floats, candidate c's G_c = guesses + 16 * c, a row-major 4x4 whose
 *     first three rows are read (the last is taken as 0, 0, 0, 1): the layout of the guessed verification.  Candidate c's source is
 *     the source cloud moved by G_c with the arithmetic of scl_transform_cloud (DM.h:247-249); fields other than x, y, z play no part.
 *     scl_icp_align_batch_guess: scl_icp_align_batch with guesses (clouds on the host).  scl_loop_icp_batch_from_store_guess, the
 *     intra-robot side: the source is submap(key_cur, 0), moved per candidate (scl_loop_guess_from_shift with both poses of the same
 *     robot gives G_c).  scl_icp_align_batch_from_store_guess, the inter-robot side: a RECEIVED cloud, voxel-filtered once with
 *     src_leaf and then moved per candidate, against submaps from the store, with the layout and gates of
 *     scl_geometric_verification_batch_from_store_guess -- whose T is the intended guess: the call answers the refined motion and
 *     the fitness for the factor's noise.
 *   * Outputs.  T_icp (n x 16, may be NULL), fitness, converged, iterations (n entries each, may be NULL): entry c is, bit for bit,
 *     what scl_icp_align answers for (scl_transform_cloud(src, G_c), tgt_c) with the same parameters, for both estimators -- in the
 *     store forms for the store's source (submap(key_cur, 0), or scl_voxel_grid(src, src_leaf)) and
 *     scl_submap_from_store(keys_pre[c], ...).  An alignment that fails (fewer than three pairs in a search) has T_icp = identity and
 *     converged 0, as there.  T (n x 16, required): the whole motion source -> candidate, T_icp[c] * G_c, every entry formed on the
 *     host in double as ((a0 b0 + a1 b1) + a2 b2) + a3 b3 and rounded to float once; where T_icp[c] is the identity, T[c] is G_c with
 *     the last row 0, 0, 0, 1.  The size gate of the store forms looks at the unmoved sizes; a gated candidate keeps T = T_icp =
 *     identity, converged 0, fitness 0, its n_tgts reported.  Identity guesses on a cloud of finite points give the unguessed call's
 *     bits.
 *   * Errors.  Whatever the unguessed call refuses, with the same status -- its parameter checks (estimator, normal_radius,
 *     max_iterations) are made here whenever n > 0 --; the received form refuses what scl_geometric_verification_batch_from_store
 *     refuses in its cloud arguments; then guesses == NULL with n > 0, or a non-finite entry in the first three rows of any guess:
 *     SCL_ERR_INVALID_ARG.  All before anything runs, no output written; that includes a key whose window holds a keyframe that was
 *     never stored.  n == 0 is SCL_OK (guesses may then be NULL); the store forms still report the source's filtered size.
 *   * How it runs.  Rounds of 32 candidates, as the unguessed calls.  A round has, in front of the unguessed chain and on the
 *     engine's stream, one launch over all candidates for each of: the moved sources (float4 clouds in source order), their boxes,
 *     their Hilbert keys, and one stable segmented sort (three passes) -- every sum of an alignment runs in the working order of its
 *     source, so each candidate gets the order the single call derives from its own moved cloud; the working clouds and the fitness
 *     pass then read candidate c's cloud through candidate c's order.  The iterations are the unguessed call's launches.  Memory, in
 *     the grow-only control workspace: (16 + 4) bytes x n_src per candidate of a round for the sources and orders, 12 bytes x n_src
 *     per candidate and the histograms for the sort; a later call without guesses reads none of it.  On a scl_create_sharded engine
 *     scl_icp_align_batch_guess sends candidate c, with its guess, to shard c mod G; the store forms run on the shard that owns the
 *     keyframe store.
 */
int  scl_icp_align_batch_guess(scl_engine *e, const void *src, int n_src, const void *const *tgts, const int *n_tgts,
                               int n_targets, int stride_bytes, const float *guesses, const scl_icp_params *p,
                               float *T, float *T_icp, float *fitness, int *converged, int *iterations);
int  scl_loop_icp_batch_from_store_guess(scl_engine *e, int robot, int key_cur, const float *pose_cur,
                                         int n_candidates, const int *keys_pre, int search_num, const float *poses_pre, float leaf,
                                         const float *guesses, const scl_icp_params *p, int min_src_points, int min_tgt_points,
                                         float *T, float *T_icp, float *fitness, int *converged, int *iterations, int *n_src, int *n_tgts);
int  scl_icp_align_batch_from_store_guess(scl_engine *e, const void *src, int n_src, int stride_bytes, float src_leaf,
                                          int robot, int n_candidates, const int *keys_pre, int search_num, const float *poses_pre, float leaf,
                                          const float *guesses, const scl_icp_params *p, int min_src_points, int min_tgt_points,
                                          float *T, float *T_icp, float *fitness, int *converged, int *iterations,
                                          int *n_src_filtered, int *n_tgts);

/*
 * BATCHED REGISTRATION SCORING: OVERLAP, RMSE AND INFORMATION MATRIX.  The chain above ends with up to 32 motions per query and one
 * scalar per motion (ICP's fitness; the RANSAC side reports no distance at all).  The reference fills the loop factor's noise with
 * that one number on all six axes, or with a constant 0.2 and the comment "change to max fitness score" (DM.h:1361-1364).  These
 * calls answer, for every candidate at its motion T_c, what a consumer chooses among candidates by and weights the factor with:
 * how much of the source takes part, how well, and the sums the 6 x 6 information matrix of the pairs is made of.
 *   * Arguments.  Those of the guessed calls they sit beside (scl_geometric_verification_batch_guess, its store form, and
 *     scl_loop_icp_batch_from_store_guess), with transforms in the place of guesses: n x 16 floats, candidate c's T_c = transforms +
 *     16 * c, a row-major 4x4 whose first three rows are read.  Candidate c's source is the source cloud moved by T_c with the
 *     arithmetic of scl_transform_cloud (DM.h:247-249); in the store forms the filter runs first, once.  The intended T_c is the T
 *     the guessed verification or the guessed ICP returned (the T of the unguessed calls serves the same way).  max_dist: the
 *     rejection distance, metres.
 *   * Outputs, n entries each; each may be NULL, but with n > 0 at least one must be given.  n_valid[c]: the moved source points
 *     whose search found a neighbour (a point with a non-finite coordinate after the move finds none: scl_geometric_verification's
 *     rule).  n_inliers[c]: those of them with nn_dist2 <= maxd2, where maxd2 = (float)(max_dist * max_dist) and nn_dist2 is the float
 *     scl_nn_correspondences reports for (scl_transform_cloud(src, T_c), tgt_c) -- ICP's rule, equality kept.  moments[10 c .. 10 c +
 *     9]: fp64 sums over the inliers of x, y, z, xx, yy, zz, xy, xz, yz and d2 -- x, y, z the coordinates of the matched TARGET point
 *     converted to double, the products formed in double (where they are exact), d2 = (double)nn_dist2.  The sums are taken in an
 *     order that depends on n_src alone (a fixed partition into workgroups, a fixed tree inside one, the workgroups' records in
 *     order, no floating-point atomics): the same inputs give the same bits on every run, and the store forms give the bits of the
 *     host form on scl_voxel_grid's / scl_submap_from_store's clouds.  Each sum is within m * 2^-53 * sum |term| of the exact one
 *     (m = n_inliers).  The store forms' size gate looks at the unmoved sizes; a gated candidate keeps zeros, its n_tgts reported.
 *     The overlap n_inliers / n_src and the RMSE sqrt(moments[9] / n_inliers) are left to the caller.
 *   * Errors.  Whatever the corresponding guessed call refuses in the arguments they share, with the same status; then max_dist
 *     non-finite or < 0, no output given with n > 0, transforms == NULL with n > 0, or a non-finite entry in the first three rows of
 *     a transform: SCL_ERR_INVALID_ARG.  All before anything runs, no output written.  n == 0 is SCL_OK; the store forms still report
 *     the source's filtered size.
 *   * How it runs.  Rounds of 32 candidates on the engine's stream, one wait per round.  A round: the submaps (store forms), then one
 *     launch over all candidates for each of the moved sources (the guessed verification's kernel), the steps of the search grids,
 *     the cold neighbour search, the reduction (blocks x candidates) and a finishing launch of one wave per candidate.  Memory: the
 *     guessed verification's, in the same grow-only workspaces; a later call of any other batch reads nothing these calls leave.
 *     On a scl_create_sharded engine the calls run on the shard that owns the keyframe store, as the guessed verification does.
 */
int  scl_registration_eval_batch(scl_engine *e, const void *src, int n_src, const void *const *tgts, const int *n_tgts,
                                 int n_targets, int stride_bytes, const float *transforms, double max_dist,
                                 int *n_valid, int *n_inliers, double *moments);
/* inter-robot: a RECEIVED cloud, voxel-filtered once with src_leaf */
int  scl_registration_eval_batch_from_store(scl_engine *e, const void *src, int n_src, int stride_bytes, float src_leaf,
                                            int robot, int n_candidates, const int *keys_pre, int search_num, const float *poses_pre, float leaf,
                                            const float *transforms, int min_src_points, int min_tgt_points, double max_dist,
                                            int *n_valid, int *n_inliers, double *moments, int *n_src_filtered, int *n_tgts);
/* intra-robot: the source is submap(key_cur, 0) */
int  scl_loop_eval_batch_from_store(scl_engine *e, int robot, int key_cur, const float *pose_cur,
                                    int n_candidates, const int *keys_pre, int search_num, const float *poses_pre, float leaf,
                                    const float *transforms, int min_src_points, int min_tgt_points, double max_dist,
                                    int *n_valid, int *n_inliers, double *moments, int *n_src, int *n_tgts);
/* The 6 x 6 information matrix of the pairs (host only, no engine): with m = n_inliers and S the sums of one candidate, info is the
 * row-major sum of G^T G for G = [-[q]x | I3] over the matched target points q, rotation first -- the convention pose-graph tools use:
 *     Syy+Szz  -Sxy     -Sxz      0    -Sz    Sy
 *     -Sxy     Sxx+Szz  -Syz      Sz    0    -Sx
 *     -Sxz     -Syz     Sxx+Syy  -Sy    Sx    0
 *      0        Sz      -Sy       m     0     0
 *     -Sz       0        Sx       0     m     0
 *      Sy      -Sx       0        0     0     m
 * Every entry is at most one fp64 addition.  A NULL pointer or n_inliers < 0: SCL_ERR_INVALID_ARG, nothing written. */
int  scl_registration_information(int n_inliers, const double moments[10], double info[36]);

/*
 * POINT-TO-PLANE REGISTRATION SCORING: PLANE HESSIAN, RESIDUALS, NORMALS.  The matrix above is the point-to-point one: its translation
 * block is n_inliers * I3 whatever the scene looks like.  It says how many pairs there are, never which directions they constrain --
 * in a corridor, a tunnel or on open ground the answer a consumer of a loop factor needs most.  These calls score the same pairs
 * against the planes of the target: the 6 x 6 normal equations sum J^T J with J = [p x n | n], whose small eigenvalues and their
 * eigenvectors name the motions the geometry leaves free.
 *   * scl_target_normals.  The normals the point-to-plane estimator (scl_icp_params.estimator = 1) uses for this cloud and radius, n_tgt
 *     x 3 floats: over all points of the cloud with d^2 <= radius^2 in double (the point itself included), fewer than three give
 *     (0, 0, 0), otherwise the eigenvector of the smallest eigenvalue of their covariance, formed in double and rounded to float (its
 *     sign is whatever the solver leaves; the sums below do not depend on it).  The call builds its own search grid and runs the kernel
 *     body the batch paths run, as the calls below do: the same bits from both, on every run.  (These calls put the points of every
 *     grid cell in index order first, so that every sum of a covariance is taken in one order; the batched ICP, which hands no
 *     normal out, leaves a cell in the order its scatter filled it, and forms the same normals from the same neighbours up to the
 *     rare float that another order of a sum of doubles rounds differently.)  n_tgt == 0: SCL_OK.  radius: refused as scl_icp_params.normal_radius is (not > 0, or NaN: SCL_ERR_INVALID_ARG).  A stride < 12 or no multiple
 *     of 4, or a NULL pointer with n_tgt > 0: SCL_ERR_INVALID_ARG.  Nothing is written on error.
 *   * The three scoring calls take the arguments of the three calls above, and normal_radius behind max_dist.  Per candidate c at T_c,
 *     with p the source point moved by T_c in float (scl_transform_cloud's arithmetic), q its nearest target point and d2 the float
 *     nn_dist2 (scl_nn_correspondences'), n the normal of q (scl_target_normals(tgt_c, normal_radius)):
 *       n_valid, n_inliers   exactly the numbers of the calls above (d2 <= (float)(max_dist * max_dist), equality kept)
 *       n_planar             the inliers whose n is not (0, 0, 0); the other inliers add nothing to sums 0 .. 27
 *       sums[0 .. 20]        the upper triangle, row by row, of sum J^T J for
 *                            J = (p_y n_z - p_z n_y, p_z n_x - p_x n_z, p_x n_y - p_y n_x, n_x, n_y, n_z)
 *                            -- rotation first, the axis order of scl_registration_information
 *       sums[21 .. 26]       sum J r with r = (q - p) . n
 *       sums[27]             sum r r
 *       sums[28]             sum (double)d2 over ALL inliers: moments[9] of the calls above, bit for bit
 *     Every input is converted to double and every product and difference is formed in double.  The sums are taken in the order of
 *     the calls above (a function of n_src alone, no floating-point atomics): the same bits on every run, and the store forms give
 *     the bits of the host form on scl_voxel_grid's / scl_submap_from_store's clouds.
 *   * Bound.  Each of the sums 0 .. 27 lies within (m + 10) * 2^-53 * M of the exact sum over the float inputs, where m = n_planar and M
 *     is the same sum with every term replaced by its majorant: R = (|p_y n_z| + |p_z n_y|, |p_z n_x| + |p_x n_z|, |p_x n_y| + |p_y n_x|,
 *     |n_x|, |n_y|, |n_z|) for J and rbar = sum_k (|q_k| + |p_k|) |n_k| for r.  Derivation: the product of two floats is exact in
 *     double, so an entry of p x n is ONE rounding of an exact difference of exact products; every addend of r passes through at
 *     most four roundings (its difference, its product, two additions), each relative to a quantity below rbar; a term J_a J_b,
 *     J_a r or r r carries the roundings of its two factors and one of its own -- at most nine (r r: 4 + 4 + 1) --, each relative to
 *     a quantity below the term's majorant; the accumulation adds m - 1, each relative to a partial sum below M.  To first order
 *     that is (m + 8) * 2^-53 * M; the remaining 2 * 2^-53 * M cover the second-order terms for every m below 2^50.  Contraction
 *     into fma only removes roundings.
 *   * Gates, errors, rounds, n == 0, outputs: those of the calls above (with n > 0 at least one of n_valid, n_inliers, n_planar, sums
 *     must be given), and normal_radius refused as in scl_target_normals.  Nothing is written on error; a gated candidate keeps zeros
 *     and reports its n_tgts.
 *   * How it runs.  The chain of the calls above with the targets' normals in front of the cold search (one launch over all
 *     candidates), a reduction that also reads the moved point and 16 bytes of normal behind every pair, and a finishing launch of
 *     one wave per candidate.  The normals live in the slot of scl_transform_cloud's output of the candidates' workspaces, which
 *     nothing in the chain writes.  Sharded engines: served as the calls above.
 */
int  scl_target_normals(scl_engine *e, const void *tgt, int n_tgt, int stride_bytes, double radius, float *normals);
int  scl_registration_eval_plane_batch(scl_engine *e, const void *src, int n_src, const void *const *tgts, const int *n_tgts,
                                       int n_targets, int stride_bytes, const float *transforms, double max_dist, double normal_radius,
                                       int *n_valid, int *n_inliers, int *n_planar, double *sums);
int  scl_registration_eval_plane_batch_from_store(scl_engine *e, const void *src, int n_src, int stride_bytes, float src_leaf,
                                                  int robot, int n_candidates, const int *keys_pre, int search_num, const float *poses_pre, float leaf,
                                                  const float *transforms, int min_src_points, int min_tgt_points, double max_dist, double normal_radius,
                                                  int *n_valid, int *n_inliers, int *n_planar, double *sums, int *n_src_filtered, int *n_tgts);
int  scl_loop_eval_plane_batch_from_store(scl_engine *e, int robot, int key_cur, const float *pose_cur,
                                          int n_candidates, const int *keys_pre, int search_num, const float *poses_pre, float leaf,
                                          const float *transforms, int min_src_points, int min_tgt_points, double max_dist, double normal_radius,
                                          int *n_valid, int *n_inliers, int *n_planar, double *sums, int *n_src, int *n_tgts);
/* Host only, no engine: info = the row-major symmetric 6 x 6 whose upper triangle is sums[0 .. 20] (rotation first), grad (may be NULL)
 * = sums[21 .. 26], the sum of J r.  sums == NULL or info == NULL: SCL_ERR_INVALID_ARG, nothing written. */
int  scl_registration_information_plane(const double sums[29], double info[36], double grad[6]);

/*
 * PAIRWISE CONSISTENCY OF LOOP CLOSURES: MATRIX, GRAPH, MAX CLIQUE.  The outlier rejection in front of a pose-graph solve (PCM, pairwise
 * consistency maximisation; the reference hands usePCM / pcmThreshold / useHeuristics to its optimiser, DM.h:147, 296, 375-377, 533,
 * 877-880): every pair of loops between two trajectories is tested for mutual consistency through the odometry of both robots, and the
 * largest mutually consistent set is kept.  N loops are N (N - 1) / 2 independent SE(3) cycle tests in fp64 and a clique search on N-bit sets.
 *   * Inputs, for one pair of trajectories A and B (A = B is allowed, and the pointers may alias).  poses_a: n_a x 7 doubles, poses_b:
 *     n_b x 7 doubles; a pose is x, y, z and a quaternion x, y, z, w -- the layout scl_loop_pose_between writes --, X^A_k keyframe k of A in
 *     A's world frame.  Loop i: idx_a[i] in [0, n_a), idx_b[i] in [0, n_b); z + 7 i = Z_i, the pose of B's keyframe in the frame of A's
 *     keyframe (poseFrom.between(poseTo) with A the current robot, DM.h:1141); cov + 36 i, a row-major 6 x 6 covariance of the right
 *     perturbation Z_i Exp(xi), rotation first (the axis order of scl_registration_information and of gtsam's Pose3), of which only the
 *     upper triangle is read.  odom_var[6] (NULL: zeros): variance added per keyframe step -- a stated drift model; the reference has no
 *     such term (its trajectories' covariances are not available at this boundary).  Quaternions are normalised in double before use.
 *   * Statistic, for i < j.  With T_A = (X^A_ai)^-1 X^A_aj and T_B = (X^B_bj)^-1 X^B_bi the cycle is E = T_A Z_j T_B Z_i^-1, the identity
 *     for two perfect loops.  Residual r = (Log_SO3(R_E), t_E): the rotation vector from the quaternion of E with w made >= 0, 2 atan2(|v|,
 *     w) v / |v|, and 2 v where |v| = 0; the translation as it is (gtsam's default Pose3 chart).
 *         Sigma = Ad(Z_i) Sigma_i Ad(Z_i)^T + Ad(M) Sigma_j Ad(M)^T + diag(odom_var) (|a_i - a_j| + |b_i - b_j|),
 *         M = Z_i T_B^-1,   Ad(R, t) = [[R, 0], [[t]x R, R]],
 *     the first-order covariance of E's right perturbation:
 *         Z_j Exp(xi_j) moves E to T_A Z_j Exp(xi_j) (T_B Z_i^-1) = E M Exp(xi_j) M^-1   = E Exp( Ad(M)   xi_j),
 *         Z_i Exp(xi_i) moves E to T_A Z_j T_B Exp(-xi_i) Z_i^-1  = E Z_i Exp(-xi_i) Z_i^-1 = E Exp(-Ad(Z_i) xi_i).
 *     d2(i, j) = r^T Sigma^-1 r by a Cholesky factorisation in double; a pivot that is not > 0 (NaN included) gives d2 = +inf.  d2(j, i) =
 *     d2(i, j) and d2(i, i) = 0 by construction: only i < j is ever computed (the statistic taken the other way round differs for large
 *     residuals).  Everything is fp64; each pair is one fixed sequence of operations with no atomics: the same inputs give the same bits
 *     on every run.  The covariance is first order: see DESIGN.md section 4, PCM, for where that stops being enough.
 *   * Graph.  i and j are adjacent iff d2(i, j) <= threshold, equality kept; +inf and NaN are never adjacent.  adj: N rows of W = (N + 63)
 *     / 64 uint64 words, bit j of row i = word j / 64, bit j % 64; the diagonal and every bit at or beyond N are zero.  degree[i]: the
 *     popcount of row i.  threshold is a chi-square quantile with 6 degrees of freedom; for the reference's pcmThreshold (a probability):
 *     0.75 -> 7.84080, 0.90 -> 10.6446, 0.95 -> 12.5916, 0.99 -> 16.8119.
 *   * Clique.  The reference's useHeuristics = true path is a greedy maximum clique; this one is fully deterministic.  For every seed s:
 *     C = {s}, P = adj[s]; while P is not empty take the u in P with the largest |adj[u] & P|, ties to the lowest u; C += u, P &= adj[u].
 *     The answer is the largest C over all seeds, ties to the lowest seed; members in ascending order, and the winning seed.  (A seed whose
 *     degree + 1 is strictly smaller than a clique already found may be skipped: it could not even have tied, so the answer does not
 *     depend on timing.)  Exact maximum clique is out of scope.
 *   * scl_pcm_consistency: d2 (n x n), adj (n x W), degree (n); each may be NULL, one must be given with n > 0.  scl_pcm_max_clique: the
 *     clique of any graph from the host; members holds up to n entries.  scl_pcm_select: both on the device -- only the inputs and the
 *     member list cross the bus --, equal to scl_pcm_max_clique on scl_pcm_consistency's adj; degree may be NULL.
 *   * Errors, all SCL_ERR_INVALID_ARG, checked before anything runs, nothing written: a NULL engine; a negative count; n_loops or n > 4096;
 *     a required pointer NULL with a positive count; no output given with n > 0; an index out of range; a non-finite pose, z, entry of
 *     the upper triangle of a cov, odom_var or threshold; a negative odom_var or threshold; a quaternion with squared norm outside
 *     [0.25, 4]; for scl_pcm_max_clique an adj that is not symmetric, has a diagonal bit set, or a bit at or beyond n.  n == 0: SCL_OK,
 *     *n_members = 0, *seed = -1.
 *   * How it runs.  A pre-pass per loop and per keyframe (normalised quaternions, Z_i^-1, Ad(Z_i) Sigma_i Ad(Z_i)^T), one thread per pair
 *     of the upper triangle whose wave's ballot is a word of the graph, one wave per row for the lower triangle and the degrees, one wave
 *     per seed for the clique, a finishing launch.  Memory: a grow-only workspace (the n x n matrix only when d2 is asked for); a later,
 *     smaller call reads nothing an earlier one left.  On a scl_create_sharded engine the calls run on the primary shard, as
 *     scl_target_normals does.
 */
int  scl_pcm_consistency(scl_engine *e, const double *poses_a, int n_a, const double *poses_b, int n_b,
                         const int *idx_a, const int *idx_b, const double *z, const double *cov, int n_loops,
                         const double *odom_var, double threshold, double *d2, uint64_t *adj, int *degree);
int  scl_pcm_max_clique(scl_engine *e, const uint64_t *adj, int n, int *members, int *n_members, int *seed);
int  scl_pcm_select(scl_engine *e, const double *poses_a, int n_a, const double *poses_b, int n_b,
                    const int *idx_a, const int *idx_b, const double *z, const double *cov, int n_loops,
                    const double *odom_var, double threshold, int *members, int *n_members, int *seed, int *degree);
/* Device time of the last of the three calls above made while scl_profile_enable(e, 1) was in force, HIP events on the engine's stream:
 * pairs_ms = pre-pass + pair kernel + lower triangle and degrees, clique_ms = clique kernel + finishing launch; 0 for a stage that call
 * did not run.  Either pointer may be NULL. */
int  scl_pcm_last_timing(scl_engine *e, double *pairs_ms, double *clique_ms);
/* Host only, no engine: cov = s2 * info^-1 by a Cholesky factorisation in double -- the covariance a loop's factor gets from the
 * information matrix of its pairs (scl_registration_information, scl_registration_information_plane) and a variance of a pair's
 * residual.  A NULL pointer, a non-finite input, s2 <= 0, or an info whose factorisation fails -- a pivot that is not above 2^-43 of its
 * diagonal entry, which rounding can leave of a column that depends on the ones before it --: SCL_ERR_INVALID_ARG, nothing written.
 * That test also refuses a positive definite info whose condition number is beyond about 1e13 (a Schur complement below 2^-43 of its
 * diagonal entry); the tests cover condition numbers up to 1e8.  A corridor's singular point-to-plane matrix is such an input: the caller regularises it first
 * (adds a prior to its diagonal).  Only the upper triangle of info is read; cov is written symmetric. */
int  scl_loop_covariance(const double info[36], double s2, double cov[36]);

/*
 * POSE-GRAPH SOLVE: SE(3) BETWEEN FACTORS AND PRIORS, LEVENBERG-MARQUARDT WITH BLOCK PCG.  The step PCM stands in front of: the reference's
 * gtsamOpt (DM.h:782-901) -- prior and odometry BetweenFactor<Pose3> (668-699), one loop BetweenFactor<Pose3> per loop_info (798-803) --
 * and the estimates updatePoses (922-985) copies back into the key poses.  It reuses PCM's conventions, so that one set of arrays serves both.
 *   * Inputs.  poses: n_poses x 7 doubles, a pose is x, y, z and a quaternion x, y, z, w; the initial estimate, all robots' keyframes in
 *     one array.  Quaternions are normalised in double before use.  Between factors: f_i[k], f_j[k] index poses; f_z + 7 k = the measured
 *     X_i^-1 X_j (what scl_loop_pose_between writes, and what an odometry step is); f_cov + 36 k a row-major 6 x 6 covariance of the right
 *     perturbation Z Exp(xi), rotation first, of which only the upper triangle is read -- the array scl_pcm_* take.  Priors: p_idx[m], p_z
 *     + 7 m (a pose), p_cov + 36 m.  Factors are numbered between factors first, then priors: factor n_factors + m is prior m.
 *   * Residuals.  A between factor has E = Z^-1 X_i^-1 X_j, a prior E = Z^-1 X.  r = (Log_SO3(R_E), t_E) by PCM's rule: the quaternion of E
 *     with w made >= 0, 2 atan2(|v|, w) v / |v|, and 2 v where |v| = 0 (gtsam's default Pose3 chart).  X_i^-1 X_j and Z^-1 X take the
 *     difference of the two translations first, as PCM does: a trajectory 2 km from its origin costs nothing.
 *   * Information and cost.  cov = L L^T by Cholesky in double from the upper triangle (the operations of scl_loop_covariance, in its
 *     order); the whitened residual is y = L^-1 r and Omega = cov^-1 = L^-T L^-1 is never formed.  chi2[k] = y . y = r^T Omega r, between
 *     factors first and then priors; cost = 1/2 sum chi2.
 *   * Jacobians, with respect to right perturbations X Exp(xi), exact at xi = 0.  D(E) = blockdiag(Jr^-1(w), R_E) with w = Log_SO3(R_E);
 *     J_j = D(E); J_i = -D(E) Ad(h^-1) with h = X_i^-1 X_j and Ad(R, t) = [[R, 0], [[t]x R, R]] as in PCM; a prior has J = D(E).
 *     Jr^-1(w) = I + 1/2 [w]x + c(theta) [w]x^2, c = 1 / theta^2 - (1 + cos theta) / (2 theta sin theta), evaluated by the half angle the
 *     quaternion already holds: (1 + cos theta) / sin theta = q_w / |v| (no cancellation at theta -> pi).  Below theta < 0.05 the series
 *     c = 1/12 + theta^2 / 720 + theta^4 / 30240 + theta^6 / 1209600 is used (its next term is below 1e-18 there).
 *   * Linear system.  With A = L^-1 J the gradient is g = sum A^T y (6 per pose), H = sum A^T A (block sparse), and the damped system is
 *     (H + lambda diag(H)) delta = -g.  Retraction is gtsam's default: R <- R Exp_SO3(delta_w), t <- t + R delta_v; the quaternion of
 *     Exp_SO3(w) is (sin(theta / 2) / theta w, cos(theta / 2)), with sin(theta / 2) / theta = 1/2 - theta^2 / 48 below theta < 1e-4; the
 *     product is normalised again.
 *   * Levenberg-Marquardt.  lambda starts at lambda_initial.  An iteration is one damped solve at the kept poses and one evaluation of the
 *     cost at the retracted ones.  A step that lowers the cost (cost_new < cost) is accepted and lambda is divided by lambda_factor; one
 *     that does not is rejected: the poses are kept and lambda is multiplied by it.  After every iteration the solve stops on the first of
 *       1 SCL_PGO_STOP_COST        the step was accepted and cost - cost_new <= relative_cost_tolerance * cost
 *       2 SCL_PGO_STOP_STEP        the step's largest component |delta|_inf <= step_tolerance
 *       3 SCL_PGO_STOP_ITERATIONS  max_iterations iterations were made (accepted and rejected ones count alike)
 *       4 SCL_PGO_STOP_LAMBDA      lambda > lambda_max
 *     The linear solve is conjugate gradients from delta = 0, preconditioned with the 6 x 6 diagonal blocks of the damped matrix, each
 *     factored by Cholesky; it stops before the iteration at which sqrt(r^T M^-1 r) <= cg_tolerance * its initial value, or after
 *     cg_max_iterations.
 *   * Defaults (scl_pgo_default_params).  They are this project's own choice, not the reference's (whose optimiser is not in its tree):
 *     max_iterations 50, lambda_initial 1e-5, lambda_factor 10, lambda_max 1e10, relative_cost_tolerance 1e-10, step_tolerance 1e-10,
 *     cg_tolerance 1e-8, cg_max_iterations 500.  Only the two stop tolerances and the CG tolerance influence the answer.
 *   * Determinism.  The same inputs give the same bits on every run, and after a larger call has grown the workspace.  No floating-point
 *     atomics.  Every per-pose sum runs over the pose's incident factors in ascending factor number (between factors before priors): one
 *     after the other for a pose of fewer than 64 incident factors; for a longer row a wave takes it, lane l adds the entries l, l + 64,
 *     ... of the list in that order and the 64 lanes are summed by a fixed butterfly.  Every dot product is per pose, then a fixed tree
 *     over blocks of 256 poses, then a fixed tree over the blocks: a shape that depends on n_poses alone.
 *   * scl_pgo_linearize: cost, gradient (6 n_poses), diag (36 n_poses: the row-major diagonal blocks of H), chi2 (n_factors + n_priors)
 *     at `poses`; each may be NULL, one must be given.  scl_pgo_hessian_apply: y = (H + lambda diag(H)) x (6 n_poses each; lambda finite,
 *     >= 0): the operator the solver iterates, exposed so that it can be held to an assembled matrix.  scl_pgo_optimize: poses_out
 *     (n_poses x 7, unit quaternions with w >= 0; may alias poses), result, chi2 at poses_out (may be NULL; params == NULL: the defaults).
 *     scl_pgo_result: iterations, accepted, rejected, cg_iterations (the total), stop_reason, initial_cost, final_cost, final_lambda,
 *     gradient_max = |g|_inf at poses_out.
 *   * Errors, all SCL_ERR_INVALID_ARG, checked on the host before anything runs, nothing written: a NULL engine; a negative count; n_poses
 *     = 0 or > 1 048 576; n_factors > 4 194 304; n_priors > n_poses; a required pointer NULL with a positive count; no output given; an
 *     index out of range; f_i == f_j; a non-finite input; a quaternion with squared norm outside [0.25, 4]; a covariance whose
 *     factorisation meets a pivot that is not above 2^-43 of its diagonal entry (scl_loop_covariance's rule); a params field that is not
 *     finite and positive, or lambda_factor <= 1; a connected component of the graph without a prior (a union-find over the factors; the
 *     reference's disconnectedGraph test, DM.h:826-864, is the same idea) -- its answer would have a free gauge.
 *   * How it runs.  One thread per factor linearises (whitened residual, A_i^T y, A_j^T y, A_i^T A_i, A_j^T A_j and the one off-diagonal
 *     block W = A_i^T A_j, which pose i's row reads as it is and pose j's row transposed); one gather per pose over its list of incident
 *     (factor, side) entries -- built on the host by a stable counting sort -- assembles g, the diagonal block and the cost; PCG is two
 *     launches per iteration with alpha and beta formed on the device from per-block partial sums that every workgroup reduces again in the
 *     same order, and a device flag that turns the launches queued behind convergence into returns; the host reads one record per LM
 *     iteration and the flag once per 32 queued CG iterations.  Memory: a grow-only workspace; every word a call reads it wrote first.  On
 *     a scl_create_sharded engine the calls run on the primary shard, as the PCM calls do.  See DESIGN.md section 4, PGO.
 */
typedef struct scl_pgo_params {
    int    max_iterations;
    double lambda_initial, lambda_factor, lambda_max;
    double relative_cost_tolerance, step_tolerance;
    double cg_tolerance;
    int    cg_max_iterations;
} scl_pgo_params;
enum { SCL_PGO_STOP_COST = 1, SCL_PGO_STOP_STEP = 2, SCL_PGO_STOP_ITERATIONS = 3, SCL_PGO_STOP_LAMBDA = 4 };
typedef struct scl_pgo_result {
    int    iterations, accepted, rejected, cg_iterations, stop_reason;
    double initial_cost, final_cost, final_lambda, gradient_max;
} scl_pgo_result;
#define SCL_PGO_MAX_POSES   1048576
#define SCL_PGO_MAX_FACTORS 4194304
int  scl_pgo_default_params(scl_pgo_params *p);
int  scl_pgo_linearize(scl_engine *e, const double *poses, int n_poses,
                       const int *f_i, const int *f_j, const double *f_z, const double *f_cov, int n_factors,
                       const int *p_idx, const double *p_z, const double *p_cov, int n_priors,
                       double *cost, double *gradient, double *diag, double *chi2);
int  scl_pgo_hessian_apply(scl_engine *e, const double *poses, int n_poses,
                           const int *f_i, const int *f_j, const double *f_z, const double *f_cov, int n_factors,
                           const int *p_idx, const double *p_z, const double *p_cov, int n_priors,
                           double lambda, const double *x, double *y);
int  scl_pgo_optimize(scl_engine *e, const double *poses, int n_poses,
                      const int *f_i, const int *f_j, const double *f_z, const double *f_cov, int n_factors,
                      const int *p_idx, const double *p_z, const double *p_cov, int n_priors,
                      const scl_pgo_params *params, double *poses_out, scl_pgo_result *result, double *chi2);
/* Device time of the last of the three calls above made while scl_profile_enable(e, 1) was in force, HIP events on the engine's stream:
 * linearize_ms = every linearisation and assembly of the call, solve_ms = every PCG solve and retraction; 0 for a stage that call did not
 * run.  Either pointer may be NULL. */
int  scl_pgo_last_timing(scl_engine *e, double *linearize_ms, double *solve_ms);

/*
 * POSE-GRAPH SOLVE, CONDENSED DIRECT STEP.  A second linear solver for the LM loop above, exact up to rounding, for graphs that are
 * odometry chains plus some hundreds of loops -- where block-Jacobi PCG does not converge within its cap.  The calls above are unchanged.
 *   * Interior poses and junctions.  Pose k is interior when its list of incident factors holds exactly two entries, both between
 *     factors, one joining k with k - 1 and one joining k with k + 1 (either in either direction).  Every other pose is a junction: the ends
 *     of a robot's block, loop endpoints, poses with a prior, with a duplicate odometry factor, or whose odometry skips an index.  A
 *     segment is a maximal run a..b of interior poses; a - 1 and b + 1 exist and are junctions.  Two junctions may be adjacent.
 *   * The step solves (H + lambda diag H) delta = -g.  Every segment is eliminated by block cyclic reduction over the path [a - 1, a..b,
 *     b + 1], whose ends are never eliminated: a level eliminates every second node between the ends of what the level before left (of
 *     the survivors s_0 .. s_m-1 those at odd positions p < m - 1), so the order depends on the segment's length alone; a path of m
 *     nodes takes about log2 m levels (one loop-free chain of 100 000 poses: 17).  The 6 x 6 pivot block D of a node is factored by
 *     Cholesky, D = L L^T; with U_l, U_m the couplings (left neighbour, node) and (node, right neighbour), P = L^-1 U_l^T, Q = L^-1 U_m and
 *     w = L^-1 b, the left neighbour gets -P^T P and -P^T w, the right one -Q^T Q and -Q^T w, and their new coupling is -P^T Q.  A
 *     surviving node takes its left contribution, then its right.  What the levels leave on the ends, which start from zero, is the
 *     segment's Schur contribution: two diagonal updates, one coupling block and two right-hand-side updates.
 *   * The dense matrix S over the n_J junctions in ascending pose order (lower triangle) is assembled in a fixed order: a block's own
 *     damped diagonal block and the W blocks of the factors between the two junctions in ascending factor number, then the segments'
 *     contributions in ascending segment number (segments are numbered by their first pose); the right-hand side likewise.  S, padded
 *     with the identity to a multiple of 32, is factored by a blocked Cholesky in fp64 (panels of 32 columns: the diagonal block, the
 *     column below it, the trailing update on v_mfma_f64_16x16x4_f64), delta of the junctions is solved for, and the interior is recovered
 *     by walking the levels back: x = L^-T (w - P x_left - Q x_right).
 *   * Determinism.  No floating-point atomics; every sum has a fixed order.  The same inputs give the same bits on every run, and
 *     after a larger call has grown the workspace.
 *   * Limits.  At most SCL_PGO_MAX_JUNCTIONS junctions: S is then at most 6144^2 doubles (302 MB) of grow-only workspace.  More:
 *     SCL_ERR_INVALID_ARG, nothing written -- the caller keeps scl_pgo_optimize.  scl_pgo_count_junctions is host only and takes no
 *     engine; it answers that before a call (any output may be NULL; SCL_ERR_INVALID_ARG for a negative count, n_poses = 0, a NULL index
 *     array with a positive count or an index out of range).  longest_segment is in poses.
 *   * A failed pivot.  scl_loop_covariance's rule: a pivot fails when it is not above 2^-43 of its diagonal entry (of the block as
 *     factored in a segment; of S as assembled in the dense factorisation).  The failure is written to a word of the record the host
 *     reads once per LM iteration.  scl_pgo_optimize_condensed makes that iteration a rejected step: the poses are kept, lambda is
 *     multiplied by lambda_factor, *failed_factorisations (may be NULL) counts it, and of the stops only 3 and 4 are looked at.
 *     scl_pgo_solve_condensed returns SCL_ERR_NUMERIC with nothing written.
 *   * scl_pgo_solve_condensed: delta (6 n_poses), one step at `poses`; lambda finite and >= 0.  scl_pgo_optimize_condensed: the LM loop
 *     above with the same four stops, the same retraction and the trial evaluated by the next linearisation; cg_tolerance and
 *     cg_max_iterations are checked as above and otherwise ignored, result.cg_iterations is 0.  The errors of scl_pgo_hessian_apply and
 *     scl_pgo_optimize apply unchanged.  On a scl_create_sharded engine both run on the primary shard.  scl_pgo_last_timing reports the
 *     condensed solve under solve_ms; scl_pgo_condensed_last_timing splits it for the last timed condensed call: ms[0] elimination, [1]
 *     assembly of S, [2] factorisation, [3] the triangular solves and the way back, each summed over the call's steps.
 */
#define SCL_PGO_MAX_JUNCTIONS 1024
int  scl_pgo_count_junctions(int n_poses, const int *f_i, const int *f_j, int n_factors, const int *p_idx, int n_priors,
                             int *n_junctions, int *n_segments, int *longest_segment);
int  scl_pgo_solve_condensed(scl_engine *e, const double *poses, int n_poses,
                             const int *f_i, const int *f_j, const double *f_z, const double *f_cov, int n_factors,
                             const int *p_idx, const double *p_z, const double *p_cov, int n_priors,
                             double lambda, double *delta);
int  scl_pgo_optimize_condensed(scl_engine *e, const double *poses, int n_poses,
                                const int *f_i, const int *f_j, const double *f_z, const double *f_cov, int n_factors,
                                const int *p_idx, const double *p_z, const double *p_cov, int n_priors,
                                const scl_pgo_params *params, double *poses_out, scl_pgo_result *result, double *chi2,
                                int *failed_factorisations);
int  scl_pgo_condensed_last_timing(scl_engine *e, double ms[4]);

/*
 * POSE-GRAPH SOLVE, MANY RIGHT-HAND SIDES AND MARGINAL COVARIANCES.  The factorisation the condensed direct step makes -- L, P, Q of
 * every eliminated node and the blocked Cholesky factor of S -- used for many right-hand sides instead of one, and on top of that the
 * covariance of a pose and of one pose relative to another under the solved graph: what gtsam's Marginals gives the reference's users
 * (its optimiser takes useCovariance, DM.h:878-880), what gates a loop candidate by Mahalanobis distance, and the covariance of PCM's
 * T_A = (X_ai)^-1 X_aj that odom_var stands in for.  The calls above are unchanged: they keep their launches and their bits.
 *   * scl_pgo_solve_condensed_many solves (H + lambda diag H) x_c = rhs_c for c < n_rhs.  Column c occupies rhs + 6 n_poses c and x + 6
 *     n_poses c, laid out as delta is; x may alias rhs.  One linearisation at `poses`, one elimination and one factorisation of S per
 *     call: the kernels of scl_pgo_solve_condensed, fed the call's lambda.  Then every column runs the forward elimination over the
 *     levels (w = L^-1 b_m, -P^T w to the left neighbour, -Q^T w to the right one; a survivor takes left, then right), the junctions'
 *     right-hand side in the order of the step's, L Y = B and L^T X = Y on the factor of S, and the way back x = L^-T (w - P x_left - Q
 *     x_right).
 *   * The core rule.  A column's arithmetic is one fixed sequence that depends on the graph and on that column alone: not on n_rhs, not
 *     on the column's position, not on what the other columns hold, not on how columns are grouped into launches.  The same column
 *     gives the same bits alone, among 1 535 others, on every run, and after a larger call has grown the workspace.  (In the dense
 *     solves a workgroup owns 16 columns through all panels of 32: the diagonal block is solved per column, c ascending -- descending
 *     in the transposed sweep --, the rows below or above are updated by v_mfma_f64_16x16x4_f64, eight per panel in ascending k; a
 *     tile's missing columns are zeros, and no entry of the product reads another column.)  A column equal to -g need NOT reproduce
 *     scl_pgo_solve_condensed's bits -- the order inside the dense solves differs --, only its accuracy.
 *   * Column groups.  Columns run in groups whose per-column arrays -- 6 n_poses doubles of the column itself and 18 doubles per path
 *     node (b / w / x, the two slots) -- stay within 256 MB: group = 256 MB / that, at most 1536, from 16 on rounded down to a multiple
 *     of 16, never below 6.  One loop-free chain of 100 000 poses: 13 columns per group.  By the core rule the figure changes no bit.
 *   * scl_pgo_marginals works at lambda = 0, on the Gauss-Newton matrix H at `poses` -- the Laplace approximation gtsam's Marginals
 *     uses; call it on the optimiser's poses_out.  Sigma = H^-1 in the tangent of the right perturbations X_k Exp(xi_k), rotation first.
 *     The distinct poses named by q_i and q_j, in ascending order, give six unit columns each (at most SCL_PGO_MAX_MARGINAL_POSES
 *     distinct poses), solved as above.  blocks + 36 k: the row-major 6 x 6 block Sigma[q_i[k], q_j[k]], read from the rows of pose
 *     q_i[k] in the columns of pose q_j[k]; where q_i[k] == q_j[k] the upper triangle is read and mirrored, so the block is exactly
 *     symmetric.  rel + 36 k: the first-order covariance of the right perturbation of h = X_i^-1 X_j.  From h' = Exp(-xi_i) h Exp(xi_j) =
 *     h Exp(xi_j - Ad(h^-1) xi_i): rel = Sigma_jj - A Sigma_ij - (A Sigma_ij)^T + A Sigma_ii A^T with A = Ad(h^-1), Ad(R, t) = [[R, 0],
 *     [[t]x R, R]] as in PCM, h^-1 formed as the linearisation forms it (the translations' difference first); the four terms are added in
 *     the order written, every 6 x 6 product sums in ascending index, the upper triangle is computed and mirrored.  q_i[k] == q_j[k]: 36
 *     exact zeros.  Either output may be NULL; one must be given.
 *   * What rel costs in accuracy.  rel is a DIFFERENCE of terms of the size of Sigma_jj.  Each of them carries the solve's error, about
 *     2^-53 cond(H) relative to |Sigma_jj|, so wherever |Sigma_jj| >> |rel| -- two neighbouring poses at the far end of a long chain, far
 *     from its prior -- rel's own relative error is that figure times |Sigma_jj| / |rel|, and its smallest eigenvalues may come out
 *     negative.  Near the prior, or between poses whose marginals differ by as much as they measure, it is as good as blocks.
 *   * Errors, all SCL_ERR_INVALID_ARG, checked on the host before anything runs, nothing written: everything scl_pgo_solve_condensed
 *     refuses (more than SCL_PGO_MAX_JUNCTIONS junctions included); n_rhs < 1 or > SCL_PGO_MAX_RHS; n_queries < 1 or >
 *     SCL_PGO_MAX_MARGINAL_QUERIES; more than SCL_PGO_MAX_MARGINAL_POSES distinct query poses; a query index out of range; a NULL rhs,
 *     x, q_i or q_j; both outputs NULL; a non-finite rhs entry.  A failed pivot: SCL_ERR_NUMERIC, nothing written, as in the single step.
 *   * On a scl_create_sharded engine both calls run on the primary shard.  scl_pgo_condensed_last_timing reports them too: ms[0..2]
 *     keep their meaning, ms[3] spans the forward eliminations, triangular solves and ways back of all columns (in
 *     scl_pgo_solve_condensed_many the copies of the groups lie between them and count).  See DESIGN.md section 4, PGO marginals.
 */
#define SCL_PGO_MAX_RHS            1536   /* 6 x SCL_PGO_MAX_MARGINAL_POSES */
#define SCL_PGO_MAX_MARGINAL_POSES 256
#define SCL_PGO_MAX_MARGINAL_QUERIES 4096
int  scl_pgo_solve_condensed_many(scl_engine *e, const double *poses, int n_poses,
                                  const int *f_i, const int *f_j, const double *f_z, const double *f_cov, int n_factors,
                                  const int *p_idx, const double *p_z, const double *p_cov, int n_priors,
                                  double lambda, const double *rhs, int n_rhs, double *x);
int  scl_pgo_marginals(scl_engine *e, const double *poses, int n_poses,
                       const int *f_i, const int *f_j, const double *f_z, const double *f_cov, int n_factors,
                       const int *p_idx, const double *p_z, const double *p_cov, int n_priors,
                       const int *q_i, const int *q_j, int n_queries, double *blocks, double *rel);

/*
 * GLOBAL MAP: A PERSISTENT VOXEL MAP OF THE KEYFRAME STORE AT SOLVED POSES.  What the solved poses are for: publishGlobalMap, DM.h:1621-1655,
 * moves every keyframe cloud of keyFrameArray by its pose, concatenates them and runs a pcl::VoxelGrid of 0.4 m over the lot, again after
 * every optimisation.  Here the map stays on the device between calls, keyed by 63-bit voxel coordinates in a hash table, filled from the
 * on-device keyframe store (scl_keyframe_put) at fp64 poses; a keyframe whose pose moved is taken out at the old pose and put in at the new
 * one, and the map is then bit for bit the one a fresh build gives.  No other call of this header changes.
 *   * One map per engine; on a scl_create_sharded engine it lives on the primary shard, as the PCM and PGO calls do.
 *   * Pose: 7 doubles x, y, z, qx, qy, qz, qw -- the layout of poses_out --, normalised in double as the pose-graph kernels do
 *     (csrc/se3_device.hpp, normalise_pose).
 *   * World point: p_w = qrot(q, (double)p) + t, qrot's operation sequence (the same header), no contraction.
 *   * Leaf: a float, finite, > 0; inv = 1.0 / (double)leaf.
 *   * Voxel of a point, per axis: s = p_w * inv; c = floor(s) as an integer; f = (uint32)floor((s - floor(s)) * 2^20).  Both operations
 *     of f are exact in fp64 except for -1 < s < 0, where the difference s + 1 is rounded to nearest (by at most 2^-54: f moves only
 *     where the point lies on a 2^-20 boundary to that precision, and f = 2^20 for -2^-54 <= s < 0: the point counts at the upper face
 *     of voxel -1).  Either way f is one fixed sequence of IEEE operations.  A point is skipped, and counted in points_skipped, when a
 *     coordinate is not finite after the move or a c lies outside [-2^20, 2^20).
 *   * Key = (cz + 2^20) << 42 | (cy + 2^20) << 21 | (cx + 2^20).
 *   * State per voxel: four unsigned 64-bit integers, the count n and Sx, Sy, Sz = sum of f.  Integration adds, removal subtracts
 *     (integer atomic adds, of the two's complement for a removal; no floating-point atomics anywhere): the sums are exact, independent
 *     of order and exactly invertible.  A voxel whose n is back at 0 has zero sums and is not part of the map.
 *   * Centroid: x = (float)(((double)cx + (double)Sx / ((double)n * 1048576.0)) * (double)leaf), likewise y and z.  Its resolution is
 *     leaf * 2^-20, and the truncation in f biases it by at most that much towards the voxel's lower corner.  Fields beyond x, y, z are
 *     not carried: PCL averages intensity, an order-independent integer sum needs a bounded range, and intensity has none.
 *   * Output: 16-byte records x, y, z (float) and n as uint32, saturated at 2^32 - 1, in ascending key -- PCL's order, x fastest, on the
 *     global lattice.  The same bits on every run, whatever the table's capacity, growth history and the order of insertion.
 *   * scl_map_reset creates or empties the map.  scl_map_set_keyframes takes n poses (n x 7 doubles) for n keyframes of the store: one not
 *     in the map is added; one in the map at bitwise the same 7 doubles is left alone; one in the map at another pose is subtracted
 *     at the old pose and added at the new one.  scl_map_remove_keyframes subtracts.  scl_map_extract: box NULL or 6 doubles (lo x, y, z,
 *     hi x, y, z); a voxel is kept when its centroid in double -- before the narrowing -- lies in the closed box; out NULL gives the
 *     count alone; a capacity too small is an error that writes nothing.  scl_map_stats: see the struct.  scl_map_last_timing: ms[0]
 *     integrate (reserve and add passes), ms[1] grow, ms[2] extract of the last set / remove / extract made under scl_profile_enable(1).
 *   * Stale clouds.  The map remembers per integrated keyframe its pose and the generation of the stored cloud; scl_keyframe_put bumps
 *     the generation.  Setting or removing an integrated keyframe whose cloud was put again since answers SCL_ERR_INVALID_ARG -- its old
 *     points can no longer be subtracted: reset the map.
 *   * The table: open addressing, linear probing, 64-bit compare-and-swap on the key, 64 bytes per slot, at most half full; it starts at
 *     2^20 slots and doubles (the voxels are re-inserted, emptied ones dropped) whenever a launch group's keys do not fit; a group is
 *     first reserved (keys only: idempotent), then added, so a growth repeats nothing that counts.  At most 2^31 slots.
 *   * Errors, all SCL_ERR_INVALID_ARG, checked on the host before anything runs, nothing written: NULL engine; n < 0; a NULL pointer with
 *     n > 0; no map yet; a listed keyframe not in the store; a pose that is not finite; a quaternion's squared norm outside [0.25, 4]; a
 *     leaf that is not finite or not > 0; a keyframe listed twice in one call; removing a keyframe that is not in the map; a stale
 *     cloud; a NaN in the box.  See DESIGN.md section 4, Global map.
 */
struct scl_map_stats {
    uint64_t keyframes;         /* keyframes in the map */
    uint64_t points_added;      /* points in the voxels' counts, net of removals */
    uint64_t points_skipped;    /* points of the integrated keyframes that were skipped, net of removals */
    uint64_t occupied_voxels;   /* voxels with n > 0 */
    uint64_t capacity;          /* slots of the table */
    uint64_t growths;           /* growths since the reset */
};
int  scl_map_reset(scl_engine *e, float leaf);
int  scl_map_set_keyframes(scl_engine *e, const int *robots, const int *indices, const double *poses, int n);
int  scl_map_remove_keyframes(scl_engine *e, const int *robots, const int *indices, int n);
int  scl_map_extract(scl_engine *e, const double *box, void *out, int out_capacity, int *n_out);
int  scl_map_stats(scl_engine *e, struct scl_map_stats *out);
int  scl_map_last_timing(scl_engine *e, double ms[3]);

/* ---- measurement ----------------------------------------------------------- */
int  scl_profile_enable(scl_engine *e, int on);   /* 0 off, 1 every kernel family, 2 SC distance only,
                                                     3 SC distance only, sampled: one launch in thirteen -- in the stream form one
                                                     pair around every second chunk's launch groups, counted as that many launches
                                                     (an event keeps the launch behind it back by 4-6 us) */
int  scl_profile_reset(scl_engine *e);
int  scl_profile_get(scl_engine *e, scl_profile *out);
/* Counters of the ICP loop's LDS-tiled neighbour search (icp.hip K4c) since the last reset, in builds made with
 * -DSCL_DIAGNOSTICS (zeros otherwise): [0] rounds asked for, [1] rounds whose box did not fit, [2] lanes finished in memory,
 * [3] table entries staged, [4] points staged, [5] row visits, [6] points compared; [8..14] 10 ns ticks of every workgroup's
 * first thread per phase (up to the ball round, box, table, row scan, staging, the queries' walk, reduction).  Device-wide. */
void scl_debug_icp_tile_stats(unsigned long long out[16], int reset);
/* The full-database pass aligns every (scan, keyframe) pair (fastAlignUsingVkey, D.h:1491-1511) with an fp32 correlation
 * filter on the matrix cores and falls back to the reference's own fp64 evaluation wherever two shifts are closer than the
 * filter's error margin.  pairs = pairs aligned since the last reset, fallbacks = those decided by the fp64 evaluation (the
 * rate depends on the data: flat or periodic sector keys fall back).  Either pointer may be NULL; reset != 0 clears both. */
int  scl_alignment_stats(scl_engine *e, uint64_t *pairs, uint64_t *fallbacks, int reset);
/* The full-database pass scores exactly (fp64, D.h:1538-1569) only the keyframes whose screening bound reaches the smallest
 * bound of their scan (sc_screen.hip): queries = scans that went through an exact pass since the last reset, survivors = keyframes
 * scored exactly for them, max_survivors = the largest such count of one scan.  The rate of the pass depends on it: a database
 * where every keyframe survives runs at the exact kernel's rate.  On a sharded engine a scan counts once per shard.  Any
 * pointer may be NULL; reset != 0 clears the counters. */
int  scl_survivor_stats(scl_engine *e, uint64_t *queries, uint64_t *survivors, uint64_t *max_survivors, int reset);
int  scl_device_name(const scl_engine *e, char *buf, int buflen);
/* GB/s of `reps` copies of `bytes` from pinned host memory to the device, one after the other on the engine's copy stream (HIP events):
 * the link's rate, i.e. the floor of scl_stream_from_points per byte of point cloud. */
int  scl_host_copy_rate(scl_engine *e, size_t bytes, int reps, double *gbytes_per_s);
/* Self test of the device's float atan -- xy2theta (D.h:1352-1374) calls std::atan(float), here glibc's atanf restated in fp32
 * (csrc/device_common.hpp) --: checksums[b] = sum mod 2^64 over the 2^24 float bit patterns of block first_block + b of
 * splitmix64((bits << 32) | result bits), NaN results counted as 0x7fc00000.  tests/golden/atanf_blocks.json holds the 256 values
 * of libm's atanf (oracle/tools/atanf_exhaustive.c). */
int  scl_selftest_atanf_blocks(scl_engine *e, int first_block, int n_blocks, uint64_t *checksums);
/* Self test of the descriptor kernel's two ways to a point's (ring, sector, dropped?) -- the reference's chain (D.h:1425-1435) and the
 * cheap approximations that stand in for it wherever they are provably the same integers (csrc/device_common.hpp) -- on n_points
 * generated points of the engine's grid (mode 0: uniform; 1: on ring boundaries; 2: on sector boundaries; 3: zeros, denormals, huge,
 * inf, NaN): *sure = points the fast path answered, *disagreements = those of them where the chain says otherwise (must be 0). */
int  scl_selftest_bin_paths(scl_engine *e, int mode, uint64_t seed, uint64_t n_points, uint64_t *disagreements, uint64_t *sure);
/* ... and HOW FAR apart the two ways' quotients are where the fast one answers: the guard bands are four times a derived error on the
 * engine's grid, and this measures the error.  *disagreements and *sure as above; *max_ring_dev / *max_sector_dev = the largest
 * |q_fast - q_chain| over the sure points, q_chain = (double)sqrtf(x*x + y*y) / max_radius * num_ring resp. (double)xy2theta(x, y) /
 * 360 * num_sector as the chain forms them.  mode 0: uniform points; 1: either side of every ring boundary at guard * (1 + u)
 * quotient units, u in [0, 1) -- the sure points closest to a boundary --; 2: likewise at every sector boundary. */
int  scl_selftest_bin_margin(scl_engine *e, int mode, uint64_t seed, uint64_t n_points, uint64_t *disagreements, uint64_t *sure,
                             double *max_ring_dev, double *max_sector_dev);

/* Self test of the verification path's own stable radix sort (csrc/device_sort.hip; it replaced hipCUB's): the n (key, value) pairs
 * sorted on the key bits [0, bits), equal keys in their input order.  key_bytes 4 or 8; n_segments > 1 (8-byte keys): every segment
 * [segment_offsets[s], segment_offsets[s + 1]) sorted on its own, as the 26 submaps of a query are (DM.h:1183-1185 through PCL's VoxelGrid). */
int  scl_selftest_sort_pairs(scl_engine *e, int key_bytes, const void *keys, const uint32_t *values, int n, int bits, const int *segment_offsets,
                             int n_segments, void *keys_out, uint32_t *values_out);
/* ... and of its prefix sums (cell counts -> cell starts): out[i] = in[0] + ... + in[i - 1], + in[i] when inclusive != 0 */
int  scl_selftest_prefix_sum(scl_engine *e, const int32_t *in, int n, int inclusive, int32_t *out);
/* Self test of the batched voxel filter (csrc/voxel.hip, assemble_submaps_batch: the path of scl_loop_icp_batch_from_store, which
 * shows only the submaps' sizes): the submaps of n_jobs windows of `robot`'s stored keyframes -- job j = keyframes keys[j] -
 * search_nums[j] .. keys[j] + search_nums[j], each moved by its pose -- assembled and filtered in ONE batched call, copied back to
 * back into `out` (records of the store's stride), n_out[j] points of job j.  More than 64 jobs: SCL_ERR_INVALID_ARG. */
int  scl_selftest_submaps_batch(scl_engine *e, int robot, int n_jobs, const int *keys, const int *search_nums,
                                const float *poses /* the jobs' windows behind each other: sum(2*sn_j+1) matrices */,
                                float leaf, void *out, int out_capacity /* points, all jobs */, int *n_out /* n_jobs */);
/* Test hook of the global map: the starting capacity in slots of the NEXT scl_map_reset (rounded up to a power of two, at least 16; 0 =
 * the default of 2^20), so that growth and long probe chains are reached with a thousand points. */
int  scl_selftest_map_capacity(scl_engine *e, uint64_t slots);

#ifdef __cplusplus
}
#endif
#endif /* SCL_ENGINE_H */
