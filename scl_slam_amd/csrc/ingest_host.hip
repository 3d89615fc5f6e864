// ingest_host.hip -- host side of what FILLS the keyframe database (kernels: make_sc.hip): the database's arrays (allocated, copied and
// freed over the one table of db_arrays.hpp), the append paths with their C entry points -- one cloud, one filtered cloud, wire
// descriptors in bulk, the staged query --, the two points pipelines (clouds from the host in groups of 16 behind a copy stream; clouds
// of the keyframe store) and the calls built on them, the pinned host buffers, the bulk read-back with the database's dump and load, and
// the sharded front's hooks into all of this.  No kernel lives here.  The engine object, its locks and what this file shares with
// engine.hip are engine_internal.hpp's; how a group of clouds travels -- one merged copy or one copy per cloud -- is ingest_plan.hpp's,
// a pure function that tests/cpp/ingest_plan_check.cpp checks without a GPU, as it checks the table.
#include "scl_engine.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "db_file.hpp"
#include "engine_internal.hpp"
#include "ingest_plan.hpp"
#include "plugin_host.hpp"

using namespace scl;

static_assert(kPlanCopyGroup == kMaxScBatch, "a group of the copy plan is a batch of the scatter");

namespace {

DbShape db_shape(const scl_engine *e)
{
    return DbShape{(size_t)e->RG * e->S, (size_t)e->S, (size_t)e->R4, (size_t)e->hstride, 8, (size_t)e->hkw, (size_t)halign_bytes(e->S), (size_t)e->RG};
}

// a fresh set for `ncap` slots and the engine's staging rows; what was allocated is freed when a later allocation fails
int db_arrays_alloc(scl_engine *e, int ncap, DbArrays *out)
{
    const DbShape sh = db_shape(e);
    DbArrays a;
    for (int id = 0; id < kDbArrayCount; ++id) {
        if (!db_array_present(kDbArrays[id], sh)) continue;
        unsigned char *p = nullptr;
        const int rc = dev_alloc(e, &p, db_array_bytes(kDbArrays[id], sh, (size_t)ncap, (size_t)e->stage_rows));
        if (rc) { db_arrays_free(a); return rc; }
        a.set(id, p);
    }
    *out = a;
    return SCL_OK;
}

// Rows [s, s + m) of `from` (arrays of from_cap slots) -> rows [d, d + m) of `to` (of to_cap slots), ordered on e's stream; consecutive
// rows are consecutive in every slot-major array: one copy per array.  peer: `from` belongs to that engine (another device, or e
// itself).  to_stage: the destination is staging rows, and the arrays that have none are left out.
int db_arrays_copy_rows(scl_engine *e, const DbArrays &to, size_t to_cap, size_t d, const DbArrays &from, size_t from_cap, size_t s, size_t m,
                        bool to_stage, const scl_engine *peer)
{
    const DbShape sh = db_shape(e);
    for (int id = 0; id < kDbArrayCount; ++id) {
        const DbArrayInfo &t = kDbArrays[id];
        if (!db_array_present(t, sh) || (to_stage && !t.staged)) continue;
        unsigned char *dst = static_cast<unsigned char *>(to.at(id)) + db_row_offset(t, sh, d);
        const unsigned char *src = static_cast<const unsigned char *>(from.at(id)) + db_row_offset(t, sh, s);
        if (!t.slot_major)
            SCL_HIP(e, hipMemcpy2DAsync(dst, t.elem_bytes * to_cap, src, t.elem_bytes * from_cap, t.elem_bytes * m, sh.*t.width, hipMemcpyDeviceToDevice, e->stream));
        else if (peer)
            SCL_HIP(e, hipMemcpyPeerAsync(dst, e->device, src, peer->device, db_row_bytes(t, sh) * m, e->stream));
        else
            SCL_HIP(e, hipMemcpyAsync(dst, src, db_row_bytes(t, sh) * m, hipMemcpyDeviceToDevice, e->stream));
    }
    return SCL_OK;
}

// ensure_capacity's copies into the fresh set, and its waits
int db_arrays_move_into(scl_engine *e, const DbArrays &fresh, int ncap)
{
    int rc;
    SCL_HIP(e, hipMemsetAsync(fresh.at(kDbRkey4), 0, db_array_bytes(kDbArrays[kDbRkey4], db_shape(e), (size_t)ncap, 0), e->stream));
    if (e->n > 0 && (rc = db_arrays_copy_rows(e, fresh, (size_t)ncap, 0, e->db, (size_t)e->cap, 0, (size_t)e->n, false, nullptr))) return rc;
    if (e->cap > 0 &&                                      // staged queries move with the arrays
        (rc = db_arrays_copy_rows(e, fresh, (size_t)ncap, (size_t)ncap, e->db, (size_t)e->cap, (size_t)e->cap, (size_t)e->stage_rows, true, nullptr)))
        return rc;
    SCL_HIP(e, hipStreamSynchronize(e->stream));
    // passes still reading the old arrays: the exact pass of a stream's chunk on the side stream, the ring-key scan, the alternate lane
    // (an append may now run between the chunks of a stream call: stream_screened_locked)
    for (hipStream_t s2 : {e->stream_alt, e->stream_surv, e->stream2})
        if (s2) SCL_HIP(e, hipStreamSynchronize(s2));
    return SCL_OK;
}

}  // namespace

namespace scl {

void db_arrays_free(DbArrays &a)
{
    for (int id = 0; id < kDbArrayCount; ++id) {
        if (a.at(id)) (void)hipFree(a.at(id));
        a.set(id, nullptr);
    }
}

// grow the database to hold at least `need` slots (geometric growth, D2D copies)
int ensure_capacity(scl_engine *e, int need)
{
    if (need <= e->cap) return SCL_OK;
    int ncap = e->cap > 0 ? e->cap : (e->cfg.initial_capacity > 0 ? e->cfg.initial_capacity : 4096);
    while (ncap < need) ncap *= 2;
    DbArrays fresh;
    int rc = db_arrays_alloc(e, ncap, &fresh);
    if (rc) return rc;
    if ((rc = db_arrays_move_into(e, fresh, ncap))) {       // the database stays as it was
        drain_keeping_error(e, {e->stream});
        db_arrays_free(fresh);
        return rc;
    }
    db_arrays_free(e->db);
    e->db = fresh;
    e->cap = ncap;
    return SCL_OK;
}

int ensure_vals(scl_engine *e, size_t floats)
{
    if (floats <= e->vals_cap) return SCL_OK;
    dev_free(e->d_vals);
    int rc = dev_alloc(e, &e->d_vals, floats);
    if (rc) { e->vals_cap = 0; return rc; }
    e->vals_cap = floats;
    return SCL_OK;
}

static int ensure_points(scl_engine *e, size_t bytes)       // (this file's, and eng_ensure_points')
{
    if (bytes <= e->points_cap) return SCL_OK;
    dev_free(e->d_points);
    size_t nb = bytes + bytes / 4 + 4096;
    int rc = dev_alloc(e, &e->d_points, nb);
    if (rc) { e->points_cap = 0; return rc; }
    e->points_cap = nb;
    return SCL_OK;
}

}  // namespace scl

namespace {

// ingest `count` wire descriptors already in e->d_vals into slots [first, first+count)
int ingest_from_vals(scl_engine *e, int count, int first_slot)
{
    ProfScope ps(e, P_INGEST);
    SCL_HIP(e, launch_ingest(ingest_args(e, first_slot, e->d_vals, nullptr, nullptr, false), count, e->stream));
    e->db_version++;                                       // the second lane (stream_alt) orders itself behind this write
    return SCL_OK;
}

// the (robot, index) of `count` keyframes whose slots have been written, and the database's size; nullptr: robot 0, index = the slot
int append_meta(scl_engine *e, int count, const int8_t *robots, const int *indexs)
{
    for (int i = 0; i < count; ++i) {
        e->robots.push_back(robots ? robots[i] : (int8_t)0);
        e->indexs.push_back(indexs ? indexs[i] : e->n + i);
    }
    e->n += count;
    return SCL_OK;
}

// the batch scatter's tiles (make_sc.hip): kMaxScBatch polar images in their initial state between calls
int ensure_tiles(scl_engine *e, hipStream_t s)
{
    int rc;
    if (!e->d_tiles) {
        if ((rc = dev_alloc(e, &e->d_tiles, (size_t)2 * kMaxScBatch * e->R * e->S))) return rc;   // two sets: the resident path scatters group g + 1 beside the ingest of group g
        e->tiles_clean = false;
    }
    if (!e->tiles_clean) {                                   // first use, or a call that failed between scatter and consumer
        SCL_HIP(e, launch_make_sc_tiles_init(e->d_tiles, 2 * kMaxScBatch, e->R, e->S, s));
        e->tiles_clean = true;
    }
    return SCL_OK;
}

int check_cloud(scl_engine *e, const void *points, int n_points, int stride_bytes)
{
    if (n_points < 0 || stride_bytes < 12 || (stride_bytes & 3)) return fail(e, SCL_ERR_INVALID_ARG, "bad point layout");
    if (n_points > 0 && !points) return fail(e, SCL_ERR_INVALID_ARG, "null points");
    return SCL_OK;
}

// K3 for up to kMaxScBatch clouds ALREADY ON THE DEVICE (dptr[i], n[i] points of `stride` bytes): one scatter launch over all of
// them into the tiles.  What consumes the tiles follows: group_ingest (append) or group_values (descriptor only).
int group_scatter(scl_engine *e, const unsigned char *const *dptr, const int *n, int count, int stride, hipStream_t s)
{
    int rc;
    if (count < 1 || count > kMaxScBatch) return fail(e, SCL_ERR_INVALID_ARG, "batch of 1..16 scans");
    if ((rc = ensure_tiles(e, s))) return rc;
    if ((rc = ensure_vals(e, (size_t)e->R * e->S * (size_t)kMaxScBatch))) return rc;
    ScanBatch b{};
    b.count = count;
    uint64_t pts = 0;
    for (int i = 0; i < count; ++i) { b.points[i] = dptr[i]; b.n[i] = n[i]; pts += (uint64_t)n[i]; }
    e->tiles_clean = false;
    ProfScope ps(e, P_MAKESC, s);
    // points of a cloud per workgroup: a workgroup's private tile is merged with up to R*S atomics, so the slice grows with the grid
    // (measured, 16 clouds: 64x120 best at 4 096 of 3 072..16 384; 80x180 at 8 192: 47 us against 60 at 4 096)
    const int slice = e->R * e->S > 10000 ? 2 * kScPointsPerWorkgroup : kScPointsPerWorkgroup;
    SCL_HIP(e, launch_make_sc_batch(b, stride, e->R, e->S, e->cfg.lidar_height, e->cfg.max_radius, e->d_tiles,
                                    scl_lab_int("SCL_SC_SLICE", slice), e->num_cu, s));
    e->prof.make_sc_points += e->prof_on ? pts : 0;
    return SCL_OK;
}

// ... tiles -> database slots [first_slot, first_slot + count) (every array of the slot) + wire-format values in e->d_vals; the tiles
// are initial again afterwards
int group_ingest(scl_engine *e, int count, int first_slot, hipStream_t s)
{
    ProfScope ps(e, P_INGEST, s);
    SCL_HIP(e, launch_ingest(ingest_args(e, first_slot, nullptr, e->d_tiles, e->d_vals, false), count, s));
    e->tiles_clean = true;
    e->db_version++;                                       // the second lane (stream_alt) orders itself behind this write
    return SCL_OK;
}

// ... tiles -> wire-format values in e->d_vals only (nothing is stored)
int group_values(scl_engine *e, int count, hipStream_t s)
{
    SCL_HIP(e, launch_make_sc_finalize(e->d_tiles, count, e->R, e->S, e->d_vals, s));
    e->tiles_clean = true;
    return SCL_OK;
}

// one cloud from the host into e->d_points, then the scatter
int scatter_host_cloud(scl_engine *e, const void *points, int n_points, int stride_bytes)
{
    int rc;
    if ((rc = check_cloud(e, points, n_points, stride_bytes))) return rc;
    const size_t bytes = (size_t)n_points * (size_t)stride_bytes;
    if ((rc = ensure_points(e, bytes + 16))) return rc;
    if (bytes) SCL_HIP(e, hipMemcpyAsync(e->d_points, points, bytes, hipMemcpyHostToDevice, e->stream));
    const unsigned char *dp = e->d_points;
    return group_scatter(e, &dp, &n_points, 1, stride_bytes, e->stream);
}

// The end of both make_and_save forms, behind the scatter of the one cloud: its tiles -> slot n, the values to the caller, the wait
// (`wait`: sync_short for a call of tens of microseconds of device time -- polled, not slept on --, sync otherwise), the keyframe counted
int save_scattered_cloud(scl_engine *e, int8_t robot, int index, float *out_values, int (*wait)(scl_engine *))
{
    int rc;
    if ((rc = group_ingest(e, 1, e->n, e->stream))) return rc;
    if (out_values)
        SCL_HIP(e, hipMemcpyAsync(out_values, e->d_vals, sizeof(float) * (size_t)e->R * e->S,
                                  hipMemcpyDeviceToHost, e->stream));
    if ((rc = wait(e))) return rc;
    return append_meta(e, 1, &robot, &index);
}

// wire descriptor -> staging row j (database index cap + j); a staged row has no tiled ring key and no alignment image
int stage_values_locked(scl_engine *e, int j, const float *values)
{
    int rc;
    const size_t cells = (size_t)e->R * e->S;
    if ((rc = ensure_vals(e, cells))) return rc;
    SCL_HIP(e, hipMemcpyAsync(e->d_vals, values, sizeof(float) * cells, hipMemcpyHostToDevice, e->stream));
    {
        ProfScope ps(e, P_INGEST);
        SCL_HIP(e, launch_ingest(ingest_args(e, e->cap + j, e->d_vals, nullptr, nullptr, true), 1, e->stream));
    }
    if ((rc = sync(e))) return rc;
    e->staged[j] = true;
    return SCL_OK;
}

}  // namespace

extern "C" {

int scl_make_and_save(scl_engine *e, const void *points, int n_points, int stride_bytes,
                      int8_t robot, int index, float *out_values)
{
    if (!e) return SCL_ERR_INVALID_ARG;
    if (e->front) return front_make_and_save(e, points, n_points, stride_bytes, robot, index, out_values, false, 0.f, nullptr);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    int rc;
    if ((rc = ensure_capacity(e, e->n + 1))) return rc;
    if ((rc = scatter_host_cloud(e, points, n_points, stride_bytes))) return rc;
    return save_scattered_cloud(e, robot, index, out_values, sync_short);
}

int scl_make_and_save_filtered(scl_engine *e, const void *points, int n_points, int stride_bytes, float leaf,
                               int8_t robot, int index, float *out_values, int *n_filtered)
{
    if (!e) return SCL_ERR_INVALID_ARG;
    if (e->front) return front_make_and_save(e, points, n_points, stride_bytes, robot, index, out_values, true, leaf, n_filtered);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    int rc;
    if ((rc = check_cloud(e, points, n_points, stride_bytes))) return rc;
    if ((rc = ensure_capacity(e, e->n + 1))) return rc;
    // makeDescriptors, DM.h:996-1002: VoxelGrid(descriptLeafSize) then makeAndSaveDescriptorAndKey -- the filtered cloud
    // never leaves the device
    std::string err;
    const void *d_cloud = nullptr;
    int m = 0;
    if ((rc = voxel_grid_to_device(&e->vox_ws, e->stream, points, n_points, stride_bytes, leaf, &d_cloud, &m, &err))) { e->last_error = err; return rc; }
    const unsigned char *dp = static_cast<const unsigned char *>(d_cloud);
    if ((rc = group_scatter(e, &dp, &m, 1, stride_bytes, e->stream))) return rc;
    if ((rc = save_scattered_cloud(e, robot, index, out_values, scl::sync))) return rc;
    if (n_filtered) *n_filtered = m;
    return SCL_OK;
}

int scl_make_descriptor(scl_engine *e, const void *points, int n_points, int stride_bytes, float *out_values)
{
    if (!e || !out_values) return SCL_ERR_INVALID_ARG;
    if (e->front) e = front_primary(e);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    int rc;
    if ((rc = scatter_host_cloud(e, points, n_points, stride_bytes))) return rc;
    if ((rc = group_values(e, 1, e->stream))) return rc;
    SCL_HIP(e, hipMemcpyAsync(out_values, e->d_vals, sizeof(float) * (size_t)e->R * e->S,
                              hipMemcpyDeviceToHost, e->stream));
    return sync(e);
}

int scl_save_from_wire(scl_engine *e, const float *values, int8_t robot, int index)
{
    return scl_save_bulk(e, values, 1, &robot, &index);
}

int scl_save_bulk(scl_engine *e, const float *values, int count, const int8_t *robots, const int *indexs)
{
    if (!e || count < 0 || (count > 0 && !values)) return SCL_ERR_INVALID_ARG;
    if (e->front) return front_save_bulk(e, values, count, robots, indexs);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    int rc;
    if ((rc = ensure_capacity(e, e->n + count))) return rc;
    const size_t cells = (size_t)e->R * e->S;
    const int chunk = 2048;
    if ((rc = ensure_vals(e, cells * (size_t)(count < chunk ? count : chunk)))) return rc;
    for (int done = 0; done < count; done += chunk) {
        const int c = count - done < chunk ? count - done : chunk;
        SCL_HIP(e, hipMemcpyAsync(e->d_vals, values + (size_t)done * cells, sizeof(float) * cells * c,
                                  hipMemcpyHostToDevice, e->stream));
        if ((rc = ingest_from_vals(e, c, e->n + done))) return rc;
        if ((rc = sync(e))) return rc;     // d_vals is reused by the next chunk
    }
    return append_meta(e, count, robots, indexs);
}

int scl_stage_query(scl_engine *e, const float *values)
{
    if (!e || !values) return SCL_ERR_INVALID_ARG;
    if (e->front) return front_stage_query(e, values);
    std::lock_guard<std::mutex> pk(e->pass_mu);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    return stage_values_locked(e, 0, values);               // (staging row 0: the public one)
}

}  // extern "C"

namespace {

constexpr int kDefaultCopyStreams = 2;

// The per-incoming-scan pipeline from raw points (DM.h:988-1025 makeDescriptors once per keyframe, then DM.h:1078 detection):
// the scans go through in GROUPS of up to kMaxScBatch.  A group's clouds are copied into one of three device buffers on the copy
// stream -- by DMA when the caller's buffers are pinned (scl_host_alloc / scl_host_register) -- while the group before is binned (one
// scatter launch), ingested (one launch: every array of its database slots), and, `detect`, searched for over the whole database
// ([0, key - NUM_EXCLUDE_RECENT), D.h:1627) by the stream form's launch group.  PCIe is the floor of this path (n x stride bytes per
// scan against ~10 us of kernels), so the only thing that matters is that the copy engine never waits: group g + 1's copy is
// enqueued before group g's kernels, and the host blocks only on group g's results.
// pass_mu (detect) and `db` = e->mu are held by the caller; the database lock is given up while a group's detection waits.
int points_pipeline_locked(scl_engine *e, std::unique_lock<std::mutex> &db, const void *const *clouds, const int *n_points, int n_scans,
                           int stride_bytes, const int8_t *robots, const int *indexs, float *out_values,
                           bool detect, int *nn_idx, int *shift, double *dist)
{
    int rc;
    for (int i = 0; i < n_scans; ++i)
        if ((rc = check_cloud(e, clouds[i], n_points[i], stride_bytes))) return rc;
    if (n_scans == 0) return SCL_OK;
    constexpr int G = kMaxScBatch;
    const int ng = (n_scans + G - 1) / G;
    const size_t cells = (size_t)e->R * e->S;
    // how every group travels and where its clouds lie in a buffer (ingest_plan.hpp), decided once; the largest group sizes the three buffers
    std::vector<uintptr_t> addr((size_t)n_scans);
    for (int i = 0; i < n_scans; ++i) addr[(size_t)i] = reinterpret_cast<uintptr_t>(clouds[i]);
    std::vector<GroupCopyPlan> plans((size_t)ng);
    size_t need = 0;
    for (int g = 0; g < ng; ++g) {
        plans[(size_t)g] = plan_group_copy(addr.data(), n_points, stride_bytes, g * G, std::min((g + 1) * G, n_scans));
        need = std::max(need, plans[(size_t)g].span);
    }
    const int nbuf = ng < 3 ? ng : 3;
    if (!e->stream_copy) SCL_HIP(e, hipStreamCreateWithFlags(&e->stream_copy, hipStreamNonBlocking));
    // several copy streams: a cloud is one copy of a megabyte or two, and the copies of ONE stream run strictly one after the other,
    // each with its own start-up (17 us: 44.8 GB/s for cloud-sized copies against 56.8 for one large copy); with the clouds of a group
    // dealt over several streams another copy is in flight while one is being set up
    const int ncs = std::min(std::max(scl_lab_int("SCL_COPY_STREAMS", kDefaultCopyStreams), 1), (int)scl_engine::kCopyStreams);
    auto cstream = [&](int c) { return c == 0 ? e->stream_copy : e->stream_copy_x[c - 1]; };
    for (int c = 1; c < ncs; ++c)
        if (!e->stream_copy_x[c - 1]) SCL_HIP(e, hipStreamCreateWithFlags(&e->stream_copy_x[c - 1], hipStreamNonBlocking));
    for (int b = 0; b < 3; ++b) {
        for (int c = 0; c < ncs; ++c)
            if (!e->ev_copied[c][b]) SCL_HIP(e, hipEventCreateWithFlags(&e->ev_copied[c][b], hipEventDisableTiming));
        if (!e->ev_consumed[b]) SCL_HIP(e, hipEventCreateWithFlags(&e->ev_consumed[b], hipEventDisableTiming));
    }
    if (need > e->pbuf_cap || !e->d_pbuf[nbuf - 1]) {      // (nothing of an earlier call is in flight: every call ends with its last group consumed)
        const size_t nb = need > e->pbuf_cap ? need + need / 4 + 4096 : e->pbuf_cap;
        for (int b = 0; b < 3; ++b) {
            if (need > e->pbuf_cap) { dev_free(e->d_pbuf[b]); e->d_pbuf[b] = nullptr; }
            if (b < nbuf && !e->d_pbuf[b] && (rc = dev_alloc(e, &e->d_pbuf[b], nb))) { e->pbuf_cap = 0; return rc; }
        }
        e->pbuf_cap = nb;
    }
    if ((rc = ensure_capacity(e, e->n + n_scans))) return rc;     // the slots of every scan of the call: no regrow between groups

    auto enqueue_copy = [&](int g) -> int {
        const int b = g % 3;
        const GroupCopyPlan &p = plans[(size_t)g];
        if (g >= 3)                                          // the group that was binned out of this buffer
            for (int c = 0; c < ncs; ++c) SCL_HIP(e, hipStreamWaitEvent(cstream(c), e->ev_consumed[b], 0));
        if (p.merged) SCL_HIP(e, hipMemcpyAsync(e->d_pbuf[b], clouds[g * G], p.span - 16, hipMemcpyHostToDevice, cstream(0)));
        else for (int i = g * G; i < n_scans && i < (g + 1) * G; ++i) {
            const size_t bytes = (size_t)n_points[i] * (size_t)stride_bytes;
            if (bytes) SCL_HIP(e, hipMemcpyAsync(e->d_pbuf[b] + p.off[i - g * G], clouds[i], bytes, hipMemcpyHostToDevice, cstream(i % ncs)));
        }
        for (int c = 0; c < ncs; ++c) SCL_HIP(e, hipEventRecord(e->ev_copied[c][b], cstream(c)));
        return SCL_OK;
    };
    // error path: nothing may still read the caller's buffers or write the point buffers when the call returns
    auto bail = [&](int code) {
        hipStream_t busy[scl_engine::kCopyStreams + 1];
        for (int c = 0; c < ncs; ++c) busy[c] = cstream(c);
        busy[ncs] = e->stream;
        drain_keeping_error(e, busy, ncs + 1);
        return code;
    };

    if ((rc = enqueue_copy(0))) return bail(rc);
    for (int g = 0; g < ng; ++g) {
        if (g + 1 < ng && (rc = enqueue_copy(g + 1))) return bail(rc);
        const int b = g % 3, i0 = g * G, m = n_scans - i0 < G ? n_scans - i0 : G;
        const unsigned char *dptr[G];
        for (int j = 0; j < m; ++j) dptr[j] = e->d_pbuf[b] + plans[(size_t)g].off[j];
        for (int c = 0; c < ncs; ++c)
            if (hipStreamWaitEvent(e->stream, e->ev_copied[c][b], 0) != hipSuccess) return bail(fail(e, SCL_ERR_HIP, "hipStreamWaitEvent(copied)"));
        if ((rc = group_scatter(e, dptr, n_points + i0, m, stride_bytes, e->stream))) return bail(rc);
        if (hipEventRecord(e->ev_consumed[b], e->stream) != hipSuccess) return bail(fail(e, SCL_ERR_HIP, "hipEventRecord(consumed)"));
        if ((rc = ensure_capacity(e, e->n + m))) return bail(rc);   // (no-op unless another thread appended while a group's detection waited)
        const int first_slot = e->n;
        if ((rc = group_ingest(e, m, first_slot, e->stream))) return bail(rc);
        if (out_values && hipMemcpyAsync(out_values + (size_t)i0 * cells, e->d_vals, sizeof(float) * cells * (size_t)m, hipMemcpyDeviceToHost, e->stream) != hipSuccess)
            return bail(fail(e, SCL_ERR_HIP, "descriptor values to the host"));
        append_meta(e, m, robots ? robots + i0 : nullptr, indexs ? indexs + i0 : nullptr);   // (stream order: whatever scores these slots is enqueued behind their ingest)
        if (detect) {
            int q[G], lo[G], hi[G];
            for (int j = 0; j < m; ++j) { q[j] = first_slot + j; lo[j] = 0; hi[j] = detect_range_hi(e, q[j]); }
            if ((rc = detect_full_stream_locked(e, db, q, lo, hi, m, G, 2, nn_idx + i0, shift + i0, dist + i0))) return bail(rc);
            if (!db.owns_lock()) db.lock();
        } else if (g + 1 == ng || out_values) {
            if ((rc = sync(e))) return bail(rc);            // (d_vals is rewritten by the next group)
        }
    }
    if ((rc = sync(e))) return bail(rc);
    return SCL_OK;
}

// The same path for clouds that are ALREADY on the device (the keyframe store): with no copy to hide, the groups' two launches go
// back to back on the stream (16 scans each), and the detection of all the new keyframes is ONE call of the stream form -- whose
// launch groups overlap (a group's finishing rides beside the next group's alignment), which separate calls per group of 16 cannot.
int device_points_pipeline_locked(scl_engine *e, std::unique_lock<std::mutex> &db, const unsigned char *const *d_clouds, const int *n_points,
                                  int n_scans, int stride_bytes, const int8_t *robots, const int *indexs, float *out_values,
                                  int *nn_idx, int *shift, double *dist)
{
    int rc;
    if (n_scans == 0) return SCL_OK;
    constexpr int G = kMaxScBatch;
    const size_t cells = (size_t)e->R * e->S;
    if ((rc = ensure_capacity(e, e->n + n_scans))) return rc;
    const int first_key = e->n;
    if ((rc = ensure_tiles(e, e->stream))) return rc;
    if ((rc = ensure_vals(e, cells * (size_t)(2 * G)))) return rc;
    for (int i = 0; i < n_scans; ++i)
        if (n_points[i] < 0 || (n_points[i] > 0 && !d_clouds[i])) return fail(e, SCL_ERR_INVALID_ARG, "stored cloud without points");
    // launch g = [ingest of group g - 1 out of tile set (g - 1) & 1] + [scatter of group g into tile set g & 1]: ng + 1 launches back to back
    const int ng = (n_scans + G - 1) / G;
    const int slice = scl_lab_int("SCL_SC_SLICE", e->R * e->S > 10000 ? 2 * kScPointsPerWorkgroup : kScPointsPerWorkgroup);
    e->tiles_clean = false;
    for (int g = 0; g <= ng; ++g) {
        ScanBatch b{};
        if (g < ng) {
            const int i0 = g * G;
            b.count = n_scans - i0 < G ? n_scans - i0 : G;
            for (int j = 0; j < b.count; ++j) { b.points[j] = d_clouds[i0 + j]; b.n[j] = n_points[i0 + j]; }
        }
        IngestArgs ia{};
        int n_ingest = 0;
        ia.R = e->R; ia.S = e->S;
        if (g > 0) {
            const int i0 = (g - 1) * G;
            n_ingest = n_scans - i0 < G ? n_scans - i0 : G;
            ia = ingest_args(e, first_key + i0, nullptr, e->d_tiles + (size_t)((g - 1) & 1) * G * cells, e->d_vals + (size_t)((g - 1) & 1) * G * cells, false);
        }
        {
            ProfScope ps(e, P_MAKESC);
            SCL_HIP(e, launch_front_fused(b, stride_bytes, e->cfg.lidar_height, e->cfg.max_radius, e->d_tiles + (size_t)(g & 1) * G * cells, slice, ia, n_ingest, e->stream));
        }
        if (g > 0 && out_values) {
            const int i0 = (g - 1) * G;
            SCL_HIP(e, hipMemcpyAsync(out_values + (size_t)i0 * cells, e->d_vals + (size_t)((g - 1) & 1) * G * cells, sizeof(float) * cells * (size_t)n_ingest,
                                      hipMemcpyDeviceToHost, e->stream));
        }
    }
    e->tiles_clean = true;
    e->db_version++;
    e->prof.make_sc_points += e->prof_on ? [&] { uint64_t t = 0; for (int i = 0; i < n_scans; ++i) t += (uint64_t)n_points[i]; return t; }() : 0;
    append_meta(e, n_scans, robots, indexs);
    std::vector<int> q((size_t)n_scans), lo((size_t)n_scans, 0), hi((size_t)n_scans);
    for (int i = 0; i < n_scans; ++i) { q[(size_t)i] = first_key + i; hi[(size_t)i] = detect_range_hi(e, first_key + i); }
    if ((rc = detect_full_stream_locked(e, db, q.data(), lo.data(), hi.data(), n_scans, G, 2, nn_idx, shift, dist))) return rc;
    if (!db.owns_lock()) db.lock();
    return sync(e);
}

}  // namespace

extern "C" {

/* makeDescriptors + full-database detection for keyframes whose clouds are in the on-device keyframe store (scl_keyframe_put) */
int scl_stream_from_store(scl_engine *e, int robot, int first_index, int count, int *nn_idx, int *shift, double *dist, float *out_values)
{
    if (!e || robot < 0 || first_index < 0 || count < 0 || (count > 0 && (!nn_idx || !shift || !dist))) return SCL_ERR_INVALID_ARG;
    if (e->front) return fail(e, SCL_ERR_UNSUPPORTED, "stream_from_store: the keyframe store lives on one engine; call it on a one-GPU engine");
    std::lock_guard<std::mutex> pk(e->pass_mu);
    std::unique_lock<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    if ((size_t)robot >= e->kf.size() || (size_t)first_index + (size_t)count > e->kf[(size_t)robot].size())
        return fail(e, SCL_ERR_OUT_OF_RANGE, "stream_from_store: keyframes not in the store");
    std::vector<const unsigned char *> d((size_t)count);
    std::vector<int> n((size_t)count), idx((size_t)count);
    std::vector<int8_t> rb((size_t)count, (int8_t)robot);
    for (int i = 0; i < count; ++i) {
        const auto &c = e->kf[(size_t)robot][(size_t)(first_index + i)];
        if (c.n < 0) return fail(e, SCL_ERR_OUT_OF_RANGE, "stream_from_store: a keyframe of the range was never stored");
        d[(size_t)i] = c.d; n[(size_t)i] = c.n; idx[(size_t)i] = first_index + i;
    }
    return device_points_pipeline_locked(e, lk, d.data(), n.data(), count, e->kf_stride, rb.data(), idx.data(), out_values, nn_idx, shift, dist);
}

/* ---- pinned host buffers ----------------------------------------------------------- */

int scl_host_alloc(scl_engine *e, size_t bytes, void **out)
{
    if (!e || !out || bytes == 0) return SCL_ERR_INVALID_ARG;
    scl_engine *t = e->front ? front_primary(e) : e;
    std::lock_guard<std::mutex> lk(t->mu);
    (void)hipSetDevice(t->device);
    void *p = nullptr;
    SCL_HIP(e, hipHostMalloc(&p, bytes, hipHostMallocPortable));
    t->host_allocs.push_back(p);
    *out = p;
    return SCL_OK;
}

int scl_host_free(scl_engine *e, void *p)
{
    if (!e) return SCL_ERR_INVALID_ARG;
    if (!p) return SCL_OK;
    scl_engine *t = e->front ? front_primary(e) : e;
    std::lock_guard<std::mutex> lk(t->mu);
    for (size_t i = 0; i < t->host_allocs.size(); ++i)
        if (t->host_allocs[i] == p) {
            t->host_allocs.erase(t->host_allocs.begin() + (long)i);
            (void)hipSetDevice(t->device);
            SCL_HIP(e, hipHostFree(p));
            return SCL_OK;
        }
    return fail(e, SCL_ERR_INVALID_ARG, "scl_host_free: not a buffer of scl_host_alloc on this engine");
}

int scl_host_register(scl_engine *e, void *p, size_t bytes)
{
    if (!e || !p || bytes == 0) return SCL_ERR_INVALID_ARG;
    scl_engine *t = e->front ? front_primary(e) : e;
    (void)hipSetDevice(t->device);
    SCL_HIP(e, hipHostRegister(p, bytes, hipHostRegisterPortable));
    return SCL_OK;
}

int scl_host_unregister(scl_engine *e, void *p)
{
    if (!e || !p) return SCL_ERR_INVALID_ARG;
    scl_engine *t = e->front ? front_primary(e) : e;
    (void)hipSetDevice(t->device);
    SCL_HIP(e, hipHostUnregister(p));
    return SCL_OK;
}

/* ---- batches of scans from raw points ------------------------------------------------ */

int scl_make_and_save_many(scl_engine *e, const void *const *clouds, const int *n_points, int count, int stride_bytes,
                           const int8_t *robots, const int *indexs, float *out_values)
{
    if (!e || count < 0 || (count > 0 && (!clouds || !n_points))) return SCL_ERR_INVALID_ARG;
    if (e->front) {                                        // sharded: keyframe by keyframe through the owners (correct, not tuned)
        const size_t cells = (size_t)e->R * e->S;
        for (int i = 0; i < count; ++i) {
            const int rc = scl_make_and_save(e, clouds[i], n_points[i], stride_bytes, robots ? robots[i] : (int8_t)0,
                                             indexs ? indexs[i] : scl_get_size(e, -1), out_values ? out_values + (size_t)i * cells : nullptr);
            if (rc) return rc;
        }
        return SCL_OK;
    }
    std::unique_lock<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    return points_pipeline_locked(e, lk, clouds, n_points, count, stride_bytes, robots, indexs, out_values, false, nullptr, nullptr, nullptr);
}

int scl_stream_from_points(scl_engine *e, const void *const *clouds, const int *n_points, int n_scans, int stride_bytes,
                           const int8_t *robots, const int *indexs, int *nn_idx, int *shift, double *dist, float *out_values)
{
    if (!e || n_scans < 0 || (n_scans > 0 && (!clouds || !n_points || !nn_idx || !shift || !dist))) return SCL_ERR_INVALID_ARG;
    if (e->front) {
        const size_t cells = (size_t)e->R * e->S;
        for (int i0 = 0; i0 < n_scans; i0 += kMaxScBatch) {
            const int m = n_scans - i0 < kMaxScBatch ? n_scans - i0 : kMaxScBatch;
            int q[kMaxScBatch], lo[kMaxScBatch], hi[kMaxScBatch];
            for (int j = 0; j < m; ++j) {
                const int key = scl_get_size(e, -1);
                if (key < 0) return key;
                const int rc = scl_make_and_save(e, clouds[i0 + j], n_points[i0 + j], stride_bytes, robots ? robots[i0 + j] : (int8_t)0,
                                                 indexs ? indexs[i0 + j] : key, out_values ? out_values + (size_t)(i0 + j) * cells : nullptr);
                if (rc) return rc;
                q[j] = key; lo[j] = 0; hi[j] = detect_range_hi(e, key);
            }
            const int rc = scl_detect_full_stream(e, q, lo, hi, m, kMaxScBatch, 2, nn_idx + i0, shift + i0, dist + i0);
            if (rc) return rc;
        }
        return SCL_OK;
    }
    std::lock_guard<std::mutex> pk(e->pass_mu);
    std::unique_lock<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    return points_pipeline_locked(e, lk, clouds, n_points, n_scans, stride_bytes, robots, indexs, out_values, true, nn_idx, shift, dist);
}

/* measurement: what ONE large copy from pinned host memory reaches on this box's link (the floor of scl_stream_from_points) */
int scl_host_copy_rate(scl_engine *e, size_t bytes, int reps, double *gbytes_per_s)
{
    if (!e || !gbytes_per_s || bytes == 0 || reps < 1) return SCL_ERR_INVALID_ARG;
    if (e->front) e = front_primary(e);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    void *h = nullptr; unsigned char *d = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t he = hipHostMalloc(&h, bytes, hipHostMallocDefault);
    if (he == hipSuccess) { memset(h, 1, bytes); he = hipMalloc((void **)&d, bytes); }
    if (he == hipSuccess) he = hipEventCreate(&e0);
    if (he == hipSuccess) he = hipEventCreate(&e1);
    if (!e->stream_copy && he == hipSuccess) he = hipStreamCreateWithFlags(&e->stream_copy, hipStreamNonBlocking);
    float ms = 0.f;
    if (he == hipSuccess) he = hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, e->stream_copy);       // warm
    if (he == hipSuccess) he = hipEventRecord(e0, e->stream_copy);
    for (int i = 0; i < reps && he == hipSuccess; ++i) he = hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, e->stream_copy);
    if (he == hipSuccess) he = hipEventRecord(e1, e->stream_copy);
    if (he == hipSuccess) he = hipEventSynchronize(e1);
    if (he == hipSuccess) he = hipEventElapsedTime(&ms, e0, e1);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (d) (void)hipFree(d);
    if (h) (void)hipHostFree(h);
    SCL_HIP(e, he);
    *gbytes_per_s = ms > 0.f ? (double)bytes * reps / (ms * 1e-3) / 1e9 : 0.0;
    return SCL_OK;
}

int scl_get_descriptors(const scl_engine *ce, int first, int count, float *values)
{
    scl_engine *e = const_cast<scl_engine *>(ce);
    if (!e || !values || first < 0 || count < 0) return SCL_ERR_INVALID_ARG;
    const size_t cells = (size_t)e->R * e->S;
    if (e->front) {                                         // sharded: keyframe by keyframe through the owners
        for (int i = 0; i < count; ++i) { const int rc = scl_get_descriptor(e, first + i, values + (size_t)i * cells); if (rc) return rc; }
        return SCL_OK;
    }
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    if (first + count > e->n) return fail(e, SCL_ERR_OUT_OF_RANGE, "get_descriptors: range exceeds the database");
    const int chunk = 512;
    int rc;
    if ((rc = ensure_vals(e, cells * (size_t)(count < chunk ? (count > 0 ? count : 1) : chunk)))) return rc;
    for (int done = 0; done < count; done += chunk) {
        const int c = count - done < chunk ? count - done : chunk;
        for (int i = 0; i < c; ++i)
            SCL_HIP(e, launch_untile(e->db.d_desc + (size_t)(first + done + i) * e->RG * e->S, e->R, e->S, e->d_vals + (size_t)i * cells, e->stream));
        SCL_HIP(e, hipMemcpyAsync(values + (size_t)done * cells, e->d_vals, sizeof(float) * cells * (size_t)c, hipMemcpyDeviceToHost, e->stream));
        if ((rc = sync(e))) return rc;
    }
    return SCL_OK;
}

int scl_db_dump_file(scl_engine *e, const char *path)
{
    if (!e || !path) return SCL_ERR_INVALID_ARG;
    const int n = scl_get_size(e, -1);
    if (n < 0) return n;
    FILE *f = std::fopen(path, "wb");
    if (!f) return fail(e, SCL_ERR_INVALID_ARG, "db_dump: cannot open the file for writing");
    DbFileHeader h{};
    std::memcpy(h.magic, kDbMagic, 8);
    h.version = 1; h.num_ring = e->R; h.num_sector = e->S; h.count = n;
    // state of detectInterLoopClosureID's periodic tree (D.h:1691-1703): reserved[0] = 1 marks the two words as present
    if (!e->front) { std::lock_guard<std::mutex> lk(e->mu); h.reserved[0] = 1; h.reserved[1] = e->tree_counter; h.reserved[2] = e->tree_n; }
    int rc = SCL_OK;
    if (std::fwrite(&h, sizeof h, 1, f) != 1) rc = SCL_ERR_INVALID_ARG;
    const size_t cells = (size_t)e->R * e->S;
    const int chunk = 512;
    std::vector<float> buf(cells * (size_t)chunk);
    for (int done = 0; done < n && !rc; done += chunk) {    // float32[N][R*S], wire order (D.h:1446-1455)
        const int c = n - done < chunk ? n - done : chunk;
        rc = scl_get_descriptors(e, done, c, buf.data());
        if (!rc && std::fwrite(buf.data(), sizeof(float) * cells, (size_t)c, f) != (size_t)c) rc = fail(e, SCL_ERR_INVALID_ARG, "db_dump: short write");
    }
    for (int k = 0; k < n && !rc; ++k) {                    // (robot, index) map, D.h:1758-1761
        int8_t r = 0; int32_t idx = 0;
        rc = scl_get_index(e, k, &r, &idx);
        const int32_t rec[2] = {(int32_t)r, idx};
        if (!rc && std::fwrite(rec, sizeof rec, 1, f) != 1) rc = fail(e, SCL_ERR_INVALID_ARG, "db_dump: short write");
    }
    if (std::fclose(f) != 0 && !rc) rc = fail(e, SCL_ERR_INVALID_ARG, "db_dump: close failed");
    return rc;
}

int scl_db_load_file(scl_engine *e, const char *path, int *n_loaded)
{
    if (!e || !path) return SCL_ERR_INVALID_ARG;
    if (n_loaded) *n_loaded = 0;
    FILE *f = std::fopen(path, "rb");
    if (!f) return fail(e, SCL_ERR_INVALID_ARG, "db_load: cannot open the file");
    const int n_before = scl_get_size(e, -1);
    DbFileHeader h{};
    int sink_rc = 0;
    // the parser (db_file.hpp: host code, fuzzed under ASan / UBSan by `make sanitize`) proves the file's length against its header before
    // anything is sized by it, and hands the descriptors over in chunks
    const int st = db_file_parse(f, e->R, e->S, &h, [&](const float *vals, int c, const int8_t *robots, const int *indexs) {
        const int rc = scl_save_bulk(e, vals, c, robots, indexs);
        if (!rc && n_loaded) *n_loaded += c;
        return rc;
    }, &sink_rc);
    std::fclose(f);
    if (st == DBF_SINK) return sink_rc;                     // (scl_save_bulk left its own message)
    if (st == DBF_NOMEM) return fail(e, SCL_ERR_NOMEM, db_file_status_string(st));
    if (st != DBF_OK) return fail(e, SCL_ERR_INVALID_ARG, db_file_status_string(st));
    // an engine that was empty takes over the dump's inter-robot tree state too (D.h:1691-1703): the next
    // detectInterLoopClosureID searches the range the dumped engine would have searched
    if (n_before == 0 && !e->front && h.reserved[0] == 1) {
        std::lock_guard<std::mutex> lk(e->mu);
        e->tree_counter = h.reserved[1]; e->tree_n = h.reserved[2];
    }
    return SCL_OK;
}

}  // extern "C"

// ---- hooks for the sharded front (engine_internal.hpp) ---------------------------------------------------------
namespace scl {

int eng_stage_from_peer(scl_engine *dst, int j, scl_engine *src, int src_slot, int count)
{
    if (!dst || !src || count < 1 || j < 0 || j + count > dst->stage_rows) return SCL_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(dst->mu);
    if (src_slot < 0 || src_slot + count > src->n) return fail(dst, SCL_ERR_OUT_OF_RANGE, "stage_from_peer: source slot out of range");
    (void)hipSetDevice(dst->device);
    // consecutive slots are consecutive rows of every array on both sides (the strides agree: same grid): one copy per array
    if (dst->hstride != src->hstride || dst->hkw != src->hkw) return fail(dst, SCL_ERR_INVALID_ARG, "stage_from_peer: the shards' layouts differ");
    const int rc = db_arrays_copy_rows(dst, dst->db, (size_t)dst->cap, (size_t)dst->cap + (size_t)j, src->db, (size_t)src->cap, (size_t)src_slot, (size_t)count, true, src);
    if (rc) return rc;
    for (int i = 0; i < count; ++i) dst->staged[j + i] = true;
    return SCL_OK;
}

int eng_set_stage_rows(scl_engine *e, int rows)
{
    if (!e || rows < scl_engine::kStage) return SCL_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->n > 0) return fail(e, SCL_ERR_INVALID_ARG, "stage rows are fixed once a keyframe is stored");
    (void)hipSetDevice(e->device);
    const int old_cap = e->cap;
    e->stage_rows = rows;
    e->staged.assign((size_t)rows, 0);
    e->cap = 0;                                            // empty database: new arrays of the new shape, nothing to copy (the old ones are freed there)
    return ensure_capacity(e, old_cap > 0 ? old_cap : 1);
}

int eng_stage_values(scl_engine *e, int j, const float *values)
{
    if (!e || !values || j < 0 || j >= e->stage_rows) return SCL_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    return stage_values_locked(e, j, values);
}

int eng_ensure_points(scl_engine *e, size_t bytes) { return ensure_points(e, bytes); }   // (the caller holds mu)

bool eng_would_regrow(const scl_engine *e, int count)
{
    std::lock_guard<std::mutex> lk(e->mu);
    return e->n + count > e->cap;
}

// Drop the keyframes from n_keep on (the sharded front undoes a multi-shard append that failed on a later shard; the slots'
// contents are simply overwritten by the next append).  Passes in flight must have been collected by the caller.
int eng_truncate(scl_engine *e, int n_keep)
{
    std::lock_guard<std::mutex> lk(e->mu);
    if (n_keep < 0 || n_keep > e->n) return SCL_ERR_INVALID_ARG;
    e->robots.resize((size_t)n_keep); e->indexs.resize((size_t)n_keep);
    e->n = n_keep;
    if (e->meta_n > n_keep) e->meta_n = n_keep;              // the slots from n_keep on will hold other keyframes: uploaded again
    return SCL_OK;
}

}  // namespace scl
