// engine.hip -- host side of the C ABI (include/scl_engine.h): keyframe database in
// HBM, locking, launch orchestration.  No compute happens on the host except the
// O(k) candidate loop of detectIntra/InterLoopClosureID (descriptor.h:1645-1673,
// 1721-1755), whose float-narrowing comparison order is part of the contract.
// (The registration entry points -- ICP, verification, scoring, submaps, the keyframe store -- are registration.hip's; the host layer of
// the screened search -- the full-database detection in its blocking, ticket and stream forms, the screened distance matrix's loop,
// scl_screen_distances* -- is screen_host.hip's; what fills the database -- its arrays' allocation and growth, the append paths, the
// points pipelines, the pinned buffers, dump and load, the front's hooks into them -- is ingest_host.hip's.  Here: the engine's creation
// and destruction, the views of the database, the ring-key and candidate searches, the readers of single keyframes, the matrix's plain
// loop and its consumers, the ranked searches, the selftests, PCM, the pose-graph solve, the profile and the remaining hooks.)
#include "scl_engine.h"

#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <atomic>
#include <chrono>
#include <thread>
#include <vector>

#include "engine_internal.hpp"
#include "device_sort.hpp"
#include "grid_limits.hpp"
#include "plugin_host.hpp"
#include "pgo_condense_plan.hpp"
#include "pgo_marginal_plan.hpp"

#ifdef SCL_DIAGNOSTICS
namespace scl { void ingest_stamps_print(); void cand_stamps_print(); }   // make_sc.hip / sc_masked.hip: phase stamps (SCL_INGEST_STAMPS=1)
#endif

using namespace scl;

namespace {

// one spin of a polling loop, on whatever the host is (the engine's host code also builds for aarch64 robots)
inline void cpu_relax()
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__) || defined(__arm__)
    asm volatile("yield" ::: "memory");
#else
    std::this_thread::yield();
#endif
}

}  // namespace

// ---- what screen_host.hip shares with this file (engine_internal.hpp declares it) ---------------------------------------------------
namespace scl {

ProfScope::ProfScope(scl_engine *e_, int kind_, hipStream_t s_) : e(e_), kind(kind_), s(s_ ? s_ : e_->stream)
{
    if (!e->prof_on || (e->prof_on >= 2 && kind != P_SC)) return;
#ifndef SCL_PROF_SAMPLE
#define SCL_PROF_SAMPLE 13
#endif
    if (e->prof_on == 3 && (e->prof_tick++ % SCL_PROF_SAMPLE) != 0) return;   // sampled: one launch in thirteen (not a divisor of the launches per chunk;
                                                                             //  an event pair keeps two launches back by 4-6 us each)
    auto get = [&]() {
        hipEvent_t ev = nullptr;
        if (!e->event_pool.empty()) { ev = e->event_pool.back(); e->event_pool.pop_back(); }
        else if (hipEventCreate(&ev) != hipSuccess) ev = nullptr;
        return ev;
    };
    start = get(); stop = get();
    if (start && stop) (void)hipEventRecord(start, s);
}

ProfScope::~ProfScope()
{
    if (!e->prof_on || !start || !stop) return;
    (void)hipEventRecord(stop, s);
    e->pending.push_back({start, stop, kind, 1});
}

void collect_profile(scl_engine *e)
{   // folds every finished (start, stop) pair into the profile; unfinished ones stay pending
    std::vector<PendingEvent> keep;
    for (auto &p : e->pending) {
        if (hipEventQuery(p.stop) != hipSuccess) { keep.push_back(p); continue; }
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.start, p.stop) == hipSuccess) {
            switch (p.kind) {
            case P_SC:     e->prof.sc_distance_ms += ms;  e->prof.sc_distance_launches += (uint64_t)(p.launches > 0 ? p.launches : 1); break;
            case P_TOPK:   e->prof.ringkey_topk_ms += ms; e->prof.ringkey_topk_launches++; break;
            case P_ARGMIN: e->prof.argmin_ms += ms;       e->prof.argmin_launches++; break;
            case P_MAKESC: e->prof.make_sc_ms += ms;      e->prof.make_sc_launches++; break;
            case P_INGEST: e->prof.ingest_ms += ms;       e->prof.ingest_launches++; break;
            case P_ICPNN:  e->prof.icp_nn_ms += ms;       e->prof.icp_nn_launches++; break;
            case P_ICPRED: e->prof.icp_reduce_ms += ms;   e->prof.icp_reduce_launches++; break;
            default: break;
            }
        }
        e->event_pool.push_back(p.start);
        e->event_pool.push_back(p.stop);
    }
    e->pending.swap(keep);
}

int sync(scl_engine *e)
{
    SCL_HIP(e, hipStreamSynchronize(e->stream));
    collect_profile(e);
    return SCL_OK;
}

// An event polled for up to `budget`, then the runtime's blocking wait (which wakes up tens of microseconds late).  relax: a wait of
// milliseconds beside threads that go through the same runtime -- 32 pauses per query, the clock looked at every 256 queries; without
// it (a wait of tens of microseconds) the event and the clock are looked at back to back.
hipError_t wait_event_polled(hipEvent_t ev, std::chrono::microseconds budget, bool relax)
{
    hipError_t q;
    const auto t0 = std::chrono::steady_clock::now();
    int spins = 0;
    while ((q = hipEventQuery(ev)) == hipErrorNotReady) {
        if (relax) {
            for (int p = 0; p < 32; ++p) cpu_relax();
            if ((++spins & 255) != 0) continue;
        }
        if (std::chrono::steady_clock::now() - t0 > budget) return hipEventSynchronize(ev);
    }
    return q;
}

// An error path's wait for what is already enqueued: last_error keeps the first failure, whatever the waits say
void drain_keeping_error(scl_engine *e, const hipStream_t *streams, int n)
{
    const std::string first_error = e->last_error;
    for (int i = 0; i < n; ++i) (void)hipStreamSynchronize(streams[i]);
    e->last_error = first_error;
}

DbView db_view(const scl_engine *e)
{
    const DbArrays &a = e->db;
    DbView v;
    v.desc = a.d_desc; v.vkey = a.d_vkey; v.norm = a.d_norm; v.rkey = a.d_rkey; v.rkey4 = a.d_rkey4;
    v.hdesc = a.d_hdesc; v.kmask = a.d_kmask; v.hkey = a.d_hkey; v.hstride = e->hstride; v.halign = a.d_halign;
    v.cap = e->cap; v.R = e->R; v.S = e->S; v.RG = e->RG;
    return v;
}

// What an ingest launch writes: every array of the slots from first_slot on, out of wire descriptors (`values`) or out of the batch
// scatter's tiles (then vals_out receives their wire form).  stage_row: first_slot is a staging row, which has no tiled ring key and
// no alignment image
IngestArgs ingest_args(const scl_engine *e, int first_slot, const float *values, int *tiles, float *vals_out, bool stage_row)
{
    const DbArrays &a = e->db;
    return IngestArgs{values, first_slot, a.d_desc, a.d_vkey, a.d_norm, a.d_rkey, stage_row ? nullptr : a.d_rkey4, a.d_hdesc, a.d_kmask, a.d_hkey,
                      e->hstride, e->cap, e->R, e->S, stage_row ? nullptr : a.d_halign, tiles, vals_out};
}

int query_view(const scl_engine *e, int query, QueryView *q)
{
    query = query_slot(e, query, e->n);
    if (query == kQueryNotStaged) return fail(e, SCL_ERR_INVALID_ARG, "no staged query (call scl_stage_query first)");
    if (query == kQueryOutOfRange) return fail(e, SCL_ERR_OUT_OF_RANGE, "query slot out of range");
    q->desc = e->db.d_desc + (size_t)query * e->RG * e->S;
    q->vkey = e->db.d_vkey + (size_t)query * e->S;
    q->norm = e->db.d_norm + (size_t)query * e->S;
    q->rkey = e->db.d_rkey + (size_t)query * e->R4;
    q->hdesc = e->db.d_hdesc + (size_t)query * e->hstride;
    q->kmask = e->db.d_kmask + (size_t)query * 8;
    return SCL_OK;
}

int ensure_pairs(scl_engine *e, size_t n)
{
    if (n <= e->pair_cap) return SCL_OK;
    dev_free(e->d_dist); dev_free(e->d_shift); dev_free(e->d_cand); dev_free(e->d_ring_d2);
    dev_free(e->d_approx); dev_free(e->d_surv); dev_free(e->d_starts);
    size_t nn = n + n / 2 + 64;
    int rc;
    e->pair_cap = 0;
    if ((rc = dev_alloc(e, &e->d_approx, nn))) return rc;
    if ((rc = dev_alloc(e, &e->d_starts, nn))) return rc;
    if ((rc = dev_alloc(e, &e->d_surv, nn))) return rc;
    if ((rc = dev_alloc(e, &e->d_ring_d2, nn))) return rc;
    if ((rc = dev_alloc(e, &e->d_dist, nn))) return rc;
    if ((rc = dev_alloc(e, &e->d_shift, nn))) return rc;
    if ((rc = dev_alloc(e, &e->d_cand, nn))) return rc;
    e->pair_cap = nn;
    return SCL_OK;
}

// screening buffers: kScreenSets sets of at least n entries each
int ensure_sets(scl_engine *e, size_t n)
{
    if (n <= e->set_stride && e->pair_cap >= e->set_stride * scl_engine::kScreenSets) return SCL_OK;
    const size_t stride = n + n / 4 + 64;
    int rc = ensure_pairs(e, stride * scl_engine::kScreenSets);
    if (rc) { e->set_stride = 0; return rc; }
    e->set_stride = stride;
    // the shift masks follow the sets (the exact passes evaluate the open shifts only: sc_masked.hip, sc_matrix.hip)
    if (e->smask_cap < stride * scl_engine::kScreenSets) {
        dev_free(e->d_smask); e->d_smask = nullptr; e->smask_cap = 0;
        if ((rc = dev_alloc(e, &e->d_smask, stride * scl_engine::kScreenSets))) { e->set_stride = 0; return rc; }
        e->smask_cap = stride * scl_engine::kScreenSets;
    }
    const size_t need = 2 * stride * sc_screen_scratch_floats(db_view(e), e->SR);   // floats: ring parts x passes x 16 shifts per pair of a launch; two launches' worth (a launch's finishing rides in the next launch)
    if (need > e->part_cap) {
        dev_free(e->d_part); e->part_cap = 0;
        if ((rc = dev_alloc(e, &e->d_part, need))) { e->set_stride = 0; return rc; }
        e->part_cap = need;
    }
    return SCL_OK;
}

int launch_topk(scl_engine *e, const QueryView &q, int lo, int hi, int k, float eps, hipStream_t on)
{
    hipStream_t s = on ? on : e->stream;
    ProfScope ps(e, P_TOPK, s);
    SCL_HIP(e, launch_ringkey_topk(db_view(e), q.rkey, lo, hi, k, eps, e->d_topk_scratch,
                                   e->d_topk_idx, e->d_topk_d2, s));
    return SCL_OK;
}

// The end of a SHORT blocking call (tens of microseconds of device time): an event behind its last launch, polled for up to 300 us,
// then a sleep in the runtime -- hipStreamSynchronize wakes up tens of microseconds late, a fifth of such a call.
int sync_short(scl_engine *e)
{
    if (!e->ev_call) SCL_HIP(e, hipEventCreateWithFlags(&e->ev_call, hipEventDisableTiming));
    SCL_HIP(e, hipEventRecord(e->ev_call, e->stream));
    const hipError_t q = wait_event_polled(e->ev_call, std::chrono::microseconds(300), false);
    SCL_HIP(e, q);
    collect_profile(e);
    return SCL_OK;
}

}  // namespace scl

namespace {

int ensure_pinned(scl_engine *e, size_t bytes)
{
    if (bytes <= e->pinned_cap) return SCL_OK;
    if (e->h_pinned) { (void)hipHostFree(e->h_pinned); e->h_pinned = nullptr; e->pinned_cap = 0; }
    SCL_HIP(e, hipHostMalloc(&e->h_pinned, bytes, hipHostMallocDefault));
    memset(e->h_pinned, 0, bytes);                          // (a polled sequence word must never start out as somebody's old number)
    e->pinned_cap = bytes;
    return SCL_OK;
}

int launch_distance(scl_engine *e, const QueryView &q, const int *d_cand, int slot_base, int n)
{
    ProfScope ps(e, P_SC);
    SCL_HIP(e, launch_sc_distance(db_view(e), q, d_cand, slot_base, n, e->SR, e->d_dist, e->d_shift,
                                  e->num_cu, e->stream));
    if (ps.active()) e->prof.sc_distance_pairs += (uint64_t)n;
    return SCL_OK;
}

// top-k in [lo,hi) followed by the SC distance of those k candidates; enqueue puts the launches and the copies
// into pinned memory on the engine's stream, finish waits for them and unpacks (the sharded front enqueues on
// every device before it waits on any).
// The ring-key scan leaves per-workgroup lists; the kernel that consumes the k nearest merges them in its prologue
// (topk_merge.hpp): the candidates' kernel of the reference-faithful detection, or the merge + pack kernel of the bare search.
int topk_enqueue_locked(scl_engine *e, int query, int lo, int hi, int k, float eps, bool want_dist, bool *have_dist)
{
    if (k <= 0 || k > kTopkMaxK) return fail(e, SCL_ERR_INVALID_ARG, "k out of range (1..64)");
    QueryView q;
    int rc = query_view(e, query, &q);
    if (rc) return rc;
    clamp_range(lo, hi, e->n);
    if ((rc = ensure_pairs(e, (size_t)k))) return rc;
    int n_lists = 0;
    {
        ProfScope ps(e, P_TOPK);
        SCL_HIP(e, launch_ringkey_lists(db_view(e), q.rkey, lo, hi, k, eps, e->d_topk_scratch, &n_lists, e->stream));
    }
    *have_dist = hi > lo && want_dist;
    const size_t need = cand_seq_offset(k) + 16;
    if ((rc = ensure_pinned(e, need))) return rc;
    e->pinned_seq = 0;
    if (*have_dist && k <= 16 && sc_cand_exact_supported(db_view(e), e->SR) && !scl_lab_int("SCL_CAND_EXACT_OFF", 0)) {
        // the reference-faithful detection's k (3) candidates: one workgroup merges the scan's lists, aligns and scores the candidates
        // and writes the block (sc_masked.hip)
        const bool fused = n_lists * k <= kCandMergeMaxKeys;
        if (!fused) SCL_HIP(e, launch_topk_merge(e->d_topk_scratch, n_lists, k, e->d_topk_idx, e->d_topk_d2, nullptr, e->stream));
        ProfScope ps(e, P_SC);
        if (++e->out_seq == 0) ++e->out_seq;
        e->pinned_seq = e->out_seq;
        // the word sits at an offset that depends on k: a call with a larger k left idx[] / d2[] data there -- cleared before the launch
        *reinterpret_cast<volatile unsigned int *>(static_cast<char *>(e->h_pinned) + cand_seq_offset(k)) = 0u;
        std::atomic_thread_fence(std::memory_order_release);
        SCL_HIP(e, launch_sc_cand_exact(db_view(e), q, e->SR, k, e->d_topk_idx, e->d_topk_d2, e->h_pinned, e->stream, e->pinned_seq,
                                        fused ? e->d_topk_scratch : nullptr, n_lists, e->d_topk_idx, e->d_topk_d2));
        if (ps.active()) e->prof.sc_distance_pairs += (uint64_t)k;
        return SCL_OK;
    }
    if (*have_dist) {
        SCL_HIP(e, launch_topk_merge(e->d_topk_scratch, n_lists, k, e->d_topk_idx, e->d_topk_d2, nullptr, e->stream));
        if ((rc = launch_distance(e, q, e->d_topk_idx, 0, k))) return rc;
        // the k results travel as ONE block written by a kernel into pinned memory (four copies of a few bytes cost more than the search)
        SCL_HIP(e, launch_topk_pack(e->d_topk_idx, e->d_topk_d2, e->d_dist, e->d_shift, k, true, e->h_pinned, e->stream));
        return SCL_OK;
    }
    // the bare search: merge and block in one launch
    SCL_HIP(e, launch_topk_merge(e->d_topk_scratch, n_lists, k, e->d_topk_idx, e->d_topk_d2, e->h_pinned, e->stream));
    return SCL_OK;
}

int topk_finish_locked(scl_engine *e, int k, bool have_dist, int *idx, float *d2, double *dist, int *shift, int *found)
{
    int rc;
    char *h = static_cast<char *>(e->h_pinned);
    bool seen = false;
    if (e->pinned_seq) {
        // the candidates' kernel writes this call's number behind the block: seen here 4-6 us before an event behind the launch would fire
        const volatile unsigned int *w = reinterpret_cast<const volatile unsigned int *>(h + cand_seq_offset(k));
        const auto t0 = std::chrono::steady_clock::now();
        int spins = 0;
        seen = true;
        while (*w != e->pinned_seq)
            if ((++spins & 255) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(300)) { seen = false; break; }
        std::atomic_thread_fence(std::memory_order_acquire);      // the block behind the word is read below through plain pointers
        if (seen) collect_profile(e);
    }
    if (!seen && (rc = sync_short(e))) return rc;
    const int *h_idx = reinterpret_cast<int *>(h);
    const float *h_d2 = reinterpret_cast<float *>(h + sizeof(int) * k);
    const double *h_dist = reinterpret_cast<double *>(h + (sizeof(int) + sizeof(float)) * k);
    const int *h_shift = reinterpret_cast<int *>(h + (sizeof(int) + sizeof(float) + sizeof(double)) * k);
    int nf = 0;
    for (int i = 0; i < k; ++i) {
        if (idx) idx[i] = h_idx[i];
        if (d2) d2[i] = h_d2[i];
        if (dist) dist[i] = have_dist ? h_dist[i] : kBigDist;
        if (shift) shift[i] = have_dist ? h_shift[i] : 0;
        if (h_idx[i] >= 0) nf++;
    }
    if (found) *found = nf;
    return SCL_OK;
}

int topk_with_distance_locked(scl_engine *e, int query, int lo, int hi, int k, float eps,
                              int *idx, float *d2, double *dist, int *shift, int *found)
{
    bool have_dist = false;
    int rc = topk_enqueue_locked(e, query, lo, hi, k, eps, dist || shift, &have_dist);
    if (rc) return rc;
    return topk_finish_locked(e, k, have_dist, idx, d2, dist, shift, found);
}

}  // namespace

extern "C" {

const char *scl_status_string(int status)
{
    switch (status) {
    case SCL_OK: return "ok";
    case SCL_ERR_INVALID_ARG: return "invalid argument";
    case SCL_ERR_NO_DEVICE: return "no HIP device";
    case SCL_ERR_HIP: return "HIP runtime error";
    case SCL_ERR_OUT_OF_RANGE: return "index out of range";
    case SCL_ERR_NOMEM: return "out of memory";
    case SCL_ERR_UNSUPPORTED: return "unsupported";
    case SCL_ERR_NUMERIC: return "a factorisation failed";
    default: return "unknown status";
    }
}

const char *scl_last_error(const scl_engine *e) { return e ? e->last_error.c_str() : "null engine"; }

int scl_abi_version(void) { return 16; }

int scl_default_config(scl_config *c)
{
    if (!c) return SCL_ERR_INVALID_ARG;
    c->num_ring = 20; c->num_sector = 60; c->num_candidates = 3;       /* D.h:1308-1310 */
    c->dist_thres = 0.14; c->lidar_height = 1.65; c->max_radius = 80.0; /* D.h:1311-1313 */
    c->num_exclude_recent = 100; c->tree_making_period = 10;            /* D.h:1314-1315 */
    c->search_ratio = 0.1;                                              /* D.h:1316 */
    c->knn_exclude_eps = 0.0f;
    c->device = 0;
    c->initial_capacity = 4096;
    return SCL_OK;
}

// Every environment switch the library reads selects a correct path, but a leftover one can cost an order of magnitude
// (SCL_SCREEN=0 scores every pair with the exact kernel): the first engine of a process says which ones it found set.
static void log_env_overrides_once()
{
    static std::atomic<bool> done{false};
    if (done.exchange(true)) return;
    static const char *const names[] = {"SCL_SCREEN", "SCL_SCREEN_FORM", "SCL_SCREEN_V2_MIN", "SCL_SCREEN_PAIR", "SCL_TAIL_PAIR", "SCL_RCCL_LIB",
                                        // experiments: read by a diagnostics build only (kernels.hpp: scl_lab_int)
                                        "SCL_SCREEN_VARIANT", "SCL_SCREEN_PROBE", "SCL_SCREEN_TAIL", "SCL_ALIGN_WGS",
                                        "SCL_ALIGN2_WGS", "SCL_ALIGN_FILTER", "SCL_SC_KERNEL", "SCL_SC_WAVES", "SCL_STAMP", "SCL_ABLATE",
                                        "SCL_ICP_REDUCE", "SCL_MATRIX_PLAIN", "SCL_MATRIX_KERNEL", "SCL_MATRIX_KR", "SCL_WIDE_EXACT", "SCL_STREAM_EXACT", "SCL_SMALL_EXACT_OFF",
                                        "SCL_SELF_ALIGN_OFF", "SCL_CAND_EXACT_OFF"};
    constexpr int kProduct = 6;
    int i = 0;
    for (const char *n : names) {
        const char *v = getenv(n);
#ifdef SCL_DIAGNOSTICS
        if (v) fprintf(stderr, "scl_engine (diagnostics build): environment override in effect: %s=%s\n", n, v);
#else
        if (v && i < kProduct) fprintf(stderr, "scl_engine: environment override in effect: %s=%s\n", n, v);
        else if (v) fprintf(stderr, "scl_engine: %s=%s is an experiment's switch: ignored by this build (make EXTRA=-DSCL_DIAGNOSTICS builds them in)\n", n, v);
#endif
        ++i;
    }
    (void)kProduct;
}

int scl_create(const scl_config *cfg, scl_engine **out)
{
    if (!cfg || !out) return SCL_ERR_INVALID_ARG;
    *out = nullptr;
    log_env_overrides_once();
    if (cfg->num_ring < 1 || cfg->num_ring > 256 || cfg->num_sector < 1 || cfg->num_sector > 1024 ||
        cfg->num_candidates < 1 || cfg->num_candidates > kTopkMaxK || cfg->tree_making_period < 1 ||
        cfg->num_exclude_recent < 0 || !(cfg->max_radius > 0.0) || !(cfg->search_ratio >= 0.0))
        return SCL_ERR_INVALID_ARG;
    {   // a grid some kernel of the front end or of the search cannot take is refused here, before the device is touched, and not at
        // its first launch (grid_limits.hpp has every limit and where it comes from)
        int SR = (int)std::round(0.5 * cfg->search_ratio * (double)cfg->num_sector);   /* D.h:1545 */
        if (SR < 0) SR = 0;
        if (!grid_supported(cfg->num_ring, cfg->num_sector, SR)) return SCL_ERR_UNSUPPORTED;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SCL_ERR_NO_DEVICE;
    if (cfg->device < 0 || cfg->device >= ndev) return SCL_ERR_INVALID_ARG;
    scl_engine *e = new (std::nothrow) scl_engine();
    if (!e) return SCL_ERR_NOMEM;
    e->cfg = *cfg;
    e->R = cfg->num_ring; e->S = cfg->num_sector;
    e->RG = (e->R + 3) / 4; e->R4 = e->RG * 4;
    e->hstride = hdesc_stride(e->RG, e->S);
    e->hkw = hkey_row_halfs(e->S);
    e->SR = (int)std::round(0.5 * cfg->search_ratio * (double)e->S);   /* D.h:1545 */
    if (e->SR < 0) e->SR = 0;
    e->device = cfg->device;
    int rc = SCL_OK;
    auto bail = [&](int code) { scl_destroy(e); return code; };
    if (hipSetDevice(e->device) != hipSuccess) return bail(SCL_ERR_HIP);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, e->device) == hipSuccess && prop.multiProcessorCount > 0)
        e->num_cu = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) return bail(SCL_ERR_HIP);
    {   // the ring-key scan is small: give its queue priority so it slips in beside the SC-distance kernel
        int lo_p = 0, hi_p = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo_p, &hi_p);
        if (hipStreamCreateWithPriority(&e->stream2, hipStreamNonBlocking, hi_p) != hipSuccess) return bail(SCL_ERR_HIP);
    }
    if (hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming) != hipSuccess) return bail(SCL_ERR_HIP);
    if (hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming) != hipSuccess) return bail(SCL_ERR_HIP);
    if (hipHostMalloc((void **)&e->h_out3, 64 * scl_engine::kSlots, hipHostMallocDefault) != hipSuccess) return bail(SCL_ERR_HIP);
    memset(e->h_out3, 0, 64 * scl_engine::kSlots);          // o[4] of a record is a polled sequence number
    for (int i = 0; i < scl_engine::kSlots; ++i)
        if (hipEventCreateWithFlags(&e->ev_done[i], hipEventDisableTiming) != hipSuccess) return bail(SCL_ERR_HIP);
    if ((rc = ensure_capacity(e, 1))) return bail(rc);
    if ((rc = dev_alloc(e, &e->d_topk_scratch, (size_t)kTopkMaxBlocks * kTopkMaxK + 2))) return bail(rc);   // partial lists + the scan's ticket counter
    if (hipMemset(e->d_topk_scratch, 0, sizeof(unsigned long long) * ((size_t)kTopkMaxBlocks * kTopkMaxK + 2)) != hipSuccess) return bail(SCL_ERR_HIP);
    if ((rc = dev_alloc(e, &e->d_topk_idx, (size_t)kTopkMaxK * scl_engine::kScreenSets))) return bail(rc);
    if ((rc = dev_alloc(e, &e->d_topk_d2, (size_t)kTopkMaxK * scl_engine::kScreenSets))) return bail(rc);
    if ((rc = dev_alloc(e, &e->d_out3, (size_t)4))) return bail(rc);
    if ((rc = dev_alloc(e, &e->d_blk_part, (size_t)kTailBlocks * kTailRec * kMaxQueryBatch))) return bail(rc);
    static_assert(kMaxQueryBatch <= 4, "done_counter holds four counters");
    if ((rc = dev_alloc(e, &e->d_done_counter, (size_t)4))) return bail(rc);
    if (hipMemset(e->d_done_counter, 0, 16) != hipSuccess) return bail(SCL_ERR_HIP);
    {
        constexpr int NS = scl_engine::kScreenSets;
        if ((rc = dev_alloc(e, &e->d_nsurv, (size_t)NS))) return bail(rc);
        static_assert(NS <= kTminEpsOffset, "the launch's largest bound sits kTminEpsOffset words behind its t_min word");
        if ((rc = dev_alloc(e, &e->d_tmin, (size_t)NS + kTminEpsOffset))) return bail(rc);
        if (hipMemset(e->d_nsurv, 0, sizeof(int) * NS) != hipSuccess) return bail(SCL_ERR_HIP);
        if (hipMemset(e->d_tmin, 0xff, sizeof(unsigned int) * NS) != hipSuccess) return bail(SCL_ERR_HIP);
        if (hipMemset(e->d_tmin + NS, 0, sizeof(unsigned int) * kTminEpsOffset) != hipSuccess) return bail(SCL_ERR_HIP);
        if ((rc = dev_alloc(e, &e->d_surv_part, (size_t)NS * kSurvivorBlocks * kTailRec))) return bail(rc);
        if ((rc = dev_alloc(e, &e->d_surv_done, (size_t)NS))) return bail(rc);
        if (hipMemset(e->d_surv_done, 0, sizeof(unsigned int) * NS) != hipSuccess) return bail(SCL_ERR_HIP);
        if (hipMalloc(&e->d_surv_args, (size_t)8 * NS * kSurvivorArgBytes) != hipSuccess) return bail(SCL_ERR_NOMEM);
        if (hipHostMalloc(&e->h_surv_args, (size_t)8 * NS * kSurvivorArgBytes, hipHostMallocDefault) != hipSuccess) return bail(SCL_ERR_HIP);
        if (hipHostMalloc((void **)&e->h_stream_out, (size_t)2 * NS * 64, hipHostMallocDefault) != hipSuccess) return bail(SCL_ERR_HIP);
        for (auto &ev : e->ev_chunk) if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return bail(SCL_ERR_HIP);
        for (auto &ev : e->ev_k1) if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return bail(SCL_ERR_HIP);
        for (auto &ev : e->ev_sub0) if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return bail(SCL_ERR_HIP);
        if (hipEventCreateWithFlags(&e->ev_align_gate, hipEventDisableTiming) != hipSuccess) return bail(SCL_ERR_HIP);
        {   // lowest priority: its workgroups take the slots the products leave, not the other way round
            int lo_p = 0, hi_p = 0;
            (void)hipDeviceGetStreamPriorityRange(&lo_p, &hi_p);
            // (80 x 180: the exact pass is a dozen short launches per chunk with a handful of survivors each, and the next-but-one chunk is
            //  submitted when it has ended: starved by the products -- 150-180 us per masked launch instead of 35 -- it ended when the
            //  next chunk's screening did and the main stream ran dry for 60 us per chunk.  There it goes FIRST.)
            const bool wide_grid = e->S == 180 && e->RG == 20;
            if (hipStreamCreateWithPriority(&e->stream_surv, hipStreamNonBlocking, wide_grid ? hi_p : lo_p) != hipSuccess) return bail(SCL_ERR_HIP);
            // never used: HIP deals streams onto the hardware queues round robin in creation order, and this one keeps stream_alt and
            // every stream created later on the queues they were measured on (engine_internal.hpp)
            if (hipStreamCreateWithPriority(&e->stream_queue_place, hipStreamNonBlocking, lo_p) != hipSuccess) return bail(SCL_ERR_HIP);
        }
    }
    if (hipStreamCreateWithFlags(&e->stream_alt, hipStreamNonBlocking) != hipSuccess) return bail(SCL_ERR_HIP);
    if (hipEventCreateWithFlags(&e->ev_db, hipEventDisableTiming) != hipSuccess) return bail(SCL_ERR_HIP);
    if ((rc = dev_alloc(e, &e->d_align_fallbacks, (size_t)1))) return bail(rc);
    if (hipMemset(e->d_align_fallbacks, 0, sizeof(unsigned long long)) != hipSuccess) return bail(SCL_ERR_HIP);
    if ((rc = dev_alloc(e, &e->d_surv_stats, (size_t)3))) return bail(rc);
    if (hipMemset(e->d_surv_stats, 0, 3 * sizeof(unsigned long long)) != hipSuccess) return bail(SCL_ERR_HIP);
    if ((rc = ensure_pairs(e, 1024))) return bail(rc);
    e->screen = sc_screen_supported(db_view(e), e->SR) && cfg->num_candidates <= kTailTopMaxK;
    if ((rc = ensure_pinned(e, 1 << 16))) return bail(rc);
    if ((rc = ensure_vals(e, (size_t)e->R * e->S))) return bail(rc);
    *out = e;
    return SCL_OK;
}

int scl_destroy(scl_engine *e)
{
#ifdef SCL_DIAGNOSTICS
    if (e && !e->front && scl_lab_int("SCL_INGEST_STAMPS", 0)) { (void)hipSetDevice(e->device); scl::ingest_stamps_print(); scl::cand_stamps_print(); }
#endif
    if (!e) return SCL_OK;
    if (e->front) return front_destroy(e);
    (void)hipSetDevice(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    for (auto &p : e->pending) { (void)hipEventDestroy(p.start); (void)hipEventDestroy(p.stop); }
    for (auto ev : e->event_pool) (void)hipEventDestroy(ev);
    icp_workspace_free(&e->icp_ws);
    icp_workspace_free(&e->vox_ws);
    for (void *slab : e->kf_slabs) (void)hipFree(slab);
    for (int i = 0; i < scl_engine::kIcpBatch; ++i) icp_workspace_free(&e->icp_batch_ws[i]);
    for (int i = 0; i < scl_engine::kIcpLanes; ++i) icp_workspace_free(&e->vox_lane_ws[i]);
    icp_workspace_free(&e->icp_batch_ctl);
    pcm_workspace_free(&e->pcm_ws);
    pgo_workspace_free(&e->pgo_ws);
    map_free(&e->gmap);
    for (int i = 0; i < scl_engine::kIcpLanes; ++i) {
        if (e->ev_lane[i]) (void)hipEventDestroy(e->ev_lane[i]);
        icp_workspace_free(&e->icp_lane_ws[i]);
        if (e->icp_lane_stream[i]) (void)hipStreamDestroy(e->icp_lane_stream[i]);
    }
    db_arrays_free(e->db);
    dev_free(e->d_vals); dev_free(e->d_points); dev_free(e->d_tiles);
    for (int b = 0; b < 3; ++b) {
        dev_free(e->d_pbuf[b]);
        for (int c = 0; c < scl_engine::kCopyStreams; ++c) if (e->ev_copied[c][b]) (void)hipEventDestroy(e->ev_copied[c][b]);
        if (e->ev_consumed[b]) (void)hipEventDestroy(e->ev_consumed[b]);
    }
    if (e->stream_copy) { (void)hipStreamSynchronize(e->stream_copy); (void)hipStreamDestroy(e->stream_copy); }
    for (hipStream_t cs : e->stream_copy_x) if (cs) { (void)hipStreamSynchronize(cs); (void)hipStreamDestroy(cs); }
    for (void *hp : e->host_allocs) (void)hipHostFree(hp);
    dev_free(e->d_dist); dev_free(e->d_shift); dev_free(e->d_cand); dev_free(e->d_ring_d2);
    dev_free(e->d_approx); dev_free(e->d_starts); dev_free(e->d_surv); dev_free(e->d_nsurv); dev_free(e->d_tmin); dev_free(e->d_part);
    dev_free(e->d_align_fallbacks);
    dev_free(e->d_smask);
    if (e->d_mat_dist) (void)hipFree(e->d_mat_dist);
    if (e->d_mat_shift) (void)hipFree(e->d_mat_shift);
    if (e->d_rank_key) (void)hipFree(e->d_rank_key);
    if (e->d_rank_pos) (void)hipFree(e->d_rank_pos);
    if (e->d_rank_out) (void)hipFree(e->d_rank_out);
    if (e->h_rank_out) (void)hipHostFree(e->h_rank_out);
    dev_free(e->d_meta_robot); dev_free(e->d_meta_index);
    if (e->h_mat) (void)hipHostFree(e->h_mat);
    for (auto &ev : e->ev_mat_k) if (ev) (void)hipEventDestroy(ev);
    for (auto &ev : e->ev_mat_c) if (ev) (void)hipEventDestroy(ev);
    dev_free(e->d_surv_stats);
    dev_free(e->d_surv_part); dev_free(e->d_surv_done);
    if (e->d_surv_args) (void)hipFree(e->d_surv_args);
    if (e->h_surv_args) (void)hipHostFree(e->h_surv_args);
    if (e->h_stream_out) (void)hipHostFree(e->h_stream_out);
    for (auto ev : e->ev_chunk) if (ev) (void)hipEventDestroy(ev);
    if (e->stream_surv) { (void)hipStreamSynchronize(e->stream_surv); (void)hipStreamDestroy(e->stream_surv); }
    if (e->stream_queue_place) (void)hipStreamDestroy(e->stream_queue_place);
    for (auto ev : e->ev_k1) if (ev) (void)hipEventDestroy(ev);
    for (auto ev : e->ev_sub0) if (ev) (void)hipEventDestroy(ev);
    if (e->ev_align_gate) (void)hipEventDestroy(e->ev_align_gate);
    dev_free(e->d_topk_scratch); dev_free(e->d_topk_idx); dev_free(e->d_topk_d2); dev_free(e->d_out3);
    dev_free(e->d_blk_part); dev_free(e->d_done_counter);
    if (e->ev_db) (void)hipEventDestroy(e->ev_db);
    if (e->stream_alt) { (void)hipStreamSynchronize(e->stream_alt); (void)hipStreamDestroy(e->stream_alt); }
    if (e->h_pinned) (void)hipHostFree(e->h_pinned);
    if (e->h_out3) (void)hipHostFree(e->h_out3);
    if (e->ev_call) (void)hipEventDestroy(e->ev_call);
    for (int i = 0; i < scl_engine::kSlots; ++i) if (e->ev_done[i]) (void)hipEventDestroy(e->ev_done[i]);
    if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
    if (e->ev_join) (void)hipEventDestroy(e->ev_join);
    if (e->stream2) { (void)hipStreamSynchronize(e->stream2); (void)hipStreamDestroy(e->stream2); }
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
    return SCL_OK;
}

/* ---- the six virtuals ------------------------------------------------------ */

int scl_detect_intra(scl_engine *e, int cur, int *loop_id, float *shift, double *dist)
{
    if (!e || !loop_id || !shift) return SCL_ERR_INVALID_ARG;
    if (e->front) return front_detect_intra(e, cur, loop_id, shift, dist);
    std::lock_guard<std::mutex> pk(e->pass_mu);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    *loop_id = -1; *shift = 0.0f;                                         /* D.h:1615 */
    if (dist) *dist = kBigDist;
    if (cur < 0 || cur >= e->n) return fail(e, SCL_ERR_OUT_OF_RANGE, "cur out of range");
    const int k = e->cfg.num_candidates;
    if (cur < e->cfg.num_exclude_recent + k + 1) return SCL_OK;           /* D.h:1620-1623 */
    const int history = cur - e->cfg.num_exclude_recent;                  /* D.h:1627 */
    int idx[kTopkMaxK]; float d2[kTopkMaxK]; double cd[kTopkMaxK]; int ca[kTopkMaxK];
    int rc = topk_with_distance_locked(e, cur, 0, history, k, e->cfg.knn_exclude_eps, idx, d2, cd, ca, nullptr);
    if (rc) return rc;
    float minDis = 10000000.0f;                                           /* D.h:1637: a float */
    int minIndex = -1, minBias = 0;
    for (int i = 0; i < k; ++i) {                                         /* D.h:1645-1659 */
        if (idx[i] < 0) continue;
        if (cd[i] < (double)minDis) {                                     /* D.h:1653 */
            minDis = (float)cd[i];                                        /* D.h:1655 narrowing */
            minIndex = idx[i];
            minBias = ca[i];
        }
    }
    if (dist) *dist = (double)minDis;
    if ((double)minDis < e->cfg.dist_thres) {                             /* D.h:1662 */
        *loop_id = minIndex;
        *shift = (float)minBias;                                          /* D.h:1665 */
    }
    return SCL_OK;
}

int scl_detect_inter(scl_engine *e, int cur, int *loop_id, float *yaw_rad, double *dist)
{
    if (!e || !loop_id || !yaw_rad) return SCL_ERR_INVALID_ARG;
    if (e->front) return front_detect_inter(e, cur, loop_id, yaw_rad, dist);
    std::lock_guard<std::mutex> pk(e->pass_mu);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    *loop_id = -1; *yaw_rad = 0.0f;                                       /* D.h:1678,1686 */
    if (dist) *dist = kBigDist;
    if (cur < 0 || cur >= e->n) return fail(e, SCL_ERR_OUT_OF_RANGE, "cur out of range");
    if (e->n < e->cfg.num_exclude_recent + 1) return SCL_OK;              /* D.h:1684-1688 */
    if (e->tree_counter % e->cfg.tree_making_period == 0)                 /* D.h:1691-1702 */
        e->tree_n = e->n - e->cfg.num_exclude_recent;
    e->tree_counter = e->tree_counter + 1;                                /* D.h:1703 */
    const int k = e->cfg.num_candidates;
    int idx[kTopkMaxK]; float d2[kTopkMaxK]; double cd[kTopkMaxK]; int ca[kTopkMaxK];
    int rc = topk_with_distance_locked(e, cur, 0, e->tree_n, k, 0.0f, idx, d2, cd, ca, nullptr);
    if (rc) return rc;
    // slots the search left unfilled read as index 0 in the reference (zero-initialised
    // candidate_indexes, D.h:1710): score slot 0 for them.
    bool need0 = false;
    for (int i = 0; i < k; ++i) need0 |= idx[i] < 0;
    double cd0 = kBigDist; int ca0 = 0;
    if (need0 && e->tree_n > 0) {
        QueryView q;
        if ((rc = query_view(e, cur, &q))) return rc;
        if ((rc = launch_distance(e, q, nullptr, 0, 1))) return rc;
        SCL_HIP(e, hipMemcpyAsync(e->h_pinned, e->d_dist, sizeof(double), hipMemcpyDeviceToHost, e->stream));
        SCL_HIP(e, hipMemcpyAsync((char *)e->h_pinned + 8, e->d_shift, sizeof(int), hipMemcpyDeviceToHost, e->stream));
        if ((rc = sync(e))) return rc;
        cd0 = *reinterpret_cast<double *>(e->h_pinned);
        ca0 = *reinterpret_cast<int *>((char *)e->h_pinned + 8);
    }
    double min_dist = 10000000;                                           /* D.h:1705 */
    int nn_align = 0, nn_idx = -1;
    for (int i = 0; i < k; ++i) {                                         /* D.h:1721-1737 */
        const int ci = idx[i] < 0 ? 0 : idx[i];
        const double c = idx[i] < 0 ? cd0 : cd[i];
        const int al = idx[i] < 0 ? ca0 : ca[i];
        if (c < min_dist) {
            if (ci == cur) continue;                                      /* D.h:1731 */
            min_dist = c; nn_align = al; nn_idx = ci;
        }
    }
    if (min_dist < e->cfg.dist_thres) *loop_id = nn_idx;                  /* D.h:1741-1744 */
    const double unit_sector_angle = 360.0 / (double)e->S;                /* D.h:1332 */
    *yaw_rad = (float)(nn_align * unit_sector_angle * M_PI / 180.0);      /* D.h:1752 */
    if (dist) *dist = min_dist;
    return SCL_OK;
}

int scl_get_index(const scl_engine *e, int key, int8_t *robot, int *index)
{
    if (!e || !robot || !index) return SCL_ERR_INVALID_ARG;
    if (e->front) return front_get_index(e, key, robot, index);
    std::lock_guard<std::mutex> lk(e->mu);
    if (key < 0 || key >= e->n) return fail(e, SCL_ERR_OUT_OF_RANGE, "key out of range");
    *robot = e->robots[key];
    *index = e->indexs[key];
    return SCL_OK;
}

int scl_get_size(const scl_engine *e, int id)
{
    (void)id;                                                             /* D.h:1763-1766 ignores idIn */
    if (!e) return SCL_ERR_INVALID_ARG;
    if (e->front) return front_get_size(e);
    std::lock_guard<std::mutex> lk(e->mu);
    return e->n;
}

/* ---- building blocks -------------------------------------------------------- */

int scl_get_descriptor(const scl_engine *ce, int key, float *values)
{
    scl_engine *e = const_cast<scl_engine *>(ce);
    if (!e || !values) return SCL_ERR_INVALID_ARG;
    if (e->front) { scl_engine *child = nullptr; int slot = 0; const int rc = front_get_slot(e, key, &child, &slot); return rc ? rc : scl_get_descriptor(child, slot, values); }
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    if (key < 0 || key >= e->n) return fail(e, SCL_ERR_OUT_OF_RANGE, "key out of range");
    int rc;
    const size_t cells = (size_t)e->R * e->S;
    if ((rc = ensure_vals(e, cells))) return rc;
    SCL_HIP(e, launch_untile(e->db.d_desc + (size_t)key * e->RG * e->S, e->R, e->S, e->d_vals, e->stream));
    SCL_HIP(e, hipMemcpyAsync(values, e->d_vals, sizeof(float) * cells, hipMemcpyDeviceToHost, e->stream));
    return sync(e);
}

int scl_get_ringkey(const scl_engine *ce, int key, float *ringkey)
{
    scl_engine *e = const_cast<scl_engine *>(ce);
    if (!e || !ringkey) return SCL_ERR_INVALID_ARG;
    if (e->front) { scl_engine *child = nullptr; int slot = 0; const int rc = front_get_slot(e, key, &child, &slot); return rc ? rc : scl_get_ringkey(child, slot, ringkey); }
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    if (key < 0 || key >= e->n) return fail(e, SCL_ERR_OUT_OF_RANGE, "key out of range");
    SCL_HIP(e, hipMemcpyAsync(ringkey, e->db.d_rkey + (size_t)key * e->R4, sizeof(float) * e->R,
                              hipMemcpyDeviceToHost, e->stream));
    return sync(e);
}

int scl_get_sectorkey(const scl_engine *ce, int key, double *sectorkey)
{
    scl_engine *e = const_cast<scl_engine *>(ce);
    if (!e || !sectorkey) return SCL_ERR_INVALID_ARG;
    if (e->front) { scl_engine *child = nullptr; int slot = 0; const int rc = front_get_slot(e, key, &child, &slot); return rc ? rc : scl_get_sectorkey(child, slot, sectorkey); }
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    if (key < 0 || key >= e->n) return fail(e, SCL_ERR_OUT_OF_RANGE, "key out of range");
    SCL_HIP(e, hipMemcpyAsync(sectorkey, e->db.d_vkey + (size_t)key * e->S, sizeof(double) * e->S,
                              hipMemcpyDeviceToHost, e->stream));
    return sync(e);
}

int scl_ringkey_topk(scl_engine *e, int query, int lo, int hi, int k, int *idx, float *d2, int *found)
{
    if (!e || !idx || !d2) return SCL_ERR_INVALID_ARG;
    if (e->front) return front_topk(e, query, lo, hi, k, idx, d2, nullptr, nullptr, found);
    std::lock_guard<std::mutex> pk(e->pass_mu);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    return topk_with_distance_locked(e, query, lo, hi, k, e->cfg.knn_exclude_eps, idx, d2, nullptr, nullptr, found);
}

int scl_topk_with_distance(scl_engine *e, int query, int lo, int hi, int k,
                           int *idx, float *d2, double *dist, int *shift, int *found)
{
    if (!e || !idx || !d2 || !dist || !shift) return SCL_ERR_INVALID_ARG;
    if (e->front) return front_topk(e, query, lo, hi, k, idx, d2, dist, shift, found);
    std::lock_guard<std::mutex> pk(e->pass_mu);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    return topk_with_distance_locked(e, query, lo, hi, k, e->cfg.knn_exclude_eps, idx, d2, dist, shift, found);
}

int scl_sc_distance_batch(scl_engine *e, int query, const int *cand, int n, double *dist, int *shift)
{
    if (!e || n < 0 || !dist || !shift) return SCL_ERR_INVALID_ARG;
    if (n == 0) return SCL_OK;
    if (e->front) return front_sc_distance_batch(e, query, cand, n, dist, shift);
    std::lock_guard<std::mutex> pk(e->pass_mu);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    QueryView q;
    int rc = query_view(e, query, &q);
    if (rc) return rc;
    if (cand) {
        for (int i = 0; i < n; ++i)
            if (cand[i] >= e->n) return fail(e, SCL_ERR_OUT_OF_RANGE, "candidate slot out of range");
    } else if (n > e->n) {
        return fail(e, SCL_ERR_OUT_OF_RANGE, "n exceeds database size");
    }
    if ((rc = ensure_pairs(e, (size_t)n))) return rc;
    if (cand) SCL_HIP(e, hipMemcpyAsync(e->d_cand, cand, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, e->stream));
    if ((rc = launch_distance(e, q, cand ? e->d_cand : nullptr, 0, n))) return rc;
    SCL_HIP(e, hipMemcpyAsync(dist, e->d_dist, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, e->stream));
    SCL_HIP(e, hipMemcpyAsync(shift, e->d_shift, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, e->stream));
    return sync(e);
}

namespace {

// The group loops of the distance matrix (matrix_plain_locked, matrix_screened_locked) produce the rows group by group into the halves
// d_mat_dist / d_mat_shift; what happens to a finished group is the consumer's: scl_sc_distance_matrix copies the rows to the host
// (MatrixToHost), the ranked search selects on the device and copies the lists (RankGroups).  (MatrixGroup and MatrixConsumer, the
// interface between the loops and the consumers, are engine_internal.hpp's: the screened loop is screen_host.hip's.)
bool matrix_is_screened(const scl_engine *e) { return e->screen && sc_masked_supported(db_view(e), e->SR) && !scl_lab_int("SCL_MATRIX_PLAIN", 0); }
int matrix_group_rows(const scl_engine *e) { return matrix_is_screened(e) ? sc_screen_max_batch(db_view(e), e->SR) : kMaxQueryBatch; }
int matrix_plain_locked(scl_engine *e, const int *slots, int nq, const int *grp_lo, const int *grp_n, MatrixConsumer &out);

// scl_sc_distance_matrix's consumer: a group's rows travel to the pinned halves on the second stream and from there to the caller
struct MatrixToHost final : MatrixConsumer {
    scl_engine *e; int nq, n, per_group; double *dist; int *shift;
    int rb = 0; size_t cap = 0;
    MatrixToHost(scl_engine *e_, int nq_, int n_, int per_group_, double *dist_, int *shift_) : e(e_), nq(nq_), n(n_), per_group(per_group_), dist(dist_), shift(shift_) {}
    int enqueued(const MatrixGroup &m) override
    {
        rb = m.rb; cap = m.cap;
        double *h_dist = static_cast<double *>(e->h_mat);
        int *h_shift = reinterpret_cast<int *>(h_dist + (size_t)2 * rb * cap);
        const int h = m.h, rows = m.rows;
        SCL_HIP(e, hipEventRecord(e->ev_mat_k[h], m.ks));
        SCL_HIP(e, hipStreamWaitEvent(e->stream2, e->ev_mat_k[h], 0));
        SCL_HIP(e, hipMemcpyAsync(h_dist + (size_t)h * rb * cap, e->d_mat_dist + (size_t)h * rb * cap, sizeof(double) * (size_t)rows * cap, hipMemcpyDeviceToHost, e->stream2));
        SCL_HIP(e, hipMemcpyAsync(h_shift + (size_t)h * rb * cap, e->d_mat_shift + (size_t)h * rb * cap, sizeof(int) * (size_t)rows * cap, hipMemcpyDeviceToHost, e->stream2));
        SCL_HIP(e, hipEventRecord(e->ev_mat_c[h], e->stream2));
        return SCL_OK;
    }
    int retire(int g) override                                             // group g's rows: pinned half -> the caller's arrays
    {
        const int h = g & 1, r0 = g * per_group, rows = nq - r0 < per_group ? nq - r0 : per_group;
        const double *h_dist = static_cast<const double *>(e->h_mat);
        const int *h_shift = reinterpret_cast<const int *>(h_dist + (size_t)2 * rb * cap);
        SCL_HIP(e, hipEventSynchronize(e->ev_mat_c[h]));
        for (int r = 0; r < rows; ++r) {
            std::memcpy(dist + (size_t)(r0 + r) * n, h_dist + ((size_t)h * rb + r) * cap, sizeof(double) * (size_t)n);
            std::memcpy(shift + (size_t)(r0 + r) * n, h_shift + ((size_t)h * rb + r) * cap, sizeof(int) * (size_t)n);
        }
        return SCL_OK;
    }
};

}  // namespace

/* The exact distance matrix (north_star: "the column-shifted SC distance matrix over the keyframe database"): rows = queries,
 * columns = keyframes lo .. hi-1, every entry the reference's distanceBtnScanContext (D.h:1538-1569) in fp64 with its shift.
 * Up to kMaxQueryBatch rows per launch of the wave program; a launch's results travel to the host (pinned halves, second
 * stream) while the next launch runs. */
int scl_sc_distance_matrix(scl_engine *e, const int *queries, int nq, int lo, int hi, double *dist, int *shift)
{
    if (!e || nq < 0 || (nq > 0 && (!queries || !dist || !shift))) return SCL_ERR_INVALID_ARG;
    if (nq == 0) return SCL_OK;
    if (e->front) return front_sc_distance_matrix(e, queries, nq, lo, hi, dist, shift);
    std::lock_guard<std::mutex> pk(e->pass_mu);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    if (lo < 0 || hi > e->n || hi < lo) return fail(e, SCL_ERR_OUT_OF_RANGE, "keyframe range out of the database");
    const int n = hi - lo;
    if (n == 0) return SCL_OK;
    std::vector<int> slots((size_t)nq);
    for (int i = 0; i < nq; ++i) {
        const int q = queries[i];
        if (q >= e->n || q < -e->stage_rows) return fail(e, SCL_ERR_OUT_OF_RANGE, "query keyframe out of range");
        if (q < 0 && !e->staged[-1 - q]) return fail(e, SCL_ERR_INVALID_ARG, "no staged query in that slot");
        slots[(size_t)i] = q >= 0 ? q : e->cap + (-1 - q);
    }
    // (the screened grids: alignment + screening of 16 rows at a time, then the exact evaluation of the shifts still open, sc_masked.hip)
    const int per_group = matrix_group_rows(e), groups = (nq + per_group - 1) / per_group;
    const std::vector<int> grp_lo((size_t)groups, lo), grp_n((size_t)groups, n);
    MatrixToHost out(e, nq, n, per_group, dist, shift);
    if (matrix_is_screened(e)) return matrix_screened_locked(e, slots.data(), nq, grp_lo.data(), grp_n.data(), out);
    return matrix_plain_locked(e, slots.data(), nq, grp_lo.data(), grp_n.data(), out);
}

namespace {

// The matrix on the grids without a screening pass: kMaxQueryBatch rows per launch of the wave program, group g into half g & 1.
// Group g covers the keyframes [grp_lo[g], grp_lo[g] + grp_n[g]) (a group of no keyframes launches nothing).
int matrix_plain_locked(scl_engine *e, const int *slots, int nq, const int *grp_lo, const int *grp_n, MatrixConsumer &out)
{
    constexpr int RB = kMaxQueryBatch;                                     // rows per launch
    const int groups = (nq + RB - 1) / RB;
    int max_n = 0;
    for (int g = 0; g < groups; ++g) max_n = grp_n[g] > max_n ? grp_n[g] : max_n;
    const size_t row = ((size_t)max_n + 63) & ~(size_t)63;
    if (e->mat_cap < row) {
        if (e->d_mat_dist) (void)hipFree(e->d_mat_dist);
        if (e->d_mat_shift) (void)hipFree(e->d_mat_shift);
        if (e->h_mat) (void)hipHostFree(e->h_mat);
        e->d_mat_dist = nullptr; e->d_mat_shift = nullptr; e->h_mat = nullptr; e->mat_cap = 0;
        if (hipMalloc((void **)&e->d_mat_dist, sizeof(double) * 2 * RB * row) != hipSuccess ||
            hipMalloc((void **)&e->d_mat_shift, sizeof(int) * 2 * RB * row) != hipSuccess ||
            hipHostMalloc(&e->h_mat, (sizeof(double) + sizeof(int)) * 2 * RB * row, hipHostMallocDefault) != hipSuccess)
            return fail(e, SCL_ERR_NOMEM, "distance matrix buffers");
        e->mat_cap = row;
        for (int h = 0; h < 2; ++h) {
            if (!e->ev_mat_k[h]) SCL_HIP(e, hipEventCreateWithFlags(&e->ev_mat_k[h], hipEventDisableTiming));
            if (!e->ev_mat_c[h]) SCL_HIP(e, hipEventCreateWithFlags(&e->ev_mat_c[h], hipEventDisableTiming));
        }
    }
    const size_t cap = e->mat_cap;
    int rc = SCL_OK;
    for (int g = 0; g < groups; ++g) {
        const int h = g & 1, r0 = g * RB, rows = nq - r0 < RB ? nq - r0 : RB;
        const int lo = grp_lo[g], n = grp_n[g];
        if (g >= 2 && (rc = out.retire(g - 2))) return rc;                 // (also: half h of the device buffers has been copied out)
        if (n > 0) {
            ProfScope ps(e, P_SC);
            SCL_HIP(e, launch_sc_distance_matrix(db_view(e), slots + r0, rows, lo, n, e->SR, e->d_mat_dist + (size_t)h * RB * cap,
                                                 e->d_mat_shift + (size_t)h * RB * cap, cap, e->num_cu, e->stream));
            if (ps.active()) e->prof.sc_distance_pairs += (uint64_t)rows * (uint64_t)n;
        }
        if ((rc = out.enqueued({g, h, r0, rows, RB, cap, lo, n, e->stream, 0, 0}))) return rc;
    }
    for (int g = groups >= 2 ? groups - 2 : 0; g < groups; ++g)
        if ((rc = out.retire(g))) return rc;
    if (e->prof_on) collect_profile(e);
    return SCL_OK;
}

}  // namespace

namespace {

// The ranked search's consumer: behind a group's exact kernel, on the SAME stream, the selection (sc_rank.hip) and the copy of the
// group's rows x k records to pinned memory.  The next group that writes this half (g + 2) runs on that stream too -- both groups of a
// half share a lane on 80 x 180 --, so a half is never written before its ranking has read it, and the host waits for nothing here.
struct RankGroups final : MatrixConsumer {
    scl_engine *e; int k; const int *qlo, *qhi; const ScRankRule *rules; size_t part_half; bool used_alt = false;
    RankGroups(scl_engine *e_, int k_, const int *qlo_, const int *qhi_, const ScRankRule *rules_, size_t part_half_)
        : e(e_), k(k_), qlo(qlo_), qhi(qhi_), rules(rules_), part_half(part_half_) {}
    int enqueued(const MatrixGroup &m) override
    {
        ScRankArgs a{};
        a.dist = e->d_mat_dist + (size_t)m.h * m.rb * m.cap; a.shift = e->d_mat_shift + (size_t)m.h * m.rb * m.cap; a.row_stride = m.cap;
        a.rows = m.rows; a.n = m.n; a.base = m.lo; a.k = k;
        for (int r = 0; r < m.rows; ++r) {                                  // the row covers the group's union; the list its own range
            const int l = qlo[m.r0 + r], h = qhi[m.r0 + r];
            a.plo[r] = h > l ? l - m.lo : 0; a.phi[r] = h > l ? h - m.lo : 0;
            if (rules) a.rule[r] = rules[m.r0 + r];
        }
        if (rules) { a.meta_robot = e->d_meta_robot; a.meta_index = e->d_meta_index; }   // (uploaded and waited for before the first group: both lanes see them)
        a.part_key = e->d_rank_key + (size_t)m.h * part_half; a.part_pos = e->d_rank_pos + (size_t)m.h * part_half;
        ScRankRecord *d_out = static_cast<ScRankRecord *>(e->d_rank_out) + (size_t)m.r0 * k;
        a.out = d_out;
        SCL_HIP(e, launch_sc_rank(a, m.ks));
        if (m.sets > 0) {
            // The group's screening launches left the smallest screened distance of every row in its buffer set's t_min word (and the
            // launch's largest bound behind it), which only the exact pass of a full-database detection re-arms -- the matrix's kernels
            // do not read them.  Left as they are, a later scl_detect_full* through these sets would select its survivors against
            // another scan's minimum; a search leaves no trace, so the words go back to their initial state here.
            SCL_HIP(e, hipMemsetAsync(e->d_tmin + m.set0, 0xff, sizeof(unsigned int) * (size_t)m.sets, m.ks));
            SCL_HIP(e, hipMemsetAsync(e->d_tmin + kTminEpsOffset + m.set0, 0, sizeof(unsigned int) * (size_t)m.sets, m.ks));
        }
        SCL_HIP(e, hipMemcpyAsync(static_cast<ScRankRecord *>(e->h_rank_out) + (size_t)m.r0 * k, d_out, sizeof(ScRankRecord) * (size_t)m.rows * k, hipMemcpyDeviceToHost, m.ks));
        used_alt |= m.ks == e->stream_alt;
        return SCL_OK;
    }
    int retire(int) override { return SCL_OK; }
};

// Is keyframe `s` in the search set of a rule?  (The host's copy of the selection's test, sc_rank.hip.)
inline bool rule_admits(const scl_engine *e, const ScRankRule &u, int s)
{
    if (!(u.flags & kScRuleActive)) return true;
    if (((int)e->robots[(size_t)s] == u.robot) == ((u.flags & kScRuleNotEqual) != 0)) return false;
    return !(u.flags & kScRuleIndex) || e->indexs[(size_t)s] < u.bound;
}

// The device copy of (robots, indexs) the ruled selection reads, brought up to the database: new arrays when the database's arrays
// have grown, then the slots behind the watermark.  The vectors are pageable and may move with the next append, so the copy is waited
// for here -- which also puts it in front of whatever either lane launches afterwards.
int meta_upload_locked(scl_engine *e)
{
    if (e->meta_cap != e->cap) {
        dev_free(e->d_meta_robot); dev_free(e->d_meta_index); e->meta_cap = 0; e->meta_n = 0;
        if (hipMalloc((void **)&e->d_meta_robot, sizeof(signed char) * (size_t)e->cap) != hipSuccess ||
            hipMalloc((void **)&e->d_meta_index, sizeof(int) * (size_t)e->cap) != hipSuccess) {
            dev_free(e->d_meta_robot); dev_free(e->d_meta_index);
            return fail(e, SCL_ERR_NOMEM, "ranked search: (robot, index) arrays");
        }
        e->meta_cap = e->cap;
    }
    if (e->meta_n >= e->n) return SCL_OK;
    const size_t o = (size_t)e->meta_n, m = (size_t)(e->n - e->meta_n);
    SCL_HIP(e, hipMemcpyAsync(e->d_meta_robot + o, e->robots.data() + o, sizeof(signed char) * m, hipMemcpyHostToDevice, e->stream));
    SCL_HIP(e, hipMemcpyAsync(e->d_meta_index + o, e->indexs.data() + o, sizeof(int) * m, hipMemcpyHostToDevice, e->stream));
    SCL_HIP(e, hipStreamSynchronize(e->stream));
    e->meta_n = e->n;
    return SCL_OK;
}

// scl_sc_search_range behind the locks; everything is validated before anything is sized or launched.  rules != nullptr: the
// robot-aware searches -- query i lists the keyframes of [lo[i], hi[i]) that satisfy rules[i], and its matrix range is narrowed to
// [first such keyframe, last such keyframe + 1) (the lists do not depend on that: what the narrowing leaves out the rule excludes).
int sc_search_locked(scl_engine *e, const int *queries, const int *lo, const int *hi, int nq, int k,
                     int *cand_ids, int *cand_shifts, double *cand_dists, int *n_found, const ScRankRule *rules = nullptr)
{
    std::vector<int> slots((size_t)nq);
    for (int i = 0; i < nq; ++i) {
        const int q = queries[i];
        if (q >= e->n || q < -e->stage_rows) return fail(e, SCL_ERR_OUT_OF_RANGE, "query keyframe out of range");
        if (q < 0 && !e->staged[-1 - q]) return fail(e, SCL_ERR_INVALID_ARG, "no staged query in that slot");
        if (lo[i] < 0 || hi[i] > e->n || hi[i] < lo[i]) return fail(e, SCL_ERR_OUT_OF_RANGE, "keyframe range out of the database");
        slots[(size_t)i] = q >= 0 ? q : e->cap + (-1 - q);
    }
    std::vector<int> nlo, nhi;
    if (rules) {
        int rc = meta_upload_locked(e);
        if (rc) return rc;
        nlo.assign((size_t)nq, 0); nhi.assign((size_t)nq, 0);
        for (int i = 0; i < nq; ++i) {
            int first = lo[i], last = hi[i];
            while (first < last && !rule_admits(e, rules[i], first)) ++first;
            while (last > first && !rule_admits(e, rules[i], last - 1)) --last;
            if (last > first) { nlo[(size_t)i] = first; nhi[(size_t)i] = last; }      // (nothing eligible: the empty range [0, 0))
        }
        lo = nlo.data(); hi = nhi.data();
    }
    // a group's matrix runs over the union of its queries' ranges
    const int per_group = matrix_group_rows(e), groups = (nq + per_group - 1) / per_group;
    std::vector<int> grp_lo((size_t)groups, 0), grp_n((size_t)groups, 0);
    int max_n = 0;
    for (int g = 0; g < groups; ++g) {
        int l = INT_MAX, h = 0;
        for (int i = g * per_group; i < nq && i < (g + 1) * per_group; ++i)
            if (hi[i] > lo[i]) { l = lo[i] < l ? lo[i] : l; h = hi[i] > h ? hi[i] : h; }
        if (h > l) { grp_lo[(size_t)g] = l; grp_n[(size_t)g] = h - l; }
        max_n = grp_n[(size_t)g] > max_n ? grp_n[(size_t)g] : max_n;
    }
    // work buffers: the tiles' lists of two groups in flight, grown like the matrix halves; the call's records and their pinned copy
    const size_t part_half = sc_rank_part_entries(per_group, max_n, k);
    if (e->rank_part_cap < part_half) {
        dev_free(e->d_rank_key); dev_free(e->d_rank_pos); e->rank_part_cap = 0;
        if (hipMalloc((void **)&e->d_rank_key, sizeof(unsigned long long) * 2 * part_half) != hipSuccess ||
            hipMalloc((void **)&e->d_rank_pos, sizeof(unsigned int) * 2 * part_half) != hipSuccess)
            return fail(e, SCL_ERR_NOMEM, "ranked search: work buffers");
        e->rank_part_cap = part_half;
    }
    const size_t recs = (size_t)nq * (size_t)k;
    if (e->rank_out_cap < recs) {
        if (e->d_rank_out) (void)hipFree(e->d_rank_out);
        if (e->h_rank_out) (void)hipHostFree(e->h_rank_out);
        e->d_rank_out = nullptr; e->h_rank_out = nullptr; e->rank_out_cap = 0;
        if (hipMalloc(&e->d_rank_out, sizeof(ScRankRecord) * recs) != hipSuccess ||
            hipHostMalloc(&e->h_rank_out, sizeof(ScRankRecord) * recs, hipHostMallocDefault) != hipSuccess)
            return fail(e, SCL_ERR_NOMEM, "ranked search: result buffers");
        e->rank_out_cap = recs;
    }
    RankGroups out(e, k, lo, hi, rules, part_half);
    int rc = matrix_is_screened(e) ? matrix_screened_locked(e, slots.data(), nq, grp_lo.data(), grp_n.data(), out)
                                   : matrix_plain_locked(e, slots.data(), nq, grp_lo.data(), grp_n.data(), out);
    if (rc) return rc;
    if (out.used_alt) SCL_HIP(e, hipStreamSynchronize(e->stream_alt));     // the one wait of the call (one per lane)
    if ((rc = sync(e))) return rc;
    const ScRankRecord *h = static_cast<const ScRankRecord *>(e->h_rank_out);
    for (int i = 0; i < nq; ++i) {
        int found = 0;
        for (int j = 0; j < k; ++j) {
            const ScRankRecord &r = h[(size_t)i * k + j];
            cand_ids[(size_t)i * k + j] = r.id;
            if (cand_shifts) cand_shifts[(size_t)i * k + j] = r.shift;
            if (cand_dists) cand_dists[(size_t)i * k + j] = r.dist;
            found += r.id >= 0;
        }
        if (n_found) n_found[i] = found;
    }
    return SCL_OK;
}

}  // namespace

/* The ranked search: the distance matrix's rows, group by group, with the selection of the k best behind each group on the device
 * (sc_rank.hip); include/scl_engine.h, THE RANKED SEARCH, has the contract. */
int scl_sc_search_range(scl_engine *e, const int *queries, const int *lo, const int *hi, int n_queries, int k,
                        int *cand_ids, int *cand_shifts, double *cand_dists, int *n_found)
{
    if (!e || n_queries < 0 || k < 1 || k > SCL_SC_SEARCH_MAX || (n_queries > 0 && (!queries || !lo || !hi || !cand_ids))) return SCL_ERR_INVALID_ARG;
    if (n_queries == 0) return SCL_OK;
    if (e->front) return front_sc_search_range(e, queries, lo, hi, n_queries, k, cand_ids, cand_shifts, cand_dists, n_found);
    std::lock_guard<std::mutex> pk(e->pass_mu);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    return sc_search_locked(e, queries, lo, hi, n_queries, k, cand_ids, cand_shifts, cand_dists, n_found);
}

int scl_sc_search(scl_engine *e, const int *curs, int count, int k, int *cand_ids, int *cand_shifts, double *cand_dists, int *n_found)
{
    if (!e || count < 0 || k < 1 || k > SCL_SC_SEARCH_MAX || (count > 0 && (!curs || !cand_ids))) return SCL_ERR_INVALID_ARG;
    if (count == 0) return SCL_OK;
    std::vector<int> lo((size_t)count, 0), hi((size_t)count, 0);
    for (int i = 0; i < count; ++i) {
        if (curs[i] < 0) return SCL_ERR_OUT_OF_RANGE;                      // (a staged query has no place in the database: scl_sc_search_range)
        hi[(size_t)i] = detect_range_hi(e, curs[i]);
    }
    return scl_sc_search_range(e, curs, lo.data(), hi.data(), count, k, cand_ids, cand_shifts, cand_dists, n_found);
}

namespace {

// both calls behind their argument checks
int sc_search_robot(scl_engine *e, const int *curs, int count, bool inter, int robot_pre, int k,
                    int *cand_ids, int *cand_shifts, double *cand_dists, int *n_found)
{
    std::lock_guard<std::mutex> pk(e->pass_mu);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    for (int i = 0; i < count; ++i)
        if (curs[i] < 0 || curs[i] >= e->n) return fail(e, SCL_ERR_OUT_OF_RANGE, "query keyframe out of range");
    std::vector<ScRankRule> rules((size_t)count);
    for (int i = 0; i < count; ++i) {
        const int r = e->robots[(size_t)curs[i]], x = e->indexs[(size_t)curs[i]];
        if (inter && robot_pre != SCL_SC_ANY_OTHER_ROBOT && robot_pre == r) return fail(e, SCL_ERR_INVALID_ARG, "robot_pre is the query's own robot: that is scl_sc_search_intra's set");
        rules[(size_t)i] = inter ? sc_inter_rule(r, robot_pre) : sc_intra_rule(r, x, e->cfg.num_exclude_recent);
    }
    const std::vector<int> lo((size_t)count, 0), hi((size_t)count, e->n);
    return sc_search_locked(e, curs, lo.data(), hi.data(), count, k, cand_ids, cand_shifts, cand_dists, n_found, rules.data());
}

}  // namespace

/* The robot-aware ranked searches: scl_sc_search's lists over the search sets a multi-robot caller needs, defined by the VALUE of each
 * keyframe's (robot, index) and not by its slot; include/scl_engine.h, THE RANKED SEARCH, has the contract. */
int scl_sc_search_intra(scl_engine *e, const int *curs, int count, int k, int *cand_ids, int *cand_shifts, double *cand_dists, int *n_found)
{
    if (!e || count < 0 || k < 1 || k > SCL_SC_SEARCH_MAX || (count > 0 && (!curs || !cand_ids))) return SCL_ERR_INVALID_ARG;
    if (count == 0) return SCL_OK;
    if (e->front) return front_sc_search_intra(e, curs, count, k, cand_ids, cand_shifts, cand_dists, n_found);
    return sc_search_robot(e, curs, count, false, 0, k, cand_ids, cand_shifts, cand_dists, n_found);
}

int scl_sc_search_inter(scl_engine *e, const int *curs, int count, int robot_pre, int k, int *cand_ids, int *cand_shifts, double *cand_dists,
                        int *n_found)
{
    if (!e || count < 0 || k < 1 || k > SCL_SC_SEARCH_MAX || (count > 0 && (!curs || !cand_ids))) return SCL_ERR_INVALID_ARG;
    if (robot_pre < SCL_SC_ANY_OTHER_ROBOT || robot_pre > 127) return SCL_ERR_INVALID_ARG;
    if (count == 0) return SCL_OK;
    if (e->front) return front_sc_search_inter(e, curs, count, robot_pre, k, cand_ids, cand_shifts, cand_dists, n_found);
    return sc_search_robot(e, curs, count, true, robot_pre, k, cand_ids, cand_shifts, cand_dists, n_found);
}

/* test hook: the descriptor scatter's fast binning (device_common.hpp: sc_bin_fast) against the reference's chain (sc_bin_exact,
 * D.h:1425-1435) on n generated points of the engine's grid */
int scl_selftest_bin_paths(scl_engine *e, int mode, uint64_t seed, uint64_t n_points, uint64_t *disagreements, uint64_t *sure)
{
    if (!e || !disagreements || !sure || mode < 0 || mode > 3) return SCL_ERR_INVALID_ARG;
    if (e->front) e = front_primary(e);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    unsigned long long *d = nullptr, h[2] = {0, 0};
    int rc = dev_alloc(e, &d, (size_t)2);
    if (rc) return rc;
    hipError_t he = launch_bin_paths_selftest(mode, seed, n_points, e->R, e->S, e->cfg.max_radius, d, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    dev_free(d);
    SCL_HIP(e, he);
    *disagreements = h[0]; *sure = h[1];
    return SCL_OK;
}

/* test hook: how far the fast binning's quotients are from the chain's on the sure points of n generated points of the engine's grid
 * (make_sc.hip: bin_margin_selftest_kernel has the modes) */
int scl_selftest_bin_margin(scl_engine *e, int mode, uint64_t seed, uint64_t n_points, uint64_t *disagreements, uint64_t *sure,
                            double *max_ring_dev, double *max_sector_dev)
{
    if (!e || !disagreements || !sure || !max_ring_dev || !max_sector_dev || mode < 0 || mode > 2) return SCL_ERR_INVALID_ARG;
    if (e->front) e = front_primary(e);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    unsigned long long *d = nullptr, h[4] = {0, 0, 0, 0};
    int rc = dev_alloc(e, &d, (size_t)4);
    if (rc) return rc;
    hipError_t he = launch_bin_margin_selftest(mode, seed, n_points, e->R, e->S, e->cfg.max_radius, d, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    dev_free(d);
    SCL_HIP(e, he);
    *disagreements = h[0]; *sure = h[1];
    memcpy(max_ring_dev, &h[2], sizeof(double)); memcpy(max_sector_dev, &h[3], sizeof(double));
    return SCL_OK;
}

/* test hook: csrc/device_sort.hip's stable radix sort on the key bits [0, bits) -- key_bytes 4 or 8; n_segments > 1: every segment
 * [segment_offsets[s], segment_offsets[s + 1]) on its own -- as the verification path uses it (voxel.hip, icp.hip) */
int scl_selftest_sort_pairs(scl_engine *e, int key_bytes, const void *keys, const uint32_t *values, int n, int bits, const int *segment_offsets,
                            int n_segments, void *keys_out, uint32_t *values_out)
{
    if (!e || n < 0 || (key_bytes != 4 && key_bytes != 8) || (n > 0 && (!keys || !values || !keys_out || !values_out))) return SCL_ERR_INVALID_ARG;
    if (n_segments < 0 || n_segments > kSortMaxSegments || (n_segments > 1 && (!segment_offsets || key_bytes != 8))) return SCL_ERR_INVALID_ARG;
    if (n == 0) return SCL_OK;
    if (e->front) e = front_primary(e);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    SortSegments seg{};
    seg.nseg = n_segments > 1 ? n_segments : 1; seg.off[0] = 0; seg.off[1] = n;
    if (n_segments > 1) {
        for (int s = 0; s <= n_segments; ++s) seg.off[s] = segment_offsets[s];
        if (seg.off[0] != 0 || seg.off[n_segments] != n) return SCL_ERR_INVALID_ARG;
    }
    unsigned char *d = nullptr;
    const size_t kb = (size_t)key_bytes * (size_t)n, vb = sizeof(uint32_t) * (size_t)n, kpad = (kb + 255) & ~(size_t)255, vpad = (vb + 255) & ~(size_t)255;
    const size_t sb = sort_scratch_bytes((size_t)n, seg.nseg);
    int rc = dev_alloc(e, &d, 2 * kpad + 2 * vpad + sb);
    if (rc) return rc;
    unsigned char *k0 = d, *k1 = d + kpad, *v0 = d + 2 * kpad, *v1 = v0 + vpad, *scratch = v1 + vpad;
    hipError_t he = hipMemcpyAsync(k0, keys, kb, hipMemcpyHostToDevice, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(v0, values, vb, hipMemcpyHostToDevice, e->stream);
    if (he == hipSuccess) {
        if (key_bytes == 4) he = sort_pairs_u32(scratch, (unsigned int *)k0, (unsigned int *)k1, (unsigned int *)v0, (unsigned int *)v1, n, bits, e->stream);
        else {
            // keys whose high word is the same throughout every segment take the 8-byte records of voxel.hip's batch (device_sort.hpp)
            unsigned int seg_hi[kSortMaxSegments];
            bool uniform = bits <= 32;
            const unsigned long long *hk = static_cast<const unsigned long long *>(keys);
            for (int s = 0; s < seg.nseg && uniform; ++s) {
                seg_hi[s] = seg.off[s] < seg.off[s + 1] ? (unsigned int)(hk[seg.off[s]] >> 32) : 0u;
                for (int i = seg.off[s]; i < seg.off[s + 1]; ++i) if ((unsigned int)(hk[i] >> 32) != seg_hi[s]) { uniform = false; break; }
            }
            he = sort_pairs_u64_segmented(scratch, (unsigned long long *)k0, (unsigned long long *)k1, (unsigned int *)v0, (unsigned int *)v1, seg, bits, e->stream,
                                          uniform ? seg_hi : nullptr);
        }
    }
    if (he == hipSuccess) he = hipMemcpyAsync(keys_out, k1, kb, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(values_out, v1, vb, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    dev_free(d);
    SCL_HIP(e, he);
    return SCL_OK;
}

/* test hook: csrc/device_sort.hip's prefix sum of n ints (in place on the device, as the cell table's is) */
int scl_selftest_prefix_sum(scl_engine *e, const int32_t *in, int n, int inclusive, int32_t *out)
{
    if (!e || n < 0 || (n > 0 && (!in || !out))) return SCL_ERR_INVALID_ARG;
    if (n == 0) return SCL_OK;
    if (e->front) e = front_primary(e);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    unsigned char *d = nullptr;
    const size_t nb = (sizeof(int32_t) * (size_t)n + 255) & ~(size_t)255;
    int rc = dev_alloc(e, &d, nb + scan_scratch_bytes((size_t)n));
    if (rc) return rc;
    hipError_t he = hipMemcpyAsync(d, in, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, e->stream);
    if (he == hipSuccess) he = prefix_sum_i32(d + nb, (const int *)d, (int *)d, n, inclusive != 0, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(out, d, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    dev_free(d);
    SCL_HIP(e, he);
    return SCL_OK;
}

/* test hook: the device's atanf (xy2theta, D.h:1352-1374) over blocks of 2^24 float bit patterns, as the checksums of
 * tests/golden/atanf_blocks.json */
int scl_selftest_atanf_blocks(scl_engine *e, int first_block, int n_blocks, uint64_t *checksums)
{
    if (!e || !checksums || first_block < 0 || n_blocks < 1 || first_block + n_blocks > 256) return SCL_ERR_INVALID_ARG;
    if (e->front) e = front_primary(e);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    unsigned long long *d = nullptr;
    int rc = dev_alloc(e, &d, (size_t)n_blocks);
    if (rc) return rc;
    hipError_t he = launch_atanf_block_checksums(first_block, n_blocks, d, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(checksums, d, sizeof(uint64_t) * (size_t)n_blocks, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    dev_free(d);
    SCL_HIP(e, he);
    return SCL_OK;
}

int scl_get_last_topk(scl_engine *e, int k, int *idx, float *d2)
{
    if (!e || !idx || !d2 || k < 1 || k > kTopkMaxK) return SCL_ERR_INVALID_ARG;
    if (e->front) return front_get_last_topk(e, k, idx, d2);
    std::lock_guard<std::mutex> pk(e->pass_mu);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    if (e->last_pass_empty) {                              // the last pass had an empty range: no neighbours
        for (int i = 0; i < k; ++i) { idx[i] = -1; d2[i] = FLT_MAX; }
        return SCL_OK;
    }
    SCL_HIP(e, hipMemcpyAsync(idx, e->d_topk_idx, sizeof(int) * k, hipMemcpyDeviceToHost, e->stream));
    SCL_HIP(e, hipMemcpyAsync(d2, e->d_topk_d2, sizeof(float) * k, hipMemcpyDeviceToHost, e->stream));
    return sync(e);
}

/* ---- index map (dump / load: ingest_host.hip) --------------------------------------- */

int scl_find_key(const scl_engine *e, int8_t robot, int index, int *key)
{
    if (!e || !key) return SCL_ERR_INVALID_ARG;
    *key = -1;
    const int n = scl_get_size(e, -1);
    if (n < 0) return n;
    // newest first: the callers of DM.h:1281-1284 ask about recent keyframes
    for (int k = n - 1; k >= 0; --k) {
        int8_t r = 0; int idx = 0;
        const int rc = scl_get_index(e, k, &r, &idx);
        if (rc) return rc;
        if (r == robot && idx == index) { *key = k; break; }
    }
    return SCL_OK;
}

/* ---- pose algebra behind the ICP block (DM.h:1130-1141, 1249-1259) ------------------------ */

int scl_matrix_to_pose(const float T[16], float *x, float *y, float *z, float *roll, float *pitch, float *yaw)
{
    if (!T || !x || !y || !z || !roll || !pitch || !yaw) return SCL_ERR_INVALID_ARG;
    *x = T[3]; *y = T[7]; *z = T[11];                       /* pcl::getTranslationAndEulerAngles, float like the reference */
    *roll = std::atan2(T[9], T[10]);
    *pitch = std::asin(-T[8]);
    *yaw = std::atan2(T[4], T[0]);
    return SCL_OK;
}

int scl_loop_pose_between(const float T_icp[16], const float pose_cur[6], const float pose_pre[6], double between_xyz_q[7], double between_rpy[3])
{
    if (!T_icp || !pose_cur || !pose_pre || !between_xyz_q) return SCL_ERR_INVALID_ARG;
    float Tw[16], Tc[16];
    scl_pose_to_matrix(pose_cur[0], pose_cur[1], pose_cur[2], pose_cur[3], pose_cur[4], pose_cur[5], Tw);   /* tfWrong, DM.h:1137 */
    for (int r = 0; r < 4; ++r)                                                                              /* tfCorrect = tfICP * tfWrong (Affine3f), DM.h:1138 */
        for (int c = 0; c < 4; ++c) {
            float s = 0.0f;
            for (int k = 0; k < 4; ++k) s += T_icp[4 * r + k] * Tw[4 * k + c];
            Tc[4 * r + c] = s;
        }
    float x, y, z, roll, pitch, yaw;
    scl_matrix_to_pose(Tc, &x, &y, &z, &roll, &pitch, &yaw);                                                 /* DM.h:1139 */
    auto rzryrx = [](double ro, double pi, double ya, double R[9]) {                                         /* gtsam::Rot3::RzRyRx */
        const double cr = std::cos(ro), sr = std::sin(ro), cp = std::cos(pi), sp = std::sin(pi), cy = std::cos(ya), sy = std::sin(ya);
        R[0] = cy * cp; R[1] = cy * sp * sr - sy * cr; R[2] = cy * sp * cr + sy * sr;
        R[3] = sy * cp; R[4] = sy * sp * sr + cy * cr; R[5] = sy * sp * cr - cy * sr;
        R[6] = -sp;     R[7] = cp * sr;                R[8] = cp * cr;
    };
    double Rf[9], Rt[9];
    rzryrx((double)roll, (double)pitch, (double)yaw, Rf);                                                    /* poseFrom, DM.h:1140 */
    rzryrx((double)pose_pre[3], (double)pose_pre[4], (double)pose_pre[5], Rt);                               /* poseTo, DM.h:1141 + 214-218 */
    const double tf[3] = {(double)x, (double)y, (double)z}, tt[3] = {(double)pose_pre[0], (double)pose_pre[1], (double)pose_pre[2]};
    double Rb[9], tb[3];                                                                                     /* poseFrom.between(poseTo) = poseFrom^-1 * poseTo */
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) { double s = 0; for (int k = 0; k < 3; ++k) s += Rf[3 * k + r] * Rt[3 * k + c]; Rb[3 * r + c] = s; }
        double s = 0; for (int k = 0; k < 3; ++k) s += Rf[3 * k + r] * (tt[k] - tf[k]);
        tb[r] = s;
    }
    between_xyz_q[0] = tb[0]; between_xyz_q[1] = tb[1]; between_xyz_q[2] = tb[2];
    // rotation matrix -> unit quaternion with w >= 0 (q and -q are the same rotation; the sign GTSAM / Eigen pick is not pinned)
    double qw, qx, qy, qz;
    const double tr = Rb[0] + Rb[4] + Rb[8];
    if (tr > 0) { const double s = std::sqrt(tr + 1.0) * 2; qw = 0.25 * s; qx = (Rb[7] - Rb[5]) / s; qy = (Rb[2] - Rb[6]) / s; qz = (Rb[3] - Rb[1]) / s; }
    else if (Rb[0] > Rb[4] && Rb[0] > Rb[8]) { const double s = std::sqrt(1.0 + Rb[0] - Rb[4] - Rb[8]) * 2; qw = (Rb[7] - Rb[5]) / s; qx = 0.25 * s; qy = (Rb[1] + Rb[3]) / s; qz = (Rb[2] + Rb[6]) / s; }
    else if (Rb[4] > Rb[8]) { const double s = std::sqrt(1.0 + Rb[4] - Rb[0] - Rb[8]) * 2; qw = (Rb[2] - Rb[6]) / s; qx = (Rb[1] + Rb[3]) / s; qy = 0.25 * s; qz = (Rb[5] + Rb[7]) / s; }
    else { const double s = std::sqrt(1.0 + Rb[8] - Rb[0] - Rb[4]) * 2; qw = (Rb[3] - Rb[1]) / s; qx = (Rb[2] + Rb[6]) / s; qy = (Rb[5] + Rb[7]) / s; qz = 0.25 * s; }
    if (qw < 0) { qw = -qw; qx = -qx; qy = -qy; qz = -qz; }
    between_xyz_q[3] = qx; between_xyz_q[4] = qy; between_xyz_q[5] = qz; between_xyz_q[6] = qw;
    if (between_rpy) {                                                                                       /* Rot3::roll/pitch/yaw (DM.h:1258) */
        between_rpy[0] = std::atan2(Rb[7], Rb[8]);
        between_rpy[1] = std::asin(-Rb[6] > 1 ? 1 : (-Rb[6] < -1 ? -1 : -Rb[6]));
        between_rpy[2] = std::atan2(Rb[3], Rb[0]);
    }
    return SCL_OK;
}

/* ---- pairwise consistency of loop closures: matrix, graph, max clique (pcm.hip) ------ */

namespace {

// scl_pcm_consistency (members == nullptr) and scl_pcm_select
int pcm_call(scl_engine *e, const PcmInputs &in, double *d2, uint64_t *adj, int *degree, int *members, int *n_members, int *seed, bool select)
{
    if (!e) return SCL_ERR_INVALID_ARG;
    if (e->front) {                                        // the primary shard does the work; its message goes to the handle the caller holds
        scl_engine *front = e;
        const int rc = pcm_call(front_primary(e), in, d2, adj, degree, members, n_members, seed, select);
        if (rc) front->last_error = scl_last_error(front_primary(front));
        return rc;
    }
    std::lock_guard<std::mutex> lk(e->mu);
    const std::string name = select ? "pcm_select: " : "pcm_consistency: ";
    if (const char *bad = pcm_inputs_bad(in)) return fail(e, SCL_ERR_INVALID_ARG, (name + bad).c_str());
    if (select && (!n_members || !seed || (in.n_loops > 0 && !members))) return fail(e, SCL_ERR_INVALID_ARG, (name + "members, n_members or seed is NULL").c_str());
    if (!select && in.n_loops > 0 && !d2 && !adj && !degree) return fail(e, SCL_ERR_INVALID_ARG, (name + "no output given").c_str());
    if (in.n_loops == 0) {
        if (select) { *n_members = 0; *seed = -1; }
        return SCL_OK;
    }
    (void)hipSetDevice(e->device);
    std::string err;
    const int rc = pcm_consistency(&e->pcm_ws, e->stream, in, d2, adj, degree, select ? members : nullptr, n_members, seed, e->prof_on == 1, &err);
    if (rc) e->last_error = err;
    return rc;
}

}  // namespace

int scl_pcm_consistency(scl_engine *e, const double *poses_a, int n_a, const double *poses_b, int n_b,
                        const int *idx_a, const int *idx_b, const double *z, const double *cov, int n_loops,
                        const double *odom_var, double threshold, double *d2, uint64_t *adj, int *degree)
{
    const PcmInputs in = {poses_a, n_a, poses_b, n_b, idx_a, idx_b, z, cov, n_loops, odom_var, threshold};
    return pcm_call(e, in, d2, adj, degree, nullptr, nullptr, nullptr, false);
}

int scl_pcm_select(scl_engine *e, const double *poses_a, int n_a, const double *poses_b, int n_b,
                   const int *idx_a, const int *idx_b, const double *z, const double *cov, int n_loops,
                   const double *odom_var, double threshold, int *members, int *n_members, int *seed, int *degree)
{
    const PcmInputs in = {poses_a, n_a, poses_b, n_b, idx_a, idx_b, z, cov, n_loops, odom_var, threshold};
    return pcm_call(e, in, nullptr, nullptr, degree, members, n_members, seed, true);
}

int scl_pcm_max_clique(scl_engine *e, const uint64_t *adj, int n, int *members, int *n_members, int *seed)
{
    if (!e) return SCL_ERR_INVALID_ARG;
    if (e->front) {
        const int rc = scl_pcm_max_clique(front_primary(e), adj, n, members, n_members, seed);
        if (rc) e->last_error = scl_last_error(front_primary(e));
        return rc;
    }
    std::lock_guard<std::mutex> lk(e->mu);
    if (!n_members || !seed || (n > 0 && !members)) return fail(e, SCL_ERR_INVALID_ARG, "pcm_max_clique: members, n_members or seed is NULL");
    if (const char *bad = pcm_graph_bad(adj, n)) return fail(e, SCL_ERR_INVALID_ARG, (std::string("pcm_max_clique: ") + bad).c_str());
    if (n == 0) { *n_members = 0; *seed = -1; return SCL_OK; }
    (void)hipSetDevice(e->device);
    std::string err;
    const int rc = pcm_max_clique(&e->pcm_ws, e->stream, adj, n, members, n_members, seed, e->prof_on == 1, &err);
    if (rc) e->last_error = err;
    return rc;
}

int scl_pcm_last_timing(scl_engine *e, double *pairs_ms, double *clique_ms)
{
    if (!e) return SCL_ERR_INVALID_ARG;
    if (e->front) e = front_primary(e);
    std::lock_guard<std::mutex> lk(e->mu);
    if (pairs_ms) *pairs_ms = e->pcm_ws.pairs_ms;
    if (clique_ms) *clique_ms = e->pcm_ws.clique_ms;
    return SCL_OK;
}

int scl_loop_covariance(const double info[36], double s2, double cov[36])
{
    if (!info || !cov || !(s2 > 0.0) || !std::isfinite(s2)) return SCL_ERR_INVALID_ARG;
    for (int k = 0; k < 36; ++k) if (!std::isfinite(info[k])) return SCL_ERR_INVALID_ARG;
    // info = L L^T from the upper triangle; a column that depends on the ones before it leaves a pivot of rounding's size
    double L[6][6] = {{0.0}};
    for (int c = 0; c < 6; ++c) {
        double s = info[6 * c + c];
        for (int k = 0; k < c; ++k) s -= L[c][k] * L[c][k];
        if (!(s > std::ldexp(info[6 * c + c], -43))) return SCL_ERR_INVALID_ARG;
        L[c][c] = std::sqrt(s);
        for (int r = c + 1; r < 6; ++r) {
            double v = info[6 * c + r];
            for (int k = 0; k < c; ++k) v -= L[r][k] * L[c][k];
            L[r][c] = v / L[c][c];
        }
    }
    // Y = L^-1 (lower triangular, column by column), info^-1 = Y^T Y
    double Y[6][6] = {{0.0}};
    for (int c = 0; c < 6; ++c)
        for (int r = c; r < 6; ++r) {
            double v = r == c ? 1.0 : 0.0;
            for (int k = c; k < r; ++k) v -= L[r][k] * Y[k][c];
            Y[r][c] = v / L[r][r];
        }
    double out[36];
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) {
            double v = 0.0;
            for (int k = b; k < 6; ++k) v += Y[k][a] * Y[k][b];
            out[6 * a + b] = out[6 * b + a] = s2 * v;
        }
    for (int k = 0; k < 36; ++k) if (!std::isfinite(out[k])) return SCL_ERR_INVALID_ARG;
    std::memcpy(cov, out, sizeof out);
    return SCL_OK;
}

/* ---- pose-graph solve: SE(3) between factors and priors, LM with block PCG (pgo.hip) ------ */

namespace {

// what = 0 scl_pgo_linearize (a, b, c, d = cost, gradient, diag, chi2), 1 scl_pgo_hessian_apply (a = x, b = y), 2 scl_pgo_optimize
// (b = poses_out, d = chi2), 3 scl_pgo_solve_condensed (b = delta), 4 scl_pgo_optimize_condensed (as 2, and failed), 5
// scl_pgo_solve_condensed_many (a_in = rhs, b = x, count = n_rhs), 6 scl_pgo_marginals (q_i, q_j, count = n_queries, a = blocks, b = rel)
int pgo_call(scl_engine *e, const PgoInputs &in, int what, double lambda, const scl_pgo_params *params, scl_pgo_result *result,
             const double *a_in, double *a, double *b, double *c, double *d, int *failed = nullptr, int count = 0, const int *q_i = nullptr,
             const int *q_j = nullptr)
{
    if (!e) return SCL_ERR_INVALID_ARG;
    if (e->front) {                                        // the primary shard does the work; its message goes to the handle the caller holds
        scl_engine *front = e;
        const int rc = pgo_call(front_primary(e), in, what, lambda, params, result, a_in, a, b, c, d, failed, count, q_i, q_j);
        if (rc) front->last_error = scl_last_error(front_primary(front));
        return rc;
    }
    std::lock_guard<std::mutex> lk(e->mu);
    static const char *const names[7] = {"pgo_linearize: ", "pgo_hessian_apply: ", "pgo_optimize: ", "pgo_solve_condensed: ", "pgo_optimize_condensed: ",
                                         "pgo_solve_condensed_many: ", "pgo_marginals: "};
    const std::string name = names[what];
    if (const char *bad = pgo_inputs_bad(in)) return fail(e, SCL_ERR_INVALID_ARG, (name + bad).c_str());
    scl_pgo_params prm;
    pgo_default_params(&prm);
    if (what == 0 && !a && !b && !c && !d) return fail(e, SCL_ERR_INVALID_ARG, (name + "no output given").c_str());
    if (what == 1) {
        if (!a_in || !b) return fail(e, SCL_ERR_INVALID_ARG, (name + "x or y is NULL").c_str());
        if (!std::isfinite(lambda) || lambda < 0.0) return fail(e, SCL_ERR_INVALID_ARG, (name + "lambda non-finite or negative").c_str());
        for (size_t k = 0; k < 6 * (size_t)in.n_poses; ++k)
            if (!std::isfinite(a_in[k])) return fail(e, SCL_ERR_INVALID_ARG, (name + "a non-finite x").c_str());
    }
    if (what == 3) {
        if (!b) return fail(e, SCL_ERR_INVALID_ARG, (name + "delta is NULL").c_str());
        if (!std::isfinite(lambda) || lambda < 0.0) return fail(e, SCL_ERR_INVALID_ARG, (name + "lambda non-finite or negative").c_str());
    }
    if (what == 2 || what == 4) {
        if (!b || !result) return fail(e, SCL_ERR_INVALID_ARG, (name + "poses_out or result is NULL").c_str());
        if (params) prm = *params;
        if (const char *bad = pgo_params_bad(prm)) return fail(e, SCL_ERR_INVALID_ARG, (name + bad).c_str());
    }
    if (what == 5) {
        if (!a_in || !b) return fail(e, SCL_ERR_INVALID_ARG, (name + "rhs or x is NULL").c_str());
        if (!std::isfinite(lambda) || lambda < 0.0) return fail(e, SCL_ERR_INVALID_ARG, (name + "lambda non-finite or negative").c_str());
        if (count < 1 || count > SCL_PGO_MAX_RHS) return fail(e, SCL_ERR_INVALID_ARG, (name + "n_rhs < 1 or > 1536").c_str());
        for (size_t k = 0; k < 6 * (size_t)in.n_poses * (size_t)count; ++k)
            if (!std::isfinite(a_in[k])) return fail(e, SCL_ERR_INVALID_ARG, (name + "a non-finite rhs").c_str());
    }
    if (what == 6) {
        if (!a && !b) return fail(e, SCL_ERR_INVALID_ARG, (name + "no output given").c_str());
        if (count < 1 || count > SCL_PGO_MAX_MARGINAL_QUERIES) return fail(e, SCL_ERR_INVALID_ARG, (name + "n_queries < 1 or > 4096").c_str());
        std::vector<int> sel, ui, uj;
        if (const char *bad = pgo_marginal_select(q_i, q_j, count, in.n_poses, &sel, &ui, &uj)) return fail(e, SCL_ERR_INVALID_ARG, (name + bad).c_str());
    }
    if (what >= 3)
        if (const char *bad = pgo_condensed_bad(in)) return fail(e, SCL_ERR_INVALID_ARG, (name + bad).c_str());
    (void)hipSetDevice(e->device);
    std::string err;
    const bool timing = e->prof_on == 1;
    const int rc = what == 5 ? pgo_solve_condensed_many(&e->pgo_ws, e->stream, in, lambda, a_in, count, b, timing, &err)
                 : what == 6 ? pgo_marginals(&e->pgo_ws, e->stream, in, q_i, q_j, count, a, b, timing, &err)
                 : what == 3 ? pgo_solve_condensed(&e->pgo_ws, e->stream, in, lambda, b, timing, &err)
                 : what == 4 ? pgo_optimize_condensed(&e->pgo_ws, e->stream, in, prm, b, result, d, failed, timing, &err)
                 : what == 0 ? pgo_linearize(&e->pgo_ws, e->stream, in, a, b, c, d, timing, &err)
                 : what == 1 ? pgo_hessian_apply(&e->pgo_ws, e->stream, in, lambda, a_in, b, timing, &err)
                             : pgo_optimize(&e->pgo_ws, e->stream, in, prm, b, result, d, timing, &err);
    if (rc) e->last_error = err;
    return rc;
}

}  // namespace

int scl_pgo_default_params(scl_pgo_params *p)
{
    if (!p) return SCL_ERR_INVALID_ARG;
    pgo_default_params(p);
    return SCL_OK;
}

int scl_pgo_linearize(scl_engine *e, const double *poses, int n_poses,
                      const int *f_i, const int *f_j, const double *f_z, const double *f_cov, int n_factors,
                      const int *p_idx, const double *p_z, const double *p_cov, int n_priors,
                      double *cost, double *gradient, double *diag, double *chi2)
{
    const PgoInputs in = {poses, n_poses, f_i, f_j, f_z, f_cov, n_factors, p_idx, p_z, p_cov, n_priors};
    return pgo_call(e, in, 0, 0.0, nullptr, nullptr, nullptr, cost, gradient, diag, chi2);
}

int scl_pgo_hessian_apply(scl_engine *e, const double *poses, int n_poses,
                          const int *f_i, const int *f_j, const double *f_z, const double *f_cov, int n_factors,
                          const int *p_idx, const double *p_z, const double *p_cov, int n_priors,
                          double lambda, const double *x, double *y)
{
    const PgoInputs in = {poses, n_poses, f_i, f_j, f_z, f_cov, n_factors, p_idx, p_z, p_cov, n_priors};
    return pgo_call(e, in, 1, lambda, nullptr, nullptr, x, nullptr, y, nullptr, nullptr);
}

int scl_pgo_optimize(scl_engine *e, const double *poses, int n_poses,
                     const int *f_i, const int *f_j, const double *f_z, const double *f_cov, int n_factors,
                     const int *p_idx, const double *p_z, const double *p_cov, int n_priors,
                     const scl_pgo_params *params, double *poses_out, scl_pgo_result *result, double *chi2)
{
    const PgoInputs in = {poses, n_poses, f_i, f_j, f_z, f_cov, n_factors, p_idx, p_z, p_cov, n_priors};
    return pgo_call(e, in, 2, 0.0, params, result, nullptr, nullptr, poses_out, nullptr, chi2);
}

int scl_pgo_count_junctions(int n_poses, const int *f_i, const int *f_j, int n_factors, const int *p_idx, int n_priors,
                            int *n_junctions, int *n_segments, int *longest_segment)
{
    if (n_poses < 1 || n_factors < 0 || n_priors < 0 || (n_factors > 0 && (!f_i || !f_j)) || (n_priors > 0 && !p_idx)) return SCL_ERR_INVALID_ARG;
    for (int k = 0; k < n_factors; ++k)
        if (f_i[k] < 0 || f_i[k] >= n_poses || f_j[k] < 0 || f_j[k] >= n_poses) return SCL_ERR_INVALID_ARG;
    for (int m = 0; m < n_priors; ++m)
        if (p_idx[m] < 0 || p_idx[m] >= n_poses) return SCL_ERR_INVALID_ARG;
    int nj = 0, ns = 0, longest = 0;
    pgo_count_junctions(n_poses, f_i, f_j, n_factors, p_idx, n_priors, &nj, &ns, &longest);
    if (n_junctions) *n_junctions = nj;
    if (n_segments) *n_segments = ns;
    if (longest_segment) *longest_segment = longest;
    return SCL_OK;
}

int scl_pgo_solve_condensed(scl_engine *e, const double *poses, int n_poses,
                            const int *f_i, const int *f_j, const double *f_z, const double *f_cov, int n_factors,
                            const int *p_idx, const double *p_z, const double *p_cov, int n_priors,
                            double lambda, double *delta)
{
    const PgoInputs in = {poses, n_poses, f_i, f_j, f_z, f_cov, n_factors, p_idx, p_z, p_cov, n_priors};
    return pgo_call(e, in, 3, lambda, nullptr, nullptr, nullptr, nullptr, delta, nullptr, nullptr);
}

int scl_pgo_optimize_condensed(scl_engine *e, const double *poses, int n_poses,
                               const int *f_i, const int *f_j, const double *f_z, const double *f_cov, int n_factors,
                               const int *p_idx, const double *p_z, const double *p_cov, int n_priors,
                               const scl_pgo_params *params, double *poses_out, scl_pgo_result *result, double *chi2,
                               int *failed_factorisations)
{
    const PgoInputs in = {poses, n_poses, f_i, f_j, f_z, f_cov, n_factors, p_idx, p_z, p_cov, n_priors};
    return pgo_call(e, in, 4, 0.0, params, result, nullptr, nullptr, poses_out, nullptr, chi2, failed_factorisations);
}

int scl_pgo_solve_condensed_many(scl_engine *e, const double *poses, int n_poses,
                                 const int *f_i, const int *f_j, const double *f_z, const double *f_cov, int n_factors,
                                 const int *p_idx, const double *p_z, const double *p_cov, int n_priors,
                                 double lambda, const double *rhs, int n_rhs, double *x)
{
    const PgoInputs in = {poses, n_poses, f_i, f_j, f_z, f_cov, n_factors, p_idx, p_z, p_cov, n_priors};
    return pgo_call(e, in, 5, lambda, nullptr, nullptr, rhs, nullptr, x, nullptr, nullptr, nullptr, n_rhs);
}

int scl_pgo_marginals(scl_engine *e, const double *poses, int n_poses,
                      const int *f_i, const int *f_j, const double *f_z, const double *f_cov, int n_factors,
                      const int *p_idx, const double *p_z, const double *p_cov, int n_priors,
                      const int *q_i, const int *q_j, int n_queries, double *blocks, double *rel)
{
    const PgoInputs in = {poses, n_poses, f_i, f_j, f_z, f_cov, n_factors, p_idx, p_z, p_cov, n_priors};
    return pgo_call(e, in, 6, 0.0, nullptr, nullptr, nullptr, blocks, rel, nullptr, nullptr, nullptr, n_queries, q_i, q_j);
}

int scl_pgo_condensed_last_timing(scl_engine *e, double ms[4])
{
    if (!e || !ms) return SCL_ERR_INVALID_ARG;
    if (e->front) e = front_primary(e);
    std::lock_guard<std::mutex> lk(e->mu);
    for (int k = 0; k < 4; ++k) ms[k] = e->pgo_ws.condensed_ms[k];
    return SCL_OK;
}

int scl_pgo_last_timing(scl_engine *e, double *linearize_ms, double *solve_ms)
{
    if (!e) return SCL_ERR_INVALID_ARG;
    if (e->front) e = front_primary(e);
    std::lock_guard<std::mutex> lk(e->mu);
    if (linearize_ms) *linearize_ms = e->pgo_ws.linearize_ms;
    if (solve_ms) *solve_ms = e->pgo_ws.solve_ms;
    return SCL_OK;
}

/* ---- measurement ------------------------------------------------------------- */

int scl_profile_enable(scl_engine *e, int on)
{
    if (!e) return SCL_ERR_INVALID_ARG;
    if (e->front) return front_profile_enable(e, on);
    std::lock_guard<std::mutex> lk(e->mu);
    e->prof_on = on < 0 ? 0 : (on > 3 ? 1 : on);
    e->prof_tick = 0;
    return SCL_OK;
}

int scl_profile_reset(scl_engine *e)
{
    if (!e) return SCL_ERR_INVALID_ARG;
    if (e->front) return front_profile_reset(e);
    std::lock_guard<std::mutex> lk(e->mu);
    std::memset(&e->prof, 0, sizeof e->prof);
    return SCL_OK;
}

int scl_profile_get(scl_engine *e, scl_profile *out)
{
    if (!e || !out) return SCL_ERR_INVALID_ARG;
    if (e->front) return front_profile_get(e, out);
    std::lock_guard<std::mutex> lk(e->mu);
    *out = e->prof;
    return SCL_OK;
}

int scl_alignment_stats(scl_engine *e, uint64_t *pairs, uint64_t *fallbacks, int reset)
{
    if (!e) return SCL_ERR_INVALID_ARG;
    if (e->front) return front_alignment_stats(e, pairs, fallbacks, reset);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    unsigned long long f = 0;
    SCL_HIP(e, hipStreamSynchronize(e->stream));
    SCL_HIP(e, hipMemcpy(&f, e->d_align_fallbacks, sizeof f, hipMemcpyDeviceToHost));
    if (pairs) *pairs = e->align_pairs;
    if (fallbacks) *fallbacks = (uint64_t)f;
    if (reset) {
        SCL_HIP(e, hipMemset(e->d_align_fallbacks, 0, sizeof f));
        e->align_pairs = 0;
    }
    return SCL_OK;
}

int scl_survivor_stats(scl_engine *e, uint64_t *queries, uint64_t *survivors, uint64_t *max_survivors, int reset)
{
    if (!e) return SCL_ERR_INVALID_ARG;
    if (e->front) return front_survivor_stats(e, queries, survivors, max_survivors, reset);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    unsigned long long s[3] = {0, 0, 0};
    SCL_HIP(e, hipStreamSynchronize(e->stream));
    if (e->stream_surv) SCL_HIP(e, hipStreamSynchronize(e->stream_surv));
    SCL_HIP(e, hipMemcpy(s, e->d_surv_stats, sizeof s, hipMemcpyDeviceToHost));
    if (survivors) *survivors = (uint64_t)s[0];
    if (max_survivors) *max_survivors = (uint64_t)s[1];
    if (queries) *queries = (uint64_t)s[2];
    if (reset) SCL_HIP(e, hipMemset(e->d_surv_stats, 0, sizeof s));
    return SCL_OK;
}

int scl_device_name(const scl_engine *e, char *buf, int buflen)
{
    if (!e || !buf || buflen <= 0) return SCL_ERR_INVALID_ARG;
    if (e->front) e = front_primary(e);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, e->device) != hipSuccess) return SCL_ERR_HIP;
    std::snprintf(buf, (size_t)buflen, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return SCL_OK;
}

}  // extern "C"

// ---- hooks for the sharded front (engine_internal.hpp) ---------------------------------------------------------
namespace scl {

int eng_topk_enqueue(scl_engine *e, int query, int lo, int hi, int k, float eps, bool want_dist, bool *have_dist)
{
    std::lock_guard<std::mutex> pk(e->pass_mu);            // pass state (pinned results, slots, buffer sets): pass_mu first, like every scoring entry point
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    return topk_enqueue_locked(e, query, lo, hi, k, eps, want_dist, have_dist);
}

int eng_topk_finish(scl_engine *e, int k, bool have_dist, int *idx, float *d2, double *dist, int *shift, int *found)
{
    std::lock_guard<std::mutex> pk(e->pass_mu);            // pass state (pinned results, slots, buffer sets): pass_mu first, like every scoring entry point
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    return topk_finish_locked(e, k, have_dist, idx, d2, dist, shift, found);
}

int eng_sync_streams(scl_engine *e)
{
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    SCL_HIP(e, hipStreamSynchronize(e->stream));
    if (e->stream_alt) SCL_HIP(e, hipStreamSynchronize(e->stream_alt));
    if (e->stream2) SCL_HIP(e, hipStreamSynchronize(e->stream2));
    return SCL_OK;
}

int eng_sc_search_ruled(scl_engine *e, const int *queries, const int *lo, const int *hi, const ScRankRule *rules, int n_queries, int k,
                        int *cand_ids, int *cand_shifts, double *cand_dists, int *n_found)
{
    if (!e || e->front || n_queries < 0 || k < 1 || k > SCL_SC_SEARCH_MAX || (n_queries > 0 && (!queries || !lo || !hi || !rules || !cand_ids)))
        return SCL_ERR_INVALID_ARG;
    if (n_queries == 0) return SCL_OK;
    std::lock_guard<std::mutex> pk(e->pass_mu);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    return sc_search_locked(e, queries, lo, hi, n_queries, k, cand_ids, cand_shifts, cand_dists, n_found, rules);
}

const double *eng_ticket_record(const scl_engine *e, int ticket, int *slot_lo, bool *empty)
{
    std::lock_guard<std::mutex> pk(e->pass_mu);
    std::lock_guard<std::mutex> lk(e->mu);
    if (ticket < 0 || ticket >= scl_engine::kSlots || !e->slot_busy[ticket]) return nullptr;
    *slot_lo = e->slot_lo[ticket];
    *empty = e->slot_empty[ticket];
    return e->h_out3 + (size_t)ticket * 8;
}

hipStream_t eng_stream(const scl_engine *e) { return e->stream; }

int eng_release_ticket(scl_engine *e, int ticket)
{
    std::lock_guard<std::mutex> pk(e->pass_mu);            // pass state (pinned results, slots, buffer sets): pass_mu first, like every scoring entry point
    std::lock_guard<std::mutex> lk(e->mu);
    if (ticket < 0 || ticket >= scl_engine::kSlots || !e->slot_busy[ticket]) return fail(e, SCL_ERR_INVALID_ARG, "unknown ticket");
    e->slot_busy[ticket] = false;
    collect_profile(e);
    return SCL_OK;
}

}  // namespace scl
