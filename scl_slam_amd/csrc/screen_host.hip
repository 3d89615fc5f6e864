// screen_host.hip -- host side of the SCREENED search (kernels: sc_screen.hip, sc_masked.hip, sc_matrix.hip): the full-database
// detection in its blocking, ticket (submit / collect) and stream forms with their C entry points, the screened distance matrix's group
// loop, and scl_screen_distances*.  No kernel lives here.  The engine object, its locks and what this file takes from engine.hip (the
// profile's scope, the buffer sets, the views of the database and of a query) are engine_internal.hpp's; the stream's launch SCHEDULE --
// pairs, who aligns whom, the wait for the other half -- is screen_plan.hpp's, a pure function that tests/cpp/screen_plan_check.cpp
// checks without a GPU.  submit_full_locked also carries the one-query pass of the grids WITHOUT a screening pass: it is the other
// branch of the same ticket.  The matrix's consumers (MatrixToHost, RankGroups) stay in engine.hip with the entry points that make
// them: the plain loop feeds them as well, and only the MatrixConsumer interface crosses the files.
#include "scl_engine.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "engine_internal.hpp"
#include "plugin_host.hpp"
#include "screen_plan.hpp"

using namespace scl;

namespace {

// enqueue one full-DB pass; results land in pinned slot `sl` when ev_done[sl] has fired
int submit_full_many_locked(scl_engine *e, const int *queries, const int *los, const int *his, int nq, int *tickets);

// ---- screened full-DB passes (64x120 grid; sc_screen.hip) --------------------------------------------------------
// The engine-owned pointers of a ScreenBatch (the queries, their ranges and buffer sets, pair_stride and no_ring_metric are the
// caller's).  lists: the batch goes through a select launch, which writes the survivor lists and their counts
void screen_batch_pointers(const scl_engine *e, ScreenBatch &sb, bool lists, unsigned long long *surv_stats, unsigned int *smask, float *part)
{
    sb.approx = e->d_approx; sb.starts = e->d_starts; sb.align_fallbacks = e->d_align_fallbacks; sb.ring_d2 = e->d_ring_d2;
    sb.survivors = lists ? e->d_surv : nullptr; sb.n_surv = lists ? e->d_nsurv : nullptr; sb.t_min = e->d_tmin; sb.surv_stats = surv_stats;
    sb.smask = smask; sb.part = part;
    sb.k = e->cfg.num_candidates; sb.exclude_eps = e->cfg.knn_exclude_eps; sb.topk_idx = e->d_topk_idx; sb.topk_d2 = e->d_topk_d2;
}

// One screening launch group: queries qslot[0..nq) against [lo[i], lo[i] + n[i]), buffer sets set0 + i.
struct ScreenGroup { const int *qslot, *lo, *n; int nq, set0; int part_half = 0; bool masks = false; bool keys_later = false; };   // part_half: which half of d_part holds the batch's partial sums;
                                                                                                             // masks: the batch's exact pass evaluates the open shifts only (the shift masks are formed and written)
                                                                                                             // keys_later: ScreenBatch::no_ring_metric
void fill_screen_batch(scl_engine *e, ScreenBatch &sb, const ScreenGroup &g)
{
    sb.nq = g.nq;
    for (int j = 0; j < g.nq; ++j) { sb.slot[j] = g.qslot[j]; sb.base[j] = g.lo[j]; sb.n[j] = g.n[j]; sb.buf[j] = g.set0 + j; }
    sb.pair_stride = e->set_stride;
    screen_batch_pointers(e, sb, false, nullptr,
                          (g.masks || sc_screen_is_wide(db_view(e), e->SR)) ? e->d_smask : nullptr,   // (the 64 x 120 stream's exact pass scores all 13 shifts of its few survivors: no masks)
                          e->d_part + (g.part_half ? e->part_cap / 2 : 0));
    sb.no_ring_metric = g.keys_later;
}

// next (optional, nq > 0): the launch that will follow; its alignment rides in this one (the next call then passes
// kScreenProducts only).
int launch_screen_group(scl_engine *e, const ScreenGroup &cur, int phases = kScreenAlign | kScreenProducts,
                        const ScreenGroup *next = nullptr, hipStream_t stream = nullptr)
{
    if (!stream) stream = e->stream;
    ScreenBatch sb{}, nx{};
    fill_screen_batch(e, sb, cur);
    const bool has_next = next && next->nq > 0;
    if (has_next) fill_screen_batch(e, nx, *next);
    if (phases & kScreenAlign) for (int j = 0; j < cur.nq; ++j) e->align_pairs += (uint64_t)cur.n[j];
    if (has_next) for (int j = 0; j < next->nq; ++j) e->align_pairs += (uint64_t)next->n[j];
    if ((phases & kScreenAlign) && (phases & kScreenProducts) && has_next) {   // a sequence's first launch: its own alignment outside the
        SCL_HIP(e, launch_sc_screen_batch(db_view(e), sb, e->SR, sc_align_filter_enabled(), e->num_cu, stream, kScreenAlign, nullptr));   // event pair
        phases = kScreenProducts;
    }
    ProfScope ps(e, P_SC, stream);
    SCL_HIP(e, launch_sc_screen_batch(db_view(e), sb, e->SR, sc_align_filter_enabled(), e->num_cu, stream, phases, has_next ? &nx : nullptr));
    if (ps.active()) { for (int j = 0; j < cur.nq; ++j) e->prof.sc_distance_pairs += (uint64_t)cur.n[j]; }
    return SCL_OK;
}

// Two consecutive full launch groups of the stream form as ONE products launch (sc_screen.hip: two scan sets share the pass over the
// database), each with its own tail.  g0 / g1 use the two halves of d_part.  align0 / align1: the group aligns for itself (no tail did it);
// next0 / next1 (optional, nq > 0): the groups whose alignment rides in the tails of g0 / g1.  One entry of the profile.
int launch_screen_pair_group(scl_engine *e, ScreenGroup g0, ScreenGroup g1, bool align0, bool align1, const ScreenGroup *next0, const ScreenGroup *next1)
{
    hipStream_t stream = e->stream;
    g0.part_half = 0; g1.part_half = 1;
    ScreenBatch sb0{}, sb1{}, nx0{}, nx1{};
    fill_screen_batch(e, sb0, g0);
    fill_screen_batch(e, sb1, g1);
    const bool has0 = next0 && next0->nq > 0, has1 = next1 && next1->nq > 0;
    if (has0) fill_screen_batch(e, nx0, *next0);
    if (has1) fill_screen_batch(e, nx1, *next1);
    const ScreenGroup *counted[4] = {align0 ? &g0 : nullptr, align1 ? &g1 : nullptr, has0 ? next0 : nullptr, has1 ? next1 : nullptr};
    for (const ScreenGroup *g : counted)
        if (g) for (int j = 0; j < g->nq; ++j) e->align_pairs += (uint64_t)g->n[j];
    // (a sequence's first pair, or a pair behind a single group: the alignment of its own outside the event pair)
    if (align0) SCL_HIP(e, launch_sc_screen_batch(db_view(e), sb0, e->SR, sc_align_filter_enabled(), e->num_cu, stream, kScreenAlign, nullptr));
    if (align1) SCL_HIP(e, launch_sc_screen_batch(db_view(e), sb1, e->SR, sc_align_filter_enabled(), e->num_cu, stream, kScreenAlign, nullptr));
    ProfScope ps(e, P_SC, stream);
    SCL_HIP(e, launch_sc_screen_pair(db_view(e), sb0, sb1, e->SR, sc_align_filter_enabled(), e->num_cu, stream, has0 ? &nx0 : nullptr, has1 ? &nx1 : nullptr));
    if (ps.active()) { for (int j = 0; j < g0.nq; ++j) e->prof.sc_distance_pairs += (uint64_t)g0.n[j] + (uint64_t)g1.n[j]; }
    return SCL_OK;
}

// The exact pass over the survivors of nq screened queries (buffer sets set0 .. set0 + nq - 1); winners to out3[i].
// phases / region: see launch_sc_distance_survivors; a caller that splits the pass passes the same region (from
// survivor_arg_region) to both halves
unsigned survivor_arg_region(scl_engine *e) { return e->surv_arg_tick++ & 7u; }
int launch_survivor_pass(scl_engine *e, const int *qslot, const int *lo, const int *n, int nq, int set0, double *const *out3, hipStream_t stream = nullptr,
                         int phases = kSurvivorArgs | kSurvivorKernel, int region_in = -1, bool ring_from_keys = false)
{
    if (!stream) stream = e->stream;
    SurvivorPass sp{};
    sp.nq = nq; sp.ring_from_keys = ring_from_keys ? 1 : 0;
    for (int j = 0; j < nq; ++j) { sp.slot[j] = qslot[j]; sp.base[j] = lo[j]; sp.n[j] = n[j]; sp.buf[j] = set0 + j; sp.out3[j] = out3[j]; }
    sp.pair_stride = e->set_stride;
    sp.approx = e->d_approx; sp.survivors = e->d_surv; sp.t_min = e->d_tmin; sp.out_dist = e->d_dist; sp.out_shift = e->d_shift;
    sp.blk_part = e->d_surv_part; sp.done_counter = e->d_surv_done; sp.surv_stats = e->d_surv_stats;
    sp.ring_d2 = e->d_ring_d2; sp.k = e->cfg.num_candidates; sp.exclude_eps = e->cfg.knn_exclude_eps; sp.topk_idx = e->d_topk_idx; sp.topk_d2 = e->d_topk_d2;
    const size_t region = (size_t)(region_in >= 0 ? (unsigned)region_in : survivor_arg_region(e)) * scl_engine::kScreenSets * kSurvivorArgBytes;   // 8 passes may be in flight
    sp.d_args = static_cast<char *>(e->d_surv_args) + region; sp.h_args = static_cast<char *>(e->h_surv_args) + region;
    if (!(phases & kSurvivorKernel)) {
        SCL_HIP(e, launch_sc_distance_survivors(db_view(e), sp, e->SR, e->num_cu, stream, phases));
        return SCL_OK;
    }
    ProfScope ps(e, P_ARGMIN, stream);
    SCL_HIP(e, launch_sc_distance_survivors(db_view(e), sp, e->SR, e->num_cu, stream, phases));
    return SCL_OK;
}

// What sc_small_exact_kernel reads and writes for the scan of buffer set `set`: slot qslot against [lo, lo + n), the winner to out3.
// smask_base: the engine's shift masks where the set's screening launch formed them, or nullptr (every shift is scored)
void small_exact_query(const scl_engine *e, SmallExactQuery &sq, int set_index, int qslot, int lo, int n, double *out3, unsigned int *smask_base)
{
    const size_t set = (size_t)set_index, off = set * e->set_stride;
    sq.qslot = qslot; sq.base = lo; sq.n = n;
    sq.approx = e->d_approx + off; sq.starts = e->d_starts + off; sq.smask = smask_base ? smask_base + off : nullptr; sq.ring_d2 = e->d_ring_d2 + off;
    sq.t_min = e->d_tmin + set; sq.list = e->d_surv + off; sq.out3 = out3;
    sq.topk_idx = e->d_topk_idx + set * kTailTopMaxK; sq.topk_d2 = e->d_topk_d2 + set * kTailTopMaxK;
}

// The same pass by sc_small_exact_kernel (sc_masked.hip): ONE workgroup per scan lists the scan's survivors, scores them (every shift:
// the stream's launches form no shift masks), forms the ring-key top-k and writes the winner.  Where the survivors' kernel above holds
// 128 workgroups of 160 KB of LDS for 130 us beside the screening launches -- whose products need every CU: the launch that met them took
// 63 us instead of 38, once per chunk -- this one holds 64 CUs for a fifth of that.  Argument sets through the same regions.
int launch_small_exact_chunk(scl_engine *e, const int *qslot, const int *lo, const int *n, int nq, int set0, double *const *out3, hipStream_t stream,
                             int phases, int region_in)
{
    static_assert(sizeof(SmallExactQuery) <= kSurvivorArgBytes && kMaxSmallExactQueries <= scl_engine::kScreenSets, "argument regions");
    if (nq < 1 || nq > kMaxSmallExactQueries) return fail(e, SCL_ERR_INVALID_ARG, "exact pass: too many scans for one launch");
    const size_t region = (size_t)(region_in >= 0 ? (unsigned)region_in : survivor_arg_region(e)) * scl_engine::kScreenSets * kSurvivorArgBytes;
    SmallExactQuery *h = reinterpret_cast<SmallExactQuery *>(static_cast<char *>(e->h_surv_args) + region);
    SmallExactQuery *d = reinterpret_cast<SmallExactQuery *>(static_cast<char *>(e->d_surv_args) + region);
    const bool wide_masks = sc_screen_is_wide(db_view(e), e->SR) && e->d_smask;   // (80 x 180: every launch forms the shift masks)
    if (phases & kSurvivorArgs) {
        for (int j = 0; j < nq; ++j) small_exact_query(e, h[j], set0 + j, qslot[j], lo[j], n[j], out3[j], wide_masks ? e->d_smask : nullptr);
        SCL_HIP(e, hipMemcpyAsync(d, h, sizeof(SmallExactQuery) * (size_t)nq, hipMemcpyHostToDevice, stream));
    }
    if (!(phases & kSurvivorKernel)) return SCL_OK;
    SmallExactArgs sa{};
    sa.nq = nq; sa.k = e->cfg.num_candidates; sa.exclude_eps = e->cfg.knn_exclude_eps; sa.two_eps = 2.0f * sc_screen_eps(); sa.surv_stats = e->d_surv_stats;
    sa.q_dev = d;
    sa.every_shift = wide_masks ? 0 : 1;
    ProfScope ps(e, P_ARGMIN, stream);
    SCL_HIP(e, launch_sc_small_exact(db_view(e), e->SR, sa, stream));
    return SCL_OK;
}

// The exact pass of the 80 x 180 grid over the screened queries of buffer sets set0 .. set0 + nq - 1: per group of up to four
// queries the select launch (survivor lists + ring-key top-k), the one-sector-per-lane program on the survivors and the arg-min.
// first_done (optional): recorded behind the pass's first group of kWideExactBatch scans
int launch_survivor_pass_wide(scl_engine *e, const int *qslot, const int *lo, const int *n, int nq, int set0, double *const *out3, hipStream_t stream, hipEvent_t first_done = nullptr)
{
    ProfScope ps(e, P_ARGMIN, stream);
    for (int g = 0; g < nq; g += kWideExactBatch) {
        const int w = nq - g < kWideExactBatch ? nq - g : kWideExactBatch;
        ScreenBatch sb{};
        sb.nq = w;
        for (int j = 0; j < w; ++j) { sb.slot[j] = qslot[g + j]; sb.base[j] = lo[g + j]; sb.n[j] = n[g + j]; sb.buf[j] = set0 + g + j; }
        sb.pair_stride = e->set_stride;
        screen_batch_pointers(e, sb, true, e->d_surv_stats, nullptr, nullptr);
        SCL_HIP(e, launch_sc_select_batch(sb, stream));
        const int *sv[kWideExactBatch]; const int *ns[kWideExactBatch]; double *od[kWideExactBatch]; int *os[kWideExactBatch];
        const int *st[kWideExactBatch]; const unsigned int *sm[kWideExactBatch];
        for (int j = 0; j < w; ++j) {
            const size_t set = (size_t)(set0 + g + j);
            sv[j] = e->d_surv + set * e->set_stride; ns[j] = e->d_nsurv + set;
            od[j] = e->d_dist + set * e->set_stride; os[j] = e->d_shift + set * e->set_stride;
            st[j] = e->d_starts + set * e->set_stride; sm[j] = e->d_smask ? e->d_smask + set * e->set_stride : nullptr;
        }
        SCL_HIP(e, launch_sc_distance_survivors_wide(db_view(e), w, qslot + g, lo + g, e->SR, sv, ns, od, os, out3 + g, e->num_cu, stream,
                                                     e->d_smask ? st : nullptr, e->d_smask ? sm : nullptr));
        if (g == 0 && first_done) SCL_HIP(e, hipEventRecord(first_done, stream));
    }
    return SCL_OK;
}

// experiments (diagnostics builds only): SCL_MATRIX_KERNEL=masked keeps round 3's one-wave-per-pair kernel, SCL_MATRIX_KR = keyframes per workgroup
static bool matrix_masked_kernel()
{
    return scl_lab_is("SCL_MATRIX_KERNEL", "m");
}
static int matrix_kr()
{
    return scl_lab_int("SCL_MATRIX_KR", 0);
}

}  // namespace

// The exact distance matrix on a screened grid.  Per group of up to `mb` rows (a screening launch's worth): alignment, screening
// products and finishing -- which leaves, per pair, the first shift and the mask of the shifts within 2 eps of the pair's smallest
// screened distance -- then sc_masked_kernel evaluates exactly those shifts in fp64.  Every entry is the reference's distance and
// shift, bit for bit; the results of a group travel to the host while the next group runs.
int scl::matrix_screened_locked(scl_engine *e, const int *slots, int nq, const int *grp_lo, const int *grp_n, MatrixConsumer &out)
{
    const int mb = sc_screen_max_batch(db_view(e), e->SR);
    const bool wide = sc_screen_is_wide(db_view(e), e->SR);
    const int v2_min = wide ? 2 : 4;                                        // smaller batches take the first form, which leaves no masks: padded
    const int groups = (nq + mb - 1) / mb;
    int max_n = 0;
    for (int g = 0; g < groups; ++g) max_n = grp_n[g] > max_n ? grp_n[g] : max_n;
    int rc = ensure_sets(e, (size_t)max_n);
    if (rc) return rc;
    const size_t need = e->set_stride * scl_engine::kScreenSets;
    if (e->smask_cap < need) {
        dev_free(e->d_smask); e->d_smask = nullptr; e->smask_cap = 0;
        if ((rc = dev_alloc(e, &e->d_smask, need))) return rc;
        e->smask_cap = need;
    }
    const size_t row = ((size_t)max_n + 63) & ~(size_t)63;
    const int RB = kMaxScreenBatch;
    if (e->mat_cap < row * (size_t)(RB / kMaxQueryBatch)) {                  // (the plain form sizes the halves for kMaxQueryBatch rows)
        if (e->d_mat_dist) (void)hipFree(e->d_mat_dist);
        if (e->d_mat_shift) (void)hipFree(e->d_mat_shift);
        if (e->h_mat) (void)hipHostFree(e->h_mat);
        e->d_mat_dist = nullptr; e->d_mat_shift = nullptr; e->h_mat = nullptr; e->mat_cap = 0;
        const size_t cap_rows = (size_t)2 * RB;
        if (hipMalloc((void **)&e->d_mat_dist, sizeof(double) * cap_rows * row) != hipSuccess ||
            hipMalloc((void **)&e->d_mat_shift, sizeof(int) * cap_rows * row) != hipSuccess ||
            hipHostMalloc(&e->h_mat, (sizeof(double) + sizeof(int)) * cap_rows * row, hipHostMallocDefault) != hipSuccess)
            return fail(e, SCL_ERR_NOMEM, "distance matrix buffers");
        e->mat_cap = row * (size_t)(RB / kMaxQueryBatch);
        for (int h = 0; h < 2; ++h) {
            if (!e->ev_mat_k[h]) SCL_HIP(e, hipEventCreateWithFlags(&e->ev_mat_k[h], hipEventDisableTiming));
            if (!e->ev_mat_c[h]) SCL_HIP(e, hipEventCreateWithFlags(&e->ev_mat_c[h], hipEventDisableTiming));
        }
    }
    const size_t cap = row;
    // Consecutive groups alternate between the engine's stream and its second lane (buffer sets, partial sums and output halves of their
    // own) on the 80 x 180 grid: a group is alignment, products and finishing -- launches that each ramp up and drain -- in front of the exact
    // kernel, and on one stream the chip went through them with nothing beside them; now they run under the group before's exact kernel:
    // 97-104 -> 108-116 M pairs/s.  On 64 x 120 the same measured 206-214 -> 194-196 M at 64 rows and nothing at 256: there the exact kernel
    // lives off its keyframes staying in the XCDs' L2s (sc_matrix.hip), which a products launch beside it streams the database through.
    for (int g = 0; g < groups; ++g) {
        const int h = g & 1, r0 = g * mb, rows = nq - r0 < mb ? nq - r0 : mb;
        const int lo = grp_lo[g], n = grp_n[g];
        const int lane = (groups > 1 && wide) ? h : 0, set0 = lane * mb;   // (64 x 120: one lane -- see above)
        hipStream_t ks = lane ? e->stream_alt : e->stream;
        if (n > 0 && lane && e->alt_seen_version != e->db_version) {                  // descriptors written on `stream` since the last pass on the second lane
            SCL_HIP(e, hipEventRecord(e->ev_db, e->stream));
            SCL_HIP(e, hipStreamWaitEvent(e->stream_alt, e->ev_db, 0));
            e->alt_seen_version = e->db_version;
        }
        int qs[kMaxScreenBatch], los[kMaxScreenBatch], ns[kMaxScreenBatch];
        const int padded = rows < v2_min ? v2_min : rows;                   // (the padding rows repeat the last one; their results are dropped)
        for (int j = 0; j < padded; ++j) { qs[j] = slots[r0 + (j < rows ? j : rows - 1)]; los[j] = lo; ns[j] = n; }
        if (n > 0) {
            ProfScope ps(e, P_SC, ks);
            ScreenGroup grp{qs, los, ns, padded, set0};
            grp.masks = true; grp.part_half = lane;
            const int prof_saved = e->prof_on;
            e->prof_on = 0;                                                  // (one event pair around the whole group: this scope's)
            rc = launch_screen_group(e, grp, kScreenAlign | kScreenProducts, nullptr, ks);
            e->prof_on = prof_saved;
            if (rc) return rc;
            const int *g_starts = e->d_starts + (size_t)set0 * e->set_stride;
            const unsigned int *g_smask = e->d_smask + (size_t)set0 * e->set_stride;
            MaskedQuery mq[kMaxMaskedQueries];
            for (int j = 0; j < rows; ++j) {
                mq[j].qslot = qs[j]; mq[j].slot_base = lo; mq[j].n = n; mq[j].n_dev = nullptr; mq[j].cand = nullptr;
                mq[j].starts = g_starts + (size_t)j * e->set_stride; mq[j].smask = g_smask + (size_t)j * e->set_stride;
                mq[j].out_dist = e->d_mat_dist + ((size_t)h * RB + j) * cap; mq[j].out_shift = e->d_mat_shift + ((size_t)h * RB + j) * cap;
            }
            if (sc_matrix_supported(db_view(e), e->SR) && !matrix_masked_kernel()) {
                SCL_HIP(e, launch_sc_matrix(db_view(e), e->SR, qs, rows, lo, n, g_starts, g_smask, e->set_stride,
                                            e->d_mat_dist + (size_t)h * RB * cap, e->d_mat_shift + (size_t)h * RB * cap, cap, matrix_kr(), ks));
            } else {
                int parts = 2 * e->num_cu / rows; parts = parts < 1 ? 1 : parts;
                const int max_parts = (n + 7) / 8; parts = parts > max_parts ? max_parts : parts;
                SCL_HIP(e, launch_sc_masked(db_view(e), e->SR, mq, rows, parts, ks));
            }
            if (ps.active()) e->prof.sc_distance_pairs += (uint64_t)rows * (uint64_t)n;
        }
        if ((rc = out.enqueued({g, h, r0, rows, RB, cap, lo, n, ks, set0, n > 0 ? padded : 0}))) return rc;
        // group g is enqueued: hand over group g - 1 now (its copy ends while g runs; the half it leaves is g + 1's) -- only the last
        // group's copy and hand-over are left behind the last kernel
        if (g >= 1 && (rc = out.retire(g - 1))) return rc;
    }
    if ((rc = out.retire(groups - 1))) return rc;
    if (e->prof_on) collect_profile(e);
    return SCL_OK;
}

namespace {

// A pass's result record in pinned memory (the exact kernels write it: distance, winner's position in its range, shift) as the
// caller's triple; o == nullptr: the pass had nothing to score
void read_result_record(const volatile double *o, int lo, int *nn_idx, int *shift, double *dist)
{
    *nn_idx = -1; *shift = 0; *dist = kBigDist;
    if (!o) return;
    *dist = o[0];
    *nn_idx = o[1] < 0 ? -1 : lo + (int)o[1];
    *shift = (int)o[2];
}

int submit_full_locked(scl_engine *e, int query, int lo, int hi, int *ticket)
{
    if (e->screen && !e->in_single_fallback) {             // one query through the screening pipeline of the batched form
        e->in_single_fallback = true;
        const int rc = submit_full_many_locked(e, &query, &lo, &hi, 1, ticket);
        e->in_single_fallback = false;
        return rc;
    }
    QueryView q;
    int rc = query_view(e, query, &q);
    if (rc) return rc;
    const int sl = (int)(e->next_slot % scl_engine::kSlots);
    if (e->slot_busy[sl]) return fail(e, SCL_ERR_INVALID_ARG, "too many full-DB passes in flight: collect first");
    const int n = clamp_range(lo, hi, e->n);
    e->slot_lo[sl] = lo;
    e->slot_empty[sl] = n <= 0;
    double *out3 = e->h_out3 + (size_t)sl * 8;
    if (n > 0) {
        if ((rc = ensure_pairs(e, (size_t)n))) return rc;
        // "full ring-key + shifted SC distance per incoming scan".  On the two-sectors-per-lane grids the
        // ring-key metric is evaluated inside the SC-distance kernel (the wave that scores a slot also reads
        // its ring key) and one epilogue launch does arg-min + top-k; otherwise the stand-alone ring-key
        // scan runs on a second stream beside the SC kernel.
        const int k = e->cfg.num_candidates;
        const bool fuse = k <= kTailTop && sc_distance_fuses_ring(db_view(e), e->SR);
        if (!fuse) SCL_HIP(e, hipEventRecord(e->ev_fork, e->stream));
        bool fused = false;
        FullTail tail{e->d_blk_part, e->d_done_counter, out3, e->d_topk_idx, e->d_topk_d2, k, e->cfg.knn_exclude_eps};
        {
            ProfScope ps(e, P_SC);
            SCL_HIP(e, launch_sc_distance(db_view(e), q, nullptr, lo, n, e->SR, e->d_dist, e->d_shift, e->num_cu, e->stream,
                                          fuse ? e->d_ring_d2 : nullptr, &fused, fuse ? &tail : nullptr));
            if (ps.active()) e->prof.sc_distance_pairs += (uint64_t)n;
        }
        if (fuse && fused) {
            // arg-min and top-k were reduced inside the kernel (last workgroup)
        } else {
            if (fuse) return fail(e, SCL_ERR_HIP, "ring-key fusion expected but not provided by the kernel");
            SCL_HIP(e, hipStreamWaitEvent(e->stream2, e->ev_fork, 0));
            if ((rc = launch_topk(e, q, lo, hi, k, e->cfg.knn_exclude_eps, e->stream2))) return rc;
            SCL_HIP(e, hipEventRecord(e->ev_join, e->stream2));
            {
                ProfScope ps(e, P_ARGMIN);
                SCL_HIP(e, launch_argmin(e->d_dist, e->d_shift, n, out3, e->stream));   // writes pinned host memory
            }
            SCL_HIP(e, hipStreamWaitEvent(e->stream, e->ev_join, 0));
        }
    }
    e->last_pass_empty = n <= 0;                            // nothing ran: the top-k buffers still hold an older pass
    SCL_HIP(e, hipEventRecord(e->ev_done[sl], e->stream));
    e->slot_ev[sl] = sl; e->slot_seq[sl] = 0;
    e->slot_busy[sl] = true;
    e->next_slot++;
    *ticket = sl;
    return SCL_OK;
}

// nq database-resident queries, one launch (workgroups [i*nb, (i+1)*nb) serve query i); every query gets its own
// result slot, all of them complete with the one event recorded behind the launch.
int submit_full_many_locked(scl_engine *e, const int *queries, const int *los, const int *his, int nq, int *tickets)
{
    const int k = e->cfg.num_candidates;
    const bool wide = e->screen && sc_screen_is_wide(db_view(e), e->SR);      // 80 x 180
    bool batchable = (nq > 1 || e->screen) && nq <= kMaxQueryBatch && (k <= kTailTop || e->screen) && (sc_distance_fuses_ring(db_view(e), e->SR) || wide);
    int qslot[kMaxQueryBatch] = {0};                       // database index of every query (staging slot j = cap + j)
    for (int i = 0; i < nq && batchable; ++i) batchable = (qslot[i] = query_slot(e, queries[i], e->n)) >= 0;
    if (!batchable) {                                      // one pass per query
        for (int i = 0; i < nq; ++i) { int rc = submit_full_locked(e, queries[i], los[i], his[i], &tickets[i]); if (rc) return rc; }
        return SCL_OK;
    }
    for (int i = 0; i < nq; ++i)
        if (e->slot_busy[(e->next_slot + (unsigned)i) % scl_engine::kSlots])
            return fail(e, SCL_ERR_INVALID_ARG, "too many full-DB passes in flight: collect first");
    QueryBatch qb{};
    unsigned int seq_of_launch = 0;                        // (the small exact pass: the number it writes behind every result record)
    int first = -1, nmax = 0;
    int lo_of[kMaxQueryBatch]; bool empty_of[kMaxQueryBatch];
    for (int i = 0; i < nq; ++i) {
        const int sl = (int)((e->next_slot + (unsigned)i) % scl_engine::kSlots);
        int lo = los[i], hi = his[i];
        const int n = clamp_range(lo, hi, e->n);
        tickets[i] = sl;
        lo_of[i] = lo; empty_of[i] = n <= 0;
        if (first < 0) first = sl;
        if (n > 0) {
            const int j = qb.nq++;
            qb.slot[j] = qslot[i]; qb.base[j] = lo; qb.n[j] = n; qb.out3[j] = e->h_out3 + (size_t)sl * 8;
            nmax = n > nmax ? n : nmax;
        }
    }
    if (qb.nq > 0) {
        int rc = e->screen ? SCL_OK : ensure_pairs(e, (size_t)nmax * qb.nq);
        if (rc) return rc;
        qb.pair_stride = (size_t)nmax;
        FullTail tail{e->d_blk_part, e->d_done_counter, nullptr, e->d_topk_idx, e->d_topk_d2, k, e->cfg.knn_exclude_eps};
        if (e->screen) {
            // screening pass (fp16 matrix-core bounds around every reference distance) -> the exact fp64 kernel on the
            // survivors only; the winner is the reference's, bit for bit (sc_screen.hip)
            if ((rc = ensure_sets(e, (size_t)nmax))) return rc;
            ScreenGroup sg{qb.slot, qb.base, qb.n, qb.nq, 0};
            sg.masks = !wide && sc_small_exact_supported(db_view(e), e->SR);
            if ((rc = launch_screen_group(e, sg))) return rc;
            const bool small_pass = (sg.masks || wide) && sc_small_exact_supported(db_view(e), e->SR) && e->d_smask && !scl_lab_int("SCL_SMALL_EXACT_OFF", 0);
            if (wide && !small_pass) {
                if ((rc = launch_survivor_pass_wide(e, qb.slot, qb.base, qb.n, qb.nq, 0, qb.out3, e->stream))) return rc;
            } else if (small_pass) {
                // a blocking call's handful of scans: one workgroup per scan selects, scores the open shifts, forms the top-k and
                // writes the winner (sc_masked.hip) -- one launch, no argument copy
                SmallExactArgs sa{};
                sa.nq = qb.nq; sa.k = k; sa.exclude_eps = e->cfg.knn_exclude_eps; sa.two_eps = 2.0f * sc_screen_eps(); sa.surv_stats = e->d_surv_stats;
                for (int j = 0; j < qb.nq; ++j) small_exact_query(e, sa.q[j], j, qb.slot[j], qb.base[j], qb.n[j], qb.out3[j], e->d_smask);
                if (++e->out_seq == 0) ++e->out_seq;
#ifndef SCL_NO_SEQ
                sa.seq = seq_of_launch = e->out_seq;
#endif
                ProfScope ps(e, P_ARGMIN);
                SCL_HIP(e, launch_sc_small_exact(db_view(e), e->SR, sa, e->stream));
            } else if ((rc = launch_survivor_pass(e, qb.slot, qb.base, qb.n, qb.nq, 0, qb.out3))) return rc;
        } else {
            ProfScope ps(e, P_SC);
            SCL_HIP(e, launch_sc_distance_batch(db_view(e), qb, e->SR, e->d_dist, e->d_shift, e->d_ring_d2, tail, e->num_cu, e->stream));
            if (ps.active()) { for (int j = 0; j < qb.nq; ++j) e->prof.sc_distance_pairs += (uint64_t)qb.n[j]; }
        }
    }
    e->last_pass_empty = qb.nq == 0 || empty_of[0];
    SCL_HIP(e, hipEventRecord(e->ev_done[first], e->stream));
    // slot state changes only now that the launch and its event are enqueued (an error above leaves every slot free)
    for (int i = 0; i < nq; ++i) {
        e->slot_lo[tickets[i]] = lo_of[i]; e->slot_empty[tickets[i]] = empty_of[i];
        e->slot_ev[tickets[i]] = first; e->slot_busy[tickets[i]] = true;
        e->slot_seq[tickets[i]] = empty_of[i] ? 0u : seq_of_launch;
    }
    e->next_slot += (unsigned)nq;
    return SCL_OK;
}

int collect_full_locked(scl_engine *e, int ticket, int *nn_idx, int *shift, double *dist)
{
    if (ticket < 0 || ticket >= scl_engine::kSlots || !e->slot_busy[ticket])
        return fail(e, SCL_ERR_INVALID_ARG, "unknown ticket");
    {
        // a pass of one or a few scans ends within tens of microseconds: poll for that long (a blocking wait wakes up tens of
        // microseconds late -- a fifth of a blocking one-scan call), then sleep in the runtime
        hipEvent_t ev = e->ev_done[e->slot_ev[ticket]];
        hipError_t q = hipSuccess;
        const unsigned int seq = e->slot_empty[ticket] ? 0u : e->slot_seq[ticket];
        if (seq) {
            // the exact pass's workgroup writes this launch's number behind the record in pinned memory: seen here 4-6 us before the
            // event's packet fires.  (The launches behind it on the stream are ordered by the stream; nothing else of this pass is read here.)
            const volatile double *o = e->h_out3 + (size_t)ticket * 8;
            const auto t0 = std::chrono::steady_clock::now();
            int spins = 0;
            while (o[4] != (double)seq)
                if ((++spins & 255) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(300)) { q = hipEventSynchronize(ev); break; }
        } else {
            q = wait_event_polled(ev, std::chrono::microseconds(300), false);
        }
        SCL_HIP(e, q);
        std::atomic_thread_fence(std::memory_order_acquire);
    }
    collect_profile(e);
    e->slot_busy[ticket] = false;
    read_result_record(e->slot_empty[ticket] ? nullptr : e->h_out3 + (size_t)ticket * 8, e->slot_lo[ticket], nn_idx, shift, dist);
    return SCL_OK;
}

}  // namespace

int scl_detect_full_submit(scl_engine *e, int query, int lo, int hi, int *ticket)
{
    if (!e || !ticket) return SCL_ERR_INVALID_ARG;
    if (e->front) return front_submit_many(e, &query, &lo, &hi, 1, ticket);
    std::lock_guard<std::mutex> pk(e->pass_mu);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    return submit_full_locked(e, query, lo, hi, ticket);
}

int scl_detect_full_submit_many(scl_engine *e, const int *queries, const int *lo, const int *hi, int n_queries, int *tickets)
{
    if (!e || !queries || !lo || !hi || !tickets || n_queries < 1 || n_queries > scl_engine::kSlots) return SCL_ERR_INVALID_ARG;
    if (e->front) {
        for (int i = 0; i < n_queries; i += kMaxQueryBatch) {
            const int m = n_queries - i < kMaxQueryBatch ? n_queries - i : kMaxQueryBatch;
            const int rc = front_submit_many(e, queries + i, lo + i, hi + i, m, tickets + i);
            if (rc) return rc;
        }
        return SCL_OK;
    }
    std::lock_guard<std::mutex> pk(e->pass_mu);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    for (int i = 0; i < n_queries; i += kMaxQueryBatch) {
        const int m = n_queries - i < kMaxQueryBatch ? n_queries - i : kMaxQueryBatch;
        int rc = submit_full_many_locked(e, queries + i, lo + i, hi + i, m, tickets + i);
        if (rc) return rc;
    }
    return SCL_OK;
}

namespace {

// The stream form on the screened grid: a chunk of up to kScreenSets scans = its screening launches back to back
// (spl scans per launch, one buffer set per scan), then ONE exact pass over the survivors of the whole chunk, one
// event.  Two chunks are kept enqueued (their results land in the two halves of h_stream_out), so the device never
// waits for the host between chunks.
// `db`: the caller's lock on the database (e->mu).  The call scores the database it was started on -- n0 keyframes -- and gives the
// lock up while it waits for a chunk's results: appends (which take e->mu only) get in there, behind the launches already enqueued on
// the stream; a capacity doubling waits for every stream of the engine before it frees the old arrays (grow_to), and the launches
// enqueued after it read the new ones (db_view is formed per launch).  pass_mu, held by the caller throughout, keeps every other
// scoring entry point out of the buffer sets.
int stream_screened_locked(scl_engine *e, std::unique_lock<std::mutex> &db, const int *queries, const int *lo, const int *hi, int n_queries, int spl,
                           int *nn_idx, int *shift, double *dist)
{
    const int n0 = e->n;                                     // the database this call scores
    constexpr int NS = scl_engine::kScreenSets;
    constexpr int CH = NS / 2;                               // scans per chunk at most: the two chunks in flight use the two halves of the buffer sets
    // ... and a whole number of launches (a short launch costs the same pass over the database as a full one)
    static_assert(CH <= kMaxSurvivorQueries, "one exact pass takes the survivors of a whole chunk");
    const bool wide = sc_screen_is_wide(db_view(e), e->SR);  // 80 x 180: same launches, its own exact pass
    // (80 x 180: chunks of 64 -- its exact pass is a chain of launches per 16 scans that runs beside the NEXT chunk's screening, and the
    //  host submits the chunk after that only when it has ended: chunks of 128 measured 3 % slower there, 4 % faster on 64 x 120)
#ifndef SCL_WIDE_CHUNK
#define SCL_WIDE_CHUNK 64
#endif
    const int chmax = wide && CH > SCL_WIDE_CHUNK ? SCL_WIDE_CHUNK : CH;
    const int chn = spl >= 1 && spl <= chmax ? (chmax / spl) * spl : chmax;
    struct List { int qslot[CH], qlo[CH], qn[CH], pos[CH], m = 0; };     // the scans of a chunk that have something to score
    struct Chunk { int first = 0, count = 0; int aligned = 0; bool busy = false, small = false; std::vector<int> lo, empty; };   // aligned: leading scans of its list that the chunk before aligned
    Chunk ch[2];
    bool sub0_valid[2] = {false, false};                    // ev_sub0[c] was recorded by the exact pass that ev_chunk[c] ends
    // 64 x 120: the chunk's exact pass by one workgroup per scan (SCL_STREAM_EXACT=survivors keeps round 3's kernel, which also forms the
    // ring-key metric of its ranges -- keys_later)
    const bool small_exact = sc_small_exact_supported(db_view(e), e->SR) && (!wide || e->d_smask) && !scl_lab_is("SCL_STREAM_EXACT", "s");
    const bool keys_later = !wide && !small_exact;
    const bool pairs = !wide && sc_screen_pairs(db_view(e), e->SR);   // two consecutive full launch groups share one products launch (SCL_SCREEN_PAIR=0: never)
    int nmax = 1;
    for (int i = 0; i < n_queries; ++i) {
        int l = lo[i], h = hi[i];
        const int n = clamp_range(l, h, n0);
        if (n > nmax) nmax = n;
    }
    int rc = ensure_sets(e, (size_t)nmax);
    if (rc) return rc;
    // the side stream starts behind everything the main stream holds (ingests wrote the arrays it reads)
    SCL_HIP(e, hipEventRecord(e->ev_align_gate, e->stream));
    SCL_HIP(e, hipStreamWaitEvent(e->stream_surv, e->ev_align_gate, 0));
    auto build = [&](int first, int count, List &L, Chunk *k) -> int {
        L.m = 0;
        for (int i = 0; i < count; ++i) {
            const int slot = query_slot(e, queries[first + i], n0);
            if (slot == kQueryOutOfRange) return fail(e, SCL_ERR_OUT_OF_RANGE, "query slot out of range");
            if (slot == kQueryNotStaged) return fail(e, SCL_ERR_INVALID_ARG, "no staged query");
            int l = lo[first + i], h = hi[first + i];
            const int n = clamp_range(l, h, n0);
            if (k) k->lo[(size_t)i] = l;
            if (n <= 0) continue;
            if (k) k->empty[(size_t)i] = 0;
            L.qslot[L.m] = slot; L.qlo[L.m] = l; L.qn[L.m] = n; L.pos[L.m] = i;
            ++L.m;
        }
        return SCL_OK;
    };
    // c = half of the buffer sets; first / count = this chunk; nfirst / ncount = the chunk behind it (ncount = 0: none)
    auto submit = [&](int c, int first, int count, int nfirst, int ncount) -> int {
        Chunk &k = ch[c];
        k.first = first; k.count = count; k.lo.assign((size_t)count, 0); k.empty.assign((size_t)count, 1);
        List cur, nxt;
        if ((rc = build(first, count, cur, &k))) return rc;
        if (ncount > 0 && (rc = build(nfirst, ncount, nxt, nullptr))) return rc;
        double *out3[CH];
        for (int j = 0; j < cur.m; ++j) out3[j] = e->h_stream_out + ((size_t)c * NS + (size_t)cur.pos[j]) * 8;
        // buffer set = first set of this half + position among the non-empty scans (consecutive within a launch).  The two
        // halves alternate, and a chunk is submitted only after the chunk two before it was collected.
        const int set0 = c * CH, nset0 = (c ^ 1) * CH;
        // the exact pass's argument sets go to the device now, ahead of the products it has to wait for
        // one workgroup per scan scores its survivors at every shift: right for the handful a scan leaves as a rule; dozens per scan (what
        // the chunks collected last reported) go to the survivors' kernel
        k.small = small_exact && !e->exact_heavy;
        const int region = (cur.m > 0 && (k.small || !wide)) ? (int)survivor_arg_region(e) : 0;
        if (cur.m > 0 && (k.small || !wide) && (rc = k.small ? launch_small_exact_chunk(e, cur.qslot, cur.qlo, cur.qn, cur.m, set0, out3, e->stream_surv, kSurvivorArgs, region)
                                                    : launch_survivor_pass(e, cur.qslot, cur.qlo, cur.qn, cur.m, set0, out3, e->stream_surv, kSurvivorArgs, region, keys_later))) return rc;
        if (ncount == 0 && cur.m > 0) SCL_HIP(e, hipEventRecord(e->ev_k1[c], e->stream_surv));   // the call's last chunk: its exact pass runs on the main stream, behind this copy
        // Sampled profile (scl_profile_enable(3)): ONE event pair around the screening launches of every second chunk, its time divided
        // by the chunk's launch groups -- a pair around a single group keeps that group's two launches back by 4-6 us each and
        // measured 5 us (8 %) more than the kernel trace; the events the chunk needs anyway (the exact pass's, the wait for the buffer
        // sets) are inside the span: they are the stream's, not the measurement's.
        struct ProfRestore { scl_engine *e; int saved; ~ProfRestore() { e->prof_on = saved; } } prof_restore{e, e->prof_on};
        hipEvent_t span_start = nullptr, span_stop = nullptr;
        int span_groups = 0;
        if (e->prof_on == 3 && cur.m > 0) {
            if ((e->prof_tick++ & 1) == 0) {
                auto get = [&]() { hipEvent_t ev = nullptr; if (!e->event_pool.empty()) { ev = e->event_pool.back(); e->event_pool.pop_back(); } else if (hipEventCreate(&ev) != hipSuccess) ev = nullptr; return ev; };
                span_start = get(); span_stop = get();
                if (span_start && span_stop) (void)hipEventRecord(span_start, e->stream); else { span_start = span_stop = nullptr; }
            }
            e->prof_on = 0;                                  // (no pairs around single groups inside)
        }
        auto span_end = [&]() {
            if (!span_start) return;
            (void)hipEventRecord(span_stop, e->stream);
            e->pending.push_back({span_start, span_stop, P_SC, span_groups});
            for (int j = 0; j < cur.m; ++j) e->prof.sc_distance_pairs += (uint64_t)cur.qn[j];
            span_start = nullptr;
        };
        // The schedule (screen_plan.hpp): which groups go as pairs -- one products launch for both (sc_screen.hip: the database crosses
        // the fabric once for 32 scans), a tail each --, which group aligns for itself, whose alignment rides in whose tail.  A plan's
        // group is scans of this chunk's list or, past its end, of the next chunk's, in the other half of the buffer sets.  Every launch
        // carries the alignment of what follows it -- the chunk's last one that of the next chunk's first group or pair, whose buffer sets
        // the exact pass of the chunk before this one may still be reading: the main stream waits for it there (it finished long ago; the
        // event behind that chunk's whole exact pass covers the sets of both groups of a pair).  Only the call's first launch aligns for itself.
        static_assert(kPlanPairGroup == kMaxScreenBatch, "a pair is two full launch groups");
        PlanUnit units[CH];
        int next_aligned = 0;
        const int n_units = plan_chunk(cur.m, ncount > 0 ? nxt.m : 0, spl, pairs, k.aligned, units, &next_aligned);
        auto group_of = [&](const PlanGroup &p) {
            ScreenGroup g{nullptr, nullptr, nullptr, 0, 0};
            const int o = p.off - cur.m;
            if (p.nq > 0) g = o < 0 ? ScreenGroup{cur.qslot + p.off, cur.qlo + p.off, cur.qn + p.off, p.nq, set0 + p.off} : ScreenGroup{nxt.qslot + o, nxt.qlo + o, nxt.qn + o, p.nq, nset0 + o};
            g.keys_later = keys_later;
            return g;
        };
        for (int i = 0; i < n_units; ++i) {
            const PlanUnit &u = units[i];
            const ScreenGroup g0 = group_of(u.g0), g1 = group_of(u.g1), n0 = group_of(u.n0), n1 = group_of(u.n1);
            if (u.over > 0) {
                // the next chunk's first buffer sets, which the exact pass of the chunk before this one may still be reading
                // (80 x 180: the exact pass of a chunk is several launch groups, one per kWideExactBatch buffer sets, and nearly as
                //  long as the next chunk's screening: this launch's alignment writes the first group's sets only and waits for those)
                if (ch[c ^ 1].busy) SCL_HIP(e, hipStreamWaitEvent(e->stream, (wide && sub0_valid[c ^ 1] && u.over <= kWideExactBatch) ? e->ev_sub0[c ^ 1] : e->ev_chunk[c ^ 1], 0));
            }
            if (g1.nq > 0) rc = launch_screen_pair_group(e, g0, g1, u.align0, u.align1, n0.nq > 0 ? &n0 : nullptr, n1.nq > 0 ? &n1 : nullptr);
            else rc = launch_screen_group(e, g0, u.align0 ? (kScreenAlign | kScreenProducts) : kScreenProducts, n0.nq > 0 ? &n0 : nullptr);
            if (rc) return rc;
            ++span_groups;
        }
        span_end();
        // The exact pass of a chunk runs beside the next chunk's products, on the side stream -- except the call's last one,
        // which nothing follows: it stays on the main stream (no hop between streams in front of it; its argument sets are
        // already on the device: wait for their copy only).
        hipStream_t xs = ncount > 0 ? e->stream_surv : e->stream;
        if (ncount > 0) {
            SCL_HIP(e, hipEventRecord(e->ev_k1[c], e->stream));
            SCL_HIP(e, hipStreamWaitEvent(e->stream_surv, e->ev_k1[c], 0));
        } else if (cur.m > 0) {
            // behind the copy of the argument sets, enqueued on the side stream before this chunk's launches: long done as a rule, and a
            // wait for a pending event keeps the main stream's next launch back by 5 us -- asked for only if the copy is still on its way
            // (the event was recorded behind the copy, at the start of this chunk's submission)
            if (hipEventQuery(e->ev_k1[c]) != hipSuccess) SCL_HIP(e, hipStreamWaitEvent(e->stream, e->ev_k1[c], 0));
        }
        sub0_valid[c] = wide && !k.small && cur.m > 0;
        if (cur.m > 0 && (rc = k.small ? launch_small_exact_chunk(e, cur.qslot, cur.qlo, cur.qn, cur.m, set0, out3, xs, kSurvivorKernel, region)
                             : wide ? launch_survivor_pass_wide(e, cur.qslot, cur.qlo, cur.qn, cur.m, set0, out3, xs, e->ev_sub0[c])
                                    : launch_survivor_pass(e, cur.qslot, cur.qlo, cur.qn, cur.m, set0, out3, xs, kSurvivorKernel, region, keys_later))) return rc;
        SCL_HIP(e, hipEventRecord(e->ev_chunk[c], xs));
        k.busy = true;
        k.aligned = 0;
        ch[c ^ 1].aligned = next_aligned;                    // the next chunk's first launch (pair) needs no alignment of its own
        e->last_pass_empty = cur.m == 0;
        return SCL_OK;
    };
    auto collect = [&](int c, bool last) -> int {
        Chunk &k = ch[c];
        // A chunk's event is polled (for up to 20 ms, then the runtime's blocking wait): the blocking wait wakes up late -- tens of
        // microseconds as a rule, but the next chunk's launches are enqueued only after it, and on the 80 x 180 grid, whose exact
        // pass ends late in the following chunk's screening, the main stream ran dry for 100-120 us of every chunk (a tenth)
        // (relaxed: a thread that appends meanwhile goes through the same runtime)
        auto wait_chunk = [&]() { return wait_event_polled(e->ev_chunk[c], std::chrono::milliseconds(20), true); };
        if (last) {
            SCL_HIP(e, wait_chunk());
        } else {
            // more to submit behind this wait: the database lock is free meanwhile (appends get in; nothing of this call's state
            // names a slot or a pointer that a capacity doubling could move: the chunks in flight are enqueued, the next one is
            // built after the lock is back)
            db.unlock();
            const hipError_t w = wait_chunk();
            db.lock();
            SCL_HIP(e, w);
        }
        collect_profile(e);
        double listed = 0.0; int scored = 0;
        for (int i = 0; i < k.count; ++i) {
            const int o_i = k.first + i;
            const volatile double *o = k.empty[(size_t)i] ? nullptr : e->h_stream_out + ((size_t)c * NS + (size_t)i) * 8;
            if (o) { listed += o[3]; ++scored; }
            read_result_record(o, k.lo[(size_t)i], &nn_idx[o_i], &shift[o_i], &dist[o_i]);
        }
        if (small_exact && scored > 0) {                      // (with hysteresis: 32 survivors per scan and more, 16 and fewer)
            const double mean = listed / (double)scored;
            if (mean > 32.0) e->exact_heavy = true; else if (mean < 16.0) e->exact_heavy = false;
        }
        k.busy = false;
        return SCL_OK;
    };
    int next = 0, c = 0;
    while (next < n_queries || ch[0].busy || ch[1].busy) {
        if (next < n_queries && !ch[c].busy) {
            const int count = n_queries - next < chn ? n_queries - next : chn;
            const int nfirst = next + count;
            const int ncount = n_queries - nfirst < chn ? n_queries - nfirst : chn;
            if ((rc = submit(c, next, count, nfirst, ncount > 0 ? ncount : 0))) {
                drain_keeping_error(e, {e->stream, e->stream_surv});
                return rc;
            }
            next += count;
            c ^= 1;
            continue;
        }
        // both halves enqueued (or nothing left to submit): wait for the older one
        const int older = ch[c].busy ? c : c ^ 1;
        if ((rc = collect(older, next >= n_queries))) return rc;
    }
    return SCL_OK;
}

}  // namespace

// scl_detect_full_stream behind its locks (pass_mu held, `lk` = the database lock): also the detection half of scl_stream_from_points
int scl::detect_full_stream_locked(scl_engine *e, std::unique_lock<std::mutex> &lk, const int *queries, const int *lo, const int *hi, int n_queries,
                              int scans_per_launch, int launches_in_flight, int *nn_idx, int *shift, double *dist)
{
    for (int i = 0; i < scl_engine::kSlots; ++i)
        if (e->slot_busy[i]) return fail(e, SCL_ERR_INVALID_ARG, "detect_full_stream: collect the passes in flight first");
    if (n_queries >= 1 && n_queries <= kMaxQueryBatch && e->screen) {
        // a handful of scans (several robots' keyframes arriving together): the blocking form's launch group -- products that align for
        // themselves, one workgroup per scan for the exact pass, the winners read off the sequence number in pinned memory -- instead of
        // the stream's chunk machinery (two scans: 114 -> 80 us); the same winners, bit for bit
        int tk[kMaxQueryBatch];
        int rc = submit_full_many_locked(e, queries, lo, hi, n_queries, tk);
        if (rc) {
            drain_keeping_error(e, {e->stream});
            for (int i = 0; i < scl_engine::kSlots; ++i) e->slot_busy[i] = false;
            return rc;
        }
        for (int i = 0; i < n_queries; ++i) {
            const int r2 = collect_full_locked(e, tk[i], &nn_idx[i], &shift[i], &dist[i]);
            if (r2 && !rc) rc = r2;
        }
        return rc;
    }
    if (e->screen && (sc_distance_fuses_ring(db_view(e), e->SR) || sc_screen_is_wide(db_view(e), e->SR))) {
        // the screened grids take up to kMaxScreenBatch scans per launch: the workgroups of a launch's queries share every
        // keyframe line through the L2 (sc_screen.hip), so more scans per launch read less per scan from HBM
        const int mb = sc_screen_max_batch(db_view(e), e->SR);
        const int spl_s = scans_per_launch < 1 ? 1 : (scans_per_launch > mb ? mb : scans_per_launch);
        return stream_screened_locked(e, lk, queries, lo, hi, n_queries, spl_s, nn_idx, shift, dist);
    }
    const int spl = scans_per_launch < 1 ? 1 : (scans_per_launch > kMaxQueryBatch ? kMaxQueryBatch : scans_per_launch);
    int depth = launches_in_flight < 1 ? 1 : launches_in_flight;
    if (depth * spl > scl_engine::kSlots) depth = scl_engine::kSlots / spl;
    std::vector<int> tk((size_t)n_queries);
    int submitted = 0, collected = 0;
    // error path: the passes already enqueued are waited for and their slots released, so the engine's pipeline is
    // usable again afterwards (their results are dropped; last_error keeps the first failure)
    auto drain = [&]() {
        drain_keeping_error(e, {e->stream});
        for (int i = collected; i < submitted; ++i) e->slot_busy[tk[(size_t)i]] = false;
    };
    while (collected < n_queries) {
        while (submitted < n_queries) {                       // keep `depth` launches enqueued
            const int m = n_queries - submitted < spl ? n_queries - submitted : spl;
            if ((submitted - collected) + m > depth * spl) break;
            const int rc = submit_full_many_locked(e, queries + submitted, lo + submitted, hi + submitted, m, tk.data() + submitted);
            if (rc) { drain(); return rc; }
            submitted += m;
        }
        const int rc = collect_full_locked(e, tk[(size_t)collected], nn_idx + collected, shift + collected, dist + collected);
        ++collected;
        if (rc) { drain(); return rc; }
    }
    return SCL_OK;
}

int scl_detect_full_stream(scl_engine *e, const int *queries, const int *lo, const int *hi, int n_queries,
                           int scans_per_launch, int launches_in_flight, int *nn_idx, int *shift, double *dist)
{
    if (!e || !queries || !lo || !hi || !nn_idx || !shift || !dist || n_queries < 0) return SCL_ERR_INVALID_ARG;
    if (e->front) return front_detect_full_stream(e, queries, lo, hi, n_queries, scans_per_launch, launches_in_flight, nn_idx, shift, dist);
    std::lock_guard<std::mutex> pk(e->pass_mu);
    std::unique_lock<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    return detect_full_stream_locked(e, lk, queries, lo, hi, n_queries, scans_per_launch, launches_in_flight, nn_idx, shift, dist);
}

int scl_detect_full_collect(scl_engine *e, int ticket, int *nn_idx, int *shift, double *dist)
{
    if (!e || !nn_idx || !shift || !dist) return SCL_ERR_INVALID_ARG;
    if (e->front) return front_collect(e, ticket, nn_idx, shift, dist);
    std::lock_guard<std::mutex> pk(e->pass_mu);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    return collect_full_locked(e, ticket, nn_idx, shift, dist);
}

int scl_detect_full_range(scl_engine *e, int query, int lo, int hi, int *nn_idx, int *shift, double *dist)
{
    if (!e || !nn_idx || !shift || !dist) return SCL_ERR_INVALID_ARG;
    if (e->front) {
        int t = -1;
        const int rc = front_submit_many(e, &query, &lo, &hi, 1, &t);
        return rc ? rc : front_collect(e, t, nn_idx, shift, dist);
    }
    std::lock_guard<std::mutex> pk(e->pass_mu);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    *nn_idx = -1; *shift = 0; *dist = kBigDist;
    int ticket = -1;
    int rc = submit_full_locked(e, query, lo, hi, &ticket);
    if (rc) return rc;
    return collect_full_locked(e, ticket, nn_idx, shift, dist);
}

int scl_screen_distances(scl_engine *e, int query, int lo, int hi, float *approx, int *survivors, int *n_survivors, float *eps)
{
    if (!e || !approx) return SCL_ERR_INVALID_ARG;
    if (e->front) return fail(e, SCL_ERR_UNSUPPORTED, "screen_distances: call it on a one-GPU engine");
    std::lock_guard<std::mutex> pk(e->pass_mu);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    if (eps) *eps = sc_screen_eps();
    if (!e->screen) return fail(e, SCL_ERR_UNSUPPORTED, "no screening pass for this grid (64x120 and 80x180 at search ratio 0.1 only)");
    const int qslot = query_slot(e, query, e->n);
    if (qslot == kQueryOutOfRange) return fail(e, SCL_ERR_OUT_OF_RANGE, "query slot out of range");
    if (qslot == kQueryNotStaged) return fail(e, SCL_ERR_INVALID_ARG, "no staged query");
    const int n = clamp_range(lo, hi, e->n);
    if (n_survivors) *n_survivors = 0;
    if (n <= 0) return SCL_OK;
    int rc;
    if ((rc = ensure_pairs(e, (size_t)n))) return rc;
    {   // scratch of the products' second form: ring parts x passes x 16 floats per pair
        const size_t per_pair = sc_screen_scratch_floats(db_view(e), e->SR) / (size_t)sc_screen_max_batch(db_view(e), e->SR);
        if ((size_t)n * per_pair > e->part_cap) {
            dev_free(e->d_part); e->part_cap = 0;
            if ((rc = dev_alloc(e, &e->d_part, (size_t)n * per_pair + 1024))) return rc;
            e->part_cap = (size_t)n * per_pair + 1024;
        }
    }
    ScreenBatch sb{};
    sb.nq = 1; sb.slot[0] = qslot; sb.base[0] = lo; sb.n[0] = n; sb.pair_stride = (size_t)n;
    screen_batch_pointers(e, sb, true, nullptr, nullptr, e->d_part);
    SCL_HIP(e, launch_sc_screen_batch(db_view(e), sb, e->SR, sc_align_filter_enabled(), e->num_cu, e->stream));
    SCL_HIP(e, launch_sc_select_batch(sb, e->stream));
    SCL_HIP(e, hipMemcpyAsync(approx, e->d_approx, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, e->stream));
    int ns = 0;
    SCL_HIP(e, hipMemcpyAsync(&ns, e->d_nsurv, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    if ((rc = sync(e))) return rc;
    if (n_survivors) *n_survivors = ns;
    if (survivors && ns > 0) {
        SCL_HIP(e, hipMemcpyAsync(survivors, e->d_surv, sizeof(int) * (size_t)ns, hipMemcpyDeviceToHost, e->stream));
        if ((rc = sync(e))) return rc;
    }
    return SCL_OK;
}

int scl_screen_distances_many(scl_engine *e, const int *queries, int n_queries, int lo, int hi, float *approx, float *eps)
{
    if (!e || !queries || !approx || n_queries < 1 || n_queries > kMaxScreenBatch) return SCL_ERR_INVALID_ARG;
    if (e->front) return fail(e, SCL_ERR_UNSUPPORTED, "screen_distances_many: call it on a one-GPU engine");
    std::lock_guard<std::mutex> pk(e->pass_mu);
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    if (eps) *eps = sc_screen_eps();
    if (!e->screen) return fail(e, SCL_ERR_UNSUPPORTED, "no screening pass for this grid (64x120 and 80x180 at search ratio 0.1 only)");
    if (n_queries > sc_screen_max_batch(db_view(e), e->SR)) return fail(e, SCL_ERR_INVALID_ARG, "more scans than a screening launch takes");
    const int n = clamp_range(lo, hi, e->n);
    if (n <= 0) return SCL_OK;
    int rc;
    if ((rc = ensure_pairs(e, (size_t)n * (size_t)n_queries))) return rc;
    {
        const size_t per_pair = sc_screen_scratch_floats(db_view(e), e->SR) / (size_t)sc_screen_max_batch(db_view(e), e->SR);
        const size_t want = (size_t)n * (size_t)n_queries * per_pair + 1024;
        if (want > e->part_cap) {
            dev_free(e->d_part); e->part_cap = 0;
            if ((rc = dev_alloc(e, &e->d_part, want))) return rc;
            e->part_cap = want;
        }
    }
    ScreenBatch sb{};
    sb.nq = n_queries; sb.pair_stride = (size_t)n;
    for (int i = 0; i < n_queries; ++i) {
        sb.slot[i] = query_slot(e, queries[i], e->n);
        if (sb.slot[i] == kQueryOutOfRange) return fail(e, SCL_ERR_OUT_OF_RANGE, "query slot out of range");
        if (sb.slot[i] == kQueryNotStaged) return fail(e, SCL_ERR_INVALID_ARG, "no staged query");
        sb.base[i] = lo; sb.n[i] = n; sb.buf[i] = i;
    }
    screen_batch_pointers(e, sb, true, nullptr, nullptr, e->d_part);
    SCL_HIP(e, launch_sc_screen_batch(db_view(e), sb, e->SR, sc_align_filter_enabled(), e->num_cu, e->stream));
    SCL_HIP(e, hipMemsetAsync(e->d_tmin, 0xff, sizeof(unsigned int) * (size_t)n_queries, e->stream));          // (no select launch re-arms the words)
    SCL_HIP(e, hipMemsetAsync(e->d_tmin + kTminEpsOffset, 0, sizeof(unsigned int) * (size_t)n_queries, e->stream));
    SCL_HIP(e, hipMemcpyAsync(approx, e->d_approx, sizeof(float) * (size_t)n * (size_t)n_queries, hipMemcpyDeviceToHost, e->stream));
    return sync(e);
}

int scl_detect_full(scl_engine *e, int cur, int *loop_id, int *nn_idx, int *shift, double *dist)
{
    if (!e || !loop_id || !nn_idx || !shift || !dist) return SCL_ERR_INVALID_ARG;
    *loop_id = -1;
    if (cur < 0) return SCL_ERR_OUT_OF_RANGE;
    const int hi = cur - e->cfg.num_exclude_recent;                       /* D.h:1627 */
    int rc = scl_detect_full_range(e, cur, 0, hi, nn_idx, shift, dist);
    if (rc) return rc;
    if (*nn_idx >= 0 && *dist < e->cfg.dist_thres) *loop_id = *nn_idx;
    return SCL_OK;
}
