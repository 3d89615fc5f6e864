// screen_plan.hpp -- the launch SCHEDULE of one chunk of the screened stream form (screen_host.hip: stream_screened_locked), host code
// only (no HIP): which launch groups of the chunk go as pairs, which group aligns for itself, whose alignment rides in whose tail, and
// when a tail's alignment reaches into the next chunk's buffer sets.  It is decided here from five integers, so that
// tests/cpp/screen_plan_check.cpp can check it on its own, under ASan / UBSan and without a GPU; the stream's submit walks the units and
// issues the HIP calls.
//
// A chunk's scans that have something to score form its list [0, cur_m); the list of the chunk behind it continues the numbering,
// [cur_m, cur_m + nxt_m) (nxt_m == 0: there is no such chunk, or it has nothing to score).  A launch GROUP is up to `spl` consecutive
// scans of ONE list -- one screening launch's worth, one buffer set per scan.  Every group needs its alignment (the first shifts of its
// pairs) before its products, and gets it from one of three places: the tail of a launch in front of it (the rule: a launch carries the
// alignment of what follows it, so the device never waits between two launches), the chunk before (aligned_in leading scans), or itself
// (a launch of its own in front of its products: the call's very first group, and the groups behind a unit that a tail skipped).
#pragma once

namespace scl {

constexpr int kPlanPairGroup = 16;      // scans of each of the two groups that share a products launch (kernels.hpp: kMaxScreenBatch)

struct PlanGroup { int off, nq; };      // scans [off, off + nq) of the numbering above; nq == 0: none

// One step of the schedule: ONE products launch with its tail(s)
struct PlanUnit {
    PlanGroup g0, g1;                   // the scans the launch scores; g1.nq > 0: two full groups of this chunk go as a pair (one pass over the database)
    PlanGroup n0, n1;                   // the groups whose alignment rides in the tail of g0 / g1 (n1 only behind a pair, for the pair that follows)
    bool align0, align1;                // g0 / g1 aligns for itself, in a launch in front of this one
    int over;                           // > 0: the tails' alignment reaches this many scans into the NEXT chunk's list, whose buffer sets the exact
                                        // pass of the chunk before this one may still be reading: the main stream waits for that pass first
};

// The units of a chunk, in launch order, into units[0 .. cur_m) at most; returns their number.
//   spl          scans per launch group (>= 1)
//   pairs        two consecutive FULL groups (kPlanPairGroup scans each) of one chunk share a products launch; a pair's two tails carry
//                the alignment of the pair behind it -- two groups ahead instead of one --, and whatever follows a pair and is no pair
//                is aligned by the first tail
//   aligned_in   leading scans of this chunk's list that the chunk before aligned (its *next_aligned)
//   next_aligned leading scans of the next chunk's list that this chunk's tails align
inline int plan_chunk(int cur_m, int nxt_m, int spl, bool pairs, int aligned_in, PlanUnit *units, int *next_aligned)
{
    const int all_m = cur_m + nxt_m;
    // the group that starts at scan `off`: it ends with its list ({0, 0} past the end of both)
    auto group_at = [&](int off) {
        const int end = off < cur_m ? cur_m : all_m;
        if (off >= end) return PlanGroup{0, 0};
        return PlanGroup{off, end - off < spl ? end - off : spl};
    };
    auto pair_at = [&](int off) { return pairs && group_at(off).nq == kPlanPairGroup && group_at(off + kPlanPairGroup).nq == kPlanPairGroup &&
                                         (off + 2 * kPlanPairGroup <= cur_m || off >= cur_m); };   // (both in ONE chunk)
    int n_units = 0, aligned_to = aligned_in;              // scans [0, aligned_to) have their first shifts (or will have, in stream order)
    for (int g = 0; g < cur_m;) {
        PlanUnit &u = units[n_units++];
        const bool pair = pair_at(g);
        u.g0 = group_at(g);
        u.g1 = pair ? group_at(g + u.g0.nq) : PlanGroup{0, 0};
        const int end = g + u.g0.nq + u.g1.nq;
        u.n0 = u.n1 = PlanGroup{0, 0};
        if (end >= aligned_to) {                           // what the tails align: the group(s) behind this unit, unless a tail before did
            u.n0 = group_at(end);
            if (pair && pair_at(end)) u.n1 = group_at(end + u.n0.nq);
        }
        const int reach = end + u.n0.nq + u.n1.nq;
        u.over = (reach > cur_m && u.n0.nq > 0) ? reach - cur_m : 0;
        u.align0 = g >= aligned_to;
        u.align1 = pair && g + u.g0.nq >= aligned_to;
        if (reach > aligned_to) aligned_to = reach;
        g = end;
    }
    *next_aligned = aligned_to > cur_m ? aligned_to - cur_m : 0;
    return n_units;
}

}  // namespace scl
