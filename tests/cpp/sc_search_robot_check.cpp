// Drives the per-robot ranked searches of the Scan Context adapter (include/scl/scan_context_hip_descriptor.hpp:
// searchIntraLoopClosureIDs, searchInterLoopClosureIDs) on an object a std::unique_ptr<scan_descriptor> owns, the way
// distributedMapping.h holds scanDescriptor, and compares every list with the C calls (scl_sc_search_intra, scl_sc_search_inter) on
// the engine of a twin object fed the same descriptors: three robots whose keyframes interleave slot by slot.  Arguments:
// <keyframes> <shards>.  Prints `ok sc:` lines; exit code 0 = all good (tests/test_gpu_sc_search_robot_adapter.py runs it).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "pcl_types_for_adapter_check.h"
#include "scl/scan_context_hip_descriptor.hpp"

typedef std::vector<std::vector<scan_context_hip_descriptor::LoopCandidate>> Lists;

static const int kRing = 20, kSector = 60, kExclude = 10, kRobots = 3;

// the wire descriptor (ring-major, descriptor.h:1446-1455) of place `place` seen under a heading of `turn` sectors
static std::vector<float> make_descriptor(int place, int turn)
{
    std::mt19937_64 rng(4000 + (unsigned)place);
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    std::vector<float> base((size_t)kRing * kSector), v(base.size());
    for (size_t c = 0; c < base.size(); ++c) base[c] = u(rng) < 0.35f ? 0.0f : 6.0f * u(rng);
    for (int r = 0; r < kRing; ++r)
        for (int s = 0; s < kSector; ++s) v[(size_t)r * kSector + (size_t)((s + turn) % kSector)] = base[(size_t)r * kSector + s];
    return v;
}

static scan_context_hip_descriptor *make(int shards)
{
    // numRing, numSector, numCandidates, distThres, lidarHeight, maxRadius, numExcludeRecent
    if (shards > 0) return new scan_context_hip_descriptor(std::vector<int>((size_t)shards, 0), kRing, kSector, 3, 0.14, 1.65, 80.0, kExclude);
    return new scan_context_hip_descriptor(kRing, kSector, 3, 0.14, 1.65, 80.0, kExclude);
}

// the adapter's lists against the C call's arrays: n_found entries per query, ids equal, the shift as a float, distances by their bits
static int compare(const char *what, int k, const Lists &got, const std::vector<int> &ids, const std::vector<int> &shifts, const std::vector<double> &dists,
                   const std::vector<int> &found)
{
    int fails = 0;
    if (got.size() != found.size()) { std::printf("FAIL %s k=%d: %zu lists for %zu queries\n", what, k, got.size(), found.size()); return 1; }
    for (size_t i = 0; i < got.size(); ++i) {
        if ((int)got[i].size() != found[i]) { std::printf("FAIL %s k=%d query %zu: %zu entries, n_found %d\n", what, k, i, got[i].size(), found[i]); ++fails; continue; }
        for (int j = 0; j < found[i]; ++j) {
            const scan_context_hip_descriptor::LoopCandidate &c = got[i][(size_t)j];
            if (c.id != ids[i * k + j] || c.shift != (float)shifts[i * k + j] || std::memcmp(&c.dist, &dists[i * k + j], sizeof(double)) != 0) {
                std::printf("FAIL %s k=%d query %zu entry %d\n", what, k, i, j);
                ++fails;
            }
        }
    }
    return fails;
}

// every list ascending by (distance, id) and inside the set `member` describes
template <class Member>
static bool lists_ok(const Lists &got, const std::vector<int> &curs, Member member, int *listed)
{
    bool ok = true;
    *listed = 0;
    for (size_t i = 0; i < got.size(); ++i) {
        *listed += (int)got[i].size();
        for (size_t j = 1; j < got[i].size(); ++j) ok &= got[i][j - 1].dist < got[i][j].dist || (got[i][j - 1].dist == got[i][j].dist && got[i][j - 1].id < got[i][j].id);
        for (size_t j = 0; j < got[i].size(); ++j) ok &= member(curs[i], got[i][j].id);
    }
    return ok;
}

int main(int argc, char **argv)
{
    const int n = argc > 1 ? std::atoi(argv[1]) : 90;
    const int shards = argc > 2 ? std::atoi(argv[2]) : 0;             // 0 = the one-GPU constructor, G > 0 = G shards, all on device 0
    if (n < 60) { std::printf("FAIL at least 60 keyframes\n"); return 1; }
    scan_context_hip_descriptor *impl = make(shards), *twin_impl = make(shards);
    std::unique_ptr<scan_descriptor> scanDescriptor(impl), twin(twin_impl);
    if (!impl->engine() || !twin_impl->engine()) { std::printf("FAIL create\n"); return 1; }
    for (int kf = 0; kf < n; ++kf) {                                   // 30 places, revisited under other headings; slot kf = keyframe kf / 3 of robot kf % 3
        const std::vector<float> v = make_descriptor(kf % 30, kf < 30 ? 0 : 7 * (kf / 30) + kf % 3);
        scanDescriptor->saveDescriptorAndKey(v.data(), (int8_t)(kf % kRobots), kf / kRobots);
        twin->saveDescriptorAndKey(v.data(), (int8_t)(kf % kRobots), kf / kRobots);
    }
    if (scanDescriptor->getSize() != n) { std::printf("FAIL size\n"); return 1; }
    int fails = 0;
    std::vector<int> curs;
    for (int cur = n - 1; cur >= 0; cur -= 4) curs.push_back(cur);      // (robots alternate; the oldest ones search an empty intra set)
    const int nq = (int)curs.size();
    const int ks[3] = {1, 5, SCL_SC_SEARCH_MAX};
    for (int t = 0; t < 3; ++t) {
        const int k = ks[t];
        std::vector<int> ids(curs.size() * k, -7), shifts(ids.size(), -7), found(curs.size(), -7);
        std::vector<double> dists(ids.size(), -7.0);
        int listed = 0;
        {
            const Lists got = impl->searchIntraLoopClosureIDs(curs, k);
            if (scl_sc_search_intra(twin_impl->engine(), curs.data(), nq, k, ids.data(), shifts.data(), dists.data(), found.data()) != SCL_OK) { std::printf("FAIL C call\n"); return 1; }
            const int f = compare("intra", k, got, ids, shifts, dists, found);
            const bool ok = lists_ok(got, curs, [](int cur, int id) { return id >= 0 && id % kRobots == cur % kRobots && id / kRobots < cur / kRobots - kExclude; }, &listed);
            if (!listed) { std::printf("FAIL intra k=%d nothing listed\n", k); ++fails; }
            if (!ok) { std::printf("FAIL intra k=%d a list out of order or out of its search set\n", k); ++fails; }
            if (!f && listed && ok) std::printf("ok sc: the intra lists of %d queries at k = %d (%d entries) equal the C call\n", nq, k, listed);
            fails += f;
        }
        {
            const Lists got = impl->searchInterLoopClosureIDs(curs, k);
            if (scl_sc_search_inter(twin_impl->engine(), curs.data(), nq, SCL_SC_ANY_OTHER_ROBOT, k, ids.data(), shifts.data(), dists.data(), found.data()) != SCL_OK) { std::printf("FAIL C call\n"); return 1; }
            const int f = compare("inter", k, got, ids, shifts, dists, found);
            const bool ok = lists_ok(got, curs, [](int cur, int id) { return id >= 0 && id % kRobots != cur % kRobots; }, &listed);
            if (!listed) { std::printf("FAIL inter k=%d nothing listed\n", k); ++fails; }
            if (!ok) { std::printf("FAIL inter k=%d a list out of order or out of its search set\n", k); ++fails; }
            if (!f && listed && ok) std::printf("ok sc: the inter lists (any other robot) of %d queries at k = %d (%d entries) equal the C call\n", nq, k, listed);
            fails += f;
        }
        for (int pre = 0; pre < kRobots; ++pre) {                        // one named robot: the queries of the other two
            std::vector<int> sub;
            for (int cur : curs) if (cur % kRobots != pre) sub.push_back(cur);
            const Lists got = impl->searchInterLoopClosureIDs(sub, k, pre);
            ids.assign(sub.size() * k, -7); shifts.assign(ids.size(), -7); dists.assign(ids.size(), -7.0); found.assign(sub.size(), -7);
            if (scl_sc_search_inter(twin_impl->engine(), sub.data(), (int)sub.size(), pre, k, ids.data(), shifts.data(), dists.data(), found.data()) != SCL_OK) { std::printf("FAIL C call\n"); return 1; }
            const int f = compare("inter robotPre", k, got, ids, shifts, dists, found);
            const bool ok = lists_ok(got, sub, [pre](int, int id) { return id >= 0 && id % kRobots == pre; }, &listed);
            if (!listed) { std::printf("FAIL inter robotPre=%d k=%d nothing listed\n", pre, k); ++fails; }
            if (!ok) { std::printf("FAIL inter robotPre=%d k=%d a list out of order or out of its search set\n", pre, k); ++fails; }
            if (!f && listed && ok) std::printf("ok sc: the inter lists (robot %d) of %zu queries at k = %d (%d entries) equal the C call\n", pre, sub.size(), k, listed);
            fails += f;
        }
    }
    // afterwards the two objects are in one state: a further single call on each
    const std::pair<int, float> a = scanDescriptor->detectIntraLoopClosureID(n - 1), b = twin->detectIntraLoopClosureID(n - 1);
    if (a.first != b.first || std::memcmp(&a.second, &b.second, sizeof(float)) != 0) { std::printf("FAIL state\n"); ++fails; }
    // a k outside [1, SCL_SC_SEARCH_MAX], an out-of-range entry, a robotPre out of range or the robot of an entry: one empty list per query
    std::vector<int> bad = {n - 1, n - 2, n, n - 3};
    const Lists none[7] = {impl->searchIntraLoopClosureIDs(curs, 0), impl->searchInterLoopClosureIDs(curs, SCL_SC_SEARCH_MAX + 1), impl->searchIntraLoopClosureIDs(bad, 5),
                           impl->searchInterLoopClosureIDs(bad, 5), impl->searchInterLoopClosureIDs(curs, 5, 128), impl->searchInterLoopClosureIDs(curs, 5, -2),
                           impl->searchInterLoopClosureIDs(curs, 5, curs[0] % kRobots)};
    const size_t sizes[7] = {curs.size(), curs.size(), bad.size(), bad.size(), curs.size(), curs.size(), curs.size()};
    int errors_ok = 1;
    for (int t = 0; t < 7; ++t) {
        if (none[t].size() != sizes[t]) { std::printf("FAIL error answer size\n"); ++fails; errors_ok = 0; }
        for (size_t i = 0; i < none[t].size(); ++i)
            if (!none[t][i].empty()) { std::printf("FAIL error answer\n"); ++fails; errors_ok = 0; }
    }
    if (errors_ok) std::printf("ok sc: k = 0, k = %d, a query out of range and a robotPre out of range or of a query answer one empty list per query\n", SCL_SC_SEARCH_MAX + 1);
    impl->close(); twin_impl->close();
    std::printf(fails ? "FAILED %d\n" : "ALL OK\n", fails);
    return fails ? 1 : 0;
}
