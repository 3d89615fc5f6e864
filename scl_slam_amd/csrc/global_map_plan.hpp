// global_map_plan.hpp -- the host-only plan of the global voxel map (include/scl_engine.h "GLOBAL MAP"; kernels: global_map.hip): the
// key's layout and the table's hash, the capacity rule, what a set / remove call does to every listed keyframe (add, skip, re-pose),
// the jobs that follow from it and how they are cut into launch groups.  No HIP in here: tests/cpp/global_map_plan_check builds it
// with the host compiler under ASan + UBSan.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

namespace scl {
namespace gmap {

constexpr int kCoordBits = 21;                             // a voxel coordinate c in [-2^20, 2^20) travels as c + 2^20
constexpr long long kCoordBias = 1LL << 20;
constexpr unsigned long long kEmptyKey = ~0ULL;            // bit 63 set: no key has it (a key has 63 bits)
constexpr size_t kMinSlots = 16, kDefaultSlots = (size_t)1 << 20, kMaxSlots = (size_t)1 << 31;
constexpr int kMaxProbe = 128;                             // steps of linear probing before the kernel gives up and asks for a larger table
constexpr int kMaxJobs = 4096;                             // jobs of one launch group: their offsets live in 16 KB of LDS
constexpr long long kMaxGroupPoints = 1LL << 30;           // points of one launch group (a single larger keyframe is a group of its own)

inline unsigned long long make_key(long long cx, long long cy, long long cz)
{
    return ((unsigned long long)(cz + kCoordBias) << (2 * kCoordBits)) | ((unsigned long long)(cy + kCoordBias) << kCoordBits) |
           (unsigned long long)(cx + kCoordBias);
}

// the table's hash (splitmix64's finaliser); a key's first slot is hash & (capacity - 1)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline unsigned long long hash_key(unsigned long long x)
{
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ULL;
    x ^= x >> 27; x *= 0x94d049bb133111ebULL;
    x ^= x >> 31;
    return x;
}

// The capacity rule.  A table is a power of two of slots and is never more than half full: capacity_for(n) is the smallest power of
// two >= max(kMinSlots, 2 n), formed in 64 bits (2^31 points ask for 2^32 slots, which the caller refuses: > kMaxSlots).
inline unsigned long long capacity_for(unsigned long long occupied)
{
    unsigned long long c = kMinSlots;
    while (c < 2 * occupied && c < (1ULL << 62)) c <<= 1;
    return c;
}
inline bool over_load(unsigned long long used_slots, unsigned long long capacity) { return 2 * used_slots > capacity; }
// inserts a reserve pass may still make before the table is more than half full
inline unsigned long long room(unsigned long long used_slots, unsigned long long capacity) { return 2 * used_slots >= capacity ? 0 : capacity / 2 - used_slots; }
// the capacity a reset starts at: the test hook's figure (0: none) rounded up to a power of two, else the default
inline unsigned long long start_capacity(unsigned long long hook_slots)
{
    if (hook_slots == 0) return kDefaultSlots;
    unsigned long long c = kMinSlots;
    while (c < hook_slots && c < kMaxSlots) c <<= 1;
    return c;
}
// the capacity after a growth: twice the old one, and never below the load bound of what the table holds now
inline unsigned long long grown_capacity(unsigned long long capacity, unsigned long long used_slots)
{
    const unsigned long long a = 2 * capacity, b = capacity_for(used_slots);
    return a > b ? a : b;
}
// steps a probe may take in a table of that capacity
inline int probe_limit(unsigned long long capacity) { return capacity < (unsigned long long)kMaxProbe ? (int)capacity : kMaxProbe; }

struct KeyframeId {
    int robot, index;
    bool operator<(const KeyframeId &o) const { return robot != o.robot ? robot < o.robot : index < o.index; }
};
// what the map remembers of an integrated keyframe: the 7 doubles it was placed at, bit for bit, and the generation of the stored cloud
struct Entry { double pose[7]; uint64_t generation; };
using Entries = std::map<KeyframeId, Entry>;

// one pass of one stored cloud through the integration kernel: item = position in the call's list, sign +1 adds, -1 subtracts
struct Job { int item; int sign; double pose[7]; };
enum Action { kSkip = 0, kAdd = 1, kRepose = 2 };

inline const char *pose_bad(const double *p)
{
    for (int k = 0; k < 7; ++k) if (!std::isfinite(p[k])) return "a pose is not finite";
    const double n2 = p[3] * p[3] + p[4] * p[4] + p[5] * p[5] + p[6] * p[6];
    if (!(n2 >= 0.25 && n2 <= 4.0)) return "a quaternion's squared norm is outside [0.25, 4]";
    return nullptr;
}

inline const char *duplicate_bad(const int *robots, const int *indices, int n)
{
    std::vector<KeyframeId> ids((size_t)(n > 0 ? n : 0));
    for (int i = 0; i < n; ++i) ids[(size_t)i] = {robots[i], indices[i]};
    std::vector<KeyframeId> s(ids);
    std::sort(s.begin(), s.end());
    for (size_t i = 1; i < s.size(); ++i)
        if (!(s[i - 1] < s[i])) return "a keyframe is listed twice";
    return nullptr;
}

// The diff of a set call.  generations[i] = the generation of keyframe i's cloud in the store now.  Returns nullptr and fills
// actions (one per listed keyframe) and jobs (a re-pose: the subtraction at the old pose, then the addition at the new one), or says
// what is wrong; nothing is written then.
inline const char *plan_set(const Entries &entries, const int *robots, const int *indices, const double *poses, const uint64_t *generations, int n,
                            std::vector<int> *actions, std::vector<Job> *jobs)
{
    for (int i = 0; i < n; ++i) if (const char *bad = pose_bad(poses + 7 * (size_t)i)) return bad;
    if (const char *bad = duplicate_bad(robots, indices, n)) return bad;
    std::vector<int> act; std::vector<Job> out;
    for (int i = 0; i < n; ++i) {
        const double *p = poses + 7 * (size_t)i;
        const auto it = entries.find({robots[i], indices[i]});
        Job add{i, +1, {0}};
        std::memcpy(add.pose, p, sizeof add.pose);
        if (it == entries.end()) { act.push_back(kAdd); out.push_back(add); continue; }
        if (it->second.generation != generations[i]) return "a listed keyframe's stored cloud was replaced since it was integrated: reset the map";
        if (std::memcmp(it->second.pose, p, sizeof add.pose) == 0) { act.push_back(kSkip); continue; }
        Job sub{i, -1, {0}};
        std::memcpy(sub.pose, it->second.pose, sizeof sub.pose);
        act.push_back(kRepose); out.push_back(sub); out.push_back(add);
    }
    actions->swap(act); jobs->swap(out);
    return nullptr;
}

inline const char *plan_remove(const Entries &entries, const int *robots, const int *indices, const uint64_t *generations, int n, std::vector<Job> *jobs)
{
    if (const char *bad = duplicate_bad(robots, indices, n)) return bad;
    std::vector<Job> out;
    for (int i = 0; i < n; ++i) {
        const auto it = entries.find({robots[i], indices[i]});
        if (it == entries.end()) return "a listed keyframe is not in the map";
        if (it->second.generation != generations[i]) return "a listed keyframe's stored cloud was replaced since it was integrated: reset the map";
        Job sub{i, -1, {0}};
        std::memcpy(sub.pose, it->second.pose, sizeof sub.pose);
        out.push_back(sub);
    }
    jobs->swap(out);
    return nullptr;
}

// Launch groups: jobs [first[g], first[g + 1]) run in one launch; offsets[j] = points of the group's jobs before job j (the kernel's
// threads find their job by bisection of them).  A group holds at most kMaxJobs jobs and kMaxGroupPoints points, or one larger job.
inline void plan_groups(const int *counts, int n_jobs, std::vector<int> *first, std::vector<int> *offsets, int max_jobs = kMaxJobs,
                        long long max_points = kMaxGroupPoints)
{
    first->assign(1, 0);
    offsets->assign((size_t)(n_jobs > 0 ? n_jobs : 0), 0);
    long long pts = 0; int in_group = 0;
    for (int j = 0; j < n_jobs; ++j) {
        if (in_group > 0 && (in_group == max_jobs || pts + (long long)counts[j] > max_points)) { first->push_back(j); pts = 0; in_group = 0; }
        (*offsets)[(size_t)j] = (int)pts;
        pts += (long long)counts[j];
        ++in_group;
    }
    if (n_jobs > 0) first->push_back(n_jobs);
}

}  // namespace gmap
}  // namespace scl
