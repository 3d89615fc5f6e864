// candidate_windows.hpp -- the keyframe windows of a list of loop candidates, and the slice of them that one round hands to the batched
// submap assembly (voxel.hip: assemble_submaps_batch).  Host code only (no HIP): registration.hip collects the windows from the keyframe
// store (kf_window) and slices them per round of kIcpBatch candidates; tests/cpp/candidate_windows_check.cpp checks the index
// arithmetic on its own, without a GPU.
#pragma once

#include <cstddef>
#include <vector>

namespace scl {

// Window w holds entries first_of[w] .. first_of[w + 1] - 1: a cloud (a device pointer, never read here), its point count and its 4 x 4
// pose.  A window may be empty (no keyframe of it exists in the store): its two offsets are equal.
struct CandidateWindows {
    std::vector<const void *> clouds;
    std::vector<int> counts;
    std::vector<float> poses;                              // 16 per entry
    std::vector<int> first_of = std::vector<int>(1, 0);

    int size() const { return (int)first_of.size() - 1; }  // windows
    int entries() const { return (int)clouds.size(); }

    // one more window: n entries
    void add(const void *const *cl, const int *cn, const float *T16, int n)
    {
        clouds.insert(clouds.end(), cl, cl + n);
        counts.insert(counts.end(), cn, cn + n);
        poses.insert(poses.end(), T16, T16 + 16 * (size_t)n);
        first_of.push_back(entries());
    }

    // what assemble_submaps_batch takes for one round: `jobs` windows back to back, window j at entries first[j] .. first[j + 1] - 1
    struct Round {
        std::vector<const void *> clouds;
        std::vector<int> counts, first = std::vector<int>(1, 0);
        std::vector<float> poses;
        int jobs = 0;

        void append(const CandidateWindows &w, int from, int n)          // windows from .. from + n - 1 of w, offsets rebased
        {
            const int p0 = w.first_of[(size_t)from], p1 = w.first_of[(size_t)(from + n)], base = first.back() - p0;
            clouds.insert(clouds.end(), w.clouds.begin() + p0, w.clouds.begin() + p1);
            counts.insert(counts.end(), w.counts.begin() + p0, w.counts.begin() + p1);
            poses.insert(poses.end(), w.poses.begin() + 16 * (size_t)p0, w.poses.begin() + 16 * (size_t)p1);
            for (int c = 1; c <= n; ++c) first.push_back(base + w.first_of[(size_t)(from + c)]);
            jobs += n;
        }
    };

    // candidates first .. first + m - 1 (m may be 0), behind lead's windows where there is a lead (the loop forms' own source,
    // loopFindNearKeyframes(cur, 0): one window, job 0 of the round)
    Round round(int first, int m, const CandidateWindows *lead = nullptr) const
    {
        Round r;
        if (lead) r.append(*lead, 0, lead->size());
        r.append(*this, first, m);
        return r;
    }
};

}  // namespace scl
