// ingest_plan.hpp -- how one GROUP of clouds of the points pipeline (ingest_host.hip: points_pipeline_locked) travels to the device, host
// code only (no HIP).  The clouds' host addresses come in as integers, so nothing here compares or subtracts pointers of unrelated
// allocations, and tests/cpp/ingest_plan_check.cpp checks the decision on its own, under ASan / UBSan and without a GPU; the pipeline
// computes every group's plan once per call and issues the copies from it.
//
// A group's clouds lie at 256-byte aligned offsets of one device buffer, each with 16 bytes behind it -- unless they lie one behind the
// other in ONE host allocation (a ring of incoming scans, an arena the host assembles its clouds in): at least two clouds, none empty,
// ascending addresses, 16-byte aligned distances from the first, gaps below a page (a gap below a page lies in pages the clouds
// themselves touch).  Such a group travels as ONE copy of its whole span -- at the link's rate for large copies (56.8 GB/s) instead of
// sixteen start-ups (44.8 GB/s on one stream) -- and lies on the device as it lay on the host.
#pragma once

#include <cstddef>
#include <cstdint>

namespace scl {

constexpr int kPlanCopyGroup = 16;      // clouds of a group at most (kernels.hpp: kMaxScBatch)

struct GroupCopyPlan {
    bool merged;                        // one copy of span - 16 bytes from the first cloud's address
    size_t span;                        // bytes of the device buffer the group needs
    size_t off[kPlanCopyGroup];         // where cloud i0 + j lies in the buffer (merged: its distance from the first cloud)
};

// the group of clouds [i0, i1) of a call (1 <= i1 - i0 <= kPlanCopyGroup): cloud i at addr[i] with n_points[i] points of `stride` bytes
inline GroupCopyPlan plan_group_copy(const uintptr_t *addr, const int *n_points, int stride, int i0, int i1)
{
    GroupCopyPlan p{};
    p.merged = i1 - i0 >= 2;
    const uintptr_t base = addr[i0];
    uintptr_t end = base;
    for (int i = i0; p.merged && i < i1; ++i) {
        const uintptr_t c = addr[i];
        const size_t bytes = (size_t)n_points[i] * (size_t)stride;
        if (!c || bytes == 0 || c < end || c - end >= 4096 || ((c - base) & 15)) p.merged = false;
        else end = c + bytes;
    }
    if (p.merged) {
        for (int i = i0; i < i1; ++i) p.off[i - i0] = (size_t)(addr[i] - base);
        p.span = (size_t)(end - base) + 16;
        return p;
    }
    for (int i = i0; i < i1; ++i) {
        p.off[i - i0] = p.span;
        p.span += (((size_t)n_points[i] * (size_t)stride + 16) + 255) & ~(size_t)255;
    }
    return p;
}

}  // namespace scl
