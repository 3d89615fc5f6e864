// global_map.hpp -- the persistent global voxel map on the device (host-side interface used by global_map.hip's entry points; contract:
// include/scl_engine.h "GLOBAL MAP"; the host-only plan: global_map_plan.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "global_map_plan.hpp"
#include "scl_engine.h"

namespace scl {

// one pass of one stored cloud (device pointer, n points of the store's stride) through the integration kernel
struct MapPass { const unsigned char *cloud; int n; int sign; double pose[7]; };

struct GlobalMap {
    bool exists = false;
    float leaf = 0.0f;
    void *table = nullptr;                                  // capacity slots of 64 bytes (global_map.hip: MapSlot)
    unsigned long long capacity = 0, used_slots = 0;        // slots that hold a key (a voxel emptied since still holds its slot until a growth)
    unsigned long long points_added = 0, points_skipped = 0, growths = 0;   // net of removals
    unsigned long long next_start_slots = 0;                // scl_selftest_map_capacity: the next reset's starting capacity (0: the default)
    gmap::Entries entries;
    unsigned long long *d_ctl = nullptr, *h_ctl = nullptr;  // control words (device) and their pinned copy
    void *buf[8] = {nullptr}; size_t cap[8] = {0};          // grow-only: a group's jobs and offsets, the extraction's keys / values (two of each), scratch, records
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    double ms[3] = {0.0, 0.0, 0.0};                         // integrate, grow, extract of the last timed call
};

void map_free(GlobalMap *m);
int map_reset(GlobalMap *m, hipStream_t stream, float leaf, std::string *err);
// every pass applied, in launch groups; the table grows as it must.  A group that fails (no memory for a larger table) leaves the sums
// as they were before it -- a reserve pass only inserts keys, and a key without points is not part of the map --, the groups before it
// stay applied: the caller invalidates the map
int map_apply(GlobalMap *m, hipStream_t stream, const MapPass *passes, int n_passes, int stride, bool timing, std::string *err);
int map_count(GlobalMap *m, hipStream_t stream, unsigned long long *occupied, std::string *err);
int map_extract(GlobalMap *m, hipStream_t stream, const double *box, void *out, int out_capacity, int *n_out, bool timing, std::string *err);

}  // namespace scl
