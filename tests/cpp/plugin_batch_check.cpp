// Drives the batch forms of the M2DP, FPFH and GRSD adapters (include/scl/{m2dp,fpfh,grsd}_hip_descriptor.hpp:
// detectIntraLoopClosureIDs, detectInterLoopClosureIDs, makeSaveAndDetect) on objects a std::unique_ptr<scan_descriptor> owns, the
// way distributedMapping.h holds scanDescriptor, and compares every answer with loops over the virtuals of a twin object fed the
// same scans.  Prints one `ok` line per adapter; exit code 0 = all good (tests/test_gpu_plugin_batch_adapter.py runs it).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "pcl_types_for_adapter_check.h"
#include "scl/fpfh_hip_descriptor.hpp"
#include "scl/grsd_hip_descriptor.hpp"
#include "scl/m2dp_hip_descriptor.hpp"

typedef pcl::PointCloud<pcl::PointXYZI> Cloud;

static Cloud make_cloud(std::mt19937_64 &rng, int n, float yaw, float dx)
{
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    Cloud c;
    const float cs = std::cos(yaw), sn = std::sin(yaw);
    for (int i = 0; i < n; ++i) {
        pcl::PointXYZI p{};
        const float x = 40.0f * u(rng), y = 15.0f * u(rng), z = 3.0f * u(rng) + 0.1f * x;
        p.x = cs * x - sn * y + dx; p.y = sn * x + cs * y; p.z = z; p.intensity = 1.0f;
        c.points.push_back(p);
    }
    return c;
}

static bool same(const std::pair<int, float> &a, const std::pair<int, float> &b)
{
    return a.first == b.first && std::memcmp(&a.second, &b.second, sizeof(float)) == 0;
}

// Adapter: the class under test; impl / twin: two objects with one configuration
template <class Adapter> static int check(const char *name, Adapter *impl, Adapter *twin_impl, const std::vector<Cloud> &clouds, int dim)
{
    std::unique_ptr<scan_descriptor> scanDescriptor(impl), twin(twin_impl);
    if (!impl->engine() || !twin_impl->engine()) { std::printf("FAIL %s create\n", name); return 1; }
    int fails = 0;
    const int n = (int)clouds.size();
    // the scans in calls of 1, 16 and the rest; every fourth keyframe is robot 1's
    std::vector<int8_t> robot((size_t)n);
    for (int kf = 0; kf < n; ++kf) robot[(size_t)kf] = kf % 4 == 3 ? 1 : 0;
    int at = 0, mine = 0, detected = 0;
    const int sizes[3] = {1, 16, n - 17};
    for (int s = 0; s < 3; ++s) {
        std::vector<const Cloud *> batch; std::vector<int8_t> robots; std::vector<int> indexs;
        for (int kf = at; kf < at + sizes[s]; ++kf) { batch.push_back(&clouds[(size_t)kf]); robots.push_back(robot[(size_t)kf]); indexs.push_back(kf); }
        const std::vector<std::pair<int, float>> got = impl->makeSaveAndDetect(batch, robots, indexs);
        const std::vector<float> &values = impl->lastDescriptors();
        if ((int)got.size() != sizes[s] || (int)values.size() != sizes[s] * dim) { std::printf("FAIL %s makeSaveAndDetect sizes\n", name); return 1; }
        for (int kf = at; kf < at + sizes[s]; ++kf) {
            const std::vector<float> v = twin->makeAndSaveDescriptorAndKey(clouds[(size_t)kf], robot[(size_t)kf], kf);
            if (std::memcmp(v.data(), values.data() + (size_t)(kf - at) * dim, sizeof(float) * dim) != 0) { std::printf("FAIL %s values %d\n", name, kf); ++fails; }
        }
        for (int kf = at; kf < at + sizes[s]; ++kf) {
            const std::pair<int, float> want = robot[(size_t)kf] == 0 ? twin->detectIntraLoopClosureID(mine) : std::pair<int, float>(-1, INFINITY);
            if (robot[(size_t)kf] == 0) { ++mine; ++detected; }
            if (!same(got[(size_t)(kf - at)], want)) {
                std::printf("FAIL %s makeSaveAndDetect %d: %d %g vs %d %g\n", name, kf, got[(size_t)(kf - at)].first, got[(size_t)(kf - at)].second, want.first, want.second);
                ++fails;
            }
        }
        at += sizes[s];
    }
    if (scanDescriptor->getSize() != n || twin->getSize() != n || scanDescriptor->getSize(0) != mine) { std::printf("FAIL %s getSize\n", name); ++fails; }
    // all intra and inter queries at once, in descending and ascending order, against loops over the virtuals
    std::vector<int> locals, keys;
    for (int cur = mine - 1; cur >= 0; --cur) locals.push_back(cur);
    for (int cur = 0; cur < mine; ++cur) locals.push_back(cur);
    for (int key = 0; key < n; ++key) keys.push_back(key);
    for (int key = n - 1; key >= 0; --key) keys.push_back(key);
    const std::vector<std::pair<int, float>> intra = impl->detectIntraLoopClosureIDs(locals), inter = impl->detectInterLoopClosureIDs(keys);
    if (intra.size() != locals.size() || inter.size() != keys.size()) { std::printf("FAIL %s batch sizes\n", name); return 1; }
    for (size_t i = 0; i < locals.size(); ++i)
        if (!same(intra[i], twin->detectIntraLoopClosureID(locals[i]))) { std::printf("FAIL %s intra %d\n", name, locals[i]); ++fails; }
    for (size_t i = 0; i < keys.size(); ++i)
        if (!same(inter[i], twin->detectInterLoopClosureID(keys[i]))) { std::printf("FAIL %s inter %d\n", name, keys[i]); ++fails; }
    // afterwards the two objects are in one state: a further single call on each
    if (!same(scanDescriptor->detectInterLoopClosureID(n - 1), twin->detectInterLoopClosureID(n - 1))) { std::printf("FAIL %s state\n", name); ++fails; }
    // an out-of-range entry: every answer {-1, 0}, as the single calls report an error
    std::vector<int> bad = {0, 1, n, 2};
    const std::vector<std::pair<int, float>> none = impl->detectInterLoopClosureIDs(bad);
    for (size_t i = 0; i < none.size(); ++i)
        if (none[i].first != -1 || none[i].second != 0.0f) { std::printf("FAIL %s error answer\n", name); ++fails; }
    impl->close(); twin_impl->close();
    if (!fails)
        std::printf("ok %s: makeSaveAndDetect of %d scans (%d detected), %zu intra and %zu inter batched queries equal the virtuals\n", name, n,
                    detected, locals.size(), keys.size());
    return fails;
}

int main(int argc, char **argv)
{
    const int n = argc > 1 ? std::atoi(argv[1]) : 44;
    if (n < 20) { std::printf("FAIL at least 20 keyframes\n"); return 1; }
    std::mt19937_64 rng(23);
    std::vector<Cloud> clouds;
    for (int kf = 0; kf < n; ++kf) clouds.push_back(make_cloud(rng, 3000 + 37 * (kf % 11), 0.1f * (kf % 11), 0.05f * (kf % 11)));
    int fails = 0;
    {
        fails += check("m2dp", new m2dp_hip_descriptor(0.3, 4, 2, 0), new m2dp_hip_descriptor(0.3, 4, 2, 0), clouds, SCL_M2DP_DIM);
    }
    {
        scl_fpfh_config cfg; scl_fpfh_default_config(&cfg);
        cfg.num_exclude_recent = 4; cfg.tree_making_period = 3; cfg.robot_num = 2; cfg.this_id = 0;
        fails += check("fpfh", new fpfh_hip_descriptor(cfg), new fpfh_hip_descriptor(cfg), clouds, SCL_FPFH_DIM);
    }
    {
        scl_grsd_config cfg; scl_grsd_default_config(&cfg);
        cfg.num_exclude_recent = 4; cfg.tree_making_period = 3; cfg.robot_num = 2; cfg.this_id = 0;
        fails += check("grsd", new grsd_hip_descriptor(cfg), new grsd_hip_descriptor(cfg), clouds, SCL_GRSD_DIM);
    }
    std::printf(fails ? "FAILED %d\n" : "ALL OK\n", fails);
    return fails ? 1 : 0;
}
