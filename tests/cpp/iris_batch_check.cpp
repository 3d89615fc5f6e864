// Drives the batch forms of the LiDAR-Iris adapter (include/scl/lidar_iris_hip_descriptor.hpp: makeAndSaveDescriptorsAndKeys,
// saveDescriptorsAndKeys, detectIntraLoopClosureIDs, detectInterLoopClosureIDs, makeSaveAndDetect) on an object a
// std::unique_ptr<scan_descriptor> owns, the way distributedMapping.h holds scanDescriptor, and compares every answer with loops
// over the six virtuals of a twin object fed the same scans.  Prints `ok iris:` lines; exit code 0 = all good
// (tests/test_gpu_iris_batch_adapter.py runs it).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "pcl_types_for_adapter_check.h"
#include "scl/lidar_iris_hip_descriptor.hpp"

typedef pcl::PointCloud<pcl::PointXYZI> Cloud;

static const int kRows = 16, kCols = 72, kValues = kRows * kCols + kRows;

// place `place` seen under heading `yaw`: walls at a few ranges and heights, the same for every visit of the place
static Cloud make_cloud(int place, float yaw, int n)
{
    std::mt19937_64 rng(1000 + (unsigned)place);
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    Cloud c;
    for (int i = 0; i < n; ++i) {
        pcl::PointXYZI p{};
        const float a = 6.2831853f * u(rng), sector = std::floor(a * 12.0f / 6.2831853f);
        const float range = 2.0f + std::fmod(sector * (3.0f + (float)place) * 1.7f, 13.0f) + 0.3f * u(rng);
        p.x = range * std::cos(a + yaw); p.y = range * std::sin(a + yaw); p.z = -1.0f + 4.0f * u(rng) * (0.3f + std::fmod(sector * 0.37f + 0.1f * (float)place, 0.7f));
        p.intensity = 1.0f;
        c.points.push_back(p);
    }
    return c;
}

static bool same(const std::pair<int, float> &a, const std::pair<int, float> &b)
{
    return a.first == b.first && std::memcmp(&a.second, &b.second, sizeof(float)) == 0;
}

static lidar_iris_hip_descriptor *make(int shiftSearch)
{
    // rows, cols, nscan, distThres, numExcludeRecent, matchNum, numCandidates, nscale, minWaveLength, mult, sigmaOnf, robotNum, thisID,
    // device, wireDecode, knnExcludeEps, shiftSearch
    return new lidar_iris_hip_descriptor(kRows, kCols, 64, 0.32, 4, 2, 3, 2, 18, 1.6f, 0.75f, 2, 0, 0, 1, FLT_EPSILON, shiftSearch);
}

static int check(const char *name, int shiftSearch, const std::vector<Cloud> &clouds)
{
    lidar_iris_hip_descriptor *impl = make(shiftSearch), *twin_impl = make(shiftSearch);
    std::unique_ptr<scan_descriptor> scanDescriptor(impl), twin(twin_impl);
    if (!impl->engine() || !twin_impl->engine()) { std::printf("FAIL %s create\n", name); return 1; }
    int fails = 0;
    const int n = (int)clouds.size();
    std::vector<int8_t> robot((size_t)n);
    for (int kf = 0; kf < n; ++kf) robot[(size_t)kf] = kf % 4 == 3 ? 1 : 0;
    // the scans in calls of 1, 16 and the rest: makeSaveAndDetect, makeAndSaveDescriptorsAndKeys, makeSaveAndDetect
    int at = 0, mine = 0, detected = 0, loops = 0;
    const int sizes[3] = {1, 16, n - 17};
    for (int s = 0; s < 3; ++s) {
        std::vector<const Cloud *> batch; std::vector<int8_t> robots; std::vector<int> indexs;
        for (int kf = at; kf < at + sizes[s]; ++kf) { batch.push_back(&clouds[(size_t)kf]); robots.push_back(robot[(size_t)kf]); indexs.push_back(kf); }
        std::vector<std::pair<int, float>> got;
        std::vector<float> values;
        if (s == 1) values = impl->makeAndSaveDescriptorsAndKeys(batch, robots, indexs);
        else { got = impl->makeSaveAndDetect(batch, robots, indexs); values = impl->lastDescriptors(); }
        if ((s != 1 && (int)got.size() != sizes[s]) || (int)values.size() != sizes[s] * kValues) { std::printf("FAIL %s batch build sizes\n", name); return 1; }
        for (int kf = at; kf < at + sizes[s]; ++kf) {
            const std::vector<float> v = twin->makeAndSaveDescriptorAndKey(clouds[(size_t)kf], robot[(size_t)kf], kf);
            if (std::memcmp(v.data(), values.data() + (size_t)(kf - at) * kValues, sizeof(float) * kValues) != 0) { std::printf("FAIL %s values %d\n", name, kf); ++fails; }
        }
        for (int kf = at; kf < at + sizes[s]; ++kf) {
            if (robot[(size_t)kf] != 0) {
                if (s != 1 && !same(got[(size_t)(kf - at)], std::pair<int, float>(-1, 0.0f))) { std::printf("FAIL %s other robot's entry %d\n", name, kf); ++fails; }
                continue;
            }
            if (s != 1) {
                const std::pair<int, float> want = twin->detectIntraLoopClosureID(mine);
                ++detected; loops += want.first >= 0;
                if (!same(got[(size_t)(kf - at)], want)) {
                    std::printf("FAIL %s makeSaveAndDetect %d: %d %g vs %d %g\n", name, kf, got[(size_t)(kf - at)].first, got[(size_t)(kf - at)].second, want.first, want.second);
                    ++fails;
                }
            }
            ++mine;
        }
        at += sizes[s];
    }
    // the first 20 descriptors again, as received from robot 1: saveDescriptorsAndKeys against a loop over saveDescriptorAndKey
    const int n_wire = 20;
    std::vector<float> wire;
    std::vector<int8_t> wrobots((size_t)n_wire, 1); std::vector<int> windexs;
    {
        lidar_iris_hip_descriptor *sender = make(shiftSearch);
        for (int k = 0; k < n_wire; ++k) {
            const std::vector<float> v = sender->makeAndSaveDescriptorAndKey(clouds[(size_t)k], 1, 100 + k);
            wire.insert(wire.end(), v.begin(), v.end()); windexs.push_back(100 + k);
        }
        sender->close(); delete sender;
    }
    impl->saveDescriptorsAndKeys(wire.data(), wrobots, windexs);
    for (int k = 0; k < n_wire; ++k) twin->saveDescriptorAndKey(wire.data() + (size_t)k * kValues, 1, 100 + k);
    const int total = n + n_wire;
    if (scanDescriptor->getSize() != total || twin->getSize() != total || scanDescriptor->getSize(0) != mine || scanDescriptor->getSize(1) != twin->getSize(1)) {
        std::printf("FAIL %s getSize\n", name); ++fails;
    }
    for (int key = 0; key < total; ++key)
        if (scanDescriptor->getIndex(key) != twin->getIndex(key)) { std::printf("FAIL %s getIndex %d\n", name, key); ++fails; }
    // all intra and inter queries at once, in descending and ascending order, against loops over the virtuals
    std::vector<int> locals, keys;
    for (int cur = mine - 1; cur >= 0; --cur) locals.push_back(cur);
    for (int cur = 0; cur < mine; ++cur) locals.push_back(cur);
    for (int key = 0; key < total; ++key) keys.push_back(key);
    for (int key = total - 1; key >= 0; --key) keys.push_back(key);
    const std::vector<std::pair<int, float>> intra = impl->detectIntraLoopClosureIDs(locals), inter = impl->detectInterLoopClosureIDs(keys);
    if (intra.size() != locals.size() || inter.size() != keys.size()) { std::printf("FAIL %s batch sizes\n", name); return 1; }
    int intra_loops = 0, inter_loops = 0;
    for (size_t i = 0; i < locals.size(); ++i) {
        const std::pair<int, float> want = twin->detectIntraLoopClosureID(locals[i]);
        intra_loops += want.first >= 0;
        if (!same(intra[i], want)) { std::printf("FAIL %s intra %d: %d %g vs %d %g\n", name, locals[i], intra[i].first, intra[i].second, want.first, want.second); ++fails; }
    }
    for (size_t i = 0; i < keys.size(); ++i) {
        const std::pair<int, float> want = twin->detectInterLoopClosureID(keys[i]);
        inter_loops += want.first >= 0;
        if (!same(inter[i], want)) { std::printf("FAIL %s inter %d: %d %g vs %d %g\n", name, keys[i], inter[i].first, inter[i].second, want.first, want.second); ++fails; }
    }
    if (intra_loops == 0 || inter_loops == 0) { std::printf("FAIL %s no loop found anywhere (%d intra, %d inter)\n", name, intra_loops, inter_loops); ++fails; }
    // afterwards the two objects are in one state: a further single call on each
    if (!same(scanDescriptor->detectInterLoopClosureID(total - 1), twin->detectInterLoopClosureID(total - 1))) { std::printf("FAIL %s state\n", name); ++fails; }
    // an out-of-range entry: every answer {-1, 0}, as the single calls report an error; mismatched sizes store nothing
    std::vector<int> bad = {0, 1, total, 2};
    const std::vector<std::pair<int, float>> none = impl->detectInterLoopClosureIDs(bad);
    for (size_t i = 0; i < none.size(); ++i)
        if (none[i].first != -1 || none[i].second != 0.0f) { std::printf("FAIL %s error answer\n", name); ++fails; }
    {
        std::vector<const Cloud *> batch(2, &clouds[0]);
        impl->makeSaveAndDetect(batch, std::vector<int8_t>(1, 0), std::vector<int>(2, 0));
        if (scanDescriptor->getSize() != total) { std::printf("FAIL %s size mismatch stored something\n", name); ++fails; }
    }
    impl->close(); twin_impl->close();
    if (!fails)
        std::printf("ok iris: %s: %d scans built in batches (%d detected, %d loops), %d received, %zu intra (%d loops) and %zu inter (%d loops) batched "
                    "queries equal the virtuals\n", name, n, detected, loops, n_wire, locals.size(), intra_loops, keys.size(), inter_loops);
    return fails;
}

int main(int argc, char **argv)
{
    const int n = argc > 1 ? std::atoi(argv[1]) : 44;
    if (n < 30) { std::printf("FAIL at least 30 keyframes\n"); return 1; }
    // 15 places walked, then walked again under other headings
    std::vector<Cloud> clouds;
    for (int kf = 0; kf < n; ++kf) clouds.push_back(make_cloud(kf % 15, kf < 15 ? 0.0f : 0.35f * (float)(kf / 15) + 0.01f * (float)(kf % 15), 3000 + 37 * (kf % 11)));
    int fails = 0;
    fails += check("windows", 0, clouds);
    fails += check("every shift", 1, clouds);
    std::printf(fails ? "FAILED %d\n" : "ALL OK\n", fails);
    return fails ? 1 : 0;
}
