// Drives the exhaustive ranked search of the LiDAR-Iris adapter (include/scl/lidar_iris_hip_descriptor.hpp:
// searchIntraLoopClosureIDs, searchInterLoopClosureIDs) on an object a std::unique_ptr<scan_descriptor> owns, the way
// distributedMapping.h holds scanDescriptor, and compares every list with the C calls (scl_iris_search_intra,
// scl_iris_search_inter) on the engine of a twin object fed the same scans.  Prints one `ok iris:` line; exit code 0 = all good
// (tests/test_gpu_iris_search_adapter.py runs it).
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
typedef std::vector<std::vector<lidar_iris_hip_descriptor::LoopCandidate>> Lists;

static const int kRows = 16, kCols = 72;

// place `place` seen under heading `yaw` (tests/cpp/iris_batch_check.cpp)
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

static lidar_iris_hip_descriptor *make()
{
    // rows, cols, nscan, distThres, numExcludeRecent, matchNum, numCandidates, nscale, minWaveLength, mult, sigmaOnf, robotNum, thisID
    return new lidar_iris_hip_descriptor(kRows, kCols, 64, 0.32, 4, 2, 3, 2, 18, 1.6f, 0.75f, 2, 0);
}

// the adapter's lists against the C call's arrays: n_found entries per query, ids equal, shifts and distances by their bits
static int compare(const char *what, int k, const Lists &got, const std::vector<int> &ids, const std::vector<float> &biases, const std::vector<float> &dists,
                   const std::vector<int> &found)
{
    int fails = 0;
    if (got.size() != found.size()) { std::printf("FAIL %s k=%d: %zu lists for %zu queries\n", what, k, got.size(), found.size()); return 1; }
    for (size_t i = 0; i < got.size(); ++i) {
        if ((int)got[i].size() != found[i]) { std::printf("FAIL %s k=%d query %zu: %zu entries, n_found %d\n", what, k, i, got[i].size(), found[i]); ++fails; continue; }
        for (int j = 0; j < found[i]; ++j) {
            const lidar_iris_hip_descriptor::LoopCandidate &c = got[i][(size_t)j];
            if (c.id != ids[i * k + j] || std::memcmp(&c.bias, &biases[i * k + j], sizeof(float)) != 0 || std::memcmp(&c.dist, &dists[i * k + j], sizeof(float)) != 0) {
                std::printf("FAIL %s k=%d query %zu entry %d\n", what, k, i, j);
                ++fails;
            }
        }
    }
    return fails;
}

int main(int argc, char **argv)
{
    const int n = argc > 1 ? std::atoi(argv[1]) : 44;
    if (n < 20) { std::printf("FAIL at least 20 keyframes\n"); return 1; }
    lidar_iris_hip_descriptor *impl = make(), *twin_impl = make();
    std::unique_ptr<scan_descriptor> scanDescriptor(impl), twin(twin_impl);
    if (!impl->engine() || !twin_impl->engine()) { std::printf("FAIL create\n"); return 1; }
    int fails = 0, mine = 0, listed = 0;
    for (int kf = 0; kf < n; ++kf) {                                   // every fourth keyframe is robot 1's
        const Cloud cloud = make_cloud(kf % 15, kf < 15 ? 0.0f : 0.35f * (float)(kf / 15) + 0.01f * (float)(kf % 15), 3000 + 37 * (kf % 11));
        const int8_t robot = kf % 4 == 3 ? 1 : 0;
        scanDescriptor->makeAndSaveDescriptorAndKey(cloud, robot, kf);
        twin->makeAndSaveDescriptorAndKey(cloud, robot, kf);
        mine += robot == 0;
    }
    std::vector<int> locals, keys;
    for (int cur = mine - 1; cur >= 0; --cur) locals.push_back(cur);
    for (int key = 0; key < n; ++key) keys.push_back(key);
    const int ks[3] = {1, 5, SCL_IRIS_SEARCH_MAX};
    for (int t = 0; t < 3; ++t) {
        const int k = ks[t];
        {
            const Lists got = impl->searchIntraLoopClosureIDs(locals, k);
            std::vector<int> ids(locals.size() * k, -7), found(locals.size(), -7);
            std::vector<float> biases(ids.size(), -7.0f), dists(ids.size(), -7.0f);
            if (scl_iris_search_intra(twin_impl->engine(), locals.data(), (int)locals.size(), k, ids.data(), biases.data(), dists.data(), found.data()) != SCL_OK) { std::printf("FAIL C intra\n"); return 1; }
            fails += compare("intra", k, got, ids, biases, dists, found);
            for (size_t i = 0; i < got.size(); ++i) listed += (int)got[i].size();
        }
        {
            const Lists got = impl->searchInterLoopClosureIDs(keys, k);
            std::vector<int> ids(keys.size() * k, -7), found(keys.size(), -7);
            std::vector<float> biases(ids.size(), -7.0f), dists(ids.size(), -7.0f);
            if (scl_iris_search_inter(twin_impl->engine(), keys.data(), (int)keys.size(), k, ids.data(), biases.data(), dists.data(), found.data()) != SCL_OK) { std::printf("FAIL C inter\n"); return 1; }
            fails += compare("inter", k, got, ids, biases, dists, found);
            for (size_t i = 0; i < got.size(); ++i) listed += (int)got[i].size();
        }
    }
    // afterwards the two objects are in one state: a further single call on each
    const std::pair<int, float> a = scanDescriptor->detectInterLoopClosureID(n - 1), b = twin->detectInterLoopClosureID(n - 1);
    if (a.first != b.first || std::memcmp(&a.second, &b.second, sizeof(float)) != 0) { std::printf("FAIL state\n"); ++fails; }
    // a k outside [1, SCL_IRIS_SEARCH_MAX] or an out-of-range entry: one empty list per query
    std::vector<int> bad = {0, 1, n, 2};
    const Lists none[3] = {impl->searchInterLoopClosureIDs(keys, 0), impl->searchIntraLoopClosureIDs(locals, SCL_IRIS_SEARCH_MAX + 1),
                           impl->searchInterLoopClosureIDs(bad, 5)};
    const size_t sizes[3] = {keys.size(), locals.size(), bad.size()};
    for (int t = 0; t < 3; ++t) {
        if (none[t].size() != sizes[t]) { std::printf("FAIL error answer size\n"); ++fails; }
        for (size_t i = 0; i < none[t].size(); ++i)
            if (!none[t][i].empty()) { std::printf("FAIL error answer\n"); ++fails; }
    }
    if (!listed) { std::printf("FAIL nothing listed\n"); ++fails; }
    impl->close(); twin_impl->close();
    if (!fails)
        std::printf("ok iris: the ranked lists of %zu intra and %zu inter queries at k = 1, 5 and %d (%d entries) equal the C calls\n", locals.size(), keys.size(),
                    SCL_IRIS_SEARCH_MAX, listed);
    std::printf(fails ? "FAILED %d\n" : "ALL OK\n", fails);
    return fails ? 1 : 0;
}
