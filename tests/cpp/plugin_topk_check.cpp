// Drives the candidate lists of the M2DP, FPFH and GRSD adapters (include/scl/{m2dp,fpfh,grsd}_hip_descriptor.hpp:
// detectIntraLoopCandidates, detectInterLoopCandidates) on objects a std::unique_ptr<scan_descriptor> owns, the way
// distributedMapping.h holds scanDescriptor, and compares every list with the C calls (scl_X_detect_intra_topk,
// scl_X_detect_inter_topk) on the engine of a twin object fed the same scans.  Prints one `ok` line per adapter; exit code 0 = all
// good (tests/test_gpu_plugin_topk_adapter.py runs it).
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
typedef std::vector<std::vector<std::pair<int, float>>> Lists;

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

// the adapter's lists against the C call's arrays: n_found pairs per query, ids equal, distances by their bits
static int compare(const char *name, const char *what, int k, const Lists &got, const std::vector<int> &ids, const std::vector<float> &dists,
                   const std::vector<int> &found)
{
    int fails = 0;
    if (got.size() != found.size()) { std::printf("FAIL %s %s k=%d: %zu lists for %zu queries\n", name, what, k, got.size(), found.size()); return 1; }
    for (size_t i = 0; i < got.size(); ++i) {
        if ((int)got[i].size() != found[i]) { std::printf("FAIL %s %s k=%d query %zu: %zu pairs, n_found %d\n", name, what, k, i, got[i].size(), found[i]); ++fails; continue; }
        for (int j = 0; j < found[i]; ++j)
            if (got[i][(size_t)j].first != ids[i * k + j] || std::memcmp(&got[i][(size_t)j].second, &dists[i * k + j], sizeof(float)) != 0) {
                std::printf("FAIL %s %s k=%d query %zu entry %d\n", name, what, k, i, j);
                ++fails;
            }
    }
    return fails;
}

template <class Adapter, class Engine>
static int check(const char *name, Adapter *impl, Adapter *twin_impl, const std::vector<Cloud> &clouds,
                 int (*intra)(Engine *, const int *, int, int, int *, float *, int *), int (*inter)(Engine *, const int *, int, int, int *, float *, int *))
{
    std::unique_ptr<scan_descriptor> scanDescriptor(impl), twin(twin_impl);
    if (!impl->engine() || !twin_impl->engine()) { std::printf("FAIL %s create\n", name); return 1; }
    int fails = 0, mine = 0, listed = 0;
    const int n = (int)clouds.size();
    for (int kf = 0; kf < n; ++kf) {                                   // every fourth keyframe is robot 1's
        const int8_t robot = kf % 4 == 3 ? 1 : 0;
        scanDescriptor->makeAndSaveDescriptorAndKey(clouds[(size_t)kf], robot, kf);
        twin->makeAndSaveDescriptorAndKey(clouds[(size_t)kf], robot, kf);
        mine += robot == 0;
    }
    std::vector<int> locals, keys;
    for (int cur = mine - 1; cur >= 0; --cur) locals.push_back(cur);
    for (int key = 0; key < n; ++key) keys.push_back(key);
    const int ks[3] = {1, 5, SCL_PLUGIN_TOPK_MAX};
    for (int t = 0; t < 3; ++t) {
        const int k = ks[t];
        {
            const Lists got = impl->detectIntraLoopCandidates(locals, k);
            std::vector<int> ids(locals.size() * k, -7), found(locals.size(), -7);
            std::vector<float> dists(ids.size(), -7.0f);
            if (intra(twin_impl->engine(), locals.data(), (int)locals.size(), k, ids.data(), dists.data(), found.data()) != SCL_OK) { std::printf("FAIL %s C intra\n", name); return 1; }
            fails += compare(name, "intra", k, got, ids, dists, found);
            for (size_t i = 0; i < got.size(); ++i) listed += (int)got[i].size();
        }
        {
            const Lists got = impl->detectInterLoopCandidates(keys, k);
            std::vector<int> ids(keys.size() * k, -7), found(keys.size(), -7);
            std::vector<float> dists(ids.size(), -7.0f);
            if (inter(twin_impl->engine(), keys.data(), (int)keys.size(), k, ids.data(), dists.data(), found.data()) != SCL_OK) { std::printf("FAIL %s C inter\n", name); return 1; }
            fails += compare(name, "inter", k, got, ids, dists, found);
            for (size_t i = 0; i < got.size(); ++i) listed += (int)got[i].size();
        }
    }
    // afterwards the two objects are in one state: a further single call on each
    const std::pair<int, float> a = scanDescriptor->detectInterLoopClosureID(n - 1), b = twin->detectInterLoopClosureID(n - 1);
    if (a.first != b.first || std::memcmp(&a.second, &b.second, sizeof(float)) != 0) { std::printf("FAIL %s state\n", name); ++fails; }
    // a k outside [1, SCL_PLUGIN_TOPK_MAX] or an out-of-range entry: one empty list per query
    std::vector<int> bad = {0, 1, n, 2};
    const Lists none[3] = {impl->detectInterLoopCandidates(keys, 0), impl->detectIntraLoopCandidates(locals, SCL_PLUGIN_TOPK_MAX + 1),
                           impl->detectInterLoopCandidates(bad, 5)};
    const size_t sizes[3] = {keys.size(), locals.size(), bad.size()};
    for (int t = 0; t < 3; ++t) {
        if (none[t].size() != sizes[t]) { std::printf("FAIL %s error answer size\n", name); ++fails; }
        for (size_t i = 0; i < none[t].size(); ++i)
            if (!none[t][i].empty()) { std::printf("FAIL %s error answer\n", name); ++fails; }
    }
    if (!listed) { std::printf("FAIL %s nothing listed\n", name); ++fails; }
    impl->close(); twin_impl->close();
    if (!fails)
        std::printf("ok %s: the candidate lists of %zu intra and %zu inter queries at k = 1, 5 and %d (%d entries) equal the C calls\n", name,
                    locals.size(), keys.size(), SCL_PLUGIN_TOPK_MAX, listed);
    return fails;
}

int main(int argc, char **argv)
{
    const int n = argc > 1 ? std::atoi(argv[1]) : 44;
    if (n < 20) { std::printf("FAIL at least 20 keyframes\n"); return 1; }
    std::mt19937_64 rng(29);
    std::vector<Cloud> clouds;
    for (int kf = 0; kf < n; ++kf) clouds.push_back(make_cloud(rng, 3000 + 37 * (kf % 11), 0.1f * (kf % 11), 0.05f * (kf % 11)));
    int fails = 0;
    {
        fails += check("m2dp", new m2dp_hip_descriptor(0.3, 4, 2, 0), new m2dp_hip_descriptor(0.3, 4, 2, 0), clouds, scl_m2dp_detect_intra_topk,
                       scl_m2dp_detect_inter_topk);
    }
    {
        scl_fpfh_config cfg; scl_fpfh_default_config(&cfg);
        cfg.num_exclude_recent = 4; cfg.tree_making_period = 3; cfg.robot_num = 2; cfg.this_id = 0;
        fails += check("fpfh", new fpfh_hip_descriptor(cfg), new fpfh_hip_descriptor(cfg), clouds, scl_fpfh_detect_intra_topk, scl_fpfh_detect_inter_topk);
    }
    {
        scl_grsd_config cfg; scl_grsd_default_config(&cfg);
        cfg.num_exclude_recent = 4; cfg.tree_making_period = 3; cfg.robot_num = 2; cfg.this_id = 0;
        fails += check("grsd", new grsd_hip_descriptor(cfg), new grsd_hip_descriptor(cfg), clouds, scl_grsd_detect_intra_topk, scl_grsd_detect_inter_topk);
    }
    std::printf(fails ? "FAILED %d\n" : "ALL OK\n", fails);
    return fails ? 1 : 0;
}
