// Drives the GRSD engine through include/scl/grsd_hip_descriptor.hpp the way distributedMapping.h drives scanDescriptor
// (makeDescriptors, globalDescriptorHandler, performIntraLoopClosure) and checks every adapter call against the C calls on a
// second engine fed the same data.  Prints one line per check; exit code 0 = all good (tests/test_gpu_grsd.py runs it).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>

#include "pcl_types_for_adapter_check.h"
#include "scl/grsd_hip_descriptor.hpp"

static pcl::PointCloud<pcl::PointXYZI> make_cloud(std::mt19937_64 &rng, int n, float yaw, float dx)
{
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    pcl::PointCloud<pcl::PointXYZI> c;
    const float cs = std::cos(yaw), sn = std::sin(yaw);
    for (int i = 0; i < n; ++i) {
        pcl::PointXYZI p{};
        const float x = 40.0f * u(rng), y = 15.0f * u(rng), z = 3.0f * u(rng) + 0.1f * x;
        p.x = cs * x - sn * y + dx; p.y = sn * x + cs * y; p.z = z; p.intensity = 1.0f;
        c.points.push_back(p);
    }
    return c;
}

int main(int argc, char **argv)
{
    const int n_keyframes = argc > 1 ? std::atoi(argv[1]) : 48;
    scl_grsd_config cfg; scl_grsd_default_config(&cfg);
    cfg.num_exclude_recent = 4; cfg.tree_making_period = 3; cfg.robot_num = 2; cfg.this_id = 0;
    grsd_hip_descriptor *impl = new grsd_hip_descriptor(cfg);
    std::unique_ptr<scan_descriptor> scanDescriptor(impl);          // the DM.h:416 line
    scl_grsd *ref = nullptr;
    if (scl_grsd_create(&cfg, &ref) != SCL_OK || !impl->engine()) { std::printf("FAIL create\n"); return 1; }
    std::mt19937_64 rng(11);
    int fails = 0;
    std::vector<pcl::PointCloud<pcl::PointXYZI>> clouds;
    for (int kf = 0; kf < n_keyframes; ++kf) clouds.push_back(make_cloud(rng, 3000 + 37 * kf, 0.1f * (kf % 12), 0.05f * kf));
    // the first half one by one, the second half through the batch form
    const int half = n_keyframes / 2;
    for (int kf = 0; kf < half; ++kf) {
        std::vector<float> a = scanDescriptor->makeAndSaveDescriptorAndKey(clouds[kf], 0, kf);
        std::vector<float> b(SCL_GRSD_DIM);
        scl_grsd_make_and_save(ref, clouds[kf].points.data(), (int)clouds[kf].points.size(), (int)sizeof(pcl::PointXYZI), 0, kf, b.data());
        if (a.size() != SCL_GRSD_DIM || std::memcmp(a.data(), b.data(), sizeof(float) * SCL_GRSD_DIM) != 0) { std::printf("FAIL make %d\n", kf); ++fails; }
    }
    std::vector<const pcl::PointCloud<pcl::PointXYZI> *> batch; std::vector<int8_t> robots; std::vector<int> indexs;
    for (int kf = half; kf < n_keyframes; ++kf) { batch.push_back(&clouds[kf]); robots.push_back(0); indexs.push_back(kf); }
    std::vector<float> vb = impl->makeAndSaveDescriptorsAndKeys(batch, robots, indexs);
    for (int kf = half; kf < n_keyframes; ++kf) {
        std::vector<float> b(SCL_GRSD_DIM);
        scl_grsd_make_and_save(ref, clouds[kf].points.data(), (int)clouds[kf].points.size(), (int)sizeof(pcl::PointXYZI), 0, kf, b.data());
        if (std::memcmp(vb.data() + (size_t)(kf - half) * SCL_GRSD_DIM, b.data(), sizeof(float) * SCL_GRSD_DIM) != 0) { std::printf("FAIL batch %d\n", kf); ++fails; }
    }
    std::printf("ok makeAndSave: %d keyframes (%d one by one, %d batched) equal the C calls\n", n_keyframes, half, n_keyframes - half);
    // a received keyframe of robot 1 (globalDescriptorHandler, DM.h:625-628)
    std::vector<float> wire(SCL_GRSD_DIM);
    scl_grsd_get_signature(ref, 3, wire.data());
    scanDescriptor->saveDescriptorAndKey(wire.data(), 1, 0);
    scl_grsd_save_from_wire(ref, wire.data(), 1, 0);
    if (scanDescriptor->getSize() != n_keyframes + 1 || scanDescriptor->getSize(1) != 1 || scanDescriptor->getSize(0) != n_keyframes) {
        std::printf("FAIL getSize\n"); ++fails;
    }
    for (int cur = 0; cur < n_keyframes; ++cur) {
        const std::pair<int, float> a = scanDescriptor->detectIntraLoopClosureID(cur);
        int id = -1; float d = 0.0f;
        scl_grsd_detect_intra(ref, cur, &id, &d);
        if (a.first != id || (cur > 4 && std::memcmp(&a.second, &d, sizeof(float)) != 0)) { std::printf("FAIL intra %d: %d %g vs %d %g\n", cur, a.first, a.second, id, d); ++fails; }
    }
    for (int key = 0; key <= n_keyframes; ++key) {
        const std::pair<int, float> a = scanDescriptor->detectInterLoopClosureID(key);
        int id = -1; float d = 0.0f;
        scl_grsd_detect_inter(ref, key, &id, &d);
        if (a.first != id || std::memcmp(&a.second, &d, sizeof(float)) != 0) { std::printf("FAIL inter %d\n", key); ++fails; }
        const std::pair<int8_t, int> gi = scanDescriptor->getIndex(key);
        int8_t r = -1; int ix = -1;
        scl_grsd_get_index(ref, key, &r, &ix);
        if (gi.first != r || gi.second != ix) { std::printf("FAIL getIndex %d\n", key); ++fails; }
    }
    const std::pair<int, float> loop = scanDescriptor->detectInterLoopClosureID(n_keyframes);   // the received copy of keyframe 3
    if (loop.first != 3 || loop.second != 0.0f) { std::printf("FAIL received copy: %d %g\n", loop.first, loop.second); ++fails; }
    std::printf("ok detect: intra %d, inter %d queries equal the C calls; the received copy finds keyframe %d\n", n_keyframes, n_keyframes + 1, loop.first);
    scl_grsd_destroy(ref);
    impl->close();
    std::printf(fails ? "FAILED %d\n" : "ALL OK\n", fails);
    return fails ? 1 : 0;
}
