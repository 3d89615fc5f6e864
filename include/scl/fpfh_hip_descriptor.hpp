// fpfh_hip_descriptor.hpp -- header-only adapter that plugs the MI355X FPFH engine (scl_fpfh.h) into the reference's descriptor
// plugin interface, beside scan_context_hip_descriptor.hpp, lidar_iris_hip_descriptor.hpp and m2dp_hip_descriptor.hpp.
//
// Include it AFTER the reference's descriptor.h (it needs `class scan_descriptor`, descriptor.h:21-36, and
// pcl::PointCloud<pcl::PointXYZI>).  The DescriptorType switch changes by one line:
//
//   distributedMapping.h:420   scanDescriptor = std::unique_ptr<scan_descriptor>(new fpfh_descriptor());
//   becomes                    scanDescriptor = std::unique_ptr<scan_descriptor>(new fpfh_hip_descriptor(numberOfRobots, id));
//
// What differs from the reference's class, on purpose (scl_fpfh.h has the details):
//   * normals come from an fp64 covariance and a Jacobi eigensolver (PCL: float covariance, eigen33), so they agree with PCL's to
//     about 1e-6, not bit for bit; the 10 neighbours are exact, ties to the lower index;
//   * detectIntraLoopClosureID works (empty in the reference, descriptor.h:376-379): this robot's keyframes [0, cur - 30);
//   * the inter detection is the reference's by default (all robots, a snapshot rebuilt every 10th call, the distance over the first
//     21 floats, loop below 100); the 1-NN is exact with ties to the lowest key.
// Errors are written to stderr and mapped to "no loop" / empty results, as the reference only logs.
// Lifetime: as for scan_context_hip_descriptor -- scan_descriptor has no virtual destructor, call close() before
// dropping the object if the host re-creates descriptors.
#pragma once

#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "scl_fpfh.h"

class fpfh_hip_descriptor : public scan_descriptor
{
public:
    fpfh_hip_descriptor(int robotNum = 1, int thisID = 0, int device = 0)
    {
        scl_fpfh_config cfg;
        scl_fpfh_default_config(&cfg);
        cfg.robot_num = robotNum; cfg.this_id = thisID; cfg.device = device;
        init(cfg);
    }

    // every field of scl_fpfh_config (dist_thres, num_exclude_recent, tree_making_period, report_dims, inter_mode, ...)
    explicit fpfh_hip_descriptor(const scl_fpfh_config &cfg) { init(cfg); }

    void init(const scl_fpfh_config &cfg)
    {
        const int rc = scl_fpfh_create(&cfg, &fpfh_);
        if (rc != SCL_OK) {
            std::fprintf(stderr, "[fpfh_hip_descriptor] engine creation failed: %s\n", scl_status_string(rc));
            fpfh_ = nullptr;
        }
    }

    ~fpfh_hip_descriptor() { close(); }
    void close()
    {
        if (fpfh_) scl_fpfh_destroy(fpfh_);
        fpfh_ = nullptr;
    }
    fpfh_hip_descriptor(const fpfh_hip_descriptor &) = delete;
    fpfh_hip_descriptor &operator=(const fpfh_hip_descriptor &) = delete;

    // descriptor.h:25 / 308-365: the 33 floats [hist_f1, hist_f2, hist_f3]
    std::vector<float> makeAndSaveDescriptorAndKey(const pcl::PointCloud<pcl::PointXYZI> &scan,
                                                   const int8_t robot, const int index) override
    {
        std::vector<float> v(SCL_FPFH_DIM, 0.0f);
        report(scl_fpfh_make_and_save(fpfh_, scan.points.data(), static_cast<int>(scan.points.size()),
                                      static_cast<int>(sizeof(pcl::PointXYZI)), robot, index, v.data()),
               "makeAndSaveDescriptorAndKey");
        return v;
    }

    // the batch form: scans[i] appended as (robots[i], indexs[i]); returns scans.size() * 33 floats
    std::vector<float> makeAndSaveDescriptorsAndKeys(const std::vector<const pcl::PointCloud<pcl::PointXYZI> *> &scans,
                                                     const std::vector<int8_t> &robots, const std::vector<int> &indexs)
    {
        std::vector<float> v(scans.size() * SCL_FPFH_DIM, 0.0f);
        if (robots.size() != scans.size() || indexs.size() != scans.size()) {
            std::fprintf(stderr, "[fpfh_hip_descriptor] makeAndSaveDescriptorsAndKeys: %zu scans, %zu robots, %zu indexs\n",
                         scans.size(), robots.size(), indexs.size());
            return v;
        }
        std::vector<const void *> ptrs(scans.size());
        std::vector<int> counts(scans.size());
        for (size_t i = 0; i < scans.size(); ++i) { ptrs[i] = scans[i]->points.data(); counts[i] = static_cast<int>(scans[i]->points.size()); }
        report(scl_fpfh_make_and_save_many(fpfh_, ptrs.data(), counts.data(), static_cast<int>(sizeof(pcl::PointXYZI)), robots.data(),
                                           indexs.data(), static_cast<int>(scans.size()), v.data()),
               "makeAndSaveDescriptorsAndKeys");
        return v;
    }

    // the batch forms (scl_fpfh.h "THE BATCH FORMS"): what the single calls in the same order return, one device wait per call.
    // {local index of the loop keyframe or -1, distance} per entry of curPtrs; on an error every entry is {-1, 0}
    std::vector<std::pair<int, float>> detectIntraLoopClosureIDs(const std::vector<int> &curPtrs)
    {
        std::vector<int> loops(curPtrs.size(), -1);
        std::vector<float> dists(curPtrs.size(), 0.0f);
        const bool ok = report(scl_fpfh_detect_intra_many(fpfh_, curPtrs.data(), static_cast<int>(curPtrs.size()), loops.data(), dists.data()),
                               "detectIntraLoopClosureIDs");
        return pairs(loops, dists, ok);
    }

    // {global key of the loop keyframe or -1, distance} per entry of curPtrs
    std::vector<std::pair<int, float>> detectInterLoopClosureIDs(const std::vector<int> &curPtrs)
    {
        std::vector<int> loops(curPtrs.size(), -1);
        std::vector<float> dists(curPtrs.size(), 0.0f);
        const bool ok = report(scl_fpfh_detect_inter_many(fpfh_, curPtrs.data(), static_cast<int>(curPtrs.size()), loops.data(), dists.data()),
                               "detectInterLoopClosureIDs");
        return pairs(loops, dists, ok);
    }

    // the candidate lists (scl_plugin_batch.h "THE CANDIDATE LISTS"): per entry of curPtrs the up to k nearest of the set the
    // detection searches, nearest first, as {local index, distance}, without the threshold -- for a verifier (ICP, RANSAC) to judge.  For FPFH the ranking is over
    // all 33 floats and the distance over report_dims of them: it need not rise with the rank
    // The inner vectors hold n_found pairs (fewer than k when the set is smaller); on an error every one is empty
    std::vector<std::vector<std::pair<int, float>>> detectIntraLoopCandidates(const std::vector<int> &curPtrs, int k)
    {
        return candidates(curPtrs, k, scl_fpfh_detect_intra_topk, "detectIntraLoopCandidates");
    }

    // the same for the inter detection: {global key, distance}
    std::vector<std::vector<std::pair<int, float>>> detectInterLoopCandidates(const std::vector<int> &curPtrs, int k)
    {
        return candidates(curPtrs, k, scl_fpfh_detect_inter_topk, "detectInterLoopCandidates");
    }

    // scans[i] appended as (robots[i], indexs[i]), then the intra detection of every new keyframe of this robot in the same call:
    // {local index of the loop keyframe or -1, distance} per scan ({-1, +inf} for another robot's); descriptors: lastDescriptors()
    std::vector<std::pair<int, float>> makeSaveAndDetect(const std::vector<const pcl::PointCloud<pcl::PointXYZI> *> &scans,
                                                         const std::vector<int8_t> &robots, const std::vector<int> &indexs)
    {
        std::vector<int> loops(scans.size(), -1);
        std::vector<float> dists(scans.size(), 0.0f);
        last_.assign(scans.size() * SCL_FPFH_DIM, 0.0f);
        if (robots.size() != scans.size() || indexs.size() != scans.size()) {
            std::fprintf(stderr, "[fpfh_hip_descriptor] makeSaveAndDetect: %zu scans, %zu robots, %zu indexs\n", scans.size(), robots.size(),
                         indexs.size());
            return pairs(loops, dists, false);
        }
        std::vector<const void *> ptrs(scans.size());
        std::vector<int> counts(scans.size());
        for (size_t i = 0; i < scans.size(); ++i) { ptrs[i] = scans[i]->points.data(); counts[i] = static_cast<int>(scans[i]->points.size()); }
        const bool ok = report(scl_fpfh_make_save_and_detect(fpfh_, ptrs.data(), counts.data(), static_cast<int>(sizeof(pcl::PointXYZI)),
                                                          robots.data(), indexs.data(), static_cast<int>(scans.size()), loops.data(),
                                                          dists.data(), last_.data()),
                               "makeSaveAndDetect");
        return pairs(loops, dists, ok);
    }

    // the descriptors of the last makeSaveAndDetect: scans.size() * 33 floats
    const std::vector<float> &lastDescriptors() const { return last_; }

    // descriptor.h:27 / 367-374, all 33 floats
    void saveDescriptorAndKey(const float *fpfhVec, const int8_t robot, const int index) override
    {
        report(scl_fpfh_save_from_wire(fpfh_, fpfhVec, robot, index), "saveDescriptorAndKey");
    }

    // descriptor.h:29 / 376-379 (empty there): {local index of the loop keyframe or -1, distance}
    std::pair<int, float> detectIntraLoopClosureID(const int curPtr) override
    {
        int loop_id = -1; float dist = 0.0f;
        if (!report(scl_fpfh_detect_intra(fpfh_, curPtr, &loop_id, &dist), "detectIntraLoopClosureID"))
            return std::pair<int, float>(-1, 0.0f);
        return std::pair<int, float>(loop_id, dist);
    }

    // descriptor.h:31 / 381-428: {global key of the loop keyframe or -1, distance}
    std::pair<int, float> detectInterLoopClosureID(const int curPtr) override
    {
        int loop_id = -1; float dist = 0.0f;
        if (!report(scl_fpfh_detect_inter(fpfh_, curPtr, &loop_id, &dist), "detectInterLoopClosureID"))
            return std::pair<int, float>(-1, 0.0f);
        return std::pair<int, float>(loop_id, dist);
    }

    // descriptor.h:33 / 430-433
    std::pair<int8_t, int> getIndex(const int key) override
    {
        int8_t robot = 0; int index = -1;
        report(scl_fpfh_get_index(fpfh_, key, &robot, &index), "getIndex");
        return std::pair<int8_t, int>(robot, index);
    }

    // descriptor.h:35 / 435-438
    int getSize(const int idIn = -1) override
    {
        if (!fpfh_) return 0;
        const int n = scl_fpfh_get_size_of(fpfh_, idIn);
        return n < 0 ? 0 : n;
    }

    scl_fpfh *engine() { return fpfh_; }

private:
    bool report(int rc, const char *where) const
    {
        if (!fpfh_) {
            std::fprintf(stderr, "[fpfh_hip_descriptor] %s: no engine (creation failed or close() was called)\n", where);
            return false;
        }
        if (rc == SCL_OK) return true;
        std::fprintf(stderr, "[fpfh_hip_descriptor] %s: %s (%s)\n", where, scl_status_string(rc), scl_fpfh_last_error(fpfh_));
        return false;
    }

    scl_fpfh *fpfh_ = nullptr;

    std::vector<std::vector<std::pair<int, float>>> candidates(const std::vector<int> &curPtrs, int k,
                                                               int (*call)(scl_fpfh *, const int *, int, int, int *, float *, int *),
                                                               const char *where)
    {
        std::vector<std::vector<std::pair<int, float>>> out(curPtrs.size());
        if (k < 1 || k > SCL_PLUGIN_TOPK_MAX) {
            std::fprintf(stderr, "[fpfh_hip_descriptor] %s: k = %d outside [1, %d]\n", where, k, SCL_PLUGIN_TOPK_MAX);
            return out;
        }
        std::vector<int> ids(curPtrs.size() * static_cast<size_t>(k), -1), found(curPtrs.size(), 0);
        std::vector<float> dists(ids.size(), 0.0f);
        if (!report(call(fpfh_, curPtrs.data(), static_cast<int>(curPtrs.size()), k, ids.data(), dists.data(), found.data()), where)) return out;
        for (size_t i = 0; i < curPtrs.size(); ++i)
            for (int j = 0; j < found[i]; ++j) out[i].push_back(std::pair<int, float>(ids[i * k + j], dists[i * k + j]));
        return out;
    }

    static std::vector<std::pair<int, float>> pairs(const std::vector<int> &loops, const std::vector<float> &dists, bool ok)
    {
        std::vector<std::pair<int, float>> out(loops.size(), std::pair<int, float>(-1, 0.0f));
        for (size_t i = 0; ok && i < loops.size(); ++i) out[i] = std::pair<int, float>(loops[i], dists[i]);
        return out;
    }

    std::vector<float> last_;
};
