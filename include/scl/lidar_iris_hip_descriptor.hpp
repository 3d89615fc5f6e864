// lidar_iris_hip_descriptor.hpp -- header-only adapter that plugs the MI355X LiDAR-Iris engine (scl_iris.h) into the
// reference's descriptor plugin interface, beside scan_context_hip_descriptor.hpp.
//
// Include it AFTER the reference's descriptor.h (it needs `class scan_descriptor`, descriptor.h:21-36, and
// pcl::PointCloud<pcl::PointXYZI>).  Same constructor arguments, defaults and return conventions as
// lidar_iris_descriptor (descriptor.h:462-1302); the DescriptorType switch changes by one line:
//
//   distributedMapping.h:408   scanDescriptor = std::unique_ptr<scan_descriptor>(new lidar_iris_descriptor(80, 360, N_SCAN, 0.4, ...));
//   becomes                    scanDescriptor = std::unique_ptr<scan_descriptor>(new lidar_iris_hip_descriptor(80, 360, N_SCAN, 0.4, ...));
//
// What differs from the reference's class, on purpose (scl_iris.h has the details):
//   * compare() follows the reference (FFT shift estimate, two five-shift Hamming windows, matchNum), but the estimate is OpenCV's
//     algorithms restated, not OpenCV's binaries: an estimate within rounding of a whole column can fall on the other side and move
//     a window by one column (parity unpinned).  shiftSearch = 1 searches every column shift instead -- then the distance is <= the
//     reference's and distThres 0.32 accepts loops the reference would not: an opt-in, re-derive the threshold for it;
//   * saveDescriptorAndKey decodes the wire vector with the reference's own indexing by default (wireDecode = 0,
//     descriptor.h:1035 -- it shears the received image); wireDecode = 1 reads the layout makeAndSave emits.
// Errors are written to stderr and mapped to "no loop" / empty results, as the reference only logs.
// Lifetime: as for scan_context_hip_descriptor -- scan_descriptor has no virtual destructor, call close() before
// dropping the object if the host re-creates descriptors.
#pragma once

#include <cfloat>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "scl_iris.h"

class lidar_iris_hip_descriptor : public scan_descriptor
{
public:
    // parameter list and defaults of lidar_iris_descriptor's ctor, descriptor.h:473-486
    lidar_iris_hip_descriptor(
        int rows               = 80,
        int cols               = 360,
        int nscan              = 64,
        double distThres       = 0.32,
        int numExcludeRecent   = 30,
        int matchNum           = 2,
        int numCandidates      = 10,
        int nscale             = 4,
        int minWaveLength      = 18,
        float mult             = 1.6f,
        float sigmaOnf         = 0.75f,
        int robotNum           = 1,
        int thisID             = 0,
        int device             = 0,
        int wireDecode         = 0,
        float knnExcludeEps    = FLT_EPSILON,
        int shiftSearch        = 0)
    {
        scl_iris_config cfg;
        scl_iris_default_config(&cfg);
        cfg.rows = rows; cfg.cols = cols; cfg.nscan = nscan; cfg.dist_thres = distThres;
        cfg.num_exclude_recent = numExcludeRecent; cfg.match_num = matchNum; cfg.num_candidates = numCandidates;
        cfg.nscale = nscale; cfg.min_wavelength = minWaveLength; cfg.mult = mult; cfg.sigma_onf = sigmaOnf;
        cfg.robot_num = robotNum; cfg.this_id = thisID; cfg.device = device; cfg.wire_decode = wireDecode;
        cfg.knn_exclude_eps = knnExcludeEps; cfg.shift_search = shiftSearch;
        values_ = rows * cols + rows;
        const int rc = scl_iris_create(&cfg, &iris_);
        if (rc != SCL_OK) {
            std::fprintf(stderr, "[lidar_iris_hip_descriptor] engine creation failed: %s\n", scl_status_string(rc));
            iris_ = nullptr;
        }
    }

    ~lidar_iris_hip_descriptor() { close(); }
    void close()
    {
        if (iris_) scl_iris_destroy(iris_);
        iris_ = nullptr;
    }
    lidar_iris_hip_descriptor(const lidar_iris_hip_descriptor &) = delete;
    lidar_iris_hip_descriptor &operator=(const lidar_iris_hip_descriptor &) = delete;

    // descriptor.h:25 / 1062-1083: image values row-major, then the row key
    std::vector<float> makeAndSaveDescriptorAndKey(const pcl::PointCloud<pcl::PointXYZI> &scan,
                                                   const int8_t robot, const int index) override
    {
        std::vector<float> vT(static_cast<size_t>(values_), 0.0f);
        report(scl_iris_make_and_save(iris_, scan.points.data(), static_cast<int>(scan.points.size()),
                                      static_cast<int>(sizeof(pcl::PointXYZI)), robot, index, vT.data()),
               "makeAndSaveDescriptorAndKey");
        return vT;
    }

    // the batch form: scans[i] appended as (robots[i], indexs[i]); returns scans.size() * (rows * cols + rows) floats
    std::vector<float> makeAndSaveDescriptorsAndKeys(const std::vector<const pcl::PointCloud<pcl::PointXYZI> *> &scans,
                                                     const std::vector<int8_t> &robots, const std::vector<int> &indexs)
    {
        std::vector<float> v(scans.size() * static_cast<size_t>(values_), 0.0f);
        if (robots.size() != scans.size() || indexs.size() != scans.size()) {
            std::fprintf(stderr, "[lidar_iris_hip_descriptor] makeAndSaveDescriptorsAndKeys: %zu scans, %zu robots, %zu indexs\n",
                         scans.size(), robots.size(), indexs.size());
            return v;
        }
        std::vector<const void *> ptrs(scans.size());
        std::vector<int> counts(scans.size());
        for (size_t i = 0; i < scans.size(); ++i) { ptrs[i] = scans[i]->points.data(); counts[i] = static_cast<int>(scans[i]->points.size()); }
        report(scl_iris_make_and_save_many(iris_, ptrs.data(), counts.data(), static_cast<int>(sizeof(pcl::PointXYZI)), robots.data(),
                                           indexs.data(), static_cast<int>(scans.size()), v.data()),
               "makeAndSaveDescriptorsAndKeys");
        return v;
    }

    // the batch form of saveDescriptorAndKey: robots.size() vectors of rows * cols + rows floats, one after the other in `iris`
    void saveDescriptorsAndKeys(const float *iris, const std::vector<int8_t> &robots, const std::vector<int> &indexs)
    {
        if (robots.size() != indexs.size()) {
            std::fprintf(stderr, "[lidar_iris_hip_descriptor] saveDescriptorsAndKeys: %zu robots, %zu indexs\n", robots.size(), indexs.size());
            return;
        }
        report(scl_iris_save_from_wire_many(iris_, iris, robots.data(), indexs.data(), static_cast<int>(robots.size())), "saveDescriptorsAndKeys");
    }

    // the batch forms (scl_iris.h "THE BATCH FORMS"): what the single calls in the same order return.
    // {local index of the loop keyframe or -1, column shift} per entry of curPtrs; on an error every entry is {-1, 0}
    std::vector<std::pair<int, float>> detectIntraLoopClosureIDs(const std::vector<int> &curPtrs)
    {
        std::vector<int> loops(curPtrs.size(), -1);
        std::vector<float> biases(curPtrs.size(), 0.0f);
        const bool ok = report(scl_iris_detect_intra_many(iris_, curPtrs.data(), static_cast<int>(curPtrs.size()), loops.data(), biases.data(), nullptr),
                               "detectIntraLoopClosureIDs");
        return pairs(loops, biases, ok);
    }

    // {global key of the loop keyframe or -1, column shift} per entry of curPtrs
    std::vector<std::pair<int, float>> detectInterLoopClosureIDs(const std::vector<int> &curPtrs)
    {
        std::vector<int> loops(curPtrs.size(), -1);
        std::vector<float> biases(curPtrs.size(), 0.0f);
        const bool ok = report(scl_iris_detect_inter_many(iris_, curPtrs.data(), static_cast<int>(curPtrs.size()), loops.data(), biases.data(), nullptr),
                               "detectInterLoopClosureIDs");
        return pairs(loops, biases, ok);
    }

    // scans[i] appended as (robots[i], indexs[i]), then the intra detection of every new keyframe of this robot in the same call:
    // {local index of the loop keyframe or -1, column shift} per scan ({-1, 0} for another robot's); descriptors: lastDescriptors()
    std::vector<std::pair<int, float>> makeSaveAndDetect(const std::vector<const pcl::PointCloud<pcl::PointXYZI> *> &scans,
                                                         const std::vector<int8_t> &robots, const std::vector<int> &indexs)
    {
        std::vector<int> loops(scans.size(), -1);
        std::vector<float> biases(scans.size(), 0.0f);
        last_.assign(scans.size() * static_cast<size_t>(values_), 0.0f);
        if (robots.size() != scans.size() || indexs.size() != scans.size()) {
            std::fprintf(stderr, "[lidar_iris_hip_descriptor] makeSaveAndDetect: %zu scans, %zu robots, %zu indexs\n", scans.size(), robots.size(),
                         indexs.size());
            return pairs(loops, biases, false);
        }
        std::vector<const void *> ptrs(scans.size());
        std::vector<int> counts(scans.size());
        for (size_t i = 0; i < scans.size(); ++i) { ptrs[i] = scans[i]->points.data(); counts[i] = static_cast<int>(scans[i]->points.size()); }
        const bool ok = report(scl_iris_make_save_and_detect(iris_, ptrs.data(), counts.data(), static_cast<int>(sizeof(pcl::PointXYZI)),
                                                          robots.data(), indexs.data(), static_cast<int>(scans.size()), loops.data(),
                                                          biases.data(), nullptr, last_.data()),
                               "makeSaveAndDetect");
        return pairs(loops, biases, ok);
    }

    // one ranked candidate of the exhaustive search: the keyframe, the column shift and the distance over every shift
    struct LoopCandidate { int id; float bias; float dist; };

    // the exhaustive ranked search (scl_iris.h "THE EXHAUSTIVE SEARCH"): per entry of curPtrs the up to k best keyframes of the whole
    // set detectIntraLoopClosureID searches, ascending by distance, distThres not applied -- for a verifier that takes several
    // candidates; ids are local indices.  On an error (k outside [1, SCL_IRIS_SEARCH_MAX], an entry out of range) every list is empty
    std::vector<std::vector<LoopCandidate>> searchIntraLoopClosureIDs(const std::vector<int> &curPtrs, int k)
    {
        return search(curPtrs, k, scl_iris_search_intra, "searchIntraLoopClosureIDs");
    }

    // the same over the set detectInterLoopClosureID searches: ids are global keys
    std::vector<std::vector<LoopCandidate>> searchInterLoopClosureIDs(const std::vector<int> &curPtrs, int k)
    {
        return search(curPtrs, k, scl_iris_search_inter, "searchInterLoopClosureIDs");
    }

    // the descriptors of the last makeSaveAndDetect: scans.size() * (rows * cols + rows) floats
    const std::vector<float> &lastDescriptors() const { return last_; }

    // descriptor.h:27 / 1026-1044 (iris = global_descriptor.values.data(), DM.h:627)
    void saveDescriptorAndKey(const float *iris, const int8_t robot, const int index) override
    {
        report(scl_iris_save_from_wire(iris_, iris, robot, index), "saveDescriptorAndKey");
    }

    // descriptor.h:29 / 1085-1151: {local index of the loop keyframe or -1, column shift}
    std::pair<int, float> detectIntraLoopClosureID(const int curPtr) override
    {
        int loop_id = -1; float bias = 0.0f;
        if (!report(scl_iris_detect_intra(iris_, curPtr, &loop_id, &bias, nullptr), "detectIntraLoopClosureID"))
            return std::pair<int, float>(-1, 0.0f);
        return std::pair<int, float>(loop_id, bias);
    }

    // descriptor.h:31 / 1153-1253: {global key of the loop keyframe or -1, column shift}
    std::pair<int, float> detectInterLoopClosureID(const int curPtr) override
    {
        int loop_id = -1; float bias = 0.0f;
        if (!report(scl_iris_detect_inter(iris_, curPtr, &loop_id, &bias, nullptr), "detectInterLoopClosureID"))
            return std::pair<int, float>(-1, 0.0f);
        return std::pair<int, float>(loop_id, bias);
    }

    // descriptor.h:33 / 1255-1258
    std::pair<int8_t, int> getIndex(const int key) override
    {
        int8_t robot = 0; int index = -1;
        report(scl_iris_get_index(iris_, key, &robot, &index), "getIndex");
        return std::pair<int8_t, int>(robot, index);
    }

    // descriptor.h:35 / 1260-1270
    int getSize(const int idIn = -1) override
    {
        if (!iris_) return 0;
        const int n = scl_iris_get_size_of(iris_, idIn);
        return n < 0 ? 0 : n;
    }

    scl_iris *engine() { return iris_; }

private:
    bool report(int rc, const char *where) const
    {
        if (!iris_) {
            std::fprintf(stderr, "[lidar_iris_hip_descriptor] %s: no engine (creation failed or close() was called)\n", where);
            return false;
        }
        if (rc == SCL_OK) return true;
        std::fprintf(stderr, "[lidar_iris_hip_descriptor] %s: %s (%s)\n", where, scl_status_string(rc), scl_iris_last_error(iris_));
        return false;
    }

    std::vector<std::vector<LoopCandidate>> search(const std::vector<int> &curPtrs, int k,
                                                   int (*call)(scl_iris *, const int *, int, int, int *, float *, float *, int *), const char *where)
    {
        std::vector<std::vector<LoopCandidate>> out(curPtrs.size());
        if (k < 1 || k > SCL_IRIS_SEARCH_MAX) {
            std::fprintf(stderr, "[lidar_iris_hip_descriptor] %s: k = %d outside [1, %d]\n", where, k, SCL_IRIS_SEARCH_MAX);
            return out;
        }
        std::vector<int> ids(curPtrs.size() * static_cast<size_t>(k), -1), found(curPtrs.size(), 0);
        std::vector<float> biases(ids.size(), 0.0f), dists(ids.size(), 0.0f);
        if (!report(call(iris_, curPtrs.data(), static_cast<int>(curPtrs.size()), k, ids.data(), biases.data(), dists.data(), found.data()), where)) return out;
        for (size_t i = 0; i < curPtrs.size(); ++i)
            for (int j = 0; j < found[i]; ++j) out[i].push_back(LoopCandidate{ids[i * k + j], biases[i * k + j], dists[i * k + j]});
        return out;
    }

    static std::vector<std::pair<int, float>> pairs(const std::vector<int> &loops, const std::vector<float> &biases, bool ok)
    {
        std::vector<std::pair<int, float>> out(loops.size(), std::pair<int, float>(-1, 0.0f));
        for (size_t i = 0; ok && i < loops.size(); ++i) out[i] = std::pair<int, float>(loops[i], biases[i]);
        return out;
    }

    scl_iris *iris_ = nullptr;
    int values_ = 0;
    std::vector<float> last_;
};
