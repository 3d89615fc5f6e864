// vector_plugin_hip_descriptor.hpp -- the adapter of the float-row descriptor plugins (scl_m2dp.h, scl_fpfh.h, scl_grsd.h) to the
// reference's descriptor plugin interface, written once: m2dp_hip_descriptor.hpp, fpfh_hip_descriptor.hpp and
// grsd_hip_descriptor.hpp each describe their plugin and derive their class from the template below.  Include those, not this.
//
// Needs `class scan_descriptor` (descriptor.h:21-36) and pcl::PointCloud<pcl::PointXYZI> declared before it.
// A plugin description P gives:
//   typedef ... handle, config;      the C handle and config types (scl_X, scl_X_config)
//   enum { DIM = ... };              floats per descriptor
//   static const char *name();       the class name, bracketed in front of every stderr message
//   static const scl_vector_plugin_api<handle, config> &api();     the plugin's C functions: SCL_VECTOR_PLUGIN_API(scl_X)
// Errors are written to stderr and mapped to "no loop" / empty results, as the reference only logs.
#pragma once

#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "scl_engine.h"
#include "scl_plugin_batch.h"

// the C functions of one plugin the adapter calls, in the order SCL_VECTOR_PLUGIN_API lists them
template <class H, class C> struct scl_vector_plugin_api {
    int (*default_config)(C *);
    int (*create)(const C *, H **);
    int (*destroy)(H *);
    const char *(*last_error)(const H *);
    int (*make_and_save)(H *, const void *, int, int, int8_t, int, float *);
    int (*make_and_save_many)(H *, const void *const *, const int *, int, const int8_t *, const int *, int, float *);
    int (*save_from_wire)(H *, const float *, int8_t, int);
    int (*detect_intra)(H *, int, int *, float *);
    int (*detect_inter)(H *, int, int *, float *);
    int (*detect_intra_many)(H *, const int *, int, int *, float *);
    int (*detect_inter_many)(H *, const int *, int, int *, float *);
    int (*detect_intra_topk)(H *, const int *, int, int, int *, float *, int *);
    int (*detect_inter_topk)(H *, const int *, int, int, int *, float *, int *);
    int (*make_save_and_detect)(H *, const void *const *, const int *, int, const int8_t *, const int *, int, int *, float *, float *);
    int (*get_index)(const H *, int, int8_t *, int *);
    int (*get_size_of)(const H *, int);
};

#define SCL_VECTOR_PLUGIN_API(X)                                                                                                   \
    {                                                                                                                              \
        X##_default_config, X##_create, X##_destroy, X##_last_error, X##_make_and_save, X##_make_and_save_many, X##_save_from_wire, \
            X##_detect_intra, X##_detect_inter, X##_detect_intra_many, X##_detect_inter_many, X##_detect_intra_topk,               \
            X##_detect_inter_topk, X##_make_save_and_detect, X##_get_index, X##_get_size_of                                        \
    }

template <class P> class vector_plugin_hip_descriptor : public scan_descriptor
{
public:
    typedef typename P::handle handle;
    typedef typename P::config config;

    vector_plugin_hip_descriptor() {}
    explicit vector_plugin_hip_descriptor(const config &cfg) { init(cfg); }

    // the plugin's default config for this robot
    static config defaults(int robotNum, int thisID, int device)
    {
        config cfg;
        P::api().default_config(&cfg);
        cfg.robot_num = robotNum; cfg.this_id = thisID; cfg.device = device;
        return cfg;
    }

    void init(const config &cfg)
    {
        const int rc = P::api().create(&cfg, &engine_);
        if (rc != SCL_OK) {
            std::fprintf(stderr, "[%s] engine creation failed: %s\n", P::name(), scl_status_string(rc));
            engine_ = nullptr;
        }
    }

    // Lifetime: scan_descriptor has no virtual destructor, call close() before dropping the object if the host re-creates descriptors
    ~vector_plugin_hip_descriptor() { close(); }
    void close()
    {
        if (engine_) P::api().destroy(engine_);
        engine_ = nullptr;
    }
    vector_plugin_hip_descriptor(const vector_plugin_hip_descriptor &) = delete;
    vector_plugin_hip_descriptor &operator=(const vector_plugin_hip_descriptor &) = delete;

    // descriptor.h:25: the DIM floats of the scan's descriptor, stored as (robot, index)
    std::vector<float> makeAndSaveDescriptorAndKey(const pcl::PointCloud<pcl::PointXYZI> &scan,
                                                   const int8_t robot, const int index) override
    {
        std::vector<float> v(P::DIM, 0.0f);
        report(P::api().make_and_save(engine_, scan.points.data(), static_cast<int>(scan.points.size()),
                                      static_cast<int>(sizeof(pcl::PointXYZI)), robot, index, v.data()),
               "makeAndSaveDescriptorAndKey");
        return v;
    }

    // the batch form: scans[i] appended as (robots[i], indexs[i]); returns scans.size() * DIM floats
    std::vector<float> makeAndSaveDescriptorsAndKeys(const std::vector<const pcl::PointCloud<pcl::PointXYZI> *> &scans,
                                                     const std::vector<int8_t> &robots, const std::vector<int> &indexs)
    {
        std::vector<float> v(scans.size() * P::DIM, 0.0f);
        if (robots.size() != scans.size() || indexs.size() != scans.size()) {
            std::fprintf(stderr, "[%s] makeAndSaveDescriptorsAndKeys: %zu scans, %zu robots, %zu indexs\n", P::name(),
                         scans.size(), robots.size(), indexs.size());
            return v;
        }
        std::vector<const void *> ptrs(scans.size());
        std::vector<int> counts(scans.size());
        for (size_t i = 0; i < scans.size(); ++i) { ptrs[i] = scans[i]->points.data(); counts[i] = static_cast<int>(scans[i]->points.size()); }
        report(P::api().make_and_save_many(engine_, ptrs.data(), counts.data(), static_cast<int>(sizeof(pcl::PointXYZI)), robots.data(),
                                           indexs.data(), static_cast<int>(scans.size()), v.data()),
               "makeAndSaveDescriptorsAndKeys");
        return v;
    }

    // the batch forms (scl_plugin_batch.h): what the single calls in the same order return, one device wait per call.
    // {local index of the loop keyframe or -1, distance} per entry of curPtrs; on an error every entry is {-1, 0}
    std::vector<std::pair<int, float>> detectIntraLoopClosureIDs(const std::vector<int> &curPtrs)
    {
        std::vector<int> loops(curPtrs.size(), -1);
        std::vector<float> dists(curPtrs.size(), 0.0f);
        const bool ok = report(P::api().detect_intra_many(engine_, curPtrs.data(), static_cast<int>(curPtrs.size()), loops.data(), dists.data()),
                               "detectIntraLoopClosureIDs");
        return pairs(loops, dists, ok);
    }

    // {global key of the loop keyframe or -1, distance} per entry of curPtrs
    std::vector<std::pair<int, float>> detectInterLoopClosureIDs(const std::vector<int> &curPtrs)
    {
        std::vector<int> loops(curPtrs.size(), -1);
        std::vector<float> dists(curPtrs.size(), 0.0f);
        const bool ok = report(P::api().detect_inter_many(engine_, curPtrs.data(), static_cast<int>(curPtrs.size()), loops.data(), dists.data()),
                               "detectInterLoopClosureIDs");
        return pairs(loops, dists, ok);
    }

    // the candidate lists (scl_plugin_batch.h "THE CANDIDATE LISTS"): per entry of curPtrs the up to k nearest of the set the
    // detection searches, nearest first, as {local index, distance}, without the threshold -- for a verifier (ICP, RANSAC) to judge.
    // The inner vectors hold n_found pairs (fewer than k when the set is smaller); on an error every one is empty
    std::vector<std::vector<std::pair<int, float>>> detectIntraLoopCandidates(const std::vector<int> &curPtrs, int k)
    {
        return candidates(curPtrs, k, P::api().detect_intra_topk, "detectIntraLoopCandidates");
    }

    // the same for the inter detection: {global key, distance}
    std::vector<std::vector<std::pair<int, float>>> detectInterLoopCandidates(const std::vector<int> &curPtrs, int k)
    {
        return candidates(curPtrs, k, P::api().detect_inter_topk, "detectInterLoopCandidates");
    }

    // scans[i] appended as (robots[i], indexs[i]), then the intra detection of every new keyframe of this robot in the same call:
    // {local index of the loop keyframe or -1, distance} per scan ({-1, +inf} for another robot's); descriptors: lastDescriptors()
    std::vector<std::pair<int, float>> makeSaveAndDetect(const std::vector<const pcl::PointCloud<pcl::PointXYZI> *> &scans,
                                                         const std::vector<int8_t> &robots, const std::vector<int> &indexs)
    {
        std::vector<int> loops(scans.size(), -1);
        std::vector<float> dists(scans.size(), 0.0f);
        last_.assign(scans.size() * P::DIM, 0.0f);
        if (robots.size() != scans.size() || indexs.size() != scans.size()) {
            std::fprintf(stderr, "[%s] makeSaveAndDetect: %zu scans, %zu robots, %zu indexs\n", P::name(), scans.size(), robots.size(),
                         indexs.size());
            return pairs(loops, dists, false);
        }
        std::vector<const void *> ptrs(scans.size());
        std::vector<int> counts(scans.size());
        for (size_t i = 0; i < scans.size(); ++i) { ptrs[i] = scans[i]->points.data(); counts[i] = static_cast<int>(scans[i]->points.size()); }
        const bool ok = report(P::api().make_save_and_detect(engine_, ptrs.data(), counts.data(), static_cast<int>(sizeof(pcl::PointXYZI)),
                                                             robots.data(), indexs.data(), static_cast<int>(scans.size()), loops.data(),
                                                             dists.data(), last_.data()),
                               "makeSaveAndDetect");
        return pairs(loops, dists, ok);
    }

    // the descriptors of the last makeSaveAndDetect: scans.size() * DIM floats
    const std::vector<float> &lastDescriptors() const { return last_; }

    // descriptor.h:27: DIM floats from the wire, stored as (robot, index)
    void saveDescriptorAndKey(const float *values, const int8_t robot, const int index) override
    {
        report(P::api().save_from_wire(engine_, values, robot, index), "saveDescriptorAndKey");
    }

    // descriptor.h:29: {local index of the loop keyframe or -1, distance}
    std::pair<int, float> detectIntraLoopClosureID(const int curPtr) override
    {
        int loop_id = -1; float dist = 0.0f;
        if (!report(P::api().detect_intra(engine_, curPtr, &loop_id, &dist), "detectIntraLoopClosureID"))
            return std::pair<int, float>(-1, 0.0f);
        return std::pair<int, float>(loop_id, dist);
    }

    // descriptor.h:31: {global key of the loop keyframe or -1, distance}
    std::pair<int, float> detectInterLoopClosureID(const int curPtr) override
    {
        int loop_id = -1; float dist = 0.0f;
        if (!report(P::api().detect_inter(engine_, curPtr, &loop_id, &dist), "detectInterLoopClosureID"))
            return std::pair<int, float>(-1, 0.0f);
        return std::pair<int, float>(loop_id, dist);
    }

    // descriptor.h:33
    std::pair<int8_t, int> getIndex(const int key) override
    {
        int8_t robot = 0; int index = -1;
        report(P::api().get_index(engine_, key, &robot, &index), "getIndex");
        return std::pair<int8_t, int>(robot, index);
    }

    // descriptor.h:35
    int getSize(const int idIn = -1) override
    {
        if (!engine_) return 0;
        const int n = P::api().get_size_of(engine_, idIn);
        return n < 0 ? 0 : n;
    }

    handle *engine() { return engine_; }

private:
    bool report(int rc, const char *where) const
    {
        if (!engine_) {
            std::fprintf(stderr, "[%s] %s: no engine (creation failed or close() was called)\n", P::name(), where);
            return false;
        }
        if (rc == SCL_OK) return true;
        std::fprintf(stderr, "[%s] %s: %s (%s)\n", P::name(), where, scl_status_string(rc), P::api().last_error(engine_));
        return false;
    }

    std::vector<std::vector<std::pair<int, float>>> candidates(const std::vector<int> &curPtrs, int k,
                                                               int (*call)(handle *, const int *, int, int, int *, float *, int *),
                                                               const char *where)
    {
        std::vector<std::vector<std::pair<int, float>>> out(curPtrs.size());
        if (k < 1 || k > SCL_PLUGIN_TOPK_MAX) {
            std::fprintf(stderr, "[%s] %s: k = %d outside [1, %d]\n", P::name(), where, k, SCL_PLUGIN_TOPK_MAX);
            return out;
        }
        std::vector<int> ids(curPtrs.size() * static_cast<size_t>(k), -1), found(curPtrs.size(), 0);
        std::vector<float> dists(ids.size(), 0.0f);
        if (!report(call(engine_, curPtrs.data(), static_cast<int>(curPtrs.size()), k, ids.data(), dists.data(), found.data()), where)) return out;
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

    handle *engine_ = nullptr;
    std::vector<float> last_;
};
