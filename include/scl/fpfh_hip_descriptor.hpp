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
//   * detectIntraLoopCandidates / detectInterLoopCandidates rank over all 33 floats and report the distance over report_dims of
//     them: it need not rise with the rank.
// The class itself, member by member: vector_plugin_hip_descriptor.hpp.  The descriptor is the 33 floats [hist_f1, hist_f2, hist_f3]
// (descriptor.h:308-365; saveDescriptorAndKey 367-374 reads all 33; the detections 376-379 and 381-428; getIndex 430-433; getSize
// 435-438).
// Errors are written to stderr and mapped to "no loop" / empty results, as the reference only logs.
// Lifetime: as for scan_context_hip_descriptor -- scan_descriptor has no virtual destructor, call close() before
// dropping the object if the host re-creates descriptors.
#pragma once

#include "scl_fpfh.h"
#include "vector_plugin_hip_descriptor.hpp"

struct fpfh_hip_plugin {
    typedef scl_fpfh handle;
    typedef scl_fpfh_config config;
    enum { DIM = SCL_FPFH_DIM };
    static const char *name() { return "fpfh_hip_descriptor"; }
    static const scl_vector_plugin_api<scl_fpfh, scl_fpfh_config> &api()
    {
        static const scl_vector_plugin_api<scl_fpfh, scl_fpfh_config> a = SCL_VECTOR_PLUGIN_API(scl_fpfh);
        return a;
    }
};

class fpfh_hip_descriptor : public vector_plugin_hip_descriptor<fpfh_hip_plugin>
{
public:
    fpfh_hip_descriptor(int robotNum = 1, int thisID = 0, int device = 0) { init(defaults(robotNum, thisID, device)); }

    // every field of scl_fpfh_config (dist_thres, num_exclude_recent, tree_making_period, report_dims, inter_mode, ...)
    explicit fpfh_hip_descriptor(const scl_fpfh_config &cfg) { init(cfg); }
};
