// grsd_hip_descriptor.hpp -- header-only adapter that plugs the MI355X GRSD engine (scl_grsd.h) into the reference's descriptor
// plugin interface, beside scan_context_hip_descriptor.hpp, lidar_iris_hip_descriptor.hpp, m2dp_hip_descriptor.hpp and
// fpfh_hip_descriptor.hpp.
//
// Include it AFTER the reference's descriptor.h (it needs `class scan_descriptor`, descriptor.h:21-36, and
// pcl::PointCloud<pcl::PointXYZI>).  The DescriptorType switch changes by one line:
//
//   distributedMapping.h:416   scanDescriptor = std::unique_ptr<scan_descriptor>(new grsd_descriptor());
//   becomes                    scanDescriptor = std::unique_ptr<scan_descriptor>(new grsd_hip_descriptor(numberOfRobots, id));
//
// What differs from the reference's class, on purpose (scl_grsd.h has the details):
//   * normals come from an exact integer scatter in fp64 and a Jacobi eigensolver (PCL: float covariance, eigen33), the RSD angles
//     from the float acosf (PCL: double acos): descriptors agree with PCL's up to voxels that sit on a class threshold, not bit for bit;
//   * detectIntraLoopClosureID works (empty in the reference, descriptor.h:111-114): this robot's keyframes [0, cur - 30);
//   * the inter detection is the reference's by default (all robots, a snapshot rebuilt every 10th call, loop below 160); the 1-NN
//     is exact with ties to the lowest key.
// The class itself, member by member: vector_plugin_hip_descriptor.hpp.  The descriptor is the 21 floats of the symmetrised
// class-transition matrix (descriptor.h:57-100; saveDescriptorAndKey 102-109; the detections 111-114 and 116-167; getIndex 169-172;
// getSize 174-177).
// Errors are written to stderr and mapped to "no loop" / empty results, as the reference only logs.
// Lifetime: as for scan_context_hip_descriptor -- scan_descriptor has no virtual destructor, call close() before
// dropping the object if the host re-creates descriptors.
#pragma once

#include "scl_grsd.h"
#include "vector_plugin_hip_descriptor.hpp"

struct grsd_hip_plugin {
    typedef scl_grsd handle;
    typedef scl_grsd_config config;
    enum { DIM = SCL_GRSD_DIM };
    static const char *name() { return "grsd_hip_descriptor"; }
    static const scl_vector_plugin_api<scl_grsd, scl_grsd_config> &api()
    {
        static const scl_vector_plugin_api<scl_grsd, scl_grsd_config> a = SCL_VECTOR_PLUGIN_API(scl_grsd);
        return a;
    }
};

class grsd_hip_descriptor : public vector_plugin_hip_descriptor<grsd_hip_plugin>
{
public:
    grsd_hip_descriptor(int robotNum = 1, int thisID = 0, int device = 0) { init(defaults(robotNum, thisID, device)); }

    // every field of scl_grsd_config (ne_radius, grsd_radius, dist_thres, num_exclude_recent, tree_making_period, inter_mode, ...)
    explicit grsd_hip_descriptor(const scl_grsd_config &cfg) { init(cfg); }
};
