// m2dp_hip_descriptor.hpp -- header-only adapter that plugs the MI355X M2DP engine (scl_m2dp.h) into the reference's descriptor
// plugin interface, beside scan_context_hip_descriptor.hpp and lidar_iris_hip_descriptor.hpp.
//
// Include it AFTER the reference's descriptor.h (it needs `class scan_descriptor`, descriptor.h:21-36, and
// pcl::PointCloud<pcl::PointXYZI>).  The DescriptorType switch changes by one line:
//
//   distributedMapping.h:412   scanDescriptor = std::unique_ptr<scan_descriptor>(new m2dp_descriptor());
//   becomes                    scanDescriptor = std::unique_ptr<scan_descriptor>(new m2dp_hip_descriptor(0.3, 30, numberOfRobots, id));
//
// What differs from the reference's class, on purpose (scl_m2dp.h has the details):
//   * the detections work (the reference's have empty bodies, descriptor.h:1998-2006): 1-NN by squared L2 in nanoflann's float
//     order, the newest numExcludeRecent keyframes of this robot kept out of intra detection, a loop when the distance is below
//     distThres -- 0.3 is a PLACEHOLDER, not validated on real data; the second member of the pair is the distance;
//   * saveDescriptorAndKey reads all 192 floats makeAndSaveDescriptorAndKey emits (the reference reads 128);
//   * the PCA axes follow a sign rule (PCL's are unpinned), which makes the signature rotation invariant.
// The class itself, member by member: vector_plugin_hip_descriptor.hpp.  The descriptor is the 192 floats [u, v]
// (descriptor.h:1820-1863; saveDescriptorAndKey 1989-1995; the detections 1998-2001 and 2003-2006; getIndex 2008-2011; getSize
// 2013-2016).
// Errors are written to stderr and mapped to "no loop" / empty results, as the reference only logs.
// Lifetime: as for scan_context_hip_descriptor -- scan_descriptor has no virtual destructor, call close() before
// dropping the object if the host re-creates descriptors.
#pragma once

#include "scl_m2dp.h"
#include "vector_plugin_hip_descriptor.hpp"

struct m2dp_hip_plugin {
    typedef scl_m2dp handle;
    typedef scl_m2dp_config config;
    enum { DIM = SCL_M2DP_DIM };
    static const char *name() { return "m2dp_hip_descriptor"; }
    static const scl_vector_plugin_api<scl_m2dp, scl_m2dp_config> &api()
    {
        static const scl_vector_plugin_api<scl_m2dp, scl_m2dp_config> a = SCL_VECTOR_PLUGIN_API(scl_m2dp);
        return a;
    }
};

class m2dp_hip_descriptor : public vector_plugin_hip_descriptor<m2dp_hip_plugin>
{
public:
    m2dp_hip_descriptor(double distThres = 0.3, int numExcludeRecent = 30, int robotNum = 1, int thisID = 0, int device = 0)
    {
        scl_m2dp_config cfg = defaults(robotNum, thisID, device);
        cfg.dist_thres = distThres; cfg.num_exclude_recent = numExcludeRecent;
        init(cfg);
    }
};
