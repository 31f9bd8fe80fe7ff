// Point-to-plane and point-to-line pose edges of the cugo API (ref: include/icp_types.h): unary edges on one pose
// vertex for LiDAR scan-to-map constraints.  With the pose estimate (q, t) read as the BA edges read it,
// y = R(q) pointP + t, the residuals are
//   plane: n . y - originDistance                 (scalar; dim() = 1 as in the reference)
//   line:  (I - u u^T)(y - a), u = (b - a) / |b - a|  (its length is the distance to the line)
// The residuals, their Jacobians for the left update and the device kernels are in csrc/kernels/icp_kernels.hip.
// The sets are plain containers, like the BA sets (ba_types.h): add them to the optimiser with addEdgeSet(), next to
// (or instead of) mono / stereo sets; initialize() checks every active edge (finite values, unit normal, a != b, a pose
// of one of the optimiser's pose sets) and optimize() minimises the joint cost.  setOutlierThreshold(t > 0) on a set
// (ref: EdgeSet::setOutlierThreshold / updateEdges, which the reference's sets inherit) takes effect with
// GraphOptimisationOptions::poseEdgeOutlierRejection: at the end of optimize() every edge of the set whose chi2 term
// exceeds t is inactivated and counted in getOutlierCount(); several sets of a kind may carry different thresholds.
// With the option off (the default) such a threshold is refused by initialize().  The same terms are also reachable
// through the kernel-level C ABI (include/cugo_hip.h: cugo_icp_edges, cugo_icp_compute_errors,
// cugo_icp_construct_quadratic_form).
#pragma once
#include "measurements.h"
#include "optimisable_graph.h"

namespace cugo
{

class CUGO_API PlaneEdge : public Edge<1, PointToPlaneMatch<double>, PoseVertex>
{
public:
    void* getMeasurement() noexcept override
    {
        touchOwner(); // mutable pointer: counts as a change (optimisable_graph.h, change tracking)
        return static_cast<void*>(&measurement);
    }
    const void* measurementData() const noexcept override { return static_cast<const void*>(&measurement); }
};

class CUGO_API LineEdge : public Edge<1, PointToLineMatch<double>, PoseVertex>
{
public:
    void* getMeasurement() noexcept override
    {
        touchOwner();
        return static_cast<void*>(&measurement);
    }
    const void* measurementData() const noexcept override { return static_cast<const void*>(&measurement); }
};

class CUGO_API PlaneEdgeSet : public EdgeSet<1, PointToPlaneMatch<double>, PoseVertex>
{
};

class CUGO_API LineEdgeSet : public EdgeSet<1, PointToLineMatch<double>, PoseVertex>
{
};

} // namespace cugo
