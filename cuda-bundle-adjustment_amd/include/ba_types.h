// Bundle-adjustment edge types of the cugo API (ref: include/ba_types.h:34-260).
// g2o mapping: MonoEdge <-> EdgeSE3ProjectXYZ, StereoEdge <-> EdgeStereoSE3ProjectXYZ;
// vertex 0 = pose (VertexSE3Expmap), vertex 1 = landmark (VertexSBAPointXYZ).
// The reference's per-set virtual computeError / constructQuadraticForm dispatch into
// gpu::computeActiveErrors_<M> / constructQuadraticForm_<M>; here all sets of an optimiser
// are flattened into ONE landmark-major edge array (mono and stereo distinguished by a flag
// bit), so the sets are plain containers.
// DepthEdge / DepthEdgeSet (ref: include/ba_types.h:171-260), the RGB-D observation (u, v, 1/Z), go into the same array
// under a flag bit of their own.  Their residual is the reference's (computeActiveErrors_DepthBa) with its true
// Jacobian — the reference pairs it with the stereo Jacobian — and an inverse-depth weight, an extension (DESIGN.md
// section 17).
#pragma once
#include "optimisable_graph.h"

namespace cugo
{

/** monocular observation: measurement (u, v) */
class CUGO_API MonoEdge : public Edge<2, Vec2d, PoseVertex, LandmarkVertex>
{
public:
    void* getMeasurement() noexcept override
    {
        touchOwner(); // mutable pointer: counts as a change (optimisable_graph.h, change tracking)
        return static_cast<void*>(measurement.data);
    }
    const void* measurementData() const noexcept override { return static_cast<const void*>(measurement.data); }
};

/** stereo observation: measurement (u, v, u_right) */
class CUGO_API StereoEdge : public Edge<3, Vec3d, PoseVertex, LandmarkVertex>
{
public:
    void* getMeasurement() noexcept override
    {
        touchOwner();
        return static_cast<void*>(measurement.data);
    }
    const void* measurementData() const noexcept override { return static_cast<const void*>(measurement.data); }
};

/** RGB-D observation: measurement (u, v, 1/Z); bf of the camera is not used */
class CUGO_API DepthEdge : public Edge<3, Vec3d, PoseVertex, LandmarkVertex>
{
public:
    void* getMeasurement() noexcept override
    {
        touchOwner();
        return static_cast<void*>(measurement.data);
    }
    const void* measurementData() const noexcept override { return static_cast<const void*>(measurement.data); }
};

/** Extension, for both sets below: setSensorPose(T_sb) gives the set's camera a fixed pose body -> sensor and makes the
 *  pose vertices body poses — one MonoEdgeSet per physical camera is a rig (optimisable_graph.h, BaseEdge::setSensorPose).
 *  A DepthEdgeSet with a sensor pose other than the identity is refused by initialize() (not yet) */
class CUGO_API MonoEdgeSet : public EdgeSet<2, Vec2d, PoseVertex, LandmarkVertex>
{
};

class CUGO_API StereoEdgeSet : public EdgeSet<3, Vec3d, PoseVertex, LandmarkVertex>
{
};

/** Residual (pu - u, pv - v, sqrt(k) (1/Z - m_d)) under the set's (or the edges') scalar information.  k, the
 *  inverse-depth weight, is an extension: it puts inverse metres (sigma ~ 1e-3) on the scale of pixels (sigma ~ 1), which
 *  one scalar information cannot; 1 (the default) is the reference's chi2.  It must be finite and > 0 and the same in
 *  every depth set of an optimiser: initialize() refuses anything else.  Changing it counts as a change of the set */
class CUGO_API DepthEdgeSet : public EdgeSet<3, Vec3d, PoseVertex, LandmarkVertex>
{
public:
    void setInverseDepthWeight(double k) noexcept
    {
        this->touch();
        inverseDepthWeight_ = k;
    }
    double inverseDepthWeight() const noexcept { return inverseDepthWeight_; }

private:
    double inverseDepthWeight_ = 1.0;
};

} // namespace cugo
