// EXTENSION (the reference has no such edge): point-to-point pose edges of the cugo API — unary edges on one pose vertex
// with a known 3-D point p, its measurement z in the pose's frame and a full 3 x 3 information matrix Omega.  With the
// pose (q, t) read as everywhere else (y = R(q) p + t) and the left update in the tangent order [omega, upsilon]:
//   r = y - z,  J = dr/dxi = [ -[y]x | I ]
// and the cost term rho(r^T Omega r) with the set's robust kernel.  Omega is symmetric positive SEMI-definite: singular
// matrices are legal, and the edges of icp_types.h are special cases (Omega = omega n n^T with z on the plane: PlaneEdge;
// Omega = omega (I - u u^T) with z = a: LineEdge).
// Uses: point-to-point ICP and the polishing step behind Horn / Umeyama; generalised ICP with Omega = (C_z + R C_p R^T)^-1
// frozen per outer iteration; 3-D - 3-D relocalisation of RGB-D / stereo frames against a fixed map; surveyed control
// points seen by a range sensor.
// The term is in csrc/kernels/point_kernels.hip.  The set is a plain container like the others: add it with addEdgeSet()
// next to any other set or alone; initialize() recognises it by type (its dim() is 3, like a stereo set's), checks every
// active edge (finite values, Omega symmetric to 1e-12 max|Omega| and positive semi-definite to -1e-12 lambda_max, a pose
// of one of the optimiser's pose sets) and optimize() minimises the joint cost.  Edges on fixed poses and inactive edges
// count for nothing.  Refused: setOutlierThreshold(t > 0) on the set (not yet supported, whatever
// GraphOptimisationOptions::poseEdgeOutlierRejection says), point sets that disagree on the robust kernel, and
// landmark-sharded optimisers.  An Omega that follows the pose during a solve is GicpEdgeSet (gicp_types.h: Omega = (C_z +
// R C_p R^T)^-1 rebuilt at every linearisation and trial); refused: a GicpEdgeSet and a PointEdgeSet with edges in one
// optimiser.  Also reachable through the kernel-level C ABI (include/cugo_hip.h: cugo_point_edges,
// cugo_point_compute_errors, cugo_point_construct_quadratic_form, cugo_point_construct_quadratic_form_schur).
#pragma once
#include <algorithm>

#include "optimisable_graph.h"

namespace cugo
{

/** a point, its measurement in the pose's frame and the 3 x 3 information (symmetric, so row- and column-major agree) */
template <typename S>
class PointToPointMatch
{
public:
    S pointP[3];
    S pointZ[3];
    S information[9];

    PointToPointMatch() // the origin twice, the identity matrix
    {
        for (int i = 0; i < 3; i++)
            pointP[i] = pointZ[i] = S(0);
        for (int i = 0; i < 9; i++)
            information[i] = i % 4 == 0 ? S(1) : S(0);
    }
    PointToPointMatch(const S* p, const S* z)
    {
        std::copy(p, p + 3, pointP);
        std::copy(z, z + 3, pointZ);
        for (int i = 0; i < 9; i++)
            information[i] = i % 4 == 0 ? S(1) : S(0);
    }
    PointToPointMatch(const S* p, const S* z, const S* info9)
    {
        std::copy(p, p + 3, pointP);
        std::copy(z, z + 3, pointZ);
        std::copy(info9, info9 + 9, information);
    }
};

class CUGO_API PointEdge : public Edge<3, PointToPointMatch<double>, PoseVertex>
{
public:
    void* getMeasurement() noexcept override
    {
        this->touchOwner(); // mutable pointer: counts as a change (optimisable_graph.h, change tracking)
        return static_cast<void*>(&this->measurement);
    }
    const void* measurementData() const noexcept override { return static_cast<const void*>(&this->measurement); }
};

/** With GraphOptimisationOptions::perEdgeInformation the edges' own matrices count, otherwise the set's (the identity
 *  until setInformationMatrix is called); the scalar setInformation() of the base class is not used.  The robust kernel
 *  is the set's own */
class CUGO_API PointEdgeSet : public EdgeSet<3, PointToPointMatch<double>, PoseVertex>
{
public:
    PointEdgeSet()
    {
        for (int i = 0; i < 9; i++)
            info9_[i] = i % 4 == 0 ? 1.0 : 0.0;
    }
    void setInformationMatrix(const double* info9) noexcept
    {
        this->touch();
        std::copy(info9, info9 + 9, info9_);
    }
    const double* informationMatrix() const noexcept { return info9_; }

private:
    double info9_[9];
};

} // namespace cugo
