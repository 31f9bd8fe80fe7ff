// EXTENSION (the reference has no such edge): pose-pose point edges of the cugo API — binary edges between two pose
// vertices a (vertex 0) and b (vertex 1) for scan-to-scan registration.  An edge carries a point p measured in a's frame
// (pointP), the same physical point measured as q in b's frame (pointZ) and a symmetric positive SEMI-definite 3 x 3
// information Omega expressed in b's frame.  With the poses read as everywhere else (y = R(q) X + t is world -> frame), the
// left update T <- Exp([omega, upsilon]) T and the tangent order [omega, upsilon]:
//   X   = R_a^T (p - t_a)                    (the point in the world)
//   y   = R_b X + t_b                        (predicted in b's frame)
//   r   = y - q
//   J_b = dr/dxi_b = [ -[y]x | I ]           (the unary point edge's Jacobian, point_edge_types.h)
//   J_a = dr/dxi_a = R_BA [ [p]x | -I ],     R_BA = R_b R_a^T
//   x = max(0, r^T Omega r),  chi2 term rho(x) with the set's robust kernel,  w = rho'(x)
//   H_aa += w J_a^T Omega J_a,  H_bb += w J_b^T Omega J_b,  H_(lo,hi) += w J_lo^T Omega J_hi   (lo < hi: free pose indices)
//   b_a  -= w J_a^T Omega r,    b_b  -= w J_b^T Omega r
// With T_a the fixed identity the term is that of the PointEdge (p, z = q, Omega) on pose b, term for term.  An edge with
// one fixed end counts in chi2 and adds only its free end's block and b; an edge between two fixed poses and an inactive
// edge count for nothing.  Singular Omega is legal: plane-to-plane and line correspondences are special cases, as for the
// point kind.
// Uses: LiDAR / RGB-D multi-scan registration (Lu-Milios, multiway ICP, the refinement step behind a pose graph);
// scan-to-scan generalised ICP with Omega = (C_q + R C_p R^T)^-1 frozen per outer iteration (GicpPairEdgeSet of
// gicp_types.h rebuilds Omega at the poses of every pass); submap alignment.
// The term is in csrc/kernels/point_pair_kernels.hip.  The set is a plain container like the others: add it with
// addEdgeSet() next to any other set or alone; initialize() recognises it by type (its dim() is 3, like a stereo set's),
// checks every active edge (finite values, Omega symmetric to 1e-12 max|Omega| and positive semi-definite to -1e-12
// lambda_max, both ends in pose sets of the optimiser, a != b) and optimize() minimises the joint cost; every pose pair a
// counting edge joins becomes a block of the Schur complement's pattern, as for relpose_types.h.
// Refused, each with a message that names the set (a later change may lift each): setOutlierThreshold(t > 0) on the set,
// whatever GraphOptimisationOptions::poseEdgeOutlierRejection says; pair sets that disagree on the robust kernel; a
// landmark-sharded optimiser (setShard / setComm); CUGO_HSC_STRIP=1 (a pair block has no landmark product).  An Omega
// that follows the rotation during a solve is GicpPairEdgeSet (gicp_types.h: Omega = (C_q + M C_p M^T)^-1 rebuilt at
// every linearisation and trial), which cannot share an optimiser with a PointPairEdgeSet that has edges and has the
// refusals above.  Not yet: correspondences re-associated inside optimize(), a landmark-frame variant.  Also reachable through the kernel-level C ABI (include/cugo_hip.h: cugo_point_pair_plan_create,
// cugo_point_pair_edges, cugo_point_pair_compute_errors, cugo_point_pair_construct_quadratic_form and its _schur, _diag
// and cugo_point_pair_add_offdiag_schur forms).
#pragma once
#include <algorithm>

#include "point_edge_types.h"

namespace cugo
{

/** PointToPointMatch of point_edge_types.h: pointP = p in a's frame, pointZ = q in b's frame, information = Omega */
class CUGO_API PointPairEdge : public Edge<3, PointToPointMatch<double>, PoseVertex, PoseVertex>
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
class CUGO_API PointPairEdgeSet : public EdgeSet<3, PointToPointMatch<double>, PoseVertex, PoseVertex>
{
public:
    PointPairEdgeSet()
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
