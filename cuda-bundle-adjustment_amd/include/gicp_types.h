// EXTENSION (the reference has no such edge): the COVARIANCE form of the two point kinds of the cugo API — the cost of
// generalised ICP (Segal, Haehnel, Thrun; fast_gicp, small_gicp, PCL's GeneralizedIterativeClosestPoint).  An edge
// carries two points and two 3 x 3 covariances instead of an information matrix, and the information FOLLOWS the poses:
//   S = C_z + M C_p M^T,  Omega = S^-1
//   GicpEdge      (one pose vertex; scan to fixed map): p and C_p in the world frame, z and C_z in the pose's frame, M = R
//   GicpPairEdge  (vertex 0 = a, vertex 1 = b; scan to scan): p and C_p in a's frame, z and C_z in b's, M = R_b R_a^T
// With this Omega, r, J, x = max(0, r^T Omega r), the robust kernel and the blocks of H and b are exactly those of
// PointEdge (point_edge_types.h) / PointPairEdge (point_pair_types.h).  Omega is rebuilt from the two covariances at every
// linearisation, and the cost of every trial step of the LM loop is evaluated with the Omega of the TRIAL poses: the
// minimised cost is the GICP cost and the gain ratio is computed against it; one optimize() converges without an outer
// loop that re-flattens the graph.  The Jacobian does NOT differentiate Omega (no GICP implementation does), and log det S
// is not part of the cost.  The marginal covariance functions use the Gauss-Newton H with Omega at the final poses.
//
// The term is in csrc/kernels/point_term.h (cov_information), point_kernels.hip and point_pair_kernels.hip.  The sets are
// plain containers like the others: add them with addEdgeSet() next to BA sets, priors, relative-pose edges, plane / line
// sets and a point set of the OTHER arity, or alone; initialize() recognises them by type (their dim() is 3).  It checks
// every active edge: finite values; each covariance symmetric to 1e-12 max|C| and positive semi-definite to -1e-12
// lambda_max; lambda_min(C_p) + lambda_min(C_z) > 1e-12 (lambda_max(C_p) + lambda_max(C_z)), which by Weyl's inequality
// makes S positive definite for EVERY rotation (a planar, rank-2 C_p with a regular C_z is legal); the ends in pose sets
// of the optimiser, a != b.
// Refused, each with a message that names the set (a later change may lift each): a covariance-form set and an
// information-form set of the SAME arity in one optimiser (GicpEdgeSet with PointEdgeSet, GicpPairEdgeSet with
// PointPairEdgeSet: one kind has one payload width); setOutlierThreshold(t > 0); a landmark-sharded optimiser (setShard /
// setComm); CUGO_HSC_STRIP=1 with a pair set; sets of one kind that disagree on the robust kernel.  Not yet:
// correspondences re-associated inside optimize(), a landmark-frame variant, dOmega/dxi and the log det term.
// Also reachable through the kernel-level C ABI (include/cugo_hip.h: cugo_gicp_edges, cugo_gicp_pair_edges and the
// cugo_gicp_* / cugo_gicp_pair_* passes).
#pragma once
#include <algorithm>

#include "optimisable_graph.h"

namespace cugo
{

/** two points and their 3 x 3 covariances (symmetric, so row- and column-major agree) */
template <typename S>
class PointCovarianceMatch
{
public:
    S pointP[3];
    S pointZ[3];
    S covP[9];
    S covZ[9];

    PointCovarianceMatch() // the origin twice, two identity matrices
    {
        for (int i = 0; i < 3; i++)
            pointP[i] = pointZ[i] = S(0);
        for (int i = 0; i < 9; i++)
            covP[i] = covZ[i] = i % 4 == 0 ? S(1) : S(0);
    }
    PointCovarianceMatch(const S* p, const S* z, const S* covP9, const S* covZ9)
    {
        std::copy(p, p + 3, pointP);
        std::copy(z, z + 3, pointZ);
        std::copy(covP9, covP9 + 9, covP);
        std::copy(covZ9, covZ9 + 9, covZ);
    }
};

class CUGO_API GicpEdge : public Edge<3, PointCovarianceMatch<double>, PoseVertex>
{
public:
    void* getMeasurement() noexcept override
    {
        this->touchOwner(); // mutable pointer: counts as a change (optimisable_graph.h, change tracking)
        return static_cast<void*>(&this->measurement);
    }
    const void* measurementData() const noexcept override { return static_cast<const void*>(&this->measurement); }
};

/** The covariances are always the edges' own; setInformation() of the base class is not used.  The robust kernel is the
 *  set's own */
class CUGO_API GicpEdgeSet : public EdgeSet<3, PointCovarianceMatch<double>, PoseVertex>
{
};

class CUGO_API GicpPairEdge : public Edge<3, PointCovarianceMatch<double>, PoseVertex, PoseVertex>
{
public:
    void* getMeasurement() noexcept override
    {
        this->touchOwner();
        return static_cast<void*>(&this->measurement);
    }
    const void* measurementData() const noexcept override { return static_cast<const void*>(&this->measurement); }
};

class CUGO_API GicpPairEdgeSet : public EdgeSet<3, PointCovarianceMatch<double>, PoseVertex, PoseVertex>
{
};

} // namespace cugo
