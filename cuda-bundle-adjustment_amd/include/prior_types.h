// EXTENSION (the reference has no such edge; g2o calls it EdgeSE3Prior): SE(3) pose priors of the cugo API — unary edges
// on one pose vertex with a measured pose Z and a full 6 x 6 information matrix Omega.  With the pose estimate
// T = (q, t) read as the BA edges read it (y = R(q) p + t) and D = T Z^-1, the residual is
//   r = [ Log_SO3(R_D) ; t_D ],  R_D = R(q) R(q_z)^T,  t_D = t - R_D t_z
// in the tangent order [rotation, translation] of the left update T <- Exp(xi) T: the order of the 6 x 6 pose
// covariances computeMarginals() hands out.  The cost term is rho(r^T Omega r) with the set's robust kernel.  At r = 0
// the Jacobian is the identity, so a prior with Z = the estimate and Omega = Sigma^-1 is exactly the Gaussian a
// marginal covariance describes (what a sliding window keeps of a dropped keyframe).
// Uses: a motion prior for degenerate scan-to-map ICP, a soft gauge / GPS / odometry anchor, marginal priors.
// The residual, its Jacobian and the device kernel are in csrc/kernels/prior_kernels.hip.  The set is a plain container
// like the BA and ICP sets: add it with addEdgeSet() next to (or instead of) the others; initialize() recognises it by
// type, checks every active edge (finite values, |q_z| = 1 to 1e-6, Omega symmetric to 1e-12 max|Omega| and positive
// semi-definite to -1e-12 lambda_max, a pose of one of the optimiser's pose sets) and optimize() minimises the joint
// cost.  setOutlierThreshold(t > 0) on the set takes effect with GraphOptimisationOptions::poseEdgeOutlierRejection: at
// the end of optimize() every prior whose chi2 term exceeds t is inactivated and counted in getOutlierCount(); with the
// option off (the default) such a threshold is refused.  Sharded optimisers are refused.  Also reachable through the kernel-level C
// ABI (include/cugo_hip.h: cugo_prior_edges, cugo_prior_compute_errors, cugo_prior_construct_quadratic_form).
#pragma once
#include <algorithm>

#include "optimisable_graph.h"

namespace cugo
{

/** a measured pose and its 6 x 6 information (symmetric, so row- and column-major agree), order [rotation, translation] */
template <typename S>
class PosePriorMatch
{
public:
    Se3<S> pose;
    S information[36];

    PosePriorMatch() // the identity pose, the identity matrix
    {
        for (int i = 0; i < 36; i++)
            information[i] = i % 7 == 0 ? S(1) : S(0);
    }
    PosePriorMatch(const Se3<S>& z, const S* info36) : pose(z) { std::copy(info36, info36 + 36, information); }
};

/** what the SE(3) edge kinds share over their vertex list (one pose: the prior; two: relpose_types.h): the edge ... */
template <typename... VertexTypes>
class Se3Edge : public Edge<6, PosePriorMatch<double>, VertexTypes...>
{
public:
    void* getMeasurement() noexcept override
    {
        this->touchOwner(); // mutable pointer: counts as a change (optimisable_graph.h, change tracking)
        return static_cast<void*>(&this->measurement);
    }
    const void* measurementData() const noexcept override { return static_cast<const void*>(&this->measurement); }
};

/** ... and the set.  With GraphOptimisationOptions::perEdgeInformation the edges' own matrices count, otherwise the
 *  set's (the identity until setInformationMatrix is called); the scalar setInformation() of the base class is not
 *  used by these sets */
template <typename... VertexTypes>
class Se3EdgeSet : public EdgeSet<6, PosePriorMatch<double>, VertexTypes...>
{
public:
    Se3EdgeSet()
    {
        for (int i = 0; i < 36; i++)
            info36_[i] = i % 7 == 0 ? 1.0 : 0.0;
    }
    void setInformationMatrix(const double* info36) noexcept
    {
        this->touch();
        std::copy(info36, info36 + 36, info36_);
    }
    const double* informationMatrix() const noexcept { return info36_; }

private:
    double info36_[36];
};

class CUGO_API PosePriorEdge : public Se3Edge<PoseVertex>
{
};

class CUGO_API PosePriorEdgeSet : public Se3EdgeSet<PoseVertex>
{
};

} // namespace cugo
