// EXTENSION (the reference has no such edge; g2o calls it EdgeXYZPrior): landmark position priors of the cugo API — unary
// edges on one landmark vertex with a measured position Z and a full 3 x 3 information matrix Omega.  With the landmark
// estimate X the residual is
//   r = X - Z,  J = I
// and the cost term rho(r^T Omega r) with the set's robust kernel.  A prior with Z = the estimate and Omega = Sigma^-1
// is exactly the Gaussian a marginal landmark covariance describes (what a sliding window keeps of a
// landmark whose other observers it drops).
// Uses: surveyed control points and GPS-tagged targets that hold gauge and scale of a monocular map, LiDAR- or
// depth-anchored map points, marginal priors, a weak prior that makes a landmark with one mono observation well-posed.
// The term is in csrc/kernels/lm_prior_term.h; in the LM loop it rides inside the BA build pass.  The set is a plain
// container like the others: add it with addEdgeSet() next to the BA sets; initialize() recognises it by type (its dim()
// is 3, like a stereo set's), checks every active edge (finite values, Omega symmetric to 1e-12 max|Omega| and positive
// semi-definite to -1e-12 lambda_max, a landmark of one of the optimiser's landmark sets) and optimize() minimises the
// joint cost.  Priors on fixed landmarks and inactive priors count for nothing; several priors on one landmark are
// allowed.  Refused: a prior that counts on a free landmark which no active BA edge observes (the back-substitution gives
// such a landmark a zero step), setOutlierThreshold(t > 0) on the set, and sharded optimisers.  Also reachable through the
// kernel-level C ABI (include/cugo_hip.h: cugo_lm_prior_edges, cugo_lm_prior_compute_errors,
// cugo_lm_prior_construct_quadratic_form, cugo_construct_quadratic_form_lm_priors).
#pragma once
#include <algorithm>

#include "optimisable_graph.h"

namespace cugo
{

/** a measured position and its 3 x 3 information (symmetric, so row- and column-major agree) */
template <typename S>
class LandmarkPriorMatch
{
public:
    S point[3];
    S information[9];

    LandmarkPriorMatch() // the origin, the identity matrix
    {
        for (int i = 0; i < 3; i++)
            point[i] = S(0);
        for (int i = 0; i < 9; i++)
            information[i] = i % 4 == 0 ? S(1) : S(0);
    }
    LandmarkPriorMatch(const S* xyz, const S* info9)
    {
        std::copy(xyz, xyz + 3, point);
        std::copy(info9, info9 + 9, information);
    }
};

class CUGO_API LandmarkPriorEdge : public Edge<3, LandmarkPriorMatch<double>, LandmarkVertex>
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
class CUGO_API LandmarkPriorEdgeSet : public EdgeSet<3, LandmarkPriorMatch<double>, LandmarkVertex>
{
public:
    LandmarkPriorEdgeSet()
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
