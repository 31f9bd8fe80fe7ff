// EXTENSION (the reference has no such edge; g2o calls it EdgeSE3): relative-pose SE(3) edges of the cugo API — binary
// edges between two pose vertices a and b with a measured relative pose Z ~ T_a T_b^-1 and a full 6 x 6 information
// matrix Omega: odometry and IMU-preintegration constraints between keyframes, loop closures, the essential graph.
// With the poses read as the BA edges read them (y = R(q) p + t) and the left update T <- Exp([omega, upsilon]) T:
//   A = T_a T_b^-1 = (R_A, t_A),   D = A Z^-1 = (R_D, t_D)
//   r = [ Log_SO3(R_D) ; t_D ]                     (tangent order [rotation, translation], as for the priors)
//   J_a = dr/dxi_a = [ J_l^-1(phi) 0 ; -[t_D]x I ] (exactly the prior's Jacobian, prior_types.h, with this D)
//   J_b = dr/dxi_b = -J_a Ad(A),   Ad(A) = [ R_A 0 ; [t_A]x R_A  R_A ]
//   x = max(0, r^T Omega r), chi2 term rho(x) with the set's robust kernel, w = rho'(x)
//   H_aa += w J_a^T Omega J_a,  H_bb += w J_b^T Omega J_b,  H_(lo,hi) += w J_lo^T Omega J_hi  (lo < hi: the pose indices)
//   b_a -= w J_a^T Omega r,     b_b -= w J_b^T Omega r
// With T_b the fixed identity this is the pose prior, term for term.  An edge with one fixed end counts in chi2 and adds
// only its free end's block and b; an edge between two fixed poses counts for nothing; a == b is refused.
// The residual, the Jacobians and the device kernel are in csrc/kernels/relpose_kernels.hip.  The set is a plain
// container like the others, vertex 0 = a, vertex 1 = b: add it with addEdgeSet() next to (or instead of) the others.
// The optimiser takes it when GraphOptimisationOptions::relativePoseEdges is on: initialize() recognises the set by
// type, checks every active edge (finite values, |q_z| = 1 to 1e-6, Omega symmetric to 1e-12 max|Omega| and positive
// semi-definite to -1e-12 lambda_max, a != b, both ends in pose sets of the optimiser), merges the pose pairs into the
// Hsc pattern and optimize() minimises the joint cost; inactive edges and edges between two fixed poses are dropped.
// setOutlierThreshold(t > 0) on the set — the gate for false loop closures — takes effect with GraphOptimisationOptions::
// poseEdgeOutlierRejection: at the end of optimize() every edge whose chi2 term exceeds t is inactivated, counted in
// getOutlierCount() and left out by the next initialize() (a pair that loses its last edge leaves the pattern then);
// with that option off (the default) such a threshold is refused.  Sets that disagree on the robust kernel and sharded
// optimisers are refused.  With the relativePoseEdges
// option off (the default) initialize() refuses the set and names the option and the kernel-level C ABI, through which
// the terms are reachable as well (include/cugo_hip.h: cugo_relpose_edges, cugo_relpose_plan_create,
// cugo_relpose_compute_errors, cugo_relpose_construct_quadratic_form[_schur]).
#pragma once
#include "prior_types.h"

namespace cugo
{

/** measurement: PosePriorMatch (the measured relative pose Z and its 6 x 6 information); vertex 0 is a, vertex 1 is b */
class CUGO_API RelPoseEdge : public Se3Edge<PoseVertex, PoseVertex>
{
};

/** the information matrix of the set: as PosePriorEdgeSet's (prior_types.h: Se3EdgeSet) */
class CUGO_API RelPoseEdgeSet : public Se3EdgeSet<PoseVertex, PoseVertex>
{
};

} // namespace cugo
