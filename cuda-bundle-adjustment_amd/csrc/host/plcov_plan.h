// Host plan of a batch of pose-landmark covariance queries (k_pose_lm_cross / k_reprojection_cov of cov_kernels.hip):
// which pose pairs cugo_chol_inverse_blocks is asked for and, per query, which of those blocks every edge slot of the
// query's landmark reads.  Host only: no HIP header is needed here or in plcov_plan.cpp, so the file can be compiled
// and run under a CPU sanitizer on its own.
#pragma once
#include <cstdint>
#include <vector>

namespace cugo_host
{

struct PlCovPlanHost
{
    int n = 0; // queries
    // the distinct pose pairs, in the order of their first use: (a, p(e)) for every slot of a query's landmark whose
    // pose is free — whether or not the slot counts on the device: the kernel decides by flag, a surplus block is
    // harmless — and (a, a) once per distinct free a
    std::vector<int32_t> rows, cols;
    // query k owns q_slot[q_ptr[k] .. q_ptr[k+1]): one entry per slot of its landmark in slot order, the index of
    // the block Sigma_{a, p(e)} in rows / cols, -1 for a slot on a fixed pose.  The range of a query with a fixed pose or
    // a fixed landmark is empty
    std::vector<int32_t> q_ptr, q_slot;
    std::vector<int32_t> q_aa; // [n] the index of Sigma_aa, -1 for a fixed pose
};

// lm_ptr [n_landmarks + 1]: the slot range of every landmark a query may name (free landmarks first, as the flattening
// has them); slot_pose: the pose index of every slot in landmark-major slot order (>= n_poses_free: a fixed pose).
// Query k is (q_pose[k], q_lm[k]): a free pose index or -1 for a fixed pose, a free landmark index or -1.
// Throws std::invalid_argument on a negative count, a null array that is needed, an index out of range, a descending
// lm_ptr or a negative slot pose of a queried landmark.
void build_plcov_plan(int n_poses_free, int n_landmarks, const int32_t* lm_ptr, const int32_t* slot_pose, int n,
                      const int32_t* q_pose, const int32_t* q_lm, PlCovPlanHost& out);

} // namespace cugo_host
