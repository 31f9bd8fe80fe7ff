// Host plan of the relative-pose edges (include/relpose_types.h, csrc/kernels/relpose_kernels.hip): which edges every
// free pose walks and which block of an upper block-CSR destination an edge's off-diagonal term goes to.  Host only:
// no HIP header is needed here or in relpose_plan.cpp (the upload lives in c_api.cpp), so the file can be compiled
// and run under a CPU sanitizer on its own.
#pragma once
#include <cstdint>
#include <vector>

namespace cugo_host
{

struct RelPosePlanHost
{
    int n = 0, n_poses_total = 0, n_poses_free = 0;
    int nnzb = 0; // blocks of the pattern the plan was built against
    // incidence lists: the counting edges (not flagged inactive, at least one free end) of free pose p are
    // inc[inc_ptr[p] .. inc_ptr[p+1]) in edge order, each entry edge << 1 | side (side 0: p is the edge's a, 1: its b)
    std::vector<int32_t> inc_ptr; // [n_poses_free + 1]
    std::vector<int32_t> inc;
    // block index of the (lo, hi) block of a counting edge between two free poses, -1 for every other edge
    std::vector<int32_t> off_blk; // [n]
};

// edges that count: not flagged CUGO_EDGE_INACTIVE (flags may be null: all active) and at least one end free (index
// < n_poses_free).  rowptr / colind: upper block CSR over the free poses, the diagonal block first in every row and the
// columns of a row ascending (the layout cugo_chol_analyze takes).  Throws std::invalid_argument on an index out of
// [0, n_poses_total), on a == b (whatever the edge's flags), on a pattern that is not of that form and on a counting
// free-free edge whose (lo, hi) block the pattern lacks.
void build_relpose_plan(int n, int n_poses_total, int n_poses_free, const int32_t* pose_a, const int32_t* pose_b,
                        const uint8_t* flags, const int32_t* rowptr, const int32_t* colind, RelPosePlanHost& out);

// the upper block-CSR pattern of a pure pose graph: row p holds p, then every hi > p joined to p by a counting
// free-free edge, ascending.  rowptr [n_poses_free + 1]; colind may be null (size query): the block count is returned
// either way.  Indices >= n_poses_free are fixed poses; throws std::invalid_argument on a negative index or a == b.
int relpose_pattern(int n, int n_poses_free, const int32_t* pose_a, const int32_t* pose_b, const uint8_t* flags,
                    int32_t* rowptr, int32_t* colind);

} // namespace cugo_host
