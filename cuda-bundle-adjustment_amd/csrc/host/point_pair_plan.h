// Host plan of the pose-pose point edges (csrc/kernels/point_pair_kernels.hip): the stable sort of the edges into runs
// of one (a, b) orientation of a pose pair, which runs every free pose's diagonal block is summed from, and which block
// of an upper block-CSR destination the off-diagonal partials of a run go to.  Host only: no HIP header is needed here
// or in point_pair_plan.cpp (the upload lives in c_api.cpp), so the file can be compiled and run under a CPU sanitizer
// on its own.
#pragma once
#include <cstdint>
#include <vector>

namespace cugo_host
{

// bits of PointPairPlanHost::run_flags
constexpr int32_t PAIR_RUN_A_FREE = 1;  // a < n_poses_free
constexpr int32_t PAIR_RUN_B_FREE = 2;  // b < n_poses_free
constexpr int32_t PAIR_RUN_A_IS_HI = 4; // a > b: the run's off-diagonal partial H_ab is the TRANSPOSE of the (lo, hi) block
constexpr int32_t PAIR_RUN_COUNTS = 8;  // at least one edge of the run is active and at least one end is free

struct PointPairPlanHost
{
    int n = 0, n_poses_total = 0, n_poses_free = 0;
    int nnzb = 0; // blocks of the pattern the plan was built against
    // The sort.  Edge perm[i] of the container stands at position i; the key is (lo, hi, orientation) with lo = min(a, b),
    // hi = max(a, b), orientation 0 for a < b, and the container order inside a run (a stable sort).  Every edge is
    // sorted, whether it counts or not: an inactive edge keeps its place in its run and contributes zeros.
    std::vector<int32_t> perm;     // [n]
    std::vector<int32_t> edge_run; // [n] run of the edge at sorted position i, ascending
    // The runs, in sorted order; the two runs of one pair (a -> b and b -> a) are adjacent.
    std::vector<int32_t> run_ptr;   // [n_runs + 1] CSR over the sorted positions
    std::vector<int32_t> run_a;     // [n_runs]
    std::vector<int32_t> run_b;     // [n_runs]
    std::vector<int32_t> run_flags; // [n_runs] PAIR_RUN_*
    std::vector<int32_t> run_blk;   // [n_runs] block index of (lo, hi) in the pattern; -1 unless the run counts and both ends are free
    // Per free pose p: the counting runs with p as an end, ascending, each entry run << 1 | side (side 0: p is the run's
    // a, 1: its b): what the pose's diagonal block and b are summed from.
    std::vector<int32_t> inc_ptr; // [n_poses_free + 1]
    std::vector<int32_t> inc;
    // Per pattern block that a counting free-free run maps to, ascending by first run: its runs (one or two), ascending.
    std::vector<int32_t> blk_id;  // [n_blocks_touched]
    std::vector<int32_t> blk_ptr; // [n_blocks_touched + 1]
    std::vector<int32_t> blk_run;
    // The pair list for the pattern: the distinct (lo, hi) of the counting free-free runs, ascending.
    std::vector<int32_t> pair_lo, pair_hi;
};

// Edges that count: not flagged CUGO_EDGE_INACTIVE (flags may be null: all active) and at least one end free (index
// < n_poses_free).  rowptr / colind: upper block CSR over the free poses, the diagonal block first in every row and the
// columns of a row ascending (the layout cugo_chol_analyze takes); both may be null for a plan without a destination
// (every run_blk is -1 then and nnzb 0: the pair list is what the caller wants).  Throws std::invalid_argument on an
// index out of [0, n_poses_total), on a == b (whatever the edge's flags), on a pattern that is not of that form and on
// a counting free-free pair whose (lo, hi) block the pattern lacks: the contracts of build_relpose_plan.
void build_point_pair_plan(int n, int n_poses_total, int n_poses_free, const int32_t* pose_a, const int32_t* pose_b,
                           const uint8_t* flags, const int32_t* rowptr, const int32_t* colind, PointPairPlanHost& out);

} // namespace cugo_host
