// Host-only layout of a flattened graph: what Engine::initialize() / build_structure() compute on plain vectors
// before (or without) a device.  No HIP, no Engine::Impl: free functions over FlatGraph and caller-owned vectors (the
// engine keeps its staging vectors between calls: a fresh 40 MB costs more in page faults than the work done on it,
// so nothing here returns a vector by value).  Every sum and every order the kernels later see is fixed by these arrays.
#pragma once
#include <cstdint>
#include <functional>
#include <vector>

#include "engine.h"

namespace cugo_host
{
using Idx = std::vector<int32_t>;

// Edge slots per group: k_build_edges, the back-substitution and the landmark-major Schur plan (kSchurGroup) sum a
// landmark's edges inside one workgroup of this many threads
constexpr int kSlotGroup = 256;

// an active edge between a free pose and a free landmark: the only edges with an Hpl block
inline bool is_free_free(uint8_t flags)
{
    return (flags & (CUGO_EDGE_FIXED_L | CUGO_EDGE_FIXED_P | CUGO_EDGE_INACTIVE)) == 0;
}
double count_free_free(const std::vector<uint8_t>& flags);

// byte compare over the pool that stops at the first difference (the lists are megabytes, a new graph differs early)
bool same_bytes(const void* a, const void* b, size_t bytes);
template <typename T>
inline bool same_bytes(const std::vector<T>& a, const std::vector<T>& b)
{
    return a.size() == b.size() && same_bytes(a.data(), b.data(), a.size() * sizeof(T));
}

// order[lm_cnt[l] .. lm_cnt[l + 1]): the edges of landmark l by pose, container order among equals
void sort_landmark_major(const FlatGraph& g, Idx& lm_cnt, Idx& order);
// global co-visibility (all shards): free landmark -> its free poses, ascending; throws on a duplicate free-free edge
void build_covisibility(const FlatGraph& g, const Idx& lm_cnt, const Idx& order, Idx& cov_ptr, Idx& cov_pose);
// contiguous landmark range of shard `rank`, balanced by edge count
void shard_range(const Idx& lm_cnt, int rank, int world, int& l0, int& l1);
// Slots of the edges of landmarks [l0, l1): landmark-major, padded with inactive slots so that no landmark with
// <= kSlotGroup edges straddles a group boundary.  A padding slot belongs to the landmark before it; slot_src[i] =
// index into `order`, or -1 for padding.  Returns whether every landmark's slots lie inside one group.
bool pad_slot_layout(const Idx& lm_cnt, int l0, int l1, Idx& lm_ptr, Idx& slot_src);

// what the edge kernels read per slot, and where a slot came from
struct SlotArrays
{
    Idx pose, lm;
    std::vector<uint8_t> flags;
    std::vector<double> meas;  // planar: [3][E]
    std::vector<double> omega; // E, or 1 when uniform
    std::vector<uint16_t> cam; // E, or empty with a single camera
    int n_omega = 1, n_cams = 1;
    Idx slot_edge;                      // slot -> edge index of the FlatGraph (-1: padding)
    std::vector<double> slot_threshold; // slot -> outlier threshold (empty: rejection disabled)
};
void fill_slots(const FlatGraph& g, const Idx& order, const Idx& slot_src, SlotArrays& out);
// pose_edge[pose_ptr[p] .. pose_ptr[p + 1]): the real slots of pose p in slot order (= ascending landmark)
void pose_major_view(int Pall, const Idx& slot_pose, const Idx& slot_src, Idx& pose_ptr, Idx& pose_edge);

// the pose edges of one kind as the kernels read them, planar: meas [meas_w][n], weight [weight_w][n_weight] with
// n_weight = n, or 1 when one value serves all (an empty kind: one column of zeros)
struct PoseKindHost
{
    Idx h_pose, h_pose_b, h_ptr, slot_set, slot_edge; // (h_pose_b: relative pose alone; h_ptr: the unary kinds alone)
    std::vector<double> h_meas, h_weight;
    int n_weight = 1;
    std::vector<double> h_threshold; // FlatPoseKind::threshold in the order of the slots (n entries, 1, or empty)
};
// edge e of the kind to slot slot_of[e] (nullptr: the edges stay in container order); slot_set / slot_edge: where the
// edge of a slot came from
void copy_pose_edges_planar(const FlatPoseKind& kind, const int32_t* slot_of, PoseKindHost& out);
// a unary kind sorted by pose (stable: container order inside a pose), with the CSR h_ptr over all Pall poses; throws
// on an edge that is not on a free pose
void sort_pose_edges_by_pose(const FlatPoseKind& kind, int Pall, int P, PoseKindHost& out);
// the pose-pose point kind sorted into the runs of its plan (point_pair_plan.h: by (lo, hi, orientation), stable: container
// order inside a run).  The sort needs no pattern: `plan` comes back built without one
struct PointPairPlanHost;
void sort_pose_edges_by_pair(const FlatPoseKind& kind, int Pall, int P, PointPairPlanHost& plan, PoseKindHost& out);

// ---- the Hsc structure on the host: pattern (upper block CSR, diagonal first) and, from the LOCAL slots, the
// contributions of the off-diagonal blocks (ascending landmark inside a block).  use_plan() is asked once the pattern
// exists: true = a landmark-major plan (schur_plan.h) serves and the lists stay empty.  lap(label) after every pass.
// pair_lo / pair_hi (optional, ascending by (lo, hi), lo < hi < P): pose pairs joined by relative-pose edges; each gets a
// block of the pattern, with an empty contribution range unless the two poses share a landmark.  The products and the
// lists come from the slots alone.
struct HostStructure
{
    double products = 0;         // all products of the graph (a free-free edge also has its diagonal one)
    Idx off_ptr, off_ei, off_ej; // per block: the two edge slots of each contribution
};
void host_structure(int P, int L, const Idx& cov_ptr, const Idx& cov_pose, const SlotArrays& slots, const Idx& lm_ptr,
                    const Idx& pose_ptr, const Idx& pose_edge, const std::function<bool()>& use_plan,
                    const std::function<void(const char*)>& lap, Idx& rowptr, Idx& colind, HostStructure& out,
                    const Idx* pair_lo = nullptr, const Idx* pair_hi = nullptr);

} // namespace cugo_host
