// Engine: device-resident BA solver driven by flat arrays.  It is the counterpart of the
// reference's BlockSolver (ref: src/block_solver.{h,cpp}) plus the LM loop of
// CudaGraphOptimisationImpl::optimize (ref: src/cuda_graph_optimisation.cpp:48-154).
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../../include/cugo_hip.h"

namespace cugo_host
{

class RcclComm;
struct InitLaps;
struct Options;

// Result of flattening a graph (ref: VertexSet::generateEstimateData + EdgeSet::init,
// src/optimisable_graph.hpp:84-126,474-572).  Indices: free vertices first.
// Edges of one kind on pose vertices alone (icp_types.h, prior_types.h: unary; relpose_types.h: binary), flattened in
// container order; inactive edges, edges all of whose poses are fixed and everything invalid never get here
// (graph_optimisation.cpp validates and drops)
enum PoseKind
{
    POSE_KIND_PLANE = 0,
    POSE_KIND_LINE,
    POSE_KIND_PRIOR,
    POSE_KIND_RELPOSE,
    POSE_KIND_POINT, // (unary; behind the four kinds of CUGO_POSE_KIND_*, whose values are those of this enum)
    POSE_KIND_PAIR,  // (binary: pose-pose point edges, point_pair_types.h; internal as the point kind is)
    POSE_KIND_COUNT
};
struct FlatPoseKind
{
    int kind = 0;                 // PoseKind
    int meas_w = 0, weight_w = 0; // doubles per edge: plane 7 (p, n, d) + 1, line 9 (p, a, unit direction) + 1, prior and
                                  // relative pose 7 (q x y z w, t) + 21 (upper triangle of Omega, row-major packed),
                                  // point and pose-pose point 6 (p, z) + 6 (upper triangle of the 3 x 3 Omega, row-major packed)
    std::vector<int32_t> pose;    // free-first pose index per edge: always < P on a unary kind; a of a binary edge
    std::vector<int32_t> pose_b;  // relative pose and pose-pose point: b (one of a, b may be a fixed pose, >= P); empty on the unary kinds
    std::vector<double> meas;     // E x meas_w
    std::vector<double> weight;   // E x weight_w, or 1 x weight_w when one value serves all
    std::vector<int32_t> src_set, src_edge; // where an edge came from: edge set (position among the optimiser's edge
                                            // sets) and position in that set's container
    std::vector<double> threshold; // outlier threshold of the edge's set (> 0, or 0: none), per edge; one entry when one
                                   // value serves all, empty when no set has one (collapse_thresholds)
    int rk = CUGO_RK_NONE;
    double delta = 1.0;
    bool rk_seen = false; // a non-empty edge set has settled rk / delta (further sets must agree)
    // point and pose-pose point only: the COVARIANCE form (gicp_types.h).  weight_w is then 12: the upper triangles of
    // C_p, then of C_z; the kernels form Omega from them at the poses of every pass
    bool cov = false;
    int n() const { return (int)pose.size(); }
    void clear()
    {
        pose.clear(), pose_b.clear(), meas.clear(), weight.clear(), src_set.clear(), src_edge.clear(), threshold.clear();
        rk = CUGO_RK_NONE, delta = 1.0, rk_seen = false;
        if (cov)
            weight_w = 6, cov = false;
    }
    void set_covariance_form() { cov = true, weight_w = 12; }
};
// a kind in messages about its edge sets, and in the engine's, which speak of the two ICP kinds as one
inline const char* pose_kind_name(int kind)
{
    return kind == POSE_KIND_PLANE  ? "point-to-plane"
           : kind == POSE_KIND_LINE ? "point-to-line"
           : kind == POSE_KIND_PRIOR ? "pose prior"
           : kind == POSE_KIND_POINT ? "point-to-point"
           : kind == POSE_KIND_PAIR  ? "pose-pose point"
                                     : "relative-pose";
}
inline const char* pose_kind_group(int kind)
{
    return kind == POSE_KIND_RELPOSE ? "relative-pose"
           : kind == POSE_KIND_PRIOR ? "pose prior"
           : kind == POSE_KIND_POINT ? "point-to-point"
           : kind == POSE_KIND_PAIR  ? "pose-pose point"
                                     : "point-to-plane / point-to-line";
}

// per-edge thresholds as flattened -> empty when none is positive, one entry when all are the same
inline void collapse_thresholds(std::vector<double>& t)
{
    bool uniform = true, any = false;
    for (size_t i = 0; i < t.size(); i++)
        uniform = uniform && t[i] == t[0], any = any || t[i] > 0.0;
    if (!any)
        t.clear();
    else if (uniform)
        t.resize(1);
}

// Landmark position priors (landmark_prior_types.h), flattened in container order: only priors that count get here
// (active, on a free landmark of the optimiser, values checked by graph_optimisation.cpp).  The engine sorts them by
// landmark (stable) and builds the CSR over all landmarks.
struct FlatLmPriors
{
    std::vector<int32_t> lm;  // free-first landmark index per prior, always < L
    std::vector<double> meas; // n x 3: Z
    std::vector<double> info; // n x 6, or 1 x 6 when one matrix serves all: upper triangle, row-major packed
    int rk = CUGO_RK_NONE;
    double delta = 1.0;
    bool rk_seen = false;
    int n() const { return (int)lm.size(); }
    void clear()
    {
        lm.clear(), meas.clear(), info.clear();
        rk = CUGO_RK_NONE, delta = 1.0, rk_seen = false;
    }
};

struct FlatGraph
{
    int Pall = 0, Lall = 0, P = 0, L = 0;
    std::vector<double> poses; // Pall x 7
    std::vector<double> lms;   // Lall x 3
    // active edges in ANY order (the engine sorts them landmark-major)
    std::vector<int32_t> e_pose, e_lm;
    std::vector<double> e_meas; // E x 3 (AoS on input)
    std::vector<double> e_omega; // E or 1
    std::vector<uint8_t> e_flags;
    std::vector<uint16_t> e_cam; // E or empty
    std::vector<double> cams;    // n_cams x 5
    // camera extrinsics (a rig; cugo_edges.has_rig / d_cam_ext): per camera-table entry the sensor pose body -> sensor
    // as {M row-major, t_s}, n_cams x 12 (or empty: all identity); has_rig iff one of them is not exactly identity
    std::vector<double> cam_ext;
    bool has_rig = false;
    // camera models (Kannala-Brandt; cugo_edges.has_rig == CUGO_RIG_MODELS): per camera-table entry (k1, k2, k3, k4,
    // type), n_cams x 5 (or empty: all pinhole); has_models iff one of them is not a pinhole.  The engine then hands the
    // kernels ONE table of stride 17 assembled from cam_ext (identities where that is empty) and this
    std::vector<double> cam_model;
    bool has_models = false;
    // radial-tangential distortion (cugo_edges.has_rig == CUGO_RIG_DISTORTION): per camera-table entry (k1, k2, p1, p2,
    // k3), n_cams x 5 (or empty: all zero); has_dist iff some entry's coefficients are not all zero.  The engine then
    // hands the kernels ONE table of stride 18 assembled from cam_ext (identities where that is empty), this and a flag
    // per entry.  Never together with has_models
    std::vector<double> cam_dist;
    bool has_dist = false;
    cugo_robust rk{CUGO_RK_NONE, 1.0, CUGO_RK_NONE, 1.0};
    // depth edge sets (flag bit CUGO_EDGE_DEPTH; cugo_edges.has_depth and the members behind it): whether the graph has
    // any, their robust kernel and their inverse-depth weight
    bool has_depth = false;
    int rk_type_depth = CUGO_RK_NONE;
    double rk_delta_depth = 1.0, depth_weight = 1.0;
    // outlier rejection (ref: EdgeSet::updateEdges, optimisable_graph.hpp:603-640): per edge
    // the chi2 threshold of its edge set, 0 = disabled; empty = disabled for all
    std::vector<double> e_outlier_threshold;
    FlatPoseKind kinds[POSE_KIND_COUNT]; // widths set by the constructor
    FlatLmPriors lm_priors;
    FlatGraph()
    {
        const int w[POSE_KIND_COUNT][2] = {{7, 1}, {9, 1}, {7, 21}, {7, 21}, {6, 6}, {6, 6}};
        for (int k = 0; k < POSE_KIND_COUNT; k++)
            kinds[k].kind = k, kinds[k].meas_w = w[k][0], kinds[k].weight_w = w[k][1];
    }
    int n_pose_edges() const // the unary kinds
    {
        return kinds[POSE_KIND_PLANE].n() + kinds[POSE_KIND_LINE].n() + kinds[POSE_KIND_PRIOR].n() + kinds[POSE_KIND_POINT].n();
    }
    int n_edges() const { return (int)e_pose.size(); }
};

struct IterRecord
{
    int iteration;
    double chi2, lambda, rho;
    int trials;
};

struct StructureStats
{
    double hsc_blocks = 0, products = 0, nnzL = 0, chol_flops = 0, supernodes = 0, stages = 0,
           front_bytes = 0, offdiag_products = 0, up_potrf_flops = 0, up_trsm_flops = 0,
           up_syrk_flops = 0, up_ea_bytes = 0, backward_bytes = 0, schur_slots = 0;
    // sharded run with rank-owned elimination subtrees: factorisation work of this rank's own subtrees / of the
    // replicated top (same unit as chol_flops' model), bytes this rank's factorisation exchanges per trial
    // (update blocks into the top + solution ranges), number of those broadcasts
    double chol_rank_flops = 0, chol_top_flops = 0, chol_bcast_bytes = 0, chol_bcasts = 0;
    double trial_sync_retries = 0; // waits for an LM trial that returned before its result was there (expected: 0)
    // sharded run: bytes of the Schur system [Hsc | bsc] this rank RECEIVES per LM trial — with rank-owned
    // subtrees only its own segment (reduce-scatter) and the top's part (all-reduce) — and what the full
    // all-reduce of the system would hand to it
    double xchg_sys_bytes = 0, xchg_sys_full_bytes = 0;
};

enum ProfItem
{
    PROF_INITIALIZE = 0,
    PROF_BUILD_STRUCTURE,
    PROF_COMPUTE_ERROR,
    PROF_BUILD_SYSTEM,
    PROF_SCHUR,
    PROF_SYMBOLIC,
    PROF_NUMERIC,
    PROF_UPDATE,
    PROF_COUNT
};

class Engine
{
public:
    // plan_only: no device is touched; initialize() stops after the host-side flattening and
    // builds the structure (Hsc pattern, product lists, ordering, symbolic factor) right away
    explicit Engine(bool plan_only = false);
    ~Engine();
    Engine(const Engine&) = delete;
    Engine& operator=(const Engine&) = delete;

    // the run-time switches of this optimiser (options.h): a snapshot of the environment taken when it was
    // created; cugo_graph_set_option changes single ones afterwards
    Options& options();
    void set_shard(int rank, int world, cugo_exchange_fn fn, void* user);
    // native exchange: RCCL communicator over the ranks of the job (shared by all optimisers of the
    // process); all-reduces then run on the solver's stream without a host synchronisation
    void set_comm(std::shared_ptr<RcclComm> comm);
    void exchange_stats(double& bytes, int& calls) const; // since the last initialize()
    // ref: BlockSolver::initialize (block_solver.cpp:21-137)
    // float storage of the Hpl / T block streams (GraphOptimisationOptions::useFloat32); takes
    // effect at the next initialize().  The environment variable CUGO_FLOAT32=1 forces it on.
    void set_float32_blocks(bool on);
    void initialize(FlatGraph& g);
    // same graph as at the last initialize(), new estimates (g.poses / g.lms): the flattened edge
    // arrays, the structure and the symbolic factor on the device stay as they are
    void refresh_estimates(const FlatGraph& g);
    // The same through PINNED host staging owned by the engine (7 doubles per pose / 3 per landmark, by index, as in
    // FlatGraph::poses / lms): the caller gathers the estimates straight into pinned_poses() / pinned_lms() and the
    // copy to the device is a DMA transfer this call does not wait for (from pageable memory the runtime stages the
    // copy synchronously: 0.13 ms of the 0.33 ms an estimates-only initialize() took on the kitti_00 shape).
    double* pinned_poses();
    double* pinned_lms();
    void refresh_estimates_pinned();
    // estimates back to the host, into the same pinned staging (single process; false on a landmark shard, whose
    // landmark estimates are summed over the ranks first: download() does that)
    bool download_pinned(const double** poses, const double** lms);
    // a FlatGraph owned by the engine whose buffers survive between initialize() calls
    FlatGraph& staging();
    // ref: optimize(); appends to records. verbose prints one line per iteration.
    void optimize(int niterations, std::vector<IterRecord>& records, bool verbose);
    // estimates back to host (ref: VertexSet::finalise, optimisable_graph.hpp:137-154)
    void download(std::vector<double>& poses, std::vector<double>& lms);
    // ref: BlockSolver::updateEdges at the end of optimize(): edges whose chi2 in the last error
    // pass exceeds their set's threshold become inactive.  Returns their indices in the order of
    // the FlatGraph passed to initialize() (all ranks return the same list).
    std::vector<int32_t> reject_outliers();
    // The same on the pose edge kinds that carry a threshold (FlatPoseKind::threshold), at the
    // same estimates: one error pass with the chi2 term of every edge and the outlier pass (cugo_pose_edges_reject) per
    // such kind, all on the device; the flags stay there, so a further optimize() on the same initialisation runs
    // without the edges.  Returns, per kind (PoseKind: the relative-pose edges last), the {edge set, position in the
    // set} of every edge that went, ascending.  The Hsc pattern is left as it is (a pair that lost its last edge keeps
    // an empty block until the next flattening), and n_*_edges() keep describing the flattening.
    using PoseOutliers = std::vector<std::pair<int32_t, int32_t>>;
    std::vector<PoseOutliers> reject_pose_outliers();
    // Extension: marginal covariances at the current estimates (include/cugo_hip.h, cugo_graph_compute_covariances).
    // Builds J^T Omega J at lambda = 0, its Schur complement and factorisation, runs the selected inverse and, for
    // what & 2, the landmark blocks; keeps the diagonal blocks (cov_pose [P][36], cov_lm [L][9], column-major) on the
    // host.  Returns false on a zero pivot or a landmark whose Hll is not positive definite.  Leaves the estimates
    // and everything the next optimize() reads as they were.
    bool compute_covariances(int what);
    // Extension: the blocks Sigma_ab of n pose pairs, given by free pose index (-1: a fixed pose, its blocks are zero),
    // into cov36 [n][36] (host, column-major, rows a).  The same build pass, Schur complement and factorisation, then
    // cugo_chol::inverse_blocks; the marginals kept by compute_covariances() are not touched.  false: a zero pivot.
    bool pose_cross_covariances(int n, const int32_t* ia, const int32_t* ib, double* cov36);
    // Extension: the pose-landmark blocks Sigma_al of n queries, given by free pose index and free landmark index (-1: a
    // fixed vertex, the block is zero), into cov18 [n][18] (host, 6x3 column-major, rows a).  One build pass, Schur
    // complement and factorisation, the plan of the batch (plcov_plan.h, from the engine's host copy of the slot
    // layout), cugo_chol::inverse_blocks for its pairs into a device buffer and k_pose_lm_cross; only the results
    // travel to the host.  The same contract as pose_cross_covariances.  false: a zero pivot, or the Hll of a queried
    // landmark is not positive definite.
    bool pose_landmark_cross_covariances(int n, const int32_t* ia, const int32_t* il, double* cov18);
    // Extension: S = J Sigma J^T of the reprojection of landmark il[k] in pose ia[k] (indices of the flattening, fixed
    // vertices included: >= n_poses_free() / n_landmarks_free()) into cov [n][dim * dim] (host, column-major), dim 2 or
    // 3, cam5 [n][5].  The above, plus the selected inverse and k_lm_covariance into a scratch buffer for Sigma_ll (its
    // own fail flag is ignored: a singular Hll counts only when a query names the landmark), then k_reprojection_cov.
    bool reprojection_covariances(int n, const int32_t* ia, const int32_t* il, int dim, const double* cam5, double* cov);
    // Extension: the predicted observation z [n][dim] and S [n][dim * dim] of the same queries for every camera kind
    // (k_predict_obs): kind CUGO_OBS_MONO / _STEREO / _DEPTH (dim 2 / 3 / 3), cam5 [n][5], cam_tab [n][17] = {M row-major,
    // t_s, k1..k4, model} or NULL (pinholes at the pose).  The path of reprojection_covariances; z is computed where both
    // vertices are fixed too.  false: both outputs zero-filled.
    bool predict_observations(int n, const int32_t* ia, const int32_t* il, int kind, const double* cam5,
                              const double* cam_tab, double* z, double* cov);
    void clear_covariances();
    int covariances_held() const { return cov_what_; } // bit 0 poses, bit 1 landmarks
    const std::vector<double>& cov_pose() const { return cov_pose_; }
    const std::vector<double>& cov_lm() const { return cov_lm_; }
    int n_poses_free() const;
    int n_landmarks_free() const;
    int n_active_edges() const { return E_global_; } // BA + ICP + point edges + priors (pose and landmark) + relative-pose and pose-pose point edges of the current flattening
    int n_icp_edges(int kind) const;                  // 0 plane, 1 line
    int n_prior_edges() const;
    int n_relpose_edges() const;
    int n_lm_prior_edges() const;
    int n_point_edges() const;
    // Diagnostic: the point edges of the current flattening as the kernels read them (sorted by pose, planar): pose [n],
    // the position of every edge in its set's container, p [3][n], z [3][n], info [6][n_info]; returns n_info (n or 1)
    int flat_point_edges(std::vector<int32_t>& pose, std::vector<int32_t>& src_edge, std::vector<double>& p,
                         std::vector<double>& z, std::vector<double>& info) const;
    int n_point_pair_edges() const;
    // whether the point / pose-pose point kind of the current flattening is in the covariance form: `info` of the two
    // diagnostics above is then [12][n_info], cov_p then cov_z
    bool point_edges_cov() const;
    bool point_pair_edges_cov() const;
    // Diagnostic: the pose-pose point edges of the current flattening as the kernels read them (the plan's sorted order,
    // planar): pose a / pose b [n], the position of every edge in its set's container, p [3][n], z [3][n], info
    // [6][n_info]; returns n_info (n or 1)
    int flat_point_pair_edges(std::vector<int32_t>& pose_a, std::vector<int32_t>& pose_b, std::vector<int32_t>& src_edge,
                              std::vector<double>& p, std::vector<double>& z, std::vector<double>& info) const;
    // sorted slot of a kind -> {edge set, position in the set} as FlatPoseKind recorded them (kept for a later
    // outlier rejection on these sets)
    const std::vector<int32_t>& icp_slot_source(int kind, bool set) const;
    const StructureStats& structure_stats() const { return sstats_; }
    const double* profile_ms() const { return prof_; }
    static const char* profile_name(int i);
    // per-kernel-group device times measured with HIP events on the engine's stream
    // (enabled by set_kernel_timing; adds event overhead, so not used inside timed runs)
    // mode 1: event pairs round every kernel group and every kernel (per-kernel figures; each pair adds a few us);
    // mode 2: one event per group boundary (group times that add up exactly to the device time of optimize()); 0: off
    void set_kernel_timing(int mode);
    struct KernelTime
    {
        std::string name;
        double ms;
        int launches;
    };
    std::vector<KernelTime> kernel_times() const;
    struct Impl;

private:
    void check_covariance_call(const char* who) const; // throws on plan-only, sharded and fp32-internal optimisers
    void queue_covariance_system();                    // build pass at lambda = 0, Schur complement, factorisation
    // queue_covariance_system(), the plan of the queries (qp, ql: free indices or -1), its pose blocks and
    // k_pose_lm_cross; `extra` rides behind the index arrays on the device.  off[6]: where q_pose, q_lm, q_ptr, q_slot,
    // q_aa and extra start in the index buffer.  false: a zero pivot
    bool queue_pose_lm_cross(int n, const int32_t* qp, const int32_t* ql, const std::vector<int32_t>& extra, size_t off[6]);
    // what reprojection_covariances() and predict_observations() share (engine.cpp)
    int queue_joint_covariances(const char* who, int n, const int32_t* ia, const int32_t* il, int third, size_t off[6]);
    bool fetch_joint_covariances(int n, bool flagged, std::vector<double>& h);
    void build_structure(); // by device_structure() or host_structure(); both end in adopt_structure()
    bool device_structure(InitLaps& laps);
    void host_structure(InitLaps& laps);
    void adopt_structure(const cugo_hsc_struct& hs, double products, double offdiag_products, double schur_slots);
    void fill_structure_stats(int B, double products, double offdiag_products);
    Impl* impl_;
    int E_global_ = 0;
    StructureStats sstats_;
    double prof_[PROF_COUNT] = {0};
    int cov_what_ = 0;
    std::vector<double> cov_pose_, cov_lm_;
};

} // namespace cugo_host
