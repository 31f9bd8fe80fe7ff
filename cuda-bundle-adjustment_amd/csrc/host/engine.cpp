// Engine implementation: flatten -> device, structure build, LM loop.
// ref: src/block_solver.cpp (step order), src/cuda_graph_optimisation.cpp:48-154 (LM control),
//      src/sparse_block_matrix.cpp:63-156 (Hsc pattern), src/optimisable_graph.hpp:642-661.
#include "engine.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>
#include <thread>

#include "../kernels/kernels.h"
#include "chol_solver.h"
#include "edge_layout.h"
#include "hip_util.h"
#include "options.h"
#include "rccl_comm.h"
#include "plcov_plan.h"
#include "point_pair_plan.h"
#include "relpose_plan.h"
#include "schur_plan.h"
#include "structure_gpu.h"
#include "thread_pool.h"

namespace cugo_host
{

namespace
{
inline void cpu_relax()
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield" ::: "memory");
#endif
}
thread_local std::string g_last_error;
using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
}
} // namespace

void set_last_error(const std::string& s) { g_last_error = s; }
const char* get_last_error() { return g_last_error.c_str(); }

// CUGO_INIT_TIMING=1: per-section host times of initialize() on stderr (diagnosis only)
struct InitLaps
{
    bool on;
    explicit InitLaps(bool enabled) : on(enabled) {}
    const Clock::time_point t0 = Clock::now(); // of the call
    Clock::time_point t = t0;
    void lap(const char* what)
    {
        if (!on)
            return;
        const auto n = Clock::now();
        std::fprintf(stderr, "[cugo init] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count());
        t = n;
    }
};

struct Engine::Impl : cugo_k::LaunchHook
{
    cugo_ctx ctx;
    cugo_chol chol;
    int rank = 0, world = 1;
    int init_rank = -1, init_world = -1; // what the last full initialize() was built for
    cugo_exchange_fn xfn = nullptr;
    void* xuser = nullptr;
    std::shared_ptr<RcclComm> comm; // native exchange (RCCL on the solver's stream); else xfn
    double xchg_bytes = 0;          // payload bytes all-reduced since initialize()
    int xchg_calls = 0;
    bool profile = false;
    bool plan_only = false; // host side only (no device): see Engine::Engine
    Options opt = Options::from_env(); // the environment switches, read once when the optimiser is created

    int Pall = 0, Lall = 0, P = 0, L = 0, E = 0;
    int shard_l0 = 0, shard_l1 = 0; // landmark index range owned by this rank
    cugo_robust rk{CUGO_RK_NONE, 1.0, CUGO_RK_NONE, 1.0};

    // host copies (sorted, local shard)
    std::vector<int32_t> h_lm_ptr, h_pose_ptr, h_pose_edge;
    // staging of initialize(), kept between calls: a fresh 40 MB of vectors costs more in page
    // faults than the work done on them
    FlatGraph staging;
    bool f32_blocks = false; // Hpl / T stored as float (fp32-internal mode)
    std::vector<int32_t> st_lm_cnt, st_order, st_slot_src;
    SlotArrays slots;             // the slot arrays (the measurement part is only staging for the upload)
    int last_err_buf = 0;         // estimate buffer of the last error pass
    bool lm_in_one_group = false; // no landmark's slots straddle two groups of kSlotGroup slots
    int Etot = 0;
    // global co-visibility: free landmark -> sorted free poses (free-free active edges, all shards)
    std::vector<int32_t> cov_ptr, cov_pose;
    // The distinct (lo, hi) pairs of free poses that a counting relative-pose or pose-pose point edge joins (the union of
    // the two kinds: a pair joined by both is one block every contributor adds into), ascending: each is a block of the
    // Hsc pattern whether or not the two poses share a landmark.  For the pattern alone a pair is a landmark seen by
    // exactly two poses: aug_* are the co-visibility lists with one such entry appended per pair (empty without pairs).
    // They feed the pattern builders only; products, contribution lists and sharding come from the real lists.
    std::vector<int32_t> pair_lo, pair_hi, aug_ptr, aug_pose;
    const std::vector<int32_t>& pat_ptr() const { return pair_lo.empty() ? cov_ptr : aug_ptr; }
    const std::vector<int32_t>& pat_pose() const { return pair_lo.empty() ? cov_pose : aug_pose; }
    int pat_lists() const { return L + (int)pair_lo.size(); }
    void build_pair_lists(const FlatPoseKind& fr, const FlatPoseKind& fp)
    {
        std::vector<std::pair<int32_t, int32_t>> pr;
        for (const FlatPoseKind* k : {&fr, &fp})
            for (int e = 0; e < k->n(); e++)
                if (k->pose[e] < P && k->pose_b[e] < P)
                    pr.emplace_back(std::min(k->pose[e], k->pose_b[e]), std::max(k->pose[e], k->pose_b[e]));
        std::sort(pr.begin(), pr.end());
        pr.erase(std::unique(pr.begin(), pr.end()), pr.end());
        pair_lo.clear(), pair_hi.clear(), aug_ptr.clear(), aug_pose.clear();
        if (pr.empty())
            return;
        aug_ptr = cov_ptr, aug_pose = cov_pose;
        for (const auto& q : pr)
        {
            pair_lo.push_back(q.first), pair_hi.push_back(q.second);
            aug_pose.push_back(q.first), aug_pose.push_back(q.second);
            aug_ptr.push_back((int32_t)aug_pose.size());
        }
    }
    // Hsc pattern (host)
    std::vector<int32_t> hsc_rowptr, hsc_colind;

    DevBuf<int32_t> d_e_pose, d_e_lm, d_lm_ptr, d_pose_ptr, d_pose_edge;
    DevBuf<int32_t> d_pose_rec; // [n][4] per entry of the pose-major list: slot, end of its landmark, landmark, flags (k_hsc_rows)
    DevBuf<unsigned long long> d_hash; // diagnosis (CUGO_DEBUG_HASH=file): per iteration 16 stage checksums
    uint64_t trial_seq = 0;        // sequence number of the last LM trial whose result the host waited for
    hipEvent_t trial_ev = nullptr; // end of a trial whose successor build is already queued (optimize)
    bool rows_on = false;       // the Schur complement by block rows (k_hsc_rows; CUGO_HSC_ROWS=0: the gather kernels)
    DevBuf<int32_t> d_pose_pos, d_off_pi; // row-strip form of the off-diagonal gather (k_hsc_offdiag_strip)
    bool strip_on = false;
    int max_row_nnz = 0;
    DevBuf<double> d_meas, d_omega, d_cams, d_cam_ext; // (d_cam_ext: FlatGraph::cam_ext, only with has_rig)
    std::vector<double> h_cam_tab;
    DevBuf<uint8_t> d_flags;
    DevBuf<uint16_t> d_cam;
    DevBuf<double> d_poses[2], d_lms[2];
    int cur = 0;
    DevBuf<double> d_Hpp, d_b, d_Hll, d_Hpl, d_T, d_invHll, d_x, d_sys, d_tmp, d_scal;
    // fused iteration (Options::pose_schur): {L^-1, L^-1 bl} of every landmark (Hll + lambda I = L L^T) in a 128-byte
    // slot for k_pose_schur / k_backsubst_landmarks (begin_call)
    DevBuf<double> d_lmrec;
    // marginal covariances (Engine::compute_covariances; allocated by the first call only): the blocks of Sigma on
    // the Hsc pattern, the landmark blocks, their positive-definiteness flag
    DevBuf<double> d_cov_sigma, d_cov_pose, d_cov_lm, d_xcov; // (d_xcov: Engine::pose_cross_covariances)
    DevBuf<int32_t> d_cov_fail; // [0] k_lm_covariance, [1] k_pose_lm_cross
    // pose-landmark queries (Engine::queue_pose_lm_cross): the index arrays of a batch behind one another, the pose
    // blocks of its plan, Sigma_al, the cameras and the result of k_reprojection_cov
    std::vector<int32_t> h_pl_idx;
    DevBuf<int32_t> d_pl_idx;
    DevBuf<double> d_pl_blocks, d_pl_cross, d_pl_cam, d_pl_out, d_pl_tab, d_pl_z; // (tab, z: k_predict_obs)
    PinnedBuf<double> h_pin_poses, h_pin_lms; // refresh_estimates_pinned / download_pinned
    Clock::duration last_trial_wait{0};       // how long the host polled for the previous trial's result
    DevBuf<int32_t> d_hsc_rowptr, d_hsc_colind, d_off_ptr, d_off_ei, d_off_ej, d_fail;
    PinnedBuf<double> h_scal;
    PinnedBuf<int32_t> h_fail;

    cugo_edges ev{};
    // The pose edge kinds (FlatGraph::kinds): point-to-plane / point-to-line (icp_kernels.hip), SE(3) priors
    // (prior_kernels.hip) and relative-pose edges (relpose_kernels.hip).  Each kind planar (structure of arrays) on the
    // device as long as the flattening lives — the unary kinds sorted by pose (stable: container order inside a pose),
    // the relative-pose edges in container order with a plan (relpose_plan.h) against the Hsc pattern in place of a
    // sort; the views the kernels take; and a scratch of their own (the BA scratch holds live scale / chi2 partials and
    // records across the same span of the stream):
    //     [pair partials | point partials | ICP partials | ICP chunk chi2 totals | point chunk chi2 totals | prior workgroup
    //      chi2 totals | relative-pose workgroup chi2 totals | landmark-prior workgroup chi2 totals | pair chunk chi2 totals |
    //      16 doubles of slack]
    // (the point-to-point edges, point_kernels.hip, are a fifth kind on the machinery of the ICP kinds, the pose-pose
    // point edges, point_pair_kernels.hip, a sixth with a plan of their own (point_pair_plan.h); without a kind its runs
    // are empty and the layout is what it was)
    // The landmark position priors (FlatGraph::lm_priors, lm_prior_kernels.hip) sit on landmarks, not poses, but their
    // chi2 travels the same way, so they live here too: sorted by landmark (stable) with a CSR over all landmarks,
    // planar on the device.  Their terms ride in the BA build pass (launch_build with the view); only the chi2 has
    // launches of its own.
    // The runs of totals are adjacent, so that the launch ending a trial sums them as one array (chi_totals).  Every
    // launch of a kind sits under its count of totals: a graph without the kind queues what it always did.
    struct PoseEdges
    {
        struct KindBufs : PoseKindHost
        {
            DevBuf<int32_t> d_pose, d_pose_b, d_ptr;
            DevBuf<double> d_meas, d_weight;
        } kind[POSE_KIND_COUNT];
        cugo_icp_edges icp{};
        cugo_prior_edges prior{};
        cugo_relpose_edges relpose{};
        cugo_point_edges point{};
        cugo_point_pair_edges pair{}; // (its plan member stays null: the launchers take the device plan)
        int n_icp = 0, n_prior = 0, n_relpose = 0, n_point = 0, n_pair = 0;
        // totals an ICP pass / a point pass / a prior pass / a relative-pose pass / a pair pass leaves (0: the pass is not launched)
        int n_icp_chi = 0, n_point_chi = 0, n_prior_wg = 0, n_relpose_wg = 0, n_pair_chi = 0;
        DevBuf<double> d_scratch;
        // the layout above, set by bind()
        size_t off_point = 0, off_icp = 0, off_icp_chi = 0, off_point_chi = 0, off_prior_chi = 0, off_relpose_chi = 0,
               off_lm_prior_chi = 0, off_pair_chi = 0;
        // landmark position priors: sorted host copies (h_lmp_lm, h_lmp_ptr: what initialize() checks against the slot
        // layout), the device arrays, the view
        std::vector<int32_t> h_lmp_lm, h_lmp_ptr;
        DevBuf<int32_t> d_lmp_lm, d_lmp_ptr;
        DevBuf<double> d_lmp_meas, d_lmp_info;
        cugo_lm_prior_edges lm_prior{};
        int n_lm_prior = 0, n_lm_prior_wg = 0;
        double* lm_prior_chi() { return d_scratch.data() + off_lm_prior_chi; }
        // the view for the build pass; nullptr without priors (the pass is then queued as it always was)
        const cugo_lm_prior_edges* lm_prior_view() const { return n_lm_prior_wg ? &lm_prior : nullptr; }
        void bind_lm_priors(const FlatLmPriors& f, int Lall, int L, hipStream_t stream, bool plan_only)
        {
            const int n = n_lm_prior = f.n();
            lm_prior = cugo_lm_prior_edges{};
            lm_prior.n_landmarks_total = Lall, lm_prior.n_landmarks_free = L, lm_prior.n = n;
            lm_prior.rk = f.rk, lm_prior.delta = f.delta;
            h_lmp_lm.clear(), h_lmp_ptr.clear();
            n_lm_prior_wg = 0;
            if (!n)
                return;
            if (n > (1 << 26))
                throw std::runtime_error("cugo: more than 2^26 landmark prior edges");
            // counting sort by landmark: stable, container order inside a landmark
            h_lmp_ptr.assign((size_t)Lall + 1, 0);
            for (int e = 0; e < n; e++)
                h_lmp_ptr[(size_t)f.lm[e] + 1]++;
            for (int l = 0; l < Lall; l++)
                h_lmp_ptr[l + 1] += h_lmp_ptr[l];
            std::vector<int32_t> at(h_lmp_ptr.begin(), h_lmp_ptr.end() - 1);
            const int n_info = f.info.size() == 6 ? 1 : n;
            std::vector<double> meas(3 * (size_t)n), info(6 * (size_t)n_info);
            h_lmp_lm.resize((size_t)n);
            for (int e = 0; e < n; e++)
            {
                const int q = at[f.lm[e]]++;
                h_lmp_lm[q] = f.lm[e];
                for (int c = 0; c < 3; c++)
                    meas[(size_t)c * n + q] = f.meas[3 * (size_t)e + c];
                if (n_info > 1)
                    for (int c = 0; c < 6; c++)
                        info[(size_t)c * n + q] = f.info[6 * (size_t)e + c];
            }
            if (n_info == 1)
                info = f.info;
            lm_prior.n_info = n_info;
            n_lm_prior_wg = cugo_k::lm_prior_workgroups(lm_prior);
            if (plan_only)
                return;
            d_lmp_lm.upload(h_lmp_lm, stream), d_lmp_ptr.upload(h_lmp_ptr, stream);
            d_lmp_meas.upload(meas, stream), d_lmp_info.upload(info, stream);
            CUGO_HIP(hipStreamSynchronize(stream)); // (meas / info are locals)
            lm_prior.d_lm = d_lmp_lm.data(), lm_prior.d_lm_ptr = d_lmp_ptr.data();
            lm_prior.d_meas = d_lmp_meas.data(), lm_prior.d_info = d_lmp_info.data();
        }
        struct RelPosePlan
        {
            DevBuf<int32_t> d_inc_ptr, d_inc, d_off_blk;
            RelPosePlanHost plan;
            bool plan_dirty = true; // the plans (this one and the pair kind's) are not those of the edges and the Hsc pattern at hand
            cugo_k::RelPosePlanDev dev{};
        } rp;
        // the plan of the pose-pose point edges (point_pair_plan.h): bind() sorts the edges by it (no pattern is needed
        // for the sort), bind_relpose_plan() rebuilds it against the Hsc pattern for the block indices
        struct PairPlan
        {
            DevBuf<int32_t> d_edge_run, d_run_ptr, d_run_a, d_run_b, d_run_flags, d_inc_ptr, d_inc, d_blk_id, d_blk_ptr, d_blk_run;
            PointPairPlanHost plan;
            cugo_k::PointPairPlanDev dev{};
        } pp;
        // Outlier rejection (Engine::reject_pose_outliers), per kind and only for a kind in which some threshold is
        // positive: the run-time flags the kind's view points at (all zero until edges go), a host copy of them, and the
        // thresholds in the order of the edges on the device (n or 1).  Every other kind keeps a NULL flag pointer in its
        // view and queues what it always queued.
        struct Reject
        {
            DevBuf<uint8_t> d_flags;
            std::vector<uint8_t> h_flags;
            DevBuf<double> d_threshold;
            int n_threshold = 0; // 0: the kind has no threshold
            bool on() const { return n_threshold > 0; }
        } rej[POSE_KIND_COUNT];
        DevBuf<double> d_rej_chi;              // the chi2 term of every edge of the kind(s) at hand
        DevBuf<int32_t> d_rej_list, d_rej_work; // the outlier pass's list and its workgroup counts
        bool any_reject() const
        {
            bool any = false;
            for (const Reject& r : rej)
                any = any || r.on();
            return any;
        }
        // flags and thresholds of kind k over its edges: nullptr (and nothing allocated) without a positive threshold
        const uint8_t* bind_reject(int k, hipStream_t stream, bool plan_only)
        {
            const int n = n_edges(k);
            const std::vector<double>& threshold = kind[k].h_threshold;
            Reject& r = rej[k];
            r.n_threshold = 0;
            r.h_flags.clear();
            if (!n || threshold.empty())
                return nullptr;
            r.n_threshold = (int)threshold.size();
            r.h_flags.assign((size_t)n, 0);
            if (plan_only)
                return nullptr;
            r.d_flags.resize((size_t)n), r.d_flags.zero(stream);
            r.d_threshold.upload(threshold, stream);
            return r.d_flags.data();
        }
        double* relpose_chi() { return d_scratch.data() + off_relpose_chi; }
        // the covariance form of the two point kinds (FlatPoseKind::cov): the weight buffer is [12][n_weight], the views'
        // d_info is cov_p and cov_z follows it; nullptr picks the information form's kernels
        bool point_cov = false, pair_cov = false;
        const double* point_cov_z() const { return point_cov ? point.d_info + 6 * (size_t)point.n_info : nullptr; }
        const double* pair_cov_z() const { return pair_cov ? pair.d_info + 6 * (size_t)pair.n_info : nullptr; }

        cugo_k::ChunkScratch icp_rs() { return cugo_k::icp_scratch_in({d_scratch.data() + off_icp, d_scratch.size() - off_icp}, icp); }
        cugo_k::ChunkScratch point_rs() { return {d_scratch.data() + off_point, d_scratch.data() + off_point_chi}; }
        cugo_k::ChunkScratch pair_rs() { return {d_scratch.data(), d_scratch.data() + off_pair_chi}; }
        double* prior_chi() { return d_scratch.data() + off_prior_chi; }
        int n_edges(int k) const { return (int)kind[k].h_pose.size(); }
        const std::vector<int32_t>& icp_slot_source(int k, bool set) const { return set ? kind[k].slot_set : kind[k].slot_edge; }
        // the chi2 totals of the last ICP, point, prior and relative-pose pass, one array; nullptr / 0 without such edges
        const double* chi_totals(int* n)
        {
            *n = n_icp_chi + n_point_chi + n_prior_wg + n_relpose_wg + n_lm_prior_wg + n_pair_chi;
            return *n ? d_scratch.data() + off_icp_chi : nullptr;
        }

        // planar copies (the unary kinds: sorted), upload by the calling thread (plan_only: no device), views and scratch
        // layout.  The relative-pose plan waits for the Hsc pattern (bind_relpose_plan)
        void bind(const FlatGraph& g, int Pall, int P, int Lall, int L, hipStream_t stream, bool plan_only)
        {
            bind_lm_priors(g.lm_priors, Lall, L, stream, plan_only);
            n_icp = g.kinds[POSE_KIND_PLANE].n() + g.kinds[POSE_KIND_LINE].n();
            n_prior = g.kinds[POSE_KIND_PRIOR].n(), n_relpose = g.kinds[POSE_KIND_RELPOSE].n();
            n_point = g.kinds[POSE_KIND_POINT].n(), n_pair = g.kinds[POSE_KIND_PAIR].n();
            for (int k = 0; k < POSE_KIND_COUNT; k++)
            {
                KindBufs& b = kind[k];
                const bool binary = k == POSE_KIND_RELPOSE || k == POSE_KIND_PAIR, is_icp = k == POSE_KIND_PLANE || k == POSE_KIND_LINE;
                if (!binary)
                    sort_pose_edges_by_pose(g.kinds[k], Pall, P, b);
                else if (g.kinds[k].n() > (1 << 26))
                    throw std::runtime_error(std::string("cugo: more than 2^26 ") + pose_kind_name(k) + " edges");
                else if (k == POSE_KIND_PAIR)
                    sort_pose_edges_by_pair(g.kinds[k], Pall, P, pp.plan, b);
                else
                    copy_pose_edges_planar(g.kinds[k], nullptr, b);
                // an empty kind uploads nothing, except that k_icp_finish reads the pose_ptr of BOTH ICP kinds whenever
                // either has edges: the empty one's is all zeros
                if (plan_only || !(g.kinds[k].n() || (is_icp && n_icp)))
                    continue;
                b.d_pose.upload(b.h_pose, stream);
                binary ? b.d_pose_b.upload(b.h_pose_b, stream) : b.d_ptr.upload(b.h_ptr, stream);
                b.d_meas.upload(b.h_meas, stream), b.d_weight.upload(b.h_weight, stream);
            }
            const KindBufs &pl = kind[POSE_KIND_PLANE], &li = kind[POSE_KIND_LINE], &pr = kind[POSE_KIND_PRIOR],
                           &rl = kind[POSE_KIND_RELPOSE];
            icp = cugo_icp_edges{};
            icp.n_poses_total = Pall, icp.n_poses_free = P;
            icp.n_plane = n_edges(POSE_KIND_PLANE), icp.n_line = n_edges(POSE_KIND_LINE);
            // (meas is planar: p [3][n], then n, d [4][n] or a, u [6][n])
            icp.d_plane_pose = pl.d_pose.data(), icp.d_plane_pose_ptr = pl.d_ptr.data();
            icp.d_plane_p = pl.d_meas.data(), icp.d_plane_nd = pl.d_meas.data() + 3 * (size_t)icp.n_plane;
            icp.d_plane_omega = pl.d_weight.data(), icp.n_plane_omega = pl.n_weight;
            icp.rk_plane = g.kinds[POSE_KIND_PLANE].rk, icp.delta_plane = g.kinds[POSE_KIND_PLANE].delta;
            icp.d_line_pose = li.d_pose.data(), icp.d_line_pose_ptr = li.d_ptr.data();
            icp.d_line_p = li.d_meas.data(), icp.d_line_au = li.d_meas.data() + 3 * (size_t)icp.n_line;
            icp.d_line_omega = li.d_weight.data(), icp.n_line_omega = li.n_weight;
            icp.rk_line = g.kinds[POSE_KIND_LINE].rk, icp.delta_line = g.kinds[POSE_KIND_LINE].delta;
            icp.d_plane_flags = bind_reject(POSE_KIND_PLANE, stream, plan_only);
            icp.d_line_flags = bind_reject(POSE_KIND_LINE, stream, plan_only);
            prior = cugo_prior_edges{};
            prior.n_poses_total = Pall, prior.n_poses_free = P, prior.n = n_prior;
            prior.d_pose = pr.d_pose.data(), prior.d_pose_ptr = pr.d_ptr.data();
            prior.d_meas = pr.d_meas.data(), prior.d_info = pr.d_weight.data(), prior.n_info = pr.n_weight;
            prior.rk = g.kinds[POSE_KIND_PRIOR].rk, prior.delta = g.kinds[POSE_KIND_PRIOR].delta;
            prior.d_flags = bind_reject(POSE_KIND_PRIOR, stream, plan_only);
            relpose = cugo_relpose_edges{};
            relpose.n_poses_total = Pall, relpose.n_poses_free = P, relpose.n = n_relpose;
            relpose.d_meas = rl.d_meas.data(), relpose.d_info = rl.d_weight.data(), relpose.n_info = rl.n_weight;
            relpose.rk = g.kinds[POSE_KIND_RELPOSE].rk, relpose.delta = g.kinds[POSE_KIND_RELPOSE].delta;
            // (run-time flags: the plan is still built with none, and an edge flagged here "counts for nothing")
            relpose.d_flags = bind_reject(POSE_KIND_RELPOSE, stream, plan_only);
            rp.plan_dirty = true;
            const KindBufs& pt = kind[POSE_KIND_POINT];
            point = cugo_point_edges{};
            point.n_poses_total = Pall, point.n_poses_free = P, point.n = n_point;
            point.d_pose = pt.d_pose.data(), point.d_pose_ptr = pt.d_ptr.data();
            // (meas is planar: p [3][n], then z [3][n])
            point.d_p = pt.d_meas.data(), point.d_z = pt.d_meas.data() + 3 * (size_t)n_point;
            point.d_info = pt.d_weight.data(), point.n_info = pt.n_weight;
            point.rk = g.kinds[POSE_KIND_POINT].rk, point.delta = g.kinds[POSE_KIND_POINT].delta;
            point_cov = g.kinds[POSE_KIND_POINT].cov, pair_cov = g.kinds[POSE_KIND_PAIR].cov;
            bind_reject(POSE_KIND_POINT, stream, plan_only); // (never on: graph_optimisation.cpp refuses a threshold on the kind)
            const KindBufs& pa = kind[POSE_KIND_PAIR];
            pair = cugo_point_pair_edges{};
            pair.n_poses_total = Pall, pair.n_poses_free = P, pair.n = n_pair;
            pair.d_pose_a = pa.d_pose.data(), pair.d_pose_b = pa.d_pose_b.data();
            pair.d_p = pa.d_meas.data(), pair.d_z = pa.d_meas.data() + 3 * (size_t)n_pair; // (planar: p [3][n], then z [3][n])
            pair.d_info = pa.d_weight.data(), pair.n_info = pa.n_weight;
            pair.rk = g.kinds[POSE_KIND_PAIR].rk, pair.delta = g.kinds[POSE_KIND_PAIR].delta;
            bind_reject(POSE_KIND_PAIR, stream, plan_only); // (never on, as for the point kind)
            // the scratch layout (the pair partials lead; the chunk totals end the ICP part; the point totals follow them)
            const int n_pair_runs = (int)pp.plan.run_a.size();
            off_point = n_pair ? cugo_k::point_pair_partial_doubles(n_pair, n_pair_runs) : 0;
            n_pair_chi = n_pair ? cugo_k::point_pair_chunk_count(n_pair) : 0;
            off_icp = off_point + (n_point ? cugo_k::point_partial_doubles(point) : 0);
            n_point_chi = n_point ? cugo_k::point_chunk_count(point) : 0;
            const size_t icp_doubles = n_icp ? cugo_k::icp_scratch_doubles(icp) : 0;
            n_icp_chi = n_icp ? cugo_k::icp_chunk_count(icp) : 0;
            n_prior_wg = cugo_k::prior_workgroups(prior), n_relpose_wg = cugo_k::relpose_workgroups(relpose);
            off_icp_chi = off_icp + icp_doubles - n_icp_chi, off_point_chi = off_icp + icp_doubles;
            off_prior_chi = off_point_chi + (size_t)n_point_chi;
            off_relpose_chi = off_prior_chi + (size_t)n_prior_wg;
            off_lm_prior_chi = off_relpose_chi + (size_t)n_relpose_wg;
            off_pair_chi = off_lm_prior_chi + (size_t)n_lm_prior_wg;
            if ((n_icp || n_point || n_prior_wg || n_relpose_wg || n_lm_prior_wg || n_pair) && !plan_only)
                d_scratch.resize(off_pair_chi + (size_t)n_pair_chi + 16);
        }
        // the plan against the Hsc pattern at hand (upper block CSR over the free poses): the engine made the pattern
        // from these very pairs, so a pair missing from it is a defect of the engine and throws
        void bind_relpose_plan(const std::vector<int32_t>& rowptr, const std::vector<int32_t>& colind, hipStream_t stream,
                               bool plan_only)
        {
            if (!rp.plan_dirty)
                return;
            rp.plan_dirty = false;
            if (n_pair)
            { // (the edges are in the plan's order already: the sort of sorted edges is the identity)
                KindBufs& pa = kind[POSE_KIND_PAIR];
                build_point_pair_plan(n_pair, pair.n_poses_total, pair.n_poses_free, pa.h_pose.data(), pa.h_pose_b.data(), nullptr,
                                      rowptr.data(), colind.data(), pp.plan);
                if (!plan_only)
                {
                    const PointPairPlanHost& h = pp.plan;
                    pp.d_edge_run.upload(h.edge_run, stream), pp.d_run_ptr.upload(h.run_ptr, stream);
                    pp.d_run_a.upload(h.run_a, stream), pp.d_run_b.upload(h.run_b, stream), pp.d_run_flags.upload(h.run_flags, stream);
                    pp.d_inc_ptr.upload(h.inc_ptr, stream), pp.d_inc.upload(h.inc, stream);
                    pp.d_blk_id.upload(h.blk_id, stream), pp.d_blk_ptr.upload(h.blk_ptr, stream), pp.d_blk_run.upload(h.blk_run, stream);
                    CUGO_HIP(hipStreamSynchronize(stream));
                    pp.dev = cugo_k::PointPairPlanDev{n_pair,
                                                      (int)h.run_a.size(),
                                                      pair.n_poses_free,
                                                      (int)h.blk_id.size(),
                                                      pp.d_edge_run.data(),
                                                      pp.d_run_ptr.data(),
                                                      pp.d_run_a.data(),
                                                      pp.d_run_b.data(),
                                                      pp.d_run_flags.data(),
                                                      pp.d_inc_ptr.data(),
                                                      pp.d_inc.data(),
                                                      pp.d_blk_id.data(),
                                                      pp.d_blk_ptr.data(),
                                                      pp.d_blk_run.data()};
                }
            }
            if (!n_relpose)
                return;
            KindBufs& rl = kind[POSE_KIND_RELPOSE];
            build_relpose_plan(n_relpose, relpose.n_poses_total, relpose.n_poses_free, rl.h_pose.data(), rl.h_pose_b.data(),
                               nullptr, rowptr.data(), colind.data(), rp.plan);
            if (plan_only)
                return;
            rp.d_inc_ptr.upload(rp.plan.inc_ptr, stream), rp.d_inc.upload(rp.plan.inc, stream);
            rp.d_off_blk.upload(rp.plan.off_blk, stream);
            CUGO_HIP(hipStreamSynchronize(stream));
            rp.dev = cugo_k::RelPosePlanDev{n_relpose, relpose.n_poses_free, rl.d_pose.data(), rl.d_pose_b.data(),
                                            rp.d_inc_ptr.data(), rp.d_inc.data(), rp.d_off_blk.data()};
        }
        // The pose edge terms of a build pass at `poses`.  Two-stream form: the ICP chunk pass and its add, then the
        // priors' ONE launch (terms and workgroup totals), both behind k_build_poses.  One-stream form (Hpp is not
        // written): the adds go behind k_pose_schur (queue_add_schur); the chunk pass still runs here, and the priors'
        // totals are computed here only where a chi2 is asked for (want_totals: iteration 0, or a trial that takes its
        // chi2 from this pass).  d_chi (once per call, iteration 0): the totals ADDED to it, ICP first
        // The landmark priors' terms are in the BA build pass itself; their chi2 (at `lms`) has a launch here only where
        // a chi2 is asked for (want_totals)
        void queue_build(hipStream_t s, const double* poses, const double* lms, bool one_stream, double* Hpp, double* bp,
                         bool want_totals, double* d_chi)
        {
            if (n_icp)
            {
                cugo_k::launch_icp_chunks(s, icp, poses, true, icp_rs());
                if (!one_stream)
                    cugo_k::launch_icp_add(s, icp, icp_rs(), Hpp, bp);
                if (d_chi)
                    cugo_k::launch_icp_chi_total(s, icp, icp_rs(), d_chi, true);
            }
            if (n_point)
            { // as the ICP kinds: the chunk pass, its add here or behind k_pose_schur
                cugo_k::launch_point_chunks(s, point, poses, true, point_rs(), nullptr, point_cov_z());
                if (!one_stream)
                    cugo_k::launch_point_add(s, point, point_rs(), Hpp, bp);
                if (d_chi)
                    cugo_k::launch_point_chi_total(s, point, point_rs(), d_chi, true);
            }
            if (n_pair)
            { // the chunk pass of the four roles; the diagonal sums here or, with the off-diagonal ones, behind the Schur pass
                cugo_k::launch_point_pair_chunks(s, pair, pp.dev, poses, true, pair_rs(), nullptr, pair_cov_z());
                if (!one_stream)
                    cugo_k::launch_point_pair_add_diag(s, pair, pp.dev, pair_rs(), Hpp, bp);
                if (d_chi)
                    cugo_k::launch_point_pair_chi_total(s, pair, pair_rs(), d_chi, true);
            }
            if (n_prior_wg)
            {
                if (!one_stream)
                    cugo_k::launch_prior_add(s, prior, poses, Hpp, bp, prior_chi());
                else if (want_totals)
                    cugo_k::launch_prior_errors(s, prior, poses, prior_chi());
                if (d_chi)
                    cugo_k::launch_pose_chi_total(s, "k_prior_chi_total", prior_chi(), n_prior_wg, d_chi, true);
            }
            if (n_relpose_wg)
            { // as the priors: ONE launch; the off-diagonal terms wait for the Schur pass (queue_offdiag_schur)
                if (!one_stream)
                    cugo_k::launch_relpose_add(s, relpose, rp.dev, poses, Hpp, bp, nullptr, relpose_chi());
                else if (want_totals)
                    cugo_k::launch_relpose_errors(s, relpose, rp.dev, poses, relpose_chi());
                if (d_chi)
                    cugo_k::launch_pose_chi_total(s, "k_relpose_chi_total", relpose_chi(), n_relpose_wg, d_chi, true);
            }
            if (n_lm_prior_wg && want_totals)
            {
                cugo_k::launch_lm_prior_errors(s, lm_prior, lms, lm_prior_chi());
                if (d_chi)
                    cugo_k::launch_pose_chi_total(s, "k_lm_prior_chi_total", lm_prior_chi(), n_lm_prior_wg, d_chi, true);
            }
        }
        // two-stream form: the off-diagonal terms of the relative-pose edges ADDED to their blocks of Hsc behind a Schur
        // pass (which wrote every block), at the poses the build pass at hand linearised at
        void queue_offdiag_schur(hipStream_t s, const double* poses, double* Hsc)
        {
            if (n_relpose_wg)
                cugo_k::launch_relpose_add_offdiag(s, relpose, rp.dev, poses, Hsc);
            // (the pair kind adds the sums of the PARTIALS of the build pass at hand: queue_build wrote them with the H the
            //  Schur pass has just consumed, and no error pass writes them)
            if (n_pair)
                cugo_k::launch_point_pair_add_offdiag(s, pair, pp.dev, pair_rs(), Hsc);
        }
        // one-stream form: the terms added to the diagonal blocks of Hsc, to bp and to bsc behind k_pose_schur (the
        // totals the prior launch leaves are those of the estimates at `poses` once more)
        void queue_add_schur(hipStream_t s, const double* poses, const int32_t* rowptr, double* Hsc, double* bp, double* bsc)
        {
            if (n_icp)
                cugo_k::launch_icp_add_schur(s, icp, icp_rs(), rowptr, Hsc, bp, bsc);
            if (n_point)
                cugo_k::launch_point_add_schur(s, point, point_rs(), rowptr, Hsc, bp, bsc);
            if (n_prior_wg)
                cugo_k::launch_prior_add_schur(s, prior, poses, rowptr, Hsc, bp, bsc, prior_chi());
            if (n_relpose_wg)
                cugo_k::launch_relpose_add_schur(s, relpose, rp.dev, poses, rowptr, Hsc, bp, bsc, relpose_chi());
            if (n_pair)
                cugo_k::launch_point_pair_add_schur(s, pair, pp.dev, pair_rs(), rowptr, Hsc, bp, bsc);
        }
        // error pass: chi_totals() at `poses` / `lms`
        void queue_errors(hipStream_t s, const double* poses, const double* lms)
        {
            if (n_icp)
                cugo_k::launch_icp_chunks(s, icp, poses, false, icp_rs());
            if (n_point)
                cugo_k::launch_point_chunks(s, point, poses, false, point_rs(), nullptr, point_cov_z());
            if (n_prior_wg)
                cugo_k::launch_prior_errors(s, prior, poses, prior_chi());
            if (n_relpose_wg)
                cugo_k::launch_relpose_errors(s, relpose, rp.dev, poses, relpose_chi());
            if (n_lm_prior_wg)
                cugo_k::launch_lm_prior_errors(s, lm_prior, lms, lm_prior_chi());
            if (n_pair)
                cugo_k::launch_point_pair_chunks(s, pair, pp.dev, poses, false, pair_rs(), nullptr, pair_cov_z());
        }
    } pe;
    cugo_hsc_struct hs{};
    SchurPlanDevice splan; // landmark-major product plan of the Schur complement (schur_plan.h)
    bool splan_on = false;
    GpuStructure gstruct;  // Hsc pattern + contribution lists built on the device (structure_gpu.h)
    bool structure_dirty = true;
    bool sig_valid = false; // sig_* hold the topology the structure at hand was built from
    // ... and the topology itself (compared on a hash hit), saved by build_structure()
    int sig_dims[8] = {0}, pending_dims[8] = {0};
    std::vector<int32_t> sig_e_pose, sig_e_lm, sig_cov_pose, sig_pair_lo, sig_pair_hi;
    // The Hsc pattern, the ordering and the symbolic factor depend on the co-visibility lists alone.  When
    // those change, initialize() starts their build on a helper thread and a second stream the moment the
    // lists exist — the slot layout, the slot arrays, their upload and the topology hash then run beside
    // it — and build_structure() (first optimize()) joins it, builds the contribution lists and uploads
    // the plan.  CUGO_ASYNC_STRUCTURE=0: everything in build_structure(), as before.
    std::thread pat_thread;
    std::exception_ptr pat_err;
    bool pat_async_ok = false;   // the helper finished a pattern + host plan for the current lists
    bool pattern_dirty = true;   // the pattern / plan in gstruct / chol are not those of the current lists
    bool plan_uploaded = false;
    // the helper's progress, for the caller of initialize(): 1 = the pattern is in gstruct (the contribution lists
    // can be built as soon as the slots are on the device), -1 = it was not built; and whether the lists of the
    // structure at hand were already built at the end of initialize()
    std::atomic<int> pat_stage{0};
    bool lists_built = false;
    int pat_P = -1, pat_L = -1;
    std::vector<int32_t> pat_cov_ptr, pat_cov_pose; // the lists the pattern in gstruct / chol was built from
    hipStream_t s2 = nullptr;
    void join_pattern()
    {
        if (pat_thread.joinable())
            pat_thread.join();
    }
    // the stages of Engine::initialize() that work on the device side (defined beside it)
    struct SlotUpload;
    bool start_pattern_helper(double* prof);
    std::vector<uint8_t> sig_flags;

    // optional HIP-event timing: 1 = an event pair round every kernel group AND every kernel (each pair adds a few
    // microseconds to what it brackets: per-kernel figures, never sums), 2 = ONE event at every group boundary —
    // the group times then add up exactly to the device time between the first and the last event of optimize()
    int ktiming = 0;
    struct Mark
    {
        int label;
        hipEvent_t e;
    };
    std::vector<Mark> marks; // (mode 2)
    void mark(int label)
    {
        Mark mk{label, nullptr};
        CUGO_HIP(hipEventCreate(&mk.e));
        CUGO_HIP(hipEventRecord(mk.e, ctx.stream));
        marks.push_back(mk);
    }
    struct KEv
    {
        int label;
        hipEvent_t a, b;
    };
    std::vector<KEv> kev;
    std::vector<std::string> klabels;
    std::vector<double> kms;
    std::vector<int> kcount;
    int klabel(const char* name)
    {
        for (size_t i = 0; i < klabels.size(); i++)
            if (klabels[i] == name)
                return (int)i;
        klabels.push_back(name);
        kms.push_back(0);
        kcount.push_back(0);
        return (int)klabels.size() - 1;
    }
    template <typename F>
    void timed(const char* name, F&& f)
    {
        if (!ktiming)
        {
            f();
            return;
        }
        if (ktiming == 2)
        {
            mark(klabel(name));
            f();
            return;
        }
        KEv e;
        e.label = klabel(name);
        CUGO_HIP(hipEventCreate(&e.a));
        CUGO_HIP(hipEventCreate(&e.b));
        CUGO_HIP(hipEventRecord(e.a, ctx.stream));
        f();
        CUGO_HIP(hipEventRecord(e.b, ctx.stream));
        kev.push_back(e);
    }
    // per-kernel events (LaunchHook): nested inside the group scopes above
    std::vector<KEv> kev_open;
    void begin(const char* kernel, hipStream_t st) override
    {
        KEv e;
        e.label = klabel(kernel);
        CUGO_HIP(hipEventCreate(&e.a));
        CUGO_HIP(hipEventCreate(&e.b));
        CUGO_HIP(hipEventRecord(e.a, st));
        kev_open.push_back(e);
    }
    void end(const char*, hipStream_t st) override
    {
        KEv e = kev_open.back();
        kev_open.pop_back();
        CUGO_HIP(hipEventRecord(e.b, st));
        kev.push_back(e);
    }
    void collect_times()
    {
        if (!marks.empty())
        { // mode 2: the time from a group's mark to the next mark belongs to the group
            mark(-1);
            CUGO_HIP(hipStreamSynchronize(ctx.stream));
            for (size_t i = 0; i + 1 < marks.size(); i++)
            {
                float ms = 0;
                CUGO_HIP(hipEventElapsedTime(&ms, marks[i].e, marks[i + 1].e));
                kms[marks[i].label] += ms;
                kcount[marks[i].label]++;
            }
            for (auto& mk : marks)
                (void)hipEventDestroy(mk.e);
            marks.clear();
        }
        if (kev.empty())
            return;
        CUGO_HIP(hipStreamSynchronize(ctx.stream));
        for (auto& e : kev)
        {
            float ms = 0;
            CUGO_HIP(hipEventElapsedTime(&ms, e.a, e.b));
            kms[e.label] += ms;
            kcount[e.label]++;
            (void)hipEventDestroy(e.a);
            (void)hipEventDestroy(e.b);
        }
        kev.clear();
    }

    double* bp() { return d_b.data(); }
    double* bl() { return d_b.data() + 6 * (size_t)P; }
    double* xp() { return d_x.data(); }
    double* xl() { return d_x.data() + 6 * (size_t)P; }
    double* Hsc() { return d_sys.data(); }
    double* bsc() { return d_sys.data() + 36 * (size_t)hs.n_blocks; }
    cugo_k::ReduceScratch rs() { return {ctx.scratch.data(), ctx.scratch.size()}; }

    // What the three collectives below share.  With a communicator (cugo_graph_set_comm) a collective is one RCCL
    // call queued on the solver's stream (on_comm): no host synchronisation, no callback.  The callback form
    // (cugo_graph_set_shard) is the test hook: it has to wait for the stream, then gets n_cb doubles and an op code
    // (0 / 1: sum / max all-reduce, -1: reduce-scatter, 2 + root: broadcast).
    template <typename Q>
    void collective(double& bytes, int& calls, size_t n_counted, Q&& on_comm, double* d, size_t n_cb, int op_cb)
    {
        bytes += 8.0 * (double)n_counted;
        calls++;
        if (comm)
        {
            timed("exchange", on_comm);
            return;
        }
        if (!xfn)
            throw std::runtime_error("cugo: sharded run without a communicator or an exchange function");
        CUGO_HIP(hipStreamSynchronize(ctx.stream));
        xfn(d, n_cb, op_cb, xuser);
    }
    // all-reduce of n doubles at d over the shards
    void exchange(double* d, size_t n, int op)
    {
        if (world <= 1 && !comm) // a 1-rank communicator still issues its (identity) collectives
            return;
        collective(xchg_bytes, xchg_calls, n, [&] { comm->all_reduce(d, n, op, ctx.stream); }, d, n, op);
    }
    // the sparse LL^T of a sharded run: each rank factors the elimination subtrees it owns and the replicated
    // top of the tree (chol_symbolic: CholPlan::owner) and gets what crosses the boundary by broadcast
    void bind_solver_exchange()
    {
        join_pattern(); // (the helper's analyze_host() reads chol.rank / world / bcast)
        chol.rank = rank, chol.world = world;
        xs_ready = false;
        if (world > 1 || comm) // (a 1-rank communicator can run the owned form too: CUGO_OWN_SUBTREES=1, the rehearsal)
        {
            chol.bcast = [this](double* d, size_t n, int root) { broadcast(d, n, root); };
            chol.bcast_group = [this](bool start) {
                if (comm)
                    comm->group(start);
            };
        }
        else
            chol.bcast = nullptr, chol.bcast_group = nullptr;
        pattern_dirty = true; // the plan depends on (rank, world)
    }
    // ---- the per-trial exchange of the Schur system [Hsc | bsc] --------------------------------------------------
    // Replicated factorisation: every rank needs all of it — one sum all-reduce.  Rank-owned elimination subtrees
    // (chol_symbolic.h: CholPlan::owner): a rank assembles only the blocks and right-hand-side rows of its own
    // fronts and of the replicated top, so the system is packed by ownership (CholPlan::xs_off), the `world`
    // segments are REDUCE-SCATTERED (rank r receives the sum of segment r: 1 / world of the bytes) and the top's
    // part is all-reduced (reduce-scatter + all-gather of the top's rows), then the received units go back to
    // their places in d_sys.  CUGO_REDUCE_SCATTER=0: the all-reduce also in the owned form.
    DevBuf<int64_t> d_xs_off;
    DevBuf<double> d_xbuf;
    bool xs_ready = false; // d_xs_off / d_xbuf are those of the plan at hand
    void prepare_owned_exchange(hipStream_t s)
    {
        xs_ready = false;
        const CholPlan& pl = chol.plan;
        if (!chol.own_subtrees() || !opt.reduce_scatter || pl.xs_off.empty())
            return;
        d_xs_off.upload(pl.xs_off, s);
        d_xbuf.resize((size_t)(pl.xs_seg * world + pl.xs_top) + 16);
        d_xbuf.zero(s); // (the padding behind the shorter segments travels, and is never read)
        CUGO_HIP(hipStreamSynchronize(s));
        xs_ready = true;
    }
    void reduce_scatter(double* d, size_t n_seg)
    { // (counted: the bytes this rank receives)
        collective(xchg_bytes, xchg_calls, n_seg, [&] { comm->reduce_scatter(d, n_seg, ctx.stream); }, d,
                   n_seg * (size_t)world, -1);
    }
    void exchange_system()
    {
        const size_t n = 36 * (size_t)hs.n_blocks + 6 * (size_t)P;
        if (!xs_ready)
        {
            exchange(d_sys.data(), n, 0);
            return;
        }
        const CholPlan& pl = chol.plan;
        const int B = hs.n_blocks;
        cugo_k::launch_xs_pack(ctx.stream, d_xs_off.data(), B, P, d_sys.data(), d_xbuf.data());
        reduce_scatter(d_xbuf.data(), (size_t)pl.xs_seg);
        if (pl.xs_top > 0)
            exchange(d_xbuf.data() + pl.xs_seg * world, (size_t)pl.xs_top, 0);
        cugo_k::launch_xs_unpack(ctx.stream, d_xs_off.data(), B, P, d_xbuf.data(), d_sys.data(), (long)(pl.xs_seg * rank),
                                 (long)(pl.xs_seg * (rank + 1)), (long)(pl.xs_seg * world));
    }
    // broadcast of n doubles at d from rank `root` (update blocks / solution ranges of rank-owned elimination
    // subtrees).  Callback form: op code 2 + root.
    double bcast_bytes = 0;
    int bcast_calls = 0;
    void broadcast(double* d, size_t n, int root)
    {
        if (world <= 1 && !comm)
            return;
        collective(bcast_bytes, bcast_calls, n, [&] { comm->broadcast(d, n, root, ctx.stream); }, d, n, 2 + root);
    }
    // ---- the LM loop's building blocks (Engine::optimize, Engine::compute_covariances) -------------------------------
    // What a call works with, set once at its top (begin_call): everything these are made of (rows_on, splan_on,
    // strip_on, lm_in_one_group, hs, max_row_nnz, the options, the communicator) is fixed once build_structure() has
    // run, so none of them changes inside a call.
    struct CallFacts
    {
        bool sharded = false;
        bool use_rows = false;  // the Schur complement by block rows (k_hsc_rows): T is never written or read
        // T = Hpl invHll is only materialised for the gather kernels (the landmark-major plan keeps it in LDS).  A
        // build pass that knows the damping of the trial behind it leaves invHll and T for it: that trial's Schur
        // complement then does not read the Hpl stream a second time (CUGO_FUSE_T=0: always the separate edge kernel)
        bool can_fuse = false;
        bool ps_on = false;     // ... in the one-stream form: G and the landmarks' lines, k_pose_schur (CUGO_POSE_SCHUR=0: never)
        // Speculative build (single process, CUGO_SPECULATE=0 turns it off): behind the error pass of a first trial
        // the host queues the NEXT iteration's build pass at the trial's estimates before it waits for the trial's
        // result — the 15-20 us the host needs to read F-hat, decide and queue again then overlap with the build
        // instead of leaving the device idle.  The damping that build prepares T for is lambda / 3: what an accepted
        // trial with rho near 1 gives (ref: cuda_graph_optimisation.cpp:97-99, the lower clamp).  Accepted with
        // another lambda: the Schur complement recomputes T (as without the fusion).  Rejected: H is rebuilt from
        // the kept estimates before the retry.  Same arithmetic on the same data in every case.
        bool speculate = false;
        bool trial_poll = false;  // (CUGO_TRIAL_POLL=0: wait by event / stream synchronisation)
        bool trial_event = false; // (CUGO_TRIAL_EVENT=0: wait for the whole stream, A/B)
        // the trial's chi2 out of the NEXT iteration's build pass: that pass is queued behind a first trial anyway
        // (speculation) and computes the residuals of every edge at the trial's estimates — the error pass would
        // compute them a launch earlier and throw them away (CUGO_TRIAL_FROM_BUILD=0; needs the polled wait)
        bool from_build = false;
        size_t blkw = 0; // doubles in a block stream (Hpl, T): 18 per edge slot, 9 when the blocks are stored as float
    } f;
    // ... and the buffers only some forms need, allocated by the first call that takes such a form: T for the
    // gather kernels, the landmarks' lines for the one-stream form of the loop
    void begin_call(bool lm_loop)
    {
        f.sharded = world > 1 || comm;
        f.use_rows = rows_on && cugo_k::schur_rows_usable(hs, max_row_nnz);
        f.can_fuse = opt.fuse_t && !splan_on && lm_in_one_group;
        f.ps_on = opt.pose_schur && f.can_fuse && !f.use_rows && !strip_on;
        f.speculate = !f.sharded && !profile && opt.speculate;
        f.trial_poll = !profile && opt.trial_poll;
        f.trial_event = opt.trial_event;
        f.from_build = opt.trial_from_build && f.speculate && f.trial_poll;
        f.blkw = (ev.block_f32 ? 9 : 18) * (size_t)E;
        if (!splan_on && !f.use_rows && d_T.size() == 0)
            d_T.resize(f.blkw + 16);
        if (lm_loop && f.ps_on && d_lmrec.size() < 16 * (size_t)std::max(L, 1))
            d_lmrec.resize(16 * (size_t)std::max(L, 1));
    }
    // What the loop knows about the buffers H lives in; queue_build() keeps the first two, optimize() the rest.
    struct LmState
    {
        // Hpp, Hpl and invHll are those of the build pass at hand: a fused build pass in the one-stream form writes
        // ONE block stream (G = Hpl L^-T, into d_T) and none of the three, so only the trial it was fused for can
        // run behind it
        bool hpp_valid = true;
        // the damping the build pass at hand left invHll and T (or G and the landmarks' lines) for; < 0: none
        double fused_lambda = -1.0;
        // the Schur complement of the build pass at hand is queued as well, for this damping (< 0: not): the trial
        // that ended the previous iteration took its chi2 from that build pass, and the Schur complement for the
        // predicted damping went out behind the reductions for the host to decide meanwhile
        double schur_lambda = -1.0;
        // H is NOT that of the estimates in force: the next iteration's build pass went out behind this iteration's
        // first trial, at the trial's estimates.  Accepted: it is the next iteration's build pass.  Rejected: H is
        // rebuilt before the retry.
        bool spec_queued = false;
        // the previous damping update hit the lower clamp (rho near 1: lambda / 3, the value the speculation
        // predicts).  Only behind such a step does a trial take its chi2 from the next build pass: right after a step
        // with a smaller gain ratio the prediction usually misses, and a missed Schur complement costs more than the
        // error pass saves (10k graph: 0.8 ms against 0.05)
        bool prev_clamped = false;
    } st;
    int32_t* d_fail_flag() { return reinterpret_cast<int32_t*>(d_scal.data() + 4); }
    // The build pass at the estimates in buffer `buf`.  fuse_lambda < 0: the two-stream pass (Hpp, b, Hll, Hpl).
    // fuse_lambda >= 0 (callers: only with f.can_fuse): it also leaves invHll and T for that damping or, with
    // f.ps_on, G and the landmarks' lines in place of Hpl / invHll / Hpp.  (d_lmrec and skip_poses only go along
    // with a damping: without d_invHll the launcher passes neither on, ba_kernels.hip: launch_build_t.)
    void queue_build(int buf, double fuse_lambda, double* d_chi = nullptr, bool chi_behind_scale = false)
    {
        const bool fuse = fuse_lambda >= 0, one_stream = fuse && f.ps_on;
        timed("build", [&] {
            cugo_k::launch_build(ctx.stream, ev, d_poses[buf].data(), d_lms[buf].data(), rk, d_Hpp.data(), bp(),
                                 d_Hll.data(), bl(), d_Hpl.data(), rs(), d_chi, fuse ? fuse_lambda : -1.0,
                                 fuse ? d_invHll.data() : nullptr, fuse && !f.use_rows ? d_T.data() : nullptr,
                                 one_stream ? d_lmrec.data() : nullptr, one_stream, chi_behind_scale, pe.lm_prior_view());
            pe.queue_build(ctx.stream, d_poses[buf].data(), d_lms[buf].data(), one_stream, d_Hpp.data(), bp(),
                           d_chi || chi_behind_scale, d_chi);
        });
        st.hpp_valid = !one_stream;
        st.fused_lambda = fuse ? fuse_lambda : -1.0;
    }
    // [Hsc | bsc] for this damping from the build pass at hand, linearised at buffer `buf`.  have_T: that pass left
    // invHll and T for it; one_stream: ... in the one-stream form (k_pose_schur forms the diagonal blocks, bp and bsc)
    void queue_schur(double lambda, bool have_T, bool one_stream, int buf)
    {
        timed("schur", [&] {
            cugo_k::launch_schur(ctx.stream, ev, hs, lambda, 0, d_Hpp.data(), bp(), d_Hll.data(), bl(), d_Hpl.data(),
                                 d_invHll.data(), splan_on || f.use_rows ? nullptr : d_T.data(), bsc(), Hsc(), have_T,
                                 f.use_rows ? cugo_k::SchurRows{d_pose_rec.data(), max_row_nnz, nullptr, opt.hsc_mfma, opt.hsc_xcd}
                                            : cugo_k::SchurRows{nullptr, 0, strip_on ? d_off_pi.data() : nullptr,
                                                                opt.hsc_mfma, opt.hsc_xcd,
                                                                one_stream ? d_lmrec.data() : nullptr,
                                                                d_poses[buf].data(), rs(), bp()});
            if (one_stream)
                pe.queue_add_schur(ctx.stream, d_poses[buf].data(), hs.d_rowptr, Hsc(), bp(), bsc());
            else
                pe.queue_offdiag_schur(ctx.stream, d_poses[buf].data(), Hsc());
        });
    }
    // diagnosis: CUGO_DEBUG_HASH=<file> — position-weighted integer checksums of the arrays every stage of the
    // first trial of an iteration leaves behind, computed by kernels queued in the same stream (no host
    // synchronisation: the flow of the loop stays what it is), appended to the file when optimize() returns
    // (hooks build only, make HOOKS=1: the product build has neither the switch nor the checksum kernel)
#ifdef CUGO_DEBUG_HOOKS
    const char* hash_file = nullptr;
    void hash_begin(int niterations)
    {
        hash_file = std::getenv("CUGO_DEBUG_HASH");
        if (!hash_file)
            return;
        d_hash.resize(64 * (size_t)std::max(niterations, 1));
        d_hash.zero(ctx.stream);
    }
    unsigned long long* hash_row(int iteration) { return hash_file && iteration >= 0 ? d_hash.data() + 64 * (size_t)iteration : nullptr; }
    void hash(int iteration, int slot, const void* p, size_t words)
    {
        if (hash_row(iteration))
            cugo_k::launch_hash_words(ctx.stream, p, words, hash_row(iteration) + slot);
    }
    void hash_end(size_t n_records)
    {
        if (!hash_file)
            return;
        std::vector<unsigned long long> h(d_hash.size());
        CUGO_HIP(hipMemcpyAsync(h.data(), d_hash.data(), h.size() * sizeof(h[0]), hipMemcpyDeviceToHost, ctx.stream));
        CUGO_HIP(hipStreamSynchronize(ctx.stream));
        if (FILE* fp = std::fopen(hash_file, "a"))
        {
            std::fprintf(fp, "run\n");
            for (size_t it = 0; it < n_records; it++)
            {
                for (int k = 0; k < 64; k++)
                    std::fprintf(fp, "%016llx ", h[64 * it + k]);
                std::fprintf(fp, "\n");
            }
            std::fclose(fp);
        }
    }
#else
    void hash_begin(int) {}
    void hash(int, int, const void*, size_t) {}
    void hash_end(size_t) {}
#endif
    // factorisation of Hsc + lambda I and the solve for xp; hash_iteration >= 0: with the stage checksums of that
    // iteration (hooks build)
    void queue_factor_solve(double lambda, int hash_iteration = -1)
    {
#ifdef CUGO_DEBUG_HOOKS
        chol.dbg_hash = hash_row(hash_iteration);
#endif
        timed("cholesky", [&] { chol.factor_solve(Hsc(), lambda, bsc(), xp(), d_fail_flag()); });
#ifdef CUGO_DEBUG_HOOKS
        chol.dbg_hash = nullptr;
#endif
    }
    // Returns when h_scal[2..4] hold the words of the trial queued last (F-hat, scale, factorisation flag).
    // behind_spec: a speculative build is queued behind the trial — the host waits for the trial's own last launch
    // only: it then decides and queues the next Schur complement while the build pass still runs.
    // retries: StructureStats::trial_sync_retries.
    void wait_for_trial(bool behind_spec, double& retries)
    {
        const volatile double* seq = h_scal.data() + 5;
        if (!f.sharded && f.trial_poll)
        {
            // the trial's last launch ends by writing the trial's sequence number behind its three words in
            // the pinned block (k_sum_partials2, system-scope release): the host polls that word — no event,
            // no stream synchronisation, and whatever is queued behind the trial keeps running
            const auto w0 = Clock::now();
            auto next_query = w0 + std::chrono::milliseconds(10);
            const auto spin_limit = std::max<Clock::duration>(std::chrono::milliseconds(2), 2 * last_trial_wait);
            for (unsigned long spin = 1; *seq != (double)trial_seq; spin++)
            {
                cpu_relax();
                if ((spin & 0x3FF) != 0)
                    continue;
                // a trial takes 1 ms (kitti_00 shape) to 3.5 ms (10k graph): the host spins through that — on a
                // loaded host a yield hands the core away for a scheduler quantum, longer than the trial —; a
                // wait that lasts longer than twice the previous one (at least 2 ms) offers the core to others
                // between polls, and every ~10 ms the stream is asked whether it is still working
                const auto now = Clock::now();
                if (now - w0 > spin_limit)
                    std::this_thread::yield();
                if (now < next_query)
                    continue;
                next_query = now + std::chrono::milliseconds(10);
                const hipError_t qe = hipStreamQuery(ctx.stream);
                if (qe == hipErrorNotReady)
                    continue;
                CUGO_HIP(qe); // a failed stream will never deliver
                // the stream is idle: everything queued has run, so the word is there (give the write a moment to
                // become visible to this core before calling it lost)
                bool there = false;
                for (int k = 0; k < 100000 && !there; k++)
                {
                    std::atomic_thread_fence(std::memory_order_acquire);
                    there = *seq == (double)trial_seq;
                    cpu_relax();
                }
                if (!there)
                    throw std::runtime_error("cugo: the result of an LM trial never arrived");
            }
            last_trial_wait = Clock::now() - w0;
            std::atomic_thread_fence(std::memory_order_acquire);
            return;
        }
        if (behind_spec && f.trial_event)
            CUGO_HIP(hipEventSynchronize(trial_ev));
        else
            CUGO_HIP(hipStreamSynchronize(ctx.stream));
        if (f.sharded) // (the three words came with a copy queued on the stream)
            return;
        // the three words in the pinned block are this trial's
        for (long spin = 0; *seq != (double)trial_seq; spin++)
        {
            if (spin == 0)
                retries += 1;
            if (spin > 2000000000L)
                throw std::runtime_error("cugo: the result of an LM trial never arrived");
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    }
};

const char* Engine::profile_name(int i)
{
    static const char* names[PROF_COUNT] = {"0: Initialize Optimizer", "1: Build Structure",
                                            "2: Compute Error",        "3: Build System",
                                            "4: Schur Complement",     "5: Symbolic Decomposition",
                                            "6: Numerical Decomposition", "7: Update Solution"};
    return names[i];
}

Engine::Engine(bool plan_only) : impl_(new Impl)
{
    if (plan_only)
    {
        impl_->plan_only = true;
        impl_->chol.ctx = nullptr; // host-only analysis (cugo_chol with a null context)
        return;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
    {
        delete impl_;
        impl_ = nullptr;
        throw std::runtime_error("cugo: no HIP device available (there is no CPU fallback)");
    }
    int dev = 0;
    CUGO_HIP(hipGetDevice(&dev));
    impl_->ctx.device = dev;
    impl_->ctx.stream = cache_stream_acquire();
    impl_->chol.ctx = &impl_->ctx;
    impl_->profile = impl_->opt.profile;
}

Engine::~Engine()
{
    if (impl_)
    {
        if (cugo_k::launch_hook() == impl_)
            cugo_k::set_launch_hook(nullptr);
        impl_->join_pattern();
        hipStream_t s = impl_->ctx.stream, s2 = impl_->s2;
        if (s)
            (void)hipStreamSynchronize(s);
        if (s2)
            (void)hipStreamSynchronize(s2);
        if (impl_->trial_ev)
            (void)hipEventDestroy(impl_->trial_ev);
        delete impl_;
        cache_stream_release(s); // back to the process-wide pool: creating one costs 1-2 ms
        if (s2)
            cache_stream_release(s2);
    }
}

Options& Engine::options() { return impl_->opt; }

void Engine::set_kernel_timing(int mode)
{
    impl_->ktiming = mode;
    cugo_k::set_launch_hook(mode == 1 ? impl_ : nullptr);
}

std::vector<Engine::KernelTime> Engine::kernel_times() const
{
    std::vector<KernelTime> out;
    for (size_t i = 0; i < impl_->klabels.size(); i++)
        out.push_back({impl_->klabels[i], impl_->kms[i], impl_->kcount[i]});
    return out;
}

void Engine::set_shard(int rank, int world, cugo_exchange_fn fn, void* user)
{
    if (world < 1 || rank < 0 || rank >= world)
        throw std::runtime_error("cugo: bad shard");
    impl_->comm.reset();
    impl_->rank = rank, impl_->world = world, impl_->xfn = fn, impl_->xuser = user;
    impl_->bind_solver_exchange();
}

void Engine::set_comm(std::shared_ptr<RcclComm> comm)
{
    if (!comm)
        throw std::runtime_error("cugo: null communicator");
    impl_->rank = comm->rank(), impl_->world = comm->world(), impl_->xfn = nullptr, impl_->xuser = nullptr;
    impl_->comm = std::move(comm);
    impl_->bind_solver_exchange();
}

void Engine::exchange_stats(double& bytes, int& calls) const
{
    bytes = impl_->xchg_bytes, calls = impl_->xchg_calls;
}

void Engine::set_float32_blocks(bool on)
{
    impl_->f32_blocks = on;
}

FlatGraph& Engine::staging()
{
    return impl_->staging;
}

// ---- the device-side stages of Engine::initialize() (the index arithmetic is edge_layout.cpp) ---------------------
// The co-visibility lists decide the Hsc pattern: if they changed, its build, the ordering and the symbolic
// factorisation start NOW on a helper thread and a second stream (see Impl::pat_thread).  Invariant: from
// here until the next join_pattern() nothing may touch P, L, the co-visibility lists or the solver's (rank, world).
bool Engine::Impl::start_pattern_helper(double* prof)
{
    join_pattern();
    if (pat_err)
    {
        pat_err = nullptr; // a failed helper of an earlier call: that structure was never used
        pattern_dirty = true;
    }
    // (the lists the pattern is made from: with relative-pose pairs the augmented ones)
    const bool pat_same = !pattern_dirty && opt.structure_reuse && P == pat_P && pat_lists() == pat_L &&
                          same_bytes(pat_ptr(), pat_cov_ptr) && same_bytes(pat_pose(), pat_cov_pose);
    pat_async_ok = false;
    lists_built = false;
    pat_stage.store(0, std::memory_order_relaxed);
    if (pat_same)
        return false;
    pattern_dirty = true;
    plan_uploaded = false;
    const bool device_build = !plan_only && !opt.schur_plan && !opt.host_structure;
    // (a pure pose graph, no BA edge, takes the host build: build_structure)
    if (!(device_build && opt.async_structure && P > 0 && !cov_pose.empty()))
        return false;
    if (!s2)
        s2 = cache_stream_acquire();
    pat_thread = std::thread([this, prof] {
        try
        {
            // (the current device is per thread: a rank of a multi-GPU job runs on LOCAL_RANK, not 0)
            CUGO_HIP(hipSetDevice(ctx.device));
            const auto t0p = Clock::now();
            if (!build_pattern_gpu(s2, P, pat_lists(), pat_ptr().data(), pat_pose().data(), gstruct))
            {
                pat_stage.store(-1, std::memory_order_release);
                return;
            }
            pat_stage.store(1, std::memory_order_release);
            hsc_rowptr = gstruct.h_rowptr, hsc_colind = gstruct.h_colind;
            prof[PROF_BUILD_STRUCTURE] += ms_since(t0p);
            const auto t1p = Clock::now();
            chol.analyze_host(P, hsc_rowptr.data(), hsc_colind.data());
            // ... and the plan goes to the device from here as well (second stream; upload() waits for
            // its copies): the first optimize() then only builds the contribution lists
            chol.upload(s2);
            plan_uploaded = true;
            prof[PROF_SYMBOLIC] += ms_since(t1p);
            pat_async_ok = true;
        }
        catch (...)
        {
            pat_err = std::current_exception();
            pat_stage.store(-1, std::memory_order_release);
        }
    });
    return true;
}

// Upload of the slot arrays and the estimates: copies from pageable memory block their caller, so a thread of its own
// issues them beside the rest of initialize() (CUGO_UPLOAD_THREAD=0: the calling thread; plan-only: nothing).
// Invariant: `err` is declared before the thread, which may still assign to it while the caller unwinds;
// the destructor joins and then, short of finish(), waits for the stream: the staging of the copies is about to go.
struct Engine::Impl::SlotUpload
{
    Impl& m;
    const FlatGraph& g;
    std::exception_ptr err;
    std::thread t;
    bool pending; // copies may be in flight
    SlotUpload(Impl& impl, const FlatGraph& graph) : m(impl), g(graph), pending(!impl.plan_only)
    {
        if (!pending)
            return;
        // (sized by this thread: it reads the pointers while the copies are still being issued)
        each([](auto& d, const auto& h) { d.resize(h.size()); });
        if (m.opt.upload_thread)
            t = std::thread([this] { copies(); });
        else
            copies(); // (finish() reports what went wrong)
    }
    ~SlotUpload()
    {
        if (t.joinable())
            t.join();
        if (pending && m.ctx.stream)
            (void)hipStreamSynchronize(m.ctx.stream);
    }
    // f(device buffer, its host source) for everything that goes up, in the order of the copies
    template <typename F>
    void each(F&& f)
    {
        const SlotArrays& sl = m.slots;
        f(m.d_e_pose, sl.pose), f(m.d_e_lm, sl.lm), f(m.d_flags, sl.flags), f(m.d_lm_ptr, m.h_lm_ptr);
        f(m.d_meas, sl.meas), f(m.d_omega, sl.omega), f(m.d_cams, g.cams);
        if (g.has_models || g.has_dist) // the model or distortion table takes the extrinsics' place
            f(m.d_cam_ext, m.h_cam_tab);
        else if (g.has_rig) // the extrinsics go up with the cameras (a table parallel to them)
            f(m.d_cam_ext, g.cam_ext);
        if (sl.n_cams > 1)
            f(m.d_cam, sl.cam);
        for (int k = 0; k < 2; k++)
            f(m.d_poses[k], g.poses), f(m.d_lms[k], g.lms);
    }
    void copies()
    {
        try
        {
            CUGO_HIP(hipSetDevice(m.ctx.device)); // (the current device is per thread)
            each([&](auto& d, const auto& h) { d.upload(h, m.ctx.stream); });
        }
        catch (...)
        {
            err = std::current_exception();
        }
    }
    void finish()
    {
        if (!pending)
            return;
        if (t.joinable())
            t.join();
        if (err)
            std::rethrow_exception(err);
        CUGO_HIP(hipStreamSynchronize(m.ctx.stream));
        pending = false;
    }
};

// What initialize() refuses of a graph's edge and camera kinds, first hit first: a kind on a landmark-sharded optimiser,
// a camera table of the wrong size, a camera table together with depth edge sets.
static void refuse_unsupported(const FlatGraph& g, int n_relpose, bool sharded)
{
    const size_t n_cams = g.cams.size() / 5;
    const struct
    {
        bool hit;
        const char* what;
    } refusals[] = {
        {g.lm_priors.n() && sharded, "landmark prior edge sets are not supported on a landmark-sharded (multi-GPU) optimiser yet"},
        {n_relpose && sharded, "relative-pose edge sets are not supported on a landmark-sharded (multi-GPU) optimiser yet"},
        {g.has_depth && sharded, "depth edge sets are not supported on a landmark-sharded (multi-GPU) optimiser yet"},
        {g.has_rig && g.cam_ext.size() != 12 * n_cams,
         "camera extrinsics (sensor poses): the table must hold 12 numbers per camera"},
        {g.has_rig && g.has_depth, "camera extrinsics (sensor poses) together with depth edge sets are not supported yet"},
        {g.has_rig && sharded,
         "camera extrinsics (sensor poses) are not supported on a landmark-sharded (multi-GPU) optimiser yet"},
        {g.has_models && g.cam_model.size() != 5 * n_cams, "camera models: the table must hold 5 numbers per camera"},
        {g.has_models && g.has_depth, "camera models (Kannala-Brandt) together with depth edge sets are not supported yet"},
        {g.has_models && sharded,
         "camera models (Kannala-Brandt) are not supported on a landmark-sharded (multi-GPU) optimiser yet"},
        {g.has_dist && g.cam_dist.size() != 5 * n_cams, "lens distortion: the table must hold 5 numbers per camera"},
        {g.has_dist && g.has_depth, "lens distortion (radial-tangential) together with depth edge sets is not supported yet"},
        {g.has_dist && g.has_models,
         "lens distortion (radial-tangential) and Kannala-Brandt cameras in one graph are not supported yet"},
        {g.has_dist && sharded,
         "lens distortion (radial-tangential) is not supported on a landmark-sharded (multi-GPU) optimiser yet"},
    };
    for (const auto& r : refusals)
        if (r.hit)
            throw std::runtime_error(std::string("cugo: ") + r.what);
}

// The model table of a graph with camera models, which takes the extrinsics' place on the device: {M, t_s, k1..k4, type}
// per entry; a graph whose sensor poses are all identities has no cam_ext.  Likewise the distortion table of a graph with
// lens distortion: {M, t_s, k1, k2, p1, p2, k3, flag} per entry, the flag 1.0 iff the entry's coefficients are not all
// zero.  Empty without either.
static void assemble_cam_table(const FlatGraph& g, std::vector<double>& tab)
{
    static const double I12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    tab.clear();
    const size_t n = g.cams.size() / 5;
    if (g.has_dist)
    {
        tab.resize(CUGO_DIST_TAB_STRIDE * n);
        for (size_t k = 0; k < n; k++)
        {
            double* e = &tab[CUGO_DIST_TAB_STRIDE * k];
            const double* x = g.has_rig ? &g.cam_ext[12 * k] : I12;
            const double* d = &g.cam_dist[5 * k];
            std::copy(x, x + 12, e);
            std::copy(d, d + 5, e + 12);
            e[17] = std::any_of(d, d + 5, [](double c) { return c != 0.0; }) ? 1.0 : 0.0;
        }
        return;
    }
    if (!g.has_models)
        return;
    tab.resize(CUGO_CAM_TAB_STRIDE * n);
    for (size_t k = 0; k < n; k++)
    {
        const double* x = g.has_rig ? &g.cam_ext[12 * k] : I12;
        std::copy(x, x + 12, &tab[CUGO_CAM_TAB_STRIDE * k]);
        std::copy(&g.cam_model[5 * k], &g.cam_model[5 * k] + 5, &tab[CUGO_CAM_TAB_STRIDE * k + 12]);
    }
}

void Engine::initialize(FlatGraph& g)
{
    const auto t0 = Clock::now();
    Impl& m = *impl_;
    InitLaps laps(m.opt.init_timing);
    // Invariant: the first statement that changes anything.  The helper thread of the previous
    // initialize() reads m.P / m.L, the co-visibility lists and the solver's (rank, world).
    m.join_pattern();
    hipStream_t s = m.ctx.stream;
    m.Pall = g.Pall, m.Lall = g.Lall, m.P = g.P, m.L = g.L;
    m.rk = g.rk;
    m.ev.has_depth = g.has_depth ? 1 : 0, m.ev.rk_type_depth = g.rk_type_depth;
    m.ev.rk_delta_depth = g.rk_delta_depth, m.ev.depth_weight = g.depth_weight;
    m.init_rank = m.rank, m.init_world = m.world;
    m.Etot = g.n_edges();
    const int n_relpose = g.kinds[POSE_KIND_RELPOSE].n();
    const int n_pair = g.kinds[POSE_KIND_PAIR].n();
    E_global_ = m.Etot + g.n_pose_edges() + n_relpose + n_pair + g.lm_priors.n();
    refuse_unsupported(g, n_relpose, m.world > 1 || m.comm);
    // (every launcher of an edge pass picks its instantiation from this: cugo_k::edge_form)
    m.ev.has_rig = g.has_dist ? CUGO_RIG_DISTORTION : g.has_models ? CUGO_RIG_MODELS : g.has_rig ? CUGO_RIG_EXTRINSICS : CUGO_RIG_NONE;
    assemble_cam_table(g, m.h_cam_tab);
    // (k_hsc_offdiag_strip reads the list entry before a block's range: a pair block without products has none)
    if (n_relpose && m.opt.hsc_strip)
        throw std::runtime_error("cugo: relative-pose edge sets cannot be combined with CUGO_HSC_STRIP=1: the row-strip "
                                 "form of the Schur complement cannot hold a block without landmark products");
    if (n_pair && m.opt.hsc_strip)
        throw std::runtime_error(std::string("cugo: pose-pose point edge sets (") +
                                 (g.kinds[POSE_KIND_PAIR].cov ? "GicpPairEdgeSet" : "PointPairEdgeSet") +
                                 ") cannot be combined with CUGO_HSC_STRIP=1: "
                                 "the row-strip form of the Schur complement cannot hold a block without landmark products");
    if (n_pair && (m.world > 1 || m.comm))
        throw std::runtime_error(std::string("cugo: pose-pose point edge sets (") +
                                 (g.kinds[POSE_KIND_PAIR].cov ? "GicpPairEdgeSet" : "PointPairEdgeSet") +
                                 ") are not supported on a landmark-sharded (multi-GPU) optimiser yet");
    if (g.kinds[POSE_KIND_POINT].n() && (m.world > 1 || m.comm))
        throw std::runtime_error(std::string("cugo: point-to-point edge sets (") +
                                 (g.kinds[POSE_KIND_POINT].cov ? "GicpEdgeSet" : "PointEdgeSet") +
                                 ") are not supported on a landmark-sharded (multi-GPU) optimiser yet");
    for (int k = POSE_KIND_PRIOR; k >= 0; k--) // (priors first: the message a graph with several kinds has always got)
        if (g.kinds[k].n() && (m.world > 1 || m.comm))
            throw std::runtime_error(std::string("cugo: ") + pose_kind_group(k) +
                                     " edge sets are not supported on a landmark-sharded (multi-GPU) optimiser yet");
    sort_landmark_major(g, m.st_lm_cnt, m.st_order);
    laps.lap("engine: landmark sort");
    // (before anything is started or uploaded) a prior on a free landmark without any edge slot — lm_ptr[l] == lm_ptr[l + 1]
    // in the slot layout, which gives a landmark slots iff it has flattened edges — would shape Hll and bl of a landmark nothing ever steps: the
    // back-substitution walks the landmarks of the slots
    for (int32_t l : g.lm_priors.lm)
        if (m.st_lm_cnt[l] == m.st_lm_cnt[l + 1])
            throw std::runtime_error("cugo: landmark prior edge set: a prior sits on free landmark " + std::to_string(l) +
                                     " (flattened index), which no active BA edge observes; the back-substitution gives such "
                                     "a landmark a zero step (not supported)");
    build_covisibility(g, m.st_lm_cnt, m.st_order, m.cov_ptr, m.cov_pose);
    m.build_pair_lists(g.kinds[POSE_KIND_RELPOSE], g.kinds[POSE_KIND_PAIR]);
    laps.lap("engine: co-visibility");
    // the helper starts before the slot work ...
    const bool helper_started = m.start_pattern_helper(prof_);
    shard_range(m.st_lm_cnt, m.rank, m.world, m.shard_l0, m.shard_l1);
    m.lm_in_one_group = pad_slot_layout(m.st_lm_cnt, m.shard_l0, m.shard_l1, m.h_lm_ptr, m.st_slot_src);
    laps.lap("engine: slot layout");
    m.E = (int)m.st_slot_src.size();
    m.last_err_buf = 0;
    m.xchg_bytes = 0, m.xchg_calls = 0;
    fill_slots(g, m.st_order, m.st_slot_src, m.slots);
    laps.lap("engine: fill slots");
    // the upload of the slot arrays runs beside everything down to the upload sync
    Impl::SlotUpload upload(m, g);
    pose_major_view(m.Pall, m.slots.pose, m.st_slot_src, m.h_pose_ptr, m.h_pose_edge);
    laps.lap("engine: pose-major view");
    m.pe.bind(g, m.Pall, m.P, m.Lall, m.L, s, m.plan_only);
    laps.lap("engine: ICP edge sort");
    // (a plan-only engine has no device: it skips to the topology compare)
    if (!m.plan_only)
    {
        m.d_pose_ptr.upload(m.h_pose_ptr, s);
        m.d_pose_edge.upload(m.h_pose_edge, s);
        m.cur = 0;
        m.d_Hpp.resize(36 * (size_t)m.P + 16), m.d_b.resize(6 * (size_t)m.P + 3 * (size_t)m.L + 16);
        m.d_Hll.resize(9 * (size_t)m.L + 16), m.d_invHll.resize(9 * (size_t)m.L + 16);
        // block streams: 18 doubles per edge slot, or 18 floats (= 9 doubles of storage)
        m.ev.block_f32 = (m.f32_blocks || m.opt.float32) ? 1 : 0;
        m.d_Hpl.resize((m.ev.block_f32 ? 9 : 18) * (size_t)m.E + 16);
        m.d_T.release(); // allocated on demand (gather kernels only), see begin_call()
        m.d_x.resize(6 * (size_t)m.P + 3 * (size_t)m.L + 16);
        m.d_tmp.resize(36 * (size_t)m.P + 16);
        m.d_scal.resize(16), m.d_fail.resize(4), m.h_scal.resize(16), m.h_fail.resize(4);
        m.d_fail.zero(s); // [0] zero-pivot flag, [2] arrival counter of the trial's last launch
        m.h_scal[5] = -1.0;
        m.d_x.zero(s);
        m.ctx.scratch.resize(cugo_k::reduce_scratch_doubles(m.E, m.P, m.L));
        laps.lap("engine: enqueue uploads");
    }
    cugo_edges& ev = m.ev; // what the edge kernels get (null pointers on a plan-only engine)
    ev.n_edges = m.E, ev.n_poses_total = m.Pall, ev.n_landmarks_total = m.Lall;
    ev.n_poses_free = m.P, ev.n_landmarks_free = m.L;
    ev.d_pose = m.d_e_pose.data(), ev.d_lm = m.d_e_lm.data(), ev.d_meas = m.d_meas.data();
    ev.d_omega = m.d_omega.data(), ev.n_omega = m.slots.n_omega, ev.d_flags = m.d_flags.data();
    ev.d_cam = m.slots.n_cams > 1 ? m.d_cam.data() : nullptr, ev.d_cams = m.d_cams.data();
    ev.n_cams = m.slots.n_cams, ev.d_lm_ptr = m.d_lm_ptr.data(), ev.d_pose_ptr = m.d_pose_ptr.data();
    ev.d_pose_edge = m.d_pose_edge.data();
    ev.d_cam_ext = ev.has_rig ? m.d_cam_ext.data() : nullptr;
    // opt-in (CUGO_HSC_ROWS=1): the Schur complement by whole block rows (k_hsc_rows; slower)
    m.rows_on = !m.plan_only && m.opt.hsc_rows && !m.opt.schur_plan;
    if (m.rows_on)
    {
        upload.finish();
        const int n = m.h_pose_ptr[m.Pall];
        m.d_pose_rec.resize(4 * (size_t)std::max(n, 1) + 16);
        cugo_k::launch_pose_rec(s, m.ev, n, m.d_pose_rec.data());
    }
    // Re-use of the Hsc structure, ordering and symbolic factor when the topology is unchanged (ref: the isDirty logic
    // of BlockSolver::buildStructure, block_solver.cpp:151-216): slots, flags and co-visibility lists are compared with
    // the copy the structure at hand was built from
    const int dims[8] = {m.Pall, m.Lall, m.P, m.L, m.E, m.rank, m.world, m.Etot};
    if (!(m.opt.structure_reuse && m.sig_valid && std::memcmp(dims, m.sig_dims, sizeof dims) == 0 &&
          same_bytes(m.slots.pose, m.sig_e_pose) && same_bytes(m.slots.lm, m.sig_e_lm) &&
          same_bytes(m.slots.flags, m.sig_flags) && same_bytes(m.cov_pose, m.sig_cov_pose) &&
          m.pair_lo == m.sig_pair_lo && m.pair_hi == m.sig_pair_hi))
        m.structure_dirty = true;
    std::memcpy(m.pending_dims, dims, sizeof dims);
    laps.lap("engine: topology compare");
    upload.finish();
    laps.lap("engine: upload sync");
    // ... and the contribution lists, which need the helper's pattern and the slots on the device, are built after
    // the upload sync, on this stream, while the helper is still ordering: off the path of the first optimize()
    if (helper_started && m.structure_dirty && !m.plan_only)
    {
        while (m.pat_stage.load(std::memory_order_acquire) == 0)
            std::this_thread::yield();
        if (m.pat_stage.load(std::memory_order_acquire) == 1)
            m.lists_built = build_lists_gpu(s, m.E, m.P, m.Lall, m.d_e_pose.data(), m.d_flags.data(), m.d_lm_ptr.data(), m.gstruct);
        laps.lap("engine: contribution lists");
    }
    prof_[PROF_INITIALIZE] += ms_since(t0);
    if (m.plan_only && m.structure_dirty)
        build_structure(); // no optimize() will follow: the structure is all there is to do
    if (m.plan_only)
        m.pe.bind_relpose_plan(m.hsc_rowptr, m.hsc_colind, s, true);
}

void Engine::fill_structure_stats(int B, double products, double offdiag_products)
{
    Impl& m = *impl_;
    // remember what this structure was built from (Engine::initialize compares on a hash hit)
    std::memcpy(m.sig_dims, m.pending_dims, sizeof m.sig_dims);
    m.sig_valid = m.opt.structure_reuse; // (re-use switched off: nothing will ever be compared with these)
    if (m.sig_valid)
    {
        // (7 MB on the kitti_00 shape, on the path of a new graph's first optimize(): copied by the pool)
        auto copy = [](auto& dst, const auto& src) {
            dst.resize(src.size());
            const size_t bytes = src.size() * sizeof(src[0]);
            if (bytes == 0)
                return; // (an empty vector's data() may be null: not a valid memcpy argument)
            const char* from = reinterpret_cast<const char*>(src.data());
            char* to = reinterpret_cast<char*>(dst.data());
            parallel_chunks(bytes, 1u << 18, [&](size_t a, size_t b, unsigned) { std::memcpy(to + a, from + a, b - a); });
        };
        copy(m.sig_e_pose, m.slots.pose), copy(m.sig_e_lm, m.slots.lm), copy(m.sig_flags, m.slots.flags);
        copy(m.sig_cov_pose, m.cov_pose);
        m.sig_pair_lo = m.pair_lo, m.sig_pair_hi = m.pair_hi;
    }
    // row strips, opt-in (CUGO_HSC_STRIP=1; default: one wave per block anywhere): per product the position of
    // its T edge in the edge list of its pose.  Bit for bit the gather kernel's sums with each T block read once,
    // but one 16-wave workgroup per CU cannot hide the gather latency the way 32 independent waves do:
    // measured 13.69 vs 11.45 ms per step (kitti_00 shape), 59.6 vs 41.2 ms (10k-pose graph)
    m.strip_on = false;
    {
        const size_t M = (size_t)offdiag_products;
        if (!m.plan_only && !m.splan_on && m.hs.d_off_ei && M > 0 && m.opt.hsc_strip)
        {
            m.d_pose_pos.resize((size_t)std::max(m.E, 1) + 16), m.d_off_pi.resize(M + 16);
            cugo_k::launch_list_pos(m.ctx.stream, m.ev, m.h_pose_ptr[m.Pall], M, m.hs.d_off_ei, m.d_pose_pos.data(),
                                    m.d_off_pi.data());
            m.strip_on = true;
        }
    }
    m.max_row_nnz = 0;
    for (size_t q = 0; q + 1 < m.hsc_rowptr.size(); q++)
        m.max_row_nnz = std::max(m.max_row_nnz, (int)(m.hsc_rowptr[q + 1] - m.hsc_rowptr[q]));
    sstats_.hsc_blocks = B;
    sstats_.products = products;
    sstats_.offdiag_products = offdiag_products;
    sstats_.nnzL = m.chol.plan.nnzL;
    sstats_.chol_flops = m.chol.plan.flops;
    sstats_.supernodes = m.chol.plan.n_super;
    sstats_.stages = m.chol.plan.n_stages;
    sstats_.front_bytes = 8.0 * (double)m.chol.plan.front_doubles;
    {
        const auto& pl = m.chol.plan;
        sstats_.chol_rank_flops = pl.rank_flops, sstats_.chol_top_flops = pl.top_flops;
        double bytes = 0;
        for (size_t k = 0; k < pl.xu_front.size(); k++)
        {
            const int f = pl.xu_front[k];
            const int64_t c0 = 6LL * pl.ncb[f], c1 = 6LL * pl.nb[f];
            if (c1 > c0)
                bytes += 8.0 * (double)((c1 - 1 - c0) * pl.ldf[f] + c1 + 1 - c0);
        }
        for (size_t k = 0; k < pl.xx_lo.size(); k++)
            bytes += 8.0 * 6.0 * (pl.xx_hi[k] - pl.xx_lo[k]);
        sstats_.chol_bcast_bytes = bytes, sstats_.chol_bcasts = (double)(pl.xu_front.size() + pl.xx_lo.size());
    }
    // sharded: what the per-trial exchange of the Schur system hands to this rank
    sstats_.xchg_sys_full_bytes = sstats_.xchg_sys_bytes = 0;
    if (m.world > 1 || m.comm)
    {
        if (!m.plan_only)
            m.prepare_owned_exchange(m.ctx.stream);
        const auto& pl = m.chol.plan;
        sstats_.xchg_sys_full_bytes = 8.0 * (36.0 * B + 6.0 * m.P);
        const bool keyed = m.plan_only ? (pl.owned && m.opt.reduce_scatter && !pl.xs_off.empty()) : m.xs_ready;
        sstats_.xchg_sys_bytes = keyed ? 8.0 * (double)(pl.xs_seg + pl.xs_top) : sstats_.xchg_sys_full_bytes;
    }
    sstats_.up_potrf_flops = m.chol.plan.up_potrf_flops;
    sstats_.up_trsm_flops = m.chol.plan.up_trsm_flops;
    sstats_.up_syrk_flops = m.chol.plan.up_syrk_flops;
    sstats_.up_ea_bytes = m.chol.plan.up_ea_bytes;
    sstats_.backward_bytes = m.chol.plan.backward_bytes;
}

void Engine::refresh_estimates(const FlatGraph& g)
{
    const auto t0 = Clock::now();
    Impl& m = *impl_;
    if ((int)(g.poses.size() / 7) != m.Pall || (int)(g.lms.size() / 3) != m.Lall)
        throw std::runtime_error("cugo: refresh_estimates on another graph");
    if (m.rank != m.init_rank || m.world != m.init_world)
        throw std::runtime_error("cugo: refresh_estimates after the shard changed (a full initialize() is needed)");
    m.last_err_buf = 0;
    m.xchg_bytes = 0, m.xchg_calls = 0;
    m.cur = 0;
    if (!m.plan_only)
    {
        hipStream_t s = m.ctx.stream;
        // one copy from (pageable) host memory per array; the second buffer is filled on the device
        m.d_poses[0].upload(g.poses, s);
        m.d_lms[0].upload(g.lms, s);
        m.d_poses[1].resize(g.poses.size()), m.d_lms[1].resize(g.lms.size());
        if (!g.poses.empty())
            CUGO_HIP(hipMemcpyAsync(m.d_poses[1].data(), m.d_poses[0].data(), g.poses.size() * sizeof(double),
                                    hipMemcpyDeviceToDevice, s));
        if (!g.lms.empty())
            CUGO_HIP(hipMemcpyAsync(m.d_lms[1].data(), m.d_lms[0].data(), g.lms.size() * sizeof(double),
                                    hipMemcpyDeviceToDevice, s));
        m.d_x.zero(s);
        CUGO_HIP(hipStreamSynchronize(s)); // the staging vectors may change after return
    }
    prof_[PROF_INITIALIZE] += ms_since(t0);
}

double* Engine::pinned_poses()
{
    Impl& m = *impl_;
    m.h_pin_poses.resize(7 * (size_t)std::max(m.Pall, 1));
    return m.h_pin_poses.data();
}
double* Engine::pinned_lms()
{
    Impl& m = *impl_;
    m.h_pin_lms.resize(3 * (size_t)std::max(m.Lall, 1));
    return m.h_pin_lms.data();
}

void Engine::refresh_estimates_pinned()
{
    const auto t0 = Clock::now();
    Impl& m = *impl_;
    if (m.rank != m.init_rank || m.world != m.init_world)
        throw std::runtime_error("cugo: refresh_estimates after the shard changed (a full initialize() is needed)");
    m.last_err_buf = 0;
    m.xchg_bytes = 0, m.xchg_calls = 0;
    m.cur = 0;
    if (!m.plan_only)
    {
        hipStream_t s = m.ctx.stream;
        const size_t np = 7 * (size_t)m.Pall, nl = 3 * (size_t)m.Lall;
        const double* hp = pinned_poses();
        const double* hl = pinned_lms();
        for (int b = 0; b < 2; b++)
            m.d_poses[b].resize(np), m.d_lms[b].resize(nl);
        if (np)
        {
            CUGO_HIP(hipMemcpyAsync(m.d_poses[0].data(), hp, np * sizeof(double), hipMemcpyHostToDevice, s));
            CUGO_HIP(hipMemcpyAsync(m.d_poses[1].data(), m.d_poses[0].data(), np * sizeof(double), hipMemcpyDeviceToDevice, s));
        }
        if (nl)
        {
            CUGO_HIP(hipMemcpyAsync(m.d_lms[0].data(), hl, nl * sizeof(double), hipMemcpyHostToDevice, s));
            CUGO_HIP(hipMemcpyAsync(m.d_lms[1].data(), m.d_lms[0].data(), nl * sizeof(double), hipMemcpyDeviceToDevice, s));
        }
        m.d_x.zero(s);
        // no wait: the staging is the engine's own pinned memory; whoever gathers into it again before these copies
        // have run queues a later copy of the whole array behind them (same stream), and that one is what counts
    }
    prof_[PROF_INITIALIZE] += ms_since(t0);
}

bool Engine::download_pinned(const double** poses, const double** lms)
{
    Impl& m = *impl_;
    if (m.world > 1 || m.plan_only)
        return false;
    hipStream_t s = m.ctx.stream;
    const size_t np = 7 * (size_t)m.Pall, nl = 3 * (size_t)m.Lall;
    double* hp = pinned_poses();
    double* hl = pinned_lms();
    if (nl)
        CUGO_HIP(hipMemcpyAsync(hl, m.d_lms[m.cur].data(), nl * sizeof(double), hipMemcpyDeviceToHost, s));
    if (np)
        CUGO_HIP(hipMemcpyAsync(hp, m.d_poses[m.cur].data(), np * sizeof(double), hipMemcpyDeviceToHost, s));
    CUGO_HIP(hipStreamSynchronize(s));
    *poses = hp, *lms = hl;
    return true;
}

// ---- Engine::build_structure(): Hsc pattern from landmark co-visibility + contribution lists + Cholesky analysis
// (ref: buildStructure, block_solver.cpp:139-248) — by one of two builders, adopted in one place
void Engine::adopt_structure(const cugo_hsc_struct& hs, double products, double offdiag_products, double schur_slots)
{
    Impl& m = *impl_;
    m.hs = hs;
    if (!m.plan_only)
        m.d_sys.resize(36 * (size_t)hs.n_blocks + 6 * (size_t)m.P + 16);
    fill_structure_stats(hs.n_blocks, products, offdiag_products);
    sstats_.schur_slots = schur_slots;
    // (a plan-only engine builds its structure in every initialize(): nothing else would ever show a changed option)
    m.structure_dirty = m.plan_only;
    m.pe.rp.plan_dirty = true; // (the block indices of the relative-pose plan are those of the pattern)
}

// Device-side build (structure_gpu.h): the same lists, in the same order, as the host passes; a shard builds the
// pattern from the global co-visibility lists.  False: the device build refused, nothing was adopted.
bool Engine::device_structure(InitLaps& laps)
{
    Impl& m = *impl_;
    hipStream_t s = m.ctx.stream;
    const int P = m.P;
    const bool have_lists = m.lists_built && m.pat_async_ok; // (built at the end of initialize() for this pattern)
    m.lists_built = false;
    // phase 1 (unless the helper thread of initialize() has done it, or the lists are those of the
    // pattern at hand): Hsc pattern from the co-visibility lists, ordering + symbolic factorisation
    if (m.pattern_dirty && !m.pat_async_ok)
    {
        if (!build_pattern_gpu(s, P, m.pat_lists(), m.pat_ptr().data(), m.pat_pose().data(), m.gstruct))
            return false;
        m.hsc_rowptr = m.gstruct.h_rowptr, m.hsc_colind = m.gstruct.h_colind;
        prof_[PROF_BUILD_STRUCTURE] += ms_since(laps.t0);
        const auto t1g = Clock::now();
        m.chol.analyze_host(P, m.hsc_rowptr.data(), m.hsc_colind.data());
        prof_[PROF_SYMBOLIC] += ms_since(t1g);
    }
    laps.lap("structure: pattern + symbolic (unless done beside initialize)");
    // phase 2: the contribution lists from the slots on the device
    const auto t2 = Clock::now();
    if (!have_lists && !build_lists_gpu(s, m.E, P, m.Lall, m.d_e_pose.data(), m.d_flags.data(), m.d_lm_ptr.data(), m.gstruct))
        return false;
    laps.lap("structure: contribution lists (device)");
    if (!m.plan_uploaded) // (the helper thread of initialize() uploads the plans it analyses)
    {
        m.chol.upload(s);
        m.plan_uploaded = true;
    }
    if (m.pattern_dirty)
        m.pat_P = P, m.pat_L = m.pat_lists(), m.pat_cov_ptr = m.pat_ptr(), m.pat_cov_pose = m.pat_pose();
    m.pattern_dirty = false;
    m.gstruct.scratch.release(), m.gstruct.scratch2.release();
    cugo_hsc_struct hs{};
    hs.n_blocks = m.gstruct.B;
    hs.d_rowptr = m.gstruct.rowptr.data(), hs.d_colind = m.gstruct.colind.data();
    hs.d_off_ptr = m.gstruct.off_ptr.data(), hs.d_off_ei = m.gstruct.off_ei.data();
    hs.d_off_ej = m.gstruct.off_ej.data();
    m.splan_on = false;
    // all products of the graph (every free-free edge also has its diagonal one) / local off-diagonal ones
    const double diag_products = m.world > 1 || m.comm ? (double)m.cov_pose.size() : count_free_free(m.slots.flags);
    prof_[PROF_BUILD_STRUCTURE] += ms_since(t2);
    laps.lap("structure: plan upload");
    // (with relative-pose pairs the pattern's lists hold one entry per pair that is no product: single process, so the
    //  off-diagonal products of the graph are those of the local lists)
    const double offdiag_global = m.pair_lo.empty() ? (double)m.gstruct.Mglobal : (double)m.gstruct.Moff;
    adopt_structure(hs, offdiag_global + diag_products, (double)m.gstruct.Moff, 0);
    return true;
}

void Engine::host_structure(InitLaps& laps)
{
    Impl& m = *impl_;
    hipStream_t s = m.ctx.stream;
    const int P = m.P;
    // The landmark-major product plan (schur_plan.h) on request (CUGO_SCHUR_PLAN=1); unusable
    // if a landmark's active edges straddle two slot groups
    HostStructure hst;
    SchurPlanHost sp;
    cugo_host::host_structure(
        P, m.L, m.cov_ptr, m.cov_pose, m.slots, m.h_lm_ptr, m.h_pose_ptr, m.h_pose_edge,
        [&] {
            if (m.opt.schur_plan)
                build_schur_plan(m.E, P, m.slots.pose.data(), m.slots.lm.data(), m.slots.flags.data(),
                                 m.hsc_rowptr.data(), m.hsc_colind.data(), sp);
            laps.lap("structure: landmark-major product plan");
            return m.splan_on = sp.usable;
        },
        [&](const char* what) { laps.lap(what); }, m.hsc_rowptr, m.hsc_colind, hst, &m.pair_lo, &m.pair_hi);
    laps.lap("structure: product lists");
    // off-diagonal products: from the lists, or (plan) all products minus one per free-free edge
    const double n_offdiag = m.splan_on ? (double)sp.prod.size() - count_free_free(m.slots.flags) : (double)hst.off_ei.size();
    cugo_hsc_struct hs{};
    hs.n_blocks = (int)m.hsc_colind.size();
    if (!m.plan_only)
    {
        m.d_hsc_rowptr.upload(m.hsc_rowptr, s), m.d_hsc_colind.upload(m.hsc_colind, s);
        m.d_off_ptr.upload(hst.off_ptr, s), m.d_off_ei.upload(hst.off_ei, s), m.d_off_ej.upload(hst.off_ej, s);
        CUGO_HIP(hipStreamSynchronize(s));
        hs.d_rowptr = m.d_hsc_rowptr.data(), hs.d_colind = m.d_hsc_colind.data();
        hs.d_off_ptr = m.d_off_ptr.data(), hs.d_off_ei = m.d_off_ei.data();
        hs.d_off_ej = m.d_off_ej.data();
        if (m.splan_on)
        {
            m.splan.upload(sp, s);
            m.splan.fill(hs);
        }
        laps.lap("structure: uploads");
    }
    prof_[PROF_BUILD_STRUCTURE] += ms_since(laps.t0);
    const auto t1 = Clock::now();
    m.chol.analyze(P, m.hsc_rowptr.data(), m.hsc_colind.data());
    prof_[PROF_SYMBOLIC] += ms_since(t1);
    if (!m.plan_only)
        laps.lap("structure: symbolic + plan upload");
    adopt_structure(hs, hst.products, n_offdiag, m.splan_on ? sp.n_slots : 0);
}

void Engine::build_structure()
{
    Impl& m = *impl_;
    InitLaps laps(m.opt.init_timing);
    m.join_pattern();
    if (m.pat_err)
    {
        std::exception_ptr e = m.pat_err;
        m.pat_err = nullptr;
        std::rethrow_exception(e);
    }
    const bool shard = m.world > 1 || m.comm; // local slots are a subset: the pattern comes from the global lists
    if (!m.plan_only && (m.E > 0 || shard) && !m.opt.schur_plan && !m.opt.host_structure && m.P > 0 &&
        !m.cov_pose.empty() && device_structure(laps))
        return;
    // the host build starts from scratch, also after a refused device build
    m.pattern_dirty = true, m.plan_uploaded = false;
    host_structure(laps);
}

void Engine::optimize(int niterations, std::vector<IterRecord>& records, bool verbose)
{
    Impl& m = *impl_;
    if (m.plan_only)
        throw std::runtime_error("cugo: no HIP device in use (plan-only optimiser)");
    hipStream_t s = m.ctx.stream;
    const int maxq = 10;
    const double tau = 1e-5;
    double nu = 2.0, lambda = 0.0, F = 0.0;

    if (m.structure_dirty)
        build_structure();
    if ((m.pe.n_relpose || m.pe.n_pair) && m.pe.rp.plan_dirty)
    {
        m.join_pattern(); // (the helper of initialize() writes the host pattern)
        m.pe.bind_relpose_plan(m.hsc_rowptr, m.hsc_colind, s, false);
    }
    m.begin_call(true);
    const Impl::CallFacts& f = m.f;
    Impl::LmState& st = m.st = Impl::LmState{};
    auto sync_prof = [&](int item, Clock::time_point t0) {
        if (m.profile)
        {
            CUGO_HIP(hipStreamSynchronize(s));
            prof_[item] += ms_since(t0);
        }
    };
    m.hash_begin(niterations);

    for (int iteration = 0; iteration < niterations; iteration++)
    {
        const auto it0 = Clock::now();
        // computeErrors + buildSystem fused: chi2 at the current estimates comes out of the
        // build pass (ref: cuda_graph_optimisation.cpp:64-67).  From the second iteration on the damping of the first
        // trial is known when the build is queued — unless the pass went out behind the previous iteration's trial
        auto tb = Clock::now();
        if (!st.spec_queued) // (chi2 of the build pass is only consumed in the first iteration, see below)
            m.queue_build(m.cur, f.can_fuse && iteration > 0 ? lambda : -1.0, iteration == 0 ? m.d_scal.data() : nullptr);
        st.spec_queued = false;
        sync_prof(PROF_BUILD_SYSTEM, tb);
        // chi2 at the current estimates is only read back in the first iteration: afterwards it is
        // the F-hat of the accepted trial (same edges, same estimates), so the host does not have
        // to wait for the build pass before queueing the Schur complement
        if (iteration == 0)
        {
            const double* hpp = m.d_Hpp.data();
            if (f.sharded)
            { // diag(Hpp) must be the global sum before taking the maximum
                CUGO_HIP(hipMemcpyAsync(m.d_tmp.data(), m.d_Hpp.data(), 36 * (size_t)m.P * sizeof(double),
                                        hipMemcpyDeviceToDevice, s));
                m.exchange(m.d_tmp.data(), 36 * (size_t)m.P, 0);
                hpp = m.d_tmp.data();
            }
            cugo_k::launch_max_diagonal(s, hpp, m.P, m.d_Hll.data(), m.L, m.rs(), m.d_scal.data() + 1);
            if (f.sharded)
            {
                m.exchange(m.d_scal.data(), 1, 0);
                m.exchange(m.d_scal.data() + 1, 1, 1);
            }
            CUGO_HIP(hipMemcpyAsync(m.h_scal.data(), m.d_scal.data(), 2 * sizeof(double), hipMemcpyDeviceToHost, s));
            CUGO_HIP(hipStreamSynchronize(s));
            F = m.h_scal[0];
            lambda = tau * m.h_scal[1];
        }

        int q = 0;
        double rho = -1.0;
        for (; q < maxq && rho < 0; q++)
        {
            const int hash_it = q == 0 ? iteration : -1; // (checksums: of an iteration's first trial)
            // ---- H: invHll and T of this lambda came with the build pass (a first trial whose damping the pass knew)
            const bool trial_fused = q == 0 && st.fused_lambda == lambda;
            const bool one_stream = trial_fused && f.ps_on; // (the build pass wrote G into d_T and the landmarks' lines)
            if (st.spec_queued || (!one_stream && !st.hpp_valid))
            { // the previous trial was rejected and the speculative pass behind it overwrote H; or the build pass at
              // hand was a one-stream one and this trial is not the one it was for — the predicted damping missed,
              // or the fused trial was rejected with no speculative build behind it: the two-stream build pass at
              // the estimates in force
                m.queue_build(m.cur, -1.0);
                st.spec_queued = false;
            }
            // what the build pass left
            m.hash(hash_it, 0, m.d_Hpp.data(), 36 * (size_t)m.P);
            m.hash(hash_it, 1, m.d_b.data(), 6 * (size_t)m.P + 3 * (size_t)m.L);
            m.hash(hash_it, 2, m.d_Hll.data(), 9 * (size_t)m.L);
            m.hash(hash_it, 3, m.d_Hpl.data(), f.blkw);
            // ---- Schur complement (unless it was queued behind the previous trial, for this very damping)
            auto ts = Clock::now();
            if (!(trial_fused && st.schur_lambda == lambda))
                m.queue_schur(lambda, trial_fused, one_stream, m.cur);
            st.schur_lambda = -1.0;
            if (f.sharded)
                m.exchange_system();
            sync_prof(PROF_SCHUR, ts);
            m.hash(hash_it, 4, m.d_sys.data(), 36 * (size_t)m.hs.n_blocks + 6 * (size_t)m.P);
            if (m.d_T.size())
                m.hash(hash_it, 5, m.d_T.data(), f.blkw);
            m.hash(hash_it, 6, m.d_invHll.data(), 9 * (size_t)m.L);
            // ---- factorisation and solve
            auto tn = Clock::now();
            m.queue_factor_solve(lambda, hash_it);
            sync_prof(PROF_NUMERIC, tn);
            m.hash(hash_it, 7, m.xp(), 6 * (size_t)m.P);
            // ---- back-substitution and update into the other estimate buffer.
            // single process: the two reductions that end a trial (scale of the update pass, chi2 of
            // the error pass) share one launch, which also drops F-hat, scale and the factorisation flag
            // (slot 4) into the pinned block — no copy is queued behind it.  A shard has to all-reduce
            // the two sums first and keeps the separate launches and the read-back.
            auto tu = Clock::now();
            const int nxt = m.cur ^ 1;
            int n_scale_part = 0;
            // one_stream: G^T dx_p from the build pass's records (CUGO_BS_RECORDS=0: from the G blocks).  The records
            // are valid from a build pass until the first error pass behind it (launch_errors_tail parks its chi2
            // partials in their area).  A one-stream trial is the first trial behind the fused build pass it was for,
            // at the estimates in m.cur: queued at the top of this iteration, or behind the previous trial — then
            // after that trial's error pass, or (from_build) in its place — and between that build pass and here only
            // the Schur pass (which reads the same records), the factorisation and the solve have run.  A retry
            // rebuilds H with the two-stream pass (fused_lambda < 0 above), so it is never one_stream
            m.timed("backsubst_update", [&] {
                n_scale_part = cugo_k::launch_backsubst_update(
                    s, m.ev, lambda, (m.rank == 0 ? lambda : 0.0), m.d_invHll.data(), m.bl(), m.bp(),
                    one_stream ? m.d_T.data() : m.d_Hpl.data(), m.xp(), m.xl(), m.d_poses[m.cur].data(), m.d_lms[m.cur].data(),
                    m.d_poses[nxt].data(), m.d_lms[nxt].data(), m.rs(), f.sharded ? m.d_scal.data() + 3 : nullptr,
                    one_stream ? m.d_lmrec.data() : nullptr, one_stream && m.opt.bs_records);
            });
            sync_prof(PROF_UPDATE, tu);
            m.hash(hash_it, 8, m.xl(), 3 * (size_t)m.L);
            m.hash(hash_it, 9, m.d_poses[nxt].data(), 7 * (size_t)m.Pall);
            m.hash(hash_it, 10, m.d_lms[nxt].data(), 3 * (size_t)m.Lall);
            // ---- end of the trial: its chi2 from the next iteration's build pass or from an error pass, and the
            // speculative work behind it, all for the damping an accepted step with rho near 1 gives
            auto te = Clock::now();
            const double lambda_pred = lambda * (1.0 / 3.0);
            const double fuse_pred = f.can_fuse ? lambda_pred : -1.0;
            const bool last = iteration + 1 == niterations;
            const bool from_build = f.from_build && q == 0 && !last && st.prev_clamped;
            if (from_build)
            {
                m.queue_build(nxt, fuse_pred, nullptr, true);
                m.timed("errors", [&] { // (the ICP chunk totals are those of the build pass just queued)
                    int n_icp_chi = 0;
                    const double* icp_chi = m.pe.chi_totals(&n_icp_chi);
                    cugo_k::launch_trial_tail_from_build(s, m.ev, m.rs(), n_scale_part, m.d_scal.data() + 2,
                                                         m.d_scal.data() + 4, m.h_scal.data() + 2, (double)++m.trial_seq,
                                                         reinterpret_cast<unsigned*>(m.d_fail.data() + 2), icp_chi,
                                                         n_icp_chi);
                });
                if (f.can_fuse)
                { // the Schur complement of the next iteration's first trial, should the damping be the predicted one:
                  // the host decides while it runs
                    m.queue_schur(lambda_pred, true, f.ps_on, nxt);
                    st.schur_lambda = lambda_pred;
                }
                st.spec_queued = true;
            }
            else
            m.timed("errors", [&] {
                if (f.sharded)
                    cugo_k::launch_errors(s, m.ev, m.d_poses[nxt].data(), m.d_lms[nxt].data(), m.rk,
                                          m.rs(), m.d_scal.data() + 2);
                else
                {
                    int n_icp_chi = 0;
                    const double* icp_chi = m.pe.chi_totals(&n_icp_chi);
                    m.pe.queue_errors(s, m.d_poses[nxt].data(), m.d_lms[nxt].data());
                    cugo_k::launch_errors_tail(s, m.ev, m.d_poses[nxt].data(), m.d_lms[nxt].data(), m.rk, m.rs(),
                                               n_scale_part, m.d_scal.data() + 2, m.d_scal.data() + 4,
                                               m.h_scal.data() + 2, (double)++m.trial_seq,
                                               reinterpret_cast<unsigned*>(m.d_fail.data() + 2), icp_chi, n_icp_chi);
                }
            });
            m.last_err_buf = nxt;
            sync_prof(PROF_COMPUTE_ERROR, te);
            if (!from_build && f.speculate && q == 0 && !last)
            {
                if (!f.trial_poll && f.trial_event)
                {
                    if (!m.trial_ev)
                        CUGO_HIP(hipEventCreateWithFlags(&m.trial_ev, hipEventDisableTiming));
                    CUGO_HIP(hipEventRecord(m.trial_ev, s));
                }
                m.queue_build(nxt, fuse_pred);
                st.spec_queued = true;
            }
            const bool flag_summed = f.sharded && m.chol.own_subtrees();
            if (f.sharded)
            {
                // ranks that factor different subtrees see different zero-pivot flags: as a double the flag
                // rides in the same sum all-reduce as F-hat and the scale
                if (flag_summed)
                    cugo_k::launch_flag_to_double(s, m.d_fail_flag());
                m.exchange(m.d_scal.data() + 2, flag_summed ? 3 : 2, 0);
                CUGO_HIP(hipMemcpyAsync(m.h_scal.data() + 2, m.d_scal.data() + 2, 3 * sizeof(double),
                                        hipMemcpyDeviceToHost, s));
            }
            m.wait_for_trial(st.spec_queued, sstats_.trial_sync_retries);
            // ---- gain ratio and damping (ref: cuda_graph_optimisation.cpp:85-120)
            int32_t fail_flag;
            std::memcpy(&fail_flag, m.h_scal.data() + 4, sizeof fail_flag);
            if (flag_summed)
                fail_flag = m.h_scal[4] > 0.5 ? 1 : 0;
            const bool success = fail_flag == 0;
            const double Fhat = m.h_scal[2];
            const double scale = (success ? m.h_scal[3] : 0.0) + 1e-3;
            const double Fdiff = Fhat - F;
            rho = success ? (F - Fhat) / scale : -1.0;
            if (!success)
                std::printf("factorize failed!\n"); // ref: cuda_linear_solver.cpp:48
            if (rho > 0)
            { // ref: cuda_graph_optimisation.cpp:97-120
                const double a = 1 - std::pow(2 * rho - 1, 3);
                lambda *= std::max(1.0 / 3.0, std::min(a, 2.0 / 3.0));
                st.prev_clamped = a <= 1.0 / 3.0;
                nu = 2.0;
                F = Fhat;
                m.cur = nxt; // accept: the trial buffer becomes the estimate (no pop needed), and a speculative
                break;       // build pass behind the trial (st.spec_queued) the next iteration's build pass
            }
            else
            {
                lambda *= nu;
                nu *= 2.0;
                st.prev_clamped = false;
                if (!std::isfinite(lambda) || (success && Fdiff < 1e-4))
                    break;
            }
        }
        records.push_back({iteration, F, lambda, rho, q});
        if (verbose)
            std::printf("iteration= %i;   time(ms): %.4f   chi2= %f;   lambda= %f   rho= %f	   "
                        "nedges= %i    levenberg iterations = %i\n",
                        iteration, ms_since(it0), F, lambda, rho, E_global_, q);
        if (q == maxq || rho < 1e-6 || !std::isfinite(lambda))
            break;
    }
    m.hash_end(records.size());
    m.collect_times();
}

std::vector<int32_t> Engine::reject_outliers()
{
    Impl& m = *impl_;
    std::vector<int32_t> out;
    if (m.slots.slot_threshold.empty() || m.E == 0)
        return out;
    hipStream_t s = m.ctx.stream;
    // chi2 per slot at the estimates of the last error pass (a rejected trial's estimates if the
    // last trial was rejected: the reference reads whatever d_chiValues holds at that point)
    DevBuf<double> d_chi;
    d_chi.resize((size_t)m.E + 16);
    cugo_k::launch_edge_chi(s, m.ev, m.d_poses[m.last_err_buf].data(), m.d_lms[m.last_err_buf].data(), m.rk,
                            d_chi.data());
    std::vector<double> chi(m.E);
    CUGO_HIP(hipMemcpyAsync(chi.data(), d_chi.data(), sizeof(double) * m.E, hipMemcpyDeviceToHost, s));
    CUGO_HIP(hipStreamSynchronize(s));
    std::vector<int32_t> slots;
    for (int i = 0; i < m.E; i++)
        if (m.slots.slot_edge[i] >= 0 && m.slots.slot_threshold[i] > 0.0 && !(m.slots.flags[i] & CUGO_EDGE_INACTIVE) &&
            chi[i] > m.slots.slot_threshold[i])
            slots.push_back(i);
    for (int i : slots)
        out.push_back(m.slots.slot_edge[i]);
    if (m.world > 1)
    { // every rank needs the union: one sum all-reduce of a 0/1 mask over the global edge ids
        std::vector<double> mask(m.Etot, 0.0);
        for (int e : out)
            mask[e] = 1.0;
        DevBuf<double> d_mask;
        d_mask.upload(mask, s);
        m.exchange(d_mask.data(), (size_t)m.Etot, 0);
        CUGO_HIP(hipMemcpyAsync(mask.data(), d_mask.data(), sizeof(double) * m.Etot, hipMemcpyDeviceToHost, s));
        CUGO_HIP(hipStreamSynchronize(s));
        out.clear();
        for (int e = 0; e < m.Etot; e++)
            if (mask[e] > 0.5)
                out.push_back(e);
    }
    else
        std::sort(out.begin(), out.end());
    if (!out.empty())
    { // the flagged edges drop out of a further optimize() on the same initialisation, too
        for (int i : slots)
            m.slots.flags[i] |= CUGO_EDGE_INACTIVE;
        m.d_flags.upload(m.slots.flags, s);
        if (m.rows_on) // the records of the pose-major list carry the flags
            cugo_k::launch_pose_rec(s, m.ev, m.h_pose_ptr[m.Pall], m.d_pose_rec.data());
        CUGO_HIP(hipStreamSynchronize(s));
        m.structure_dirty = true;
        E_global_ -= (int)out.size();
    }
    return out;
}

std::vector<Engine::PoseOutliers> Engine::reject_pose_outliers()
{
    Impl& m = *impl_;
    Impl::PoseEdges& pe = m.pe;
    std::vector<PoseOutliers> out(POSE_KIND_COUNT);
    if (m.plan_only || !pe.any_reject())
        return out;
    hipStream_t s = m.ctx.stream;
    const double* poses = m.d_poses[m.last_err_buf].data(); // (the estimates the BA path judges at)
    // the outlier pass over the edges of kind k whose chi2 terms are at d_chi, and the way back to the edge sets through
    // the kind's slot_set / slot_edge (its order on the device)
    auto reject = [&](int k, const double* d_chi) {
        Impl::PoseEdges::Reject& r = pe.rej[k];
        const int n = pe.n_edges(k);
        const std::vector<int32_t>&set_of = pe.kind[k].slot_set, &edge_of = pe.kind[k].slot_edge;
        pe.d_rej_list.resize((size_t)n), pe.d_rej_work.resize(cugo_k::pose_reject_work_ints(n));
        const int32_t* d_count = cugo_k::launch_pose_reject(s, n, d_chi, r.d_threshold.data(), r.n_threshold > 1,
                                                            r.d_flags.data(), pe.d_rej_list.data(), pe.d_rej_work.data());
        int32_t count = 0;
        CUGO_HIP(hipMemcpyAsync(&count, d_count, sizeof count, hipMemcpyDeviceToHost, s));
        CUGO_HIP(hipStreamSynchronize(s));
        if (count <= 0)
            return;
        std::vector<int32_t> list((size_t)count);
        CUGO_HIP(hipMemcpyAsync(list.data(), pe.d_rej_list.data(), sizeof(int32_t) * (size_t)count, hipMemcpyDeviceToHost, s));
        CUGO_HIP(hipStreamSynchronize(s));
        for (int32_t e : list)
        {
            r.h_flags[(size_t)e] |= CUGO_EDGE_INACTIVE;
            out[k].emplace_back(set_of[(size_t)e], edge_of[(size_t)e]);
        }
        std::sort(out[k].begin(), out[k].end());
    };
    m.timed("pose_outliers", [&] {
        // The error passes below overwrite the chi2 totals in the pose-edge scratch (and the ICP partials).  Nothing
        // reads them afterwards: every optimize() starts from a fresh LmState (no speculative pass is pending) with a
        // build pass that writes partials and totals anew, flags included.
        // Per kind: the error pass that leaves the chi2 term of each of its n_pass edges (the two ICP kinds share one,
        // the line edges behind the plane edges; a relative-pose pass writes only the edges that count: the rest stay 0)
        // and where the kind's terms begin in it
        using Pass = std::function<void(double*)>;
        const Pass icp = [&](double* d) { cugo_k::launch_icp_chunks(s, pe.icp, poses, false, pe.icp_rs(), d); };
        const Pass prior = [&](double* d) { cugo_k::launch_prior_errors(s, pe.prior, poses, pe.prior_chi(), d); };
        const Pass relpose = [&](double* d) { cugo_k::launch_relpose_errors(s, pe.relpose, pe.rp.dev, poses, pe.relpose_chi(), d); };
        const int n_plane = pe.icp.n_plane, n_line = pe.icp.n_line;
        const struct
        {
            int kind, n_pass;
            const Pass* pass;
            size_t off;
        } table[] = {{POSE_KIND_PLANE, n_plane + n_line, &icp, 0},
                     {POSE_KIND_LINE, n_plane + n_line, &icp, (size_t)n_plane},
                     {POSE_KIND_PRIOR, pe.n_prior, &prior, 0},
                     {POSE_KIND_RELPOSE, pe.n_relpose_wg ? pe.n_relpose : 0, &relpose, 0}};
        const Pass* ran = nullptr;
        for (const auto& row : table)
        {
            if (!pe.rej[row.kind].on() || !row.n_pass)
                continue;
            if (row.pass != ran)
            {
                pe.d_rej_chi.resize((size_t)row.n_pass);
                pe.d_rej_chi.zero(s);
                (*(ran = row.pass))(pe.d_rej_chi.data());
            }
            reject(row.kind, pe.d_rej_chi.data() + row.off);
        }
    });
    m.collect_times();
    for (const PoseOutliers& k : out)
        E_global_ -= (int)k.size();
    return out;
}

int Engine::n_icp_edges(int kind) const { return kind == 0 || kind == 1 ? impl_->pe.n_edges(kind) : 0; }
const std::vector<int32_t>& Engine::icp_slot_source(int kind, bool set) const
{
    return impl_->pe.icp_slot_source(kind == 1 ? 1 : 0, set);
}
int Engine::n_prior_edges() const { return impl_->pe.n_prior; }
int Engine::n_relpose_edges() const { return impl_->pe.n_relpose; }
int Engine::n_lm_prior_edges() const { return impl_->pe.n_lm_prior; }
int Engine::n_point_edges() const { return impl_->pe.n_point; }
int Engine::flat_point_edges(std::vector<int32_t>& pose, std::vector<int32_t>& src_edge, std::vector<double>& p,
                             std::vector<double>& z, std::vector<double>& info) const
{
    const auto& k = impl_->pe.kind[POSE_KIND_POINT];
    const size_t n = k.h_pose.size();
    pose = k.h_pose, src_edge = k.slot_edge;
    p.assign(k.h_meas.begin(), k.h_meas.begin() + 3 * n); // (meas is planar: p [3][n], then z [3][n])
    z.assign(k.h_meas.begin() + 3 * n, k.h_meas.begin() + 6 * n);
    info = k.h_weight;
    return k.n_weight;
}
int Engine::n_point_pair_edges() const { return impl_->pe.n_pair; }
bool Engine::point_edges_cov() const { return impl_->pe.point_cov; }
bool Engine::point_pair_edges_cov() const { return impl_->pe.pair_cov; }
int Engine::flat_point_pair_edges(std::vector<int32_t>& pose_a, std::vector<int32_t>& pose_b, std::vector<int32_t>& src_edge,
                                  std::vector<double>& p, std::vector<double>& z, std::vector<double>& info) const
{
    const auto& k = impl_->pe.kind[POSE_KIND_PAIR];
    const size_t n = k.h_pose.size();
    pose_a = k.h_pose, pose_b = k.h_pose_b, src_edge = k.slot_edge;
    p.assign(k.h_meas.begin(), k.h_meas.begin() + 3 * n); // (meas is planar: p [3][n], then z [3][n])
    z.assign(k.h_meas.begin() + 3 * n, k.h_meas.begin() + 6 * n);
    info = k.h_weight;
    return k.n_weight;
}
int Engine::n_poses_free() const { return impl_->P; }
int Engine::n_landmarks_free() const { return impl_->L; }

void Engine::clear_covariances()
{
    cov_what_ = 0;
    cov_pose_.clear();
    cov_lm_.clear();
}

// The optimisers both covariance entry points refuse
void Engine::check_covariance_call(const char* who) const
{
    const Impl& m = *impl_;
    const std::string w(who);
    if (m.plan_only)
        throw std::runtime_error(w + ": plan-only optimiser (no HIP device in use)");
    if (m.world > 1 || m.comm)
        throw std::runtime_error(w + ": not available on a sharded (multi-GPU) optimiser");
    if (m.ev.block_f32)
        throw std::runtime_error(w + ": not available in the fp32-internal mode");
}

// What both covariance entry points queue first: H at the current estimates, undamped — the two-stream build pass (Hpp,
// b, Hll, Hpl) as a retried trial of optimize() queues it —, its Schur complement and one factorisation at lambda = 0.
// optimize() starts every call with a build pass of its own, so nothing it reads is lost.
void Engine::queue_covariance_system()
{
    Impl& m = *impl_;
    if (m.structure_dirty)
        build_structure();
    hipStream_t s = m.ctx.stream;
    if ((m.pe.n_relpose || m.pe.n_pair) && m.pe.rp.plan_dirty)
    {
        m.join_pattern(); // (the helper of initialize() writes the host pattern)
        m.pe.bind_relpose_plan(m.hsc_rowptr, m.hsc_colind, s, false);
    }
    m.begin_call(false);
    m.queue_build(m.cur, -1.0);
    if (m.P > 0)
    {
        m.queue_schur(0.0, false, false, m.cur);
        m.queue_factor_solve(0.0);
    }
}

bool Engine::compute_covariances(int what)
{
    Impl& m = *impl_;
    if (what < 1 || what > 3)
        throw std::invalid_argument("cugo_graph_compute_covariances: what must be 1 (poses), 2 (landmarks) or 3 (both)");
    check_covariance_call("cugo_graph_compute_covariances");
    clear_covariances();
    queue_covariance_system();
    hipStream_t s = m.ctx.stream;
    const int B = m.hs.n_blocks;
    m.d_cov_sigma.resize(36 * (size_t)B + 16);
    if (m.P > 0 && !m.chol.selected_inverse(m.d_cov_sigma.data()))
        return false;
    std::vector<int32_t> fail(1, 0);
    if (what & 2)
    {
        m.d_cov_lm.resize(9 * (size_t)m.L + 16);
        m.d_cov_fail.resize(16);
        m.d_cov_fail.zero(s);
        cugo_k::launch_lm_covariance(s, m.L, m.ev.d_lm_ptr, m.ev.d_pose, m.ev.d_flags, m.d_Hll.data(),
                                     reinterpret_cast<const double*>(m.d_Hpl.data()), m.hs.d_rowptr, m.hs.d_colind,
                                     m.d_cov_sigma.data(), m.d_cov_lm.data(), m.d_cov_fail.data());
        cov_lm_.resize(9 * (size_t)m.L);
        if (m.L > 0)
            CUGO_HIP(hipMemcpyAsync(cov_lm_.data(), m.d_cov_lm.data(), cov_lm_.size() * sizeof(double),
                                    hipMemcpyDeviceToHost, s));
        CUGO_HIP(hipMemcpyAsync(fail.data(), m.d_cov_fail.data(), sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    // the diagonal blocks of the poses, gathered on the device: only they travel to the host
    if ((what & 1) && m.P > 0)
    {
        m.d_cov_pose.resize(36 * (size_t)m.P + 16);
        cugo_k::launch_cov_pose_diag(s, m.P, m.hs.d_rowptr, m.d_cov_sigma.data(), m.d_cov_pose.data());
        cov_pose_.resize(36 * (size_t)m.P);
        CUGO_HIP(hipMemcpyAsync(cov_pose_.data(), m.d_cov_pose.data(), cov_pose_.size() * sizeof(double),
                                hipMemcpyDeviceToHost, s));
    }
    CUGO_HIP(hipStreamSynchronize(s));
    if (fail[0])
    {
        clear_covariances();
        return false;
    }
    if (!(what & 1))
        cov_pose_.clear();
    cov_what_ = what;
    return true;
}

// Sigma_ab of the pairs (ia[k], ib[k]) of free pose indices (-1: a fixed pose, the block is zero) through
// cugo_chol::inverse_blocks on the same factorisation compute_covariances() runs; the stored marginals stay.
bool Engine::pose_cross_covariances(int n, const int32_t* ia, const int32_t* ib, double* cov36)
{
    Impl& m = *impl_;
    check_covariance_call("cugo_graph_compute_pose_cross_covariances");
    std::vector<int32_t> ra, rb, where;
    for (int k = 0; k < n; k++)
        if (ia[k] >= 0 && ib[k] >= 0)
        {
            if (ia[k] >= m.P || ib[k] >= m.P)
                throw std::invalid_argument("cugo_graph_compute_pose_cross_covariances: pose index out of range");
            ra.push_back(ia[k]), rb.push_back(ib[k]), where.push_back(k);
        }
    std::fill(cov36, cov36 + 36 * (size_t)n, 0.0);
    if (ra.empty()) // (every pair holds a fixed pose: nothing to factor)
        return true;
    queue_covariance_system();
    hipStream_t s = m.ctx.stream;
    m.d_xcov.resize(36 * ra.size() + 16);
    if (!m.chol.inverse_blocks((int)ra.size(), ra.data(), rb.data(), m.d_xcov.data()))
        return false;
    std::vector<double> h(36 * ra.size());
    CUGO_HIP(hipMemcpyAsync(h.data(), m.d_xcov.data(), h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    CUGO_HIP(hipStreamSynchronize(s));
    for (size_t q = 0; q < where.size(); q++)
        std::copy(h.begin() + 36 * q, h.begin() + 36 * q + 36, cov36 + 36 * (size_t)where[q]);
    return true;
}

// The plan needs the pose of every slot on the host: the engine keeps the slot arrays of the flattening (slots.pose,
// what d_e_pose was uploaded from; build_structure() reads it too), so nothing is downloaded.
bool Engine::queue_pose_lm_cross(int n, const int32_t* qp, const int32_t* ql, const std::vector<int32_t>& extra,
                                 size_t off[6])
{
    Impl& m = *impl_;
    PlCovPlanHost plan;
    build_plcov_plan(m.P, m.L, m.h_lm_ptr.data(), m.slots.pose.data(), n, qp, ql, plan);
    queue_covariance_system();
    hipStream_t s = m.ctx.stream;
    m.d_pl_blocks.resize(36 * plan.rows.size() + 16);
    if (!plan.rows.empty() &&
        !m.chol.inverse_blocks((int)plan.rows.size(), plan.rows.data(), plan.cols.data(), m.d_pl_blocks.data()))
        return false;
    std::vector<int32_t>& h = m.h_pl_idx; // (pageable: it lives until the caller's synchronisation)
    h.clear();
    auto put = [&h](const int32_t* p, size_t k) {
        const size_t at = h.size();
        h.insert(h.end(), p, p + k);
        return at;
    };
    off[0] = put(qp, (size_t)n), off[1] = put(ql, (size_t)n);
    off[2] = put(plan.q_ptr.data(), plan.q_ptr.size()), off[3] = put(plan.q_slot.data(), plan.q_slot.size());
    off[4] = put(plan.q_aa.data(), plan.q_aa.size()), off[5] = put(extra.data(), extra.size());
    m.d_pl_idx.upload(h, s);
    m.d_pl_cross.resize(18 * (size_t)n + 16);
    m.d_cov_fail.resize(16);
    m.d_cov_fail.zero(s);
    const int32_t* ix = m.d_pl_idx.data();
    cugo_k::launch_pose_lm_cross(s, n, ix + off[0], ix + off[1], ix + off[2], ix + off[3], m.ev.d_lm_ptr, m.ev.d_flags,
                                 m.d_Hll.data(), reinterpret_cast<const double*>(m.d_Hpl.data()), m.d_pl_blocks.data(),
                                 m.d_pl_cross.data(), m.d_cov_fail.data() + 1);
    return true;
}

bool Engine::pose_landmark_cross_covariances(int n, const int32_t* ia, const int32_t* il, double* cov18)
{
    Impl& m = *impl_;
    const char* who = "cugo_graph_compute_pose_landmark_cross_covariances";
    check_covariance_call(who);
    bool any = false;
    for (int k = 0; k < n; k++)
    {
        if (ia[k] < -1 || ia[k] >= m.P || il[k] < -1 || il[k] >= m.L)
            throw std::invalid_argument(std::string(who) + ": vertex index out of range");
        any = any || il[k] >= 0; // (a free landmark is looked at under a fixed pose too: its Hll must factor)
    }
    std::fill(cov18, cov18 + 18 * (size_t)n, 0.0);
    if (!any) // (every query holds a fixed landmark: nothing to factor)
        return true;
    size_t off[6];
    if (!queue_pose_lm_cross(n, ia, il, {}, off))
        return false;
    hipStream_t s = m.ctx.stream;
    int32_t fail = 0;
    CUGO_HIP(hipMemcpyAsync(cov18, m.d_pl_cross.data(), 18 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    CUGO_HIP(hipMemcpyAsync(&fail, m.d_cov_fail.data() + 1, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CUGO_HIP(hipStreamSynchronize(s));
    if (fail)
        std::fill(cov18, cov18 + 18 * (size_t)n, 0.0);
    return !fail;
}

// What reprojection_covariances and predict_observations queue before their own kernel: the vertex indices of the
// flattening as the kernel reads them, with `third` (a dim or a kind) per query behind them, Sigma_aa and Sigma_al
// (queue_pose_lm_cross) and Sigma_ll of every free landmark on the same factorisation.  1: queued; 0: both vertices of
// every query are fixed, nothing was queued; -1: a zero pivot
int Engine::queue_joint_covariances(const char* who, int n, const int32_t* ia, const int32_t* il, int third, size_t off[6])
{
    Impl& m = *impl_;
    std::vector<int32_t> qp((size_t)n), ql((size_t)n), extra(3 * (size_t)n);
    bool any = false, any_lm = false;
    for (int k = 0; k < n; k++)
    {
        if (ia[k] < 0 || ia[k] >= m.Pall || il[k] < 0 || il[k] >= m.Lall)
            throw std::invalid_argument(std::string(who) + ": vertex index out of range");
        qp[k] = ia[k] < m.P ? ia[k] : -1, ql[k] = il[k] < m.L ? il[k] : -1;
        extra[k] = ia[k], extra[(size_t)n + k] = il[k], extra[2 * (size_t)n + k] = third;
        any = any || qp[k] >= 0 || ql[k] >= 0;
        any_lm = any_lm || ql[k] >= 0;
    }
    if (!any)
        return 0;
    if (!queue_pose_lm_cross(n, qp.data(), ql.data(), extra, off))
        return -1;
    hipStream_t s = m.ctx.stream;
    // Sigma_ll of every free landmark on the same factorisation; whether one of them fails is the first kernel's call
    m.d_cov_lm.resize(9 * (size_t)m.L + 16);
    if (any_lm)
    {
        m.d_cov_sigma.resize(36 * (size_t)m.hs.n_blocks + 16);
        if (m.P > 0 && !m.chol.selected_inverse(m.d_cov_sigma.data()))
            return -1;
        cugo_k::launch_lm_covariance(s, m.L, m.ev.d_lm_ptr, m.ev.d_pose, m.ev.d_flags, m.d_Hll.data(),
                                     reinterpret_cast<const double*>(m.d_Hpl.data()), m.hs.d_rowptr, m.hs.d_colind,
                                     m.d_cov_sigma.data(), m.d_cov_lm.data(), m.d_cov_fail.data());
    }
    return 1;
}

// the 3 x 3 blocks of m.d_pl_out to the host with the fail flag of k_pose_lm_cross (read only where one was queued);
// false, nothing copied: the flag is set
bool Engine::fetch_joint_covariances(int n, bool flagged, std::vector<double>& h)
{
    Impl& m = *impl_;
    hipStream_t s = m.ctx.stream;
    h.resize(9 * (size_t)n);
    int32_t fail = 0;
    CUGO_HIP(hipMemcpyAsync(h.data(), m.d_pl_out.data(), h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    if (flagged)
        CUGO_HIP(hipMemcpyAsync(&fail, m.d_cov_fail.data() + 1, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CUGO_HIP(hipStreamSynchronize(s));
    return !fail;
}

bool Engine::reprojection_covariances(int n, const int32_t* ia, const int32_t* il, int dim, const double* cam5, double* cov)
{
    Impl& m = *impl_;
    const char* who = "cugo_graph_reprojection_covariances";
    check_covariance_call(who);
    if (dim != 2 && dim != 3)
        throw std::invalid_argument(std::string(who) + ": dim must be 2 (mono) or 3 (stereo)");
    const size_t dd = (size_t)dim * dim;
    std::fill(cov, cov + dd * (size_t)n, 0.0);
    size_t off[6];
    const int queued = queue_joint_covariances(who, n, ia, il, dim, off);
    if (queued <= 0) // (both vertices of every query are fixed, or a zero pivot)
        return queued == 0;
    hipStream_t s = m.ctx.stream;
    m.d_pl_cam.upload(cam5, 5 * (size_t)n, s);
    m.d_pl_out.resize(9 * (size_t)n + 16);
    const int32_t* ix = m.d_pl_idx.data();
    cugo_k::launch_reprojection_cov(s, n, m.L, ix + off[5], ix + off[5] + n, ix + off[5] + 2 * (size_t)n, ix + off[4],
                                    m.d_pl_cam.data(), m.d_poses[m.cur].data(), m.d_lms[m.cur].data(), m.d_pl_blocks.data(),
                                    m.d_pl_cross.data(), m.d_cov_lm.data(), m.d_pl_out.data());
    std::vector<double> h;
    if (!fetch_joint_covariances(n, true, h))
        return false;
    for (int k = 0; k < n; k++)
        for (int c = 0; c < dim; c++)
            for (int r = 0; r < dim; r++)
                cov[dd * (size_t)k + r + (size_t)dim * c] = h[9 * (size_t)k + r + 3 * c];
    return true;
}

bool Engine::predict_observations(int n, const int32_t* ia, const int32_t* il, int kind, const double* cam5,
                                  const double* cam_tab, double* z, double* cov)
{
    Impl& m = *impl_;
    const char* who = "cugo_graph_predict_observations";
    check_covariance_call(who);
    if (kind != CUGO_OBS_MONO && kind != CUGO_OBS_STEREO && kind != CUGO_OBS_DEPTH)
        throw std::invalid_argument(std::string(who) + ": kind must be 2 (mono), 3 (stereo) or 4 (depth)");
    const int dim = kind == CUGO_OBS_MONO ? 2 : 3;
    const size_t dd = (size_t)dim * dim;
    std::fill(z, z + (size_t)dim * n, 0.0);
    std::fill(cov, cov + dd * (size_t)n, 0.0);
    if (n == 0)
        return true;
    size_t off[6];
    const int queued = queue_joint_covariances(who, n, ia, il, kind, off);
    if (queued < 0)
        return false;
    hipStream_t s = m.ctx.stream;
    if (queued == 0)
    {
        // both vertices of every query are fixed: no system is built, and of the covariance inputs the kernel reads none
        // (q_aa = -1, every landmark index >= L) — z still needs the indices on the device
        std::vector<int32_t>& h = m.h_pl_idx;
        h.assign(ia, ia + n);
        h.insert(h.end(), il, il + n);
        h.insert(h.end(), (size_t)n, kind);
        h.insert(h.end(), (size_t)n, -1);
        m.d_pl_idx.upload(h, s);
        off[5] = 0, off[4] = 3 * (size_t)n;
        m.d_pl_blocks.resize(16), m.d_pl_cross.resize(16), m.d_cov_lm.resize(16);
    }
    m.d_pl_cam.upload(cam5, 5 * (size_t)n, s);
    if (cam_tab)
        m.d_pl_tab.upload(cam_tab, 17 * (size_t)n, s);
    m.d_pl_out.resize(9 * (size_t)n + 16);
    m.d_pl_z.resize(3 * (size_t)n + 16);
    const int32_t* ix = m.d_pl_idx.data();
    cugo_k::launch_predict_obs(s, n, m.L, ix + off[5], ix + off[5] + n, ix + off[5] + 2 * (size_t)n, ix + off[4],
                               m.d_pl_cam.data(), cam_tab ? m.d_pl_tab.data() : nullptr, m.d_poses[m.cur].data(),
                               m.d_lms[m.cur].data(), m.d_pl_blocks.data(), m.d_pl_cross.data(), m.d_cov_lm.data(),
                               m.d_pl_z.data(), m.d_pl_out.data());
    std::vector<double> hz(3 * (size_t)n), h;
    CUGO_HIP(hipMemcpyAsync(hz.data(), m.d_pl_z.data(), hz.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    if (!fetch_joint_covariances(n, queued > 0, h))
        return false;
    for (int k = 0; k < n; k++)
    {
        for (int r = 0; r < dim; r++)
            z[(size_t)dim * k + r] = hz[3 * (size_t)k + r];
        for (int c = 0; c < dim; c++)
            for (int r = 0; r < dim; r++)
                cov[dd * (size_t)k + r + (size_t)dim * c] = h[9 * (size_t)k + r + 3 * c];
    }
    return true;
}

void Engine::download(std::vector<double>& poses, std::vector<double>& lms)
{
    Impl& m = *impl_;
    hipStream_t s = m.ctx.stream;
    poses.resize(7 * (size_t)m.Pall);
    lms.resize(3 * (size_t)m.Lall);
    if (m.world > 1 && m.L > 0)
    {
        // landmark estimates live on their owner: zero the others and sum over ranks
        std::vector<double> own(3 * (size_t)m.Lall, 0.0), cur(3 * (size_t)m.Lall);
        CUGO_HIP(hipMemcpyAsync(cur.data(), m.d_lms[m.cur].data(), cur.size() * sizeof(double),
                                hipMemcpyDeviceToHost, s));
        CUGO_HIP(hipStreamSynchronize(s));
        // ownership = the shard's landmark range (ranges partition [0, Lall))
        for (int l = m.shard_l0; l < m.shard_l1; l++)
            for (int k = 0; k < 3; k++)
                own[3 * (size_t)l + k] = cur[3 * (size_t)l + k];
        // NOTE: edges of a landmark never straddle shards (cuts are at landmark boundaries)
        CUGO_HIP(hipMemcpyAsync(m.d_lms[m.cur ^ 1].data(), own.data(), own.size() * sizeof(double),
                                hipMemcpyHostToDevice, s));
        m.exchange(m.d_lms[m.cur ^ 1].data(), own.size(), 0);
        CUGO_HIP(hipMemcpyAsync(lms.data(), m.d_lms[m.cur ^ 1].data(), lms.size() * sizeof(double),
                                hipMemcpyDeviceToHost, s));
    }
    else if (!lms.empty())
        CUGO_HIP(hipMemcpyAsync(lms.data(), m.d_lms[m.cur].data(), lms.size() * sizeof(double),
                                hipMemcpyDeviceToHost, s));
    if (!poses.empty())
        CUGO_HIP(hipMemcpyAsync(poses.data(), m.d_poses[m.cur].data(), poses.size() * sizeof(double),
                                hipMemcpyDeviceToHost, s));
    CUGO_HIP(hipStreamSynchronize(s));
    if (m.world > 1)
    { // keep both buffers consistent for a following initialize-less optimize()
        CUGO_HIP(hipMemcpyAsync(m.d_lms[m.cur].data(), lms.data(), lms.size() * sizeof(double),
                                hipMemcpyHostToDevice, s));
        CUGO_HIP(hipMemcpyAsync(m.d_lms[m.cur ^ 1].data(), lms.data(), lms.size() * sizeof(double),
                                hipMemcpyHostToDevice, s));
        CUGO_HIP(hipStreamSynchronize(s));
    }
}

} // namespace cugo_host
