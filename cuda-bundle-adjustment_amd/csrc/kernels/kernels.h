// Host-callable launchers of the HIP kernels (internal; the public surface is include/cugo_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../../include/cugo_hip.h"

namespace cugo_k
{

// Optional per-kernel timing hook: when installed, every kernel launch of the library is
// bracketed by begin(name)/end(name) (the engine records HIP events on the launch stream).
struct LaunchHook
{
    virtual void begin(const char* kernel, hipStream_t s) = 0;
    virtual void end(const char* kernel, hipStream_t s) = 0;
    virtual ~LaunchHook() {}
};
void set_launch_hook(LaunchHook* h); // nullptr = off (default)
LaunchHook* launch_hook();
struct LaunchScope
{
    const char* name;
    hipStream_t s;
    LaunchHook* h;
    LaunchScope(const char* n, hipStream_t st) : name(n), s(st), h(launch_hook())
    {
        if (h)
            h->begin(name, s);
    }
    ~LaunchScope()
    {
        if (h)
            h->end(name, s);
    }
};
// launch + per-kernel timing scope
#define CUGO_LAUNCH(kernel, grid, block, lds, stream, ...)                          \
    do                                                                              \
    {                                                                               \
        ::cugo_k::LaunchScope _scope(#kernel, stream);                              \
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);          \
    } while (0)

// scratch for deterministic two-stage reductions: partial sums per workgroup
struct ReduceScratch
{
    double* d_partials; // capacity doubles
    size_t capacity;
};
// where a pass of a chunked pose edge kind (pose_chunks.h: ICP, point, point pair) leaves its partials and its one
// chi2 total per chunk: behind one another in one scratch (*_scratch_in, which checks the capacity: the kernel-level C
// ABI, and the ICP kinds everywhere), or the totals elsewhere (the LM loop keeps them beside the other kinds' totals)
struct ChunkScratch
{
    double* d_part;
    double* d_cchi;
};

// --- edge / landmark / pose passes (ba_kernels.hip) ---------------------------------------
// The form of an edge view: which instantiation of its kernel every launcher below that forms residuals or Jacobians
// (launch_errors*, launch_edge_chi, launch_build, launch_schur's pose pass, launch_backsubst_update from records) picks,
// and what it takes from ev for it (ba_kernels.hip: with_form, the one place).  In this order of precedence:
//   Distortion  ev.has_rig == CUGO_RIG_DISTORTION: ev.d_cam_ext is the distortion table [n_cams][18] (section 20)
//   Models  ev.has_rig == CUGO_RIG_MODELS: ev.d_cam_ext is the model table [n_cams][17]
//   Rig     any other ev.has_rig != 0: ev.d_cam_ext holds the extrinsics [n_cams][12], parallel to ev.d_cams (section 18)
//   Depth   ev.has_depth != 0: slots may carry CUGO_EDGE_DEPTH; the depth kind's robust kernel and sqrt(ev.depth_weight)
//           come from ev (section 17)
//   Plain   the kernels, and their arguments, are the ones there have always been
// A table never goes together with ev.has_depth, and the caller has checked the members (c_api.cpp: check_edge_form;
// the engine's come from initialize(), which refuses such a graph).
enum class EdgeForm
{
    Plain,
    Depth,
    Rig,
    Models,
    Distortion
};
EdgeForm edge_form(const cugo_edges& ev);
void launch_errors(hipStream_t s, const cugo_edges& ev, const double* d_poses, const double* d_lms,
                   cugo_robust rk, ReduceScratch rs, double* d_chi);

// d_Hpl / d_T below: double [E][18], or float [E][18] when ev.block_f32 is set
// fuse_lambda >= 0 with d_invHll and d_T given: the pass also leaves invHll = (Hll + lambda I)^-1 and
// T = Hpl invHll (what launch_schur's edge kernel computes; pass have_T = true there).  Only for slot
// layouts that keep every landmark's edges inside one 256-slot group (the engine's).
// With d_lmrec as well (16 doubles per free landmark) the pass writes ONE block stream instead: G = Hpl L^-T into d_T
// (Hll + lambda I = L L^T), the line {L^-1 (6), L^-1 bl (3)} of every landmark into d_lmrec, and neither d_Hpl nor
// d_invHll; skip_poses then also leaves out the pose pass (d_Hpp, d_bp).  launch_schur and launch_backsubst_update take
// the same d_lmrec and d_T for that form (SchurRows::d_lmrec).
// chi_behind_scale: the chi2 partials of the pass go behind the scale partials of the update pass in the scratch, for
// launch_trial_tail_from_build.
// lm_priors (optional; nullptr or n == 0: the pass as it is without them, the same instantiation with the same
// arguments): landmark position priors (lm_prior_kernels.hip).  The owner lane of every free landmark adds the
// landmark's priors, in sorted order, behind the landmark's edges and before Hll / bl are stored, factored or inverted:
// Hll, bl, invHll, T, G and the landmarks' lines all carry them.  The chi2 of the pass stays that of the BA edges.
void launch_build(hipStream_t s, const cugo_edges& ev, const double* d_poses, const double* d_lms,
                  cugo_robust rk, double* d_Hpp, double* d_bp, double* d_Hll, double* d_bl,
                  void* d_Hpl, ReduceScratch rs, double* d_chi, double fuse_lambda = -1.0,
                  double* d_invHll = nullptr, void* d_T = nullptr, double* d_lmrec = nullptr, bool skip_poses = false,
                  bool chi_behind_scale = false, const cugo_lm_prior_edges* lm_priors = nullptr);

// the reductions that end a trial, with the chi2 partials of a build pass queued with chi_behind_scale (ba_kernels.hip)
// d_icp_chi / n_icp_chi (both tails): chi2 totals of the chunks of an ICP pass at the trial's estimates (icp_chunk_count),
// summed in their order and added to F-hat by the same launch; nullptr / 0: no such edges
void launch_trial_tail_from_build(hipStream_t s, const cugo_edges& ev, ReduceScratch rs, int n_scale_partials,
                                  double* d_out, const double* d_flag, double* h_out, double seq, unsigned* d_done,
                                  const double* d_icp_chi = nullptr, int n_icp_chi = 0);

void launch_max_diagonal(hipStream_t s, const double* d_Hpp, int nP, const double* d_Hll, int nL,
                         ReduceScratch rs, double* d_out);

// SchurRows (optional): the per-entry records of the pose-major edge list (launch_pose_rec) and the longest
// block row of Hsc.  Given, the H-side and b-side of the Schur complement run as ONE kernel that forms the
// whole block row of a pose (k_hsc_rows): T = Hpl invHll is never written or read (d_T may be NULL) and the
// product lists of hs are not used; have_T then means "d_invHll already holds (Hll + lambda I)^-1".
struct SchurRows
{
    const int32_t* d_pose_rec = nullptr; // [n][4]: slot, end of its landmark's slots, landmark, flags
    int max_row_nnz = 0;
    // row-strip form of the gather kernels (k_hsc_offdiag_strip): per product, the position of its T edge in
    // the edge list of its pose (launch_list_pos).  Given, the off-diagonal blocks are formed one block row per
    // workgroup with the row's T blocks staged in LDS once; same sums, bit for bit
    const int32_t* d_off_pi = nullptr;
    // which form of the H-side gather kernels (Options::hsc_mfma / hsc_xcd, read once per context / optimiser):
    // 1 both on the matrix cores, 2 only the off-diagonal one, 0 the vector-lane kernels; blocks dealt to the XCDs
    // in contiguous ranges or in dispatch order
    int mfma = 1;
    bool xcd = true;
    // fused iteration in the one-stream form (launch_build with d_lmrec and skip_poses for this lambda: d_T holds G):
    // the off-diagonal kernel takes both operands from d_T, and k_pose_schur forms the diagonal blocks, bp (d_bp_out) and
    // bsc from the build pass's records, the landmarks' lines and the poses the pass linearised at (d_poses)
    const double* d_lmrec = nullptr;
    const double* d_poses = nullptr;
    ReduceScratch rs{nullptr, 0};
    double* d_bp_out = nullptr;
};
// d_pose_pos [n_edges] scratch/out: position of every slot in its pose's list; d_off_pi [M] out
void launch_list_pos(hipStream_t s, const cugo_edges& ev, int n_list, size_t M, const int32_t* d_off_ei,
                     int32_t* d_pose_pos, int32_t* d_off_pi);
void launch_pose_rec(hipStream_t s, const cugo_edges& ev, int n, int32_t* d_rec);
// false: the row kernel cannot take this structure (no pattern on the device, or a block row too long for
// its LDS accumulators): launch_schur then runs the gather kernels, which need d_T
bool schur_rows_usable(const cugo_hsc_struct& hs, int max_row_nnz);
void launch_schur(hipStream_t s, const cugo_edges& ev, const cugo_hsc_struct& hs, double lambda,
                  int damp_hsc_diag, const double* d_Hpp, const double* d_bp, const double* d_Hll,
                  const double* d_bl, const void* d_Hpl, double* d_invHll, void* d_T,
                  double* d_bsc, double* d_Hsc, bool have_T = false, SchurRows rows = SchurRows());

// lambda_pose: damping used in the pose part of the scale sum (0 on ranks > 0 of a sharded run
// so that the all-reduced scale counts lambda*|xp|^2 once)
// d_scale == nullptr: the scale partials are left in the scratch (launch_errors_tail sums them);
// returns their number
int launch_backsubst_update(hipStream_t s, const cugo_edges& ev, double lambda, double lambda_pose,
                            const double* d_invHll, const double* d_bl, const double* d_bp,
                            const void* d_Hpl, const double* d_xp, double* d_xl,
                            const double* d_poses_in, const double* d_lms_in, double* d_poses_out,
                            double* d_lms_out, ReduceScratch rs, double* d_scale,
                            const double* d_lmrec = nullptr, // d_lmrec: d_Hpl holds G, see k_backsubst_landmarks
                            bool from_records = false);
// from_records (only with d_lmrec): the kernel re-forms G_e^T dx_p from the 64-byte records the build pass left in the
// scratch `rs`, the poses it linearised at (d_poses_in) and the landmarks' lines instead of reading the 144-byte G
// blocks — the same bits.  The records live from a build pass until the first error pass behind it
// (launch_errors_tail parks its chi2 partials in their area): the caller vouches that none has run since the build
// pass that wrote d_lmrec and G.
// error pass of an LM trial + BOTH final reductions in one launch: d_out[0] = chi2, d_out[1] = scale
// (from the n_scale_partials left by launch_backsubst_update); h_out (pinned host memory, may be
// null) receives {chi2, scale, the 8 bytes at d_flag}: readable after the stream has been waited for
void launch_errors_tail(hipStream_t s, const cugo_edges& ev, const double* d_poses, const double* d_lms,
                        cugo_robust rk, ReduceScratch rs, int n_scale_partials, double* d_out,
                        const double* d_flag, double* h_out, double seq, unsigned* d_done,
                        const double* d_icp_chi = nullptr, int n_icp_chi = 0);

size_t reduce_scratch_doubles(int n_edges, int n_poses, int n_landmarks);

// --- shared by the unary pose edge kinds (pose_edge_kernels.hip) ---------------------------
// the sum of n chi2 totals (ICP chunks, prior workgroups), in their order, to d_chi[0] (added to what is there with
// chi_add), in a launch of its own under `label`
void launch_pose_chi_total(hipStream_t s, const char* label, const double* d_totals, int n, double* d_chi, bool chi_add);
// with pose_ptr known to ascend from 0 to n per kind: 1 if an edge of a kind does not lie in its pose's pose_ptr range
// (the edges are not sorted by pose, or a pose index is out of range), else 0.  One launch per non-empty kind under
// its label; d_bad: a device int for the flag.  Synchronises the stream.  `who` names the caller in the message
struct PoseIndexCheck
{
    const int32_t *d_pose, *d_pose_ptr;
    int n;
    const char* label;
};
int pose_check_indices(hipStream_t s, const char* who, const PoseIndexCheck* kinds, int n_kinds, int n_poses_total, int* d_bad);
// Outlier pass of the four pose edge kinds (include/cugo_hip.h: cugo_pose_edges_reject): edge e goes iff it is not
// flagged CUGO_EDGE_INACTIVE, its threshold (d_threshold[per_edge ? e : 0]) is > 0 and d_edge_chi[e] > threshold.  Its
// flag byte gains the bit and d_rejected receives the indices, ascending.  Three launches (count, scan, place) and no
// synchronisation; d_work: pose_reject_work_ints(n) ints of scratch.  Returns the device address of the count (inside
// d_work), or nullptr when nothing was launched (n == 0).  A workgroup walks a contiguous run of edges; beyond
// pose_reject_grid_cap() workgroups of 256 edges each walks several tiles.
size_t pose_reject_work_ints(int n);
int pose_reject_grid_cap();
const int32_t* launch_pose_reject(hipStream_t s, int n, const double* d_edge_chi, const double* d_threshold, bool per_edge,
                                  uint8_t* d_flags, int32_t* d_rejected, int32_t* d_work);

// --- point-to-plane / point-to-line pose edges (icp_kernels.hip) -------------------------
// scratch the launchers need: [plane partials | line partials | one chi2 total per chunk, plane chunks then line chunks
// (icp_chunk_count() of them: what launch_errors_tail / launch_trial_tail_from_build sum into F-hat)]
size_t icp_scratch_doubles(const cugo_icp_edges& ev);
int icp_chunk_count(const cugo_icp_edges& ev);
ChunkScratch icp_scratch_in(ReduceScratch rs, const cugo_icp_edges& ev);
// ADDS the ICP terms to d_Hpp / d_bp; chi2 total to d_chi[0] if given (added to what is there with chi_add)
void launch_icp_build(hipStream_t s, const cugo_icp_edges& ev, const double* d_poses, double* d_Hpp, double* d_bp,
                      ChunkScratch rs, double* d_chi, bool chi_add = false);
// chi2 only (the same bits as launch_icp_build's); d_edge_chi: per edge, plane edges first, or nullptr
void launch_icp_errors(hipStream_t s, const cugo_icp_edges& ev, const double* d_poses, ChunkScratch rs, double* d_chi,
                       bool chi_add = false, double* d_edge_chi = nullptr);
// The pieces of the two above, for the LM loop (engine.cpp), which places them itself:
// the chunk pass alone — full: the partials of H, b and chi2 of every (chunk, pose) pair; otherwise chi2 only — leaves
// its partials and the chi2 total of every chunk in the scratch
void launch_icp_chunks(hipStream_t s, const cugo_icp_edges& ev, const double* d_poses, bool full, ChunkScratch rs,
                       double* d_edge_chi = nullptr);
// the per-pose sums of a full chunk pass ADDED to d_Hpp / d_bp (behind k_build_poses) ...
void launch_icp_add(hipStream_t s, const cugo_icp_edges& ev, ChunkScratch rs, double* d_Hpp, double* d_bp);
// ... or to the diagonal blocks of d_Hsc (upper block CSR d_rowptr: the first block of a row), d_bp and d_bsc (behind
// k_pose_schur, which writes the three in the one-stream form)
void launch_icp_add_schur(hipStream_t s, const cugo_icp_edges& ev, ChunkScratch rs, const int32_t* d_rowptr,
                          double* d_Hsc, double* d_bp, double* d_bsc);
// the sum of the chunk totals to d_chi[0]
void launch_icp_chi_total(hipStream_t s, const cugo_icp_edges& ev, ChunkScratch rs, double* d_chi, bool chi_add);

// --- point-to-point pose edges with 3 x 3 information (point_kernels.hip) -----------------
// The launchers of the ICP kinds, for the one kind of cugo_point_edges.  A pass leaves its partials (point_partial_doubles()
// doubles) and one chi2 total per chunk (point_chunk_count()) where its ChunkScratch says
size_t point_scratch_doubles(const cugo_point_edges& ev); // partials + totals
size_t point_partial_doubles(const cugo_point_edges& ev);
int point_chunk_count(const cugo_point_edges& ev);
ChunkScratch point_scratch_in(ReduceScratch rs, const cugo_point_edges& ev);
// The covariance form (cugo_gicp_edges) runs through the same launchers: with d_cov_z the chunk pass is the covariance
// instantiation, which reads ev.d_info as cov_p and ev.n_info as the count of both covariances.
// ADDS the terms to d_Hpp / d_bp; chi2 total to d_chi[0] if given (added to what is there with chi_add)
void launch_point_build(hipStream_t s, const cugo_point_edges& ev, const double* d_poses, double* d_Hpp, double* d_bp,
                        ChunkScratch rs, double* d_chi, bool chi_add = false, const double* d_cov_z = nullptr);
// chi2 only (the same bits as launch_point_build's); d_edge_chi: per edge, or nullptr
void launch_point_errors(hipStream_t s, const cugo_point_edges& ev, const double* d_poses, ChunkScratch rs, double* d_chi,
                         bool chi_add = false, double* d_edge_chi = nullptr, const double* d_cov_z = nullptr);
// the pieces: the chunk pass alone, the per-pose sums ADDED to d_Hpp / d_bp or to the Schur destination, the chi2 total
void launch_point_chunks(hipStream_t s, const cugo_point_edges& ev, const double* d_poses, bool full, ChunkScratch rs,
                         double* d_edge_chi = nullptr, const double* d_cov_z = nullptr);
void launch_point_add(hipStream_t s, const cugo_point_edges& ev, ChunkScratch rs, double* d_Hpp, double* d_bp);
void launch_point_add_schur(hipStream_t s, const cugo_point_edges& ev, ChunkScratch rs, const int32_t* d_rowptr,
                            double* d_Hsc, double* d_bp, double* d_bsc);
void launch_point_chi_total(hipStream_t s, const cugo_point_edges& ev, ChunkScratch rs, double* d_chi, bool chi_add);

// --- SE(3) pose priors with 6 x 6 information (prior_kernels.hip) --------------------------
// One kernel per pass: 32 lanes per free pose walk its priors in container order and ADD their sums straight to the
// destination; every workgroup leaves one chi2 total in d_wg_chi [prior_workgroups()].  The LM loop appends these
// totals to the ICP chunk totals (icp_chunk_count), so that the launch ending a trial sums them as well.
int prior_workgroups(const cugo_prior_edges& ev); // 0 without edges or free poses: nothing is launched
// chi2 only; d_edge_chi [n] (sorted order, 0 for edges that do not count) or nullptr
void launch_prior_errors(hipStream_t s, const cugo_prior_edges& ev, const double* d_poses, double* d_wg_chi,
                         double* d_edge_chi = nullptr);
// the terms ADDED to d_Hpp / d_bp (behind k_build_poses) ...
void launch_prior_add(hipStream_t s, const cugo_prior_edges& ev, const double* d_poses, double* d_Hpp, double* d_bp,
                      double* d_wg_chi);
// ... or to the diagonal blocks of d_Hsc (upper block CSR d_rowptr: the first block of a row), d_bp and d_bsc (behind
// k_pose_schur, which writes the three in the one-stream form)
void launch_prior_add_schur(hipStream_t s, const cugo_prior_edges& ev, const double* d_poses, const int32_t* d_rowptr,
                            double* d_Hsc, double* d_bp, double* d_bsc, double* d_wg_chi);

// --- landmark position priors with 3 x 3 information (lm_prior_kernels.hip) -----------------
// One lane per free landmark walks its priors in sorted order; every 256-lane workgroup leaves one chi2 total in
// d_wg_chi [lm_prior_workgroups()], its lanes in order.  The LM loop places these totals behind the relative-pose
// totals; the terms themselves it takes inside the build pass (launch_build with lm_priors).
int lm_prior_workgroups(const cugo_lm_prior_edges& ev); // 0 without priors or free landmarks: nothing is launched
// chi2 only; d_edge_chi [n] (sorted order, 0 for priors that do not count; priors on fixed landmarks are not written)
void launch_lm_prior_errors(hipStream_t s, const cugo_lm_prior_edges& ev, const double* d_lms, double* d_wg_chi,
                            double* d_edge_chi = nullptr);
// the terms ADDED to d_Hll [Lfree][9] / d_bl [Lfree][3]; the same totals, bit for bit
void launch_lm_prior_add(hipStream_t s, const cugo_lm_prior_edges& ev, const double* d_lms, double* d_Hll, double* d_bl,
                         double* d_wg_chi);

// --- relative-pose SE(3) edges (relpose_kernels.hip) ---------------------------------------
// the device side of a cugo_relpose_plan (csrc/host/relpose_plan.h): index arrays and incidence lists
struct RelPosePlanDev
{
    int n, n_poses_free;
    const int32_t *pose_a, *pose_b; // [n]
    const int32_t *inc_ptr, *inc;   // [n_poses_free + 1], [inc_ptr[n_poses_free]]: edge << 1 | side
    const int32_t* off_blk;         // [n] block of the (lo, hi) term, -1 without one
};
// One kernel per pass: one 64-lane wave per free pose walks its incidence list in edge order and ADDS the pose's
// diagonal term and b at the end, the off-diagonal term of every edge whose other end is a free pose of larger index
// edge after edge; every workgroup leaves one chi2 total in d_wg_chi [relpose_workgroups()].
int relpose_workgroups(const cugo_relpose_edges& ev); // 0 without edges or free poses: nothing is launched
// chi2 only; d_edge_chi [n] (edge order; only the edges that count are written) or nullptr
void launch_relpose_errors(hipStream_t s, const cugo_relpose_edges& ev, const RelPosePlanDev& plan, const double* d_poses,
                           double* d_wg_chi, double* d_edge_chi = nullptr);
// the terms ADDED to d_Hpp / d_bp, the off-diagonal blocks to d_Hoff [nnzb][36] by block index (d_Hoff null: the
// off-diagonal terms are stored nowhere, launch_relpose_add_offdiag adds them later) ...
void launch_relpose_add(hipStream_t s, const cugo_relpose_edges& ev, const RelPosePlanDev& plan, const double* d_poses,
                        double* d_Hpp, double* d_bp, double* d_Hoff, double* d_wg_chi);
// ... or to d_Hsc (diagonal through d_rowptr, off-diagonal by block index), d_bp and d_bsc
void launch_relpose_add_schur(hipStream_t s, const cugo_relpose_edges& ev, const RelPosePlanDev& plan, const double* d_poses,
                              const int32_t* d_rowptr, double* d_Hsc, double* d_bp, double* d_bsc, double* d_wg_chi);
// ... or the off-diagonal terms alone ADDED to d_Hsc by block index: behind a Schur pass of the two-stream form, which
// has just overwritten every block, at the poses the build pass (launch_relpose_add with a null d_Hoff) linearised at.
// The terms and their order are those of launch_relpose_add_schur; no chi2 totals are written
void launch_relpose_add_offdiag(hipStream_t s, const cugo_relpose_edges& ev, const RelPosePlanDev& plan, const double* d_poses,
                                double* d_Hsc);

// --- pose-pose point edges with 3 x 3 information (point_pair_kernels.hip) ------------------
// the device side of a cugo_point_pair_plan (csrc/host/point_pair_plan.h)
struct PointPairPlanDev
{
    int n, n_runs, n_poses_free, n_blocks; // n_blocks: pattern blocks touched
    const int32_t* edge_run;                          // [n]
    const int32_t *run_ptr, *run_a, *run_b, *run_flags; // [n_runs + 1], [n_runs] x 3
    const int32_t *inc_ptr, *inc;                     // [n_poses_free + 1], run << 1 | side
    const int32_t *blk_id, *blk_ptr, *blk_run;        // [n_blocks], [n_blocks + 1], runs of every touched block
};
// A chunk pass leaves its partials (point_pair_partial_doubles() doubles: four roles of chunks + runs slots) and one
// chi2 total per chunk (point_pair_chunk_count()) where its ChunkScratch says
size_t point_pair_scratch_doubles(int n, int n_runs); // partials + totals
size_t point_pair_partial_doubles(int n, int n_runs);
int point_pair_chunk_count(int n);
ChunkScratch point_pair_scratch_in(ReduceScratch rs, int n, int n_runs);
// 1 if d_pose_a / d_pose_b of an edge are not those of its run in the plan, else 0; d_bad: a device int.  Synchronises
int point_pair_check_indices(hipStream_t s, const cugo_point_pair_edges& ev, const PointPairPlanDev& plan, int* d_bad);
// the chunk pass — full: the partials of the four roles and chi2; otherwise chi2 only (role 0; of the partials only
// element 27 of role 0's slots is written, which no finishing pass reads); d_edge_chi: errors only, sorted order.
// With d_cov_z: the covariance instantiation (cugo_gicp_pair_edges), ev.d_info = cov_p, ev.n_info = the count of both
void launch_point_pair_chunks(hipStream_t s, const cugo_point_pair_edges& ev, const PointPairPlanDev& plan, const double* d_poses,
                              bool full, ChunkScratch rs, double* d_edge_chi = nullptr, const double* d_cov_z = nullptr);
// the sums of a full chunk pass ADDED: diagonal blocks and b to d_Hpp / d_bp, the off-diagonal blocks to d_Hoff by block
// index if it is given ...
void launch_point_pair_add(hipStream_t s, const cugo_point_pair_edges& ev, const PointPairPlanDev& plan, ChunkScratch rs,
                           double* d_Hpp, double* d_bp, double* d_Hoff);
// ... everything to the Schur destination (diagonal through d_rowptr, b to d_bp and d_bsc, off-diagonal by block index) ...
void launch_point_pair_add_schur(hipStream_t s, const cugo_point_pair_edges& ev, const PointPairPlanDev& plan, ChunkScratch rs,
                                 const int32_t* d_rowptr, double* d_Hsc, double* d_bp, double* d_bsc);
// ... or its pieces: the diagonal part alone, plain or Schur, and the off-diagonal sums alone ADDED to d_H by block index
// (behind a Schur pass that has overwritten every block; reads the partials, not the poses)
void launch_point_pair_add_diag(hipStream_t s, const cugo_point_pair_edges& ev, const PointPairPlanDev& plan, ChunkScratch rs,
                                double* d_Hpp, double* d_bp);
void launch_point_pair_add_diag_schur(hipStream_t s, const cugo_point_pair_edges& ev, const PointPairPlanDev& plan,
                                      ChunkScratch rs, const int32_t* d_rowptr, double* d_Hsc, double* d_bp, double* d_bsc);
void launch_point_pair_add_offdiag(hipStream_t s, const cugo_point_pair_edges& ev, const PointPairPlanDev& plan, ChunkScratch rs,
                                   double* d_H);
void launch_point_pair_chi_total(hipStream_t s, const cugo_point_pair_edges& ev, ChunkScratch rs, double* d_chi, bool chi_add);

// chi_e per edge slot (outlier rejection, ref: computeOutliersKernel cuda_block_solver.cu:1135)
void launch_edge_chi(hipStream_t s, const cugo_edges& e, const double* d_poses, const double* d_lms,
                     cugo_robust rk, double* d_chi_e);

// --- multifrontal LL^T (chol_kernels.hip) -------------------------------------------------
// Device-side plan; all index arrays in units of 6x6 blocks unless noted.
constexpr int TMETA = 36; // ints per task record (CholPlanDev::tmeta)
constexpr int EA1_REC = 16; // ints per child link record (CholPlanDev::ea1): one 64-byte line
struct CholPlanDev
{
    int n_fronts;
    // per front
    const int32_t* ncb;        // pivot block columns
    const int32_t* nb;         // total block rows (pivot + boundary); the rhs row is row 6*nb
    const int64_t* off;        // offset (doubles) of the front matrix in `fronts`
    const int64_t* ldf;        // leading dimension: 6*nb + 1, or the child's when the front lives in
                               // the update block of its only child (single-child chains)
    const int32_t* alias_of;   // that child, or -1
    const int32_t* bw_np;      // backward: leading boundary block rows owned by the parent when the
                               // rest of the front's mat-vec is done ahead of time, else -1
    const int32_t* la_np;      // look-ahead: leading boundary block rows inside the parent's pivot columns
                               // (the front's "lead rows"; 0 for a root)
    const int64_t* woff;       // offset (doubles) of W = L11^-1 (pad16(6*ncb)^2, column-major) in winv
    double* winv;
    const int64_t* l21off;     // offset of the front's L21 (+ rhs row) in l21, or -1: in the front itself
    double* l21;               // column-major, leading dimension 6*(nb-ncb)+1
    int nc_max;                // widest pivot block (scalars)
    int ea_lds;                // potrf: children's contributions to F11 go straight into its LDS copy
    int panel16;               // potrf: 16-column register panels (CUGO_PANEL16=0: the 6-column LDS panels)
    int ea_direct;             // potrf: the children's F11 terms are added in registers as F11 is loaded, read
                               // straight from their lead blocks through the ea1 block masks (CUGO_EA_DIRECT=0: gathered
                               // child after child into the LDS copy)
#ifdef CUGO_DEBUG_HOOKS // (make HOOKS=1 -> libcugo_hip_hooks.so; the product build carries none of this)
    int kernel_acquire;        // CUGO_KERNEL_ACQUIRE: bit 0 = every kernel of the factorisation starts with an agent-scope acquire fence, bit 1 = ends with a release fence
    int dbg_delay;             // diagnosis (CUGO_DEBUG_DELAY): which waves / workgroups of the factorisation's kernels sleep (chol_kernels.hip: dbg_sleep)
    int zero_lds;              // diagnosis (CUGO_DEBUG_ZERO_LDS=1 / 2): every kernel fills its LDS with zeros / NaNs first
    int lds_doubles;           // (set per launch: the dynamic LDS of this launch, for that fill)
    int dbg_skip_wg;           // (set per launch, -1: none) fault injection: this workgroup returns at once (CUGO_DEBUG_SKIP)
#endif
    const int32_t* col0;       // first pivot column (new ordering, block units)
    const int32_t* rows_ptr;   // [n_fronts+1] into rows: boundary block rows (new ordering)
    const int32_t* rows;
    const int32_t* child_ptr;  // [n_fronts+1] children of each front
    const int32_t* child;      // child front ids
    const int32_t* rel_ptr;    // [n_fronts+1] (indexed by CHILD front) into rel
    const int32_t* rel;        // position (block row in the parent front) of each boundary row
    // schedule
    int n_stages;
    const int32_t* ea1;        // per child link, EA1_REC ints: {child, its boundary block rows, its leading rows inside
                               // the parent's pivots, offset of its rel list, update-block offset (int64), its leading
                               // dimension (int64), block mask of the parent pivot block rows those leading rows land
                               // on (bit rel[b], b < leading rows), 0 ...} — the potrf workgroup's extend-add into F11
                               // (tmeta[16..17])
    const int32_t* tmeta;      // [n_tasks_total][TMETA] (16..17: range in ea1, 18..19 unused): {fronts in the task, first front, its ncb, nb, col0, bw_np,
                               // rows_ptr, has-children-to-add flag, off, ldf, woff, l21off (four int64)} (potrf, backward substitution);
                               // 20..35: the front's first 16 boundary block rows (those inside its parent's pivot block: the
                               // backward substitution gathers x_R through them without a round trip to the row lists)
    // k_assemble_fronts (chol_symbolic.h: CholPlan::asm_map): per stored front its map at asm_off[front]
    const int32_t* asm_map;
    const int64_t* asm_off;
    const int32_t* wl_base;    // the work-item triples (chol_symbolic.h: CholPlan::wl) ...
    const int32_t* fat;        // ... and one 64-byte record per item for the tile kernels (TileItem)
    const int32_t* bc_rec;     // k_backward_chain, BC_REC ints per ticket (chol_symbolic.h: CholPlan::bc_front): {front, ncb, nb, col0,
                               // rows_ptr, first segment, segments, 0, woff, l21off, off, ldf (four int64)}
    const int32_t* bc_seg;     // ... and 4 ints per segment: {ancestor front, first boundary block row, block rows, 0}
    const int32_t* task_ptr;   // [n_tasks_total+1] into task_fronts
    const int32_t* task_fronts;
    // assembly of A (one entry per Hsc block)
    int n_hsc_blocks;
    const int32_t* blk_front;
    const int32_t* blk_row;    // block row in the front
    const int32_t* blk_col;    // block col in the front
    const uint8_t* blk_trans;  // 1: store transposed
    // rhs / solution mapping
    int n;                     // block rows of the matrix
    const int32_t* perm;       // new -> old
    const int32_t* col_front;  // new col -> front
    // sink for masked-off lanes: lets conditional stores/loads be emitted branch-free (a branch
    // per store makes the compiler wait vmcnt(0) before each one, serialising the stores)
    double* junk;              // 64 x 1024 doubles
};

// clears the fronts (their lower triangles through the nclear items front / first / past-last column;
// nclear == 0: the whole buffer), scatters Hsc (+lambda) and bsc into them and resets *d_fail
void launch_chol_assemble(hipStream_t s, const CholPlanDev& p, double* d_fronts, size_t front_doubles,
                          const double* d_Hsc, double lambda, const double* d_bsc, int32_t* d_fail,
                          const int32_t* d_clear_items, int nclear, const int32_t* d_asm_items = nullptr,
                          int nasm = 0);
void launch_chol_subtree_stage(hipStream_t s, const CholPlanDev& p, double* d_fronts, int task0,
                               int ntasks, size_t lds_bytes, int32_t* d_fail);
// one etree level: extend-add(pivot columns) / potrf (+ extend-add of the boundary columns) /
// fused trsm+syrk kernels over the work items d_wl[...]
// tile: edge of the update-matrix tiles of this level's items (64, or 32 on levels with few fronts)
void launch_chol_upper_stage(hipStream_t s, const CholPlanDev& p, double* d_fronts, int task0,
                             int ntasks, const int32_t* d_wl, int eap0, int neap, int ea0, int nea,
                             int sy0, int nsy, int tile, size_t lds_bytes, int32_t* d_fail,
                             double* dbg_line = nullptr, double* dbg_scratch = nullptr);
#ifdef CUGO_DEBUG_HOOKS
// diagnosis (CUGO_DEBUG_STALE): exchanges the 16 doubles at `line` with those at `scratch`
void launch_swap16(hipStream_t s, double* line, double* scratch);
#endif
// two-phase form of a level's tile work (stage_tile == 0): trsm items (front, first row below the pivots,
// rows) then syrk items (front, linear tile index, tile columns)
void launch_chol_two_phase(hipStream_t s, const CholPlanDev& p, double* d_fronts, const int32_t* d_trsm, int ntrsm,
                           const int32_t* d_syrk, int nsyrk);
// look-ahead schedule, two launches per level (see k_up_potrf_la / k_up_lead):
//   potrf of level k (ntasks fronts from task0) together with the non-lead update tiles of level k-1
//   (items front, ti, tj of edge `tile`); then the lead workgroups of level k (items front,-,-)
//   together with the extend-add below the lead rows (items front, first, past-last block column)
void launch_chol_potrf_la(hipStream_t s, const CholPlanDev& p, double* d_fronts, int task0, int ntasks,
                          const int32_t* d_tiles, int ntiles, int tile, int32_t* d_fail);
void launch_chol_lead(hipStream_t s, const CholPlanDev& p, double* d_fronts, const int32_t* d_lead,
                      int nlead, const int32_t* d_eap, int neap, const int32_t* d_eab, int neab);
// backward substitution of one level: ntasks workgroups solve the level's fronts; ngemv more
// workgroups (items d_wl_gemv: front, first column, -) do the ancestor part of the mat-vec of
// the CHILDREN of these fronts, which the next launch then does not have to wait for
void launch_chol_backward_stage(hipStream_t s, const CholPlanDev& p, double* d_fronts, int task0,
                                int ntasks, size_t lds_bytes, double* d_xnew, double* d_x,
                                const int32_t* d_wl_gemv, int ngemv);
// the whole backward substitution in one launch, one workgroup per front, x handed from front to front inside
// the launch (k_backward_chain).  d_state: the solver's words (uint32, hipMalloc, zeroed ONCE when they are
// allocated): [BC_HEAD] the ticket head, [BC_ABORT] set by a workgroup whose wait ran into its time bound,
// [BC_ERROR] the same, never cleared, [BC_DONE + f] = epoch once front f has published its x.  ticket_base: what
// the head holds when the launch starts (nfronts per call, modulo 2^32); epoch: never 0, another one every call.
// h_error: pinned host word that is set with [BC_ERROR] (the caller looks at it after a synchronisation)
constexpr int BC_REC = 16, BC_HEAD = 0, BC_ABORT = 32, BC_ERROR = 33, BC_DONE = 64;
void launch_chol_backward_chain(hipStream_t s, const CholPlanDev& p, double* d_fronts, int nfronts, double* d_xnew,
                                double* d_x, uint32_t* d_state, uint32_t ticket_base, uint32_t epoch, int32_t* d_fail,
                                uint32_t* h_error);
#ifdef CUGO_DEBUG_HOOKS
void launch_nop(hipStream_t s); // diagnosis (CUGO_DEBUG_GAP): an empty kernel
// fault injection (CUGO_DEBUG_SKIP): the launches of the factorisation that follows are counted from 0; workgroup
// target_wg of launch target_launch returns at once; dump_path: the launch table (index, kernel, grid, first items) goes there
void chol_dbg_skip_begin(int target_launch, int target_wg, const char* dump_path);
void chol_dbg_skip_end();
// diagnosis (CUGO_DEBUG_HASH): *out += the sum of the n 64-bit words at p (integer sum: order-independent)
void launch_hash_words(hipStream_t s, const void* p, size_t n_words, unsigned long long* out);
#endif
void launch_flag_to_double(hipStream_t s, int32_t* d_flag); // int32 0 / 1 -> double 0.0 / 1.0 in the same 8-byte slot
void launch_chol_unpermute(hipStream_t s, const CholPlanDev& p, const double* d_xnew, double* d_x);
// ownership-keyed exchange of [Hsc | bsc] (chol_symbolic.h: CholPlan::xs_off; d_off [B + n] packed offsets):
// every unit of d_sys into the packed buffer / the units at packed offsets [lo, hi) or >= top0 back into d_sys
void launch_xs_pack(hipStream_t s, const int64_t* d_off, int B, int n, const double* d_sys, double* d_xbuf);
void launch_xs_unpack(hipStream_t s, const int64_t* d_off, int B, int n, const double* d_xbuf, double* d_sys, long lo,
                      long hi, long top0);
void set_debug_stamps(long long* d_buf); // diagnostic s_memtime stamps (nullptr = off)
void set_chain_stamps(long long* d_buf); // k_backward_chain: three 100 MHz stamps per ticket (stamps build; nullptr = off)
size_t chol_lds_factor_bytes(int nc_max);
size_t chol_lds_backward_bytes(int nc_max, long ld_max);
int chol_max_pivot_cols(); // widest pivot block the kernels support (scalars)

// --- marginal covariances (cov_kernels.hip) ----------------------------------------------
// selected inverse of the factorisation a factor_solve left (W, L21 where the backward pass reads them) into
// Sigma-fronts laid out like the fronts.  d_sinfo [n_fronts][4]: offset and leading dimension of the parent's
// Sigma-front, offset of the front's rel list, 1 = copy S_RR into the front's own Sigma-front
// rows: items (front, first row) of 64-row tiles of R; jj: one workgroup per task of an upper stage;
// subtree: one workgroup per subtree task of stage 0 (both parts, front by front)
void launch_selinv_rows(hipStream_t s, const CholPlanDev& p, const double* d_fronts, double* d_sig,
                        const int64_t* d_sinfo, const int32_t* d_items, int nitems);
void launch_selinv_jj(hipStream_t s, const CholPlanDev& p, const double* d_fronts, double* d_sig, int task0,
                      int ntasks);
void launch_selinv_subtree(hipStream_t s, const CholPlanDev& p, const double* d_fronts, double* d_sig,
                           const int64_t* d_sinfo, int task0, int ntasks);
// d_out [n_hsc_blocks][36]: the blocks of Sigma on the Hsc pattern (layout of d_Hsc)
void launch_selinv_gather(hipStream_t s, const CholPlanDev& p, const double* d_sig, double* d_out);
int selinv_row_tile(); // rows of R per k_selinv_rows item
// blocks of the inverse for arbitrary pairs, from forward solves alone (k_inv_path_walk, k_inv_pair_blocks).
// d_rows [nrows]: distinct query block rows in the solver's ordering; d_ws [nrows][6 n][6], zeroed by the caller, holds
// Y_v = L^-1 E_v of row g at d_ws + g * 36 n afterwards.  d_sparent [n_fronts]: CholPlan::sparent
void launch_inv_path_walk(hipStream_t s, const CholPlanDev& p, const double* d_fronts, const int32_t* d_sparent,
                          const int32_t* d_rows, int nrows, double* d_ws);
// d_pairs [npairs][3]: {workspace slot of a, slot of b, a in the solver's ordering}; d_out [npairs][36]: Y_a^T Y_b,
// column-major (rows a, columns b)
void launch_inv_pair_blocks(hipStream_t s, const CholPlanDev& p, const int32_t* d_sparent, const int32_t* d_pairs,
                            int npairs, const double* d_ws, double* d_out);
// d_out [P][36]: the diagonal blocks of d_sigma (the first block of every row of the upper block CSR d_rowptr)
void launch_cov_pose_diag(hipStream_t s, int P, const int32_t* d_rowptr, const double* d_sigma, double* d_out);
// Sigma_l [L][9] of every free landmark from Hll, Hpl (landmark-major edge slots) and the pose blocks d_sigma on the
// Hsc pattern (upper block CSR d_rowptr / d_colind); *d_fail = 1 if an Hll is not positive definite
void launch_lm_covariance(hipStream_t s, int L, const int32_t* d_lm_ptr, const int32_t* d_e_pose,
                          const uint8_t* d_flags, const double* d_Hll, const double* d_Hpl, const int32_t* d_rowptr,
                          const int32_t* d_colind, const double* d_sigma, double* d_out, int32_t* d_fail);
// Sigma_al [n][18] (6 x 3 column-major, rows a) of n queries (d_q_pose / d_q_lm: free indices, -1 for a fixed vertex: 18
// zeros): slot k of the query's landmark reads the block d_blocks[d_q_slot[d_q_ptr[q] + k]] ([.][36], column-major, rows
// a; csrc/host/plcov_plan.h); *d_fail = 1 if the Hll of a queried landmark is not positive definite (18 zeros)
void launch_pose_lm_cross(hipStream_t s, int n, const int32_t* d_q_pose, const int32_t* d_q_lm, const int32_t* d_q_ptr,
                          const int32_t* d_q_slot, const int32_t* d_lm_ptr, const uint8_t* d_flags, const double* d_Hll,
                          const double* d_Hpl, const double* d_blocks, double* d_out, int32_t* d_fail);
// S [n][9] (3 x 3 column-major) = J Sigma J^T of the reprojection of landmark d_q_lm[q] in pose d_q_pose[q] (indices into
// d_lms / d_poses, fixed vertices included; d_q_aa: the block of Sigma_aa in d_blocks, -1 for a fixed pose; a landmark
// index >= Lfree is fixed); d_cross: what launch_pose_lm_cross wrote, d_lmcov: what launch_lm_covariance wrote
void launch_reprojection_cov(hipStream_t s, int n, int Lfree, const int32_t* d_q_pose, const int32_t* d_q_lm,
                             const int32_t* d_q_dim, const int32_t* d_q_aa, const double* d_cam5, const double* d_poses,
                             const double* d_lms, const double* d_blocks, const double* d_cross, const double* d_lmcov,
                             double* d_out);
// z3 [n][3] and S [n][9] of n predicted observations (k_predict_obs): as launch_reprojection_cov with a kind per query
// (CUGO_OBS_*) instead of a dim and d_cam_tab [n][17] = {M row-major, t_s, k1..k4, model} per query, or NULL (pinholes
// at the pose; kinds 2 / 3 then give the bits of launch_reprojection_cov)
void launch_predict_obs(hipStream_t s, int n, int Lfree, const int32_t* d_q_pose, const int32_t* d_q_lm,
                        const int32_t* d_q_kind, const int32_t* d_q_aa, const double* d_cam5, const double* d_cam_tab,
                        const double* d_poses, const double* d_lms, const double* d_blocks, const double* d_cross,
                        const double* d_lmcov, double* d_z3, double* d_out);

} // namespace cugo_k
