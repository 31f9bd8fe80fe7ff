/*
 * cugo_hip.h — C ABI of libcugo_hip.so, the MI355X (gfx950) implementation of the bundle-
 * adjustment hot path of KudanLimited/cuda-bundle-adjustment.
 *
 * Two layers, both plain C (pointers + sizes, no C++ or torch types):
 *
 *  (1) kernel-level entry points  cugo_*  — one per free function of the reference's
 *      `namespace cugo::gpu` (src/cuda/cuda_block_solver.h:55-256) and per method of its
 *      linear-solver object (src/cuda_linear_solver.h:31-53).  All pointers named d_* are
 *      DEVICE pointers; work is enqueued on the context's HIP stream and is asynchronous
 *      unless the function returns a host value.
 *  (2) graph-level entry points   cugo_graph_*  — what a foreign-language binding of the
 *      reference's public class (include/cuda_graph_optimisation.h:132-252) would call:
 *      flat host arrays in, BatchStatistics / estimates out.
 *
 * Citations "ref:" are file:line in the reference repository.
 * Every function returns CUGO_OK (0) or a negative error code; cugo_last_error() gives text.
 * There is NO CPU fallback: without a HIP device every call fails with CUGO_ERR_NO_DEVICE.
 */
#ifndef CUGO_HIP_H
#define CUGO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CUGO_OK 0
#define CUGO_ERR_NO_DEVICE (-1)
#define CUGO_ERR_HIP (-2)
#define CUGO_ERR_INVALID (-3)
#define CUGO_ERR_NUMERIC (-4) /* zero pivot: ref src/cuda_linear_solver.cpp:44-52 */

/* ref: src/robust_kernel.h:12-17 */
enum { CUGO_RK_NONE = 0, CUGO_RK_CAUCHY = 1, CUGO_RK_TUKEY = 2,
       CUGO_RK_HUBER = 3 /* extension: g2o RobustKernelHuber, rho(x) = x | 2*delta*sqrt(x) - delta^2 */ };

/* edge flag bits; bits 0/1 are the reference's EdgeFlag (ref: src/constants.h:28-32) */
enum
{
    CUGO_EDGE_FIXED_L = 1,
    CUGO_EDGE_FIXED_P = 2,
    CUGO_EDGE_STEREO = 4,  /* 3-d measurement (StereoEdge) instead of 2-d (MonoEdge) */
    CUGO_EDGE_INACTIVE = 8, /* outlier / removed: contributes nothing (ref: outliers[e]!=0) */
    CUGO_EDGE_DEPTH = 16    /* extension: 3-d measurement (u, v, 1/Z) of a DepthEdge; never together with STEREO.
                             * Looked at only when cugo_edges.has_depth != 0 */
};

typedef struct cugo_ctx cugo_ctx; /* device + stream + scratch; replaces CudaDevice */

const char* cugo_last_error(void);
int cugo_device_count(void);
/* ref: src/cuda_device.cpp:166-282 (device pick + streams). device<0 = current device. */
int cugo_ctx_create(int device, cugo_ctx** out);
void cugo_ctx_destroy(cugo_ctx* ctx);
int cugo_ctx_sync(cugo_ctx* ctx);
void* cugo_ctx_stream(cugo_ctx* ctx); /* hipStream_t */

/* ref: src/device_buffer.h:33-276 (RAII device array) — plain allocation helpers */
int cugo_malloc(void** d_ptr, size_t bytes);
int cugo_free(void* d_ptr);
int cugo_memcpy_h2d(cugo_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int cugo_memcpy_d2h(cugo_ctx* ctx, void* h_dst, const void* d_src, size_t bytes); /* syncs */
int cugo_memset(cugo_ctx* ctx, void* d_dst, int value, size_t bytes);

/*
 * Flattened edge data of ALL edge sets of one optimiser, landmark-major:
 * edges are sorted by (landmark index, pose index); the edges of landmark l are
 * [lm_ptr[l], lm_ptr[l+1]).  Mono and stereo edges share the arrays (flag bit STEREO).
 * This replaces the per-set arrays of ref: src/optimisable_graph.hpp:474-601
 * (measurements | edge2PL | flags | omegas | cameras) and edge2Hpl: the Hpl block of edge
 * e is block e (identity map), valid when (flags & 3) == 0.
 * pose_ptr/pose_edge give the same edges grouped by pose (CSR over pose index).
 */
typedef struct cugo_edges
{
    int n_edges;
    int n_poses_total, n_landmarks_total; /* incl. fixed (indices >= n_free are fixed) */
    int n_poses_free, n_landmarks_free;
    const int32_t* d_pose;   /* [E] pose index      (ref edge2PL[e][0]) */
    const int32_t* d_lm;     /* [E] landmark index  (ref edge2PL[e][1]) */
    const double* d_meas;    /* [3][E] planar: u, v, u_right (stereo slot) or 1/Z (depth slot) */
    const double* d_omega;   /* [E] or [1] information (ref omegas) */
    int n_omega;             /* E or 1  (ref: perEdgeInformation) */
    const uint8_t* d_flags;  /* [E] CUGO_EDGE_* */
    const uint16_t* d_cam;   /* [E] index into d_cams, or NULL when n_cams == 1 */
    const double* d_cams;    /* [n_cams][5] fx fy cx cy bf (ref cameras, deduplicated) */
    int n_cams;
    const int32_t* d_lm_ptr;    /* [n_landmarks_total+1] */
    const int32_t* d_pose_ptr;  /* [n_poses_total+1]     */
    const int32_t* d_pose_edge; /* [E] edge ids grouped by pose, ascending landmark */
    /* Element type of the two per-edge block arrays d_Hpl and d_T ([E][18] each) handed to
     * cugo_construct_quadratic_form / cugo_compute_schur / cugo_backsubst_update:
     * 0 = double, 1 = float (the fp32-internal mode, ref: the USE_FLOAT32 build option,
     * CMakeLists.txt:8, src/scalar.h:24-28).  Only the storage of these two streams changes:
     * every value is widened on load, all arithmetic and every other array stay fp64. */
    int block_f32;
    /* Extension: inverse-depth slots (CUGO_EDGE_DEPTH, ref: DepthEdge include/ba_types.h:171-260).  Residual
     *   e = (pu - m_u, pv - m_v, s (1/Z - m_d)),  s = sqrt(depth_weight);  bf of the camera is not used.
     * has_depth == 0 (every zero-initialised struct): none of the members below is read, the DEPTH bit of d_flags is
     * not looked at and every entry point runs the kernels it has always run.  has_depth != 0: slots with the DEPTH
     * bit are depth slots (there may be none: the results then have the bits of has_depth == 0), their robust kernel is
     * (rk_type_depth, rk_delta_depth) — cugo_robust keeps describing the mono and stereo kinds — and depth_weight must
     * be finite and > 0 (CUGO_ERR_INVALID otherwise).  Mono and stereo slots come out with the same bits either way. */
    int has_depth;
    int rk_type_depth;     /* CUGO_RK_* */
    double rk_delta_depth;
    double depth_weight;   /* k: the set's inverse-depth weight (1: chi2 of the reference's computeActiveErrors_DepthBa) */
    /* Extension: camera extrinsics (a multi-camera rig).  The pose is world -> body, and camera-table entry k carries a
     * fixed sensor pose body -> sensor, d_cam_ext[12 k] = {M row-major (9), t_s (3)}:
     *   Xb = R(q) Xw + t,  Xs = M Xb + t_s,  residual and robust kernel as always, evaluated at Xs;
     * the Jacobians are those of the left update on the body pose.  The slot's camera index (d_cam, 16 bits) selects
     * the entry; with n_cams == 1 entry 0 serves every slot.  has_rig == 0 (every zero-initialised struct): d_cam_ext
     * is not read and every entry point runs the kernels it has always run.  has_rig != 0 with d_cam_ext == NULL, or
     * together with has_depth != 0 (not yet), is CUGO_ERR_INVALID before anything is launched.
     * Extension: camera models (Kannala-Brandt fisheye).  has_rig takes one of the CUGO_RIG_* values below; every
     * non-zero value other than CUGO_RIG_MODELS (2) and CUGO_RIG_DISTORTION (3) means CUGO_RIG_EXTRINSICS, as it always
     * did (3 used to fall under that rule until the distortion tables below took the value).  With has_rig == CUGO_RIG_MODELS d_cam_ext is a MODEL
     * table of stride 17, d_cam_ext[17 k] = {M row-major (9), t_s (3), k1, k2, k3, k4, model}, model 0.0 (pinhole) or
     * 1.0 (Kannala-Brandt):
     *   theta = atan2(sqrt(x^2 + y^2), z),  theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8),
     *   pu = fx theta_d x / r + cx,  pv = fy theta_d y / r + cy          at Xs = (x, y, z);  z <= 0 is a legal point.
     * A pinhole entry of a model table gives the bits of the same entry under CUGO_RIG_EXTRINSICS.  A Kannala-Brandt
     * entry has two rows: bf has no meaning there, and a stereo slot on such an entry is NOT DEFINED at this level (the
     * graph level refuses it).  CUGO_RIG_MODELS with d_cam_ext == NULL or together with has_depth != 0 is
     * CUGO_ERR_INVALID before anything is launched.
     * Extension: radial-tangential lens distortion (OpenCV's distCoeffs, Kalibr's radtan, ROS's plumb_bob).  With
     * has_rig == CUGO_RIG_DISTORTION d_cam_ext is a DISTORTION table of stride 18, d_cam_ext[18 k] = {M row-major (9),
     * t_s (3), k1, k2, p1, p2, k3, flag}, flag 0.0 (undistorted) or 1.0 (distorted); at Xs = (x, y, z):
     *   a = x / z,  b = y / z,  r2 = a^2 + b^2,  rad = 1 + k1 r2 + k2 r2^2 + k3 r2^3,
     *   a' = a rad + 2 p1 a b + p2 (r2 + 2 a^2),  b' = b rad + p1 (r2 + 2 b^2) + 2 p2 a b,
     *   pu = fx a' + cx,  pv = fy b' + cy;                       measurements are RAW (distorted) pixels.
     * An undistorted entry of a distortion table gives the bits of the same entry under CUGO_RIG_EXTRINSICS, stereo
     * slots included.  A distorted entry has two rows: bf has no meaning there and the stereo bit of a slot on it is not
     * looked at for them (as on a Kannala-Brandt entry it still picks the robust kernel; the graph level refuses such a
     * slot).  z <= 0 is the caller's problem, as for the pinhole.  A distorted
     * and a Kannala-Brandt entry cannot share a table.  CUGO_RIG_DISTORTION with d_cam_ext == NULL or together with
     * has_depth != 0 is CUGO_ERR_INVALID before anything is launched. */
    int has_rig;
    const double* d_cam_ext; /* [n_cams][12], [n_cams][17] with CUGO_RIG_MODELS, [n_cams][18] with CUGO_RIG_DISTORTION */
} cugo_edges;

/* cugo_edges.has_rig */
#define CUGO_RIG_NONE 0       /* d_cam_ext is not read */
#define CUGO_RIG_EXTRINSICS 1 /* d_cam_ext [n_cams][12]: sensor poses */
#define CUGO_RIG_MODELS 2     /* d_cam_ext [n_cams][17]: sensor poses, Kannala-Brandt coefficients, model flag */
#define CUGO_CAM_TAB_STRIDE 17
#define CUGO_RIG_DISTORTION 3 /* d_cam_ext [n_cams][18]: sensor poses, (k1, k2, p1, p2, k3), distortion flag */
#define CUGO_DIST_TAB_STRIDE 18

typedef struct cugo_robust
{
    int type;     /* CUGO_RK_* for 2-d (mono) edges */
    double delta; /* ref: createRkFunction src/cuda/cuda_block_solver.h:61 — passed by value */
    int type_stereo; /* same for 3-d (stereo) edges: per edge set, not process-global */
    double delta_stereo;
} cugo_robust;

/* ---- (1) kernel-level entry points --------------------------------------------------- */

/* ref: gpu::computeActiveErrors_<2|3> (cuda_block_solver.h:179-193; .cu:1060-1133).
 * d_poses: [n_poses_total][7] (qx qy qz qw tx ty tz), d_lms: [n_landmarks_total][3].
 * Writes the total chi2 to d_chi[0] (device).  Deterministic (fixed reduction order). */
int cugo_compute_active_errors(cugo_ctx* ctx, const cugo_edges* ev, const double* d_poses,
                               const double* d_lms, cugo_robust rk, double* d_chi);

/* Extension: d_edge_chi[e] = rho(omega |e|^2) of every edge slot, 0 for an inactive slot ([n_edges], device): what the
 * outlier rejection compares with the set's threshold (ref: d_chiValues, computeOutliersKernel .cu:1135).  Asynchronous. */
int cugo_compute_edge_chi(cugo_ctx* ctx, const cugo_edges* ev, const double* d_poses, const double* d_lms,
                          cugo_robust rk, double* d_edge_chi);

/* ref: gpu::constructQuadraticForm_<2|3> (cuda_block_solver.h:159-176; .cu:1152-1220) plus
 * the four fillZero calls of BlockSolver::buildSystem (block_solver.cpp:287-294).
 * Outputs (all column-major blocks, reference layout):
 *   d_Hpp [Pfree][36], d_bp [Pfree][6], d_Hll [Lfree][9], d_bl [Lfree][3], d_Hpl [E][18]
 *   (d_Hpl and, below, d_T: double, or float when ev->block_f32).
 * Also writes chi2 at these estimates to d_chi[0] if d_chi != NULL. No atomics. */
int cugo_construct_quadratic_form(cugo_ctx* ctx, const cugo_edges* ev, const double* d_poses,
                                  const double* d_lms, cugo_robust rk, double* d_Hpp,
                                  double* d_bp, double* d_Hll, double* d_bl, void* d_Hpl,
                                  double* d_chi);

/* ref: gpu::maxDiagonal x2 (cuda_block_solver.h:78-81; block_solver.cpp:309-320).
 * d_out[0] = max(0, max diag(Hpp), max diag(Hll)). */
int cugo_max_diagonal(cugo_ctx* ctx, const double* d_Hpp, int n_poses, const double* d_Hll,
                      int n_landmarks, double* d_out);

/* Hsc block structure on the device (ref: HschurSparseBlockMatrix,
 * src/sparse_block_matrix.cpp:63-156, and mulBlockIds .cu:1347-1378).
 * Upper-triangular block CSR, diagonal block first in each row.  Off-diagonal block k has
 * the contribution list [d_off_ptr[k], d_off_ptr[k+1]) of (edge_i, edge_j) pairs:
 * Hsc[k] -= T[edge_i] * Hpl[edge_j]^T. (diagonal blocks use the pose's own edge list).
 * ZERO-INITIALISE the struct (memset / = {0}) before filling it: cugo_compute_schur selects the
 * landmark-major plan kernels when the plan fields (d_grp_ptr ...) are non-NULL. */
typedef struct cugo_hsc_struct
{
    int n_blocks;             /* B */
    const int32_t* d_rowptr;  /* [Pfree+1] */
    const int32_t* d_colind;  /* [B] */
    const int32_t* d_off_ptr; /* [B+1] (empty range for diagonal blocks) */
    const int32_t* d_off_ei;  /* [M_off] */
    const int32_t* d_off_ej;  /* [M_off] */
    /* Landmark-major product plan (optional: with d_grp_ptr == NULL cugo_compute_schur gathers the
     * products destination-major through the contribution lists above).  A group = 256 consecutive
     * edge slots; the products of a group's landmarks are summed per (group, Hsc block) into a
     * partial slot, the slots of every block are then added in group order.  Built by
     * cugo_hsc_plan_create(); requires that no landmark has active edges in two groups. */
    int n_groups;                /* ceil(n_edges / 256) */
    int n_slots, n_rhs;
    const int32_t* d_grp_ptr;    /* [n_groups+1] partial slots of each group (longest product list first) */
    const int32_t* d_grp_nwave;  /* [n_groups] leading slots of the group that a whole wave works on */
    const int32_t* d_slot_rhs;   /* [n_slots] index of the slot's rhs partial (diagonal block) or -1 */
    const int32_t* d_slot_ptr;   /* [n_slots+1] product range of each slot */
    const uint16_t* d_prod;      /* [M] a | b << 8: slots (within the group) of the T and Hpl operand */
    const int32_t* d_red_ptr;    /* [B+1] partial slots of every Hsc block ... */
    const int32_t* d_red_slot;   /* [n_slots] ... in group order */
    const int32_t* d_blk_pose;   /* [B] pose of a diagonal block, -1 otherwise */
    double* d_part_H;            /* [n_slots][36] scratch */
    double* d_part_b;            /* [n_rhs][6] scratch */
} cugo_hsc_struct;

/* Builds the landmark-major plan of a flattened edge set on the host and uploads it (ref: the device
 * structure set-up findHschureMulBlockIndices, src/cuda/cuda_block_solver.cu:1347-1378,1606-1634).
 * h_* are HOST arrays: the edge slots (pose index, landmark index, flags; landmark-major) and the
 * Hsc pattern.  Fills the plan fields of *hs (the pattern / contribution-list fields are left
 * alone).  Returns CUGO_ERR_INVALID, with the plan fields cleared, when a landmark's active edges
 * straddle two 256-slot groups: cugo_compute_schur then takes the gather kernels. */
typedef struct cugo_hsc_plan cugo_hsc_plan;
int cugo_hsc_plan_create(cugo_ctx* ctx, int n_edges, int n_poses_free, const int32_t* h_pose,
                         const int32_t* h_lm, const uint8_t* h_flags, const int32_t* h_rowptr,
                         const int32_t* h_colind, cugo_hsc_struct* hs, cugo_hsc_plan** out);
void cugo_hsc_plan_destroy(cugo_hsc_plan* plan);

/* ref: gpu::addLambda(Hll) + gpu::computeBschure + gpu::computeHschure
 * (cuda_block_solver.h:83-109; .cu:1256-1345).  Damping is applied on the fly (Hpp/Hll are
 * left undamped, so no backup/restoreDiagonal pass exists).
 *   d_invHll [Lfree][9] = (Hll + lambda I)^-1 (written by the landmark's first edge slot: the block of a free landmark
 *   without any edge slot is left untouched — nothing reads it, cugo_backsubst_update gives such a landmark a zero step),
 *   d_T [E][18] = Hpl * invHll (zero blocks for edges with a fixed endpoint and for inactive slots),
 *   d_bsc [Pfree][6] = bp - sum T bl,
 *   d_Hsc [B][36] = Hpp(diag) - sum T Hpl^T            (+ lambda I on diagonal blocks when
 *   damp_hsc_diag != 0, which reproduces the reference's damped Hsc exactly).
 * With a landmark-major plan in *hs (cugo_hsc_plan_create) the products are formed inside the edge
 * pass and d_T may be NULL (T is then never written). */
int cugo_compute_schur(cugo_ctx* ctx, const cugo_edges* ev, const cugo_hsc_struct* hs,
                       double lambda, int damp_hsc_diag, const double* d_Hpp, const double* d_bp,
                       const double* d_Hll, const double* d_bl, const void* d_Hpl,
                       double* d_invHll, void* d_T, double* d_bsc, double* d_Hsc);

/* Sparse block LL^T of Hsc: replaces HscSparseLinearSolver / CuSparseCholeskySolver
 * (ref: src/cuda_linear_solver.cpp:27-57, src/cholesky.hpp:170-309 — cuSOLVER csrchol +
 * METIS).  analyze() = ordering + symbolic (host) once per structure; factor_solve() =
 * numeric multifrontal LL^T + triangular solves on the device per LM trial. */
typedef struct cugo_chol cugo_chol;
int cugo_chol_create(cugo_ctx* ctx, cugo_chol** out);
void cugo_chol_destroy(cugo_chol* s);
/* host pattern: upper block CSR incl. diagonal (ref: initialize(Hsc pattern)) */
int cugo_chol_analyze(cugo_chol* s, int n_block_rows, const int32_t* h_rowptr,
                      const int32_t* h_colind);
/* solve (Hsc + lambda I) x = bsc.  d_Hsc [B][36] upper blocks in the analysed pattern,
 * d_bsc / d_x [n_block_rows][6].  Asynchronous: the zero-pivot flag is written to
 * d_fail[0] (int32 device, 0 = ok) — ref: solve()->bool, zero pivot tol 1e-14. */
int cugo_chol_factor_solve(cugo_chol* s, const double* d_Hsc, double lambda, const double* d_bsc,
                           double* d_x, int32_t* d_fail);
/* Extension (g2o SparseOptimizer::computeMarginals, Ceres Covariance): after a successful
 * cugo_chol_factor_solve(s, d_Hsc, lambda, ...): the blocks of (A + lambda I)^-1 on the analysed
 * pattern, same layout as d_Hsc ([nnzb][36], upper block CSR, diagonal first, column-major).
 * Synchronises once to read the zero-pivot flag of that factorisation (CUGO_ERR_NUMERIC if it is set;
 * its d_fail must still be valid), then enqueues on the context's stream.  CUGO_ERR_INVALID if no
 * factorisation ran since analyze(), or if the solver factors rank-owned subtrees.  The first call
 * after analyze() allocates a buffer of the size of the fronts (cugo_chol_stats: front_bytes). */
int cugo_chol_selected_inverse(cugo_chol* s, double* d_sigma);
/* Extension (g2o computeMarginals(spinv, blockIndices)): the blocks (h_rows[k], h_cols[k]) of (A + lambda I)^-1 for
 * ANY block pairs of the analysed numbering — off the pattern, below the diagonal (a > b) and a == b included —
 * from the factorisation the last cugo_chol_factor_solve left.  d_out [n_pairs][36] (device), each block 6x6
 * column-major with rows a and columns b, as a block of d_sigma above.  The index lists are host arrays.  The
 * contract of cugo_chol_selected_inverse: one synchronisation for the zero-pivot flag (CUGO_ERR_NUMERIC if set),
 * then enqueued on the context's stream; CUGO_ERR_INVALID before any factorisation, on a host-only solver, with
 * rank-owned subtrees, for n_pairs < 0 or an index outside [0, n_block_rows).  Every distinct query row takes a
 * workspace of 288 n_block_rows bytes; the pairs are processed in batches whose rows fit 512 MB (or CUGO_XCOV_BATCH
 * rows, read when the solver is created).  The same bits on every call, whatever the batches. */
int cugo_chol_inverse_blocks(cugo_chol* s, int n_pairs, const int32_t* h_rows, const int32_t* h_cols, double* d_out);
/* Extension: the 3x3 marginal covariances of the free landmarks from the pose blocks of the inverse.  With
 * Hll_l = L L^T and G_e = Hpl_e L^-T,
 *   d_cov9[l] = L^-T (I + sum_{e, f} G_e^T Sigma_{p(e) p(f)} G_f) L^-1      (3x3, column-major, exactly symmetric),
 * e and f over the edge slots [lm_ptr[l], lm_ptr[l+1]) of landmark l that COUNT: those with none of
 * CUGO_EDGE_FIXED_L, CUGO_EDGE_FIXED_P, CUGO_EDGE_INACTIVE set.  Of every other slot only the flag is read: its pose
 * index and its Hpl block may hold anything.  A landmark without a counted edge gets Hll^-1.
 *   d_Hll [Lfree][9], d_Hpl [E][18] (double: CUGO_ERR_INVALID with ev->block_f32), as cugo_construct_quadratic_form
 *   leaves them (undamped);
 *   d_sigma [hs->n_blocks][36]: the blocks of the pose covariance on the pattern of hs (d_rowptr / d_colind: upper
 *   block CSR, diagonal block first, columns ascending), each 6x6 column-major with the rows of the block row — the
 *   layout cugo_chol_selected_inverse writes, diagonal blocks exactly symmetric as it writes them (the result is the
 *   lower triangle of the expression above, mirrored).  The pattern must hold the block (min, max) of every pair of poses that
 *   counted edges of one landmark join; Sigma_{ab} with a > b is read as the transpose of block (b, a).
 * d_fail[0] (int32, device) is zeroed here and set to 1 by every landmark whose Hll has a pivot <= 0 or a NaN in its
 * 3x3 Cholesky factorisation (a free landmark without any active edge at lambda = 0 among them): the block of such a
 * landmark is nine zeros, every other block is as without it.  Asynchronous on the context's stream; the flag stays on
 * the device, as cugo_chol_factor_solve leaves its own.  One thread per landmark, no atomics: the same bits on every
 * call.  CUGO_ERR_INVALID for a null argument; CUGO_OK with nothing launched when n_landmarks_free == 0. */
int cugo_landmark_covariances(cugo_ctx* ctx, const cugo_edges* ev, const cugo_hsc_struct* hs, const double* d_Hll,
                              const double* d_Hpl, const double* d_sigma, double* d_cov9 /* [9 * n_landmarks_free] */,
                              int32_t* d_fail);
/* Extension (g2o computeMarginals(spinv, blockIndices) / Ceres Covariance with mixed pairs): the pose-landmark blocks
 * of the covariance.  With Sigma_pp the pose covariance, Hll_l = L L^T and G_e = Hpl_e L^-T as above,
 *   Sigma_al = -(sum_e Sigma_{a p(e)} G_e) L^-1                              (6x3, column-major, rows a),
 * e over the counted slots of landmark l (as for cugo_landmark_covariances) in slot order.
 *
 * The plan of a batch of n queries (host only, no device needed).  h_lm_ptr [n_landmarks + 1] and h_slot_pose (the pose
 * index of every edge slot, landmark-major slot order; an index >= n_poses_free is a fixed pose) are those of the
 * flattened edges; query k is (h_q_pose[k], h_q_lm[k]): a free pose index, or -1 for a fixed pose, and a free landmark
 * index, or -1.  Named int32 arrays of the plan (cugo_plcov_plan_array returns the length or a negative error; the
 * pointer is valid until the plan is destroyed):
 *   "rows", "cols"   the distinct pose pairs to hand to cugo_chol_inverse_blocks, in the order of their first use:
 *                    (a, p(e)) for every slot of a query's landmark whose pose is free (whether or not the slot counts:
 *                    the kernel decides by flag), and (a, a) once per distinct free a.  One pose against every landmark
 *                    of a map gives at most n_poses_free + 1 pairs;
 *   "q_ptr" [n + 1], "q_slot"   per query one entry per slot of its landmark, in slot order: the index of the block
 *                    Sigma_{a p(e)} in that list, -1 for a slot on a fixed pose; an empty range for a query with a fixed
 *                    pose or a fixed landmark;
 *   "q_aa" [n]       the index of Sigma_aa, -1 for a fixed pose.
 * CUGO_ERR_INVALID for a null argument that is needed, a negative count or an index out of range. */
typedef struct cugo_plcov_plan cugo_plcov_plan;
int cugo_plcov_plan_create(int n_poses_free, int n_landmarks, const int32_t* h_lm_ptr, const int32_t* h_slot_pose, int n,
                           const int32_t* h_q_pose, const int32_t* h_q_lm, cugo_plcov_plan** out);
int cugo_plcov_plan_array(const cugo_plcov_plan* plan, const char* name, const int32_t** out);
void cugo_plcov_plan_destroy(cugo_plcov_plan* plan);
/* d_cov18 [n][18] = Sigma_al of the n queries (d_q_pose, d_q_lm, d_q_ptr, d_q_slot: device copies of the query lists and
 * of the plan's arrays).  d_blocks [.][36]: the blocks of the plan's pair list, each 6x6 column-major with rows a, as
 * cugo_chol_inverse_blocks writes them; only the blocks that counted slots refer to are read.  d_Hll, d_Hpl, ev as for
 * cugo_landmark_covariances (ev->d_lm_ptr and ev->d_flags are read; of a slot that does not count only the flag).
 * A query with a fixed vertex (an index of -1) gets 18 zeros: its range in d_q_slot is empty and no block is read.
 * d_fail[0] (int32, device) is zeroed here and set to 1 by every query whose free landmark's Hll has a pivot <= 0 or a
 * NaN in its 3x3 Cholesky factorisation (under a fixed pose too: the flag is about the landmark): that query gets 18
 * zeros, every other query is as without it.  A landmark that factors and has no counted slot gives zeros and no
 * failure.  Asynchronous on the context's stream; one thread per query, no atomics:
 * the same bits on every call.  CUGO_ERR_INVALID for a null argument, n < 0 or ev->block_f32; CUGO_OK with nothing
 * launched (the flag untouched) when n == 0. */
int cugo_pose_landmark_cross_covariances(cugo_ctx* ctx, const cugo_edges* ev, int n, const int32_t* d_q_pose,
                                         const int32_t* d_q_lm, const int32_t* d_q_ptr, const int32_t* d_q_slot,
                                         const double* d_Hll, const double* d_Hpl, const double* d_blocks,
                                         double* d_cov18, int32_t* d_fail);
/* Covariance of the predicted reprojection of landmark l in pose a at the estimates d_poses / d_lms:
 *   S = J_p Sigma_aa J_p^T + J_p Sigma_al J_l^T + (J_p Sigma_al J_l^T)^T + J_l Sigma_ll J_l^T
 * with the Jacobians of the projection as the build pass forms them (left update, tangent order [rotation,
 * translation]); no edge between a and l is needed.  Per query: d_q_pose / d_q_lm index d_poses [.][7] / d_lms [.][3]
 * (fixed vertices included); d_q_dim is 2 (mono) or 3 (stereo); d_cam5 [n][5] = fx, fy, cx, cy, bf; d_q_aa is the index
 * of Sigma_aa in d_blocks (the plan's "q_aa"), -1 for a fixed pose: the three terms with J_p go; a landmark index
 * >= n_landmarks_free is a fixed landmark: the terms with J_l go.  d_cross18 [n][18]: what
 * cugo_pose_landmark_cross_covariances wrote for the same queries; d_lmcov9 [n_landmarks_free][9]: what
 * cugo_landmark_covariances wrote.  d_cov9 [n][9]: 3x3 column-major, exactly symmetric (the lower triangle, mirrored);
 * for dim 2 the third row and column are zero.  Asynchronous, one thread per query.  CUGO_ERR_INVALID for a null
 * argument or a negative count; CUGO_OK with nothing launched when n == 0. */
int cugo_reprojection_covariances(cugo_ctx* ctx, int n, int n_landmarks_free, const int32_t* d_q_pose,
                                  const int32_t* d_q_lm, const int32_t* d_q_dim, const int32_t* d_q_aa,
                                  const double* d_cam5, const double* d_poses, const double* d_lms,
                                  const double* d_blocks, const double* d_cross18, const double* d_lmcov9, double* d_cov9);
/* Predicted observation z and its covariance S = J Sigma J^T (the sum above) for every camera kind the optimiser accepts.
 * Kind of a query, d_q_kind: */
#define CUGO_OBS_MONO 2   /* z = (u, v) */
#define CUGO_OBS_STEREO 3 /* z = (u, v, u_right) */
#define CUGO_OBS_DEPTH 4  /* z = (u, v, 1 / Z_s) */
/* Camera of a query: d_cam5 [n][5] = fx, fy, cx, cy, bf and, where d_cam_tab is not NULL, d_cam_tab [n][17] = {M row-major
 * (9), t_s (3), k1..k4, model}: the sensor pose body -> sensor and the projection model (0.0 pinhole, 1.0 Kannala-Brandt)
 * — the layout of a CUGO_RIG_MODELS camera table, one entry per query.  Geometry: Xb = R(q_a) X_l + t_a,
 * Xs = M Xb + t_s, z = the projection of Xs; J_p and J_l are the build pass's Jacobians of z - m: with A = -dz/dXs and
 * B = A M, J_p = [-B [Xb]x, B] and J_l = B R(q_a).  The depth row is that of 1 / Z_s with unit weight: S is in
 * measurement units, and the inverse-depth weight of a DepthEdgeSet belongs to the caller's noise term.  A depth kind
 * behind a sensor pose is defined here although the optimiser refuses such graphs.  A Kannala-Brandt entry has two
 * rows: with kind 3 or 4 it gives those and a zero third row and column (the edge kernels ignore the stereo bit
 * there).  d_z3 [n][3] (the third 0 where there is no third row) is written for every query, fixed vertices included;
 * d_cov9 [n][9] and every other argument as for cugo_reprojection_covariances.  With d_cam_tab == NULL and kinds 2 / 3
 * d_cov9 has the bits of cugo_reprojection_covariances.  Nothing is checked on the device: the caller keeps Z_s != 0
 * for pinhole entries and the point off the negative optical axis for Kannala-Brandt entries, or reads inf / NaN.
 * Asynchronous, one thread per query, the same bits on every call.  CUGO_ERR_INVALID for a null required argument or a
 * negative count; CUGO_OK with nothing launched when n == 0. */
int cugo_predict_observations(cugo_ctx* ctx, int n, int n_landmarks_free, const int32_t* d_q_pose, const int32_t* d_q_lm,
                              const int32_t* d_q_kind, const int32_t* d_q_aa, const double* d_cam5,
                              const double* d_cam_tab /* may be NULL */, const double* d_poses, const double* d_lms,
                              const double* d_blocks, const double* d_cross18, const double* d_lmcov9, double* d_z3,
                              double* d_cov9);
/* statistics of the analysis: nnz(L) in scalars, factorisation flops, #supernodes, #stages */
int cugo_chol_stats(const cugo_chol* s, double* nnzL, double* flops, int* n_supernodes,
                    int* n_stages, double* front_bytes);
/* symbolic plan export (host arrays) so tests can replay the plan with numpy.  A solver
 * created with ctx == NULL is host-only: analyze() builds the plan and skips the upload. */
int cugo_chol_plan_sizes(const cugo_chol* s, int* n, int* n_super, int* n_rows_total);
int cugo_chol_plan_get(const cugo_chol* s, int32_t* perm, int32_t* super_ptr, int32_t* rows_ptr,
                       int32_t* rows, int32_t* parent);
/* named int32 plan array ("perm", "super_ptr", "rows_ptr", "rows", "sparent", "child_ptr",
 * "child", "rel_ptr", "rel", "ncb", "nb", "col0", "col_front", "stage_task_ptr", "task_ptr",
 * "task_fronts", "blk_front", "blk_row", "blk_col", "blk_trans"; "stage_tile": per stage the edge of
 * its update tiles, 32 or 64, 0 for the two-phase form; "ea1": the potrf's child link
 * records, 16 ints each); pointer valid until the next analyze()/destroy. Returns the length or a
 * negative error. */
int cugo_chol_plan_array(cugo_chol* s, const char* name, const int32_t** out);
/* the same for the int64 per-front arrays of the storage layout: "off" (offset of the front in the
 * fronts buffer, doubles), "ldf" (its leading dimension), "woff" (offset of W = L11^-1), "l21off"
 * (offset of the compact L21, -1: in the front itself) */
int cugo_chol_plan_array64(cugo_chol* s, const char* name, const int64_t** out);

/* ref: gpu::schurComplementPost + updatePoses + updateLandmarks + computeScale
 * (cuda_block_solver.h:133-150; .cu:1419-1490).  Reads estimates from d_*_in, writes the
 * updated ("trial") estimates to d_*_out (push/pop of block_solver.cpp:431-439 becomes a
 * buffer swap).  d_scale[0] = sum_i x_i (lambda x_i + b_i) over [xp; xl].  Only the rows of FREE vertices of
 * d_poses_out / d_lms_out are written: the rows of fixed vertices are left untouched (the caller keeps them equal in
 * both buffers).  A free landmark without any edge slot gets a zero step. */
int cugo_backsubst_update(cugo_ctx* ctx, const cugo_edges* ev, double lambda,
                          const double* d_invHll, const double* d_bl, const double* d_bp,
                          const void* d_Hpl, const double* d_xp, double* d_xl,
                          const double* d_poses_in, const double* d_lms_in, double* d_poses_out,
                          double* d_lms_out, double* d_scale);

/* ---- the fused iteration at kernel level (DESIGN.md sections 4c / 4d) -------------------
 * The three passes in the forms the LM loop runs from its second iteration on, when the damping of the first trial is
 * known before the build pass is queued.  Call them in this order with the same ctx, ev, lambda and arrays.
 * form 1, two streams: the build pass also leaves d_invHll = (Hll + lambda I)^-1 and d_T = Hpl invHll, the bits
 *   cugo_compute_schur would form from the Hll and Hpl written here; every output of cugo_construct_quadratic_form is
 *   written as well.
 * form 2, one stream: with Hll + lambda I = L L^T per free landmark (a pivot that is not positive gives NaNs),
 *   d_Hll, d_bl, d_chi as in form 1;
 *   d_lmrec [Lfree][16]: the landmark's line {L^-1 (0,0) (1,0) (1,1) (2,0) (2,1) (2,2), y = L^-1 bl (3), 7 unused},
 *     written by the landmark's first edge slot: the line of a free landmark without any slot is left untouched;
 *   d_T [E][18] = G = Hpl L^-T (zero blocks for slots that are inactive or have a fixed endpoint);
 *   d_Hpp, d_bp, d_Hpl and d_invHll are NOT written (d_invHll must still be non-NULL; the others may be NULL).
 * The build pass also leaves one 64-byte record per edge slot in the context's scratch.  cugo_compute_schur_fused
 * (form 2) and cugo_backsubst_update_fused (from_records) read them: the records are valid from
 * cugo_construct_quadratic_form_fused until the next call on this context that is not one of these three entries, and
 * they belong to the ev, d_poses and lambda of that call; the caller vouches for this, nothing checks it.
 * h_lm_ptr: HOST copy of ev->d_lm_ptr [n_landmarks_total + 1].  CUGO_ERR_INVALID, with nothing launched, for
 * lambda < 0, an unknown form, a null array the form needs, or a landmark whose slots lie in two 256-slot groups (the
 * fused kernel sums a landmark inside one workgroup; the engine pads its slot layout so that none does). */
int cugo_construct_quadratic_form_fused(cugo_ctx* ctx, const cugo_edges* ev, const int32_t* h_lm_ptr,
                                        const double* d_poses, const double* d_lms, cugo_robust rk, double lambda,
                                        int form, double* d_Hpp, double* d_bp, double* d_Hll, double* d_bl, void* d_Hpl,
                                        double* d_invHll, void* d_T, double* d_lmrec, double* d_chi);
/* [Hsc | bsc] from what cugo_construct_quadratic_form_fused left for this lambda, by the gather kernels (CUGO_ERR_INVALID
 * if *hs carries a landmark-major plan).  form 1: cugo_compute_schur without its edge pass (d_invHll and d_T are read,
 * d_poses, d_lmrec and d_bp_out are not used).  form 2: the off-diagonal blocks are - sum G_i G_j^T with both operands
 * from d_T; the diagonal blocks (+ lambda I with damp_hsc_diag), d_bp_out [Pfree][6] = bp and d_bsc come from the
 * records, the lines d_lmrec and the poses d_poses the build pass linearised at; d_Hpp, d_bp, d_Hll, d_bl, d_Hpl and
 * d_invHll are not read.  The off-diagonal kernel is the context's (CUGO_HSC_MFMA / CUGO_HSC_XCD when it was created).
 * CUGO_ERR_INVALID, with nothing launched, for lambda < 0, an unknown form or a null array the form needs. */
int cugo_compute_schur_fused(cugo_ctx* ctx, const cugo_edges* ev, const cugo_hsc_struct* hs, double lambda,
                             int damp_hsc_diag, int form, const double* d_poses, const double* d_Hpp,
                             const double* d_bp, const double* d_Hll, const double* d_bl, const void* d_Hpl,
                             double* d_invHll, void* d_T, const double* d_lmrec, double* d_bp_out, double* d_bsc,
                             double* d_Hsc);
/* cugo_backsubst_update in the one-stream form: dx_l = L^-T (y - sum G_e^T dx_p) from the lines d_lmrec and d_G (what
 * form 2 left in d_T); everything else as cugo_backsubst_update.  from_records != 0: G_e^T dx_p is re-formed from the
 * records in the scratch, d_poses_in (which must be the poses of the build pass) and the lines instead of read from
 * d_G — the same bits.  CUGO_ERR_INVALID, with nothing launched, for lambda < 0 or a null array (d_lmrec included). */
int cugo_backsubst_update_fused(cugo_ctx* ctx, const cugo_edges* ev, double lambda, const double* d_lmrec,
                                const double* d_bl, const double* d_bp, const void* d_G, const double* d_xp,
                                double* d_xl, const double* d_poses_in, const double* d_lms_in, double* d_poses_out,
                                double* d_lms_out, double* d_scale, int from_records);

/*
 * Point-to-plane and point-to-line pose edges (the reference's include/icp_types.h: PlaneEdgeSet, LineEdgeSet):
 * unary edges on a pose.  With y = R(q) p + t (the pose read as the BA edges read it) and the left update in the
 * tangent order [omega, upsilon]:
 *   plane (normal n, offset d):        r = n.y - d,                        J = [ y x n | n^T ]      (1 x 6)
 *   line (point a, unit direction u):  r = (I - u u^T)(y - a) (3-vector),  J = (I - u u^T)[ -[y]x | I ]
 * chi2 term rho(omega |r|^2) with the kind's robust kernel, weight w = omega rho'(omega |r|^2).
 * The edges of each kind are SORTED by pose index (ascending), in structure-of-arrays form; pose_ptr is the CSR
 * over the pose index (the edges of pose p are [pose_ptr[p], pose_ptr[p+1])).  Edges on fixed poses (index >=
 * n_poses_free) and edges flagged CUGO_EDGE_INACTIVE contribute nothing.
 */
typedef struct cugo_icp_edges
{
    int n_poses_total, n_poses_free;
    int n_plane;
    const int32_t* d_plane_pose;     /* [n_plane] ascending */
    const int32_t* d_plane_pose_ptr; /* [n_poses_total+1] */
    const double* d_plane_p;         /* [3][n_plane] pointP */
    const double* d_plane_nd;        /* [4][n_plane] nx ny nz d */
    const double* d_plane_omega;     /* [n_plane] or [1] */
    int n_plane_omega;
    const uint8_t* d_plane_flags;    /* [n_plane] CUGO_EDGE_INACTIVE, or NULL: all active */
    int rk_plane;                    /* CUGO_RK_* */
    double delta_plane;
    int n_line;
    const int32_t* d_line_pose;
    const int32_t* d_line_pose_ptr;
    const double* d_line_p;          /* [3][n_line] pointP */
    const double* d_line_au;         /* [6][n_line] ax ay az ux uy uz (|u| = 1) */
    const double* d_line_omega;
    int n_line_omega;
    const uint8_t* d_line_flags;
    int rk_line;
    double delta_line;
} cugo_icp_edges;

/* ref: gpu::computeActiveErrors_Plane / _Line.  Writes the total chi2 of both kinds to d_chi[0]; with d_edge_chi
 * (optional, [n_plane + n_line], plane edges first, in the sorted order) also the chi2 term of every edge (0 for
 * edges that do not count).  Before launching, checks pose_ptr on the host (n_poses_total + 1 entries) and the pose
 * index of every edge against it on the device, and refuses a bad layout with CUGO_ERR_INVALID; the call therefore
 * synchronises once (one flag is read back).  The robust-kernel codes are checked; the values (finite, |u| = 1) are
 * the caller's, as for cugo_construct_quadratic_form.  Deterministic. */
int cugo_icp_compute_errors(cugo_ctx* ctx, const cugo_icp_edges* ev, const double* d_poses, double* d_chi,
                            double* d_edge_chi);

/* ref: gpu::constructQuadraticForm_Plane / _Line.  ADDS sum w J^T J to d_Hpp [n_poses_free][36] and -sum w J^T r
 * to d_bp [n_poses_free][6], J = dr/dxi: the layout and the sign of cugo_construct_quadratic_form, whose Jacobian is
 * d(meas - proj)/dxi, so that bp stays minus half the gradient of chi2 and the step of H dx = bp is applied as
 * exp(+dx) (cugo_backsubst_update).  Writes the chi2 total to d_chi[0] if d_chi != NULL (the bits of
 * cugo_icp_compute_errors).  Index checks as above.  No atomics. */
int cugo_icp_construct_quadratic_form(cugo_ctx* ctx, const cugo_icp_edges* ev, const double* d_poses, double* d_Hpp,
                                      double* d_bp, double* d_chi);

/* The same terms into the Schur destination, as the default LM loop adds them (the chunk pass, then the per-pose sums,
 * then the chi2 total: the launches of that loop).  d_rowptr [>= n_poses_free]: rowptr[p] is the BLOCK INDEX of pose p's
 * diagonal block in d_Hsc (the first block of row p of the upper block CSR of cugo_hsc_struct); sum w J^T J is ADDED to
 * that 6 x 6 column-major block and to no other, -sum w J^T r is ADDED to d_bp [n_poses_free][6] and, the same term, to
 * d_bsc [n_poses_free][6].  d_chi and the checks as above; rowptr is the caller's (it is not checked against a block
 * count).  The diagonal blocks and bp receive the bits cugo_icp_construct_quadratic_form adds to Hpp and bp. */
int cugo_icp_construct_quadratic_form_schur(cugo_ctx* ctx, const cugo_icp_edges* ev, const double* d_poses,
                                            const int32_t* d_rowptr, double* d_Hsc, double* d_bp, double* d_bsc, double* d_chi);

/*
 * Extension (the reference has no such edge): point-to-point pose edges, unary edges on a pose with a known 3-D point
 * p, its measurement z in the pose's frame and a full 3 x 3 information matrix Omega (symmetric, positive SEMI-definite:
 * singular matrices are legal).  Conventions as for cugo_icp_edges: y = R(q) p + t, left update, tangent order
 * [omega, upsilon]:
 *   r = y - z (3-vector),  J = dr/dxi = [ -[y]x | I ]  (3 x 6)
 *   chi2 term rho(max(0, r^T Omega r)) with the set's robust kernel, weight w = rho';  H += w J^T Omega J,
 *   b -= w J^T Omega r.
 * Omega = omega n n^T with n.z = d is the plane edge, Omega = omega (I - u u^T) with z = a the line edge.  With Omega =
 * (C_z + R C_p R^T)^-1 frozen per outer iteration the edge is that of generalised ICP.  The edges are SORTED by pose index
 * (ascending), structure of arrays; pose_ptr is the CSR over the pose index.  Edges on fixed poses (index >=
 * n_poses_free) and edges flagged CUGO_EDGE_INACTIVE contribute nothing.
 */
typedef struct cugo_point_edges
{
    int n_poses_total, n_poses_free;
    int n;
    const int32_t* d_pose;     /* [n] ascending */
    const int32_t* d_pose_ptr; /* [n_poses_total+1] */
    const double* d_p;         /* [3][n] the point p */
    const double* d_z;         /* [3][n] its measurement z */
    const double* d_info;      /* [6][n] or [6][1]: upper triangle of Omega, row-major packed 00 01 02 11 12 22 */
    int n_info;                /* n or 1 */
    const uint8_t* d_flags;    /* [n] CUGO_EDGE_INACTIVE, or NULL: all active */
    int rk;                    /* CUGO_RK_* */
    double delta;
} cugo_point_edges;

/* The three entry points of the ICP kinds, for the point edges: the chi2 total to d_chi[0] and, with d_edge_chi
 * (optional, [n], sorted order), the chi2 term of every edge (0 for edges that do not count); the terms ADDED to d_Hpp
 * [n_poses_free][36] / d_bp [n_poses_free][6]; the terms ADDED to the Schur destination (rowptr[p]: the block index of
 * pose p's diagonal block in d_Hsc; b to d_bp and to d_bsc alike; the diagonal blocks and bp receive the bits the plain
 * form adds).  The chi2 of a build pass has the bits of cugo_point_compute_errors.  A pose without a counting edge keeps
 * the bits of its blocks.  Before launching, pose_ptr is checked on the host and the pose index of every edge against
 * it on the device; a bad layout, an unknown kernel code or an n_info that is neither n nor 1 gives CUGO_ERR_INVALID
 * (one flag is read back: the call synchronises once).  The values (finite, Omega symmetric positive semi-definite)
 * are the caller's.  Deterministic, no atomics. */
int cugo_point_compute_errors(cugo_ctx* ctx, const cugo_point_edges* ev, const double* d_poses, double* d_chi,
                              double* d_edge_chi);
int cugo_point_construct_quadratic_form(cugo_ctx* ctx, const cugo_point_edges* ev, const double* d_poses, double* d_Hpp,
                                        double* d_bp, double* d_chi);
int cugo_point_construct_quadratic_form_schur(cugo_ctx* ctx, const cugo_point_edges* ev, const double* d_poses,
                                              const int32_t* d_rowptr, double* d_Hsc, double* d_bp, double* d_bsc,
                                              double* d_chi);

/*
 * Extension (the reference has no such edge): SE(3) pose priors, unary edges on a pose with a measurement
 * Z = (q_z, t_z) and a full 6 x 6 information matrix Omega (symmetric, positive semi-definite).  With the pose (q, t)
 * read as everywhere else and the left update T <- Exp([omega, upsilon]) T:
 *   R_D = R(q) R(q_z)^T, t_D = t - R_D t_z (D = T Z^-1);  r = [ Log_SO3(R_D) ; t_D ]  (the tangent order of the
 *   covariances of cugo_graph_get_pose_covariances);  J = dr/dxi = [ J_l^-1(phi) 0 ; -[t_D]x I ]
 *   chi2 term rho(max(0, r^T Omega r)) with the set's robust kernel, weight w = rho'.
 * At r = 0, J = I: a prior with Z = the estimate and Omega = Sigma^-1 is the Gaussian a marginal covariance describes.
 * The edges are SORTED by pose index (ascending), structure of arrays; pose_ptr is the CSR over the pose index.  Edges
 * on fixed poses (index >= n_poses_free) and edges flagged CUGO_EDGE_INACTIVE contribute nothing.
 */
typedef struct cugo_prior_edges
{
    int n_poses_total, n_poses_free;
    int n;
    const int32_t* d_pose;     /* [n] ascending */
    const int32_t* d_pose_ptr; /* [n_poses_total+1] */
    const double* d_meas;      /* [7][n] qx qy qz qw tx ty tz of Z */
    const double* d_info;      /* [21][n] or [21][1]: upper triangle of Omega, row-major packed (00 01 .. 05 11 ..) */
    int n_info;                /* n or 1 */
    const uint8_t* d_flags;    /* [n] CUGO_EDGE_INACTIVE, or NULL: all active */
    int rk;                    /* CUGO_RK_* */
    double delta;
} cugo_prior_edges;

/* Writes the chi2 total to d_chi[0]; with d_edge_chi (optional, [n], sorted order) also the chi2 term of every edge
 * (0 for edges that do not count).  Checks pose_ptr on the host and the pose index of every edge on the device before
 * launching, and refuses a bad layout or an unknown kernel code with CUGO_ERR_INVALID (one flag is read back: the
 * call synchronises once).  The values (finite, |q_z| = 1, Omega symmetric positive semi-definite) are the caller's.
 * Deterministic. */
int cugo_prior_compute_errors(cugo_ctx* ctx, const cugo_prior_edges* ev, const double* d_poses, double* d_chi,
                              double* d_edge_chi);

/* ADDS sum w J^T Omega J to d_Hpp [n_poses_free][36] and -sum w J^T Omega r to d_bp [n_poses_free][6], in the layout
 * and with the sign of cugo_construct_quadratic_form / cugo_icp_construct_quadratic_form.  Writes the chi2 total to
 * d_chi[0] if d_chi != NULL (the bits of cugo_prior_compute_errors).  A pose without priors keeps the bits of its
 * blocks.  Index checks as above.  No atomics. */
int cugo_prior_construct_quadratic_form(cugo_ctx* ctx, const cugo_prior_edges* ev, const double* d_poses, double* d_Hpp,
                                        double* d_bp, double* d_chi);

/* The same terms into the Schur destination (see cugo_icp_construct_quadratic_form_schur): rowptr[p] is the block index
 * of pose p's diagonal block in d_Hsc; b is ADDED to d_bp and to d_bsc alike.  A pose without a counting prior keeps the
 * bits of its blocks. */
int cugo_prior_construct_quadratic_form_schur(cugo_ctx* ctx, const cugo_prior_edges* ev, const double* d_poses,
                                              const int32_t* d_rowptr, double* d_Hsc, double* d_bp, double* d_bsc, double* d_chi);

/*
 * Extension (the reference has no such edge; g2o: EdgeXYZPrior): landmark position priors, unary edges on a landmark
 * with a measured position Z and a 3 x 3 information matrix Omega (symmetric, positive semi-definite):
 *   r = X - Z,  J = I,  chi2 term rho(max(0, r^T Omega r)) with the set's robust kernel,  w = rho'
 *   Hll += w Omega,  bl -= w Omega r          (sign and column-major blocks of cugo_construct_quadratic_form)
 * The priors are SORTED by landmark index (ascending), structure of arrays; lm_ptr is the CSR over ALL landmarks (the
 * priors of landmark l are [lm_ptr[l], lm_ptr[l+1])).  Priors on fixed landmarks (index >= n_landmarks_free) and priors
 * flagged CUGO_EDGE_INACTIVE contribute nothing.
 */
typedef struct cugo_lm_prior_edges
{
    int n_landmarks_total, n_landmarks_free;
    int n;
    const int32_t* d_lm;     /* [n] ascending */
    const int32_t* d_lm_ptr; /* [n_landmarks_total+1] */
    const double* d_meas;    /* [3][n] x y z of Z */
    const double* d_info;    /* [6][n] or [6][1]: upper triangle of Omega, row-major packed 00 01 02 11 12 22 */
    int n_info;              /* n or 1 */
    const uint8_t* d_flags;  /* [n] CUGO_EDGE_INACTIVE, or NULL: all active */
    int rk;                  /* CUGO_RK_* */
    double delta;
} cugo_lm_prior_edges;

/* Writes the chi2 total to d_chi[0]; with d_edge_chi (optional, [n], sorted order) also the chi2 term of every prior (0
 * for priors that do not count).  d_lms [n_landmarks_total][3].  Checks lm_ptr on the host and the landmark index of
 * every prior on the device before launching, and refuses a bad layout or an unknown kernel code with CUGO_ERR_INVALID
 * (one flag is read back: the call synchronises once).  The values (finite, Omega symmetric positive semi-definite) are
 * the caller's.  Deterministic. */
int cugo_lm_prior_compute_errors(cugo_ctx* ctx, const cugo_lm_prior_edges* ev, const double* d_lms, double* d_chi,
                                 double* d_edge_chi);

/* ADDS sum w Omega to d_Hll [n_landmarks_free][9] and -sum w Omega r to d_bl [n_landmarks_free][3], one lane per
 * landmark over its priors in sorted order.  Writes the chi2 total to d_chi[0] if d_chi != NULL (the bits of
 * cugo_lm_prior_compute_errors).  A landmark none of whose priors counts keeps the bits of its blocks.  Checks as
 * above.  No atomics. */
int cugo_lm_prior_construct_quadratic_form(cugo_ctx* ctx, const cugo_lm_prior_edges* ev, const double* d_lms, double* d_Hll,
                                           double* d_bl, double* d_chi);

/* cugo_construct_quadratic_form with the priors taken INSIDE the edge kernel of the build pass, the form the LM loop
 * uses: the lane that sums a landmark's Hll / bl adds the landmark's priors behind its edges, in sorted order.  d_Hll /
 * d_bl receive the bits of cugo_construct_quadratic_form followed by cugo_lm_prior_construct_quadratic_form; d_Hpp,
 * d_bp and d_Hpl those of cugo_construct_quadratic_form; d_chi[0], if given, the BA chi2 plus the priors' chi2.  lp must
 * describe the landmarks of ev (the same totals).  Checks as above. */
int cugo_construct_quadratic_form_lm_priors(cugo_ctx* ctx, const cugo_edges* ev, const cugo_lm_prior_edges* lp,
                                            const double* d_poses, const double* d_lms, cugo_robust rk, double* d_Hpp,
                                            double* d_bp, double* d_Hll, double* d_bl, void* d_Hpl, double* d_chi);

/*
 * Extension (the reference has no such edge): relative-pose SE(3) edges, binary edges between poses a and b with a
 * measurement Z = (q_z, t_z) ~ T_a T_b^-1 and a full 6 x 6 information matrix Omega (relpose_types.h).  Conventions as
 * for cugo_prior_edges:
 *   A = T_a T_b^-1 = (R_A, t_A),  D = A Z^-1,  r = [ Log_SO3(R_D) ; t_D ]
 *   J_a = [ J_l^-1(phi) 0 ; -[t_D]x I ] (the prior's J with this D),  J_b = -J_a Ad(A),  Ad(A) = [ R_A 0 ; [t_A]x R_A  R_A ]
 *   chi2 term rho(max(0, r^T Omega r)), w = rho';  H_aa += w J_a^T Omega J_a, H_bb += w J_b^T Omega J_b,
 *   H_(lo,hi) += w J_lo^T Omega J_hi (lo < hi the two pose indices),  b_a -= w J_a^T Omega r,  b_b -= w J_b^T Omega r
 * An edge with one fixed end (index >= n_poses_free) counts in chi2 and adds only its free end's block and b; an edge
 * between two fixed poses, or flagged CUGO_EDGE_INACTIVE, counts for nothing.  The edges stay in the caller's order:
 * the library's own plan (below) holds what every free pose walks and where the off-diagonal block of an edge goes.
 *
 * The plan.  h_* are HOST arrays: the two pose indices and the flags of every edge (h_flags may be NULL: all active),
 * and an upper block-CSR pattern over the free poses, the diagonal block first in every row and the columns of a row
 * ascending — the layout cugo_chol_analyze takes and cugo_hsc_struct describes.  Refused with CUGO_ERR_INVALID: an
 * index outside [0, n_poses_total), a == b, a pattern of another form, and a counting edge between two free poses
 * whose (lo, hi) block the pattern lacks.  The plan holds, per free pose, its counting edges with the side each is seen
 * from, in edge order, and, per edge, the block index of its off-diagonal destination or -1, and uploads both with the
 * index arrays.  ctx == NULL gives a host-only plan (cugo_relpose_plan_array reads it; the kernels refuse it).
 */
typedef struct cugo_relpose_plan cugo_relpose_plan;
int cugo_relpose_plan_create(cugo_ctx* ctx, int n, int n_poses_total, int n_poses_free, const int32_t* h_pose_a,
                             const int32_t* h_pose_b, const uint8_t* h_flags, const int32_t* h_rowptr,
                             const int32_t* h_colind, cugo_relpose_plan** out);
void cugo_relpose_plan_destroy(cugo_relpose_plan* plan);
/* named int32 plan array: "inc_ptr" [n_poses_free + 1], "inc" [inc_ptr[n_poses_free]] (edge << 1 | side; side 0: the
 * pose is the edge's a, 1: its b), "off_blk" [n].  The pointer is valid until the plan is destroyed.  Returns the
 * length or a negative error. */
int cugo_relpose_plan_array(const cugo_relpose_plan* plan, const char* name, const int32_t** out);
/* The upper block-CSR pattern of a pure pose graph (host arrays): row p holds p, then every hi > p that a counting
 * edge between two free poses joins to p.  rowptr_out [n_poses_free + 1] and colind_out may each be NULL; *nnzb
 * receives the block count either way (call once for the size, once more with colind_out [*nnzb]).  Indices >=
 * n_poses_free are fixed poses.  CUGO_ERR_INVALID on a negative index or a == b. */
int cugo_relpose_pattern(int n, int n_poses_free, const int32_t* h_pose_a, const int32_t* h_pose_b,
                         const uint8_t* h_flags, int32_t* rowptr_out, int32_t* colind_out, int* nnzb);

typedef struct cugo_relpose_edges
{
    int n_poses_total, n_poses_free; /* those of the plan */
    int n;                           /* that of the plan */
    const double* d_meas;            /* [7][n] qx qy qz qw tx ty tz of Z */
    const double* d_info;            /* [21][n] or [21][1]: upper triangle of Omega, row-major packed */
    int n_info;                      /* n or 1 */
    const uint8_t* d_flags;          /* [n] CUGO_EDGE_INACTIVE, or NULL.  The plan lists the edges that counted under
                                        ITS flags: an edge it left out stays out; one flagged here in addition counts
                                        for nothing */
    int rk;                          /* CUGO_RK_* */
    double delta;
    const cugo_relpose_plan* plan;   /* with a device context */
} cugo_relpose_edges;

/* Writes the chi2 total to d_chi[0] (every counting edge once); with d_edge_chi (optional, [n], edge order) also the
 * chi2 term of every edge (0 for edges that do not count).  The layout is the plan's, so no index check runs on the
 * device; the counts, the arrays and the robust-kernel code are checked (CUGO_ERR_INVALID).  One launch plus the chi2
 * total.  Deterministic: no atomics, one summation order. */
int cugo_relpose_compute_errors(cugo_ctx* ctx, const cugo_relpose_edges* ev, const double* d_poses, double* d_chi,
                                double* d_edge_chi);
/* ADDS the diagonal terms to d_Hpp [n_poses_free][36] and b to d_bp [n_poses_free][6] (layout and sign of
 * cugo_prior_construct_quadratic_form), and the off-diagonal terms to d_Hoff [nnzb][36]: block k of the plan's pattern,
 * 6 x 6 column-major, holds H_(lo,hi) (rows: pose lo); the diagonal blocks of d_Hoff are not touched.  Edges on the
 * same pair, in either orientation, are summed into one block.  A free pose without a counting edge and a block no
 * counting edge maps to keep their bits.  chi2 total to d_chi[0] if d_chi != NULL (the bits of
 * cugo_relpose_compute_errors).  d_Hoff may be NULL when no edge joins two free poses. */
int cugo_relpose_construct_quadratic_form(cugo_ctx* ctx, const cugo_relpose_edges* ev, const double* d_poses,
                                          double* d_Hpp, double* d_bp, double* d_Hoff, double* d_chi);
/* The same terms into the Schur destination: the diagonal term of pose p into block d_rowptr[p] of d_Hsc (see
 * cugo_icp_construct_quadratic_form_schur), the off-diagonal terms into d_Hsc by the plan's block indices, b into d_bp
 * and d_bsc alike.  d_Hsc must be laid out by the pattern the plan was built against. */
int cugo_relpose_construct_quadratic_form_schur(cugo_ctx* ctx, const cugo_relpose_edges* ev, const double* d_poses,
                                                const int32_t* d_rowptr, double* d_Hsc, double* d_bp, double* d_bsc,
                                                double* d_chi);

/* The two launches the two-stream form of the LM loop makes of the same terms.  The build pass: the diagonal terms and
 * b ADDED to d_Hpp / d_bp as cugo_relpose_construct_quadratic_form adds them, the off-diagonal terms stored nowhere ... */
int cugo_relpose_construct_quadratic_form_diag(cugo_ctx* ctx, const cugo_relpose_edges* ev, const double* d_poses,
                                               double* d_Hpp, double* d_bp, double* d_chi);
/* ... and, behind a Schur pass (which has written every block of d_Hsc), the off-diagonal terms alone ADDED to d_Hsc by
 * the plan's block indices, at the same poses: the terms, in the order, of cugo_relpose_construct_quadratic_form_schur.
 * Nothing else is written.  Deterministic: no atomics, one summation order. */
int cugo_relpose_add_offdiag_schur(cugo_ctx* ctx, const cugo_relpose_edges* ev, const double* d_poses, double* d_Hsc);

/*
 * Extension (the reference has no such edge): pose-pose point edges, binary edges between poses a and b for scan-to-scan
 * registration.  An edge carries a point p measured in a's frame, the same physical point measured as z in b's frame,
 * and a 3 x 3 information matrix Omega (symmetric, positive SEMI-definite: singular matrices are legal) expressed in
 * b's frame.  Conventions as for cugo_point_edges: y = R(q) X + t is world -> frame, left update, tangent order
 * [omega, upsilon]:
 *   X = R_a^T (p - t_a),  y = R_b X + t_b,  r = y - z
 *   J_b = dr/dxi_b = [ -[y]x | I ]  (the Jacobian of cugo_point_edges),  J_a = dr/dxi_a = R_BA [ [p]x | -I ],  R_BA = R_b R_a^T
 *   chi2 term rho(max(0, r^T Omega r)) with the set's robust kernel, w = rho';  H_aa += w J_a^T Omega J_a,
 *   H_bb += w J_b^T Omega J_b,  H_(lo,hi) += w J_lo^T Omega J_hi (lo < hi the two pose indices),  b_a -= w J_a^T Omega r,
 *   b_b -= w J_b^T Omega r
 * With T_a the identity the term on pose b is that of the cugo_point_edges edge (p, z, Omega).  An edge with one fixed
 * end (index >= n_poses_free) counts in chi2 and adds only its free end's block and b; an edge between two fixed poses,
 * or flagged CUGO_EDGE_INACTIVE, counts for nothing.
 *
 * The plan.  h_* are HOST arrays in the caller's order: the two pose indices and the flags of every edge (h_flags may be
 * NULL: all active) and an upper block-CSR pattern over the free poses, as for cugo_relpose_plan_create (h_rowptr and
 * h_colind may both be NULL: a plan without a destination, for its "pair_lo" / "pair_hi" alone; the kernels refuse it).
 * The plan sorts the edges, stably, into RUNS: one run per (a, b) orientation of a pose pair, ordered by (lo, hi,
 * orientation) so that the runs of one block are adjacent.  It holds the permutation, the runs, per free pose the
 * counting runs its diagonal block is summed from, per block touched its runs, and the distinct pairs.  The same
 * refusals as cugo_relpose_plan_create (CUGO_ERR_INVALID).  ctx == NULL gives a host-only plan.
 */
typedef struct cugo_point_pair_plan cugo_point_pair_plan;
int cugo_point_pair_plan_create(cugo_ctx* ctx, int n, int n_poses_total, int n_poses_free, const int32_t* h_pose_a,
                                const int32_t* h_pose_b, const uint8_t* h_flags, const int32_t* h_rowptr,
                                const int32_t* h_colind, cugo_point_pair_plan** out);
void cugo_point_pair_plan_destroy(cugo_point_pair_plan* plan);
/* named int32 plan array: "perm" [n] (container index of the edge at sorted position i), "edge_run" [n], "run_ptr"
 * [n_runs + 1], "run_a", "run_b", "run_flags" (1: a free, 2: b free, 4: a is hi, 8: the run counts), "run_blk" [n_runs],
 * "inc_ptr" [n_poses_free + 1], "inc" (run << 1 | side; side 0: the pose is the run's a), "blk_id" [n_touched], "blk_ptr"
 * [n_touched + 1], "blk_run", "pair_lo", "pair_hi".  The pointer is valid until the plan is destroyed.  Returns the
 * length or a negative error. */
int cugo_point_pair_plan_array(const cugo_point_pair_plan* plan, const char* name, const int32_t** out);

/* The edges in the plan's SORTED order (position i holds edge perm[i] of the container), structure of arrays. */
typedef struct cugo_point_pair_edges
{
    int n_poses_total, n_poses_free; /* those of the plan */
    int n;                           /* that of the plan */
    const int32_t* d_pose_a;         /* [n] pose a of every edge, sorted order */
    const int32_t* d_pose_b;         /* [n] pose b */
    const double* d_p;               /* [3][n] the point in a's frame */
    const double* d_z;               /* [3][n] its measurement in b's frame */
    const double* d_info;            /* [6][n] or [6][1]: upper triangle of Omega, row-major packed 00 01 02 11 12 22 */
    int n_info;                      /* n or 1 */
    const uint8_t* d_flags;          /* [n] CUGO_EDGE_INACTIVE, or NULL, sorted order.  A run that did not count under
                                        the PLAN's flags stays out; an edge flagged here in addition counts for nothing */
    int rk;                          /* CUGO_RK_* */
    double delta;
    const cugo_point_pair_plan* plan; /* with a device context and a pattern */
} cugo_point_pair_edges;

/* Writes the chi2 total to d_chi[0] (every counting edge once); with d_edge_chi (optional, [n], sorted order) also the
 * chi2 term of every edge (0 for edges that do not count).  The counts, the arrays and the robust-kernel code are checked
 * on the host, d_pose_a / d_pose_b of every edge against the plan's runs on the device; a mismatch gives
 * CUGO_ERR_INVALID with nothing launched (one flag is read back: the call synchronises once).  Deterministic: no atomics,
 * one summation order. */
int cugo_point_pair_compute_errors(cugo_ctx* ctx, const cugo_point_pair_edges* ev, const double* d_poses, double* d_chi,
                                   double* d_edge_chi);
/* ADDS the diagonal terms to d_Hpp [n_poses_free][36] and b to d_bp [n_poses_free][6] (layout and sign of
 * cugo_point_construct_quadratic_form) and the off-diagonal terms to d_Hoff [nnzb][36]: block k of the plan's pattern, 6 x
 * 6 column-major, holds H_(lo,hi) (rows: pose lo); the diagonal blocks of d_Hoff are not touched.  The two runs of a
 * pair are summed into one block.  A free pose without a counting run and a block no counting run maps to keep their
 * bits; fixed ends are never written.  chi2 total to d_chi[0] if d_chi != NULL (the bits of
 * cugo_point_pair_compute_errors).  d_Hoff may be NULL when no counting run joins two free poses. */
int cugo_point_pair_construct_quadratic_form(cugo_ctx* ctx, const cugo_point_pair_edges* ev, const double* d_poses,
                                             double* d_Hpp, double* d_bp, double* d_Hoff, double* d_chi);
/* The same terms into the Schur destination: the diagonal term of pose p into block d_rowptr[p] of d_Hsc, the
 * off-diagonal terms into d_Hsc by the plan's block indices, b into d_bp and d_bsc alike. */
int cugo_point_pair_construct_quadratic_form_schur(cugo_ctx* ctx, const cugo_point_pair_edges* ev, const double* d_poses,
                                                   const int32_t* d_rowptr, double* d_Hsc, double* d_bp, double* d_bsc,
                                                   double* d_chi);
/* The split a two-stream LM loop makes of the same terms.  The build pass: the diagonal terms and b ADDED to d_Hpp / d_bp;
 * the off-diagonal partials stay in the plan's scratch (a plan made with a context owns the scratch of its passes) ... */
int cugo_point_pair_construct_quadratic_form_diag(cugo_ctx* ctx, const cugo_point_pair_edges* ev, const double* d_poses,
                                                  double* d_Hpp, double* d_bp, double* d_chi);
/* ... and the off-diagonal sums of those partials ADDED to d_Hsc by the plan's block indices.  It reads the PARTIALS the
 * last cugo_point_pair_construct_quadratic_form* call left in the plan's scratch, not the poses (CUGO_ERR_INVALID before
 * any such call); cugo_point_pair_compute_errors in between does not disturb them.  Nothing else is written.  The sums
 * and their order are those of the Schur form. */
int cugo_point_pair_add_offdiag_schur(cugo_ctx* ctx, const cugo_point_pair_edges* ev, double* d_Hsc);

/*
 * Extension (the reference has no such edge): the COVARIANCE form of the two point kinds, the cost of generalised ICP.
 * An edge carries two covariances instead of an information matrix, and Omega follows the poses:
 *   S = C_z + M C_p M^T,  Omega = S^-1,   M = R (unary: C_p in the world frame, C_z in the pose's frame)
 *                                         M = R_b R_a^T (pair: C_p in a's frame, C_z in b's frame)
 * formed at the poses every pass is given: the chi2 of an error pass is the cost at those poses, the H and b of a build
 * pass use the Omega of the linearisation point.  r, J, x = max(0, r^T Omega r), rho, w and the blocks of H and b are
 * those of cugo_point_edges / cugo_point_pair_edges with this Omega.  The Jacobian does NOT differentiate Omega (no GICP
 * implementation does), and log det S is not part of the cost.  S is formed as an upper triangle and mirrored, and
 * inverted through its 3 x 3 L L^T factor.
 * d_cov_p, d_cov_z: [6][n] or [6][1], the upper triangle row-major packed 00 01 02 11 12 22 (the layout of d_info); n_cov
 * is the count of BOTH.  Every other member, the sorted layout, the plan, the checks, the error codes, d_edge_chi and
 * the invariants (no atomics, one summation order, error-pass chi2 bits = build-pass chi2 bits, what has no counting
 * edge or run keeps its bits, fixed ends are never written) are those of the information form; an n_cov that is neither
 * n nor 1 gives CUGO_ERR_INVALID.  The values are the caller's: covariances symmetric positive semi-definite with S
 * positive definite (lambda_min(C_p) + lambda_min(C_z) > 0 suffices for every rotation); an S that is not gives NaNs.
 */
typedef struct cugo_gicp_edges
{
    int n_poses_total, n_poses_free;
    int n;
    const int32_t* d_pose;     /* [n] ascending */
    const int32_t* d_pose_ptr; /* [n_poses_total+1] */
    const double* d_p;         /* [3][n] the point p (world) */
    const double* d_z;         /* [3][n] its measurement z (the pose's frame) */
    const double* d_cov_p;     /* [6][n] or [6][1]: upper triangle of C_p (world frame) */
    const double* d_cov_z;     /* [6][n] or [6][1]: upper triangle of C_z (the pose's frame) */
    int n_cov;                 /* n or 1 */
    const uint8_t* d_flags;    /* [n] CUGO_EDGE_INACTIVE, or NULL: all active */
    int rk;                    /* CUGO_RK_* */
    double delta;
} cugo_gicp_edges;

/* as cugo_point_compute_errors / _construct_quadratic_form / _construct_quadratic_form_schur */
int cugo_gicp_compute_errors(cugo_ctx* ctx, const cugo_gicp_edges* ev, const double* d_poses, double* d_chi,
                             double* d_edge_chi);
int cugo_gicp_construct_quadratic_form(cugo_ctx* ctx, const cugo_gicp_edges* ev, const double* d_poses, double* d_Hpp,
                                       double* d_bp, double* d_chi);
int cugo_gicp_construct_quadratic_form_schur(cugo_ctx* ctx, const cugo_gicp_edges* ev, const double* d_poses,
                                             const int32_t* d_rowptr, double* d_Hsc, double* d_bp, double* d_bsc,
                                             double* d_chi);

/* The pair kind, in the SORTED order of its plan (cugo_point_pair_plan_create: the plan does not depend on the form). */
typedef struct cugo_gicp_pair_edges
{
    int n_poses_total, n_poses_free; /* those of the plan */
    int n;                           /* that of the plan */
    const int32_t* d_pose_a;         /* [n] pose a of every edge, sorted order */
    const int32_t* d_pose_b;         /* [n] pose b */
    const double* d_p;               /* [3][n] the point in a's frame */
    const double* d_z;               /* [3][n] its measurement in b's frame */
    const double* d_cov_p;           /* [6][n] or [6][1]: upper triangle of C_p (a's frame) */
    const double* d_cov_z;           /* [6][n] or [6][1]: upper triangle of C_z (b's frame) */
    int n_cov;                       /* n or 1 */
    const uint8_t* d_flags;          /* as cugo_point_pair_edges.d_flags */
    int rk;                          /* CUGO_RK_* */
    double delta;
    const cugo_point_pair_plan* plan; /* with a device context and a pattern */
} cugo_gicp_pair_edges;

/* as the cugo_point_pair_* call of the same name.  The partials a build pass leaves in the plan's scratch are those of
 * the form that ran last: cugo_gicp_pair_add_offdiag_schur adds what the last build pass over the plan left. */
int cugo_gicp_pair_compute_errors(cugo_ctx* ctx, const cugo_gicp_pair_edges* ev, const double* d_poses, double* d_chi,
                                  double* d_edge_chi);
int cugo_gicp_pair_construct_quadratic_form(cugo_ctx* ctx, const cugo_gicp_pair_edges* ev, const double* d_poses,
                                            double* d_Hpp, double* d_bp, double* d_Hoff, double* d_chi);
int cugo_gicp_pair_construct_quadratic_form_schur(cugo_ctx* ctx, const cugo_gicp_pair_edges* ev, const double* d_poses,
                                                  const int32_t* d_rowptr, double* d_Hsc, double* d_bp, double* d_bsc,
                                                  double* d_chi);
int cugo_gicp_pair_construct_quadratic_form_diag(cugo_ctx* ctx, const cugo_gicp_pair_edges* ev, const double* d_poses,
                                                 double* d_Hpp, double* d_bp, double* d_chi);
int cugo_gicp_pair_add_offdiag_schur(cugo_ctx* ctx, const cugo_gicp_pair_edges* ev, double* d_Hsc);

/*
 * Outlier pass of the four pose edge kinds (ref: EdgeSet::updateEdges, optimisable_graph.hpp:603-640), over the chi2
 * term of every edge as cugo_icp_compute_errors / cugo_prior_compute_errors / cugo_relpose_compute_errors write it.
 * Edge e becomes an outlier iff !(d_flags[e] & CUGO_EDGE_INACTIVE) && t_e > 0 && d_edge_chi[e] > t_e
 * (t_e = d_threshold[n_threshold == 1 ? 0 : e]; strict '>', ref: computeOutliersKernel, cuda_block_solver.cu:1145;
 * a NaN chi2 is therefore kept, +inf goes).  For those edges d_flags[e] |= CUGO_EDGE_INACTIVE; no other bit and no
 * other byte changes.  d_rejected[0 .. *n_rejected) receives their indices in ASCENDING order; entries behind
 * them are not written.  One host synchronisation (the count).  n == 0: nothing is launched.
 * On the device: a count pass, a scan of the workgroups' counts and a place pass, lane per edge; positions come from
 * ballots and fixed-order integer sums, so two calls on equal inputs give equal bytes (no atomics, no floating-point
 * arithmetic).  Up to 1024 workgroups of 256 edges; beyond 262144 edges every workgroup walks several runs of 256.
 * CUGO_ERR_INVALID: a null array with n > 0, n_threshold other than 1 or n, n < 0 or n > 2^26.
 */
int cugo_pose_edges_reject(cugo_ctx* ctx, int n, const double* d_edge_chi, const double* d_threshold, int n_threshold,
                           uint8_t* d_flags, int32_t* d_rejected /* [n] */, int* n_rejected);

/* ---- (2) graph-level entry points ---------------------------------------------------- */

typedef struct cugo_graph cugo_graph; /* CudaGraphOptimisationImpl + its vertex/edge sets */

/* ref: CudaGraphOptimisationImpl(options) include/cuda_graph_optimisation.h:206;
 * GraphOptimisationOptions src/graph_optimisation_options.h:8-19 */
int cugo_graph_create(int per_edge_information, int per_edge_camera, cugo_graph** out);
/* Extension: a plan-only graph needs no GPU.  cugo_graph_initialize() then runs the host side only —
 * flattening and index assignment (ref: src/block_solver.cpp:21-137), Hsc pattern and product lists
 * (ref: src/sparse_block_matrix.cpp:63-156), ordering + symbolic factorisation (ref:
 * src/cholesky.hpp:97-98,295-296) — and cugo_graph_structure_stats() reports the result;
 * cugo_graph_optimize() fails.  Sizes a problem ahead of time; also what `make SAN=1` exercises. */
int cugo_graph_create_plan_only(int per_edge_information, int per_edge_camera, cugo_graph** out);
void cugo_graph_destroy(cugo_graph* g);
/* vertices: ids are caller ids (ref: PoseVertex(id, Se3D, fixed), LandmarkVertex(id, Vec3d,
 * fixed); src/optimisable_graph.h:109-155) */
int cugo_graph_add_poses(cugo_graph* g, int n, const int32_t* ids, const double* q_t7,
                         const uint8_t* fixed);
int cugo_graph_add_landmarks(cugo_graph* g, int n, const int32_t* ids, const double* xyz,
                             const uint8_t* fixed);
/* edges: dim = 2 -> MonoEdgeSet, 3 -> StereoEdgeSet (ref: include/ba_types.h:34-169,238-254).
 * meas is [n][dim]; info [n]; cam [n][5] or NULL to use the set camera. */
int cugo_graph_add_edges(cugo_graph* g, int dim, int n, const int32_t* pose_ids,
                         const int32_t* landmark_ids, const double* meas, const double* info,
                         const double* cam5);
int cugo_graph_set_camera(cugo_graph* g, int dim, const double* cam5);
int cugo_graph_set_information(cugo_graph* g, int dim, double info);
int cugo_graph_set_robust_kernel(cugo_graph* g, int dim, int type, double delta);
/* Extension: camera extrinsics (a multi-camera rig; cugo_edges.has_rig).  The poses are then world -> body, and a
 * camera carries a fixed sensor pose body -> sensor, q_t7 = (qx, qy, qz, qw, tx, ty, tz): Xs = R(q) Xb + t.  The
 * extrinsic follows the camera: cugo_graph_set_sensor_pose sets that of the mono (dim 2) or stereo (dim 3) set;
 * cugo_graph_add_edges_rig is cugo_graph_add_edges with a sensor pose per edge, sensor_q_t7 [n][7].  Like cam5 it
 * counts on a graph created with per_edge_camera (NULL: these edges keep the identity) and is not looked at on a
 * graph without, where the set's applies.  The default is the identity, and a graph whose sensor
 * poses are all identities runs the kernels it has always run.  cugo_graph_initialize normalises the quaternion and
 * refuses one that is not finite or has norm 0, sensor poses together with depth edges (not yet) and on a
 * landmark-sharded graph (not yet).  Pose priors, relative-pose and ICP edges act on the pose vertex: the body.
 * cugo_graph_reprojection_covariances keeps describing a camera at the pose; cugo_graph_predict_observations answers
 * for the camera behind its sensor pose.
 * cugo_graph_n_rig_cameras: entries of the camera table of the current flattening whose sensor pose is not the
 * identity.  cugo_graph_get_flat_cameras (diagnostic): that table — returns the number of entries and fills the first
 * `cap` of cam5 [cap][5] and ext12 [cap][12] = {M row-major, t} where not NULL; *has_rig: what the edge kernels get. */
int cugo_graph_set_sensor_pose(cugo_graph* g, int dim, const double* q_t7);
int cugo_graph_add_edges_rig(cugo_graph* g, int dim, int n, const int32_t* pose_ids, const int32_t* landmark_ids,
                             const double* meas, const double* info, const double* cam5, const double* sensor_q_t7);
int cugo_graph_n_rig_cameras(cugo_graph* g);
int cugo_graph_get_flat_cameras(cugo_graph* g, int cap, double* cam5, double* ext12, int* has_rig);
/* Extension: camera models (Kannala-Brandt fisheye; cugo_edges.has_rig == CUGO_RIG_MODELS).  model: 0 pinhole (the
 * default), 1 Kannala-Brandt with coefficients k4 = (k1, k2, k3, k4) (NULL: zeros, the equidistant model).  Like the
 * sensor pose the model follows the camera: cugo_graph_set_camera_model sets that of the mono (dim 2) or stereo (dim 3)
 * set; cugo_graph_add_edges_model is cugo_graph_add_edges with, per edge, a camera cam5 [n][5], a sensor pose
 * sensor_q_t7 [n][7] and a model model_k5 [n][5] = (k1, k2, k3, k4, model) — each of the three may be NULL and counts
 * on a graph created with per_edge_camera only.  A graph whose models are all pinhole runs the kernels it ran before.
 * cugo_graph_initialize refuses a Kannala-Brandt model on stereo edges, together with depth edges (not yet), on a
 * landmark-sharded graph (not yet), and coefficients that are not finite.
 * cugo_graph_reprojection_covariances keeps describing a pinhole camera at the pose; cugo_graph_predict_observations
 * answers for a Kannala-Brandt camera.
 * cugo_graph_n_fisheye_cameras: entries of the camera table of the current flattening whose model is Kannala-Brandt.
 * cugo_graph_get_flat_camera_models (diagnostic): returns the number of entries of that table and fills the first
 * `cap` of model_k5 [cap][5] = (k1, k2, k3, k4, model) where not NULL; parallel to cugo_graph_get_flat_cameras. */
int cugo_graph_set_camera_model(cugo_graph* g, int dim, int model, const double* k4);
int cugo_graph_add_edges_model(cugo_graph* g, int dim, int n, const int32_t* pose_ids, const int32_t* landmark_ids,
                               const double* meas, const double* info, const double* cam5, const double* sensor_q_t7,
                               const double* model_k5);
int cugo_graph_n_fisheye_cameras(cugo_graph* g);
int cugo_graph_get_flat_camera_models(cugo_graph* g, int cap, double* model_k5);
/* Extension: radial-tangential lens distortion (cugo_edges.has_rig == CUGO_RIG_DISTORTION).  d5 = (k1, k2, p1, p2, k3)
 * in OpenCV's order and meaning (NULL: zeros, no distortion); measurements on a distorted camera are raw pixels.  Like
 * the sensor pose the distortion follows the camera: cugo_graph_set_camera_distortion sets that of the mono (dim 2) or
 * stereo (dim 3) set; cugo_graph_add_edges_distorted is cugo_graph_add_edges with, per edge, a camera cam5 [n][5], a
 * sensor pose sensor_q_t7 [n][7] and a distortion dist5 [n][5] — each of the three may be NULL and counts on a graph
 * created with per_edge_camera only.  A graph whose distortions are all zero runs the kernels it ran before.
 * cugo_graph_initialize refuses a non-zero distortion on stereo edges, together with depth edges (not yet), on a camera
 * with a Kannala-Brandt model, in a graph that also has Kannala-Brandt cameras (not yet), on a landmark-sharded graph
 * (not yet), and coefficients that are not finite.  cugo_graph_predict_observations with cam5 == NULL refuses a set
 * whose distortion is not zero (a distorted kind there is a later step); with cam5 given it keeps describing an
 * undistorted camera at the pose, as cugo_graph_reprojection_covariances does.
 * cugo_graph_n_distorted_cameras: entries of the camera table of the current flattening whose distortion is not zero.
 * cugo_graph_get_flat_camera_distortions (diagnostic): returns the number of entries of that table and fills the first
 * `cap` of dist5 [cap][5] = (k1, k2, p1, p2, k3) where not NULL; parallel to cugo_graph_get_flat_cameras. */
int cugo_graph_set_camera_distortion(cugo_graph* g, int dim, const double* d5);
int cugo_graph_add_edges_distorted(cugo_graph* g, int dim, int n, const int32_t* pose_ids, const int32_t* landmark_ids,
                                   const double* meas, const double* info, const double* cam5, const double* sensor_q_t7,
                                   const double* dist5);
int cugo_graph_n_distorted_cameras(cugo_graph* g);
int cugo_graph_get_flat_camera_distortions(cugo_graph* g, int cap, double* dist5);
/* Point-to-plane / point-to-line pose edges (the reference's PlaneEdgeSet / LineEdgeSet, include/icp_types.h), next to
 * or instead of the BA edges; residuals and conventions as for cugo_icp_edges above.  pointP [n][3]; plane: unit normal
 * [n][3] (used as given) and origin_distance [n]; line: two distinct points a, b [n][3]; info [n] or NULL (the set's
 * value).  pose_ids must be ids given to cugo_graph_add_poses.  cugo_graph_initialize() refuses non-finite values, a
 * normal whose length differs from 1 by more than 1e-6, a == b, an outlier threshold on these sets unless the option
 * "pose_edge_outliers" is on (cugo_graph_set_option) and a sharded optimiser; edges on fixed poses count for nothing.  The existing setters select a set by dim, which cannot tell the
 * two kinds apart (both are 1-d): the two setters below take the kind. */
#define CUGO_ICP_PLANE 0
#define CUGO_ICP_LINE 1
int cugo_graph_add_plane_edges(cugo_graph* g, int n, const int32_t* pose_ids, const double* pointP,
                               const double* normal, const double* origin_distance, const double* info);
int cugo_graph_add_line_edges(cugo_graph* g, int n, const int32_t* pose_ids, const double* pointP, const double* a,
                              const double* b, const double* info);
int cugo_graph_set_icp_information(cugo_graph* g, int kind, double info);
int cugo_graph_set_icp_robust_kernel(cugo_graph* g, int kind, int type, double delta);
/* outlier threshold of an ICP set (ref: EdgeSet::setOutlierThreshold).  With cugo_graph_set_option(g,
 * "pose_edge_outliers", 1): at the end of cugo_graph_optimize every edge of the set whose chi2 term exceeds a finite
 * threshold > 0 becomes inactive (left out by the next initialize; cugo_graph_n_pose_edge_outliers,
 * cugo_graph_get_pose_edge_active); any other value disables.  Without the option a positive value makes
 * cugo_graph_initialize() refuse the graph */
int cugo_graph_set_icp_outlier_threshold(cugo_graph* g, int kind, double threshold);
/* active edges of the kind in the current flattening (edges on fixed poses are not counted); -1: unknown kind */
int cugo_graph_n_icp_edges(cugo_graph* g, int kind);
/* Extension: SE(3) pose priors (PosePriorEdgeSet, cuda-bundle-adjustment_amd/include/prior_types.h), next to or instead
 * of the other sets; term and conventions as for cugo_prior_edges above.  q_t7 [n][7]: the measured pose Z (q x y z w,
 * then t); info36 [n][36]: Omega of every edge (symmetric, so row- and column-major agree), or NULL for the set's
 * matrix (cugo_graph_set_prior_information; the identity until it is set).  As for the other sets, the per-edge values
 * count when the graph was created with per_edge_information, the set's otherwise.  cugo_graph_initialize() refuses
 * non-finite values, |q_z| off 1 by more than 1e-6, an Omega that is asymmetric beyond 1e-12 max|Omega| or has an
 * eigenvalue below -1e-12 lambda_max (semi-definite is allowed: a translation-only prior), a pose of no pose set of
 * the optimiser, an outlier threshold on the set unless the option "pose_edge_outliers" is on and a sharded optimiser;
 * edges on fixed poses count for nothing. */
int cugo_graph_add_pose_priors(cugo_graph* g, int n, const int32_t* pose_ids, const double* q_t7, const double* info36);
int cugo_graph_set_prior_information(cugo_graph* g, const double* info36);
int cugo_graph_set_prior_robust_kernel(cugo_graph* g, int type, double delta);
/* as cugo_graph_set_icp_outlier_threshold (refused by cugo_graph_initialize() unless "pose_edge_outliers" is on) */
int cugo_graph_set_prior_outlier_threshold(cugo_graph* g, double threshold);
/* active priors in the current flattening (priors on fixed poses are not counted) */
int cugo_graph_n_prior_edges(cugo_graph* g);
/* Extension: landmark position priors (LandmarkPriorEdgeSet, cuda-bundle-adjustment_amd/include/landmark_prior_types.h),
 * next to the other sets; term and conventions as for cugo_lm_prior_edges above.  lm_ids [n]: ids given to
 * cugo_graph_add_landmarks (an unknown id refuses the whole call: nothing is added); xyz3 [n][3]: the measured position
 * Z; info9 [n][9]: Omega of every prior (symmetric, so row- and column-major agree), or NULL for the set's matrix
 * (cugo_graph_set_landmark_prior_information; the identity until it is set), with the per_edge_information rule of the
 * pose priors.  Several priors on one landmark are allowed.  cugo_graph_initialize() refuses non-finite values, an Omega
 * that is asymmetric beyond 1e-12 max|Omega| or has an eigenvalue below -1e-12 lambda_max (semi-definite is allowed: a
 * height-only prior), a landmark of no landmark set of the optimiser, a prior that counts on a free landmark without any
 * BA edge (the back-substitution gives such a landmark a zero step), an outlier threshold on the set and a sharded
 * optimiser; priors on fixed landmarks and inactive priors count for nothing. */
int cugo_graph_add_landmark_priors(cugo_graph* g, int n, const int32_t* lm_ids, const double* xyz3, const double* info9);
int cugo_graph_set_landmark_prior_information(cugo_graph* g, const double* info9);
int cugo_graph_set_landmark_prior_robust_kernel(cugo_graph* g, int type, double delta);
/* active landmark priors in the current flattening (priors on fixed landmarks are not counted) */
int cugo_graph_n_landmark_prior_edges(cugo_graph* g);
/* Extension: point-to-point pose edges (PointEdgeSet, cuda-bundle-adjustment_amd/include/point_edge_types.h), next to the
 * other sets or alone; term and conventions as for cugo_point_edges above.  pose_ids [n]: ids given to
 * cugo_graph_add_poses (an unknown id refuses the whole call: nothing is added); pointP [n][3]: the known points;
 * pointZ [n][3]: their measurements in the pose's frame; info9 [n][9]: Omega of every edge (symmetric, so row- and
 * column-major agree), or NULL for a COPY of the set's matrix as it is at the time of the add
 * (cugo_graph_set_point_information; the identity until it is set: a later change of the set's matrix does not reach an
 * edge already added), with the per_edge_information rule of the pose priors (off: the set's matrix counts for all).  cugo_graph_initialize() refuses non-finite values, an Omega that is
 * asymmetric beyond 1e-12 max|Omega| or has an eigenvalue below -1e-12 lambda_max (semi-definite is allowed), a pose of no
 * pose set of the optimiser, an outlier threshold on the set and a sharded optimiser; edges on fixed poses and inactive
 * edges count for nothing.  The set is no kind of cugo_graph_n_pose_edge_outliers (CUGO_POSE_KIND_*). */
int cugo_graph_add_point_edges(cugo_graph* g, int n, const int32_t* pose_ids, const double* pointP, const double* pointZ,
                               const double* info9);
int cugo_graph_set_point_information(cugo_graph* g, const double* info9);
int cugo_graph_set_point_robust_kernel(cugo_graph* g, int type, double delta);
/* point edges that count in the current flattening (edges on fixed poses are not counted) */
int cugo_graph_n_point_edges(cugo_graph* g);
/* Diagnostic: the point edges of the current flattening as the kernels read them (works on a plan-only graph): sorted
 * by pose (stable: insertion order inside a pose), planar.  Returns their number n (or a negative error) and *n_info (n,
 * or 1 when one matrix serves all); with cap >= n fills the arrays that are not NULL: pose [n] (flattened index), src_edge
 * [n] (position among the edges added), p [3][n], z [3][n], info [6][n_info] (upper triangle of the symmetric part of
 * Omega, row-major packed 00 01 02 11 12 22). */
int cugo_graph_get_flat_point_edges(cugo_graph* g, int cap, int32_t* pose, int32_t* src_edge, double* p, double* z,
                                    double* info, int* n_info);
/* Extension: pose-pose point edges (PointPairEdgeSet, cuda-bundle-adjustment_amd/include/point_pair_types.h) for
 * scan-to-scan registration, next to the other sets or alone; term and conventions as for cugo_point_pair_edges above.
 * pose_ids_a / pose_ids_b [n]: ids given to cugo_graph_add_poses (an unknown id, or a == b, refuses the whole call: nothing
 * is added); pointP [n][3]: the points in a's frame; pointZ [n][3]: the same points measured in b's frame; info9 [n][9]:
 * Omega of every edge in b's frame, or NULL for a COPY of the set's matrix at the time of the add
 * (cugo_graph_set_point_pair_information; the identity until it is set), with the per_edge_information rule of the point
 * edges.  cugo_graph_initialize() checks the values as for the point edges and refuses, naming the set: an outlier
 * threshold > 0 on the set (cugo_graph_set_point_pair_outlier_threshold exists so that the set has every setter; not yet
 * supported), a sharded optimiser and CUGO_HSC_STRIP=1.  Edges between two fixed poses and inactive edges count for
 * nothing; an edge with one fixed end counts.  Every pair of free poses a counting edge joins is a block of the Schur
 * complement's pattern.  The set is no kind of cugo_graph_n_pose_edge_outliers (CUGO_POSE_KIND_*). */
int cugo_graph_add_point_pair_edges(cugo_graph* g, int n, const int32_t* pose_ids_a, const int32_t* pose_ids_b,
                                    const double* pointP, const double* pointZ, const double* info9);
int cugo_graph_set_point_pair_information(cugo_graph* g, const double* info9);
int cugo_graph_set_point_pair_robust_kernel(cugo_graph* g, int type, double delta);
int cugo_graph_set_point_pair_outlier_threshold(cugo_graph* g, double threshold);
/* active flag of n edges from `first` on, in insertion order (active[i] != 0: active); counts as a change of the set */
int cugo_graph_set_point_pair_active(cugo_graph* g, int first, int n, const uint8_t* active);
/* pair edges that count in the current flattening: active, at least one free end */
int cugo_graph_n_point_pair_edges(cugo_graph* g);
/* Diagnostic: the pair edges of the current flattening as the kernels read them (works on a plan-only graph): in the
 * order of their plan — runs of one (a, b) orientation of a pair, ordered by (lo, hi, orientation), insertion order inside
 * a run —, planar.  Returns their number n (or a negative error) and *n_info (n, or 1 when one matrix serves all); with
 * cap >= n fills the arrays that are not NULL: pose_a, pose_b [n] (flattened indices), src_edge [n] (position among the
 * edges added), p [3][n], z [3][n], info [6][n_info] (upper triangle of the symmetric part of Omega, row-major packed). */
/* Extension: the covariance form of the two point kinds (GicpEdgeSet / GicpPairEdgeSet,
 * cuda-bundle-adjustment_amd/include/gicp_types.h; term: cugo_gicp_edges above): generalised ICP in ONE optimize(), Omega =
 * (C_z + M C_p M^T)^-1 rebuilt at every linearisation and evaluated at the trial poses of every trial.  covP9 / covZ9: [n][9]
 * (symmetric).  An unknown id, or a == b, refuses the whole call.  cugo_graph_initialize refuses, naming the set: a
 * covariance that is not finite, symmetric (1e-12 max|C|) and positive semi-definite (-1e-12 lambda_max), lambda_min(C_p) +
 * lambda_min(C_z) <= 1e-12 (lambda_max(C_p) + lambda_max(C_z)); these edges next to information-form point edges of the
 * same arity; a positive outlier threshold; a sharded optimiser; CUGO_HSC_STRIP=1 with pair edges.  The flat getters work
 * on a plan-only graph: cov_p, cov_z [6][n_cov] packed upper triangles, *n_cov = n or 1; they return n (copying only
 * when cap >= n). */
int cugo_graph_add_gicp_edges(cugo_graph* g, int n, const int32_t* pose_ids, const double* pointP, const double* pointZ,
                              const double* covP9, const double* covZ9);
int cugo_graph_add_gicp_pair_edges(cugo_graph* g, int n, const int32_t* pose_ids_a, const int32_t* pose_ids_b, const double* pointP,
                                   const double* pointZ, const double* covP9, const double* covZ9);
int cugo_graph_set_gicp_robust_kernel(cugo_graph* g, int type, double delta);
int cugo_graph_set_gicp_pair_robust_kernel(cugo_graph* g, int type, double delta);
int cugo_graph_set_gicp_outlier_threshold(cugo_graph* g, double threshold);
int cugo_graph_set_gicp_pair_outlier_threshold(cugo_graph* g, double threshold);
int cugo_graph_set_gicp_pair_active(cugo_graph* g, int first, int n, const uint8_t* active);
int cugo_graph_n_gicp_edges(cugo_graph* g);
int cugo_graph_n_gicp_pair_edges(cugo_graph* g);
int cugo_graph_get_flat_gicp_edges(cugo_graph* g, int cap, int32_t* pose, int32_t* src_edge, double* p, double* z, double* cov_p,
                                   double* cov_z, int* n_cov);
int cugo_graph_get_flat_gicp_pair_edges(cugo_graph* g, int cap, int32_t* pose_a, int32_t* pose_b, int32_t* src_edge, double* p,
                                        double* z, double* cov_p, double* cov_z, int* n_cov);
int cugo_graph_get_flat_point_pair_edges(cugo_graph* g, int cap, int32_t* pose_a, int32_t* pose_b, int32_t* src_edge, double* p,
                                         double* z, double* info, int* n_info);
/* Extension: relative-pose SE(3) edges (RelPoseEdgeSet, cuda-bundle-adjustment_amd/include/relpose_types.h), next to or
 * instead of the other sets; term and conventions as for cugo_relpose_edges above (Z ~ T_a T_b^-1).  pose_ids_a /
 * pose_ids_b [n]: ids given to cugo_graph_add_poses; q_t7 [n][7] the measured relative pose; info36 [n][36] or NULL for
 * the set's matrix (cugo_graph_set_relpose_information; the identity until it is set), with the per_edge_information
 * rule of the priors.  The graph object switches GraphOptimisationOptions::relativePoseEdges on itself.
 * cugo_graph_initialize() refuses a == b, a pose of no pose set of the optimiser, non-finite values, |q_z| off 1 by more
 * than 1e-6, an Omega that is asymmetric or indefinite (the bounds of the priors), an outlier threshold on the set unless
 * the option "pose_edge_outliers" is on and a sharded optimiser; inactive edges and edges between two fixed poses count for nothing, an edge with one fixed end
 * counts in chi2 and adds its free end's terms.  The pose pairs join the Hsc pattern. */
int cugo_graph_add_relpose_edges(cugo_graph* g, int n, const int32_t* pose_ids_a, const int32_t* pose_ids_b,
                                 const double* q_t7, const double* info36);
int cugo_graph_set_relpose_information(cugo_graph* g, const double* info36);
int cugo_graph_set_relpose_robust_kernel(cugo_graph* g, int type, double delta);
/* as cugo_graph_set_icp_outlier_threshold (refused by cugo_graph_initialize() unless "pose_edge_outliers" is on): the
 * gate for false loop closures.  A pair whose last edge goes keeps its (then empty) block of Hsc until the next
 * cugo_graph_initialize() */
int cugo_graph_set_relpose_outlier_threshold(cugo_graph* g, double threshold);
/* active flag of the edges [first, first + n) of the set, in insertion order (an inactive edge is left out by the next
 * cugo_graph_initialize(); a pair no active edge joins any more leaves the Hsc pattern) */
int cugo_graph_set_relpose_active(cugo_graph* g, int first, int n, const uint8_t* active);
/* relative-pose edges that count in the current flattening */
int cugo_graph_n_relpose_edges(cugo_graph* g);
/* multi-GPU: this process handles shard `rank` of `world` (landmark ranges).  exchange() is
 * called on the host with a DEVICE buffer that must be all-reduced in place over all ranks
 * (op 0 = sum, 1 = max) before it returns, or — op >= 2 — overwritten on every rank with rank
 * (op - 2)'s content (a broadcast: the update blocks and solution ranges of the elimination subtrees a
 * rank owns in the sparse LL^T; CUGO_OWN_SUBTREES=0 keeps the factorisation replicated and never asks). */
/* op == -1: a sum REDUCE-SCATTER of `world` equal segments (n_doubles / world doubles each): on return segment `rank`
 * of the buffer must hold the sum over ranks of that segment (the other segments are not read afterwards) — the
 * ownership-keyed exchange of the Schur system: a rank only needs the Hsc blocks its own fronts assemble. */
typedef void (*cugo_exchange_fn)(void* d_buf, size_t n_doubles, int op, void* user);
/* ref: EdgeSet::setOutlierThreshold (src/optimisable_graph.h:737-740) + updateEdges
 * (optimisable_graph.hpp:603-640): at the end of cugo_graph_optimize every edge of the set (dim 2
 * = mono, 3 = stereo) whose chi2 in the last error pass exceeds `threshold` becomes inactive
 * (left out by the next initialize / optimize).  0 disables (default). */
int cugo_graph_set_outlier_threshold(cugo_graph* g, int dim, double threshold);
/* outliers found since the last initialize (ref: getOutlierCount) */
int cugo_graph_n_outliers(cugo_graph* g, int dim);
/* active flag of the first n edges of the set, in insertion order */
int cugo_graph_get_edge_active(cugo_graph* g, int dim, int n, uint8_t* active);
/* Extension: depth edges (DepthEdgeSet, ref: include/ba_types.h:171-260): observations (u, v, 1/Z) with the residual
 * (pu - u, pv - v, sqrt(k) (1/Z - m_d)); k is the set's inverse-depth weight (default 1, the reference's chi2).  They
 * share the landmark-major array, the Schur complement and the covariance entry points with the mono and stereo edges;
 * the dim-keyed functions above keep meaning mono (2) and stereo (3), these are their counterparts for the depth set.
 * meas3 [n][3]; info [n] (with per-edge information) or NULL; cam5 [n][5] or NULL for the set's camera (bf unused).
 * cugo_graph_initialize refuses a weight that is not finite and > 0, and a depth set on a landmark-sharded (multi-GPU)
 * graph.  cugo_graph_reprojection_covariances keeps its two kinds (2, 3); cugo_graph_predict_observations has the
 * depth kind (CUGO_OBS_DEPTH). */
int cugo_graph_add_depth_edges(cugo_graph* g, int n, const int32_t* pose_ids, const int32_t* landmark_ids,
                               const double* meas3, const double* info, const double* cam5);
int cugo_graph_set_depth_camera(cugo_graph* g, const double* cam5);
int cugo_graph_set_depth_information(cugo_graph* g, double info);
int cugo_graph_set_depth_robust_kernel(cugo_graph* g, int type, double delta);
int cugo_graph_set_depth_outlier_threshold(cugo_graph* g, double threshold);
int cugo_graph_set_depth_weight(cugo_graph* g, double weight);
int cugo_graph_n_depth_outliers(cugo_graph* g);
int cugo_graph_get_depth_edge_active(cugo_graph* g, int n, uint8_t* active);
/* Diagnostic: the pose-landmark edges of the current flattening in flattening order (set by set, insertion order; mono,
 * stereo and depth edges share the array).  Returns their number (or a negative error) and fills the first `cap`
 * entries of the arrays that are not NULL: flattened pose and landmark index, CUGO_EDGE_* flags, meas3 [cap][3] (the
 * third 0 for a mono edge); *has_depth / *depth_weight: what the edge kernels get in cugo_edges. */
int cugo_graph_get_flat_edges(cugo_graph* g, int cap, int32_t* pose, int32_t* landmark, uint8_t* flags, double* meas3,
                              int* has_depth, double* depth_weight);
/* The same for the four pose edge kinds: CUGO_ICP_PLANE / CUGO_ICP_LINE under their other names, the priors and the
 * relative-pose edges.  Outliers found in the kind's set since the last initialize (a negative error code for an
 * unknown kind), and the active flag of its first n edges in insertion order (CUGO_ERR_INVALID: unknown kind, n
 * beyond the edges added). */
#define CUGO_POSE_KIND_PLANE 0
#define CUGO_POSE_KIND_LINE 1
#define CUGO_POSE_KIND_PRIOR 2
#define CUGO_POSE_KIND_RELPOSE 3
int cugo_graph_n_pose_edge_outliers(cugo_graph* g, int kind);
int cugo_graph_get_pose_edge_active(cugo_graph* g, int kind, int n, uint8_t* active);
int cugo_graph_set_shard(cugo_graph* g, int rank, int world, cugo_exchange_fn fn, void* user);
/* Native exchange (one process per GPU, RCCL over xGMI; not in the reference, which is single-GPU:
 * src/cuda_device.cpp:264-282).  Rank 0 of the job calls cugo_comm_unique_id() (ncclGetUniqueId,
 * CUGO_UNIQUE_ID_BYTES bytes) and hands the id to every rank by any channel; every rank then calls
 * cugo_comm_create() (a collective: ncclCommInitRank on the current device) once per process and
 * attaches the communicator to its optimisers with cugo_graph_set_comm().  From then on the
 * per-trial sum of [Hsc | bsc] and of (F-hat, scale) are ncclAllReduce calls queued on the
 * solver's own stream: no host synchronisation and no callback.  librccl is loaded on first use.
 * The communicator must outlive the last optimize() of the graphs that use it. */
#define CUGO_UNIQUE_ID_BYTES 128
typedef struct cugo_comm cugo_comm;
int cugo_comm_unique_id(void* id128);
int cugo_comm_create(const void* id128, int rank, int world, cugo_comm** out);
void cugo_comm_destroy(cugo_comm* comm);
int cugo_graph_set_comm(cugo_graph* g, cugo_comm* comm);
/* payload bytes and number of all-reduce calls since the last cugo_graph_initialize() */
int cugo_graph_exchange_stats(cugo_graph* g, double* bytes, int32_t* calls);
/* hipSetDevice for the calling thread: a rank binds its GPU (LOCAL_RANK) before creating graphs */
int cugo_set_device(int device);
/* the landmark index range [*l0, *l1) that shard `rank` of `world` owns, given the number
 * of active edges of every landmark (host only; the rule cugo_graph_initialize applies) */
int cugo_shard_range(int n_landmarks_total, const int32_t* edges_per_landmark, int rank, int world,
                     int* l0, int* l1);
/* ref: initialize() :147.  When nothing but vertex estimates changed since the last call (no vertex /
 * edge added or removed, no fixed flag, measurement, information, camera, robust kernel or threshold
 * touched) the flattened graph on the device is kept and only the estimates are uploaded; the
 * counter below says how often that happened (CUGO_NO_FLATTEN_REUSE=1 disables it). */
int cugo_graph_initialize(cugo_graph* g);
int cugo_graph_flatten_reuses(cugo_graph* g);
/* Run-time switches of one optimiser.  Every optimiser takes a snapshot of the CUGO_* environment variables when it
 * is created (README.md lists them; nothing is read per call); this changes a single switch afterwards:
 *   "flatten_reuse"   (0 = CUGO_NO_FLATTEN_REUSE: flatten and upload the whole graph in every initialize)
 *   "structure_reuse" (0 = CUGO_NO_STRUCTURE_REUSE: Hsc pattern, lists, ordering, symbolic factor rebuilt every time —
 *                      what a caller that builds a new graph per call, e.g. ORB-SLAM2, pays)
 *   "init_timing"     (1 = CUGO_INIT_TIMING: per-section host times of initialize / optimize on stderr)
 * and one option of the graph itself, off by default, which takes effect at the next cugo_graph_initialize() (a kept
 * flattening is not reused across a change of it):
 *   "pose_edge_outliers" (1 = GraphOptimisationOptions::poseEdgeOutlierRejection: outlier thresholds on the plane, line,
 *                      prior and relative-pose sets are taken instead of refused)
 * Returns CUGO_ERR_INVALID for an unknown name. */
int cugo_graph_set_option(cugo_graph* g, const char* name, int value);
int cugo_graph_optimize(cugo_graph* g, int n_iters);  /* ref: optimize(n)  :153 */
int cugo_graph_n_stats(cugo_graph* g);                /* ref: batchStatistics() :158 */
int cugo_graph_get_stats(cugo_graph* g, int32_t* iteration, double* chi2, int cap);
int cugo_graph_get_trace(cugo_graph* g, double* lambda, double* rho, int32_t* trials, int cap);
int cugo_graph_get_poses(cugo_graph* g, int n, const int32_t* ids, double* q_t7);
int cugo_graph_get_landmarks(cugo_graph* g, int n, const int32_t* ids, double* xyz);
/* overwrite estimates of existing vertices (ref: Vertex::setEstimate,
 * src/optimisable_graph.h:128); takes effect at the next cugo_graph_initialize() */
int cugo_graph_set_poses(cugo_graph* g, int n, const int32_t* ids, const double* q_t7);
int cugo_graph_set_landmarks(cugo_graph* g, int n, const int32_t* ids, const double* xyz);
int cugo_graph_n_active_edges(cugo_graph* g);
/* Extension: marginal covariances (g2o SparseOptimizer::computeMarginals, Ceres Covariance).
 * what: 1 poses, 2 landmarks, 3 both.  Builds J^T Omega J at lambda = 0 at the current estimates (robust
 * weights included, the edges of the current flattening), forms the Schur complement, factors it and runs
 * the selected inverse (cugo_chol_selected_inverse); the landmark blocks follow from the pose blocks.  The
 * results are kept until the next initialize(); the estimates and the LM state are left as they were.
 * CUGO_ERR_NUMERIC on a zero pivot (e.g. an unconstrained gauge or an edgeless free pose).  A free landmark without
 * an active edge — it never had one, or outlier rejection took them all — has Hll = 0 at lambda = 0: what = 2 and
 * what = 3 then fail as a whole with CUGO_ERR_NUMERIC and keep nothing, what = 1 succeeds (the poses do not depend on
 * it); fix such a landmark or remove it to get the others.
 * CUGO_ERR_INVALID before initialize(), on plan-only, sharded or fp32-internal graphs. */
int cugo_graph_compute_covariances(cugo_graph* g, int what);
/* diagonal blocks by caller id: cov36 [n][36] (6x6, column-major, tangent order [rotation, translation]
 * of the left update T <- exp([w, v]) T), cov9 [n][9] (3x3, column-major); zeros for fixed vertices.
 * CUGO_ERR_INVALID if that kind was not computed since the last initialize(). */
int cugo_graph_get_pose_covariances(cugo_graph* g, int n, const int32_t* ids, double* cov36);
int cugo_graph_get_landmark_covariances(cugo_graph* g, int n, const int32_t* ids, double* cov9);
/* Extension: the cross-covariance blocks Sigma_ab of the pose pairs (ids_a[k], ids_b[k]) — any pairs, in the Hsc
 * pattern or not — at the current estimates: cov36 [n][36] (host), layout and tangent order as above, rows a and
 * columns b; a == b gives the diagonal block, a fixed pose in the pair gives zeros.  Runs the build pass at
 * lambda = 0, the Schur complement and one factorisation as cugo_graph_compute_covariances does, then
 * cugo_chol_inverse_blocks.  Same error codes; also CUGO_ERR_INVALID for an id that is not a pose of the current
 * flattening.  Leaves the estimates, the LM state and the marginals kept by cugo_graph_compute_covariances alone. */
int cugo_graph_compute_pose_cross_covariances(cugo_graph* g, int n, const int32_t* ids_a, const int32_t* ids_b,
                                              double* cov36);
/* covariance of the relative pose A = T_a T_b^-1 in the tangent convention of relpose_types.h (J_a = I,
 * J_b = -Ad(A) at Z = A):  Sigma_aa - Sigma_ab Ad(A)^T - Ad(A) Sigma_ba + Ad(A) Sigma_bb Ad(A)^T, on the host from the
 * blocks above and the current estimates.  A positive definite result inverts to the information of a relative-pose
 * edge that summarises the graph between a and b.  CUGO_ERR_INVALID for a == b. */
int cugo_graph_relative_pose_covariances(cugo_graph* g, int n, const int32_t* ids_a, const int32_t* ids_b,
                                         double* cov36);
/* Extension: the pose-landmark blocks Sigma_al of the pairs (pose_ids[k], lm_ids[k]) — any pairs, with or without an
 * edge — at the current estimates: cov18 [n][18] (host), 6x3 column-major, rows in the tangent order above; zeros where
 * the pose or the landmark is fixed.  One build pass at lambda = 0, Schur complement and factorisation as above, then
 * cugo_chol_inverse_blocks for the pose pairs the queries need and cugo_pose_landmark_cross_covariances; only the
 * results travel to the host.  CUGO_ERR_NUMERIC on a zero pivot or when the Hll of a QUERIED landmark is not positive
 * definite (a free landmark without an active edge); other landmarks in that state do not matter.  CUGO_ERR_INVALID for
 * an id that is not a vertex of the current flattening, before initialize(), on plan-only, sharded or fp32-internal
 * graphs.  Leaves the estimates, the LM state and the kept marginals alone. */
int cugo_graph_compute_pose_landmark_cross_covariances(cugo_graph* g, int n, const int32_t* pose_ids,
                                                       const int32_t* lm_ids, double* cov18);
/* the covariance S = J Sigma J^T of the predicted reprojection of landmark lm_ids[k] in pose pose_ids[k] over the joint
 * [pose; landmark] block (the search ellipse of guided matching, the denominator of a normalised-innovation test):
 * cov [n][dim*dim] (host), column-major, dim = 2 (mono: u, v) or 3 (stereo: u, v, u_right).  cam5 [n][5] = fx, fy, cx,
 * cy, bf per query, or NULL for the camera set with cugo_graph_set_camera(g, dim, ...).  A fixed pose contributes no
 * pose terms, a fixed landmark no landmark terms; both fixed gives zeros.  Error codes as above; also CUGO_ERR_INVALID
 * for dim outside {2, 3}. */
int cugo_graph_reprojection_covariances(cugo_graph* g, int n, const int32_t* pose_ids, const int32_t* lm_ids, int dim,
                                        const double* cam5, double* cov);
/* the predicted observation z of landmark lm_ids[k] seen from pose pose_ids[k] and its covariance S = J Sigma J^T over
 * the joint [pose; landmark] block, for every camera kind (cugo_predict_observations above: kinds, geometry, the depth
 * row in measurement units).  kind: CUGO_OBS_MONO / _STEREO / _DEPTH, dim = 2 / 3 / 3; z [n][dim], cov [n][dim*dim]
 * column-major (host).  cam5 [n][5] per query, with sensor_q_t7 [n][7] = (qx, qy, qz, qw, tx, ty, tz) body -> sensor
 * (NULL: the identity; the quaternion is normalised in fp64) and model_k5 [n][5] = (k1, k2, k3, k4, model) (NULL: a
 * pinhole).  cam5 == NULL takes the camera, sensor pose and model of the graph's mono / stereo / depth set for kind
 * 2 / 3 / 4; the other two must then be NULL too.  Fixed vertices as for cugo_graph_reprojection_covariances; z is
 * computed for them too.  Error codes as above (CUGO_ERR_NUMERIC: both outputs zero-filled); also CUGO_ERR_INVALID for
 * a kind outside {2, 3, 4}, a quaternion that is not finite or has norm 0, coefficients that are not finite, an
 * unknown model and a Kannala-Brandt model with kind 3 or 4. */
int cugo_graph_predict_observations(cugo_graph* g, int n, const int32_t* pose_ids, const int32_t* lm_ids, int kind,
                                    const double* cam5, const double* sensor_q_t7, const double* model_k5, double* z,
                                    double* cov);
/* per-phase milliseconds accumulated since initialize(): ref getTimeProfile
 * (block_solver.cpp:470-488).  names is a '\n' separated list written into buf. */
int cugo_graph_time_profile(cugo_graph* g, char* names_buf, int buf_len, double* ms, int cap);
int cugo_graph_set_verbose(cugo_graph* g, int verbose);
/* HIP-event timing on the solver's own stream (diagnostic).  on = 1: an event pair round every kernel group (build,
 * errors, schur, cholesky, backsubst_update, exchange) and every kernel — per-kernel figures; a pair brackets the kernel
 * and its dispatch, 1 - 2 us more than the kernel's own duration, so these are never to be summed; on = 2: ONE event per group boundary, so that the group times add up exactly to the device time
 * between the first and the last event of cugo_graph_optimize; 0: off.  names: '\n' separated. */
int cugo_graph_set_kernel_timing(cugo_graph* g, int on);
/* fp32-internal mode (ref: the USE_FLOAT32 build option, CMakeLists.txt:8; here a run-time switch,
 * GraphOptimisationOptions::useFloat32): float storage of the Hpl / Hpl*Hll^-1 block streams,
 * everything else fp64.  Takes effect at the next cugo_graph_initialize(). */
int cugo_graph_set_float32(cugo_graph* g, int on);
int cugo_graph_kernel_times(cugo_graph* g, char* names_buf, int buf_len, double* ms,
                            int32_t* launches, int cap);
/* device-to-device copy on the context stream (used by exchange callbacks) */
int cugo_memcpy_d2d(cugo_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);
/* solver statistics of the last buildStructure, in this order: B (Hsc blocks), M (block
 * products), nnz(L), Cholesky flops, supernodes, stages, front bytes, off-diagonal products,
 * then the algorithmic work of the batched Cholesky kernels per factorisation: potrf flops,
 * trsm flops, syrk flops, extend-add bytes, backward bytes.  Returns the count written. */
int cugo_graph_structure_stats(cugo_graph* g, double* out, int cap);

/* seeded ORB-SLAM-style synthetic graph built directly into a graph.
 * Returns arrays through the getters above; also usable to feed the CPU oracle. */
typedef struct cugo_synth_params
{
    int n_poses, n_landmarks, n_edges; /* exact counts */
    double stereo_fraction;            /* fraction of landmarks observed in stereo */
    double pixel_noise, pose_rot_noise, pose_trans_noise, landmark_noise_rel;
    int n_loop_closures;
    uint64_t seed;
} cugo_synth_params;
/* fills caller-provided arrays (sizes from params): poses [P][7], lms [L][3],
 * e_pose/e_lm [E], e_stereo [E], e_meas [E][3], e_omega [E]; cam5 [5].  ids == positions;
 * pose 0 is the gauge (fixed). */
int cugo_synth_generate(const cugo_synth_params* p, double* poses, double* lms, int32_t* e_pose,
                        int32_t* e_lm, uint8_t* e_stereo, double* e_meas, double* e_omega,
                        double* cam5);

#ifdef __cplusplus
}
#endif
#endif /* CUGO_HIP_H */
