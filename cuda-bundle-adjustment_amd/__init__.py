"""ctypes binding of libcugo_hip.so — the MI355X bundle-adjustment hot path.

The directory name contains a hyphen, so import it with
    importlib.import_module("cuda-bundle-adjustment_amd")
(tests/conftest.py and bench.py do).  This module is plumbing only: all compute lives in the
HIP library; if the library is missing every entry point raises (no CPU fallback).
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CUGO_LIB selects another build of the same library (tools/run_san.sh: the sanitizer build; the diagnosis tools:
# the hooks build)
LIB_PATH = os.environ.get("CUGO_LIB") or os.path.join(_HERE, "libcugo_hip.so")
HOOKS_LIB_PATH = os.path.join(_HERE, "libcugo_hip_hooks.so")  # make HOOKS=1: delay patterns, checksums, fault injection
_lib = None

OK = 0
RK_NONE, RK_CAUCHY, RK_TUKEY, RK_HUBER = 0, 1, 2, 3
ICP_PLANE, ICP_LINE = 0, 1
# the four pose edge kinds of Graph.n_pose_edge_outliers / pose_edge_active (the first two are ICP_PLANE / ICP_LINE)
POSE_KIND_PLANE, POSE_KIND_LINE, POSE_KIND_PRIOR, POSE_KIND_RELPOSE = 0, 1, 2, 3
# pose_edges_reject: edges one trip of its grid covers (1024 workgroups of 256); beyond, a workgroup walks several runs
POSE_REJECT_GRID_EDGES = 1024 * 256
EDGE_FIXED_L, EDGE_FIXED_P, EDGE_STEREO, EDGE_INACTIVE, EDGE_DEPTH = 1, 2, 4, 8, 16

_i32p = C.POINTER(C.c_int32)
_f64p = C.POINTER(C.c_double)
_u8p = C.POINTER(C.c_uint8)
_u16p = C.POINTER(C.c_uint16)

EXCHANGE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)


class CugoError(RuntimeError):
    pass


class Edges(C.Structure):
    """The HEAD of cugo_edges: every member up to depth_weight.  The C struct has since grown (RigEdges, below) and
    the library reads has_rig behind depth_weight of every edge view it is given, so sizeof(Edges) != sizeof(cugo_edges).
    Edges() — the constructor — is safe: it hands out the head of a zeroed full-size struct (has_rig = 0).  An Edges
    made any other way (from_buffer_copy, copy.copy, (Edges * n)(), a member of another Structure) has nothing behind
    it and must NOT be passed to the library: build a RigEdges for those, which is the struct in full."""
    _fields_ = [("n_edges", C.c_int), ("n_poses_total", C.c_int), ("n_landmarks_total", C.c_int),
                ("n_poses_free", C.c_int), ("n_landmarks_free", C.c_int),
                ("d_pose", C.c_void_p), ("d_lm", C.c_void_p), ("d_meas", C.c_void_p),
                ("d_omega", C.c_void_p), ("n_omega", C.c_int), ("d_flags", C.c_void_p),
                ("d_cam", C.c_void_p), ("d_cams", C.c_void_p), ("n_cams", C.c_int),
                ("d_lm_ptr", C.c_void_p), ("d_pose_ptr", C.c_void_p), ("d_pose_edge", C.c_void_p),
                ("block_f32", C.c_int),
                # depth slots (EDGE_DEPTH): nothing behind has_depth is read while it is 0
                ("has_depth", C.c_int), ("rk_type_depth", C.c_int), ("rk_delta_depth", C.c_double),
                ("depth_weight", C.c_double)]

    def __new__(cls, *args, **kwargs):
        # cugo_edges has grown behind depth_weight (RigEdges below) and the library reads has_rig of every edge view it
        # is given: an Edges() is the head of a zeroed full-size struct, so has_rig is 0 for it
        if cls is Edges:
            return cls.from_buffer(RigEdges())
        return super().__new__(cls)


class RigEdges(Edges):
    """cugo_edges in full: Edges plus the members appended for camera extrinsics (a rig).  has_rig != 0: d_cam_ext
    [n_cams][12] = {M row-major, t_s} per camera-table entry, body -> sensor; d_cam_ext is not read while has_rig is 0"""
    _fields_ = [("has_rig", C.c_int), ("d_cam_ext", C.c_void_p)]


RIG_NONE, RIG_EXTRINSICS, RIG_MODELS = 0, 1, 2   # cugo_edges.has_rig (CUGO_RIG_*)
OBS_MONO, OBS_STEREO, OBS_DEPTH = 2, 3, 4        # kind of a predicted observation (CUGO_OBS_*)
CAM_TAB_STRIDE = 17


RIG_DISTORTION = 3                               # cugo_edges.has_rig (CUGO_RIG_DISTORTION)
DIST_TAB_STRIDE = 18


def distortion_table(ext12, dist5, flags=None):
    """the table d_cam_ext points to under has_rig = RIG_DISTORTION: [n][18] = {M row-major (9), t_s (3), k1, k2, p1, p2,
    k3, flag}, from ext12 [n][12] (None: identities) and dist5 [n][5] = (k1, k2, p1, p2, k3) in OpenCV's order.  flags [n]:
    0 undistorted / 1 distorted (None: distorted iff the entry's coefficients are not all zero)"""
    d = np.asarray(dist5, np.float64).reshape(-1, 5)
    n = len(d)
    tab = np.zeros((n, DIST_TAB_STRIDE))
    tab[:, :12] = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0.0]) if ext12 is None else np.asarray(ext12, np.float64).reshape(n, 12)
    tab[:, 12:17] = d
    tab[:, 17] = np.any(d != 0.0, axis=1) if flags is None else np.asarray(flags, np.float64).reshape(n)
    if not np.all((tab[:, 17] == 0.0) | (tab[:, 17] == 1.0)):
        raise CugoError("distortion_table: flag must be 0 (undistorted) or 1 (distorted)")
    return tab


def camera_model_table(ext12=None, model_k5=None, n=None):
    """the table d_cam_ext points to under has_rig = RIG_MODELS: [n][17] = {M row-major (9), t_s (3), k1, k2, k3, k4,
    model}, from ext12 [n][12] (None: identities) and model_k5 [n][5] = (k1, k2, k3, k4, model) (None: pinholes)"""
    if n is None:
        n = len(ext12) if ext12 is not None else len(model_k5)
    tab = np.zeros((n, CAM_TAB_STRIDE))
    tab[:, :12] = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0.0]) if ext12 is None else np.asarray(ext12, np.float64).reshape(n, 12)
    if model_k5 is not None:
        tab[:, 12:] = np.asarray(model_k5, np.float64).reshape(n, 5)
    if not np.all((tab[:, 16] == 0.0) | (tab[:, 16] == 1.0)):
        raise CugoError("camera_model_table: model must be 0 (pinhole) or 1 (Kannala-Brandt)")
    return tab


class Robust(C.Structure):
    _fields_ = [("type", C.c_int), ("delta", C.c_double), ("type_stereo", C.c_int),
                ("delta_stereo", C.c_double)]


class IcpEdges(C.Structure):
    """cugo_icp_edges: point-to-plane / point-to-line pose edges, pose-sorted structure of arrays (cugo_hip.h)."""
    _fields_ = [("n_poses_total", C.c_int), ("n_poses_free", C.c_int),
                ("n_plane", C.c_int), ("d_plane_pose", C.c_void_p), ("d_plane_pose_ptr", C.c_void_p),
                ("d_plane_p", C.c_void_p), ("d_plane_nd", C.c_void_p), ("d_plane_omega", C.c_void_p),
                ("n_plane_omega", C.c_int), ("d_plane_flags", C.c_void_p), ("rk_plane", C.c_int),
                ("delta_plane", C.c_double),
                ("n_line", C.c_int), ("d_line_pose", C.c_void_p), ("d_line_pose_ptr", C.c_void_p),
                ("d_line_p", C.c_void_p), ("d_line_au", C.c_void_p), ("d_line_omega", C.c_void_p),
                ("n_line_omega", C.c_int), ("d_line_flags", C.c_void_p), ("rk_line", C.c_int),
                ("delta_line", C.c_double)]


class PriorEdges(C.Structure):
    """cugo_prior_edges: SE(3) pose priors with 6 x 6 information, pose-sorted structure of arrays (cugo_hip.h)."""
    _fields_ = [("n_poses_total", C.c_int), ("n_poses_free", C.c_int), ("n", C.c_int),
                ("d_pose", C.c_void_p), ("d_pose_ptr", C.c_void_p), ("d_meas", C.c_void_p), ("d_info", C.c_void_p),
                ("n_info", C.c_int), ("d_flags", C.c_void_p), ("rk", C.c_int), ("delta", C.c_double)]


class PointEdges(C.Structure):
    """cugo_point_edges: point-to-point pose edges with 3 x 3 information, pose-sorted structure of arrays (cugo_hip.h):
    d_p, d_z [3][n]; d_info [6][n_info], the upper triangle of Omega packed row-major (00 01 02 11 12 22), n_info = n or 1."""
    _fields_ = [("n_poses_total", C.c_int), ("n_poses_free", C.c_int), ("n", C.c_int),
                ("d_pose", C.c_void_p), ("d_pose_ptr", C.c_void_p), ("d_p", C.c_void_p), ("d_z", C.c_void_p),
                ("d_info", C.c_void_p), ("n_info", C.c_int), ("d_flags", C.c_void_p), ("rk", C.c_int), ("delta", C.c_double)]


class LmPriorEdges(C.Structure):
    """cugo_lm_prior_edges: landmark position priors with 3 x 3 information, landmark-sorted structure of arrays
    (cugo_hip.h)."""
    _fields_ = [("n_landmarks_total", C.c_int), ("n_landmarks_free", C.c_int), ("n", C.c_int),
                ("d_lm", C.c_void_p), ("d_lm_ptr", C.c_void_p), ("d_meas", C.c_void_p), ("d_info", C.c_void_p),
                ("n_info", C.c_int), ("d_flags", C.c_void_p), ("rk", C.c_int), ("delta", C.c_double)]


class RelPoseEdges(C.Structure):
    """cugo_relpose_edges: relative-pose SE(3) edges with 6 x 6 information in the caller's order; the layout (who walks
    which edge, where the off-diagonal block goes) is the plan's (relpose_plan_create; cugo_hip.h)."""
    _fields_ = [("n_poses_total", C.c_int), ("n_poses_free", C.c_int), ("n", C.c_int),
                ("d_meas", C.c_void_p), ("d_info", C.c_void_p), ("n_info", C.c_int), ("d_flags", C.c_void_p),
                ("rk", C.c_int), ("delta", C.c_double), ("plan", C.c_void_p)]


class PointPairEdges(C.Structure):
    """cugo_point_pair_edges: pose-pose point edges with 3 x 3 information in the SORTED order of their plan
    (PointPairPlan; cugo_hip.h): d_pose_a, d_pose_b [n]; d_p, d_z [3][n]; d_info [6][n_info], n_info = n or 1."""
    _fields_ = [("n_poses_total", C.c_int), ("n_poses_free", C.c_int), ("n", C.c_int),
                ("d_pose_a", C.c_void_p), ("d_pose_b", C.c_void_p), ("d_p", C.c_void_p), ("d_z", C.c_void_p),
                ("d_info", C.c_void_p), ("n_info", C.c_int), ("d_flags", C.c_void_p), ("rk", C.c_int), ("delta", C.c_double),
                ("plan", C.c_void_p)]


class GicpEdges(C.Structure):
    """cugo_gicp_edges: the covariance form of PointEdges (generalised ICP, cugo_hip.h): d_cov_p, d_cov_z [6][n_cov], the
    upper triangles of C_p (world frame) and C_z (the pose's frame), n_cov = n or 1; Omega = (C_z + R C_p R^T)^-1 is formed
    at the poses of every pass."""
    _fields_ = [("n_poses_total", C.c_int), ("n_poses_free", C.c_int), ("n", C.c_int),
                ("d_pose", C.c_void_p), ("d_pose_ptr", C.c_void_p), ("d_p", C.c_void_p), ("d_z", C.c_void_p),
                ("d_cov_p", C.c_void_p), ("d_cov_z", C.c_void_p), ("n_cov", C.c_int), ("d_flags", C.c_void_p), ("rk", C.c_int),
                ("delta", C.c_double)]


class GicpPairEdges(C.Structure):
    """cugo_gicp_pair_edges: the covariance form of PointPairEdges in the SORTED order of their plan (PointPairPlan: the
    plan does not depend on the form): d_cov_p (a's frame), d_cov_z (b's frame) [6][n_cov], n_cov = n or 1; Omega =
    (C_z + M C_p M^T)^-1 with M = R_b R_a^T is formed at the poses of every pass."""
    _fields_ = [("n_poses_total", C.c_int), ("n_poses_free", C.c_int), ("n", C.c_int),
                ("d_pose_a", C.c_void_p), ("d_pose_b", C.c_void_p), ("d_p", C.c_void_p), ("d_z", C.c_void_p),
                ("d_cov_p", C.c_void_p), ("d_cov_z", C.c_void_p), ("n_cov", C.c_int), ("d_flags", C.c_void_p), ("rk", C.c_int),
                ("delta", C.c_double), ("plan", C.c_void_p)]


class HscStruct(C.Structure):
    _fields_ = [("n_blocks", C.c_int), ("d_rowptr", C.c_void_p), ("d_colind", C.c_void_p),
                ("d_off_ptr", C.c_void_p), ("d_off_ei", C.c_void_p), ("d_off_ej", C.c_void_p),
                # landmark-major product plan (cugo_hsc_plan_create fills these; NULL = gather kernels)
                ("n_groups", C.c_int), ("n_slots", C.c_int), ("n_rhs", C.c_int),
                ("d_grp_ptr", C.c_void_p), ("d_grp_nwave", C.c_void_p), ("d_slot_rhs", C.c_void_p),
                ("d_slot_ptr", C.c_void_p),
                ("d_prod", C.c_void_p), ("d_red_ptr", C.c_void_p), ("d_red_slot", C.c_void_p),
                ("d_blk_pose", C.c_void_p), ("d_part_H", C.c_void_p), ("d_part_b", C.c_void_p)]


class SynthParams(C.Structure):
    _fields_ = [("n_poses", C.c_int), ("n_landmarks", C.c_int), ("n_edges", C.c_int),
                ("stereo_fraction", C.c_double), ("pixel_noise", C.c_double),
                ("pose_rot_noise", C.c_double), ("pose_trans_noise", C.c_double),
                ("landmark_noise_rel", C.c_double), ("n_loop_closures", C.c_int),
                ("seed", C.c_uint64)]


def build(force=False):
    """compile libcugo_hip.so in-tree with hipcc for gfx950 (no GPU needed to build)"""
    if force or not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-C", _HERE, "-j8", "-s"])
    else:
        subprocess.check_call(["make", "-C", _HERE, "-j8", "-s"])  # make decides what is stale
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CugoError("libcugo_hip.so is not built (run __graft_entry__.build()); "
                            "there is no CPU fallback")
        _lib = C.CDLL(LIB_PATH)
        _lib.cugo_last_error.restype = C.c_char_p
        _lib.cugo_ctx_stream.restype = C.c_void_p
        # (ctx, ev, hs, d_Hll, d_Hpl, d_sigma, d_cov9, d_fail): device pointers as c_void_p, None = NULL
        _lib.cugo_landmark_covariances.argtypes = [C.c_void_p, C.POINTER(Edges), C.POINTER(HscStruct)] + [C.c_void_p] * 5
        _lib.cugo_landmark_covariances.restype = C.c_int
        # (ctx, ev, n, d_q_pose, d_q_lm, d_q_ptr, d_q_slot, d_Hll, d_Hpl, d_blocks, d_cov18, d_fail)
        _lib.cugo_pose_landmark_cross_covariances.argtypes = [C.c_void_p, C.POINTER(Edges), C.c_int] + [C.c_void_p] * 9
        _lib.cugo_pose_landmark_cross_covariances.restype = C.c_int
        # (ctx, n, n_landmarks_free, d_q_pose, d_q_lm, d_q_dim, d_q_aa, d_cam5, d_poses, d_lms, d_blocks, d_cross18,
        #  d_lmcov9, d_cov9)
        _lib.cugo_reprojection_covariances.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 11
        _lib.cugo_reprojection_covariances.restype = C.c_int
        # (ctx, n, n_landmarks_free, d_q_pose, d_q_lm, d_q_kind, d_q_aa, d_cam5, d_cam_tab, d_poses, d_lms, d_blocks,
        #  d_cross18, d_lmcov9, d_z3, d_cov9)
        _lib.cugo_predict_observations.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 13
        _lib.cugo_predict_observations.restype = C.c_int
        _lib.cugo_graph_predict_observations.argtypes = [C.c_void_p, C.c_int, _i32p, _i32p, C.c_int, _f64p, _f64p, _f64p,
                                                         _f64p, _f64p]
        _lib.cugo_graph_predict_observations.restype = C.c_int
        _lib.cugo_plcov_plan_create.argtypes = [C.c_int, C.c_int, _i32p, _i32p, C.c_int, _i32p, _i32p,
                                                C.POINTER(C.c_void_p)]
        _lib.cugo_plcov_plan_create.restype = C.c_int
        _lib.cugo_plcov_plan_array.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(_i32p)]
        _lib.cugo_plcov_plan_array.restype = C.c_int
        _lib.cugo_plcov_plan_destroy.argtypes = [C.c_void_p]
        _lib.cugo_plcov_plan_destroy.restype = None
        _lib.cugo_graph_compute_pose_landmark_cross_covariances.argtypes = [C.c_void_p, C.c_int, _i32p, _i32p, _f64p]
        _lib.cugo_graph_compute_pose_landmark_cross_covariances.restype = C.c_int
        _lib.cugo_graph_reprojection_covariances.argtypes = [C.c_void_p, C.c_int, _i32p, _i32p, C.c_int, _f64p, _f64p]
        _lib.cugo_graph_reprojection_covariances.restype = C.c_int
        # the fused iteration at kernel level (cugo_hip.h); device pointers as c_void_p, None = NULL
        # (ctx, ev, h_lm_ptr, d_poses, d_lms, rk, lambda, form, d_Hpp, d_bp, d_Hll, d_bl, d_Hpl, d_invHll, d_T, d_lmrec, d_chi)
        _lib.cugo_construct_quadratic_form_fused.argtypes = ([C.c_void_p, C.POINTER(Edges), _i32p, C.c_void_p, C.c_void_p,
                                                              Robust, C.c_double, C.c_int] + [C.c_void_p] * 9)
        _lib.cugo_construct_quadratic_form_fused.restype = C.c_int
        # (ctx, ev, hs, lambda, damp_hsc_diag, form, d_poses, d_Hpp, d_bp, d_Hll, d_bl, d_Hpl, d_invHll, d_T, d_lmrec,
        #  d_bp_out, d_bsc, d_Hsc)
        _lib.cugo_compute_schur_fused.argtypes = ([C.c_void_p, C.POINTER(Edges), C.POINTER(HscStruct), C.c_double, C.c_int,
                                                   C.c_int] + [C.c_void_p] * 12)
        _lib.cugo_compute_schur_fused.restype = C.c_int
        # (ctx, ev, lambda, d_lmrec, d_bl, d_bp, d_G, d_xp, d_xl, d_poses_in, d_lms_in, d_poses_out, d_lms_out, d_scale,
        #  from_records)
        _lib.cugo_backsubst_update_fused.argtypes = ([C.c_void_p, C.POINTER(Edges), C.c_double] + [C.c_void_p] * 11 +
                                                     [C.c_int])
        _lib.cugo_backsubst_update_fused.restype = C.c_int
        _lib.cugo_compute_edge_chi.argtypes = [C.c_void_p, C.POINTER(Edges), C.c_void_p, C.c_void_p, Robust, C.c_void_p]
        _lib.cugo_compute_edge_chi.restype = C.c_int
    return _lib


def check(rc):
    if rc != OK:
        raise CugoError("cugo error %d: %s" % (rc, lib().cugo_last_error().decode()))


def icp_construct_quadratic_form_schur(ctx, ev, d_poses, d_rowptr, d_Hsc, d_bp, d_bsc, d_chi=None):
    """cugo_icp_construct_quadratic_form_schur: the ICP terms of `ev` (IcpEdges) ADDED to the Schur destination, as the
    default LM loop adds them.  ctx: a cugo_ctx handle; the d_* are device pointers; d_rowptr (int32): rowptr[p] is the
    block index of pose p's diagonal block in d_Hsc; b goes to d_bp and to d_bsc alike.  Every handle and pointer must be a
    ctypes.c_void_p (what tests/devmem.py's Ctx hands out): a plain Python int would be passed as a C int"""
    check(lib().cugo_icp_construct_quadratic_form_schur(ctx, C.byref(ev), d_poses, d_rowptr, d_Hsc, d_bp, d_bsc, d_chi))


def prior_construct_quadratic_form_schur(ctx, ev, d_poses, d_rowptr, d_Hsc, d_bp, d_bsc, d_chi=None):
    """cugo_prior_construct_quadratic_form_schur: as icp_construct_quadratic_form_schur, for PriorEdges"""
    check(lib().cugo_prior_construct_quadratic_form_schur(ctx, C.byref(ev), d_poses, d_rowptr, d_Hsc, d_bp, d_bsc, d_chi))


def point_compute_errors(ctx, ev, d_poses, d_chi, d_edge_chi=None):
    """cugo_point_compute_errors: the chi2 of the point edges `ev` (PointEdges) to d_chi[0], and the term of every edge
    to d_edge_chi [n] if given.  Handles and pointers as for icp_construct_quadratic_form_schur"""
    check(lib().cugo_point_compute_errors(ctx, C.byref(ev), d_poses, d_chi, d_edge_chi))


def point_construct_quadratic_form(ctx, ev, d_poses, d_Hpp, d_bp, d_chi=None):
    """cugo_point_construct_quadratic_form: the terms ADDED to d_Hpp [n_poses_free][36] and d_bp [n_poses_free][6]"""
    check(lib().cugo_point_construct_quadratic_form(ctx, C.byref(ev), d_poses, d_Hpp, d_bp, d_chi))


def point_construct_quadratic_form_schur(ctx, ev, d_poses, d_rowptr, d_Hsc, d_bp, d_bsc, d_chi=None):
    """cugo_point_construct_quadratic_form_schur: as icp_construct_quadratic_form_schur, for PointEdges"""
    check(lib().cugo_point_construct_quadratic_form_schur(ctx, C.byref(ev), d_poses, d_rowptr, d_Hsc, d_bp, d_bsc, d_chi))


def gicp_compute_errors(ctx, ev, d_poses, d_chi, d_edge_chi=None):
    """cugo_gicp_compute_errors: as point_compute_errors, for GicpEdges (Omega formed at d_poses)"""
    check(lib().cugo_gicp_compute_errors(ctx, C.byref(ev), d_poses, d_chi, d_edge_chi))


def gicp_construct_quadratic_form(ctx, ev, d_poses, d_Hpp, d_bp, d_chi=None):
    """cugo_gicp_construct_quadratic_form: as point_construct_quadratic_form, for GicpEdges"""
    check(lib().cugo_gicp_construct_quadratic_form(ctx, C.byref(ev), d_poses, d_Hpp, d_bp, d_chi))


def gicp_construct_quadratic_form_schur(ctx, ev, d_poses, d_rowptr, d_Hsc, d_bp, d_bsc, d_chi=None):
    """cugo_gicp_construct_quadratic_form_schur: as point_construct_quadratic_form_schur, for GicpEdges"""
    check(lib().cugo_gicp_construct_quadratic_form_schur(ctx, C.byref(ev), d_poses, d_rowptr, d_Hsc, d_bp, d_bsc, d_chi))


def lm_prior_compute_errors(ctx, ev, d_lms, d_chi, d_edge_chi=None):
    """cugo_lm_prior_compute_errors: the chi2 of the landmark priors `ev` (LmPriorEdges) to d_chi[0], and the term of
    every prior to d_edge_chi [n] if given.  Handles and pointers as for icp_construct_quadratic_form_schur"""
    check(lib().cugo_lm_prior_compute_errors(ctx, C.byref(ev), d_lms, d_chi, d_edge_chi))


def lm_prior_construct_quadratic_form(ctx, ev, d_lms, d_Hll, d_bl, d_chi=None):
    """cugo_lm_prior_construct_quadratic_form: the terms ADDED to d_Hll [Lfree][9] and d_bl [Lfree][3]"""
    check(lib().cugo_lm_prior_construct_quadratic_form(ctx, C.byref(ev), d_lms, d_Hll, d_bl, d_chi))


def construct_quadratic_form_lm_priors(ctx, ev, lp, d_poses, d_lms, rk, d_Hpp, d_bp, d_Hll, d_bl, d_Hpl, d_chi=None):
    """cugo_construct_quadratic_form_lm_priors: the BA build pass of `ev` (Edges, rk: Robust) with the landmark priors
    `lp` taken inside its edge kernel, the form the LM loop uses"""
    check(lib().cugo_construct_quadratic_form_lm_priors(ctx, C.byref(ev), C.byref(lp), d_poses, d_lms, rk, d_Hpp, d_bp,
                                                        d_Hll, d_bl, d_Hpl, d_chi))


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def relpose_pattern(n_poses_free, pose_a, pose_b, flags=None):
    """cugo_relpose_pattern: (rowptr, colind) of the upper block CSR of a pure pose graph (host arrays, no GPU)"""
    a, b = _i32(pose_a), _i32(pose_b)
    fl = None if flags is None else np.ascontiguousarray(flags, np.uint8)
    args = (len(a), int(n_poses_free), a.ctypes.data_as(_i32p), b.ctypes.data_as(_i32p),
            None if fl is None else fl.ctypes.data_as(_u8p))
    nnzb = C.c_int(0)
    rowptr = np.zeros(int(n_poses_free) + 1, np.int32)
    check(lib().cugo_relpose_pattern(*args, rowptr.ctypes.data_as(_i32p), None, C.byref(nnzb)))
    colind = np.zeros(max(nnzb.value, 1), np.int32)
    check(lib().cugo_relpose_pattern(*args, rowptr.ctypes.data_as(_i32p), colind.ctypes.data_as(_i32p), C.byref(nnzb)))
    return rowptr, colind[:nnzb.value]


class RelPosePlan:
    """cugo_relpose_plan: incidence lists and off-diagonal block indices of a set of relative-pose edges against an
    upper block-CSR pattern (host arrays).  ctx: a cugo_ctx handle (ctypes.c_void_p), or None for a host-only plan"""

    def __init__(self, ctx, n_poses_total, n_poses_free, pose_a, pose_b, flags, rowptr, colind):
        a, b, rp, ci = _i32(pose_a), _i32(pose_b), _i32(rowptr), _i32(colind)
        fl = None if flags is None else np.ascontiguousarray(flags, np.uint8)
        self._p = C.c_void_p()
        self.n, self.n_poses_total, self.n_poses_free = len(a), int(n_poses_total), int(n_poses_free)
        check(lib().cugo_relpose_plan_create(ctx, len(a), self.n_poses_total, self.n_poses_free,
                                             a.ctypes.data_as(_i32p), b.ctypes.data_as(_i32p),
                                             None if fl is None else fl.ctypes.data_as(_u8p),
                                             rp.ctypes.data_as(_i32p), ci.ctypes.data_as(_i32p), C.byref(self._p)))

    @property
    def handle(self):
        return self._p

    def array(self, name):
        """a copy of the plan array inc_ptr, inc (edge << 1 | side) or off_blk"""
        out = _i32p()
        n = lib().cugo_relpose_plan_array(self._p, name.encode(), C.byref(out))
        if n < 0:
            raise CugoError("cugo error %d: %s" % (n, lib().cugo_last_error().decode()))
        return np.array(out[:n], np.int32)

    def close(self):
        if self._p:
            lib().cugo_relpose_plan_destroy(self._p)
            self._p = C.c_void_p()


class PointPairPlan:
    """cugo_point_pair_plan: the stable sort of a set of pose-pose point edges into runs of one (a, b) orientation of a
    pair, the incidence lists of the free poses and the runs of every pattern block (host arrays).  ctx: a cugo_ctx handle
    (ctypes.c_void_p), or None for a host-only plan; rowptr / colind: the upper block-CSR pattern, or both None for a
    plan without a destination (its pair_lo / pair_hi are what a pattern needs)"""
    ARRAYS = ("perm", "edge_run", "run_ptr", "run_a", "run_b", "run_flags", "run_blk", "inc_ptr", "inc", "blk_id", "blk_ptr",
              "blk_run", "pair_lo", "pair_hi")

    def __init__(self, ctx, n_poses_total, n_poses_free, pose_a, pose_b, flags=None, rowptr=None, colind=None):
        a, b = _i32(pose_a), _i32(pose_b)
        rp, ci = (None if rowptr is None else _i32(rowptr)), (None if colind is None else _i32(colind))
        fl = None if flags is None else np.ascontiguousarray(flags, np.uint8)
        self._p = C.c_void_p()
        self.n, self.n_poses_total, self.n_poses_free = len(a), int(n_poses_total), int(n_poses_free)
        check(lib().cugo_point_pair_plan_create(ctx, len(a), self.n_poses_total, self.n_poses_free,
                                                a.ctypes.data_as(_i32p), b.ctypes.data_as(_i32p),
                                                None if fl is None else fl.ctypes.data_as(_u8p),
                                                None if rp is None else rp.ctypes.data_as(_i32p),
                                                None if ci is None else ci.ctypes.data_as(_i32p), C.byref(self._p)))

    @property
    def handle(self):
        return self._p

    def array(self, name):
        """a copy of the plan array `name` (one of ARRAYS)"""
        out = _i32p()
        n = lib().cugo_point_pair_plan_array(self._p, name.encode(), C.byref(out))
        if n < 0:
            raise CugoError("cugo error %d: %s" % (n, lib().cugo_last_error().decode()))
        return np.array(out[:n], np.int32)

    def close(self):
        if self._p:
            lib().cugo_point_pair_plan_destroy(self._p)
            self._p = C.c_void_p()


class PlCovPlan:
    """cugo_plcov_plan: the plan of a batch of pose-landmark covariance queries (host only, no GPU): the pose pairs to
    ask cugo_chol_inverse_blocks for and, per query, the block every slot of its landmark reads.  lm_ptr / slot_pose:
    the flattened edges (landmark-major slots); q_pose / q_lm: free indices, -1 for a fixed vertex"""

    def __init__(self, n_poses_free, lm_ptr, slot_pose, q_pose, q_lm):
        lp, sp, qp, ql = _i32(lm_ptr), _i32(slot_pose), _i32(q_pose), _i32(q_lm)
        if len(qp) != len(ql):
            raise ValueError("q_pose and q_lm must have the same length")
        self._p = C.c_void_p()
        self.n = len(qp)
        check(lib().cugo_plcov_plan_create(int(n_poses_free), max(len(lp) - 1, 0), _p(lp, _i32p), _p(sp, _i32p), self.n,
                                           _p(qp, _i32p), _p(ql, _i32p), C.byref(self._p)))

    def array(self, name):
        """a copy of the plan array rows, cols, q_ptr, q_slot or q_aa"""
        out = _i32p()
        n = lib().cugo_plcov_plan_array(self._p, name.encode(), C.byref(out))
        if n < 0:
            raise CugoError("cugo error %d: %s" % (n, lib().cugo_last_error().decode()))
        return np.array(out[:n], np.int32)

    def close(self):
        if self._p:
            lib().cugo_plcov_plan_destroy(self._p)
            self._p = C.c_void_p()


def pose_landmark_cross_covariances(ctx, ev, n, d_q_pose, d_q_lm, d_q_ptr, d_q_slot, d_Hll, d_Hpl, d_blocks, d_cov18,
                                    d_fail):
    """cugo_pose_landmark_cross_covariances: Sigma_al [n][18] of n queries from the blocks of a PlCovPlan's pair list
    (device pointers as ctypes.c_void_p; ev: Edges)"""
    check(lib().cugo_pose_landmark_cross_covariances(ctx, C.byref(ev), int(n), d_q_pose, d_q_lm, d_q_ptr, d_q_slot, d_Hll,
                                                     d_Hpl, d_blocks, d_cov18, d_fail))


def reprojection_covariances(ctx, n, n_landmarks_free, d_q_pose, d_q_lm, d_q_dim, d_q_aa, d_cam5, d_poses, d_lms,
                             d_blocks, d_cross18, d_lmcov9, d_cov9):
    """cugo_reprojection_covariances: S = J Sigma J^T [n][9] of n queries (device pointers as ctypes.c_void_p)"""
    check(lib().cugo_reprojection_covariances(ctx, int(n), int(n_landmarks_free), d_q_pose, d_q_lm, d_q_dim, d_q_aa,
                                              d_cam5, d_poses, d_lms, d_blocks, d_cross18, d_lmcov9, d_cov9))


def predict_observations(ctx, n, n_landmarks_free, d_q_pose, d_q_lm, d_q_kind, d_q_aa, d_cam5, d_cam_tab, d_poses, d_lms,
                         d_blocks, d_cross18, d_lmcov9, d_z3, d_cov9):
    """cugo_predict_observations: the predicted observation z [n][3] and S = J Sigma J^T [n][9] of n queries of kind
    OBS_MONO / OBS_STEREO / OBS_DEPTH; d_cam_tab [n][17] (camera_model_table) or None for pinholes at the pose (device
    pointers as ctypes.c_void_p)"""
    check(lib().cugo_predict_observations(ctx, int(n), int(n_landmarks_free), d_q_pose, d_q_lm, d_q_kind, d_q_aa, d_cam5,
                                          d_cam_tab, d_poses, d_lms, d_blocks, d_cross18, d_lmcov9, d_z3, d_cov9))


def relpose_compute_errors(ctx, ev, d_poses, d_chi, d_edge_chi=None):
    """cugo_relpose_compute_errors: chi2 total of `ev` (RelPoseEdges) to d_chi[0], optionally the term of every edge"""
    check(lib().cugo_relpose_compute_errors(ctx, C.byref(ev), d_poses, d_chi, d_edge_chi))


def relpose_construct_quadratic_form(ctx, ev, d_poses, d_Hpp, d_bp, d_Hoff, d_chi=None):
    """cugo_relpose_construct_quadratic_form: diagonal terms ADDED to d_Hpp / d_bp, off-diagonal blocks to d_Hoff
    [nnzb][36] by the plan's block indices"""
    check(lib().cugo_relpose_construct_quadratic_form(ctx, C.byref(ev), d_poses, d_Hpp, d_bp, d_Hoff, d_chi))


def relpose_construct_quadratic_form_diag(ctx, ev, d_poses, d_Hpp, d_bp, d_chi=None):
    """cugo_relpose_construct_quadratic_form_diag: the build pass of the two-stream loop (diagonal terms and b alone)"""
    check(lib().cugo_relpose_construct_quadratic_form_diag(ctx, C.byref(ev), d_poses, d_Hpp, d_bp, d_chi))


def relpose_add_offdiag_schur(ctx, ev, d_poses, d_Hsc):
    """cugo_relpose_add_offdiag_schur: the off-diagonal terms alone ADDED to d_Hsc by the plan's block indices"""
    check(lib().cugo_relpose_add_offdiag_schur(ctx, C.byref(ev), d_poses, d_Hsc))


def relpose_construct_quadratic_form_schur(ctx, ev, d_poses, d_rowptr, d_Hsc, d_bp, d_bsc, d_chi=None):
    """cugo_relpose_construct_quadratic_form_schur: as prior_construct_quadratic_form_schur, plus the off-diagonal
    blocks into d_Hsc by the plan's block indices"""
    check(lib().cugo_relpose_construct_quadratic_form_schur(ctx, C.byref(ev), d_poses, d_rowptr, d_Hsc, d_bp, d_bsc, d_chi))


def point_pair_compute_errors(ctx, ev, d_poses, d_chi, d_edge_chi=None):
    """cugo_point_pair_compute_errors: chi2 total of `ev` (PointPairEdges) to d_chi[0], optionally the term of every edge
    (sorted order)"""
    check(lib().cugo_point_pair_compute_errors(ctx, C.byref(ev), d_poses, d_chi, d_edge_chi))


def point_pair_construct_quadratic_form(ctx, ev, d_poses, d_Hpp, d_bp, d_Hoff, d_chi=None):
    """cugo_point_pair_construct_quadratic_form: diagonal terms ADDED to d_Hpp / d_bp, off-diagonal blocks to d_Hoff
    [nnzb][36] by the plan's block indices"""
    check(lib().cugo_point_pair_construct_quadratic_form(ctx, C.byref(ev), d_poses, d_Hpp, d_bp, d_Hoff, d_chi))


def point_pair_construct_quadratic_form_schur(ctx, ev, d_poses, d_rowptr, d_Hsc, d_bp, d_bsc, d_chi=None):
    """cugo_point_pair_construct_quadratic_form_schur: the same terms into the Schur destination"""
    check(lib().cugo_point_pair_construct_quadratic_form_schur(ctx, C.byref(ev), d_poses, d_rowptr, d_Hsc, d_bp, d_bsc, d_chi))


def point_pair_construct_quadratic_form_diag(ctx, ev, d_poses, d_Hpp, d_bp, d_chi=None):
    """cugo_point_pair_construct_quadratic_form_diag: the diagonal terms and b alone; the off-diagonal partials stay in
    the plan's scratch for point_pair_add_offdiag_schur"""
    check(lib().cugo_point_pair_construct_quadratic_form_diag(ctx, C.byref(ev), d_poses, d_Hpp, d_bp, d_chi))


def point_pair_add_offdiag_schur(ctx, ev, d_Hsc):
    """cugo_point_pair_add_offdiag_schur: the off-diagonal sums of the last build pass ADDED to d_Hsc by block index"""
    check(lib().cugo_point_pair_add_offdiag_schur(ctx, C.byref(ev), d_Hsc))


def gicp_pair_compute_errors(ctx, ev, d_poses, d_chi, d_edge_chi=None):
    """cugo_gicp_pair_compute_errors: as point_pair_compute_errors, for GicpPairEdges (Omega formed at d_poses)"""
    check(lib().cugo_gicp_pair_compute_errors(ctx, C.byref(ev), d_poses, d_chi, d_edge_chi))


def gicp_pair_construct_quadratic_form(ctx, ev, d_poses, d_Hpp, d_bp, d_Hoff, d_chi=None):
    """cugo_gicp_pair_construct_quadratic_form: as point_pair_construct_quadratic_form, for GicpPairEdges"""
    check(lib().cugo_gicp_pair_construct_quadratic_form(ctx, C.byref(ev), d_poses, d_Hpp, d_bp, d_Hoff, d_chi))


def gicp_pair_construct_quadratic_form_schur(ctx, ev, d_poses, d_rowptr, d_Hsc, d_bp, d_bsc, d_chi=None):
    """cugo_gicp_pair_construct_quadratic_form_schur: the same terms into the Schur destination"""
    check(lib().cugo_gicp_pair_construct_quadratic_form_schur(ctx, C.byref(ev), d_poses, d_rowptr, d_Hsc, d_bp, d_bsc, d_chi))


def gicp_pair_construct_quadratic_form_diag(ctx, ev, d_poses, d_Hpp, d_bp, d_chi=None):
    """cugo_gicp_pair_construct_quadratic_form_diag: the diagonal terms and b alone; the off-diagonal partials stay in
    the plan's scratch"""
    check(lib().cugo_gicp_pair_construct_quadratic_form_diag(ctx, C.byref(ev), d_poses, d_Hpp, d_bp, d_chi))


def gicp_pair_add_offdiag_schur(ctx, ev, d_Hsc):
    """cugo_gicp_pair_add_offdiag_schur: the off-diagonal sums of the last build pass ADDED to d_Hsc by block index"""
    check(lib().cugo_gicp_pair_add_offdiag_schur(ctx, C.byref(ev), d_Hsc))


def pose_edges_reject(ctx, n, d_edge_chi, d_threshold, n_threshold, d_flags, d_rejected):
    """cugo_pose_edges_reject: the outlier pass of the pose edge kinds.  Edge e goes iff it is not flagged EDGE_INACTIVE,
    its threshold t (d_threshold[0] with n_threshold == 1, else d_threshold[e]) is > 0 and d_edge_chi[e] > t; its flag byte
    gains EDGE_INACTIVE and its index goes to d_rejected (int32 [n], ascending).  Returns the number of edges that went.
    Handles and pointers as for icp_construct_quadratic_form_schur (ctypes.c_void_p)"""
    count = C.c_int(0)
    check(lib().cugo_pose_edges_reject(ctx, int(n), d_edge_chi, d_threshold, int(n_threshold), d_flags, d_rejected,
                                       C.byref(count)))
    return count.value


def device_count():
    return lib().cugo_device_count()


UNIQUE_ID_BYTES = 128


def set_device(device):
    check(lib().cugo_set_device(int(device)))


class Comm:
    """cugo_comm_*: RCCL communicator over the ranks of a multi-GPU job (collective constructor)"""

    def __init__(self, unique_id, rank, world):
        self._c = C.c_void_p()
        buf = C.create_string_buffer(bytes(unique_id), UNIQUE_ID_BYTES)
        check(lib().cugo_comm_create(buf, int(rank), int(world), C.byref(self._c)))

    def close(self):
        if self._c:
            lib().cugo_comm_destroy(self._c)
            self._c = C.c_void_p()


def create_comm_agreed(dist, rank, world, make_comm, can_try=True, deadline_s=180.0, log=None):
    """Collective creation of the RCCL communicator of a multi-process job WITHOUT the two ways such a step hangs a
    job: a rank that cannot even try (no librccl, no device of its own) while the others block inside
    ncclCommInitRank waiting for it, and a rank whose init never returns.  `dist`: an initialised torch.distributed
    group used as the rendezvous (gloo); `make_comm()`: creates this rank's communicator (cugo.Comm(...)), called in
    a helper thread.  Every rank first reports — without entering a collective — whether it can try (`can_try`); only
    if ALL can, they create their communicators, each with a deadline, and then agree on the outcome.

    Returns ("native", comm) when every rank has a communicator, ("fallback", None) when some rank could not try
    (nobody entered the collective: the job may go on with the host-staged exchange), ("failed", None) when some
    rank's init raised or missed the deadline — the caller must then END THE PROCESS on every rank (os._exit: a
    thread stuck inside RCCL cannot be joined, and the ranks that did get a communicator must not wait for the
    others in the next collective)."""
    import threading
    import torch
    pre = torch.tensor([1.0 if can_try else 0.0])
    dist.all_reduce(pre, op=dist.ReduceOp.MIN)
    if float(pre.item()) < 0.5:
        return "fallback", None
    result = {}

    def run():
        try:
            result["comm"] = make_comm()
        except BaseException as e:  # noqa: BLE001 (reported below; the agreement decides what happens)
            result["error"] = e
    th = threading.Thread(target=run, daemon=True)
    th.start()
    th.join(deadline_s)
    mine_ok = "comm" in result and not th.is_alive()
    if not mine_ok and log is not None:
        log("rank %d: communicator %s" % (rank, "failed: %s" % result["error"] if "error" in result
                                          else "did not come back within %.0f s" % deadline_s))
    ok = torch.tensor([1.0 if mine_ok else 0.0])
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    if float(ok.item()) < 0.5:
        return "failed", None
    return "native", result["comm"]


def comm_unique_id():
    """rank 0 of a multi-GPU job: the RCCL unique id to hand to every rank (bytes)"""
    buf = C.create_string_buffer(UNIQUE_ID_BYTES)
    check(lib().cugo_comm_unique_id(buf))
    return buf.raw


def _p(a, t):
    return a.ctypes.data_as(t)


def synth(n_poses, n_landmarks, n_edges, seed, stereo_fraction=0.7, pixel_noise=1.0,
          pose_rot_noise=0.005, pose_trans_noise=0.05, landmark_noise_rel=0.01, n_loop_closures=0):
    """seeded synthetic graph (host only). Returns dict of numpy arrays (ids == positions)."""
    prm = SynthParams(n_poses, n_landmarks, n_edges, stereo_fraction, pixel_noise, pose_rot_noise,
                      pose_trans_noise, landmark_noise_rel, n_loop_closures, seed)
    d = dict(pose=np.zeros((n_poses, 7)), lm=np.zeros((n_landmarks, 3)),
             e_pose=np.zeros(n_edges, np.int32), e_lm=np.zeros(n_edges, np.int32),
             e_stereo=np.zeros(n_edges, np.uint8), e_meas=np.zeros((n_edges, 3)),
             e_omega=np.zeros(n_edges), cam=np.zeros(5))
    check(lib().cugo_synth_generate(C.byref(prm), _p(d["pose"], _f64p), _p(d["lm"], _f64p),
                                    _p(d["e_pose"], _i32p), _p(d["e_lm"], _i32p),
                                    _p(d["e_stereo"], _u8p), _p(d["e_meas"], _f64p),
                                    _p(d["e_omega"], _f64p), _p(d["cam"], _f64p)))
    d["pose_fixed"] = np.zeros(n_poses, np.uint8)
    d["pose_fixed"][0] = 1
    d["lm_fixed"] = np.zeros(n_landmarks, np.uint8)
    d["e_cam"] = np.tile(d["cam"], (n_edges, 1))
    return d


def shard_range(edges_per_landmark, rank, world):
    e = np.ascontiguousarray(edges_per_landmark, np.int32)
    a, b = C.c_int(), C.c_int()
    check(lib().cugo_shard_range(len(e), _p(e, _i32p), rank, world, C.byref(a), C.byref(b)))
    return a.value, b.value


class Graph:
    """cugo_graph_*: the reference's public optimiser class behind a flat-array interface
    (ref: include/cuda_graph_optimisation.h:132-252)."""

    def __init__(self, per_edge_information=True, per_edge_camera=True, plan_only=False):
        self._g = C.c_void_p()
        create = lib().cugo_graph_create_plan_only if plan_only else lib().cugo_graph_create
        check(create(int(per_edge_information), int(per_edge_camera), C.byref(self._g)))
        self._cb = None
        self.pose_ids = np.zeros(0, np.int32)
        self.lm_ids = np.zeros(0, np.int32)

    def close(self):
        if self._g:
            lib().cugo_graph_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_poses(self, ids, q_t7, fixed):
        ids = np.ascontiguousarray(ids, np.int32); q = np.ascontiguousarray(q_t7, np.float64)
        f = np.ascontiguousarray(fixed, np.uint8)
        check(lib().cugo_graph_add_poses(self._g, len(ids), _p(ids, _i32p), _p(q, _f64p), _p(f, _u8p)))
        self.pose_ids = np.concatenate([self.pose_ids, ids])

    def add_landmarks(self, ids, xyz, fixed):
        ids = np.ascontiguousarray(ids, np.int32); x = np.ascontiguousarray(xyz, np.float64)
        f = np.ascontiguousarray(fixed, np.uint8)
        check(lib().cugo_graph_add_landmarks(self._g, len(ids), _p(ids, _i32p), _p(x, _f64p), _p(f, _u8p)))
        self.lm_ids = np.concatenate([self.lm_ids, ids])

    def add_edges(self, dim, pose_ids, lm_ids, meas, info, cam5=None, sensor=None, model=None, distortion=None):
        """distortion: a radial-tangential lens distortion per edge, [n][5] = (k1, k2, p1, p2, k3) in OpenCV's order (the
        measurements are then raw pixels); like cam5 and sensor it follows the camera (per_edge_camera) and does not go
        together with model.  None: the set's (set_camera_distortion).
        model: a projection model per edge, [n][5] = (k1, k2, k3, k4, type) with type 0 pinhole / 1 Kannala-Brandt; like
        cam5 and sensor it follows the camera (per_edge_camera).  None: the set's (set_camera_model).
        sensor: a sensor pose (q, t) body -> sensor per edge, [n][7] (a rig: the poses are then world -> body); it
        follows the camera, so it counts on a graph with per_edge_camera, like cam5.  None: the set's (set_sensor_pose)"""
        n = len(pose_ids)
        if n == 0:
            return
        pi = np.ascontiguousarray(pose_ids, np.int32); li = np.ascontiguousarray(lm_ids, np.int32)
        m = np.ascontiguousarray(np.asarray(meas, np.float64)[:, :dim])
        w = np.ascontiguousarray(info, np.float64)
        cam = None if cam5 is None else np.ascontiguousarray(cam5, np.float64)
        if distortion is not None:
            if model is not None:
                raise CugoError("add_edges: distortion and model do not go together")
            d5 = np.ascontiguousarray(distortion, np.float64)
            if d5.shape != (n, 5):
                raise CugoError("add_edges: distortion must be [n][5] (k1, k2, p1, p2, k3)")
            sx = None if sensor is None else np.ascontiguousarray(sensor, np.float64)
            if sx is not None and sx.shape != (n, 7):
                raise CugoError("add_edges: sensor must be [n][7] (qx, qy, qz, qw, tx, ty, tz)")
            check(lib().cugo_graph_add_edges_distorted(self._g, dim, n, _p(pi, _i32p), _p(li, _i32p), _p(m, _f64p),
                                                       _p(w, _f64p), None if cam is None else _p(cam, _f64p),
                                                       None if sx is None else _p(sx, _f64p), _p(d5, _f64p)))
            return
        if model is not None:
            mk = np.ascontiguousarray(model, np.float64)
            if mk.shape != (n, 5):
                raise CugoError("add_edges: model must be [n][5] (k1, k2, k3, k4, type)")
            sx = None if sensor is None else np.ascontiguousarray(sensor, np.float64)
            if sx is not None and sx.shape != (n, 7):
                raise CugoError("add_edges: sensor must be [n][7] (qx, qy, qz, qw, tx, ty, tz)")
            check(lib().cugo_graph_add_edges_model(self._g, dim, n, _p(pi, _i32p), _p(li, _i32p), _p(m, _f64p),
                                                   _p(w, _f64p), None if cam is None else _p(cam, _f64p),
                                                   None if sx is None else _p(sx, _f64p), _p(mk, _f64p)))
            return
        if sensor is None:
            check(lib().cugo_graph_add_edges(self._g, dim, n, _p(pi, _i32p), _p(li, _i32p), _p(m, _f64p),
                                             _p(w, _f64p), None if cam is None else _p(cam, _f64p)))
            return
        sx = np.ascontiguousarray(sensor, np.float64)
        if sx.shape != (n, 7):
            raise CugoError("add_edges: sensor must be [n][7] (qx, qy, qz, qw, tx, ty, tz)")
        check(lib().cugo_graph_add_edges_rig(self._g, dim, n, _p(pi, _i32p), _p(li, _i32p), _p(m, _f64p), _p(w, _f64p),
                                             None if cam is None else _p(cam, _f64p), _p(sx, _f64p)))

    def set_sensor_pose(self, dim, q_t7):
        """the sensor pose body -> sensor (qx, qy, qz, qw, tx, ty, tz) of the mono (dim 2) or stereo (dim 3) set"""
        q = np.ascontiguousarray(q_t7, np.float64)
        if q.shape != (7,):
            raise CugoError("set_sensor_pose: q_t7 must hold 7 numbers")
        check(lib().cugo_graph_set_sensor_pose(self._g, dim, _p(q, _f64p)))

    def set_camera_model(self, dim, model, k4=None):
        """the projection model of the mono (dim 2) or stereo (dim 3) set: model 0 pinhole, 1 Kannala-Brandt with the
        coefficients k4 = (k1, k2, k3, k4) (None: zeros, the equidistant model)"""
        k = np.zeros(4) if k4 is None else np.ascontiguousarray(k4, np.float64)
        if k.shape != (4,):
            raise CugoError("set_camera_model: k4 must hold 4 numbers")
        check(lib().cugo_graph_set_camera_model(self._g, dim, int(model), _p(k, _f64p)))

    def set_camera_distortion(self, dim, d5=None):
        """the radial-tangential lens distortion of the mono (dim 2) or stereo (dim 3) set: d5 = (k1, k2, p1, p2, k3) in
        OpenCV's order (None: zeros, no distortion).  The set's measurements are then raw pixels"""
        d = np.zeros(5) if d5 is None else np.ascontiguousarray(d5, np.float64)
        if d.shape != (5,):
            raise CugoError("set_camera_distortion: d5 must hold 5 numbers")
        check(lib().cugo_graph_set_camera_distortion(self._g, dim, _p(d, _f64p)))

    def n_distorted_cameras(self):
        """camera-table entries of the current flattening whose lens distortion is not all zero"""
        n = lib().cugo_graph_n_distorted_cameras(self._g)
        if n < 0:
            check(n)
        return n

    def flat_camera_distortions(self):
        """the lens distortions of the camera table of the current flattening, [n][5] = (k1, k2, p1, p2, k3), parallel to
        flat_cameras()"""
        n = lib().cugo_graph_get_flat_camera_distortions(self._g, 0, None)
        if n < 0:
            check(n)
        d = np.zeros((n, 5))
        rc = lib().cugo_graph_get_flat_camera_distortions(self._g, n, _p(d, _f64p))
        if rc < 0:
            check(rc)
        return d

    def n_fisheye_cameras(self):
        """camera-table entries of the current flattening whose model is Kannala-Brandt"""
        n = lib().cugo_graph_n_fisheye_cameras(self._g)
        if n < 0:
            check(n)
        return n

    def flat_camera_models(self):
        """the projection models of the camera table of the current flattening, [n][5] = (k1, k2, k3, k4, type),
        parallel to flat_cameras()"""
        n = lib().cugo_graph_get_flat_camera_models(self._g, 0, None)
        if n < 0:
            check(n)
        mk = np.zeros((n, 5))
        rc = lib().cugo_graph_get_flat_camera_models(self._g, n, _p(mk, _f64p))
        if rc < 0:
            check(rc)
        return mk

    def n_rig_cameras(self):
        """camera-table entries of the current flattening whose sensor pose is not the identity"""
        n = lib().cugo_graph_n_rig_cameras(self._g)
        if n < 0:
            check(n)
        return n

    def flat_cameras(self):
        """the camera table of the current flattening: dict(cams [n][5], ext [n][12] = {M row-major, t_s}, has_rig)"""
        n = lib().cugo_graph_get_flat_cameras(self._g, 0, None, None, None)
        if n < 0:
            check(n)
        cams = np.zeros((n, 5)); ext = np.zeros((n, 12)); hr = C.c_int(0)
        rc = lib().cugo_graph_get_flat_cameras(self._g, n, _p(cams, _f64p), _p(ext, _f64p), C.byref(hr))
        if rc < 0:
            check(rc)
        return dict(cams=cams, ext=ext, has_rig=bool(hr.value))

    def set_camera(self, dim, cam5):
        c = np.ascontiguousarray(cam5, np.float64)
        check(lib().cugo_graph_set_camera(self._g, dim, _p(c, _f64p)))

    def set_information(self, dim, info):
        check(lib().cugo_graph_set_information(self._g, dim, C.c_double(info)))

    def set_robust_kernel(self, dim, rk_type, delta):
        check(lib().cugo_graph_set_robust_kernel(self._g, dim, int(rk_type), C.c_double(delta)))

    def add_plane_edges(self, pose_ids, pointP, normal, origin_distance, info=None):
        """point-to-plane pose edges (ref: PlaneEdgeSet): residual normal . (R pointP + t) - origin_distance; the
        normal must be of unit length (initialize() refuses otherwise).  info: per edge, or None for the set's value"""
        n = len(pose_ids)
        if n == 0:
            return
        pi = np.ascontiguousarray(pose_ids, np.int32)
        p = np.ascontiguousarray(np.asarray(pointP, np.float64).reshape(n, 3))
        nn = np.ascontiguousarray(np.asarray(normal, np.float64).reshape(n, 3))
        d = np.ascontiguousarray(np.asarray(origin_distance, np.float64).reshape(n))
        w = None if info is None else np.ascontiguousarray(np.broadcast_to(np.asarray(info, np.float64), (n,)))
        check(lib().cugo_graph_add_plane_edges(self._g, n, _p(pi, _i32p), _p(p, _f64p), _p(nn, _f64p), _p(d, _f64p),
                                               None if w is None else _p(w, _f64p)))

    def add_line_edges(self, pose_ids, pointP, a, b, info=None):
        """point-to-line pose edges (ref: LineEdgeSet): the distance of R pointP + t to the line through a and b"""
        n = len(pose_ids)
        if n == 0:
            return
        pi = np.ascontiguousarray(pose_ids, np.int32)
        p = np.ascontiguousarray(np.asarray(pointP, np.float64).reshape(n, 3))
        aa = np.ascontiguousarray(np.asarray(a, np.float64).reshape(n, 3))
        bb = np.ascontiguousarray(np.asarray(b, np.float64).reshape(n, 3))
        w = None if info is None else np.ascontiguousarray(np.broadcast_to(np.asarray(info, np.float64), (n,)))
        check(lib().cugo_graph_add_line_edges(self._g, n, _p(pi, _i32p), _p(p, _f64p), _p(aa, _f64p), _p(bb, _f64p),
                                              None if w is None else _p(w, _f64p)))

    def set_icp_information(self, kind, info):
        """kind: ICP_PLANE / ICP_LINE; the set's information (used when per_edge_information is off)"""
        check(lib().cugo_graph_set_icp_information(self._g, int(kind), C.c_double(info)))

    def set_icp_robust_kernel(self, kind, rk_type, delta):
        check(lib().cugo_graph_set_icp_robust_kernel(self._g, int(kind), int(rk_type), C.c_double(delta)))

    def set_icp_outlier_threshold(self, kind, threshold):
        """chi2 threshold of the set (kind: ICP_PLANE / ICP_LINE; ref: EdgeSet::setOutlierThreshold).  With
        set_option("pose_edge_outliers", 1) the edges above it are inactivated at the end of optimize(); without the
        option initialize() refuses a positive threshold.  0 (or any value that is not a finite positive number) disables"""
        check(lib().cugo_graph_set_icp_outlier_threshold(self._g, int(kind), C.c_double(threshold)))

    def n_icp_edges(self, kind):
        """active edges of the kind in the current flattening (edges on fixed poses are not counted)"""
        return lib().cugo_graph_n_icp_edges(self._g, int(kind))

    def add_pose_priors(self, pose_ids, q_t7, info36=None):
        """SE(3) pose priors (an extension; PosePriorEdgeSet): residual [Log_SO3(R R_z^T); t - R R_z^T t_z] against the
        measured pose q_t7 [n, 7], cost r^T Omega r.  info36: [n, 6, 6] (or one 6 x 6 for all), order [rotation,
        translation] as pose_covariances(); None for the set's matrix (set_prior_information)"""
        n = len(pose_ids)
        if n == 0:
            return
        pi = np.ascontiguousarray(pose_ids, np.int32)
        z = np.ascontiguousarray(np.asarray(q_t7, np.float64).reshape(n, 7))
        w = None if info36 is None else np.ascontiguousarray(
            np.broadcast_to(np.asarray(info36, np.float64).reshape(-1, 36), (n, 36)))
        check(lib().cugo_graph_add_pose_priors(self._g, n, _p(pi, _i32p), _p(z, _f64p),
                                               None if w is None else _p(w, _f64p)))

    def set_prior_information(self, info36):
        """the prior set's 6 x 6 information (used when per_edge_information is off, or for priors added without one)"""
        w = np.ascontiguousarray(np.asarray(info36, np.float64).reshape(36))
        check(lib().cugo_graph_set_prior_information(self._g, _p(w, _f64p)))

    def set_prior_robust_kernel(self, rk_type, delta):
        check(lib().cugo_graph_set_prior_robust_kernel(self._g, int(rk_type), C.c_double(delta)))

    def set_prior_outlier_threshold(self, threshold):
        """chi2 threshold of the prior set, as set_icp_outlier_threshold (needs set_option("pose_edge_outliers", 1))"""
        check(lib().cugo_graph_set_prior_outlier_threshold(self._g, C.c_double(threshold)))

    def n_prior_edges(self):
        """active priors in the current flattening (priors on fixed poses are not counted)"""
        return lib().cugo_graph_n_prior_edges(self._g)

    def add_landmark_priors(self, lm_ids, xyz3, info9=None):
        """landmark position priors (an extension; LandmarkPriorEdgeSet): residual X - Z against the measured position
        xyz3 [n, 3], cost r^T Omega r.  info9: [n, 3, 3] (or one 3 x 3 for all); None for the set's matrix
        (set_landmark_prior_information).  An unknown landmark id refuses the whole call"""
        n = len(lm_ids)
        if n == 0:
            return
        li = np.ascontiguousarray(lm_ids, np.int32)
        z = np.ascontiguousarray(np.asarray(xyz3, np.float64).reshape(n, 3))
        w = None if info9 is None else np.ascontiguousarray(
            np.broadcast_to(np.asarray(info9, np.float64).reshape(-1, 9), (n, 9)))
        check(lib().cugo_graph_add_landmark_priors(self._g, n, _p(li, _i32p), _p(z, _f64p),
                                                   None if w is None else _p(w, _f64p)))

    def set_landmark_prior_information(self, info9):
        """the landmark-prior set's 3 x 3 information (used when per_edge_information is off, or for priors added
        without one)"""
        w = np.ascontiguousarray(np.asarray(info9, np.float64).reshape(9))
        check(lib().cugo_graph_set_landmark_prior_information(self._g, _p(w, _f64p)))

    def set_landmark_prior_robust_kernel(self, rk_type, delta):
        check(lib().cugo_graph_set_landmark_prior_robust_kernel(self._g, int(rk_type), C.c_double(delta)))

    def n_landmark_prior_edges(self):
        """landmark priors that count in the current flattening (priors on fixed landmarks are not counted)"""
        return lib().cugo_graph_n_landmark_prior_edges(self._g)

    def add_point_edges(self, pose_ids, pointP, pointZ, info9=None):
        """point-to-point pose edges (an extension; PointEdgeSet): residual R(q) p + t - z of the known points pointP [n, 3]
        against their measurements pointZ [n, 3] in the pose's frame, cost r^T Omega r.  info9: [n, 3, 3] (or one 3 x 3 for
        all; positive SEMI-definite); None for the set's matrix (set_point_information).  An unknown pose id refuses the
        whole call"""
        n = len(pose_ids)
        if n == 0:
            return
        pi = np.ascontiguousarray(pose_ids, np.int32)
        p = np.ascontiguousarray(np.asarray(pointP, np.float64).reshape(n, 3))
        z = np.ascontiguousarray(np.asarray(pointZ, np.float64).reshape(n, 3))
        w = None if info9 is None else np.ascontiguousarray(
            np.broadcast_to(np.asarray(info9, np.float64).reshape(-1, 9), (n, 9)))
        check(lib().cugo_graph_add_point_edges(self._g, n, _p(pi, _i32p), _p(p, _f64p), _p(z, _f64p),
                                               None if w is None else _p(w, _f64p)))

    def set_point_information(self, info9):
        """the point set's 3 x 3 information: the matrix that counts when per_edge_information is off.  An edge added
        without a matrix of its own takes a COPY of the set's matrix at the time of the add; a later call does not
        reach it when per_edge_information is on"""
        w = np.ascontiguousarray(np.asarray(info9, np.float64).reshape(9))
        check(lib().cugo_graph_set_point_information(self._g, _p(w, _f64p)))

    def set_point_robust_kernel(self, rk_type, delta):
        check(lib().cugo_graph_set_point_robust_kernel(self._g, int(rk_type), C.c_double(delta)))

    def n_point_edges(self):
        """point edges that count in the current flattening (edges on fixed poses are not counted)"""
        return lib().cugo_graph_n_point_edges(self._g)

    def flat_point_edges(self):
        """the point edges of the current flattening as the kernels read them (a diagnostic; works on a plan-only graph):
        dict(pose [n] ascending flattened pose index, src [n] position of each edge among the edges added, p [3, n],
        z [3, n], info [6, n_info] the packed upper triangles 00 01 02 11 12 22, n_info = n or 1)"""
        ni = C.c_int(0)
        n = lib().cugo_graph_get_flat_point_edges(self._g, 0, None, None, None, None, None, C.byref(ni))
        if n < 0:
            check(n)
        pose, src = np.zeros(n, np.int32), np.zeros(n, np.int32)
        p, z, info = np.zeros((3, n)), np.zeros((3, n)), np.zeros((6, ni.value if n else 0))
        rc = lib().cugo_graph_get_flat_point_edges(self._g, n, _p(pose, _i32p), _p(src, _i32p), _p(p, _f64p), _p(z, _f64p),
                                                   _p(info, _f64p), C.byref(ni))
        if rc < 0:
            check(rc)
        return dict(pose=pose, src=src, p=p, z=z, info=info, n_info=ni.value)

    def add_point_pair_edges(self, pose_ids_a, pose_ids_b, pointP, pointZ, info9=None):
        """pose-pose point edges (an extension; PointPairEdgeSet) for scan-to-scan registration: the points pointP [n, 3]
        measured in pose a's frame, the same physical points measured as pointZ [n, 3] in pose b's frame; residual
        R_b R_a^T (p - t_a) + t_b - z, cost r^T Omega r with Omega in b's frame.  info9: [n, 3, 3] (or one 3 x 3 for all;
        positive SEMI-definite); None for the set's matrix (set_point_pair_information).  An unknown pose id or a == b
        refuses the whole call"""
        n = len(pose_ids_a)
        if n == 0:
            return
        ia, ib = np.ascontiguousarray(pose_ids_a, np.int32), np.ascontiguousarray(pose_ids_b, np.int32)
        if len(ib) != n:
            raise ValueError("pose_ids_a and pose_ids_b must have the same length")
        p = np.ascontiguousarray(np.asarray(pointP, np.float64).reshape(n, 3))
        z = np.ascontiguousarray(np.asarray(pointZ, np.float64).reshape(n, 3))
        w = None if info9 is None else np.ascontiguousarray(
            np.broadcast_to(np.asarray(info9, np.float64).reshape(-1, 9), (n, 9)))
        check(lib().cugo_graph_add_point_pair_edges(self._g, n, _p(ia, _i32p), _p(ib, _i32p), _p(p, _f64p), _p(z, _f64p),
                                                    None if w is None else _p(w, _f64p)))

    def set_point_pair_information(self, info9):
        """the pair set's 3 x 3 information, with the rule of set_point_information"""
        w = np.ascontiguousarray(np.asarray(info9, np.float64).reshape(9))
        check(lib().cugo_graph_set_point_pair_information(self._g, _p(w, _f64p)))

    def set_point_pair_robust_kernel(self, rk_type, delta):
        check(lib().cugo_graph_set_point_pair_robust_kernel(self._g, int(rk_type), C.c_double(delta)))

    def set_point_pair_outlier_threshold(self, threshold):
        """chi2 threshold of the pair set; initialize() refuses a positive one (outlier rejection on the set: not yet)"""
        check(lib().cugo_graph_set_point_pair_outlier_threshold(self._g, C.c_double(threshold)))

    def set_point_pair_active(self, active, first=0):
        """active flags of the pair edges first, first + 1, ... (insertion order); takes effect at the next initialize()"""
        a = np.ascontiguousarray(np.asarray(active).astype(np.uint8))
        check(lib().cugo_graph_set_point_pair_active(self._g, int(first), len(a), _p(a, _u8p)))

    def n_point_pair_edges(self):
        """pair edges that count in the current flattening (edges between two fixed poses do not)"""
        return lib().cugo_graph_n_point_pair_edges(self._g)

    def flat_point_pair_edges(self):
        """the pair edges of the current flattening as the kernels read them (a diagnostic; works on a plan-only graph):
        dict(pose_a, pose_b [n] flattened pose indices in the order of the plan (runs of one orientation of a pair, by
        (lo, hi, orientation)), src [n] position of each edge among the edges added, p [3, n], z [3, n], info [6, n_info]
        the packed upper triangles 00 01 02 11 12 22, n_info = n or 1)"""
        ni = C.c_int(0)
        n = lib().cugo_graph_get_flat_point_pair_edges(self._g, 0, None, None, None, None, None, None, C.byref(ni))
        if n < 0:
            check(n)
        pa, pb, src = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        p, z, info = np.zeros((3, n)), np.zeros((3, n)), np.zeros((6, ni.value if n else 0))
        rc = lib().cugo_graph_get_flat_point_pair_edges(self._g, n, _p(pa, _i32p), _p(pb, _i32p), _p(src, _i32p), _p(p, _f64p),
                                                        _p(z, _f64p), _p(info, _f64p), C.byref(ni))
        if rc < 0:
            check(rc)
        return dict(pose_a=pa, pose_b=pb, src=src, p=p, z=z, info=info, n_info=ni.value)

    @staticmethod
    def _cov9(c, n):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(c, np.float64).reshape(-1, 9), (n, 9)))

    def add_gicp_edges(self, pose_ids, pointP, pointZ, covP9, covZ9):
        """covariance-form point edges (an extension; GicpEdgeSet, generalised ICP against a fixed map): known points
        pointP [n, 3] with covariances covP9 [n, 3, 3] in the world frame, their measurements pointZ with covZ9 in the
        pose's frame (one 3 x 3 serves all); Omega = (C_z + R C_p R^T)^-1 is rebuilt at every linearisation and trial of
        optimize().  An unknown pose id refuses the whole call"""
        n = len(pose_ids)
        if n == 0:
            return
        ids = np.ascontiguousarray(pose_ids, np.int32)
        p = np.ascontiguousarray(np.asarray(pointP, np.float64).reshape(n, 3))
        z = np.ascontiguousarray(np.asarray(pointZ, np.float64).reshape(n, 3))
        cp, cz = self._cov9(covP9, n), self._cov9(covZ9, n)
        check(lib().cugo_graph_add_gicp_edges(self._g, n, _p(ids, _i32p), _p(p, _f64p), _p(z, _f64p), _p(cp, _f64p), _p(cz, _f64p)))

    def add_gicp_pair_edges(self, pose_ids_a, pose_ids_b, pointP, pointZ, covP9, covZ9):
        """covariance-form pose-pose point edges (an extension; GicpPairEdgeSet, scan-to-scan generalised ICP): pointP,
        covP9 in pose a's frame, pointZ, covZ9 in pose b's; Omega = (C_z + M C_p M^T)^-1 with M = R_b R_a^T follows the
        poses inside optimize().  An unknown pose id or a == b refuses the whole call"""
        n = len(pose_ids_a)
        if n == 0:
            return
        ia, ib = np.ascontiguousarray(pose_ids_a, np.int32), np.ascontiguousarray(pose_ids_b, np.int32)
        if len(ib) != n:
            raise ValueError("pose_ids_a and pose_ids_b must have the same length")
        p = np.ascontiguousarray(np.asarray(pointP, np.float64).reshape(n, 3))
        z = np.ascontiguousarray(np.asarray(pointZ, np.float64).reshape(n, 3))
        cp, cz = self._cov9(covP9, n), self._cov9(covZ9, n)
        check(lib().cugo_graph_add_gicp_pair_edges(self._g, n, _p(ia, _i32p), _p(ib, _i32p), _p(p, _f64p), _p(z, _f64p),
                                                   _p(cp, _f64p), _p(cz, _f64p)))

    def set_gicp_robust_kernel(self, rk_type, delta):
        check(lib().cugo_graph_set_gicp_robust_kernel(self._g, int(rk_type), C.c_double(delta)))

    def set_gicp_pair_robust_kernel(self, rk_type, delta):
        check(lib().cugo_graph_set_gicp_pair_robust_kernel(self._g, int(rk_type), C.c_double(delta)))

    def set_gicp_outlier_threshold(self, threshold):
        """initialize() refuses a positive one (outlier rejection on the set: not yet)"""
        check(lib().cugo_graph_set_gicp_outlier_threshold(self._g, C.c_double(threshold)))

    def set_gicp_pair_outlier_threshold(self, threshold):
        """initialize() refuses a positive one (outlier rejection on the set: not yet)"""
        check(lib().cugo_graph_set_gicp_pair_outlier_threshold(self._g, C.c_double(threshold)))

    def set_gicp_pair_active(self, active, first=0):
        """active flags of the covariance-form pair edges first, first + 1, ...; takes effect at the next initialize()"""
        a = np.ascontiguousarray(np.asarray(active).astype(np.uint8))
        check(lib().cugo_graph_set_gicp_pair_active(self._g, int(first), len(a), _p(a, _u8p)))

    def n_gicp_edges(self):
        return lib().cugo_graph_n_gicp_edges(self._g)

    def n_gicp_pair_edges(self):
        return lib().cugo_graph_n_gicp_pair_edges(self._g)

    def flat_gicp_edges(self):
        """the covariance-form point edges of the current flattening as the kernels read them (a diagnostic; works on a
        plan-only graph): dict(pose, src [n], p, z [3, n], cov_p, cov_z [6, n_cov] packed upper triangles, n_cov = n or 1)"""
        nc = C.c_int(0)
        n = lib().cugo_graph_get_flat_gicp_edges(self._g, 0, None, None, None, None, None, None, C.byref(nc))
        if n < 0:
            check(n)
        pose, src = np.zeros(n, np.int32), np.zeros(n, np.int32)
        p, z, cp, cz = np.zeros((3, n)), np.zeros((3, n)), np.zeros((6, nc.value)), np.zeros((6, nc.value))
        rc = lib().cugo_graph_get_flat_gicp_edges(self._g, n, _p(pose, _i32p), _p(src, _i32p), _p(p, _f64p), _p(z, _f64p),
                                                  _p(cp, _f64p), _p(cz, _f64p), C.byref(nc))
        if rc < 0:
            check(rc)
        return dict(pose=pose, src=src, p=p, z=z, cov_p=cp, cov_z=cz, n_cov=nc.value)

    def flat_gicp_pair_edges(self):
        """as flat_point_pair_edges, with cov_p, cov_z [6, n_cov] in place of info"""
        nc = C.c_int(0)
        n = lib().cugo_graph_get_flat_gicp_pair_edges(self._g, 0, None, None, None, None, None, None, None, C.byref(nc))
        if n < 0:
            check(n)
        pa, pb, src = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        p, z, cp, cz = np.zeros((3, n)), np.zeros((3, n)), np.zeros((6, nc.value)), np.zeros((6, nc.value))
        rc = lib().cugo_graph_get_flat_gicp_pair_edges(self._g, n, _p(pa, _i32p), _p(pb, _i32p), _p(src, _i32p), _p(p, _f64p),
                                                       _p(z, _f64p), _p(cp, _f64p), _p(cz, _f64p), C.byref(nc))
        if rc < 0:
            check(rc)
        return dict(pose_a=pa, pose_b=pb, src=src, p=p, z=z, cov_p=cp, cov_z=cz, n_cov=nc.value)

    def add_relpose_edges(self, pose_ids_a, pose_ids_b, q_t7, info36=None):
        """relative-pose SE(3) edges (an extension; RelPoseEdgeSet): residual [Log_SO3(R_D); t_D] of D = T_a T_b^-1 Z^-1
        against the measured relative pose q_t7 [n, 7], cost r^T Omega r.  info36 as for add_pose_priors; None for the
        set's matrix (set_relpose_information).  The pose pairs become blocks of the Schur complement's pattern"""
        n = len(pose_ids_a)
        if n == 0:
            return
        if len(pose_ids_b) != n:
            raise ValueError("add_relpose_edges: pose_ids_a and pose_ids_b differ in length")
        pa, pb = _i32(pose_ids_a), _i32(pose_ids_b)
        z = np.ascontiguousarray(np.asarray(q_t7, np.float64).reshape(n, 7))
        w = None if info36 is None else np.ascontiguousarray(
            np.broadcast_to(np.asarray(info36, np.float64).reshape(-1, 36), (n, 36)))
        check(lib().cugo_graph_add_relpose_edges(self._g, n, _p(pa, _i32p), _p(pb, _i32p), _p(z, _f64p),
                                                 None if w is None else _p(w, _f64p)))

    def set_relpose_information(self, info36):
        """the relative-pose set's 6 x 6 information (used when per_edge_information is off, or for edges added without one)"""
        w = np.ascontiguousarray(np.asarray(info36, np.float64).reshape(36))
        check(lib().cugo_graph_set_relpose_information(self._g, _p(w, _f64p)))

    def set_relpose_robust_kernel(self, rk_type, delta):
        check(lib().cugo_graph_set_relpose_robust_kernel(self._g, int(rk_type), C.c_double(delta)))

    def set_relpose_outlier_threshold(self, threshold):
        """chi2 threshold of the relative-pose set, as set_icp_outlier_threshold (needs set_option("pose_edge_outliers",
        1)): false loop closures are dropped at the end of optimize() and left out by the next initialize()"""
        check(lib().cugo_graph_set_relpose_outlier_threshold(self._g, C.c_double(threshold)))

    def set_relpose_active(self, active, first=0):
        """active flags of the relative-pose edges first, first + 1, ... (insertion order); takes effect at the next initialize()"""
        a = np.ascontiguousarray(np.asarray(active).astype(np.uint8))
        check(lib().cugo_graph_set_relpose_active(self._g, int(first), len(a), _p(a, _u8p)))

    def n_relpose_edges(self):
        """relative-pose edges that count in the current flattening (edges between two fixed poses do not)"""
        return lib().cugo_graph_n_relpose_edges(self._g)

    def add_depth_edges(self, pose_ids, lm_ids, meas3, info, cam5=None):
        """depth edges (ref: DepthEdgeSet): observations (u, v, 1/Z) with the residual
        (pu - u, pv - v, sqrt(k) (1/Z - m_d)), k the set's inverse-depth weight (set_depth_weight).  info: per edge, or
        None for the set's value; cam5 [n][5] or None for the set's camera (bf is not used)"""
        n = len(pose_ids)
        if n == 0:
            return
        pi = np.ascontiguousarray(pose_ids, np.int32); li = np.ascontiguousarray(lm_ids, np.int32)
        m = np.ascontiguousarray(np.asarray(meas3, np.float64)[:, :3])
        w = None if info is None else np.ascontiguousarray(info, np.float64)
        cam = None if cam5 is None else np.ascontiguousarray(cam5, np.float64)
        check(lib().cugo_graph_add_depth_edges(self._g, n, _p(pi, _i32p), _p(li, _i32p), _p(m, _f64p),
                                               None if w is None else _p(w, _f64p),
                                               None if cam is None else _p(cam, _f64p)))

    def set_depth_camera(self, cam5):
        c = np.ascontiguousarray(cam5, np.float64)
        check(lib().cugo_graph_set_depth_camera(self._g, _p(c, _f64p)))

    def set_depth_information(self, info):
        check(lib().cugo_graph_set_depth_information(self._g, C.c_double(info)))

    def set_depth_robust_kernel(self, rk_type, delta):
        check(lib().cugo_graph_set_depth_robust_kernel(self._g, int(rk_type), C.c_double(delta)))

    def set_depth_outlier_threshold(self, threshold):
        """as set_outlier_threshold, for the depth edge set"""
        check(lib().cugo_graph_set_depth_outlier_threshold(self._g, C.c_double(threshold)))

    def set_depth_weight(self, weight):
        """k, the inverse-depth weight of the depth edge set (default 1); initialize() refuses a value that is not
        finite and > 0.  Changing it counts as a change of the set"""
        check(lib().cugo_graph_set_depth_weight(self._g, C.c_double(weight)))

    def n_depth_outliers(self):
        return lib().cugo_graph_n_depth_outliers(self._g)

    def depth_edge_active(self, n):
        out = np.zeros(n, np.uint8)
        check(lib().cugo_graph_get_depth_edge_active(self._g, n, _p(out, _u8p)))
        return out.astype(bool)

    def flat_edges(self):
        """the pose-landmark edges of the current flattening, in flattening order: dict(pose, lm, flags, meas [n][3],
        has_depth, depth_weight) — mono, stereo and depth edges share the array (flag bits EDGE_*)"""
        n = lib().cugo_graph_get_flat_edges(self._g, 0, None, None, None, None, None, None)
        if n < 0:
            check(n)
        pose = np.zeros(n, np.int32); lm = np.zeros(n, np.int32); fl = np.zeros(n, np.uint8)
        meas = np.zeros((n, 3)); hd = C.c_int(0); w = C.c_double(0.0)
        rc = lib().cugo_graph_get_flat_edges(self._g, n, _p(pose, _i32p), _p(lm, _i32p), _p(fl, _u8p), _p(meas, _f64p),
                                             C.byref(hd), C.byref(w))
        if rc < 0:
            check(rc)
        return dict(pose=pose, lm=lm, flags=fl, meas=meas, has_depth=bool(hd.value), depth_weight=w.value)

    def set_outlier_threshold(self, dim, threshold):
        """edges of the set (dim 2 mono / 3 stereo) with chi2 > threshold are inactivated at the
        end of optimize(); 0 disables (ref: EdgeSet::setOutlierThreshold / updateEdges)"""
        check(lib().cugo_graph_set_outlier_threshold(self._g, dim, C.c_double(threshold)))

    def n_outliers(self, dim):
        return lib().cugo_graph_n_outliers(self._g, dim)

    def edge_active(self, dim, n):
        out = np.zeros(n, np.uint8)
        check(lib().cugo_graph_get_edge_active(self._g, dim, n, _p(out, _u8p)))
        return out.astype(bool)

    def n_pose_edge_outliers(self, kind):
        """outliers found in the set of the kind (POSE_KIND_*) since the last initialize()"""
        n = lib().cugo_graph_n_pose_edge_outliers(self._g, int(kind))
        if n < 0:
            raise CugoError("cugo error %d: %s" % (n, lib().cugo_last_error().decode()))
        return n

    def pose_edge_active(self, kind, n):
        """active flag of the first n edges of the kind (POSE_KIND_*), in insertion order"""
        out = np.zeros(n, np.uint8)
        check(lib().cugo_graph_get_pose_edge_active(self._g, int(kind), int(n), _p(out, _u8p)))
        return out.astype(bool)

    def set_shard(self, rank, world, fn):
        """fn(device_ptr:int, n_doubles:int, op:int) must all-reduce in place"""
        def _cb(ptr, n, op, user):
            fn(ptr, n, op)
        self._cb = EXCHANGE_FN(_cb)
        check(lib().cugo_graph_set_shard(self._g, rank, world, self._cb, None))

    def set_comm(self, comm):
        """native RCCL exchange on the solver's stream (comm: a Comm object)"""
        check(lib().cugo_graph_set_comm(self._g, comm._c))
        self._comm = comm  # keep it alive

    def exchange_stats(self):
        b, c = C.c_double(), C.c_int32()
        check(lib().cugo_graph_exchange_stats(self._g, C.byref(b), C.byref(c)))
        return dict(bytes=b.value, calls=c.value)

    def set_verbose(self, v):
        lib().cugo_graph_set_verbose(self._g, int(v))

    def initialize(self):
        check(lib().cugo_graph_initialize(self._g))

    def set_option(self, name, value):
        """one run-time switch of this optimiser: "flatten_reuse", "structure_reuse", "init_timing" (the CUGO_*
        environment variables are read once, when the optimiser is created), and "pose_edge_outliers" (1: outlier
        thresholds on plane / line / prior / relative-pose sets are taken, GraphOptimisationOptions::
        poseEdgeOutlierRejection; off by default; takes effect at the next initialize())"""
        check(lib().cugo_graph_set_option(self._g, name.encode(), int(value)))

    def flatten_reuses(self):
        """initialize() calls that found the graph unchanged and only refreshed the estimates"""
        return lib().cugo_graph_flatten_reuses(self._g)

    def optimize(self, n):
        check(lib().cugo_graph_optimize(self._g, int(n)))

    def stats(self):
        n = lib().cugo_graph_n_stats(self._g)
        it = np.zeros(max(n, 1), np.int32); chi = np.zeros(max(n, 1))
        lam = np.zeros(max(n, 1)); rho = np.zeros(max(n, 1)); tr = np.zeros(max(n, 1), np.int32)
        n1 = lib().cugo_graph_get_stats(self._g, _p(it, _i32p), _p(chi, _f64p), n)
        lib().cugo_graph_get_trace(self._g, _p(lam, _f64p), _p(rho, _f64p), _p(tr, _i32p), n)
        return [dict(iteration=int(it[i]), chi2=float(chi[i]), lam=float(lam[i]), rho=float(rho[i]),
                     trials=int(tr[i])) for i in range(n1)]

    def poses(self, ids=None):
        ids = self.pose_ids if ids is None else np.ascontiguousarray(ids, np.int32)
        out = np.zeros((len(ids), 7))
        check(lib().cugo_graph_get_poses(self._g, len(ids), _p(ids, _i32p), _p(out, _f64p)))
        return out

    def landmarks(self, ids=None):
        ids = self.lm_ids if ids is None else np.ascontiguousarray(ids, np.int32)
        out = np.zeros((len(ids), 3))
        check(lib().cugo_graph_get_landmarks(self._g, len(ids), _p(ids, _i32p), _p(out, _f64p)))
        return out

    def compute_covariances(self, poses=True, landmarks=True):
        """marginal covariances at the current estimates: Sigma = H^-1 of the undamped J^T Omega J over the free
        vertices (diagonal blocks); kept until the next initialize().  Raises CugoError (code -4) on a zero pivot."""
        what = (1 if poses else 0) | (2 if landmarks else 0)
        if what:
            check(lib().cugo_graph_compute_covariances(self._g, what))

    def pose_covariances(self, ids=None):
        """[n, 6, 6] per pose id (tangent order [rotation, translation], left update); zeros for fixed poses"""
        ids = self.pose_ids if ids is None else np.ascontiguousarray(ids, np.int32)
        out = np.zeros((len(ids), 36))
        check(lib().cugo_graph_get_pose_covariances(self._g, len(ids), _p(ids, _i32p), _p(out, _f64p)))
        return out.reshape(-1, 6, 6).transpose(0, 2, 1).copy()  # (column-major blocks)

    def landmark_covariances(self, ids=None):
        """[n, 3, 3] per landmark id; zeros for fixed landmarks"""
        ids = self.lm_ids if ids is None else np.ascontiguousarray(ids, np.int32)
        out = np.zeros((len(ids), 9))
        check(lib().cugo_graph_get_landmark_covariances(self._g, len(ids), _p(ids, _i32p), _p(out, _f64p)))
        return out.reshape(-1, 3, 3).transpose(0, 2, 1).copy()

    def _pair_blocks(self, fn, ids_a, ids_b):
        a = np.ascontiguousarray(ids_a, np.int32).reshape(-1)
        b = np.ascontiguousarray(ids_b, np.int32).reshape(-1)
        if len(a) != len(b):
            raise ValueError("ids_a and ids_b must have the same length")
        out = np.zeros((len(a), 36))
        check(fn(self._g, len(a), _p(a, _i32p), _p(b, _i32p), _p(out, _f64p)))
        return out.reshape(-1, 6, 6).transpose(0, 2, 1).copy()  # (column-major blocks)

    def pose_cross_covariances(self, ids_a, ids_b):
        """[n, 6, 6]: Sigma_ab of the pose pairs (ids_a[k], ids_b[k]) at the current estimates — any pairs, inside the
        Hsc pattern or not (rows a, columns b; tangent order as pose_covariances(); a == b gives the diagonal block,
        zeros when either pose is fixed).  Does not touch what compute_covariances() stored.  Raises CugoError (code
        -4) on a zero pivot."""
        return self._pair_blocks(lib().cugo_graph_compute_pose_cross_covariances, ids_a, ids_b)

    def relative_pose_covariances(self, ids_a, ids_b):
        """[n, 6, 6]: covariance of the relative pose T_a T_b^-1 in the tangent convention of the relative-pose edges;
        its inverse is the information of an edge that summarises the graph between a and b.  a == b is refused."""
        return self._pair_blocks(lib().cugo_graph_relative_pose_covariances, ids_a, ids_b)

    def pose_landmark_cross_covariances(self, pose_ids, lm_ids):
        """[n, 6, 3]: Sigma_al of the pairs (pose_ids[k], lm_ids[k]) at the current estimates — any pairs, with or
        without an edge (rows in the tangent order of pose_covariances(); zeros where either vertex is fixed).  With
        pose_covariances() and landmark_covariances() it completes the joint covariance of a camera and a map point.
        Does not touch what compute_covariances() stored.  Raises CugoError (code -4) on a zero pivot or when a
        queried landmark has no active edge."""
        a = np.ascontiguousarray(pose_ids, np.int32).reshape(-1)
        b = np.ascontiguousarray(lm_ids, np.int32).reshape(-1)
        if len(a) != len(b):
            raise ValueError("pose_ids and lm_ids must have the same length")
        out = np.zeros((len(a), 18))
        check(lib().cugo_graph_compute_pose_landmark_cross_covariances(self._g, len(a), _p(a, _i32p), _p(b, _i32p),
                                                                       _p(out, _f64p)))
        return out.reshape(-1, 3, 6).transpose(0, 2, 1).copy()  # (column-major blocks)

    def reprojection_covariances(self, pose_ids, lm_ids, dim=2, cam=None):
        """[n, dim, dim]: covariance S = J Sigma J^T of the predicted reprojection of landmark lm_ids[k] in pose
        pose_ids[k] over their joint covariance (dim 2: u, v; dim 3: u, v, u_right).  cam: [5] or [n, 5] (fx, fy, cx,
        cy, bf); None: the camera given to set_camera(dim, ...).  A fixed vertex contributes no terms."""
        a = np.ascontiguousarray(pose_ids, np.int32).reshape(-1)
        b = np.ascontiguousarray(lm_ids, np.int32).reshape(-1)
        if len(a) != len(b):
            raise ValueError("pose_ids and lm_ids must have the same length")
        c = None if cam is None else np.ascontiguousarray(
            np.broadcast_to(np.asarray(cam, np.float64).reshape(-1, 5), (len(a), 5)))
        dd = int(dim) * int(dim) if dim in (2, 3) else 9
        out = np.zeros((len(a), dd))
        check(lib().cugo_graph_reprojection_covariances(self._g, len(a), _p(a, _i32p), _p(b, _i32p), int(dim),
                                                        None if c is None else _p(c, _f64p), _p(out, _f64p)))
        return out.reshape(-1, int(dim), int(dim)).transpose(0, 2, 1).copy()

    def predict_observations(self, pose_ids, lm_ids, kind=OBS_MONO, cam=None, sensor=None, model=None):
        """(z [n, dim], cov [n, dim, dim]): the predicted observation of landmark lm_ids[k] seen from pose pose_ids[k] and
        its covariance S = J Sigma J^T, for every camera kind.  kind: OBS_MONO (u, v), OBS_STEREO (u, v, u_right),
        OBS_DEPTH (u, v, 1/Z_s; S in measurement units, the set's inverse-depth weight not applied).  cam: [5] or [n, 5]
        (fx, fy, cx, cy, bf); sensor: [7] or [n, 7] (q, t) body -> sensor, None: the identity; model: [5] or [n, 5]
        (k1, k2, k3, k4, type), type 0 pinhole / 1 Kannala-Brandt, None: a pinhole.  cam=None: the camera, sensor pose
        and model of the graph's mono / stereo / depth set for that kind (sensor and model must then be None; refused
        when that set has a lens distortion, which these predictions do not model yet)."""
        a = np.ascontiguousarray(pose_ids, np.int32).reshape(-1)
        b = np.ascontiguousarray(lm_ids, np.int32).reshape(-1)
        if len(a) != len(b):
            raise ValueError("pose_ids and lm_ids must have the same length")
        n = len(a)

        def per_query(v, w):
            return None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float64).reshape(-1, w), (n, w)))
        c, s, m = per_query(cam, 5), per_query(sensor, 7), per_query(model, 5)
        dim = 2 if kind == OBS_MONO else 3
        z, out = np.zeros((n, dim)), np.zeros((n, dim * dim))
        check(lib().cugo_graph_predict_observations(self._g, n, _p(a, _i32p), _p(b, _i32p), int(kind),
                                                    None if c is None else _p(c, _f64p), None if s is None else _p(s, _f64p),
                                                    None if m is None else _p(m, _f64p), _p(z, _f64p), _p(out, _f64p)))
        return z, out.reshape(-1, dim, dim).transpose(0, 2, 1).copy()

    def set_poses(self, ids, q_t7):
        ids = np.ascontiguousarray(ids, np.int32); q = np.ascontiguousarray(q_t7, np.float64)
        check(lib().cugo_graph_set_poses(self._g, len(ids), _p(ids, _i32p), _p(q, _f64p)))

    def set_landmarks(self, ids, xyz):
        ids = np.ascontiguousarray(ids, np.int32); x = np.ascontiguousarray(xyz, np.float64)
        check(lib().cugo_graph_set_landmarks(self._g, len(ids), _p(ids, _i32p), _p(x, _f64p)))

    def n_active_edges(self):
        return lib().cugo_graph_n_active_edges(self._g)

    def time_profile(self):
        buf = C.create_string_buffer(2048); ms = np.zeros(16)
        n = lib().cugo_graph_time_profile(self._g, buf, 2048, _p(ms, _f64p), 16)
        names = buf.value.decode().split("\n")[:n]
        return dict(zip(names, ms[:n].tolist()))

    def set_float32(self, on):
        """fp32-internal mode: float storage of the Hpl / T block streams (next initialize())"""
        check(lib().cugo_graph_set_float32(self._g, int(on)))

    def set_kernel_timing(self, on):
        """1: event pairs per kernel group and per kernel; 2: one event per group boundary (sums exactly); 0: off"""
        lib().cugo_graph_set_kernel_timing(self._g, int(on))

    def kernel_times(self):
        buf = C.create_string_buffer(8192); ms = np.zeros(96); cnt = np.zeros(96, np.int32)
        n = lib().cugo_graph_kernel_times(self._g, buf, 8192, _p(ms, _f64p), _p(cnt, _i32p), 96)
        names = buf.value.decode().split("\n")[:n]
        return {names[i]: dict(ms=float(ms[i]), launches=int(cnt[i])) for i in range(n)}

    def structure_stats(self):
        o = np.zeros(24)
        n = lib().cugo_graph_structure_stats(self._g, _p(o, _f64p), 24)
        keys = ["hsc_blocks", "products", "nnzL", "chol_flops", "supernodes", "stages", "front_bytes",
                "offdiag_products", "up_potrf_flops", "up_trsm_flops", "up_syrk_flops", "up_ea_bytes",
                "backward_bytes", "schur_slots", "chol_rank_flops", "chol_top_flops", "chol_bcast_bytes",
                "chol_bcasts", "trial_sync_retries", "xchg_sys_bytes", "xchg_sys_full_bytes"]
        return dict(zip(keys[:n], o[:n].tolist()))


def graph_from_arrays(d, per_edge_information=True, per_edge_camera=True, rk=(RK_NONE, 1.0),
                      pose_ids=None, lm_ids=None, plan_only=False):
    """Build a Graph from the flat-array problem dict used by tests/oracle.Problem
    (positions are used as ids unless ids are given)."""
    g = Graph(per_edge_information, per_edge_camera, plan_only)
    P, L = len(d["pose"]), len(d["lm"])
    pid = np.arange(P, dtype=np.int32) if pose_ids is None else np.asarray(pose_ids, np.int32)
    lid = np.arange(L, dtype=np.int32) if lm_ids is None else np.asarray(lm_ids, np.int32)
    g.add_poses(pid, d["pose"], d["pose_fixed"])
    g.add_landmarks(lid, d["lm"], d["lm_fixed"])
    st = np.asarray(d["e_stereo"]).astype(bool)
    ep, el = np.asarray(d["e_pose"]), np.asarray(d["e_lm"])
    meas, om = np.asarray(d["e_meas"], np.float64), np.asarray(d["e_omega"], np.float64)
    cam = np.asarray(d["e_cam"], np.float64).reshape(-1, 5)
    if len(cam) == 1:
        cam = np.tile(cam, (len(ep), 1))
    for dim, sel in ((2, ~st), (3, st)):
        if not per_edge_camera and sel.any():
            g.set_camera(dim, cam[sel][0])
        if not per_edge_information and sel.any():
            g.set_information(dim, float(om[sel][0]))
        g.add_edges(dim, pid[ep[sel]], lid[el[sel]], meas[sel], om[sel],
                    cam[sel] if per_edge_camera else None)
        g.set_robust_kernel(dim, rk[0], rk[1])
    return g


# ---- reference graph-file format (ref: samples/sample_ba_from_file/main.cpp:89-160) ---------
def save_ba_json(path, d, pose_ids=None, lm_ids=None):
    """write a flat-array problem in the JSON layout of the reference's ba_kitti_*.json"""
    import json
    P, L = len(d["pose"]), len(d["lm"])
    pid = np.arange(P) if pose_ids is None else np.asarray(pose_ids)
    lid = np.arange(L) if lm_ids is None else np.asarray(lm_ids)
    cam = np.asarray(d["e_cam"], np.float64).reshape(-1, 5)[0]
    out = {"fx": cam[0], "fy": cam[1], "cx": cam[2], "cy": cam[3], "bf": cam[4],
           "pose_vertices": [{"id": int(pid[i]), "fixed": int(d["pose_fixed"][i]),
                              "q": [float(x) for x in d["pose"][i][:4]],
                              "t": [float(x) for x in d["pose"][i][4:]]} for i in range(P)],
           "landmark_vertices": [{"id": int(lid[i]), "fixed": int(d["lm_fixed"][i]),
                                  "Xw": [float(x) for x in d["lm"][i]]} for i in range(L)],
           "monocular_edges": [], "stereo_edges": []}
    for e in range(len(d["e_pose"])):
        st = bool(d["e_stereo"][e])
        out["stereo_edges" if st else "monocular_edges"].append(
            {"vertexP": int(pid[d["e_pose"][e]]), "vertexL": int(lid[d["e_lm"][e]]),
             "measurement": [float(x) for x in d["e_meas"][e][:3 if st else 2]],
             "information": float(d["e_omega"][e])})
    with open(path, "w") as f:
        json.dump(out, f)


def load_ba_json(path):
    """read ba_kitti_*.json (reference sample format) into the flat-array dict + id arrays"""
    import json
    j = json.load(open(path))
    pv, lv = j["pose_vertices"], j["landmark_vertices"]
    pose_ids = np.array([v["id"] for v in pv], np.int32)
    lm_ids = np.array([v["id"] for v in lv], np.int32)
    ppos = {int(i): k for k, i in enumerate(pose_ids)}
    lpos = {int(i): k for k, i in enumerate(lm_ids)}
    cam = np.array([j["fx"], j["fy"], j["cx"], j["cy"], j["bf"]], np.float64)
    ep, el, st, meas, om = [], [], [], [], []
    for key, stereo in (("monocular_edges", 0), ("stereo_edges", 1)):
        for e in j.get(key, []):
            ep.append(ppos[e["vertexP"]]); el.append(lpos[e["vertexL"]]); st.append(stereo)
            m = list(e["measurement"]) + [0.0] * (3 - len(e["measurement"]))
            meas.append(m); om.append(e["information"])
    d = dict(pose=np.array([v["q"] + v["t"] for v in pv], np.float64).reshape(-1, 7),
             pose_fixed=np.array([v["fixed"] for v in pv], np.uint8),
             lm=np.array([v["Xw"] for v in lv], np.float64).reshape(-1, 3),
             lm_fixed=np.array([v["fixed"] for v in lv], np.uint8),
             e_pose=np.array(ep, np.int32), e_lm=np.array(el, np.int32), e_stereo=np.array(st, np.uint8),
             e_meas=np.array(meas, np.float64).reshape(-1, 3), e_omega=np.array(om, np.float64),
             e_cam=np.tile(cam, (len(ep), 1)))
    return d, pose_ids, lm_ids
