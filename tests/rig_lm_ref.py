"""Reference for graphs whose BA edges carry camera extrinsics (a rig): the dense numpy LM of tests/golden/make_golden.py
(Graph) with the edge seen through a sensor pose, float64, numpy only — and, stacked under tests/relpose_lm_ref.RelPoseGraph,
next to body-frame pose priors and relative-pose edges.  The pose is world -> body; a sensor pose (q, t) is body -> sensor:
    Xb = R(q_b) Xw + t_b,   Xs = M Xb + t_s,   e = proj(Xs) - meas,
    J_pose = -(dproj/dXs) M [-[Xb]x, I]   (left update on the body, order [w, v]),   J_lm = -(dproj/dXs) M R(q_b)
written here by the chain rule, not taken from tests/rig_ref.py (test_rig_ref_host.py holds the two against each other).
Also the input recipes of tests/test_rig_graph.py: rig problems with their own trajectory and landmarks in view of the
camera that sees them."""
import os
import sys

import numpy as np

import relpose_lm_ref as RL
import rig_ref
import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden as MG  # noqa: E402


def rig_edge(pose, Xw, meas, stereo, cam, ext12):
    fx, fy, cx, cy, bf = cam
    M, ts = ext12[:9].reshape(3, 3), ext12[9:]
    R = MG.quat_to_R(pose[:4])
    Xb = R @ Xw + pose[4:]
    X, Y, Z = M @ Xb + ts
    proj = np.array([fx * X / Z + cx, fy * Y / Z + cy, fx * X / Z + cx - bf / Z])
    dim = 3 if stereo else 2
    e = proj[:dim] - meas[:dim]
    dp = np.array([[fx / Z, 0, -fx * X / Z**2], [0, fy / Z, -fy * Y / Z**2], [fx / Z, 0, -fx * X / Z**2 + bf / Z**2]])[:dim]
    skew = np.array([[0, -Xb[2], Xb[1]], [Xb[2], 0, -Xb[0]], [-Xb[1], Xb[0], 0]])
    return e, Xb, -dp @ M @ np.hstack([-skew, np.eye(3)]), -dp @ M @ R


class RigBA(MG.Graph):
    """make_golden.Graph whose edges go through d["e_sensor"] [E][7] (normalised and expanded as the host does), with a
    robust kernel per kind d["rk2"] = {0: mono, 1: stereo} and a mask `live` (outlier rejection)"""

    def __init__(self, d, rk=(0, 1.0)):
        super().__init__(d, rk)
        self.ext = np.stack([rig_ref.quat_to_ext(q) for q in np.asarray(d["e_sensor"], np.float64)])
        self.rk2 = d.get("rk2", {0: rk, 1: rk})
        self.live = np.ones(len(self.ep), bool)

    def _edge(self, i):
        return rig_edge(self.pose[self.ep[i]], self.lm[self.el[i]], self.meas[i], self.st[i], self.cam[i], self.ext[i])

    def edge_chi(self):
        out = np.zeros(len(self.ep))
        for i in np.nonzero(self.active & self.live)[0]:
            e = self._edge(i)[0]
            rk = self.rk2[int(self.st[i])]
            out[i] = MG.rho(rk[0], rk[1], self.om[i] * (e @ e))
        return out

    def chi2(self):
        return float(self.edge_chi().sum())

    def normal_equations(self):
        n = 6 * self.np_ + 3 * self.nl
        H = np.zeros((n, n))
        b = np.zeros(n)
        for i in np.nonzero(self.active & self.live)[0]:
            ip, il = self.ep[i], self.el[i]
            e, _, JP, JL = self._edge(i)
            rk = self.rk2[int(self.st[i])]
            w = self.om[i] * MG.drho(rk[0], rk[1], self.om[i] * (e @ e))
            cols, J = [], []
            if not self.pf[ip]:
                cols.append(np.arange(6) + 6 * self.pidx[ip]); J.append(JP)
            if not self.lf[il]:
                cols.append(np.arange(3) + 6 * self.np_ + 3 * self.lidx[il]); J.append(JL)
            c, J = np.concatenate(cols), np.hstack(J)
            H[np.ix_(c, c)] += w * J.T @ J
            b[c] += w * J.T @ e
        return H, b


class RigGraph(RigBA):
    def __init__(self, d, via_schur=True):
        super().__init__(d)
        self.via_schur = via_schur

    def solve(self, H, b, lam, via_schur=True):
        return super().solve(H, b, lam, via_schur=self.via_schur)


class RigRelPoseGraph(RL.RelPoseGraph, RigBA):
    """pose priors and relative-pose edges (on the pose vertex: the body) next to rig BA edges"""


def permute_edges(d, seed=91):
    perm = np.random.default_rng(seed).permutation(len(d["e_pose"]))
    out = dict(d)
    for key in ("e_pose", "e_lm", "e_stereo", "e_meas", "e_omega", "e_cam", "e_sensor"):
        out[key] = np.asarray(d[key])[perm]
    return out


def reference_runs(d, niter, make=None):
    """the trajectory, the final estimates and what the reference differs by from itself (Schur against dense solve, the
    edges permuted); make(d, via_schur) -> graph"""
    make = make or (lambda dd, vs: RigGraph(dd, via_schur=vs))
    runs = []
    for dd, vs in ((d, True), (d, False), (permute_edges(d), True)):
        g = make(dd, vs)
        runs.append((g.optimize(niter), g.pose.copy(), g.lm.copy()))
    tr = runs[0][0]
    sens, est = [0.0] * len(tr), 0.0
    for t2, pose2, lm2 in runs[1:]:
        assert [t[4] for t in t2] == [t[4] for t in tr], "the reference disagrees with itself on the trial counts"
        for i in range(len(tr)):
            sens[i] = max(sens[i], abs(tr[i][1] - t2[i][1]) / abs(tr[i][1]))
        est = max(est, float(np.abs(runs[0][1] - pose2).max()), float(np.abs(runs[0][2] - lm2).max()))
    return RL.icp_lm_ref.trace_dicts(tr), runs[0][1], runs[0][2], sens, est


def yaw_pose(deg, t):
    """sensor pose: the camera looks along the body direction `deg` of yaw (about the body's y axis) from the body
    point c = t:  Xs = Ry(-deg) (Xb - c)"""
    h = np.deg2rad(-deg) / 2
    q = np.array([0.0, np.sin(h), 0.0, np.cos(h)])
    M = rig_ref.quat_to_ext(np.concatenate([q, [0, 0, 0]]))[:9].reshape(3, 3)
    return np.concatenate([q, -M @ np.asarray(t, np.float64)])


def make_rig_problem(sensors, stereo_of, n_poses=8, n_landmarks=60, seed=0, yaw_step=0.03, pix_noise=1.0,
                     pose_noise=(0.01, 0.05), lm_noise=0.02, depth=(6.0, 40.0), cams=None):
    """a rig moving along its body z axis with a yaw of ~yaw_step rad per pose; landmark l is seen by camera
    l % len(sensors) from a window of consecutive poses, placed in that camera's view; stereo_of[c]: camera c's edges are
    stereo edges.  Returns the dict of synth.make_problem (body poses) plus e_sensor [E][7], e_camera [E] (the index
    into sensors), sensors"""
    rng = np.random.default_rng(seed)
    sensors = np.asarray(sensors, np.float64)
    ext = np.stack([rig_ref.quat_to_ext(q) for q in sensors])
    cams = np.tile(synth.KITTI_CAM, (len(sensors), 1)) if cams is None else np.asarray(cams, np.float64)
    Rwb, twb, yaw, pos = [], [], 0.0, np.zeros(3)
    for i in range(n_poses):
        yaw += yaw_step + rng.normal(0, 0.005)
        R = synth.quat_to_R(synth.quat_from_rotvec(np.array([rng.normal(0, 0.002), yaw, rng.normal(0, 0.002)])))
        Rwb.append(R), twb.append(pos.copy())
        pos = pos + R @ np.array([0, 0, 1.0 + rng.normal(0, 0.05)])
    pose_gt = np.zeros((n_poses, 7))
    for i in range(n_poses):
        pose_gt[i, :4] = synth._R_to_quat(Rwb[i].T)
        pose_gt[i, 4:] = -Rwb[i].T @ twb[i]
    lm_gt = np.zeros((n_landmarks, 3))
    e_pose, e_lm, e_st, e_meas, e_om, e_c = [], [], [], [], [], []
    for l in range(n_landmarks):
        c = l % len(sensors)
        M, ts, cam = ext[c, :9].reshape(3, 3), ext[c, 9:], cams[c]
        first = int(rng.integers(0, n_poses - 2))
        obs = list(range(first, min(n_poses, first + int(rng.integers(3, 6)))))
        mid = obs[len(obs) // 2]
        z = rng.uniform(*depth)
        u, v = rng.uniform(300, 900), rng.uniform(60, 310)
        Xs = np.array([(u - cam[2]) / cam[0] * z, (v - cam[3]) / cam[1] * z, z])
        lm_gt[l] = Rwb[mid] @ (M.T @ (Xs - ts)) + twb[mid]
        for p in obs:
            xs = M @ (synth.quat_to_R(pose_gt[p, :4]) @ lm_gt[l] + pose_gt[p, 4:]) + ts
            if xs[2] < 0.3 * z:
                continue
            uu = cam[0] * xs[0] / xs[2] + cam[2] + rng.normal(0, pix_noise)
            vv = cam[1] * xs[1] / xs[2] + cam[3] + rng.normal(0, pix_noise)
            ur = uu - cam[4] / xs[2] + rng.normal(0, pix_noise)
            e_pose.append(p), e_lm.append(l), e_st.append(1 if stereo_of[c] else 0), e_c.append(c)
            e_meas.append([uu, vv, ur if stereo_of[c] else 0.0])
            e_om.append(1.0 / (1.2 ** int(rng.integers(0, 8))) ** 2)
    pose = pose_gt.copy()
    for i in range(1, n_poses):
        q = synth.quat_mul(synth.quat_from_rotvec(rng.normal(0, pose_noise[0], 3)), pose[i, :4])
        pose[i, :4] = q / np.linalg.norm(q) * (1 if q[3] >= 0 else -1)
        pose[i, 4:] += rng.normal(0, pose_noise[1], 3)
    lm = lm_gt + rng.normal(0, 1, lm_gt.shape) * lm_noise * np.linalg.norm(lm_gt - np.array(twb).mean(0), axis=1, keepdims=True) * 0.1
    pf = np.zeros(n_poses, np.uint8)
    pf[0] = 1
    e_c = np.array(e_c)
    assert len(set(zip(e_pose, e_lm))) == len(e_pose) and np.bincount(e_lm, minlength=n_landmarks).min() >= 2
    return dict(pose=pose, pose_fixed=pf, lm=lm, lm_fixed=np.zeros(n_landmarks, np.uint8),
                e_pose=np.array(e_pose, np.int32), e_lm=np.array(e_lm, np.int32), e_stereo=np.array(e_st, np.uint8),
                e_meas=np.array(e_meas), e_omega=np.array(e_om), e_cam=cams[e_c], pose_gt=pose_gt, lm_gt=lm_gt,
                e_sensor=sensors[e_c], e_camera=e_c, sensors=sensors)


# a two-camera mono rig, forward and 90 degrees of yaw, 0.4 m apart, and a stereo camera on a third entry
RIG3 = (yaw_pose(0.0, (0.2, 0.0, 0.0)), yaw_pose(90.0, (-0.2, 0.0, 0.0)),
        np.concatenate([np.array([0.03, -0.05, 0.02, 1.0]) / np.linalg.norm([0.03, -0.05, 0.02, 1.0]), [0.0, -0.3, 0.1]]))
# the scale case: forward and backward cameras 1.4 m apart on a body that yaws 0.25 rad per pose
RIG_SCALE = (yaw_pose(0.0, (0.5, 0.0, 0.5)), yaw_pose(180.0, (-0.5, 0.0, -0.5)))
SCALE_ITERS = 11


def scaled_about_fixed_pose(d, factor):
    """the start of d with every body centre and every landmark scaled by `factor` about the centre of the fixed pose 0"""
    out = dict(d)
    pose, lm = d["pose"].copy(), d["lm"].copy()
    c0 = -MG.quat_to_R(pose[0, :4]).T @ pose[0, 4:]
    for i in range(1, len(pose)):
        Ri = MG.quat_to_R(pose[i, :4])
        pose[i, 4:] = -Ri @ (c0 + factor * (-Ri.T @ pose[i, 4:] - c0))
    out["pose"], out["lm"] = pose, c0 + factor * (lm - c0)
    return out


def scale_of(d, lm):
    c0 = -MG.quat_to_R(d["pose_gt"][0, :4]).T @ d["pose_gt"][0, 4:]
    return float(np.median(np.linalg.norm(lm - c0, axis=1) / np.linalg.norm(d["lm_gt"] - c0, axis=1)))


def scale_problem(sensors):
    return scaled_about_fixed_pose(make_rig_problem(sensors, (0, 0), seed=33, yaw_step=0.25, pix_noise=0.0,
                                                      pose_noise=(0.0, 0.0), lm_noise=0.0, depth=(3.0, 8.0)), 1.2)
