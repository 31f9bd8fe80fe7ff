"""Reference for graphs whose BA edges carry camera models (Kannala-Brandt fisheye): rig_lm_ref's dense numpy LM with
the edge seen through a sensor pose AND a projection model per edge, float64, numpy only.  The fisheye edge is written
here by the chain rule in the plain quotient form, on its own (tests/fisheye_ref.py is the kernels' reference; no
point of these scenes is near the optical axis):
    Xs = M Xb + t_s,  r = |(x, y)|,  th = atan2(r, z),  thd = th (1 + k1 th^2 + ... + k4 th^8),  proj = f thd (x, y) / r + c
    dproj/dXs from  d(thd / r)/dXs = (D dth/dXs - (thd / r) dr/dXs) / r,   D = 1 + 3 k1 th^2 + ... + 9 k4 th^8
Also the input recipe of tests/test_fisheye_graph.py: the ring scene — a body inside a ring of landmarks with four
fisheye cameras at 0 / 90 / 180 / 270 degrees of yaw, each of which sees landmarks beyond 90 degrees off its axis."""
import numpy as np

import relpose_lm_ref as RL
import rig_lm_ref as G
import rig_ref
from rig_lm_ref import MG


def fisheye_edge(pose, Xw, meas, cam, ext12, k):
    fx, fy, cx, cy, _ = cam
    M, ts = ext12[:9].reshape(3, 3), ext12[9:]
    R = MG.quat_to_R(pose[:4])
    Xb = R @ Xw + pose[4:]
    x, y, z = M @ Xb + ts
    r = np.hypot(x, y)
    R2 = r * r + z * z
    th = np.arctan2(r, z)
    thd = th * (1 + k[0] * th**2 + k[1] * th**4 + k[2] * th**6 + k[3] * th**8)
    D = 1 + 3 * k[0] * th**2 + 5 * k[1] * th**4 + 7 * k[2] * th**6 + 9 * k[3] * th**8
    rho = thd / r
    e = np.array([fx * rho * x + cx, fy * rho * y + cy]) - meas[:2]
    dth = np.array([x * z / (r * R2), y * z / (r * R2), -r / R2])
    dr = np.array([x / r, y / r, 0.0])
    drho = (D * dth - rho * dr) / r
    dp = np.array([fx * (rho * np.array([1.0, 0, 0]) + x * drho), fy * (rho * np.array([0, 1.0, 0]) + y * drho)])
    skew = np.array([[0, -Xb[2], Xb[1]], [Xb[2], 0, -Xb[0]], [-Xb[1], Xb[0], 0]])
    return e, Xb, -dp @ M @ np.hstack([-skew, np.eye(3)]), -dp @ M @ R


class FisheyeBA(G.RigBA):
    """rig_lm_ref.RigBA with d["e_model"] [E][5] = (k1, k2, k3, k4, type): type 1 edges are Kannala-Brandt mono edges"""

    def __init__(self, d, rk=(0, 1.0)):
        super().__init__(d, rk)
        self.model = np.asarray(d["e_model"], np.float64)
        assert not np.any(self.st & (self.model[:, 4] != 0))

    def _edge(self, i):
        if self.model[i, 4] != 0:
            return fisheye_edge(self.pose[self.ep[i]], self.lm[self.el[i]], self.meas[i], self.cam[i], self.ext[i], self.model[i, :4])
        return super()._edge(i)


class FisheyeGraph(FisheyeBA):
    def __init__(self, d, via_schur=True):
        super().__init__(d)
        self.via_schur = via_schur

    def solve(self, H, b, lam, via_schur=True):
        return super().solve(H, b, lam, via_schur=self.via_schur)


class FisheyeRelPoseGraph(RL.RelPoseGraph, FisheyeBA):
    """pose priors and relative-pose edges (on the pose vertex: the body) next to fisheye rig edges"""


def permute_edges(d, seed=91):
    perm = np.random.default_rng(seed).permutation(len(d["e_pose"]))
    out = dict(d)
    for key in ("e_pose", "e_lm", "e_stereo", "e_meas", "e_omega", "e_cam", "e_sensor", "e_model", "e_camera"):
        out[key] = np.asarray(d[key])[perm]
    return out


def reference_runs(d, niter, make=None):
    """rig_lm_ref.reference_runs with this module's graph and permutation"""
    make = make or (lambda dd, vs: FisheyeGraph(dd, via_schur=vs))
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


RING_LEVERS = ((0.0, 0.0, 0.3), (0.4, 0.05, 0.0), (0.0, -0.1, -0.5), (-0.35, 0.1, 0.1))
RING_K = (np.array([-0.0131, 0.0212, -0.0071, 0.0012]), np.zeros(4), np.array([0.0342, -0.0094, 0.0038, -0.0009]),
          np.array([-0.0065, 0.0106, -0.0035, 0.0006]))
RING_CAMS = np.array([400.0, 410.0, 320.0, 240.0, 0.0])[None, :] * np.array([1.0, 1.01, 0.99, 1.02])[:, None]


def ring_problem(seed=7, n_poses=5, nl=32, wide=110.0, pix_noise=0.5, pose_noise=(0.02, 0.1), lm_noise=0.15):
    """nl landmarks on a ring of 6 m (heights within +-1 m) round a body that moves a few decimetres and turns a few
    degrees between n_poses poses (pose 0 fixed); the cameras within `wide` degrees of a landmark see it from the poses
    in turn (a pose sees a landmark once), so every camera has edges beyond 90 degrees off its axis.  The dict of
    rig_lm_ref.make_rig_problem plus e_model [E][5]"""
    rng = np.random.default_rng(seed)
    sensors = np.stack([G.yaw_pose(90.0 * k, c) for k, c in enumerate(RING_LEVERS)])
    ext = np.stack([rig_ref.quat_to_ext(q) for q in sensors])
    ang = 2 * np.pi * (np.arange(nl) + 0.5) / nl
    lm_gt = np.stack([6 * np.sin(ang), np.linspace(-1, 1, nl) * np.cos(3 * ang), 6 * np.cos(ang)], 1)
    pose_gt = np.zeros((n_poses, 7))
    pose_gt[:, 3] = 1.0
    for i in range(1, n_poses):
        q = MG_quat(rng.normal(0, 0.08, 3))
        pose_gt[i, :4], pose_gt[i, 4:] = q, rng.normal(0, 0.25, 3)
    e_pose, e_lm, e_c, e_meas, e_om = [], [], [], [], []
    beyond = np.zeros(4, int)
    for l in range(nl):
        off = [np.rad2deg(abs((ang[l] - k * np.pi / 2 + np.pi) % (2 * np.pi) - np.pi)) for k in range(4)]
        sees = [k for k in range(4) if off[k] < wide]
        for p in range(n_poses):
            c = sees[(l + p) % len(sees)]
            zero = np.zeros(3)
            proj = fisheye_edge(pose_gt[p], lm_gt[l], zero, RING_CAMS[c], ext[c], RING_K[c])[0]
            xs = ext[c, :9].reshape(3, 3) @ (MG.quat_to_R(pose_gt[p, :4]) @ lm_gt[l] + pose_gt[p, 4:]) + ext[c, 9:]
            beyond[c] += xs[2] < 0
            e_pose.append(p), e_lm.append(l), e_c.append(c)
            e_meas.append([proj[0] + rng.normal(0, pix_noise), proj[1] + rng.normal(0, pix_noise), 0.0])
            e_om.append(1.0 / (1.2 ** int(rng.integers(0, 8))) ** 2)
    assert beyond.min() >= 3, "a camera sees nothing beyond 90 degrees off its axis"
    pose = pose_gt.copy()
    for i in range(1, n_poses):
        q = quat_mul(MG_quat(rng.normal(0, pose_noise[0], 3)), pose[i, :4])
        pose[i, :4] = q / np.linalg.norm(q) * (1 if q[3] >= 0 else -1)
        pose[i, 4:] += rng.normal(0, pose_noise[1], 3)
    lm = lm_gt + rng.normal(0, lm_noise, lm_gt.shape)
    pf = np.zeros(n_poses, np.uint8)
    pf[0] = 1
    e_c = np.array(e_c)
    E = len(e_c)
    return dict(pose=pose, pose_fixed=pf, lm=lm, lm_fixed=np.zeros(nl, np.uint8), e_pose=np.array(e_pose, np.int32),
                e_lm=np.array(e_lm, np.int32), e_stereo=np.zeros(E, np.uint8), e_meas=np.array(e_meas), e_omega=np.array(e_om),
                e_cam=RING_CAMS[e_c], pose_gt=pose_gt, lm_gt=lm_gt, e_sensor=sensors[e_c], e_camera=e_c, sensors=sensors,
                e_model=np.stack([np.concatenate([RING_K[c], [1.0]]) for c in e_c]))


def MG_quat(rotvec):
    a = np.linalg.norm(rotvec)
    if a == 0:
        return np.array([0.0, 0, 0, 1])
    return np.concatenate([np.sin(a / 2) * rotvec / a, [np.cos(a / 2)]])


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])
