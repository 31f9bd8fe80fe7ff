"""Reference for graphs whose BA edges carry a radial-tangential lens distortion: rig_lm_ref's dense numpy LM with the
edge seen through a sensor pose AND a distortion per edge, float64, numpy only.  The distorted edge is written here by
the chain rule through (a, b) = (x, y) / z, on its own (tests/distort_ref.py is the kernels' reference):
    Xs = M Xb + t_s,  a = x / z,  b = y / z,  r2 = a^2 + b^2,  rad = 1 + k1 r2 + k2 r2^2 + k3 r2^3
    a' = a rad + 2 p1 a b + p2 (r2 + 2 a^2),  b' = b rad + p1 (r2 + 2 b^2) + 2 p2 a b,  proj = (fx a' + cx, fy b' + cy)
    dproj/dXs = diag(fx, fy) [d(a', b')/d(a, b)] [d(a, b)/dXs],   d(a, b)/dXs = [[1, 0, -a], [0, 1, -b]] / z
Also the input recipe of tests/test_distort_graph.py: a two-camera rig, camera 0 distorted with all five coefficients,
camera 1 undistorted."""
import numpy as np

import relpose_lm_ref as RL
import rig_lm_ref as G
from rig_lm_ref import MG

DIST = np.array([-0.28, 0.07, 0.002, -0.001, -0.01])


def distort(a, b, d):
    """(a', b') and the 2 x 2 matrix d(a', b')/d(a, b)"""
    k1, k2, p1, p2, k3 = d
    r2 = a * a + b * b
    rad = 1 + k1 * r2 + k2 * r2**2 + k3 * r2**3
    drad = k1 + 2 * k2 * r2 + 3 * k3 * r2**2                   # d rad / d r2; d r2 / da = 2 a, d r2 / db = 2 b
    ad = a * rad + 2 * p1 * a * b + p2 * (r2 + 2 * a * a)
    bd = b * rad + p1 * (r2 + 2 * b * b) + 2 * p2 * a * b
    J = np.array([[rad + a * drad * 2 * a + 2 * p1 * b + p2 * (2 * a + 4 * a), a * drad * 2 * b + 2 * p1 * a + p2 * 2 * b],
                  [b * drad * 2 * a + p1 * 2 * a + 2 * p2 * b, rad + b * drad * 2 * b + p1 * (2 * b + 4 * b) + 2 * p2 * a]])
    return ad, bd, J


def distorted_edge(pose, Xw, meas, cam, ext12, d):
    fx, fy, cx, cy, _ = cam
    M, ts = ext12[:9].reshape(3, 3), ext12[9:]
    R = MG.quat_to_R(pose[:4])
    Xb = R @ Xw + pose[4:]
    x, y, z = M @ Xb + ts
    a, b = x / z, y / z
    ad, bd, J = distort(a, b, d)
    e = np.array([fx * ad + cx, fy * bd + cy]) - meas[:2]
    dab = np.array([[1.0, 0.0, -a], [0.0, 1.0, -b]]) / z
    dp = np.diag([fx, fy]) @ J @ dab
    skew = np.array([[0, -Xb[2], Xb[1]], [Xb[2], 0, -Xb[0]], [-Xb[1], Xb[0], 0]])
    return e, Xb, -dp @ M @ np.hstack([-skew, np.eye(3)]), -dp @ M @ R


class DistortBA(G.RigBA):
    """rig_lm_ref.RigBA with d["e_dist"] [E][5] = (k1, k2, p1, p2, k3): edges whose coefficients are not all zero are
    distorted mono edges"""

    def __init__(self, d, rk=(0, 1.0)):
        super().__init__(d, rk)
        self.dist = np.asarray(d["e_dist"], np.float64)
        self.distorted = np.any(self.dist != 0, axis=1)
        assert not np.any(self.st & self.distorted)

    def _edge(self, i):
        if self.distorted[i]:
            return distorted_edge(self.pose[self.ep[i]], self.lm[self.el[i]], self.meas[i], self.cam[i], self.ext[i], self.dist[i])
        return super()._edge(i)


class DistortGraph(DistortBA):
    def __init__(self, d, via_schur=True):
        super().__init__(d)
        self.via_schur = via_schur

    def solve(self, H, b, lam, via_schur=True):
        return super().solve(H, b, lam, via_schur=self.via_schur)


def permute_edges(d, seed=91):
    perm = np.random.default_rng(seed).permutation(len(d["e_pose"]))
    out = dict(d)
    for key in ("e_pose", "e_lm", "e_stereo", "e_meas", "e_omega", "e_cam", "e_sensor", "e_dist", "e_camera"):
        out[key] = np.asarray(d[key])[perm]
    return out


def reference_runs(d, niter, make=None):
    """rig_lm_ref.reference_runs with this module's graph and permutation"""
    make = make or (lambda dd, vs: DistortGraph(dd, via_schur=vs))
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


# forward and 90 degrees of yaw, 0.4 m apart: camera 0 carries DIST, camera 1 none
RIG2 = G.RIG3[:2]
RIG2_DIST = np.stack([DIST, np.zeros(5)])


def rig_problem(seed=21, n_poses=6, n_landmarks=80, pix_noise=0.1, dist=RIG2_DIST, n_fixed=2, **recipe):
    """rig_lm_ref.make_rig_problem's geometry (two mono cameras; landmark l seen by camera l % 2 from a window of
    poses; `recipe` goes to it), every measurement the projection of the TRUE geometry through its camera's distortion +
    pix_noise; the first n_fixed poses are fixed at the truth (two: the scale does not hang on the 0.4 m between the
    cameras alone, and a wrong model cannot hide in the trajectory).  The dict of make_rig_problem plus e_dist [E][5]"""
    d = G.make_rig_problem(RIG2, (0, 0), n_poses=n_poses, n_landmarks=n_landmarks, seed=seed, pix_noise=0.0, **recipe)
    rng = np.random.default_rng(1000 + seed)
    e_dist = np.asarray(dist, np.float64)[d["e_camera"]]
    ext = np.stack([G.rig_ref.quat_to_ext(q) for q in d["e_sensor"]])
    meas = d["e_meas"].copy()
    r2max = 0.0
    for i in range(len(meas)):
        p, l = d["e_pose"][i], d["e_lm"][i]
        proj = distorted_edge(d["pose_gt"][p], d["lm_gt"][l], np.zeros(3), d["e_cam"][i], ext[i], e_dist[i])[0]
        if np.any(e_dist[i] != 0):
            x, y, z = ext[i, :9].reshape(3, 3) @ (MG.quat_to_R(d["pose_gt"][p, :4]) @ d["lm_gt"][l] + d["pose_gt"][p, 4:]) + ext[i, 9:]
            r2max = max(r2max, (x * x + y * y) / (z * z))
        else:
            assert np.abs(proj - d["e_meas"][i, :2]).max() < 1e-9       # (all zero: the pinhole of the recipe)
        meas[i, :2] = proj + rng.normal(0, pix_noise, 2)
    assert r2max > 0.1, "the distorted camera sees nothing away from its axis"
    pose, pf = d["pose"].copy(), d["pose_fixed"].copy()
    pose[:n_fixed], pf[:n_fixed] = d["pose_gt"][:n_fixed], 1
    return dict(d, e_meas=meas, e_dist=e_dist, pose=pose, pose_fixed=pf)


def without_distortion(d):
    """the same graph (the same raw measurements) with every coefficient zero: the wrong model"""
    return dict(d, e_dist=np.zeros_like(d["e_dist"]))
