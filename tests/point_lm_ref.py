"""Reference for graphs that hold point-to-point edge sets (PointEdgeSet) next to, or instead of, BA edges, ICP sets and
pose priors: the dense numpy LM of tests/golden/make_golden.py through prior_ref.PriorGraph, plus the point terms of
tests/point_edge_ref.py evaluated in float64 (numpy only, no product code), the input recipes of tests/test_point_*.py
and the reference's own round-off sensitivity.

A point set is a dict pose (positions in d['pose']), p [E,3], z [E,3], info [E,3,3] or [1,3,3], active [E] bool, rk."""
import importlib

import numpy as np

import icp_lm_ref
import icp_ref
import point_edge_ref as PE
import prior_ref as PR
import relpose_lm_ref


class PointGraph(PR.PriorGraph):
    """PriorGraph + point-to-point edges"""

    def __init__(self, d, icp, prior, pts, rk=(0, 1.0), via_schur=True):
        super().__init__(d, icp, relpose_lm_ref.empty_prior() if prior is None else prior, rk, via_schur)
        self.pts = pts

    def _pts(self):
        poses = self.pose[np.argsort(self.pidx)]                 # free-first order
        e = dict(self.pts, pose=self.pidx[np.asarray(self.pts["pose"], int)],
                 info6=PE.pack(np.asarray(self.pts["info"], np.float64).reshape(-1, 3, 3)))
        r = PE.point_build(poses, self.np_, e, dtype=np.float64)
        return r["H"], r["b"], float(r["chi"])

    def chi2(self):
        return super().chi2() + self._pts()[2]

    def normal_equations(self):
        H, b = super().normal_equations()
        Hi, bi, _ = self._pts()
        for p in range(self.np_):
            H[6 * p:6 * p + 6, 6 * p:6 * p + 6] += Hi[p]
            b[6 * p:6 * p + 6] += bi[p]
        return H, b


def permuted_points(pts, seed=96):
    perm = np.random.default_rng(seed).permutation(len(pts["pose"]))
    out = dict(pts)
    for k in ("pose", "p", "z", "active"):
        out[k] = np.asarray(pts[k])[perm]
    if len(pts["info"]) > 1:
        out["info"] = np.asarray(pts["info"])[perm]
    return out


def reference_runs(d, icp, prior, pts, niter, rk=(0, 1.0)):
    """as icp_lm_ref.reference_runs: the trajectory, the final estimates and what the reference differs by from itself
    (Schur solve against the full dense solve; every pose edge set in a permuted order)"""
    prior = relpose_lm_ref.empty_prior() if prior is None else prior
    runs = []
    for icp_k, pr_k, pt_k, vs in ((icp, prior, pts, True), (icp, prior, pts, False),
                                  (icp_lm_ref.permuted(icp), PR.permuted_prior(prior), permuted_points(pts), True)):
        g = PointGraph(d, icp_k, pr_k, pt_k, rk, via_schur=vs)
        runs.append((g.optimize(niter), g.pose.copy(), g.lm.copy()))
    tr = runs[0][0]
    sens = [0.0] * len(tr)
    est = 0.0
    for t2, pose2, lm2 in runs[1:]:
        assert [t[4] for t in t2] == [t[4] for t in tr], "the reference disagrees with itself on the trial counts"
        for i in range(len(tr)):
            sens[i] = max(sens[i], abs(tr[i][1] - t2[i][1]) / max(abs(tr[i][1]), 1e-300))
        est = max(est, float(np.abs(runs[0][1] - pose2).max()), float(np.abs(runs[0][2] - lm2).max()) if len(lm2) else 0.0)
    return icp_lm_ref.trace_dicts(tr), runs[0][1], runs[0][2], sens, est


# ------------------------------------------------------------------ input recipes ----------
def random_spd3(rng, scale=1.0, cond=1.0):
    Q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    return scale * (Q * np.array([1.0, cond ** 0.5, cond])) @ Q.T


def make_points(rng, pose_of_edge, gt, noise, info, rk=(0, 1.0), active=None, spread=3.0):
    """points p ~ N(0, spread), measured at the poses `gt` with noise N(0, noise)"""
    pose = np.asarray(pose_of_edge, np.int32)
    E = len(pose)
    p = rng.normal(0, spread, (E, 3))
    z = np.array([icp_ref.transform(gt[q], x) for q, x in zip(pose, p)]).reshape(E, 3) + (rng.normal(0, noise, (E, 3)) if noise else 0.0)
    return dict(pose=pose, p=p, z=z, info=np.asarray(info, np.float64).reshape(-1, 3, 3),
                active=np.ones(E, bool) if active is None else np.asarray(active, bool), rk=rk)


def no_ba(pose, pose_fixed, gt):
    return dict(pose=pose, pose_fixed=pose_fixed, lm=np.zeros((0, 3)), lm_fixed=np.zeros(0, np.uint8),
                e_pose=np.zeros(0, np.int32), e_lm=np.zeros(0, np.int32), e_stereo=np.zeros(0, np.uint8),
                e_meas=np.zeros((0, 3)), e_omega=np.zeros(0), e_cam=np.zeros((0, 5)), pose_gt=gt)


def points_only_case(seed=11, P=6):
    """(a) 6 poses, the last fixed, no landmarks: 300 edges (30 of them on the fixed pose), per-edge Omega of condition up
    to 100, Huber"""
    rng = np.random.default_rng(seed)
    gt = np.array([icp_ref.random_pose(rng) for _ in range(P)])
    pose = gt.copy()
    for i in range(P - 1):
        pose[i] = icp_ref.left_update(gt[i], np.concatenate([rng.normal(0, 0.3, 3), rng.normal(0, 1.0, 3)]))
    pf = np.zeros(P, np.uint8)
    pf[P - 1] = 1
    d = no_ba(pose, pf, gt)
    pe = np.repeat(np.arange(P, dtype=np.int32), [70, 45, 80, 35, 40, 30])
    rng.shuffle(pe)
    info = np.array([random_spd3(rng, rng.uniform(50, 200), 10.0 ** rng.uniform(0, 2)) for _ in pe])
    return d, [], None, make_points(rng, pe, gt, 0.02, info, rk=(icp_ref.RK_HUBER, 1.5))


def mixed_case(seed=5):
    """(b) prior_ref.mixed_prior_case (BA + plane + line + priors, pose 0 fixed) + 180 point edges with a shared singular-free
    Omega on poses 1, 2, 5, 8 and the fixed pose 0, Cauchy, 10 % inactive"""
    d, icp, prior = PR.mixed_prior_case(seed=seed)
    rng = np.random.default_rng(seed + 300)
    pe = np.repeat(np.array([0, 1, 2, 5, 8], np.int32), [20, 50, 30, 45, 35])
    rng.shuffle(pe)
    info = np.array([random_spd3(rng, rng.uniform(1e3, 4e3), 10.0 ** rng.uniform(0, 1.5)) for _ in pe])
    return d, icp, prior, make_points(rng, pe, d["pose_gt"], 0.02, info, rk=(icp_ref.RK_CAUCHY, 3.0), active=rng.random(len(pe)) >= 0.1)


def reject_case(seed=3):
    """(c) icp_lm_ref.reject_case (it takes rejected trials) + 20 point edges per free pose placed at the INITIAL poses, one
    Omega for all"""
    d, icp = icp_lm_ref.reject_case(seed=seed)
    rng = np.random.default_rng(seed + 400)
    free = np.nonzero(np.asarray(d["pose_fixed"]) == 0)[0].astype(np.int32)
    pe = np.repeat(free, 20)
    return d, icp, None, make_points(rng, pe, d["pose"], 0.05, random_spd3(rng, 3.0, 4.0)[None])


def zero_noise_case(seed=13, n=200):
    """(d) one free pose, 200 exact correspondences, the start 0.5 rad / 1 m away: ends at the truth"""
    rng = np.random.default_rng(seed)
    gt = np.array([icp_ref.random_pose(rng)])
    ax = rng.normal(size=3)
    t = rng.normal(size=3)
    pose = np.array([icp_ref.left_update(gt[0], np.concatenate([0.5 * ax / np.linalg.norm(ax), t / np.linalg.norm(t)]))])
    d = no_ba(pose, np.zeros(1, np.uint8), gt)
    return d, [], None, make_points(rng, np.zeros(n, np.int32), gt, 0.0, np.eye(3)[None])


CASES = {  # name -> (recipe, iterations)
    "points_only": (points_only_case, 6),
    "mixed": (mixed_case, 8),
    "reject": (reject_case, 8),
    "zero_noise": (zero_noise_case, 8),
}


# ---- the product's graph from a recipe ----------------------------------------------------------------------------
def add_points(g, pts, pose_ids=None):
    """the point set of a recipe into a cugo Graph; inactive edges are left out (the C ABI adds active edges only)"""
    act = np.asarray(pts["active"], bool)
    ids = np.asarray(pts["pose"], np.int32) if pose_ids is None else np.asarray(pose_ids, np.int32)[pts["pose"]]
    info = np.asarray(pts["info"], np.float64).reshape(-1, 3, 3)
    g.set_point_information(info[0])
    g.add_point_edges(ids[act], np.asarray(pts["p"])[act], np.asarray(pts["z"])[act],
                      np.broadcast_to(info, (len(act), 3, 3))[act])
    g.set_point_robust_kernel(pts["rk"][0], pts["rk"][1])


def build_graph(d, icp, prior, pts, rk=(0, 1.0), plan_only=False, per_edge_information=True):
    g = PR.build_graph(d, icp, prior, rk=rk, plan_only=plan_only, per_edge_information=per_edge_information)
    if pts is not None:
        add_points(g, pts)
    return g
