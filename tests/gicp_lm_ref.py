"""Reference for graphs that hold covariance-form point edge sets (GicpEdgeSet, GicpPairEdgeSet: generalised ICP) next to, or
instead of, the other sets: the dense numpy LM of point_pair_lm_ref.PairGraph with Omega = (C_z + M C_p M^T)^-1 RE-EVALUATED
from the covariances at the poses of every linearisation and of every trial (numpy only, float64, no product code), the
input recipes of tests/test_gicp_graph*.py and the reference's own round-off sensitivity, measured as
point_pair_lm_ref.reference_runs measures it.  `frozen=True` keeps the Omega of the INITIAL poses instead: what an
implementation that does not follow the poses would minimise.

A covariance-form set is the dict of point_lm_ref (pose, p, z, active, rk) or point_pair_lm_ref (a, b, p, z, active, rk) with
cov_p, cov_z [E,3,3] or [1,3,3] in place of info."""
import numpy as np

import icp_lm_ref
import icp_ref
import point_lm_ref as PL
import point_pair_lm_ref as PPL
import point_pair_ref as PP
import prior_ref as PR
import relpose_lm_ref as RL


def empty_pairs():
    z = np.zeros(0, np.int32)
    return dict(a=z, b=z, p=np.zeros((0, 3)), z=np.zeros((0, 3)), cov_p=np.eye(3)[None], cov_z=np.eye(3)[None], active=np.zeros(0, bool), rk=(0, 1.0))


def empty_points():
    return dict(pose=np.zeros(0, np.int32), p=np.zeros((0, 3)), z=np.zeros((0, 3)), cov_p=np.eye(3)[None], cov_z=np.eye(3)[None],
                active=np.zeros(0, bool), rk=(0, 1.0))


def omega(M, cov_p, cov_z):
    """[E,3,3] = (C_z + M C_p M^T)^-1, symmetrised"""
    E = len(M)
    Cp = np.broadcast_to(np.asarray(cov_p, np.float64).reshape(-1, 3, 3), (E, 3, 3))
    Cz = np.broadcast_to(np.asarray(cov_z, np.float64).reshape(-1, 3, 3), (E, 3, 3))
    S = Cz + np.einsum("eik,ekl,ejl->eij", M, Cp, M)
    Om = np.linalg.inv((S + S.transpose(0, 2, 1)) / 2) if E else np.zeros((0, 3, 3))
    return (Om + Om.transpose(0, 2, 1)) / 2


class GicpGraph(PPL.PairGraph):
    """PairGraph whose point set (gpts) and pair set (gpairs) are in the covariance form; `pts` stays an information-form
    PointEdgeSet beside them"""

    def __init__(self, d, icp, prior, pts, relpose, gpts, gpairs, rk=(0, 1.0), via_schur=True, frozen=False):
        super().__init__(d, icp, prior, pts, relpose, None, rk, via_schur)
        self.gpts = empty_points() if gpts is None else gpts
        self.gpairs = empty_pairs() if gpairs is None else gpairs
        self.frozen_poses = self.pose.copy() if frozen else None

    def _rot(self, idx, frozen_ok=True):
        src = self.frozen_poses if self.frozen_poses is not None else self.pose
        return PP._rot(np.asarray(src, np.float64)[np.asarray(idx, int), :4])[0]

    def _pairs(self):
        P = self.np_
        poses = self.pose[np.argsort(self.pidx)]
        g = self.gpairs
        M = np.einsum("eik,ejk->eij", self._rot(g["b"]), self._rot(g["a"]))
        e = dict(a=self.pidx[np.asarray(g["a"], int)], b=self.pidx[np.asarray(g["b"], int)], p=g["p"], z=g["z"], active=g["active"], rk=g["rk"],
                 info6=PP.pack(omega(M, g["cov_p"], g["cov_z"])) if len(M) else np.zeros((1, 6)))
        r = PP.pair_build(poses, P, len(poses), e, dtype=np.float64)
        A, bv = np.zeros((6 * P, 6 * P)), r["b"][:P].reshape(-1).copy()
        for p in range(P):
            A[6 * p:6 * p + 6, 6 * p:6 * p + 6] = r["H"][p]
        for lo, hi, blk in zip(r["pair_lo"], r["pair_hi"], r["Hoff"]):
            A[6 * lo:6 * lo + 6, 6 * hi:6 * hi + 6] = blk
            A[6 * hi:6 * hi + 6, 6 * lo:6 * lo + 6] = blk.T
        return A, bv, float(r["chi"])

    def _gpts(self):
        import point_edge_ref as PE
        poses = self.pose[np.argsort(self.pidx)]
        g = self.gpts
        e = dict(pose=self.pidx[np.asarray(g["pose"], int)], p=g["p"], z=g["z"], active=g["active"], rk=g["rk"],
                 info6=PE.pack(omega(self._rot(g["pose"]), g["cov_p"], g["cov_z"])) if len(g["pose"]) else np.zeros((1, 6)))
        r = PE.point_build(poses, self.np_, e, dtype=np.float64)
        return r["H"], r["b"], float(r["chi"])

    def chi2(self):
        return super().chi2() + self._gpts()[2]

    def normal_equations(self):
        H, b = super().normal_equations()
        Hi, bi, _ = self._gpts()
        for p in range(self.np_):
            H[6 * p:6 * p + 6, 6 * p:6 * p + 6] += Hi[p]
            b[6 * p:6 * p + 6] += bi[p]
        return H, b


def permuted(s, keys, seed):
    n = len(s[keys[0]])
    perm = np.random.default_rng(seed).permutation(n)
    out = dict(s)
    for k in keys + ("p", "z", "active"):
        out[k] = np.asarray(s[k])[perm]
    for k in ("cov_p", "cov_z"):
        if len(s[k]) > 1:
            out[k] = np.asarray(s[k])[perm]
    return out


def reference_runs(d, icp, prior, pts, relpose, gpts, gpairs, niter, rk=(0, 1.0), frozen=False):
    """the trajectory, the final estimates and what the reference differs by from itself (Schur solve against the full dense
    solve; every pose edge set in a permuted order)"""
    prior = RL.empty_prior() if prior is None else prior
    pts = PPL.empty_points() if pts is None else pts
    relpose = PPL.empty_relpose() if relpose is None else relpose
    gpts = empty_points() if gpts is None else gpts
    gpairs = empty_pairs() if gpairs is None else gpairs
    runs = []
    for icp_k, pr_k, pt_k, rp_k, gp_k, gq_k, vs in (
            (icp, prior, pts, relpose, gpts, gpairs, True), (icp, prior, pts, relpose, gpts, gpairs, False),
            (icp_lm_ref.permuted(icp), PR.permuted_prior(prior), PL.permuted_points(pts), RL.permuted_relpose(relpose),
             permuted(gpts, ("pose",), 97), permuted(gpairs, ("a", "b"), 98), True)):
        g = GicpGraph(d, icp_k, pr_k, pt_k, rp_k, gp_k, gq_k, rk, via_schur=vs, frozen=frozen)
        runs.append((g.optimize(niter), g.pose.copy(), g.lm.copy()))
    tr = runs[0][0]
    sens, est = [0.0] * len(tr), 0.0
    for t2, pose2, lm2 in runs[1:]:
        assert [t[4] for t in t2] == [t[4] for t in tr], "the reference disagrees with itself on the trial counts"
        for i in range(len(tr)):
            sens[i] = max(sens[i], abs(tr[i][1] - t2[i][1]) / max(abs(tr[i][1]), 1e-300))
        est = max(est, float(np.abs(runs[0][1] - pose2).max()), float(np.abs(runs[0][2] - lm2).max()) if len(lm2) else 0.0)
    return icp_lm_ref.trace_dicts(tr), runs[0][1], runs[0][2], sens, est


# ------------------------------------------------------------------ input recipes ----------
def surface_cov(rng, n, sigma, thin=1e-3):
    """class 'gicp': sigma^2 x eigenvalues (1, 1, thin) x a scale in 0.5 .. 2, in random frames"""
    Q = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    lam = sigma * sigma * rng.uniform(0.5, 2.0, n)[:, None] * np.array([1.0, 1.0, thin])
    C = np.einsum("eik,ek,ejk->eij", Q, lam, Q)
    return (C + C.transpose(0, 2, 1)) / 2


def iso_cov(rng, n, sigma):
    return (sigma * sigma * rng.uniform(0.5, 2.0, n))[:, None, None] * np.eye(3)[None]


def with_cov(rng, s, cls, sigma=0.05):
    n = len(s["p"])
    out = {k: v for k, v in s.items() if k != "info"}
    f = iso_cov if cls == "iso" else surface_cov
    out["cov_p"], out["cov_z"] = f(rng, n, sigma), f(rng, n, sigma)
    return out


def scan_to_map_case(seed=31):
    """unary: 5 poses, pose 4 fixed, 150 edges per pose against a fixed map, class gicp, the start 10 - 20 degrees and 0.5 m
    away; no landmarks"""
    rng = np.random.default_rng(seed)
    P = 5
    gt = np.array([icp_ref.random_pose(rng) for _ in range(P)])
    pose = gt.copy()
    for i in range(P - 1):
        w = rng.normal(size=3)
        w *= np.deg2rad(rng.uniform(10, 20)) / np.linalg.norm(w)
        pose[i] = icp_ref.left_update(gt[i], np.concatenate([w, rng.normal(0, 0.5, 3)]))
    pf = np.zeros(P, np.uint8)
    pf[P - 1] = 1
    d = PL.no_ba(pose, pf, gt)
    pe = np.repeat(np.arange(P, dtype=np.int32), 150)
    rng.shuffle(pe)
    pts = PL.make_points(rng, pe, gt, 0.02, np.eye(3)[None], rk=(icp_ref.RK_NONE, 1.0))
    return d, [], None, None, None, with_cov(rng, pts, "gicp"), None


def multi_scan_case(seed=32, cls="gicp"):
    """pair: the ring of 6 plus two chords, 40 edges per pair, pose 5 fixed, Huber"""
    d, icp, prior, pts, rp, pairs = PPL.multi_scan_case(seed, rk=(icp_ref.RK_HUBER, 2.0))
    rng = np.random.default_rng(seed + 1)
    return d, icp, prior, pts, rp, None, with_cov(rng, pairs, cls)


def iso_case(seed=32):
    return multi_scan_case(seed, "iso")


def mixed_case(seed=8):
    """point_pair_lm_ref.mixed_case (BA + plane + line + priors + relative-pose edges + a PointEdgeSet) with its pair set in
    the covariance form"""
    d, icp, prior, pts, rp, pairs = PPL.mixed_case(seed)
    rng = np.random.default_rng(seed + 700)
    return d, icp, prior, pts, rp, None, with_cov(rng, pairs, "gicp", sigma=0.02)


def zero_noise_case(seed=33):
    d, icp, prior, pts, rp, pairs = PPL.zero_noise_case(seed)
    rng = np.random.default_rng(seed + 1)
    return d, icp, prior, pts, rp, None, with_cov(rng, pairs, "gicp", sigma=1.0)


def reject_case(seed=3):
    d, icp, prior, pts, rp, pairs = PPL.reject_case(seed)
    rng = np.random.default_rng(seed + 800)
    return d, icp, prior, pts, rp, None, with_cov(rng, pairs, "gicp", sigma=0.5)


CASES = {  # name -> (recipe, iterations)
    "scan_to_map": (scan_to_map_case, 4),
    "multi_scan": (multi_scan_case, 5),
    "mixed": (mixed_case, 8),
    "iso": (iso_case, 3),
    "reject": (reject_case, 8),
}


# ---- the product's graph from a recipe ----------------------------------------------------------------------------
def _cov9(c, n):
    return np.broadcast_to(np.asarray(c, np.float64).reshape(-1, 3, 3), (n, 3, 3))


def add_gicp(g, gpts, gpairs):
    if gpts is not None and len(gpts["pose"]):
        n = len(gpts["pose"])
        assert np.all(gpts["active"])
        g.add_gicp_edges(gpts["pose"], gpts["p"], gpts["z"], _cov9(gpts["cov_p"], n), _cov9(gpts["cov_z"], n))
        g.set_gicp_robust_kernel(gpts["rk"][0], gpts["rk"][1])
    if gpairs is not None and len(gpairs["a"]):
        n = len(gpairs["a"])
        g.add_gicp_pair_edges(gpairs["a"], gpairs["b"], gpairs["p"], gpairs["z"], _cov9(gpairs["cov_p"], n), _cov9(gpairs["cov_z"], n))
        if not np.all(gpairs["active"]):
            g.set_gicp_pair_active(gpairs["active"])
        g.set_gicp_pair_robust_kernel(gpairs["rk"][0], gpairs["rk"][1])


def build_graph(d, icp, prior, pts, rp, gpts, gpairs, plan_only=False):
    g = PPL.build_graph(d, icp, prior, pts, rp, None, plan_only=plan_only)
    add_gicp(g, gpts, gpairs)
    return g
