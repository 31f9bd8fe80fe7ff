"""Reference for graphs that hold pose-pose point edge sets (PointPairEdgeSet) next to, or instead of, the other sets:
the dense numpy LM of point_lm_ref.PointGraph, plus the relative-pose terms of relpose_lm_ref and the pair terms of
tests/point_pair_ref.py evaluated in float64, off-diagonal blocks included (numpy only, no product code), the input
recipes of tests/test_point_pair_graph*.py and the reference's own round-off sensitivity.

A pair set is a dict a, b (positions in d['pose']), p [E,3] (in a's frame), z [E,3] (in b's frame), info [E,3,3] or
[1,3,3], active [E] bool, rk."""
import numpy as np

import icp_lm_ref
import icp_ref
import point_lm_ref as PL
import point_pair_ref as PP
import prior_ref as PR
import relpose_lm_ref as RL
import relpose_ref as RR
import synth


def empty_points():
    return dict(pose=np.zeros(0, np.int32), p=np.zeros((0, 3)), z=np.zeros((0, 3)), info=np.eye(3)[None], active=np.zeros(0, bool), rk=(0, 1.0))


def empty_relpose():
    return RR.make_edges(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 7)), np.eye(6)[None])


class PairGraph(PL.PointGraph):
    """PointGraph + relative-pose edges + pose-pose point edges"""

    def __init__(self, d, icp, prior, pts, relpose, pairs, rk=(0, 1.0), via_schur=True):
        super().__init__(d, icp, prior, empty_points() if pts is None else pts, rk, via_schur)
        self.relpose = empty_relpose() if relpose is None else relpose
        self.pairs = pairs

    def _pairs(self):
        """dense [6P, 6P] matrix, rhs and chi2 of the pair terms, free-first order"""
        P = self.np_
        poses = self.pose[np.argsort(self.pidx)]
        e = dict(self.pairs, a=self.pidx[np.asarray(self.pairs["a"], int)], b=self.pidx[np.asarray(self.pairs["b"], int)],
                 info6=PP.pack(np.asarray(self.pairs["info"], np.float64).reshape(-1, 3, 3)))
        r = PP.pair_build(poses, P, len(poses), e, dtype=np.float64)
        A, bv = np.zeros((6 * P, 6 * P)), r["b"][:P].reshape(-1).copy()
        for p in range(P):
            A[6 * p:6 * p + 6, 6 * p:6 * p + 6] = r["H"][p]
        for lo, hi, blk in zip(r["pair_lo"], r["pair_hi"], r["Hoff"]):
            A[6 * lo:6 * lo + 6, 6 * hi:6 * hi + 6] = blk
            A[6 * hi:6 * hi + 6, 6 * lo:6 * lo + 6] = blk.T
        return A, bv, float(r["chi"])

    def chi2(self):
        return super().chi2() + RL.RelPoseGraph._relpose(self)[2] + self._pairs()[2]

    def normal_equations(self):
        H, b = super().normal_equations()
        n = 6 * self.np_
        for A, bp, _ in (RL.RelPoseGraph._relpose(self), self._pairs()):
            H[:n, :n] += A
            b[:n] += bp
        return H, b


def permuted_pairs(pairs, seed=95):
    perm = np.random.default_rng(seed).permutation(len(pairs["a"]))
    out = dict(pairs)
    for k in ("a", "b", "p", "z", "active"):
        out[k] = np.asarray(pairs[k])[perm]
    if len(pairs["info"]) > 1:
        out["info"] = np.asarray(pairs["info"])[perm]
    return out


def reference_runs(d, icp, prior, pts, relpose, pairs, niter, rk=(0, 1.0)):
    """as point_lm_ref.reference_runs: the trajectory, the final estimates and what the reference differs by from itself
    (Schur solve against the full dense solve; every pose edge set in a permuted order)"""
    prior = RL.empty_prior() if prior is None else prior
    pts = empty_points() if pts is None else pts
    relpose = empty_relpose() if relpose is None else relpose
    runs = []
    for icp_k, pr_k, pt_k, rp_k, pp_k, vs in (
            (icp, prior, pts, relpose, pairs, True), (icp, prior, pts, relpose, pairs, False),
            (icp_lm_ref.permuted(icp), PR.permuted_prior(prior), PL.permuted_points(pts), RL.permuted_relpose(relpose),
             permuted_pairs(pairs), True)):
        g = PairGraph(d, icp_k, pr_k, pt_k, rp_k, pp_k, rk, via_schur=vs)
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
RING = [(0, 1), (2, 1), (2, 3), (4, 3), (4, 5), (0, 5), (0, 3), (4, 1)]     # a ring of 6 plus two chords, mixed orientation


def make_pairs(rng, pairs, gt, n_per_pair, noise, info_of, rk=(0, 1.0), inactive=0.0, spread=3.0):
    """n_per_pair correspondences per pair from one synthetic cloud ~ N(0, spread) in the world, seen from a and from b at
    the poses `gt` with noise N(0, noise) each; info_of(rng) gives an edge's Omega"""
    a = np.repeat([p[0] for p in pairs], n_per_pair).astype(np.int32)
    b = np.repeat([p[1] for p in pairs], n_per_pair).astype(np.int32)
    E = len(a)
    cloud = rng.normal(0, spread, (200, 3))
    X = cloud[rng.integers(0, len(cloud), E)]
    see = lambda q, x: np.array([icp_ref.transform(gt[i], v) for i, v in zip(q, x)]).reshape(E, 3) + (rng.normal(0, noise, (E, 3)) if noise else 0.0)
    info = np.array([info_of(rng) for _ in range(E)])
    return dict(a=a, b=b, p=see(a, X), z=see(b, X), info=info, active=rng.random(E) >= inactive, rk=rk)


def multi_scan_case(seed=21, rk=(0, 1.0), noise=0.02):
    """(a) a pure multi-scan graph: 6 poses, pose 5 fixed, the ring plus two chords, 40 noisy correspondences per pair
    from a common cloud, per-edge Omega of condition up to 100; no landmarks"""
    rng = np.random.default_rng(seed)
    P = 6
    gt = np.array([icp_ref.random_pose(rng) for _ in range(P)])
    pose = gt.copy()
    for i in range(P - 1):
        pose[i] = icp_ref.left_update(gt[i], np.concatenate([rng.normal(0, 0.25, 3), rng.normal(0, 0.8, 3)]))
    pf = np.zeros(P, np.uint8)
    pf[P - 1] = 1
    d = PL.no_ba(pose, pf, gt)
    pairs = make_pairs(rng, RING, gt, 40, noise, lambda r: PL.random_spd3(r, r.uniform(50, 200), 10.0 ** r.uniform(0, 2)), rk=rk,
                       inactive=0.05)
    return d, [], None, None, None, pairs


def huber_case(seed=22):
    """(c) the same with Huber and ten times the noise on a tenth of the edges"""
    d, icp, prior, pts, rp, pairs = multi_scan_case(seed, rk=(icp_ref.RK_HUBER, 1.0))
    rng = np.random.default_rng(seed + 1)
    bad = rng.random(len(pairs["a"])) < 0.1
    pairs["z"] = pairs["z"] + bad[:, None] * rng.normal(0, 0.2, pairs["z"].shape)
    return d, icp, prior, pts, rp, pairs


def mixed_case(seed=8):
    """(b) relpose_lm_ref.mixed_case (BA + plane + line + priors + relative-pose edges, pose 0 fixed) + a PointEdgeSet + pair
    edges over two co-visible pairs that ALSO carry relative-pose edges (one block, three contributors), a pair with the
    fixed end and, where the BA part leaves one, a pair that shares no landmark and no relative-pose edge; Cauchy"""
    d, icp, prior, rp = RL.mixed_case(seed=seed)
    rng = np.random.default_rng(seed + 500)
    gt = d["pose_gt"]
    pe = np.repeat(np.array([1, 4], np.int32), [25, 30])
    pts = PL.make_points(rng, pe, gt, 0.02, np.array([PL.random_spd3(rng, 2e3, 10.0) for _ in pe]), rk=(icp_ref.RK_NONE, 1.0))
    pidx, _ = RL.free_first(d)
    cov, joined = RL.covisible_pairs(d), RL.relpose_pairs(d, rp)
    key = lambda a, b: (min(pidx[a], pidx[b]), max(pidx[a], pidx[b]))
    free = [(a, b) for a in range(1, 6) for b in range(a + 1, 6)]
    shared = [q for q in free if key(*q) in joined and key(*q) in cov]
    alone = [q for q in free if key(*q) not in joined and key(*q) not in cov]
    assert shared, "the recipe needs a co-visible pair that a relative-pose edge joins"
    chosen = [shared[0], shared[-1][::-1], (0, 2)] + ([alone[0]] if alone else [])
    pairs = make_pairs(rng, chosen, gt, 40, 0.01, lambda r: PL.random_spd3(r, r.uniform(1e3, 4e3), 10.0 ** r.uniform(0, 1.5)),
                       rk=(icp_ref.RK_CAUCHY, 3.0))
    return d, icp, prior, pts, rp, pairs


def zero_noise_case(seed=23):
    """(d) the multi-scan graph with exact correspondences and Omega = I: ends at the truth"""
    rng = np.random.default_rng(seed)
    d, icp, prior, pts, rp, _ = multi_scan_case(seed)
    pairs = make_pairs(rng, RING, d["pose_gt"], 40, 0.0, lambda r: np.eye(3))
    return d, icp, prior, pts, rp, pairs


def reject_case(seed=3):
    """icp_lm_ref.reject_case's BA part (the golden stress fixture reject_8x60: it takes rejected trials) + 20 pair edges
    over every consecutive pair and two closures, placed at the INITIAL poses, one Omega for all"""
    d, _ = icp_lm_ref.reject_case(seed=seed)
    rng = np.random.default_rng(seed + 600)
    P = len(d["pose"])
    chosen = [(i, i + 1) if i % 2 == 0 else (i + 1, i) for i in range(P - 1)] + [(0, P - 1), (5, 2)]
    om = PL.random_spd3(rng, 3.0, 4.0)
    return d, [], None, None, None, make_pairs(rng, chosen, np.asarray(d["pose"]), 20, 0.05, lambda r: om)


CASES = {  # name -> (recipe, iterations)
    "reject": (reject_case, 8),
    "multi_scan": (multi_scan_case, 4),
    "mixed": (mixed_case, 8),
    "huber": (huber_case, 6),
    "zero_noise": (zero_noise_case, 8),
}


def free_first_pairs(d, pairs):
    pidx, P = RL.free_first(d)
    a, b = pidx[np.asarray(pairs["a"], int)], pidx[np.asarray(pairs["b"], int)]
    return a, b, P


def counting_edges(d, pairs):
    a, b, P = free_first_pairs(d, pairs)
    return int((np.asarray(pairs["active"], bool) & ((a < P) | (b < P))).sum())


def pair_blocks(d, pairs):
    """{(lo, hi)}: the free-free pairs the counting pair edges join, free-first indices"""
    a, b, P = free_first_pairs(d, pairs)
    ok = np.asarray(pairs["active"], bool) & (a < P) & (b < P)
    return {(int(min(x, y)), int(max(x, y))) for x, y in zip(a[ok], b[ok])}


# ---- the product's graph from a recipe ----------------------------------------------------------------------------
def add_pairs(g, pairs, with_inactive=True):
    """the pair set of a recipe into a cugo Graph: every edge is added and the inactive ones are switched off"""
    info = np.broadcast_to(np.asarray(pairs["info"], np.float64).reshape(-1, 3, 3), (len(pairs["a"]), 3, 3))
    g.add_point_pair_edges(pairs["a"], pairs["b"], pairs["p"], pairs["z"], info)
    if with_inactive and not np.all(pairs["active"]):
        g.set_point_pair_active(pairs["active"])
    g.set_point_pair_robust_kernel(pairs["rk"][0], pairs["rk"][1])


def build_graph(d, icp, prior, pts, rp, pairs, rk=(0, 1.0), plan_only=False, per_edge_information=True):
    g = PR.build_graph(d, icp, prior, rk=rk, plan_only=plan_only, per_edge_information=per_edge_information)
    if pts is not None:
        PL.add_points(g, pts)
    if rp is not None:
        RL.add_relpose(g, rp)
    if pairs is not None:
        add_pairs(g, pairs)
    return g
