"""Reference for graphs that hold relative-pose SE(3) edge sets (include/relpose_types.h) next to, or instead of, BA
edges, ICP edges and pose priors: the dense numpy LM of tests/prior_ref.PriorGraph plus tests/relpose_ref.reference_build
for the pose-pose terms (numpy only, no product code), the input recipes of tests/test_relpose_graph*.py and the
reference's own round-off sensitivity.

With these edges Hpp is no longer block-diagonal: an edge between two free poses adds both diagonal blocks, the (lo, hi)
block and its transpose.  The Schur form of the reference therefore ends with Hsc(lo, hi) = Hpp(lo, hi) - sum of products.
Edge ends are positions in d["pose"]; Graph.pidx maps them to the free-first index.
"""
import numpy as np

import icp_lm_ref
import icp_ref
import prior_ref as PR
import relpose_ref as RR
import synth


class RelPoseGraph(PR.PriorGraph):
    """PriorGraph + relative-pose edges.  relpose: dict a, b (positions in d['pose']), z [E,7], info [E,6,6] or [1,6,6],
    active [E] bool, rk (relpose_ref.make_edges)"""

    def __init__(self, d, icp, prior, relpose, rk=(0, 1.0), via_schur=True):
        super().__init__(d, icp, prior, rk, via_schur)
        self.relpose = relpose

    def _relpose(self):
        poses = self.pose[np.argsort(self.pidx)]  # free-first order, as reference_build indexes
        rp = dict(self.relpose, a=self.pidx[np.asarray(self.relpose["a"], int)],
                  b=self.pidx[np.asarray(self.relpose["b"], int)])
        rowptr, colind = RR.pattern(rp, self.np_)
        H, b, Hoff, chi, _ = RR.reference_build(poses, self.np_, rp, rowptr, colind)
        return RR.dense_system(H, b, Hoff, rowptr, colind) + (chi,)

    def chi2(self):
        return super().chi2() + self._relpose()[2]

    def normal_equations(self):
        H, b = super().normal_equations()
        A, bp, _ = self._relpose()
        n = 6 * self.np_
        H[:n, :n] += A
        b[:n] += bp
        return H, b


def empty_prior():
    return PR.make_prior(np.zeros(0, np.int32), np.zeros((0, 7)), np.eye(6)[None])


def permuted_relpose(rp, seed=97):
    perm = np.random.default_rng(seed).permutation(len(rp["a"]))
    out = dict(rp)
    for k in ("a", "b", "z", "active"):
        out[k] = np.asarray(rp[k])[perm]
    if len(rp["info"]) > 1:
        out["info"] = np.asarray(rp["info"])[perm]
    return out


def reference_runs(d, icp, prior, relpose, niter, rk=(0, 1.0)):
    """as prior_ref.reference_runs: the trajectory, the final estimates and what the reference differs by from itself
    (Schur solve against the full dense solve; the edges of every kind in a permuted order)"""
    runs = []
    for icp_k, pr_k, rp_k, vs in ((icp, prior, relpose, True), (icp, prior, relpose, False),
                                  (icp_lm_ref.permuted(icp), PR.permuted_prior(prior), permuted_relpose(relpose), True)):
        g = RelPoseGraph(d, icp_k, pr_k, rp_k, rk, via_schur=vs)
        runs.append((g.optimize(niter), g.pose.copy(), g.lm.copy()))
    tr = runs[0][0]
    sens = [0.0] * len(tr)
    est = 0.0
    for t2, pose2, lm2 in runs[1:]:
        assert [t[4] for t in t2] == [t[4] for t in tr], "the reference disagrees with itself on the trial counts"
        for i in range(len(tr)):
            sens[i] = max(sens[i], abs(tr[i][1] - t2[i][1]) / abs(tr[i][1]))
        est = max(est, float(np.abs(runs[0][1] - pose2).max()), float(np.abs(runs[0][2] - lm2).max()) if len(lm2) else 0.0)
    return icp_lm_ref.trace_dicts(tr), runs[0][1], runs[0][2], sens, est


# ---- what the product must report, in numpy ------------------------------------------------------------------------
def free_first(d):
    pf = np.asarray(d["pose_fixed"]).astype(bool)
    pidx = np.zeros(len(pf), int)
    pidx[~pf] = np.arange((~pf).sum())
    pidx[pf] = (~pf).sum() + np.arange(pf.sum())
    return pidx, int((~pf).sum())


def counting_edges(d, relpose):
    """number of relative-pose edges that count: active, at least one free end"""
    pidx, P = free_first(d)
    rp = dict(relpose, a=pidx[np.asarray(relpose["a"], int)], b=pidx[np.asarray(relpose["b"], int)])
    return int(RR.counting(rp, P).sum())


def covisible_pairs(d):
    """{(lo, hi)}: pairs of free poses (free-first indices) that see a common free landmark through active BA edges"""
    pidx, P = free_first(d)
    lf = np.asarray(d["lm_fixed"]).astype(bool)
    seen = {}
    for p, l in zip(np.asarray(d["e_pose"]), np.asarray(d["e_lm"])):
        if pidx[p] < P and not lf[l]:
            seen.setdefault(int(l), set()).add(int(pidx[p]))
    out = set()
    for ps in seen.values():
        ps = sorted(ps)
        out |= {(a, b) for i, a in enumerate(ps) for b in ps[i + 1:]}
    return out


def relpose_pairs(d, relpose):
    """{(lo, hi)}: the free-free pairs the counting relative-pose edges join (relpose_ref.pattern's off-diagonal blocks)"""
    pidx, P = free_first(d)
    rp = dict(relpose, a=pidx[np.asarray(relpose["a"], int)], b=pidx[np.asarray(relpose["b"], int)])
    rowptr, colind = RR.pattern(rp, P)
    return {(p, int(colind[k])) for p in range(P) for k in range(rowptr[p] + 1, rowptr[p + 1])}


def union_pattern_blocks(d, relpose):
    """blocks of the Hsc pattern: one per free pose, one per pair that is co-visible or joined by a counting edge"""
    return free_first(d)[1] + len(covisible_pairs(d) | relpose_pairs(d, relpose))


# ---- input recipes ---------------------------------------------------------------------------------------------
def no_ba(pose, pose_fixed, gt):
    return dict(pose=pose, pose_fixed=np.asarray(pose_fixed, np.uint8), lm=np.zeros((0, 3)), lm_fixed=np.zeros(0, np.uint8),
                e_pose=np.zeros(0, np.int32), e_lm=np.zeros(0, np.int32), e_stereo=np.zeros(0, np.uint8),
                e_meas=np.zeros((0, 3)), e_omega=np.zeros(0), e_cam=np.zeros((0, 5)), pose_gt=gt)


def edges_between(rng, gt, pairs, rot, trans, scale, rk=(RR.RK_NONE, 1.0)):
    """edges over `pairs` (positions, orientation as given) measured at gt with noise N(0, rot), N(0, trans), dense Omega"""
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    z = np.array([RR.measured(rng, gt[a], gt[b], rot, trans) for a, b in pairs])
    info = np.array([PR.random_spd(rng, scale) for _ in pairs])
    return RR.make_edges(pairs[:, 0], pairs[:, 1], z, info, rk=rk)


def chain_case(seed=4):
    """a pure pose graph (no landmark, no BA edge): 6 poses, pose 0 fixed; odometry edges 0-1 ... 4-5 in alternating
    orientation (a < b, a > b), the first of them with its fixed end; a loop closure 1-5; the pair 2-3 carries two edges"""
    rng = np.random.default_rng(seed)
    P = 6
    gt = np.array([icp_ref.random_pose(rng, rot=0.4) for _ in range(P)])
    pose = gt.copy()
    for i in range(1, P):
        pose[i] = PR.displaced(rng, gt[i], 0.3, 1.5)
    pf = np.zeros(P, np.uint8)
    pf[0] = 1
    pairs = [(i, i + 1) if i % 2 == 0 else (i + 1, i) for i in range(P - 1)] + [(1, 5), (3, 2)]
    return no_ba(pose, pf, gt), [], empty_prior(), edges_between(rng, gt, pairs, 0.01, 0.05, 10.0)


def gauge_case(seed=6):
    """no fixed pose, no landmark: a ring of 5 poses held by ONE prior (Omega = 1e4 I on pose 2 at its ground truth),
    Huber kernel on the relative-pose set"""
    rng = np.random.default_rng(seed)
    P = 5
    gt = np.array([icp_ref.random_pose(rng, rot=0.4) for _ in range(P)])
    pose = np.array([PR.displaced(rng, gt[i], 0.3, 1.5) for i in range(P)])
    pairs = [(i, (i + 1) % P) if i % 2 == 0 else ((i + 1) % P, i) for i in range(P)]
    rp = edges_between(rng, gt, pairs, 0.02, 0.1, 5.0, rk=(RR.RK_HUBER, 2.0))
    prior = PR.make_prior([2], gt[2][None], 1e4 * np.eye(6)[None])
    return no_ba(pose, np.zeros(P, np.uint8), gt), [], prior, rp


def mixed_case(seed=8):
    """a small BA problem (6 poses / 40 landmarks, pose 0 fixed) + plane, line, prior and relative-pose edges.  The
    relative-pose edges: odometry over the consecutive pairs (co-visible: their blocks carry products AND edge terms), a
    second edge on one of those pairs, the fixed end 0-1, and closures over pairs that share NO landmark (their blocks
    carry the edge term alone); Cauchy kernel.  Both kinds of pair are asserted from the co-visibility"""
    rng = np.random.default_rng(seed)
    d = synth.make_problem(n_poses=6, n_landmarks=40, seed=seed, fixed_poses=(0,), mean_obs=2.5)
    pl = icp_lm_ref.icp_edges(rng, d, [5, 12, 0, 9, 7, 4], "plane", 0.02)
    li = icp_lm_ref.icp_edges(rng, d, [2, 0, 5, 4, 0, 3], "line", 0.02)
    icp = [("plane", pl, rng.uniform(0.5, 2.0, len(pl["pose"])) * 2e3, np.ones(len(pl["pose"]), bool), (icp_ref.RK_HUBER, 4.0)),
           ("line", li, np.array([2.4e3]), np.ones(len(li["pose"]), bool), (icp_ref.RK_NONE, 1.0))]
    gt = d["pose_gt"]
    prior = PR.make_prior([3, 5], [PR.displaced(rng, gt[p], 0.01, 0.05) for p in (3, 5)],
                          [PR.random_spd(rng, 50.0) for _ in range(2)])
    pidx, _ = free_first(d)
    cov = covisible_pairs(d)
    far = [(a, b) for a in range(1, 6) for b in range(a + 1, 6)
           if (min(pidx[a], pidx[b]), max(pidx[a], pidx[b])) not in cov]
    assert len(far) >= 2, "the recipe needs pairs of free poses that share no landmark"
    pairs = [(i, i + 1) if i % 2 == 0 else (i + 1, i) for i in range(5)] + [(3, 2)] + [far[0], far[-1][::-1]]
    rp = edges_between(rng, gt, pairs, 0.005, 0.02, 200.0, rk=(RR.RK_CAUCHY, 5.0))
    joined = relpose_pairs(d, rp)
    assert joined & cov and joined - cov, "the recipe needs a pair with products and a pair without"
    return d, icp, prior, rp


def reject_case(seed=3):
    """icp_lm_ref.reject_case's BA part (the golden stress fixture reject_8x60: it takes rejected trials) + an odometry
    chain and two closures measured at the INITIAL poses"""
    d, _ = icp_lm_ref.reject_case(seed=seed)
    rng = np.random.default_rng(seed + 300)
    P = len(d["pose"])
    pairs = [(i, i + 1) if i % 2 == 0 else (i + 1, i) for i in range(P - 1)] + [(0, P - 1), (5, 2)]
    return d, [], empty_prior(), edges_between(rng, np.asarray(d["pose"]), pairs, 0.02, 0.1, 2.0)


CASES = {  # name -> (recipe, iterations)
    "chain": (chain_case, 4),
    "gauge": (gauge_case, 4),
    "mixed": (mixed_case, 8),
    "reject": (reject_case, 8),
}


_REF = {}


def reference(name):
    """(d, icp, prior, relpose, niter, reference trace, pose, lm, chi2 tolerances, estimate tolerance) of a case, with the
    conditions every case has to meet asserted on the reference alone"""
    if name not in _REF:
        recipe, niter = CASES[name]
        d, icp, prior, rp = recipe()
        tr, pose, lm, sens, est = reference_runs(d, icp, prior, rp, niter)
        assert len(tr) == niter, (name, len(tr))
        assert all(abs(t["rho"]) >= 0.1 for t in tr), "a decision at rho near 0 is not a fair comparison"
        if name == "reject":
            assert sum(t["trials"] for t in tr) >= 1, "the recipe no longer takes a rejected trial"
        print("reference %s: self-sensitivity %.3g (chi2), %.3g (estimates); trials %s" %
              (name, max(sens), est, [t["trials"] for t in tr]))
        tol, etol = icp_lm_ref.tolerances(sens, est)
        _REF[name] = (d, icp, prior, rp, niter, tr, pose, lm, tol, etol)
    return _REF[name]


# ---- the product's graph from a recipe ----------------------------------------------------------------------------
def add_relpose(g, rp, pose_ids=None):
    """the relative-pose edges of a recipe into a cugo Graph; inactive ones are left out (the C ABI adds active edges only)"""
    act = np.asarray(rp["active"], bool)
    ids = (lambda x: np.asarray(x, np.int32)) if pose_ids is None else (lambda x: np.asarray(pose_ids, np.int32)[x])
    info = np.broadcast_to(np.asarray(rp["info"], np.float64).reshape(-1, 6, 6), (len(act), 6, 6))
    g.add_relpose_edges(ids(rp["a"])[act], ids(rp["b"])[act], np.asarray(rp["z"])[act], info[act])
    rk = rp.get("rk", (RR.RK_NONE, 1.0))
    g.set_relpose_robust_kernel(rk[0], rk[1])


def build_graph(d, icp, prior, rp, rk=(0, 1.0), plan_only=False, per_edge_information=True):
    g = PR.build_graph(d, icp, prior, rk=rk, plan_only=plan_only, per_edge_information=per_edge_information)
    if rp is not None:
        add_relpose(g, rp)
    return g
