"""Reference for graphs that hold point-to-plane / point-to-line edge sets next to (or instead of) BA edges: the dense
numpy LM of tests/golden/make_golden.py plus tests/icp_ref.reference_build for the ICP terms (numpy only, no product
code), the input recipes of tests/test_icp_graph*.py, and the reference's own round-off sensitivity.

Both files use the sign of the BA build pass: b is minus half the gradient of chi2.  ICP pose indices are positions in
d["pose"]; Graph.pidx maps them to the free-first index.
"""
import importlib
import os
import sys

import numpy as np

import icp_ref
import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden as mg  # noqa: E402


class IcpGraph(mg.Graph):
    """make_golden.Graph + unary ICP edges.
    icp: list of (kind, edges dict with pose = position in d['pose'], omega [E] or [1], active [E] bool, (rk type, delta))"""

    def __init__(self, d, icp, rk=(0, 1.0), via_schur=True):
        super().__init__(d, rk)
        self.icp, self.via_schur = icp, via_schur

    def _icp(self):
        poses = self.pose[np.argsort(self.pidx)]                 # free-first order, as reference_build indexes
        kinds = [(k, {**e, "pose": self.pidx[np.asarray(e["pose"])]}, om, act, rk) for k, e, om, act, rk in self.icp]
        return icp_ref.reference_build(poses, self.np_, kinds)   # H [P,6,6], b [P,6], chi2, per-edge chi2

    def chi2(self):
        return super().chi2() + self._icp()[2]

    def normal_equations(self):
        H, b = super().normal_equations()
        Hi, bi, _, _ = self._icp()
        for p in range(self.np_):
            H[6 * p:6 * p + 6, 6 * p:6 * p + 6] += Hi[p]
            b[6 * p:6 * p + 6] += bi[p]                          # same sign in both files: minus half the gradient
        return H, b

    def solve(self, H, b, lam, via_schur=True):
        return super().solve(H, b, lam, self.via_schur)           # False: the full dense solve (self-sensitivity)


def trace_dicts(trace):
    return [dict(iteration=int(t[0]), chi2=float(t[1]), lam=float(t[2]), rho=float(t[3]), trials=int(t[4])) for t in trace]


def permuted(icp, seed=99):
    rng = np.random.default_rng(seed)
    out = []
    for kind, e, om, act, rk in icp:
        perm = rng.permutation(len(e["pose"]))
        out.append((kind, {k: v[perm] for k, v in e.items()}, om[perm] if len(om) > 1 else om, act[perm], rk))
    return out


def reference_runs(d, icp, niter, rk=(0, 1.0)):
    """The reference trajectory, its final estimates, and what the reference differs by FROM ITSELF: its Schur solve
    against its full dense solve, and the ICP edges in a permuted order.  Returns (trace dicts, pose, lm, per-iteration
    relative chi2 sensitivity, sensitivity of the final estimates)."""
    runs = []
    for icp_k, vs in ((icp, True), (icp, False), (permuted(icp), True)):
        g = IcpGraph(d, icp_k, rk, via_schur=vs)
        runs.append((g.optimize(niter), g.pose.copy(), g.lm.copy()))
    tr = runs[0][0]
    sens = [0.0] * len(tr)
    est = 0.0
    for t2, pose2, lm2 in runs[1:]:
        assert [t[4] for t in t2] == [t[4] for t in tr], "the reference disagrees with itself on the trial counts"
        for i in range(len(tr)):
            sens[i] = max(sens[i], abs(tr[i][1] - t2[i][1]) / abs(tr[i][1]))
        est = max(est, float(np.abs(runs[0][1] - pose2).max()), float(np.abs(runs[0][2] - lm2).max()) if len(lm2) else 0.0)
    return trace_dicts(tr), runs[0][1], runs[0][2], sens, est


def tolerances(sens, est):
    """the rule of conftest.golden_tolerances: max(1e-10, 4 x self-sensitivity) per iteration; estimates max(1e-9, 4 x)"""
    return [max(1e-10, 4.0 * s) for s in sens], max(1e-9, 4.0 * est)


# ---- input recipes ---------------------------------------------------------------------------------------------
def icp_edges(rng, d, per_pose, kind, noise, gt=None):
    pose_of_edge = np.concatenate([np.full(per_pose[k], k, np.int32) for k in range(len(d["pose"]))])
    rng.shuffle(pose_of_edge)
    return icp_ref.make_edges(rng, pose_of_edge, kind, d["pose_gt"] if gt is None else gt, noise=noise)


def mixed_case(pose_noise=(0.01, 0.05), seed=5, om_scale=2e4, delta_pl=4.0, delta_li=6.0):
    """10 poses / 120 landmarks with a loop closure + 169 plane (Huber, per-edge omega, 10 % inactive) + 37 line edges
    (Cauchy, one omega).  Poses 5 and 9 have no ICP edge, pose 2 only line edges, the fixed pose 0 has 31."""
    rng = np.random.default_rng(seed)
    d = synth.make_problem(n_poses=10, n_landmarks=120, seed=seed, fixed_poses=(0,), loop_closure=True,
                           pose_noise=pose_noise)
    pl = icp_edges(rng, d, [25, 30, 0, 40, 12, 0, 33, 8, 21, 0], "plane", 0.02)
    li = icp_edges(rng, d, [6, 0, 9, 10, 0, 0, 7, 5, 0, 0], "line", 0.02)
    om_pl = rng.uniform(0.5, 2.0, len(pl["pose"])) * om_scale
    om_li = np.array([1.2 * om_scale])
    act_pl = rng.random(len(pl["pose"])) >= 0.1
    act_li = np.ones(len(li["pose"]), bool)
    return d, [("plane", pl, om_pl, act_pl, (icp_ref.RK_HUBER, delta_pl)), ("line", li, om_li, act_li, (icp_ref.RK_CAUCHY, delta_li))]


def icp_only_case(seed=7, rot=0.6, tr=2.0, P=6):
    """6 poses (the last fixed), no landmarks: 285 plane (one omega, no kernel) + 42 line edges (per-edge omega, Huber)"""
    rng = np.random.default_rng(seed)
    gt = np.array([icp_ref.random_pose(rng) for _ in range(P)])
    pose = gt.copy()
    for i in range(P - 1):
        pose[i] = icp_ref.left_update(gt[i], np.concatenate([rng.normal(0, rot, 3), rng.normal(0, tr, 3)]))
    pf = np.zeros(P, np.uint8)
    pf[P - 1] = 1
    d = dict(pose=pose, pose_fixed=pf, lm=np.zeros((0, 3)), lm_fixed=np.zeros(0, np.uint8),
             e_pose=np.zeros(0, np.int32), e_lm=np.zeros(0, np.int32), e_stereo=np.zeros(0, np.uint8),
             e_meas=np.zeros((0, 3)), e_omega=np.zeros(0), e_cam=np.zeros((0, 5)), pose_gt=gt)
    pl = icp_edges(rng, d, [60, 45, 80, 30, 50, 20], "plane", 0.01)
    li = icp_edges(rng, d, [10, 0, 15, 12, 0, 5], "line", 0.01)
    icp = [("plane", pl, np.array([1.0]), np.ones(len(pl["pose"]), bool), (icp_ref.RK_NONE, 1.0)),
           ("line", li, rng.uniform(0.5, 2, len(li["pose"])), np.ones(len(li["pose"]), bool), (icp_ref.RK_HUBER, 0.5))]
    return d, icp


def reject_case(om=3.0, seed=3, noise=0.05):
    """the golden stress fixture reject_8x60 (it takes rejected trials) + 122 plane (Huber 1, one omega) + 26 line
    edges (per-edge omega) placed at the INITIAL poses"""
    g8 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reject_8x60.npz"))
    d = {k: g8[k] for k in g8.files}
    rng = np.random.default_rng(seed)
    pl = icp_edges(rng, d, [20, 0, 30, 25, 10, 0, 15, 22], "plane", noise, gt=d["pose"])
    li = icp_edges(rng, d, [5, 6, 0, 8, 0, 0, 4, 3], "line", noise, gt=d["pose"])
    icp = [("plane", pl, np.array([om]), np.ones(len(pl["pose"]), bool), (icp_ref.RK_HUBER, 1.0)),
           ("line", li, rng.uniform(0.5, 2, len(li["pose"])) * om, np.ones(len(li["pose"]), bool), (icp_ref.RK_NONE, 1.0))]
    return d, icp


CASES = {  # name -> (recipe, iterations, rejected trials per iteration the reference takes)
    "mixed": (mixed_case, 8, [0] * 8),
    "mixed_far": (lambda: mixed_case(pose_noise=(0.08, 0.5)), 10, [0] * 10),
    "icp_only": (icp_only_case, 3, [0] * 3),
    "reject": (reject_case, 8, [2, 0, 0, 0, 1, 0, 0, 0]),
}


# ---- the product's graph from a recipe ----------------------------------------------------------------------------
def add_icp(g, icp, pose_ids=None):
    """the ICP sets of a recipe into a cugo Graph; inactive edges are left out (the C ABI adds active edges only)"""
    cugo = importlib.import_module("cuda-bundle-adjustment_amd")
    for kind, e, om, act, rk in icp:
        act = np.asarray(act, bool)
        ids = np.asarray(e["pose"], np.int32) if pose_ids is None else np.asarray(pose_ids, np.int32)[e["pose"]]
        w = np.broadcast_to(np.asarray(om, np.float64), (len(act),))[act]
        if kind == "plane":
            g.add_plane_edges(ids[act], e["p"][act], e["n"][act], e["d"][act], w)
            code = cugo.ICP_PLANE
        else:
            g.add_line_edges(ids[act], e["p"][act], e["a"][act], e["b"][act], w)
            code = cugo.ICP_LINE
        g.set_icp_robust_kernel(code, rk[0], rk[1])
        if len(w):
            g.set_icp_information(code, float(w[0]))


def build_graph(d, icp, rk=(0, 1.0), plan_only=False, per_edge_information=True):
    cugo = importlib.import_module("cuda-bundle-adjustment_amd")
    g = cugo.graph_from_arrays(d, per_edge_information=per_edge_information, rk=rk, plan_only=plan_only)
    add_icp(g, icp)
    return g


# ---- block-diagonal LM for graphs of ICP edges only (no landmarks): per-pose 6 x 6 solves, vectorised ---------------
def icp_only_lm(d, icp, niter):
    """the LM control of make_golden.Graph.optimize on a system that is block-diagonal (no landmarks, no BA edges):
    reference_build for the terms, one batched 6 x 6 solve per trial, the base class's expm update"""
    g = IcpGraph(d, icp)
    assert g.nl == 0 and not g.active.any()
    maxq, tau = 10, 1e-5
    nu, lam = 2.0, 0.0
    trace = []
    for it in range(niter):
        H, b, F, _ = g._icp()
        if it == 0:
            lam = tau * max(0.0, np.einsum("pii->pi", H).max())
        q, rho_ = 0, -1.0
        while q < maxq and rho_ < 0:
            bak = g.pose.copy()
            ok = True
            try:
                Hd = H + lam * np.eye(6)[None]
                np.linalg.cholesky(Hd)
                dx = np.linalg.solve(Hd, b[:, :, None])[:, :, 0]
                g.apply(dx.reshape(-1))
            except np.linalg.LinAlgError:
                ok, dx = False, np.zeros_like(b)
            Fhat = g._icp()[2]
            scale = float((dx * (lam * dx + b)).sum()) + 1e-3
            rho_ = (F - Fhat) / scale if ok else -1.0
            if rho_ > 0:
                lam *= min(max(1 - (2 * rho_ - 1) ** 3, 1 / 3), 2 / 3)
                nu = 2.0
                F = Fhat
                break
            lam *= nu
            nu *= 2
            g.pose = bak
            if not np.isfinite(lam) or (ok and Fhat - F < 1e-4):
                break
            q += 1
        trace.append((it, F, lam, rho_, q))
        if q == maxq or rho_ < 1e-6 or not np.isfinite(lam):
            break
    return trace_dicts(trace), g.pose.copy()
