"""numpy restatement of the SE(3) pose priors (include/prior_types.h; an extension: the reference has no such edge) and
of the cugo_prior_edges layout of include/cugo_hip.h (numpy only, no product code).

Pose (q, t), quaternion (x, y, z, w), read as everywhere else (y = R(q) p + t); left update T <- Exp([w, v]) T in the
tangent order [w, v].  For a prior with measurement Z = (q_z, t_z) and information Omega (6 x 6):
    R_D = R(q) R(q_z)^T,  t_D = t - R_D t_z          (D = T Z^-1)
    r   = [phi; t_D],  phi = Log_SO3(R_D)
    J   = dr/dxi = [[J_l^-1(phi), 0], [-[t_D]x, I]],  J_l^-1 = I - [phi]x / 2 + c(theta) [phi]x^2
    c   = 1/theta^2 - (1 + cos theta) / (2 theta sin theta)   (1/12 + theta^2/720 for small theta)
    x = max(0, r^T Omega r), chi2 term rho(x), w = rho'(x), H = sum w J^T Omega J, b = -sum w J^T Omega r
b has the sign of the BA and ICP build passes (tests/icp_ref.py): minus half the gradient of chi2.
"""
import importlib

import numpy as np

import icp_lm_ref
import icp_ref
import synth

RK_NONE, RK_CAUCHY, RK_TUKEY, RK_HUBER = 0, 1, 2, 3
SMALL_THETA = 1e-3


def log_so3(R):
    """rotation vector of R, |phi| <= pi (not for use next to pi, where the log has its branch cut)"""
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.linalg.norm(v)
    c = 0.5 * (np.trace(R) - 1.0)
    theta = np.arctan2(s, c)
    return (theta / s if s > 1e-12 else 1.0) * v


def inv_left_jacobian(phi):
    theta = np.linalg.norm(phi)
    if theta < SMALL_THETA:
        c = 1.0 / 12 + theta * theta / 720
    else:
        c = 1.0 / theta ** 2 - (1.0 + np.cos(theta)) / (2.0 * theta * np.sin(theta))
    K = icp_ref.skew(phi)
    return np.eye(3) - 0.5 * K + c * K @ K


def residual(pose7, z7):
    RD = synth.quat_to_R(pose7[:4]) @ synth.quat_to_R(z7[:4]).T
    return np.concatenate([log_so3(RD), pose7[4:] - RD @ z7[4:]])


def jacobian(pose7, z7):
    r = residual(pose7, z7)
    J = np.eye(6)
    J[:3, :3] = inv_left_jacobian(r[:3])
    J[3:, :3] = -icp_ref.skew(r[3:])
    return J


def pack_info(Om):
    """[..., 6, 6] -> [..., 21]: the upper triangle, row-major packed (the layout of cugo_prior_edges::d_info)"""
    iu = np.triu_indices(6)
    return np.asarray(Om)[..., iu[0], iu[1]]


def edge_terms(pose7, z7, Om, rk):
    """(chi2 term, H 6x6, b 6) of one prior"""
    r, J = residual(pose7, z7), jacobian(pose7, z7)
    x = max(0.0, float(r @ Om @ r))
    w = icp_ref.drho(rk[0], rk[1], x)
    return icp_ref.rho(rk[0], rk[1], x), w * J.T @ Om @ J, -w * J.T @ Om @ r


def reference_build(poses, n_free, pr):
    """pr: dict pose [E] (free-first index), z [E,7], info [E,6,6] or [1,6,6], active [E] bool, rk (type, delta).
    Per free pose H [P,6,6], b [P,6], the chi2 total and the chi2 term of every edge (0 where it does not count).
    Vectorised over the edges."""
    pose = np.asarray(pr["pose"], int)
    E = len(pose)
    H = np.zeros((n_free, 6, 6))
    b = np.zeros((n_free, 6))
    if E == 0:
        return H, b, 0.0, np.zeros(0)
    z = np.asarray(pr["z"], np.float64).reshape(E, 7)
    Om = np.broadcast_to(np.asarray(pr["info"], np.float64).reshape(-1, 6, 6), (E, 6, 6))
    rk = pr.get("rk", (RK_NONE, 1.0))
    R = np.array([synth.quat_to_R(q[:4]) for q in poses])[pose]
    Rz = np.array([synth.quat_to_R(q[:4]) for q in z])
    D = np.einsum("eij,ekj->eik", R, Rz)
    v = 0.5 * np.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], axis=1)
    s = np.linalg.norm(v, axis=1)
    c = 0.5 * (np.einsum("eii->e", D) - 1.0)
    theta = np.arctan2(s, c)
    phi = np.where(s > 1e-12, theta / np.where(s > 1e-12, s, 1.0), 1.0)[:, None] * v
    tD = poses[pose, 4:] - np.einsum("eij,ej->ei", D, z[:, 4:])
    r = np.concatenate([phi, tD], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        cc = np.where(theta < SMALL_THETA, 1.0 / 12 + theta * theta / 720,
                      1.0 / theta ** 2 - (1.0 + c) / (2.0 * theta * s))

    def skews(a):
        K = np.zeros((len(a), 3, 3))
        K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -a[:, 2], a[:, 1], a[:, 2]
        K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -a[:, 0], -a[:, 1], a[:, 0]
        return K
    K = skews(phi)
    J = np.zeros((E, 6, 6))
    J[:, :3, :3] = np.eye(3)[None] - 0.5 * K + cc[:, None, None] * np.einsum("eij,ejk->eik", K, K)
    J[:, 3:, :3] = -skews(tD)
    J[:, 3:, 3:] = np.eye(3)[None]
    Or = np.einsum("eij,ej->ei", Om, r)
    x = np.maximum(0.0, np.einsum("ei,ei->e", r, Or))
    ce = icp_ref._rho_vec(rk, x)
    w = icp_ref._drho_vec(rk, x)
    keep = (pose < n_free) & np.asarray(pr["active"], bool)
    ce = np.where(keep, ce, 0.0)
    w = np.where(keep, w, 0.0)
    h = np.einsum("e,eki,ekl,elj->eij", w, J, Om, J)
    g = -np.einsum("e,eki,ek->ei", w, J, Or)
    np.add.at(H, pose[keep], h[keep])
    np.add.at(b, pose[keep], g[keep])
    return H, b, float(ce.sum()), ce


# ------------------------------------------------------------------ device layout -----------
def sort_by_pose(pr):
    order = np.argsort(pr["pose"], kind="stable")
    out = {}
    for k, v in pr.items():
        if k == "rk" or (k == "info" and len(v) == 1):
            out[k] = v
        else:
            out[k] = np.asarray(v)[order]
    return out, order


def upload(ctx, n_poses_total, n_free, pr):
    """cugo_prior_edges over a sorted prior dict (pose, z, info [E or 1, 6, 6], optional flags, rk)"""
    cugo = importlib.import_module("cuda-bundle-adjustment_amd")
    ev = cugo.PriorEdges()
    n = len(pr["pose"])
    ev.n_poses_total, ev.n_poses_free, ev.n = n_poses_total, n_free, n
    ev.d_pose = ctx.to_dev(np.asarray(pr["pose"], np.int32))
    ev.d_pose_ptr = ctx.to_dev(icp_ref.pose_ptr(np.asarray(pr["pose"], np.int32), n_poses_total))
    ev.d_meas = ctx.to_dev(np.ascontiguousarray(np.asarray(pr["z"], np.float64).reshape(n, 7).T))
    info = pack_info(np.asarray(pr["info"], np.float64).reshape(-1, 6, 6))
    ev.d_info = ctx.to_dev(np.ascontiguousarray(info.T))
    ev.n_info = len(info)
    if pr.get("flags") is not None:
        ev.d_flags = ctx.to_dev(np.asarray(pr["flags"], np.uint8))
    rk = pr.get("rk", (RK_NONE, 1.0))
    ev.rk, ev.delta = rk[0], rk[1]
    return ev


# ------------------------------------------------------------------ the LM reference ----------
class PriorGraph(icp_lm_ref.IcpGraph):
    """IcpGraph + pose priors.  prior: dict pose (position in d['pose']), z [E,7], info [E,6,6] or [1,6,6],
    active [E] bool, rk"""

    def __init__(self, d, icp, prior, rk=(0, 1.0), via_schur=True):
        super().__init__(d, icp, rk, via_schur)
        self.prior = prior

    def _prior(self):
        poses = self.pose[np.argsort(self.pidx)]
        pr = dict(self.prior, pose=self.pidx[np.asarray(self.prior["pose"], int)])
        return reference_build(poses, self.np_, pr)

    def chi2(self):
        return super().chi2() + self._prior()[2]

    def normal_equations(self):
        H, b = super().normal_equations()
        Hi, bi, _, _ = self._prior()
        for p in range(self.np_):
            H[6 * p:6 * p + 6, 6 * p:6 * p + 6] += Hi[p]
            b[6 * p:6 * p + 6] += bi[p]
        return H, b


def permuted_prior(prior, seed=98):
    perm = np.random.default_rng(seed).permutation(len(prior["pose"]))
    out = dict(prior)
    for k in ("pose", "z", "active"):
        out[k] = np.asarray(prior[k])[perm]
    if len(prior["info"]) > 1:
        out["info"] = np.asarray(prior["info"])[perm]
    return out


def reference_runs(d, icp, prior, niter, rk=(0, 1.0)):
    """as icp_lm_ref.reference_runs: the trajectory, the final estimates and what the reference differs by from itself
    (Schur solve against the full dense solve; ICP edges and priors in a permuted order)"""
    runs = []
    for icp_k, pr_k, vs in ((icp, prior, True), (icp, prior, False), (icp_lm_ref.permuted(icp), permuted_prior(prior), True)):
        g = PriorGraph(d, icp_k, pr_k, rk, via_schur=vs)
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


# ------------------------------------------------------------------ input recipes ----------
def random_spd(rng, scale=1.0):
    """a dense, well-conditioned 6 x 6 information matrix"""
    A = rng.normal(size=(6, 6))
    return scale * (A @ A.T + 6 * np.eye(6))


def displaced(rng, pose7, rot=0.05, trans=0.3):
    return icp_ref.left_update(pose7, np.concatenate([rng.normal(0, rot, 3), rng.normal(0, trans, 3)]))


def make_prior(pose, z, info, rk=(RK_NONE, 1.0), active=None):
    pose = np.asarray(pose, np.int32)
    return dict(pose=pose, z=np.asarray(z, np.float64).reshape(len(pose), 7),
                info=np.asarray(info, np.float64).reshape(-1, 6, 6),
                active=np.ones(len(pose), bool) if active is None else np.asarray(active, bool), rk=rk)


def gauge_case(seed=5):
    """no fixed pose: 10 poses / 120 landmarks with a loop closure, the gauge held by Omega = 1e6 I on pose 0 at its ground
    truth, plus three dense-Omega priors (two on pose 3, one on pose 7) displaced by N(0, 0.05) rad and N(0, 0.3)"""
    d = synth.make_problem(10, 120, seed=seed, fixed_poses=(), loop_closure=True)
    rng = np.random.default_rng(seed)
    gt = d["pose_gt"]
    pose = [0, 3, 3, 7]
    z = [gt[0]] + [displaced(rng, gt[p]) for p in pose[1:]]
    info = [1e6 * np.eye(6)] + [random_spd(rng) for _ in pose[1:]]
    return d, [], make_prior(pose, z, info)


def mixed_prior_case(seed=5):
    """icp_lm_ref.mixed_case (BA + plane + line, pose 0 fixed) + priors: one on the fixed pose (counts for nothing), two on
    pose 4, one each on poses 1, 6, 9, dense Omega, Huber"""
    d, icp = icp_lm_ref.mixed_case(seed=seed)
    rng = np.random.default_rng(seed + 100)
    gt = d["pose_gt"]
    pose = [0, 4, 1, 4, 6, 9]
    z = [displaced(rng, gt[p], 0.01, 0.05) for p in pose]
    info = [random_spd(rng, 50.0) for _ in pose]
    return d, icp, make_prior(pose, z, info, rk=(RK_HUBER, 3.0))


def reject_prior_case(seed=3):
    """icp_lm_ref.reject_case (it takes rejected trials) + one prior per free pose displaced from the INITIAL poses"""
    d, icp = icp_lm_ref.reject_case(seed=seed)
    rng = np.random.default_rng(seed + 200)
    free = np.nonzero(np.asarray(d["pose_fixed"]) == 0)[0]
    z = [displaced(rng, d["pose"][p], 0.02, 0.1) for p in free]
    info = [random_spd(rng, 2.0) for _ in free]
    return d, icp, make_prior(free, z, info)


def corridor_case(seed=9, P=5):
    """no landmarks; every plane normal is perpendicular to the x axis, so the planes leave the x translation of every
    pose unobserved; one weak dense-Omega prior per free pose observes it (the last pose is fixed)"""
    rng = np.random.default_rng(seed)
    gt = np.array([icp_ref.random_pose(rng, rot=0.3) for _ in range(P)])
    pose = gt.copy()
    for i in range(P - 1):
        pose[i] = displaced(rng, gt[i], 0.05, 0.3)
    pf = np.zeros(P, np.uint8)
    pf[P - 1] = 1
    d = dict(pose=pose, pose_fixed=pf, lm=np.zeros((0, 3)), lm_fixed=np.zeros(0, np.uint8),
             e_pose=np.zeros(0, np.int32), e_lm=np.zeros(0, np.int32), e_stereo=np.zeros(0, np.uint8),
             e_meas=np.zeros((0, 3)), e_omega=np.zeros(0), e_cam=np.zeros((0, 5)), pose_gt=gt)
    per_pose = [40, 35, 50, 30, 20][:P]
    pl = icp_lm_ref.icp_edges(rng, d, per_pose, "plane", 0.01)
    n = pl["n"].copy()
    n[:, 0] = 0.0
    n /= np.linalg.norm(n, axis=1)[:, None]
    y = np.array([icp_ref.transform(gt[q], p) for q, p in zip(pl["pose"], pl["p"])])
    pl["n"], pl["d"] = n, np.einsum("ij,ij->i", n, y) + rng.normal(0, 0.01, len(n))
    icp = [("plane", pl, np.array([100.0]), np.ones(len(n), bool), (icp_ref.RK_NONE, 1.0))]
    free = np.arange(P - 1)
    z = [displaced(rng, gt[p], 0.02, 0.2) for p in free]
    info = [random_spd(rng, 0.05) for _ in free]
    return d, icp, make_prior(free, z, info)


CASES = {  # name -> (recipe, iterations)
    "gauge": (gauge_case, 8),
    "mixed": (mixed_prior_case, 8),
    "reject": (reject_prior_case, 8),
    "corridor": (corridor_case, 4),
}


# ---- the product's graph from a recipe ----------------------------------------------------------------------------
def add_priors(g, prior, pose_ids=None):
    """the priors of a recipe into a cugo Graph; inactive ones are left out (the C ABI adds active edges only)"""
    act = np.asarray(prior["active"], bool)
    ids = np.asarray(prior["pose"], np.int32) if pose_ids is None else np.asarray(pose_ids, np.int32)[prior["pose"]]
    info = np.broadcast_to(np.asarray(prior["info"], np.float64).reshape(-1, 6, 6), (len(act), 6, 6))
    g.add_pose_priors(ids[act], np.asarray(prior["z"])[act], info[act])
    rk = prior.get("rk", (RK_NONE, 1.0))
    g.set_prior_robust_kernel(rk[0], rk[1])


def build_graph(d, icp, prior, rk=(0, 1.0), plan_only=False, per_edge_information=True):
    g = icp_lm_ref.build_graph(d, icp, rk=rk, plan_only=plan_only, per_edge_information=per_edge_information)
    if prior is not None:
        add_priors(g, prior)
    return g
