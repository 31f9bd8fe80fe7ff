"""Reference of the landmark position priors (landmark_prior_types.h, lm_prior_term.h), numpy only, no product code.

The term.  Landmark estimate X, measurement Z, information Omega (3 x 3, symmetric, positive semi-definite):
    r = X - Z,  J = I,  x = max(0, r^T Omega r),  chi2 term rho(x),  w = rho'(x),  Hll += w Omega,  bl -= w Omega r
with the sign of the BA build pass (b is minus half the gradient of chi2).

reference_build evaluates it in np.longdouble with the per-entry bounds (n + c) u sum|terms| of tests/kernel_ref.py,
whose conventions it follows: a difference a - b has the mass |a| + |b|, the residual's mass is ADDED to |r| wherever r
enters a product, and the error of x enters the weight through rho''.  c per output, on the longest path of the formula:
    r_i = X_i - Z_i                      1, mass |X_i| + |Z_i|
    q_i = sum_j Omega_ij r_j             r 1, product 1, 2 additions                               ->  4
    x   = sum_i r_i q_i                  r 1, q 4, product 1, 2 additions                          ->  8
    w   = rho'(x)                        x 8 (through rho'', carried by the mass), rho' 6         -> 14
    Hll += w Omega_ij                    14, product 1                                             -> C_HLL = 15
    bl  -= w q_i                         14, q 4, product 1                                        -> C_BL  = 19
    chi += rho(x)                        x 8, rho 6                                                -> C_CHI = 14
Summed behind the BA terms of a landmark the constants are the larger BA ones (kernel_ref.C_HLL, C_BL, C_CHI) over the
joint count and the joint mass: combined().

LmPriorGraph is the dense numpy LM of tests/golden/make_golden.py (through prior_ref.PriorGraph, so that ICP sets and
pose priors can sit in the same graph) with the term added to Hll, bl and chi2.
"""
import numpy as np

import icp_lm_ref
import kernel_ref as kr
import prior_ref

LD = kr.LD
C_HLL, C_BL, C_CHI = 15, 19, 14
RK_NONE, RK_CAUCHY, RK_TUKEY, RK_HUBER = 0, 1, 2, 3


def make_prior(lm, z, info, rk=(RK_NONE, 1.0), active=None):
    """lm: landmark per prior (a position in d['lm'] for the graph level, a flattened index for the kernel level),
    z [n,3], info [n,3,3] or [1,3,3]"""
    lm = np.asarray(lm, np.int32)
    return dict(lm=lm, z=np.asarray(z, np.float64).reshape(len(lm), 3), info=np.asarray(info, np.float64).reshape(-1, 3, 3),
                active=np.ones(len(lm), bool) if active is None else np.asarray(active, bool), rk=rk)


def edge_terms(X, Z, info, rk, dtype=np.float64):
    """one prior: (chi2 term, w Omega [3,3], -w Omega r [3])"""
    dt = dtype
    r = np.asarray(X, dt) - np.asarray(Z, dt)
    Om = np.asarray(info, dt)
    q = Om @ r
    x = max(dt(0), r @ q)
    rho, w, _ = kr._rho(int(rk[0]), rk[1], np.asarray([x], dt), dt)
    return rho[0], w[0] * Om, -w[0] * q


def reference_build(lms, L, pr, dtype=LD):
    """Hll [L,3,3], bl [L,3], chi and the chi2 term of every prior (0 where it does not count) of the priors `pr` on the
    landmarks lms [Lall,3] (flattened order; pr['lm'] indexes it; index >= L: a fixed landmark), with X_mass and X_n of
    each.  Priors of a landmark are summed in the order they are given."""
    dt = dtype
    lm = np.asarray(pr["lm"], int)
    n = len(lm)
    counts = np.asarray(pr["active"], bool) & (lm < L)
    X = np.asarray(lms, dt)[lm]
    Z = np.asarray(pr["z"], dt)
    Om = np.broadcast_to(np.asarray(pr["info"], dt), (n, 3, 3))
    r = X - Z
    rb = np.abs(r) + np.abs(X) + np.abs(Z)
    q = np.einsum("nij,nj->ni", Om, r)
    qm = np.einsum("nij,nj->ni", np.abs(Om), rb)
    x = np.maximum(dt(0), (r * q).sum(1))
    xm = (rb * qm).sum(1)
    rho, w, d2 = kr._rho(int(pr["rk"][0]), pr["rk"][1], x, dt)
    live = counts.astype(dt)
    w, aw = live * w, live * (w + d2 * xm)
    tH, mH = w[:, None, None] * Om, aw[:, None, None] * np.abs(Om)
    tb, mb = -w[:, None] * q, aw[:, None] * qm
    sel = np.flatnonzero(counts)
    cnt = np.bincount(lm[sel], minlength=L)[:L]
    return dict(Hll=kr._scatter(lm[sel], tH[sel], L), Hll_mass=kr._scatter(lm[sel], mH[sel], L), Hll_n=cnt[:, None, None],
                bl=kr._scatter(lm[sel], tb[sel], L), bl_mass=kr._scatter(lm[sel], mb[sel], L), bl_n=cnt[:, None],
                chi=(live * rho).sum(), chi_mass=(live * (np.abs(rho) + xm)).sum(), chi_n=int(counts.sum()),
                edge_chi=live * rho, edge_chi_mass=live * (np.abs(rho) + xm), w=w, x=x, counts=counts)


def bounds(ref):
    """the per-entry bounds of the stand-alone entries"""
    return dict(Hll=kr.bound(ref["Hll_n"], C_HLL, ref["Hll_mass"]), bl=kr.bound(ref["bl_n"], C_BL, ref["bl_mass"]),
                chi=kr.bound(ref["chi_n"], C_CHI, ref["chi_mass"]), edge_chi=kr.bound(1, C_CHI, ref["edge_chi_mass"]))


def combined(ba, pr):
    """Hll, bl and chi of a BA build (kernel_ref.build) with the priors' terms (reference_build) summed behind them, and
    their bounds: the joint count, the larger (BA) constant, the joint mass"""
    out = {}
    for k, c in (("Hll", kr.C_HLL), ("bl", kr.C_BL), ("chi", kr.C_CHI)):
        out[k] = ba[k] + pr[k]
        out[k + "_bound"] = kr.bound(np.asarray(ba[k + "_n"]) + np.asarray(pr[k + "_n"]), max(c, dict(Hll=C_HLL, bl=C_BL, chi=C_CHI)[k]),
                                     ba[k + "_mass"] + pr[k + "_mass"])
    return out


def sort_by_landmark(pr, Lall):
    """the device layout of `pr` (flattened landmark indices): stable sort by landmark, CSR over all landmarks, planar
    measurements, the upper triangle of Omega row-major packed (planar, [6][n] or [6][1]), flag bytes (8 = inactive).
    Returns (order, dict lm, lm_ptr, meas [3,n], info [6,n_info], flags)"""
    lm = np.asarray(pr["lm"], np.int32)
    order = np.argsort(lm, kind="stable")
    ptr = np.zeros(Lall + 1, np.int32)
    np.add.at(ptr, lm + 1, 1)
    info = np.asarray(pr["info"], np.float64)
    if len(info) > 1:
        info = info[order]
    tri = np.stack([info[:, 0, 0], info[:, 0, 1], info[:, 0, 2], info[:, 1, 1], info[:, 1, 2], info[:, 2, 2]], 0)
    return order, dict(lm=lm[order], lm_ptr=np.cumsum(ptr).astype(np.int32), meas=np.ascontiguousarray(np.asarray(pr["z"])[order].T),
                       info=np.ascontiguousarray(tri), flags=np.where(np.asarray(pr["active"], bool)[order], 0, 8).astype(np.uint8))


# ------------------------------------------------------------------ the LM reference ----------
def no_pose_prior():
    return prior_ref.make_prior(np.zeros(0, np.int32), np.zeros((0, 7)), np.eye(6)[None])


class LmPriorGraph(prior_ref.PriorGraph):
    """make_golden.Graph (+ ICP sets and pose priors) + landmark priors.  lmp: make_prior() with lm = positions in
    d['lm']"""

    def __init__(self, d, lmp, icp=(), prior=None, rk=(0, 1.0), via_schur=True):
        super().__init__(d, list(icp), no_pose_prior() if prior is None else prior, rk, via_schur)
        self.lmp = lmp

    def _lmp(self):
        lms = self.lm[np.argsort(self.lidx)]   # free-first order
        pr = dict(self.lmp, lm=self.lidx[np.asarray(self.lmp["lm"], int)])
        return reference_build(lms, self.nl, pr, dtype=np.float64)

    def chi2(self):
        return super().chi2() + float(self._lmp()["chi"])

    def normal_equations(self):
        H, b = super().normal_equations()
        t = self._lmp()
        for l in range(self.nl):
            c = 6 * self.np_ + 3 * l
            H[c:c + 3, c:c + 3] += t["Hll"][l]
            b[c:c + 3] += t["bl"][l]
        return H, b


def permuted(lmp, seed=97):
    perm = np.random.default_rng(seed).permutation(len(lmp["lm"]))
    out = dict(lmp)
    for k in ("lm", "z", "active"):
        out[k] = np.asarray(lmp[k])[perm]
    if len(lmp["info"]) > 1:
        out["info"] = np.asarray(lmp["info"])[perm]
    return out


def reference_runs(d, lmp, niter, icp=(), prior=None, rk=(0, 1.0)):
    """as icp_lm_ref.reference_runs: the trajectory, the final estimates and what the reference differs by from itself
    (its Schur solve against its full dense solve; the landmark priors in a permuted order)"""
    runs = []
    for lmp_k, vs in ((lmp, True), (lmp, False), (permuted(lmp), True)):
        g = LmPriorGraph(d, lmp_k, icp, prior, rk, via_schur=vs)
        runs.append((g.optimize(niter), g.pose.copy(), g.lm.copy()))
    tr = runs[0][0]
    sens, est = [0.0] * len(tr), 0.0
    for t2, pose2, lm2 in runs[1:]:
        assert [t[4] for t in t2] == [t[4] for t in tr], "the reference disagrees with itself on the trial counts"
        for i in range(len(tr)):
            sens[i] = max(sens[i], abs(tr[i][1] - t2[i][1]) / abs(tr[i][1]))
        est = max(est, float(np.abs(runs[0][1] - pose2).max()), float(np.abs(runs[0][2] - lm2).max()))
    return icp_lm_ref.trace_dicts(tr), runs[0][1], runs[0][2], sens, est


def random_spd3(rng, scale=1.0):
    A = rng.normal(size=(3, 3))
    return scale * (A @ A.T + 3 * np.eye(3))


# ---- the product's graph from a recipe ----------------------------------------------------------------------------
def add_lm_priors(g, lmp):
    """the landmark priors of a recipe into a cugo Graph; inactive ones are left out (the C ABI adds active edges only)"""
    act = np.asarray(lmp["active"], bool)
    info = np.broadcast_to(np.asarray(lmp["info"], np.float64).reshape(-1, 3, 3), (len(act), 3, 3))
    g.add_landmark_priors(np.asarray(lmp["lm"], np.int32)[act], np.asarray(lmp["z"])[act], info[act])
    g.set_landmark_prior_robust_kernel(lmp["rk"][0], lmp["rk"][1])


def build_graph(d, lmp, icp=(), prior=None, rk=(0, 1.0), plan_only=False, per_edge_information=True):
    g = prior_ref.build_graph(d, list(icp), prior, rk=rk, plan_only=plan_only, per_edge_information=per_edge_information)
    if lmp is not None:
        add_lm_priors(g, lmp)
    return g


# ------------------------------------------------------------------ input recipes ----------
# each returns (d, landmark priors, icp kinds, pose priors or None); graphs of about 8 poses x 80 landmarks, the size of
# the goldens
def _observed(d):
    act = ~((np.asarray(d["pose_fixed"])[d["e_pose"]] != 0) & (np.asarray(d["lm_fixed"])[d["e_lm"]] != 0))
    return np.unique(np.asarray(d["e_lm"])[act])


def tenth_case(seed=11):
    """BA edges + priors on a tenth of the landmarks (one landmark has two), dense Omega, Huber, measured N(0, 0.05) off
    the ground truth; one of the landmarks with a prior is fixed (that prior counts for nothing)"""
    import synth
    d = synth.make_problem(n_poses=8, n_landmarks=80, seed=seed, fixed_poses=(0,), fixed_landmarks=(20,))
    rng = np.random.default_rng(seed)
    seen = set(_observed(d).tolist())
    lm = [l for l in range(0, 80, 10) if l in seen] + [30]
    assert 20 in lm and len(lm) >= 8
    z = d["lm_gt"][lm] + rng.normal(0, 0.05, (len(lm), 3))
    info = [random_spd3(rng, 20.0) for _ in lm]
    return d, make_prior(lm, z, info, rk=(RK_HUBER, 2.0)), [], None


def gauge_case(seed=12):
    """no fixed vertex at all: the gauge is held by four landmark priors (Omega = 1e6 I at the ground truth)"""
    import synth
    d = synth.make_problem(n_poses=8, n_landmarks=80, seed=seed, fixed_poses=())
    assert not d["pose_fixed"].any() and not d["lm_fixed"].any()
    lm = [3, 25, 50, 77]
    assert set(lm) <= set(_observed(d).tolist())
    assert abs(np.linalg.det(np.c_[d["lm_gt"][lm], np.ones(4)])) > 1e-3, "the four landmarks are coplanar"
    return d, make_prior(lm, d["lm_gt"][lm], 1e6 * np.eye(3)[None]), [], None


def single_mono_case(seed=13):
    """a landmark that ONE mono edge observes (rank-2 Hll from the BA side) made well-posed by a weak prior"""
    import synth
    d = synth.make_problem(n_poses=8, n_landmarks=79, seed=seed, fixed_poses=(0,))
    rng = np.random.default_rng(seed)
    p = 3
    cam = synth.KITTI_CAM
    R = synth.quat_to_R(d["pose_gt"][p, :4])
    Xc = np.array([0.4, -0.3, 9.0])
    Xw = R.T @ (Xc - d["pose_gt"][p, 4:])
    meas = np.array([cam[0] * Xc[0] / Xc[2] + cam[2], cam[1] * Xc[1] / Xc[2] + cam[3], 0.0]) + np.r_[rng.normal(0, 1.0, 2), 0.0]
    d = dict(d)
    d["lm"] = np.vstack([d["lm"], Xw + rng.normal(0, 0.05, 3)])
    d["lm_gt"] = np.vstack([d["lm_gt"], Xw])
    d["lm_fixed"] = np.r_[d["lm_fixed"], 0].astype(np.uint8)
    d["e_pose"] = np.r_[d["e_pose"], p].astype(np.int32)
    d["e_lm"] = np.r_[d["e_lm"], 79].astype(np.int32)
    d["e_stereo"] = np.r_[d["e_stereo"], 0].astype(np.uint8)
    d["e_meas"] = np.vstack([d["e_meas"], meas])
    d["e_omega"] = np.r_[d["e_omega"], 1.0]
    d["e_cam"] = np.vstack([d["e_cam"], cam])
    assert (d["e_lm"] == 79).sum() == 1
    lm = [79, 5]
    return d, make_prior(lm, d["lm_gt"][lm] + rng.normal(0, 0.05, (2, 3)), np.array([4.0 * np.eye(3), random_spd3(rng, 5.0)])), [], None


def reject_case(seed=3):
    """the golden stress fixture reject_8x60 (it takes rejected trials) + priors on every seventh landmark displaced from
    the INITIAL landmarks"""
    import os
    g8 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reject_8x60.npz"))
    d = {k: g8[k] for k in g8.files}
    rng = np.random.default_rng(seed + 300)
    seen = set(_observed(d).tolist())
    lm = [l for l in range(0, len(d["lm"]), 7) if l in seen and not d["lm_fixed"][l]]
    z = d["lm"][lm] + rng.normal(0, 0.1, (len(lm), 3))
    return d, make_prior(lm, z, [random_spd3(rng, 2.0) for _ in lm]), [], None


def mixed_case(seed=5):
    """prior_ref.mixed_prior_case (BA + plane + line + pose priors, pose 0 fixed) + landmark priors on every tenth
    landmark, Cauchy"""
    d, icp, prior = prior_ref.mixed_prior_case(seed=seed)
    rng = np.random.default_rng(seed + 400)
    seen = set(_observed(d).tolist())
    lm = [l for l in range(0, len(d["lm"]), 10) if l in seen]
    z = d["lm_gt"][lm] + rng.normal(0, 0.05, (len(lm), 3))
    return d, make_prior(lm, z, [random_spd3(rng, 10.0) for _ in lm], rk=(RK_CAUCHY, 3.0)), icp, prior


CASES = {  # name -> (recipe, iterations)
    "tenth": (tenth_case, 6),
    "gauge": (gauge_case, 6),
    "single_mono": (single_mono_case, 6),
    "reject": (reject_case, 8),
    "mixed": (mixed_case, 8),
}
