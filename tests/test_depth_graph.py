"""GPU tests of depth edges through the optimiser (cugo.Graph): the LM trajectory against the numpy reference of
tests/golden/make_golden.py (Graph) subclassed with the depth row, under the tolerance rule of icp_lm_ref.tolerances
(per iteration max(1e-10, 4 x what the reference differs by from itself — Schur against dense solve, edges permuted),
estimates max(1e-9, 4 x)); outlier rejection on the depth set against the reference's verdicts; the forms of the loop;
covariances against the dense inverse; flatten re-use.  Graphs of 8 poses x 60 landmarks (below small_10x200)."""
import importlib
import os
import sys

import numpy as np
import pytest

import icp_lm_ref as R
import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden as MG  # noqa: E402

pytestmark = pytest.mark.gpu

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
MONO, STEREO, DEPTH = 0, 1, 2


def depth_edge(pose, Xw, meas, cam, s):
    """residual (pu - u, pv - v, s (1/Z - m_d)) and J = -de/dx (left perturbation [omega, upsilon]; landmark)"""
    fx, fy, cx, cy, _ = cam
    Rm = MG.quat_to_R(pose[:4])
    Xc = Rm @ Xw + pose[4:]
    X, Y, Z = Xc
    e = np.array([fx * X / Z + cx - meas[0], fy * Y / Z + cy - meas[1], s * (1.0 / Z - meas[2])])
    de = np.array([[fx / Z, 0, -fx * X / Z**2], [0, fy / Z, -fy * Y / Z**2], [0, 0, -s / Z**2]])    # de / dXc
    skew = np.array([[0, -Z, Y], [Z, 0, -X], [-Y, X, 0]])
    return e, Xc, -de @ np.hstack([-skew, np.eye(3)]), -de @ Rm


class DepthGraph(MG.Graph):
    """make_golden.Graph with a kind per edge (mono, stereo, depth), a robust kernel per kind and the inverse-depth
    weight k"""

    def __init__(self, d, kind, rk3, k, via_schur=True):
        super().__init__(d)
        self.kind, self.rk3, self.s, self.via_schur = np.asarray(kind), rk3, np.sqrt(k), via_schur
        self.live = np.ones(len(self.ep), bool)

    def _edge(self, i):
        p, X = self.pose[self.ep[i]], self.lm[self.el[i]]
        if self.kind[i] == DEPTH:
            return depth_edge(p, X, self.meas[i], self.cam[i], self.s)
        return MG.edge(p, X, self.meas[i], self.kind[i] == STEREO, self.cam[i])

    def edge_chi(self):
        out = np.zeros(len(self.ep))
        for i in np.nonzero(self.active & self.live)[0]:
            e = self._edge(i)[0]
            rk = self.rk3[self.kind[i]]
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
            rk = self.rk3[self.kind[i]]
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

    def solve(self, H, b, lam, via_schur=True):
        return super().solve(H, b, lam, via_schur=self.via_schur)


def permute_edges(d, kind, seed=91):
    perm = np.random.default_rng(seed).permutation(len(kind))
    out = dict(d)
    for key in ("e_pose", "e_lm", "e_stereo", "e_meas", "e_omega", "e_cam"):
        out[key] = np.asarray(d[key])[perm]
    return out, np.asarray(kind)[perm]


def reference_runs(d, kind, rk3, k, niter):
    runs = []
    dp, kp = permute_edges(d, kind)
    for dd, kk, vs in ((d, kind, True), (d, kind, False), (dp, kp, True)):
        g = DepthGraph(dd, kk, rk3, k, via_schur=vs)
        runs.append((g.optimize(niter), g.pose.copy(), g.lm.copy()))
    tr = runs[0][0]
    sens, est = [0.0] * len(tr), 0.0
    for t2, pose2, lm2 in runs[1:]:
        assert [t[4] for t in t2] == [t[4] for t in tr], "the reference disagrees with itself on the trial counts"
        for i in range(len(tr)):
            sens[i] = max(sens[i], abs(tr[i][1] - t2[i][1]) / abs(tr[i][1]))
        est = max(est, float(np.abs(runs[0][1] - pose2).max()), float(np.abs(runs[0][2] - lm2).max()))
    return R.trace_dicts(tr), runs[0][1], runs[0][2], sens, est


NONE = (0, 1.0)


def base_problem(seed, kinds, sigma_d=1e-3, **kw):
    """8 poses (pose 0 fixed) x 60 landmarks; kinds: the kinds the landmarks' edges take in turn.  Depth measurement:
    1/Z of the generating geometry + N(0, sigma_d)"""
    d = synth.make_problem(n_poses=8, n_landmarks=60, mean_obs=3.0, seed=seed, per_edge_cam=True, **kw)
    rng = np.random.default_rng(seed + 100)
    E = len(d["e_pose"])
    kind = np.array([kinds[l % len(kinds)] for l in d["e_lm"]])
    meas = d["e_meas"].copy()
    for i in range(E):
        Xc = MG.quat_to_R(d["pose_gt"][d["e_pose"][i], :4]) @ d["lm_gt"][d["e_lm"][i]] + d["pose_gt"][d["e_pose"][i], 4:]
        uu = meas[i, 0]
        if kind[i] == DEPTH:
            meas[i, 2] = 1.0 / Xc[2] + rng.normal(0, sigma_d)
        elif kind[i] == STEREO:
            meas[i, 2] = uu - d["e_cam"][i, 4] / Xc[2] + rng.normal(0, 1.0)
        else:
            meas[i, 2] = 0.0
    d = dict(d, e_meas=meas, e_stereo=(kind == STEREO).astype(np.uint8))
    return d, kind


def scaled_about_fixed_pose(d, factor):
    """the start of d with every camera centre and every landmark scaled by `factor` about the centre of the fixed pose 0"""
    out = dict(d)
    pose, lm = d["pose"].copy(), d["lm"].copy()
    R0 = MG.quat_to_R(pose[0, :4])
    c0 = -R0.T @ pose[0, 4:]
    for i in range(1, len(pose)):
        Ri = MG.quat_to_R(pose[i, :4])
        c = -Ri.T @ pose[i, 4:]
        pose[i, 4:] = -Ri @ (c0 + factor * (c - c0))
    out["pose"], out["lm"] = pose, c0 + factor * (lm - c0)
    return out


def scale_of(d, pose, lm):
    """the scale of (pose, lm) about the fixed pose's centre relative to the generating geometry"""
    c0 = -MG.quat_to_R(d["pose_gt"][0, :4]).T @ d["pose_gt"][0, 4:]
    return float(np.median(np.linalg.norm(lm - c0, axis=1) / np.linalg.norm(d["lm_gt"] - c0, axis=1)))


def case(name):
    if name == "depth_only":
        d, kind = base_problem(31, (DEPTH,))
        return d, kind, {MONO: NONE, STEREO: NONE, DEPTH: NONE}, 1e4, 6
    if name == "scale":
        d, kind = base_problem(33, (MONO, DEPTH), pose_noise=(0.0, 0.0), lm_noise=0.0)
        # (k = 1 / sigma_d^2: the depth residual in units of its noise, as the pixel residuals are)
        return scaled_about_fixed_pose(d, 1.2), kind, {MONO: NONE, STEREO: NONE, DEPTH: NONE}, 1e6, 10
    if name == "mixed":
        d, kind = base_problem(35, (MONO, STEREO, DEPTH))
        return d, kind, {MONO: (1, 3.0), STEREO: NONE, DEPTH: (3, 1.5)}, 1e4, 6
    raise KeyError(name)


_REF = {}


def reference(name):
    if name not in _REF:
        d, kind, rk3, k, niter = case(name)
        tr, pose, lm, sens, est = reference_runs(d, kind, rk3, k, niter)
        print("reference %s: self-sensitivity %.3g (chi2), %.3g (estimates); trials %s; chi2 %.6g -> %.6g" %
              (name, max(sens), est, [t["trials"] for t in tr], tr[0]["chi2"], tr[-1]["chi2"]))
        tol, etol = R.tolerances(sens, est)
        _REF[name] = (d, kind, rk3, k, niter, tr, pose, lm, tol, etol)
    return _REF[name]


def build_graph(d, kind, rk3, k, threshold=0.0):
    g = cugo.Graph(True, True)
    P, L = len(d["pose"]), len(d["lm"])
    g.add_poses(np.arange(P, dtype=np.int32), d["pose"], d["pose_fixed"])
    g.add_landmarks(np.arange(L, dtype=np.int32), d["lm"], d["lm_fixed"])
    for dim, q in ((2, MONO), (3, STEREO)):
        sel = kind == q
        g.add_edges(dim, d["e_pose"][sel], d["e_lm"][sel], d["e_meas"][sel], d["e_omega"][sel], d["e_cam"][sel])
        g.set_robust_kernel(dim, rk3[q][0], rk3[q][1])
    sel = kind == DEPTH
    g.add_depth_edges(d["e_pose"][sel], d["e_lm"][sel], d["e_meas"][sel], d["e_omega"][sel], d["e_cam"][sel])
    g.set_depth_robust_kernel(rk3[DEPTH][0], rk3[DEPTH][1])
    g.set_depth_weight(k)
    if threshold:
        g.set_depth_outlier_threshold(threshold)
    return g


def run(name_or_case, float32=False, keep=False, threshold=0.0):
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    d, kind, rk3, k, niter = case(name_or_case) if isinstance(name_or_case, str) else name_or_case
    g = build_graph(d, kind, rk3, k, threshold)
    if float32:
        g.set_float32(1)
    g.initialize()
    g.optimize(niter)
    out = dict(stats=g.stats(), pose=g.poses(), lm=g.landmarks(), nedges=g.n_active_edges())
    if keep:
        out["g"] = g
    else:
        g.close()
    return out


def assert_trajectories_match(stats, tr, tol, check_trials=True):
    assert len(stats) == len(tr), (len(stats), len(tr))
    for s, t, tl in zip(stats, tr, tol if isinstance(tol, list) else [tol] * len(tr)):
        print("it %d chi2 %.12g ref %.12g rel %.3g (tol %.3g) trials %d/%d" %
              (t["iteration"], s["chi2"], t["chi2"], abs(s["chi2"] - t["chi2"]) / abs(t["chi2"]), tl, s["trials"], t["trials"]))
        assert abs(s["chi2"] - t["chi2"]) <= tl * abs(t["chi2"])
        if check_trials:
            assert s["trials"] == t["trials"]


@pytest.mark.parametrize("name", ["depth_only", "scale", "mixed"])
def test_lm_trajectory_matches_the_reference(name):
    d, kind, rk3, k, niter, tr, pose, lm, tol, etol = reference(name)
    assert len(tr) == niter
    out = run(name)
    assert out["nedges"] == len(kind)
    assert_trajectories_match(out["stats"], tr, tol)
    np.testing.assert_allclose(out["pose"], pose, rtol=0, atol=etol)
    np.testing.assert_allclose(out["lm"], lm, rtol=0, atol=10 * etol)
    if name == "scale":
        # the start is 20 % too large; mono edges alone cannot tell: the depth edges bring the scale back
        s0, s_ref, s_got = scale_of(d, d["pose"], d["lm"]), scale_of(d, pose, lm), scale_of(d, out["pose"], out["lm"])
        print("scale: start %.4f, reference %.6f, optimiser %.6f" % (s0, s_ref, s_got))
        # (checked on the CPU: the reference is back at 1.006 after these 10 iterations; a depth measurement with
        # sigma_d = 1e-3 at 20 m is 2 % of the depth, the median over 60 landmarks well below 1 %)
        assert abs(s0 - 1.2) < 1e-6 and abs(s_ref - 1) < 1e-2 and abs(s_got - s_ref) < 1e-8


def test_outlier_rejection_on_the_depth_set_agrees_with_the_reference():
    """a tenth of the depth measurements off by 30 sigma; the verdicts of the reference at ITS final estimates with a
    margin round the threshold (no edge of the reference within 1 % of it), as reject_8x60 is used"""
    d, kind, rk3, k, niter = case("mixed")
    rng = np.random.default_rng(5)
    dep = np.flatnonzero(kind == DEPTH)
    bad = dep[rng.random(len(dep)) < 0.1]
    meas = d["e_meas"].copy()
    meas[bad, 2] += 0.03
    d = dict(d, e_meas=meas)
    ref = DepthGraph(d, kind, rk3, k)
    ref.optimize(niter)
    chi = ref.edge_chi()[dep]
    threshold = 4.0
    assert np.all(np.abs(chi - threshold) > 0.01 * threshold), "an edge of the reference sits on the threshold"
    verdict = chi > threshold
    assert 3 <= verdict.sum() < len(dep) // 2
    out = run((d, kind, rk3, k, niter), keep=True, threshold=threshold)
    g = out["g"]
    active = g.depth_edge_active(len(dep))
    assert np.array_equal(~active, verdict)
    assert g.n_depth_outliers() == verdict.sum() and g.n_outliers(2) == 0 and g.n_outliers(3) == 0
    # the next initialize() leaves them out
    g.initialize()
    assert g.n_active_edges() == len(kind) - verdict.sum()
    g.close()


FORMS = ["CUGO_POSE_SCHUR=0", "CUGO_BS_RECORDS=0", "CUGO_TRIAL_FROM_BUILD=0", "CUGO_SCHUR_PLAN=1", "CUGO_HSC_MFMA=0"]


@pytest.mark.parametrize("form", FORMS)
def test_forms_of_the_loop_take_depth_edges(form, monkeypatch):
    """every form follows the reference's trajectory under the same rule; the record form of the back-substitution and
    the chi2 out of the next build pass are bit-neutral, as for the other sets"""
    d, kind, rk3, k, niter, tr, pose, lm, tol, etol = reference("mixed")
    base = run("mixed")
    var, val = form.split("=")
    monkeypatch.setenv(var, val)
    out = run("mixed")
    assert_trajectories_match(out["stats"], tr, tol)
    np.testing.assert_allclose(out["pose"], pose, rtol=0, atol=etol)
    np.testing.assert_allclose(out["lm"], lm, rtol=0, atol=10 * etol)
    if var in ("CUGO_BS_RECORDS", "CUGO_TRIAL_FROM_BUILD"):
        assert [(s["chi2"], s["lam"], s["trials"]) for s in out["stats"]] == [(s["chi2"], s["lam"], s["trials"]) for s in base["stats"]]
        assert np.array_equal(out["pose"], base["pose"]) and np.array_equal(out["lm"], base["lm"])


def test_float32_internal_mode_with_depth_edges():
    """float block storage: the bar tests/test_prior_graph.py states for the mode (chi2 to 1e-5, the same trials)"""
    d, kind, rk3, k, niter, tr, pose, lm, tol, etol = reference("mixed")
    out = run("mixed", float32=True)
    assert_trajectories_match(out["stats"], tr, 1e-5, check_trials=False)
    assert [s["trials"] for s in out["stats"]] == [t["trials"] for t in tr]


def test_covariances_match_the_dense_inverse():
    """pose and landmark covariances of a graph with depth edges against the inverse of the reference's undamped
    system at the optimiser's estimates: the rule of tests/test_covariance.py (1e-8 of the block norm)"""
    d, kind, rk3, k, niter = case("mixed")
    out = run("mixed", keep=True)
    g = out["g"]
    g.compute_covariances()
    ref = DepthGraph(d, kind, rk3, k)
    ref.pose[:], ref.lm[:] = out["pose"], out["lm"]
    H, _ = ref.normal_equations()
    inv = np.linalg.inv(H)
    cp, cl = g.pose_covariances(), g.landmark_covariances()
    worst = [0.0, 0.0]
    for blocks, offs, w, q in ((cp, np.where(ref.pf, -1, 6 * ref.pidx), 6, 0),
                               (cl, np.where(ref.lf, -1, 6 * ref.np_ + 3 * ref.lidx), 3, 1)):
        for i, o in enumerate(offs):
            if o < 0:
                assert not blocks[i].any()
                continue
            blk = inv[o:o + w, o:o + w]
            worst[q] = max(worst[q], np.abs(blocks[i] - blk).max() / np.linalg.norm(blk))
    print("covariance blocks off by %.3g (poses), %.3g (landmarks) of the block norm" % tuple(worst))
    assert worst[0] <= 1e-8 and worst[1] <= 1e-8
    g.close()


def test_second_initialize_after_estimates_changed_reuses_the_flattening():
    d, kind, rk3, k, niter = case("mixed")
    out = run("mixed", keep=True)
    g = out["g"]
    assert g.flatten_reuses() == 0
    g.set_poses(np.arange(len(d["pose"]), dtype=np.int32), d["pose"])
    g.set_landmarks(np.arange(len(d["lm"]), dtype=np.int32), d["lm"])
    g.initialize()
    assert g.flatten_reuses() == 1
    g.optimize(niter)
    assert [(s["chi2"], s["trials"]) for s in g.stats()] == [(s["chi2"], s["trials"]) for s in out["stats"]]
    assert np.array_equal(g.poses(), out["pose"]) and np.array_equal(g.landmarks(), out["lm"])
    g.close()
