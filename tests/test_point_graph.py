"""Point-to-point edge sets (PointEdgeSet) in the LM loop, on the GPU: the optimiser against the dense numpy LM of
tests/point_lm_ref.py in every form the loop takes — the one-stream iteration, the two-stream one, without speculative
build passes, trials whose chi2 comes out of the next build pass, rejected trials — and the relations between those forms.

Tolerance: the project's rule (conftest.golden_tolerances): relative chi2 per iteration within max(1e-10, 4 x the
self-sensitivity), estimates within max(1e-9, 4 x), the same trial counts, no decision at |rho| < 0.1.  The
self-sensitivity is measured by the reference ON ITSELF (its Schur solve against its full dense solve, and every pose
edge set in a permuted order) and printed."""
import importlib

import numpy as np
import pytest

import icp_lm_ref
import icp_ref
import point_lm_ref as R
from test_gpu import assert_trajectories_match

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
pytestmark = pytest.mark.gpu

_REF = {}
TRIALS = {"points_only": [0] * 6, "mixed": [0] * 8, "reject": [2, 2, 0, 0, 0, 0, 0, 0]}


def reference(name):
    if name not in _REF:
        recipe, niter = R.CASES[name]
        d, icp, prior, pts = recipe()
        tr, pose, lm, sens, est = R.reference_runs(d, icp, prior, pts, niter)
        assert [t["trials"] for t in tr] == TRIALS[name], "the recipe no longer gives the trials it was chosen for"
        assert all(abs(t["rho"]) >= 0.1 for t in tr), "a decision at rho near 0 is not a fair comparison"
        print("reference %s: self-sensitivity %.3g (chi2), %.3g (estimates)" % (name, max(sens), est))
        tol, etol = icp_lm_ref.tolerances(sens, est)
        _REF[name] = (d, icp, prior, pts, niter, tr, pose, lm, tol, etol)
    return _REF[name]


def run(d, icp, prior, pts, niter, float32=False, timing=False):
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    g = R.build_graph(d, icp, prior, pts)
    if float32:
        g.set_float32(1)
    if timing:
        g.set_kernel_timing(1)
    g.initialize()
    g.optimize(niter)
    out = dict(stats=g.stats(), pose=g.poses(), lm=g.landmarks(), sstats=g.structure_stats(), nedges=g.n_active_edges(),
               n_point=g.n_point_edges())
    if timing:
        out["kernels"] = g.kernel_times()
    g.close()
    return out


def key(stats):
    return [(s["chi2"], s["lam"], s["trials"]) for s in stats]


def same_bits(a, b):
    assert key(a["stats"]) == key(b["stats"])
    assert np.array_equal(a["pose"], b["pose"]) and np.array_equal(a["lm"], b["lm"])


def launches(k, name):
    return k.get(name, dict(launches=0))["launches"]


@pytest.mark.parametrize("form", ["one_stream", "two_stream", "no_speculation"])
@pytest.mark.parametrize("name", list(TRIALS))
def test_lm_trajectory_against_the_reference(name, form, monkeypatch):
    """(a) points only, (b) mixed with BA, plane, line and prior sets, (c) rejected trials: CUGO_POSE_SCHUR=1 (the point sums
    are added behind k_pose_schur), =0 (to Hpp / bp behind k_build_poses), and CUGO_SPECULATE=0"""
    set_form(form, monkeypatch)
    d, icp, prior, pts, niter, tr, pose, lm, tol, etol = reference(name)
    out = run(d, icp, prior, pts, niter, timing=True)
    for a, b in zip(out["stats"], tr):
        print(name, form, "chi2 %.15g ref %.15g rel %.3g lam %.6g ref %.6g trials %d ref %d" %
              (a["chi2"], b["chi2"], abs(a["chi2"] - b["chi2"]) / b["chi2"], a["lam"], b["lam"], a["trials"], b["trials"]))
    k = out["kernels"]
    assert launches(k, "k_point_chunks_build") > 0 and "k_point_check" not in k
    if len(d["lm"]):           # (a graph without landmarks has no k_pose_schur: its terms go to Hpp / bp)
        assert (launches(k, "k_point_add_schur") > 0) == (form != "two_stream")
        assert (launches(k, "k_point_add") > 0) or form != "two_stream"
    assert out["n_point"] == int((pts["active"] & (np.asarray(d["pose_fixed"])[pts["pose"]] == 0)).sum())
    assert_trajectories_match(out["stats"], tr, tol)
    np.testing.assert_allclose(out["pose"], pose, rtol=0, atol=etol)
    if len(lm):
        np.testing.assert_allclose(out["lm"], lm, rtol=0, atol=10 * etol)
    assert out["sstats"]["trial_sync_retries"] == 0


def set_form(form, monkeypatch):
    if form == "two_stream":
        monkeypatch.setenv("CUGO_POSE_SCHUR", "0")
    if form == "no_speculation":
        monkeypatch.setenv("CUGO_SPECULATE", "0")


_ZERO = {}


def zero_noise_reference():
    """case (d) through the reference: chi2 falls to rounding level (1e-21), where a relative comparison, a gain ratio and a
    trial count mean nothing; the iterations with chi2 above 1e-6 are held to the rule (their rho and trial counts as
    reference() asks of the other cases), the end to the truth"""
    if not _ZERO:
        d, icp, prior, pts = R.zero_noise_case()
        tr, pose, lm, sens, est = R.reference_runs(d, icp, prior, pts, 8)
        n = sum(t["chi2"] > 1e-6 for t in tr)
        assert n >= 2 and [t["trials"] for t in tr[:n]] == [0] * n, "the recipe no longer gives the trials it was chosen for"
        assert all(abs(t["rho"]) >= 0.1 for t in tr[:n]), "a decision at rho near 0 is not a fair comparison"
        print("reference zero_noise: self-sensitivity %.3g (chi2), %.3g (estimates)" % (max(sens[:n]), est))
        tol, etol = icp_lm_ref.tolerances(sens, est)
        _ZERO.update(d=d, icp=icp, prior=prior, pts=pts, tr=tr, n=n, tol=tol, etol=etol)
    return _ZERO


@pytest.mark.parametrize("form", ["one_stream", "two_stream", "no_speculation"])
def test_zero_noise_ends_at_the_truth(form, monkeypatch):
    """(d) one free pose, 200 exact correspondences, the start 0.5 rad / 1 m away, in the three forms of the loop"""
    set_form(form, monkeypatch)
    z = zero_noise_reference()
    out = run(z["d"], z["icp"], z["prior"], z["pts"], 8)
    print("zero noise", form, "chi2", [s["chi2"] for s in out["stats"]], "reference", [t["chi2"] for t in z["tr"]])
    n = z["n"]
    assert_trajectories_match(out["stats"][:n], z["tr"][:n], z["tol"][:n])
    np.testing.assert_allclose(out["pose"], z["d"]["pose_gt"], rtol=0, atol=z["etol"])
    assert out["stats"][-1]["chi2"] < 1e-15 and out["sstats"]["trial_sync_retries"] == 0


def test_trial_chi2_from_the_next_build_pass_is_bit_neutral(monkeypatch):
    for name in ("mixed", "reject", "points_only"):
        d, icp, prior, pts = R.CASES[name][0]()
        runs = []
        for v in ("1", "0"):
            monkeypatch.setenv("CUGO_TRIAL_FROM_BUILD", v)
            runs.append(run(d, icp, prior, pts, R.CASES[name][1]))
        same_bits(runs[0], runs[1])
        monkeypatch.delenv("CUGO_TRIAL_FROM_BUILD")
        same_bits(runs[0], run(d, icp, prior, pts, R.CASES[name][1]))      # and a fresh optimiser gives the same bits


def test_float32_internal_mode_runs():
    """the point terms stay fp64 (they touch no stored block): the bar test_float32_block_storage states for the mode"""
    d, icp, prior, pts, niter, tr, pose, lm, tol, etol = reference("mixed")
    out = run(d, icp, prior, pts, niter, float32=True)
    assert_trajectories_match(out["stats"], tr, 1e-5, check_trials=False)
    assert [s["trials"] for s in out["stats"]] == [t["trials"] for t in tr]


def test_a_set_that_counts_for_nothing_changes_no_bit():
    """point edges all on fixed poses, or no point edge at all, next to a BA graph: bit for bit the run without them"""
    d, icp, prior, pts = R.mixed_case()
    ba = run(d, icp, prior, None, 8)
    assert ba["n_point"] == 0
    sel = np.asarray(d["pose_fixed"], bool)[pts["pose"]]
    assert sel.sum() == 20
    on_fixed = dict(pts, **{k: np.asarray(pts[k])[sel] for k in ("pose", "p", "z", "active", "info")})
    out = run(d, icp, prior, on_fixed, 8)
    assert out["n_point"] == 0 and out["nedges"] == ba["nedges"]
    same_bits(ba, out)
    empty = dict(pts, **{k: np.asarray(pts[k])[:0] for k in ("pose", "p", "z", "active")}, info=pts["info"][:1])
    same_bits(ba, run(d, icp, prior, empty, 8))


def test_the_sets_matrix_counts_without_per_edge_information():
    """perEdgeInformation off: the set's matrix counts and the edges' own are not looked at — the bits of the run in which
    every edge carries that matrix"""
    d, _, _, pts = R.points_only_case()
    a = run(d, [], None, dict(pts, info=pts["info"][:1]), 6)
    other = dict(pts, info=np.tile(7.0 * np.eye(3), (len(pts["pose"]), 1, 1)))
    g = R.build_graph(d, [], None, other, per_edge_information=False)
    g.set_point_information(pts["info"][0])
    g.initialize()
    g.optimize(6)
    assert key(g.stats()) == key(a["stats"]) and np.array_equal(g.poses(), a["pose"])
    g.close()
    b = run(d, [], None, other, 6)                      # and with per-edge information the edges' matrices do count
    assert key(b["stats"]) != key(a["stats"])


def test_covariances_with_point_sets():
    """computeMarginals of case (a): Sigma_p = (the reference's H_p)^-1 per pose, zeros for the fixed one, held as
    test_icp_graph.test_covariances_with_icp_sets holds its own"""
    d, icp, prior, pts = R.points_only_case()
    g = R.build_graph(d, icp, prior, pts)
    g.initialize()
    g.optimize(5)
    g.compute_covariances(poses=True, landmarks=False)
    Hi = R.PointGraph(dict(d, pose=g.poses()), icp, prior, pts)._pts()[0]
    cov = g.pose_covariances()
    for p in range(5):
        ref = np.linalg.inv(Hi[p])
        assert np.abs(cov[p] - ref).max() <= 1e-8 * np.linalg.norm(ref), p
    assert not cov[5].any()
    g.close()


def test_three_axis_planes_per_correspondence_equal_one_identity_point_edge():
    """a graph of three axis-plane edges per correspondence (n = e_k, d = z_k) and the same graph with one Omega = I point edge
    each minimise the same cost: the same estimates, to the estimate tolerance"""
    d, _, _, pts = R.points_only_case()
    pts = dict(pts, info=np.eye(3)[None], rk=(icp_ref.RK_NONE, 1.0))
    tr, pose, lm, sens, est = R.reference_runs(d, [], None, pts, 8)
    _, etol = icp_lm_ref.tolerances(sens, est)
    a = run(d, [], None, pts, 8)
    E = len(pts["pose"])
    pl = dict(pose=np.repeat(pts["pose"], 3), p=np.repeat(pts["p"], 3, axis=0), n=np.tile(np.eye(3), (E, 1)), d=pts["z"].reshape(-1))
    icp = [("plane", pl, np.array([1.0]), np.ones(3 * E, bool), (icp_ref.RK_NONE, 1.0))]
    g = icp_lm_ref.build_graph(d, icp)
    g.initialize()
    g.optimize(8)
    b_pose = g.poses()
    g.close()
    print("planes against points: largest difference %.3g (tolerance %.3g)" % (np.abs(a["pose"] - b_pose).max(), etol))
    np.testing.assert_allclose(a["pose"], pose, rtol=0, atol=etol)
    np.testing.assert_allclose(b_pose, a["pose"], rtol=0, atol=etol)
