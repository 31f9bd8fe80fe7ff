"""Covariance-form point edge sets (GicpEdgeSet, GicpPairEdgeSet: generalised ICP) in the LM loop, on the GPU: the
optimiser against the dense numpy LM of tests/gicp_lm_ref.py, in which Omega = (C_z + M C_p M^T)^-1 is re-evaluated at every
linearisation and every trial, under the default form of the loop, CUGO_POSE_SCHUR=0 and CUGO_SPECULATE=0.

Tolerance: the project's rule (icp_lm_ref.tolerances): relative chi2 per iteration within max(1e-10, 4 x the
self-sensitivity), estimates within max(1e-9, 4 x), the same trial counts.  test_gicp_graph_host.py holds, on the CPU, that
no decision is at |rho| < 0.1 and that an Omega frozen at the initial poses misses this tolerance by more than 100 x."""
import importlib

import numpy as np
import pytest

import gicp_lm_ref as G
import icp_lm_ref
import point_pair_lm_ref as PPL
from test_gpu import assert_trajectories_match

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
pytestmark = pytest.mark.gpu

_REF = {}
FORMS = ["default", "two_stream", "no_speculation"]


def reference(name):
    if name not in _REF:
        recipe, niter = G.CASES[name]
        case = recipe()
        tr, pose, lm, sens, est = G.reference_runs(*case, niter)
        print("reference %s: self-sensitivity %.3g (chi2), %.3g (estimates); trials %s" % (name, max(sens), est, [t["trials"] for t in tr]))
        tol, etol = icp_lm_ref.tolerances(sens, est)
        _REF[name] = (case, niter, tr, pose, lm, tol, etol)
    return _REF[name]


def run(case, niter, timing=False, graph=None, float32=False):
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    g = G.build_graph(*case) if graph is None else graph
    if float32:
        g.set_float32(1)
    if timing:
        g.set_kernel_timing(1)
    g.initialize()
    g.optimize(niter)
    out = dict(stats=g.stats(), pose=g.poses(), lm=g.landmarks(), sstats=g.structure_stats(), nedges=g.n_active_edges(),
               n_gicp=g.n_gicp_edges(), n_gicp_pair=g.n_gicp_pair_edges())
    if timing:
        out["kernels"] = g.kernel_times()
    g.close()
    return out


def same_bits(a, b):
    key = lambda s: [(x["chi2"], x["lam"], x["trials"]) for x in s["stats"]]
    assert key(a) == key(b) and np.array_equal(a["pose"], b["pose"]) and np.array_equal(a["lm"], b["lm"])


def set_form(form, monkeypatch):
    if form == "two_stream":
        monkeypatch.setenv("CUGO_POSE_SCHUR", "0")
    if form == "no_speculation":
        monkeypatch.setenv("CUGO_SPECULATE", "0")


def launches(k, name):
    return k.get(name, dict(launches=0))["launches"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["scan_to_map", "multi_scan", "mixed", "iso"])
def test_lm_trajectory_against_the_reference(name, form, monkeypatch):
    set_form(form, monkeypatch)
    case, niter, tr, pose, lm, tol, etol = reference(name)
    out = run(case, niter, timing=True)
    for a, b in zip(out["stats"], tr):
        print(name, form, "chi2 %.15g ref %.15g rel %.3g trials %d ref %d" % (a["chi2"], b["chi2"], abs(a["chi2"] - b["chi2"]) / b["chi2"],
                                                                             a["trials"], b["trials"]))
    k = out["kernels"]
    if name == "scan_to_map":                 # the covariance instantiations ran, the information form's did not
        assert launches(k, "k_gicp_chunks_build") > 0 and launches(k, "k_point_chunks_build") == 0 and out["n_gicp"] == 600
    else:
        assert launches(k, "k_gicp_pair_chunks_build") > 0 and launches(k, "k_point_pair_chunks_build") == 0 and out["n_gicp_pair"] > 0
    assert_trajectories_match(out["stats"], tr, tol)
    np.testing.assert_allclose(out["pose"], pose, rtol=0, atol=etol)
    if len(lm):
        np.testing.assert_allclose(out["lm"], lm, rtol=0, atol=10 * etol)
    assert out["sstats"]["trial_sync_retries"] == 0


def test_iso_is_the_information_form_with_the_scaled_identity():
    """Omega = I / (sigma_p^2 + sigma_z^2) whatever the rotation: a PointPairEdgeSet with that Omega follows the same
    trajectory under the same rule (not the same bits: an inverse rounds)"""
    case, niter, tr, pose, lm, tol, etol = reference("iso")
    d, icp, prior, pts, rp, _, gp = case
    s = np.asarray(gp["cov_p"])[:, 0, 0] + np.asarray(gp["cov_z"])[:, 0, 0]
    pairs = dict(a=gp["a"], b=gp["b"], p=gp["p"], z=gp["z"], active=gp["active"], rk=gp["rk"], info=np.eye(3)[None] / s[:, None, None])
    g = PPL.build_graph(d, icp, prior, pts, rp, pairs)
    out = run(None, niter, graph=g)
    got = run(case, niter)
    assert_trajectories_match(out["stats"], tr, tol)
    assert_trajectories_match(got["stats"], tr, tol)
    np.testing.assert_allclose(out["pose"], got["pose"], rtol=0, atol=2 * etol)


def test_float32_internal_mode_runs():
    """useFloat32 behaves as for the point kinds (test_point_graph.py::test_float32_internal_mode_runs, its bar): the
    covariance terms stay fp64, the BA blocks of the mixed case are stored in float"""
    case, niter, tr, pose, lm, tol, etol = reference("mixed")
    out = run(case, niter, float32=True)
    assert_trajectories_match(out["stats"], tr, 1e-5, check_trials=False)
    assert [s["trials"] for s in out["stats"]] == [t["trials"] for t in tr]


def test_zero_noise_ends_at_the_truth():
    case = G.zero_noise_case()
    out = run(case, 10)
    print("zero noise chi2", [s["chi2"] for s in out["stats"]])
    np.testing.assert_allclose(out["pose"], case[0]["pose_gt"], rtol=0, atol=1e-9)
    assert out["stats"][-1]["chi2"] < 1e-15


@pytest.mark.parametrize("name", ["mixed", "multi_scan", "reject"])
def test_trial_chi2_from_the_next_build_pass_is_bit_neutral(name, monkeypatch):
    recipe, niter = G.CASES[name]
    case = recipe()
    runs = []
    for v in ("1", "0"):
        monkeypatch.setenv("CUGO_TRIAL_FROM_BUILD", v)
        runs.append(run(case, niter))
    same_bits(runs[0], runs[1])
    monkeypatch.delenv("CUGO_TRIAL_FROM_BUILD")
    same_bits(runs[0], run(case, niter))


@pytest.mark.parametrize("form", FORMS)
def test_rejected_trials_rebuild_the_partials(form, monkeypatch):
    set_form(form, monkeypatch)
    case, niter, tr, pose, lm, tol, etol = reference("reject")
    assert sum(t["trials"] for t in tr) >= 1 and all(abs(t["rho"]) >= 0.1 for t in tr)
    out = run(case, niter)
    assert_trajectories_match(out["stats"], tr, tol)
    np.testing.assert_allclose(out["pose"], pose, rtol=0, atol=etol)


def test_a_set_that_counts_for_nothing_changes_no_bit():
    d, icp, prior, pts, rp, _, gp = G.mixed_case()
    base = run((d, icp, prior, pts, rp, None, None), 8)
    assert base["n_gicp_pair"] == 0
    off = dict(gp, active=np.zeros(len(gp["a"]), bool))
    out = run((d, icp, prior, pts, rp, None, off), 8)
    assert out["n_gicp_pair"] == 0 and out["nedges"] == base["nedges"] and out["sstats"]["hsc_blocks"] == base["sstats"]["hsc_blocks"]
    same_bits(base, out)


def test_covariances_with_gicp_pair_sets():
    """computeMarginals on multi_scan: Sigma = (the reference's Gauss-Newton H with Omega at the final poses)^-1, at the
    tolerance of test_point_pair_graph.py::test_covariances_with_pair_sets"""
    case = G.multi_scan_case()
    d = case[0]
    g = G.build_graph(*case)
    g.initialize()
    g.optimize(5)
    g.compute_covariances(poses=True, landmarks=False)
    ref = G.GicpGraph(dict(d, pose=g.poses()), case[1], G.RL.empty_prior(), None, None, None, case[6])
    S = np.linalg.inv(ref._pairs()[0])
    cov = g.pose_covariances()
    pidx, P = G.RL.free_first(d)
    for p in range(len(d["pose"])):
        if pidx[p] >= P:
            assert not cov[p].any()
            continue
        blk = S[6 * pidx[p]:6 * pidx[p] + 6, 6 * pidx[p]:6 * pidx[p] + 6]
        assert np.abs(cov[p] - blk).max() <= 1e-8 * np.linalg.norm(blk), p
    g.close()
