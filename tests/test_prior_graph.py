"""SE(3) pose prior sets in the LM loop, on the GPU: the optimiser against the dense numpy LM of tests/prior_ref.py
(icp_lm_ref.IcpGraph + prior_ref.reference_build) in the forms the loop takes, the relations between those forms that
tests/test_icp_graph.py asserts for ICP sets, and the covariance -> prior round trip.

Tolerance: the rule of icp_lm_ref.tolerances, computed from the reference's own runs: relative chi2 per iteration
within max(1e-10, 4 x the self-sensitivity), the same trial counts, estimates within max(1e-9, 4 x)."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import icp_lm_ref as R
import prior_ref as PR
import synth
from conftest import ROOT
from test_gpu import assert_trajectories_match

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
pytestmark = pytest.mark.gpu

_REF = {}


def reference(name):
    """(d, icp, prior, niter, reference trace, pose, lm, chi2 tolerances, estimate tolerance) of a case of prior_ref.CASES"""
    if name not in _REF:
        recipe, niter = PR.CASES[name]
        d, icp, prior = recipe()
        tr, pose, lm, sens, est = PR.reference_runs(d, icp, prior, niter)
        assert len(tr) == niter
        assert all(abs(t["rho"]) >= 0.1 for t in tr), "a decision at rho near 0 is not a fair comparison"
        print("reference %s: self-sensitivity %.3g (chi2), %.3g (estimates); trials %s" %
              (name, max(sens), est, [t["trials"] for t in tr]))
        tol, etol = R.tolerances(sens, est)
        _REF[name] = (d, icp, prior, niter, tr, pose, lm, tol, etol)
    return _REF[name]


def run(d, icp, prior, niter, float32=False, timing=False):
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    g = PR.build_graph(d, icp, prior)
    if float32:
        g.set_float32(1)
    if timing:
        g.set_kernel_timing(1)
    g.initialize()
    g.optimize(niter)
    out = dict(stats=g.stats(), pose=g.poses(), lm=g.landmarks(), sstats=g.structure_stats(), nedges=g.n_active_edges(),
               n_prior=g.n_prior_edges())
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


@pytest.mark.parametrize("pose_schur", ["1", "0"])
@pytest.mark.parametrize("name", list(PR.CASES))
def test_lm_trajectory_against_the_reference(name, pose_schur, monkeypatch):
    """gauge: no fixed pose, the gauge held by a prior; mixed: BA + plane + line + priors; reject: rejected trials;
    corridor: planes that leave one translation unobserved, which only the priors hold.  In the one-stream form of the
    loop (the prior terms are added behind k_pose_schur) and in the two-stream form (behind k_build_poses)"""
    monkeypatch.setenv("CUGO_POSE_SCHUR", pose_schur)
    d, icp, prior, niter, tr, pose, lm, tol, etol = reference(name)
    if name == "reject":
        assert sum(t["trials"] for t in tr) >= 1, "the recipe no longer takes a rejected trial"
    out = run(d, icp, prior, niter, timing=True)
    for a, b in zip(out["stats"], tr):
        print(name, pose_schur, "chi2 %.15g ref %.15g rel %.3g lam %.6g ref %.6g trials %d ref %d" %
              (a["chi2"], b["chi2"], abs(a["chi2"] - b["chi2"]) / b["chi2"], a["lam"], b["lam"], a["trials"], b["trials"]))
    k = out["kernels"]
    builds = launches(k, "k_prior_add") + launches(k, "k_prior_add_schur")
    assert launches(k, "k_prior_add") > 0 and "k_prior_check" not in k
    if pose_schur == "1":  # the default run really took the one-stream form, and the prior add behind it
        assert launches(k, "k_pose_schur") > 0 and launches(k, "k_prior_add_schur") > 0
    else:
        assert "k_pose_schur" not in k and "k_prior_add_schur" not in k
    # the launch budget: one prior launch per build pass or Schur pass that takes the terms, one per error pass, and one
    # chi2 total per call (iteration 0)
    # ("build", "schur", "errors": the groups Engine::optimize times, one count per pass)
    assert launches(k, "k_prior_chi_total") == 1
    assert launches(k, "k_prior_add") + launches(k, "k_prior_errors") <= launches(k, "build") + launches(k, "errors")
    assert launches(k, "k_prior_add_schur") <= launches(k, "schur") and builds >= niter
    assert_trajectories_match(out["stats"], tr, tol)
    np.testing.assert_allclose(out["pose"], pose, rtol=0, atol=etol)
    if len(lm):
        np.testing.assert_allclose(out["lm"], lm, rtol=0, atol=10 * etol)
    assert out["sstats"]["trial_sync_retries"] == 0
    if name == "corridor":  # the direction only the priors observe ends at the reference's value
        np.testing.assert_allclose(out["pose"][:, 4], pose[:, 4], rtol=0, atol=etol)
        assert out["sstats"]["hsc_blocks"] == 4


def subset_recipe(seed=21):
    """4 poses (pose 0 fixed) / 30 landmarks with BA edges, 600 plane edges on the free poses (two chunks of 512: the
    priors' totals start behind more than one chunk total; per-edge omega, Huber), 40 line edges (less than a chunk;
    pose 2 has none; one omega) and one dense-Omega prior per free pose"""
    d = synth.make_problem(n_poses=4, n_landmarks=30, seed=seed, fixed_poses=(0,))
    rng = np.random.default_rng(seed)
    pl = R.icp_edges(rng, d, [0, 250, 200, 150], "plane", 0.02)
    li = R.icp_edges(rng, d, [0, 25, 0, 15], "line", 0.02)
    kinds = dict(plane=("plane", pl, rng.uniform(0.5, 2.0, len(pl["pose"])) * 2e3, np.ones(len(pl["pose"]), bool),
                        (R.icp_ref.RK_HUBER, 4.0)),
                 line=("line", li, np.array([2.4e3]), np.ones(len(li["pose"]), bool), (R.icp_ref.RK_NONE, 1.0)))
    free = np.array([1, 2, 3])
    gt = d["pose_gt"]
    prior = PR.make_prior(free, [PR.displaced(rng, gt[p], 0.01, 0.05) for p in free], [PR.random_spd(rng, 50.0) for _ in free])
    return d, kinds, prior


_SUBSET_REF = {}
SUBSETS = [("plane",), ("line",), ("prior",), ("plane", "line"), ("plane", "prior"), ("line", "prior"),
           ("plane", "line", "prior")]


@pytest.mark.parametrize("subset", SUBSETS, ids="+".join)
def test_every_subset_of_pose_edge_kinds(subset, monkeypatch):
    """BA edges + every non-empty subset of {plane, line, prior}: an ICP kind alone (the other one's pose_ptr is all
    zeros), an ICP kind with priors, priors behind two chunk totals.  5 iterations in both forms of the loop against
    prior_ref.PriorGraph, by the comparison and the tolerance rule of test_lm_trajectory_against_the_reference (from
    reference_runs' own sensitivity), and two runs agree to the bit"""
    niter = 5
    d, kinds, prior = subset_recipe()
    icp = [kinds[k] for k in ("plane", "line") if k in subset]
    if subset not in _SUBSET_REF:
        none = PR.make_prior(prior["pose"][:0], prior["z"][:0], prior["info"][:1])
        tr, pose, lm, sens, est = PR.reference_runs(d, icp, prior if "prior" in subset else none, niter)
        assert len(tr) == niter
        assert all(abs(t["rho"]) >= 0.1 for t in tr), "a decision at rho near 0 is not a fair comparison"
        _SUBSET_REF[subset] = (tr, pose, lm) + R.tolerances(sens, est)
    tr, pose, lm, tol, etol = _SUBSET_REF[subset]
    for pose_schur in ("1", "0"):
        monkeypatch.setenv("CUGO_POSE_SCHUR", pose_schur)
        out = run(d, icp, prior if "prior" in subset else None, niter)
        for a, b in zip(out["stats"], tr):
            print("+".join(subset), pose_schur, "chi2 %.15g ref %.15g rel %.3g lam %.6g ref %.6g trials %d ref %d" %
                  (a["chi2"], b["chi2"], abs(a["chi2"] - b["chi2"]) / b["chi2"], a["lam"], b["lam"], a["trials"], b["trials"]))
        assert out["n_prior"] == (3 if "prior" in subset else 0)
        assert out["nedges"] == len(d["e_pose"]) + sum(len(k[1]["pose"]) for k in icp) + out["n_prior"]
        assert_trajectories_match(out["stats"], tr, tol)
        np.testing.assert_allclose(out["pose"], pose, rtol=0, atol=etol)
        np.testing.assert_allclose(out["lm"], lm, rtol=0, atol=10 * etol)
        assert out["sstats"]["trial_sync_retries"] == 0
        same_bits(out, run(d, icp, prior if "prior" in subset else None, niter))


def bit_cases():
    for name in ("gauge", "mixed", "reject"):
        d, icp, prior = PR.CASES[name][0]()
        yield name, d, icp, prior, PR.CASES[name][1]


def test_trial_chi2_from_the_next_build_pass_is_bit_neutral_with_prior_sets(monkeypatch):
    """CUGO_TRIAL_FROM_BUILD 1 / 0: the priors' chi2 at a trial's estimates out of the prior pass queued with the
    speculative build, or out of the error-only form in front of the tail: the same totals summed by the same launch"""
    for name, d, icp, prior, niter in bit_cases():
        runs = []
        for v in ("1", "0"):
            monkeypatch.setenv("CUGO_TRIAL_FROM_BUILD", v)
            runs.append(run(d, icp, prior, niter))
        same_bits(runs[0], runs[1])


def test_wait_forms_and_profile_mode_are_bit_neutral_with_prior_sets(monkeypatch):
    for name, d, icp, prior, niter in bit_cases():
        base = run(d, icp, prior, niter)
        same_bits(base, run(d, icp, prior, niter))  # two fresh optimisers: the same bits
        for var in ("CUGO_TRIAL_POLL", "CUGO_TRIAL_EVENT"):
            monkeypatch.setenv(var, "0")
            same_bits(base, run(d, icp, prior, niter))
            monkeypatch.delenv(var)
        monkeypatch.setenv("CUGO_SPECULATE", "0")
        nospec = run(d, icp, prior, niter)
        monkeypatch.delenv("CUGO_SPECULATE")
        monkeypatch.setenv("CUGO_PROFILE", "1")
        same_bits(nospec, run(d, icp, prior, niter))
        monkeypatch.delenv("CUGO_PROFILE")


@pytest.mark.parametrize("form", ["CUGO_HSC_ROWS", "CUGO_HSC_STRIP", "CUGO_SCHUR_PLAN"])
def test_opt_in_schur_forms_take_the_prior_terms(form, monkeypatch):
    """these forms read Hpp / bp, where the two-stream build pass adds the prior terms: the reference's trajectory"""
    monkeypatch.setenv(form, "1")
    d, icp, prior, niter, tr, pose, lm, tol, etol = reference("gauge")
    out = run(d, icp, prior, niter)
    assert_trajectories_match(out["stats"], tr, tol)
    np.testing.assert_allclose(out["pose"], pose, rtol=0, atol=etol)


def test_sets_that_count_for_nothing_change_no_bit():
    """priors all on fixed poses, or no prior at all, next to a BA graph: bit for bit the run without them"""
    d, icp, prior = PR.mixed_prior_case()
    ba = run(d, [], None, 8)
    assert ba["n_prior"] == 0
    fixed = np.asarray(d["pose_fixed"], bool)[prior["pose"]]
    assert fixed.sum() == 1
    on_fixed = PR.make_prior(prior["pose"][fixed], prior["z"][fixed], prior["info"][fixed], rk=prior["rk"])
    out = run(d, [], on_fixed, 8)
    assert out["n_prior"] == 0 and out["nedges"] == ba["nedges"]
    same_bits(ba, out)
    empty = PR.make_prior(prior["pose"][:0], prior["z"][:0], prior["info"][:1], rk=prior["rk"])
    same_bits(ba, run(d, [], empty, 8))


def test_float32_internal_mode_with_prior_sets():
    """the prior terms stay fp64 (they touch no stored block): the bar the fp32 ICP test states for the mode"""
    d, icp, prior, niter, tr, pose, lm, tol, etol = reference("mixed")
    out = run(d, icp, prior, niter, float32=True)
    assert_trajectories_match(out["stats"], tr, 1e-5, check_trials=False)
    assert [s["trials"] for s in out["stats"]] == [t["trials"] for t in tr]


def test_covariance_round_trip_through_a_prior():
    """Sigma_p of a free pose of a BA graph, handed back as a prior on a graph that holds only that pose: the same
    Sigma_p comes out (J = I at r = 0), within the slack of inverting twice in fp64, and the pose stays where it is"""
    d = synth.make_problem(n_poses=6, n_landmarks=60, seed=11)
    g = cugo.graph_from_arrays(d)
    g.initialize()
    g.optimize(5)
    g.compute_covariances(poses=True, landmarks=False)
    p = 3
    assert not d["pose_fixed"][p]
    sigma = g.pose_covariances([p])[0]
    est = g.poses([p])[0]
    g.close()
    assert np.abs(sigma).max() > 0
    omega = np.linalg.inv(sigma)
    omega = 0.5 * (omega + omega.T)
    one = dict(pose=est[None, :], pose_fixed=np.zeros(1, np.uint8), lm=np.zeros((0, 3)), lm_fixed=np.zeros(0, np.uint8),
               e_pose=np.zeros(0, np.int32), e_lm=np.zeros(0, np.int32), e_stereo=np.zeros(0, np.uint8),
               e_meas=np.zeros((0, 3)), e_omega=np.zeros(0), e_cam=np.zeros((0, 5)))
    h = PR.build_graph(one, [], PR.make_prior([0], est[None, :], omega[None]))
    h.initialize()
    h.compute_covariances(poses=True, landmarks=False)
    back = h.pose_covariances([0])[0]
    err = np.abs(back - sigma).max()
    print("round trip: |Sigma' - Sigma| = %.3g of %.3g, cond %.3g" % (err, np.abs(sigma).max(), np.linalg.cond(sigma)))
    assert err <= 1e-9 * np.abs(sigma).max()
    h.optimize(3)
    moved = np.abs(h.poses([0])[0] - est).max()
    print("the pose moved by %.3g" % moved)
    assert moved <= 1e-12
    h.close()


@pytest.mark.parametrize("mode", ["1", "2"])
def test_poisoned_allocations_change_nothing(mode):
    """CUGO_POISON_ALLOC (hip_util.h) in a child process, on this file's trajectory cases in both forms of the loop:
    nothing reads memory nobody wrote (workgroup totals, blocks of poses without priors)"""
    env = dict(os.environ, CUGO_POISON_ALLOC=mode)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p",
                        "no:cacheprovider", "-k", "against_the_reference or round_trip"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "guard zone" not in r.stderr
