"""Landmark prior sets in the LM loop, on the GPU: the optimiser against the dense numpy LM of tests/lm_prior_ref.py
(make_golden.Graph + the term in Hll, bl and chi2) in the forms the loop takes, the relations between those forms that
tests/test_prior_graph.py asserts for the pose priors, the marginal covariances with the prior terms and the
covariance -> prior round trip on a landmark.

Tolerance: the rule of icp_lm_ref.tolerances, computed from the reference's own runs: relative chi2 per iteration
within max(1e-10, 4 x the self-sensitivity), the same trial counts, estimates within max(1e-9, 4 x).

Covariances: against a dense numpy inverse of the full H (prior terms included) at the optimiser's estimates, every
diagonal block within 1e-8 of the block's norm — the tolerance tests/test_covariance.py (assert_blocks_match) applies
to the same quantities at graph level; the per-entry bound of tests/test_lm_cov.py is stated on the landmark kernel's own
device inputs, which a graph-level test does not see."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import icp_lm_ref as R
import lm_prior_ref as LR
from conftest import ROOT
from test_gpu import assert_trajectories_match

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
pytestmark = pytest.mark.gpu

_REF = {}


def reference(name):
    """(d, lmp, icp, prior, niter, reference trace, pose, lm, chi2 tolerances, estimate tolerance) of a case"""
    if name not in _REF:
        recipe, niter = LR.CASES[name]
        d, lmp, icp, prior = recipe()
        tr, pose, lm, sens, est = LR.reference_runs(d, lmp, niter, icp, prior)
        assert len(tr) == niter
        assert all(abs(t["rho"]) >= 0.1 for t in tr), "a decision at rho near 0 is not a fair comparison"
        print("reference %s: self-sensitivity %.3g (chi2), %.3g (estimates); trials %s" %
              (name, max(sens), est, [t["trials"] for t in tr]))
        tol, etol = R.tolerances(sens, est)
        _REF[name] = (d, lmp, icp, prior, niter, tr, pose, lm, tol, etol)
    return _REF[name]


def run(d, lmp, icp, prior, niter, float32=False, timing=False, keep=False):
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    g = LR.build_graph(d, lmp, icp, prior)
    if float32:
        g.set_float32(1)
    if timing:
        g.set_kernel_timing(1)
    g.initialize()
    g.optimize(niter)
    out = dict(stats=g.stats(), pose=g.poses(), lm=g.landmarks(), sstats=g.structure_stats(), nedges=g.n_active_edges(),
               n_lmp=g.n_landmark_prior_edges())
    if timing:
        out["kernels"] = g.kernel_times()
    if keep:
        out["g"] = g
    else:
        g.close()
    return out


def key(stats):
    return [(s["chi2"], s["lam"], s["trials"]) for s in stats]


def same_bits(a, b):
    assert key(a["stats"]) == key(b["stats"])
    assert np.array_equal(a["pose"], b["pose"]) and np.array_equal(a["lm"], b["lm"])


def launches(k, name):
    return k.get(name, dict(launches=0))["launches"]


def counting(d, lmp):
    return int((np.asarray(lmp["active"], bool) & (np.asarray(d["lm_fixed"])[lmp["lm"]] == 0)).sum())


FORMS = {"one_stream": {"CUGO_POSE_SCHUR": "1"}, "two_stream": {"CUGO_POSE_SCHUR": "0"}, "no_fuse": {"CUGO_FUSE_T": "0"}}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(LR.CASES))
def test_lm_trajectory_against_the_reference(name, form, monkeypatch):
    """tenth: BA + priors on a tenth of the landmarks; gauge: no fixed vertex, four landmark priors hold the gauge;
    single_mono: a landmark with one mono edge and a prior; reject: rejected trials; mixed: BA + plane + line + pose
    priors + landmark priors.  In the one-stream form of the fused build pass (G and the landmarks' lines carry the
    priors), in the two-stream fused form (invHll and T do) and without fusing (Hll / bl do)"""
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    d, lmp, icp, prior, niter, tr, pose, lm, tol, etol = reference(name)
    if name == "reject":
        assert sum(t["trials"] for t in tr) >= 1, "the recipe no longer takes a rejected trial"
    out = run(d, lmp, icp, prior, niter, timing=True)
    for a, b in zip(out["stats"], tr):
        print(name, form, "chi2 %.15g ref %.15g rel %.3g lam %.6g ref %.6g trials %d ref %d" %
              (a["chi2"], b["chi2"], abs(a["chi2"] - b["chi2"]) / b["chi2"], a["lam"], b["lam"], a["trials"], b["trials"]))
    assert out["n_lmp"] == counting(d, lmp)
    k = out["kernels"]
    if form == "one_stream":
        assert launches(k, "k_pose_schur") > 0
    else:
        assert "k_pose_schur" not in k
    # the launch budget: nothing in a build or Schur pass beyond the chi2 where it is taken, one launch per error pass
    # that is not taken from a build pass, one chi2 total per call (iteration 0); no add launch and no index check
    assert "k_lm_prior_add" not in k and "k_lm_prior_check" not in k
    assert launches(k, "k_lm_prior_chi_total") == 1
    assert 1 <= launches(k, "k_lm_prior_errors") <= launches(k, "errors") + 1
    assert_trajectories_match(out["stats"], tr, tol)
    np.testing.assert_allclose(out["pose"], pose, rtol=0, atol=etol)
    np.testing.assert_allclose(out["lm"], lm, rtol=0, atol=10 * etol)
    assert out["sstats"]["trial_sync_retries"] == 0


def bit_cases():
    for name in ("tenth", "reject", "mixed"):
        d, lmp, icp, prior = LR.CASES[name][0]()
        yield name, d, lmp, icp, prior, LR.CASES[name][1]


def test_trial_chi2_from_the_next_build_pass_is_bit_neutral_with_landmark_priors(monkeypatch):
    """CUGO_TRIAL_FROM_BUILD 1 / 0: the priors' chi2 at a trial's estimates out of the launch queued with the speculative
    build pass, or in front of the tail of an error pass: the same totals summed by the same launch"""
    for name, d, lmp, icp, prior, niter in bit_cases():
        runs = []
        for v in ("1", "0"):
            monkeypatch.setenv("CUGO_TRIAL_FROM_BUILD", v)
            runs.append(run(d, lmp, icp, prior, niter))
        same_bits(runs[0], runs[1])


def test_wait_forms_and_profile_mode_are_bit_neutral_with_landmark_priors(monkeypatch):
    for name, d, lmp, icp, prior, niter in bit_cases():
        base = run(d, lmp, icp, prior, niter)
        same_bits(base, run(d, lmp, icp, prior, niter))  # two fresh optimisers: the same bits
        for var in ("CUGO_TRIAL_POLL", "CUGO_TRIAL_EVENT"):
            monkeypatch.setenv(var, "0")
            same_bits(base, run(d, lmp, icp, prior, niter))
            monkeypatch.delenv(var)
        monkeypatch.setenv("CUGO_SPECULATE", "0")
        nospec = run(d, lmp, icp, prior, niter)
        monkeypatch.delenv("CUGO_SPECULATE")
        monkeypatch.setenv("CUGO_PROFILE", "1")
        same_bits(nospec, run(d, lmp, icp, prior, niter))
        monkeypatch.delenv("CUGO_PROFILE")


@pytest.mark.parametrize("form", ["CUGO_HSC_ROWS=1", "CUGO_HSC_STRIP=1", "CUGO_SCHUR_PLAN=1", "CUGO_HSC_MFMA=0", "CUGO_HSC_MFMA=2"])
def test_opt_in_schur_forms_take_the_prior_terms(form, monkeypatch):
    """these forms read Hll / bl (or invHll / T, or the landmarks' lines) as the build pass left them: the reference's
    trajectory"""
    var, val = form.split("=")
    monkeypatch.setenv(var, val)
    d, lmp, icp, prior, niter, tr, pose, lm, tol, etol = reference("gauge")
    out = run(d, lmp, icp, prior, niter)
    assert_trajectories_match(out["stats"], tr, tol)
    np.testing.assert_allclose(out["pose"], pose, rtol=0, atol=etol)
    np.testing.assert_allclose(out["lm"], lm, rtol=0, atol=10 * etol)


def test_sets_that_count_for_nothing_change_no_bit():
    """priors all on fixed landmarks, or no prior at all, next to a BA graph: bit for bit the run without them"""
    d, lmp, icp, prior = LR.tenth_case()
    ba = run(d, None, [], None, 6)
    assert ba["n_lmp"] == 0
    fixed = np.asarray(d["lm_fixed"], bool)[lmp["lm"]]
    assert fixed.sum() == 1
    on_fixed = LR.make_prior(lmp["lm"][fixed], lmp["z"][fixed], lmp["info"][fixed], rk=lmp["rk"])
    out = run(d, on_fixed, [], None, 6)
    assert out["n_lmp"] == 0 and out["nedges"] == ba["nedges"]
    same_bits(ba, out)
    empty = LR.make_prior(lmp["lm"][:0], lmp["z"][:0], lmp["info"][:1], rk=lmp["rk"])
    same_bits(ba, run(d, empty, [], None, 6))
    # and the priors that count do change the run
    assert key(run(d, lmp, [], None, 6)["stats"]) != key(ba["stats"])


def test_float32_internal_mode_with_landmark_priors():
    """the prior terms stay fp64 (they touch no stored block): the bar tests/test_prior_graph.py states for the mode"""
    d, lmp, icp, prior, niter, tr, pose, lm, tol, etol = reference("mixed")
    out = run(d, lmp, icp, prior, niter, float32=True)
    assert_trajectories_match(out["stats"], tr, 1e-5, check_trials=False)
    assert [s["trials"] for s in out["stats"]] == [t["trials"] for t in tr]


def dense_inverse(d, lmp, icp, prior, pose, lm):
    """H^-1 over the free vertices from the reference's normal equations (prior terms included) at the given estimates;
    (inverse, offset of every pose's block or -1, offset of every landmark's block or -1)"""
    g = LR.LmPriorGraph(d, lmp, icp, prior)
    g.pose[:], g.lm[:] = pose, lm
    H, _ = g.normal_equations()
    ip = np.where(g.pf, -1, 6 * g.pidx)
    il = np.where(g.lf, -1, 6 * g.np_ + 3 * g.lidx)
    return np.linalg.inv(H), ip, il


@pytest.mark.parametrize("name", ["tenth", "gauge", "single_mono"])
def test_covariances_carry_the_prior_terms(name):
    """compute_covariances runs the two-stream build pass, whose Hll holds the priors: poses and landmarks against the
    dense inverse.  gauge: without the priors H is singular (no fixed vertex); single_mono: without its prior the
    landmark's Hll is (a rank-2 matrix)"""
    d, lmp, icp, prior, niter = LR.CASES[name][0]() + (LR.CASES[name][1],)
    out = run(d, lmp, icp, prior, niter, keep=True)
    g = out["g"]
    g.compute_covariances()
    inv, ip, il = dense_inverse(d, lmp, icp, prior, out["pose"], out["lm"])
    cp, cl = g.pose_covariances(), g.landmark_covariances()
    worst = [0.0, 0.0]
    for blocks, offs, w, k in ((cp, ip, 6, 0), (cl, il, 3, 1)):
        for i, o in enumerate(offs):
            if o < 0:
                assert not blocks[i].any()
                continue
            ref = inv[o:o + w, o:o + w]
            worst[k] = max(worst[k], np.abs(blocks[i] - ref).max() / np.linalg.norm(ref))
    print("%s: covariance blocks off by %.3g (poses), %.3g (landmarks) of the block norm" % (name, worst[0], worst[1]))
    assert worst[0] <= 1e-8 and worst[1] <= 1e-8
    # the landmarks with a strong prior are the ones it pins: Sigma_l <= Omega^-1
    if name == "gauge":
        for l in lmp["lm"]:
            assert np.linalg.eigvalsh(cl[l]).max() <= 1e-6 * (1 + 1e-6)
    g.close()


def test_covariance_round_trip_through_a_landmark_prior():
    """Sigma_l of a free landmark handed back as a prior (Omega = Sigma_l^-1, Z = X) on a graph in which only that
    landmark and its observers' edges to it remain, the observers fixed: the estimate is a fixed point, and the
    landmark's covariance with the prior alone is Sigma_l again"""
    d, lmp, icp, prior = LR.tenth_case()
    out = run(d, lmp, icp, prior, 6, keep=True)
    g = out["g"]
    g.compute_covariances(poses=False, landmarks=True)
    l = 40
    assert not d["lm_fixed"][l] and (d["e_lm"] == l).sum() >= 2
    sigma = g.landmark_covariances([l])[0]
    g.close()
    omega = np.linalg.inv(sigma)
    omega = 0.5 * (omega + omega.T)
    # the dropped observers: every pose fixed at the optimum, the landmark alone free, one edge kept so that the landmark
    # has an edge slot, with zero information (it holds no information of its own: the prior is all there is)
    es = np.flatnonzero(d["e_lm"] == l)[:1]
    one = dict(pose=out["pose"], pose_fixed=np.ones(len(out["pose"]), np.uint8), lm=out["lm"][l][None, :],
               lm_fixed=np.zeros(1, np.uint8), e_pose=d["e_pose"][es], e_lm=np.zeros(1, np.int32), e_stereo=d["e_stereo"][es],
               e_meas=d["e_meas"][es], e_omega=np.zeros(1), e_cam=d["e_cam"][es])
    back_prior = LR.make_prior([0], out["lm"][l][None, :], omega[None])
    h = LR.build_graph(one, back_prior)
    h.initialize()
    assert h.n_landmark_prior_edges() == 1
    h.compute_covariances(poses=False, landmarks=True)
    back = h.landmark_covariances([0])[0]
    err = np.abs(back - sigma).max()
    print("round trip: |Sigma' - Sigma| = %.3g of %.3g, cond %.3g" % (err, np.abs(sigma).max(), np.linalg.cond(sigma)))
    assert err <= 1e-9 * np.abs(sigma).max()
    h.optimize(3)
    moved = np.abs(h.landmarks([0])[0] - out["lm"][l]).max()
    print("the landmark moved by %.3g" % moved)
    assert moved <= 1e-12
    h.close()


@pytest.mark.parametrize("mode", ["1", "2"])
def test_poisoned_allocations_change_nothing(mode):
    """CUGO_POISON_ALLOC (hip_util.h) in a child process, on this file's trajectory cases in the forms of the loop:
    nothing reads memory nobody wrote (workgroup totals, blocks of landmarks without priors)"""
    env = dict(os.environ, CUGO_POISON_ALLOC=mode)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p",
                        "no:cacheprovider", "-k", "against_the_reference or round_trip"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "guard zone" not in r.stderr
