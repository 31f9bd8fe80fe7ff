"""Pose-pose point edge sets (PointPairEdgeSet) in the LM loop, on the GPU: the optimiser against the dense numpy LM of
tests/point_pair_lm_ref.py (the pair terms in float64, off-diagonal blocks included) under the default form of the loop
under CUGO_POSE_SCHUR=0 and without speculative build passes, and the relations between the forms.

Tolerance: the project's rule (conftest.golden_tolerances): relative chi2 per iteration within max(1e-10, 4 x the
self-sensitivity), estimates within max(1e-9, 4 x), the same trial counts, no decision at |rho| < 0.1.  The
self-sensitivity is measured by the reference ON ITSELF (its Schur solve against its full dense solve, and every pose
edge set in a permuted order) and printed."""
import importlib

import numpy as np
import pytest

import icp_lm_ref
import point_pair_lm_ref as R
import point_pair_ref as PP
from test_gpu import assert_trajectories_match

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
pytestmark = pytest.mark.gpu

_REF = {}
FORMS = ["default", "two_stream", "no_speculation"]


def reference(name):
    if name not in _REF:
        recipe, niter = R.CASES[name]
        d, icp, prior, pts, rp, pairs = recipe()
        tr, pose, lm, sens, est = R.reference_runs(d, icp, prior, pts, rp, pairs, niter)
        assert len(tr) == niter, (name, len(tr))
        assert all(abs(t["rho"]) >= 0.1 for t in tr), "a decision at rho near 0 is not a fair comparison"
        print("reference %s: self-sensitivity %.3g (chi2), %.3g (estimates); trials %s" % (name, max(sens), est, [t["trials"] for t in tr]))
        tol, etol = icp_lm_ref.tolerances(sens, est)
        _REF[name] = (d, icp, prior, pts, rp, pairs, niter, tr, pose, lm, tol, etol)
    return _REF[name]


def run(d, icp, prior, pts, rp, pairs, niter, timing=False):
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    g = R.build_graph(d, icp, prior, pts, rp, pairs)
    if timing:
        g.set_kernel_timing(1)
    g.initialize()
    g.optimize(niter)
    out = dict(stats=g.stats(), pose=g.poses(), lm=g.landmarks(), sstats=g.structure_stats(), nedges=g.n_active_edges(),
               n_pair=g.n_point_pair_edges())
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


def set_form(form, monkeypatch):
    if form == "two_stream":
        monkeypatch.setenv("CUGO_POSE_SCHUR", "0")
    if form == "no_speculation":
        monkeypatch.setenv("CUGO_SPECULATE", "0")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["multi_scan", "mixed", "huber"])
def test_lm_trajectory_against_the_reference(name, form, monkeypatch):
    """(a) a pure multi-scan graph, (b) next to BA edges, plane, line, point, prior and relative-pose sets that share pairs
    with it, (c) with Huber; under the default form, under CUGO_POSE_SCHUR=0 and under CUGO_SPECULATE=0"""
    set_form(form, monkeypatch)
    d, icp, prior, pts, rp, pairs, niter, tr, pose, lm, tol, etol = reference(name)
    out = run(d, icp, prior, pts, rp, pairs, niter, timing=True)
    for a, b in zip(out["stats"], tr):
        print(name, form, "chi2 %.15g ref %.15g rel %.3g lam %.6g ref %.6g trials %d ref %d" %
              (a["chi2"], b["chi2"], abs(a["chi2"] - b["chi2"]) / b["chi2"], a["lam"], b["lam"], a["trials"], b["trials"]))
    k = out["kernels"]
    assert launches(k, "k_point_pair_chunks_build") > 0 and "k_point_pair_check" not in k
    assert launches(k, "k_point_pair_offdiag") > 0
    if form != "two_stream":                   # the one-stream form: diagonal and off-diagonal sums behind k_pose_schur
        assert launches(k, "k_point_pair_add_schur") > 0     # (iteration 0 builds in the two-stream form)
    else:                                      # the build pass adds the diagonal sums, every Schur pass the off-diagonal ones
        assert launches(k, "k_point_pair_add") > 0 and launches(k, "k_point_pair_add_schur") == 0
    assert out["n_pair"] == R.counting_edges(d, pairs)
    assert_trajectories_match(out["stats"], tr, tol)
    np.testing.assert_allclose(out["pose"], pose, rtol=0, atol=etol)
    if len(lm):
        np.testing.assert_allclose(out["lm"], lm, rtol=0, atol=10 * etol)
    assert out["sstats"]["trial_sync_retries"] == 0


_ZERO = {}


def zero_noise_reference():
    """case (d) through the reference: chi2 falls to rounding level, where a relative comparison, a gain ratio and a trial
    count mean nothing; the iterations with chi2 above 1e-6 are held to the rule, the end to the truth"""
    if not _ZERO:
        d, icp, prior, pts, rp, pairs = R.zero_noise_case()
        tr, pose, lm, sens, est = R.reference_runs(d, icp, prior, pts, rp, pairs, 8)
        n = sum(t["chi2"] > 1e-6 for t in tr)
        assert n >= 2 and [t["trials"] for t in tr[:n]] == [0] * n, "the recipe no longer gives the trials it was chosen for"
        assert all(abs(t["rho"]) >= 0.1 for t in tr[:n]), "a decision at rho near 0 is not a fair comparison"
        print("reference zero_noise: self-sensitivity %.3g (chi2), %.3g (estimates)" % (max(sens[:n]), est))
        tol, etol = icp_lm_ref.tolerances(sens, est)
        _ZERO.update(d=d, pairs=pairs, tr=tr, n=n, tol=tol, etol=etol)
    return _ZERO


@pytest.mark.parametrize("form", FORMS)
def test_zero_noise_ends_at_the_truth(form, monkeypatch):
    """(d) exact correspondences, Omega = I, the start 0.25 rad / 0.8 m away: ends at the truth"""
    set_form(form, monkeypatch)
    z = zero_noise_reference()
    out = run(z["d"], [], None, None, None, z["pairs"], 8)
    print("zero noise", form, "chi2", [s["chi2"] for s in out["stats"]], "reference", [t["chi2"] for t in z["tr"]])
    n = z["n"]
    assert_trajectories_match(out["stats"][:n], z["tr"][:n], z["tol"][:n])
    np.testing.assert_allclose(out["pose"], z["d"]["pose_gt"], rtol=0, atol=z["etol"])
    assert out["stats"][-1]["chi2"] < 1e-15 and out["sstats"]["trial_sync_retries"] == 0


@pytest.mark.parametrize("name", ["mixed", "huber", "reject"])
def test_trial_chi2_from_the_next_build_pass_is_bit_neutral(name, monkeypatch):
    """the partials the off-diagonal pass reads are those of the build pass whose H the Schur pass consumed, whether a trial
    takes its chi2 from an error pass or from the next build pass (queued ahead with its Schur complement): the same bits,
    on a case with rejected trials too; and a fresh optimiser gives them again"""
    d, icp, prior, pts, rp, pairs = R.CASES[name][0]()
    niter = R.CASES[name][1]
    runs = []
    for v in ("1", "0"):
        monkeypatch.setenv("CUGO_TRIAL_FROM_BUILD", v)
        runs.append(run(d, icp, prior, pts, rp, pairs, niter))
    same_bits(runs[0], runs[1])
    monkeypatch.delenv("CUGO_TRIAL_FROM_BUILD")
    same_bits(runs[0], run(d, icp, prior, pts, rp, pairs, niter))


@pytest.mark.parametrize("form", FORMS)
def test_rejected_trials_rebuild_the_partials(form, monkeypatch):
    """a BA part that takes rejected trials: behind a rejection H is rebuilt at the estimates in force, and with it the
    partials the off-diagonal pass reads; the trajectory of the reference through the retries"""
    set_form(form, monkeypatch)
    d, icp, prior, pts, rp, pairs, niter, tr, pose, lm, tol, etol = reference("reject")
    assert sum(t["trials"] for t in tr) >= 1, "the recipe no longer takes a rejected trial"
    out = run(d, icp, prior, pts, rp, pairs, niter)
    assert_trajectories_match(out["stats"], tr, tol)
    np.testing.assert_allclose(out["pose"], pose, rtol=0, atol=etol)
    assert out["sstats"]["trial_sync_retries"] == 0


def test_a_set_that_counts_for_nothing_changes_no_bit():
    """pair edges all between fixed poses or all inactive, or no pair edge at all, next to a BA graph: bit for bit the run
    without them, and the pattern gains no block"""
    d, icp, prior, pts, rp, pairs = R.mixed_case()
    base = run(d, icp, prior, pts, rp, None, 8)
    assert base["n_pair"] == 0
    off = dict(pairs, active=np.zeros(len(pairs["a"]), bool))
    out = run(d, icp, prior, pts, rp, off, 8)
    assert out["n_pair"] == 0 and out["nedges"] == base["nedges"] and out["sstats"]["hsc_blocks"] == base["sstats"]["hsc_blocks"]
    same_bits(base, out)
    empty = dict(pairs, **{k: np.asarray(pairs[k])[:0] for k in ("a", "b", "p", "z", "active")}, info=pairs["info"][:1])
    same_bits(base, run(d, icp, prior, pts, rp, empty, 8))


def test_covariances_with_pair_sets():
    """computeMarginals of case (a) goes through Impl::queue_build and the two-stream Schur pass: Sigma = (the reference's
    dense H)^-1, zeros for the fixed pose"""
    d, icp, prior, pts, rp, pairs = R.multi_scan_case()
    g = R.build_graph(d, icp, prior, pts, rp, pairs)
    g.initialize()
    g.optimize(4)
    g.compute_covariances(poses=True, landmarks=False)
    ref = R.PairGraph(dict(d, pose=g.poses()), icp, R.RL.empty_prior(), pts, rp, pairs)
    A = ref._pairs()[0]
    S = np.linalg.inv(A)
    cov = g.pose_covariances()
    pidx, P = R.RL.free_first(d)
    for p in range(len(d["pose"])):
        if pidx[p] >= P:
            assert not cov[p].any()
            continue
        blk = S[6 * pidx[p]:6 * pidx[p] + 6, 6 * pidx[p]:6 * pidx[p] + 6]
        assert np.abs(cov[p] - blk).max() <= 1e-8 * np.linalg.norm(blk), p
    x = g.pose_cross_covariances([0], [1])[0]
    blk = S[6 * pidx[0]:6 * pidx[0] + 6, 6 * pidx[1]:6 * pidx[1] + 6]
    assert np.abs(x - blk).max() <= 1e-8 * np.linalg.norm(S)
    g.close()
