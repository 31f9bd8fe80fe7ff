"""Point-to-plane / point-to-line edge sets in the LM loop, on the GPU: the optimiser against the dense numpy LM of
tests/icp_lm_ref.py (make_golden.Graph + icp_ref.reference_build) in every form the loop takes — the one-stream
iteration, the two-stream one, speculative build passes, trials whose chi2 comes out of the next build pass, rejected
trials — and the relations between those forms that tests/test_gpu.py asserts for BA graphs.

Tolerance: the project's rule (conftest.golden_tolerances): relative chi2 per iteration within max(1e-10, 4 x the
self-sensitivity), the same trial counts, lambda as in assert_trajectories_match.  The self-sensitivity is measured by
the reference ON ITSELF (its Schur solve against its full dense solve, and the ICP edges in a permuted order)."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import icp_lm_ref as R
import icp_ref
from conftest import ROOT
from test_gpu import assert_trajectories_match

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
pytestmark = pytest.mark.gpu

_REF = {}


def reference(name):
    """(d, icp, niter, reference trace, pose, lm, chi2 tolerances, estimate tolerance) of a case of icp_lm_ref.CASES"""
    if name not in _REF:
        recipe, niter, trials = R.CASES[name]
        d, icp = recipe()
        tr, pose, lm, sens, est = R.reference_runs(d, icp, niter)
        assert [t["trials"] for t in tr] == trials, "the recipe no longer gives the trials it was chosen for"
        assert all(abs(t["rho"]) >= 0.1 for t in tr), "a decision at rho near 0 is not a fair comparison"
        print("reference %s: self-sensitivity %.3g (chi2), %.3g (estimates)" % (name, max(sens), est))
        tol, etol = R.tolerances(sens, est)
        _REF[name] = (d, icp, niter, tr, pose, lm, tol, etol)
    return _REF[name]


def run(d, icp, niter, float32=False, timing=False, again=0):
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    g = R.build_graph(d, icp)
    if float32:
        g.set_float32(1)
    if timing:
        g.set_kernel_timing(1)
    g.initialize()
    g.optimize(niter)
    out = dict(stats=g.stats(), pose=g.poses(), lm=g.landmarks(), sstats=g.structure_stats(), nedges=g.n_active_edges(),
               n_icp=(g.n_icp_edges(cugo.ICP_PLANE), g.n_icp_edges(cugo.ICP_LINE)))
    if timing:
        out["kernels"] = g.kernel_times()
    if again:
        g.optimize(again)
        out["stats2"], out["pose2"], out["lm2"] = g.stats(), g.poses(), g.landmarks()
    g.close()
    return out


def key(stats):
    return [(s["chi2"], s["lam"], s["trials"]) for s in stats]


def same_bits(a, b):
    assert key(a["stats"]) == key(b["stats"])
    assert np.array_equal(a["pose"], b["pose"]) and np.array_equal(a["lm"], b["lm"])


@pytest.mark.parametrize("pose_schur", ["1", "0"])
@pytest.mark.parametrize("name", list(R.CASES))
def test_lm_trajectory_against_the_reference(name, pose_schur, monkeypatch):
    """the four cases, in the one-stream form of the loop (k_pose_schur forms the diagonal blocks of Hsc, bp and bsc;
    the ICP sums are added behind it) and in the two-stream form (they are added to Hpp / bp behind k_build_poses)"""
    monkeypatch.setenv("CUGO_POSE_SCHUR", pose_schur)
    d, icp, niter, tr, pose, lm, tol, etol = reference(name)
    out = run(d, icp, niter, timing=True)
    for a, b in zip(out["stats"], tr):
        print(name, pose_schur, "chi2 %.15g ref %.15g rel %.3g lam %.6g ref %.6g trials %d ref %d" %
              (a["chi2"], b["chi2"], abs(a["chi2"] - b["chi2"]) / b["chi2"], a["lam"], b["lam"], a["trials"], b["trials"]))
    k = out["kernels"]
    if pose_schur == "1":  # the default run really took the one-stream form, and the ICP add behind it
        assert k.get("k_pose_schur", dict(launches=0))["launches"] > 0
        assert k.get("k_icp_add_schur", dict(launches=0))["launches"] > 0
    else:
        assert "k_pose_schur" not in k and "k_icp_add_schur" not in k
    assert k["k_icp_add"]["launches"] > 0 and k["k_icp_chunks_build"]["launches"] > 0
    assert "k_icp_check" not in k
    assert_trajectories_match(out["stats"], tr, tol)
    np.testing.assert_allclose(out["pose"], pose, rtol=0, atol=etol)
    if len(lm):
        np.testing.assert_allclose(out["lm"], lm, rtol=0, atol=10 * etol)
    assert out["sstats"]["trial_sync_retries"] == 0


def medium_mixed(n_plane=20000, seed=12):
    d = cugo.synth(200, 3000, 12500, seed=seed, n_loop_closures=100)
    rng = np.random.default_rng(seed)
    pose_of_edge = rng.integers(0, 200, n_plane).astype(np.int32)
    pl = icp_ref.make_edges(rng, pose_of_edge, "plane", d["pose"], noise=0.05)
    li = icp_ref.make_edges(rng, rng.integers(0, 200, 300).astype(np.int32), "line", d["pose"], noise=0.05)
    icp = [("plane", pl, np.array([40.0]), np.ones(n_plane, bool), (icp_ref.RK_HUBER, 2.0)),
           ("line", li, rng.uniform(20, 60, 300), np.ones(300, bool), (icp_ref.RK_NONE, 1.0))]
    return d, icp


def bit_cases():
    for name in ("mixed", "reject"):
        d, icp = R.CASES[name][0]()
        yield name, d, icp, R.CASES[name][1]
    d, icp = medium_mixed()
    yield "medium", d, icp, 8


def test_trial_chi2_from_the_next_build_pass_is_bit_neutral_with_icp_sets(monkeypatch):
    """CUGO_TRIAL_FROM_BUILD 1 / 0: the ICP chi2 at a trial's estimates out of the ICP build pass queued with the
    speculative build, or out of an ICP error pass in front of the tail: the same chunk totals summed by the same launch"""
    for name, d, icp, niter in bit_cases():
        runs = []
        for v in ("1", "0"):
            monkeypatch.setenv("CUGO_TRIAL_FROM_BUILD", v)
            runs.append(run(d, icp, niter))
        same_bits(runs[0], runs[1])


def test_wait_forms_and_profile_mode_are_bit_neutral_with_icp_sets(monkeypatch):
    for name, d, icp, niter in bit_cases():
        base = run(d, icp, niter)
        again = run(d, icp, niter)  # two fresh optimisers: the same bits
        same_bits(base, again)
        assert base["sstats"]["trial_sync_retries"] == 0
        for var in ("CUGO_TRIAL_POLL", "CUGO_TRIAL_EVENT"):
            monkeypatch.setenv(var, "0")
            same_bits(base, run(d, icp, niter))
            monkeypatch.delenv(var)
        monkeypatch.setenv("CUGO_SPECULATE", "0")
        nospec = run(d, icp, niter)
        monkeypatch.delenv("CUGO_SPECULATE")
        monkeypatch.setenv("CUGO_PROFILE", "1")
        same_bits(nospec, run(d, icp, niter))
        monkeypatch.delenv("CUGO_PROFILE")


@pytest.mark.parametrize("form", ["CUGO_HSC_ROWS", "CUGO_HSC_STRIP", "CUGO_SCHUR_PLAN"])
def test_opt_in_schur_forms_take_the_icp_terms(form, monkeypatch):
    """these forms read Hpp / bp, where the two-stream build pass adds the ICP terms: the reference's trajectory"""
    monkeypatch.setenv(form, "1")
    d, icp, niter, tr, pose, lm, tol, etol = reference("mixed")
    out = run(d, icp, niter)
    assert_trajectories_match(out["stats"], tr, tol)
    np.testing.assert_allclose(out["pose"], pose, rtol=0, atol=etol)


def test_sets_that_count_for_nothing_change_no_bit():
    """ICP edges all on fixed poses, or sets with zero edges, next to a BA graph: bit for bit the run without them"""
    d, icp = R.mixed_case()
    ba = run(d, [], 8)
    assert ba["n_icp"] == (0, 0)
    on_fixed = []
    for kind, e, om, act, rk in icp:
        sel = np.asarray(d["pose_fixed"], bool)[e["pose"]]
        on_fixed.append((kind, {k: v[sel] for k, v in e.items()}, om[sel] if len(om) > 1 else om, act[sel], rk))
    assert sum(len(e[1]["pose"]) for e in on_fixed) == 31
    out = run(d, on_fixed, 8)
    assert out["n_icp"] == (0, 0) and out["nedges"] == ba["nedges"]
    same_bits(ba, out)
    empty = [(kind, {k: v[:0] for k, v in e.items()}, om[:0] if len(om) > 1 else om, act[:0], rk) for kind, e, om, act, rk in icp]
    same_bits(ba, run(d, empty, 8))


def medium_icp_only(seed=4):
    """300 free poses + 1 fixed, ~600 k plane and 6 k line edges, one pose with 1e5 plane edges"""
    rng = np.random.default_rng(seed)
    P = 301
    gt = np.array([icp_ref.random_pose(rng, rot=0.3, trans=20.0) for _ in range(P)])
    pose = gt.copy()
    for i in range(P - 1):
        pose[i] = icp_ref.left_update(gt[i], np.concatenate([rng.normal(0, 0.05, 3), rng.normal(0, 0.3, 3)]))
    pf = np.zeros(P, np.uint8)
    pf[P - 1] = 1
    d = dict(pose=pose, pose_fixed=pf, lm=np.zeros((0, 3)), lm_fixed=np.zeros(0, np.uint8),
             e_pose=np.zeros(0, np.int32), e_lm=np.zeros(0, np.int32), e_stereo=np.zeros(0, np.uint8),
             e_meas=np.zeros((0, 3)), e_omega=np.zeros(0), e_cam=np.zeros((0, 5)), pose_gt=gt)
    per_pose = rng.integers(1200, 2200, P)
    per_pose[17] = 100000
    per_pose[40] = 0
    pe = np.repeat(np.arange(P, dtype=np.int32), per_pose)
    rng.shuffle(pe)
    pl = icp_ref.make_edges(rng, pe, "plane", gt, noise=0.03)
    le = np.repeat(np.arange(P, dtype=np.int32), 20)
    rng.shuffle(le)
    li = icp_ref.make_edges(rng, le, "line", gt, noise=0.03)
    icp = [("plane", pl, np.array([100.0]), np.ones(len(pe), bool), (icp_ref.RK_HUBER, 1.0)),
           ("line", li, rng.uniform(50, 200, len(le)), np.ones(len(le), bool), (icp_ref.RK_CAUCHY, 2.0))]
    return d, icp


def test_medium_icp_only_graph_against_the_vectorised_reference():
    d, icp = medium_icp_only()
    assert len(icp[0][1]["pose"]) > 550000
    tr, pose = R.icp_only_lm(d, icp, 3)
    tr2, pose2 = R.icp_only_lm(d, R.permuted(icp), 3)
    assert [t["trials"] for t in tr] == [t["trials"] for t in tr2]
    sens = [abs(a["chi2"] - b["chi2"]) / abs(a["chi2"]) for a, b in zip(tr, tr2)]
    est = float(np.abs(pose - pose2).max())
    print("medium ICP-only: self-sensitivity %.3g (chi2) %.3g (estimates); rho %s" % (max(sens), est, [t["rho"] for t in tr]))
    assert all(abs(t["rho"]) >= 0.1 for t in tr)
    tol, etol = R.tolerances(sens, est)
    out = run(d, icp, 3)
    for a, b in zip(out["stats"], tr):
        print("chi2 %.15g ref %.15g rel %.3g" % (a["chi2"], b["chi2"], abs(a["chi2"] - b["chi2"]) / b["chi2"]))
    assert out["sstats"]["hsc_blocks"] == 300
    assert_trajectories_match(out["stats"], tr, tol)
    np.testing.assert_allclose(out["pose"], pose, rtol=0, atol=etol)


def test_float32_internal_mode_with_icp_sets():
    """the ICP terms stay fp64 (they touch no stored block): the bar test_float32_block_storage states for the mode"""
    d, icp, niter, tr, pose, lm, tol, etol = reference("mixed")
    out = run(d, icp, niter, float32=True)
    assert_trajectories_match(out["stats"], tr, 1e-5, check_trials=False)
    assert [s["trials"] for s in out["stats"]] == [t["trials"] for t in tr]


def dense_inverse_with_icp(d, icp, pose, lm):
    """as test_covariance.dense_inverse: H^-1 over the free vertices from the oracle's normal equations at (pose, lm),
    with the per-pose ICP blocks of reference_build added"""
    from test_covariance import oracle_problem
    prob = oracle_problem(d, pose=pose, lm=lm)
    pi, li, npf, nlf = prob.indices()
    sysm = prob.build_system()
    fp = (prob.pose_fixed == 0) & (pi < npf)
    fl = (prob.lm_fixed == 0) & (li < nlf)
    n = 6 * npf + 3 * nlf
    H = np.zeros((n, n))
    Hi = R.IcpGraph(dict(d, pose=pose, lm=lm), icp)._icp()[0]  # free-first, as the oracle indexes
    for p in range(npf):
        H[6 * p:6 * p + 6, 6 * p:6 * p + 6] = sysm["Hpp"][p].reshape(6, 6).T + Hi[p]
    for l in range(nlf):
        o = 6 * npf + 3 * l
        H[o:o + 3, o:o + 3] = sysm["Hll"][l].reshape(3, 3).T
    for e in range(prob.n_edges):
        p, l = prob.e_pose[e], prob.e_lm[e]
        if fp[p] and fl[l]:
            a, o = 6 * pi[p], 6 * npf + 3 * li[l]
            blk = sysm["Hpl"][e].reshape(3, 6).T
            H[a:a + 6, o:o + 3] += blk
            H[o:o + 3, a:a + 6] += blk.T
    return np.linalg.inv(H), np.where(fp, 6 * pi, -1), np.where(fl, 6 * npf + 3 * li, -1)


def test_covariances_with_icp_sets():
    from test_covariance import assert_blocks_match
    # mixed: the dense inverse of (the oracle's H + the ICP blocks) at the estimates the optimiser ended with
    d, icp = R.mixed_case()
    g = R.build_graph(d, icp)
    g.initialize()
    g.optimize(5)
    pose, lm = g.poses(), g.landmarks()
    g.compute_covariances()
    inv, ip, il = dense_inverse_with_icp(d, icp, pose, lm)
    assert_blocks_match(g, inv, ip, il)
    # ... and the optimiser is left as it was found: optimize(5); compute_covariances(); optimize(5) = optimize(5) x 2
    g.optimize(5)
    plain = run(d, icp, 5, again=5)
    assert key(g.stats()) == key(plain["stats2"])
    assert np.array_equal(g.poses(), plain["pose2"]) and np.array_equal(g.landmarks(), plain["lm2"])
    g.close()
    # ICP only: Sigma_p = (sum w J^T J)^-1 per pose, zeros for the fixed one
    d, icp = R.icp_only_case()
    g = R.build_graph(d, icp)
    g.initialize()
    g.optimize(5)
    g.compute_covariances(poses=True, landmarks=False)
    Hi = R.IcpGraph(dict(d, pose=g.poses()), icp)._icp()[0]
    cov = g.pose_covariances()
    for p in range(5):
        ref = np.linalg.inv(Hi[p])
        assert np.abs(cov[p] - ref).max() <= 1e-8 * np.linalg.norm(ref), p
    assert not cov[5].any()
    g.close()


@pytest.mark.parametrize("mode", ["1", "2"])
def test_poisoned_allocations_change_nothing(mode):
    """CUGO_POISON_ALLOC (hip_util.h) in a child process, on the mixed and the ICP-only case in both forms of the loop:
    nothing reads memory nobody wrote (partial slots of poses without ICP edges, bl[0] when no landmark exists)"""
    env = dict(os.environ, CUGO_POISON_ALLOC=mode)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p",
                        "no:cacheprovider", "-k", "against_the_reference and (mixed or icp_only) and not mixed_far"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "guard zone" not in r.stderr
