"""Relative-pose SE(3) edge sets in the LM loop, on the GPU: the optimiser against the dense numpy LM of
tests/relpose_lm_ref.py (prior_ref.PriorGraph + relpose_ref.reference_build) in the forms the loop takes, the relations
between those forms that tests/test_prior_graph.py asserts for prior sets, marginal covariances, and the two launches of
the two-stream form at kernel level.

Tolerance: the rule of icp_lm_ref.tolerances, computed from the reference's own runs: relative chi2 per iteration
within max(1e-10, 4 x the self-sensitivity), the same trial counts, estimates within max(1e-9, 4 x)."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import icp_ref
import prior_ref as PR
import relpose_lm_ref as L
import relpose_ref as RR
from conftest import ROOT
from test_gpu import assert_trajectories_match

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
pytestmark = pytest.mark.gpu

RELPOSE_KERNELS = ("k_relpose_add", "k_relpose_add_schur", "k_relpose_add_offdiag", "k_relpose_errors")


def run(d, icp, prior, rp, niter, float32=False, timing=False, covariances=False, hook=None):
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    g = L.build_graph(d, icp, prior, rp)
    if float32:
        g.set_float32(1)
    if timing:
        g.set_kernel_timing(1)
    if hook:
        hook(g)
    g.initialize()
    g.optimize(niter)
    out = dict(stats=g.stats(), pose=g.poses(), lm=g.landmarks(), sstats=g.structure_stats(), nedges=g.n_active_edges(),
               n_relpose=g.n_relpose_edges())
    if timing:
        out["kernels"] = g.kernel_times()
    if covariances:
        g.compute_covariances(poses=True, landmarks=False)
        out["cov"] = g.pose_covariances(np.arange(len(d["pose"])))
    g.close()
    return out


def key(stats):
    return [(s["chi2"], s["lam"], s["trials"]) for s in stats]


def same_bits(a, b):
    assert key(a["stats"]) == key(b["stats"])
    assert np.array_equal(a["pose"], b["pose"]) and np.array_equal(a["lm"], b["lm"])


def launches(k, name):
    return k.get(name, dict(launches=0))["launches"]


def print_trajectory(tag, stats, tr):
    for a, b in zip(stats, tr):
        print(tag, "chi2 %.15g ref %.15g rel %.3g lam %.6g ref %.6g trials %d ref %d" %
              (a["chi2"], b["chi2"], abs(a["chi2"] - b["chi2"]) / b["chi2"], a["lam"], b["lam"], a["trials"], b["trials"]))


@pytest.mark.parametrize("pose_schur", ["1", "0"])
@pytest.mark.parametrize("name", list(L.CASES))
def test_lm_trajectory_against_the_reference(name, pose_schur, monkeypatch):
    """chain: a pure pose graph with a fixed end, a closure and a doubled pair; gauge: a ring held by one prior, Huber;
    mixed: BA + plane + line + prior + relative-pose edges, pairs with and without common landmarks; reject: rejected
    trials.  In the one-stream form of the loop (every term behind k_pose_schur, one launch) and in the two-stream form
    (diagonal terms behind k_build_poses, off-diagonal terms behind the Schur pass)"""
    monkeypatch.setenv("CUGO_POSE_SCHUR", pose_schur)
    d, icp, prior, rp, niter, tr, pose, lm, tol, etol = L.reference(name)
    out = run(d, icp, prior, rp, niter, timing=True)
    print_trajectory("%s %s" % (name, pose_schur), out["stats"], tr)
    k = out["kernels"]
    print({n: launches(k, n) for n in RELPOSE_KERNELS + ("k_relpose_chi_total", "build", "schur", "errors", "k_pose_schur")})
    assert out["n_relpose"] == L.counting_edges(d, rp)
    assert out["sstats"]["hsc_blocks"] == L.union_pattern_blocks(d, rp)
    if pose_schur == "1":  # the default run really took the one-stream form, and the relative-pose add behind it
        assert launches(k, "k_pose_schur") > 0 and launches(k, "k_relpose_add_schur") > 0
    else:
        assert "k_pose_schur" not in k and "k_relpose_add_schur" not in k
    # the two-stream passes (all of them with CUGO_POSE_SCHUR=0, iteration 0 and retried trials otherwise) add the
    # off-diagonal terms behind their Schur pass
    assert launches(k, "k_relpose_add_offdiag") > 0 and launches(k, "k_relpose_add") > 0
    # the launch budget: at most one launch per build pass, per Schur pass and per error pass, one chi2 total per call
    assert launches(k, "k_relpose_chi_total") == 1
    assert launches(k, "k_relpose_add") + launches(k, "k_relpose_errors") <= launches(k, "build") + launches(k, "errors")
    assert launches(k, "k_relpose_add_schur") + launches(k, "k_relpose_add_offdiag") <= launches(k, "schur")
    assert launches(k, "k_relpose_add") + launches(k, "k_relpose_add_schur") >= niter
    assert_trajectories_match(out["stats"], tr, tol)
    np.testing.assert_allclose(out["pose"], pose, rtol=0, atol=etol)
    if len(lm):
        np.testing.assert_allclose(out["lm"], lm, rtol=0, atol=10 * etol)
    assert out["sstats"]["trial_sync_retries"] == 0


def test_chain_goes_through_the_sparse_cholesky_to_the_dense_gauss_newton_solution():
    """the pure pose graph is no block-diagonal system: the pattern holds the pairs, and the poses the optimiser ends at
    are those of a dense Gauss-Newton iteration in numpy on the same cost.  (One optimize() stops 2e-8 from that point,
    where the damped steps no longer gain 1e-6 of their prediction; a second and a third call, each starting from
    lambda = 1e-5 max diag again, take it to 2e-10: the reference LM called the same way does the same.)"""
    d, icp, prior, rp, niter, tr, pose, lm, tol, etol = L.reference("chain")
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    g = L.build_graph(d, icp, prior, rp)
    g.initialize()
    for n in (6, 3, 3):
        g.optimize(n)
    got, sstats = g.poses(), g.structure_stats()
    g.close()
    n_free = int((np.asarray(d["pose_fixed"]) == 0).sum())
    assert sstats["hsc_blocks"] > n_free and sstats["nnzL"] > 0
    gn = L.RelPoseGraph(d, icp, prior, rp)
    for _ in range(30):
        H, b = gn.normal_equations()
        dx = np.linalg.solve(H, b)
        gn.apply(dx)
        if np.abs(dx).max() < 1e-13:
            break
    print("Gauss-Newton: last step %.3g; optimiser against it %.3g (etol %.3g)" %
          (np.abs(dx).max(), np.abs(got - gn.pose).max(), etol))
    np.testing.assert_allclose(got, gn.pose, rtol=0, atol=etol)


def bit_cases():
    for name in ("chain", "mixed", "reject"):
        d, icp, prior, rp = L.CASES[name][0]()
        yield name, d, icp, prior, rp, L.CASES[name][1]


def test_sets_that_count_for_nothing_change_no_bit():
    """an empty set, a set whose edges are all inactive and a set between fixed poses only, next to a BA + ICP + prior
    graph with two fixed poses: bit for bit the run without the set, and no relative-pose launch"""
    d, icp, prior, rp = L.mixed_case()
    d = dict(d, pose_fixed=np.asarray(d["pose_fixed"]).copy())
    d["pose_fixed"][4] = 1  # (poses 0 and 4 fixed)
    base = run(d, icp, prior, None, 8, timing=True)
    assert base["n_relpose"] == 0 and not any(n in base["kernels"] for n in RELPOSE_KERNELS)
    empty = RR.make_edges(rp["a"][:0], rp["b"][:0], rp["z"][:0], rp["info"][:1], rk=rp["rk"])
    out = run(d, icp, prior, empty, 8, timing=True)
    same_bits(base, out)
    assert not any(n in out["kernels"] for n in RELPOSE_KERNELS + ("k_relpose_chi_total",))
    fixed_only = RR.make_edges([0, 4], [4, 0], rp["z"][:2], rp["info"][:2], rk=rp["rk"])
    out = run(d, icp, prior, fixed_only, 8)
    assert out["n_relpose"] == 0 and out["nedges"] == base["nedges"] and out["sstats"]["hsc_blocks"] == base["sstats"]["hsc_blocks"]
    same_bits(base, out)
    out = run(d, icp, prior, rp, 8, hook=lambda g: g.set_relpose_active(np.zeros(len(rp["a"]), bool)))
    assert out["n_relpose"] == 0 and out["nedges"] == base["nedges"] and out["sstats"]["hsc_blocks"] == base["sstats"]["hsc_blocks"]
    same_bits(base, out)


def test_trial_chi2_from_the_next_build_pass_is_bit_neutral_with_relpose_sets(monkeypatch):
    for name, d, icp, prior, rp, niter in bit_cases():
        runs = []
        for v in ("1", "0"):
            monkeypatch.setenv("CUGO_TRIAL_FROM_BUILD", v)
            runs.append(run(d, icp, prior, rp, niter))
        same_bits(runs[0], runs[1])


def test_wait_forms_and_profile_mode_are_bit_neutral_with_relpose_sets(monkeypatch):
    for name, d, icp, prior, rp, niter in bit_cases():
        base = run(d, icp, prior, rp, niter)
        same_bits(base, run(d, icp, prior, rp, niter))  # two fresh optimisers: the same bits
        for var in ("CUGO_TRIAL_POLL", "CUGO_TRIAL_EVENT"):
            monkeypatch.setenv(var, "0")
            same_bits(base, run(d, icp, prior, rp, niter))
            monkeypatch.delenv(var)
        monkeypatch.setenv("CUGO_SPECULATE", "0")
        nospec = run(d, icp, prior, rp, niter)
        monkeypatch.delenv("CUGO_SPECULATE")
        monkeypatch.setenv("CUGO_PROFILE", "1")
        same_bits(nospec, run(d, icp, prior, rp, niter))
        monkeypatch.delenv("CUGO_PROFILE")


@pytest.mark.parametrize("form", ["CUGO_HSC_ROWS", "CUGO_HSC_STRIP", "CUGO_SCHUR_PLAN", "CUGO_HSC_MFMA=0"])
def test_opt_in_schur_forms_with_relpose_sets(form, monkeypatch):
    """mixed holds a pair block without landmark products.  The block-row form, the landmark-major plan and the
    vector-lane gather write such a block as zero and take the edge term on top: the reference's trajectory.  The
    row-strip form reads the list entry in front of a block's range, which such a block does not have: initialize()
    refuses the combination"""
    var, _, val = form.partition("=")
    monkeypatch.setenv(var, val or "1")
    d, icp, prior, rp, niter, tr, pose, lm, tol, etol = L.reference("mixed")
    if var == "CUGO_HSC_STRIP":
        with pytest.raises(cugo.CugoError, match="CUGO_HSC_STRIP"):
            run(d, icp, prior, rp, niter)
        return
    out = run(d, icp, prior, rp, niter)
    print_trajectory(form, out["stats"], tr)
    assert out["sstats"]["hsc_blocks"] == L.union_pattern_blocks(d, rp)
    assert_trajectories_match(out["stats"], tr, tol)
    np.testing.assert_allclose(out["pose"], pose, rtol=0, atol=etol)


def test_a_new_pair_after_an_optimize_gives_the_bits_of_a_fresh_graph():
    """optimise the chain, add a loop closure on a NEW pair, initialize() and optimize() again: pattern, ordering,
    symbolic factor and plan are rebuilt on the device that already held the old ones; bit for bit a fresh graph that
    starts from the same estimates with that edge"""
    d, icp, prior, rp = L.chain_case()
    rng = np.random.default_rng(77)
    extra = L.edges_between(rng, d["pose_gt"], [(4, 2)], 0.01, 0.05, 10.0)
    assert (1, 3) not in L.relpose_pairs(d, rp)  # (free-first: poses 2 and 4)
    g = L.build_graph(d, icp, prior, rp)
    g.initialize()
    g.optimize(3)
    mid = g.poses()
    blocks = g.structure_stats()["hsc_blocks"]
    g.add_relpose_edges(extra["a"], extra["b"], extra["z"], extra["info"])
    g.initialize()
    g.optimize(4)
    got = dict(stats=g.stats(), pose=g.poses(), lm=g.landmarks())
    assert g.structure_stats()["hsc_blocks"] == blocks + 1 and g.n_relpose_edges() == len(rp["a"]) + 1
    g.close()
    both = RR.make_edges(np.concatenate([rp["a"], extra["a"]]), np.concatenate([rp["b"], extra["b"]]),
                         np.concatenate([rp["z"], extra["z"]]), np.concatenate([rp["info"], extra["info"]]))
    fresh = run(dict(d, pose=mid), icp, prior, both, 4)
    same_bits(got, fresh)


@pytest.mark.parametrize("name", ["chain", "gauge"])
def test_pose_covariances_are_the_blocks_of_the_dense_inverse(name):
    """after convergence: pose_covariances() against the 6 x 6 diagonal blocks of the inverse of the reference's dense
    H at the optimiser's estimates.  The selected inverse runs on the Hsc pattern, which holds the pairs.  Bound as in
    test_prior_graph.test_covariance_round_trip_through_a_prior: 1e-9 of max|Sigma|"""
    d, icp, prior, rp = L.CASES[name][0]()
    out = run(d, icp, prior, rp, 12, covariances=True)
    g = L.RelPoseGraph(dict(d, pose=out["pose"]), icp, prior, rp)
    H, _ = g.normal_equations()
    S = np.linalg.inv(H)
    worst = 0.0
    for i in range(len(d["pose"])):
        if d["pose_fixed"][i]:
            assert not out["cov"][i].any()
            continue
        p = g.pidx[i]
        want = S[6 * p:6 * p + 6, 6 * p:6 * p + 6]
        worst = max(worst, np.abs(out["cov"][i] - want).max())
    print("%s: |Sigma - inv(H) blocks| = %.3g of %.3g, cond %.3g" % (name, worst, np.abs(S).max(), np.linalg.cond(H)))
    assert worst <= 1e-9 * np.abs(S).max()


def test_float32_internal_mode_with_relpose_sets():
    """the relative-pose terms stay fp64 (they touch no stored block): the bar the fp32 prior test states for the mode"""
    d, icp, prior, rp, niter, tr, pose, lm, tol, etol = L.reference("mixed")
    out = run(d, icp, prior, rp, niter, float32=True)
    assert_trajectories_match(out["stats"], tr, 1e-5, check_trials=False)
    assert [s["trials"] for s in out["stats"]] == [t["trials"] for t in tr]


@pytest.mark.parametrize("mode", ["1", "2"])
def test_poisoned_allocations_change_nothing(mode):
    """CUGO_POISON_ALLOC (hip_util.h) in a child process, on this file's trajectory, covariance and kernel-level cases:
    nothing reads memory nobody wrote (workgroup totals, pair blocks without products, the plan's arrays)"""
    env = dict(os.environ, CUGO_POISON_ALLOC=mode)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p",
                        "no:cacheprovider", "-k", "against_the_reference or dense_inverse or two_stream_launches"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "guard zone" not in r.stderr and " passed" in r.stdout


# ---- the two launches of the two-stream form, at kernel level ---------------------------------------------------------
def test_two_stream_launches_leave_what_the_schur_form_leaves():
    """the 5 free + 2 fixed designed graph of tests/test_relpose_host.py on a pattern with extra blocks (rowptr[p] != p)
    and a pre-filled Hsc.  Two-stream sequence: the build form without an off-diagonal destination adds the diagonal
    terms and b to Hpp / bp; a stand-in for the Schur pass copies Hpp into the diagonal blocks of Hsc and bp into bsc
    (on the host, exact); the off-diagonal add follows.  Hsc, bp and bsc are then those of the Schur form within 1e-12
    of max|H|, a second call gives the same bits, and a repeated Schur pass from the same build pass gives Hsc again"""
    import devmem
    from test_relpose import blocks, designed, full_pattern
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    ctx = devmem.Ctx()
    rng, poses, rp = designed(seed=31, rk=(3, 4.0))
    P = 5
    rowptr, colind = full_pattern(P)
    nnzb = len(colind)
    assert all(rowptr[p] != p for p in range(1, P))
    ev, pl = RR.upload(ctx, len(poses), P, rp, rowptr, colind)
    d_poses, d_rowptr = ctx.to_dev(poses), ctx.to_dev(rowptr)
    Hsc0 = rng.normal(size=(nnzb, 36))
    Hsc0[rowptr[:-1]] = 0.0  # (a Schur pass writes Hpp - products there; the stand-in below has no products)
    Hpp0, bp0 = rng.normal(size=(P, 36)), rng.normal(size=(P, 6))

    def two_stream():
        d_H, d_b, d_chi = ctx.to_dev(Hpp0), ctx.to_dev(bp0), ctx.empty(2)
        cugo.relpose_construct_quadratic_form_diag(ctx.h, ev, d_poses, d_H, d_b, d_chi)
        Hpp, bp = ctx.to_host(d_H, (P, 36)), ctx.to_host(d_b, (P, 6))
        out = []
        for _ in range(2):  # (the Schur pass of a retried trial: from the same build pass)
            Hsc = Hsc0.copy()
            Hsc[rowptr[:-1]] = Hpp
            d_Hsc = ctx.to_dev(Hsc)
            cugo.relpose_add_offdiag_schur(ctx.h, ev, d_poses, d_Hsc)
            out.append(ctx.to_host(d_Hsc, (nnzb, 36)))
        assert np.array_equal(out[0], out[1])
        return out[0], bp, bp.copy(), ctx.to_host(d_chi, 1)[0]

    def one_stream():
        Hsc = Hsc0.copy()
        Hsc[rowptr[:-1]] = Hpp0
        d_Hsc, d_bp, d_bsc, d_chi = ctx.to_dev(Hsc), ctx.to_dev(bp0), ctx.to_dev(bp0), ctx.empty(2)
        cugo.relpose_construct_quadratic_form_schur(ctx.h, ev, d_poses, d_rowptr, d_Hsc, d_bp, d_bsc, d_chi)
        return ctx.to_host(d_Hsc, (nnzb, 36)), ctx.to_host(d_bp, (P, 6)), ctx.to_host(d_bsc, (P, 6)), ctx.to_host(d_chi, 1)[0]

    a, b = two_stream(), one_stream()
    Hr, br, Hoffr, chir, _ = RR.reference_build(poses, P, rp, rowptr, colind)
    scale = max(np.abs(Hr).max(), np.abs(Hoffr).max())
    for x, y, what in zip(a[:3], b[:3], ("Hsc", "bp", "bsc")):
        err = np.abs(x - y).max()
        print("%s: two-stream against one-stream %.3g of max|H| %.3g" % (what, err, scale))
        assert err <= 1e-12 * scale
    assert a[3] == b[3] and abs(a[3] - chir) <= 1e-12 * chir
    # ... and both are the reference's terms on top of what was there
    want = blocks(Hsc0, nnzb) + Hoffr
    want[rowptr[:-1]] = blocks(Hpp0, P) + Hr
    assert np.abs(blocks(a[0], nnzb) - want).max() <= 1e-12 * scale
    untouched = np.array([not Hoffr[k].any() for k in range(nnzb)])
    untouched[rowptr[:-1]] = False
    assert untouched.any() and not untouched.all() and np.array_equal(a[0][untouched], Hsc0[untouched])
    a2 = two_stream()
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], a2[:3])) and a[3] == a2[3]
    pl.close()
    ctx.close()
