"""GPU tests of the pose-landmark covariances at the graph level (Graph.pose_landmark_cross_covariances,
Graph.reprojection_covariances) against the dense inverse of the oracle's normal equations at the optimiser's
estimates (test_covariance.dense_inverse and its kin for the graphs with pose edge sets and landmark priors).

Sigma_al of EVERY (pose, landmark) pair is held to 1e-8 sqrt(|Sigma_aa|_F |Sigma_ll|_F): the project's graph-level
figure (test_cross_cov.py) on the natural scale of a cross block — on these graphs |Sigma_al| falls to 3e-4 of that
scale.  S = J Sigma J^T of every pair whose depth at the estimates exceeds 0.1 — and of every pair whose landmark lies
more than 0.1 behind the camera, see test_reprojection_covariances_vs_dense_inverse — is held to
1e-8 (|J_p Sigma_aa J_p^T|_F + |J_l Sigma_ll J_l^T|_F), mono and stereo, with the Jacobian formulas of pl_cov_ref.
The worst measured ratios per case are printed (and recorded in DESIGN.md section 11b).

Measured on an MI355X, in units of the two bounds: Sigma_al 9.3e-5 (small_10x200), 1.5e-3 (loop_12x150), 8.4e-4
(huber_8x80), 1.4e-3 (stereo synth), 3.5e-5 (ICP sets), 9.2e-5 (landmark priors); S at most 9.1e-3 (stereo synth, dim 2).
"""
import importlib

import numpy as np
import pytest

import pl_cov_ref as pr
from test_covariance import dense_inverse, golden, oracle_problem, stereo_synth

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
pytestmark = pytest.mark.gpu
CASES = ("small_10x200", "loop_12x150", "huber_8x80", "synth_stereo", "icp_sets", "lm_priors")


def build(case):
    """(graph after optimize(5), problem dict, dense H^-1 at its estimates, offsets of the pose blocks, of the landmark
    blocks (-1: fixed))"""
    if case == "icp_sets":
        import icp_lm_ref as R
        from test_icp_graph import dense_inverse_with_icp
        d, icp = R.mixed_case()
        g = R.build_graph(d, icp)
        g.initialize()
        g.optimize(5)
        inv, ip, il = dense_inverse_with_icp(d, icp, g.poses(), g.landmarks())
    elif case == "lm_priors":
        # (the reference adds Omega to the landmark's block of the dense H; no robust kernel on the set)
        import lm_prior_ref as LR
        from test_lm_prior_graph import dense_inverse as dense_inverse_lmp
        d, lmp, icp, prior = LR.tenth_case()
        lmp = dict(lmp, rk=(0, 1.0))
        g = LR.build_graph(d, lmp, icp, prior)
        g.initialize()
        g.optimize(5)
        inv, ip, il = dense_inverse_lmp(d, lmp, icp, prior, g.poses(), g.landmarks())
    else:
        d, rk = stereo_synth((0, 1.0)) if case == "synth_stereo" else golden(case)
        g = cugo.graph_from_arrays(d, rk=rk)
        g.initialize()
        g.optimize(5)
        inv, ip, il = dense_inverse(oracle_problem(d, rk, g.poses(), g.landmarks()))
    return g, d, inv, np.asarray(ip), np.asarray(il)


@pytest.fixture(scope="module")
def built():
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = build(case)
        return cache[case]
    yield get
    for v in cache.values():
        v[0].close()


def all_pairs(P, L):
    a, l = np.meshgrid(np.arange(P, dtype=np.int32), np.arange(L, dtype=np.int32), indexing="ij")
    return a.reshape(-1), l.reshape(-1)


def ref_blocks(inv, ip, il, a, l):
    """Sigma_aa [n,6,6], Sigma_al [n,6,3], Sigma_ll [n,3,3] of the pairs from the dense inverse, zero where a vertex is
    fixed"""
    n = len(a)
    Saa, Sal, Sll = np.zeros((n, 6, 6)), np.zeros((n, 6, 3)), np.zeros((n, 3, 3))
    for k in range(n):
        o, q = ip[a[k]], il[l[k]]
        if o >= 0:
            Saa[k] = inv[o:o + 6, o:o + 6]
        if q >= 0:
            Sll[k] = inv[q:q + 3, q:q + 3]
        if o >= 0 and q >= 0:
            Sal[k] = inv[o:o + 6, q:q + 3]
    return Saa, Sal, Sll


@pytest.mark.parametrize("case", CASES)
def test_every_pose_landmark_pair_vs_dense_inverse(built, case):
    g, d, inv, ip, il = built(case)
    a, l = all_pairs(len(ip), len(il))
    got = g.pose_landmark_cross_covariances(a, l)
    again = g.pose_landmark_cross_covariances(a, l)
    assert np.array_equal(got.view(np.int64), again.view(np.int64))
    Saa, Sal, Sll = ref_blocks(inv, ip, il, a, l)
    fixed = (ip[a] < 0) | (il[l] < 0)
    assert fixed.any() and not got[fixed].any()
    scale = np.sqrt(np.linalg.norm(Saa, axis=(1, 2)) * np.linalg.norm(Sll, axis=(1, 2)))
    err = np.abs(got - Sal).reshape(len(a), -1).max(1)
    r = err[~fixed] / (1e-8 * scale[~fixed])
    rel = np.linalg.norm(Sal, axis=(1, 2))[~fixed] / scale[~fixed]
    print("%s: %d pairs (%d with a fixed vertex), worst |Sigma_al - ref| = %.3g of the 1e-8 bound; |Sigma_al| from %.3g to "
          "%.3g of sqrt(|Sigma_aa| |Sigma_ll|)" % (case, len(a), fixed.sum(), r.max(), rel.min(), rel.max()))
    assert r.max() <= 1, (case, int(np.flatnonzero(~fixed)[r.argmax()]), float(r.max()))


@pytest.mark.parametrize("case", ("small_10x200", "synth_stereo"))
def test_joint_covariance_of_a_camera_and_a_point(built, case):
    """[[Sigma_aa, Sigma_al], [Sigma_al^T, Sigma_ll]] of 50 pairs assembled from this call, pose_covariances() and
    landmark_covariances(): symmetric, smallest eigenvalue >= -1e-8 |joint|"""
    g, d, inv, ip, il = built(case)
    rng = np.random.default_rng(2)
    fa, fl = np.flatnonzero(ip >= 0), np.flatnonzero(il >= 0)
    a, l = rng.choice(fa, 50).astype(np.int32), rng.choice(fl, 50).astype(np.int32)
    g.compute_covariances()
    Saa, Sll = g.pose_covariances(a), g.landmark_covariances(l)
    Sal = g.pose_landmark_cross_covariances(a, l)
    assert np.array_equal(g.pose_covariances(a), Saa) and np.array_equal(g.landmark_covariances(l), Sll)
    worst = 0.0
    for k in range(50):
        J = np.block([[Saa[k], Sal[k]], [Sal[k].T, Sll[k]]])
        assert np.array_equal(J, J.T) and Sal[k].any()
        worst = min(worst, np.linalg.eigvalsh(J)[0] / np.linalg.norm(J))
        ref = inv[np.ix_(np.r_[ip[a[k]]:ip[a[k]] + 6, il[l[k]]:il[l[k]] + 3], np.r_[ip[a[k]]:ip[a[k]] + 6, il[l[k]]:il[l[k]] + 3])]
        assert np.abs(J - ref).max() <= 1e-8 * np.linalg.norm(ref)
    print("%s: smallest eigenvalue of a joint block / its norm: %.3g" % (case, worst))
    assert worst >= -1e-8


@pytest.mark.parametrize("case", CASES)
def test_reprojection_covariances_vs_dense_inverse(built, case):
    g, d, inv, ip, il = built(case)
    pose, lm = g.poses(), g.landmarks()
    a, l = all_pairs(len(ip), len(il))
    cam = np.asarray(d["e_cam"], np.float64).reshape(-1, 5)[0]
    cams = np.tile(cam, (len(a), 1))
    Z = pr.jacobians(pose[a], lm[l], cams, np.zeros(len(a), bool), np.float64)[4]
    # Every pair whose depth exceeds 0.1 is checked, and so is every pair whose landmark lies more than 0.1 BEHIND the
    # camera: the projection and its Jacobians are as regular there, and on the stereo synth, whose 40 poses look along
    # a trajectory, 8 % of all (pose, landmark) pairs are of that kind.  Left out are the pairs within 0.1 of the
    # camera plane alone, at most 2 % of a case.
    keep = np.abs(Z) > 0.1
    print("%s: %d of %d pairs left out for depth (%.2f %%); %.2f %% have a depth <= 0.1"
          % (case, (~keep).sum(), len(a), 100.0 * (~keep).mean(), 100.0 * (Z <= 0.1).mean()))
    assert (~keep).mean() <= 0.02
    a, l, cams = a[keep], l[keep], cams[keep]
    n = len(a)
    Saa, Sal, Sll = ref_blocks(inv, ip, il, a, l)
    fp, fl = ip[a] >= 0, il[l] >= 0
    assert (~fp).any() and (fp & fl).any()
    seen = set(zip(np.asarray(d["e_pose"]).tolist(), np.asarray(d["e_lm"]).tolist()))
    observed = np.array([(int(x), int(y)) in seen for x, y in zip(a, l)]) & fp & fl
    st = np.asarray(d["e_stereo"]).astype(bool)
    seen3 = set(zip(np.asarray(d["e_pose"])[st].tolist(), np.asarray(d["e_lm"])[st].tolist()))
    observed3 = np.array([(int(x), int(y)) in seen3 for x, y in zip(a, l)]) & fp & fl
    for dim in (2, 3):
        got = g.reprojection_covariances(a, l, dim=dim, cam=cam)
        assert got.shape == (n, dim, dim) and np.array_equal(got, got.transpose(0, 2, 1))
        if dim == 2:   # one camera for all, one per query, the set camera: the same bits
            assert np.array_equal(got, g.reprojection_covariances(a, l, dim=2, cam=cams))
            g.set_camera(2, cam)
            assert np.array_equal(got, g.reprojection_covariances(a, l, dim=2))
        JP, _, JL, _, _ = pr.jacobians(pose[a], lm[l], cams, np.full(n, dim == 3), np.float64)
        JP, JL = JP * fp[:, None, None], JL * fl[:, None, None]
        Mp = np.einsum("nik,nkm,njm->nij", JP, Saa, JP)
        Ml = np.einsum("nik,nkm,njm->nij", JL, Sll, JL)
        X = np.einsum("nik,nkm,njm->nij", JP, Sal, JL)
        ref = (Mp + X + X.transpose(0, 2, 1) + Ml)[:, :dim, :dim]
        tol = 1e-8 * (np.linalg.norm(Mp, axis=(1, 2)) + np.linalg.norm(Ml, axis=(1, 2)))
        both = ~fp & ~fl
        assert not got[both].any()
        r = np.abs(got - ref).reshape(n, -1).max(1)[~both] / tol[~both]
        # the point of the feature: for a pose that observes the landmark S is smaller than the two marginal parts
        part = np.linalg.norm(got, axis=(1, 2)) / np.maximum(np.linalg.norm(Mp[:, :dim, :dim], axis=(1, 2)) +
                                                              np.linalg.norm(Ml[:, :dim, :dim], axis=(1, 2)), 1e-300)
        # (of what the pose observes: u and v through any edge, the right image's u through a stereo edge — on the
        # graph with ICP sets three mono observations predict a third row that is not smaller)
        smaller = part[observed if dim == 2 else observed3] < 1
        shrink = part[fp & fl]
        print("%s dim %d: %d pairs, worst |S - J Sigma J^T| = %.3g of the 1e-8 bound; S smaller than its marginal parts for "
              "%d of %d observing pairs; |S| / (|J_p S_aa J_p^T| + |J_l S_ll J_l^T|) falls to %.3g"
              % (case, dim, n, r.max(), smaller.sum(), len(smaller), shrink.min()))
        assert r.max() <= 1, (case, dim, float(r.max()))
        assert len(smaller) and smaller.all(), (case, dim)


def test_queries_leave_the_optimiser_and_the_marginals_alone():
    """optimize(5); queries; optimize(5) gives the bits of optimize(5); optimize(5), and the marginals stored before the
    queries are handed out unchanged after them: the contract of pose_cross_covariances (test_cross_cov.py).  One call
    of optimize(10) is no reference for this: every optimize() call starts its damping anew (lambda = tau max diag H,
    nu = 2), so two calls of five iterations differ from one of ten with or without the queries between them"""
    d = cugo.synth(60, 900, 3700, seed=1)
    a = cugo.graph_from_arrays(d)
    a.initialize()
    a.optimize(5)
    a.compute_covariances()
    cp, cl = a.pose_covariances(), a.landmark_covariances()
    rng = np.random.default_rng(1)
    qa, ql = rng.integers(0, 60, 200), rng.integers(0, 900, 200)
    assert a.pose_landmark_cross_covariances(qa, ql).any()
    assert a.reprojection_covariances(qa, ql, dim=3, cam=d["cam"]).any()
    assert np.array_equal(a.pose_covariances(), cp) and np.array_equal(a.landmark_covariances(), cl)
    a.optimize(5)
    b = cugo.graph_from_arrays(d)
    b.initialize()
    b.optimize(5)
    b.optimize(5)
    assert a.stats() == b.stats()
    assert np.array_equal(a.poses(), b.poses()) and np.array_equal(a.landmarks(), b.landmarks())
    a.close()
    b.close()


def test_refusals_and_a_landmark_without_an_edge():
    d = cugo.synth(20, 300, 1300, seed=6)
    g = cugo.graph_from_arrays(d)
    with pytest.raises(cugo.CugoError, match="error -3"):
        g.pose_landmark_cross_covariances([1], [2])
    with pytest.raises(cugo.CugoError, match="error -3"):
        g.reprojection_covariances([1], [2], dim=2, cam=d["cam"])
    g.initialize()
    for bad in (([1], [300]), ([20], [2]), ([-1], [2])):
        with pytest.raises(cugo.CugoError, match="error -3"):
            g.pose_landmark_cross_covariances(*bad)
        with pytest.raises(cugo.CugoError, match="error -3"):
            g.reprojection_covariances(*bad, dim=2, cam=d["cam"])
    with pytest.raises(cugo.CugoError, match="error -3"):
        g.reprojection_covariances([1], [2], dim=4, cam=d["cam"])
    assert g.pose_landmark_cross_covariances([1], [2]).any()
    assert g.pose_landmark_cross_covariances([], []).shape == (0, 6, 3)
    assert not g.pose_landmark_cross_covariances([0], [2]).any()           # pose 0 is fixed
    g.close()
    f = cugo.graph_from_arrays(d)
    f.set_float32(1)
    f.initialize()
    with pytest.raises(cugo.CugoError, match="error -3"):
        f.pose_landmark_cross_covariances([1], [2])
    with pytest.raises(cugo.CugoError, match="error -3"):
        f.reprojection_covariances([1], [2], dim=2, cam=d["cam"])
    f.close()
    # a free landmark without any edge: CUGO_ERR_NUMERIC when a query names it, and only then
    e = dict(d)
    e["lm"] = np.concatenate([d["lm"], d["lm"][:1] + 0.5])
    e["lm_fixed"] = np.concatenate([d["lm_fixed"], [0]]).astype(np.uint8)
    h = cugo.graph_from_arrays(e)
    h.initialize()
    h.optimize(3)
    with pytest.raises(cugo.CugoError, match="error -4"):
        h.pose_landmark_cross_covariances([1, 2], [2, 300])
    with pytest.raises(cugo.CugoError, match="error -4"):
        h.reprojection_covariances([1, 0], [2, 300], dim=2, cam=d["cam"])
    assert h.pose_landmark_cross_covariances([1, 2], [2, 299]).any()
    assert h.reprojection_covariances([1, 0], [2, 299], dim=2, cam=d["cam"]).any()
    h.close()
