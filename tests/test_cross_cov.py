"""GPU tests of the pose cross-covariances for any pair: cugo_chol_inverse_blocks (k_inv_path_walk, k_inv_pair_blocks of
cov_kernels.hip) against numpy's inverse on general patterns under every layout the factorisation can leave W and L21
in, against the refined inverse and the per-case bound of tests/cross_cov_ref.py on the designed fronts, on a path as
long as the matrix, and its invariants; then the graph level (Graph.pose_cross_covariances,
Graph.relative_pose_covariances) against H^-1 built from the CPU oracle's normal equations."""
import ctypes as C
import importlib

import numpy as np
import pytest

import chol_designed as cd
import cross_cov_ref as xr
from test_covariance import dense_inverse, golden, oracle_problem
from test_host import covis_pattern, patterns, random_spd_bsr

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_NUMERIC = -3, -4
I32P = C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def ctx():
    import devmem
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    c = devmem.Ctx()
    yield c
    c.close()


class Solver:
    """one analysed pattern on the device with its buffers"""

    def __init__(self, ctx, rowptr, colind):
        self.ctx, self.lib = ctx, cugo.lib()
        self.n, self.B = len(rowptr) - 1, len(colind)
        self.s = cd.analyze(self.lib, rowptr, colind, ctx.h)
        self.dx, self.fail = ctx.empty(6 * self.n), ctx.empty(2, np.int32)

    def factor(self, dH, lam, db):
        cugo.check(self.lib.cugo_chol_factor_solve(self.s, dH, C.c_double(lam), db, self.dx, self.fail))

    def inverse_blocks(self, rows, cols):
        """(return code, blocks [n_pairs, 6, 6] with rows a and columns b)"""
        rows, cols = np.ascontiguousarray(rows, np.int32), np.ascontiguousarray(cols, np.int32)
        d = self.ctx.empty(36 * len(rows))
        rc = self.lib.cugo_chol_inverse_blocks(self.s, len(rows), rows.ctypes.data_as(I32P), cols.ctypes.data_as(I32P), d)
        return rc, self.ctx.to_host(d, 36 * len(rows)).reshape(-1, 6, 6).transpose(0, 2, 1).copy()

    def selected_inverse(self):
        d = self.ctx.empty(36 * self.B)
        cugo.check(self.lib.cugo_chol_selected_inverse(self.s, d))
        return self.ctx.to_host(d, 36 * self.B).reshape(self.B, 36).copy()

    def close(self):
        self.lib.cugo_chol_destroy(self.s)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def expected_blocks(inv, rows, cols):
    return np.array([inv[6 * a:6 * a + 6, 6 * b:6 * b + 6] for a, b in zip(rows, cols)])


def general_patterns():
    out = {name: cd.csr(rows) for name, rows in patterns().items()}
    d = cugo.synth(160, 2500, 10500, seed=3, n_loop_closures=80)
    ep = d["e_pose"].astype(np.int64) - 1
    ep[ep < 0] = 10**6
    out["synthetic"] = covis_pattern(159, ep, d["e_lm"])
    return out


# ------------------------------------------------------------------ kernel level, general patterns ---------
SMALL_FRONTS = {"CUGO_ND_LEAF": "4", "CUGO_MAX_SUPER_COLS": "3", "CUGO_TARGET_TASKS": "4", "CUGO_MIN_SUBTREE_TASKS": "0"}
# the environment sets of test_covariance.test_selected_inverse_vs_numpy that change where W and L21 live
LAYOUT_ENVS = [{}, {"CUGO_MIN_SUBTREE_TASKS": "0"}, {"CUGO_ALIAS_CHAINS": "0"}, SMALL_FRONTS,
               {"CUGO_ND_LEAF": "1000", "CUGO_MAX_SUPER_COLS": "1", "CUGO_TARGET_TASKS": "100000"},
               {"CUGO_MAX_SUPER_COLS": "24", "CUGO_ZERO_FRAC": "0.9", "CUGO_MIN_SUBTREE_TASKS": "0"},
               {"CUGO_LOOKAHEAD": "1"}, {"CUGO_TWO_PHASE_MIN_TILES": "1", "CUGO_TILE32_MAX_TILES": "0"},
               {"CUGO_PANEL16": "0"}]


@pytest.mark.parametrize("env", LAYOUT_ENVS, ids=cd.option_id)
def test_inverse_blocks_vs_numpy(ctx, env, monkeypatch):
    """any block of (A + lambda I)^-1: all pairs of the small patterns (and 20 in the other order); on the 159-row
    pattern 200 random pairs and those the plan singles out (two rows of one front, root with leaf, paths that meet at
    the root only, a subtree-stage front, a front stored in its child's update block)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(5)
    for name, (rowptr, colind) in general_patterns().items():
        n = len(rowptr) - 1
        A, vals = random_spd_bsr(rowptr, colind, rng)
        sv = Solver(ctx, rowptr, colind)
        pl = xr.plan_of(sv.lib, sv.s)
        if n <= 72:
            rows, cols = xr.all_pairs(n, rng)
            if name == "random":  # (all pairs: among them rows whose paths meet at the root only)
                assert "meet_at_root" in xr.special_rows(pl), name
        else:
            # (the root of this pattern's plan has one child under every environment here: no two paths meet at the
            # root only, special_rows() leaves that kind out; `random` above and the `widths` design hold it)
            rows, cols = xr.plan_pairs(pl, rng)
            kinds = set(xr.special_rows(pl))
            assert {"one_front", "root_leaf"} <= kinds, (name, kinds)
            if env is SMALL_FRONTS:  # the subtree stage: several fronts per task, L21 left inside the fronts
                assert {"subtree_stage", "aliased"} <= kinds and (pl["l21off"] < 0).any(), (name, kinds)
            if not env:
                assert "aliased" in kinds and (pl["l21off"] >= 0).all(), (name, kinds)
        dH, db = ctx.to_dev(vals), ctx.to_dev(rng.normal(size=6 * n))
        for lam in (0.0, 2.5):
            sv.factor(dH, lam, db)
            rc, got = sv.inverse_blocks(rows, cols)
            assert rc == 0, (name, lam, sv.lib.cugo_last_error())
            inv = np.linalg.inv(A + lam * np.eye(6 * n))
            np.testing.assert_allclose(got, expected_blocks(inv, rows, cols), rtol=1e-9, atol=1e-9 * np.abs(inv).max(),
                                       err_msg="%s lambda %.1f" % (name, lam))
        sv.close()


# ------------------------------------------------------------------ kernel level, designed fronts ---------
@pytest.mark.parametrize("cls", cd.CLASSES)
@pytest.mark.parametrize("name", cd.NAMES)
def test_inverse_blocks_on_designed_fronts(ctx, name, cls):
    """pivot widths 1 .. 16, boundaries at the 16-, 32- and 64-row edges, the 67-child front: every queried entry within
    k_xcov_case x u (|A^-1| |L| |L^T| |A^-1|)_ab of the refined inverse (4 x what the numpy replay of the two passes
    reaches, tests/test_cross_cov_host.py)"""
    rowptr, colind, _ = cd.design(name)
    n = len(rowptr) - 1
    sv = Solver(ctx, rowptr, colind)
    rows, cols = xr.design_pairs(name, xr.plan_of(sv.lib, sv.s))
    A, vals, b = cd.values(name, cls)
    dH, db = ctx.to_dev(vals), ctx.to_dev(b)
    for lam in cd.LAMBDAS:
        sv.factor(dH, lam, db)
        rc, got = sv.inverse_blocks(rows, cols)
        assert rc == 0, (name, cls, lam)
        _, X1, scale = cd.inverse_reference(name, cls, lam)
        X, mask = xr.pairs_to_dense(got.transpose(0, 2, 1).reshape(-1, 36), rows, cols, n)
        r, bound = cd.sinv_ratio(X, X1, scale, mask), xr.k_xcov_case(name, cls, lam)
        print("%s %s lambda %.1f: inverse blocks ratio %.3g (replay %.3g, bound %.3g)"
              % (name, cls, lam, r, xr.XCOV_REPLAY[(name, cls, lam)], bound))
        assert r <= bound, (name, cls, lam, r)
    sv.close()


# ------------------------------------------------------------------ kernel level, long path ---------
def test_a_path_as_long_as_the_matrix(ctx, monkeypatch):
    """the band pattern with one-column fronts: the first row's path runs through every front of the plan"""
    monkeypatch.setenv("CUGO_ND_LEAF", "1000")
    monkeypatch.setenv("CUGO_MAX_SUPER_COLS", "1")
    rowptr, colind = cd.csr(patterns()["band"])
    n = len(rowptr) - 1
    rng = np.random.default_rng(7)
    A, vals = random_spd_bsr(rowptr, colind, rng)
    sv = Solver(ctx, rowptr, colind)
    pl = xr.plan_of(sv.lib, sv.s)
    lengths = [len(xr.path(pl, pl["iperm"][v])) for v in (0, n - 1)]
    assert max(lengths) == len(pl["ncb"]) >= 60, (lengths, len(pl["ncb"]))
    rows, cols = np.array([0, n - 1, 0, n - 1], np.int32), np.array([n - 1, 0, 0, n - 1], np.int32)
    for lam in (0.0, 2.5):
        sv.factor(ctx.to_dev(vals), lam, ctx.to_dev(rng.normal(size=6 * n)))
        rc, got = sv.inverse_blocks(rows, cols)
        assert rc == 0
        inv = np.linalg.inv(A + lam * np.eye(6 * n))
        np.testing.assert_allclose(got, expected_blocks(inv, rows, cols), rtol=1e-9, atol=1e-9 * np.abs(inv).max())
    sv.close()


# ------------------------------------------------------------------ kernel level, invariants ---------
def test_inverse_blocks_invariants(ctx, monkeypatch):
    """the same bits on a second call and with three rows per batch; on the pairs of the analysed pattern the blocks
    agree with cugo_chol_selected_inverse to twice the bound of the case and (b, a) is the transpose of (a, b) bit for
    bit; an index outside [0, n) is refused; CUGO_ERR_NUMERIC after a factorisation that raised the zero-pivot flag"""
    name, cls, lam = "widths", "dd", 0.0
    rowptr, colind, _ = cd.design(name)
    n = len(rowptr) - 1
    A, vals, b = cd.values(name, cls)
    dH, db = ctx.to_dev(vals), ctx.to_dev(b)
    sv = Solver(ctx, rowptr, colind)
    assert sv.inverse_blocks([0], [0])[0] == ERR_INVALID  # no factorisation yet
    sv.factor(dH, lam, db)
    rng = np.random.default_rng(3)
    rows, cols = xr.plan_pairs(xr.plan_of(sv.lib, sv.s), rng, 300)
    rc, got = sv.inverse_blocks(rows, cols)
    rc2, again = sv.inverse_blocks(rows, cols)
    assert rc == 0 and rc2 == 0 and same_bits(got, again)
    # three distinct rows per batch: over a hundred batches for these pairs.  The C ABI does not hand out the number
    # of batches, so that several ran is not observed here: what is held is that the bits do not depend on the cut
    monkeypatch.setenv("CUGO_XCOV_BATCH", "3")
    sb = Solver(ctx, rowptr, colind)
    monkeypatch.delenv("CUGO_XCOV_BATCH")
    sb.factor(dH, lam, db)
    rc, batched = sb.inverse_blocks(rows, cols)
    assert rc == 0 and same_bits(got, batched)
    sb.close()
    # the pattern's own pairs, both orders
    pr = np.repeat(np.arange(n), np.diff(rowptr)).astype(np.int32)
    rc, up = sv.inverse_blocks(pr, colind)
    rc2, lo = sv.inverse_blocks(colind, pr)
    assert rc == 0 and rc2 == 0 and same_bits(lo, up.transpose(0, 2, 1).copy())
    S = sv.selected_inverse().reshape(-1, 6, 6).transpose(0, 2, 1)
    _, X1, scale = cd.inverse_reference(name, cls, lam)
    sc = expected_blocks(scale, pr, colind)
    worst = float((np.abs(up - S) / sc).max())
    twice = 2 * xr.k_xcov_case(name, cls, lam)
    print("inverse blocks against the selected inverse on the pattern: %.3g (twice the bound: %.3g)" % (worst, twice))
    assert worst <= twice
    assert sv.inverse_blocks([0], [n])[0] == ERR_INVALID and sv.inverse_blocks([-1], [0])[0] == ERR_INVALID
    bad = vals.copy()
    bad[rowptr[n // 2]] = -np.eye(6).reshape(-1)
    sv.factor(ctx.to_dev(bad), lam, db)
    assert sv.inverse_blocks(rows, cols)[0] == ERR_NUMERIC
    sv.factor(dH, lam, db)
    rc, back = sv.inverse_blocks(rows, cols)
    assert rc == 0 and same_bits(got, back)
    sv.close()


# ------------------------------------------------------------------ graph level ----------
def optimised(case, niter=5):
    d, rk = golden(case)
    g = cugo.graph_from_arrays(d, rk=rk)
    g.initialize()
    g.optimize(niter)
    inv, ip, _ = dense_inverse(oracle_problem(d, rk, g.poses(), g.landmarks()))
    return d, g, inv, ip


def all_pose_pairs(P):
    a, b = np.meshgrid(np.arange(P, dtype=np.int32), np.arange(P, dtype=np.int32), indexing="ij")
    return a.reshape(-1), b.reshape(-1)


@pytest.mark.parametrize("case", ["small_10x200", "loop_12x150", "huber_8x80"])
def test_graph_cross_covariances_vs_dense_inverse(ctx, case):
    """every pose pair, both orders, against the pose-pose blocks of the oracle's H^-1; zeros with the fixed pose; the
    pairs (a, a) are the stored marginals"""
    d, g, inv, ip = optimised(case)
    P = len(ip)
    a, b = all_pose_pairs(P)
    got = g.pose_cross_covariances(a, b)
    assert (ip < 0).any()
    for k in range(len(a)):
        if ip[a[k]] < 0 or ip[b[k]] < 0:
            assert not got[k].any(), (a[k], b[k])
        else:
            ref = inv[ip[a[k]]:ip[a[k]] + 6, ip[b[k]]:ip[b[k]] + 6]
            assert np.abs(got[k] - ref).max() <= 1e-8 * np.linalg.norm(ref), (a[k], b[k])
    g.compute_covariances(poses=True, landmarks=False)
    diag = g.pose_covariances(np.arange(P, dtype=np.int32))
    own = got.reshape(P, P, 6, 6)[np.arange(P), np.arange(P)]
    assert np.abs(own - diag).max() <= 1e-9 * np.abs(diag).max()
    g.close()


def test_pose_graph_pairs_far_outside_the_pattern(ctx):
    """a pure pose graph (relative-pose edges only): for the free pairs no edge joins, the joint covariance
    [[S_aa, S_ab], [S_ba, S_bb]] is symmetric and positive definite and its diagonal blocks are the marginals"""
    import relpose_lm_ref as L
    d, icp, prior, rp = L.chain_case()
    g = L.build_graph(d, icp, prior, rp)
    g.initialize()
    g.optimize(4)
    joined = {(min(x, y), max(x, y)) for x, y in zip(rp["a"], rp["b"])}
    far = [(x, y) for x in range(1, 6) for y in range(x + 1, 6) if (x, y) not in joined]
    assert (1, 4) in far and len(far) >= 3
    g.compute_covariances(poses=True, landmarks=False)
    marg = g.pose_covariances(np.arange(6, dtype=np.int32))
    for x, y in far + [(1, 5)]:  # ((1, 5): the free ends of the chain, joined by the closure)
        blk = g.pose_cross_covariances([x, x, y, y], [x, y, x, y])
        J = np.block([[blk[0], blk[1]], [blk[2], blk[3]]])
        assert np.abs(J - J.T).max() <= 1e-12 * np.abs(J).max(), (x, y)
        assert np.linalg.eigvalsh(0.5 * (J + J.T))[0] > 0, (x, y)
        assert blk[1].any()
        for k, v in ((0, x), (3, y)):
            assert np.abs(blk[k] - marg[v]).max() <= 1e-9 * np.abs(marg[v]).max(), (x, y)
    assert not g.pose_cross_covariances([0], [3]).any()  # pose 0 is fixed
    g.close()


def test_relative_pose_covariances(ctx):
    """Sigma_aa - Sigma_ab Ad^T - Ad Sigma_ba + Ad Sigma_bb Ad^T with Ad = Ad(T_a T_b^-1), from the oracle's dense blocks
    and the estimates; Sigma_aa when b is fixed; a == b is refused"""
    import relpose_ref as RR
    d, g, inv, ip = optimised("small_10x200")
    P = len(ip)
    pose = g.poses()
    a, b = all_pose_pairs(P)
    keep = a != b
    a, b = a[keep], b[keep]
    got = g.relative_pose_covariances(a, b)
    blk = lambda x, y: (inv[ip[x]:ip[x] + 6, ip[y]:ip[y] + 6] if ip[x] >= 0 and ip[y] >= 0 else np.zeros((6, 6)))
    fixed_seen = False
    for k in range(len(a)):
        Ad = RR.adjoint(*RR.relative(pose[a[k]], pose[b[k]]))
        ref = blk(a[k], a[k]) - blk(a[k], b[k]) @ Ad.T - Ad @ blk(b[k], a[k]) + Ad @ blk(b[k], b[k]) @ Ad.T
        # every block is held to 1e-8 of its norm (assert_blocks_match); the four terms carry that through
        nA = np.linalg.norm(Ad, 2)
        tol = 1e-8 * (np.linalg.norm(blk(a[k], a[k])) + 2 * nA * np.linalg.norm(blk(a[k], b[k])) +
                      nA * nA * np.linalg.norm(blk(b[k], b[k])))
        assert np.abs(got[k] - ref).max() <= tol, (a[k], b[k])
        if ip[b[k]] < 0 and ip[a[k]] >= 0:
            fixed_seen = True
            assert np.abs(got[k] - blk(a[k], a[k])).max() <= 1e-8 * np.linalg.norm(blk(a[k], a[k]))
    assert fixed_seen
    with pytest.raises(cugo.CugoError, match="error -3"):
        g.relative_pose_covariances([1, 2], [3, 2])
    g.close()


def test_cross_covariances_leave_the_optimiser_and_the_marginals_alone(ctx):
    """optimize(5); pose_cross_covariances(); optimize(5) gives the bits of optimize(5); optimize(5); marginals stored
    before the call are handed out unchanged after it"""
    d = cugo.synth(60, 900, 3700, seed=1)
    a = cugo.graph_from_arrays(d)
    a.initialize()
    a.optimize(5)
    a.compute_covariances()
    cp, cl = a.pose_covariances(), a.landmark_covariances()
    rng = np.random.default_rng(1)
    x1 = a.pose_cross_covariances(rng.integers(0, 60, 40), rng.integers(0, 60, 40))
    assert x1.any()
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


def test_cross_covariances_refusals(ctx):
    """before initialize(), for an id the graph does not know, and in the fp32-internal mode"""
    d = cugo.synth(20, 300, 1300, seed=6)
    g = cugo.graph_from_arrays(d)
    with pytest.raises(cugo.CugoError, match="error -3"):
        g.pose_cross_covariances([1], [2])
    g.initialize()
    with pytest.raises(cugo.CugoError, match="error -3"):
        g.pose_cross_covariances([1], [20])
    with pytest.raises(cugo.CugoError, match="error -3"):
        g.relative_pose_covariances([-1], [2])
    assert g.pose_cross_covariances([1], [2]).any()
    g.close()
    f = cugo.graph_from_arrays(d)
    f.set_float32(1)
    f.initialize()
    with pytest.raises(cugo.CugoError, match="error -3"):
        f.pose_cross_covariances([1], [2])
    f.close()
