"""GPU tests of the marginal covariances: the selected inverse of the sparse LL^T
(cugo_chol_selected_inverse) against numpy's inverse, and the graph-level covariances
(cugo_graph_compute_covariances) against H^-1 built independently from the CPU oracle's normal
equations at the same estimates."""
import ctypes as C
import importlib

import numpy as np
import pytest

from conftest import PROBLEM_KEYS, golden_path

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
ERR_NUMERIC = -4


@pytest.fixture(scope="module")
def ctx():
    import devmem
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    c = devmem.Ctx()
    yield c
    c.close()


# ------------------------------------------------------------------ kernel level ---------
@pytest.mark.gpu
# the environment variants of tests/test_gpu.py::test_sparse_cholesky_vs_numpy: every layout the factorisation can
# leave W and L21 in
@pytest.mark.parametrize("env", [{}, {"CUGO_MIN_SUBTREE_TASKS": "0"}, {"CUGO_ALIAS_CHAINS": "0"},
                                 {"CUGO_ND_LEAF": "4", "CUGO_MAX_SUPER_COLS": "3", "CUGO_TARGET_TASKS": "4",
                                  "CUGO_MIN_SUBTREE_TASKS": "0"},
                                 {"CUGO_ND_LEAF": "1000", "CUGO_MAX_SUPER_COLS": "1", "CUGO_TARGET_TASKS": "100000"},
                                 {"CUGO_MAX_SUPER_COLS": "24", "CUGO_ZERO_FRAC": "0.9", "CUGO_MIN_SUBTREE_TASKS": "0"},
                                 {"CUGO_TILE32_MAX_TILES": "0"},
                                 {"CUGO_TILE32_MAX_TILES": "0", "CUGO_ALIAS_CHAINS": "0", "CUGO_MAX_SUPER_COLS": "5"},
                                 {"CUGO_LOOKAHEAD": "1"},
                                 {"CUGO_LOOKAHEAD": "1", "CUGO_TILE32_MAX_TILES": "0", "CUGO_ALIAS_CHAINS": "0"},
                                 {"CUGO_LOOKAHEAD": "1", "CUGO_MIN_SUBTREE_TASKS": "0", "CUGO_MAX_SUPER_COLS": "5"},
                                 {"CUGO_TWO_PHASE_MIN_TILES": "1", "CUGO_TILE32_MAX_TILES": "0"},
                                 {"CUGO_TWO_PHASE_MIN_TILES": "1", "CUGO_TILE32_MAX_TILES": "0", "CUGO_ALIAS_CHAINS": "0",
                                  "CUGO_MAX_SUPER_COLS": "5"},
                                 {"CUGO_PANEL16": "0"},
                                 {"CUGO_PANEL16": "0", "CUGO_MIN_SUBTREE_TASKS": "0", "CUGO_MAX_SUPER_COLS": "5"},
                                 {"CUGO_ASM_FRONTS": "0"},
                                 {"CUGO_ASM_FRONTS": "0", "CUGO_ALIAS_CHAINS": "0", "CUGO_MAX_SUPER_COLS": "5"}])
def test_selected_inverse_vs_numpy(ctx, env, monkeypatch):
    """the blocks of (A + lambda I)^-1 on the pattern, every factorisation form the plan can take; the same bits
    on a second call; CUGO_ERR_NUMERIC after a factorisation that raised the zero-pivot flag"""
    from test_host import covis_pattern, patterns, random_spd_bsr
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(5)
    cases = dict(patterns())
    d = cugo.synth(160, 2500, 10500, seed=3, n_loop_closures=80)
    ep = d["e_pose"].astype(np.int64) - 1
    ep[ep < 0] = 10**6
    cases["synthetic"] = covis_pattern(159, ep, d["e_lm"])
    L = cugo.lib()
    for name, pat in cases.items():
        if isinstance(pat, tuple):
            rowptr, colind = pat
        else:
            rowptr = np.array([0] + list(np.cumsum([len(r) for r in pat])), np.int32)
            colind = np.array([c for r in pat for c in r], np.int32)
        n, B = len(rowptr) - 1, len(colind)
        A, vals = random_spd_bsr(rowptr, colind, rng)
        s = C.c_void_p()
        cugo.check(L.cugo_chol_create(ctx.h, C.byref(s)))
        cugo.check(L.cugo_chol_analyze(s, n, rowptr.ctypes.data_as(C.POINTER(C.c_int32)),
                                       colind.ctypes.data_as(C.POINTER(C.c_int32))))
        assert L.cugo_chol_selected_inverse(s, None) == -3, name  # no factorisation yet
        b = rng.normal(size=6 * n)
        dH, db, dx, fail = ctx.to_dev(vals), ctx.to_dev(b), ctx.empty(6 * n), ctx.empty(2, np.int32)
        dS = ctx.empty(36 * B)
        for lam in (0.0, 2.5):
            cugo.check(L.cugo_chol_factor_solve(s, dH, C.c_double(lam), db, dx, fail))
            cugo.check(L.cugo_chol_selected_inverse(s, dS))
            got = ctx.to_host(dS, 36 * B).reshape(B, 36)
            inv = np.linalg.inv(A + lam * np.eye(6 * n))
            for r in range(n):
                for k in range(rowptr[r], rowptr[r + 1]):
                    c = colind[k]
                    np.testing.assert_allclose(got[k].reshape(6, 6).T, inv[6 * r:6 * r + 6, 6 * c:6 * c + 6],
                                               rtol=1e-9, atol=1e-9 * np.abs(inv).max(), err_msg=name)
            cugo.check(L.cugo_chol_selected_inverse(s, dS))
            assert np.array_equal(ctx.to_host(dS, 36 * B).reshape(B, 36), got), name
        bad = vals.copy()
        bad[rowptr[n // 2]] = -np.eye(6).reshape(-1)
        cugo.check(L.cugo_chol_factor_solve(s, ctx.to_dev(bad), C.c_double(0.0), db, dx, fail))
        assert L.cugo_chol_selected_inverse(s, dS) == ERR_NUMERIC, name
        L.cugo_chol_destroy(s)


# ------------------------------------------------------------------ graph level ----------
def oracle_problem(d, rk=(0, 1.0), pose=None, lm=None):
    import oracle
    prob = oracle.Problem(*[d[k] for k in PROBLEM_KEYS], rk_type=rk[0], rk_delta=rk[1])
    if pose is not None:
        prob.pose[:] = pose
        prob.lm[:] = lm
    return prob


def dense_inverse(prob):
    """H^-1 over the free vertices from the oracle's normal equations; pose p's block starts at ip[p],
    landmark l's at il[l] (-1: fixed)"""
    pi, li, npf, nlf = prob.indices()
    sysm = prob.build_system()
    Hpp, Hll, Hpl = sysm["Hpp"], sysm["Hll"], sysm["Hpl"]
    fp = (prob.pose_fixed == 0) & (pi < npf)
    fl = (prob.lm_fixed == 0) & (li < nlf)
    n = 6 * npf + 3 * nlf
    H = np.zeros((n, n))
    for p in range(npf):
        H[6 * p:6 * p + 6, 6 * p:6 * p + 6] = Hpp[p].reshape(6, 6).T
    for l in range(nlf):
        o = 6 * npf + 3 * l
        H[o:o + 3, o:o + 3] = Hll[l].reshape(3, 3).T
    for e in range(prob.n_edges):
        p, l = prob.e_pose[e], prob.e_lm[e]
        if fp[p] and fl[l]:
            a, o = 6 * pi[p], 6 * npf + 3 * li[l]
            blk = Hpl[e].reshape(3, 6).T
            H[a:a + 6, o:o + 3] += blk
            H[o:o + 3, a:a + 6] += blk.T
    ip = np.where(fp, 6 * pi, -1)
    il = np.where(fl, 6 * npf + 3 * li, -1)
    return np.linalg.inv(H), ip, il


def assert_blocks_match(g, inv, ip, il, tol=1e-8, tol_lm=None):
    tol_lm = tol if tol_lm is None else tol_lm
    P = len(ip)
    cp = g.pose_covariances(np.arange(P, dtype=np.int32))
    for p in range(P):
        if ip[p] < 0:
            assert not cp[p].any()
        else:
            ref = inv[ip[p]:ip[p] + 6, ip[p]:ip[p] + 6]
            assert np.abs(cp[p] - ref).max() <= tol * np.linalg.norm(ref), p
    cl = g.landmark_covariances(np.arange(len(il), dtype=np.int32))
    for l in range(len(il)):
        if il[l] < 0:
            assert not cl[l].any()
        else:
            ref = inv[il[l]:il[l] + 3, il[l]:il[l] + 3]
            assert np.abs(cl[l] - ref).max() <= tol_lm * np.linalg.norm(ref), l


def golden(name):
    z = np.load(golden_path(name + ".npz"))
    return {k: z[k] for k in PROBLEM_KEYS}, (int(z["rk_type"]), float(z["rk_delta"]))


def stereo_synth(rk):
    d = cugo.synth(40, 700, 2900, seed=21, stereo_fraction=0.6)
    assert d["pose_fixed"][0] == 1 and d["e_stereo"].any()
    return d, rk


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["small_10x200", "loop_12x150", "cauchy_8x80", "huber_8x80",
                                  "synth_none", "synth_cauchy", "synth_huber"])
def test_graph_covariances_vs_dense_inverse(ctx, case):
    if case.startswith("synth"):
        d, rk = stereo_synth({"synth_none": (0, 1.0), "synth_cauchy": (1, 2.0), "synth_huber": (3, 2.0)}[case])
    else:
        d, rk = golden(case)
    g = cugo.graph_from_arrays(d, rk=rk)
    g.initialize()
    g.optimize(5)
    g.compute_covariances()
    prob = oracle_problem(d, rk, g.poses(), g.landmarks())
    inv, ip, il = dense_inverse(prob)
    assert_blocks_match(g, inv, ip, il)
    g.close()


@pytest.mark.gpu
def test_all_landmarks_fixed_gives_inverse_hpp(ctx):
    d = cugo.synth(20, 300, 1300, seed=4)
    d["lm_fixed"][:] = 1
    g = cugo.graph_from_arrays(d)
    g.initialize()
    g.optimize(3)
    g.compute_covariances()
    prob = oracle_problem(d, (0, 1.0), g.poses(), g.landmarks())
    pi, _, npf, _ = prob.indices()
    Hpp = prob.build_system()["Hpp"]
    cp = g.pose_covariances(np.arange(20, dtype=np.int32))
    assert not cp[0].any()
    for p in range(1, 20):
        ref = np.linalg.inv(Hpp[pi[p]].reshape(6, 6).T)
        assert np.abs(cp[p] - ref).max() <= 1e-8 * np.linalg.norm(ref)
    assert not g.landmark_covariances(np.arange(300, dtype=np.int32)).any()
    g.close()


@pytest.mark.gpu
def test_all_poses_fixed_gives_inverse_hll(ctx):
    d = cugo.synth(20, 300, 1300, seed=4)
    d["pose_fixed"][:] = 1
    g = cugo.graph_from_arrays(d)
    g.initialize()
    g.optimize(3)
    g.compute_covariances()
    prob = oracle_problem(d, (0, 1.0), g.poses(), g.landmarks())
    _, li, _, _ = prob.indices()
    Hll = prob.build_system()["Hll"]
    cl = g.landmark_covariances(np.arange(300, dtype=np.int32))
    for l in range(300):
        ref = np.linalg.inv(Hll[li[l]].reshape(3, 3).T)
        assert np.abs(cl[l] - ref).max() <= 1e-8 * np.linalg.norm(ref)
    assert not g.pose_covariances(np.arange(20, dtype=np.int32)).any()
    g.close()


@pytest.mark.gpu
def test_free_pose_without_edges_is_a_zero_pivot(ctx):
    """a free pose that no edge observes stays free in the flattening (its Hpp block is exactly zero at
    lambda = 0): CUGO_ERR_NUMERIC; optimize() on the same graph still runs as on the graph without it"""
    d = cugo.synth(20, 300, 1300, seed=6)
    ref = cugo.graph_from_arrays(d)
    ref.initialize()
    ref.optimize(4)
    e = dict(d)
    e["pose"] = np.concatenate([d["pose"], d["pose"][-1:]])
    e["pose_fixed"] = np.concatenate([d["pose_fixed"], [0]]).astype(d["pose_fixed"].dtype)
    g = cugo.graph_from_arrays(e)
    g.initialize()
    with pytest.raises(cugo.CugoError, match="error -4"):
        g.compute_covariances()
    g.optimize(4)
    assert [s["chi2"] for s in g.stats()] == pytest.approx([s["chi2"] for s in ref.stats()], rel=1e-10)
    with pytest.raises(cugo.CugoError):
        g.pose_covariances(np.arange(3, dtype=np.int32))  # nothing was kept
    g.close()
    ref.close()


@pytest.mark.gpu
def test_covariances_leave_the_optimiser_as_they_found_it(ctx):
    """optimize(5); compute_covariances(); optimize(5) gives the bits of optimize(5); optimize(5); two calls give
    the same bits; before initialize() the call is refused"""
    d = cugo.synth(60, 900, 3700, seed=1)
    a = cugo.graph_from_arrays(d)
    with pytest.raises(cugo.CugoError, match="error -3"):
        a.compute_covariances()
    a.initialize()
    a.optimize(5)
    a.compute_covariances()
    c1p, c1l = a.pose_covariances(), a.landmark_covariances()
    a.compute_covariances()
    assert np.array_equal(a.pose_covariances(), c1p) and np.array_equal(a.landmark_covariances(), c1l)
    a.optimize(5)
    b = cugo.graph_from_arrays(d)
    b.initialize()
    b.optimize(5)
    b.optimize(5)
    assert a.stats() == b.stats()
    assert np.array_equal(a.poses(), b.poses()) and np.array_equal(a.landmarks(), b.landmarks())
    a.initialize()  # the results go with the flattening they were computed on
    with pytest.raises(cugo.CugoError):
        a.landmark_covariances()
    a.close()
    b.close()


@pytest.mark.gpu
def test_covariances_after_an_estimates_only_initialize(ctx):
    """initialize(); optimize(); initialize() on the unchanged graph (the estimates-only path SLAM back ends take)
    and then compute_covariances(): the call runs and gives the same bits as on a graph flattened in full from the
    same estimates"""
    d = cugo.synth(60, 900, 3700, seed=2)
    g = cugo.graph_from_arrays(d)
    g.initialize()
    g.optimize(3)
    g.initialize()
    assert g.flatten_reuses() == 1
    g.compute_covariances()
    f = cugo.graph_from_arrays(dict(d, pose=g.poses(), lm=g.landmarks()))
    f.initialize()
    f.compute_covariances()
    assert np.array_equal(g.pose_covariances(), f.pose_covariances())
    assert np.array_equal(g.landmark_covariances(), f.landmark_covariances())
    g.close()
    f.close()


@pytest.mark.gpu
def test_covariances_refuse_vertices_the_flattening_does_not_know(ctx):
    """a vertex added after compute_covariances() (no new initialize()) has no block: the getter fails instead of
    returning another vertex's block or zeros, and so does a new compute_covariances() until initialize() runs"""
    d = cugo.synth(30, 400, 1700, seed=3)
    g = cugo.graph_from_arrays(d)
    g.initialize()
    g.optimize(2)
    g.compute_covariances(poses=True, landmarks=False)
    before = g.pose_covariances(np.arange(30, dtype=np.int32))
    with pytest.raises(cugo.CugoError, match="error -3"):
        g.landmark_covariances(np.arange(3, dtype=np.int32))  # (not asked for)
    g.add_landmarks(np.array([400], np.int32), np.zeros((1, 3)), np.zeros(1, np.uint8))
    assert np.array_equal(g.pose_covariances(np.arange(30, dtype=np.int32)), before)  # (the pose set is unchanged)
    g.add_poses(np.array([30], np.int32), d["pose"][-1:], np.zeros(1, np.uint8))
    with pytest.raises(cugo.CugoError, match="error -3"):
        g.pose_covariances(np.array([30], np.int32))
    with pytest.raises(cugo.CugoError, match="error -3"):
        g.pose_covariances(np.array([1], np.int32))
    with pytest.raises(cugo.CugoError, match="error -3"):
        g.compute_covariances()
    g.close()


@pytest.mark.gpu
def test_medium_graph_with_loop_closures_vs_oracle_schur(ctx):
    """a few hundred poses (many levels, alias chains, tile launches): the pose blocks against numpy.linalg.solve
    of the oracle's dense Hsc at lambda = 0, the landmark blocks against Hll^-1 + sum T_e^T Sigma T_f"""
    d = cugo.synth(300, 6000, 26000, seed=9, n_loop_closures=120)
    g = cugo.graph_from_arrays(d)
    g.initialize()
    g.optimize(5)
    g.compute_covariances()
    prob = oracle_problem(d, (0, 1.0), g.poses(), g.landmarks())
    pi, li, npf, nlf = prob.indices()
    Hsc, _ = prob.schur_dense(0.0)
    Hsc = np.asarray(Hsc).reshape(6 * npf, 6 * npf)
    S = np.linalg.inv(Hsc)
    P, Lm = len(d["pose"]), len(d["lm"])
    cp = g.pose_covariances(np.arange(P, dtype=np.int32))
    free_p = (d["pose_fixed"] == 0)
    for p in range(P):
        if not free_p[p]:
            assert not cp[p].any()
            continue
        ref = S[6 * pi[p]:6 * pi[p] + 6, 6 * pi[p]:6 * pi[p] + 6]
        assert np.abs(cp[p] - ref).max() <= 1e-8 * np.linalg.norm(ref), p
    sysm = prob.build_system()
    Hll, Hpl = sysm["Hll"], sysm["Hpl"]
    cl = g.landmark_covariances(np.arange(Lm, dtype=np.int32))
    order = np.argsort(d["e_lm"], kind="stable")
    starts = np.searchsorted(d["e_lm"][order], np.arange(Lm + 1))
    for l in range(0, Lm, 7):  # every seventh landmark
        if d["lm_fixed"][l]:
            continue
        Hinv = np.linalg.inv(Hll[li[l]].reshape(3, 3).T)
        es = [e for e in order[starts[l]:starts[l + 1]] if free_p[d["e_pose"][e]]]
        T = [(6 * pi[d["e_pose"][e]], Hpl[e].reshape(3, 6).T @ Hinv) for e in es]
        ref = Hinv.copy()
        for a, Ta in T:
            for b, Tb in T:
                ref += Ta.T @ S[a:a + 6, b:b + 6] @ Tb
        assert np.abs(cl[l] - ref).max() <= 1e-8 * np.linalg.norm(ref), l
    g.close()


@pytest.mark.gpu
def test_kitti00_shape_covariances_are_positive_definite(ctx):
    """the kitti_00 shape at full size (the graph tools/cov_time.py times): every block finite, symmetric and
    positive definite"""
    d = cugo.synth(1322, 133383, 561116, seed=0, n_loop_closures=4000)
    g = cugo.graph_from_arrays(d)
    g.initialize()
    g.optimize(10)
    g.compute_covariances()
    cp = g.pose_covariances()[1:]  # (pose 0 is the fixed gauge)
    cl = g.landmark_covariances()
    assert not g.pose_covariances(np.array([0], np.int32)).any()
    for blocks in (cp, cl):
        assert np.isfinite(blocks).all()
        assert np.array_equal(blocks, blocks.transpose(0, 2, 1))
        assert (np.linalg.eigvalsh(blocks)[:, 0] > 0).all()
    g.close()


# ------------------------------------------------------------------ graph level: degrees, outliers, dead landmarks ----------
def layout_b_graph(with_300):
    """the landmark degree set of layout B (tests/designed.py: 1, 2, 100, 255, 256, 3, 257, 300, ... on 304 poses, four of
    them fixed) as a graph the covariances exist for: its edgeless landmarks fixed, the one edge of the degree-1
    landmark stereo (a mono edge alone leaves Hll with rank 2), and 40 further landmarks of 64 edges laid out with a
    stride so that every pose sees at least eight landmarks in both variants (layout B alone leaves poses with two or
    three edges, and H singular at lambda = 0).  with_300 = False: the 300-edge landmark loses its pose set (and is
    fixed with the other edgeless ones)"""
    import designed
    import synth
    n_poses, fixed_p = 304, (1, 77, 150, 200)
    degs = [k if (with_300 or k != 300) else 0 for k in designed.B_LM_DEGREES]
    lmd = degs[:2] + [3] + degs[2:9] + [3] + degs[9:]
    fixed_l = [2, 10] + [i for i, k in enumerate(lmd) if k == 0]
    rng = np.random.default_rng(5)
    free_p = np.array([p for p in range(n_poses) if p not in fixed_p])
    sets = [np.sort(rng.choice(free_p if l in fixed_l else np.arange(n_poses), k, replace=False)) if k else [] for l, k in enumerate(lmd)]
    sets += [np.sort((37 * j + 5 * np.arange(64)) % n_poses) for j in range(40)]      # (5 and 304 are coprime)
    lmd = [len(s) for s in sets]
    ep = [int(p) for s in sets for p in s]
    el = [l for l, s in enumerate(sets) for _ in s]
    d = designed._assemble(rng, n_poses, len(sets), ep, el, fixed_p, tuple(fixed_l))
    l1 = lmd.index(1)
    e = int(np.flatnonzero(d["e_lm"] == l1)[0])
    if not d["e_stereo"][e]:
        p = d["pose_gt"][d["e_pose"][e]]
        z = (synth.quat_to_R(p[:4]) @ d["lm_gt"][l1] + p[4:])[2]
        d["e_stereo"][e] = 1
        d["e_meas"][e, 2] = d["e_meas"][e, 0] - synth.KITTI_CAM[4] / z
    deg = np.bincount(d["e_lm"], minlength=len(lmd))
    assert deg.tolist() == lmd and (300 in lmd) == with_300 and np.bincount(d["e_pose"], minlength=n_poses).min() >= 8
    assert sorted(k for k in lmd[:19] if k) == sorted([k for k in designed.B_LM_DEGREES if k and (with_300 or k != 300)] + [3, 3])
    assert np.flatnonzero(d["lm_fixed"]).tolist() == sorted(fixed_l) and not d["lm_fixed"][-1]
    return d


def schur_route(prob, d):
    """the second CPU route to the blocks (test_medium_graph_with_loop_closures_vs_oracle_schur): the pose blocks from
    numpy.linalg.inv of the oracle's dense Hsc at lambda = 0, the landmark blocks Hll^-1 + sum T_e^T Sigma T_f; blocks
    by caller id, None for fixed vertices"""
    pi, li, npf, nlf = prob.indices()
    Hsc, _ = prob.schur_dense(0.0)
    S = np.linalg.inv(np.asarray(Hsc).reshape(6 * npf, 6 * npf))
    free_p, free_l = d["pose_fixed"] == 0, d["lm_fixed"] == 0
    cp = [S[6 * pi[p]:6 * pi[p] + 6, 6 * pi[p]:6 * pi[p] + 6] if free_p[p] else None for p in range(len(free_p))]
    sysm = prob.build_system()
    Hll, Hpl = sysm["Hll"], sysm["Hpl"]
    order = np.argsort(d["e_lm"], kind="stable")
    starts = np.searchsorted(d["e_lm"][order], np.arange(len(free_l) + 1))
    cl = []
    for l in range(len(free_l)):
        if not free_l[l]:
            cl.append(None)
            continue
        Hinv = np.linalg.inv(Hll[li[l]].reshape(3, 3).T)
        es = [e for e in order[starts[l]:starts[l + 1]] if free_p[d["e_pose"][e]]]
        ref = Hinv.copy()
        if es:
            T = np.concatenate([Hpl[e].reshape(3, 6).T @ Hinv for e in es])                       # [6 d, 3]
            idx = (6 * pi[d["e_pose"][es]][:, None] + np.arange(6)).reshape(-1)
            ref += T.T @ S[np.ix_(idx, idx)] @ T
        cl.append(ref)
    return cp, cl


@pytest.mark.gpu
@pytest.mark.parametrize("with_300", [True, False], ids=["all", "without_300"])
def test_layout_b_degree_set_vs_dense_inverse(ctx, with_300):
    """landmarks of 1 to 300 edges in one graph: every pose and landmark block against the dense inverse of the oracle's
    normal equations at the graph's estimates.  The tolerance is measured on the same problem: 4 x the disagreement
    between numpy.linalg.inv of the full H and the Schur route, per kind of block, relative to the block's norm"""
    d = layout_b_graph(with_300)
    g = cugo.graph_from_arrays(d)
    g.initialize()
    g.optimize(3)
    g.compute_covariances()
    prob = oracle_problem(d, (0, 1.0), g.poses(), g.landmarks())
    inv, ip, il = dense_inverse(prob)
    cp, cl = schur_route(prob, d)
    dis_p = max(np.abs(cp[p] - inv[ip[p]:ip[p] + 6, ip[p]:ip[p] + 6]).max() / np.linalg.norm(inv[ip[p]:ip[p] + 6, ip[p]:ip[p] + 6])
                for p in range(len(ip)) if ip[p] >= 0)
    dis_l = max(np.abs(cl[l] - inv[il[l]:il[l] + 3, il[l]:il[l] + 3]).max() / np.linalg.norm(inv[il[l]:il[l] + 3, il[l]:il[l] + 3])
                for l in range(len(il)) if il[l] >= 0)
    got_p, got_l = g.pose_covariances(np.arange(len(ip), dtype=np.int32)), g.landmark_covariances(np.arange(len(il), dtype=np.int32))
    err_p = max(np.abs(got_p[p] - inv[ip[p]:ip[p] + 6, ip[p]:ip[p] + 6]).max() / np.linalg.norm(inv[ip[p]:ip[p] + 6, ip[p]:ip[p] + 6])
                for p in range(len(ip)) if ip[p] >= 0)
    err_l = max(np.abs(got_l[l] - inv[il[l]:il[l] + 3, il[l]:il[l] + 3]).max() / np.linalg.norm(inv[il[l]:il[l] + 3, il[l]:il[l] + 3])
                for l in range(len(il)) if il[l] >= 0)
    print("layout B degrees (%s): the two CPU routes disagree by %.3g (poses) and %.3g (landmarks) of a block's norm; "
          "tolerances 4 x that; the graph is off by %.3g and %.3g" % ("all" if with_300 else "without 300", dis_p, dis_l, err_p, err_l))
    assert (il < 0).sum() == (7 if with_300 else 8) and (ip < 0).sum() == 4
    assert_blocks_match(g, inv, ip, il, tol=4 * dis_p, tol_lm=4 * dis_l)
    g.close()


def edge_flags(g, d):
    """the active flags of the mono and stereo sets in the order of d's edges (mono edges, then stereo edges, each in
    insertion order)"""
    st = d["e_stereo"].astype(bool)
    act = np.ones(len(st), bool)
    act[~st] = g.edge_active(2, int((~st).sum()))
    act[st] = g.edge_active(3, int(st.sum()))
    return act


def without_edges(d, keep, pose=None, lm=None, fix_lm=()):
    e = dict(d)
    for k in ("e_pose", "e_lm", "e_stereo", "e_meas", "e_omega", "e_cam"):
        e[k] = d[k][keep]
    if pose is not None:
        e["pose"], e["lm"] = pose, lm
    e["lm_fixed"] = d["lm_fixed"].copy()
    e["lm_fixed"][list(fix_lm)] = 1
    return e


# chi2 thresholds of the outlier tests below, mono and stereo.  The 95 % quantiles of test_outlier_rejection_matches_oracle
# (5.991, 7.815) also reject some two hundred good edges of the poses that the gross outliers drag along, and with them every
# edge of a few low-degree landmarks; these reject the gross outliers (chi2 > 500) and a handful of their neighbours
OUTLIER_THRESHOLDS = {2: 100.0, 3: 130.0}


@pytest.mark.gpu
def test_landmark_covariances_after_reprojection_outlier_rejection(ctx):
    """gross outliers (+-60 px, as in test_outlier_rejection_matches_oracle) on 20 edges of landmarks with ten edges or
    more, one per landmark: after optimize() with thresholds the rejected edges are INACTIVE slots of the same
    flattening, and compute_covariances() must leave them out; after a new initialize() they are gone from the
    flattening.  Both against the dense inverse of the reduced system at the same estimates.  No free landmark is left
    with fewer than two edges (asserted from the flags the graph reports)"""
    d = cugo.synth(20, 300, 2400, seed=2)
    deg = np.bincount(d["e_lm"], minlength=300)
    rng = np.random.default_rng(4)
    cand = [int(rng.choice(np.flatnonzero(d["e_lm"] == l))) for l in np.flatnonzero(deg >= 10)]
    bad = rng.choice(cand, 20, replace=False)
    d["e_meas"] = d["e_meas"].copy()
    d["e_meas"][bad, :2] += rng.choice([-1.0, 1.0], (20, 2)) * 60.0
    g = cugo.graph_from_arrays(d)
    for dim, t in OUTLIER_THRESHOLDS.items():
        g.set_outlier_threshold(dim, t)
    g.initialize()
    g.optimize(5)
    act = edge_flags(g, d)
    assert not act[bad].any() and 20 <= (~act).sum() <= 60, int((~act).sum())
    left = np.bincount(d["e_lm"][act], minlength=300)
    assert left.min() >= 2, "a landmark lost its edges: %s" % np.flatnonzero(left < 2)
    assert g.n_active_edges() == int(act.sum())
    g.compute_covariances()
    red = without_edges(d, act, g.poses(), g.landmarks())
    inv, ip, il = dense_inverse(oracle_problem(red))
    full, _, _ = dense_inverse(oracle_problem(d, (0, 1.0), g.poses(), g.landmarks()))
    lb = int(d["e_lm"][bad[0]])
    assert np.abs(full[il[lb]:il[lb] + 3, il[lb]:il[lb] + 3] - inv[il[lb]:il[lb] + 3, il[lb]:il[lb] + 3]).max() > \
        1e-4 * np.linalg.norm(inv[il[lb]:il[lb] + 3, il[lb]:il[lb] + 3])   # (the rejected edge would show)
    assert_blocks_match(g, inv, ip, il)
    first = g.landmark_covariances()
    g.initialize()
    with pytest.raises(cugo.CugoError):
        g.landmark_covariances()
    g.compute_covariances()
    assert np.array_equal(g.poses(), red["pose"]) and np.array_equal(g.landmarks(), red["lm"])
    assert_blocks_match(g, inv, ip, il)
    assert np.abs(g.landmark_covariances() - first).max() <= 2e-8 * np.abs(first).max()
    g.close()


def dead_landmark_case(case):
    """(problem dict, id of the free landmark that ends without an active edge, thresholds or None).  never: a free
    landmark that no edge ever saw; rejected: a degree-2 landmark whose two edges are gross outliers that cannot be
    triangulated together (+60, -60 on one, -60, +60 on the other)"""
    d = cugo.synth(20, 300, 1300, seed=6)
    if case == "never":
        d = dict(d, lm=np.concatenate([d["lm"], d["lm"][-1:] + 1.0]),
                 lm_fixed=np.concatenate([d["lm_fixed"], [0]]).astype(d["lm_fixed"].dtype))
        return d, 300, None
    deg = np.bincount(d["e_lm"], minlength=300)
    dead = int(np.flatnonzero(deg == 2)[2])
    es = np.flatnonzero(d["e_lm"] == dead)
    d["e_meas"] = d["e_meas"].copy()
    d["e_meas"][es[0], :2] += [60.0, -60.0]
    d["e_meas"][es[1], :2] += [-60.0, 60.0]
    return d, dead, OUTLIER_THRESHOLDS


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["never", "rejected"])
def test_free_landmark_without_an_active_edge(ctx, case):
    """Hll of such a landmark is exactly zero at lambda = 0: the landmark covariances (what = 2 and 3) fail as a whole
    with CUGO_ERR_NUMERIC and keep nothing, the pose covariances (what = 1) succeed and match the dense inverse of the
    system without that landmark, and optimize() afterwards gives the bits it gives without the covariance calls"""
    d, dead, th = dead_landmark_case(case)

    def start():
        g = cugo.graph_from_arrays(d)
        for dim, t in (th or {}).items():
            g.set_outlier_threshold(dim, t)
        g.initialize()
        g.optimize(5)
        return g
    g, twin = start(), start()
    act = edge_flags(g, d)
    if case == "rejected":
        assert not act[d["e_lm"] == dead].any() and (~act).sum() == 2, np.flatnonzero(~act)
    else:
        assert act.all()
    left = np.bincount(d["e_lm"][act], minlength=len(d["lm"]))
    assert left[dead] == 0 and (np.delete(left, dead) >= 2).all()
    with pytest.raises(cugo.CugoError, match="error -4"):
        g.compute_covariances(poses=False, landmarks=True)
    with pytest.raises(cugo.CugoError, match="error -4"):
        g.compute_covariances()
    with pytest.raises(cugo.CugoError, match="error -3"):
        g.pose_covariances(np.arange(3, dtype=np.int32))       # nothing was kept
    with pytest.raises(cugo.CugoError, match="error -3"):
        g.landmark_covariances(np.arange(3, dtype=np.int32))
    g.compute_covariances(poses=True, landmarks=False)
    red = without_edges(d, act, g.poses(), g.landmarks(), fix_lm=(dead,))
    inv, ip, _ = dense_inverse(oracle_problem(red))
    cp = g.pose_covariances(np.arange(len(ip), dtype=np.int32))
    for p in range(len(ip)):
        if ip[p] < 0:
            assert not cp[p].any()
        else:
            ref = inv[ip[p]:ip[p] + 6, ip[p]:ip[p] + 6]
            assert np.abs(cp[p] - ref).max() <= 1e-8 * np.linalg.norm(ref), p
    with pytest.raises(cugo.CugoError, match="error -3"):
        g.landmark_covariances(np.arange(3, dtype=np.int32))   # (not asked for)
    g.optimize(4)
    twin.optimize(4)
    assert g.stats() == twin.stats()
    assert np.array_equal(g.poses(), twin.poses()) and np.array_equal(g.landmarks(), twin.landmarks())
    g.close()
    twin.close()
