"""CPU tests of the separator refinement of the nested-dissection ordering (chol_symbolic.cpp, ND::refine_split,
CUGO_ND_REFINE): the plans stay valid (numpy replay solves the system), the ordering is deterministic, the switch
reproduces the unrefined plan, the kitti_00 plan gets shorter, and no bench shape gets a worse plan."""
import ctypes as C
import importlib

import numpy as np
import pytest

from test_host import covis_pattern, patterns, plan_arrays, random_spd_bsr, replay_multifrontal

cugo = importlib.import_module("cuda-bundle-adjustment_amd")

# (poses, landmarks, edges, seed, loop-closure landmarks, stereo fraction) of the bench workloads
SHAPES = {
    "kitti00": (1322, 133383, 561116, 0, 4000, 0.7),
    "kitti07": (248, 26127, 95037, 7, 500, 0.7),
    "synth10k": (10000, 1000000, 5000000, 10000, 0, 0.0),
    "localba": (30, 3000, 12600, 30, 0, 0.7),
}


@pytest.fixture(scope="module")
def lib():
    cugo.build()
    return cugo.lib()


def small_pattern(name):
    if name == "synthetic":
        d = cugo.synth(120, 1500, 6200, seed=3, n_loop_closures=60)
        ep = d["e_pose"].astype(np.int64) - 1  # pose 0 is fixed
        ep[ep < 0] = 10**6
        return covis_pattern(119, ep, d["e_lm"])
    rows = patterns()[name]
    return (np.array([0] + list(np.cumsum([len(r) for r in rows])), np.int32),
            np.array([c for r in rows for c in r], np.int32))


def covis_pattern_np(d):
    """covis_pattern of test_host for a flat-array problem, vectorised: edges grouped by landmark, every pair of
    free poses of a group (upper triangle, diagonal included) is a block"""
    pf, lf = d["pose_fixed"].astype(bool), d["lm_fixed"].astype(bool)
    index = np.cumsum(~pf) - 1
    keep = ~pf[d["e_pose"]] & ~lf[d["e_lm"]]
    p, l = index[d["e_pose"][keep]].astype(np.int64), d["e_lm"][keep].astype(np.int64)
    n = int((~pf).sum())
    o = np.lexsort((p, l))
    p, l = p[o], l[o]
    starts = np.flatnonzero(np.r_[True, l[1:] != l[:-1]])
    cnt = np.diff(np.r_[starts, len(l)])
    rem = np.repeat(cnt, cnt) - (np.arange(len(l)) - np.repeat(starts, cnt))  # partners at or after, itself included
    a = np.repeat(p, rem)
    b = p[np.repeat(np.arange(len(l)), rem) + np.arange(len(a)) - np.repeat(np.cumsum(rem) - rem, rem)]
    key = np.unique(np.r_[a * n + b, np.arange(n) * (n + 1)])
    rowptr = np.r_[0, np.cumsum(np.bincount(key // n, minlength=n))].astype(np.int32)
    return n, rowptr, (key % n).astype(np.int32)


def analyze(lib, n, rowptr, colind):
    s = C.c_void_p()
    assert lib.cugo_chol_create(None, C.byref(s)) == 0
    rc = lib.cugo_chol_analyze(s, n, rowptr.ctypes.data_as(C.POINTER(C.c_int32)),
                               colind.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0, lib.cugo_last_error()
    pl = plan_arrays(lib, s)
    nnzL, flops, nsup, nst, fb = C.c_double(), C.c_double(), C.c_int(), C.c_int(), C.c_double()
    lib.cugo_chol_stats(s, C.byref(nnzL), C.byref(flops), C.byref(nsup), C.byref(nst), C.byref(fb))
    lib.cugo_chol_destroy(s)
    assert nst.value == len(pl["stage_task_ptr"]) - 1
    slots = 0  # sum over the stages of the 16-column potrf slots of the stage's widest front
    for st in range(nst.value):
        t0, t1 = pl["stage_task_ptr"][st], pl["stage_task_ptr"][st + 1]
        fronts = pl["task_fronts"][pl["task_ptr"][t0]:pl["task_ptr"][t1]]
        slots += int(np.max(-(-6 * pl["ncb"][fronts] // 16)))
    return pl, {"stages": nst.value, "slots": slots, "chol_flops": flops.value, "front_bytes": fb.value}


@pytest.mark.parametrize("refine", ["1", "0", "2"])
@pytest.mark.parametrize("name", list(patterns().keys()) + ["synthetic"])
@pytest.mark.parametrize("env", [{}, {"CUGO_ND_LEAF": "4", "CUGO_MAX_SUPER_COLS": "3", "CUGO_TARGET_TASKS": "4"},
                                 {"CUGO_ND_LEAF": "1000", "CUGO_MAX_SUPER_COLS": "1", "CUGO_TARGET_TASKS": "100000"}])
def test_replay_solves_the_system_with_and_without_refinement(lib, name, env, refine, monkeypatch):
    """an invalid separator (an edge between the two halves) shows up here as a wrong solve; CUGO_ND_REFINE=2 keeps
    the refined ordering also where the default setting would prefer the plan of the unrefined one"""
    monkeypatch.setenv("CUGO_ND_REFINE", refine)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(1)
    rowptr, colind = small_pattern(name)
    n = len(rowptr) - 1
    A, vals = random_spd_bsr(rowptr, colind, rng)
    pl, _ = analyze(lib, n, rowptr, colind)
    assert sorted(pl["perm"]) == list(range(n))
    lam, b = 0.37, rng.normal(size=6 * n)
    x = replay_multifrontal(pl, vals, lam, b)
    np.testing.assert_allclose(x, np.linalg.solve(A + lam * np.eye(6 * n), b), rtol=1e-9, atol=1e-11)


def test_refinement_is_exercised_on_the_small_graphs(lib, monkeypatch):
    """with 4-node leaves the 120-pose graph is dissected many times over: the refined ordering differs from the
    unrefined one there, so the replay test above does check refined separators"""
    monkeypatch.setenv("CUGO_ND_LEAF", "4")
    rowptr, colind = small_pattern("synthetic")
    perms = []
    for refine in ("2", "0"):
        monkeypatch.setenv("CUGO_ND_REFINE", refine)
        perms.append(analyze(lib, len(rowptr) - 1, rowptr, colind)[0]["perm"])
    assert not np.array_equal(perms[0], perms[1])


@pytest.mark.parametrize("name", ["band_loops", "random", "synthetic"])
@pytest.mark.parametrize("leaf", ["4", "8", "24"])
def test_default_keeps_the_better_of_the_two_plans(lib, name, leaf, monkeypatch):
    """the default setting analyses both orderings and keeps the one with the smaller (stages, slots, flops),
    compared in that order; on a tie the unrefined one"""
    monkeypatch.setenv("CUGO_ND_LEAF", leaf)
    rowptr, colind = small_pattern(name)
    cost, perm = {}, {}
    for refine in ("0", "1", "2"):
        monkeypatch.setenv("CUGO_ND_REFINE", refine)
        pl, st = analyze(lib, len(rowptr) - 1, rowptr, colind)
        cost[refine], perm[refine] = (st["stages"], st["slots"], st["chol_flops"]), pl["perm"]
    assert cost["1"] == min(cost["0"], cost["2"])
    assert np.array_equal(perm["1"], perm["2"] if cost["2"] < cost["0"] else perm["0"])


@pytest.fixture(scope="module")
def kitti00_pattern():
    P, L, E, seed, nlc, stereo = SHAPES["kitti00"]
    return covis_pattern_np(cugo.synth(P, L, E, seed=seed, n_loop_closures=nlc, stereo_fraction=stereo))


def test_ordering_is_deterministic(lib, kitti00_pattern, monkeypatch):
    """two analyses, and one thread against the default two threads per dissection, give the same permutation"""
    n, rowptr, colind = kitti00_pattern
    a = analyze(lib, n, rowptr, colind)[0]["perm"]
    b = analyze(lib, n, rowptr, colind)[0]["perm"]
    monkeypatch.setenv("CUGO_ND_PAR", "0")
    c = analyze(lib, n, rowptr, colind)[0]["perm"]
    assert sorted(a) == list(range(n))
    assert np.array_equal(a, b) and np.array_equal(a, c)


def kitti00_stats(monkeypatch, refine):
    if refine is not None:
        monkeypatch.setenv("CUGO_ND_REFINE", refine)
    else:
        monkeypatch.delenv("CUGO_ND_REFINE", raising=False)
    P, L, E, seed, nlc, stereo = SHAPES["kitti00"]
    g = cugo.graph_from_arrays(cugo.synth(P, L, E, seed=seed, n_loop_closures=nlc, stereo_fraction=stereo),
                               plan_only=True)
    g.initialize()
    s = g.structure_stats()
    g.close()
    return s


def test_kitti00_plan_with_the_switch_off_is_the_unrefined_plan(lib, monkeypatch):
    s = kitti00_stats(monkeypatch, "0")
    assert int(s["stages"]) == 17 and int(s["chol_flops"]) == 1626715944


def test_kitti00_plan_by_default_is_shorter(lib, monkeypatch):
    s = kitti00_stats(monkeypatch, None)
    print("kitti00 default plan: stages %d chol_flops %.4e front_bytes %.4e" % (s["stages"], s["chol_flops"], s["front_bytes"]))
    assert int(s["stages"]) <= 16
    assert s["chol_flops"] <= 1.40e9
    assert s["front_bytes"] <= 1.20e8


@pytest.mark.parametrize("shape", ["kitti07", "localba", "synth10k"])
def test_no_shape_gets_a_worse_plan(lib, shape, monkeypatch):
    """stages, potrf slots along the chain and flops: none is larger than in the plan of CUGO_ND_REFINE=0"""
    P, L, E, seed, nlc, stereo = SHAPES[shape]
    n, rowptr, colind = covis_pattern_np(cugo.synth(P, L, E, seed=seed, n_loop_closures=nlc, stereo_fraction=stereo))
    monkeypatch.setenv("CUGO_ND_REFINE", "0")
    _, off = analyze(lib, n, rowptr, colind)
    monkeypatch.delenv("CUGO_ND_REFINE")
    pl, on = analyze(lib, n, rowptr, colind)
    print(shape, "unrefined", off, "default", on)
    assert sorted(pl["perm"]) == list(range(n))
    for key in ("stages", "slots", "chol_flops"):
        assert on[key] <= off[key], key
