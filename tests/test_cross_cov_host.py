"""CPU tests of the blocks of the inverse off the pattern (cugo_chol_inverse_blocks): the path lemma the kernels rest
on, over host-only solvers' plans; the numpy replay of the two device passes (tests/cross_cov_ref.py) against its
per-entry bound, where the constants of that bound are measured; deliberate mistakes that must break the bound; and the
refusals of the C ABI entry point."""
import ctypes as C
import importlib

import numpy as np
import pytest

import chol_designed as cd
import cross_cov_ref as xr
from test_host import covis_pattern, patterns

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
I32P = C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def lib():
    cugo.build()
    return cugo.lib()


def synthetic_pattern():
    d = cugo.synth(160, 2500, 10500, seed=3, n_loop_closures=80)
    ep = d["e_pose"].astype(np.int64) - 1
    ep[ep < 0] = 10**6
    return covis_pattern(159, ep, d["e_lm"])


def all_patterns():
    out = {}
    for name, rows in patterns().items():
        out[name] = cd.csr(rows)
    out["synthetic"] = synthetic_pattern()
    for name in cd.NAMES:
        out[name] = cd.design(name)[:2]
    return out


# the option sets of chol_designed.OPTION_SETS that change the plan (tile edge, two-phase and look-ahead schedules,
# subtree stage, alias chains; the others only choose kernels), and the orderings / supernode widths of
# test_covariance_host.ENVS
PLAN_ENVS = [e for e in cd.OPTION_SETS
             if not set(e) & {"CUGO_PANEL16", "CUGO_ASM_FRONTS", "CUGO_BW_CHAIN", "CUGO_EA_LDS", "CUGO_EA_DIRECT"}] + [
    {"CUGO_ND_LEAF": "4", "CUGO_MAX_SUPER_COLS": "3", "CUGO_TARGET_TASKS": "4"},
    {"CUGO_ND_LEAF": "1000", "CUGO_MAX_SUPER_COLS": "1", "CUGO_TARGET_TASKS": "100000"},
    {"CUGO_MIN_SUBTREE_TASKS": "0", "CUGO_ND_LEAF": "8"}]


@pytest.mark.parametrize("env", PLAN_ENVS, ids=cd.option_id)
def test_boundary_rows_are_pivot_columns_of_ancestors(lib, env, monkeypatch):
    """the lemma: Y_v = L^-1 E_v lives on the pivot columns of the fronts between v's front and the root, because every
    boundary row of a front is a pivot column of one of its ancestors"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for name, (rowptr, colind) in all_patterns().items():
        pl = xr.host_plan(lib, rowptr, colind)
        assert len(pl["perm"]) == len(rowptr) - 1
        assert not xr.lemma_violations(pl), (name, xr.lemma_violations(pl)[:5])
        # (and what the walk indexes with: col_front covers every column, the paths end at a root)
        assert (pl["col_front"] >= 0).all() and (pl["sparent"] < len(pl["ncb"])).all()
        assert np.array_equal(pl["perm"][pl["iperm"]], np.arange(len(pl["perm"])))


@pytest.fixture(scope="module")
def design_plans(lib):
    return {name: xr.host_plan(lib, *cd.design(name)[:2]) for name in cd.NAMES}


def replay_ratio(pl, name, cls, lam, mutate=None):
    rowptr, colind, _ = cd.design(name)
    A, vals, b = cd.values(name, cls)
    rows, cols = xr.design_pairs(name, pl)
    _, X1, scale = cd.inverse_reference(name, cls, lam)
    got = xr.inverse_blocks(pl, xr.factor(pl, vals, lam, b), rows, cols, mutate)
    X, mask = xr.pairs_to_dense(got, rows, cols, len(rowptr) - 1)
    return cd.sinv_ratio(X, X1, scale, mask)


@pytest.mark.parametrize("cls", cd.CLASSES)
@pytest.mark.parametrize("name", cd.NAMES)
def test_replay_stays_inside_its_bound(design_plans, name, cls):
    """here the constants cross_cov_ref.XCOV_REPLAY are measured: the replay of the device's two passes against the
    refined inverse, per entry in units of u (|A^-1| |L| |L^T| |A^-1|)_ab, over the pairs the device is asked for"""
    for lam in cd.LAMBDAS:
        r = replay_ratio(design_plans[name], name, cls, lam)
        print("%s %s lambda %.1f: ratio of the replay %.3g (recorded %.3g, bound for the device %.3g)"
              % (name, cls, lam, r, xr.XCOV_REPLAY[(name, cls, lam)], xr.k_xcov_case(name, cls, lam)))
        assert r <= xr.k_xcov_case(name, cls, lam), (name, cls, lam, r)


def test_special_rows_of_the_designs(design_plans):
    """the pairs picked from the plan exist where the designs are meant to supply them"""
    assert {"one_front", "root_leaf"} <= set(xr.special_rows(design_plans["tiles"]))
    assert "meet_at_root" in xr.special_rows(design_plans["widths"])
    assert "aliased" in xr.special_rows(design_plans["fan"])
    for name in cd.NAMES:  # every front of the designs keeps a compact L21 (the layout "ld_nrs" is about)
        assert (design_plans[name]["l21off"] >= 0).all()


@pytest.mark.parametrize("mutate", ["ld_nrs", "stop_short", "no_iperm", "transposed", "first_front"])
def test_deliberate_mistakes_break_the_bound(design_plans, mutate):
    """each mistake a kernel could make puts the replay far outside the bound the device is held to (all pairs of
    `widths`, 20 of them with a > b)"""
    name, cls, lam = "widths", "dd", 0.0
    r = replay_ratio(design_plans[name], name, cls, lam, mutate)
    print("%s: ratio %.3g (bound %.3g)" % (mutate, r, xr.k_xcov_case(name, cls, lam)))
    assert r > 1e6 * xr.k_xcov_case(name, cls, lam), (mutate, r)


def test_inverse_blocks_entry_point_is_exported_and_refuses(lib):
    """a host-only solver never factored: CUGO_ERR_INVALID, as for an index equal to n and a negative count"""
    rowptr, colind = cd.csr(patterns()["band"])
    n = len(rowptr) - 1
    s = cd.analyze(lib, rowptr, colind, None)
    ok, bad = np.array([0], np.int32), np.array([n], np.int32)
    p = lambda a: a.ctypes.data_as(I32P)
    assert lib.cugo_chol_inverse_blocks(s, 1, p(ok), p(ok), None) == -3
    assert b"factorisation" in lib.cugo_last_error()
    assert lib.cugo_chol_inverse_blocks(s, 1, p(ok), p(bad), None) == -3
    assert b"outside" in lib.cugo_last_error()
    assert lib.cugo_chol_inverse_blocks(s, 1, p(bad), p(ok), None) == -3
    assert lib.cugo_chol_inverse_blocks(s, -1, p(ok), p(ok), None) == -3
    assert b"negative" in lib.cugo_last_error()
    lib.cugo_chol_destroy(s)


def test_plan_only_graph_refuses_cross_covariances(lib):
    """a plan-only graph has no device: the graph-level calls are refused as compute_covariances() is"""
    d = cugo.synth(12, 150, 600, seed=2)
    g = cugo.graph_from_arrays(d, plan_only=True)
    g.initialize()
    with pytest.raises(cugo.CugoError, match="plan-only"):
        g.pose_cross_covariances([1], [2])
    with pytest.raises(cugo.CugoError, match="plan-only"):
        g.relative_pose_covariances([1], [2])
    g.close()
