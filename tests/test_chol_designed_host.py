"""CPU tests of the designed Cholesky cases (tests/chol_designed.py): the plans really hold the fronts the designs are
there for, under every factorisation form tests/test_chol_shapes.py runs; the references stay inside the bounds K_x /
K_s the device is held to; and the metric notices a mistake at each of the edges — five deliberate ones in the numpy
replay break K_x by a stated factor."""
import importlib

import numpy as np
import pytest

import chol_designed as cd
from test_host import replay_multifrontal

cugo = importlib.import_module("cuda-bundle-adjustment_amd")


@pytest.fixture(scope="module")
def lib():
    cugo.build()
    return cugo.lib()


def host_plan(lib, name):
    rowptr, colind, _ = cd.design(name)
    s = cd.analyze(lib, rowptr, colind)
    pl = cd.plan(lib, s)
    lib.cugo_chol_destroy(s)
    return pl


@pytest.fixture(scope="module")
def default_plans(lib):
    return {name: host_plan(lib, name) for name in cd.NAMES}


# ------------------------------------------------------------------ census -----------
@pytest.mark.parametrize("env", cd.OPTION_SETS, ids=cd.option_id)
def test_designs_hold_the_fronts_they_are_there_for(lib, env, monkeypatch):
    """under the defaults and under every option set of the GPU file: every leaf (c, r) of every design is a front
    with ncb = c and nb - ncb = r, and the union of the designs has every pivot width 1..16, the boundaries at the tile
    edges, a front of >= 65 children, a child whose boundary passes 64 blocks, a boundary of >= 3 backward-chain
    segments one of which is exactly 16 rows, and stages of both tile edges (unless the option forces one)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cs = {}
    for name in cd.NAMES:
        c = cs[name] = cd.census(host_plan(lib, name))
        missing = [leaf for leaf in set(cd.DESIGNS[name][1]) if leaf not in c["pairs"]]
        assert not missing, (name, missing)
    ncb = set().union(*[c["ncb"] for c in cs.values()])
    bnd = set().union(*[c["bnd"] for c in cs.values()])
    assert set(range(1, 17)) <= ncb
    assert {0, 1, 5, 6, 10, 11, 16, 21, 22, 32, 33, 65} <= bnd
    assert {(c, r) for c in cd.TILES_C for r in cd.TILES_R} <= cs["tiles"]["pairs"]
    assert cs["fan"]["max_children"] >= 65 and cs["fan"]["max_child_bnd"] > 64
    assert cs["tiles"]["seg3_with_16"] >= 1
    tiles = set().union(*[c["tiles"] for c in cs.values()])
    t32 = env.get("CUGO_TILE32_MAX_TILES")
    if t32 is None:
        assert {32, 64} <= tiles, tiles
    else:  # (the option forces one edge on every stage: the two sets of the GPU file cover both between them)
        assert (64 if t32 == "0" else 32) in tiles and (32 if t32 == "0" else 64) not in tiles, tiles
    assert (0 in tiles) == (env.get("CUGO_TWO_PHASE_MIN_TILES") == "1"), tiles


# ------------------------------------------------------------------ references inside their bounds -----------
@pytest.mark.parametrize("cls", cd.CLASSES)
@pytest.mark.parametrize("name", cd.NAMES)
def test_replay_stays_inside_k_x(default_plans, name, cls):
    """K_x is 4 x the largest omega of the replay (W = L11^-1 formed, as on the device): here is where it is measured"""
    A, vals, b = cd.values(name, cls)
    for lam in cd.LAMBDAS:
        x = replay_multifrontal(default_plans[name], vals, lam, b, explicit_w=True)
        w = cd.case_omega(name, cls, lam, x)
        print("%s %s lambda %.1f: omega(replay) = %.2f u" % (name, cls, lam, w))
        assert w <= cd.K_X, (name, cls, lam, w)


@pytest.mark.parametrize("cls", cd.CLASSES)
@pytest.mark.parametrize("name", ["widths", "fan"])
def test_inverses_stay_inside_k_s(lib, name, cls):
    """numpy's unrefined float64 inverse against the refined one, per entry in units of u (|A^-1| |L| |L^T| |A^-1|):
    K_S is 4 x its largest ratio.  numpy inverts through LU, which is not stable row by row: on (widths, gram, 0) its
    ratio is 8.4e5, and K_S with it.  The numpy replay of the device's own pass (test_covariance_host, W formed
    explicitly) gives the per-case bound that bites, chol_designed.k_s_case."""
    import test_covariance_host as tch
    rowptr, colind, _ = cd.design(name)
    pl = tch._plan(lib, rowptr, colind)
    A, vals, _ = cd.values(name, cls)
    mask = cd.block_mask(rowptr, colind)
    for lam in cd.LAMBDAS:
        X0, X1, scale = cd.inverse_reference(name, cls, lam)
        r0 = cd.sinv_ratio(X0, X1, scale)
        W, L21 = tch._factor(pl, vals, lam, explicit_w=True)
        got = cd.blocks_to_dense(tch.replay_selected_inverse(pl, W, L21), rowptr, colind)
        r1 = cd.sinv_ratio(got, X1, scale, mask)
        print("%s %s lambda %.1f: ratio numpy inv %.3g, replay of the device pass %.3g" % (name, cls, lam, r0, r1))
        assert r0 <= cd.K_S, (name, cls, lam, r0)
        assert r1 <= cd.k_s_case(name, cls, lam), (name, cls, lam, r1)


# ------------------------------------------------------------------ the metric bites -----------
def fan_front(pl):
    f = int(np.argmax(np.diff(pl["child_ptr"])))
    assert pl["child_ptr"][f + 1] - pl["child_ptr"][f] >= 65
    return f


def mutation(pl_by_name, which):
    """(design, mutate tuple of replay_multifrontal, factor by which omega must pass K_x on BOTH value classes)"""
    if which == "rhs_row_of_boundary_32":   # (a) the lone row of the fourth 64-row tile: nt = 193 = 3 * 64 + 1
        pl = pl_by_name["tiles"]
        return "tiles", ("skip_rhs_update", cd.front_of(pl, 8, 32)), 1e5
    if which == "child_33_of_the_fan":      # (b) the first child of the second EA_BATCH
        pl = pl_by_name["fan"]
        return "fan", ("drop_child", fan_front(pl), 32), 1e5
    if which == "rel_64_off_by_one":        # (c) the first entry of the second 64-lane stride
        pl = pl_by_name["fan"]
        c = cd.front_of(pl, 3, 65)
        rel = pl["rel"][pl["rel_ptr"][c]:pl["rel_ptr"][c + 1]]
        d = 1 if rel[64] + 1 < pl["nb"][pl["sparent"][c]] else -1
        return "fan", ("rel_shift", c, 64, d), 1e5
    if which == "padding_column_leaks":     # (d) ncb = 5: 30 columns padded to 32
        # (the 1.0 sits in column 6 ncb of the panel [L11; L21] where the update's sum over k reads it: in the padding
        # of L11 alone it could not reach a result — W stays triangular and the padding of B is zero)
        pl = pl_by_name["widths"]
        return "widths", ("pad_leak", cd.front_of(pl, 5, 11)), 1e5
    if which == "rsqrt_short_of_a_newton_step":  # (e) expected: omega ~ 2e-12 / u ~ 1e4 u
        return "widths", ("rsqrt_err", 1e-12), 50.0
    raise KeyError(which)


MUTATIONS = ["rhs_row_of_boundary_32", "child_33_of_the_fan", "rel_64_off_by_one", "padding_column_leaks",
             "rsqrt_short_of_a_newton_step"]


@pytest.mark.parametrize("which", MUTATIONS)
def test_omega_notices_a_mistake_at_each_edge(default_plans, which):
    """one wrong index or one lost Newton step in the replay, at the places the designs are built around: omega passes
    K_x by the stated factor on both value classes — the structural ones by >= 1e5 (measured: 1e6 .. 1e13 x K_x, or a
    front left indefinite), the 1e-12 error of d^-1/2 by >= 50 (measured: 120 and 291 x K_x, omega = 3.7e3 and 8.8e3 u,
    where rtol = 1e-9 sees nothing)"""
    name, mut, factor = mutation(default_plans, which)
    for cls in cd.CLASSES:
        A, vals, b = cd.values(name, cls)
        try:
            x = replay_multifrontal(default_plans[name], vals, 0.0, b, explicit_w=True, mutate=mut)
            w = cd.case_omega(name, cls, 0.0, x)
        except np.linalg.LinAlgError:  # (the mistake left a front indefinite: the device raises its flag there)
            w = np.inf
        print("%s on %s %s: omega = %.3g u = %.3g K_x" % (which, name, cls, w, w / cd.K_X))
        assert w >= factor * cd.K_X, (which, cls, w)
    if which == "rsqrt_short_of_a_newton_step":  # the check this metric replaces does not see it
        A, vals, b = cd.values(name, "dd")
        x = replay_multifrontal(default_plans[name], vals, 0.0, b, explicit_w=True, mutate=mut)
        np.testing.assert_allclose(x, np.linalg.solve(A, b), rtol=1e-9, atol=1e-12)
