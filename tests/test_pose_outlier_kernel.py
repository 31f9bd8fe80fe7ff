"""cugo_pose_edges_reject on the device: the outlier pass the four pose edge kinds share (count, scan, place).  Everything
goes through the C entry point and is compared with EXACT equality against the one-line numpy restatement `expected`."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INACTIVE, FIXED_P = cugo.EDGE_INACTIVE, cugo.EDGE_FIXED_P
WG = 256                                  # edges per workgroup and tile (pose_edge_kernels.hip: POSE_WG)
GRID_EDGES = cugo.POSE_REJECT_GRID_EDGES  # one trip of the launcher's grid: its cap of 1024 workgroups x 256 edges
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, GRID_EDGES + WG + 1]
GUARD = 64                                # canary entries in front of and behind the flags


@pytest.fixture(scope="module")
def ctx():
    from devmem import Ctx
    c = Ctx()
    yield c
    c.close()


def expected(chi, thr, flags):
    """the rejected edges, ascending (a NaN compares false: kept)"""
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(((flags & INACTIVE) == 0) & (thr > 0) & (chi > thr)).astype(np.int32)


def run(ctx, chi, thr, flags, n=None):
    """-> (return code, count, the whole list buffer with its canaries, the whole flag buffer with its canaries)"""
    n = len(chi) if n is None else n
    fl = np.concatenate([np.full(GUARD, 0xA5, np.uint8), flags.astype(np.uint8), np.full(GUARD, 0x5A, np.uint8)])
    d_fl = ctx.to_dev(fl)
    d_flags = C.c_void_p(d_fl.value + GUARD)
    d_list = ctx.to_dev(np.full(len(chi) + GUARD, -7, np.int32))
    d_chi, d_thr = ctx.to_dev(np.asarray(chi, np.float64)), ctx.to_dev(np.asarray(thr, np.float64))
    count = C.c_int(-1)
    rc = cugo.lib().cugo_pose_edges_reject(ctx.h, n, d_chi, d_thr, len(thr), d_flags, d_list, C.byref(count))
    return rc, count.value, ctx.to_host(d_list, len(chi) + GUARD, np.int32), ctx.to_host(d_fl, len(fl), np.uint8)


def check(ctx, chi, thr, flags):
    """one call against the restatement: list, count, canaries, flag bytes; then the second call on the flags it left"""
    n = len(chi)
    t_e = np.broadcast_to(thr, (n,)) if len(thr) == 1 else thr
    want = expected(chi, t_e, flags)
    rc, count, lst, fl = run(ctx, chi, thr, flags)
    assert rc == 0, cugo.lib().cugo_last_error().decode()
    assert count == len(want)
    assert np.array_equal(lst[:count], want)
    assert (lst[count:] == -7).all()                               # nothing behind the count is written
    assert (fl[:GUARD] == 0xA5).all() and (fl[GUARD + n:] == 0x5A).all()
    want_flags = flags.copy()
    want_flags[want] |= INACTIVE
    assert np.array_equal(fl[GUARD:GUARD + n], want_flags)         # no other bit, no other byte
    rc2, count2, lst2, fl2 = run(ctx, chi, thr, flags)             # equal inputs: equal bytes
    assert rc2 == 0 and count2 == count and np.array_equal(lst2, lst) and np.array_equal(fl2, fl)
    rc3, count3, lst3, fl3 = run(ctx, chi, thr, want_flags)        # on the flags left behind: nothing more goes
    assert rc3 == 0 and count3 == 0 and (lst3 == -7).all() and np.array_equal(fl3, fl)
    return want


def patterns(n):
    """name -> boolean mask of the edges to reject"""
    idx = np.arange(n)
    out = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "first": idx == 0, "last": idx == n - 1,
           "every_64th": idx % 64 == 0,
           "wave_seams": (idx % 64 == 63) | ((idx % 64 == 0) & (idx > 0)),  # last lane of a wave, first of the next
           "workgroup_seams": (idx % WG == WG - 1) | ((idx % WG == 0) & (idx > 0))}
    if n > GRID_EDGES:  # the seam between the runs of two workgroups that walk two tiles each
        m = np.zeros(n, bool)
        m[[2 * WG - 1, 2 * WG, n - 1]] = True
        out["run_seams"] = m
    return out


@pytest.mark.parametrize("n", SIZES)
def test_designed_patterns_scalar_and_per_edge_thresholds(ctx, n):
    rng = np.random.default_rng(n)
    if n == 0:
        rc, count, lst, fl = run(ctx, np.zeros(0), np.array([1.0]), np.zeros(0, np.uint8))
        assert rc == 0 and count == 0 and (lst == -7).all() and (fl[:GUARD] == 0xA5).all() and (fl[GUARD:] == 0x5A).all()
        return
    for name, mask in patterns(n).items():
        # scalar threshold 2: rejected edges at 3 .. 4, kept ones at 0 .. 1
        chi = np.where(mask, 3.0 + rng.random(n), rng.random(n))
        flags = np.zeros(n, np.uint8)
        want = check(ctx, chi, np.array([2.0]), flags)
        assert np.array_equal(want, np.flatnonzero(mask)), name
        # per-edge thresholds between 1 and 5, chi2 at twice or half of them
        thr = 1.0 + 4.0 * rng.random(n)
        want = check(ctx, np.where(mask, 2.0 * thr, 0.5 * thr), thr, flags)
        assert np.array_equal(want, np.flatnonzero(mask)), name


@pytest.mark.parametrize("n", [65, 257, 1025, GRID_EDGES + WG + 1])
def test_preset_flags_zero_and_negative_thresholds_random_mix(ctx, n):
    rng = np.random.default_rng(100 + n)
    chi = rng.random(n) * 10.0
    # already INACTIVE with chi2 above the threshold: neither listed nor counted; FIXED_P and the other bits survive
    flags = rng.choice(np.array([0, 0, 0, INACTIVE, FIXED_P, FIXED_P | INACTIVE, 0xF7], np.uint8), n)
    want = check(ctx, chi, np.array([5.0]), flags)
    assert len(want) and (flags[want] & INACTIVE == 0).all() and ((flags & INACTIVE != 0) & (chi > 5.0)).any()
    # per-edge array with zeros and negatives (rejection off on those edges) and NaN thresholds
    thr = rng.choice(np.array([0.0, -1.0, -np.inf, np.nan, 2.0, 7.0]), n)
    want = check(ctx, chi, thr, flags)
    assert len(want) and (thr[want] > 0).all()
    # a threshold array of one entry that is 0, negative or NaN: nothing goes
    for t in (0.0, -3.0, np.nan):
        assert len(check(ctx, chi, np.array([t]), flags)) == 0


def test_threshold_edge_values(ctx):
    t = 3.0
    chi = np.array([t, np.nextafter(t, np.inf), np.nan, np.inf, np.nextafter(t, -np.inf), -np.inf, 0.0, -0.0])
    want = check(ctx, chi, np.array([t]), np.zeros(len(chi), np.uint8))
    assert list(want) == [1, 3]  # chi == t kept, the next double goes, NaN kept, +inf goes
    want = check(ctx, chi, np.full(len(chi), t), np.zeros(len(chi), np.uint8))
    assert list(want) == [1, 3]
    # an infinite threshold rejects nothing (chi > inf is never true), the smallest positive one everything positive
    assert len(check(ctx, chi, np.array([np.inf]), np.zeros(len(chi), np.uint8))) == 0
    assert list(check(ctx, chi, np.array([5e-324]), np.zeros(len(chi), np.uint8))) == [0, 1, 3, 4]


def test_refusals_write_nothing(ctx):
    n = 300
    chi, thr, flags = np.full(n, 9.0), np.array([1.0]), np.zeros(n, np.uint8)
    L = cugo.lib()
    d_chi, d_thr, d_fl, d_list = ctx.to_dev(chi), ctx.to_dev(thr), ctx.to_dev(flags), ctx.to_dev(np.full(n, -7, np.int32))
    count = C.c_int(-1)
    f = L.cugo_pose_edges_reject
    assert f(ctx.h, n, None, d_thr, 1, d_fl, d_list, C.byref(count)) == -3
    assert f(ctx.h, n, d_chi, None, 1, d_fl, d_list, C.byref(count)) == -3
    assert f(ctx.h, n, d_chi, d_thr, 1, None, d_list, C.byref(count)) == -3
    assert f(ctx.h, n, d_chi, d_thr, 1, d_fl, None, C.byref(count)) == -3
    assert f(ctx.h, n, d_chi, d_thr, 1, d_fl, d_list, None) == -3
    for bad in (0, 2, n - 1, n + 1, -1):
        assert f(ctx.h, n, d_chi, d_thr, bad, d_fl, d_list, C.byref(count)) == -3, bad
    assert f(ctx.h, (1 << 26) + 1, d_chi, d_thr, 1, d_fl, d_list, C.byref(count)) == -3
    assert "2^26" in L.cugo_last_error().decode()
    assert f(ctx.h, -1, d_chi, d_thr, 1, d_fl, d_list, C.byref(count)) == -3
    assert not ctx.to_host(d_fl, n, np.uint8).any() and (ctx.to_host(d_list, n, np.int32) == -7).all()
    # n == 0 takes null arrays: nothing is launched
    assert f(ctx.h, 0, None, None, 1, None, None, C.byref(count)) == 0 and count.value == 0
    assert cugo.pose_edges_reject(ctx.h, n, d_chi, d_thr, 1, d_fl, d_list) == n  # (the Python wrapper, and the arrays were fine)
    assert np.array_equal(ctx.to_host(d_list, n, np.int32), np.arange(n))


@pytest.mark.parametrize("mode", ["1"])
def test_poisoned_allocations_change_nothing(mode):
    """CUGO_POISON_ALLOC (hip_util.h) in a fresh child process: the workgroup counts live in the context's scratch,
    which then starts as NaN bytes between guard zones"""
    env = dict(os.environ, CUGO_POISON_ALLOC=mode)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p",
                        "no:cacheprovider", "-k", "not poisoned"], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "guard zone" not in r.stderr and " passed" in r.stdout
