"""CPU tests of the selected inverse (marginal covariances): a numpy replay of the top-down pass of
cov_kernels.hip over a host-only solver's plan — Sigma-fronts with the fronts' offsets and leading
dimensions, S_RR read from the parent's Sigma-front through `rel`, copied into the front's own
Sigma-front unless the parent lives in it (alias chains), and the Hsc-pattern blocks gathered through
blk_front / blk_row / blk_col / blk_trans — must reproduce numpy.linalg.inv(A) on the pattern."""
import ctypes as C
import importlib

import numpy as np
import pytest

from test_host import covis_pattern, patterns, plan_arrays, random_spd_bsr, tri_inverse

cugo = importlib.import_module("cuda-bundle-adjustment_amd")


@pytest.fixture(scope="module")
def lib():
    cugo.build()
    return cugo.lib()


def _plan(lib, rowptr, colind):
    s = C.c_void_p()
    assert lib.cugo_chol_create(None, C.byref(s)) == 0
    rc = lib.cugo_chol_analyze(s, len(rowptr) - 1, rowptr.ctypes.data_as(C.POINTER(C.c_int32)),
                               colind.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0, lib.cugo_last_error()
    pl = plan_arrays(lib, s)
    p = C.POINTER(C.c_int32)()
    k = lib.cugo_chol_plan_array(s, b"alias_of", C.byref(p))
    assert k >= 0
    pl["alias_of"] = np.ctypeslib.as_array(p, shape=(k,)).copy() if k else np.zeros(0, np.int32)
    for nm in ("off", "ldf"):  # the storage layout the device uses for the fronts and the Sigma-fronts
        q = C.POINTER(C.c_int64)()
        k = lib.cugo_chol_plan_array64(s, nm.encode(), C.byref(q))
        assert k == len(pl["ncb"]), (nm, lib.cugo_last_error())
        pl[nm] = np.ctypeslib.as_array(q, shape=(k,)).copy() if k else np.zeros(0, np.int64)
    lib.cugo_chol_destroy(s)
    return pl


def _factor(pl, vals, lam, explicit_w=False):
    """per front: L11^-1 (W) and L21, the factorisation the plan describes (extend-add through rel); explicit_w: W by
    forward substitution and L21 = B W^T, as the device forms them (the default goes through numpy's LU)"""
    ns = len(pl["ncb"])
    F = [np.zeros((6 * pl["nb"][f], 6 * pl["nb"][f])) for f in range(ns)]
    for k in range(len(pl["blk_front"])):
        f, rb, cb, tr = pl["blk_front"][k], pl["blk_row"][k], pl["blk_col"][k], pl["blk_trans"][k]
        B = vals[k].reshape(6, 6).T
        if rb == cb:
            F[f][6 * rb:6 * rb + 6, 6 * cb:6 * cb + 6] = np.tril(B) + lam * np.eye(6)
        else:
            F[f][6 * rb:6 * rb + 6, 6 * cb:6 * cb + 6] = B.T if tr else B
    W, L21 = [None] * ns, [None] * ns
    for st in range(len(pl["stage_task_ptr"]) - 1):
        for t in range(pl["stage_task_ptr"][st], pl["stage_task_ptr"][st + 1]):
            for f in pl["task_fronts"][pl["task_ptr"][t]:pl["task_ptr"][t + 1]]:
                for c in pl["child"][pl["child_ptr"][f]:pl["child_ptr"][f + 1]]:
                    ncb = pl["ncb"][c]
                    rel = pl["rel"][pl["rel_ptr"][c]:pl["rel_ptr"][c + 1]]
                    idx = (6 * np.repeat(rel, 6) + np.tile(np.arange(6), len(rel))).astype(int)
                    F[f][np.ix_(idx, idx)] += np.tril(F[c][6 * ncb:, 6 * ncb:])
                nc = 6 * pl["ncb"][f]
                A11 = np.tril(F[f][:nc, :nc])
                A11 = A11 + np.tril(A11, -1).T
                L11 = np.linalg.cholesky(A11)
                if explicit_w:
                    W[f] = tri_inverse(L11)
                    l21 = F[f][nc:, :nc] @ W[f].T
                else:
                    l21 = np.linalg.solve(L11, F[f][nc:, :nc].T).T
                    W[f] = np.linalg.inv(L11)
                L21[f] = l21
                F[f][nc:, nc:] -= l21 @ l21.T
    return W, L21


def replay_selected_inverse(pl, W, L21):
    """the device pass: returns the Sigma blocks on the Hsc pattern ([B][36], column-major)"""
    ns = len(pl["ncb"])
    # the fronts' storage, shared by the Sigma-fronts: the plan's own offsets and leading dimensions
    off, ld = pl["off"], pl["ldf"]
    total = int(max([off[f] + ld[f] * 6 * pl["nb"][f] for f in range(ns)], default=0))
    for f in range(ns):  # (every front inside the buffer, a front stored in its child at the child's update block)
        c = pl["alias_of"][f]
        if c >= 0:
            assert ld[f] == ld[c] and off[f] == off[c] + 6 * pl["ncb"][c] * (ld[c] + 1)
        else:
            assert ld[f] == 6 * pl["nb"][f] + 1
    sig = np.full(total, np.nan)  # a read before a write shows up as NaN

    def at(f, r, c):  # flat index of entry (r, c) of front f's Sigma-front
        return off[f] + c * ld[f] + r

    order = []
    for st in range(len(pl["stage_task_ptr"]) - 1):
        for t in range(pl["stage_task_ptr"][st], pl["stage_task_ptr"][st + 1]):
            order += list(pl["task_fronts"][pl["task_ptr"][t]:pl["task_ptr"][t + 1]])
    for f in reversed(order):
        ncs, nrs = 6 * pl["ncb"][f], 6 * (pl["nb"][f] - pl["ncb"][f])
        S = np.zeros((nrs, nrs))
        if nrs:
            p = pl["sparent"][f]
            rel = pl["rel"][pl["rel_ptr"][f]:pl["rel_ptr"][f + 1]]
            ri = (6 * np.repeat(rel, 6) + np.tile(np.arange(6), len(rel))).astype(int)
            hi, lo = np.maximum.outer(ri, ri), np.minimum.outer(ri, ri)
            S = sig[off[p] + lo * ld[p] + hi]
            assert not np.isnan(S).any()
            if pl["alias_of"][p] != f:  # copy the lower triangle into the own R x R region
                i, k = np.tril_indices(nrs)
                sig[at(f, ncs + i, ncs + k)] = S[i, k]
            else:  # the parent sits there already
                assert off[p] == off[f] + ncs * (ld[f] + 1) and ld[p] == ld[f]
        Srj = -(S @ L21[f]) @ W[f]
        Sjj = W[f].T @ (W[f] - L21[f].T @ Srj)
        r, c = np.meshgrid(np.arange(nrs), np.arange(ncs), indexing="ij")
        sig[at(f, ncs + r, c)] = Srj
        r, c = np.meshgrid(np.arange(ncs), np.arange(ncs), indexing="ij")
        sig[at(f, r, c)] = Sjj
    B = len(pl["blk_front"])
    out = np.zeros((B, 36))
    e = np.arange(36)
    for k in range(B):
        f, tr = pl["blk_front"][k], pl["blk_trans"][k]
        rr, cc = (e % 6, e // 6) if not tr else (e // 6, e % 6)
        ra, ca = 6 * pl["blk_row"][k] + rr, 6 * pl["blk_col"][k] + cc
        out[k] = sig[off[f] + np.minimum(ra, ca) * ld[f] + np.maximum(ra, ca)]
    assert not np.isnan(out).any()
    return out


def _pattern(name):
    if name == "synthetic":
        d = cugo.synth(120, 1500, 6200, seed=3, n_loop_closures=60)
        ep = d["e_pose"].astype(np.int64) - 1
        ep[ep < 0] = 10**6
        return covis_pattern(119, ep, d["e_lm"])
    rows = patterns()[name]
    rowptr = np.array([0] + list(np.cumsum([len(r) for r in rows])), np.int32)
    colind = np.array([c for r in rows for c in r], np.int32)
    return rowptr, colind


ENVS = [{}, {"CUGO_ALIAS_CHAINS": "0"},
        {"CUGO_ND_LEAF": "4", "CUGO_MAX_SUPER_COLS": "3", "CUGO_TARGET_TASKS": "4"},
        {"CUGO_ND_LEAF": "1000", "CUGO_MAX_SUPER_COLS": "1", "CUGO_TARGET_TASKS": "100000"},
        {"CUGO_MIN_SUBTREE_TASKS": "0", "CUGO_ND_LEAF": "8"}]


@pytest.mark.parametrize("name", list(patterns().keys()) + ["synthetic"])
@pytest.mark.parametrize("env", ENVS, ids=["default", "no_alias", "small_fronts", "one_column", "subtree_stage"])
def test_selected_inverse_replay_matches_numpy_inverse(lib, name, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rowptr, colind = _pattern(name)
    n = len(rowptr) - 1
    A, vals = random_spd_bsr(rowptr, colind, np.random.default_rng(11))
    pl = _plan(lib, rowptr, colind)
    lam = 0.0 if name != "band" else 2.5
    W, L21 = _factor(pl, vals, lam)
    got = replay_selected_inverse(pl, W, L21)
    inv = np.linalg.inv(A + lam * np.eye(6 * n))
    scale = np.abs(inv).max()
    for r in range(n):
        for k in range(rowptr[r], rowptr[r + 1]):
            c = colind[k]
            ref = inv[6 * r:6 * r + 6, 6 * c:6 * c + 6]
            np.testing.assert_allclose(got[k].reshape(6, 6).T, ref, rtol=0, atol=1e-10 * scale)


def test_synthetic_pattern_has_alias_chains(lib):
    """the default plan of the synthetic pattern stores fronts in their child's update block, so the in-place
    S_RR of the replay above is exercised"""
    pl = _plan(lib, *_pattern("synthetic"))
    assert (pl["alias_of"] >= 0).any()


def test_selected_inverse_entry_point_is_exported_and_checks_its_solver(lib):
    """the C ABI entry refuses a solver that never factored (here: a host-only one)"""
    rowptr, colind = _pattern("band")
    s = C.c_void_p()
    assert lib.cugo_chol_create(None, C.byref(s)) == 0
    assert lib.cugo_chol_analyze(s, len(rowptr) - 1, rowptr.ctypes.data_as(C.POINTER(C.c_int32)),
                                 colind.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    assert lib.cugo_chol_selected_inverse(s, None) == -3  # CUGO_ERR_INVALID
    assert b"factorisation" in lib.cugo_last_error()
    lib.cugo_chol_destroy(s)
