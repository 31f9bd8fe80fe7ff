"""GPU tests of the sparse Cholesky and the selected inverse on designed fronts (tests/chol_designed.py): every pivot
width 1..16, boundaries at the edges of the 32- and 64-row tiles, a front of 67 children with a boundary of 65 blocks,
under every factorisation form; x held to the componentwise backward error K_x and the selected inverse to its
per-entry bound, both measured on numpy references (tests/test_chol_designed_host.py), on a strongly diagonally
dominant class and on a clique-Gram class of condition ~1e9.  Then the zero-pivot flag: a non-positive pivot placed at
chosen scalar columns of chosen fronts, a NaN, and power-of-two scalings either side of the pivot tolerance."""
import ctypes as C
import importlib

import numpy as np
import pytest

import chol_designed as cd

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
pytestmark = pytest.mark.gpu
ERR_NUMERIC = -4
PIVOT_TOL = 1e-14  # chol_kernels.hip


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
        self.dx, self.fail, self.dS = ctx.empty(6 * self.n), ctx.empty(2, np.int32), ctx.empty(36 * self.B)

    def solve(self, dH, lam, db):
        """(fail flag, x)"""
        cugo.check(self.lib.cugo_chol_factor_solve(self.s, dH, C.c_double(lam), db, self.dx, self.fail))
        return int(self.ctx.to_host(self.fail, 1, np.int32)[0]), self.ctx.to_host(self.dx, 6 * self.n).copy()

    def selected_inverse(self):
        """(return code, blocks [B, 36])"""
        rc = self.lib.cugo_chol_selected_inverse(self.s, self.dS)
        return rc, self.ctx.to_host(self.dS, 36 * self.B).reshape(self.B, 36).copy()

    def close(self):
        self.lib.cugo_chol_destroy(self.s)


def same_bits(a, b):
    return np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("env", cd.OPTION_SETS, ids=cd.option_id)
@pytest.mark.parametrize("name", cd.NAMES)
def test_designed_fronts_in_every_form(ctx, name, env, monkeypatch):
    """one analysis, both value classes, lambda = 0 and 2.5: no flag, omega(x) <= K_x; on widths and fan every block of
    the selected inverse inside its bound; a second call of each gives the same bits"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rowptr, colind, _ = cd.design(name)
    sv = Solver(ctx, rowptr, colind)
    with_inverse = name in ("widths", "fan")
    mask = cd.block_mask(rowptr, colind) if with_inverse else None
    worst_w = worst_r = 0.0
    for cls in cd.CLASSES:
        A, vals, b = cd.values(name, cls)
        dH, db = ctx.to_dev(vals), ctx.to_dev(b)
        for lam in cd.LAMBDAS:
            fail, x = sv.solve(dH, lam, db)
            assert fail == 0, (name, cls, lam)
            w = cd.case_omega(name, cls, lam, x)
            worst_w = max(worst_w, w)
            print("%s [%s] %s lambda %.1f: omega %.2f u" % (name, cd.option_id(env), cls, lam, w))
            assert w <= cd.K_X, (name, cls, lam, w)
            if with_inverse:
                rc, S = sv.selected_inverse()
                assert rc == 0, (name, cls, lam)
                _, X1, scale = cd.inverse_reference(name, cls, lam)
                r = cd.sinv_ratio(cd.blocks_to_dense(S, rowptr, colind), X1, scale, mask)
                bound = cd.k_s_case(name, cls, lam)
                worst_r = max(worst_r, r / bound)
                print("%s [%s] %s lambda %.1f: selected inverse ratio %.3g (bound %.3g)"
                      % (name, cd.option_id(env), cls, lam, r, bound))
                assert r <= cd.K_S and r <= bound, (name, cls, lam, r)
                rc, S2 = sv.selected_inverse()
                assert rc == 0 and same_bits(S, S2), (name, cls, lam)
            fail, x2 = sv.solve(dH, lam, db)
            assert fail == 0 and same_bits(x, x2), (name, cls, lam)
    print("MAX %s [%s]: omega %.2f u, selected inverse %.3f of its bound" % (name, cd.option_id(env), worst_w, worst_r))
    sv.close()


# ------------------------------------------------------------------ the zero-pivot flag -----------
PIVOT_ENVS = [{}, {"CUGO_PANEL16": "0"}, {"CUGO_MIN_SUBTREE_TASKS": "0"}]


def pivot_places(pl):
    """(front, scalar column) of the placed pivots on `widths`: columns 0, 15, 16, 63, 64, 95 of the 96-wide front (the
    edges of the 16-column panels and of the first wave's 64), the last column of a 6-wide front, column 29 of the
    30-wide one (the last before the padding), and one in the root"""
    f96, f6, f30 = cd.front_of(pl, 16, 11), cd.front_of(pl, 1, 11), cd.front_of(pl, 5, 11)
    root = int(np.flatnonzero(pl["sparent"] == -1)[-1])
    return [(f96, c) for c in (0, 15, 16, 63, 64, 95)] + [(f6, 5), (f30, 29), (root, 3 * pl["ncb"][root] + 1)]


def with_pivot_at(A, vals, rowptr, Lp, sidx, j):
    """vals with 1.5 L_jj^2 taken off the diagonal entry of permuted scalar column j: pivot j becomes -L_jj^2 / 2, the
    first non-positive one; the pivots before it are untouched"""
    i = int(sidx[j])
    out = vals.copy()
    out[rowptr[i // 6], 7 * (i % 6)] -= 1.5 * Lp[j, j] ** 2
    return out


@pytest.mark.parametrize("env", PIVOT_ENVS, ids=cd.option_id)
def test_flag_for_a_pivot_placed_anywhere_in_a_front(ctx, env, monkeypatch):
    """each placed pivot raises fail == 1 and makes the selected inverse refuse; a good factorisation straight after,
    on the same solver, clears the flag, gives the bits it gave before and lets the selected inverse succeed with its
    own earlier bits; a NaN in one off-diagonal Hsc entry raises the flag too"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rowptr, colind, _ = cd.design("widths")
    A, vals, b = cd.values("widths", "dd")
    sv = Solver(ctx, rowptr, colind)
    pl = cd.plan(sv.lib, sv.s)
    sidx = cd.scalar_perm(pl)
    Lp = np.linalg.cholesky(A[np.ix_(sidx, sidx)])
    dH, db = ctx.to_dev(vals), ctx.to_dev(b)
    fail, x0 = sv.solve(dH, 0.0, db)
    rc, S0 = sv.selected_inverse()
    assert fail == 0 and rc == 0
    bad = [with_pivot_at(A, vals, rowptr, Lp, sidx, 6 * pl["col0"][f] + c) for f, c in pivot_places(pl)]
    nan = vals.copy()
    mid = len(rowptr) // 2
    assert rowptr[mid + 1] - rowptr[mid] >= 2
    nan[rowptr[mid] + 1, 8] = np.nan   # (the first off-diagonal block of a row in the middle)
    for k, v in enumerate(bad + [nan]):
        fail, _ = sv.solve(ctx.to_dev(v), 0.0, db)
        assert fail == 1, (k, pivot_places(pl)[k] if k < len(bad) else "nan")
        assert sv.lib.cugo_chol_selected_inverse(sv.s, sv.dS) == ERR_NUMERIC, k
        fail, x = sv.solve(dH, 0.0, db)
        assert fail == 0 and same_bits(x, x0), k
        rc, S = sv.selected_inverse()
        assert rc == 0 and same_bits(S, S0), k
    sv.close()


@pytest.mark.parametrize("env", PIVOT_ENVS, ids=cd.option_id)
def test_pivot_tolerance_under_power_of_two_scaling(ctx, env, monkeypatch):
    """D A D with D = 2^-k I (exact, so the reference stays exact): smallest pivot ~1e-12, above PIVOT_TOL = 1e-14 — no
    flag and omega <= K_x; ~1e-15, below it — the flag"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rowptr, colind, _ = cd.design("widths")
    A, vals, b = cd.values("widths", "dd")
    sv = Solver(ctx, rowptr, colind)
    sidx = cd.scalar_perm(cd.plan(sv.lib, sv.s))
    dmin = float(np.min(np.diag(np.linalg.cholesky(A[np.ix_(sidx, sidx)])) ** 2))
    db = ctx.to_dev(b)
    for target, want in ((1e-12, 0), (1e-15, 1)):
        k = int(round(np.log2(dmin / target) / 2))
        sc = 4.0 ** -k
        assert 0.4 * target < dmin * sc < 2.5 * target and (dmin * sc > 40 * PIVOT_TOL) == (want == 0)
        fail, x = sv.solve(ctx.to_dev(vals * sc), 0.0, db)
        assert fail == want, (target, dmin * sc)
        if want == 0:
            w = cd.omega(A * sc, 0.0, b, x)
            print("smallest pivot %.2e [%s]: omega %.2f u" % (dmin * sc, cd.option_id(env), w))
            assert w <= cd.K_X, w
    sv.close()
