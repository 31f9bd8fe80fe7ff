"""GPU tests of the pose-landmark covariance kernels (k_pose_lm_cross and k_reprojection_cov of cov_kernels.hip) through
cugo_pose_landmark_cross_covariances and cugo_reprojection_covariances, on the designs of tests/lm_cov_designed.py
against the longdouble reference and the per-entry bounds of tests/pl_cov_ref.py (tests/test_pl_cov_host.py measures
their constants and shows that the bound sees a dropped edge, a transposed block, the sign, L^-1 on the wrong side and
a read of a slot that does not count).

The pose covariance is numpy's inverse of the float64 Schur complement (data, fed to both sides).  The block list is the
plan's (cugo_plcov_plan_*), shuffled; every block that no counted slot of a query refers to is NaN on the device, and so
is the Hpl block of every slot that does not count.  The output is NaN before the call with 18 spare doubles behind it,
the flag holds 7 before the call.
"""
import ctypes as C
import importlib

import numpy as np
import pytest

import kernel_ref as kr
import lm_cov_designed as ld
import lm_cov_ref as lr
import pl_cov_ref as pr

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
pytestmark = pytest.mark.gpu
ERR_INVALID = -3


@pytest.fixture(scope="module")
def ctx():
    import devmem
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    c = devmem.Ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(name):
        if name not in cache:
            des = ld.design(name)
            Sigma = pr.dense_sigma(des, ld.B_PRIOR if name.startswith("B") else 0.0)
            qp, ql = pr.queries(des)
            cache[name] = (des, Sigma, qp, ql, pr.reference(des, Sigma, qp, ql))
        return cache[name]
    return get


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


class Case:
    """the queries (qp, ql) of one design on the device"""

    def __init__(self, ctx, des, Sigma, qp, ql, seed=3):
        import devmem
        self.ctx, self.lib = ctx, cugo.lib()
        f = self.f = des["f"]
        P = f["P"]
        self.n = n = len(qp)
        plan = cugo.PlCovPlan(P, f["lm_ptr"], f["pose"], qp, ql)
        rows, cols, q_ptr, q_slot, self.q_aa = (plan.array(k) for k in ("rows", "cols", "q_ptr", "q_slot", "q_aa"))
        plan.close()
        # the block list shuffled: block k of the plan sits at place[k]
        B = len(rows)
        place = np.random.default_rng(seed).permutation(B)
        blocks = np.full((B, 36), np.nan)
        counted = np.zeros(B, bool)
        for k in range(n):
            if qp[k] < 0 or ql[k] < 0:
                continue
            l = int(ql[k])
            fl = f["flags"][f["lm_ptr"][l]:f["lm_ptr"][l + 1]]
            sl = q_slot[q_ptr[k]:q_ptr[k + 1]]
            assert len(sl) == len(fl)
            counted[sl[(fl & lr.SKIP) == 0]] = True
        for k in np.flatnonzero(counted):
            a, b = int(rows[k]), int(cols[k])
            blocks[place[k]] = kr.colmajor(Sigma[None, 6 * a:6 * a + 6, 6 * b:6 * b + 6])[0]
        self.n_nan = int((~counted).sum())
        self.place = place
        self.ev = devmem.upload_edges(ctx, f)
        self.d_qp, self.d_ql = ctx.to_dev(np.asarray(qp, np.int32)), ctx.to_dev(np.asarray(ql, np.int32))
        self.d_ptr = ctx.to_dev(q_ptr)
        self.d_slot = ctx.to_dev(np.where(q_slot >= 0, place[np.maximum(q_slot, 0)], -1).astype(np.int32))
        self.dHll = ctx.to_dev(kr.colmajor(des["Hll"]))
        assert np.all(np.isnan(des["Hpl"][(f["flags"] & lr.SKIP) != 0]))
        self.dHpl = ctx.to_dev(kr.colmajor(des["Hpl"]))
        self.dblocks = ctx.to_dev(blocks)
        self.dout = ctx.to_dev(np.full(18 * n + 18, np.nan))
        self.dfail = ctx.to_dev(np.array([7, 7], np.int32))

    def args(self):
        return [self.ctx.h, C.byref(self.ev), self.n, self.d_qp, self.d_ql, self.d_ptr, self.d_slot, self.dHll, self.dHpl,
                self.dblocks, self.dout, self.dfail]

    def run(self, dHll=None):
        """(cov [n,6,3], the 18 doubles behind it, flag) of one call on a NaN-filled output and a flag of 7"""
        nan, seven = np.full(18 * self.n + 18, np.nan), np.array([7, 7], np.int32)
        cugo.check(self.lib.cugo_memcpy_h2d(self.ctx.h, self.dout, nan.ctypes.data_as(C.c_void_p), nan.nbytes))
        cugo.check(self.lib.cugo_memcpy_h2d(self.ctx.h, self.dfail, seven.ctypes.data_as(C.c_void_p), seven.nbytes))
        a = self.args()
        if dHll is not None:
            a[7] = dHll
        cugo.check(self.lib.cugo_pose_landmark_cross_covariances(*a))
        out = self.ctx.to_host(self.dout, 18 * self.n + 18)
        flag = self.ctx.to_host(self.dfail, 2, np.int32)
        assert flag[1] == 7
        return (kr.from_colmajor(out[:18 * self.n].reshape(self.n, 18), 6, 3).copy(), out[18 * self.n:].copy(), int(flag[0]))


def check_blocks(name, got, ref, what=""):
    """every entry of every query that the reference does not fail inside its bound; failed queries 18 zeros, and so
    the queries on a landmark without a counted slot (nothing is summed); a marginal landmark either; returns the
    queries whose block is zero"""
    r = pr.ratios(got, ref, pr.bound(ref))
    zero = [k for k in range(len(got)) if not got[k].any()]
    sure = ~ref["marginal"]
    print("%s%s: %d queries, worst ratio to the bound %.3g (fp64 replay: %.3g of the same bound), %d zero blocks"
          % (name, what, len(got), r.max() if len(r) else 0.0, pr.REPLAY.get(name, np.nan) / pr.K_PL, len(zero)))
    assert np.all(np.isfinite(got)), name
    assert len(r) == 0 or r.max() <= 1, (name, int(r.argmax()), float(r.max()))
    empty = ref["fail"] | (ref["deg"] == 0)
    assert set(zero) - set(np.flatnonzero(~sure).tolist()) == set(np.flatnonzero(empty & sure).tolist()), (name, zero)
    return zero


def expected_flag(ref, zero):
    return int(bool(ref["fail"].any()) or any(ref["marginal"][k] for k in zero))


# ------------------------------------------------------------------ every design ---------
@pytest.mark.parametrize("name", ("B", "B_padded", "mixed", "corners", "far"))
def test_blocks_within_bound_repeatable(ctx, cases, name):
    """every entry of every block within K_PL (n + C_PL) u sqrt(cond Hll) mass of the reference; the same bits on a
    second call; the 18 doubles behind the output untouched; the flag 0 on a design without a degenerate landmark"""
    des, Sigma, qp, ql, ref = cases(name)
    case = Case(ctx, des, Sigma, qp, ql)
    if name in ("B", "B_padded", "mixed"):   # (in corners and far every listed block is one that a counted slot reads)
        assert case.n_nan > 0, "no block is NaN: the design does not show a read of a block that must not be read"
    got, tail, flag = case.run()
    zero = check_blocks(name, got, ref)
    assert np.all(np.isnan(tail)), (name, tail)
    assert flag == expected_flag(ref, zero), (name, flag)
    if not name.startswith("B"):
        assert flag == 0 and zero == np.flatnonzero(ref["deg"] == 0).tolist()
    again, tail2, flag2 = case.run()
    assert same_bits(got, again) and np.all(np.isnan(tail2)) and flag2 == flag, name


def test_layout_B_edgeless_landmarks_fail_and_leave_the_rest(ctx, cases):
    """B and its padded form: flag 1, 18 zeros for exactly the queries on the free landmarks without an edge (and
    possibly on the marginal one that a single mono edge sees), every other query within bound; padding changes no bit"""
    got = {}
    for name in ("B", "B_padded"):
        des, Sigma, qp, ql, ref = cases(name)
        f = des["f"]
        edgeless = [l for l in range(f["L"]) if not ((f["flags"][f["lm_ptr"][l]:f["lm_ptr"][l + 1]] & 8) == 0).any()]
        assert len(edgeless) == 5
        on_edgeless = set(np.flatnonzero(np.isin(ql, edgeless)).tolist())
        assert on_edgeless == set(np.flatnonzero(ref["fail"]).tolist())
        got[name], _, flag = Case(ctx, des, Sigma, qp, ql).run()
        zero = check_blocks(name, got[name], ref, " (edgeless landmarks)")
        assert flag == 1
        assert on_edgeless <= set(zero) and all(ref["marginal"][k] for k in set(zero) - on_edgeless), zero
    assert same_bits(got["B"], got["B_padded"])


@pytest.mark.parametrize("n", (0, 1, 255, 256, 257, 513))
def test_query_counts_at_the_edges_of_the_grid(ctx, cases, n):
    """the first n queries of grid513: the edges of a 256-thread grid.  n = 0: CUGO_OK, nothing written, flag untouched"""
    des, Sigma, qp, ql, ref = cases("grid513")
    sub = {k: v[:n] for k, v in ref.items()}
    case = Case(ctx, des, Sigma, qp[:n], ql[:n])
    got, tail, flag = case.run()
    assert np.all(np.isnan(tail))
    if n == 0:
        assert flag == 7
        return
    zero = check_blocks("grid513[:%d]" % n, got, sub)
    assert flag == 0 and not zero
    again, _, _ = case.run()
    assert same_bits(got, again)


def test_fixed_vertices_and_a_failing_landmark_on_mixed(ctx, cases):
    """queries with a fixed pose, a fixed landmark or both give 18 zeros and raise no flag, the others keep their bits.
    One landmark's Hll replaced by a matrix with a negative second pivot, then by one with a NaN: the flag is 1, the
    queries on that landmark are 18 zeros (under a fixed pose too), every other query keeps the bits of the clean run"""
    des, Sigma, qp, ql, ref = cases("mixed")
    clean, _, flag = Case(ctx, des, Sigma, qp, ql).run()
    assert flag == 0
    n = len(qp)
    qp2, ql2 = qp.copy(), ql.copy()
    qp2[0::5] = -1
    ql2[1::5] = -1
    qp2[2::5], ql2[2::5] = -1, -1
    fixed = (qp2 < 0) | (ql2 < 0)
    case = Case(ctx, des, Sigma, qp2, ql2, seed=4)   # (another shuffle of another block list: the bits must not care)
    got, tail, flag = case.run()
    assert flag == 0 and np.all(np.isnan(tail))
    assert not got[fixed].any() and not np.isnan(got[fixed]).any()
    assert same_bits(got[~fixed], clean[~fixed])
    # a landmark of degree >= 3 that is queried under a free pose and under a fixed one
    cand = [int(l) for l in np.unique(ql2[~fixed & (ref["deg"] >= 3)]) if ((ql2 == l) & (qp2 < 0)).any()]
    assert len(cand) >= 8
    lt = cand[len(cand) // 2]
    on_lt = (ql2 == lt)
    assert (on_lt & (qp2 < 0)).any() and (on_lt & ~fixed).any()
    Lf = lr.chol3(np.asarray(des["Hll"][lt], kr.LD), kr.LD)
    H1 = des["Hll"].copy()
    H1[lt, 1, 1] -= float(1.5 * Lf[1, 1] ** 2)
    H2 = des["Hll"].copy()
    H2[lt, 2, 1] = H2[lt, 1, 2] = np.nan
    for what, H in (("pivot 1", H1), ("NaN", H2)):
        bad, tail, flag = case.run(ctx.to_dev(kr.colmajor(H)))
        assert flag == 1, what
        assert not bad[on_lt].any() and not np.isnan(bad[on_lt]).any(), what
        assert same_bits(bad[~on_lt], got[~on_lt]) and np.all(np.isnan(tail)), what
        back, _, flag = case.run()
        assert flag == 0 and same_bits(back, got), what


def test_refusals(ctx, cases):
    """CUGO_ERR_INVALID for block_f32, a negative count and every null argument, nothing written"""
    des, Sigma, qp, ql, _ = cases("corners")
    case = Case(ctx, des, Sigma, qp, ql)
    lib = case.lib

    def untouched():
        out = ctx.to_host(case.dout, 18 * case.n + 18)
        return np.all(np.isnan(out)) and ctx.to_host(case.dfail, 2, np.int32).tolist() == [7, 7]
    args = case.args()
    for k in range(len(args)):
        if k == 2:
            continue
        a = list(args)
        a[k] = None
        assert lib.cugo_pose_landmark_cross_covariances(*a) == ERR_INVALID, k
        assert b"null" in lib.cugo_last_error()
    a = list(args)
    a[2] = -1
    assert lib.cugo_pose_landmark_cross_covariances(*a) == ERR_INVALID
    case.ev.block_f32 = 1
    assert lib.cugo_pose_landmark_cross_covariances(*args) == ERR_INVALID
    assert b"block_f32" in lib.cugo_last_error()
    case.ev.block_f32 = 0
    assert untouched()
    got, _, flag = case.run()
    assert flag == 0 and np.all(np.isfinite(got))


# ------------------------------------------------------------------ S = J Sigma J^T ---------
@pytest.mark.parametrize("name", ("B", "mixed", "corners", "far"))
def test_reprojection_covariances(ctx, cases, name):
    """k_reprojection_cov on the design's estimates and cameras with Sigma_aa, the reference's Sigma_al and Sigma_ll of
    lm_cov_ref as inputs, every query as mono and as stereo, fixed poses, fixed landmarks and both: every entry within
    K_S (n + C_S) u mass of the longdouble J Sigma J^T, exactly symmetric, the third row and column zero for mono,
    zeros with both vertices fixed, the same bits on a second call, the nine doubles behind the output untouched"""
    des, Sigma, qp, ql, ref = cases(name)
    f = des["f"]
    inp = pr.reprojection_inputs(des, Sigma, qp, ql, ref)
    S, mass = pr.reprojection_of(inp)
    n = len(S)
    assert inp["stereo"].any() and (~inp["stereo"]).any()
    if name != "far":   # (every pose of `far` is free)
        assert (~inp["free_p"] & inp["free_l"]).any()
    if name in ("mixed", "corners"):
        assert (inp["free_p"] & ~inp["free_l"]).any() and (~inp["free_p"] & ~inp["free_l"]).any()
    lib = cugo.lib()
    q_aa = np.where(inp["free_p"], np.arange(n), -1).astype(np.int32)
    dev = [ctx.to_dev(inp["ip"].astype(np.int32)), ctx.to_dev(inp["il"].astype(np.int32)),
           ctx.to_dev(np.where(inp["stereo"], 3, 2).astype(np.int32)), ctx.to_dev(q_aa), ctx.to_dev(inp["cam"]),
           ctx.to_dev(f["poses"]), ctx.to_dev(f["lms"]), ctx.to_dev(kr.colmajor(inp["Saa"])),
           ctx.to_dev(kr.colmajor(inp["Sal"])), ctx.to_dev(kr.colmajor(inp["lmcov"]))]
    dout = ctx.to_dev(np.full(9 * n + 9, np.nan))

    def run():
        nan = np.full(9 * n + 9, np.nan)
        cugo.check(lib.cugo_memcpy_h2d(ctx.h, dout, nan.ctypes.data_as(C.c_void_p), nan.nbytes))
        cugo.reprojection_covariances(ctx.h, n, f["L"], *dev, dout)
        out = ctx.to_host(dout, 9 * n + 9)
        return kr.from_colmajor(out[:9 * n].reshape(n, 9), 3, 3).copy(), out[9 * n:].copy()
    got, tail = run()
    assert np.all(np.isfinite(got)) and np.all(np.isnan(tail))
    bnd = pr.bound_s(mass)
    r = np.array([kr.ratio(got[k], S[k], bnd[k]) for k in range(n)])
    print("%s: S of %d queries, worst ratio to the bound %.3g (fp64 replay: %.3g of the same bound)"
          % (name, n, r.max(), pr.REPLAY_S[name] / pr.K_S))
    assert r.max() <= 1, (name, int(r.argmax()), float(r.max()))
    assert same_bits(got, got.transpose(0, 2, 1).copy())
    mono = ~inp["stereo"]
    assert not got[mono][:, 2].any() and not got[mono][:, :, 2].any()
    assert got[inp["stereo"] & inp["free_p"] & inp["free_l"]][:, 2, 2].all()
    assert not got[~inp["free_p"] & ~inp["free_l"]].any()
    again, _ = run()
    assert same_bits(got, again)
    # refusals: every null argument, a negative count; n = 0 launches nothing
    args = [ctx.h, n, f["L"]] + dev + [dout]
    for k in [0] + list(range(3, len(args))):
        a = list(args)
        a[k] = None
        assert lib.cugo_reprojection_covariances(*a) == ERR_INVALID, k
    a = list(args)
    a[1] = -1
    assert lib.cugo_reprojection_covariances(*a) == ERR_INVALID
    nan = np.full(9 * n + 9, np.nan)
    cugo.check(lib.cugo_memcpy_h2d(ctx.h, dout, nan.ctypes.data_as(C.c_void_p), nan.nbytes))
    a[1] = 0
    assert lib.cugo_reprojection_covariances(*a) == 0
    assert np.all(np.isnan(ctx.to_host(dout, 9 * n + 9)))
