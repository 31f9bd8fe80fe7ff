"""GPU tests of k_predict_obs (cov_kernels.hip) through cugo.predict_observations, on the designs `mixed`, `corners`
and `grid513` of tests/lm_cov_designed.py with the inputs of pl_cov_ref.reprojection_inputs and the designed camera
tables of tests/predict_ref.py (one 64-lane wave holds pinhole-identity, rig and Kannala-Brandt entries, the kinds
2 / 3 / 4, fixed poses, fixed landmarks, both, and the hand-placed Kannala-Brandt points of tests/fisheye_designed.py),
against the longdouble reference and the per-entry bounds of predict_ref (tests/test_predict_ref_host.py measures their
constants and shows that the bounds see eight planted mistakes).

Query counts 1, 255, 256, 257, 513: the block edges of a one-thread-per-query, 256-wide launch.  Both outputs are NaN
before every call, with spare doubles behind them.  The Sigma blocks of fixed vertices are NaN on the device."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import kernel_ref as kr
import lm_cov_designed as ld
import pl_cov_ref as pr
import predict_ref as P

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
pytestmark = pytest.mark.gpu
COUNTS = (1, 255, 256, 257, 513)


@pytest.fixture(scope="module")
def ctx():
    import devmem
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    c = devmem.Ctx()
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def designed(name):
    """(design, inputs of the reprojection reference, designed queries, reference with the table, queries a pinhole at
    the pose can answer, their reference without a table): computed once, never modified"""
    des = ld.design(name)
    Sigma = pr.dense_sigma(des, 0.0)
    qp, ql = pr.queries(des)
    inp = pr.reprojection_inputs(des, Sigma, qp, ql, pr.reference(des, Sigma, qp, ql))
    q = P.designed_queries(des, inp)
    plain = P.without_hand_points(q)
    return des, inp, q, P.predict_of(q), plain, P.predict_of(plain, table=False)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


class Device:
    """n designed queries on the device; run(table, kind) -> (z [n,3], S [n,3,3])"""

    def __init__(self, ctx, q, n):
        self.ctx, self.n, self.q = ctx, n, q
        s = slice(0, n)
        self.L = q["Lfree"]
        self.ip, self.il = ctx.to_dev(q["ip"][s].astype(np.int32)), ctx.to_dev(q["il"][s].astype(np.int32))
        self.kind = ctx.to_dev(q["kind"][s].astype(np.int32))
        self.aa = ctx.to_dev(q["q_aa"][s].astype(np.int32))
        self.cam = ctx.to_dev(np.ascontiguousarray(q["cam"][s]))
        self.tab = ctx.to_dev(np.ascontiguousarray(q["tab"][s]))
        self.poses, self.lms = ctx.to_dev(q["poses"]), ctx.to_dev(q["lms"])
        # (q_aa indexes the per-query blocks: all of them are uploaded, NaN where the pose is fixed)
        self.Saa = ctx.to_dev(kr.colmajor(q["Saa"]))
        self.Sal = ctx.to_dev(kr.colmajor(q["Sal"][s]))
        self.lmcov = ctx.to_dev(kr.colmajor(q["lmcov"]))
        self.dz, self.dS = ctx.to_dev(np.full(3 * n + 3, np.nan)), ctx.to_dev(np.full(9 * n + 9, np.nan))

    def args(self, table=True, kind=None):
        return [self.ctx.h, self.n, self.L, self.ip, self.il, self.kind if kind is None else kind, self.aa, self.cam,
                self.tab if table is True else table, self.poses, self.lms, self.Saa, self.Sal, self.lmcov, self.dz, self.dS]

    def fill_nan(self):
        lib = cugo.lib()
        for d, k in ((self.dz, 3), (self.dS, 9)):
            nan = np.full(k * self.n + k, np.nan)
            cugo.check(lib.cugo_memcpy_h2d(self.ctx.h, d, nan.ctypes.data_as(C.c_void_p), nan.nbytes))

    def fetch(self):
        n = self.n
        z, S = self.ctx.to_host(self.dz, 3 * n + 3), self.ctx.to_host(self.dS, 9 * n + 9)
        assert np.all(np.isnan(z[3 * n:])) and np.all(np.isnan(S[9 * n:])), "the doubles behind the outputs were written"
        return z[:3 * n].reshape(n, 3).copy(), kr.from_colmajor(S[:9 * n].reshape(n, 9), 3, 3).copy()

    def run(self, table=True, kind=None):
        self.fill_nan()
        cugo.predict_observations(*self.args(table, kind))
        return self.fetch()


def check(name, z, S, ref, n, what):
    """z and S of the first n queries per entry inside the bounds; S exactly symmetric; the third row and column zero
    where the query has no third row; zeros where both vertices are fixed, z computed there too"""
    sub = {k: v[:n] for k, v in ref.items()}
    assert np.all(np.isfinite(z)) and np.all(np.isfinite(S)), (name, what)
    rs, rz = P.ratios(S, sub["S"], P.bound_s(sub)), P.ratios(z, sub["z"], P.bound_z(sub))
    print("%-8s %-22s n = %4d: worst S %.3g, z %.3g of the bound (fp64 replay: %.3g, %.3g of the same bounds)"
          % (name, what, n, rs.max(), rz.max(), P.REPLAY_S[name] / P.K_S_PRED, P.REPLAY_Z[name] / P.K_Z_PRED))
    assert rs.max() <= 1, (name, what, int(rs.argmax()), float(rs.max()))
    assert rz.max() <= 1, (name, what, int(rz.argmax()), float(rz.max()))
    assert same_bits(S, S.transpose(0, 2, 1).copy())
    no3 = ~sub["rows3"]
    assert not S[no3][:, 2].any() and not S[no3][:, :, 2].any() and not z[no3][:, 2].any()
    return rs, rz


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name", P.DESIGNS)
def test_designed_tables_within_bounds_repeatable(ctx, name, n):
    des, inp, q, ref, _, _ = designed(name)
    assert q["n"] >= 513 or name == "corners"
    n = min(n, q["n"])       # (`corners` has 498 queries: its last count is all of them, still two blocks, the second partial)
    c = q["census"]
    assert min(c["pinhole_identity"], c["pinhole_rig"], c["kb_rig"], c["fixed_pose"], c["fixed_lm"], c["both_fixed"]) >= 3
    assert c["hand"] == q["n_hand"] and c["kinds"] == [2, 3, 4]
    dev = Device(ctx, q, n)
    z, S = dev.run()
    check(name, z, S, ref, n, "designed table")
    fp, fl, fish = q["free_p"][:n], q["free_l"][:n], q["tab"][:n, 16] != 0
    assert not S[~fp & ~fl].any() and z[~fp & ~fl].any() == bool((~fp & ~fl).any())
    assert not S[fish][:, 2].any() and not S[fish][:, :, 2].any()                  # whatever the kind
    if n >= P.WAVE:
        assert (fish & (q["kind"][:n] != 2)).any() and (~fish & (q["kind"][:n] == 4) & fp & fl).any()
        assert S[~fish & (q["kind"][:n] != 2) & fp & fl][:, 2, 2].all()
    z2, S2 = dev.run()
    assert same_bits(z, z2) and same_bits(S, S2), name


@pytest.mark.parametrize("name", P.DESIGNS)
def test_without_a_table_the_bits_of_reprojection_covariances(ctx, name):
    """NULL table: kinds 2 / 3 give np.array_equal with cugo.reprojection_covariances on the same inputs; the kinds
    2 / 3 / 4 in turn are inside the bounds of the table-free reference; an all-pinhole-identity table stays inside the
    same bounds"""
    des, inp, q, _, plain, ref = designed(name)
    n = min(plain["n"], 1025)
    dev = Device(ctx, plain, n)
    z, S = dev.run(table=None)
    check(name, z, S, ref, n, "no table")
    assert (plain["kind"][:n] == 4).any()
    # the same queries as mono / stereo through both entry points
    dim = np.where(np.arange(n) % 2 == 0, 2, 3).astype(np.int32)
    ddim = ctx.to_dev(dim)
    z23, S23 = dev.run(table=None, kind=ddim)
    a = dev.args(None, ddim)
    dold = ctx.to_dev(np.full(9 * n, np.nan))
    cugo.reprojection_covariances(*(a[:8] + a[9:14] + [dold]))
    old = kr.from_colmajor(ctx.to_host(dold, 9 * n).reshape(n, 9), 3, 3)
    assert np.array_equal(S23, old) and same_bits(S23, np.ascontiguousarray(old)), name
    ref23 = P.predict(plain["pose"][:n], plain["Xw"][:n], plain["cam"][:n], dim, None, plain["Saa"][:n], plain["Sal"][:n],
                      plain["Sll"][:n], plain["free_p"][:n], plain["free_l"][:n])
    check(name, z23, S23, ref23, n, "no table, kinds 2 / 3")
    # an identity table: another sequence of operations, the same bounds
    ident = ctx.to_dev(cugo.camera_model_table(n=n))
    zi, Si = dev.run(table=ident)
    check(name, zi, Si, ref, n, "identity table")


def test_refusals(ctx):
    """CUGO_ERR_INVALID for every null required argument and a negative count, nothing written; a NULL table is no
    refusal; n = 0 launches nothing"""
    des, inp, q, ref, _, _ = designed("corners")
    dev = Device(ctx, q, 64)
    lib = cugo.lib()
    args = dev.args()
    dev.fill_nan()
    for k in [0] + [i for i in range(3, len(args)) if i != 8]:
        a = list(args)
        a[k] = None
        assert lib.cugo_predict_observations(*a) == -3, k
        assert b"null" in lib.cugo_last_error()
    for bad in ((1, -1), (2, -1)):
        a = list(args)
        a[bad[0]] = bad[1]
        assert lib.cugo_predict_observations(*a) == -3
    a = list(args)
    a[1] = 0
    assert lib.cugo_predict_observations(*a) == 0
    z, S = dev.ctx.to_host(dev.dz, 3 * 64 + 3), dev.ctx.to_host(dev.dS, 9 * 64 + 9)
    assert np.all(np.isnan(z)) and np.all(np.isnan(S))
    z, S = dev.run()
    check("corners", z, S, ref, 64, "after the refusals")
