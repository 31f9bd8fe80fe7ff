"""GPU tests of the landmark covariance kernel (k_lm_covariance of cov_kernels.hip) through cugo_landmark_covariances,
on the designs of tests/lm_cov_designed.py against the longdouble reference and the per-entry bound of
tests/lm_cov_ref.py (K_LM (n + C_LM) u sqrt(cond Hll) mass; tests/test_lm_cov_host.py measures K_LM and shows that the
bound sees a dropped term, a transposed block and a neighbouring block).

In every design the Hpl block of every slot that does not count (FIXED_P, FIXED_L, INACTIVE, padding) is NaN on the
device, the output is NaN before the call and has nine spare doubles behind it, and the flag holds 7 before the call.
"""
import ctypes as C
import importlib

import numpy as np
import pytest

import designed
import kernel_ref as kr
import lm_cov_designed as ld
import lm_cov_ref as lr

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
def refs():
    cache = {}

    def get(name):
        if name not in cache:
            des = ld.design(name)
            cache[name] = (des, lr.reference(des["f"], des["rowptr"], des["colind"], des["Hll"], des["Hpl"], des["sigma"]))
        return cache[name]
    return get


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


class Case:
    """one design on the device"""

    def __init__(self, ctx, des, f=None, Hpl=None):
        import devmem
        self.ctx, self.lib = ctx, cugo.lib()
        self.f = des["f"] if f is None else f
        designed.check_layout(self.f)
        Hpl = des["Hpl"] if Hpl is None else Hpl
        assert len(Hpl) == self.f["E"] and np.all(np.isnan(Hpl[(self.f["flags"] & lr.SKIP) != 0]))
        self.L = self.f["L"]
        self.ev = devmem.upload_edges(ctx, self.f)
        self.hs = cugo.HscStruct()
        self.hs.n_blocks = len(des["colind"])
        self.hs.d_rowptr, self.hs.d_colind = ctx.to_dev(des["rowptr"]), ctx.to_dev(des["colind"])
        self.dHll = ctx.to_dev(kr.colmajor(des["Hll"]))
        self.dHpl = ctx.to_dev(kr.colmajor(Hpl))
        self.dsigma = ctx.to_dev(des["sigma"])
        self.dout = ctx.to_dev(np.full(9 * self.L + 9, np.nan))
        self.dfail = ctx.to_dev(np.array([7, 7], np.int32))

    def run(self, dHll=None):
        """(cov [L,3,3], the nine doubles behind it, flag) of one call on a NaN-filled output and a flag of 7"""
        nan, seven = np.full(9 * self.L + 9, np.nan), np.array([7, 7], np.int32)
        cugo.check(self.lib.cugo_memcpy_h2d(self.ctx.h, self.dout, nan.ctypes.data_as(C.c_void_p), nan.nbytes))
        cugo.check(self.lib.cugo_memcpy_h2d(self.ctx.h, self.dfail, seven.ctypes.data_as(C.c_void_p), seven.nbytes))
        cugo.check(self.lib.cugo_landmark_covariances(self.ctx.h, C.byref(self.ev), C.byref(self.hs),
                                                      self.dHll if dHll is None else dHll, self.dHpl, self.dsigma,
                                                      self.dout, self.dfail))
        out = self.ctx.to_host(self.dout, 9 * self.L + 9)
        flag = self.ctx.to_host(self.dfail, 2, np.int32)
        assert flag[1] == 7
        return kr.from_colmajor(out[:9 * self.L].reshape(self.L, 9), 3, 3).copy(), out[9 * self.L:].copy(), int(flag[0])


def check_blocks(name, got, ref, what=""):
    """every entry of every block that the reference does not fail inside its bound; failed blocks nine zeros; a
    marginal landmark (lm_cov_ref) either; returns the landmarks whose block is zero"""
    r = lr.ratios(got, ref, lr.bound(ref))
    zero = [l for l in range(len(got)) if not got[l].any()]
    sure = ~ref["marginal"]
    print("%s%s: worst ratio to the bound %.3g (fp64 replay: %.3g of the same bound), zero blocks %s"
          % (name, what, r.max(), lr.REPLAY.get(name, np.nan) / lr.K_LM, zero))
    assert np.all(np.isfinite(got)), name
    assert r.max() <= 1, (name, int(r.argmax()), float(r.max()))
    assert set(zero) - set(np.flatnonzero(~sure).tolist()) == set(np.flatnonzero(ref["fail"] & sure).tolist()), (name, zero)
    return zero


def expected_flag(ref, zero):
    """1 when a landmark fails; a marginal landmark raises it exactly when its block came out as zeros"""
    return int(bool(ref["fail"].any()) or any(ref["marginal"][l] for l in zero))


# ------------------------------------------------------------------ every design ---------
@pytest.mark.parametrize("name", ld.NAMES)
def test_blocks_within_bound_symmetric_repeatable(ctx, refs, name):
    """every entry of every non-failing block within K_LM (n + C_LM) u sqrt(cond Hll) mass of the reference; each block
    exactly symmetric; the same bits on a second call; the nine doubles behind the output untouched; the flag 0 on a
    design without a degenerate landmark (B and B_padded have edgeless free landmarks: test_layout_B_...)"""
    des, ref = refs(name)
    case = Case(ctx, des)
    got, tail, flag = case.run()
    zero = check_blocks(name, got, ref)
    assert same_bits(got, got.transpose(0, 2, 1).copy()), name
    assert np.all(np.isnan(tail)), (name, tail)
    assert flag == expected_flag(ref, zero), (name, flag)
    if not name.startswith("B"):
        assert flag == 0 and not zero
    again, tail2, flag2 = case.run()
    assert same_bits(got, again) and np.all(np.isnan(tail2)) and flag2 == flag, name


def test_layout_B_with_its_edgeless_free_landmarks(ctx, refs):
    """layout B and its padded form: flag 1, nine zeros for exactly the free landmarks without an edge, all others
    non-zero and within bound.  The one landmark that a single mono edge sees has a rank-2 Hll: whether its last pivot
    comes out positive is a matter of rounding (lm_cov_ref: marginal), so it may be zeros too."""
    for name in ("B", "B_padded"):
        des, ref = refs(name)
        f = des["f"]
        edgeless = [l for l in range(f["L"]) if not ((f["flags"][f["lm_ptr"][l]:f["lm_ptr"][l + 1]] & 8) == 0).any()]
        assert len(edgeless) == 5 and edgeless == np.flatnonzero(ref["fail"]).tolist()
        got, _, flag = Case(ctx, des).run()
        zero = check_blocks(name, got, ref, " (edgeless landmarks)")
        assert flag == 1
        assert set(edgeless) <= set(zero) and all(ref["marginal"][l] for l in set(zero) - set(edgeless)), zero
        assert int(ref["marginal"].sum()) == 1


def test_padding_changes_no_bit(ctx, refs):
    """B_padded holds the edges of B in other slots with INACTIVE padding between them: the same bits"""
    a, _, _ = Case(ctx, refs("B")[0]).run()
    b, _, _ = Case(ctx, refs("B_padded")[0]).run()
    assert same_bits(a, b)


# ------------------------------------------------------------------ the failure flag ---------
def test_failure_flag_on_mixed(ctx, refs):
    """one landmark's Hll replaced in turn by a matrix whose first, second or third pivot is -L_jj^2 / 2 (built from the
    reference's own Cholesky factor: 1.5 L_jj^2 taken off the diagonal entry, the pivots before it untouched), then by
    one with a NaN off the diagonal and one with a NaN on it: the flag is 1, that block is nine zeros, every other
    block keeps the bits of the clean run; a clean call afterwards clears the flag"""
    des, ref = refs("mixed")
    case = Case(ctx, des)
    clean, _, flag = case.run()
    assert flag == 0
    lt = int(np.flatnonzero(ref["deg"] >= 3)[len(np.flatnonzero(ref["deg"] >= 3)) // 2])
    Lf = lr.chol3(np.asarray(des["Hll"][lt], kr.LD), kr.LD)
    bad = []
    for j in range(3):
        H = des["Hll"].copy()
        H[lt, j, j] -= float(1.5 * Lf[j, j] ** 2)
        Lb = lr.chol3(np.asarray(H[lt], kr.LD), kr.LD)
        assert Lb is None
        if j:   # the pivots before it hold
            top = lr.chol3(np.asarray(np.block([[H[lt, :j, :j], np.zeros((j, 3 - j))], [np.zeros((3 - j, j)), np.eye(3 - j)]]),
                                      kr.LD), kr.LD)
            assert top is not None
        bad.append(("pivot %d" % j, H))
    H = des["Hll"].copy()
    H[lt, 1, 0] = H[lt, 0, 1] = np.nan
    bad.append(("NaN off the diagonal", H))
    H = des["Hll"].copy()
    H[lt, 2, 2] = np.nan
    bad.append(("NaN on the diagonal", H))
    others = np.arange(case.L) != lt
    for what, H in bad:
        got, tail, flag = case.run(ctx.to_dev(kr.colmajor(H)))
        assert flag == 1, what
        assert not got[lt].any() and not np.isnan(got[lt]).any(), what
        assert same_bits(got[others], clean[others]), what
        assert np.all(np.isnan(tail)), what
        back, _, flag = case.run()
        assert flag == 0 and same_bits(back, clean), what


# ------------------------------------------------------------------ slot order ---------
def test_invariance_under_a_permutation_of_a_landmarks_slots(ctx, refs):
    """designed.check_layout asks for landmark-major slots and leaves the order within a landmark free.  mixed with the
    slots of every landmark reversed, B with the slots of the 300-edge landmark shuffled and those of the 100-edge one
    reversed: the permuted landmarks within the sum of the two bounds of the unpermuted run, both runs within bound,
    the landmarks whose slots stayed bit for bit"""
    rng = np.random.default_rng(9)
    for name in ("mixed", "B"):
        des, ref = refs(name)
        f = des["f"]
        deg_slots = np.diff(f["lm_ptr"])[:f["L"]]
        if name == "mixed":
            perms = {l: np.arange(deg_slots[l])[::-1].tolist() for l in range(f["L"]) if deg_slots[l] >= 2}
        else:
            perms = {int(np.argmax(deg_slots)): rng.permutation(int(deg_slots.max())).tolist(),
                     designed.B_LM_DEGREES.index(100): np.arange(100)[::-1].tolist()}
        g, src = ld.permuted_slots(f, perms)
        moved = np.array([l in perms and ref["deg"][l] >= 2 for l in range(f["L"])])
        assert moved.sum() >= 2 and any(np.any(np.diff(g["pose"][g["lm_ptr"][l]:g["lm_ptr"][l + 1]]) < 0) for l in perms)
        base, _, _ = Case(ctx, des).run()
        got, tail, flag = Case(ctx, des, f=g, Hpl=des["Hpl"][src]).run()
        check_blocks(name, got, ref, " (permuted slots)")
        bnd = np.asarray(lr.bound(ref), np.float64)
        worst = float((np.abs(got - base)[moved] / (2 * bnd[moved])).max())
        print("%s: permuted against unpermuted, worst %.3g of the sum of the two bounds" % (name, worst))
        assert worst <= 1
        assert same_bits(got[~moved], base[~moved]) and np.all(np.isnan(tail))


# ------------------------------------------------------------------ refusals ---------
def test_refusals(ctx, refs):
    """CUGO_ERR_INVALID for block_f32 and for every null argument, nothing written; CUGO_OK and nothing launched when
    there is no free landmark"""
    des, _ = refs("grid1")
    case = Case(ctx, des)
    lib = case.lib
    args = [ctx.h, C.byref(case.ev), C.byref(case.hs), case.dHll, case.dHpl, case.dsigma, case.dout, case.dfail]

    def untouched():
        out = ctx.to_host(case.dout, 9 * case.L + 9)
        return np.all(np.isnan(out)) and ctx.to_host(case.dfail, 2, np.int32).tolist() == [7, 7]
    for k in range(len(args)):
        a = list(args)
        a[k] = None
        assert lib.cugo_landmark_covariances(*a) == ERR_INVALID, k
        assert b"null" in lib.cugo_last_error()
    assert untouched()
    case.ev.block_f32 = 1
    assert lib.cugo_landmark_covariances(*args) == ERR_INVALID
    assert b"block_f32" in lib.cugo_last_error() and untouched()
    case.ev.block_f32 = 0
    case.ev.n_landmarks_free = 0
    assert lib.cugo_landmark_covariances(*args) == 0
    assert untouched()
    case.ev.n_landmarks_free = case.L
    got, _, flag = case.run()
    assert flag == 0 and np.all(np.isfinite(got))
