"""GPU tests of the bundle-adjustment kernels (ba_kernels.hip, ba_math.h) on DESIGNED layouts, through the C ABI, against
the extended-precision reference tests/kernel_ref.py with per-entry bounds (n + c) u mass.

Layouts (tests/designed.py, asserted legal on the CPU before any upload): A pose degrees round every chunking constant
(0, 1, 6..8, 13..15, 64, 65, 223..225, 256, 257, 449, 512, 513, 705, 1025), B landmark degrees 1, 2, 255, 256, 257, 300
with straddled 256-slot boundaries and edgeless landmarks, C more landmarks than edge slots, U 64 free poses for the
pose update.  Rotations are general (all quaternion components O(0.4), some |qw| < 0.05).

Every output array is uploaded filled with NaN: an entry a kernel should have written and did not shows up.  Left
untouched by documented contract (include/cugo_hip.h): the estimates of fixed vertices in d_poses_out / d_lms_out and
d_invHll of a free landmark without edge slots.

Tolerances: nothing here was tuned on a GPU.  Sums: (n + c) u mass per entry (kernel_ref's docstring counts c); an entry
whose mass is zero must be exactly zero.  Measured on the CPU against the C oracle (test_kernel_ref_host.py), 4 x what
the oracle reaches: inverse K_INV = 20 u kappa max|inv| (oracle 4.99), pose update KQ = 10 u (oracle 2.41) and
KT = 21 u (|t| + |v| (1 + 1 / max(theta, 1e-5))) (oracle 5.07).

Schur complement, staged: (1) inv against the reference inverse; (2) T against Hpl x the DEVICE's inv; (3a) Hsc, bsc
against the reference evaluated from the DEVICE's T with (n + c) u mass — on the off-diagonal blocks, on the upper
triangle of the diagonal blocks and on bsc: the gather kernels form the upper triangle of a diagonal block and mirror
it, so its lower triangle is the sum over T's OTHER rows only up to T's rounding; (3b) every entry of Hsc and bsc
against the reference evaluated from the device's inv with exact T, bound (n + c + 4) u (mass with |Hpl| |inv| for
|T|): 4 = the roundings of the 3-term sum T, plus 2^-24 of the product mass where a kernel reads T stored as float (the
landmark-major plan never does: it keeps T in fp64 in LDS, so it gets no float term, and no 3a in the float mode);
(4) every form gives bitwise the same inv and T, and Hsc pairwise within the sum of the two bounds.
"""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import designed
import devmem
import kernel_ref as kr
import synth

pytestmark = pytest.mark.gpu

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
U = kr.U
F32 = 2.0 ** -24


@pytest.fixture(scope="module")
def ctx():
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    c = devmem.Ctx()
    yield c
    c.close()


def nan_dev(ctx, n, dtype=np.float64):
    return ctx.to_dev(np.full(max(int(n), 1), np.nan, dtype))


def upload(ctx, f, f32):
    designed.check_layout(f)       # no kernel is fed an illegal layout
    ev = devmem.upload_edges(ctx, f)
    ev.block_f32 = int(f32)
    return ev


def blk_dtype(f32):
    return np.float32 if f32 else np.float64


def report(what, r):
    print("%-40s %.3g of the bound" % (what, r))
    return r


# ------------------------------------------------------------------ a. build pass
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("kind", ["none", "huber", "tukey"])
@pytest.mark.parametrize("name", ["A", "B", "C", "A_padded"])
def test_build_pass(ctx, name, kind, f32):
    """A_padded: layout A in the engine's slot layout (devmem.pad_to_groups), whose padding slots are INACTIVE edges"""
    base = name.split("_")[0]
    _, prob0, f, _ = designed.layout(base)
    if name.endswith("_padded"):
        f = padded(base)[0]
        assert (f["flags"] & 8).any()
    rk = designed.robust_kernels(base)[kind]
    prob = prob0.copy()
    prob.rk_type, prob.rk_delta = rk
    ref = kr.build(prob, rk, f)
    if kind == "tukey":
        zero = float((np.asarray(ref["w"])[(f["flags"] & 8) == 0] == 0).mean())
        assert zero >= 0.1 and 1 - zero >= 0.1
    L = cugo.lib()
    P, Lf, E = f["P"], f["L"], f["E"]
    ev = upload(ctx, f, f32)
    rkc = cugo.Robust(rk[0], rk[1], rk[0], rk[1])
    d_poses, d_lms = ctx.to_dev(f["poses"]), ctx.to_dev(f["lms"])
    d = dict(Hpp=nan_dev(ctx, 36 * P), bp=nan_dev(ctx, 6 * P), Hll=nan_dev(ctx, 9 * Lf), bl=nan_dev(ctx, 3 * Lf),
             Hpl=nan_dev(ctx, 18 * E, blk_dtype(f32)), chi=nan_dev(ctx, 4))
    cugo.check(L.cugo_construct_quadratic_form(ctx.h, C.byref(ev), d_poses, d_lms, rkc, d["Hpp"], d["bp"], d["Hll"],
                                               d["bl"], d["Hpl"], d["chi"]))
    got = dict(Hpp=kr.from_colmajor(ctx.to_host(d["Hpp"], (P, 36)), 6, 6), bp=ctx.to_host(d["bp"], (P, 6)),
               Hll=kr.from_colmajor(ctx.to_host(d["Hll"], (Lf, 9)), 3, 3), bl=ctx.to_host(d["bl"], (Lf, 3)),
               Hpl=kr.from_colmajor(ctx.to_host(d["Hpl"], (E, 18), blk_dtype(f32)).astype(np.float64), 6, 3),
               chi=ctx.to_host(d["chi"], 1)[0])
    for k in ("Hpp", "bp", "Hll", "bl", "Hpl", "chi"):
        bnd = kr.bound(ref[k + "_n"], kr.BUILD_C[k], ref[k + "_mass"])
        if k == "Hpl" and f32:
            bnd = bnd + F32 * (np.abs(ref[k]) + bnd)          # the block rounded to float
        assert report("%s %s f32=%d %s" % (name, kind, f32, k), kr.ratio(got[k], ref[k], bnd)) <= 1, k
    # nothing contributes -> exact zeros: the pose without edges, the landmarks without edges, the blocks of edges
    # with a fixed endpoint (ratio() demands them where the mass is zero; spelled out here)
    deg = np.diff(f["pose_ptr"])[:P]
    lmdeg = np.diff(f["lm_ptr"])[:Lf]
    assert np.all(got["Hpp"][deg == 0] == 0) and np.all(got["bp"][deg == 0] == 0)
    assert np.all(got["Hll"][lmdeg == 0] == 0) and np.all(got["bl"][lmdeg == 0] == 0)
    assert np.all(got["Hpl"][(f["flags"] & 11) != 0] == 0)
    if base == "A":
        assert (deg == 0).sum() == 1
    else:
        assert (lmdeg == 0).sum() >= 4
    # the error-only pass
    chi2 = nan_dev(ctx, 2)
    cugo.check(L.cugo_compute_active_errors(ctx.h, C.byref(ev), d_poses, d_lms, rkc, chi2))
    bnd = kr.bound(ref["chi_n"], kr.C_CHI, ref["chi_mass"])
    assert report("%s %s chi (error pass)" % (name, kind), kr.ratio(ctx.to_host(chi2, 1)[0], ref["chi"], bnd)) <= 1
    # max diagonal of the device's own blocks: a maximum is exact
    md = nan_dev(ctx, 2)
    cugo.check(L.cugo_max_diagonal(ctx.h, d["Hpp"], P, d["Hll"], Lf, md))
    want = max(0.0, got["Hpp"][:, range(6), range(6)].max(), got["Hll"][:, range(3), range(3)].max())
    assert ctx.to_host(md, 1)[0] == want


# ------------------------------------------------------------------ b. Schur complement from supplied blocks
FORMS = {"default": {}, "mfma0": {"CUGO_HSC_MFMA": "0"}, "mfma2": {"CUGO_HSC_MFMA": "2"}, "xcd0": {"CUGO_HSC_XCD": "0"}}
LAMBDAS = (0.5, 300.0)


def form_ctx(monkeypatch, env):
    """a context of its own: it takes its snapshot of the CUGO_* switches when it is created"""
    with monkeypatch.context() as m:
        for k in ("CUGO_HSC_MFMA", "CUGO_HSC_XCD"):
            m.delenv(k, raising=False)
        for k, v in env.items():
            m.setenv(k, v)
        return devmem.Ctx()


@functools.lru_cache(maxsize=None)
def padded(name):
    f = devmem.pad_to_groups(designed.layout(name)[2])
    return f, devmem.hsc_structure(f)


class SchurCase:
    """supplied blocks of one layout, uploaded to one context"""

    def __init__(self, c, f, hs, blk, f32):
        self.c, self.f, self.hs, self.f32 = c, f, hs, f32
        self.ev = upload(c, f, f32)
        rowptr, colind, off_ptr, ei, ej = hs
        self.B = len(colind)
        self.hsd = cugo.HscStruct(self.B, c.to_dev(rowptr), c.to_dev(colind), c.to_dev(off_ptr), c.to_dev(ei), c.to_dev(ej))
        self.dev = dict(Hpp=c.to_dev(kr.colmajor(blk["Hpp"])), bp=c.to_dev(blk["bp"]), Hll=c.to_dev(kr.colmajor(blk["Hll"])),
                        bl=c.to_dev(blk["bl"]), Hpl=c.to_dev(kr.colmajor(blk["Hpl"]).astype(blk_dtype(f32))))
        self.plan = None

    def make_plan(self):
        f, (rowptr, colind, _, _, _) = self.f, self.hs
        as_p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        plan = C.c_void_p()
        rc = cugo.lib().cugo_hsc_plan_create(self.c.h, f["E"], f["P"], as_p(f["pose"], C.c_int32), as_p(f["lm"], C.c_int32),
                                             as_p(f["flags"], C.c_uint8), as_p(rowptr, C.c_int32), as_p(colind, C.c_int32),
                                             C.byref(self.hsd), C.byref(plan))
        self.plan = plan if rc == 0 else None
        return rc

    def run(self, lam, damp):
        c, f, d = self.c, self.f, self.dev
        P, Lf, E, B = f["P"], f["L"], f["E"], self.B
        bt = blk_dtype(self.f32)
        inv, T, bsc, Hsc = nan_dev(c, 9 * Lf), nan_dev(c, 18 * E, bt), nan_dev(c, 6 * P), nan_dev(c, 36 * B)
        cugo.check(cugo.lib().cugo_compute_schur(c.h, C.byref(self.ev), C.byref(self.hsd), C.c_double(lam), int(damp),
                                                 d["Hpp"], d["bp"], d["Hll"], d["bl"], d["Hpl"], inv, T, bsc, Hsc))
        return dict(inv=kr.from_colmajor(c.to_host(inv, (Lf, 9)), 3, 3),
                    T=kr.from_colmajor(c.to_host(T, (E, 18), bt).astype(np.float64), 6, 3),
                    bsc=c.to_host(bsc, (P, 6)), Hsc=kr.from_colmajor(c.to_host(Hsc, (B, 36)), 6, 6))

    def close(self):
        if self.plan:
            cugo.lib().cugo_hsc_plan_destroy(self.plan)
        self.c.close()


class SchurReference:
    """the staged references and bounds of one (layout, blocks, lambda); damp only adds lambda to the diagonal"""

    def __init__(self, f, hs, blk, lam, f32, first):
        self.f, self.lam = f, lam
        P, Lf = f["P"], f["L"]
        Hpl = kr.colmajor(blk["Hpl"]).astype(blk_dtype(f32)).astype(np.float64)     # the values the device holds
        Hpl = kr.from_colmajor(Hpl, 6, 3)
        args = (blk["Hpp"], blk["bp"], blk["Hll"], blk["bl"], Hpl)
        self.has_edges = np.diff(f["lm_ptr"])[:Lf] > 0
        self.diag = np.asarray(hs[0][:P])
        self.s3a = kr.schur(f, hs, lam, 0, *args, T=first["T"], inv=first["inv"], want=("mass",))
        self.s3b = kr.schur(f, hs, lam, 0, *args, inv=first["inv"], want=("Tmass",))
        s = self.s3b
        self.inv_ref, self.kappa = s["inv"], s["kappa"]
        self.eye = np.zeros((len(hs[1]), 6, 6))
        self.eye[self.diag] = np.eye(6)
        hpp = np.zeros((len(hs[1]), 6, 6))
        hpp[self.diag] = np.abs(blk["Hpp"])
        self.hpp, self.abp = hpp, np.abs(blk["bp"])
        # 3a is claimed on the off-diagonal blocks and the upper triangle (row <= column) of the diagonal blocks
        self.mask3a = np.ones((len(hs[1]), 6, 6), bool)
        self.mask3a[self.diag] = np.triu(np.ones((6, 6), bool))
        self.f32 = f32
        self.cache = {}

    def prepared(self, damp):
        """references and bounds of one damp flag, formed once for all forms"""
        if damp in self.cache:
            return self.cache[damp]
        s3a, s3b, m = self.s3a, self.s3b, self.mask3a
        dl = damp * self.lam
        p = dict(H3a=(s3a["Hsc"] + dl * self.eye)[m], bH3a=kr.bound(s3a["Hsc_n"], kr.C_HSC, s3a["Hsc_mass"] + dl * self.eye)[m],
                 bb3a=kr.bound(s3a["bsc_n"], kr.C_BSC, s3a["bsc_mass"]), H3b=s3b["Hsc"] + dl * self.eye)
        for flt in (0.0, F32):
            p["bH3b", flt] = (kr.bound(s3b["Hsc_n"], kr.C_HSC + 4, self.hpp + dl * self.eye + s3b["Hsc_Tmass"]) +
                              flt * s3b["Hsc_Tmass"])
            p["bb3b", flt] = kr.bound(s3b["bsc_n"], kr.C_BSC + 4, self.abp + s3b["bsc_Tmass"]) + flt * s3b["bsc_Tmass"]
            p["bH3b64", flt] = np.asarray(p["bH3b", flt], np.float64)
        self.cache = {damp: p}
        return p

    def check(self, got, damp, form, reads_stored_T, tag):
        s3a, s3b = self.s3a, self.s3b
        he = self.has_edges
        p = self.prepared(damp)
        # 1. the inverse, where a landmark has an edge slot
        binv = kr.K_INV * U * (self.kappa * np.abs(self.inv_ref).reshape(len(he), -1).max(1))[:, None, None] * np.ones((1, 3, 3))
        assert report(tag + " inv", kr.ratio(got["inv"][he], self.inv_ref[he], binv[he])) <= 1
        # 2. T against Hpl x the device's own inverse (3a's and 3b's T: same product)
        bT = kr.bound(3, kr.C_T, s3b["T_mass"])
        if self.f32:
            bT = bT + F32 * (np.abs(s3b["T"]) + bT)
        assert report(tag + " T", kr.ratio(got["T"], s3b["T"], bT)) <= 1
        # 3a. from the device's own T
        if reads_stored_T:
            assert report(tag + " Hsc (3a)", kr.ratio(got["Hsc"][self.mask3a], p["H3a"], p["bH3a"])) <= 1
            assert report(tag + " bsc (3a)", kr.ratio(got["bsc"], s3a["bsc"], p["bb3a"])) <= 1
        # 3b. every entry, from the device's inverse
        flt = F32 if (self.f32 and reads_stored_T) else 0.0
        assert report(tag + " Hsc (3b)", kr.ratio(got["Hsc"], p["H3b"], p["bH3b", flt])) <= 1
        assert report(tag + " bsc (3b)", kr.ratio(got["bsc"], s3b["bsc"], p["bb3b", flt])) <= 1
        return p["bH3b64", flt]


def same_outputs(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("inv", "T", "bsc", "Hsc"))


def check_forms(ref, cases, lam, damp, tag, reads_stored_T=lambda form: True):
    """runs every form, checks it against the staged references (a form whose four outputs are bitwise those of a
    form already checked shares its verdict), then compares the forms with each other"""
    results, bounds = {}, {}
    for form, case in cases.items():
        got = case.run(lam, damp)
        if ref[0] is None:
            ref[0] = SchurReference(case.f, case.hs, ref[1], lam, case.f32, got)
        twin = [o for o in results if same_outputs(results[o], got) and reads_stored_T(o) == reads_stored_T(form)]
        if twin:
            print("%s %s: bitwise the outputs of %s" % (tag, form, twin[0]))
            bounds[form] = bounds[twin[0]]
        else:
            bounds[form] = ref[0].check(got, damp, form, reads_stored_T(form), "%s damp=%d %s" % (tag, damp, form))
        results[form] = got
    compare_forms(results, bounds, "%s damp=%d" % (tag, damp))


def compare_forms(results, bounds, tag):
    """4. bitwise the same inv and T (where written), Hsc pairwise within the sum of the two bounds"""
    names = list(results)
    a = results[names[0]]
    for n in names[1:]:
        b = results[n]
        assert np.array_equal(a["inv"], b["inv"], equal_nan=True) and np.array_equal(a["T"], b["T"]), (tag, n)
        diff = np.abs(a["Hsc"] - b["Hsc"])
        assert np.all(diff <= bounds[names[0]] + bounds[n]), (tag, n)


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_schur_complement_from_supplied_blocks(name, f32, lam, monkeypatch):
    _, _, f, hs = designed.layout(name)
    blk = designed.random_blocks(f, seed=11)
    cases = {}
    try:
        for form, env in FORMS.items():
            cases[form] = SchurCase(form_ctx(monkeypatch, env), f, hs, blk, f32)
        ref = [None, blk]
        for damp in (0, 1):
            check_forms(ref, cases, lam, damp, "%s f32=%d lam=%g" % (name, f32, lam))
    finally:
        for case in cases.values():
            case.close()


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("name", ["A", "B"])
def test_schur_complement_landmark_major_plan(name, f32, lam, monkeypatch):
    """cugo_hsc_plan_create on the engine's padded slot layout (devmem.pad_to_groups).  B keeps landmarks of 257 and 300
    edges, which no padding brings inside one 256-slot group: the plan refuses them by contract (CUGO_ERR_INVALID, plan
    fields cleared), and B runs without them (layout B_plan)."""
    if name == "B":
        f0 = designed.layout("B")[2]
        g0 = devmem.pad_to_groups(f0)
        refused = SchurCase(form_ctx(monkeypatch, {}), g0, devmem.hsc_structure(g0), designed.random_blocks(g0, seed=11), f32)
        try:
            assert refused.make_plan() == -3 and not refused.plan and not refused.hsd.d_grp_ptr
        finally:
            refused.close()
        name = "B_plan"
    f, hs = padded(name)
    assert f["E"] > designed.layout(name)[2]["E"] and (f["flags"] & 8).any()
    blk = designed.random_blocks(f, seed=11)
    cases = {}
    try:
        for form in ("gather", "plan"):
            cases[form] = SchurCase(form_ctx(monkeypatch, {}), f, hs, blk, f32)
        assert cases["plan"].make_plan() == 0 and cases["plan"].hsd.d_grp_ptr
        assert cases["plan"].hsd.n_groups == (f["E"] + 255) // 256
        ref = [None, blk]
        for damp in (0, 1):
            # the plan forms its products from T in fp64 in LDS: the stored (float) T is an output only
            check_forms(ref, cases, lam, damp, "%s padded f32=%d lam=%g" % (name, f32, lam),
                        reads_stored_T=lambda form: form == "gather" or not f32)
    finally:
        for case in cases.values():
            case.close()


# ------------------------------------------------------------------ c. landmark back-substitution
def run_backsubst(ctx, f, ev, lam, inv, bl, bp, Hpl, xp, poses_in, f32):
    """cugo_backsubst_update with NaN-filled outputs; the rows of fixed vertices in the *_out arrays are documented as
    left untouched and hold the input"""
    P, Lf, E = f["P"], f["L"], f["E"]
    lms_in = f["lms"]
    poses_out, lms_out = poses_in.copy(), lms_in.copy()
    poses_out[:P] = np.nan
    lms_out[:Lf] = np.nan
    d_xl, d_scale = nan_dev(ctx, 3 * Lf), nan_dev(ctx, 2)
    d_po, d_lo = ctx.to_dev(poses_out), ctx.to_dev(lms_out)
    cugo.check(cugo.lib().cugo_backsubst_update(
        ctx.h, C.byref(ev), C.c_double(lam), ctx.to_dev(kr.colmajor(inv)), ctx.to_dev(bl), ctx.to_dev(bp),
        ctx.to_dev(kr.colmajor(Hpl).astype(blk_dtype(f32))), ctx.to_dev(xp), d_xl, ctx.to_dev(poses_in), ctx.to_dev(lms_in),
        d_po, d_lo, d_scale))
    return dict(xl=ctx.to_host(d_xl, (Lf, 3)), scale=ctx.to_host(d_scale, 1)[0],
                poses=ctx.to_host(d_po, (f["Pall"], 7)), lms=ctx.to_host(d_lo, (f["Lall"], 3)))


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_landmark_back_substitution(ctx, name, f32):
    _, _, f, _ = designed.layout(name)
    blk = designed.random_blocks(f, seed=12)
    lam = 0.5
    P, Lf = f["P"], f["L"]
    inv = np.asarray(kr.inv3(np.asarray(blk["Hll"] + lam * np.eye(3), kr.LD)), np.float64)
    inv = 0.5 * (inv + inv.transpose(0, 2, 1))
    Hpl = kr.from_colmajor(kr.colmajor(blk["Hpl"]).astype(blk_dtype(f32)).astype(np.float64), 6, 3)
    ev = upload(ctx, f, f32)
    got = run_backsubst(ctx, f, ev, lam, inv, blk["bl"], blk["bp"], Hpl, blk["xp"], f["poses"], f32)
    ref = kr.backsubst(f, lam, inv, blk["bl"], blk["bp"], Hpl, blk["xp"], xl=got["xl"])
    tag = "%s f32=%d " % (name, f32)
    assert report(tag + "xl", kr.ratio(got["xl"], ref["xl"], kr.bound(ref["xl_n"], kr.C_XL, ref["xl_mass"]))) <= 1
    lmdeg = np.diff(f["lm_ptr"])[:Lf]
    assert (lmdeg == 0).sum() >= (0 if name == "A" else 4) and np.all(got["xl"][lmdeg == 0] == 0)
    assert np.array_equal(got["lms"][:Lf], f["lms"][:Lf] + got["xl"])
    assert np.array_equal(got["lms"][Lf:], f["lms"][Lf:]) and np.array_equal(got["poses"][P:], f["poses"][P:])
    assert np.all(np.isfinite(got["poses"][:P]))
    assert report(tag + "scale", kr.ratio(got["scale"], ref["scale"],
                                          kr.bound(ref["scale_n"], kr.C_SCALE, ref["scale_mass"]))) <= 1


# ------------------------------------------------------------------ d. pose update
def test_pose_update_every_branch(ctx):
    """pose_exp_update through cugo_backsubst_update on layout U: theta in designed.THETAS (both sides of the 1e-5 switch,
    of trace = 0 at 2 pi / 3, and of pi) about x, y, z (the branches i = 0, 1, 2 of trace <= 0) and a general axis, and 12
    poses for which dq q has w = +-1e-6 / +-1e-13 (the sign flip)"""
    _, _, f, _ = designed.layout("U")
    P = f["P"]
    cases, dxs = designed.pose_update_cases()
    assert len(cases) == P == 64 and len(designed.THETAS) == 13
    blk = designed.random_blocks(f, seed=13)
    lam = 0.5
    poses_in = f["poses"].copy()
    poses_in[:P] = cases
    inv = np.asarray(kr.inv3(np.asarray(blk["Hll"] + lam * np.eye(3), kr.LD)), np.float64)
    inv = 0.5 * (inv + inv.transpose(0, 2, 1))
    ev = upload(ctx, f, False)
    got = run_backsubst(ctx, f, ev, lam, inv, blk["bl"], blk["bp"], blk["Hpl"], dxs, poses_in, False)
    assert np.array_equal(got["poses"][P:], poses_in[P:])          # fixed poses: bitwise unchanged
    wq = wt = 0.0
    flips = 0
    for i in range(P):
        ref = kr.pose_update(poses_in[i], dxs[i])
        q = got["poses"][i, :4]
        assert q[3] >= 0 and abs(np.linalg.norm(q) - 1) < 1e-15, (i, q)
        eq, et = kr.pose_update_error(got["poses"][i], ref, poses_in[i], dxs[i])
        print("case %2d theta %.9g: quaternion %.3g u, translation %.3g x base" % (i, np.linalg.norm(dxs[i][:3]), eq, et))
        assert eq <= kr.KQ and et <= kr.KT, (i, dxs[i], eq, et)
        wq, wt = max(wq, eq), max(wt, et)
        if i >= 52:
            dq = synth.quat_from_rotvec(dxs[i][:3])
            flips += synth.quat_mul(dq, poses_in[i, :4])[3] < 0
    assert flips == 6                                             # half of the w ~ 0 cases need the flip
    print("pose update: worst quaternion %.3g u (KQ %g), translation %.3g (KT %g)" % (wq, kr.KQ, wt, kr.KT))
    ref = kr.backsubst(f, lam, inv, blk["bl"], blk["bp"], blk["Hpl"], dxs, xl=got["xl"])
    assert report("U scale", kr.ratio(got["scale"], ref["scale"], kr.bound(ref["scale_n"], kr.C_SCALE, ref["scale_mass"]))) <= 1


# ------------------------------------------------------------------ e. graph level
GRAPH_FORMS = {"default": {}, "pose_schur0": {"CUGO_POSE_SCHUR": "0"}, "hsc_rows": {"CUGO_HSC_ROWS": "1"},
               "hsc_strip": {"CUGO_HSC_STRIP": "1"}, "schur_plan": {"CUGO_SCHUR_PLAN": "1"}, "mfma0": {"CUGO_HSC_MFMA": "0"}}
GRAPH_ITERS = 4


@pytest.fixture(scope="module")
def graph_reference():
    import oracle
    d = designed.graph_d()
    prob = oracle.Problem(*synth.problem_fields(d))
    sens, est = oracle.self_sensitivity(prob, GRAPH_ITERS, with_estimates=True)
    # the 1e-10 / 1e-9 bars are fair on this graph: the oracle against itself (other summation orders, other
    # factorisation) moves by far less (9.95e-15 and 1.2e-14 where this was written)
    assert sens is not None and max(sens) < 1e-11 and est < 1e-11, (sens, est)
    ref = prob.optimize(GRAPH_ITERS)
    assert len(ref) == GRAPH_ITERS
    return d, prob, ref


@pytest.mark.parametrize("form", list(GRAPH_FORMS))
def test_designed_graph_trajectory(graph_reference, form, monkeypatch):
    """4 LM iterations on layout A without the poses of degree < 6 (degrees 705 and 1025 exceed HS_CAP = 704 of the strip
    form; several rounds of k_pose_schur and k_hsc_rows) under every form of the Schur complement, against the oracle"""
    from test_gpu import assert_trajectories_match, run_graph
    d, prob, ref = graph_reference
    for k in ("CUGO_POSE_SCHUR", "CUGO_HSC_ROWS", "CUGO_HSC_STRIP", "CUGO_SCHUR_PLAN", "CUGO_HSC_MFMA", "CUGO_HSC_XCD",
              "CUGO_FLOAT32"):
        monkeypatch.delenv(k, raising=False)
    for k, v in GRAPH_FORMS[form].items():
        monkeypatch.setenv(k, v)
    out = run_graph(d, GRAPH_ITERS)
    assert_trajectories_match(out["stats"], ref, 1e-10)
    assert np.abs(out["pose"] - prob.pose).max() <= 1e-9 and np.abs(out["lm"] - prob.lm).max() <= 1e-9
    if form == "schur_plan":
        assert out["sstats"]["schur_slots"] > 0
    assert out["nedges"] == len(d["e_pose"])


def test_designed_graph_float32_block_storage(graph_reference):
    """the tolerance of test_gpu.test_float32_block_storage: chi2 of every iteration within 1e-5 relative of the fp64
    oracle, the same LM trials, estimates within 1e-4 (poses) / 1e-3 (landmarks)"""
    d, prob, ref = graph_reference
    g = cugo.graph_from_arrays(d)
    g.set_float32(True)
    g.initialize(); g.optimize(GRAPH_ITERS)
    st, pose, lm = g.stats(), g.poses(), g.landmarks()
    g.close()
    assert [a["trials"] for a in st] == [b["trials"] for b in ref]
    rel = max(abs(a["chi2"] - b["chi2"]) / b["chi2"] for a, b in zip(st, ref))
    assert rel < 1e-5, rel
    assert np.abs(pose - prob.pose).max() < 1e-4 and np.abs(lm - prob.lm).max() < 1e-3
