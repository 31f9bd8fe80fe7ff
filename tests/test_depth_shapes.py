"""GPU tests of the depth kind (flag bit 16, cugo_edges.has_depth) at kernel level, through the C
ABI, on the designed layouts of tests/depth_designed.py against the longdouble reference of tests/depth_ref.py with
kernel_ref's per-entry bounds (n + c) u mass — test_depth_ref_host.py shows on the CPU that a float64 evaluation is
inside them and five plausible mistakes are outside.

Plain entries (cugo_compute_active_errors, cugo_compute_edge_chi, cugo_construct_quadratic_form, with and without
landmark priors inside the build pass): every pattern, k in {1, 1e4}, double and float block storage, per-edge cameras
and information (the designs' own), a robust kernel per kind.  Fused entries (the drivers of test_fused_shapes.py: lines,
G, pose pass, record and block form of the back-substitution, the two-stream form): the patterns on the padded layouts.
Bit tests: the pattern without any depth slot has the bits of has_depth = 0; a second run has the bits of the first.
Every output is uploaded filled with NaN."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import depth_designed as dd
import depth_ref as dr
import designed
import devmem
import kernel_ref as kr
import lm_prior_ref as LR
import test_fused_shapes as tfs
import test_lm_prior_shapes as tls

pytestmark = pytest.mark.gpu

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
LD = kr.LD
F32 = LD(2.0 ** -24)
LAM = 0.5


def report(what, r):
    print("%-64s %.3g of the bound" % (what, r))
    return r


@pytest.fixture(scope="module")
def ctx():
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    c = devmem.Ctx()
    yield c
    c.close()


class DRun(tfs.Run):
    """test_fused_shapes.Run with a robust kernel per kind and the depth members of the edge view"""

    def __init__(self, c, f, hs, f32, rk3, k, has_depth=1, padded=True):
        if padded:
            designed.check_fused_layout(f)
        else:
            designed.check_layout(dict(f, flags=np.where(f["src"] >= 0, f["flags"] & 7, f["flags"]).astype(np.uint8)))
        self.c, self.f, self.hs, self.f32 = c, f, hs, f32
        self.bt = np.float32 if f32 else np.float64
        self.ev = devmem.upload_edges(c, f)
        self.ev.block_f32 = int(f32)
        self.ev.has_depth = int(has_depth)
        self.ev.rk_type_depth, self.ev.rk_delta_depth = int(rk3["depth"][0]), float(rk3["depth"][1])
        self.ev.depth_weight = float(k)
        rowptr, colind, off_ptr, ei, ej = hs
        self.B = len(colind)
        self.hsd = cugo.HscStruct(self.B, c.to_dev(rowptr), c.to_dev(colind), c.to_dev(off_ptr), c.to_dev(ei), c.to_dev(ej))
        self.d_poses, self.d_lms = c.to_dev(f["poses"]), c.to_dev(f["lms"])
        self.rk = cugo.Robust(int(rk3["mono"][0]), float(rk3["mono"][1]), int(rk3["stereo"][0]), float(rk3["stereo"][1]))
        self.h_lm_ptr = np.ascontiguousarray(f["lm_ptr"], np.int32)

    def errors(self):
        d = self.nan(4)
        cugo.check(cugo.lib().cugo_compute_active_errors(self.c.h, C.byref(self.ev), self.d_poses, self.d_lms, self.rk, d))
        return self.c.to_host(d, 1)[0]

    def edge_chi(self):
        d = self.nan(self.f["E"])
        cugo.check(cugo.lib().cugo_compute_edge_chi(self.c.h, C.byref(self.ev), self.d_poses, self.d_lms, self.rk, d))
        return self.c.to_host(d, self.f["E"])

    def prior_build(self, lev):
        d = self.build_arrays()
        cugo.construct_quadratic_form_lm_priors(self.c.h, self.ev, lev, self.d_poses, self.d_lms, self.rk, d["Hpp"], d["bp"],
                                                d["Hll"], d["bl"], d["Hpl"], d["chi"])
        return self.fetch_build(d)


@functools.lru_cache(maxsize=None)
def reference(design, pattern, k, fused):
    f, hs = dd.case(design, pattern, fused)
    rk3 = dd.robust3(design, 0, fused)
    return f, hs, rk3, dr.build(f, rk3, k)


def check_build(tag, got, ref, f32, keys=dr.KEYS):
    m = tfs.mats(got)
    vals = dict(Hpp=m["Hpp"], bp=got["bp"], Hll=m["Hll"], bl=got["bl"], Hpl=m["Hpl"], chi=got["chi"][0])
    for key in keys:
        bnd = kr.bound(ref[key + "_n"], kr.BUILD_C[key], ref[key + "_mass"])
        if key == "Hpl" and f32:
            bnd = bnd + F32 * (np.abs(ref[key]) + bnd)          # the block rounded to float
        assert report("%s %s" % (tag, key), kr.ratio(vals[key], ref[key], bnd)) <= 1, key


@functools.lru_cache(maxsize=None)
def priors_on(design, pattern):
    """landmark priors for the case: two on every fifth free landmark that has edge slots, Huber"""
    f, _ = dd.case(design, pattern)
    rng = np.random.default_rng(5)
    has = np.flatnonzero(np.diff(f["lm_ptr"])[:f["L"]] > 0)[::5]
    lm = np.repeat(has, 2).astype(np.int32)
    z = f["lms"][lm] + rng.normal(0, 0.2, (len(lm), 3))
    info = np.array([LR.random_spd3(rng, 2.0) for _ in lm])
    pr = LR.make_prior(lm, z, info, rk=(3, 0.4), active=np.ones(len(lm), bool))
    order, lay = LR.sort_by_landmark(pr, f["Lall"])
    ref_p = LR.reference_build(f["lms"], f["L"], dict(pr, lm=lay["lm"], z=pr["z"][order], info=pr["info"][order],
                                                      active=pr["active"][order]))
    return pr, lay, ref_p


PLAIN = [(d, p, k) for d, p in dd.PLAIN_CASES for k in dd.WEIGHTS]


@pytest.mark.parametrize("design,pattern,k", PLAIN, ids=["%s-%s-k%g" % c for c in PLAIN])
@pytest.mark.parametrize("f32", [False, True])
def test_plain_entries(ctx, design, pattern, k, f32):
    f, hs, rk3, ref = reference(design, pattern, k, False)
    tag = "%s %s k=%g f32=%d" % (design, pattern, k, f32)
    run = DRun(ctx, f, hs, f32, rk3, k, padded=False)
    chi = run.errors()
    assert report(tag + " errors chi", kr.ratio(chi, ref["chi"], kr.bound(ref["chi_n"], kr.C_CHI, ref["chi_mass"]))) <= 1
    chi_e = run.edge_chi()
    assert report(tag + " edge chi", dr.chi_e_ratio(chi_e, ref)) <= 1
    assert np.all(chi_e[(f["flags"] & 8) != 0] == 0)
    _, got = run.plain_build()
    check_build(tag, got, ref, f32)
    # the same bits on a second run of every entry
    assert run.errors() == chi and np.array_equal(run.edge_chi(), chi_e)
    _, again = run.plain_build()
    assert tfs.bits_equal(got, again, ("Hpp", "bp", "Hll", "bl", "Hpl", "chi"))
    # landmark priors riding in the build pass: Hpp, bp, Hpl keep their bits, Hll, bl, chi inside the joint bounds
    pr, lay, ref_p = priors_on(design, pattern)
    lev = tls.upload_priors(ctx, f, pr, lay)
    gp = run.prior_build(lev)
    assert tfs.bits_equal(gp, got, ("Hpp", "bp", "Hpl"))
    both = LR.combined(ref, ref_p)
    assert report(tag + " Hll (priors inside)", kr.ratio(tfs.mats(gp)["Hll"], both["Hll"], both["Hll_bound"])) <= 1
    assert report(tag + " bl (priors inside)", kr.ratio(gp["bl"], both["bl"], both["bl_bound"])) <= 1
    assert np.abs(gp["Hll"] - got["Hll"]).max() > 0
    if pattern == "none":
        # no depth slot at all: has_depth = 1 gives the bits of has_depth = 0 (the kernels the library has always run)
        old = DRun(ctx, f, hs, f32, rk3, k, has_depth=0, padded=False)
        assert old.errors() == chi and np.array_equal(old.edge_chi(), chi_e)
        assert tfs.bits_equal(old.plain_build()[1], got, ("Hpp", "bp", "Hll", "bl", "Hpl", "chi"))
        assert tfs.bits_equal(old.prior_build(lev), gp, ("Hpp", "bp", "Hll", "bl", "Hpl"))
    if pattern == "inactive":
        # an inactive slot with the DEPTH bit counts for nothing, whatever the kind: the bits of has_depth = 0
        old = DRun(ctx, f, hs, f32, rk3, k, has_depth=0, padded=False)
        assert tfs.bits_equal(old.plain_build()[1], got, ("Hpp", "bp", "Hll", "bl", "Hpl", "chi"))


FUSED = [(d, p, k) for d, p in dd.FUSED_CASES for k in dd.WEIGHTS]


@pytest.mark.parametrize("design,pattern,k", FUSED, ids=["%s-%s-k%g" % c for c in FUSED])
@pytest.mark.parametrize("f32", [False, True])
def test_fused_entries(ctx, design, pattern, k, f32):
    f, hs, rk3, ref = reference(design, pattern, k, True)
    P, L = f["P"], f["L"]
    dk = np.asarray(hs[0][:P])
    has = np.diff(f["lm_ptr"])[:L] > 0
    tag = "%s %s k=%g f32=%d" % (design, pattern, k, f32)
    xp = designed.random_blocks(f, seed=12)["xp"]

    def one_stream(run):
        d2, g2 = run.fused_build(LAM, 2)
        sch = {damp: run.fused_schur(d2, LAM, damp, 2) for damp in (0, 1)}
        d_bp = run.c.to_dev(sch[0]["bp_out"])
        bs = {rec: run.fused_backsubst(d2, d_bp, LAM, xp, rec) for rec in (0, 1)}
        return g2, sch, bs

    run = DRun(ctx, f, hs, f32, rk3, k)
    g2, sch, bs = one_stream(run)
    g2b, schb, bsb = one_stream(run)
    assert tfs.bits_equal(g2, g2b, ("Hll", "bl", "chi", "T")) and np.array_equal(g2["lmrec"][:, :9], g2b["lmrec"][:, :9], equal_nan=True)
    for damp in (0, 1):
        assert tfs.bits_equal(sch[damp], schb[damp], ("Hsc", "bp_out", "bsc")), "a second call gives other bits"
    for rec in (0, 1):
        assert tfs.bits_equal(bs[rec], bsb[rec], ("xl", "scale", "poses", "lms")), "a second call gives other bits"
    dp, plain = run.plain_build()
    check_build(tag, plain, ref, f32)
    # lines and G (stages 1 - 3 of test_fused_shapes)
    lines, G = tfs.check_one_stream_build(run, g2, plain, ref, LAM, tag)
    # the pose pass and the off-diagonal blocks (stage 4)
    ps = kr.pose_schur(None, None, f, LAM, lines, ref=ref)
    for damp in (0, 1):
        s = sch[damp]
        assert all(np.all(np.isfinite(s[key])) for key in ("Hsc", "bp_out", "bsc")), "an entry was not written"
        Hsc = kr.from_colmajor(s["Hsc"], 6, 6)
        r = kr.fused_stage_pose(Hsc[dk], s["bp_out"], s["bsc"], ps, damp * LAM)
        t = "%s damp=%d" % (tag, damp)
        assert report(t + " diagonal", r["diag"]) <= 1 and report(t + " bp", r["bp"]) <= 1 and report(t + " bsc", r["bsc"]) <= 1
        assert report(t + " off-diagonal", kr.fused_stage_offdiag(Hsc, hs, G, P)) <= 1
    # back-substitution: record form and block form (stage 7)
    b0, b1 = bs[0], bs[1]
    assert tfs.bits_equal(b0, b1, ("xl", "scale", "poses", "lms")), "from_records = 1 gives other bits than the G blocks"
    rb = kr.backsubst_lines(f, LAM, lines["Linv"], lines["y"], g2["bl"], sch[0]["bp_out"], G, xp, xl=b0["xl"])
    assert report(tag + " xl", kr.ratio(b0["xl"], rb["xl"], kr.bound(rb["xl_n"], kr.C_XL_LINES, rb["xl_mass"]))) <= 1
    assert np.all(b0["xl"][~has] == 0)
    assert report(tag + " scale", kr.ratio(b0["scale"][0], rb["scale"], kr.bound(rb["scale_n"], kr.C_SCALE, rb["scale_mass"]))) <= 1
    # the two-stream form: every build output bitwise that of the plain build pass
    _, g1 = run.fused_build(LAM, 1)
    assert tfs.bits_equal(g1, plain, ("Hpp", "bp", "Hll", "bl", "Hpl", "chi")), "form 1 differs from the plain build pass"
    if pattern == "none":
        old = DRun(ctx, f, hs, f32, rk3, k, has_depth=0)
        o2, osch, obs = one_stream(old)
        assert tfs.bits_equal(o2, g2, ("Hll", "bl", "chi", "T")) and np.array_equal(o2["lmrec"][:, :9], g2["lmrec"][:, :9], equal_nan=True)
        for damp in (0, 1):
            assert tfs.bits_equal(osch[damp], sch[damp], ("Hsc", "bp_out", "bsc"))
        for rec in (0, 1):
            assert tfs.bits_equal(obs[rec], bs[rec], ("xl", "scale", "poses", "lms"))


def test_bad_depth_members_are_refused(ctx):
    """has_depth with a weight that is not finite and > 0, or with an unknown robust kernel: CUGO_ERR_INVALID with a
    message, nothing launched; with has_depth = 0 the same members are never read"""
    f, hs, rk3, _ = reference("A", "third", 1.0, False)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        run = DRun(ctx, f, hs, False, rk3, bad, padded=False)
        d = run.nan(4)
        rc = cugo.lib().cugo_compute_active_errors(ctx.h, C.byref(run.ev), run.d_poses, run.d_lms, run.rk, d)
        assert rc == -3 and b"depth_weight" in cugo.lib().cugo_last_error()
        b = run.build_arrays()
        rc = cugo.lib().cugo_construct_quadratic_form(ctx.h, C.byref(run.ev), run.d_poses, run.d_lms, run.rk, b["Hpp"], b["bp"],
                                                      b["Hll"], b["bl"], b["Hpl"], b["chi"])
        assert rc == -3 and all(np.all(np.isnan(v)) for v in run.fetch_build(b).values())
        assert np.isnan(ctx.to_host(d, 1)[0])
        run.ev.has_depth = 0
        assert np.isfinite(run.errors())
    run = DRun(ctx, f, hs, False, dict(rk3, depth=(7, 1.0)), 1.0, padded=False)
    assert cugo.lib().cugo_compute_edge_chi(ctx.h, C.byref(run.ev), run.d_poses, run.d_lms, run.rk, run.nan(f["E"])) == -3
