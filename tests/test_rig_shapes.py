"""GPU tests of camera extrinsics (cugo_edges.has_rig / d_cam_ext) at kernel level, through the C
ABI, on the designed layouts of tests/rig_designed.py against the longdouble reference of tests/rig_ref.py with its
per-entry bounds (n + c) u mass — test_rig_ref_host.py shows on the CPU that a float64 evaluation is inside them and
seven plausible mistakes are far outside.

Plain entries (cugo_compute_active_errors, cugo_compute_edge_chi, cugo_construct_quadratic_form, with and without
landmark priors inside the build pass): every pattern, double and float block storage, a robust kernel per kind.  Fused
entries (the drivers of test_fused_shapes.py: lines, G, pose pass, record and block form of the back-substitution, the
two-stream form): the patterns on the padded layouts.  The tables whose sensor poses are all identities are also held
to the bounds of the PLAIN reference (kernel_ref.build with kernel_ref's constants).  has_rig = 0 never reads
d_cam_ext; has_rig with a null table or with depth slots is CUGO_ERR_INVALID before any launch.  Every output is
uploaded filled with NaN."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import designed
import devmem
import kernel_ref as kr
import lm_prior_ref as LR
import rig_designed as rd
import rig_ref as rr
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


def upload_rig_edges(c, f, has_rig=1, table=None):
    """devmem.upload_edges as the full struct (cugo.RigEdges) with the extrinsics table (table: instead of f's)"""
    head = devmem.upload_edges(c, f)
    ev = cugo.RigEdges()
    for name, _ in cugo.Edges._fields_:
        setattr(ev, name, getattr(head, name))
    ev.has_rig = int(has_rig)
    ev.d_cam_ext = c.to_dev(np.ascontiguousarray(f["cam_ext"] if table is None else table, np.float64))
    return ev


class RRun(tfs.Run):
    """test_fused_shapes.Run with a robust kernel per kind and the rig members of the edge view"""

    def __init__(self, c, f, hs, f32, rk2, has_rig=1, padded=True, table=None):
        if padded:
            designed.check_fused_layout(f)
        else:
            designed.check_layout(dict(f, flags=np.where(f["src"] >= 0, f["flags"] & 7, f["flags"]).astype(np.uint8)))
        assert f["cam_ext"].shape == (len(f["cams"]), 12) and int(f["cam_id"].max()) < len(f["cams"])   # bounds of the table
        self.c, self.f, self.hs, self.f32 = c, f, hs, f32
        self.bt = np.float32 if f32 else np.float64
        self.ev = upload_rig_edges(c, f, has_rig, table)
        self.ev.block_f32 = int(f32)
        rowptr, colind, off_ptr, ei, ej = hs
        self.B = len(colind)
        self.hsd = cugo.HscStruct(self.B, c.to_dev(rowptr), c.to_dev(colind), c.to_dev(off_ptr), c.to_dev(ei), c.to_dev(ej))
        self.d_poses, self.d_lms = c.to_dev(f["poses"]), c.to_dev(f["lms"])
        self.rk = cugo.Robust(int(rk2["mono"][0]), float(rk2["mono"][1]), int(rk2["stereo"][0]), float(rk2["stereo"][1]))
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
def reference(design, pattern, fused, which=0):
    """which: rig_designed.robust2 — 0: none / Huber, 1: Tukey on the mono slots, which gives ACTIVE slots a weight of
    exactly 0 (the build pass forms their B, the record passes select zeros for it: every term carries the weight)"""
    f, hs = rd.case(design, pattern, fused)
    rk2 = rd.robust2(design, which, fused)
    ref = rr.build(f, rk2)
    if which == 1:
        dead = (np.asarray(ref["w"]) == 0) & ((f["flags"] & 8) == 0) & np.any(f["cam_ext"][f["cam_id"]] != rr.IDENTITY12, 1)
        assert ((f["flags"][dead] & 3) == 0).sum() >= 10, "too few active rig slots of weight 0 between free vertices"
    return f, hs, rk2, ref


@functools.lru_cache(maxsize=None)
def plain_reference(design, pattern, fused):
    """kernel_ref.build of a case whose sensor poses are all identities, with ONE robust kernel (kernel_ref has one)"""
    f, hs = rd.case(design, pattern, fused)
    assert np.all(f["cam_ext"] == rr.IDENTITY12[None, :])
    rk = rd.robust2(design, 0, fused)["stereo"]
    return f, hs, dict(mono=rk, stereo=rk), kr.build(None, rk, f)


def check_build(tag, got, ref, f32, consts=rr.BUILD_C, keys=rr.KEYS):
    m = tfs.mats(got)
    vals = dict(Hpp=m["Hpp"], bp=got["bp"], Hll=m["Hll"], bl=got["bl"], Hpl=m["Hpl"], chi=got["chi"][0])
    for key in keys:
        bnd = rr.bound_of(ref, key, consts)
        if key == "Hpl" and f32:
            bnd = bnd + F32 * (np.abs(ref[key]) + bnd)          # the block rounded to float
        assert report("%s %s" % (tag, key), kr.ratio(vals[key], ref[key], bnd)) <= 1, key


@functools.lru_cache(maxsize=None)
def priors_on(design, pattern):
    """landmark priors for the case: two on every fifth free landmark that has edge slots, Huber"""
    f, _ = rd.case(design, pattern)
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


def joint_bound(ref, ref_p, key):
    """the BA terms and the priors' summed: the joint count, the larger (the rig reference's) constant, the joint mass"""
    return kr.bound(np.asarray(ref[key + "_n"]) + np.asarray(ref_p[key + "_n"]), rr.BUILD_C[key],
                    ref[key + "_mass"] + ref_p[key + "_mass"])


def plain_entries(ctx, f, hs, rk2, ref, f32, tag, consts):
    run = RRun(ctx, f, hs, f32, rk2, padded=False)
    chi = run.errors()
    assert report(tag + " errors chi", kr.ratio(chi, ref["chi"], kr.bound(ref["chi_n"], consts["chi"], ref["chi_mass"]))) <= 1
    chi_e = run.edge_chi()
    if "chi_e" in ref:
        assert report(tag + " edge chi", rr.chi_e_ratio(chi_e, ref, consts["chi"])) <= 1
    else:   # (kernel_ref.build has no per-edge chi: the slots' sum against its chi, the additions of the sum on top)
        assert report(tag + " sum of edge chi", kr.ratio(np.asarray(chi_e, LD).sum(), ref["chi"],
                                                         kr.bound(ref["chi_n"], consts["chi"], ref["chi_mass"]))) <= 1
    assert np.all(chi_e[(f["flags"] & 8) != 0] == 0)
    _, got = run.plain_build()
    check_build(tag, got, ref, f32, consts)
    # the same bits on a second run of every entry
    assert run.errors() == chi and np.array_equal(run.edge_chi(), chi_e)
    _, again = run.plain_build()
    assert tfs.bits_equal(got, again, ("Hpp", "bp", "Hll", "bl", "Hpl", "chi"))
    return run, chi, chi_e, got


PLAIN = [c + (0,) for c in rd.PLAIN_CASES] + [("A", "one", 1), ("A", "many", 1)]
FUSED = [c + (0,) for c in rd.FUSED_CASES] + [("A", "one", 1), ("A", "many", 1)]


@pytest.mark.parametrize("design,pattern,which", PLAIN, ids=["%s-%s-rk%d" % c for c in PLAIN])
@pytest.mark.parametrize("f32", [False, True])
def test_plain_entries(ctx, design, pattern, which, f32):
    f, hs, rk2, ref = reference(design, pattern, False, which)
    tag = "%s %s rk%d f32=%d" % (design, pattern, which, f32)
    run, chi, chi_e, got = plain_entries(ctx, f, hs, rk2, ref, f32, tag, rr.BUILD_C)
    # landmark priors riding in the build pass: Hpp, bp, Hpl keep their bits, Hll, bl inside the joint bounds
    pr, lay, ref_p = priors_on(design, pattern)
    lev = tls.upload_priors(ctx, f, pr, lay)
    gp = run.prior_build(lev)
    assert tfs.bits_equal(gp, got, ("Hpp", "bp", "Hpl"))
    assert report(tag + " Hll (priors inside)", kr.ratio(tfs.mats(gp)["Hll"], ref["Hll"] + ref_p["Hll"], joint_bound(ref, ref_p, "Hll"))) <= 1
    assert report(tag + " bl (priors inside)", kr.ratio(gp["bl"], ref["bl"] + ref_p["bl"], joint_bound(ref, ref_p, "bl"))) <= 1
    assert np.abs(gp["Hll"] - got["Hll"]).max() > 0


@pytest.mark.parametrize("pattern", ["identity", "none"])
@pytest.mark.parametrize("f32", [False, True])
def test_identity_tables_are_inside_the_plain_bounds(ctx, pattern, f32):
    """has_rig = 1 with identities only: the rig-aware kernels, held to kernel_ref.build with kernel_ref's constants"""
    f, hs, rk2, ref = plain_reference("A", pattern, False)
    plain_entries(ctx, f, hs, rk2, ref, f32, "A %s (plain bounds) f32=%d" % (pattern, f32), kr.BUILD_C)


@pytest.mark.parametrize("design,pattern,which", FUSED, ids=["%s-%s-rk%d" % c for c in FUSED])
@pytest.mark.parametrize("f32", [False, True])
def test_fused_entries(ctx, design, pattern, which, f32):
    f, hs, rk2, ref = reference(design, pattern, True, which)
    P, L = f["P"], f["L"]
    dk = np.asarray(hs[0][:P])
    has = np.diff(f["lm_ptr"])[:L] > 0
    tag = "%s %s rk%d f32=%d" % (design, pattern, which, f32)
    xp = designed.random_blocks(f, seed=12)["xp"]

    def one_stream(run):
        d2, g2 = run.fused_build(LAM, 2)
        sch = {damp: run.fused_schur(d2, LAM, damp, 2) for damp in (0, 1)}
        d_bp = run.c.to_dev(sch[0]["bp_out"])
        bs = {rec: run.fused_backsubst(d2, d_bp, LAM, xp, rec) for rec in (0, 1)}
        return g2, sch, bs

    run = RRun(ctx, f, hs, f32, rk2)
    g2, sch, bs = one_stream(run)
    g2b, schb, bsb = one_stream(run)
    assert tfs.bits_equal(g2, g2b, ("Hll", "bl", "chi", "T")) and np.array_equal(g2["lmrec"][:, :9], g2b["lmrec"][:, :9], equal_nan=True)
    for damp in (0, 1):
        assert tfs.bits_equal(sch[damp], schb[damp], ("Hsc", "bp_out", "bsc")), "a second call gives other bits"
    for rec in (0, 1):
        assert tfs.bits_equal(bs[rec], bsb[rec], ("xl", "scale", "poses", "lms")), "a second call gives other bits"
    dp, plain = run.plain_build()
    check_build(tag, plain, ref, f32)
    # stages 1 - 3 of test_fused_shapes.check_one_stream_build, with the rig reference's constants
    assert np.all(np.isfinite(g2["Hll"])) and np.all(np.isfinite(g2["bl"])) and np.all(np.isfinite(g2["chi"]))
    assert np.all(np.isfinite(g2["T"]))
    for k in ("Hpp", "bp", "Hpl", "inv"):
        assert np.all(np.isnan(g2[k])), k + " is documented as not written in form 2"
    assert np.all(np.isfinite(g2["lmrec"][has, :9])) and np.all(np.isnan(g2["lmrec"][~has]))
    assert tfs.bits_equal(g2, plain, ("Hll", "bl", "chi")), "Hll, bl, chi differ from the plain build pass"
    m = tfs.mats(g2)
    Linv, y = kr.lines_from6(g2["lmrec"][:L])
    st = kr.fused_stage_lines(Linv[has], y[has], m["Hll"][has], g2["bl"][has], LAM)
    assert report(tag + " lines", st["lines"]) <= 1 and report(tag + " y", st["y"]) <= 1
    G = m["T"]
    assert report(tag + " G", rr.fused_stage_G(G, ref, f, Linv, f32)) <= 1
    assert np.all(G[(f["flags"] & 11) != 0] == 0)
    lines = dict(Linv=Linv, y=y)
    # the pose pass and the off-diagonal blocks (stage 4)
    ps = kr.pose_schur(None, None, f, LAM, lines, ref=ref)
    for damp in (0, 1):
        s = sch[damp]
        assert all(np.all(np.isfinite(s[key])) for key in ("Hsc", "bp_out", "bsc")), "an entry was not written"
        Hsc = kr.from_colmajor(s["Hsc"], 6, 6)
        r = rr.fused_stage_pose(Hsc[dk], s["bp_out"], s["bsc"], ps, damp * LAM)
        t = "%s damp=%d" % (tag, damp)
        assert report(t + " diagonal", r["diag"]) <= 1 and report(t + " bp", r["bp"]) <= 1 and report(t + " bsc", r["bsc"]) <= 1
        assert report(t + " off-diagonal", kr.fused_stage_offdiag(Hsc, hs, G, P)) <= 1
    # back-substitution: record form and block form (stage 7): the record form re-forms G with the build pass's bits
    b0, b1 = bs[0], bs[1]
    assert tfs.bits_equal(b0, b1, ("xl", "scale", "poses", "lms")), "from_records = 1 gives other bits than the G blocks"
    rb = kr.backsubst_lines(f, LAM, lines["Linv"], lines["y"], g2["bl"], sch[0]["bp_out"], G, xp, xl=b0["xl"])
    assert report(tag + " xl", kr.ratio(b0["xl"], rb["xl"], kr.bound(rb["xl_n"], kr.C_XL_LINES, rb["xl_mass"]))) <= 1
    assert np.all(b0["xl"][~has] == 0)
    assert report(tag + " scale", kr.ratio(b0["scale"][0], rb["scale"], kr.bound(rb["scale_n"], kr.C_SCALE, rb["scale_mass"]))) <= 1
    # the two-stream form: every build output bitwise that of the plain build pass
    _, g1 = run.fused_build(LAM, 1)
    assert tfs.bits_equal(g1, plain, ("Hpp", "bp", "Hll", "bl", "Hpl", "chi")), "form 1 differs from the plain build pass"


@pytest.mark.parametrize("fused", [False, True])
def test_has_rig_0_never_reads_the_table(ctx, fused):
    """has_rig = 0 with a d_cam_ext that points at NaNs (a small valid buffer): finite results inside the plain bounds,
    and bitwise those of a struct whose d_cam_ext is NULL"""
    f, hs, rk2, ref = plain_reference("A", "none", fused)
    nans = np.full((len(f["cams"]), 12), np.nan)
    run = RRun(ctx, f, hs, False, rk2, has_rig=0, padded=fused, table=nans)
    null = RRun(ctx, f, hs, False, rk2, has_rig=0, padded=fused)
    null.ev.d_cam_ext = None
    chi, chi_e = run.errors(), run.edge_chi()
    assert np.isfinite(chi) and np.all(np.isfinite(chi_e)) and chi == null.errors() and np.array_equal(chi_e, null.edge_chi())
    _, got = run.plain_build()
    check_build("has_rig=0 fused=%d" % fused, got, ref, False, kr.BUILD_C)
    assert tfs.bits_equal(got, null.plain_build()[1], ("Hpp", "bp", "Hll", "bl", "Hpl", "chi"))
    if fused:
        xp = designed.random_blocks(f, seed=12)["xp"]
        outs = []
        for r in (run, null):
            d2, g2 = r.fused_build(LAM, 2)
            s = r.fused_schur(d2, LAM, 1, 2)
            b = r.fused_backsubst(d2, r.c.to_dev(s["bp_out"]), LAM, xp, 1)
            assert all(np.all(np.isfinite(s[k])) for k in ("Hsc", "bp_out", "bsc")) and np.all(np.isfinite(b["xl"]))
            outs.append((g2, s, b))
        assert tfs.bits_equal(outs[0][0], outs[1][0], ("Hll", "bl", "chi", "T"))
        assert tfs.bits_equal(outs[0][1], outs[1][1], ("Hsc", "bp_out", "bsc"))
        assert tfs.bits_equal(outs[0][2], outs[1][2], ("xl", "scale", "poses", "lms"))


@pytest.mark.parametrize("what", ["null_table", "with_depth"])
def test_invalid_rig_members_are_refused_before_any_launch(ctx, what):
    """has_rig with a null table, or together with has_depth: CUGO_ERR_INVALID from every kernel-level entry, with a
    message, and every output still NaN"""
    f, hs, rk2, _ = reference("A", "third", True)
    run = RRun(ctx, f, hs, False, rk2)
    if what == "null_table":
        run.ev.d_cam_ext = None
    else:
        run.ev.has_depth, run.ev.depth_weight = 1, 1.0
    needle = b"d_cam_ext" if what == "null_table" else b"not supported yet"
    L_ = cugo.lib()
    ev = C.byref(run.ev)
    d = run.nan(4)
    assert L_.cugo_compute_active_errors(ctx.h, ev, run.d_poses, run.d_lms, run.rk, d) == -3 and needle in L_.cugo_last_error()
    assert np.isnan(ctx.to_host(d, 1)[0])
    de = run.nan(f["E"])
    assert L_.cugo_compute_edge_chi(ctx.h, ev, run.d_poses, run.d_lms, run.rk, de) == -3
    assert np.all(np.isnan(ctx.to_host(de, f["E"])))
    b = run.build_arrays()
    assert L_.cugo_construct_quadratic_form(ctx.h, ev, run.d_poses, run.d_lms, run.rk, b["Hpp"], b["bp"], b["Hll"], b["bl"],
                                            b["Hpl"], b["chi"]) == -3
    pr, lay, _ = priors_on("A", "third")
    lev = tls.upload_priors(ctx, f, pr, lay)
    with pytest.raises(cugo.CugoError):
        cugo.construct_quadratic_form_lm_priors(ctx.h, run.ev, lev, run.d_poses, run.d_lms, run.rk, b["Hpp"], b["bp"], b["Hll"],
                                                b["bl"], b["Hpl"], b["chi"])
    lmp = run.h_lm_ptr.ctypes.data_as(C.POINTER(C.c_int32))
    assert L_.cugo_construct_quadratic_form_fused(ctx.h, ev, lmp, run.d_poses, run.d_lms, run.rk, LAM, 2, b["Hpp"], b["bp"],
                                                  b["Hll"], b["bl"], b["Hpl"], b["inv"], b["T"], b["lmrec"], b["chi"]) == -3
    assert all(np.all(np.isnan(v)) for v in run.fetch_build(b).values())
    P = f["P"]
    Hsc, bpo, bsc = run.nan(36 * run.B), run.nan(6 * P), run.nan(6 * P)
    assert L_.cugo_compute_schur_fused(ctx.h, ev, C.byref(run.hsd), LAM, 1, 2, run.d_poses, b["Hpp"], b["bp"], b["Hll"], b["bl"],
                                       b["Hpl"], b["inv"], b["T"], b["lmrec"], bpo, bsc, Hsc) == -3
    assert all(np.all(np.isnan(v)) for v in run.fetch_schur(Hsc, bpo, bsc).values())
    d_xl, d_scale = run.nan(3 * f["L"]), run.nan(2)
    xp = designed.random_blocks(f, seed=12)["xp"]
    d_po, d_lo = ctx.to_dev(np.full_like(f["poses"], np.nan)), ctx.to_dev(np.full_like(f["lms"], np.nan))
    assert L_.cugo_backsubst_update_fused(ctx.h, ev, LAM, b["lmrec"], b["bl"], bpo, b["T"], ctx.to_dev(xp), d_xl, run.d_poses,
                                          run.d_lms, d_po, d_lo, d_scale, 1) == -3
    assert np.all(np.isnan(ctx.to_host(d_xl, (f["L"], 3)))) and np.all(np.isnan(ctx.to_host(d_po, (f["Pall"], 7))))
