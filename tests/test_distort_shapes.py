"""GPU tests of distortion tables (radial-tangential lens distortion; cugo_edges.has_rig = 3) at
kernel level, through the C ABI, on the designed layouts of tests/distort_designed.py against the longdouble reference
of tests/distort_ref.py with its per-entry bounds (n + c) u mass — test_distort_ref_host.py shows on the CPU that a
float64 evaluation is inside them and ten plausible mistakes are far outside.

Plain entries (cugo_compute_active_errors, cugo_compute_edge_chi, cugo_construct_quadratic_form, with and without
landmark priors inside the build pass): every pattern and the hand-placed points, double and float block storage, and
a Tukey kernel that gives active distorted slots a weight of exactly 0.  Fused entries (the drivers of
test_fused_shapes.py): the patterns on the padded layouts, from_records = 1 against the block form bit for bit.  A
table of undistorted entries under has_rig = 3 gives the bits of has_rig = 1; every pattern run twice gives the same
bits; has_rig = 3 with a null table or with depth slots is CUGO_ERR_INVALID before any launch.  Every output is uploaded
filled with NaN."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import designed
import devmem
import distort_designed as dd
import distort_ref as dr
import kernel_ref as kr
import test_fused_shapes as tfs
import test_lm_prior_shapes as tls
import test_rig_shapes as trs

pytestmark = pytest.mark.gpu

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
LD = kr.LD
LAM = trs.LAM
report = trs.report
BUILD_KEYS = ("Hpp", "bp", "Hll", "bl", "Hpl", "chi")


@pytest.fixture(scope="module")
def ctx():
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    c = devmem.Ctx()
    yield c
    c.close()


class DRun(trs.RRun):
    """test_rig_shapes.RRun with the distortion table: has_rig = 3 and d_cam_ext -> f["cam_tab"] ([n][18])"""

    def __init__(self, c, f, hs, f32, rk2, has_rig=cugo.RIG_DISTORTION, padded=True, table=None):
        if table is None:
            table = f["cam_tab"] if has_rig == cugo.RIG_DISTORTION else f["cam_ext"]
        if has_rig == cugo.RIG_DISTORTION:      # bounds of the table: one 18-number entry per camera, every index inside
            assert table.shape == (len(f["cams"]), cugo.DIST_TAB_STRIDE) and int(f["cam_id"].max()) < len(table)
        super().__init__(c, f, hs, f32, rk2, has_rig, padded, table)


@functools.lru_cache(maxsize=None)
def reference(design, pattern, fused, which=0):
    """which: 0 none / Huber; 1 Tukey on the mono slots, which gives ACTIVE distorted slots a weight of exactly 0"""
    f, hs = dd.case(design, pattern, fused)
    rk2 = dd.robust2(design, which, fused)
    ref = dr.build(f, rk2)
    if which == 1:
        dead = (np.asarray(ref["w"]) == 0) & ((f["flags"] & 8) == 0) & f["dist"]
        assert ((f["flags"][dead] & 3) == 0).sum() >= 10, "too few active distorted slots of weight 0 between free vertices"
    return f, hs, rk2, ref


@functools.lru_cache(maxsize=None)
def hand_reference():
    f, hs = dd.hand_points()
    rk2 = dict(mono=(0, 1.0), stereo=(0, 1.0))
    return f, hs, rk2, dr.build(f, rk2)


def plain_entries(ctx, f, hs, rk2, ref, f32, tag, **kw):
    run = DRun(ctx, f, hs, f32, rk2, padded=False, **kw)
    chi = run.errors()
    assert report(tag + " errors chi", kr.ratio(chi, ref["chi"], kr.bound(ref["chi_n"], dr.C_CHI, ref["chi_mass"]))) <= 1
    chi_e = run.edge_chi()
    assert report(tag + " edge chi", dr.chi_e_ratio(chi_e, ref)) <= 1
    assert np.all(chi_e[(f["flags"] & 8) != 0] == 0)
    _, got = run.plain_build()
    trs.check_build(tag, got, ref, f32, dr.BUILD_C)
    assert run.errors() == chi and np.array_equal(run.edge_chi(), chi_e)
    _, again = run.plain_build()
    assert tfs.bits_equal(got, again, BUILD_KEYS)
    return run, chi, chi_e, got


@functools.lru_cache(maxsize=None)
def priors_on(design, pattern):
    """test_rig_shapes.priors_on for a case of this file (the layouts are the rig cases')"""
    return trs.priors_on(design, dd.BASE[pattern])


def joint_bound(ref, ref_p, key):
    return kr.bound(np.asarray(ref[key + "_n"]) + np.asarray(ref_p[key + "_n"]), dr.BUILD_C[key],
                    ref[key + "_mass"] + ref_p[key + "_mass"])


PLAIN = [c + (0,) for c in dd.PLAIN_CASES] + [("A", "all", 1), ("A", "third", 1)]
FUSED = [c + (0,) for c in dd.FUSED_CASES] + [("A", "all", 1), ("A", "third", 1)]


@pytest.mark.parametrize("design,pattern,which", PLAIN, ids=["%s-%s-rk%d" % c for c in PLAIN])
@pytest.mark.parametrize("f32", [False, True])
def test_plain_entries(ctx, design, pattern, which, f32):
    f, hs, rk2, ref = reference(design, pattern, False, which)
    tag = "%s %s rk%d f32=%d" % (design, pattern, which, f32)
    run, chi, chi_e, got = plain_entries(ctx, f, hs, rk2, ref, f32, tag)
    # landmark priors riding in the build pass: Hpp, bp, Hpl keep their bits, Hll, bl inside the joint bounds
    pr, lay, ref_p = priors_on(design, pattern)
    lev = tls.upload_priors(ctx, f, pr, lay)
    gp = run.prior_build(lev)
    assert tfs.bits_equal(gp, got, ("Hpp", "bp", "Hpl"))
    assert report(tag + " Hll (priors inside)", kr.ratio(tfs.mats(gp)["Hll"], ref["Hll"] + ref_p["Hll"], joint_bound(ref, ref_p, "Hll"))) <= 1
    assert report(tag + " bl (priors inside)", kr.ratio(gp["bl"], ref["bl"] + ref_p["bl"], joint_bound(ref, ref_p, "bl"))) <= 1
    assert np.abs(gp["Hll"] - got["Hll"]).max() > 0


@pytest.mark.parametrize("f32", [False, True])
def test_hand_placed_points(ctx, f32):
    """on the axis, a = 0 only, b = 0 only, r2 near 1 under a strong barrel k1, either side of and at the sign change of
    the radial factor, tangential only, k3 only: every output finite and inside the bounds, and per slot the Hpl block
    inside its own"""
    f, hs, rk2, ref = hand_reference()
    run, chi, chi_e, got = plain_entries(ctx, f, hs, rk2, ref, f32, "hand-placed f32=%d" % f32)
    assert np.isfinite(chi) and np.all(np.isfinite(chi_e)) and all(np.all(np.isfinite(got[k])) for k in BUILD_KEYS)
    bnd = kr.bound(1, dr.C_HPL, ref["Hpl_mass"])
    if f32:
        bnd = bnd + trs.F32 * (np.abs(ref["Hpl"]) + bnd)
    per = (np.abs(np.asarray(tfs.mats(got)["Hpl"], LD) - ref["Hpl"]) / np.where(bnd > 0, bnd, 1)).reshape(f["E"], -1).max(1)
    for i in range(f["E"]):
        print("%-24s %-16s Hpl %.3g of the bound" % (dd.HAND_NAMES[f["lm"][i]], dd.HAND_ENTRIES[f["cam_id"][i]][0], per[i]))
    assert per.max() <= 1


@pytest.mark.parametrize("design,pattern,which", FUSED, ids=["%s-%s-rk%d" % c for c in FUSED])
@pytest.mark.parametrize("f32", [False, True])
def test_fused_entries(ctx, design, pattern, which, f32):
    f, hs, rk2, ref = reference(design, pattern, True, which)
    P, L = f["P"], f["L"]
    dk = np.asarray(hs[0][:P])
    has = np.diff(f["lm_ptr"])[:L] > 0
    tag = "%s %s rk%d f32=%d" % (design, pattern, which, f32)
    xp = designed.random_blocks(f, seed=12)["xp"]
    run = DRun(ctx, f, hs, f32, rk2)
    d2, g2 = run.fused_build(LAM, 2)
    sch = {damp: run.fused_schur(d2, LAM, damp, 2) for damp in (0, 1)}
    d_bp = run.c.to_dev(sch[0]["bp_out"])
    bs = {rec: run.fused_backsubst(d2, d_bp, LAM, xp, rec) for rec in (0, 1)}
    dp, plain = run.plain_build()
    trs.check_build(tag, plain, ref, f32, dr.BUILD_C)
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
    assert report(tag + " G", dr.fused_stage_G(G, ref, f, Linv, f32)) <= 1
    assert np.all(G[(f["flags"] & 11) != 0] == 0)
    lines = dict(Linv=Linv, y=y)
    ps = kr.pose_schur(None, None, f, LAM, lines, ref=ref)
    for damp in (0, 1):
        s = sch[damp]
        assert all(np.all(np.isfinite(s[key])) for key in ("Hsc", "bp_out", "bsc")), "an entry was not written"
        Hsc = kr.from_colmajor(s["Hsc"], 6, 6)
        r = dr.fused_stage_pose(Hsc[dk], s["bp_out"], s["bsc"], ps, damp * LAM)
        t = "%s damp=%d" % (tag, damp)
        assert report(t + " diagonal", r["diag"]) <= 1 and report(t + " bp", r["bp"]) <= 1 and report(t + " bsc", r["bsc"]) <= 1
        assert report(t + " off-diagonal", kr.fused_stage_offdiag(Hsc, hs, G, P)) <= 1
    # back-substitution: the record form re-forms Xs, A and B with the build pass's functions -> the block form's bits
    b0, b1 = bs[0], bs[1]
    assert tfs.bits_equal(b0, b1, ("xl", "scale", "poses", "lms")), "from_records = 1 gives other bits than the G blocks"
    rb = kr.backsubst_lines(f, LAM, lines["Linv"], lines["y"], g2["bl"], sch[0]["bp_out"], G, xp, xl=b0["xl"])
    assert report(tag + " xl", kr.ratio(b0["xl"], rb["xl"], kr.bound(rb["xl_n"], kr.C_XL_LINES, rb["xl_mass"]))) <= 1
    assert np.all(b0["xl"][~has] == 0)
    # the two-stream form: every build output bitwise that of the plain build pass
    _, g1 = run.fused_build(LAM, 1)
    assert tfs.bits_equal(g1, plain, BUILD_KEYS), "form 1 differs from the plain build pass"


def all_entries(run, f, fused):
    """every kernel-level entry once: a flat list of (name, array)"""
    out = [("errors", np.array([run.errors()])), ("edge_chi", run.edge_chi())]
    _, got = run.plain_build()
    out += [("plain " + k, got[k]) for k in BUILD_KEYS]
    if fused:
        xp = designed.random_blocks(f, seed=12)["xp"]
        d2, g2 = run.fused_build(LAM, 2)
        s = run.fused_schur(d2, LAM, 1, 2)
        out += [("fused " + k, g2[k]) for k in ("Hll", "bl", "chi", "T")] + [("lmrec", g2["lmrec"][:, :9])]
        out += [("schur " + k, s[k]) for k in ("Hsc", "bp_out", "bsc")]
        for rec in (0, 1):
            b = run.fused_backsubst(d2, run.c.to_dev(s["bp_out"]), LAM, xp, rec)
            out += [("backsubst rec=%d %s" % (rec, k), b[k]) for k in ("xl", "scale", "poses", "lms")]
    return out


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("f32", [False, True])
def test_a_table_of_undistorted_entries_gives_the_bits_of_has_rig_1(ctx, fused, f32):
    """(the coefficients of the pattern's entries are not zero: a flag of 0 means they are not read)"""
    f, hs, rk2, _ = reference("A", "plain", fused)
    assert np.all(f["cam_tab"][:, 17] == 0) and np.all(f["cam_tab"][:, 12:17] != 0) and np.any(f["cam_ext"] != dr.IDENTITY12[None, :])
    assert np.any((f["flags"] & 4) != 0), "no stereo slot: the third row would go unchecked"
    three = all_entries(DRun(ctx, f, hs, f32, rk2, padded=fused), f, fused)
    one = all_entries(DRun(ctx, f, hs, f32, rk2, has_rig=cugo.RIG_EXTRINSICS, padded=fused), f, fused)
    for (name, a), (_, b) in zip(three, one):
        assert np.array_equal(a, b, equal_nan=True), name + ": has_rig = 3 with undistorted entries only differs from has_rig = 1"
    assert all(np.all(np.isfinite(a)) for name, a in three if name != "lmrec")


TWICE = [c + (False,) for c in dd.PLAIN_CASES] + [c + (True,) for c in dd.FUSED_CASES]


@pytest.mark.parametrize("design,pattern,fused", TWICE, ids=["%s-%s-fused%d" % c for c in TWICE])
def test_every_pattern_run_twice_gives_the_same_bits(ctx, design, pattern, fused):
    f, hs, rk2, _ = reference(design, pattern, fused)
    a = all_entries(DRun(ctx, f, hs, False, rk2, padded=fused), f, fused)
    b = all_entries(DRun(ctx, f, hs, False, rk2, padded=fused), f, fused)
    for (name, x), (_, y) in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True), name


@pytest.mark.parametrize("what", ["null_table", "with_depth"])
def test_invalid_distortion_members_are_refused_before_any_launch(ctx, what):
    """has_rig = 3 with a null table, or together with has_depth: CUGO_ERR_INVALID from every kernel-level entry, with
    a message, and every output still NaN"""
    f, hs, rk2, _ = reference("A", "third", True)
    run = DRun(ctx, f, hs, False, rk2)
    assert run.ev.has_rig == 3
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
