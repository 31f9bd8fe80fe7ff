"""GPU tests of the FUSED iteration's kernels (DESIGN.md sections 4c / 4d) on designed layouts, through the kernel-level C
entries cugo_construct_quadratic_form_fused / cugo_compute_schur_fused / cugo_backsubst_update_fused, against the
longdouble references of tests/kernel_ref.py with per-entry bounds: k_build_edges' gform branch (the 3 x 3 factorisation,
the landmarks' lines, G), k_pose_schur, the off-diagonal kernels with both operands out of G, k_backsubst_landmarks with
the lines (from the G blocks and from the records), and the two-stream fused form.

Layouts (designed.fused_layout, each with its census asserted on the CPU; all in the engine's padded slot layout): A
(pose degrees round k_pose_schur's 256 lanes: 0, 1, ..., 256, 257, 512, 513, 1025), B_plan (landmark degrees 1, 2, 255,
256, owners on the first and the last slot of a group, edgeless landmarks), C (more landmarks than slots), U (the pose
update), F-dead (a landmark and a pose all of whose edges are INACTIVE), F-allfixed (no free landmark: the landmark
lines are 16 NaNs), F-cond (kappa(Hll + lam I) from 1e2 to 1e10).  Robust kernels none, Huber, Tukey; both storage
types; damp_hsc_diag 0 and 1; the off-diagonal forms CUGO_HSC_MFMA 0, 1, 2 x CUGO_HSC_XCD 0, 1 (the full product on
A, the default and one other value of each elsewhere).

Every output is uploaded filled with NaN.  Contract (include/cugo_hip.h): what must be written is finite; in form 2
d_Hpp, d_bp, d_Hpl, d_invHll and the lines of landmarks without any slot are NOT written and still NaN.

Stages (kernel_ref.fused_stage_*; nothing here was tuned on a GPU, test_fused_ref_host.py sizes every bound on the CPU):
 1. Hll, bl, chi of the fused entry: against kernel_ref.build with BUILD_C, and bitwise those of
    cugo_construct_quadratic_form.
 2. the lines: L^-1 against fused_lines of the DEVICE's Hll, bl with K_CHOL u kappa max|L^-1|; y against the DEVICE's
    L^-1 x bl with (3 + C_LINE_Y) u mass.
 3. G against the reference Hpl x the DEVICE's L^-1 (Hpl's bound carried through |L^-1|, + (3 + C_G) u mass, + the
    float rounding); exact zeros on slots that take no part.
 4. off-diagonal Hsc against - sum G_i G_j^T from the DEVICE's G; diagonal blocks, bp, bsc against pose_schur from the
    DEVICE's lines.
 5. every entry of Hsc and bsc against kernel_ref.schur of the reference build with end_to_end_bounds: the build
    bounds carried through the Schur complement, stage 2's allowance for the lines (6 K_CHOL) or K_INV for the adjugate
    inverse, each form's own arithmetic (stage 4's masses for the one-stream form: |L^-T| |L^-1| has none of the
    cancellation of inv) and float_storage_bounds.  Hence the one-stream form, the two-stream form and
    cugo_compute_schur agree pairwise within the sum of their bounds, which is asserted as well.
 6. the two-stream fused form: every build output bitwise that of cugo_construct_quadratic_form, invHll and T bitwise
    those of cugo_compute_schur from them, Hsc and bsc bitwise those of the unfused call.
 7. back-substitution: xl against backsubst_lines from the DEVICE's lines and G with (n + C_XL_LINES) u mass,
    lms_out == lms_in + xl bitwise, scale within its bound, from_records = 1 the bits of from_records = 0.
A second run of the three entries gives the same bits.
"""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import designed
import devmem
import kernel_ref as kr

pytestmark = pytest.mark.gpu

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
LD, U = kr.LD, kr.U
MF, XC = "CUGO_HSC_MFMA", "CUGO_HSC_XCD"
FORMS_ALL = {"default": {}, "mfma0": {MF: "0"}, "mfma2": {MF: "2"}, "xcd0": {XC: "0"}, "mfma0_xcd0": {MF: "0", XC: "0"},
             "mfma2_xcd0": {MF: "2", XC: "0"}}
FORMS_FEW = {k: FORMS_ALL[k] for k in ("default", "mfma0", "xcd0")}
WORST = {}


def report(what, key, r):
    print("%-52s %.3g of the bound" % (what + " " + key, r))
    WORST[key] = max(WORST.get(key, 0.0), r)
    return r


def form_ctx(monkeypatch, env):
    """a context of its own: it takes its snapshot of the CUGO_* switches when it is created"""
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    with monkeypatch.context() as m:
        for k in (MF, XC):
            m.delenv(k, raising=False)
        for k, v in env.items():
            m.setenv(k, v)
        return devmem.Ctx()


def bits_equal(a, b, keys):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


class Run:
    """one layout uploaded to one context; every output array of every call starts as NaN"""

    def __init__(self, c, f, hs, f32, rk):
        designed.check_fused_layout(f)          # no kernel is fed an illegal layout
        self.c, self.f, self.hs, self.f32 = c, f, hs, f32
        self.bt = np.float32 if f32 else np.float64
        self.ev = devmem.upload_edges(c, f)
        self.ev.block_f32 = int(f32)
        rowptr, colind, off_ptr, ei, ej = hs
        self.B = len(colind)
        self.hsd = cugo.HscStruct(self.B, c.to_dev(rowptr), c.to_dev(colind), c.to_dev(off_ptr), c.to_dev(ei), c.to_dev(ej))
        self.d_poses, self.d_lms = c.to_dev(f["poses"]), c.to_dev(f["lms"])
        self.rk = cugo.Robust(rk[0], rk[1], rk[0], rk[1])
        self.h_lm_ptr = np.ascontiguousarray(f["lm_ptr"], np.int32)

    def nan(self, n, dtype=np.float64):
        return self.c.to_dev(np.full(max(int(n), 1), np.nan, dtype))

    def build_arrays(self):
        f = self.f
        P, L, E = f["P"], f["L"], f["E"]
        return dict(Hpp=self.nan(36 * P), bp=self.nan(6 * P), Hll=self.nan(9 * L), bl=self.nan(3 * L),
                    Hpl=self.nan(18 * E, self.bt), inv=self.nan(9 * L), T=self.nan(18 * E, self.bt),
                    lmrec=self.nan(16 * max(L, 1)), chi=self.nan(4))

    def fetch_build(self, d):
        f, c = self.f, self.c
        P, L, E = f["P"], f["L"], f["E"]
        return dict(Hpp=c.to_host(d["Hpp"], (P, 36)), bp=c.to_host(d["bp"], (P, 6)), Hll=c.to_host(d["Hll"], (L, 9)),
                    bl=c.to_host(d["bl"], (L, 3)), Hpl=c.to_host(d["Hpl"], (E, 18), self.bt),
                    inv=c.to_host(d["inv"], (L, 9)), T=c.to_host(d["T"], (E, 18), self.bt),
                    lmrec=c.to_host(d["lmrec"], (max(L, 1), 16)), chi=c.to_host(d["chi"], 1))

    def plain_build(self):
        d = self.build_arrays()
        cugo.check(cugo.lib().cugo_construct_quadratic_form(self.c.h, C.byref(self.ev), self.d_poses, self.d_lms, self.rk,
                                                            d["Hpp"], d["bp"], d["Hll"], d["bl"], d["Hpl"], d["chi"]))
        return d, self.fetch_build(d)

    def fused_build(self, lam, form):
        d = self.build_arrays()
        cugo.check(cugo.lib().cugo_construct_quadratic_form_fused(
            self.c.h, C.byref(self.ev), self.h_lm_ptr.ctypes.data_as(C.POINTER(C.c_int32)), self.d_poses, self.d_lms,
            self.rk, lam, form, d["Hpp"], d["bp"], d["Hll"], d["bl"], d["Hpl"], d["inv"], d["T"], d["lmrec"], d["chi"]))
        return d, self.fetch_build(d)

    def fetch_schur(self, Hsc, bpo, bsc):
        P, c = self.f["P"], self.c
        return dict(Hsc=c.to_host(Hsc, (self.B, 36)), bp_out=c.to_host(bpo, (P, 6)), bsc=c.to_host(bsc, (P, 6)))

    def fused_schur(self, d, lam, damp, form):
        P = self.f["P"]
        Hsc, bpo, bsc = self.nan(36 * self.B), self.nan(6 * P), self.nan(6 * P)
        cugo.check(cugo.lib().cugo_compute_schur_fused(
            self.c.h, C.byref(self.ev), C.byref(self.hsd), lam, int(damp), form, self.d_poses, d["Hpp"], d["bp"], d["Hll"],
            d["bl"], d["Hpl"], d["inv"], d["T"], d["lmrec"], bpo, bsc, Hsc))
        return self.fetch_schur(Hsc, bpo, bsc)

    def unfused_schur(self, d, lam, damp):
        """cugo_compute_schur from the arrays of a plain build pass; inv and T into fresh NaN arrays"""
        f, c = self.f, self.c
        P, L, E = f["P"], f["L"], f["E"]
        inv, T = self.nan(9 * L), self.nan(18 * E, self.bt)
        Hsc, bpo, bsc = self.nan(36 * self.B), self.nan(6 * P), self.nan(6 * P)
        cugo.check(cugo.lib().cugo_compute_schur(c.h, C.byref(self.ev), C.byref(self.hsd), C.c_double(lam), int(damp),
                                                 d["Hpp"], d["bp"], d["Hll"], d["bl"], d["Hpl"], inv, T, bsc, Hsc))
        out = self.fetch_schur(Hsc, bpo, bsc)
        out.update(inv=c.to_host(inv, (L, 9)), T=c.to_host(T, (E, 18), self.bt))
        return out

    def fused_backsubst(self, d, d_bp, lam, xp, from_records):
        f, c = self.f, self.c
        P, L = f["P"], f["L"]
        poses_out, lms_out = f["poses"].copy(), f["lms"].copy()
        poses_out[:P] = np.nan
        lms_out[:L] = np.nan
        d_xl, d_scale, d_po, d_lo = self.nan(3 * L), self.nan(2), c.to_dev(poses_out), c.to_dev(lms_out)
        cugo.check(cugo.lib().cugo_backsubst_update_fused(
            c.h, C.byref(self.ev), lam, d["lmrec"], d["bl"], d_bp, d["T"], c.to_dev(xp), d_xl, self.d_poses, self.d_lms,
            d_po, d_lo, d_scale, int(from_records)))
        return dict(xl=c.to_host(d_xl, (L, 3)), scale=c.to_host(d_scale, 1), poses=c.to_host(d_po, (f["Pall"], 7)),
                    lms=c.to_host(d_lo, (f["Lall"], 3)))


def mats(h):
    """the matrices of fetched flat arrays"""
    out = {}
    for k, (r, c) in (("Hpp", (6, 6)), ("Hll", (3, 3)), ("Hpl", (6, 3)), ("T", (6, 3)), ("inv", (3, 3)), ("Hsc", (6, 6))):
        if k in h:
            out[k] = kr.from_colmajor(np.asarray(h[k], np.float64), r, c)
    return out


@functools.lru_cache(maxsize=4)
def references(name, kind):
    _, f, hs = designed.fused_layout(name)
    rk = designed.fused_robust_kernels(name)[kind]
    ref = kr.build(None, rk, f)
    if kind == "tukey":
        zero = float((np.asarray(ref["w"])[(f["flags"] & 8) == 0] == 0).mean())
        assert zero >= 0.1 and 1 - zero >= 0.1
    return f, hs, rk, ref


@functools.lru_cache(maxsize=2)
def end_to_end(name, kind, lam):
    f, hs, rk, ref = references(name, kind)
    return kr.end_to_end_parts(f, hs, lam, ref, rk)


def check_one_stream_build(run, got, plain, ref, lam, tag):
    """contract, stages 1 - 3 of a form 2 build; returns the device's lines (Linv, y; NaN where never written) and G"""
    f, f32 = run.f, run.f32
    L = f["L"]
    has = np.diff(f["lm_ptr"])[:L] > 0
    # contract: written and finite / documented as not written and still NaN
    assert np.all(np.isfinite(got["Hll"])) and np.all(np.isfinite(got["bl"])) and np.all(np.isfinite(got["chi"]))
    assert np.all(np.isfinite(got["T"]))
    for k in ("Hpp", "bp", "Hpl", "inv"):
        assert np.all(np.isnan(got[k])), k + " is documented as not written in form 2"
    if L:
        assert np.all(np.isfinite(got["lmrec"][has, :9])) and np.all(np.isnan(got["lmrec"][~has]))
    else:
        assert np.all(np.isnan(got["lmrec"]))
    # 1. Hll, bl, chi: the owner's sum is the same code
    assert bits_equal(got, plain, ("Hll", "bl", "chi")), "Hll, bl, chi differ from the plain build pass"
    m = mats(got)
    for k, v in (("Hll", m["Hll"]), ("bl", got["bl"]), ("chi", got["chi"][0])):
        bnd = kr.bound(ref[k + "_n"], kr.BUILD_C[k], ref[k + "_mass"])
        assert report(tag, k, kr.ratio(v, ref[k], bnd)) <= 1, k
    # 2. the lines, from the device's own Hll, bl
    Linv, y = kr.lines_from6(got["lmrec"][:L]) if L else (np.zeros((0, 3, 3)), np.zeros((0, 3)))
    st = kr.fused_stage_lines(Linv[has], y[has], m["Hll"][has], got["bl"][has], lam)
    assert report(tag, "lines", st["lines"]) <= 1 and report(tag, "y", st["y"]) <= 1
    # 3. G from the reference Hpl and the device's L^-1
    G = m["T"]
    assert report(tag, "G", kr.fused_stage_G(G, ref, f, Linv, f32)) <= 1
    assert np.all(G[(f["flags"] & 11) != 0] == 0)
    return dict(Linv=Linv, y=y), G


def dead_vertices(f):
    """(free pose all of whose listed edges are INACTIVE, free landmark all of whose slots are INACTIVE real edges)"""
    fl, pp, lp = f["flags"], f["pose_ptr"], f["lm_ptr"]
    ps = [p for p in range(f["P"]) if pp[p + 1] > pp[p] and np.all(fl[f["pose_edge"][pp[p]:pp[p + 1]]] & 8)]
    ls = [l for l in range(f["L"]) if lp[l + 1] > lp[l] and np.all(fl[lp[l]:lp[l + 1]] & 8) and np.all(f["src"][lp[l]:lp[l + 1]] >= 0)]
    return ps, ls


def run_case(monkeypatch, name, kind, f32, lam, forms):
    f, hs, rk, ref = references(name, kind)
    P, L, E = f["P"], f["L"], f["E"]
    dk = np.asarray(hs[0][:P])
    has = np.diff(f["lm_ptr"])[:L] > 0
    tag = "%s %s f32=%d lam=%g" % (name, kind, f32, lam)
    if name == "U":
        xp = designed.pose_update_cases()[1]
        assert len(xp) == P and (np.abs(f["poses"][:P, 3]) < 0.05).sum() >= 2
    else:
        xp = designed.random_blocks(f, seed=12)["xp"]
    runs = {}
    try:
        for form, env in forms.items():
            runs[form] = Run(form_ctx(monkeypatch, env), f, hs, f32, rk)
        main = runs["default"]
        # ---- the one-stream form on the default context, twice (the records live until the plain build below)
        first = None
        for rep in range(2):
            d2, g2 = main.fused_build(lam, 2)
            sch = {damp: main.fused_schur(d2, lam, damp, 2) for damp in (0, 1)}
            d_bp = main.c.to_dev(sch[0]["bp_out"])
            bs = {rec: main.fused_backsubst(d2, d_bp, lam, xp, rec) for rec in (0, 1)}
            if first is None:
                first = (g2, sch, bs)
        g2b, schb, bsb = g2, sch, bs
        g2, sch, bs = first
        assert bits_equal(g2, g2b, ("Hll", "bl", "chi", "T")) and np.array_equal(g2["lmrec"][:, :9], g2b["lmrec"][:, :9], equal_nan=True)
        for damp in (0, 1):
            assert bits_equal(sch[damp], schb[damp], ("Hsc", "bp_out", "bsc")), "a second call gives other bits"
        for rec in (0, 1):
            assert bits_equal(bs[rec], bsb[rec], ("xl", "scale", "poses", "lms")), "a second call gives other bits"
        dp, plain = main.plain_build()
        lines, G = check_one_stream_build(main, g2, plain, ref, lam, tag)
        # ---- 4. Schur complement of the one-stream form
        ps = kr.pose_schur(None, rk, f, lam, lines, ref=ref)
        for damp in (0, 1):
            s = sch[damp]
            assert all(np.all(np.isfinite(s[k])) for k in ("Hsc", "bp_out", "bsc")), "an entry was not written"
            Hsc = kr.from_colmajor(s["Hsc"], 6, 6)
            r = kr.fused_stage_pose(Hsc[dk], s["bp_out"], s["bsc"], ps, damp * lam)
            t = "%s damp=%d" % (tag, damp)
            assert report(t, "diagonal", r["diag"]) <= 1 and report(t, "bp", r["bp"]) <= 1 and report(t, "bsc", r["bsc"]) <= 1
            assert report(t, "off-diagonal", kr.fused_stage_offdiag(Hsc, hs, G, P)) <= 1
        assert np.array_equal(sch[0]["bp_out"], sch[1]["bp_out"]) and np.array_equal(sch[0]["bsc"], sch[1]["bsc"])
        # ---- 7. back-substitution
        b0, b1 = bs[0], bs[1]
        assert bits_equal(b0, b1, ("xl", "scale", "poses", "lms")), "from_records = 1 gives other bits than the G blocks"
        rb = kr.backsubst_lines(f, lam, lines["Linv"], lines["y"], g2["bl"], sch[0]["bp_out"], G, xp, xl=b0["xl"])
        assert report(tag, "xl", kr.ratio(b0["xl"], rb["xl"], kr.bound(rb["xl_n"], kr.C_XL_LINES, rb["xl_mass"]))) <= 1
        assert np.all(b0["xl"][~has] == 0)
        assert np.array_equal(b0["lms"][:L], f["lms"][:L] + b0["xl"]) and np.array_equal(b0["lms"][L:], f["lms"][L:])
        assert np.array_equal(b0["poses"][P:], f["poses"][P:]) and np.all(np.isfinite(b0["poses"][:P]))
        assert report(tag, "scale", kr.ratio(b0["scale"][0], rb["scale"], kr.bound(rb["scale_n"], kr.C_SCALE, rb["scale_mass"]))) <= 1
        if name == "U":
            for i in range(P):
                eq, et = kr.pose_update_error(b0["poses"][i], kr.pose_update(f["poses"][i], xp[i]), f["poses"][i], xp[i])
                assert eq <= kr.KQ and et <= kr.KT, (i, eq, et)
        # ---- the designed special cases
        if name == "F-dead":
            pdead, ldead = dead_vertices(f)
            assert len(pdead) == 1 and len(ldead) == 1
            p, l = pdead[0], ldead[0]
            i = 1.0 / np.sqrt(lam)
            assert np.array_equal(lines["Linv"][l], np.diag([i, i, i])) and np.all(lines["y"][l] == 0)
            assert np.all(b0["xl"][l] == 0) and np.array_equal(b0["lms"][l], f["lms"][l])
            for damp in (0, 1):
                assert np.array_equal(kr.from_colmajor(sch[damp]["Hsc"], 6, 6)[dk[p]], damp * lam * np.eye(6))
                assert np.all(sch[damp]["bp_out"][p] == 0) and np.all(sch[damp]["bsc"][p] == 0)
        if name == "F-allfixed":
            Hd = kr.from_colmajor(sch[0]["Hsc"], 6, 6)[dk]
            Hpp = kr.from_colmajor(plain["Hpp"], 6, 6)
            bnd = kr.bound(ps["Hd_n"], kr.C_PS_H, ps["Hd_mass"]) + kr.bound(ref["Hpp_n"], kr.C_HPP, ref["Hpp_mass"])
            assert report(tag, "diagonal against Hpp", kr.ratio(Hd, Hpp, bnd)) <= 1
        # ---- 6. the two-stream fused form and the unfused call
        d1, g1 = main.fused_build(lam, 1)
        assert bits_equal(g1, plain, ("Hpp", "bp", "Hll", "bl", "Hpl", "chi")), "form 1 differs from the plain build pass"
        un, tw = {}, {}
        for damp in (0, 1):
            tw[damp] = main.fused_schur(d1, lam, damp, 1)
            un[damp] = main.unfused_schur(dp, lam, damp)
            if damp == 0:
                assert np.array_equal(g1["inv"], un[0]["inv"], equal_nan=True), "invHll of form 1 is not k_schur_edges'"
                assert np.array_equal(g1["T"], un[0]["T"]), "T of form 1 is not k_schur_edges'"
                assert np.all(np.isfinite(g1["inv"][has])) and np.all(np.isnan(g1["inv"][~has])) and np.all(np.isfinite(g1["T"]))
            assert bits_equal(tw[damp], un[damp], ("Hsc", "bsc")), "Hsc, bsc of form 1 differ from the unfused call"
            assert np.all(np.isfinite(un[damp]["Hsc"])) and np.all(np.isfinite(un[damp]["bsc"]))
        # ---- the other off-diagonal forms: same build, same pose pass, their own off-diagonal blocks
        one = {"default": sch}
        for form, run in runs.items():
            if form == "default":
                continue
            dd, gg = run.fused_build(lam, 2)
            assert bits_equal(gg, g2, ("Hll", "bl", "chi", "T")) and np.array_equal(gg["lmrec"][:, :9], g2["lmrec"][:, :9], equal_nan=True)
            one[form] = {}
            for damp in (0, 1):
                s = one[form][damp] = run.fused_schur(dd, lam, damp, 2)
                assert np.all(np.isfinite(s["Hsc"])) and bits_equal(s, sch[damp], ("bp_out", "bsc"))
                Hsc = kr.from_colmajor(s["Hsc"], 6, 6)
                assert np.array_equal(Hsc[dk], kr.from_colmajor(sch[damp]["Hsc"], 6, 6)[dk])
                if np.array_equal(s["Hsc"], sch[damp]["Hsc"]):
                    print("%s damp=%d %s: bitwise the Hsc of the default form" % (tag, damp, form))
                else:
                    assert report("%s damp=%d %s" % (tag, damp, form), "off-diagonal", kr.fused_stage_offdiag(Hsc, hs, G, P)) <= 1
        # ---- 5. end to end, and the forms pairwise
        parts = end_to_end(name, kind, lam)
        for damp in (0, 1):
            H1, b1_, bH1, bb1 = kr.end_to_end_bounds(parts, damp, one_stream=True)
            H2, b2_, bH2, bb2 = kr.end_to_end_bounds(parts, damp, one_stream=False)
            if f32:
                (fH1, fb1), (fH2, fb2) = kr.float_storage_bounds(parts, True), kr.float_storage_bounds(parts, False)
                bH1, bb1, bH2, bb2 = bH1 + fH1, bb1 + fb1, bH2 + fH2, bb2 + fb2
            t = "%s damp=%d" % (tag, damp)
            for form in one:
                s = one[form][damp]
                assert report(t + " " + form, "Hsc end to end", kr.ratio(kr.from_colmajor(s["Hsc"], 6, 6), H1, bH1)) <= 1
                assert report(t + " " + form, "bsc end to end", kr.ratio(s["bsc"], b1_, bb1)) <= 1
            Hu = kr.from_colmajor(un[damp]["Hsc"], 6, 6)
            assert report(t + " unfused", "Hsc end to end", kr.ratio(Hu, H2, bH2)) <= 1
            assert report(t + " unfused", "bsc end to end", kr.ratio(un[damp]["bsc"], b2_, bb2)) <= 1
            for form in one:
                Ho = kr.from_colmajor(one[form][damp]["Hsc"], 6, 6)
                assert np.all(np.abs(np.asarray(Ho, LD) - Hu) <= bH1 + bH2), (t, form)
                assert np.all(np.abs(np.asarray(one[form][damp]["bsc"], LD) - un[damp]["bsc"]) <= bb1 + bb2), (t, form)
    finally:
        for run in runs.values():
            run.c.close()


CASES = [(name, 0.5) for name in ("A", "B_plan", "C", "U", "F-dead", "F-allfixed")] + \
        [("F-cond", lam) for lam in designed.F_COND_LAMBDAS]


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("kind", ["none", "huber", "tukey"])
@pytest.mark.parametrize("name,lam", CASES, ids=["%s-lam%g" % c for c in CASES])
def test_fused_iteration(name, lam, kind, f32, monkeypatch):
    run_case(monkeypatch, name, kind, f32, lam, FORMS_ALL if name == "A" else FORMS_FEW)


def test_worst_fractions():
    """(last in the file) the worst fraction of every bound over the cases that ran, for the record"""
    for k in sorted(WORST):
        print("worst %-24s %.3g of the bound" % (k, WORST[k]))
    assert all(v <= 1 for v in WORST.values())


# ------------------------------------------------------------------ entry refusals
def test_entry_refusals_launch_nothing():
    """negative lambda, a straddling layout, null d_lmrec with form 2, from_records without lines: CUGO_ERR_INVALID, and
    every output array still holds its NaNs"""
    _, f, hs = designed.fused_layout("U")
    rk = designed.fused_robust_kernels("U")["none"]
    c = devmem.Ctx()
    try:
        run = Run(c, f, hs, False, rk)
        L_ = cugo.lib()
        d = run.build_arrays()
        args = lambda lam, form, lmrec, ptr: (c.h, C.byref(run.ev), ptr.ctypes.data_as(C.POINTER(C.c_int32)), run.d_poses,
                                              run.d_lms, run.rk, lam, form, d["Hpp"], d["bp"], d["Hll"], d["bl"], d["Hpl"],
                                              d["inv"], d["T"], lmrec, d["chi"])
        assert L_.cugo_construct_quadratic_form_fused(*args(-1.0, 2, d["lmrec"], run.h_lm_ptr)) == -3
        assert L_.cugo_construct_quadratic_form_fused(*args(0.5, 2, None, run.h_lm_ptr)) == -3
        assert L_.cugo_construct_quadratic_form_fused(*args(0.5, 3, d["lmrec"], run.h_lm_ptr)) == -3
        g = devmem.pad_to_groups(designed.layout("B")[2])
        assert designed.straddlers(g)
        run_b = Run.__new__(Run)
        run_b.c, run_b.f, run_b.bt = c, g, np.float64
        run_b.ev = devmem.upload_edges(c, g)
        db = Run.build_arrays(run_b)
        assert L_.cugo_construct_quadratic_form_fused(
            c.h, C.byref(run_b.ev), np.ascontiguousarray(g["lm_ptr"], np.int32).ctypes.data_as(C.POINTER(C.c_int32)),
            c.to_dev(g["poses"]), c.to_dev(g["lms"]), run.rk, 0.5, 2, db["Hpp"], db["bp"], db["Hll"], db["bl"], db["Hpl"],
            db["inv"], db["T"], db["lmrec"], db["chi"]) == -3
        P = f["P"]
        Hsc, bpo, bsc = run.nan(36 * run.B), run.nan(6 * P), run.nan(6 * P)
        assert L_.cugo_compute_schur_fused(c.h, C.byref(run.ev), C.byref(run.hsd), 0.5, 0, 2, run.d_poses, d["Hpp"], d["bp"],
                                           d["Hll"], d["bl"], d["Hpl"], d["inv"], d["T"], None, bpo, bsc, Hsc) == -3
        assert L_.cugo_compute_schur_fused(c.h, C.byref(run.ev), C.byref(run.hsd), -0.5, 0, 2, run.d_poses, d["Hpp"], d["bp"],
                                           d["Hll"], d["bl"], d["Hpl"], d["inv"], d["T"], d["lmrec"], bpo, bsc, Hsc) == -3
        xl = run.nan(3 * f["L"])
        for lam, lmrec in ((0.5, None), (-0.5, d["lmrec"])):
            assert L_.cugo_backsubst_update_fused(c.h, C.byref(run.ev), lam, lmrec, d["bl"], d["bp"], d["T"], d["bp"], xl,
                                                  run.d_poses, run.d_lms, bpo, bsc, Hsc, 1) == -3
        c.sync()
        got = run.fetch_build(d)
        assert all(np.all(np.isnan(v)) for v in got.values())
        assert all(np.all(np.isnan(v)) for v in Run.fetch_build(run_b, db).values())
        assert all(np.all(np.isnan(v)) for v in run.fetch_schur(Hsc, bpo, bsc).values())
        assert np.all(np.isnan(c.to_host(xl, (f["L"], 3))))
    finally:
        c.close()
