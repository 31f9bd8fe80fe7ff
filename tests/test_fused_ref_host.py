"""CPU tests of the references of the fused iteration (kernel_ref: fused_lines, fused_G, pose_schur, backsubst_lines) and
of the bounds test_fused_shapes.py holds the device to.  No GPU, no product code.

1. The float64 REPLAY of the device's operations (kernel_ref.replay_*: the 3 x 3 factorisation of k_build_edges, its G
   block, every edge term of k_pose_schur) stays inside every bound of the staged comparison, on every layout of
   designed.fused_layout, with every robust kernel; the worst fraction of each bound is printed.  K_CHOL is measured
   here: the worst error of the replayed L^-1 in u kappa max|L^-1| is printed, and kernel_ref.K_CHOL must be 4 x that
   (rounded up), the margin of K_INV, KQ, KT.  The C oracle inverts Hll by the adjugate and has no 3 x 3 Cholesky
   factorisation to measure next to it.
2. Longdouble identities tie the new reference to the old one (kernel_ref.schur / backsubst):
       G G^T = T Hpl^T,   sum JP^T N JP = Hpp - sum T Hpl^T,   L^-T (y - sum G^T x) = inv (bl - sum Hpl^T x)
   to 1e-17 (about 100 longdouble roundings) relative to the entry's mass for the sums over a pose's edges (whose mass
   holds the uncancelled w JP^T JP).  The per-slot and per-landmark identities compare two routes to the inverse of
   Hll + lam I entry by entry, and each route carries kappa roundings: there the tolerance is 1e-17 kappa mass with the
   landmark's own kappa (a few thousand at most on these layouts at lambda = 0.5).
3. Mutations of the replay — each a mistake a kernel could make — are seen by at least one stage at 10 x its bound.
"""
import functools

import numpy as np
import pytest

import designed
import kernel_ref as kr

LD, U = kr.LD, kr.U
LAYOUTS = ("A", "B_plan", "C", "U", "F-dead", "F-allfixed", "F-cond")


def lambdas(name):
    return designed.F_COND_LAMBDAS if name == "F-cond" else (0.5,)


@functools.lru_cache(maxsize=None)
def builds(name, kind):
    _, f, hs = designed.fused_layout(name)
    rk = designed.fused_robust_kernels(name)[kind]
    return f, hs, rk, kr.build(None, rk, f), kr.build(None, rk, f, dtype=np.float64)


def replay_case(name, kind, lam, f32=False, mut=None):
    """the stages of test_fused_shapes.py with the float64 replay in the device's place: {quantity: fraction of its bound}"""
    f, hs, rk, ref, ref64 = builds(name, kind)
    P, L = f["P"], f["L"]
    Hll, bl = np.asarray(ref64["Hll"], np.float64), np.asarray(ref64["bl"], np.float64)
    has = np.diff(f["lm_ptr"])[:L] > 0
    rl = kr.replay_lines(Hll, bl, lam, mut)
    out = {}
    st = kr.fused_stage_lines(rl["Linv"][has], rl["y"][has], Hll[has], bl[has], lam)
    out["lines"], out["y"], out["raw"] = st["lines"], st["y"], st["raw"]
    # as the device leaves them: the line of a landmark without any slot is never written
    lines = dict(Linv=np.where(has[:, None, None], rl["Linv"], np.nan), y=np.where(has[:, None], rl["y"], np.nan))
    act, Li, _ = kr._per_edge_lines(f, lines["Linv"], lines["y"], np.float64)
    G = kr.replay_G(ref64["Hpl"], Li, act, f32, mut)
    out["G"] = kr.fused_stage_G(G, ref, f, lines["Linv"], f32)
    out["offdiag"] = kr.fused_stage_offdiag(kr.offdiag_from_G(hs, G, np.float64)[0], hs, G, P)
    if mut == "inactive_times_zero":      # what the landmark lines hold where nobody wrote them
        lines = dict(Linv=np.full((max(L, 1), 3, 3), np.nan), y=np.full((max(L, 1), 3), np.nan)) if L == 0 else lines
    ps = kr.pose_schur(None, rk, f, lam, lines, ref=ref)
    rp = kr.replay_pose_schur(f, ref64, lines, mut)
    out.update(kr.fused_stage_pose(rp["Hd"], rp["bp"], rp["bsc"], ps))
    xp = designed.random_blocks(f, seed=12)["xp"]
    x64 = kr.backsubst_lines(f, lam, lines["Linv"], lines["y"], bl, rp["bp"], G, xp, dtype=np.float64)
    bs = kr.backsubst_lines(f, lam, lines["Linv"], lines["y"], bl, rp["bp"], G, xp, xl=x64["xl"])
    out["xl"] = kr.ratio(x64["xl"], bs["xl"], kr.bound(bs["xl_n"], kr.C_XL_LINES, bs["xl_mass"]))
    out["scale"] = kr.ratio(x64["scale"], bs["scale"], kr.bound(bs["scale_n"], kr.C_SCALE, bs["scale_mass"]))
    return out


def test_float64_replay_stays_inside_every_bound():
    worst = {}
    for name in LAYOUTS:
        for kind in ("none", "huber", "tukey"):
            for lam in lambdas(name):
                for f32 in (False, True):
                    r = replay_case(name, kind, lam, f32)
                    for k, v in r.items():
                        k = "G (float storage)" if (k == "G" and f32) else k
                        worst[k] = max(worst.get(k, 0.0), v)
                    assert all(v <= 1 for k, v in r.items() if k != "raw"), (name, kind, lam, f32, r)
    for k in ("lines", "y", "G", "G (float storage)", "offdiag", "diag", "bp", "bsc", "xl", "scale"):
        print("float64 replay: %-17s %.3g of the bound" % (k, worst[k]))
    raw = worst["raw"]
    print("float64 replay: L^-1 error %.3g u kappa max|L^-1|  ->  K_CHOL = 4 x = %.3g (kernel_ref.K_CHOL = %g)"
          % (raw, 4 * raw, kr.K_CHOL))
    assert 4 * raw <= kr.K_CHOL <= 4 * raw + 1, "K_CHOL is 4 x the measured figure, rounded up"


@pytest.mark.parametrize("name", ["A", "B_plan", "C", "U", "F-dead"])
def test_longdouble_identities(name):
    f, hs, rk, ref, _ = builds(name, "huber")
    lam = 0.5
    P, L = f["P"], f["L"]
    ln = kr.fused_lines(ref["Hll"], ref["bl"], lam)
    act, Li, ye = kr._per_edge_lines(f, ln["Linv"], ln["y"], LD)
    G, _ = kr.fused_G(ref["Hpl"], Li)
    s = kr.schur(f, hs, lam, 0, ref["Hpp"], ref["bp"], ref["Hll"], ref["bl"], ref["Hpl"], want=())
    kap = np.asarray(ln["kappa"], LD)
    kap_e = np.where(act, kap[np.where(act, f["lm"], 0)], 1)
    tol = LD(1e-17)
    aH = np.abs(ref["Hpl"])
    # G G^T = T Hpl^T, slot by slot
    lhs = np.einsum("erm,ecm->erc", G, G)
    rhs = np.einsum("erm,ecm->erc", s["T"], ref["Hpl"])
    mass = np.einsum("erm,ecm->erc", s["T_mass"], aH)
    r1 = kr.ratio(lhs, rhs, tol * kap_e[:, None, None] * mass)
    # sum JP^T N JP = Hpp - sum T Hpl^T (the diagonal blocks), and its right-hand sides
    ps = kr.pose_schur(None, rk, f, lam, ln, ref=ref)
    dk = np.asarray(hs[0][:P])
    r2 = kr.ratio(ps["Hd"], s["Hsc"][dk], tol * ps["Hd_mass"])
    r3 = kr.ratio(ps["bsc"], s["bsc"], tol * ps["bsc_mass"])
    r4 = kr.ratio(ps["bp"], ref["bp"], tol * ps["bp_mass"])
    # L^-T (y - sum G^T x) = inv (bl - sum Hpl^T x)
    xp = designed.random_blocks(f, seed=12)["xp"]
    a = kr.backsubst_lines(f, lam, ln["Linv"], ln["y"], ref["bl"], ref["bp"], G, xp)
    b = kr.backsubst(f, lam, s["inv"], ref["bl"], ref["bp"], ref["Hpl"], xp)
    has = np.diff(f["lm_ptr"])[:L] > 0
    r5 = kr.ratio(a["xl"][has], b["xl"][has], (tol * kap[:, None] * b["xl_mass"])[has])
    print("%s: diagonal %.3g, bsc %.3g, bp %.3g of 1e-17 mass; G G^T %.3g, xl %.3g of 1e-17 kappa mass (kappa <= %.3g)"
          % (name, r2, r3, r4, r1, r5, float(kap.max())))
    assert max(r1, r2, r3, r4, r5) <= 1
    assert r1 > 0 or not act.any()          # (the identity is not an identity of the code: two routes)


# (mutation, layout, robust kernel, the quantities that must see it)
MUTATIONS = [("swap_20_21", "A", "none", ("lines",)),
             ("i20_without_l21_i10", "A", "none", ("lines",)),
             ("y_is_bl", "A", "none", ("y",)),
             ("G_with_Linv", "A", "none", ("G",)),
             ("N_without_w2", "A", "huber", ("diag",)),
             ("u_with_plus", "A", "none", ("bsc",)),
             ("drop_last_lane", "A", "none", ("diag", "bp", "bsc")),
             ("inactive_times_zero", "F-allfixed", "none", ("diag", "bsc")),
             ("mono_third_row", "A", "none", ("diag", "bsc")),      # (bp: e[2] = 0 on a mono edge)
             ("lm_from_slot0", "A", "none", ("diag", "bsc"))]


@pytest.mark.parametrize("mut,name,kind,seen_by", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_mutations_of_the_replay_are_seen(mut, name, kind, seen_by):
    good = replay_case(name, kind, 0.5)
    bad = replay_case(name, kind, 0.5, mut=mut)
    assert all(v <= 1 for k, v in good.items() if k != "raw")
    for k in seen_by:
        print("mutation %-22s %-6s %.3g x its bound (unmutated %.3g)" % (mut, k, bad[k], good[k]))
        assert bad[k] >= 10, (mut, k, bad[k])


def test_entry_refusals_need_no_device():
    """the fused entries check their arguments before they touch the context: negative lambda, a layout with a landmark in
    two 256-slot groups, form 2 without d_lmrec, from_records without the lines — each CUGO_ERR_INVALID, here with a
    null context and pointers that are never followed (test_fused_shapes.py repeats them on a device and checks that
    nothing was written)"""
    import ctypes as C
    import importlib
    import devmem
    cugo = importlib.import_module("cuda-bundle-adjustment_amd")
    L_ = cugo.lib()
    _, f, hs = designed.fused_layout("U")
    ev = cugo.Edges()
    ev.n_edges, ev.n_poses_total, ev.n_landmarks_total = f["E"], f["Pall"], f["Lall"]
    ev.n_poses_free, ev.n_landmarks_free = f["P"], f["L"]
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    ok_ptr = np.ascontiguousarray(f["lm_ptr"], np.int32)
    rk = cugo.Robust(0, 1.0, 0, 1.0)
    p = C.c_void_p(64)                  # "a pointer": non-null, never followed
    build = lambda lam, form, lmrec, lp, e=ev: L_.cugo_construct_quadratic_form_fused(
        None, C.byref(e), ptr(lp), p, p, rk, lam, form, p, p, p, p, p, p, p, lmrec, p)
    assert build(-1.0, 2, p, ok_ptr) == -3 and b"lambda" in L_.cugo_last_error()
    assert build(float("nan"), 2, p, ok_ptr) == -3
    assert build(0.5, 2, None, ok_ptr) == -3 and b"d_lmrec" in L_.cugo_last_error()
    assert build(0.5, 0, p, ok_ptr) == -3
    g = devmem.pad_to_groups(designed.layout("B")[2])     # keeps landmarks of 257 and 300 edges
    assert designed.straddlers(g)
    evb = cugo.Edges()
    evb.n_edges, evb.n_poses_total, evb.n_landmarks_total = g["E"], g["Pall"], g["Lall"]
    evb.n_poses_free, evb.n_landmarks_free = g["P"], g["L"]
    assert build(0.5, 2, p, np.ascontiguousarray(g["lm_ptr"], np.int32), evb) == -3 and b"two 256-slot groups" in L_.cugo_last_error()
    assert build(0.5, 1, p, np.ascontiguousarray(g["lm_ptr"], np.int32), evb) == -3
    # with every argument in order the only thing left to refuse is the null context: nothing else was wrong
    assert build(0.5, 2, p, ok_ptr) == -3 and b"null context" in L_.cugo_last_error()
    hsd = cugo.HscStruct()
    hsd.d_rowptr = 64
    schur = lambda lam, form, lmrec: L_.cugo_compute_schur_fused(None, C.byref(ev), C.byref(hsd), lam, 0, form, p, p, p, p, p,
                                                                 p, p, p, lmrec, p, p, p)
    assert schur(-0.5, 2, p) == -3 and schur(0.5, 2, None) == -3 and schur(0.5, 5, p) == -3
    assert schur(0.5, 2, p) == -3 and b"null context" in L_.cugo_last_error()
    back = lambda lam, lmrec, rec: L_.cugo_backsubst_update_fused(None, C.byref(ev), lam, lmrec, p, p, p, p, p, p, p, p, p, p, rec)
    assert back(0.5, None, 1) == -3 and b"from_records without" in L_.cugo_last_error()
    assert back(0.5, None, 0) == -3 and back(-0.5, p, 0) == -3
    assert back(0.5, p, 1) == -3 and b"null context" in L_.cugo_last_error()
