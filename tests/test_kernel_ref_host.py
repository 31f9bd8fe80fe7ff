"""CPU checks of tests/kernel_ref.py and tests/designed.py (no GPU): they pin the extended-precision reference, its
per-entry bounds and the designed layouts before test_kernel_shapes.py holds a kernel against them.

* the C oracle (oracle/ba_oracle.c, double, one summation order) and an fp64 run of kernel_ref itself lie inside the
  bounds of the longdouble reference on layouts A, B, C: the reference passes its own bar;
* the bounds see a subtle error: a dropped edge, a dropped product, a transposed block, a lambda off the diagonal each
  break a bound by more than 1000 x;
* the constants of the two tolerances that are measured, not derived (kernel_ref.K_INV, KQ, KT: 4 x what the oracle
  reaches against the reference) are measured here.

Measured where this was written (x86-64, 80-bit longdouble: eps 1.08e-19), largest error / bound per output:
  oracle build pass, kernels none / Huber / Tukey:  Hpp 0.025, bp 0.0038, Hll 0.014, bl 0.0024, Hpl 0.037, chi 5.2e-4
  (in u mass, on the 1025-edge pose of layout A: Hpp 17.1, bp 0.033, against bounds of (1025 + 131) and (1025 + 112))
  oracle Schur complement and landmark step (own inverse and T):  Hsc 0.26, bsc 0.083, xl 0.0093
  ba_sym3_inv against the longdouble inverse: 4.99 u kappa max|inv|     -> kernel_ref.K_INV = 20
  oracle.pose_update: quaternion 2.41 u, translation 5.07 x its base   -> kernel_ref.KQ = 10, KT = 21
"""
import numpy as np
import pytest

import designed
import devmem
import kernel_ref as kr
import oracle

LAYOUTS = ("A", "B", "C")
LAM = 3.7


def oracle_build(prob, f):
    """the oracle's build_system() as matrices in the flattened order"""
    o = prob.build_system()
    return dict(Hpp=kr.from_colmajor(o["Hpp"], 6, 6), bp=o["bp"], Hll=kr.from_colmajor(o["Hll"], 3, 3), bl=o["bl"],
                Hpl=kr.from_colmajor(o["Hpl"][f["src"]], 6, 3), chi=o["chi"])


@pytest.mark.parametrize("name", ["A", "B", "C", "B_plan", "U"])
def test_layouts_are_legal_and_as_designed(name):
    d, prob, f, hs = designed.layout(name)   # asserts check_geometry, check_layout and check_named
    designed.check_layout(f)
    designed.check_named(name, d, f, hs)
    if name in ("A", "B_plan"):
        g = devmem.pad_to_groups(f)
        designed.check_layout(g)
        assert not [l for l in designed.straddlers(g) if np.diff(g["lm_ptr"])[l] <= 256]
    if name == "B":                      # the engine's padding cannot help a landmark of more than 256 edges
        g = devmem.pad_to_groups(f)
        designed.check_layout(g)
        assert designed.straddlers(g)


def test_graph_layout_keeps_the_long_poses():
    d = designed.graph_d()
    deg = np.bincount(d["e_pose"], minlength=len(d["pose"]))
    assert deg.max() == 1025 and 705 in deg and deg.min() >= 6


@pytest.mark.parametrize("kind", ["none", "huber", "tukey"])
@pytest.mark.parametrize("name", LAYOUTS)
def test_oracle_and_fp64_reference_build_inside_bounds(name, kind):
    _, prob0, f, _ = designed.layout(name)
    rk = designed.robust_kernels(name)[kind]
    prob = prob0.copy()
    prob.rk_type, prob.rk_delta = rk
    ref = kr.build(prob, rk, f)
    if kind == "tukey":
        zero = float((np.asarray(ref["w"]) == 0).mean())
        assert zero >= 0.1 and 1 - zero >= 0.1
    got = oracle_build(prob, f)
    r64 = kr.build(prob, rk, f, dtype=np.float64)
    for k in ("Hpp", "bp", "Hll", "bl", "Hpl", "chi"):
        bnd = kr.bound(ref[k + "_n"], kr.BUILD_C[k], ref[k + "_mass"])
        ro, rr = kr.ratio(got[k], ref[k], bnd), kr.ratio(r64[k], ref[k], bnd)
        print("%s %s %-3s oracle %.3g  fp64 reference %.3g of the bound" % (name, kind, k, ro, rr))
        assert ro <= 1 and rr <= 1, (k, ro, rr)
    # nothing contributes: exact zeros in the reference (and, through ratio(), in the oracle)
    deg = np.diff(f["pose_ptr"])[:f["P"]]
    assert np.all(np.asarray(ref["Hpp"])[deg == 0] == 0) and np.all(np.asarray(ref["Hpp_mass"])[deg == 0] == 0)
    lmdeg = np.diff(f["lm_ptr"])[:f["L"]]
    assert np.all(np.asarray(ref["Hll_mass"])[lmdeg == 0] == 0)
    assert np.all(np.asarray(ref["Hpl_mass"])[(f["flags"] & 3) != 0] == 0)


def own_T_bounds(s, lam, damp, Hpp, bp, float_T=False):
    """bounds of Hsc / bsc for an implementation that forms its own inverse and its own T = Hpl inv from the same
    arrays: (n + c + 4) u (|Hpp| + lambda + sum |Hpl| |inv| |Hpl|^T) + K_INV u imass; the 4 is the 3-term sum of T
    (kernel_ref C_T + 3); float_T: T stored as float, 2^-24 of the product mass more"""
    eye = np.zeros_like(s["Hsc_mass"])
    if damp:
        eye[s["diag"]] = abs(lam) * np.eye(6)
    hpp = np.zeros_like(s["Hsc_mass"])
    hpp[s["diag"]] = np.abs(Hpp)
    bH = kr.bound(s["Hsc_n"], kr.C_HSC + 4, hpp + eye + s["Hsc_Tmass"]) + kr.K_INV * kr.U * s["Hsc_imass"]
    bb = kr.bound(s["bsc_n"], kr.C_BSC + 4, np.abs(bp) + s["bsc_Tmass"]) + kr.K_INV * kr.U * s["bsc_imass"]
    if float_T:
        bH = bH + 2.0 ** -24 * s["Hsc_Tmass"]
        bb = bb + 2.0 ** -24 * s["bsc_Tmass"]
    return bH, bb


def dense_from_blocks(H, rowptr, colind, P):
    D = np.zeros((6 * P, 6 * P), H.dtype)
    for r in range(P):
        for k in range(rowptr[r], rowptr[r + 1]):
            c = colind[k]
            D[6 * r:6 * r + 6, 6 * c:6 * c + 6] = H[k]
            if c != r:
                D[6 * c:6 * c + 6, 6 * r:6 * r + 6] = H[k].T
    return D


@pytest.mark.parametrize("name", LAYOUTS)
def test_oracle_schur_and_landmark_step_inside_bounds(name):
    """schur_dense and solve_step of the oracle, which form their own inverse and T, against kernel_ref.schur /
    backsubst evaluated in longdouble from the ORACLE's fp64 build arrays (so that only the Schur arithmetic differs)"""
    _, prob, f, hs = designed.layout(name)
    o = oracle_build(prob, f)
    P = f["P"]
    for dt in (kr.LD, np.float64):
        s = kr.schur(f, hs, LAM, 1, o["Hpp"], o["bp"], o["Hll"], o["bl"], o["Hpl"], dtype=dt)
        if dt is kr.LD:
            ref = s
            ref["diag"] = np.asarray(hs[0][:P])
            bH, bb = own_T_bounds(ref, LAM, 1, o["Hpp"], o["bp"])
            Hd, bd = prob.schur_dense(LAM)
            rH = kr.ratio(Hd, dense_from_blocks(ref["Hsc"], hs[0], hs[1], P), dense_from_blocks(bH, hs[0], hs[1], P))
            rb = kr.ratio(bd.reshape(P, 6), ref["bsc"], bb)
            print("%s oracle Hsc %.3g bsc %.3g of the bound" % (name, rH, rb))
        else:
            rH, rb = kr.ratio(s["Hsc"], ref["Hsc"], bH), kr.ratio(s["bsc"], ref["bsc"], bb)
            print("%s fp64 reference Hsc %.3g bsc %.3g of the bound" % (name, rH, rb))
        assert rH <= 1 and rb <= 1
    ok, dxp, dxl = prob.solve_step(LAM, dense=True)
    assert ok
    b = kr.backsubst(f, LAM, ref["inv"], o["bl"], o["bp"], o["Hpl"], dxp, kappa=ref["kappa"])
    bx = kr.bound(b["xl_n"], kr.C_XL, b["xl_mass"]) + kr.K_INV * kr.U * b["xl_imass"]
    rx = kr.ratio(dxl, b["xl"], bx)
    b64 = kr.backsubst(f, LAM, np.asarray(ref["inv"], np.float64), o["bl"], o["bp"], o["Hpl"], dxp, dtype=np.float64)
    r64 = kr.ratio(b64["xl"], b["xl"], bx)
    print("%s xl: oracle %.3g, fp64 reference %.3g of the bound" % (name, rx, r64))
    assert rx <= 1 and r64 <= 1
    lmdeg = np.diff(f["lm_ptr"])[:f["L"]]
    assert np.all(dxl[lmdeg == 0] == 0)


def test_inverse_constant():
    """K_INV: the oracle's ba_sym3_inv (the adjugate formula in C double) against the longdouble inverse, on the
    matrices test_kernel_shapes supplies (designed.random_blocks of A, B, C with lambda 0.5 and 300), in units of
    u kappa max|inv|; kernel_ref.K_INV is 4 x the largest ratio, rounded up"""
    worst = 0.0
    for name in LAYOUTS:
        f = designed.layout(name)[2]
        Hll = designed.random_blocks(f, seed=11)["Hll"]
        for lam in (0.5, 300.0):
            A = Hll + lam * np.eye(3)
            ref = kr.inv3(np.asarray(A, kr.LD))
            kap = np.linalg.cond(A)
            got = np.array([oracle.sym3_inv(a) for a in A])
            r = np.abs(got - ref).reshape(len(A), -1).max(1) / (kr.U * kap * np.abs(ref).reshape(len(A), -1).max(1))
            worst = max(worst, float(r.max()))
    print("ba_sym3_inv: %.3g u kappa max|inv|" % worst)
    assert 4 * worst <= kr.K_INV


def test_pose_update_oracle_vs_reference():
    """KQ, KT: oracle.pose_update against kernel_ref.pose_update on the case list of the GPU test"""
    poses, dxs = designed.pose_update_cases()
    wq = wt = 0.0
    for p, dx in zip(poses, dxs):
        got = oracle.pose_update(p, dx)
        ref = kr.pose_update(p, dx)
        assert abs(float((ref[:4] ** 2).sum()) - 1) < 1e-17 and ref[3] >= 0
        eq, et = kr.pose_update_error(got, ref, p, dx)
        wq, wt = max(wq, eq), max(wt, et)
        # the fp64 run of the reference itself
        eq64, et64 = kr.pose_update_error(kr.pose_update(p, dx, dtype=np.float64), ref, p, dx)
        assert eq64 <= kr.KQ and et64 <= kr.KT, (dx, eq64, et64)
    print("oracle.pose_update: quaternion %.3g u, translation %.3g x base" % (wq, wt))
    assert 4 * wq <= kr.KQ and 4 * wt <= kr.KT


# ------------------------------------------------------------------ the bounds see a subtle error
@pytest.fixture(scope="module")
def schur_A():
    _, prob, f, hs = designed.layout("A")
    blk = designed.random_blocks(f, seed=11)
    s = kr.schur(f, hs, 0.5, 1, blk["Hpp"], blk["bp"], blk["Hll"], blk["bl"], blk["Hpl"])
    bH = kr.bound(s["Hsc_n"], kr.C_HSC, s["Hsc_mass"])
    return f, hs, blk, s, bH


@pytest.mark.parametrize("degree", [225, 513, 1025])
def test_bounds_see_a_dropped_last_edge(degree, schur_A):
    f, hs, blk, s, bH = schur_A
    _, prob, _, _ = designed.layout("A")
    p = int(np.flatnonzero(np.diff(f["pose_ptr"])[:f["P"]] == degree)[0])
    last = int(f["pose_edge"][f["pose_ptr"][p + 1] - 1])
    # build pass: Hpp and bp of the pose without its last edge
    ref = kr.build(prob, (0, 1.0), f)
    g = dict(f)
    g["flags"] = f["flags"].copy()
    g["flags"][last] |= 8
    mut = kr.build(prob, (0, 1.0), g)
    for k in ("Hpp", "bp"):
        assert kr.ratio(mut[k][p], ref[k][p], kr.bound(ref[k + "_n"], kr.BUILD_C[k], ref[k + "_mass"])[p]) > 1000
    # Schur complement: the diagonal block and bsc without the last edge's product (a free-free edge)
    if f["flags"][last] & 3:
        last = int([e for e in f["pose_edge"][f["pose_ptr"][p]:f["pose_ptr"][p + 1]] if not f["flags"][e] & 3][-1])
    T = np.array(s["T"])
    T[last] = 0
    m = kr.schur(f, hs, 0.5, 1, blk["Hpp"], blk["bp"], blk["Hll"], blk["bl"], blk["Hpl"], T=T)
    k = hs[0][p]
    assert kr.ratio(m["Hsc"][k], s["Hsc"][k], bH[k]) > 1000
    assert kr.ratio(m["bsc"][p], s["bsc"][p], kr.bound(s["bsc_n"], kr.C_BSC, s["bsc_mass"])[p]) > 1000


def test_bounds_see_a_dropped_product_a_transposed_block_and_a_stray_lambda(schur_A):
    f, hs, blk, s, bH = schur_A
    rowptr, colind, off_ptr, ei, ej = hs
    n = np.diff(off_ptr)
    k = int(np.flatnonzero((n % 14 == 1) & (n > 14))[0]) if np.any((n % 14 == 1) & (n > 14)) else int(np.flatnonzero(n % 14 == 1)[0])
    keep = np.ones(len(ei), bool)
    keep[off_ptr[k + 1] - 1] = False
    op = off_ptr.copy()
    op[k + 1:] -= 1
    m = kr.schur(f, (rowptr, colind, op, ei[keep], ej[keep]), 0.5, 1, blk["Hpp"], blk["bp"], blk["Hll"], blk["bl"], blk["Hpl"])
    assert kr.ratio(m["Hsc"][k], s["Hsc"][k], bH[k]) > 1000
    H = np.array(s["Hsc"])
    assert kr.ratio(H[k].T, s["Hsc"][k], bH[k]) > 1000            # (r, c) swapped
    d = int(rowptr[3])
    stray = H[d].copy()
    stray[0, 1] += 0.5                                            # lambda off the diagonal
    assert kr.ratio(stray, s["Hsc"][d], bH[d]) > 1000
    undamped = kr.schur(f, hs, 0.5, 0, blk["Hpp"], blk["bp"], blk["Hll"], blk["bl"], blk["Hpl"])
    assert kr.ratio(undamped["Hsc"][d], s["Hsc"][d], bH[d]) > 1000
