"""CPU tests of the distortion reference (tests/distort_ref.py) and of the designed distortion tables
(tests/distort_designed.py): a known answer in exact rationals, the Jacobians against five-point central differences in
longdouble at every hand-placed point, a plain float64 evaluation inside the per-entry bounds on every pattern, each of
the plausible mistakes outside them, and the all-undistorted table against rig_ref.build."""
import functools
from fractions import Fraction as Fr

import numpy as np
import pytest

import distort_designed as dd
import distort_ref as dr
import kernel_ref as kr
import rig_ref as rr

LD = kr.LD
NONE2 = dict(mono=(0, 1.0), stereo=(0, 1.0))


@functools.lru_cache(maxsize=None)
def reference(design, pattern, fused=False):
    f, hs = dd.case(design, pattern, fused)
    rk2 = dd.robust2(design, 0, fused)
    return f, hs, rk2, dr.build(f, rk2)


@functools.lru_cache(maxsize=None)
def hand_reference():
    f, hs = dd.hand_points()
    return f, hs, dr.build(f, NONE2)


def rational_answer(cam4, d5, Xs):
    """(r2, rad, pu, pv, dpu/dXs, dpv/dXs) in exact rationals, from the formulas of the term"""
    fx, fy, cx, cy = cam4
    k1, k2, p1, p2, k3 = d5
    x, y, z = Xs
    iz = 1 / z
    a, b = x * iz, y * iz
    r2 = a * a + b * b
    rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    drad = k1 + r2 * (2 * k2 + 3 * k3 * r2)
    ad = a * rad + 2 * p1 * a * b + p2 * (r2 + 2 * a * a)
    bd = b * rad + p1 * (r2 + 2 * b * b) + 2 * p2 * a * b
    Jaa = rad + 2 * a * a * drad + 2 * p1 * b + 6 * p2 * a
    Jab = 2 * a * b * drad + 2 * p1 * a + 2 * p2 * b
    Jbb = rad + 2 * b * b * drad + 6 * p1 * b + 2 * p2 * a
    du = [fx * iz * Jaa, fx * iz * Jab, -fx * iz * (Jaa * a + Jab * b)]
    dv = [fy * iz * Jab, fy * iz * Jbb, -fy * iz * (Jab * a + Jbb * b)]
    return r2, rad, fx * ad + cx, fy * bd + cy, du, dv


def test_known_answer_in_exact_rationals():
    cam4 = [Fr(v) for v in (500, 480, 320, 240)]
    d5 = [Fr(s) for s in ("-0.28", "0.07", "0.002", "-0.001", "-0.01")]
    Xs = [Fr(s) for s in ("0.3", "-0.2", "2")]
    r2, rad, pu, pv, du, dv = rational_answer(cam4, d5, Xs)
    assert r2 == Fr("0.0325") and rad == Fr("0.99097359421875")
    # (the digits DESIGN.md section 20 quotes; the comparisons below are against the rationals, not against these)
    assert abs(float(pu) - 394.25426956640626) < 1e-12 and abs(float(pv) - 192.4980674775) < 1e-12
    for got, want in zip(du + dv, (244.3192295703125, 2.26611265625, -36.421273169921875, 2.17546815, 236.1513505125, 23.28881482875)):
        assert abs(float(got) - want) <= 1e-12 * abs(want)
    # the reference's functions at the same point, longdouble against the rationals
    as_ld = lambda v: LD(v.numerator) / LD(v.denominator)
    X = np.array([[as_ld(v) for v in Xs]], LD)
    D = np.array([[as_ld(v) for v in d5]], LD)
    A, _, (ad, bd), _ = dr.dist_A(X, np.array([LD(500)]), np.array([LD(480)]), D, LD)
    eps = LD(np.finfo(LD).eps)
    tol = 64 * eps
    assert abs(LD(500) * ad[0] + LD(320) - as_ld(pu)) <= tol * as_ld(pu)
    assert abs(LD(480) * bd[0] + LD(240) - as_ld(pv)) <= tol * as_ld(pv)
    for j in range(3):
        assert abs(-A[0, 0, j] - as_ld(du[j])) <= tol * abs(as_ld(du[0])), j
        assert abs(-A[0, 1, j] - as_ld(dv[j])) <= tol * abs(as_ld(dv[1])), j
    assert np.all(A[0, 2] == 0)
    # and through build(): the hand-placed point "r2 = 0.0325" on entry 0 carries these inputs
    f, hs, ref = hand_reference()
    i = int(np.flatnonzero((f["lm"] == dd.HAND_NAMES.index("r2 = 0.0325")) & (f["cam_id"] == 0))[0])
    assert np.array_equal(f["cams"][0, :4], [500, 480, 320, 240]) and np.array_equal(f["cam_tab"][0, 12:17], dd.D_TYP)
    # (float64 inputs: 0.3, -0.2 and the coefficients are the nearest doubles, so 2^-50 of the entries, not of longdouble)
    for j in range(3):
        assert abs(-ref["A"][i, 0, j] - as_ld(du[j])) <= 2.0 ** -48 * abs(as_ld(du[0]))
        assert abs(-ref["A"][i, 1, j] - as_ld(dv[j])) <= 2.0 ** -48 * abs(as_ld(dv[1]))
    assert np.array_equal(ref["JL"][i], ref["A"][i])


def central_differences(f, ref, h):
    """largest |numerical - analytic| entry of JP and of JL per slot, each relative to the slot's largest entry of
    that Jacobian.  Central differences on the five-point stencil (f(-2h), f(-h), f(h), f(2h)): truncation
    h^4 |e^(5)| / 30"""
    E = f["E"]

    def residuals(poses, lms):
        return dr.build(dict(f, poses=poses, lms=lms), NONE2)["e"]

    base_p, base_l = np.asarray(f["poses"], LD), np.asarray(f["lms"], LD)
    err_p, err_l = np.zeros(E, LD), np.zeros(E, LD)
    for p in range(f["Pall"]):
        on = f["pose"] == p
        for k in range(6):
            d = np.zeros(6, LD); d[k] = h

            def at(m):
                q = base_p.copy()
                q[p] = kr.pose_update(base_p[p], m * d)
                return residuals(q, base_l)
            num = -(8 * (at(1) - at(-1)) - (at(2) - at(-2))) / (12 * h)                # the arrays hold -de/d.
            err_p[on] = np.maximum(err_p[on], np.abs(num[on] - ref["JP"][on][:, :, k]).max(1))
    for l in range(f["Lall"]):
        on = f["lm"] == l
        for k in range(3):
            def at(m):
                x = base_l.copy()
                x[l, k] += m * h
                return residuals(base_p, x)
            num = -(8 * (at(1) - at(-1)) - (at(2) - at(-2))) / (12 * h)
            err_l[on] = np.maximum(err_l[on], np.abs(num[on] - ref["JL"][on][:, :, k]).max(1))
    sp = np.abs(np.asarray(ref["JP"], LD)).reshape(E, -1).max(1)
    sl = np.abs(np.asarray(ref["JL"], LD)).reshape(E, -1).max(1)
    return err_p / sp, err_l / sl


def test_jacobians_against_central_differences_at_every_hand_placed_point():
    """Held to 2e-12 of the slot's largest entry.  With the identity poses and sensor poses of the hand-placed points
    JL = A, so this is the check of A.  h = 1e-5 times the point's depth: the rounding of the residual (u_LD x 2000 px)
    over h is ~2e-11 px at the nearest point (0.25 m), ~1e-14 of its entries of order 2000; the truncation
    h^4 |e^(5)| / 30 of a polynomial of degree 7 in (a, b) = (x, y) / z stays below that"""
    f, hs, ref = hand_reference()
    worst_p, worst_l = np.zeros(f["E"], LD), np.zeros(f["E"], LD)
    depth = f["lms"][f["lm"], 2]
    for zd in np.unique(f["lms"][:, 2]):
        rp, rl = central_differences(f, ref, LD(1e-5) * LD(zd))
        on = depth == zd
        worst_p[on], worst_l[on] = rp[on], rl[on]
    for i in range(f["E"]):
        print("%-24s %-16s JP %.3g   JL %.3g of the slot's largest entry" % (dd.HAND_NAMES[f["lm"][i]],
                                                                            dd.HAND_ENTRIES[f["cam_id"][i]][0], worst_p[i], worst_l[i]))
    assert worst_p.max() <= 2e-12 and worst_l.max() <= 2e-12


def test_float64_evaluation_of_the_hand_placed_points_is_inside_the_bounds():
    f, hs, ref = hand_reference()
    got = dr.build(f, NONE2, dtype=np.float64)
    r = dr.ratios(got, ref)
    print({k: "%.3g" % v for k, v in r.items()})
    assert max(r.values()) <= 1 and dr.chi_e_ratio(got["chi_e"], ref) <= 1
    per = kr.bound(1, dr.C_HPL, ref["Hpl_mass"])
    worst = (np.abs(np.asarray(got["Hpl"], LD) - ref["Hpl"]) / np.where(per > 0, per, 1)).reshape(f["E"], -1).max(1)
    for i in np.argsort(-worst)[:5]:
        print("%-24s %-16s Hpl %.3g of the bound" % (dd.HAND_NAMES[f["lm"][i]], dd.HAND_ENTRIES[f["cam_id"][i]][0], worst[i]))


@pytest.mark.parametrize("design,pattern", dd.PLAIN_CASES, ids=["%s-%s" % c for c in dd.PLAIN_CASES])
def test_a_float64_evaluation_is_inside_the_bounds(design, pattern):
    f, hs, rk2, ref = reference(design, pattern)
    got = dr.build(f, rk2, dtype=np.float64)
    r = dr.ratios(got, ref)
    print(design, pattern, {k: "%.3g" % v for k, v in r.items()})
    assert max(r.values()) <= 1
    assert dr.chi_e_ratio(got["chi_e"], ref) <= 1


# the patterns on which each mistake must show
DISTORTED = ("all", "third", "blocks", "beyond", "one", "many")
SHOWS_ON = {"p_swapped": DISTORTED, "two_dropped": DISTORTED, "six_as_two": DISTORTED, "dr_without_k3": DISTORTED,
            "dr_by_r": DISTORTED, "pixel_units": DISTORTED, "A3_pinhole": DISTORTED,
            "stereo_kept": ("all",),            # (the one pattern with stereo bits on distorted entries)
            "stride17": ("all", "third", "many"), "neighbour_flag": ("third", "many")}


@pytest.mark.parametrize("mut", dr.MUTATIONS)
def test_each_mistake_breaks_the_bounds(mut):
    for pattern in SHOWS_ON[mut]:
        f, hs, rk2, ref = reference("A", pattern)
        with np.errstate(all="ignore"):                  # (a confused stride reads a translation as a flag)
            r = dr.ratios(dr.build(f, rk2, mut=mut, dtype=np.float64), ref)
        print(mut, pattern, {k: "%.3g" % v for k, v in r.items()})
        assert max(r.values()) > 10, (mut, pattern)
    # and where no slot sits on a distorted entry no mistake in the term can show
    if mut not in ("stride17", "neighbour_flag"):
        f, hs, rk2, ref = reference("A", "plain")
        assert max(dr.ratios(dr.build(f, rk2, mut=mut, dtype=np.float64), ref).values()) <= 1


def test_a_mistake_in_the_jacobian_alone_leaves_chi():
    f, hs, rk2, ref = reference("A", "third")
    for mut in ("six_as_two", "dr_without_k3", "dr_by_r", "A3_pinhole"):
        r = dr.ratios(dr.build(f, rk2, mut=mut, dtype=np.float64), ref)
        assert r["chi"] <= 1 and min(r[k] for k in ("Hpp", "bp", "Hll", "bl", "Hpl")) > 10, (mut, r)


@pytest.mark.parametrize("fused", [False, True])
def test_all_undistorted_tables_equal_the_rig_reference(fused):
    f, hs, rk2, ref = reference("A", "plain", fused)
    rig = rr.build(f, rk2)
    for key in dr.KEYS:
        assert np.array_equal(np.asarray(ref[key]), np.asarray(rig[key])), key
        assert np.array_equal(np.asarray(ref[key + "_mass"]), np.asarray(rig[key + "_mass"])), key
    real = (f["flags"] & 8) == 0
    assert all(np.array_equal(ref[k][real], rig[k][real]) for k in ("JP", "JL", "e", "w"))
