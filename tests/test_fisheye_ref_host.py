"""CPU tests of the fisheye reference (tests/fisheye_ref.py) and of the designed model tables
(tests/fisheye_designed.py): the Jacobians against central differences in longdouble at every hand-placed point and on
the ring scene, a plain float64 evaluation inside the per-entry bounds on every pattern, each of the eight plausible
mistakes outside them with its factor, and the all-pinhole table against rig_ref.build."""
import functools

import numpy as np
import pytest

import fisheye_designed as fd
import fisheye_ref as fr
import kernel_ref as kr
import rig_ref as rr

LD = kr.LD
NONE2 = dict(mono=(0, 1.0), stereo=(0, 1.0))


@functools.lru_cache(maxsize=None)
def reference(design, pattern, fused=False):
    f, hs = fd.case(design, pattern, fused)
    rk2 = fd.robust2(design, 0, fused)
    return f, hs, rk2, fr.build(f, rk2)


@functools.lru_cache(maxsize=None)
def hand_reference():
    f, hs = fd.hand_points()
    return f, hs, fr.build(f, NONE2)


def central_differences(f, ref, h):
    """largest |numerical - analytic| entry of JP and of JL per slot, each relative to the slot's largest entry of
    that Jacobian.  Central differences on the five-point stencil (f(-2h), f(-h), f(h), f(2h)): truncation
    h^4 |e^(5)| / 30"""
    E = f["E"]

    def residuals(poses, lms):
        return fr.build(dict(f, poses=poses, lms=lms), NONE2)["e"]

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
    """Held to 2e-12 of the slot's largest entry.  h = 1e-5: the rounding of the residual (u_LD x 700 px) over h is
    ~4e-12 px, ~1e-13 of an entry of order 100; the truncation h^4 |e^(5)| / 30 is below that even at the nearest point
    (0.25 m).  (The two-point difference cannot reach the figure here: its rounding and truncation meet at ~1e-12.)  At
    r = 0 the stencil straddles the axis, on which e is smooth"""
    f, hs, ref = hand_reference()
    rp, rl = central_differences(f, ref, LD(1e-5))
    for i in range(f["E"]):
        print("%-24s entry %d   JP %.3g   JL %.3g of the slot's largest entry" % (fd.HAND_NAMES[f["lm"][i]], f["cam_id"][i],
                                                                                 rp[i], rl[i]))
    assert rp.max() <= 2e-12 and rl.max() <= 2e-12


def test_jacobians_against_central_differences_on_the_ring():
    f = fd.ring_scene()
    ref = fr.build(f, NONE2)
    rp, rl = central_differences(f, ref, LD(1e-5))
    print("ring: JP %.3g, JL %.3g of the slot's largest entry" % (rp.max(), rl.max()))
    assert rp.max() <= 2e-12 and rl.max() <= 2e-12
    assert np.abs(np.asarray(f["cam_tab"])[1:, :9] - np.eye(3).ravel()).max() > 0.9    # large rotations


def test_float64_evaluation_of_the_hand_placed_points_is_inside_the_bounds():
    f, hs, ref = hand_reference()
    got = fr.build(f, NONE2, dtype=np.float64)
    r = fr.ratios(got, ref)
    print({k: "%.3g" % v for k, v in r.items()})
    assert max(r.values()) <= 1 and fr.chi_e_ratio(got["chi_e"], ref) <= 1
    per = kr.bound(1, fr.C_HPL, ref["Hpl_mass"])
    worst = (np.abs(np.asarray(got["Hpl"], LD) - ref["Hpl"]) / np.where(per > 0, per, 1)).reshape(f["E"], -1).max(1)
    for i in np.argsort(-worst)[:5]:
        print("%-24s entry %d   Hpl %.3g of the bound" % (fd.HAND_NAMES[f["lm"][i]], f["cam_id"][i], worst[i]))


@pytest.mark.parametrize("design,pattern", fd.PLAIN_CASES, ids=["%s-%s" % c for c in fd.PLAIN_CASES])
def test_a_float64_evaluation_is_inside_the_bounds(design, pattern):
    f, hs, rk2, ref = reference(design, pattern)
    got = fr.build(f, rk2, dtype=np.float64)
    r = fr.ratios(got, ref)
    print(design, pattern, {k: "%.3g" % v for k, v in r.items()})
    assert max(r.values()) <= 1
    assert fr.chi_e_ratio(got["chi_e"], ref) <= 1


# the patterns on which each mistake must show
SHOWS_ON = {"k_ignored": ("all", "third", "blocks", "beyond", "one", "many"),
            "pinhole_A": ("all", "third", "blocks", "beyond", "one", "many"),
            "D_as_P": ("all", "third", "one", "many"),
            "z_sign": ("all", "third", "blocks", "beyond", "one", "many"),
            "stride12": ("all", "third", "many"),
            "neighbour_flag": ("third", "many"),
            "pose_pass_rig": ("all", "third", "blocks", "one", "many")}


@pytest.mark.parametrize("mut", [m for m in fr.MUTATIONS if m != "quotient_c"])
def test_each_mistake_breaks_the_bounds(mut):
    for pattern in SHOWS_ON[mut]:
        f, hs, rk2, ref = reference("A", pattern)
        with np.errstate(all="ignore"):                  # (a confused stride reads a translation as a flag)
            r = fr.ratios(fr.build(f, rk2, mut=mut, dtype=np.float64), ref)
        print(mut, pattern, {k: "%.3g" % v for k, v in r.items()})
        assert max(r.values()) > 10, (mut, pattern)
    # and where no slot sits on a Kannala-Brandt entry no mistake in the model can show
    if mut not in ("stride12", "neighbour_flag"):
        f, hs, rk2, ref = reference("A", "pinhole")
        assert max(fr.ratios(fr.build(f, rk2, mut=mut, dtype=np.float64), ref).values()) <= 1


def test_pose_pass_rig_leaves_everything_but_the_pose_pass():
    f, hs, rk2, ref = reference("A", "third")
    r = fr.ratios(fr.build(f, rk2, mut="pose_pass_rig", dtype=np.float64), ref)
    assert r["Hpp"] > 10 and r["bp"] > 10 and max(r[k] for k in ("Hll", "bl", "Hpl", "chi")) <= 1


def test_the_quotient_form_of_c_breaks_the_bounds_at_the_near_axis_points():
    """float64 with c = (D z / R2 - rho) / r2 below the switch: the difference loses its digits like 1 / s^2.  Held per
    slot: outside the bound (factor > 10) on every hand-placed near-axis point, while the same evaluation with the
    near-axis form is inside on all of them (test above).  Measured: 1.9e11, 2.4e7 and 1.2e3 of the bound at s^2 = 1e-24,
    1e-12 and 1e-8; at s^2 = 1e-4 the quotient form is still inside (0.66): its loss, ~u / s^2, is then below the ~1500 u
    the entries of A are allowed, so that point is not among fisheye_designed.HAND_NEAR_AXIS"""
    f, hs, ref = hand_reference()
    got = fr.build(f, NONE2, mut="quotient_c", dtype=np.float64)
    per = kr.bound(1, fr.C_HPL, ref["Hpl_mass"])
    ratio = (np.abs(np.asarray(got["Hpl"], LD) - ref["Hpl"]) / np.where(per > 0, per, 1)).reshape(f["E"], -1).max(1)
    for i in range(f["E"]):
        if f["lm"][i] in fd.HAND_NEAR_AXIS:
            print("%-24s entry %d   Hpl %.3g of the bound" % (fd.HAND_NAMES[f["lm"][i]], f["cam_id"][i], ratio[i]))
            assert ratio[i] > 10
    assert fr.ratios(got, ref)["Hpl"] > 10


@pytest.mark.parametrize("fused", [False, True])
def test_all_pinhole_model_tables_equal_the_rig_reference(fused):
    f, hs, rk2, ref = reference("A", "pinhole", fused)
    rig = rr.build(f, rk2)
    for key in fr.KEYS:
        assert np.array_equal(np.asarray(ref[key]), np.asarray(rig[key])), key
        assert np.array_equal(np.asarray(ref[key + "_mass"]), np.asarray(rig[key + "_mass"])), key
    real = (f["flags"] & 8) == 0
    assert all(np.array_equal(ref[k][real], rig[k][real]) for k in ("JP", "JL", "e", "w"))
