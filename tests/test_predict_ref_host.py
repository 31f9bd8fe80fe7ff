"""CPU checks of tests/predict_ref.py (no GPU): they pin the extended-precision reference of the predicted observation
and its covariance, and its per-entry bounds, before test_predict_shapes.py holds k_predict_obs against them.

* K_S_PRED and K_Z_PRED: a float64 run of the reference's own formulas against the longdouble run (S in two summation
  orders), with the designed camera tables and without a table, in units of (n + C) u mass and c_z u mass; the constants
  are 4 x the largest ratio over the designs, rounded up, the per-design ratios are recorded in REPLAY_S / REPLAY_Z;
  the replay is inside the bounds on every design;
* the designed tables hold in one wave what they say they hold;
* without a table and with kinds 2 / 3 the reference IS pl_cov_ref.reprojection;
* J_p and J_l against five-point central differences of the longdouble projection, left update on the body, per kind, at
  the hand-placed points of tests/fisheye_designed.py (r = 0, both sides of the 0.5 rad switch, z at 0 and a few ulp
  either side, theta up to 1.9), exactly there (identity pose and sensor pose) and behind a body pose and a sensor pose;
* each of the eight planted mistakes leaves the bounds.
"""
import functools

import numpy as np
import pytest

import fisheye_designed as fd
import kernel_ref as kr
import lm_cov_designed as ld
import pl_cov_ref as pr
import predict_ref as P
import rig_ref

LD = kr.LD


@functools.lru_cache(maxsize=None)
def designed(name):
    des = ld.design(name)
    Sigma = pr.dense_sigma(des, 0.0)
    qp, ql = pr.queries(des)
    inp = pr.reprojection_inputs(des, Sigma, qp, ql, pr.reference(des, Sigma, qp, ql))
    return des, inp, P.designed_queries(des, inp)


def test_one_wave_holds_every_kind_of_query():
    for name in P.DESIGNS:
        des, inp, q = designed(name)
        c = q["census"]
        print(name, q["n"], "queries; first wave:", c)
        assert c["pinhole_identity"] >= 3 and c["pinhole_rig"] >= 3 and c["kb_rig"] >= 3 and c["kinds"] == [2, 3, 4], (name, c)
        assert c["hand"] == len(fd.HAND_POINTS) == q["n_hand"], (name, c)
        assert c["fixed_pose"] >= 3 and c["fixed_lm"] >= 3 and c["both_fixed"] >= 3, (name, c)
        # every (kind, entry kind) pair among the free-free queries of the wave
        w = slice(0, P.WAVE)
        free = q["free_p"][w] & q["free_l"][w] & (q["base"][w] >= 0)
        fish = q["tab"][w, 16] != 0
        rig = ~np.all(q["tab"][w, :12] == rig_ref.IDENTITY12, axis=1)
        assert len({(int(k), bool(a), bool(b)) for k, a, b in zip(q["kind"][w][free], fish[free], rig[free])}) == 12, name
        # the hand-placed points arrive exactly: identity pose, identity sensor pose
        hand = q["base"] < 0
        assert np.array_equal(q["pose"][hand], np.tile([0, 0, 0, 1, 0, 0, 0.0], (hand.sum(), 1)))
        assert np.array_equal(np.sort(q["Xw"][hand], 0), np.sort(np.tile(np.array(fd.HAND_POINTS), (2, 1)), 0))
        assert q["n"] >= 513 or name != "grid513"
        th = np.arctan2(np.hypot(*P.predict_of(q, np.float64)["Xs"][:, :2].T), P.predict_of(q, np.float64)["Xs"][:, 2])
        assert (th[q["tab"][:, 16] != 0] > np.pi / 2).any(), "no Kannala-Brandt query beyond 90 degrees"


def test_replay_ratios_and_the_constants():
    worst_s, worst_z = {}, {}
    for name in P.DESIGNS:
        des, inp, q = designed(name)
        ws, wz = 0.0, 0.0
        for table, qq in ((True, q), (False, P.without_hand_points(q))):
            ref = P.predict_of(qq, table=table)
            assert np.all(np.isfinite(np.asarray(ref["S"], np.float64))) and np.all(np.isfinite(np.asarray(ref["z"], np.float64)))
            both = ~qq["free_p"] & ~qq["free_l"]
            assert not ref["S"][both].any() and not ref["S_mass"][both].any() and ref["z"][both].any()
            no3 = ~ref["rows3"]
            assert not ref["S"][no3][:, 2].any() and not ref["S"][no3][:, :, 2].any() and not ref["z"][no3][:, 2].any()
            for order in ("terms", "joint"):
                got = P.predict_of(qq, np.float64, order, table=table)
                rs, rz = P.ratios(got["S"], ref["S"], P.unit_s(ref)), P.ratios(got["z"], ref["z"], P.unit_z(ref))
                print("%-8s %-8s %-5s fp64 replay: S %.3g of (n + C) u mass, z %.3g of c_z u mass, %d queries"
                      % (name, "table" if table else "no table", order, rs.max(), rz.max(), qq["n"]))
                assert P.ratios(got["S"], ref["S"], P.bound_s(ref)).max() <= 1, (name, table, order)
                assert P.ratios(got["z"], ref["z"], P.bound_z(ref)).max() <= 1, (name, table, order)
                ws, wz = max(ws, float(rs.max())), max(wz, float(rz.max()))
        worst_s[name], worst_z[name] = ws, wz
        print("%-8s recorded S %.3g, z %.3g" % (name, P.REPLAY_S[name], P.REPLAY_Z[name]))
    for what, worst, K, rec in (("K_S_PRED", worst_s, P.K_S_PRED, P.REPLAY_S), ("K_Z_PRED", worst_z, P.K_Z_PRED, P.REPLAY_Z)):
        k = 4 * max(worst.values())
        print("%s: 4 x %.3g = %.3g (predict_ref: %g)" % (what, max(worst.values()), k, K))
        assert k <= K <= 64 and K <= 2 * k + 0.01
        for name in P.DESIGNS:
            assert worst[name] <= 4 * rec[name], (what, name)


def test_without_a_table_mono_and_stereo_are_the_reprojection_reference():
    des, inp, _ = designed("mixed")
    S, mass = pr.reprojection_of(inp)
    kind = np.where(inp["stereo"], 3, 2)
    got = P.predict(inp["pose"], inp["Xw"], inp["cam"], kind, None, inp["Saa"], inp["Sal"], inp["Sll"], inp["free_p"], inp["free_l"])
    assert np.array_equal(got["S"], S) and np.array_equal(got["S_mass"], mass)


# ------------------------------------------------------------------ central differences
def central_differences(pose, Xw, cam, kind, tab, h):
    """per query and row: largest |numerical - analytic| entry of JP and of JL, relative to the row's largest entry (1 for
    a row of zeros).  Five-point stencil, left update T <- exp([w, v]) T on the body"""
    ref = P.project(pose, Xw, cam, kind, tab, LD)
    base_p, base_l = np.asarray(pose, LD), np.asarray(Xw, LD)
    n = len(kind)

    def z_at(poses, lms):
        return P.project(poses, lms, cam, kind, tab, LD)["z"]
    err_p, err_l = np.zeros((n, 3), LD), np.zeros((n, 3), LD)
    for k in range(6):
        d = np.zeros(6, LD); d[k] = h

        def at(m):
            return z_at(np.array([kr.pose_update(base_p[i], m * d) for i in range(n)]), base_l)
        num = -(8 * (at(1) - at(-1)) - (at(2) - at(-2))) / (12 * h)        # the arrays hold -dz/d.
        err_p = np.maximum(err_p, np.abs(num - ref["JP"][:, :, k]))
    for k in range(3):
        def at(m):
            x = base_l.copy()
            x[:, k] += m * h
            return z_at(base_p, x)
        num = -(8 * (at(1) - at(-1)) - (at(2) - at(-2))) / (12 * h)
        err_l = np.maximum(err_l, np.abs(num - ref["JL"][:, :, k]))
    sp, sl = np.abs(ref["JP"]).max(2), np.abs(ref["JL"]).max(2)
    return err_p / np.where(sp > 0, sp, 1), err_l / np.where(sl > 0, sl, 1), ref


BODY = np.array([0.12, -0.2, 0.31, 0.92, 0.4, -1.1, 0.7])
BODY[:4] /= np.linalg.norm(BODY[:4])


def hand_queries(behind):
    """(pose, Xw, cam, tab [17] per coefficient set, names): the hand-placed points as Xs.  behind = False: identity
    pose and sensor pose, Xs = X_l exactly.  behind = True: the body pose BODY and the sensor pose SENSORS_KB[2], the
    landmark mapped back in float64 (Xs is the hand point to a few ulp: the special places of the term are those of
    the exact set, this set moves every frame)"""
    pts = np.array(fd.HAND_POINTS, np.float64)
    n = len(pts)
    cam = np.tile([400.0, 410.0, 320.0, 240.0, 35.0], (n, 1))
    e = np.zeros(17)
    if not behind:
        e[:12] = rig_ref.IDENTITY12
        return np.tile([0, 0, 0, 1, 0, 0, 0.0], (n, 1)), pts, cam, e
    e[:12] = rig_ref.quat_to_ext(P.SENSORS_KB[2])
    M, ts = e[:9].reshape(3, 3), e[9:12]
    R = P.frames(BODY[None], np.zeros((1, 3)), np.float64)[0][0]
    Xb = (pts - ts) @ M              # M^T (Xs - t_s), row-wise
    Xw = (Xb - BODY[4:]) @ R
    return np.tile(BODY, (n, 1)), Xw, cam, e


@pytest.mark.parametrize("behind", (False, True))
def test_jacobians_against_central_differences_at_the_hand_placed_points(behind):
    """Kannala-Brandt (equidistant and K_TYP) at every hand-placed point; the pinhole kinds 2, 3 and 4 at those with
    z >= 0.25 (a pinhole has no projection at z = 0).  Held to 2e-12 of the row's largest entry with h = 1e-5, the
    figures of tests/test_fisheye_ref_host.py: rounding u_LD x 700 px / h ~ 1e-13 of an entry of order 100, truncation
    h^4 |z^(5)| / 30 below that at the nearest point (0.25 m); the depth row's entries are of order 1 / z^2 >= 0.01 and
    its value of order 1 / z: rounding 4e-19 / 1e-5"""
    pose, Xw, cam, e = hand_queries(behind)
    n = len(Xw)
    names = set(fd.HAND_NAMES)
    assert {"r = 0", "switch - 1e-9", "switch + 1e-9", "z = 0", "z = +3 ulp of 0", "z = -3 ulp of 0", "theta = 1.9"} <= names
    worst = {}
    for label, coeff in (("kb equidistant", fd.K_ZERO), ("kb K_TYP", fd.K_TYP)):
        tab = np.tile(e, (n, 1))
        tab[:, 12:16], tab[:, 16] = coeff, 1.0
        rp, rl, ref = central_differences(pose, Xw, cam, np.full(n, 2), tab, LD(1e-5))
        worst[label] = (float(rp.max()), float(rl.max()))
        assert not ref["JP"][:, 2].any() and not ref["JL"][:, 2].any()
    front = np.array(fd.HAND_POINTS)[:, 2] >= 0.25
    assert front.sum() >= 15
    for kind in (2, 3, 4):
        tab = np.tile(e, (n, 1))[front]
        rp, rl, ref = central_differences(pose[front], Xw[front], cam[front], np.full(front.sum(), kind), tab, LD(1e-5))
        worst["pinhole kind %d" % kind] = (float(rp.max()), float(rl.max()))
        assert bool(ref["JP"][:, 2].any()) == (kind != 2)
    for label, (a, b) in worst.items():
        print("%-9s %-16s JP %.3g   JL %.3g of the row's largest entry" % ("behind" if behind else "exact", label, a, b))
        assert a <= 2e-12 and b <= 2e-12, label


# ------------------------------------------------------------------ the bound sees a mistake
@pytest.mark.parametrize("mut", P.MUTATIONS)
def test_each_mistake_leaves_the_bounds(mut):
    """the mistake planted in the reference's own formulas (longdouble; float64 for the quotient form of c, which is a
    loss of digits and no other formula) on the designed queries of `mixed`: the queries it applies to leave the bound
    of S or of z.  The quotient form shows where S holds the square of a small entry of A alone (set B of the
    hand-placed points): under a full Sigma the entries with rho cover it"""
    des, inp, q = designed("mixed")
    if mut == "fixed_pose_kept":      # (the inputs hold NaN for the blocks of a fixed pose: give them the first block)
        q = dict(q, Saa=np.where(np.isnan(q["Saa"]), q["Saa"][np.flatnonzero(q["free_p"])[0]], q["Saa"]))
    ref = P.predict_of(q)
    dt = np.float64 if mut == "quotient_c" else LD
    got = P.predict_of(q, dt, mut=mut)
    rs, rz = P.ratios(got["S"], ref["S"], P.bound_s(ref)), P.ratios(got["z"], ref["z"], P.bound_z(ref))
    fish = q["tab"][:, 16] != 0
    rig = ~np.all(q["tab"][:, :12] == rig_ref.IDENTITY12, axis=1)
    free = q["free_p"] | q["free_l"]
    applies = {"B_without_M": rig & free, "Xs_cross": rig & q["free_p"], "pinhole_A": fish & free,
               "ts_dropped": rig, "depth_weight": (q["kind"] == 4) & ~fish, "cross_once": q["free_p"] & q["free_l"],
               "fixed_pose_kept": ~q["free_p"],
               # (below the switch and off the axis: where the quotient form is another formula)
               "quotient_c": (q["base"] == -2) & (np.hypot(q["Xw"][:, 0], q["Xw"][:, 1]) > 0) &
                             (np.arctan2(np.hypot(q["Xw"][:, 0], q["Xw"][:, 1]), q["Xw"][:, 2]) < 0.5)}[mut]
    out = (rs > 1) | (rz > 1)
    print("%-16s %d of the %d queries it applies to leave the bounds (S up to %.3g, z up to %.3g of the bound); %d others"
          % (mut, (out & applies).sum(), applies.sum(), rs[applies].max(), rz[applies].max(), (out & ~applies).sum()))
    assert applies.sum() >= 3 and not (out & ~applies).any()
    if mut == "quotient_c":
        k = np.flatnonzero(q["base"] == -2)[fd.HAND_NAMES.index("s^2 = 1e-8")]
        assert applies[k] and rs[k] > 1, float(rs[k])
        assert all(rs[np.flatnonzero(q["base"] == -2)[i]] > 10 for i in fd.HAND_NEAR_AXIS)
        clean = P.predict_of(q, np.float64)
        assert P.ratios(clean["S"], ref["S"], P.bound_s(ref)).max() <= 1
    else:
        assert (out & applies).sum() >= 0.9 * applies.sum()
