"""CPU tests of the rig reference (tests/rig_ref.py) and of the designed rig layouts (tests/rig_designed.py): the
Jacobians against central differences in longdouble on the ring scene (large rotations), a plain float64 evaluation
inside the per-entry bounds on every pattern, each of the seven plausible mistakes outside them, the all-identity table
against kernel_ref.build, and the equivalence that checks the reference against itself: with one sensor pose T_s on
every slot and body poses T_b = T_s^-1 T_c the rig reference is the plain reference at the camera poses T_c, pushed
through the adjoint of T_s."""
import functools

import numpy as np
import pytest

import kernel_ref as kr
import rig_designed as rd
import rig_lm_ref as rl
import rig_ref as rr

LD = kr.LD
NONE2 = dict(mono=(0, 1.0), stereo=(0, 1.0))


@functools.lru_cache(maxsize=None)
def reference(design, pattern, fused=False):
    f, hs = rd.case(design, pattern, fused)
    rk2 = rd.robust2(design, 0, fused)
    return f, hs, rk2, rr.build(f, rk2)


def test_jacobians_against_central_differences_on_the_ring():
    f = rd.ring_scene()
    ref = rr.build(f, NONE2)
    E = f["E"]
    h = LD(1e-6)
    scale = np.abs(np.asarray(ref["JP"], LD)).max()

    def residuals(poses, lms):
        return rr.build(dict(f, poses=poses, lms=lms), NONE2)["e"]

    base_p, base_l = np.asarray(f["poses"], LD), np.asarray(f["lms"], LD)
    worst_p = worst_l = LD(0)
    for p in range(f["Pall"]):
        on = f["pose"] == p
        for k in range(6):
            d = np.zeros(6, LD); d[k] = h
            plus, minus = base_p.copy(), base_p.copy()
            plus[p], minus[p] = kr.pose_update(base_p[p], d), kr.pose_update(base_p[p], -d)
            num = -(residuals(plus, base_l) - residuals(minus, base_l)) / (2 * h)      # the arrays hold -de/d.
            worst_p = max(worst_p, np.abs(num[on] - ref["JP"][on][:, :, k]).max())
    for l in range(f["Lall"]):
        on = f["lm"] == l
        for k in range(3):
            plus, minus = base_l.copy(), base_l.copy()
            plus[l, k] += h; minus[l, k] -= h
            num = -(residuals(base_p, plus) - residuals(base_p, minus)) / (2 * h)
            worst_l = max(worst_l, np.abs(num[on] - ref["JL"][on][:, :, k]).max())
    print("central differences: JP %.3g, JL %.3g of the largest entry %.3g" % (worst_p / scale, worst_l / scale, scale))
    # truncation h^2 |e'''| / 6 ~ 1e-12 relative, rounding u_LD / h ~ 1e-13
    assert worst_p <= 1e-9 * scale and worst_l <= 1e-9 * scale
    assert E == 72 and np.abs(np.asarray(f["cam_ext"])[1:, :9] - np.eye(3).ravel()).max() > 0.9    # large rotations


@pytest.mark.parametrize("design,pattern", rd.PLAIN_CASES, ids=["%s-%s" % c for c in rd.PLAIN_CASES])
def test_a_float64_evaluation_is_inside_the_bounds(design, pattern):
    f, hs, rk2, ref = reference(design, pattern)
    got = rr.build(f, rk2, dtype=np.float64)
    r = rr.ratios(got, ref)
    print(design, pattern, {k: "%.3g" % v for k, v in r.items()})
    assert max(r.values()) <= 1
    assert rr.chi_e_ratio(got["chi_e"], ref) <= 1


# the patterns on which each mistake must show (found on the CPU: the reference against its own mutant)
SHOWS_ON = {"ext_ignored": ("third", "blocks", "beyond", "poses", "one", "many", "stereo"),
            "jac_at_Xs": ("third", "one", "many", "stereo"),
            "M_transposed": ("third", "one", "many", "stereo"),
            "JL_without_M": ("third", "one", "many", "stereo"),
            "ts_dropped": ("third", "one", "many", "stereo"),
            "stride5": ("third", "many", "stereo"),
            "pose_pass_plain": ("third", "one", "many", "stereo")}


@pytest.mark.parametrize("mut", rr.MUTATIONS)
def test_each_mistake_breaks_the_bounds(mut):
    for pattern in SHOWS_ON[mut]:
        f, hs, rk2, ref = reference("A", pattern)
        with np.errstate(all="ignore"):                  # (a confused stride reads a translation as a depth: 1 / 0)
            r = rr.ratios(rr.build(f, rk2, mut=mut, dtype=np.float64), ref)
        print(mut, pattern, {k: "%.3g" % v for k, v in r.items()})
        assert max(r.values()) > 10, (mut, pattern)
    # and where no slot sits on a non-identity entry no mistake of this kind can show: the plain graph stays inside
    f, hs, rk2, ref = reference("A", "none")
    assert max(rr.ratios(rr.build(f, rk2, mut=mut, dtype=np.float64), ref).values()) <= 1


def test_pose_pass_plain_leaves_everything_but_the_pose_pass():
    f, hs, rk2, ref = reference("A", "third")
    r = rr.ratios(rr.build(f, rk2, mut="pose_pass_plain", dtype=np.float64), ref)
    assert r["Hpp"] > 10 and r["bp"] > 10 and max(r[k] for k in ("Hll", "bl", "Hpl", "chi")) <= 1


@pytest.mark.parametrize("pattern", ["identity", "none"])
def test_identity_tables_reproduce_the_plain_reference(pattern):
    f, hs, rk2, ref = reference("A", pattern)
    rk = rk2["mono"]
    plain = kr.build(None, rk, f)
    both = rr.build(f, dict(mono=rk, stereo=rk))
    r = rr.ratios(both, plain, kr.BUILD_C)           # the plain reference's own bounds
    print(pattern, {k: "%.3g" % v for k, v in r.items()})
    assert max(r.values()) <= 1e-2                   # two longdouble evaluations of one function
    # and the rig reference's masses are no smaller than the plain ones': its bounds contain the plain bounds
    for key in rr.KEYS:
        assert np.all(np.asarray(both[key + "_mass"]) >= np.asarray(plain[key + "_mass"]) * (1 - 1e-12))


def _quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], LD)


@pytest.mark.parametrize("k", [1, 2])
def test_one_sensor_pose_on_every_slot_is_the_plain_reference_through_the_adjoint(k):
    """T_b = T_s^-1 T_c on every pose: chi2, Hll, bl of the plain reference at T_c; Hpp, bp, Hpl through Ad(T_s).  Every
    entry within the sum of the two references' own bounds, the plain one's pushed through |Ad|.  (Everything in
    longdouble, the quaternions normalised there: R(q_b) = M^T R(q_c) to 1e-19.)"""
    f, hs = rd.case("A", "none")
    rk = rd.robust2("A", 0)["stereo"]
    qs = np.asarray(rd.SENSOR_POSES[k], LD)
    qs[:4] /= np.sqrt((qs[:4] * qs[:4]).sum())
    x, y, z, w = qs[:4]
    M = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], LD)
    ext = np.concatenate([M.ravel(), qs[4:]])[None, :]
    pc = np.asarray(f["poses"], LD).copy()
    pc[:, :4] /= np.sqrt((pc[:, :4] * pc[:, :4]).sum(1))[:, None]
    pb = pc.copy()
    conj = np.array([-x, -y, -z, w], LD)
    for i in range(len(pc)):
        pb[i, :4] = _quat_mul(conj, pc[i, :4])
        pb[i, 4:] = M.T @ (pc[i, 4:] - qs[4:])
    plain = kr.build(None, rk, dict(f, poses=pc))
    rig = rr.build(dict(f, poses=pb, cam_ext=ext), dict(mono=rk, stereo=rk))
    Ad = rr.adjoint(ext[0])
    aAd = np.abs(Ad)
    worst = {}
    for key in ("chi", "Hll", "bl"):
        bnd = rr.bound_of(rig, key) + rr.bound_of(plain, key, kr.BUILD_C)
        worst[key] = kr.ratio(rig[key], plain[key], bnd)
    push = {"Hpp": lambda a, T: np.einsum("ir,pij,jc->prc", T, a, T), "bp": lambda a, T: np.einsum("ir,pi->pr", T, a),
            "Hpl": lambda a, T: np.einsum("ir,eic->erc", T, a)}
    for key, fn in push.items():
        bnd = rr.bound_of(rig, key) + fn(rr.bound_of(plain, key, kr.BUILD_C) * np.ones_like(plain[key]), aAd)
        worst[key] = kr.ratio(rig[key], fn(np.asarray(plain[key], LD), Ad), bnd)
    print("sensor pose %d: %s" % (k, {a: "%.3g" % b for a, b in worst.items()}))
    assert max(worst.values()) <= 1
    assert np.abs(np.asarray(rig["Hpp"], np.float64) - np.asarray(plain["Hpp"], np.float64)).max() > 1.0   # not trivially equal


def test_the_lm_reference_and_the_kernel_reference_agree_on_an_edge():
    """rig_lm_ref.rig_edge (chain rule, float64) against rr.build on the ring scene: the same residuals and
    Jacobians (the LM reference of test_rig_graph.py is written by the chain rule, on its own)"""
    f = rd.ring_scene()
    ref = rr.build(f, NONE2)
    for i in range(f["E"]):
        st = bool(f["flags"][i] & 4)
        e, Xb, JP, JL = rl.rig_edge(f["poses"][f["pose"][i]], f["lms"][f["lm"][i]], f["meas"][:, i], st, f["cams"][f["cam_id"][i]],
                                   f["cam_ext"][f["cam_id"][i]])
        n = 3 if st else 2
        assert np.allclose(e, np.asarray(ref["e"][i][:n], float), rtol=0, atol=1e-9)
        assert np.allclose(JP, np.asarray(ref["JP"][i][:n], float), rtol=1e-11, atol=1e-9)
        assert np.allclose(JL, np.asarray(ref["JL"][i][:n], float), rtol=1e-11, atol=1e-9)


def test_without_the_lever_arms_the_scale_stays():
    """the same trajectory, landmarks and camera directions with both lever arms zero (every camera at the body's
    origin), shown on the reference: a start scaled by 1.2 is a minimum, chi2 0 — it is the lever arm that makes scale
    observable.  (With both sensor poses the identity the backward camera's landmarks would be behind it.)"""
    sensors = np.array(rl.RIG_SCALE).copy()
    sensors[:, 4:] = 0
    d = rl.scale_problem(sensors)
    g = rl.RigGraph(d)
    assert g.chi2() < 1e-12
    g.optimize(3)
    assert abs(rl.scale_of(d, g.lm) - 1.2) < 1e-9
