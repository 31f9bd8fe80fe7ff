"""CPU tests of the depth reference (tests/depth_ref.py) and of the depth layouts (tests/depth_designed.py): the
Jacobians of the depth row against central differences in np.longdouble, a plain float64 evaluation inside the per-entry
bounds on every pattern, and five deliberate mistakes of an implementation each OUTSIDE them on every pattern they can
touch — the bounds the GPU tests of test_depth_shapes.py hold the kernels to are tight enough to tell."""
import functools

import numpy as np
import pytest

import depth_designed as dd
import depth_ref as dr
import kernel_ref as kr
import synth

LD = kr.LD
RK_NONE = dict(mono=(0, 1.0), stereo=(0, 1.0), depth=(0, 1.0))


def single_edges(n=12, seed=3):
    """n problems of one pose, one landmark and one edge each, flattened by hand: kinds mono, stereo, depth in turn, the
    geometry of make_golden.kat_edges"""
    rng = np.random.default_rng(seed)
    poses, lms, cams, flags, meas = [], [], [], [], []
    for i in range(n):
        q = synth.quat_from_rotvec(rng.normal(0, 0.4, 3))
        q = q / np.linalg.norm(q)
        t = rng.normal(0, 1.0, 3)
        Xc0 = np.array([rng.uniform(-5, 5), rng.uniform(-3, 3), rng.uniform(4, 40)])
        R = np.asarray(kr._quat_R(np.asarray(q, LD)), np.float64)
        poses.append(np.concatenate([q, t]))
        lms.append(R.T @ (Xc0 - t))
        cam = synth.KITTI_CAM * (1 + 0.01 * i)
        cams.append(cam)
        kind = i % 3
        flags.append((0, dr.STEREO, dr.DEPTH)[kind])
        pu, pv = cam[0] * Xc0[0] / Xc0[2] + cam[2], cam[1] * Xc0[1] / Xc0[2] + cam[3]
        third = (0.0, pu - cam[4] / Xc0[2], 1.0 / Xc0[2] + rng.normal(0, 1e-3))[kind]
        meas.append([pu + rng.normal(0, 2.0), pv + rng.normal(0, 2.0), third])
    idx = np.arange(n, dtype=np.int32)
    return dict(E=n, P=n, L=n, Pall=n, Lall=n, pose=idx, lm=idx.copy(), flags=np.array(flags, np.uint8),
                meas=np.ascontiguousarray(np.array(meas).T), omega=np.ones(n), cams=np.array(cams),
                cam_id=idx.astype(np.uint16), poses=np.array(poses), lms=np.array(lms))


@pytest.mark.parametrize("k", dd.WEIGHTS)
def test_jacobians_match_central_differences(k):
    """-de/dxi (left perturbation exp(d) T, order [omega, upsilon]) and -de/dXw by central differences in longdouble:
    step 1e-6 and rtol 1e-6 as make_golden.kat_edges; the absolute term is 1e-6 of the row's largest entry instead of
    kat_edges' fixed 1e-4 / 1e-5, under which a depth row of size 1e-3 would pass whatever it held"""
    f = single_edges()
    n = f["E"]
    ref = dr.build(f, RK_NONE, k)
    h = LD(1e-6)

    def residual(poses, lms):
        g = dict(f)
        g["poses"], g["lms"] = poses, lms
        return dr.build(g, RK_NONE, k)["e"]

    P0, L0 = np.asarray(f["poses"], LD), np.asarray(f["lms"], LD)
    JP = np.zeros((n, 3, 6), LD)
    JL = np.zeros((n, 3, 3), LD)
    for j in range(6):
        d = np.zeros(6, LD)
        d[j] = h
        pp = np.array([kr.pose_update(P0[i], d) for i in range(n)], LD)
        pm = np.array([kr.pose_update(P0[i], -d) for i in range(n)], LD)
        JP[:, :, j] = -(residual(pp, L0) - residual(pm, L0)) / (2 * h)
    for j in range(3):
        d = np.zeros(3, LD)
        d[j] = h
        JL[:, :, j] = -(residual(P0, L0 + d) - residual(P0, L0 - d)) / (2 * h)
    depth = (f["flags"] & dr.DEPTH) != 0
    assert depth.sum() >= 3 and np.all(np.abs(ref["JP"][depth, 2]).max(1) > 0)
    for name, got, num in (("JP", ref["JP"], JP), ("JL", ref["JL"], JL)):
        for i in range(n):
            for m in range(3):
                a, b = np.asarray(got[i, m], np.float64), np.asarray(num[i, m], np.float64)
                tol = 1e-6 * np.abs(b) + 1e-6 * np.abs(b).max()
                assert np.all(np.abs(a - b) <= tol), (name, i, m, a, b)
    # the mono rows of a depth slot are the mono rows; its third row is not the stereo row
    assert np.all(ref["JP"][depth, 2, 2:5] == 0)


CASES = [(d, p, k) for d, p in dd.PLAIN_CASES for k in dd.WEIGHTS]


@functools.lru_cache(maxsize=None)
def reference(design, pattern, k, which=0):
    f, _ = dd.case(design, pattern)
    rk3 = dd.robust3(design, which)
    return f, rk3, dr.build(f, rk3, k)


def test_census_of_every_pattern():
    for design, pattern in dd.PLAIN_CASES:
        f, _ = dd.case(design, pattern)
        n = int(((f["flags"] & dr.DEPTH) != 0).sum())
        assert (n == 0) == (pattern == "none"), (design, pattern, n)
        assert not np.any((f["flags"] & dr.STEREO != 0) & (f["flags"] & dr.DEPTH != 0))
    for design, pattern in dd.FUSED_CASES:
        f, _ = dd.case(design, pattern, fused=True)
        assert (((f["flags"] & dr.DEPTH) != 0).sum() == 0) == (pattern == "none")
    assert {p for _, p in dd.PLAIN_CASES} == set(dd.PATTERNS)


@pytest.mark.parametrize("design,pattern,k", CASES)
def test_float64_evaluation_stays_inside_the_bounds(design, pattern, k):
    for which in (0, 1):
        f, rk3, ref = reference(design, pattern, k, which)
        got = dr.build(f, rk3, k, dtype=np.float64)
        r = dr.ratios(got, ref)
        r["chi_e"] = dr.chi_e_ratio(got["chi_e"], ref)
        print(design, pattern, k, which, {key: "%.3g" % v for key, v in r.items()})
        assert max(r.values()) <= 1, r


def touched(f, mut, k):
    """the outputs mistake `mut` can touch on the flattened case f (empty: none)"""
    fl = f["flags"]
    act = ((fl & dr.DEPTH) != 0) & ((fl & dr.INACTIVE) == 0)
    if not act.any() or (mut == "s_residual_only" and k == 1.0):
        return set()
    free_p = act & (f["pose"] < f["P"])
    free_l = act & (f["lm"] < f["L"])
    both = act & ((fl & 3) == 0)
    out = set()
    if mut in ("as_stereo", "as_mono"):
        out.add("chi")
    if mut in ("as_stereo", "as_mono", "s_residual_only"):
        out |= {"Hll", "bl"} if free_l.any() else set()
    if free_p.any():
        out |= {"Hpp", "bp"}
    if both.any() and mut != "pose_pass_mono":
        out.add("Hpl")
    return out


@pytest.mark.parametrize("mut", dr.MUTATIONS)
@pytest.mark.parametrize("design,pattern,k", CASES)
def test_each_mistake_breaks_the_bounds(design, pattern, k, mut):
    f, rk3, ref = reference(design, pattern, k)
    r = dr.ratios(dr.build(f, rk3, k, mut=mut), ref)
    t = touched(f, mut, k)
    print(design, pattern, k, mut, sorted(t), {key: "%.3g" % v for key, v in r.items()})
    # (a mistake is found when ANY output leaves its bounds: at k = 1 the depth row is 1e-3 of the pixel rows, and what
    # it adds to a sum of a thousand pixel terms can stay below their rounding allowance in some outputs, never in all)
    if t:
        assert max(r[key] for key in t) > 1, "a build with the mistake %r is inside the bounds: %r" % (mut, r)
    for key in dr.KEYS:
        if key not in t:
            assert r[key] <= 1, "%s moved although the mistake %r cannot touch it" % (key, mut)
