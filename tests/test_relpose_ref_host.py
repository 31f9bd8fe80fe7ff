"""CPU checks of the relative-pose part of tests/pose_edge_ref.py and tests/pose_designed.py (no GPU): they pin the
extended-precision reference of the relative-pose SE(3) edges, its per-entry bounds and the designed layouts before
test_relpose_shapes.py holds relpose_kernels.hip against them.

* every layout's census, the plan arrays read back from a host-only cugo_relpose_plan (ctx == NULL);
* a float64 replay of the device's order (pose_edge_ref.relpose_replay over relpose_ref.edge_terms) lies inside the
  bounds of the longdouble reference on every layout, for H, Hoff, b, chi per pose, chi per edge and chi;
* R-zero is exact; one shared information matrix and the same matrix per edge replay to the same bits;
* every structural mutation of the replay breaks a bound on a named layout;
* a relative change of w by 1e-12 on a one-edge pose is seen per entry, and is NOT seen by a tolerance of 1e-12 max|.|.

Measured where this was written (x86-64, 80-bit longdouble):
  replay in device order, largest error / bound over the layouts:
        H 0.055  Hoff 0.079  b 0.037  chi 0.019  chi per edge 0.092  chi per pose 0.080
  mutations, the factor over the bound of the outputs they touch (asserted > 1; the untouched outputs of the purely
  structural ones asserted <= 1):
    chi2_twice       R-sides   chi 4.6e12, chi per pose 1.8e13       transposed   R-sides  Hoff 4.6e14
    overwrite        R-sides   Hoff 2.1e14                           drop_second  R-sides  Hoff 1.8e14
    Ja_for_Jb_fixed  R-sides   H 1.5e13, b 2.0e12                    chi_from_b   R-sides  chi per pose 5.5e12 (chi itself 6e-4: the
    rt_counted       R-sides   inf (entries whose bound is exactly 0)                       total cannot tell)
    no_tA = u = t_D  R-wg9     H 7.7e12, b 3.9e12, Hoff 2.4e13;  R-sides  H 3.3e13, b 3.3e12, Hoff 5.3e13;  R-far  H 2.5e11,
                     b 5.1e9, Hoff 5.1e11 (relpose_ref's "no_tA" and "u = t_D instead of t_D - t_A" are one and the same
                     formula: -J_a Ad(A) without the [t_A]x R_A block has [t_D]x R_A in its lower left)
    totals_256       R-totals1025  chi 3.3e9;  R-totals1029  chi 2.8e10
  a relative change of w by 1e-12 on R-sides' one-edge pose: 12.7 .. 429 x the bound on the diagonal of its block; under
  1e-12 max|.| the same change is 0.018 (H), 0.36 (b), 0.059 (Hoff) of the tolerance
"""
import importlib

import numpy as np
import pytest

import pose_designed as pd
import pose_edge_ref as per
import relpose_ref as RR

cugo = importlib.import_module("cuda-bundle-adjustment_amd")

ALL = pd.RELPOSE_NAMES + pd.RELPOSE_ZERO + pd.RELPOSE_TOTALS
KEYS = ("H", "b", "Hoff", "chi", "chi_edge", "chi_pose")


def reference(name):
    lay = pd.relpose_layout(name)
    return per.relpose_build(lay["poses"], lay["n_free"], lay["rp"], lay["rowptr"], lay["colind"])


def replay(name, mut=None, rp=None):
    lay = pd.relpose_layout(name)
    return dict(zip(KEYS, per.relpose_replay(lay["poses"], lay["n_free"], lay["rp"] if rp is None else rp, lay["rowptr"], lay["colind"], mut)))


def ratios(got, ref):
    return {k: per.ratio(got[k], ref[k], per.relpose_bound(ref, k)) for k in KEYS}


def c_plan_census(lay):
    """the census from the arrays of a host-only C plan; they equal relpose_ref.plan's"""
    rp = lay["rp"]
    pl = cugo.RelPosePlan(None, lay["P"], lay["n_free"], rp["a"], rp["b"], rp["flags"], lay["rowptr"], lay["colind"])
    arrays = [pl.array(k) for k in ("inc_ptr", "inc", "off_blk")]
    pl.close()
    for got, want in zip(arrays, RR.plan(rp, lay["n_free"], lay["rowptr"], lay["colind"])):
        assert np.array_equal(got, want)
    c = pd.relpose_census(lay, *arrays)
    assert {k: v for k, v in c.items()} == {k: lay["census"][k] for k in c}
    return c


# ------------------------------------------------------------------ census
@pytest.mark.parametrize("nf", [1, 3, 4, 5, 8, 9])
def test_layout_wg_counts_round_a_workgroup_of_four(nf):
    lay = pd.relpose_layout("R-wg%d" % nf)
    c = c_plan_census(lay)
    assert lay["n_free"] == nf and lay["P"] == nf + 2 and len(lay["rp"]["a"]) == nf + 3        # a chain and two chords
    assert c["workgroups"] == (nf + 3) // 4 and c["idle_waves_in_last_workgroup"] == (-nf) % 4
    assert all(d > 0 for d in c["degrees"])
    both = (lay["rp"]["a"] >= nf).sum() + (lay["rp"]["b"] >= nf).sum()
    assert both >= 3                                                                           # the fixed poses sit mid-chain
    if nf >= 3:
        assert c["rows_with_rowptr_ne_p"] == nf - 1 and c["blocks_no_edge_maps_to"] >= 1


def test_layout_sides_holds_every_case():
    lay = pd.relpose_layout("R-sides")
    c = c_plan_census(lay)
    print(c)
    assert c["hub"] == dict(a_hi=1, a_lo=1, b_hi=1, b_lo=1, a_fixed=1, b_fixed=1)
    assert c["degrees"][pd.SIDES_BIG] == 300 and c["degrees"][pd.SIDES_ONE] == 1
    assert c["poses_without_any_edge_between_active"] == [pd.SIDES_EMPTY]
    assert c["fixed_fixed"] == 1 and c["fixed_fixed_walked"] == 0
    assert 3 in c["pairs_in_mixed_orientation"] and 40 in c["pairs_in_mixed_orientation"]
    assert c["poses_all_inactive_in_plan"] == [pd.SIDES_PLAN_OFF] and c["poses_inactive_at_run_time_only"] == [pd.SIDES_RT_OFF]
    assert c["no_block_next_to_block"] >= 1 and c["blocks_no_edge_maps_to"] >= 1
    rp = lay["rp"]
    off = RR.plan(rp, lay["n_free"], lay["rowptr"], lay["colind"])[2]
    assert off[0] == -1 and off[1] >= 0 and rp["a"][0] == rp["a"][1] == pd.SIDES_HUB            # (hub, fixed) next to (hub, hi)
    # the run-time-inactive pose's blocks are in the pattern (the plan sees its edges) and no counting edge maps to them
    assert RR.block_of(lay["rowptr"], lay["colind"], 2, pd.SIDES_RT_OFF) and RR.block_of(lay["rowptr"], lay["colind"], 5, pd.SIDES_RT_OFF)
    assert c["workgroups"] == 4 and c["idle_waves_in_last_workgroup"] == 3


def test_layout_angles_on_both_sides_of_the_switches():
    lay = pd.relpose_layout("R-angles")
    c = c_plan_census(lay)
    ang = lay["census"]["angles"]
    n = 9                                             # three axes, three roles per angle
    print({k: v for k, v in ang.items() if k not in ("theta", "sn")}, c["hub"], lay["census"]["R_A_angle"])
    assert (ang["sn_le_1e-12"], ang["sn_gt_1e-12"], ang["theta_lt_1e-3"], ang["theta_ge_1e-3"], ang["near_pi"]) == (3 * n, 9 * n, 6 * n, 6 * n, 2 * n)
    assert c["hub"] == dict(a_hi=18, a_lo=18, b_hi=18, b_lo=18, a_fixed=36, b_fixed=0)
    lo, hi = lay["census"]["R_A_angle"]
    assert 1.8 < lo <= hi < 2.2                       # D is small only because Z cancels R_A
    # (an angle read back from a product of three rounded quaternions carries an absolute error of a few ulps of 1)
    np.testing.assert_allclose(ang["theta"], lay["angles"], rtol=1e-6, atol=1e-15)
    # the reference and a double evaluation of the formula under test stand on the sides the census counts
    t = reference("R-angles")["terms"]
    theta, sn = np.asarray(t["theta"], np.float64), np.asarray(t["sn"], np.float64)
    m = per.relpose_terms(lay["poses"], lay["n_free"], lay["rp"], np.float64, "matrix")
    for th_, sn_ in ((theta, sn), (m["theta"], m["sn"])):
        assert np.array_equal(sn_ > 1e-12, ang["sn"] > 1e-12) and np.array_equal(th_ < 1e-3, ang["theta"] < 1e-3)


def test_layout_far_cancels_three_digits():
    lay = pd.relpose_layout("R-far")
    c = c_plan_census(lay)
    rel, tn, td = np.array(lay["census"]["tA_rel"]), np.array(lay["census"]["t_norm"]), np.array(lay["census"]["tD_norm"])
    print("R-far: |t_A| / (|t_a| + |R_A t_b|) %.3g .. %.3g, |t| %.3g .. %.3g, |t_D| up to %.3g" % (rel.min(), rel.max(), tn.min(), tn.max(), td.max()))
    assert lay["P"] == 12 and rel.min() < 2e-3 and rel.max() < 2e-3 and tn.min() > 900 and td.max() < 0.1
    t = reference("R-far")["terms"]
    assert float(np.min(t["tA_rel"])) < 2e-3
    assert c["workgroups"] == 3


@pytest.mark.parametrize("k", range(4))
def test_layout_rk_edges_on_both_sides_of_the_threshold(k):
    lay = pd.relpose_layout("R-rk%d" % k)
    c_plan_census(lay)
    x = lay["census"]["x"]
    print("R-rk%d: %d edges inside delta^2, %d outside" % (k, x["inside"], x["outside"]))
    assert lay["rp"]["rk"] == pd.RKS[k] and x["inside"] > 50 and x["outside"] > 50
    if k == 2:                                        # Tukey: the outside ones have w = 0
        t = reference("R-rk2")["terms"]
        w = np.asarray(t["w"], np.float64)[t["live"]]
        assert (w == 0).sum() == x["outside"] and (w > 0).sum() == x["inside"]


def test_layout_info_dynamic_range_singular_and_indefinite():
    per_edge, one = pd.relpose_layout("R-info_perEdge"), pd.relpose_layout("R-info_one")
    E = len(per_edge["rp"]["a"])
    assert per_edge["rp"]["info"].shape == (E, 6, 6) and one["rp"]["info"].shape == (1, 6, 6)
    for Om in per_edge["rp"]["info"]:
        assert np.abs(Om[:3, :3]).max() / np.abs(Om[3:, 3:]).max() > 1e4 and np.linalg.eigvalsh(Om).min() > 0
    assert np.array_equal(one["rp"]["info"][0], per_edge["rp"]["info"][0])
    sing = pd.relpose_layout("R-info_singular")["rp"]["info"][0]
    assert np.linalg.matrix_rank(sing) == 3 and not sing[:3].any()
    ind = pd.relpose_layout("R-info_indef")
    x = ind["census"]["x"]
    print("R-info_indef: r^T Omega r < 0 on %d of %d counting edges" % (x["negative"], x["inside"] + x["outside"]))
    assert x["negative"] >= 1 and x["negative"] < x["inside"] + x["outside"]
    t = reference("R-info_indef")["terms"]
    neg = np.asarray(t["xr"], np.float64) < 0
    assert neg.sum() == x["negative"] and np.all(np.asarray(t["chi"].v)[neg] == 0) and np.all(np.asarray(t["x"])[neg] == 0)
    for name in ("R-info_perEdge", "R-info_one", "R-info_singular", "R-info_indef"):
        c_plan_census(pd.relpose_layout(name))


@pytest.mark.parametrize("nf,wgs", [(1024, 256), (1025, 257), (1029, 258)])
def test_layout_totals_reach_the_second_trip_of_the_chi_total(nf, wgs):
    lay = pd.relpose_layout("R-totals%d" % nf)
    c = c_plan_census(lay)
    assert c["workgroups"] == wgs and len(lay["rp"]["a"]) == nf + 1 and lay["P"] == nf + 1
    assert c["degrees"] == [2] * nf and (wgs > pd.TOTALS) == (nf > 1024)


# ------------------------------------------------------------------ float64 inside the bounds
@pytest.mark.parametrize("name", ALL)
def test_fp64_replay_inside_bounds(name):
    ref, got = reference(name), replay(name)
    r = ratios(got, ref)
    print("%-16s replay / bound: %s" % (name, "  ".join("%s %.3g" % (k, r[k]) for k in KEYS)))
    for k in KEYS:
        assert r[k] <= 1, (name, k, r[k])
    assert np.all(np.isfinite(np.asarray(ref["H"], np.float64))) and np.all(np.isfinite(got["H"]))
    dead = ~ref["terms"]["live"]
    assert np.all(np.asarray(ref["chi_edge_mass"])[dead] == 0) and np.all(got["chi_edge"][dead] == 0)


@pytest.mark.parametrize("k", range(4))
def test_zero_residual_is_exact(k):
    """R-zero: r = 0 and x = 0 in exact arithmetic and in float64: chi2 and b are exactly 0 under every robust kernel, H is
    finite and is rho'(0) J^T Omega J = the sum without a robust kernel, bit for bit in the reference and in the replay"""
    name = "R-zero%d" % k
    lay = pd.relpose_layout(name)
    ref, got = reference(name), replay(name)
    t = ref["terms"]
    assert np.all(t["r"] == 0) and np.all(t["x"] == 0) and np.all(t["theta"] == 0)
    assert ref["chi"] == 0 and np.all(ref["b"] == 0) and np.all(ref["chi_edge"] == 0)
    assert got["chi"] == 0.0 and not got["b"].any() and not got["chi_edge"].any()
    plain = dict(lay["rp"], rk=(0, 1.0))
    ref0 = per.relpose_build(lay["poses"], lay["n_free"], plain, lay["rowptr"], lay["colind"])
    got0 = replay(name, rp=plain)
    for key in ("H", "Hoff"):
        assert np.all(np.isfinite(got[key])) and got[key].any()
        assert np.array_equal(ref[key], ref0[key]) and np.array_equal(got[key], got0[key])
    # J^T Omega J with J_a = I, J_b = -Ad(A): entries of R_A in {0, +-1}, t_A in quarters
    for e in range(len(plain["a"])):
        assert np.array_equal(np.asarray(t["Ja"][e], np.float64), np.eye(6))
        RA, tA = RR.relative(lay["poses"][plain["a"][e]], lay["poses"][plain["b"][e]])
        assert np.array_equal(np.asarray(t["Jb"][e], np.float64), -RR.adjoint(RA, tA))


def test_one_info_for_all_equals_per_edge_info():
    lay = pd.relpose_layout("R-info_one")
    a, b = replay("R-info_one"), replay("R-info_one", rp=pd.relpose_per_edge_info(lay["rp"]))
    assert all(np.array_equal(a[k], b[k]) for k in KEYS) and a["chi"] > 0


# ------------------------------------------------------------------ the bounds see a subtle error
@pytest.mark.parametrize("mut,name,outputs", [
    ("chi2_twice", "R-sides", ("chi", "chi_pose")),          # an edge between two free poses counted by both walks
    ("transposed", "R-sides", ("Hoff",)),                    # the block of an edge whose b is lo not transposed into place
    ("no_tA", "R-wg9", ("H", "b", "Hoff")),                  # Ad(A) without its [t_A]x R_A block
    ("overwrite", "R-sides", ("Hoff",)),                     # the 3 and the 40 edges on one pair
    ("Ja_for_Jb_fixed", "R-sides", ("H", "b")),              # side b against a fixed pose (the hub and pose 0 have such edges)
    ("chi_from_b", "R-sides", ("chi_pose",)),                # the total is the same: only the per-pose sums tell
    ("rt_counted", "R-sides", ("H", "b", "Hoff", "chi", "chi_edge")),
    ("drop_second", "R-sides", ("Hoff",)),
    ("no_tA", "R-sides", ("H", "b", "Hoff")),                # = u = t_D instead of t_D - t_A; translations of order 1
    ("no_tA", "R-far", ("H", "b", "Hoff")),                  # the same where it is large
    ("totals_256", "R-totals1025", ("chi",)),                # the 257th workgroup total
    ("totals_256", "R-totals1029", ("chi",)),
])
def test_structural_mutations_of_the_replay_break_the_bound(mut, name, outputs):
    ref = reference(name)
    r = ratios(replay(name, mut), ref)
    print("%-16s on %-13s %s" % (mut, name, "  ".join("%s %.3g" % (k, r[k]) for k in KEYS)))
    for k in outputs:
        assert r[k] > 1, (mut, name, k, r[k])
    for k in set(KEYS) - set(outputs):                       # what the mutation does not touch stays inside
        if mut in ("chi2_twice", "transposed", "overwrite", "chi_from_b", "drop_second", "totals_256"):
            assert r[k] <= 1, (mut, name, k, r[k])


def _one_edge_change():
    lay = pd.relpose_layout("R-sides")
    rp, p = lay["rp"], pd.SIDES_ONE
    e = int(np.flatnonzero((rp["a"] == p) | (rp["b"] == p))[0])
    assert rp["rk"][0] == 0 and lay["census"]["degrees"][p] == 1
    scale = np.ones(len(rp["a"]), per.LD)
    scale[e] += per.LD(1e-12)
    ref = reference("R-sides")
    got = per.relpose_build(lay["poses"], lay["n_free"], rp, lay["rowptr"], lay["colind"], w_scale=scale)
    return p, ref, got


def test_a_relative_change_of_w_by_1e_12_on_a_one_edge_pose_is_seen():
    """R-sides has no robust kernel and pose 12 has one edge: every entry of its block is w times one sum, so w (1 + 1e-12)
    moves each by 1e-12 of itself.  Measured: 12.7 .. 429 x the bound on the diagonal of H."""
    p, ref, got = _one_edge_change()
    r = np.abs(got["H"][p] - ref["H"][p]) / per.relpose_bound(ref, "H")[p]
    d = np.arange(6)
    print("a 1e-12 change of w on R-sides' one-edge pose: %.3g .. %.3g x the bound on the diagonal of H" % (float(r[d, d].min()), float(r[d, d].max())))
    assert ref["H_n"][p, 0, 0] == 1 and r[d, d].min() > 1, np.asarray(r, np.float64)


def test_the_same_change_is_not_seen_by_a_tolerance_scaled_by_the_largest_entry():
    """what tests/test_relpose.py asks (1e-12 of max|.|) lets the same change pass on R-sides, where pose 0 sums 300 edges:
    the reason for the per-entry bound"""
    p, ref, got = _one_edge_change()
    for k in ("H", "b", "Hoff"):
        err, scale = float(np.abs(got[k] - ref[k]).max()), float(np.abs(ref[k]).max())
        print("%-4s max error %.3g, 1e-12 max|.| = %.3g" % (k, err, 1e-12 * scale))
        assert 0 < err < 1e-12 * scale, (k, err, scale)
    assert per.ratio(got["H"], ref["H"], per.relpose_bound(ref, "H")) > 1
