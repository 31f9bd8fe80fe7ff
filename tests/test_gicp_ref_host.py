"""CPU pins of the covariance-form reference (tests/gicp_ref.py) and its designed layouts (tests/gicp_designed.py): the
census of every layout and class; C_OMEGA against what the float64 replay of the device's inverse shows; a plain float64
evaluation and the replay of the device's operation order inside the bounds everywhere; the mutations a wrong kernel would
be (Omega not rotated, rotated the wrong way, the covariances swapped, role 0's Omega rotated twice, Omega frozen at
earlier poses) each break a bound by at least 1e3; the anchor to the information form."""
import functools

import numpy as np
import pytest

import gicp_designed as gd
import gicp_ref as gr
import point_edge_ref as ptr_ref
import point_pair_ref as ppr

LD = gr.LD
PAIR_KEYS = ("H", "b", "Hoff", "chi", "chi_edge")
POINT_KEYS = ("H", "b", "chi", "chi_edge")


@functools.lru_cache(maxsize=None)
def pair_reference(name):
    lay = gd.pair_layout(name)
    return gr.pair_build(lay["poses"], lay["n_free"], lay["P"], lay["e"])


@functools.lru_cache(maxsize=None)
def point_reference(name):
    lay = gd.point_layout(name)
    return gr.point_build(lay["poses"], lay["n_free"], lay["e"])


def pair_ratios(got, ref):
    H, b, Hoff, chi, edge = got
    return {k: gr.ratio(v, ref[k], gr.pair_bound(ref, k)) for k, v in (("H", H), ("b", b), ("Hoff", Hoff), ("chi", chi), ("chi_edge", edge))}


def point_ratios(got, ref):
    H, b, chi, edge = got[:4]
    return {k: gr.ratio(v, ref[k], gr.point_bound(ref, k)) for k, v in (("H", H), ("b", b), ("chi", chi), ("chi_edge", edge))}


# ------------------------------------------------------------------ census
def all_layouts():
    return [("pair", n) for n in gd.PAIR_NAMES] + [("point", n) for n in gd.POINT_NAMES]


def layout_of(kind, name):
    return gd.pair_layout(name) if kind == "pair" else gd.point_layout(name)


@pytest.mark.parametrize("kind,name", all_layouts())
def test_census(kind, name):
    lay = layout_of(kind, name)
    c, cls = lay["census"], lay["cov_class"]
    print(kind, name, {k: ("%.3g" % v if isinstance(v, float) else v) for k, v in c.items()})
    assert c["n_cov"] == (1 if cls == "one" else c["n"])
    if cls == "iso":
        assert c["kappa_max"] < 1 + 1e-12
    elif cls in ("gicp", "one"):
        assert 1 < c["kappa_min"] and c["kappa_max"] < 5e3 and c["lam_min_p"] < 2.1e-3
    elif cls == "aligned":
        assert 4e5 < c["kappa_min"] and c["kappa_max"] < 3e6
    elif cls == "zero_p":
        assert c["lam_max_p"] == 0.0 and c["lam_min_z"] > 1e-3
    elif cls == "rank2_p":
        assert abs(c["lam_min_p"]) < 1e-15 and c["lam_mid_p"] > 0.4 and c["lam_min_z"] > 0.04
    if name.startswith("A_") and kind == "pair":
        assert c["n"] == 2502 and c["n_inactive"] > 100
    if name.startswith("D_"):
        assert c["n_inactive"] == len(gd.INACT_D)


def test_pair_layout_A_is_the_information_forms():
    import pair_designed as pdz
    a, b = gd.pair_layout("A_gicp"), pdz.layout("A_spd")
    ca, cb = pdz.census(dict(a["e"], info6=None), a["n_free"], a["P"]), b["census"]
    for k in ("n", "n_runs", "run_ends", "slots", "max_chunks_of_a_run", "max_runs_in_a_group", "n_pairs", "two_run_pairs", "runs_a_fixed",
              "runs_b_fixed"):
        assert ca[k] == cb[k], k
    assert gd.pair_layout("B_gicp")["census"]["n"] == 320


# ------------------------------------------------------------------ C_OMEGA
def test_c_omega_is_four_times_the_observed_maximum():
    worst = {}
    for kind, name in all_layouts():
        lay = layout_of(kind, name)
        cls = lay["cov_class"]
        worst[cls] = max(worst.get(cls, 0.0), gr.c_omega_ratio(lay["poses"], lay["e"]), gr.c_omega_ratio(gd.moved(lay["poses"]), lay["e"]))
    print("largest |Omega_f64 - Omega| / (u |Omega| |S|a |Omega|) per class:", {k: "%.3g" % v for k, v in worst.items()})
    top = max(worst.values())
    assert set(worst) == set(gd.CLASSES)
    assert top <= gr.C_OMEGA_OBSERVED, "gicp_ref.C_OMEGA_OBSERVED is out of date"
    assert gr.C_OMEGA >= 4 * gr.C_OMEGA_OBSERVED and gr.C_OMEGA_OBSERVED <= 1.25 * top
    assert gr.C_OMEGA == int(np.ceil(4 * top)), "C_OMEGA is 4 x the largest observed ratio, rounded up"


def test_iso_is_the_scaled_identity():
    """exactly so for an orthogonal M; the layout's quaternions are unit to a few u (|q|^2 = 1 + eps, |eps| <= 4 u from the
    normalisation in double), M M^T = (1 + eps)^2 I for each of the two rotations, so Omega is off by at most ~4 eps"""
    lay = gd.pair_layout("A_iso")
    e = lay["e"]
    Om, _ = gr.omega_of(lay["poses"], e)
    s = (np.asarray(e["cov_p6"], LD)[:, 0] + np.asarray(e["cov_z6"], LD)[:, 0])
    want = np.eye(3, dtype=LD)[None] / s[:, None, None]
    assert np.abs(Om - want).max() <= 16 * gr.U * want.max()


# ------------------------------------------------------------------ float64 evaluations inside the bounds
@pytest.mark.parametrize("name", gd.PAIR_NAMES)
def test_pair_float64_and_replay_inside_the_bounds(name):
    lay = gd.pair_layout(name)
    ref = pair_reference(name)
    e = lay["e"]
    plain = ppr.pair_build(lay["poses"], lay["n_free"], lay["P"], gr.with_info(e, gr.omega_of_replay(lay["poses"], e)), np.float64)
    r1 = pair_ratios((plain["H"], plain["b"], plain["Hoff"], plain["chi"], plain["chi_edge"]), ref)
    r2 = pair_ratios(gr.pair_replay(lay["poses"], lay["n_free"], lay["P"], e), ref)
    print(name, "plain float64 / bound", {k: "%.3g" % v for k, v in r1.items()}, "replay", {k: "%.3g" % v for k, v in r2.items()})
    assert max(r1.values()) <= 1 and max(r2.values()) <= 1
    assert np.all(np.asarray(ref["H_extra"])[lay["n_free"]:] == 0), "a fixed pose has a bound"


@pytest.mark.parametrize("name", gd.POINT_NAMES)
def test_point_float64_and_replay_inside_the_bounds(name):
    lay = gd.point_layout(name)
    ref = point_reference(name)
    e = lay["e"]
    plain = ptr_ref.point_build(lay["poses"], lay["n_free"], gr.with_info(e, gr.omega_of_replay(lay["poses"], e)), np.float64)
    r1 = point_ratios((plain["H"], plain["b"], plain["chi"], plain["chi_edge"]), ref)
    r2 = point_ratios(gr.point_replay(lay["poses"], lay["n_free"], lay["P"], e), ref)
    print(name, "plain float64 / bound", {k: "%.3g" % v for k, v in r1.items()}, "replay", {k: "%.3g" % v for k, v in r2.items()})
    assert max(r1.values()) <= 1 and max(r2.values()) <= 1


# ------------------------------------------------------------------ mutations
@pytest.mark.parametrize("mut", gr.OMEGA_MUTATIONS + ("role0_twice",))
def test_pair_mutations_break_a_bound(mut):
    name = "A_gicp"
    lay, ref = gd.pair_layout(name), pair_reference(name)
    r = pair_ratios(gr.pair_replay(lay["poses"], lay["n_free"], lay["P"], lay["e"], mut=mut), ref)
    print(mut, {k: "%.3g" % v for k, v in r.items()})
    assert max(r.values()) >= 1e3, (mut, r)
    if mut == "role0_twice":
        assert max(r["chi"], r["chi_edge"], r["Hoff"]) <= 1 and r["H"] >= 1e3


@pytest.mark.parametrize("mut", gr.OMEGA_MUTATIONS)
def test_point_mutations_break_a_bound(mut):
    name = "A_gicp"
    lay, ref = gd.point_layout(name), point_reference(name)
    r = point_ratios(gr.point_replay(lay["poses"], lay["n_free"], lay["P"], lay["e"], mut=mut), ref)
    print(mut, {k: "%.3g" % v for k, v in r.items()})
    assert max(r.values()) >= 1e3, (mut, r)


@pytest.mark.parametrize("kind", ["pair", "point"])
def test_omega_frozen_at_the_first_poses_breaks_a_bound_at_the_second(kind):
    """two evaluations, at the layout's poses and after a step: the second with the Omega of the first"""
    lay = layout_of(kind, "A_gicp")
    e, P2 = lay["e"], gd.moved(lay["poses"])
    frozen = gr.with_info(e, gr.omega_of_replay(lay["poses"], e))
    if kind == "pair":
        ref2 = gr.pair_build(P2, lay["n_free"], lay["P"], e)
        ok = pair_ratios(gr.pair_replay(P2, lay["n_free"], lay["P"], e), ref2)
        bad = pair_ratios(ppr.pair_replay(P2, lay["n_free"], lay["P"], frozen), ref2)
    else:
        ref2 = gr.point_build(P2, lay["n_free"], e)
        ok = point_ratios(gr.point_replay(P2, lay["n_free"], lay["P"], e), ref2)
        bad = point_ratios(ptr_ref.point_replay(P2, lay["n_free"], lay["P"], frozen), ref2)
    assert max(ok.values()) <= 1 and min(bad["chi"], bad["H"], bad["b"]) >= 1e3, (ok, bad)


def test_the_classes_that_do_not_see_the_rotation():
    """iso and zero_p: Omega does not depend on M, so 'M_identity' stays inside the bounds: those classes cannot hold
    that mutation, the others do"""
    for name in ("A_iso", "A_zero_p"):
        lay, ref = gd.pair_layout(name), pair_reference(name)
        r = pair_ratios(gr.pair_replay(lay["poses"], lay["n_free"], lay["P"], lay["e"], mut="M_identity"), ref)
        assert max(r.values()) <= 1, (name, r)


# ------------------------------------------------------------------ the anchor to the information form
@pytest.mark.parametrize("name", ["A_gicp", "A_aligned", "B_gicp"])
def test_pair_anchor_information_form_with_the_rounded_omega(name):
    lay, ref = gd.pair_layout(name), pair_reference(name)
    info = gr.with_info(lay["e"], np.asarray(ref["Omega"]).astype(np.float64))
    ri = ppr.pair_build(lay["poses"], lay["n_free"], lay["P"], info)
    for k in PAIR_KEYS:
        r = gr.ratio(np.asarray(ri[k], LD), ref[k], gr.pair_bound(ref, k) + ppr.pair_bound(ri, k))
        assert r <= 1, (name, k, r)
        assert np.abs(np.asarray(ref[k], np.float64)).sum() > 0


@pytest.mark.parametrize("name", ["A_gicp", "B_aligned", "C_one"])
def test_point_anchor_information_form_with_the_rounded_omega(name):
    lay, ref = gd.point_layout(name), point_reference(name)
    info = gr.with_info(lay["e"], np.asarray(ref["Omega"]).astype(np.float64))
    ri = ptr_ref.point_build(lay["poses"], lay["n_free"], info)
    for k in POINT_KEYS:
        r = gr.ratio(np.asarray(ri[k], LD), ref[k], gr.point_bound(ref, k) + ptr_ref.point_bound(ri, k))
        assert r <= 1, (name, k, r)
