"""CPU checks of the pose-pose point edge reference (tests/point_pair_ref.py) and of the designed layouts
(tests/pair_designed.py) the GPU tests of test_point_pair_shapes.py rest on: the census of every design; the plain
float64 evaluation and the replay of the device's order inside the per-entry bounds; the term with T_a the fixed identity
against the unary point edge of point_edge_ref; the exchange of the roles under Omega = omega I; the Jacobians against
central differences of the left update; and mutations of the order and of the arithmetic, each of which must BREAK the
bounds on at least one design (a reference whose bounds a wrong kernel passes checks nothing)."""
import functools

import numpy as np
import pytest

import pair_designed as pdz
import point_edge_ref as ptr_ref
import point_pair_ref as ppr
from kernel_ref import LD, pose_update


@functools.lru_cache(maxsize=None)
def reference(name):
    lay = pdz.layout(name)
    return ppr.pair_build(lay["poses"], lay["n_free"], lay["P"], lay["e"])


def ratios(ref, H, b, Hoff, chi, chi_edge):
    return {k: ppr.ratio(g, ref[k], ppr.pair_bound(ref, k))
            for k, g in (("H", H), ("b", b), ("Hoff", Hoff), ("chi", chi), ("chi_edge", chi_edge))}


def evaluate64(lay):
    r = ppr.pair_build(lay["poses"], lay["n_free"], lay["P"], lay["e"], dtype=np.float64)
    return r["H"], r["b"], r["Hoff"], r["chi"], r["chi_edge"]


# ------------------------------------------------------------------ the designs hold what they were designed to hold
def test_census_of_layout_A():
    c = pdz.layout("A_spd")["census"]
    assert c["n"] == 2502 and c["n_runs"] == 10 + 64 + 17 + 5
    assert {63, 64, 65, 511, 512, 513, 1023, 1024, 2324, 2368} <= c["run_ends"]
    assert c["max_chunks_of_a_run"] == 3 and c["max_runs_in_a_group"] == 64
    assert c["slots"] == c["n_runs"] + 2              # the 1300-run lies in three chunks, every other run in one
    inc = c["incident"]
    assert inc[70] == 17 and inc[67] == 1 and inc[2] == 66 and not inc[[68, 69, 71]].any() and len(inc) == 72
    assert c["two_run_pairs"] == 1 and c["runs_a_fixed"] == 2 and c["runs_b_fixed"] == 2
    assert c["runs_not_counting"] == 2 and c["n_inactive"] > 100      # the inactive run and the fixed-fixed one
    lay = pdz.layout("A_spd")
    a, b = lay["e"]["a"], lay["e"]["b"]
    assert np.any(a[1:] < a[:-1])                                      # the container is not sorted
    assert pdz.layout("A_one")["e"]["info6"].shape == (1, 6) and not pdz.layout("A_zero")["e"]["info6"].any()
    assert np.all(np.abs(np.linalg.det(ptr_ref.unpack(pdz.layout("A_rank1")["e"]["info6"]))) < 1e-12)
    assert np.linalg.norm(lay["poses"][:, :3], axis=1).min() > 0.05   # general rotations


def test_census_of_layout_B_and_Z():
    c = pdz.layout("B")["census"]
    assert c["n"] == 320 and c["n_runs"] == 8 and c["n_pairs"] == 6 and c["runs_a_fixed"] + c["runs_b_fixed"] == 2
    z = pdz.zero_residual((0, 1.0))
    t = ppr.pair_terms(z["poses"], z["n_free"], z["e"], np.float64)
    assert not t["r"].any() and not t["chi"].any()


# ------------------------------------------------------------------ float64 and the replay lie inside the bounds
@pytest.mark.parametrize("name", pdz.NAMES)
def test_float64_evaluation_and_replay_within_bounds(name):
    lay = pdz.layout(name)
    ref = reference(name)
    r64 = ratios(ref, *evaluate64(lay))
    rep = ratios(ref, *ppr.pair_replay(lay["poses"], lay["n_free"], lay["P"], lay["e"]))
    print(name, "float64 / bound:", {k: "%.3g" % v for k, v in r64.items()}, " replay / bound:", {k: "%.3g" % v for k, v in rep.items()})
    assert max(r64.values()) <= 1 and max(rep.values()) <= 1
    assert not ref["H"][lay["n_free"]:].any() and not ref["H_mass"][lay["n_free"]:].any()   # fixed poses: zero, zero mass


@pytest.mark.parametrize("rk", [(0, 1.0), (1, 0.5), (2, 0.7), (3, 0.3)])
def test_zero_residuals(rk):
    lay = pdz.zero_residual(rk)
    ref = ppr.pair_build(lay["poses"], lay["n_free"], lay["P"], lay["e"])
    H, b, Hoff, chi, chi_edge = ppr.pair_replay(lay["poses"], lay["n_free"], lay["P"], lay["e"])
    assert chi == 0.0 and not chi_edge.any() and not b.any() and H.any() and Hoff.any()
    assert max(ratios(ref, H, b, Hoff, chi, chi_edge).values()) <= 1


# ------------------------------------------------------------------ properties of the term
def test_identity_a_is_the_unary_point_edge():
    """T_a the fixed identity: H_bb, b_b, chi2 are those of the PointEdge (p, z = q, Omega) on pose b, within the SUM of
    the two references' bounds"""
    rng = np.random.default_rng(5)
    lay = pdz.layout("B")
    P, nf = 4, 3
    poses = np.concatenate([lay["poses"][:3], [[0, 0, 0, 1.0, 0, 0, 0]]])
    E = 200
    b = np.sort(rng.integers(0, 3, E)).astype(np.int32)
    p = rng.normal(0, 2, (E, 3))
    z = np.einsum("eij,ej->ei", ppr._rot(poses[b, :4])[0], p) + poses[b, 4:] + rng.normal(0, 0.2, (E, 3))
    info6 = pdz.pt.make_info(rng, "spd", E)[0]
    for rk in ((0, 1.0), (3, 0.5), (1, 0.4)):
        pair = dict(a=np.full(E, 3, np.int32), b=b, p=p, z=z, info6=info6, active=np.ones(E, bool), rk=rk)
        unary = dict(pose=b, p=p, z=z, info6=info6, active=np.ones(E, bool), rk=rk)
        rp = ppr.pair_build(poses, nf, P, pair)
        ru = ptr_ref.point_build(poses, nf, unary)
        for k in ("H", "b", "chi"):
            got = rp[k][:nf] if k != "chi" else rp[k]
            bnd = (ppr.pair_bound(rp, k)[:nf] if k != "chi" else ppr.pair_bound(rp, k)) + ptr_ref.point_bound(ru, k)
            assert ppr.ratio(got, ru[k], bnd) <= 1, (rk, k)
        assert len(rp["pair_lo"]) == 0 and not rp["H"][3].any()


def test_exchanging_the_roles_keeps_chi2_under_isotropic_information():
    """Omega = omega I: (a, b, p, q) and (b, a, q, p) have the same chi2 (|R_b X + t_b - q| = |R_a X' + t_a - p| with X' the
    world point of q) up to the bounds; H is not compared, the Gauss-Newton models differ"""
    lay = pdz.layout("B")
    e = lay["e"]
    om = np.random.default_rng(8).uniform(0.5, 3.0, len(e["a"]))
    iso = np.stack([om, 0 * om, 0 * om, om, 0 * om, om], 1)
    for rk in ((0, 1.0), (3, 0.1)):
        fwd = dict(e, info6=iso, rk=rk)
        rev = dict(e, a=e["b"], b=e["a"], p=e["z"], z=e["p"], info6=iso, rk=rk)
        rf = ppr.pair_build(lay["poses"], lay["n_free"], lay["P"], fwd)
        rr = ppr.pair_build(lay["poses"], lay["n_free"], lay["P"], rev)
        assert ppr.ratio(rf["chi_edge"], rr["chi_edge"], ppr.pair_bound(rf, "chi_edge") + ppr.pair_bound(rr, "chi_edge")) <= 1
        assert ppr.ratio(rf["chi"], rr["chi"], ppr.pair_bound(rf, "chi") + ppr.pair_bound(rr, "chi")) <= 1 and rf["chi"] > 0


def test_jacobians_against_central_differences():
    """every edge gets poses of its own (a: index i, b: index E + i), so that a step of one end moves nothing else"""
    lay = pdz.layout("B")
    E = 40
    e0 = lay["e"]
    poses = np.asarray(np.concatenate([lay["poses"][e0["a"][:E]], lay["poses"][e0["b"][:E]]]), LD)
    e = dict(a=np.arange(E), b=E + np.arange(E), p=e0["p"][:E], z=e0["z"][:E], info6=e0["info6"][:E], active=np.ones(E, bool), rk=(0, 1.0))
    t0 = ppr.pair_terms(poses, 2 * E, e)
    h = LD(1e-6)
    worst = 0.0
    for side, J in (("a", t0["Ja"]), ("b", t0["Jb"])):
        for k in range(6):
            r = []
            for sgn in (1, -1):
                pp = poses.copy()
                dx = np.zeros(6, LD)
                dx[k] = sgn * h
                for i in e[side]:
                    pp[i] = pose_update(poses[i], dx)
                r.append(ppr.pair_terms(pp, 2 * E, e)["r"])
            num = (r[0] - r[1]) / (2 * h)
            worst = max(worst, float(np.abs(num - J[:, :, k]).max()))
    print("largest |J - central difference| at step 1e-6: %.3g" % worst)
    assert worst < 1e-8


# ------------------------------------------------------------------ wrong kernels break the bounds
@pytest.mark.parametrize("mut", ppr.ORDER_MUTATIONS + ppr.TERM_MUTATIONS)
def test_mutations_break_the_bounds(mut):
    broke = []
    for name in ("A_spd", "A_one", "B"):
        lay = pdz.layout(name)
        r = ratios(reference(name), *ppr.pair_replay(lay["poses"], lay["n_free"], lay["P"], lay["e"], mut=mut))
        if max(r.values()) > 1:
            broke.append((name, {k: v for k, v in r.items() if v > 1}))
    print(mut, "breaks:", [(n, {k: "%.3g" % v for k, v in d.items()}) for n, d in broke])
    assert broke, mut
