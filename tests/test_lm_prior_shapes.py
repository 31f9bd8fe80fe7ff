"""GPU tests of the landmark-prior kernels (lm_prior_kernels.hip, and the priors inside k_build_edges) on DESIGNED
layouts, through the kernel-level C ABI, against the extended-precision reference tests/lm_prior_ref.py with per-entry
bounds (n + c) u mass.

BA layouts (tests/designed.py builders, asserted legal on the CPU before any upload):
  D         landmark degrees 1, 254, 1, 255, 0, 256, 3, 257, 0, 300, ...: a 1-edge landmark whose owner slot is 0 and one
            whose owner slot is 255 of its group; landmarks of 256 / 257 / 300 edges across 256-slot boundaries, so that
            the owner walks edges beyond its block; edgeless landmarks, the last free one among them; Lfree = 17
  D_padded  the same in the engine's slot layout (inactive padding slots; no landmark of <= 256 edges straddles)
  C         designed.layout("C"): 598 free landmarks on 3 edge slots — priors on edgeless landmarks whose index exceeds E,
            Lfree no multiple of 256, three workgroups of the prior kernel
One landmark of D has all its BA edges flagged inactive.  Priors: 0 / 1 / 3 / 17 per free landmark in turn (the last
free landmark has 3), two on every fixed landmark, a tenth flagged inactive, given in random order (the sort is the
reference's, stable); zero residuals, semi-definite and zero Omega among them; every robust kernel on the prior set
with a different one on the BA sets; Tukey with priors beyond delta (w = 0).

Every output array is uploaded filled with NaN, or pre-filled where an entry ADDS.  Tolerances: nothing here was tuned
on a GPU; the bounds are lm_prior_ref's and kernel_ref's.
"""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import designed
import devmem
import kernel_ref as kr
import lm_prior_ref as LR
import oracle
import synth

pytestmark = pytest.mark.gpu

cugo = importlib.import_module("cuda-bundle-adjustment_amd")

D_LM_DEGREES = (1, 254, 1, 255, 0, 256, 3, 257, 0, 300, 5, 4, 7, 0, 2, 0, 0)
PER_LANDMARK = (0, 1, 3, 17)
# (prior set, BA sets): always different kernels
KERNELS = {"none": ((0, 1.0), (3, 1.5)), "cauchy": ((1, 0.7), (0, 1.0)), "huber": ((3, 0.4), (1, 2.0)), "tukey": ((2, None), (3, 1.5))}


@pytest.fixture(scope="module")
def ctx():
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    c = devmem.Ctx()
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def layout(name):
    """the flattened BA layout `name` (never modified: copy before changing anything)"""
    if name == "C":
        return designed.layout("C")[2]
    degs = list(D_LM_DEGREES)
    lmd = degs[:2] + [3] + degs[2:9] + [3] + degs[9:]   # two fixed landmarks (3 edges each), as designed.layout("B")
    d = designed.designed_by_landmark(lmd, 304, fixed_poses=(1, 77, 150, 200), fixed_landmarks=(2, 10), seed=6)
    f = devmem.flatten(oracle.Problem(*synth.problem_fields(d)))
    designed.check_layout(f)
    lp, L = f["lm_ptr"], f["L"]
    assert np.diff(lp)[:L].tolist() == list(D_LM_DEGREES) and L % 256 != 0
    assert lp[0] == 0 and lp[2] == 255 and lp[3] == 256          # owner slots 0 and 255 of group 0, one edge each
    st = designed.straddlers(f)
    assert {5, 7, 9} <= set(st)                                   # 256, 257 and 300 edges: edges beyond the owner's block
    if name == "D_padded":
        f = devmem.pad_to_groups(f)
        designed.check_layout(f)
        assert (f["flags"] & 8).any() and set(designed.straddlers(f)) == {7, 9}
    f = dict(f, flags=f["flags"].copy())
    lp = f["lm_ptr"]
    f["flags"][lp[6]:lp[7]] |= 8                                  # landmark 6: all of its BA edges inactive
    return f


@functools.lru_cache(maxsize=None)
def priors(name, kind, one_info=False):
    """(prior dict in the given order with flattened landmark indices, device layout, the order of the sort)"""
    f = layout(name)
    L, Lall = f["L"], f["Lall"]
    rng = np.random.default_rng({"D": 1, "D_padded": 1, "C": 2}[name])
    per = [PER_LANDMARK[l % 4] for l in range(L)]
    per[L - 1] = 3                                                # the last free landmark
    if name != "C":
        per[6] = 3                                                # the landmark whose BA edges are all inactive
        assert per[4] == 0 and per[5] == 1 and per[7] == 17 and per[8] == 0 and per[9] == 1 and per[16] == 3
    else:
        assert L > 256 + f["E"] and per[401] == 1 and per[403] == 17   # edgeless, index > E, in the second workgroup
    lm = np.concatenate([np.full(k, l) for l, k in enumerate(per)] + [np.full(2, l) for l in range(L, Lall)]).astype(np.int32)
    n = len(lm)
    z = f["lms"][lm] + rng.normal(0, 0.2, (n, 3))
    info = np.array([LR.random_spd3(rng, 2.0) for _ in range(n)])
    Q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    semi = Q @ np.diag([4.0, 0.0, 0.0]) @ Q.T
    special = rng.permutation(n)
    z[special[:5]] = f["lms"][lm[special[:5]]]                     # zero residuals
    info[special[3:8]] = 0.5 * (semi + semi.T)                    # semi-definite (two of them at a zero residual)
    info[special[8:11]] = np.diag([0.0, 0.0, 3.0])                # height only
    info[special[11:14]] = 0.0                                    # the zero matrix
    active = rng.random(n) >= 0.1
    if one_info:
        info = info[:1]
    rk, _ = KERNELS[kind]
    pr = LR.make_prior(lm, z, info, rk=(rk[0], rk[1] or 1.0), active=active)
    if rk[0] == 2:   # Tukey: about 30 % of the priors beyond delta
        x = np.asarray(LR.reference_build(f["lms"], L, pr)["x"], np.float64)
        delta = designed.tukey_delta(x[x > 0])
        pr["rk"] = (2, delta)
        beyond = float((x > delta * delta).mean())
        assert 0.1 <= beyond <= 0.9
    perm = rng.permutation(n)
    for k in ("lm", "z", "active"):
        pr[k] = pr[k][perm]
    if not one_info:
        pr["info"] = pr["info"][perm]
    order, lay = LR.sort_by_landmark(pr, Lall)
    assert (lay["flags"] != 0).any() and (lay["lm"] >= L).any()
    return pr, lay, order


def upload_priors(ctx, f, pr, lay, with_flags=True):
    ev = cugo.LmPriorEdges()
    ev.n_landmarks_total, ev.n_landmarks_free, ev.n = f["Lall"], f["L"], len(lay["lm"])
    ev.d_lm, ev.d_lm_ptr = ctx.to_dev(lay["lm"]), ctx.to_dev(lay["lm_ptr"])
    ev.d_meas, ev.d_info, ev.n_info = ctx.to_dev(lay["meas"]), ctx.to_dev(lay["info"]), lay["info"].shape[1]
    ev.d_flags = ctx.to_dev(lay["flags"]) if with_flags else None
    ev.rk, ev.delta = int(pr["rk"][0]), float(pr["rk"][1])
    return ev


def nan_dev(ctx, n, dtype=np.float64):
    return ctx.to_dev(np.full(max(int(n), 1), np.nan, dtype))


def report(what, r):
    print("%-48s %.3g of the bound" % (what, r))
    return r


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def run_errors(ctx, ev, d_lms, n):
    chi, ec = nan_dev(ctx, 2), nan_dev(ctx, n)
    cugo.lm_prior_compute_errors(ctx.h, ev, d_lms, chi, ec)
    return ctx.to_host(chi, 1), ctx.to_host(ec, n)


def run_add(ctx, ev, d_lms, Hll0, bl0):
    Hll, bl, chi = ctx.to_dev(Hll0), ctx.to_dev(bl0), nan_dev(ctx, 2)
    cugo.lm_prior_construct_quadratic_form(ctx.h, ev, d_lms, Hll, bl, chi)
    return ctx.to_host(Hll, Hll0.shape), ctx.to_host(bl, bl0.shape), ctx.to_host(chi, 1)


def run_build(ctx, f, bev, lev, rkc, f32=False):
    """the BA build pass, plain (lev None) or with the priors inside: Hpp, bp, Hll, bl, Hpl, chi as stored"""
    P, L, E = f["P"], f["L"], f["E"]
    bt = np.float32 if f32 else np.float64
    d_poses, d_lms = ctx.to_dev(f["poses"]), ctx.to_dev(f["lms"])
    d = dict(Hpp=nan_dev(ctx, 36 * P), bp=nan_dev(ctx, 6 * P), Hll=nan_dev(ctx, 9 * L), bl=nan_dev(ctx, 3 * L),
             Hpl=nan_dev(ctx, 18 * E, bt), chi=nan_dev(ctx, 4))
    if lev is None:
        cugo.check(cugo.lib().cugo_construct_quadratic_form(ctx.h, C.byref(bev), d_poses, d_lms, rkc, d["Hpp"], d["bp"], d["Hll"],
                                                            d["bl"], d["Hpl"], d["chi"]))
    else:
        cugo.construct_quadratic_form_lm_priors(ctx.h, bev, lev, d_poses, d_lms, rkc, d["Hpp"], d["bp"], d["Hll"], d["bl"],
                                                d["Hpl"], d["chi"])
    return dict(Hpp=ctx.to_host(d["Hpp"], (P, 36)), bp=ctx.to_host(d["bp"], (P, 6)), Hll=ctx.to_host(d["Hll"], (L, 9)),
                bl=ctx.to_host(d["bl"], (L, 3)), Hpl=ctx.to_host(d["Hpl"], (E, 18), bt), chi=ctx.to_host(d["chi"], 1))


@pytest.mark.parametrize("kind", list(KERNELS))
@pytest.mark.parametrize("name", ["D", "D_padded", "C"])
def test_stand_alone_entries(ctx, name, kind):
    """cugo_lm_prior_compute_errors and cugo_lm_prior_construct_quadratic_form against the reference's bounds; the add
    entry on pre-filled blocks; chi2 bit-equal between the two; repeatable bits"""
    f = layout(name)
    L = f["L"]
    pr, lay, order = priors(name, kind)
    n = len(order)
    ref = LR.reference_build(f["lms"], L, dict(pr, lm=lay["lm"], z=pr["z"][order], info=pr["info"][order], active=pr["active"][order]))
    bnd = LR.bounds(ref)
    assert ref["chi_n"] > 0 and (np.diff(lay["lm_ptr"])[:L] == 17).any() and (ref["Hll_n"][:L] == 0).any()
    if kind == "tukey":
        assert (np.asarray(ref["w"])[ref["counts"]] == 0).any()
    ev = upload_priors(ctx, f, pr, lay)
    d_lms = ctx.to_dev(f["lms"])
    chi, ec = run_errors(ctx, ev, d_lms, n)
    assert report("%s %s chi2 (error entry)" % (name, kind), kr.ratio(chi[0], ref["chi"], bnd["chi"])) <= 1
    assert report("%s %s chi2 per prior" % (name, kind), kr.ratio(ec, ref["edge_chi"], bnd["edge_chi"])) <= 1
    assert np.all(ec[~ref["counts"]] == 0)
    # the add entry on pre-filled blocks (not symmetric: it ADDS to all nine entries)
    rng = np.random.default_rng(5)
    H0, b0 = rng.normal(0, 3, (L, 9)), rng.normal(0, 3, (L, 3))
    H1, b1, chi_add = run_add(ctx, ev, d_lms, H0, b0)
    assert same_bits(chi_add, chi), "the chi2 of the add entry has other bits than the error entry's"
    none = np.asarray(ref["Hll_n"]).reshape(L) == 0
    assert none.any() and same_bits(H1[none], H0[none]) and same_bits(b1[none], b0[none])
    H0m, gotH = kr.from_colmajor(H0, 3, 3), kr.from_colmajor(H1, 3, 3)
    bH = kr.bound(ref["Hll_n"], LR.C_HLL, ref["Hll_mass"] + np.abs(H0m) * (~none)[:, None, None])
    bb = kr.bound(ref["bl_n"], LR.C_BL, ref["bl_mass"] + np.abs(b0) * (~none)[:, None])
    assert report("%s %s Hll (add entry)" % (name, kind), kr.ratio((gotH - H0m)[~none], ref["Hll"][~none], bH[~none])) <= 1
    assert report("%s %s bl (add entry)" % (name, kind), kr.ratio((b1 - b0)[~none], ref["bl"][~none], bb[~none])) <= 1
    # the same bits on a second call
    H2, b2, chi2 = run_add(ctx, ev, d_lms, H0, b0)
    assert same_bits(H1, H2) and same_bits(b1, b2) and same_bits(chi_add, chi2)
    chi3, ec3 = run_errors(ctx, ev, d_lms, n)
    assert same_bits(chi, chi3) and same_bits(ec, ec3)


@pytest.mark.parametrize("kind,f32,one_info", [("none", False, False), ("cauchy", False, True), ("huber", True, False),
                                               ("tukey", False, False)])
@pytest.mark.parametrize("name", ["D", "D_padded", "C"])
def test_build_pass_with_the_priors_inside(ctx, name, kind, f32, one_info):
    """cugo_construct_quadratic_form_lm_priors: Hll / bl bit-equal to the plain build pass followed by the add entry,
    Hpp / bp / Hpl bit-equal to the plain build pass, everything inside the joint bounds of the references"""
    f = layout(name)
    L = f["L"]
    pr, lay, order = priors(name, kind, one_info)
    info_sorted = pr["info"] if one_info else pr["info"][order]
    ref_p = LR.reference_build(f["lms"], L, dict(pr, lm=lay["lm"], z=pr["z"][order], info=info_sorted, active=pr["active"][order]))
    rk_ba = KERNELS[kind][1]
    ref_b = kr.build(None, rk_ba, f)
    both = LR.combined(ref_b, ref_p)
    bev = devmem.upload_edges(ctx, f)
    bev.block_f32 = int(f32)
    lev = upload_priors(ctx, f, pr, lay)
    assert lev.n_info == (1 if one_info else len(order))
    rkc = cugo.Robust(rk_ba[0], rk_ba[1], rk_ba[0], rk_ba[1])
    plain = run_build(ctx, f, bev, None, rkc, f32)
    fused = run_build(ctx, f, bev, lev, rkc, f32)
    for k in ("Hpp", "bp", "Hpl"):
        assert same_bits(plain[k], fused[k]), k
    d_lms = ctx.to_dev(f["lms"])
    H2, b2, chi_p = run_add(ctx, lev, d_lms, plain["Hll"], plain["bl"])
    assert same_bits(fused["Hll"], H2), "Hll: the fused pass and the two-call form differ"
    assert same_bits(fused["bl"], b2), "bl: the fused pass and the two-call form differ"
    # landmark 6 of D (all BA edges inactive, three priors) and the edgeless landmarks carry the priors alone
    gotH = kr.from_colmajor(fused["Hll"], 3, 3)
    assert report("%s %s Hll (priors inside)" % (name, kind), kr.ratio(gotH, both["Hll"], both["Hll_bound"])) <= 1
    assert report("%s %s bl (priors inside)" % (name, kind), kr.ratio(fused["bl"], both["bl"], both["bl_bound"])) <= 1
    assert report("%s %s chi2 (BA + priors)" % (name, kind), kr.ratio(fused["chi"][0], both["chi"], both["chi_bound"])) <= 1
    edgeless = np.diff(f["lm_ptr"])[:L] == 0
    with_prior = np.asarray(ref_p["Hll_n"]).reshape(L) > 0
    assert (edgeless & with_prior).any() and (edgeless & ~with_prior).any()
    assert np.all(fused["Hll"][edgeless & ~with_prior] == 0) and np.all(fused["bl"][edgeless & ~with_prior] == 0)
    assert np.abs(fused["Hll"][edgeless & with_prior]).max() > 0
    if name == "C":
        assert (np.flatnonzero(edgeless & with_prior) > f["E"]).any()
    # the same bits on a second call
    again = run_build(ctx, f, bev, lev, rkc, f32)
    for k in fused:
        assert same_bits(fused[k], again[k]), k
    # without flags (NULL: all active) the flagged priors count
    if kind == "none" and name == "D":
        lev0 = upload_priors(ctx, f, pr, lay, with_flags=False)
        all_on = LR.reference_build(f["lms"], L, dict(pr, lm=lay["lm"], z=pr["z"][order], info=info_sorted,
                                                      active=np.ones(len(order), bool)))
        chi, _ = run_errors(ctx, lev0, d_lms, len(order))
        assert kr.ratio(chi[0], all_on["chi"], LR.bounds(all_on)["chi"]) <= 1 and all_on["chi_n"] > ref_p["chi_n"]


def test_no_priors_is_the_plain_pass_and_launches_nothing(ctx):
    """n == 0: the entry with the priors inside is the plain build pass bit for bit; the stand-alone entries write chi2 = 0
    ... of nothing: they launch nothing and leave Hll / bl alone"""
    f = layout("D")
    L = f["L"]
    bev = devmem.upload_edges(ctx, f)
    rkc = cugo.Robust(0, 1.0, 0, 1.0)
    ev = cugo.LmPriorEdges()
    ev.n_landmarks_total, ev.n_landmarks_free, ev.n = f["Lall"], L, 0
    ev.d_lm_ptr = ctx.to_dev(np.zeros(f["Lall"] + 1, np.int32))
    ev.n_info, ev.rk, ev.delta = 1, 0, 1.0
    plain = run_build(ctx, f, bev, None, rkc)
    fused = run_build(ctx, f, bev, ev, rkc)
    for k in plain:
        assert same_bits(plain[k], fused[k]), k
    H0, b0 = np.random.default_rng(1).normal(size=(L, 9)), np.zeros((L, 3))
    Hll, bl = ctx.to_dev(H0), ctx.to_dev(b0)
    cugo.lm_prior_construct_quadratic_form(ctx.h, ev, ctx.to_dev(f["lms"]), Hll, bl, None)
    assert same_bits(ctx.to_host(Hll, H0.shape), H0)


def test_bad_layouts_are_refused(ctx):
    f = layout("D")
    pr, lay, order = priors("D", "none")
    d_lms = ctx.to_dev(f["lms"])
    chi = nan_dev(ctx, 2)

    def refused(change, match):
        bad = {k: v.copy() for k, v in lay.items()}
        p = dict(pr)
        tot = change(bad, p)
        ev = upload_priors(ctx, f, p, bad)
        if tot is not None:
            ev.n_landmarks_total, ev.n_landmarks_free = tot
        with pytest.raises(cugo.CugoError, match=match):
            cugo.lm_prior_compute_errors(ctx.h, ev, d_lms, chi, None)
        with pytest.raises(cugo.CugoError, match=match):
            cugo.lm_prior_construct_quadratic_form(ctx.h, ev, d_lms, nan_dev(ctx, 9 * f["L"]), nan_dev(ctx, 3 * f["L"]), None)
        return ev

    def short_ptr(b, p):
        b["lm_ptr"][-1] -= 1
    refused(short_ptr, "lm_ptr does not span")

    def descending(b, p):
        b["lm_ptr"][3] = b["lm_ptr"][2] - 1
    refused(descending, "lm_ptr not ascending")

    def unsorted(b, p):
        b["lm"][[0, -1]] = b["lm"][[-1, 0]]
    refused(unsorted, "not sorted by landmark")

    def out_of_range(b, p):
        b["lm"][5] = f["Lall"] + 3
    refused(out_of_range, "landmark index disagrees")

    def negative(b, p):
        b["lm"][5] = -1
    refused(negative, "landmark index disagrees")

    def bad_kernel(b, p):
        p["rk"] = (7, 1.0)
    refused(bad_kernel, "unknown robust kernel")

    def bad_delta(b, p):
        p["rk"] = (3, -1.0)
    refused(bad_delta, "unknown robust kernel or bad delta")
    refused(lambda b, p: (3, 5), "bad landmark or edge counts")
    # the entry with the priors inside: the same checks, and the priors must describe the landmarks of the edges
    bev = devmem.upload_edges(ctx, f)
    rkc = cugo.Robust(0, 1.0, 0, 1.0)
    P, L, E = f["P"], f["L"], f["E"]
    out = [nan_dev(ctx, k) for k in (36 * P, 6 * P, 9 * L, 3 * L, 18 * E)]
    d_poses = ctx.to_dev(f["poses"])
    good = upload_priors(ctx, f, pr, lay)
    good.n_landmarks_free -= 1
    with pytest.raises(cugo.CugoError, match="do not describe the landmarks"):
        cugo.construct_quadratic_form_lm_priors(ctx.h, bev, good, d_poses, d_lms, rkc, *out, None)
    bad = {k: v.copy() for k, v in lay.items()}
    unsorted(bad, None)
    with pytest.raises(cugo.CugoError, match="not sorted by landmark"):
        cugo.construct_quadratic_form_lm_priors(ctx.h, bev, upload_priors(ctx, f, pr, bad), d_poses, d_lms, rkc, *out, None)
    # nothing was written by a refused call
    assert np.all(np.isnan(ctx.to_host(out[2], 9 * L)))
