"""CPU checks of tests/lm_cov_ref.py and tests/lm_cov_designed.py (no GPU): they pin the extended-precision reference of
the landmark covariance kernel, its per-entry bound and the designs before test_lm_cov.py holds k_lm_covariance
against them.

* every design is legal (designed.check_layout) and has what it was built for (lm_cov_designed.check_design);
* K_LM: a float64 run of the reference's own formula (numpy, another summation order than the kernel's) against the
  longdouble run, in units of (n + C_LM) u sqrt(cond Hll) mass; lm_cov_ref.K_LM is 4 x the largest ratio over all
  designs, rounded up; the per-design ratios are recorded in lm_cov_ref.REPLAY;
* the form of kappa_l: on `far` the ratio per decade of cond(Hll) in units without kappa, with its square root and with
  cond itself;
* the bound sees an error: for every landmark of degree >= 2 in B, mixed and corners (and far), dropping the one
  off-diagonal (e, f) term of median magnitude, transposing the Sigma block of that term, or reading the neighbouring
  CSR block in its place each move the reference by more than 100 x the entry bound somewhere in the block.

Measured where this was written (x86-64, 80-bit longdouble), replay's worst ratio per design in the unit above:
  see lm_cov_ref.REPLAY;  far, per decade of cond(Hll) 1e4 .. 1e10: without kappa 0.0045 .. 0.0084 (flat), with
  sqrt(cond) 3e-5 falling to 3e-8, with cond 1.6e-7 falling to 2e-13.
  smallest margin of the three changes, in bounds: B 5.9e4, mixed 5.8e8, corners 1.4e8; far: 36 of 48 landmarks above
  100, the ten beyond depth 400 and two of the deepest before it below (FAR_EXEMPT).
"""
import numpy as np
import pytest

import designed
import kernel_ref as kr
import lm_cov_designed as ld
import lm_cov_ref as lr

# `far`: landmarks that do not clear the margin of 100 bounds under some change.  Their bound is wide: sqrt(cond Hll) is
# 1e3 .. 1e5 there, and Hpl_e annihilates the weak (depth) direction of Hll, so L^-T (G_e^T Sigma G_f) L^-1 cancels to
# about mass / cond while the near-identical cameras make Sigma_ef almost symmetric.  At most a quarter of the
# design's landmarks.
FAR_EXEMPT = (30, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47)


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(name):
        if name not in cache:
            des = ld.design(name)
            cache[name] = (des, lr.reference(des["f"], des["rowptr"], des["colind"], des["Hll"], des["Hpl"], des["sigma"]))
        return cache[name]
    return get


@pytest.mark.parametrize("name", ld.NAMES)
def test_designs_are_legal_and_as_designed(name):
    des = ld.design(name)
    designed.check_layout(des["f"])
    ld.check_design(des)
    f = des["f"]
    assert f["L"] <= 600 and (f["P"] <= 40 or name.startswith("B"))
    assert max(len(lr.counted_slots(f, l)) for l in range(f["L"])) <= 300


def test_replay_ratios_and_k_lm(refs):
    """lm_cov_ref.K_LM = 4 x the largest ratio of the float64 replay, rounded up; the unit is right if that is <= 64"""
    worst = {}
    for name in ld.NAMES:
        des, ref = refs(name)
        by_order = {}
        for order in ("rows", "pairs"):
            r64 = lr.reference(des["f"], des["rowptr"], des["colind"], des["Hll"], des["Hpl"], des["sigma"], dtype=np.float64,
                               order=order)
            sure = ~ref["marginal"]
            assert np.array_equal(r64["fail"][sure], ref["fail"][sure]), name
            by_order[order] = float(lr.ratios(np.where(ref["marginal"][:, None, None], 0, r64["cov"]), ref, lr.unit(ref)).max())
        worst[name] = max(by_order.values())
        print("%-9s fp64 replay: worst ratio %.3g (rows first) %.3g (pair by pair) of (n + C_LM) u sqrt(cond) mass (recorded "
              "%.3g), %d failed, %d marginal" % (name, by_order["rows"], by_order["pairs"], lr.REPLAY[name], ref["fail"].sum(),
                                                 ref["marginal"].sum()))
    k = 4 * max(worst.values())
    print("K_LM: 4 x %.3g = %.3g (lm_cov_ref.K_LM = %g)" % (max(worst.values()), k, lr.K_LM))
    assert k <= lr.K_LM <= 64 and lr.K_LM <= 2 * k + 0.01
    # the record: Sigma comes from numpy.linalg.inv, whose roundings differ from one BLAS to the next, and with it the
    # designs' last bits; the ratios move by a small factor, the record holds to that
    for name in ld.NAMES:
        assert worst[name] <= 4 * lr.REPLAY[name], name


def test_failed_and_marginal_landmarks(refs):
    """B: the edgeless free landmarks fail (Hll = 0 exactly), the landmark that one mono edge sees is marginal (a rank-2
    Hll), nothing else is; no other design has either"""
    for name in ld.NAMES:
        des, ref = refs(name)
        f = des["f"]
        if name.startswith("B"):
            slots = np.diff(f["lm_ptr"])[:f["L"]]
            real = np.array([int(((f["flags"][f["lm_ptr"][l]:f["lm_ptr"][l + 1]] & 8) == 0).sum()) for l in range(f["L"])])
            assert np.array_equal(ref["fail"], real == 0) and ref["fail"].sum() == 5 and (slots[ref["fail"]] == 0).sum() >= 4
            assert not np.any(des["Hll"][ref["fail"]])
            for l in np.flatnonzero(ref["marginal"]):
                es = np.arange(f["lm_ptr"][l], f["lm_ptr"][l + 1])
                es = es[(f["flags"][es] & 8) == 0]
                assert len(es) == 1 and not f["flags"][es[0]] & 4, l
        else:
            assert not ref["fail"].any() and not ref["marginal"].any(), name


def test_fixed_poses_only_gives_inverse_hll(refs):
    """mixed: the landmark that fixed poses alone see has no counted edge; its block is Hll^-1, the identity term"""
    des, ref = refs("mixed")
    l7 = int(des["f"]["lidx"][7])
    assert ref["deg"][l7] == 0 and ref["n"][l7] == 0
    inv = kr.inv3(np.asarray(des["Hll"][l7:l7 + 1], kr.LD))[0]
    assert np.abs(ref["cov"][l7] - inv).max() <= 1e-17 * ref["kappa"][l7] * np.abs(inv).max()


def test_form_of_kappa_on_far(refs):
    """the replay's ratio per decade of cond(Hll) in the three candidate units: flat without kappa, falling with its
    square root, falling twice as fast with cond itself: the square root is the smaller form that holds"""
    des, ref = refs("far")
    r64 = lr.reference(des["f"], des["rowptr"], des["colind"], des["Hll"], des["Hpl"], des["sigma"], dtype=np.float64)
    dec = np.floor(np.log10(ref["kappa"])).astype(int)
    assert dec.max() - dec.min() >= 6
    table = {}
    for pw in (0.0, 0.5, 1.0):
        r = lr.ratios(r64["cov"], ref, lr.unit(ref, pw))
        table[pw] = [float(r[dec == k].max()) for k in range(dec.min(), dec.max() + 1) if (dec == k).any()]
        print("far, unit kappa^%.1f, worst ratio per decade of cond(Hll) from 1e%d: %s"
              % (pw, dec.min(), " ".join("%.2g" % v for v in table[pw])))
    lo, hi = dec <= dec.min() + 1, dec >= dec.max() - 1
    r0, rs = lr.ratios(r64["cov"], ref, lr.unit(ref, 0.0)), lr.ratios(r64["cov"], ref, lr.unit(ref, 0.5))
    assert r0[hi].max() <= 16 * r0[lo].max()      # no growth left for a kappa to carry ...
    assert rs[hi].max() <= rs[lo].max()           # ... so with sqrt(cond) the ill-conditioned end is the slack one


# ------------------------------------------------------------------ the bound sees a subtle error
def changes(des, ref, l):
    """margins (largest |moved - ref| / bound over the block) of the three changes on landmark l, and the pair"""
    f = des["f"]
    es = lr.counted_slots(f, l)
    ps = f["pose"][es]
    look = lr.BlockLookup(des["rowptr"], des["colind"], des["sigma"], kr.LD)
    _, _, Li, G, S = lr.landmark(des["Hll"][l], des["Hpl"][es], ps, look)
    Li64, G64, S64 = (np.asarray(a, np.float64) for a in (Li, G, S))
    T = np.einsum("eka,efkl,flb->efab", G64 @ Li64, S64, G64 @ Li64)     # the terms as they enter the block
    mag = np.abs(T).reshape(len(es), len(es), 9).max(2)
    ee, ff = np.nonzero(~np.eye(len(es), dtype=bool))
    order = np.argsort(mag[ee, ff], kind="stable")
    e, g = int(ee[order[len(order) // 2]]), int(ff[order[len(order) // 2]])
    k, _ = look.index(ps[e:e + 1], ps[g:g + 1])
    kn = int(k[0]) + 1 if int(k[0]) + 1 < len(des["colind"]) else int(k[0]) - 1
    own = S[e, g]
    moved = {"dropped": 0 * own, "transposed": own.T, "neighbour": look.get(ps[e:e + 1], ps[g:g + 1], k=np.array([kn]))[0]}
    bnd = lr.bound(ref)[l]
    out = {}
    for what, Sm in moved.items():
        delta = Li.T @ (G[e].T @ (Sm - own) @ G[g]) @ Li
        out[what] = float((np.abs(delta) / bnd).max())
    return out, (e, g)


@pytest.mark.parametrize("name", ld.MUTATED + ("far",))
def test_bound_sees_a_dropped_term_a_transposed_block_and_a_neighbouring_block(name, refs):
    des, ref = refs(name)
    f = des["f"]
    todo = [l for l in range(f["L"]) if ref["deg"][l] >= 2 and not ref["fail"][l]]
    assert len(todo) >= 10
    low, below = {}, []
    for l in todo:
        m, pair = changes(des, ref, l)
        for what, v in m.items():
            low[what] = min(low.get(what, np.inf), v)
        if min(m.values()) <= 100:
            below.append(l)
    print("%s: %d landmarks of degree >= 2 (largest %d); smallest margin in bounds: %s; below 100: %s"
          % (name, len(todo), ref["deg"][todo].max(), ", ".join("%s %.3g" % kv for kv in low.items()), below))
    if name == "far":
        assert len(FAR_EXEMPT) <= f["L"] // 4 and set(below) <= set(FAR_EXEMPT), below
    else:
        assert not below, below
