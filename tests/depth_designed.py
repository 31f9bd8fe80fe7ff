"""Designed layouts with depth slots (flag bit 16): relabellings of the flattened designs of
tests/designed.py (layout, fused_layout).  A pattern is a function of the flattened design: it names the slots that
become depth slots; relabel() clears STEREO, sets DEPTH and sets meas[2] to 1/Z at the design's geometry plus noise.
Every pattern asserts its census on the design it is used on, here, on the CPU.

Patterns:
    "third"      every third real slot: mono, stereo and depth meet in every wave
    "blocks"     every slot of every second whole 256-slot block: a workgroup sees depth only
    "beyond"     the slots of block-straddling landmarks that lie beyond their owner's block (k_build_edges' re-computation)
    "poses"      every edge of the pose of degree 1025 and of a pose of degree 1 (layout A)
    "fixed"      the slots with FIXED_P or FIXED_L
    "inactive"   inactive slots carrying the DEPTH bit (and nothing else of the depth kind)
    "none"       no slot at all (with has_depth = 1)
"""
import functools

import numpy as np

import designed

STEREO, INACTIVE, DEPTH = 4, 8, 16
SIGMA_INV_DEPTH = 1e-3        # noise of the 1/Z measurement, inverse metres
PATTERNS = ("third", "blocks", "beyond", "poses", "fixed", "inactive", "none")
WEIGHTS = (1.0, 1e4)


def real_slots(f):
    """slots that hold an edge of the problem (the engine's padding slots have src < 0)"""
    return np.flatnonzero(np.asarray(f["src"]) >= 0)


def pattern_slots(name, f):
    E = f["E"]
    fl = f["flags"]
    real = real_slots(f)
    lp = f["lm_ptr"]
    if name == "third":
        slots = real[::3]
        kinds = np.where(np.isin(np.arange(E), slots), 2, (fl & STEREO) // STEREO)   # 0 mono, 1 stereo, 2 depth
        waves = [w for w in range(E // 64) if np.all(np.asarray(f["src"])[64 * w:64 * w + 64] >= 0) and
                 not np.any(fl[64 * w:64 * w + 64] & INACTIVE)]
        assert len(waves) >= 1
        for w in waves:
            assert set(kinds[64 * w:64 * w + 64].tolist()) == {0, 1, 2}, "wave %d does not hold all three kinds" % w
    elif name == "blocks":
        nb = E // 256
        assert nb >= 2, "the design has fewer than two whole 256-slot blocks"
        blocks = np.arange(1, nb, 2)
        slots = np.concatenate([np.arange(256 * b, 256 * b + 256) for b in blocks])
        slots = slots[np.isin(slots, real)]
        act = slots[(fl[slots] & INACTIVE) == 0]
        assert len(act) >= 200, "the depth-only blocks hold too few active slots"
    elif name == "beyond":
        st = designed.straddlers(f)
        assert len(st) >= 1, "the design has no block-straddling landmark"
        slots = np.concatenate([np.arange((lp[l] // 256 + 1) * 256, lp[l + 1]) for l in st])
        assert len(slots) >= 1 and np.any((fl[slots] & INACTIVE) == 0)
        assert any(l < f["L"] for l in st), "no straddling landmark is free: the owner's sum is never formed"
        # and nothing inside an owner's block is relabelled: the two paths stay apart
        assert not np.any(np.isin(slots, np.concatenate([np.arange(lp[l], (lp[l] // 256 + 1) * 256) for l in st])))
    elif name == "poses":
        deg = np.diff(f["pose_ptr"])
        big = np.flatnonzero(deg[:f["P"]] == 1025)
        one = np.flatnonzero(deg[:f["P"]] == 1)
        assert len(big) >= 1 and len(one) >= 1, "the design has no free pose of degree 1025 / 1"
        pe, pp = f["pose_edge"], f["pose_ptr"]
        slots = np.concatenate([pe[pp[big[0]]:pp[big[0] + 1]], pe[pp[one[0]]:pp[one[0] + 1]]])
        assert len(slots) == 1026
    elif name == "fixed":
        slots = np.flatnonzero((fl & 3) != 0)
        assert np.any(fl[slots] & 1) and np.any(fl[slots] & 2), "the design lacks FIXED_L or FIXED_P slots"
    elif name == "inactive":
        act = real[(fl[real] & INACTIVE) == 0]
        slots = act[5::97]
        assert len(slots) >= 1
    elif name == "none":
        slots = np.zeros(0, np.int64)
    else:
        raise KeyError(name)
    return np.asarray(slots, np.int64)


def relabel(f, slots, seed=0, inactive=False):
    """a copy of the flattened dict with `slots` as depth slots: STEREO cleared, DEPTH set, meas[2] = 1/Z of the slot at
    the design's geometry + N(0, SIGMA_INV_DEPTH); inactive: INACTIVE set on them as well"""
    g = dict(f)
    g["flags"] = f["flags"].copy()
    g["meas"] = f["meas"].copy()
    slots = np.asarray(slots, np.int64)
    if len(slots) == 0:
        return g
    q = f["poses"][f["pose"][slots]]
    X = f["lms"][f["lm"][slots]]
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    Z = 2 * (x * z - y * w) * X[:, 0] + 2 * (y * z + x * w) * X[:, 1] + (1 - 2 * (x * x + y * y)) * X[:, 2] + q[:, 6]
    assert np.all(Z > 0.1), "a relabelled slot has its landmark behind (or at) the camera"
    rng = np.random.default_rng(1000 + seed)
    g["flags"][slots] = (g["flags"][slots] & ~np.uint8(STEREO)) | np.uint8(DEPTH | (INACTIVE if inactive else 0))
    g["meas"][2, slots] = 1.0 / Z + rng.normal(0.0, SIGMA_INV_DEPTH, len(slots))
    return g


@functools.lru_cache(maxsize=None)
def _design(design, fused):
    if fused:
        _, f, hs = designed.fused_layout(design)
    else:
        _, _, f, hs = designed.layout(design)
        f = dict(f)
    if "src" not in f:
        f["src"] = np.arange(f["E"])
    return f, hs


@functools.lru_cache(maxsize=None)
def case(design, pattern, fused=False):
    """(flattened dict with the pattern's depth slots, hsc structure) of design `design` of designed.layout (fused:
    designed.fused_layout, the engine's padded slot layout); built once, never modified"""
    f, hs = _design(design, fused)
    slots = pattern_slots(pattern, f)
    g = relabel(f, slots, seed=PATTERNS.index(pattern), inactive=pattern == "inactive")
    n_depth = int(((g["flags"] & DEPTH) != 0).sum())
    assert n_depth == len(slots)
    if pattern == "inactive":
        assert np.all(g["flags"][slots] & INACTIVE)
    return g, hs


# which pattern goes on which design: (design, fused layout?) per pattern.  "beyond" needs straddling landmarks, which the
# engine's padded layouts never have; "poses" the degrees of layout A
PLAIN_CASES = (("A", "third"), ("A", "blocks"), ("A", "beyond"), ("B", "beyond"), ("A", "poses"), ("A", "fixed"),
               ("A", "inactive"), ("A", "none"))
FUSED_CASES = (("A", "third"), ("A", "blocks"), ("A", "poses"), ("A", "fixed"), ("A", "inactive"), ("A", "none"),
               ("B_plan", "third"))


@functools.lru_cache(maxsize=None)
def robust3(design, which, fused=False):
    """a robust kernel per kind, the depth kind's different from the other two, with the kinks where
    designed.robust_kernels / fused_robust_kernels place them"""
    rk = designed.fused_robust_kernels(design) if fused else designed.robust_kernels(design)
    if which == 0:
        return dict(mono=rk["none"], stereo=rk["huber"], depth=rk["tukey"])
    return dict(mono=rk["tukey"], stereo=rk["none"], depth=rk["huber"])
