"""Designed layouts with distortion tables (radial-tangential lens distortion; cugo_edges.has_rig = 3, DESIGN.md section
20): the rig layouts of tests/rig_designed.py with a distortion per camera-table entry and a hand-placed set of points
round every special place of the term.  attach() writes cam_tab ([n][18]) next to cams / cam_ext / cam_id and re-measures
every slot on a distorted entry (the distorted projection at the design's geometry plus pixel noise).  Except in the
pattern "all" it also makes such a slot a MONO slot, as the graph level would have it; "all" keeps the design's stereo
bits on distorted entries, where they are not looked at for the rows (and still pick the robust kernel).  Every pattern
asserts its census on the design it is used on, here, on the CPU.

Patterns (the slots' entries are those of the rig pattern named in brackets):
    "all"        [third]  every entry distorted: no undistorted slot; slots with the stereo bit among them
    "third"      [third]  every third real slot on a distorted entry (1..4) among undistorted slots (entry 0, identity),
                          the design's stereo slots among the latter: both kinds share a wave
    "blocks"     [blocks] every slot of every second whole 256-slot block on the distorted entry 2
    "beyond"     [beyond] only the slots of block-straddling landmarks beyond their owner's block (k_build_edges'
                          re-computation) on the distorted entry 3
    "one"        a one-entry table (n_cams == 1, d_cam == NULL): distorted with the IDENTITY sensor pose
    "many"       [many]   a 300-entry table (indices above 255 occur), odd entries distorted; entries 298 / 299 share
                          intrinsics, sensor pose and k1, k2, p1, p2 and differ in k3 alone
    "plain"      [third]  every flag 0 (the coefficients there all the same: they must not be read), under has_rig = 3:
                          the bits of has_rig = 1
Coefficients (k1, k2, p1, p2, k3): D_TYP (a barrel lens as calibrations give it), D_TYP2 (pincushion, other signs) and
D_TAN (tangential only), in turn over the entries.  The designs see their landmarks within |X/Z|, |Y/Z| <= 0.41 of the
body, so r2 stays below about 0.6 behind the sensor poses.
"""
import functools

import numpy as np

import designed
import devmem
import distort_ref as dr
import rig_designed as rd

STEREO, INACTIVE = 4, 8
PATTERNS = ("all", "third", "blocks", "beyond", "one", "many", "plain")
BASE = dict(all="third", third="third", blocks="blocks", beyond="beyond", one="one", many="many", plain="third")
D_TYP = np.array([-0.28, 0.07, 0.002, -0.001, -0.01])
D_TYP2 = np.array([0.12, -0.21, -0.0007, 0.0013, 0.09])
D_TAN = np.array([0.0, 0.0, 0.003, -0.002, 0.0])
D_BARREL = np.array([-0.3, 0.0, 0.0, 0.0, 0.0])
D_K3 = np.array([0.0, 0.0, 0.0, 0.0, 0.05])
PIXEL_SIGMA = 1.0


def project(Xs, cam, d):
    """float64 distorted projection (measurements only)"""
    a, b = Xs[:, 0] / Xs[:, 2], Xs[:, 1] / Xs[:, 2]
    r2 = a * a + b * b
    rad = 1 + r2 * (d[:, 0] + r2 * (d[:, 1] + r2 * d[:, 4]))
    ad = a * rad + 2 * d[:, 2] * a * b + d[:, 3] * (r2 + 2 * a * a)
    bd = b * rad + d[:, 2] * (r2 + 2 * b * b) + 2 * d[:, 3] * a * b
    return cam[:, 0] * ad + cam[:, 2], cam[:, 1] * bd + cam[:, 3]


def pattern_distortions(name, n):
    """(dist5 [n][5], flags [n]) of the pattern for a table of n entries"""
    d = np.zeros((n, 5))
    ds = (D_TYP, D_TYP2, D_TAN)
    if name == "all":
        for k in range(n):
            d[k] = ds[k % 3]
    elif name == "third":
        for k in range(1, n):
            d[k] = ds[k % 3]
    elif name == "blocks":
        d[2] = D_TYP
    elif name == "beyond":
        d[3] = D_TYP2
    elif name == "one":
        d[0] = D_TYP
    elif name == "many":
        for k in range(1, n, 2):
            d[k] = ds[(k // 2) % 3]
        d[298] = D_TYP
        d[299] = d[298]
        d[299, 4] = D_TYP[4] * 1.5
    elif name == "plain":
        d[:] = D_TYP
        return d, np.zeros(n)
    else:
        raise KeyError(name)
    return d, np.any(d != 0, axis=1).astype(np.float64)


def attach(f, dist5, flags, seed=0, keep_stereo=False):
    """f: a rig case (rig_designed.attach).  Returns a copy with cam_tab and distorted measurements on the slots of
    distorted entries, which are mono slots unless keep_stereo"""
    g = dict(f)
    tab = dr.dist_table(f["cam_ext"], dist5, flags)
    g["cam_tab"] = tab
    cid = np.asarray(f["cam_id"], np.int64)
    dist = tab[cid, 17] != 0
    real = np.asarray(f["src"]) >= 0
    if not keep_stereo:
        g["flags"] = np.where(dist, f["flags"] & ~np.uint8(STEREO), f["flags"]).astype(np.uint8)
    q = f["poses"][f["pose"]]
    X = f["lms"][f["lm"]]
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]).transpose(2, 0, 1)
    Xb = np.einsum("eij,ej->ei", R, X) + q[:, 4:]
    Xs = np.einsum("eij,ej->ei", tab[cid, :9].reshape(-1, 3, 3), Xb) + tab[cid, 9:12]
    redo = np.flatnonzero(real & dist)
    rng = np.random.default_rng(4000 + seed)
    pu, pv = project(Xs[redo], np.asarray(f["cams"])[cid[redo]], tab[cid[redo], 12:17])
    noise = rng.normal(0.0, PIXEL_SIGMA, (2, len(redo)))
    g["meas"] = f["meas"].copy()
    g["meas"][0, redo], g["meas"][1, redo] = pu + noise[0], pv + noise[1]
    if not keep_stereo:
        g["meas"][2, redo] = 0.0
    g["dist"] = dist
    return g


@functools.lru_cache(maxsize=None)
def case(design, pattern, fused=False):
    """(flattened dict with the pattern's distortion table, hsc structure); built once, never modified"""
    f, hs = rd.case(design, BASE[pattern], fused)
    d, fl = pattern_distortions(pattern, len(f["cams"]))
    if pattern == "one":
        f = dict(f, cam_ext=dr.IDENTITY12[None, :].copy())
    if pattern == "many":       # 298 / 299 share everything but k3
        ext, cams = f["cam_ext"].copy(), f["cams"].copy()
        ext[299], cams[299] = ext[298], cams[298]
        f = dict(f, cam_ext=ext, cams=cams)
    g = attach(f, d, fl, seed=PATTERNS.index(pattern), keep_stereo=pattern == "all")
    act = (np.asarray(g["src"]) >= 0) & ((g["flags"] & INACTIVE) == 0)
    n_dist, n_und = int((g["dist"] & act).sum()), int((~g["dist"] & act).sum())
    st = (g["flags"] & STEREO) != 0
    if pattern == "plain":
        assert n_dist == 0 and np.all(g["cam_tab"][:, 12:17] != 0) and np.array_equal(g["meas"], f["meas"])
    elif pattern == "all":
        assert n_und == 0 and n_dist >= 100 and (st & act).sum() >= 10
    elif pattern == "one":
        assert n_und == 0 and n_dist >= 100 and not np.any(st & act)
    else:
        assert n_dist >= 1 and n_und >= 1 and not np.any(st & act & g["dist"]), (pattern, n_dist, n_und)
    if pattern == "third":
        assert (st & act & ~g["dist"]).sum() >= 10, "no stereo slot on an undistorted entry"
    if pattern == "many":
        t = g["cam_tab"]
        assert np.array_equal(t[298, :16], t[299, :16]) and t[298, 16] != t[299, 16] and np.array_equal(g["cams"][298], g["cams"][299])
        assert g["cam_id"].max() > 255 and {298, 299} <= set(g["cam_id"][act].tolist())
    return g, hs


# "beyond" needs straddling landmarks, which the engine's padded layouts never have
PLAIN_CASES = (("A", "all"), ("A", "third"), ("A", "blocks"), ("A", "beyond"), ("B", "beyond"), ("A", "one"), ("A", "many"),
               ("A", "plain"))
FUSED_CASES = (("A", "all"), ("A", "third"), ("A", "blocks"), ("A", "one"), ("A", "many"), ("A", "plain"), ("B_plan", "third"))


def robust2(design, which, fused=False):
    return rd.robust2(design, which, fused)


# ---- small hand-built layouts ------------------------------------------------------------------------------------------
def small_flat(poses, n_free, lms, pose_i, lm_i, cam_i, cams, tab, meas=None):
    """a flattened dict (landmark-major, every slot mono and active, every landmark free) of the observations
    (pose_i, lm_i, cam_i); poses [Pall][7] with the n_free free ones first"""
    pose_i, lm_i, cam_i = (np.asarray(a, np.int64) for a in (pose_i, lm_i, cam_i))
    order = np.lexsort((pose_i, lm_i))
    pose_i, lm_i, cam_i = pose_i[order], lm_i[order], cam_i[order]
    E, Pall, Lall = len(pose_i), len(poses), len(lms)
    flags = np.where(pose_i >= n_free, 2, 0).astype(np.uint8)
    f = dict(E=E, P=n_free, L=Lall, Pall=Pall, Lall=Lall, src=np.arange(E), pose=pose_i.astype(np.int32),
             lm=lm_i.astype(np.int32), flags=flags, meas=np.zeros((3, E)), omega=np.ones(E),
             cams=np.ascontiguousarray(cams, np.float64), cam_id=cam_i.astype(np.uint16),
             poses=np.ascontiguousarray(poses, np.float64), lms=np.ascontiguousarray(lms, np.float64))
    lp = np.zeros(Lall + 1, np.int64); np.add.at(lp, lm_i + 1, 1); f["lm_ptr"] = np.cumsum(lp).astype(np.int32)
    f["pose_edge"] = np.lexsort((lm_i, pose_i)).astype(np.int32)
    pp = np.zeros(Pall + 1, np.int64); np.add.at(pp, pose_i + 1, 1); f["pose_ptr"] = np.cumsum(pp).astype(np.int32)
    f["cam_tab"] = np.ascontiguousarray(tab, np.float64)
    f["cam_ext"] = np.ascontiguousarray(f["cam_tab"][:, :12])
    f["dist"] = f["cam_tab"][f["cam_id"], 17] != 0
    if meas is not None:
        f["meas"] = np.ascontiguousarray(meas, np.float64)
    designed.check_layout(f)
    return f


_S = np.sqrt
# entry 1 (D_BARREL, k1 = -0.3): rad = 1 - 0.3 r2 is 0.706 at r2 = 0.98 and changes sign at r2 = 10 / 3
HAND_NAMES, HAND_POINTS = zip(*(
    ("on the axis", (0.0, 0.0, 5.0)),
    ("on the axis, near", (0.0, 0.0, 0.25)),
    ("a = 0", (0.0, 0.7, 4.0)),
    ("b = 0", (-0.3, 0.0, 4.0)),
    ("r2 = 1e-12", (3e-6, 4e-6, 5.0)),
    ("r2 = 0.0325", (0.3, -0.2, 2.0)),
    ("r2 = 0.32", (-1.2, 1.2, 3.0)),
    ("r2 = 0.98", (2.1, 2.1, 3.0)),
    ("r2 = 0.98, a = 0", (0.0, -_S(0.98) * 2.0, 2.0)),
    ("rad > 0: r2 = 3.2", (_S(1.6) * 1.5, -_S(1.6) * 1.5, 1.5)),
    ("rad ~ 0: r2 = 10 / 3", (_S(5.0 / 3.0) * 2.5, _S(5.0 / 3.0) * 2.5, 2.5)),
    ("rad < 0: r2 = 3.5", (-_S(1.75) * 1.1, _S(1.75) * 1.1, 1.1)),
))
HAND_ENTRIES = (("typical", D_TYP), ("barrel k1", D_BARREL), ("tangential only", D_TAN), ("k3 only", D_K3))
HAND_RAD_SIGN = tuple(HAND_NAMES.index(n) for n in ("rad > 0: r2 = 3.2", "rad ~ 0: r2 = 10 / 3", "rad < 0: r2 = 3.5"))


@functools.lru_cache(maxsize=None)
def hand_points():
    """the hand-placed points, each a landmark seen by four free body poses at the origin (identity: Xb = Xw exactly)
    through four distorted entries with the identity sensor pose (Xs = Xb exactly, so JL = A): pose k through entry k of
    HAND_ENTRIES.  Measurements: the projection + a few pixels, so that e is of ordinary size"""
    lms = np.array(HAND_POINTS, np.float64)
    n, ne = len(lms), len(HAND_ENTRIES)
    poses = np.tile(np.array([0, 0, 0, 1, 0, 0, 0], np.float64), (ne, 1))
    cams = np.array([[500.0, 480.0, 320.0, 240.0, 0.0], [400.0, 410.0, 320.0, 240.0, 0.0], [380.0, 375.0, 330.0, 250.0, 0.0],
                     [450.0, 455.0, 300.0, 260.0, 0.0]])
    tab = dr.dist_table(np.tile(dr.IDENTITY12, (ne, 1)), [d for _, d in HAND_ENTRIES])
    pose_i, lm_i = np.repeat(np.arange(ne), n), np.tile(np.arange(n), ne)
    f = small_flat(poses, ne, lms, pose_i, lm_i, pose_i, cams, tab)
    rng = np.random.default_rng(11)
    pu, pv = project(lms[f["lm"]], cams[f["cam_id"]], tab[f["cam_id"], 12:17])
    f["meas"] = np.ascontiguousarray(np.stack([pu + rng.normal(0, 2.0, f["E"]), pv + rng.normal(0, 2.0, f["E"]), np.zeros(f["E"])]))
    assert np.all(np.isfinite(f["meas"]))
    a, b = lms[:, 0] / lms[:, 2], lms[:, 1] / lms[:, 2]
    rad = 1 + D_BARREL[0] * (a * a + b * b)
    i, j, k = HAND_RAD_SIGN
    assert rad[i] > 0.03 and abs(rad[j]) < 1e-12 and rad[k] < -0.03 and abs(rad[HAND_NAMES.index("r2 = 0.98")] - 0.706) < 1e-12
    return f, devmem.hsc_structure(f)
