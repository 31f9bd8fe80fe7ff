"""Designed layouts with camera-model tables (Kannala-Brandt fisheye entries; cugo_edges.has_rig = 2, DESIGN.md section
19): the rig layouts of tests/rig_designed.py with a model per camera-table entry, a hand-placed set of points round
every special place of the term, and a ring scene of four fisheye cameras.  attach() writes cam_tab ([n][17]) next to
cams / cam_ext / cam_id, makes every slot on a Kannala-Brandt entry a MONO slot (a stereo slot there is not defined)
and re-measures it (the fisheye projection at the design's geometry plus pixel noise).  Every pattern asserts its
census on the design it is used on, here, on the CPU.

Patterns (the slots' entries are those of the rig pattern named in brackets):
    "all"        [third]  every entry Kannala-Brandt: no pinhole slot, no stereo slot
    "third"      [third]  every third real slot on a Kannala-Brandt entry (1..4) among pinhole slots (entry 0, identity):
                          both kinds share a wave
    "blocks"     [blocks] every slot of every second whole 256-slot block on the Kannala-Brandt entry 2
    "beyond"     [beyond] only the slots of block-straddling landmarks beyond their owner's block (k_build_edges'
                          re-computation) on the Kannala-Brandt entry 3
    "one"        a one-entry table (n_cams == 1, d_cam == NULL): Kannala-Brandt with the IDENTITY sensor pose
    "many"       [many]   a 300-entry table (indices above 255 occur), odd entries Kannala-Brandt; entries 298 / 299 share
                          intrinsics, sensor pose and k1..k3 and differ in k4 alone
    "pinhole"    [third]  every model a pinhole, under has_rig = 2: the bits of has_rig = 1
Coefficients: K_ZERO (the equidistant model) and K_TYP (|k| of 1e-2 .. 1e-3, mixed signs), in turn over the entries.
"""
import functools

import numpy as np

import designed
import devmem
import fisheye_ref as fr
import rig_designed as rd

STEREO, INACTIVE = 4, 8
PATTERNS = ("all", "third", "blocks", "beyond", "one", "many", "pinhole")
BASE = dict(all="third", third="third", blocks="blocks", beyond="beyond", one="one", many="many", pinhole="third")
K_ZERO = np.zeros(4)
K_TYP = np.array([-0.0131, 0.0212, -0.0071, 0.0012])
K_TYP2 = np.array([0.0342, -0.0094, 0.0038, -0.0009])
PIXEL_SIGMA = 1.0


def kb_project(Xs, cam, k):
    """float64 Kannala-Brandt projection (plain quotient form: measurements only)"""
    r = np.hypot(Xs[:, 0], Xs[:, 1])
    th = np.arctan2(r, Xs[:, 2])
    t2 = th * th
    thd = th * (1 + t2 * (k[:, 0] + t2 * (k[:, 1] + t2 * (k[:, 2] + t2 * k[:, 3]))))
    with np.errstate(all="ignore"):
        rho = np.where(r > 0, thd / np.where(r > 0, r, 1.0), 1.0 / Xs[:, 2])
    return cam[:, 0] * rho * Xs[:, 0] + cam[:, 2], cam[:, 1] * rho * Xs[:, 1] + cam[:, 3]


def pattern_models(name, n):
    """model_k5 [n][5] = (k1, k2, k3, k4, model) of the pattern for a table of n entries"""
    m = np.zeros((n, 5))
    ks = (K_ZERO, K_TYP, K_TYP2)
    if name == "all":
        for k in range(n):
            m[k] = np.concatenate([ks[k % 3], [1.0]])
    elif name == "third":
        for k in range(1, n):
            m[k] = np.concatenate([ks[k % 3], [1.0]])
    elif name == "blocks":
        m[2] = np.concatenate([K_TYP, [1.0]])
    elif name == "beyond":
        m[3] = np.concatenate([K_TYP2, [1.0]])
    elif name == "one":
        m[0] = np.concatenate([K_TYP, [1.0]])
    elif name == "many":
        for k in range(1, n, 2):
            m[k] = np.concatenate([ks[(k // 2) % 3], [1.0]])
        m[298] = np.concatenate([K_TYP, [1.0]])
        m[299] = m[298]
        m[299, 3] = K_TYP[3] * 1.5
    elif name != "pinhole":
        raise KeyError(name)
    return m


def attach(f, model_k5, seed=0):
    """f: a rig case (rig_designed.attach).  Returns a copy with cam_tab, mono flags and fisheye measurements on the
    slots of Kannala-Brandt entries"""
    g = dict(f)
    tab = fr.model_table(f["cam_ext"], model_k5)
    g["cam_tab"] = tab
    cid = np.asarray(f["cam_id"], np.int64)
    fish = tab[cid, 16] != 0
    real = np.asarray(f["src"]) >= 0
    g["flags"] = np.where(fish, f["flags"] & ~np.uint8(STEREO), f["flags"]).astype(np.uint8)
    q = f["poses"][f["pose"]]
    X = f["lms"][f["lm"]]
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]).transpose(2, 0, 1)
    Xb = np.einsum("eij,ej->ei", R, X) + q[:, 4:]
    Xs = np.einsum("eij,ej->ei", tab[cid, :9].reshape(-1, 3, 3), Xb) + tab[cid, 9:12]
    redo = np.flatnonzero(real & fish)
    rng = np.random.default_rng(3000 + seed)
    pu, pv = kb_project(Xs[redo], np.asarray(f["cams"])[cid[redo]], tab[cid[redo], 12:16])
    noise = rng.normal(0.0, PIXEL_SIGMA, (2, len(redo)))
    g["meas"] = f["meas"].copy()
    g["meas"][0, redo], g["meas"][1, redo], g["meas"][2, redo] = pu + noise[0], pv + noise[1], 0.0
    g["fish"] = fish
    return g


@functools.lru_cache(maxsize=None)
def case(design, pattern, fused=False):
    """(flattened dict with the pattern's model table, hsc structure); built once, never modified"""
    f, hs = rd.case(design, BASE[pattern], fused)
    m = pattern_models(pattern, len(f["cams"]))
    if pattern == "one":
        f = dict(f, cam_ext=fr.IDENTITY12[None, :].copy())
    if pattern == "many":       # 298 / 299 share everything but k4
        ext, cams = f["cam_ext"].copy(), f["cams"].copy()
        ext[299], cams[299] = ext[298], cams[298]
        f = dict(f, cam_ext=ext, cams=cams)
    g = attach(f, m, seed=PATTERNS.index(pattern))
    act = (np.asarray(g["src"]) >= 0) & ((g["flags"] & INACTIVE) == 0)
    n_fish, n_pin = int((g["fish"] & act).sum()), int((~g["fish"] & act).sum())
    if pattern == "pinhole":
        assert n_fish == 0
    elif pattern in ("all", "one"):
        assert n_pin == 0 and n_fish >= 100 and not np.any(g["flags"][act] & STEREO)
    else:
        assert n_fish >= 1 and n_pin >= 1, (pattern, n_fish, n_pin)
    if pattern == "many":
        t = g["cam_tab"]
        assert np.array_equal(t[298, :15], t[299, :15]) and t[298, 15] != t[299, 15] and np.array_equal(g["cams"][298], g["cams"][299])
        assert g["cam_id"].max() > 255 and {298, 299} <= set(g["cam_id"][act].tolist())
    return g, hs


# "beyond" needs straddling landmarks, which the engine's padded layouts never have
PLAIN_CASES = (("A", "all"), ("A", "third"), ("A", "blocks"), ("A", "beyond"), ("B", "beyond"), ("A", "one"), ("A", "many"),
               ("A", "pinhole"))
FUSED_CASES = (("A", "all"), ("A", "third"), ("A", "blocks"), ("A", "one"), ("A", "many"), ("A", "pinhole"), ("B_plan", "third"))


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
    f["fish"] = f["cam_tab"][f["cam_id"], 16] != 0
    if meas is not None:
        f["meas"] = np.ascontiguousarray(meas, np.float64)
    designed.check_layout(f)
    return f


def _dir(th, phi, R):
    return np.array([R * np.sin(th) * np.cos(phi), R * np.sin(th) * np.sin(phi), R * np.cos(th)])


TINY = 3 * 2.0 ** -1074           # three ulp of 0
HAND_NAMES, HAND_POINTS = zip(*(
    ("r = 0", (0.0, 0.0, 5.0)),
    ("r = 0, near", (0.0, 0.0, 0.25)),
    ("x = 0", (0.0, 0.7, 4.0)),
    ("y = 0", (-0.3, 0.0, 4.0)),
    ("s^2 = 1e-24", (3e-12, -4e-12, 5.0)),
    ("s^2 = 1e-12", (3e-6, 4e-6, 5.0)),
    ("s^2 = 1e-8", (3e-4, -4e-4, 5.0)),
    ("s^2 = 1e-4", (0.03, 0.04, 5.0)),
    ("s^2 = 1e-2", (-0.3, 0.4, 5.0)),
    ("theta = 0.25", tuple(_dir(0.25, 0.7, 6.0))),
    ("switch - 1e-3", tuple(_dir(0.499, 2.1, 7.0))),
    ("switch - 1e-9", tuple(_dir(0.5 - 1e-9, -1.0, 3.0))),
    ("switch + 1e-9", tuple(_dir(0.5 + 1e-9, -1.0, 3.0))),
    ("switch + 1e-3", tuple(_dir(0.501, 2.1, 7.0))),
    ("theta = pi / 4", tuple(_dir(np.pi / 4, 0.3, 9.0))),
    ("theta = pi / 4 + 1e-6", tuple(_dir(np.pi / 4 + 1e-6, -2.6, 2.0))),
    ("theta = 1.2", tuple(_dir(1.2, 1.9, 4.0))),
    ("z = +3 ulp of 0", (1.5, -2.0, TINY)),
    ("z = -3 ulp of 0", (1.5, -2.0, -TINY)),
    ("z = 0", (-2.0, 1.0, 0.0)),
    ("z = +1e-16", (0.8, 0.6, 1e-16)),
    ("z = -1e-16", (0.8, 0.6, -1e-16)),
    ("theta = 1.7", tuple(_dir(1.7, -0.4, 5.0))),
    ("theta = 1.9", tuple(_dir(1.9, 2.9, 3.0))),
    ("theta = 1.9, x = 0", (0.0, 3.0 * np.sin(1.9), 3.0 * np.cos(1.9))),
))
# the points at which the quotient form of c has lost more digits (~ u / s^2) than the bounds allow (~ 1500 u)
HAND_NEAR_AXIS = tuple(i for i, n in enumerate(HAND_NAMES) if n in ("s^2 = 1e-24", "s^2 = 1e-12", "s^2 = 1e-8"))


@functools.lru_cache(maxsize=None)
def hand_points():
    """the hand-placed points, each a landmark seen by two free body poses at the origin (identity: Xb = Xw exactly)
    through two Kannala-Brandt entries with the identity sensor pose (Xs = Xb exactly): entry 0 equidistant (pose 0),
    entry 1 K_TYP (pose 1).  Measurements: the projection + a few pixels, so that e is of ordinary size"""
    lms = np.array(HAND_POINTS, np.float64)
    n = len(lms)
    poses = np.tile(np.array([0, 0, 0, 1, 0, 0, 0], np.float64), (2, 1))
    cams = np.array([[400.0, 410.0, 320.0, 240.0, 0.0], [380.0, 375.0, 330.0, 250.0, 0.0]])
    tab = fr.model_table(np.tile(fr.IDENTITY12, (2, 1)), [np.concatenate([K_ZERO, [1.0]]), np.concatenate([K_TYP, [1.0]])])
    pose_i, lm_i = np.repeat([0, 1], n), np.tile(np.arange(n), 2)
    f = small_flat(poses, 2, lms, pose_i, lm_i, pose_i, cams, tab)
    rng = np.random.default_rng(11)
    pu, pv = kb_project(lms[f["lm"]], cams[f["cam_id"]], tab[f["cam_id"], 12:16])
    f["meas"] = np.ascontiguousarray(np.stack([pu + rng.normal(0, 2.0, f["E"]), pv + rng.normal(0, 2.0, f["E"]), np.zeros(f["E"])]))
    assert np.all(np.isfinite(f["meas"]))
    return f, devmem.hsc_structure(f)


RING_K = (K_TYP, K_ZERO, K_TYP2, K_TYP * 0.5)


@functools.lru_cache(maxsize=None)
def ring_scene(noise=0.5, wide=110.0):
    """rig_designed.ring_scene's geometry (24 landmarks on a ring of 6 m round the body, four cameras at 0 / 90 / 180 /
    270 degrees of yaw with lever arms, three body poses, one fixed) with four Kannala-Brandt cameras of different
    coefficients; the cameras within `wide` degrees of a landmark see it from the three poses in turn, so each
    camera sees landmarks beyond 90 degrees off its axis (Z_s < 0).  Mono slots, exact measurements + `noise` px"""
    base = rd.ring_scene()
    nl = base["Lall"]
    cams = np.tile(np.array([400.0, 410.0, 320.0, 240.0, 0.0]), (4, 1)) * np.array([1.0, 1.01, 0.99, 1.02])[:, None]
    tab = fr.model_table(base["cam_ext"], [np.concatenate([k, [1.0]]) for k in RING_K])
    ang = 2 * np.pi * (np.arange(nl) + 0.5) / nl
    pose_i, lm_i, cam_i = [], [], []
    for l in range(nl):
        off = [np.rad2deg(abs((ang[l] - k * np.pi / 2 + np.pi) % (2 * np.pi) - np.pi)) for k in range(4)]
        sees = [k for k in range(4) if off[k] < wide]
        for p in range(3):      # (a pose sees a landmark once: the cameras that see it take the poses in turn)
            pose_i.append(p), lm_i.append(l), cam_i.append(sees[(l + p) % len(sees)])
    f = small_flat(base["poses"], 2, base["lms"], pose_i, lm_i, cam_i, cams, tab)
    ref = fr.build(f, dict(mono=(0, 1.0), stereo=(0, 1.0)), dtype=np.float64)
    zs = ref["Xs"][:, 2]
    for k in range(4):
        assert (zs[f["cam_id"] == k] < -0.3).sum() >= 2, "camera %d sees nothing beyond 90 degrees" % k
    th = np.arctan2(np.hypot(ref["Xs"][:, 0], ref["Xs"][:, 1]), zs)
    assert th.max() < 2.1 and th.max() > 1.7
    rng = np.random.default_rng(7)
    meas = np.asarray(ref["e"]).T + rng.normal(0, noise, (3, f["E"]))       # (with meas = 0 the residual is the projection)
    meas[2] = 0.0
    f["meas"] = np.ascontiguousarray(meas)
    return f
