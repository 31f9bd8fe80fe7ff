"""Designed layouts with camera extrinsics (a rig; cugo_edges.has_rig): the flattened designs of
tests/designed.py (layout, fused_layout) with a camera table and a table of sensor poses attached.  A pattern is a
function of the flattened design: it gives every slot a camera-table entry; attach() writes cams, cam_ext and cam_id
and re-measures the slots whose entry is not the design's own (projection through the sensor pose at the design's
geometry plus pixel noise).  Every pattern asserts its census on the design it is used on, here, on the CPU — among it
that every active slot has Z_s above MIN_DEPTH_FRACTION of its body-frame depth.

The sensor poses EXT[1..4] are general rotations (axes off every coordinate axis, 6 to 11 degrees) with lever arms of
0.3 to 0.5 m; EXT[0] is the identity.  The designs see their landmarks at 11 to 30 m within |X/Z|, |Y/Z| <= 0.41, so
Z_s >= Z_b (cos 11 deg - 2 x 0.41 sin 11 deg) - 0.5 > 0.75 Z_b.

Patterns:
    "third"      every third real slot on a non-identity entry (1..4 in turn): identity and non-identity share a wave
    "blocks"     every slot of every second whole 256-slot block on entry 2
    "beyond"     the slots of block-straddling landmarks beyond their owner's block on entry 3 (k_build_edges' re-computation)
    "poses"      every edge of the pose of degree 1025 on entry 1, of a pose of degree 1 on entry 4
    "one"        a one-entry table (n_cams == 1, d_cam == NULL) with sensor pose 1
    "many"       a 300-entry table (indices above 255 occur): entries 296 / 297 share the sensor pose and differ in the
                 intrinsics, 298 / 299 share the intrinsics and differ in the sensor pose
    "identity"   a three-entry table (different intrinsics) whose sensor poses are all the identity
    "stereo"     the stereo slots on non-identity entries, the mono slots on the identity
    "none"       the design's own one-entry table with the identity (the plain graph)
"""
import functools

import numpy as np

import designed
import rig_ref

STEREO, INACTIVE = 4, 8
PATTERNS = ("third", "blocks", "beyond", "poses", "one", "many", "identity", "stereo", "none")
MIN_DEPTH_FRACTION = 0.75
PIXEL_SIGMA = 1.0


def _axis_angle(axis, deg, t):
    a = np.asarray(axis, np.float64)
    a = a / np.sqrt((a * a).sum())
    h = np.deg2rad(deg) / 2
    return np.concatenate([np.sin(h) * a, [np.cos(h)], t])


# (qx, qy, qz, qw, tx, ty, tz), body -> sensor
SENSOR_POSES = (np.array([0, 0, 0, 1, 0, 0, 0], np.float64),
                _axis_angle((1, 2, -1), 8.0, (0.4, -0.1, 0.2)),
                _axis_angle((-2, 1, 3), 11.0, (-0.3, 0.25, -0.3)),
                _axis_angle((1, -1, 1), 6.0, (0.1, 0.45, 0.15)),
                _axis_angle((3, 1, 1), 9.0, (-0.35, -0.3, 0.1)))
EXT = np.stack([rig_ref.quat_to_ext(q) for q in SENSOR_POSES])


def real_slots(f):
    return np.flatnonzero(np.asarray(f["src"]) >= 0)


def pattern_table(name, f):
    """(cams [n][5], cam_ext [n][12], cam_id [E]) of the pattern on the flattened design f (one camera, f["cams"][0])"""
    E, fl = f["E"], f["flags"]
    real = real_slots(f)
    lp = f["lm_ptr"]
    c0 = np.asarray(f["cams"][0], np.float64)
    cams = np.tile(c0, (5, 1))
    ext = EXT.copy()
    cid = np.zeros(E, np.int64)
    if name == "third":
        slots = real[::3]
        cid[slots] = 1 + np.arange(len(slots)) % 4
        waves = [w for w in range(E // 64) if np.all(np.asarray(f["src"])[64 * w:64 * w + 64] >= 0)]
        assert len(waves) >= 1
        for w in waves:
            assert 0 in cid[64 * w:64 * w + 64] and np.any(cid[64 * w:64 * w + 64] > 0), "wave %d holds one kind only" % w
    elif name == "blocks":
        nb = E // 256
        assert nb >= 2, "the design has fewer than two whole 256-slot blocks"
        slots = np.concatenate([np.arange(256 * b, 256 * b + 256) for b in range(1, nb, 2)])
        slots = slots[np.isin(slots, real)]
        assert ((fl[slots] & INACTIVE) == 0).sum() >= 200
        cid[slots] = 2
    elif name == "beyond":
        st = designed.straddlers(f)
        assert len(st) >= 1 and any(l < f["L"] for l in st), "the design has no free block-straddling landmark"
        slots = np.concatenate([np.arange((lp[l] // 256 + 1) * 256, lp[l + 1]) for l in st])
        assert len(slots) >= 1 and np.any((fl[slots] & INACTIVE) == 0)
        cid[slots] = 3
    elif name == "poses":
        deg = np.diff(f["pose_ptr"])
        big, one = np.flatnonzero(deg[:f["P"]] == 1025), np.flatnonzero(deg[:f["P"]] == 1)
        assert len(big) >= 1 and len(one) >= 1, "the design has no free pose of degree 1025 / 1"
        pe, pp = f["pose_edge"], f["pose_ptr"]
        cid[pe[pp[big[0]]:pp[big[0] + 1]]] = 1
        cid[pe[pp[one[0]]:pp[one[0] + 1]]] = 4
    elif name == "one":
        cams, ext = cams[:1], EXT[1:2].copy()
    elif name == "many":
        k = np.arange(300)
        cams = c0[None, :] * (1 + 1e-3 * (k % 7))[:, None]
        ext = EXT[k % 5].copy()
        cams[297], ext[297] = cams[296] * (1 + 2e-3), ext[296]         # the sensor pose shared, the intrinsics not
        cams[299], ext[299] = cams[298], EXT[(298 % 5 + 1) % 5]        # the intrinsics shared, the sensor pose not
        cid[real] = (real * 37) % 300
        cid[real[:4]] = (296, 297, 298, 299)
        assert cid.max() > 255 and np.array_equal(ext[296], ext[297]) and not np.array_equal(cams[296], cams[297])
        assert np.array_equal(cams[298], cams[299]) and not np.array_equal(ext[298], ext[299])
    elif name == "identity":
        cams = c0[None, :] * np.array([1.0, 1.001, 0.998])[:, None]
        ext = np.tile(rig_ref.IDENTITY12, (3, 1))
        cid[real] = real % 3
    elif name == "stereo":
        slots = real[(fl[real] & STEREO) != 0]
        assert len(slots) >= 100 and len(slots) < len(real), "the design lacks stereo or mono slots"
        cid[slots] = 1 + np.arange(len(slots)) % 4
    elif name == "none":
        cams, ext = cams[:1], EXT[:1].copy()
    else:
        raise KeyError(name)
    return cams, ext, cid


def attach(f, cams, ext, cid, seed=0):
    """a copy of the flattened dict with the camera table, the sensor poses and the slots' entries; the measurement of
    every real slot whose entry is not (the design's intrinsics, identity) is the projection through its sensor pose
    at the design's geometry + N(0, PIXEL_SIGMA)"""
    g = dict(f)
    g["cams"], g["cam_ext"] = np.ascontiguousarray(cams), np.ascontiguousarray(ext)
    g["cam_id"] = cid.astype(np.uint16)
    g["meas"] = f["meas"].copy()
    q = f["poses"][f["pose"]]
    X = f["lms"][f["lm"]]
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]).transpose(2, 0, 1)
    Xb = np.einsum("eij,ej->ei", R, X) + q[:, 4:]
    e12 = ext[cid]
    Xs = np.einsum("eij,ej->ei", e12[:, :9].reshape(-1, 3, 3), Xb) + e12[:, 9:]
    act = (np.asarray(f["src"]) >= 0) & ((f["flags"] & INACTIVE) == 0)
    assert np.all(Xs[act, 2] > MIN_DEPTH_FRACTION * Xb[act, 2]) and np.all(Xb[act, 2] > 0.1), \
        "an active slot has Z_s below %g of its body-frame depth" % MIN_DEPTH_FRACTION
    own = np.all(cams[cid] == np.asarray(f["cams"][0])[None, :], 1) & np.all(e12 == rig_ref.IDENTITY12[None, :], 1)
    redo = np.flatnonzero((np.asarray(f["src"]) >= 0) & ~own)
    rng = np.random.default_rng(2000 + seed)
    c = cams[cid[redo]]
    iz = 1 / Xs[redo, 2]
    pu, pv = c[:, 0] * Xs[redo, 0] * iz + c[:, 2], c[:, 1] * Xs[redo, 1] * iz + c[:, 3]
    noise = rng.normal(0.0, PIXEL_SIGMA, (3, len(redo)))
    st = (f["flags"][redo] & STEREO) != 0
    g["meas"][0, redo], g["meas"][1, redo] = pu + noise[0], pv + noise[1]
    g["meas"][2, redo] = np.where(st, pu - c[:, 4] * iz + noise[2], 0.0)
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
    assert len(f["cams"]) == 1
    return f, hs


@functools.lru_cache(maxsize=None)
def case(design, pattern, fused=False):
    """(flattened dict with the pattern's camera table and sensor poses, hsc structure); built once, never modified"""
    f, hs = _design(design, fused)
    cams, ext, cid = pattern_table(pattern, f)
    g = attach(f, cams, ext, cid, seed=PATTERNS.index(pattern))
    return g, hs


# which pattern goes on which design.  "beyond" needs straddling landmarks, which the engine's padded layouts never have;
# "poses" the degrees of layout A
PLAIN_CASES = (("A", "third"), ("A", "blocks"), ("A", "beyond"), ("B", "beyond"), ("A", "poses"), ("A", "one"), ("A", "many"),
               ("A", "identity"), ("A", "stereo"), ("A", "none"))
FUSED_CASES = (("A", "third"), ("A", "blocks"), ("A", "poses"), ("A", "one"), ("A", "many"), ("A", "identity"),
               ("A", "stereo"), ("B_plan", "third"))


@functools.lru_cache(maxsize=None)
def robust2(design, which, fused=False):
    """a robust kernel per kind with the kinks where designed.robust_kernels / fused_robust_kernels place them"""
    rk = designed.fused_robust_kernels(design) if fused else designed.robust_kernels(design)
    if which == 0:
        return dict(mono=rk["none"], stereo=rk["huber"])
    return dict(mono=rk["tukey"], stereo=rk["none"])


def ring_scene():
    """a small hand-built scene for LARGE rotations: 24 landmarks on a ring of radius 6 m (heights -1 .. 1) round a body
    at the origin, four cameras at 0 / 90 / 180 / 270 degrees of yaw (about the body's y axis) with lever arms of 0.3 to
    0.5 m; every camera sees the six landmarks in front of it from three body poses (one fixed).  Returns a flattened dict
    (landmark-major slots, mono and stereo alternating) with exact measurements + 0.5 px noise"""
    rng = np.random.default_rng(7)
    nl, npose = 24, 3
    ang = 2 * np.pi * (np.arange(nl) + 0.5) / nl
    lms = np.stack([6 * np.sin(ang), np.linspace(-1, 1, nl) * np.cos(3 * ang), 6 * np.cos(ang)], 1)
    poses = np.array([_axis_angle((0.1, 1, 0.05), d, t) for d, t in ((0.0, (0, 0, 0)), (7.0, (0.3, 0.05, -0.2)),
                                                                     (-9.0, (-0.25, -0.1, 0.3)))])
    levers = ((0.0, 0.0, 0.3), (0.4, 0.05, 0.0), (0.0, -0.1, -0.5), (-0.35, 0.1, 0.1))
    # body -> sensor: Xs = Ry(-yaw) (Xb - c) for a camera at c looking along the body direction of yaw
    sens = []
    for k, c in enumerate(levers):
        q = _axis_angle((0, 1, 0), -90.0 * k, (0, 0, 0))
        M = rig_ref.quat_to_ext(q)[:9].reshape(3, 3)
        sens.append(np.concatenate([q[:4], -M @ np.asarray(c)]))
    ext = np.stack([rig_ref.quat_to_ext(q) for q in sens])
    cams = np.tile(np.array([400.0, 410.0, 320.0, 240.0, 40.0]), (4, 1))
    pose_i, lm_i, cam_i = [], [], []
    for l in range(nl):
        k = int(((ang[l] + np.pi / 4) % (2 * np.pi)) // (np.pi / 2))   # the camera whose quadrant holds the landmark
        for p in range(npose):
            pose_i.append(p), lm_i.append(l), cam_i.append(k)
    pose_i, lm_i, cam_i = (np.array(a, np.int32) for a in (pose_i, lm_i, cam_i))
    E = len(pose_i)
    flags = np.where(np.arange(E) % 2 == 1, STEREO, 0).astype(np.uint8)
    # free poses first: pose 0 is the fixed one -> flattened index 2
    order = np.array([2, 0, 1])
    fpose = order[pose_i]
    flags |= np.where(fpose == 2, 2, 0).astype(np.uint8)
    fposes = np.zeros((3, 7)); fposes[order] = poses
    f = dict(E=E, P=2, L=nl, Pall=3, Lall=nl, src=np.arange(E), pose=fpose.astype(np.int32), lm=lm_i, flags=flags,
             meas=np.zeros((3, E)), omega=np.ones(E), cams=cams, cam_id=cam_i.astype(np.uint16), poses=fposes, lms=lms)
    lm_ptr = np.zeros(nl + 1, np.int32); np.add.at(lm_ptr, lm_i + 1, 1); f["lm_ptr"] = np.cumsum(lm_ptr).astype(np.int32)
    f["pose_edge"] = np.lexsort((lm_i, fpose)).astype(np.int32)
    pp = np.zeros(4, np.int32); np.add.at(pp, fpose + 1, 1); f["pose_ptr"] = np.cumsum(pp).astype(np.int32)
    f["cam_ext"] = ext
    ref = rig_ref.build(f, dict(mono=(0, 1.0), stereo=(0, 1.0)), dtype=np.float64)
    assert np.all(ref["Xs"][:, 2] > 2.0), "a ring landmark is not in front of its camera"
    # (with meas = 0 the residual is the projection itself)
    meas = np.asarray(ref["e"]).T + rng.normal(0, 0.5, (3, E))
    meas[2] = np.where((flags & STEREO) != 0, meas[2], 0.0)
    f["meas"] = meas
    return f
