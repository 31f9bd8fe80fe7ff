"""Seeded BA problems with PRESCRIBED vertex degrees and general rotations (numpy only, no product code).

synth.make_problem gives every pose about 70 edges and yaws gently about y; the chunking constants of the
bundle-adjustment kernels (256 edge slots per workgroup, 7 / 14 edges per wave and chunk, 16 waves) and the
cross terms of the rotation formulas are outside what that family reaches.  Here the degrees are an input,
and the geometry is a "turntable": a landmark cloud (sigma 1.5) at the origin, every camera 15-25 away
looking at it with a uniformly random orientation about the optical axis and a uniformly random viewing
direction, so that all four quaternion components are O(0.4); a few poses get |qw| < 0.05.

The dicts returned have the field names of synth.make_problem: oracle.Problem(*synth.problem_fields(d)),
devmem.flatten and cugo.graph_from_arrays take them unchanged.
"""
import functools

import numpy as np

import synth

CAM = synth.KITTI_CAM

# pose degrees of layout A: around 7 / 14 (chunk of k_hsc_diag / k_hsc_diag_mfma), 64 (a wave), 224 = 16 x 14 (a
# second chunk per wave), 256 / 512 (half-round / round of k_build_poses), 704 (HS_CAP), 1024
A_FREE_DEGREES = (0, 1, 6, 7, 8, 13, 14, 15, 64, 65, 223, 224, 225, 256, 257, 449, 512, 513, 705, 1025)
A_FIXED_DEGREES = (40, 40)
# landmark degrees of layout B in free-index order (0 = no edge at all).  Slots: 1 + 2 + 100 = 103, so the
# 255-edge landmark occupies [103, 358) and straddles slot 256; the 300-edge one spans two blocks
B_LM_DEGREES = (1, 2, 100, 255, 0, 256, 3, 257, 0, 300, 5, 4, 7, 0, 2, 0, 0)


def _cameras(rng, n, n_small_w):
    """n world->camera poses looking at the origin from 15-25 away; the first n_small_w with |qw| < 0.05"""
    pose = np.zeros((n, 7))
    for i in range(n):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        if i < n_small_w:
            q[3] = rng.uniform(0.005, 0.045)
            q[:3] *= np.sqrt(1 - q[3] ** 2) / np.linalg.norm(q[:3])
        if q[3] < 0:
            q = -q
        pose[i, :4] = q
        # the camera centre is -R^T t: with t ~ (0, 0, r) the origin is on the optical axis, whatever R is
        pose[i, 4:] = [rng.normal(0, 0.5), rng.normal(0, 0.5), rng.uniform(15, 25)]
    return pose[rng.permutation(n)]


def _assemble(rng, n_poses, n_landmarks, e_pose, e_lm, fixed_poses, fixed_landmarks, stereo_frac=0.5,
              pix_noise=1.0, pose_noise=(0.01, 0.05), lm_noise=0.02, cameras=None):
    """cameras (optional): a function (rng, n, n_small_w) -> poses in place of _cameras"""
    n_small_w = max(2, n_poses // 8)
    pose_gt = (cameras or _cameras)(rng, n_poses, n_small_w)
    lm_gt = rng.normal(0, 1.5, (n_landmarks, 3))
    nrm = np.linalg.norm(lm_gt, axis=1, keepdims=True)
    lm_gt *= np.minimum(1.0, 6.0 / np.maximum(nrm, 1e-30))   # inside a ball of radius 6: depth >= 15 - 6 - noise
    pose = pose_gt.copy()
    for i in range(n_poses):
        if i in fixed_poses:
            continue
        q = synth.quat_mul(synth.quat_from_rotvec(rng.normal(0, pose_noise[0], 3)), pose[i, :4])
        pose[i, :4] = q / np.linalg.norm(q) * (1 if q[3] >= 0 else -1)
        pose[i, 4:] += rng.normal(0, pose_noise[1], 3)
    lm = lm_gt + rng.normal(0, lm_noise, lm_gt.shape)
    for l in fixed_landmarks:
        lm[l] = lm_gt[l]
    e_pose, e_lm = np.asarray(e_pose, np.int32), np.asarray(e_lm, np.int32)
    E = len(e_pose)
    assert len(set(zip(e_pose.tolist(), e_lm.tolist()))) == E, "duplicate (pose, landmark) edge"
    R = np.array([synth.quat_to_R(p[:4]) for p in pose_gt])
    Xc = np.einsum("eij,ej->ei", R[e_pose], lm_gt[e_lm]) + pose_gt[e_pose, 4:]
    stereo = (rng.random(E) < stereo_frac).astype(np.uint8)
    u = CAM[0] * Xc[:, 0] / Xc[:, 2] + CAM[2]
    v = CAM[1] * Xc[:, 1] / Xc[:, 2] + CAM[3]
    ur = u - CAM[4] / Xc[:, 2]
    meas = np.stack([u, v, ur], 1) + rng.normal(0, pix_noise, (E, 3))
    meas[stereo == 0, 2] = 0.0
    omega = 1.0 / (1.2 ** rng.integers(0, 8, E)) ** 2       # octave levels, as synth
    pf = np.zeros(n_poses, np.uint8); pf[list(fixed_poses)] = 1
    lf = np.zeros(n_landmarks, np.uint8); lf[list(fixed_landmarks)] = 1
    d = dict(pose=pose, pose_fixed=pf, lm=lm, lm_fixed=lf, e_pose=e_pose, e_lm=e_lm, e_stereo=stereo,
             e_meas=meas, e_omega=omega, e_cam=np.tile(CAM, (E, 1)), pose_gt=pose_gt, lm_gt=lm_gt)
    check_geometry(d)
    return d


def check_geometry(d):
    """the properties the turntable promises: general rotations, some |qw| < 0.05, every depth > 5, fixed vertices
    not at the end of the id range"""
    q = np.abs(d["pose"][:, :4])
    assert np.allclose(np.linalg.norm(d["pose"][:, :4], axis=1), 1.0, atol=1e-12)
    if len(q) >= 16:
        med = np.median(q, axis=0)
        assert np.all(med[:3] > 0.2) and np.all(med < 0.8) and med[3] > 0.1, med
    assert (q[:, 3] < 0.05).sum() >= 2, "no pose with |qw| < 0.05"
    for key_p, key_l in (("pose", "lm"), ("pose_gt", "lm_gt")):
        R = np.array([synth.quat_to_R(p[:4]) for p in d[key_p]])
        z = np.einsum("ej,ej->e", R[d["e_pose"], 2], d[key_l][d["e_lm"]]) + d[key_p][d["e_pose"], 6]
        assert len(z) == 0 or z.min() > 5.0, z.min()
    for fx in (d["pose_fixed"], d["lm_fixed"]):
        if fx.any():
            assert not fx[-1], "a fixed vertex has the last id"


def designed(pose_degrees, n_landmarks, fixed_poses=(), fixed_landmarks=(), seed=0, **kw):
    """pose i observes exactly pose_degrees[i] distinct landmarks (a fixed pose: free landmarks only, so that every
    one of its edges is active and its degree in the flattened layout is the prescribed one)"""
    rng = np.random.default_rng(seed)
    free_lms = np.array([l for l in range(n_landmarks) if l not in set(fixed_landmarks)])
    ep, el = [], []
    for i, deg in enumerate(pose_degrees):
        pool = free_lms if i in fixed_poses else np.arange(n_landmarks)
        assert deg <= len(pool)
        pick = np.sort(rng.choice(pool, deg, replace=False)) if deg else []
        ep += [i] * deg
        el += list(pick)
    return _assemble(rng, len(pose_degrees), n_landmarks, ep, el, tuple(fixed_poses), tuple(fixed_landmarks), **kw)


def designed_by_landmark(lm_degrees, n_poses, fixed_poses=(), fixed_landmarks=(), seed=0, **kw):
    """landmark l is observed by exactly lm_degrees[l] distinct poses (a fixed landmark: by free poses only)"""
    rng = np.random.default_rng(seed)
    free_poses = np.array([p for p in range(n_poses) if p not in set(fixed_poses)])
    ep, el = [], []
    for l, deg in enumerate(lm_degrees):
        pool = free_poses if l in fixed_landmarks else np.arange(n_poses)
        assert deg <= len(pool)
        pick = np.sort(rng.choice(pool, deg, replace=False)) if deg else []
        ep += list(pick)
        el += [l] * deg
    return _assemble(rng, n_poses, len(lm_degrees), ep, el, tuple(fixed_poses), tuple(fixed_landmarks), **kw)


def check_layout(f):
    """a flattened dict (devmem.flatten / pad_to_groups) is a legal cugo_edges layout (include/cugo_hip.h): lm_ptr,
    pose_ptr and pose_edge consistent and in range, edges landmark-major, fixed indices behind the free ones.  Run on
    the CPU before anything is uploaded."""
    E, P, L, Pall, Lall = f["E"], f["P"], f["L"], f["Pall"], f["Lall"]
    assert 0 <= P <= Pall and 0 <= L <= Lall
    for k in ("pose", "lm", "flags", "omega", "cam_id", "pose_edge"):
        assert len(f[k]) == E, k
    assert f["meas"].shape == (3, E)
    pose, lm, fl = f["pose"], f["lm"], f["flags"]
    if E:
        assert pose.min() >= 0 and pose.max() < Pall and lm.min() >= 0 and lm.max() < Lall
        assert np.all(np.diff(lm) >= 0), "edges are not landmark-major"
        assert f["cam_id"].max() < len(f["cams"])
    lp, pp = f["lm_ptr"], f["pose_ptr"]
    assert len(lp) == Lall + 1 and lp[0] == 0 and lp[-1] == E and np.all(np.diff(lp) >= 0)
    assert len(pp) == Pall + 1 and pp[0] == 0 and pp[-1] <= E and np.all(np.diff(pp) >= 0)
    for l in np.flatnonzero(np.diff(lp)):
        assert np.all(lm[lp[l]:lp[l + 1]] == l)
    real = (fl & 8) == 0
    n_real = int(real.sum())
    assert pp[-1] == n_real
    pe = f["pose_edge"]
    assert pe.min(initial=0) >= 0 and pe.max(initial=0) < max(E, 1)
    assert len(np.unique(pe[:n_real])) == n_real and np.all(real[pe[:n_real]])
    for p in np.flatnonzero(np.diff(pp)):
        es = pe[pp[p]:pp[p + 1]]
        assert np.all(pose[es] == p) and np.all(np.diff(lm[es]) > 0), "pose_edge: not this pose's edges by landmark"
    # free indices first: the flag bits agree with the index ranges, and no real edge joins two fixed vertices
    assert np.array_equal((fl[real] & 2) != 0, pose[real] >= P)
    assert np.array_equal((fl[real] & 1) != 0, lm[real] >= L)
    assert not np.any((fl[real] & 3) == 3)
    assert np.all(np.isfinite(f["meas"])) and np.all(np.isfinite(f["omega"])) and np.all(np.isfinite(f["poses"]))


def straddlers(f, group=256):
    """landmarks whose edge slots lie in more than one `group`-slot block"""
    lp = f["lm_ptr"]
    return [l for l in range(f["Lall"]) if lp[l + 1] > lp[l] and lp[l] // group != (lp[l + 1] - 1) // group]


def _flat(d, oracle):
    import devmem
    prob = oracle.Problem(*synth.problem_fields(d))
    f = devmem.flatten(prob)
    check_layout(f)
    return prob, f


@functools.lru_cache(maxsize=None)
def layout(name):
    """(problem dict, oracle.Problem, flattened dict, (rowptr, colind, off_ptr, ei, ej)) of layout "A", "B", "C",
    "B_plan" (B without the landmarks of more than 256 edges, which the landmark-major plan refuses) or "U" (66 poses,
    for the pose-update test); built once per process and never modified: copy before changing anything"""
    import devmem
    import oracle
    if name == "A":
        deg = list(A_FREE_DEGREES)
        deg.insert(3, A_FIXED_DEGREES[0]); deg.insert(11, A_FIXED_DEGREES[1])
        d = designed(deg, 1100, fixed_poses=(3, 11), fixed_landmarks=(5, 42, 300, 700, 1000), seed=0)
    elif name in ("B", "B_plan"):
        degs = [k if (name == "B" or k <= 256) else 0 for k in B_LM_DEGREES]
        # ids: two fixed landmarks (3 edges each) in front and in the middle, the free ones in B_LM_DEGREES order
        lmd = degs[:2] + [3] + degs[2:9] + [3] + degs[9:]
        d = designed_by_landmark(lmd, 304, fixed_poses=(1, 77, 150, 200), fixed_landmarks=(2, 10), seed=1)
    elif name == "C":
        lmd = [0] * 600
        lmd[10], lmd[300], lmd[301] = 1, 1, 1
        d = designed_by_landmark(lmd, 3, fixed_poses=(0,), fixed_landmarks=(7, 450), seed=2)
    elif name == "U":
        d = designed([2] * 66, 12, fixed_poses=(5, 40), fixed_landmarks=(3,), seed=3)
    else:
        raise KeyError(name)
    prob, f = _flat(d, oracle)
    hs = devmem.hsc_structure(f)
    check_named(name, d, f, hs)
    return d, prob, f, hs


def check_named(name, d, f, hs):
    """the properties each layout was designed for, asserted where it is built"""
    rowptr, colind, off_ptr, ei, ej = hs
    deg = np.diff(f["pose_ptr"])
    lmdeg = np.diff(f["lm_ptr"])
    if name == "A":
        assert sorted(deg[:f["P"]].tolist()) == sorted(A_FREE_DEGREES)
        assert deg[f["P"]:].tolist() == list(A_FIXED_DEGREES)
        assert f["E"] == sum(A_FREE_DEGREES) + sum(A_FIXED_DEGREES) and f["Lall"] - f["L"] == 5
        n = np.diff(off_ptr)
        n = n[n > 0]
        for what, ok in (("1..7", (n <= 7)), ("8..14", (n >= 8) & (n <= 14)), ("15..28", (n >= 15) & (n <= 28)),
                         (">28", n > 28), ("0 mod 14", n % 14 == 0), ("1 mod 14", n % 14 == 1)):
            assert ok.any(), "no off-diagonal product list of length " + what
        assert len(straddlers(f)) >= 1
    elif name == "B":
        got = lmdeg[:f["L"]].tolist()
        assert got == list(B_LM_DEGREES), got
        for k in (1, 2, 255, 256, 257, 300):
            assert k in got
        lp = f["lm_ptr"]
        st = straddlers(f)
        assert any(lmdeg[l] <= 256 for l in st), "no landmark of <= 256 edges straddles a block boundary"
        l300 = got.index(300)
        assert lp[l300] // 256 != (lp[l300 + 1] - 1) // 256
        mid = [l for l in range(f["L"]) if lmdeg[l] == 0]
        assert mid[0] < f["L"] - 1 and lmdeg[mid[0] + 1] > 0 and mid[-1] == f["L"] - 1
        assert deg.max() <= 16 and f["Pall"] - f["P"] == 4
    elif name == "C":
        assert f["E"] == 3 and f["L"] == 598 and f["L"] > 256 + f["E"]
    elif name == "B_plan":
        assert lmdeg.max() <= 256 and 256 in lmdeg and 255 in lmdeg
    elif name == "U":
        assert f["P"] == 64 and f["Pall"] == 66


def graph_d():
    """layout A without the poses of degree < 6 (a graph the LM loop can run on): keeps degrees 705 and 1025 >
    HS_CAP = 704 of the strip form and several rounds of k_pose_schur / k_hsc_rows"""
    deg = [k for k in A_FREE_DEGREES if k >= 6]
    deg.insert(2, A_FIXED_DEGREES[0]); deg.insert(9, A_FIXED_DEGREES[1])
    d = designed(deg, 1100, fixed_poses=(2, 9), fixed_landmarks=(5, 42, 300, 700, 1000), seed=4)
    assert max(deg) == 1025 and 705 in deg
    return d


def random_blocks(f, seed, kappa_max=100.0):
    """supplied inputs of the Schur complement / back-substitution on a flattened layout, NOT from a build pass: Hpl
    [E,6,3] ~ N(0,1) with zero blocks where an edge takes no part (fixed endpoint, padding), Hll [L,3,3] random SPD with
    condition number <= kappa_max, Hpp [P,6,6] symmetric, bp, bl (zero for a landmark without edges, as a build pass
    leaves it), xp ~ N(0, 0.01) random"""
    rng = np.random.default_rng(seed)
    E, P, L = f["E"], f["P"], f["L"]
    ff = (f["flags"] & 11) == 0
    Hpl = rng.normal(size=(E, 6, 3)) * ff[:, None, None]
    Q = np.linalg.qr(rng.normal(size=(L, 3, 3)))[0]
    ev = np.exp(rng.uniform(0, np.log(kappa_max), (L, 3))) * rng.uniform(0.5, 20, (L, 1))
    Hll = np.einsum("lij,lj,lkj->lik", Q, ev, Q)
    Hll = 0.5 * (Hll + Hll.transpose(0, 2, 1))
    assert L == 0 or np.linalg.cond(Hll).max() <= kappa_max * (1 + 1e-9)
    G = rng.normal(size=(P, 6, 6))
    Hpp = G + G.transpose(0, 2, 1) + 30 * np.eye(6)
    bl = rng.normal(size=(L, 3)) * (np.diff(f["lm_ptr"])[:L] > 0)[:, None]   # no edge: no gradient either
    return dict(Hpl=Hpl, Hll=Hll, Hpp=Hpp, bp=rng.normal(size=(P, 6)), bl=bl, xp=rng.normal(0, 0.01, (P, 6)))


def tukey_delta(x):
    """a Tukey delta for which about 30 % (at least one, not all) of the edges with kernel arguments x = omega |e|^2 get
    weight 0: delta^2 halfway between two neighbouring arguments"""
    xs = np.sort(np.asarray(x, np.float64))
    k = max(1, min(len(xs) - 1, int(round(0.7 * len(xs)))))
    return float(np.sqrt(0.5 * (xs[k - 1] + xs[k])))


THETAS = (0.0, 1e-9, 0.99e-5, 1.01e-5, 3e-5, 1e-3, 1.0, 2 * np.pi / 3 - 1e-6, 2 * np.pi / 3 + 1e-6, 2.5, np.pi - 1e-6,
          np.pi, 3.5)


def pose_update_cases(seed=7):
    """(poses [64,7], dx [64,6]): every theta of THETAS about x, y, z and a general axis (the three i branches of the
    trace <= 0 case and the general one) on general quaternions, then 12 poses chosen so that dq q has w = +-1e-6 or
    +-1e-13: the sign flip"""
    rng = np.random.default_rng(seed)
    poses, dxs = [], []
    gen = rng.normal(size=3)
    gen /= np.linalg.norm(gen)
    for th in THETAS:
        for axis in (np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 0, 1.0]), gen):
            q = rng.normal(size=4)
            q /= np.linalg.norm(q)
            poses.append(np.concatenate([q, rng.normal(0, 5, 3)]))
            dxs.append(np.concatenate([th * axis, rng.normal(0, 0.3, 3)]))
    for th in (1e-3, 1.0, 2.5):
        for w in (1e-6, -1e-6, 1e-13, -1e-13):
            ax = rng.normal(size=3)
            ax /= np.linalg.norm(ax)
            dq = np.concatenate([np.sin(th / 2) * ax, [np.cos(th / 2)]])
            r = rng.normal(size=4)
            r[3] = 0
            r /= np.linalg.norm(r)
            r[3] = w
            q = synth.quat_mul(dq * np.array([-1, -1, -1, 1.0]), r)   # dq^-1 r
            poses.append(np.concatenate([q / np.linalg.norm(q), rng.normal(0, 5, 3)]))
            dxs.append(np.concatenate([th * ax, rng.normal(0, 0.3, 3)]))
    return np.array(poses), np.array(dxs)


@functools.lru_cache(maxsize=None)
def robust_kernels(name):
    """the robust kernels of the build-pass tests on layout `name`: none, Huber, and Tukey with a delta chosen on the
    reference so that at least 10 % of the edges get weight 0 and at least 10 % do not (asserted)"""
    import kernel_ref
    _, prob, f, _ = layout(name)
    x = np.asarray(kernel_ref.build(prob, (0, 1.0), f)["x"], np.float64)
    delta = tukey_delta(x)
    zero = float((x > delta * delta).mean())
    assert zero >= 0.1 and 1 - zero >= 0.1, zero
    return {"none": (0, 1.0), "huber": (3, 1.5), "tukey": (2, delta)}


# ------------------------------------------------------------------ layouts of the fused iteration (test_fused_shapes.py)
F_COND_LAMBDAS = (1e-6, 1e-3, 0.5)
# landmark degrees of the fused tests' "B_plan" in free-index order: B_LM_DEGREES without the landmarks of more than 256
# edges, and 2 + 100 + 153 = 255 slots in front of the degree-1 landmark, whose owner slot is then the LAST of its group;
# the landmarks of 255 and 256 edges are owned by the FIRST slot of theirs (one padding slot between them)
FUSED_B_LM_DEGREES = (2, 100, 153, 1, 255, 0, 256, 3, 0, 5, 4, 7, 0, 2, 0, 0)


def deactivate(f, slots):
    """a copy of the flattened dict with CUGO_EDGE_INACTIVE set on `slots`, as the engine's outlier rejection leaves
    them: the flag is set, the slots STAY in the pose lists (pose_ptr / pose_edge) and keep their measurements"""
    g = dict(f)
    g["flags"] = f["flags"].copy()
    g["flags"][np.asarray(slots, np.int64)] |= 8
    return g


def check_fused_layout(f):
    """check_layout for a layout that may hold deactivated edges (deactivate(): INACTIVE slots that are not padding and
    are still listed by their pose): legal with those flags cleared, the padding slots are the ones with src < 0, and no
    landmark's slots lie in two 256-slot groups"""
    g = dict(f)
    g["flags"] = np.where(f["src"] >= 0, f["flags"] & 7, f["flags"]).astype(np.uint8)
    check_layout(g)
    assert np.all((f["flags"][f["src"] < 0] & 8) != 0)
    assert straddlers(f) == []


def _pairs_of_cameras(rng, n, n_small_w):
    """_cameras, with every odd pose a near copy of the pose before it (rotation 2e-3, translation 0.02): a landmark seen
    by such a pair only has small parallax"""
    pose = _cameras(rng, n, n_small_w)
    for i in range(1, n, 2):
        q = synth.quat_mul(synth.quat_from_rotvec(rng.normal(0, 2e-3, 3)), pose[i - 1, :4])
        pose[i, :4] = q / np.linalg.norm(q) * (1 if q[3] >= 0 else -1)
        pose[i, 4:] = pose[i - 1, 4:] + rng.normal(0, 0.02, 3)
    return pose


@functools.lru_cache(maxsize=None)
def fused_layout(name):
    """(oracle.Problem, flattened dict in the engine's slot layout, hsc structure) of a layout of the fused-iteration
    tests: "A", "C", "U" (layout()) and "B_plan" (FUSED_B_LM_DEGREES) padded (devmem.pad_to_groups), and
    "F-dead": a free landmark all of whose slots are INACTIVE, a free pose all of whose edges are, edges whose only free
              end is the pose and edges whose only free end is the landmark;
    "F-allfixed": every landmark fixed (Lfree = 0), free poses;
    "F-cond": monocular landmarks of degree 1 and 2, the pairs of poses close together (small parallax).
    Built once per process and never modified; the census of each is asserted here, on the CPU."""
    import devmem
    import oracle
    dead = None
    if name in ("A", "C", "U"):
        prob, f0 = layout(name)[1:3]
    elif name == "B_plan":
        # ids: two fixed landmarks (3 edges each) in front and in the middle, the free ones in FUSED_B_LM_DEGREES order
        degs = list(FUSED_B_LM_DEGREES)
        d = designed_by_landmark(degs[:2] + [3] + degs[2:9] + [3] + degs[9:], 304, fixed_poses=(1, 77, 150, 200),
                                 fixed_landmarks=(2, 10), seed=1)
        prob, f0 = _flat(d, oracle)
    elif name == "F-dead":
        # landmark ids: 3 is fixed; free landmark 6 (degree 3) and pose 7 are the dead ones; four poses are fixed
        lmd = [100, 100, 100, 40, 5, 4, 3, 6, 5, 4, 6, 5]
        d = designed_by_landmark(lmd, 130, fixed_poses=(2, 50, 90, 120), fixed_landmarks=(3,), seed=5)
        prob, f0 = _flat(d, oracle)
        dead = (int(prob.indices()[0][7]), int(prob.indices()[1][6]))
    elif name == "F-allfixed":
        d = designed_by_landmark([30] * 20, 40, seed=6)
        d["lm_fixed"][:] = 1
        prob, f0 = _flat(d, oracle)
    elif name == "F-cond":
        lmd = [2, 1] * 150            # 255 slots in front of a degree-2 landmark: one padding slot
        rng = np.random.default_rng(7)
        ep, el = [], []
        for l, deg in enumerate(lmd):
            a = 2 * int(rng.integers(0, 20))          # a pair (a, a + 1) of near-identical cameras
            ep += [a, a + 1][:deg]
            el += [l] * deg
        d = _assemble(rng, 40, len(lmd), ep, el, (), (), stereo_frac=0.0, cameras=_pairs_of_cameras)
        prob, f0 = _flat(d, oracle)
    else:
        raise KeyError(name)
    f = devmem.pad_to_groups(f0)
    P, L = f["P"], f["L"]
    if dead:
        p_dead, l_dead = dead
        slots = np.flatnonzero(((f["pose"] == p_dead) | (f["lm"] == l_dead)) & (f["src"] >= 0))
        f = deactivate(f, slots)
    check_fused_layout(f)
    hs = devmem.hsc_structure(f)
    fl, lmdeg, deg = f["flags"], np.diff(f["lm_ptr"]), np.diff(f["pose_ptr"])
    pad = f["src"] < 0
    if name not in ("C", "U"):           # (these two have fewer than 256 slots: nothing to pad)
        assert pad.any() and f["E"] > f0["E"], "no padding slot"
    if name == "A":
        assert sorted(deg[:P].tolist()) == sorted(A_FREE_DEGREES) and f["Pall"] - P == 2 and f["Lall"] - L == 5
        rounds = sorted(set(-(-k // 256) for k in A_FREE_DEGREES))
        assert rounds == [0, 1, 2, 3, 5]                      # rounds of k_pose_schur's 256 lanes
        assert 256 in deg and 512 in deg and 257 in deg and 513 in deg and 1025 in deg   # last round full / 1 lane
    elif name == "B_plan":
        real_deg = np.bincount(f["lm"][~pad], minlength=f["Lall"])[:L]
        for k in (1, 2, 255, 256):
            assert k in real_deg
        mid = [l for l in range(L) if lmdeg[l] == 0]
        assert len(mid) >= 4 and mid[0] < L - 1 and lmdeg[mid[0] + 1] > 0 and mid[-1] == L - 1
        own = f["lm_ptr"][:L][lmdeg[:L] > 0]
        assert (own % 256 == 0).any() and (own % 256 == 255).any(), "no landmark owned by the first / last slot of a group"
    elif name == "C":
        assert L > 256 + f["E"] and f["E"] == 3                # back-substitution workgroups past the last slot
    elif name == "U":
        assert P == 64
    elif name == "F-dead":
        assert P == 126 and f["Pall"] == 130 and f["Lall"] - L == 1
        sl = np.arange(f["lm_ptr"][l_dead], f["lm_ptr"][l_dead + 1])
        assert len(sl) == 3 and np.all(fl[sl] & 8) and l_dead < L
        pe = f["pose_edge"][f["pose_ptr"][p_dead]:f["pose_ptr"][p_dead + 1]]
        assert len(pe) >= 2 and np.all(fl[pe] & 8) and p_dead < P
        live = (fl & 8) == 0
        assert (live & ((fl & 3) == 1)).sum() >= 10 and (live & ((fl & 3) == 2)).sum() >= 5
        # the landmarks the dead pose saw keep other, live edges
        assert all((live[f["lm_ptr"][l]:f["lm_ptr"][l + 1]]).any() for l in set(f["lm"][pe].tolist()) - {l_dead})
    elif name == "F-allfixed":
        assert L == 0 and P == 40 and np.all((fl[~pad] & 3) == 1) and len(hs[1]) == P and len(hs[3]) == 0
    elif name == "F-cond":
        assert not (fl & 4).any() and sorted(set(lmdeg[:L].tolist()) - {0}) >= [1, 2]
        import kernel_ref
        ref = kernel_ref.build(prob, (0, 1.0), f)
        kap = []
        for lam in F_COND_LAMBDAS:
            ln = kernel_ref.fused_lines(ref["Hll"], ref["bl"], lam)
            assert np.all(ln["piv"] > 0), "a non-positive pivot in the reference factorisation"
            kap.append(ln["kappa"])
        assert (kap[0] > 1e6).mean() >= 0.1 and kap[0].max() > 1e9 and kap[2].min() < 1e4, (kap[0].max(), kap[2].min())
    return prob, f, hs


@functools.lru_cache(maxsize=None)
def fused_robust_kernels(name):
    """robust_kernels for a layout of fused_layout (the Tukey delta from the layout's own kernel arguments)"""
    if name in ("A", "C", "U"):
        return robust_kernels(name)
    import kernel_ref
    prob, f, _ = fused_layout(name)
    x = np.asarray(kernel_ref.build(prob, (0, 1.0), f)["x"], np.float64)[(f["flags"] & 8) == 0]
    delta = tukey_delta(x)
    zero = float((x > delta * delta).mean())
    assert zero >= 0.1 and 1 - zero >= 0.1, zero
    return {"none": (0, 1.0), "huber": (3, 1.5), "tukey": (2, delta)}
