"""Designed layouts for the unary pose edge kernels (icp_kernels.hip, prior_kernels.hip, pose_edge_kernels.hip): pose
degrees placed around the kernels' constants — ICP_CHUNK = 512 edges per wave in 64-lane groups, PRIOR_POSES = 8 poses per
workgroup, 256 totals per trip of k_pose_chi_total, 1024 x 256 edges per trip of k_pose_check — built programmatically
with fixed seeds (numpy only).  Every layout comes with its census, which test_pose_edge_ref_host.py asserts, so that a
change of a recipe cannot silently lose what the layout is for.

An ICP kind is a dict pose [E] (ascending), p [E,3], n [E,3] + d [E] (plane) or a, b, u [E,3] (line; u = (b - a) / |b - a| in
double, the array the device is given), omega [E] or [1], active [E] bool, flags [E] uint8, rk (type, delta).  A prior set is
the dict of prior_ref.make_prior, sorted by pose, with flags.

The relative-pose kernel (relpose_kernels.hip: RELPOSE_POSES = 4 poses per workgroup, one wave walks a pose's incidence
list) has its layouts at the end of the file (relpose_layout); test_relpose_ref_host.py asserts their census."""
import functools

import numpy as np

import icp_ref
import prior_ref

CHUNK, GROUP, PRIOR_POSES, TOTALS = 512, 64, 8, 256
INACTIVE = 1 << 3   # CUGO_EDGE_INACTIVE (include/cugo_hip.h)

# ---------------------------------------------------------------- ICP: degrees per pose
# I-A: pose ranges end at 63, 64, 65 | 511, 512, 513 | 1023, 1024; pose 0 edgeless; runs of 1, 2 and 5 edgeless poses; a
# one-edge pose on the last edge of chunk 0 (511) and one on the first of chunk 1 (512); a pose of exactly 512 edges on
# chunk 2 (1024..1535); a pose of 1100 edges from 1736 (mid-chunk 3) to 2835 (chunk 5); 3073 = 6 x 512 + 1 edges
DEG_A = [0, 63, 1, 1, 0, 446, 1, 1, 0, 0, 510, 1, 512, 0, 0, 0, 0, 0, 200, 1100, 100, 136, 1]
# I-B: 70 poses of one edge on edges 445..514 (the group 448..511 holds 64 different poses, the run crosses the chunk
# boundary 512), then 40 of two, 30 of three; poses 0 and 1 carry nothing of this layout
DEG_B = [0, 0, 445] + [1] * 70 + [2] * 40 + [3] * 30 + [7]
# I-C (free | fixed): the free/fixed boundary at edge 180 (inside the group 128..191); chunk 1 (512..1023) holds fixed-pose
# edges only and chunk 2 starts on them.  C2: the boundary exactly on the chunk boundary 512
DEG_C, FREE_C = [100, 50, 30, 400, 600], 3
DEG_C2, FREE_C2 = [300, 212, 100, 30], 2
DEG_C2B = [300, 112, 100, 100, 30]          # the same with three free poses (beside DEG_C in one call)
# I-D: pose 1 (edges 100..159) all inactive between active poses; the first 64 edges of chunk 1 (512..575) inactive;
# chunk 2 (1024..1535) inactive as a whole
DEG_D = [100, 60, 352, 264, 512, 300]


def _census_kind(pose, n_free, active):
    """what the chunk pass meets on one kind's sorted edges"""
    pose = np.asarray(pose)
    n = len(pose)
    ends = set((np.flatnonzero(np.diff(pose)) + 1).tolist()) | ({n} if n else set())
    g0 = np.arange(0, n, GROUP)
    flushes = [len(np.unique(pose[a:min(a + GROUP, n)])) - 1 for a in g0]
    chunks = (n + CHUNK - 1) // CHUNK
    slots = sorted({int(e // CHUNK + pose[e]) for e in range(n)}) if n <= 5000 else None
    counts = active & (pose < n_free)
    c0 = np.arange(0, n, CHUNK)
    return dict(n=n, ends=ends, max_flushes=max(flushes) if flushes else 0, chunks=chunks, slots=slots,
                last_chunk=n - (chunks - 1) * CHUNK if n else 0,
                chunks_without_counting_edge=[int(a // CHUNK) for a in c0 if not counts[a:a + CHUNK].any()],
                chunks_all_fixed=[int(a // CHUNK) for a in c0 if (pose[a:a + CHUNK] >= n_free).all()],
                chunks_starting_fixed=[int(a // CHUNK) for a in c0 if pose[a] >= n_free],
                chunks_all_inactive=[int(a // CHUNK) for a in c0 if not active[a:a + CHUNK].any()])


def _kind(rng, kind, deg, poses, rk, noise=0.3):
    pose = np.repeat(np.arange(len(deg), dtype=np.int32), deg)
    e = icp_ref.make_edges(rng, pose, kind, poses, noise=noise)
    if kind == "line":
        e["u"] = (e["b"] - e["a"]) / np.linalg.norm(e["b"] - e["a"], axis=1)[:, None]
    E = len(pose)
    e["omega"] = rng.uniform(0.5, 3.0, E)
    e["active"] = np.ones(E, bool)
    e["rk"] = rk
    return e


def _finish(e):
    e["flags"] = np.where(e["active"], 0, INACTIVE).astype(np.uint8)
    return e


def _pad(deg, n):
    return list(deg) + [0] * (n - len(deg))


def _icp(seed, deg_plane, deg_line, n_free, rk_plane, rk_line, inactive=None):
    """poses + the two kinds (None for an empty kind) from degree lists; inactive: {kind: index array}"""
    rng = np.random.default_rng(seed)
    P = max(len(deg_plane or []), len(deg_line or []))
    poses = np.array([icp_ref.random_pose(rng) for _ in range(P)])
    out = dict(poses=poses, n_free=P if n_free is None else n_free, P=P, plane=None, line=None)
    for kind, deg, rk in (("plane", deg_plane, rk_plane), ("line", deg_line, rk_line)):
        if deg is None:
            continue
        e = _kind(rng, kind, _pad(deg, P), poses, rk)
        if inactive and kind in inactive:
            e["active"][inactive[kind]] = False
        out[kind] = _finish(e)
    out["census"] = {k: _census_kind(out[k]["pose"], out["n_free"], out[k]["active"]) for k in ("plane", "line") if out[k] is not None}
    return out


def kinds_of(lay):
    """the (name, dict) list pose_edge_ref.icp_build takes"""
    return [(k, lay[k]) for k in ("plane", "line") if lay[k] is not None]


def ref_kinds(lay):
    """the tuple list icp_ref.reference_build takes"""
    return [(k, lay[k], lay[k]["omega"], lay[k]["active"], lay[k]["rk"]) for k in ("plane", "line") if lay[k] is not None]


INACT_D = np.concatenate([np.arange(100, 160), np.arange(512, 576), np.arange(1024, 1536)])
CAUCHY, TUKEY, HUBER, NONE = (1, 0.3), (2, 0.5), (3, 0.2), (0, 1.0)

ICP_LAYOUTS = {
    # name: (plane degrees, line degrees, n_free, rk plane, rk line, inactive)
    "A_plane": (DEG_A, None, None, CAUCHY, NONE, None),
    "A_line": (None, DEG_A, None, NONE, HUBER, None),
    "B_plane": (DEG_B, None, None, NONE, NONE, None),
    "B_line": (None, DEG_B, None, NONE, TUKEY, None),
    "AB": (DEG_A, DEG_B, None, CAUCHY, HUBER, None),          # pose 1 plane edges only, poses 23.. line edges only
    "BA": (DEG_B, DEG_A, None, TUKEY, NONE, None),
    "C_plane": (DEG_C, None, FREE_C, TUKEY, NONE, None),
    "C_line": (None, DEG_C, FREE_C, NONE, CAUCHY, None),
    "C_both": (DEG_C, DEG_C2B, FREE_C, HUBER, CAUCHY, None),
    "C2_plane": (DEG_C2, None, FREE_C2, NONE, NONE, None),
    "C2_line": (None, DEG_C2, FREE_C2, NONE, HUBER, None),
    "C0": (DEG_C, DEG_C2B, 0, CAUCHY, HUBER, None),        # n_poses_free = 0
    "D_plane": (DEG_D, None, None, HUBER, NONE, {"plane": INACT_D}),
    "D_line": (None, DEG_D, None, NONE, CAUCHY, {"line": INACT_D}),
    "D_both": (DEG_D, DEG_A[:6], None, HUBER, CAUCHY, {"plane": INACT_D, "line": np.arange(63, 65)}),
}


def _degrees(rng, n, P):
    d = rng.multinomial(n - P, np.ones(P) / P) + 1
    assert d.sum() == n
    return d.tolist()


@functools.lru_cache(maxsize=None)
def icp_layout(name):
    if name in ICP_LAYOUTS:
        dp, dl, nf, rp, rl, ina = ICP_LAYOUTS[name]
        return _icp(100 + sorted(ICP_LAYOUTS).index(name), dp, dl, nf, rp, rl, ina)
    if name == "F":       # 129 x 512 + 1 plane and 127 x 512 line edges: 130 + 127 = 257 chunk totals
        rng = np.random.default_rng(7)
        return _icp(201, _degrees(rng, 128 * CHUNK + 1, 40) + [300, 212], _degrees(rng, 127 * CHUNK - 100, 40) + [60, 40], 40,
                    (1, 0.2), (3, 0.1))
    if name == "G":       # 513 x 512 plane edges, the error pass only: 513 totals, 262 656 edges (> 1024 x 256)
        rng = np.random.default_rng(8)
        return _icp(202, _degrees(rng, 513 * CHUNK - 700, 30) + [400, 300], None, 30, HUBER, NONE)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def icp_zero_residual(rk):
    """I-E: identity rotations, integer translations and points, axis-aligned planes through / lines along the
    transformed point: r is exactly 0 in double.  3 poses x (5 plane + 5 line) edges, robust kernel `rk` on both kinds"""
    rng = np.random.default_rng(55)
    P = 3
    poses = np.zeros((P, 7))
    poses[:, 3] = 1.0
    poses[:, 4:] = rng.integers(-8, 9, (P, 3))
    out = dict(poses=poses, n_free=P, P=P)
    for kind in ("plane", "line"):
        pose = np.repeat(np.arange(P, dtype=np.int32), 5)
        E = len(pose)
        p = rng.integers(-9, 10, (E, 3)).astype(np.float64)
        y = p + poses[pose, 4:]
        ax = np.zeros((E, 3))
        ax[np.arange(E), rng.integers(0, 3, E)] = rng.choice([-1.0, 1.0], E)
        e = dict(pose=pose, p=p, omega=rng.uniform(0.5, 3.0, E), active=np.ones(E, bool), rk=rk)
        if kind == "plane":
            e["n"], e["d"] = ax, (ax * y).sum(1)
        else:
            e["u"] = ax
            e["a"] = y - rng.integers(-3, 4, E)[:, None] * ax
            e["b"] = e["a"] + 2 * ax
        out[kind] = _finish(e)
    out["census"] = {k: _census_kind(out[k]["pose"], P, out[k]["active"]) for k in ("plane", "line")}
    return out


def device_arrays(e, kind):
    """the planar arrays of cugo_icp_edges for one kind: p [3][n], geo ([4][n] n d | [6][n] a u)"""
    p = np.ascontiguousarray(e["p"].T)
    geo = np.vstack([e["n"].T, e["d"][None, :]]) if kind == "plane" else np.vstack([e["a"].T, e["u"].T])
    return p, np.ascontiguousarray(geo)


def pose_ptr(pose, n_poses_total):
    return np.searchsorted(np.asarray(pose), np.arange(n_poses_total + 1)).astype(np.int32)


# ---------------------------------------------------------------- priors
ANGLES = [0.0, 1e-13, 5e-13, 2e-12, 1e-9, 0.999e-3, 1.001e-3, 0.05, np.pi / 2, 3.0, np.pi - 1e-3, np.pi - 1e-6]
RKS = [(0, 1.0), (1, 0.8), (2, 5.0), (3, 4.0)]
COUNTS_CYCLE = [1, 2, 17, 1, 2, 1]


def counts_A(n_free):
    """P-A: priors per free pose in {0, 1, 2, 17}; no prior on the first and on the last pose of every full workgroup"""
    if n_free == 1:
        return [2]
    c = []
    for p in range(n_free):
        c.append(0 if p % PRIOR_POSES in (0, PRIOR_POSES - 1) else COUNTS_CYCLE[(p - p // PRIOR_POSES) % len(COUNTS_CYCLE)])
    return c


def _prior(seed, counts, n_free, rk=(0, 1.0), info="per_edge", angles=None, inactive_pose=None, rot=0.3, trans=0.5):
    rng = np.random.default_rng(seed)
    P = len(counts)
    poses = np.array([icp_ref.random_pose(rng) for _ in range(P)])
    pose = np.repeat(np.arange(P, dtype=np.int32), counts)
    E = len(pose)
    z = np.zeros((E, 7))
    for i, p in enumerate(pose):
        if angles is None:
            z[i] = prior_ref.displaced(rng, poses[p], rot, trans)
        elif angles[i] == 0.0:
            z[i] = poses[p]                  # theta = 0 exactly: the prior equals the pose
        else:
            axis = rng.normal(size=3)
            axis /= np.linalg.norm(axis)
            z[i] = icp_ref.left_update(poses[p], np.concatenate([-angles[i] * axis, rng.normal(0, 1.0, 3)]))
    if info == "per_edge":
        Om = np.array([prior_ref.random_spd(rng, rng.uniform(0.5, 3.0)) for _ in range(E)]).reshape(-1, 6, 6)
    elif info == "one":
        Om = prior_ref.random_spd(rng, 1.3)[None]
    elif info == "rank3":
        A = rng.normal(size=(6, 3))
        Om = (A @ A.T)[None]
    elif info == "diag":
        Om = np.diag(np.logspace(-6, 6, 6))[None]
    else:
        Om = np.zeros((1, 6, 6))
    active = np.ones(E, bool)
    if inactive_pose is not None:
        active[pose == inactive_pose] = False
    pr = prior_ref.make_prior(pose, z, Om, rk=rk, active=active)
    pr["flags"] = np.where(active, 0, INACTIVE).astype(np.uint8)
    return dict(poses=poses, n_free=n_free, P=P, pr=pr, counts=list(counts), census=_census_prior(poses, n_free, pr, counts))


def _census_prior(poses, n_free, pr, counts):
    """what k_prior meets: priors per free pose, empty poses at the first / last place of a workgroup, poses all of
    whose priors are inactive, fixed poses with priors, workgroup totals, and per residual angle (theta, sin theta from
    the quaternion of D, in double) the side of each of the kernel's two switches"""
    counts = np.asarray(counts)
    pose = np.asarray(pr["pose"], int)
    free = counts[:n_free]
    place = np.arange(n_free) % PRIOR_POSES
    qa, qb = poses[pose, :4], np.asarray(pr["z"]).reshape(-1, 7)[:, :4]
    v = qb[:, 3:] * qa[:, :3] - qa[:, 3:] * qb[:, :3] - np.cross(qa[:, :3], qb[:, :3])
    w = np.abs(qa[:, 3] * qb[:, 3] + (qa[:, :3] * qb[:, :3]).sum(1))
    nv = np.linalg.norm(v, axis=1)
    theta, sn = 2 * np.arctan2(nv, w), 2 * w * nv
    on_free = pose < n_free
    th, s = theta[on_free], sn[on_free]
    return {"priors_per_free_pose": sorted(set(free.tolist())), "workgroups": (n_free + PRIOR_POSES - 1) // PRIOR_POSES if len(pose) else 0,
            "empty_at_first_of_workgroup": int(((free == 0) & (place == 0)).sum()),
            "empty_at_last_of_workgroup": int(((free == 0) & (place == PRIOR_POSES - 1)).sum()),
            "all_inactive_poses": [p for p in range(n_free) if counts[p] and not pr["active"][pose == p].any()],
            "fixed_poses_with_priors": int((counts[n_free:] > 0).sum()), "theta": th, "sn": s,
            "sn_le_1e-12": int((s <= 1e-12).sum()), "sn_gt_1e-12": int((s > 1e-12).sum()),
            "theta_lt_1e-3": int((th < 1e-3).sum()), "theta_ge_1e-3": int((th >= 1e-3).sum()), "near_pi": int((np.pi - th < 2e-3).sum())}


@functools.lru_cache(maxsize=None)
def prior_layout(name):
    """'A<n_free>', 'A_empty', 'B', 'C_<info>_<rk index>', 'D2049', 'D4104'"""
    if name == "A_empty":
        return _prior(300, [0, 0, 0], 2)
    if name.startswith("A"):
        nf = int(name[1:])
        counts = counts_A(nf) + [2, 1]                            # two fixed poses with priors
        return _prior(300 + nf, counts, nf, rk=RKS[nf % 4], inactive_pose=2 if nf >= 7 else None)
    if name == "B":
        return _prior(330, [1] * len(ANGLES), len(ANGLES), angles=ANGLES)
    if name.startswith("C_"):
        _, info, k = name.split("_")
        info = {"perEdge": "per_edge"}.get(info, info)
        lay = _prior(340, [2, 1, 3, 0, 2], 5, rk=RKS[int(k)], info=info, trans=2.0)
        lay["pr"]["z"][0] = lay["poses"][0]                       # a prior equal to its pose: x = 0 up to rounding
        return lay
    if name.startswith("D"):
        nf = int(name[1:])
        return _prior(350, [1] * nf, nf, rk=(3, 4.0), info="one")
    raise KeyError(name)


PRIOR_NAMES = (["A%d" % n for n in (1, 7, 8, 9, 16, 17)] + ["A_empty", "B"] +
               ["C_%s_%d" % (i, k) for i in ("one", "perEdge", "rank3", "diag", "zero") for k in range(4)] + ["D2049", "D4104"])


def per_edge_info(pr):
    return dict(pr, info=np.tile(pr["info"], (len(pr["pose"]), 1, 1))) if len(pr["info"]) == 1 else pr


# ---------------------------------------------------------------- Schur destination
def schur_rows(P, seed=77):
    """an upper block CSR with rows of 1 to 4 blocks in which NO diagonal block sits at index p: one spare block in
    front.  Returns rowptr [P + 1] (rowptr[p] = pose p's diagonal block) and the block count"""
    rng = np.random.default_rng(seed)
    n = rng.integers(1, 5, P)
    rowptr = np.concatenate([[1], 1 + np.cumsum(n)]).astype(np.int32)
    assert np.all(rowptr[:P] != np.arange(P))
    return rowptr, int(rowptr[-1])


# ---------------------------------------------------------------- relative-pose edges (relpose_kernels.hip)
# A layout is dict(poses [P,7], n_free, P (all poses, free first), rp (relpose_ref.make_edges + flags = the plan's flags,
# rt_active / rt_flags = what the device is given), rowptr, colind (the pattern of the plan's edges plus spare blocks no edge
# maps to: (p, n_free - 1) in every row), census).  RELPOSE_POSES = 4 poses (waves) per workgroup.
RELPOSE_POSES = 4
RELPOSE_NAMES = (["R-wg%d" % n for n in (1, 3, 4, 5, 8, 9)] + ["R-sides", "R-angles", "R-far"] + ["R-rk%d" % k for k in range(4)] +
                 ["R-info_perEdge", "R-info_one", "R-info_singular", "R-info_indef"])
RELPOSE_ZERO = ["R-zero%d" % k for k in range(4)]
RELPOSE_TOTALS = ["R-totals%d" % n for n in (1024, 1025, 1029)]
SIDES_HUB, SIDES_BIG, SIDES_EMPTY, SIDES_PLAN_OFF, SIDES_RT_OFF, SIDES_ONE, SIDES_FREE = 3, 0, 4, 10, 11, 12, 13
RK_X = [0.1, 0.5, 0.9, 1.1, 2.0, 10.0]          # R-rk: x / delta^2 of the edges, in turn


def relpose_pattern_with_spares(rp, n_free):
    import relpose_ref as RR
    rowptr, colind = RR.pattern(rp, n_free)
    rows = [set(colind[rowptr[p] + 1:rowptr[p + 1]].tolist()) | ({n_free - 1} if p < n_free - 1 else set()) for p in range(n_free)]
    ci, rp_ = [], [0]
    for p in range(n_free):
        ci += [p] + sorted(rows[p])
        rp_.append(len(ci))
    return np.array(rp_, np.int32), np.array(ci, np.int32)


def relpose_census(lay, inc_ptr=None, inc=None, off_blk=None):
    """what k_relpose meets, from the plan's arrays (those of relpose_ref.plan unless the C plan's are handed in)"""
    import relpose_ref as RR
    rp, nf = lay["rp"], lay["n_free"]
    if inc_ptr is None:
        inc_ptr, inc, off_blk = RR.plan(rp, nf, lay["rowptr"], lay["colind"])
    a, b = np.asarray(rp["a"], int), np.asarray(rp["b"], int)
    E = len(a)
    rt = np.asarray(rp["rt_active"], bool)
    deg = np.diff(inc_ptr)
    wgs = (nf + RELPOSE_POSES - 1) // RELPOSE_POSES if E and nf else 0
    walked = np.zeros(E, bool)
    walked[np.asarray(inc, int) >> 1] = True
    touching = [np.flatnonzero((a == p) | (b == p)) for p in range(nf)]
    c = dict(workgroups=wgs, idle_waves_in_last_workgroup=wgs * RELPOSE_POSES - nf, degrees=deg.tolist(),
             fixed_fixed=int(((a >= nf) & (b >= nf)).sum()), fixed_fixed_walked=int((walked & (a >= nf) & (b >= nf)).sum()),
             poses_without_any_edge_between_active=[p for p in range(1, nf - 1) if len(touching[p]) == 0 and deg[p - 1] and deg[p + 1]],
             poses_all_inactive_in_plan=[p for p in range(nf) if len(touching[p]) and deg[p] == 0],
             poses_inactive_at_run_time_only=[p for p in range(nf) if deg[p] and not rt[touching[p]].any() and rp["active"][touching[p]].all()],
             blocks_no_edge_maps_to=int(len(lay["colind"]) - nf - len(set(off_blk[off_blk >= 0].tolist()))),
             rows_with_rowptr_ne_p=int((lay["rowptr"][:nf] != np.arange(nf)).sum()))
    k = np.asarray(off_blk)
    cnt = RR.counting(rp, nf)
    nb = np.zeros(E, bool)
    nb[:-1] |= k[1:] >= 0
    nb[1:] |= k[:-1] >= 0
    c["no_block_next_to_block"] = int((cnt & (k < 0) & nb).sum())
    per_pair, mixed = {}, {}
    for e in np.flatnonzero(k >= 0):
        per_pair[k[e]] = per_pair.get(k[e], 0) + 1
        mixed.setdefault(k[e], set()).add(bool(a[e] < b[e]))
    c["edges_per_pair"] = sorted(set(per_pair.values()))
    c["pairs_in_mixed_orientation"] = sorted(per_pair[q] for q in per_pair if len(mixed[q]) == 2)
    h = lay.get("hub")
    if h is not None:
        cases = dict(a_hi=0, a_lo=0, b_hi=0, b_lo=0, a_fixed=0, b_fixed=0)
        for rec in inc[inc_ptr[h]:inc_ptr[h + 1]]:
            e, side = int(rec) >> 1, int(rec) & 1
            other = a[e] if side else b[e]
            cases[("b_" if side else "a_") + ("fixed" if other >= nf else "hi" if other > h else "lo")] += 1
        c["hub"] = cases
    return c


def _rel_finish(poses, n_free, rp, rt_active=None, **extra):
    rp["flags"] = np.where(rp["active"], 0, INACTIVE).astype(np.uint8)
    rp["rt_active"] = rp["active"].copy() if rt_active is None else np.asarray(rt_active, bool) & rp["active"]
    rp["rt_flags"] = np.where(rp["rt_active"], 0, INACTIVE).astype(np.uint8)
    rowptr, colind = relpose_pattern_with_spares(rp, n_free)
    lay = dict(poses=poses, n_free=n_free, P=len(poses), rp=rp, rowptr=rowptr, colind=colind, **extra)
    lay["census"] = relpose_census(lay)
    return lay


def _chain_pairs(n_free):
    """n_free free poses and two fixed ones with mid-range ids (remapped to the tail: free first): a chain in alternating
    orientation plus two chords"""
    N = n_free + 2
    fixed = [N // 3, (2 * N) // 3] if N > 3 else [1, 2]
    new = {}
    for i in range(N):
        if i not in fixed:
            new[i] = len(new)
    for i in fixed:
        new[i] = len(new)
    pairs = [(new[i], new[i + 1]) if i % 2 == 0 else (new[i + 1], new[i]) for i in range(N - 1)]
    pairs += [(new[0], new[N - 1]), (new[N // 2], new[0])]
    return pairs


def _rel_random(seed, n_free, pairs, rk=(0, 1.0), rot=0.05, trans=0.3, per_edge_info=True, P=None):
    import relpose_ref as RR
    rng = np.random.default_rng(seed)
    P = n_free + 2 if P is None else P
    poses = np.array([icp_ref.random_pose(rng) for _ in range(P)])
    return rng, poses, RR.random_edges(rng, poses, pairs, rk=rk, rot=rot, trans=trans, per_edge_info=per_edge_info)


def _sides(seed, rk, scale_to_rk=False):
    """R-sides: see the census.  13 free poses, 2 fixed"""
    nf = SIDES_FREE
    h, f0, f1 = SIDES_HUB, nf, nf + 1
    pairs = [(h, f0), (h, 5), (h, 1), (5, h), (1, h), (f1, h),            # the hub: a to fixed (no block) next to a to hi
             (f0, f1),                                                      # fixed-fixed
             (6, 8), (8, 6), (6, 8),                                        # three on one pair
             (SIDES_ONE, 2)]                                                # a pose with this one edge
    pairs += [(7, 9) if k % 2 == 0 else (9, 7) for k in range(40)]          # 40 on one pair, alternating
    n_plan_off = len(pairs)
    pairs += [(SIDES_PLAN_OFF, 2), (1, SIDES_PLAN_OFF)]                     # inactive in the plan
    n_rt_off = len(pairs)
    pairs += [(SIDES_RT_OFF, 2), (5, SIDES_RT_OFF), (SIDES_RT_OFF, f0)]     # inactive at run time only
    n_big = len(pairs)
    partners = [1, 2, 5, 6, 7, 8, 9, f0, f1]
    rng0 = np.random.default_rng(seed + 1000)
    for k in range(300):
        q = partners[k % len(partners)]
        pairs.append((SIDES_BIG, q) if rng0.random() < 0.5 else (q, SIDES_BIG))
    rng, poses, rp = _rel_random(seed, nf, pairs, rk=rk, rot=0.1, trans=0.3)
    rp["active"][n_plan_off:n_rt_off] = False
    rt = np.ones(len(pairs), bool)
    rt[n_rt_off:n_big] = False
    if scale_to_rk:
        import relpose_ref as RR
        d2 = rk[1] ** 2
        for e in range(len(pairs)):
            r = RR.residual(poses[rp["a"][e]], poses[rp["b"][e]], rp["z"][e])
            rp["info"][e] *= RK_X[e % len(RK_X)] * d2 / float(r @ rp["info"][e] @ r)
    return _rel_finish(poses, nf, rp, rt, hub=h)


def _census_x(lay):
    """R-rk: counting edges inside / outside delta^2 (x in double)"""
    import relpose_ref as RR
    rp = lay["rp"]
    eff = dict(rp, active=rp["rt_active"])
    x = np.array([float(RR.residual(lay["poses"][a], lay["poses"][b], z) @ Om @ RR.residual(lay["poses"][a], lay["poses"][b], z))
                  for a, b, z, Om in zip(rp["a"], rp["b"], rp["z"], np.broadcast_to(rp["info"], (len(rp["a"]), 6, 6)))])
    x = x[RR.counting(eff, lay["n_free"])]
    return dict(inside=int((x <= rp["rk"][1] ** 2).sum()), outside=int((x > rp["rk"][1] ** 2).sum()), negative=int((x < 0).sum()))


def _census_angles(lay):
    """theta and sin theta of D from its quaternion, in double, per edge (as _census_prior)"""
    import synth
    rp, poses = lay["rp"], lay["poses"]
    th, sn = [], []

    def conj(q):
        return np.array([-q[0], -q[1], -q[2], q[3]])
    for a, b, z in zip(rp["a"], rp["b"], rp["z"]):
        q = synth.quat_mul(synth.quat_mul(poses[a][:4], conj(poses[b][:4])), conj(z[:4]))
        nv, w = np.linalg.norm(q[:3]), abs(q[3])
        th.append(2 * np.arctan2(nv, w)), sn.append(2 * w * nv)
    th, sn = np.array(th), np.array(sn)
    return {"theta": th, "sn": sn, "sn_le_1e-12": int((sn <= 1e-12).sum()), "sn_gt_1e-12": int((sn > 1e-12).sum()),
            "theta_lt_1e-3": int((th < 1e-3).sum()), "theta_ge_1e-3": int((th >= 1e-3).sum()), "near_pi": int((np.pi - th < 2e-3).sum())}


HURWITZ = [np.array(q, float) for q in
           [(1, 0, 0, 0), (0, -1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (.5, .5, .5, .5), (-.5, .5, .5, .5), (.5, -.5, .5, .5),
            (.5, .5, -.5, .5), (-.5, -.5, .5, .5), (.5, -.5, -.5, .5)]]


@functools.lru_cache(maxsize=None)
def relpose_layout(name):
    """'R-wg<n_free>', 'R-sides', 'R-angles', 'R-far', 'R-zero<k>', 'R-rk<k>' (k: index into RKS), 'R-info_<perEdge | one | singular |
    indef>', 'R-totals<n_free>'"""
    import relpose_ref as RR
    import synth
    if name.startswith("R-wg"):
        nf = int(name[4:])
        rng, poses, rp = _rel_random(400 + nf, nf, _chain_pairs(nf), rk=RKS[nf % 4], rot=0.2, trans=0.5)
        return _rel_finish(poses, nf, rp)
    if name == "R-sides":
        return _sides(420, (0, 1.0))
    if name.startswith("R-rk"):
        lay = _sides(421, RKS[int(name[4:])], scale_to_rk=True)
        lay["census"]["x"] = _census_x(lay)
        return lay
    if name == "R-angles":
        # hub 3; partners 0..2, 4..6 free, 7 fixed; R_partner = Rot(2 rad about its own axis)^T R_hub, so R_A is that rotation
        # (or its transpose with the hub as b) and D is small only because Z cancels it
        rng = np.random.default_rng(430)
        nf, h = 7, 3
        poses = np.zeros((8, 7))
        poses[h] = icp_ref.random_pose(rng)
        for p in range(8):
            if p != h:
                ax = rng.normal(size=3)
                q = synth.quat_mul(synth.quat_from_rotvec(-rng.uniform(1.9, 2.1) * ax / np.linalg.norm(ax)), poses[h][:4])
                poses[p] = np.concatenate([q / np.linalg.norm(q), rng.normal(0, 2.0, 3)])
        free = [0, 1, 2, 4, 5, 6]
        pairs, angles = [], []
        for role in range(3):
            for i, th in enumerate(ANGLES):
                for k in range(3):
                    q = free[(3 * i + k) % 6]
                    pairs.append([(h, q), (q, h), (h, 7)][role])
                    angles.append(th)
        z = np.array([RR.measured(rng, poses[a], poses[b], trans=1.0, angle=th) for (a, b), th in zip(pairs, angles)])
        info = np.array([prior_ref.random_spd(rng, rng.uniform(0.5, 3.0)) for _ in pairs])
        pairs = np.array(pairs, np.int32)
        lay = _rel_finish(poses, nf, RR.make_edges(pairs[:, 0], pairs[:, 1], z, info), hub=h)
        lay["census"]["angles"] = _census_angles(lay)
        lay["angles"] = np.array(angles)
        RA = [RR.relative(poses[a], poses[b])[0] for a, b in pairs]
        lay["census"]["R_A_angle"] = (min(np.arccos((np.trace(R) - 1) / 2) for R in RA), max(np.arccos((np.trace(R) - 1) / 2) for R in RA))
        return lay
    if name == "R-far":
        # camera centres c = C0 + N(0, 1), t = -R c: |t| ~ 1e3, t_A = R_a (c_b - c_a) of order 1
        rng = np.random.default_rng(440)
        nf = 10
        poses = np.array([icp_ref.random_pose(rng) for _ in range(12)])
        for p in range(12):
            poses[p, 4:] = -synth.quat_to_R(poses[p, :4]) @ (np.array([600.0, -500.0, 700.0]) + rng.normal(0, 1.0, 3))
        pairs = _chain_pairs(nf) + [(2, 7), (9, 4), (5, 1)]
        rp = RR.random_edges(rng, poses, pairs, rot=0.05, trans=1e-2)
        lay = _rel_finish(poses, nf, rp)
        t = [RR.relative(poses[a], poses[b]) for a, b in pairs]
        lay["census"]["tA_rel"] = [float(np.linalg.norm(tA) / (np.abs(poses[a][4:]).sum() + (np.abs(RA) @ np.abs(poses[b][4:])).sum()))
                                   for (RA, tA), (a, b) in zip(t, pairs)]
        lay["census"]["t_norm"] = [float(np.linalg.norm(p[4:])) for p in poses]
        lay["census"]["tD_norm"] = [float(np.linalg.norm(RR.residual(poses[a], poses[b], z)[3:])) for (a, b), z in zip(pairs, rp["z"])]
        return lay
    if name.startswith("R-zero"):
        # unit quaternions with entries in {0, +-1, +-1/2} (their products are again such: exact), translations in quarters
        rng = np.random.default_rng(450)
        nf = 6
        poses = np.array([np.concatenate([HURWITZ[i], rng.integers(-16, 17, 3) / 4.0]) for i in rng.permutation(len(HURWITZ))[:nf + 1]])
        pairs = [(0, 1), (2, 1), (2, 3), (4, 3), (4, 5), (6, 5), (0, 6), (5, 0), (3, 1), (1, 3)]
        z = []
        for a, b in pairs:
            qb = poses[b][:4] * np.array([-1, -1, -1, 1.0])
            RA = synth.quat_to_R(poses[a][:4]) @ synth.quat_to_R(poses[b][:4]).T
            z.append(np.concatenate([synth.quat_mul(poses[a][:4], qb), poses[a][4:] - RA @ poses[b][4:]]))
        info = np.array([prior_ref.random_spd(rng, 1.5) for _ in pairs])
        pairs = np.array(pairs, np.int32)
        return _rel_finish(poses, nf, RR.make_edges(pairs[:, 0], pairs[:, 1], np.array(z), info, rk=RKS[int(name[6:])]))
    if name.startswith("R-info_"):
        kind = name[7:]
        nf = 9
        rng, poses, rp = _rel_random(460, nf, _chain_pairs(nf) + [(0, 1), (4, 2)], rk=RKS[1] if kind in ("perEdge", "one") else (0, 1.0),
                                     rot=0.3, trans=0.3)
        E = len(rp["a"])
        S = np.diag([1e3] * 3 + [1.0] * 3)          # Omega = A A^T: rotation block 1e6 x the translation block
        per = np.array([(lambda A: A @ A.T)(S @ rng.normal(size=(6, 6))) for _ in range(E)])
        rp["info"] = {"perEdge": per, "one": per[:1], "singular": np.diag([0, 0, 0, 4.0, 2.0, 1.0])[None],
                      "indef": np.diag([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0])[None]}[kind]
        lay = _rel_finish(poses, nf, rp)
        lay["census"]["x"] = _census_x(lay)
        return lay
    if name.startswith("R-totals"):
        nf = int(name[8:])
        N = nf + 1                                   # a ring, one fixed pose (index nf), one edge per pose
        rng = np.random.default_rng(470)
        poses = np.array([icp_ref.random_pose(rng) for _ in range(N)])
        pairs = [(i, (i + 1) % N) for i in range(N)]
        rp = RR.random_edges(rng, poses, pairs, rk=(3, 4.0), per_edge_info=False, rot=0.1, trans=0.3)
        return _rel_finish(poses, nf, rp)
    raise KeyError(name)


def relpose_per_edge_info(rp):
    return dict(rp, info=np.tile(rp["info"], (len(rp["a"]), 1, 1))) if len(rp["info"]) == 1 else rp
