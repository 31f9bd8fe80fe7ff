"""Designed layouts for the pose-pose point edge kernels (point_pair_kernels.hip): the smallest shapes at which the run /
chunk / role reduction can go wrong, around ICP_CHUNK = 512 and the 64-lane groups.  Built programmatically with fixed
seeds (numpy only); every layout carries its census, which test_point_pair_ref_host.py asserts.

A set is the dict of point_pair_ref: a, b [E] in the CALLER's order (a random permutation of the sorted order, so that
fixed-fixed and inactive edges are sprinkled through the container and the plan's stable sort has work to do), p, z
[E,3], info6 [E,6] or [1,6], active [E], flags [E] uint8, rk.

The layout 'A' (80 poses, 72 free; 2502 edges), runs in the plan's order (lo, hi, orientation), a -> b:
    0->1 63 | 1->0 1 | 0->2 1        runs ending at edges 63 / 64 / 65; the pair (0, 1) in both orientations: two runs, one
                                     block, the second transposed
    0->3 446 | 4->0 1 | 0->5 1       ... at 511 / 512 / 513 (10 % of the 446 inactive)
    0->72 510 | 73->0 1              ... at 1023 / 1024; b fixed; a fixed
    1->2 1300                        one run over three chunks (1024 .. 2323), 10 % inactive
    3->1 44                          up to the group boundary 2368
    2->3+k / 3+k->2, k < 64, 1 each  64 different runs inside one 64-lane group; pose 2 has 66 incident runs
    l->70 / 70->l, l = 4 .. 20, 3    pose 70: a in some runs and b in others, 17 incident runs
    21->67 5                         pose 67: one incident run; poses 68, 69, 71: free, no edge, between poses with edges
    22->23 6                         a run that is entirely inactive
    74->22 2 | 23->75 2              runs whose a / b is fixed
    72->73 4                         fixed-fixed: counts for nothing
under the Omega classes of point_designed.make_info ('spd', 'one' = one matrix for all, 'rank1', 'rank2', 'zero') and
general rotations.  'B': 6 poses, one fixed, a ring plus two chords in random orientations, 40 edges per pair.  'Z':
exactly zero residuals.  'G': 270 000 edges on three poses, for the index check beyond its first grid-stride trip only."""
import functools

import numpy as np

import icp_ref
import point_designed as pt
import point_pair_ref as ppr
from pose_designed import CAUCHY, TUKEY, HUBER, NONE, CHUNK, INACTIVE

P_ALL_A, P_FREE_A = 80, 72


def runs_A():
    """(a, b, size, inactive fraction) in the plan's order"""
    runs = [(0, 1, 63, 0), (1, 0, 1, 0), (0, 2, 1, 0), (0, 3, 446, 0.1), (4, 0, 1, 0), (0, 5, 1, 0), (0, 72, 510, 0), (73, 0, 1, 0),
            (1, 2, 1300, 0.1), (3, 1, 44, 0)]
    runs += [((2, 3 + k) if k % 2 == 0 else (3 + k, 2)) + (1, 0) for k in range(64)]
    runs += [((l, 70) if l % 2 == 0 else (70, l)) + (3, 0) for l in range(4, 21)]
    runs += [(21, 67, 5, 0), (22, 23, 6, 1.0), (74, 22, 2, 0), (23, 75, 2, 0), (72, 73, 4, 0)]
    return runs


def _make(seed, n_poses, n_free, runs, rk, cls, noise=0.3, shuffle=True):
    rng = np.random.default_rng(seed)
    poses = np.array([icp_ref.random_pose(rng) for _ in range(n_poses)])
    a = np.concatenate([np.full(r[2], r[0]) for r in runs]).astype(np.int32)
    b = np.concatenate([np.full(r[2], r[1]) for r in runs]).astype(np.int32)
    E = len(a)
    active = np.ones(E, bool)
    i0 = 0
    for r in runs:
        if r[3] >= 1.0:
            active[i0:i0 + r[2]] = False
        elif r[3] > 0:
            active[i0:i0 + r[2]][rng.random(r[2]) < r[3]] = False
        i0 += r[2]
    Xw = rng.normal(0, 2.0, (E, 3))
    R = lambda i: ppr._rot(poses[i, :4])[0]
    p = np.einsum("eij,ej->ei", R(a), Xw) + poses[a, 4:] + rng.normal(0, noise, (E, 3))
    z = np.einsum("eij,ej->ei", R(b), Xw) + poses[b, 4:] + rng.normal(0, noise, (E, 3))
    info6, lam = pt.make_info(rng, cls, E)
    sorted_e = dict(a=a, b=b, p=p, z=z, info6=info6, active=active)
    order = rng.permutation(E) if shuffle else np.arange(E)
    e = {k: (v[order] if len(v) == E else v) for k, v in sorted_e.items()}
    e["flags"] = np.where(e["active"], 0, INACTIVE).astype(np.uint8)
    e["rk"] = rk
    return dict(poses=poses, n_free=n_free, P=n_poses, e=e, runs=runs, census=census(e, n_free, n_poses), omega_class=cls, lam=lam)


def census(e, n_free, n_poses):
    """what the layout is designed to hold, from the set alone"""
    plan = ppr.numpy_plan(e["a"], e["b"], e["active"], n_free)
    rp = plan["run_ptr"]
    ends = rp[1:]
    slots = sum((rp[r + 1] - 1) // CHUNK - rp[r] // CHUNK + 1 for r in range(len(plan["run_a"])))
    groups = plan["edge_run"][: len(plan["edge_run"]) // 64 * 64].reshape(-1, 64)
    fl = plan["run_flags"]
    cnt = fl & ppr.RUN_COUNTS != 0
    return dict(n=len(e["a"]), n_runs=len(plan["run_a"]), run_ends=set(int(x) for x in ends), slots=int(slots),
                max_chunks_of_a_run=int(max((rp[r + 1] - 1) // CHUNK - rp[r] // CHUNK + 1 for r in range(len(plan["run_a"])))),
                max_runs_in_a_group=int(max(len(np.unique(g)) for g in groups)) if len(groups) else 0,
                incident=np.diff(plan["inc_ptr"]), n_pairs=len(plan["pair_lo"]),
                two_run_pairs=int(sum(np.diff(ppr.numpy_plan(e["a"], e["b"], e["active"], n_free,
                                                             *ppr.pair_pattern(n_free, plan["pair_lo"], plan["pair_hi"]))["blk_ptr"]) == 2)),
                runs_a_fixed=int(np.sum(cnt & (fl & ppr.RUN_A_FREE == 0))), runs_b_fixed=int(np.sum(cnt & (fl & ppr.RUN_B_FREE == 0))),
                runs_not_counting=int(np.sum(~cnt)), n_inactive=int(np.sum(~np.asarray(e["active"]))))


LAYOUTS = {
    "A_spd": (CAUCHY, "spd"), "A_one": (HUBER, "one"), "A_rank1": (TUKEY, "rank1"), "A_rank2": (NONE, "rank2"), "A_zero": (NONE, "zero"),
}
NAMES = list(LAYOUTS) + ["B"]


@functools.lru_cache(maxsize=None)
def layout(name):
    if name in LAYOUTS:
        rk, cls = LAYOUTS[name]
        return _make(700 + list(LAYOUTS).index(name), P_ALL_A, P_FREE_A, runs_A(), rk, cls)
    if name == "B":       # a ring of 6 plus two chords, pose 5 fixed, random orientations
        rng = np.random.default_rng(31)
        pairs = [(i, (i + 1) % 6) for i in range(6)] + [(0, 3), (1, 4)]
        runs = sorted(((p if rng.random() < 0.5 else p[::-1]) + (40, 0.05) for p in pairs), key=lambda r: (min(r[:2]), max(r[:2]), r[0] > r[1]))
        return _make(731, 6, 5, runs, HUBER, "spd", noise=0.05)
    if name == "G":       # more edges than one grid-stride trip of the index check covers (1024 x 256)
        return _make(741, 3, 2, [(0, 1, 200000, 0), (0, 2, 70000, 0)], NONE, "one", shuffle=False)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def zero_residual(rk):
    """identity rotations, integer translations and points, z = y exactly, Omega with small integer entries (SPD): r and x
    are exactly 0 in double.  4 poses (one fixed), 6 pairs x 3 edges"""
    rng = np.random.default_rng(57)
    P = 4
    poses = np.zeros((P, 7))
    poses[:, 3] = 1.0
    poses[:, 4:] = rng.integers(-8, 9, (P, 3))
    pairs = [(0, 1), (2, 0), (0, 3), (1, 2), (3, 1), (2, 3)]
    a = np.repeat([x[0] for x in pairs], 3).astype(np.int32)
    b = np.repeat([x[1] for x in pairs], 3).astype(np.int32)
    E = len(a)
    p = rng.integers(-9, 10, (E, 3)).astype(np.float64)
    A = rng.integers(-2, 3, (E, 3, 3)).astype(np.float64)
    Om = np.einsum("eik,ejk->eij", A, A) + np.eye(3)[None]
    e = dict(a=a, b=b, p=p, z=p - poses[a, 4:] + poses[b, 4:], info6=ppr.pack(Om), active=np.ones(E, bool), flags=np.zeros(E, np.uint8), rk=rk)
    return dict(poses=poses, n_free=3, P=P, e=e, census=census(e, 3, P))


def device_arrays(e, perm):
    """the arrays of cugo_point_pair_edges in the plan's sorted order: pose_a, pose_b [n], p [3][n], z [3][n], info
    [6][n_info], flags [n]"""
    info = np.asarray(e["info6"], np.float64).reshape(-1, 6)
    if len(info) > 1:
        info = info[perm]
    return (np.asarray(e["a"], np.int32)[perm], np.asarray(e["b"], np.int32)[perm],
            np.ascontiguousarray(np.asarray(e["p"], np.float64)[perm].T), np.ascontiguousarray(np.asarray(e["z"], np.float64)[perm].T),
            np.ascontiguousarray(info.T), None if e.get("flags") is None else np.asarray(e["flags"], np.uint8)[perm])
