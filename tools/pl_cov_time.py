"""Host-clock time of Graph.pose_landmark_cross_covariances and Graph.reprojection_covariances — Sigma_al and
S = J Sigma J^T of (pose, landmark) pairs: the build pass, the Schur complement and one factorisation at lambda = 0, the
plan of the batch, cugo_chol_inverse_blocks for its pose pairs, then k_pose_lm_cross (and, for S, the selected inverse,
k_lm_covariance and k_reprojection_cov) — for two batches:

    one keyframe x every landmark      on the local-BA window (30 / 3 000 / 12 600) and on the kitti_00 shape
    1 000 random pairs                 on both

median of --reps calls after a warm-up; every figure ends in a device synchronise (the call returns with its results on
the host).  Next to each: Graph.pose_cross_covariances for the pose pairs the batch needs (the plan's list, rebuilt here
from the edges: (a, p) for every free pose p that observes the query's landmark, and (a, a)) — what the pose blocks
alone cost.

    python tools/pl_cov_time.py [--reps 5] [--shapes window,kitti00]

For the per-kernel averages run it in a pass of its own under
`rocprofv3 --kernel-trace --stats -- python tools/pl_cov_time.py` (k_pose_lm_cross, k_reprojection_cov)."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
cugo = importlib.import_module("cuda-bundle-adjustment_amd")

SHAPES = {  # (poses, landmarks, edges, seed, loop-closure landmarks, stereo fraction)
    "window": (30, 3000, 12600, 0, 0, 0.7),
    "kitti00": (1322, 133383, 561116, 0, 4000, 0.7),   # as in bench.py
}


def median_ms(fn, reps):
    fn()  # warm-up: the first call allocates the buffers
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def pose_pairs(d, qa, ql):
    """the distinct pose pairs a batch needs: (a, p) for every free pose p with an edge to the query's landmark, (a, a)"""
    order = np.argsort(d["e_lm"], kind="stable")
    ptr = np.searchsorted(d["e_lm"][order], np.arange(len(d["lm"]) + 1))
    free = d["pose_fixed"] == 0
    keys = set()
    P = len(d["pose"])
    for a, l in zip(qa.tolist(), ql.tolist()):
        if not free[a]:
            continue
        keys.add(a * P + a)
        for p in d["e_pose"][order[ptr[l]:ptr[l + 1]]].tolist():
            if free[p]:
                keys.add(a * P + p)
    keys = np.array(sorted(keys), np.int64)
    return (keys // P).astype(np.int32), (keys % P).astype(np.int32)


def time_shape(g, d, name, a):
    P, L = len(d["pose"]), len(d["lm"])
    rng = np.random.default_rng(1)
    kf = P - 1   # the newest keyframe
    # (a landmark with fewer than two edges may have a singular Hll: a query that names it fails the call)
    lms = np.flatnonzero(np.bincount(d["e_lm"], minlength=L) >= 2).astype(np.int32)
    batches = [("keyframe %d x %d landmarks" % (kf, len(lms)), np.full(len(lms), kf, np.int32), lms),
               ("1000 random pairs", rng.integers(1, P, 1000).astype(np.int32), rng.choice(lms, 1000).astype(np.int32))]
    for what, qa, ql in batches:
        pa, pb = pose_pairs(d, qa, ql)
        cross = median_ms(lambda: g.pose_landmark_cross_covariances(qa, ql), a.reps)
        s2 = median_ms(lambda: g.reprojection_covariances(qa, ql, dim=2, cam=d["cam"]), a.reps)
        pp = median_ms(lambda: g.pose_cross_covariances(pa, pb), a.reps)
        print("%-8s %-32s %6d queries, %6d pose pairs | Sigma_al: median %.3f ms (min %.3f, max %.3f) | S: median %.3f ms "
              "(min %.3f, max %.3f) | pose_cross_covariances of the pairs: median %.3f ms (%d reps)"
              % (name, what, len(qa), len(pa), cross[0], cross[1], cross[2], s2[0], s2[1], s2[2], pp[0], a.reps), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="window,kitti00")
    a = ap.parse_args()
    for name in a.shapes.split(","):
        P, L, E, seed, lc, st = SHAPES[name]
        d = cugo.synth(P, L, E, seed=seed, n_loop_closures=lc, stereo_fraction=st)
        g = cugo.graph_from_arrays(d)
        g.initialize()
        g.optimize(10)
        g.optimize(10)  # (as tools/cov_time.py: the covariances of the estimates 20 iterations leave)
        try:
            time_shape(g, d, name, a)
        except cugo.CugoError as e:  # (a zero pivot or an edgeless landmark: nothing to time)
            print("%-8s not measured: %s" % (name, e), flush=True)
        g.close()


if __name__ == "__main__":
    main()
