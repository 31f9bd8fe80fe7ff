"""Host-clock time of Graph.pose_cross_covariances(ids_a, ids_b) — Sigma_ab of arbitrary pose pairs from the kept
Cholesky factor (k_inv_path_walk + k_inv_pair_blocks behind the build pass, the Schur complement and one factorisation
at lambda = 0) — with 1, 64 and 1024 random pairs on the kitti_00 shape and the 10k shape of bench.py: median of
--reps calls after a warm-up.  Each figure ends in a device synchronise (the call returns after its results are on the
host).  The time of compute_covariances(poses only) on the same graph, which queues the same system and then the
selected inverse, is printed next to it for scale.

    python tools/cross_cov_time.py [--reps 5] [--shapes kitti00,synth10k] [--pairs 1,64,1024]

For the per-kernel averages run it in a pass of its own under
`rocprofv3 --kernel-trace --stats -- python tools/cross_cov_time.py` (k_inv_path_walk, k_inv_pair_blocks)."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
cugo = importlib.import_module("cuda-bundle-adjustment_amd")

SHAPES = {  # (poses, landmarks, edges, seed, loop-closure landmarks, stereo fraction) as in bench.py
    "kitti00": (1322, 133383, 561116, 0, 4000, 0.7),
    "synth10k": (10000, 1000000, 5000000, 10000, 0, 0.0),
}


def median_ms(fn, reps):
    fn()  # warm-up: the first call allocates the workspace and uploads the parent list
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def time_shape(g, name, shape, s, a):
    P, L, E = shape
    base = median_ms(lambda: g.compute_covariances(poses=True, landmarks=False), a.reps)
    print("%-9s P=%d L=%d E=%d supernodes=%d stages=%d | compute_covariances(poses): median %.3f ms"
          % (name, P, L, E, s["supernodes"], s["stages"], base[0]), flush=True)
    rng = np.random.default_rng(1)
    for n in [int(x) for x in a.pairs.split(",")]:
        ia, ib = rng.integers(1, P, n).astype(np.int32), rng.integers(1, P, n).astype(np.int32)  # (pose 0 is fixed)
        rows = len(set(ia.tolist()) | set(ib.tolist()))
        med, lo, hi = median_ms(lambda: g.pose_cross_covariances(ia, ib), a.reps)
        print("%-9s   %5d pairs (%4d distinct rows, workspace %.1f MB): median %.3f ms (min %.3f, max %.3f, %d reps)"
              % (name, n, rows, rows * 288.0 * (P - 1) / 1e6, med, lo, hi, a.reps), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="kitti00,synth10k")
    ap.add_argument("--pairs", default="1,64,1024")
    a = ap.parse_args()
    for name in a.shapes.split(","):
        P, L, E, seed, lc, st = SHAPES[name]
        d = cugo.synth(P, L, E, seed=seed, n_loop_closures=lc, stereo_fraction=st)
        g = cugo.graph_from_arrays(d)
        g.initialize()
        g.optimize(10)
        g.optimize(10)  # (as tools/cov_time.py: the covariances of the estimates 20 iterations leave)
        s = g.structure_stats()
        try:
            time_shape(g, name, (P, L, E), s, a)
        except cugo.CugoError as e:  # (a zero pivot: H is singular at these estimates — nothing to time)
            print("%-9s not measured: %s" % (name, e), flush=True)
        g.close()


if __name__ == "__main__":
    main()
