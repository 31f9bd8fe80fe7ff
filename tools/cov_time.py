"""Host-clock time of Graph.compute_covariances(poses=True, landmarks=True) — the marginal covariances (selected
inverse of the Schur complement's factorisation + landmark blocks) — on the kitti_00 shape and the 10k shape of
bench.py, after warm-up.  Each figure ends in a device synchronise (the call returns after its results are on the
host).  The optimize() time of the same graph is printed next to it for scale.

    python tools/cov_time.py [--reps 5] [--shapes kitti00,synth10k]

For the per-kernel figures run it under `rocprofv3 --kernel-trace --stats -- python tools/cov_time.py`."""
import argparse
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
cugo = importlib.import_module("cuda-bundle-adjustment_amd")

SHAPES = {  # (poses, landmarks, edges, seed, loop-closure landmarks, stereo fraction) as in bench.py
    "kitti00": (1322, 133383, 561116, 0, 4000, 0.7),
    "synth10k": (10000, 1000000, 5000000, 10000, 0, 0.0),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="kitti00,synth10k")
    a = ap.parse_args()
    for name in a.shapes.split(","):
        P, L, E, seed, lc, st = SHAPES[name]
        d = cugo.synth(P, L, E, seed=seed, n_loop_closures=lc, stereo_fraction=st)
        g = cugo.graph_from_arrays(d)
        g.initialize()
        g.optimize(10)
        t = time.perf_counter()
        g.optimize(10)
        t_opt = (time.perf_counter() - t) * 1e3
        g.compute_covariances()  # warm-up: the first call allocates the Sigma-fronts and builds the tile lists
        ms = []
        for _ in range(a.reps):
            t = time.perf_counter()
            g.compute_covariances()
            ms.append((time.perf_counter() - t) * 1e3)
        ms.sort()
        s = g.structure_stats()
        print("%-9s P=%d L=%d E=%d supernodes=%d stages=%d chol_gflop=%.2f | compute_covariances(3): median %.3f ms "
              "(min %.3f, max %.3f, %d reps) | optimize(10): %.3f ms"
              % (name, P, L, E, s["supernodes"], s["stages"], s["chol_flops"] / 1e9, ms[len(ms) // 2], ms[0], ms[-1],
                 len(ms), t_opt), flush=True)
        g.close()


if __name__ == "__main__":
    main()
