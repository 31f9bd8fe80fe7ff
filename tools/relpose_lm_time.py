"""Times the LM loop with and without relative-pose SE(3) edges on the kitti_00-shaped BA graph of bench.py (1322 poses,
133 383 landmarks, 561 116 edges): one odometry edge per consecutive pose pair plus --closures loop closures between
random poses (dense 6 x 6 information, measured at the initial poses with a little noise) against the same graph
without.  `initialize(); optimize(--iters)` per run, the two sides INTERLEAVED (--reps runs per side after --warmup),
host-clock medians and ranges of optimize() per side, the gap per iteration, how much the pairs grow the Hsc pattern and
the factor (structure_stats), and — with --kernels — the per-kernel HIP-event times of one more run of the side with
the edges.

The yardstick is the launch budget: one added launch per build pass, one per Schur pass, one per
error pass, one chi2 total per call.  A gap per iteration larger than those launches explain means a launch, a copy or a
synchronisation got into the loop.  Odometry pairs are co-visible anyway: they should add no block."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import prior_ref  # noqa: E402
import relpose_ref  # noqa: E402

cugo = importlib.import_module("cuda-bundle-adjustment_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--closures", type=int, default=20)
    ap.add_argument("--kernels", action="store_true", help="per-kernel HIP-event times of one more run with the edges")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    d = cugo.synth(1322, 133383, 561116, seed=0, n_loop_closures=4000, stereo_fraction=0.7)
    P = len(d["pose"])
    ids = np.arange(P, dtype=np.int32)
    lids = np.arange(len(d["lm"]), dtype=np.int32)
    pairs = [(i, i + 1) if i % 2 == 0 else (i + 1, i) for i in range(P - 1)]
    n_odo = len(pairs)
    while len(pairs) < n_odo + a.closures:
        i, j = (int(x) for x in rng.choice(P, 2, replace=False))
        if abs(i - j) > 50:
            pairs.append((i, j))
    pairs = np.array(pairs, np.int32)
    z = np.array([relpose_ref.measured(rng, d["pose"][i], d["pose"][j], 0.002, 0.02) for i, j in pairs])
    info = np.array([prior_ref.random_spd(rng, 10.0) for _ in pairs])
    sets = {"ba": 0, "odometry": n_odo, "odometry+closures": len(pairs)}
    graphs = {}
    for side, n in sets.items():
        g = cugo.graph_from_arrays(d)
        if n:
            g.add_relpose_edges(pairs[:n, 0], pairs[:n, 1], z[:n], info[:n])
        graphs[side] = g
    times = {side: [] for side in graphs}
    for rep in range(a.warmup + a.reps):
        for side, g in graphs.items():
            g.set_poses(ids, d["pose"])
            g.set_landmarks(lids, d["lm"])
            g.initialize()
            t0 = time.perf_counter()
            g.optimize(a.iters)
            if rep >= a.warmup:
                times[side].append(1e3 * (time.perf_counter() - t0))
    med = {}
    base = graphs["ba"].structure_stats()
    for side, g in graphs.items():
        st, ss = g.stats(), g.structure_stats()
        t = sorted(times[side])
        med[side] = t[len(t) // 2]
        print("%s: edges %d (relative-pose %d); optimize(%d) median %.3f ms, range %.3f .. %.3f (%d runs); %d iterations, "
              "rejected trials %s, chi2 %.6g -> %.6g" %
              (side, g.n_active_edges(), g.n_relpose_edges(), a.iters, med[side], t[0], t[-1], len(t), len(st),
               [s["trials"] for s in st], st[0]["chi2"], st[-1]["chi2"]))
        print("  hsc_blocks %d (%+d), nnzL %d (%+d), chol_flops %.4g (%+.3g %%)" %
              (ss["hsc_blocks"], ss["hsc_blocks"] - base["hsc_blocks"], ss["nnzL"], ss["nnzL"] - base["nnzL"],
               ss["chol_flops"], 100.0 * (ss["chol_flops"] / base["chol_flops"] - 1.0)))
    for side in list(sets)[1:]:
        n_it = max(len(graphs[side].stats()), 1)
        print("gap %s - ba: %.1f us per optimize(), %.2f us per iteration" %
              (side, 1e3 * (med[side] - med["ba"]), 1e3 * (med[side] - med["ba"]) / n_it))
    if a.kernels:
        g = graphs["odometry+closures"]
        g.set_kernel_timing(1)
        g.set_poses(ids, d["pose"])
        g.set_landmarks(lids, d["lm"])
        g.initialize()
        g.optimize(a.iters)
        for name, k in sorted(g.kernel_times().items()):
            if k["launches"] and ("relpose" in name or name in ("build", "schur", "errors", "cholesky")):
                print("  %-28s %4d launches  %9.2f us each (event pair: 1 - 2 us over the kernel)" %
                      (name, k["launches"], 1e3 * k["ms"] / k["launches"]))
    for g in graphs.values():
        g.close()


if __name__ == "__main__":
    main()
