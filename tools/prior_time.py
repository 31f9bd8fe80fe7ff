"""Times the LM loop with and without SE(3) pose priors on the kitti_00-shaped BA graph of bench.py (1322 poses,
133 383 landmarks, 561 116 edges): one prior per free pose (dense 6 x 6 information, displaced from the initial pose)
against the same graph without.  `initialize(); optimize(--iters)` per run, the two sides INTERLEAVED (--reps runs per
side after --warmup), host-clock medians and ranges of optimize() per side, the gap per iteration, and — with
--kernels — the per-kernel HIP-event times of one more run of the side with priors.

The yardstick is the launch budget: one added launch per build pass (two-stream) or per Schur
pass (one-stream), one per error pass, one chi2 total per call.  A gap per iteration larger than those launches explain
means a launch, a copy or a synchronisation got into the loop."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import prior_ref  # noqa: E402

cugo = importlib.import_module("cuda-bundle-adjustment_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--kernels", action="store_true", help="per-kernel HIP-event times of one more run with priors")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    d = cugo.synth(1322, 133383, 561116, seed=0, n_loop_closures=4000, stereo_fraction=0.7)
    P = len(d["pose"])
    ids = np.arange(P, dtype=np.int32)
    lids = np.arange(len(d["lm"]), dtype=np.int32)
    free = np.nonzero(np.asarray(d["pose_fixed"]) == 0)[0].astype(np.int32)
    z = np.array([prior_ref.displaced(rng, d["pose"][p], 0.002, 0.02) for p in free])
    info = np.array([prior_ref.random_spd(rng, 10.0) for _ in free])
    graphs = {}
    for side in ("ba", "prior"):
        g = cugo.graph_from_arrays(d)
        if side == "prior":
            g.add_pose_priors(free, z, info)
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
    for side, g in graphs.items():
        st = g.stats()
        t = sorted(times[side])
        med[side] = t[len(t) // 2]
        print("%s: edges %d (priors %d); optimize(%d) median %.3f ms, range %.3f .. %.3f (%d runs); %d iterations, "
              "rejected trials %s, chi2 %.6g -> %.6g" %
              (side, g.n_active_edges(), g.n_prior_edges(), a.iters, med[side], t[0], t[-1], len(t), len(st),
               [s["trials"] for s in st], st[0]["chi2"], st[-1]["chi2"]))
    n_it = max(len(graphs["prior"].stats()), 1)
    print("gap: %.1f us per optimize(), %.2f us per iteration" %
          (1e3 * (med["prior"] - med["ba"]), 1e3 * (med["prior"] - med["ba"]) / n_it))
    if a.kernels:
        g = graphs["prior"]
        g.set_kernel_timing(1)
        g.set_poses(ids, d["pose"])
        g.set_landmarks(lids, d["lm"])
        g.initialize()
        g.optimize(a.iters)
        for name, k in sorted(g.kernel_times().items()):
            if k["launches"] and ("prior" in name or name in ("build", "schur", "errors")):
                print("  %-28s %4d launches  %9.2f us each (event pair: 1 - 2 us over the kernel)" %
                      (name, k["launches"], 1e3 * k["ms"] / k["launches"]))
    for g in graphs.values():
        g.close()


if __name__ == "__main__":
    main()
