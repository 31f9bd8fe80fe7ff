"""Times the LM loop with and without landmark position priors on the kitti_00-shaped BA graph of bench.py (1322 poses,
133 383 landmarks, 561 116 edges): one prior on every free landmark that an edge observes (dense 3 x 3 information,
measured a little off the initial landmark) against the same graph without.  `initialize(); optimize(--iters)` per run,
the two sides INTERLEAVED (--reps runs per side after --warmup), host-clock medians and ranges of optimize() per side,
the gap per iteration, and — with --kernels — the per-kernel HIP-event times of one more run of each side:
k_build_edges in both (the instantiation with the priors inside against the one without) and k_lm_prior_*.

The yardstick is the launch budget: nothing added to a build pass or a Schur pass, one launch
per error pass that is not taken from a build pass, one in a build pass whose chi2 is taken, one chi2 total per call.
A gap per iteration larger than those launches plus the difference of the two k_build_edges instantiations means a
launch, a copy or a synchronisation got into the loop."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

cugo = importlib.import_module("cuda-bundle-adjustment_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--kernels", action="store_true", help="per-kernel HIP-event times of one more run of each side")
    ap.add_argument("--weight", type=float, default=5.0,
                    help="scale of the priors' information; a small one (0.01) leaves the LM trajectory, and with it the "
                         "number of build and Schur passes, that of the graph without priors")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    d = cugo.synth(1322, 133383, 561116, seed=0, n_loop_closures=4000, stereo_fraction=0.7)
    ids = np.arange(len(d["pose"]), dtype=np.int32)
    lids = np.arange(len(d["lm"]), dtype=np.int32)
    active = ~((np.asarray(d["pose_fixed"])[d["e_pose"]] != 0) & (np.asarray(d["lm_fixed"])[d["e_lm"]] != 0))
    seen = np.zeros(len(d["lm"]), bool)
    seen[np.asarray(d["e_lm"])[active]] = True
    on = np.flatnonzero(seen & (np.asarray(d["lm_fixed"]) == 0)).astype(np.int32)
    z = d["lm"][on] + rng.normal(0, 0.02, (len(on), 3))
    A = rng.normal(size=(len(on), 3, 3))
    info = a.weight * (np.einsum("nij,nkj->nik", A, A) + 3 * np.eye(3))
    graphs = {}
    for side in ("ba", "lm_prior"):
        g = cugo.graph_from_arrays(d)
        if side == "lm_prior":
            g.add_landmark_priors(on, z, info)
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
        print("%s: edges %d (landmark priors %d); optimize(%d) median %.3f ms, range %.3f .. %.3f (%d runs); %d iterations, "
              "rejected trials %s, chi2 %.6g -> %.6g" %
              (side, g.n_active_edges(), g.n_landmark_prior_edges(), a.iters, med[side], t[0], t[-1], len(t), len(st),
               [s["trials"] for s in st], st[0]["chi2"], st[-1]["chi2"]))
    n_it = max(len(graphs["lm_prior"].stats()), 1)
    print("gap: %.1f us per optimize(), %.2f us per iteration" %
          (1e3 * (med["lm_prior"] - med["ba"]), 1e3 * (med["lm_prior"] - med["ba"]) / n_it))
    if a.kernels:
        for side, g in graphs.items():
            g.set_kernel_timing(1)
            g.set_poses(ids, d["pose"])
            g.set_landmarks(lids, d["lm"])
            g.initialize()
            g.optimize(a.iters)
            for name, k in sorted(g.kernel_times().items()):
                if k["launches"] and ("lm_prior" in name or name in ("k_build_edges", "build", "schur", "errors")):
                    print("  %-9s %-24s %4d launches  %9.2f us each (event pair: 1 - 2 us over the kernel)" %
                          (side, name, k["launches"], 1e3 * k["ms"] / k["launches"]))
    for g in graphs.values():
        g.close()


if __name__ == "__main__":
    main()
