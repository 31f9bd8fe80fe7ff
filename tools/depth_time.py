"""Times the LM loop with depth edges on the kitti_00-shaped BA graph of bench.py (1322 poses, 133 383 landmarks,
561 116 edges): the graph as it is (mono + stereo) against the same graph with every stereo edge relabelled as a depth
edge (u, v, 1/Z).  The depth measurement is 1/Z of the generating geometry plus noise, read off the stereo measurement
the generator made from it: u - u_right = bf / Z with pixel noise on both, so m_d = (u - u_right) / bf has
sigma_d = sqrt(2) sigma_pixel / bf and the inverse-depth weight k = 1 / sigma_d^2 (at sigma_pixel = 1) puts the depth
residual on the scale of the pixel residuals.  The two kinds move the same bytes (same array, same records, same
blocks): the difference is the arithmetic of the third row in k_build_edges, k_pose_schur and k_backsubst_landmarks.

`initialize(); optimize(--iters)` per run, the two sides INTERLEAVED (--reps runs per side after --warmup), host-clock
medians and ranges of both calls per side, and — with --kernels — the per-kernel HIP-event times of one more run of each
side (the depth-aware instantiations against the ones the library has always run)."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

cugo = importlib.import_module("cuda-bundle-adjustment_amd")


def depth_graph(d):
    """the graph of `d` with its stereo edges as depth edges"""
    st = np.asarray(d["e_stereo"]).astype(bool)
    mono = dict(d)
    for key in ("e_pose", "e_lm", "e_stereo", "e_meas", "e_omega", "e_cam"):
        mono[key] = np.asarray(d[key])[~st]
    g = cugo.graph_from_arrays(mono)
    meas = np.asarray(d["e_meas"], np.float64)[st].copy()
    cam = np.asarray(d["e_cam"], np.float64).reshape(-1, 5)[st]
    meas[:, 2] = (meas[:, 0] - meas[:, 2]) / cam[:, 4]
    g.add_depth_edges(np.asarray(d["e_pose"])[st], np.asarray(d["e_lm"])[st], meas, np.asarray(d["e_omega"])[st], cam)
    g.set_depth_weight(float(np.median(cam[:, 4])) ** 2 / 2.0)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--kernels", action="store_true", help="per-kernel HIP-event times of one more run of each side")
    a = ap.parse_args()
    d = cugo.synth(1322, 133383, 561116, seed=0, n_loop_closures=4000, stereo_fraction=0.7)
    ids = np.arange(len(d["pose"]), dtype=np.int32)
    lids = np.arange(len(d["lm"]), dtype=np.int32)
    graphs = {"stereo": cugo.graph_from_arrays(d), "depth": depth_graph(d)}
    t_init = {side: [] for side in graphs}
    t_opt = {side: [] for side in graphs}
    for rep in range(a.warmup + a.reps):
        for side, g in graphs.items():
            g.set_poses(ids, d["pose"])
            g.set_landmarks(lids, d["lm"])
            t0 = time.perf_counter()
            g.initialize()
            t1 = time.perf_counter()
            g.optimize(a.iters)
            t2 = time.perf_counter()
            if rep >= a.warmup:
                t_init[side].append(1e3 * (t1 - t0))
                t_opt[side].append(1e3 * (t2 - t1))
    med = {}
    for side, g in graphs.items():
        st = g.stats()
        ti, to = sorted(t_init[side]), sorted(t_opt[side])
        med[side] = to[len(to) // 2]
        print("%s: edges %d; initialize() median %.3f ms; optimize(%d) median %.3f ms, range %.3f .. %.3f (%d runs); "
              "%d iterations, rejected trials %s, chi2 %.6g -> %.6g" %
              (side, g.n_active_edges(), ti[len(ti) // 2], a.iters, med[side], to[0], to[-1], len(to), len(st),
               [s["trials"] for s in st], st[0]["chi2"], st[-1]["chi2"]))
    print("depth - stereo: %.1f us per optimize(), %.2f %%" %
          (1e3 * (med["depth"] - med["stereo"]), 100.0 * (med["depth"] - med["stereo"]) / med["stereo"]))
    if a.kernels:
        for side, g in graphs.items():
            g.set_kernel_timing(1)
            g.set_poses(ids, d["pose"])
            g.set_landmarks(lids, d["lm"])
            g.initialize()
            g.optimize(a.iters)
            for name, k in sorted(g.kernel_times().items()):
                if k["launches"] and name in ("k_build_edges", "k_build_poses", "k_pose_schur", "k_backsubst_landmarks",
                                              "k_errors", "k_edge_chi", "build", "schur", "errors"):
                    print("  %-7s %-24s %4d launches  %9.2f us each (event pair: 1 - 2 us over the kernel)" %
                          (side, name, k["launches"], 1e3 * k["ms"] / k["launches"]))
    for g in graphs.values():
        g.close()


if __name__ == "__main__":
    main()
