"""Times the LM loop with camera extrinsics on the kitti_00-shaped BA graph of bench.py (1322 poses, 133 383 landmarks,
561 116 edges): the graph as it is against the same graph with its edges relabelled onto a 4-camera rig — landmark l is
seen by camera l % 4, whose sensor pose (body -> sensor) is a rotation of 6 to 11 degrees about a general axis with a
lever arm of 0.3 to 0.5 m.  Every measurement is moved by what the sensor pose moves its projection at the start
estimates, so both graphs start from the same residuals.  The two graphs move the same bytes per edge (the rig adds 96
bytes per CAMERA-TABLE ENTRY, four entries here): the difference is the arithmetic of Xs = M Xb + t_s and B = A M in
k_errors, k_build_edges, k_pose_schur and k_backsubst_landmarks, and the occupancy of the rig-aware k_pose_schur (two
waves per SIMD instead of three).

`initialize(); optimize(--iters)` per run, the two sides INTERLEAVED (--reps runs per side after --warmup), host-clock
medians and ranges of both calls per side, and — with --kernels — the per-kernel HIP-event times of one more run of each
side (the rig-aware instantiations against the ones the library has always run)."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

cugo = importlib.import_module("cuda-bundle-adjustment_amd")


def axis_angle(axis, deg, t):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    h = np.deg2rad(deg) / 2
    return np.concatenate([np.sin(h) * a, [np.cos(h)], t])


SENSORS = np.stack([axis_angle((1, 2, -1), 8.0, (0.4, -0.1, 0.2)), axis_angle((-2, 1, 3), 11.0, (-0.3, 0.25, -0.3)),
                    axis_angle((1, -1, 1), 6.0, (0.1, 0.45, 0.15)), axis_angle((3, 1, 1), 9.0, (-0.35, -0.3, 0.1))])


def quat_R(q):
    x, y, z, w = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


def project(X, cam, stereo):
    iz = 1.0 / X[:, 2]
    u = cam[:, 0] * X[:, 0] * iz + cam[:, 2]
    return np.stack([u, cam[:, 1] * X[:, 1] * iz + cam[:, 3], np.where(stereo, u - cam[:, 4] * iz, 0.0)], 1)


def rig_graph(d):
    """the graph of `d` with landmark l on camera l % 4 of the rig"""
    ep, el = np.asarray(d["e_pose"]), np.asarray(d["e_lm"])
    st = np.asarray(d["e_stereo"]).astype(bool)
    cam = np.asarray(d["e_cam"], np.float64).reshape(-1, 5)
    sens = SENSORS[el % 4]
    pose = np.asarray(d["pose"], np.float64)[ep]
    Xb = np.einsum("eij,ej->ei", quat_R(pose[:, :4]), np.asarray(d["lm"], np.float64)[el]) + pose[:, 4:]
    Xs = np.einsum("eij,ej->ei", quat_R(sens[:, :4]), Xb) + sens[:, 4:]
    assert np.all(Xs[:, 2] > 0.5 * Xb[:, 2]), "a landmark leaves the view of its rig camera"
    meas = np.asarray(d["e_meas"], np.float64) + project(Xs, cam, st) - project(Xb, cam, st)
    g = cugo.Graph(True, True)
    g.add_poses(np.arange(len(d["pose"]), dtype=np.int32), d["pose"], d["pose_fixed"])
    g.add_landmarks(np.arange(len(d["lm"]), dtype=np.int32), d["lm"], d["lm_fixed"])
    for dim, sel in ((2, ~st), (3, st)):
        g.add_edges(dim, ep[sel], el[sel], meas[sel], np.asarray(d["e_omega"])[sel], cam[sel], sensor=sens[sel])
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
    graphs = {"plain": cugo.graph_from_arrays(d), "rig": rig_graph(d)}
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
        print("%s: edges %d, rig cameras %d; initialize() median %.3f ms; optimize(%d) median %.3f ms, range %.3f .. %.3f "
              "(%d runs); %d iterations, rejected trials %s, chi2 %.6g -> %.6g" %
              (side, g.n_active_edges(), g.n_rig_cameras(), ti[len(ti) // 2], a.iters, med[side], to[0], to[-1], len(to),
               len(st), [s["trials"] for s in st], st[0]["chi2"], st[-1]["chi2"]))
    print("rig - plain: %.1f us per optimize(), %.2f %%" %
          (1e3 * (med["rig"] - med["plain"]), 100.0 * (med["rig"] - med["plain"]) / med["plain"]))
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
