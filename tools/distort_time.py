"""Times the LM loop with radial-tangential lens distortion on the kitti_00-shaped BA graph of bench.py (1322 poses,
133 383 landmarks, 561 116 edges, here all of them MONO edges: a distorted entry has no stereo row): the 4-camera rig of
tools/rig_time.py with undistorted cameras against the same rig with a distortion (k1, k2, p1, p2, k3) on every camera
(coefficients as calibrations give them).  Every measurement is moved by what the distortion moves its projection at
the start estimates, so both graphs start from the same residuals.  Both sides move the same bytes per edge (the
distortion table is 144 bytes per CAMERA-TABLE ENTRY against 96, four entries here): the difference is the two
polynomials and the 2 x 3 block A of the distorted term in k_errors, k_build_edges, k_pose_schur and
k_backsubst_landmarks; there is no transcendental in it.

`initialize(); optimize(--iters)` per run, the two sides INTERLEAVED (--reps runs per side after --warmup), host-clock
medians and ranges per side, and — with --kernels — the per-kernel HIP-event times of one more run of each side."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import rig_time as RT  # noqa: E402

cugo = importlib.import_module("cuda-bundle-adjustment_amd")

D = np.array([[-0.28, 0.07, 0.002, -0.001, -0.01], [0.12, -0.21, -0.0007, 0.0013, 0.09], [-0.05, 0.01, 0.003, -0.002, 0.0],
              [-0.19, 0.04, -0.001, 0.0005, -0.004]])


def project_distorted(X, cam, d):
    a, b = X[:, 0] / X[:, 2], X[:, 1] / X[:, 2]
    r2 = a * a + b * b
    rad = 1 + r2 * (d[:, 0] + r2 * (d[:, 1] + r2 * d[:, 4]))
    ad = a * rad + 2 * d[:, 2] * a * b + d[:, 3] * (r2 + 2 * a * a)
    bd = b * rad + d[:, 2] * (r2 + 2 * b * b) + 2 * d[:, 3] * a * b
    return np.stack([cam[:, 0] * ad + cam[:, 2], cam[:, 1] * bd + cam[:, 3], np.zeros(len(X))], 1)


def graphs_of(d):
    """(undistorted rig, distorted rig) of the mono graph `d`, landmark l on camera l % 4, the same residuals at the start"""
    ep, el = np.asarray(d["e_pose"]), np.asarray(d["e_lm"])
    assert not np.asarray(d["e_stereo"]).any()
    no = np.zeros(len(ep), bool)
    cam = np.asarray(d["e_cam"], np.float64).reshape(-1, 5)
    sens = RT.SENSORS[el % 4]
    pose = np.asarray(d["pose"], np.float64)[ep]
    Xb = np.einsum("eij,ej->ei", RT.quat_R(pose[:, :4]), np.asarray(d["lm"], np.float64)[el]) + pose[:, 4:]
    Xs = np.einsum("eij,ej->ei", RT.quat_R(sens[:, :4]), Xb) + sens[:, 4:]
    assert np.all(Xs[:, 2] > 0.5 * Xb[:, 2]), "a landmark leaves the view of its rig camera"
    res = np.asarray(d["e_meas"], np.float64) - RT.project(Xb, cam, no)       # (minus) the residuals of the plain graph
    out = {}
    for side, meas, dk in (("rig", res + RT.project(Xs, cam, no), None), ("distorted", res + project_distorted(Xs, cam, D[el % 4]), D[el % 4])):
        g = cugo.Graph(True, True)
        g.add_poses(np.arange(len(d["pose"]), dtype=np.int32), d["pose"], d["pose_fixed"])
        g.add_landmarks(np.arange(len(d["lm"]), dtype=np.int32), d["lm"], d["lm_fixed"])
        g.add_edges(2, ep, el, meas, np.asarray(d["e_omega"]), cam, sensor=sens, distortion=dk)
        out[side] = g
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--kernels", action="store_true", help="per-kernel HIP-event times of one more run of each side")
    a = ap.parse_args()
    d = cugo.synth(1322, 133383, 561116, seed=0, n_loop_closures=4000, stereo_fraction=0.0)
    ids = np.arange(len(d["pose"]), dtype=np.int32)
    lids = np.arange(len(d["lm"]), dtype=np.int32)
    graphs = graphs_of(d)
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
        print("%s: edges %d, rig cameras %d, distorted cameras %d; initialize() median %.3f ms; optimize(%d) median %.3f ms, "
              "range %.3f .. %.3f (%d runs); %d iterations, rejected trials %s, chi2 %.6g -> %.6g" %
              (side, g.n_active_edges(), g.n_rig_cameras(), g.n_distorted_cameras(), ti[len(ti) // 2], a.iters, med[side], to[0],
               to[-1], len(to), len(st), [s["trials"] for s in st], st[0]["chi2"], st[-1]["chi2"]))
    print("distorted - rig: %.1f us per optimize(), %.2f %%" %
          (1e3 * (med["distorted"] - med["rig"]), 100.0 * (med["distorted"] - med["rig"]) / med["rig"]))
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
                    print("  %-9s %-24s %4d launches  %9.2f us each (event pair: 1 - 2 us over the kernel)" %
                          (side, name, k["launches"], 1e3 * k["ms"] / k["launches"]))
    for g in graphs.values():
        g.close()


if __name__ == "__main__":
    main()
