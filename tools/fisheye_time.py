"""Times the LM loop with Kannala-Brandt fisheye cameras on the kitti_00-shaped BA graph of bench.py (1322 poses,
133 383 landmarks, 561 116 edges, here all of them MONO edges: a fisheye entry has no stereo row): the 4-camera rig of
tools/rig_time.py with pinhole cameras against the same rig with a Kannala-Brandt model on every camera (typical
coefficients, |k| of 1e-2 .. 1e-3).  Every measurement is moved by what the model moves its projection at the start
estimates, so both graphs start from the same residuals.  Both sides move the same bytes per edge (the model table is
136 bytes per CAMERA-TABLE ENTRY against 96, four entries here): the difference is atan2, the polynomials and the 2 x 3
block A of the fisheye term in k_errors, k_build_edges, k_pose_schur and k_backsubst_landmarks, and the 250 registers
of k_pose_schur<CamModelPar> against 212.

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

K = np.array([[-0.0131, 0.0212, -0.0071, 0.0012], [0.0342, -0.0094, 0.0038, -0.0009], [0.0, 0.0, 0.0, 0.0],
              [-0.0065, 0.0106, -0.0035, 0.0006]])


def project_kb(X, cam, k):
    r = np.hypot(X[:, 0], X[:, 1])
    th = np.arctan2(r, X[:, 2])
    t2 = th * th
    rho = th * (1 + t2 * (k[:, 0] + t2 * (k[:, 1] + t2 * (k[:, 2] + t2 * k[:, 3])))) / r
    return np.stack([cam[:, 0] * rho * X[:, 0] + cam[:, 2], cam[:, 1] * rho * X[:, 1] + cam[:, 3], np.zeros(len(X))], 1)


def graphs_of(d):
    """(pinhole rig, fisheye rig) of the mono graph `d`, landmark l on camera l % 4, the same residuals at the start"""
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
    model = np.concatenate([K[el % 4], np.ones((len(el), 1))], 1)
    out = {}
    for side, meas, mk in (("rig", res + RT.project(Xs, cam, no), None), ("fisheye", res + project_kb(Xs, cam, K[el % 4]), model)):
        g = cugo.Graph(True, True)
        g.add_poses(np.arange(len(d["pose"]), dtype=np.int32), d["pose"], d["pose_fixed"])
        g.add_landmarks(np.arange(len(d["lm"]), dtype=np.int32), d["lm"], d["lm_fixed"])
        g.add_edges(2, ep, el, meas, np.asarray(d["e_omega"]), cam, sensor=sens, model=mk)
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
        print("%s: edges %d, rig cameras %d, fisheye cameras %d; initialize() median %.3f ms; optimize(%d) median %.3f ms, "
              "range %.3f .. %.3f (%d runs); %d iterations, rejected trials %s, chi2 %.6g -> %.6g" %
              (side, g.n_active_edges(), g.n_rig_cameras(), g.n_fisheye_cameras(), ti[len(ti) // 2], a.iters, med[side], to[0],
               to[-1], len(to), len(st), [s["trials"] for s in st], st[0]["chi2"], st[-1]["chi2"]))
    print("fisheye - rig: %.1f us per optimize(), %.2f %%" %
          (1e3 * (med["fisheye"] - med["rig"]), 100.0 * (med["fisheye"] - med["rig"]) / med["rig"]))
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
