"""Times point-to-point edge sets (PointEdgeSet, point_kernels.hip) in the LM loop, and for scale the same correspondences
as plane edges (one per correspondence) and as three axis-plane edges each (what a caller had to use before):

  one     one free pose x 100 000 correspondences, no landmarks
  many    1 000 free poses x 500 correspondences, no landmarks
  kitti   the `many` load on the first 1 000 poses of the kitti_00-shaped BA graph of bench.py (1322 poses, 133 383
          landmarks, 561 116 edges), next to the BA graph alone

Per shape and edge kind: host-clock median of `optimize(--iters)` over --reps runs on one optimiser (initialize() outside
the clock), then one more run with HIP-event pairs round every kernel: the launches and the time per launch of the chunk
passes and the finishing pass, and the bytes per second of the chunk passes against the streams they read (pose index 4 B,
p 24 B, z 24 B, Omega 48 B per edge with per-edge matrices: 100 B per edge; 52 B with one matrix for all).  An event pair
adds 1 - 2 us to the kernel it brackets."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import icp_ref  # noqa: E402
import point_lm_ref as PL  # noqa: E402

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
KERNELS = ("k_point_chunks_build", "k_point_chunks_errors", "k_point_add", "k_point_add_schur", "k_icp_chunks_build",
           "k_icp_chunks_errors", "k_icp_add", "k_icp_add_schur")


def pose_graph(rng, P):
    gt = np.array([icp_ref.random_pose(rng, rot=0.3, trans=20.0) for _ in range(P + 1)])
    pose = gt.copy()
    for i in range(P):
        pose[i] = icp_ref.left_update(gt[i], np.concatenate([rng.normal(0, 0.05, 3), rng.normal(0, 0.3, 3)]))
    pf = np.zeros(P + 1, np.uint8)
    pf[P] = 1
    return PL.no_ba(pose, pf, gt)


def correspondences(rng, gt, pose_of_edge, noise=0.03):
    E = len(pose_of_edge)
    p = rng.normal(0, 3.0, (E, 3))
    q = gt[pose_of_edge, :4]
    # y = R(q) p + t, vectorised (the cross-product form)
    t1 = 2 * np.cross(q[:, :3], p)
    y = p + q[:, 3:] * t1 + np.cross(q[:, :3], t1) + gt[pose_of_edge, 4:]
    return p, y + rng.normal(0, noise, (E, 3))


def add_kind(g, kind, pe, p, z, rng, per_edge_info):
    E = len(pe)
    if kind == "point":
        if per_edge_info:
            A = rng.normal(size=(E, 3, 3))
            info = np.einsum("eik,ejk->eij", A, A) + 3 * np.eye(3)[None]
        else:
            info = np.eye(3)[None]
        g.add_point_edges(pe, p, z, np.broadcast_to(info, (E, 3, 3)))
        g.set_point_robust_kernel(cugo.RK_HUBER, 0.5)
        return 100 if per_edge_info else 52
    w = rng.uniform(0.5, 2.0, E) if per_edge_info else np.ones(E)
    if kind == "plane":       # one plane per correspondence: a random unit normal through z
        n = rng.normal(size=(E, 3))
        n /= np.linalg.norm(n, axis=1)[:, None]
        g.add_plane_edges(pe, p, n, (n * z).sum(1), w)
    else:                     # plane3: three axis planes per correspondence
        g.add_plane_edges(np.repeat(pe, 3), np.repeat(p, 3, axis=0), np.tile(np.eye(3), (E, 1)), z.reshape(-1), np.repeat(w, 3))
    g.set_icp_robust_kernel(cugo.ICP_PLANE, cugo.RK_HUBER, 0.5)
    return 4 + 24 + 32 + (8 if per_edge_info else 0)


def measure(a, name, d, kind, pe, p, z):
    rng = np.random.default_rng(1)
    g = cugo.graph_from_arrays(d)
    bytes_per_edge = add_kind(g, kind, pe, p, z, rng, a.per_edge_info) if kind != "ba" else 0
    ids, lids = np.arange(len(d["pose"]), dtype=np.int32), np.arange(len(d["lm"]), dtype=np.int32)
    times = []
    for rep in range(a.warmup + a.reps + 1):
        timing = rep == a.warmup + a.reps
        if timing:
            g.set_kernel_timing(1)
        g.set_poses(ids, d["pose"])
        if len(lids):
            g.set_landmarks(lids, d["lm"])
        g.initialize()
        t0 = time.perf_counter()
        g.optimize(a.iters)
        if a.warmup <= rep and not timing:
            times.append(1e3 * (time.perf_counter() - t0))
    st = g.stats()
    times.sort()
    n_edges = g.n_point_edges() if kind == "point" else g.n_icp_edges(cugo.ICP_PLANE) if kind != "ba" else 0
    print("%-6s %-6s pose edges %8d  optimize(%d) median %9.3f ms, range %.3f .. %.3f (%d runs); %d iterations, trials %s, chi2 %.6g -> %.6g"
          % (name, kind, n_edges, a.iters, times[len(times) // 2], times[0], times[-1], len(times), len(st),
             [s["trials"] for s in st], st[0]["chi2"], st[-1]["chi2"]))
    for kname, k in sorted(g.kernel_times().items()):
        if kname in KERNELS and k["launches"]:
            us = 1e3 * k["ms"] / k["launches"]
            bw = "  %7.1f GB/s of the %d B per edge it reads" % (n_edges * bytes_per_edge / (us * 1e3), bytes_per_edge) if "chunks" in kname else ""
            print("    %-24s %4d launches %10.2f us each%s" % (kname, k["launches"], us, bw))
    g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="one,many,kitti")
    ap.add_argument("--kinds", default="point,plane,plane3")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shared-info", dest="per_edge_info", action="store_false", help="one Omega / omega for all edges")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    for shape in a.shapes.split(","):
        if shape == "one":
            d = pose_graph(rng, 1)
            pe = np.zeros(100000, np.int32)
        elif shape == "many":
            d = pose_graph(rng, 1000)
            pe = np.repeat(np.arange(1000, dtype=np.int32), 500)
        else:
            d = cugo.synth(1322, 133383, 561116, seed=0, n_loop_closures=4000, stereo_fraction=0.7)
            free = np.flatnonzero(np.asarray(d["pose_fixed"]) == 0)[:1000].astype(np.int32)
            pe = np.repeat(free, 500)
        p, z = correspondences(rng, d.get("pose_gt", d["pose"]), pe)
        for kind in (["ba"] if shape == "kitti" else []) + a.kinds.split(","):
            measure(a, shape, d, kind, pe, p, z)


if __name__ == "__main__":
    main()
