"""Times what outlier rejection on pose edge sets (GraphOptimisationOptions::poseEdgeOutlierRejection, DESIGN.md section
15) adds to the END of optimize(): the same graph with a relative-pose threshold that rejects nothing (1e300) against
threshold 0, on
  pose:  the pure pose graph of tools/relpose_time.py — --poses poses (one fixed), a chain and loop closures to --edges
         relative-pose edges in mixed orientation — at KERNEL level (the graph object refuses it: see pose_graph_kernels);
  kitti: the kitti_00-shaped BA graph of tools/relpose_lm_time.py with its 1321 odometry edges.
`initialize(); optimize(--iters)` per run, the two sides INTERLEAVED (--reps runs per side after --warmup), host-clock
medians and ranges of optimize() per side and their gap; then one more run of the side with the threshold under HIP-event
timing for the per-launch times of the pass's kernels (k_relpose_errors with the per-edge terms, k_pose_reject_count /
_scan / _place).  The pass is one error launch, a memset, three launches and one 4-byte read-back per kind and call: a
gap beyond those means something else got behind the loop."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import prior_ref  # noqa: E402
import relpose_ref as RR  # noqa: E402
import synth  # noqa: E402

cugo = importlib.import_module("cuda-bundle-adjustment_amd")


def pose_graph_kernels(rng, P, E, a):
    """tools/relpose_time.py's chain + loop closures (the last pose fixed).  Its factor holds a front wider than the
    solver takes (a random graph of mean degree 10 has no small separators), so the graph object refuses it: what the end
    of optimize() would queue for it is timed at kernel level instead — the error pass with the per-edge terms and
    cugo_pose_edges_reject (three launches and the 4-byte read-back), against the error pass alone"""
    import devmem
    poses = np.zeros((P, 7))
    for i in range(P):
        q = synth.quat_from_rotvec(rng.normal(0, 0.5, 3))
        poses[i] = np.concatenate([q / np.linalg.norm(q), rng.normal(0, 2.0, 3)])
    chain = (np.stack([np.arange(P), (np.arange(P) + 1) % P], 1)[:P - 1] + P - 1) % P
    la = rng.integers(0, P, E - len(chain))
    lb = (la + rng.integers(2, P - 1, len(la))) % P
    pairs = np.concatenate([chain, np.stack([la, lb], 1)]).astype(np.int32)
    swap = rng.random(len(pairs)) < 0.5
    pairs[swap] = pairs[swap][:, ::-1]
    z = np.array([RR.measured(rng, poses[i], poses[j], 0.01, 0.05) for i, j in pairs])
    info = prior_ref.random_spd(rng)[None] * rng.uniform(0.5, 2.0, len(pairs))[:, None, None]
    rp = RR.make_edges(pairs[:, 0], pairs[:, 1], z, info, rk=(RR.RK_HUBER, 2.0))
    ctx = devmem.Ctx()
    rowptr, colind = cugo.relpose_pattern(P - 1, rp["a"], rp["b"])
    ev, pl = RR.upload(ctx, P, P - 1, rp, rowptr, colind)
    d_poses, d_chi, d_edge_chi = ctx.to_dev(poses), ctx.empty(2), ctx.empty(E)
    d_flags, d_list, d_thr = ctx.to_dev(np.zeros(E, np.uint8)), ctx.empty(E, np.int32), ctx.to_dev(np.array([1e300]))
    ev.d_flags = d_flags
    passes = {
        "errors with per-edge terms": lambda: cugo.relpose_compute_errors(ctx.h, ev, d_poses, d_chi, d_edge_chi),
        "the same + cugo_pose_edges_reject": lambda: (cugo.relpose_compute_errors(ctx.h, ev, d_poses, d_chi, d_edge_chi),
                                                      cugo.pose_edges_reject(ctx.h, E, d_edge_chi, d_thr, 1, d_flags, d_list)),
    }
    print("pose graph: %d poses, %d relative-pose edges (kernel level)" % (P, E))
    for what, call in passes.items():
        per_call = []
        for rep in range(a.warmup + a.reps):
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                call()
            ctx.sync()
            if rep >= a.warmup:
                per_call.append(1e6 * (time.perf_counter() - t0) / a.calls)
        per_call.sort()
        print("  %-36s %9.1f us per call (median of %d batches of %d calls; range %.1f .. %.1f)" %
              (what, per_call[len(per_call) // 2], a.reps, a.calls, per_call[0], per_call[-1]))
    pl.close()
    ctx.close()


def kitti_graph(rng):
    d = cugo.synth(1322, 133383, 561116, seed=0, n_loop_closures=4000, stereo_fraction=0.7)
    P = len(d["pose"])
    pairs = np.array([(i, i + 1) if i % 2 == 0 else (i + 1, i) for i in range(P - 1)], np.int32)
    z = np.array([RR.measured(rng, d["pose"][i], d["pose"][j], 0.002, 0.02) for i, j in pairs])
    info = np.array([prior_ref.random_spd(rng, 10.0) for _ in pairs])

    def make():
        g = cugo.graph_from_arrays(d)
        g.add_relpose_edges(pairs[:, 0], pairs[:, 1], z, info)
        return g
    return make, d


def measure(name, make, d, a):
    ids, lids = np.arange(len(d["pose"]), dtype=np.int32), np.arange(len(d["lm"]), dtype=np.int32)
    graphs = {}
    for side, t in (("threshold 0", 0.0), ("threshold 1e300", 1e300)):
        g = make()
        g.set_option("pose_edge_outliers", 1)
        g.set_relpose_outlier_threshold(t)
        graphs[side] = g
    times = {side: [] for side in graphs}

    def run(g):
        g.set_poses(ids, d["pose"])
        if len(lids):
            g.set_landmarks(lids, d["lm"])
        g.initialize()
        t0 = time.perf_counter()
        g.optimize(a.iters)
        return 1e3 * (time.perf_counter() - t0)
    for rep in range(a.warmup + a.reps):
        for side, g in graphs.items():
            t = run(g)
            if rep >= a.warmup:
                times[side].append(t)
    med = {}
    for side, g in graphs.items():
        t = sorted(times[side])
        med[side] = t[len(t) // 2]
        st = g.stats()
        print("%s, %s: %d relative-pose edges of %d; optimize(%d) median %.3f ms, range %.3f .. %.3f (%d runs); chi2 %.6g -> %.6g; "
              "outliers %d" % (name, side, g.n_relpose_edges(), g.n_active_edges(), a.iters, med[side], t[0], t[-1], len(t),
                               st[0]["chi2"], st[-1]["chi2"], g.n_pose_edge_outliers(cugo.POSE_KIND_RELPOSE)))
    print("%s: gap %.1f us per optimize() (medians; the side without a threshold ranges over %.1f us)" %
          (name, 1e3 * (med["threshold 1e300"] - med["threshold 0"]),
           1e3 * (max(times["threshold 0"]) - min(times["threshold 0"]))))
    g = graphs["threshold 1e300"]
    g.set_kernel_timing(1)
    run(g)
    for kname, k in sorted(g.kernel_times().items()):
        if k["launches"] and (kname.startswith("k_pose_reject") or kname in ("k_relpose_errors", "pose_outliers")):
            print("  %-24s %4d launches  %9.2f us each (event pair: 1 - 2 us over the kernel)" %
                  (kname, k["launches"], 1e3 * k["ms"] / k["launches"]))
    for g in graphs.values():
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--poses", type=int, default=10000)
    ap.add_argument("--edges", type=int, default=50000)
    ap.add_argument("--calls", type=int, default=50, help="calls per batch of the kernel-level timing")
    ap.add_argument("--graphs", default="pose,kitti")
    a = ap.parse_args()
    if cugo.device_count() == 0:
        sys.exit("no HIP device")
    rng = np.random.default_rng(0)
    if "pose" in a.graphs:
        pose_graph_kernels(rng, a.poses, a.edges, a)
    if "kitti" in a.graphs:
        measure("kitti_00 shape", *kitti_graph(rng), a)


if __name__ == "__main__":
    main()
