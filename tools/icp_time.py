"""Times the point-to-plane / point-to-line passes (cugo_icp_construct_quadratic_form, cugo_icp_compute_errors) on a
kitti_00-sized pose set (1322 poses) with about 2000 plane edges per pose (about 2.6 M edges) and a few line edges.

Run under `rocprofv3 --kernel-trace --stats -d OUT -o icp -- python tools/icp_time.py` for the per-kernel times; the
script prints the bytes each pass must read, so that the kernel_stats rows give the bandwidth.  Wall times per call
include the layout check before the launches (k_icp_check and one synchronisation), so read the kernel times from
the trace.

`--graph`: the LM loop instead — the kitti_00-shaped BA graph of bench.py (1322 poses, 133 383 landmarks, 561 116 edges)
with and without the same ICP load added as plane / line edge sets, `initialize(); optimize(--iters)` repeated --reps
times on one optimiser: host-clock medians of optimize() per side and the kernel launches of the side with ICP sets
(`--graph --only icp` / `--only ba` under rocprofv3 for the per-kernel averages of one side)."""
import argparse
import ctypes as C
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import devmem  # noqa: E402
import icp_ref  # noqa: E402

cugo = importlib.import_module("cuda-bundle-adjustment_amd")


def graph_mode(a):
    """step time of the LM loop with and without ICP edge sets on the kitti_00-shaped graph"""
    rng = np.random.default_rng(0)
    d = cugo.synth(1322, 133383, 561116, seed=0, n_loop_closures=4000, stereo_fraction=0.7)
    P = len(d["pose"])
    sets = {}
    for kind, per in (("plane", a.planes_per_pose), ("line", a.lines_per_pose)):
        sets[kind] = icp_ref.make_edges(rng, np.repeat(np.arange(P, dtype=np.int32), per), kind, d["pose"], noise=0.05)
    ids = np.arange(P, dtype=np.int32)
    for side in ("ba", "icp"):
        if a.only and a.only != side:
            continue
        g = cugo.graph_from_arrays(d)
        if side == "icp":
            pl, li = sets["plane"], sets["line"]
            g.set_icp_robust_kernel(cugo.ICP_PLANE, icp_ref.RK_HUBER, 0.1)
            g.set_icp_robust_kernel(cugo.ICP_LINE, icp_ref.RK_HUBER, 0.1)
            g.add_plane_edges(pl["pose"], pl["p"], pl["n"], pl["d"], np.ones(len(pl["pose"])))
            g.add_line_edges(li["pose"], li["p"], li["a"], li["b"], np.ones(len(li["pose"])))
        times = []
        for rep in range(a.warmup + a.reps):
            g.set_poses(ids, d["pose"])
            g.set_landmarks(np.arange(len(d["lm"]), dtype=np.int32), d["lm"])
            g.initialize()
            t0 = time.perf_counter()
            g.optimize(a.iters)
            if rep >= a.warmup:
                times.append(1e3 * (time.perf_counter() - t0))
        st = g.stats()
        times.sort()
        print("%s: edges %d (plane %d, line %d); optimize(%d) median %.3f ms, range %.3f .. %.3f (%d runs); %d iterations, "
              "rejected trials %s, chi2 %.6g -> %.6g" %
              (side, g.n_active_edges(), g.n_icp_edges(0), g.n_icp_edges(1), a.iters, times[len(times) // 2], times[0],
               times[-1], len(times), len(st), [s["trials"] for s in st], st[0]["chi2"], st[-1]["chi2"]))
        if a.kernels:
            g.set_kernel_timing(1)
            g.set_poses(ids, d["pose"])
            g.set_landmarks(np.arange(len(d["lm"]), dtype=np.int32), d["lm"])
            g.initialize()
            g.optimize(a.iters)
            for name, k in sorted(g.kernel_times().items()):
                if k["launches"]:
                    print("  %-28s %4d launches  %9.2f us each (event pair: 1 - 2 us over the kernel)" %
                          (name, k["launches"], 1e3 * k["ms"] / k["launches"]))
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", action="store_true", help="the LM loop with and without ICP edge sets")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=["ba", "icp"], default=None)
    ap.add_argument("--kernels", action="store_true", help="graph mode: per-kernel HIP-event times of one more run")
    ap.add_argument("--poses", type=int, default=1322)
    ap.add_argument("--planes-per-pose", type=int, default=2000)
    ap.add_argument("--lines-per-pose", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if a.graph:
        return graph_mode(a)
    rng = np.random.default_rng(0)
    P = a.poses
    poses = np.array([icp_ref.random_pose(rng, rot=0.3, trans=50.0) for _ in range(P)])
    case = {}
    for kind, per in (("plane", a.planes_per_pose), ("line", a.lines_per_pose)):
        e = icp_ref.make_edges(rng, np.repeat(np.arange(P, dtype=np.int32), per), kind, poses, noise=0.05)
        e["omega"] = np.array([1.0])
        e["rk"] = (icp_ref.RK_HUBER, 0.1)
        case[kind] = e
    ctx = devmem.Ctx()
    ev = icp_ref.upload(ctx, P, P - 1, plane=case["plane"], line=case["line"])
    d_poses = ctx.to_dev(poses)
    d_H, d_b, d_chi = ctx.empty(36 * P), ctx.empty(6 * P), ctx.empty(2)
    npl, nli = len(case["plane"]["pose"]), len(case["line"]["pose"])
    # bytes the passes must read: pose index, pointP, geometry (plane n, d / line a, u); omega is one per set
    read = npl * (4 + 24 + 32) + nli * (4 + 24 + 48)
    print("edges plane %d line %d; bytes read per pass %.1f MB" % (npl, nli, read / 1e6))
    L = cugo.lib()
    for name, call in (("build", lambda: L.cugo_icp_construct_quadratic_form(ctx.h, C.byref(ev), d_poses, d_H, d_b,
                                                                             d_chi)),
                       ("errors", lambda: L.cugo_icp_compute_errors(ctx.h, C.byref(ev), d_poses, d_chi, None))):
        cugo.check(call())
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            cugo.check(call())
        ctx.sync()
        print("%s: %.3f ms per call (wall, incl. the layout check)" % (name, 1e3 * (time.perf_counter() - t0) / a.reps))
    print("chi2", ctx.to_host(d_chi, 1)[0])
    ctx.close()


if __name__ == "__main__":
    main()
