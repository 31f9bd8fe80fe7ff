"""Times the point-to-plane / point-to-line passes (cugo_icp_construct_quadratic_form, cugo_icp_compute_errors) on a
kitti_00-sized pose set (1322 poses) with about 2000 plane edges per pose (about 2.6 M edges) and a few line edges.

Run under `rocprofv3 --kernel-trace --stats -d OUT -o icp -- python tools/icp_time.py` for the per-kernel times; the
script prints the bytes each pass must read, so that the kernel_stats rows give the bandwidth.  Wall times per call
include the layout check before the launches (k_icp_check and one synchronisation), so read the kernel times from
the trace."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=1322)
    ap.add_argument("--planes-per-pose", type=int, default=2000)
    ap.add_argument("--lines-per-pose", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
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
