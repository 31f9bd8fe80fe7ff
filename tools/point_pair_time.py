"""Times pose-pose point edge sets (PointPairEdgeSet, point_pair_kernels.hip) in the LM loop on a synthetic multi-scan graph
— --scans scans (default 8, the last one fixed), ALL pairs of them (28), --per-pair correspondences per pair (default
4096) from one cloud, no landmarks — and, as the nearest existing yardstick, the unary point kind (PointEdgeSet,
point_kernels.hip) on the same number of edges spread over the same free poses: half the outputs per edge (one block and
one b instead of three blocks and two).  A yardstick, not a target.

Per kind: host-clock median of `optimize(--iters)` over --reps runs on one optimiser after --warmup runs (initialize()
outside the clock; every run starts from the same estimates), then one more run with HIP-event pairs round every kernel:
the launches and the device time per launch of the kind's chunk passes (build, errors) and of its finishing passes.  An
event pair adds 1 - 2 us to the kernel it brackets."""
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
KERNELS = ("k_point_pair_chunks_build", "k_point_pair_chunks_errors", "k_point_pair_add", "k_point_pair_add_schur",
           "k_point_pair_offdiag", "k_point_chunks_build", "k_point_chunks_errors", "k_point_add", "k_point_add_schur")


def see(pose, X):
    """y = R(q) X + t, vectorised (the cross-product form)"""
    q = pose[:, :4]
    t1 = 2 * np.cross(q[:, :3], X)
    return X + q[:, 3:] * t1 + np.cross(q[:, :3], t1) + pose[:, 4:]


def scans(rng, S):
    gt = np.array([icp_ref.random_pose(rng, rot=0.3, trans=5.0) for _ in range(S)])
    pose = gt.copy()
    for i in range(S - 1):
        pose[i] = icp_ref.left_update(gt[i], np.concatenate([rng.normal(0, 0.05, 3), rng.normal(0, 0.3, 3)]))
    pf = np.zeros(S, np.uint8)
    pf[S - 1] = 1
    return PL.no_ba(pose, pf, gt)


def measure(a, d, kind, ia, ib, X, noise=0.03):
    rng = np.random.default_rng(1)
    E = len(ia)
    gt = d["pose_gt"]
    A = rng.normal(size=(E, 3, 3))
    info = np.einsum("eik,ejk->eij", A, A) + 3 * np.eye(3)[None]
    g = cugo.graph_from_arrays(d)
    if kind == "pair":
        g.add_point_pair_edges(ia, ib, see(gt[ia], X) + rng.normal(0, noise, (E, 3)), see(gt[ib], X) + rng.normal(0, noise, (E, 3)), info)
        g.set_point_pair_robust_kernel(cugo.RK_HUBER, 0.5)
    else:   # the same number of unary edges on the free ends
        free = np.where(np.asarray(d["pose_fixed"])[ib] == 0, ib, ia).astype(np.int32)
        g.add_point_edges(free, X, see(gt[free], X) + rng.normal(0, noise, (E, 3)), info)
        g.set_point_robust_kernel(cugo.RK_HUBER, 0.5)
    ids = np.arange(len(d["pose"]), dtype=np.int32)
    times = []
    for rep in range(a.warmup + a.reps + 1):
        timing = rep == a.warmup + a.reps
        if timing:
            g.set_kernel_timing(1)
        g.set_poses(ids, d["pose"])
        g.initialize()
        t0 = time.perf_counter()
        g.optimize(a.iters)
        if a.warmup <= rep and not timing:
            times.append(1e3 * (time.perf_counter() - t0))
    st = g.stats()
    times.sort()
    n_edges = g.n_point_pair_edges() if kind == "pair" else g.n_point_edges()
    print("%-5s pose edges %8d  optimize(%d) median %9.3f ms, range %.3f .. %.3f (%d runs); %d iterations, trials %s, chi2 %.6g -> %.6g"
          % (kind, n_edges, a.iters, times[len(times) // 2], times[0], times[-1], len(times), len(st), [s["trials"] for s in st],
             st[0]["chi2"], st[-1]["chi2"]))
    for kname, k in sorted(g.kernel_times().items()):
        if kname in KERNELS and k["launches"]:
            print("    %-28s %4d launches %10.2f us each" % (kname, k["launches"], 1e3 * k["ms"] / k["launches"]))
    g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=8)
    ap.add_argument("--per-pair", type=int, default=4096)
    ap.add_argument("--kinds", default="pair,point")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    d = scans(rng, a.scans)
    pairs = [(i, j) if (i + j) % 2 else (j, i) for i in range(a.scans) for j in range(i + 1, a.scans)]   # mixed orientation
    ia = np.repeat([p[0] for p in pairs], a.per_pair).astype(np.int32)
    ib = np.repeat([p[1] for p in pairs], a.per_pair).astype(np.int32)
    order = rng.permutation(len(ia))            # the container is not sorted by pair
    ia, ib = ia[order], ib[order]
    X = rng.normal(0, 3.0, (len(ia), 3))
    print("%d scans (one fixed), %d pairs x %d correspondences = %d edges, per-edge Omega, Huber 0.5" % (a.scans, len(pairs), a.per_pair, len(ia)))
    for kind in a.kinds.split(","):
        measure(a, d, kind, ia, ib, X)


if __name__ == "__main__":
    main()
