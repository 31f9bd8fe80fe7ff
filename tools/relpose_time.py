"""Times the kernel-level passes of the relative-pose SE(3) edges (cugo_relpose_construct_quadratic_form_schur,
cugo_relpose_compute_errors) on two pose graphs:
  chain: 10 000 poses (pose 0 fixed), a chain i -> i+1 and loop closures to 50 000 edges in mixed orientation;
  hub:   2 001 poses, one hub pose joined to every other by one edge (2 000 edges): ONE wave walks 2 000 edges.
Per graph and pass: --calls calls queued back to back on the context's stream, then one synchronisation; host clock per
call, the median and the range over --reps such batches after --warmup.  A call is the pass's one launch plus the chi2
total's.  The hub figure is what says whether a serial walk per pose is enough for the engine."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import devmem  # noqa: E402
import prior_ref  # noqa: E402
import relpose_ref as RR  # noqa: E402
import synth  # noqa: E402

cugo = importlib.import_module("cuda-bundle-adjustment_amd")


def graph(rng, P, pairs):
    """P poses (index P - 1 fixed: free-first order), noisy measurements of the pairs, one dense Omega per edge"""
    poses = np.zeros((P, 7))
    for i in range(P):
        q = synth.quat_from_rotvec(rng.normal(0, 0.5, 3))
        poses[i] = np.concatenate([q / np.linalg.norm(q), rng.normal(0, 2.0, 3)])
    z = np.array([RR.measured(rng, poses[a], poses[b], 0.01, 0.05) for a, b in pairs])
    base = prior_ref.random_spd(rng)
    info = base[None] * rng.uniform(0.5, 2.0, len(pairs))[:, None, None]
    return poses, RR.make_edges(pairs[:, 0], pairs[:, 1], z, info, rk=(RR.RK_HUBER, 2.0))


def time_graph(ctx, name, poses, rp, a):
    P = len(poses) - 1
    rowptr, colind = cugo.relpose_pattern(P, rp["a"], rp["b"])
    ev, pl = RR.upload(ctx, P + 1, P, rp, rowptr, colind)
    nnzb = len(colind)
    d_poses, d_rowptr = ctx.to_dev(poses), ctx.to_dev(rowptr)
    d_Hsc, d_bp, d_bsc, d_chi = ctx.empty(36 * nnzb), ctx.empty(6 * P), ctx.empty(6 * P), ctx.empty(2)
    deg = np.diff(pl.array("inc_ptr"))
    print("%s: %d poses (%d free), %d edges, %d blocks; incident edges per pose: max %d, mean %.1f" %
          (name, P + 1, P, len(rp["a"]), nnzb, deg.max(), deg.mean()))
    passes = {
        "build (Schur form)": lambda: cugo.relpose_construct_quadratic_form_schur(ctx.h, ev, d_poses, d_rowptr, d_Hsc,
                                                                                  d_bp, d_bsc, d_chi),
        "errors": lambda: cugo.relpose_compute_errors(ctx.h, ev, d_poses, d_chi),
    }
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
        print("  %-20s %9.1f us per call (median of %d batches of %d calls; range %.1f .. %.1f)" %
              (what, per_call[len(per_call) // 2], a.reps, a.calls, per_call[0], per_call[-1]))
    print("  chi2 %.6g" % ctx.to_host(d_chi, 1)[0])
    pl.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--poses", type=int, default=10000)
    ap.add_argument("--edges", type=int, default=50000)
    ap.add_argument("--hub", type=int, default=2000)
    a = ap.parse_args()
    if cugo.device_count() == 0:
        sys.exit("no HIP device")
    rng = np.random.default_rng(0)
    ctx = devmem.Ctx()
    # chain + loop closures; the fixed pose (the chain's first) is index P - 1 in the free-first order
    P = a.poses
    chain = np.stack([np.arange(P), (np.arange(P) + 1) % P], 1)[:P - 1]
    chain = (chain + P - 1) % P  # pose 0 of the chain -> index P - 1
    n_loops = a.edges - len(chain)
    la = rng.integers(0, P, n_loops)
    lb = (la + rng.integers(2, P - 1, n_loops)) % P
    pairs = np.concatenate([chain, np.stack([la, lb], 1)]).astype(np.int32)
    swap = rng.random(len(pairs)) < 0.5
    pairs[swap] = pairs[swap][:, ::-1]
    time_graph(ctx, "chain + loop closures", *graph(rng, P, pairs), a)
    # hub: pose 0 joined to every other pose, the last pose fixed
    H = a.hub
    pairs = np.stack([np.zeros(H, int), np.arange(1, H + 1)], 1).astype(np.int32)
    swap = rng.random(H) < 0.5
    pairs[swap] = pairs[swap][:, ::-1]
    time_graph(ctx, "hub", *graph(rng, H + 1, pairs), a)
    ctx.close()


if __name__ == "__main__":
    main()
