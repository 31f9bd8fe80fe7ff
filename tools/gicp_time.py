"""Times the build and error passes of the covariance form of the two point kinds (cugo_gicp_pair_*, cugo_gicp_*:
generalised ICP, Omega formed from two covariances at the poses of the pass) against the information form
(cugo_point_pair_*, cugo_point_*) ON THE SAME EDGES AND POSES, through the kernel-level C ABI.  The information form is
fed the Omega the covariances give at those poses, so both forms compute the same term; its kernels are untouched by the
covariance form, so its number is the yardstick.

The shape is that of tools/point_pair_time.py: --scans scans (default 8, the last one fixed), ALL pairs of them (28),
--per-pair correspondences per pair (default 4096), per-edge covariances with eigenvalues (1, 1, 1e-3) in random frames;
the unary kind on the same number of edges spread over the free poses.

Per pass: host-clock median over --reps calls after --warmup, each call followed by a stream synchronisation.  A call is
the whole entry point: the index check with its one flag read back, the chunk pass, for a build pass the finishing passes
and the sum of the chunk totals.  Everything but the chunk pass is the same code for both forms, so the DIFFERENCE of two
rows is the chunk kernels' and the ratio understates theirs."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import devmem  # noqa: E402
import gicp_designed as gd  # noqa: E402
import gicp_ref as gr  # noqa: E402
import icp_ref  # noqa: E402
import pair_designed as pdz  # noqa: E402
import point_designed as pt  # noqa: E402
import point_pair_ref as ppr  # noqa: E402
import pose_designed as pd  # noqa: E402

cugo = importlib.import_module("cuda-bundle-adjustment_amd")


def see(pose, X):
    """y = R(q) X + t, vectorised (the cross-product form)"""
    q = pose[:, :4]
    t1 = 2 * np.cross(q[:, :3], X)
    return X + q[:, 3:] * t1 + np.cross(q[:, :3], t1) + pose[:, 4:]


def clock(ctx, a, f):
    times = []
    for rep in range(a.warmup + a.reps):
        ctx.sync()
        t0 = time.perf_counter()
        f()
        ctx.sync()
        if rep >= a.warmup:
            times.append(1e3 * (time.perf_counter() - t0))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def report(rows):
    for name in ("build", "errors"):
        cov, info = rows["cov " + name], rows["info " + name]
        for form, t in (("covariance ", cov), ("information", info)):
            print("    %-7s %s  median %8.3f ms, range %.3f .. %.3f" % (name, form, t[0], t[1], t[2]))
        print("    %-7s ratio covariance / information %.3f, difference %.3f ms" % (name, cov[0] / info[0], cov[0] - info[0]))


def time_pair(ctx, a, poses, P, ia, ib, p, z, cov_p6, cov_z6):
    Pall, E = len(poses), len(ia)
    e = dict(a=ia, b=ib, p=p, z=z, cov_p6=cov_p6, cov_z6=cov_z6, active=np.ones(E, bool), flags=None, rk=(cugo.RK_HUBER, 0.5))
    free = ppr.numpy_plan(ia, ib, None, P)
    rowptr, colind = ppr.pair_pattern(P, free["pair_lo"], free["pair_hi"])
    plan = cugo.PointPairPlan(ctx.h, Pall, P, ia, ib, None, rowptr, colind)
    perm = plan.array("perm")
    pa, pb, dp, dz, cp, cz, _ = gd.pair_device_arrays(e, perm)
    info = pdz.device_arrays(gr.with_info(e, gr.omega_of_replay(poses, e)), perm)[4]
    common = dict(n_poses_total=Pall, n_poses_free=P, n=E, d_pose_a=ctx.to_dev(pa), d_pose_b=ctx.to_dev(pb), d_p=ctx.to_dev(dp),
                  d_z=ctx.to_dev(dz), rk=cugo.RK_HUBER, delta=0.5, plan=plan.handle)
    ev_c = cugo.GicpPairEdges(d_cov_p=ctx.to_dev(cp), d_cov_z=ctx.to_dev(cz), n_cov=E, **common)
    ev_i = cugo.PointPairEdges(d_info=ctx.to_dev(info), n_info=E, **common)
    d_poses, d_chi = ctx.to_dev(poses), ctx.to_dev(np.zeros(2))
    d_H, d_b, d_Hoff = ctx.to_dev(np.zeros((Pall, 36))), ctx.to_dev(np.zeros((Pall, 6))), ctx.to_dev(np.zeros((len(colind), 36)))
    rows = {
        "cov build": clock(ctx, a, lambda: cugo.gicp_pair_construct_quadratic_form(ctx.h, ev_c, d_poses, d_H, d_b, d_Hoff, d_chi)),
        "info build": clock(ctx, a, lambda: cugo.point_pair_construct_quadratic_form(ctx.h, ev_i, d_poses, d_H, d_b, d_Hoff, d_chi)),
        "cov errors": clock(ctx, a, lambda: cugo.gicp_pair_compute_errors(ctx.h, ev_c, d_poses, d_chi)),
        "info errors": clock(ctx, a, lambda: cugo.point_pair_compute_errors(ctx.h, ev_i, d_poses, d_chi)),
    }
    chi = []
    for f, ev in ((cugo.gicp_pair_compute_errors, ev_c), (cugo.point_pair_compute_errors, ev_i)):
        f(ctx.h, ev, d_poses, d_chi)
        chi.append(ctx.to_host(d_chi, 1)[0])
    print("pair kind, %d edges in %d runs: chi2 %.9g (covariance form), %.9g (information form fed its Omega)" % (E, len(free["run_a"]), chi[0], chi[1]))
    report(rows)
    plan.close()


def time_point(ctx, a, poses, P, pose, p, z, cov_p6, cov_z6):
    order = np.argsort(pose, kind="stable")
    pose, p, z, cov_p6, cov_z6 = pose[order], p[order], z[order], cov_p6[order], cov_z6[order]
    Pall, E = len(poses), len(pose)
    e = dict(pose=pose, p=p, z=z, cov_p6=cov_p6, cov_z6=cov_z6, active=np.ones(E, bool), flags=None, rk=(cugo.RK_HUBER, 0.5))
    dp, dz, cp, cz = gd.point_device_arrays(e)
    info = pt.device_arrays(gr.with_info(e, gr.omega_of_replay(poses, e)))[2]
    common = dict(n_poses_total=Pall, n_poses_free=P, n=E, d_pose=ctx.to_dev(pose.astype(np.int32)),
                  d_pose_ptr=ctx.to_dev(pd.pose_ptr(pose, Pall)), d_p=ctx.to_dev(dp), d_z=ctx.to_dev(dz), rk=cugo.RK_HUBER, delta=0.5)
    ev_c = cugo.GicpEdges(d_cov_p=ctx.to_dev(cp), d_cov_z=ctx.to_dev(cz), n_cov=E, **common)
    ev_i = cugo.PointEdges(d_info=ctx.to_dev(info), n_info=E, **common)
    d_poses, d_chi = ctx.to_dev(poses), ctx.to_dev(np.zeros(2))
    d_H, d_b = ctx.to_dev(np.zeros((Pall, 36))), ctx.to_dev(np.zeros((Pall, 6)))
    rows = {
        "cov build": clock(ctx, a, lambda: cugo.gicp_construct_quadratic_form(ctx.h, ev_c, d_poses, d_H, d_b, d_chi)),
        "info build": clock(ctx, a, lambda: cugo.point_construct_quadratic_form(ctx.h, ev_i, d_poses, d_H, d_b, d_chi)),
        "cov errors": clock(ctx, a, lambda: cugo.gicp_compute_errors(ctx.h, ev_c, d_poses, d_chi)),
        "info errors": clock(ctx, a, lambda: cugo.point_compute_errors(ctx.h, ev_i, d_poses, d_chi)),
    }
    print("unary kind, %d edges on %d free poses" % (E, P))
    report(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=8)
    ap.add_argument("--per-pair", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=21)
    a = ap.parse_args()
    if cugo.device_count() == 0:
        raise SystemExit("no HIP device")
    rng = np.random.default_rng(0)
    S = a.scans
    gt = np.array([icp_ref.random_pose(rng, rot=0.3, trans=5.0) for _ in range(S)])
    poses = gt.copy()
    for i in range(S - 1):
        poses[i] = icp_ref.left_update(gt[i], np.concatenate([rng.normal(0, 0.05, 3), rng.normal(0, 0.3, 3)]))
    pairs = [(i, j) if (i + j) % 2 else (j, i) for i in range(S) for j in range(i + 1, S)]   # mixed orientation
    ia = np.repeat([q[0] for q in pairs], a.per_pair).astype(np.int32)
    ib = np.repeat([q[1] for q in pairs], a.per_pair).astype(np.int32)
    order = rng.permutation(len(ia))            # the container is not sorted by pair
    ia, ib = ia[order], ib[order]
    E = len(ia)
    X = rng.normal(0, 3.0, (E, 3))
    cov_p6, cov_z6 = gd.make_cov(rng, "gicp", np.zeros((E, 3, 3)))
    print("%d scans (one fixed), %d pairs x %d correspondences = %d edges, per-edge covariances (1, 1, 1e-3), Huber 0.5"
          % (S, len(pairs), a.per_pair, E))
    ctx = devmem.Ctx()
    time_pair(ctx, a, poses, S - 1, ia, ib, see(gt[ia], X) + rng.normal(0, 0.03, (E, 3)), see(gt[ib], X) + rng.normal(0, 0.03, (E, 3)),
              cov_p6, cov_z6)
    free = np.where(ib == S - 1, ia, ib).astype(np.int32)
    time_point(ctx, a, poses, S - 1, free, X, see(gt[free], X) + rng.normal(0, 0.03, (E, 3)), cov_p6, cov_z6)
    ctx.close()


if __name__ == "__main__":
    main()
