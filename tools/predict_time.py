"""Host-clock time of Graph.predict_observations next to Graph.reprojection_covariances on the kitti_00-shaped BA graph
of bench.py (1322 poses, 133 383 landmarks, 561 116 edges): the newest keyframe against every landmark with two edges
or more, as tools/pl_cov_time.py asks.  Four calls, INTERLEAVED, --reps each after a warm-up round:

    reprojection_covariances(dim=2)                       k_reprojection_cov
    predict_observations(kind=2)                          k_predict_obs without a table: the same operations, z besides
    predict_observations(kind=2, sensor=rig)              landmark l through camera l % 4 of the rig of tools/rig_time.py
    predict_observations(kind=2, sensor=rig, model=KB)    the same cameras as Kannala-Brandt fisheyes

Every call runs the build pass, the Schur complement, one factorisation at lambda = 0, the plan of the batch, the pose
blocks, k_pose_lm_cross, the selected inverse and k_lm_covariance before its own kernel, and ends with its results on
the host: the four differ in the last kernel and in what travels (17 doubles per query up with a table, 3 more down).

    python tools/predict_time.py [--reps 6] [--shapes kitti00]

For the kernels alone run it in a pass of its own under
`rocprofv3 --kernel-trace --stats -- python tools/predict_time.py --reps 2` (k_reprojection_cov, k_predict_obs)."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
cugo = importlib.import_module("cuda-bundle-adjustment_amd")
from pl_cov_time import SHAPES  # noqa: E402
from rig_time import SENSORS  # noqa: E402

KB = np.array([[-0.0131, 0.0212, -0.0071, 0.0012, 1.0], [0.0, 0.0, 0.0, 0.0, 1.0], [0.0342, -0.0094, 0.0038, -0.0009, 1.0],
               [-0.00655, 0.0106, -0.00355, 0.0006, 1.0]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--shapes", default="kitti00")
    a = ap.parse_args()
    for name in a.shapes.split(","):
        P, L, E, seed, lc, st = SHAPES[name]
        d = cugo.synth(P, L, E, seed=seed, n_loop_closures=lc, stereo_fraction=st)
        g = cugo.graph_from_arrays(d)
        g.initialize()
        g.optimize(10)
        g.optimize(10)
        lms = np.flatnonzero(np.bincount(d["e_lm"], minlength=L) >= 2).astype(np.int32)
        qa = np.full(len(lms), P - 1, np.int32)
        cam = np.asarray(d["cam"], np.float64)
        sens, model = SENSORS[lms % 4], KB[lms % 4]
        calls = (("reprojection_covariances", lambda: g.reprojection_covariances(qa, lms, dim=2, cam=cam)),
                 ("predict, no table", lambda: g.predict_observations(qa, lms, kind=2, cam=cam)),
                 ("predict, 4-camera rig", lambda: g.predict_observations(qa, lms, kind=2, cam=cam, sensor=sens)),
                 ("predict, Kannala-Brandt rig", lambda: g.predict_observations(qa, lms, kind=2, cam=cam, sensor=sens, model=model)))
        ms = {what: [] for what, _ in calls}
        try:
            for rep in range(a.reps + 1):     # (round 0 warms up: the first call of a kind allocates its buffers)
                for what, fn in calls:
                    t = time.perf_counter()
                    fn()
                    if rep:
                        ms[what].append((time.perf_counter() - t) * 1e3)
        except cugo.CugoError as e:           # (a zero pivot or an edgeless landmark: nothing to time)
            print("%-8s not measured: %s" % (name, e), flush=True)
            g.close()
            continue
        z, S = g.predict_observations(qa, lms, kind=2, cam=cam)
        assert np.array_equal(S, g.reprojection_covariances(qa, lms, dim=2, cam=cam))
        for what, _ in calls:
            v = sorted(ms[what])
            print("%-8s keyframe %d x %d landmarks | %-28s median %.3f ms (min %.3f, max %.3f; %d interleaved reps)"
                  % (name, P - 1, len(lms), what, v[len(v) // 2], v[0], v[-1], len(v)), flush=True)
        g.close()


if __name__ == "__main__":
    main()
