"""GPU tests of radial-tangential lens distortion through the optimiser (cugo.Graph): the LM trajectory of a two-camera
rig (camera 0 distorted with all five coefficients, camera 1 undistorted; 6 poses, two of them fixed, x 80 landmarks)
against the numpy reference of tests/distort_lm_ref.py under the tolerance rule of icp_lm_ref.tolerances, as tests/test_fisheye_graph.py
uses it (per iteration max(1e-10, 4 x what the reference differs by from itself), estimates max(1e-9, 4 x)); zero-noise
recovery; the rig built from sets through C++ against the per-edge form; the fp32-internal mode; outlier rejection;
covariances against the dense inverse; flatten re-use after a changed coefficient; all-zero distortion against no
distortion, bit for bit; and the graph optimised WITHOUT its distortion, which must end far worse, as the reference's
does."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import distort_lm_ref as D
import icp_lm_ref as R
import rig_ref
import test_rig_graph as trg

pytestmark = pytest.mark.gpu

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
INC = trg.INC
NONE = (0, 1.0)
NITER = 6
assert_trajectories_match = trg.assert_trajectories_match


def case(name):
    if name == "rig":
        return dict(D.rig_problem(seed=21), rk2={0: NONE, 1: NONE}), NITER
    if name == "rig_huber":
        return dict(D.rig_problem(seed=22), rk2={0: (3, 1.5), 1: NONE}), NITER
    if name == "rig_exact":
        # (near landmarks and a turning body: every direction of the problem is well determined, so LM gets to the bottom)
        return dict(D.rig_problem(seed=23, pix_noise=0.0, depth=(2.0, 5.0), lm_noise=0.6, yaw_step=0.2), rk2={0: NONE, 1: NONE}), 12
    if name == "rig_wrong_model":
        d, niter = case("rig")
        return D.without_distortion(d), niter
    raise KeyError(name)


_REF = {}


def reference(name):
    if name not in _REF:
        d, niter = case(name)
        tr, pose, lm, sens, est = D.reference_runs(d, niter)
        print("reference %s: self-sensitivity %.3g (chi2), %.3g (estimates); trials %s; chi2 %.6g -> %.6g" %
              (name, max(sens), est, [t["trials"] for t in tr], tr[0]["chi2"], tr[-1]["chi2"]))
        tol, etol = R.tolerances(sens, est)
        _REF[name] = (d, niter, tr, pose, lm, tol, etol)
    return _REF[name]


def build_graph(d, threshold=0.0, distortion=True):
    """one mono set with a camera, a sensor pose and a distortion per edge (distortion False: the call without it)"""
    g = cugo.Graph(True, True)
    P, L = len(d["pose"]), len(d["lm"])
    g.add_poses(np.arange(P, dtype=np.int32), d["pose"], d["pose_fixed"])
    g.add_landmarks(np.arange(L, dtype=np.int32), d["lm"], d["lm_fixed"])
    assert not d["e_stereo"].any()
    g.add_edges(2, d["e_pose"], d["e_lm"], d["e_meas"], d["e_omega"], d["e_cam"], sensor=d["e_sensor"],
                distortion=d["e_dist"] if distortion else None)
    g.set_robust_kernel(2, d["rk2"][0][0], d["rk2"][0][1])
    if threshold:
        g.set_outlier_threshold(2, threshold)
    return g


def run(name_or_case, float32=False, keep=False, threshold=0.0, distortion=True):
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    d, niter = case(name_or_case) if isinstance(name_or_case, str) else name_or_case
    g = build_graph(d, threshold, distortion)
    if float32:
        g.set_float32(1)
    g.initialize()
    table = dict(g.flat_cameras(), dist=g.flat_camera_distortions())
    g.optimize(niter)
    out = dict(stats=g.stats(), pose=g.poses(), lm=g.landmarks(), nedges=g.n_active_edges(), table=table,
               n_dist=g.n_distorted_cameras())
    if keep:
        out["g"] = g
    else:
        g.close()
    return out


@pytest.mark.parametrize("name", ["rig", "rig_huber"])
def test_lm_trajectory_matches_the_reference(name):
    d, niter, tr, pose, lm, tol, etol = reference(name)
    assert len(tr) == niter and np.all(D.DIST != 0)
    out = run(name)
    assert out["nedges"] == len(d["e_pose"]) and out["n_dist"] == 1
    first = [int(np.flatnonzero(d["e_camera"] == c)[0]) for c in range(2)]
    order = np.argsort(first)                                  # first-seen order
    assert len(out["table"]["cams"]) == 2
    for k, c in enumerate(order):
        i = first[c]
        assert np.array_equal(out["table"]["cams"][k], d["e_cam"][i])
        assert np.array_equal(out["table"]["ext"][k], rig_ref.quat_to_ext(d["e_sensor"][i]))
        assert np.array_equal(out["table"]["dist"][k], d["e_dist"][i])
    assert_trajectories_match(out["stats"], tr, tol)
    np.testing.assert_allclose(out["pose"], pose, rtol=0, atol=etol)
    np.testing.assert_allclose(out["lm"], lm, rtol=0, atol=10 * etol)


def test_zero_noise_recovery_from_a_perturbed_start():
    """exact measurements, a start some centimetres and degrees off: chi2 falls by twelve orders and the estimates come
    back to the truth (poses 0 and 1 are fixed, which fixes the scale), as the reference's do"""
    d, niter, tr, pose, lm, tol, etol = reference("rig_exact")
    out = run("rig_exact")
    chi = [s["chi2"] for s in out["stats"]]
    print("chi2 %s; reference %s" % (["%.3g" % c for c in chi], ["%.3g" % t["chi2"] for t in tr]))
    assert tr[-1]["chi2"] < 1e-12 * tr[0]["chi2"] and chi[-1] < 1e-12 * chi[0]
    assert np.abs(out["lm"] - d["lm_gt"]).max() < 1e-6 and np.abs(out["pose"] - d["pose_gt"]).max() < 1e-7
    assert np.abs(d["lm"] - d["lm_gt"]).max() > 0.1


SETS_PROGRAM = (trg.SETS_PROGRAM
                .replace("double delta, c[5], q[7];", "double delta, c[5], q[7], dk[5];")
                .replace("        if (std::fscanf(f, \"%d\", &n) != 1) return 2;\n        const auto kernel",
                         "        for (double& x : dk) if (std::fscanf(f, \"%lf\", &x) != 1) return 2;\n"
                         "        if (std::fscanf(f, \"%d\", &n) != 1) return 2;\n        const auto kernel")
                .replace("        set->setSensorPose(cugo::Se3D(q, q + 4));\n",
                         "        set->setSensorPose(cugo::Se3D(q, q + 4));\n"
                         "        set->setDistortion(cugo::CameraDistortion(dk[0], dk[1], dk[2], dk[3], dk[4]));\n")
                .replace("    std::printf(\"table %d %d\", rig ? 1 : 0, opt.nRigCameras());\n",
                         "    std::vector<double> d5;\n    opt.flatCameraDistortions(d5);\n"
                         "    std::printf(\"distortions %d\", opt.nDistortedCameras());\n    for (double x : d5) std::printf(\" %a\", x);\n"
                         "    std::printf(\"\\ntable %d %d\", rig ? 1 : 0, opt.nRigCameras());\n"))
assert SETS_PROGRAM.count("dk[") >= 6 and "flatCameraDistortions" in SETS_PROGRAM


def sets_input(d, niter):
    """test_rig_graph.sets_input with the distortion (k1, k2, p1, p2, k3) behind the sensor pose of every set"""
    fl = lambda a: " ".join("%.17g" % x for x in a)
    lines = ["%d %d %d %d" % (len(d["pose"]), len(d["lm"]), len(d["sensors"]), niter)]
    lines += ["%d %s" % (f, fl(p)) for p, f in zip(d["pose"], d["pose_fixed"])]
    lines += ["%d %s" % (f, fl(x)) for x, f in zip(d["lm"], d["lm_fixed"])]
    for c in range(len(d["sensors"])):
        sel = np.flatnonzero(d["e_camera"] == c)
        rk = d["rk2"][0]
        lines.append("2 %d %.17g %s %s %s %d" % (rk[0], rk[1], fl(d["e_cam"][sel[0]]), fl(d["sensors"][c]), fl(d["e_dist"][sel[0]]), len(sel)))
        lines += ["%d %d %s %.17g" % (d["e_pose"][i], d["e_lm"][i], fl(d["e_meas"][i]), d["e_omega"][i]) for i in sel]
    return "\n".join(lines) + "\n"


def test_one_edge_set_per_camera_gives_the_per_edge_table_and_trajectory(tmp_path):
    """two MonoEdgeSets, each with its camera, sensor pose and distortion (one of them none), on the same pose vertices
    through the C++ interface, against the per-edge form: the same tables (as sets of entries) and the trajectory inside
    the reference's tolerances"""
    d, niter, tr, pose, lm, tol, etol = reference("rig_huber")
    per_edge = run("rig_huber")
    (tmp_path / "rig.txt").write_text(sets_input(d, niter))
    src, exe = tmp_path / "distort_sets.cpp", tmp_path / "distort_sets"
    src.write_text(SETS_PROGRAM)
    lib_dir = os.path.dirname(cugo.LIB_PATH)
    c = subprocess.run(["g++", "-std=c++17", "-O1", "-I", INC, str(src), "-L", lib_dir, "-lcugo_hip", "-Wl,-rpath," + lib_dir,
                        "-o", str(exe)], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-3000:]
    p = subprocess.run([str(exe), str(tmp_path / "rig.txt")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    rows = {ln.split()[0]: ln.split()[1:] for ln in p.stdout.splitlines() if ln.strip()}
    hexes = lambda k, a=0: np.array([float.fromhex(x) for x in rows[k][a:]])
    assert rows["table"][:2] == ["1", "2"] and rows["distortions"][0] == "1"
    table, dists = hexes("table", 2), hexes("distortions", 1).reshape(2, 5)
    full = np.concatenate([table[:10].reshape(2, 5), table[10:].reshape(2, 12), dists], 1)
    want = np.concatenate([per_edge["table"]["cams"], per_edge["table"]["ext"], per_edge["table"]["dist"]], 1)
    assert sorted(map(tuple, full)) == sorted(map(tuple, want))
    assert np.array_equal(dists, D.RIG2_DIST)                  # the sets' order is the cameras'
    chi, trials = hexes("chi2"), [int(x) for x in rows["trials"]]
    assert_trajectories_match([dict(chi2=float(x), trials=t) for x, t in zip(chi, trials)], tr, tol)
    got_pose, got_lm = hexes("pose").reshape(-1, 7), hexes("lm").reshape(-1, 3)
    np.testing.assert_allclose(got_pose, pose, rtol=0, atol=etol)
    np.testing.assert_allclose(got_lm, lm, rtol=0, atol=10 * etol)
    np.testing.assert_allclose(got_pose, per_edge["pose"], rtol=0, atol=2 * etol)


def test_float32_internal_mode_with_distorted_graphs():
    """float block storage: the bar tests/test_rig_graph.py states for the mode (chi2 to 1e-5, the same trials)"""
    d, niter, tr, pose, lm, tol, etol = reference("rig_huber")
    out = run("rig_huber", float32=True)
    assert_trajectories_match(out["stats"], tr, 1e-5, check_trials=False)
    assert [s["trials"] for s in out["stats"]] == [t["trials"] for t in tr]


def test_outlier_rejection_on_a_distorted_set_agrees_with_the_reference():
    """a tenth of the distorted camera's measurements off by 30 px; the verdicts of the reference at ITS final estimates,
    with no edge of the reference within 1 % of the threshold"""
    d, niter = case("rig")
    rng = np.random.default_rng(5)
    cam0 = np.flatnonzero(d["e_camera"] == 0)
    bad = cam0[rng.random(len(cam0)) < 0.1]
    assert len(bad) >= 2
    meas = d["e_meas"].copy()
    meas[bad, 0] += 30.0
    d = dict(d, e_meas=meas)
    ref = D.DistortGraph(d)
    ref.optimize(niter)
    chi = ref.edge_chi()
    srt = np.sort(chi)
    gaps = np.flatnonzero((srt[1:] > 1.2 * srt[:-1]) & (srt[:-1] > 5.0))
    assert len(gaps) >= 1, "the reference's chi2 terms leave no gap for a threshold"
    threshold = float(np.sqrt(srt[gaps[0]] * srt[gaps[0] + 1]))
    assert np.all(np.abs(chi - threshold) > 0.01 * threshold)
    verdict = chi > threshold
    assert 2 <= verdict.sum() < len(chi) // 2
    out = run((d, niter), keep=True, threshold=threshold)
    g = out["g"]
    assert np.array_equal(~g.edge_active(2, len(chi)), verdict)
    assert g.n_outliers(2) == verdict.sum()
    g.initialize()
    assert g.n_active_edges() == len(d["e_pose"]) - verdict.sum()
    g.close()


def test_covariances_match_the_dense_inverse():
    """the rule of tests/test_covariance.py (1e-8 of the block norm) against the inverse of the reference's undamped
    system at the optimiser's estimates"""
    d, niter = case("rig_huber")
    out = run("rig_huber", keep=True)
    g = out["g"]
    g.compute_covariances()
    ref = D.DistortGraph(d)
    ref.pose[:], ref.lm[:] = out["pose"], out["lm"]
    H, _ = ref.normal_equations()
    inv = np.linalg.inv(H)
    cp, cl = g.pose_covariances(), g.landmark_covariances()
    worst = [0.0, 0.0]
    for blocks, offs, w, q in ((cp, np.where(ref.pf, -1, 6 * ref.pidx), 6, 0),
                               (cl, np.where(ref.lf, -1, 6 * ref.np_ + 3 * ref.lidx), 3, 1)):
        for i, o in enumerate(offs):
            if o < 0:
                assert not blocks[i].any()
                continue
            blk = inv[o:o + w, o:o + w]
            worst[q] = max(worst[q], np.abs(blocks[i] - blk).max() / np.linalg.norm(blk))
    print("covariance blocks off by %.3g (poses), %.3g (landmarks) of the block norm" % tuple(worst))
    assert worst[0] <= 1e-8 and worst[1] <= 1e-8
    g.close()


def one_camera_graph(d, sel, dist):
    """set-level: camera 0's edges alone, with the set's camera, sensor pose and distortion (None: never set)"""
    g = cugo.Graph(True, False)
    g.add_poses(np.arange(len(d["pose"]), dtype=np.int32), d["pose"], d["pose_fixed"])
    g.add_landmarks(np.arange(len(d["lm"]), dtype=np.int32), d["lm"], d["lm_fixed"])
    g.add_edges(2, d["e_pose"][sel], d["e_lm"][sel], d["e_meas"][sel], d["e_omega"][sel])
    g.set_camera(2, d["e_cam"][np.flatnonzero(sel)[0]])
    g.set_sensor_pose(2, d["sensors"][0])
    if dist is not None:
        g.set_camera_distortion(2, dist)
    return g


def restart(g, d, niter=3):
    g.set_poses(np.arange(len(d["pose"]), dtype=np.int32), d["pose"])
    g.set_landmarks(np.arange(len(d["lm"]), dtype=np.int32), d["lm"])
    g.initialize()
    g.optimize(niter)
    return [(s["chi2"], s["trials"]) for s in g.stats()], g.poses(), g.landmarks()


def test_a_changed_coefficient_is_a_new_flattening_and_another_trajectory():
    """set-level distortion: the same scene with ONE camera (camera 0's edges), one coefficient changed between two
    initialize() calls — the second run is the run of a fresh graph with the new coefficients, bit for bit, and a third
    initialize() with nothing changed re-uses the flattening"""
    d, niter = case("rig")
    sel = d["e_camera"] == 0
    d_new = D.DIST.copy()
    d_new[4] *= 3.0                                            # k3 alone
    g = one_camera_graph(d, sel, D.DIST)
    a = restart(g, d)
    assert g.flatten_reuses() == 0
    g.set_camera_distortion(2, d_new)
    b = restart(g, d)
    assert g.flatten_reuses() == 0 and np.array_equal(g.flat_camera_distortions()[0], d_new)
    c = restart(g, d)
    assert g.flatten_reuses() == 1
    g.close()
    fresh = one_camera_graph(d, sel, d_new)
    f = restart(fresh, d)
    fresh.close()
    assert a[0] != b[0], "the changed coefficient did not reach the kernels"
    for x, y in ((b, f), (c, f)):
        assert x[0] == y[0] and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2])


def test_all_zero_distortion_gives_the_bits_of_the_graph_without_the_calls():
    """zeros given at set level, zeros given per edge, and nothing given: the same kernels, the same bits"""
    d, niter = case("rig_wrong_model")
    assert not d["e_dist"].any()
    plain = run((d, niter), distortion=False)
    zeros = run((d, niter), distortion=True)
    assert plain["n_dist"] == 0 and zeros["n_dist"] == 0 and plain["table"]["has_rig"] and zeros["table"]["has_rig"]
    assert [(s["chi2"], s["trials"]) for s in plain["stats"]] == [(s["chi2"], s["trials"]) for s in zeros["stats"]]
    assert np.array_equal(plain["pose"], zeros["pose"]) and np.array_equal(plain["lm"], zeros["lm"])
    sel = d["e_camera"] == 0
    a, b = one_camera_graph(d, sel, None), one_camera_graph(d, sel, np.zeros(5))
    ra, rb = restart(a, d), restart(b, d)
    assert a.n_distorted_cameras() == 0 and b.n_distorted_cameras() == 0
    a.close(), b.close()
    assert ra[0] == rb[0] and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])


def test_the_graph_optimised_without_its_distortion_ends_far_worse():
    """the same raw measurements with every coefficient zero (what a caller gets who forgets the distortion): the
    reference's own two runs end a factor `ratio` apart, far more than 10; the optimiser follows the reference on the
    wrong model as closely as on the right one (that run's own tolerances), so its ratio is the reference's to the sum
    of the two final tolerances"""
    d, niter, tr, pose, lm, tol, etol = reference("rig")
    dw, _, trw, posew, lmw, tolw, etolw = reference("rig_wrong_model")
    ratio_ref = trw[-1]["chi2"] / tr[-1]["chi2"]
    right, wrong = run("rig"), run("rig_wrong_model")
    assert wrong["n_dist"] == 0 and right["n_dist"] == 1
    assert_trajectories_match(wrong["stats"], trw, tolw)
    ratio = wrong["stats"][-1]["chi2"] / right["stats"][-1]["chi2"]
    print("final chi2 without / with the distortion: %.6g (reference %.6g)" % (ratio, ratio_ref))
    assert ratio_ref > 10 and ratio > 10
    last = lambda t: t[-1] if isinstance(t, list) else t
    assert abs(ratio - ratio_ref) <= 2 * (last(tol) + last(tolw)) * ratio_ref
