"""GPU tests of camera models (Kannala-Brandt fisheye) through the optimiser (cugo.Graph): the LM trajectory of the ring
scene (four fisheye cameras, each with edges beyond 90 degrees off its axis) against the numpy reference of
tests/fisheye_lm_ref.py under the tolerance rule of icp_lm_ref.tolerances, as tests/test_rig_graph.py uses it (per
iteration max(1e-10, 4 x what the reference differs by from itself), estimates max(1e-9, 4 x)); zero-noise recovery;
the rig built from sets through C++ against the per-edge form; the fp32-internal mode; outlier rejection; covariances
against the dense inverse; flatten re-use after a changed coefficient; body-frame priors and relative-pose edges next
to fisheye edges.  Graphs of 5 poses x 32 landmarks."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import fisheye_lm_ref as F
import icp_lm_ref as R
import prior_ref as PR
import relpose_lm_ref as RL
import relpose_ref as RR
import rig_ref
import test_rig_graph as trg

pytestmark = pytest.mark.gpu

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
INC = trg.INC
NONE = (0, 1.0)
NITER = 6
assert_trajectories_match = trg.assert_trajectories_match


def case(name):
    if name == "ring":
        return dict(F.ring_problem(seed=7), rk2={0: NONE, 1: NONE}), NITER
    if name == "ring_huber":
        return dict(F.ring_problem(seed=8), rk2={0: (3, 1.5), 1: NONE}), NITER
    if name == "ring_exact":
        return dict(F.ring_problem(seed=9, pix_noise=0.0), rk2={0: NONE, 1: NONE}), 10
    raise KeyError(name)


_REF = {}


def reference(name):
    if name not in _REF:
        d, niter = case(name)
        tr, pose, lm, sens, est = F.reference_runs(d, niter)
        print("reference %s: self-sensitivity %.3g (chi2), %.3g (estimates); trials %s; chi2 %.6g -> %.6g" %
              (name, max(sens), est, [t["trials"] for t in tr], tr[0]["chi2"], tr[-1]["chi2"]))
        tol, etol = R.tolerances(sens, est)
        _REF[name] = (d, niter, tr, pose, lm, tol, etol)
    return _REF[name]


def build_graph(d, threshold=0.0):
    """one mono set with a camera, a sensor pose and a model per edge"""
    g = cugo.Graph(True, True)
    P, L = len(d["pose"]), len(d["lm"])
    g.add_poses(np.arange(P, dtype=np.int32), d["pose"], d["pose_fixed"])
    g.add_landmarks(np.arange(L, dtype=np.int32), d["lm"], d["lm_fixed"])
    assert not d["e_stereo"].any()
    g.add_edges(2, d["e_pose"], d["e_lm"], d["e_meas"], d["e_omega"], d["e_cam"], sensor=d["e_sensor"], model=d["e_model"])
    g.set_robust_kernel(2, d["rk2"][0][0], d["rk2"][0][1])
    if threshold:
        g.set_outlier_threshold(2, threshold)
    return g


def run(name_or_case, float32=False, keep=False, threshold=0.0, extra=None):
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    d, niter = case(name_or_case) if isinstance(name_or_case, str) else name_or_case
    g = build_graph(d, threshold)
    if extra:
        extra(g)
    if float32:
        g.set_float32(1)
    g.initialize()
    table = dict(g.flat_cameras(), model=g.flat_camera_models())
    g.optimize(niter)
    out = dict(stats=g.stats(), pose=g.poses(), lm=g.landmarks(), nedges=g.n_active_edges(), table=table,
               n_fish=g.n_fisheye_cameras())
    if keep:
        out["g"] = g
    else:
        g.close()
    return out


@pytest.mark.parametrize("name", ["ring", "ring_huber"])
def test_lm_trajectory_matches_the_reference(name):
    d, niter, tr, pose, lm, tol, etol = reference(name)
    assert len(tr) == niter
    out = run(name)
    assert out["nedges"] == len(d["e_pose"]) and out["n_fish"] == 4
    first = [int(np.flatnonzero(d["e_camera"] == c)[0]) for c in range(4)]
    order = np.argsort(first)                                  # first-seen order
    assert len(out["table"]["cams"]) == 4
    for k, c in enumerate(order):
        i = first[c]
        assert np.array_equal(out["table"]["cams"][k], d["e_cam"][i])
        assert np.array_equal(out["table"]["ext"][k], rig_ref.quat_to_ext(d["e_sensor"][i]))
        assert np.array_equal(out["table"]["model"][k], d["e_model"][i])
    assert_trajectories_match(out["stats"], tr, tol)
    np.testing.assert_allclose(out["pose"], pose, rtol=0, atol=etol)
    np.testing.assert_allclose(out["lm"], lm, rtol=0, atol=10 * etol)


def test_zero_noise_recovery_from_a_perturbed_start():
    """exact measurements, a start some centimetres and degrees off: chi2 falls by twelve orders and the estimates come
    back to the truth (pose 0 is fixed and the lever arms fix the scale), as the reference's do"""
    d, niter, tr, pose, lm, tol, etol = reference("ring_exact")
    out = run("ring_exact")
    chi = [s["chi2"] for s in out["stats"]]
    print("chi2 %s; reference %s" % (["%.3g" % c for c in chi], ["%.3g" % t["chi2"] for t in tr]))
    assert tr[-1]["chi2"] < 1e-12 * tr[0]["chi2"] and chi[-1] < 1e-12 * chi[0]
    assert np.abs(out["lm"] - d["lm_gt"]).max() < 1e-6 and np.abs(out["pose"] - d["pose_gt"]).max() < 1e-7
    assert np.abs(d["lm"] - d["lm_gt"]).max() > 0.1


SETS_PROGRAM = (trg.SETS_PROGRAM
                .replace("double delta, c[5], q[7];", "double delta, c[5], q[7], mk[5];")
                .replace("        if (std::fscanf(f, \"%d\", &n) != 1) return 2;\n        const auto kernel",
                         "        for (double& x : mk) if (std::fscanf(f, \"%lf\", &x) != 1) return 2;\n"
                         "        if (std::fscanf(f, \"%d\", &n) != 1) return 2;\n        const auto kernel")
                .replace("        set->setSensorPose(cugo::Se3D(q, q + 4));\n",
                         "        set->setSensorPose(cugo::Se3D(q, q + 4));\n"
                         "        set->setCameraModel(cugo::CameraModel(mk[4] != 0.0 ? cugo::KannalaBrandt : cugo::Pinhole, mk[0], mk[1], "
                         "mk[2], mk[3]));\n")
                .replace("    std::printf(\"table %d %d\", rig ? 1 : 0, opt.nRigCameras());\n",
                         "    std::vector<double> m5;\n    opt.flatCameraModels(m5);\n"
                         "    std::printf(\"models %d\", opt.nFisheyeCameras());\n    for (double x : m5) std::printf(\" %a\", x);\n"
                         "    std::printf(\"\\ntable %d %d\", rig ? 1 : 0, opt.nRigCameras());\n"))
assert SETS_PROGRAM.count("mk[") >= 6 and "flatCameraModels" in SETS_PROGRAM


def sets_input(d, niter):
    """test_rig_graph.sets_input with the model (k1, k2, k3, k4, type) behind the sensor pose of every set"""
    fl = lambda a: " ".join("%.17g" % x for x in a)
    lines = ["%d %d %d %d" % (len(d["pose"]), len(d["lm"]), len(d["sensors"]), niter)]
    lines += ["%d %s" % (f, fl(p)) for p, f in zip(d["pose"], d["pose_fixed"])]
    lines += ["%d %s" % (f, fl(x)) for x, f in zip(d["lm"], d["lm_fixed"])]
    for c in range(len(d["sensors"])):
        sel = np.flatnonzero(d["e_camera"] == c)
        rk = d["rk2"][0]
        lines.append("2 %d %.17g %s %s %s %d" % (rk[0], rk[1], fl(d["e_cam"][sel[0]]), fl(d["sensors"][c]), fl(d["e_model"][sel[0]]), len(sel)))
        lines += ["%d %d %s %.17g" % (d["e_pose"][i], d["e_lm"][i], fl(d["e_meas"][i]), d["e_omega"][i]) for i in sel]
    return "\n".join(lines) + "\n"


def test_one_edge_set_per_fisheye_camera_gives_the_per_edge_table_and_trajectory(tmp_path):
    """four MonoEdgeSets, each with its camera, sensor pose and Kannala-Brandt coefficients, on the same pose vertices
    through the C++ interface, against the per-edge form: the same tables (as sets of entries: a landmark's edges are
    several cameras' here, so the sets' first-seen order is the cameras') and the trajectory inside the reference's
    tolerances"""
    d, niter, tr, pose, lm, tol, etol = reference("ring_huber")
    per_edge = run("ring_huber")
    (tmp_path / "ring.txt").write_text(sets_input(d, niter))
    src, exe = tmp_path / "fisheye_sets.cpp", tmp_path / "fisheye_sets"
    src.write_text(SETS_PROGRAM)
    lib_dir = os.path.dirname(cugo.LIB_PATH)
    c = subprocess.run(["g++", "-std=c++17", "-O1", "-I", INC, str(src), "-L", lib_dir, "-lcugo_hip", "-Wl,-rpath," + lib_dir,
                        "-o", str(exe)], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-3000:]
    p = subprocess.run([str(exe), str(tmp_path / "ring.txt")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    rows = {ln.split()[0]: ln.split()[1:] for ln in p.stdout.splitlines() if ln.strip()}
    hexes = lambda k, a=0: np.array([float.fromhex(x) for x in rows[k][a:]])
    assert rows["table"][:2] == ["1", "4"] and rows["models"][0] == "4"
    table, models = hexes("table", 2), hexes("models", 1).reshape(4, 5)
    full = np.concatenate([table[:20].reshape(4, 5), table[20:].reshape(4, 12), models], 1)
    want = np.concatenate([per_edge["table"]["cams"], per_edge["table"]["ext"], per_edge["table"]["model"]], 1)
    assert sorted(map(tuple, full)) == sorted(map(tuple, want))
    for c_ in range(4):                                        # the sets' order is the cameras'
        assert np.array_equal(models[c_], np.concatenate([F.RING_K[c_], [1.0]]))
    chi, trials = hexes("chi2"), [int(x) for x in rows["trials"]]
    assert_trajectories_match([dict(chi2=float(x), trials=t) for x, t in zip(chi, trials)], tr, tol)
    got_pose, got_lm = hexes("pose").reshape(-1, 7), hexes("lm").reshape(-1, 3)
    np.testing.assert_allclose(got_pose, pose, rtol=0, atol=etol)
    np.testing.assert_allclose(got_lm, lm, rtol=0, atol=10 * etol)
    np.testing.assert_allclose(got_pose, per_edge["pose"], rtol=0, atol=2 * etol)


def test_float32_internal_mode_with_fisheye_graphs():
    """float block storage: the bar tests/test_rig_graph.py states for the mode (chi2 to 1e-5, the same trials)"""
    d, niter, tr, pose, lm, tol, etol = reference("ring_huber")
    out = run("ring_huber", float32=True)
    assert_trajectories_match(out["stats"], tr, 1e-5, check_trials=False)
    assert [s["trials"] for s in out["stats"]] == [t["trials"] for t in tr]


def test_outlier_rejection_on_a_fisheye_set_agrees_with_the_reference():
    """a tenth of the side camera's measurements off by 30 px; the verdicts of the reference at ITS final estimates,
    with no edge of the reference within 1 % of the threshold"""
    d, niter = case("ring")
    rng = np.random.default_rng(5)
    side = np.flatnonzero(d["e_camera"] == 1)
    bad = side[rng.random(len(side)) < 0.1]
    assert len(bad) >= 2
    meas = d["e_meas"].copy()
    meas[bad, 0] += 30.0
    d = dict(d, e_meas=meas)
    ref = F.FisheyeGraph(d)
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
    d, niter = case("ring_huber")
    out = run("ring_huber", keep=True)
    g = out["g"]
    g.compute_covariances()
    ref = F.FisheyeGraph(d)
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


def test_a_changed_coefficient_is_a_new_flattening_and_another_trajectory():
    """set-level models: the same scene with ONE camera (camera 0's edges), its coefficients changed between two
    initialize() calls — the second run is the run of a fresh graph with the new coefficients, bit for bit, and a third
    initialize() with nothing changed re-uses the flattening"""
    d, niter = case("ring")
    sel = d["e_camera"] == 0
    k_new = F.RING_K[0] * 1.1

    def make(k):
        g = cugo.Graph(True, False)
        g.add_poses(np.arange(len(d["pose"]), dtype=np.int32), d["pose"], d["pose_fixed"])
        g.add_landmarks(np.arange(len(d["lm"]), dtype=np.int32), d["lm"], d["lm_fixed"])
        g.add_edges(2, d["e_pose"][sel], d["e_lm"][sel], d["e_meas"][sel], d["e_omega"][sel])
        g.set_camera(2, F.RING_CAMS[0])
        g.set_sensor_pose(2, d["sensors"][0])
        g.set_camera_model(2, 1, k)
        return g

    def go(g):
        g.set_poses(np.arange(len(d["pose"]), dtype=np.int32), d["pose"])
        g.set_landmarks(np.arange(len(d["lm"]), dtype=np.int32), d["lm"])
        g.initialize()
        g.optimize(3)
        return [(s["chi2"], s["trials"]) for s in g.stats()], g.poses(), g.landmarks()

    g = make(F.RING_K[0])
    a = go(g)
    assert g.flatten_reuses() == 0
    g.set_camera_model(2, 1, k_new)
    b = go(g)
    assert g.flatten_reuses() == 0 and np.array_equal(g.flat_camera_models()[0], np.concatenate([k_new, [1.0]]))
    c = go(g)
    assert g.flatten_reuses() == 1
    g.close()
    fresh = make(k_new)
    f = go(fresh)
    fresh.close()
    assert a[0] != b[0], "the changed coefficient did not reach the kernels"
    for x, y in ((b, f), (c, f)):
        assert x[0] == y[0] and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2])


def test_body_frame_priors_and_relative_pose_edges_next_to_fisheye_edges():
    d, niter = case("ring")
    rng = np.random.default_rng(9)
    gt = d["pose_gt"]
    prior = PR.make_prior([2, 4], [PR.displaced(rng, gt[p], 0.01, 0.05) for p in (2, 4)], [PR.random_spd(rng, 50.0) for _ in range(2)])
    pairs = [(i, i + 1) if i % 2 == 0 else (i + 1, i) for i in range(len(gt) - 1)]
    rp = RL.edges_between(rng, gt, pairs, 0.005, 0.02, 200.0, rk=(RR.RK_CAUCHY, 5.0))
    make = lambda dd, vs: F.FisheyeRelPoseGraph(dd, [], prior, rp, via_schur=vs)
    tr, pose, lm, sens, est = F.reference_runs(d, niter, make)
    tol, etol = R.tolerances(sens, est)

    def extra(g):
        PR.add_priors(g, prior)
        RL.add_relpose(g, rp)

    out = run((d, niter), extra=extra)
    assert_trajectories_match(out["stats"], tr, tol)
    np.testing.assert_allclose(out["pose"], pose, rtol=0, atol=etol)
    np.testing.assert_allclose(out["lm"], lm, rtol=0, atol=10 * etol)
    assert abs(tr[-1]["chi2"] - reference("ring")[2][-1]["chi2"]) > 1e-3 * tr[-1]["chi2"]
