"""GPU tests of camera extrinsics through the optimiser (cugo.Graph): the LM trajectory against the numpy reference of
tests/rig_lm_ref.py (make_golden.Graph with the edge seen through a sensor pose) under the tolerance rule of
icp_lm_ref.tolerances (per iteration max(1e-10, 4 x what the reference differs by from itself — Schur against dense
solve, edges permuted), estimates max(1e-9, 4 x)); scale from mono edges and a lever arm; the forms of the loop; the
fp32-internal mode; outlier rejection; covariances against the dense inverse; body-frame pose priors and relative-pose
edges next to rig edges; flatten re-use.  Graphs of 8 poses x 60 landmarks."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import icp_lm_ref as R
import prior_ref as PR
import relpose_lm_ref as RL
import relpose_ref as RR
import rig_lm_ref as G
import rig_ref
from rig_lm_ref import MG

pytestmark = pytest.mark.gpu

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cuda-bundle-adjustment_amd", "include")
NONE = (0, 1.0)
RIG3, RIG_SCALE, SCALE_ITERS = G.RIG3, G.RIG_SCALE, G.SCALE_ITERS
scale_problem, scale_of = G.scale_problem, G.scale_of


def case(name):
    if name == "rig3":
        return dict(G.make_rig_problem(RIG3, (0, 0, 1), seed=41), rk2={0: NONE, 1: NONE}), 6
    if name == "mixed":
        return dict(G.make_rig_problem(RIG3, (0, 0, 1), seed=43), rk2={0: (1, 3.0), 1: (3, 1.5)}), 6
    if name == "scale":
        return dict(scale_problem(RIG_SCALE), rk2={0: NONE, 1: NONE}), SCALE_ITERS
    raise KeyError(name)


_REF = {}


def reference(name):
    if name not in _REF:
        d, niter = case(name)
        tr, pose, lm, sens, est = G.reference_runs(d, niter)
        print("reference %s: self-sensitivity %.3g (chi2), %.3g (estimates); trials %s; chi2 %.6g -> %.6g" %
              (name, max(sens), est, [t["trials"] for t in tr], tr[0]["chi2"], tr[-1]["chi2"]))
        tol, etol = R.tolerances(sens, est)
        _REF[name] = (d, niter, tr, pose, lm, tol, etol)
    return _REF[name]


def build_graph(d, threshold=0.0, per_edge=True):
    """per_edge: one mono and one stereo set with a sensor pose per edge; otherwise (graphs with ONE camera per kind)
    the sets' sensor poses"""
    g = cugo.Graph(True, per_edge)
    P, L = len(d["pose"]), len(d["lm"])
    g.add_poses(np.arange(P, dtype=np.int32), d["pose"], d["pose_fixed"])
    g.add_landmarks(np.arange(L, dtype=np.int32), d["lm"], d["lm_fixed"])
    for dim in (2, 3):
        sel = d["e_stereo"] == (dim == 3)
        if not sel.any():
            continue
        if per_edge:
            g.add_edges(dim, d["e_pose"][sel], d["e_lm"][sel], d["e_meas"][sel], d["e_omega"][sel], d["e_cam"][sel],
                        sensor=d["e_sensor"][sel])
        else:
            assert len(np.unique(d["e_camera"][sel])) == 1
            g.add_edges(dim, d["e_pose"][sel], d["e_lm"][sel], d["e_meas"][sel], d["e_omega"][sel])
            g.set_camera(dim, d["e_cam"][sel][0])
            g.set_sensor_pose(dim, d["e_sensor"][sel][0])
        g.set_robust_kernel(dim, d["rk2"][dim - 2][0], d["rk2"][dim - 2][1])
        if threshold:
            g.set_outlier_threshold(dim, threshold)
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
    table = g.flat_cameras()
    g.optimize(niter)
    out = dict(stats=g.stats(), pose=g.poses(), lm=g.landmarks(), nedges=g.n_active_edges(), table=table,
               n_rig=g.n_rig_cameras())
    if keep:
        out["g"] = g
    else:
        g.close()
    return out


def assert_trajectories_match(stats, tr, tol, check_trials=True):
    assert len(stats) == len(tr), (len(stats), len(tr))
    for s, t, tl in zip(stats, tr, tol if isinstance(tol, list) else [tol] * len(tr)):
        print("it %d chi2 %.12g ref %.12g rel %.3g (tol %.3g) trials %d/%d" %
              (t["iteration"], s["chi2"], t["chi2"], abs(s["chi2"] - t["chi2"]) / abs(t["chi2"]), tl, s["trials"], t["trials"]))
        assert abs(s["chi2"] - t["chi2"]) <= tl * abs(t["chi2"])
        if check_trials:
            assert s["trials"] == t["trials"]


@pytest.mark.parametrize("name", ["rig3", "mixed", "scale"])
def test_lm_trajectory_matches_the_reference(name):
    d, niter, tr, pose, lm, tol, etol = reference(name)
    assert len(tr) == niter
    out = run(name)
    assert out["nedges"] == len(d["e_pose"])
    assert out["table"]["has_rig"] and out["n_rig"] == len(d["sensors"])
    # the flattened table: one entry per (camera, sensor pose) pair of the recipe, first-seen order
    first = [int(np.flatnonzero((d["e_camera"] == c) & (d["e_stereo"] == s))[0]) for s in (0, 1) for c in range(len(d["sensors"]))
             if np.any((d["e_camera"] == c) & (d["e_stereo"] == s))]
    assert len(out["table"]["cams"]) == len(first)
    for k, i in enumerate(first):
        assert np.array_equal(out["table"]["cams"][k], d["e_cam"][i])
        assert np.array_equal(out["table"]["ext"][k], rig_ref.quat_to_ext(d["e_sensor"][i]))
    assert_trajectories_match(out["stats"], tr, tol)
    np.testing.assert_allclose(out["pose"], pose, rtol=0, atol=etol)
    np.testing.assert_allclose(out["lm"], lm, rtol=0, atol=10 * etol)
    if name == "scale":
        # the start is 20 % too large and the edges are mono edges: the lever arms bring the scale back.  (Checked on the
        # CPU: the reference is at 1.0003 after these 11 iterations, chi2 83 -> 1.7e-4 without a rejected trial; three
        # iterations more take it to 1 + 3e-9 and chi2 to 1e-14, where a relative chi2 comparison says nothing.)
        s0, s_ref, s_got = scale_of(d, d["lm"]), scale_of(d, lm), scale_of(d, out["lm"])
        print("scale: start %.4f, reference %.8f, optimiser %.8f" % (s0, s_ref, s_got))
        assert abs(s0 - 1.2) < 1e-6 and abs(s_ref - 1) < 1e-3 and abs(s_got - s_ref) <= 10 * etol


SETS_PROGRAM = r"""
// a caller of the mirrored public headers: a rig as ONE EDGE SET PER PHYSICAL CAMERA (MonoEdgeSet / StereoEdgeSet by the
// set's dim), each with its own camera and sensor pose, all on the same pose vertices; optimised on the GPU
#include "ba_types.h"
#include "cuda_graph_optimisation.h"
#include <cstdio>
#include <deque>
#include <memory>
#include <vector>
int main(int argc, char** argv)
{
    std::FILE* f = argc > 1 ? std::fopen(argv[1], "r") : nullptr;
    int P, L, n_sets, niter;
    if (!f || std::fscanf(f, "%d %d %d %d", &P, &L, &n_sets, &niter) != 4) return 2;
    cugo::PoseVertexSet poses(false);
    cugo::LandmarkVertexSet lms(true);
    std::deque<cugo::PoseVertex> ps;
    std::deque<cugo::LandmarkVertex> ls;
    for (int i = 0; i < P; i++)
    {
        int fixed;
        double v[7];
        if (std::fscanf(f, "%d", &fixed) != 1) return 2;
        for (double& x : v) if (std::fscanf(f, "%lf", &x) != 1) return 2;
        ps.emplace_back(i, cugo::Se3D(v, v + 4), fixed != 0);
        poses.addVertex(&ps.back());
    }
    for (int j = 0; j < L; j++)
    {
        int fixed;
        double v[3];
        if (std::fscanf(f, "%d", &fixed) != 1) return 2;
        for (double& x : v) if (std::fscanf(f, "%lf", &x) != 1) return 2;
        ls.emplace_back(j, cugo::Vec3d(v), fixed != 0);
        lms.addVertex(&ls.back());
    }
    cugo::GraphOptimisationOptions o;
    o.perEdgeInformation = true;
    o.perEdgeCamera = false;
    cugo::CudaGraphOptimisationImpl opt(o);
    opt.addVertexSet(&poses);
    opt.addVertexSet(&lms);
    std::vector<std::unique_ptr<cugo::MonoEdgeSet>> monos;
    std::vector<std::unique_ptr<cugo::StereoEdgeSet>> stereos;
    std::deque<cugo::MonoEdge> me;
    std::deque<cugo::StereoEdge> se;
    for (int s = 0; s < n_sets; s++)
    {
        int dim, rk, n;
        double delta, c[5], q[7];
        if (std::fscanf(f, "%d %d %lf", &dim, &rk, &delta) != 3) return 2;
        for (double& x : c) if (std::fscanf(f, "%lf", &x) != 1) return 2;
        for (double& x : q) if (std::fscanf(f, "%lf", &x) != 1) return 2;
        if (std::fscanf(f, "%d", &n) != 1) return 2;
        const auto kernel = rk == 3 ? cugo::RobustKernelType::Huber : rk == 1 ? cugo::RobustKernelType::Cauchy
                            : rk == 2 ? cugo::RobustKernelType::Tukey : cugo::RobustKernelType::None;
        cugo::BaseEdgeSet* set;
        if (dim == 2)
            monos.emplace_back(new cugo::MonoEdgeSet), set = monos.back().get();
        else
            stereos.emplace_back(new cugo::StereoEdgeSet), set = stereos.back().get();
        set->setCamera(cugo::Camera(c[0], c[1], c[2], c[3], c[4]));
        set->setSensorPose(cugo::Se3D(q, q + 4));
        set->setRobustKernel(kernel, delta);
        for (int e = 0; e < n; e++)
        {
            int ip, il;
            double m[3], w;
            if (std::fscanf(f, "%d %d %lf %lf %lf %lf", &ip, &il, &m[0], &m[1], &m[2], &w) != 6) return 2;
            if (dim == 2)
            {
                me.emplace_back();
                me.back().setVertex(&ps[(size_t)ip], 0), me.back().setVertex(&ls[(size_t)il], 1);
                me.back().setMeasurement(cugo::Vec2d(m));
                me.back().setInformation(w);
                set->addEdge(&me.back());
            }
            else
            {
                se.emplace_back();
                se.back().setVertex(&ps[(size_t)ip], 0), se.back().setVertex(&ls[(size_t)il], 1);
                se.back().setMeasurement(cugo::Vec3d(m));
                se.back().setInformation(w);
                set->addEdge(&se.back());
            }
        }
        opt.addEdgeSet(set);
    }
    std::fclose(f);
    opt.initialize();
    std::vector<double> c5, x12;
    const bool rig = opt.flatCameras(c5, x12);
    std::printf("table %d %d", rig ? 1 : 0, opt.nRigCameras());
    for (double x : c5) std::printf(" %a", x);
    for (double x : x12) std::printf(" %a", x);
    std::printf("\n");
    opt.optimize(niter);
    std::printf("chi2");
    for (const auto& b : opt.batchStatistics().get()) std::printf(" %a", b.chi2);
    std::printf("\ntrials");
    for (const auto& t : opt.lmTrace()) std::printf(" %d", t.trials);
    std::printf("\npose");
    for (auto& v : ps)
    {
        double e[7];
        v.getEstimate().copyTo(e, e + 4);
        for (double x : e) std::printf(" %a", x);
    }
    std::printf("\nlm");
    for (auto& v : ls)
    {
        double e[3];
        v.getEstimate().copyTo(e);
        for (double x : e) std::printf(" %a", x);
    }
    std::printf("\nOK\n");
    return 0;
}
"""


def sets_input(d, niter):
    """the recipe as one edge set per camera of the rig, in camera order: `P L n_sets niter`, the vertices, then per set
    `dim rk delta cam5 sensor7 n` and its edges `pose lm u v third omega`"""
    fl = lambda a: " ".join("%.17g" % x for x in a)
    lines = ["%d %d %d %d" % (len(d["pose"]), len(d["lm"]), len(d["sensors"]), niter)]
    lines += ["%d %s" % (f, fl(p)) for p, f in zip(d["pose"], d["pose_fixed"])]
    lines += ["%d %s" % (f, fl(x)) for x, f in zip(d["lm"], d["lm_fixed"])]
    for c in range(len(d["sensors"])):
        sel = np.flatnonzero(d["e_camera"] == c)
        st = int(d["e_stereo"][sel[0]])
        assert np.all(d["e_stereo"][sel] == st) and np.all(d["e_cam"][sel] == d["e_cam"][sel[0]])
        rk = d["rk2"][st]
        lines.append("%d %d %.17g %s %s %d" % (3 if st else 2, rk[0], rk[1], fl(d["e_cam"][sel[0]]), fl(d["sensors"][c]), len(sel)))
        lines += ["%d %d %s %.17g" % (d["e_pose"][i], d["e_lm"][i], fl(d["e_meas"][i]), d["e_omega"][i]) for i in sel]
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("name", ["rig3", "mixed"])
def test_one_edge_set_per_camera_gives_the_per_edge_table_and_trajectory(name, tmp_path):
    """the two-camera mono rig with a stereo camera on a third entry, built from SETS through the C++ interface — two
    MonoEdgeSets and a StereoEdgeSet with their own sensor poses on the same pose vertices — against the same rig
    through one mono and one stereo set with per-edge cameras: the same flattened table, the same trajectory (a
    landmark's edges are one camera's, so the landmark-major slots hold the same edges in the same order: bit for
    bit), and both against the reference"""
    d, niter, tr, pose, lm, tol, etol = reference(name)
    per_edge = run(name)
    (tmp_path / "rig.txt").write_text(sets_input(d, niter))
    src, exe = tmp_path / "rig_sets.cpp", tmp_path / "rig_sets"
    src.write_text(SETS_PROGRAM)
    lib_dir = os.path.dirname(cugo.LIB_PATH)
    c = subprocess.run(["g++", "-std=c++17", "-O1", "-I", INC, str(src), "-L", lib_dir, "-lcugo_hip", "-Wl,-rpath," + lib_dir,
                        "-o", str(exe)], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-3000:]
    p = subprocess.run([str(exe), str(tmp_path / "rig.txt")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    rows = {ln.split()[0]: ln.split()[1:] for ln in p.stdout.splitlines() if ln.strip()}
    hexes = lambda k, a=0: np.array([float.fromhex(x) for x in rows[k][a:]])
    # the table: three entries, all of them sensor poses, entry for entry that of the per-edge graph
    n = len(d["sensors"])
    assert rows["table"][:2] == ["1", str(n)]
    table = hexes("table", 2)
    assert len(table) == 17 * n
    assert np.array_equal(table[:5 * n].reshape(n, 5), per_edge["table"]["cams"])
    assert np.array_equal(table[5 * n:].reshape(n, 12), per_edge["table"]["ext"])
    # the trajectory: the per-edge graph's, and the reference's
    chi, trials = hexes("chi2"), [int(x) for x in rows["trials"]]
    stats = [dict(chi2=float(x), trials=t) for x, t in zip(chi, trials)]
    assert_trajectories_match(stats, tr, tol)
    assert [s["chi2"] for s in per_edge["stats"]] == list(chi) and [s["trials"] for s in per_edge["stats"]] == trials
    got_pose, got_lm = hexes("pose").reshape(-1, 7), hexes("lm").reshape(-1, 3)
    assert np.array_equal(got_pose, per_edge["pose"]) and np.array_equal(got_lm, per_edge["lm"])
    np.testing.assert_allclose(got_pose, pose, rtol=0, atol=etol)
    np.testing.assert_allclose(got_lm, lm, rtol=0, atol=10 * etol)


def test_set_level_sensor_poses_give_the_per_edge_trajectory():
    """one camera per kind: the sets' sensor poses (no per-edge cameras) against the same graph through per-edge
    cameras — the same table and the same trajectory, bit for bit"""
    d = G.make_rig_problem(RIG3[1:], (0, 1), seed=47)
    d = dict(d, rk2={0: NONE, 1: (3, 1.5)})
    outs = []
    for per_edge in (True, False):
        g = build_graph(d, per_edge=per_edge)
        g.initialize()
        t = g.flat_cameras()
        g.optimize(5)
        outs.append((t, g.stats(), g.poses(), g.landmarks()))
        g.close()
    a, b = outs
    assert a[0]["has_rig"] and np.array_equal(a[0]["cams"], b[0]["cams"]) and np.array_equal(a[0]["ext"], b[0]["ext"])
    assert [(s["chi2"], s["trials"]) for s in a[1]] == [(s["chi2"], s["trials"]) for s in b[1]]
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    tr, pose, lm, sens, est = G.reference_runs(d, 5)
    tol, etol = R.tolerances(sens, est)
    assert_trajectories_match(a[1], tr, tol)


FORMS = ["CUGO_POSE_SCHUR=0", "CUGO_BS_RECORDS=0", "CUGO_TRIAL_FROM_BUILD=0", "CUGO_SCHUR_PLAN=1", "CUGO_HSC_MFMA=0"]


@pytest.mark.parametrize("form", FORMS)
def test_forms_of_the_loop_take_rig_graphs(form, monkeypatch):
    d, niter, tr, pose, lm, tol, etol = reference("mixed")
    base = run("mixed")
    var, val = form.split("=")
    monkeypatch.setenv(var, val)
    out = run("mixed")
    assert_trajectories_match(out["stats"], tr, tol)
    np.testing.assert_allclose(out["pose"], pose, rtol=0, atol=etol)
    np.testing.assert_allclose(out["lm"], lm, rtol=0, atol=10 * etol)
    if var in ("CUGO_BS_RECORDS", "CUGO_TRIAL_FROM_BUILD"):
        assert [(s["chi2"], s["lam"], s["trials"]) for s in out["stats"]] == [(s["chi2"], s["lam"], s["trials"]) for s in base["stats"]]
        assert np.array_equal(out["pose"], base["pose"]) and np.array_equal(out["lm"], base["lm"])


def test_float32_internal_mode_with_rig_graphs():
    """float block storage: the bar tests/test_prior_graph.py states for the mode (chi2 to 1e-5, the same trials)"""
    d, niter, tr, pose, lm, tol, etol = reference("mixed")
    out = run("mixed", float32=True)
    assert_trajectories_match(out["stats"], tr, 1e-5, check_trials=False)
    assert [s["trials"] for s in out["stats"]] == [t["trials"] for t in tr]


def test_outlier_rejection_on_a_rig_set_agrees_with_the_reference():
    """a tenth of the side camera's measurements off by 30 px; the verdicts of the reference at ITS final estimates with
    a margin round the threshold (no edge of the reference within 1 % of it)"""
    d, niter = case("rig3")
    rng = np.random.default_rng(5)
    mono = np.flatnonzero(d["e_stereo"] == 0)
    side = np.flatnonzero((d["e_stereo"] == 0) & (d["e_camera"] == 1))
    bad = side[rng.random(len(side)) < 0.1]
    meas = d["e_meas"].copy()
    meas[bad, 0] += 30.0
    d = dict(d, e_meas=meas)
    ref = G.RigGraph(d)
    ref.optimize(niter)
    chi = ref.edge_chi()[mono]
    threshold = 28.0                # (the reference's chi2 terms next to it: 25.3 and 30.7)
    assert np.all(np.abs(chi - threshold) > 0.01 * threshold), "an edge of the reference sits on the threshold"
    verdict = chi > threshold
    assert 2 <= verdict.sum() < len(mono) // 2
    out = run((d, niter), keep=True, threshold=threshold)
    g = out["g"]
    assert np.array_equal(~g.edge_active(2, len(mono)), verdict)
    assert g.n_outliers(2) == verdict.sum() and g.n_outliers(3) == 0
    g.initialize()
    assert g.n_active_edges() == len(d["e_pose"]) - verdict.sum()
    g.close()


def test_covariances_match_the_dense_inverse():
    """the rule of tests/test_covariance.py (1e-8 of the block norm) against the inverse of the reference's undamped
    system at the optimiser's estimates"""
    d, niter = case("mixed")
    out = run("mixed", keep=True)
    g = out["g"]
    g.compute_covariances()
    ref = G.RigGraph(d)
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


def test_body_frame_priors_and_relative_pose_edges_next_to_rig_edges():
    """a PosePriorEdgeSet and a RelPoseEdgeSet act on the pose vertex, which is now the body: measured in the body
    frame, next to rig BA edges; trajectory against the reference"""
    d, niter = case("rig3")
    rng = np.random.default_rng(9)
    gt = d["pose_gt"]
    prior = PR.make_prior([3, 6], [PR.displaced(rng, gt[p], 0.01, 0.05) for p in (3, 6)], [PR.random_spd(rng, 50.0) for _ in range(2)])
    pairs = [(i, i + 1) if i % 2 == 0 else (i + 1, i) for i in range(len(gt) - 1)]
    rp = RL.edges_between(rng, gt, pairs, 0.005, 0.02, 200.0, rk=(RR.RK_CAUCHY, 5.0))
    make = lambda dd, vs: G.RigRelPoseGraph(dd, [], prior, rp, via_schur=vs)
    tr, pose, lm, sens, est = G.reference_runs(d, niter, make)
    tol, etol = R.tolerances(sens, est)

    def extra(g):
        PR.add_priors(g, prior)
        RL.add_relpose(g, rp)

    out = run((d, niter), extra=extra)
    assert_trajectories_match(out["stats"], tr, tol)
    np.testing.assert_allclose(out["pose"], pose, rtol=0, atol=etol)
    np.testing.assert_allclose(out["lm"], lm, rtol=0, atol=10 * etol)
    # and the priors do pull: another trajectory than the BA edges alone
    assert abs(tr[-1]["chi2"] - reference("rig3")[2][-1]["chi2"]) > 1e-3 * tr[-1]["chi2"]


def test_second_initialize_after_estimates_changed_reuses_the_flattening():
    d, niter = case("mixed")
    out = run("mixed", keep=True)
    g = out["g"]
    assert g.flatten_reuses() == 0
    g.set_poses(np.arange(len(d["pose"]), dtype=np.int32), d["pose"])
    g.set_landmarks(np.arange(len(d["lm"]), dtype=np.int32), d["lm"])
    g.initialize()
    assert g.flatten_reuses() == 1 and g.flat_cameras()["has_rig"]
    g.optimize(niter)
    assert [(s["chi2"], s["trials"]) for s in g.stats()] == [(s["chi2"], s["trials"]) for s in out["stats"]]
    assert np.array_equal(g.poses(), out["pose"]) and np.array_equal(g.landmarks(), out["lm"])
    g.close()
