"""CPU tests of the host side of radial-tangential lens distortion (no GPU): the flattened distortion table of a
plan-only Graph next to cameras and sensor poses, the de-duplication key (5 + 7 + 5 + 5 numbers), has_rig = 3 with
identity sensor poses and an unchanged table without distortion, flatten re-use at set level and — through a C++ caller
of the mirrored headers with one MonoEdgeSet per distorted camera — at edge level, the refusals of initialize() and of
the predicted observations with their messages, the exported symbols, and the truth table of the edge form for
has_rig = 3."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import rig_ref as rr
import test_rig_host as trh

cugo = importlib.import_module("cuda-bundle-adjustment_amd")

ROOT = trh.ROOT
INC = trh.INC
CAM, IDENT, S1, S2 = trh.CAM, trh.IDENT, trh.S1, trh.S2
D1 = np.array([-0.28, 0.07, 0.002, -0.001, -0.01])
D2 = np.array([-0.28, 0.07, 0.002, -0.001, -0.015])         # differs from D1 in k3 alone
NONE = np.zeros(5)
KB = np.array([-0.0131, 0.0212, -0.0071, 0.0012])


def graph(d, per_edge_camera, sensor=None, cams=None, dist=None, stereo_sel=None, depth_sel=None, model=None):
    """test_rig_host.graph with a distortion per edge (dist [n][5] or None) or a model per edge"""
    g = cugo.Graph(True, per_edge_camera, plan_only=True)
    g.add_poses(np.arange(4, dtype=np.int32), d["pose"], np.array([1, 0, 0, 0], np.uint8))
    g.add_landmarks(np.arange(12, dtype=np.int32), d["lm"], np.zeros(12, np.uint8))
    n = len(d["ep"])
    st = np.zeros(n, bool) if stereo_sel is None else stereo_sel
    dp = np.zeros(n, bool) if depth_sel is None else depth_sel
    for dim, sel in ((2, ~st & ~dp), (3, st)):
        g.add_edges(dim, d["ep"][sel], d["el"][sel], d["meas"][sel], np.ones(int(sel.sum())),
                    None if cams is None else cams[sel], None if sensor is None else sensor[sel],
                    model=None if model is None else model[sel], distortion=None if dist is None else dist[sel])
    if dp.any():
        g.add_depth_edges(d["ep"][dp], d["el"][dp], d["meas"][dp] * np.array([1, 1, 1e-4]), np.ones(int(dp.sum())))
        g.set_depth_camera(CAM)
    g.set_camera(2, CAM)
    g.set_camera(3, CAM)
    return g


def test_distortions_flatten_beside_cameras_and_sensor_poses():
    d = trh.problem()
    n = 48
    sensor = np.stack([IDENT, S1])[np.arange(n) % 2]
    dist = np.stack([NONE, D1, D2])[np.arange(n) % 3]
    g = graph(d, True, sensor, np.tile(CAM, (n, 1)), dist)
    g.initialize()
    t, m = g.flat_cameras(), g.flat_camera_distortions()
    # six distinct (sensor pose, distortion) pairs in first-seen order: edge i has pair (i % 2, i % 3)
    seen = []
    for i in range(n):
        if (i % 2, i % 3) not in seen:
            seen.append((i % 2, i % 3))
    assert len(t["cams"]) == 6 and m.shape == (6, 5) and g.n_distorted_cameras() == 4 and g.n_rig_cameras() == 3
    assert g.n_fisheye_cameras() == 0 and np.all(g.flat_camera_models() == 0)
    for k, (a, b) in enumerate(seen):
        assert np.array_equal(t["ext"][k], rr.quat_to_ext((IDENT, S1)[a]))
        assert np.array_equal(m[k], (NONE, D1, D2)[b])
    g.close()


def test_the_key_covers_the_distortion():
    d = trh.problem()
    n = 48
    cams, sensor = np.tile(CAM, (n, 1)), np.tile(S1, (n, 1))
    for dists, want, nd in (((NONE, NONE), 1, 0), ((NONE, D1), 2, 1), ((D1, D2), 2, 2), ((D1, D1), 1, 1),
                            ((NONE, -NONE), 1, 0)):                        # a zero of either sign is a zero
        dist = np.stack(dists)[np.arange(n) % 2]
        g = graph(d, True, sensor, cams, dist)
        g.initialize()
        assert len(g.flat_cameras()["cams"]) == want and g.n_distorted_cameras() == nd, (dists, want)
        g.close()
    # zeros given against nothing given: one entry, and the tables of a graph that never heard of distortion
    a = graph(d, True, sensor, cams)
    b = graph(d, True, sensor, cams, np.tile(NONE, (n, 1)))
    a.initialize(), b.initialize()
    ta, tb = a.flat_cameras(), b.flat_cameras()
    assert len(ta["cams"]) == 1 and np.array_equal(ta["cams"], tb["cams"]) and np.array_equal(ta["ext"], tb["ext"])
    assert a.n_distorted_cameras() == 0 and b.n_distorted_cameras() == 0
    assert np.array_equal(a.flat_camera_distortions(), np.zeros((1, 5))) and np.array_equal(b.flat_camera_distortions(), np.zeros((1, 5)))
    a.close(), b.close()


def test_has_rig_is_3_iff_some_distortion_is_not_zero():
    """a distortion makes the kernels take the distortion table even when every sensor pose is the identity; the tables
    of cugo_graph_get_flat_cameras keep their shapes (its has_rig keeps saying whether a sensor pose is not the identity)"""
    d = trh.problem()
    g = graph(d, False)
    g.set_camera_distortion(2, D1)
    g.initialize()
    t, m = g.flat_cameras(), g.flat_camera_distortions()
    assert g.n_distorted_cameras() == 1 and g.n_rig_cameras() == 0 and not t["has_rig"]
    assert t["ext"].shape == (1, 12) and np.all(t["ext"] == rr.IDENTITY12[None, :]) and np.array_equal(m, D1[None, :])
    g.set_camera_distortion(2, None)                      # back to zeros: no table at all
    g.initialize()
    assert g.n_distorted_cameras() == 0 and np.all(g.flat_camera_distortions() == 0)
    g.close()
    # without per-edge cameras the set's distortion applies and a per-edge one is not looked at
    n = 48
    g = graph(d, False, None, np.tile(CAM, (n, 1)), np.tile(D1, (n, 1)))
    g.initialize()
    assert g.n_distorted_cameras() == 0
    g.set_camera_distortion(2, D1)
    g.initialize()
    assert g.n_distorted_cameras() == 1
    g.close()


def test_flat_camera_distortions_is_parallel_to_flat_cameras():
    d = trh.problem()
    n = 48
    cams = np.tile(CAM, (n, 1))
    cams[np.arange(n) % 2 == 1] *= 1.01
    dist = np.stack([D1, NONE, D2])[np.arange(n) % 3]
    g = graph(d, True, None, cams, dist)
    g.initialize()
    t, m = g.flat_cameras(), g.flat_camera_distortions()
    assert len(t["cams"]) == 6 and m.shape == (6, 5) and not t["has_rig"] and g.n_distorted_cameras() == 4
    for k in range(6):                                   # entry k is the pair of the first edge that carries it: edge k
        assert np.array_equal(t["cams"][k], cams[k]) and np.array_equal(m[k], dist[k])
    g.close()


def test_flatten_reuse_notices_a_changed_coefficient_of_the_set():
    d = trh.problem()
    g = graph(d, False)
    g.set_camera_distortion(2, D1)
    g.initialize()
    g.initialize()
    assert g.flatten_reuses() == 1
    g.set_camera_distortion(2, D2)
    g.initialize()
    assert g.flatten_reuses() == 1, "a changed coefficient must count as a change of the set"
    assert np.array_equal(g.flat_camera_distortions(), D2[None, :])
    g.initialize()
    assert g.flatten_reuses() == 2
    g.close()


def test_distortion_on_stereo_edges_is_refused():
    d = trh.problem()
    g = graph(d, False, stereo_sel=np.arange(48) % 2 == 1)
    g.initialize()
    g.set_camera_distortion(3, D1)
    with pytest.raises(cugo.CugoError, match="lens distortion .*on a stereo edge set is not supported"):
        g.initialize()
    g.set_camera_distortion(3, None)
    g.set_camera_distortion(2, D1)                             # distorted mono next to rectified stereo: fine
    g.initialize()
    assert g.n_distorted_cameras() == 1 and len(g.flat_cameras()["cams"]) == 2
    g.close()
    # per edge
    n = 48
    st = np.arange(n) % 2 == 1
    g = graph(d, True, None, np.tile(CAM, (n, 1)), np.tile(D1, (n, 1)), stereo_sel=st)
    with pytest.raises(cugo.CugoError, match="lens distortion .*on a stereo edge set is not supported"):
        g.initialize()
    g.close()


def test_distortion_with_a_depth_set_is_refused():
    d = trh.problem()
    g = graph(d, False, depth_sel=np.arange(48) % 3 == 0)
    g.initialize()
    g.set_camera_distortion(2, D1)
    with pytest.raises(cugo.CugoError, match="lens distortion .*together with depth edge sets is not supported yet"):
        g.initialize()
    g.close()


def test_distortion_on_a_kannala_brandt_camera_is_refused():
    d = trh.problem()
    g = graph(d, False)
    g.set_camera_model(2, 1, KB)
    g.set_camera_distortion(2, D1)
    with pytest.raises(cugo.CugoError, match="lens distortion .*on a Kannala-Brandt camera"):
        g.initialize()
    g.set_camera_distortion(2, None)
    g.initialize()
    assert g.n_fisheye_cameras() == 1 and g.n_distorted_cameras() == 0
    g.close()


def test_distorted_and_kannala_brandt_cameras_in_one_graph_are_refused():
    d = trh.problem()
    n = 48
    odd = np.arange(n) % 2 == 1
    dist = np.where(odd[:, None], D1[None, :], NONE[None, :])
    g = cugo.Graph(True, True, plan_only=True)
    g.add_poses(np.arange(4, dtype=np.int32), d["pose"], np.array([1, 0, 0, 0], np.uint8))
    g.add_landmarks(np.arange(12, dtype=np.int32), d["lm"], np.zeros(12, np.uint8))
    cams = np.tile(CAM, (n, 1))
    g.add_edges(2, d["ep"][odd], d["el"][odd], d["meas"][odd], np.ones(int(odd.sum())), cams[odd], distortion=dist[odd])
    g.add_edges(2, d["ep"][~odd], d["el"][~odd], d["meas"][~odd], np.ones(int((~odd).sum())), cams[~odd],
                model=np.tile(np.concatenate([KB, [1.0]]), (int((~odd).sum()), 1)))
    with pytest.raises(cugo.CugoError, match="lens distortion .*and Kannala-Brandt cameras in one graph are not supported yet"):
        g.initialize()
    g.close()
    with pytest.raises(cugo.CugoError, match="distortion and model do not go together"):
        graph(d, True, None, cams, dist, model=np.zeros((n, 5)))


def test_distortion_on_a_sharded_optimiser_is_refused():
    g = graph(trh.problem(), False)
    g.set_camera_distortion(2, D1)
    g.set_shard(0, 2, lambda ptr, n, op: None)
    with pytest.raises(cugo.CugoError, match="lens distortion .*not supported on a landmark-sharded"):
        g.initialize()
    g.close()


@pytest.mark.parametrize("bad", [np.array([np.nan, 0, 0, 0, 0.0]), np.array([0, 0, np.inf, 0, 0.0]), np.array([0, 0, 0, 0, -np.inf])])
def test_coefficients_that_are_not_finite_are_refused(bad):
    g = graph(trh.problem(), False)
    g.set_camera_distortion(2, bad)
    with pytest.raises(cugo.CugoError, match="lens distortion .*coefficients k1, k2, p1, p2, k3 must be finite"):
        g.initialize()
    g.set_camera_distortion(2, D1)
    g.initialize()
    g.close()
    with pytest.raises(cugo.CugoError, match="d5 must hold 5 numbers"):
        graph(trh.problem(), False).set_camera_distortion(2, D1[:4])


def test_predicted_observations_refuse_the_distorted_camera_of_a_set():
    """cam=None takes the camera from the set: with a distortion there the answer would be that of another camera"""
    g = graph(trh.problem(), False)
    g.set_camera_distortion(2, D1)
    g.initialize()
    with pytest.raises(cugo.CugoError, match="lens distortion .*predicted observations do not model yet"):
        g.predict_observations([1], [0], cugo.OBS_MONO)
    g.close()


def test_symbols_are_exported_and_declared():
    L = cugo.lib()
    header = open(os.path.join(ROOT, "include", "cugo_hip.h")).read()
    for name in ("cugo_graph_set_camera_distortion", "cugo_graph_add_edges_distorted", "cugo_graph_n_distorted_cameras",
                 "cugo_graph_get_flat_camera_distortions"):
        assert hasattr(L, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name + " is not declared in cugo_hip.h"
    for name, value in (("CUGO_RIG_DISTORTION", 3), ("CUGO_DIST_TAB_STRIDE", 18), ("CUGO_RIG_MODELS", 2), ("CUGO_CAM_TAB_STRIDE", 17)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name
    assert (cugo.RIG_DISTORTION, cugo.DIST_TAB_STRIDE) == (3, 18)
    # the struct has not grown
    assert re.search(r"double depth_weight;.*?int has_rig;[^;]*const double\* d_cam_ext;[^;]*\}\s*cugo_edges;", header, re.S)
    assert C.sizeof(cugo.RigEdges) == C.sizeof(cugo.Edges) + 16
    for m in ("set_camera_distortion", "n_distorted_cameras", "flat_camera_distortions"):
        assert hasattr(cugo.Graph, m), m
    tab = cugo.distortion_table(np.stack([rr.quat_to_ext(S1), rr.IDENTITY12, rr.IDENTITY12]), np.stack([D1, NONE, D2]))
    assert tab.shape == (3, 18) and np.array_equal(tab[0, :12], rr.quat_to_ext(S1)) and np.array_equal(tab[0, 12:17], D1)
    assert np.array_equal(tab[:, 17], [1.0, 0.0, 1.0])
    assert np.array_equal(cugo.distortion_table(None, D2[None, :])[0, :12], rr.IDENTITY12)
    assert np.array_equal(cugo.distortion_table(None, np.stack([D1, D2]), flags=[0, 1])[:, 17], [0.0, 1.0])
    with pytest.raises(cugo.CugoError):
        cugo.distortion_table(None, D1[None, :], flags=[2.0])


PROGRAM = r"""
// a caller of the mirrored public headers with a two-camera rig of distorted cameras: one MonoEdgeSet per camera
#include "ba_types.h"
#include "camera_distortion.h"
#include "cuda_graph_optimisation.h"
#include <cmath>
#include <cstdio>
#include <deque>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
static bool refused(cugo::CudaGraphOptimisationImpl& opt, const char* needle)
{
    try { opt.initialize(); }
    catch (const std::runtime_error& e) { return std::string(e.what()).find(needle) != std::string::npos; }
    return false;
}
int main()
{
    cugo::GraphOptimisationOptions options;
    options.planOnly = true;
    options.perEdgeCamera = false;
    cugo::CudaGraphOptimisationImpl opt(options);
    cugo::PoseVertexSet poses(false);
    cugo::LandmarkVertexSet lms(true);
    std::deque<cugo::PoseVertex> ps;
    std::deque<cugo::LandmarkVertex> ls;
    const double q[4] = {0, 0, 0, 1};
    for (int i = 0; i < 3; i++)
    {
        const double t[3] = {0.5 * i, 0, 0};
        ps.emplace_back(i, cugo::Se3D(q, t), i == 0);
        poses.addVertex(&ps.back());
    }
    for (int j = 0; j < 7; j++)
    {
        const double x[3] = {j - 2.5, 0.3 * j, 10.0 + j};
        ls.emplace_back(j, cugo::Vec3d(x), false);
        lms.addVertex(&ls.back());
    }
    cugo::MonoEdgeSet front, side;
    const cugo::Camera cam(300.0, 300.0, 600.0, 180.0, 0.0);
    front.setCamera(cam), side.setCamera(cam);
    front.setInformation(1.0), side.setInformation(1.0);
    const double qs[4] = {0, 0.7071067811865476, 0, 0.7071067811865476}, tsd[3] = {-0.4, 0.0, 0.0};
    side.setSensorPose(cugo::Se3D(qs, tsd));
    CHECK(front.distortionData().isZero() && cugo::CameraDistortion().isZero());                       // the default
    const cugo::CameraDistortion dFront(-0.28, 0.07, 0.002, -0.001, -0.01);
    cugo::CameraDistortion dSide = dFront;
    dSide.k3 = -0.015;
    CHECK(!dFront.isZero() && !cugo::CameraDistortion(0, 0, 0, 0, std::numeric_limits<double>::quiet_NaN()).isZero());
    front.setDistortion(dFront), side.setDistortion(dSide);
    std::deque<cugo::MonoEdge> es;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 6; j++)
        {
            es.emplace_back();
            cugo::MonoEdge& e = es.back();
            e.setVertex(&ps[i], 0), e.setVertex(&ls[j], 1);
            const double m[2] = {600.0 + 10 * j, 180.0 + i};
            e.setMeasurement(cugo::Vec2d(m));
            e.setInformation(1.0);
            (j % 2 ? side : front).addEdge(&e);
        }
    opt.addVertexSet(&poses);
    opt.addVertexSet(&lms);
    opt.addEdgeSet(&front);
    opt.addEdgeSet(&side);
    opt.initialize();
    std::vector<double> c5, x12, d5, m5;
    CHECK(opt.flatCameras(c5, x12) && c5.size() == 10 && x12.size() == 24);
    CHECK(opt.flatCameraDistortions(d5) && d5.size() == 10 && opt.nDistortedCameras() == 2 && opt.nRigCameras() == 1);
    CHECK(!opt.flatCameraModels(m5) && opt.nFisheyeCameras() == 0);
    CHECK(d5[0] == -0.28 && d5[2] == 0.002 && d5[4] == -0.01 && d5[5 + 3] == -0.001 && d5[5 + 4] == -0.015);
    opt.initialize();
    CHECK(opt.flattenReuses() == 1);
    // set level: a mutable reference counts as a change
    side.getDistortion().k1 = -0.2;
    opt.initialize();
    CHECK(opt.flattenReuses() == 1 && opt.flatCameraDistortions(d5) && d5[5] == -0.2);
    // edge level: only with per-edge cameras is an edge's distortion looked at, but a change is a change
    opt.initialize();
    CHECK(opt.flattenReuses() == 2);
    es[1].setDistortion(dSide);
    opt.initialize();
    CHECK(opt.flattenReuses() == 2 && opt.nDistortedCameras() == 2);
    opt.initialize();
    CHECK(opt.flattenReuses() == 3);
    es[2].getDistortion();
    opt.initialize();
    CHECK(opt.flattenReuses() == 3);
    // both sets back to zeros: no distortion table, the rig as it was
    front.setDistortion(cugo::CameraDistortion()), side.setDistortion(cugo::CameraDistortion());
    opt.initialize();
    CHECK(!opt.flatCameraDistortions(d5) && d5.size() == 10 && d5[0] == 0.0 && opt.nDistortedCameras() == 0 && opt.nRigCameras() == 1);
    front.setDistortion(dFront), side.setDistortion(dSide);
    // coefficients that are not finite are refused with a message
    side.getDistortion().p2 = std::numeric_limits<double>::quiet_NaN();
    CHECK(refused(opt, "coefficients k1, k2, p1, p2, k3 must be finite"));
    side.setDistortion(dSide);
    opt.initialize();
    // a Kannala-Brandt model on a distorted camera, and next to one
    side.setCameraModel(cugo::CameraModel(cugo::KannalaBrandt, 0.01, 0, 0, 0));
    CHECK(refused(opt, "on a Kannala-Brandt camera"));
    side.setDistortion(cugo::CameraDistortion());
    CHECK(refused(opt, "and Kannala-Brandt cameras in one graph are not supported yet"));
    side.setCameraModel(cugo::CameraModel()), side.setDistortion(dSide);
    opt.initialize();
    // a distortion on a stereo set is refused
    cugo::StereoEdgeSet stereo;
    stereo.setCamera(cam);
    stereo.setInformation(1.0);
    cugo::StereoEdge se;
    se.setVertex(&ps[1], 0), se.setVertex(&ls[6], 1);
    const double m3[3] = {600.0, 180.0, 590.0};
    se.setMeasurement(cugo::Vec3d(m3));
    se.setInformation(1.0);
    stereo.addEdge(&se);
    opt.addEdgeSet(&stereo);
    opt.initialize();                                   // a rectified stereo set next to distorted mono sets: fine
    CHECK(opt.flatCameraDistortions(d5) && d5.size() == 15 && opt.nDistortedCameras() == 2);
    stereo.setDistortion(dFront);
    CHECK(refused(opt, "on a stereo edge set is not supported"));
    stereo.setDistortion(cugo::CameraDistortion());
    opt.initialize();
    // a depth set next to distorted cameras is refused ("not yet"), and so is one that carries the distortion itself
    cugo::DepthEdgeSet depth;
    depth.setCamera(cam);
    depth.setInformation(1.0);
    cugo::DepthEdge de;
    de.setVertex(&ps[2], 0), de.setVertex(&ls[6], 1);
    const double md[3] = {600.0, 180.0, 0.1};
    de.setMeasurement(cugo::Vec3d(md));
    de.setInformation(1.0);
    depth.addEdge(&de);
    opt.addEdgeSet(&depth);
    side.setSensorPose(cugo::Se3D());                   // (no rig: the refusal below is the distortion's)
    CHECK(refused(opt, "lens distortion (radial-tangential) together with depth edge sets is not supported yet"));
    front.setDistortion(cugo::CameraDistortion()), side.setDistortion(cugo::CameraDistortion());
    opt.initialize();
    depth.setDistortion(dFront);
    CHECK(refused(opt, "lens distortion (radial-tangential) together with depth edge sets is not supported yet"));
    std::printf("OK\n");
    return 0;
}
"""


def test_a_caller_of_the_mirrored_headers_compiles_and_links(tmp_path):
    src = tmp_path / "distort_caller.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "distort_caller"
    lib_dir = os.path.dirname(cugo.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", INC, str(src), "-L", lib_dir, "-lcugo_hip",
                        "-Wl,-rpath," + lib_dir, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr


EDGE_FORM_PROGRAM = r"""
#include "cugo_hip.h"
#include <cstdio>
#include <stdexcept>
#include <string>
// the library's internal names (csrc/kernels/kernels.h, csrc/host/c_api.cpp)
namespace cugo_k
{
enum class EdgeForm { Plain, Depth, Rig, Models, Distortion };
EdgeForm edge_form(const cugo_edges& ev);
}
namespace cugo_host
{
void check_edge_form(const cugo_edges* ev, const char* who);
}
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #c, what.c_str()); return 1; } } while (0)
int main()
{
    static const double table[18] = {1, 0, 0, 0, 1, 0, 0, 0, 1}; // (a host address: never read)
    int n_forms = 0, n_refused = 0;
    for (int rig = 0; rig <= 8; rig++)
        for (int depth = 0; depth < 2; depth++)
            for (int given = 0; given < 2; given++)
            {
                cugo_edges ev = {};
                ev.has_rig = rig, ev.has_depth = depth, ev.d_cam_ext = given ? table : nullptr;
                ev.depth_weight = 2.0, ev.rk_type_depth = CUGO_RK_NONE;
                std::string what = "has_rig " + std::to_string(rig) + " has_depth " + std::to_string(depth) + " table " +
                                   std::to_string(given);
                std::string refusal;
                if (rig && !given)
                    refusal = ": has_rig needs the extrinsics table d_cam_ext";
                else if (rig && depth)
                    refusal = ": camera extrinsics (has_rig) together with depth slots (has_depth) are not supported yet";
                // 3 is the distortion table, 2 the model table, every other non-zero value the extrinsics
                const cugo_k::EdgeForm form = rig == CUGO_RIG_DISTORTION ? cugo_k::EdgeForm::Distortion
                                              : rig == CUGO_RIG_MODELS   ? cugo_k::EdgeForm::Models
                                              : rig                      ? cugo_k::EdgeForm::Rig
                                              : depth                    ? cugo_k::EdgeForm::Depth
                                                                         : cugo_k::EdgeForm::Plain;
                CHECK(cugo_k::edge_form(ev) == form);
                CHECK((int)cugo_k::EdgeForm::Distortion == 4 && (int)cugo_k::EdgeForm::Models == 3);
                std::string got;
                try { cugo_host::check_edge_form(&ev, "who"); }
                catch (const std::runtime_error& e) { got = e.what(); }
                CHECK(got == (refusal.empty() ? "" : "who" + refusal));
                if (refusal.empty())
                {
                    n_forms++;
                    continue;
                }
                n_refused++;
                const cugo_robust none = {};
                CHECK(cugo_compute_active_errors(nullptr, &ev, nullptr, nullptr, none, nullptr) == CUGO_ERR_INVALID);
                what += std::string(" -> ") + cugo_last_error();
                CHECK(cugo_last_error() == "cugo_compute_active_errors" + refusal);
            }
    std::printf("OK %d forms %d refusals\n", n_forms, n_refused);
    return 0;
}
"""


def test_edge_form_truth_table_with_the_distortion_form(tmp_path):
    """has_rig = 3 gives the new form with a table and the existing refusals without one or with depth slots; every
    other value keeps its form"""
    src = tmp_path / "edge_form_distortion.cpp"
    src.write_text(EDGE_FORM_PROGRAM)
    exe = tmp_path / "edge_form_distortion"
    lib_dir = os.path.dirname(cugo.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-L", lib_dir, "-lcugo_hip",
                        "-Wl,-rpath," + lib_dir, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    # 9 x 2 x 2 = 36 views.  has_rig 0: 4 forms; has_rig 1..8: one form each (table, no depth), three refusals each
    assert "OK 12 forms 24 refusals" in r.stdout, r.stdout
