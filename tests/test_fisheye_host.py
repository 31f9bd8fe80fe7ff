"""CPU tests of the host side of camera models (Kannala-Brandt fisheye; no GPU): the flattened model table of a plan-only
Graph next to cameras and sensor poses, the de-duplication key (5 + 7 + 5 numbers), has_rig = 2 with identity sensor
poses and an unchanged table without models, flatten re-use at set level and — through a C++ caller of the mirrored
headers with one MonoEdgeSet per fisheye camera — at edge level, the refusals of initialize() with their messages, and
the exported symbols."""
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
K1 = np.array([-0.0131, 0.0212, -0.0071, 0.0012])
K2 = np.array([-0.0131, 0.0212, -0.0071, 0.0018])           # differs from K1 in k4 alone
PIN = np.zeros(5)


def kb(k):
    return np.concatenate([k, [1.0]])


def graph(d, per_edge_camera, sensor=None, cams=None, model=None, stereo_sel=None, depth_sel=None):
    """test_rig_host.graph with a model per edge (model [n][5] or None)"""
    g = cugo.Graph(True, per_edge_camera, plan_only=True)
    g.add_poses(np.arange(4, dtype=np.int32), d["pose"], np.array([1, 0, 0, 0], np.uint8))
    g.add_landmarks(np.arange(12, dtype=np.int32), d["lm"], np.zeros(12, np.uint8))
    n = len(d["ep"])
    st = np.zeros(n, bool) if stereo_sel is None else stereo_sel
    dp = np.zeros(n, bool) if depth_sel is None else depth_sel
    for dim, sel in ((2, ~st & ~dp), (3, st)):
        g.add_edges(dim, d["ep"][sel], d["el"][sel], d["meas"][sel], np.ones(int(sel.sum())),
                    None if cams is None else cams[sel], None if sensor is None else sensor[sel],
                    None if model is None else model[sel])
    if dp.any():
        g.add_depth_edges(d["ep"][dp], d["el"][dp], d["meas"][dp] * np.array([1, 1, 1e-4]), np.ones(int(dp.sum())))
        g.set_depth_camera(CAM)
    g.set_camera(2, CAM)
    g.set_camera(3, CAM)
    return g


def test_models_flatten_beside_cameras_and_sensor_poses():
    d = trh.problem()
    n = 48
    sensor = np.stack([IDENT, S1])[np.arange(n) % 2]
    model = np.stack([PIN, kb(K1), kb(K2)])[np.arange(n) % 3]
    g = graph(d, True, sensor, np.tile(CAM, (n, 1)), model)
    g.initialize()
    t, m = g.flat_cameras(), g.flat_camera_models()
    # six distinct (sensor pose, model) pairs in first-seen order: edge i has pair (i % 2, i % 3)
    seen = []
    for i in range(n):
        if (i % 2, i % 3) not in seen:
            seen.append((i % 2, i % 3))
    assert len(t["cams"]) == 6 and m.shape == (6, 5) and g.n_fisheye_cameras() == 4 and g.n_rig_cameras() == 3
    for k, (a, b) in enumerate(seen):
        assert np.array_equal(t["ext"][k], rr.quat_to_ext((IDENT, S1)[a]))
        assert np.array_equal(m[k], (PIN, kb(K1), kb(K2))[b])
    g.close()


def test_the_key_covers_the_model():
    d = trh.problem()
    n = 48
    cams, sensor = np.tile(CAM, (n, 1)), np.tile(S1, (n, 1))
    for models, want, fish in (((PIN, PIN), 1, 0), ((PIN, kb(K1)), 2, 1), ((kb(K1), kb(K2)), 2, 2), ((kb(K1), kb(K1)), 1, 1),
                               ((kb(np.zeros(4)), PIN), 2, 1),            # the equidistant model is not the pinhole
                               ((np.concatenate([K1, [0.0]]), PIN), 1, 0)):    # a pinhole's coefficients are not looked at
        model = np.stack(models)[np.arange(n) % 2]
        g = graph(d, True, sensor, cams, model)
        g.initialize()
        assert len(g.flat_cameras()["cams"]) == want and g.n_fisheye_cameras() == fish, (models, want)
        g.close()


def test_has_rig_is_2_with_identity_sensor_poses():
    """a fisheye model makes the kernels take the model table even when every sensor pose is the identity; the tables
    of cugo_graph_get_flat_cameras keep their shapes (its has_rig keeps saying whether a sensor pose is not the identity)"""
    d = trh.problem()
    g = graph(d, False)
    g.set_camera_model(2, 1, K1)
    g.initialize()
    t, m = g.flat_cameras(), g.flat_camera_models()
    assert g.n_fisheye_cameras() == 1 and g.n_rig_cameras() == 0 and not t["has_rig"]
    assert t["ext"].shape == (1, 12) and np.all(t["ext"] == rr.IDENTITY12[None, :]) and np.array_equal(m, kb(K1)[None, :])
    g.close()


def test_without_models_the_tables_are_what_they_were():
    d = trh.problem()
    n = 48
    sensor = np.stack([IDENT, S1, S2])[np.arange(n) % 3]
    cams = np.tile(CAM, (n, 1))
    cams[np.arange(n) % 2 == 1] *= 1.01
    a = graph(d, True, sensor, cams)
    b = graph(d, True, sensor, cams, np.tile(PIN, (n, 1)))              # pinholes given explicitly
    a.initialize(), b.initialize()
    ta, tb = a.flat_cameras(), b.flat_cameras()
    assert ta["has_rig"] and tb["has_rig"] and np.array_equal(ta["cams"], tb["cams"]) and np.array_equal(ta["ext"], tb["ext"])
    assert a.n_fisheye_cameras() == 0 and b.n_fisheye_cameras() == 0 and np.all(a.flat_camera_models() == 0)
    assert a.flat_camera_models().shape == (6, 5)
    a.close(), b.close()
    # no sensor poses, no models: has_rig 0
    g = graph(d, True, None, cams)
    g.initialize()
    assert not g.flat_cameras()["has_rig"] and g.n_fisheye_cameras() == 0
    g.close()
    # without per-edge cameras the set's model applies and a per-edge one is not looked at
    g = graph(d, False, None, cams, np.tile(kb(K1), (n, 1)))
    g.initialize()
    assert g.n_fisheye_cameras() == 0
    g.set_camera_model(2, 1, K1)
    g.initialize()
    assert g.n_fisheye_cameras() == 1
    g.close()


def test_flatten_reuse_notices_a_changed_coefficient_of_the_set():
    d = trh.problem()
    g = graph(d, False)
    g.set_camera_model(2, 1, K1)
    g.initialize()
    g.initialize()
    assert g.flatten_reuses() == 1
    g.set_camera_model(2, 1, K2)
    g.initialize()
    assert g.flatten_reuses() == 1, "a changed coefficient must count as a change of the set"
    assert np.array_equal(g.flat_camera_models(), kb(K2)[None, :])
    g.initialize()
    assert g.flatten_reuses() == 2
    g.close()


def test_a_fisheye_model_on_stereo_edges_is_refused():
    d = trh.problem()
    g = graph(d, False, stereo_sel=np.arange(48) % 2 == 1)
    g.initialize()
    g.set_camera_model(3, 1, K1)
    with pytest.raises(cugo.CugoError, match="Kannala-Brandt camera model on a stereo edge set is not defined"):
        g.initialize()
    g.set_camera_model(3, 0)
    g.set_camera_model(2, 1, K1)                               # mono fisheye next to pinhole stereo: fine
    g.initialize()
    assert g.n_fisheye_cameras() == 1
    g.close()
    # per edge
    n = 48
    st = np.arange(n) % 2 == 1
    g = graph(d, True, None, np.tile(CAM, (n, 1)), np.tile(kb(K1), (n, 1)), stereo_sel=st)
    with pytest.raises(cugo.CugoError, match="Kannala-Brandt camera model on a stereo edge set is not defined"):
        g.initialize()
    g.close()


def test_a_fisheye_model_with_a_depth_set_is_refused():
    d = trh.problem()
    g = graph(d, False, depth_sel=np.arange(48) % 3 == 0)
    g.initialize()
    g.set_camera_model(2, 1, K1)
    with pytest.raises(cugo.CugoError, match="camera models .*together with depth edge sets are not supported yet"):
        g.initialize()
    g.close()


def test_a_fisheye_model_on_a_sharded_optimiser_is_refused():
    g = graph(trh.problem(), False)
    g.set_camera_model(2, 1, K1)
    g.set_shard(0, 2, lambda ptr, n, op: None)
    with pytest.raises(cugo.CugoError, match="camera models .*not supported on a landmark-sharded"):
        g.initialize()
    g.close()


@pytest.mark.parametrize("bad", [np.array([np.nan, 0, 0, 0.0]), np.array([0, 0, np.inf, 0.0]), np.array([0, -np.inf, 0, 0.0])])
def test_coefficients_that_are_not_finite_are_refused(bad):
    g = graph(trh.problem(), False)
    g.set_camera_model(2, 1, bad)
    with pytest.raises(cugo.CugoError, match="camera model .*coefficients k1..k4 must be finite"):
        g.initialize()
    g.set_camera_model(2, 1, K1)
    g.initialize()
    g.close()
    with pytest.raises(cugo.CugoError, match="model must be 0 .*or 1"):
        graph(trh.problem(), False).set_camera_model(2, 2, K1)


def test_symbols_are_exported_and_declared():
    L = cugo.lib()
    header = open(os.path.join(ROOT, "include", "cugo_hip.h")).read()
    for name in ("cugo_graph_set_camera_model", "cugo_graph_add_edges_model", "cugo_graph_n_fisheye_cameras",
                 "cugo_graph_get_flat_camera_models"):
        assert hasattr(L, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name + " is not declared in cugo_hip.h"
    for name, value in (("CUGO_RIG_NONE", 0), ("CUGO_RIG_EXTRINSICS", 1), ("CUGO_RIG_MODELS", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name
    assert (cugo.RIG_NONE, cugo.RIG_EXTRINSICS, cugo.RIG_MODELS, cugo.CAM_TAB_STRIDE) == (0, 1, 2, 17)
    # the struct has not grown
    assert re.search(r"double depth_weight;.*?int has_rig;[^;]*const double\* d_cam_ext;[^;]*\}\s*cugo_edges;", header, re.S)
    assert C.sizeof(cugo.RigEdges) == C.sizeof(cugo.Edges) + 16
    for m in ("set_camera_model", "n_fisheye_cameras", "flat_camera_models"):
        assert hasattr(cugo.Graph, m), m
    tab = cugo.camera_model_table(np.stack([rr.quat_to_ext(S1), rr.IDENTITY12]), np.stack([kb(K1), PIN]))
    assert tab.shape == (2, 17) and np.array_equal(tab[0, :12], rr.quat_to_ext(S1)) and np.array_equal(tab[0, 12:], kb(K1))
    assert np.array_equal(cugo.camera_model_table(None, np.stack([kb(K2)]))[0, :12], rr.IDENTITY12)
    with pytest.raises(cugo.CugoError):
        cugo.camera_model_table(None, np.array([[0, 0, 0, 0, 2.0]]))


PROGRAM = r"""
// a caller of the mirrored public headers with a two-camera fisheye rig: one MonoEdgeSet per fisheye camera
#include "ba_types.h"
#include "camera_model.h"
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
    CHECK(front.cameraModelData().type == cugo::Pinhole && front.cameraModelData().k[3] == 0.0);       // the default
    const cugo::CameraModel kbFront(cugo::KannalaBrandt, -0.0131, 0.0212, -0.0071, 0.0012);
    cugo::CameraModel kbSide = kbFront;
    kbSide.k[3] = 0.0018;
    front.setCameraModel(kbFront), side.setCameraModel(kbSide);
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
    std::vector<double> c5, x12, m5;
    CHECK(opt.flatCameras(c5, x12) && c5.size() == 10 && x12.size() == 24);
    CHECK(opt.flatCameraModels(m5) && m5.size() == 10 && opt.nFisheyeCameras() == 2 && opt.nRigCameras() == 1);
    CHECK(m5[0] == -0.0131 && m5[3] == 0.0012 && m5[4] == 1.0 && m5[5 + 3] == 0.0018 && m5[5 + 4] == 1.0);
    opt.initialize();
    CHECK(opt.flattenReuses() == 1);
    // set level: a mutable reference counts as a change
    side.getCameraModel().k[0] = -0.02;
    opt.initialize();
    CHECK(opt.flattenReuses() == 1 && opt.flatCameraModels(m5) && m5[5] == -0.02);
    // edge level: only with per-edge cameras is an edge's model looked at, but a change is a change
    opt.initialize();
    CHECK(opt.flattenReuses() == 2);
    es[1].setCameraModel(kbSide);
    opt.initialize();
    CHECK(opt.flattenReuses() == 2 && opt.nFisheyeCameras() == 2);
    opt.initialize();
    CHECK(opt.flattenReuses() == 3);
    es[2].getCameraModel();
    opt.initialize();
    CHECK(opt.flattenReuses() == 3);
    // both sets back to pinholes: no model table, the rig as it was
    front.setCameraModel(cugo::CameraModel()), side.setCameraModel(cugo::CameraModel());
    opt.initialize();
    CHECK(!opt.flatCameraModels(m5) && m5.size() == 10 && m5[4] == 0.0 && opt.nFisheyeCameras() == 0 && opt.nRigCameras() == 1);
    front.setCameraModel(kbFront), side.setCameraModel(kbSide);
    // coefficients that are not finite are refused with a message
    side.getCameraModel().k[2] = std::numeric_limits<double>::quiet_NaN();
    CHECK(refused(opt, "coefficients k1..k4 must be finite"));
    side.setCameraModel(kbSide);
    opt.initialize();
    // a Kannala-Brandt model on a stereo set is refused
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
    opt.initialize();                                   // a pinhole stereo set next to fisheye mono sets: fine
    stereo.setCameraModel(kbFront);
    CHECK(refused(opt, "Kannala-Brandt camera model on a stereo edge set is not defined"));
    stereo.setCameraModel(cugo::CameraModel());
    opt.initialize();
    // a depth set next to fisheye cameras is refused ("not yet"), and so is one that carries the model itself
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
    side.setSensorPose(cugo::Se3D());                   // (no rig: the refusal below is the models')
    CHECK(refused(opt, "camera models (Kannala-Brandt) together with depth edge sets are not supported yet"));
    front.setCameraModel(cugo::CameraModel()), side.setCameraModel(cugo::CameraModel());
    opt.initialize();
    depth.setCameraModel(kbFront);
    CHECK(refused(opt, "camera models (Kannala-Brandt) together with depth edge sets are not supported yet"));
    std::printf("OK\n");
    return 0;
}
"""


def test_a_caller_of_the_mirrored_headers_compiles_and_links(tmp_path):
    src = tmp_path / "fisheye_caller.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "fisheye_caller"
    lib_dir = os.path.dirname(cugo.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", INC, str(src), "-L", lib_dir, "-lcugo_hip",
                        "-Wl,-rpath," + lib_dir, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
