"""CPU tests of the host side of camera extrinsics (no GPU): the flattened camera table of a plan-only Graph (sensor
poses beside the cameras, the de-duplication key, has_rig), flatten re-use at set level and — through a C++ caller of
the mirrored headers — at edge level, the refusals of initialize() with their messages, and the exported symbols."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import rig_ref as rr

cugo = importlib.import_module("cuda-bundle-adjustment_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "include")
CAM = np.array([718.856, 718.856, 607.1928, 185.2157, 386.1448])
IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
S1 = np.array([0.02, 0.06, -0.01, 0.99, 0.4, 0.0, 0.1])          # (not normalised on purpose)
S2 = np.array([0.0, 0.7071067811865476, 0.0, 0.7071067811865476, -0.4, 0.0, 0.0])   # 90 degrees of yaw


def problem(seed=0):
    rng = np.random.default_rng(seed)
    pose = np.zeros((4, 7))
    pose[:, 3] = 1.0
    pose[:, 4] = np.arange(4) * 0.5
    lm = np.column_stack([rng.uniform(-4, 4, 12), rng.uniform(-2, 2, 12), rng.uniform(8, 30, 12)])
    ep, el = np.repeat(np.arange(4), 12).astype(np.int32), np.tile(np.arange(12), 4).astype(np.int32)
    return dict(pose=pose, lm=lm, ep=ep, el=el, meas=np.column_stack([rng.uniform(0, 1200, 48), rng.uniform(0, 370, 48), rng.uniform(0, 1200, 48)]))


def graph(d, per_edge_camera, sensor=None, cams=None, stereo_sel=None, depth_sel=None):
    """mono edges (and stereo edges where stereo_sel); sensor / cams: per edge, or None"""
    g = cugo.Graph(True, per_edge_camera, plan_only=True)
    g.add_poses(np.arange(4, dtype=np.int32), d["pose"], np.array([1, 0, 0, 0], np.uint8))
    g.add_landmarks(np.arange(12, dtype=np.int32), d["lm"], np.zeros(12, np.uint8))
    n = len(d["ep"])
    st = np.zeros(n, bool) if stereo_sel is None else stereo_sel
    dp = np.zeros(n, bool) if depth_sel is None else depth_sel
    for dim, sel in ((2, ~st & ~dp), (3, st)):
        g.add_edges(dim, d["ep"][sel], d["el"][sel], d["meas"][sel], np.ones(int(sel.sum())),
                    None if cams is None else cams[sel], None if sensor is None else sensor[sel])
    if dp.any():
        g.add_depth_edges(d["ep"][dp], d["el"][dp], d["meas"][dp] * np.array([1, 1, 1e-4]), np.ones(int(dp.sum())))
        g.set_depth_camera(CAM)
    g.set_camera(2, CAM)
    g.set_camera(3, CAM)
    return g


def test_sensor_poses_flatten_beside_the_cameras():
    d = problem()
    n = 48
    sensor = np.stack([IDENT, S1, S2])[np.arange(n) % 3]
    cams = np.tile(CAM, (n, 1))
    cams[np.arange(n) % 2 == 1] *= 1.01
    g = graph(d, True, sensor, cams)
    g.initialize()
    t = g.flat_cameras()
    # six distinct (intrinsics, sensor pose) pairs, first-seen order: edge i has pair (i % 2, i % 3)
    assert t["has_rig"] and len(t["cams"]) == 6 and g.n_rig_cameras() == 4
    seen = []
    for i in range(n):
        if (i % 2, i % 3) not in seen:
            seen.append((i % 2, i % 3))
    for k, (a, b) in enumerate(seen):
        assert np.array_equal(t["cams"][k], CAM * (1.01 if a else 1.0))
        assert np.array_equal(t["ext"][k], rr.quat_to_ext((IDENT, S1, S2)[b])), "normalised and expanded on the host, in fp64"
    M = t["ext"][:, :9].reshape(-1, 3, 3)
    # orthonormal to fp64: an entry of M carries ~4 roundings, a row product sums three such -> well inside 16 u
    assert np.abs(np.einsum("kij,klj->kil", M, M) - np.eye(3)).max() < 16 * 2.0 ** -53
    g.close()


def test_the_key_covers_intrinsics_and_sensor_pose():
    d = problem()
    n = 48
    # same intrinsics, two sensor poses -> two entries; same sensor pose, two intrinsics -> two entries; all four -> four
    for sensor_of, cam_of, want in ((lambda i: i % 2, lambda i: 0, 2), (lambda i: 1, lambda i: i % 2, 2),
                                    (lambda i: i % 2, lambda i: (i // 2) % 2, 4), (lambda i: 1, lambda i: 0, 1)):
        sensor = np.stack([S1 if sensor_of(i) else IDENT for i in range(n)])
        cams = np.stack([CAM * (1.0 + 0.01 * cam_of(i)) for i in range(n)])
        g = graph(d, True, sensor, cams)
        g.initialize()
        assert len(g.flat_cameras()["cams"]) == want
        g.close()


def test_has_rig_is_0_without_sensor_poses_and_with_identities_only():
    d = problem()
    g = graph(d, True, None, np.tile(CAM, (48, 1)))
    g.initialize()
    t = g.flat_cameras()
    assert not t["has_rig"] and g.n_rig_cameras() == 0 and np.all(t["ext"] == rr.IDENTITY12[None, :])
    g.close()
    # identities, one of them as a scaled quaternion and one as -q: still the kernels the library has always run
    sensor = np.stack([IDENT, 3.0 * IDENT, -IDENT])[np.arange(48) % 3]
    g = graph(d, True, sensor, np.tile(CAM, (48, 1)))
    g.initialize()
    t = g.flat_cameras()
    assert not t["has_rig"] and g.n_rig_cameras() == 0 and len(t["cams"]) == 3
    g.close()
    # without per-edge cameras the set's sensor pose applies and a per-edge one is not looked at
    g = graph(d, False, np.tile(S1, (48, 1)), np.tile(CAM, (48, 1)))
    g.initialize()
    assert not g.flat_cameras()["has_rig"]
    g.set_sensor_pose(2, S2)
    g.initialize()
    t = g.flat_cameras()
    assert t["has_rig"] and len(t["cams"]) == 1 and np.array_equal(t["ext"][0], rr.quat_to_ext(S2))
    g.close()


def test_flatten_reuse_notices_a_changed_sensor_pose_of_the_set():
    d = problem()
    g = graph(d, False, stereo_sel=np.arange(48) % 2 == 1)
    g.initialize()
    g.initialize()
    assert g.flatten_reuses() == 1
    g.set_sensor_pose(3, S1)
    g.initialize()
    assert g.flatten_reuses() == 1, "a changed sensor pose must count as a change of the set"
    t = g.flat_cameras()
    assert t["has_rig"] and len(t["cams"]) == 2 and g.n_rig_cameras() == 1      # mono: identity, stereo: S1
    g.initialize()
    assert g.flatten_reuses() == 2
    g.close()


def test_rig_with_a_depth_set_is_refused():
    d = problem()
    g = graph(d, False, depth_sel=np.arange(48) % 3 == 0)
    g.initialize()                                           # identities: an ordinary graph with depth edges
    g.set_sensor_pose(2, S1)
    with pytest.raises(cugo.CugoError, match="camera extrinsics .*together with depth edge sets are not supported yet"):
        g.initialize()
    g.close()


def test_rig_on_a_sharded_optimiser_is_refused():
    g = graph(problem(), False)
    g.set_sensor_pose(2, S1)
    g.set_shard(0, 2, lambda ptr, n, op: None)
    with pytest.raises(cugo.CugoError, match="camera extrinsics .*not supported on a landmark-sharded"):
        g.initialize()
    g.close()


@pytest.mark.parametrize("bad", [np.array([0, 0, 0, 0, 0.1, 0, 0.0]), np.array([np.nan, 0, 0, 1, 0, 0, 0.0]),
                                 np.array([0, 0, 0, 1, np.inf, 0, 0.0])])
def test_a_bad_sensor_pose_is_refused(bad):
    g = graph(problem(), False)
    g.set_sensor_pose(2, bad)
    with pytest.raises(cugo.CugoError, match="camera extrinsics .*quaternion must be finite with a norm > 0"):
        g.initialize()
    g.set_sensor_pose(2, S1)
    g.initialize()
    g.close()


def test_symbols_are_exported_and_declared():
    L = cugo.lib()
    header = open(os.path.join(ROOT, "include", "cugo_hip.h")).read()
    for name in ("cugo_graph_set_sensor_pose", "cugo_graph_add_edges_rig", "cugo_graph_n_rig_cameras",
                 "cugo_graph_get_flat_cameras"):
        assert hasattr(L, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name + " is not declared in cugo_hip.h"
    assert re.search(r"double depth_weight;.*?int has_rig;\s*const double\* d_cam_ext;[^;]*\}\s*cugo_edges;", header, re.S), \
        "has_rig, d_cam_ext must be the last members of cugo_edges"
    names = [n for n, _ in cugo.Edges._fields_] + [n for n, _ in cugo.RigEdges._fields_]
    assert names[-3:] == ["depth_weight", "has_rig", "d_cam_ext"]
    ev = cugo.RigEdges()
    assert ev.has_rig == 0 and C.sizeof(cugo.RigEdges) == C.sizeof(cugo.Edges) + 16
    assert cugo.RigEdges.has_rig.offset == C.sizeof(cugo.Edges)
    # an Edges() is the head of a zeroed full struct: the library reads has_rig = 0 behind it
    head = cugo.Edges()
    assert C.cast(C.byref(head), C.POINTER(cugo.RigEdges)).contents.has_rig == 0
    for m in ("set_sensor_pose", "n_rig_cameras", "flat_cameras"):
        assert hasattr(cugo.Graph, m), m


PROGRAM = r"""
// a caller of the mirrored public headers with a two-camera rig: one MonoEdgeSet per physical camera
#include "ba_types.h"
#include "cuda_graph_optimisation.h"
#include <cmath>
#include <cstdio>
#include <deque>
#include <stdexcept>
#include <string>
#include <vector>
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
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
    for (int j = 0; j < 7; j++) // (landmark 6 is seen by the depth edge further down only)
    {
        const double x[3] = {j - 2.5, 0.3 * j, 10.0 + j};
        ls.emplace_back(j, cugo::Vec3d(x), false);
        lms.addVertex(&ls.back());
    }
    cugo::MonoEdgeSet front, side;
    const cugo::Camera cam(700.0, 700.0, 600.0, 180.0, 0.0);
    front.setCamera(cam), side.setCamera(cam);
    front.setInformation(1.0), side.setInformation(1.0);
    // body -> sensor: the side camera is yawed by 90 degrees, 0.4 m to the left of the front one
    const double qs[4] = {0, 0.7071067811865476, 0, 0.7071067811865476}, tsd[3] = {-0.4, 0.0, 0.0};
    const cugo::Se3D T_side(qs, tsd);
    CHECK(front.sensorPoseData().r.data[3] == 1.0 && front.sensorPoseData().t.data[0] == 0.0);   // identity by default
    side.setSensorPose(T_side);
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
    std::vector<double> c5, x12;
    CHECK(opt.flatCameras(c5, x12) && c5.size() == 10 && x12.size() == 24 && opt.nRigCameras() == 1);
    CHECK(x12[0] == 1.0 && x12[9] == 0.0);                       // the front camera: identity
    // Ry(90 degrees): M02 = 1, M20 = -1
    CHECK(std::fabs(x12[12 + 2] - 1.0) < 1e-15 && std::fabs(x12[12 + 6] + 1.0) < 1e-15 && x12[12 + 9] == -0.4);
    opt.initialize();
    CHECK(opt.flattenReuses() == 1);
    // set level: a mutable reference counts as a change
    side.getSensorPose().t.data[0] = -0.5;
    opt.initialize();
    CHECK(opt.flattenReuses() == 1 && opt.flatCameras(c5, x12) && x12[12 + 9] == -0.5);
    // edge level: only with per-edge cameras is an edge's sensor pose looked at, but a change is a change
    opt.initialize();
    CHECK(opt.flattenReuses() == 2);
    es[1].setSensorPose(T_side);
    opt.initialize();
    CHECK(opt.flattenReuses() == 2);
    opt.initialize();
    CHECK(opt.flattenReuses() == 3);
    es[2].getSensorPose();
    opt.initialize();
    CHECK(opt.flattenReuses() == 3);
    // a quaternion of norm 0 is refused with a message
    const double q0[4] = {0, 0, 0, 0};
    side.setSensorPose(cugo::Se3D(q0, tsd));
    bool threw = false;
    try { opt.initialize(); }
    catch (const std::runtime_error& e) { threw = std::string(e.what()).find("quaternion must be finite with a norm > 0") != std::string::npos; }
    CHECK(threw);
    side.setSensorPose(T_side);
    // a depth set next to a rig is refused ("not yet")
    cugo::DepthEdgeSet depth;
    depth.setCamera(cam);
    depth.setInformation(1.0);
    cugo::DepthEdge de;
    de.setVertex(&ps[1], 0), de.setVertex(&ls[6], 1);
    const double m3[3] = {600.0, 180.0, 0.1};
    de.setMeasurement(cugo::Vec3d(m3));
    de.setInformation(1.0);
    depth.addEdge(&de);
    opt.addEdgeSet(&depth);
    threw = false;
    try { opt.initialize(); }
    catch (const std::runtime_error& e) { threw = std::string(e.what()).find("together with depth edge sets are not supported yet") != std::string::npos; }
    CHECK(threw);
    // ... and so is a DepthEdgeSet that carries a sensor pose itself
    side.setSensorPose(cugo::Se3D());
    opt.initialize();
    depth.setSensorPose(T_side);
    threw = false;
    try { opt.initialize(); }
    catch (const std::runtime_error& e) { threw = std::string(e.what()).find("together with depth edge sets are not supported yet") != std::string::npos; }
    CHECK(threw);
    std::printf("OK\n");
    return 0;
}
"""


def test_a_caller_of_the_mirrored_headers_compiles_and_links(tmp_path):
    src = tmp_path / "rig_caller.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "rig_caller"
    lib_dir = os.path.dirname(cugo.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", INC, str(src), "-L", lib_dir, "-lcugo_hip",
                        "-Wl,-rpath," + lib_dir, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
