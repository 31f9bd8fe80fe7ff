"""Point-to-plane / point-to-line edge sets in the optimiser, host side only (plan-only optimisers: flattening,
validation, structure; no GPU): what initialize() accepts, counts, refuses and re-uses."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import icp_lm_ref as R
import icp_ref
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "include")
cugo = importlib.import_module("cuda-bundle-adjustment_amd")


def active_on_free(d, icp):
    """edges a flattening must keep, per kind: active and on a free pose"""
    return [int((np.asarray(act, bool) & ~np.asarray(d["pose_fixed"], bool)[e["pose"]]).sum()) for _, e, _, act, _ in icp]


def test_plan_only_graph_with_ba_plane_and_line_sets_initialises():
    d, icp = R.mixed_case()
    g = R.build_graph(d, icp, plan_only=True)
    g.initialize()
    n_pl, n_li = active_on_free(d, icp)
    # (the recipe: 169 plane edges of which 25 on the fixed pose 0 and ~10 % inactive, 37 line edges with 6 on pose 0)
    assert 0 < n_pl < 169 - 25 and n_li == 37 - 6
    assert g.n_icp_edges(cugo.ICP_PLANE) == n_pl and g.n_icp_edges(cugo.ICP_LINE) == n_li
    ba = cugo.graph_from_arrays(d, plan_only=True)
    ba.initialize()
    assert g.n_active_edges() == ba.n_active_edges() + n_pl + n_li
    assert g.n_icp_edges(2) == -1
    # ICP edges do not change the Hsc pattern
    assert g.structure_stats()["hsc_blocks"] == ba.structure_stats()["hsc_blocks"]
    with pytest.raises(cugo.CugoError, match="plan-only"):
        g.optimize(1)
    g.close()
    ba.close()


def test_icp_only_plan_only_graph_is_block_diagonal():
    d, icp = R.icp_only_case()
    g = R.build_graph(d, icp, plan_only=True)
    g.initialize()
    assert g.n_icp_edges(cugo.ICP_PLANE) == 285 - 20 and g.n_icp_edges(cugo.ICP_LINE) == 42 - 5
    assert g.n_active_edges() == 285 - 20 + 42 - 5
    # the same poses in a BA graph whose landmarks are all fixed: diagonal blocks only
    s = synth.make_problem(n_poses=6, n_landmarks=30, seed=1, fixed_poses=(5,))
    s["lm_fixed"] = np.ones(len(s["lm"]), np.uint8)
    ba = cugo.graph_from_arrays(s, plan_only=True)
    ba.initialize()
    assert g.structure_stats()["hsc_blocks"] == ba.structure_stats()["hsc_blocks"] == 5
    g.close()
    ba.close()


def test_free_pose_with_icp_edges_only_owns_a_diagonal_block():
    d = synth.make_problem(n_poses=6, n_landmarks=40, seed=2)
    e = dict(d)
    e["pose"] = np.concatenate([d["pose"], d["pose"][-1:]])  # a seventh, free pose that no BA edge observes
    e["pose_fixed"] = np.concatenate([d["pose_fixed"], [0]]).astype(np.uint8)
    rng = np.random.default_rng(0)
    pl = icp_ref.make_edges(rng, np.full(12, 6, np.int32), "plane", e["pose"], noise=0.01)
    icp = [("plane", pl, np.array([2.0]), np.ones(12, bool), (0, 1.0))]
    g = R.build_graph(e, icp, plan_only=True)
    g.initialize()
    ba = cugo.graph_from_arrays(d, plan_only=True)
    ba.initialize()
    assert g.n_icp_edges(cugo.ICP_PLANE) == 12
    assert g.structure_stats()["hsc_blocks"] == ba.structure_stats()["hsc_blocks"] + 1
    g.close()
    ba.close()


def small_graph():
    d = synth.make_problem(n_poses=4, n_landmarks=20, seed=3)
    g = cugo.graph_from_arrays(d, plan_only=True)
    return d, g


def plane_args(n=3, pose=1):
    nrm = np.tile([0.0, 0.6, 0.8], (n, 1))
    return np.full(n, pose, np.int32), np.arange(3.0 * n).reshape(n, 3), nrm, np.ones(n), np.ones(n)


def refused(g, match):
    with pytest.raises(cugo.CugoError, match=match):
        g.initialize()
    g.close()


def test_non_unit_normal_is_refused():
    _, g = small_graph()
    ids, p, nrm, dist, w = plane_args()
    nrm[1] *= 1.0 + 1e-5
    g.add_plane_edges(ids, p, nrm, dist, w)
    refused(g, "unit length")
    # ... and one that is off by less than 1e-6 is taken as given
    _, g = small_graph()
    nrm = plane_args()[2] * (1.0 + 5e-7)
    g.add_plane_edges(ids, p, nrm, dist, w)
    g.initialize()
    assert g.n_icp_edges(cugo.ICP_PLANE) == 3
    g.close()


def test_line_with_equal_points_is_refused():
    _, g = small_graph()
    a = np.array([[1.0, 2.0, 3.0], [0.0, 0.0, 1.0]])
    b = np.array([[2.0, 2.0, 3.0], [0.0, 0.0, 1.0]])
    g.add_line_edges(np.array([1, 2], np.int32), np.zeros((2, 3)), a, b, np.ones(2))
    refused(g, "a == b")


@pytest.mark.parametrize("where", ["point", "normal", "distance", "information", "line"])
def test_non_finite_values_are_refused(where):
    _, g = small_graph()
    ids, p, nrm, dist, w = plane_args()
    if where == "point":
        p[2, 1] = np.nan
    elif where == "normal":
        nrm[0, 0] = np.inf
    elif where == "distance":
        dist[1] = np.nan
    elif where == "information":
        w[1] = np.nan
    if where == "line":
        a = np.zeros((1, 3))
        b = np.array([[1.0, np.nan, 0.0]])
        g.add_line_edges(np.array([1], np.int32), np.zeros((1, 3)), a, b, np.ones(1))
    else:
        g.add_plane_edges(ids, p, nrm, dist, w)
    refused(g, "non-finite")


def test_unknown_pose_id_is_refused_and_adds_nothing():
    _, g = small_graph()
    ids, p, nrm, dist, w = plane_args()
    ids[2] = 77
    with pytest.raises(cugo.CugoError, match="unknown pose id 77"):
        g.add_plane_edges(ids, p, nrm, dist, w)
    with pytest.raises(cugo.CugoError, match="unknown pose id 77"):
        g.add_line_edges(ids, p, p, p + 1.0, w)
    g.initialize()
    assert g.n_icp_edges(cugo.ICP_PLANE) == 0 and g.n_icp_edges(cugo.ICP_LINE) == 0
    g.close()


def test_outlier_threshold_on_an_icp_set_is_refused():
    for kind in (cugo.ICP_PLANE, cugo.ICP_LINE):
        _, g = small_graph()
        g.add_plane_edges(*plane_args())
        g.set_icp_outlier_threshold(kind, 5.0)
        refused(g, "outlier rejection is not available")
    _, g = small_graph()
    g.add_plane_edges(*plane_args())
    g.set_icp_outlier_threshold(cugo.ICP_PLANE, 0.0)
    g.initialize()
    g.close()


def test_sharded_optimiser_refuses_icp_sets():
    _, g = small_graph()
    g.add_plane_edges(*plane_args())
    g.set_shard(0, 2, lambda ptr, n, op: None)
    refused(g, "sharded")
    # the same shard without ICP edges is taken
    _, g = small_graph()
    g.set_shard(0, 2, lambda ptr, n, op: None)
    g.initialize()
    g.close()


def test_estimates_only_initialize_with_icp_sets():
    d, icp = R.mixed_case()
    g = R.build_graph(d, icp, plan_only=True)
    g.initialize()
    n0 = g.n_icp_edges(cugo.ICP_PLANE)
    assert g.flatten_reuses() == 0
    g.set_poses(np.arange(len(d["pose"]), dtype=np.int32), d["pose_gt"])
    g.initialize()
    assert g.flatten_reuses() == 1 and g.n_icp_edges(cugo.ICP_PLANE) == n0
    # an ICP edge more: a new flattening
    g.add_plane_edges(*plane_args(n=1, pose=3))
    g.initialize()
    assert g.flatten_reuses() == 1 and g.n_icp_edges(cugo.ICP_PLANE) == n0 + 1
    g.initialize()
    assert g.flatten_reuses() == 2
    # the set's robust kernel or information touched: a new flattening, too
    g.set_icp_robust_kernel(cugo.ICP_LINE, cugo.RK_HUBER, 2.0)
    g.initialize()
    assert g.flatten_reuses() == 2
    g.close()


GRAPH_PROGRAM = r"""
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>
#include "cuda_graph_optimisation.h"
#include "icp_types.h"
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)
int main()
{
    cugo::GraphOptimisationOptions options;
    options.perEdgeInformation = true;
    options.planOnly = true;
    cugo::CudaGraphOptimisationImpl opt(options);
    cugo::PoseVertexSet poses(false);
    cugo::PoseVertex v0(0, cugo::Se3D(), false), v1(1, cugo::Se3D(), false), v2(2, cugo::Se3D(), true);
    poses.addVertex(&v0), poses.addVertex(&v1), poses.addVertex(&v2);
    cugo::PlaneEdgeSet planes;
    cugo::LineEdgeSet lines;
    std::vector<cugo::PlaneEdge> pe(5);
    std::vector<cugo::LineEdge> le(3);
    cugo::Vec3d n, p, a, b;
    n[0] = 0, n[1] = 0, n[2] = 1;
    for (int i = 0; i < 5; i++)
    {
        p[0] = i, p[1] = 1, p[2] = 2;
        pe[i].setMeasurement(cugo::PointToPlaneMatch<double>(n, 0.5 * i, p));
        pe[i].setVertex(i < 2 ? &v0 : i < 4 ? &v1 : &v2, 0); // the last one sits on the fixed pose
        pe[i].setInformation(1.0 + i);
        planes.addEdge(&pe[i]);
    }
    for (int i = 0; i < 3; i++)
    {
        a[0] = 1, a[1] = i, a[2] = 0;
        b[0] = 2, b[1] = i, b[2] = 1;
        cugo::PointToLineMatch<double> m(a, b);
        m.pointP = p;
        le[i].setMeasurement(m);
        le[i].setVertex(&v1, 0);
        le[i].setInformation(2.0);
        lines.addEdge(&le[i]);
    }
    planes.setRobustKernel(cugo::RobustKernelType::Huber, 1.5);
    opt.addVertexSet(&poses);
    opt.addEdgeSet(&planes);
    opt.addEdgeSet(&lines);
    opt.initialize();
    CHECK(opt.nIcpEdges(0) == 4 && opt.nIcpEdges(1) == 3 && opt.nActiveEdges() == 7);
    CHECK(planes.nActiveEdges() == 4 && lines.nActiveEdges() == 3);
    // an inactive edge is left out
    pe[0].inactivate();
    opt.initialize();
    CHECK(opt.nIcpEdges(0) == 3 && opt.flattenReuses() == 0);
    opt.initialize();
    CHECK(opt.flattenReuses() == 1);
    // touching a measurement through the mutable pointer forces a new flattening
    static_cast<cugo::PointToPlaneMatch<double>*>(pe[1].getMeasurement())->originDistance = 0.25;
    opt.initialize();
    CHECK(opt.flattenReuses() == 1);
    // a second plane set with another robust kernel is refused; with the same one it is taken
    cugo::PlaneEdgeSet planes2;
    cugo::PlaneEdge extra;
    extra.setMeasurement(cugo::PointToPlaneMatch<double>(n, 1.0, p));
    extra.setVertex(&v0, 0);
    extra.setInformation(1.0);
    planes2.addEdge(&extra);
    opt.addEdgeSet(&planes2);
    bool threw = false;
    try { opt.initialize(); } catch (const std::runtime_error& e) { threw = std::string(e.what()).find("same robust kernel") != std::string::npos; }
    CHECK(threw);
    planes2.setRobustKernel(cugo::RobustKernelType::Huber, 1.5);
    opt.initialize();
    CHECK(opt.nIcpEdges(0) == 4);
    // an edge on a pose vertex of no vertex set of the optimiser is refused
    cugo::PoseVertexSet other(false);
    cugo::PoseVertex w(9, cugo::Se3D(), false);
    other.addVertex(&w);
    cugo::PlaneEdge stray;
    stray.setMeasurement(cugo::PointToPlaneMatch<double>(n, 1.0, p));
    stray.setVertex(&w, 0);
    planes2.addEdge(&stray);
    threw = false;
    try { opt.initialize(); } catch (const std::runtime_error& e) { threw = std::string(e.what()).find("no pose vertex set") != std::string::npos; }
    CHECK(threw);
    std::printf("OK\n");
    return 0;
}
"""


def test_cpp_sets_are_taken_by_a_plan_only_optimiser(tmp_path):
    src = tmp_path / "icp_graph.cpp"
    src.write_text(GRAPH_PROGRAM)
    exe = tmp_path / "icp_graph"
    lib_dir = os.path.dirname(cugo.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", INC, str(src), "-L", lib_dir, "-lcugo_hip",
                        "-Wl,-rpath," + lib_dir, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
