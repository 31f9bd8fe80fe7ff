"""CPU tests of the depth edges' host side (no GPU): flattening through a plan-only Graph, flatten re-use, the refusals
of initialize() with their messages, the exported symbols, and a C++ translation unit written as a caller of the
reference's ba_types.h would write it."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

cugo = importlib.import_module("cuda-bundle-adjustment_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "include")
CAM = np.array([718.856, 718.856, 607.1928, 185.2157, 386.1448])


def problem(seed=0):
    """4 poses (pose 0 fixed), 12 landmarks in front of them (landmark 11 fixed), every pose sees every landmark"""
    rng = np.random.default_rng(seed)
    pose = np.zeros((4, 7))
    pose[:, 3] = 1.0
    pose[:, 4] = np.arange(4) * 0.5
    lm = np.column_stack([rng.uniform(-4, 4, 12), rng.uniform(-2, 2, 12), rng.uniform(8, 30, 12)])
    ep, el = np.repeat(np.arange(4), 12).astype(np.int32), np.tile(np.arange(12), 4).astype(np.int32)
    Xc = lm[el] + pose[ep, 4:]
    u = CAM[0] * Xc[:, 0] / Xc[:, 2] + CAM[2]
    v = CAM[1] * Xc[:, 1] / Xc[:, 2] + CAM[3]
    return dict(pose=pose, lm=lm, ep=ep, el=el, u=u, v=v, ur=u - CAM[4] / Xc[:, 2], invz=1.0 / Xc[:, 2])


def graph(d, weight=None, depth_sel=None):
    g = cugo.Graph(True, True, plan_only=True)
    g.add_poses(np.arange(4, dtype=np.int32), d["pose"], np.array([1, 0, 0, 0], np.uint8))
    fixed_l = np.zeros(12, np.uint8)
    fixed_l[11] = 1
    g.add_landmarks(np.arange(12, dtype=np.int32), d["lm"], fixed_l)
    kind = np.arange(48) % 3 if depth_sel is None else depth_sel
    n = len(kind)
    cam = np.tile(CAM, (n, 1))
    for dim, sel, third in ((2, kind == 0, None), (3, kind == 1, d["ur"])):
        meas = np.column_stack([d["u"], d["v"], np.zeros(n) if third is None else third])[sel]
        g.add_edges(dim, d["ep"][sel], d["el"][sel], meas, np.ones(int(sel.sum())), cam[sel])
    sel = kind == 2
    g.add_depth_edges(d["ep"][sel], d["el"][sel], np.column_stack([d["u"], d["v"], d["invz"]])[sel], 0.5 * np.ones(int(sel.sum())),
                      cam[sel] * 1.01)
    if weight is not None:
        g.set_depth_weight(weight)
    return g, kind


def test_depth_edges_flatten_into_the_shared_array():
    d = problem()
    g, kind = graph(d, weight=1e4)
    g.initialize()
    fe = g.flat_edges()
    # every edge but those between the fixed pose and the fixed landmark; mono, stereo, then the depth set (added last)
    keep = ~((d["ep"] == 0) & (d["el"] == 11))
    order = np.concatenate([np.flatnonzero(keep & (kind == q)) for q in (0, 1, 2)])
    assert len(fe["pose"]) == keep.sum() == 47
    is_depth = (fe["flags"] & cugo.EDGE_DEPTH) != 0
    assert is_depth.sum() == (keep & (kind == 2)).sum() and not np.any(is_depth & ((fe["flags"] & cugo.EDGE_STEREO) != 0))
    assert np.array_equal(is_depth, kind[order] == 2)
    assert np.array_equal(((fe["flags"] & cugo.EDGE_STEREO) != 0), kind[order] == 1)
    assert np.array_equal(fe["meas"][is_depth, 2], d["invz"][order][is_depth])
    assert np.array_equal(fe["meas"][:, 0], d["u"][order]) and np.all(fe["meas"][kind[order] == 0, 2] == 0)
    # fixed-vertex bits as for the other kinds: pose 0 and landmark 11 are the fixed ones (flattened behind the free)
    assert np.array_equal((fe["flags"] & 2) != 0, d["ep"][order] == 0) and np.array_equal((fe["flags"] & 1) != 0, d["el"][order] == 11)
    assert fe["has_depth"] and fe["depth_weight"] == 1e4
    assert g.n_active_edges() == 47
    g.close()


def test_a_graph_without_depth_edges_says_so():
    d = problem()
    g, _ = graph(d, weight=3.0, depth_sel=np.arange(48) % 2)
    g.initialize()
    fe = g.flat_edges()
    assert not fe["has_depth"] and not np.any(fe["flags"] & cugo.EDGE_DEPTH)
    g.close()


def test_flatten_reuse_notices_a_changed_weight():
    d = problem()
    g, _ = graph(d)
    g.initialize()
    assert g.flatten_reuses() == 0 and g.flat_edges()["depth_weight"] == 1.0
    g.initialize()
    assert g.flatten_reuses() == 1
    g.set_depth_weight(25.0)
    g.initialize()
    assert g.flatten_reuses() == 1, "a changed inverse-depth weight must count as a change of the set"
    assert g.flat_edges()["depth_weight"] == 25.0
    g.initialize()
    assert g.flatten_reuses() == 2
    g.set_depth_robust_kernel(cugo.RK_HUBER, 1.5)
    g.set_depth_outlier_threshold(9.0)
    g.initialize()
    assert g.flatten_reuses() == 2
    assert g.n_depth_outliers() == 0 and g.depth_edge_active(16).all()
    g.close()


@pytest.mark.parametrize("bad", [0.0, -2.0, float("nan"), float("inf")])
def test_a_bad_weight_is_refused_by_initialize(bad):
    g, _ = graph(problem(), weight=bad)
    with pytest.raises(cugo.CugoError, match="inverse-depth weight must be finite and > 0"):
        g.initialize()
    g.set_depth_weight(2.0)
    g.initialize()
    g.close()


def test_a_sharded_optimiser_refuses_depth_sets():
    g, _ = graph(problem())
    g.set_shard(0, 2, lambda ptr, n, op: None)
    with pytest.raises(cugo.CugoError, match="depth edge sets are not supported on a landmark-sharded"):
        g.initialize()
    g.close()


def test_symbols_are_exported():
    L = cugo.lib()
    for name in ("cugo_graph_add_depth_edges", "cugo_graph_set_depth_camera", "cugo_graph_set_depth_information",
                 "cugo_graph_set_depth_robust_kernel", "cugo_graph_set_depth_outlier_threshold", "cugo_graph_set_depth_weight",
                 "cugo_graph_n_depth_outliers", "cugo_graph_get_depth_edge_active", "cugo_graph_get_flat_edges",
                 "cugo_compute_edge_chi"):
        assert hasattr(L, name), name
    assert cugo.EDGE_DEPTH == 16
    names = [n for n, _ in cugo.Edges._fields_]
    assert names[-5:] == ["block_f32", "has_depth", "rk_type_depth", "rk_delta_depth", "depth_weight"]
    ev = cugo.Edges()
    assert ev.has_depth == 0
    for m in ("add_depth_edges", "set_depth_camera", "set_depth_information", "set_depth_robust_kernel",
              "set_depth_outlier_threshold", "set_depth_weight", "n_depth_outliers", "depth_edge_active"):
        assert hasattr(cugo.Graph, m), m


PROGRAM = r"""
// a caller of the reference's public header: DepthEdge / DepthEdgeSet of ba_types.h
#include "ba_types.h"
#include "cuda_graph_optimisation.h"
#include <cstdio>
#include <deque>
#include <stdexcept>
#include <string>
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
int main()
{
    cugo::GraphOptimisationOptions options;
    options.planOnly = true;
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
    for (int j = 0; j < 5; j++)
    {
        const double x[3] = {j - 2.0, 0.3 * j, 10.0 + j};
        ls.emplace_back(j, cugo::Vec3d(x), false);
        lms.addVertex(&ls.back());
    }
    cugo::DepthEdgeSet depth, depth2;
    depth.setCamera(cugo::Camera(700.0, 700.0, 600.0, 180.0, 0.0));
    depth.setInformation(1.0);
    CHECK(depth.inverseDepthWeight() == 1.0 && depth.dim() == 3);
    std::deque<cugo::DepthEdge> es;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 5; j++)
        {
            es.emplace_back();
            cugo::DepthEdge& e = es.back();
            e.setVertex(&ps[i], 0), e.setVertex(&ls[j], 1);
            const double X = j - 2.0 + 0.5 * i, Y = 0.3 * j, Z = 10.0 + j;
            const double m[3] = {700 * X / Z + 600, 700 * Y / Z + 180, 1 / Z};
            e.setMeasurement(cugo::Vec3d(m));
            e.setInformation(1.0);
            (i == 2 && j == 4 ? depth2 : depth).addEdge(&e);
        }
    opt.addVertexSet(&poses);
    opt.addVertexSet(&lms);
    opt.addEdgeSet(&depth);
    opt.initialize();
    CHECK(opt.nActiveEdges() == 14);
    double w = 0;
    CHECK(opt.flatDepth(w) && w == 1.0);
    depth.setInverseDepthWeight(1e4);
    opt.initialize();
    CHECK(opt.flattenReuses() == 0 && opt.flatDepth(w) && w == 1e4);
    // a second depth set with another weight: one weight per optimiser
    depth2.setCamera(cugo::Camera(700.0, 700.0, 600.0, 180.0, 0.0));
    opt.addEdgeSet(&depth2);
    bool threw = false;
    try { opt.initialize(); }
    catch (const std::runtime_error& e) { threw = std::string(e.what()).find("disagree on the inverse-depth weight") != std::string::npos; }
    CHECK(threw);
    depth2.setInverseDepthWeight(1e4);
    opt.initialize();
    CHECK(opt.nActiveEdges() == 15);
    depth2.setInverseDepthWeight(-1.0);
    threw = false;
    try { opt.initialize(); }
    catch (const std::runtime_error& e) { threw = std::string(e.what()).find("must be finite and > 0") != std::string::npos; }
    CHECK(threw);
    std::printf("OK\n");
    return 0;
}
"""


def test_a_caller_of_the_reference_header_compiles_and_links(tmp_path):
    src = tmp_path / "depth_caller.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "depth_caller"
    lib_dir = os.path.dirname(cugo.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", INC, str(src), "-L", lib_dir, "-lcugo_hip",
                        "-Wl,-rpath," + lib_dir, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
