"""Point-to-point edge sets (PointEdgeSet, point_edge_types.h) without a GPU: what a plan-only optimiser accepts, counts,
refuses and re-uses, the C++ sets as a caller would use them, the exported symbols and the ctypes layout of
cugo_point_edges."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "include")
cugo = importlib.import_module("cuda-bundle-adjustment_amd")

SYMBOLS = ["cugo_point_compute_errors", "cugo_point_construct_quadratic_form", "cugo_point_construct_quadratic_form_schur",
           "cugo_graph_add_point_edges", "cugo_graph_set_point_information", "cugo_graph_set_point_robust_kernel",
           "cugo_graph_n_point_edges", "cugo_graph_get_flat_point_edges"]


def small_graph(per_edge_information=True, fixed_poses=(0,)):
    d = synth.make_problem(n_poses=4, n_landmarks=20, seed=3, fixed_poses=fixed_poses)
    return d, cugo.graph_from_arrays(d, plan_only=True, per_edge_information=per_edge_information)


def point_args(poses=(1, 2, 2, 0), seed=1):
    rng = np.random.default_rng(seed)
    ids = np.asarray(poses, np.int32)
    return ids, rng.normal(size=(len(ids), 3)), rng.normal(size=(len(ids), 3)), np.tile(np.eye(3), (len(ids), 1, 1))


def refused(g, match):
    with pytest.raises(cugo.CugoError, match=match):
        g.initialize()
    g.close()


def test_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "cugo_hip.h")).read()
    for s in SYMBOLS:
        assert hasattr(cugo.lib(), s), s
        assert re.search(r"\bint %s\(" % s, header), s
    assert "typedef struct cugo_point_edges" in header


def test_plan_only_graph_takes_point_sets_and_drops_what_counts_for_nothing():
    d, g = small_graph()
    assert d["pose_fixed"][0] and not d["pose_fixed"][1]
    g.add_point_edges(*point_args())                       # the last one sits on the fixed pose 0
    g.initialize()
    assert g.n_point_edges() == 3
    d2, no = small_graph()
    no.initialize()
    assert no.n_point_edges() == 0 and g.n_active_edges() == no.n_active_edges() + 3
    for k in ("hsc_blocks", "products", "nnzL", "supernodes"):   # unary edges change neither the pattern nor the factor
        assert g.structure_stats()[k] == no.structure_stats()[k], k
    with pytest.raises(cugo.CugoError, match="plan-only"):
        g.optimize(1)
    # the four kinds of CUGO_POSE_KIND_* stay four: the point set is none of them
    assert cugo.lib().cugo_graph_n_pose_edge_outliers(g._g, 4) < 0
    g.close()
    no.close()


def pack6(M):
    M = np.asarray(M)
    return np.array([M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2]])


def flat_case(per_edge_information, seed=7):
    """4 poses (pose 0 fixed) and 9 point edges added in an order that is NOT sorted by pose: two on the fixed pose, per-edge
    matrices that all differ, one of them asymmetric inside the tolerance"""
    d, g = small_graph(per_edge_information=per_edge_information)
    rng = np.random.default_rng(seed)
    ids = np.array([3, 1, 0, 2, 1, 3, 0, 1, 2], np.int32)
    p, z = rng.normal(size=(9, 3)), rng.normal(size=(9, 3))
    A = rng.normal(size=(9, 3, 3))
    info = np.einsum("eik,ejk->eij", A, A) + np.eye(3)[None]
    info[4, 0, 2] += 1e-13 * np.abs(info[4]).max()         # asymmetric, inside 1e-12 max|Omega|: taken and symmetrised
    g.add_point_edges(ids, p, z, info)
    return d, g, ids, p, z, info


def test_the_flattened_arrays_per_edge_information():
    """what the flattening hands the kernels: edges on the fixed pose dropped, the others sorted by pose (stable: insertion
    order inside a pose), p [3][n] and z [3][n] planar, Omega as the packed upper triangle 00 01 02 11 12 22 of its symmetric
    part, one column per edge"""
    d, g, ids, p, z, info = flat_case(True)
    g.initialize()
    f = g.flat_point_edges()
    keep = np.flatnonzero(ids != 0)
    order = keep[np.argsort(ids[keep], kind="stable")]     # the expected slot -> edge added
    assert g.n_point_edges() == 7 and np.array_equal(f["src"], order) and f["n_info"] == 7
    assert np.all(np.diff(f["pose"]) >= 0) and len(np.unique(f["pose"])) == 3 and f["pose"].max() < 3   # free poses 0..2
    # pose ids 1, 2, 3 are free and keep their ascending order in the free-first index
    assert np.array_equal(f["pose"], ids[order] - 1)
    assert f["p"].shape == (3, 7) and np.array_equal(f["p"], p[order].T) and np.array_equal(f["z"], z[order].T)
    want = np.array([pack6(0.5 * (info[e] + info[e].T)) for e in order]).T
    assert f["info"].shape == (6, 7) and np.array_equal(f["info"], want)
    k = int(np.flatnonzero(order == 4)[0])
    assert info[4, 0, 2] != info[4, 2, 0] and f["info"][2, k] == 0.5 * (info[4, 0, 2] + info[4, 2, 0])
    # (a transposed meas or a column-packed triangle would show: the rows differ)
    assert not np.array_equal(f["info"][2], f["info"][3]) and not np.array_equal(f["p"][0], f["p"][1])
    g.close()


def test_the_flattened_arrays_set_level_information_and_uniform_matrices():
    """without perEdgeInformation the set's matrix counts: ONE column (n_info = 1), the edges' own matrices are not looked at;
    with it, matrices that are all equal collapse to one column as well"""
    d, g, ids, p, z, info = flat_case(False)
    S = np.array([[4.0, 1, 0.5], [1, 3, 0.2], [0.5, 0.2, 2]])
    g.set_point_information(S)
    g.initialize()
    f = g.flat_point_edges()
    assert f["n_info"] == 1 and f["info"].shape == (6, 1) and np.array_equal(f["info"][:, 0], pack6(S))
    assert len(f["pose"]) == 7 and np.array_equal(f["p"], p[f["src"]].T) and np.array_equal(f["z"], z[f["src"]].T)
    g.close()
    d, g = small_graph()
    ids, p, z, _ = point_args(poses=(2, 1, 2))
    g.add_point_edges(ids, p, z, np.tile(S, (3, 1, 1)))
    g.initialize()
    f = g.flat_point_edges()
    assert f["n_info"] == 1 and np.array_equal(f["info"][:, 0], pack6(S)) and np.array_equal(f["src"], [1, 0, 2])
    g.close()
    # edges added WITHOUT a matrix take a copy of the set's matrix at the time of the add
    d, g = small_graph()
    g.set_point_information(S)
    g.add_point_edges(ids[:2], p[:2], z[:2])
    g.set_point_information(2 * S)
    g.add_point_edges(ids[2:], p[2:], z[2:])
    g.initialize()
    f = g.flat_point_edges()
    assert f["n_info"] == 3 and np.array_equal(f["src"], [1, 0, 2])
    assert np.array_equal(f["info"].T, [pack6(S), pack6(S), pack6(2 * S)])
    g.close()


def test_the_flattened_arrays_of_a_graph_without_point_edges():
    d, g = small_graph()
    g.add_point_edges(*point_args(poses=(0, 0)))           # the fixed pose only: nothing is flattened
    g.initialize()
    f = g.flat_point_edges()
    assert len(f["pose"]) == 0 and f["p"].shape == (3, 0)
    g.close()


def test_point_sets_alone_without_landmarks():
    rng = np.random.default_rng(4)
    pose = np.tile(np.array([0, 0, 0, 1.0, 0, 0, 0]), (3, 1))
    d = dict(pose=pose, pose_fixed=np.array([0, 0, 1], np.uint8), lm=np.zeros((0, 3)), lm_fixed=np.zeros(0, np.uint8),
             e_pose=np.zeros(0, np.int32), e_lm=np.zeros(0, np.int32), e_stereo=np.zeros(0, np.uint8), e_meas=np.zeros((0, 3)),
             e_omega=np.zeros(0), e_cam=np.zeros((0, 5)))
    g = cugo.graph_from_arrays(d, plan_only=True)
    g.add_point_edges(np.array([0, 1, 1, 2], np.int32), rng.normal(size=(4, 3)), rng.normal(size=(4, 3)))
    g.initialize()
    assert g.n_point_edges() == 3 and g.n_active_edges() == 3 and g.structure_stats()["hsc_blocks"] == 2
    g.close()


@pytest.mark.parametrize("where", ["p", "z", "information"])
def test_non_finite_values_are_refused(where):
    d, g = small_graph()
    ids, p, z, info = point_args()
    if where == "p":
        p[1, 2] = np.nan
    elif where == "z":
        z[0, 0] = np.inf
    else:
        info[2, 0, 1] = info[2, 1, 0] = np.inf
    g.add_point_edges(ids, p, z, info)
    refused(g, "point-to-point edge .*non-finite")


def test_asymmetric_or_indefinite_information_is_refused_and_semi_definite_is_taken():
    ids, p, z, info = point_args()
    d, g = small_graph()
    bad = info.copy()
    bad[0, 0, 2] += 1e-9
    g.add_point_edges(ids, p, z, bad)
    refused(g, "point-to-point edge 0 .*not symmetric")
    d, g = small_graph()
    ok = info.copy()
    ok[1, 0, 2] += 1e-13                                   # (inside 1e-12 max|Omega|)
    g.add_point_edges(ids, p, z, ok)
    g.initialize()
    g.close()
    Q = np.linalg.qr(np.random.default_rng(2).normal(size=(3, 3)))[0]
    d, g = small_graph()
    neg = Q @ np.diag([5.0, 1.0, -1e-9]) @ Q.T
    g.add_point_edges(ids[:1], p[:1], z[:1], 0.5 * (neg + neg.T))
    refused(g, "point-to-point edge .*positive semi-definite")
    # rank 1 (a plane), rank 2 (a line) and the zero matrix are legal
    d, g = small_graph()
    n = Q[:, 0]
    g.add_point_edges(ids[:3], p[:3], z[:3], np.array([np.outer(n, n), np.eye(3) - np.outer(n, n), np.zeros((3, 3))]))
    g.initialize()
    assert g.n_point_edges() == 3
    g.close()
    # without per-edge information the set's matrix is the one that counts, and the one that is checked
    d, g = small_graph(per_edge_information=False)
    g.add_point_edges(ids, p, z, bad)                      # (the edges' own matrices are not looked at)
    g.initialize()
    assert g.n_point_edges() == 3
    g.set_point_information(-np.eye(3))
    refused(g, "point-to-point edge set .*positive semi-definite")


def test_unknown_pose_id_is_refused_and_adds_nothing():
    d, g = small_graph()
    ids, p, z, info = point_args()
    ids[1] = 77
    with pytest.raises(cugo.CugoError, match="unknown pose id 77"):
        g.add_point_edges(ids, p, z, info)
    g.initialize()
    assert g.n_point_edges() == 0
    g.close()


def test_sharded_optimiser_refuses_point_sets_that_count():
    d, g = small_graph()
    g.add_point_edges(*point_args())
    g.set_shard(0, 2, lambda ptr, n, op: None)
    refused(g, r"point-to-point edge sets \(PointEdgeSet\) are not supported on a landmark-sharded")
    d, g = small_graph()
    g.add_point_edges(*point_args(poses=(0, 0)))           # the fixed pose only
    g.set_shard(0, 2, lambda ptr, n, op: None)
    g.initialize()
    assert g.n_point_edges() == 0
    g.close()


def test_estimates_only_initialize_with_point_sets():
    d, g = small_graph()
    g.add_point_edges(*point_args())
    g.initialize()
    assert g.flatten_reuses() == 0 and g.n_point_edges() == 3
    g.set_landmarks(np.arange(len(d["lm"]), dtype=np.int32), d["lm"] + 0.01)
    g.initialize()
    assert g.flatten_reuses() == 1 and g.n_point_edges() == 3
    g.add_point_edges(*point_args(poses=(3,)))             # an edge more: a new flattening
    g.initialize()
    assert g.flatten_reuses() == 1 and g.n_point_edges() == 4
    g.initialize()
    assert g.flatten_reuses() == 2
    g.set_point_robust_kernel(cugo.RK_CAUCHY, 2.0)         # the set's robust kernel or matrix touched: a new flattening, too
    g.initialize()
    assert g.flatten_reuses() == 2
    g.set_point_information(2.0 * np.eye(3))
    g.initialize()
    assert g.flatten_reuses() == 2
    g.close()


GRAPH_PROGRAM = r"""
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>
#include "ba_types.h"
#include "cuda_graph_optimisation.h"
#include "icp_types.h"
#include "point_edge_types.h"
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)
static bool refuses(cugo::CudaGraphOptimisationImpl& opt, const char* what)
{
    try { opt.initialize(); } catch (const std::runtime_error& e) { return std::string(e.what()).find(what) != std::string::npos; }
    return false;
}
int main()
{
    cugo::GraphOptimisationOptions options;
    options.perEdgeInformation = true;
    options.poseEdgeOutlierRejection = true;
    options.planOnly = true;
    cugo::CudaGraphOptimisationImpl opt(options);
    cugo::PoseVertexSet poses(false);
    cugo::PoseVertex p0(0, cugo::Se3D(), true), p1(1, cugo::Se3D(), false), p2(2, cugo::Se3D(), false);
    poses.addVertex(&p0), poses.addVertex(&p1), poses.addVertex(&p2);
    cugo::PointEdgeSet points;
    CHECK(points.dim() == 3);
    for (int i = 0; i < 9; i++)
        CHECK(points.informationMatrix()[i] == (i % 4 == 0 ? 1.0 : 0.0));
    cugo::PointToPointMatch<double> dflt;
    CHECK(dflt.pointP[0] == 0 && dflt.pointZ[2] == 0 && dflt.information[0] == 1 && dflt.information[1] == 0 && dflt.information[8] == 1);
    const double p[3] = {1, 0, 0}, z[3] = {1.5, 2, 3.5}, info[9] = {4, 1, 0, 1, 1, 0, 0, 0, 2};
    std::vector<cugo::PointEdge> pe(4);
    cugo::PoseVertex* on[4] = {&p1, &p1, &p2, &p0}; // the last one sits on the fixed pose
    for (int i = 0; i < 4; i++)
    {
        pe[i].setMeasurement(cugo::PointToPointMatch<double>(p, z, info));
        pe[i].setVertex(on[i], 0);
        points.addEdge(&pe[i]);
    }
    const auto* pm = static_cast<const cugo::PointToPointMatch<double>*>(pe[1].measurementData());
    CHECK(pm->information[1] == 1.0 && pm->pointZ[2] == 3.5 && pm->pointP[0] == 1.0);
    points.setRobustKernel(cugo::RobustKernelType::Huber, 1.5);
    opt.addVertexSet(&poses);
    opt.addEdgeSet(&points); // alone: no landmark set, no BA set
    opt.initialize();
    CHECK(opt.nPointEdges() == 3 && points.nActiveEdges() == 3 && opt.nActiveEdges() == 3);
    pe[0].inactivate();
    opt.initialize();
    CHECK(opt.nPointEdges() == 2 && opt.flattenReuses() == 0);
    {   // the flattened arrays: the inactive edge 0 and edge 3 on the fixed pose are gone, edge 1 (pose 1) before edge 2 (pose 2)
        std::vector<int> fp, fs;
        std::vector<double> vp, vz, vi;
        const int n_info = opt.flatPointEdges(fp, fs, vp, vz, vi);
        CHECK(fp.size() == 2 && fs[0] == 1 && fs[1] == 2 && fp[0] == 0 && fp[1] == 1);
        CHECK(n_info == 1 && vi.size() == 6); // (all matrices equal: one column) 00 01 02 11 12 22
        CHECK(vi[0] == 4 && vi[1] == 1 && vi[2] == 0 && vi[3] == 1 && vi[4] == 0 && vi[5] == 2);
        CHECK(vp.size() == 6 && vp[0] == 1 && vp[1] == 1 && vp[2] == 0 && vz[0] == 1.5 && vz[2] == 2 && vz[4] == 3.5);
    }
    opt.initialize();
    CHECK(opt.flattenReuses() == 1);
    // changed estimates alone re-use the flattening
    p1.setEstimate(cugo::Se3D());
    opt.initialize();
    CHECK(opt.flattenReuses() == 2);
    // touching a measurement through the mutable pointer, or the set's matrix, forces a new flattening
    static_cast<cugo::PointToPointMatch<double>*>(pe[1].getMeasurement())->information[0] = 5.0;
    opt.initialize();
    CHECK(opt.flattenReuses() == 2);
    points.setInformationMatrix(info);
    opt.initialize();
    CHECK(opt.flattenReuses() == 2);
    // an outlier threshold on the set is refused although poseEdgeOutlierRejection is on, with the feature in the message
    points.setOutlierThreshold(5.0);
    CHECK(refuses(opt, "outlier rejection is not supported on PointEdgeSet yet"));
    points.setOutlierThreshold(0.0);
    opt.initialize();
    // next to a plane set
    cugo::PlaneEdgeSet planes;
    cugo::PlaneEdge pl;
    const double nrm[3] = {0, 0, 1};
    pl.setVertex(&p2, 0);
    pl.setMeasurement(cugo::PointToPlaneMatch<double>(cugo::Vec3d(nrm), 0.5, cugo::Vec3d(p)));
    pl.setInformation(1.0);
    planes.addEdge(&pl);
    opt.addEdgeSet(&planes);
    opt.initialize();
    CHECK(opt.nPointEdges() == 2 && opt.nIcpEdges(0) == 1 && opt.nActiveEdges() == 3);
    // a second set with another robust kernel is refused; with the same one it is taken
    cugo::PointEdgeSet points2;
    cugo::PointEdge extra;
    extra.setVertex(&p2, 0);
    points2.addEdge(&extra);
    opt.addEdgeSet(&points2);
    CHECK(refuses(opt, "point-to-point edge sets of one optimiser must use the same robust kernel"));
    points2.setRobustKernel(cugo::RobustKernelType::Huber, 1.5);
    opt.initialize();
    CHECK(opt.nPointEdges() == 3);
    // an edge on a pose vertex of no vertex set of the optimiser is refused
    cugo::PoseVertexSet other(false);
    cugo::PoseVertex w(9, cugo::Se3D(), false);
    other.addVertex(&w);
    cugo::PointEdge stray;
    stray.setVertex(&w, 0);
    points2.addEdge(&stray);
    CHECK(refuses(opt, "its pose vertex is in no pose vertex set"));
    std::printf("OK\n");
    return 0;
}
"""


def test_cpp_point_sets_are_taken_by_a_plan_only_optimiser(tmp_path):
    src = tmp_path / "point_graph.cpp"
    src.write_text(GRAPH_PROGRAM)
    exe = tmp_path / "point_graph"
    lib_dir = os.path.dirname(cugo.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", INC, str(src), "-L", lib_dir, "-lcugo_hip",
                        "-Wl,-rpath," + lib_dir, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr


LAYOUT_PROGRAM = r"""
#include <cstddef>
#include <cstdio>
#include "cugo_hip.h"
#define F(x) std::printf("%s %zu\n", #x, offsetof(cugo_point_edges, x));
int main()
{
    F(n_poses_total) F(n_poses_free) F(n) F(d_pose) F(d_pose_ptr) F(d_p) F(d_z) F(d_info) F(n_info) F(d_flags) F(rk) F(delta)
    std::printf("sizeof %zu\n", sizeof(cugo_point_edges));
    return 0;
}
"""


def test_ctypes_layout_of_point_edges_matches_the_c_struct(tmp_path):
    src = tmp_path / "layout.cpp"
    src.write_text(LAYOUT_PROGRAM)
    exe = tmp_path / "layout"
    r = subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split("\n") if line)
    assert len(out) == len(cugo.PointEdges._fields_) + 1
    for name, _ in cugo.PointEdges._fields_:
        assert int(out[name]) == getattr(cugo.PointEdges, name).offset, name
    assert int(out["sizeof"]) == C.sizeof(cugo.PointEdges)
