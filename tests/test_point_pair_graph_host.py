"""Pose-pose point edge sets (PointPairEdgeSet, point_pair_types.h) without a GPU: what a plan-only optimiser accepts, counts
and hands the kernels; the blocks the Schur complement's pattern gains; every refusal with its message; the flattening
re-used for new estimates; and the C++ interface, compiled with plain g++ against the public headers."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import point_pair_lm_ref as L
import point_pair_ref as PP
import relpose_lm_ref as RL
from conftest import ROOT

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
INC = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "include")

SYMBOLS = ["cugo_graph_add_point_pair_edges", "cugo_graph_set_point_pair_information", "cugo_graph_set_point_pair_robust_kernel",
           "cugo_graph_set_point_pair_outlier_threshold", "cugo_graph_set_point_pair_active", "cugo_graph_n_point_pair_edges",
           "cugo_graph_get_flat_point_pair_edges"]


def test_graph_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "cugo_hip.h")).read()
    for s in SYMBOLS:
        assert hasattr(cugo.lib(), s) and s + "(" in header, s
    for name in ("add_point_pair_edges", "set_point_pair_information", "set_point_pair_robust_kernel", "set_point_pair_active",
                 "n_point_pair_edges", "flat_point_pair_edges"):
        assert hasattr(cugo.Graph, name), name


def scan_graph(plan_only=True, **kw):
    d, icp, prior, pts, rp, pairs = L.multi_scan_case()
    return d, pairs, L.build_graph(d, icp, prior, pts, rp, None, plan_only=plan_only, **kw)


def refused(g, what):
    with pytest.raises(cugo.CugoError, match=what):
        g.initialize()
    g.close()


def test_plan_only_graph_takes_the_set_and_counts_what_counts():
    d, pairs, g = scan_graph()
    fixed = int(np.flatnonzero(d["pose_fixed"])[0])
    extra = dict(pairs, a=np.concatenate([pairs["a"], [fixed, 0]]), b=np.concatenate([pairs["b"], [fixed - 1, fixed]]),
                 p=np.concatenate([pairs["p"], pairs["p"][:2]]), z=np.concatenate([pairs["z"], pairs["z"][:2]]),
                 info=np.concatenate([pairs["info"], pairs["info"][:2]]), active=np.concatenate([pairs["active"], [True, True]]))
    L.add_pairs(g, extra)
    g.initialize()
    n = L.counting_edges(d, extra)
    assert g.n_point_pair_edges() == n == int(extra["active"].sum()) and g.n_active_edges() == n   # (one fixed end: counts)
    assert (~extra["active"]).sum() > 5
    P = int((np.asarray(d["pose_fixed"]) == 0).sum())
    assert g.structure_stats()["hsc_blocks"] == P + len(L.pair_blocks(d, extra))
    g.close()


def test_the_flattened_arrays_are_in_the_order_of_the_plan():
    d, pairs, g = scan_graph()
    L.add_pairs(g, pairs)
    g.initialize()
    f = g.flat_point_pair_edges()
    a, b, P = L.free_first_pairs(d, pairs)
    keep = np.flatnonzero(pairs["active"] & ((a < P) | (b < P)))
    plan = PP.numpy_plan(a[keep], b[keep], None, P)
    order = keep[plan["perm"]]
    assert np.array_equal(f["pose_a"], a[order]) and np.array_equal(f["pose_b"], b[order]) and np.array_equal(f["src"], order)
    assert np.array_equal(f["p"], pairs["p"][order].T) and np.array_equal(f["z"], pairs["z"][order].T)
    sym = 0.5 * (pairs["info"] + pairs["info"].transpose(0, 2, 1))      # (the symmetric part is what is flattened)
    assert f["n_info"] == len(order) and np.array_equal(f["info"], PP.pack(sym[order]).T)
    g.close()
    # one matrix for all: one column
    d, pairs, g = scan_graph(per_edge_information=False)
    L.add_pairs(g, pairs)
    g.set_point_pair_information(np.diag([1.0, 2.0, 3.0]))
    g.initialize()
    f = g.flat_point_pair_edges()
    assert f["n_info"] == 1 and np.array_equal(f["info"][:, 0], [1, 0, 0, 2, 0, 3])
    g.close()


def test_the_pattern_gains_exactly_the_pair_blocks():
    """next to BA edges and a relative-pose set: a pair that is co-visible or already joined gains nothing, a new pair
    one block"""
    d, icp, prior, pts, rp, pairs = L.mixed_case()
    g = L.build_graph(d, icp, prior, pts, rp, None, plan_only=True)
    g.initialize()
    before = g.structure_stats()["hsc_blocks"]
    assert before == RL.union_pattern_blocks(d, rp)
    g.close()
    have = RL.covisible_pairs(d) | RL.relpose_pairs(d, rp)
    assert L.pair_blocks(d, pairs) <= have                      # every free-free pair of the recipe is there already
    g = L.build_graph(d, icp, prior, pts, rp, pairs, plan_only=True)
    g.initialize()
    assert g.structure_stats()["hsc_blocks"] == before and g.n_point_pair_edges() == L.counting_edges(d, pairs)
    g.close()
    # a relative-pose-free, landmark-free graph: the blocks are the pairs
    d, pairs, g = scan_graph()
    L.add_pairs(g, pairs)
    g.initialize()
    assert g.structure_stats()["hsc_blocks"] == 5 + len(L.pair_blocks(d, pairs)) == 5 + 6     # (two of the 8 pairs touch the fixed pose)
    g.set_point_pair_active(np.where((pairs["a"] == 0) & (pairs["b"] == 3), False, pairs["active"]))
    g.initialize()
    assert g.structure_stats()["hsc_blocks"] == 5 + 5           # the chord's only edges switched off: one block fewer
    g.close()


def test_flatten_reuse_covers_the_set():
    d, pairs, g = scan_graph()
    L.add_pairs(g, pairs)
    g.initialize()
    n = g.n_point_pair_edges()
    assert g.flatten_reuses() == 0
    ids = np.arange(len(d["pose"]), dtype=np.int32)
    g.set_poses(ids, d["pose_gt"])
    g.initialize()
    assert g.flatten_reuses() == 1 and g.n_point_pair_edges() == n
    g.add_point_pair_edges([1], [3], [[0, 0, 1.0]], [[0, 1.0, 0]], np.eye(3)[None])      # an edge more: a new flattening
    g.initialize()
    assert g.flatten_reuses() == 1 and g.n_point_pair_edges() == n + 1
    g.initialize()
    assert g.flatten_reuses() == 2
    g.set_point_pair_robust_kernel(cugo.RK_CAUCHY, 2.0)          # the set touched: a new flattening, too
    g.initialize()
    assert g.flatten_reuses() == 2
    g.close()


# ------------------------------------------------------------------ refusals
def test_outlier_threshold_on_the_set_is_refused():
    d, pairs, g = scan_graph()
    L.add_pairs(g, pairs)
    g.set_option("pose_edge_outliers", 1)
    g.set_point_pair_outlier_threshold(5.0)
    refused(g, "outlier rejection is not supported on PointPairEdgeSet yet")
    d, pairs, g = scan_graph()
    L.add_pairs(g, pairs)
    g.set_point_pair_outlier_threshold(0.0)
    g.initialize()
    g.close()


def test_sharded_optimiser_refuses_the_set():
    d, pairs, g = scan_graph()
    L.add_pairs(g, pairs)
    g.set_shard(0, 2, lambda ptr, n, op: None)
    refused(g, r"pose-pose point edge sets \(PointPairEdgeSet\) are not supported on a landmark-sharded")


def test_row_strip_form_of_the_schur_complement_is_refused(monkeypatch):
    monkeypatch.setenv("CUGO_HSC_STRIP", "1")
    d, pairs, g = scan_graph()
    L.add_pairs(g, pairs)
    refused(g, r"PointPairEdgeSet\) cannot be combined with CUGO_HSC_STRIP=1")
    d, pairs, g = scan_graph()      # (no edge that counts: nothing to refuse)
    L.add_pairs(g, dict(pairs, active=np.zeros(len(pairs["a"]), bool)))
    g.initialize()
    assert g.n_point_pair_edges() == 0
    g.close()


def test_the_new_kind_is_no_public_outlier_kind():
    d, pairs, g = scan_graph()
    L.add_pairs(g, pairs)
    g.initialize()
    for kind in (4, 5):
        with pytest.raises(cugo.CugoError):
            g.n_pose_edge_outliers(kind)
        with pytest.raises(cugo.CugoError):
            g.pose_edge_active(kind, 1)
    g.close()


def test_a_pose_joined_to_itself_and_an_unknown_id_add_nothing():
    d, pairs, g = scan_graph()
    one = (np.zeros((1, 3)), np.ones((1, 3)), np.eye(3)[None])
    with pytest.raises(cugo.CugoError, match="joins pose 2 to itself"):
        g.add_point_pair_edges([0, 2], [1, 2], np.zeros((2, 3)), np.ones((2, 3)), np.tile(np.eye(3), (2, 1, 1)))
    with pytest.raises(cugo.CugoError):
        g.add_point_pair_edges([77], [1], *one)
    g.initialize()
    assert g.n_point_pair_edges() == 0
    g.close()


@pytest.mark.parametrize("where", ["p", "z", "info"])
def test_non_finite_values_are_refused(where):
    d, pairs, g = scan_graph()
    bad = {k: np.array(pairs[k], np.float64) for k in ("p", "z", "info")}
    bad[where].reshape(len(pairs["a"]), -1)[7, 1] = np.nan
    assert pairs["active"][7]
    L.add_pairs(g, dict(pairs, **bad))
    refused(g, r"pose-pose point edge 7 of edge set \d+: non-finite")


def test_asymmetric_or_indefinite_information_is_refused_and_semi_definite_is_taken():
    for M, what in ((np.array([[1, 0.1, 0], [0, 1, 0], [0, 0, 1.0]]), "not symmetric"), (np.diag([1.0, 1.0, -1e-3]), "not positive semi-definite")):
        d, pairs, g = scan_graph()
        info = pairs["info"].copy()
        info[3] = M
        assert pairs["active"][3]
        L.add_pairs(g, dict(pairs, info=info))
        refused(g, r"pose-pose point edge 3 of edge set \d+: the information matrix is " + what)
    d, pairs, g = scan_graph()
    info = pairs["info"].copy()
    info[3], info[4] = np.diag([1.0, 0, 0]), np.zeros((3, 3))
    L.add_pairs(g, dict(pairs, info=info))
    g.initialize()
    g.close()
    d, pairs, g = scan_graph(per_edge_information=False)
    L.add_pairs(g, pairs)
    g.set_point_pair_information(-np.eye(3))
    refused(g, r"pose-pose point edge set \d+: .*positive semi-definite")


GRAPH_PROGRAM = r"""
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>
#include "ba_types.h"
#include "cuda_graph_optimisation.h"
#include "point_pair_types.h"
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
    cugo::PoseVertex p0(0, cugo::Se3D(), true), p1(1, cugo::Se3D(), false), p2(2, cugo::Se3D(), false), p3(3, cugo::Se3D(), true);
    poses.addVertex(&p0), poses.addVertex(&p1), poses.addVertex(&p2), poses.addVertex(&p3);
    cugo::PointPairEdgeSet pairs;
    CHECK(pairs.dim() == 3);
    for (int i = 0; i < 9; i++)
        CHECK(pairs.informationMatrix()[i] == (i % 4 == 0 ? 1.0 : 0.0));
    const double p[3] = {1, 0, 0}, z[3] = {1.5, 2, 3.5}, info[9] = {4, 1, 0, 1, 1, 0, 0, 0, 2};
    std::vector<cugo::PointPairEdge> pe(5);
    cugo::PoseVertex* a[5] = {&p2, &p1, &p1, &p0, &p0};
    cugo::PoseVertex* b[5] = {&p1, &p2, &p0, &p3, &p2}; // 2->1, 1->2, 1->fixed, fixed->fixed, fixed->2
    for (int i = 0; i < 5; i++)
    {
        pe[i].setMeasurement(cugo::PointToPointMatch<double>(p, z, info));
        pe[i].setVertex(a[i], 0), pe[i].setVertex(b[i], 1);
        pairs.addEdge(&pe[i]);
    }
    pairs.setRobustKernel(cugo::RobustKernelType::Huber, 1.5);
    opt.addVertexSet(&poses);
    opt.addEdgeSet(&pairs); // alone: no landmark set, no BA set
    opt.initialize();
    CHECK(opt.nPointPairEdges() == 4 && pairs.nActiveEdges() == 4 && opt.nActiveEdges() == 4); // the fixed-fixed edge is dropped
    {   // the plan's order: (lo, hi, orientation) with free poses first: 1 -> index 0, 2 -> index 1, fixed 0 -> 2, fixed 3 -> 3
        std::vector<int> fa, fb, fs;
        std::vector<double> vp, vz, vi;
        const int n_info = opt.flatPointPairEdges(fa, fb, fs, vp, vz, vi);
        CHECK(fa.size() == 4 && n_info == 1 && vi.size() == 6 && vi[0] == 4 && vi[1] == 1 && vi[3] == 1 && vi[5] == 2);
        CHECK(fs[0] == 1 && fa[0] == 0 && fb[0] == 1);  // 1->2: (0, 1, a is lo)
        CHECK(fs[1] == 0 && fa[1] == 1 && fb[1] == 0);  // 2->1: (0, 1, a is hi)
        CHECK(fs[2] == 2 && fa[2] == 0 && fb[2] == 2);  // 1->fixed 0
        CHECK(fs[3] == 4 && fa[3] == 2 && fb[3] == 1);  // fixed 0->2
        CHECK(vp.size() == 12 && vp[0] == 1 && vp[4] == 0 && vz[0] == 1.5 && vz[4] == 2 && vz[8] == 3.5);
    }
    opt.initialize();
    CHECK(opt.flattenReuses() == 1);
    static_cast<cugo::PointToPointMatch<double>*>(pe[1].getMeasurement())->information[0] = 5.0; // the mutable pointer: a change
    opt.initialize();
    CHECK(opt.flattenReuses() == 1);
    pe[0].inactivate();
    opt.initialize();
    CHECK(opt.nPointPairEdges() == 3);
    // an outlier threshold on the set is refused although poseEdgeOutlierRejection is on
    pairs.setOutlierThreshold(5.0);
    CHECK(refuses(opt, "outlier rejection is not supported on PointPairEdgeSet yet"));
    pairs.setOutlierThreshold(0.0);
    opt.initialize();
    // a second set with another robust kernel is refused; with the same one it is taken
    cugo::PointPairEdgeSet pairs2;
    cugo::PointPairEdge extra;
    extra.setVertex(&p2, 0), extra.setVertex(&p1, 1);
    pairs2.addEdge(&extra);
    opt.addEdgeSet(&pairs2);
    CHECK(refuses(opt, "pose-pose point edge sets of one optimiser must use the same robust kernel"));
    pairs2.setRobustKernel(cugo::RobustKernelType::Huber, 1.5);
    opt.initialize();
    CHECK(opt.nPointPairEdges() == 4);
    // a == b and a vertex of no vertex set of the optimiser are refused
    cugo::PointPairEdge self;
    self.setVertex(&p1, 0), self.setVertex(&p1, 1);
    pairs2.addEdge(&self);
    CHECK(refuses(opt, "it joins a pose to itself (a == b)"));
    self.inactivate();
    opt.initialize();
    cugo::PoseVertexSet other(false);
    cugo::PoseVertex w(9, cugo::Se3D(), false);
    other.addVertex(&w);
    cugo::PointPairEdge stray;
    stray.setVertex(&p1, 0), stray.setVertex(&w, 1);
    pairs2.addEdge(&stray);
    CHECK(refuses(opt, "one of its pose vertices is in no pose vertex set"));
    std::printf("OK\n");
    return 0;
}
"""


def test_cpp_pair_sets_are_taken_by_a_plan_only_optimiser(tmp_path):
    src = tmp_path / "pair_graph.cpp"
    src.write_text(GRAPH_PROGRAM)
    exe = tmp_path / "pair_graph"
    lib_dir = os.path.dirname(cugo.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", INC, str(src), "-L", lib_dir, "-lcugo_hip",
                        "-Wl,-rpath," + lib_dir, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
