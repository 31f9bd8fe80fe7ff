"""CPU checks of the covariance form of the two point kinds (no GPU): the symbols of the kernel-level C ABI, exported,
declared and wrapped; the ctypes mirrors of cugo_gicp_edges and cugo_gicp_pair_edges against the C structs, and the
information-form structs unchanged beside them; refusals that need no device."""
import ctypes as C
import importlib
import os
import re
import subprocess

import pytest

from conftest import ROOT

cugo = importlib.import_module("cuda-bundle-adjustment_amd")

SYMBOLS = ["cugo_gicp_compute_errors", "cugo_gicp_construct_quadratic_form", "cugo_gicp_construct_quadratic_form_schur",
           "cugo_gicp_pair_compute_errors", "cugo_gicp_pair_construct_quadratic_form", "cugo_gicp_pair_construct_quadratic_form_schur",
           "cugo_gicp_pair_construct_quadratic_form_diag", "cugo_gicp_pair_add_offdiag_schur"]


def test_symbols_are_exported_declared_and_wrapped():
    header = open(os.path.join(ROOT, "include", "cugo_hip.h")).read()
    for s in SYMBOLS:
        assert hasattr(cugo.lib(), s), s
        assert re.search(r"\b%s\(" % s, header), s
        assert callable(getattr(cugo, s[len("cugo_"):])), s
    assert "typedef struct cugo_gicp_edges" in header and "typedef struct cugo_gicp_pair_edges" in header
    assert hasattr(cugo, "GicpEdges") and hasattr(cugo, "GicpPairEdges")


LAYOUT_PROGRAM = r"""
#include <cstddef>
#include <cstdio>
#include "cugo_hip.h"
#define F(x) std::printf("%s %zu\n", #x, offsetof(S, x));
int main()
{
    {
        typedef cugo_gicp_edges S;
        std::printf("struct gicp\n");
        F(n_poses_total) F(n_poses_free) F(n) F(d_pose) F(d_pose_ptr) F(d_p) F(d_z) F(d_cov_p) F(d_cov_z) F(n_cov) F(d_flags) F(rk) F(delta)
        std::printf("sizeof %zu\n", sizeof(S));
    }
    {
        typedef cugo_gicp_pair_edges S;
        std::printf("struct pair\n");
        F(n_poses_total) F(n_poses_free) F(n) F(d_pose_a) F(d_pose_b) F(d_p) F(d_z) F(d_cov_p) F(d_cov_z) F(n_cov) F(d_flags) F(rk) F(delta) F(plan)
        std::printf("sizeof %zu\n", sizeof(S));
    }
    std::printf("struct info\nsizeof_point %zu\nsizeof_point_pair %zu\n", sizeof(cugo_point_edges), sizeof(cugo_point_pair_edges));
    return 0;
}
"""


def test_ctypes_layouts_match_the_c_structs(tmp_path):
    src = tmp_path / "layout.cpp"
    src.write_text(LAYOUT_PROGRAM)
    exe = tmp_path / "layout"
    r = subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out, cur = {}, None
    for line in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split("\n"):
        if line.startswith("struct "):
            cur = out.setdefault(line.split()[1], {})
        elif line:
            cur[line.split()[0]] = int(line.split()[1])
    for key, cls in (("gicp", cugo.GicpEdges), ("pair", cugo.GicpPairEdges)):
        assert len(out[key]) == len(cls._fields_) + 1
        for name, _ in cls._fields_:
            assert out[key][name] == getattr(cls, name).offset, (key, name)
        assert out[key]["sizeof"] == C.sizeof(cls)
    # the members of the information form with d_info, n_info replaced by d_cov_p, d_cov_z, n_cov: one pointer more; the
    # information-form structs have not grown
    swap = lambda fields: [n for n, _ in fields if n not in ("d_info", "n_info", "d_cov_p", "d_cov_z", "n_cov")]
    assert swap(cugo.GicpEdges._fields_) == swap(cugo.PointEdges._fields_)
    assert swap(cugo.GicpPairEdges._fields_) == swap(cugo.PointPairEdges._fields_)
    assert out["info"]["sizeof_point"] == C.sizeof(cugo.PointEdges) and out["info"]["sizeof_point_pair"] == C.sizeof(cugo.PointPairEdges)


@pytest.mark.parametrize("fn", ["cugo_gicp_pair_compute_errors", "cugo_gicp_pair_construct_quadratic_form_diag"])
def test_pair_calls_without_a_context_or_a_plan_are_refused(fn):
    ev = cugo.GicpPairEdges()
    lib = cugo.lib()
    args = [None, C.byref(ev), None, None, None] + ([None] if fn.endswith("_diag") else [])
    assert getattr(lib, fn)(*args) == -3
    assert b"cugo_gicp_pair: no context" in lib.cugo_last_error()
    assert getattr(lib, fn)(None, None, *args[2:]) == -3


# ------------------------------------------------------------------ plan-only graphs (no GPU)
import numpy as np  # noqa: E402

import gicp_lm_ref as G  # noqa: E402
import point_pair_lm_ref as PPL  # noqa: E402

GRAPH_SYMBOLS = ["cugo_graph_add_gicp_edges", "cugo_graph_add_gicp_pair_edges", "cugo_graph_set_gicp_robust_kernel",
                 "cugo_graph_set_gicp_pair_robust_kernel", "cugo_graph_set_gicp_pair_active", "cugo_graph_n_gicp_edges",
                 "cugo_graph_n_gicp_pair_edges", "cugo_graph_get_flat_gicp_edges", "cugo_graph_get_flat_gicp_pair_edges"]
INC = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "include")


def test_graph_symbols_are_exported_declared_and_wrapped():
    header = open(os.path.join(ROOT, "include", "cugo_hip.h")).read()
    for s in GRAPH_SYMBOLS:
        assert hasattr(cugo.lib(), s), s
        assert re.search(r"\b%s\(" % s, header), s
    for m in ("add_gicp_edges", "add_gicp_pair_edges", "set_gicp_robust_kernel", "set_gicp_pair_robust_kernel", "set_gicp_pair_active",
              "n_gicp_edges", "n_gicp_pair_edges", "flat_gicp_edges", "flat_gicp_pair_edges"):
        assert callable(getattr(cugo.Graph, m)), m


def pair_graph(**kw):
    d, icp, prior, pts, rp, gpts, gpairs = G.multi_scan_case()
    return d, gpairs, G.build_graph(d, icp, prior, pts, rp, None, None, plan_only=True, **kw)


def refused(g, what):
    with pytest.raises(cugo.CugoError, match=what):
        g.initialize()
    g.close()


def tri(C):
    C = np.asarray(C).reshape(-1, 3, 3)
    return np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]])


def test_pair_flattening_order_inactive_edges_and_the_collapse():
    d, gp, g = pair_graph()
    fixed = int(np.flatnonzero(d["pose_fixed"])[0])
    n0 = len(gp["a"])
    cat = lambda k, extra: np.concatenate([gp[k], extra])
    more = dict(gp, a=cat("a", [fixed]), b=cat("b", [fixed - 1]), p=cat("p", gp["p"][:1]), z=cat("z", gp["z"][:1]),
                cov_p=cat("cov_p", gp["cov_p"][:1]), cov_z=cat("cov_z", gp["cov_z"][:1]), active=cat("active", [True]))
    G.add_gicp(g, None, more)
    g.initialize()
    assert not np.all(gp["active"])
    assert g.n_gicp_pair_edges() == int(gp["active"].sum()) + 1 == g.n_active_edges() and g.n_point_pair_edges() == 0 and g.n_gicp_edges() == 0
    f = g.flat_gicp_pair_edges()
    assert f["n_cov"] == len(f["src"]) == g.n_gicp_pair_edges()
    empty = g.flat_point_pair_edges()                                   # the information-form getter sees no edge of this form
    assert empty["n_info"] == 0 and all(np.asarray(empty[k]).size == 0 for k in ("pose_a", "src", "p", "z", "info"))
    assert g.flat_point_edges()["src"].size == 0                        # (the unary kind is empty and in the information form)
    src = f["src"]
    assert np.all(more["active"][src]) and n0 in src                    # inactive edges are dropped, the fixed-to-free edge is kept
    lo, hi = np.minimum(f["pose_a"], f["pose_b"]), np.maximum(f["pose_a"], f["pose_b"])
    key = list(zip(lo, hi, f["pose_a"] > f["pose_b"], src))
    assert key == sorted(key)                                           # the plan's order: (lo, hi, orientation), stable
    assert np.array_equal(f["p"].T, more["p"][src]) and np.array_equal(f["z"].T, more["z"][src])
    assert np.array_equal(f["cov_p"], tri(more["cov_p"][src])) and np.array_equal(f["cov_z"], tri(more["cov_z"][src]))
    g.close()
    # one covariance pair for all collapses to n_cov = 1 (the C++ program below holds the edge between two fixed poses)
    d, gp, g = pair_graph()
    one = dict(gp, cov_p=np.tile(gp["cov_p"][:1], (n0, 1, 1)), cov_z=np.tile(gp["cov_z"][:1], (n0, 1, 1)))
    G.add_gicp(g, None, one)
    g.initialize()
    f = g.flat_gicp_pair_edges()
    assert f["n_cov"] == 1 and f["cov_p"].shape == (6, 1) and np.array_equal(f["cov_z"], tri(gp["cov_z"][:1]))
    g.close()


def test_unary_flattening():
    d, icp, prior, pts, rp, gpts, _ = G.scan_to_map_case()
    g = G.build_graph(d, icp, prior, pts, rp, gpts, None, plan_only=True)
    g.initialize()
    fixed = int(np.flatnonzero(d["pose_fixed"])[0])
    keep = np.flatnonzero(gpts["pose"] != fixed)
    assert g.n_gicp_edges() == len(keep) and g.n_point_edges() == 0
    empty = g.flat_point_edges()                                        # (not 12-wide covariances behind a 6-wide header)
    assert empty["n_info"] == 0 and all(np.asarray(empty[k]).size == 0 for k in ("pose", "src", "p", "z", "info"))
    f = g.flat_gicp_edges()
    assert np.all(np.diff(f["pose"]) >= 0) and set(f["src"].tolist()) == set(keep.tolist()) and f["n_cov"] == len(keep)
    assert np.array_equal(f["cov_p"], tri(gpts["cov_p"][f["src"]])) and np.array_equal(f["p"].T, gpts["p"][f["src"]])
    g.close()


def test_refusals_name_the_set(monkeypatch):
    d, gp, g = pair_graph()
    G.add_gicp(g, None, gp)
    g.set_gicp_pair_outlier_threshold(5.0)
    refused(g, "outlier rejection is not supported on GicpPairEdgeSet yet")
    d, gp, g = pair_graph()
    G.add_gicp(g, None, gp)
    g.set_shard(0, 2, lambda ptr, n, op: None)
    refused(g, r"\(GicpPairEdgeSet\) are not supported on a landmark-sharded")
    d, gp, g = pair_graph()
    G.add_gicp(g, None, gp)
    g.add_point_pair_edges(gp["a"][:3], gp["b"][:3], gp["p"][:3], gp["z"][:3], np.tile(np.eye(3), (3, 1, 1)))
    refused(g, r"GicpPairEdgeSet with PointPairEdgeSet\) cannot be combined")
    d, icp, prior, pts, rp, gpts, _ = G.scan_to_map_case()
    g = G.build_graph(d, icp, prior, pts, rp, gpts, None, plan_only=True)
    g.set_gicp_outlier_threshold(1.0)
    refused(g, "outlier rejection is not supported on GicpEdgeSet yet")
    g = G.build_graph(d, icp, prior, pts, rp, gpts, None, plan_only=True)
    g.add_point_edges(gpts["pose"][:2], gpts["p"][:2], gpts["z"][:2], np.tile(np.eye(3), (2, 1, 1)))
    refused(g, r"GicpEdgeSet with PointEdgeSet\) cannot be combined")
    g = G.build_graph(d, icp, prior, pts, rp, gpts, None, plan_only=True)
    g.set_shard(0, 2, lambda ptr, n, op: None)
    refused(g, r"\(GicpEdgeSet\) are not supported on a landmark-sharded")
    monkeypatch.setenv("CUGO_HSC_STRIP", "1")
    d, gp, g = pair_graph()
    G.add_gicp(g, None, gp)
    refused(g, r"GicpPairEdgeSet\) cannot be combined with CUGO_HSC_STRIP=1")


def test_a_point_set_of_the_other_arity_combines():
    d, gp, g = pair_graph()
    G.add_gicp(g, None, gp)
    g.add_point_edges([0, 1], np.zeros((2, 3)), np.ones((2, 3)), np.tile(np.eye(3), (2, 1, 1)))
    g.initialize()
    assert g.n_point_edges() == 2 and g.n_gicp_pair_edges() == int(gp["active"].sum())
    g.close()


def test_unknown_id_and_self_edge_add_nothing():
    d, gp, g = pair_graph()
    c = np.tile(np.eye(3), (2, 1, 1))
    with pytest.raises(cugo.CugoError, match="joins pose 2 to itself"):
        g.add_gicp_pair_edges([0, 2], [1, 2], np.zeros((2, 3)), np.ones((2, 3)), c, c)
    with pytest.raises(cugo.CugoError):
        g.add_gicp_edges([0, 77], np.zeros((2, 3)), np.ones((2, 3)), c, c)
    g.initialize()
    assert g.n_gicp_pair_edges() == 0 and g.n_gicp_edges() == 0
    g.close()


def with_edge7(gp, cov_p=None, cov_z=None, p=None):
    out = dict(gp, cov_p=gp["cov_p"].copy(), cov_z=gp["cov_z"].copy(), p=gp["p"].copy())
    assert gp["active"][7]
    if cov_p is not None:
        out["cov_p"][7] = cov_p
    if cov_z is not None:
        out["cov_z"][7] = cov_z
    if p is not None:
        out["p"][7] = p
    return out


PLANE = np.diag([1.0, 1.0, 0.0])


@pytest.mark.parametrize("what,kw,accepted", [
    ("non-finite point", dict(p=[np.nan, 0, 0]), False),
    ("non-finite covariance covP", dict(cov_p=np.diag([1.0, np.inf, 1.0])), False),
    ("covP is not symmetric", dict(cov_p=np.array([[1, 3e-12, 0], [0, 1, 0], [0, 0, 1.0]])), False),
    ("", dict(cov_p=np.array([[1, 0.3e-12, 0], [0, 1, 0], [0, 0, 1.0]])), True),
    ("covZ is not positive semi-definite", dict(cov_z=np.diag([1.0, 1.0, -3e-12])), False),
    ("", dict(cov_z=np.diag([1.0, 1.0, -0.3e-12]), cov_p=np.eye(3)), True),
    ("", dict(cov_p=PLANE, cov_z=np.diag([1.0, 0.5, 0.1])), True),                       # a planar C_p with a regular C_z
    ("covP and covZ are both singular", dict(cov_p=PLANE, cov_z=PLANE), False),
    ("covP and covZ are both singular", dict(cov_p=PLANE, cov_z=np.diag([1.0, 1.0, 0.3e-12 * 2])), False),
    ("", dict(cov_p=PLANE, cov_z=np.diag([1.0, 1.0, 3e-12 * 2])), True),
])
def test_covariance_checks_at_their_thresholds(what, kw, accepted):
    d, gp, g = pair_graph()
    G.add_gicp(g, None, with_edge7(gp, **kw))
    if accepted:
        g.initialize()
        g.close()
    else:
        refused(g, r"GicpPairEdgeSet edge 7 of edge set \d+: .*" + what)


GRAPH_PROGRAM = r"""
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>
#include "ba_types.h"
#include "cuda_graph_optimisation.h"
#include "gicp_types.h"
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)
static bool refuses(cugo::CudaGraphOptimisationImpl& opt, const char* what)
{
    try { opt.initialize(); } catch (const std::runtime_error& e) { return std::string(e.what()).find(what) != std::string::npos; }
    return false;
}
int main()
{
    cugo::GraphOptimisationOptions options;
    options.planOnly = true;
    cugo::CudaGraphOptimisationImpl opt(options);
    cugo::PoseVertexSet poses(false);
    cugo::PoseVertex p0(0, cugo::Se3D(), true), p1(1, cugo::Se3D(), false), p2(2, cugo::Se3D(), false), p3(3, cugo::Se3D(), true);
    poses.addVertex(&p0), poses.addVertex(&p1), poses.addVertex(&p2), poses.addVertex(&p3);
    const double p[3] = {1, 0, 0}, z[3] = {1.5, 2, 3.5}, cp[9] = {4, 1, 0, 1, 1, 0, 0, 0, 2}, cz[9] = {1, 0, 0, 0, 1, 0, 0, 0, 0};
    cugo::GicpEdgeSet unary;
    cugo::GicpPairEdgeSet pairs;
    CHECK(unary.dim() == 3 && pairs.dim() == 3);
    std::vector<cugo::GicpEdge> ue(3);
    cugo::PoseVertex* on[3] = {&p2, &p0, &p1}; // the edge on the fixed pose is dropped
    for (int i = 0; i < 3; i++)
    {
        ue[i].setMeasurement(cugo::PointCovarianceMatch<double>(p, z, cp, cz));
        ue[i].setVertex(on[i], 0);
        unary.addEdge(&ue[i]);
    }
    std::vector<cugo::GicpPairEdge> pe(4);
    cugo::PoseVertex* a[4] = {&p2, &p1, &p0, &p0};
    cugo::PoseVertex* b[4] = {&p1, &p2, &p2, &p3}; // the last joins two FIXED poses: it counts for nothing
    for (int i = 0; i < 4; i++)
    {
        pe[i].setMeasurement(cugo::PointCovarianceMatch<double>(p, z, cp, cz));
        pe[i].setVertex(a[i], 0), pe[i].setVertex(b[i], 1);
        pairs.addEdge(&pe[i]);
    }
    pairs.setRobustKernel(cugo::RobustKernelType::Huber, 1.5);
    opt.addVertexSet(&poses);
    opt.addEdgeSet(&unary), opt.addEdgeSet(&pairs);
    opt.initialize();
    CHECK(opt.nGicpEdges() == 2 && opt.nGicpPairEdges() == 3 && opt.nPointEdges() == 0 && opt.nPointPairEdges() == 0);
    CHECK(pairs.nActiveEdges() == 3 && unary.nActiveEdges() == 2 && opt.nActiveEdges() == 5); // fixed-fixed and on-fixed edges dropped
    std::vector<int> q, s, fa, fb;
    std::vector<double> vp, vz, c1, c2;
    CHECK(opt.flatGicpEdges(q, s, vp, vz, c1, c2) == 1); // one covariance pair serves all
    CHECK(q.size() == 2 && q[0] == 0 && q[1] == 1 && s[0] == 2 && s[1] == 0);
    const double tp[6] = {4, 1, 0, 1, 0, 2}, tz[6] = {1, 0, 0, 1, 0, 0};
    for (int i = 0; i < 6; i++)
        CHECK(c1[i] == tp[i] && c2[i] == tz[i]);
    CHECK(opt.flatGicpPairEdges(fa, fb, s, vp, vz, c1, c2) == 1 && fa.size() == 3);
    CHECK(fa[0] == 0 && fb[0] == 1 && s[0] == 1 && fa[1] == 1 && fb[1] == 0 && s[1] == 0 && fa[2] == 2 && fb[2] == 1 && s[2] == 2);
    {   // the information-form getters see no edge of a kind in the covariance form
        std::vector<double> vi;
        CHECK(opt.flatPointEdges(q, s, vp, vz, vi) == 0 && q.empty() && vi.empty());
        CHECK(opt.flatPointPairEdges(fa, fb, s, vp, vz, vi) == 0 && fa.empty() && vi.empty());
    }
    // sets of one kind must agree on the robust kernel: the message names the set class
    cugo::GicpPairEdgeSet pairs2;
    cugo::GicpPairEdge more;
    more.setMeasurement(cugo::PointCovarianceMatch<double>(p, z, cp, cz));
    more.setVertex(&p1, 0), more.setVertex(&p2, 1);
    pairs2.addEdge(&more);
    pairs2.setRobustKernel(cugo::RobustKernelType::Huber, 2.5);
    opt.addEdgeSet(&pairs2);
    CHECK(refuses(opt, "the GicpPairEdgeSet edge sets of one optimiser must use the same robust kernel"));
    pairs2.setRobustKernel(cugo::RobustKernelType::Huber, 1.5);
    opt.initialize();
    CHECK(opt.nGicpPairEdges() == 4);
    cugo::GicpEdgeSet unary2;
    cugo::GicpEdge more1;
    more1.setMeasurement(cugo::PointCovarianceMatch<double>(p, z, cp, cz));
    more1.setVertex(&p1, 0);
    unary2.addEdge(&more1);
    unary2.setRobustKernel(cugo::RobustKernelType::Cauchy, 1.0);
    opt.addEdgeSet(&unary2);
    CHECK(refuses(opt, "the GicpEdgeSet edge sets of one optimiser must use the same robust kernel"));
    std::printf("OK\n");
    return 0;
}
"""


def test_cpp_gicp_sets_are_taken_by_a_plan_only_optimiser(tmp_path):
    src = tmp_path / "gicp_graph.cpp"
    src.write_text(GRAPH_PROGRAM)
    exe = tmp_path / "gicp_graph"
    lib_dir = os.path.dirname(cugo.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", INC, str(src), "-L", lib_dir, "-lcugo_hip",
                        "-Wl,-rpath," + lib_dir, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
