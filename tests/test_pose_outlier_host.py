"""Outlier rejection on plane, line, prior and relative-pose edge sets, without a GPU: the design conditions of the
reference cases (tests/pose_outlier_ref.py), the opt-in (GraphOptimisationOptions::poseEdgeOutlierRejection, the graph
option "pose_edge_outliers"), plan-only graphs of every case, the C++ interface, and the host path under CPU sanitizers in
a program of its own."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import pose_outlier_ref as R
from test_relpose_graph_host import INC, HOST, ROCM, ROOT, SAN_SOURCES, c_array

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
PYTHON_CASES = [n for n in R.CASES if n != "icp"]  # (icp holds two plane sets: the C graph object has one)


# ---- the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_cases_meet_their_design_conditions(name):
    """reference() asserts (a) the gap of a factor 2 round every threshold, (b) an accepted last trial, (c) an edge lost
    and an edge kept per set with a threshold; here: what each case was designed to hold on top"""
    r = R.reference(name)
    rej = r["rej"]
    if name == "closures":
        assert list(np.flatnonzero(rej["relpose"])) == [8, 9]
        rp = r["rp"]
        pair = lambda e: tuple(sorted((int(rp["a"][e]), int(rp["b"][e]))))
        assert pair(8) == pair(7) and not rej["relpose"][7]             # a false closure next to a true one on its pair
        assert sum(pair(e) == pair(9) for e in range(len(rp["a"]))) == 1  # the other alone on its pair
        assert r["d"]["pose_fixed"][rp["a"][0]] and not rej["relpose"][0]  # an odometry edge with a fixed end stays
    if name == "closures_fixed_end":
        assert list(np.flatnonzero(rej["relpose"])) == [8] and r["d"]["pose_fixed"][r["rp"]["b"][8]]
    if name == "icp":
        kinds = [e[0] for e in r["icp"]]
        assert kinds == ["plane", "plane", "line"] and r["thr"]["icp"][1] == 0.0
        assert rej["icp"][0].any() and not rej["icp"][1].any() and rej["icp"][2].any()
        assert np.nanmax(r["terms"]["icp"][1]) > 2 * r["thr"]["icp"][0]  # the gross outliers of the set without a threshold stay
    if name == "gps":
        assert list(np.flatnonzero(rej["prior"])) == [2]
    if name == "mixed":
        st = np.asarray(r["d"]["e_stereo"]).astype(bool)
        assert rej["ba"][~st].any() and rej["ba"][st].any() and all(x.any() for x in rej["icp"])
        assert rej["prior"].any() and rej["relpose"].any()
    # the run on the reduced graph starts where the first ended and goes down from there
    assert r["tr2"][0]["chi2"] < r["tr"][-1]["chi2"]


# ---- the option ---------------------------------------------------------------------------------------------------
def with_threshold(kind, option):
    r = R.reference("mixed")
    g = R.build_graph(cugo, r, None, plan_only=True, option=option)
    {0: lambda: g.set_icp_outlier_threshold(cugo.ICP_PLANE, 5.0), 1: lambda: g.set_icp_outlier_threshold(cugo.ICP_LINE, 5.0),
     2: lambda: g.set_prior_outlier_threshold(5.0), 3: lambda: g.set_relpose_outlier_threshold(5.0)}[kind]()
    return g


@pytest.mark.parametrize("kind,name", [(0, "point-to-plane"), (1, "point-to-line"), (2, "pose prior"), (3, "relative-pose")])
def test_without_the_option_a_threshold_is_refused_with_the_message_of_old(kind, name):
    g = with_threshold(kind, option=False)
    with pytest.raises(cugo.CugoError) as e:
        g.initialize()
    assert ("cugo: outlier rejection is not available on %s edge sets yet (setOutlierThreshold must stay 0)" % name) in str(e.value)
    g.set_option("pose_edge_outliers", 1)  # the same graph is taken once the option is on ...
    g.initialize()
    g.set_option("pose_edge_outliers", 0)  # ... and refused again when it is off: the flattening is not reused across it
    with pytest.raises(cugo.CugoError, match="outlier rejection is not available"):
        g.initialize()
    g.close()


@pytest.mark.parametrize("name", PYTHON_CASES)
def test_plan_only_graph_of_each_case_initialises_with_thresholds(name):
    r = R.reference(name)
    g = R.build_graph(cugo, r, plan_only=True)
    g.initialize()
    plain = R.build_graph(cugo, r, None, plan_only=True, option=False)
    plain.initialize()
    # thresholds change neither the flattening nor the pattern
    assert g.n_active_edges() == plain.n_active_edges() and g.structure_stats() == plain.structure_stats()
    for kind in range(4):
        assert g.n_pose_edge_outliers(kind) == 0
    n_rp = 0 if r["rp"] is None else int(np.asarray(r["rp"]["active"]).sum())
    assert g.pose_edge_active(cugo.POSE_KIND_RELPOSE, n_rp).all()
    assert g.pose_edge_active(cugo.POSE_KIND_PRIOR, int(np.asarray(r["prior"]["active"]).sum())).all()
    with pytest.raises(cugo.CugoError, match="fewer edges"):
        g.pose_edge_active(cugo.POSE_KIND_RELPOSE, n_rp + 1)
    with pytest.raises(cugo.CugoError, match="no HIP device in use"):
        g.optimize(2)
    plain.close()
    g.close()


def test_unknown_option_names_and_kinds_are_refused():
    g = cugo.Graph(plan_only=True)
    for name in ("pose_edge_outlier", "POSE_EDGE_OUTLIERS", ""):
        with pytest.raises(cugo.CugoError, match="unknown option"):
            g.set_option(name, 1)
    assert cugo.lib().cugo_graph_set_option(g._g, None, 1) == -3
    for kind in (-1, 4):
        with pytest.raises(cugo.CugoError, match="kind must be one of"):
            g.n_pose_edge_outliers(kind)
        with pytest.raises(cugo.CugoError, match="kind must be one of"):
            g.pose_edge_active(kind, 0)
    g.close()


def test_flipping_the_option_forces_a_new_flattening():
    r = R.reference("closures")
    g = R.build_graph(cugo, r, None, plan_only=True, option=False)
    g.initialize()
    g.initialize()
    assert g.flatten_reuses() == 1
    g.set_option("pose_edge_outliers", 1)
    g.initialize()
    assert g.flatten_reuses() == 1  # flattened anew
    g.initialize()
    assert g.flatten_reuses() == 2
    g.set_option("pose_edge_outliers", 1)  # the same value again: nothing to redo
    g.initialize()
    assert g.flatten_reuses() == 3
    g.set_relpose_outlier_threshold(r["thr"]["relpose"])  # a threshold counts as a change of the set
    g.initialize()
    assert g.flatten_reuses() == 3
    g.close()


def test_sharded_optimiser_still_refuses_these_sets_with_the_option_on():
    r = R.reference("closures")
    g = R.build_graph(cugo, r, plan_only=True)
    g.set_shard(0, 2, lambda ptr, n, op: None)
    with pytest.raises(cugo.CugoError, match="relative-pose edge sets are not supported on a landmark-sharded"):
        g.initialize()
    g.close()


# ---- the new entry points ----------------------------------------------------------------------------------------------
def test_declarations_and_ctypes_calls_of_the_new_entry_points_agree():
    hdr = open(os.path.join(ROOT, "include", "cugo_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = {m.group(1): [" ".join(a.split()) for a in m.group(2).split(",")]
            for m in re.finditer(r"\bint\s+(cugo_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)}
    assert decl["cugo_pose_edges_reject"] == ["cugo_ctx* ctx", "int n", "const double* d_edge_chi", "const double* d_threshold",
                                              "int n_threshold", "uint8_t* d_flags", "int32_t* d_rejected", "int* n_rejected"]
    assert decl["cugo_graph_n_pose_edge_outliers"] == ["cugo_graph* g", "int kind"]
    assert decl["cugo_graph_get_pose_edge_active"] == ["cugo_graph* g", "int kind", "int n", "uint8_t* active"]
    for name, value in (("PLANE", 0), ("LINE", 1), ("PRIOR", 2), ("RELPOSE", 3)):
        assert re.search(r"#define CUGO_POSE_KIND_%s %d\b" % (name, value), hdr) and getattr(cugo, "POSE_KIND_" + name) == value
    assert (cugo.POSE_KIND_PLANE, cugo.POSE_KIND_LINE) == (cugo.ICP_PLANE, cugo.ICP_LINE)
    L = cugo.lib()
    for f in decl:
        assert hasattr(L, f), f
    # the calls as the wrappers make them, where no device is needed: refusals that touch nothing
    count = C.c_int(5)
    assert L.cugo_pose_edges_reject(None, 0, None, None, 1, None, None, C.byref(count)) == -3 and count.value == 5
    g = cugo.Graph(plan_only=True)
    out = np.full(4, 7, np.uint8)
    assert L.cugo_graph_get_pose_edge_active(g._g, 3, 1, out.ctypes.data_as(C.POINTER(C.c_uint8))) == -3 and (out == 7).all()
    assert L.cugo_graph_get_pose_edge_active(g._g, 3, 0, None) == 0 and L.cugo_graph_n_pose_edge_outliers(g._g, 2) == 0
    assert L.cugo_graph_n_pose_edge_outliers(g._g, 9) == -3 and L.cugo_graph_n_pose_edge_outliers(None, 0) == -3
    g.close()


# ---- the C++ interface ------------------------------------------------------------------------------------------------
GRAPH_PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <string>
#include "cuda_graph_optimisation.h"
#include "icp_types.h"
#include "prior_types.h"
#include "relpose_types.h"
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)
static std::string refusal(cugo::CudaGraphOptimisationImpl& opt)
{
    try { opt.initialize(); }
    catch (const std::exception& e) { return e.what(); }
    return "";
}
int main()
{
    cugo::PoseVertexSet poses(false);
    cugo::PoseVertex v0(0, cugo::Se3D(), true), v1(1, cugo::Se3D(), false), v2(2, cugo::Se3D(), false);
    poses.addVertex(&v0), poses.addVertex(&v1), poses.addVertex(&v2);
    cugo::PlaneEdgeSet planes, planes2;
    cugo::PlaneEdge pe[4];
    for (int i = 0; i < 4; i++)
    {
        cugo::PointToPlaneMatch<double> m;
        m.pointP[0] = 1 + i, m.pointP[1] = 2, m.pointP[2] = 3;
        m.normal[0] = 0, m.normal[1] = 0, m.normal[2] = 1;
        m.originDistance = 3;
        pe[i].setMeasurement(m);
        pe[i].setVertex(i % 2 ? &v1 : &v2, 0);
        (i < 2 ? planes : planes2).addEdge(&pe[i]);
    }
    cugo::LineEdgeSet lines;
    cugo::PosePriorEdgeSet priors;
    cugo::PosePriorEdge pr;
    pr.setVertex(&v2, 0);
    priors.addEdge(&pr);
    cugo::RelPoseEdgeSet rel;
    cugo::RelPoseEdge e01, e12;
    e01.setVertex(&v0, 0), e01.setVertex(&v1, 1);
    e12.setVertex(&v1, 0), e12.setVertex(&v2, 1);
    rel.addEdge(&e01), rel.addEdge(&e12);
    cugo::GraphOptimisationOptions off, on;
    off.planOnly = on.planOnly = true;
    off.relativePoseEdges = on.relativePoseEdges = true;
    CHECK(!off.poseEdgeOutlierRejection); // the new last member, off by default
    on.poseEdgeOutlierRejection = true;
    cugo::BaseEdgeSet* sets[] = {&planes, &planes2, &lines, &priors, &rel};
    const char* names[] = {"point-to-plane", "point-to-plane", "point-to-line", "pose prior", "relative-pose"};
    auto threshold = [&](int k, double t) { // (setOutlierThreshold is a member of the typed sets, as in the reference)
        k == 0 ? planes.setOutlierThreshold(t) : k == 1 ? planes2.setOutlierThreshold(t) : k == 2 ? lines.setOutlierThreshold(t)
        : k == 3 ? priors.setOutlierThreshold(t) : rel.setOutlierThreshold(t);
    };
    {   // the option off: every kind refuses a positive threshold with its message; 0, negative and NaN are no threshold
        cugo::CudaGraphOptimisationImpl opt(off);
        opt.addVertexSet(&poses);
        for (cugo::BaseEdgeSet* s : sets)
            opt.addEdgeSet(s);
        opt.initialize();
        for (int k = 0; k < 5; k++)
        {
            if (k == 2)
                continue; // (an empty set settles nothing but its threshold is looked at all the same: below)
            threshold(k, 2.5);
            const std::string w = refusal(opt);
            std::printf("refusal: %s\n", w.c_str());
            CHECK(w == std::string("cugo: outlier rejection is not available on ") + names[k] +
                           " edge sets yet (setOutlierThreshold must stay 0)");
            threshold(k, k % 2 ? -1.0 : std::numeric_limits<double>::quiet_NaN());
            opt.initialize();
            threshold(k, 0.0);
        }
        lines.setOutlierThreshold(1.0);
        CHECK(refusal(opt).find("point-to-line") != std::string::npos);
        lines.setOutlierThreshold(0.0);
    }
    {   // the option on: thresholds are taken, two sets of a kind with different ones (a 0 among them), NaN and inf as 0
        cugo::CudaGraphOptimisationImpl opt(on);
        opt.addVertexSet(&poses);
        for (cugo::BaseEdgeSet* s : sets)
            opt.addEdgeSet(s);
        planes.setOutlierThreshold(2.5), planes2.setOutlierThreshold(0.0);
        priors.setOutlierThreshold(std::numeric_limits<double>::quiet_NaN());
        rel.setOutlierThreshold(4.0);
        lines.setOutlierThreshold(9.0); // (an empty set with a threshold)
        opt.initialize();
        CHECK(opt.nIcpEdges(0) == 4 && opt.nPriorEdges() == 1 && opt.nRelPoseEdges() == 2 && opt.nActiveEdges() == 7);
        for (cugo::BaseEdgeSet* s : sets)
            CHECK(s->getOutlierCount() == 0);
        CHECK(planes.getInlierCount() == 2 && planes2.getInlierCount() == 2 && rel.getInlierCount() == 2);
        planes2.setOutlierThreshold(7.0); // both sets with one, different
        opt.initialize();
        planes.setOutlierThreshold(std::numeric_limits<double>::infinity()), planes2.setOutlierThreshold(-3.0);
        opt.initialize();
        CHECK(opt.nIcpEdges(0) == 4);
        // an edge switched off by hand is left out, as a rejected one will be
        e12.inactivate();
        opt.initialize();
        CHECK(opt.nRelPoseEdges() == 1 && rel.getInlierCount() == 1 && opt.structureStats()[0] == 2);
        e12.setActive();
        // the option through setOption, and unknown names
        CHECK(opt.setOption("pose_edge_outliers", 0) && !opt.setOption("pose_edge_outlier", 1));
        planes.setOutlierThreshold(0.0);
        CHECK(refusal(opt).find("point-to-line edge sets yet") != std::string::npos); // (the first set with one: the empty one)
        lines.setOutlierThreshold(0.0);
        CHECK(refusal(opt).find("relative-pose edge sets yet") != std::string::npos);
        CHECK(opt.setOption("pose_edge_outliers", 1));
        opt.initialize();
        bool threw = false;
        try { opt.optimize(1); }
        catch (const std::exception& e) { threw = std::string(e.what()).find("plan-only") != std::string::npos; }
        CHECK(threw);
    }
    std::printf("OK\n");
    return 0;
}
"""


def test_cpp_thresholds_are_taken_with_the_option_and_refused_without(tmp_path):
    src = tmp_path / "pose_outlier_graph.cpp"
    src.write_text(GRAPH_PROGRAM)
    exe = tmp_path / "pose_outlier_graph"
    lib_dir = os.path.dirname(cugo.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", INC, str(src), "-L", lib_dir, "-lcugo_hip",
                        "-Wl,-rpath," + lib_dir, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr


# ---- the host path under CPU sanitizers, in a program of its own ------------------------------------------------------
CASE_STRUCT = """
struct Case
{
    int P, L, E, n_plane, n_line, n_prior, n_rp;
    double thr[6]; // mono, stereo, plane, line, prior, relative-pose
    const double* pose; const uint8_t* pose_fixed; const double* lm; const uint8_t* lm_fixed;
    const int32_t *e_pose, *e_lm; const uint8_t* e_stereo; const double *e_meas, *e_omega, *e_cam;
    const int32_t* pl_pose; const double *pl_p, *pl_n, *pl_d, *pl_w;
    const int32_t* li_pose; const double *li_p, *li_a, *li_b, *li_w;
    const int32_t* prior_pose; const double *prior_z, *prior_info;
    const int32_t *rp_a, *rp_b; const double *rp_z, *rp_info;
};
"""

SAN_PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "cugo_hip.h"
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s (%s)\n", __FILE__, __LINE__, #c, cugo_last_error()); return 1; } } while (0)
#include "cases.inc"
static cugo_graph* build(const Case& c, bool option, double scale)
{
    cugo_graph* g = nullptr;
    if (cugo_graph_create_plan_only(1, 1, &g) != 0)
        return nullptr;
    std::vector<int32_t> pid(c.P), lid(c.L);
    for (int i = 0; i < c.P; i++) pid[i] = i;
    for (int i = 0; i < c.L; i++) lid[i] = i;
    cugo_graph_add_poses(g, c.P, pid.data(), c.pose, c.pose_fixed);
    cugo_graph_add_landmarks(g, c.L, lid.data(), c.lm, c.lm_fixed);
    for (int dim = 2; dim <= 3; dim++)
    {
        std::vector<int32_t> ep, el;
        std::vector<double> meas, om, cam;
        for (int e = 0; e < c.E; e++)
            if ((c.e_stereo[e] != 0) == (dim == 3))
            {
                ep.push_back(c.e_pose[e]), el.push_back(c.e_lm[e]), om.push_back(c.e_omega[e]);
                meas.insert(meas.end(), c.e_meas + 3 * e, c.e_meas + 3 * e + dim);
                cam.insert(cam.end(), c.e_cam + 5 * e, c.e_cam + 5 * e + 5);
            }
        cugo_graph_add_edges(g, dim, (int)ep.size(), ep.data(), el.data(), meas.data(), om.data(), cam.data());
        cugo_graph_set_outlier_threshold(g, dim, scale * c.thr[dim - 2]);
    }
    if (c.n_plane)
        cugo_graph_add_plane_edges(g, c.n_plane, c.pl_pose, c.pl_p, c.pl_n, c.pl_d, c.pl_w);
    if (c.n_line)
        cugo_graph_add_line_edges(g, c.n_line, c.li_pose, c.li_p, c.li_a, c.li_b, c.li_w);
    if (c.n_prior)
        cugo_graph_add_pose_priors(g, c.n_prior, c.prior_pose, c.prior_z, c.prior_info);
    if (c.n_rp)
        cugo_graph_add_relpose_edges(g, c.n_rp, c.rp_a, c.rp_b, c.rp_z, c.rp_info);
    cugo_graph_set_icp_outlier_threshold(g, CUGO_ICP_PLANE, scale * c.thr[2]);
    cugo_graph_set_icp_outlier_threshold(g, CUGO_ICP_LINE, scale * c.thr[3]);
    cugo_graph_set_prior_outlier_threshold(g, scale * c.thr[4]);
    cugo_graph_set_relpose_outlier_threshold(g, scale * c.thr[5]);
    if (option && cugo_graph_set_option(g, "pose_edge_outliers", 1) != 0)
        return nullptr;
    return g;
}
int main()
{
    for (const Case* c : {&closures, &gps, &mixed})
    {
        const int n_of[4] = {c->n_plane, c->n_line, c->n_prior, c->n_rp};
        // without the option: refused through the message, nothing half-built is left behind
        cugo_graph* g = build(*c, false, 1.0);
        CHECK(g && cugo_graph_initialize(g) != 0 && std::strstr(cugo_last_error(), "outlier rejection is not available"));
        // the option on the same graph: taken; estimates only: reused; thresholds scaled: flattened anew
        CHECK(cugo_graph_set_option(g, "pose_edge_outliers", 1) == 0 && cugo_graph_initialize(g) == 0);
        const int edges = cugo_graph_n_active_edges(g);
        CHECK(cugo_graph_initialize(g) == 0 && cugo_graph_flatten_reuses(g) == 1);
        for (int kind = 0; kind < 4; kind++)
        {
            std::vector<uint8_t> act((size_t)n_of[kind] + 1, 9);
            CHECK(cugo_graph_n_pose_edge_outliers(g, kind) == 0);
            CHECK(cugo_graph_get_pose_edge_active(g, kind, n_of[kind], act.data()) == 0 && act[(size_t)n_of[kind]] == 9);
            for (int i = 0; i < n_of[kind]; i++)
                CHECK(act[(size_t)i] == 1);
            CHECK(cugo_graph_get_pose_edge_active(g, kind, n_of[kind] + 1, act.data()) == CUGO_ERR_INVALID);
        }
        CHECK(cugo_graph_n_pose_edge_outliers(g, 4) == CUGO_ERR_INVALID && cugo_graph_n_pose_edge_outliers(g, -1) == CUGO_ERR_INVALID);
        CHECK(cugo_graph_optimize(g, 2) != 0); // plan-only: its own message, and the flags stay untouched
        CHECK(std::strstr(cugo_last_error(), "no HIP device in use"));
        CHECK(cugo_graph_set_option(g, "pose_edge_outliers", 0) == 0 && cugo_graph_initialize(g) != 0);
        CHECK(cugo_graph_set_option(g, "pose_edge_outlier", 1) == CUGO_ERR_INVALID);
        cugo_graph_destroy(g);
        // thresholds that mean "none" on every set, with the option on and off: the same flattening
        for (double scale : {0.0, -1.0, (double)NAN})
            for (int option = 0; option < 2; option++)
            {
                g = build(*c, option != 0, scale);
                CHECK(g && cugo_graph_initialize(g) == 0 && cugo_graph_n_active_edges(g) == edges);
                cugo_graph_destroy(g);
            }
        g = build(*c, true, (double)INFINITY); // (an infinite threshold on a set that has one: as 0)
        CHECK(g && cugo_graph_initialize(g) == 0 && cugo_graph_n_active_edges(g) == edges);
        cugo_graph_destroy(g);
    }
    // the kernel-level entry point refuses before it touches a device
    int count = 3;
    CHECK(cugo_pose_edges_reject(nullptr, 4, nullptr, nullptr, 1, nullptr, nullptr, &count) == CUGO_ERR_INVALID && count == 3);
    std::printf("OK\n");
    return 0;
}
"""


def case_source(name):
    r = R.reference(name)
    d, icp, prior, rp, thr = r["d"], r["icp"], r["prior"], r["rp"], r["thr"]
    by_kind = {k: (e, np.broadcast_to(np.asarray(om, np.float64), (len(act),)), np.asarray(act, bool)) for k, e, om, act, _ in icp}
    empty = (dict(pose=np.zeros(0, np.int32), p=np.zeros((0, 3)), n=np.zeros((0, 3)), d=np.zeros(0), a=np.zeros((0, 3)),
                  b=np.zeros((0, 3))), np.zeros(0), np.zeros(0, bool))
    pl, pl_w, pl_act = by_kind.get("plane", empty)
    li, li_w, li_act = by_kind.get("line", empty)
    act = np.asarray(prior["active"], bool)
    pinfo = np.broadcast_to(prior["info"], (len(act), 6, 6))[act]
    n_rp = 0 if rp is None else len(rp["a"])
    rinfo = np.broadcast_to(rp["info"], (n_rp, 6, 6)) if n_rp else np.zeros((0, 6, 6))
    z = lambda k, w: np.asarray(rp[k]) if n_rp else np.zeros((0, w))
    arrays = [("double", "pose", d["pose"]), ("uint8_t", "pose_fixed", d["pose_fixed"]), ("double", "lm", d["lm"]),
              ("uint8_t", "lm_fixed", d["lm_fixed"]), ("int32_t", "e_pose", d["e_pose"]), ("int32_t", "e_lm", d["e_lm"]),
              ("uint8_t", "e_stereo", d["e_stereo"]), ("double", "e_meas", d["e_meas"]), ("double", "e_omega", d["e_omega"]),
              ("double", "e_cam", d["e_cam"]),
              ("int32_t", "pl_pose", pl["pose"][pl_act]), ("double", "pl_p", pl["p"][pl_act]), ("double", "pl_n", pl["n"][pl_act]),
              ("double", "pl_d", pl["d"][pl_act]), ("double", "pl_w", pl_w[pl_act]),
              ("int32_t", "li_pose", li["pose"][li_act]), ("double", "li_p", li["p"][li_act]), ("double", "li_a", li["a"][li_act]),
              ("double", "li_b", li["b"][li_act]), ("double", "li_w", li_w[li_act]),
              ("int32_t", "prior_pose", np.asarray(prior["pose"])[act]), ("double", "prior_z", np.asarray(prior["z"])[act]),
              ("double", "prior_info", pinfo), ("int32_t", "rp_a", z("a", 1)), ("int32_t", "rp_b", z("b", 1)),
              ("double", "rp_z", z("z", 7)), ("double", "rp_info", rinfo)]
    s = "".join(c_array(t, "%s_%s" % (name, n), a) for t, n, a in arrays)
    ba, ic = thr.get("ba", (0.0, 0.0)), thr.get("icp", [0.0, 0.0])
    thr6 = [ba[0], ba[1], ic[0], ic[1], thr.get("prior", 0.0), thr.get("relpose", 0.0)]
    s += "static const Case %s = {%d, %d, %d, %d, %d, %d, %d, {%s}, %s};\n" % (
        name, len(d["pose"]), len(d["lm"]), len(d["e_pose"]), int(pl_act.sum()), int(li_act.sum()), int(act.sum()), n_rp,
        ", ".join(repr(float(t)) for t in thr6), ", ".join("%s_%s" % (name, n) for _, n, _ in arrays))
    return s


def test_thresholds_through_the_c_abi_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The host sources (flattening with the thresholds and the edge pointers, engine, layout, plans, symbolic analysis, C
    ABI) compiled by g++ with -fsanitize=address,undefined into a program of its own, built as
    tests/test_relpose_graph_host.py builds its program, that drives plan-only graphs of the closures, gps and mixed cases
    with their thresholds through the C ABI.  No sanitizer runtime is preloaded and nothing is loaded into python."""
    (tmp_path / "cases.inc").write_text(CASE_STRUCT + "".join(case_source(n) for n in ("closures", "gps", "mixed")))
    (tmp_path / "main.cpp").write_text(SAN_PROGRAM)
    flags = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", os.path.join(ROOT, "include"), "-I", str(tmp_path)]
    jobs = [(subprocess.Popen(flags + ["-c", os.path.join(HOST, f), "-o", str(tmp_path / (f + ".o"))],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True), f) for f in SAN_SOURCES]
    jobs.append((subprocess.Popen(flags + ["-c", str(tmp_path / "main.cpp"), "-o", str(tmp_path / "main.o")],
                                  stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True), "main.cpp"))
    for p, f in jobs:
        out, err = p.communicate(timeout=600)
        assert p.returncode == 0, f + ": " + err[-3000:]
    lib_dir = os.path.dirname(cugo.LIB_PATH)
    exe = tmp_path / "pose_outlier_san"
    objs = [str(tmp_path / (f + ".o")) for f in SAN_SOURCES] + [str(tmp_path / "main.o")]
    r = subprocess.run(["g++", "-fsanitize=address,undefined"] + objs + ["-L", lib_dir, "-lcugo_hip", "-Wl,-rpath," + lib_dir,
                        "-L", os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(ROCM, "lib"),
                        "-lpthread", "-ldl", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
