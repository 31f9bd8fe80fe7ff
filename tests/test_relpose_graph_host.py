"""Relative-pose SE(3) edge sets in the optimiser, without a GPU: plan-only graphs of the cases of tests/relpose_lm_ref.py
(flattening, the pose pairs in the Hsc pattern, the plan), every refusal of initialize() by its message, re-use of the
flattening, the C++ interface, and the host path under CPU sanitizers in a program of its own."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import prior_ref as PR
import relpose_lm_ref as L
import relpose_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "include")
HOST = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "csrc", "host")
cugo = importlib.import_module("cuda-bundle-adjustment_amd")


# ---- the cases, plan-only ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(L.CASES))
def test_plan_only_graph_of_each_case(name):
    d, icp, prior, rp = L.CASES[name][0]()
    g = L.build_graph(d, icp, prior, rp, plan_only=True)
    g.initialize()
    assert g.n_relpose_edges() == L.counting_edges(d, rp)
    s = g.structure_stats()
    assert s["hsc_blocks"] == L.union_pattern_blocks(d, rp)
    free = np.asarray(d["pose_fixed"]) == 0
    n_icp = sum(int((np.asarray(k[3], bool) & free[k[1]["pose"]]).sum()) for k in icp)  # (active, on a free pose)
    n_prior = int((np.asarray(d["pose_fixed"])[prior["pose"]] == 0).sum())
    assert g.n_active_edges() == len(d["e_pose"]) + n_icp + n_prior + g.n_relpose_edges()
    if len(d["lm"]) == 0:  # a pure pose graph is no block-diagonal system: the factor holds the pairs
        n_free = L.free_first(d)[1]
        assert s["hsc_blocks"] > n_free and s["nnzL"] >= s["hsc_blocks"] and s["products"] == 0
    g.close()


def test_pairs_without_a_common_landmark_add_exactly_their_blocks():
    d, icp, prior, rp = L.mixed_case()
    g = L.build_graph(d, icp, prior, None, plan_only=True)
    g.initialize()
    without = g.structure_stats()
    g.close()
    g = L.build_graph(d, icp, prior, rp, plan_only=True)
    g.initialize()
    with_ = g.structure_stats()
    g.close()
    far = L.relpose_pairs(d, rp) - L.covisible_pairs(d)
    assert len(far) >= 1 and with_["hsc_blocks"] == without["hsc_blocks"] + len(far)
    # products and contribution lists come from the real slots alone
    assert with_["products"] == without["products"] and with_["offdiag_products"] == without["offdiag_products"]


def test_the_landmark_major_plan_and_the_host_structure_agree_on_the_pattern(monkeypatch):
    d, icp, prior, rp = L.mixed_case()
    monkeypatch.setenv("CUGO_SCHUR_PLAN", "1")
    g = L.build_graph(d, icp, prior, rp, plan_only=True)
    g.initialize()
    s = g.structure_stats()
    g.close()
    assert s["hsc_blocks"] == L.union_pattern_blocks(d, rp) and s["schur_slots"] > 0


# ---- refusals ------------------------------------------------------------------------------------------------------
def chain_graph(per_edge_information=True):
    d, icp, prior, rp = L.chain_case()
    g = PR.build_graph(d, icp, prior, plan_only=True, per_edge_information=per_edge_information)
    return d, rp, g


def args(rp, sel=slice(None)):
    info = np.broadcast_to(rp["info"], (len(rp["a"]), 6, 6)).copy()
    return rp["a"][sel].copy(), rp["b"][sel].copy(), rp["z"][sel].copy(), info[sel]


def refused(g, what):
    with pytest.raises(cugo.CugoError, match=what):
        g.initialize()
    g.close()


def test_an_edge_from_a_pose_to_itself_is_refused():
    d, rp, g = chain_graph()
    a, b, z, info = args(rp)
    b[3] = a[3]
    g.add_relpose_edges(a, b, z, info)
    refused(g, r"relative-pose edge 3 of edge set \d+: it joins a pose to itself \(a == b\)")


def test_unknown_pose_id_is_refused_and_adds_nothing():
    d, rp, g = chain_graph()
    a, b, z, info = args(rp)
    b[2] = 77
    with pytest.raises(cugo.CugoError, match="unknown pose id 77"):
        g.add_relpose_edges(a, b, z, info)
    g.initialize()
    assert g.n_relpose_edges() == 0
    g.close()


@pytest.mark.parametrize("where", ["quaternion", "translation", "information"])
def test_non_finite_values_are_refused(where):
    d, rp, g = chain_graph()
    a, b, z, info = args(rp)
    if where == "quaternion":
        z[1, 2] = np.nan
    elif where == "translation":
        z[0, 5] = np.inf
    else:
        info[1, 2, 3] = info[1, 3, 2] = np.nan
    g.add_relpose_edges(a, b, z, info)
    refused(g, "relative-pose edge . of edge set .*non-finite")


def test_non_unit_measured_quaternion_is_refused_not_normalised():
    d, rp, g = chain_graph()
    a, b, z, info = args(rp)
    z[1, :4] *= 1.0 + 1e-5
    g.add_relpose_edges(a, b, z, info)
    refused(g, "relative-pose edge 1 .*unit length")
    d, rp, g = chain_graph()
    z = rp["z"].copy()
    z[:, :4] *= 1.0 + 5e-7
    g.add_relpose_edges(a, b, z, info)
    g.initialize()
    assert g.n_relpose_edges() == len(a)
    g.close()


def test_asymmetric_or_indefinite_information_is_refused_and_semi_definite_is_taken():
    d, rp, g = chain_graph()
    a, b, z, info = args(rp)
    bad = info.copy()
    bad[0, 1, 4] += 1e-9 * np.abs(bad[0]).max()
    g.add_relpose_edges(a, b, z, bad)
    refused(g, "relative-pose edge 0 .*not symmetric")
    d, rp, g = chain_graph()
    ok = info.copy()
    ok[1, 1, 4] += 1e-13 * np.abs(ok[1]).max()  # (inside 1e-12 max|Omega|)
    g.add_relpose_edges(a, b, z, ok)
    g.initialize()
    g.close()
    rng = np.random.default_rng(2)
    Q = np.linalg.qr(rng.normal(size=(6, 6)))[0]
    d, rp, g = chain_graph()
    ind = Q @ np.diag([5.0, 3.0, 2.0, 1.0, 0.5, -1e-9]) @ Q.T
    g.add_relpose_edges(a[:1], b[:1], z[:1], 0.5 * (ind + ind.T))
    refused(g, "positive semi-definite")
    # a translation-only edge, and a rank-one matrix that is singular in a rotated frame
    d, rp, g = chain_graph()
    semi = Q @ np.diag([5.0, 0, 0, 0, 0, 0]) @ Q.T
    g.add_relpose_edges(a[:2], b[:2], z[:2], np.array([np.diag([0, 0, 0, 1.0, 1.0, 1.0]), 0.5 * (semi + semi.T)]))
    g.initialize()
    assert g.n_relpose_edges() == 2
    g.close()
    # without per-edge information the set's matrix is the one that counts, and it is checked once, with the set
    d, rp, g = chain_graph(per_edge_information=False)
    g.add_relpose_edges(a, b, z, info)
    g.set_relpose_information(-np.eye(6))
    refused(g, r"relative-pose edge set \d+: .*positive semi-definite")


def test_outlier_threshold_on_a_relpose_set_is_refused():
    d, rp, g = chain_graph()
    g.add_relpose_edges(*args(rp))
    g.set_relpose_outlier_threshold(5.0)
    refused(g, "outlier rejection is not available on relative-pose edge sets")
    d, rp, g = chain_graph()
    g.add_relpose_edges(*args(rp))
    g.set_relpose_outlier_threshold(0.0)
    g.initialize()
    g.close()


def test_sharded_optimiser_refuses_relpose_sets():
    d, rp, g = chain_graph()
    g.add_relpose_edges(*args(rp))
    g.set_shard(0, 2, lambda ptr, n, op: None)
    refused(g, "relative-pose edge sets are not supported on a landmark-sharded")
    # the same shard with edges that count for nothing is taken
    d, rp, g = chain_graph()
    g.add_relpose_edges(*args(rp))
    g.set_relpose_active(np.zeros(len(rp["a"]), bool))
    g.set_shard(0, 2, lambda ptr, n, op: None)
    g.initialize()
    assert g.n_relpose_edges() == 0
    g.close()


def test_row_strip_form_of_the_schur_complement_is_refused_with_relpose_sets(monkeypatch):
    monkeypatch.setenv("CUGO_HSC_STRIP", "1")
    d, rp, g = chain_graph()
    g.add_relpose_edges(*args(rp))
    refused(g, "cannot be combined with CUGO_HSC_STRIP=1")
    d, rp, g = chain_graph()  # (no edge that counts: nothing to refuse)
    g.initialize()
    g.close()


# ---- what is dropped, what is kept -----------------------------------------------------------------------------------
def test_inactive_and_fixed_fixed_edges_are_dropped_and_a_fixed_end_stays():
    d, icp, prior, rp = L.mixed_case()
    d = dict(d, pose_fixed=np.asarray(d["pose_fixed"]).copy())
    d["pose_fixed"][4] = 1
    more = RR.make_edges([0, 4, 0], [4, 0, 1], rp["z"][:3], rp["info"][:3])
    both = RR.make_edges(np.concatenate([rp["a"], more["a"]]), np.concatenate([rp["b"], more["b"]]),
                         np.concatenate([rp["z"], more["z"]]), np.concatenate([rp["info"], more["info"]]))
    g = L.build_graph(d, icp, prior, both, plan_only=True)
    g.initialize()
    n = L.counting_edges(d, both)
    assert g.n_relpose_edges() == n == len(both["a"]) - 2  # (0-4 and 4-0 join two fixed poses; 0-1 has its free end)
    assert g.structure_stats()["hsc_blocks"] == L.union_pattern_blocks(d, both)
    off = np.ones(len(both["a"]), bool)
    off[[1, 3]] = False
    g.set_relpose_active(off)
    g.initialize()
    assert g.n_relpose_edges() == L.counting_edges(d, dict(both, active=off))
    assert g.structure_stats()["hsc_blocks"] == L.union_pattern_blocks(d, dict(both, active=off))
    g.close()


def test_reinitialize_after_changes_of_every_kind():
    """estimates only: the flattening is kept; a measurement, an edge on an existing pair: a new flattening, the same
    pattern; an edge on a new pair: one block more; the pair's only edge switched off: one block fewer"""
    d, icp, prior, rp = L.chain_case()
    g = L.build_graph(d, icp, prior, rp, plan_only=True)
    g.initialize()
    blocks, n = g.structure_stats()["hsc_blocks"], g.n_relpose_edges()
    assert g.flatten_reuses() == 0
    g.set_poses(np.arange(len(d["pose"]), dtype=np.int32), d["pose_gt"])
    g.initialize()
    assert g.flatten_reuses() == 1 and g.structure_stats()["hsc_blocks"] == blocks and g.n_relpose_edges() == n
    g.set_relpose_information(2.0 * np.eye(6))  # (a measurement-side change: counted by the set)
    g.initialize()
    assert g.flatten_reuses() == 1 and g.structure_stats()["hsc_blocks"] == blocks
    a, b, z, info = args(rp, slice(2, 3))
    g.add_relpose_edges(b, a, z, info)  # the pair of edge 2 once more, the other way round
    g.initialize()
    assert g.flatten_reuses() == 1 and g.structure_stats()["hsc_blocks"] == blocks and g.n_relpose_edges() == n + 1
    assert (1, 3) not in L.relpose_pairs(d, rp)
    g.add_relpose_edges([4], [2], z, info)  # free-first (1, 3): a new pair
    g.initialize()
    assert g.structure_stats()["hsc_blocks"] == blocks + 1 and g.n_relpose_edges() == n + 2
    g.initialize()
    assert g.flatten_reuses() == 2
    g.set_relpose_active([0], first=len(rp["a"]) + 1)
    g.initialize()
    assert g.structure_stats()["hsc_blocks"] == blocks and g.n_relpose_edges() == n + 1
    g.close()


# ---- the C++ interface ----------------------------------------------------------------------------------------------
GRAPH_PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>
#include "cuda_graph_optimisation.h"
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
    cugo::PoseVertexSet poses(false), strangers(false);
    cugo::PoseVertex v0(0, cugo::Se3D(), true), v1(1, cugo::Se3D(), false), v2(2, cugo::Se3D(), false),
        v3(3, cugo::Se3D(), false), alien(9, cugo::Se3D(), false);
    poses.addVertex(&v0), poses.addVertex(&v1), poses.addVertex(&v2), poses.addVertex(&v3);
    strangers.addVertex(&alien);
    cugo::RelPoseEdgeSet rel, rel2;
    cugo::RelPoseEdge e01, e12, e21, e31;
    e01.setVertex(&v0, 0), e01.setVertex(&v1, 1);
    e12.setVertex(&v1, 0), e12.setVertex(&v2, 1);
    e21.setVertex(&v2, 0), e21.setVertex(&v1, 1);
    e31.setVertex(&v3, 0), e31.setVertex(&v1, 1);
    rel.addEdge(&e01), rel.addEdge(&e12), rel.addEdge(&e21);
    rel2.addEdge(&e31);
    cugo::PosePriorEdgeSet priors;
    cugo::PosePriorEdge p;
    p.setVertex(&v2, 0);
    priors.addEdge(&p);
    cugo::GraphOptimisationOptions off, on;
    off.planOnly = on.planOnly = true;
    on.relativePoseEdges = true;
    {   // the option off: the refusal of old, which now names the option as well
        cugo::CudaGraphOptimisationImpl opt(off);
        opt.addVertexSet(&poses);
        opt.addEdgeSet(&rel);
        const std::string w = refusal(opt);
        std::printf("refusal: %s\n", w.c_str());
        CHECK(w.find("relative-pose") != std::string::npos && w.find("cugo_relpose_") != std::string::npos &&
              w.find("relativePoseEdges") != std::string::npos);
    }
    for (int order = 0; order < 2; order++)
    {   // the option on: the set is taken, next to a prior set, whichever comes first
        cugo::CudaGraphOptimisationImpl opt(on);
        opt.addVertexSet(&poses);
        opt.addEdgeSet(order ? (cugo::BaseEdgeSet*)&priors : (cugo::BaseEdgeSet*)&rel);
        opt.addEdgeSet(order ? (cugo::BaseEdgeSet*)&rel : (cugo::BaseEdgeSet*)&priors);
        opt.initialize();
        CHECK(opt.nRelPoseEdges() == 3 && opt.nPriorEdges() == 1 && opt.nActiveEdges() == 4);
        CHECK(opt.structureStats()[0] == 3 + 1); // poses 1 2 3, the pair (1, 2)
        // a second set on a new pair
        opt.addEdgeSet(&rel2);
        opt.initialize();
        CHECK(opt.nRelPoseEdges() == 4 && opt.structureStats()[0] == 3 + 2);
        // ... that disagrees on the robust kernel
        rel2.setRobustKernel(cugo::RobustKernelType::Huber, 2.0);
        const std::string w = refusal(opt);
        std::printf("refusal: %s\n", w.c_str());
        CHECK(w.find("relative-pose edge sets of one optimiser must use the same robust kernel") != std::string::npos);
        rel2.setRobustKernel(cugo::RobustKernelType::None, 1.0);
        opt.initialize();
        // an inactive edge is dropped; the pair keeps its block through the other edge
        e12.inactivate();
        opt.initialize();
        CHECK(opt.nRelPoseEdges() == 3 && opt.structureStats()[0] == 3 + 2);
        e21.inactivate();
        opt.initialize();
        CHECK(opt.nRelPoseEdges() == 2 && opt.structureStats()[0] == 3 + 1);
        e12.setActive(), e21.setActive();
    }
    {   // a vertex of no pose set of the optimiser
        cugo::RelPoseEdgeSet bad;
        cugo::RelPoseEdge e;
        e.setVertex(&v1, 0), e.setVertex(&alien, 1);
        bad.addEdge(&e);
        cugo::CudaGraphOptimisationImpl opt(on);
        opt.addVertexSet(&poses);
        opt.addEdgeSet(&bad);
        const std::string w = refusal(opt);
        std::printf("refusal: %s\n", w.c_str());
        CHECK(w.find("relative-pose edge 0") != std::string::npos && w.find("in no pose vertex set of this optimiser") != std::string::npos);
    }
    {   // a == b, by the same vertex object
        cugo::RelPoseEdgeSet bad;
        cugo::RelPoseEdge e;
        e.setVertex(&v2, 0), e.setVertex(&v2, 1);
        bad.addEdge(&e);
        cugo::CudaGraphOptimisationImpl opt(on);
        opt.addVertexSet(&poses);
        opt.addEdgeSet(&bad);
        CHECK(refusal(opt).find("a == b") != std::string::npos);
    }
    std::printf("OK\n");
    return 0;
}
"""


def test_cpp_relpose_set_is_taken_with_the_option_and_refused_without(tmp_path):
    src = tmp_path / "relpose_graph.cpp"
    src.write_text(GRAPH_PROGRAM)
    exe = tmp_path / "relpose_graph"
    lib_dir = os.path.dirname(cugo.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", INC, str(src), "-L", lib_dir, "-lcugo_hip",
                        "-Wl,-rpath," + lib_dir, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr


# ---- the host path under CPU sanitizers, in a program of its own ------------------------------------------------------
SAN_PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "cugo_hip.h"
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s (%s)\n", __FILE__, __LINE__, #c, cugo_last_error()); return 1; } } while (0)
#include "cases.inc"
static cugo_graph* build(const Case& c, int upto_relpose)
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
    }
    if (c.n_prior)
        cugo_graph_add_pose_priors(g, c.n_prior, c.prior_pose, c.prior_z, c.prior_info);
    if (upto_relpose)
        cugo_graph_add_relpose_edges(g, upto_relpose, c.rp_a, c.rp_b, c.rp_z, c.rp_info);
    return g;
}
static double blocks(cugo_graph* g)
{
    double s[24] = {0};
    cugo_graph_structure_stats(g, s, 24);
    return s[0];
}
static bool refused(cugo_graph* g, const char* what)
{
    const bool r = cugo_graph_initialize(g) != 0 && std::strstr(cugo_last_error(), what) != nullptr;
    if (!r)
        std::printf("expected a refusal with '%s', got '%s'\n", what, cugo_last_error());
    cugo_graph_destroy(g);
    return r;
}
int main()
{
    for (const Case* c : {&chain, &mixed})
    {
        cugo_graph* g = build(*c, c->n_rp);
        CHECK(g && cugo_graph_initialize(g) == 0);
        CHECK(cugo_graph_n_relpose_edges(g) == c->n_counting && blocks(g) == c->hsc_blocks);
        // estimates only; then every edge off and on again: the pairs leave the pattern and come back
        CHECK(cugo_graph_initialize(g) == 0 && cugo_graph_flatten_reuses(g) == 1);
        std::vector<uint8_t> flags((size_t)c->n_rp, 0);
        CHECK(cugo_graph_set_relpose_active(g, 0, c->n_rp, flags.data()) == 0 && cugo_graph_initialize(g) == 0);
        CHECK(cugo_graph_n_relpose_edges(g) == 0 && blocks(g) == c->hsc_blocks_without);
        flags.assign(flags.size(), 1);
        CHECK(cugo_graph_set_relpose_active(g, 0, c->n_rp, flags.data()) == 0 && cugo_graph_initialize(g) == 0);
        CHECK(cugo_graph_n_relpose_edges(g) == c->n_counting && blocks(g) == c->hsc_blocks);
        CHECK(cugo_graph_set_relpose_active(g, 1, c->n_rp, flags.data()) != 0); // past the end: refused, nothing read
        cugo_graph_destroy(g);
        // growing edge by edge: every prefix of the set gives a pattern and a plan
        for (int n = 1; n < c->n_rp; n++)
        {
            g = build(*c, n);
            CHECK(g && cugo_graph_initialize(g) == 0 && blocks(g) <= c->hsc_blocks);
            cugo_graph_destroy(g);
        }
    }
    // the checks, each leaving through its message with nothing read out of range on the way
    {
        Case c = chain;
        std::vector<int32_t> b(c.rp_b, c.rp_b + c.n_rp);
        b[3] = c.rp_a[3];
        c.rp_b = b.data();
        CHECK(refused(build(c, c.n_rp), "a == b"));
    }
    {
        Case c = chain;
        std::vector<double> z(c.rp_z, c.rp_z + 7 * c.n_rp), w(c.rp_info, c.rp_info + 36 * c.n_rp);
        z[7 * 2 + 1] *= 1.001;
        c.rp_z = z.data();
        CHECK(refused(build(c, c.n_rp), "unit length"));
        z[7 * 2 + 1] = HUGE_VAL;
        CHECK(refused(build(c, c.n_rp), "non-finite"));
        c.rp_z = chain.rp_z;
        w[36 * 4 + 6 * 1 + 4] += 1e-6 * w[36 * 4];
        c.rp_info = w.data();
        CHECK(refused(build(c, c.n_rp), "not symmetric"));
        for (int i = 0; i < 36; i++)
            w[36 * 4 + i] = i % 7 == 0 ? -1.0 : 0.0;
        CHECK(refused(build(c, c.n_rp), "positive semi-definite"));
        for (int i = 0; i < 36; i++)
            w[36 * 4 + i] = i == 21 ? 3.0 : 0.0; // rank one: accepted
        cugo_graph* g = build(c, c.n_rp);
        CHECK(g && cugo_graph_initialize(g) == 0 && cugo_graph_n_relpose_edges(g) == c.n_counting);
        CHECK(cugo_graph_set_relpose_outlier_threshold(g, 3.0) == 0);
        CHECK(refused(g, "outlier rejection is not available on relative-pose"));
    }
    std::printf("OK\n");
    return 0;
}
"""

SAN_SOURCES = ["graph_optimisation.cpp", "engine.cpp", "edge_layout.cpp", "relpose_plan.cpp", "schur_plan.cpp",
               "chol_symbolic.cpp", "chol_solver.cpp", "thread_pool.cpp", "c_api.cpp", "synthetic.cpp", "device_cache.cpp",
               "rccl_comm.cpp"]
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def c_array(ctype, name, a):
    a = np.asarray(a).reshape(-1)
    body = ", ".join(repr(float(x)) if ctype == "double" else str(int(x)) for x in a) if len(a) else "0"
    return "static const %s %s[] = {%s};\n" % (ctype, name, body)


def case_source(name):
    d, icp, prior, rp = L.CASES[name][0]()
    act = np.asarray(prior["active"], bool)
    pinfo = np.broadcast_to(prior["info"], (len(act), 6, 6))[act]
    info = np.broadcast_to(rp["info"], (len(rp["a"]), 6, 6))
    arrays = [("double", "pose", d["pose"]), ("uint8_t", "pose_fixed", d["pose_fixed"]), ("double", "lm", d["lm"]),
              ("uint8_t", "lm_fixed", d["lm_fixed"]), ("int32_t", "e_pose", d["e_pose"]), ("int32_t", "e_lm", d["e_lm"]),
              ("uint8_t", "e_stereo", d["e_stereo"]), ("double", "e_meas", d["e_meas"]), ("double", "e_omega", d["e_omega"]),
              ("double", "e_cam", d["e_cam"]), ("int32_t", "prior_pose", np.asarray(prior["pose"])[act]),
              ("double", "prior_z", np.asarray(prior["z"])[act]), ("double", "prior_info", pinfo),
              ("int32_t", "rp_a", rp["a"]), ("int32_t", "rp_b", rp["b"]), ("double", "rp_z", rp["z"]), ("double", "rp_info", info)]
    s = "".join(c_array(t, "%s_%s" % (name, n), a) for t, n, a in arrays)
    none = RR.make_edges(rp["a"][:0], rp["b"][:0], rp["z"][:0], rp["info"][:1])
    s += "static const Case %s = {%d, %d, %d, %d, %d, %d, %d, %d, %s};\n" % (
        name, len(d["pose"]), len(d["lm"]), len(d["e_pose"]), int(act.sum()), len(rp["a"]), L.counting_edges(d, rp),
        L.union_pattern_blocks(d, rp), L.union_pattern_blocks(d, none),
        ", ".join("%s_%s" % (name, n) for _, n, _ in arrays))
    return s


CASE_STRUCT = """
struct Case
{
    int P, L, E, n_prior, n_rp, n_counting, hsc_blocks, hsc_blocks_without;
    const double* pose; const uint8_t* pose_fixed; const double* lm; const uint8_t* lm_fixed;
    const int32_t *e_pose, *e_lm; const uint8_t* e_stereo; const double *e_meas, *e_omega, *e_cam;
    const int32_t* prior_pose; const double *prior_z, *prior_info;
    const int32_t *rp_a, *rp_b; const double *rp_z, *rp_info;
};
"""


def test_flattening_pattern_and_plan_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The host sources that take part (flattening and checks, engine, layout and augmented pattern lists, plans,
    symbolic analysis, solver front end, C ABI) compiled by g++ with -fsanitize=address,undefined into a program of its own that drives
    plan-only graphs of the chain and mixed cases through the C ABI; what stays (kernel launchers, which a plan-only
    graph never calls) comes from the product library.  No sanitizer runtime is preloaded and nothing is loaded into
    python.  (The ICP sets of mixed are left out: the pattern does not depend on them.)"""
    (tmp_path / "cases.inc").write_text(CASE_STRUCT + case_source("chain") + case_source("mixed"))
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
    exe = tmp_path / "relpose_san"
    objs = [str(tmp_path / (f + ".o")) for f in SAN_SOURCES] + [str(tmp_path / "main.o")]
    r = subprocess.run(["g++", "-fsanitize=address,undefined"] + objs + ["-L", lib_dir, "-lcugo_hip", "-Wl,-rpath," + lib_dir,
                        "-L", os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(ROCM, "lib"),
                        "-lpthread", "-ldl", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
