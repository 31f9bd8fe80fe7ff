"""Outlier rejection on plane, line, prior and relative-pose edge sets in the optimiser, on the GPU, against the numpy
reference of tests/pose_outlier_ref.py: which edges go at the end of optimize(), that the flags take effect on the
device (a second optimize() on the same initialisation), that the next initialize() flattens without them (bit for bit
a graph that never held them), thresholds that reject nothing, the launch budget, covariances, poisoned allocations.

Bounds: icp_lm_ref.tolerances over the reference's own runs (pose_outlier_ref.reference); the rejected sets are compared
exactly (the cases keep a factor 2 between every term and its threshold).

The case `icp` holds two plane sets with different thresholds, which the C graph object cannot express (it has one plane
set): it runs through the C++ interface in a small program that prints what the other cases read through Python."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import pose_outlier_ref as R
import relpose_lm_ref as L
from conftest import ROOT
from test_gpu import assert_trajectories_match

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
pytestmark = pytest.mark.gpu
INC = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "include")
PYTHON_CASES = [n for n in R.CASES if n != "icp"]
REJECT_KERNELS = ("k_pose_reject_count", "k_pose_reject_scan", "k_pose_reject_place")
ERROR_KERNELS = ("k_icp_chunks_errors", "k_prior_errors", "k_relpose_errors")  # one per kind group with d_edge_chi


def need_gpu():
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")


def key(stats):
    return [(s["chi2"], s["lam"], s["trials"]) for s in stats]


def counts(r):
    """edges the C graph object holds per pose kind (the active ones of the recipe)"""
    by = {k: int(np.asarray(act, bool).sum()) for k, _, _, act, _ in r["icp"]}
    return [by.get("plane", 0), by.get("line", 0), int(np.asarray(r["prior"]["active"]).sum()),
            0 if r["rp"] is None else int(np.asarray(r["rp"]["active"]).sum())]


def expected_rejected(r):
    """per pose kind, and for mono / stereo: positions in the C graph object's insertion order of the edges that go"""
    icp = {k: R.product_index(act, rej) for (k, _, _, act, _), rej in zip(r["icp"], r["rej"]["icp"])}
    none = np.zeros(0, int)
    st = np.asarray(r["d"]["e_stereo"]).astype(bool)
    pose = [icp.get("plane", none), icp.get("line", none), R.product_index(r["prior"]["active"], r["rej"]["prior"]),
            none if r["rp"] is None else R.product_index(r["rp"]["active"], r["rej"]["relpose"])]
    return pose, {2: np.flatnonzero(r["rej"]["ba"][~st]), 3: np.flatnonzero(r["rej"]["ba"][st])}


def rejected_of(g, r):
    n = counts(r)
    return [np.flatnonzero(~g.pose_edge_active(kind, n[kind])) for kind in range(4)]


def show(tag, stats, tr):
    for a, b in zip(stats, tr):
        print(tag, "chi2 %.15g ref %.15g rel %.3g trials %d ref %d" %
              (a["chi2"], b["chi2"], abs(a["chi2"] - b["chi2"]) / b["chi2"], a["trials"], b["trials"]))


def full_run(name, scale=1.0, thresholds="all", timing=False):
    """initialize, optimize(n), optimize(n2) on the same initialisation, initialize, optimize(n2) -> everything read.
    thresholds: "all" the case's, "ba" those of the mono and stereo sets alone, None"""
    need_gpu()
    r = R.reference(name)
    thr = {"all": r["thr"], "ba": {k: v for k, v in r["thr"].items() if k == "ba"}, None: None}[thresholds]
    g = R.build_graph(cugo, r, thr, scale=scale)
    if timing:
        g.set_kernel_timing(1)
    out = dict(r=r)
    g.initialize()
    g.optimize(r["niter"])
    out["stats1"], out["pose1"], out["lm1"] = g.stats(), g.poses(), g.landmarks()
    out["rejected"] = rejected_of(g, r)
    out["n_outliers"] = [g.n_pose_edge_outliers(k) for k in range(4)]
    st = np.asarray(r["d"]["e_stereo"]).astype(bool)
    out["ba_rejected"] = {2: np.flatnonzero(~g.edge_active(2, int((~st).sum()))), 3: np.flatnonzero(~g.edge_active(3, int(st.sum())))}
    out["ba_outliers"] = {2: g.n_outliers(2), 3: g.n_outliers(3)}
    out["n_relpose_after"], out["blocks1"] = g.n_relpose_edges(), g.structure_stats()["hsc_blocks"]
    if timing:
        out["kernels1"] = g.kernel_times()
    g.optimize(r["niter2"])
    out["stats2"], out["pose2"], out["lm2"] = g.stats()[len(out["stats1"]):], g.poses(), g.landmarks()
    out["rejected_twice"] = rejected_of(g, r)
    out["blocks2"] = g.structure_stats()["hsc_blocks"]
    g.initialize()
    g.optimize(r["niter2"])
    out["stats3"], out["pose3"], out["lm3"] = g.stats(), g.poses(), g.landmarks()
    out["blocks3"], out["n_relpose3"] = g.structure_stats()["hsc_blocks"], g.n_relpose_edges()
    out["graph"] = g
    return out


@pytest.mark.parametrize("pose_schur", ["1", "0"])
@pytest.mark.parametrize("name", PYTHON_CASES)
def test_rejected_sets_and_both_runs_against_the_reference(name, pose_schur, monkeypatch):
    """in the default loop and with CUGO_POSE_SCHUR=0: the first optimize() follows the reference (rejection happens
    behind the loop), the rejected sets are the reference's per kind, the second optimize() on the same initialisation
    follows the reference on the reduced graph (the flags took effect on the device), and initialize() + optimize() after
    that is bit for bit a fresh graph that never held the rejected edges"""
    monkeypatch.setenv("CUGO_POSE_SCHUR", pose_schur)
    out = full_run(name)
    r, g = out["r"], out["graph"]
    g.close()
    show("%s first" % name, out["stats1"], r["tr"])
    show("%s second" % name, out["stats2"], r["tr2"])
    want_pose, want_ba = expected_rejected(r)
    print("rejected", [list(x) for x in out["rejected"]], "BA", {k: list(v) for k, v in out["ba_rejected"].items()})
    for kind in range(4):
        assert np.array_equal(out["rejected"][kind], want_pose[kind]), R.KINDS[kind]
        assert out["n_outliers"][kind] == len(want_pose[kind])
        assert np.array_equal(out["rejected_twice"][kind], want_pose[kind])  # the second run ends without new outliers
    for dim in (2, 3):
        assert np.array_equal(out["ba_rejected"][dim], want_ba[dim]) and out["ba_outliers"][dim] == len(want_ba[dim])
    assert_trajectories_match(out["stats1"], r["tr"], r["tol"])
    np.testing.assert_allclose(out["pose1"], r["pose"], rtol=0, atol=r["etol"])
    assert_trajectories_match(out["stats2"], r["tr2"], r["tol2"])
    np.testing.assert_allclose(out["pose2"], r["pose2"], rtol=0, atol=r["etol2"])
    if len(r["lm"]):
        np.testing.assert_allclose(out["lm1"], r["lm"], rtol=0, atol=10 * r["etol"])
        np.testing.assert_allclose(out["lm2"], r["lm2"], rtol=0, atol=10 * r["etol2"])
    # n_*_edges() and the pattern keep describing the flattening until the next initialize()
    if r["rp"] is not None:
        assert out["n_relpose_after"] == L.counting_edges(r["d"], r["rp"])
        assert out["n_relpose3"] == L.counting_edges(r["d2"], r["rp2"])
    blocks = L.union_pattern_blocks(r["d"], R.no_relpose() if r["rp"] is None else r["rp"])
    assert out["blocks1"] == blocks
    if not len(want_ba[2]) and not len(want_ba[3]):
        assert out["blocks2"] == blocks  # (pose edges alone do not dirty the pattern: the emptied pair keeps its block)
    # a fresh graph without the rejected edges, from the estimates the second run ended at, without thresholds
    fresh = L.build_graph(dict(r["d2"], pose=out["pose2"], lm=out["lm2"]), r["icp2"], r["prior2"], r["rp2"], rk=r["rk"])
    fresh.initialize()
    fresh.optimize(r["niter2"])
    assert key(fresh.stats()) == key(out["stats3"])
    assert np.array_equal(fresh.poses(), out["pose3"]) and np.array_equal(fresh.landmarks(), out["lm3"])
    assert fresh.structure_stats()["hsc_blocks"] == out["blocks3"]
    fresh.close()
    if name == "closures":
        # the pair (2, 7) lost its only edge: one block fewer after the next flattening; (1, 5) kept a true edge
        assert out["blocks3"] == blocks - 1
        assert len(L.relpose_pairs(r["d"], r["rp"])) - len(L.relpose_pairs(r["d2"], r["rp2"])) == 1
    if name == "closures_fixed_end":
        # the edge with the fixed end is no block of the pattern: its free end's diagonal term went with it (second run)
        assert out["blocks3"] == blocks


def test_thresholds_that_reject_nothing_change_no_bit():
    """thresholds at 10 x the largest reference term: trajectory, estimates and a second optimize() are bit for bit those
    of the same graph with thresholds 0 (zeroed flag arrays in the views, four outlier passes that find nothing)"""
    for name in ("closures", "mixed"):
        r = R.reference(name)
        top = np.nanmax(R.flat(r["terms"]))
        scale = 10.0 * top / min(t for t in R.flat(R.thresholds_per_edge(r["d"], r["icp"], r["prior"], r["rp"], r["thr"])) if t > 0)
        a, b = full_run(name, scale=scale), full_run(name, thresholds=None)
        a["graph"].close(), b["graph"].close()
        assert not any(len(x) for x in a["rejected"]) and a["n_outliers"] == [0, 0, 0, 0]
        assert not len(a["ba_rejected"][2]) and not len(a["ba_rejected"][3])
        for k in ("1", "2", "3"):
            assert key(a["stats" + k]) == key(b["stats" + k]), (name, k)
            assert np.array_equal(a["pose" + k], b["pose" + k]) and np.array_equal(a["lm" + k], b["lm" + k])


def launches(k, name):
    return k.get(name, dict(launches=0))["launches"]


def test_launch_budget():
    """no pose threshold: no new kernel name, the counts of old.  With thresholds, per optimize() call: one error launch
    per kind group (ICP, prior, relative-pose) and the three launches of the outlier pass per kind; nothing else changes"""
    r = R.reference("mixed")
    scale = 1e6  # (nothing goes: both graphs run the same loop)
    with_t, without = full_run("mixed", scale=scale, timing=True), full_run("mixed", scale=scale, thresholds="ba", timing=True)
    with_t["graph"].close(), without["graph"].close()
    assert key(with_t["stats1"]) == key(without["stats1"])
    k1, k0 = with_t["kernels1"], without["kernels1"]
    print({n: (launches(k1, n), launches(k0, n)) for n in sorted(set(k1) | set(k0))})
    assert not any(n in k0 for n in REJECT_KERNELS + ("pose_outliers",))
    # (k_edge_chi, the BA path's launch behind the loop, is left out below: its events are read with the NEXT call's
    #  times unless the pose-edge pass behind it collects them)
    assert set(k1) - set(k0) - {"k_edge_chi"} == set(REJECT_KERNELS) | {"pose_outliers"}
    for n in REJECT_KERNELS:
        assert launches(k1, n) == 4  # plane, line, prior, relative-pose
    assert launches(k1, "pose_outliers") == 1
    for n in set(k0) - {"k_edge_chi"}:
        extra = 1 if n in ERROR_KERNELS else 0
        assert launches(k1, n) == launches(k0, n) + extra, n
    # a single kind with a threshold: its error launch and its three launches alone
    need_gpu()
    for kind, err in ((cugo.POSE_KIND_PRIOR, "k_prior_errors"), (cugo.POSE_KIND_RELPOSE, "k_relpose_errors"),
                      (cugo.POSE_KIND_LINE, "k_icp_chunks_errors")):
        g = R.build_graph(cugo, r, {k: v for k, v in r["thr"].items() if k == "ba"}, scale=scale)
        {cugo.POSE_KIND_PRIOR: lambda: g.set_prior_outlier_threshold(1e9), cugo.POSE_KIND_RELPOSE: lambda: g.set_relpose_outlier_threshold(1e9),
         cugo.POSE_KIND_LINE: lambda: g.set_icp_outlier_threshold(cugo.ICP_LINE, 1e9)}[kind]()
        g.set_kernel_timing(1)
        g.initialize()
        g.optimize(r["niter"])
        k = g.kernel_times()
        g.close()
        assert all(launches(k, n) == 1 for n in REJECT_KERNELS)
        for n in set(k0) - {"k_edge_chi"}:
            assert launches(k, n) == launches(k0, n) + (1 if n == err else 0), (kind, n)


def test_covariances_after_rejection_are_the_blocks_of_the_dense_inverse_of_the_reduced_system():
    """closures: reject, then compute_covariances() on the same initialisation — the flags are in force, the pattern still
    holds the emptied pair — against the inverse of the reference's dense H of the REDUCED graph at the optimiser's
    estimates.  Bound as in test_relpose_graph.py: 1e-9 of max|Sigma|"""
    need_gpu()
    r = R.reference("closures")
    g = R.build_graph(cugo, r)
    g.initialize()
    g.optimize(r["niter"])
    g.optimize(8)  # (to convergence on the reduced graph)
    pose = g.poses()
    g.compute_covariances(poses=True, landmarks=False)
    cov = g.pose_covariances(np.arange(len(pose)))
    g.close()
    ref = L.RelPoseGraph(dict(r["d2"], pose=pose), r["icp2"], r["prior2"], r["rp2"])
    S = np.linalg.inv(ref.normal_equations()[0])
    full = L.RelPoseGraph(dict(r["d"], pose=pose), r["icp"], r["prior"], r["rp"])
    S_full = np.linalg.inv(full.normal_equations()[0])
    worst = apart = 0.0
    for i in range(len(pose)):
        if r["d"]["pose_fixed"][i]:
            assert not cov[i].any()
            continue
        p = ref.pidx[i]
        worst = max(worst, np.abs(cov[i] - S[6 * p:6 * p + 6, 6 * p:6 * p + 6]).max())
        apart = max(apart, np.abs(cov[i] - S_full[6 * p:6 * p + 6, 6 * p:6 * p + 6]).max())
    print("|Sigma - inv(H reduced) blocks| = %.3g of %.3g; against the unreduced system %.3g" % (worst, np.abs(S).max(), apart))
    assert worst <= 1e-9 * np.abs(S).max() < apart  # (and the unreduced system is told apart by the same bound)


@pytest.mark.parametrize("mode", ["1"])
def test_poisoned_allocations_change_nothing(mode):
    """CUGO_POISON_ALLOC (hip_util.h) in a child process on the mixed case: flags, thresholds, the chi2 terms, the list and
    the workgroup counts are written before they are read, and nothing is stored past a buffer's end"""
    env = dict(os.environ, CUGO_POISON_ALLOC=mode)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p",
                        "no:cacheprovider", "-k", "against_the_reference and mixed"], env=env, capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "guard zone" not in r.stderr and " passed" in r.stdout


# ---- two plane sets with different thresholds: through the C++ interface ------------------------------------------------
ICP_PROGRAM = r"""
#include <cstdio>
#include <deque>
#include <memory>
#include <vector>
#include "cuda_graph_optimisation.h"
#include "icp_types.h"
struct SetIn { int kind, rk; double thr, delta; std::vector<int> pose; std::vector<double> v, w; };
static void print_run(const char* tag, cugo::CudaGraphOptimisationImpl& opt, std::deque<cugo::PoseVertex>& vs)
{
    std::printf("%s", tag);
    for (const auto& s : opt.batchStatistics().get())
        std::printf(" %a", s.chi2);
    std::printf("\n%s_pose", tag);
    for (const auto& v : vs)
    {
        double q[4], t[3];
        v.getEstimate().copyTo(q, t);
        for (double x : q) std::printf(" %a", x);
        for (double x : t) std::printf(" %a", x);
    }
    std::printf("\n");
}
struct Graph
{
    std::deque<cugo::PoseVertex> vs;
    cugo::PoseVertexSet poses{false};
    std::deque<cugo::PlaneEdge> pe;
    std::deque<cugo::LineEdge> le;
    std::vector<std::unique_ptr<cugo::PlaneEdgeSet>> planes;
    std::vector<std::unique_ptr<cugo::LineEdgeSet>> lines;
    std::vector<cugo::BaseEdgeSet*> sets;
    std::vector<std::vector<cugo::BaseEdge*>> edges;
};
// keep: per set and edge, 0 = leave the edge out; thresholds: whether the sets get theirs
static void build(Graph& g, const std::vector<double>& pose7, const std::vector<int>& fixed, const std::vector<SetIn>& in,
                  const std::vector<std::vector<int>>* keep, bool thresholds)
{
    for (size_t i = 0; i < fixed.size(); i++)
    {
        g.vs.emplace_back((int)i, cugo::Se3D(&pose7[7 * i], &pose7[7 * i + 4]), fixed[i] != 0);
        g.poses.addVertex(&g.vs.back());
    }
    for (size_t s = 0; s < in.size(); s++)
    {
        const SetIn& si = in[s];
        const auto rk = si.rk == 3 ? cugo::RobustKernelType::Huber : si.rk == 1 ? cugo::RobustKernelType::Cauchy
                        : si.rk == 2 ? cugo::RobustKernelType::Tukey : cugo::RobustKernelType::None;
        g.edges.emplace_back();
        if (si.kind == 0)
        {
            g.planes.emplace_back(new cugo::PlaneEdgeSet);
            g.planes.back()->setRobustKernel(rk, si.delta);
            if (thresholds) g.planes.back()->setOutlierThreshold(si.thr);
            g.sets.push_back(g.planes.back().get());
        }
        else
        {
            g.lines.emplace_back(new cugo::LineEdgeSet);
            g.lines.back()->setRobustKernel(rk, si.delta);
            if (thresholds) g.lines.back()->setOutlierThreshold(si.thr);
            g.sets.push_back(g.lines.back().get());
        }
        for (size_t e = 0; e < si.pose.size(); e++)
        {
            if (keep && !(*keep)[s][e])
                continue;
            const double* v = &si.v[(si.kind == 0 ? 7 : 9) * e];
            if (si.kind == 0)
            {
                g.pe.emplace_back();
                g.pe.back().setVertex(&g.vs[(size_t)si.pose[e]], 0);
                g.pe.back().setMeasurement(cugo::PointToPlaneMatch<double>(cugo::Vec3d(v + 3), v[6], cugo::Vec3d(v)));
                g.pe.back().setInformation(si.w[e]);
                g.planes.back()->addEdge(&g.pe.back());
                g.edges.back().push_back(&g.pe.back());
            }
            else
            {
                g.le.emplace_back();
                g.le.back().setVertex(&g.vs[(size_t)si.pose[e]], 0);
                cugo::PointToLineMatch<double> mz(cugo::Vec3d(v + 3), cugo::Vec3d(v + 6));
                mz.pointP = cugo::Vec3d(v);
                g.le.back().setMeasurement(mz);
                g.le.back().setInformation(si.w[e]);
                g.lines.back()->addEdge(&g.le.back());
                g.edges.back().push_back(&g.le.back());
            }
        }
    }
}
int main(int argc, char** argv)
{
    std::FILE* f = std::fopen(argv[1], "r");
    int P, n_sets, n1, n2;
    if (!f || std::fscanf(f, "%d %d %d %d", &P, &n_sets, &n1, &n2) != 4) return 2;
    std::vector<double> pose7(7 * (size_t)P);
    std::vector<int> fixed((size_t)P);
    for (int i = 0; i < P; i++)
    {
        if (std::fscanf(f, "%d", &fixed[(size_t)i]) != 1) return 2;
        for (int c = 0; c < 7; c++) if (std::fscanf(f, "%lf", &pose7[7 * (size_t)i + c]) != 1) return 2;
    }
    std::vector<SetIn> in((size_t)n_sets);
    for (SetIn& s : in)
    {
        int n;
        if (std::fscanf(f, "%d %lf %d %lf %d", &s.kind, &s.thr, &s.rk, &s.delta, &n) != 5) return 2;
        const int w = s.kind == 0 ? 7 : 9;
        s.pose.resize((size_t)n), s.v.resize((size_t)w * n), s.w.resize((size_t)n);
        for (int e = 0; e < n; e++)
        {
            if (std::fscanf(f, "%d", &s.pose[(size_t)e]) != 1) return 2;
            for (int c = 0; c < w; c++) if (std::fscanf(f, "%lf", &s.v[(size_t)w * e + c]) != 1) return 2;
            if (std::fscanf(f, "%lf", &s.w[(size_t)e]) != 1) return 2;
        }
    }
    std::fclose(f);
    cugo::GraphOptimisationOptions o;
    o.perEdgeInformation = true;
    o.poseEdgeOutlierRejection = true;
    Graph g;
    build(g, pose7, fixed, in, nullptr, true);
    cugo::CudaGraphOptimisationImpl opt(o);
    opt.addVertexSet(&g.poses);
    for (auto* s : g.sets) opt.addEdgeSet(s);
    opt.initialize();
    opt.optimize(n1);
    print_run("run1", opt, g.vs);
    std::vector<std::vector<int>> keep;
    for (size_t s = 0; s < g.sets.size(); s++)
    {
        std::printf("set%zu outliers %u inliers %u inactive", s, g.sets[s]->getOutlierCount(), g.sets[s]->getInlierCount());
        keep.emplace_back();
        for (size_t e = 0; e < g.edges[s].size(); e++)
        {
            keep.back().push_back(g.edges[s][e]->isActive() ? 1 : 0);
            if (!g.edges[s][e]->isActive()) std::printf(" %zu", e);
        }
        std::printf("\n");
    }
    opt.optimize(n2);
    {   // (the statistics of both calls: the second call's are the last n2)
        std::printf("run2");
        const auto& st = opt.batchStatistics().get();
        for (size_t i = st.size() - (size_t)n2; i < st.size(); i++) std::printf(" %a", st[i].chi2);
        std::printf("\n");
    }
    std::vector<double> mid(7 * (size_t)P);
    for (int i = 0; i < P; i++)
        g.vs[(size_t)i].getEstimate().copyTo(&mid[7 * (size_t)i], &mid[7 * (size_t)i + 4]);
    for (size_t s = 0; s < g.sets.size(); s++)
        for (size_t e = 0; e < g.edges[s].size(); e++)
            if ((g.edges[s][e]->isActive() ? 1 : 0) != keep[s][e]) { std::printf("a second optimize() changed an edge\n"); return 1; }
    opt.initialize();
    opt.optimize(n2);
    print_run("run3", opt, g.vs);
    std::printf("n_icp %d %d\n", opt.nIcpEdges(0), opt.nIcpEdges(1));
    // a fresh optimiser over fresh sets that never held the rejected edges, from the estimates in between, no thresholds
    cugo::GraphOptimisationOptions plain;
    plain.perEdgeInformation = true;
    Graph h;
    build(h, mid, fixed, in, &keep, false);
    cugo::CudaGraphOptimisationImpl fresh(plain);
    fresh.addVertexSet(&h.poses);
    for (auto* s : h.sets) fresh.addEdgeSet(s);
    fresh.initialize();
    fresh.optimize(n2);
    print_run("fresh", fresh, h.vs);
    std::printf("OK\n");
    return 0;
}
"""


def icp_input(r):
    lines = ["%d %d %d %d" % (len(r["d"]["pose"]), len(r["icp"]), r["niter"], r["niter2"])]
    for p, f in zip(r["d"]["pose"], r["d"]["pose_fixed"]):
        lines.append("%d " % f + " ".join("%.17g" % x for x in p))
    for (kind, e, om, act, rk), thr in zip(r["icp"], r["thr"]["icp"]):
        assert np.asarray(act).all()
        om = np.broadcast_to(np.asarray(om, np.float64), (len(act),))
        lines.append("%d %.17g %d %.17g %d" % (0 if kind == "plane" else 1, thr, rk[0], rk[1], len(act)))
        for i in range(len(act)):
            v = np.concatenate([e["p"][i], e["n"][i], [e["d"][i]]] if kind == "plane" else [e["p"][i], e["a"][i], e["b"][i]])
            lines.append("%d " % e["pose"][i] + " ".join("%.17g" % x for x in v) + " %.17g" % om[i])
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("pose_schur", ["1", "0"])
def test_two_plane_sets_with_different_thresholds_through_the_cpp_interface(pose_schur, tmp_path):
    need_gpu()
    r = R.reference("icp")
    (tmp_path / "icp.txt").write_text(icp_input(r))
    src, exe = tmp_path / "icp_outliers.cpp", tmp_path / "icp_outliers"
    src.write_text(ICP_PROGRAM)
    lib_dir = os.path.dirname(cugo.LIB_PATH)
    c = subprocess.run(["g++", "-std=c++17", "-O1", "-I", INC, str(src), "-L", lib_dir, "-lcugo_hip", "-Wl,-rpath," + lib_dir,
                        "-o", str(exe)], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-3000:]
    p = subprocess.run([str(exe), str(tmp_path / "icp.txt")], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, CUGO_POSE_SCHUR=pose_schur))
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    rows = {ln.split()[0]: ln.split()[1:] for ln in p.stdout.splitlines() if ln.strip()}
    hexes = lambda k: [float.fromhex(x) for x in rows[k]]
    # per set: the rejected edges, the counts of the set
    for s, rej in enumerate(r["rej"]["icp"]):
        row = rows["set%d" % s]
        assert [int(x) for x in row[row.index("inactive") + 1:]] == list(np.flatnonzero(rej)), s
        judged = int((~np.isnan(r["terms"]["icp"][s])).sum())  # (edges on the fixed pose are never flattened)
        assert int(row[1]) == int(rej.sum()) and int(row[3]) == judged - int(rej.sum())
    chi1, chi2 = hexes("run1"), hexes("run2")
    for tag, got, tr, tol in (("first", chi1, r["tr"], r["tol"]), ("second", chi2, r["tr2"], r["tol2"])):
        assert len(got) == len(tr)
        for x, t, e in zip(got, tr, tol):
            print(tag, "chi2 %.15g ref %.15g rel %.3g (tol %.3g)" % (x, t["chi2"], abs(x - t["chi2"]) / t["chi2"], e))
            assert abs(x - t["chi2"]) <= e * t["chi2"]
    np.testing.assert_allclose(np.array(hexes("run1_pose")).reshape(-1, 7), r["pose"], rtol=0, atol=r["etol"])
    # the next flattening: bit for bit the fresh sets, and the counts of the reduced graph
    assert rows["run3"] == rows["fresh"] and rows["run3_pose"] == rows["fresh_pose"] and len(rows["run3"]) == r["niter2"]
    free = np.asarray(r["d"]["pose_fixed"]) == 0
    n_kind = {"plane": 0, "line": 0}
    for (kind, e, _, act, _) in r["icp2"]:
        n_kind[kind] += int((np.asarray(act, bool) & free[e["pose"]]).sum())
    assert [int(x) for x in rows["n_icp"]] == [n_kind["plane"], n_kind["line"]]
