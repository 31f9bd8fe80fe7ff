"""Landmark position priors without a GPU: the numpy restatement (tests/lm_prior_ref.py) against central finite
differences and against its own per-entry bounds, what a plan-only optimiser accepts, counts, refuses and re-uses, the
C++ sets (landmark_prior_types.h) and the ctypes layout of cugo_lm_prior_edges."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import kernel_ref as kr
import lm_prior_ref as LR
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "include")
cugo = importlib.import_module("cuda-bundle-adjustment_amd")

KERNELS = [(LR.RK_NONE, 1.0), (LR.RK_CAUCHY, 1.3), (LR.RK_TUKEY, 4.0), (LR.RK_HUBER, 0.8)]


# ---- the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rk", KERNELS, ids=lambda k: "rk%d" % k[0])
def test_gradient_and_chi2_match_central_differences(rk):
    """b is minus half the gradient of chi2 (J = I), and w Omega is the Gauss-Newton block of that chi2"""
    rng = np.random.default_rng(10 + rk[0])
    X, Z, Om = rng.normal(size=3), rng.normal(size=3), LR.random_spd3(rng)
    chi, H, b = LR.edge_terms(X, Z, Om, rk)
    r = X - Z
    x = r @ Om @ r
    rho, w, _ = kr._rho(rk[0], rk[1], np.array([x]), np.float64)
    assert abs(chi - rho[0]) <= 1e-14 * abs(rho[0])
    h = 1e-6
    g = np.array([(LR.edge_terms(X + h * e, Z, Om, rk)[0] - LR.edge_terms(X - h * e, Z, Om, rk)[0]) / (2 * h) for e in np.eye(3)])
    np.testing.assert_allclose(b, -0.5 * g, rtol=1e-6, atol=1e-8 * np.abs(b).max())
    np.testing.assert_allclose(H, w[0] * Om, rtol=1e-14)
    # the derivative of rho: w
    drho = (kr._rho(rk[0], rk[1], np.array([x + h]), np.float64)[0][0] - kr._rho(rk[0], rk[1], np.array([x - h]), np.float64)[0][0]) / (2 * h)
    assert abs(drho - w[0]) <= 1e-6


def ref_case(seed=3, L=40, Lall=44, n=90):
    rng = np.random.default_rng(seed)
    lms = rng.normal(0, 5, (Lall, 3))
    lm = rng.integers(0, Lall, n)
    z = lms[lm] + rng.normal(0, 0.3, (n, 3))
    info = np.array([LR.random_spd3(rng, 3.0) for _ in range(n)])
    return lms, L, LR.make_prior(lm, z, info, rk=(LR.RK_HUBER, 1.0), active=rng.random(n) > 0.15)


def test_reference_build_sums_the_per_edge_terms_and_skips_what_does_not_count():
    lms, L, pr = ref_case()
    ref = LR.reference_build(lms, L, pr, dtype=np.float64)
    H, b, chi = np.zeros((L, 3, 3)), np.zeros((L, 3)), 0.0
    for i, l in enumerate(pr["lm"]):
        if l < L and pr["active"][i]:
            c, h, g = LR.edge_terms(lms[l], pr["z"][i], pr["info"][i], pr["rk"])
            H[l] += h
            b[l] += g
            chi += c
            assert abs(ref["edge_chi"][i] - c) <= 1e-13 * c
        else:
            assert ref["edge_chi"][i] == 0.0
    assert (pr["lm"] >= L).any() and (~pr["active"]).any()
    np.testing.assert_allclose(ref["Hll"], H, rtol=1e-13, atol=1e-13 * np.abs(H).max())
    np.testing.assert_allclose(ref["bl"], b, rtol=1e-13, atol=1e-13 * np.abs(b).max())
    assert abs(ref["chi"] - chi) <= 1e-13 * chi


def test_double_evaluation_is_inside_the_bounds_and_a_wrong_sum_is_not():
    """the bounds hold for the fp64 evaluation of the same formula; a dropped prior, or a prior added to the neighbouring
    landmark, breaks them"""
    lms, L, pr = ref_case()
    ref = LR.reference_build(lms, L, pr)
    bnd = LR.bounds(ref)
    dbl = LR.reference_build(lms, L, pr, dtype=np.float64)
    for k in ("Hll", "bl", "chi", "edge_chi"):
        r = kr.ratio(dbl[k], ref[k], bnd[k])
        print("fp64 against extended precision, %s: %.3g of the bound" % (k, r))
        assert r <= 1
    # a permuted order of the priors is inside as well (the bound is on the formula, not on the order)
    perm = LR.permuted(pr)
    p2 = LR.reference_build(lms, L, perm, dtype=np.float64)
    assert kr.ratio(p2["Hll"], ref["Hll"], bnd["Hll"]) <= 1 and kr.ratio(p2["bl"], ref["bl"], bnd["bl"]) <= 1
    k = int(np.flatnonzero(ref["counts"])[5])
    dropped = dict(pr, active=pr["active"].copy())
    dropped["active"][k] = False
    bad = LR.reference_build(lms, L, dropped, dtype=np.float64)
    assert kr.ratio(bad["Hll"], ref["Hll"], bnd["Hll"]) > 1e6 and kr.ratio(bad["chi"], ref["chi"], bnd["chi"]) > 1e6
    moved = dict(pr, lm=pr["lm"].copy())
    moved["lm"][k] = (pr["lm"][k] + 1) % L
    bad = LR.reference_build(lms, L, moved, dtype=np.float64)
    assert kr.ratio(bad["Hll"], ref["Hll"], bnd["Hll"]) > 1e6 and kr.ratio(bad["bl"], ref["bl"], bnd["bl"]) > 1e6


def test_device_layout_of_the_reference_is_sorted_stably_with_a_csr_over_all_landmarks():
    lms, L, pr = ref_case()
    order, lay = LR.sort_by_landmark(pr, len(lms))
    assert np.all(np.diff(lay["lm"]) >= 0) and lay["lm_ptr"][0] == 0 and lay["lm_ptr"][-1] == len(pr["lm"])
    for l in range(len(lms)):
        mine = order[lay["lm_ptr"][l]:lay["lm_ptr"][l + 1]]
        assert np.all(pr["lm"][mine] == l) and np.all(np.diff(mine) > 0)
    assert lay["meas"].shape == (3, len(order)) and lay["info"].shape == (6, len(order))
    assert lay["info"][4, 7] == pr["info"][order[7], 1, 2]


# ---- plan-only optimisers ------------------------------------------------------------------------------------------
def small_graph(per_edge_information=True, fixed_landmarks=(2, 9)):
    d = synth.make_problem(n_poses=4, n_landmarks=20, seed=3, fixed_landmarks=fixed_landmarks)
    return d, cugo.graph_from_arrays(d, plan_only=True, per_edge_information=per_edge_information)


def observed(d):
    """landmarks (positions in d['lm']) with at least one active BA edge"""
    act = ~((np.asarray(d["pose_fixed"])[d["e_pose"]] != 0) & (np.asarray(d["lm_fixed"])[d["e_lm"]] != 0))
    return np.unique(np.asarray(d["e_lm"])[act])


def prior_args(d, lms=(1, 5, 5)):
    lms = np.asarray(lms, np.int32)
    return lms, d["lm"][lms] + 0.1, np.tile(np.eye(3), (len(lms), 1, 1))


def refused(g, match):
    with pytest.raises(cugo.CugoError, match=match):
        g.initialize()
    g.close()


def test_plan_only_graph_takes_landmark_prior_sets():
    d, g = small_graph()
    assert set([1, 5, 2]) <= set(observed(d).tolist())
    g.add_landmark_priors(*prior_args(d, (1, 5, 5, 2)))    # two on landmark 5, one on the fixed landmark 2
    g.initialize()
    assert g.n_landmark_prior_edges() == 3
    d2, no = small_graph()
    no.initialize()
    assert no.n_landmark_prior_edges() == 0
    assert g.n_active_edges() == no.n_active_edges() + 3
    # unary edges change neither the Hsc pattern nor the symbolic factor
    for k in ("hsc_blocks", "products", "nnzL", "supernodes"):
        assert g.structure_stats()[k] == no.structure_stats()[k], k
    with pytest.raises(cugo.CugoError, match="plan-only"):
        g.optimize(1)
    g.close()
    no.close()


@pytest.mark.parametrize("where", ["position", "information"])
def test_non_finite_values_are_refused(where):
    d, g = small_graph()
    ids, z, info = prior_args(d)
    if where == "position":
        z[1, 2] = np.nan
    else:
        info[2, 0, 1] = info[2, 1, 0] = np.inf
    g.add_landmark_priors(ids, z, info)
    refused(g, "landmark prior edge .*non-finite")


def test_asymmetric_or_indefinite_information_is_refused_and_semi_definite_is_taken():
    d, g = small_graph()
    ids, z, info = prior_args(d)
    info[0, 0, 2] += 1e-9
    g.add_landmark_priors(ids, z, info)
    refused(g, "landmark prior edge .*not symmetric")
    d, g = small_graph()
    info = prior_args(d)[2]
    info[1, 0, 2] += 1e-13  # (inside 1e-12 max|Omega|)
    g.add_landmark_priors(ids, z, info)
    g.initialize()
    g.close()
    d, g = small_graph()
    Q = np.linalg.qr(np.random.default_rng(2).normal(size=(3, 3)))[0]
    bad = Q @ np.diag([5.0, 1.0, -1e-9]) @ Q.T
    g.add_landmark_priors(ids[:1], z[:1], 0.5 * (bad + bad.T))
    refused(g, "landmark prior edge .*positive semi-definite")
    # a height-only prior, a rank-one matrix in a rotated frame and the zero matrix
    d, g = small_graph()
    semi = Q @ np.diag([5.0, 0, 0]) @ Q.T
    g.add_landmark_priors(ids, z, np.array([np.diag([0, 0, 1.0]), 0.5 * (semi + semi.T), np.zeros((3, 3))]))
    g.initialize()
    assert g.n_landmark_prior_edges() == 3
    g.close()
    # without per-edge information the set's matrix is the one that counts, and the one that is checked
    d, g = small_graph(per_edge_information=False)
    g.add_landmark_priors(ids, z, info)
    g.set_landmark_prior_information(-np.eye(3))
    refused(g, "landmark prior edge set .*positive semi-definite")


def test_unknown_landmark_id_is_refused_and_adds_nothing():
    d, g = small_graph()
    ids, z, info = prior_args(d)
    ids[1] = 77
    with pytest.raises(cugo.CugoError, match="unknown landmark id 77"):
        g.add_landmark_priors(ids, z, info)
    g.initialize()
    assert g.n_landmark_prior_edges() == 0
    g.close()


def test_prior_on_a_free_landmark_without_a_ba_edge_is_refused():
    d, g = small_graph()
    g.add_landmarks(np.array([500, 501], np.int32), np.zeros((2, 3)), np.array([0, 1], np.uint8))
    g.add_landmark_priors(np.array([500], np.int32), np.zeros((1, 3)), np.eye(3)[None])
    refused(g, "landmark prior edge set.*no active BA edge")
    # on the FIXED edgeless landmark the prior counts for nothing: taken
    d, g = small_graph()
    g.add_landmarks(np.array([500, 501], np.int32), np.zeros((2, 3)), np.array([0, 1], np.uint8))
    g.add_landmark_priors(np.array([501], np.int32), np.zeros((1, 3)), np.eye(3)[None])
    g.initialize()
    assert g.n_landmark_prior_edges() == 0
    g.close()


def test_sharded_optimiser_refuses_landmark_prior_sets_that_count():
    d, g = small_graph()
    g.add_landmark_priors(*prior_args(d))
    g.set_shard(0, 2, lambda ptr, n, op: None)
    refused(g, "landmark prior edge sets are not supported on a landmark-sharded")
    d, g = small_graph()
    assert d["lm_fixed"][2]
    g.add_landmark_priors(*prior_args(d, (2, 9)))   # fixed landmarks only
    g.set_shard(0, 2, lambda ptr, n, op: None)
    g.initialize()
    assert g.n_landmark_prior_edges() == 0
    g.close()


def test_estimates_only_initialize_with_landmark_prior_sets():
    d, g = small_graph()
    g.add_landmark_priors(*prior_args(d))
    g.initialize()
    assert g.flatten_reuses() == 0 and g.n_landmark_prior_edges() == 3
    g.set_landmarks(np.arange(len(d["lm"]), dtype=np.int32), d["lm"] + 0.01)
    g.initialize()
    assert g.flatten_reuses() == 1 and g.n_landmark_prior_edges() == 3
    # a prior more: a new flattening
    g.add_landmark_priors(*prior_args(d, (7,)))
    g.initialize()
    assert g.flatten_reuses() == 1 and g.n_landmark_prior_edges() == 4
    g.initialize()
    assert g.flatten_reuses() == 2
    # the set's robust kernel or matrix touched: a new flattening, too
    g.set_landmark_prior_robust_kernel(cugo.RK_CAUCHY, 2.0)
    g.initialize()
    assert g.flatten_reuses() == 2
    g.set_landmark_prior_information(2.0 * np.eye(3))
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
#include "landmark_prior_types.h"
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
    options.planOnly = true;
    cugo::CudaGraphOptimisationImpl opt(options);
    cugo::PoseVertexSet poses(false);
    cugo::LandmarkVertexSet lms(true);
    cugo::PoseVertex p0(0, cugo::Se3D(), true), p1(1, cugo::Se3D(), false);
    poses.addVertex(&p0), poses.addVertex(&p1);
    const double x0[3] = {0, 0, 5}, x1[3] = {1, 0, 6}, x2[3] = {0, 1, 7}, x3[3] = {1, 1, 8};
    cugo::LandmarkVertex l0(0, cugo::Vec3d(x0), false), l1(1, cugo::Vec3d(x1), false), l2(2, cugo::Vec3d(x2), true),
        l3(3, cugo::Vec3d(x3), false);
    lms.addVertex(&l0), lms.addVertex(&l1), lms.addVertex(&l2), lms.addVertex(&l3);
    // stereo edges (3-d, like the prior set) from both poses to landmarks 0, 1, 2; landmark 3 has no edge
    cugo::StereoEdgeSet stereo;
    std::vector<cugo::StereoEdge> se(6);
    cugo::LandmarkVertex* lv[3] = {&l0, &l1, &l2};
    const double m[3] = {600, 180, 560};
    for (int i = 0; i < 6; i++)
    {
        se[i].setVertex(i < 3 ? &p0 : &p1, 0), se[i].setVertex(lv[i % 3], 1);
        se[i].setMeasurement(cugo::Vec3d(m));
        se[i].setInformation(1.0);
        se[i].setCamera(cugo::Camera(700.0, 700.0, 600.0, 180.0, 380.0));
        stereo.addEdge(&se[i]);
    }
    cugo::LandmarkPriorEdgeSet priors;
    CHECK(priors.dim() == 3);
    for (int i = 0; i < 9; i++)
        CHECK(priors.informationMatrix()[i] == (i % 4 == 0 ? 1.0 : 0.0));
    cugo::LandmarkPriorMatch<double> dflt;
    CHECK(dflt.point[0] == 0 && dflt.point[2] == 0 && dflt.information[0] == 1 && dflt.information[1] == 0 && dflt.information[8] == 1);
    std::vector<cugo::LandmarkPriorEdge> pe(4);
    double info[9] = {2, 0, 0, 0, 3, 0, 0, 0, 4};
    cugo::LandmarkVertex* on[4] = {&l0, &l0, &l1, &l2}; // the last one sits on the fixed landmark
    for (int i = 0; i < 4; i++)
    {
        pe[i].setMeasurement(cugo::LandmarkPriorMatch<double>(x1, info));
        pe[i].setVertex(on[i], 0);
        priors.addEdge(&pe[i]);
    }
    const auto* pm = static_cast<const cugo::LandmarkPriorMatch<double>*>(pe[1].measurementData());
    CHECK(pm->information[4] == 3.0 && pm->point[2] == 6.0);
    priors.setRobustKernel(cugo::RobustKernelType::Huber, 1.5);
    opt.addVertexSet(&poses), opt.addVertexSet(&lms);
    opt.addEdgeSet(&stereo), opt.addEdgeSet(&priors);
    opt.initialize();
    // the stereo set keeps its own count: the line that sizes the BA arrays does not see the priors
    CHECK(opt.nLandmarkPriorEdges() == 3 && priors.nActiveEdges() == 3 && stereo.nActiveEdges() == 5);
    CHECK(opt.nActiveEdges() == 5 + 3);
    pe[0].inactivate();
    opt.initialize();
    CHECK(opt.nLandmarkPriorEdges() == 2 && opt.nActiveEdges() == 5 + 2 && opt.flattenReuses() == 0);
    opt.initialize();
    CHECK(opt.flattenReuses() == 1);
    // touching a measurement through the mutable pointer, or the set's matrix, forces a new flattening
    static_cast<cugo::LandmarkPriorMatch<double>*>(pe[1].getMeasurement())->information[0] = 3.0;
    opt.initialize();
    CHECK(opt.flattenReuses() == 1);
    priors.setInformationMatrix(info);
    opt.initialize();
    CHECK(opt.flattenReuses() == 1);
    // an outlier threshold on the set is refused, with the kind in the message
    priors.setOutlierThreshold(5.0);
    CHECK(refuses(opt, "outlier rejection is not available on landmark prior edge sets"));
    priors.setOutlierThreshold(0.0);
    opt.initialize();
    // a second set with another robust kernel is refused; with the same one it is taken
    cugo::LandmarkPriorEdgeSet priors2;
    cugo::LandmarkPriorEdge extra;
    extra.setVertex(&l1, 0);
    priors2.addEdge(&extra);
    opt.addEdgeSet(&priors2);
    CHECK(refuses(opt, "landmark prior edge sets of one optimiser must use the same robust kernel"));
    priors2.setRobustKernel(cugo::RobustKernelType::Huber, 1.5);
    opt.initialize();
    CHECK(opt.nLandmarkPriorEdges() == 3);
    // a prior on the free landmark no BA edge observes is refused; inactive, it counts for nothing
    cugo::LandmarkPriorEdge lonely;
    lonely.setVertex(&l3, 0);
    priors2.addEdge(&lonely);
    CHECK(refuses(opt, "no active BA edge"));
    lonely.inactivate();
    opt.initialize();
    CHECK(opt.nLandmarkPriorEdges() == 3);
    // a prior on a landmark vertex of no vertex set of the optimiser is refused
    cugo::LandmarkVertexSet other(true);
    cugo::LandmarkVertex w(9, cugo::Vec3d(x0), false);
    other.addVertex(&w);
    cugo::LandmarkPriorEdge stray;
    stray.setVertex(&w, 0);
    priors2.addEdge(&stray);
    CHECK(refuses(opt, "no landmark vertex set"));
    std::printf("OK\n");
    return 0;
}
"""


def test_cpp_landmark_prior_sets_are_taken_by_a_plan_only_optimiser(tmp_path):
    src = tmp_path / "lm_prior_graph.cpp"
    src.write_text(GRAPH_PROGRAM)
    exe = tmp_path / "lm_prior_graph"
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
#define F(x) std::printf("%s %zu\n", #x, offsetof(cugo_lm_prior_edges, x));
int main()
{
    F(n_landmarks_total) F(n_landmarks_free) F(n) F(d_lm) F(d_lm_ptr) F(d_meas) F(d_info) F(n_info) F(d_flags) F(rk) F(delta)
    std::printf("sizeof %zu\n", sizeof(cugo_lm_prior_edges));
    return 0;
}
"""


def test_ctypes_layout_of_lm_prior_edges_matches_the_c_struct(tmp_path):
    src = tmp_path / "layout.cpp"
    src.write_text(LAYOUT_PROGRAM)
    exe = tmp_path / "layout"
    r = subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split("\n")
               if line)
    assert len(out) == len(cugo.LmPriorEdges._fields_) + 1
    for name, _ in cugo.LmPriorEdges._fields_:
        assert int(out[name]) == getattr(cugo.LmPriorEdges, name).offset, name
    assert int(out["sizeof"]) == C.sizeof(cugo.LmPriorEdges)
