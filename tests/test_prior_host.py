"""SE(3) pose priors without a GPU: the numpy restatement (tests/prior_ref.py) against central finite differences of
the left update, what a plan-only optimiser accepts, counts, refuses and re-uses, the C++ sets (prior_types.h) and the
ctypes layout of cugo_prior_edges."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import icp_ref
import prior_ref as PR
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "include")
cugo = importlib.import_module("cuda-bundle-adjustment_amd")

ANGLES = [0.0, 1e-9, 1e-5, 1e-3, 0.3, 1.0, 3.0]


def fd_jacobian(f, pose7, h=1e-6):
    r0 = f(pose7)
    J = np.zeros((len(r0), 6))
    for k in range(6):
        xi = np.zeros(6)
        xi[k] = h
        J[:, k] = (f(icp_ref.left_update(pose7, xi)) - f(icp_ref.left_update(pose7, -xi))) / (2 * h)
    return J


def pose_at_angle(rng, z, theta):
    """a pose whose residual against z has the rotation angle theta and a translation part of size ~1"""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    return icp_ref.left_update(z, np.concatenate([theta * axis, rng.normal(0, 1.0, 3)]))


@pytest.mark.parametrize("theta", ANGLES)
def test_jacobian_matches_finite_differences(theta):
    """the tolerance tests/test_icp_host.py applies to the ICP Jacobians"""
    rng = np.random.default_rng(int(theta * 1000) + 7)
    z = icp_ref.random_pose(rng)
    pose = pose_at_angle(rng, z, theta)
    r = PR.residual(pose, z)
    assert abs(np.linalg.norm(r[:3]) - theta) <= 1e-12 * max(1.0, theta) + 1e-15
    J = PR.jacobian(pose, z)
    Jfd = fd_jacobian(lambda x: PR.residual(x, z), pose)
    err = np.abs(J - Jfd).max()
    print("theta %g: |J - Jfd| = %.3g" % (theta, err))
    np.testing.assert_allclose(J, Jfd, rtol=0, atol=1e-7 * max(1.0, np.abs(J).max()))


def test_jacobian_is_the_identity_at_zero_residual():
    rng = np.random.default_rng(1)
    z = icp_ref.random_pose(rng)
    # (R R^T is the identity up to rounding only, and J - I is linear in the residual: the same few ulps)
    assert np.abs(PR.residual(z, z)).max() < 1e-15
    assert np.abs(PR.jacobian(z, z) - np.eye(6)).max() < 1e-15
    # where r is exactly zero, J is exactly the identity
    z = np.array([0.0, 0.0, 0.0, 1.0, 3.0, -2.0, 5.0])
    assert not PR.residual(z, z).any()
    assert np.array_equal(PR.jacobian(z, z), np.eye(6))


def test_b_has_the_sign_of_the_build_passes_and_the_vectorised_build_matches_per_edge_terms():
    rng = np.random.default_rng(4)
    poses = np.array([icp_ref.random_pose(rng) for _ in range(4)])
    pose = rng.integers(0, 4, 12)
    z = [PR.displaced(rng, poses[p], 0.3, 0.5) for p in pose]
    info = [PR.random_spd(rng) for _ in pose]
    rk = (PR.RK_CAUCHY, 2.0)
    pr = PR.make_prior(pose, z, info, rk=rk, active=rng.random(12) > 0.2)
    H, b, chi, ce = PR.reference_build(poses, 3, pr)
    H2, b2, chi2 = np.zeros_like(H), np.zeros_like(b), 0.0
    for i, q in enumerate(pose):
        if q < 3 and pr["active"][i]:
            c, h, g = PR.edge_terms(poses[q], pr["z"][i], pr["info"][i], rk)
            H2[q] += h
            b2[q] += g
            chi2 += c
            assert abs(ce[i] - c) <= 1e-12 * c
        else:
            assert ce[i] == 0.0
    np.testing.assert_allclose(H, H2, rtol=1e-12, atol=1e-12 * np.abs(H2).max())
    np.testing.assert_allclose(b, b2, rtol=1e-12, atol=1e-12 * np.abs(b2).max())
    assert abs(chi - chi2) <= 1e-12 * chi2
    # minus half the gradient of chi2 under the left update
    g = np.zeros(6)
    for k in range(6):
        xi = np.zeros(6)
        xi[k] = 1e-6
        f = [PR.edge_terms(icp_ref.left_update(poses[0], s * xi), pr["z"][0], pr["info"][0], (0, 1.0))[0] for s in (1, -1)]
        g[k] = (f[0] - f[1]) / 2e-6
    _, _, b0 = PR.edge_terms(poses[0], pr["z"][0], pr["info"][0], (0, 1.0))
    np.testing.assert_allclose(b0, -0.5 * g, rtol=1e-6, atol=1e-7 * np.abs(b0).max())


# ---- plan-only optimisers ------------------------------------------------------------------------------------------
def test_plan_only_graph_takes_prior_sets():
    d, icp, prior = PR.mixed_prior_case()
    g = PR.build_graph(d, icp, prior, plan_only=True)
    g.initialize()
    n_prior = int((~np.asarray(d["pose_fixed"], bool)[prior["pose"]]).sum())
    assert n_prior == 5 and g.n_prior_edges() == 5  # (the one on the fixed pose 0 is dropped)
    no = PR.build_graph(d, icp, None, plan_only=True)
    no.initialize()
    assert no.n_prior_edges() == 0
    assert g.n_active_edges() == no.n_active_edges() + 5
    # unary edges do not change the Hsc pattern
    assert g.structure_stats()["hsc_blocks"] == no.structure_stats()["hsc_blocks"]
    with pytest.raises(cugo.CugoError, match="plan-only"):
        g.optimize(1)
    g.close()
    no.close()


def test_priors_only_graph_without_a_fixed_pose_is_block_diagonal():
    rng = np.random.default_rng(0)
    P = 5
    pose = np.array([icp_ref.random_pose(rng) for _ in range(P)])
    d = dict(pose=pose, pose_fixed=np.zeros(P, np.uint8), lm=np.zeros((0, 3)), lm_fixed=np.zeros(0, np.uint8),
             e_pose=np.zeros(0, np.int32), e_lm=np.zeros(0, np.int32), e_stereo=np.zeros(0, np.uint8),
             e_meas=np.zeros((0, 3)), e_omega=np.zeros(0), e_cam=np.zeros((0, 5)))
    g = PR.build_graph(d, [], PR.make_prior(np.arange(P), pose, [np.eye(6)]), plan_only=True)
    g.initialize()
    assert g.n_prior_edges() == P and g.n_active_edges() == P
    assert g.structure_stats()["hsc_blocks"] == P
    g.close()


def small_graph(per_edge_information=True):
    d = synth.make_problem(n_poses=4, n_landmarks=20, seed=3)
    return d, cugo.graph_from_arrays(d, plan_only=True, per_edge_information=per_edge_information)


def refused(g, match):
    with pytest.raises(cugo.CugoError, match=match):
        g.initialize()
    g.close()


def prior_args(d, n=2, pose=1):
    return np.full(n, pose, np.int32), np.tile(d["pose"][pose], (n, 1)), np.tile(np.eye(6), (n, 1, 1))


@pytest.mark.parametrize("where", ["quaternion", "translation", "information"])
def test_non_finite_values_are_refused(where):
    d, g = small_graph()
    ids, z, info = prior_args(d)
    if where == "quaternion":
        z[1, 2] = np.nan
    elif where == "translation":
        z[0, 5] = np.inf
    else:
        info[1, 2, 3] = info[1, 3, 2] = np.nan
    g.add_pose_priors(ids, z, info)
    refused(g, "non-finite")


def test_non_unit_measured_quaternion_is_refused_not_normalised():
    d, g = small_graph()
    ids, z, info = prior_args(d)
    z[1, :4] *= 1.0 + 1e-5
    g.add_pose_priors(ids, z, info)
    refused(g, "unit length")
    d, g = small_graph()
    z = prior_args(d)[1]
    z[:, :4] *= 1.0 + 5e-7
    g.add_pose_priors(ids, z, info)
    g.initialize()
    assert g.n_prior_edges() == 2
    g.close()


def test_asymmetric_or_indefinite_information_is_refused_and_semi_definite_is_taken():
    d, g = small_graph()
    ids, z, info = prior_args(d)
    info[0, 1, 4] += 1e-9
    g.add_pose_priors(ids, z, info)
    refused(g, "not symmetric")
    d, g = small_graph()
    info = prior_args(d)[2]
    info[1, 1, 4] += 1e-13  # (inside 1e-12 max|Omega|)
    g.add_pose_priors(ids, z, info)
    g.initialize()
    g.close()
    d, g = small_graph()
    rng = np.random.default_rng(2)
    Q = np.linalg.qr(rng.normal(size=(6, 6)))[0]
    bad = Q @ np.diag([5.0, 3.0, 2.0, 1.0, 0.5, -1e-9]) @ Q.T
    g.add_pose_priors(ids[:1], z[:1], 0.5 * (bad + bad.T))
    refused(g, "positive semi-definite")
    # a translation-only prior, and a rank-one matrix that is singular in a rotated frame
    d, g = small_graph()
    semi = Q @ np.diag([5.0, 0, 0, 0, 0, 0]) @ Q.T
    g.add_pose_priors(ids, z, np.array([np.diag([0, 0, 0, 1.0, 1.0, 1.0]), 0.5 * (semi + semi.T)]))
    g.initialize()
    assert g.n_prior_edges() == 2
    g.close()
    # without per-edge information the set's matrix is the one that counts, and the one that is checked
    d, g = small_graph(per_edge_information=False)
    g.add_pose_priors(ids, z, info)
    g.set_prior_information(-np.eye(6))
    refused(g, "positive semi-definite")


def test_unknown_pose_id_is_refused_and_adds_nothing():
    d, g = small_graph()
    ids, z, info = prior_args(d)
    ids[1] = 77
    with pytest.raises(cugo.CugoError, match="unknown pose id 77"):
        g.add_pose_priors(ids, z, info)
    g.initialize()
    assert g.n_prior_edges() == 0
    g.close()


def test_outlier_threshold_on_a_prior_set_is_refused():
    d, g = small_graph()
    g.add_pose_priors(*prior_args(d))
    g.set_prior_outlier_threshold(5.0)
    refused(g, "outlier rejection is not available")
    d, g = small_graph()
    g.add_pose_priors(*prior_args(d))
    g.set_prior_outlier_threshold(0.0)
    g.initialize()
    g.close()


def test_sharded_optimiser_refuses_prior_sets():
    d, g = small_graph()
    g.add_pose_priors(*prior_args(d))
    g.set_shard(0, 2, lambda ptr, n, op: None)
    refused(g, "sharded")
    # the same shard with priors on the fixed pose only (they count for nothing) is taken
    d, g = small_graph()
    assert d["pose_fixed"][0]
    g.add_pose_priors(*prior_args(d, pose=0))
    g.set_shard(0, 2, lambda ptr, n, op: None)
    g.initialize()
    assert g.n_prior_edges() == 0
    g.close()


def test_estimates_only_initialize_with_prior_sets():
    d, icp, prior = PR.mixed_prior_case()
    g = PR.build_graph(d, icp, prior, plan_only=True)
    g.initialize()
    assert g.flatten_reuses() == 0 and g.n_prior_edges() == 5
    g.set_poses(np.arange(len(d["pose"]), dtype=np.int32), d["pose_gt"])
    g.initialize()
    assert g.flatten_reuses() == 1 and g.n_prior_edges() == 5
    # a prior more: a new flattening
    g.add_pose_priors(*prior_args(d, n=1, pose=3))
    g.initialize()
    assert g.flatten_reuses() == 1 and g.n_prior_edges() == 6
    g.initialize()
    assert g.flatten_reuses() == 2
    # the set's robust kernel or matrix touched: a new flattening, too
    g.set_prior_robust_kernel(cugo.RK_CAUCHY, 2.0)
    g.initialize()
    assert g.flatten_reuses() == 2
    g.set_prior_information(2.0 * np.eye(6))
    g.initialize()
    assert g.flatten_reuses() == 2
    g.close()


GRAPH_PROGRAM = r"""
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>
#include "cuda_graph_optimisation.h"
#include "prior_types.h"
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
    cugo::PosePriorEdgeSet priors;
    CHECK(priors.dim() == 6);
    for (int i = 0; i < 36; i++)
        CHECK(priors.informationMatrix()[i] == (i % 7 == 0 ? 1.0 : 0.0));
    std::vector<cugo::PosePriorEdge> pe(4);
    double info[36] = {0};
    for (int i = 0; i < 6; i++)
        info[7 * i] = 2.0 + i;
    for (int i = 0; i < 4; i++)
    {
        pe[i].setMeasurement(cugo::PosePriorMatch<double>(cugo::Se3D(), info));
        pe[i].setVertex(i < 2 ? &v0 : i < 3 ? &v1 : &v2, 0); // the last one sits on the fixed pose
        priors.addEdge(&pe[i]);
    }
    const auto* pm = static_cast<const cugo::PosePriorMatch<double>*>(pe[1].measurementData());
    CHECK(pm->information[14] == 4.0 && pm->pose.r.w == 1.0);
    priors.setRobustKernel(cugo::RobustKernelType::Huber, 1.5);
    // a graph of priors only: one vertex set, one edge set
    opt.addVertexSet(&poses);
    opt.addEdgeSet(&priors);
    opt.initialize();
    CHECK(opt.nPriorEdges() == 3 && opt.nActiveEdges() == 3 && priors.nActiveEdges() == 3);
    pe[0].inactivate();
    opt.initialize();
    CHECK(opt.nPriorEdges() == 2 && opt.flattenReuses() == 0);
    opt.initialize();
    CHECK(opt.flattenReuses() == 1);
    // touching a measurement through the mutable pointer, or the set's matrix, forces a new flattening
    static_cast<cugo::PosePriorMatch<double>*>(pe[1].getMeasurement())->information[0] = 3.0;
    opt.initialize();
    CHECK(opt.flattenReuses() == 1);
    priors.setInformationMatrix(info);
    opt.initialize();
    CHECK(opt.flattenReuses() == 1);
    // a second prior set with another robust kernel is refused; with the same one it is taken
    cugo::PosePriorEdgeSet priors2;
    cugo::PosePriorEdge extra;
    extra.setVertex(&v0, 0);
    priors2.addEdge(&extra);
    opt.addEdgeSet(&priors2);
    bool threw = false;
    try { opt.initialize(); } catch (const std::runtime_error& e) { threw = std::string(e.what()).find("same robust kernel") != std::string::npos; }
    CHECK(threw);
    priors2.setRobustKernel(cugo::RobustKernelType::Huber, 1.5);
    opt.initialize();
    CHECK(opt.nPriorEdges() == 3);
    // a prior on a pose vertex of no vertex set of the optimiser is refused
    cugo::PoseVertexSet other(false);
    cugo::PoseVertex w(9, cugo::Se3D(), false);
    other.addVertex(&w);
    cugo::PosePriorEdge stray;
    stray.setVertex(&w, 0);
    priors2.addEdge(&stray);
    threw = false;
    try { opt.initialize(); } catch (const std::runtime_error& e) { threw = std::string(e.what()).find("no pose vertex set") != std::string::npos; }
    CHECK(threw);
    std::printf("OK\n");
    return 0;
}
"""


def test_cpp_prior_sets_are_taken_by_a_plan_only_optimiser(tmp_path):
    src = tmp_path / "prior_graph.cpp"
    src.write_text(GRAPH_PROGRAM)
    exe = tmp_path / "prior_graph"
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
#define F(x) std::printf("%s %zu\n", #x, offsetof(cugo_prior_edges, x));
int main()
{
    F(n_poses_total) F(n_poses_free) F(n) F(d_pose) F(d_pose_ptr) F(d_meas) F(d_info) F(n_info) F(d_flags) F(rk) F(delta)
    std::printf("sizeof %zu\n", sizeof(cugo_prior_edges));
    return 0;
}
"""


def test_ctypes_layout_of_prior_edges_matches_the_c_struct(tmp_path):
    src = tmp_path / "layout.cpp"
    src.write_text(LAYOUT_PROGRAM)
    exe = tmp_path / "layout"
    r = subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split("\n")
               if line)
    assert len(out) == len(cugo.PriorEdges._fields_) + 1
    for name, _ in cugo.PriorEdges._fields_:
        assert int(out[name]) == getattr(cugo.PriorEdges, name).offset, name
    assert int(out["sizeof"]) == C.sizeof(cugo.PriorEdges)
