"""Relative-pose SE(3) edges without a GPU: the numpy restatement (tests/relpose_ref.py) against central finite
differences, against the prior reference and against itself with planted mistakes; the host plan and the pattern
through the host-only C ABI; the C++ set (relpose_types.h) refused by initialize(); the plan under a CPU sanitizer."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import icp_ref
import prior_ref as PR
import relpose_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "include")
HOST = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "csrc", "host")
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


def edge_at_angle(rng, theta):
    pa, pb = icp_ref.random_pose(rng), icp_ref.random_pose(rng)
    return pa, pb, RR.measured(rng, pa, pb, trans=1.0, angle=theta)


# ---- the term ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta", ANGLES)
def test_both_jacobians_match_central_differences(theta):
    """the tolerance tests/test_prior_host.py applies to the prior's Jacobian (differencing error at h = 1e-6)"""
    rng = np.random.default_rng(int(theta * 1000) + 3)
    worst = 0.0
    for _ in range(3):
        pa, pb, z = edge_at_angle(rng, theta)
        r = RR.residual(pa, pb, z)
        assert abs(np.linalg.norm(r[:3]) - theta) <= 1e-9 * max(1.0, theta) + 1e-15
        Ja, Jb = RR.jacobians(pa, pb, z)
        Ja_fd = fd_jacobian(lambda x: RR.residual(x, pb, z), pa)
        Jb_fd = fd_jacobian(lambda x: RR.residual(pa, x, z), pb)
        worst = max(worst, np.abs(Ja - Ja_fd).max(), np.abs(Jb - Jb_fd).max())
        np.testing.assert_allclose(Ja, Ja_fd, rtol=0, atol=1e-7 * max(1.0, np.abs(Ja).max()))
        np.testing.assert_allclose(Jb, Jb_fd, rtol=0, atol=1e-7 * max(1.0, np.abs(Jb).max()))
    print("theta %g: worst |J - Jfd| = %.3g" % (theta, worst))


def small_graph(seed=2, rk=(RR.RK_NONE, 1.0)):
    """3 free poses (0..2) + 1 fixed (3): a triangle, a duplicate in the other orientation, an edge to the fixed pose"""
    rng = np.random.default_rng(seed)
    poses = np.array([icp_ref.random_pose(rng) for _ in range(4)])
    rp = RR.random_edges(rng, poses, [(0, 1), (2, 1), (0, 2), (1, 0), (3, 1), (2, 3)], rk=rk, rot=0.1, trans=0.3)
    return poses, rp


def test_b_is_minus_half_the_gradient_and_the_solved_step_goes_downhill():
    poses, rp = small_graph()
    H, b, Hoff, chi0, _ = RR.reference_build(poses, 3, rp)
    g = np.zeros((3, 6))
    for p in range(3):
        for k in range(6):
            xi = np.zeros(6)
            xi[k] = 1e-6
            f = []
            for s in (1, -1):
                moved = poses.copy()
                moved[p] = icp_ref.left_update(poses[p], s * xi)
                f.append(RR.total_chi2(moved, 3, rp))
            g[p, k] = (f[0] - f[1]) / 2e-6
    np.testing.assert_allclose(b, -0.5 * g, rtol=1e-6, atol=1e-7 * np.abs(b).max())
    rowptr, colind = RR.pattern(rp, 3)
    A, rhs = RR.dense_system(H, b, Hoff, rowptr, colind)
    assert np.abs(A - A.T).max() <= 1e-13 * np.abs(A).max() and np.linalg.eigvalsh(0.5 * (A + A.T)).min() > 0
    dx = np.linalg.solve(A, rhs).reshape(3, 6)
    chi1 = []
    for s in (1.0, -1.0):  # (the measurements carry independent noise: the minimum is not zero)
        moved = poses.copy()
        for p in range(3):
            moved[p] = icp_ref.left_update(poses[p], s * dx[p])
        chi1.append(RR.total_chi2(moved, 3, rp))
    print("chi2 %.6g -> %.6g (exp(+dx)), %.6g (exp(-dx))" % (chi0, chi1[0], chi1[1]))
    assert chi1[0] < 0.5 * chi0 and chi1[1] > chi0
    # the off-diagonal blocks matter: without them the step is another one
    A0, _ = RR.dense_system(H, b, 0 * Hoff, rowptr, colind)
    assert np.abs(np.linalg.solve(A0, rhs) - dx.reshape(-1)).max() > 1e-3 * np.abs(dx).max()


@pytest.mark.parametrize("rk", [(0, 1.0), (3, 0.5)])
def test_with_the_fixed_identity_as_b_the_edge_is_the_prior(rk):
    rng = np.random.default_rng(6)
    poses = np.array([icp_ref.random_pose(rng) for _ in range(2)] + [RR.IDENTITY])
    z = np.array([PR.displaced(rng, poses[p], 0.2, 0.4) for p in (0, 1, 1)])
    info = np.array([PR.random_spd(rng) for _ in range(3)])
    rp = RR.make_edges([0, 1, 1], [2, 2, 2], z, info, rk=rk)
    H, b, Hoff, chi, ce = RR.reference_build(poses, 2, rp)
    Hp, bp, chip, cep = PR.reference_build(poses, 2, PR.make_prior([0, 1, 1], z, info, rk=rk))
    np.testing.assert_allclose(H, Hp, rtol=0, atol=1e-13 * np.abs(Hp).max())
    np.testing.assert_allclose(b, bp, rtol=0, atol=1e-13 * np.abs(bp).max())
    np.testing.assert_allclose(ce, cep, rtol=1e-13)
    assert abs(chi - chip) <= 1e-13 * chip and len(Hoff) == 2 and not Hoff.any()


def swapped(z, Om):
    """the edge (b, a) that states the same constraint to first order: Z^-1, and Omega carried by the linear map M of
    r' = M r + O(|r|^2), M = [[-R_z^T, 0], [R_z^T [t_z]x, -R_z^T]]"""
    Rz = RR.synth.quat_to_R(z[:4])
    M = np.zeros((6, 6))
    M[:3, :3] = M[3:, 3:] = -Rz.T
    M[3:, :3] = Rz.T @ icp_ref.skew(z[4:])
    Mi = np.linalg.inv(M)
    return RR.pose_inv(z), Mi.T @ Om @ Mi, M


def test_swapping_the_ends_changes_the_cost_by_one_order_in_r_only():
    """What is invariant under (a, b, Z) -> (b, a, Z^-1): D' = Z^-1 D^-1 Z, so the rotation angle |phi| exactly, and
    the residual to first order, r' = M r + O(|r|^2) with the M of swapped().  What is not: the translation part of the
    residual is t_D, not the translation of the SE(3) logarithm, so r' = M r holds to first order only, and Omega has
    to be carried along (Omega' = M^-T Omega M^-1): with the SAME Omega the two edges are different costs.  With the
    carried Omega the costs agree to a relative O(|r|): checked at two residual sizes, whose relative differences scale
    with the size."""
    rng = np.random.default_rng(12)
    rel = []
    for scale in (1e-2, 1e-4):
        pa, pb = icp_ref.random_pose(rng), icp_ref.random_pose(rng)
        z = RR.measured(rng, pa, pb, rot=scale, trans=scale)
        Om = PR.random_spd(rng)
        r = RR.residual(pa, pb, z)
        zi, Omi, M = swapped(z, Om)
        r2 = RR.residual(pb, pa, zi)
        assert abs(np.linalg.norm(r2[:3]) - np.linalg.norm(r[:3])) <= 1e-10 * scale + 1e-15
        nr = np.linalg.norm(r)
        assert np.abs(r2 - M @ r).max() <= 10 * (1 + np.linalg.norm(z[4:])) * nr * nr
        c1, c2 = r @ Om @ r, r2 @ Omi @ r2
        rel.append(abs(c1 - c2) / c1)
        print("scale %g: |r| %.3g  chi2 %.6g swapped %.6g  rel %.3g" % (scale, nr, c1, c2, rel[-1]))
        assert rel[-1] <= 20 * (1 + np.linalg.norm(z[4:])) * nr * np.linalg.cond(Om)
        # the same Omega on the swapped edge is another cost
        assert abs(r2 @ Om @ r2 - c1) > 1e-2 * c1
    assert 10 < rel[0] / rel[1] < 1000


# ---- planted mistakes -------------------------------------------------------------------------------------------
def differs(got, want, rel=1e-12):
    return np.abs(got - want).max() > rel * max(np.abs(want).max(), 1e-300)


def test_planted_mistakes_break_the_comparison():
    """the bound of tests/test_relpose.py (1e-12 of max|.|) separates each of these from the correct build"""
    poses, rp = small_graph(seed=4)
    rowptr, colind = RR.pattern(rp, 3)
    H, b, Hoff, chi, _ = RR.reference_build(poses, 3, rp, rowptr, colind)
    # the same build with the edges in another order agrees: the bound is not met by accident
    perm = np.random.default_rng(0).permutation(len(rp["a"]))
    rp2 = dict(rp, **{k: rp[k][perm] for k in ("a", "b", "z", "info", "active")})
    H2, b2, Hoff2, chi2, _ = RR.reference_build(poses, 3, rp2, rowptr, colind)
    assert not differs(H2, H) and not differs(b2, b) and not differs(Hoff2, Hoff) and abs(chi2 - chi) <= 1e-12 * chi
    _, _, _, chi_m, _ = RR.reference_build(poses, 3, rp, rowptr, colind, mistake="chi2_twice")
    assert abs(chi_m - chi) > 1e-12 * chi
    Hm, bm, Hoffm, _, _ = RR.reference_build(poses, 3, rp, rowptr, colind, mistake="transposed")
    assert differs(Hoffm, Hoff) and not differs(Hm, H)
    Hm, bm, Hoffm, _, _ = RR.reference_build(poses, 3, rp, rowptr, colind, mistake="no_tA")
    assert differs(Hm, H) and differs(bm, b) and differs(Hoffm, Hoff)
    Hm, bm, Hoffm, _, _ = RR.reference_build(poses, 3, rp, rowptr, colind, mistake="overwrite")
    assert differs(Hoffm, Hoff) and not differs(Hm, H)


# ---- the plan through the host-only ABI -------------------------------------------------------------------------
def designed_graph():
    """5 free + 2 fixed poses: duplicates in both orientations, edges to fixed poses from either side, a fixed-fixed
    edge, inactive edges (one of them the only edge of its pair), a free pose without any edge (4)"""
    a = [0, 1, 1, 3, 5, 2, 6, 5, 0, 3, 2]
    b = [1, 0, 0, 2, 0, 6, 3, 6, 3, 1, 3]
    active = np.ones(len(a), bool)
    active[[2, 9]] = False  # a duplicate of (0, 1), and the only (1, 3) edge
    rng = np.random.default_rng(1)
    poses = np.array([icp_ref.random_pose(rng) for _ in range(7)])
    rp = RR.random_edges(rng, poses, list(zip(a, b)))
    rp["active"] = active
    return poses, rp


def test_plan_lists_and_block_indices_match_the_restatement():
    poses, rp = designed_graph()
    rowptr, colind = RR.pattern(rp, 5)
    assert list(rowptr) == [0, 3, 4, 6, 7, 8] and list(colind) == [0, 1, 3, 1, 2, 3, 3, 4]
    pl = cugo.RelPosePlan(None, 7, 5, rp["a"], rp["b"], RR.flags_of(rp), rowptr, colind)
    inc_ptr, inc, off = RR.plan(rp, 5, rowptr, colind)
    assert np.array_equal(pl.array("inc_ptr"), inc_ptr)
    assert np.array_equal(pl.array("inc"), inc)
    assert np.array_equal(pl.array("off_blk"), off)
    # spelled out: pose 0 sees edges 0 (as a), 1 (as b), 4 (as b), 8 (as a); pose 4 nothing
    assert list(inc[inc_ptr[0]:inc_ptr[1]]) == [0, 3, 9, 16] and inc_ptr[4] == inc_ptr[5]
    assert list(off) == [1, 1, -1, 5, -1, -1, -1, -1, 2, -1, 5]
    with pytest.raises(cugo.CugoError, match="unknown array"):
        pl.array("nothing")
    pl.close()
    # a larger pattern (the engine's Hsc will have more blocks than the pose graph needs) is taken: indices follow it
    full_ptr = np.arange(0, 16, 1, dtype=np.int32)[[0, 5, 9, 12, 14, 15]]
    full_ind = np.concatenate([np.arange(p, 5) for p in range(5)]).astype(np.int32)
    pl = cugo.RelPosePlan(None, 7, 5, rp["a"], rp["b"], RR.flags_of(rp), full_ptr, full_ind)
    assert np.array_equal(pl.array("off_blk"), RR.plan(rp, 5, full_ptr, full_ind)[2])
    pl.close()


def test_plan_refusals():
    poses, rp = designed_graph()
    rowptr, colind = RR.pattern(rp, 5)
    fl = RR.flags_of(rp)

    def refused(match, a=rp["a"], b=rp["b"], flags=fl, rowptr=rowptr, colind=colind, Pall=7):
        with pytest.raises(cugo.CugoError, match=match):
            cugo.RelPosePlan(None, Pall, 5, a, b, flags, rowptr, colind)

    for bad in (7, -1):
        a = rp["a"].copy()
        a[3] = bad
        refused("edge 3: pose index out of range", a=a)
        b = rp["b"].copy()
        b[10] = bad
        refused("edge 10: pose index out of range", b=b)
    b = rp["b"].copy()
    b[4] = 5
    refused("edge 4 joins pose 5 to itself", b=b)
    b[4], b[2] = 0, 1  # (an inactive edge is refused as well)
    refused("edge 2 joins pose 1 to itself", b=b)
    # the inactive edge 9 becomes active: its pair (1, 3) is not in the pattern
    refused(r"edge 9: block \(1, 3\) is missing from the pattern", flags=np.zeros(len(fl), np.uint8))
    refused(r"edge 9: block \(1, 3\) is missing from the pattern", flags=None)
    # patterns of another form
    ci = colind.copy()
    ci[0], ci[1] = 1, 0
    refused("does not start with its diagonal block", colind=ci)
    ci = colind.copy()
    ci[1], ci[2] = 3, 1
    refused("not ascending", colind=ci)
    refused("bad pose or edge counts", Pall=4)


def test_pattern_matches_a_dense_adjacency():
    rng = np.random.default_rng(5)
    P, Pall, E = 23, 27, 90
    a = rng.integers(0, Pall, E)
    b = (a + rng.integers(1, Pall, E)) % Pall
    active = rng.random(E) > 0.2
    flags = np.where(active, 0, cugo.EDGE_INACTIVE).astype(np.uint8)
    rowptr, colind = cugo.relpose_pattern(P, a, b, flags)
    adj = np.eye(P, dtype=bool)
    for x, y, f in zip(a, b, active):
        if f and x < P and y < P:
            adj[min(x, y), max(x, y)] = True
    rr, cc = np.nonzero(np.triu(adj))
    assert np.array_equal(colind, cc) and np.array_equal(rowptr, np.searchsorted(rr, np.arange(P + 1)))
    rp_, ci_ = RR.pattern(dict(a=a, b=b, active=active), P)
    assert np.array_equal(rowptr, rp_) and np.array_equal(colind, ci_)
    # no edges, no flags
    rowptr, colind = cugo.relpose_pattern(3, [], [])
    assert list(rowptr) == [0, 1, 2, 3] and list(colind) == [0, 1, 2]
    with pytest.raises(cugo.CugoError, match="joins pose 2 to itself"):
        cugo.relpose_pattern(3, [0, 2], [1, 2])
    with pytest.raises(cugo.CugoError, match="negative"):
        cugo.relpose_pattern(3, [0, -1], [1, 2])


# ---- C++ ----------------------------------------------------------------------------------------------------------
GRAPH_PROGRAM = r"""
#include <cstdio>
#include <stdexcept>
#include <string>
#include "cuda_graph_optimisation.h"
#include "relpose_types.h"
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)
// a 6-d set that is neither a prior set nor a relative-pose set
class OtherSet : public cugo::EdgeSet<6, cugo::PosePriorMatch<double>, cugo::PoseVertex> {};
static std::string refusal(cugo::CudaGraphOptimisationImpl& opt)
{
    try { opt.initialize(); } catch (const std::runtime_error& e) { return e.what(); }
    return "";
}
int main()
{
    cugo::GraphOptimisationOptions options;
    options.perEdgeInformation = true;
    options.planOnly = true;
    cugo::PoseVertexSet poses(false);
    cugo::PoseVertex v0(0, cugo::Se3D(), false), v1(1, cugo::Se3D(), false), v2(2, cugo::Se3D(), true);
    poses.addVertex(&v0), poses.addVertex(&v1), poses.addVertex(&v2);
    cugo::RelPoseEdgeSet rel;
    CHECK(rel.dim() == 6);
    for (int i = 0; i < 36; i++)
        CHECK(rel.informationMatrix()[i] == (i % 7 == 0 ? 1.0 : 0.0));
    double info[36] = {0};
    for (int i = 0; i < 6; i++)
        info[7 * i] = 2.0 + i;
    cugo::RelPoseEdge e01, e12;
    e01.setMeasurement(cugo::PosePriorMatch<double>(cugo::Se3D(), info));
    e01.setVertex(&v0, 0), e01.setVertex(&v1, 1);
    e12.setVertex(&v1, 0), e12.setVertex(&v2, 1);
    rel.addEdge(&e01), rel.addEdge(&e12);
    CHECK(rel.nedges() == 2 && e01.getVertex(0) == &v0 && e01.getVertex(1) == &v1 && e01.dim() == 6);
    CHECK(!e01.allVerticesFixed() && e01.allVerticesNotFixed() && !e12.allVerticesNotFixed());
    const auto* pm = static_cast<const cugo::PosePriorMatch<double>*>(e01.measurementData());
    CHECK(pm->information[14] == 4.0 && pm->pose.r.w == 1.0);
    rel.setInformationMatrix(info);
    CHECK(rel.informationMatrix()[35] == 7.0);
    {
        cugo::CudaGraphOptimisationImpl opt(options);
        opt.addVertexSet(&poses);
        opt.addEdgeSet(&rel);
        const std::string w = refusal(opt);
        std::printf("refusal: %s\n", w.c_str());
        CHECK(w.find("relative-pose") != std::string::npos && w.find("cugo_relpose_") != std::string::npos);
    }
    {   // next to a prior set: still refused, whichever comes first
        cugo::PosePriorEdgeSet priors;
        cugo::PosePriorEdge p;
        p.setVertex(&v0, 0);
        priors.addEdge(&p);
        cugo::CudaGraphOptimisationImpl opt(options);
        opt.addVertexSet(&poses);
        opt.addEdgeSet(&priors);
        opt.addEdgeSet(&rel);
        CHECK(refusal(opt).find("cugo_relpose_") != std::string::npos);
        // the prior set alone is taken as before
        cugo::CudaGraphOptimisationImpl opt2(options);
        opt2.addVertexSet(&poses);
        opt2.addEdgeSet(&priors);
        opt2.initialize();
        CHECK(opt2.nPriorEdges() == 1);
    }
    {   // a 6-d set of neither kind gets the message it always got
        OtherSet other;
        cugo::CudaGraphOptimisationImpl opt(options);
        opt.addVertexSet(&poses);
        opt.addEdgeSet(&other);
        CHECK(refusal(opt).find("a 6-d edge set must be a PosePriorEdgeSet") != std::string::npos);
    }
    std::printf("OK\n");
    return 0;
}
"""


def test_cpp_relpose_set_is_refused_by_initialize_naming_the_kernel_level_entry_points(tmp_path):
    src = tmp_path / "relpose_graph.cpp"
    src.write_text(GRAPH_PROGRAM)
    exe = tmp_path / "relpose_graph"
    lib_dir = os.path.dirname(cugo.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", INC, str(src), "-L", lib_dir, "-lcugo_hip",
                        "-Wl,-rpath," + lib_dir, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr


PLAN_PROGRAM = r"""
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>
#include "relpose_plan.h"
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)
using namespace cugo_host;
static std::string refused(int n, int Pall, int P, const std::vector<int32_t>& a, const std::vector<int32_t>& b,
                           const uint8_t* fl, const std::vector<int32_t>& rp, const std::vector<int32_t>& ci)
{
    RelPosePlanHost h;
    try { build_relpose_plan(n, Pall, P, a.data(), b.data(), fl, rp.data(), ci.data(), h); }
    catch (const std::invalid_argument& e) { return e.what(); }
    return "";
}
int main()
{
    // the designed graph of the Python test: 5 free + 2 fixed poses
    const std::vector<int32_t> a = {0, 1, 1, 3, 5, 2, 6, 5, 0, 3, 2}, b = {1, 0, 0, 2, 0, 6, 3, 6, 3, 1, 3};
    std::vector<uint8_t> fl(a.size(), 0);
    fl[2] = fl[9] = 8;
    const int n = (int)a.size();
    std::vector<int32_t> rp(6);
    const int nnzb = relpose_pattern(n, 5, a.data(), b.data(), fl.data(), rp.data(), nullptr);
    CHECK(nnzb == 8 && rp[5] == 8);
    std::vector<int32_t> ci((size_t)nnzb);
    CHECK(relpose_pattern(n, 5, a.data(), b.data(), fl.data(), rp.data(), ci.data()) == 8);
    RelPosePlanHost h;
    build_relpose_plan(n, 7, 5, a.data(), b.data(), fl.data(), rp.data(), ci.data(), h);
    CHECK(h.nnzb == 8 && (int)h.inc.size() == h.inc_ptr[5] && h.inc_ptr[5] == 13 && (int)h.off_blk.size() == n);
    CHECK(h.inc[0] == 0 && h.inc[1] == 3 && h.inc[2] == 9 && h.inc[3] == 16);
    CHECK(h.off_blk[0] == 1 && h.off_blk[1] == 1 && h.off_blk[2] == -1 && h.off_blk[3] == 5 && h.off_blk[8] == 2);
    // every refusal leaves through an exception, with nothing read out of range on the way
    CHECK(refused(n, 7, 5, a, b, nullptr, rp, ci).find("missing from the pattern") != std::string::npos);
    std::vector<int32_t> a2 = a;
    a2[10] = 7;
    CHECK(refused(n, 7, 5, a2, b, fl.data(), rp, ci).find("out of range") != std::string::npos);
    a2[10] = -3;
    CHECK(refused(n, 7, 5, a2, b, fl.data(), rp, ci).find("out of range") != std::string::npos);
    a2[10] = 3;
    CHECK(refused(n, 7, 5, a2, b, fl.data(), rp, ci).find("to itself") != std::string::npos);
    std::vector<int32_t> ci2 = ci;
    ci2[2] = 9;
    CHECK(refused(n, 7, 5, a, b, fl.data(), rp, ci2).find("leaves the free poses") != std::string::npos);
    std::vector<int32_t> rp2 = rp;
    rp2[2] = rp2[1];
    CHECK(!refused(n, 7, 5, a, b, fl.data(), rp2, ci).empty());
    // empty inputs
    RelPosePlanHost e;
    const int32_t zero = 0;
    build_relpose_plan(0, 0, 0, nullptr, nullptr, nullptr, &zero, nullptr, e);
    CHECK(e.inc_ptr.size() == 1 && e.inc.empty() && e.off_blk.empty());
    std::printf("OK\n");
    return 0;
}
"""


def test_host_plan_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """relpose_plan.cpp needs no HIP header: compiled with g++ -fsanitize=address,undefined next to a main of its own"""
    src = tmp_path / "plan_main.cpp"
    src.write_text(PLAN_PROGRAM)
    exe = tmp_path / "plan_main"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", HOST, str(src), os.path.join(HOST, "relpose_plan.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr[-3000:]


LAYOUT_PROGRAM = r"""
#include <cstddef>
#include <cstdio>
#include "cugo_hip.h"
#define F(x) std::printf("%s %zu\n", #x, offsetof(cugo_relpose_edges, x));
int main()
{
    F(n_poses_total) F(n_poses_free) F(n) F(d_meas) F(d_info) F(n_info) F(d_flags) F(rk) F(delta) F(plan)
    std::printf("sizeof %zu\n", sizeof(cugo_relpose_edges));
    return 0;
}
"""


def test_ctypes_layout_of_relpose_edges_matches_the_c_struct(tmp_path):
    src = tmp_path / "layout.cpp"
    src.write_text(LAYOUT_PROGRAM)
    exe = tmp_path / "layout"
    r = subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split("\n")
               if line)
    assert len(out) == len(cugo.RelPoseEdges._fields_) + 1
    for name, _ in cugo.RelPoseEdges._fields_:
        assert int(out[name]) == getattr(cugo.RelPoseEdges, name).offset, name
    assert int(out["sizeof"]) == C.sizeof(cugo.RelPoseEdges)
