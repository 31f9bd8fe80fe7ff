"""Point-to-plane / point-to-line pose edges without a GPU: the numpy restatement (tests/icp_ref.py) against
central finite differences of the left update, the mirrored public headers (include/icp_types.h,
measurements.h) against the reference's sample and API, and the ctypes layout of cugo_icp_edges."""
import ctypes as C
import importlib
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import icp_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "include")
REF_SAMPLE = "/root/reference/samples/sample_ba_from_file/main.cpp"
cugo = importlib.import_module("cuda-bundle-adjustment_amd")


def fd_jacobian(f, pose7, h=1e-6):
    r0 = f(pose7)
    J = np.zeros((len(r0), 6))
    for k in range(6):
        xi = np.zeros(6)
        xi[k] = h
        J[:, k] = (f(icp_ref.left_update(pose7, xi)) - f(icp_ref.left_update(pose7, -xi))) / (2 * h)
    return J


@pytest.mark.parametrize("seed", range(5))
def test_plane_jacobian_matches_finite_differences(seed):
    rng = np.random.default_rng(seed)
    pose = icp_ref.random_pose(rng)
    n = rng.normal(size=3)
    n /= np.linalg.norm(n)
    d, p = rng.normal(), rng.normal(0, 3, 3)
    J = icp_ref.plane_jacobian(pose, n, d, p)
    Jfd = fd_jacobian(lambda x: icp_ref.plane_residual(x, n, d, p), pose)
    assert J.shape == (1, 6)
    np.testing.assert_allclose(J, Jfd, rtol=0, atol=1e-7 * max(1.0, np.abs(J).max()))
    # the residual is the signed distance of y to the plane
    y = icp_ref.transform(pose, p)
    assert abs(icp_ref.plane_residual(pose, n, d, p)[0] - (n @ y - d)) < 1e-14 * max(1.0, abs(d) + np.abs(y).sum())


@pytest.mark.parametrize("seed", range(5))
def test_line_jacobian_matches_finite_differences(seed):
    rng = np.random.default_rng(100 + seed)
    pose = icp_ref.random_pose(rng)
    a, b, p = rng.normal(0, 3, 3), rng.normal(0, 3, 3), rng.normal(0, 3, 3)
    u = icp_ref.line_direction(a, b)
    J = icp_ref.line_jacobian(pose, a, u, p)
    Jfd = fd_jacobian(lambda x: icp_ref.line_residual(x, a, u, p), pose)
    assert J.shape == (3, 6)
    np.testing.assert_allclose(J, Jfd, rtol=0, atol=1e-7 * max(1.0, np.abs(J).max()))
    # |r| is the point-to-line distance: |(y - a) x u|
    y = icp_ref.transform(pose, p)
    r = icp_ref.line_residual(pose, a, u, p)
    assert abs(np.linalg.norm(r) - np.linalg.norm(np.cross(y - a, u))) < 1e-12


def test_vectorised_reference_build_matches_per_edge_terms():
    rng = np.random.default_rng(7)
    poses = np.array([icp_ref.random_pose(rng) for _ in range(4)])
    kinds = []
    for kind in ("plane", "line"):
        e = icp_ref.make_edges(rng, rng.integers(0, 4, 30), kind, poses, noise=0.3)
        kinds.append((kind, e, rng.uniform(0.5, 2, 30), rng.random(30) > 0.2, (icp_ref.RK_CAUCHY, 0.4)))
    H, b, chi, _ = icp_ref.reference_build(poses, 3, kinds)
    H2, b2, chi2 = np.zeros_like(H), np.zeros_like(b), 0.0
    for kind, e, om, act, rk in kinds:
        for i, q in enumerate(e["pose"]):
            if q < 3 and act[i]:
                c, h, g = icp_ref.edge_terms(kind, e, i, poses[q], om[i], rk)
                H2[q] += h
                b2[q] += g
                chi2 += c
    np.testing.assert_allclose(H, H2, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(b, b2, rtol=1e-12, atol=1e-12)
    assert abs(chi - chi2) <= 1e-12 * chi2


@pytest.mark.skipif(not os.path.exists(REF_SAMPLE), reason="reference checkout not present")
def test_reference_sample_type_checks_against_product_headers_without_icp_stub(tmp_path):
    # only the OpenCV stand-in is used: icp_types.h must come from the product's headers
    shutil.copytree(os.path.join(ROOT, "tests", "boundary_stubs", "opencv2"), tmp_path / "opencv2")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", INC, "-I", str(tmp_path), REF_SAMPLE],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


API_PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include "icp_types.h"
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)
int main()
{
    cugo::PoseVertexSet poses(false);
    cugo::PoseVertex v0(0, cugo::Se3D(), false), v1(1, cugo::Se3D(), true);
    poses.addVertex(&v0);
    poses.addVertex(&v1);
    cugo::PlaneEdgeSet planes;
    cugo::LineEdgeSet lines;
    CHECK(planes.dim() == 1 && lines.dim() == 1);
    cugo::PlaneEdge pe;
    cugo::Vec3d n, p;
    n[0] = 0, n[1] = 0, n[2] = 1;
    p[0] = 1, p[1] = 2, p[2] = 3;
    pe.setMeasurement(cugo::PointToPlaneMatch<double>(n, 2.5, p));
    pe.setVertex(&v0, 0);
    pe.setInformation(4.0);
    planes.addEdge(&pe);
    const auto* pm = static_cast<const cugo::PointToPlaneMatch<double>*>(pe.measurementData());
    CHECK(pm->normal[2] == 1 && pm->originDistance == 2.5 && pm->pointP[1] == 2);
    cugo::LineEdge le;
    cugo::Vec3d a, b;
    a[0] = 1, a[1] = 1, a[2] = 1;
    b[0] = 4, b[1] = 5, b[2] = 1;
    cugo::PointToLineMatch<double> lm(a, b);
    lm.pointP = p;
    CHECK(std::fabs(lm.length - 5.0) < 1e-15);
    CHECK(lm.start()[0] == 1 && lm.end()[1] == 5);
    le.setMeasurement(lm);
    le.setVertex(&v1, 0);
    lines.addEdge(&le);
    const auto* lmm = static_cast<const cugo::PointToLineMatch<double>*>(le.measurementData());
    CHECK(lmm->a[0] == 1 && lmm->b[1] == 5 && lmm->pointP[2] == 3 && lmm->length == lm.length);
    CHECK(planes.nedges() == 1 && lines.nedges() == 1);
    CHECK(v0.getEdges().size() == 1 && le.allVerticesFixed() && !pe.allVerticesFixed());
    // a new measurement counts as one change of the set, and so does handing out the mutable measurement pointer;
    // reading through measurementData() does not
    const unsigned long long c0 = planes.changeCount();
    pe.setMeasurement(cugo::PointToPlaneMatch<double>(n, 3.0, p));
    CHECK(planes.changeCount() == c0 + 1);
    (void)pe.getMeasurement();
    CHECK(planes.changeCount() == c0 + 2);
    (void)pe.measurementData();
    CHECK(planes.changeCount() == c0 + 2);
    const unsigned long long l0 = lines.changeCount();
    le.setInformation(2.0);
    CHECK(lines.changeCount() == l0 + 1);
    planes.removeEdge(&pe);
    CHECK(planes.nedges() == 0 && v0.getEdges().size() == 0);
    std::printf("OK\n");
    return 0;
}
"""


def test_icp_classes_have_the_reference_shape(tmp_path):
    src = tmp_path / "icp_api.cpp"
    src.write_text(API_PROGRAM)
    exe = tmp_path / "icp_api"
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
#define F(x) std::printf("%s %zu\n", #x, offsetof(cugo_icp_edges, x));
int main()
{
    F(n_poses_total) F(n_poses_free) F(n_plane) F(d_plane_pose) F(d_plane_pose_ptr) F(d_plane_p) F(d_plane_nd)
    F(d_plane_omega) F(n_plane_omega) F(d_plane_flags) F(rk_plane) F(delta_plane) F(n_line) F(d_line_pose)
    F(d_line_pose_ptr) F(d_line_p) F(d_line_au) F(d_line_omega) F(n_line_omega) F(d_line_flags) F(rk_line)
    F(delta_line)
    std::printf("sizeof %zu\n", sizeof(cugo_icp_edges));
    return 0;
}
"""


def fd_gradient(f, pose7, h=1e-6):
    g = np.zeros(6)
    for k in range(6):
        xi = np.zeros(6)
        xi[k] = h
        g[k] = (f(icp_ref.left_update(pose7, xi)) - f(icp_ref.left_update(pose7, -xi))) / (2 * h)
    return g


def test_icp_b_has_the_sign_of_the_ba_build_pass():
    """b of both kinds is minus half the gradient of chi2 under the left update, as the BA pass's bp is (its Jacobian
    is d(meas - proj), tests/golden/make_golden.py): the solver takes H dx = b and applies exp(+dx)."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden
    rng = np.random.default_rng(3)
    pose = icp_ref.random_pose(rng, rot=0.2, trans=0.5)
    # BA, restated by the golden generator
    Xw = np.array([0.4, -0.3, 6.0])
    meas = np.array([600.0, 180.0, 560.0])
    cam = np.array([718.856, 718.856, 607.1928, 185.2157, 386.1448])

    def ba_chi2(x):
        e = make_golden.edge(x, Xw, meas, True, cam)[0]
        return float(e @ e)
    e, _, JP, _ = make_golden.edge(pose, Xw, meas, True, cam)
    b_ba = JP.T @ e
    np.testing.assert_allclose(b_ba, -0.5 * fd_gradient(ba_chi2, pose), rtol=1e-6, atol=1e-6 * np.abs(b_ba).max())
    # ICP, one edge of each kind, weight 1, no robust kernel
    poses = pose[None, :]
    for kind in ("plane", "line"):
        ed = icp_ref.make_edges(rng, [0], kind, poses, noise=0.5)

        def chi2(x, ed=ed, kind=kind):
            return icp_ref.edge_terms(kind, ed, 0, x, 1.0, (0, 1.0))[0]
        _, _, b = icp_ref.edge_terms(kind, ed, 0, pose, 1.0, (0, 1.0))
        np.testing.assert_allclose(b, -0.5 * fd_gradient(chi2, pose), rtol=1e-6, atol=1e-7 * np.abs(b).max())


def test_ctypes_layout_of_icp_edges_matches_the_c_struct(tmp_path):
    src = tmp_path / "layout.cpp"
    src.write_text(LAYOUT_PROGRAM)
    exe = tmp_path / "layout"
    r = subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split("\n")
               if line)
    for name, _ in cugo.IcpEdges._fields_:
        assert int(out[name]) == getattr(cugo.IcpEdges, name).offset, name
    assert int(out["sizeof"]) == C.sizeof(cugo.IcpEdges)
