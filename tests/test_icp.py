"""Point-to-plane / point-to-line pose edges on the GPU: the kernel-level C ABI (cugo_icp_construct_quadratic_form,
cugo_icp_compute_errors) against the numpy restatement of tests/icp_ref.py.

Tolerances: per-pose H, b and chi2 within 1e-12 relative to the block's scale (the sums run in different orders)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import icp_ref

pytestmark = pytest.mark.gpu

cugo = importlib.import_module("cuda-bundle-adjustment_amd")


@pytest.fixture(scope="module")
def ctx():
    import devmem
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    c = devmem.Ctx()
    yield c
    c.close()


def make_case(seed, counts, n_free, rk_plane=(0, 1.0), rk_line=(0, 1.0), inactive_frac=0.0, per_edge_omega=True,
              noise=0.05):
    """Poses with counts[k] = (plane edges, line edges) on pose k; poses >= n_free are fixed."""
    rng = np.random.default_rng(seed)
    Pall = len(counts)
    poses = np.array([icp_ref.random_pose(rng) for _ in range(Pall)])
    out = {}
    for j, (kind, rk) in enumerate((("plane", rk_plane), ("line", rk_line))):
        pose_of_edge = np.concatenate([np.full(c[j], k, np.int32) for k, c in enumerate(counts)])
        rng.shuffle(pose_of_edge)
        e, _ = icp_ref.sort_by_pose(icp_ref.make_edges(rng, pose_of_edge, kind, poses, noise=noise))
        E = len(pose_of_edge)
        e["omega"] = rng.uniform(0.5, 3.0, E) if per_edge_omega else np.array([1.7])
        e["flags"] = np.where(rng.random(E) >= inactive_frac, 0, cugo.EDGE_INACTIVE).astype(np.uint8)
        e["rk"] = rk
        out[kind] = e
    return poses, out


def reference(poses, n_free, case):
    kinds = []
    for kind in ("plane", "line"):
        e = case[kind]
        kinds.append((kind, e, e["omega"], e["flags"] == 0, e["rk"]))
    return icp_ref.reference_build(poses, n_free, kinds)


def run_build(ctx, poses, n_free, case, H0=None, b0=None):
    Pall = len(poses)
    ev = icp_ref.upload(ctx, Pall, n_free, plane=case["plane"], line=case["line"])
    d_poses = ctx.to_dev(poses)
    d_H = ctx.to_dev(np.zeros((n_free, 36)) if H0 is None else H0)
    d_b = ctx.to_dev(np.zeros((n_free, 6)) if b0 is None else b0)
    d_chi = ctx.empty(2)
    cugo.check(cugo.lib().cugo_icp_construct_quadratic_form(ctx.h, C.byref(ev), d_poses, d_H, d_b, d_chi))
    H = ctx.to_host(d_H, (n_free, 6, 6)).transpose(0, 2, 1)  # column-major blocks
    b = ctx.to_host(d_b, (n_free, 6))
    chi = ctx.to_host(d_chi, 1)[0]
    return H, b, chi, (ev, d_poses)


def assert_close(got, want, rel=1e-12):
    scale = max(np.abs(want).max(), 1e-300)
    err = np.abs(got - want).max()
    assert err <= rel * scale, (err, scale)


RKS = [(0, 1.0), (1, 0.3), (2, 0.5), (3, 0.2)]


@pytest.mark.parametrize("rk", RKS)
def test_build_matches_numpy_for_plane_and_line_edges(ctx, rk):
    counts = [(30, 20), (0, 15), (25, 0), (7, 9), (40, 33), (12, 5)]  # poses 4 and 5 are fixed
    poses, case = make_case(11 + rk[0], counts, 4, rk_plane=rk, rk_line=rk, inactive_frac=0.15, noise=0.3)
    H, b, chi, _ = run_build(ctx, poses, 4, case)
    Hr, br, chir, _ = reference(poses, 4, case)
    for p in range(4):
        assert_close(H[p], Hr[p])
        assert_close(b[p], br[p])
    assert abs(chi - chir) <= 1e-12 * chir
    assert np.array_equal(H, H.transpose(0, 2, 1))


def test_build_adds_to_what_is_there_and_fixed_or_inactive_edges_count_for_nothing(ctx):
    counts = [(50, 40), (30, 30), (20, 10)]
    poses, case = make_case(5, counts, 2, inactive_frac=0.3, per_edge_omega=False)
    rng = np.random.default_rng(1)
    H0, b0 = rng.normal(size=(2, 36)), rng.normal(size=(2, 6))
    H, b, chi, _ = run_build(ctx, poses, 2, case, H0, b0)
    Hr, br, chir, _ = reference(poses, 2, case)
    assert_close(H - H0.reshape(2, 6, 6).transpose(0, 2, 1), Hr)
    assert_close(b - b0, br)
    assert abs(chi - chir) <= 1e-12 * chir
    # all edges inactive: nothing changes, chi2 = 0
    for kind in ("plane", "line"):
        case[kind]["flags"][:] = cugo.EDGE_INACTIVE
    H, b, chi, _ = run_build(ctx, poses, 2, case, H0, b0)
    assert np.array_equal(H, H0.reshape(2, 6, 6).transpose(0, 2, 1)) and np.array_equal(b, b0) and chi == 0.0


def test_chunking_with_one_pose_of_1e5_edges_and_repeatable_bits(ctx):
    counts = [(3, 3)] * 40 + [(100000, 3000)] + [(3, 3)] * 40 + [(2, 1)] * 5
    poses, case = make_case(21, counts, 81, rk_plane=(1, 0.2), rk_line=(3, 0.1), inactive_frac=0.05)
    H, b, chi, (ev, d_poses) = run_build(ctx, poses, 81, case)
    Hr, br, chir, per_edge = reference(poses, 81, case)
    for p in range(81):
        assert_close(H[p], Hr[p])
        assert_close(b[p], br[p])
    assert abs(chi - chir) <= 1e-12 * chir
    H2, b2, chi2, _ = run_build(ctx, poses, 81, case)
    assert np.array_equal(H, H2) and np.array_equal(b, b2) and chi == chi2
    # the error pass: the same chi2 bits, and the chi2 term of every edge
    E = len(case["plane"]["pose"]) + len(case["line"]["pose"])
    d_chi, d_edge = ctx.empty(2), ctx.empty(E)
    cugo.check(cugo.lib().cugo_icp_compute_errors(ctx.h, C.byref(ev), d_poses, d_chi, d_edge))
    assert ctx.to_host(d_chi, 1)[0] == chi
    ce = ctx.to_host(d_edge, E)
    want = np.concatenate(per_edge)
    # (small residuals are differences of coordinates of size 10: their relative error grows by that ratio)
    np.testing.assert_allclose(ce, want, rtol=1e-12, atol=1e-12 * want.max())


def test_empty_kinds_and_refused_layouts(ctx):
    counts = [(10, 0), (5, 0), (0, 0)]
    poses, case = make_case(3, counts, 3)
    H, b, chi, _ = run_build(ctx, poses, 3, {"plane": case["plane"], "line": None})
    Hr, br, chir, _ = reference(poses, 3, case)
    assert_close(H, Hr)
    assert_close(b, br)
    assert not H[2].any() and abs(chi - chir) <= 1e-12 * chir
    # edges not sorted by pose are refused before anything runs
    e = dict(case["plane"])
    e["pose"] = e["pose"][::-1].copy()
    ev = icp_ref.upload(ctx, 3, 3, plane=e)
    ev.d_plane_pose_ptr = ctx.to_dev(icp_ref.pose_ptr(case["plane"]["pose"], 3))
    d_H, d_b = ctx.empty(36 * 3), ctx.empty(6 * 3)
    assert cugo.lib().cugo_icp_construct_quadratic_form(ctx.h, C.byref(ev), ctx.to_dev(poses), d_H, d_b,
                                                         None) == -3
    # a pose_ptr that does not span the edges
    ev = icp_ref.upload(ctx, 3, 3, plane=case["plane"])
    ev.d_plane_pose_ptr = ctx.to_dev(np.array([0, 10, 12, 14], np.int32))
    assert cugo.lib().cugo_icp_compute_errors(ctx.h, C.byref(ev), ctx.to_dev(poses), ctx.empty(2), None) == -3
    assert not ctx.to_host(d_H, 36 * 3).any()


@pytest.mark.parametrize("kind", ["plane", "line"])
def test_the_step_of_the_kernels_system_goes_downhill_as_the_solver_applies_it(ctx, kind):
    """Solve H dx = b with the kernel's own H and b and apply exp(+dx) on the left, as cugo_backsubst_update does
    with the BA system: chi2 must fall to the noise floor (an opposite sign of b would climb)."""
    rng = np.random.default_rng(31 if kind == "plane" else 32)
    counts = [(60, 0), (5, 0)] if kind == "plane" else [(0, 60), (0, 5)]
    poses, case = make_case(41 if kind == "plane" else 42, counts, 1, noise=1e-4)
    if kind == "plane":
        case["line"] = None
    else:
        case["plane"] = None
    start = poses.copy()
    start[0] = icp_ref.left_update(poses[0], np.concatenate([rng.normal(0, 0.02, 3), rng.normal(0, 0.05, 3)]))
    H, b, chi0, (ev, _) = run_build(ctx, start, 1, case)
    dx = np.linalg.solve(H[0], b[0])
    moved = start.copy()
    moved[0] = icp_ref.left_update(start[0], dx)
    d_chi = ctx.empty(2)
    cugo.check(cugo.lib().cugo_icp_compute_errors(ctx.h, C.byref(ev), ctx.to_dev(moved), d_chi, None))
    chi1 = ctx.to_host(d_chi, 1)[0]
    assert chi1 < 1e-2 * chi0, (chi0, chi1)
