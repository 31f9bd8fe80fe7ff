"""SE(3) pose priors on the GPU: the kernel-level C ABI (cugo_prior_construct_quadratic_form,
cugo_prior_compute_errors) against the numpy restatement of tests/prior_ref.py.

Tolerances: per-pose H and b within 1e-12 of max|H| (resp. max|b|), chi2 within 1e-12 relative: the bound
tests/test_icp.py uses (the sums run in different orders)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import icp_ref
import prior_ref as PR

pytestmark = pytest.mark.gpu

cugo = importlib.import_module("cuda-bundle-adjustment_amd")

ANGLES = [0.0, 1e-9, 1e-5, 1e-3, 0.3, 1.0, 3.0]
RKS = [(0, 1.0), (1, 0.8), (2, 5.0), (3, 4.0)]  # (Tukey and Huber: edges on both sides of delta^2)


@pytest.fixture(scope="module")
def ctx():
    import devmem
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    c = devmem.Ctx()
    yield c
    c.close()


def make_case(seed, counts, rk=(0, 1.0), inactive_frac=0.0, per_edge_info=True, rot=0.3, trans=0.5, angles=None):
    """Poses with counts[k] priors on pose k, shuffled and then sorted by pose (stable).  angles: the residual angle
    of edge i is angles[i % len(angles)]"""
    rng = np.random.default_rng(seed)
    Pall = len(counts)
    poses = np.array([icp_ref.random_pose(rng) for _ in range(Pall)])
    pose = np.concatenate([np.full(c, k, np.int32) for k, c in enumerate(counts)] + [np.zeros(0, np.int32)])
    rng.shuffle(pose)
    E = len(pose)
    z = np.zeros((E, 7))
    for i, p in enumerate(pose):
        if angles is None:
            z[i] = PR.displaced(rng, poses[p], rot, trans)
        else:  # pose = Exp([theta a, v]) z  <=>  z = Exp(-[theta a, v]) pose to first order in v: the angle is exact
            axis = rng.normal(size=3)
            axis /= np.linalg.norm(axis)
            z[i] = icp_ref.left_update(poses[p], np.concatenate([-angles[i % len(angles)] * axis, rng.normal(0, trans, 3)]))
    info = np.array([PR.random_spd(rng, rng.uniform(0.5, 3.0)) for _ in range(E if per_edge_info else 1)]).reshape(-1, 6, 6)
    pr = PR.make_prior(pose, z, info, rk=rk, active=rng.random(E) >= inactive_frac)
    pr["flags"] = np.where(pr["active"], 0, cugo.EDGE_INACTIVE).astype(np.uint8)
    pr, _ = PR.sort_by_pose(pr)
    return poses, pr


def run_build(ctx, poses, n_free, pr, H0=None, b0=None):
    ev = PR.upload(ctx, len(poses), n_free, pr)
    d_poses = ctx.to_dev(poses)
    d_H = ctx.to_dev(np.zeros((n_free, 36)) if H0 is None else H0)
    d_b = ctx.to_dev(np.zeros((n_free, 6)) if b0 is None else b0)
    d_chi = ctx.empty(2)
    cugo.check(cugo.lib().cugo_prior_construct_quadratic_form(ctx.h, C.byref(ev), d_poses, d_H, d_b, d_chi))
    H = ctx.to_host(d_H, (n_free, 6, 6)).transpose(0, 2, 1)  # column-major blocks
    b = ctx.to_host(d_b, (n_free, 6))
    return H, b, ctx.to_host(d_chi, 1)[0], (ev, d_poses)


def run_errors(ctx, ev, d_poses, n):
    d_chi, d_edge = ctx.empty(2), ctx.empty(max(n, 1))
    cugo.check(cugo.lib().cugo_prior_compute_errors(ctx.h, C.byref(ev), d_poses, d_chi, d_edge))
    return ctx.to_host(d_chi, 1)[0], ctx.to_host(d_edge, max(n, 1))[:n]


def assert_close(got, want, rel=1e-12):
    scale = max(np.abs(want).max(), 1e-300)
    err = np.abs(got - want).max()
    print("err %.3g of scale %.3g" % (err, scale))
    assert err <= rel * scale, (err, scale)


def check(ctx, poses, n_free, pr):
    H, b, chi, keep = run_build(ctx, poses, n_free, pr)
    Hr, br, chir, ce = PR.reference_build(poses, n_free, pr)
    assert_close(H, Hr)
    assert_close(b, br)
    assert abs(chi - chir) <= 1e-12 * max(chir, 1e-300), (chi, chir)
    assert np.array_equal(H, H.transpose(0, 2, 1))
    return H, b, chi, ce, keep


def test_one_pose_with_one_prior(ctx):
    poses, pr = make_case(1, [1])
    H, b, chi, ce, (ev, d_poses) = check(ctx, poses, 1, pr)
    assert H[0].any() and chi > 0
    chi_e, edge = run_errors(ctx, ev, d_poses, 1)
    assert chi_e == chi and abs(edge[0] - ce[0]) <= 1e-12 * ce[0]


@pytest.mark.parametrize("rk", RKS)
def test_small_graph_with_fixed_poses_inactive_flags_and_every_robust_kernel(ctx, rk):
    """5 free + 2 fixed poses with 0, 1 and 3 priors per pose, priors on a fixed pose, inactive flags"""
    counts = [3, 0, 1, 3, 1, 2, 0]
    poses, pr = make_case(20 + rk[0], counts, rk=rk, inactive_frac=0.25)
    assert (~pr["active"]).any() and pr["active"].sum() >= 5
    H, b, chi, ce, _ = check(ctx, poses, 5, pr)
    assert not H[1].any() and not b[1].any()
    if rk[0] in (2, 3):  # kernels with a threshold: edges on both sides of it
        x = PR.reference_build(poses, 5, dict(pr, rk=(0, 1.0)))[3][pr["active"] & (pr["pose"] < 5)]
        assert (x > rk[1] ** 2).any() and (x < rk[1] ** 2).any()


def test_300_priors_on_70_free_poses_and_repeatable_bits(ctx):
    """uneven counts including zero: more than a wave and more than a workgroup of poses"""
    rng = np.random.default_rng(8)
    counts = rng.integers(0, 9, 75)
    counts[[3, 40, 69]] = 0
    counts[70:] = 2
    counts[10] += 300 - counts[:70].sum()
    assert counts[:70].sum() == 300 and counts.min() == 0
    poses, pr = make_case(9, list(counts), rk=(3, 1.5), inactive_frac=0.05)
    H, b, chi, ce, (ev, d_poses) = check(ctx, poses, 70, pr)
    H2, b2, chi2, _ = run_build(ctx, poses, 70, pr)
    assert np.array_equal(H, H2) and np.array_equal(b, b2) and chi == chi2
    # the error pass: the chi2 bits of the build pass, and the chi2 term of every edge
    E = len(pr["pose"])
    chi_e, edge = run_errors(ctx, ev, d_poses, E)
    assert chi_e == chi
    np.testing.assert_allclose(edge, ce, rtol=1e-12, atol=1e-12 * ce.max())
    assert not edge[pr["pose"] >= 70].any() and not edge[~pr["active"]].any()


def test_residual_angles_from_zero_to_three(ctx):
    poses, pr = make_case(13, [len(ANGLES)] * 3, angles=ANGLES, trans=1.0)
    r = np.array([PR.residual(poses[p], z) for p, z in zip(pr["pose"], pr["z"])])
    got = np.sort(np.linalg.norm(r[:, :3], axis=1))
    # (an angle read back from a rotation matrix carries an absolute error of a few ulps of 1)
    np.testing.assert_allclose(got, np.sort(np.tile(ANGLES, 3)), rtol=1e-9, atol=1e-15)
    check(ctx, poses, 3, pr)


def test_semi_definite_information_translation_only(ctx):
    poses, pr = make_case(14, [2, 1, 3], per_edge_info=False)
    pr["info"] = np.diag([0, 0, 0, 4.0, 2.0, 1.0])[None]
    H, b, chi, ce, _ = check(ctx, poses, 3, pr)
    # one matrix for all and one per edge give the same bits
    pr2 = dict(pr, info=np.tile(pr["info"], (len(pr["pose"]), 1, 1)))
    H2, b2, chi2, _ = run_build(ctx, poses, 3, pr2)
    assert np.array_equal(H, H2) and np.array_equal(b, b2) and chi == chi2


def test_build_adds_to_what_is_there_and_poses_without_priors_keep_their_bits(ctx):
    poses, pr = make_case(5, [2, 0, 3, 1], inactive_frac=0.3)
    pr["flags"][pr["pose"] == 3] = cugo.EDGE_INACTIVE  # pose 3: a prior that does not count
    pr["active"] = pr["flags"] == 0
    rng = np.random.default_rng(1)
    H0, b0 = rng.normal(size=(4, 36)), rng.normal(size=(4, 6))
    H, b, chi, _ = run_build(ctx, poses, 4, pr, H0, b0)
    Hr, br, chir, _ = PR.reference_build(poses, 4, pr)
    H0m = H0.reshape(4, 6, 6).transpose(0, 2, 1)
    assert_close(H, H0m + Hr)  # (pre-fill + terms)
    assert_close(b, b0 + br)
    assert abs(chi - chir) <= 1e-12 * chir
    for p in (1, 3):
        assert np.array_equal(H[p], H0m[p]) and np.array_equal(b[p], b0[p])
    # all edges inactive: nothing changes, chi2 = 0
    pr["flags"][:] = cugo.EDGE_INACTIVE
    H, b, chi, _ = run_build(ctx, poses, 4, pr, H0, b0)
    assert np.array_equal(H, H0m) and np.array_equal(b, b0) and chi == 0.0


def test_refused_layouts_write_nothing(ctx):
    poses, pr = make_case(3, [4, 2, 1])
    d_H, d_b = ctx.to_dev(np.zeros(36 * 3)), ctx.to_dev(np.zeros(6 * 3))
    d_poses = ctx.to_dev(poses)
    build = cugo.lib().cugo_prior_construct_quadratic_form
    # edges not sorted by pose are refused before anything runs
    bad = dict(pr, pose=pr["pose"][::-1].copy())
    ev = PR.upload(ctx, 3, 3, bad)
    ev.d_pose_ptr = ctx.to_dev(icp_ref.pose_ptr(pr["pose"], 3))
    assert build(ctx.h, C.byref(ev), d_poses, d_H, d_b, None) == -3
    # a pose_ptr that does not span the edges, one that does not ascend
    for ptr in ([0, 4, 6, 8], [0, 5, 4, 7]):
        ev = PR.upload(ctx, 3, 3, pr)
        ev.d_pose_ptr = ctx.to_dev(np.array(ptr, np.int32))
        assert build(ctx.h, C.byref(ev), d_poses, d_H, d_b, None) == -3
        assert cugo.lib().cugo_prior_compute_errors(ctx.h, C.byref(ev), d_poses, ctx.empty(2), None) == -3
    # a pose index out of range
    ev = PR.upload(ctx, 3, 3, pr)
    p = pr["pose"].copy()
    p[-1] = 3
    ev.d_pose = ctx.to_dev(p)
    assert build(ctx.h, C.byref(ev), d_poses, d_H, d_b, None) == -3
    # an unknown robust kernel code
    ev = PR.upload(ctx, 3, 3, pr)
    ev.rk = 7
    assert build(ctx.h, C.byref(ev), d_poses, d_H, d_b, None) == -3
    assert not ctx.to_host(d_H, 36 * 3).any() and not ctx.to_host(d_b, 6 * 3).any()
    # ... and the good layout is taken
    ev = PR.upload(ctx, 3, 3, pr)
    assert build(ctx.h, C.byref(ev), d_poses, d_H, d_b, None) == 0
    assert ctx.to_host(d_H, 36 * 3).any()


def test_the_step_of_the_kernels_system_goes_downhill_as_the_solver_applies_it(ctx):
    """Solve H dx = b with the kernel's own H and b and apply exp(+dx) on the left: chi2 must fall (an opposite sign of
    b, or a transposed Jacobian, would climb)"""
    poses, pr = make_case(41, [1], rot=0.1, trans=0.3)
    H, b, chi0, (ev, _) = run_build(ctx, poses, 1, pr)
    moved = poses.copy()
    moved[0] = icp_ref.left_update(poses[0], np.linalg.solve(H[0], b[0]))
    chi1, _ = run_errors(ctx, ev, ctx.to_dev(moved), 1)
    assert chi1 < 1e-2 * chi0, (chi0, chi1)
