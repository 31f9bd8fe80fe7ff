"""Relative-pose SE(3) edges on the GPU: the kernel-level C ABI (cugo_relpose_construct_quadratic_form[_schur],
cugo_relpose_compute_errors over a cugo_relpose_plan) against the numpy restatement of tests/relpose_ref.py.

Tolerances, those of tests/test_prior.py: blocks and b within 1e-12 of the reference's max|.|, chi2 within 1e-12
relative (the sums run in different orders; the inputs have |t| = O(1))."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import icp_ref
import prior_ref as PR
import relpose_ref as RR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def random_poses(seed, n):
    rng = np.random.default_rng(seed)
    return rng, np.array([icp_ref.random_pose(rng) for _ in range(n)])


def full_pattern(P):
    """every block of the upper triangle: more blocks than a pose graph maps to"""
    rowptr = np.concatenate([[0], np.cumsum(np.arange(P, 0, -1))]).astype(np.int32)
    return rowptr, np.concatenate([np.arange(p, P) for p in range(P)] + [np.zeros(0, int)]).astype(np.int32)


def blocks(a, n):
    """[n][36] column-major blocks -> [n, 6, 6]"""
    return a.reshape(n, 6, 6).transpose(0, 2, 1)


def run_build(ctx, poses, n_free, rp, rowptr, colind, H0=None, b0=None, Hoff0=None, flags=None):
    ev, pl = RR.upload(ctx, len(poses), n_free, rp, rowptr, colind, flags)
    nnzb = len(colind)
    d_poses = ctx.to_dev(poses)
    d_H = ctx.to_dev(np.zeros((n_free, 36)) if H0 is None else H0)
    d_b = ctx.to_dev(np.zeros((n_free, 6)) if b0 is None else b0)
    d_Hoff = ctx.to_dev(np.zeros((nnzb, 36)) if Hoff0 is None else Hoff0)
    d_chi = ctx.empty(2)
    cugo.relpose_construct_quadratic_form(ctx.h, ev, d_poses, d_H, d_b, d_Hoff, d_chi)
    out = (blocks(ctx.to_host(d_H, (n_free, 36)), n_free), ctx.to_host(d_b, (n_free, 6)),
           blocks(ctx.to_host(d_Hoff, (nnzb, 36)), nnzb), ctx.to_host(d_chi, 1)[0])
    return out + ((ev, pl, d_poses),)


def run_schur(ctx, poses, n_free, rp, rowptr, colind, Hsc0=None, bp0=None, bsc0=None):
    ev, pl = RR.upload(ctx, len(poses), n_free, rp, rowptr, colind)
    nnzb = len(colind)
    d_Hsc = ctx.to_dev(np.zeros((nnzb, 36)) if Hsc0 is None else Hsc0)
    d_bp = ctx.to_dev(np.zeros((n_free, 6)) if bp0 is None else bp0)
    d_bsc = ctx.to_dev(np.zeros((n_free, 6)) if bsc0 is None else bsc0)
    d_chi = ctx.empty(2)
    cugo.relpose_construct_quadratic_form_schur(ctx.h, ev, ctx.to_dev(poses), ctx.to_dev(rowptr), d_Hsc, d_bp, d_bsc, d_chi)
    out = (blocks(ctx.to_host(d_Hsc, (nnzb, 36)), nnzb), ctx.to_host(d_bp, (n_free, 6)), ctx.to_host(d_bsc, (n_free, 6)),
           ctx.to_host(d_chi, 1)[0])
    pl.close()
    return out


def run_errors(ctx, ev, d_poses, n):
    d_chi, d_edge = ctx.empty(2), ctx.to_dev(np.full(max(n, 1), -7.0))
    cugo.relpose_compute_errors(ctx.h, ev, d_poses, d_chi, d_edge)
    return ctx.to_host(d_chi, 1)[0], ctx.to_host(d_edge, max(n, 1))[:n]


def assert_close(got, want, rel=1e-12, what=""):
    scale = max(np.abs(want).max(), 1e-300)
    err = np.abs(got - want).max()
    print("%s err %.3g of scale %.3g" % (what, err, scale))
    assert err <= rel * scale, (what, err, scale)


def check(ctx, poses, n_free, rp, rowptr=None, colind=None):
    """the build pass against the reference; then the error pass: the bits of the build's chi2, the term of every edge"""
    if rowptr is None:
        rowptr, colind = RR.pattern(rp, n_free)
    H, b, Hoff, chi, (ev, pl, d_poses) = run_build(ctx, poses, n_free, rp, rowptr, colind)
    Hr, br, Hoffr, chir, ce = RR.reference_build(poses, n_free, rp, rowptr, colind)
    assert_close(H, Hr, what="H")
    assert_close(b, br, what="b")
    if Hoffr.any():
        assert_close(Hoff, Hoffr, what="Hoff")
    for k in range(len(colind)):  # (the blocks nothing maps to, the diagonal ones among them)
        assert Hoffr[k].any() or not Hoff[k].any(), k
    print("chi2 %.17g ref %.17g" % (chi, chir))
    assert abs(chi - chir) <= 1e-12 * max(chir, 1e-300), (chi, chir)
    assert np.array_equal(H, H.transpose(0, 2, 1))
    E = len(rp["a"])
    chi_e, edge = run_errors(ctx, ev, d_poses, E)
    assert chi_e == chi
    np.testing.assert_allclose(edge, ce, rtol=1e-12, atol=0)
    pl.close()
    return H, b, Hoff, chi, ce


# ---- the smallest graphs --------------------------------------------------------------------------------------
def test_one_free_free_edge(ctx):
    rng, poses = random_poses(1, 2)
    for pair in ((0, 1), (1, 0)):
        rp = RR.random_edges(rng, poses, [pair], rot=0.3, trans=0.5)
        H, b, Hoff, chi, ce = check(ctx, poses, 2, rp)
        assert H[0].any() and H[1].any() and Hoff[1].any() and not Hoff[0].any() and not Hoff[2].any() and chi > 0


@pytest.mark.parametrize("pair", [(0, 1), (1, 0)])
def test_one_free_fixed_edge_from_either_side(ctx, pair):
    rng, poses = random_poses(2, 2)
    rp = RR.random_edges(rng, poses, [pair], rot=0.3, trans=0.5)
    H, b, Hoff, chi, ce = check(ctx, poses, 1, rp)
    assert H[0].any() and b[0].any() and chi > 0 and ce[0] == pytest.approx(chi, rel=1e-12)


def test_one_fixed_fixed_edge_leaves_everything_untouched(ctx):
    rng, poses = random_poses(3, 3)
    rp = RR.random_edges(rng, poses, [(1, 2)])
    rowptr, colind = RR.pattern(rp, 1)
    H0, b0, Hoff0 = rng.normal(size=(1, 36)), rng.normal(size=(1, 6)), rng.normal(size=(1, 36))
    H, b, Hoff, chi, (ev, pl, d_poses) = run_build(ctx, poses, 1, rp, rowptr, colind, H0, b0, Hoff0)
    assert np.array_equal(H, blocks(H0, 1)) and np.array_equal(b, b0) and np.array_equal(Hoff, blocks(Hoff0, 1))
    assert chi == 0.0
    chi_e, edge = run_errors(ctx, ev, d_poses, 1)
    assert chi_e == 0.0 and edge[0] == 0.0
    pl.close()


def test_three_edges_on_one_pair_in_mixed_orientation(ctx):
    rng, poses = random_poses(4, 3)
    rp = RR.random_edges(rng, poses, [(0, 2), (2, 0), (0, 2)], rot=0.2, trans=0.4)
    H, b, Hoff, chi, ce = check(ctx, poses, 3, rp)
    assert not H[1].any() and list(RR.pattern(rp, 3)[1]) == [0, 2, 1, 2]
    # the block is the sum of the three, the middle one transposed into place
    one = [RR.edge_terms(poses[a], poses[b], z, Om, (0, 1.0))[3] for a, b, z, Om in zip(rp["a"], rp["b"], rp["z"], rp["info"])]
    assert_close(Hoff[1], one[0] + one[1].T + one[2], what="sum")


# ---- walks of every length, workgroup edges ---------------------------------------------------------------------
def test_poses_with_0_1_63_64_65_and_300_incident_edges(ctx):
    degrees = [0, 1, 63, 64, 65, 300]
    rng, poses = random_poses(5, 6 + 20)
    n_free = 6 + 16  # hubs 0..5, partners 6..21 free, 22..25 fixed
    pairs = []
    for hub, deg in enumerate(degrees):
        for k in range(deg):
            partner = 6 + (k * 7 + hub) % 20
            pairs.append((hub, partner) if rng.random() < 0.5 else (partner, hub))
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    rp = RR.random_edges(rng, poses, pairs, rk=(3, 1.5))
    inc_ptr = RR.plan(rp, n_free, *RR.pattern(rp, n_free))[0]
    assert list(np.diff(inc_ptr)[:6]) == degrees
    H, b, Hoff, chi, ce = check(ctx, poses, n_free, rp)
    assert not H[0].any() and not b[0].any()


@pytest.mark.parametrize("n_free", [3, 4, 5, 7, 8, 9, 70])
def test_free_pose_counts_round_a_workgroup_with_fixed_poses_and_repeatable_bits(ctx, n_free):
    """a workgroup holds four poses (RELPOSE_POSES, one wave each): 3, 4, 5 and 7, 8, 9 free poses stand round one and two
    workgroups, 70 leaves the last one half empty"""
    # (seed 14 draws no edge between two free poses for n_free = 4, which the pattern assertion below asks for)
    rng, poses = random_poses(114 if n_free == 4 else 10 + n_free, n_free + 3)
    Pall = n_free + 3
    E = 3 * n_free
    a = rng.integers(0, Pall, E)
    b = (a + rng.integers(1, Pall, E)) % Pall
    rp = RR.random_edges(rng, poses, np.stack([a, b], 1), rk=(1, 2.0), inactive_frac=0.1)
    rowptr, colind = RR.pattern(rp, n_free)
    assert (np.diff(rowptr) > 1).any() and rowptr[n_free - 1] != n_free - 1
    H, b_, Hoff, chi, ce = check(ctx, poses, n_free, rp, rowptr, colind)
    H2, b2, Hoff2, chi2, keep = run_build(ctx, poses, n_free, rp, rowptr, colind)
    keep[1].close()
    assert np.array_equal(H, H2) and np.array_equal(b_, b2) and np.array_equal(Hoff, Hoff2) and chi == chi2
    # the Schur form: the same bits through rowptr (rowptr[p] != p), bsc = bp
    Hsc, bp, bsc, chis = run_schur(ctx, poses, n_free, rp, rowptr, colind)
    diag = rowptr[:-1]
    assert np.array_equal(Hsc[diag], H) and np.array_equal(bp, b_) and np.array_equal(bsc, b_) and chis == chi
    off = np.ones(len(colind), bool)
    off[diag] = False
    assert np.array_equal(Hsc[off], Hoff[off])


# ---- flags, kernels, angles, information ------------------------------------------------------------------------
def designed(seed=6, rk=(0, 1.0), inactive=(2, 9), **kw):
    """5 free + 2 fixed poses (tests/test_relpose_host.py designed_graph): duplicates in both orientations, fixed ends
    on either side, a fixed-fixed edge, inactive edges, pose 4 without any edge"""
    a = [0, 1, 1, 3, 5, 2, 6, 5, 0, 3, 2]
    b = [1, 0, 0, 2, 0, 6, 3, 6, 3, 1, 3]
    rng, poses = random_poses(seed, 7)
    rp = RR.random_edges(rng, poses, list(zip(a, b)), rk=rk, **kw)
    rp["active"][:] = True
    rp["active"][list(inactive)] = False
    return rng, poses, rp


def test_inactive_flags_in_the_plan_and_at_run_time(ctx):
    rng, poses, rp = designed()
    H, b, Hoff, chi, ce = check(ctx, poses, 5, rp)
    assert ce[2] == 0 and ce[9] == 0 and ce[7] == 0 and (ce[[0, 1, 3, 4, 5, 6, 8, 10]] > 0).all()
    # the plan sees every edge active (so the pattern needs the pair (1, 3)); the flags reach the kernel alone
    rowptr, colind = RR.pattern(dict(rp, active=np.ones(11, bool)), 5)
    H2, b2, Hoff2, chi2, (ev, pl, d_poses) = run_build(ctx, poses, 5, rp, rowptr, colind, flags=RR.flags_of(rp))
    Hr, br, Hoffr, chir, _ = RR.reference_build(poses, 5, rp, rowptr, colind)
    assert_close(H2, Hr), assert_close(b2, br), assert_close(Hoff2, Hoffr)
    assert abs(chi2 - chir) <= 1e-12 * chir
    k13 = RR.block_of(rowptr, colind, 1, 3)
    assert not Hoff2[k13].any()
    chi_e, edge = run_errors(ctx, ev, d_poses, 11)
    assert chi_e == chi2 and edge[2] == 0 and edge[9] == 0
    pl.close()
    # all edges of pose 1 inactive at run time: its blocks keep their bits
    fl = RR.flags_of(rp)
    fl[[0, 1, 2, 9]] = cugo.EDGE_INACTIVE
    H0, b0 = rng.normal(size=(5, 36)), rng.normal(size=(5, 6))
    H3, b3, _, _, keep = run_build(ctx, poses, 5, rp, rowptr, colind, H0, b0, flags=fl)
    keep[1].close()
    for p in (1, 4):
        assert np.array_equal(H3[p], blocks(H0, 5)[p]) and np.array_equal(b3[p], b0[p])


@pytest.mark.parametrize("rk", RKS)
def test_every_robust_kernel(ctx, rk):
    rng, poses, rp = designed(seed=20 + rk[0], rk=rk, rot=0.3, trans=0.5)
    check(ctx, poses, 5, rp)
    if rk[0] in (2, 3):  # kernels with a threshold: edges on both sides of it
        x = RR.reference_build(poses, 5, dict(rp, rk=(0, 1.0)))[4][RR.counting(rp, 5)]
        assert (x > rk[1] ** 2).any() and (x < rk[1] ** 2).any()


def test_residual_angles_from_zero_to_three(ctx):
    rng, poses = random_poses(13, 5)
    pairs = [(i % 4, (i % 4 + 1 + (i // 4) % 4) % 5) for i in range(3 * len(ANGLES))]  # (never a == b; 4 is fixed)
    rp = RR.random_edges(rng, poses, pairs, trans=1.0, angles=ANGLES)
    r = np.array([RR.residual(poses[a], poses[b], z) for a, b, z in zip(rp["a"], rp["b"], rp["z"])])
    got = np.sort(np.linalg.norm(r[:, :3], axis=1))
    # (an angle read back from a rotation matrix carries an absolute error of a few ulps of 1)
    np.testing.assert_allclose(got, np.sort(np.tile(ANGLES, 3)), rtol=1e-9, atol=1e-15)
    check(ctx, poses, 4, rp)


def test_one_shared_information_matrix_and_a_singular_one(ctx):
    rng, poses, rp = designed(seed=14, per_edge_info=False)
    assert rp["info"].shape == (1, 6, 6)
    H, b, Hoff, chi, ce = check(ctx, poses, 5, rp)
    # one matrix for all and one per edge give the same bits
    rowptr, colind = RR.pattern(rp, 5)
    rp2 = dict(rp, info=np.tile(rp["info"], (11, 1, 1)))
    H2, b2, Hoff2, chi2, keep = run_build(ctx, poses, 5, rp2, rowptr, colind)
    keep[1].close()
    assert np.array_equal(H, H2) and np.array_equal(b, b2) and np.array_equal(Hoff, Hoff2) and chi == chi2
    # translation only
    rp["info"] = np.diag([0, 0, 0, 4.0, 2.0, 1.0])[None]
    H, b, Hoff, chi, ce = check(ctx, poses, 5, rp)
    assert chi > 0 and np.linalg.matrix_rank(H[3]) <= 6


@pytest.mark.parametrize("rk", RKS)
def test_an_edge_to_the_fixed_identity_is_the_prior_term_for_term(ctx, rk):
    """relpose_types.h: "With T_b the fixed identity this is the pose prior, term for term."  5 free poses and a fixed
    pose at the identity; the same measurements (every angle of ANGLES on every pose) and per-edge Omegas once as priors
    and once as relative-pose edges a = the free pose, b = the fixed one.  The two kernels share the residual and J_l^-1
    (ba_math.h), R_a I^T and t_a - R_A 0 are exact up to the sign of a zero and the products sum in the same order, so
    H, b, chi2 and the per-edge chi2 of the two entry points are the same bits (measured before it was asserted: see
    profiles/se3_edges_refactor_ab.txt)."""
    rng = np.random.default_rng(40 + rk[0])
    poses = np.array([icp_ref.random_pose(rng) for _ in range(5)] + [[0, 0, 0, 1.0, 0, 0, 0]])
    E = 5 * len(ANGLES)
    pose = np.repeat(np.arange(5, dtype=np.int32), len(ANGLES))  # (sorted by pose: the walks of both kernels are this order)
    z = np.zeros((E, 7))
    for i, p in enumerate(pose):  # as tests/test_prior.py make_case: the residual angle is exact
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        z[i] = icp_ref.left_update(poses[p], np.concatenate([-ANGLES[i % len(ANGLES)] * axis, rng.normal(0, 0.5, 3)]))
    info = np.array([PR.random_spd(rng, rng.uniform(0.5, 3.0)) for _ in range(E)])
    pr = PR.make_prior(pose, z, info, rk=rk)
    rp = RR.make_edges(pose, np.full(E, 5), z, info, rk=rk)
    # the priors
    evp = PR.upload(ctx, 6, 5, pr)
    d_poses = ctx.to_dev(poses)
    d_H, d_b, d_chi, d_edge = ctx.to_dev(np.zeros((5, 36))), ctx.to_dev(np.zeros((5, 6))), ctx.empty(2), ctx.empty(E)
    cugo.check(cugo.lib().cugo_prior_construct_quadratic_form(ctx.h, C.byref(evp), d_poses, d_H, d_b, d_chi))
    Hp, bp, chip = blocks(ctx.to_host(d_H, (5, 36)), 5), ctx.to_host(d_b, (5, 6)), ctx.to_host(d_chi, 1)[0]
    cugo.check(cugo.lib().cugo_prior_compute_errors(ctx.h, C.byref(evp), d_poses, d_chi, d_edge))
    chip_e, edgep = ctx.to_host(d_chi, 1)[0], ctx.to_host(d_edge, E)
    # the relative-pose edges
    rowptr, colind = RR.pattern(rp, 5)
    assert len(colind) == 5  # no pair of free poses
    H, b, Hoff, chi, (ev, pl, d_poses2) = run_build(ctx, poses, 5, rp, rowptr, colind)
    chi_e, edge = run_errors(ctx, ev, d_poses2, E)
    pl.close()
    assert Hp.any() and bp.any() and chip > 0 and (edgep > 0).all() and not Hoff.any()
    for what, got, want in (("H", H, Hp), ("b", b, bp), ("chi2", chi, chip), ("chi2 (error pass)", chi_e, chip_e),
                            ("edge chi2", edge, edgep)):
        got, want = np.asarray(got), np.asarray(want)
        print("%s: max |relpose - prior| %.3g of scale %.3g" % (what, np.abs(got - want).max(), np.abs(want).max()))
    assert np.array_equal(H, Hp) and np.array_equal(b, bp) and chi == chip
    assert chi_e == chip_e and np.array_equal(edge, edgep)


def test_terms_are_added_and_unreferenced_blocks_keep_their_canaries(ctx):
    rng, poses, rp = designed(seed=15)
    rowptr, colind = full_pattern(5)
    nnzb = len(colind)
    H0, b0, Hoff0 = rng.normal(size=(5, 36)), rng.normal(size=(5, 6)), rng.normal(size=(nnzb, 36))
    H, b, Hoff, chi, keep = run_build(ctx, poses, 5, rp, rowptr, colind, H0, b0, Hoff0)
    keep[1].close()
    Hr, br, Hoffr, chir, _ = RR.reference_build(poses, 5, rp, rowptr, colind)
    assert_close(H, blocks(H0, 5) + Hr, what="H")
    assert_close(b, b0 + br, what="b")
    assert_close(Hoff, blocks(Hoff0, nnzb) + Hoffr, what="Hoff")
    mapped = np.array([Hoffr[k].any() for k in range(nnzb)])
    assert mapped.sum() == 3 and not mapped[rowptr[:-1]].any()
    assert np.array_equal(Hoff[~mapped], blocks(Hoff0, nnzb)[~mapped])
    assert np.array_equal(H[4], blocks(H0, 5)[4]) and np.array_equal(b[4], b0[4])
    # the Schur form on the same pattern: Hsc holds both kinds of block, bp and bsc start differently and get one term
    Hsc0, bsc0 = rng.normal(size=(nnzb, 36)), rng.normal(size=(5, 6))
    Hsc, bp, bsc, chis = run_schur(ctx, poses, 5, rp, rowptr, colind, Hsc0, b0, bsc0)
    want = blocks(Hsc0, nnzb) + Hoffr
    want[rowptr[:-1]] += Hr
    assert_close(Hsc, want, what="Hsc")
    touched = mapped.copy()
    touched[rowptr[[0, 1, 2, 3]]] = True
    assert np.array_equal(Hsc[~touched], blocks(Hsc0, nnzb)[~touched])
    assert np.array_equal(bp, b) and chis == chi
    assert_close(bsc, bsc0 + br, what="bsc")
    assert np.array_equal(bsc[4], bsc0[4])


def test_refused_arguments_write_nothing(ctx):
    rng, poses, rp = designed(seed=16)
    rowptr, colind = RR.pattern(rp, 5)
    ev, pl = RR.upload(ctx, 7, 5, rp, rowptr, colind)
    d_poses = ctx.to_dev(poses)
    d_H, d_b, d_Hoff = ctx.to_dev(np.zeros(36 * 5)), ctx.to_dev(np.zeros(6 * 5)), ctx.to_dev(np.zeros(36 * len(colind)))
    build = cugo.lib().cugo_relpose_construct_quadratic_form

    def rc(**kw):
        e2 = cugo.RelPoseEdges.from_buffer_copy(ev)
        for k, v in kw.items():
            setattr(e2, k, v)
        return build(ctx.h, C.byref(e2), d_poses, d_H, d_b, d_Hoff, None)

    assert rc(n=10) == -3 and rc(n_poses_free=4) == -3 and rc(n_poses_total=8) == -3  # not the plan's counts
    assert rc(rk=7) == -3 and rc(rk=3, delta=0.0) == -3 and rc(n_info=2) == -3 and rc(d_meas=None) == -3
    assert rc(plan=None) == -3
    host_only = cugo.RelPosePlan(None, 7, 5, rp["a"], rp["b"], RR.flags_of(rp), rowptr, colind)
    assert rc(plan=host_only.handle) == -3 and "host-only" in cugo.lib().cugo_last_error().decode()
    host_only.close()
    assert build(ctx.h, C.byref(ev), d_poses, d_H, d_b, None, None) == -3  # an edge joins two free poses: Hoff is needed
    assert not ctx.to_host(d_H, 36 * 5).any() and not ctx.to_host(d_b, 6 * 5).any()
    assert rc() == 0 and ctx.to_host(d_H, 36 * 5).any()
    pl.close()


@pytest.mark.parametrize("mode", ["2"])
def test_poisoned_allocations_change_nothing(mode):
    """CUGO_POISON_ALLOC (hip_util.h) in a fresh child process: nothing reads memory nobody wrote (workgroup totals,
    the plan's arrays), nothing is stored past a buffer's end"""
    env = dict(os.environ, CUGO_POISON_ALLOC=mode)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p",
                        "no:cacheprovider", "-k", "inactive_flags or canaries or three_edges or (round_a_workgroup and 9)"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "guard zone" not in r.stderr and " passed" in r.stdout


# ---- end to end -------------------------------------------------------------------------------------------------
def lm_loop(poses0, n_free, rp, rowptr, colind, system, solve, iters=6):
    """Levenberg-Marquardt over the pose graph: system(poses) -> whatever solve(system, lambda) -> dx [P, 6] needs and
    chi2; the step is applied with left_update in numpy; returns chi2 per iteration (after it) and the poses"""
    poses = poses0.copy()
    lam, chis = 1e-4, []
    sys_, chi = system(poses)
    for _ in range(iters):
        for _trial in range(10):
            dx = solve(sys_, lam)
            trial = poses.copy()
            for p in range(n_free):
                trial[p] = icp_ref.left_update(poses[p], dx[p])
            sys_t, chi_t = system(trial)
            if chi_t < chi:
                poses, sys_, chi, lam = trial, sys_t, chi_t, lam / 3
                break
            lam *= 5
        chis.append(chi)
    return chis, poses


def test_ring_with_chords_through_the_sparse_cholesky_matches_a_dense_solve_and_reaches_the_ground_truth(ctx):
    gt, start, rp = RR.ring_case()
    P = len(gt) - 1
    rowptr, colind = cugo.relpose_pattern(P, rp["a"], rp["b"])
    rp_, ci_ = RR.pattern(rp, P)
    assert np.array_equal(rowptr, rp_) and np.array_equal(colind, ci_) and len(colind) > 2 * P
    nnzb = len(colind)

    # the reference loop: numpy build, dense solve.  Twice, for what the reference differs by from itself: the edges in
    # another order, and the unknowns of the dense solve in another order
    def dense(rp_k, order):
        def system(poses):
            H, b, Hoff, chi, _ = RR.reference_build(poses, P, rp_k, rowptr, colind)
            return RR.dense_system(H, b, Hoff, rowptr, colind), chi

        def solve(s, lam):
            A = s[0] + lam * np.eye(6 * P)
            x = np.zeros(6 * P)
            x[order] = np.linalg.solve(A[np.ix_(order, order)], s[1][order])
            return x.reshape(P, 6)
        return lm_loop(start, P, rp_k, rowptr, colind, system, solve)
    chis_ref, poses_ref = dense(rp, np.arange(6 * P))
    sens = [0.0] * len(chis_ref)
    for seed in (3, 4, 5):
        r = np.random.default_rng(seed)
        perm = r.permutation(len(rp["a"]))
        chis_perm, _ = dense(dict(rp, **{k: rp[k][perm] for k in ("a", "b", "z", "info", "active")}), r.permutation(6 * P))
        sens = [max(s, abs(x - y) / abs(x)) for s, x, y in zip(sens, chis_ref, chis_perm)]
    print("self-sensitivity of the reference per iteration:", ["%.2g" % s for s in sens])
    tol = [max(1e-10, 4.0 * s) for s in sens]  # (the rule of tests/test_icp_graph.py against its dense LM)

    # the product loop: Schur-form build -> cugo_chol_analyze / cugo_chol_factor_solve on the pattern
    ev, pl = RR.upload(ctx, P + 1, P, rp, rowptr, colind)
    L = cugo.lib()
    chol = C.c_void_p()
    cugo.check(L.cugo_chol_create(ctx.h, C.byref(chol)))
    cugo.check(L.cugo_chol_analyze(chol, P, rowptr.ctypes.data_as(C.POINTER(C.c_int32)),
                                   colind.ctypes.data_as(C.POINTER(C.c_int32))))
    d_rowptr = ctx.to_dev(rowptr)
    d_Hsc, d_bp, d_bsc = ctx.empty(36 * nnzb), ctx.empty(6 * P), ctx.empty(6 * P)
    d_x, d_fail, d_chi, d_poses = ctx.empty(6 * P), ctx.empty(2, np.int32), ctx.empty(2), ctx.empty(7 * (P + 1))

    def system(poses):
        cugo.check(L.cugo_memcpy_h2d(ctx.h, d_poses, poses.ctypes.data_as(C.c_void_p), poses.nbytes))
        for d, n in ((d_Hsc, 36 * nnzb), (d_bp, 6 * P), (d_bsc, 6 * P)):
            cugo.check(L.cugo_memset(ctx.h, d, 0, 8 * n))
        cugo.relpose_construct_quadratic_form_schur(ctx.h, ev, d_poses, d_rowptr, d_Hsc, d_bp, d_bsc, d_chi)
        return (ctx.to_host(d_Hsc, (nnzb, 36)), ctx.to_host(d_bsc, 6 * P)), ctx.to_host(d_chi, 1)[0]

    def solve(s, lam):
        cugo.check(L.cugo_memcpy_h2d(ctx.h, d_Hsc, s[0].ctypes.data_as(C.c_void_p), s[0].nbytes))
        cugo.check(L.cugo_memcpy_h2d(ctx.h, d_bsc, s[1].ctypes.data_as(C.c_void_p), s[1].nbytes))
        cugo.check(L.cugo_chol_factor_solve(chol, d_Hsc, C.c_double(lam), d_bsc, d_x, d_fail))
        assert ctx.to_host(d_fail, 1, np.int32)[0] == 0
        return ctx.to_host(d_x, (P, 6))
    chis, poses = lm_loop(start, P, rp, rowptr, colind, system, solve)
    L.cugo_chol_destroy(chol)
    pl.close()
    for i, (x, y) in enumerate(zip(chis, chis_ref)):
        print("iteration %d: chi2 %.15g ref %.15g rel %.3g (tol %.3g)" % (i, x, y, abs(x - y) / abs(y), tol[i]))
    chi0 = RR.total_chi2(start, P, rp)
    for i, (x, y) in enumerate(zip(chis, chis_ref)):
        # (zero-noise measurements: chi2 ends at rounding level — residuals of 1e-16 |t| squared, some 1e-30 of the
        #  start — where the two loops no longer take the same trials and "relative" has no meaning; the floor of
        #  1e-20 chi2_0 is residuals 1e-10 of the initial ones, ten orders of magnitude above that level)
        assert abs(x - y) <= tol[i] * abs(y) + 1e-20 * chi0, (i, x, y)
    err = max(np.abs(PR.residual(poses[p], gt[p])).max() for p in range(P))  # [Log(R R_gt^T); t - R R_gt^T t_gt]
    print("chi2 %.3g -> %.3g; distance to the ground truth %.3g" % (chi0, chis[-1], err))
    assert chis[-1] < 1e-16 * chi0 and err < 1e-8
