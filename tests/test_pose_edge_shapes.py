"""The unary pose edge kernels (icp_kernels.hip, prior_kernels.hip, pose_edge_kernels.hip) on the designed layouts of
tests/pose_designed.py, through the kernel-level C ABI, against the extended-precision reference of
tests/pose_edge_ref.py with its per-entry bounds (test_pose_edge_ref_host.py pins both on the CPU).

For every layout: H (both triangles, exactly symmetric), b, the chi2 total and the error pass's chi2 per edge inside the
bounds; error-pass chi2 bit-equal to the build pass's; a second run bit-equal; fixed and inactive edges exactly 0; with
a random prefill the poses without a counting edge keep their bits.  The Schur destination (the form the default LM loop
uses) through cugo_icp_construct_quadratic_form_schur / cugo_prior_construct_quadratic_form_schur with rowptr[p] != p.
The index check beyond its first grid-stride trip (more than 1024 x 256 edges)."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import pose_designed as pd
import pose_edge_ref as per
import prior_ref

pytestmark = pytest.mark.gpu

cugo = importlib.import_module("cuda-bundle-adjustment_amd")

ICP_NAMES = list(pd.ICP_LAYOUTS) + ["F"]
KEYS = ("H", "b", "chi", "chi_edge")


@pytest.fixture(scope="module")
def ctx():
    import devmem
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    c = devmem.Ctx()
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def icp_reference(name):
    lay = pd.icp_layout(name)
    return per.icp_build(lay["poses"], lay["n_free"], pd.kinds_of(lay), full=name != "G")


@functools.lru_cache(maxsize=None)
def prior_reference(name):
    lay = pd.prior_layout(name)
    return per.prior_build(lay["poses"], lay["n_free"], lay["pr"])


def blocks(a, n):
    """[n][36] column-major device blocks -> [n, 6, 6] matrices"""
    return np.asarray(a).reshape(n, 6, 6).transpose(0, 2, 1)


def upload_icp(ctx, lay, flags="given", pose_override=None):
    ev = cugo.IcpEdges()
    ev.n_poses_total, ev.n_poses_free = lay["P"], lay["n_free"]
    for kind in ("plane", "line"):
        e = lay[kind]
        n = 0 if e is None else len(e["pose"])
        setattr(ev, "n_" + kind, n)
        if e is None:
            setattr(ev, "d_%s_pose_ptr" % kind, ctx.to_dev(np.zeros(lay["P"] + 1, np.int32)))
            continue
        pose = np.asarray(e["pose"], np.int32)
        setattr(ev, "d_%s_pose_ptr" % kind, ctx.to_dev(pd.pose_ptr(pose, lay["P"])))
        if pose_override is not None and kind in pose_override:
            pose = pose_override[kind]
        setattr(ev, "d_%s_pose" % kind, ctx.to_dev(pose))
        p, geo = pd.device_arrays(e, kind)
        setattr(ev, "d_%s_p" % kind, ctx.to_dev(p))
        setattr(ev, "d_plane_nd" if kind == "plane" else "d_line_au", ctx.to_dev(geo))
        omega = np.asarray(e["omega"], np.float64)
        setattr(ev, "d_%s_omega" % kind, ctx.to_dev(omega))
        setattr(ev, "n_%s_omega" % kind, len(omega))
        if flags == "given":
            setattr(ev, "d_%s_flags" % kind, ctx.to_dev(e["flags"]))
        elif flags == "zeros":
            setattr(ev, "d_%s_flags" % kind, ctx.to_dev(np.zeros(n, np.uint8)))
        setattr(ev, "rk_" + kind, e["rk"][0])
        setattr(ev, "delta_" + kind, e["rk"][1])
    return ev


def n_edges(lay):
    return sum(len(lay[k]["pose"]) for k in ("plane", "line") if lay.get(k) is not None)


class Runner:
    """one uploaded edge set (ICP or prior) and the passes over it"""

    def __init__(self, ctx, ev, poses, n_free, n_edges, prior):
        self.ctx, self.ev, self.P, self.E = ctx, ev, n_free, n_edges
        self.d_poses = ctx.to_dev(poses)
        lib = cugo.lib()
        self.f_build = lib.cugo_prior_construct_quadratic_form if prior else lib.cugo_icp_construct_quadratic_form
        self.f_err = lib.cugo_prior_compute_errors if prior else lib.cugo_icp_compute_errors
        self.f_schur = cugo.prior_construct_quadratic_form_schur if prior else cugo.icp_construct_quadratic_form_schur

    def build(self, H0=None, b0=None, rc=0, all_rows=False):
        """-> H [P,6,6], b [P,6], chi (all_rows: every row of the prefill, for n_poses_free = 0)"""
        H0 = np.zeros((max(self.P, 1), 36)) if H0 is None else H0
        b0 = np.zeros((max(self.P, 1), 6)) if b0 is None else b0
        d_H, d_b, d_chi = self.ctx.to_dev(H0), self.ctx.to_dev(b0), self.ctx.to_dev(np.array([-7.0, 0.0]))
        got = self.f_build(self.ctx.h, C.byref(self.ev), self.d_poses, d_H, d_b, d_chi)
        assert got == rc, (got, cugo.lib().cugo_last_error())
        keep = len(H0) if all_rows else self.P
        return blocks(self.ctx.to_host(d_H, H0.shape), len(H0))[:keep], self.ctx.to_host(d_b, b0.shape)[:keep], self.ctx.to_host(d_chi, 1)[0]

    def errors(self):
        d_chi, d_edge = self.ctx.empty(2), self.ctx.to_dev(np.full(max(self.E, 1), -3.0))
        cugo.check(self.f_err(self.ctx.h, C.byref(self.ev), self.d_poses, d_chi, d_edge))
        return self.ctx.to_host(d_chi, 1)[0], self.ctx.to_host(d_edge, max(self.E, 1))[:self.E]

    def schur(self, rowptr, Hsc0, bp0, bsc0):
        d_H, d_bp, d_bsc, d_chi = (self.ctx.to_dev(a) for a in (Hsc0, bp0, bsc0, np.zeros(2)))
        self.f_schur(self.ctx.h, self.ev, self.d_poses, self.ctx.to_dev(rowptr), d_H, d_bp, d_bsc, d_chi)
        return (self.ctx.to_host(d_H, Hsc0.shape), self.ctx.to_host(d_bp, bp0.shape), self.ctx.to_host(d_bsc, bsc0.shape),
                self.ctx.to_host(d_chi, 1)[0])


def icp_runner(ctx, lay, **kw):
    return Runner(ctx, upload_icp(ctx, lay, **kw), lay["poses"], lay["n_free"], n_edges(lay), False)


def prior_runner(ctx, lay, pr=None):
    pr = lay["pr"] if pr is None else pr
    return Runner(ctx, prior_ref.upload(ctx, lay["P"], lay["n_free"], pr), lay["poses"], lay["n_free"], len(pr["pose"]), True)


def check_all(tag, run, ref, bound_of, counting, keys=KEYS):
    """the checks every layout gets; counting [P]: the number of counting edges per free pose"""
    P = run.P
    out = {}
    chi_e, edge = run.errors()
    if "H" in keys:
        H, b, chi = run.build()
        assert np.array_equal(H, H.transpose(0, 2, 1)), "H not exactly symmetric"
        out = dict(H=H, b=b, chi=chi)
        assert chi_e == chi, ("error-pass chi2 differs from the build pass's", chi_e, chi)
        H2, b2, chi2 = run.build()
        assert np.array_equal(H, H2) and np.array_equal(b, b2) and chi == chi2, "a second run differs"
        # random prefill: poses without a counting edge keep their bits, the others moved
        rng = np.random.default_rng(5)
        H0, b0 = rng.normal(size=(max(P, 1), 36)), rng.normal(size=(max(P, 1), 6))
        H3, b3, chi3 = run.build(H0, b0)
        idle = np.flatnonzero(np.asarray(counting) == 0)
        assert np.array_equal(H3[idle], blocks(H0, len(H0))[:P][idle]) and np.array_equal(b3[idle], b0[:P][idle]) and chi3 == chi
    else:
        out = dict(chi=chi_e)
    out["chi_edge"] = edge
    chi_e2, edge2 = run.errors()
    assert chi_e2 == chi_e and np.array_equal(edge, edge2)
    assert np.all(edge[np.asarray(ref["chi_edge_mass"]) == 0] == 0), "a fixed or inactive edge has a chi2 term"
    msg = []
    for k in keys:
        r = per.ratio(out[k], ref[k], bound_of(ref, k))
        msg.append("%s %.3g" % (k, r))
        assert r <= 1, (tag, k, r)
    print("%s: largest error / bound: %s" % (tag, "  ".join(msg)))
    return out


def icp_counting(lay):
    cnt = np.zeros(max(lay["n_free"], 0), np.int64)
    for _, e in pd.kinds_of(lay):
        live = (e["pose"] < lay["n_free"]) & e["active"]
        cnt += np.bincount(e["pose"][live], minlength=lay["n_free"])[:lay["n_free"]]
    return cnt


# ------------------------------------------------------------------ ICP
@pytest.mark.parametrize("name", [n for n in ICP_NAMES if n != "C0"])
def test_icp_layout(ctx, name):
    lay = pd.icp_layout(name)
    check_all("icp " + name, icp_runner(ctx, lay), icp_reference(name), per.icp_bound, icp_counting(lay))


def test_icp_without_free_poses_touches_nothing(ctx):
    """I-C with n_poses_free = 0: H and b keep their bits, chi2 is exactly 0"""
    lay = pd.icp_layout("C0")
    run = icp_runner(ctx, lay)
    rng = np.random.default_rng(6)
    H0, b0 = rng.normal(size=(lay["P"], 36)), rng.normal(size=(lay["P"], 6))
    H, b, chi = run.build(H0, b0, all_rows=True)
    assert np.array_equal(H, blocks(H0, lay["P"])) and np.array_equal(b, b0) and chi == 0.0
    chi_e, edge = run.errors()
    assert chi_e == 0.0 and not edge.any()


def test_icp_error_pass_on_513_chunks(ctx):
    """I-G: 262 656 plane edges, 513 chunk totals (three trips of k_pose_chi_total); also the sorted layout beyond the
    first trip of the index check is accepted"""
    lay = pd.icp_layout("G")
    check_all("icp G", icp_runner(ctx, lay), icp_reference("G"), per.icp_bound, icp_counting(lay), keys=("chi", "chi_edge"))


@pytest.mark.parametrize("rk", pd.RKS)
def test_icp_zero_residual(ctx, rk):
    """I-E: r exactly 0 in double: everything finite, chi2 and b exactly 0, H inside its bounds"""
    lay = pd.icp_zero_residual(rk)
    ref = per.icp_build(lay["poses"], lay["n_free"], pd.kinds_of(lay))
    out = check_all("icp E rk %d" % rk[0], icp_runner(ctx, lay), ref, per.icp_bound, icp_counting(lay))
    assert out["chi"] == 0.0 and not out["chi_edge"].any() and not out["b"].any() and np.all(np.isfinite(out["H"])) and out["H"].any()


def test_icp_null_flags_equal_zero_flags_and_one_omega_equals_tiled(ctx):
    lay = pd.icp_layout("AB")
    a = icp_runner(ctx, lay, flags=None).build()
    b = icp_runner(ctx, lay, flags="zeros").build()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    one = dict(lay, plane=dict(lay["plane"], omega=np.array([1.7])), line=dict(lay["line"], omega=np.array([0.6])))
    tiled = dict(lay, plane=dict(lay["plane"], omega=np.full(len(lay["plane"]["pose"]), 1.7)),
                 line=dict(lay["line"], omega=np.full(len(lay["line"]["pose"]), 0.6)))
    a, b = icp_runner(ctx, one).build(), icp_runner(ctx, tiled).build()
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[2] > 0
    ea, eb = icp_runner(ctx, one).errors(), icp_runner(ctx, tiled).errors()
    assert ea[0] == eb[0] == a[2] and np.array_equal(ea[1], eb[1])


# ------------------------------------------------------------------ priors
def prior_counting(lay):
    pr = lay["pr"]
    live = (pr["pose"] < lay["n_free"]) & pr["active"]
    return np.bincount(pr["pose"][live], minlength=lay["n_free"])[:lay["n_free"]]


@pytest.mark.parametrize("name", pd.PRIOR_NAMES)
def test_prior_layout(ctx, name):
    lay = pd.prior_layout(name)
    ref = prior_reference(name)
    out = check_all("prior " + name, prior_runner(ctx, lay), ref, per.prior_bound, prior_counting(lay))
    assert np.all(np.isfinite(out["H"])) and np.all(np.isfinite(out["b"])) and np.isfinite(out["chi"])
    if name == "B":     # the figures per angle (DESIGN.md section 13 quotes the two next to pi)
        bH = per.prior_bound(ref, "H")
        for p, th in enumerate(pd.ANGLES):
            err = float(np.abs(out["H"][p] - ref["H"][p]).max() / np.abs(ref["H"][p]).max())
            print("  theta %-22.17g H: relative error %.3g, %.3g of its bound" % (th, err, per.ratio(out["H"][p], ref["H"][p], bH[p])))
    if name.startswith("C_zero"):
        assert not out["H"].any() and not out["b"].any() and out["chi"] == 0.0
    if name.startswith("C_one"):    # one matrix for all edges and the same matrix per edge: the same bits
        a = prior_runner(ctx, lay, pd.per_edge_info(lay["pr"])).build()
        assert np.array_equal(a[0], out["H"]) and np.array_equal(a[1], out["b"]) and a[2] == out["chi"]


# ------------------------------------------------------------------ the Schur destination
def schur_checks(tag, run, P):
    rowptr, B = pd.schur_rows(P)
    diag = rowptr[:P]
    rng = np.random.default_rng(9)
    H, b, chi = run.build()
    # zero prefill: the diagonal blocks, bp (and bsc) have the bits of the Hpp form
    Hs, bp, bsc, chis = run.schur(rowptr, np.zeros((B, 36)), np.zeros((P, 6)), np.zeros((P, 6)))
    Hs = blocks(Hs, B)
    assert np.array_equal(Hs[diag], H) and np.array_equal(bp, b) and np.array_equal(bsc, b) and chis == chi
    other = np.setdiff1d(np.arange(B), diag)
    assert not Hs[other].any()
    # random prefill of the whole array: every block but rowptr[p] keeps its bits; bp and bsc receive the same term
    H0, bp0, bsc0 = rng.normal(size=(B, 36)), rng.normal(size=(P, 6)), 100 * rng.normal(size=(P, 6))
    Hs, bp, bsc, _ = run.schur(rowptr, H0, bp0, bsc0)
    assert np.array_equal(Hs[other], H0[other]), "a block that is not a diagonal block changed"
    moved = np.flatnonzero((np.abs(b).sum(1) > 0) | (np.abs(H).sum((1, 2)) > 0))
    assert len(moved) and all(not np.array_equal(Hs[diag[p]], H0[diag[p]]) for p in moved if H[p].any())
    idle = np.setdiff1d(np.arange(P), moved)
    assert np.array_equal(Hs[diag[idle]], H0[diag[idle]]) and np.array_equal(bp[idle], bp0[idle]) and np.array_equal(bsc[idle], bsc0[idle])
    # the term that arrives is the Hpp form's, bit for bit: one add of it to the prefill, which numpy repeats exactly (no
    # subtraction of rounded sums); so bp and bsc, prefilled differently, receive the SAME term
    assert np.array_equal(bp, bp0 + b) and np.array_equal(bsc, bsc0 + b), "bp and bsc did not receive the Hpp form's term"
    assert np.array_equal(blocks(Hs, B)[diag], blocks(H0, B)[diag] + H), "a diagonal block did not receive the Hpp form's term"
    ulp = 2.0 ** -52      # (what the above implies: the two increments agree within one ulp of the prefilled values' scale)
    tol = ulp * (np.maximum(np.abs(bp0), np.abs(bp)) + np.maximum(np.abs(bsc0), np.abs(bsc)))
    d = np.abs((bp - bp0) - (bsc - bsc0))
    assert np.all(d <= tol), ("bp and bsc received different terms", float((d / tol).max()))
    print("%s: Schur destination bit-equal to the Hpp form on %d poses (%d blocks, %d moved)" % (tag, P, B, len(moved)))


@pytest.mark.parametrize("name", ["A_plane", "AB", "C_both", "C2_line"])
def test_icp_schur_destination(ctx, name):
    lay = pd.icp_layout(name)
    schur_checks("icp " + name, icp_runner(ctx, lay), lay["n_free"])


@pytest.mark.parametrize("name", ["A9", "A17", "B"])
def test_prior_schur_destination(ctx, name):
    lay = pd.prior_layout(name)
    schur_checks("prior " + name, prior_runner(ctx, lay), lay["n_free"])


# ------------------------------------------------------------------ the index check beyond its first trip
def test_index_check_sees_an_edge_beyond_the_first_grid_stride_trip(ctx):
    lay = pd.icp_layout("G")
    pose = lay["plane"]["pose"].astype(np.int32).copy()
    i = 1024 * 256 + 300
    assert i < len(pose) and pose[i] != 0
    pose[i] = 0                                            # outside its pose's range; every edge before it is in place
    run = icp_runner(ctx, lay, pose_override={"plane": pose})
    H, b, chi = run.build(rc=-3)
    assert not H.any() and not b.any() and chi == -7.0     # refused: nothing written
    d_chi = ctx.to_dev(np.array([-7.0, 0.0]))
    assert cugo.lib().cugo_icp_compute_errors(ctx.h, C.byref(run.ev), run.d_poses, d_chi, None) == -3
    assert ctx.to_host(d_chi, 1)[0] == -7.0
    H, b, chi = icp_runner(ctx, lay).build()               # the sorted layout is accepted
    assert H.any() and chi > 0


def test_index_check_on_a_prior_set_beyond_the_first_trip(ctx):
    n = 1024 * 256 + 512
    rng = np.random.default_rng(12)
    pose = np.zeros(n, np.int32)
    pose[-56:] = 1
    z = rng.normal(size=(n, 7))
    z[:, :4] /= np.linalg.norm(z[:, :4], axis=1)[:, None]
    pr = prior_ref.make_prior(pose, z, np.eye(6)[None])
    poses = np.array([[0, 0, 0, 1.0, 0, 0, 0]] * 2)
    ev = prior_ref.upload(ctx, 2, 2, pr)
    bad = pose.copy()
    bad[1024 * 256 + 300] = 1
    ev.d_pose = ctx.to_dev(bad)
    d_H, d_b, d_chi = ctx.to_dev(np.zeros(72)), ctx.to_dev(np.zeros(12)), ctx.to_dev(np.array([-7.0, 0.0]))
    assert cugo.lib().cugo_prior_construct_quadratic_form(ctx.h, C.byref(ev), ctx.to_dev(poses), d_H, d_b, d_chi) == -3
    assert not ctx.to_host(d_H, 72).any() and not ctx.to_host(d_b, 12).any() and ctx.to_host(d_chi, 1)[0] == -7.0
