"""The covariance form of the two point kinds (k_gicp_chunks_*, k_gicp_pair_chunks_*) on the designed layouts of
tests/gicp_designed.py, through the kernel-level C ABI (cugo_gicp_*, cugo_gicp_pair_*), against the extended-precision
reference of tests/gicp_ref.py with its per-entry bounds and its constant C_OMEGA unchanged (test_gicp_ref_host.py pins
both on the CPU).

For every layout and covariance class: the error pass, the plain form and the Schur form (rowptr[p] != p) inside the
bounds; H exactly symmetric; the build pass's chi2 bit-equal to the error pass's; a second run bit-equal; with a random
prefill what has no counting edge or run and the rows of fixed poses keep their bits and what arrives is ADDED; _diag +
add_offdiag_schur give the bits of the Schur form with an error pass at other poses in between; an error pass at other
poses gives the cost AT those poses.  With T_a the fixed identity the pair term is the unary term on b; class zero_p is
the information form fed C_z^-1; the index check beyond its first grid-stride trip; refusals before any launch."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import gicp_designed as gd
import gicp_ref as gr
import pair_designed as pdz
import point_designed as pt
import point_edge_ref as ptr_ref
import point_pair_ref as ppr
import pose_designed as pd
from test_pose_edge_shapes import Runner as UnaryRunner, blocks, check_all, schur_checks
from test_point_pair_shapes import Runner as InfoPairRunner, pattern_of
from test_point_edge_shapes import PointRunner as InfoPointRunner

pytestmark = pytest.mark.gpu

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
LD = gr.LD


@pytest.fixture(scope="module")
def ctx():
    import devmem
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    c = devmem.Ctx()
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def pair_reference(name):
    lay = gd.pair_layout(name)
    return gr.pair_build(lay["poses"], lay["n_free"], lay["P"], lay["e"])


@functools.lru_cache(maxsize=None)
def point_reference(name):
    lay = gd.point_layout(name)
    return gr.point_build(lay["poses"], lay["n_free"], lay["e"])


# ------------------------------------------------------------------ the unary kind
def upload_point(ctx, lay, pose_override=None):
    e = lay["e"]
    ev = cugo.GicpEdges()
    ev.n_poses_total, ev.n_poses_free, ev.n = lay["P"], lay["n_free"], len(e["pose"])
    pose = np.asarray(e["pose"], np.int32)
    ev.d_pose_ptr = ctx.to_dev(pd.pose_ptr(pose, lay["P"]))
    ev.d_pose = ctx.to_dev(pose if pose_override is None else pose_override)
    p, z, cp, cz = gd.point_device_arrays(e)
    ev.d_p, ev.d_z, ev.d_cov_p, ev.d_cov_z, ev.n_cov = ctx.to_dev(p), ctx.to_dev(z), ctx.to_dev(cp), ctx.to_dev(cz), cp.shape[1]
    if e.get("flags") is not None:
        ev.d_flags = ctx.to_dev(e["flags"])
    ev.rk, ev.delta = e["rk"]
    return ev


class GicpRunner(UnaryRunner):
    def __init__(self, ctx, lay, poses=None, **kw):
        self.ctx, self.ev, self.P, self.E = ctx, upload_point(ctx, lay, **kw), lay["n_free"], len(lay["e"]["pose"])
        self.d_poses = ctx.to_dev(lay["poses"] if poses is None else poses)
        lib = cugo.lib()
        self.f_build, self.f_err = lib.cugo_gicp_construct_quadratic_form, lib.cugo_gicp_compute_errors
        self.f_schur = cugo.gicp_construct_quadratic_form_schur


@pytest.mark.parametrize("name", gd.POINT_NAMES)
def test_point_layout(ctx, name):
    lay = gd.point_layout(name)
    run = GicpRunner(ctx, lay)
    check_all("gicp " + name, run, point_reference(name), gr.point_bound, gd.counting(lay))
    schur_checks("gicp " + name, run, lay["n_free"])


def test_point_error_pass_at_other_poses_is_the_cost_at_those_poses(ctx):
    lay = gd.point_layout("A_gicp")
    P2 = gd.moved(lay["poses"])
    ref2 = gr.point_build(P2, lay["n_free"], lay["e"], full=False)
    chi, edge = GicpRunner(ctx, lay, poses=P2).errors()
    assert gr.ratio(chi, ref2["chi"], gr.point_bound(ref2, "chi")) <= 1
    assert gr.ratio(edge, ref2["chi_edge"], gr.point_bound(ref2, "chi_edge")) <= 1
    frozen = ptr_ref.point_build(P2, lay["n_free"], gr.with_info(lay["e"], gr.omega_of(lay["poses"], lay["e"])[0]), full=False)
    assert gr.ratio(frozen["chi"], ref2["chi"], gr.point_bound(ref2, "chi")) > 1e3      # (what a frozen Omega would give)


def test_point_zero_p_is_the_information_form_fed_the_inverse_of_cov_z(ctx):
    lay = gd.point_layout("B_zero_p")
    ref = point_reference("B_zero_p")
    info = gr.with_info(lay["e"], np.asarray(ref["Omega"]).astype(np.float64))
    ref_i = ptr_ref.point_build(lay["poses"], lay["n_free"], info)
    rg, ri = GicpRunner(ctx, lay), InfoPointRunner(ctx, dict(lay, e=info))
    got, want = rg.build() + (rg.errors()[1],), ri.build() + (ri.errors()[1],)
    for k, a, b in zip(("H", "b", "chi", "chi_edge"), got, want):
        r = gr.ratio(a, b, gr.point_bound(ref, k) + ptr_ref.point_bound(ref_i, k))
        assert r <= 1, (k, r)
    assert got[2] > 0


# ------------------------------------------------------------------ the pair kind
class PairRunner:
    """one uploaded covariance-form set in its plan's order and the passes over it"""

    def __init__(self, ctx, lay, ref, pose_a_override=None):
        e = lay["e"]
        self.ctx, self.P, self.Pall, self.E = ctx, lay["n_free"], lay["P"], len(e["a"])
        self.rowptr, self.colind = pattern_of(lay, ref)
        self.nnzb = len(self.colind)
        self.plan = cugo.PointPairPlan(ctx.h, self.Pall, self.P, e["a"], e["b"], e.get("flags"), self.rowptr, self.colind)
        self.perm = self.plan.array("perm")
        self.blk_id = self.plan.array("blk_id")
        pa, pb, p, z, cp, cz, fl = gd.pair_device_arrays(e, self.perm)
        ev = cugo.GicpPairEdges()
        ev.n_poses_total, ev.n_poses_free, ev.n = self.Pall, self.P, self.E
        ev.d_pose_a, ev.d_pose_b = ctx.to_dev(pa if pose_a_override is None else pose_a_override), ctx.to_dev(pb)
        ev.d_p, ev.d_z, ev.d_cov_p, ev.d_cov_z, ev.n_cov = ctx.to_dev(p), ctx.to_dev(z), ctx.to_dev(cp), ctx.to_dev(cz), cp.shape[1]
        if fl is not None:
            ev.d_flags = ctx.to_dev(fl)
        ev.rk, ev.delta = e["rk"]
        ev.plan = self.plan.handle
        self.ev = ev
        self.d_poses = ctx.to_dev(lay["poses"])
        self.d_rowptr = ctx.to_dev(self.rowptr)

    def close(self):
        self.plan.close()

    def _dev(self, a, shape):
        return self.ctx.to_dev(np.zeros(shape) if a is None else a)

    def _chi(self):
        return self.ctx.to_dev(np.array([-7.0, 0.0]))

    def errors(self, d_poses=None):
        """chi2 total and the term of every edge in the CALLER's order"""
        d_chi, d_edge = self._chi(), self.ctx.to_dev(np.full(self.E, -3.0))
        cugo.gicp_pair_compute_errors(self.ctx.h, self.ev, self.d_poses if d_poses is None else d_poses, d_chi, d_edge)
        edge = np.zeros(self.E)
        edge[self.perm] = self.ctx.to_host(d_edge, self.E)
        return self.ctx.to_host(d_chi, 1)[0], edge

    def build(self, H0=None, b0=None, Hoff0=None):
        d_H, d_b, d_Hoff = self._dev(H0, (self.Pall, 36)), self._dev(b0, (self.Pall, 6)), self._dev(Hoff0, (self.nnzb, 36))
        d_chi = self._chi()
        cugo.gicp_pair_construct_quadratic_form(self.ctx.h, self.ev, self.d_poses, d_H, d_b, d_Hoff, d_chi)
        return (blocks(self.ctx.to_host(d_H, (self.Pall, 36)), self.Pall), self.ctx.to_host(d_b, (self.Pall, 6)),
                blocks(self.ctx.to_host(d_Hoff, (self.nnzb, 36)), self.nnzb), self.ctx.to_host(d_chi, 1)[0])

    def build_diag(self):
        d_H, d_b, d_chi = self._dev(None, (self.Pall, 36)), self._dev(None, (self.Pall, 6)), self._chi()
        cugo.gicp_pair_construct_quadratic_form_diag(self.ctx.h, self.ev, self.d_poses, d_H, d_b, d_chi)
        return blocks(self.ctx.to_host(d_H, (self.Pall, 36)), self.Pall), self.ctx.to_host(d_b, (self.Pall, 6)), self.ctx.to_host(d_chi, 1)[0]

    def add_offdiag(self, Hsc0=None):
        d_H = self._dev(Hsc0, (self.nnzb, 36))
        cugo.gicp_pair_add_offdiag_schur(self.ctx.h, self.ev, d_H)
        return blocks(self.ctx.to_host(d_H, (self.nnzb, 36)), self.nnzb)

    def schur(self, Hsc0=None, bp0=None, bsc0=None):
        d_H, d_bp, d_bsc = self._dev(Hsc0, (self.nnzb, 36)), self._dev(bp0, (self.Pall, 6)), self._dev(bsc0, (self.Pall, 6))
        d_chi = self._chi()
        cugo.gicp_pair_construct_quadratic_form_schur(self.ctx.h, self.ev, self.d_poses, self.d_rowptr, d_H, d_bp, d_bsc, d_chi)
        return (blocks(self.ctx.to_host(d_H, (self.nnzb, 36)), self.nnzb), self.ctx.to_host(d_bp, (self.Pall, 6)),
                self.ctx.to_host(d_bsc, (self.Pall, 6)), self.ctx.to_host(d_chi, 1)[0])


def check_pair_layout(tag, ctx, lay, ref):
    run = PairRunner(ctx, lay, ref)
    P, Pall, nnzb = run.P, run.Pall, run.nnzb
    diag, touched = run.rowptr[:P], run.blk_id
    assert len(touched) == len(ref["pair_lo"])
    untouched = np.setdiff1d(np.arange(nnzb), touched)               # the diagonal blocks and the blocks no run maps to
    idle = np.flatnonzero(np.asarray(ref["H_n"]).reshape(-1) == 0)   # poses without a counting run, the fixed ones among them
    assert set(range(P, Pall)) <= set(idle.tolist())
    chi_e, edge = run.errors()
    H, b, Hoff, chi = run.build()
    assert chi_e == chi, ("error-pass chi2 differs from the build pass's", chi_e, chi)
    assert np.array_equal(H, H.transpose(0, 2, 1)), "H not exactly symmetric"
    assert not Hoff[untouched].any() and not H[idle].any() and not b[idle].any()
    assert np.all(edge[np.asarray(ref["chi_edge_mass"]) == 0] == 0), "an edge that does not count has a chi2 term"
    msg = []
    for k, got in (("H", H), ("b", b), ("Hoff", Hoff[touched]), ("chi", chi), ("chi_edge", edge)):
        r = gr.ratio(got, ref[k], gr.pair_bound(ref, k))
        msg.append("%s %.3g" % (k, r))
        assert r <= 1, (tag, k, r)
    print("%s: largest error / bound: %s" % (tag, "  ".join(msg)))
    again = run.build()
    assert all(np.array_equal(x, y) for x, y in zip((H, b, Hoff, chi), again)), "a second run differs"
    chi_e2, edge2 = run.errors()
    assert chi_e2 == chi_e and np.array_equal(edge, edge2)
    # random prefill: what has no counting run keeps its bits (fixed rows among them), everything else receives the term, ADDED
    rng = np.random.default_rng(5)
    H0, b0, Hoff0 = rng.normal(size=(Pall, 36)), rng.normal(size=(Pall, 6)), rng.normal(size=(nnzb, 36))
    H3, b3, Hoff3, chi3 = run.build(H0, b0, Hoff0)
    assert chi3 == chi
    assert np.array_equal(H3, blocks(H0, Pall) + H) and np.array_equal(b3, b0 + b) and np.array_equal(Hoff3, blocks(Hoff0, nnzb) + Hoff)
    assert np.array_equal(H3[idle], blocks(H0, Pall)[idle]) and np.array_equal(b3[idle], b0[idle])
    assert np.array_equal(Hoff3[untouched], blocks(Hoff0, nnzb)[untouched])
    # the Schur destination: the bits of the plain form, the diagonal through rowptr (rowptr[p] != p), b to bp and bsc
    assert np.any(diag != np.arange(P))
    Hs, bp, bsc, chis = run.schur()
    assert chis == chi and np.array_equal(Hs[diag], H[:P]) and np.array_equal(Hs[touched], Hoff[touched])
    assert np.array_equal(bp, b) and np.array_equal(bsc, b)
    assert not Hs[np.setdiff1d(untouched, diag)].any()
    bp0, bsc0 = rng.normal(size=(Pall, 6)), 100 * rng.normal(size=(Pall, 6))
    Hs2, bp2, bsc2, _ = run.schur(Hoff0, bp0, bsc0)
    want = blocks(Hoff0, nnzb).copy()
    want[diag] += H[:P]
    want[touched] += Hoff[touched]
    assert np.array_equal(Hs2, want), "Hsc was not added to, block by block"
    assert np.array_equal(bp2, bp0 + b) and np.array_equal(bsc2, bsc0 + b)
    # the split: the diagonal pass, an error pass at OTHER poses (its chi2 is the cost there), then the off-diagonal sums
    Hd, bd, chid = run.build_diag()
    assert np.array_equal(Hd, H) and np.array_equal(bd, b) and chid == chi
    other = gd.moved(lay["poses"])
    ref_o = gr.pair_build(other, lay["n_free"], lay["P"], lay["e"])
    chi_o, edge_o = run.errors(ctx.to_dev(other))
    assert gr.ratio(chi_o, ref_o["chi"], gr.pair_bound(ref_o, "chi")) <= 1 and gr.ratio(edge_o, ref_o["chi_edge"], gr.pair_bound(ref_o, "chi_edge")) <= 1
    Ho = run.add_offdiag(Hoff0)
    want = blocks(Hoff0, nnzb).copy()
    want[touched] += Hoff[touched]
    assert np.array_equal(Ho, want), "the error pass disturbed the partials, or the off-diagonal pass is not the Schur form's"
    run.close()
    return dict(H=H, b=b, Hoff=Hoff, chi=chi, chi_edge=edge)


@pytest.mark.parametrize("name", gd.PAIR_NAMES)
def test_pair_layout(ctx, name):
    out = check_pair_layout("gicp pair " + name, ctx, gd.pair_layout(name), pair_reference(name))
    assert out["chi"] > 0 and out["Hoff"].any()


def test_pair_with_the_fixed_identity_as_a_is_the_unary_term_on_b(ctx):
    lp, lu = gd.pair_unary_twin()
    ref_p = gr.pair_build(lp["poses"], lp["n_free"], lp["P"], lp["e"])
    ref_u = gr.point_build(lu["poses"], lu["n_free"], lu["e"])
    rp, ru = PairRunner(ctx, lp, ref_p), GicpRunner(ctx, lu)
    Hp, bp, _, chip = rp.build()
    edge_p = rp.errors()[1]
    Hu, bu, chiu = ru.build()
    edge_u = ru.errors()[1]
    P = lp["n_free"]
    assert not Hp[P:].any() and not bp[P:].any()                # the fixed identity is never written
    msg = []
    for k, a, b, bnd in (("H", Hp[:P], Hu, gr.pair_bound(ref_p, "H")[:P] + gr.point_bound(ref_u, "H")),
                         ("b", bp[:P], bu, gr.pair_bound(ref_p, "b")[:P] + gr.point_bound(ref_u, "b")),
                         ("chi", chip, chiu, gr.pair_bound(ref_p, "chi") + gr.point_bound(ref_u, "chi")),
                         ("chi_edge", edge_p, edge_u, gr.pair_bound(ref_p, "chi_edge") + gr.point_bound(ref_u, "chi_edge"))):
        r = gr.ratio(a, b, bnd)
        msg.append("%s %.3g" % (k, r))
        assert r <= 1, (k, r)
    print("pair with a the fixed identity against the unary kind: largest difference / summed bounds: %s" % "  ".join(msg))
    assert chiu > 0 and Hu.any()
    rp.close()


def test_pair_zero_p_is_the_information_form_fed_the_inverse_of_cov_z(ctx):
    lay, ref = gd.pair_layout("A_zero_p"), pair_reference("A_zero_p")
    info = gr.with_info(lay["e"], np.asarray(ref["Omega"]).astype(np.float64))
    ref_i = ppr.pair_build(lay["poses"], lay["n_free"], lay["P"], info)
    rg, ri = PairRunner(ctx, lay, ref), InfoPairRunner(ctx, lay, ref, e=info)
    got, want = rg.build() + (rg.errors()[1],), ri.build() + (ri.errors()[1],)
    for k, a, b in zip(("H", "b", "Hoff", "chi", "chi_edge"), got, want):
        if k == "Hoff":
            a, b = a[rg.blk_id], b[ri.blk_id]
        r = gr.ratio(a, b, gr.pair_bound(ref, k) + ppr.pair_bound(ref_i, k))
        assert r <= 1, (k, r)
    assert got[3] > 0
    rg.close()
    ri.close()


def test_one_covariance_pair_equals_tiled(ctx):
    lay, ref = gd.pair_layout("A_one"), pair_reference("A_one")
    E = len(lay["e"]["a"])
    tiled = dict(lay, e=dict(lay["e"], cov_p6=np.tile(lay["e"]["cov_p6"], (E, 1)), cov_z6=np.tile(lay["e"]["cov_z6"], (E, 1))))
    a, b = PairRunner(ctx, lay, ref), PairRunner(ctx, tiled, ref)
    assert a.ev.n_cov == 1 and b.ev.n_cov == E
    assert all(np.array_equal(x, y) for x, y in zip(a.build(), b.build()))
    assert all(np.array_equal(x, y) for x, y in zip(a.errors(), b.errors()))
    a.close()
    b.close()


# ------------------------------------------------------------------ refusals before any launch
def test_pair_index_check_sees_an_edge_beyond_the_first_grid_stride_trip(ctx):
    lay = gd.index_check_layout("pair")
    e = lay["e"]
    ref = dict(pair_lo=np.array([0]), pair_hi=np.array([1]))
    pose_a = np.asarray(e["a"], np.int32).copy()
    i = 1024 * 256 + 300
    assert i < len(pose_a) and pose_a[i] == 0
    pose_a[i] = 1                                           # not the a of its run; every edge before it is in place
    run = PairRunner(ctx, lay, ref, pose_a_override=pose_a)
    assert np.array_equal(run.perm, np.arange(len(pose_a)))
    d_H, d_b, d_Hoff = ctx.to_dev(np.zeros((3, 36))), ctx.to_dev(np.zeros((3, 6))), ctx.to_dev(np.zeros((run.nnzb, 36)))
    d_chi = ctx.to_dev(np.array([-7.0, 0.0]))
    lib = cugo.lib()
    assert lib.cugo_gicp_pair_construct_quadratic_form(ctx.h, C.byref(run.ev), run.d_poses, d_H, d_b, d_Hoff, d_chi) == -3
    assert lib.cugo_gicp_pair_compute_errors(ctx.h, C.byref(run.ev), run.d_poses, d_chi, None) == -3
    assert not ctx.to_host(d_H, (3, 36)).any() and not ctx.to_host(d_b, (3, 6)).any() and ctx.to_host(d_chi, 1)[0] == -7.0
    run.close()


def test_point_index_check_sees_an_edge_beyond_the_first_grid_stride_trip(ctx):
    lay = gd.index_check_layout("point")
    pose = lay["e"]["pose"].astype(np.int32).copy()
    i = 1024 * 256 + 300
    assert i < len(pose) and pose[i] != 0
    pose[i] = 0                                             # outside its pose's range; every edge before it is in place
    run = GicpRunner(ctx, lay, pose_override=pose)
    H, b, chi = run.build(rc=-3)
    assert not H.any() and not b.any() and chi == -7.0      # refused: nothing written
    d_chi = ctx.to_dev(np.array([-7.0, 0.0]))
    assert cugo.lib().cugo_gicp_compute_errors(ctx.h, C.byref(run.ev), run.d_poses, d_chi, None) == -3
    assert ctx.to_host(d_chi, 1)[0] == -7.0


@pytest.mark.parametrize("what", ["n_cov_0", "n_cov_2", "n_cov_n_minus_1", "null_cov_p", "null_cov_z", "null_p", "null_z", "rk_4", "delta_0"])
def test_point_bad_arguments_are_refused_before_any_launch(ctx, what):
    lay = gd.point_layout("C_one")
    run = GicpRunner(ctx, lay)
    ev = run.ev
    if what.startswith("n_cov"):
        ev.n_cov = {"n_cov_0": 0, "n_cov_2": 2, "n_cov_n_minus_1": ev.n - 1}[what]
    elif what.startswith("null_"):
        setattr(ev, "d_" + what[5:], None)
    elif what == "rk_4":
        ev.rk = 4
    else:
        ev.rk, ev.delta = 1, 0.0
    H, b, chi = run.build(rc=-3)
    assert not H.any() and not b.any() and chi == -7.0
    d_chi, d_edge = ctx.to_dev(np.array([-7.0, 0.0])), ctx.to_dev(np.full(ev.n, -3.0))
    assert cugo.lib().cugo_gicp_compute_errors(ctx.h, C.byref(ev), run.d_poses, d_chi, d_edge) == -3
    assert ctx.to_host(d_chi, 1)[0] == -7.0 and np.all(ctx.to_host(d_edge, ev.n) == -3.0)
    rowptr, B = pd.schur_rows(lay["n_free"])
    d_H, d_bp, d_bsc = ctx.to_dev(np.zeros((B, 36))), ctx.to_dev(np.zeros((lay["n_free"], 6))), ctx.to_dev(np.zeros((lay["n_free"], 6)))
    assert cugo.lib().cugo_gicp_construct_quadratic_form_schur(ctx.h, C.byref(ev), run.d_poses, ctx.to_dev(rowptr), d_H, d_bp, d_bsc,
                                                               d_chi) == -3
    assert not ctx.to_host(d_H, (B, 36)).any() and not ctx.to_host(d_bp, (lay["n_free"], 6)).any()


@pytest.mark.parametrize("what", ["n_cov_0", "n_cov_2", "null_cov_p", "null_cov_z", "null_pose_a", "rk_4", "delta_0", "other_n", "no_plan"])
def test_pair_bad_arguments_are_refused_before_any_launch(ctx, what):
    lay, ref = gd.pair_layout("B_gicp"), pair_reference("B_gicp")
    run = PairRunner(ctx, lay, ref)
    ev = run.ev
    if what.startswith("n_cov"):
        ev.n_cov = {"n_cov_0": 0, "n_cov_2": 2}[what]
    elif what.startswith("null_"):
        setattr(ev, "d_" + what[5:], None)
    elif what == "rk_4":
        ev.rk = 4
    elif what == "delta_0":
        ev.rk, ev.delta = 1, 0.0
    elif what == "other_n":
        ev.n -= 1
    else:
        ev.plan = None
    Pall, nnzb = run.Pall, run.nnzb
    d_H, d_b, d_Hoff, d_bsc = (ctx.to_dev(np.zeros(s)) for s in ((Pall, 36), (Pall, 6), (nnzb, 36), (Pall, 6)))
    d_chi, d_edge = ctx.to_dev(np.array([-7.0, 0.0])), ctx.to_dev(np.full(run.E, -3.0))
    lib = cugo.lib()
    assert lib.cugo_gicp_pair_construct_quadratic_form(ctx.h, C.byref(ev), run.d_poses, d_H, d_b, d_Hoff, d_chi) == -3
    assert lib.cugo_gicp_pair_construct_quadratic_form_diag(ctx.h, C.byref(ev), run.d_poses, d_H, d_b, d_chi) == -3
    assert lib.cugo_gicp_pair_construct_quadratic_form_schur(ctx.h, C.byref(ev), run.d_poses, run.d_rowptr, d_Hoff, d_b, d_bsc, d_chi) == -3
    assert lib.cugo_gicp_pair_compute_errors(ctx.h, C.byref(ev), run.d_poses, d_chi, d_edge) == -3
    assert lib.cugo_gicp_pair_add_offdiag_schur(ctx.h, C.byref(ev), d_Hoff) == -3
    assert not ctx.to_host(d_H, (Pall, 36)).any() and not ctx.to_host(d_b, (Pall, 6)).any() and not ctx.to_host(d_Hoff, (nnzb, 36)).any()
    assert ctx.to_host(d_chi, 1)[0] == -7.0 and np.all(ctx.to_host(d_edge, run.E) == -3.0)
    run.close()


def test_offdiag_pass_before_any_build_pass_is_refused(ctx):
    lay = gd.pair_layout("B_gicp")
    run = PairRunner(ctx, lay, pair_reference("B_gicp"))
    d_H = ctx.to_dev(np.zeros((run.nnzb, 36)))
    assert cugo.lib().cugo_gicp_pair_add_offdiag_schur(ctx.h, C.byref(run.ev), d_H) == -3
    run.errors()                                            # (an error pass leaves no partials either)
    assert cugo.lib().cugo_gicp_pair_add_offdiag_schur(ctx.h, C.byref(run.ev), d_H) == -3
    assert not ctx.to_host(d_H, (run.nnzb, 36)).any()
    run.build_diag()
    assert run.add_offdiag().any()
    run.close()
