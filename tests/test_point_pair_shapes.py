"""The pose-pose point edge kernels (point_pair_kernels.hip) on the designed layouts of tests/pair_designed.py, through the
kernel-level C ABI (cugo_point_pair_*), against the extended-precision reference of tests/point_pair_ref.py with its
per-entry bounds (test_point_pair_ref_host.py pins both on the CPU).

For every layout: the error pass (chi2 total and per edge), the plain form with Hoff and the Schur form with rowptr[p] !=
p inside the bounds; H exactly symmetric; the build pass's chi2 bit-equal to the error pass's; a second run bit-equal;
with a random prefill the poses and blocks without a counting run, the diagonal blocks of Hoff and the rows of fixed
poses keep their bits, and what arrives is ADDED; _diag + add_offdiag_schur give the bits of the Schur form, with an
error pass at other poses in between; a relative-pose set on the same pairs adds into the same blocks in either order of
the two calls; the index check beyond its first grid-stride trip; refusals before any launch."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import pair_designed as pdz
import point_pair_ref as ppr
import pose_edge_ref as per
import relpose_ref as RR

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


@functools.lru_cache(maxsize=None)
def reference(name):
    lay = pdz.layout(name)
    return ppr.pair_build(lay["poses"], lay["n_free"], lay["P"], lay["e"])


def blocks(a, n):
    """[n][36] column-major device blocks -> [n, 6, 6] matrices"""
    return np.asarray(a).reshape(n, 6, 6).transpose(0, 2, 1)


def pattern_of(lay, ref):
    """the pairs of the set plus, where there is room, two blocks no run maps to"""
    P = lay["n_free"]
    have = set(zip(ref["pair_lo"].tolist(), ref["pair_hi"].tolist()))
    extra = [(l, h) for l, h in ((0, P - 1), (1, P - 2)) if l < h and (l, h) not in have]
    return ppr.pair_pattern(P, ref["pair_lo"], ref["pair_hi"], extra)


class Runner:
    """one uploaded set in its plan's order and the passes over it"""

    def __init__(self, ctx, lay, ref, e=None, flags="given", pose_a_override=None):
        e = lay["e"] if e is None else e
        self.ctx, self.P, self.Pall, self.E = ctx, lay["n_free"], lay["P"], len(e["a"])
        self.rowptr, self.colind = pattern_of(lay, ref)
        self.nnzb = len(self.colind)
        self.plan = cugo.PointPairPlan(ctx.h, self.Pall, self.P, e["a"], e["b"], e.get("flags"), self.rowptr, self.colind)
        self.perm = self.plan.array("perm")
        self.blk_id = self.plan.array("blk_id")
        pa, pb, p, z, info, fl = pdz.device_arrays(e, self.perm)
        ev = cugo.PointPairEdges()
        ev.n_poses_total, ev.n_poses_free, ev.n = self.Pall, self.P, self.E
        ev.d_pose_a, ev.d_pose_b = ctx.to_dev(pa if pose_a_override is None else pose_a_override), ctx.to_dev(pb)
        ev.d_p, ev.d_z, ev.d_info, ev.n_info = ctx.to_dev(p), ctx.to_dev(z), ctx.to_dev(info), info.shape[1]
        if flags == "given" and fl is not None:
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

    def errors(self, d_poses=None):
        """chi2 total and the term of every edge in the CALLER's order"""
        d_chi, d_edge = self.ctx.to_dev(np.array([-7.0, 0.0])), self.ctx.to_dev(np.full(self.E, -3.0))
        cugo.point_pair_compute_errors(self.ctx.h, self.ev, self.d_poses if d_poses is None else d_poses, d_chi, d_edge)
        edge = np.zeros(self.E)
        edge[self.perm] = self.ctx.to_host(d_edge, self.E)
        return self.ctx.to_host(d_chi, 1)[0], edge

    def build(self, H0=None, b0=None, Hoff0=None):
        """plain form -> H [Pall,6,6], b [Pall,6] (Pall rows: the rows of fixed poses must keep their bits), Hoff, chi"""
        d_H, d_b, d_Hoff = self._dev(H0, (self.Pall, 36)), self._dev(b0, (self.Pall, 6)), self._dev(Hoff0, (self.nnzb, 36))
        d_chi = self.ctx.to_dev(np.array([-7.0, 0.0]))
        cugo.point_pair_construct_quadratic_form(self.ctx.h, self.ev, self.d_poses, d_H, d_b, d_Hoff, d_chi)
        return (blocks(self.ctx.to_host(d_H, (self.Pall, 36)), self.Pall), self.ctx.to_host(d_b, (self.Pall, 6)),
                blocks(self.ctx.to_host(d_Hoff, (self.nnzb, 36)), self.nnzb), self.ctx.to_host(d_chi, 1)[0])

    def build_diag(self, H0=None, b0=None):
        d_H, d_b, d_chi = self._dev(H0, (self.Pall, 36)), self._dev(b0, (self.Pall, 6)), self.ctx.to_dev(np.array([-7.0, 0.0]))
        cugo.point_pair_construct_quadratic_form_diag(self.ctx.h, self.ev, self.d_poses, d_H, d_b, d_chi)
        return blocks(self.ctx.to_host(d_H, (self.Pall, 36)), self.Pall), self.ctx.to_host(d_b, (self.Pall, 6)), self.ctx.to_host(d_chi, 1)[0]

    def add_offdiag(self, Hsc0=None):
        d_H = self._dev(Hsc0, (self.nnzb, 36))
        cugo.point_pair_add_offdiag_schur(self.ctx.h, self.ev, d_H)
        return blocks(self.ctx.to_host(d_H, (self.nnzb, 36)), self.nnzb)

    def schur(self, Hsc0=None, bp0=None, bsc0=None):
        d_H, d_bp, d_bsc = self._dev(Hsc0, (self.nnzb, 36)), self._dev(bp0, (self.Pall, 6)), self._dev(bsc0, (self.Pall, 6))
        d_chi = self.ctx.to_dev(np.array([-7.0, 0.0]))
        cugo.point_pair_construct_quadratic_form_schur(self.ctx.h, self.ev, self.d_poses, self.d_rowptr, d_H, d_bp, d_bsc, d_chi)
        return (blocks(self.ctx.to_host(d_H, (self.nnzb, 36)), self.nnzb), self.ctx.to_host(d_bp, (self.Pall, 6)),
                self.ctx.to_host(d_bsc, (self.Pall, 6)), self.ctx.to_host(d_chi, 1)[0])


def check_layout(tag, ctx, lay, ref):
    run = Runner(ctx, lay, ref)
    P, Pall, nnzb = run.P, run.Pall, run.nnzb
    diag, touched = run.rowptr[:P], run.blk_id
    assert len(touched) == len(ref["pair_lo"])
    untouched = np.setdiff1d(np.arange(nnzb), touched)          # the diagonal blocks and the blocks no run maps to
    idle = np.flatnonzero(np.asarray(ref["H_n"]).reshape(-1) == 0)   # poses without a counting run, the fixed ones among them
    assert set(range(P, Pall)) <= set(idle.tolist())
    # the error pass and the plain form
    chi_e, edge = run.errors()
    H, b, Hoff, chi = run.build()
    assert chi_e == chi, ("error-pass chi2 differs from the build pass's", chi_e, chi)
    assert np.array_equal(H, H.transpose(0, 2, 1)), "H not exactly symmetric"
    assert not Hoff[untouched].any() and not H[idle].any() and not b[idle].any()
    assert np.all(edge[np.asarray(ref["chi_edge_mass"]) == 0] == 0), "an edge that does not count has a chi2 term"
    msg = []
    for k, got in (("H", H), ("b", b), ("Hoff", Hoff[touched]), ("chi", chi), ("chi_edge", edge)):
        r = ppr.ratio(got, ref[k], ppr.pair_bound(ref, k))
        msg.append("%s %.3g" % (k, r))
        assert r <= 1, (tag, k, r)
    print("%s: largest error / bound: %s" % (tag, "  ".join(msg)))
    again = run.build()
    assert all(np.array_equal(x, y) for x, y in zip((H, b, Hoff, chi), again)), "a second run differs"
    chi_e2, edge2 = run.errors()
    assert chi_e2 == chi_e and np.array_equal(edge, edge2)
    # random prefill: what has no counting run keeps its bits, everything else receives the same term, ADDED
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
    rest = np.setdiff1d(untouched, diag)
    assert not Hs[rest].any()
    bp0, bsc0 = rng.normal(size=(Pall, 6)), 100 * rng.normal(size=(Pall, 6))
    Hs2, bp2, bsc2, _ = run.schur(Hoff0, bp0, bsc0)
    want = blocks(Hoff0, nnzb).copy()
    want[diag] += H[:P]
    want[touched] += Hoff[touched]
    assert np.array_equal(Hs2, want), "Hsc was not added to, block by block"
    assert np.array_equal(bp2, bp0 + b) and np.array_equal(bsc2, bsc0 + b)
    # the split: the diagonal pass, an error pass at OTHER poses, then the off-diagonal sums of the build pass's partials
    Hd, bd, chid = run.build_diag()
    assert np.array_equal(Hd, H) and np.array_equal(bd, b) and chid == chi
    other = lay["poses"].copy()
    other[:, 4:] += 0.25
    chi_o, _ = run.errors(ctx.to_dev(other))
    assert chi_o != chi or chi == 0.0
    Ho = run.add_offdiag(Hoff0)
    want = blocks(Hoff0, nnzb).copy()
    want[touched] += Hoff[touched]
    assert np.array_equal(Ho, want), "the error pass disturbed the partials, or the off-diagonal pass is not the Schur form's"
    run.close()
    return dict(H=H, b=b, Hoff=Hoff, chi=chi, chi_edge=edge)


@pytest.mark.parametrize("name", pdz.NAMES)
def test_pair_layout(ctx, name):
    lay = pdz.layout(name)
    out = check_layout("pair " + name, ctx, lay, reference(name))
    if name == "A_zero":
        assert not out["H"].any() and not out["b"].any() and not out["Hoff"].any() and out["chi"] == 0.0


@pytest.mark.parametrize("rk", [(0, 1.0), (1, 0.5), (2, 0.7), (3, 0.3)])
def test_pair_zero_residual(ctx, rk):
    """r exactly 0 in double: everything finite, chi2 and b exactly 0, H and Hoff inside their bounds"""
    lay = pdz.zero_residual(rk)
    ref = ppr.pair_build(lay["poses"], lay["n_free"], lay["P"], lay["e"])
    out = check_layout("pair zero rk %d" % rk[0], ctx, lay, ref)
    assert out["chi"] == 0.0 and not out["chi_edge"].any() and not out["b"].any()
    assert np.all(np.isfinite(out["H"])) and out["H"].any() and out["Hoff"].any()


def test_null_flags_equal_zero_flags_and_one_matrix_equals_tiled(ctx):
    lay = pdz.layout("A_one")
    e = dict(lay["e"], active=np.ones(len(lay["e"]["a"]), bool), flags=np.zeros(len(lay["e"]["a"]), np.uint8))
    ref = ppr.pair_build(lay["poses"], lay["n_free"], lay["P"], e)
    a = Runner(ctx, lay, ref, e=e).build()
    b = Runner(ctx, lay, ref, e=dict(e, flags=None)).build()
    c = Runner(ctx, lay, ref, e=dict(e, info6=np.tile(e["info6"], (len(e["a"]), 1)))).build()
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and all(np.array_equal(x, y) for x, y in zip(a, c)) and a[3] > 0


def test_run_time_flags_drop_edges_the_plan_kept(ctx):
    """the plan built with every edge active, the device given the flags: the bits of the set planned with its flags"""
    lay = pdz.layout("B")
    ref = reference("B")
    e = lay["e"]
    run = Runner(ctx, lay, ref)
    planned = run.build()
    rt = Runner(ctx, lay, ref, e=dict(e, flags=np.zeros(len(e["a"]), np.uint8)))
    rt.ev.d_flags = ctx.to_dev(np.asarray(e["flags"])[rt.perm])
    got = rt.build()
    assert all(np.array_equal(x, y) for x, y in zip(planned, got)) and (~e["active"]).any()


def test_a_relative_pose_set_on_the_same_pairs_adds_into_the_same_blocks_in_either_order(ctx):
    lay = pdz.layout("B")
    ref = reference("B")
    run = Runner(ctx, lay, ref)
    P, nnzb = run.P, run.nnzb
    rng = np.random.default_rng(12)
    pairs = [(int(l), int(h)) if k % 2 else (int(h), int(l)) for k, (l, h) in enumerate(zip(ref["pair_lo"], ref["pair_hi"]))]
    rp = RR.random_edges(rng, lay["poses"], pairs)
    ref_rp = per.relpose_build(lay["poses"], P, rp, run.rowptr, run.colind)
    ev_rp, plan_rp = RR.upload(ctx, lay["P"], P, rp, run.rowptr, run.colind)
    outs = []
    for order in ("pair first", "relpose first"):
        d_H, d_bp, d_bsc = ctx.to_dev(np.zeros((nnzb, 36))), ctx.to_dev(np.zeros((lay["P"], 6))), ctx.to_dev(np.zeros((lay["P"], 6)))
        calls = [lambda: cugo.point_pair_construct_quadratic_form_schur(ctx.h, run.ev, run.d_poses, run.d_rowptr, d_H, d_bp, d_bsc),
                 lambda: cugo.relpose_construct_quadratic_form_schur(ctx.h, ev_rp, run.d_poses, run.d_rowptr, d_H, d_bp, d_bsc)]
        for f in (calls if order == "pair first" else calls[::-1]):
            f()
        outs.append((blocks(ctx.to_host(d_H, (nnzb, 36)), nnzb), ctx.to_host(d_bp, (lay["P"], 6))[:P]))
    diag, touched = run.rowptr[:P], run.blk_id
    for Hs, bp in outs:
        for k, got, want, bnd in (
                ("H", Hs[diag], ref["H"][:P] + ref_rp["H"], ppr.pair_bound(ref, "H")[:P] + per.relpose_bound(ref_rp, "H")),
                ("b", bp, ref["b"][:P] + ref_rp["b"], ppr.pair_bound(ref, "b")[:P] + per.relpose_bound(ref_rp, "b")),
                ("Hoff", Hs[touched], ref["Hoff"] + ref_rp["Hoff"][touched],
                 ppr.pair_bound(ref, "Hoff") + per.relpose_bound(ref_rp, "Hoff")[touched])):
            r = ppr.ratio(got, want, bnd)
            assert r <= 1, (k, r)
            assert np.abs(np.asarray(ref_rp[k], np.float64)).sum() > 0
    plan_rp.close()
    run.close()


def test_index_check_sees_an_edge_beyond_the_first_grid_stride_trip(ctx):
    lay = pdz.layout("G")
    e = lay["e"]
    ref = dict(pair_lo=np.array([0]), pair_hi=np.array([1]))
    pose_a = np.asarray(e["a"], np.int32).copy()
    i = 1024 * 256 + 300
    assert i < len(pose_a) and pose_a[i] == 0
    pose_a[i] = 1                                           # not the a of its run; every edge before it is in place
    run = Runner(ctx, lay, ref, pose_a_override=pose_a)
    assert np.array_equal(run.perm, np.arange(len(pose_a)))
    d_H, d_b, d_Hoff = ctx.to_dev(np.zeros((3, 36))), ctx.to_dev(np.zeros((3, 6))), ctx.to_dev(np.zeros((run.nnzb, 36)))
    d_chi = ctx.to_dev(np.array([-7.0, 0.0]))
    lib = cugo.lib()
    assert lib.cugo_point_pair_construct_quadratic_form(ctx.h, C.byref(run.ev), run.d_poses, d_H, d_b, d_Hoff, d_chi) == -3
    assert lib.cugo_point_pair_compute_errors(ctx.h, C.byref(run.ev), run.d_poses, d_chi, None) == -3
    assert not ctx.to_host(d_H, (3, 36)).any() and not ctx.to_host(d_b, (3, 6)).any() and ctx.to_host(d_chi, 1)[0] == -7.0
    good = Runner(ctx, lay, ref)                            # the layout in place is accepted
    chi, edge = good.errors()
    assert chi > 0 and np.all(edge > 0)
    run.close()
    good.close()


@pytest.mark.parametrize("what", ["n_info_0", "n_info_2", "null_info", "null_p", "null_z", "null_pose_a", "null_pose_b", "rk_4", "delta_0",
                                  "other_n", "host_only_plan", "plan_without_pattern", "no_plan"])
def test_bad_arguments_are_refused_before_any_launch(ctx, what):
    lay = pdz.layout("B")
    ref = reference("B")
    run = Runner(ctx, lay, ref)
    ev = run.ev
    keep = None
    if what.startswith("n_info"):
        ev.n_info = {"n_info_0": 0, "n_info_2": 2}[what]
    elif what.startswith("null_"):
        setattr(ev, "d_" + what[5:], None)
    elif what == "rk_4":
        ev.rk = 4
    elif what == "delta_0":
        ev.rk, ev.delta = 1, 0.0
    elif what == "other_n":
        ev.n -= 1
    elif what == "no_plan":
        ev.plan = None
    else:
        e = lay["e"]
        pat = (None, None) if what == "plan_without_pattern" else (run.rowptr, run.colind)
        keep = cugo.PointPairPlan(None if what == "host_only_plan" else ctx.h, lay["P"], lay["n_free"], e["a"], e["b"], e["flags"], *pat)
        ev.plan = keep.handle
    Pall, nnzb = run.Pall, run.nnzb
    d_H, d_b, d_Hoff, d_bsc = (ctx.to_dev(np.zeros(s)) for s in ((Pall, 36), (Pall, 6), (nnzb, 36), (Pall, 6)))
    d_chi, d_edge = ctx.to_dev(np.array([-7.0, 0.0])), ctx.to_dev(np.full(run.E, -3.0))
    lib = cugo.lib()
    assert lib.cugo_point_pair_construct_quadratic_form(ctx.h, C.byref(ev), run.d_poses, d_H, d_b, d_Hoff, d_chi) == -3
    assert lib.cugo_point_pair_construct_quadratic_form_diag(ctx.h, C.byref(ev), run.d_poses, d_H, d_b, d_chi) == -3
    assert lib.cugo_point_pair_construct_quadratic_form_schur(ctx.h, C.byref(ev), run.d_poses, run.d_rowptr, d_Hoff, d_b, d_bsc, d_chi) == -3
    assert lib.cugo_point_pair_compute_errors(ctx.h, C.byref(ev), run.d_poses, d_chi, d_edge) == -3
    assert not ctx.to_host(d_H, (Pall, 36)).any() and not ctx.to_host(d_b, (Pall, 6)).any() and not ctx.to_host(d_Hoff, (nnzb, 36)).any()
    assert ctx.to_host(d_chi, 1)[0] == -7.0 and np.all(ctx.to_host(d_edge, run.E) == -3.0)
    if keep is not None:
        keep.close()
    run.close()


def test_offdiag_pass_before_any_build_pass_is_refused(ctx):
    lay = pdz.layout("B")
    run = Runner(ctx, lay, reference("B"))
    d_H = ctx.to_dev(np.zeros((run.nnzb, 36)))
    assert cugo.lib().cugo_point_pair_add_offdiag_schur(ctx.h, C.byref(run.ev), d_H) == -3
    run.errors()                                            # (an error pass leaves no partials either)
    assert cugo.lib().cugo_point_pair_add_offdiag_schur(ctx.h, C.byref(run.ev), d_H) == -3
    assert not ctx.to_host(d_H, (run.nnzb, 36)).any()
    run.build_diag()
    assert run.add_offdiag().any()
    run.close()
