"""The relative-pose kernels (relpose_kernels.hip) on the designed layouts of tests/pose_designed.py (relpose_layout),
through the kernel-level C ABI, against the extended-precision reference of tests/pose_edge_ref.py (relpose_build) with
its per-entry bounds (test_relpose_ref_host.py pins both on the CPU).

For every layout: the diagonal blocks exactly symmetric; H, Hoff, b, the chi2 total and the error pass's chi2 per edge
inside the bounds; the error pass's chi2 bit-equal to the build pass's, and its per-edge terms summed in the device's
order bit-equal to both; a second run bit-equal; with a random prefill the poses without a counting edge, the blocks of
Hoff no counting edge maps to and its diagonal blocks keep their bits; edges that do not count have a chi2 term of
exactly 0.  The four destinations — Hpp + Hoff, the Schur form (through rowptr, rowptr[p] != p), the diag form with no
Hoff and add_offdiag onto a prefilled Hsc — agree bit for bit."""
import functools
import importlib

import numpy as np
import pytest

import pose_designed as pd
import pose_edge_ref as per
import prior_ref

pytestmark = pytest.mark.gpu

cugo = importlib.import_module("cuda-bundle-adjustment_amd")

KEYS = ("H", "Hoff", "b", "chi", "chi_edge")


@pytest.fixture(scope="module")
def ctx():
    import devmem
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    c = devmem.Ctx()
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def reference(name, full=True):
    lay = pd.relpose_layout(name)
    return per.relpose_build(lay["poses"], lay["n_free"], lay["rp"], lay["rowptr"], lay["colind"], full=full)


def blocks(a, n):
    """[n][36] column-major device blocks -> [n, 6, 6] matrices"""
    return np.asarray(a).reshape(n, 6, 6).transpose(0, 2, 1)


class Runner:
    """one uploaded relative-pose edge set (the plan built with the layout's plan flags, the device given its run-time
    flags) and the passes over it.  flags: 'given', 'zeros' or None (a null d_flags)"""

    def __init__(self, ctx, lay, rp=None, flags="given"):
        rp = lay["rp"] if rp is None else rp
        self.ctx, self.P, self.E, self.nnzb = ctx, lay["n_free"], len(rp["a"]), len(lay["colind"])
        self.rowptr = lay["rowptr"]
        self.plan = cugo.RelPosePlan(ctx.h, lay["P"], self.P, rp["a"], rp["b"], rp["flags"], lay["rowptr"], lay["colind"])
        ev = cugo.RelPoseEdges()
        ev.n_poses_total, ev.n_poses_free, ev.n = lay["P"], self.P, self.E
        ev.d_meas = ctx.to_dev(np.ascontiguousarray(np.asarray(rp["z"], np.float64).reshape(self.E, 7).T))
        info = prior_ref.pack_info(np.asarray(rp["info"], np.float64).reshape(-1, 6, 6))
        ev.d_info, ev.n_info = ctx.to_dev(np.ascontiguousarray(info.T)), len(info)
        if flags is not None:
            ev.d_flags = ctx.to_dev(rp["rt_flags"] if flags == "given" else np.zeros(self.E, np.uint8))
        ev.rk, ev.delta = rp["rk"]
        ev.plan = self.plan.handle
        self.ev = ev
        self.d_poses = ctx.to_dev(lay["poses"])
        self.d_rowptr = ctx.to_dev(lay["rowptr"])

    def close(self):
        self.plan.close()

    def _dev(self, a, shape):
        return self.ctx.to_dev(np.zeros(shape) if a is None else a)

    def errors(self):
        d_chi, d_edge = self.ctx.to_dev(np.array([-7.0, 0.0])), self.ctx.to_dev(np.full(self.E, -3.0))
        cugo.relpose_compute_errors(self.ctx.h, self.ev, self.d_poses, d_chi, d_edge)
        return self.ctx.to_host(d_chi, 1)[0], self.ctx.to_host(d_edge, self.E)

    def build(self, H0=None, b0=None, Hoff0=None):
        """Hpp + Hoff -> H [P,6,6], b [P,6], Hoff [nnzb,6,6], chi"""
        d_H, d_b, d_Hoff = self._dev(H0, (self.P, 36)), self._dev(b0, (self.P, 6)), self._dev(Hoff0, (self.nnzb, 36))
        d_chi = self.ctx.to_dev(np.array([-7.0, 0.0]))
        cugo.relpose_construct_quadratic_form(self.ctx.h, self.ev, self.d_poses, d_H, d_b, d_Hoff, d_chi)
        return (blocks(self.ctx.to_host(d_H, (self.P, 36)), self.P), self.ctx.to_host(d_b, (self.P, 6)),
                blocks(self.ctx.to_host(d_Hoff, (self.nnzb, 36)), self.nnzb), self.ctx.to_host(d_chi, 1)[0])

    def build_diag(self, H0=None, b0=None):
        d_H, d_b, d_chi = self._dev(H0, (self.P, 36)), self._dev(b0, (self.P, 6)), self.ctx.to_dev(np.array([-7.0, 0.0]))
        cugo.relpose_construct_quadratic_form_diag(self.ctx.h, self.ev, self.d_poses, d_H, d_b, d_chi)
        return blocks(self.ctx.to_host(d_H, (self.P, 36)), self.P), self.ctx.to_host(d_b, (self.P, 6)), self.ctx.to_host(d_chi, 1)[0]

    def add_offdiag(self, Hsc0):
        d_H = self.ctx.to_dev(Hsc0)
        cugo.relpose_add_offdiag_schur(self.ctx.h, self.ev, self.d_poses, d_H)
        return blocks(self.ctx.to_host(d_H, (self.nnzb, 36)), self.nnzb)

    def schur(self, Hsc0=None, bp0=None, bsc0=None):
        d_H, d_bp, d_bsc = self._dev(Hsc0, (self.nnzb, 36)), self._dev(bp0, (self.P, 6)), self._dev(bsc0, (self.P, 6))
        d_chi = self.ctx.to_dev(np.array([-7.0, 0.0]))
        cugo.relpose_construct_quadratic_form_schur(self.ctx.h, self.ev, self.d_poses, self.d_rowptr, d_H, d_bp, d_bsc, d_chi)
        return (blocks(self.ctx.to_host(d_H, (self.nnzb, 36)), self.nnzb), self.ctx.to_host(d_bp, (self.P, 6)),
                self.ctx.to_host(d_bsc, (self.P, 6)), self.ctx.to_host(d_chi, 1)[0])


def structure(lay, ref):
    """idle [P]: free poses without a counting edge; mapped [nnzb]: blocks a counting edge maps to; diag [P]"""
    idle = np.flatnonzero(np.asarray(ref["chi_pose_n"]) + np.asarray(ref["H_n"]).reshape(-1) == 0)
    mapped = np.asarray(ref["Hoff_n"]).reshape(-1) > 0
    return idle, mapped, np.asarray(lay["rowptr"][:-1])


def check_all_relpose(tag, run, ref, lay):
    P, nnzb = run.P, run.nnzb
    idle, mapped, diag = structure(lay, ref)
    assert not mapped[diag].any()
    live = ref["terms"]["live"]
    # ---- symmetry, pass agreement, repeatability
    chi_e, edge = run.errors()
    H, b, Hoff, chi = run.build()
    out = dict(H=H, b=b, Hoff=Hoff, chi=chi, chi_edge=edge)
    assert np.array_equal(H, H.transpose(0, 2, 1)), "a diagonal block is not exactly symmetric"
    assert chi_e == chi, ("error-pass chi2 differs from the build pass's", chi_e, chi)
    in_order = per.relpose_chi_in_device_order(edge, P, lay["rp"], lay["rowptr"], lay["colind"])
    assert in_order == chi, ("the error pass's per-edge terms do not sum to the build pass's chi2", in_order, chi)
    assert np.all(edge[~live] == 0), "an edge that does not count has a chi2 term"
    H2, b2, Hoff2, chi2 = run.build()
    chi_e2, edge2 = run.errors()
    assert np.array_equal(H, H2) and np.array_equal(b, b2) and np.array_equal(Hoff, Hoff2) and chi == chi2, "a second run differs"
    assert chi_e2 == chi_e and np.array_equal(edge, edge2)
    # ---- canaries
    rng = np.random.default_rng(5)
    H0, b0, Hoff0 = rng.normal(size=(P, 36)), rng.normal(size=(P, 6)), rng.normal(size=(nnzb, 36))
    H3, b3, Hoff3, chi3 = run.build(H0, b0, Hoff0)
    assert np.array_equal(H3[idle], blocks(H0, P)[idle]) and np.array_equal(b3[idle], b0[idle]) and chi3 == chi
    assert np.array_equal(Hoff3[~mapped], blocks(Hoff0, nnzb)[~mapped]), "a block no counting edge maps to changed"
    busy = np.setdiff1d(np.arange(P), idle)
    assert all(not np.array_equal(H3[p], blocks(H0, P)[p]) for p in busy if H[p].any())
    assert np.array_equal(H3, blocks(H0, P) + H) and np.array_equal(b3, b0 + b), "H and b did not receive one add of the walk's sum"
    # ---- destinations: the Schur form through rowptr
    assert P < 2 or (lay["rowptr"][1:P] != np.arange(1, P)).all()
    Hs, bp, bsc, chis = run.schur()
    assert np.array_equal(Hs[diag], H) and np.array_equal(bp, b) and np.array_equal(bsc, b) and chis == chi
    offd = np.ones(nnzb, bool)
    offd[diag] = False
    assert np.array_equal(Hs[offd], Hoff[offd]) and not Hoff[diag].any()
    Hsc0, bp0, bsc0 = rng.normal(size=(nnzb, 36)), rng.normal(size=(P, 6)), 100 * rng.normal(size=(P, 6))
    Hs4, bp4, bsc4, chis4 = run.schur(Hsc0, bp0, bsc0)
    assert np.array_equal(bp4, bp0 + b) and np.array_equal(bsc4, bsc0 + b) and chis4 == chi
    assert np.array_equal(Hs4[diag], blocks(Hsc0, nnzb)[diag] + H)
    assert np.array_equal(Hs4[offd & ~mapped], blocks(Hsc0, nnzb)[offd & ~mapped])
    assert np.array_equal(Hs4[offd], run.build(Hoff0=Hsc0)[2][offd])            # Hoff on the same prefill
    # ---- the diag form with no Hoff, then add_offdiag onto the same prefill
    Hd, bd, chid = run.build_diag()
    assert np.array_equal(Hd, H) and np.array_equal(bd, b) and chid == chi
    Ha = run.add_offdiag(Hsc0)
    assert np.array_equal(Ha[offd], Hs4[offd]), "add_offdiag differs from the Schur form's off-diagonal blocks"
    assert np.array_equal(Ha[diag], blocks(Hsc0, nnzb)[diag])
    # ---- bounds
    msg = []
    for k in KEYS:
        r = per.ratio(out[k], ref[k], per.relpose_bound(ref, k))
        msg.append("%s %.3g" % (k, r))
    print("relpose %s: largest error / bound: %s" % (tag, "  ".join(msg)))
    for k in KEYS:
        assert per.ratio(out[k], ref[k], per.relpose_bound(ref, k)) <= 1, (tag, k, msg)
    assert np.all(np.isfinite(H)) and np.all(np.isfinite(Hoff)) and np.all(np.isfinite(b)) and np.isfinite(chi)
    return out


@pytest.mark.parametrize("name", pd.RELPOSE_NAMES)
def test_relpose_layout(ctx, name):
    lay = pd.relpose_layout(name)
    run = Runner(ctx, lay)
    out = check_all_relpose(name, run, reference(name), lay)
    run.close()
    if name == "R-sides":        # what the layout is for, seen on the device
        idle = structure(lay, reference(name))[0]
        assert set(idle) == {pd.SIDES_EMPTY, pd.SIDES_PLAN_OFF, pd.SIDES_RT_OFF} and out["H"][pd.SIDES_ONE].any()
    if name == "R-info_indef":
        neg = np.asarray(reference(name)["terms"]["xr"], np.float64) < 0
        assert neg.any() and not out["chi_edge"][neg].any()


@pytest.mark.parametrize("k", range(4))
def test_relpose_zero_residual(ctx, k):
    """R-zero: r exactly 0 in double under every robust kernel: chi2 and b exactly 0, H and Hoff finite, inside their bounds
    and the bits of the layout without a robust kernel (w = rho'(0) = 1)"""
    name = "R-zero%d" % k
    lay = pd.relpose_layout(name)
    run = Runner(ctx, lay)
    out = check_all_relpose(name, run, reference(name), lay)
    run.close()
    assert out["chi"] == 0.0 and not out["chi_edge"].any() and not out["b"].any()
    assert np.all(np.isfinite(out["H"])) and out["H"].any() and out["Hoff"].any()
    plain = Runner(ctx, lay, rp=dict(lay["rp"], rk=(0, 1.0)))
    H, b, Hoff, chi = plain.build()
    plain.close()
    assert np.array_equal(H, out["H"]) and np.array_equal(Hoff, out["Hoff"]) and chi == 0.0


@pytest.mark.parametrize("nf", [1024, 1025, 1029])
def test_relpose_totals_beyond_one_trip_of_the_chi_total(ctx, nf):
    """256, 257 and 258 workgroup totals: one full trip of k_pose_chi_total, a second trip of one and of two"""
    name = "R-totals%d" % nf
    lay = pd.relpose_layout(name)
    ref = reference(name, full=False)
    run = Runner(ctx, lay)
    chi_e, edge = run.errors()
    H, b, Hoff, chi = run.build()
    chi_e2, edge2 = run.errors()
    H2, b2, Hoff2, chi2 = run.build()
    run.close()
    assert chi_e == chi and chi_e2 == chi_e and np.array_equal(edge, edge2)
    assert np.array_equal(H, H2) and np.array_equal(b, b2) and np.array_equal(Hoff, Hoff2) and chi == chi2
    assert per.relpose_chi_in_device_order(edge, nf, lay["rp"], lay["rowptr"], lay["colind"]) == chi
    r = {k: per.ratio(v, ref[k], per.relpose_bound(ref, k)) for k, v in (("chi", chi), ("chi_edge", edge))}
    print("relpose %s: largest error / bound: chi %.3g  chi_edge %.3g" % (name, r["chi"], r["chi_edge"]))
    assert r["chi"] <= 1 and r["chi_edge"] <= 1
    assert np.array_equal(H, H.transpose(0, 2, 1)) and np.all(np.isfinite(H))


def test_relpose_one_shared_information_matrix_equals_the_same_matrix_per_edge(ctx):
    lay = pd.relpose_layout("R-info_one")
    a, b = Runner(ctx, lay), Runner(ctx, lay, rp=pd.relpose_per_edge_info(lay["rp"]))
    assert a.ev.n_info == 1 and b.ev.n_info == b.E
    for x, y in zip(a.build() + a.errors(), b.build() + b.errors()):
        assert np.array_equal(x, y)
    assert a.build()[3] > 0
    a.close(), b.close()


def test_relpose_null_flags_equal_zero_flags(ctx):
    lay = pd.relpose_layout("R-wg9")
    assert lay["rp"]["active"].all()
    a, b = Runner(ctx, lay, flags=None), Runner(ctx, lay, flags="zeros")
    assert not a.ev.d_flags and b.ev.d_flags
    for x, y in zip(a.build() + a.errors() + a.schur(), b.build() + b.errors() + b.schur()):
        assert np.array_equal(x, y)
    assert a.build()[3] > 0
    a.close(), b.close()
