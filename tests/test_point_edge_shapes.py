"""The point-to-point pose edge kernels (point_kernels.hip) on the designed layouts of tests/point_designed.py, through
the kernel-level C ABI (cugo_point_*), against the extended-precision reference of tests/point_edge_ref.py with its
per-entry bounds (test_point_edge_ref_host.py pins both on the CPU).

For every layout and Omega class: H (both triangles, exactly symmetric), b, the chi2 total and the error pass's chi2 per
edge inside the bounds; error-pass chi2 bit-equal to the build pass's; a second run bit-equal; fixed and inactive edges
exactly 0; with a random prefill the poses without a counting edge keep their bits.  The Schur destination with
rowptr[p] != p (pose_designed.schur_rows) is bit-equal to what the plain form adds.  The two equivalences on the device:
Omega = omega n n^T is the plane edge, Omega = omega (I - u u^T) the line edge, against cugo_icp_* results to the summed
bounds.  The index check beyond its first grid-stride trip; a null array or a bad n_info refused before any launch."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import pose_designed as pd
import pose_edge_ref as per
import point_designed as pt
import point_edge_ref as ptr_ref
from test_pose_edge_shapes import Runner, blocks, check_all, schur_checks, icp_runner

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
    lay = pt.layout(name)
    return ptr_ref.point_build(lay["poses"], lay["n_free"], lay["e"], full=name != "G")


def upload(ctx, lay, flags="given", pose_override=None, e=None):
    e = lay["e"] if e is None else e
    ev = cugo.PointEdges()
    ev.n_poses_total, ev.n_poses_free, ev.n = lay["P"], lay["n_free"], len(e["pose"])
    pose = np.asarray(e["pose"], np.int32)
    ev.d_pose_ptr = ctx.to_dev(pd.pose_ptr(pose, lay["P"]))
    ev.d_pose = ctx.to_dev(pose if pose_override is None else pose_override)
    p, z, info = pt.device_arrays(e)
    ev.d_p, ev.d_z, ev.d_info, ev.n_info = ctx.to_dev(p), ctx.to_dev(z), ctx.to_dev(info), info.shape[1]
    if flags == "given" and e.get("flags") is not None:
        ev.d_flags = ctx.to_dev(e["flags"])
    elif flags == "zeros":
        ev.d_flags = ctx.to_dev(np.zeros(ev.n, np.uint8))
    ev.rk, ev.delta = e["rk"]
    return ev


class PointRunner(Runner):
    def __init__(self, ctx, lay, **kw):
        self.ctx, self.ev, self.P, self.E = ctx, upload(ctx, lay, **kw), lay["n_free"], len((kw.get("e") or lay["e"])["pose"])
        self.d_poses = ctx.to_dev(lay["poses"])
        lib = cugo.lib()
        self.f_build, self.f_err = lib.cugo_point_construct_quadratic_form, lib.cugo_point_compute_errors
        self.f_schur = cugo.point_construct_quadratic_form_schur


# ------------------------------------------------------------------ every layout and Omega class
@pytest.mark.parametrize("name", [n for n in pt.NAMES if n != "C0"] + ["F"])
def test_point_layout(ctx, name):
    lay = pt.layout(name)
    out = check_all("point " + name, PointRunner(ctx, lay), reference(name), ptr_ref.point_bound, pt.counting(lay))
    if name == "D_zero":
        assert not out["H"].any() and not out["b"].any() and out["chi"] == 0.0


def test_point_without_free_poses_touches_nothing(ctx):
    lay = pt.layout("C0")
    run = PointRunner(ctx, lay)
    rng = np.random.default_rng(6)
    H0, b0 = rng.normal(size=(lay["P"], 36)), rng.normal(size=(lay["P"], 6))
    H, b, chi = run.build(H0, b0, all_rows=True)
    assert np.array_equal(H, blocks(H0, lay["P"])) and np.array_equal(b, b0) and chi == 0.0
    chi_e, edge = run.errors()
    assert chi_e == 0.0 and not edge.any()


def test_point_error_pass_on_513_chunks(ctx):
    """G: 262 656 edges, 513 chunk totals (three trips of the totals' sum); the sorted layout beyond the first trip of the
    index check is accepted"""
    lay = pt.layout("G")
    check_all("point G", PointRunner(ctx, lay), reference("G"), ptr_ref.point_bound, pt.counting(lay), keys=("chi", "chi_edge"))


@pytest.mark.parametrize("rk", pd.RKS)
def test_point_zero_residual(ctx, rk):
    """r exactly 0 in double: everything finite, chi2 and b exactly 0, H inside its bounds"""
    lay = pt.zero_residual(rk)
    ref = ptr_ref.point_build(lay["poses"], lay["n_free"], lay["e"])
    out = check_all("point zero rk %d" % rk[0], PointRunner(ctx, lay), ref, ptr_ref.point_bound, pt.counting(lay))
    assert out["chi"] == 0.0 and not out["chi_edge"].any() and not out["b"].any() and np.all(np.isfinite(out["H"])) and out["H"].any()


def test_null_flags_equal_zero_flags_and_one_matrix_equals_tiled(ctx):
    lay = pt.layout("A_one")
    a = PointRunner(ctx, lay, flags=None).build()
    b = PointRunner(ctx, lay, flags="zeros").build()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    tiled = dict(lay["e"], info6=np.tile(lay["e"]["info6"], (len(lay["e"]["pose"]), 1)))
    c = PointRunner(ctx, lay, e=tiled).build()
    assert all(np.array_equal(x, y) for x, y in zip(a, c)) and a[2] > 0
    ea, ec = PointRunner(ctx, lay).errors(), PointRunner(ctx, lay, e=tiled).errors()
    assert ea[0] == ec[0] == a[2] and np.array_equal(ea[1], ec[1])


# ------------------------------------------------------------------ the Schur destination
@pytest.mark.parametrize("name", ["A_spd", "B_rank1", "C_spd", "C2_one", "D_spd"])
def test_point_schur_destination(ctx, name):
    lay = pt.layout(name)
    schur_checks("point " + name, PointRunner(ctx, lay), lay["n_free"])


# ------------------------------------------------------------------ the two equivalences on the device
@pytest.mark.parametrize("kind,name", [("plane", "A_plane"), ("plane", "B_plane"), ("plane", "D_plane"), ("line", "A_line"),
                                       ("line", "B_line"), ("line", "D_line")])
def test_plane_and_line_edges_are_special_cases_on_the_device(ctx, kind, name):
    lay = (pt.from_plane if kind == "plane" else pt.from_line)(name)
    icp = lay["icp"]
    ref_p = ptr_ref.point_build(lay["poses"], lay["n_free"], lay["e"])
    ref_i = per.icp_build(icp["poses"], icp["n_free"], [(kind, icp[kind])])
    rp, ri = PointRunner(ctx, lay), icp_runner(ctx, icp)
    Hp, bp, chip = rp.build()
    Hi, bi, chii = ri.build()
    edge_p, edge_i = rp.errors()[1], ri.errors()[1]
    msg = []
    for k, a, b in (("H", Hp, Hi), ("b", bp, bi), ("chi", chip, chii), ("chi_edge", edge_p, edge_i)):
        bnd = ptr_ref.point_bound(ref_p, k) + per.icp_bound(ref_i, k)
        r = ptr_ref.ratio(a, b, bnd)
        msg.append("%s %.3g" % (k, r))
        assert r <= 1, (name, k, r)
    print("%s as point edges on the device: largest difference / summed bounds: %s" % (name, "  ".join(msg)))


# ------------------------------------------------------------------ refusals before any launch
def test_index_check_sees_an_edge_beyond_the_first_grid_stride_trip(ctx):
    lay = pt.layout("G")
    pose = lay["e"]["pose"].astype(np.int32).copy()
    i = 1024 * 256 + 300
    assert i < len(pose) and pose[i] != 0
    pose[i] = 0                                            # outside its pose's range; every edge before it is in place
    run = PointRunner(ctx, lay, pose_override=pose)
    H, b, chi = run.build(rc=-3)
    assert not H.any() and not b.any() and chi == -7.0     # refused: nothing written
    d_chi = ctx.to_dev(np.array([-7.0, 0.0]))
    assert cugo.lib().cugo_point_compute_errors(ctx.h, C.byref(run.ev), run.d_poses, d_chi, None) == -3
    assert ctx.to_host(d_chi, 1)[0] == -7.0


@pytest.mark.parametrize("what", ["n_info_0", "n_info_2", "n_info_n_minus_1", "null_info", "null_p", "null_z", "rk_4", "delta_0",
                                  "null_pose_ptr", "free_gt_total"])
def test_bad_arguments_are_refused_before_any_launch(ctx, what):
    lay = pt.layout("C2_one")
    run = PointRunner(ctx, lay)
    ev = run.ev
    if what.startswith("n_info"):
        ev.n_info = {"n_info_0": 0, "n_info_2": 2, "n_info_n_minus_1": ev.n - 1}[what]
    elif what.startswith("null_"):
        setattr(ev, "d_" + what[5:], None)
    elif what == "rk_4":
        ev.rk = 4
    elif what == "delta_0":
        ev.rk, ev.delta = 1, 0.0
    else:
        ev.n_poses_free = ev.n_poses_total + 1
    H, b, chi = run.build(rc=-3)
    assert not H.any() and not b.any() and chi == -7.0
    d_chi, d_edge = ctx.to_dev(np.array([-7.0, 0.0])), ctx.to_dev(np.full(ev.n, -3.0))
    assert cugo.lib().cugo_point_compute_errors(ctx.h, C.byref(ev), run.d_poses, d_chi, d_edge) == -3
    assert ctx.to_host(d_chi, 1)[0] == -7.0 and np.all(ctx.to_host(d_edge, ev.n) == -3.0)
    rowptr, B = pd.schur_rows(lay["n_free"])
    d_H, d_bp, d_bsc = ctx.to_dev(np.zeros((B, 36))), ctx.to_dev(np.zeros((lay["n_free"], 6))), ctx.to_dev(np.zeros((lay["n_free"], 6)))
    assert cugo.lib().cugo_point_construct_quadratic_form_schur(ctx.h, C.byref(ev), run.d_poses, ctx.to_dev(rowptr), d_H, d_bp, d_bsc,
                                                                d_chi) == -3
    assert not ctx.to_host(d_H, (B, 36)).any() and not ctx.to_host(d_bp, (lay["n_free"], 6)).any()
