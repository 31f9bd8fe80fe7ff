"""CPU checks of tests/point_edge_ref.py and tests/point_designed.py (no GPU): they pin the extended-precision reference of
the point-to-point pose edges, its per-entry bounds and the designed layouts before test_point_edge_shapes.py holds the
kernels of point_kernels.hip against them.

* every layout's census: the boundaries, flush counts, chunk structure and Omega class it is built for;
* the known answer of the term, recomputed with fractions.Fraction;
* a plain float64 evaluation and the float64 replay of the device's chunk order lie inside the bounds on every layout;
* central differences: b against chi2, and H against b at r = 0, at hand-placed points;
* the two equivalences: Omega = omega n n^T, n.z = d is the plane edge of pose_edge_ref.icp_terms, Omega = omega (I - u u^T),
  z = a the line edge, each to the sum of the two references' own bounds;
* every mutation of the replay lands outside a bound.

Mutations, the layout that shows each and the factor over the bound there (x86-64, 80-bit longdouble):
  Omega read column-packed (02 <-> 11)     A_spd    H 2.6e19
  off-diagonals of Omega dropped            A_spd    H 2.9e11
  sign of [y]x                              A_spd    H 4.3e11
  p instead of y in the cross product       A_spd    H 1.9e11
  r = z - y with J unchanged                A_spd    b 2.2e10
  w applied twice                           A_spd    H 2.9e11   (Cauchy: w < 1)
  chi2 without Omega                        A_spd    chi 1.9e4
  the shared matrix indexed per edge        A_one    H 4.6e11
  a chunk's last edge dropped               A_spd    H 2.9e11
  a pose's second chunk dropped (finish)    A_one    H 5.3e6    (A_spd: 5.5e4)
Largest error / bound over the layouts, unmutated: plain float64 and replay alike H 0.066, b 0.014, chi 6.7e-6, chi per
edge 0.0024 (H, b and chi per edge on B_spd, no robust kernel; chi on C_rank2: the masses of the other layouts are dominated
by |Omega| |y|^2 under a kernel that flattens rho)."""
from fractions import Fraction as Fr

import numpy as np
import pytest

import icp_ref
import pose_designed as pd
import pose_edge_ref as per
import point_designed as pt
import point_edge_ref as ptr_ref

ALL = pt.NAMES + ["F"]
BOUNDARIES = {63, 64, 65, 511, 512, 513, 1023, 1024}


# ------------------------------------------------------------------ census
@pytest.mark.parametrize("name", ["A_spd", "A_one", "A_rank2"])
def test_layout_A_boundaries(name):
    lay = pt.layout(name)
    c, pose = lay["census"], lay["e"]["pose"]
    assert BOUNDARIES <= c["ends"]
    assert c["n"] == 6 * 512 + 1 and c["chunks"] == 7 and c["last_chunk"] == 1
    ptr = pd.pose_ptr(pose, lay["P"])
    deg = np.diff(ptr)
    assert deg[0] == 0 and deg[pose[511]] == 1 and deg[pose[512]] == 1 and pose[511] != pose[512]
    big = int(np.flatnonzero(deg == 1100)[0])
    assert ptr[big] % 512 != 0 and (ptr[big + 1] - 1) // 512 - ptr[big] // 512 == 2      # starts mid-chunk, three chunks
    runs = "".join("0" if d == 0 else "x" for d in deg[1:23])
    assert {len(r) for r in runs.split("x") if r} >= {1, 2, 5}                        # runs of edgeless poses
    assert set(range(c["slots"][0], c["slots"][-1] + 1)) - set(c["slots"])            # slots jump over them


@pytest.mark.parametrize("name", ["B_spd", "B_rank1", "B_one"])
def test_layout_B_many_poses_per_group(name):
    lay = pt.layout(name)
    c, pose = lay["census"], lay["e"]["pose"]
    assert c["max_flushes"] == 63 and len(np.unique(pose[448:512])) == 64


def test_layout_C_fixed_and_D_inactive():
    lay = pt.layout("C_spd")
    pose = lay["e"]["pose"]
    assert int(np.flatnonzero(pose >= lay["n_free"])[0]) == 180 and lay["census"]["chunks_all_fixed"] == [1, 2]
    assert int(np.flatnonzero(pt.layout("C2_one")["e"]["pose"] >= pd.FREE_C2)[0]) == 512
    assert pt.layout("C0")["n_free"] == 0
    for name in ("D_spd", "D_rank1", "D_zero"):
        lay = pt.layout(name)
        e = lay["e"]
        assert not e["active"][e["pose"] == 1].any() and not e["active"][512:576].any() and e["active"][576]
        assert lay["census"]["chunks_all_inactive"] == [2] and np.array_equal(e["flags"] != 0, ~e["active"])


def test_omega_classes():
    seen = set()
    for name in pt.NAMES:
        c = pt.layout(name)["census"]
        seen.add(c["omega_class"])
        Om = ptr_ref.unpack(pt.layout(name)["e"]["info6"])
        ev = np.linalg.eigvalsh(Om)
        assert np.all(ev[:, 0] >= -1e-12 * np.maximum(ev[:, 2], 1e-300)), name           # positive semi-definite
        if c["omega_class"] == "spd":
            cond = ev[:, 2] / ev[:, 0]
            assert c["n_info"] == c["n"] and cond.max() > 9e5 and cond.max() < 1.1e6 and cond.min() < 1e3
        if c["omega_class"] in ("one", "zero"):
            assert c["n_info"] == 1
        if c["omega_class"] == "rank1":
            assert np.all(ev[:, 1] < 1e-15 * 4) and np.all(ev[:, 2] > 0.4)
        if c["omega_class"] == "rank2":
            assert np.all(np.abs(ev[:, 0]) < 1e-15 * 4) and np.all(ev[:, 1] > 0.4)
        if c["omega_class"] == "zero":
            assert not Om.any()
    assert seen == set(pt.OMEGA_CLASSES)


def test_layouts_F_G_totals():
    f, g = pt.layout("F")["census"], pt.layout("G")["census"]
    assert f["n"] == 256 * 512 + 1 and f["chunks"] == 257 > pd.TOTALS
    assert g["n"] == 513 * 512 > 1024 * 256 and g["chunks"] == 513 > 2 * pd.TOTALS


@pytest.mark.parametrize("rk", pd.RKS)
def test_zero_residual_is_exact_and_finite(rk):
    lay = pt.zero_residual(rk)
    t = ptr_ref.point_terms(lay["poses"], lay["n_free"], lay["e"], np.float64)
    assert np.all(t["x"] == 0) and np.all(t["chi"] == 0) and np.all(t["b"] == 0) and np.all(np.isfinite(t["H"])) and t["H"].any()


# ------------------------------------------------------------------ the known answer
def test_known_answer_with_fractions():
    t, p, z = [Fr(1), Fr(2), Fr(3)], [Fr(1), Fr(0), Fr(0)], [Fr(3, 2), Fr(2), Fr(7, 2)]
    Om = [[Fr(4), Fr(1), Fr(0)], [Fr(1), Fr(1), Fr(0)], [Fr(0), Fr(0), Fr(2)]]
    y = [p[i] + t[i] for i in range(3)]                                  # the identity rotation
    r = [y[i] - z[i] for i in range(3)]
    q = [sum(Om[i][k] * r[k] for k in range(3)) for i in range(3)]
    chi = sum(r[i] * q[i] for i in range(3))
    S = [[Fr(0), y[2], -y[1]], [-y[2], Fr(0), y[0]], [y[1], -y[0], Fr(0)]]      # -[y]x
    J = [S[i] + [Fr(int(i == j)) for j in range(3)] for i in range(3)]
    H = [[sum(J[k][a] * Om[k][l] * J[l][c] for k in range(3) for l in range(3)) for c in range(6)] for a in range(6)]
    b = [-sum(J[k][a] * q[k] for k in range(3)) for a in range(6)]
    assert y == [2, 2, 3] and r == [Fr(1, 2), 0, Fr(-1, 2)] and q == [2, Fr(1, 2), -1] and chi == Fr(3, 2)
    assert b == [Fr(7, 2), -8, 3, -2, Fr(-1, 2), 1]
    yx = [[Fr(0), -y[2], y[1]], [y[2], Fr(0), -y[0]], [-y[1], y[0], Fr(0)]]      # [y]x
    assert [row[3:] for row in H[3:]] == Om
    assert [row[3:] for row in H[:3]] == [[sum(yx[i][k] * Om[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
    assert [row[:3] for row in H[:3]] == [[sum(yx[i][k] * Om[k][l] * yx[j][l] for k in range(3) for l in range(3)) for j in range(3)]
                                          for i in range(3)]
    e = dict(pose=np.array([0]), p=np.array([[1.0, 0, 0]]), z=np.array([[1.5, 2, 3.5]]), info6=np.array([[4.0, 1, 0, 1, 0, 2]]),
             active=np.array([True]), rk=(0, 1.0))
    poses = np.array([[0, 0, 0, 1.0, 1, 2, 3]])
    for dt in (np.float64, ptr_ref.LD):                                  # every number is a dyadic rational: exact in both
        got = ptr_ref.point_terms(poses, 1, e, dt)
        assert float(got["chi"][0]) == 1.5 and [float(v) for v in got["b"][0]] == [float(v) for v in b]
        assert np.array_equal(np.asarray(got["H"][0], np.float64), np.array([[float(v) for v in row] for row in H]))
    Hr, br, chir, _, _ = ptr_ref.point_replay(poses, 1, 1, e)
    assert chir == 1.5 and np.array_equal(br[0], [3.5, -8, 3, -2, -0.5, 1]) and np.array_equal(Hr[0], np.asarray(got["H"][0], np.float64))


# ------------------------------------------------------------------ float64 inside the bounds
@pytest.mark.parametrize("name", ALL)
def test_float64_and_replay_inside_the_bounds(name):
    lay = pt.layout(name)
    ref = ptr_ref.point_build(lay["poses"], lay["n_free"], lay["e"])
    plain = ptr_ref.point_build(lay["poses"], lay["n_free"], lay["e"], np.float64)
    H, b, chi, chi_edge, chi_pose = ptr_ref.point_replay(lay["poses"], lay["n_free"], lay["P"], lay["e"])
    assert np.array_equal(H, H.transpose(0, 2, 1))
    msg = []
    for k, got in (("H", H), ("b", b), ("chi", chi), ("chi_edge", chi_edge), ("chi_pose", chi_pose)):
        r1, r2 = ptr_ref.ratio(plain[k], ref[k], ptr_ref.point_bound(ref, k)), ptr_ref.ratio(got, ref[k], ptr_ref.point_bound(ref, k))
        msg.append("%s %.2g / %.2g" % (k, r1, r2))
        assert r1 <= 1 and r2 <= 1, (name, k, r1, r2)
    print("%s: largest error / bound, plain float64 / replay: %s" % (name, "  ".join(msg)))
    idle = pt.counting(lay) == 0
    assert not H[idle].any() and not b[idle].any()


def test_error_pass_layout_G_inside_the_bounds():
    lay = pt.layout("G")
    ref = ptr_ref.point_build(lay["poses"], lay["n_free"], lay["e"], full=False)
    plain = ptr_ref.point_build(lay["poses"], lay["n_free"], lay["e"], np.float64, full=False)
    for k in ("chi", "chi_edge"):
        assert ptr_ref.ratio(plain[k], ref[k], ptr_ref.point_bound(ref, k)) <= 1


# ------------------------------------------------------------------ mutations
MUTATIONS = [("col_packed", "A_spd", "H"), ("no_offdiag", "A_spd", "H"), ("skew_sign", "A_spd", "H"), ("p_for_y", "A_spd", "H"),
             ("r_flipped", "A_spd", "b"), ("w_twice", "A_spd", "H"), ("chi_no_info", "A_spd", "chi"), ("shared_per_edge", "A_one", "H"),
             ("drop_chunk_last", "A_spd", "H"), ("drop_second_chunk", "A_one", "H")]


@pytest.mark.parametrize("mut,name,key", MUTATIONS)
def test_mutation_lands_outside_the_bounds(mut, name, key):
    lay = pt.layout(name)
    ref = ptr_ref.point_build(lay["poses"], lay["n_free"], lay["e"])
    H, b, chi, _, _ = ptr_ref.point_replay(lay["poses"], lay["n_free"], lay["P"], lay["e"], mut=mut)
    r = ptr_ref.ratio(dict(H=H, b=b, chi=chi)[key], ref[key], ptr_ref.point_bound(ref, key))
    print("%s on %s: %s at %.3g x its bound" % (mut, name, key, r))
    assert r > 1e3, (mut, name, key, r)


def test_sensitivity_of_the_bound():
    """one edge on a pose, no robust kernel: H[3][3] = Omega_00 has the bound (1 + 50) u |Omega_00|, so a relative change of
    w by 1e-12 is seen 170 x over"""
    e = dict(pose=np.array([0]), p=np.array([[0.3, -1.2, 2.0]]), z=np.array([[1.0, 0.5, 2.5]]), info6=np.array([[2.0, 0.3, -0.1, 1.5, 0.2, 0.7]]),
             active=np.array([True]), rk=(0, 1.0))
    poses = np.array([icp_ref.random_pose(np.random.default_rng(3))])
    ref = ptr_ref.point_build(poses, 1, e)
    off = ptr_ref.point_terms(poses, 1, e, w_scale=1 + 1e-12)["H"][0]
    r = float(abs(off[3, 3] - ref["H"][0, 3, 3]) / ptr_ref.point_bound(ref, "H")[0, 3, 3])
    assert 100 < r < 250, r


# ------------------------------------------------------------------ central differences
def _one_edge(rk, z_is_y=False):
    pose = np.concatenate([[0.1, -0.2, 0.3, np.sqrt(1 - 0.14)], [0.5, -1.0, 2.0]])
    p = np.array([1.2, -0.7, 0.4])
    z = icp_ref.transform(pose, p) if z_is_y else np.array([0.9, -1.9, 2.2])
    e = dict(pose=np.array([0]), p=p[None], z=np.asarray(z)[None], info6=np.array([[3.0, 0.5, -0.4, 2.0, 0.3, 1.0]]),
             active=np.array([True]), rk=rk)
    return pose, e


@pytest.mark.parametrize("rk", pd.RKS)
def test_b_is_minus_half_the_gradient_of_chi2(rk):
    """central differences with h = 1e-5 under the left update: truncation h^2 x the third derivative (of the size of
    max|H| |y|, ~1e-9 here), rounding 2 u chi / h ~ 1e-11; 1e-7 max|b| leaves two orders"""
    pose, e = _one_edge(rk)
    t = ptr_ref.point_terms(pose[None], 1, e, np.float64)
    h = 1e-5
    for k in range(6):
        xi = np.zeros(6)
        xi[k] = h
        cp = ptr_ref.point_terms(icp_ref.left_update(pose, xi)[None], 1, e)["chi"][0]
        cm = ptr_ref.point_terms(icp_ref.left_update(pose, -xi)[None], 1, e)["chi"][0]
        assert abs(float((cp - cm) / (2 * h)) + 2 * t["b"][0, k]) <= 1e-7 * np.abs(t["b"]).max(), (k, rk)


def test_H_is_minus_the_derivative_of_b_at_zero_residual():
    """at r = 0 the Gauss-Newton H is the exact second derivative: d b / d xi = -H.  h = 1e-5: truncation h^2 x the third
    derivative ~1e-9 max|H|, rounding u max|b| / h = 0 at r = 0 up to u |y| |Omega| / h ~ 1e-10; 1e-7 max|H|"""
    pose, e = _one_edge((0, 1.0), z_is_y=True)
    H = ptr_ref.point_terms(pose[None], 1, e, np.float64)["H"][0]
    h = 1e-5
    for k in range(6):
        xi = np.zeros(6)
        xi[k] = h
        bp = ptr_ref.point_terms(icp_ref.left_update(pose, xi)[None], 1, e)["b"][0]
        bm = ptr_ref.point_terms(icp_ref.left_update(pose, -xi)[None], 1, e)["b"][0]
        assert np.abs(np.asarray((bp - bm) / (2 * h), np.float64) + H[:, k]).max() <= 1e-7 * np.abs(H).max(), k


# ------------------------------------------------------------------ the two equivalences
@pytest.mark.parametrize("kind,name", [("plane", "A_plane"), ("plane", "D_plane"), ("plane", "B_plane"), ("line", "A_line"),
                                       ("line", "B_line"), ("line", "D_line")])
def test_plane_and_line_edges_are_special_cases(kind, name):
    lay = (pt.from_plane if kind == "plane" else pt.from_line)(name)
    icp = lay["icp"]
    a = ptr_ref.point_build(lay["poses"], lay["n_free"], lay["e"])
    b = per.icp_build(icp["poses"], icp["n_free"], [(kind, icp[kind])])
    msg = []
    for k in ("H", "b", "chi", "chi_edge", "chi_pose"):
        r = ptr_ref.ratio(a[k], b[k], ptr_ref.point_bound(a, k) + per.icp_bound(b, k))
        msg.append("%s %.3g" % (k, r))
        assert r <= 1, (name, k, r)
    print("%s as point edges: largest difference / summed bounds: %s" % (name, "  ".join(msg)))
