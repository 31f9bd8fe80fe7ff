"""GPU tests of Graph.predict_observations against the dense inverse of the references' normal equations at the
optimiser's estimates, on the graphs of tests/test_rig_graph.py (8 x 60, three cameras with lever arms, mono and stereo,
robust kernels), tests/test_fisheye_graph.py (the 5 x 32 ring of four Kannala-Brandt cameras, Huber) and
tests/test_depth_graph.py (8 x 60, mono, stereo and depth edges).

After optimize(), EVERY (pose, landmark, camera-of-the-rig) triple is asked for, in every kind the graph's cameras have.
S is held to the graph-level rule of tests/test_pl_cov_graph.py, 1e-8 (|J_p Sigma_aa J_p^T|_F + |J_l Sigma_ll J_l^T|_F),
with the float64 Jacobians of tests/predict_ref.py.  Left out are only the triples of a pinhole camera with |Z_s| <= 0.1
and those of a Kannala-Brandt camera within 0.1 rad of the negative optical axis; at most 2 % of a case (measured at the
references' estimates on the CPU: rig 0.56 %, fisheye 1.56 %, depth 0 %).  Triples with Z_s <= 0 on fisheye cameras
are among those checked.
"""
import functools
import importlib

import numpy as np
import pytest

import fisheye_lm_ref as F
import predict_ref as P
import rig_lm_ref as G
import rig_ref
import test_depth_graph as tdg
import test_fisheye_graph as tfg
import test_rig_graph as trg
from test_covariance import golden

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
pytestmark = pytest.mark.gpu
CASES = ("rig", "fisheye", "depth")
IDENTITY7 = np.array([0, 0, 0, 1, 0, 0, 0.0])
PINHOLE5 = np.zeros(5)


def cameras_of(case, d):
    """the distinct cameras of the graph's edges: (cam5, sensor q_t7, model k5) each, and the kinds asked of them"""
    E = len(d["e_pose"])
    sensor = d["e_sensor"] if "e_sensor" in d else np.tile(IDENTITY7, (E, 1))
    model = d["e_model"] if "e_model" in d else np.tile(PINHOLE5, (E, 1))
    rows = np.unique(np.concatenate([d["e_cam"], sensor, model], 1), axis=0)
    if case == "depth":      # (every edge of that graph has a camera of its own: four of them, spread over the list)
        rows = rows[::max(1, len(rows) // 4)][:4]
    cams = [(r[:5].copy(), r[5:12].copy(), r[12:].copy()) for r in rows]
    return cams, {"rig": (2, 3), "fisheye": (2,), "depth": (2, 3, 4)}[case]


def triples(cams, P_, L_):
    a, l, c = np.meshgrid(np.arange(P_, dtype=np.int32), np.arange(L_, dtype=np.int32), np.arange(len(cams)), indexing="ij")
    a, l, c = a.reshape(-1), l.reshape(-1), c.reshape(-1)
    cam = np.array([cams[k][0] for k in c])
    sensor = np.array([cams[k][1] for k in c])
    model = np.array([cams[k][2] for k in c])
    tab = np.concatenate([np.array([rig_ref.quat_to_ext(s) for s in sensor]), model], 1)
    return a, l, c, cam, sensor, model, tab


def left_out(pose, lm, a, l, cam, tab):
    """(mask of the triples left out, Z_s, theta)"""
    Xs = P.project(pose[a], lm[l], cam, np.full(len(a), 2), tab, np.float64)["Xs"]
    th = np.arctan2(np.hypot(Xs[:, 0], Xs[:, 1]), Xs[:, 2])
    fish = tab[:, 16] != 0
    return np.where(fish, th > np.pi - 0.1, np.abs(Xs[:, 2]) <= 0.1), Xs[:, 2], th


def build(case):
    """(graph after optimize, problem dict, dense H^-1 at its estimates, offsets of the pose / landmark blocks (-1: fixed))"""
    if case == "rig":
        d, _ = trg.case("mixed")
        out = trg.run("mixed", keep=True)
        ref = G.RigGraph(d)
    elif case == "fisheye":
        d, _ = tfg.case("ring_huber")
        out = tfg.run("ring_huber", keep=True)
        ref = F.FisheyeGraph(d)
    else:
        d, kind, rk3, k, _ = tdg.case("mixed")
        out = tdg.run("mixed", keep=True)
        ref = tdg.DepthGraph(d, kind, rk3, k)
        d = dict(d, kind=kind)      # (test_depth_graph's kinds: 0 mono, 1 stereo, 2 depth)
    ref.pose[:], ref.lm[:] = out["pose"], out["lm"]
    H, _ = ref.normal_equations()
    inv = np.linalg.inv(H)
    ip = np.where(ref.pf, -1, 6 * ref.pidx)
    il = np.where(ref.lf, -1, 6 * ref.np_ + 3 * ref.lidx)
    return out["g"], d, inv, np.asarray(ip), np.asarray(il)


@pytest.fixture(scope="module")
def built():
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = build(case)
        return cache[case]
    yield get
    for v in cache.values():
        v[0].close()


def ref_blocks(inv, ip, il, a, l):
    n = len(a)
    Saa, Sal, Sll = np.zeros((n, 6, 6)), np.zeros((n, 6, 3)), np.zeros((n, 3, 3))
    for k in range(n):
        o, q = ip[a[k]], il[l[k]]
        if o >= 0:
            Saa[k] = inv[o:o + 6, o:o + 6]
        if q >= 0:
            Sll[k] = inv[q:q + 3, q:q + 3]
        if o >= 0 and q >= 0:
            Sal[k] = inv[o:o + 6, q:q + 3]
    return Saa, Sal, Sll


@pytest.mark.parametrize("case", CASES)
def test_every_triple_vs_dense_inverse(built, case):
    g, d, inv, ip, il = built(case)
    pose, lm = g.poses(), g.landmarks()
    cams, kinds = cameras_of(case, d)
    assert len(cams) >= (3 if case != "depth" else 1)
    a, l, c, cam, sensor, model, tab = triples(cams, len(ip), len(il))
    out, Zs, th = left_out(pose, lm, a, l, cam, tab)
    fish = tab[:, 16] != 0
    print("%s: %d cameras, %d triples, %d left out (%.2f %%); %d fisheye triples with Z_s <= 0 checked"
          % (case, len(cams), len(a), out.sum(), 100.0 * out.mean(), (fish & ~out & (Zs <= 0)).sum()))
    assert out.mean() <= 0.02
    if case == "fisheye":
        assert fish.all() and (~out & (Zs <= 0)).sum() >= 100
    keep = ~out
    a, l, c, cam, sensor, model, tab = (v[keep] for v in (a, l, c, cam, sensor, model, tab))
    n = len(a)
    Saa, Sal, Sll = ref_blocks(inv, ip, il, a, l)
    fp, fl = ip[a] >= 0, il[l] >= 0
    assert (~fp).any() and (fp & fl).any()
    for kind in kinds:
        dim = 2 if kind == 2 else 3
        z, S = g.predict_observations(a, l, kind=kind, cam=cam, sensor=sensor, model=model)
        assert z.shape == (n, dim) and S.shape == (n, dim, dim) and np.array_equal(S, S.transpose(0, 2, 1))
        z2, S2 = g.predict_observations(a, l, kind=kind, cam=cam, sensor=sensor, model=model)
        assert np.array_equal(z, z2) and np.array_equal(S, S2)
        p = P.project(pose[a], lm[l], cam, np.full(n, kind), tab, np.float64)
        JP, JL = p["JP"] * fp[:, None, None], p["JL"] * fl[:, None, None]
        Mp = np.einsum("nik,nkm,njm->nij", JP, Saa, JP)
        Ml = np.einsum("nik,nkm,njm->nij", JL, Sll, JL)
        X = np.einsum("nik,nkm,njm->nij", JP, Sal, JL)
        ref = (Mp + X + X.transpose(0, 2, 1) + Ml)[:, :dim, :dim]
        tol = 1e-8 * (np.linalg.norm(Mp, axis=(1, 2)) + np.linalg.norm(Ml, axis=(1, 2)))
        both = ~fp & ~fl
        assert not S[both].any()
        r = np.abs(S - ref).reshape(n, -1).max(1)[~both] / tol[~both]
        # z: the float64 projection of predict_ref differs from the longdouble one by less than the z bound
        pl = P.project(pose[a], lm[l], cam, np.full(n, kind), tab)
        rz = P.ratios(z, pl["z"][:, :dim], P.bound_z(pl)[:, :dim])
        print("%s kind %d: %d triples, worst |S - J Sigma J^T| = %.3g of the 1e-8 bound, worst z %.3g of its bound"
              % (case, kind, n, r.max(), rz.max()))
        assert r.max() <= 1, (case, kind, float(r.max()))
        assert rz.max() <= 1, (case, kind, float(rz.max()))
        if kind == 2:
            # the wrong camera is another answer: the old call's pinhole at the body origin misses by far more than the bound
            old = g.reprojection_covariances(a, l, dim=2, cam=cam)
            far = np.abs(old - ref).reshape(n, -1).max(1)[~both] / tol[~both]
            if case != "depth":
                assert np.median(far) > 1e3, float(np.median(far))
            else:
                assert np.array_equal(old, S)


@pytest.mark.parametrize("case", CASES)
def test_a_query_on_an_edge_gives_the_edges_residual(built, case):
    """for the (pose, landmark, camera) of every edge of the graph, z - measurement is the numpy reference's residual of
    that edge (the longdouble projection of predict_ref at the optimiser's estimates, unit weight on the depth row)
    within the z bound"""
    g, d, inv, ip, il = built(case)
    pose, lm = g.poses(), g.landmarks()
    E = len(d["e_pose"])
    sensor = d["e_sensor"] if "e_sensor" in d else np.tile(IDENTITY7, (E, 1))
    model = d["e_model"] if "e_model" in d else np.tile(PINHOLE5, (E, 1))
    kind = np.asarray(d["kind"]) + 2 if case == "depth" else np.where(np.asarray(d["e_stereo"]).astype(bool), 3, 2)
    tab = np.concatenate([np.array([rig_ref.quat_to_ext(s) for s in sensor]), model], 1)
    for k in sorted(set(kind.tolist())):
        sel = np.flatnonzero(kind == k)
        dim = 2 if k == 2 else 3
        a, l = d["e_pose"][sel].astype(np.int32), d["e_lm"][sel].astype(np.int32)
        z, _ = g.predict_observations(a, l, kind=k, cam=d["e_cam"][sel], sensor=sensor[sel], model=model[sel])
        p = P.project(pose[a], lm[l], d["e_cam"][sel], np.full(len(sel), k), tab[sel])
        meas = np.asarray(d["e_meas"], np.longdouble)[sel][:, :dim]
        e_ref = p["z"][:, :dim] - meas
        r = P.ratios(np.asarray(z, np.longdouble) - meas, e_ref, P.bound_z(p)[:, :dim])
        print("%s kind %d: %d edges, z - m off the reference's residual by %.3g of the z bound; |e| up to %.3g"
              % (case, k, len(sel), r.max(), float(np.abs(e_ref).max())))
        assert r.max() <= 1 and np.abs(e_ref[:, :2]).max() < 50


def test_the_sets_camera_is_what_cam_none_takes(built):
    """cam=None: the camera, sensor pose and model of the mono / stereo / depth set, bit for bit what passing them gives"""
    g, d, inv, ip, il = built("fisheye")
    cams, _ = cameras_of("fisheye", d)
    cam, sensor, model = cams[1]
    a, l = np.meshgrid(np.arange(len(ip), dtype=np.int32), np.arange(0, len(il), 3, dtype=np.int32), indexing="ij")
    a, l = a.reshape(-1), l.reshape(-1)
    g.set_camera(2, cam), g.set_sensor_pose(2, sensor), g.set_camera_model(2, 1, model[:4])
    z0, S0 = g.predict_observations(a, l)
    z1, S1 = g.predict_observations(a, l, kind=2, cam=cam, sensor=sensor, model=model)
    assert np.array_equal(z0, z1) and np.array_equal(S0, S1) and S0.any()
    z2, S2 = g.predict_observations(a, l, kind=2, cam=cam)           # (a pinhole at the body origin is another camera)
    assert not np.array_equal(S0, S2)
    with pytest.raises(cugo.CugoError, match="must be NULL"):
        g.predict_observations(a, l, kind=2, sensor=sensor)
    g, d, inv, ip, il = built("depth")
    cam = d["e_cam"][0]
    a, l = a[a < len(ip)], l[a < len(ip)]
    l = l % len(il)
    g.set_camera(3, cam), g.set_sensor_pose(3, cams[2][1]), g.set_depth_camera(cam * 1.01)
    z0, S0 = g.predict_observations(a, l, kind=3)
    z1, S1 = g.predict_observations(a, l, kind=3, cam=cam, sensor=cams[2][1])
    assert np.array_equal(z0, z1) and np.array_equal(S0, S1) and S0[:, 2, 2].any()
    z0, S0 = g.predict_observations(a, l, kind=4)
    z1, S1 = g.predict_observations(a, l, kind=4, cam=cam * 1.01)
    assert np.array_equal(z0, z1) and np.array_equal(S0, S1) and S0[:, 2, 2].any()
    # the set's inverse-depth weight (1e4 here) is the caller's noise term: the depth row of S is in measurement units
    assert np.allclose(z0[:, 2], 1.0 / P.project(g.poses()[a], g.landmarks()[l], np.tile(cam, (len(a), 1)), np.full(len(a), 4),
                                                 None, np.float64)["Xs"][:, 2], rtol=1e-12)


def test_on_a_plain_pinhole_graph_the_bits_of_reprojection_covariances():
    d, rk = golden("small_10x200")
    g = cugo.graph_from_arrays(d, rk=rk)
    g.initialize()
    g.optimize(5)
    P_, L_ = len(d["pose"]), len(d["lm"])
    a, l = np.meshgrid(np.arange(P_, dtype=np.int32), np.arange(L_, dtype=np.int32), indexing="ij")
    a, l = a.reshape(-1), l.reshape(-1)
    cam = np.asarray(d["e_cam"], np.float64).reshape(-1, 5)[0]
    for kind in (2, 3):
        z, S = g.predict_observations(a, l, kind=kind, cam=cam)
        old = g.reprojection_covariances(a, l, dim=kind, cam=cam)
        assert np.array_equal(S, old) and S.any(), kind
        z1, S1 = g.predict_observations(a, l, kind=kind, cam=cam, sensor=IDENTITY7, model=PINHOLE5)
        assert np.array_equal(S1, old) and np.array_equal(z1, z)
        g.set_camera(kind, cam)
        z2, S2 = g.predict_observations(a, l, kind=kind)
        assert np.array_equal(S2, old) and np.array_equal(z2, z)
    # both vertices fixed in every query: no system is built, S is zero, z is there
    fixed_p = np.flatnonzero(d["pose_fixed"])
    e = dict(d)
    e["lm_fixed"] = d["lm_fixed"].copy()
    e["lm_fixed"][:3] = 1
    h = cugo.graph_from_arrays(e, rk=rk)
    h.initialize()
    z, S = h.predict_observations(np.repeat(fixed_p[:1], 3), [0, 1, 2], kind=3, cam=cam)
    assert not S.any() and np.all(np.isfinite(z)) and z.all()
    zf, _ = h.predict_observations(np.repeat(fixed_p[:1], 3).tolist() + [1], [0, 1, 2, 5], kind=3, cam=cam)
    assert np.array_equal(zf[:3], z)
    h.close()
    g.close()


def test_refusals_and_a_landmark_without_an_edge():
    d = cugo.synth(20, 300, 1300, seed=6)
    cam = d["cam"]
    g = cugo.graph_from_arrays(d)
    with pytest.raises(cugo.CugoError, match="needs initialize"):
        g.predict_observations([1], [2], cam=cam)
    g.initialize()
    for bad in (([1], [300]), ([20], [2]), ([-1], [2])):
        with pytest.raises(cugo.CugoError, match="error -3"):
            g.predict_observations(*bad, cam=cam)
    for kind in (0, 1, 5):
        with pytest.raises(cugo.CugoError, match="predict_observations: kind must be 2"):
            g.predict_observations([1], [2], kind=kind, cam=cam)
    for q in ([0, 0, 0, 0, 0, 0, 0.0], [np.nan, 0, 0, 1, 0, 0, 0.0], [0, 0, 0, 1, np.inf, 0, 0.0]):
        with pytest.raises(cugo.CugoError, match=r"predictObservations\(\).*quaternion must be finite with a norm > 0"):
            g.predict_observations([1], [2], cam=cam, sensor=q)
    with pytest.raises(cugo.CugoError, match=r"predictObservations\(\).*coefficients k1..k4 must be finite"):
        g.predict_observations([1], [2], cam=cam, model=[0, np.nan, 0, 0, 1.0])
    with pytest.raises(cugo.CugoError, match="predict_observations: unknown model type"):
        g.predict_observations([1], [2], cam=cam, model=[0, 0, 0, 0, 2.0])
    for kind in (3, 4):
        with pytest.raises(cugo.CugoError, match=r"predictObservations\(\).*Kannala-Brandt camera has the rows \(u, v\) only"):
            g.predict_observations([1], [2], kind=kind, cam=cam, model=[0, 0, 0, 0, 1.0])
    with pytest.raises(ValueError):
        g.predict_observations([1, 2, 3], [2, 3, 4], cam=np.tile(cam, (2, 1)))      # neither one camera nor one per query
    z, S = g.predict_observations([1], [2], cam=cam, sensor=[0, 0, 0, 2.0, 0.1, 0, 0], model=[0.01, 0, 0, 0, 1.0])
    assert S.any() and z.shape == (1, 2)
    z, S = g.predict_observations([], [], cam=cam)
    assert z.shape == (0, 2) and S.shape == (0, 2, 2)
    g.close()
    f = cugo.graph_from_arrays(d)
    f.set_float32(1)
    f.initialize()
    with pytest.raises(cugo.CugoError, match="fp32-internal"):
        f.predict_observations([1], [2], cam=cam)
    f.close()
    s = cugo.graph_from_arrays(d)
    s.set_shard(0, 2, lambda ptr, n, op: None)       # (one shard of two; the exchange is never waited for)
    s.initialize()
    with pytest.raises(cugo.CugoError, match="predict_observations: not available on a sharded"):
        s.predict_observations([1], [2], cam=cam)
    s.close()
    # a free landmark without any edge: CUGO_ERR_NUMERIC when a query names it, and only then
    e = dict(d)
    e["lm"] = np.concatenate([d["lm"], d["lm"][:1] + 0.5])
    e["lm_fixed"] = np.concatenate([d["lm_fixed"], [0]]).astype(np.uint8)
    h = cugo.graph_from_arrays(e)
    h.initialize()
    h.optimize(3)
    with pytest.raises(cugo.CugoError, match="error -4"):
        h.predict_observations([1, 0], [2, 300], kind=4, cam=cam)
    z, S = h.predict_observations([1, 0], [2, 299], kind=4, cam=cam)
    assert S.any() and z.all()
    h.close()
