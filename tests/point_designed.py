"""Designed layouts for the point-to-point pose edge kernels (point_kernels.hip): the pose degrees of pose_designed.py
(DEG_A, DEG_B, DEG_C, DEG_D, INACT_D: pose ranges ending at edges 63 / 64 / 65, 511 / 512 / 513 and 1023 / 1024, 64 different
poses in one 64-lane group, runs of edgeless poses, fixed poses, whole inactive chunks) under the classes of Omega the
term is built for.  Built programmatically with fixed seeds (numpy only); every layout carries the census of
pose_designed._census_kind plus what its Omega class is, which test_point_edge_ref_host.py asserts.

A set is the dict of point_edge_ref: pose [E] (ascending), p, z [E,3], info6 [E,6] or [1,6], active [E], flags [E] uint8, rk.
Omega classes: 'spd' per-edge symmetric positive definite with condition 1 .. 1e6; 'one' a single matrix for all edges;
'rank1' omega n n^T per edge; 'rank2' omega (I - u u^T) per edge; 'zero' the zero matrix (shared).

No layout but the two that need their edge COUNT has more than a few thousand edges: 'F' (256 x 512 + 1 edges: 257 chunk
totals, one more than a trip of the totals' sum) and 'G' (513 x 512 edges: 513 totals, and more edges than one
grid-stride trip of the index check covers, 1024 x 256) cannot be smaller."""
import functools

import numpy as np

import icp_ref
import pose_designed as pd
import point_edge_ref as ptr_ref
from pose_designed import DEG_A, DEG_B, DEG_C, DEG_C2, DEG_D, FREE_C, FREE_C2, INACT_D, CAUCHY, TUKEY, HUBER, NONE, CHUNK, INACTIVE

OMEGA_CLASSES = ("spd", "one", "rank1", "rank2", "zero")


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def make_info(rng, cls, E):
    """[E,6] or [1,6] packed upper triangles of the class, and the eigenvalues [*,3] they were built from"""
    if cls == "zero":
        return np.zeros((1, 6)), np.zeros((1, 3))
    n = 1 if cls == "one" else E
    if cls in ("spd", "one"):
        Q = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
        lam = rng.uniform(0.5, 3.0, n)[:, None] * 10.0 ** np.stack([np.zeros(n), rng.uniform(0, 6, n), np.full(n, 6.0) * (np.arange(n) % 3 == 0)], 1)
        Om = np.einsum("eik,ek,ejk->eij", Q, lam, Q)
    elif cls == "rank1":
        u, om = _unit(rng.normal(size=(n, 3))), rng.uniform(0.5, 3.0, n)
        Om, lam = om[:, None, None] * u[:, :, None] * u[:, None, :], np.stack([om, 0 * om, 0 * om], 1)
    else:
        u, om = _unit(rng.normal(size=(n, 3))), rng.uniform(0.5, 3.0, n)
        Om, lam = om[:, None, None] * (np.eye(3)[None] - u[:, :, None] * u[:, None, :]), np.stack([om, om, 0 * om], 1)
    return ptr_ref.pack(Om), lam


def _point(seed, deg, n_free, rk, cls, inactive=None, noise=0.3):
    rng = np.random.default_rng(seed)
    P = len(deg)
    poses = np.array([icp_ref.random_pose(rng) for _ in range(P)])
    pose = np.repeat(np.arange(P, dtype=np.int32), deg)
    E = len(pose)
    p = rng.normal(0, 2.0, (E, 3))
    y = np.einsum("eij,ej->ei", ptr_ref._rot(poses[pose, :4])[0], p) + poses[pose, 4:]
    z = y + rng.normal(0, noise, (E, 3))
    info6, lam = make_info(rng, cls, E)
    active = np.ones(E, bool)
    if inactive is not None:
        active[inactive] = False
    e = dict(pose=pose, p=p, z=z, info6=info6, active=active, flags=np.where(active, 0, INACTIVE).astype(np.uint8), rk=rk)
    n_free = P if n_free is None else n_free
    census = pd._census_kind(pose, n_free, active)
    census.update(omega_class=cls, n_info=len(info6), lam=lam)
    return dict(poses=poses, n_free=n_free, P=P, e=e, census=census)


LAYOUTS = {
    # name: (degrees, n_free, robust kernel, Omega class, inactive)
    "A_spd": (DEG_A, None, CAUCHY, "spd", None),
    "A_one": (DEG_A, None, HUBER, "one", None),
    "A_rank2": (DEG_A, None, TUKEY, "rank2", None),
    "B_spd": (DEG_B, None, NONE, "spd", None),
    "B_rank1": (DEG_B, None, TUKEY, "rank1", None),
    "B_one": (DEG_B, None, CAUCHY, "one", None),
    "C_spd": (DEG_C, FREE_C, HUBER, "spd", None),
    "C_rank2": (DEG_C, FREE_C, NONE, "rank2", None),
    "C2_one": (DEG_C2, FREE_C2, HUBER, "one", None),
    "C0": (DEG_C, 0, CAUCHY, "spd", None),                 # n_poses_free = 0
    "D_spd": (DEG_D, None, HUBER, "spd", INACT_D),
    "D_rank1": (DEG_D, None, CAUCHY, "rank1", INACT_D),
    "D_zero": (DEG_D, None, NONE, "zero", INACT_D),
}
NAMES = list(LAYOUTS)


@functools.lru_cache(maxsize=None)
def layout(name):
    if name in LAYOUTS:
        deg, nf, rk, cls, ina = LAYOUTS[name]
        return _point(500 + NAMES.index(name), deg, nf, rk, cls, ina)
    if name == "F":       # 256 x 512 + 1 edges: 257 chunk totals
        rng = np.random.default_rng(17)
        return _point(601, pd._degrees(rng, 256 * CHUNK + 1 - 512, 40) + [300, 212], 40, (1, 0.2), "one")
    if name == "G":       # 513 x 512 edges, the error pass only: 513 totals, more than 1024 x 256 edges
        rng = np.random.default_rng(18)
        return _point(602, pd._degrees(rng, 513 * CHUNK - 700, 30) + [400, 300], 30, HUBER, "one")
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def zero_residual(rk):
    """identity rotations, integer translations and points, z = y exactly, Omega with small integer entries (SPD): r and
    x are exactly 0 in double.  3 poses x 5 edges"""
    rng = np.random.default_rng(56)
    P = 3
    poses = np.zeros((P, 7))
    poses[:, 3] = 1.0
    poses[:, 4:] = rng.integers(-8, 9, (P, 3))
    pose = np.repeat(np.arange(P, dtype=np.int32), 5)
    E = len(pose)
    p = rng.integers(-9, 10, (E, 3)).astype(np.float64)
    A = rng.integers(-2, 3, (E, 3, 3)).astype(np.float64)
    Om = np.einsum("eik,ejk->eij", A, A) + np.eye(3)[None]
    e = dict(pose=pose, p=p, z=p + poses[pose, 4:], info6=ptr_ref.pack(Om), active=np.ones(E, bool), flags=np.zeros(E, np.uint8), rk=rk)
    return dict(poses=poses, n_free=P, P=P, e=e, census=pd._census_kind(pose, P, e["active"]))


@functools.lru_cache(maxsize=None)
def from_plane(name="A_plane"):
    """the plane kind of a pose_designed layout as point edges (Omega = omega n n^T, n.z = d), next to the layout"""
    lay = pd.icp_layout(name)
    return dict(poses=lay["poses"], n_free=lay["n_free"], P=lay["P"], e=ptr_ref.plane_as_point(lay["plane"]), icp=lay)


@functools.lru_cache(maxsize=None)
def from_line(name="A_line"):
    """the line kind of a pose_designed layout as point edges (Omega = omega (I - u u^T), z = a)"""
    lay = pd.icp_layout(name)
    return dict(poses=lay["poses"], n_free=lay["n_free"], P=lay["P"], e=ptr_ref.line_as_point(lay["line"]), icp=lay)


def device_arrays(e):
    """the planar arrays of cugo_point_edges: p [3][n], z [3][n], info [6][n_info]"""
    return (np.ascontiguousarray(np.asarray(e["p"], np.float64).T), np.ascontiguousarray(np.asarray(e["z"], np.float64).T),
            np.ascontiguousarray(np.asarray(e["info6"], np.float64).reshape(-1, 6).T))


def counting(lay):
    """the number of counting edges per free pose"""
    e, nf = lay["e"], lay["n_free"]
    live = (e["pose"] < nf) & e["active"]
    return np.bincount(e["pose"][live], minlength=nf)[:nf]
