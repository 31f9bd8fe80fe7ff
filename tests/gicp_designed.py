"""Designed layouts for the covariance form of the two point kinds (cugo_gicp_edges, cugo_gicp_pair_edges): the edge
layouts the information form is tested on (the run list of pair_designed.runs_A(), its ring 'B'; the degree lists of
point_designed / pose_designed: imported, not restated) with general rotations, under the covariance classes

    iso      sigma_p^2 I, sigma_z^2 I: Omega = I / (sigma_p^2 + sigma_z^2) in exact arithmetic, whatever the rotation
    gicp     eigenvalues (1, 1, 1e-3) times a scale in 0.5 .. 2, in random frames (the surface covariances of GICP)
    aligned  the thin directions of M C_p M^T and C_z coincide at the layout's poses, thin eigenvalue 1e-6: kappa(S) ~ 1e6
    zero_p   C_p = 0: Omega = C_z^-1, independent of the poses
    rank2_p  a planar C_p (eigenvalues 1, 1, 0 times a scale), a regular C_z
    one      one covariance pair for all edges (n_cov = 1), of class gicp

A set is the dict of tests/gicp_ref.py.  Nothing here has more than a few thousand edges: the chunk and run boundaries of
the shared reduction are held by the layouts themselves, which the information form's shape tests keep running on too.
Built programmatically with fixed seeds (numpy only); every layout carries its census, which test_gicp_ref_host.py
asserts."""
import functools

import numpy as np

import gicp_ref as gr
import pair_designed as pdz
import point_designed as pt
from pose_designed import DEG_A, DEG_B, DEG_C, DEG_D, FREE_C, INACT_D, CAUCHY, TUKEY, HUBER, NONE

CLASSES = ("iso", "gicp", "aligned", "zero_p", "rank2_p", "one")
THIN = {"gicp": 1e-3, "aligned": 1e-6}


def _frames(rng, n):
    return np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]


def _sym(Q, lam):
    C = np.einsum("eik,ek,ejk->eij", Q, lam, Q)
    return (C + C.transpose(0, 2, 1)) / 2


def make_cov(rng, cls, M):
    """cov_p6, cov_z6 ([E,6], or [1,6] for 'one') of the class; M [E,3,3]: the rotation of every edge at the layout's poses
    (the class 'aligned' is built against it)"""
    E = len(M)
    n = 1 if cls == "one" else E
    sp, sz = rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, n)
    I3 = np.broadcast_to(np.eye(3), (n, 3, 3))
    if cls == "iso":
        Cp, Cz = sp[:, None, None] * I3, sz[:, None, None] * I3
    elif cls in ("gicp", "one"):
        lam = np.array([1.0, 1.0, THIN["gicp"]])
        Cp, Cz = _sym(_frames(rng, n), sp[:, None] * lam), _sym(_frames(rng, n), sz[:, None] * lam)
    elif cls == "aligned":
        Qz = _frames(rng, n)
        Qp = np.einsum("eki,ekj->eij", M, Qz)                    # M^T Qz: M C_p M^T has the frame of C_z
        lam = np.array([1.0, 1.0, THIN["aligned"]])
        Cp, Cz = _sym(Qp, lam[None] * np.stack([sp, np.ones(n), np.ones(n)], 1)), _sym(Qz, lam[None] * np.stack([np.ones(n), sz, np.ones(n)], 1))
    elif cls == "zero_p":
        Cp, Cz = np.zeros((n, 3, 3)), _sym(_frames(rng, n), sz[:, None] * np.array([1.0, 0.3, 1e-2]))
    elif cls == "rank2_p":
        Cp, Cz = _sym(_frames(rng, n), sp[:, None] * np.array([1.0, 1.0, 0.0])), _sym(_frames(rng, n), sz[:, None] * np.array([1.0, 0.5, 0.1]))
    else:
        raise KeyError(cls)
    return gr.pack(Cp), gr.pack(Cz)


def _with_cov(lay, cls, seed):
    e = {k: v for k, v in lay["e"].items() if k != "info6"}
    M = gr._rotations(lay["poses"], e, np.float64)[0]
    e["cov_p6"], e["cov_z6"] = make_cov(np.random.default_rng(seed), cls, M)
    out = dict(poses=lay["poses"], n_free=lay["n_free"], P=lay["P"], e=e, cov_class=cls)
    out["census"] = census(out)
    return out


def census(lay):
    """what the class is designed to hold, from the set alone: kappa(S) at the layout's poses, the smallest eigenvalue of
    C_p and C_z relative to their largest, n_cov"""
    e = lay["e"]
    E = gr.n_edges(e)
    M = gr._rotations(lay["poses"], e, np.float64)[0]
    Cp, Cz = gr._cov(e, "cov_p6", E, np.float64), gr._cov(e, "cov_z6", E, np.float64)
    S = Cz + np.einsum("eik,ekl,ejl->eij", M, Cp, M)
    ev = np.linalg.eigvalsh((S + S.transpose(0, 2, 1)) / 2)
    lp, lz = np.linalg.eigvalsh(Cp), np.linalg.eigvalsh(Cz)
    return dict(n=E, n_cov=len(np.asarray(e["cov_p6"]).reshape(-1, 6)), kappa_max=float((ev[:, 2] / ev[:, 0]).max()),
                kappa_min=float((ev[:, 2] / ev[:, 0]).min()), lam_min_p=float(lp[:, 0].min()), lam_max_p=float(lp[:, 2].max()),
                lam_mid_p=float(lp[:, 1].min()), lam_min_z=float(lz[:, 0].min()), n_inactive=int(np.sum(~np.asarray(e["active"]))))


# ------------------------------------------------------------------ the pair kind
PAIR_LAYOUTS = {
    # name: (robust kernel, class)
    "A_gicp": (CAUCHY, "gicp"), "A_aligned": (HUBER, "aligned"), "A_iso": (NONE, "iso"), "A_zero_p": (TUKEY, "zero_p"),
    "A_rank2_p": (NONE, "rank2_p"), "A_one": (HUBER, "one"), "B_gicp": (HUBER, "gicp"), "B_aligned": (NONE, "aligned"),
}
PAIR_NAMES = list(PAIR_LAYOUTS)


@functools.lru_cache(maxsize=None)
def pair_layout(name):
    rk, cls = PAIR_LAYOUTS[name]
    k = PAIR_NAMES.index(name)
    if name.startswith("A_"):
        base = pdz._make(900 + k, pdz.P_ALL_A, pdz.P_FREE_A, pdz.runs_A(), rk, "zero")
    else:
        base = dict(pdz.layout("B"))
        base["e"] = dict(base["e"], rk=rk)
    return _with_cov(base, cls, 950 + k)


@functools.lru_cache(maxsize=None)
def index_check_layout(kind):
    """the layouts 'G' of pair_designed / point_designed (more edges than one grid-stride trip of the index check covers)
    with one covariance pair for all edges: for the index check alone"""
    return _with_cov(pdz.layout("G") if kind == "pair" else pt.layout("G"), "one", 990)


def pair_device_arrays(e, perm):
    """the arrays of cugo_gicp_pair_edges in the plan's sorted order: pose_a, pose_b [n], p, z [3][n], cov_p, cov_z
    [6][n_cov], flags [n]"""
    pa, pb, p, z, cp, fl = pdz.device_arrays(dict(e, info6=e["cov_p6"]), perm)
    cz = pdz.device_arrays(dict(e, info6=e["cov_z6"]), perm)[4]
    return pa, pb, p, z, cp, cz, fl


@functools.lru_cache(maxsize=None)
def pair_unary_twin(cls="gicp"):
    """the last pose the FIXED identity (index P - 1, n_free = P - 1), every edge from it to a free pose b: the pair term on
    b is the unary term (p, z, C_p, C_z) on b.  Returns the pair layout and the unary layout on the same poses"""
    rng = np.random.default_rng(977)
    deg = [40, 1, 70, 13]
    P = len(deg) + 1
    lay = pt._point(978, deg + [0], P - 1, HUBER, "zero")
    poses = lay["poses"].copy()
    poses[P - 1] = [0, 0, 0, 1, 0, 0, 0]
    eu = {k: v for k, v in lay["e"].items() if k != "info6"}
    M = gr._rotations(poses, eu, np.float64)[0]
    eu["cov_p6"], eu["cov_z6"] = make_cov(rng, cls, M)
    E = len(eu["pose"])
    ep = dict(a=np.full(E, P - 1, np.int32), b=eu["pose"].astype(np.int32), p=eu["p"], z=eu["z"], cov_p6=eu["cov_p6"], cov_z6=eu["cov_z6"],
              active=eu["active"], flags=eu["flags"], rk=eu["rk"])
    return dict(poses=poses, n_free=P - 1, P=P, e=ep), dict(poses=poses, n_free=P - 1, P=P, e=eu)


# ------------------------------------------------------------------ the unary kind
POINT_LAYOUTS = {
    # name: (degrees, n_free, robust kernel, class, inactive)
    "A_gicp": (DEG_A, None, CAUCHY, "gicp", None), "A_iso": (DEG_A, None, NONE, "iso", None),
    "B_aligned": (DEG_B, None, HUBER, "aligned", None), "B_zero_p": (DEG_B, None, TUKEY, "zero_p", None),
    "C_one": (DEG_C, FREE_C, HUBER, "one", None), "D_rank2_p": (DEG_D, None, NONE, "rank2_p", INACT_D),
    "D_gicp": (DEG_D, None, TUKEY, "gicp", INACT_D),
}
POINT_NAMES = list(POINT_LAYOUTS)


@functools.lru_cache(maxsize=None)
def point_layout(name):
    deg, nf, rk, cls, ina = POINT_LAYOUTS[name]
    k = POINT_NAMES.index(name)
    return _with_cov(pt._point(800 + k, deg, nf, rk, "zero", ina), cls, 850 + k)


def point_device_arrays(e):
    """the planar arrays of cugo_gicp_edges: p, z [3][n], cov_p, cov_z [6][n_cov]"""
    p, z, cp = pt.device_arrays(dict(e, info6=e["cov_p6"]))
    return p, z, cp, pt.device_arrays(dict(e, info6=e["cov_z6"]))[2]


def counting(lay):
    return pt.counting(lay)


def moved(poses, seed=5, angle=0.2, shift=0.1):
    """the poses after a step: every rotation turned by up to `angle`, every translation moved (the second evaluation of
    the 'frozen' mutation; also the OTHER poses of an error pass)"""
    rng = np.random.default_rng(seed)
    out = np.asarray(poses, np.float64).copy()
    for k in range(len(out)):
        w = rng.normal(size=3)
        w *= rng.uniform(0.5, 1.0) * angle / np.linalg.norm(w)
        th = np.linalg.norm(w)
        dq = np.concatenate([np.sin(th / 2) * w / th, [np.cos(th / 2)]])
        x1, y1, z1, w1 = dq
        x2, y2, z2, w2 = out[k, :4]
        q = np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                      w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])
        out[k, :4] = q / np.linalg.norm(q)
        out[k, 4:] += rng.normal(0, shift, 3)
    return out
