"""numpy restatement of the point-to-plane / point-to-line pose edges (include/icp_types.h) and of the
cugo_icp_edges layout of include/cugo_hip.h (numpy only, no product code).

Pose (q, t), quaternion (x, y, z, w), read as the BA edges read it: y = R(q) p + t.  Left update
T <- exp([w, v]) T in the tangent order [w, v], so dy/dxi = [-[y]x | I].
    plane: r = n.y - d                      J = n^T [-[y]x | I]
    line:  r = (I - u u^T)(y - a)           J = (I - u u^T) [-[y]x | I],  u = (b - a) / |b - a|
chi2 term rho(omega |r|^2), weight w = omega rho'(omega |r|^2); H = sum w J^T J and b = -sum w J^T r: the convention
of the BA build pass (tests/golden/make_golden.py: its Jacobian is d(meas - proj), so b is minus half the gradient of
chi2), under which the solver takes H dx = b and applies exp(+dx).
"""
import importlib

import numpy as np

import synth

RK_NONE, RK_CAUCHY, RK_TUKEY, RK_HUBER = 0, 1, 2, 3


def rho(kind, delta, x):
    d2 = delta * delta
    if kind == RK_TUKEY:
        return (d2 / 3) * (1 - (1 - x / d2) ** 3) if x <= d2 else d2 / 3
    if kind == RK_CAUCHY:
        return d2 * np.log(x / d2 + 1.0)
    if kind == RK_HUBER:
        return x if x <= d2 else 2 * delta * np.sqrt(x) - d2
    return x


def drho(kind, delta, x):
    d2 = delta * delta
    if kind == RK_TUKEY:
        return (1 - x / d2) ** 2 if x <= d2 else 0.0
    if kind == RK_CAUCHY:
        return 1.0 / (x / d2 + 1.0)
    if kind == RK_HUBER:
        return 1.0 if x <= d2 else delta / np.sqrt(x)
    return 1.0


def skew(y):
    return np.array([[0.0, -y[2], y[1]], [y[2], 0.0, -y[0]], [-y[1], y[0], 0.0]])


def transform(pose7, p):
    return synth.quat_to_R(pose7[:4]) @ p + pose7[4:]


def left_update(pose7, xi):
    """exp([w, v]) T to first order in v (exact in w): R' = Exp(w) R, t' = Exp(w) t + v."""
    dq = synth.quat_from_rotvec(xi[:3])
    q = synth.quat_mul(dq, pose7[:4])
    t = synth.quat_to_R(dq) @ pose7[4:] + xi[3:]
    return np.concatenate([q / np.linalg.norm(q), t])


def plane_residual(pose7, n, d, p):
    return np.array([n @ transform(pose7, p) - d])


def plane_jacobian(pose7, n, d, p):
    y = transform(pose7, p)
    return (n @ np.hstack([-skew(y), np.eye(3)]))[None, :]


def line_direction(a, b):
    u = b - a
    return u / np.linalg.norm(u)


def line_residual(pose7, a, u, p):
    P = np.eye(3) - np.outer(u, u)
    return P @ (transform(pose7, p) - a)


def line_jacobian(pose7, a, u, p):
    y = transform(pose7, p)
    P = np.eye(3) - np.outer(u, u)
    return P @ np.hstack([-skew(y), np.eye(3)])


def random_pose(rng, rot=0.5, trans=2.0):
    q = synth.quat_from_rotvec(rng.normal(0, rot, 3))
    return np.concatenate([q / np.linalg.norm(q), rng.normal(0, trans, 3)])


def make_edges(rng, pose_of_edge, kind, poses, noise=0.05):
    """Edges of one kind on the given poses (pose_of_edge: pose index per edge), consistent with the poses up to
    `noise`.  Returns a dict with pose, p [E,3], and n [E,3], d [E] (plane) or a, b [E,3] (line)."""
    E = len(pose_of_edge)
    p = rng.normal(0, 4.0, (E, 3))
    pose = np.asarray(pose_of_edge, np.int32)
    R = np.array([synth.quat_to_R(q[:4]) for q in poses])
    y = np.einsum("eij,ej->ei", R[pose], p) + poses[pose, 4:] + rng.normal(0, noise, (E, 3))
    out = dict(pose=pose, p=p)
    if kind == "plane":
        n = rng.normal(0, 1, (E, 3))
        n /= np.linalg.norm(n, axis=1)[:, None]
        out["n"] = n
        out["d"] = np.einsum("ij,ij->i", n, y)
    else:
        u = rng.normal(0, 1, (E, 3))
        u /= np.linalg.norm(u, axis=1)[:, None]
        a = y - rng.uniform(-3, 3, E)[:, None] * u
        out["a"] = a
        out["b"] = a + rng.uniform(0.5, 4, E)[:, None] * u
    return out


def edge_terms(kind, e, i, pose7, omega, rk):
    """(chi2 term, H 6x6, b 6) of edge i of a make_edges dict (b = -w J^T r, see the module's docstring)."""
    if kind == "plane":
        r = plane_residual(pose7, e["n"][i], e["d"][i], e["p"][i])
        J = plane_jacobian(pose7, e["n"][i], e["d"][i], e["p"][i])
    else:
        u = line_direction(e["a"][i], e["b"][i])
        r = line_residual(pose7, e["a"][i], u, e["p"][i])
        J = line_jacobian(pose7, e["a"][i], u, e["p"][i])
    x = omega * float(r @ r)
    w = omega * drho(rk[0], rk[1], x)
    return rho(rk[0], rk[1], x), w * J.T @ J, -w * J.T @ r


def _rho_vec(rk, x):
    return np.array([rho(rk[0], rk[1], v) for v in x]) if rk[0] else x.copy()


def _drho_vec(rk, x):
    return np.array([drho(rk[0], rk[1], v) for v in x]) if rk[0] else np.ones_like(x)


def reference_build(poses, n_free, kinds):
    """kinds: list of (kind, edges dict, omega [E] or [1], active [E] bool, rk (type, delta)).  Per free pose
    H [P,6,6], b [P,6], the chi2 total and the chi2 term of every edge (per kind; 0 where the edge does not count)."""
    H = np.zeros((n_free, 6, 6))
    b = np.zeros((n_free, 6))
    chi = 0.0
    per_edge = []
    for kind, e, omega, active, rk in kinds:
        pose = np.asarray(e["pose"])
        E = len(pose)
        omega = np.broadcast_to(np.asarray(omega, np.float64), (E,))
        R = np.array([synth.quat_to_R(q[:4]) for q in poses])
        y = np.einsum("eij,ej->ei", R[pose], e["p"]) + poses[pose, 4:]
        S = np.zeros((E, 3, 3))  # -[y]x
        S[:, 0, 1], S[:, 0, 2], S[:, 1, 0] = y[:, 2], -y[:, 1], -y[:, 2]
        S[:, 1, 2], S[:, 2, 0], S[:, 2, 1] = y[:, 0], y[:, 1], -y[:, 0]
        G = np.concatenate([S, np.broadcast_to(np.eye(3), (E, 3, 3))], axis=2)  # dy/dxi [E,3,6]
        if kind == "plane":
            r = (np.einsum("ei,ei->e", e["n"], y) - e["d"])[:, None]
            J = np.einsum("ei,eij->ej", e["n"], G)[:, None, :]
        else:
            u = (e["b"] - e["a"]) / np.linalg.norm(e["b"] - e["a"], axis=1)[:, None]
            Pm = np.eye(3)[None] - np.einsum("ei,ej->eij", u, u)
            r = np.einsum("eij,ej->ei", Pm, y - e["a"])
            J = np.einsum("eij,ejk->eik", Pm, G)
        x = omega * np.einsum("ei,ei->e", r, r)
        ce = _rho_vec(rk, x)
        w = omega * _drho_vec(rk, x)
        keep = (pose < n_free) & np.asarray(active, bool)
        ce = np.where(keep, ce, 0.0)
        w = np.where(keep, w, 0.0)
        h = np.einsum("e,eki,ekj->eij", w, J, J)
        g = -np.einsum("e,eki,ek->ei", w, J, r)
        q = np.where(keep, pose, 0)
        np.add.at(H, q[keep], h[keep])
        np.add.at(b, q[keep], g[keep])
        chi += float(ce.sum())
        per_edge.append(ce)
    return H, b, chi, per_edge


# ------------------------------------------------------------------ device layout -----------
def sort_by_pose(e):
    """The edges stably sorted by pose (the order cugo_icp_edges requires) and the permutation."""
    order = np.argsort(e["pose"], kind="stable")
    return {k: v[order] for k, v in e.items()}, order


def pose_ptr(pose, n_poses_total):
    ptr = np.zeros(n_poses_total + 1, np.int32)
    np.add.at(ptr, pose + 1, 1)
    return np.cumsum(ptr).astype(np.int32)


def upload(ctx, n_poses_total, n_free, plane=None, line=None):
    """cugo_icp_edges over sorted edge dicts with 'omega' (per edge or [1]), optional 'flags', 'rk' (type, delta)."""
    cugo = importlib.import_module("cuda-bundle-adjustment_amd")
    ev = cugo.IcpEdges()
    ev.n_poses_total, ev.n_poses_free = n_poses_total, n_free
    for name, e in (("plane", plane), ("line", line)):
        n = 0 if e is None else len(e["pose"])
        setattr(ev, "n_" + name, n)
        if e is None:
            setattr(ev, "d_%s_pose_ptr" % name, ctx.to_dev(np.zeros(n_poses_total + 1, np.int32)))
            continue
        setattr(ev, "d_%s_pose" % name, ctx.to_dev(e["pose"].astype(np.int32)))
        setattr(ev, "d_%s_pose_ptr" % name, ctx.to_dev(pose_ptr(e["pose"], n_poses_total)))
        setattr(ev, "d_%s_p" % name, ctx.to_dev(np.ascontiguousarray(e["p"].T)))
        if name == "plane":
            geo = np.vstack([e["n"].T, e["d"][None, :]])
            ev.d_plane_nd = ctx.to_dev(np.ascontiguousarray(geo))
        else:
            u = (e["b"] - e["a"]) / np.linalg.norm(e["b"] - e["a"], axis=1)[:, None]
            ev.d_line_au = ctx.to_dev(np.ascontiguousarray(np.vstack([e["a"].T, u.T])))
        omega = np.asarray(e["omega"], np.float64)
        setattr(ev, "d_%s_omega" % name, ctx.to_dev(omega))
        setattr(ev, "n_%s_omega" % name, len(omega))
        if e.get("flags") is not None:
            setattr(ev, "d_%s_flags" % name, ctx.to_dev(np.asarray(e["flags"], np.uint8)))
        rk = e.get("rk", (RK_NONE, 1.0))
        setattr(ev, "rk_" + name, rk[0])
        setattr(ev, "delta_" + name, rk[1])
    return ev
