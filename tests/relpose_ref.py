"""numpy restatement of the relative-pose SE(3) edges (include/relpose_types.h; an extension: the reference has no such
edge) and of the cugo_relpose_edges / cugo_relpose_plan layout of include/cugo_hip.h (numpy only, no product code).

Poses (q, t), quaternion (x, y, z, w), read as everywhere else (y = R(q) p + t); left update T <- Exp([w, v]) T in the
tangent order [w, v].  For an edge between poses a and b with measurement Z ~ T_a T_b^-1 and information Omega:
    A = T_a T_b^-1 = (R_A, t_A),  D = A Z^-1 = (R_D, t_D)
    r = [Log_SO3(R_D); t_D]
    J_a = [[J_l^-1(phi), 0], [-[t_D]x, I]]       (prior_ref.jacobian with the pose A)
    J_b = -J_a Ad(A),  Ad(A) = [[R_A, 0], [[t_A]x R_A, R_A]]
         (Exp(xi) T_b turns A into A Exp(-xi) = Exp(-Ad(A) xi) A)
    x = max(0, r^T Omega r), chi2 term rho(x), w = rho'(x)
    H_aa += w J_a^T Omega J_a,  H_bb += w J_b^T Omega J_b,  H_(lo,hi) += w J_lo^T Omega J_hi,  b_s -= w J_s^T Omega r
An edge with one fixed end counts in chi2 and adds only its free end's block and b; one with two fixed ends, or
inactive, counts for nothing.  The sums over the edges are taken in extended precision (np.longdouble) and rounded once.

`mistake` in reference_build plants one deliberate error (tests/test_relpose_host.py checks that each of them breaks
the comparison with the correct build): "chi2_twice", "transposed", "no_tA", "overwrite".
"""
import importlib

import numpy as np

import icp_ref
import prior_ref as PR
import synth

RK_NONE, RK_CAUCHY, RK_TUKEY, RK_HUBER = 0, 1, 2, 3
EDGE_INACTIVE = 8
LD = np.longdouble


# ------------------------------------------------------------------ pose algebra ------------
def pose_mul(A, B):
    q = synth.quat_mul(A[:4], B[:4])
    return np.concatenate([q / np.linalg.norm(q), synth.quat_to_R(A[:4]) @ B[4:] + A[4:]])


def pose_inv(A):
    q = np.array([-A[0], -A[1], -A[2], A[3]])
    return np.concatenate([q, -(synth.quat_to_R(A[:4]).T @ A[4:])])


def relative(pa, pb):
    """(R_A, t_A) of A = T_a T_b^-1, in the operation order of the kernel"""
    RA = synth.quat_to_R(pa[:4]) @ synth.quat_to_R(pb[:4]).T
    return RA, pa[4:] - RA @ pb[4:]


IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


# ------------------------------------------------------------------ one edge ----------------
def residual(pa, pb, z):
    RA, tA = relative(pa, pb)
    RD = RA @ synth.quat_to_R(z[:4]).T
    return np.concatenate([PR.log_so3(RD), tA - RD @ z[4:]])


def adjoint(RA, tA, with_tA=True):
    Ad = np.zeros((6, 6))
    Ad[:3, :3] = Ad[3:, 3:] = RA
    if with_tA:
        Ad[3:, :3] = icp_ref.skew(tA) @ RA
    return Ad


def jacobians(pa, pb, z, with_tA=True):
    """(J_a, J_b) = (dr/dxi_a, dr/dxi_b) under the left update"""
    r = residual(pa, pb, z)
    Ja = np.eye(6)
    Ja[:3, :3] = PR.inv_left_jacobian(r[:3])
    Ja[3:, :3] = -icp_ref.skew(r[3:])
    RA, tA = relative(pa, pb)
    return Ja, -Ja @ adjoint(RA, tA, with_tA)


def edge_terms(pa, pb, z, Om, rk, with_tA=True):
    """(chi2 term, w J_a^T Om J_a, w J_b^T Om J_b, w J_a^T Om J_b, b_a, b_b) of one edge"""
    r = residual(pa, pb, z)
    Ja, Jb = jacobians(pa, pb, z, with_tA)
    x = max(0.0, float(r @ Om @ r))
    w = icp_ref.drho(rk[0], rk[1], x)
    return (icp_ref.rho(rk[0], rk[1], x), w * Ja.T @ Om @ Ja, w * Jb.T @ Om @ Jb, w * Ja.T @ Om @ Jb,
            -w * Ja.T @ Om @ r, -w * Jb.T @ Om @ r)


# ------------------------------------------------------------------ edge sets ---------------
def make_edges(a, b, z, info, rk=(RK_NONE, 1.0), active=None):
    a, b = np.asarray(a, np.int32), np.asarray(b, np.int32)
    return dict(a=a, b=b, z=np.asarray(z, np.float64).reshape(len(a), 7),
                info=np.asarray(info, np.float64).reshape(-1, 6, 6),
                active=np.ones(len(a), bool) if active is None else np.asarray(active, bool), rk=rk)


def flags_of(rp):
    return np.where(rp["active"], 0, EDGE_INACTIVE).astype(np.uint8)


def counting(rp, n_free):
    return rp["active"] & ((rp["a"] < n_free) | (rp["b"] < n_free))


def pattern(rp, n_free):
    """upper block CSR of the pose graph: row p = p, then the hi > p joined to it by a counting free-free edge"""
    rows = [set() for _ in range(n_free)]
    for a, b, c in zip(rp["a"], rp["b"], counting(rp, n_free)):
        if c and a < n_free and b < n_free:
            rows[min(a, b)].add(int(max(a, b)))
    rowptr, colind = [0], []
    for p in range(n_free):
        colind += [p] + sorted(rows[p])
        rowptr.append(len(colind))
    return np.array(rowptr, np.int32), np.array(colind, np.int32)


def block_of(rowptr, colind, lo, hi):
    k = rowptr[lo] + int(np.searchsorted(colind[rowptr[lo]:rowptr[lo + 1]], hi))
    assert k < rowptr[lo + 1] and colind[k] == hi, (lo, hi)
    return k


def plan(rp, n_free, rowptr, colind):
    """(inc_ptr, inc, off_blk) as cugo_relpose_plan_create builds them"""
    E = len(rp["a"])
    lists = [[] for _ in range(n_free)]
    off = np.full(E, -1, np.int32)
    cnt = counting(rp, n_free)
    for e in range(E):
        if not cnt[e]:
            continue
        a, b = int(rp["a"][e]), int(rp["b"][e])
        if a < n_free:
            lists[a].append(2 * e)
        if b < n_free:
            lists[b].append(2 * e + 1)
        if a < n_free and b < n_free:
            off[e] = block_of(rowptr, colind, min(a, b), max(a, b))
    inc_ptr = np.zeros(n_free + 1, np.int32)
    inc_ptr[1:] = np.cumsum([len(x) for x in lists])
    return inc_ptr, np.array([x for lst in lists for x in lst], np.int32), off


def reference_build(poses, n_free, rp, rowptr=None, colind=None, mistake=None):
    """rp: dict a, b [E] (free-first indices), z [E,7], info [E,6,6] or [1,6,6], active [E] bool, rk.
    Returns the diagonal blocks H [P,6,6], b [P,6], the blocks of the pattern Hoff [nnzb,6,6] (only off-diagonal ones are
    filled: block (lo, hi) holds H_(lo,hi), rows of pose lo), the chi2 total and the chi2 term of every edge (0 where it
    does not count).  Sums in extended precision."""
    if rowptr is None:
        rowptr, colind = pattern(rp, n_free)
    E = len(rp["a"])
    H = np.zeros((n_free, 6, 6), LD)
    b = np.zeros((n_free, 6), LD)
    Hoff = np.zeros((len(colind), 6, 6), LD)
    ce = np.zeros(E)
    chi = LD(0)
    Om = np.broadcast_to(np.asarray(rp["info"], np.float64).reshape(-1, 6, 6), (E, 6, 6)) if E else None
    rk = rp.get("rk", (RK_NONE, 1.0))
    cnt = counting(rp, n_free)
    for e in range(E):
        if not cnt[e]:
            continue
        ia, ib = int(rp["a"][e]), int(rp["b"][e])
        c, Haa, Hbb, Hab, ba, bb = edge_terms(poses[ia], poses[ib], rp["z"][e], Om[e], rk, with_tA=mistake != "no_tA")
        ce[e] = c
        chi += c
        if mistake == "chi2_twice" and ia < n_free and ib < n_free:
            chi += c
        if ia < n_free:
            H[ia] += Haa
            b[ia] += ba
        if ib < n_free:
            H[ib] += Hbb
            b[ib] += bb
        if ia < n_free and ib < n_free:
            k = block_of(rowptr, colind, min(ia, ib), max(ia, ib))
            # block (lo, hi) = J_lo^T Om J_hi: J_a^T Om J_b when a is lo, its transpose when b is
            blk = Hab if ia < ib or mistake == "transposed" else Hab.T
            if mistake == "overwrite":
                Hoff[k] = blk
            else:
                Hoff[k] += blk
    return H.astype(np.float64), b.astype(np.float64), Hoff.astype(np.float64), float(chi), ce


def dense_system(H, b, Hoff, rowptr, colind):
    """the symmetric [6P, 6P] matrix and rhs of the block form"""
    P = len(H)
    A = np.zeros((6 * P, 6 * P))
    for p in range(P):
        A[6 * p:6 * p + 6, 6 * p:6 * p + 6] = H[p]
        for k in range(rowptr[p] + 1, rowptr[p + 1]):
            q = colind[k]
            A[6 * p:6 * p + 6, 6 * q:6 * q + 6] = Hoff[k]
            A[6 * q:6 * q + 6, 6 * p:6 * p + 6] = Hoff[k].T
    return A, b.reshape(-1)


def total_chi2(poses, n_free, rp):
    return reference_build(poses, n_free, rp)[3]


# ------------------------------------------------------------------ device layout -----------
def upload(ctx, n_poses_total, n_free, rp, rowptr, colind, flags=None):
    """(cugo_relpose_edges, plan) over an edge dict; the plan is built with the dict's own flags unless `flags` is
    given (then the plan sees all edges active and `flags` go to the device: run-time flags)"""
    cugo = importlib.import_module("cuda-bundle-adjustment_amd")
    n = len(rp["a"])
    pl = cugo.RelPosePlan(ctx.h, n_poses_total, n_free, rp["a"], rp["b"], flags_of(rp) if flags is None else None,
                          rowptr, colind)
    ev = cugo.RelPoseEdges()
    ev.n_poses_total, ev.n_poses_free, ev.n = n_poses_total, n_free, n
    ev.d_meas = ctx.to_dev(np.ascontiguousarray(np.asarray(rp["z"], np.float64).reshape(n, 7).T))
    info = PR.pack_info(np.asarray(rp["info"], np.float64).reshape(-1, 6, 6))
    ev.d_info = ctx.to_dev(np.ascontiguousarray(info.T))
    ev.n_info = len(info)
    ev.d_flags = ctx.to_dev(flags_of(rp) if flags is None else np.asarray(flags, np.uint8))
    rk = rp.get("rk", (RK_NONE, 1.0))
    ev.rk, ev.delta = rk[0], rk[1]
    ev.plan = pl.handle
    return ev, pl


# ------------------------------------------------------------------ input recipes -----------
def measured(rng, pa, pb, rot=0.05, trans=0.3, angle=None):
    """Z with D = T_a T_b^-1 Z^-1 = Exp(xi): xi ~ N(0, rot), N(0, trans), or a rotation of exactly `angle`.
    (Z = Exp(-xi) A to first order in the translation part: the angle is exact.)"""
    A = pose_mul(pa, pose_inv(pb))
    if angle is None:
        w = rng.normal(0, rot, 3)
    else:
        w = rng.normal(size=3)
        w *= angle / np.linalg.norm(w)
    return icp_ref.left_update(A, np.concatenate([-w, rng.normal(0, trans, 3)]))


def random_edges(rng, poses, pairs, rk=(RK_NONE, 1.0), inactive_frac=0.0, per_edge_info=True, rot=0.05, trans=0.3,
                 angles=None):
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    E = len(pairs)
    z = np.array([measured(rng, poses[a], poses[b], rot, trans, None if angles is None else angles[i % len(angles)])
                  for i, (a, b) in enumerate(pairs)]).reshape(E, 7)
    info = np.array([PR.random_spd(rng, rng.uniform(0.5, 3.0)) for _ in range(E if per_edge_info else 1)])
    return make_edges(pairs[:, 0], pairs[:, 1], z, info, rk=rk, active=rng.random(E) >= inactive_frac)


def ring_case(seed=11, P=40, n_chords=12, rot=0.03, trans=0.1):
    """P poses on a ring, position = index (pose 0 fixed and therefore LAST in the free-first order), edges i -> i+1 and
    n_chords chords in mixed orientation, zero-noise measurements; returns ground truth, perturbed start (free-first
    order), the edge dict in free-first indices"""
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(P) / P
    gt = np.zeros((P, 7))
    for i in range(P):
        q = synth.quat_from_rotvec(np.array([0.0, 0.0, ang[i]]) + rng.normal(0, 0.1, 3))
        gt[i] = np.concatenate([q / np.linalg.norm(q), [5 * np.cos(ang[i]), 5 * np.sin(ang[i]), rng.normal(0, 0.3)]])
    # free-first: poses 1..P-1 are 0..P-2, pose 0 is P-1
    order = np.concatenate([np.arange(1, P), [0]])
    gt = gt[order]
    idx = np.empty(P, int)
    idx[order] = np.arange(P)
    pairs = [(idx[i], idx[(i + 1) % P]) for i in range(P)]
    for _ in range(n_chords):
        i, j = rng.choice(P, 2, replace=False)
        pairs.append((idx[i], idx[j]))
    pairs = np.array(pairs, np.int32)
    z = np.array([pose_mul(gt[a], pose_inv(gt[b])) for a, b in pairs])
    info = np.array([PR.random_spd(rng, 2.0) for _ in pairs])
    start = gt.copy()
    for p in range(P - 1):
        start[p] = PR.displaced(rng, gt[p], rot, trans)
    return gt, start, make_edges(pairs[:, 0], pairs[:, 1], z, info)
