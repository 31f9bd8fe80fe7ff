"""Extended-precision reference of the predicted observation and its covariance (k_predict_obs of cov_kernels.hip,
reached through cugo_predict_observations) with PER-ENTRY error bounds (numpy, test only).

One query: pose a (q, t), landmark X_l, camera cam5 = (fx, fy, cx, cy, bf), kind 2 (u, v) / 3 (u, v, u_right) /
4 (u, v, 1 / Z_s), and an optional camera-table entry {M row-major, t_s, k1..k4, model} (cugo.camera_model_table):
    Xb = R(q) X_l + t,   Xs = M Xb + t_s,   z = proj(Xs)
    A = -dz/dXs,  B = A M,  JP[:, 3:6] = B,  JP[:, 0:3] = -B [Xb]x  (left update on the body),  JL = B R(q)
    S = JP Saa JP^T + X + X^T + JL Sll JL^T,   X = JP Sal JL^T
A fixed pose drops the terms with JP, a fixed landmark those with JL.  Pinhole rows: rig_ref's A (mono, stereo) and, for
kind 4, A2 = (0, 0, 1 / Zs^2), z2 = 1 / Zs (the depth row under unit weight: S in measurement units).  A Kannala-Brandt
entry (fisheye_ref.kb_terms / kb_A / kb_A_mass) has two rows whatever the kind: the third row and column are zero.

Without a table (tab = None) the camera sits at the pose and the Jacobians are the closed forms of
pl_cov_ref.jacobians (what k_reprojection_cov evaluates), with the depth row JP2 = (Y, -X, 0, 0, 0, 1) / Z^2,
JL2 = R[2] / Z^2 added for kind 4.

Bounds, in the project's form.  S: K_S_PRED (n + C) u mass per entry, n = 81 summed terms as in pl_cov_ref, mass the
same expression with the Jacobian masses and |Sigma|.  C per kind of entry, counted as pl_cov_ref counts C_S (two Jacobian
entries on the longest path and two products):
    no table            J_P 40 (kernel_ref)   -> C = 2 x 40 + 2 = 82    (the depth row: 1/Z 9, squared 19, x Y 8 -> 28 <= 40)
    pinhole entry       J_P 55 (rig_ref)      -> C = 2 x 55 + 2 = 112   (the depth row: 1/Zs 13, squared 27, B 30 <= 45)
    Kannala-Brandt      J_P 1483 (fisheye_ref)-> C = 2 x 1483 + 2 = 2968
z: K_Z_PRED c_z u mass per entry with c_z the residual's count without the measurement (kernel_ref e_i 21 -> 20,
rig_ref 29 -> 28, fisheye_ref 462 -> 461; the depth row 1 / Zs: 13) and mass |terms of the projection| (+ the lever
sum_i |dz/dXs_i| aXs_i for a Kannala-Brandt entry, as fisheye_ref builds the mass of e).

K_S_PRED and K_Z_PRED are measured, not derived (test_predict_ref_host.py): 4 x the largest ratio that the float64 run of
this same module reaches against its longdouble run — S in two summation orders ("terms", "joint"), z has one — over
the designs DESIGNS with the queries of designed_queries(), with the table and without, rounded up.  REPLAY_S / REPLAY_Z:
the float64 replay's worst ratio per design in units of (n + C) u mass / c_z u mass (x86-64, 80-bit longdouble).

`mut` names ONE deliberate mistake (test_predict_ref_host.py shows that each leaves the bounds):
    "B_without_M"      B = A
    "Xs_cross"         [Xs]x in the place of [Xb]x
    "pinhole_A"        the pinhole A on a Kannala-Brandt entry
    "quotient_c"       the quotient form of c below the switch (shows in a float64 evaluation only)
    "ts_dropped"       rotation applied, lever arm not
    "depth_weight"     the depth row scaled by a weight of 2
    "cross_once"       J_p Sigma_al J_l^T added once
    "fixed_pose_kept"  the terms of a fixed pose kept
"""
import numpy as np

import fisheye_designed as fd
import fisheye_ref as fr
import kernel_ref as kr
import pl_cov_ref as pr
import rig_ref

LD = kr.LD
U = kr.U
MONO, STEREO, DEPTH = 2, 3, 4
N_S = 81
C_PLAIN, C_RIG, C_KB = 82, 112, 2968
CZ_PLAIN, CZ_RIG, CZ_KB = 20, 28, 461
DESIGNS = ("mixed", "corners", "grid513")
MUTATIONS = ("B_without_M", "Xs_cross", "pinhole_A", "quotient_c", "ts_dropped", "depth_weight", "cross_once",
             "fixed_pose_kept")
K_S_PRED = 0.13   # 4 x 0.0320 (design `mixed`, no table, four terms), rounded up
K_Z_PRED = 0.38   # 4 x 0.0935 (design `grid513`, with the table, a depth row), rounded up
# the fp64 replay's worst ratio per design (S: the larger of its two summation orders; the larger of the run with the
# table and the run without), rounded up (test_predict_ref_host.py)
REPLAY_S = {"mixed": 0.032, "corners": 0.0059, "grid513": 0.0072}
REPLAY_Z = {"mixed": 0.087, "corners": 0.075, "grid513": 0.094}


def dim_of(kind):
    return 2 if kind == MONO else 3


# ------------------------------------------------------------------ geometry
def frames(pose, Xw, dt):
    """R, |R| terms, Xb, its mass: the formulas of kernel_ref.build for one pose and one landmark per query"""
    pose, Xw = np.asarray(pose, dt), np.asarray(Xw, dt)
    E = len(pose)
    x, y, z, w = (pose[:, k] for k in range(4))
    R = np.empty((E, 3, 3), dt)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - z * w); R[:, 0, 2] = 2 * (x * z + y * w)
    R[:, 1, 0] = 2 * (x * y + z * w); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - x * w)
    R[:, 2, 0] = 2 * (x * z - y * w); R[:, 2, 1] = 2 * (y * z + x * w); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    ax_, ay_, az_, aw_ = (np.abs(pose[:, k]) for k in range(4))
    aR = np.empty((E, 3, 3), dt)
    aR[:, 0, 0] = 1 + 2 * (ay_ * ay_ + az_ * az_); aR[:, 0, 1] = 2 * (ax_ * ay_ + az_ * aw_); aR[:, 0, 2] = 2 * (ax_ * az_ + ay_ * aw_)
    aR[:, 1, 0] = aR[:, 0, 1]; aR[:, 1, 1] = 1 + 2 * (ax_ * ax_ + az_ * az_); aR[:, 1, 2] = 2 * (ay_ * az_ + ax_ * aw_)
    aR[:, 2, 0] = aR[:, 0, 2]; aR[:, 2, 1] = aR[:, 1, 2]; aR[:, 2, 2] = 1 + 2 * (ax_ * ax_ + ay_ * ay_)
    Xb = np.einsum("eij,ej->ei", R, Xw) + pose[:, 4:]
    aXb = np.einsum("eij,ej->ei", aR, np.abs(Xw)) + np.abs(pose[:, 4:])
    return R, aR, Xb, aXb


def project(pose, Xw, cam, kind, tab=None, dt=LD, mut=None):
    """per query: z [n,3] and its mass, JP [n,3,6], JL [n,3,3] and their masses, rows3 [n] (whether there is a third
    row), C and c_z [n] (the constants of the bounds), Xs [n,3].  kind [n]; tab [n,17] or None"""
    cam, kind = np.asarray(cam, dt), np.asarray(kind)
    E = len(kind)
    fx, fy, cx, cy, bf = (cam[:, i] for i in range(5))
    st, dp = kind == STEREO, kind == DEPTH
    s, dd = st.astype(dt), dp.astype(dt)
    wd = dt(2) if mut == "depth_weight" else dt(1)
    zero = np.zeros(E, dt)
    R, aR, Xb, aXb = frames(pose, Xw, dt)
    if tab is None:
        JP, aJP, JL, aJL, Z = pr.jacobians(pose, Xw, cam, st, dt)
        JP, aJP, JL, aJL = JP.copy(), aJP.copy(), JL.copy(), aJL.copy()
        iz = 1 / Z
        aiz = aXb[:, 2] * iz * iz
        izz, aizz = iz * iz, np.abs(iz * iz) + 2 * np.abs(iz) * aiz
        JP[:, 2] += (dd * wd * izz)[:, None] * np.stack([Xb[:, 1], -Xb[:, 0], zero, zero, zero, zero + 1], 1)
        aJP[:, 2] += (dd * wd * aizz)[:, None] * np.stack([aXb[:, 1], aXb[:, 0], zero, zero, zero, zero + 1], 1)
        JL[:, 2] += (dd * wd * izz)[:, None] * R[:, 2]
        aJL[:, 2] += (dd * wd * aizz)[:, None] * aR[:, 2]
        xn, yn = Xb[:, 0] * iz, Xb[:, 1] * iz
        axn, ayn = aXb[:, 0] * aiz, aXb[:, 1] * aiz
        pu, pv = fx * xn + cx, fy * yn + cy
        z = np.stack([pu, pv, s * (pu - bf * iz) + dd * wd * iz], 1)
        az = np.stack([fx * axn + np.abs(cx), fy * ayn + np.abs(cy), s * (fx * axn + np.abs(cx) + bf * aiz) + dd * wd * aiz], 1)
        return dict(z=z, z_mass=np.abs(az), JP=JP, aJP=aJP, JL=JL, aJL=aJL, rows3=st | dp, C=np.full(E, C_PLAIN),
                    cz=np.full(E, CZ_PLAIN), Xs=Xb)
    ent = np.asarray(tab, dt)
    assert ent.shape == (E, fr.STRIDE)
    M, ts, kk = ent[:, :9].reshape(E, 3, 3), ent[:, 9:12], ent[:, 12:16]
    fish = np.asarray(tab)[:, 16] != 0
    if mut == "ts_dropped":
        ts = np.zeros((E, 3), dt)
    aM = np.abs(M)
    Xs = np.einsum("eij,ej->ei", M, Xb) + ts
    aXs = np.einsum("eij,ej->ei", aM, aXb) + np.abs(ts)
    st, dp = st & ~fish, dp & ~fish
    s, dd = st.astype(dt), dp.astype(dt)
    # ---- the pinhole rows, as rig_ref (evaluated on every query and selected: a fisheye query may have Z_s <= 0) ----
    with np.errstate(all="ignore"):
        iz = 1 / Xs[:, 2]
        xn, yn = Xs[:, 0] * iz, Xs[:, 1] * iz
        aiz = aXs[:, 2] * iz * iz
        axn, ayn = aXs[:, 0] * aiz, aXs[:, 1] * aiz
        izz, aizz = iz * iz, np.abs(iz * iz) + 2 * np.abs(iz) * aiz
        A = np.zeros((E, 3, 3), dt); aA = np.zeros((E, 3, 3), dt)
        A[:, 0] = np.stack([-fx * iz, zero, fx * xn * iz], 1)
        A[:, 1] = np.stack([zero, -fy * iz, fy * yn * iz], 1)
        A[:, 2] = s[:, None] * np.stack([A[:, 0, 0], zero, A[:, 0, 2] - bf * iz * iz], 1) + \
            (dd * wd)[:, None] * np.stack([zero, zero, izz], 1)
        aA[:, 0] = np.stack([fx * aiz, zero, fx * axn * aiz], 1)
        aA[:, 1] = np.stack([zero, fy * aiz, fy * ayn * aiz], 1)
        aA[:, 2] = s[:, None] * np.stack([aA[:, 0, 0], zero, aA[:, 0, 2] + bf * aiz * aiz], 1) + \
            (dd * wd)[:, None] * np.stack([zero, zero, aizz], 1)
        pu, pv = fx * xn + cx, fy * yn + cy
        z = np.stack([pu, pv, s * (pu - bf * iz) + dd * wd * iz], 1)
        az = np.stack([fx * axn + np.abs(cx), fy * ayn + np.abs(cy), s * (fx * axn + np.abs(cx) + bf * aiz) + dd * wd * aiz], 1)
    A, aA, z, az = (np.where(fish.reshape((E,) + (1,) * (a.ndim - 1)), 0, a) for a in (A, aA, z, az))
    if np.any(fish):
        A_pin = np.zeros((E, 3, 3), dt)
        with np.errstate(all="ignore"):
            A_pin[:, 0] = np.stack([-fx * iz, zero, fx * xn * iz], 1)
            A_pin[:, 1] = np.stack([zero, -fy * iz, fy * yn * iz], 1)
        Ak, _, rho, rho_a = fr.kb_A(Xs[fish], fx[fish], fy[fish], kk[fish], dt, "quotient_c" if mut == "quotient_c" else None)
        aAk = fr.kb_A_mass(Xs[fish], aXs[fish], fx[fish], fy[fish], kk[fish]).astype(dt)
        Ak0 = fr.kb_A(np.asarray(Xs[fish], LD), np.asarray(fx[fish], LD), np.asarray(fy[fish], LD), np.asarray(kk[fish], LD), LD)[0]
        lever = (np.abs(Ak0) * np.asarray(aXs[fish], LD)[:, None, :]).sum(2).astype(dt)
        xs, ys = Xs[fish, 0], Xs[fish, 1]
        z[fish] = np.stack([fx[fish] * rho * xs + cx[fish], fy[fish] * rho * ys + cy[fish], zero[fish]], 1)
        az[fish] = np.stack([fx[fish] * rho_a * np.abs(xs) + np.abs(cx[fish]) + lever[:, 0],
                             fy[fish] * rho_a * np.abs(ys) + np.abs(cy[fish]) + lever[:, 1], zero[fish]], 1)
        A[fish] = A_pin[fish] if mut == "pinhole_A" else Ak
        aA[fish] = aAk
    B = A if mut == "B_without_M" else np.einsum("emk,ekj->emj", A, M)
    aB = aA if mut == "B_without_M" else np.einsum("emk,ekj->emj", aA, aM)
    Xr, aXr = (Xs, aXs) if mut == "Xs_cross" else (Xb, aXb)
    JP = np.concatenate([rig_ref._cross_cols(B, Xr, -1), B], 2)
    aJP = np.concatenate([rig_ref._cross_cols(aB, aXr, 1), aB], 2)
    JL = np.einsum("emk,ekj->emj", B, R)
    aJL = np.einsum("emk,ekj->emj", aB, aR)
    return dict(z=z, z_mass=np.abs(az), JP=JP, aJP=np.abs(aJP), JL=JL, aJL=np.abs(aJL), rows3=st | dp,
                C=np.where(fish, C_KB, C_RIG), cz=np.where(fish, CZ_KB, CZ_RIG), Xs=Xs)


def predict(pose, Xw, cam, kind, tab, Saa, Sal, Sll, free_p, free_l, dtype=LD, order="terms", mut=None):
    """z [n,3], S [n,3,3], their masses and bound constants for n queries from float64 inputs (as
    pl_cov_ref.reprojection, which the table-free mono / stereo case reduces to).  order: "terms" or "joint" """
    dt = dtype
    p = project(pose, Xw, cam, kind, tab, dt, mut)
    fp = np.asarray(free_p, bool) | (mut == "fixed_pose_kept")
    fp, fl = fp.astype(dt)[:, None, None], np.asarray(free_l, bool).astype(dt)[:, None, None]
    JP, aJP, JL, aJL = p["JP"] * fp, p["aJP"] * fp, p["JL"] * fl, p["aJL"] * fl
    Saa, Sal, Sll = (np.nan_to_num(np.asarray(a, dt)) for a in (Saa, Sal, Sll))
    if order == "terms":
        X = np.einsum("nik,nkm,njm->nij", JP, Sal, JL)
        Xt = 0 if mut == "cross_once" else X.transpose(0, 2, 1)
        S = np.einsum("nik,nkm,njm->nij", JP, Saa, JP) + X + Xt + np.einsum("nik,nkm,njm->nij", JL, Sll, JL)
    else:
        J = np.concatenate([JP, JL], 2)
        Sig = np.concatenate([np.concatenate([Saa, Sal], 2), np.concatenate([Sal.transpose(0, 2, 1), Sll], 2)], 1)
        S = J @ Sig @ J.transpose(0, 2, 1)
    aX = np.einsum("nik,nkm,njm->nij", aJP, np.abs(Sal), aJL)
    mass = np.einsum("nik,nkm,njm->nij", aJP, np.abs(Saa), aJP) + aX + aX.transpose(0, 2, 1) + \
        np.einsum("nik,nkm,njm->nij", aJL, np.abs(Sll), aJL)
    return dict(p, S=S, S_mass=mass)


def unit_s(ref):
    """(n + C) u mass per entry of S: the bound without K_S_PRED"""
    return (LD(N_S) + np.asarray(ref["C"], LD))[:, None, None] * LD(U) * np.asarray(ref["S_mass"], LD)


def unit_z(ref):
    return np.asarray(ref["cz"], LD)[:, None] * LD(U) * np.asarray(ref["z_mass"], LD)


def bound_s(ref):
    return LD(K_S_PRED) * unit_s(ref)


def bound_z(ref):
    return LD(K_Z_PRED) * unit_z(ref)


def ratios(got, ref, bnd):
    """per query: the largest |got - ref| / bound over the entries (kernel_ref.ratio: an entry with a zero bound must be
    exactly zero)"""
    return np.array([kr.ratio(got[k], ref[k], bnd[k]) for k in range(len(got))])


# ------------------------------------------------------------------ designed queries
# sensor poses (q, t) body -> sensor: modest ones for pinhole entries (the point stays in front), wide ones for
# Kannala-Brandt entries (points beyond 90 degrees off the axis occur)
def _qt(axis, angle, t):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([np.sin(angle / 2) * a, [np.cos(angle / 2)], t])


SENSORS_PIN = (_qt((0, 1, 0), 0.2, (0.3, -0.1, 0.05)), _qt((1, 0, 0), -0.25, (-0.2, 0.15, 0.1)),
               _qt((1, 2, -1), 0.15, (0.05, 0.3, -0.1)), _qt((0, 0, 1), 0.3, (0.1, 0.1, 0.2)))
SENSORS_KB = (_qt((0, 1, 0), 1.75, (0.3, -0.1, 0.05)), _qt((1, 0, 0), -1.2, (-0.2, 0.15, 0.1)),
              _qt((1, 2, -1), 0.8, (0.05, 0.3, -0.1)), _qt((0, 1, 0), -2.0, (0.1, 0.1, 0.2)))
KB_COEFFS = (fd.K_TYP, fd.K_ZERO, fd.K_TYP2)
ENTRY_KINDS = ("identity", "rig", "kb_rig", "kb")      # of base query k: ENTRY_KINDS[(k // 3) % 4]; kind 2 + k % 3
WAVE = 64


def _entry(k, kind_name, Xb):
    """the table entry [17] of base query k: the first sensor pose of its list that keeps a pinhole's point in front
    (Z_s > 0.25 |Xs|) / a Kannala-Brandt point more than 0.2 rad off the negative optical axis"""
    e = np.zeros(17)
    e[:12] = rig_ref.IDENTITY12
    if kind_name in ("kb_rig", "kb"):
        e[12:16], e[16] = KB_COEFFS[k % 3], 1.0
    if kind_name in ("rig", "kb_rig"):
        cands = SENSORS_PIN if kind_name == "rig" else SENSORS_KB
        for j in range(len(cands)):
            ext = rig_ref.quat_to_ext(cands[(k + j) % len(cands)])
            Xs = ext[:9].reshape(3, 3) @ Xb + ext[9:]
            if (kind_name == "rig" and Xs[2] > 0.25 * np.linalg.norm(Xs)) or \
               (kind_name == "kb_rig" and np.arctan2(np.hypot(Xs[0], Xs[1]), Xs[2]) < np.pi - 0.2):
                e[:12] = ext
                return e
        raise AssertionError("no sensor pose of the list suits query %d" % k)
    return e


def designed_queries(des, inp):
    """the inputs of cugo_predict_observations on a design: the queries of pl_cov_ref.reprojection_inputs (inp) with a
    kind (2, 3, 4 in turn) and a table entry (ENTRY_KINDS in turn) each, and the hand-placed points of
    fisheye_designed.py seen from an identity pose appended to the poses through Kannala-Brandt entries with the
    identity sensor pose (Xs = X_l exactly) as free landmarks PREPENDED to the landmarks, twice: set A with K_TYP and
    the Sigma blocks of the first free-free queries; set B with K_ZERO, the pose FIXED and Sigma_ll = e_j e_j^T, j = 0, 1
    in turn, so that S = A[:, j] A[:, j]^T holds the squares of single entries of A — the small ones (x y c) among them,
    where a loss of digits in c is not covered by the large ones.  Ordered so that the first 64 queries — one wave
    — hold twelve free-free queries (every kind x entry), six each with a fixed pose, a fixed landmark and both (where
    the design has them) and set A.  Returns a dict: poses, lms, Lfree, lmcov, and per query ip, il, kind, cam, tab,
    Saa, Sal, Sll, free_p, free_l, q_aa, plus base [n] (the query's index in inp; -1 / -2 for a hand point of set A / B) and the census
    of the first wave"""
    f = des["f"]
    m = len(inp["ip"])
    H = len(fd.HAND_POINTS)
    hand = np.array(fd.HAND_POINTS, np.float64)
    poses = np.concatenate([f["poses"], [[0, 0, 0, 1, 0, 0, 0.0]]])
    lms = np.concatenate([hand, hand, f["lms"]])
    _, _, Xb, _ = frames(inp["pose"], inp["Xw"], np.float64)
    kind = 2 + np.arange(m) % 3
    names = [ENTRY_KINDS[(k // 3) % 4] for k in range(m)]
    tab = np.array([_entry(k, names[k], Xb[k]) for k in range(m)])
    free = np.flatnonzero(inp["free_p"] & inp["free_l"])
    assert len(free) >= 2 * H
    q = dict(ip=inp["ip"], il=inp["il"] + 2 * H, kind=kind, cam=inp["cam"], tab=tab, Saa=inp["Saa"], Sal=inp["Sal"],
             Sll=inp["Sll"], free_p=inp["free_p"], free_l=inp["free_l"], base=np.arange(m))
    onehot = np.zeros((H, 3, 3))
    onehot[np.arange(H), np.arange(H) % 2, np.arange(H) % 2] = 1.0
    lmcov = np.concatenate([inp["Sll"][free[:H]], onehot, inp["lmcov"]])
    parts = [q]
    for s_, coeff in ((0, fd.K_TYP), (1, fd.K_ZERO)):
        src = free[s_ * H:(s_ + 1) * H]
        e = np.zeros((H, 17))
        e[:, :12], e[:, 12:16], e[:, 16] = rig_ref.IDENTITY12, coeff, 1.0
        a = s_ == 0
        parts.append(dict(ip=np.full(H, len(f["poses"])), il=s_ * H + np.arange(H), kind=2 + np.arange(H) % 3,
                          cam=inp["cam"][src], tab=e, Saa=inp["Saa"][src] if a else np.full((H, 6, 6), np.nan),
                          Sal=inp["Sal"][src] if a else np.full((H, 6, 3), np.nan), Sll=inp["Sll"][free[:H]] if a else onehot,
                          free_p=np.full(H, a), free_l=np.ones(H, bool), base=np.full(H, -1 - s_)))
    allq = {k: np.concatenate([p[k] for p in parts]) for k in q}
    n = m + 2 * H
    fp, fl = allq["free_p"], allq["free_l"]
    pick = lambda sel, c: np.flatnonzero(sel)[:c]
    first = np.concatenate([pick(fp & fl & (allq["base"] >= 0), 12), pick(~fp & fl, 6), pick(fp & ~fl, 6), pick(~fp & ~fl, 6),
                            np.arange(m, m + H)])
    assert len(first) <= WAVE and len(np.unique(first)) == len(first)
    rest = np.setdiff1d(np.arange(n), first)
    order = np.concatenate([first, rest])
    out = {k: np.ascontiguousarray(v[order]) for k, v in allq.items()}
    out["q_aa"] = np.where(out["free_p"], np.arange(n), -1).astype(np.int32)
    out.update(poses=poses, lms=lms, Lfree=f["L"] + 2 * H, lmcov=lmcov, n=n, n_hand=H,
               pose=poses[out["ip"]], Xw=lms[out["il"]])
    w = slice(0, WAVE)
    fish = out["tab"][w, 16] != 0
    ident = np.all(out["tab"][w, :12] == rig_ref.IDENTITY12, axis=1)
    out["census"] = dict(pinhole_identity=int((~fish & ident).sum()), pinhole_rig=int((~fish & ~ident).sum()),
                         kb=int(fish.sum()), kb_rig=int((fish & ~ident).sum()), kinds=sorted(set(out["kind"][w].tolist())),
                         fixed_pose=int((~out["free_p"][w] & out["free_l"][w]).sum()),
                         fixed_lm=int((out["free_p"][w] & ~out["free_l"][w]).sum()),
                         both_fixed=int((~out["free_p"][w] & ~out["free_l"][w]).sum()),
                         hand=int((out["base"][w] < 0).sum()))
    return out


PER_QUERY = ("ip", "il", "kind", "cam", "tab", "Saa", "Sal", "Sll", "free_p", "free_l", "base", "pose", "Xw")


def subset(q, mask):
    """the designed queries selected by mask, in their order (q_aa renumbered: the blocks of Saa are per query)"""
    out = dict(q)
    for k in PER_QUERY:
        out[k] = np.ascontiguousarray(q[k][mask])
    out["n"] = len(out["ip"])
    out["q_aa"] = np.where(out["free_p"], np.arange(out["n"]), -1).astype(np.int32)
    return out


def without_hand_points(q):
    """the queries a pinhole at the pose can answer: the hand-placed points hold Z = 0"""
    return subset(q, q["base"] >= 0)


def predict_of(q, dtype=LD, order="terms", mut=None, table=True, n=None):
    """predict() on the first n designed queries; table=False: without the table (every camera a pinhole at the pose)"""
    s = slice(0, q["n"] if n is None else n)
    return predict(q["pose"][s], q["Xw"][s], q["cam"][s], q["kind"][s], q["tab"][s] if table else None, q["Saa"][s],
                   q["Sal"][s], q["Sll"][s], q["free_p"][s], q["free_l"][s], dtype, order, mut)
