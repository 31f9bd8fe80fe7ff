"""Extended-precision reference of the COVARIANCE form of the two point kinds (generalised ICP: cugo_gicp_edges,
cugo_gicp_pair_edges; point_term.h: cov_information) with PER-ENTRY error bounds, on top of tests/point_edge_ref.py and
tests/point_pair_ref.py (numpy, test only).

A set is the dict of point_edge_ref (pose, p, z, active, rk) or point_pair_ref (a, b, p, z, active, rk) with cov_p6,
cov_z6 [E,6] or [1,6] (upper triangles, row-major packed 00 01 02 11 12 22: the arrays the device is given) in place of
info6.  With M = R (unary) or M = R_b R_a^T (pair):
    S = C_z + M C_p M^T,  Omega = S^-1
and everything else is the information form's term with this Omega: the reference forms Omega in np.longdouble (adjugate
over the determinant, from the longdouble M) and hands it, unrounded, to point_terms / pair_terms as info6.

The bound
---------
Each summed output keeps the (n + c) u mass bound of the information form (C_POINT, C_PAIR: the roundings AFTER Omega,
whose mass takes |Omega_ij|).  What the device's Omega_e differs from the exact one by adds, to first order, the term of a
perturbation dOmega_e with
    |dOmega_e| <= C_OMEGA u D_e,   D_e = |Omega_e| (|C_z| + aM |C_p| aM^T) |Omega_e|     entrywise
(aM the cancellation-free |M|: aR of pose_edge_ref._rot, aRb aRa^T for the pair), pushed through the term:
    x:      rb^T D rb =: xD                                  (rb = |r| + ar as in the information form)
    chi:    rho' xD
    H:      rho' aJ1^T D aJ2 + |rho''| xD aJ1^T |Omega| aJ2
    b:      rho' aJ^T D rb   + |rho''| xD aJ^T |Omega| rb
summed over the edges of an entry like its mass ("extra").  bound = (n + c) u mass + C_OMEGA u extra.

C_OMEGA is measured, not derived: omega_replay() below evaluates the device's operation order in float64 (quat_to_rot, M,
T = M C_p, the upper triangle of S, L L^T, L^-1, L^-T L^-1) and c_omega_ratio() takes the largest |Omega_f64 - Omega| /
(u D) over every class of tests/gicp_designed.py; test_gicp_ref_host.py asserts that 4 x that maximum (the margin this
repository uses for K_x and K_s) is what stands here:
    observed maximum 4.12 (class 'iso'; 'gicp' 3.7, 'rank2_p' 3.1, 'zero_p' 2.8, 'aligned' with kappa(S) ~ 1e6 1.5)
    ->  C_OMEGA = 17 >= 4 x 4.2
(the kernels invert through L L^T: the adjugate in float64 loses this componentwise bound on ill-conditioned S.)
"""
import numpy as np

import point_edge_ref as ptr_ref
import point_pair_ref as ppr
from kernel_ref import LD, U, bound, ratio, _rho, _scatter  # noqa: F401
from point_edge_ref import pack, unpack
from pose_edge_ref import _rot, _skew_neg

C_OMEGA = 17
C_OMEGA_OBSERVED = 4.2          # the largest ratio c_omega_ratio() has seen (asserted within 4 x in test_gicp_ref_host.py)
OMEGA_MUTATIONS = ("M_identity", "M_transposed", "cov_swapped")


# ------------------------------------------------------------------ Omega
def _cov(e, key, E, dt):
    return unpack(np.broadcast_to(np.asarray(e[key], dt).reshape(-1, 6), (E, 6)))


def _inv_ld(S):
    """adjugate / determinant of symmetric [E,3,3] (longdouble: the reference's inverse)"""
    a, b, c, d, e, f = S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]
    A, B, Cc = d * f - e * e, c * e - b * f, b * e - c * d
    det = a * A + b * B + c * Cc
    D, Ee, F = a * f - c * c, b * c - a * e, a * d - b * b
    out = np.empty_like(S)
    out[:, 0, 0], out[:, 0, 1], out[:, 0, 2] = A / det, B / det, Cc / det
    out[:, 1, 0], out[:, 1, 1], out[:, 1, 2] = B / det, D / det, Ee / det
    out[:, 2, 0], out[:, 2, 1], out[:, 2, 2] = Cc / det, Ee / det, F / det
    return out


def omega_ref(M, aM, Cp, Cz, mut=None):
    """Omega [E,3,3] and D = |Omega| (|C_z| + aM |C_p| aM^T) |Omega| in the dtype of M.  mut: one of OMEGA_MUTATIONS"""
    if mut == "M_identity":
        M = np.broadcast_to(np.eye(3, dtype=M.dtype), M.shape)
    elif mut == "M_transposed":
        M = M.transpose(0, 2, 1)
    elif mut == "cov_swapped":
        Cp, Cz = Cz, Cp
    S = Cz + np.einsum("eik,ekl,ejl->eij", M, Cp, M)
    S = (S + S.transpose(0, 2, 1)) / 2
    Om = _inv_ld(S)
    Sa = np.abs(Cz) + np.einsum("eik,ekl,ejl->eij", aM, np.abs(Cp), aM)
    D = np.einsum("eik,ekl,elj->eij", np.abs(Om), Sa, np.abs(Om))
    return Om, D


def quat_to_rot64(q):
    """ba_math.h quat_to_rot, operation by operation, float64 [E,4] -> [E,3,3]"""
    q = np.asarray(q, np.float64)
    x, y, z, w = (q[:, k] for k in range(4))
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.empty((len(q), 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - (tyy + tzz), txy - twz, txz + twy
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = txy + twz, 1 - (txx + tzz), tyz - twx
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = txz - twy, tyz + twx, 1 - (txx + tyy)
    return R


def pair_rotation64(Ra, Rb):
    """point_pair_kernels.hip pair_rotation: M_ij = Rb_i0 Ra_j0 + Rb_i1 Ra_j1 + Rb_i2 Ra_j2, in that order"""
    M = np.empty_like(Ra)
    for i in range(3):
        for j in range(3):
            M[:, i, j] = Rb[:, i, 0] * Ra[:, j, 0] + Rb[:, i, 1] * Ra[:, j, 1] + Rb[:, i, 2] * Ra[:, j, 2]
    return M


def omega_replay(M, Cp, Cz, mut=None):
    """point_term.h cov_information in float64, operation by operation: [E,3,3] each -> Omega [E,3,3] exactly symmetric"""
    M, Cp, Cz = (np.asarray(a, np.float64) for a in (M, Cp, Cz))
    if mut == "M_identity":
        M = np.broadcast_to(np.eye(3), M.shape)
    elif mut == "M_transposed":
        M = M.transpose(0, 2, 1)
    elif mut == "cov_swapped":
        Cp, Cz = Cz, Cp
    T = np.empty_like(Cp)
    for i in range(3):
        for j in range(3):
            T[:, i, j] = M[:, i, 0] * Cp[:, 0, j] + M[:, i, 1] * Cp[:, 1, j] + M[:, i, 2] * Cp[:, 2, j]
    s = lambda i, j: Cz[:, i, j] + (T[:, i, 0] * M[:, j, 0] + T[:, i, 1] * M[:, j, 1] + T[:, i, 2] * M[:, j, 2])
    s00, s01, s02, s11, s12, s22 = s(0, 0), s(0, 1), s(0, 2), s(1, 1), s(1, 2), s(2, 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        l00 = np.sqrt(s00)
        i00 = 1.0 / l00
        l10, l20 = s01 * i00, s02 * i00
        l11 = np.sqrt(s11 - l10 * l10)
        i11 = 1.0 / l11
        l21 = (s12 - l20 * l10) * i11
        l22 = np.sqrt(s22 - l20 * l20 - l21 * l21)
        i22 = 1.0 / l22
        i10 = -(l10 * i00) * i11
        i21 = -(l21 * i11) * i22
        i20 = -(l20 * i00 + l21 * i10) * i22
    O = np.empty_like(Cp)
    O[:, 0, 0] = i00 * i00 + i10 * i10 + i20 * i20
    O[:, 0, 1] = O[:, 1, 0] = i10 * i11 + i20 * i21
    O[:, 0, 2] = O[:, 2, 0] = i20 * i22
    O[:, 1, 1] = i11 * i11 + i21 * i21
    O[:, 1, 2] = O[:, 2, 1] = i21 * i22
    O[:, 2, 2] = i22 * i22
    return O


def _rotations(poses, e, dt):
    """(M, aM) of every edge of a unary or pair set, in dt"""
    P = np.asarray(poses, dt)
    if "pose" in e:
        return _rot(P[np.asarray(e["pose"], int), :4])
    Ra, aRa = _rot(P[np.asarray(e["a"], int), :4])
    Rb, aRb = _rot(P[np.asarray(e["b"], int), :4])
    return np.einsum("eik,ejk->eij", Rb, Ra), np.einsum("eik,ejk->eij", aRb, aRa)


def n_edges(e):
    return len(e["pose"] if "pose" in e else e["a"])


def omega_of(poses, e, mut=None):
    """the reference's Omega and D [E,3,3] (longdouble) of a set at `poses`"""
    E = n_edges(e)
    M, aM = _rotations(poses, e, LD)
    return omega_ref(M, aM, _cov(e, "cov_p6", E, LD), _cov(e, "cov_z6", E, LD), mut)


def omega_of_replay(poses, e, mut=None):
    """the device's Omega [E,3,3] (float64, its operation order) of a set at `poses`"""
    E = n_edges(e)
    P = np.asarray(poses, np.float64)
    if "pose" in e:
        M = quat_to_rot64(P[np.asarray(e["pose"], int), :4])
    else:
        M = pair_rotation64(quat_to_rot64(P[np.asarray(e["a"], int), :4]), quat_to_rot64(P[np.asarray(e["b"], int), :4]))
    return omega_replay(M, _cov(e, "cov_p6", E, np.float64), _cov(e, "cov_z6", E, np.float64), mut)


def with_info(e, Om):
    """the information-form set of `e` with the given Omega [E,3,3] (any dtype: it is not rounded here)"""
    out = {k: v for k, v in e.items() if k not in ("cov_p6", "cov_z6")}
    out["info6"] = pack(Om)
    return out


def c_omega_ratio(poses, e):
    """largest |Omega_replay - Omega| / (u D) over the edges of a set"""
    Om, D = omega_of(poses, e)
    got = omega_of_replay(poses, e).astype(LD)
    return float((np.abs(got - Om) / (LD(U) * D)).max())


# ------------------------------------------------------------------ the extra term of the bound
def _kernel_derivs(e, x):
    kind, delta = int(e["rk"][0]), e["rk"][1]
    _, drho, d2rho = _rho(kind, delta, x, LD)
    return drho, np.abs(d2rho)


def _push(aJ1, aJ2, rb, D, aOm, drho, d2rho, lv):
    """the first-order term of dOmega through H (aJ1, aJ2 given) or b (aJ2 = None)"""
    xD = np.einsum("ei,eij,ej->e", rb, D, rb)
    if aJ2 is None:
        return (lv * drho)[:, None] * np.einsum("eka,ekl,el->ea", aJ1, D, rb) + \
            (lv * d2rho * xD)[:, None] * np.einsum("eka,ekl,el->ea", aJ1, aOm, rb)
    return (lv * drho)[:, None, None] * np.einsum("eka,ekl,elc->eac", aJ1, D, aJ2) + \
        (lv * d2rho * xD)[:, None, None] * np.einsum("eka,ekl,elc->eac", aJ1, aOm, aJ2)


# ------------------------------------------------------------------ the unary kind
def point_build(poses, n_free, e, full=True, mut=None):
    """point_edge_ref.point_build with the Omega of the covariances at `poses`, plus X_extra for every output"""
    E = n_edges(e)
    Om, D = omega_of(poses, e, mut)
    ref = ptr_ref.point_build(poses, n_free, with_info(e, Om), full=full)
    pose = np.asarray(e["pose"], int)
    P7 = np.asarray(poses, LD)[pose]
    R, aR = _rot(P7[:, :4])
    p, z, t = np.asarray(e["p"], LD).reshape(E, 3), np.asarray(e["z"], LD).reshape(E, 3), P7[:, 4:]
    y = np.einsum("eij,ej->ei", R, p) + t
    ay = np.einsum("eij,ej->ei", aR, np.abs(p)) + np.abs(t)
    rb = np.abs(y - z) + ay + np.abs(z)
    I3 = np.broadcast_to(np.eye(3, dtype=LD), (E, 3, 3))
    aJ = np.concatenate([np.abs(_skew_neg(ay)), I3], 2)
    live = (pose < n_free) & np.asarray(e["active"], bool)
    lv = live.astype(LD)
    x = np.maximum(0, np.einsum("ei,eij,ej->e", y - z, Om, y - z))
    drho, d2rho = _kernel_derivs(e, x)
    xD = np.einsum("ei,eij,ej->e", rb, D, rb)
    chi_x = lv * drho * xD
    P = n_free
    q = pose[live]
    ref["chi_edge_extra"], ref["chi_extra"] = chi_x, chi_x.sum()
    ref["chi_pose_extra"] = _scatter(q, chi_x[live], P)
    if full:
        ref["H_extra"] = _scatter(q, _push(aJ, aJ, rb, D, np.abs(Om), drho, d2rho, lv)[live], P)
        ref["b_extra"] = _scatter(q, _push(aJ, None, rb, D, np.abs(Om), drho, d2rho, lv)[live], P)
    ref["Omega"], ref["D"] = Om, D
    return ref


def point_bound(ref, key):
    return ptr_ref.point_bound(ref, key) + C_OMEGA * LD(U) * np.asarray(ref[key + "_extra"], LD)


def point_replay(poses, n_free, n_poses_total, e, mut=None):
    """point_edge_ref.point_replay fed the device-order Omega.  mut: one of OMEGA_MUTATIONS (or None)"""
    return ptr_ref.point_replay(poses, n_free, n_poses_total, with_info(e, omega_of_replay(poses, e, mut)))


# ------------------------------------------------------------------ the pair kind
def pair_build(poses, n_free, n_poses_total, e, mut=None):
    """point_pair_ref.pair_build with the Omega of the covariances at `poses`, plus X_extra for every output"""
    E, Pall = n_edges(e), n_poses_total
    Om, D = omega_of(poses, e, mut)
    ref = ppr.pair_build(poses, n_free, n_poses_total, with_info(e, Om))
    a, b = np.asarray(e["a"], int), np.asarray(e["b"], int)
    Pa, Pb = np.asarray(poses, LD)[a], np.asarray(poses, LD)[b]
    Ra, aRa = _rot(Pa[:, :4])
    Rb, aRb = _rot(Pb[:, :4])
    p, z = np.asarray(e["p"], LD).reshape(E, 3), np.asarray(e["z"], LD).reshape(E, 3)
    ta, tb = Pa[:, 4:], Pb[:, 4:]
    X = np.einsum("eji,ej->ei", Ra, p - ta)
    aX = np.einsum("eji,ej->ei", aRa, np.abs(p) + np.abs(ta))
    y = np.einsum("eij,ej->ei", Rb, X) + tb
    ay = np.einsum("eij,ej->ei", aRb, aX) + np.abs(tb)
    aM = np.einsum("eik,ejk->eij", aRb, aRa)
    r = y - z
    rb = np.abs(r) + ay + np.abs(z)
    I3 = np.broadcast_to(np.eye(3, dtype=LD), (E, 3, 3))
    aJb = np.concatenate([np.abs(_skew_neg(ay)), I3], 2)
    aJa = np.einsum("eij,ejk->eik", aM, np.concatenate([np.abs(_skew_neg(p)), I3], 2))
    fa, fb = a < n_free, b < n_free
    live = (fa | fb) & np.asarray(e["active"], bool)
    x = np.maximum(0, np.einsum("ei,eij,ej->e", r, Om, r))
    drho, d2rho = _kernel_derivs(e, x)
    aOm = np.abs(Om)
    push = lambda J1, J2, m: _push(J1, J2, rb, D, aOm, drho, d2rho, (live & m).astype(LD))
    ref["H_extra"] = _scatter(a, push(aJa, aJa, fa), Pall) + _scatter(b, push(aJb, aJb, fb), Pall)
    ref["b_extra"] = _scatter(a, push(aJa, None, fa), Pall) + _scatter(b, push(aJb, None, fb), Pall)
    ff = live & fa & fb
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = lo * Pall + hi
    pairs = np.unique(key[ff])
    idx = np.searchsorted(pairs, key[ff])
    Hab_x = push(aJa, aJb, fa & fb)[ff]
    blk = np.where((a > b)[ff][:, None, None], Hab_x.transpose(0, 2, 1), Hab_x)
    ref["Hoff_extra"] = _scatter(idx, blk, len(pairs))
    chi_x = live.astype(LD) * drho * np.einsum("ei,eij,ej->e", rb, D, rb)
    ref["chi_edge_extra"], ref["chi_extra"] = chi_x, chi_x.sum()
    ref["Omega"], ref["D"] = Om, D
    return ref


def pair_bound(ref, key):
    return ppr.pair_bound(ref, key) + C_OMEGA * LD(U) * np.asarray(ref[key + "_extra"], LD)


def pair_replay(poses, n_free, n_poses_total, e, mut=None):
    """point_pair_ref.pair_replay fed the device-order Omega.  mut: one of OMEGA_MUTATIONS, or 'role0_twice' (role 0
    takes Omega' = M^T Omega M and then rotates it into a's frame once more)"""
    Om = omega_of_replay(poses, e, mut if mut in OMEGA_MUTATIONS else None)
    out = ppr.pair_replay(poses, n_free, n_poses_total, with_info(e, Om))
    if mut == "role0_twice":
        P = np.asarray(poses, np.float64)
        M = pair_rotation64(quat_to_rot64(P[np.asarray(e["a"], int), :4]), quat_to_rot64(P[np.asarray(e["b"], int), :4]))
        Om2 = np.einsum("eki,ekl,elj->eij", M, Om, M)
        Om2 = (Om2 + Om2.transpose(0, 2, 1)) / 2
        # H and b of a pose are the sums of both sides: replace the a-side share by the wrong one
        ea = dict(with_info(e, Om), active=np.asarray(e["active"], bool))
        ta, tw = ppr.pair_terms(poses, n_free, ea, np.float64), ppr.pair_terms(poses, n_free, with_info(e, Om2), np.float64)
        a = np.asarray(e["a"], int)
        H = out[0] + _scatter(a, tw["Haa"] - ta["Haa"], n_poses_total)
        b = out[1] + _scatter(a, tw["ba"] - ta["ba"], n_poses_total)
        return (H, b) + tuple(out[2:])
    return out
