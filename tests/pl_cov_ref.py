"""Extended-precision reference of the pose-landmark covariance kernels (k_pose_lm_cross and k_reprojection_cov of
cov_kernels.hip, reached through cugo_pose_landmark_cross_covariances and cugo_reprojection_covariances) with PER-ENTRY
error bounds (numpy, test only).

Sigma_al.  Written from the formula in np.longdouble.  For a free pose a and a free landmark l with Hll = L L^T (lower
Cholesky factor) and G_e = Hpl_e L^-T over the COUNTED edge slots of l (lm_cov_ref.counted_slots), in slot order,

    Sigma_al = -(sum_e Sigma_{a p(e)} G_e) L^-1                                      (6 x 3, rows a)

Sigma_{ab}: the 6 x 6 block (rows a, columns b) of the dense pose covariance handed in (data, fed identically to the
kernel: its own accuracy is not under test).  A query with a fixed vertex (index -1) is zero.  A non-positive or NaN
pivot of the 3 x 3 factorisation marks the query as failed: 18 zeros.  Nothing is read of a slot that does not count
except its flags.

Bound.  With every block comes
    mass = (sum_e |Sigma_{a p(e)}| |G_e|) |L^-1|,   |G_e| = |Hpl_e| |L^-1|^T
(the same expression without cancellation) and the number of summed terms n = 6 deg_counted.  The bound of an entry is

    K_PL (n + C_PL) u kappa_l mass,     u = 2^-53,  kappa_l = sqrt(cond_2(Hll)) = cond_2(L)

(the form of kappa_l: lm_cov_ref.py; L^-1 comes out of the same factorisation).  C_PL = 131 roundings on the longest
path, counted per formula as lm_cov_ref.py counts C_LM:
    L^-1 entries (lm_cov_ref)                                                                  -> 62
    G = Hpl L^-T  62 + product 1 + 2 additions -> 65;  Sigma G  65 + product 1 (the additions are n) -> 66
    (sum) L^-1    66 + 62 + product 1 + 2 additions                                            -> 131
Marginal landmarks (lm_cov_ref.chol3(..., marginal=)) may either fail or lie inside the bound.

K_PL is measured, not derived (test_pl_cov_host.py): 4 x the largest ratio that the float64 run of this same module
reaches against its longdouble run, in either of two summation orders (cross()), over the designs DESIGNS below with
the queries of queries(), rounded up.

S = J Sigma J^T (reprojection()).  Inputs in float64: the estimates, the camera, Sigma_aa, Sigma_al, Sigma_ll.  The
Jacobians are the formulas of kernel_ref.build (x = X/Z, y = Y/Z form, mono and stereo), restated here for one pose and
one landmark per query, with their masses (every sign a plus).  Per entry
    S_ij = sum_km JP_ik Saa_km JP_jm + sum_km (JP_ik Sal_km JL_jm + JP_jk Sal_km JL_im) + sum_km JL_ik Sll_km JL_jm
    mass = the same with the Jacobian masses and |Sigma|,  n = 36 + 2 x 18 + 9 = 81 summed terms,
    C_S = 82: two Jacobian entries of at most 40 roundings each (kernel_ref: J_P 40, J_L 36) and two products;
the bound of an entry is K_S (n + C_S) u mass, K_S by the same 4 x rule over the same designs, mono and stereo.

Measured where this was written (x86-64, 80-bit longdouble), worst ratio of the float64 replay per design in the units
above (the larger of the two summation orders), rounded up: REPLAY (Sigma_al) and REPLAY_S (S).
"""
import numpy as np

import kernel_ref as kr
import lm_cov_ref as lr

LD = kr.LD
assert np.finfo(LD).eps < 1e-18, "pl_cov_ref needs an extended-precision np.longdouble: eps = %g" % np.finfo(LD).eps
U = kr.U
C_PL = 131
C_S, N_S = 82, 81
DESIGNS = ("B", "B_padded", "mixed", "corners", "far", "grid513")
K_PL = 0.03    # 4 x 0.00705 (design `mixed`), rounded up
K_S = 0.13     # 4 x 0.0319 (design `mixed`, stereo), rounded up
# the fp64 replay's worst ratio per design (the larger of its two summation orders), rounded up (test_pl_cov_host.py):
# Sigma_al in units of (n + C_PL) u sqrt(cond) mass, S in units of (n + C_S) u mass
REPLAY = {"B": 0.0046, "B_padded": 0.0046, "mixed": 0.0071, "corners": 0.004, "far": 0.0044, "grid513": 0.0051}
REPLAY_S = {"B": 0.012, "B_padded": 0.012, "mixed": 0.032, "corners": 0.0059, "far": 0.00032, "grid513": 0.0072}


# ------------------------------------------------------------------ inputs shared by the tests
def dense_sigma(des, prior=0.0):
    """the dense pose covariance of a design of lm_cov_designed.py, [6 P, 6 P]: numpy.linalg.inv of the float64 Schur
    complement, symmetrised — what lm_cov_designed.schur_sigma cuts its pattern blocks from (the same expression)"""
    f, Hll, Hpl = des["f"], des["Hll"], des["Hpl"]
    import oracle
    import synth
    P = f["P"]
    b = kr.build(oracle.Problem(*synth.problem_fields(des["d"])), (0, 1.0), f)
    Hpp = np.asarray(b["Hpp"], np.float64)
    Hsc = np.zeros((6 * P, 6 * P))
    for p in range(P):
        Hsc[6 * p:6 * p + 6, 6 * p:6 * p + 6] = Hpp[p] + prior * np.eye(6)
    for l in range(f["L"]):
        es = lr.counted_slots(f, l)
        if len(es) == 0 or not np.linalg.cond(Hll[l]) < 1e13:
            continue
        A = Hpl[es].reshape(-1, 3)
        idx = (6 * f["pose"][es][:, None] + np.arange(6)).reshape(-1)
        Hsc[np.ix_(idx, idx)] -= A @ np.linalg.solve(Hll[l], A.T)
    Hsc = 0.5 * (Hsc + Hsc.T)
    S = np.linalg.inv(Hsc)
    return 0.5 * (S + S.T)


def queries(des):
    """(q_pose, q_lm): per free landmark a pose that observes it through a counted slot, a free pose that does not,
    pose 0 and pose P - 1 (each where there is one)"""
    f = des["f"]
    P = f["P"]
    qp, ql = [], []
    for l in range(f["L"]):
        ps = f["pose"][lr.counted_slots(f, l)]
        picks = []
        if len(ps):
            picks.append(int(ps[len(ps) // 2]))
        rest = np.setdiff1d(np.arange(P), ps)
        if len(rest):
            picks.append(int(rest[len(rest) // 2]))
        picks += [0, P - 1]
        qp += picks
        ql += [l] * len(picks)
    return np.array(qp, np.int32), np.array(ql, np.int32)


def block(Sigma, a, ps, dt):
    """[d, 6, 6]: Sigma_{a p} for p in ps"""
    rows = Sigma[6 * a:6 * a + 6]
    return np.asarray(rows.reshape(6, -1, 6)[:, np.asarray(ps, np.int64), :].transpose(1, 0, 2), dt)


# ------------------------------------------------------------------ Sigma_al
def cross(H, hpl, S, dt=LD, marginal=None, order="slots", mutate=None):
    """one query: (cov [6,3], mass [6,3]) from Hll [3,3], the Hpl blocks [d,6,3] and the pose blocks [d,6,6] of the
    counted slots in slot order; None when the factorisation fails.  order: "slots" (the terms Sigma_e G_e added one
    after the other in slot order) or "reversed" (G stacked to [6 d, 3] and one matrix product over the slots in
    reverse order).  mutate: one of the mistakes test_pl_cov_host.py plants — ("drop", e), ("transpose", e), "sign",
    "side" — None otherwise"""
    H = np.asarray(H, dt)
    Lf = lr.chol3(H, dt, marginal)
    if Lf is None:
        return None
    Li = lr.lower_inverse(Lf, dt)
    aLi = np.abs(Li)
    d = len(hpl)
    acc, am = np.zeros((6, 3), dt), np.zeros((6, 3), dt)
    if d:
        hpl, S = np.asarray(hpl, dt), np.asarray(S, dt)
        G = hpl @ Li.T
        aG = np.abs(hpl) @ aLi.T
        if isinstance(mutate, tuple) and mutate[0] == "transpose":
            S = S.copy()
            S[mutate[1]] = S[mutate[1]].T
        keep = np.ones(d, bool)
        if isinstance(mutate, tuple) and mutate[0] == "drop":
            keep[mutate[1]] = False
        T = np.einsum("ekl,elb->ekb", S, G)[keep]
        if order == "slots":
            acc = np.cumsum(np.concatenate([acc[None], T]), axis=0)[-1]
        else:
            Sr, Gr = S[keep][::-1], G[keep][::-1]
            acc = Sr.transpose(1, 0, 2).reshape(6, -1) @ Gr.reshape(-1, 3)
        am = np.einsum("ekl,elb->kb", np.abs(S), aG)
    cov = acc @ (Li.T if mutate == "side" else Li)
    return (cov if mutate == "sign" else -cov), am @ aLi


def reference(des, Sigma, qp, ql, dtype=LD, order="slots", hpl_all=False):
    """cov [n,6,3], mass [n,6,3], n [n], kappa [n], fail [n], marginal [n], deg [n] of the queries on design des with
    the dense pose covariance Sigma.  hpl_all: the mistake of reading every slot of the landmark, counted or not"""
    f, Hll, Hpl = des["f"], np.asarray(des["Hll"]), np.asarray(des["Hpl"])
    n = len(qp)
    cov, mass = np.zeros((n, 6, 3), dtype), np.zeros((n, 6, 3), dtype)
    fail, marginal = np.zeros(n, bool), np.zeros(n, bool)
    deg = np.zeros(n, np.int64)
    kappa = np.ones(n)
    for k in range(n):
        a, l = int(qp[k]), int(ql[k])
        if a < 0 or l < 0:
            continue
        es = np.arange(f["lm_ptr"][l], f["lm_ptr"][l + 1]) if hpl_all else lr.counted_slots(f, l)
        ps = np.minimum(f["pose"][es], f["P"] - 1)   # (hpl_all: a fixed pose has no block; any block shows the NaN)
        deg[k] = len(es)
        m = [False]
        r = cross(Hll[l], Hpl[es], block(Sigma, a, ps, dtype), dtype, m, order)
        marginal[k] = m[0]
        if r is None:
            fail[k] = True
        else:
            cov[k], mass[k] = r
            kappa[k] = np.linalg.cond(np.asarray(Hll[l], np.float64))
    return dict(cov=cov, mass=mass, n=6 * deg, kappa=kappa, fail=fail, marginal=marginal, deg=deg)


def unit(ref):
    """(n + C_PL) u sqrt(kappa) mass per entry [n,6,3]: the bound without K_PL"""
    return (np.asarray(ref["n"], LD) + C_PL)[:, None, None] * LD(U) * np.sqrt(np.asarray(ref["kappa"], LD))[:, None, None] \
        * np.asarray(ref["mass"], LD)


def bound(ref):
    return LD(K_PL) * unit(ref)


def ratios(got, ref, bnd):
    """per query: the largest |got - ref| / bound over the 18 entries (0 for failed queries, whose block must be exactly
    zero: inf otherwise; a marginal landmark may be either)"""
    got = np.asarray(got, LD).reshape(-1, 6, 3)
    out = np.zeros(len(got))
    for k in range(len(got)):
        if ref["marginal"][k] and not np.any(got[k] != 0):
            out[k] = 0.0
        elif ref["fail"][k]:
            out[k] = 0.0 if not np.any(got[k] != 0) else np.inf
        else:
            out[k] = kr.ratio(got[k], ref["cov"][k], bnd[k])
    return out


# ------------------------------------------------------------------ S = J Sigma J^T
def jacobians(pose, Xw, cam, stereo, dt=LD):
    """JP [n,3,6], JL [n,3,3] of the projection of Xw [n,3] in pose [n,7] (q, t) with cam [n,5], and their masses aJP,
    aJL: the formulas of kernel_ref.build; also the depth Z [n].  stereo [n] bool: the third row is zero for mono"""
    pose, Xw, cam = np.asarray(pose, dt), np.asarray(Xw, dt), np.asarray(cam, dt)
    E = len(pose)
    fx, fy, bf = cam[:, 0], cam[:, 1], cam[:, 4]
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
    Xc = np.einsum("eij,ej->ei", R, Xw) + pose[:, 4:]
    aXc = np.einsum("eij,ej->ei", aR, np.abs(Xw)) + np.abs(pose[:, 4:])
    X, Y, Z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    iz = 1 / Z
    xn, yn = X * iz, Y * iz
    aiz = aXc[:, 2] * iz * iz
    axn, ayn = aXc[:, 0] * aiz, aXc[:, 1] * aiz
    zero = np.zeros(E, dt)
    JP = np.zeros((E, 3, 6), dt); aJP = np.zeros((E, 3, 6), dt)
    JP[:, 0] = np.stack([fx * xn * yn, -fx * (1 + xn * xn), fx * yn, -fx * iz, zero, fx * xn * iz], 1)
    JP[:, 1] = np.stack([fy * (1 + yn * yn), -fy * xn * yn, -fy * xn, zero, -fy * iz, fy * yn * iz], 1)
    aJP[:, 0] = np.stack([fx * axn * ayn, fx * (1 + axn * axn), fx * ayn, fx * np.abs(aiz), zero, fx * axn * np.abs(aiz)], 1)
    aJP[:, 1] = np.stack([fy * (1 + ayn * ayn), fy * axn * ayn, fy * axn, zero, fy * np.abs(aiz), fy * ayn * np.abs(aiz)], 1)
    s = np.asarray(stereo, bool).astype(dt)
    JP[:, 2] = s[:, None] * np.stack([JP[:, 0, 0] - bf * yn * iz, JP[:, 0, 1] + bf * xn * iz, JP[:, 0, 2], JP[:, 0, 3], zero,
                                      JP[:, 0, 5] - bf * iz * iz], 1)
    aJP[:, 2] = s[:, None] * np.stack([aJP[:, 0, 0] + bf * ayn * aiz, aJP[:, 0, 1] + bf * axn * aiz, aJP[:, 0, 2], aJP[:, 0, 3],
                                       zero, aJP[:, 0, 5] + bf * aiz * aiz], 1)
    JL = np.zeros((E, 3, 3), dt); aJL = np.zeros((E, 3, 3), dt)
    JL[:, 0] = -(fx * iz)[:, None] * (R[:, 0] - xn[:, None] * R[:, 2])
    JL[:, 1] = -(fy * iz)[:, None] * (R[:, 1] - yn[:, None] * R[:, 2])
    JL[:, 2] = s[:, None] * (JL[:, 0] - (bf * iz * iz)[:, None] * R[:, 2])
    aJL[:, 0] = (fx * aiz)[:, None] * (aR[:, 0] + axn[:, None] * aR[:, 2])
    aJL[:, 1] = (fy * aiz)[:, None] * (aR[:, 1] + ayn[:, None] * aR[:, 2])
    aJL[:, 2] = s[:, None] * (aJL[:, 0] + (bf * aiz * aiz)[:, None] * aR[:, 2])
    return JP, np.abs(aJP), JL, np.abs(aJL), Z


def reprojection(pose, Xw, cam, stereo, Saa, Sal, Sll, free_p, free_l, dtype=LD, order="terms"):
    """S [n,3,3] and its mass [n,3,3] from the float64 inputs of n queries: pose [n,7], Xw [n,3], cam [n,5], stereo [n],
    Saa [n,6,6], Sal [n,6,3], Sll [n,3,3]; free_p / free_l [n]: a fixed pose drops the terms with J_p, a fixed landmark
    those with J_l.  order: "terms" (the four parts one after the other) or "joint" (one 9 x 9 product J Sigma J^T)"""
    dt = dtype
    JP, aJP, JL, aJL, _ = jacobians(pose, Xw, cam, stereo, dt)
    fp, fl = np.asarray(free_p, bool).astype(dt)[:, None, None], np.asarray(free_l, bool).astype(dt)[:, None, None]
    JP, aJP, JL, aJL = JP * fp, aJP * fp, JL * fl, aJL * fl
    Saa, Sal, Sll = (np.nan_to_num(np.asarray(a, dt)) for a in (Saa, Sal, Sll))
    if order == "terms":
        X = np.einsum("nik,nkm,njm->nij", JP, Sal, JL)
        S = np.einsum("nik,nkm,njm->nij", JP, Saa, JP) + X + X.transpose(0, 2, 1) + np.einsum("nik,nkm,njm->nij", JL, Sll, JL)
    else:
        J = np.concatenate([JP, JL], 2)
        Sig = np.concatenate([np.concatenate([Saa, Sal], 2), np.concatenate([Sal.transpose(0, 2, 1), Sll], 2)], 1)
        S = J @ Sig @ J.transpose(0, 2, 1)
    aX = np.einsum("nik,nkm,njm->nij", aJP, np.abs(Sal), aJL)
    mass = np.einsum("nik,nkm,njm->nij", aJP, np.abs(Saa), aJP) + aX + aX.transpose(0, 2, 1) + \
        np.einsum("nik,nkm,njm->nij", aJL, np.abs(Sll), aJL)
    return S, mass


def reprojection_inputs(des, Sigma, qp, ql, ref):
    """the inputs of the reprojection reference for the queries of a design: every query as mono and as stereo; then
    the first 40 with the pose replaced by a fixed one, with the landmark replaced by a fixed one, and with both (where
    the design has fixed vertices)"""
    f = des["f"]
    n = len(qp)
    lmref = lr.reference(f, des["rowptr"], des["colind"], des["Hll"], des["Hpl"], des["sigma"])
    Sll = np.asarray(lmref["cov"], np.float64)[ql]
    Saa = np.array([Sigma[6 * a:6 * a + 6, 6 * a:6 * a + 6] for a in qp]).reshape(n, 6, 6)
    Sal = np.asarray(ref["cov"], np.float64)
    ok = ~(ref["fail"] | ref["marginal"] | lmref["fail"][ql] | lmref["marginal"][ql])
    ip, il = qp.astype(np.int64)[ok], ql.astype(np.int64)[ok]
    Saa, Sal, Sll = Saa[ok], Sal[ok], Sll[ok]
    m = len(ip)
    free_p, free_l = np.ones(m, bool), np.ones(m, bool)
    parts = [(ip, il, Saa, Sal, Sll, free_p, free_l)]
    k = min(m, 40)
    nfp, nfl = f["Pall"] - f["P"], f["Lall"] - f["L"]
    if nfp:
        fixp = f["P"] + np.arange(k) % nfp
        parts.append((fixp, il[:k], np.full((k, 6, 6), np.nan), np.full((k, 6, 3), np.nan), Sll[:k], ~free_p[:k], free_l[:k]))
    if nfl:
        fixl = f["L"] + np.arange(k) % nfl
        parts.append((ip[:k], fixl, Saa[:k], np.full((k, 6, 3), np.nan), np.full((k, 3, 3), np.nan), free_p[:k], ~free_l[:k]))
    if nfp and nfl:
        parts.append((fixp, fixl, np.full((k, 6, 6), np.nan), np.full((k, 6, 3), np.nan), np.full((k, 3, 3), np.nan),
                      ~free_p[:k], ~free_l[:k]))
    ip, il, Saa, Sal, Sll, free_p, free_l = (np.concatenate([p[i] for p in parts]) for i in range(7))
    m = len(ip)
    two = lambda a: np.concatenate([a, a])
    stereo = np.concatenate([np.zeros(m, bool), np.ones(m, bool)])
    cam = f["cams"][np.arange(2 * m) % len(f["cams"])]
    return dict(lmcov=np.asarray(lmref["cov"], np.float64), ip=two(ip), il=two(il), pose=f["poses"][two(ip)], Xw=f["lms"][two(il)], cam=cam, stereo=stereo, Saa=two(Saa),
                Sal=two(Sal), Sll=two(Sll), free_p=two(free_p), free_l=two(free_l))


def reprojection_of(inp, dtype=LD, order="terms"):
    return reprojection(inp["pose"], inp["Xw"], inp["cam"], inp["stereo"], inp["Saa"], inp["Sal"], inp["Sll"],
                           inp["free_p"], inp["free_l"], dtype, order)


def unit_s(mass):
    return LD(N_S + C_S) * LD(U) * np.asarray(mass, LD)


def bound_s(mass):
    return LD(K_S) * unit_s(mass)
