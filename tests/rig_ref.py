"""Extended-precision reference of the build pass WITH camera extrinsics (a rig; cugo_edges.has_rig, DESIGN.md section
18), numpy, test only.  kernel_ref.build / depth_ref.build restated with a fixed sensor pose per camera-table entry,
f["cam_ext"] [n_cams][12] = {M row-major, t_s} (body -> sensor), selected by the slot's camera index.  It returns the dict
kernel_ref.build returns (per-entry values, masses and term counts, and the per-edge parts; "Xc" is the BODY-frame
point, which is what the 64-byte record holds), so kernel_ref's references of the fused iteration take it as `ref`.

The term, in the kernels' sign convention (the arrays hold -de/d.):
    Xb = R(q) Xw + t,   Xs = M Xb + t_s,   e = proj(Xs) - meas  (stereo third row with bf, at Xs)
    A  = -de/dXs:  A0 = (-fx/Z, 0, fx x/Z),  A1 = (0, -fy/Z, fy y/Z),  stereo A2 = A0 - (0, 0, bf/Z^2)   (x = Xs/Zs, ...)
    B  = A M,   JP[:, 3:6] = B,   JP[:, 0:3] = -B [Xb]x,   JL = B R(q)
(the left update T_b <- exp([w, v]) T_b moves Xb by w x Xb + v).  test_rig_ref_host.py checks JP and JL against central
differences in longdouble.

Bounds: (n + c) u mass per entry, c counted as kernel_ref's docstring counts (R_ij 4, Xb_i 8 there):
    Xs_i = sum_j M_ij Xb_j + ts_i   Xb 8, product 1, 3 additions                                   -> 12   (Xc: 8)
    1/Zs 13;  x = Xs/Zs              12 + 13 + 1                                                    -> 26   (18)
    A entries                        (fx/Z) x: (1 + 13) + 26 + 1 = 41; stereo row one more          -> 42
    B = A M                          A 42, product 1, 2 additions                                   -> 45
    J_P entries                      columns 3..5: B, 45; columns 0..2: B 45 + Xb 8 + product 1 + subtraction 1
                                                                                                    -> 55   (40)
    J_L = B R                        B 45 + R 4 + product 1 + 2 additions                           -> 52   (36)
    e_i                              26 + 3                                                         -> 29   (21)
    w                                2 x 29 + 5                                                     -> 63   (47)
    Hpp 63 + 55 + 55 + 4 = 177 (131);  bp 63 + 55 + 29 + 4 = 151 (112);  Hll 63 + 52 + 52 + 4 = 171 (123);
    bl 63 + 52 + 29 + 4 = 148 (108);   Hpl 63 + 55 + 52 + 4 = 174 (127); chi 2 x 29 + 1 + 2 + 1 + 6 = 68 (52)
Every count exceeds kernel_ref's, so the rig reference has constants of its own (BUILD_C below); kernel_ref's are
untouched.  The fused iteration, counted as kernel_ref counts it above C_LINE_Y:
    A = JL L^-T 55;  A A^T 113;  N = w I - w^2 A A^T: (2 x 63 + 1) + 113 + 1 + 1 = 242
    JP^T N JP  242 + 55 + 3 + 55 + 3 + 1 -> C_PS_H = 359 (265);  bp = C_BP -> C_PS_BP = 151 (112)
    u = w (e - A y): (55 + 3), 63 + 58 + 1, 1 = 123;  bsc += JP^T u: 123 + 55 + 3 -> C_PS_BSC = 181 (134)
Masses: aXb as kernel_ref; aXs = |M| aXb + |t_s|; aiz = aZs / Zs^2, ax = aXs aiz, ay = aYs aiz; aA is A with these and
plus signs; aB = aA |M|; aJP[:, 3:6] = aB, aJP[:, 0:3] = aB |[aXb]x|; aJL = aB aR; the residual's mass |proj| + |meas|.

`mut` names ONE deliberate mistake of an implementation (test_rig_ref_host.py shows that each breaks the bounds):
    "ext_ignored"      slot built with M = I, t_s = 0
    "jac_at_Xs"        rotation columns of JP formed with [Xs]x instead of [Xb]x
    "M_transposed"     M^T in the place of M
    "JL_without_M"     JL = A R
    "ts_dropped"       rotation applied, lever arm not
    "stride5"          extrinsic k read at 5 k of the flat table (the stride of the camera table), wrapping at its end
    "pose_pass_plain"  Hpp and bp from the record without the extrinsic (the plain Jacobian at Xb), everything else right
"""
import numpy as np

import kernel_ref as kr

LD = kr.LD
STEREO, INACTIVE = 4, 8
MUTATIONS = ("ext_ignored", "jac_at_Xs", "M_transposed", "JL_without_M", "ts_dropped", "stride5", "pose_pass_plain")
C_HPP, C_BP, C_HLL, C_BL, C_HPL, C_CHI = 177, 151, 171, 148, 174, 68
C_PS_H, C_PS_BP, C_PS_BSC = 359, 151, 181
BUILD_C = dict(Hpp=C_HPP, bp=C_BP, Hll=C_HLL, bl=C_BL, Hpl=C_HPL, chi=C_CHI)
IDENTITY12 = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)


def quat_to_ext(q_t7):
    """{M row-major, t} of a sensor pose (qx, qy, qz, qw, tx, ty, tz), the quaternion normalised: float64, as the
    host's flattening forms it"""
    q = np.asarray(q_t7, np.float64)
    inv = 1.0 / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])      # (the host's operations, in its order)
    x, y, z, w = q[:4] * inv
    return np.array([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y), q[4], q[5], q[6]])


def _cross_cols(B, X, sign):
    """columns 0..2 of -B [X]x (sign = -1: the values; +1: the masses, every sign a plus)"""
    return np.stack([B[:, :, 2] * X[:, None, 1] + sign * B[:, :, 1] * X[:, None, 2],
                     B[:, :, 0] * X[:, None, 2] + sign * B[:, :, 2] * X[:, None, 0],
                     B[:, :, 1] * X[:, None, 0] + sign * B[:, :, 0] * X[:, None, 1]], 2)


def build(f, rk2, mut=None, dtype=LD):
    """rk2 = {"mono": (type, delta), "stereo": ...}; f["cam_ext"] [n_cams][12]"""
    dt = dtype
    E, P, L = f["E"], f["P"], f["L"]
    fl = f["flags"]
    real = (fl & INACTIVE) == 0
    ip, il = f["pose"], f["lm"]
    pose = np.asarray(f["poses"], dt)[ip]
    Xw = np.asarray(f["lms"], dt)[il]
    cid = np.asarray(f["cam_id"], np.int64)
    cam = np.asarray(f["cams"], dt)[cid]
    fx, fy, cx, cy, bf = (cam[:, i] for i in range(5))
    table = np.asarray(f["cam_ext"], dt)
    assert table.shape == (len(f["cams"]), 12)
    if mut == "stride5":
        flat = table.ravel()
        ext = flat[(5 * cid[:, None] + np.arange(12)[None, :]) % len(flat)]
    else:
        ext = table[cid]
    M, ts = ext[:, :9].reshape(E, 3, 3), ext[:, 9:]
    if mut == "ext_ignored":
        M, ts = np.broadcast_to(np.eye(3, dtype=dt), (E, 3, 3)), np.zeros((E, 3), dt)
    elif mut == "M_transposed":
        M = M.transpose(0, 2, 1)
    elif mut == "ts_dropped":
        ts = np.zeros((E, 3), dt)
    aM = np.abs(M)
    meas = np.asarray(f["meas"], dt).T
    omega = np.asarray(f["omega"], dt)
    st = (fl & STEREO) != 0
    x, y, z, w = (pose[:, i] for i in range(4))
    R = np.empty((E, 3, 3), dt)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - z * w); R[:, 0, 2] = 2 * (x * z + y * w)
    R[:, 1, 0] = 2 * (x * y + z * w); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - x * w)
    R[:, 2, 0] = 2 * (x * z - y * w); R[:, 2, 1] = 2 * (y * z + x * w); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    ax_, ay_, az_, aw_ = (np.abs(pose[:, i]) for i in range(4))
    aR = np.empty((E, 3, 3), dt)
    aR[:, 0, 0] = 1 + 2 * (ay_ * ay_ + az_ * az_); aR[:, 0, 1] = 2 * (ax_ * ay_ + az_ * aw_); aR[:, 0, 2] = 2 * (ax_ * az_ + ay_ * aw_)
    aR[:, 1, 0] = aR[:, 0, 1]; aR[:, 1, 1] = 1 + 2 * (ax_ * ax_ + az_ * az_); aR[:, 1, 2] = 2 * (ay_ * az_ + ax_ * aw_)
    aR[:, 2, 0] = aR[:, 0, 2]; aR[:, 2, 1] = aR[:, 1, 2]; aR[:, 2, 2] = 1 + 2 * (ax_ * ax_ + ay_ * ay_)
    Xb = np.einsum("eij,ej->ei", R, Xw) + pose[:, 4:]
    aXb = np.einsum("eij,ej->ei", aR, np.abs(Xw)) + np.abs(pose[:, 4:])
    Xs = np.einsum("eij,ej->ei", M, Xb) + ts
    aXs = np.einsum("eij,ej->ei", aM, aXb) + np.abs(ts)
    iz = 1 / Xs[:, 2]
    xn, yn = Xs[:, 0] * iz, Xs[:, 1] * iz
    aiz = aXs[:, 2] * iz * iz
    axn, ayn = aXs[:, 0] * aiz, aXs[:, 1] * aiz
    zero = np.zeros(E, dt)
    s = st.astype(dt)
    A = np.zeros((E, 3, 3), dt); aA = np.zeros((E, 3, 3), dt)
    A[:, 0] = np.stack([-fx * iz, zero, fx * xn * iz], 1)
    A[:, 1] = np.stack([zero, -fy * iz, fy * yn * iz], 1)
    A[:, 2] = s[:, None] * np.stack([A[:, 0, 0], zero, A[:, 0, 2] - bf * iz * iz], 1)
    aA[:, 0] = np.stack([fx * aiz, zero, fx * axn * aiz], 1)
    aA[:, 1] = np.stack([zero, fy * aiz, fy * ayn * aiz], 1)
    aA[:, 2] = s[:, None] * np.stack([aA[:, 0, 0], zero, aA[:, 0, 2] + bf * aiz * aiz], 1)
    B = np.einsum("emk,ekj->emj", A, M)
    aB = np.einsum("emk,ekj->emj", aA, aM)
    Xr, aXr = (Xs, aXs) if mut == "jac_at_Xs" else (Xb, aXb)
    JP = np.concatenate([_cross_cols(B, Xr, -1), B], 2)
    aJP = np.concatenate([_cross_cols(aB, aXr, 1), aB], 2)
    JL = np.einsum("emk,ekj->emj", A if mut == "JL_without_M" else B, R)
    aJL = np.einsum("emk,ekj->emj", aA if mut == "JL_without_M" else aB, aR)
    pu, pv = fx * xn + cx, fy * yn + cy
    e = np.stack([pu - meas[:, 0], pv - meas[:, 1], s * ((pu - bf * iz) - meas[:, 2])], 1)
    ae = np.stack([fx * axn + np.abs(cx) + np.abs(meas[:, 0]), fy * ayn + np.abs(cy) + np.abs(meas[:, 1]),
                   s * (fx * axn + np.abs(cx) + bf * aiz + np.abs(meas[:, 2]))], 1)
    xr = omega * (e * e).sum(1)
    xmass = omega * (np.abs(e) * (np.abs(e) + 2 * ae)).sum(1)
    rho, drho, d2rho = (np.zeros(E, dt) for _ in range(3))
    for sel, key in ((~st, "mono"), (st, "stereo")):
        r0, r1, r2 = kr._rho(int(rk2[key][0]), rk2[key][1], xr, dt)
        rho, drho, d2rho = np.where(sel, r0, rho), np.where(sel, r1, drho), np.where(sel, r2, d2rho)
    live = real.astype(dt)
    wgt = live * omega * drho
    awgt = live * (omega * drho + omega * d2rho * xmass)
    eb = np.abs(e) + ae
    JPp, aJPp = JP, aJP                          # the rows the pose pass (Hpp, bp) is built from
    if mut == "pose_pass_plain":
        plain = build(f, rk2, mut="ext_ignored", dtype=dt)
        JPp, aJPp = plain["JP"], plain["aJP"]
    tHpp = wgt[:, None, None] * np.einsum("emr,emc->erc", JPp, JPp)
    mHpp = awgt[:, None, None] * np.einsum("emr,emc->erc", aJPp, aJPp)
    tbp = wgt[:, None] * np.einsum("emr,em->er", JPp, e)
    mbp = awgt[:, None] * np.einsum("emr,em->er", aJPp, eb)
    tHll = wgt[:, None, None] * np.einsum("emr,emc->erc", JL, JL)
    mHll = awgt[:, None, None] * np.einsum("emr,emc->erc", aJL, aJL)
    tbl = wgt[:, None] * np.einsum("emr,em->er", JL, e)
    mbl = awgt[:, None] * np.einsum("emr,em->er", aJL, eb)
    ff = ((fl & 11) == 0).astype(dt)
    Hpl = (ff * wgt)[:, None, None] * np.einsum("emr,emc->erc", JP, JL)
    mHpl = (ff * awgt)[:, None, None] * np.einsum("emr,emc->erc", aJP, aJL)
    pf = real & (ip < P)
    lf = real & (il < L)
    out = dict(Hpp=kr._scatter(ip[pf], tHpp[pf], P), Hpp_mass=kr._scatter(ip[pf], mHpp[pf], P),
               bp=kr._scatter(ip[pf], tbp[pf], P), bp_mass=kr._scatter(ip[pf], mbp[pf], P),
               Hll=kr._scatter(il[lf], tHll[lf], L), Hll_mass=kr._scatter(il[lf], mHll[lf], L),
               bl=kr._scatter(il[lf], tbl[lf], L), bl_mass=kr._scatter(il[lf], mbl[lf], L),
               Hpl=Hpl, Hpl_mass=mHpl, Hpl_n=np.ones((E, 1, 1)),
               chi=(live * rho).sum(), chi_mass=(live * (np.abs(rho) + xmass)).sum(), chi_n=int(real.sum()),
               w=wgt, x=xr, f=f,
               Xc=Xb, Xs=Xs, R=R, e=e, JP=JPp, JL=JL, aJP=aJPp, aJL=aJL, eb=eb, aw=awgt,
               chi_e=live * rho, chi_e_mass=live * (np.abs(rho) + xmass))
    npose = np.bincount(ip[pf], minlength=P)[:P]
    nlm = np.bincount(il[lf], minlength=L)[:L]
    out["Hpp_n"], out["bp_n"] = npose[:, None, None], npose[:, None]
    out["Hll_n"], out["bl_n"] = nlm[:, None, None], nlm[:, None]
    return out


KEYS = ("Hpp", "bp", "Hll", "bl", "Hpl", "chi")


def bound_of(ref, key, consts=None):
    return kr.bound(ref[key + "_n"], (consts or BUILD_C)[key], ref[key + "_mass"])


def ratios(got, ref, consts=None):
    """{output: largest error / bound} of a build `got` (a dict with KEYS, matrices as build returns them) against the
    reference `ref`; consts: BUILD_C, or kernel_ref.BUILD_C for the bounds of the plain reference"""
    return {key: kr.ratio(got[key], ref[key], bound_of(ref, key, consts)) for key in KEYS}


def chi_e_ratio(got, ref, c=C_CHI):
    return kr.ratio(got, ref["chi_e"], kr.bound(1, c, ref["chi_e_mass"]))


def fused_stage_G(got_G, ref, f, got_Linv, f32=False):
    """kernel_ref.fused_stage_G with the rig reference's C_HPL"""
    _, Li, _ = kr._per_edge_lines(f, got_Linv, np.zeros((max(f["L"], 1), 3)), LD)
    bH = kr.bound(1, C_HPL, ref["Hpl_mass"])
    G, _ = kr.fused_G(ref["Hpl"], Li)
    _, Gm = kr.fused_G(np.abs(ref["Hpl"]) + bH, Li)
    bnd = np.einsum("erm,ecm->erc", bH, np.abs(Li)) + kr.bound(3, kr.C_G, Gm)
    if f32:
        bnd = bnd + LD(2.0 ** -24) * (np.abs(G) + bnd)
    return kr.ratio(got_G, G, bnd)


def fused_stage_pose(got_Hd, got_bp, got_bsc, ps, damp_lam=0.0):
    """kernel_ref.fused_stage_pose with the rig reference's C_PS_*"""
    I6 = damp_lam * np.eye(6, dtype=LD)
    return dict(diag=kr.ratio(got_Hd, ps["Hd"] + I6, kr.bound(ps["Hd_n"], C_PS_H, ps["Hd_mass"] + I6)),
                bp=kr.ratio(got_bp, ps["bp"], kr.bound(ps["bp_n"], C_PS_BP, ps["bp_mass"])),
                bsc=kr.ratio(got_bsc, ps["bsc"], kr.bound(ps["bsc_n"], C_PS_BSC, ps["bsc_mass"])))


def adjoint(ext12, dtype=LD):
    """Ad = [[M, 0], [[t_s]x M, M]] (order [w, v]) of a sensor pose {M, t_s}: the body twist as the sensor sees it"""
    e = np.asarray(ext12, dtype)
    M, t = e[:9].reshape(3, 3), e[9:]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], dtype)
    Ad = np.zeros((6, 6), dtype)
    Ad[:3, :3] = M
    Ad[3:, :3] = tx @ M
    Ad[3:, 3:] = M
    return Ad
