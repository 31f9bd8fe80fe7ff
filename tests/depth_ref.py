"""Extended-precision reference of the build pass WITH the inverse-depth kind (flag bit 16), numpy,
test only.  kernel_ref.build restated with a kind per slot (mono, stereo, depth), a robust kernel per kind and the
inverse-depth weight k (s = sqrt(k)); it returns the dict kernel_ref.build returns (per-entry values, masses and term
counts, and the per-edge parts), so kernel_ref's references of the fused iteration (pose_schur, fused_stage_*,
end_to_end_parts) take it as their `ref`.

The depth row, in kernel_ref's x = X/Z, y = Y/Z form and the kernels' sign convention (the arrays hold -de/d.):
    e2     = s (1/Z - m_d)
    JP[2]  = (s/Z) (y, -x, 0, 0, 0, 1/Z)
    JL[2]j = (s/Z^2) R_2j
Rows 0 and 1, the weight and every sum are kernel_ref's.

Bounds: kernel_ref's (n + c) u mass with ITS constants.  c of the depth row, counted as kernel_ref's docstring counts
(1/Z carries 9, x and y 18, R_ij 4, Xc 8; s = sqrt(k) is one rounding, formed once on the host):
    e2     = s (1/Z - m_d)       1/Z 9, the subtraction 1, s 1, product 1                     -> 12  <= 21 (e_i)
    JP[2]  = (s/Z) y, (s/Z)/Z    s 1, 1/Z 9, product 1; y 18 (or 1/Z 9); product 1            -> 30  <= 40 (J_P)
    JL[2]j = (s/Z^2) R_2j        s 1, 1/Z 9 twice, two products; R 4; product 1               -> 26  <= 36 (J_L)
    w                            the stereo formula (three squares) on these residuals         -> 47, as there
so C_HPP, C_BP, C_HLL, C_BL, C_HPL and C_CHI, which are sums of these per-factor counts, cover the depth row: no new
constant.  Masses: |1/Z| -> aiz = aZ/Z^2, |y| -> ayn, |x| -> axn as in kernel_ref; ae2 = s (aiz + |m_d|);
aJP[2] = s aiz (ayn, axn, 0, 0, 0, aiz); aJL[2]j = s aiz^2 aR_2j.

`mut` names ONE deliberate mistake of an implementation (test_depth_ref_host.py shows that each breaks the bounds):
    "as_stereo"        a depth slot built as a stereo slot (residual, Jacobians, robust kernel)
    "as_mono"          a depth slot built as a mono slot: third row dropped
    "s_residual_only"  s applied to the residual but not to the Jacobian rows
    "flip_x"           JP[2][1] = +s x / Z
    "pose_pass_mono"   the record bit lost: Hpp and bp built from the mono rows, everything else right
"""
import numpy as np

import kernel_ref as kr

LD = kr.LD
STEREO, INACTIVE, DEPTH = 4, 8, 16
MUTATIONS = ("as_stereo", "as_mono", "s_residual_only", "flip_x", "pose_pass_mono")


def build(f, rk3, k=1.0, mut=None, dtype=LD):
    """rk3 = {"mono": (type, delta), "stereo": ..., "depth": ...}; k: the inverse-depth weight.  Slots with bit 16 are
    depth slots (never together with bit 4)"""
    dt = dtype
    E, P, L = f["E"], f["P"], f["L"]
    fl = f["flags"]
    assert not np.any((fl & STEREO != 0) & (fl & DEPTH != 0)), "a slot carries at most one of STEREO and DEPTH"
    real = (fl & INACTIVE) == 0
    ip, il = f["pose"], f["lm"]
    pose = np.asarray(f["poses"], dt)[ip]
    Xw = np.asarray(f["lms"], dt)[il]
    cam = np.asarray(f["cams"], dt)[f["cam_id"]]
    fx, fy, cx, cy, bf = (cam[:, i] for i in range(5))
    meas = np.asarray(f["meas"], dt).T
    omega = np.asarray(f["omega"], dt)
    st = (fl & STEREO) != 0
    dp = (fl & DEPTH) != 0
    rk_st, rk_dp = st.copy(), dp.copy()          # which robust kernel a slot takes
    if mut == "as_stereo":
        st, dp = st | dp, np.zeros(E, bool)
        rk_st, rk_dp = st, dp
    elif mut == "as_mono":
        dp = np.zeros(E, bool)
        rk_st, rk_dp = st, dp
    sd = np.sqrt(dt(k))
    sj = dt(1) if mut == "s_residual_only" else sd
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
    Xc = np.einsum("eij,ej->ei", R, Xw) + pose[:, 4:]
    aXc = np.einsum("eij,ej->ei", aR, np.abs(Xw)) + np.abs(pose[:, 4:])
    X, Y, Z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    iz = 1 / Z
    xn, yn = X * iz, Y * iz
    aiz = aXc[:, 2] * iz * iz
    axn, ayn = aXc[:, 0] * aiz, aXc[:, 1] * aiz
    zero = np.zeros(E, dt)
    s = st.astype(dt)
    d = dp.astype(dt)
    JP = np.zeros((E, 3, 6), dt); aJP = np.zeros((E, 3, 6), dt)
    JP[:, 0] = np.stack([fx * xn * yn, -fx * (1 + xn * xn), fx * yn, -fx * iz, zero, fx * xn * iz], 1)
    JP[:, 1] = np.stack([fy * (1 + yn * yn), -fy * xn * yn, -fy * xn, zero, -fy * iz, fy * yn * iz], 1)
    aJP[:, 0] = np.stack([fx * axn * ayn, fx * (1 + axn * axn), fx * ayn, fx * aiz, zero, fx * axn * aiz], 1)
    aJP[:, 1] = np.stack([fy * (1 + ayn * ayn), fy * axn * ayn, fy * axn, zero, fy * aiz, fy * ayn * aiz], 1)
    sx = -1 if mut != "flip_x" else 1
    JP[:, 2] = (s[:, None] * np.stack([JP[:, 0, 0] - bf * yn * iz, JP[:, 0, 1] + bf * xn * iz, JP[:, 0, 2], JP[:, 0, 3], zero,
                                       JP[:, 0, 5] - bf * iz * iz], 1) +
                d[:, None] * np.stack([sj * iz * yn, sx * sj * iz * xn, zero, zero, zero, sj * iz * iz], 1))
    aJP[:, 2] = (s[:, None] * np.stack([aJP[:, 0, 0] + bf * ayn * aiz, aJP[:, 0, 1] + bf * axn * aiz, aJP[:, 0, 2],
                                        aJP[:, 0, 3], zero, aJP[:, 0, 5] + bf * aiz * aiz], 1) +
                 d[:, None] * np.stack([sj * aiz * ayn, sj * aiz * axn, zero, zero, zero, sj * aiz * aiz], 1))
    JL = np.zeros((E, 3, 3), dt); aJL = np.zeros((E, 3, 3), dt)
    JL[:, 0] = -(fx * iz)[:, None] * (R[:, 0] - xn[:, None] * R[:, 2])
    JL[:, 1] = -(fy * iz)[:, None] * (R[:, 1] - yn[:, None] * R[:, 2])
    JL[:, 2] = s[:, None] * (JL[:, 0] - (bf * iz * iz)[:, None] * R[:, 2]) + d[:, None] * (sj * iz * iz)[:, None] * R[:, 2]
    aJL[:, 0] = (fx * aiz)[:, None] * (aR[:, 0] + axn[:, None] * aR[:, 2])
    aJL[:, 1] = (fy * aiz)[:, None] * (aR[:, 1] + ayn[:, None] * aR[:, 2])
    aJL[:, 2] = s[:, None] * (aJL[:, 0] + (bf * aiz * aiz)[:, None] * aR[:, 2]) + d[:, None] * (sj * aiz * aiz)[:, None] * aR[:, 2]
    pu, pv = fx * xn + cx, fy * yn + cy
    e = np.stack([pu - meas[:, 0], pv - meas[:, 1], s * ((pu - bf * iz) - meas[:, 2]) + d * (sd * (iz - meas[:, 2]))], 1)
    ae = np.stack([fx * axn + np.abs(cx) + np.abs(meas[:, 0]), fy * ayn + np.abs(cy) + np.abs(meas[:, 1]),
                   s * (fx * axn + np.abs(cx) + bf * aiz + np.abs(meas[:, 2])) + d * (sd * (aiz + np.abs(meas[:, 2])))], 1)
    xr = omega * (e * e).sum(1)
    xmass = omega * (np.abs(e) * (np.abs(e) + 2 * ae)).sum(1)
    rho, drho, d2rho = (np.zeros(E, dt) for _ in range(3))
    for sel, key in ((~rk_st & ~rk_dp, "mono"), (rk_st, "stereo"), (rk_dp, "depth")):
        r0, r1, r2 = kr._rho(int(rk3[key][0]), rk3[key][1], xr, dt)
        rho, drho, d2rho = np.where(sel, r0, rho), np.where(sel, r1, drho), np.where(sel, r2, d2rho)
    live = real.astype(dt)
    wgt = live * omega * drho
    awgt = live * (omega * drho + omega * d2rho * xmass)
    eb = np.abs(e) + ae
    JPp, aJPp = JP, aJP                          # the rows the pose pass (Hpp, bp) is built from
    if mut == "pose_pass_mono":
        JPp, aJPp = JP.copy(), aJP.copy()
        JPp[dp, 2] = 0
        aJPp[dp, 2] = 0
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
               Xc=Xc, R=R, e=e, JP=JPp, JL=JL, aJP=aJPp, aJL=aJL, eb=eb, aw=awgt,
               # per-edge chi (the per-edge chi pass): value and mass, n = 1
               chi_e=live * rho, chi_e_mass=live * (np.abs(rho) + xmass))
    npose = np.bincount(ip[pf], minlength=P)[:P]
    nlm = np.bincount(il[lf], minlength=L)[:L]
    out["Hpp_n"], out["bp_n"] = npose[:, None, None], npose[:, None]
    out["Hll_n"], out["bl_n"] = nlm[:, None, None], nlm[:, None]
    return out


KEYS = ("Hpp", "bp", "Hll", "bl", "Hpl", "chi")


def ratios(got, ref):
    """{output: largest error / bound} of a build `got` (a dict with KEYS, matrices as kernel_ref.build returns them)
    against the reference `ref`"""
    return {key: kr.ratio(got[key], ref[key], kr.bound(ref[key + "_n"], kr.BUILD_C[key], ref[key + "_mass"])) for key in KEYS}


def chi_e_ratio(got, ref):
    return kr.ratio(got, ref["chi_e"], kr.bound(1, kr.C_CHI, ref["chi_e_mass"]))
