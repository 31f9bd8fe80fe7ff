"""Extended-precision reference of the build pass WITH a distortion table (radial-tangential lens distortion;
cugo_edges.has_rig = 3), numpy, test only.  rig_ref.build restated with a distortion per
camera-table entry: f["cam_tab"] [n_cams][18] = {M row-major (9), t_s (3), k1, k2, p1, p2, k3, flag}, selected by the
slot's camera index; flag 0 is the pinhole of rig_ref (stereo third row included), flag 1 a distorted entry.  It returns
the dict rig_ref.build returns ("Xc" is the BODY-frame point), so kernel_ref's references of the fused iteration take it
as `ref`.

The term of a distorted entry at Xs = (x, y, z) = M Xb + t_s, in the kernels' sign convention:
    iz = 1 / z,  a = x iz,  b = y iz,  r2 = a^2 + b^2
    rad = 1 + r2 (k1 + r2 (k2 + r2 k3)),   dr = d rad / d r2 = k1 + r2 (2 k2 + 3 k3 r2)
    a' = a rad + 2 p1 a b + p2 (r2 + 2 a^2),   b' = b rad + p1 (r2 + 2 b^2) + 2 p2 a b
    e = (fx a' + cx - mu, fy b' + cy - mv, 0)
    Jaa = rad + 2 a^2 dr + 2 p1 b + 6 p2 a,  Jab = 2 a b dr + 2 p1 a + 2 p2 b,  Jbb = rad + 2 b^2 dr + 6 p1 b + 2 p2 a
    A = -de/dXs:  A0 = -fx iz (Jaa, Jab, -(Jaa a + Jab b)),  A1 = -fy iz (Jab, Jbb, -(Jab a + Jbb b)),  A2 = 0
    B = A M,   JP[:, 3:6] = B,   JP[:, 0:3] = -B [Xb]x,   JL = B R(q)
A distorted entry has two rows; the stereo bit of a slot on it is not looked at for them (it still picks the robust
kernel, as the kernels' launchers do for every table).  test_distort_ref_host.py checks A against central differences
in longdouble and against a known answer in exact rationals.

Bounds: (n + c) u mass per entry.  c counted as rig_ref's docstring counts (a product: the operands' counts + 1; a sum:
the larger count + 1, the masses added; a coefficient 0; Xs_i 12 there).  No transcendental: no ulp assumption.
    iz = 1 / z           12 + 1                                                                        ->   13
    a = x iz, b          12 + 13 + 1                                                                   ->   26
    a a, b b, a b        26 + 26 + 1                                                                   ->   53
    r2 = a a + b b       53 + 1                                                                        ->   54
    rad                  Horner: k3 r2 55, + k2 56, r2: 111, + k1 112, r2: 167, 1 +                    ->  168
    dr                   3 k3: 1, r2: 56, + 2 k2: 57, r2: 112, + k1                                    ->  113
    a', b'               a rad: 26 + 168 + 1 = 195; + 2 p1 a b (55): 196; + p2 (r2 + 2 a a) (56)       ->  197
    e_i                  fx a': 198; + cx, - m                                                         ->  200
    Jaa, Jbb             2 a a: 54; dr: 168; rad +: 169; + 2 p1 b (28): 170; + 6 p2 a (28)             ->  171   (Jab 170)
    A entries            fu = -(fx iz): 14;  fu Jaa: 186;  Jaa a: 198, + Jab b: 199, fu: 14 + 199 + 1  ->  214
    B = A M              214 + 1 + 2                                                                   ->  217
    J_P entries          columns 0..2: B 217 + Xb 8 + product 1 + subtraction 1                        ->  227
    J_L = B R            217 + 4 + 1 + 2                                                               ->  224
    w                    2 x 200 + 5                                                                   ->  405
    Hpp 405 + 2 x 227 + 4 = 863;  bp 405 + 227 + 200 + 4 = 836;  Hll 405 + 2 x 224 + 4 = 857;
    bl 405 + 224 + 200 + 4 = 833;  Hpl 405 + 227 + 224 + 4 = 860;  chi 2 x 200 + 1 + 2 + 1 + 6 = 410
Every count exceeds rig_ref's, and an undistorted entry of a distortion table is held to these too (one constant per
output); a table of undistorted entries only is compared with rig_ref.build itself (test_distort_ref_host.py).  The
fused iteration, counted as rig_ref counts it:
    A = JL L^-T 227;  A A^T 457;  N = w I - w^2 A A^T: (2 x 405 + 1) + 457 + 1 + 1 = 1270
    JP^T N JP  1270 + 227 + 3 + 227 + 3 + 1 -> C_PS_H = 1731;  bp -> C_PS_BP = 836
    u = w (e - A y): (227 + 3), 405 + 230 + 1, 1 = 637;  bsc += JP^T u: 637 + 227 + 3 -> C_PS_BSC = 867
Masses of a distorted entry: aXb, aXs as rig_ref.  A quantity q(Xs) gets  |terms of q| + sum_i |dq/dXs_i| aXs_i: the
first part carries q's own roundings (the formulas above with |a|, |b|, |k_j|, |p_j| and every sign a plus, so that a
radial factor that changes sign has its cancellation inside the bound), the second the 12 u aXs the point arrives with.
de/dXs = -A is exact; dA/dXs is formed by central differences in longdouble (a mass needs two digits).  From there on as
rig_ref: aB = aA |M|, aJP[:, 0:3] = aB |[aXb]x|, aJL = aB aR.

`mut` names ONE deliberate mistake of an implementation (test_distort_ref_host.py shows that each breaks the bounds):
    "p_swapped"        p1 and p2 swapped
    "two_dropped"      the factor 2 in 2 p1 a b (and in 2 p2 a b) of the residual dropped
    "six_as_two"       the 6 written as 2 in Jaa and Jbb
    "dr_without_k3"    k3 dropped from dr only (rad right)
    "dr_by_r"          dr taken with respect to r instead of r2 (2 r times too large)
    "pixel_units"      the distortion applied in pixel units: to (fx a, fy b) instead of (a, b)
    "A3_pinhole"       the third column of A formed from the undistorted (a, b) without J
    "stereo_kept"      the stereo row kept on a distorted entry (for a slot that carries the stereo bit)
    "stride17"         entry k read at 17 k of the flat table (the model table's stride), wrapping at its end
    "neighbour_flag"   the flag of entry k + 1 (wrapping)
"""
import numpy as np

import kernel_ref as kr

LD = kr.LD
STEREO, INACTIVE = 4, 8
MUTATIONS = ("p_swapped", "two_dropped", "six_as_two", "dr_without_k3", "dr_by_r", "pixel_units", "A3_pinhole",
             "stereo_kept", "stride17", "neighbour_flag")
STRIDE = 18
C_HPP, C_BP, C_HLL, C_BL, C_HPL, C_CHI = 863, 836, 857, 833, 860, 410
C_PS_H, C_PS_BP, C_PS_BSC = 1731, 836, 867
BUILD_C = dict(Hpp=C_HPP, bp=C_BP, Hll=C_HLL, bl=C_BL, Hpl=C_HPL, chi=C_CHI)
IDENTITY12 = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)
KEYS = ("Hpp", "bp", "Hll", "bl", "Hpl", "chi")


def dist_table(ext12, dist5, flags=None):
    """[n][18] from ext12 [n][12], dist5 [n][5] = (k1, k2, p1, p2, k3) and flags [n] (None: coefficients not all zero)"""
    d = np.asarray(dist5, np.float64).reshape(-1, 5)
    fl = np.any(d != 0, axis=1).astype(np.float64) if flags is None else np.asarray(flags, np.float64)
    return np.ascontiguousarray(np.concatenate([np.asarray(ext12, np.float64), d, fl[:, None]], 1))


def dist_terms(Xs, d, dt, mut=None):
    """a, b, a', b', Jaa, Jab, Jbb, iz at Xs [E][3] with coefficients d [E][5], and the sums of the absolute values of
    the terms of a', b', Jaa, Jab, Jbb"""
    one = dt(1)
    k1, k2, p1, p2, k3 = (d[:, i] for i in range(5))
    if mut == "p_swapped":
        p1, p2 = p2, p1
    iz = one / Xs[:, 2]
    a, b = Xs[:, 0] * iz, Xs[:, 1] * iz

    def terms(a, b, k1, k2, p1, p2, k3, mut):
        a2, b2, ab = a * a, b * b, a * b
        r2 = a2 + b2
        rad = one + r2 * (k1 + r2 * (k2 + r2 * k3))
        dr = k1 + r2 * (2 * k2 + 3 * k3 * r2)
        if mut == "dr_without_k3":
            dr = k1 + r2 * (2 * k2)
        if mut == "dr_by_r":
            dr = 2 * np.sqrt(r2) * dr
        two = 1 if mut == "two_dropped" else 2
        six = 2 if mut == "six_as_two" else 6
        ad = a * rad + two * p1 * ab + p2 * (r2 + 2 * a2)
        bd = b * rad + p1 * (r2 + 2 * b2) + two * p2 * ab
        Jaa = rad + 2 * a2 * dr + 2 * p1 * b + six * p2 * a
        Jab = 2 * ab * dr + 2 * p1 * a + 2 * p2 * b
        Jbb = rad + 2 * b2 * dr + six * p1 * b + 2 * p2 * a
        return ad, bd, Jaa, Jab, Jbb

    val = terms(a, b, k1, k2, p1, p2, k3, mut)
    mass = terms(np.abs(a), np.abs(b), np.abs(k1), np.abs(k2), np.abs(p1), np.abs(p2), np.abs(k3), None)
    return (a, b) + val + (iz,), mass


def dist_A(Xs, fx, fy, d, dt, mut=None):
    """A = -d(pu, pv)/dXs [E][3][3] (third row zero), the sums of the absolute values of its terms, (a', b') and the
    sums of the absolute values of their terms"""
    (a, b, ad, bd, Jaa, Jab, Jbb, iz), (ad_a, bd_a, Jaa_a, Jab_a, Jbb_a) = dist_terms(Xs, d, dt, mut)
    n = len(a)
    fu, fv = -(fx * iz), -(fy * iz)
    A = np.zeros((n, 3, 3), dt)
    T = np.zeros((n, 3, 3), dt)
    A[:, 0] = np.stack([fu * Jaa, fu * Jab, -(fu * (Jaa * a + Jab * b))], 1)
    A[:, 1] = np.stack([fv * Jab, fv * Jbb, -(fv * (Jab * a + Jbb * b))], 1)
    if mut == "A3_pinhole":
        A[:, 0, 2], A[:, 1, 2] = -(fu * a), -(fv * b)
    aa, ab_, aiz = np.abs(a), np.abs(b), np.abs(iz)
    T[:, 0] = np.stack([fx * aiz * Jaa_a, fx * aiz * Jab_a, fx * aiz * (Jaa_a * aa + Jab_a * ab_)], 1)
    T[:, 1] = np.stack([fy * aiz * Jab_a, fy * aiz * Jbb_a, fy * aiz * (Jab_a * aa + Jbb_a * ab_)], 1)
    return A, T, (ad, bd), (ad_a, bd_a)


def dist_A_mass(Xs, aXs, fx, fy, d):
    """|terms of A| + sum_i |dA/dXs_i| aXs_i, longdouble, the derivative by central differences (step 2^-26 of |Xs|)"""
    Xs, aXs, fx, fy, d = (np.asarray(x, LD) for x in (Xs, aXs, fx, fy, d))
    T = dist_A(Xs, fx, fy, d, LD)[1]
    h = LD(2.0 ** -26) * np.sqrt((Xs * Xs).sum(1))
    mass = T
    for i in range(3):
        s = np.zeros_like(Xs); s[:, i] = h
        plus, minus = dist_A(Xs + s, fx, fy, d, LD)[0], dist_A(Xs - s, fx, fy, d, LD)[0]
        mass = mass + np.abs(plus - minus) / (2 * h)[:, None, None] * aXs[:, i][:, None, None]
    return mass


def _cross_cols(B, X, sign):
    """columns 0..2 of -B [X]x (sign = -1: the values; +1: the masses, every sign a plus)"""
    return np.stack([B[:, :, 2] * X[:, None, 1] + sign * B[:, :, 1] * X[:, None, 2],
                     B[:, :, 0] * X[:, None, 2] + sign * B[:, :, 2] * X[:, None, 0],
                     B[:, :, 1] * X[:, None, 0] + sign * B[:, :, 0] * X[:, None, 1]], 2)


def build(f, rk2, mut=None, dtype=LD):
    """rk2 = {"mono": (type, delta), "stereo": ...}; f["cam_tab"] [n_cams][18]"""
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
    table = np.asarray(f["cam_tab"], dt)
    n_cams = len(f["cams"])
    assert table.shape == (n_cams, STRIDE)
    if mut == "stride17":
        flat = table.ravel()
        ent = flat[(17 * cid[:, None] + np.arange(STRIDE)[None, :]) % len(flat)]
    else:
        ent = table[cid]
    M, ts, dd = ent[:, :9].reshape(E, 3, 3), ent[:, 9:12], ent[:, 12:17]
    dist = ent[:, 17] != 0
    if mut == "neighbour_flag":
        dist = table[(cid + 1) % n_cams, 17] != 0
    aM = np.abs(M)
    meas = np.asarray(f["meas"], dt).T
    omega = np.asarray(f["omega"], dt)
    bit = (fl & STEREO) != 0                      # picks the robust kernel, on every entry
    st = bit & ~dist                              # has the third row
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
    zero = np.zeros(E, dt)
    s = st.astype(dt)
    # ---- the pinhole, as rig_ref ----
    with np.errstate(all="ignore"):
        iz = 1 / Xs[:, 2]
        xn, yn = Xs[:, 0] * iz, Xs[:, 1] * iz
        aiz = aXs[:, 2] * iz * iz
        axn, ayn = aXs[:, 0] * aiz, aXs[:, 1] * aiz
        A = np.zeros((E, 3, 3), dt); aA = np.zeros((E, 3, 3), dt)
        A[:, 0] = np.stack([-fx * iz, zero, fx * xn * iz], 1)
        A[:, 1] = np.stack([zero, -fy * iz, fy * yn * iz], 1)
        A[:, 2] = s[:, None] * np.stack([A[:, 0, 0], zero, A[:, 0, 2] - bf * iz * iz], 1)
        aA[:, 0] = np.stack([fx * aiz, zero, fx * axn * aiz], 1)
        aA[:, 1] = np.stack([zero, fy * aiz, fy * ayn * aiz], 1)
        aA[:, 2] = s[:, None] * np.stack([aA[:, 0, 0], zero, aA[:, 0, 2] + bf * aiz * aiz], 1)
        pu, pv = fx * xn + cx, fy * yn + cy
        e = np.stack([pu - meas[:, 0], pv - meas[:, 1], s * ((pu - bf * iz) - meas[:, 2])], 1)
        ae = np.stack([fx * axn + np.abs(cx) + np.abs(meas[:, 0]), fy * ayn + np.abs(cy) + np.abs(meas[:, 1]),
                       s * (fx * axn + np.abs(cx) + bf * aiz + np.abs(meas[:, 2]))], 1)
    # ---- distorted entries ----
    if np.any(dist):
        D = dist
        kmut = mut if mut in ("p_swapped", "two_dropped", "six_as_two", "dr_without_k3", "dr_by_r", "A3_pinhole") else None
        with np.errstate(all="ignore"):
            Ad, _, (ad, bd), (ad_a, bd_a) = dist_A(Xs[D], fx[D], fy[D], dd[D], dt, kmut)
            aAd = dist_A_mass(Xs[D], aXs[D], fx[D], fy[D], dd[D]).astype(dt)
            Ad0 = dist_A(*(np.asarray(v, LD) for v in (Xs[D], fx[D], fy[D], dd[D])), LD)[0]
            if mut == "pixel_units":            # the same polynomial on (fx a, fy b)
                pix = np.stack([fx[D] * Xs[D, 0] / Xs[D, 2], fy[D] * Xs[D, 1] / Xs[D, 2], np.ones(int(D.sum()), dt)], 1)
                (_, _, adp, bdp, _, _, _, _), _ = dist_terms(pix, dd[D], dt)
                pud, pvd = adp + cx[D], bdp + cy[D]
            else:
                pud, pvd = fx[D] * ad + cx[D], fy[D] * bd + cy[D]
        ed = np.stack([pud - meas[D, 0], pvd - meas[D, 1], zero[D]], 1)
        lever = (np.abs(Ad0) * np.asarray(aXs[D], LD)[:, None, :]).sum(2).astype(dt)         # sum_i |de_m/dXs_i| aXs_i
        aed = np.stack([fx[D] * ad_a + np.abs(cx[D]) + np.abs(meas[D, 0]) + lever[:, 0],
                        fy[D] * bd_a + np.abs(cy[D]) + np.abs(meas[D, 1]) + lever[:, 1], zero[D]], 1)
        if mut == "stereo_kept":                 # the pinhole's third row stays where the slot carries the bit
            keep = bit[D].astype(dt)
            with np.errstate(all="ignore"):
                Ad[:, 2] = keep[:, None] * np.stack([-fx[D] * iz[D], zero[D], fx[D] * xn[D] * iz[D] - bf[D] * iz[D] * iz[D]], 1)
                ed[:, 2] = keep * ((pud - bf[D] * iz[D]) - meas[D, 2])
        A, aA, e, ae = A.copy(), aA.copy(), e.copy(), ae.copy()
        A[D], aA[D], e[D], ae[D] = Ad, aAd, ed, aed
    B = np.einsum("emk,ekj->emj", A, M)
    aB = np.einsum("emk,ekj->emj", aA, aM)
    JP = np.concatenate([_cross_cols(B, Xb, -1), B], 2)
    aJP = np.concatenate([_cross_cols(aB, aXb, 1), aB], 2)
    JL = np.einsum("emk,ekj->emj", B, R)
    aJL = np.einsum("emk,ekj->emj", aB, aR)
    xr = omega * (e * e).sum(1)
    xmass = omega * (np.abs(e) * (np.abs(e) + 2 * ae)).sum(1)
    rho_, drho, d2rho = (np.zeros(E, dt) for _ in range(3))
    for sel, key in ((~bit, "mono"), (bit, "stereo")):
        r0, r1, r2 = kr._rho(int(rk2[key][0]), rk2[key][1], xr, dt)
        rho_, drho, d2rho = np.where(sel, r0, rho_), np.where(sel, r1, drho), np.where(sel, r2, d2rho)
    # (selected, not multiplied: an inactive slot of the layouts may sit anywhere behind a sensor pose)
    wgt = np.where(real, omega * drho, 0)
    awgt = np.where(real, omega * drho + omega * d2rho * xmass, 0)
    eb = np.abs(e) + ae
    dead = ~real
    if np.any(dead):                             # 0 x (inf or nan) of a slot that does not count
        JP, JL, aJP, aJL, e, eb = (np.where(dead.reshape((E,) + (1,) * (a.ndim - 1)), 0, a)
                                   for a in (JP, JL, aJP, aJL, e, eb))
    tHpp = wgt[:, None, None] * np.einsum("emr,emc->erc", JP, JP)
    mHpp = awgt[:, None, None] * np.einsum("emr,emc->erc", aJP, aJP)
    tbp = wgt[:, None] * np.einsum("emr,em->er", JP, e)
    mbp = awgt[:, None] * np.einsum("emr,em->er", aJP, eb)
    tHll = wgt[:, None, None] * np.einsum("emr,emc->erc", JL, JL)
    mHll = awgt[:, None, None] * np.einsum("emr,emc->erc", aJL, aJL)
    tbl = wgt[:, None] * np.einsum("emr,em->er", JL, e)
    mbl = awgt[:, None] * np.einsum("emr,em->er", aJL, eb)
    ff = ((fl & 11) == 0).astype(dt)
    Hpl = (ff * wgt)[:, None, None] * np.einsum("emr,emc->erc", JP, JL)
    mHpl = (ff * awgt)[:, None, None] * np.einsum("emr,emc->erc", aJP, aJL)
    pf = real & (ip < P)
    lf = real & (il < L)
    chi_e = np.where(real, rho_, 0)
    chi_e_mass = np.where(real, np.abs(rho_) + xmass, 0)
    out = dict(Hpp=kr._scatter(ip[pf], tHpp[pf], P), Hpp_mass=kr._scatter(ip[pf], mHpp[pf], P),
               bp=kr._scatter(ip[pf], tbp[pf], P), bp_mass=kr._scatter(ip[pf], mbp[pf], P),
               Hll=kr._scatter(il[lf], tHll[lf], L), Hll_mass=kr._scatter(il[lf], mHll[lf], L),
               bl=kr._scatter(il[lf], tbl[lf], L), bl_mass=kr._scatter(il[lf], mbl[lf], L),
               Hpl=Hpl, Hpl_mass=mHpl, Hpl_n=np.ones((E, 1, 1)),
               chi=chi_e.sum(), chi_mass=chi_e_mass.sum(), chi_n=int(real.sum()),
               w=wgt, x=xr, f=f, dist=dist, A=A,
               Xc=Xb, Xs=Xs, R=R, e=e, JP=JP, JL=JL, aJP=aJP, aJL=aJL, eb=eb, aw=awgt,
               chi_e=chi_e, chi_e_mass=chi_e_mass)
    npose = np.bincount(ip[pf], minlength=P)[:P]
    nlm = np.bincount(il[lf], minlength=L)[:L]
    out["Hpp_n"], out["bp_n"] = npose[:, None, None], npose[:, None]
    out["Hll_n"], out["bl_n"] = nlm[:, None, None], nlm[:, None]
    return out


def bound_of(ref, key, consts=None):
    return kr.bound(ref[key + "_n"], (consts or BUILD_C)[key], ref[key + "_mass"])


def ratios(got, ref, consts=None):
    """{output: largest error / bound} of a build `got` (a dict with KEYS) against the reference `ref`"""
    return {key: kr.ratio(got[key], ref[key], bound_of(ref, key, consts)) for key in KEYS}


def chi_e_ratio(got, ref, c=C_CHI):
    return kr.ratio(got, ref["chi_e"], kr.bound(1, c, ref["chi_e_mass"]))


def fused_stage_G(got_G, ref, f, got_Linv, f32=False):
    """kernel_ref.fused_stage_G with this reference's C_HPL"""
    _, Li, _ = kr._per_edge_lines(f, got_Linv, np.zeros((max(f["L"], 1), 3)), LD)
    bH = kr.bound(1, C_HPL, ref["Hpl_mass"])
    G, _ = kr.fused_G(ref["Hpl"], Li)
    _, Gm = kr.fused_G(np.abs(ref["Hpl"]) + bH, Li)
    bnd = np.einsum("erm,ecm->erc", bH, np.abs(Li)) + kr.bound(3, kr.C_G, Gm)
    if f32:
        bnd = bnd + LD(2.0 ** -24) * (np.abs(G) + bnd)
    return kr.ratio(got_G, G, bnd)


def fused_stage_pose(got_Hd, got_bp, got_bsc, ps, damp_lam=0.0):
    """kernel_ref.fused_stage_pose with this reference's C_PS_*"""
    I6 = damp_lam * np.eye(6, dtype=LD)
    return dict(diag=kr.ratio(got_Hd, ps["Hd"] + I6, kr.bound(ps["Hd_n"], C_PS_H, ps["Hd_mass"] + I6)),
                bp=kr.ratio(got_bp, ps["bp"], kr.bound(ps["bp_n"], C_PS_BP, ps["bp_mass"])),
                bsc=kr.ratio(got_bsc, ps["bsc"], kr.bound(ps["bsc_n"], C_PS_BSC, ps["bsc_mass"])))
