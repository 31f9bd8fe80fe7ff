"""Extended-precision reference of the build pass WITH a camera-model table (Kannala-Brandt fisheye entries;
cugo_edges.has_rig = 2), numpy, test only.  rig_ref.build restated with a model per camera-table
entry: f["cam_tab"] [n_cams][17] = {M row-major (9), t_s (3), k1, k2, k3, k4, model}, selected by the slot's camera
index; model 0 is the pinhole of rig_ref, model 1 Kannala-Brandt.  It returns the dict rig_ref.build returns ("Xc" is
the BODY-frame point), so kernel_ref's references of the fused iteration take it as `ref`.

The term of a Kannala-Brandt entry at Xs = (x, y, z) = M Xb + t_s, in the kernels' sign convention:
    r2 = x^2 + y^2,  R2 = r2 + z^2,  th = atan2(r, z),  t2 = th^2
    P = 1 + k1 t2 + k2 t2^2 + k3 t2^3 + k4 t2^4  (theta_d = th P),  Q = dP/dt2,  D = d theta_d / d th = P + 2 t2 Q
    g = th / r (1 / z at r = 0),  rho = g P,  e = (fx rho x + cx - mu, fy rho y + cy - mv, 0)
    c = (D z / R2 - rho) / r2                                                            th >= NEAR_AXIS (0.5 rad)
    c = g^2 (4 g P S(4 t2) + 2 Q z / R2),  S(w) = sum_{n=1..9} (-1)^n w^(n-1) / (2n+1)!   th <  NEAR_AXIS
    A = -de/dXs:  A0 = -fx (rho + x^2 c, x y c, -x D / R2),  A1 = -fy (x y c, rho + y^2 c, -y D / R2),  A2 = 0
    B = A M,   JP[:, 3:6] = B,   JP[:, 0:3] = -B [Xb]x,   JL = B R(q)
test_fisheye_ref_host.py checks JP and JL against central differences in longdouble.

Bounds: (n + c) u mass per entry.  c counted as rig_ref's docstring counts (a product: the operands' counts + 1; a sum:
the larger count + 1, the masses added; Xs_i 12 there).  atan2: the documents that come with the ROCm installation
state no accuracy for the device library's double atan2, so the OpenCL bound for double atan2, 6 ulp, is used.
    r2 = x x + y y       12 + 12 + 1, + 1                                                              ->   26
    r = sqrt(r2), R2     26 + 1                                                                        ->   27
    th = atan2(r, z)     27 + 12 + 6 (|d th / d ln r|, |z d th / dz| / th <= 1)                        ->   45
    t2                   45 + 45 + 1                                                                   ->   91
    P                    Horner, four levels of (product with t2: + 92, addition: + 1)                 ->  372
    Q                    the same with a constant factor per coefficient                               ->  375
    D = P + 2 t2 Q       1 + 91 + 375 + 1 = 468, + 1                                                   ->  469
    g = th / r           45 + 27 + 1                                                                   ->   73
    rho = g P            73 + 372 + 1                                                                  ->  446
    D / R2               469 + 27 + 1                                                                  ->  497
    c, general           (D / R2) z: 510; - rho: 511; / r2: 511 + 26 + 1                               ->  538
    c, near axis         S: w 92, eight levels of 94: 752 + 92 = 844; 4 g P S: 73 + 372 + 844 + 4 = 1293;
                         2 Q z / R2: 417; sum 1294; g g: 147; product 1294 + 147 + 1                   -> 1442
    A entries            x c: 12 + 1442 + 1 = 1455; x (x c): 1468; + rho: 1469; fx: + 1, negation 0    -> 1470
    B = A M              1470 + 1 + 2                                                                  -> 1473
    J_P entries          columns 0..2: B 1473 + Xb 8 + product 1 + subtraction 1                       -> 1483
    J_L = B R            1473 + 4 + 1 + 2                                                              -> 1480
    e_i                  fx rho x: 1 + 446 + 1 + 12 = 460; + cx, - m                                   ->  462
    w                    2 x 462 + 5                                                                   ->  929
    Hpp 929 + 2 x 1483 + 4 = 3899;  bp 929 + 1483 + 462 + 4 = 2878;  Hll 929 + 2 x 1480 + 4 = 3893;
    bl 929 + 1480 + 462 + 4 = 2875;  Hpl 929 + 1483 + 1480 + 4 = 3896;  chi 2 x 462 + 1 + 2 + 1 + 6 = 934
Every count exceeds rig_ref's, and a pinhole entry of a model table is held to these too (one constant per output); a
table of pinholes only is compared with rig_ref.build itself (test_fisheye_ref_host.py).  The fused iteration, counted
as rig_ref counts it:
    A = JL L^-T 1483;  A A^T 2969;  N = w I - w^2 A A^T: (2 x 929 + 1) + 2969 + 1 + 1 = 4830
    JP^T N JP  4830 + 1483 + 3 + 1483 + 3 + 1 -> C_PS_H = 7803;  bp -> C_PS_BP = 2878
    u = w (e - A y): (1483 + 3), 929 + 1486 + 1, 1 = 2417;  bsc += JP^T u: 2417 + 1483 + 3 -> C_PS_BSC = 3903
Masses of a Kannala-Brandt entry: aXb, aXs as rig_ref.  A quantity q(Xs) gets  |terms of q| + sum_i |dq/dXs_i| aXs_i:
the first part carries q's own roundings (with |k_j| for k_j and every sign a plus, and on the general branch BOTH
terms of the difference in c, so that its cancellation is inside the bound), the second the 12 u aXs the point arrives
with.  de/dXs = -A is exact; dA/dXs is formed by central differences in longdouble (a mass needs two digits).  From
there on as rig_ref: aB = aA |M|, aJP[:, 0:3] = aB |[aXb]x|, aJL = aB aR.

`mut` names ONE deliberate mistake of an implementation (test_fisheye_ref_host.py shows that each breaks the bounds):
    "k_ignored"        the coefficients not read (the equidistant model on every fisheye entry)
    "pinhole_A"        residual right, A of the pinhole on a fisheye entry
    "D_as_P"           D replaced by theta_d / theta
    "z_sign"           the z column of A with the wrong sign
    "stride12"         entry k read at 12 k of the flat table (RigPar's stride), wrapping at its end
    "neighbour_flag"   the model flag of entry k + 1 (wrapping)
    "pose_pass_rig"    Hpp and bp from the RigPar Jacobian (pinhole A at Xs), everything else right
    "quotient_c"       the quotient form of c below the switch as well (shows in a float64 evaluation only)
"""
import numpy as np

import kernel_ref as kr

LD = kr.LD
STEREO, INACTIVE = 4, 8
MUTATIONS = ("k_ignored", "pinhole_A", "D_as_P", "z_sign", "stride12", "neighbour_flag", "pose_pass_rig", "quotient_c")
NEAR_AXIS = 0.5
STRIDE = 17
C_HPP, C_BP, C_HLL, C_BL, C_HPL, C_CHI = 3899, 2878, 3893, 2875, 3896, 934
C_PS_H, C_PS_BP, C_PS_BSC = 7803, 2878, 3903
BUILD_C = dict(Hpp=C_HPP, bp=C_BP, Hll=C_HLL, bl=C_BL, Hpl=C_HPL, chi=C_CHI)
IDENTITY12 = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)
KEYS = ("Hpp", "bp", "Hll", "bl", "Hpl", "chi")
_FACT = [None] + [float(np.prod(np.arange(1, 2 * n + 2, dtype=np.float64))) for n in range(1, 10)]   # (2n+1)!


def model_table(ext12, model_k5):
    """[n][17] from ext12 [n][12] and model_k5 [n][5] = (k1, k2, k3, k4, model)"""
    return np.ascontiguousarray(np.concatenate([np.asarray(ext12, np.float64), np.asarray(model_k5, np.float64)], 1))


def kb_terms(Xs, k, dt, mut=None):
    """rho, c, D / R2 at Xs [E][3] with coefficients k [E][4], and the sums of the absolute values of their terms"""
    x, y, z = Xs[:, 0], Xs[:, 1], Xs[:, 2]
    one = dt(1)
    r2 = x * x + y * y
    r = np.sqrt(r2)
    R2 = r2 + z * z
    th = np.arctan2(r, z)
    t2 = th * th
    k1, k2, k3, k4 = (k[:, i] for i in range(4))
    a1, a2, a3, a4 = (np.abs(k[:, i]) for i in range(4))
    P = one + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))
    Pa = one + t2 * (a1 + t2 * (a2 + t2 * (a3 + t2 * a4)))
    Q = k1 + t2 * (2 * k2 + t2 * (3 * k3 + t2 * (4 * k4)))
    Qa = a1 + t2 * (2 * a2 + t2 * (3 * a3 + t2 * (4 * a4)))
    D = P + 2 * t2 * Q
    Da = Pa + 2 * t2 * Qa
    if mut == "D_as_P":
        D = P
    with np.errstate(all="ignore"):
        g = np.where(r > 0, th / np.where(r > 0, r, one), one / z)
        rho, rho_a = g * P, np.abs(g) * Pa
        dR, dR_a = D / R2, Da / R2
        w = 4 * t2
        S = dt(0) * w
        for n in range(9, 0, -1):
            S = S * w + dt((-1) ** n) / dt(_FACT[n])
        c_near = (g * g) * (4 * g * P * S + 2 * Q * (z / R2))
        c_near_a = (g * g) * (4 * np.abs(g) * Pa * np.abs(S) + 2 * Qa * (np.abs(z) / R2))
        c_gen = (dR * z - rho) / r2
        c_gen_a = (dR_a * np.abs(z) + rho_a) / r2
    near = th < NEAR_AXIS
    if mut == "quotient_c":
        near = near & (r2 == 0)             # (0 / 0 at r = 0 itself is not what this mistake is about)
    return rho, np.where(near, c_near, c_gen), dR, rho_a, np.where(near, c_near_a, c_gen_a), dR_a


def kb_A(Xs, fx, fy, k, dt, mut=None):
    """A = -d(pu, pv)/dXs [E][3][3] (third row zero), the sums of the absolute values of its terms, rho and |rho| terms"""
    x, y = Xs[:, 0], Xs[:, 1]
    rho, c, dR, rho_a, c_a, dR_a = kb_terms(Xs, k, dt, mut)
    zero = np.zeros(len(x), dt)
    sz = -1 if mut == "z_sign" else 1
    A = np.zeros((len(x), 3, 3), dt)
    T = np.zeros((len(x), 3, 3), dt)
    A[:, 0] = np.stack([-(fx * (rho + x * (x * c))), -(fx * (y * (x * c))), sz * fx * (x * dR)], 1)
    A[:, 1] = np.stack([-(fy * (x * (y * c))), -(fy * (rho + y * (y * c))), sz * fy * (y * dR)], 1)
    ax, ay = np.abs(x), np.abs(y)
    T[:, 0] = np.stack([fx * (rho_a + ax * ax * c_a), fx * (ay * ax * c_a), fx * (ax * dR_a)], 1)
    T[:, 1] = np.stack([fy * (ax * ay * c_a), fy * (rho_a + ay * ay * c_a), fy * (ay * dR_a)], 1)
    del zero
    return A, T, rho, rho_a


def kb_A_mass(Xs, aXs, fx, fy, k):
    """|terms of A| + sum_i |dA/dXs_i| aXs_i, longdouble, the derivative by central differences (step 2^-26 of |Xs|)"""
    Xs, aXs, fx, fy, k = (np.asarray(a, LD) for a in (Xs, aXs, fx, fy, k))
    _, T, _, _ = kb_A(Xs, fx, fy, k, LD)
    h = LD(2.0 ** -26) * np.sqrt((Xs * Xs).sum(1))
    mass = T
    for i in range(3):
        d = np.zeros_like(Xs); d[:, i] = h
        plus, minus = kb_A(Xs + d, fx, fy, k, LD)[0], kb_A(Xs - d, fx, fy, k, LD)[0]
        mass = mass + np.abs(plus - minus) / (2 * h)[:, None, None] * aXs[:, i][:, None, None]
    return mass


def _cross_cols(B, X, sign):
    """columns 0..2 of -B [X]x (sign = -1: the values; +1: the masses, every sign a plus)"""
    return np.stack([B[:, :, 2] * X[:, None, 1] + sign * B[:, :, 1] * X[:, None, 2],
                     B[:, :, 0] * X[:, None, 2] + sign * B[:, :, 2] * X[:, None, 0],
                     B[:, :, 1] * X[:, None, 0] + sign * B[:, :, 0] * X[:, None, 1]], 2)


def build(f, rk2, mut=None, dtype=LD):
    """rk2 = {"mono": (type, delta), "stereo": ...}; f["cam_tab"] [n_cams][17]"""
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
    if mut == "stride12":
        flat = table.ravel()
        ent = flat[(12 * cid[:, None] + np.arange(STRIDE)[None, :]) % len(flat)]
    else:
        ent = table[cid]
    M, ts, kk = ent[:, :9].reshape(E, 3, 3), ent[:, 9:12], ent[:, 12:16]
    fish = ent[:, 16] != 0
    if mut == "neighbour_flag":
        fish = table[(cid + 1) % n_cams, 16] != 0
    if mut == "k_ignored":
        kk = np.zeros_like(kk)
    aM = np.abs(M)
    meas = np.asarray(f["meas"], dt).T
    omega = np.asarray(f["omega"], dt)
    st = ((fl & STEREO) != 0) & ~fish
    assert not np.any(real & ((fl & STEREO) != 0) & (table[cid, 16] != 0)), "a stereo slot on a Kannala-Brandt entry is not defined"
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
    # ---- the pinhole, as rig_ref (evaluated on every slot and selected: a fisheye slot may have Z_s <= 0) ----
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
    A_pin, aA_pin = A, aA
    # ---- Kannala-Brandt entries ----
    if np.any(fish):
        kmut = mut if mut in ("D_as_P", "z_sign", "quotient_c") else None
        Ak, _, rho, rho_a = kb_A(Xs[fish], fx[fish], fy[fish], kk[fish], dt, kmut)
        aAk = kb_A_mass(Xs[fish], aXs[fish], fx[fish], fy[fish], kk[fish]).astype(dt)
        Ak0 = kb_A(np.asarray(Xs[fish], LD), np.asarray(fx[fish], LD), np.asarray(fy[fish], LD), np.asarray(kk[fish], LD), LD)[0]
        xs, ys = Xs[fish, 0], Xs[fish, 1]
        ek = np.stack([(fx[fish] * rho * xs + cx[fish]) - meas[fish, 0], (fy[fish] * rho * ys + cy[fish]) - meas[fish, 1],
                       zero[fish]], 1)
        lever = (np.abs(Ak0) * np.asarray(aXs[fish], LD)[:, None, :]).sum(2).astype(dt)      # sum_i |de_m/dXs_i| aXs_i
        aek = np.stack([fx[fish] * rho_a * np.abs(xs) + np.abs(cx[fish]) + np.abs(meas[fish, 0]) + lever[:, 0],
                        fy[fish] * rho_a * np.abs(ys) + np.abs(cy[fish]) + np.abs(meas[fish, 1]) + lever[:, 1], zero[fish]], 1)
        A, aA, e, ae = A.copy(), aA.copy(), e.copy(), ae.copy()
        e[fish], ae[fish] = ek, aek
        if mut != "pinhole_A":
            A[fish], aA[fish] = Ak, aAk
        else:
            aA[fish] = aAk
    B = np.einsum("emk,ekj->emj", A, M)
    aB = np.einsum("emk,ekj->emj", aA, aM)
    JP = np.concatenate([_cross_cols(B, Xb, -1), B], 2)
    aJP = np.concatenate([_cross_cols(aB, aXb, 1), aB], 2)
    JL = np.einsum("emk,ekj->emj", B, R)
    aJL = np.einsum("emk,ekj->emj", aB, aR)
    xr = omega * (e * e).sum(1)
    xmass = omega * (np.abs(e) * (np.abs(e) + 2 * ae)).sum(1)
    rho_, drho, d2rho = (np.zeros(E, dt) for _ in range(3))
    for sel, key in ((~st, "mono"), (st, "stereo")):
        r0, r1, r2 = kr._rho(int(rk2[key][0]), rk2[key][1], xr, dt)
        rho_, drho, d2rho = np.where(sel, r0, rho_), np.where(sel, r1, drho), np.where(sel, r2, d2rho)
    live = real.astype(dt)
    # (selected, not multiplied: an inactive slot of the layouts may sit anywhere behind a sensor pose)
    wgt = np.where(real, omega * drho, 0)
    awgt = np.where(real, omega * drho + omega * d2rho * xmass, 0)
    eb = np.abs(e) + ae
    JPp, aJPp = JP, aJP                          # the rows the pose pass (Hpp, bp) is built from
    if mut == "pose_pass_rig":
        Bp = np.einsum("emk,ekj->emj", A_pin, M)
        JPp = np.concatenate([_cross_cols(Bp, Xb, -1), Bp], 2)
    dead = ~real
    if np.any(dead):                             # 0 x (inf or nan) of a slot that does not count
        JP, JL, JPp, aJP, aJL, aJPp, e, eb = (np.where(dead.reshape((E,) + (1,) * (a.ndim - 1)), 0, a)
                                              for a in (JP, JL, JPp, aJP, aJL, aJPp, e, eb))
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
    chi_e = np.where(real, rho_, 0)
    chi_e_mass = np.where(real, np.abs(rho_) + xmass, 0)
    out = dict(Hpp=kr._scatter(ip[pf], tHpp[pf], P), Hpp_mass=kr._scatter(ip[pf], mHpp[pf], P),
               bp=kr._scatter(ip[pf], tbp[pf], P), bp_mass=kr._scatter(ip[pf], mbp[pf], P),
               Hll=kr._scatter(il[lf], tHll[lf], L), Hll_mass=kr._scatter(il[lf], mHll[lf], L),
               bl=kr._scatter(il[lf], tbl[lf], L), bl_mass=kr._scatter(il[lf], mbl[lf], L),
               Hpl=Hpl, Hpl_mass=mHpl, Hpl_n=np.ones((E, 1, 1)),
               chi=chi_e.sum(), chi_mass=chi_e_mass.sum(), chi_n=int(real.sum()),
               w=wgt, x=xr, f=f, fish=fish,
               Xc=Xb, Xs=Xs, R=R, e=e, JP=JPp, JL=JL, aJP=aJPp, aJL=aJL, eb=eb, aw=awgt,
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
