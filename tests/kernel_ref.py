"""Extended-precision reference of the bundle-adjustment kernels with PER-ENTRY error bounds (numpy, test only).

A restatement of SURVEY.md Appendix A in np.longdouble (64-bit mantissa here), written from the formulas: rotation by
an explicit 3 x 3 matrix, the Jacobians in the x = X/Z, y = Y/Z form of A.3 for mono and stereo alike, the 3 x 3
inverse by cross products, the pose update by the half-angle quaternion.  Every array is in the FLATTENED order of
devmem.flatten (free-first vertex indices, landmark-major edge slots); blocks are matrices ([n, rows, cols]),
colmajor() gives the device layout.

Bounds.  Every summed output comes with
    mass[entry] = sum over the contributing scalar products of the product of the ABSOLUTE values, evaluated without
                  cancellation (a difference a - b counts |a| + |b|), and
    n[entry]    = the number of summed terms (edges, products).
A double evaluation of the same formula, in any summation order, with or without FMA, differs from the exact value by
at most (n + c) u mass (1 + O(u)), u = 2^-53: a scalar product that passes through k roundings carries a factor
(1 + d)^k, |d| <= u; n of the k are the additions of the sum, c the roundings inside one term and behind the sum.
c per output, counted on the longest path of the formulas below (and of the kernels: the count is per formula, not
per implementation):
    Xc_i = sum_j R_ij Xw_j + t_i      R_ij 4, product 1, 3 additions                              ->  8
    1/Z  9;  x = X/Z, y = Y/Z        8 + 9 + 1                                                   -> 18
    J_P entries                       fx(1 + x^2): 2 x 18 + 3; stereo row 2 one more              -> 40
    J_L entries                       (fx/Z)(R_0j - x R_2j): 10 + (18 + 4 + 2) + 1; stereo + 1    -> 36
    e_i = proj_i - meas_i             18 + 3, relative to the residual's mass |proj| + |meas|     -> 21
    w = omega rho'(omega |e|^2)       squares, sum, omega, rho', omega: 10 relative to w; the error of e enters
                                      through rho'' and is carried by the mass (below), factor 2 x 21 + 5 -> 47
    Hpp += w J_P^T J_P                47 + 40 + 40 + product 1 + 2 additions over the rows + w 1 -> C_HPP = 131
    bp  += w J_P^T e                  47 + 40 + 21 + 4                                            -> C_BP  = 112
    Hll += w J_L^T J_L                47 + 36 + 36 + 4                                            -> C_HLL = 123
    bl  += w J_L^T e                  47 + 36 + 21 + 4                                            -> C_BL  = 108
    Hpl  = w J_P^T J_L   (n = 1)      47 + 40 + 36 + 4                                            -> C_HPL = 127
    chi += rho(omega |e|^2)           2 x 21 + 1 per square, 2 additions, omega 1, rho 6           -> C_CHI = 52
    T = Hpl inv          (n = 3)      product 1                                                   -> C_T   = 1
    Hsc = Hpp (+ lambda) - sum T Hpl^T   product 1, 2 additions, the subtraction, lambda           -> C_HSC = 5
    bsc = bp - sum T bl               product 1, 2 additions, the subtraction                     -> C_BSC = 4
    xl = inv (bl - sum Hpl^T xp)      product 1, 5 additions, subtraction, product 1, 2 additions -> C_XL  = 10
    scale = sum x (lambda x + b)      3                                                           -> C_SCALE = 3
(these are worst-case path counts; measured errors are far smaller: test_kernel_ref_host records the oracle's).
The fused iteration (lines, G, k_pose_schur, its back-substitution) has its own list of c and the measured K_CHOL
further down, above C_LINE_Y.
Masses of the geometric build: aXc_i = sum_j |R|_ij |Xw_j| + |t_i| with |R| the quaternion formula with every sign a
plus; ax = aX aZ / Z^2 (mass of X/Z), aiz = aZ / Z^2 (mass of 1/Z); the Jacobian masses are A.3 with these and plus
signs; the residual's mass is |proj| + |meas| and is ADDED to |e| wherever e enters a product; the weight's mass is
aw = w + omega |rho''| omega sum_i |e_i| (|e_i| + 2 ae_i) (first order in the error of e; rho' is continuous for every
kernel here, |rho''| is taken as the larger one-sided value at Huber's kink).
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, ("kernel_ref needs an extended-precision np.longdouble (x87 80-bit or better): eps = %g "
                                  "here, the reference would be no more precise than the code under test" % np.finfo(LD).eps)
U = 2.0 ** -53
C_HPP, C_BP, C_HLL, C_BL, C_HPL, C_CHI = 131, 112, 123, 108, 127, 52
C_T, C_HSC, C_BSC, C_XL, C_SCALE = 1, 5, 4, 10, 3
# measured, not derived (test_kernel_ref_host.py: 4 x what the C oracle reaches against this reference, rounded up):
# entrywise error of the 3 x 3 adjugate inverse in u kappa max|inv|; quaternion of the pose update in u; its translation
# in u (|t| + |v| (1 + 1 / max(theta, 1e-5)))
K_INV, KQ, KT = 20.0, 10.0, 21.0


def colmajor(M):
    """[n, r, c] matrices -> [n, r * c] column-major blocks (the device layout)"""
    M = np.asarray(M)
    return np.ascontiguousarray(M.transpose(0, 2, 1).reshape(len(M), -1))


def from_colmajor(a, r, c):
    return np.asarray(a).reshape(-1, c, r).transpose(0, 2, 1)


def bound(n, c, mass):
    return (np.asarray(n, LD) + c) * LD(U) * np.asarray(mass, LD)


def ratio(got, ref, bnd):
    """largest |got - ref| / bound over the entries with a positive bound; entries whose bound is exactly zero (mass
    zero: nothing contributes) must be exactly zero in `got`, else inf"""
    got, ref, bnd = np.asarray(got, LD), np.asarray(ref, LD), np.asarray(bnd, LD)
    if got.size == 0:
        return 0.0
    if not np.all(np.isfinite(got)):
        return float("inf")
    err = np.abs(got - ref)
    pos = bnd > 0
    if np.any(got[~pos] != 0):
        return float("inf")
    return float((err[pos] / bnd[pos]).max()) if pos.any() else 0.0


def _rho(kind, delta, x, dt):
    d2 = dt(delta) * dt(delta)
    one = dt(1)
    if kind == 2:    # Tukey
        inside = x <= d2
        u = one - x / d2
        return (np.where(inside, d2 / 3 * (one - u ** 3), d2 / 3), np.where(inside, u * u, 0 * x),
                np.where(inside, 2 * np.abs(u) / d2, 0 * x))
    if kind == 1:    # Cauchy
        v = one + x / d2
        return d2 * np.log(v), one / v, one / (d2 * v * v)
    if kind == 3:    # Huber
        inside = x <= d2
        xs = np.maximum(x, d2)
        return (np.where(inside, x, 2 * dt(delta) * np.sqrt(xs) - d2), np.where(inside, one + 0 * x, dt(delta) / np.sqrt(xs)),
                dt(delta) / (2 * xs * np.sqrt(xs)))
    return x, one + 0 * x, 0 * x


def _scatter(idx, vals, n):
    """out[i] = sum of vals[k] over idx[k] == i, each sum in the order of k (segment sums of the stably sorted terms:
    np.add.at is an order of magnitude slower on longdouble)"""
    out = np.zeros((n,) + vals.shape[1:], vals.dtype)
    idx = np.asarray(idx)
    if len(idx) == 0:
        return out
    if np.any(np.diff(idx) < 0):
        order = np.argsort(idx, kind="stable")
        idx, vals = idx[order], vals[order]
    starts = np.concatenate([[0], np.flatnonzero(np.diff(idx)) + 1])
    out[idx[starts]] = np.add.reduceat(vals, starts, axis=0)
    return out


def build(prob, rk=(0, 1.0), f=None, dtype=LD):
    """Hpp [P,6,6], bp [P,6], Hll [L,3,3], bl [L,3], Hpl [E,6,3], chi of the problem in the flattened order, with
    X_mass and X_n for each.  rk = (type, delta) for both edge sets."""
    import devmem
    f = devmem.flatten(prob) if f is None else f
    dt = dtype
    E, P, L = f["E"], f["P"], f["L"]
    fl = f["flags"]
    real = (fl & 8) == 0
    ip, il = f["pose"], f["lm"]
    pose = np.asarray(f["poses"], dt)[ip]
    Xw = np.asarray(f["lms"], dt)[il]
    cam = np.asarray(f["cams"], dt)[f["cam_id"]]
    fx, fy, cx, cy, bf = (cam[:, k] for k in range(5))
    meas = np.asarray(f["meas"], dt).T
    omega = np.asarray(f["omega"], dt)
    st = (fl & 4) != 0
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
    aJP[:, 0] = np.stack([fx * axn * ayn, fx * (1 + axn * axn), fx * ayn, fx * aiz, zero, fx * axn * aiz], 1)
    aJP[:, 1] = np.stack([fy * (1 + ayn * ayn), fy * axn * ayn, fy * axn, zero, fy * aiz, fy * ayn * aiz], 1)
    s = st.astype(dt)
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
    pu, pv = fx * xn + cx, fy * yn + cy
    e = np.stack([pu - meas[:, 0], pv - meas[:, 1], s * ((pu - bf * iz) - meas[:, 2])], 1)
    ae = np.stack([fx * axn + np.abs(cx) + np.abs(meas[:, 0]), fy * ayn + np.abs(cy) + np.abs(meas[:, 1]),
                   s * (fx * axn + np.abs(cx) + bf * aiz + np.abs(meas[:, 2]))], 1)
    xr = omega * (e * e).sum(1)
    xmass = omega * (np.abs(e) * (np.abs(e) + 2 * ae)).sum(1)
    rho, drho, d2rho = _rho(int(rk[0]), rk[1], xr, dt)
    live = real.astype(dt)
    wgt = live * omega * drho
    awgt = live * (omega * drho + omega * d2rho * xmass)
    eb = np.abs(e) + ae
    # per-edge terms
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
    out = dict(Hpp=_scatter(ip[pf], tHpp[pf], P), Hpp_mass=_scatter(ip[pf], mHpp[pf], P),
               bp=_scatter(ip[pf], tbp[pf], P), bp_mass=_scatter(ip[pf], mbp[pf], P),
               Hll=_scatter(il[lf], tHll[lf], L), Hll_mass=_scatter(il[lf], mHll[lf], L),
               bl=_scatter(il[lf], tbl[lf], L), bl_mass=_scatter(il[lf], mbl[lf], L),
               Hpl=Hpl, Hpl_mass=mHpl, Hpl_n=np.ones((E, 1, 1)),
               chi=(live * rho).sum(), chi_mass=(live * (np.abs(rho) + xmass)).sum(), chi_n=int(real.sum()),
               w=wgt, x=xr, f=f,
               # per-edge parts, for the references of the fused iteration (pose_schur)
               Xc=Xc, R=R, e=e, JP=JP, JL=JL, aJP=aJP, aJL=aJL, eb=eb, aw=awgt)
    npose = np.bincount(ip[pf], minlength=P)[:P]
    nlm = np.bincount(il[lf], minlength=L)[:L]
    out["Hpp_n"], out["bp_n"] = npose[:, None, None], npose[:, None]
    out["Hll_n"], out["bl_n"] = nlm[:, None, None], nlm[:, None]
    return out


BUILD_C = dict(Hpp=C_HPP, bp=C_BP, Hll=C_HLL, bl=C_BL, Hpl=C_HPL, chi=C_CHI)


def inv3(A):
    """inverse of [n,3,3] symmetric matrices by cross products of the columns: A^-1 = [b x c, c x a, a x b]^T / det"""
    a, b, c = A[:, :, 0], A[:, :, 1], A[:, :, 2]
    bc, ca, ab = np.cross(b, c), np.cross(c, a), np.cross(a, b)
    det = (a * bc).sum(1)
    return np.stack([bc, ca, ab], 1) / det[:, None, None]


def schur(f, hs, lam, damp, Hpp, bp, Hll, bl, Hpl, T=None, inv=None, dtype=LD, want=("mass", "Tmass", "imass")):
    """inv [L,3,3] = (Hll + lam I)^-1, T [E,6,3] = Hpl inv, Hsc [B,6,6], bsc [P,6] from the arrays it is given
    (matrices, see from_colmajor).  With `inv` given T is formed from it; with `T` given Hsc and bsc are formed from it.
    Returns masses and term counts of T, Hsc, bsc; Hsc_Tmass / bsc_Tmass: the product sums with |Hpl| |inv| in place
    of |T| (what bounds an implementation whose T differs from Hpl inv by its own rounding: each unit of relative T
    error adds u x this); kappa [L] = cond(Hll + lam I); and Hsc_imass / bsc_imass: the
    sensitivity of Hsc / bsc to an error of inv, sum |Hpl| 11^T |Hpl|^T kappa max|inv| (an implementation that forms its
    own inverse with entrywise error <= K u kappa max|inv| is inside (n + c) u mass + K u imass).  `want`: which of
    the three product-list sums of the off-diagonal blocks are formed (each costs as much as Hsc itself); the others
    are then valid on the diagonal blocks only."""
    dt = dtype
    rowptr, colind, off_ptr, ei, ej = hs
    P, L, E = f["P"], f["L"], f["E"]
    B = len(colind)
    Hpp, bp, Hll, bl, Hpl = (np.asarray(a, dt) for a in (Hpp, bp, Hll, bl, Hpl))
    lam = dt(lam)
    A = Hll + lam * np.eye(3, dtype=dt)
    inv_ref = inv3(A) if L else np.zeros((0, 3, 3), dt)
    kappa = np.linalg.cond(np.asarray(A, np.float64)) if L else np.zeros(0)
    inv_use = inv_ref if inv is None else np.asarray(inv, dt)
    ff = (f["flags"] & 11) == 0
    il = np.where(ff, f["lm"], 0)
    iv_e = inv_use[il] if L else np.zeros((E, 3, 3), dt)
    T_ref = ff[:, None, None] * np.einsum("erm,emc->erc", Hpl, iv_e)
    T_mass = ff[:, None, None] * np.einsum("erm,emc->erc", np.abs(Hpl), np.abs(iv_e))
    T_use = T_ref if T is None else np.asarray(T, dt)
    aT, aH = np.abs(T_use), np.abs(Hpl)
    es = np.flatnonzero(ff)
    ps = f["pose"][es]
    ble = bl[f["lm"][es]]
    bsc = bp - _scatter(ps, np.einsum("erm,em->er", T_use[es], ble), P)
    bsc_mass = np.abs(bp) + _scatter(ps, np.einsum("erm,em->er", aT[es], np.abs(ble)), P)
    npose = np.bincount(ps, minlength=P)[:P]
    Hsc = np.zeros((B, 6, 6), dt); Hsc_mass = np.zeros((B, 6, 6), dt); Hsc_n = np.zeros(B, np.int64)
    dk = np.asarray(rowptr[:P])
    Hsc[dk] = Hpp - _scatter(ps, np.einsum("erm,ecm->erc", T_use[es], Hpl[es]), P)
    Hsc_mass[dk] = np.abs(Hpp) + _scatter(ps, np.einsum("erm,ecm->erc", aT[es], aH[es]), P)
    if damp:
        Hsc[dk] += lam * np.eye(6, dtype=dt)
        Hsc_mass[dk] += np.abs(lam) * np.eye(6, dtype=dt)
    Hsc_n[dk] = npose
    blk = np.repeat(np.arange(B), np.diff(off_ptr))
    Hsc -= _scatter(blk, np.einsum("erm,ecm->erc", T_use[ei], Hpl[ej]), B)
    if "mass" in want:
        Hsc_mass += _scatter(blk, np.einsum("erm,ecm->erc", aT[ei], aH[ej]), B)
    Hsc_n += np.diff(off_ptr)
    # sensitivity to the inverse
    sc = (dt(1) * kappa * np.abs(inv_ref).reshape(L, -1).max(1))[il] * ff if L else np.zeros(E, dt)
    rs = aH.sum(2)                                              # [E,6]: |Hpl| 1
    Hsc_imass = np.zeros((B, 6, 6), dt)
    if "imass" in want:
        Hsc_imass[dk] = _scatter(ps, (sc[es, None, None] * rs[es, :, None] * rs[es, None, :]), P)
        Hsc_imass += _scatter(blk, sc[ei, None, None] * rs[ei, :, None] * rs[ej, None, :], B)
    bsc_imass = _scatter(ps, sc[es, None] * rs[es] * np.abs(ble).sum(1)[:, None], P)
    # the same masses with |Hpl| |inv| in place of |T|: what bounds an implementation that forms its own T
    Hsc_own = np.zeros((B, 6, 6), dt)
    Hsc_own[dk] = _scatter(ps, np.einsum("erm,ecm->erc", T_mass[es], aH[es]), P)
    if "Tmass" in want:
        Hsc_own += _scatter(blk, np.einsum("erm,ecm->erc", T_mass[ei], aH[ej]), B)
    bsc_own = _scatter(ps, np.einsum("erm,em->er", T_mass[es], np.abs(ble)), P)
    return dict(inv=inv_ref, kappa=kappa, T=T_ref, T_mass=T_mass, T_n=3, Hsc=Hsc, Hsc_mass=Hsc_mass,
                Hsc_Tmass=Hsc_own, bsc_Tmass=bsc_own,
                Hsc_n=Hsc_n[:, None, None], bsc=bsc, bsc_mass=bsc_mass, bsc_n=npose[:, None],
                Hsc_imass=Hsc_imass, bsc_imass=bsc_imass)


def backsubst(f, lam, inv, bl, bp, Hpl, xp, xl=None, kappa=None, dtype=LD):
    """xl [L,3] = inv (bl - sum_e Hpl_e^T xp[pose(e)]) over the free-free edges of each landmark, and scale = sum x (lam
    x + b) over [xp; xl] (with `xl` given: over that xl), split into its pose and landmark parts; masses and counts."""
    dt = dtype
    P, L = f["P"], f["L"]
    inv, bl, bp, Hpl, xp = (np.asarray(a, dt) for a in (inv, bl, bp, Hpl, xp))
    lam = dt(lam)
    ff = (f["flags"] & 11) == 0
    es = np.flatnonzero(ff)
    ls, ps = f["lm"][es], f["pose"][es]
    cl = bl - _scatter(ls, np.einsum("erc,er->ec", Hpl[es], xp[ps]), L)
    cl_mass = np.abs(bl) + _scatter(ls, np.einsum("erc,er->ec", np.abs(Hpl[es]), np.abs(xp[ps])), L)
    x = np.einsum("lrc,lc->lr", inv, cl)
    x_mass = np.einsum("lrc,lc->lr", np.abs(inv), cl_mass)
    nl = np.bincount(ls, minlength=L)[:L]
    xu = x if xl is None else np.asarray(xl, dt)
    sp, sl = (xp * (lam * xp + bp)).sum(), (xu * (lam * xu + bl)).sum()
    mp = (np.abs(xp) * (np.abs(lam) * np.abs(xp) + np.abs(bp))).sum()
    ml = (np.abs(xu) * (np.abs(lam) * np.abs(xu) + np.abs(bl))).sum()
    # sensitivity of xl to an error of inv (entrywise <= K u kappa max|inv|): kappa max|inv| sum_c |cl|-mass
    imass = None if kappa is None else (np.asarray(kappa, dt) * np.abs(inv).reshape(L, -1).max(1) * cl_mass.sum(1))[:, None]
    return dict(xl=x, xl_mass=x_mass, xl_n=nl[:, None], xl_imass=imass, scale=sp + sl, scale_mass=mp + ml, scale_n=6 * P + 3 * L,
                scale_pose=sp, scale_pose_mass=mp, scale_pose_n=6 * P)


def _quat_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def pose_update(pose, dx, dtype=LD):
    """T <- exp([w, v]) T for one pose (7) and one step (6): half-angle quaternion of the rotation, closed-form V with
    (1 - cos t) / t^2 written 2 sin^2(t/2) / t^2, series below t = 1e-7; q <- normalize(dq q) with w >= 0."""
    dt = dtype
    pose, dx = np.asarray(pose, dt), np.asarray(dx, dt)
    om, v = dx[:3], dx[3:]
    th = np.sqrt((om * om).sum())
    O = np.array([[0 * th, -om[2], om[1]], [om[2], 0 * th, -om[0]], [-om[1], om[0], 0 * th]])
    O2 = O @ O
    I = np.eye(3, dtype=dt)
    if th < 1e-7:
        t2 = th * th
        dq = np.concatenate([om * (dt(1) / 2 - t2 / 48), [1 - t2 / 8]])
        V = I + O / 2 + O2 / 6
    else:
        sh = np.sin(th / 2)
        dq = np.concatenate([om * (sh / th), [np.cos(th / 2)]])
        V = I + (2 * sh * sh / (th * th)) * O + ((th - np.sin(th)) / (th * th * th)) * O2
    t = V @ v + _quat_R(dq) @ pose[4:]
    ax, ay, az, aw = dq
    bx, by, bz, bw = pose[:4]
    q = np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                  aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])
    q = q / np.sqrt((q * q).sum())
    if q[3] < 0:
        q = -q
    return np.concatenate([q, t])


def pose_update_error(got, ref, pose, dx):
    """(quaternion error in u, translation error over its base u (|t| + |v| (1 + 1 / max(theta, 1e-5)))) of one updated
    pose; the quaternion is compared up to the sign ambiguity at w ~ 0 (both candidates have w >= 0 to rounding)"""
    got, ref = np.asarray(got, LD), np.asarray(ref, LD)
    assert got[3] >= 0
    eq = np.abs(got[:4] - ref[:4]).max()
    if abs(ref[3]) < 1e-9:
        eq = min(eq, np.abs(got[:4] + ref[:4]).max())
    th = float(np.linalg.norm(np.asarray(dx[:3], np.float64)))
    base = np.linalg.norm(np.asarray(pose[4:], np.float64)) + np.linalg.norm(np.asarray(dx[3:], np.float64)) * (1 + 1 / max(th, 1e-5))
    et = np.abs(got[4:] - ref[4:]).max()
    return float(eq / U), float(et / (U * base))


# ------------------------------------------------------------------ the fused iteration (DESIGN.md sections 4c / 4d)
"""References of the one-stream form: per free landmark Hll + lam I = L L^T, the line {L^-1, y = L^-1 bl},
G_e = Hpl_e L^-T; per pose sum JP^T N JP, sum JP^T (w e), sum JP^T u with A = JL L^-T, N = w I - w^2 A A^T,
u = w (e - A y); dx_l = L^-T (y - sum G_e^T dx_p).  Each in longdouble with n and mass as above, and a float64 REPLAY
in the order of the device's operations (k_build_edges' gform branch, k_pose_schur) on which the bounds are sized on
the CPU (test_fused_ref_host.py) — nothing here was tuned on a GPU.

c, counted on the longest path of the kernels' formulas (the entries of the list above carry over):
    y = L^-1 bl            (n = 3)  product 1, against the DEVICE's L^-1                           -> C_LINE_Y = 1
    G = Hpl L^-T           (n = 3)  product 1, against reference Hpl x the DEVICE's L^-1; Hpl's own bound
                                    (1 + C_HPL) u mass is carried through |L^-1|                   -> C_G = 1
    A = JL L^-T                     J_L 36, product 1, 2 additions                                 -> 39
    A A^T                           2 x 39, product 1, 2 additions                                 -> 81
    N = w I - w^2 A A^T             w^2: 2 x 47 + 1; times A A^T: 95 + 81 + 1; the subtraction 1   -> 178
    JP^T N JP                       N JP: 178 + 40 + 1 + 2; JP^T (.): + 40 + 1 + 2; lambda 1       -> C_PS_H = 265
    bp  += JP^T (w e)               w e: 47 + 21 + 1; JP: 40 + 1 + 2  (= C_BP)                     -> C_PS_BP = 112
    u = w (e - A y)                 A y: 39 + 1 + 2; times w: 47 + 42 + 1; the subtraction 1       -> 91
    bsc += JP^T u                   91 + 40 + 1 + 2                                                -> C_PS_BSC = 134
    dx_l = L^-T (y - sum G^T dx_p)  product 1, 5 additions, subtraction, product 1, 2 additions    -> C_XL_LINES = 10
The cancellation inside N and u is inside the mass: |JP|^T (w I + w^2 |A| |A|^T) |JP| and w |JP|^T (|e| + |A| |y|),
with the build reference's masses for |JP|, |JL|, |e| and w.

K_CHOL: entrywise error of L^-1 in u kappa(Hll + lam I) max|L^-1| per landmark.  Measured, not derived
(test_fused_ref_host.py prints it): the float64 replay of the device's factorisation against longdouble over the
designed layouts (designed.fused_layout: A, B_plan, C, U, F-dead, F-cond at lambda 1e-6, 1e-3, 0.5; kappa up to 1e10)
reaches 1.48; the C oracle has no 3 x 3 Cholesky (it inverts by the adjugate) and sets no second figure.
K_CHOL = 4 x that, rounded up: the margin of K_INV, KQ, KT.
"""
C_LINE_Y, C_G, C_PS_H, C_PS_BP, C_PS_BSC, C_XL_LINES = 1, 1, 265, 112, 134, 10
K_CHOL = 6.0


def _lines(Hll, bl, lam, dt, mut=None):
    """the 3 x 3 factorisation of k_build_edges' gform branch, operation by operation, in dtype dt"""
    Hll, bl = np.asarray(Hll, dt), np.asarray(bl, dt)
    n = len(Hll)
    lam, one = dt(lam), dt(1)
    a0, a1, a2, a3, a4, a5 = Hll[:, 0, 0], Hll[:, 0, 1], Hll[:, 0, 2], Hll[:, 1, 1], Hll[:, 1, 2], Hll[:, 2, 2]
    b0, b1, b2 = bl[:, 0], bl[:, 1], bl[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        p0 = a0 + lam
        l00 = np.sqrt(p0)
        i00 = one / l00
        l10, l20 = a1 * i00, a2 * i00
        p1 = a3 + lam - l10 * l10
        l11 = np.sqrt(p1)
        i11 = one / l11
        l21 = (a4 - l20 * l10) * i11
        p2 = a5 + lam - l20 * l20 - l21 * l21
        l22 = np.sqrt(p2)
        i22 = one / l22
        i10 = -(l10 * i00) * i11
        i21 = -(l21 * i11) * i22
        i20 = -(l20 * i00 + l21 * i10) * i22
        if mut == "i20_without_l21_i10":
            i20 = -(l20 * i00) * i22
        if mut == "swap_20_21":
            i20, i21 = i21, i20
        y0 = i00 * b0
        y1 = i10 * b0 + i11 * b1
        y2 = i20 * b0 + i21 * b1 + i22 * b2
        if mut == "y_is_bl":
            y0, y1, y2 = b0, b1, b2
    z = np.zeros(n, dt)
    L = np.stack([np.stack([l00, z, z], 1), np.stack([l10, l11, z], 1), np.stack([l20, l21, l22], 1)], 1)
    Linv = np.stack([np.stack([i00, z, z], 1), np.stack([i10, i11, z], 1), np.stack([i20, i21, i22], 1)], 1)
    return dict(L=L, Linv=Linv, y=np.stack([y0, y1, y2], 1), piv=np.stack([p0, p1, p2], 1))


def fused_lines(Hll, bl, lam):
    """L, Linv = L^-1 (lower triangular [n,3,3]), y = L^-1 bl and the pivots piv [n,3] (the squares under the three
    roots) of Hll + lam I = L L^T in longdouble; kappa [n] = cond(Hll + lam I)"""
    out = _lines(Hll, bl, lam, LD)
    A = np.asarray(Hll, np.float64) + lam * np.eye(3)
    out["kappa"] = np.linalg.cond(A) if len(A) else np.zeros(0)
    return out


def replay_lines(Hll, bl, lam, mut=None):
    """the float64 replay of the device's factorisation; mut: one of the mutations of test_fused_ref_host.py"""
    return _lines(Hll, bl, lam, np.float64, mut)


def lines_bound(kappa, Linv):
    """[n,1,1]: K_CHOL u kappa max|L^-1| per landmark"""
    Linv = np.asarray(Linv, LD)
    return (K_CHOL * LD(U) * np.asarray(kappa, LD) * np.abs(Linv).reshape(len(Linv), 9).max(1))[:, None, None]


def line_y(Linv, bl):
    """y = L^-1 bl from a given L^-1 with its mass (n = 3, C_LINE_Y)"""
    Linv, bl = np.asarray(Linv, LD), np.asarray(bl, LD)
    return np.einsum("lrc,lc->lr", Linv, bl), np.einsum("lrc,lc->lr", np.abs(Linv), np.abs(bl))


def lines6(Linv, y):
    """[n,16] device lines {L^-1 (0,0) (1,0) (1,1) (2,0) (2,1) (2,2), y, 7 unused (NaN here)} and back"""
    out = np.full((len(Linv), 16), np.nan)
    for k, (r, c) in enumerate(((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2))):
        out[:, k] = Linv[:, r, c]
    out[:, 6:9] = y
    return out


def lines_from6(rec):
    rec = np.asarray(rec)
    Linv = np.zeros((len(rec), 3, 3), rec.dtype)
    for k, (r, c) in enumerate(((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2))):
        Linv[:, r, c] = rec[:, k]
    return Linv, rec[:, 6:9].copy()


def _per_edge_lines(f, Linv, y, dt, slot0=False):
    """(act [E], L^-1 [E,3,3], y [E,3]) of every slot's landmark; zeros SELECTED for a slot that takes no part in the
    Schur complement (its landmark's line may hold anything)"""
    E, L = f["E"], f["L"]
    act = (f["flags"] & 11) == 0
    if L == 0:
        return act, np.zeros((E, 3, 3), dt), np.zeros((E, 3), dt)
    il = np.where(act, f["lm"], 0)
    if slot0:
        il = 0 * il
    Linv, y = np.asarray(Linv, dt), np.asarray(y, dt)
    return act, np.where(act[:, None, None], Linv[il], 0), np.where(act[:, None], y[il], 0)


def fused_G(Hpl, Linv_e, dtype=LD):
    """G [E,6,3] = Hpl L^-T from per-slot L^-1 [E,3,3] (zeros where the slot takes no part), and its product mass"""
    H, Li = np.asarray(Hpl, dtype), np.asarray(Linv_e, dtype)
    return np.einsum("erm,ecm->erc", H, Li), np.einsum("erm,ecm->erc", np.abs(H), np.abs(Li))


def replay_G(H, Linv_e, act, f32=False, mut=None):
    """float64 replay of the G block of k_build_edges: G[:, m] = sum_{n <= m} H[:, n] L^-1[m][n], left to right, rounded
    to float for float storage; exact zeros where the slot takes no part"""
    H, q = np.asarray(H, np.float64), np.asarray(Linv_e, np.float64)
    if mut == "G_with_Linv":            # L^-1 in place of L^-T: G[:, m] = sum_{n >= m} H[:, n] L^-1[n][m]
        q = q.transpose(0, 2, 1)
    G = np.zeros_like(H)
    for m in range(3):
        s = H[:, :, 0] * q[:, m, 0, None]
        for n in range(1, 3 if mut == "G_with_Linv" else m + 1):
            s = s + H[:, :, n] * q[:, m, n, None]
        G[:, :, m] = s
    G = np.where(np.asarray(act)[:, None, None], G, 0.0)
    return G.astype(np.float32).astype(np.float64) if f32 else G


def pose_schur(prob, rk, f, lam, lines, ref=None, dtype=LD):
    """what k_pose_schur forms, from GIVEN lines (dict Linv [L,3,3], y [L,3]; `lam` is in them already and only named
    here) and the build reference's Xc, e, w (ref = build(prob, rk, f), formed here if not given):
    Hd [P,6,6] = sum JP^T N JP, bp [P,6] = sum JP^T (w e), bsc [P,6] = sum JP^T u over the real edges of each free pose,
    N = w I - w^2 A A^T, u = w (e - A y), A = JL L^-T for an edge between two free vertices and A = 0 otherwise.
    X_mass with absolute values throughout, so that the cancellation inside N and u is inside the bound; n [P]."""
    dt = dtype
    ref = build(prob, rk, f) if ref is None else ref
    P = f["P"]
    real = (f["flags"] & 8) == 0
    ip = f["pose"]
    pf = real & (ip < P)
    _, Li, ye = _per_edge_lines(f, lines["Linv"], lines["y"], dt)
    JP, JL, e, w = (np.asarray(ref[k], dt) for k in ("JP", "JL", "e", "w"))
    aJP, aJL, eb, aw = (np.asarray(ref[k], dt) for k in ("aJP", "aJL", "eb", "aw"))
    A = np.einsum("emi,eji->emj", JL, Li)
    aA = np.einsum("emi,eji->emj", aJL, np.abs(Li))
    I3 = np.eye(3, dtype=dt)
    N = w[:, None, None] * I3 - (w * w)[:, None, None] * np.einsum("emj,enj->emn", A, A)
    # (the mass of w^2 to first order in the error of w, as the mass of |e|^2 in build(): |w| (|w| + 2 (aw - |w|)))
    aw2 = np.abs(w) * (2 * aw - np.abs(w))
    aN = aw[:, None, None] * I3 + aw2[:, None, None] * np.einsum("emj,enj->emn", aA, aA)
    u = w[:, None] * (e - np.einsum("emj,ej->em", A, ye))
    au = aw[:, None] * (eb + np.einsum("emj,ej->em", aA, np.abs(ye)))
    tH = np.einsum("emr,emn,enc->erc", JP, N, JP)
    mH = np.einsum("emr,emn,enc->erc", aJP, aN, aJP)
    tbp = w[:, None] * np.einsum("emr,em->er", JP, e)
    mbp = aw[:, None] * np.einsum("emr,em->er", aJP, eb)
    tbs = np.einsum("emr,em->er", JP, u)
    mbs = np.einsum("emr,em->er", aJP, au)
    s = lambda t: _scatter(ip[pf], t[pf], P)
    n = np.bincount(ip[pf], minlength=P)[:P]
    return dict(Hd=s(tH), Hd_mass=s(mH), bp=s(tbp), bp_mass=s(mbp), bsc=s(tbs), bsc_mass=s(mbs),
                Hd_n=n[:, None, None], bp_n=n[:, None], bsc_n=n[:, None])


def backsubst_lines(f, lam, Linv, y, bl, bp, G, xp, xl=None, dtype=LD):
    """xl [L,3] = L^-T (y - sum_e G_e^T xp[pose(e)]) over the free-free edges of each landmark (zero for a landmark
    without any slot, whatever its line holds), and scale as backsubst(); masses and counts as backsubst()"""
    dt = dtype
    P, L = f["P"], f["L"]
    has = np.diff(f["lm_ptr"])[:L] > 0
    Linv = np.where(has[:, None, None], np.asarray(Linv, dt), 0)
    y = np.where(has[:, None], np.asarray(y, dt), 0)
    bl, bp, G, xp = (np.asarray(a, dt) for a in (bl, bp, G, xp))
    lam = dt(lam)
    ff = (f["flags"] & 11) == 0
    es = np.flatnonzero(ff)
    ls, ps = f["lm"][es], f["pose"][es]
    c = y - _scatter(ls, np.einsum("erc,er->ec", G[es], xp[ps]), L)
    c_mass = np.abs(y) + _scatter(ls, np.einsum("erc,er->ec", np.abs(G[es]), np.abs(xp[ps])), L)
    x = np.einsum("lcr,lc->lr", Linv, c)
    x_mass = np.einsum("lcr,lc->lr", np.abs(Linv), c_mass)
    nl = np.bincount(ls, minlength=L)[:L]
    xu = x if xl is None else np.asarray(xl, dt)
    sp, sl = (xp * (lam * xp + bp)).sum(), (xu * (lam * xu + bl)).sum()
    mp = (np.abs(xp) * (np.abs(lam) * np.abs(xp) + np.abs(bp))).sum()
    ml = (np.abs(xu) * (np.abs(lam) * np.abs(xu) + np.abs(bl))).sum()
    return dict(xl=x, xl_mass=x_mass, xl_n=nl[:, None], scale=sp + sl, scale_mass=mp + ml, scale_n=6 * P + 3 * L)


def _jac_f64(Xc, R, cam, stereo, third_row_for_mono=False):
    """ba_math.h's jac_pose and jac_landmark_R in float64, both branches in their own order of operations"""
    X, Y, Z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    iz = 1.0 / Z
    fu, fv, bf = cam[:, 0], cam[:, 1], cam[:, 4]
    zero = np.zeros_like(X)
    x, y = iz * X, iz * Y
    fu_iz, fv_iz = fu * iz, fv * iz
    JPm = np.zeros((len(X), 3, 6))
    JPm[:, 0] = np.stack([fu * x * y, -fu * (1 + x * x), fu * y, -fu_iz, zero, fu_iz * x], 1)
    JPm[:, 1] = np.stack([fv * (1 + y * y), -fv * x * y, -fv * x, zero, -fv_iz, fv_iz * y], 1)
    JLm = np.zeros((len(X), 3, 3))
    JLm[:, 0] = -fu_iz[:, None] * (R[:, 0] - x[:, None] * R[:, 2])
    JLm[:, 1] = -fv_iz[:, None] * (R[:, 1] - y[:, None] * R[:, 2])
    izz = iz * iz
    JPs = np.zeros((len(X), 3, 6))
    JPs[:, 0] = np.stack([X * Y * izz * fu, -(1 + (X * X * izz)) * fu, Y * iz * fu, -1 * iz * fu, zero, X * izz * fu], 1)
    JPs[:, 1] = np.stack([(1 + Y * Y * izz) * fv, -X * Y * izz * fv, -X * iz * fv, zero, -1 * iz * fv, Y * izz * fv], 1)
    JPs[:, 2] = np.stack([JPs[:, 0, 0] - bf * Y * izz, JPs[:, 0, 1] + bf * X * izz, JPs[:, 0, 2], JPs[:, 0, 3], zero,
                          JPs[:, 0, 5] - bf * izz], 1)
    JLs = np.zeros((len(X), 3, 3))
    JLs[:, 0] = -fu[:, None] * R[:, 0] * iz[:, None] + fu[:, None] * X[:, None] * R[:, 2] * izz[:, None]
    JLs[:, 1] = -fv[:, None] * R[:, 1] * iz[:, None] + fv[:, None] * Y[:, None] * R[:, 2] * izz[:, None]
    JLs[:, 2] = JLs[:, 0] - bf[:, None] * R[:, 2] * izz[:, None]
    if third_row_for_mono:
        JPm[:, 2], JLm[:, 2] = JPs[:, 2], JLs[:, 2]
    st = np.asarray(stereo, bool)[:, None, None]
    return np.where(st, JPs, JPm), np.where(st, JLs, JLm)


def replay_pose_schur(f, ref64, lines, mut=None):
    """float64 replay of k_pose_schur: every edge term in the kernel's order of operations (records Xc, e, w of a
    float64 build reference ref64 = build(..., dtype=np.float64); the rotation of the pose; A, N, u, N JP, JP^T (N JP)),
    inactive terms SELECTED away, then summed per pose.  Returns Hd [P,6,6] (upper triangle mirrored, as the kernel
    stores it), bp, bsc.  mut: one of the mutations of test_fused_ref_host.py"""
    P, E = f["P"], f["E"]
    real = (f["flags"] & 8) == 0
    ip = f["pose"]
    pf = real & (ip < P)
    act, Li, ye = _per_edge_lines(f, lines["Linv"], lines["y"], np.float64, slot0=(mut == "lm_from_slot0"))
    if mut == "inactive_times_zero":    # 0 x whatever the line holds, with the line of slot 0 for an inactive edge
        Linv, y = np.asarray(lines["Linv"], np.float64), np.asarray(lines["y"], np.float64)
        il = np.where(act, f["lm"], 0)
        Li, ye = (Linv[il], y[il]) if f["L"] else (np.full((E, 3, 3), np.nan), np.full((E, 3), np.nan))
    Xc, R, e, wgt = (np.asarray(ref64[k], np.float64) for k in ("Xc", "R", "e", "w"))
    cam = np.asarray(f["cams"], np.float64)[f["cam_id"]]
    stereo = (f["flags"] & 4) != 0
    JP, JL = _jac_f64(Xc, R, cam, stereo, third_row_for_mono=(mut == "mono_third_row"))
    we = wgt[:, None] * e
    K = np.zeros((E, 3, 3))
    K[:, :, 0] = JL[:, :, 0] * Li[:, 0, 0, None]
    K[:, :, 1] = JL[:, :, 0] * Li[:, 1, 0, None] + JL[:, :, 1] * Li[:, 1, 1, None]
    K[:, :, 2] = JL[:, :, 0] * Li[:, 2, 0, None] + JL[:, :, 1] * Li[:, 2, 1, None] + JL[:, :, 2] * Li[:, 2, 2, None]
    w2 = wgt if mut == "N_without_w2" else wgt * wgt
    sel = (lambda v: act.astype(np.float64) * v) if mut == "inactive_times_zero" else (lambda v: np.where(act, v, 0.0))
    N = np.zeros((E, 3, 3))
    for m in range(3):
        for n in range(m, 3):
            mm = K[:, m, 0] * K[:, n, 0] + K[:, m, 1] * K[:, n, 1] + K[:, m, 2] * K[:, n, 2]
            N[:, m, n] = N[:, n, m] = (wgt if m == n else 0.0) - sel(w2 * mm)
    u = np.zeros((E, 3))
    for m in range(3):
        jz = K[:, m, 0] * ye[:, 0] + K[:, m, 1] * ye[:, 1] + K[:, m, 2] * ye[:, 2]
        u[:, m] = we[:, m] + sel(wgt * jz) if mut == "u_with_plus" else we[:, m] - sel(wgt * jz)
    tbp = np.zeros((E, 6)); tbs = np.zeros((E, 6)); tH = np.zeros((E, 6, 6))
    for r in range(6):
        tbp[:, r] = JP[:, 0, r] * we[:, 0] + JP[:, 1, r] * we[:, 1] + JP[:, 2, r] * we[:, 2]
        tbs[:, r] = JP[:, 0, r] * u[:, 0] + JP[:, 1, r] * u[:, 1] + JP[:, 2, r] * u[:, 2]
    for c in range(6):
        g = [N[:, m, 0] * JP[:, 0, c] + N[:, m, 1] * JP[:, 1, c] + N[:, m, 2] * JP[:, 2, c] for m in range(3)]
        for r in range(c + 1):
            tH[:, r, c] = tH[:, c, r] = JP[:, 0, r] * g[0] + JP[:, 1, r] * g[1] + JP[:, 2, r] * g[2]
    if mut == "drop_last_lane":         # the last lane of every 256-lane round of a pose takes no part
        pos = np.zeros(E, np.int64)
        pp = f["pose_ptr"]
        for p in range(P):
            pos[f["pose_edge"][pp[p]:pp[p + 1]]] = np.arange(pp[p + 1] - pp[p])
        deg = np.diff(pp)[np.minimum(ip, len(pp) - 2)]
        pf = pf & ~((pos % 256 == 255) | (pos == deg - 1))
    s = lambda t: _scatter(ip[pf], t[pf], P)
    with np.errstate(invalid="ignore"):
        return dict(Hd=s(tH), bp=s(tbp), bsc=s(tbs))


# ------------------------------------------------------------------ the staged comparison of the fused iteration
# Shared by test_fused_ref_host.py (got = the float64 replay) and test_fused_shapes.py (got = the device).  Every stage
# takes what the stage before it PRODUCED as its input, so that no stage inherits another's conditioning.  Each
# returns the largest |got - ref| / bound of its quantities (ratio()).

def fused_stage_lines(got_Linv, got_y, Hll, bl, lam):
    """stage 2, over the landmarks handed in: L^-1 against fused_lines of the SAME Hll, bl (bound K_CHOL u kappa
    max|L^-1|), y against the given L^-1 x bl ((3 + C_LINE_Y) u mass).  "raw": the L^-1 error in u kappa max|L^-1|."""
    ref = fused_lines(Hll, bl, lam)
    bnd = lines_bound(ref["kappa"], ref["Linv"]) * np.ones((1, 3, 3), LD)
    yr, ym = line_y(got_Linv, bl)
    r = ratio(got_Linv, ref["Linv"], bnd)
    return dict(lines=r, raw=r * K_CHOL, y=ratio(got_y, yr, bound(3, C_LINE_Y, ym)))


def fused_stage_G(got_G, ref, f, got_Linv, f32=False):
    """stage 3: G against the build reference's Hpl x the given L^-1; Hpl's bound carried through |L^-1|, (3 + C_G) u of
    the product mass, float storage 2^-24 (|G| + bound); slots that take no part are exact zeros (mass zero)"""
    _, Li, _ = _per_edge_lines(f, got_Linv, np.zeros((max(f["L"], 1), 3)), LD)
    bH = bound(1, C_HPL, ref["Hpl_mass"])
    G, _ = fused_G(ref["Hpl"], Li)
    _, Gm = fused_G(np.abs(ref["Hpl"]) + bH, Li)
    bnd = np.einsum("erm,ecm->erc", bH, np.abs(Li)) + bound(3, C_G, Gm)
    if f32:
        bnd = bnd + LD(2.0 ** -24) * (np.abs(G) + bnd)
    return ratio(got_G, G, bnd)


def offdiag_from_G(hs, G, dtype=LD):
    """(H [B,6,6] = - sum G_i G_j^T over the product lists of hs, its mass, n [B,1,1]); zero on the diagonal blocks"""
    rowptr, colind, off_ptr, ei, ej = hs
    B = len(colind)
    G = np.asarray(G, dtype)
    blk = np.repeat(np.arange(B), np.diff(off_ptr))
    H = -_scatter(blk, np.einsum("erm,ecm->erc", G[ei], G[ej]), B)
    m = _scatter(blk, np.einsum("erm,ecm->erc", np.abs(G[ei]), np.abs(G[ej])), B)
    return H, m, np.diff(off_ptr)[:, None, None]


def fused_stage_offdiag(got_Hsc, hs, G, P):
    """stage 4, off-diagonal blocks: against - sum G_i G_j^T from the given G with (n + C_HSC) u mass"""
    H, m, n = offdiag_from_G(hs, G)
    off = np.ones(len(hs[1]), bool)
    off[np.asarray(hs[0][:P])] = False
    return ratio(np.asarray(got_Hsc)[off], H[off], bound(n, C_HSC, m)[off])


def fused_stage_pose(got_Hd, got_bp, got_bsc, ps, damp_lam=0.0):
    """stage 4, diagonal blocks, bp and bsc against pose_schur `ps` evaluated from the given lines"""
    I6 = damp_lam * np.eye(6, dtype=LD)
    return dict(diag=ratio(got_Hd, ps["Hd"] + I6, bound(ps["Hd_n"], C_PS_H, ps["Hd_mass"] + I6)),
                bp=ratio(got_bp, ps["bp"], bound(ps["bp_n"], C_PS_BP, ps["bp_mass"])),
                bsc=ratio(got_bsc, ps["bsc"], bound(ps["bsc_n"], C_PS_BSC, ps["bsc_mass"])))


def _schur_sums(f, hs, Tl, Hl, bl_like):
    """(sum T_i H_j^T per block of hs, diagonal blocks over the pose's own edges; sum T bl per pose) for given per-slot
    6 x 3 arrays Tl, Hl and per-landmark 3-vectors bl_like, over the slots between two free vertices"""
    rowptr, colind, off_ptr, ei, ej = hs
    P, B = f["P"], len(colind)
    ff = (f["flags"] & 11) == 0
    es = np.flatnonzero(ff)
    ps = f["pose"][es]
    S = np.zeros((B, 6, 6), LD)
    S[np.asarray(rowptr[:P])] = _scatter(ps, np.einsum("erm,ecm->erc", Tl[es], Hl[es]), P)
    blk = np.repeat(np.arange(B), np.diff(off_ptr))
    S += _scatter(blk, np.einsum("erm,ecm->erc", Tl[ei], Hl[ej]), B)
    ble = bl_like[f["lm"][es]] if f["L"] else np.zeros((len(es), 3), LD)
    return S, _scatter(ps, np.einsum("erm,em->er", Tl[es], ble), P)


def end_to_end_parts(f, hs, lam, ref, rk=None):
    """stage 5: Hsc, bsc of kernel_ref.schur on the build reference `ref` (undamped) and the parts of the per-entry bounds
    for an implementation that builds its own blocks and inverts Hll + lam I itself with entrywise error
    <= k_inv u kappa max|inv| (end_to_end_bounds puts them together).  First order in the errors.
    What every form carries ("prop": the errors of the build pass, through the Schur complement):
      Hpp's, bp's build bound   on the diagonal blocks / on bsc
      Hpl's build bound bH      sum (bH |inv| |Hpl|^T + |Hpl| |inv| bH^T)
      Hll's build bound bL      through the inverse: d = 1.01 |inv| bL |inv| (+ k_inv u kappa max|inv| 11^T: S_k, b_k),
                                sum |Hpl| d |Hpl|^T
      bl's build bound          sum |Hpl| |inv| bbl
    The arithmetic of the forms that store T = Hpl inv ("two": cugo_compute_schur, the two-stream fused form):
      (n + C_HSC + 4) u (|Hpp| + lam + sum |Hpl| |inv| |Hpl|^T), (n + C_BSC + 4) u (|bp| + sum |Hpl| |inv| |bl|)
      (3b of test_kernel_shapes), float storage per rounding 2^-24 S_T.
    The arithmetic of the one-stream form ("one"), whose operands are G = Hpl L^-T and A = JL L^-T: the product
    |L^-T| |L^-1| has none of the cancellation of inv = L^-T L^-1, so its masses are larger than |inv|'s:
      diagonal blocks, bsc      stage 4's own bounds, (n + C_PS_H) u Hd_mass and (n + C_PS_BSC) u bsc_mass of pose_schur
                                at the reference's lines
      off-diagonal blocks       (n + C_HSC + 2 (3 + C_G)) u S_G, S_G = sum |Hpl| |L^-T| |L^-1| |Hpl|^T (the sum, and G's
                                own (3 + C_G) u on either operand); float storage per rounding 2^-24 S_G."""
    P, L = f["P"], f["L"]
    s = schur(f, hs, lam, 0, ref["Hpp"], ref["bp"], ref["Hll"], ref["bl"], ref["Hpl"], want=())
    inv, kappa = np.abs(s["inv"]), s["kappa"]
    il = np.where((f["flags"] & 11) == 0, f["lm"], 0)
    per = lambda a: a[il] if L else np.zeros((f["E"],) + a.shape[1:], LD)
    aH = np.abs(ref["Hpl"])
    bH = bound(1, C_HPL, ref["Hpl_mass"])
    bL = bound(ref["Hll_n"], C_HLL, ref["Hll_mass"])
    bbl = bound(ref["bl_n"], C_BL, ref["bl_mass"])
    ln = fused_lines(ref["Hll"], ref["bl"], lam)
    d = dk_ = LL = np.zeros((0, 3, 3), LD)
    if L:
        d = LD(1.01) * np.einsum("lij,ljk,lkm->lim", inv, bL, inv)
        dk_ = (LD(U) * np.asarray(kappa, LD) * inv.reshape(L, 9).max(1))[:, None, None] * np.ones((1, 3, 3), LD)
        has = np.diff(f["lm_ptr"])[:L] > 0
        aL = np.where(has[:, None, None], np.abs(ln["Linv"]), 0)
        LL = np.einsum("lki,lkj->lij", aL, aL)                      # |L^-T| |L^-1|
    abl = np.abs(ref["bl"])
    HI = np.einsum("erm,emc->erc", aH, per(inv))
    S_T, b_T = _schur_sums(f, hs, HI, aH, abl)
    S_1, b_1 = _schur_sums(f, hs, np.einsum("erm,emc->erc", bH, per(inv)), aH, abl)
    S_2, _ = _schur_sums(f, hs, HI, bH, abl)
    S_d, b_d = _schur_sums(f, hs, np.einsum("erm,emc->erc", aH, per(d)), aH, abl)
    S_k, b_k = _schur_sums(f, hs, np.einsum("erm,emc->erc", aH, per(dk_)), aH, abl)
    S_G, _ = _schur_sums(f, hs, np.einsum("erm,emc->erc", aH, per(LL)), aH, abl)
    _, b_l = _schur_sums(f, hs, HI, aH, bbl)
    dk = np.asarray(hs[0][:P])
    diag = np.zeros((len(hs[1]), 6, 6), LD)
    diag[dk] = np.abs(ref["Hpp"])
    prop_H = S_1 + S_2 + S_d
    prop_H[dk] += bound(ref["Hpp_n"], C_HPP, ref["Hpp_mass"])
    prop_b = bound(ref["bp_n"], C_BP, ref["bp_mass"]) + b_1 + b_d + b_l
    two_H = bound(s["Hsc_n"], C_HSC + 4, diag + S_T)
    two_b = bound(s["bsc_n"], C_BSC + 4, np.abs(ref["bp"]) + b_T)
    ps = pose_schur(None, rk, f, lam, ln, ref=ref)
    one_H = bound(s["Hsc_n"], C_HSC + 2 * (3 + C_G), S_G)
    one_H[dk] = bound(ps["Hd_n"], C_PS_H, ps["Hd_mass"])
    one_b = bound(ps["bsc_n"], C_PS_BSC, ps["bsc_mass"])
    return dict(Hsc=s["Hsc"], bsc=s["bsc"], prop_H=prop_H, prop_b=prop_b, two_H=two_H, two_b=two_b, one_H=one_H,
                one_b=one_b, S_k=S_k, b_k=b_k, S_T=S_T, b_T=b_T, S_G=S_G, dk=dk, Hsc_n=s["Hsc_n"], ps_n=ps["Hd_n"], lam=lam)


def end_to_end_bounds(parts, damp, one_stream):
    """(Hsc, bsc, bound of Hsc, bound of bsc) from end_to_end_parts for one damp flag and one implementation.
    one_stream: its own arithmetic and k_inv = 6 K_CHOL for inv = L^-T L^-1 from lines within stage 2's bound (2 x 3
    products of an entry <= max|L^-1| with an error <= K_CHOL u kappa max|L^-1|, and max|L^-1|^2 <= max|inv|); else the
    arithmetic of the forms that store T and k_inv = K_INV for the adjugate inverse.  The roundings of blocks stored
    as float are added by float_storage_bounds()."""
    p = parts
    dk = p["dk"]
    k_inv = 6 * K_CHOL if one_stream else K_INV
    Hsc = p["Hsc"].copy()
    bH = p["prop_H"] + k_inv * p["S_k"] + (p["one_H"] if one_stream else p["two_H"])
    bb = p["prop_b"] + k_inv * p["b_k"] + (p["one_b"] if one_stream else p["two_b"])
    if damp:
        lamI = p["lam"] * np.eye(6, dtype=LD)
        Hsc[dk] += lamI
        bH[dk] += bound(p["ps_n"], C_PS_H, lamI) if one_stream else bound(p["Hsc_n"][dk], C_HSC + 4, lamI)
    return Hsc, p["bsc"], bH, bb


def float_storage_bounds(parts, one_stream):
    """what float storage of the block streams adds to end_to_end_bounds, 2^-24 of the product sum per rounding on the
    way.  The one-stream form: G = float(Hpl L^-T) from the unrounded Hpl, both operands of an off-diagonal block: 2,
    of S_G; its diagonal blocks and bsc never see a stored block.  The forms that store T: Hpl stored as float,
    T = float(float(Hpl) inv), every block T Hpl^T: 3, of S_T, and 2 for bsc = bp - sum T bl."""
    p = parts
    f24 = LD(2.0 ** -24)
    if one_stream:
        flt = 2 * f24 * p["S_G"]
        flt[p["dk"]] = 0
        return flt, 0 * p["b_T"]
    return 3 * f24 * p["S_T"], 2 * f24 * p["b_T"]
