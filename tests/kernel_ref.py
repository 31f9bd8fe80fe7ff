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
               w=wgt, x=xr, f=f)
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
