"""Extended-precision reference of the unary pose edges (point-to-plane / point-to-line: icp_kernels.hip; SE(3) priors:
prior_kernels.hip) and of the binary relative-pose SE(3) edges (relpose_kernels.hip, last section) with PER-ENTRY error
bounds, in the manner of tests/kernel_ref.py (numpy, test only).

Written from the formulas in the header comments of the two kernel files, in np.longdouble, vectorised over the edges.
Inputs are plain arrays in the device order (edges sorted by pose); poses [P, 7] = (q x y z w, t).

ICP edges: value, mass, n as kernel_ref defines them
----------------------------------------------------
mass = the same formula with every factor replaced by its cancellation-free absolute value (a difference a - b counts
|a| + |b|), n = the number of edges summed into the entry; a double evaluation in any order, with or without FMA, lies
within (n + c) u mass.  c counts the roundings on the longest path of one term:
    y_i = sum_j R_ij p_j + t_i           R_ij 4, product 1, 3 additions                           ->  8   (mass ay)
  plane
    r = n.y - d                          8, product 1, 2 additions, the subtraction               -> 12   (mass ar)
    J_0..2 = y x n                       8, product 1, the subtraction                            -> 10
    J_3..5 = n                           exact                                                    ->  0
    w = omega rho'(omega r^2)            as kernel_ref: 2 c_r + 5                                 -> 29   (mass aw)
    H += w J_a J_c                       29 + 10 + 10 + product 1 + w 1                           -> 51
    b -= w J_a r                         29 + 10 + 12 + 2                                         -> 53
    chi += rho(omega r^2)                2 x 12 + 1 (square), omega 1, rho 6, 2 spare             -> 34
  line
    dv = y - a                           8 + 1                                                    ->  9
    P_ij = delta_ij - u_i u_j            product, subtraction                                     ->  2
    r_i = sum_j P_ij dv_j                9 + 2 + product 1 + 2 additions                          -> 14
    J_ij = sum_k P_ik S_kj (S = -[y]x)   2 + 8 + 1 + 2                                            -> 13;  J_i,3+j = P_ij -> 2
    w                                    2 x 14 + 5                                               -> 33
    H += w sum_i J_ia J_ic               33 + 13 + 13 + product 1 + 2 additions + w 1             -> 63
    b -= w sum_i J_ia r_i                33 + 13 + 14 + 4                                         -> 64
    chi                                  2 x 14 + 1, 2 additions, omega 1, rho 6                  -> 38
A pose sums both kinds, so the per-pose outputs use the larger (line) constants: C_ICP = H 63, b 64, chi 38.  The masses
follow kernel_ref: |r| + ar wherever r enters a product, aw = w + omega |rho''| omega sum |r_i| (|r_i| + 2 ar_i); the mass
of a chi2 term is |rho| + xmass + rho0.  rho0 (_rho0) is a LOOSENING against kernel_ref's |rho| + xmass, by a constant of
size delta^2 for Cauchy, inside Tukey's and outside Huber's threshold: the robust kernels' own formulas cancel against it
(d2 log(1 + x / d2) rounds 1 + x / d2, so its error is u d2 however small x is), and a chi2 term PER EDGE, which kernel_ref
never bounds, shows it: without rho0 plain double evaluations reach 3.2 x the bound on the smallest residuals of 66 049.
Sensitivity (test_pose_edge_ref_host): on a pose with one plane edge and no robust kernel H[3][3] = w n_x^2 has the
bound (1 + 63) u w n_x^2 = 7.1e-15 relative, so a relative change of w by 1e-12 is seen 140 x over.

Priors: value, first-order error, mass, n
-----------------------------------------
Near theta = pi the rotation part of the residual, phi = (theta / sin theta) s with s = vee(D - D^T) / 2, multiplies a
vector whose mass stays O(1) (|D_ji| + |D_ij|) / 2 by theta / sin theta -> infinity.  Carrying that as a MASS through the
products of J^T Omega J would square the amplification (mass x mass) and bound nothing, so the prior terms carry, next
to the value, a first-order ERROR in units of u, propagated by the two rules of a running error analysis
    a + b:  E = E_a + E_b + |a| + |b|         a b:  E = |a| E_b + |b| E_a + |a b|
(every addition and product one rounding; the same worst-case path count as above, taken per entry instead of as one
constant), and per summed entry `X_err` = sum of the terms' E, `X_mass` = sum |term| and `X_n` = the number of terms:
    bound = u (X_err + n X_mass)                                            (prior_bound)
The angle route.  The reference takes phi from the quaternion of D (q ⊗ conj(q_z), both normalised, w >= 0):
theta = 2 atan2(|v|, w), phi = theta v / |v|, sin theta = 2 w |v|, cos theta = w^2 - |v|^2, cot(theta / 2) = w / |v| —
well conditioned at 0 and at pi — and c(theta) from the Bernoulli series below theta = 0.3 and from
1 / theta^2 - cot(theta / 2) / (2 theta) above.  The ERROR attached to these is that of the formula under test:
    s_i = (D_ji - D_ij) / 2, cs = (tr D - 1) / 2     by the two rules from R_ij (4 roundings each) + 4 u for |q|^2 - 1 of
                                                     the two input quaternions (the formula's R is no rotation then)
    sn = sqrt(s.s)                                   E = |E_s|_2 + K_SQRT sn
    theta = atan2(sn, cs)                            E = |cs| E_sn + sn E_cs + K_ATAN theta       (d atan2, sn^2 + cs^2 = 1)
    f = theta / sn                                   E = |cs sn - theta| / sn^2 E_sn + E_cs + (K_ATAN + 2) f
                                                     (df/dsn, df/dcs: the errors of theta and sn are correlated; below
                                                     theta = 1e-4 the first factor is 2 theta / 3)
    c = A - B, A = 1/theta^2,                        E = |dc/dsn| E_sn + |dc/dcs| E_cs + (2 K_ATAN + 6) (A + B), with theta
        B = (1 + cs) / (2 theta sn)                      eliminated (d theta = cs dsn - sn dcs):
                                                         dc/dsn = -2 cs / theta^3 + B / sn + B cs / theta  (O(1/theta) at 0: the
                                                         errors of A and B through sn cancel), dc/dcs = 2 sn / theta^3
                                                         - 1 / (2 theta sn) - B sn / theta (1 / (2 theta^2) at 0: the ~12 digits
                                                         the closed form loses just above 1e-3; 1 / (2 pi sn) at pi: 1 + cs)
    c = 1/12 + theta^2 / 720 (theta < 1e-3)          E = 2 theta E_theta / 720 + 4 c + theta^4 / (30240 u)
    w = rho'(x), chi = rho(x)                        E_w = |rho''| E_x + K_RHO w,  E_chi = rho' E_x + K_RHO |rho|
K_* are not rounding counts but library / propagation allowances.  Measured on the CPU (test_pose_edge_ref_host.py:
numpy's sqrt, arctan2, log against longdouble on the layouts' values; the largest error in units of u of the result),
4 x rounded up:
    sqrt 0.49 -> K_SQRT = 2;   arctan2 1.18 -> K_ATAN = 5;   rho, rho' (log, sqrt, the cube) 1.62 -> K_RHO = 7

Relative-pose edges (relpose_kernels.hip): the prior's running error carried through A = T_a T_b^-1
----------------------------------------------------------------------------------------------------
The same two rules, per entry; no new allowance constant.  Roundings on the longest path of one entry (what the
running error adds up; the masses are those of the operands, so t_A and u carry the digits they lose):
    R_a, R_b, R_z                        the explicit formula                                     ->  4
    R_A = R_a R_b^T                      4 + 4, product 1, 2 additions                            -> 11
    t_A = t_a - R_A t_b                  11, product 1, 2 additions, the subtraction              -> 15   (|t_a| + |R_A| |t_b|)
    D = R_A R_z^T                        11 + 4, product 1, 2 additions, + 6 for |q|^2 - 1 of the
                                         THREE input quaternions (2 u each, as the prior's + 4)   -> 24
    s, cs, sn, theta, f, c, phi          so3_log_terms: the prior's derivation on this D          (shared code)
    t_D = t_A - D t_z                    24, product 1, 2 additions, the subtraction (15 beside)  -> 28   (|t_A| + |D| |t_z|)
    J_a = [[J_l^-1, 0], [-[t_D]x, I]]    se3_jacobian: the prior's J                              (shared code)
    J_b top left  -J_l^-1 R_A            e(J_l^-1) + 11, product 1, 2 additions
        bottom left ([u]x R_A)_ij        u = t_D - t_A a COUNTED subtraction (28 + 15 + 1, mass |t_D| + |t_A|), times
                                         R_A (11), product 1, the subtraction 1
        bottom right -R_A                11
    Or = Omega r, x = r.Or               6 terms each (1 product, 5 additions); x = max(0, .) is 1-Lipschitz
    rho, w                               E_chi = rho' E_x + K_RHO (|rho| + rho0),  E_w = |rho''| E_x + K_RHO w
    Omega J, J^T (Omega J), J^T Or       6 terms each, then w times the sum (1)
H_aa, H_bb, b_a, b_b and the block H_(lo,hi) = J_lo^T Omega J_hi (J_a^T Omega J_b when a is lo, J_b^T Omega J_a when b is: the
kernel forms it from the side of lo and never transposes) are V-valued per edge; relpose_build scatters value, error
and |value| into H, b, Hoff, chi per pose (at the pose whose walk counts the edge), chi per edge and chi with
    bound = u (X_err + n X_mass)                                            (relpose_bound = prior_bound)
n = the number of edge terms in the entry (the walk's sum, the block's read-modify-write chain, the totals).
Largest error / bound per output over the layouts of pose_designed.relpose_layout (every ratio is printed by the tests):
    float64 replay in the device's order (x86-64, test_relpose_ref_host.py)
        H 0.055   Hoff 0.079   b 0.037   chi 0.019   chi per edge 0.092   chi per pose 0.080
    MI355X (gfx950, test_relpose_shapes.py)
        H 0.062   Hoff 0.095   b 0.032   chi 0.019   chi per edge 0.18 (R-rk2: Tukey, x next to delta^2)
    per layout on the MI355X, H / Hoff / b / chi / chi per edge:
        R-wg1 .0086 / 0 / .0069 / .0042 / .013     R-wg3 .014 / .023 / .012 / .0030 / .019    R-wg4 .053 / .067 / .018 / 1.1e-4 / .010
        R-wg5 .0069 / .015 / .0032 / 6.4e-5 / .011 R-wg8 .053 / .064 / .015 / .0012 / .014    R-wg9 .011 / .030 / .0063 / 1.2e-4 / .016
        R-sides .048 / .057 / .0074 / 4.9e-4 / .027   R-angles .044 / .066 / .017 / 5.5e-4 / .025   R-far .045 / .076 / .032 / 2.2e-4 / .034
        R-rk0 .059 / .080 / .0078 / 4.7e-4 / .032  R-rk1 .0068 / .021 / .0040 / .0026 / .025  R-rk2 .0068 / .0093 / .0078 / .0031 / .18
        R-rk3 .0056 / .025 / .0046 / .0022 / .032  R-info_perEdge .017 / .029 / .021 / .0077 / .068   R-info_one .021 / .028 / .015 / .019 / .060
        R-info_singular .062 / .095 / .018 / 4.7e-4 / .022   R-info_indef .046 / .095 / .018 / 1.3e-4 / .019
        R-zero0..3 .042 / .017 / 0 / 0 / 0         R-totals1024 / 1025 / 1029: chi 1.3e-4 / .0010 / .0018, chi per edge .041 / .035 / .029
"""
import numpy as np

from kernel_ref import LD, U, bound, ratio, _rho, _scatter  # noqa: F401 (re-exported for the tests)

C_ICP = dict(H=63, b=64, chi=38)
C_ICP_PLANE = dict(H=51, b=53, chi=34)
K_SQRT, K_ATAN, K_RHO = 2.0, 5.0, 7.0
ICP_CHUNK, PRIOR_POSES, TOTAL_WG = 512, 8, 256
RELPOSE_POSES = 4


def _rot(q):
    """R(q) by the explicit formula and |R| (every sign a plus), [E, 3, 3]"""
    x, y, z, w = (q[:, k] for k in range(4))
    E = len(q)
    R = np.empty((E, 3, 3), q.dtype)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - z * w); R[:, 0, 2] = 2 * (x * z + y * w)
    R[:, 1, 0] = 2 * (x * y + z * w); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - x * w)
    R[:, 2, 0] = 2 * (x * z - y * w); R[:, 2, 1] = 2 * (y * z + x * w); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    x, y, z, w = (np.abs(q[:, k]) for k in range(4))
    A = np.empty((E, 3, 3), q.dtype)
    A[:, 0, 0] = 1 + 2 * (y * y + z * z); A[:, 0, 1] = 2 * (x * y + z * w); A[:, 0, 2] = 2 * (x * z + y * w)
    A[:, 1, 0] = A[:, 0, 1]; A[:, 1, 1] = 1 + 2 * (x * x + z * z); A[:, 1, 2] = 2 * (y * z + x * w)
    A[:, 2, 0] = A[:, 0, 2]; A[:, 2, 1] = A[:, 1, 2]; A[:, 2, 2] = 1 + 2 * (x * x + y * y)
    return R, A


def _rho0(kind, delta, x, dt):
    """what the mass of rho(x) holds beyond |rho|: Cauchy's d2 log(1 + x / d2) rounds 1 + x / d2 (absolute error u d2 however
    small x is), Tukey's d2 / 3 (1 - (1 - x / d2)^3) is a difference of terms of size d2 / 3 whose cube carries the error of
    1 - x / d2 three times, Huber's outer branch 2 delta sqrt(x) - d2 is a difference: |a| + |b| = |rho| + 2 d2"""
    d2 = dt(delta) * dt(delta)
    if kind == 1:
        return d2 + 0 * x
    if kind in (2, 3):
        return np.where(x <= d2, 2 * d2 if kind == 2 else 0 * d2, 2 * d2 if kind == 3 else 0 * d2) + 0 * x
    return 0 * x


def _skew_neg(y):
    """-[y]x, [E, 3, 3]"""
    S = np.zeros((len(y), 3, 3), y.dtype)
    S[:, 0, 1], S[:, 0, 2], S[:, 1, 0] = y[:, 2], -y[:, 1], -y[:, 2]
    S[:, 1, 2], S[:, 2, 0], S[:, 2, 1] = y[:, 0], y[:, 1], -y[:, 0]
    return S


def icp_terms(kind, poses, n_free, e, dtype=LD, full=True, w_scale=None):
    """per-edge terms of one kind: e = dict(pose [E], p [E,3], n [E,3] + d [E] | a [E,3] + u [E,3], omega [E] or [1],
    active [E] bool, rk).  Returns dict H [E,6,6], b [E,6], chi [E] with X_mass each; edges that do not count are zero.
    w_scale: a factor on the weight (the sensitivity test)"""
    dt = dtype
    pose = np.asarray(e["pose"], int)
    E = len(pose)
    P7 = np.asarray(poses, dt)[pose]
    R, aR = _rot(P7[:, :4])
    p, t = np.asarray(e["p"], dt), P7[:, 4:]
    y = np.einsum("eij,ej->ei", R, p) + t
    ay = np.einsum("eij,ej->ei", aR, np.abs(p)) + np.abs(t)
    S, aS = _skew_neg(y), np.abs(_skew_neg(ay))
    if kind == "plane":
        n, d = np.asarray(e["n"], dt), np.asarray(e["d"], dt)
        an = np.abs(n)
        r = ((n * y).sum(1) - d)[:, None]
        ar = ((an * ay).sum(1) + np.abs(d))[:, None]
        J = np.concatenate([np.einsum("ek,ekj->ej", n, S), n], 1)[:, None, :]
        aJ = np.concatenate([np.einsum("ek,ekj->ej", an, aS), an], 1)[:, None, :]
    else:
        a, u = np.asarray(e["a"], dt), np.asarray(e["u"], dt)
        Pm = np.eye(3, dtype=dt)[None] - u[:, :, None] * u[:, None, :]
        aP = np.eye(3, dtype=dt)[None] + np.abs(u[:, :, None] * u[:, None, :])
        r = np.einsum("eij,ej->ei", Pm, y - a)
        ar = np.einsum("eij,ej->ei", aP, ay + np.abs(a))
        J = np.concatenate([np.einsum("eik,ekj->eij", Pm, S), Pm], 2)
        aJ = np.concatenate([np.einsum("eik,ekj->eij", aP, aS), aP], 2)
    omega = np.broadcast_to(np.asarray(e["omega"], dt), (E,))
    x = omega * (r * r).sum(1)
    xmass = omega * (np.abs(r) * (np.abs(r) + 2 * ar)).sum(1)
    rho, drho, d2rho = _rho(int(e["rk"][0]), e["rk"][1], x, dt)
    live = ((pose < n_free) & np.asarray(e["active"], bool)).astype(dt)
    out = dict(chi=live * rho, chi_mass=live * (np.abs(rho) + xmass + _rho0(int(e["rk"][0]), e["rk"][1], x, dt)), live=live > 0, x=x)
    if full:
        w = live * omega * drho
        if w_scale is not None:
            w = w * dt(w_scale)
        aw = live * (omega * drho + omega * d2rho * xmass)
        rb = np.abs(r) + ar
        out.update(H=w[:, None, None] * np.einsum("eka,ekc->eac", J, J), H_mass=aw[:, None, None] * np.einsum("eka,ekc->eac", aJ, aJ),
                   b=-(w[:, None] * np.einsum("eka,ek->ea", J, r)), b_mass=aw[:, None] * np.einsum("eka,ek->ea", aJ, rb), w=w)
    return out


def icp_build(poses, n_free, kinds, dtype=LD, full=True):
    """kinds: list of (name, e) with name 'plane' / 'line', in the order of the pass (plane first).  H [P,6,6], b [P,6],
    chi_pose [P] (P = n_free), chi_edge (concatenated over the kinds), chi, each with X_mass and X_n"""
    dt = dtype
    P = n_free
    out = dict(H=np.zeros((P, 6, 6), dt), b=np.zeros((P, 6), dt), chi_pose=np.zeros(P, dt))
    for k in ("H", "b", "chi_pose"):
        out[k + "_mass"] = np.zeros_like(out[k])
    cnt = np.zeros(P, np.int64)
    ce, cm = [], []
    for name, e in kinds:
        t = icp_terms(name, poses, n_free, e, dt, full)
        live = t["live"]
        q = np.asarray(e["pose"], int)[live]
        cnt += np.bincount(q, minlength=P)[:P]
        for k in (("H", "b") if full else ()) + ("chi",):
            ko = "chi_pose" if k == "chi" else k
            out[ko] = out[ko] + _scatter(q, t[k][live], P)
            out[ko + "_mass"] = out[ko + "_mass"] + _scatter(q, t[k + "_mass"][live], P)
        ce.append(t["chi"]); cm.append(t["chi_mass"])
    out["chi_edge"] = np.concatenate(ce) if ce else np.zeros(0, dt)
    out["chi_edge_mass"] = np.concatenate(cm) if cm else np.zeros(0, dt)
    out["chi_edge_n"] = 0
    out["chi"], out["chi_mass"], out["chi_n"] = out["chi_edge"].sum(), out["chi_edge_mass"].sum(), int(cnt.sum())
    out["H_n"], out["b_n"], out["chi_pose_n"] = cnt[:, None, None], cnt[:, None], cnt
    return out


def icp_bound(ref, key):
    return bound(ref[key + "_n"], C_ICP["chi" if key.startswith("chi") else key], ref[key + "_mass"])


# ------------------------------------------------------------------ priors: values with a first-order error
class V:
    """an array with a first-order error bound in units of u (see the module docstring)"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v
        self.e = np.zeros_like(v) if e is None else e

    def __add__(self, o):
        return V(self.v + o.v, self.e + o.e + np.abs(self.v) + np.abs(o.v))

    def __sub__(self, o):
        return V(self.v - o.v, self.e + o.e + np.abs(self.v) + np.abs(o.v))

    def __mul__(self, o):
        return V(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + np.abs(self.v * o.v))

    def __neg__(self):
        return V(-self.v, self.e)

    def __getitem__(self, i):
        return V(self.v[i], self.e[i])

    def half(self):
        return V(self.v / 2, self.e / 2)


def mm(spec, A, B, nterms):
    """sum of products under an einsum spec; every product sum passes `nterms` roundings (1 product, nterms - 1 additions)"""
    av, bv = np.abs(A.v), np.abs(B.v)
    return V(np.einsum(spec, A.v, B.v), np.einsum(spec, av, B.e) + np.einsum(spec, A.e, bv) + nterms * np.einsum(spec, av, bv))


def _stack(vs, axis=1):
    return V(np.stack([x.v for x in vs], axis), np.stack([x.e for x in vs], axis))


_BERN = [1.0 / 12, 1.0 / 720, 1.0 / 30240, 1.0 / 1209600, 1.0 / 47900160, 691.0 / 1307674368000, 1.0 / 74724249600]


def c_theta(theta, cot_half):
    """c(theta) = 1/theta^2 - cot(theta/2) / (2 theta): Bernoulli series sum |B_2n| theta^(2n-2) / (2n)! below 0.3"""
    dt = theta.dtype.type
    t2 = theta * theta
    ser = sum(dt(b) * t2 ** k for k, b in enumerate(_BERN))
    with np.errstate(divide="ignore", invalid="ignore"):
        big = 1 / t2 - cot_half / (2 * theta)
    return np.where(theta < 0.3, ser, big)


def _qmul_conj(va, wa, vb, wb):
    """(v, w) of q_a (x) conj(q_b); v [E,3], w [E,1]"""
    return wb * va - wa * vb - np.cross(va, vb), wa * wb + (va * vb).sum(1)[:, None]


def _unit(q):
    return q / np.sqrt((q ** 2).sum(1))[:, None]


def so3_log_terms(D, route, qD=None, sn_switch=1e-12, series_below=1e-3):
    """from D (a V, [E,3,3]) to phi = Log_SO3(D) (a V) and c(theta), its error e_c, theta, sn: the part the prior and the
    relative-pose edges share.  route 'quat': the values from qD = (v [E,3], w [E]), the quaternion of D in longdouble
    (any sign), the errors those of the matrix formula; 'matrix': the formula under test on D.v as it stands"""
    dt = D.v.dtype.type
    E = len(D.v)
    s = _stack([(D[:, 2, 1] - D[:, 1, 2]).half(), (D[:, 0, 2] - D[:, 2, 0]).half(), (D[:, 1, 0] - D[:, 0, 1]).half()])
    one = V(np.ones(E, dt))
    cs = (D[:, 0, 0] + D[:, 1, 1] + D[:, 2, 2] - one).half()
    if route == "quat":
        v, w = qD
        sg = np.where(w < 0, -1, 1).astype(dt)
        v, w = v * sg[:, None], w * sg
        nv = np.sqrt((v * v).sum(1))
        theta = 2 * np.arctan2(nv, w)
        with np.errstate(divide="ignore", invalid="ignore"):
            axis = np.where(nv[:, None] > 0, v / nv[:, None], 0)
            cot_half = w / nv
        s.v, cs.v = 2 * w[:, None] * v, w * w - nv * nv
        sn = 2 * w * nv
        phi_v = theta[:, None] * axis
        cc = c_theta(theta, cot_half)
    else:
        sn = np.sqrt((s.v * s.v).sum(1))
        theta = np.arctan2(sn, cs.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(sn > sn_switch, theta / sn, 1)
        e_sn = np.sqrt((s.e * s.e).sum(1)) + K_SQRT * sn
        e_th = np.abs(cs.v) * e_sn + sn * cs.e + K_ATAN * theta
        g = np.where(theta < 1e-4, theta * 2 / 3 * 1.01, np.abs(cs.v * sn - theta) / (sn * sn))
        e_f = g * e_sn + cs.e + (K_ATAN + 2) * f
        if route != "quat":
            cc = np.where(theta < series_below, dt(1) / 12 + theta * theta / 720, 1 / (theta * theta) - (1 + cs.v) / (2 * theta * sn))
        A, B = 1 / (theta * theta), (1 + cs.v) / (2 * theta * sn)
        dc_dsn = -2 * cs.v / theta ** 3 + B / sn + B * cs.v / theta
        dc_dcs = 2 * sn / theta ** 3 - 1 / (2 * theta * sn) - B * sn / theta
        e_c = np.where(theta < 1e-3, 2 * theta * e_th / 720 + 4 * np.abs(cc) + theta ** 4 / (30240 * U),
                       np.abs(dc_dsn) * e_sn + np.abs(dc_dcs) * cs.e + (2 * K_ATAN + 6) * (A + np.abs(B)))
    phi = V(f[:, None] * s.v, f[:, None] * s.e + np.abs(s.v) * e_f[:, None] + np.abs(f[:, None] * s.v))
    if route == "quat":
        phi.v = phi_v
    return phi, cc, e_c, theta, sn


def se3_jacobian(phi, cc, e_c, tD):
    """J = [[J_l^-1, 0], [-[tD]x, I]] (a V, [E,6,6]) and J_l^-1 = I - K/2 + c K2, K = [phi]x, K2 = K K written out"""
    dt = phi.v.dtype.type
    E = len(phi.v)
    p0, p1, p2 = phi[:, 0], phi[:, 1], phi[:, 2]
    zero = V(np.zeros(E, dt))
    K = _stack([_stack([zero, -p2, p1]), _stack([p2, zero, -p0]), _stack([-p1, p0, zero])])
    K2 = _stack([_stack([-(p1 * p1 + p2 * p2), p0 * p1, p0 * p2]), _stack([p0 * p1, -(p0 * p0 + p2 * p2), p1 * p2]),
                 _stack([p0 * p2, p1 * p2, -(p0 * p0 + p1 * p1)])])
    cV = V(cc[:, None, None] + 0 * K2.v, e_c[:, None, None] + 0 * K2.v)
    I3 = V(np.broadcast_to(np.eye(3, dtype=dt), (E, 3, 3)).copy())
    Jr = (I3 - K.half()) + cV * K2
    t0, t1, t2 = tD[:, 0], tD[:, 1], tD[:, 2]
    Jt = _stack([_stack([zero, t2, -t1]), _stack([-t2, zero, t0]), _stack([t1, -t0, zero])])
    J = V(np.zeros((E, 6, 6), dt))
    J.v[:, :3, :3], J.e[:, :3, :3] = Jr.v, Jr.e
    J.v[:, 3:, :3], J.e[:, 3:, :3] = Jt.v, Jt.e
    J.v[:, 3:, 3:] = np.eye(3, dtype=dt)
    return J, Jr


def prior_terms(poses, n_free, pr, dtype=LD, route="quat", sn_switch=1e-12, series_below=1e-3, full=True, w_scale=None):
    """per-edge terms of a prior set pr = dict(pose [E], z [E,7], info [E or 1,6,6], active [E], rk): V-valued H [E,6,6],
    b [E,6], chi [E] (zero where the edge does not count) and the angle quantities theta, sn.  route 'quat': the
    well-conditioned reference values (longdouble); 'matrix': the formula under test as it stands (what a double
    evaluation does; sn_switch and series_below are its two switches)"""
    dt = dtype
    pose = np.asarray(pr["pose"], int)
    E = len(pose)
    P7 = np.asarray(poses, dt)[pose]
    z = np.asarray(pr["z"], dt).reshape(E, 7)
    Om = np.broadcast_to(np.asarray(pr["info"], dt).reshape(-1, 6, 6), (E, 6, 6))
    Rv, aR = _rot(P7[:, :4])
    Zv, aZ = _rot(z[:, :4])
    R, Rz = V(Rv, 4 * aR), V(Zv, 4 * aZ)
    D = mm("eik,ejk->eij", R, Rz, 3)
    D.e = D.e + 4                                         # |q|^2 - 1 of the two input quaternions
    qD = None
    if route == "quat":
        qa, qb = _unit(P7[:, :4]), _unit(z[:, :4])
        v, w = _qmul_conj(qa[:, :3], qa[:, 3:], qb[:, :3], qb[:, 3:])
        qD = (v, w[:, 0])
    phi, cc, e_c, theta, sn = so3_log_terms(D, route, qD, sn_switch, series_below)
    T = V(P7[:, 4:].copy())
    tD = T - mm("eij,ej->ei", D, V(z[:, 4:].copy()), 3)
    r = V(np.concatenate([phi.v, tD.v], 1), np.concatenate([phi.e, tD.e], 1))
    OmV = V(np.ascontiguousarray(Om))
    Or = mm("eij,ej->ei", OmV, r, 6)
    xr = mm("ei,ei->e", r, Or, 6)
    x = np.maximum(0, xr.v)
    rho, drho, d2rho = _rho(int(pr["rk"][0]), pr["rk"][1], x, dt)
    live = ((pose < n_free) & np.asarray(pr["active"], bool)).astype(dt)
    chi = V(live * rho, live * (drho * xr.e + K_RHO * (np.abs(rho) + _rho0(int(pr["rk"][0]), pr["rk"][1], x, dt))))
    out = dict(chi=chi, theta=theta, sn=sn, x=x, live=live > 0, c=cc, e_c=e_c, e_phi=phi.e, phi=phi.v)
    if not full:
        return out
    w = V(live * drho, live * (d2rho * xr.e + K_RHO * drho))
    if w_scale is not None:                 # (the sensitivity test)
        w.v = w.v * dt(w_scale)
    J, _ = se3_jacobian(phi, cc, e_c, tD)
    OJ = mm("eik,ekj->eij", OmV, J, 6)
    Hs = mm("eka,ekc->eac", J, OJ, 6)
    bs = mm("eka,ek->ea", J, Or, 6)
    out["H"] = V(w.v[:, None, None] + 0 * Hs.v, w.e[:, None, None] + 0 * Hs.v) * Hs
    out["b"] = -(V(w.v[:, None] + 0 * bs.v, w.e[:, None] + 0 * bs.v) * bs)
    return out


def prior_build(poses, n_free, pr, dtype=LD, route="quat", full=True, **switches):
    """H [P,6,6], b [P,6], chi_pose [P], chi_edge [E], chi with X_err, X_mass, X_n each (prior_bound)"""
    dt = dtype
    P = n_free
    E = len(pr["pose"])
    out = {}
    if E == 0:
        for k, shp in (("H", (P, 6, 6)), ("b", (P, 6)), ("chi_pose", (P,)), ("chi_edge", (0,))):
            out[k], out[k + "_err"], out[k + "_mass"], out[k + "_n"] = np.zeros(shp, dt), np.zeros(shp, dt), np.zeros(shp, dt), 0
        out["chi"], out["chi_err"], out["chi_mass"], out["chi_n"] = dt(0), dt(0), dt(0), 0
        out["terms"] = None
        return out
    t = prior_terms(poses, n_free, pr, dt, route, full=full, **switches)
    live = t["live"]
    q = np.asarray(pr["pose"], int)[live]
    cnt = np.bincount(q, minlength=P)[:P]
    for k in (("H", "b") if full else ()) + ("chi",):
        ko = "chi_pose" if k == "chi" else k
        out[ko] = _scatter(q, t[k].v[live], P)
        out[ko + "_err"] = _scatter(q, t[k].e[live], P)
        out[ko + "_mass"] = _scatter(q, np.abs(t[k].v[live]), P)
    if full:
        out["H_n"], out["b_n"] = cnt[:, None, None], cnt[:, None]
    out["chi_pose_n"] = cnt
    out["chi_edge"], out["chi_edge_err"], out["chi_edge_mass"], out["chi_edge_n"] = t["chi"].v, t["chi"].e, np.abs(t["chi"].v), 0
    out["chi"], out["chi_err"], out["chi_mass"], out["chi_n"] = t["chi"].v.sum(), t["chi"].e.sum(), np.abs(t["chi"].v).sum(), int(cnt.sum())
    out["terms"] = t
    return out


def prior_bound(ref, key):
    return LD(U) * (np.asarray(ref[key + "_err"], LD) + np.asarray(ref[key + "_n"], LD) * np.asarray(ref[key + "_mass"], LD))


# ------------------------------------------------------------------ float64 replays of the device's order
def chi_total(totals, cap=None):
    """k_pose_chi_total: thread t sums totals[t], totals[t + 256], ...; then the threads in order.  cap: a mutation,
    totals from index `cap` on are dropped"""
    totals = np.asarray(totals, np.float64)
    if cap is not None:
        totals = totals[:cap]
    x = np.zeros(TOTAL_WG)
    for i0 in range(0, len(totals), TOTAL_WG):
        seg = totals[i0:i0 + TOTAL_WG]
        x[:len(seg)] += seg
    tot = 0.0
    for v in x:
        tot += v
    return tot


def icp_replay(poses, n_free, n_poses_total, kinds, mut=None):
    """float64 evaluation in the order of icp_kernels.hip: per kind chunks of 512 edges in groups of 64 lanes, the lanes
    of one pose summed into the wave's accumulators, a partial flushed to slot chunk + pose whenever the pose changes
    and at the chunk's end, one chi2 total per chunk; the finishing pass sums slots c + p in chunk order (plane, then
    line) and mirrors the upper triangle.  mut: one of None, 'finish_early', 'rank_slots', 'drop_lane', 'fixed_free',
    'totals_256', 'no_mirror'.  Returns H [P,6,6], b [P,6], chi, chi_edge, chi per pose"""
    P = n_free
    nf = n_free + 1 if mut == "fixed_free" else n_free
    iu = np.triu_indices(6)
    H, b = np.zeros((P, 6, 6)), np.zeros((P, 6))
    sums = np.zeros((P, 28))
    totals, chi_edge = [], []
    for name, e in kinds:
        pose = np.asarray(e["pose"], int)
        n = len(pose)
        t = icp_terms(name, poses, nf, e, np.float64)
        v = np.concatenate([t["H"][:, iu[0], iu[1]], t["b"], t["chi"][:, None]], 1)      # [n, 28]
        chi_edge.append(t["chi"])
        nc = (n + ICP_CHUNK - 1) // ICP_CHUNK
        part = np.zeros((nc + n_poses_total + 1, 28))
        has = np.zeros(n_poses_total, bool)
        has[pose] = True
        rank = np.cumsum(has) - 1
        idx = np.arange(n)
        if mut == "drop_lane" and n:     # a flush inside a 64-lane group (two poses in it): its last lane is lost
            g0 = np.arange(0, n, 64)
            g1 = np.minimum(g0 + 64, n) - 1
            v[g1[pose[g0] != pose[g1]]] = 0.0
        # segments of equal (group, pose): group boundaries include chunk boundaries
        key_change = np.flatnonzero((np.diff(idx // 64) != 0) | (np.diff(pose) != 0)) + 1 if n > 1 else np.zeros(0, int)
        starts = np.concatenate([[0], key_change]).astype(int) if n else np.zeros(0, int)
        ends = np.concatenate([starts[1:], [n]]).astype(int) if n else starts
        seg = np.add.reduceat(v, starts, axis=0) if n else np.zeros((0, 28))
        cchi = np.zeros(nc)
        acc, cur = np.zeros(28), None          # cur = (chunk, pose)
        for k in range(len(starts)):
            s0 = starts[k]
            c, q = s0 // ICP_CHUNK, pose[s0]
            if cur is not None and cur != (c, q):
                slot = cur[0] + (rank[cur[1]] if mut == "rank_slots" else cur[1])
                part[slot] = acc
                cchi[cur[0]] += acc[27]
                acc = np.zeros(28)
            cur = (c, q)
            acc = acc + seg[k]
        if cur is not None:
            slot = cur[0] + (rank[cur[1]] if mut == "rank_slots" else cur[1])
            part[slot] = acc
            cchi[cur[0]] += acc[27]
        totals.append(cchi)
        ptr = np.searchsorted(pose, np.arange(n_poses_total + 1))
        for p in range(P):
            i0, i1 = ptr[p], ptr[p + 1]
            if i1 > i0:
                c0, c1 = i0 // ICP_CHUNK, (i1 - 1) // ICP_CHUNK
                ssum = np.zeros(28)
                for c in range(c0, c1 if mut == "finish_early" else c1 + 1):
                    ssum = ssum + part[c + p]
                sums[p] = sums[p] + ssum
    H[:, iu[0], iu[1]] = sums[:, :21]
    if mut != "no_mirror":
        H[:, iu[1], iu[0]] = sums[:, :21]
    b[:] = sums[:, 21:27]
    totals = np.concatenate(totals) if totals else np.zeros(0)
    chi = chi_total(totals, TOTAL_WG if mut == "totals_256" else None)
    return H, b, chi, (np.concatenate(chi_edge) if chi_edge else np.zeros(0)), sums[:, 27].copy()


def prior_replay(poses, n_free, pr, mut=None):
    """float64 evaluation in the order of prior_kernels.hip: the priors of a pose in container order, one chi2 total per
    workgroup of 8 poses, the totals by chi_total.  mut: None, 'f_switch_1e-9', 'f_switch_1e-3', 'series_1e-1',
    'totals_256', 'no_mirror'"""
    P = n_free
    sw = {}
    if mut == "f_switch_1e-9":
        sw["sn_switch"] = 1e-9
    if mut == "f_switch_1e-3":
        sw["sn_switch"] = 1e-3
    if mut == "series_1e-1":
        sw["series_below"] = 1e-1
    H, b, cp = np.zeros((P, 6, 6)), np.zeros((P, 6)), np.zeros(P)
    E = len(pr["pose"])
    if E == 0 or P == 0:
        return H, b, 0.0, np.zeros(E), cp
    t = prior_terms(poses, n_free, pr, np.float64, "matrix", **sw)
    pose = np.asarray(pr["pose"], int)
    live = t["live"]
    iu = np.triu_indices(6)
    for e in np.flatnonzero(live):
        p = pose[e]
        H[p][iu] += t["H"].v[e][iu]
        b[p] += t["b"].v[e]
        cp[p] += t["chi"].v[e]
    if mut != "no_mirror":
        H[:, iu[1], iu[0]] = H[:, iu[0], iu[1]]
    nwg = (P + PRIOR_POSES - 1) // PRIOR_POSES
    wg = np.zeros(nwg)
    for g in range(nwg):
        tot = 0.0
        for i in range(PRIOR_POSES):
            if g * PRIOR_POSES + i < P:
                tot += cp[g * PRIOR_POSES + i]
        wg[g] = tot
    return H, b, chi_total(wg, TOTAL_WG if mut == "totals_256" else None), t["chi"].v, cp


# ------------------------------------------------------------------ relative-pose edges (relpose_kernels.hip)
def relpose_effective(rp):
    """the edge dict with the run-time flags folded in: an edge counts when the plan's flags (rp['active']) AND the
    flags the device is given (rp['rt_active'], optional) leave it active"""
    rt = rp.get("rt_active")
    return rp if rt is None else dict(rp, active=np.asarray(rp["active"], bool) & np.asarray(rt, bool))


def _bc(w, like):
    """a per-edge V broadcast to the shape of `like`"""
    idx = (slice(None),) + (None,) * (like.v.ndim - 1)
    return V(w.v[idx] + 0 * like.v, w.e[idx] + 0 * like.v)


def relpose_terms(poses, n_free, rp, dtype=LD, route="quat", full=True, w_scale=None, sn_switch=1e-12, series_below=1e-3):
    """per-edge terms of a relpose_ref.make_edges dict (optionally with rt_active): V-valued chi [E], and with `full`
    H_aa, H_bb, H_lohi [E,6,6] (the block (lo, hi) = J_lo^T Omega J_hi whichever of a, b is lo), b_a, b_b [E,6]; each is zero
    where the edge does not count or the pose it belongs to is fixed.  Routes as prior_terms"""
    import relpose_ref as RR
    dt = dtype
    a, b = np.asarray(rp["a"], int), np.asarray(rp["b"], int)
    E = len(a)
    Pa, Pb = np.asarray(poses, dt)[a], np.asarray(poses, dt)[b]
    z = np.asarray(rp["z"], dt).reshape(E, 7)
    Om = np.broadcast_to(np.asarray(rp["info"], dt).reshape(-1, 6, 6), (E, 6, 6))
    Ra, Rb, Rz = (V(v, 4 * m) for v, m in (_rot(Pa[:, :4]), _rot(Pb[:, :4]), _rot(z[:, :4])))
    RA = mm("eik,ejk->eij", Ra, Rb, 3)
    tA = V(Pa[:, 4:].copy()) - mm("eij,ej->ei", RA, V(Pb[:, 4:].copy()), 3)
    D = mm("eik,ejk->eij", RA, Rz, 3)
    D.e = D.e + 6                                         # |q|^2 - 1 of the three input quaternions, 2 u each as for the prior
    qD = None
    if route == "quat":
        qa, qb, qz = _unit(Pa[:, :4]), _unit(Pb[:, :4]), _unit(z[:, :4])
        v, w = _qmul_conj(qa[:, :3], qa[:, 3:], qb[:, :3], qb[:, 3:])
        v, w = _qmul_conj(v, w, qz[:, :3], qz[:, 3:])
        qD = (v, w[:, 0])
    phi, cc, e_c, theta, sn = so3_log_terms(D, route, qD, sn_switch, series_below)
    tD = tA - mm("eij,ej->ei", D, V(z[:, 4:].copy()), 3)
    r = V(np.concatenate([phi.v, tD.v], 1), np.concatenate([phi.e, tD.e], 1))
    OmV = V(np.ascontiguousarray(Om))
    Or = mm("eij,ej->ei", OmV, r, 6)
    xr = mm("ei,ei->e", r, Or, 6)
    x = np.maximum(0, xr.v)
    kind, delta = int(rp["rk"][0]), rp["rk"][1]
    rho, drho, d2rho = _rho(kind, delta, x, dt)
    eff = relpose_effective(rp)
    cnt = RR.counting(eff, n_free)
    live = cnt.astype(dt)
    chi = V(live * rho, live * (drho * xr.e + K_RHO * (np.abs(rho) + _rho0(kind, delta, x, dt))))
    tA_rel = np.sqrt((tA.v ** 2).sum(1)) / np.maximum(np.abs(Pa[:, 4:]).sum(1) + np.einsum("eij,ej->ei", np.abs(RA.v), np.abs(Pb[:, 4:])).sum(1), dt(1e-300))
    out = dict(chi=chi, theta=theta, sn=sn, x=x, xr=xr.v, live=cnt, r=r.v, tA=tA.v, tA_rel=tA_rel)
    if not full:
        return out
    w = V(live * drho, live * (d2rho * xr.e + K_RHO * drho))
    if w_scale is not None:                 # (the sensitivity test: one factor, or one per edge)
        w.v = w.v * np.asarray(w_scale, dt)
    Ja, Jl = se3_jacobian(phi, cc, e_c, tD)
    # J_b entry by entry as the kernel writes it: [[-J_l^-1 R_A, 0], [[u]x R_A, -R_A]], u = t_D - t_A
    u = tD - tA
    u0, u1, u2 = (V(u.v[:, k:k + 1], u.e[:, k:k + 1]) for k in range(3))
    bot = _stack([u1 * RA[:, 2, :] - u2 * RA[:, 1, :], u2 * RA[:, 0, :] - u0 * RA[:, 2, :], u0 * RA[:, 1, :] - u1 * RA[:, 0, :]])
    top = -mm("eik,ekj->eij", Jl, RA, 3)
    Jb = V(np.zeros((E, 6, 6), dt))
    Jb.v[:, :3, :3], Jb.e[:, :3, :3] = top.v, top.e
    Jb.v[:, 3:, :3], Jb.e[:, 3:, :3] = bot.v, bot.e
    Jb.v[:, 3:, 3:], Jb.e[:, 3:, 3:] = -RA.v, RA.e
    OJa, OJb = mm("eik,ekj->eij", OmV, Ja, 6), mm("eik,ekj->eij", OmV, Jb, 6)
    fa, fb = (a < n_free).astype(dt), (b < n_free).astype(dt)
    a_lo = a < b

    def scaled(Xs, keep):
        t = _bc(w, Xs) * Xs
        k = keep[(slice(None),) + (None,) * (Xs.v.ndim - 1)]
        return V(t.v * k, t.e * k)
    Hab, Hba = mm("eka,ekc->eac", Ja, OJb, 6), mm("eka,ekc->eac", Jb, OJa, 6)
    lohi = V(np.where(a_lo[:, None, None], Hab.v, Hba.v), np.where(a_lo[:, None, None], Hab.e, Hba.e))
    out.update(H_aa=scaled(mm("eka,ekc->eac", Ja, OJa, 6), fa), H_bb=scaled(mm("eka,ekc->eac", Jb, OJb, 6), fb),
               H_lohi=scaled(lohi, fa * fb), b_a=-scaled(mm("eka,ek->ea", Ja, Or, 6), fa), b_b=-scaled(mm("eka,ek->ea", Jb, Or, 6), fb),
               w=w.v, Ja=Ja.v, Jb=Jb.v)
    return out


def relpose_build(poses, n_free, rp, rowptr=None, colind=None, dtype=LD, route="quat", full=True, w_scale=None):
    """H [P,6,6], b [P,6], Hoff [nnzb,6,6] on the pattern (relpose_ref.pattern of the plan's edges unless one is given; only
    the (lo, hi) blocks are filled), chi_pose [P] (an edge's term at the pose whose walk counts it: a when a is free,
    else b), chi_edge [E], chi; each with X_err, X_mass, X_n (relpose_bound).  An edge counts as relpose_ref.counting says"""
    import relpose_ref as RR
    dt = dtype
    P = n_free
    if rowptr is None:
        rowptr, colind = RR.pattern(rp, n_free)
    nnzb = len(colind)
    a, b = np.asarray(rp["a"], int), np.asarray(rp["b"], int)
    t = relpose_terms(poses, n_free, rp, dt, route, full=full, w_scale=w_scale)
    live = t["live"]
    out = dict(terms=t)

    def put(key, idx, n, parts):
        """parts: list of (edge mask, V) scattered by idx[mask]"""
        val = err = mass = 0
        cnt = np.zeros(n, np.int64)
        for (m, X), ix in zip(parts, idx):
            val = val + _scatter(ix[m], X.v[m], n)
            err = err + _scatter(ix[m], X.e[m], n)
            mass = mass + _scatter(ix[m], np.abs(X.v[m]), n)
            cnt += np.bincount(ix[m], minlength=n)[:n]
        out[key], out[key + "_err"], out[key + "_mass"] = val, err, mass
        out[key + "_n"] = cnt.reshape((n,) + (1,) * (np.ndim(val) - 1))
    ma, mb = live & (a < P), live & (b < P)
    if full:
        put("H", (a, b), P, [(ma, t["H_aa"]), (mb, t["H_bb"])])
        put("b", (a, b), P, [(ma, t["b_a"]), (mb, t["b_b"])])
        both = ma & mb
        blk = np.full(len(a), 0, int)
        for e in np.flatnonzero(both):
            blk[e] = RR.block_of(rowptr, colind, min(a[e], b[e]), max(a[e], b[e]))
        put("Hoff", (blk,), nnzb, [(both, t["H_lohi"])])
    owner = np.where(a < P, a, b)
    put("chi_pose", (owner,), P, [(live, t["chi"])])
    out["chi_edge"], out["chi_edge_err"], out["chi_edge_mass"], out["chi_edge_n"] = t["chi"].v, t["chi"].e, np.abs(t["chi"].v), 0
    out["chi"], out["chi_err"], out["chi_mass"], out["chi_n"] = t["chi"].v.sum(), t["chi"].e.sum(), np.abs(t["chi"].v).sum(), int(live.sum())
    return out


def relpose_bound(ref, key):
    return prior_bound(ref, key)


def relpose_chi_in_device_order(chi_edge, n_free, rp, rowptr, colind):
    """the chi2 total of given per-edge terms summed as relpose_kernels.hip sums them (float64 additions only, so the
    device's own per-edge terms give the device's total bit for bit): per free pose the terms its walk counts, in edge
    order; one total per RELPOSE_POSES poses; chi_total"""
    import relpose_ref as RR
    P = n_free
    a, b = np.asarray(rp["a"], int), np.asarray(rp["b"], int)
    inc_ptr, inc, _ = RR.plan(rp, n_free, rowptr, colind)
    rt = np.ones(len(a), bool) if rp.get("rt_active") is None else np.asarray(rp["rt_active"], bool)
    chi_edge = np.asarray(chi_edge, np.float64)
    wg = np.zeros((P + RELPOSE_POSES - 1) // RELPOSE_POSES)
    for g in range(len(wg)):
        tot = 0.0
        for p in range(g * RELPOSE_POSES, min((g + 1) * RELPOSE_POSES, P)):
            chi = 0.0
            for rec in inc[inc_ptr[p]:inc_ptr[p + 1]]:
                e, side = int(rec) >> 1, int(rec) & 1
                if rt[e] and (side == 0 or (a[e] if side else b[e]) >= P):
                    chi += chi_edge[e]
            tot += chi
        wg[g] = tot
    return chi_total(wg)


def relpose_replay(poses, n_free, rp, rowptr, colind, mut=None):
    """float64 evaluation in the order of relpose_kernels.hip: per free pose its incidence list in edge order (the plan of
    relpose_ref.plan over rp['active']; rp['rt_active'] are the flags the device skips by), the diagonal term and b
    summed over the walk and added once (upper triangle, mirrored), Hoff added edge after edge in the walk of lo, chi2
    counted by the walk of a when a is free, else by b's, one total per RELPOSE_POSES poses, then chi_total.  Per-edge
    terms from relpose_ref.edge_terms.  mut: None, 'chi2_twice', 'transposed', 'no_tA' (= u = t_D instead of t_D - t_A),
    'overwrite', 'Ja_for_Jb_fixed', 'chi_from_b', 'rt_counted', 'drop_second', 'totals_256'.
    Returns H [P,6,6], b [P,6], Hoff [nnzb,6,6], chi, chi_edge [E], chi per pose [P]"""
    import relpose_ref as RR
    P = n_free
    a, b = np.asarray(rp["a"], int), np.asarray(rp["b"], int)
    E = len(a)
    inc_ptr, inc, off = RR.plan(rp, n_free, rowptr, colind)
    rt = np.ones(E, bool) if rp.get("rt_active") is None or mut == "rt_counted" else np.asarray(rp["rt_active"], bool)
    Om = np.broadcast_to(np.asarray(rp["info"], np.float64).reshape(-1, 6, 6), (E, 6, 6)) if E else None
    rk = rp.get("rk", (0, 1.0))
    poses = np.asarray(poses, np.float64)
    terms = {}
    H, bb, Hoff = np.zeros((P, 6, 6)), np.zeros((P, 6)), np.zeros((len(colind), 6, 6))
    ce, cp = np.zeros(E), np.zeros(P)
    iu = np.triu_indices(6)
    seen = {}
    for p in range(P):
        mH, mb, chi = np.zeros((6, 6)), np.zeros(6), 0.0
        for rec in inc[inc_ptr[p]:inc_ptr[p + 1]]:
            e, side = int(rec) >> 1, int(rec) & 1
            if not rt[e]:
                continue
            if e not in terms:
                terms[e] = RR.edge_terms(poses[a[e]], poses[b[e]], rp["z"][e], Om[e], rk, with_tA=mut != "no_tA")
            c, Haa, Hbb, Hab, ba, b_b = terms[e]
            other = a[e] if side else b[e]
            counts_chi = (side == 1 or other >= P) if mut == "chi_from_b" else (side == 0 or other >= P)
            if mut == "chi2_twice":
                counts_chi = True
            if counts_chi:
                chi += c
                ce[e] = c
            own_b = side == 1 and not (mut == "Ja_for_Jb_fixed" and other >= P)
            mH += Hbb if own_b else Haa
            mb += b_b if own_b else ba
            if other < P and p < other:
                k = off[e]
                seen[k] = seen.get(k, 0) + 1
                blk = Hab if side == 0 or mut == "transposed" else Hab.T
                if mut == "overwrite":
                    Hoff[k] = blk
                elif not (mut == "drop_second" and seen[k] == 2):
                    Hoff[k] += blk
        H[p][iu] += mH[iu]
        bb[p] += mb
        cp[p] = chi
    H[:, iu[1], iu[0]] = H[:, iu[0], iu[1]]
    nwg = (P + RELPOSE_POSES - 1) // RELPOSE_POSES
    wg = np.zeros(nwg)
    for g in range(nwg):
        tot = 0.0
        for i in range(RELPOSE_POSES):
            if g * RELPOSE_POSES + i < P:
                tot += cp[g * RELPOSE_POSES + i]
        wg[g] = tot
    return H, bb, Hoff, chi_total(wg, TOTAL_WG if mut == "totals_256" else None), ce, cp
