"""Extended-precision reference of the landmark covariance kernel (k_lm_covariance of cov_kernels.hip, reached through
cugo_landmark_covariances) with PER-ENTRY error bounds (numpy, test only).

Written from the formula in np.longdouble.  For a free landmark l with Hll = L L^T (lower Cholesky factor) and
G_e = Hpl_e L^-T over its COUNTED edge slots (flags without FIXED_L, FIXED_P, INACTIVE; padding slots are INACTIVE):

    Sigma_l = L^-T (I + sum_{e, f} G_e^T Sigma_{p(e) p(f)} G_f) L^-1

Sigma_{ab}: the block of the pose covariance handed in on the upper block CSR pattern, rows a and columns b; for a > b
the transpose of block (b, a).  The lookup here is a search over the keys a * P + b of ALL blocks that must hit the key
asked for (a pair off the pattern is an error of the design, never another block).  A non-positive or NaN pivot of the
3 x 3 factorisation marks the landmark as failed: its block is nine zeros.  Nothing is read of a slot that does not
count except its flags.

Bound.  With every block comes
    mass = |L^-1|^T (I + sum_{e, f} |G_e|^T |Sigma_ef| |G_f|) |L^-1|,   |G_e| = |Hpl_e| |L^-1|^T
(the same expression without cancellation) and the number of summed terms n = 6 deg_counted^2 (per entry of the sum,
the six products of G_e^T X for every pair).  The bound of an entry is

    K_LM (n + C_LM) u kappa_l mass,     u = 2^-53,  kappa_l = sqrt(cond_2(Hll)) = cond_2(L)

C_LM = 267 roundings on the longest path, counted per formula as kernel_ref.py counts its own:
    L^-1 entries: l10 2, l11 7, l21 14, l22 32, (L^-1)_20 = -(l20 li00 + l21 li10) / l22           -> 62
    G = Hpl L^-T  62 + product 1 + 2 additions -> 65;  X = Sigma G  product 1, 5 additions          -> 71
    G^T X         65 + 71 + product 1 (the additions are n)                                         -> 137
    Y = M L^-1    137 + 62 + 1 + 2 -> 202;  L^-T Y  202 + 62 + 1 + 2                                -> 267
kappa_l: the factor L^-1 comes from a Cholesky factorisation whose differences H11 - l10^2 and H22 - l20^2 - l21^2
cancel, so the error of an entry may grow with a condition number of Hll that a plain count of roundings does not
carry.  Of the two candidate forms, cond(Hll) and its square root, the measurement (tests/test_lm_cov_host.py, design
`far`, cond(Hll) from 1e4 to 4e10) supports the square root, the smaller one: the fp64 replay's worst ratio per decade
of cond(Hll) is flat already in units of (n + C_LM) u mass alone (0.0045 .. 0.0084: |L^-1| grows with the conditioning
and the mass with it), falls by three decades over the range in units of sqrt(cond), and by six in units of
cond.  kappa_l is computed from the inputs alone (numpy.linalg.cond of the float64 Hll).

A pivot that cancellation leaves without a significant bit (|d_j| <= 64 u (H_jj + sum_k l_jk^2), the mass of the
difference) makes the outcome of a double factorisation a matter of rounding: `marginal` names such landmarks (a
landmark that a single mono edge sees has a rank-2 Hll and is one).  For them either a failure or a block inside the
bound is right; everywhere else the reference decides.

K_LM is measured, not derived (test_lm_cov_host.py): 4 x the largest ratio that the float64 run of this same module
reaches against its longdouble run, in either of two summation orders (landmark()), over all designs of
lm_cov_designed.py, rounded up.
"""
import numpy as np

import kernel_ref as kr

LD = kr.LD   # (kernel_ref asserts that np.longdouble is an extended-precision type here)
assert np.finfo(LD).eps < 1e-18, "lm_cov_ref needs an extended-precision np.longdouble: eps = %g" % np.finfo(LD).eps
U = kr.U
C_LM = 267
K_LM = 0.02   # 4 x 0.00422 (design `mixed`), rounded up
# the fp64 replay's worst ratio per design (the larger of its two summation orders) in units of
# (n + C_LM) u sqrt(cond) mass, rounded up (test_lm_cov_host.py)
REPLAY = {"B": 0.0007, "B_padded": 0.0007, "mixed": 0.0043, "corners": 0.0006, "far": 3.0e-5, "grid1": 0.0003,
          "grid256": 0.0015, "grid257": 0.003, "grid513": 0.0021}
SKIP = 1 | 2 | 8   # CUGO_EDGE_FIXED_L | CUGO_EDGE_FIXED_P | CUGO_EDGE_INACTIVE


def counted_slots(f, l):
    lp = f["lm_ptr"]
    es = np.arange(lp[l], lp[l + 1])
    return es[(f["flags"][es] & SKIP) == 0]


def chol3(H, dt, marginal=None):
    """lower Cholesky factor of a symmetric 3 x 3 matrix (its lower triangle is read), or None when a pivot is not
    positive (NaN included); marginal[0] is set when a pivot has no significant bit left"""
    Lf = np.zeros((3, 3), dt)
    for j in range(3):
        sq = (Lf[j, :j] * Lf[j, :j]).sum()
        d = H[j, j] - sq
        if marginal is not None and abs(d) <= 64 * U * (abs(H[j, j]) + sq) and abs(H[j, j]) + sq > 0:
            marginal[0] = True
        if not d > 0:
            return None
        Lf[j, j] = np.sqrt(d)
        for i in range(j + 1, 3):
            Lf[i, j] = (H[i, j] - (Lf[i, :j] * Lf[j, :j]).sum()) / Lf[j, j]
    if not np.all(np.isfinite(Lf)):
        return None
    return Lf


def lower_inverse(Lf, dt):
    """inverse of a lower triangular 3 x 3 matrix by forward substitution, column by column"""
    X = np.zeros((3, 3), dt)
    for c in range(3):
        for r in range(c, 3):
            s = dt(1) if r == c else dt(0)
            X[r, c] = (s - (Lf[r, c:r] * X[c:r, c]).sum()) / Lf[r, r]
    return X


class BlockLookup:
    """Sigma_{ab} for any pair of free poses from the blocks on the upper block CSR pattern"""

    def __init__(self, rowptr, colind, sigma, dt):
        rowptr, colind = np.asarray(rowptr, np.int64), np.asarray(colind, np.int64)
        self.P = len(rowptr) - 1
        rows = np.repeat(np.arange(self.P), np.diff(rowptr))
        self.keys = rows * self.P + colind
        assert np.all(np.diff(self.keys) > 0), "the pattern's columns do not ascend within the rows"
        self.blocks = kr.from_colmajor(np.asarray(sigma, dt).reshape(-1, 36), 6, 6)   # [B, 6, 6], rows a, columns b

    def index(self, pa, pb):
        """(block index, transposed) of Sigma_{pa pb} for arrays of pose indices"""
        a, b = np.minimum(pa, pb), np.maximum(pa, pb)
        key = a.astype(np.int64) * self.P + b
        k = np.searchsorted(self.keys, key)
        assert np.all(k < len(self.keys)) and np.all(self.keys[np.minimum(k, len(self.keys) - 1)] == key), \
            "a pose pair of one landmark is not on the pattern"
        return k, pa > pb

    def get(self, pa, pb, k=None):
        """[..., 6, 6] blocks Sigma_{pa pb}; with k given, the blocks k are read in place of the pair's own"""
        k0, tr = self.index(pa, pb)
        S = self.blocks[k0 if k is None else k]
        return np.where(tr[..., None, None], np.swapaxes(S, -1, -2), S)


def landmark(H, hpl, ps, look, dt=LD, marginal=None, order="rows"):
    """one landmark: (cov [3,3], mass [3,3], Linv, G [d,6,3], S [d,d,6,6]) from its Hll [3,3], the Hpl blocks [d,6,3] and
    pose indices [d] of its counted edges; None when the factorisation fails.  order: how the double sum is added up,
    "rows" (X_e = sum_f Sigma_ef G_f first, then sum_e G_e^T X_e) or "pairs" (the 3 x 3 terms G_e^T Sigma_ef G_f added
    to I one after the other, e outer and f inner: every addition happens at the size of the partial sum)"""
    H = np.asarray(H, dt)
    Lf = chol3(H, dt, marginal)
    if Lf is None:
        return None
    Li = lower_inverse(Lf, dt)
    aLi = np.abs(Li)
    I = np.eye(3, dtype=dt)
    d = len(ps)
    if d:
        hpl = np.asarray(hpl, dt)
        G = hpl @ Li.T
        aG = np.abs(hpl) @ aLi.T
        S = look.get(ps[:, None], ps[None, :])
        if order == "pairs":
            T = np.einsum("eka,efkb->efab", G, np.einsum("efkl,flb->efkb", S, G))
            M = np.cumsum(np.concatenate([I[None], T.reshape(-1, 3, 3)]), axis=0)[-1]
        else:
            M = I + np.einsum("eka,ekb->ab", G, np.einsum("efkl,flb->ekb", S, G))
        aM = I + np.einsum("eka,ekb->ab", aG, np.einsum("efkl,flb->ekb", np.abs(S), aG))
    else:
        G, S, M, aM = np.zeros((0, 6, 3), dt), np.zeros((0, 0, 6, 6), dt), I, I
    return Li.T @ M @ Li, aLi.T @ aM @ aLi, Li, G, S


def reference(f, rowptr, colind, Hll, Hpl, sigma, dtype=LD, only=None, order="rows"):
    """cov [L,3,3], mass [L,3,3], n [L], kappa [L], fail [L], marginal [L] (bool), deg [L] of the free landmarks of the flattened
    layout f from Hll [L,3,3], Hpl [E,6,3] (matrices; slots that do not count are never read) and sigma [B,36]
    (column-major blocks on the pattern).  `only`: the landmarks to evaluate (the others are left zero); `order`: see
    landmark()."""
    dt = dtype
    L = f["L"]
    look = BlockLookup(rowptr, colind, sigma, dt)
    cov, mass = np.zeros((L, 3, 3), dt), np.zeros((L, 3, 3), dt)
    fail = np.zeros(L, bool)
    deg = np.zeros(L, np.int64)
    marginal = np.zeros(L, bool)
    Hll = np.asarray(Hll)
    for l in (range(L) if only is None else only):
        es = counted_slots(f, l)
        deg[l] = len(es)
        m = [False]
        r = landmark(Hll[l], np.asarray(Hpl)[es], f["pose"][es], look, dt, m, order)
        marginal[l] = m[0]
        if r is None:
            fail[l] = True
        else:
            cov[l], mass[l] = r[0], r[1]
    kappa = np.ones(L)   # (of the landmarks that factor; a failed one has no bound)
    if (~fail).any():
        kappa[~fail] = np.linalg.cond(np.asarray(Hll, np.float64)[~fail])
    return dict(cov=cov, mass=mass, n=6 * deg * deg, kappa=kappa, fail=fail, marginal=marginal, deg=deg)


def unit(ref, power=0.5):
    """(n + C_LM) u kappa^power mass per entry [L,3,3]: the bound without K_LM"""
    return (np.asarray(ref["n"], LD) + C_LM)[:, None, None] * LD(U) * (np.asarray(ref["kappa"], LD) ** LD(power))[:, None, None] \
        * np.asarray(ref["mass"], LD)


def bound(ref):
    return LD(K_LM) * unit(ref)


def ratios(got, ref, bnd):
    """per landmark: the largest |got - ref| / bound over the nine entries (0 for failed landmarks, whose block must be
    exactly zero: inf otherwise; a marginal landmark may be either)"""
    got = np.asarray(got, LD).reshape(-1, 3, 3)
    out = np.zeros(len(got))
    for l in range(len(got)):
        if ref["marginal"][l] and not np.any(got[l] != 0):
            out[l] = 0.0
        elif ref["fail"][l]:
            out[l] = 0.0 if not np.any(got[l] != 0) else np.inf
        else:
            out[l] = kr.ratio(got[l], ref["cov"][l], bnd[l])
    return out
