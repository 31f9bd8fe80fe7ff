"""Sparse patterns with PRESCRIBED fronts for the sparse Cholesky, value classes for them, and the metrics the designed
Cholesky tests hold results against (numpy only besides the plan getters; a plain helper module).

The kernels of chol_kernels.hip / cov_kernels.hip branch on a front's pivot width ncb (ncp = pad16(6 ncb), two waves on
the first panel when ncp > 64), on its boundary nb - ncb (the right-hand-side row nt = 6 (nb - ncb) + 1 against the
32- and 64-row tiles, SI_R = 64 / SI_K = 32 of the selected inverse, the <= 16-row segments of k_backward_chain) and on
its children (EA_BATCH = 32 per batch, `rel` counted in 64-lane strides).  test_host.patterns() reaches few of these
edges, so here they are an input:

a *clique pattern* is a separator clique of `sep` block nodes plus leaves; a leaf (c, r) is c private nodes that form a
clique with each other and with the first r separator nodes.  The ordering eliminates a leaf's private nodes first and
as one supernode, so the plan holds a front with ncb = c and nb - ncb = r (census() checks it; `sep` must stay larger
than the largest r, or the widest leaf is merged into the separator chain).
"""
import ctypes as C
import functools

import numpy as np

U = 2.0 ** -53

TILES_C = (1, 5, 8, 11, 16)
TILES_R = (1, 5, 6, 10, 11, 16, 21, 22, 32, 33)
# name -> (sep, leaves (c, r))
DESIGNS = {
    "widths": (12, tuple((c, 11) for c in range(1, 17))),
    # (the leaf (1, 48) makes the separator chain 48 = 3 x 16 block columns long: boundary segments of exactly 16 rows)
    "tiles": (49, tuple((c, r) for c in TILES_C for r in TILES_R) + ((1, 48),)),
    "fan": (72, tuple((1, 2) for _ in range(65)) + ((3, 65),)),
}
NAMES = tuple(DESIGNS)
LAMBDAS = (0.0, 2.5)
CLASSES = ("dd", "gram")
GRAM_EPS = 1e-8

# environment of the factorisation forms (chol_symbolic.cpp / chol_solver.cpp read them at analyze / create time)
OPTION_SETS = [
    {},
    {"CUGO_TILE32_MAX_TILES": "0"},
    {"CUGO_TILE32_MAX_TILES": "100000"},
    {"CUGO_TWO_PHASE_MIN_TILES": "1", "CUGO_TILE32_MAX_TILES": "0"},
    {"CUGO_LOOKAHEAD": "1"},
    {"CUGO_MIN_SUBTREE_TASKS": "0"},
    {"CUGO_PANEL16": "0"},
    {"CUGO_ASM_FRONTS": "0"},
    {"CUGO_ALIAS_CHAINS": "0"},
    {"CUGO_BW_CHAIN": "0"},
    {"CUGO_EA_LDS": "0"},
    {"CUGO_EA_DIRECT": "0"},
]


def option_id(env):
    return ",".join("%s=%s" % (k[5:], v) for k, v in env.items()) or "default"


# Bounds, measured on the references (tests/test_chol_designed_host.py asserts them on every case and prints the figures).
# The factor 4 is the convention of kernel_ref.py: the device sums in a fixed but different order and accumulates in
# MFMA.
#
# omega of test_host.replay_multifrontal(explicit_w=True), in u, at lambda = 0 / 2.5:
#     dd    widths 3.24 / 2.99   tiles 3.77 / 3.89   fan 2.14 / 2.49
#     gram  widths 7.53 / 2.40   tiles 7.03 / 2.41   fan 1.99 / 2.03     (cond 1.4e9 .. 4.3e9 at lambda = 0)
# (the stock replay, L21 through numpy's LU: 1.1 .. 6.0; numpy.linalg.solve itself: 3.4 .. 8.4 on the well conditioned
# cases and 1e6 .. 3e7 on the Gram class at lambda = 0 — LU is stable normwise, not row by row)
OMEGA_REPLAY_MAX = 7.53
K_X = 4 * OMEGA_REPLAY_MAX   # 30.1

# Selected inverse, per entry in units of u (|A^-1| |L| |L^T| |A^-1|)_ij against the refined inverse, lambda = 0 / 2.5:
#   numpy's unrefined float64 inverse            replay of the device pass (test_covariance_host, W formed explicitly)
#     dd    widths 9.69 / 8.84   fan 10.0 / 9.91       widths 12.2 / 11.8    fan 8.62 / 13.9
#     gram  widths 8.37e5 / 5.53 fan 10.7 / 5.10       widths 0.152 / 11.9   fan 3.86e3 / 7.07
# K_S is the bound as the ratio of numpy's inverse defines it; one case (LU on the Gram class) makes it 3.3e6, which
# no kernel would miss.  The bound that bites is per case: 4 x the ratio of the replay of the device's own pass on that
# case, and no less than 4 x its largest ratio over the cases where it stays of order 10 (a lucky 0.152 is no bound
# for another order of summation).
SINV_NUMPY_MAX = 8.37e5
K_S = 4 * SINV_NUMPY_MAX     # 3.35e6
SINV_REPLAY = {("widths", "dd", 0.0): 12.2, ("widths", "dd", 2.5): 11.8, ("widths", "gram", 0.0): 0.152,
               ("widths", "gram", 2.5): 11.9, ("fan", "dd", 0.0): 8.62, ("fan", "dd", 2.5): 13.9,
               ("fan", "gram", 0.0): 3.86e3, ("fan", "gram", 2.5): 7.07}
SINV_REPLAY_ORDINARY = 13.9
# (On an MI355X the twelve forms of tests/test_chol_shapes.py gave omega <= 8.78 u, on tiles / gram / lambda = 0, and
# selected-inverse ratios up to 0.48 of the per-case bound: 7.5e3 on fan / gram / 0 with CUGO_PANEL16=0, 4.6e3 by
# default; 10 .. 13 on the well conditioned cases.)


def k_s_case(name, cls, lam):
    """the selected-inverse bound of one case: 55.6, and 1.54e4 on (fan, gram, 0)"""
    return 4 * max(SINV_REPLAY[(name, cls, lam)], SINV_REPLAY_ORDINARY)


# ------------------------------------------------------------------ patterns -----------
def clique_pattern(sep, leaves):
    """(rows, cliques): rows[r] the ascending block columns >= r of block row r (upper block CSR, diagonal first);
    cliques the node lists the pattern is the union of, the separator's first.  Separator nodes carry the LAST ids."""
    n_leaf = sum(c for c, _ in leaves)
    n = n_leaf + sep
    s0 = n_leaf
    cliques = [list(range(s0, n))]
    at = 0
    for c, r in leaves:
        assert 0 <= r < sep
        cliques.append(list(range(at, at + c)) + list(range(s0, s0 + r)))
        at += c
    rows = [set([i]) for i in range(n)]
    for q in cliques:
        for i, a in enumerate(q):
            rows[a].update(q[i:])
    return [sorted(r) for r in rows], cliques


def csr(rows):
    rowptr = np.array([0] + list(np.cumsum([len(r) for r in rows])), np.int32)
    colind = np.array([c for r in rows for c in r], np.int32)
    return rowptr, colind


@functools.lru_cache(maxsize=None)
def design(name):
    """(rowptr, colind, cliques) of a design; built once, never modified"""
    sep, leaves = DESIGNS[name]
    rows, cliques = clique_pattern(sep, leaves)
    return csr(rows) + (cliques,)


# ------------------------------------------------------------------ values -----------
def vals_from_dense(A, rowptr, colind):
    """the Hsc blocks (column-major 6x6, upper block CSR) of a dense symmetric matrix"""
    n = len(rowptr) - 1
    vals = np.zeros((len(colind), 36))
    for r in range(n):
        for k in range(rowptr[r], rowptr[r + 1]):
            c = colind[k]
            vals[k] = A[6 * r:6 * r + 6, 6 * c:6 * c + 6].T.reshape(-1)
    return vals


def gram_spd(n, cliques, rng, eps=GRAM_EPS):
    """A = sum_k M_k M_k^T / m_k + eps I over the cliques, M_k of m_k x floor(m_k / 2) standard normals: every clique
    is rank deficient on its own, the matrix is positive definite only through the overlaps and eps — the
    conditioning of real Schur complements (cond ~ 1e9, smallest pivot ~ eps)"""
    A = np.zeros((6 * n, 6 * n))
    for q in cliques:
        idx = (6 * np.repeat(q, 6) + np.tile(np.arange(6), len(q))).astype(int)
        m = len(idx)
        M = rng.normal(size=(m, m // 2))
        A[np.ix_(idx, idx)] += M @ M.T / m
    A = 0.5 * (A + A.T)
    return A + eps * np.eye(6 * n)


@functools.lru_cache(maxsize=None)
def values(name, cls, seed=11):
    """(A [6n, 6n], vals [B, 36], b [6n]) of a design in value class "dd" (test_host.random_spd_bsr: strongly
    diagonally dominant) or "gram"; built once, never modified: copy before changing anything"""
    from test_host import random_spd_bsr
    rowptr, colind, cliques = design(name)
    rng = np.random.default_rng(seed)
    if cls == "dd":
        A, vals = random_spd_bsr(rowptr, colind, rng)
    elif cls == "gram":
        A = gram_spd(len(rowptr) - 1, cliques, rng)
        vals = vals_from_dense(A, rowptr, colind)
    else:
        raise KeyError(cls)
    b = rng.normal(size=A.shape[0])
    for a in (A, vals, b):
        a.setflags(write=False)
    return A, vals, b


# ------------------------------------------------------------------ metrics -----------
def omega(A, lam, b, x, L=None):
    """componentwise backward error of x as a solution of (A + lam I) x = b through a Cholesky factorisation, in units
    of u = 2^-53:  max_i |b - (A + lam I) x|_i / (|L| |L^T| |x| + |b|)_i  with the residual in np.longdouble and L
    from numpy in float64 (it only scales the bound; pass |L| if it is at hand).  It does not grow with the condition
    number.  A NaN in x gives inf."""
    if not np.isfinite(x).all():
        return np.inf
    n = A.shape[0]
    Al = A + lam * np.eye(n)
    if L is None:
        L = np.abs(np.linalg.cholesky(Al))
    r = np.asarray(b, np.longdouble) - exact_matmul(Al, np.asarray(x, np.float64).reshape(n, 1))[:, 0]
    den = L @ (L.T @ np.abs(x)) + np.abs(b)
    return float(np.max(np.abs(r).astype(np.float64) / den) / U)


@functools.lru_cache(maxsize=None)
def _abs_chol(name, cls, lam):
    A, _, _ = values(name, cls)
    return np.abs(np.linalg.cholesky(A + lam * np.eye(A.shape[0])))


def case_omega(name, cls, lam, x):
    """omega of x on a designed case (the Cholesky factor that scales it is computed once per case)"""
    A, _, b = values(name, cls)
    return omega(A, lam, b, x, L=_abs_chol(name, cls, lam))


def _split(M, axis, bits, pieces):
    """M = sum of `pieces` float64 matrices plus a remainder below 2^(-pieces (bits + 1)) of the largest entry along
    `axis`; every entry of a piece is an integer of at most bits + 1 bits times a power of two common to its row (axis
    1) or column (axis 0)"""
    M = M.copy()
    out = []
    for _ in range(pieces):
        mx = np.abs(M).max(axis=axis, keepdims=True)
        e = np.ceil(np.log2(np.where(mx > 0, mx, 1.0)))
        sigma = 1.5 * 2.0 ** (e - bits + 52)  # (doubles around sigma are 2^(e - bits) apart)
        P = (M + sigma) - sigma
        out.append(P)
        M = M - P
    return out


def exact_matmul(A, X, pieces=4):
    """A @ X to np.longdouble accuracy out of float64 matrix products (the splitting of Ozaki et al.): both factors
    are cut into slices of `bits` bits (21 for n = 888, 20 for n = 2760), so that every partial sum of a product of two
    slices is an integer below 2^53 times a power of two (n (2^bits + 1)^2 < 2^53) and the float64 product is exact
    whatever its order of summation; the products are then added in np.longdouble, smallest first.  What is cut off
    lies below 2^-84 of the row maxima of A times the column maxima of X.  (numpy's own longdouble product takes 30 times as long.)"""
    bits = (52 - int(np.ceil(np.log2(A.shape[1])))) // 2
    assert A.shape[1] * (2.0 ** bits + 1) ** 2 < 2.0 ** 53
    As, Xs = _split(np.asarray(A, np.float64), 1, bits, pieces), _split(np.asarray(X, np.float64), 0, bits, pieces)
    prods = [(p + q, As[p] @ Xs[q]) for p in range(pieces) for q in range(pieces) if p + q < pieces]
    acc = np.zeros((A.shape[0], X.shape[1]), np.longdouble)
    for _, P in sorted(prods, key=lambda t: -t[0]):
        acc += P
    return acc


def refined_inverse(Al):
    """numpy's float64 inverse X0 and X1 = X0 (2 I - Al X0), one Newton-Schulz step with the residual R = I - Al X0 in
    np.longdouble (the correction X0 R is O(cond u) small: float64 carries it).  On the worst case here (widths, Gram
    class, lambda = 0: |R| ~ 5e-8) a second step moves no entry by more than 0.03 of its bound u (|X| |L| |L^T| |X|)."""
    n = Al.shape[0]
    X0 = np.linalg.inv(Al)
    R = (np.eye(n, dtype=np.longdouble) - exact_matmul(Al, X0)).astype(np.float64)
    X1 = X0.astype(np.longdouble) + X0 @ R
    return X0, X1


@functools.lru_cache(maxsize=None)
def inverse_reference(name, cls, lam):
    """(numpy's inverse X0, the refined inverse X1 in np.longdouble, the per-entry scale u (|X1| |L| |L^T| |X1|)) of a
    design's A + lam I; computed once per case"""
    A, _, _ = values(name, cls)
    Al = A + lam * np.eye(A.shape[0])
    X0, X1 = refined_inverse(Al)
    L = np.abs(np.linalg.cholesky(Al))
    aX = np.abs(X1).astype(np.float64)
    scale = U * (aX @ L @ L.T @ aX)
    return X0, X1, scale


def sinv_ratio(X, X1, scale, mask=None):
    """largest |X - X1|_ij / (u (|A^-1| |L| |L^T| |A^-1|)_ij), over the entries of `mask` if given"""
    q = np.abs(np.asarray(X, np.longdouble) - X1).astype(np.float64) / scale
    return float(q.max() if mask is None else q[mask].max())


def blocks_to_dense(blocks, rowptr, colind):
    """the [B, 36] column-major blocks of an upper block CSR as a dense symmetric matrix (zero off the pattern)"""
    n = len(rowptr) - 1
    X = np.zeros((6 * n, 6 * n))
    for r in range(n):
        for k in range(rowptr[r], rowptr[r + 1]):
            c = colind[k]
            B = blocks[k].reshape(6, 6).T
            X[6 * r:6 * r + 6, 6 * c:6 * c + 6] = B
            if c != r:
                X[6 * c:6 * c + 6, 6 * r:6 * r + 6] = B.T
    return X


def block_mask(rowptr, colind):
    """the scalar entries the pattern covers (both triangles)"""
    return blocks_to_dense(np.ones((len(colind), 36)), rowptr, colind) != 0


# ------------------------------------------------------------------ plan -----------
def analyze(lib, rowptr, colind, ctx=None):
    s = C.c_void_p()
    assert lib.cugo_chol_create(ctx, C.byref(s)) == 0
    rc = lib.cugo_chol_analyze(s, len(rowptr) - 1, rowptr.ctypes.data_as(C.POINTER(C.c_int32)),
                               colind.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0, lib.cugo_last_error()
    return s


def plan32(lib, s, name):
    p = C.POINTER(C.c_int32)()
    n = lib.cugo_chol_plan_array(s, name.encode(), C.byref(p))
    assert n >= 0, name
    return np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, np.int32)


def plan(lib, s):
    """test_host.plan_arrays plus what the census needs"""
    from test_host import plan_arrays
    pl = plan_arrays(lib, s)
    for nm in ("stage_tile", "bc_seg_ptr", "bc_seg"):
        pl[nm] = plan32(lib, s, nm)
    return pl


def census(pl):
    """what a plan holds of the quantities the kernels branch on"""
    ncb, bnd = pl["ncb"], pl["nb"] - pl["ncb"]
    nch = np.diff(pl["child_ptr"])
    seg = pl["bc_seg"].reshape(-1, 3)
    nseg = np.diff(pl["bc_seg_ptr"])
    child_bnd = [int(bnd[c]) for c in pl["child"]]
    seg16 = [f for f in range(len(ncb)) if nseg[f] >= 3 and
             (seg[pl["bc_seg_ptr"][f]:pl["bc_seg_ptr"][f + 1], 2] == 16).any()]
    return dict(ncb=set(int(v) for v in ncb), bnd=set(int(v) for v in bnd),
                pairs=set((int(a), int(b)) for a, b in zip(ncb, bnd)),
                max_children=int(nch.max()), max_child_bnd=max(child_bnd, default=0),
                seg3_with_16=len(seg16), tiles=set(int(t) for t in pl["stage_tile"]))


def front_of(pl, ncb, bnd):
    """the first front of pivot width ncb and boundary bnd (block columns / rows)"""
    hit = np.flatnonzero((pl["ncb"] == ncb) & (pl["nb"] - pl["ncb"] == bnd))
    assert len(hit), (ncb, bnd)
    return int(hit[0])


def scalar_perm(pl):
    """scalar index of the permuted system: (P A P^T)[i, j] = A[sidx[i], sidx[j]]"""
    n = len(pl["perm"])
    return (6 * np.repeat(pl["perm"], 6) + np.tile(np.arange(6), n)).astype(int)
