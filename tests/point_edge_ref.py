"""Extended-precision reference of the point-to-point pose edges with 3 x 3 information (point_kernels.hip) with PER-ENTRY
error bounds, in the manner of tests/pose_edge_ref.py (numpy, test only), and a float64 replay of the device's chunk
order with mutation hooks.

Written from the formulas in the header comment of point_kernels.hip, in np.longdouble, vectorised over the edges.  A
set is a dict pose [E] (ascending), p [E,3], z [E,3], info6 [E,6] or [1,6] (the upper triangle of Omega, row-major packed
00 01 02 11 12 22: the array the device is given, so Omega is exactly symmetric), active [E] bool, rk (type, delta).

value, mass, n as kernel_ref defines them
-----------------------------------------
mass = the same formula with every factor replaced by its cancellation-free absolute value (a difference a - b counts
|a| + |b|; Omega enters as |Omega_ij|, so a matrix of condition 1e6 whose products cancel is covered by its mass),
n = the number of edges summed into the entry; a double evaluation in any order, with or without FMA, lies within
(n + c) u mass.  c counts the roundings on the longest path of one term, in the operation order of point_edge():
    y_i = sum_j R_ij p_j + t_i           as pose_edge_ref (R_ij 4, product 1, 3 additions)        ->  8   (mass ay)
    r = y - z                            8, the subtraction                                        ->  9   (mass ar = ay + |z|)
    q = Omega r                          9, product 1, 2 additions                                 -> 12
    x = max(0, r.q)                      12 + 9, product 1, 2 additions (max is 1-Lipschitz)       -> 24
    chi += rho(x)                        24, rho 6, 2 spare                                        -> 32
    w = rho'(x)                          24 + 5 (as kernel_ref's 2 c_r + 5)                        -> 29   (mass aw)
    G = Omega S, S = -[y]x               8, product 1, the subtraction (two non-zero terms)        -> 10
    H_ww = w S^T G                       8 + 10, product 1, the subtraction; 29, product 1         -> 50
    H_wv = w G^T                         29 + 10 + 1                                               -> 40
    H_vv = w Omega                       29 + 1                                                    -> 30
    b_w = -w (y x q)                     8 + 12, product 1, the subtraction; 29, product 1         -> 52
    b_v = -w q                           29 + 12 + 1                                               -> 42
so C_POINT = H 50, b 52, chi 32 (the largest of each output).  The masses: rb = |r| + ar wherever r enters a product;
xmass = rb^T |Omega| rb; aw = rho' + |rho''| xmass; the mass of a chi2 term is |rho| + xmass + rho0 (pose_edge_ref._rho0);
H mass = aw aJ^T |Omega| aJ and b mass = aw aJ^T |Omega| rb with aJ = [ |[ay]x| | I ].

The two equivalences (Omega = omega n n^T with n.z = d is the plane edge; Omega = omega (I - u u^T) with z = a the line
edge) are held to the SUM of this reference's bound and pose_edge_ref's.  The converted data (plane_as_point,
line_as_point) is formed in longdouble and rounded once per number, so the point edge is the plane / line edge up to
one rounding of each Omega_ij and of z; each perturbs an entry by at most u times a product of the factors its mass
holds, i.e. by a few of the (n + c) units of the two bounds, whose sum has c = 50 + 51 and more.
"""
import numpy as np

from kernel_ref import LD, U, bound, ratio, _rho, _scatter  # noqa: F401 (re-exported for the tests)
from pose_edge_ref import ICP_CHUNK, _rho0, _rot, _skew_neg, chi_total

C_POINT = dict(H=50, b=52, chi=32)
TERM_MUTATIONS = ("col_packed", "no_offdiag", "skew_sign", "p_for_y", "r_flipped", "w_twice", "chi_no_info", "shared_per_edge")
ORDER_MUTATIONS = ("drop_chunk_last", "drop_second_chunk")


def unpack(info6):
    """[E,6] packed upper triangles -> [E,3,3] symmetric matrices"""
    a = np.asarray(info6)
    M = np.empty((len(a), 3, 3), a.dtype)
    for k, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        M[:, i, j] = M[:, j, i] = a[:, k]
    return M


def pack(Om):
    """[E,3,3] -> [E,6]: the upper triangle, row-major packed"""
    Om = np.asarray(Om)
    return np.stack([Om[:, 0, 0], Om[:, 0, 1], Om[:, 0, 2], Om[:, 1, 1], Om[:, 1, 2], Om[:, 2, 2]], 1)


def point_terms(poses, n_free, e, dtype=LD, full=True, mut=None, w_scale=None):
    """per-edge terms: dict H [E,6,6], b [E,6], chi [E] with X_mass each; edges that do not count are zero.  mut: one of
    TERM_MUTATIONS (what a wrong kernel would compute); w_scale: a factor on the weight (the sensitivity test)"""
    dt = dtype
    pose = np.asarray(e["pose"], int)
    E = len(pose)
    P7 = np.asarray(poses, dt)[pose]
    R, aR = _rot(P7[:, :4])
    p, z, t = np.asarray(e["p"], dt).reshape(E, 3), np.asarray(e["z"], dt).reshape(E, 3), P7[:, 4:]
    y = np.einsum("eij,ej->ei", R, p) + t
    ay = np.einsum("eij,ej->ei", aR, np.abs(p)) + np.abs(t)
    info6 = np.asarray(e["info6"], dt).reshape(-1, 6)
    if mut == "shared_per_edge" and len(info6) == 1:      # [6][1] indexed k + e instead of k: edge e reads from element e on
        flat = np.concatenate([info6[0], np.zeros(E + 6, dt)])
        info6 = np.stack([flat[k:k + 6] for k in range(E)]) if E else info6
    info6 = np.broadcast_to(info6, (E, 6))
    if mut == "col_packed":                               # the triangle read column-packed: 02 and 11 change places
        info6 = info6[:, [0, 1, 3, 2, 4, 5]]
    Om = unpack(info6)
    if mut == "no_offdiag":
        Om = Om * np.eye(3, dtype=dt)[None]
    aOm = np.abs(unpack(np.broadcast_to(np.asarray(e["info6"], dt).reshape(-1, 6), (E, 6))))
    r = y - z
    ar = ay + np.abs(z)
    if mut == "r_flipped":
        r = -r
    S = _skew_neg(p if mut == "p_for_y" else y)
    if mut == "skew_sign":
        S = -S
    aS = np.abs(_skew_neg(ay))
    I3 = np.broadcast_to(np.eye(3, dtype=dt), (E, 3, 3))
    J, aJ = np.concatenate([S, I3], 2), np.concatenate([aS, I3], 2)
    q = np.einsum("eij,ej->ei", Om, r)
    x = np.maximum(0, (r * q).sum(1))
    rb = np.abs(r) + ar
    xmass = np.einsum("ei,eij,ej->e", rb, aOm, rb)
    kind, delta = int(e["rk"][0]), e["rk"][1]
    rho, drho, d2rho = _rho(kind, delta, x, dt)
    if mut == "chi_no_info":
        rho = _rho(kind, delta, (r * r).sum(1), dt)[0]
    live = ((pose < n_free) & np.asarray(e["active"], bool)).astype(dt)
    out = dict(chi=live * rho, chi_mass=live * (np.abs(rho) + xmass + _rho0(kind, delta, x, dt)), live=live > 0, x=x)
    if full:
        w = live * drho
        if mut == "w_twice":
            w = w * drho
        if w_scale is not None:
            w = w * dt(w_scale)
        aw = live * (drho + d2rho * xmass)
        out.update(H=w[:, None, None] * np.einsum("eka,ekl,elc->eac", J, Om, J),
                   H_mass=aw[:, None, None] * np.einsum("eka,ekl,elc->eac", aJ, aOm, aJ),
                   b=-(w[:, None] * np.einsum("eka,ek->ea", J, q)), b_mass=aw[:, None] * np.einsum("eka,ekl,el->ea", aJ, aOm, rb), w=w)
    return out


def point_build(poses, n_free, e, dtype=LD, full=True, mut=None):
    """H [P,6,6], b [P,6], chi_pose [P] (P = n_free), chi_edge [E], chi, each with X_mass and X_n"""
    dt = dtype
    P = n_free
    t = point_terms(poses, n_free, e, dt, full, mut)
    live = t["live"]
    q = np.asarray(e["pose"], int)[live]
    cnt = np.bincount(q, minlength=P)[:P] if P else np.zeros(0, np.int64)
    out = {}
    for k, shp in (("H", (P, 6, 6)), ("b", (P, 6))):
        out[k], out[k + "_mass"] = np.zeros(shp, dt), np.zeros(shp, dt)
    for k in (("H", "b") if full else ()) + ("chi",):
        ko = "chi_pose" if k == "chi" else k
        out[ko] = _scatter(q, t[k][live], P)
        out[ko + "_mass"] = _scatter(q, t[k + "_mass"][live], P)
    out["chi_edge"], out["chi_edge_mass"], out["chi_edge_n"] = t["chi"], t["chi_mass"], 0
    out["chi"], out["chi_mass"], out["chi_n"] = t["chi"].sum(), t["chi_mass"].sum(), int(cnt.sum())
    out["H_n"], out["b_n"], out["chi_pose_n"] = cnt[:, None, None], cnt[:, None], cnt
    return out


def point_bound(ref, key):
    return bound(ref[key + "_n"], C_POINT["chi" if key.startswith("chi") else key], ref[key + "_mass"])


def point_replay(poses, n_free, n_poses_total, e, mut=None):
    """float64 evaluation in the order of point_kernels.hip: chunks of 512 edges in groups of 64 lanes, the lanes of one
    pose summed into the wave's accumulators, a partial flushed to slot chunk + pose whenever the pose changes and at the
    chunk's end, one chi2 total per chunk; the finishing pass sums slots c + p in chunk order and mirrors the upper
    triangle; the totals by pose_edge_ref.chi_total.  mut: None, one of TERM_MUTATIONS (the per-edge terms), or
    'drop_chunk_last' (the last edge of every full chunk is lost), 'drop_second_chunk' (the finishing sum skips the second
    chunk of a pose).  Returns H [P,6,6], b [P,6], chi, chi_edge, chi per pose"""
    P = n_free
    iu = np.triu_indices(6)
    pose = np.asarray(e["pose"], int)
    n = len(pose)
    t = point_terms(poses, n_free, e, np.float64, mut=mut if mut in TERM_MUTATIONS else None)
    v = np.concatenate([t["H"][:, iu[0], iu[1]], t["b"], t["chi"][:, None]], 1) if n else np.zeros((0, 28))
    chi_edge = t["chi"].copy()
    if mut == "drop_chunk_last" and n >= ICP_CHUNK:
        v[np.arange(ICP_CHUNK - 1, n, ICP_CHUNK)] = 0.0
    nc = (n + ICP_CHUNK - 1) // ICP_CHUNK
    part = np.zeros((nc + n_poses_total + 1, 28))
    idx = np.arange(n)
    key_change = np.flatnonzero((np.diff(idx // 64) != 0) | (np.diff(pose) != 0)) + 1 if n > 1 else np.zeros(0, int)
    starts = np.concatenate([[0], key_change]).astype(int) if n else np.zeros(0, int)
    seg = np.add.reduceat(v, starts, axis=0) if n else np.zeros((0, 28))
    cchi = np.zeros(nc)
    acc, cur = np.zeros(28), None          # cur = (chunk, pose)
    for k in range(len(starts)):
        s0 = starts[k]
        c, q = s0 // ICP_CHUNK, pose[s0]
        if cur is not None and cur != (c, q):
            part[cur[0] + cur[1]] = acc
            cchi[cur[0]] += acc[27]
            acc = np.zeros(28)
        cur = (c, q)
        acc = acc + seg[k]
    if cur is not None:
        part[cur[0] + cur[1]] = acc
        cchi[cur[0]] += acc[27]
    sums = np.zeros((P, 28))
    ptr = np.searchsorted(pose, np.arange(n_poses_total + 1))
    for p in range(P):
        i0, i1 = ptr[p], ptr[p + 1]
        if i1 > i0:
            c0, c1 = i0 // ICP_CHUNK, (i1 - 1) // ICP_CHUNK
            for c in range(c0, c1 + 1):
                if not (mut == "drop_second_chunk" and c == c0 + 1):
                    sums[p] = sums[p] + part[c + p]
    H, b = np.zeros((P, 6, 6)), np.zeros((P, 6))
    H[:, iu[0], iu[1]] = sums[:, :21]
    H[:, iu[1], iu[0]] = sums[:, :21]
    b[:] = sums[:, 21:27]
    return H, b, chi_total(cchi), chi_edge, sums[:, 27].copy()


# ------------------------------------------------------------------ the two equivalences
def plane_as_point(e):
    """the plane kind `e` of pose_designed (n, d, omega) as point edges: Omega = omega n n^T, z = d n / (n.n) (n.z = d), each
    number formed in longdouble and rounded once"""
    n, d = np.asarray(e["n"], LD), np.asarray(e["d"], LD)
    om = np.broadcast_to(np.asarray(e["omega"], LD), (len(n),))
    Om = om[:, None, None] * n[:, :, None] * n[:, None, :]
    z = d[:, None] * n / (n * n).sum(1)[:, None]
    return dict(pose=e["pose"], p=e["p"], z=z.astype(np.float64), info6=pack(Om).astype(np.float64), active=e["active"],
                flags=e.get("flags"), rk=e["rk"])


def line_as_point(e):
    """the line kind `e` (a, u, omega) as point edges: Omega = omega (I - u u^T) rounded once per entry, z = a"""
    u = np.asarray(e["u"], LD)
    om = np.broadcast_to(np.asarray(e["omega"], LD), (len(u),))
    Om = om[:, None, None] * (np.eye(3, dtype=LD)[None] - u[:, :, None] * u[:, None, :])
    return dict(pose=e["pose"], p=e["p"], z=np.asarray(e["a"], np.float64), info6=pack(Om).astype(np.float64),
                active=e["active"], flags=e.get("flags"), rk=e["rk"])
