"""Extended-precision reference of the pose-pose point edges (point_pair_kernels.hip) with PER-ENTRY error bounds, in the
manner of tests/point_edge_ref.py (numpy, test only), a numpy restatement of the host plan (point_pair_plan.h) and a
float64 replay of the device's run / chunk / role order with mutation hooks.

Written from the term in include/cugo_hip.h (cugo_point_pair_edges), in np.longdouble, vectorised over the edges.  A set
is a dict a [E], b [E] (pose indices, the caller's order), p [E,3] (the point in a's frame), z [E,3] (its measurement in
b's frame), info6 [E,6] or [1,6] (the upper triangle of Omega, row-major packed 00 01 02 11 12 22: the array the device is
given, so Omega is exactly symmetric), active [E] bool, rk (type, delta).
    X = R_a^T (p - t_a),  y = R_b X + t_b,  r = y - z,  x = max(0, r^T Omega r),  chi2 term rho(x),  w = rho'(x)
    J_b = [ -[y]x | I ],  J_a = M [ [p]x | -I ],  M = R_b R_a^T
    H_aa = w J_a^T Omega J_a,  H_bb = w J_b^T Omega J_b,  H_ab = w J_a^T Omega J_b,  b_a = -w J_a^T Omega r,  b_b = -w J_b^T Omega r
The reference forms J_a and J_b as written and multiplies out; the kernel goes through N = M^T Omega and Omega' = N M.

value, mass, n as kernel_ref defines them
-----------------------------------------
mass = the same formula with every factor replaced by its cancellation-free absolute value, n = the number of edges
summed into the entry; a double evaluation in any order, with or without FMA, lies within (n + c) u mass.  c counts the
roundings on the longest path of one term, in the operation order of pair_edge() (an entry R_ij costs 4, a product 1
more than its factors together, a sum of k terms k - 1 more than its worst term):
    d = p - t_a                          1
    X_i = sum_j Ra_ji d_j                4 + 1, product 1, 2 additions                              ->  8
    y_i = sum_j Rb_ij X_j + tb_i         4 + 8, product 1, 3 additions                              -> 16   (mass ay)
    r = y - z                            16, the subtraction                                        -> 17   (mass ar = ay + |z|)
    q = Omega r                          17, product 1, 2 additions                                 -> 20
    x = max(0, r.q)                      17 + 20, product 1, 2 additions                            -> 40
    chi += rho(x)                        40, rho 6, 2 spare                                         -> 48
    w = rho'(x)                          40 + 5                                                     -> 45
  self-b (the unary point term at y):
    G = Omega S_y                        16, product 1, the subtraction                             -> 18
    H_bb ww = w S_y^T G                  16 + 18, product 1, the subtraction; 45, product 1         -> 82
    b_b w = -w (y x q)                   16 + 20, product 1, the subtraction; 45, product 1         -> 84
  self-a (the unary point term at p, which is exact, with Omega' = N M):
    M_ij = sum_k Rb_ik Ra_jk             4 + 4, product 1, 2 additions                              -> 11
    N = M^T Omega                        11, product 1, 2 additions                                 -> 14
    Omega' = N M                         14 + 11, product 1, 2 additions                            -> 28
    G' = Omega' S_p                      28, product 1, the subtraction                             -> 30
    H_aa ww = w S_p^T G'                 30, product 1, the subtraction; 45, product 1              -> 78
    q' = M^T q                           11 + 20, product 1, 2 additions                            -> 34
    b_a w = w (p x q')                   34, product 1, the subtraction; 45, product 1              -> 82
  off-diagonal, the longest path J_a = M [[p]x | -I] against J_b:
    W = N S_y                            14 + 16, product 1, the subtraction                        -> 32
    H_ab ww = -w [p]x W                  32, product 1, the subtraction; 45, product 1              -> 80
so C_PAIR = H 82 (a diagonal block sums terms of both sides), Hoff 80, b 84, chi 48.  The masses: rb = |r| + ar wherever r
enters a product; xmass = rb^T |Omega| rb; aw = rho' + |rho''| xmass; the mass of a chi2 term is |rho| + xmass + rho0
(pose_edge_ref._rho0); aJ_b = [ |[ay]x| | I ], aJ_a = aM [ |[p]x| | I ] with aM = aRb aRa^T; H mass = aw aJ^T |Omega| aJ
and b mass = aw aJ^T |Omega| rb.
"""
import numpy as np

from kernel_ref import LD, U, bound, ratio, _rho, _scatter  # noqa: F401 (re-exported for the tests)
from point_edge_ref import pack, unpack  # noqa: F401
from pose_edge_ref import ICP_CHUNK, _rho0, _rot, _skew_neg, chi_total

C_PAIR = dict(H=82, Hoff=80, b=84, chi=48)
TERM_MUTATIONS = ("skew_sign", "R_AB")
ORDER_MUTATIONS = ("drop_chunk_last", "drop_second_chunk", "no_transpose", "fixed_a_adds", "side_swapped", "second_run_overwrites")
RUN_A_FREE, RUN_B_FREE, RUN_A_IS_HI, RUN_COUNTS = 1, 2, 4, 8
INACTIVE = 8


# ------------------------------------------------------------------ the host plan, brute force
def numpy_plan(a, b, active, n_free, rowptr=None, colind=None):
    """what build_point_pair_plan produces, as a dict of int arrays under the names of cugo_point_pair_plan_array"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    active = np.ones(len(a), bool) if active is None else np.asarray(active, bool)
    P = n_free
    lo, hi, ori = np.minimum(a, b), np.maximum(a, b), (a > b).astype(np.int64)
    perm = np.lexsort((np.arange(len(a)), ori, hi, lo))
    sa, sb = a[perm], b[perm]
    new = np.ones(len(a), bool)
    new[1:] = (sa[1:] != sa[:-1]) | (sb[1:] != sb[:-1])
    edge_run = np.cumsum(new) - 1
    starts = np.flatnonzero(new)
    run_a, run_b = sa[starts], sb[starts]
    R = len(starts)
    run_ptr = np.concatenate([starts, [len(a)]])
    counts_e = active[perm] & ((sa < P) | (sb < P))
    run_counts = np.zeros(R, bool)
    np.logical_or.at(run_counts, edge_run, counts_e)
    run_flags = (run_a < P) * RUN_A_FREE + (run_b < P) * RUN_B_FREE + (run_a > run_b) * RUN_A_IS_HI + run_counts * RUN_COUNTS
    run_blk = np.full(R, -1)
    inc = [[] for _ in range(P)]
    blocks = {}
    for r in range(R):
        if not run_counts[r]:
            continue
        if run_a[r] < P:
            inc[run_a[r]].append(2 * r)
        if run_b[r] < P:
            inc[run_b[r]].append(2 * r + 1)
        if run_a[r] < P and run_b[r] < P:
            blocks.setdefault((min(run_a[r], run_b[r]), max(run_a[r], run_b[r])), []).append(r)
    pairs = sorted(blocks)
    blk_id, blk_ptr, blk_run = [], [0], []
    for (l, h) in pairs:
        if rowptr is not None:
            row = np.asarray(colind[rowptr[l]:rowptr[l + 1]])
            k = int(np.searchsorted(row, h))
            assert k < len(row) and row[k] == h, "pair (%d, %d) is missing from the pattern" % (l, h)
            for r in blocks[(l, h)]:
                run_blk[r] = rowptr[l] + k
            blk_id.append(rowptr[l] + k)
            blk_run += blocks[(l, h)]
            blk_ptr.append(len(blk_run))
    i32 = lambda x: np.asarray(x, np.int32).reshape(-1)
    return dict(perm=i32(perm), edge_run=i32(edge_run), run_ptr=i32(run_ptr), run_a=i32(run_a), run_b=i32(run_b),
                run_flags=i32(run_flags), run_blk=i32(run_blk), inc_ptr=i32(np.concatenate([[0], np.cumsum([len(x) for x in inc])])),
                inc=i32([x for l in inc for x in l]), blk_id=i32(blk_id), blk_ptr=i32(blk_ptr), blk_run=i32(blk_run),
                pair_lo=i32([p[0] for p in pairs]), pair_hi=i32([p[1] for p in pairs]))


def pair_pattern(n_free, pair_lo, pair_hi, extra=()):
    """upper block CSR (rowptr, colind) over the free poses holding the diagonal, the pairs and `extra` (lo, hi) blocks"""
    rows = [{p} for p in range(n_free)]
    for l, h in list(zip(pair_lo, pair_hi)) + list(extra):
        rows[int(l)].add(int(h))
    colind = [c for r in rows for c in sorted(r)]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    return rowptr.astype(np.int32), np.asarray(colind, np.int32)


# ------------------------------------------------------------------ the term
def _skew(p):
    return -_skew_neg(p)


def pair_terms(poses, n_free, e, dtype=LD, mut=None, w_scale=None):
    """per-edge terms in the caller's order: Haa, Hbb, Hab [E,6,6] (Hab: rows a, columns b), ba, bb [E,6], chi [E], each
    with X_mass; the terms of a fixed end and of edges that do not count are zero.  mut: one of TERM_MUTATIONS"""
    dt = dtype
    a, b = np.asarray(e["a"], int), np.asarray(e["b"], int)
    E = len(a)
    Pa, Pb = np.asarray(poses, dt)[a], np.asarray(poses, dt)[b]
    Ra, aRa = _rot(Pa[:, :4])
    Rb, aRb = _rot(Pb[:, :4])
    p, z = np.asarray(e["p"], dt).reshape(E, 3), np.asarray(e["z"], dt).reshape(E, 3)
    ta, tb = Pa[:, 4:], Pb[:, 4:]
    X = np.einsum("eji,ej->ei", Ra, p - ta)
    aX = np.einsum("eji,ej->ei", aRa, np.abs(p) + np.abs(ta))
    y = np.einsum("eij,ej->ei", Rb, X) + tb
    ay = np.einsum("eij,ej->ei", aRb, aX) + np.abs(tb)
    M = np.einsum("eik,ejk->eij", Rb, Ra)
    aM = np.einsum("eik,ejk->eij", aRb, aRa)
    if mut == "R_AB":
        M = M.transpose(0, 2, 1)
    info6 = np.broadcast_to(np.asarray(e["info6"], dt).reshape(-1, 6), (E, 6))
    Om, aOm = unpack(info6), np.abs(unpack(info6))
    r = y - z
    ar = ay + np.abs(z)
    I3 = np.broadcast_to(np.eye(3, dtype=dt), (E, 3, 3))
    Jb, aJb = np.concatenate([_skew_neg(y), I3], 2), np.concatenate([np.abs(_skew_neg(ay)), I3], 2)
    Sp = _skew(p)
    if mut == "skew_sign":
        Sp = -Sp
    Ja = np.einsum("eij,ejk->eik", M, np.concatenate([Sp, -I3], 2))
    aJa = np.einsum("eij,ejk->eik", aM, np.concatenate([np.abs(Sp), I3], 2))
    q = np.einsum("eij,ej->ei", Om, r)
    x = np.maximum(0, (r * q).sum(1))
    rb = np.abs(r) + ar
    xmass = np.einsum("ei,eij,ej->e", rb, aOm, rb)
    kind, delta = int(e["rk"][0]), e["rk"][1]
    rho, drho, d2rho = _rho(kind, delta, x, dt)
    fa, fb = a < n_free, b < n_free
    live = ((fa | fb) & np.asarray(e["active"], bool))
    lv = live.astype(dt)
    w = lv * drho
    if w_scale is not None:
        w = w * dt(w_scale)
    aw = lv * (drho + d2rho * xmass)
    wa, wb, wab = w * fa, w * fb, w * (fa & fb)
    awa, awb, awab = aw * fa, aw * fb, aw * (fa & fb)
    H = lambda ww, J1, J2: ww[:, None, None] * np.einsum("eka,ekl,elc->eac", J1, Om, J2)
    Hm = lambda ww, J1, J2: ww[:, None, None] * np.einsum("eka,ekl,elc->eac", J1, aOm, J2)
    return dict(chi=lv * rho, chi_mass=lv * (np.abs(rho) + xmass + _rho0(kind, delta, x, dt)), live=live, x=x,
                Haa=H(wa, Ja, Ja), Haa_mass=Hm(awa, aJa, aJa), Hbb=H(wb, Jb, Jb), Hbb_mass=Hm(awb, aJb, aJb),
                Hab=H(wab, Ja, Jb), Hab_mass=Hm(awab, aJa, aJb),
                ba=-(wa[:, None] * np.einsum("eka,ek->ea", Ja, q)), ba_mass=awa[:, None] * np.einsum("eka,ekl,el->ea", aJa, aOm, rb),
                bb=-(wb[:, None] * np.einsum("eka,ek->ea", Jb, q)), bb_mass=awb[:, None] * np.einsum("eka,ekl,el->ea", aJb, aOm, rb),
                Ja=Ja, Jb=Jb, r=r)


def pair_build(poses, n_free, n_poses_total, e, dtype=LD, mut=None):
    """H [Pall,6,6], b [Pall,6] (the rows of fixed poses are zero with zero mass: they must not be written), Hoff
    [n_pairs,6,6] for the distinct counting free-free pairs (pair_lo, pair_hi ascending; rows: pose lo), chi_edge [E] in
    the caller's order, chi; each with X_mass and X_n"""
    Pall = n_poses_total
    t = pair_terms(poses, n_free, e, dtype, mut)
    a, b = np.asarray(e["a"], int), np.asarray(e["b"], int)
    live = t["live"]
    out = {}
    for k in ("H", "b"):
        for suf in ("", "_mass"):
            out[k + suf] = _scatter(a, t[k + "aa" + suf if k == "H" else k + "a" + suf], Pall) + \
                _scatter(b, t[k + "bb" + suf if k == "H" else k + "b" + suf], Pall)
    cnt = np.bincount(a[live], minlength=Pall)[:Pall] + np.bincount(b[live], minlength=Pall)[:Pall]
    cnt[n_free:] = 0
    out["H_n"], out["b_n"] = cnt[:, None, None], cnt[:, None]
    ff = live & (a < n_free) & (b < n_free)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = lo * Pall + hi
    pairs = np.unique(key[ff])
    out["pair_lo"], out["pair_hi"] = pairs // Pall, pairs % Pall
    idx = np.searchsorted(pairs, key[ff])
    tr = (a > b)[ff]
    for suf in ("", "_mass"):
        blk = np.where(tr[:, None, None], t["Hab" + suf][ff].transpose(0, 2, 1), t["Hab" + suf][ff])
        out["Hoff" + suf] = _scatter(idx, blk, len(pairs))
    out["Hoff_n"] = np.bincount(idx, minlength=len(pairs))[:, None, None]
    out["chi_edge"], out["chi_edge_mass"], out["chi_edge_n"] = t["chi"], t["chi_mass"], 0
    out["chi"], out["chi_mass"], out["chi_n"] = t["chi"].sum(), t["chi_mass"].sum(), int(live.sum())
    return out


def pair_bound(ref, key):
    return bound(ref[key + "_n"], C_PAIR["chi" if key.startswith("chi") else key], ref[key + "_mass"])


# ------------------------------------------------------------------ the device's order, in float64
def pair_replay(poses, n_free, n_poses_total, e, mut=None):
    """float64 evaluation in the order of point_pair_kernels.hip: the plan's sort; per role chunks of 512 sorted edges in
    groups of 64 lanes, the lanes of one run summed into the wave's accumulators, a partial flushed to slot chunk + run
    whenever the run changes and at the chunk's end, one chi2 total per chunk; the finishing passes sum a pose's (run,
    side) partials in incidence order then chunk order and mirror the upper triangle, and a block's runs ascending,
    transposing a run whose a is hi.  mut: None, one of TERM_MUTATIONS or of ORDER_MUTATIONS.  Returns H [Pall,6,6], b
    [Pall,6], Hoff [n_pairs,6,6] (the pairs of numpy_plan), chi, chi_edge (the caller's order)"""
    P, Pall = n_free, n_poses_total
    a, b = np.asarray(e["a"], int), np.asarray(e["b"], int)
    n = len(a)
    plan = numpy_plan(a, b, e["active"], P)
    perm, edge_run, flags = plan["perm"], plan["edge_run"], plan["run_flags"]
    t = pair_terms(poses, n_free, e, np.float64, mut=mut if mut in TERM_MUTATIONS else None)
    if mut == "fixed_a_adds":      # role 0 does not look at RUN_A_FREE: the term of a fixed a is formed (and added below)
        t2 = pair_terms(poses, n_poses_total, e, np.float64)
        live = t["live"]
        t["Haa"], t["ba"] = t2["Haa"] * live[:, None, None], t2["ba"] * live[:, None]
    iu = np.triu_indices(6)
    z1 = np.zeros((n, 1))
    cols = lambda c0: t["Hab"][:, :, c0:c0 + 3].transpose(0, 2, 1).reshape(n, 18)   # v[6 c + i] = Hab[i][c0 + c]
    role_v = [np.concatenate([t["Haa"][:, iu[0], iu[1]], t["ba"], t["chi"][:, None]], 1),
              np.concatenate([t["Hbb"][:, iu[0], iu[1]], t["bb"], z1], 1),
              np.concatenate([cols(0), np.zeros((n, 9)), z1], 1), np.concatenate([cols(3), np.zeros((n, 9)), z1], 1)]
    nc = (n + ICP_CHUNK - 1) // ICP_CHUNK
    R = len(plan["run_a"])
    part = np.zeros((4, nc + R + 1, 28))
    cchi = np.zeros(nc)
    idx = np.arange(n)
    key_change = np.flatnonzero((np.diff(idx // 64) != 0) | (np.diff(edge_run) != 0)) + 1 if n > 1 else np.zeros(0, int)
    starts = np.concatenate([[0], key_change]).astype(int) if n else np.zeros(0, int)
    for role in range(4):
        v = role_v[role][perm]
        if mut == "drop_chunk_last" and n >= ICP_CHUNK:
            v[np.arange(ICP_CHUNK - 1, n, ICP_CHUNK)] = 0.0
        seg = np.add.reduceat(v, starts, axis=0) if n else np.zeros((0, 28))
        acc, cur = np.zeros(28), None          # cur = (chunk, run)
        for k in range(len(starts)):
            s0 = starts[k]
            c, r = s0 // ICP_CHUNK, edge_run[s0]
            if cur is not None and cur != (c, r):
                part[role, cur[0] + cur[1]] = acc
                if role == 0:
                    cchi[cur[0]] += acc[27]
                acc = np.zeros(28)
            cur = (c, r)
            acc = acc + seg[k]
        if cur is not None:
            part[role, cur[0] + cur[1]] = acc
            if role == 0:
                cchi[cur[0]] += acc[27]

    def run_sum(role, r):
        i0, i1 = plan["run_ptr"][r], plan["run_ptr"][r + 1]
        c0, c1 = i0 // ICP_CHUNK, (i1 - 1) // ICP_CHUNK
        s = np.zeros(28)
        for c in range(c0, c1 + 1):
            if not (mut == "drop_second_chunk" and c == c0 + 1):
                s = s + part[role, c + r]
        return s

    sums = np.zeros((Pall, 28))
    for p in range(P):
        for j in range(plan["inc_ptr"][p], plan["inc_ptr"][p + 1]):
            rs = plan["inc"][j]
            side = rs & 1
            if mut == "side_swapped" and j == plan["inc_ptr"][p]:
                side ^= 1
            sums[p] = sums[p] + run_sum(side, rs >> 1)
    if mut == "fixed_a_adds":
        for r in range(R):
            if (flags[r] & RUN_COUNTS) and not (flags[r] & RUN_A_FREE):
                sums[plan["run_a"][r]] = sums[plan["run_a"][r]] + run_sum(0, r)
    H, bv = np.zeros((Pall, 6, 6)), np.zeros((Pall, 6))
    H[:, iu[0], iu[1]] = sums[:, :21]
    H[:, iu[1], iu[0]] = sums[:, :21]
    bv[:] = sums[:, 21:27]
    # the off-diagonal blocks: the pairs ascending are the blocks touched, in order
    full = numpy_plan(a, b, e["active"], P, *pair_pattern(P, plan["pair_lo"], plan["pair_hi"]))
    Hoff = np.zeros((len(full["blk_id"]), 6, 6))
    for k in range(len(full["blk_id"])):
        for j in range(full["blk_ptr"][k], full["blk_ptr"][k + 1]):
            r = full["blk_run"][j]
            Hab = np.concatenate([run_sum(2, r)[:18].reshape(3, 6).T, run_sum(3, r)[:18].reshape(3, 6).T], 1)
            blk = Hab.T if (flags[r] & RUN_A_IS_HI) and mut != "no_transpose" else Hab
            if mut == "second_run_overwrites" and j > full["blk_ptr"][k]:
                Hoff[k] = blk
            else:
                Hoff[k] = Hoff[k] + blk
    chi_edge = t["chi"].copy()
    return H, bv, Hoff, chi_total(cchi), chi_edge
