"""Designs for the landmark covariance kernel (cugo_landmark_covariances): flattened layouts with the inputs the kernel
and tests/lm_cov_ref.py are both fed (numpy only, no product code).

Per design: Hll and Hpl from kernel_ref.build at the design's estimates, rounded to double; the pattern from
devmem.hsc_structure; sigma = the pattern blocks of numpy.linalg.inv of the float64 Schur complement of those inputs, symmetrised
(data, fed identically to both sides: its own accuracy is not under test).  The Hpl block of every slot that does not
count (FIXED_P, FIXED_L, INACTIVE, padding) is NaN: a kernel that reads one shows it.

  B         layout B of designed.py: landmark degrees 1, 2, 100, 255, 0, 256, 3, 257, 0, 300, ... (the edgeless free
            landmarks have Hll = 0: they fail)
  B_padded  the same through devmem.pad_to_groups: INACTIVE padding slots with pose index 0
  mixed     fixed and free poses on one landmark, a landmark of fixed poses only, about 15 % INACTIVE slots, a
            landmark with one active edge left, fixed landmarks
  corners   a CSR row with its diagonal block only, a pair at the last column of its row, pose 0 with pose P-1, pose
            P-1 alone
  far       low parallax: mono edges from 2 to 4 cameras within a baseline of about 1, depths 30 to 3000
  grid1, grid256, grid257, grid513   that many free landmarks of low degree
"""
import functools

import numpy as np

import designed
import devmem
import kernel_ref as kr
import lm_cov_ref as lr
import synth

NAMES = ("B", "B_padded", "mixed", "corners", "far", "grid1", "grid256", "grid257", "grid513")
# Layout B was made for the edge passes: its 300 free poses see as few as two landmarks, and the Schur complement of its
# build pass alone is singular (cond 4e19).  Its inverse would be noise with a few blocks of 1e16 that swamp the mass of
# every landmark, and no change to a term of ordinary size could show.  Every free pose of B therefore gets a prior of
# unit information, as a pose prior edge would add to Hpp, before Hsc is inverted.
B_PRIOR = 1.0
MUTATED = ("B", "mixed", "corners")   # the designs whose landmarks of degree >= 2 must show the three changes


def with_inactive(f, slots):
    """a copy of the flattened dict with the INACTIVE bit set on `slots`, pose_ptr / pose_edge rebuilt over the slots
    that are left (designed.check_layout: they list the real edges only)"""
    g = dict(f)
    g["flags"] = f["flags"].copy()
    g["flags"][np.asarray(slots, np.int64)] |= 8
    real = np.flatnonzero((g["flags"] & 8) == 0)
    order = np.lexsort((g["lm"][real], g["pose"][real]))
    g["pose_edge"] = np.concatenate([real[order], np.zeros(g["E"] - len(real), np.int64)]).astype(np.int32)
    pp = np.zeros(g["Pall"] + 1, np.int64)
    np.add.at(pp, g["pose"][real] + 1, 1)
    g["pose_ptr"] = np.cumsum(pp).astype(np.int32)
    return g


def permuted_slots(f, perms):
    """a copy of the flattened dict with the slots of every landmark l of `perms` in the order perms[l] (check_layout
    asks for landmark-major slots, not for ascending pose indices within a landmark); returns (dict, old slot of every
    new one)"""
    src = np.arange(f["E"])
    for l, perm in perms.items():
        a, b = int(f["lm_ptr"][l]), int(f["lm_ptr"][l + 1])
        assert sorted(perm) == list(range(b - a))
        src[a:b] = a + np.asarray(perm)
    g = dict(f)
    for k in ("pose", "lm", "flags", "omega", "cam_id", "src"):
        g[k] = np.ascontiguousarray(f[k][src])
    g["meas"] = np.ascontiguousarray(f["meas"][:, src])
    return with_inactive(g, []), src


def schur_sigma(f, hs, Hpp, Hll, Hpl, prior=0.0):
    """sigma [B, 36]: the blocks of inv(Hsc) on the pattern, Hsc = Hpp (+ prior I) - sum Hpl_e Hll^-1 Hpl_f^T in float64
    over the counted edges of every landmark whose Hll is regular in float64 (cond < 1e13; a rank-deficient Hll has no
    Schur term worth the name); also cond(Hsc)"""
    rowptr, colind = hs[0], hs[1]
    P = f["P"]
    Hsc = np.zeros((6 * P, 6 * P))
    for p in range(P):
        Hsc[6 * p:6 * p + 6, 6 * p:6 * p + 6] = Hpp[p] + prior * np.eye(6)
    for l in range(f["L"]):
        es = lr.counted_slots(f, l)
        if len(es) == 0 or not np.linalg.cond(Hll[l]) < 1e13:
            continue
        A = Hpl[es].reshape(-1, 3)                                   # [6 d, 3]
        idx = (6 * f["pose"][es][:, None] + np.arange(6)).reshape(-1)
        Hsc[np.ix_(idx, idx)] -= A @ np.linalg.solve(Hll[l], A.T)
    Hsc = 0.5 * (Hsc + Hsc.T)
    S = np.linalg.inv(Hsc)
    S = 0.5 * (S + S.T)   # a covariance: the diagonal blocks exactly symmetric, as cugo_chol_selected_inverse writes them
    rows = np.repeat(np.arange(P), np.diff(rowptr))
    blocks = np.array([S[6 * a:6 * a + 6, 6 * b:6 * b + 6] for a, b in zip(rows, colind)]).reshape(-1, 6, 6)
    return kr.colmajor(blocks), float(np.linalg.cond(Hsc))


def finish(name, d, f, hs=None, prior=0.0):
    """the inputs of design `name` on the flattened layout f of problem dict d; prior: the information of a prior on
    every free pose that Hsc is given before it is inverted"""
    import oracle
    designed.check_layout(f)
    prob = oracle.Problem(*synth.problem_fields(d))
    hs = devmem.hsc_structure(f) if hs is None else hs
    b = kr.build(prob, (0, 1.0), f)
    Hpp, Hll, Hpl = (np.asarray(b[k], np.float64) for k in ("Hpp", "Hll", "Hpl"))
    sigma, cond = schur_sigma(f, hs, Hpp, Hll, Hpl, prior)
    assert np.all(np.isfinite(sigma)), name
    skipped = (f["flags"] & lr.SKIP) != 0
    assert not np.any(Hpl[skipped])          # (the build pass leaves zero blocks there)
    Hpl = Hpl.copy()
    Hpl[skipped] = np.nan
    return dict(name=name, d=d, f=f, rowptr=hs[0], colind=hs[1], Hll=Hll, Hpl=Hpl, sigma=sigma, cond_hsc=cond,
                skipped=skipped)


def _edges(sets):
    ep = [p for l, ps in enumerate(sets) for p in sorted(ps)]
    el = [l for l, ps in enumerate(sets) for _ in ps]
    return ep, el


def _mixed():
    rng = np.random.default_rng(31)
    n_poses, n_lm = 30, 130
    fixed_p, fixed_l = (2, 9, 16, 23), (4, 60)
    free_p = [p for p in range(n_poses) if p not in fixed_p]
    sets = []
    for l in range(n_lm):
        pool = free_p if l in fixed_l else np.arange(n_poses)
        sets.append(set(rng.choice(pool, int(rng.integers(2, 13)), replace=False).tolist()))
    sets[7] = {2, 9, 16}                      # a free landmark that fixed poses alone see
    sets[12] = {0, 5, 11, 20, 27}             # ... and one that keeps a single active edge
    sets[13] = {1, 2, 9, 14}                  # fixed and free poses together (among many)
    ep, el = _edges(sets)
    d = designed._assemble(rng, n_poses, n_lm, ep, el, fixed_p, fixed_l, stereo_frac=0.7)
    f = designed._flat(d, __import__("oracle"))[1]
    # about 15 % of the slots INACTIVE; every free landmark keeps two real edges, except landmark 12, which keeps one
    # stereo edge (three equations: Hll stays positive definite)
    lidx = f["lidx"]
    off = rng.random(f["E"]) < 0.15
    l12 = int(lidx[12])
    for l in range(f["L"]):
        a, b = f["lm_ptr"][l], f["lm_ptr"][l + 1]
        if l == l12:
            st = [e for e in range(a, b) if f["flags"][e] & 4 and not f["flags"][e] & 2]
            assert st, "landmark 12 has no stereo edge from a free pose"
            off[a:b] = True
            off[st[len(st) // 2]] = False
        else:
            k = a
            while (b - a) - off[a:b].sum() < 2:
                off[k] = False
                k += 1
    g = with_inactive(f, np.flatnonzero(off))
    return d, g


def _corners():
    """8 poses, pose id 2 fixed: free indices 0 .. 6 are the ids 0, 1, 3, 4, 5, 6, 7.  Free index 3 shares landmarks
    with lower indices only (its CSR row is its diagonal block), 0 and 6 share one (the last column of row 0)"""
    rng = np.random.default_rng(32)
    FX = "fixed"
    fid = lambda i: 2 if i == FX else (i if i < 2 else i + 1)
    groups = ([{0, 1, 2, FX}] * 6 + [{0, 3}, {1, 3}, {2, 3}, {0, 1, 3}, {1, 2, 3}, {0, 2, 3, FX}] +
              [{4, 5}, {4, 6}, {5, 6}, {4, 5, 6}, {0, 4, 5}, {1, 5, 6}, {2, 4}, {0, 6}, {0, 6, FX}, {6, FX}, {6, FX}] +
              [{4, 5, FX}, {5, 6, FX}, {4, 6, FX}])
    sets = [{fid(p) for p in s} for s in groups]
    # anchors: fixed landmarks that every free pose sees (ids in the middle of the range)
    n_anchor = 12
    sets = sets[:10] + [set(fid(i) for i in range(7))] * n_anchor + sets[10:]
    fixed_l = tuple(range(10, 10 + n_anchor))
    ep, el = _edges(sets)
    d = designed._assemble(rng, 8, len(sets), ep, el, (2,), fixed_l, stereo_frac=0.7)
    f = designed._flat(d, __import__("oracle"))[1]
    return d, f


def _far():
    """6 cameras within a ball of diameter 1 looking the same way (all free: the anchors hold the gauge; cameras 4 and 5 are 0.03 apart), 30
    fixed anchor landmarks at depth 5 to 15 that hold the poses, 48 free landmarks at depths 30 to 3000 with mono edges
    from 2 to 4 cameras"""
    rng = np.random.default_rng(33)
    cam = synth.KITTI_CAM
    n_poses, n_anchor, n_far = 6, 30, 48
    q0 = rng.normal(size=4)
    q0 /= np.linalg.norm(q0)
    centres = rng.normal(size=(n_poses, 3))
    centres *= (0.45 * rng.uniform(0.4, 1.0, n_poses) / np.linalg.norm(centres, axis=1))[:, None]
    centres[5] = centres[4] + 0.03 * np.array([1.0, 0.3, 0.1]) / np.linalg.norm([1.0, 0.3, 0.1])
    pose_gt = np.zeros((n_poses, 7))
    for i in range(n_poses):
        q = synth.quat_mul(synth.quat_from_rotvec(rng.normal(0, 0.03, 3)), q0)
        q = q / np.linalg.norm(q) * (1 if q[3] >= 0 else -1)
        pose_gt[i, :4] = q
        pose_gt[i, 4:] = -synth.quat_to_R(q) @ centres[i]
    R0 = synth.quat_to_R(q0)
    # 38 landmarks out to depth 200 from 3 or 4 cameras, 10 beyond from 2: cond(Hll) grows with (depth / baseline)^2, and
    # with it the cancellation in L^-T (G^T Sigma G) L^-1 that the mass does not see, so the far end has wide bounds
    n_near = 38
    depth = np.concatenate([rng.uniform(5, 15, n_anchor), np.exp(np.linspace(np.log(30.0), np.log(200.0), n_near)),
                            np.exp(np.linspace(np.log(400.0), np.log(3000.0), n_far - n_near))])
    xy = rng.uniform(-0.25, 0.25, (n_anchor + n_far, 2))
    lm_gt = (R0.T @ np.stack([xy[:, 0] * depth, xy[:, 1] * depth, depth], 0)).T
    sets = [set(range(n_poses))] * n_anchor
    for k in range(n_far):
        if k < n_near:
            sets.append(set(rng.choice(n_poses, 3 + k % 2, replace=False).tolist()))
        elif k % 2:
            sets.append({4, 5})                                   # the shortest baseline
        else:
            sets.append(set(rng.choice(n_poses, 2, replace=False).tolist()))
    ep, el = _edges(sets)
    ep, el = np.array(ep, np.int32), np.array(el, np.int32)
    E = len(ep)
    pose = pose_gt.copy()
    for i in range(n_poses):
        q = synth.quat_mul(synth.quat_from_rotvec(rng.normal(0, 1e-3, 3)), pose[i, :4])
        pose[i, :4] = q / np.linalg.norm(q) * (1 if q[3] >= 0 else -1)
        pose[i, 4:] += rng.normal(0, 5e-3, 3)
    lm = lm_gt * (1 + rng.normal(0, 0.01, (len(lm_gt), 1)))
    lm[:n_anchor] = lm_gt[:n_anchor]
    R = np.array([synth.quat_to_R(p[:4]) for p in pose_gt])
    Xc = np.einsum("eij,ej->ei", R[ep], lm_gt[el]) + pose_gt[ep, 4:]
    assert Xc[:, 2].min() > 4.0
    meas = np.stack([cam[0] * Xc[:, 0] / Xc[:, 2] + cam[2], cam[1] * Xc[:, 1] / Xc[:, 2] + cam[3], np.zeros(E)], 1)
    meas[:, :2] += rng.normal(0, 0.3, (E, 2))
    pf = np.zeros(n_poses, np.uint8)
    lf = np.zeros(len(lm), np.uint8); lf[:n_anchor] = 1
    d = dict(pose=pose, pose_fixed=pf, lm=lm, lm_fixed=lf, e_pose=ep, e_lm=el, e_stereo=np.zeros(E, np.uint8),
             e_meas=meas, e_omega=np.ones(E), e_cam=np.tile(cam, (E, 1)), pose_gt=pose_gt, lm_gt=lm_gt)
    f = designed._flat(d, __import__("oracle"))[1]
    return d, f


def _grid(n_free):
    """n_free free landmarks of degree 2 or 3 on 6 poses (pose 1 fixed) and 10 fixed landmarks that every free pose
    sees (they keep the Schur complement regular when one free landmark is all there is)"""
    rng = np.random.default_rng(40 + n_free)
    n_poses, n_anchor = 6, 10
    free_p = [0, 2, 3, 4, 5]
    sets = [set(free_p)] * n_anchor + [set(rng.choice(n_poses, 2 + (k % 2), replace=False).tolist()) for k in range(n_free)]
    ep, el = _edges(sets)
    d = designed._assemble(rng, n_poses, len(sets), ep, el, (1,), tuple(range(n_anchor)), stereo_frac=0.7)
    f = designed._flat(d, __import__("oracle"))[1]
    assert f["L"] == n_free
    return d, f


@functools.lru_cache(maxsize=None)
def design(name):
    """the inputs of a design (built once per process and never modified: copy before changing anything), checked
    against what the design promises"""
    if name == "B":
        d, _, f, hs = designed.layout("B")
        des = finish(name, d, f, hs, prior=B_PRIOR)
    elif name == "B_padded":
        d, _, f, hs = designed.layout("B")
        g = devmem.pad_to_groups(f)
        des = finish(name, d, g, prior=B_PRIOR)
        assert np.array_equal(des["rowptr"], hs[0]) and np.array_equal(des["colind"], hs[1])
    elif name == "mixed":
        des = finish(name, *_mixed())
    elif name == "corners":
        des = finish(name, *_corners())
    elif name == "far":
        des = finish(name, *_far())
    elif name.startswith("grid"):
        des = finish(name, *_grid(int(name[4:])))
    else:
        raise KeyError(name)
    check_design(des)
    return des


def pattern_rows(des):
    rp, ci = des["rowptr"], des["colind"]
    return [ci[rp[p]:rp[p + 1]].tolist() for p in range(len(rp) - 1)]


def counted_poses(des, l):
    return des["f"]["pose"][lr.counted_slots(des["f"], l)].tolist()


def check_design(des):
    """what each design was built for, asserted on the CPU from the layout and the pattern"""
    name, f = des["name"], des["f"]
    P, L, fl = f["P"], f["L"], f["flags"]
    lmdeg = np.diff(f["lm_ptr"])[:L]
    rows = pattern_rows(des)
    seen = [counted_poses(des, l) for l in range(L)]
    assert len(des["Hll"]) == L and len(des["Hpl"]) == f["E"] and len(des["sigma"]) == len(des["colind"])
    assert np.all(np.isnan(des["Hpl"][des["skipped"]])) and np.all(np.isfinite(des["Hpl"][~des["skipped"]]))
    if name in ("B", "B_padded"):
        degs = [len(s) + int(((fl[f["lm_ptr"][l]:f["lm_ptr"][l + 1]] & 11) == 2).sum()) for l, s in enumerate(seen)]
        assert degs == list(designed.B_LM_DEGREES), degs
        assert max(len(s) for s in seen) >= 290
        if name == "B_padded":
            pad = (fl & 8) != 0
            assert pad.any() and not f["pose"][pad].any() and f["E"] > designed.layout("B")[2]["E"]
    elif name == "mixed":
        slots = lambda l: np.arange(f["lm_ptr"][l], f["lm_ptr"][l + 1])
        both = [l for l in range(L) if (fl[slots(l)] & 10 == 2).any() and len(seen[l]) >= 1]
        assert len(both) >= 20
        l7, l12 = int(f["lidx"][7]), int(f["lidx"][12])
        assert l7 < L and lmdeg[l7] == 3 and np.all(fl[slots(l7)] & 2) and not seen[l7]
        assert l12 < L and lmdeg[l12] == 5 and len(seen[l12]) == 1 and int((fl[slots(l12)] & 8 != 0).sum()) == 4
        free_slots = f["lm"] < L
        frac = float(((fl & 8) != 0)[free_slots].mean())
        assert 0.10 <= frac <= 0.20, frac
        assert f["Lall"] - L == 2 and f["Pall"] - P == 4
        assert not des["d"]["pose_fixed"][-1] and not des["d"]["lm_fixed"][-1]
    elif name == "corners":
        assert P == 7 and rows[3] == [3], rows[3]                              # a row with its diagonal block only
        assert rows[P - 1] == [P - 1]
        assert rows[0][-1] == P - 1 and any(0 in s and P - 1 in s for s in seen)   # pose 0 with pose P-1, at the last
        assert any(s == [P - 1] for s in seen)                                 # column of row 0; pose P-1 alone
        assert any(len(r) > 2 and r[-1] < P - 1 for r in rows)                 # a last column that is not the last pose
    elif name == "far":
        assert not (fl & 4).any(), "far: mono edges only"
        assert all(2 <= len(s) <= 4 for s in seen) and {len(s) for s in seen} == {2, 3, 4}
        kap = np.linalg.cond(des["Hll"])
        assert np.all(np.linalg.eigvalsh(des["Hll"])[:, 0] > 0), "far: an Hll is not positive definite in float64"
        assert kap.max() / kap.min() >= 1e6, (kap.min(), kap.max())
        c = np.array([-synth.quat_to_R(p[:4]).T @ p[4:] for p in des["d"]["pose_gt"]])
        assert max(np.linalg.norm(a - b) for a in c for b in c) <= 1.0 + 1e-12
    elif name.startswith("grid"):
        assert L == int(name[4:]) and lmdeg.max() <= 3 and lmdeg.min() >= 2
