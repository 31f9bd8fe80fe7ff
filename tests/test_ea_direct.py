"""The children's contributions to F11 read straight from their update blocks (k_up_potrf,
l11_add_children): the plan's child link records (ea1) replayed with numpy, and on the GPU the
factorisation with CUGO_EA_DIRECT=1 (default) against the unit-by-unit gather (CUGO_EA_DIRECT=0),
bit for bit."""
import ctypes as C
import importlib

import numpy as np
import pytest

from test_host import covis_pattern, patterns, plan_arrays, random_spd_bsr

cugo = importlib.import_module("cuda-bundle-adjustment_amd")

EA1_REC = 16  # kernels.h: ints per child link record


@pytest.fixture(scope="module")
def lib():
    cugo.build()
    return cugo.lib()


def pattern(name):
    if name == "synthetic":
        d = cugo.synth(160, 2500, 10500, seed=3, n_loop_closures=80)
        ep = d["e_pose"].astype(np.int64) - 1
        ep[ep < 0] = 10**6
        return covis_pattern(159, ep, d["e_lm"])
    rows = patterns()[name]
    rowptr = np.array([0] + list(np.cumsum([len(r) for r in rows])), np.int32)
    colind = np.array([c for r in rows for c in r], np.int32)
    return rowptr, colind


def analyze(lib, rowptr, colind, ctx=None):
    s = C.c_void_p()
    assert lib.cugo_chol_create(ctx, C.byref(s)) == 0
    rc = lib.cugo_chol_analyze(s, len(rowptr) - 1, rowptr.ctypes.data_as(C.POINTER(C.c_int32)),
                               colind.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0, lib.cugo_last_error()
    return s


def plan64(lib, s, name):
    p = C.POINTER(C.c_int64)()
    n = lib.cugo_chol_plan_array64(s, name.encode(), C.byref(p))
    assert n >= 0, name
    return np.ctypeslib.as_array(p, shape=(n,)).copy()


def ea1_records(lib, s):
    p = C.POINTER(C.c_int32)()
    n = lib.cugo_chol_plan_array(s, b"ea1", C.byref(p))
    assert n >= 0 and n % EA1_REC == 0
    return np.ctypeslib.as_array(p, shape=(n,)).copy().reshape(-1, EA1_REC) if n else np.zeros((0, EA1_REC), np.int32)


def direct_map(m, x):
    """parent pivot scalar x -> (covered by the child of block mask m, the child's own row / column)"""
    b = x // 6
    return bool((m >> b) & 1), 6 * bin(m & ((1 << b) - 1)).count("1") + x % 6


ENVS = [{}, {"CUGO_ALIAS_CHAINS": "0"}, {"CUGO_MAX_SUPER_COLS": "5", "CUGO_ALIAS_CHAINS": "0"},
        {"CUGO_ND_LEAF": "4", "CUGO_MAX_SUPER_COLS": "3", "CUGO_TARGET_TASKS": "4"},
        {"CUGO_MAX_SUPER_COLS": "24", "CUGO_ZERO_FRAC": "0.9"}]


@pytest.mark.parametrize("name", list(patterns().keys()) + ["synthetic"])
@pytest.mark.parametrize("env", ENVS)
def test_child_records_map_lead_entries_where_the_gather_adds_them(lib, name, env, monkeypatch):
    """every record belongs to a child of a front that gathers (not stored in its child), in child order;
    its block mask holds exactly the parent pivot block rows of the child's leading rows; and for every
    entry (i, j), j <= i, of a child's leading block, the parent F11 position the gather (ea_chunk) adds it to
    is covered by the mask and maps back to (i, j) — and no other position is covered.  Then F11 + the
    children's terms formed both ways, in child order, is the same array bit for bit."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rowptr, colind = pattern(name)
    s = analyze(lib, rowptr, colind)
    pl = plan_arrays(lib, s)
    alias = plan_arrays_alias(lib, s)
    off, ldf = plan64(lib, s, "off"), plan64(lib, s, "ldf")
    rec = ea1_records(lib, s)
    ncb, nb, cp, ch, rp, rel = pl["ncb"], pl["nb"], pl["child_ptr"], pl["child"], pl["rel_ptr"], pl["rel"]
    rng = np.random.default_rng(7)
    k = 0
    for f in range(len(ncb)):
        if alias[f] >= 0:
            continue
        nc = 6 * ncb[f]
        F11 = rng.normal(size=(nc, nc))
        gathered, direct = F11.copy(), F11.copy()
        terms = []
        for c in ch[cp[f]:cp[f + 1]]:
            r = rec[k]
            k += 1
            nbr = nb[c] - ncb[c]
            crel = rel[rp[c]:rp[c] + nbr]
            npl = int((crel < ncb[f]).sum())
            assert (crel[:npl] < ncb[f]).all() and (np.diff(crel) > 0).all()  # leading rows first, ascending
            assert list(r[:4]) == [c, nbr, npl, rp[c]]
            ncs_c = 6 * ncb[c]
            assert r[4:6].view(np.int64)[0] == off[c] + ncs_c * ldf[c] + ncs_c
            assert r[6:8].view(np.int64)[0] == ldf[c]
            m = int(np.uint32(r[8]))
            assert m == sum(1 << int(b) for b in crel[:npl])
            assert not r[9:].any()
            # the gather's target of every leading entry (ea_chunk: parent column from the child column,
            # parent row from the child row)
            q = 6 * npl
            pidx = 6 * np.repeat(crel[:npl], 6) + np.tile(np.arange(6), npl)
            covered = set()
            for j in range(q):
                for i in range(j, q):
                    pr, pc = int(pidx[i]), int(pidx[j])
                    assert pr >= pc
                    okr, jr = direct_map(m, pr)
                    okc, jc = direct_map(m, pc)
                    assert okr and okc and (jr, jc) == (i, j)
                    covered.add((pr, pc))
            for pc in range(nc):
                for pr in range(pc, nc):
                    assert (direct_map(m, pr)[0] and direct_map(m, pc)[0]) == ((pr, pc) in covered)
            terms.append((m, pidx, rng.normal(size=(q, q))))
        # F11 + children, the gather's way (child after child through rel) and the direct way (entry by
        # entry, children in order, uncovered positions skipped)
        for m, pidx, U in terms:
            q = len(pidx)
            for j in range(q):
                for i in range(j, q):
                    gathered[pidx[i], pidx[j]] = gathered[pidx[i], pidx[j]] + U[i, j]
        for pc in range(nc):
            for pr in range(pc, nc):
                v = direct[pr, pc]
                for m, pidx, U in terms:
                    okr, jr = direct_map(m, pr)
                    okc, jc = direct_map(m, pc)
                    if okr and okc:
                        v = v + U[jr, jc]
                direct[pr, pc] = v
        lo = np.tril(np.ones((nc, nc), bool))
        assert np.array_equal(gathered[lo].view(np.int64), direct[lo].view(np.int64))
    assert k == len(rec)
    lib.cugo_chol_destroy(s)


def plan_arrays_alias(lib, s):
    p = C.POINTER(C.c_int32)()
    n = lib.cugo_chol_plan_array(s, b"alias_of", C.byref(p))
    assert n >= 0
    return np.ctypeslib.as_array(p, shape=(n,)).copy()


# ------------------------------------------------------------------ on the GPU -----------
# the Cholesky variants in which the potrf adds its children's F11 terms (k_up_potrf with the extend-add into
# LDS): default tiles, 64x64 tiles, the two-phase form, the 6-column panels, no storage sharing, narrow fronts
CHOL_ENVS = [{}, {"CUGO_ALIAS_CHAINS": "0"}, {"CUGO_TILE32_MAX_TILES": "0", "CUGO_MAX_SUPER_COLS": "5"},
             {"CUGO_TWO_PHASE_MIN_TILES": "1", "CUGO_TILE32_MAX_TILES": "0", "CUGO_ALIAS_CHAINS": "0"},
             {"CUGO_PANEL16": "0"}, {"CUGO_ASM_FRONTS": "0", "CUGO_MAX_SUPER_COLS": "24", "CUGO_ZERO_FRAC": "0.9"}]


@pytest.fixture(scope="module")
def ctx():
    import devmem
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    c = devmem.Ctx()
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("env", CHOL_ENVS)
def test_direct_children_terms_give_the_gathers_bits(ctx, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    lib = cugo.lib()
    for name in list(patterns().keys()) + ["synthetic"]:
        rowptr, colind = pattern(name)
        n = len(rowptr) - 1
        A, vals = random_spd_bsr(rowptr, colind, np.random.default_rng(11))
        b = np.random.default_rng(12).normal(size=6 * n)
        xs = {}
        for direct in ("1", "0"):
            monkeypatch.setenv("CUGO_EA_DIRECT", direct)  # (read when the solver is created)
            s = analyze(lib, rowptr, colind, ctx.h)
            dH, db, dx, fail = ctx.to_dev(vals), ctx.to_dev(b), ctx.empty(6 * n), ctx.empty(2, np.int32)
            out = []
            for lam in (0.0, 2.5):
                cugo.check(lib.cugo_chol_factor_solve(s, dH, C.c_double(lam), db, dx, fail))
                assert ctx.to_host(fail, 1, np.int32)[0] == 0, name
                out.append(ctx.to_host(dx, 6 * n).copy())
            lib.cugo_chol_destroy(s)
            xs[direct] = out
        for a, g in zip(xs["1"], xs["0"]):
            assert np.array_equal(a.view(np.int64), g.view(np.int64)), name
        np.testing.assert_allclose(xs["1"][1], np.linalg.solve(A + 2.5 * np.eye(6 * n), b), rtol=1e-9, atol=1e-12)


@pytest.mark.gpu
def test_direct_children_terms_give_the_same_trajectory(monkeypatch):
    """a medium graph end to end: chi2, lambda, rho and the estimates bit for bit with and without"""
    runs = {}
    for direct in ("1", "0"):
        monkeypatch.setenv("CUGO_EA_DIRECT", direct)
        d = cugo.synth(400, 8000, 33000, seed=11, n_loop_closures=200)
        g = cugo.graph_from_arrays(d)
        g.initialize()
        g.optimize(10)
        runs[direct] = (g.stats(), g.poses().copy(), g.landmarks().copy())
        g.close()
    (sa, pa, la), (sb, pb, lb) = runs["1"], runs["0"]
    assert sa == sb
    assert np.array_equal(pa.view(np.int64), pb.view(np.int64))
    assert np.array_equal(la.view(np.int64), lb.view(np.int64))
