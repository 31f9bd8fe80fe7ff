"""The backward substitution in one launch (k_backward_chain, CUGO_BW_CHAIN=1, the default): the plan's ticket order
and ancestor segments replayed with numpy, and on the GPU the chain form against numpy, against itself (bits) and
against the launch-per-stage form (CUGO_BW_CHAIN=0) on the smallest shapes at which the hand-off can go wrong."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":  # (the child process of the delay test: the package lies one directory up)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import chol_designed
from test_host import covis_pattern, patterns, plan_arrays, random_spd_bsr

cugo = importlib.import_module("cuda-bundle-adjustment_amd")


@pytest.fixture(scope="module")
def lib():
    cugo.build()
    return cugo.lib()


def csr(rows):
    rowptr = np.array([0] + list(np.cumsum([len(r) for r in rows])), np.int32)
    colind = np.array([c for r in rows for c in r], np.int32)
    return rowptr, colind


def synth_pattern(n_poses, n_lm, n_edges, seed, lc):
    d = cugo.synth(n_poses, n_lm, n_edges, seed=seed, n_loop_closures=lc)
    ep = d["e_pose"].astype(np.int64) - 1  # pose 0 is fixed
    ep[ep < 0] = 10**6
    return covis_pattern(n_poses - 1, ep, d["e_lm"])


def pattern(name):
    if name == "synthetic":
        return synth_pattern(160, 2500, 10500, 3, 80)
    if name in chol_designed.NAMES:
        return chol_designed.design(name)[:2]
    return csr(patterns()[name])


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


def chain_arrays(lib, s):
    seg = plan32(lib, s, "bc_seg")
    assert len(seg) % 3 == 0
    return plan32(lib, s, "bc_front"), plan32(lib, s, "bc_seg_ptr"), seg.reshape(-1, 3)


# ------------------------------------------------------------------ host, no GPU -----------
HOST_ENVS = [{}, {"CUGO_ND_LEAF": "4", "CUGO_MAX_SUPER_COLS": "3", "CUGO_TARGET_TASKS": "4"},
             {"CUGO_MAX_SUPER_COLS": "1"}]


@pytest.mark.parametrize("name", list(patterns().keys()) + ["synthetic"] + list(chol_designed.NAMES))
@pytest.mark.parametrize("env", HOST_ENVS)
def test_ticket_order_and_segments_replay_the_backward_pass(lib, name, env, monkeypatch):
    """every front holds one ticket; every segment names a front with a smaller ticket; the segments of a front tile
    its boundary block rows exactly once, in row order, every one inside the pivot columns of the front it names and
    at most 16 block rows long, the parent's first; and the backward pass walked in ticket order through the
    segments (topmost first, as the kernel adds them) on a numpy L L^T of the permuted matrix gives solve(A, b)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rowptr, colind = pattern(name)
    n = len(rowptr) - 1
    s = analyze(lib, rowptr, colind)
    pl = plan_arrays(lib, s)
    order, seg_ptr, seg = chain_arrays(lib, s)
    ns = len(pl["ncb"])
    assert sorted(order) == list(range(ns)) and len(seg_ptr) == ns + 1 and seg_ptr[-1] == len(seg)
    ticket = np.empty(ns, np.int64)
    ticket[order] = np.arange(ns)
    rows_ptr, rows, ncb, col0, col_front = pl["rows_ptr"], pl["rows"], pl["ncb"], pl["col0"], pl["col_front"]
    for f in range(ns):
        nbr = rows_ptr[f + 1] - rows_ptr[f]
        nxt = 0
        for k in range(seg_ptr[f], seg_ptr[f + 1]):
            a, r0, cnt = seg[k]
            assert ticket[a] < ticket[f]
            assert r0 == nxt and 1 <= cnt <= 16
            rr = rows[rows_ptr[f] + r0:rows_ptr[f] + r0 + cnt]
            assert (col_front[rr] == a).all() and (rr >= col0[a]).all() and (rr < col0[a] + ncb[a]).all()
            nxt = r0 + cnt
        assert nxt == nbr
        if nbr:
            assert seg[seg_ptr[f]][0] == pl["sparent"][f]
        else:
            assert pl["sparent"][f] == -1
    # numpy L L^T of P (A + lam I) P^T, forward solve, then the backward pass front by front in ticket order
    rng = np.random.default_rng(5)
    A, _ = random_spd_bsr(rowptr, colind, rng)
    lam = 0.37
    b = rng.normal(size=6 * n)
    sidx = (6 * np.repeat(pl["perm"], 6) + np.tile(np.arange(6), n)).astype(int)
    Lf = np.linalg.cholesky((A + lam * np.eye(6 * n))[np.ix_(sidx, sidx)])
    y = np.linalg.solve(Lf, b[sidx])
    xnew = np.full(6 * n, np.nan)  # (a value read before its front has run poisons the result)
    for f in order:
        J = np.arange(6 * col0[f], 6 * (col0[f] + ncb[f]))
        acc = np.zeros(len(J))
        for k in range(seg_ptr[f + 1] - 1, seg_ptr[f] - 1, -1):
            a, r0, cnt = seg[k]
            rr = rows[rows_ptr[f] + r0:rows_ptr[f] + r0 + cnt]
            ridx = (6 * np.repeat(rr, 6) + np.tile(np.arange(6), cnt)).astype(int)
            acc += Lf[np.ix_(ridx, J)].T @ xnew[ridx]
        xnew[J] = np.linalg.solve(Lf[np.ix_(J, J)].T, y[J] - acc)
    x = np.empty(6 * n)
    x[sidx] = xnew
    np.testing.assert_allclose(x, np.linalg.solve(A + lam * np.eye(6 * n), b), rtol=1e-10, atol=1e-10)
    lib.cugo_chol_destroy(s)


# ------------------------------------------------------------------ on the GPU -----------
def arrow_rows(n=60, tail=20):
    """a band whose every column also couples with the last `tail` columns: the fronts below the top carry more
    than 16 boundary block rows"""
    return [sorted(set(list(range(r, min(n, r + 3))) + list(range(max(r, n - tail), n)))) for r in range(n)]


def case(name):
    """(rowptr, colind, environment of the analysis)"""
    if name == "one_front":  # (a) no hand-off at all
        return csr([list(range(r, 10)) for r in range(10)]) + ({},)
    if name == "dense_band":  # (b) a parent stored in its only child's update block
        return csr([list(range(r, 20)) for r in range(20)]) + ({},)
    if name == "pose_graph":  # (c) 6 stages, two-children fronts, boundaries that span parent, grandparent and beyond
        return synth_pattern(120, 1500, 6200, 3, 60) + ({"CUGO_ND_LEAF": "4"},)
    if name == "wide_boundary":  # (d) more than 16 boundary block rows
        return csr(arrow_rows()) + ({},)
    if name == "long_path":  # (e) more fronts than the chip holds workgroups at once
        return csr([[r] + ([r + 1] if r + 1 < 700 else []) for r in range(700)]) + ({"CUGO_MAX_SUPER_COLS": "1"},)
    raise KeyError(name)


CASES = ["one_front", "dense_band", "pose_graph", "wide_boundary", "long_path"]
LAMBDAS = (0.0, 2.5, 0.125)


@pytest.fixture(scope="module")
def ctx():
    import devmem
    if cugo.device_count() == 0:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    c = devmem.Ctx()
    yield c
    c.close()


def check_shape(lib, name, s):
    """the case has the property it is there for"""
    pl = plan_arrays(lib, s)
    ns, nbr = len(pl["ncb"]), pl["nb"] - pl["ncb"]
    nst = len(pl["stage_task_ptr"]) - 1
    if name == "one_front":
        assert ns == 1
    elif name == "dense_band":
        assert ns >= 2 and (plan32(lib, s, "alias_of") >= 0).any()
    elif name == "pose_graph":
        _, seg_ptr, _ = chain_arrays(lib, s)
        assert nst >= 6 and np.diff(pl["child_ptr"]).max() >= 2 and np.diff(seg_ptr).max() >= 3
    elif name == "wide_boundary":
        assert nbr.max() > 16
    elif name == "long_path":
        assert ns == 700 and nst > 32


def solve_rounds(lib, ctx, s, n, vals, rhs, rounds=1):
    dH, dx, fail = ctx.to_dev(vals), ctx.empty(6 * n), ctx.empty(2, np.int32)
    out = []
    for _ in range(rounds):
        xs = []
        for lam, b in zip(LAMBDAS, rhs):
            cugo.check(lib.cugo_chol_factor_solve(s, dH, C.c_double(lam), ctx.to_dev(b), dx, fail))
            assert ctx.to_host(fail, 1, np.int32)[0] == 0
            xs.append(ctx.to_host(dx, 6 * n).copy())
        out.append(xs)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_chain_form_against_numpy_itself_and_the_staged_form(ctx, name, monkeypatch):
    """three consecutive calls on ONE solver with different lambda and right-hand sides, each against numpy (a stale
    epoch or x of the previous call shows here); the same three again: identical bits; CUGO_BW_CHAIN=0: equal to
    rounding, max |dx| <= 1e-12 max |x| (the two forms associate the sum over the ancestor rows differently); an
    indefinite matrix raises the flag, the call returns and the solver goes on working."""
    lib = cugo.lib()
    rowptr, colind, env = case(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n = len(rowptr) - 1
    A, vals = random_spd_bsr(rowptr, colind, np.random.default_rng(21))
    rhs = [np.random.default_rng(30 + k).normal(size=6 * n) for k in range(len(LAMBDAS))]
    monkeypatch.setenv("CUGO_BW_CHAIN", "1")  # (read when the solver is created)
    s = analyze(lib, rowptr, colind, ctx.h)
    check_shape(lib, name, s)
    first, again = solve_rounds(lib, ctx, s, n, vals, rhs, rounds=2)
    for lam, b, x in zip(LAMBDAS, rhs, first):
        np.testing.assert_allclose(x, np.linalg.solve(A + lam * np.eye(6 * n), b), rtol=1e-9, atol=1e-12, err_msg=name)
    for x, x2 in zip(first, again):
        assert np.array_equal(x.view(np.int64), x2.view(np.int64)), name
    # indefinite: the flag as before, nothing waits, and the next call is right again
    bad = vals.copy()
    bad[rowptr[n // 2]] = -np.eye(6).reshape(-1)
    dx, fail = ctx.empty(6 * n), ctx.empty(2, np.int32)
    cugo.check(lib.cugo_chol_factor_solve(s, ctx.to_dev(bad), C.c_double(0.0), ctx.to_dev(rhs[0]), dx, fail))
    assert ctx.to_host(fail, 1, np.int32)[0] == 1, name
    (after,) = solve_rounds(lib, ctx, s, n, vals, rhs)
    for x, x2 in zip(first, after):
        assert np.array_equal(x.view(np.int64), x2.view(np.int64)), name
    lib.cugo_chol_destroy(s)
    monkeypatch.setenv("CUGO_BW_CHAIN", "0")
    s0 = analyze(lib, rowptr, colind, ctx.h)
    (staged,) = solve_rounds(lib, ctx, s0, n, vals, rhs)
    lib.cugo_chol_destroy(s0)
    for x, x0 in zip(first, staged):
        d, m = np.abs(x - x0).max(), np.abs(x).max()
        print("%s: max |dx| %.3e  max |x| %.3e" % (name, d, m))
        assert d <= 1e-12 * m, name


@pytest.mark.gpu
def test_chain_form_gives_the_staged_forms_trajectory(monkeypatch):
    """a medium graph end to end in both forms: the same number of trials in every iteration, chi2 equal to 1e-10
    relative; the chain form twice: the same bits"""
    runs = []
    for chain in ("1", "1", "0"):
        monkeypatch.setenv("CUGO_BW_CHAIN", chain)
        d = cugo.synth(400, 8000, 33000, seed=11, n_loop_closures=200)
        g = cugo.graph_from_arrays(d)
        g.initialize()
        g.optimize(10)
        runs.append((g.stats(), g.poses().copy(), g.landmarks().copy()))
        g.close()
    (sa, pa, la), (sb, pb, lb), (sc, _, _) = runs
    assert sa == sb
    assert np.array_equal(pa.view(np.int64), pb.view(np.int64))
    assert np.array_equal(la.view(np.int64), lb.view(np.int64))
    assert len(sa) == len(sc)
    for a, c in zip(sa, sc):
        assert a["trials"] == c["trials"] and a["iteration"] == c["iteration"]
        print("chi2 %r / %r" % (a["chi2"], c["chi2"]))
        assert abs(a["chi2"] - c["chi2"]) <= 1e-10 * abs(c["chi2"])


DELAYS = ["0", "31", "0"]


def delay_child():
    """(child process with the hooks library) case (c), CUGO_DEBUG_DELAY as listed: prints one line per value"""
    import devmem
    lib = cugo.lib()
    c = devmem.Ctx()
    rowptr, colind, env = case("pose_graph")
    os.environ.update(env)
    n = len(rowptr) - 1
    _, vals = random_spd_bsr(rowptr, colind, np.random.default_rng(21))
    rhs = [np.random.default_rng(30 + k).normal(size=6 * n) for k in range(len(LAMBDAS))]
    ref = None
    for delay in DELAYS:
        os.environ["CUGO_DEBUG_DELAY"] = delay  # (read when a plan is uploaded)
        s = analyze(lib, rowptr, colind, c.h)
        (xs,) = solve_rounds(lib, c, s, n, vals, rhs)
        lib.cugo_chol_destroy(s)
        ref = xs if ref is None else ref
        same = all(np.array_equal(a.view(np.int64), r.view(np.int64)) for a, r in zip(xs, ref))
        print("CUGO_DEBUG_DELAY=%s %s" % (delay, "same" if same else "DIFFERENT"), flush=True)
    c.close()


@pytest.mark.gpu
def test_chain_gives_the_same_bits_whichever_front_runs_late():
    """hooks build, CUGO_DEBUG_DELAY=31: every second front's workgroup sleeps ~25 k cycles before its first poll and
    between its last x store and its done store — the bits of no delay (case (c))"""
    from conftest import ROOT
    hooks = cugo.HOOKS_LIB_PATH
    if not os.path.exists(hooks):
        pytest.fail("libcugo_hip_hooks.so missing: run __graft_entry__.build()")
    env = dict(os.environ, CUGO_LIB=hooks, CUGO_BW_CHAIN="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "test_backward_chain.py"), "--delay-child"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert r.stdout.count(" same") == len(DELAYS) and "DIFFERENT" not in r.stdout, r.stdout


if __name__ == "__main__" and "--delay-child" in sys.argv:
    delay_child()
