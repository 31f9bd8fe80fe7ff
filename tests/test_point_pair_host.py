"""CPU checks of the pose-pose point edges (no GPU): the symbols of the C ABI, exported and declared; the host-only plan
(csrc/host/point_pair_plan.cpp) against the brute-force numpy plan of tests/point_pair_ref.py on the designed layouts;
its refusals; the ctypes mirror of cugo_point_pair_edges; and the plan compiled with g++ -fsanitize=address,undefined into
a stand-alone program that builds the designs' plans (nothing is preloaded, nothing is loaded into python)."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import pair_designed as pdz
import point_pair_ref as ppr
from conftest import ROOT

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
HOST = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "csrc", "host")

SYMBOLS = ["cugo_point_pair_plan_create", "cugo_point_pair_plan_destroy", "cugo_point_pair_plan_array",
           "cugo_point_pair_compute_errors", "cugo_point_pair_construct_quadratic_form",
           "cugo_point_pair_construct_quadratic_form_schur", "cugo_point_pair_construct_quadratic_form_diag",
           "cugo_point_pair_add_offdiag_schur"]


def test_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "cugo_hip.h")).read()
    for s in SYMBOLS:
        assert hasattr(cugo.lib(), s), s
        assert re.search(r"\b%s\(" % s, header), s
    assert "typedef struct cugo_point_pair_edges" in header and "typedef struct cugo_point_pair_plan cugo_point_pair_plan;" in header
    for name in ("PointPairPlan", "PointPairEdges", "point_pair_compute_errors", "point_pair_construct_quadratic_form",
                 "point_pair_construct_quadratic_form_schur", "point_pair_construct_quadratic_form_diag", "point_pair_add_offdiag_schur"):
        assert hasattr(cugo, name), name


def host_plan(lay, pattern=True):
    e = lay["e"]
    P = lay["n_free"]
    free = ppr.numpy_plan(e["a"], e["b"], e["active"], P)
    pat = ppr.pair_pattern(P, free["pair_lo"], free["pair_hi"], [(0, P - 1)] if P > 1 else []) if pattern else (None, None)
    return cugo.PointPairPlan(None, lay["P"], P, e["a"], e["b"], e["flags"], *pat), ppr.numpy_plan(e["a"], e["b"], e["active"], P, *pat)


@pytest.mark.parametrize("name", pdz.NAMES + ["Z"])
def test_host_only_plan_matches_the_numpy_plan(name):
    lay = pdz.zero_residual((0, 1.0)) if name == "Z" else pdz.layout(name)
    plan, want = host_plan(lay)
    for k in cugo.PointPairPlan.ARRAYS:
        assert np.array_equal(plan.array(k), want[k]), (name, k)
    # the sort is stable and by (lo, hi, orientation); the runs of a block are adjacent
    perm = plan.array("perm")
    a, b = lay["e"]["a"][perm], lay["e"]["b"][perm]
    key = np.stack([np.minimum(a, b), np.maximum(a, b), a > b, perm], 1).astype(np.int64)
    assert all(tuple(key[i]) < tuple(key[i + 1]) for i in range(len(key) - 1))
    assert np.all(np.diff(plan.array("blk_ptr")) <= 2) and np.all(np.diff(plan.array("blk_run")) > 0)
    with pytest.raises(cugo.CugoError):
        plan.array("no_such_array")
    plan.close()


def test_plan_without_a_pattern_lists_the_pairs():
    lay = pdz.layout("A_spd")
    plan, want = host_plan(lay, pattern=False)
    assert np.array_equal(plan.array("pair_lo"), want["pair_lo"]) and np.array_equal(plan.array("pair_hi"), want["pair_hi"])
    assert np.all(plan.array("run_blk") == -1) and len(plan.array("blk_id")) == 0
    # distinct, counting, free-free: neither the inactive run 22->23 nor a pair with a fixed end
    pairs = set(zip(plan.array("pair_lo").tolist(), plan.array("pair_hi").tolist()))
    assert (0, 1) in pairs and (22, 23) not in pairs and all(h < lay["n_free"] for _, h in pairs) and len(pairs) == len(want["pair_lo"])
    plan.close()


def test_plan_refusals():
    P = 4
    rowptr, colind = ppr.pair_pattern(P, [0], [1])

    def refused(a, b, what, n_total=5, rp=rowptr, ci=colind, flags=None):
        with pytest.raises(cugo.CugoError) as ei:
            cugo.PointPairPlan(None, n_total, P, a, b, flags, rp, ci)
        assert what in str(ei.value), str(ei.value)

    refused([0, 2], [1, 2], "joins pose 2 to itself")
    refused([0, 2], [1, 2], "joins pose 2 to itself", flags=[0, 8])            # whatever the edge's flags
    refused([0, 5], [1, 1], "pose index out of range")
    refused([0, -1], [1, 1], "pose index out of range")
    refused([0, 1], [1, 2], "block (1, 2) is missing from the pattern")
    refused([0], [1], "does not start with its diagonal block", ci=np.array([1, 0, 1, 2, 3], np.int32))
    refused([0], [1], "bad pose or edge counts", n_total=3)
    # an inactive edge, an edge to a fixed pose and one between fixed poses need no block
    plan = cugo.PointPairPlan(None, 6, P, [0, 1, 2, 4], [1, 2, 4, 5], [0, 8, 0, 0], rowptr, colind)
    assert plan.array("run_blk").tolist() == [0 + 1, -1, -1, -1] and plan.array("run_flags").tolist() == [11, 3, 9, 0]
    plan.close()


LAYOUT_PROGRAM = r"""
#include <cstddef>
#include <cstdio>
#include "cugo_hip.h"
#define F(x) std::printf("%s %zu\n", #x, offsetof(cugo_point_pair_edges, x));
int main()
{
    F(n_poses_total) F(n_poses_free) F(n) F(d_pose_a) F(d_pose_b) F(d_p) F(d_z) F(d_info) F(n_info) F(d_flags) F(rk) F(delta) F(plan)
    std::printf("sizeof %zu\n", sizeof(cugo_point_pair_edges));
    return 0;
}
"""


def test_ctypes_layout_of_point_pair_edges_matches_the_c_struct(tmp_path):
    src = tmp_path / "layout.cpp"
    src.write_text(LAYOUT_PROGRAM)
    exe = tmp_path / "layout"
    r = subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split("\n") if line)
    assert len(out) == len(cugo.PointPairEdges._fields_) + 1
    for name, _ in cugo.PointPairEdges._fields_:
        assert int(out[name]) == getattr(cugo.PointPairEdges, name).offset, name
    assert int(out["sizeof"]) == C.sizeof(cugo.PointPairEdges)


def c_array(ctype, name, a):
    return "static const %s %s[] = {%s};\n" % (ctype, name, ", ".join(str(int(x)) for x in a) if len(a) else "0")


PLAN_MAIN = r"""
#include <cstdio>
#include <stdexcept>
#include "point_pair_plan.h"
static int check(const char* name, const std::vector<int32_t>& got, const int32_t* want, size_t n)
{
    if (got.size() != n) { std::printf("%s: %zu entries, want %zu\n", name, got.size(), n); return 1; }
    for (size_t i = 0; i < n; i++)
        if (got[i] != want[i]) { std::printf("%s[%zu] = %d, want %d\n", name, i, got[i], want[i]); return 1; }
    return 0;
}
int main()
{
    int bad = 0;
    cugo_host::PointPairPlanHost plan;
@BODY@
    const int32_t self_a[] = {0, 1}, self_b[] = {1, 1};
    try { cugo_host::build_point_pair_plan(2, 3, 3, self_a, self_b, nullptr, nullptr, nullptr, plan); bad++; } catch (const std::invalid_argument&) {}
    const int32_t far_b[] = {1, 7};
    try { cugo_host::build_point_pair_plan(2, 3, 3, self_a, far_b, nullptr, nullptr, nullptr, plan); bad++; } catch (const std::invalid_argument&) {}
    std::printf(bad ? "FAILED\n" : "OK\n");
    return bad;
}
"""


def test_host_plan_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """point_pair_plan.cpp needs no HIP header: compiled with g++ -fsanitize=address,undefined next to a main of its own,
    which builds the plans of the designs and compares them with the numpy plan"""
    data, body = "", ""
    for i, name in enumerate(["A_spd", "B", "Z"]):
        lay = pdz.zero_residual((0, 1.0)) if name == "Z" else pdz.layout(name)
        e, P = lay["e"], lay["n_free"]
        free = ppr.numpy_plan(e["a"], e["b"], e["active"], P)
        rowptr, colind = ppr.pair_pattern(P, free["pair_lo"], free["pair_hi"])
        want = ppr.numpy_plan(e["a"], e["b"], e["active"], P, rowptr, colind)
        data += c_array("int32_t", "a%d" % i, e["a"]) + c_array("int32_t", "b%d" % i, e["b"]) + c_array("uint8_t", "f%d" % i, e["flags"])
        data += c_array("int32_t", "rp%d" % i, rowptr) + c_array("int32_t", "ci%d" % i, colind)
        body += "    cugo_host::build_point_pair_plan(%d, %d, %d, a%d, b%d, f%d, rp%d, ci%d, plan);\n" % (len(e["a"]), lay["P"], P, i, i, i, i, i)
        for k in cugo.PointPairPlan.ARRAYS:
            data += c_array("int32_t", "%s%d" % (k, i), want[k])
            body += '    bad += check("%s %s", plan.%s, %s%d, %d);\n' % (name, k, k, k, i, len(want[k]))
    src = tmp_path / "plan_main.cpp"
    src.write_text("#include <cstdint>\n" + data + PLAN_MAIN.replace("@BODY@", body))
    exe = tmp_path / "plan_main"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", HOST, str(src), os.path.join(HOST, "point_pair_plan.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr[-3000:]
