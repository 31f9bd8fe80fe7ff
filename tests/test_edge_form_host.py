"""CPU test of the one classification of an edge view (no GPU): the truth table of cugo_k::edge_form() and of the check
the kernel-level entries run before they launch anything (c_api.cpp: check_edge_form), from a stand-alone C++ program
linked against the library.  Every combination gives its form, or the exact refusal the entries have always given."""
import importlib
import os
import subprocess

cugo = importlib.import_module("cuda-bundle-adjustment_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")

PROGRAM = r"""
#include "cugo_hip.h"
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <string>
// the library's internal names (csrc/kernels/kernels.h, csrc/host/c_api.cpp); PUBLIC_ONLY: only what cugo_hip.h declares
#ifndef PUBLIC_ONLY
namespace cugo_k
{
enum class EdgeForm { Plain, Depth, Rig, Models };
EdgeForm edge_form(const cugo_edges& ev);
}
namespace cugo_host
{
void check_edge_form(const cugo_edges* ev, const char* who);
}
#endif
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #c, what.c_str()); return 1; } } while (0)
int main()
{
    static const double table[17] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0}; // (a host address: never read)
    const int rigs[4] = {0, 1, 2, 7};
    const double weights[4] = {0.0, -2.0, std::nan(""), 2.0};
    // {rk_type_depth, rk_delta_depth}: none, Huber, out of range above and below, Huber with a delta that is not > 0
    const struct { int type; double delta; bool ok; } rks[5] = {{CUGO_RK_NONE, 0.0, true}, {CUGO_RK_HUBER, 1.5, true},
                                                               {9, 1.0, false}, {-1, 1.0, false}, {CUGO_RK_HUBER, 0.0, false}};
    int n_forms = 0, n_refused = 0;
    for (int rig : rigs)
        for (int depth = 0; depth < 2; depth++)
            for (int given = 0; given < 2; given++)
                for (int iw = 0; iw < 4; iw++)
                    for (const auto& rk : rks)
                    {
                        cugo_edges ev = {};
                        ev.has_rig = rig, ev.has_depth = depth, ev.d_cam_ext = given ? table : nullptr;
                        ev.depth_weight = weights[iw], ev.rk_type_depth = rk.type, ev.rk_delta_depth = rk.delta;
                        std::string what = "has_rig " + std::to_string(rig) + " has_depth " + std::to_string(depth) + " table " +
                                           std::to_string(given) + " weight " + std::to_string(iw) + " rk " + std::to_string(rk.type);
                        // what the entries have always said, and in which order
                        std::string refusal;
                        if (rig && !given)
                            refusal = ": has_rig needs the extrinsics table d_cam_ext";
                        else if (rig && depth)
                            refusal = ": camera extrinsics (has_rig) together with depth slots (has_depth) are not supported yet";
                        else if (depth && iw != 3)
                            refusal = ": depth_weight must be finite and > 0 with has_depth";
                        else if (depth && !rk.ok)
                            refusal = ": unknown robust kernel or bad delta of the depth kind";
#ifndef PUBLIC_ONLY
                        // any non-zero has_rig other than CUGO_RIG_MODELS means extrinsics; a table wins over depth slots
                        const cugo_k::EdgeForm form = rig == CUGO_RIG_MODELS ? cugo_k::EdgeForm::Models
                                                      : rig                  ? cugo_k::EdgeForm::Rig
                                                      : depth                ? cugo_k::EdgeForm::Depth
                                                                             : cugo_k::EdgeForm::Plain;
                        CHECK(cugo_k::edge_form(ev) == form);
                        std::string got;
                        try { cugo_host::check_edge_form(&ev, "who"); }
                        catch (const std::runtime_error& e) { got = e.what(); }
                        CHECK(got == (refusal.empty() ? "" : "who" + refusal));
#endif
                        if (refusal.empty())
                        {
                            n_forms++;
                            continue;
                        }
                        // a refused view never reaches the context or the device: CUGO_ERR_INVALID before anything is launched
                        n_refused++;
                        const cugo_robust none = {};
                        CHECK(cugo_compute_active_errors(nullptr, &ev, nullptr, nullptr, none, nullptr) == CUGO_ERR_INVALID);
                        what += std::string(" -> ") + cugo_last_error();
                        CHECK(cugo_last_error() == "cugo_compute_active_errors" + refusal);
                    }
#ifndef PUBLIC_ONLY
    try { cugo_host::check_edge_form(nullptr, "who"); } // (no view: nothing to check)
    catch (const std::runtime_error&) { std::printf("FAILED: a null view was refused\n"); return 1; }
#endif
    std::printf("OK %d forms %d refusals\n", n_forms, n_refused);
    return 0;
}
"""


def test_edge_form_and_its_check_cover_the_truth_table(tmp_path):
    src = tmp_path / "edge_form_caller.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "edge_form_caller"
    lib_dir = os.path.dirname(cugo.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", INC, str(src), "-L", lib_dir, "-lcugo_hip",
                        "-Wl,-rpath," + lib_dir, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    # 4 x 2 x 2 x 4 x 5 = 320 views.  has_rig 0, table or not: 2 x 20 plain, 2 x 2 depth (the good weight with the two
    # good kernels); every has_rig != 0 with a table and without depth: 3 x 20
    assert "OK 104 forms 216 refusals" in r.stdout, r.stdout
