#pragma once
#include "../kernels/kernels.h"
#include "chol_symbolic.h"
#include "hip_util.h"
#include "options.h"

#include <array>
#include <functional>
#include <memory>

// definition of the opaque cugo_chol of include/cugo_hip.h
struct cugo_chol
{
    cugo_ctx* ctx = nullptr;
    bool analyzed = false;
    cugo_host::Options opt = cugo_host::Options::from_env(); // the environment switches, read once when the solver is created
    cugo_host::CholPlan plan;
    std::vector<int32_t> trans32; // blk_trans widened for cugo_chol_plan_array
    std::vector<int32_t> asm_info; // (cugo_chol_plan_array)
    std::vector<int32_t> ea1;      // the child link records of CholPlanDev::ea1 (pack; cugo_chol_plan_array)
    cugo_k::CholPlanDev dev{};
    size_t lds_factor = 0, lds_backward = 0;
    // CUGO_LOOKAHEAD=1 at analyze(): the bulk of a level's update matrix is computed while the next level
    // factors (k_up_potrf_la / k_up_lead).  Measured slower than the level-synchronous default on MI355X
    // (kitti_00 shape: 17.5 vs 14.7 ms per step, profiles/r02_lookahead_timeline.txt): the lead workgroup
    // that the next potrf waits for costs as much as a whole single-round tile launch.  Kept under test.
    bool lookahead = false;
    bool asm_fronts = true; // one assembly launch that writes every entry (k_assemble_fronts) instead of clear + scatter

    // the plan's index arrays, packed (chol_solver.cpp: upload)
    std::vector<int32_t> pack32;
    std::vector<int64_t> pack64;
    std::array<size_t, 32> po{}; // offsets of the arrays inside the packs (pack)
    cugo_host::DevBuf<int32_t> d_pack32;
    cugo_host::DevBuf<int64_t> d_pack64;
    const int32_t* d_wl_ptr = nullptr; // work-item triples inside d_pack32
    cugo_host::DevBuf<double> d_fronts, d_xnew, d_junk, d_winv, d_l21;
    // the backward pass in one launch (k_backward_chain; CUGO_BW_CHAIN=0 or a plan it does not cover: one launch per
    // stage): its device words (kernels.h: BC_HEAD ..., zeroed once in upload()), the pinned word the kernel sets
    // when a wait runs into its time bound, what the ticket head holds before the next launch, the last epoch
    bool bw_chain = false;
    cugo_host::DevBuf<uint32_t> d_bc_state;
    cugo_host::PinnedBuf<uint32_t> h_bc_error;
    uint32_t bc_base = 0, bc_epoch = 0;
    void check_chain_error(); // throws if an earlier call's k_backward_chain gave up

    // rank-owned elimination subtrees of a landmark-sharded run (CholPlan::owner): this rank factors its own
    // subtrees and the replicated top; update blocks that enter the top and the solution of the other ranks'
    // subtrees arrive by `bcast(device pointer, doubles, root rank)` on the solver's stream
    int rank = 0, world = 1;
    std::function<void(double*, size_t, int)> bcast;
    std::function<void(bool)> bcast_group; // brackets the broadcasts that may be fused into one operation
    ~cugo_chol();
#ifdef CUGO_DEBUG_HOOKS // ---- diagnosis, only in libcugo_hip_hooks.so (make HOOKS=1) ----
    // diagnosis (CUGO_DEBUG_HASH): 64 checksum slots of the factorisation being queued, or null —
    // 11 fronts after the assembly, 12 / 13 / 14 W, L21, fronts after the forward pass, 15 x after the backward pass,
    // 16 + st: W after the potrf launch of stage st, 40 + st: the fronts after the tile launches of stage st
    unsigned long long* dbg_hash = nullptr;
    int dbg_calls = 0; // factor_solve calls so far (CUGO_DEBUG_SKIP counts them)
    // diagnosis (CUGO_DEBUG_KEEP=1): after every one of the first 16 factor_solve calls the fronts, W, L21, x (permuted)
    // and x are copied (same stream) into a slot of their own; cugo_debug_dump() writes the slots of the solver that
    // ran last to files — the autopsy of a run that deviated from its twin (tools/autopsy.py)
    std::vector<std::unique_ptr<cugo_host::DevBuf<double>>> keep;
    cugo_host::DevBuf<double> dbg_scratch; // (CUGO_DEBUG_STALE: the other version of the line under test)
    void dump_kept(const char* dir);
    void dump_slot(int call, const char* path);
#endif
    bool own_subtrees() const { return bcast && plan.owned; }

    // selected inverse (cugo_chol_selected_inverse): the zero-pivot flag of the last factor_solve, whether one ran
    // since analyze(), and — built on the first call after analyze() — the Sigma-fronts (laid out like the fronts),
    // per front {offset and leading dimension of the parent's Sigma-front, offset of its rel list, copy S_RR}, and
    // per upper stage the (front, first row) items of the 64-row tiles of R
    const int32_t* last_fail = nullptr;
    bool factored = false;
    bool si_ready = false;
    cugo_host::DevBuf<double> d_sig;
    cugo_host::DevBuf<int64_t> d_sinfo;
    cugo_host::DevBuf<int32_t> d_sitems;
    std::vector<int32_t> si_ptr; // [n_stages+1] item ranges
    // false: the zero-pivot flag of the last factorisation is set (nothing queued)
    bool selected_inverse(double* d_sigma);

    // blocks of the inverse for arbitrary pairs (cugo_chol_inverse_blocks): h_rows / h_cols in the caller's numbering,
    // d_out [n_pairs][36].  The distinct rows of a batch of pairs each take a [6 n][6] workspace (at most
    // XCOV_WS_BYTES in all, or CUGO_XCOV_BATCH rows); sparent goes to the device on the first call after analyze().
    // false: the zero-pivot flag of the last factorisation is set (nothing queued)
    static constexpr size_t XCOV_WS_BYTES = size_t(512) << 20;
    bool xc_ready = false;
    cugo_host::DevBuf<int32_t> d_sparent, d_xc_meta;
    cugo_host::DevBuf<double> d_xc_ws;
    std::vector<int32_t> xc_meta, xc_slot; // the batches' row and pair lists (kept until the next call: the copy reads it)
    bool inverse_blocks(int n_pairs, const int32_t* h_rows, const int32_t* h_cols, double* d_out);

    void analyze(int n, const int32_t* rowptr, const int32_t* colind);
    void analyze_host(int n, const int32_t* rowptr, const int32_t* colind); // without upload()
    void pack(); // host half of upload() (analyze_host calls it)
    void upload(hipStream_t s);
    void factor_solve(const double* d_Hsc, double lambda, const double* d_bsc, double* d_x,
                      int32_t* d_fail);
};

#ifdef CUGO_DEBUG_HOOKS
// diagnosis: writes the CUGO_DEBUG_KEEP slots of the solver that ran last to dir/call<k>.bin; returns their number
int cugo_debug_dump_last_solver(const char* dir);
cugo_chol* cugo_debug_solver(int which); // 0: the solver that ran last with CUGO_DEBUG_KEEP, 1: the pinned one
void cugo_debug_pin_reference_solver();
#endif
