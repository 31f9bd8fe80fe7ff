// Pose-pose point edges (include/cugo_hip.h: cugo_point_pair_edges; an extension, the reference has no such edge): a
// point p measured in pose a's frame, the same physical point measured as z in pose b's frame, a 3 x 3 information matrix
// Omega in b's frame (symmetric positive SEMI-definite, its upper triangle row-major packed, [6][n] or [6][1]).
// Conventions as for the unary point kind (point_kernels.hip): y = R(q) X + t, left update, tangent order [omega, upsilon].
//   X = R_a^T (p - t_a),  y = R_b X + t_b,  r = y - z,  x = max(0, r^T Omega r),  chi2 term rho(x),  w = rho'(x)
//   J_b = [ S_y | I ],  S_u = -[u]x            (the unary point edge's Jacobian)
//   J_a = M [ [p]x | -I ] = -M [ S_p | I ],    M = R_BA = R_b R_a^T
// With N = M^T Omega, Omega' = N M (Omega seen from a's frame) and q = Omega r, q' = M^T q:
//   H_bb = w [S_y | I]^T Omega  [S_y | I],   b_b = -w (y x q, q)        the unary term at (y, Omega)
//   H_aa = w [S_p | I]^T Omega' [S_p | I],   b_a = +w (p x q', q')      the unary term at (p, Omega'), b with the other sign
//   H_ab = w J_a^T Omega J_b = -w [ [p]x W ; W ],  W = N [S_y | I] = [ N S_y | N ]     (3 x 6; rows a, columns b)
// With T_a the identity M = I, Omega' = Omega and the term on b is the unary point edge (p, z, Omega), term for term.
//
// The covariance form (include/cugo_hip.h: cugo_gicp_pair_edges; point_term.h): Omega = (C_z + M C_p M^T)^-1 formed at
// the poses the pass is given, from cov_p (a's frame) and cov_z (b's frame).  Every role and the error pass form M and
// Omega first, from the same inputs in the same operation order, and continue as above.  It is an instantiation of its
// own of the chunk kernels (k_gicp_pair_chunks_*); the information form's kernels carry no branch for it.
//
// Invariants (the project's own for every pose kind):
//   - no atomics and no summation order that depends on the schedule: one fixed order;
//   - the error pass forms the chunk and (chunk, run) chi2 totals of the build pass bit for bit;
//   - a pose without a counting run and a pattern block without a counting run keep the bits they had;
//   - fixed ends are never written.
//
// Layout and reduction.  The plan (csrc/host/point_pair_plan.h) sorts the edges into RUNS of one (a, b) orientation of a
// pair; the runs of one block are adjacent.  One wave per chunk of ICP_CHUNK sorted edges walks its edges in groups of 64
// lanes; the lanes of each run in turn join the wave's accumulators, which are reduced (icp_wave_reduce32) and stored
// whenever a later run begins and at the chunk's end — the chunk scheme of pose_chunks.h, keyed by run.  An edge
// feeds 27 + 27 + 36 sums; instead of 90 accumulators per lane the launch has four ROLES (blockIdx.y), each of which
// recomputes the edge and keeps at most 27 sums under static indices:
//   role 0  self-a: H_aa (21) + b_a (6), and the chi2 of the edge     role 2  H_ab columns 0-2 (18)
//   role 1  self-b: H_bb (21) + b_b (6)                               role 3  H_ab columns 3-5 (18)
// A role stores an ICP_NP-wide partial at slot (role, chunk + run): chunk + run is unique because both ascend.  A role
// whose destination does not exist for an edge (a fixed end's block; the off-diagonal of a run with a fixed end) skips
// the arithmetic and stores zeros that nothing reads.  The error pass is role 0 alone without the H arithmetic: it
// writes element 27 of its slots and the chunk totals, never elements 0-26, so the build partials survive it.
// Finishing, fixed order: 32 threads per free pose sum the pose's (run, side) partials in incidence order, then chunk
// order, and ADD them to Hpp / bp or the Schur destination (pose_term_add); 64 threads per touched block sum its runs'
// off-diagonal partials, runs ascending, then chunk order, transposing a run whose a is hi, and ADD them to the block.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdexcept>

#include "point_term.h"
#include "pose_chunks.h"

namespace
{

using namespace cugo_dev;

constexpr int RUN_A_FREE = 1, RUN_B_FREE = 2, RUN_A_IS_HI = 4, RUN_COUNTS = 8; // (point_pair_plan.h: PAIR_RUN_*)
constexpr int N_ROLES = 4;

struct PairArgs
{
    static constexpr bool COV = false;
    int n;
    const int32_t *pose_a, *pose_b; // [n] sorted order
    const double* p;                // [3][n]
    const double* z;                // [3][n]
    const double* info;             // [6][n] or [6][1]
    int n_info;
    const uint8_t* flags;
    Robust rk;
    cugo_k::PointPairPlanDev plan;
    double* part; // [N_ROLES][n_chunks + n_runs][ICP_NP]
    double* cchi; // [n_chunks] chi2 total of every chunk
    const double* poses;
    double* edge_chi; // error pass: [n] or nullptr
};
// the covariance form: info is cov_p [6][n_info], n_info the count of both covariances
struct GicpPairArgs : PairArgs
{
    static constexpr bool COV = true;
    const double* cov_z; // [6][n] or [6][1]
};

// M = R_b R_a^T
__device__ __forceinline__ void pair_rotation(const double (&Ra)[3][3], const double (&Rb)[3][3], double (&M)[3][3])
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            M[i][j] = Rb[i][0] * Ra[j][0] + Rb[i][1] * Ra[j][1] + Rb[i][2] * Ra[j][2];
}

__device__ __forceinline__ size_t pair_slots(const PairArgs& k) { return ChunkLayout(k.n, k.plan.n_runs).slots; }

// Edge e between poses a and b, seen by `role`.  Returns the chi2 term.  FULL and term: v[0..26] receive the role's
// contribution (roles 2 and 3: v[6 c + i] = H_ab[i][3 (role - 2) + c], 18 values); FULL without term: zeros
template <bool FULL, int role, class K>
__device__ __forceinline__ double pair_edge(const K& k, int e, int a, int b, bool term, double (&v)[32])
{
    const size_t n = (size_t)k.n;
    const double* __restrict__ pa = k.poses + 7 * (size_t)a;
    const double* __restrict__ pb = k.poses + 7 * (size_t)b;
    const double pp[3] = {k.p[e], k.p[n + e], k.p[2 * n + e]};
    double Ra[3][3], Rb[3][3];
    quat_to_rot(pa, Ra);
    quat_to_rot(pb, Rb);
    const double d[3] = {pp[0] - pa[4], pp[1] - pa[5], pp[2] - pa[6]};
    double X[3], y[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
        X[i] = Ra[0][i] * d[0] + Ra[1][i] * d[1] + Ra[2][i] * d[2];
#pragma unroll
    for (int i = 0; i < 3; i++)
        y[i] = Rb[i][0] * X[0] + Rb[i][1] * X[1] + Rb[i][2] * X[2] + pb[4 + i];
    const double z[3] = {k.z[e], k.z[n + e], k.z[2 * n + e]};
    double O[3][3], q[3], x; // Omega, Omega r
    double Mc[3][3]; // R_b R_a^T of the covariance form, which needs it for Omega in every role
    double chi;
    if constexpr (K::COV)
    {
        pair_rotation(Ra, Rb, Mc);
        chi = point_residual<true>(y, z, k.info, k.n_info, n, e, k.rk, O, q, x, k.cov_z, &Mc);
    }
    else
        chi = point_residual(y, z, k.info, k.n_info, n, e, k.rk, O, q, x);
    if (FULL)
    {
        chunk_zero(v);
        if (term)
        {
            const double w = rk_drho(k.rk, x);
            if (role == 1)
            {
                unary_block(y, O, w, v);
                unary_b(y, q, -w, v);
            }
            else
            {
                double M[3][3], N[3][3]; // M = R_b R_a^T, N = M^T Omega
                if constexpr (K::COV)
                {
#pragma unroll
                    for (int i = 0; i < 3; i++)
#pragma unroll
                        for (int j = 0; j < 3; j++)
                            M[i][j] = Mc[i][j];
                }
                else
                {
#pragma unroll
                    for (int i = 0; i < 3; i++)
#pragma unroll
                        for (int j = 0; j < 3; j++)
                            M[i][j] = Rb[i][0] * Ra[j][0] + Rb[i][1] * Ra[j][1] + Rb[i][2] * Ra[j][2];
                }
#pragma unroll
                for (int i = 0; i < 3; i++)
#pragma unroll
                    for (int j = 0; j < 3; j++)
                        N[i][j] = M[0][i] * O[0][j] + M[1][i] * O[1][j] + M[2][i] * O[2][j];
                if (role == 0)
                {
                    double Op[3][3]; // Omega' = N M, its upper triangle mirrored: exactly symmetric
#pragma unroll
                    for (int i = 0; i < 3; i++)
#pragma unroll
                        for (int j = i; j < 3; j++)
                            Op[i][j] = Op[j][i] = N[i][0] * M[0][j] + N[i][1] * M[1][j] + N[i][2] * M[2][j];
                    double qp[3]; // M^T q
#pragma unroll
                    for (int i = 0; i < 3; i++)
                        qp[i] = M[0][i] * q[0] + M[1][i] * q[1] + M[2][i] * q[2];
                    unary_block(pp, Op, w, v);
                    unary_b(pp, qp, w, v);
                }
                else
                {
                    double W[3][3]; // columns 3 (role - 2) .. + 2 of [ N S_y | N ]
#pragma unroll
                    for (int i = 0; i < 3; i++)
                    {
                        W[i][0] = role == 2 ? N[i][2] * y[1] - N[i][1] * y[2] : N[i][0];
                        W[i][1] = role == 2 ? N[i][0] * y[2] - N[i][2] * y[0] : N[i][1];
                        W[i][2] = role == 2 ? N[i][1] * y[0] - N[i][0] * y[1] : N[i][2];
                    }
#pragma unroll
                    for (int c = 0; c < 3; c++)
                    {
                        v[6 * c + 0] = -(w * (pp[1] * W[2][c] - pp[2] * W[1][c]));
                        v[6 * c + 1] = -(w * (pp[2] * W[0][c] - pp[0] * W[2][c]));
                        v[6 * c + 2] = -(w * (pp[0] * W[1][c] - pp[1] * W[0][c]));
                        v[6 * c + 3] = -(w * W[0][c]);
                        v[6 * c + 4] = -(w * W[1][c]);
                        v[6 * c + 5] = -(w * W[2][c]);
                    }
                }
            }
        }
    }
    return chi;
}

// One wave per (chunk of ICP_CHUNK sorted edges, role): pose_chunks.h's chunk_walk keyed by run, on the role's part of
// the partials.  FULL: the role's partials, role 0 also chi2; otherwise (role 0 alone is launched) chi2 only: element 27
// of role 0's slots, the chunk total and, with edge_chi, the chi2 term of every edge.
template <bool FULL, int role, class K>
__device__ __forceinline__ void pair_chunks(const K& k)
{
    const int c = (int)((blockIdx.x * (size_t)ICP_WG + threadIdx.x) >> 6);
    if (c >= chunk_count(k.n))
        return;
    double* const part = k.part + (size_t)role * pair_slots(k) * ICP_NP;
    chunk_walk<FULL, role == 0, true>(k.n, k.plan.edge_run, c, part, k.cchi, k.edge_chi, [&](int e, bool in, int r, double (&v)[32]) {
        const int f = in ? k.plan.run_flags[r] : 0;
        const bool live = (f & RUN_COUNTS) && !(k.flags && (k.flags[e] & CUGO_EDGE_INACTIVE));
        // the role's destination exists: a free end's own block; the off-diagonal block of two free ends
        const int need = role == 0 ? RUN_A_FREE : role == 1 ? RUN_B_FREE : (RUN_A_FREE | RUN_B_FREE);
        const bool term = live && (f & need) == need;
        if (FULL ? term || (role == 0 && live) : live)
            return pair_edge<FULL, role>(k, e, k.pose_a[e], k.pose_b[e], term, v);
        if (FULL)
            chunk_zero(v);
        return 0.0;
    });
}

// the role is blockIdx.y (uniform over the workgroup); every role is an instantiation of its own, so that the kernel's
// registers are those of its largest role and not of the four together
__global__ __launch_bounds__(ICP_WG) void k_point_pair_chunks_build(PairArgs a)
{
    switch (blockIdx.y)
    {
    case 0: pair_chunks<true, 0>(a); break;
    case 1: pair_chunks<true, 1>(a); break;
    case 2: pair_chunks<true, 2>(a); break;
    default: pair_chunks<true, 3>(a); break;
    }
}
__global__ __launch_bounds__(ICP_WG) void k_point_pair_chunks_errors(PairArgs a) { pair_chunks<false, 0>(a); }
// the covariance form
__global__ __launch_bounds__(ICP_WG) void k_gicp_pair_chunks_build(GicpPairArgs a)
{
    switch (blockIdx.y)
    {
    case 0: pair_chunks<true, 0>(a); break;
    case 1: pair_chunks<true, 1>(a); break;
    case 2: pair_chunks<true, 2>(a); break;
    default: pair_chunks<true, 3>(a); break;
    }
}
__global__ __launch_bounds__(ICP_WG) void k_gicp_pair_chunks_errors(GicpPairArgs a) { pair_chunks<false, 0>(a); }

// element t of run r's partials of `role`, summed in chunk order
__device__ __forceinline__ double run_sum(const PairArgs& k, int role, int r, int t)
{
    return chunk_key_sum<false>(k.plan.run_ptr, k.part + (size_t)role * pair_slots(k) * ICP_NP, r, t);
}

// the finishing pass (pose_chunks.h: chunk_finish) over the free poses with an incidence: a pose's sum runs over its
// (run, side) entries in incidence order, each over its chunks in order
template <bool SCHUR>
__global__ __launch_bounds__(ICP_WG) void k_point_pair_finish(PairArgs a, double* __restrict__ H, const int32_t* __restrict__ rowptr,
                                                               double* __restrict__ bp, double* __restrict__ bsc)
{
    chunk_finish<SCHUR>(
        a.plan.n_poses_free, [&](int p) { return a.plan.inc_ptr[p] != a.plan.inc_ptr[p + 1]; },
        [&](int p, int t) {
            double s = 0.0;
            for (int j = a.plan.inc_ptr[p], j1 = a.plan.inc_ptr[p + 1]; j < j1; j++)
            {
                const int rs = a.plan.inc[j];
                s += run_sum(a, rs & 1, rs >> 1, t);
            }
            return s;
        },
        H, rowptr, bp, bsc);
}

// 64 threads per touched block; thread t < 36 adds element t (column-major: row t % 6 of pose lo, column t / 6 of pose
// hi) of the block's sum — its runs ascending, each over its chunks in order — to block blk_id of H.  A run whose a is
// hi holds H_ab = H_(hi,lo): its element (row, col) is read at (col, row)
__global__ __launch_bounds__(ICP_WG) void k_point_pair_offdiag(PairArgs a, double* __restrict__ H)
{
    const int k = (int)((blockIdx.x * (size_t)ICP_WG + threadIdx.x) >> 6), t = threadIdx.x & 63;
    if (k >= a.plan.n_blocks || t >= 36)
        return;
    const int row = t % 6, col = t / 6;
    double s = 0.0;
    for (int j = a.plan.blk_ptr[k], j1 = a.plan.blk_ptr[k + 1]; j < j1; j++)
    {
        const int r = a.plan.blk_run[j];
        const bool tr = (a.plan.run_flags[r] & RUN_A_IS_HI) != 0;
        const int i = tr ? col : row, cc = tr ? row : col; // element (i, cc) of H_ab
        s += run_sum(a, 2 + cc / 3, r, 6 * (cc % 3) + i);
    }
    H[36 * (size_t)a.plan.blk_id[k] + t] += s;
}

// every edge's (a, b) is its run's, and its run is the one whose range holds it.  Offending threads write 1
__global__ __launch_bounds__(ICP_WG) void k_point_pair_check(const int32_t* __restrict__ pose_a, const int32_t* __restrict__ pose_b,
                                                              cugo_k::PointPairPlanDev plan, int* __restrict__ bad)
{
    for (int i = blockIdx.x * ICP_WG + threadIdx.x; i < plan.n; i += gridDim.x * ICP_WG)
    {
        const int r = plan.edge_run[i];
        if (pose_a[i] != plan.run_a[r] || pose_b[i] != plan.run_b[r])
            bad[0] = 1;
    }
}

PairArgs args_of(const cugo_point_pair_edges& ev, const cugo_k::PointPairPlanDev& plan, const double* d_poses,
                 cugo_k::ChunkScratch ps, double* d_edge_chi)
{
    return PairArgs{ev.n,      ev.d_pose_a, ev.d_pose_b,          ev.d_p, ev.d_z,    ev.d_info, ev.n_info,
                    ev.d_flags, Robust{ev.rk, ev.delta}, plan, ps.d_part, ps.d_cchi, d_poses,   d_edge_chi};
}

} // namespace

namespace cugo_k
{

size_t point_pair_scratch_doubles(int n, int n_runs) { return ChunkLayout(n, n_runs, N_ROLES).end; }
size_t point_pair_partial_doubles(int n, int n_runs) { return ChunkLayout(n, n_runs, N_ROLES).cchi; }
int point_pair_chunk_count(int n) { return chunk_count(n); }

ChunkScratch point_pair_scratch_in(ReduceScratch rs, int n, int n_runs)
{
    const ChunkLayout lay(n, n_runs, N_ROLES);
    return chunk_scratch_in(rs, lay.cchi, lay.end, "point pair edge");
}

int point_pair_check_indices(hipStream_t s, const cugo_point_pair_edges& ev, const PointPairPlanDev& plan, int* d_bad)
{
    if (hipMemsetAsync(d_bad, 0, sizeof(int), s) != hipSuccess)
        throw std::runtime_error("cugo: hipMemsetAsync failed");
    if (plan.n > 0)
    {
        const unsigned grid = (unsigned)std::min<size_t>(1024, ((size_t)plan.n + ICP_WG - 1) / ICP_WG);
        CUGO_LAUNCH(k_point_pair_check, dim3(grid), dim3(ICP_WG), 0, s, ev.d_pose_a, ev.d_pose_b, plan, d_bad);
    }
    int bad = 0;
    if (hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        throw std::runtime_error("cugo: point pair index check failed to run");
    return bad;
}

void launch_point_pair_chunks(hipStream_t s, const cugo_point_pair_edges& ev, const PointPairPlanDev& plan, const double* d_poses,
                              bool full, ChunkScratch rs, double* d_edge_chi, const double* d_cov_z)
{
    const size_t waves = (size_t)chunk_count(ev.n);
    if (waves == 0)
        return;
    const PairArgs a = args_of(ev, plan, d_poses, rs, full ? nullptr : d_edge_chi);
    const unsigned grid = chunk_grid(waves);
    if (d_cov_z)
    {
        const GicpPairArgs g{a, d_cov_z};
        if (full)
            CUGO_LAUNCH(k_gicp_pair_chunks_build, dim3(grid, N_ROLES), dim3(ICP_WG), 0, s, g);
        else
            CUGO_LAUNCH(k_gicp_pair_chunks_errors, dim3(grid), dim3(ICP_WG), 0, s, g);
    }
    else if (full)
        CUGO_LAUNCH(k_point_pair_chunks_build, dim3(grid, N_ROLES), dim3(ICP_WG), 0, s, a);
    else
        CUGO_LAUNCH(k_point_pair_chunks_errors, dim3(grid), dim3(ICP_WG), 0, s, a);
}

static void launch_finish(hipStream_t s, const char* label, bool schur, const cugo_point_pair_edges& ev, const PointPairPlanDev& plan,
                          ChunkScratch rs, double* d_H, const int32_t* d_rowptr, double* d_bp, double* d_bsc)
{
    if (plan.n_poses_free <= 0 || ev.n == 0)
        return;
    const PairArgs a = args_of(ev, plan, nullptr, rs, nullptr);
    const unsigned grid = finish_grid(plan.n_poses_free);
    LaunchScope scope(label, s);
    if (schur)
        hipLaunchKernelGGL(k_point_pair_finish<true>, dim3(grid), dim3(ICP_WG), 0, s, a, d_H, d_rowptr, d_bp, d_bsc);
    else
        hipLaunchKernelGGL(k_point_pair_finish<false>, dim3(grid), dim3(ICP_WG), 0, s, a, d_H, d_rowptr, d_bp, d_bsc);
}

void launch_point_pair_add_diag(hipStream_t s, const cugo_point_pair_edges& ev, const PointPairPlanDev& plan, ChunkScratch rs,
                                double* d_Hpp, double* d_bp)
{
    launch_finish(s, "k_point_pair_add", false, ev, plan, rs, d_Hpp, nullptr, d_bp, nullptr);
}

void launch_point_pair_add_diag_schur(hipStream_t s, const cugo_point_pair_edges& ev, const PointPairPlanDev& plan,
                                      ChunkScratch rs, const int32_t* d_rowptr, double* d_Hsc, double* d_bp, double* d_bsc)
{
    launch_finish(s, "k_point_pair_add_schur", true, ev, plan, rs, d_Hsc, d_rowptr, d_bp, d_bsc);
}

void launch_point_pair_add_offdiag(hipStream_t s, const cugo_point_pair_edges& ev, const PointPairPlanDev& plan, ChunkScratch rs,
                                   double* d_H)
{
    if (plan.n_blocks <= 0 || ev.n == 0)
        return;
    const PairArgs a = args_of(ev, plan, nullptr, rs, nullptr);
    const unsigned grid = (unsigned)((64 * (size_t)plan.n_blocks + ICP_WG - 1) / ICP_WG);
    CUGO_LAUNCH(k_point_pair_offdiag, dim3(grid), dim3(ICP_WG), 0, s, a, d_H);
}

void launch_point_pair_add(hipStream_t s, const cugo_point_pair_edges& ev, const PointPairPlanDev& plan, ChunkScratch rs,
                           double* d_Hpp, double* d_bp, double* d_Hoff)
{
    launch_point_pair_add_diag(s, ev, plan, rs, d_Hpp, d_bp);
    if (d_Hoff)
        launch_point_pair_add_offdiag(s, ev, plan, rs, d_Hoff);
}

void launch_point_pair_add_schur(hipStream_t s, const cugo_point_pair_edges& ev, const PointPairPlanDev& plan, ChunkScratch rs,
                                 const int32_t* d_rowptr, double* d_Hsc, double* d_bp, double* d_bsc)
{
    launch_point_pair_add_diag_schur(s, ev, plan, rs, d_rowptr, d_Hsc, d_bp, d_bsc);
    launch_point_pair_add_offdiag(s, ev, plan, rs, d_Hsc);
}

void launch_point_pair_chi_total(hipStream_t s, const cugo_point_pair_edges& ev, ChunkScratch rs, double* d_chi, bool chi_add)
{
    launch_pose_chi_total(s, "k_point_pair_chi_total", rs.d_cchi, point_pair_chunk_count(ev.n), d_chi, chi_add);
}

} // namespace cugo_k
