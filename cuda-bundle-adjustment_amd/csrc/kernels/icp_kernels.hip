// Point-to-plane and point-to-line pose edges (the reference's include/icp_types.h): unary edges on a pose vertex.
// y = R(q) p + t is read as BA reads a pose (ba_math.h world_to_cam); the update is the left update in the tangent
// order [omega, upsilon], so dy/dxi = [ -[y]x | I ].
//   plane: r = n.y - d (scalar),            J = [ y x n | n^T ]          (1 x 6)
//   line:  r = P (y - a), P = I - u u^T,    J = P [ -[y]x | I ]          (3 x 6; |r| is the distance to the line)
// chi2 term rho(omega |r|^2), weight w = omega rho'(omega |r|^2); H += w J^T J, b -= w J^T r.  The minus is the BA
// build pass's convention: its Jacobian is d(meas - proj)/dxi = -de/dxi (ba_math.h jac_pose), so its bp is minus half
// the gradient of chi2, the solver takes H dx = b and the update applies exp(+dx) (k_backsubst_poses).  Edges on fixed
// poses (index >= n_poses_free) and inactive edges contribute nothing.
//
// Layout and reduction (no atomics, one fixed order):  each kind's edges are sorted by pose index.  The edge range
// is cut into chunks of ICP_CHUNK edges regardless of pose boundaries, one wave per chunk; a chunk writes one partial
// of 28 doubles (21 of the upper triangle of H, 6 of b, chi2) per pose it touches.  Chunk c and pose p meet in at
// most one partial, and along the sorted edges c and p never decrease and one of them grows at each step from one
// (chunk, pose) pair to the next: c + p is therefore a unique slot index — no prefix sums, no plan.  The finishing
// pass sums a pose's partials in chunk order (plane kind, then line kind) and adds them to Hpp / bp or, behind
// k_pose_schur in the one-stream form of the LM loop, to the pose's diagonal block of Hsc, to bp and to bsc.  Every
// chunk also leaves ONE chi2 total (its partials in the order it wrote them); the chi2 total of the pass is the sum of
// the chunk totals — plane chunks, then line chunks: a plain array that the reduction ending an LM trial sums next to
// the BA partials (ba_kernels.hip: k_sum_partials2).  The error pass forms the very same chunk totals, so its total
// has the bits of the build pass's.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <stdexcept>

#include "ba_math.h"
#include "kernels.h"
#include "pose_chunks.h"

namespace
{

using namespace cugo_dev;

struct IcpKind
{
    int n;
    const int32_t* pose;
    const int32_t* pose_ptr;
    const double* p;   // [3][n]
    const double* geo; // plane: [4][n] n, d; line: [6][n] a, u
    const double* omega;
    int n_omega;
    const uint8_t* flags;
    Robust rk;
    double* part; // [n_chunks + n_poses_total][ICP_NP]
    double* cchi; // [n_chunks] chi2 total of every chunk
};

__device__ __forceinline__ int n_chunks(int n) { return (n + ICP_CHUNK - 1) / ICP_CHUNK; }

// contribution of edge e of one kind: v[0..20] upper triangle of w J^T J (row-major packed), v[21..26] -w J^T r;
// returns the chi2 term
template <bool LINE, bool FULL>
__device__ __forceinline__ double icp_edge(const IcpKind& k, int e, const double* __restrict__ pose, double (&v)[32])
{
    const int n = k.n;
    const double pp[3] = {k.p[e], k.p[n + e], k.p[2 * (size_t)n + e]};
    double y[3];
    world_to_cam(pose, pp, y);
    double r[3], J[3][6];
    double sq;
    if (!LINE)
    {
        const double nx = k.geo[e], ny = k.geo[n + e], nz = k.geo[2 * (size_t)n + e], d = k.geo[3 * (size_t)n + e];
        r[0] = nx * y[0] + ny * y[1] + nz * y[2] - d;
        sq = r[0] * r[0];
        // y x n
        J[0][0] = y[1] * nz - y[2] * ny;
        J[0][1] = y[2] * nx - y[0] * nz;
        J[0][2] = y[0] * ny - y[1] * nx;
        J[0][3] = nx, J[0][4] = ny, J[0][5] = nz;
    }
    else
    {
        const double a[3] = {k.geo[e], k.geo[n + e], k.geo[2 * (size_t)n + e]};
        const double u[3] = {k.geo[3 * (size_t)n + e], k.geo[4 * (size_t)n + e], k.geo[5 * (size_t)n + e]};
        const double dv[3] = {y[0] - a[0], y[1] - a[1], y[2] - a[2]};
        const double ud = u[0] * dv[0] + u[1] * dv[1] + u[2] * dv[2];
        double P[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++)
        {
#pragma unroll
            for (int j = 0; j < 3; j++)
                P[i][j] = (i == j ? 1.0 : 0.0) - u[i] * u[j];
            r[i] = dv[i] - u[i] * ud;
        }
        sq = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
        // -[y]x columns: (0, -y2, y1), (y2, 0, -y0), (-y1, y0, 0)
        const double S[3][3] = {{0.0, y[2], -y[1]}, {-y[2], 0.0, y[0]}, {y[1], -y[0], 0.0}};
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++)
            {
                J[i][j] = P[i][0] * S[0][j] + P[i][1] * S[1][j] + P[i][2] * S[2][j];
                J[i][3 + j] = P[i][j];
            }
    }
    const double omega = k.omega[k.n_omega == 1 ? 0 : e];
    const double x = omega * sq;
    const double chi = rk_rho(k.rk, x);
    if (FULL)
    {
        const double w = omega * rk_drho(k.rk, x);
        constexpr int R = LINE ? 3 : 1;
        int t = 0;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int c = a; c < 6; c++)
            {
                double s = J[0][a] * J[0][c];
#pragma unroll
                for (int i = 1; i < R; i++)
                    s += J[i][a] * J[i][c];
                v[t++] = w * s;
            }
#pragma unroll
        for (int a = 0; a < 6; a++)
        {
            double s = J[0][a] * r[0];
#pragma unroll
            for (int i = 1; i < R; i++)
                s += J[i][a] * r[i];
            v[21 + a] = -(w * s);
        }
    }
    return chi;
}

// One wave per chunk of ICP_CHUNK edges of one kind.  FULL: partials of H, b and chi2; otherwise chi2 only (slot
// element 27, the same value FULL writes there) and, with edge_chi, the chi2 term of every edge.
template <bool LINE, bool FULL>
__device__ void icp_chunk(const IcpKind& k, int c, int n_poses_free, const double* __restrict__ poses,
                          double* __restrict__ edge_chi)
{
    const int lane = threadIdx.x & 63;
    const int e0 = c * ICP_CHUNK, e1 = min(k.n, e0 + ICP_CHUNK);
    int qcur = k.pose[e0]; // (wave-uniform)
    double acc[32];
#pragma unroll
    for (int i = 0; i < 32; i++)
        acc[i] = 0.0;
    double chi_acc = 0.0, chunk_chi = 0.0;
    auto flush = [&](int q) {
        const double cs = icp_wave_sum(chi_acc);
        chunk_chi += cs; // (the same value in every lane)
        double* out = k.part + (size_t)(c + q) * ICP_NP;
        if (FULL)
        {
            icp_wave_reduce32(acc);
            if (!(lane & 1) && (lane >> 1) < 27)
                out[lane >> 1] = acc[0];
#pragma unroll
            for (int i = 0; i < 32; i++)
                acc[i] = 0.0;
        }
        if (lane == 0)
            out[27] = cs;
        chi_acc = 0.0;
    };
    for (int base = e0; base < e1; base += 64)
    {
        const int e = base + lane;
        const bool in = e < e1;
        const int q = in ? k.pose[e] : INT_MAX;
        double v[32];
        double chi = 0.0;
        if (in && q < n_poses_free && !(k.flags && (k.flags[e] & CUGO_EDGE_INACTIVE)))
            chi = icp_edge<LINE, FULL>(k, e, poses + 7 * (size_t)q, v);
        else if (FULL)
        {
#pragma unroll
            for (int i = 0; i < 27; i++)
                v[i] = 0.0;
        }
        if (!FULL && edge_chi && in)
            edge_chi[e] = chi;
        // the poses of the 64 lanes ascend: the lanes of each pose in turn join the wave's accumulators
        for (;;)
        {
            if (q == qcur)
            {
                chi_acc += chi;
                if (FULL)
                {
#pragma unroll
                    for (int i = 0; i < 27; i++)
                        acc[i] += v[i];
                }
            }
            const unsigned long long later = __ballot(in && q > qcur);
            if (later == 0)
                break;
            const int qn = __shfl(q, __ffsll((long long)later) - 1, 64);
            flush(qcur);
            qcur = qn;
        }
    }
    flush(qcur);
    if (lane == 0)
        k.cchi[c] = chunk_chi;
}

struct IcpArgs
{
    IcpKind plane, line;
    int n_poses_free;
    const double* poses;
    double* edge_chi; // error pass: [n_plane + n_line] or nullptr
};

template <bool FULL>
__device__ __forceinline__ void icp_chunks(const IcpArgs& a)
{
    const int wave = (int)((blockIdx.x * (size_t)ICP_WG + threadIdx.x) >> 6);
    const int cp = n_chunks(a.plane.n), cl = n_chunks(a.line.n);
    if (wave < cp)
        icp_chunk<false, FULL>(a.plane, wave, a.n_poses_free, a.poses, a.edge_chi);
    else if (wave < cp + cl)
        icp_chunk<true, FULL>(a.line, wave - cp, a.n_poses_free, a.poses, a.edge_chi ? a.edge_chi + a.plane.n : nullptr);
}

__global__ __launch_bounds__(ICP_WG) void k_icp_chunks_build(IcpArgs a) { icp_chunks<true>(a); }
// (six waves per SIMD, as before the chunk totals: the pass is bound by the loads it has in flight)
__global__ __launch_bounds__(ICP_WG) __attribute__((amdgpu_waves_per_eu(6))) void k_icp_chunks_errors(IcpArgs a)
{
    icp_chunks<false>(a);
}

// sum of pose p's partials of one kind, element t, in chunk order
__device__ __forceinline__ double icp_pose_sum(const IcpKind& k, int p, int t)
{
    return chunk_pose_sum(k.pose_ptr, k.part, p, t);
}

// 32 threads per free pose that has ICP edges; thread t < 27 adds element t of the pose's sums.  SCHUR = false: to
// Hpp / bp (behind k_build_poses).  SCHUR = true: to the diagonal block of Hsc (the first block of the pose's row,
// through rowptr), to bp and to bsc — behind k_pose_schur, which WRITES the three in the one-stream form of the loop
// (there Hpp is not formed at all; the ICP terms of a pose enter its row of the Schur complement unchanged, as Hpp does)
template <bool SCHUR>
__global__ __launch_bounds__(ICP_WG) void k_icp_finish(IcpArgs a, double* __restrict__ H, const int32_t* __restrict__ rowptr,
                                                        double* __restrict__ bp, double* __restrict__ bsc)
{
    const int p = (int)((blockIdx.x * (size_t)ICP_WG + threadIdx.x) >> 5), t = threadIdx.x & 31;
    if (p >= a.n_poses_free || t >= 27)
        return;
    if (a.plane.pose_ptr[p] == a.plane.pose_ptr[p + 1] && a.line.pose_ptr[p] == a.line.pose_ptr[p + 1])
        return; // (nothing to add: the pose's blocks keep their bits, and its partial slots were never written)
    const double s = icp_pose_sum(a.plane, p, t) + icp_pose_sum(a.line, p, t);
    int r = 0, c = 0;
    if (t < 21)
        tri6_unpack(t, r, c);
    pose_term_add<SCHUR>(p, t, r, c, s, H, rowptr, bp, bsc);
}

// scratch = [plane partials (cp + n_poses_total slots) | line partials (cl + n_poses_total) | chunk totals (cp + cl)]
struct IcpLayout
{
    size_t cp, cl, line_part, cchi, end;
    explicit IcpLayout(const cugo_icp_edges& ev)
    {
        cp = (size_t)(ev.n_plane + ICP_CHUNK - 1) / ICP_CHUNK, cl = (size_t)(ev.n_line + ICP_CHUNK - 1) / ICP_CHUNK;
        line_part = (cp + ev.n_poses_total) * ICP_NP;
        cchi = (cp + cl + 2 * (size_t)ev.n_poses_total) * ICP_NP;
        end = cchi + cp + cl;
    }
};

IcpKind kind_of(const cugo_icp_edges& ev, bool line, double* part, double* cchi)
{
    IcpKind k;
    if (!line)
        k = IcpKind{ev.n_plane, ev.d_plane_pose, ev.d_plane_pose_ptr, ev.d_plane_p, ev.d_plane_nd,
                    ev.d_plane_omega, ev.n_plane_omega, ev.d_plane_flags, Robust{ev.rk_plane, ev.delta_plane}, part, cchi};
    else
        k = IcpKind{ev.n_line, ev.d_line_pose, ev.d_line_pose_ptr, ev.d_line_p, ev.d_line_au,
                    ev.d_line_omega, ev.n_line_omega, ev.d_line_flags, Robust{ev.rk_line, ev.delta_line}, part, cchi};
    return k;
}

IcpArgs args_of(const cugo_icp_edges& ev, const double* d_poses, cugo_k::ReduceScratch rs, double* d_edge_chi)
{
    if (rs.capacity < IcpLayout(ev).end)
        throw std::runtime_error("cugo: ICP scratch too small");
    const IcpLayout lay(ev);
    IcpArgs a;
    a.plane = kind_of(ev, false, rs.d_partials, rs.d_partials + lay.cchi);
    a.line = kind_of(ev, true, rs.d_partials + lay.line_part, rs.d_partials + lay.cchi + lay.cp);
    a.n_poses_free = ev.n_poses_free;
    a.poses = d_poses;
    a.edge_chi = d_edge_chi;
    return a;
}

unsigned finish_grid(const cugo_icp_edges& ev) { return (unsigned)((32 * (size_t)ev.n_poses_free + ICP_WG - 1) / ICP_WG); }

} // namespace

namespace cugo_k
{

size_t icp_scratch_doubles(const cugo_icp_edges& ev)
{
    return IcpLayout(ev).end;
}

void launch_icp_chunks(hipStream_t s, const cugo_icp_edges& ev, const double* d_poses, bool full, ReduceScratch rs,
                       double* d_edge_chi)
{
    const IcpArgs a = args_of(ev, d_poses, rs, full ? nullptr : d_edge_chi);
    const IcpLayout lay(ev);
    const size_t waves = lay.cp + lay.cl;
    if (waves == 0)
        return;
    const unsigned grid = (unsigned)((waves * 64 + ICP_WG - 1) / ICP_WG);
    if (full)
        CUGO_LAUNCH(k_icp_chunks_build, dim3(grid), dim3(ICP_WG), 0, s, a);
    else
        CUGO_LAUNCH(k_icp_chunks_errors, dim3(grid), dim3(ICP_WG), 0, s, a);
}

void launch_icp_add(hipStream_t s, const cugo_icp_edges& ev, ReduceScratch rs, double* d_Hpp, double* d_bp)
{
    if (ev.n_poses_free <= 0 || ev.n_plane + ev.n_line == 0)
        return;
    const IcpArgs a = args_of(ev, nullptr, rs, nullptr);
    LaunchScope scope("k_icp_add", s);
    hipLaunchKernelGGL(k_icp_finish<false>, dim3(finish_grid(ev)), dim3(ICP_WG), 0, s, a, d_Hpp,
                       (const int32_t*)nullptr, d_bp, (double*)nullptr);
}

void launch_icp_add_schur(hipStream_t s, const cugo_icp_edges& ev, ReduceScratch rs, const int32_t* d_rowptr,
                          double* d_Hsc, double* d_bp, double* d_bsc)
{
    if (ev.n_poses_free <= 0 || ev.n_plane + ev.n_line == 0)
        return;
    const IcpArgs a = args_of(ev, nullptr, rs, nullptr);
    LaunchScope scope("k_icp_add_schur", s);
    hipLaunchKernelGGL(k_icp_finish<true>, dim3(finish_grid(ev)), dim3(ICP_WG), 0, s, a, d_Hsc, d_rowptr, d_bp, d_bsc);
}

int icp_chunk_count(const cugo_icp_edges& ev)
{
    const IcpLayout lay(ev);
    return (int)(lay.cp + lay.cl);
}

static void launch_icp_chi_total(hipStream_t s, const cugo_icp_edges& ev, ReduceScratch rs, double* d_chi, bool chi_add)
{
    launch_pose_chi_total(s, "k_icp_chi_total", rs.d_partials + IcpLayout(ev).cchi, icp_chunk_count(ev), d_chi, chi_add);
}

void launch_icp_build(hipStream_t s, const cugo_icp_edges& ev, const double* d_poses, double* d_Hpp, double* d_bp,
                      ReduceScratch rs, double* d_chi, bool chi_add)
{
    launch_icp_chunks(s, ev, d_poses, true, rs);
    launch_icp_add(s, ev, rs, d_Hpp, d_bp);
    if (d_chi)
        launch_icp_chi_total(s, ev, rs, d_chi, chi_add);
}

void launch_icp_errors(hipStream_t s, const cugo_icp_edges& ev, const double* d_poses, ReduceScratch rs, double* d_chi,
                       bool chi_add, double* d_edge_chi)
{
    launch_icp_chunks(s, ev, d_poses, false, rs, d_edge_chi);
    if (d_chi)
        launch_icp_chi_total(s, ev, rs, d_chi, chi_add);
}

} // namespace cugo_k
