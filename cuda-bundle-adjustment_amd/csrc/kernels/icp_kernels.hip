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
// Layout and reduction are the chunk scheme of pose_chunks.h, twice: each kind's edges are sorted by pose index (the
// key) and have their own partials, 21 of the upper triangle of H, 6 of b and chi2.  The finishing pass sums a pose's
// partials in chunk order (plane kind, then line kind).  The chi2 total of a pass is the sum of the chunk totals —
// plane chunks, then line chunks: a plain array that the reduction ending an LM trial sums next to the BA partials
// (ba_kernels.hip: k_sum_partials2).
#include <hip/hip_runtime.h>
#include <algorithm>

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

struct IcpArgs
{
    IcpKind plane, line;
    int n_poses_free;
    const double* poses;
    double* edge_chi; // error pass: [n_plane + n_line] or nullptr
};

// chunk c of one kind (pose_chunks.h: chunk_walk, keyed by pose)
template <bool LINE, bool FULL>
__device__ __forceinline__ void icp_chunk(const IcpKind& k, int c, int n_poses_free, const double* __restrict__ poses,
                                          double* __restrict__ edge_chi)
{
    chunk_walk<FULL, true>(k.n, k.pose, c, k.part, k.cchi, edge_chi, [&](int e, bool in, int q, double (&v)[32]) {
        if (in && q < n_poses_free && !(k.flags && (k.flags[e] & CUGO_EDGE_INACTIVE)))
            return icp_edge<LINE, FULL>(k, e, poses + 7 * (size_t)q, v);
        if (FULL)
            chunk_zero(v);
        return 0.0;
    });
}

// one wave per chunk: the plane chunks, then the line chunks
template <bool FULL>
__device__ __forceinline__ void icp_chunks(const IcpArgs& a)
{
    const int wave = (int)((blockIdx.x * (size_t)ICP_WG + threadIdx.x) >> 6);
    const int cp = chunk_count(a.plane.n), cl = chunk_count(a.line.n);
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

// the finishing pass (pose_chunks.h: chunk_finish) over the free poses that have ICP edges of either kind
template <bool SCHUR>
__global__ __launch_bounds__(ICP_WG) void k_icp_finish(IcpArgs a, double* __restrict__ H, const int32_t* __restrict__ rowptr,
                                                        double* __restrict__ bp, double* __restrict__ bsc)
{
    chunk_finish<SCHUR>(
        a.n_poses_free,
        [&](int p) { return a.plane.pose_ptr[p] != a.plane.pose_ptr[p + 1] || a.line.pose_ptr[p] != a.line.pose_ptr[p + 1]; },
        [&](int p, int t) { return chunk_key_sum(a.plane.pose_ptr, a.plane.part, p, t) + chunk_key_sum(a.line.pose_ptr, a.line.part, p, t); },
        H, rowptr, bp, bsc);
}

// scratch = [plane partials (cp + n_poses_total slots) | line partials (cl + n_poses_total) | chunk totals (cp + cl)]
struct IcpLayout
{
    ChunkLayout plane, line;
    size_t cchi, end;
    explicit IcpLayout(const cugo_icp_edges& ev) : plane(ev.n_plane, ev.n_poses_total), line(ev.n_line, ev.n_poses_total)
    {
        cchi = plane.cchi + line.cchi;
        end = cchi + plane.chunks + line.chunks;
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

IcpArgs args_of(const cugo_icp_edges& ev, const double* d_poses, cugo_k::ChunkScratch rs, double* d_edge_chi)
{
    const IcpLayout lay(ev);
    IcpArgs a;
    a.plane = kind_of(ev, false, rs.d_part, rs.d_cchi);
    a.line = kind_of(ev, true, rs.d_part + lay.plane.cchi, rs.d_cchi + lay.plane.chunks);
    a.n_poses_free = ev.n_poses_free;
    a.poses = d_poses;
    a.edge_chi = d_edge_chi;
    return a;
}

} // namespace

namespace cugo_k
{

size_t icp_scratch_doubles(const cugo_icp_edges& ev) { return IcpLayout(ev).end; }

int icp_chunk_count(const cugo_icp_edges& ev) { return chunk_count(ev.n_plane) + chunk_count(ev.n_line); }

ChunkScratch icp_scratch_in(ReduceScratch rs, const cugo_icp_edges& ev)
{
    const IcpLayout lay(ev);
    return chunk_scratch_in(rs, lay.cchi, lay.end, "ICP");
}

void launch_icp_chunks(hipStream_t s, const cugo_icp_edges& ev, const double* d_poses, bool full, ChunkScratch rs,
                       double* d_edge_chi)
{
    const IcpArgs a = args_of(ev, d_poses, rs, full ? nullptr : d_edge_chi);
    const size_t waves = (size_t)icp_chunk_count(ev);
    if (waves == 0)
        return;
    if (full)
        CUGO_LAUNCH(k_icp_chunks_build, dim3(chunk_grid(waves)), dim3(ICP_WG), 0, s, a);
    else
        CUGO_LAUNCH(k_icp_chunks_errors, dim3(chunk_grid(waves)), dim3(ICP_WG), 0, s, a);
}

void launch_icp_add(hipStream_t s, const cugo_icp_edges& ev, ChunkScratch rs, double* d_Hpp, double* d_bp)
{
    if (ev.n_poses_free <= 0 || ev.n_plane + ev.n_line == 0)
        return;
    const IcpArgs a = args_of(ev, nullptr, rs, nullptr);
    LaunchScope scope("k_icp_add", s);
    hipLaunchKernelGGL(k_icp_finish<false>, dim3(finish_grid(ev.n_poses_free)), dim3(ICP_WG), 0, s, a, d_Hpp,
                       (const int32_t*)nullptr, d_bp, (double*)nullptr);
}

void launch_icp_add_schur(hipStream_t s, const cugo_icp_edges& ev, ChunkScratch rs, const int32_t* d_rowptr,
                          double* d_Hsc, double* d_bp, double* d_bsc)
{
    if (ev.n_poses_free <= 0 || ev.n_plane + ev.n_line == 0)
        return;
    const IcpArgs a = args_of(ev, nullptr, rs, nullptr);
    LaunchScope scope("k_icp_add_schur", s);
    hipLaunchKernelGGL(k_icp_finish<true>, dim3(finish_grid(ev.n_poses_free)), dim3(ICP_WG), 0, s, a, d_Hsc, d_rowptr, d_bp,
                       d_bsc);
}

void launch_icp_chi_total(hipStream_t s, const cugo_icp_edges& ev, ChunkScratch rs, double* d_chi, bool chi_add)
{
    launch_pose_chi_total(s, "k_icp_chi_total", rs.d_cchi, icp_chunk_count(ev), d_chi, chi_add);
}

void launch_icp_build(hipStream_t s, const cugo_icp_edges& ev, const double* d_poses, double* d_Hpp, double* d_bp,
                      ChunkScratch rs, double* d_chi, bool chi_add)
{
    launch_icp_chunks(s, ev, d_poses, true, rs);
    launch_icp_add(s, ev, rs, d_Hpp, d_bp);
    if (d_chi)
        launch_icp_chi_total(s, ev, rs, d_chi, chi_add);
}

void launch_icp_errors(hipStream_t s, const cugo_icp_edges& ev, const double* d_poses, ChunkScratch rs, double* d_chi,
                       bool chi_add, double* d_edge_chi)
{
    launch_icp_chunks(s, ev, d_poses, false, rs, d_edge_chi);
    if (d_chi)
        launch_icp_chi_total(s, ev, rs, d_chi, chi_add);
}

} // namespace cugo_k
