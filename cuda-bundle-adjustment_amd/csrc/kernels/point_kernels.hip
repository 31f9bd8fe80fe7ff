// Point-to-point pose edges with a 3 x 3 information matrix (include/point_edge_types.h; an extension, the reference has
// no such edge): a known 3-D point p, measured as the point z in the pose's frame.  Conventions as for the ICP kinds
// (icp_kernels.hip): y = R(q) p + t (ba_math.h world_to_cam), left update in the tangent order [omega, upsilon].
//   r = y - z (3-vector),  J = dr/dxi = [ S | I ],  S = -[y]x
//   x = max(0, r^T Omega r),  chi2 term rho(x) with the set's robust kernel,  w = rho'(x)
//   H += w J^T Omega J,  b -= w J^T Omega r        (the sign of cugo_icp_construct_quadratic_form)
// Omega r and Omega S are formed once:  H_ww = S^T (Omega S),  H_wv = (Omega S)^T,  H_vv = Omega,
// b = -w (y x (Omega r), Omega r).  Omega is symmetric positive SEMI-definite (singular matrices are legal: Omega =
// omega n n^T with z on the plane is the plane edge, Omega = omega (I - u u^T) with z = a the line edge); it comes as its
// upper triangle, row-major packed (00 01 02 11 12 22), [6][n] or one matrix for all edges ([6][1]: wave-uniform).
//
// Layout and reduction are those of icp_kernels.hip, for one kind: edges sorted by pose, one wave per chunk of ICP_CHUNK
// edges, a partial of 28 doubles at slot chunk + pose, one chi2 total per chunk, a finishing pass of 32 threads per free
// pose.  No atomics, one fixed order; the error pass forms the chunk totals of the build pass bit for bit.
#include <hip/hip_runtime.h>
#include <climits>
#include <stdexcept>

#include "ba_math.h"
#include "kernels.h"
#include "pose_chunks.h"

namespace
{

using namespace cugo_dev;

struct PointArgs
{
    int n;
    const int32_t* pose;
    const int32_t* pose_ptr;
    const double* p;    // [3][n]
    const double* z;    // [3][n]
    const double* info; // [6][n] or [6][1]
    int n_info;
    const uint8_t* flags;
    Robust rk;
    double* part; // [n_chunks + n_poses_total][ICP_NP]
    double* cchi; // [n_chunks] chi2 total of every chunk
    int n_poses_free;
    const double* poses;
    double* edge_chi; // error pass: [n] or nullptr
};

// contribution of edge e: v[0..20] upper triangle of w J^T Omega J (row-major packed), v[21..26] -w J^T Omega r;
// returns the chi2 term
template <bool FULL>
__device__ __forceinline__ double point_edge(const PointArgs& k, int e, const double* __restrict__ pose, double (&v)[32])
{
    const size_t n = (size_t)k.n;
    const double pp[3] = {k.p[e], k.p[n + e], k.p[2 * n + e]};
    double y[3];
    world_to_cam(pose, pp, y);
    const double r0 = y[0] - k.z[e], r1 = y[1] - k.z[n + e], r2 = y[2] - k.z[2 * n + e];
    const size_t s = k.n_info == 1 ? 1 : n; // [6][1]: one matrix for all
    const int i = k.n_info == 1 ? 0 : e;
    const double o00 = k.info[i], o01 = k.info[s + i], o02 = k.info[2 * s + i];
    const double o11 = k.info[3 * s + i], o12 = k.info[4 * s + i], o22 = k.info[5 * s + i];
    const double O[3][3] = {{o00, o01, o02}, {o01, o11, o12}, {o02, o12, o22}};
    double q[3]; // Omega r
#pragma unroll
    for (int a = 0; a < 3; a++)
        q[a] = O[a][0] * r0 + O[a][1] * r1 + O[a][2] * r2;
    const double x = fmax(0.0, r0 * q[0] + r1 * q[1] + r2 * q[2]);
    const double chi = rk_rho(k.rk, x);
    if (FULL)
    {
        const double w = rk_drho(k.rk, x);
        // Omega S, S = -[y]x: row a is y x (row a of Omega)
        double G[3][3];
#pragma unroll
        for (int a = 0; a < 3; a++)
        {
            G[a][0] = O[a][2] * y[1] - O[a][1] * y[2];
            G[a][1] = O[a][0] * y[2] - O[a][2] * y[0];
            G[a][2] = O[a][1] * y[0] - O[a][0] * y[1];
        }
        // S^T (Omega S): row 0 = y1 G2. - y2 G1., row 1 = y2 G0. - y0 G2., row 2 = y0 G1. - y1 G0.
        v[0] = w * (y[1] * G[2][0] - y[2] * G[1][0]);
        v[1] = w * (y[1] * G[2][1] - y[2] * G[1][1]);
        v[2] = w * (y[1] * G[2][2] - y[2] * G[1][2]);
        v[6] = w * (y[2] * G[0][1] - y[0] * G[2][1]);
        v[7] = w * (y[2] * G[0][2] - y[0] * G[2][2]);
        v[11] = w * (y[0] * G[1][2] - y[1] * G[0][2]);
        // (Omega S)^T
#pragma unroll
        for (int j = 0; j < 3; j++)
        {
            v[3 + j] = w * G[j][0];
            v[8 + j] = w * G[j][1];
            v[12 + j] = w * G[j][2];
        }
        v[15] = w * o00, v[16] = w * o01, v[17] = w * o02;
        v[18] = w * o11, v[19] = w * o12, v[20] = w * o22;
        v[21] = -(w * (y[1] * q[2] - y[2] * q[1]));
        v[22] = -(w * (y[2] * q[0] - y[0] * q[2]));
        v[23] = -(w * (y[0] * q[1] - y[1] * q[0]));
        v[24] = -(w * q[0]), v[25] = -(w * q[1]), v[26] = -(w * q[2]);
    }
    return chi;
}

// One wave per chunk of ICP_CHUNK edges (the walk of icp_kernels.hip's icp_chunk).  FULL: partials of H, b and chi2;
// otherwise chi2 only (slot element 27, the same value FULL writes there) and, with edge_chi, the chi2 term of every edge.
template <bool FULL>
__device__ __forceinline__ void point_chunks(const PointArgs& k)
{
    const int c = (int)((blockIdx.x * (size_t)ICP_WG + threadIdx.x) >> 6);
    if (c >= (k.n + ICP_CHUNK - 1) / ICP_CHUNK)
        return;
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
        if (in && q < k.n_poses_free && !(k.flags && (k.flags[e] & CUGO_EDGE_INACTIVE)))
            chi = point_edge<FULL>(k, e, k.poses + 7 * (size_t)q, v);
        else if (FULL)
        {
#pragma unroll
            for (int i = 0; i < 27; i++)
                v[i] = 0.0;
        }
        if (!FULL && k.edge_chi && in)
            k.edge_chi[e] = chi;
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

__global__ __launch_bounds__(ICP_WG) void k_point_chunks_build(PointArgs a) { point_chunks<true>(a); }
// (six waves per SIMD, as k_icp_chunks_errors: the pass is bound by the loads it has in flight)
__global__ __launch_bounds__(ICP_WG) __attribute__((amdgpu_waves_per_eu(6))) void k_point_chunks_errors(PointArgs a)
{
    point_chunks<false>(a);
}

// 32 threads per free pose that has point edges; thread t < 27 adds element t of the pose's sums to Hpp / bp or, SCHUR,
// to the diagonal block of Hsc, to bp and to bsc (k_icp_finish, for one kind)
template <bool SCHUR>
__global__ __launch_bounds__(ICP_WG) void k_point_finish(PointArgs a, double* __restrict__ H, const int32_t* __restrict__ rowptr,
                                                          double* __restrict__ bp, double* __restrict__ bsc)
{
    const int p = (int)((blockIdx.x * (size_t)ICP_WG + threadIdx.x) >> 5), t = threadIdx.x & 31;
    if (p >= a.n_poses_free || t >= 27)
        return;
    if (a.pose_ptr[p] == a.pose_ptr[p + 1])
        return; // (nothing to add: the pose's blocks keep their bits, and its partial slots were never written)
    const double s = chunk_pose_sum(a.pose_ptr, a.part, p, t);
    int r = 0, c = 0;
    if (t < 21)
        tri6_unpack(t, r, c);
    pose_term_add<SCHUR>(p, t, r, c, s, H, rowptr, bp, bsc);
}

// the two runs of a pass and, where they share one scratch, its layout: [partials (chunks + n_poses_total slots) | chunk totals]
struct PointLayout
{
    size_t chunks, cchi, end;
    explicit PointLayout(const cugo_point_edges& ev)
    {
        chunks = (size_t)(ev.n + ICP_CHUNK - 1) / ICP_CHUNK;
        cchi = (chunks + ev.n_poses_total) * ICP_NP;
        end = cchi + chunks;
    }
};

PointArgs args_of(const cugo_point_edges& ev, const double* d_poses, cugo_k::PointScratch ps, double* d_edge_chi)
{
    return PointArgs{ev.n,      ev.d_pose, ev.d_pose_ptr, ev.d_p,     ev.d_z,       ev.d_info,       ev.n_info,
                     ev.d_flags, Robust{ev.rk, ev.delta}, ps.d_part, ps.d_cchi, ev.n_poses_free, d_poses, d_edge_chi};
}

} // namespace

namespace cugo_k
{

size_t point_scratch_doubles(const cugo_point_edges& ev)
{
    return PointLayout(ev).end;
}

size_t point_partial_doubles(const cugo_point_edges& ev)
{
    return PointLayout(ev).cchi;
}

PointScratch point_scratch_in(ReduceScratch rs, const cugo_point_edges& ev)
{
    const PointLayout lay(ev);
    if (rs.capacity < lay.end)
        throw std::runtime_error("cugo: point edge scratch too small");
    return PointScratch{rs.d_partials, rs.d_partials + lay.cchi};
}

int point_chunk_count(const cugo_point_edges& ev)
{
    return (int)PointLayout(ev).chunks;
}

void launch_point_chunks(hipStream_t s, const cugo_point_edges& ev, const double* d_poses, bool full, PointScratch rs,
                         double* d_edge_chi)
{
    const PointArgs a = args_of(ev, d_poses, rs, full ? nullptr : d_edge_chi);
    const size_t waves = PointLayout(ev).chunks;
    if (waves == 0)
        return;
    const unsigned grid = (unsigned)((waves * 64 + ICP_WG - 1) / ICP_WG);
    if (full)
        CUGO_LAUNCH(k_point_chunks_build, dim3(grid), dim3(ICP_WG), 0, s, a);
    else
        CUGO_LAUNCH(k_point_chunks_errors, dim3(grid), dim3(ICP_WG), 0, s, a);
}

static unsigned finish_grid(const cugo_point_edges& ev) { return (unsigned)((32 * (size_t)ev.n_poses_free + ICP_WG - 1) / ICP_WG); }

void launch_point_add(hipStream_t s, const cugo_point_edges& ev, PointScratch rs, double* d_Hpp, double* d_bp)
{
    if (ev.n_poses_free <= 0 || ev.n == 0)
        return;
    const PointArgs a = args_of(ev, nullptr, rs, nullptr);
    LaunchScope scope("k_point_add", s);
    hipLaunchKernelGGL(k_point_finish<false>, dim3(finish_grid(ev)), dim3(ICP_WG), 0, s, a, d_Hpp, (const int32_t*)nullptr,
                       d_bp, (double*)nullptr);
}

void launch_point_add_schur(hipStream_t s, const cugo_point_edges& ev, PointScratch rs, const int32_t* d_rowptr,
                            double* d_Hsc, double* d_bp, double* d_bsc)
{
    if (ev.n_poses_free <= 0 || ev.n == 0)
        return;
    const PointArgs a = args_of(ev, nullptr, rs, nullptr);
    LaunchScope scope("k_point_add_schur", s);
    hipLaunchKernelGGL(k_point_finish<true>, dim3(finish_grid(ev)), dim3(ICP_WG), 0, s, a, d_Hsc, d_rowptr, d_bp, d_bsc);
}

void launch_point_chi_total(hipStream_t s, const cugo_point_edges& ev, PointScratch rs, double* d_chi, bool chi_add)
{
    launch_pose_chi_total(s, "k_point_chi_total", rs.d_cchi, point_chunk_count(ev), d_chi, chi_add);
}

void launch_point_build(hipStream_t s, const cugo_point_edges& ev, const double* d_poses, double* d_Hpp, double* d_bp,
                        PointScratch rs, double* d_chi, bool chi_add)
{
    launch_point_chunks(s, ev, d_poses, true, rs);
    launch_point_add(s, ev, rs, d_Hpp, d_bp);
    if (d_chi)
        launch_point_chi_total(s, ev, rs, d_chi, chi_add);
}

void launch_point_errors(hipStream_t s, const cugo_point_edges& ev, const double* d_poses, PointScratch rs, double* d_chi,
                         bool chi_add, double* d_edge_chi)
{
    launch_point_chunks(s, ev, d_poses, false, rs, d_edge_chi);
    if (d_chi)
        launch_point_chi_total(s, ev, rs, d_chi, chi_add);
}

} // namespace cugo_k
