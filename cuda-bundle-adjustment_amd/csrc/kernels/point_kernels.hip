// Point-to-point pose edges with a 3 x 3 information matrix (include/point_edge_types.h; an extension, the reference has
// no such edge): a known 3-D point p, measured as the point z in the pose's frame.  Conventions as for the ICP kinds
// (icp_kernels.hip): y = R(q) p + t (ba_math.h world_to_cam), left update in the tangent order [omega, upsilon].
//   r = y - z (3-vector),  J = dr/dxi = [ S | I ],  S = -[y]x
//   x = max(0, r^T Omega r),  chi2 term rho(x) with the set's robust kernel,  w = rho'(x)
//   H += w J^T Omega J,  b -= w J^T Omega r        (the sign of cugo_icp_construct_quadratic_form)
// The term is point_term.h's at (y, Omega): b = -w (y x (Omega r), Omega r).  Omega is symmetric positive SEMI-definite
// (singular matrices are legal: Omega = omega n n^T with z on the plane is the plane edge, Omega = omega (I - u u^T) with
// z = a the line edge); it comes as its upper triangle, row-major packed (00 01 02 11 12 22), [6][n] or [6][1].
//
// The covariance form (include/cugo_hip.h: cugo_gicp_edges; point_term.h): Omega = (C_z + R C_p R^T)^-1 formed at the poses
// the pass is given, from the upper triangles cov_p (world frame) and cov_z (the pose's frame).  It is an instantiation of
// its own of the chunk kernels (k_gicp_chunks_*); the information form's kernels carry no branch for it.
//
// Layout and reduction are the chunk scheme of pose_chunks.h, for one kind keyed by pose.
#include <hip/hip_runtime.h>

#include "point_term.h"
#include "pose_chunks.h"

namespace
{

using namespace cugo_dev;

struct PointArgs
{
    static constexpr bool COV = false;
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
// the covariance form: info is cov_p [6][n_info], n_info the count of both covariances
struct GicpArgs : PointArgs
{
    static constexpr bool COV = true;
    const double* cov_z; // [6][n] or [6][1]
};

// contribution of edge e: v[0..20] upper triangle of w J^T Omega J (row-major packed), v[21..26] -w J^T Omega r;
// returns the chi2 term
template <bool FULL, class K>
__device__ __forceinline__ double point_edge(const K& k, int e, const double* __restrict__ pose, double (&v)[32])
{
    const size_t n = (size_t)k.n;
    const double pp[3] = {k.p[e], k.p[n + e], k.p[2 * n + e]};
    double y[3];
    world_to_cam(pose, pp, y);
    const double z[3] = {k.z[e], k.z[n + e], k.z[2 * n + e]};
    double O[3][3], q[3], x;
    double chi;
    if constexpr (K::COV)
    {
        double R[3][3]; // M = R
        quat_to_rot(pose, R);
        chi = point_residual<true>(y, z, k.info, k.n_info, n, e, k.rk, O, q, x, k.cov_z, &R);
    }
    else
        chi = point_residual(y, z, k.info, k.n_info, n, e, k.rk, O, q, x);
    if (FULL)
    {
        const double w = rk_drho(k.rk, x);
        unary_block(y, O, w, v);
        unary_b(y, q, -w, v);
    }
    return chi;
}

// one wave per chunk (pose_chunks.h: chunk_walk, keyed by pose)
template <bool FULL, class K>
__device__ __forceinline__ void point_chunks(const K& k)
{
    const int c = (int)((blockIdx.x * (size_t)ICP_WG + threadIdx.x) >> 6);
    if (c >= chunk_count(k.n))
        return;
    chunk_walk<FULL, true>(k.n, k.pose, c, k.part, k.cchi, k.edge_chi, [&](int e, bool in, int q, double (&v)[32]) {
        if (in && q < k.n_poses_free && !(k.flags && (k.flags[e] & CUGO_EDGE_INACTIVE)))
            return point_edge<FULL>(k, e, k.poses + 7 * (size_t)q, v);
        if (FULL)
            chunk_zero(v);
        return 0.0;
    });
}

__global__ __launch_bounds__(ICP_WG) void k_point_chunks_build(PointArgs a) { point_chunks<true>(a); }
// (six waves per SIMD, as k_icp_chunks_errors: the pass is bound by the loads it has in flight)
__global__ __launch_bounds__(ICP_WG) __attribute__((amdgpu_waves_per_eu(6))) void k_point_chunks_errors(PointArgs a)
{
    point_chunks<false>(a);
}
// the covariance form.  Its error pass holds M, two covariances and the factor next to the loads in flight: it does not fit
// the 80 VGPRs of six waves per SIMD without spilling, so it keeps the bound of the workgroup size alone
__global__ __launch_bounds__(ICP_WG) void k_gicp_chunks_build(GicpArgs a) { point_chunks<true>(a); }
__global__ __launch_bounds__(ICP_WG) void k_gicp_chunks_errors(GicpArgs a) { point_chunks<false>(a); }

// the finishing pass (pose_chunks.h: chunk_finish) over the free poses that have point edges
template <bool SCHUR>
__global__ __launch_bounds__(ICP_WG) void k_point_finish(PointArgs a, double* __restrict__ H, const int32_t* __restrict__ rowptr,
                                                          double* __restrict__ bp, double* __restrict__ bsc)
{
    chunk_finish<SCHUR>(
        a.n_poses_free, [&](int p) { return a.pose_ptr[p] != a.pose_ptr[p + 1]; },
        [&](int p, int t) { return chunk_key_sum(a.pose_ptr, a.part, p, t); }, H, rowptr, bp, bsc);
}

ChunkLayout layout_of(const cugo_point_edges& ev) { return ChunkLayout(ev.n, ev.n_poses_total); }

PointArgs args_of(const cugo_point_edges& ev, const double* d_poses, cugo_k::ChunkScratch ps, double* d_edge_chi)
{
    return PointArgs{ev.n,      ev.d_pose, ev.d_pose_ptr, ev.d_p,     ev.d_z,       ev.d_info,       ev.n_info,
                     ev.d_flags, Robust{ev.rk, ev.delta}, ps.d_part, ps.d_cchi, ev.n_poses_free, d_poses, d_edge_chi};
}

} // namespace

namespace cugo_k
{

size_t point_scratch_doubles(const cugo_point_edges& ev) { return layout_of(ev).end; }
size_t point_partial_doubles(const cugo_point_edges& ev) { return layout_of(ev).cchi; }
int point_chunk_count(const cugo_point_edges& ev) { return chunk_count(ev.n); }

ChunkScratch point_scratch_in(ReduceScratch rs, const cugo_point_edges& ev)
{
    const ChunkLayout lay = layout_of(ev);
    return chunk_scratch_in(rs, lay.cchi, lay.end, "point edge");
}

void launch_point_chunks(hipStream_t s, const cugo_point_edges& ev, const double* d_poses, bool full, ChunkScratch rs,
                         double* d_edge_chi, const double* d_cov_z)
{
    const PointArgs a = args_of(ev, d_poses, rs, full ? nullptr : d_edge_chi);
    const size_t waves = (size_t)chunk_count(ev.n);
    if (waves == 0)
        return;
    if (d_cov_z)
    {
        const GicpArgs g{a, d_cov_z};
        if (full)
            CUGO_LAUNCH(k_gicp_chunks_build, dim3(chunk_grid(waves)), dim3(ICP_WG), 0, s, g);
        else
            CUGO_LAUNCH(k_gicp_chunks_errors, dim3(chunk_grid(waves)), dim3(ICP_WG), 0, s, g);
    }
    else if (full)
        CUGO_LAUNCH(k_point_chunks_build, dim3(chunk_grid(waves)), dim3(ICP_WG), 0, s, a);
    else
        CUGO_LAUNCH(k_point_chunks_errors, dim3(chunk_grid(waves)), dim3(ICP_WG), 0, s, a);
}

void launch_point_add(hipStream_t s, const cugo_point_edges& ev, ChunkScratch rs, double* d_Hpp, double* d_bp)
{
    if (ev.n_poses_free <= 0 || ev.n == 0)
        return;
    const PointArgs a = args_of(ev, nullptr, rs, nullptr);
    LaunchScope scope("k_point_add", s);
    hipLaunchKernelGGL(k_point_finish<false>, dim3(finish_grid(ev.n_poses_free)), dim3(ICP_WG), 0, s, a, d_Hpp,
                       (const int32_t*)nullptr, d_bp, (double*)nullptr);
}

void launch_point_add_schur(hipStream_t s, const cugo_point_edges& ev, ChunkScratch rs, const int32_t* d_rowptr,
                            double* d_Hsc, double* d_bp, double* d_bsc)
{
    if (ev.n_poses_free <= 0 || ev.n == 0)
        return;
    const PointArgs a = args_of(ev, nullptr, rs, nullptr);
    LaunchScope scope("k_point_add_schur", s);
    hipLaunchKernelGGL(k_point_finish<true>, dim3(finish_grid(ev.n_poses_free)), dim3(ICP_WG), 0, s, a, d_Hsc, d_rowptr, d_bp,
                       d_bsc);
}

void launch_point_chi_total(hipStream_t s, const cugo_point_edges& ev, ChunkScratch rs, double* d_chi, bool chi_add)
{
    launch_pose_chi_total(s, "k_point_chi_total", rs.d_cchi, point_chunk_count(ev), d_chi, chi_add);
}

void launch_point_build(hipStream_t s, const cugo_point_edges& ev, const double* d_poses, double* d_Hpp, double* d_bp,
                        ChunkScratch rs, double* d_chi, bool chi_add, const double* d_cov_z)
{
    launch_point_chunks(s, ev, d_poses, true, rs, nullptr, d_cov_z);
    launch_point_add(s, ev, rs, d_Hpp, d_bp);
    if (d_chi)
        launch_point_chi_total(s, ev, rs, d_chi, chi_add);
}

void launch_point_errors(hipStream_t s, const cugo_point_edges& ev, const double* d_poses, ChunkScratch rs, double* d_chi,
                         bool chi_add, double* d_edge_chi, const double* d_cov_z)
{
    launch_point_chunks(s, ev, d_poses, false, rs, d_edge_chi, d_cov_z);
    if (d_chi)
        launch_point_chi_total(s, ev, rs, d_chi, chi_add);
}

} // namespace cugo_k
