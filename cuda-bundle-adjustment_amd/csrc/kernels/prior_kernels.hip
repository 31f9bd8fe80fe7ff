// SE(3) pose priors (include/prior_types.h; an extension, the reference has no such edge): unary edges on a pose vertex
// with an SE(3) measurement Z = (q_z, t_z) and a full 6 x 6 information matrix Omega.  The pose (q, t) is read as
// everywhere else (y = R(q) p + t), the update is T <- Exp([omega, upsilon]) T (ba_math.h pose_exp_update).
//   R_D = R(q) R(q_z)^T,  t_D = t - R_D t_z                      (D = T Z^-1)
//   r   = [ phi ; t_D ],  phi = Log_SO3(R_D)                     (tangent order [omega, upsilon], that of the covariances)
//   J   = dr/dxi = [ J_l^-1(phi)  0 ]      J_l^-1(phi) = I - 1/2 [phi]x + c(theta) [phi]x^2,  theta = |phi|,
//                  [ -[t_D]x      I ]      c = 1/theta^2 - (1 + cos theta) / (2 theta sin theta)   (1/12 + theta^2/720 near 0)
//   x = max(0, r^T Omega r), chi2 term rho(x), w = rho'(x), H += w J^T Omega J, b -= w J^T Omega r
// The sign and the column-major blocks are those of the BA and ICP build passes (icp_kernels.hip): b is minus half the
// gradient of chi2 and the step of H dx = b is applied as exp(+dx).
//
// Layout: edges sorted by pose index with a CSR pose_ptr, structure of arrays; Omega as its upper triangle, row-major
// packed (the order of the first 21 entries of icp_kernels.hip's edge vector), per edge or one for all.
//
// The workload is small (about one prior per pose), so what counts is launches, not throughput: ONE kernel per pass.
// 32 lanes own a free pose (eight poses per workgroup) and walk its priors in container order; every lane recomputes r,
// J and Omega J of an edge in registers (static indices only) and forms the element it owns: lane t < 21 entry t of
// the upper triangle of H, lanes 21..26 b.  The sums are ADDED straight to their destination — Hpp / bp
// behind k_build_poses, or the pose's diagonal block of Hsc, bp and bsc behind k_pose_schur in the one-stream form of the
// LM loop — with no partials, no atomics and one fixed order.  Every workgroup leaves ONE chi2 total (its poses in
// order); the error-only form computes exactly these totals, so its chi2 has the bits of the build pass's.  A pose
// without priors keeps the bits of its blocks; fixed poses (index >= n_poses_free) are never visited.
#include <hip/hip_runtime.h>
#include <stdexcept>

#include "ba_math.h"
#include "kernels.h"

namespace
{

using namespace cugo_dev;

constexpr int PRIOR_WG = 256;
constexpr int PRIOR_LANES = 32;                     // lanes per pose
constexpr int PRIOR_POSES = PRIOR_WG / PRIOR_LANES; // poses per workgroup

enum PriorMode
{
    PRIOR_ERRORS = 0, // chi2 only
    PRIOR_HPP = 1,    // + H into Hpp [P][36], b into bp
    PRIOR_SCHUR = 2   // + H into the diagonal block of Hsc (through rowptr), b into bp and bsc
};

struct PriorArgs
{
    int n, n_poses_free;
    const int32_t* pose_ptr;
    const double* meas; // [7][n]
    const double* info; // [21][n] or [21][1]
    int n_info;
    const uint8_t* flags;
    Robust rk;
    const double* poses;
    double* wg_chi;   // [workgroups]
    double* edge_chi; // [n] or nullptr (error pass)
};

// chi2 term of edge e; with FULL also the element the lane owns, into `mine`: entry (ri, ci) of w J^T Omega J
// (ci < 6, sign +1) or entry ri of -w J^T Omega r (ci == 6, sign -1).  J and Omega J are held in registers under static indices;
// the lane's columns are picked by compare-and-select.
template <bool FULL>
__device__ __forceinline__ double prior_edge(const PriorArgs& a, int e, const double* __restrict__ pose, int ri, int ci,
                                             double sign, double& mine)
{
    double qz[4], tz[3];
    const int stride = se3_load_meas(a.meas, a.n, e, qz, tz);
    double R[3][3], Rz[3][3], D[3][3];
    quat_to_rot(pose, R);
    quat_to_rot(qz, Rz);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            D[i][j] = R[i][0] * Rz[j][0] + R[i][1] * Rz[j][1] + R[i][2] * Rz[j][2];
    double r[6], sn, cs, theta;
    se3_residual(D, pose + 4, tz, r, sn, cs, theta);
    double Om[6][6], Or[6];
    se3_load_info(a.info, a.n_info, e, stride, Om);
    const double x = se3_quadratic(Om, r, Or);
    const double chi = rk_rho(a.rk, x);
    if (FULL)
    {
        const double w = rk_drho(a.rk, x);
        double Jl[3][3], J[6][6];
        se3_jl_inv(r, theta, sn, cs, Jl);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++)
            {
                J[i][j] = Jl[i][j];
                J[i][3 + j] = 0.0;
                J[3 + i][3 + j] = i == j ? 1.0 : 0.0;
            }
        // -[t_D]x
        J[3][0] = 0.0, J[3][1] = r[5], J[3][2] = -r[4];
        J[4][0] = -r[5], J[4][1] = 0.0, J[4][2] = r[3];
        J[5][0] = r[4], J[5][1] = -r[3], J[5][2] = 0.0;
        double OJ[6][6]; // Omega J
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j < 6; j++)
            {
                double s = Om[i][0] * J[0][j];
#pragma unroll
                for (int k = 1; k < 6; k++)
                    s += Om[i][k] * J[k][j];
                OJ[i][j] = s;
            }
        double sum = 0.0;
#pragma unroll
        for (int k = 0; k < 6; k++)
        {
            double jc = J[k][0], oc = OJ[k][0];
#pragma unroll
            for (int c = 1; c < 6; c++)
            {
                jc = ri == c ? J[k][c] : jc;
                oc = ci == c ? OJ[k][c] : oc;
            }
            oc = ci == 6 ? Or[k] : oc;
            sum = k == 0 ? jc * oc : sum + jc * oc;
        }
        mine = sign * (w * sum);
    }
    return chi;
}

template <int MODE>
__global__ __launch_bounds__(PRIOR_WG) void k_prior(PriorArgs a, double* __restrict__ H, const int32_t* __restrict__ rowptr,
                                                     double* __restrict__ bp, double* __restrict__ bsc)
{
    __shared__ double s_chi[PRIOR_POSES];
    const int g = threadIdx.x / PRIOR_LANES, t = threadIdx.x % PRIOR_LANES;
    const int p = blockIdx.x * PRIOR_POSES + g;
    double mine = 0.0, chi = 0.0;
    bool any = false; // an edge of this pose counted
    // the element lane t owns: t < 21 entry (ri, ci) of the upper triangle of H (row-major packed), 21..26 entry ri of b
    int ri = 0, ci = 0;
    const bool is_b = t >= 21;
    if (is_b)
        ri = t < 27 ? t - 21 : 0, ci = 6;
    else
        tri6_unpack(t, ri, ci);
    if (p < a.n_poses_free)
    {
        const double* pose = a.poses + 7 * (size_t)p;
        for (int e = a.pose_ptr[p], e1 = a.pose_ptr[p + 1]; e < e1; e++)
        {
            const bool active = !(a.flags && (a.flags[e] & CUGO_EDGE_INACTIVE));
            double c = 0.0;
            if (active)
            {
                double term = 0.0;
                // (opaque copies: the compare masks of the column selects are formed per edge instead of being kept
                //  in scalar registers across the loop, where they would not all fit)
                int ri_e = ri, ci_e = ci;
                asm volatile("" : "+v"(ri_e), "+v"(ci_e));
                c = prior_edge<MODE != PRIOR_ERRORS>(a, e, pose, ri_e, ci_e, is_b ? -1.0 : 1.0, term);
                mine += term;
                chi += c;
                any = true;
            }
            if (MODE == PRIOR_ERRORS && a.edge_chi && t == 0)
                a.edge_chi[e] = c;
        }
    }
    if (t == 0)
        s_chi[g] = chi;
    if (MODE != PRIOR_ERRORS && any)
        pose_term_add<MODE == PRIOR_SCHUR>(p, t, ri, ci, mine, H, rowptr, bp, bsc);
    pose_groups_chi_total<PRIOR_POSES>(s_chi, a.wg_chi);
}

template <int MODE>
void launch(hipStream_t s, const char* label, const cugo_prior_edges& ev, const double* d_poses, double* d_wg_chi,
            double* d_edge_chi, double* d_H, const int32_t* d_rowptr, double* d_bp, double* d_bsc)
{
    const int wgs = cugo_k::prior_workgroups(ev);
    if (!wgs)
        return;
    PriorArgs a;
    a.n = ev.n, a.n_poses_free = ev.n_poses_free;
    a.pose_ptr = ev.d_pose_ptr, a.meas = ev.d_meas, a.info = ev.d_info, a.n_info = ev.n_info;
    a.flags = ev.d_flags;
    a.rk = Robust{ev.rk, ev.delta};
    a.poses = d_poses;
    a.wg_chi = d_wg_chi, a.edge_chi = d_edge_chi;
    cugo_k::LaunchScope scope(label, s);
    hipLaunchKernelGGL(k_prior<MODE>, dim3(wgs), dim3(PRIOR_WG), 0, s, a, d_H, d_rowptr, d_bp, d_bsc);
}

} // namespace

namespace cugo_k
{

int prior_workgroups(const cugo_prior_edges& ev)
{
    return ev.n > 0 && ev.n_poses_free > 0 ? (ev.n_poses_free + PRIOR_POSES - 1) / PRIOR_POSES : 0;
}

void launch_prior_errors(hipStream_t s, const cugo_prior_edges& ev, const double* d_poses, double* d_wg_chi,
                         double* d_edge_chi)
{
    launch<PRIOR_ERRORS>(s, "k_prior_errors", ev, d_poses, d_wg_chi, d_edge_chi, nullptr, nullptr, nullptr, nullptr);
}

void launch_prior_add(hipStream_t s, const cugo_prior_edges& ev, const double* d_poses, double* d_Hpp, double* d_bp,
                      double* d_wg_chi)
{
    launch<PRIOR_HPP>(s, "k_prior_add", ev, d_poses, d_wg_chi, nullptr, d_Hpp, nullptr, d_bp, nullptr);
}

void launch_prior_add_schur(hipStream_t s, const cugo_prior_edges& ev, const double* d_poses, const int32_t* d_rowptr,
                            double* d_Hsc, double* d_bp, double* d_bsc, double* d_wg_chi)
{
    launch<PRIOR_SCHUR>(s, "k_prior_add_schur", ev, d_poses, d_wg_chi, nullptr, d_Hsc, d_rowptr, d_bp, d_bsc);
}

} // namespace cugo_k
