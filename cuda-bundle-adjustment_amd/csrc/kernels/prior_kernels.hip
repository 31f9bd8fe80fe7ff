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
    // (the stride as an opaque per-lane value: the 28 multiples of n the planar arrays are read at would otherwise
    //  each take a pair of scalar registers across the edge loop; 32-bit indices: 21 n stays far below 2^31)
    int stride = a.n;
    asm volatile("" : "+v"(stride));
    double qz[4], tz[3];
    {
        int i = e;
#pragma unroll
        for (int c = 0; c < 4; c++, i += stride)
            qz[c] = a.meas[i];
#pragma unroll
        for (int c = 0; c < 3; c++, i += stride)
            tz[c] = a.meas[i];
    }
    double R[3][3], Rz[3][3], D[3][3];
    quat_to_rot(pose, R);
    quat_to_rot(qz, Rz);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            D[i][j] = R[i][0] * Rz[j][0] + R[i][1] * Rz[j][1] + R[i][2] * Rz[j][2];
    // phi = theta / sin(theta) * vee(D - D^T) / 2, theta = atan2(|vee| / 2, (tr D - 1) / 2) in [0, pi]
    const double s0 = 0.5 * (D[2][1] - D[1][2]), s1 = 0.5 * (D[0][2] - D[2][0]), s2 = 0.5 * (D[1][0] - D[0][1]);
    const double sn = sqrt(s0 * s0 + s1 * s1 + s2 * s2);
    const double cs = 0.5 * (D[0][0] + D[1][1] + D[2][2] - 1.0);
    const double theta = atan2(sn, cs);
    const double f = sn > 1e-12 ? theta / sn : 1.0;
    double r[6];
    r[0] = f * s0, r[1] = f * s1, r[2] = f * s2;
#pragma unroll
    for (int i = 0; i < 3; i++)
        r[3 + i] = pose[4 + i] - (D[i][0] * tz[0] + D[i][1] * tz[1] + D[i][2] * tz[2]);
    // Omega, full symmetric
    double Om[6][6];
    {
        int at = a.n_info == 1 ? 0 : e;
        const int step = a.n_info == 1 ? 1 : stride;
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = i; j < 6; j++)
            {
                const double w = a.info[at];
                Om[i][j] = w, Om[j][i] = w;
                at += step;
            }
    }
    double Or[6]; // Omega r
#pragma unroll
    for (int i = 0; i < 6; i++)
    {
        double s = Om[i][0] * r[0];
#pragma unroll
        for (int j = 1; j < 6; j++)
            s += Om[i][j] * r[j];
        Or[i] = s;
    }
    double x = r[0] * Or[0];
#pragma unroll
    for (int i = 1; i < 6; i++)
        x += r[i] * Or[i];
    x = fmax(0.0, x);
    const double chi = rk_rho(a.rk, x);
    if (FULL)
    {
        const double w = rk_drho(a.rk, x);
        const double th2 = theta * theta;
        // (sn and cs ARE sin theta and cos theta: no call of sin / cos)
        const double c = theta < 1e-3 ? 1.0 / 12 + th2 * (1.0 / 720) : 1.0 / th2 - (1.0 + cs) / (2.0 * theta * sn);
        const double p0 = r[0], p1 = r[1], p2 = r[2];
        // [phi]x and its square
        const double K[3][3] = {{0.0, -p2, p1}, {p2, 0.0, -p0}, {-p1, p0, 0.0}};
        const double K2[3][3] = {{-(p1 * p1 + p2 * p2), p0 * p1, p0 * p2},
                                 {p0 * p1, -(p0 * p0 + p2 * p2), p1 * p2},
                                 {p0 * p2, p1 * p2, -(p0 * p0 + p1 * p1)}};
        double J[6][6];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++)
            {
                J[i][j] = (i == j ? 1.0 : 0.0) - 0.5 * K[i][j] + c * K2[i][j];
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
    __syncthreads();
    if (threadIdx.x == 0)
    {
        double tot = 0.0;
#pragma unroll
        for (int i = 0; i < PRIOR_POSES; i++)
            tot += s_chi[i];
        a.wg_chi[blockIdx.x] = tot;
    }
}

PriorArgs args_of(const cugo_prior_edges& ev, const double* d_poses, double* d_wg_chi, double* d_edge_chi)
{
    PriorArgs a;
    a.n = ev.n, a.n_poses_free = ev.n_poses_free;
    a.pose_ptr = ev.d_pose_ptr, a.meas = ev.d_meas, a.info = ev.d_info, a.n_info = ev.n_info;
    a.flags = ev.d_flags;
    a.rk = Robust{ev.rk, ev.delta};
    a.poses = d_poses;
    a.wg_chi = d_wg_chi, a.edge_chi = d_edge_chi;
    return a;
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
    const int wgs = prior_workgroups(ev);
    if (!wgs)
        return;
    const PriorArgs a = args_of(ev, d_poses, d_wg_chi, d_edge_chi);
    LaunchScope scope("k_prior_errors", s);
    hipLaunchKernelGGL(k_prior<PRIOR_ERRORS>, dim3(wgs), dim3(PRIOR_WG), 0, s, a, (double*)nullptr, (const int32_t*)nullptr,
                       (double*)nullptr, (double*)nullptr);
}

void launch_prior_add(hipStream_t s, const cugo_prior_edges& ev, const double* d_poses, double* d_Hpp, double* d_bp,
                      double* d_wg_chi)
{
    const int wgs = prior_workgroups(ev);
    if (!wgs)
        return;
    const PriorArgs a = args_of(ev, d_poses, d_wg_chi, nullptr);
    LaunchScope scope("k_prior_add", s);
    hipLaunchKernelGGL(k_prior<PRIOR_HPP>, dim3(wgs), dim3(PRIOR_WG), 0, s, a, d_Hpp, (const int32_t*)nullptr, d_bp,
                       (double*)nullptr);
}

void launch_prior_add_schur(hipStream_t s, const cugo_prior_edges& ev, const double* d_poses, const int32_t* d_rowptr,
                            double* d_Hsc, double* d_bp, double* d_bsc, double* d_wg_chi)
{
    const int wgs = prior_workgroups(ev);
    if (!wgs)
        return;
    const PriorArgs a = args_of(ev, d_poses, d_wg_chi, nullptr);
    LaunchScope scope("k_prior_add_schur", s);
    hipLaunchKernelGGL(k_prior<PRIOR_SCHUR>, dim3(wgs), dim3(PRIOR_WG), 0, s, a, d_Hsc, d_rowptr, d_bp, d_bsc);
}

} // namespace cugo_k
