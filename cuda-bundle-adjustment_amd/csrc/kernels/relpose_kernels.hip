// Relative-pose SE(3) edges (include/relpose_types.h; an extension, the reference has no such edge): binary edges between
// poses a and b with an SE(3) measurement Z = (q_z, t_z) ~ T_a T_b^-1 and a full 6 x 6 information matrix Omega.
// Poses and update as in prior_kernels.hip (y = R(q) p + t, T <- Exp([omega, upsilon]) T, tangent order [omega, upsilon]).
//   R_A = R_a R_b^T,  t_A = t_a - R_A t_b                        (A = T_a T_b^-1)
//   R_D = R_A R_z^T,  t_D = t_A - R_D t_z                        (D = A Z^-1)
//   r   = [ phi ; t_D ],  phi = Log_SO3(R_D)
//   J_a = dr/dxi_a = [ J_l^-1(phi)  0 ]                          (the prior's J with this D)
//                    [ -[t_D]x      I ]
//   J_b = dr/dxi_b = -J_a Ad(A): Exp(xi) T_b turns A into A Exp(-xi) = Exp(-Ad(A) xi) A.  With Ad(A) = [ R_A 0 ;
//         [t_A]x R_A  R_A ] the product is
//         J_b = [ -J_l^-1(phi) R_A     0    ]
//               [ [t_D - t_A]x R_A    -R_A  ]                    (both Jacobians have a zero upper right block)
//   x = max(0, r^T Omega r), chi2 term rho(x), w = rho'(x)
//   H_aa += w J_a^T Omega J_a, H_bb += w J_b^T Omega J_b, H_(lo,hi) += w J_lo^T Omega J_hi, b_s -= w J_s^T Omega r
//
// Layout: the edges stay in the caller's order, structure of arrays (meas [7][n], Omega as its packed upper triangle
// [21][n] or [21][1]); the plan (csrc/host/relpose_plan.h) holds per free pose the list of its counting edges with the
// side each is seen from, and per edge the block index of its (lo, hi) block in an upper block CSR, or -1.
//
// The workload is small, so launches count: ONE kernel per pass.  One 64-lane wave owns a free pose (four poses per
// workgroup) and walks its list in edge order; every lane recomputes r and both Jacobians of an edge in registers
// (static indices only), picks the two columns it needs, multiplies one of them with Omega and forms the one element
// it owns:
//   lanes  0..20  entry t of the upper triangle of the pose's diagonal block,        sum_k J_self[k][i] (Omega J_self)[k][j]
//   lanes 21..26  entry t - 21 of b,                                                -sum_k J_self[k][i] (Omega r)[k]
//   lanes 27..62  entry (i, j) of the off-diagonal block, i + 6 j = t - 27,          sum_k J_self[k][i] (Omega J_other)[k][j]
// The diagonal term and b are summed over the walk and ADDED to their destination at its end.  The off-diagonal term
// belongs to the walk of pose lo (self < other, the other end free): there J_self = J_lo and J_other = J_hi whichever
// of a, b is lo, so the orientation of an edge needs no transposition; the lane ADDS its element to the block edge
// after edge (a lane re-reads what it wrote itself: program order), so several edges on one pair need no special case.
// No partials, no atomics, one fixed order.  chi2 is counted by ONE of the two walks that see an edge: that of a when a
// is free, else that of b; every workgroup leaves one chi2 total (its poses in order) and the error-only form walks the
// same lists, so its chi2 has the bits of the build pass's.  A pose whose list is empty or all flagged inactive keeps
// the bits of its blocks; fixed poses are never walked.
//
// The LM loop's two-stream form builds Hpp first and the Schur complement, which OVERWRITES every block of Hsc, later
// and possibly more than once (a retried trial).  There the build form gets no off-diagonal destination (Hoff null: its
// lanes 27..62 store nothing) and a fourth form, queued behind the Schur pass at the same poses, walks only the edges
// whose off-diagonal term belongs to the pose and adds lanes 27..62's element into Hsc by block index: the same terms in
// the same order as the Schur form adds them, no second Hsc-sized buffer, nothing else written (no chi2 totals).
#include <hip/hip_runtime.h>

#include "ba_math.h"
#include "kernels.h"

namespace
{

using namespace cugo_dev;

constexpr int RELPOSE_WG = 256;
constexpr int RELPOSE_LANES = 64;                         // lanes per pose: one wave
constexpr int RELPOSE_POSES = RELPOSE_WG / RELPOSE_LANES; // poses per workgroup

enum RelPoseMode
{
    RELPOSE_ERRORS = 0, // chi2 only
    RELPOSE_HPP = 1,    // + diagonal into Hpp [P][36], b into bp, off-diagonal into Hoff [nnzb][36] (or nowhere: Hoff null)
    RELPOSE_SCHUR = 2,  // + diagonal (through rowptr) and off-diagonal into Hsc, b into bp and bsc
    RELPOSE_OFFDIAG = 3 // the off-diagonal terms alone into Hoff (= Hsc) by block index; no chi2 totals
};

struct RelPoseArgs
{
    cugo_k::RelPosePlanDev plan;
    const double* meas; // [7][n]
    const double* info; // [21][n] or [21][1]
    int n_info;
    const uint8_t* flags;
    Robust rk;
    const double* poses;
    double* wg_chi;   // [workgroups]
    double* edge_chi; // [n] or nullptr (error pass)
};

// chi2 term of edge e between the poses pa (the edge's a) and pb (its b); with FULL also the element the lane owns,
// into `mine`: sum_k J_self[k][ri] Y[k][ci] times w (sign +1), Y = Omega J_self (use_other false), Omega J_other
// (use_other true) or, with ci == 6, Omega r (sign -1).  side: 0 self is a, 1 self is b (uniform over the wave).
// Both Jacobians live in registers under static indices; the lane's columns are picked by compare-and-select.
template <bool FULL>
__device__ __forceinline__ double relpose_edge(const RelPoseArgs& a, int e, const double* __restrict__ pa,
                                               const double* __restrict__ pb, int side, bool use_other, int ri, int ci,
                                               double sign, double& mine)
{
    double qz[4], tz[3];
    const int stride = se3_load_meas(a.meas, a.plan.n, e, qz, tz);
    double RA[3][3], tA[3], D[3][3];
    {
        double Ra[3][3], Rb[3][3], Rz[3][3];
        quat_to_rot(pa, Ra);
        quat_to_rot(pb, Rb);
        quat_to_rot(qz, Rz);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++)
                RA[i][j] = Ra[i][0] * Rb[j][0] + Ra[i][1] * Rb[j][1] + Ra[i][2] * Rb[j][2];
#pragma unroll
        for (int i = 0; i < 3; i++)
            tA[i] = pa[4 + i] - (RA[i][0] * pb[4] + RA[i][1] * pb[5] + RA[i][2] * pb[6]);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++)
                D[i][j] = RA[i][0] * Rz[j][0] + RA[i][1] * Rz[j][1] + RA[i][2] * Rz[j][2];
    }
    double r[6], sn, cs, theta;
    se3_residual(D, tA, tz, r, sn, cs, theta);
    double Om[6][6], Or[6];
    se3_load_info(a.info, a.n_info, e, stride, Om);
    const double x = se3_quadratic(Om, r, Or);
    const double chi = rk_rho(a.rk, x);
    if (FULL)
    {
        const double w = rk_drho(a.rk, x);
        // the 27 entries of J_a and of J_b that are not structurally zero: left half [6][3], lower right [3][3]
        double Jl[3][3];
        se3_jl_inv(r, theta, sn, cs, Jl);
        // [u]x with u = t_D - t_A
        const double u0 = r[3] - tA[0], u1 = r[4] - tA[1], u2 = r[5] - tA[2];
        const bool sb = side != 0; // self is b
        // XL [6][3], XR [3][3]: J_self; YL, YR: the Jacobian under Omega (J_self, or J_other for an off-diagonal lane)
        double XL[6][3], XR[3][3], YL[6][3], YR[3][3];
        const bool yb = sb != use_other; // Y is J_b
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++)
            {
                const double a_top = Jl[i][j];
                const double b_top = -(Jl[i][0] * RA[0][j] + Jl[i][1] * RA[1][j] + Jl[i][2] * RA[2][j]);
                // -[t_D]x
                const double a_bot = i == j ? 0.0
                                            : (i == 0 && j == 1)   ? r[5]
                                              : (i == 0 && j == 2) ? -r[4]
                                              : (i == 1 && j == 0) ? -r[5]
                                              : (i == 1 && j == 2) ? r[3]
                                              : (i == 2 && j == 0) ? r[4]
                                                                   : -r[3];
                // ([u]x R_A)[i][j]
                const double b_bot = i == 0   ? u1 * RA[2][j] - u2 * RA[1][j]
                                     : i == 1 ? u2 * RA[0][j] - u0 * RA[2][j]
                                              : u0 * RA[1][j] - u1 * RA[0][j];
                const double a_r = i == j ? 1.0 : 0.0;
                const double b_r = -RA[i][j];
                XL[i][j] = sb ? b_top : a_top, XL[3 + i][j] = sb ? b_bot : a_bot, XR[i][j] = sb ? b_r : a_r;
                YL[i][j] = yb ? b_top : a_top, YL[3 + i][j] = yb ? b_bot : a_bot, YR[i][j] = yb ? b_r : a_r;
            }
        // column ri of J_self and column ci of Y (ci == 6: r, whose Omega r gives b), picked before the product with
        // Omega: the lane needs one column of Omega Y only, 36 multiplications instead of 216
        double jc[6], yc[6];
#pragma unroll
        for (int k = 0; k < 6; k++)
        {
            double v = XL[k][0], y = YL[k][0];
            v = ri == 1 ? XL[k][1] : v, y = ci == 1 ? YL[k][1] : y;
            v = ri == 2 ? XL[k][2] : v, y = ci == 2 ? YL[k][2] : y;
            if (k < 3)
                v = ri >= 3 ? 0.0 : v, y = ci >= 3 ? 0.0 : y;
            else
            {
                v = ri == 3 ? XR[k - 3][0] : v, y = ci == 3 ? YR[k - 3][0] : y;
                v = ri == 4 ? XR[k - 3][1] : v, y = ci == 4 ? YR[k - 3][1] : y;
                v = ri == 5 ? XR[k - 3][2] : v, y = ci == 5 ? YR[k - 3][2] : y;
            }
            jc[k] = v, yc[k] = ci == 6 ? r[k] : y;
        }
        double oc[6]; // Omega yc
#pragma unroll
        for (int i = 0; i < 6; i++)
        {
            double s = Om[i][0] * yc[0];
#pragma unroll
            for (int k = 1; k < 6; k++)
                s += Om[i][k] * yc[k];
            oc[i] = s;
        }
        double sum = jc[0] * oc[0];
#pragma unroll
        for (int k = 1; k < 6; k++)
            sum += jc[k] * oc[k];
        mine = sign * (w * sum);
    }
    return chi;
}

template <int MODE>
__global__ __launch_bounds__(RELPOSE_WG) void k_relpose(RelPoseArgs a, double* H, double* Hoff, // (one array in the Schur form)
                                                         const int32_t* __restrict__ rowptr, double* __restrict__ bp,
                                                         double* __restrict__ bsc)
{
    __shared__ double s_chi[RELPOSE_POSES];
    const int g = threadIdx.x / RELPOSE_LANES, t = threadIdx.x % RELPOSE_LANES;
    const int p = blockIdx.x * RELPOSE_POSES + g;
    const int P = a.plan.n_poses_free;
    double mine = 0.0, chi = 0.0;
    bool any = false; // an edge of this pose counted
    // the element lane t owns (see the head of the file); lane 63 owns none
    int ri = 0, ci = 0;
    const bool is_b = t >= 21 && t < 27, is_off = t >= 27 && t < 63;
    if (t < 21)
        tri6_unpack(t, ri, ci);
    else if (is_b)
        ri = t - 21, ci = 6;
    else if (is_off)
        ri = (t - 27) % 6, ci = (t - 27) / 6;
    if (p < P)
    {
        const double* self = a.poses + 7 * (size_t)p;
        for (int k = a.plan.inc_ptr[p], k1 = a.plan.inc_ptr[p + 1]; k < k1; k++)
        {
            const int rec = a.plan.inc[k];
            const int e = rec >> 1, side = rec & 1;
            if (a.flags && (a.flags[e] & CUGO_EDGE_INACTIVE))
                continue;
            const int other = side ? a.plan.pose_a[e] : a.plan.pose_b[e];
            // chi2 belongs to the walk of a when a is free, else to that of b
            const bool counts_chi = side == 0 || other >= P;
            if (MODE == RELPOSE_ERRORS && !counts_chi)
                continue;
            if (MODE == RELPOSE_OFFDIAG && !(other < P && p < other))
                continue;
            const double* op = a.poses + 7 * (size_t)other;
            const double* pa = side ? op : self;
            const double* pb = side ? self : op;
            // the off-diagonal term belongs to the walk of lo
            const bool off = MODE != RELPOSE_ERRORS && other < P && p < other;
            double term = 0.0;
            // (opaque copies, as in k_prior: the compare masks of the column selects are formed per edge instead of
            //  being kept in scalar registers across the loop)
            int ri_e = ri, ci_e = ci;
            asm volatile("" : "+v"(ri_e), "+v"(ci_e));
            const double c = relpose_edge<MODE != RELPOSE_ERRORS>(a, e, pa, pb, side, is_off, ri_e, ci_e, is_b ? -1.0 : 1.0, term);
            any = true;
            if (MODE != RELPOSE_OFFDIAG && counts_chi)
            {
                chi += c;
                if (MODE == RELPOSE_ERRORS && a.edge_chi && t == 0)
                    a.edge_chi[e] = c;
            }
            if (MODE != RELPOSE_ERRORS)
            {
                if (!is_off)
                    mine += term;
                else if (off && Hoff)
                    Hoff[36 * (size_t)a.plan.off_blk[e] + (t - 27)] += term;
            }
        }
    }
    if (MODE == RELPOSE_OFFDIAG)
        return;
    if (t == 0)
        s_chi[g] = chi;
    if (MODE != RELPOSE_ERRORS && any)
        pose_term_add<MODE == RELPOSE_SCHUR>(p, t, ri, ci, mine, H, rowptr, bp, bsc);
    pose_groups_chi_total<RELPOSE_POSES>(s_chi, a.wg_chi);
}

template <int MODE>
void launch(hipStream_t s, const char* label, const cugo_relpose_edges& ev, const cugo_k::RelPosePlanDev& plan,
            const double* d_poses, double* d_wg_chi, double* d_edge_chi, double* d_H, double* d_Hoff, const int32_t* d_rowptr,
            double* d_bp, double* d_bsc)
{
    const int wgs = cugo_k::relpose_workgroups(ev);
    if (!wgs)
        return;
    RelPoseArgs a;
    a.plan = plan;
    a.meas = ev.d_meas, a.info = ev.d_info, a.n_info = ev.n_info;
    a.flags = ev.d_flags;
    a.rk = Robust{ev.rk, ev.delta};
    a.poses = d_poses;
    a.wg_chi = d_wg_chi, a.edge_chi = d_edge_chi;
    cugo_k::LaunchScope scope(label, s);
    hipLaunchKernelGGL(k_relpose<MODE>, dim3(wgs), dim3(RELPOSE_WG), 0, s, a, d_H, d_Hoff, d_rowptr, d_bp, d_bsc);
}

} // namespace

namespace cugo_k
{

int relpose_workgroups(const cugo_relpose_edges& ev)
{
    return ev.n > 0 && ev.n_poses_free > 0 ? (ev.n_poses_free + RELPOSE_POSES - 1) / RELPOSE_POSES : 0;
}

void launch_relpose_errors(hipStream_t s, const cugo_relpose_edges& ev, const RelPosePlanDev& plan, const double* d_poses,
                           double* d_wg_chi, double* d_edge_chi)
{
    launch<RELPOSE_ERRORS>(s, "k_relpose_errors", ev, plan, d_poses, d_wg_chi, d_edge_chi, nullptr, nullptr, nullptr, nullptr,
                           nullptr);
}

void launch_relpose_add(hipStream_t s, const cugo_relpose_edges& ev, const RelPosePlanDev& plan, const double* d_poses,
                        double* d_Hpp, double* d_bp, double* d_Hoff, double* d_wg_chi)
{
    launch<RELPOSE_HPP>(s, "k_relpose_add", ev, plan, d_poses, d_wg_chi, nullptr, d_Hpp, d_Hoff, nullptr, d_bp, nullptr);
}

void launch_relpose_add_schur(hipStream_t s, const cugo_relpose_edges& ev, const RelPosePlanDev& plan, const double* d_poses,
                              const int32_t* d_rowptr, double* d_Hsc, double* d_bp, double* d_bsc, double* d_wg_chi)
{
    launch<RELPOSE_SCHUR>(s, "k_relpose_add_schur", ev, plan, d_poses, d_wg_chi, nullptr, d_Hsc, d_Hsc, d_rowptr, d_bp, d_bsc);
}

void launch_relpose_add_offdiag(hipStream_t s, const cugo_relpose_edges& ev, const RelPosePlanDev& plan, const double* d_poses,
                                double* d_Hsc)
{
    launch<RELPOSE_OFFDIAG>(s, "k_relpose_add_offdiag", ev, plan, d_poses, nullptr, nullptr, nullptr, d_Hsc, nullptr, nullptr,
                            nullptr);
}

} // namespace cugo_k
