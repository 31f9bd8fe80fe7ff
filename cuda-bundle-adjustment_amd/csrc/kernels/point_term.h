// The term of a point measured with a 3 x 3 information matrix, as the unary point kind (point_kernels.hip) and both
// ends of the pose-pose point kind (point_pair_kernels.hip) form it: a point u in the frame of a pose with the Jacobian
// [ S_u | I ], S_u = -[u]x (left update, tangent order [omega, upsilon]), and a symmetric O.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_math.h"

namespace cugo_dev
{

// r = y - z, O = Omega_e (its upper triangle row-major packed 00 01 02 11 12 22, [6][n] or one matrix for all edges,
// [6][1]: wave-uniform), q = Omega r, x = max(0, r^T Omega r).  Returns the chi2 term rho(x)
__device__ __forceinline__ double point_residual(const double (&y)[3], const double (&z)[3], const double* info,
                                                 int n_info, size_t n, int e, const Robust& rk, double (&O)[3][3], double (&q)[3],
                                                 double& x)
{
    const double r0 = y[0] - z[0], r1 = y[1] - z[1], r2 = y[2] - z[2];
    const size_t s = n_info == 1 ? 1 : n;
    const int i = n_info == 1 ? 0 : e;
    O[0][0] = info[i], O[0][1] = O[1][0] = info[s + i], O[0][2] = O[2][0] = info[2 * s + i];
    O[1][1] = info[3 * s + i], O[1][2] = O[2][1] = info[4 * s + i], O[2][2] = info[5 * s + i];
#pragma unroll
    for (int a = 0; a < 3; a++)
        q[a] = O[a][0] * r0 + O[a][1] * r1 + O[a][2] * r2;
    x = fmax(0.0, r0 * q[0] + r1 * q[1] + r2 * q[2]);
    return rk_rho(rk, x);
}

// v[0..20]: upper triangle, row-major packed, of w [S_u | I]^T O [S_u | I].  O S_u is formed once:
// H_ww = S_u^T (O S_u),  H_wv = (O S_u)^T,  H_vv = O
__device__ __forceinline__ void unary_block(const double (&u)[3], const double (&O)[3][3], double w, double (&v)[32])
{
    double G[3][3]; // O S_u: row a is u x (row a of O)
#pragma unroll
    for (int a = 0; a < 3; a++)
    {
        G[a][0] = O[a][2] * u[1] - O[a][1] * u[2];
        G[a][1] = O[a][0] * u[2] - O[a][2] * u[0];
        G[a][2] = O[a][1] * u[0] - O[a][0] * u[1];
    }
    // S_u^T (O S_u): row 0 = u1 G2. - u2 G1., row 1 = u2 G0. - u0 G2., row 2 = u0 G1. - u1 G0.
    v[0] = w * (u[1] * G[2][0] - u[2] * G[1][0]);
    v[1] = w * (u[1] * G[2][1] - u[2] * G[1][1]);
    v[2] = w * (u[1] * G[2][2] - u[2] * G[1][2]);
    v[6] = w * (u[2] * G[0][1] - u[0] * G[2][1]);
    v[7] = w * (u[2] * G[0][2] - u[0] * G[2][2]);
    v[11] = w * (u[0] * G[1][2] - u[1] * G[0][2]);
#pragma unroll
    for (int j = 0; j < 3; j++)
    {
        v[3 + j] = w * G[j][0];
        v[8 + j] = w * G[j][1];
        v[12 + j] = w * G[j][2];
    }
    v[15] = w * O[0][0], v[16] = w * O[0][1], v[17] = w * O[0][2];
    v[18] = w * O[1][1], v[19] = w * O[1][2], v[20] = w * O[2][2];
}

// v[21..26] = w (u x q, q): w [S_u | I]^T q.  The b of the build pass is MINUS this at the measured end (pass -w: the
// negation is exact) and plus this, at (p, M^T q), at the other end of a pair edge
__device__ __forceinline__ void unary_b(const double (&u)[3], const double (&q)[3], double w, double (&v)[32])
{
    v[21] = w * (u[1] * q[2] - u[2] * q[1]);
    v[22] = w * (u[2] * q[0] - u[0] * q[2]);
    v[23] = w * (u[0] * q[1] - u[1] * q[0]);
    v[24] = w * q[0], v[25] = w * q[1], v[26] = w * q[2];
}

} // namespace cugo_dev
