// The term of a point measured with a 3 x 3 information matrix, as the unary point kind (point_kernels.hip) and both
// ends of the pose-pose point kind (point_pair_kernels.hip) form it: a point u in the frame of a pose with the Jacobian
// [ S_u | I ], S_u = -[u]x (left update, tangent order [omega, upsilon]), and a symmetric O.
//
// Two forms of O, a compile-time parameter (COV) of point_residual and of the edge functions above it:
//   information form   O is given (the upper triangle of Omega_e)
//   covariance form    O = (C_z + M C_p M^T)^-1 is formed from two covariances at the poses the pass is given (generalised
//                      ICP): M = R for the unary kind, M = R_b R_a^T for the pair kind.  The Jacobian does NOT
//                      differentiate Omega (no GICP implementation does), and log det is not part of the cost.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_math.h"

namespace cugo_dev
{

// upper triangle of a symmetric 3 x 3 matrix, row-major packed 00 01 02 11 12 22, [6][n] or one matrix for all edges,
// [6][1] (wave-uniform), mirrored into A
__device__ __forceinline__ void load_sym3(const double* tri, int n_tri, size_t n, int e, double (&A)[3][3])
{
    const size_t s = n_tri == 1 ? 1 : n;
    const int i = n_tri == 1 ? 0 : e;
    A[0][0] = tri[i], A[0][1] = A[1][0] = tri[s + i], A[0][2] = A[2][0] = tri[2 * s + i];
    A[1][1] = tri[3 * s + i], A[1][2] = A[2][1] = tri[4 * s + i], A[2][2] = tri[5 * s + i];
}

// O = (C_z + M C_p M^T)^-1.  S is formed as an upper triangle (T = M C_p, S_ij = C_z,ij + T_i. . M_j.), so O is exactly
// symmetric; S = L L^T, L^-1, O = L^-T L^-1 (the 3 x 3 factorisation k_build_edges uses for Hll + lambda I: its
// componentwise error is a small multiple of u |O| |S|a |O|, the adjugate's is not).  The values are the caller's: an S
// that is not positive definite gives NaNs.  One operation order for every caller: the four roles of a pair edge and
// the error pass form the same bits
__device__ __forceinline__ void cov_information(const double (&M)[3][3], const double* cov_p, const double* cov_z, int n_cov,
                                                size_t n, int e, double (&O)[3][3])
{
    double Cp[3][3], Cz[3][3], T[3][3];
    load_sym3(cov_p, n_cov, n, e, Cp);
    load_sym3(cov_z, n_cov, n, e, Cz);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            T[i][j] = M[i][0] * Cp[0][j] + M[i][1] * Cp[1][j] + M[i][2] * Cp[2][j];
    const double s00 = Cz[0][0] + (T[0][0] * M[0][0] + T[0][1] * M[0][1] + T[0][2] * M[0][2]);
    const double s01 = Cz[0][1] + (T[0][0] * M[1][0] + T[0][1] * M[1][1] + T[0][2] * M[1][2]);
    const double s02 = Cz[0][2] + (T[0][0] * M[2][0] + T[0][1] * M[2][1] + T[0][2] * M[2][2]);
    const double s11 = Cz[1][1] + (T[1][0] * M[1][0] + T[1][1] * M[1][1] + T[1][2] * M[1][2]);
    const double s12 = Cz[1][2] + (T[1][0] * M[2][0] + T[1][1] * M[2][1] + T[1][2] * M[2][2]);
    const double s22 = Cz[2][2] + (T[2][0] * M[2][0] + T[2][1] * M[2][1] + T[2][2] * M[2][2]);
    const double l00 = sqrt(s00);
    const double i00 = 1.0 / l00;
    const double l10 = s01 * i00, l20 = s02 * i00;
    const double l11 = sqrt(s11 - l10 * l10);
    const double i11 = 1.0 / l11;
    const double l21 = (s12 - l20 * l10) * i11;
    const double l22 = sqrt(s22 - l20 * l20 - l21 * l21);
    const double i22 = 1.0 / l22;
    const double i10 = -(l10 * i00) * i11;
    const double i21 = -(l21 * i11) * i22;
    const double i20 = -(l20 * i00 + l21 * i10) * i22;
    O[0][0] = i00 * i00 + i10 * i10 + i20 * i20;
    O[0][1] = O[1][0] = i10 * i11 + i20 * i21;
    O[0][2] = O[2][0] = i20 * i22;
    O[1][1] = i11 * i11 + i21 * i21;
    O[1][2] = O[2][1] = i21 * i22;
    O[2][2] = i22 * i22;
}

// r = y - z, q = Omega r, x = max(0, r^T Omega r).  Returns the chi2 term rho(x).  Information form: O = Omega_e from
// `info` (load_sym3's layout).  Covariance form: `info` is cov_p, n_info its count, and O = cov_information(M, ...)
template <bool COV = false>
__device__ __forceinline__ double point_residual(const double (&y)[3], const double (&z)[3], const double* info,
                                                 int n_info, size_t n, int e, const Robust& rk, double (&O)[3][3], double (&q)[3],
                                                 double& x, const double* cov_z = nullptr, const double (*M)[3][3] = nullptr)
{
    const double r0 = y[0] - z[0], r1 = y[1] - z[1], r2 = y[2] - z[2];
    if constexpr (COV)
        cov_information(*M, info, cov_z, n_info, n, e, O);
    else
        load_sym3(info, n_info, n, e, O);
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
