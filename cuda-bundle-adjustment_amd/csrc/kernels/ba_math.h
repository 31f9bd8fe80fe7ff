// Device-side geometry for the BA kernels (gfx950).  fp64 throughout.
// Formulas restate SURVEY.md Appendix A; citations "ref:" are into the reference repo.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cugo_dev
{

struct Robust
{
    int type;
    double delta;
};

// ref: src/cuda/cuda_block_solver.cu:972-1027
__device__ __forceinline__ double rk_rho(const Robust rk, double x)
{
    const double d2 = rk.delta * rk.delta;
    if (rk.type == 2)
    {
        const double u = 1.0 - x / d2;
        const double mx = (1.0 / 3) * d2;
        return x <= d2 ? mx * (1.0 - u * u * u) : mx;
    }
    if (rk.type == 1)
        return d2 * log((1.0 / d2) * x + 1.0);
    if (rk.type == 3) // Huber (not in the reference's enum; g2o RobustKernelHuber, what ORB-SLAM2 uses)
        return x <= d2 ? x : 2.0 * rk.delta * sqrt(x) - d2;
    return x;
}
__device__ __forceinline__ double rk_drho(const Robust rk, double x)
{
    const double d2 = rk.delta * rk.delta;
    if (rk.type == 2)
    {
        const double u = 1.0 - x / d2;
        return x <= d2 ? u * u : 0.0;
    }
    if (rk.type == 1)
        return 1.0 / ((1.0 / d2) * x + 1.0);
    if (rk.type == 3)
        return x <= d2 ? 1.0 : rk.delta / sqrt(x);
    return 1.0;
}

struct EdgeGeom
{
    double Xc[3];
    double e[3]; // e[2] = 0 for mono
    double w;    // omega * rho'
    double chi;  // rho(omega |e|^2)
};

// Xc = R(q) Xw + t in the cross-product form (ref: .cu:379-402)
__device__ __forceinline__ void world_to_cam(const double* __restrict__ pose,
                                             const double* __restrict__ Xw, double* Xc)
{
    const double qx = pose[0], qy = pose[1], qz = pose[2], qw = pose[3];
    double t1x = qy * Xw[2] - qz * Xw[1];
    double t1y = qz * Xw[0] - qx * Xw[2];
    double t1z = qx * Xw[1] - qy * Xw[0];
    t1x += t1x;
    t1y += t1y;
    t1z += t1z;
    const double t2x = qy * t1z - qz * t1y;
    const double t2y = qz * t1x - qx * t1z;
    const double t2z = qx * t1y - qy * t1x;
    Xc[0] = Xw[0] + qw * t1x + t2x + pose[4];
    Xc[1] = Xw[1] + qw * t1y + t2y + pose[5];
    Xc[2] = Xw[2] + qw * t1z + t2z + pose[6];
}

// The kind of a pose-landmark slot: mono, stereo, or (DEP only) inverse depth (DepthEdge) with the
// third residual sd (1/Z - m_d), sd = sqrt(inverse-depth weight); at most one of stereo and depth is set.  DEP = false
// is what `bool stereo` has always said: those instantiations hold the code of the overloads that take the bool alone,
// operation by operation, and never read depth or sd.  Only the kernels for edge arrays that may hold depth slots are
// built with DEP.  (The kind travels as scalars: a one-byte struct handed through these functions ends up in LDS.)

// residual (proj - meas), weight and chi for one edge (ref: .cu:410-424, 1100-1109, 1190-1192); mr is the third
// measurement: u_right of a stereo slot, 1/Z of a depth slot
template <bool DEP>
__device__ __forceinline__ void edge_residual_k(const double* __restrict__ pose,
                                                const double* __restrict__ Xw, double mu, double mv,
                                                double mr, bool stereo, bool depth, double sd, double omega,
                                                const double* __restrict__ cam, const Robust rk,
                                                EdgeGeom& g)
{
    world_to_cam(pose, Xw, g.Xc);
    const double invZ = 1.0 / g.Xc[2];
    const double pu = cam[0] * invZ * g.Xc[0] + cam[2];
    const double pv = cam[1] * invZ * g.Xc[1] + cam[3];
    g.e[0] = pu - mu;
    g.e[1] = pv - mv;
    double sq = g.e[0] * g.e[0] + g.e[1] * g.e[1];
    if (stereo)
    {
        g.e[2] = (pu - cam[4] * invZ) - mr;
        sq += g.e[2] * g.e[2];
    }
    else
    {
        g.e[2] = 0.0;
        if constexpr (DEP)
            if (depth)
            {
                g.e[2] = sd * (invZ - mr);
                sq += g.e[2] * g.e[2];
            }
    }
    const double x = omega * sq;
    g.chi = rk_rho(rk, x);
    g.w = omega * rk_drho(rk, x);
}
__device__ __forceinline__ void edge_residual(const double* __restrict__ pose,
                                              const double* __restrict__ Xw, double mu, double mv,
                                              double mr, bool stereo, double omega,
                                              const double* __restrict__ cam, const Robust rk,
                                              EdgeGeom& g)
{
    edge_residual_k<false>(pose, Xw, mu, mv, mr, stereo, false, 0.0, omega, cam, rk, g);
}

// rotation matrix rows from quaternion (ref: .cu:449-478). R[r][c]
__device__ __forceinline__ void quat_to_rot(const double* __restrict__ q, double R[3][3])
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0][0] = 1 - (tyy + tzz);
    R[0][1] = txy - twz;
    R[0][2] = txz + twy;
    R[1][0] = txy + twz;
    R[1][1] = 1 - (txx + tzz);
    R[1][2] = tyz - twx;
    R[2][0] = txz - twy;
    R[2][1] = tyz + twx;
    R[2][2] = 1 - (txx + tyy);
}

// Pose Jacobian rows JP[m][6] (m < dim); third row zero for mono. ref: .cu:491-578
// Depth: rows 0 and 1 are the mono rows, JP[2] = s/Z^2 (Y, -X, 0, 0, 0, 1) — minus the derivative of s/Z, as the
// stereo row is JP[0] - bf/Z^2 dZ/dxi with dZ/dxi = (Y, -X, 0, 0, 0, 1)
template <bool DEP>
__device__ __forceinline__ void jac_pose_k(const double* Xc, const double* __restrict__ cam,
                                           bool stereo, bool depth, double sd, double JP[3][6])
{
    const double X = Xc[0], Y = Xc[1], Z = Xc[2];
    const double invZ = 1.0 / Z;
    const double fu = cam[0], fv = cam[1];
    if (!stereo)
    {
        const double x = invZ * X, y = invZ * Y;
        const double fu_iz = fu * invZ, fv_iz = fv * invZ;
        JP[0][0] = fu * x * y;
        JP[0][1] = -fu * (1 + x * x);
        JP[0][2] = fu * y;
        JP[0][3] = -fu_iz;
        JP[0][4] = 0;
        JP[0][5] = fu_iz * x;
        JP[1][0] = fv * (1 + y * y);
        JP[1][1] = -fv * x * y;
        JP[1][2] = -fv * x;
        JP[1][3] = 0;
        JP[1][4] = -fv_iz;
        JP[1][5] = fv_iz * y;
#pragma unroll
        for (int c = 0; c < 6; c++)
            JP[2][c] = 0;
        if constexpr (DEP)
            if (depth)
            {
                const double sZZ = sd * (invZ * invZ);
                JP[2][0] = sZZ * Y;
                JP[2][1] = -(sZZ * X);
                JP[2][5] = sZZ;
            }
    }
    else
    {
        const double iZZ = invZ * invZ, bf = cam[4];
        JP[0][0] = X * Y * iZZ * fu;
        JP[0][1] = -(1 + (X * X * iZZ)) * fu;
        JP[0][2] = Y * invZ * fu;
        JP[0][3] = -1 * invZ * fu;
        JP[0][4] = 0;
        JP[0][5] = X * iZZ * fu;
        JP[1][0] = (1 + Y * Y * iZZ) * fv;
        JP[1][1] = -X * Y * iZZ * fv;
        JP[1][2] = -X * invZ * fv;
        JP[1][3] = 0;
        JP[1][4] = -1 * invZ * fv;
        JP[1][5] = Y * iZZ * fv;
        JP[2][0] = JP[0][0] - bf * Y * iZZ;
        JP[2][1] = JP[0][1] + bf * X * iZZ;
        JP[2][2] = JP[0][2];
        JP[2][3] = JP[0][3];
        JP[2][4] = 0;
        JP[2][5] = JP[0][5] - bf * iZZ;
    }
}
__device__ __forceinline__ void jac_pose(const double* Xc, const double* __restrict__ cam,
                                         bool stereo, double JP[3][6])
{
    jac_pose_k<false>(Xc, cam, stereo, false, 0.0, JP);
}

// Landmark Jacobian rows JL[m][3] from the rotation matrix of the pose. ref: .cu:508-513, 546-556
// Depth: JL[2][j] = s/Z^2 R[2][j]
template <bool DEP>
__device__ __forceinline__ void jac_landmark_R_k(const double* Xc, const double R[3][3],
                                                 const double* __restrict__ cam, bool stereo, bool depth, double sd,
                                                 double JL[3][3])
{
    const double X = Xc[0], Y = Xc[1], Z = Xc[2];
    const double invZ = 1.0 / Z;
    const double fu = cam[0], fv = cam[1];
    if (!stereo)
    {
        const double x = invZ * X, y = invZ * Y;
        const double fu_iz = fu * invZ, fv_iz = fv * invZ;
#pragma unroll
        for (int j = 0; j < 3; j++)
        {
            JL[0][j] = -fu_iz * (R[0][j] - x * R[2][j]);
            JL[1][j] = -fv_iz * (R[1][j] - y * R[2][j]);
            JL[2][j] = 0;
        }
        if constexpr (DEP)
            if (depth)
            {
                const double sZZ = sd * (invZ * invZ);
#pragma unroll
                for (int j = 0; j < 3; j++)
                    JL[2][j] = sZZ * R[2][j];
            }
    }
    else
    {
        const double iZZ = invZ * invZ, bf = cam[4];
#pragma unroll
        for (int j = 0; j < 3; j++)
        {
            JL[0][j] = -fu * R[0][j] * invZ + fu * X * R[2][j] * iZZ;
            JL[1][j] = -fv * R[1][j] * invZ + fv * Y * R[2][j] * iZZ;
            JL[2][j] = JL[0][j] - bf * R[2][j] * iZZ;
        }
    }
}
__device__ __forceinline__ void jac_landmark_R(const double* Xc, const double R[3][3],
                                               const double* __restrict__ cam, bool stereo,
                                               double JL[3][3])
{
    jac_landmark_R_k<false>(Xc, R, cam, stereo, false, 0.0, JL);
}
template <bool DEP>
__device__ __forceinline__ void jac_landmark_k(const double* Xc, const double* __restrict__ q,
                                               const double* __restrict__ cam, bool stereo, bool depth, double sd,
                                               double JL[3][3])
{
    double R[3][3];
    quat_to_rot(q, R);
    jac_landmark_R_k<DEP>(Xc, R, cam, stereo, depth, sd, JL);
}
__device__ __forceinline__ void jac_landmark(const double* Xc, const double* __restrict__ q,
                                             const double* __restrict__ cam, bool stereo,
                                             double JL[3][3])
{
    jac_landmark_k<false>(Xc, q, cam, stereo, false, 0.0, JL);
}

// ---- camera extrinsics (rig) ---------------------------------------------------------------
// The pose vertex is world -> body; a camera-table entry carries a fixed sensor pose T_sb = (M, t_s), body -> sensor,
// as 12 doubles {M row-major, t_s}:  Xb = R(q) Xw + t (world_to_cam, unchanged),  Xs = M Xb + t_s.  The residual is the
// one above evaluated at Xs; EdgeGeom::Xc (and with it the 64-byte record) keeps holding Xb.  With
//   A = JP[:, 3:6] of jac_pose at Xs  (= -de/dXs),   B = A M:
//   JP[:, 3:6] = B,   JP[:, 0:3] = -B [Xb]x   (left update T_b <- exp([w, v]) T_b),   JL = B R(q).
// Only the rig-aware instantiations of the kernels (cugo_edges.has_rig != 0) hold this code; every pass that needs
// Xs or B forms them with the functions below, so the record forms repeat the build pass's bits.
__device__ __forceinline__ void body_to_sensor(const double* __restrict__ ext, const double* Xb, double Xs[3])
{
#pragma unroll
    for (int r = 0; r < 3; r++)
        Xs[r] = ext[3 * r] * Xb[0] + ext[3 * r + 1] * Xb[1] + ext[3 * r + 2] * Xb[2] + ext[9 + r];
}

// ---- Kannala-Brandt fisheye entries ---------------------------------------------------------
// A camera-table entry of a MODEL table (cugo_edges.has_rig == CUGO_RIG_MODELS) is 17 doubles: the 12 above, then
// k1..k4 and the model flag (0.0 pinhole, 1.0 Kannala-Brandt).  For a Kannala-Brandt entry, at Xs = (x, y, z):
//   r2 = x^2 + y^2,  R2 = r2 + z^2,  th = atan2(r, z),  t2 = th^2
//   P = 1 + k1 t2 + k2 t2^2 + k3 t2^3 + k4 t2^4          (theta_d = th P)
//   Q = dP/dt2 = k1 + 2 k2 t2 + 3 k3 t2^2 + 4 k4 t2^3,   D = d theta_d / d th = P + 2 t2 Q
//   g = th / r  (1 / z at r == 0),   rho = g P,   pu = fx rho x + cx,   pv = fy rho y + cy
//   c = (D z / R2 - rho) / r2                                                   th >= KB_NEAR_AXIS
//   c = g^2 (4 g P S(4 t2) + 2 Q z / R2),  S(w) = sum_{n>=1} (-1)^n w^(n-1) / (2n+1)!   th <  KB_NEAR_AXIS
// The second form is the first with  z / R2 - th / r = (sin 2th - 2th) / (2 r)  expanded: no difference of nearly equal
// terms and no division by r, so it holds at r == 0 (c = -2 / (3 z^3) for k = 0).  Below the switch z > 0; above it
// nothing divides by z.  The switch and the nine terms of S: DESIGN.md section 19.
constexpr double KB_NEAR_AXIS = 0.5; // rad
struct KbTerms
{
    double rho, c, dR; // dR = D / R2
};
__device__ __forceinline__ KbTerms kb_terms(const double* Xs, const double* __restrict__ k)
{
    const double x = Xs[0], y = Xs[1], z = Xs[2];
    const double r2 = x * x + y * y;
    const double r = sqrt(r2);
    const double R2 = r2 + z * z;
    const double th = atan2(r, z);
    const double t2 = th * th;
    const double P = 1.0 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3])));
    const double Q = k[0] + t2 * (2.0 * k[1] + t2 * (3.0 * k[2] + t2 * (4.0 * k[3])));
    const double D = P + 2.0 * t2 * Q;
    const double g = r > 0.0 ? th / r : 1.0 / z;
    KbTerms o;
    o.rho = g * P;
    o.dR = D / R2;
    if (th < KB_NEAR_AXIS)
    {
        const double w = 4.0 * t2;
        // S(w), n = 9 down to 1: (-1)^n / (2n+1)!
        double S = -1.0 / 121645100408832000.0;
        S = S * w + 1.0 / 355687428096000.0;
        S = S * w - 1.0 / 1307674368000.0;
        S = S * w + 1.0 / 6227020800.0;
        S = S * w - 1.0 / 39916800.0;
        S = S * w + 1.0 / 362880.0;
        S = S * w - 1.0 / 5040.0;
        S = S * w + 1.0 / 120.0;
        S = S * w - 1.0 / 6.0;
        o.c = (g * g) * (4.0 * g * P * S + 2.0 * Q * (z / R2));
    }
    else
        o.c = (o.dR * z - o.rho) / r2;
    return o;
}

// ---- radial-tangential distortion entries ---------------------------------------------------
// A camera-table entry of a DISTORTION table (cugo_edges.has_rig == CUGO_RIG_DISTORTION) is 18 doubles: the 12 of the
// extrinsic, then (k1, k2, p1, p2, k3) in OpenCV's order and the flag (0.0 undistorted, 1.0 distorted).  For a distorted
// entry, at Xs = (x, y, z):
//   iz = 1 / z,  a = x iz,  b = y iz,  r2 = a^2 + b^2
//   rad = 1 + r2 (k1 + r2 (k2 + r2 k3)),   dr = d rad / d r2 = k1 + r2 (2 k2 + 3 k3 r2)
//   a' = a rad + 2 p1 a b + p2 (r2 + 2 a^2),   b' = b rad + p1 (r2 + 2 b^2) + 2 p2 a b
//   pu = fx a' + cx,  pv = fy b' + cy
//   Jaa = rad + 2 a^2 dr + 2 p1 b + 6 p2 a,   Jab = 2 a b dr + 2 p1 a + 2 p2 b,   Jbb = rad + 2 b^2 dr + 6 p1 b + 2 p2 a
// Nothing here subtracts nearly equal numbers: one form, no near-axis branch.  z <= 0 is the caller's, as for the pinhole.
struct DistTerms
{
    double a, b, ad, bd, Jaa, Jab, Jbb, iz; // (ad, bd) = (a', b')
};
__device__ __forceinline__ DistTerms dist_terms(const double* Xs, const double* __restrict__ d)
{
    const double k1 = d[0], k2 = d[1], p1 = d[2], p2 = d[3], k3 = d[4];
    DistTerms o;
    o.iz = 1.0 / Xs[2];
    o.a = Xs[0] * o.iz;
    o.b = Xs[1] * o.iz;
    const double a2 = o.a * o.a, b2 = o.b * o.b, ab = o.a * o.b;
    const double r2 = a2 + b2;
    const double rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3));
    const double dr = k1 + r2 * (2.0 * k2 + 3.0 * k3 * r2);
    o.ad = o.a * rad + 2.0 * p1 * ab + p2 * (r2 + 2.0 * a2);
    o.bd = o.b * rad + p1 * (r2 + 2.0 * b2) + 2.0 * p2 * ab;
    o.Jaa = rad + 2.0 * a2 * dr + 2.0 * p1 * o.b + 6.0 * p2 * o.a;
    o.Jab = 2.0 * ab * dr + 2.0 * p1 * o.a + 2.0 * p2 * o.b;
    o.Jbb = rad + 2.0 * b2 * dr + 6.0 * p1 * o.b + 2.0 * p2 * o.a;
    return o;
}

// residual, weight and chi of a mono or stereo slot seen through the extrinsic; g.Xc = Xb.
// KB: ext is an entry of a model table (17 doubles); an entry whose flag is 0 takes the path below, operation for
// operation.  A Kannala-Brandt entry has no third row: bf means nothing there and the stereo bit is not looked at.
// DIST: ext is an entry of a distortion table (18 doubles), likewise: flag 0 takes the path below, a distorted entry has
// two rows.  Never together with KB: the two are different tables.
template <bool KB = false, bool DIST = false>
__device__ __forceinline__ void edge_residual_rig(const double* __restrict__ pose, const double* __restrict__ Xw,
                                                  double mu, double mv, double mr, bool stereo, double omega,
                                                  const double* __restrict__ cam, const double* __restrict__ ext,
                                                  const Robust rk, EdgeGeom& g)
{
    world_to_cam(pose, Xw, g.Xc);
    double Xs[3];
    body_to_sensor(ext, g.Xc, Xs);
    if constexpr (KB)
        if (ext[16] != 0.0)
        {
            const KbTerms kt = kb_terms(Xs, ext + 12);
            g.e[0] = (cam[0] * kt.rho * Xs[0] + cam[2]) - mu;
            g.e[1] = (cam[1] * kt.rho * Xs[1] + cam[3]) - mv;
            g.e[2] = 0.0;
            const double xk = omega * (g.e[0] * g.e[0] + g.e[1] * g.e[1]);
            g.chi = rk_rho(rk, xk);
            g.w = omega * rk_drho(rk, xk);
            return;
        }
    if constexpr (DIST)
        if (ext[17] != 0.0)
        {
            const DistTerms dt = dist_terms(Xs, ext + 12);
            g.e[0] = (cam[0] * dt.ad + cam[2]) - mu;
            g.e[1] = (cam[1] * dt.bd + cam[3]) - mv;
            g.e[2] = 0.0;
            const double xk = omega * (g.e[0] * g.e[0] + g.e[1] * g.e[1]);
            g.chi = rk_rho(rk, xk);
            g.w = omega * rk_drho(rk, xk);
            return;
        }
    const double invZ = 1.0 / Xs[2];
    const double pu = cam[0] * invZ * Xs[0] + cam[2];
    const double pv = cam[1] * invZ * Xs[1] + cam[3];
    g.e[0] = pu - mu;
    g.e[1] = pv - mv;
    double sq = g.e[0] * g.e[0] + g.e[1] * g.e[1];
    if (stereo)
    {
        g.e[2] = (pu - cam[4] * invZ) - mr;
        sq += g.e[2] * g.e[2];
    }
    else
        g.e[2] = 0.0;
    const double x = omega * sq;
    g.chi = rk_rho(rk, x);
    g.w = omega * rk_drho(rk, x);
}

// B = A M from the body-frame point (third row zero for mono).  live = false: zeros, SELECTED — the record of an
// inactive slot holds Xb = (0, 0, 1) and weight 0, which is a finite point for the plain Jacobians but may have
// Z_s = 0 behind a sensor pose, and 0 x inf would not do
// KB: as for edge_residual_rig; for a Kannala-Brandt entry A = -d(pu, pv)/dXs, third row zero:
//   A[0] = -fx (rho + x^2 c,  x y c,  -x D / R2),   A[1] = -fy (x y c,  rho + y^2 c,  -y D / R2)
// DIST: for a distorted entry A = -d(pu, pv)/dXs, third row zero:
//   A[0] = -fx iz (Jaa,  Jab,  -(Jaa a + Jab b)),   A[1] = -fy iz (Jab,  Jbb,  -(Jab a + Jbb b))
template <bool KB = false, bool DIST = false>
__device__ __forceinline__ void rig_B(const double* Xb, const double* __restrict__ cam,
                                      const double* __restrict__ ext, bool stereo, bool live, double B[3][3])
{
    double Xs[3];
    body_to_sensor(ext, Xb, Xs);
    if constexpr (KB)
        if (ext[16] != 0.0)
        {
            const KbTerms kt = kb_terms(Xs, ext + 12);
            const double xc = Xs[0] * kt.c, yc = Xs[1] * kt.c;
            double A[2][3];
            A[0][0] = -(cam[0] * (kt.rho + Xs[0] * xc));
            A[0][1] = -(cam[0] * (Xs[1] * xc));
            A[0][2] = cam[0] * (Xs[0] * kt.dR);
            A[1][0] = -(cam[1] * (Xs[0] * yc));
            A[1][1] = -(cam[1] * (kt.rho + Xs[1] * yc));
            A[1][2] = cam[1] * (Xs[1] * kt.dR);
#pragma unroll
            for (int j = 0; j < 3; j++)
            {
                const double b0 = A[0][0] * ext[j] + A[0][1] * ext[3 + j] + A[0][2] * ext[6 + j];
                const double b1 = A[1][0] * ext[j] + A[1][1] * ext[3 + j] + A[1][2] * ext[6 + j];
                B[0][j] = live ? b0 : 0.0;
                B[1][j] = live ? b1 : 0.0;
                B[2][j] = 0.0;
            }
            return;
        }
    if constexpr (DIST)
        if (ext[17] != 0.0)
        {
            const DistTerms dt = dist_terms(Xs, ext + 12);
            const double fu = -(cam[0] * dt.iz), fv = -(cam[1] * dt.iz);
            double A[2][3];
            A[0][0] = fu * dt.Jaa;
            A[0][1] = fu * dt.Jab;
            A[0][2] = -(fu * (dt.Jaa * dt.a + dt.Jab * dt.b));
            A[1][0] = fv * dt.Jab;
            A[1][1] = fv * dt.Jbb;
            A[1][2] = -(fv * (dt.Jab * dt.a + dt.Jbb * dt.b));
#pragma unroll
            for (int j = 0; j < 3; j++)
            {
                const double b0 = A[0][0] * ext[j] + A[0][1] * ext[3 + j] + A[0][2] * ext[6 + j];
                const double b1 = A[1][0] * ext[j] + A[1][1] * ext[3 + j] + A[1][2] * ext[6 + j];
                B[0][j] = live ? b0 : 0.0;
                B[1][j] = live ? b1 : 0.0;
                B[2][j] = 0.0;
            }
            return;
        }
    double JPs[3][6]; // (only the translation columns are used: the others are never formed)
    jac_pose(Xs, cam, stereo, JPs);
#pragma unroll
    for (int m = 0; m < 3; m++)
#pragma unroll
        for (int j = 0; j < 3; j++)
        {
            const double b = JPs[m][3] * ext[j] + JPs[m][4] * ext[3 + j] + JPs[m][5] * ext[6 + j];
            B[m][j] = live ? b : 0.0;
        }
}
__device__ __forceinline__ void jac_pose_rig(const double* Xb, const double B[3][3], double JP[3][6])
{
    const double X = Xb[0], Y = Xb[1], Z = Xb[2];
#pragma unroll
    for (int m = 0; m < 3; m++)
    {
        JP[m][0] = B[m][2] * Y - B[m][1] * Z;
        JP[m][1] = B[m][0] * Z - B[m][2] * X;
        JP[m][2] = B[m][1] * X - B[m][0] * Y;
        JP[m][3] = B[m][0];
        JP[m][4] = B[m][1];
        JP[m][5] = B[m][2];
    }
}
__device__ __forceinline__ void jac_landmark_rig(const double B[3][3], const double R[3][3], double JL[3][3])
{
#pragma unroll
    for (int m = 0; m < 3; m++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            JL[m][j] = B[m][0] * R[0][j] + B[m][1] * R[1][j] + B[m][2] * R[2][j];
}

// symmetric 3x3 inverse by adjugate, A column-major 9 with lambda added to the diagonal.
// ref: .cu:639-669 (no pivot / SPD check there either). Returns the 6 unique entries.
struct Sym3
{
    double b00, b01, b02, b11, b12, b22;
};
__device__ __forceinline__ Sym3 sym3_inv(const double* __restrict__ A, double lambda)
{
    const double A00 = A[0] + lambda, A01 = A[3], A11 = A[4] + lambda;
    const double A02 = A[2], A12 = A[7], A22 = A[8] + lambda;
    const double det = A00 * A11 * A22 + A01 * A12 * A02 + A02 * A01 * A12 - A00 * A12 * A12 -
                       A02 * A11 * A02 - A01 * A01 * A22;
    const double id = 1 / det;
    Sym3 s;
    s.b00 = id * (A11 * A22 - A12 * A12);
    s.b01 = id * (A02 * A12 - A01 * A22);
    s.b11 = id * (A00 * A22 - A02 * A02);
    s.b02 = id * (A01 * A12 - A02 * A11);
    s.b12 = id * (A02 * A01 - A00 * A12);
    s.b22 = id * (A00 * A11 - A01 * A01);
    return s;
}

// quaternion of a rotation whose trace is not positive, I the index of its largest diagonal entry (ref: .cu:721-754)
template <int I>
__device__ __forceinline__ void quat_of_rot_diag(const double R[3][3], double dq[4])
{
    constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
    double t = sqrt(R[I][I] - R[J][J] - R[K][K] + 1);
    dq[I] = 0.5 * t;
    t = 0.5 / t;
    dq[3] = (R[K][J] - R[J][K]) * t;
    dq[J] = (R[J][I] + R[I][J]) * t;
    dq[K] = (R[K][I] + R[I][K]) * t;
}

// T <- exp([w,v]) * T  (ref: updateExp .cu:781-809, updatePose .cu:811-823)
__device__ __forceinline__ void pose_exp_update(const double* __restrict__ dx,
                                                const double* __restrict__ pin,
                                                double* __restrict__ pout)
{
    const double wx = dx[0], wy = dx[1], wz = dx[2];
    const double theta = sqrt(wx * wx + wy * wy + wz * wz);
    double a1, a2, b1, b2;
    if (theta < 0.00001)
    {
        a1 = 1.0, a2 = 0.5, b1 = 0.5, b2 = 1.0 / 6;
    }
    else
    {
        a1 = sin(theta) / theta;
        a2 = (1 - cos(theta)) / (theta * theta);
        b1 = a2;
        b2 = (theta - sin(theta)) / (theta * theta * theta);
    }
    // O1 = [w]x, O2 = [w]x^2 ; R = I + a1 O1 + a2 O2 ; V = I + b1 O1 + b2 O2 (row-major here)
    const double xx = wx * wx, yy = wy * wy, zz = wz * wz;
    const double xy = wx * wy, yz = wy * wz, zx = wz * wx;
    const double O1[3][3] = {{0, -wz, wy}, {wz, 0, -wx}, {-wy, wx, 0}};
    const double O2[3][3] = {{-yy - zz, xy, zx}, {xy, -zz - xx, yz}, {zx, yz, -xx - yy}};
    double R[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
        {
            const double I = (i == j) ? 1.0 : 0.0;
            R[i][j] = I + a1 * O1[i][j] + a2 * O2[i][j];
            V[i][j] = I + b1 * O1[i][j] + b2 * O2[i][j];
        }
    // quaternion of R (ref: .cu:721-754)
    double dq[4];
    double t = R[0][0] + R[1][1] + R[2][2];
    if (t > 0)
    {
        t = sqrt(t + 1);
        dq[3] = 0.5 * t;
        t = 0.5 / t;
        dq[0] = (R[2][1] - R[1][2]) * t;
        dq[1] = (R[0][2] - R[2][0]) * t;
        dq[2] = (R[1][0] - R[0][1]) * t;
    }
    else
    {
        // the largest diagonal entry picks one of three cases, each with compile-time indices: R[i][i] and dq[i] with
        // a run-time i would put both arrays into private memory (and a private segment on every wave of the launch)
        const bool c1 = R[1][1] > R[0][0];
        const bool c2 = R[2][2] > (c1 ? R[1][1] : R[0][0]);
        if (c2)
            quat_of_rot_diag<2>(R, dq);
        else if (c1)
            quat_of_rot_diag<1>(R, dq);
        else
            quat_of_rot_diag<0>(R, dq);
    }
    const double dt0 = V[0][0] * dx[3] + V[0][1] * dx[4] + V[0][2] * dx[5];
    const double dt1 = V[1][0] * dx[3] + V[1][1] * dx[4] + V[1][2] * dx[5];
    const double dt2 = V[2][0] * dx[3] + V[2][1] * dx[4] + V[2][2] * dx[5];
    // t' = dt + R(dq) t   (rotate in cross-product form)
    const double q0 = pin[0], q1 = pin[1], q2 = pin[2], q3 = pin[3];
    const double tx = pin[4], ty = pin[5], tz = pin[6];
    double c1x = dq[1] * tz - dq[2] * ty;
    double c1y = dq[2] * tx - dq[0] * tz;
    double c1z = dq[0] * ty - dq[1] * tx;
    c1x += c1x;
    c1y += c1y;
    c1z += c1z;
    const double c2x = dq[1] * c1z - dq[2] * c1y;
    const double c2y = dq[2] * c1x - dq[0] * c1z;
    const double c2z = dq[0] * c1y - dq[1] * c1x;
    pout[4] = dt0 + (tx + dq[3] * c1x + c2x);
    pout[5] = dt1 + (ty + dq[3] * c1y + c2y);
    pout[6] = dt2 + (tz + dq[3] * c1z + c2z);
    // q' = normalise(dq * q), w >= 0  (ref: .cu:756-775)
    double r3 = dq[3] * q3 - dq[0] * q0 - dq[1] * q1 - dq[2] * q2;
    double r0 = dq[3] * q0 + dq[0] * q3 + dq[1] * q2 - dq[2] * q1;
    double r1 = dq[3] * q1 + dq[1] * q3 + dq[2] * q0 - dq[0] * q2;
    double r2 = dq[3] * q2 + dq[2] * q3 + dq[0] * q1 - dq[1] * q0;
    double invn = 1 / sqrt(r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3);
    if (r3 < 0)
        invn = -invn;
    pout[0] = invn * r0;
    pout[1] = invn * r1;
    pout[2] = invn * r2;
    pout[3] = invn * r3;
}

// ---- shared by the unary pose edge kinds (icp_kernels.hip, prior_kernels.hip): the 27 terms of a pose are the upper
// triangle of its 6 x 6 block of H, row-major packed (t < 21), then b (t = 21..26)
// entry t < 21 of the packed upper triangle -> (r, c), r <= c
__device__ __forceinline__ void tri6_unpack(int t, int& r, int& c)
{
    r = 0;
    int k = t;
    while (k >= 6 - r)
        k -= 6 - r, r++;
    c = r + k;
}
// term t < 27 of pose p, value s, ADDED to its destination; (r, c) = tri6_unpack(t) where t < 21.  SCHUR = false: the
// block of Hpp (mirrored off the diagonal) / bp.  SCHUR = true: the diagonal block of Hsc (the first block of the pose's
// row, through rowptr), bp and bsc
template <bool SCHUR>
__device__ __forceinline__ void pose_term_add(int p, int t, int r, int c, double s, double* __restrict__ H,
                                              const int32_t* __restrict__ rowptr, double* __restrict__ bp,
                                              double* __restrict__ bsc)
{
    if (t < 21)
    {
        double* blk = H + 36 * (size_t)(SCHUR ? rowptr[p] : p);
        blk[r + 6 * c] += s;
        if (r != c)
            blk[c + 6 * r] += s;
    }
    else if (t < 27)
    {
        bp[6 * (size_t)p + (t - 21)] += s;
        if (SCHUR)
            bsc[6 * (size_t)p + (t - 21)] += s;
    }
}

// the chi2 total of a workgroup of N pose groups: lane 0 of group g has stored the group's chi2 to s_chi[g] (shared
// memory; the store stays in the kernel, in front of the group's term adds); thread 0 sums them in group order
template <int N>
__device__ __forceinline__ void pose_groups_chi_total(const double* s_chi, double* wg_chi)
{
    __syncthreads();
    if (threadIdx.x == 0)
    {
        double tot = 0.0;
#pragma unroll
        for (int i = 0; i < N; i++)
            tot += s_chi[i];
        wg_chi[blockIdx.x] = tot;
    }
}

// ---- shared by the SE(3) edge kinds (prior_kernels.hip, relpose_kernels.hip): the residual of D = T Z^-1 (the prior) or
// D = T_a T_b^-1 Z^-1 (a relative-pose edge) under a full 6 x 6 information matrix, every lane in registers.
// Z = (q_z, t_z) of edge e from the planar meas [7][n].  Returns the stride n as an opaque per-lane value: the 28
// multiples of n the planar arrays are read at would otherwise each take a pair of scalar registers across the edge
// loop (32-bit indices: 21 n stays far below 2^31)
__device__ __forceinline__ int se3_load_meas(const double* meas, int n, int e, double qz[4], double tz[3])
{
    int stride = n;
    asm volatile("" : "+v"(stride));
    int i = e;
#pragma unroll
    for (int c = 0; c < 4; c++, i += stride)
        qz[c] = meas[i];
#pragma unroll
    for (int c = 0; c < 3; c++, i += stride)
        tz[c] = meas[i];
    return stride;
}
// r = [ phi ; t - R_D t_z ], phi = Log_SO3(R_D) = theta / sin(theta) * vee(D - D^T) / 2 with
// theta = atan2(|vee| / 2, (tr D - 1) / 2) in [0, pi]; sn and cs ARE sin theta and cos theta
__device__ __forceinline__ void se3_residual(const double D[3][3], const double* t, const double tz[3], double r[6],
                                             double& sn, double& cs, double& theta)
{
    const double s0 = 0.5 * (D[2][1] - D[1][2]), s1 = 0.5 * (D[0][2] - D[2][0]), s2 = 0.5 * (D[1][0] - D[0][1]);
    sn = sqrt(s0 * s0 + s1 * s1 + s2 * s2);
    cs = 0.5 * (D[0][0] + D[1][1] + D[2][2] - 1.0);
    theta = atan2(sn, cs);
    const double f = sn > 1e-12 ? theta / sn : 1.0;
    r[0] = f * s0, r[1] = f * s1, r[2] = f * s2;
#pragma unroll
    for (int i = 0; i < 3; i++)
        r[3 + i] = t[i] - (D[i][0] * tz[0] + D[i][1] * tz[1] + D[i][2] * tz[2]);
}
// Omega of edge e, full symmetric, from its packed upper triangle info [21][n_info] (n_info == 1: one for all);
// stride: what se3_load_meas returned
__device__ __forceinline__ void se3_load_info(const double* info, int n_info, int e, int stride, double Om[6][6])
{
    int at = n_info == 1 ? 0 : e;
    const int step = n_info == 1 ? 1 : stride;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++)
        {
            const double w = info[at];
            Om[i][j] = w, Om[j][i] = w;
            at += step;
        }
}
// Or = Omega r; returns x = max(0, r^T Omega r)
__device__ __forceinline__ double se3_quadratic(const double Om[6][6], const double r[6], double Or[6])
{
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
    return fmax(0.0, x);
}
// J_l^-1(phi) = I - 1/2 [phi]x + c(theta) [phi]x^2, phi = r[0..2]; no call of sin / cos (sn, cs of se3_residual)
__device__ __forceinline__ void se3_jl_inv(const double r[6], double theta, double sn, double cs, double Jl[3][3])
{
    const double th2 = theta * theta;
    const double c = theta < 1e-3 ? 1.0 / 12 + th2 * (1.0 / 720) : 1.0 / th2 - (1.0 + cs) / (2.0 * theta * sn);
    const double p0 = r[0], p1 = r[1], p2 = r[2];
    // [phi]x and its square
    const double K[3][3] = {{0.0, -p2, p1}, {p2, 0.0, -p0}, {-p1, p0, 0.0}};
    const double K2[3][3] = {{-(p1 * p1 + p2 * p2), p0 * p1, p0 * p2},
                             {p0 * p1, -(p0 * p0 + p2 * p2), p1 * p2},
                             {p0 * p2, p1 * p2, -(p0 * p0 + p1 * p1)}};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            Jl[i][j] = (i == j ? 1.0 : 0.0) - 0.5 * K[i][j] + c * K2[i][j];
}

} // namespace cugo_dev
