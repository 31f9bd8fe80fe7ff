// Landmark position priors (include/landmark_prior_types.h; g2o calls the edge EdgeXYZPrior): unary edges on a landmark
// with a measured position Z and a 3 x 3 information matrix Omega (symmetric, positive semi-definite).
//   r = X - Z,  J = I,  x = max(0, r^T Omega r),  chi2 term rho(x),  w = rho'(x),  Hll += w Omega,  bl -= w Omega r
// Sign and blocks are those of the BA build pass.  The term lives here once, for the kernel of its own
// (lm_prior_kernels.hip) and for the owner lane of k_build_edges (ba_kernels.hip): every product and every sum inside
// it is an explicitly rounded operation (__dmul_rn / __dadd_rn), so that no compiler setting can contract them into a
// caller's additions in one kernel and not in the other — both add the same nine doubles per prior, in sorted order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/cugo_hip.h"
#include "ba_math.h"

namespace cugo_dev
{

// the priors as the kernels see them: sorted by landmark, planar; lm_ptr is the CSR over ALL landmarks
struct LmPriorView
{
    int n, n_info;
    const int32_t* lm_ptr; // [n_landmarks_total + 1]
    const double* meas;    // [3][n]
    const double* info;    // [6][n] or [6][1]: 00 01 02 11 12 22
    const uint8_t* flags;  // [n] or nullptr
    Robust rk;
};

// the view of a cugo_lm_prior_edges (host side of a launch)
inline LmPriorView lm_prior_view(const cugo_lm_prior_edges& ev)
{
    LmPriorView v;
    v.n = ev.n, v.n_info = ev.n_info;
    v.lm_ptr = ev.d_lm_ptr, v.meas = ev.d_meas, v.info = ev.d_info, v.flags = ev.d_flags;
    v.rk = Robust{ev.rk, ev.delta};
    return v;
}

// prior e at the landmark estimate X: returns its chi2 term; with FULL, t = {w Omega (00 01 02 11 12 22), -w Omega r}
template <bool FULL>
__device__ __forceinline__ double lm_prior_term(const LmPriorView& v, int e, const double* __restrict__ X, double t[9])
{
    const size_t n = (size_t)v.n;
    const double r0 = __dadd_rn(X[0], -v.meas[e]);
    const double r1 = __dadd_rn(X[1], -v.meas[n + e]);
    const double r2 = __dadd_rn(X[2], -v.meas[2 * n + e]);
    const size_t s = v.n_info > 1 ? n : 1; // [6][n], or [6][1]: one matrix for all
    const int i = v.n_info > 1 ? e : 0;
    const double o00 = v.info[i], o01 = v.info[s + i], o02 = v.info[2 * s + i];
    const double o11 = v.info[3 * s + i], o12 = v.info[4 * s + i], o22 = v.info[5 * s + i];
    const double q0 = __dadd_rn(__dadd_rn(__dmul_rn(o00, r0), __dmul_rn(o01, r1)), __dmul_rn(o02, r2));
    const double q1 = __dadd_rn(__dadd_rn(__dmul_rn(o01, r0), __dmul_rn(o11, r1)), __dmul_rn(o12, r2));
    const double q2 = __dadd_rn(__dadd_rn(__dmul_rn(o02, r0), __dmul_rn(o12, r1)), __dmul_rn(o22, r2));
    const double x = fmax(0.0, __dadd_rn(__dadd_rn(__dmul_rn(r0, q0), __dmul_rn(r1, q1)), __dmul_rn(r2, q2)));
    if (FULL)
    {
        const double w = rk_drho(v.rk, x);
        t[0] = __dmul_rn(w, o00), t[1] = __dmul_rn(w, o01), t[2] = __dmul_rn(w, o02);
        t[3] = __dmul_rn(w, o11), t[4] = __dmul_rn(w, o12), t[5] = __dmul_rn(w, o22);
        t[6] = -__dmul_rn(w, q0), t[7] = -__dmul_rn(w, q1), t[8] = -__dmul_rn(w, q2);
    }
    return rk_rho(v.rk, x);
}

// The priors of landmark l, in sorted order, ADDED to a = {Hll 00 01 02 11 12 22, bl 0 1 2}: what the owner lane of
// k_build_edges does behind the landmark's edges.  Returns whether a prior counted.
__device__ __forceinline__ bool lm_prior_accumulate(const LmPriorView& v, int l, const double* __restrict__ X, double a[9])
{
    bool any = false;
    for (int e = v.lm_ptr[l], e1 = v.lm_ptr[l + 1]; e < e1; e++)
    {
        if (v.flags && (v.flags[e] & CUGO_EDGE_INACTIVE))
            continue;
        double t[9];
        lm_prior_term<true>(v, e, X, t);
#pragma unroll
        for (int k = 0; k < 9; k++)
            a[k] = __dadd_rn(a[k], t[k]);
        any = true;
    }
    return any;
}

} // namespace cugo_dev
