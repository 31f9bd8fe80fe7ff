// Landmark position priors (include/landmark_prior_types.h; the term: lm_prior_term.h), the passes of their own.
//
// Layout: priors sorted by landmark index (stable: container order inside a landmark) with a CSR lm_ptr over ALL
// landmarks, structure of arrays; Omega as its upper triangle, row-major packed 00 01 02 11 12 22, per prior or one for
// all.
//
// In the LM loop the terms themselves ride in the BA build pass: the owner lane of k_build_edges (ba_kernels.hip) adds a
// landmark's priors behind its edges, before Hll / bl are stored, factored or inverted.  What is left for this file is
// the chi2 (k_lm_prior<0>: one launch per error pass) and the stand-alone add of the kernel-level C ABI
// (k_lm_prior<1>).  One lane per free landmark walks its priors in sorted order; the sums are ADDED straight to Hll / bl
// with no partials, no atomics and one fixed order.  Every workgroup leaves ONE chi2 total, its lanes in order; both
// modes compute exactly these totals, so their chi2 agree bit for bit.  A landmark none of whose priors counts keeps
// the bits of its blocks; fixed landmarks (index >= n_landmarks_free) are never visited.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "lm_prior_term.h"

namespace
{

using namespace cugo_dev;

constexpr int LMP_WG = 256;

enum LmPriorMode
{
    LMP_ERRORS = 0, // chi2 only (and, optionally, the chi2 term of every prior)
    LMP_ADD = 1     // + the terms into Hll [L][9] and bl [L][3]
};

template <int MODE>
__global__ __launch_bounds__(LMP_WG) void k_lm_prior(LmPriorView v, int n_landmarks_free, const double* __restrict__ lms,
                                                      double* __restrict__ wg_chi, double* __restrict__ edge_chi,
                                                      double* __restrict__ Hll, double* __restrict__ bl)
{
    __shared__ double s_chi[LMP_WG];
    const int l = blockIdx.x * LMP_WG + threadIdx.x;
    double chi = 0.0;
    if (l < n_landmarks_free)
    {
        const double X[3] = {lms[3 * (size_t)l], lms[3 * (size_t)l + 1], lms[3 * (size_t)l + 2]};
        // the block as stored, column-major: the upper triangle in the order of the term, then the lower one
        double a[9], lo[3];
        bool any = false, loaded = false;
        for (int e = v.lm_ptr[l], e1 = v.lm_ptr[l + 1]; e < e1; e++)
        {
            const bool active = !(v.flags && (v.flags[e] & CUGO_EDGE_INACTIVE));
            double c = 0.0;
            if (active)
            {
                double t[9];
                c = lm_prior_term<MODE == LMP_ADD>(v, e, X, t);
                chi = __dadd_rn(chi, c);
                if (MODE == LMP_ADD)
                {
                    if (!loaded)
                    {
                        const double* H = Hll + 9 * (size_t)l;
                        a[0] = H[0], a[1] = H[3], a[2] = H[6], a[3] = H[4], a[4] = H[7], a[5] = H[8];
                        lo[0] = H[1], lo[1] = H[2], lo[2] = H[5];
                        a[6] = bl[3 * (size_t)l], a[7] = bl[3 * (size_t)l + 1], a[8] = bl[3 * (size_t)l + 2];
                        loaded = true;
                    }
#pragma unroll
                    for (int k = 0; k < 9; k++)
                        a[k] = __dadd_rn(a[k], t[k]);
                    lo[0] = __dadd_rn(lo[0], t[1]), lo[1] = __dadd_rn(lo[1], t[2]), lo[2] = __dadd_rn(lo[2], t[4]);
                    any = true;
                }
            }
            if (MODE == LMP_ERRORS && edge_chi)
                edge_chi[e] = c;
        }
        if (MODE == LMP_ADD && any)
        {
            double* H = Hll + 9 * (size_t)l;
            H[0] = a[0], H[3] = a[1], H[6] = a[2], H[4] = a[3], H[7] = a[4], H[8] = a[5];
            H[1] = lo[0], H[2] = lo[1], H[5] = lo[2];
            bl[3 * (size_t)l] = a[6], bl[3 * (size_t)l + 1] = a[7], bl[3 * (size_t)l + 2] = a[8];
        }
    }
    s_chi[threadIdx.x] = chi;
    __syncthreads();
    if (threadIdx.x == 0)
    { // one total per workgroup, its lanes in order
        double tot = 0.0;
        for (int i = 0; i < LMP_WG; i++)
            tot += s_chi[i];
        wg_chi[blockIdx.x] = tot;
    }
}

template <int MODE>
void launch(hipStream_t s, const char* label, const cugo_lm_prior_edges& ev, const double* d_lms, double* d_wg_chi,
            double* d_edge_chi, double* d_Hll, double* d_bl)
{
    const int wgs = cugo_k::lm_prior_workgroups(ev);
    if (!wgs)
        return;
    cugo_k::LaunchScope scope(label, s);
    hipLaunchKernelGGL(k_lm_prior<MODE>, dim3(wgs), dim3(LMP_WG), 0, s, lm_prior_view(ev), ev.n_landmarks_free, d_lms, d_wg_chi,
                       d_edge_chi, d_Hll, d_bl);
}

} // namespace

namespace cugo_k
{

int lm_prior_workgroups(const cugo_lm_prior_edges& ev)
{
    return ev.n > 0 && ev.n_landmarks_free > 0 ? (ev.n_landmarks_free + LMP_WG - 1) / LMP_WG : 0;
}

void launch_lm_prior_errors(hipStream_t s, const cugo_lm_prior_edges& ev, const double* d_lms, double* d_wg_chi,
                            double* d_edge_chi)
{
    launch<LMP_ERRORS>(s, "k_lm_prior_errors", ev, d_lms, d_wg_chi, d_edge_chi, nullptr, nullptr);
}

void launch_lm_prior_add(hipStream_t s, const cugo_lm_prior_edges& ev, const double* d_lms, double* d_Hll, double* d_bl,
                         double* d_wg_chi)
{
    launch<LMP_ADD>(s, "k_lm_prior_add", ev, d_lms, d_wg_chi, nullptr, d_Hll, d_bl);
}

} // namespace cugo_k
