// Marginal covariances on gfx950 (fp64): the selected inverse of the multifrontal block LL^T of Hsc
// (chol_kernels.hip) and the landmark blocks built from it.
//
// Selected inverse (supernodal Takahashi recurrences), top-down over the stages of the factorisation.
// For a front with pivot columns J and boundary rows R (W = L11^-1 and L21 as dev_backward reads them):
//
//   S_RR  = Sigma on R x R, read from the parent's Sigma-front through the extend-add map `rel`
//   S_RJ  = -S_RR L21 W
//   S_JJ  = W^T (W - L21^T S_RJ)
//
// Every front owns a Sigma-front with the offset and leading dimension of its front (CholPlan::off / ldf): the
// Sigma-front of a front stored in its only child's update block (alias chains) then already sits in that
// child's R x R region, and the child reads it in place.  Other fronts copy the lower triangle of S_RR into
// their own R x R region while they read it, so their children find it there.
//
//   k_selinv_rows    one workgroup per 64-row tile of R: S_RJ of those rows (and the copy of their S_RR rows)
//   k_selinv_jj      one workgroup per front: S_JJ
//   k_selinv_subtree one workgroup per subtree task of stage 0: both, front by front, top-down
//   k_selinv_gather  the blocks of the Hsc pattern out of the Sigma-fronts (permutation and blk_trans undone)
//
// Every entry is one thread's sum in a fixed order: no atomics, the same bits on every call.
//
// Blocks off the pattern (any pair a, b) come from forward solves on the same W and L21 instead:
//   k_inv_path_walk   one workgroup per distinct query row: Y_v = L^-1 E_v along the path from v's front to the root
//   k_inv_pair_blocks one workgroup per pair: Y_a^T Y_b
//
// Landmarks (k_lm_covariance): with Hll = L L^T and G_e = Hpl_e L^-T of the landmark's free-pose edges,
//   Sigma_l = L^-T (I + sum_{e,f} G_e^T Sigma_{p(e) p(f)} G_f) L^-1,
// one thread per landmark, the pose blocks looked up in the upper block CSR of Hsc.
//
// Pose-landmark blocks (k_pose_lm_cross), with the same L and G_e: Sigma_al = -(sum_e Sigma_{a p(e)} G_e) L^-1, and the
// covariance of a reprojection from them (k_reprojection_cov): J Sigma J^T over the joint [a; l] block.  One thread per
// query, the pose blocks handed in by index (csrc/host/plcov_plan.h).  k_predict_obs: the same for a camera behind a
// sensor pose, a Kannala-Brandt camera and the depth kind, with the predicted observation itself.
#include <algorithm>

#include "ba_math.h"
#include "kernels.h"

namespace
{

using cugo_k::CholPlanDev;

constexpr int SI_T = 256;        // workgroup size (16 x 16 threads)
constexpr int SI_R = 64;         // rows of R per tile workgroup
constexpr int SI_K = 32;         // depth of one LDS chunk
constexpr int SI_N = 96;         // widest pivot block (scalars, NC_MAX of chol_kernels.hip)
constexpr int SI_LD = SI_N + 1;  // LDS leading dimension
constexpr size_t SI_LDS_ROWS = (size_t)SI_R * SI_LD;          // max(S chunk + L21 chunk + maps, Z tile)
constexpr size_t SI_LDS_JJ = (size_t)SI_N * SI_LD;            // max(two chunks, W - T)
static_assert((size_t)SI_R * (SI_K + 1) + (size_t)SI_K * SI_LD + (SI_R + SI_K) / 2 + 1 <= SI_LDS_ROWS, "LDS");
static_assert((size_t)2 * SI_K * SI_LD <= SI_LDS_JJ, "LDS");

__device__ __forceinline__ int pad16(int nc) { return (nc + 15) & ~15; }

// where a front's W and L21 are: the places dev_backward (chol_kernels.hip) reads them from
struct SelFront
{
    int ncs, nrs, ncp;
    long off, ld, ldl;
    const double* L; // L21[i][m] = L[m * ldl + i]
    const double* W; // W[k][j] = W[j * ncp + k], j <= k < ncs (the rest is not defined)
};
__device__ __forceinline__ SelFront sel_front(const CholPlanDev& p, const double* __restrict__ fronts, int f)
{
    SelFront F;
    F.ncs = 6 * p.ncb[f];
    F.nrs = 6 * (p.nb[f] - p.ncb[f]);
    F.ncp = pad16(F.ncs);
    F.off = p.off[f];
    F.ld = p.ldf[f];
    const long l21o = p.l21off[f];
    F.L = l21o >= 0 ? p.l21 + l21o : fronts + F.off + F.ncs;
    F.ldl = l21o >= 0 ? F.nrs + 1 : F.ld;
    F.W = p.winv + p.woff[f];
    return F;
}

// S_RJ of the rows [r0, r0 + 64) of R.  sinfo[4 f ..]: offset and leading dimension of the parent's Sigma-front,
// offset of the front's rel list, and whether S_RR must be copied into the front's own Sigma-front (0 when the
// parent is stored in this front's update block: the copy would be the parent itself)
__device__ void selinv_rows(const CholPlanDev& p, const double* __restrict__ fronts, double* sig,
                            const int64_t* __restrict__ sinfo, int f, int r0, double* __restrict__ lds)
{
    const SelFront F = sel_front(p, fronts, f);
    const long offp = sinfo[4 * f], ldp = sinfo[4 * f + 1];
    const int32_t* __restrict__ rel = p.rel + sinfo[4 * f + 2];
    const bool copy_s = sinfo[4 * f + 3] != 0;
    const int nt = min(SI_R, F.nrs - r0);
    double* Ss = lds;                        // [SI_R][SI_K + 1]
    double* Ls = lds + SI_R * (SI_K + 1);    // [SI_K][SI_LD]
    int* rmap = reinterpret_cast<int*>(Ls + SI_K * SI_LD); // row of the parent front of each tile row ...
    int* kmap = rmap + SI_R;                               // ... and of each row of the chunk
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    __syncthreads(); // (the LDS may still be read by the previous front of a subtree task)
    if (t < nt)
    {
        const int i = r0 + t;
        rmap[t] = 6 * rel[i / 6] + i % 6;
    }
    double acc[4][6];
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int r = 0; r < 6; r++)
            acc[q][r] = 0.0;
    // Z = S_RR[tile, :] L21
    for (int k0 = 0; k0 < F.nrs; k0 += SI_K)
    {
        const int nk = min(SI_K, F.nrs - k0);
        __syncthreads();
        if (t < nk)
        {
            const int k = k0 + t;
            kmap[t] = 6 * rel[k / 6] + k % 6;
        }
        __syncthreads();
        for (int e = t; e < SI_R * SI_K; e += SI_T)
        {
            const int i = e / SI_K, k = e % SI_K;
            double v = 0.0;
            if (i < nt && k < nk)
            {
                const int a = rmap[i], b = kmap[k];
                v = sig[offp + (long)min(a, b) * ldp + max(a, b)];
                if (copy_s && k0 + k <= r0 + i)
                    sig[F.off + (long)(F.ncs + k0 + k) * F.ld + F.ncs + r0 + i] = v;
            }
            Ss[i * (SI_K + 1) + k] = v;
        }
        for (int e = t; e < SI_K * SI_N; e += SI_T)
        {
            const int k = e % SI_K, m = e / SI_K;
            Ls[k * SI_LD + m] = (k < nk && m < F.ncs) ? F.L[(long)m * F.ldl + k0 + k] : 0.0;
        }
        __syncthreads();
        for (int k = 0; k < nk; k++)
        {
            double s[4], l[6];
#pragma unroll
            for (int q = 0; q < 4; q++)
                s[q] = Ss[(ty + 16 * q) * (SI_K + 1) + k];
#pragma unroll
            for (int r = 0; r < 6; r++)
                l[r] = Ls[k * SI_LD + tx + 16 * r];
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int r = 0; r < 6; r++)
                    acc[q][r] += s[q] * l[r];
        }
    }
    __syncthreads();
    double* Zs = lds; // [SI_R][SI_LD]
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int r = 0; r < 6; r++)
            Zs[(ty + 16 * q) * SI_LD + tx + 16 * r] = acc[q][r];
    __syncthreads();
    // S_RJ[tile, j] = -sum_{m >= j} Z[tile, m] W[m, j]
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int r = 0; r < 6; r++)
            acc[q][r] = 0.0;
    for (int m = 0; m < F.ncs; m++)
    {
        double w[6], z[4];
#pragma unroll
        for (int r = 0; r < 6; r++)
        {
            const int j = tx + 16 * r;
            w[r] = (j <= m) ? F.W[(long)j * F.ncp + m] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 4; q++)
            z[q] = Zs[(ty + 16 * q) * SI_LD + m];
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int r = 0; r < 6; r++)
                acc[q][r] += z[q] * w[r];
    }
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int r = 0; r < 6; r++)
        {
            const int i = ty + 16 * q, j = tx + 16 * r;
            if (i < nt && j < F.ncs)
                sig[F.off + (long)j * F.ld + F.ncs + r0 + i] = -acc[q][r];
        }
}

// S_JJ = W^T (W - L21^T S_RJ) of front f (S_RJ written before)
__device__ void selinv_jj(const CholPlanDev& p, const double* __restrict__ fronts, double* sig, int f,
                          double* __restrict__ lds)
{
    const SelFront F = sel_front(p, fronts, f);
    double* La = lds;               // [SI_K][SI_LD]  L21 rows
    double* Sa = lds + SI_K * SI_LD; // [SI_K][SI_LD]  S_RJ rows
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    double acc[6][6];
#pragma unroll
    for (int q = 0; q < 6; q++)
#pragma unroll
        for (int r = 0; r < 6; r++)
            acc[q][r] = 0.0;
    // T = L21^T S_RJ (J x J), summed over R in row order
    for (int i0 = 0; i0 < F.nrs; i0 += SI_K)
    {
        const int ni = min(SI_K, F.nrs - i0);
        __syncthreads();
        for (int e = t; e < SI_K * SI_N; e += SI_T)
        {
            const int i = e % SI_K, m = e / SI_K;
            const bool ok = i < ni && m < F.ncs;
            La[i * SI_LD + m] = ok ? F.L[(long)m * F.ldl + i0 + i] : 0.0;
            Sa[i * SI_LD + m] = ok ? sig[F.off + (long)m * F.ld + F.ncs + i0 + i] : 0.0;
        }
        __syncthreads();
        for (int i = 0; i < ni; i++)
        {
            double a[6], b[6];
#pragma unroll
            for (int q = 0; q < 6; q++)
                a[q] = La[i * SI_LD + ty + 16 * q];
#pragma unroll
            for (int r = 0; r < 6; r++)
                b[r] = Sa[i * SI_LD + tx + 16 * r];
#pragma unroll
            for (int q = 0; q < 6; q++)
#pragma unroll
                for (int r = 0; r < 6; r++)
                    acc[q][r] += a[q] * b[r];
        }
    }
    __syncthreads();
    double* Ms = lds; // [SI_N][SI_LD]: W - T
#pragma unroll
    for (int q = 0; q < 6; q++)
#pragma unroll
        for (int r = 0; r < 6; r++)
        {
            const int m = ty + 16 * q, j = tx + 16 * r;
            const double w = (j <= m && m < F.ncs) ? F.W[(long)j * F.ncp + m] : 0.0;
            Ms[m * SI_LD + j] = w - acc[q][r];
        }
    __syncthreads();
    // S_JJ[a][b] = sum_{m >= a} W[m][a] M[m][b]
#pragma unroll
    for (int q = 0; q < 6; q++)
#pragma unroll
        for (int r = 0; r < 6; r++)
            acc[q][r] = 0.0;
    for (int m = 0; m < F.ncs; m++)
    {
        double w[6], b[6];
#pragma unroll
        for (int q = 0; q < 6; q++)
        {
            const int a = ty + 16 * q;
            w[q] = (a <= m) ? F.W[(long)a * F.ncp + m] : 0.0;
        }
#pragma unroll
        for (int r = 0; r < 6; r++)
            b[r] = Ms[m * SI_LD + tx + 16 * r];
#pragma unroll
        for (int q = 0; q < 6; q++)
#pragma unroll
            for (int r = 0; r < 6; r++)
                acc[q][r] += w[q] * b[r];
    }
#pragma unroll
    for (int q = 0; q < 6; q++)
#pragma unroll
        for (int r = 0; r < 6; r++)
        {
            const int a = ty + 16 * q, b = tx + 16 * r;
            if (a < F.ncs && b < F.ncs)
                sig[F.off + (long)b * F.ld + a] = acc[q][r];
        }
}

// items: (front, first row of the tile) pairs of one stage
__global__ __launch_bounds__(SI_T) void k_selinv_rows(CholPlanDev p, const double* __restrict__ fronts, double* sig,
                                                      const int64_t* __restrict__ sinfo, const int32_t* __restrict__ items)
{
    extern __shared__ double lds[];
    const int32_t* it = items + 2 * blockIdx.x;
    selinv_rows(p, fronts, sig, sinfo, it[0], it[1], lds);
}

__global__ __launch_bounds__(SI_T) void k_selinv_jj(CholPlanDev p, const double* __restrict__ fronts, double* sig,
                                                    int task0)
{
    extern __shared__ double lds[];
    const int t = task0 + blockIdx.x;
    selinv_jj(p, fronts, sig, p.task_fronts[p.task_ptr[t]], lds);
}

// a subtree task of stage 0: its fronts are listed children first, so walked backwards every parent is done
// before its children
__global__ __launch_bounds__(SI_T) void k_selinv_subtree(CholPlanDev p, const double* __restrict__ fronts, double* sig,
                                                         const int64_t* __restrict__ sinfo, int task0)
{
    extern __shared__ double lds[];
    const int t = task0 + blockIdx.x;
    for (int fi = p.task_ptr[t + 1] - 1; fi >= p.task_ptr[t]; fi--)
    {
        const int f = p.task_fronts[fi];
        const int nrs = 6 * (p.nb[f] - p.ncb[f]);
        for (int r0 = 0; r0 < nrs; r0 += SI_R)
            selinv_rows(p, fronts, sig, sinfo, f, r0, lds);
        __threadfence_block();
        __syncthreads();
        selinv_jj(p, fronts, sig, f, lds);
        __threadfence_block();
        __syncthreads();
    }
}

// out[k] (column-major 6 x 6) = the block of Sigma at the position of Hsc block k
__global__ __launch_bounds__(SI_T) void k_selinv_gather(CholPlanDev p, const double* __restrict__ sig,
                                                        double* __restrict__ out)
{
    const long i = (long)blockIdx.x * SI_T + threadIdx.x;
    if (i >= 36L * p.n_hsc_blocks)
        return;
    const int k = (int)(i / 36), e = (int)(i % 36), r = e % 6, c = e / 6;
    const int f = p.blk_front[k];
    const bool tr = p.blk_trans[k] != 0;
    const int ra = 6 * p.blk_row[k] + (tr ? c : r), ca = 6 * p.blk_col[k] + (tr ? r : c);
    out[i] = sig[p.off[f] + (long)min(ra, ca) * p.ldf[f] + max(ra, ca)];
}

// ---------------------------------------------------------------- landmarks --------------
// lower Cholesky factor of a 3x3 SPD block (column-major in), its inverse (lower, row-major li[r][c]); false on a
// pivot <= 0 or NaN
__device__ __forceinline__ bool chol3_inv(const double* __restrict__ H, double (&li)[3][3])
{
    const double l00 = H[0] > 0.0 ? sqrt(H[0]) : 0.0;
    const double l10 = H[1] / l00, l20 = H[2] / l00;
    const double d1 = H[4] - l10 * l10;
    const double l11 = d1 > 0.0 ? sqrt(d1) : 0.0;
    const double l21 = (H[5] - l20 * l10) / l11;
    const double d2 = H[8] - l20 * l20 - l21 * l21;
    const double l22 = d2 > 0.0 ? sqrt(d2) : 0.0;
    if (!(l00 > 0.0 && l11 > 0.0 && l22 > 0.0))
        return false;
    li[0][0] = 1.0 / l00, li[1][1] = 1.0 / l11, li[2][2] = 1.0 / l22;
    li[1][0] = -l10 * li[0][0] / l11;
    li[2][1] = -l21 * li[1][1] / l22;
    li[2][0] = -(l20 * li[0][0] + l21 * li[1][0]) / l22;
    li[0][1] = li[0][2] = li[1][2] = 0.0;
    return true;
}

// G = Hpl_e L^-T (6 x 3): G[r][c] = sum_k Hpl[r][k] Linv[c][k]
__device__ __forceinline__ void lm_g(const double* __restrict__ hpl, const double (&li)[3][3], double (&g)[6][3])
{
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
        for (int c = 0; c < 3; c++)
        {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++)
                s += hpl[r + 6 * k] * li[c][k];
            g[r][c] = s;
        }
}

__global__ __launch_bounds__(256) void k_lm_covariance(int L, const int32_t* __restrict__ lm_ptr,
                                                       const int32_t* __restrict__ e_pose, const uint8_t* __restrict__ flags,
                                                       const double* __restrict__ Hll, const double* __restrict__ Hpl,
                                                       const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                       const double* __restrict__ sigma, double* __restrict__ out,
                                                       int32_t* __restrict__ fail)
{
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= L)
        return;
    double li[3][3];
    if (!chol3_inv(Hll + 9L * l, li))
    {
        *fail = 1; // (every writer stores the same value)
        for (int k = 0; k < 9; k++)
            out[9L * l + k] = 0.0;
        return;
    }
    double M[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    const int e0 = lm_ptr[l], e1 = lm_ptr[l + 1];
    for (int e = e0; e < e1; e++)
    {
        if (flags[e] & (CUGO_EDGE_FIXED_L | CUGO_EDGE_FIXED_P | CUGO_EDGE_INACTIVE))
            continue;
        double ge[6][3];
        lm_g(Hpl + 18L * e, li, ge);
        const int pe = e_pose[e];
        for (int f = e0; f < e1; f++)
        {
            if (flags[f] & (CUGO_EDGE_FIXED_L | CUGO_EDGE_FIXED_P | CUGO_EDGE_INACTIVE))
                continue;
            const int pf = e_pose[f];
            // the Hsc block (min, max) of the pair: row min(pe, pf) of the upper block CSR
            const int a = min(pe, pf), b = max(pe, pf);
            int lo = rowptr[a], hi = rowptr[a + 1] - 1;
            while (lo < hi)
            {
                const int mid = (lo + hi) >> 1;
                if (colind[mid] < b)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            const double* S = sigma + 36L * lo; // Sigma_{a b}, column-major; Sigma_{pe pf} is it or its transpose
            const bool tr = pe > pf;
            double gf[6][3];
            lm_g(Hpl + 18L * f, li, gf);
            // X = Sigma_{pe pf} G_f (6 x 3), then M += G_e^T X
            double X[6][3];
#pragma unroll
            for (int r = 0; r < 6; r++)
#pragma unroll
                for (int c = 0; c < 3; c++)
                {
                    double s = 0.0;
#pragma unroll
                    for (int k = 0; k < 6; k++)
                        s += (tr ? S[k + 6 * r] : S[r + 6 * k]) * gf[k][c];
                    X[r][c] = s;
                }
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++)
                {
                    double s = 0.0;
#pragma unroll
                    for (int k = 0; k < 6; k++)
                        s += ge[k][r] * X[k][c];
                    M[r][c] += s;
                }
        }
    }
    // Sigma_l = L^-T M L^-1: [r][c] = sum_{a, b} Linv[a][r] M[a][b] Linv[b][c]
    double Y[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int c = 0; c < 3; c++)
            Y[a][c] = M[a][0] * li[0][c] + M[a][1] * li[1][c] + M[a][2] * li[2][c];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++)
        {
            const int rr = max(r, c), cc = min(r, c); // (the lower triangle, mirrored: exactly symmetric)
            out[9L * l + r + 3 * c] = li[0][rr] * Y[0][cc] + li[1][rr] * Y[1][cc] + li[2][rr] * Y[2][cc];
        }
}

// Pose-landmark blocks: Sigma_al = -(sum_e Sigma_{a p(e)} G_e) L^-1 over the counted slots e of landmark l in slot
// order, one thread per query.  Query q: q_pose[q] / q_lm[q] are the free indices of a and l, -1 for a fixed vertex
// (18 zeros; of a free landmark under a fixed pose Hll alone is read, for the flag); its slot k reads the block
// blocks[q_slot[q_ptr[q] + k]] (6 x 6 column-major, rows a).
// Every index into acc, g and li is a compile-time constant (the loops are unrolled), so all of it lives in registers.
__global__ __launch_bounds__(256) void k_pose_lm_cross(int n, const int32_t* __restrict__ q_pose,
                                                       const int32_t* __restrict__ q_lm, const int32_t* __restrict__ q_ptr,
                                                       const int32_t* __restrict__ q_slot, const int32_t* __restrict__ lm_ptr,
                                                       const uint8_t* __restrict__ flags, const double* __restrict__ Hll,
                                                       const double* __restrict__ Hpl, const double* __restrict__ blocks,
                                                       double* __restrict__ out, int32_t* __restrict__ fail)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n)
        return;
    double* o = out + 18L * q;
    const int l = q_lm[q];
    double li[3][3];
    bool ok = l >= 0;
    if (ok && !chol3_inv(Hll + 9L * l, li)) // (a free landmark is factored under a fixed pose too: the flag is about it)
    {
        *fail = 1; // (every writer stores the same value)
        ok = false;
    }
    ok = ok && q_pose[q] >= 0;
    if (!ok)
    {
#pragma unroll
        for (int k = 0; k < 18; k++)
            o[k] = 0.0;
        return;
    }
    double acc[6][3];
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
        for (int c = 0; c < 3; c++)
            acc[r][c] = 0.0;
    const int s0 = q_ptr[q], ns = q_ptr[q + 1] - s0, e0 = lm_ptr[l];
    for (int k = 0; k < ns; k++)
    {
        if (flags[e0 + k] & (CUGO_EDGE_FIXED_L | CUGO_EDGE_FIXED_P | CUGO_EDGE_INACTIVE))
            continue;
        double g[6][3];
        lm_g(Hpl + 18L * (e0 + k), li, g);
        const double* __restrict__ S = blocks + 36L * q_slot[s0 + k];
#pragma unroll
        for (int j = 0; j < 6; j++) // acc += S[:, j] g[j, :], column by column of the block
#pragma unroll
            for (int r = 0; r < 6; r++)
            {
                const double s = S[r + 6 * j];
#pragma unroll
                for (int c = 0; c < 3; c++)
                    acc[r][c] += s * g[j][c];
            }
    }
    // -(acc L^-1): [r][c] = -sum_{k >= c} acc[r][k] Linv[k][c]
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int r = 0; r < 6; r++)
        {
            double s = acc[r][c] * li[c][c];
#pragma unroll
            for (int k = c + 1; k < 3; k++)
                s += acc[r][k] * li[k][c];
            o[r + 6 * c] = -s;
        }
}

// The lower triangle of S = J_p Sigma_aa J_p^T + X + X^T + J_l Sigma_ll J_l^T, X = J_p Sigma_al J_l^T, for both kernels
// below: the terms in this order, every sum in index order.  Saa [36] / Sal [18] / Sll [9] column-major; each is read only
// where its vertices are free
__device__ __forceinline__ void joint_cov_lower(const double JP[3][6], const double JL[3][3], bool free_p, bool free_l,
                                                const double* __restrict__ Saa, const double* __restrict__ Sal,
                                                const double* __restrict__ Sll, double S[3][3])
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            S[i][j] = 0.0;
    if (free_p)
    {
        // A = Sigma_aa J_p^T (6 x 3), then the lower triangle of J_p A
        double A[6][3];
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int j = 0; j < 3; j++)
            {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 6; k++)
                    s += Saa[r + 6 * k] * JP[j][k];
                A[r][j] = s;
            }
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j <= i; j++)
            {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 6; k++)
                    s += JP[i][k] * A[k][j];
                S[i][j] = s;
            }
    }
    if (free_p && free_l)
    {
        // B = Sigma_al J_l^T (6 x 3), X = J_p B; S += X + X^T on the lower triangle
        double B[6][3], X[3][3];
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int j = 0; j < 3; j++)
                B[r][j] = Sal[r] * JL[j][0] + Sal[r + 6] * JL[j][1] + Sal[r + 12] * JL[j][2];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++)
            {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 6; k++)
                    s += JP[i][k] * B[k][j];
                X[i][j] = s;
            }
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j <= i; j++)
                S[i][j] += X[i][j] + X[j][i];
    }
    if (free_l)
    {
        double C[3][3]; // Sigma_ll J_l^T
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int j = 0; j < 3; j++)
                C[r][j] = Sll[r] * JL[j][0] + Sll[r + 3] * JL[j][1] + Sll[r + 6] * JL[j][2];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j <= i; j++)
                S[i][j] += JL[i][0] * C[0][j] + JL[i][1] * C[1][j] + JL[i][2] * C[2][j];
    }
}

// Covariance of the reprojection of landmark l in pose a at the current estimates, S = J Sigma J^T over the joint
// [a; l] block with J = [J_p J_l] of ba_math.h, one thread per query:
//   S = J_p Sigma_aa J_p^T + X + X^T + J_l Sigma_ll J_l^T,   X = J_p Sigma_al J_l^T.
// q_pose / q_lm: indices into poses [.][7] / lms [.][3] (fixed vertices included); q_aa: the block of Sigma_aa in
// `blocks`, -1 for a fixed pose (the terms with J_p go); a landmark index >= Lfree is a fixed landmark (the terms with
// J_l go).  cross [n][18] (k_pose_lm_cross), lmcov [Lfree][9] (k_lm_covariance).  out [n][9]: the lower triangle,
// mirrored; the third row and column are zero for dim 2.
__global__ __launch_bounds__(256) void k_reprojection_cov(int n, int Lfree, const int32_t* __restrict__ q_pose,
                                                          const int32_t* __restrict__ q_lm, const int32_t* __restrict__ q_dim,
                                                          const int32_t* __restrict__ q_aa, const double* __restrict__ cam5,
                                                          const double* __restrict__ poses, const double* __restrict__ lms,
                                                          const double* __restrict__ blocks, const double* __restrict__ cross,
                                                          const double* __restrict__ lmcov, double* __restrict__ out)
{
    using namespace cugo_dev;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n)
        return;
    const double* __restrict__ pose = poses + 7L * q_pose[q];
    const int l = q_lm[q], aa = q_aa[q];
    const double* __restrict__ cam = cam5 + 5L * q;
    const bool stereo = q_dim[q] == 3, free_p = aa >= 0, free_l = l < Lfree;
    double Xc[3], JP[3][6], JL[3][3];
    world_to_cam(pose, lms + 3L * l, Xc);
    jac_pose(Xc, cam, stereo, JP);
    jac_landmark(Xc, pose, cam, stereo, JL);
    double S[3][3];
    joint_cov_lower(JP, JL, free_p, free_l, blocks + 36L * aa, cross + 18L * q, lmcov + 9L * l, S);
    double* o = out + 9L * q;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
        {
            const int rr = i > j ? i : j, cc = i > j ? j : i; // (the lower triangle, mirrored: exactly symmetric)
            o[i + 3 * j] = (!stereo && rr == 2) ? 0.0 : S[rr][cc];
        }
}

// Predicted observation and its covariance for every camera kind, one thread per query:
// z = the projection of Xs = M Xb + t_s, Xb = R(q_a) X_l + t_a, and S = J Sigma J^T with the build pass's Jacobians
// of z - m.  q_kind: CUGO_OBS_MONO (u, v), CUGO_OBS_STEREO (u, v, u_right), CUGO_OBS_DEPTH (u, v, 1 / Z_s; the row of
// DepthEdge with sd = 1, so S is in measurement units).  cam_tab [n][17] = {M row-major, t_s, k1..k4, model} per query,
// or NULL: every camera a pinhole at the pose, and for the kinds MONO / STEREO the operations of k_reprojection_cov
// in their order (the same bits).  A Kannala-Brandt entry has two rows whatever the kind (the edge kernels ignore
// the stereo bit there).  z is the residual of ba_math.h against a zero measurement under unit weight: e - 0 is e.
// The rest as k_reprojection_cov; z3 [n][3] holds 0 where a kind has no third row.
__global__ __launch_bounds__(256) void k_predict_obs(int n, int Lfree, const int32_t* __restrict__ q_pose,
                                                     const int32_t* __restrict__ q_lm, const int32_t* __restrict__ q_kind,
                                                     const int32_t* __restrict__ q_aa, const double* __restrict__ cam5,
                                                     const double* __restrict__ cam_tab, const double* __restrict__ poses,
                                                     const double* __restrict__ lms, const double* __restrict__ blocks,
                                                     const double* __restrict__ cross, const double* __restrict__ lmcov,
                                                     double* __restrict__ z3, double* __restrict__ out)
{
    using namespace cugo_dev;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n)
        return;
    const double* __restrict__ pose = poses + 7L * q_pose[q];
    const int l = q_lm[q], aa = q_aa[q], kind = q_kind[q];
    const double* __restrict__ cam = cam5 + 5L * q;
    const double* __restrict__ Xw = lms + 3L * l;
    const bool stereo = kind == CUGO_OBS_STEREO, depth = kind == CUGO_OBS_DEPTH;
    const bool free_p = aa >= 0, free_l = l < Lfree;
    const Robust none = {0, 1.0};
    bool rows3 = stereo || depth;
    EdgeGeom g;
    double JP[3][6], JL[3][3];
    if (!cam_tab)
    {
        edge_residual_k<true>(pose, Xw, 0.0, 0.0, 0.0, stereo, depth, 1.0, 1.0, cam, none, g);
        jac_pose_k<true>(g.Xc, cam, stereo, depth, 1.0, JP);
        jac_landmark_k<true>(g.Xc, pose, cam, stereo, depth, 1.0, JL);
    }
    else
    {
        const double* __restrict__ ext = cam_tab + 17L * q;
        double B[3][3], R[3][3];
        if (ext[16] != 0.0)
        {
            // (kb_terms is formed in edge_residual_rig and in rig_B from the same Xs, side by side in this branch: one
            // evaluation after inlining)
            edge_residual_rig<true>(pose, Xw, 0.0, 0.0, 0.0, false, 1.0, cam, ext, none, g);
            rig_B<true>(g.Xc, cam, ext, false, true, B);
            rows3 = false;
        }
        else
        {
            // A = JP[:, 3:6] of the pinhole at Xs, the depth row included (rig_B knows mono and stereo only); B = A M
            edge_residual_rig<true>(pose, Xw, 0.0, 0.0, 0.0, stereo, 1.0, cam, ext, none, g);
            double Xs[3], JPs[3][6];
            body_to_sensor(ext, g.Xc, Xs);
            jac_pose_k<true>(Xs, cam, stereo, depth, 1.0, JPs);
#pragma unroll
            for (int m = 0; m < 3; m++)
#pragma unroll
                for (int j = 0; j < 3; j++)
                    B[m][j] = JPs[m][3] * ext[j] + JPs[m][4] * ext[3 + j] + JPs[m][5] * ext[6 + j];
            if (depth)
                g.e[2] = 1.0 / Xs[2]; // (the third residual of edge_residual_k at sd = 1 against 0, taken at Xs)
        }
        quat_to_rot(pose, R);
        jac_pose_rig(g.Xc, B, JP);
        jac_landmark_rig(B, R, JL);
    }
    double S[3][3];
    joint_cov_lower(JP, JL, free_p, free_l, blocks + 36L * aa, cross + 18L * q, lmcov + 9L * l, S);
    double* oz = z3 + 3L * q;
    oz[0] = g.e[0], oz[1] = g.e[1], oz[2] = rows3 ? g.e[2] : 0.0;
    double* o = out + 9L * q;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
        {
            const int rr = i > j ? i : j, cc = i > j ? j : i; // (the lower triangle, mirrored: exactly symmetric)
            o[i + 3 * j] = (!rows3 && rr == 2) ? 0.0 : S[rr][cc];
        }
}

// out[p] = the diagonal block of pose p: the first block of row p of the upper block CSR
__global__ __launch_bounds__(256) void k_cov_pose_diag(int P, const int32_t* __restrict__ rowptr,
                                                       const double* __restrict__ sigma, double* __restrict__ out)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 36L * P)
        return;
    out[i] = sigma[36L * rowptr[i / 36] + i % 36];
}

// ---------------------------------------------------------------- blocks of the inverse off the pattern --------------
// (A + lambda I)^-1 [a, b] = Y_a^T Y_b with Y_v = L^-1 E_v (6 columns).  Y_v is non-zero only on the pivot columns of
// the fronts on the path from v's front to the root of the elimination tree: the boundary rows of a front are pivot
// columns of its ancestors, and every front of the path has one child on it, so one workgroup walks the path alone.
constexpr int XC_T = 256;     // workgroup size of both kernels
constexpr int XC_SLICES = 7;  // k_inv_pair_blocks: 7 x 36 threads, slice s sums the columns k = s (mod 7)

// One workgroup per distinct query row.  rows[g]: the row's block index in the solver's ordering; its workspace
// t = ws + g * 36 n ([6 n][6], zeroed by the caller) holds Y_v afterwards.
__global__ __launch_bounds__(XC_T) void k_inv_path_walk(CholPlanDev p, const double* __restrict__ fronts,
                                                        const int32_t* __restrict__ sparent,
                                                        const int32_t* __restrict__ rows, double* ws)
{
    __shared__ double tj[SI_N * 6]; // t_J, then y_J
    __shared__ double yj[SI_N * 6];
    const int tid = threadIdx.x;
    const int v = rows[blockIdx.x];
    double* t = ws + (size_t)blockIdx.x * 36 * (size_t)p.n;
    if (tid < 6)
        t[(6L * v + tid) * 6 + tid] = 1.0;
    __threadfence_block();
    __syncthreads();
    for (int f = p.col_front[v]; f >= 0; f = sparent[f])
    {
        const SelFront F = sel_front(p, fronts, f);
        double* tJ = t + 36L * p.col0[f];
        for (int e = tid; e < 6 * F.ncs; e += XC_T)
            tj[e] = tJ[e];
        __syncthreads();
        // y_J = W t_J: y[k][c] = sum_{j <= k} W[k][j] t[j][c], j ascending
        for (int e = tid; e < 6 * F.ncs; e += XC_T)
        {
            const int k = e % F.ncs, c = e / F.ncs;
            double s = 0.0;
#pragma unroll 8 // (the loads of eight steps in flight: the walk is bound by their latency)
            for (int j = 0; j <= k; j++)
                s += F.W[(long)j * F.ncp + k] * tj[6 * j + c];
            yj[6 * k + c] = s;
            tJ[6 * k + c] = s;
        }
        __syncthreads();
        // t_R -= L21 y_J, one boundary row per thread (the right-hand-side row behind a compact L21 is not a row of it)
        const int32_t* __restrict__ rb = p.rows + p.rows_ptr[f];
        for (int i = tid; i < F.nrs; i += XC_T)
        {
            double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
            for (int j = 0; j < F.ncs; j++)
            {
                const double l = F.L[(long)j * F.ldl + i];
#pragma unroll
                for (int c = 0; c < 6; c++)
                    acc[c] += l * yj[6 * j + c];
            }
            double* tr = t + (6L * rb[i / 6] + i % 6) * 6;
#pragma unroll
            for (int c = 0; c < 6; c++)
                tr[c] -= acc[c];
        }
        __threadfence_block();
        __syncthreads(); // this front's stores before the next front's loads
    }
}

// One workgroup per pair.  pairs[q] = {slot of a, slot of b, a's block index in the solver's ordering}; the sum runs
// over the pivot columns of a's path (Y_b is zero on those that are not on b's path too).  Slice s adds the columns
// k = s (mod 7) in ascending path order and the slices are added in order, whichever of the two paths is walked: the
// block of (b, a) is the transpose of the block of (a, b) bit for bit.
__global__ __launch_bounds__(XC_T) void k_inv_pair_blocks(CholPlanDev p, const int32_t* __restrict__ sparent,
                                                          const int32_t* __restrict__ pairs, const double* __restrict__ ws,
                                                          double* __restrict__ out)
{
    __shared__ double part[XC_SLICES * 36];
    const int tid = threadIdx.x;
    const int32_t* pr = pairs + 3L * blockIdx.x;
    const double* __restrict__ ya = ws + (size_t)pr[0] * 36 * (size_t)p.n;
    const double* __restrict__ yb = ws + (size_t)pr[1] * 36 * (size_t)p.n;
    if (tid < XC_SLICES * 36)
    {
        const int s = tid / 36, e = tid % 36, r = e % 6, c = e / 6;
        double acc = 0.0;
        for (int f = p.col_front[pr[2]]; f >= 0; f = sparent[f])
        {
            const long k0 = 6L * p.col0[f], k1 = k0 + 6L * p.ncb[f];
            for (long k = k0 + (s + XC_SLICES - (int)(k0 % XC_SLICES)) % XC_SLICES; k < k1; k += XC_SLICES)
                acc += ya[6 * k + r] * yb[6 * k + c];
        }
        part[tid] = acc;
    }
    __syncthreads();
    if (tid < 36)
    {
        double sum = part[tid];
#pragma unroll
        for (int s = 1; s < XC_SLICES; s++)
            sum += part[36 * s + tid];
        out[36L * blockIdx.x + tid] = sum; // column-major: rows a, columns b
    }
}

void ensure_lds(const void* fn, size_t bytes)
{
    if (bytes > 48 * 1024)
        (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

} // namespace

namespace cugo_k
{

void launch_selinv_rows(hipStream_t s, const CholPlanDev& p, const double* d_fronts, double* d_sig,
                        const int64_t* d_sinfo, const int32_t* d_items, int nitems)
{
    if (nitems <= 0)
        return;
    const size_t lds = SI_LDS_ROWS * sizeof(double);
    ensure_lds(reinterpret_cast<const void*>(k_selinv_rows), lds);
    CUGO_LAUNCH(k_selinv_rows, dim3(nitems), dim3(SI_T), lds, s, p, d_fronts, d_sig, d_sinfo, d_items);
}

void launch_selinv_jj(hipStream_t s, const CholPlanDev& p, const double* d_fronts, double* d_sig, int task0,
                      int ntasks)
{
    if (ntasks <= 0)
        return;
    const size_t lds = SI_LDS_JJ * sizeof(double);
    ensure_lds(reinterpret_cast<const void*>(k_selinv_jj), lds);
    CUGO_LAUNCH(k_selinv_jj, dim3(ntasks), dim3(SI_T), lds, s, p, d_fronts, d_sig, task0);
}

void launch_selinv_subtree(hipStream_t s, const CholPlanDev& p, const double* d_fronts, double* d_sig,
                           const int64_t* d_sinfo, int task0, int ntasks)
{
    if (ntasks <= 0)
        return;
    const size_t lds = std::max(SI_LDS_ROWS, SI_LDS_JJ) * sizeof(double);
    ensure_lds(reinterpret_cast<const void*>(k_selinv_subtree), lds);
    CUGO_LAUNCH(k_selinv_subtree, dim3(ntasks), dim3(SI_T), lds, s, p, d_fronts, d_sig, d_sinfo, task0);
}

void launch_selinv_gather(hipStream_t s, const CholPlanDev& p, const double* d_sig, double* d_out)
{
    const long n = 36L * p.n_hsc_blocks;
    if (n <= 0)
        return;
    CUGO_LAUNCH(k_selinv_gather, dim3((unsigned)((n + SI_T - 1) / SI_T)), dim3(SI_T), 0, s, p, d_sig, d_out);
}

int selinv_row_tile() { return SI_R; }

void launch_inv_path_walk(hipStream_t s, const CholPlanDev& p, const double* d_fronts, const int32_t* d_sparent,
                          const int32_t* d_rows, int nrows, double* d_ws)
{
    if (nrows <= 0)
        return;
    CUGO_LAUNCH(k_inv_path_walk, dim3(nrows), dim3(XC_T), 0, s, p, d_fronts, d_sparent, d_rows, d_ws);
}

void launch_inv_pair_blocks(hipStream_t s, const CholPlanDev& p, const int32_t* d_sparent, const int32_t* d_pairs,
                            int npairs, const double* d_ws, double* d_out)
{
    if (npairs <= 0)
        return;
    CUGO_LAUNCH(k_inv_pair_blocks, dim3(npairs), dim3(XC_T), 0, s, p, d_sparent, d_pairs, d_ws, d_out);
}

void launch_cov_pose_diag(hipStream_t s, int P, const int32_t* d_rowptr, const double* d_sigma, double* d_out)
{
    const long n = 36L * P;
    if (n <= 0)
        return;
    CUGO_LAUNCH(k_cov_pose_diag, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P, d_rowptr, d_sigma, d_out);
}

void launch_lm_covariance(hipStream_t s, int L, const int32_t* d_lm_ptr, const int32_t* d_e_pose,
                          const uint8_t* d_flags, const double* d_Hll, const double* d_Hpl, const int32_t* d_rowptr,
                          const int32_t* d_colind, const double* d_sigma, double* d_out, int32_t* d_fail)
{
    if (L <= 0)
        return;
    CUGO_LAUNCH(k_lm_covariance, dim3((L + 255) / 256), dim3(256), 0, s, L, d_lm_ptr, d_e_pose, d_flags, d_Hll, d_Hpl,
                d_rowptr, d_colind, d_sigma, d_out, d_fail);
}

void launch_pose_lm_cross(hipStream_t s, int n, const int32_t* d_q_pose, const int32_t* d_q_lm, const int32_t* d_q_ptr,
                          const int32_t* d_q_slot, const int32_t* d_lm_ptr, const uint8_t* d_flags, const double* d_Hll,
                          const double* d_Hpl, const double* d_blocks, double* d_out, int32_t* d_fail)
{
    if (n <= 0)
        return;
    CUGO_LAUNCH(k_pose_lm_cross, dim3((n + 255) / 256), dim3(256), 0, s, n, d_q_pose, d_q_lm, d_q_ptr, d_q_slot, d_lm_ptr,
                d_flags, d_Hll, d_Hpl, d_blocks, d_out, d_fail);
}

void launch_reprojection_cov(hipStream_t s, int n, int Lfree, const int32_t* d_q_pose, const int32_t* d_q_lm,
                             const int32_t* d_q_dim, const int32_t* d_q_aa, const double* d_cam5, const double* d_poses,
                             const double* d_lms, const double* d_blocks, const double* d_cross, const double* d_lmcov,
                             double* d_out)
{
    if (n <= 0)
        return;
    CUGO_LAUNCH(k_reprojection_cov, dim3((n + 255) / 256), dim3(256), 0, s, n, Lfree, d_q_pose, d_q_lm, d_q_dim, d_q_aa,
                d_cam5, d_poses, d_lms, d_blocks, d_cross, d_lmcov, d_out);
}

void launch_predict_obs(hipStream_t s, int n, int Lfree, const int32_t* d_q_pose, const int32_t* d_q_lm,
                        const int32_t* d_q_kind, const int32_t* d_q_aa, const double* d_cam5, const double* d_cam_tab,
                        const double* d_poses, const double* d_lms, const double* d_blocks, const double* d_cross,
                        const double* d_lmcov, double* d_z3, double* d_out)
{
    if (n <= 0)
        return;
    CUGO_LAUNCH(k_predict_obs, dim3((n + 255) / 256), dim3(256), 0, s, n, Lfree, d_q_pose, d_q_lm, d_q_kind, d_q_aa, d_cam5,
                d_cam_tab, d_poses, d_lms, d_blocks, d_cross, d_lmcov, d_z3, d_out);
}

} // namespace cugo_k
