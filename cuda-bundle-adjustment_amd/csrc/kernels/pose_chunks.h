// The chunked, atomics-free reduction of the key-sorted pose edge kinds (icp_kernels.hip, point_kernels.hip,
// point_pair_kernels.hip), once: the constants, the scratch layout and grids, the two wave reductions, the walk of a
// chunk, the finishing sum of a key's partials and the frame of a finishing kernel.
//
// A kind's edges are sorted by a KEY (the pose of a unary kind, the run of the pair kind).  The edge range is cut into
// chunks of ICP_CHUNK edges regardless of key boundaries, one wave per chunk; a chunk writes one partial of ICP_NP
// doubles (21 of the upper triangle of a 6 x 6 block or any 27 sums of the kind's choosing, then chi2) per key it
// touches.  Along the sorted edges chunk c and key q never decrease and one of them grows from one (chunk, key) pair to
// the next: c + q is a unique slot index — no prefix sums, no plan.  Every chunk also leaves ONE chi2 total, its
// partials in the order it wrote them.  No atomics, one fixed order; an error pass (FULL = false) forms the very chunk
// totals of the build pass and never touches elements 0-26 of a slot.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <climits>
#include <stdexcept>
#include <string>

#include "ba_math.h"
#include "kernels.h"

namespace cugo_dev
{

constexpr int ICP_CHUNK = 512; // edges per wave
constexpr int ICP_NP = 28;     // doubles per partial
constexpr int ICP_WG = 256;

__host__ __device__ __forceinline__ int chunk_count(int n) { return (n + ICP_CHUNK - 1) / ICP_CHUNK; }
// one range of sorted edges in a scratch: [roles x (chunks + n_keys) slots of ICP_NP | one chi2 total per chunk]
struct ChunkLayout
{
    size_t chunks, slots, cchi, end;
    __host__ __device__ ChunkLayout(int n, int n_keys, int roles = 1)
    {
        chunks = (size_t)(n + ICP_CHUNK - 1) / ICP_CHUNK;
        slots = chunks + (size_t)n_keys;
        cchi = roles * slots * ICP_NP;
        end = cchi + chunks;
    }
};
// workgroups of ICP_WG threads: a chunk pass of `waves` chunks, a finishing pass of 32 threads per free pose
inline unsigned chunk_grid(size_t waves) { return (unsigned)((waves * 64 + ICP_WG - 1) / ICP_WG); }
inline unsigned finish_grid(int n_poses_free) { return (unsigned)((32 * (size_t)n_poses_free + ICP_WG - 1) / ICP_WG); }
// partials at the front of rs, the chunk totals at cchi, `end` doubles in all
inline cugo_k::ChunkScratch chunk_scratch_in(cugo_k::ReduceScratch rs, size_t cchi, size_t end, const char* kind)
{
    if (rs.capacity < end)
        throw std::runtime_error(std::string("cugo: ") + kind + " scratch too small");
    return cugo_k::ChunkScratch{rs.d_partials, rs.d_partials + cchi};
}

// 32 accumulators -> their 64-lane sums; afterwards a[0] of lane L holds the sum of accumulator L >> 1
// (the halving exchange of ba_kernels.hip's wave_reduce32, fixed order)
__device__ __forceinline__ void icp_wave_reduce32(double (&a)[32])
{
    const int lane = threadIdx.x & 63;
#define CUGO_HALVE(N, OFF)                                     \
    {                                                          \
        const bool hi = (lane & OFF) != 0;                     \
        _Pragma("unroll") for (int i = 0; i < N; i++)          \
        {                                                      \
            const double send = hi ? a[i] : a[i + N];          \
            const double keep = hi ? a[i + N] : a[i];          \
            a[i] = keep + __shfl_xor(send, OFF, 64);           \
        }                                                      \
    }
    CUGO_HALVE(16, 32)
    CUGO_HALVE(8, 16)
    CUGO_HALVE(4, 8)
    CUGO_HALVE(2, 4)
    CUGO_HALVE(1, 2)
#undef CUGO_HALVE
    a[0] += __shfl_xor(a[0], 1, 64);
}

// sum over the wave in a fixed butterfly order (every lane gets it)
__device__ __forceinline__ double icp_wave_sum(double x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        x += __shfl_xor(x, off, 64);
    return x;
}

__device__ __forceinline__ void chunk_zero(double (&v)[32])
{
#pragma unroll
    for (int i = 0; i < 27; i++)
        v[i] = 0.0;
}

// One wave, chunk c of the n edges sorted by key[].  edge(e, in, q, v) -> chi2 term: the kind's liveness test and
// arithmetic for edge e of key q (in: e is inside the chunk; otherwise q is INT_MAX); with FULL it fills v[0..26], with
// zeros where the edge contributes nothing.  FULL: the partials of the 27 sums at slot c + q of part; CHI: element 27
// of the slot (the same value with and without FULL), the chunk's total in cchi[c] and, without FULL and with
// edge_chi, the chi2 term of every edge.  CHI_EARLY: element 27 is stored before the 27 sums are reduced instead of
// behind them.  Either order gives the same bits; it decides how long the value stays in a register, and with it the
// register allocation of the whole kernel: the pair kind's build kernel is 6 % slower with the late store, the unary
// kinds' kernels change with the early one (profiles/pose_chunks_refactor_ab.txt).
template <bool FULL, bool CHI, bool CHI_EARLY = false, class Edge>
__device__ __forceinline__ void chunk_walk(int n, const int32_t* key, int c, double* part, double* cchi, double* edge_chi, Edge edge)
{
    const int lane = threadIdx.x & 63;
    const int e0 = c * ICP_CHUNK, e1 = min(n, e0 + ICP_CHUNK);
    int qcur = key[e0]; // (wave-uniform)
    double acc[32];
#pragma unroll
    for (int i = 0; i < 32; i++)
        acc[i] = 0.0;
    double chi_acc = 0.0, chunk_chi = 0.0;
    auto flush = [&](int q) {
        double cs = 0.0;
        if (CHI)
        {
            cs = icp_wave_sum(chi_acc);
            chunk_chi += cs; // (the same value in every lane)
        }
        double* out = part + (size_t)(c + q) * ICP_NP;
        if (CHI && CHI_EARLY && lane == 0)
            out[27] = cs;
        if (FULL)
        {
            icp_wave_reduce32(acc);
            if (!(lane & 1) && (lane >> 1) < 27)
                out[lane >> 1] = acc[0];
#pragma unroll
            for (int i = 0; i < 32; i++)
                acc[i] = 0.0;
        }
        if (CHI && !CHI_EARLY && lane == 0)
            out[27] = cs;
        chi_acc = 0.0;
    };
    for (int base = e0; base < e1; base += 64)
    {
        const int e = base + lane;
        const bool in = e < e1;
        const int q = in ? key[e] : INT_MAX;
        double v[32];
        const double chi = edge(e, in, q, v);
        if (!FULL && edge_chi && in)
            edge_chi[e] = chi;
        // the keys of the 64 lanes ascend: the lanes of each key in turn join the wave's accumulators
        for (;;)
        {
            if (q == qcur)
            {
                if (CHI)
                    chi_acc += chi;
                if (FULL)
                {
#pragma unroll
                    for (int i = 0; i < 27; i++)
                        acc[i] += v[i];
                }
            }
            const unsigned long long later = __ballot(in && q > qcur);
            if (later == 0)
                break;
            const int qn = __shfl(q, __ffsll((long long)later) - 1, 64);
            flush(qcur);
            qcur = qn;
        }
    }
    flush(qcur);
    if (CHI && lane == 0)
        cchi[c] = chunk_chi;
}

// element t of key q's partials, summed in chunk order (ptr: the CSR of the sorted edges over the keys).  MAY_BE_EMPTY:
// a key without edges (a pose of a unary kind; a run never is) has no slot and gives 0
template <bool MAY_BE_EMPTY = true>
__device__ __forceinline__ double chunk_key_sum(const int32_t* __restrict__ ptr, const double* __restrict__ part, int q, int t)
{
    const int i0 = ptr[q], i1 = ptr[q + 1];
    double s = 0.0;
    if (!MAY_BE_EMPTY || i1 > i0)
        for (int c = i0 / ICP_CHUNK, c1 = (i1 - 1) / ICP_CHUNK; c <= c1; c++)
            s += part[(size_t)(c + q) * ICP_NP + t];
    return s;
}

// The frame of a finishing kernel: 32 threads per free pose; thread t < 27 adds sum(p, t), element t of pose p's sums,
// to Hpp / bp (SCHUR = false: behind k_build_poses) or to the diagonal block of Hsc (the first block of the pose's row,
// through rowptr), to bp and to bsc (SCHUR = true: behind k_pose_schur, which WRITES the three in the one-stream form
// of the loop; there Hpp is not formed at all, and a pose's terms enter its row of the Schur complement unchanged, as
// Hpp does).  A pose without terms (has_terms(p) false) keeps the bits of its blocks: its slots were never written
template <bool SCHUR, class Has, class Sum>
__device__ __forceinline__ void chunk_finish(int n_poses_free, Has has_terms, Sum sum, double* H, const int32_t* rowptr, double* bp,
                                             double* bsc)
{
    const int p = (int)((blockIdx.x * (size_t)ICP_WG + threadIdx.x) >> 5), t = threadIdx.x & 31;
    if (p >= n_poses_free || t >= 27)
        return;
    if (!has_terms(p))
        return;
    const double s = sum(p, t);
    int r = 0, c = 0;
    if (t < 21)
        tri6_unpack(t, r, c);
    pose_term_add<SCHUR>(p, t, r, c, s, H, rowptr, bp, bsc);
}

} // namespace cugo_dev
