// The chunked, atomics-free reduction of the pose-sorted unary edge kinds (icp_kernels.hip, point_kernels.hip): the
// constants, the two wave reductions and the finishing sum of a pose's partials.  See icp_kernels.hip for the layout:
// chunks of ICP_CHUNK edges, one wave per chunk, a partial of ICP_NP doubles at slot chunk + pose, one chi2 total per
// chunk.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cugo_dev
{

constexpr int ICP_CHUNK = 512; // edges per wave
constexpr int ICP_NP = 28;     // doubles per partial
constexpr int ICP_WG = 256;

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

// sum of pose p's partials, element t, in chunk order (pose_ptr: the CSR of the kind's sorted edges over the poses)
__device__ __forceinline__ double chunk_pose_sum(const int32_t* __restrict__ pose_ptr, const double* __restrict__ part, int p, int t)
{
    const int i0 = pose_ptr[p], i1 = pose_ptr[p + 1];
    double s = 0.0;
    if (i1 > i0)
        for (int c = i0 / ICP_CHUNK, c1 = (i1 - 1) / ICP_CHUNK; c <= c1; c++)
            s += part[(size_t)(c + p) * ICP_NP + t];
    return s;
}

} // namespace cugo_dev
