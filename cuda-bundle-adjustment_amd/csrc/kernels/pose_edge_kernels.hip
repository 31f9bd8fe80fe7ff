// What the unary pose edge kinds share on the device side (point-to-plane / point-to-line: icp_kernels.hip, SE(3)
// priors: prior_kernels.hip): the sum of a pass's chi2 totals and the index check of a kind's (pose, pose_ptr) pair.
// Their shared __device__ pieces (tri6_unpack, pose_term_add) are in ba_math.h.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdexcept>
#include <string>

#include "kernels.h"

namespace
{

constexpr int POSE_WG = 256;

// chi2 total: the totals a pass left (ICP chunks, prior workgroups) in their order (one workgroup: strided per thread,
// then the threads in order)
__global__ __launch_bounds__(POSE_WG) void k_pose_chi_total(const double* __restrict__ pchi, int n, double* __restrict__ out,
                                                             int add)
{
    __shared__ double s[POSE_WG];
    double x = 0.0;
    for (int i = threadIdx.x; i < n; i += POSE_WG)
        x += pchi[i];
    s[threadIdx.x] = x;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        double tot = 0.0;
        for (int i = 0; i < POSE_WG; i++)
            tot += s[i];
        out[0] = add ? out[0] + tot : tot;
    }
}

// index check of one kind, with pose_ptr already known to ascend from 0 to n: every edge lies in its pose's range,
// i.e. the edges are sorted by pose and agree with pose_ptr.  Offending threads write 1 (no atomics needed).
__global__ __launch_bounds__(POSE_WG) void k_pose_check(const int32_t* __restrict__ pose, const int32_t* __restrict__ ptr,
                                                         int n, int P, int* __restrict__ bad)
{
    for (int i = blockIdx.x * POSE_WG + threadIdx.x; i < n; i += gridDim.x * POSE_WG)
    {
        const int q = pose[i];
        if (q < 0 || q >= P || i < ptr[q] || i >= ptr[q + 1])
            bad[0] = 1;
    }
}

} // namespace

namespace cugo_k
{

void launch_pose_chi_total(hipStream_t s, const char* label, const double* d_totals, int n, double* d_chi, bool chi_add)
{
    LaunchScope scope(label, s);
    hipLaunchKernelGGL(k_pose_chi_total, dim3(1), dim3(POSE_WG), 0, s, d_totals, n, d_chi, chi_add ? 1 : 0);
}

int pose_check_indices(hipStream_t s, const char* who, const PoseIndexCheck* kinds, int n_kinds, int n_poses_total, int* d_bad)
{
    if (hipMemsetAsync(d_bad, 0, sizeof(int), s) != hipSuccess)
        throw std::runtime_error("cugo: hipMemsetAsync failed");
    for (int k = 0; k < n_kinds; k++)
        if (kinds[k].n > 0)
        {
            const unsigned grid = (unsigned)std::min<size_t>(1024, ((size_t)kinds[k].n + POSE_WG - 1) / POSE_WG);
            LaunchScope scope(kinds[k].label, s);
            hipLaunchKernelGGL(k_pose_check, dim3(grid), dim3(POSE_WG), 0, s, kinds[k].d_pose, kinds[k].d_pose_ptr, kinds[k].n,
                               n_poses_total, d_bad);
        }
    int bad = 0;
    if (hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        throw std::runtime_error(std::string("cugo: ") + who + " index check failed to run");
    return bad;
}

} // namespace cugo_k
