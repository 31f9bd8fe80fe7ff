// What the unary pose edge kinds share on the device side (point-to-plane / point-to-line: icp_kernels.hip, SE(3)
// priors: prior_kernels.hip): the sum of a pass's chi2 totals and the index check of a kind's (pose, pose_ptr) pair.
// Their shared __device__ pieces (tri6_unpack, pose_term_add) are in ba_math.h.
// And what all four pose edge kinds share, the relative-pose edges included: the outlier pass over the chi2 term of every
// edge (k_pose_reject_count / _scan / _place).
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

// ---- outlier pass (ref: computeOutliersKernel, cuda_block_solver.cu:1145, and EdgeSet::updateEdges) -----------------
// Lane per edge.  Workgroup b owns the contiguous run of `tiles` tiles of POSE_WG edges from tile b * tiles on, so the
// list comes out ascending: the count pass leaves every workgroup's number of outliers, one wave turns the counts into
// offsets (and the total), and the place pass walks the same tiles again, a lane's position being
//   offset of its workgroup + outliers of the tiles before + of the waves before in the tile + of the lanes before in the wave
// (__ballot / popcount).  Nothing but comparisons and integer sums: no atomics, no floating-point arithmetic; a lane
// stores its own flag byte and its own list entry and nothing else.
constexpr int REJECT_GRID_CAP = 1024;

__device__ __forceinline__ bool pose_edge_is_outlier(int e, int n, const double* __restrict__ chi, const double* __restrict__ thr,
                                                     int per_edge, const uint8_t* __restrict__ flags)
{
    if (e >= n || (flags[e] & CUGO_EDGE_INACTIVE))
        return false;
    const double t = thr[per_edge ? e : 0];
    return t > 0.0 && chi[e] > t; // (strict: a NaN chi2 or threshold keeps the edge)
}

__global__ __launch_bounds__(POSE_WG) void k_pose_reject_count(int n, int tiles, const double* __restrict__ chi,
                                                                const double* __restrict__ thr, int per_edge,
                                                                const uint8_t* __restrict__ flags, int32_t* __restrict__ counts)
{
    __shared__ int s_w[POSE_WG / 64];
    const int tile0 = blockIdx.x * tiles;
    int cnt = 0; // (the same in every lane of a wave)
    for (int t = 0; t < tiles && (tile0 + t) * POSE_WG < n; t++)
        cnt += __popcll(__ballot(pose_edge_is_outlier((tile0 + t) * POSE_WG + (int)threadIdx.x, n, chi, thr, per_edge, flags)));
    if ((threadIdx.x & 63) == 0)
        s_w[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        int tot = 0;
        for (int w = 0; w < POSE_WG / 64; w++)
            tot += s_w[w];
        counts[blockIdx.x] = tot;
    }
}

// one wave: counts[0 .. G) -> their exclusive prefix sums in place, the total in counts[G] (G <= REJECT_GRID_CAP)
__global__ __launch_bounds__(64) void k_pose_reject_scan(int G, int32_t* __restrict__ counts)
{
    const int lane = threadIdx.x, per = (G + 63) / 64;
    const int i0 = lane * per, i1 = min(i0 + per, G);
    int mine = 0;
    for (int i = i0; i < i1; i++)
        mine += counts[i];
    int incl = mine;
    for (int d = 1; d < 64; d <<= 1)
    {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d)
            incl += up;
    }
    int run = incl - mine;
    for (int i = i0; i < i1; i++)
    {
        const int c = counts[i];
        counts[i] = run;
        run += c;
    }
    if (lane == 63)
        counts[G] = incl;
}

__global__ __launch_bounds__(POSE_WG) void k_pose_reject_place(int n, int tiles, const double* __restrict__ chi,
                                                                const double* __restrict__ thr, int per_edge,
                                                                uint8_t* __restrict__ flags, const int32_t* __restrict__ offsets,
                                                                int32_t* __restrict__ rejected)
{
    __shared__ int s_w[POSE_WG / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile0 = blockIdx.x * tiles;
    int base = offsets[blockIdx.x];
    for (int t = 0; t < tiles && (tile0 + t) * POSE_WG < n; t++)
    {
        const int e = (tile0 + t) * POSE_WG + (int)threadIdx.x;
        const bool out = pose_edge_is_outlier(e, n, chi, thr, per_edge, flags);
        const unsigned long long mask = __ballot(out);
        if (lane == 0)
            s_w[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, tot = 0;
        for (int w = 0; w < POSE_WG / 64; w++)
        {
            const int c = s_w[w];
            before += w < wave ? c : 0;
            tot += c;
        }
        if (out)
        {
            rejected[base + before + __popcll(mask & ((1ull << lane) - 1ull))] = e;
            flags[e] = (uint8_t)(flags[e] | CUGO_EDGE_INACTIVE);
        }
        base += tot;
        __syncthreads();
    }
}

} // namespace

namespace cugo_k
{

// workgroups of the outlier pass over n edges, and the tiles each of them walks
static int pose_reject_grid(int n, int* tiles)
{
    const int ntiles = (n + POSE_WG - 1) / POSE_WG;
    *tiles = (ntiles + REJECT_GRID_CAP - 1) / REJECT_GRID_CAP;
    return *tiles ? (ntiles + *tiles - 1) / *tiles : 0;
}
int pose_reject_grid_cap() { return REJECT_GRID_CAP; }
size_t pose_reject_work_ints(int n)
{
    int tiles;
    return (size_t)pose_reject_grid(n, &tiles) + 1;
}
const int32_t* launch_pose_reject(hipStream_t s, int n, const double* d_edge_chi, const double* d_threshold, bool per_edge,
                                  uint8_t* d_flags, int32_t* d_rejected, int32_t* d_work)
{
    int tiles;
    const int grid = pose_reject_grid(n, &tiles);
    if (!grid)
        return nullptr;
    CUGO_LAUNCH(k_pose_reject_count, dim3(grid), dim3(POSE_WG), 0, s, n, tiles, d_edge_chi, d_threshold, per_edge ? 1 : 0,
                d_flags, d_work);
    CUGO_LAUNCH(k_pose_reject_scan, dim3(1), dim3(64), 0, s, grid, d_work);
    CUGO_LAUNCH(k_pose_reject_place, dim3(grid), dim3(POSE_WG), 0, s, n, tiles, d_edge_chi, d_threshold, per_edge ? 1 : 0,
                d_flags, d_work, d_rejected);
    return d_work + grid;
}

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
