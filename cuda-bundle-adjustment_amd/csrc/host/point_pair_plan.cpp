// Host plan of the pose-pose point edges: see point_pair_plan.h.  No HIP header.
#include "point_pair_plan.h"

#include <algorithm>
#include <numeric>
#include <stdexcept>
#include <string>

#include "../../../include/cugo_hip.h"

namespace cugo_host
{

namespace
{
[[noreturn]] void refuse(const std::string& what) { throw std::invalid_argument("cugo_point_pair_plan_create: " + what); }
} // namespace

void build_point_pair_plan(int n, int Pall, int P, const int32_t* pose_a, const int32_t* pose_b, const uint8_t* flags,
                           const int32_t* rowptr, const int32_t* colind, PointPairPlanHost& out)
{
    if (n < 0 || P < 0 || Pall < P)
        refuse("bad pose or edge counts");
    if (n > 0 && (!pose_a || !pose_b))
        refuse("missing index arrays");
    const bool pattern = rowptr != nullptr;
    if (pattern)
    {
        // ascending rowptr from 0, every row starts with its diagonal block, columns ascending and < P
        if (P > 0 && !colind)
            refuse("missing pattern");
        if (rowptr[0] != 0)
            refuse("rowptr does not start at 0");
        for (int p = 0; p < P; p++)
        {
            if (rowptr[p + 1] <= rowptr[p])
                refuse("row " + std::to_string(p) + " of the pattern is empty or rowptr descends");
            if (colind[rowptr[p]] != p)
                refuse("row " + std::to_string(p) + " of the pattern does not start with its diagonal block");
            for (int k = rowptr[p] + 1; k < rowptr[p + 1]; k++)
                if (colind[k] <= colind[k - 1] || colind[k] >= P)
                    refuse("row " + std::to_string(p) + " of the pattern is not ascending or leaves the free poses");
        }
    }
    else if (colind)
        refuse("colind without rowptr");
    for (int e = 0; e < n; e++)
    {
        const int a = pose_a[e], b = pose_b[e];
        if (a < 0 || a >= Pall || b < 0 || b >= Pall)
            refuse("edge " + std::to_string(e) + ": pose index out of range");
        if (a == b)
            refuse("edge " + std::to_string(e) + " joins pose " + std::to_string(a) + " to itself");
    }
    out = PointPairPlanHost{};
    out.n = n, out.n_poses_total = Pall, out.n_poses_free = P, out.nnzb = pattern ? rowptr[P] : 0;

    // the stable sort by (lo, hi, orientation)
    out.perm.resize((size_t)n);
    std::iota(out.perm.begin(), out.perm.end(), 0);
    auto key_less = [&](int32_t x, int32_t y) {
        const int lx = std::min(pose_a[x], pose_b[x]), hx = std::max(pose_a[x], pose_b[x]);
        const int ly = std::min(pose_a[y], pose_b[y]), hy = std::max(pose_a[y], pose_b[y]);
        if (lx != ly)
            return lx < ly;
        if (hx != hy)
            return hx < hy;
        return (pose_a[x] > pose_b[x]) < (pose_a[y] > pose_b[y]);
    };
    std::stable_sort(out.perm.begin(), out.perm.end(), key_less);

    // the runs
    out.edge_run.resize((size_t)n);
    for (int i = 0; i < n; i++)
    {
        const int e = out.perm[i], a = pose_a[e], b = pose_b[e];
        if (i == 0 || a != out.run_a.back() || b != out.run_b.back())
        {
            out.run_ptr.push_back(i);
            out.run_a.push_back(a);
            out.run_b.push_back(b);
            out.run_flags.push_back((a < P ? PAIR_RUN_A_FREE : 0) | (b < P ? PAIR_RUN_B_FREE : 0) | (a > b ? PAIR_RUN_A_IS_HI : 0));
        }
        const int r = (int)out.run_a.size() - 1;
        out.edge_run[i] = r;
        if (!(flags && (flags[e] & CUGO_EDGE_INACTIVE)) && (a < P || b < P))
            out.run_flags[r] |= PAIR_RUN_COUNTS;
    }
    out.run_ptr.push_back(n);
    const int R = (int)out.run_a.size();
    out.run_blk.assign((size_t)R, -1);

    // per run: the block; per block: its runs (adjacent: the two orientations of a pair follow one another)
    out.inc_ptr.assign((size_t)P + 1, 0);
    out.blk_ptr.push_back(0);
    for (int r = 0; r < R; r++)
    {
        const int a = out.run_a[r], b = out.run_b[r], f = out.run_flags[r];
        if (!(f & PAIR_RUN_COUNTS))
            continue;
        if (a < P)
            out.inc_ptr[a + 1]++;
        if (b < P)
            out.inc_ptr[b + 1]++;
        if (a >= P || b >= P)
            continue;
        const int lo = std::min(a, b), hi = std::max(a, b);
        const bool same_pair = !out.pair_lo.empty() && out.pair_lo.back() == lo && out.pair_hi.back() == hi;
        if (!same_pair)
        {
            out.pair_lo.push_back(lo);
            out.pair_hi.push_back(hi);
        }
        if (!pattern)
            continue;
        const int32_t *first = colind + rowptr[lo], *last = colind + rowptr[lo + 1];
        const int32_t* at = std::lower_bound(first, last, hi);
        if (at == last || *at != hi)
            refuse("run " + std::to_string(r) + ": block (" + std::to_string(lo) + ", " + std::to_string(hi) +
                   ") is missing from the pattern");
        out.run_blk[r] = (int32_t)(at - colind);
        if (same_pair)
            out.blk_ptr.back()++;
        else
        {
            out.blk_id.push_back(out.run_blk[r]);
            out.blk_ptr.push_back(out.blk_ptr.back() + 1);
        }
        out.blk_run.push_back(r);
    }

    // the incidence lists, runs ascending
    for (int p = 0; p < P; p++)
        out.inc_ptr[p + 1] += out.inc_ptr[p];
    out.inc.resize((size_t)out.inc_ptr[P]);
    std::vector<int32_t> fill(out.inc_ptr.begin(), out.inc_ptr.end() - 1);
    for (int r = 0; r < R; r++)
    {
        if (!(out.run_flags[r] & PAIR_RUN_COUNTS))
            continue;
        if (out.run_a[r] < P)
            out.inc[fill[out.run_a[r]]++] = r << 1;
        if (out.run_b[r] < P)
            out.inc[fill[out.run_b[r]]++] = r << 1 | 1;
    }
}

} // namespace cugo_host
