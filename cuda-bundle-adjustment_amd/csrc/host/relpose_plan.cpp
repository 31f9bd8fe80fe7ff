// Host plan of the relative-pose edges: see relpose_plan.h.  No HIP header.
#include "relpose_plan.h"

#include <algorithm>
#include <stdexcept>
#include <string>

#include "../../../include/cugo_hip.h"

namespace cugo_host
{

namespace
{
[[noreturn]] void refuse(const char* who, const std::string& what) { throw std::invalid_argument(std::string(who) + ": " + what); }

bool counts(const uint8_t* flags, int e, int a, int b, int P)
{
    return !(flags && (flags[e] & CUGO_EDGE_INACTIVE)) && (a < P || b < P);
}
} // namespace

void build_relpose_plan(int n, int Pall, int P, const int32_t* pose_a, const int32_t* pose_b, const uint8_t* flags,
                        const int32_t* rowptr, const int32_t* colind, RelPosePlanHost& out)
{
    const char* who = "cugo_relpose_plan_create";
    if (n < 0 || P < 0 || Pall < P)
        refuse(who, "bad pose or edge counts");
    if (n > 0 && (!pose_a || !pose_b))
        refuse(who, "missing index arrays");
    if (!rowptr || (P > 0 && !colind))
        refuse(who, "missing pattern");
    // the pattern: ascending rowptr from 0, every row starts with its diagonal block, columns ascending and < P
    if (rowptr[0] != 0)
        refuse(who, "rowptr does not start at 0");
    for (int p = 0; p < P; p++)
    {
        if (rowptr[p + 1] <= rowptr[p])
            refuse(who, "row " + std::to_string(p) + " of the pattern is empty or rowptr descends");
        if (colind[rowptr[p]] != p)
            refuse(who, "row " + std::to_string(p) + " of the pattern does not start with its diagonal block");
        for (int k = rowptr[p] + 1; k < rowptr[p + 1]; k++)
            if (colind[k] <= colind[k - 1] || colind[k] >= P)
                refuse(who, "row " + std::to_string(p) + " of the pattern is not ascending or leaves the free poses");
    }
    out = RelPosePlanHost{};
    out.n = n, out.n_poses_total = Pall, out.n_poses_free = P, out.nnzb = rowptr[P];
    out.inc_ptr.assign((size_t)P + 1, 0);
    out.off_blk.assign((size_t)n, -1);
    for (int e = 0; e < n; e++)
    {
        const int a = pose_a[e], b = pose_b[e];
        if (a < 0 || a >= Pall || b < 0 || b >= Pall)
            refuse(who, "edge " + std::to_string(e) + ": pose index out of range");
        if (a == b)
            refuse(who, "edge " + std::to_string(e) + " joins pose " + std::to_string(a) + " to itself");
        if (!counts(flags, e, a, b, P))
            continue;
        if (a < P)
            out.inc_ptr[a + 1]++;
        if (b < P)
            out.inc_ptr[b + 1]++;
        if (a < P && b < P)
        {
            const int lo = std::min(a, b), hi = std::max(a, b);
            const int32_t *first = colind + rowptr[lo], *last = colind + rowptr[lo + 1];
            const int32_t* at = std::lower_bound(first, last, hi);
            if (at == last || *at != hi)
                refuse(who, "edge " + std::to_string(e) + ": block (" + std::to_string(lo) + ", " + std::to_string(hi) +
                                ") is missing from the pattern");
            out.off_blk[e] = (int32_t)(at - colind);
        }
    }
    for (int p = 0; p < P; p++)
        out.inc_ptr[p + 1] += out.inc_ptr[p];
    out.inc.resize((size_t)out.inc_ptr[P]);
    std::vector<int32_t> fill(out.inc_ptr.begin(), out.inc_ptr.end() - 1);
    for (int e = 0; e < n; e++) // (edge order inside every list)
    {
        const int a = pose_a[e], b = pose_b[e];
        if (!counts(flags, e, a, b, P))
            continue;
        if (a < P)
            out.inc[fill[a]++] = e << 1;
        if (b < P)
            out.inc[fill[b]++] = e << 1 | 1;
    }
}

int relpose_pattern(int n, int P, const int32_t* pose_a, const int32_t* pose_b, const uint8_t* flags, int32_t* rowptr,
                    int32_t* colind)
{
    const char* who = "cugo_relpose_pattern";
    if (n < 0 || P < 0 || (n > 0 && (!pose_a || !pose_b)))
        refuse(who, "bad counts or missing index arrays");
    std::vector<std::vector<int32_t>> rows((size_t)P);
    for (int e = 0; e < n; e++)
    {
        const int a = pose_a[e], b = pose_b[e];
        if (a < 0 || b < 0)
            refuse(who, "edge " + std::to_string(e) + ": negative pose index");
        if (a == b)
            refuse(who, "edge " + std::to_string(e) + " joins pose " + std::to_string(a) + " to itself");
        if (a < P && b < P && counts(flags, e, a, b, P))
            rows[std::min(a, b)].push_back(std::max(a, b));
    }
    int nnzb = 0;
    for (int p = 0; p < P; p++)
    {
        std::vector<int32_t>& r = rows[p];
        std::sort(r.begin(), r.end());
        r.erase(std::unique(r.begin(), r.end()), r.end());
        if (rowptr)
            rowptr[p] = nnzb;
        if (colind)
        {
            colind[nnzb] = p;
            std::copy(r.begin(), r.end(), colind + nnzb + 1);
        }
        nnzb += 1 + (int)r.size();
    }
    if (rowptr)
        rowptr[P] = nnzb;
    return nnzb;
}

} // namespace cugo_host
