// Host plan of a batch of pose-landmark covariance queries: see plcov_plan.h.  No HIP header.
#include "plcov_plan.h"

#include <stdexcept>
#include <string>
#include <unordered_map>

namespace cugo_host
{

void build_plcov_plan(int P, int n_landmarks, const int32_t* lm_ptr, const int32_t* slot_pose, int n,
                      const int32_t* q_pose, const int32_t* q_lm, PlCovPlanHost& out)
{
    const std::string who = "cugo_plcov_plan_create";
    if (P < 0 || n_landmarks < 0 || n < 0)
        throw std::invalid_argument(who + ": negative count");
    if (n > 0 && (!q_pose || !q_lm))
        throw std::invalid_argument(who + ": null query array");
    out = PlCovPlanHost{};
    out.n = n;
    out.q_ptr.assign((size_t)n + 1, 0);
    out.q_aa.assign((size_t)n, -1);
    // One query pose against every landmark of a map asks for the same few pairs over and over: the block of a pair is
    // found by its key, behind a direct table for the row of the query pose at hand (a run of queries with one pose
    // then looks every pair up in the map once)
    std::unordered_map<int64_t, int32_t> where;
    std::vector<int32_t> row((size_t)P, -1), touched;
    int32_t row_of = -1;
    auto block_of = [&](int32_t a, int32_t b) {
        if (a != row_of)
        {
            for (int32_t c : touched)
                row[c] = -1;
            touched.clear();
            row_of = a;
        }
        if (row[b] < 0)
        {
            const auto it = where.emplace((int64_t)a * P + b, (int32_t)out.rows.size());
            if (it.second)
                out.rows.push_back(a), out.cols.push_back(b);
            row[b] = it.first->second;
            touched.push_back(b);
        }
        return row[b];
    };
    for (int k = 0; k < n; k++)
    {
        const int32_t a = q_pose[k], l = q_lm[k];
        if (a < -1 || a >= P || l < -1 || l >= n_landmarks)
            throw std::invalid_argument(who + ": query " + std::to_string(k) + " names a pose outside [-1, " +
                                        std::to_string(P) + ") or a landmark outside [-1, " + std::to_string(n_landmarks) + ")");
        if (a >= 0)
            out.q_aa[k] = block_of(a, a);
        if (a >= 0 && l >= 0)
        {
            if (!lm_ptr || lm_ptr[l] < 0 || lm_ptr[l + 1] < lm_ptr[l])
                throw std::invalid_argument(who + ": lm_ptr is null or does not ascend at landmark " + std::to_string(l));
            if (lm_ptr[l + 1] > lm_ptr[l] && !slot_pose)
                throw std::invalid_argument(who + ": null slot pose array");
            for (int32_t e = lm_ptr[l]; e < lm_ptr[l + 1]; e++)
            {
                const int32_t p = slot_pose[e];
                if (p < 0)
                    throw std::invalid_argument(who + ": slot " + std::to_string(e) + " has a negative pose index");
                out.q_slot.push_back(p < P ? block_of(a, p) : -1);
            }
        }
        if (out.q_slot.size() > (size_t)INT32_MAX)
            throw std::invalid_argument(who + ": more than 2^31 slot entries");
        out.q_ptr[(size_t)k + 1] = (int32_t)out.q_slot.size();
    }
}

} // namespace cugo_host
