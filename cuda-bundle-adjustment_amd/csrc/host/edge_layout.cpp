// Host-only layout of a flattened graph (edge_layout.h).
// ref: src/optimisable_graph.hpp:474-572 (EdgeSet::init), src/sparse_block_matrix.cpp:63-156 (Hsc pattern).
#include "edge_layout.h"
#include "point_pair_plan.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <numeric>
#include <stdexcept>
#include <string>

#include "thread_pool.h"

namespace cugo_host
{

bool same_bytes(const void* a, const void* b, size_t bytes)
{
    const char* pa = static_cast<const char*>(a);
    const char* pb = static_cast<const char*>(b);
    std::atomic<bool> eq{true};
    parallel_chunks(bytes, 1u << 18, [&](size_t lo, size_t hi, unsigned) {
        for (size_t o = lo; o < hi && eq.load(std::memory_order_relaxed); o += 1u << 16)
            if (std::memcmp(pa + o, pb + o, std::min<size_t>(1u << 16, hi - o)) != 0)
                eq.store(false, std::memory_order_relaxed);
    });
    return eq.load();
}

double count_free_free(const std::vector<uint8_t>& flags)
{
    std::atomic<int64_t> n{0};
    parallel_chunks(flags.size(), 100000, [&](size_t a, size_t b, unsigned) {
        n += std::count_if(flags.begin() + a, flags.begin() + b, is_free_free);
    });
    return (double)n.load();
}

// ---- landmark-major order: stable counting sort by landmark (threads own landmark ranges), then by pose inside ----
namespace
{
// insertion sort by pose index inside every landmark (a landmark has few edges)
void sort_by_pose(const FlatGraph& g, const Idx& lm_cnt, Idx& order)
{
    parallel_chunks((size_t)g.Lall, 65536, [&](size_t la, size_t lb, unsigned) {
        for (size_t l = la; l < lb; l++)
        {
            int32_t* b = order.data() + lm_cnt[l];
            const int k = lm_cnt[l + 1] - lm_cnt[l];
            for (int i = 1; i < k; i++)
            {
                const int32_t v = b[i];
                const int pv = g.e_pose[v];
                int j = i - 1;
                for (; j >= 0 && g.e_pose[b[j]] > pv; j--)
                    b[j + 1] = b[j];
                b[j + 1] = v;
            }
        }
    });
}

// Callers usually add the edges landmark by landmark (ORB-SLAM2 walks its map points): then the counting sort is the
// identity, and a landmark ends where the next one starts.
void sort_identity(const FlatGraph& g, Idx& lm_cnt, Idx& order)
{
    const int32_t* elm = g.e_lm.data();
    const size_t Etot = (size_t)g.n_edges();
    parallel_chunks(Etot, 100000, [&](size_t a, size_t b, unsigned) {
        for (size_t e = a; e < b; e++)
        {
            order[e] = (int32_t)e;
            if (e + 1 == Etot || elm[e + 1] != elm[e])
                lm_cnt[elm[e] + 1] = (int32_t)(e + 1);
        }
    });
    for (int l = 0; l < g.Lall; l++) // (a landmark without edges ends where it starts)
        lm_cnt[l + 1] = std::max(lm_cnt[l + 1], lm_cnt[l]);
}

constexpr int kMaxRuns = 64;

// starts of the sorted runs of the container order, the end of the last one behind them (at most kMaxRuns + 1 per
// chunk are looked for: more than kMaxRuns in all and the merge is not taken)
Idx sorted_runs(const FlatGraph& g)
{
    const int32_t* elm = g.e_lm.data();
    std::vector<int32_t> run_start(1, 0);
    std::vector<std::vector<int32_t>> desc(pool_threads());
    parallel_chunks((size_t)g.n_edges(), 100000, [&](size_t a, size_t b, unsigned t) {
        for (size_t e = std::max<size_t>(a, 1); e < b && desc[t].size() <= (size_t)kMaxRuns; e++)
            if (elm[e - 1] > elm[e])
                desc[t].push_back((int32_t)e);
    });
    for (const auto& d : desc)
        run_start.insert(run_start.end(), d.begin(), d.end());
    run_start.push_back(g.n_edges());
    return run_start;
}

// Not sorted as a whole — but callers add their edges set by set and, inside a set, landmark by landmark (the
// reference sample: all mono edges, then all stereo edges, each in landmark order): the container order is a FEW
// sorted runs.  Then the counting sort is a merge of runs: a thread owns a landmark range, finds its part of every
// run by binary search and lays the edges of each landmark down run after run (= container order: stable).  O(E)
// work in all, where the general path has every thread scan all edges twice.  The landmark starts go straight into
// lm_cnt: nothing is counted.
void sort_merge_runs(const FlatGraph& g, const Idx& run_start, Idx& lm_cnt, Idx& order)
{
    const int32_t* elm = g.e_lm.data();
    const int nruns = (int)run_start.size() - 1, Lall = g.Lall;
    const unsigned nt = std::max(1u, std::min<unsigned>(pool_threads(), (unsigned)std::max(1, Lall / 1024)));
    auto lrange = [&](unsigned t) { return (size_t)Lall * t / nt; };
    auto run_lo = [&](int r, size_t l) {
        return (int32_t)(std::lower_bound(elm + run_start[r], elm + run_start[r + 1], (int32_t)l) - elm);
    };
    pool_for(nt, [&](unsigned t) {
        const size_t la = lrange(t), lb = lrange(t + 1);
        if (la == lb)
            return;
        std::vector<int32_t> cur(nruns), lim(nruns);
        for (int r = 0; r < nruns; r++)
            cur[r] = run_lo(r, la), lim[r] = run_lo(r, lb);
        int32_t pos = 0; // the edges of the landmarks before la
        for (int r = 0; r < nruns; r++)
            pos += cur[r] - run_start[r];
        for (size_t l = la; l < lb; l++)
        {
            lm_cnt[l] = pos; // (start of landmark l; lm_cnt[Lall] is set below)
            for (int r = 0; r < nruns; r++)
                while (cur[r] < lim[r] && elm[cur[r]] == (int32_t)l)
                    order[pos++] = cur[r]++;
        }
    });
    lm_cnt[Lall] = g.n_edges();
}

// any order: every thread scans all edges (8 B per edge, from cache) for those of its own landmarks, twice
void sort_general(const FlatGraph& g, Idx& lm_cnt, Idx& order)
{
    const int32_t* elm = g.e_lm.data();
    const int Etot = g.n_edges();
    parallel_chunks((size_t)g.Lall, 65536, [&](size_t la, size_t lb, unsigned) {
        for (int e = 0; e < Etot; e++)
        {
            const size_t l = (size_t)elm[e];
            if (l >= la && l < lb)
                lm_cnt[l + 1]++;
        }
    });
    std::partial_sum(lm_cnt.begin(), lm_cnt.end(), lm_cnt.begin());
    parallel_chunks((size_t)g.Lall, 65536, [&](size_t la, size_t lb, unsigned) {
        if (la == lb)
            return;
        std::vector<int32_t> pos(lm_cnt.begin() + la, lm_cnt.begin() + lb);
        for (int e = 0; e < Etot; e++)
        {
            const size_t l = (size_t)elm[e];
            if (l >= la && l < lb)
                order[pos[l - la]++] = e;
        }
    });
}
} // namespace

void sort_landmark_major(const FlatGraph& g, Idx& lm_cnt, Idx& order)
{
    lm_cnt.assign(g.Lall + 1, 0);
    order.resize(g.n_edges());
    const Idx run_start = sorted_runs(g);
    const int nruns = (int)run_start.size() - 1;
    if (nruns == 1)
        sort_identity(g, lm_cnt, order);
    else if (nruns <= kMaxRuns)
        sort_merge_runs(g, run_start, lm_cnt, order);
    else
        sort_general(g, lm_cnt, order);
    sort_by_pose(g, lm_cnt, order);
}

void build_covisibility(const FlatGraph& g, const Idx& lm_cnt, const Idx& order, Idx& cov_ptr, Idx& cov_pose)
{
    const int L = g.L;
    auto is_ff = [&](int e) { return is_free_free(g.e_flags[e]); };
    cov_ptr.assign(L + 1, 0);
    parallel_chunks((size_t)L, 65536, [&](size_t la, size_t lb, unsigned) {
        for (size_t l = la; l < lb; l++)
        {
            int c = 0;
            for (int i = lm_cnt[l]; i < lm_cnt[l + 1]; i++)
                c += is_ff(order[i]);
            cov_ptr[l + 1] = c;
        }
    });
    std::partial_sum(cov_ptr.begin(), cov_ptr.end(), cov_ptr.begin());
    cov_pose.resize((size_t)cov_ptr[L]);
    std::atomic<int> dup_lm{-1};
    parallel_chunks((size_t)L, 65536, [&](size_t la, size_t lb, unsigned) {
        for (size_t l = la; l < lb; l++)
        {
            int o = cov_ptr[l];
            for (int i = lm_cnt[l]; i < lm_cnt[l + 1]; i++)
                if (is_ff(order[i]))
                {
                    // (the edges of a landmark are sorted by pose: equal poses are neighbours)
                    if (o > cov_ptr[l] && cov_pose[o - 1] == g.e_pose[order[i]])
                        dup_lm.store((int)l, std::memory_order_relaxed);
                    cov_pose[o++] = g.e_pose[order[i]];
                }
        }
    });
    // Two active edges between the same free pose and free landmark: the reference stores ONE Hpl block
    // per (pose, landmark) pair and forms only one of the two cross products of such a pair
    // (ref: .cu:1347-1378 iterates j >= i inside a column), i.e. it has no defined behaviour for them;
    // here every structure (Hpl slots, Hsc lists, the device structure build) assumes distinct pairs.
    if (dup_lm.load() >= 0)
        throw std::runtime_error("cugo: two active edges join the same free pose and free landmark (landmark index " +
                                 std::to_string(dup_lm.load()) + "): duplicate (pose, landmark) edges are not supported");
}

void shard_range(const Idx& lm_cnt, int rank, int world, int& l0, int& l1)
{
    const int Lall = (int)lm_cnt.size() - 1;
    l0 = 0, l1 = Lall;
    if (world <= 1)
        return;
    const int64_t Etot = lm_cnt[Lall];
    auto cut = [&](int r) {
        const int64_t target = Etot * r / world;
        return (int)(std::lower_bound(lm_cnt.begin(), lm_cnt.end(), (int32_t)target) - lm_cnt.begin());
    };
    l0 = rank == 0 ? 0 : std::min(cut(rank), Lall);
    l1 = rank == world - 1 ? Lall : std::min(cut(rank + 1), Lall);
    if (l1 < l0)
        l1 = l0;
}

bool pad_slot_layout(const Idx& lm_cnt, int l0, int l1, Idx& lm_ptr, Idx& slot_src)
{
    const int Lall = (int)lm_cnt.size() - 1;
    lm_ptr.assign(Lall + 1, 0);
    // first the start slot of every landmark (sequential: a padding decision moves everything
    // behind it), then the slots are filled per landmark range in parallel
    int pos = 0, last_l = -1; // last_l: last landmark that owns slots
    for (int l = l0; l < l1; l++)
    {
        const int k = lm_cnt[l + 1] - lm_cnt[l];
        if (k > 0 && k <= kSlotGroup && pos % kSlotGroup + k > kSlotGroup && last_l >= 0)
        {
            pos += kSlotGroup - pos % kSlotGroup;
            for (int q = last_l + 1; q <= l; q++)
                lm_ptr[q] = pos; // the padding extends landmark last_l
        }
        lm_ptr[l] = pos;
        pos += k;
        if (k > 0)
            last_l = l;
    }
    const int total = pos;
    slot_src.assign((size_t)total, -1);
    parallel_chunks((size_t)(l1 - l0), 65536, [&](size_t a, size_t b, unsigned) {
        for (size_t q = a; q < b; q++)
        {
            const int l = l0 + (int)q;
            int32_t* dst = slot_src.data() + lm_ptr[l]; // (the fix-ups only move landmarks without edges)
            for (int i = lm_cnt[l]; i < lm_cnt[l + 1]; i++)
                *dst++ = i;
        }
    });
    for (int l = l1; l <= Lall; l++)
        lm_ptr[l] = total;
    // lm_ptr[l] for l < l0 stays 0; fix up the entries between padded landmarks
    for (int l = l0 + 1; l <= l1; l++)
        lm_ptr[l] = std::max(lm_ptr[l], lm_ptr[l - 1]);
    for (int l = 0; l < Lall; l++)
        if (lm_ptr[l + 1] > lm_ptr[l] && lm_ptr[l] / kSlotGroup != (lm_ptr[l + 1] - 1) / kSlotGroup)
            return false;
    return true;
}

void fill_slots(const FlatGraph& g, const Idx& order, const Idx& slot_src, SlotArrays& out)
{
    const size_t E = slot_src.size();
    std::vector<double>&meas = out.meas, &omega = out.omega;
    std::vector<uint16_t>& cam = out.cam;
    out.pose.resize(E), out.lm.resize(E), out.flags.resize(E);
    meas.resize(3 * E); // every slot is written below
    omega.clear(), cam.clear();
    out.n_omega = g.e_omega.size() > 1 ? (int)E : 1;
    out.n_cams = (int)(g.cams.size() / 5);
    const bool per_omega = out.n_omega > 1, per_cam = out.n_cams > 1;
    if (per_omega)
        omega.resize(E);
    else
        omega.assign(1, g.e_omega.empty() ? 1.0 : g.e_omega[0]);
    if (per_cam)
        cam.resize(E);
    out.slot_edge.assign(E, -1);
    out.slot_threshold.clear();
    const bool any_threshold = std::any_of(g.e_outlier_threshold.begin(), g.e_outlier_threshold.end(), [](double t) { return t > 0.0; });
    if (any_threshold)
        out.slot_threshold.assign(E, 0.0);
    // independent per slot: split over a few host threads for big graphs
    parallel_chunks((size_t)E, 100000, [&](size_t ia, size_t ib, unsigned) {
        for (size_t i = ia; i < ib; i++)
        {
            // padding: an inactive edge of the landmark of the nearest real slot before it, everything else zero
            const bool pad = slot_src[i] < 0;
            size_t j = i;
            while (slot_src[j] < 0)
                j--;
            const int e = order[slot_src[j]];
            out.lm[i] = g.e_lm[e];
            out.pose[i] = pad ? 0 : g.e_pose[e];
            out.flags[i] = pad ? (uint8_t)CUGO_EDGE_INACTIVE : g.e_flags[e];
            for (size_t c = 0; c < 3; c++)
                meas[c * E + i] = pad ? 0.0 : g.e_meas[3 * (size_t)e + c];
            if (per_omega)
                omega[i] = pad ? 0.0 : g.e_omega[e];
            if (per_cam)
                cam[i] = pad ? 0 : g.e_cam[e];
            if (pad)
                continue;
            out.slot_edge[i] = e;
            if (any_threshold)
                out.slot_threshold[i] = g.e_outlier_threshold[e];
        }
    });
}

// Stable counting sort.  Threads own slot ranges: a histogram per thread, then offsets per (pose, thread) in thread
// order, so every thread places its own slots and the slot order inside a pose is kept.
void pose_major_view(int Pall, const Idx& slot_pose, const Idx& slot_src, Idx& pose_ptr, Idx& pose_edge)
{
    const size_t E = slot_src.size();
    pose_ptr.assign(Pall + 1, 0);
    pose_edge.assign(std::max<size_t>(E, 1), 0);
    const size_t serial_below = (size_t)Pall * pool_threads() > E ? E + 1 : 100000;
    const int32_t* ep = slot_pose.data();
    const int32_t* src = slot_src.data();
    std::vector<std::vector<int32_t>> hist(pool_threads());
    const unsigned nt = parallel_chunks(E, serial_below, [&](size_t a, size_t b, unsigned t) {
        Idx& h = hist[t];
        h.assign(Pall, 0);
        for (size_t i = a; i < b; i++)
            if (src[i] >= 0)
                h[ep[i]]++;
    });
    // per pose: its total over the threads' histograms (parallel over poses), the prefix sum over poses, then the
    // first output position of every (pose, thread) — thread order inside a pose keeps the slot order
    parallel_chunks((size_t)Pall, 2048, [&](size_t qa, size_t qb, unsigned) {
        for (size_t q = qa; q < qb; q++)
        {
            int32_t c = 0;
            for (unsigned t = 0; t < nt; t++)
                c += hist[t][q];
            pose_ptr[q + 1] = c;
        }
    });
    std::partial_sum(pose_ptr.begin(), pose_ptr.end(), pose_ptr.begin());
    parallel_chunks((size_t)Pall, 2048, [&](size_t qa, size_t qb, unsigned) {
        for (size_t q = qa; q < qb; q++)
        {
            int32_t run = pose_ptr[q];
            for (unsigned t = 0; t < nt; t++)
            {
                const int32_t c = hist[t][q];
                hist[t][q] = run; // first output position of thread t for pose q
                run += c;
            }
        }
    });
    parallel_chunks(E, serial_below, [&](size_t a, size_t b, unsigned t) {
        Idx& pos = hist[t];
        for (size_t i = a; i < b; i++)
            if (src[i] >= 0)
                pose_edge[pos[ep[i]]++] = (int32_t)i;
    });
}

void copy_pose_edges_planar(const FlatPoseKind& fk, const int32_t* slot_of, PoseKindHost& b)
{
    const int n = fk.n(), mw = fk.meas_w, ww = fk.weight_w;
    b.h_pose.resize(n), b.h_pose_b.resize(fk.pose_b.size()), b.slot_set.resize(n), b.slot_edge.resize(n);
    b.h_meas.resize((size_t)mw * n);
    const bool per_edge = fk.weight.size() > (size_t)ww;
    b.n_weight = per_edge ? n : 1;
    b.h_weight.assign((size_t)ww * b.n_weight, 0.0);
    if (!per_edge)
        std::copy(fk.weight.begin(), fk.weight.end(), b.h_weight.begin());
    const bool per_edge_threshold = fk.threshold.size() > 1;
    b.h_threshold = fk.threshold; // (empty or one entry: as it is)
    for (int e = 0; e < n; e++)
    {
        const size_t i = slot_of ? (size_t)slot_of[e] : (size_t)e;
        b.h_pose[i] = fk.pose[e];
        if (!fk.pose_b.empty())
            b.h_pose_b[i] = fk.pose_b[e];
        b.slot_set[i] = fk.src_set[e], b.slot_edge[i] = fk.src_edge[e];
        for (int c = 0; c < mw; c++)
            b.h_meas[(size_t)c * n + i] = fk.meas[(size_t)mw * e + c];
        if (per_edge)
            for (int c = 0; c < ww; c++)
                b.h_weight[(size_t)c * n + i] = fk.weight[(size_t)ww * e + c];
        if (per_edge_threshold)
            b.h_threshold[i] = fk.threshold[e];
    }
}

void sort_pose_edges_by_pose(const FlatPoseKind& fk, int Pall, int P, PoseKindHost& b)
{
    const int n = fk.n();
    b.h_ptr.assign((size_t)Pall + 1, 0);
    for (int e = 0; e < n; e++)
    {
        if (fk.pose[e] < 0 || fk.pose[e] >= P)
            throw std::runtime_error(std::string("cugo: a ") + pose_kind_group(fk.kind) +
                                     (fk.kind == POSE_KIND_PRIOR ? "" : " edge") + " is not on a free pose");
        b.h_ptr[(size_t)fk.pose[e] + 1]++;
    }
    std::partial_sum(b.h_ptr.begin(), b.h_ptr.end(), b.h_ptr.begin());
    std::vector<int32_t> pos(b.h_ptr.begin(), b.h_ptr.end() - 1), slot_of(n);
    for (int e = 0; e < n; e++) // container order inside a pose: the summation order depends on the graph alone
        slot_of[e] = pos[fk.pose[e]]++;
    copy_pose_edges_planar(fk, slot_of.data(), b);
}

void sort_pose_edges_by_pair(const FlatPoseKind& fk, int Pall, int P, PointPairPlanHost& plan, PoseKindHost& b)
{
    const int n = fk.n();
    build_point_pair_plan(n, Pall, P, fk.pose.data(), fk.pose_b.data(), nullptr, nullptr, nullptr, plan);
    std::vector<int32_t> slot_of((size_t)n);
    for (int i = 0; i < n; i++)
        slot_of[(size_t)plan.perm[i]] = i;
    copy_pose_edges_planar(fk, slot_of.data(), b);
}

// ---- the Hsc structure on the host: pose-major co-visibility, pattern (O(M) with a marker array instead of the
// reference's dense P x P byte map, ref: sparse_block_matrix.cpp:80-155), then the off-diagonal product lists
void host_structure(int P, int L, const Idx& cov_ptr, const Idx& cov_pose, const SlotArrays& slots, const Idx& lm_ptr,
                    const Idx& pose_ptr, const Idx& pose_edge, const std::function<bool()>& use_plan,
                    const std::function<void(const char*)>& lap, Idx& rowptr, Idx& colind, HostStructure& out,
                    const Idx* pair_lo, const Idx* pair_hi)
{
    Idx pc_ptr(P + 1, 0), pc_lm(cov_pose.size());
    for (int32_t p : cov_pose)
        pc_ptr[p + 1]++;
    std::partial_sum(pc_ptr.begin(), pc_ptr.end(), pc_ptr.begin());
    {
        Idx pos(pc_ptr.begin(), pc_ptr.end() - 1);
        for (int l = 0; l < L; l++)
            for (int k = cov_ptr[l]; k < cov_ptr[l + 1]; k++)
                pc_lm[pos[cov_pose[k]]++] = l;
    }
    // The passes over the pose rows are independent per row: contiguous row ranges, balanced by
    // their number of co-visibility entries, go to a few host threads (SLAM calls BA with a new
    // topology every time, so this "cold" work is paid on every call there).
    const unsigned nth = cov_pose.size() < 200000 ? 1u : std::max(1u, pool_threads());
    std::vector<int> row_split(nth + 1, P);
    row_split[0] = 0;
    for (unsigned t = 1; t < nth; t++)
    {
        const int32_t target = (int32_t)((int64_t)pc_ptr[P] * t / nth);
        const int at = (int)(std::lower_bound(pc_ptr.begin(), pc_ptr.end(), target) - pc_ptr.begin());
        row_split[t] = std::min(std::max(at, row_split[t - 1]), P);
    }
    auto parallel_rows = [&](auto&& f) { pool_for(nth, [&](unsigned t) { f(t, row_split[t], row_split[t + 1]); }); };
    lap("structure: pose-major covis");
    rowptr.assign(P + 1, 0);
    std::vector<Idx> cols_t(nth);
    std::vector<double> products_t(nth, 0.0);
    parallel_rows([&](unsigned t, int p0, int p1) {
        Idx mark(P, -1);
        Idx& cols = cols_t[t];
        double products = 0;
        for (int p = p0; p < p1; p++)
        {
            const size_t start = cols.size();
            cols.push_back(p);
            mark[p] = p;
            for (int i = pc_ptr[p]; i < pc_ptr[p + 1]; i++)
                for (int k = cov_ptr[pc_lm[i]]; k < cov_ptr[pc_lm[i] + 1]; k++)
                {
                    const int q = cov_pose[k];
                    if (q >= p)
                        products += 1;
                    if (q > p && mark[q] != p)
                    {
                        mark[q] = p;
                        cols.push_back(q);
                    }
                }
            if (pair_lo && !pair_lo->empty()) // the pose pairs of row p (no products)
                for (size_t i = std::lower_bound(pair_lo->begin(), pair_lo->end(), p) - pair_lo->begin();
                     i < pair_lo->size() && (*pair_lo)[i] == p; i++)
                {
                    const int q = (*pair_hi)[i];
                    if (mark[q] != p)
                    {
                        mark[q] = p;
                        cols.push_back(q);
                    }
                }
            std::sort(cols.begin() + start + 1, cols.end());
            rowptr[p + 1] = (int32_t)(cols.size() - start); // row length; prefix sum below
        }
        products_t[t] = products;
    });
    out.products = 0;
    colind.clear();
    for (unsigned t = 0; t < nth; t++)
    {
        out.products += products_t[t];
        colind.insert(colind.end(), cols_t[t].begin(), cols_t[t].end());
    }
    std::partial_sum(rowptr.begin(), rowptr.end(), rowptr.begin());
    lap("structure: Hsc pattern");
    Idx& off_ptr = out.off_ptr;
    off_ptr.assign(colind.size() + 1, 0);
    out.off_ei.clear(), out.off_ej.clear();
    if (use_plan())
        return;
    // Built row by row (pose-major): pos[q] gives the block of column q in the current row, so every product is
    // placed with O(1) work.  A row only touches the counters / entries of its own blocks: rows are independent.
    // per_product(block, a, b) for every pair of free-free slots a < b of one landmark, a on a pose of the range
    auto walk = [&](auto&& per_product) {
        parallel_rows([&](unsigned, int p0, int p1) {
            Idx pos(P, -1);
            for (int p = p0; p < p1; p++)
            {
                for (int k = rowptr[p]; k < rowptr[p + 1]; k++)
                    pos[colind[k]] = k;
                for (int i = pose_ptr[p]; i < pose_ptr[p + 1]; i++)
                {
                    const int a = pose_edge[i];
                    if (!is_free_free(slots.flags[a]))
                        continue;
                    const int e1 = lm_ptr[slots.lm[a] + 1];
                    for (int b = a + 1; b < e1; b++)
                        if (is_free_free(slots.flags[b]))
                            per_product(pos[slots.pose[b]], a, b);
                }
            }
        });
    };
    walk([&](int blk, int, int) { off_ptr[blk + 1]++; });
    std::partial_sum(off_ptr.begin(), off_ptr.end(), off_ptr.begin());
    out.off_ei.resize((size_t)off_ptr.back()), out.off_ej.resize((size_t)off_ptr.back());
    Idx fill(off_ptr.begin(), off_ptr.end() - 1);
    walk([&](int blk, int a, int b) {
        const int q = fill[blk]++;
        out.off_ei[q] = a, out.off_ej[q] = b;
    });
}

} // namespace cugo_host
