// extern "C" surface of libcugo_hip.so (declared in include/cugo_hip.h).
#include <cmath>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <unordered_map>

#include "../../../include/cugo_hip.h"
#include "../../include/cuda_graph_optimisation.h"
#include "../../include/icp_types.h"
#include "../../include/landmark_prior_types.h"
#include "../../include/point_edge_types.h"
#include "../../include/gicp_types.h"
#include "../../include/point_pair_types.h"
#include "../../include/prior_types.h"
#include "../../include/relpose_types.h"
#include "../kernels/kernels.h"
#include "chol_solver.h"
#include "edge_layout.h"
#include "engine.h"
#include "hip_util.h"
#include "rccl_comm.h"
#include "plcov_plan.h"
#include "point_pair_plan.h"
#include "relpose_plan.h"
#include "schur_plan.h"

using namespace cugo_host;

namespace
{
template <typename F>
int guarded(F&& f)
{
    try
    {
        f();
        return CUGO_OK;
    }
    catch (const HipError& e)
    {
        set_last_error(e.what());
        return e.code == hipErrorNoDevice ? CUGO_ERR_NO_DEVICE : CUGO_ERR_HIP;
    }
    catch (const std::exception& e)
    {
        set_last_error(e.what());
        const char* w = e.what();
        return std::strstr(w, "no HIP device") ? CUGO_ERR_NO_DEVICE : CUGO_ERR_INVALID;
    }
}

cugo_k::ReduceScratch scratch_for(cugo_ctx* ctx, const cugo_edges* ev)
{
    const size_t need = cugo_k::reduce_scratch_doubles(ev ? ev->n_edges : 0, ev ? ev->n_poses_free : 0,
                                                       ev ? ev->n_landmarks_free : 0);
    if (ctx->scratch.size() < need)
    {
        CUGO_HIP(hipStreamSynchronize(ctx->stream));
        ctx->scratch.resize(need);
    }
    return {ctx->scratch.data(), ctx->scratch.size()};
}

} // namespace

namespace cugo_host
{
// The members of an edge view that go with its form (cugo_k::edge_form) are checked before anything is launched: with a
// table (Rig, Models, Distortion) d_cam_ext must be there, and the kernels that read one hold no depth code yet; with depth slots the
// kernels take sqrt(depth_weight) and the depth kind's robust kernel.  Nothing of either is read otherwise.
// (not in the unnamed namespace: tests/test_edge_form_host.py links against it)
void check_edge_form(const cugo_edges* ev, const char* who)
{
    if (!ev)
        return;
    const cugo_k::EdgeForm form = cugo_k::edge_form(*ev);
    if (form == cugo_k::EdgeForm::Rig || form == cugo_k::EdgeForm::Models || form == cugo_k::EdgeForm::Distortion)
    {
        if (!ev->d_cam_ext)
            throw std::runtime_error(std::string(who) + ": has_rig needs the extrinsics table d_cam_ext");
        if (ev->has_depth)
            throw std::runtime_error(std::string(who) + ": camera extrinsics (has_rig) together with depth slots "
                                                        "(has_depth) are not supported yet");
    }
    if (!ev->has_depth)
        return;
    if (!(ev->depth_weight > 0.0) || !std::isfinite(ev->depth_weight))
        throw std::runtime_error(std::string(who) + ": depth_weight must be finite and > 0 with has_depth");
    const int rk = ev->rk_type_depth;
    if (rk < CUGO_RK_NONE || rk > CUGO_RK_HUBER ||
        (rk != CUGO_RK_NONE && !(ev->rk_delta_depth > 0.0 && std::isfinite(ev->rk_delta_depth))))
        throw std::runtime_error(std::string(who) + ": unknown robust kernel or bad delta of the depth kind");
}
} // namespace cugo_host

extern "C" {

const char* cugo_last_error(void) { return get_last_error(); }

int cugo_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

int cugo_ctx_create(int device, cugo_ctx** out)
{
    return guarded([&] {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
            throw std::runtime_error("cugo: no HIP device available (there is no CPU fallback)");
        if (device >= 0)
            CUGO_HIP(hipSetDevice(device));
        auto* c = new cugo_ctx;
        CUGO_HIP(hipGetDevice(&c->device));
        CUGO_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        *out = c;
    });
}

void cugo_ctx_destroy(cugo_ctx* ctx)
{
    if (!ctx)
        return;
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int cugo_ctx_sync(cugo_ctx* ctx)
{
    return guarded([&] { CUGO_HIP(hipStreamSynchronize(ctx->stream)); });
}
void* cugo_ctx_stream(cugo_ctx* ctx) { return ctx->stream; }

int cugo_malloc(void** p, size_t bytes)
{
    return guarded([&] { CUGO_HIP(hipMalloc(p, bytes ? bytes : 16)); });
}
int cugo_free(void* p)
{
    return guarded([&] { CUGO_HIP(hipFree(p)); });
}
int cugo_memcpy_h2d(cugo_ctx* ctx, void* d, const void* h, size_t bytes)
{
    return guarded([&] {
        CUGO_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, ctx->stream));
        CUGO_HIP(hipStreamSynchronize(ctx->stream));
    });
}
int cugo_memcpy_d2h(cugo_ctx* ctx, void* h, const void* d, size_t bytes)
{
    return guarded([&] {
        CUGO_HIP(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, ctx->stream));
        CUGO_HIP(hipStreamSynchronize(ctx->stream));
    });
}
int cugo_memset(cugo_ctx* ctx, void* d, int value, size_t bytes)
{
    return guarded([&] { CUGO_HIP(hipMemsetAsync(d, value, bytes, ctx->stream)); });
}

// ---------------------------------------------------------------- kernel level ---------
int cugo_compute_active_errors(cugo_ctx* ctx, const cugo_edges* ev, const double* d_poses,
                               const double* d_lms, cugo_robust rk, double* d_chi)
{
    return guarded([&] {
        check_edge_form(ev, "cugo_compute_active_errors");
        cugo_k::launch_errors(ctx->stream, *ev, d_poses, d_lms, rk, scratch_for(ctx, ev), d_chi);
        CUGO_HIP(hipGetLastError());
    });
}

int cugo_compute_edge_chi(cugo_ctx* ctx, const cugo_edges* ev, const double* d_poses, const double* d_lms,
                          cugo_robust rk, double* d_edge_chi)
{
    return guarded([&] {
        if (!ctx || !ev || !d_edge_chi)
            throw std::runtime_error("cugo_compute_edge_chi: null argument");
        check_edge_form(ev, "cugo_compute_edge_chi");
        cugo_k::launch_edge_chi(ctx->stream, *ev, d_poses, d_lms, rk, d_edge_chi);
        CUGO_HIP(hipGetLastError());
    });
}

int cugo_construct_quadratic_form(cugo_ctx* ctx, const cugo_edges* ev, const double* d_poses,
                                  const double* d_lms, cugo_robust rk, double* d_Hpp, double* d_bp,
                                  double* d_Hll, double* d_bl, void* d_Hpl, double* d_chi)
{
    return guarded([&] {
        check_edge_form(ev, "cugo_construct_quadratic_form");
        cugo_k::launch_build(ctx->stream, *ev, d_poses, d_lms, rk, d_Hpp, d_bp, d_Hll, d_bl, d_Hpl,
                             scratch_for(ctx, ev), d_chi);
        CUGO_HIP(hipGetLastError());
    });
}

} // extern "C"

namespace
{
// The pose edge kernels read pose_ptr and index by it (the ICP kernels their partials by chunk + pose): before anything
// is launched, pose_ptr (P + 1 entries) is checked on the host and the pose index of every edge against it on the
// device (check_pose_indices: one flag comes back), so that a bad layout is refused instead of addressing memory out
// of range.  label: " (plane)" / " (line)" behind the ICP messages; arrays_missing: what the kind needs with n > 0
void check_pose_kind(cugo_ctx* ctx, const char* prefix, const std::string& label, int n, int P, const int32_t* d_pose,
                     const int32_t* d_ptr, int rk, double delta, bool arrays_missing)
{
    auto refuse = [&](const char* what) { throw std::runtime_error(std::string(prefix) + ": " + what + label); };
    if (!d_ptr)
        refuse("no pose_ptr");
    if (rk < CUGO_RK_NONE || rk > CUGO_RK_HUBER || (rk != CUGO_RK_NONE && !(delta > 0.0 && std::isfinite(delta))))
        refuse("unknown robust kernel or bad delta");
    if (n > 0 && (!d_pose || arrays_missing))
        refuse("missing arrays");
    std::vector<int32_t> ptr(P + 1);
    CUGO_HIP(hipMemcpyAsync(ptr.data(), d_ptr, sizeof(int32_t) * (P + 1), hipMemcpyDeviceToHost, ctx->stream));
    CUGO_HIP(hipStreamSynchronize(ctx->stream));
    if (ptr[0] != 0 || ptr[P] != n)
        refuse("pose_ptr does not span the edges");
    for (int p = 0; p < P; p++)
        if (ptr[p + 1] < ptr[p])
            refuse("pose_ptr not ascending");
}

// the context's scratch with room for what a kind's launchers need + 16 doubles of slack for the flag of the index check
cugo_k::ReduceScratch pose_scratch_for(cugo_ctx* ctx, size_t need)
{
    if (ctx->scratch.size() < need + 16)
    {
        CUGO_HIP(hipStreamSynchronize(ctx->stream));
        ctx->scratch.resize(need + 16);
    }
    return {ctx->scratch.data(), ctx->scratch.size()};
}

void check_pose_indices(cugo_ctx* ctx, const char* prefix, const char* who, std::initializer_list<cugo_k::PoseIndexCheck> kinds,
                        int P, cugo_k::ReduceScratch rs, size_t need)
{
    if (cugo_k::pose_check_indices(ctx->stream, who, kinds.begin(), (int)kinds.size(), P, reinterpret_cast<int*>(rs.d_partials + need)))
        throw std::runtime_error(std::string(prefix) + ": edges not sorted by pose, or a pose index disagrees with pose_ptr");
}

cugo_k::ChunkScratch check_icp(cugo_ctx* ctx, const cugo_icp_edges* ev)
{
    if (!ev || ev->n_poses_total < 0 || ev->n_poses_free < 0 || ev->n_poses_free > ev->n_poses_total ||
        ev->n_plane < 0 || ev->n_line < 0)
        throw std::runtime_error("cugo_icp: bad pose or edge counts");
    const int P = ev->n_poses_total;
    const size_t need = cugo_k::icp_scratch_doubles(*ev);
    const cugo_k::ReduceScratch rs = pose_scratch_for(ctx, need);
    check_pose_kind(ctx, "cugo_icp", " (plane)", ev->n_plane, P, ev->d_plane_pose, ev->d_plane_pose_ptr, ev->rk_plane,
                    ev->delta_plane,
                    !ev->d_plane_p || !ev->d_plane_nd || !ev->d_plane_omega ||
                        (ev->n_plane_omega != 1 && ev->n_plane_omega != ev->n_plane));
    check_pose_kind(ctx, "cugo_icp", " (line)", ev->n_line, P, ev->d_line_pose, ev->d_line_pose_ptr, ev->rk_line,
                    ev->delta_line,
                    !ev->d_line_p || !ev->d_line_au || !ev->d_line_omega ||
                        (ev->n_line_omega != 1 && ev->n_line_omega != ev->n_line));
    check_pose_indices(ctx, "cugo_icp", "ICP",
                       {{ev->d_plane_pose, ev->d_plane_pose_ptr, ev->n_plane, "k_icp_check"},
                        {ev->d_line_pose, ev->d_line_pose_ptr, ev->n_line, "k_icp_check"}},
                       P, rs, need);
    return cugo_k::icp_scratch_in(rs, *ev);
}
} // namespace

extern "C" {

int cugo_icp_compute_errors(cugo_ctx* ctx, const cugo_icp_edges* ev, const double* d_poses, double* d_chi,
                            double* d_edge_chi)
{
    return guarded([&] {
        const cugo_k::ChunkScratch rs = check_icp(ctx, ev);
        cugo_k::launch_icp_errors(ctx->stream, *ev, d_poses, rs, d_chi, false, d_edge_chi);
        CUGO_HIP(hipGetLastError());
    });
}

int cugo_icp_construct_quadratic_form(cugo_ctx* ctx, const cugo_icp_edges* ev, const double* d_poses, double* d_Hpp,
                                      double* d_bp, double* d_chi)
{
    return guarded([&] {
        const cugo_k::ChunkScratch rs = check_icp(ctx, ev);
        cugo_k::launch_icp_build(ctx->stream, *ev, d_poses, d_Hpp, d_bp, rs, d_chi, false);
        CUGO_HIP(hipGetLastError());
    });
}

int cugo_icp_construct_quadratic_form_schur(cugo_ctx* ctx, const cugo_icp_edges* ev, const double* d_poses,
                                            const int32_t* d_rowptr, double* d_Hsc, double* d_bp, double* d_bsc, double* d_chi)
{
    return guarded([&] {
        const cugo_k::ChunkScratch rs = check_icp(ctx, ev);
        if (!d_rowptr || !d_Hsc || !d_bp || !d_bsc)
            throw std::runtime_error("cugo_icp: missing rowptr, Hsc, bp or bsc");
        // (what the one-stream form of the LM loop queues: the chunk pass, the per-pose sums into the Schur destination,
        //  the sum of the chunk totals)
        cugo_k::launch_icp_chunks(ctx->stream, *ev, d_poses, true, rs);
        cugo_k::launch_icp_add_schur(ctx->stream, *ev, rs, d_rowptr, d_Hsc, d_bp, d_bsc);
        if (d_chi)
            cugo_k::launch_icp_chi_total(ctx->stream, *ev, rs, d_chi, false);
        CUGO_HIP(hipGetLastError());
    });
}

} // extern "C"

namespace
{
// as check_icp, for the one kind of the point edges.  Both forms come here as a cugo_point_edges view: the covariance
// form (cugo_gicp_edges) with d_info = cov_p, n_info = n_cov and its cov_z beside it (PointView)
struct PointView
{
    cugo_point_edges ev;
    const double* d_cov_z; // nullptr: the information form
    bool cov;
    const char* who;
};
const cugo_point_edges NO_POINT_EDGES = {-1, -1, -1, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, 0.0}; // (refused)
PointView view_of(const cugo_point_edges* ev) { return {ev ? *ev : NO_POINT_EDGES, nullptr, false, "cugo_point"}; }
PointView view_of(const cugo_gicp_edges* g)
{
    if (!g)
        return {NO_POINT_EDGES, nullptr, true, "cugo_gicp"};
    return {{g->n_poses_total, g->n_poses_free, g->n, g->d_pose, g->d_pose_ptr, g->d_p, g->d_z, g->d_cov_p, g->n_cov, g->d_flags,
             g->rk, g->delta},
            g->d_cov_z, true, "cugo_gicp"};
}
cugo_k::ChunkScratch check_point(cugo_ctx* ctx, const PointView& v)
{
    const cugo_point_edges* ev = &v.ev;
    if (ev->n_poses_total < 0 || ev->n_poses_free < 0 || ev->n_poses_free > ev->n_poses_total || ev->n < 0)
        throw std::runtime_error(std::string(v.who) + ": bad pose or edge counts");
    const size_t need = cugo_k::point_scratch_doubles(*ev);
    const cugo_k::ReduceScratch rs = pose_scratch_for(ctx, need);
    check_pose_kind(ctx, v.who, "", ev->n, ev->n_poses_total, ev->d_pose, ev->d_pose_ptr, ev->rk, ev->delta,
                    !ev->d_p || !ev->d_z || !ev->d_info || (v.cov && !v.d_cov_z) || (ev->n_info != 1 && ev->n_info != ev->n));
    check_pose_indices(ctx, v.who, "point", {{ev->d_pose, ev->d_pose_ptr, ev->n, "k_point_check"}}, ev->n_poses_total, rs, need);
    return cugo_k::point_scratch_in(rs, *ev);
}
int point_errors(cugo_ctx* ctx, const PointView& v, const double* d_poses, double* d_chi, double* d_edge_chi)
{
    return guarded([&] {
        const cugo_k::ChunkScratch rs = check_point(ctx, v);
        cugo_k::launch_point_errors(ctx->stream, v.ev, d_poses, rs, d_chi, false, d_edge_chi, v.d_cov_z);
        CUGO_HIP(hipGetLastError());
    });
}
int point_form(cugo_ctx* ctx, const PointView& v, const double* d_poses, double* d_Hpp, double* d_bp,
               double* d_chi)
{
    return guarded([&] {
        const cugo_k::ChunkScratch rs = check_point(ctx, v);
        cugo_k::launch_point_build(ctx->stream, v.ev, d_poses, d_Hpp, d_bp, rs, d_chi, false, v.d_cov_z);
        CUGO_HIP(hipGetLastError());
    });
}
int point_form_schur(cugo_ctx* ctx, const PointView& v, const double* d_poses, const int32_t* d_rowptr,
                     double* d_Hsc, double* d_bp, double* d_bsc, double* d_chi)
{
    return guarded([&] {
        const cugo_k::ChunkScratch rs = check_point(ctx, v);
        if (!d_rowptr || !d_Hsc || !d_bp || !d_bsc)
            throw std::runtime_error(std::string(v.who) + ": missing rowptr, Hsc, bp or bsc");
        cugo_k::launch_point_chunks(ctx->stream, v.ev, d_poses, true, rs, nullptr, v.d_cov_z);
        cugo_k::launch_point_add_schur(ctx->stream, v.ev, rs, d_rowptr, d_Hsc, d_bp, d_bsc);
        if (d_chi)
            cugo_k::launch_point_chi_total(ctx->stream, v.ev, rs, d_chi, false);
        CUGO_HIP(hipGetLastError());
    });
}
} // namespace

extern "C" {

int cugo_point_compute_errors(cugo_ctx* ctx, const cugo_point_edges* ev, const double* d_poses, double* d_chi,
                              double* d_edge_chi)
{
    return point_errors(ctx, view_of(ev), d_poses, d_chi, d_edge_chi);
}
int cugo_point_construct_quadratic_form(cugo_ctx* ctx, const cugo_point_edges* ev, const double* d_poses, double* d_Hpp,
                                        double* d_bp, double* d_chi)
{
    return point_form(ctx, view_of(ev), d_poses, d_Hpp, d_bp, d_chi);
}
int cugo_point_construct_quadratic_form_schur(cugo_ctx* ctx, const cugo_point_edges* ev, const double* d_poses,
                                              const int32_t* d_rowptr, double* d_Hsc, double* d_bp, double* d_bsc, double* d_chi)
{
    return point_form_schur(ctx, view_of(ev), d_poses, d_rowptr, d_Hsc, d_bp, d_bsc, d_chi);
}

int cugo_gicp_compute_errors(cugo_ctx* ctx, const cugo_gicp_edges* ev, const double* d_poses, double* d_chi, double* d_edge_chi)
{
    return point_errors(ctx, view_of(ev), d_poses, d_chi, d_edge_chi);
}
int cugo_gicp_construct_quadratic_form(cugo_ctx* ctx, const cugo_gicp_edges* ev, const double* d_poses, double* d_Hpp,
                                       double* d_bp, double* d_chi)
{
    return point_form(ctx, view_of(ev), d_poses, d_Hpp, d_bp, d_chi);
}
int cugo_gicp_construct_quadratic_form_schur(cugo_ctx* ctx, const cugo_gicp_edges* ev, const double* d_poses,
                                             const int32_t* d_rowptr, double* d_Hsc, double* d_bp, double* d_bsc, double* d_chi)
{
    return point_form_schur(ctx, view_of(ev), d_poses, d_rowptr, d_Hsc, d_bp, d_bsc, d_chi);
}

} // extern "C"

namespace
{
// what the two SE(3) kinds check alike: the edge count against the kernels' 32-bit indices, the robust kernel, the arrays
template <class Edges>
void check_se3_edges(const char* prefix, const Edges* ev)
{
    auto refuse = [&](const char* what) { throw std::runtime_error(std::string(prefix) + ": " + what); };
    if (ev->n > (1 << 26))
        refuse("more than 2^26 edges (the kernel indexes the planar arrays with 32 bits)");
    if (ev->rk < CUGO_RK_NONE || ev->rk > CUGO_RK_HUBER ||
        (ev->rk != CUGO_RK_NONE && !(ev->delta > 0.0 && std::isfinite(ev->delta))))
        refuse("unknown robust kernel or bad delta");
    if (ev->n > 0 && (!ev->d_meas || !ev->d_info || (ev->n_info != 1 && ev->n_info != ev->n)))
        refuse("missing arrays");
}
// as check_icp: pose_ptr on the host, the pose index of every edge against it on the device, before anything is launched
cugo_k::ReduceScratch check_prior(cugo_ctx* ctx, const cugo_prior_edges* ev)
{
    if (!ev || ev->n_poses_total < 0 || ev->n_poses_free < 0 || ev->n_poses_free > ev->n_poses_total || ev->n < 0)
        throw std::runtime_error("cugo_prior: bad pose or edge counts");
    if (!ev->d_pose_ptr) // (check_pose_kind's first refusal comes before those of the shared check)
        throw std::runtime_error("cugo_prior: no pose_ptr");
    check_se3_edges("cugo_prior", ev);
    check_pose_kind(ctx, "cugo_prior", "", ev->n, ev->n_poses_total, ev->d_pose, ev->d_pose_ptr, ev->rk, ev->delta, false);
    const size_t need = (size_t)cugo_k::prior_workgroups(*ev);
    const cugo_k::ReduceScratch rs = pose_scratch_for(ctx, need);
    check_pose_indices(ctx, "cugo_prior", "prior", {{ev->d_pose, ev->d_pose_ptr, ev->n, "k_prior_check"}}, ev->n_poses_total,
                       rs, need);
    return rs;
}
} // namespace

extern "C" {

int cugo_prior_compute_errors(cugo_ctx* ctx, const cugo_prior_edges* ev, const double* d_poses, double* d_chi,
                              double* d_edge_chi)
{
    return guarded([&] {
        const cugo_k::ReduceScratch rs = check_prior(ctx, ev);
        if (d_edge_chi && ev->n > 0 && ev->n_poses_free < ev->n_poses_total) // (the kernel never visits a fixed pose)
            CUGO_HIP(hipMemsetAsync(d_edge_chi, 0, sizeof(double) * ev->n, ctx->stream));
        cugo_k::launch_prior_errors(ctx->stream, *ev, d_poses, rs.d_partials, d_edge_chi);
        if (d_chi)
            cugo_k::launch_pose_chi_total(ctx->stream, "k_prior_chi_total", rs.d_partials, cugo_k::prior_workgroups(*ev), d_chi, false);
        CUGO_HIP(hipGetLastError());
    });
}

int cugo_prior_construct_quadratic_form(cugo_ctx* ctx, const cugo_prior_edges* ev, const double* d_poses, double* d_Hpp,
                                        double* d_bp, double* d_chi)
{
    return guarded([&] {
        const cugo_k::ReduceScratch rs = check_prior(ctx, ev);
        cugo_k::launch_prior_add(ctx->stream, *ev, d_poses, d_Hpp, d_bp, rs.d_partials);
        if (d_chi)
            cugo_k::launch_pose_chi_total(ctx->stream, "k_prior_chi_total", rs.d_partials, cugo_k::prior_workgroups(*ev), d_chi, false);
        CUGO_HIP(hipGetLastError());
    });
}

int cugo_prior_construct_quadratic_form_schur(cugo_ctx* ctx, const cugo_prior_edges* ev, const double* d_poses,
                                              const int32_t* d_rowptr, double* d_Hsc, double* d_bp, double* d_bsc, double* d_chi)
{
    return guarded([&] {
        const cugo_k::ReduceScratch rs = check_prior(ctx, ev);
        if (!d_rowptr || !d_Hsc || !d_bp || !d_bsc)
            throw std::runtime_error("cugo_prior: missing rowptr, Hsc, bp or bsc");
        cugo_k::launch_prior_add_schur(ctx->stream, *ev, d_poses, d_rowptr, d_Hsc, d_bp, d_bsc, rs.d_partials);
        if (d_chi)
            cugo_k::launch_pose_chi_total(ctx->stream, "k_prior_chi_total", rs.d_partials, cugo_k::prior_workgroups(*ev), d_chi, false);
        CUGO_HIP(hipGetLastError());
    });
}

} // extern "C"

namespace
{
// Landmark position priors: as check_prior, with lm_ptr (n_landmarks_total + 1 entries) on the host and the landmark
// index of every prior against it on the device.  `before`: doubles of the scratch in front of the workgroup totals
// (what a BA build pass of the same call needs); the totals start there
double* check_lm_prior(cugo_ctx* ctx, const cugo_lm_prior_edges* ev, size_t before = 0)
{
    const char* prefix = "cugo_lm_prior";
    auto refuse = [&](const char* what) { throw std::runtime_error(std::string(prefix) + ": " + what); };
    if (!ctx || !ev || ev->n_landmarks_total < 0 || ev->n_landmarks_free < 0 || ev->n_landmarks_free > ev->n_landmarks_total ||
        ev->n < 0)
        refuse("bad landmark or edge counts");
    if (!ev->d_lm_ptr)
        refuse("no lm_ptr");
    if (ev->n > (1 << 26))
        refuse("more than 2^26 edges (the kernel indexes the planar arrays with 32 bits)");
    if (ev->rk < CUGO_RK_NONE || ev->rk > CUGO_RK_HUBER || (ev->rk != CUGO_RK_NONE && !(ev->delta > 0.0 && std::isfinite(ev->delta))))
        refuse("unknown robust kernel or bad delta");
    if (ev->n > 0 && (!ev->d_lm || !ev->d_meas || !ev->d_info || (ev->n_info != 1 && ev->n_info != ev->n)))
        refuse("missing arrays");
    const int L = ev->n_landmarks_total;
    std::vector<int32_t> ptr((size_t)L + 1);
    CUGO_HIP(hipMemcpyAsync(ptr.data(), ev->d_lm_ptr, sizeof(int32_t) * ((size_t)L + 1), hipMemcpyDeviceToHost, ctx->stream));
    CUGO_HIP(hipStreamSynchronize(ctx->stream));
    if (ptr[0] != 0 || ptr[L] != ev->n)
        refuse("lm_ptr does not span the edges");
    for (int l = 0; l < L; l++)
        if (ptr[l + 1] < ptr[l])
            refuse("lm_ptr not ascending");
    const size_t need = before + (size_t)cugo_k::lm_prior_workgroups(*ev);
    const cugo_k::ReduceScratch rs = pose_scratch_for(ctx, need);
    const cugo_k::PoseIndexCheck kind{ev->d_lm, ev->d_lm_ptr, ev->n, "k_lm_prior_check"};
    if (cugo_k::pose_check_indices(ctx->stream, "landmark prior", &kind, 1, L, reinterpret_cast<int*>(rs.d_partials + need)))
        refuse("edges not sorted by landmark, or a landmark index disagrees with lm_ptr");
    return rs.d_partials + before;
}
} // namespace

extern "C" {

int cugo_lm_prior_compute_errors(cugo_ctx* ctx, const cugo_lm_prior_edges* ev, const double* d_lms, double* d_chi,
                                 double* d_edge_chi)
{
    return guarded([&] {
        double* d_wg = check_lm_prior(ctx, ev);
        if (d_edge_chi && ev->n > 0 && ev->n_landmarks_free < ev->n_landmarks_total) // (the kernel never visits a fixed landmark)
            CUGO_HIP(hipMemsetAsync(d_edge_chi, 0, sizeof(double) * ev->n, ctx->stream));
        cugo_k::launch_lm_prior_errors(ctx->stream, *ev, d_lms, d_wg, d_edge_chi);
        if (d_chi)
            cugo_k::launch_pose_chi_total(ctx->stream, "k_lm_prior_chi_total", d_wg, cugo_k::lm_prior_workgroups(*ev), d_chi, false);
        CUGO_HIP(hipGetLastError());
    });
}

int cugo_lm_prior_construct_quadratic_form(cugo_ctx* ctx, const cugo_lm_prior_edges* ev, const double* d_lms, double* d_Hll,
                                           double* d_bl, double* d_chi)
{
    return guarded([&] {
        double* d_wg = check_lm_prior(ctx, ev);
        if (ev->n > 0 && ev->n_landmarks_free > 0 && (!d_Hll || !d_bl))
            throw std::runtime_error("cugo_lm_prior: missing Hll or bl");
        cugo_k::launch_lm_prior_add(ctx->stream, *ev, d_lms, d_Hll, d_bl, d_wg);
        if (d_chi)
            cugo_k::launch_pose_chi_total(ctx->stream, "k_lm_prior_chi_total", d_wg, cugo_k::lm_prior_workgroups(*ev), d_chi, false);
        CUGO_HIP(hipGetLastError());
    });
}

int cugo_construct_quadratic_form_lm_priors(cugo_ctx* ctx, const cugo_edges* ev, const cugo_lm_prior_edges* lp,
                                            const double* d_poses, const double* d_lms, cugo_robust rk, double* d_Hpp,
                                            double* d_bp, double* d_Hll, double* d_bl, void* d_Hpl, double* d_chi)
{
    return guarded([&] {
        if (!ev || !lp)
            throw std::runtime_error("cugo_lm_prior: no edges or no priors");
        if (lp->n_landmarks_total != ev->n_landmarks_total || lp->n_landmarks_free != ev->n_landmarks_free)
            throw std::runtime_error("cugo_lm_prior: the priors do not describe the landmarks of the edges");
        check_edge_form(ev, "cugo_construct_quadratic_form_lm_priors");
        // (the scratch of the BA pass in front, the priors' workgroup totals and the flag of the index check behind it)
        const size_t ba = cugo_k::reduce_scratch_doubles(ev->n_edges, ev->n_poses_free, ev->n_landmarks_free);
        double* d_wg = check_lm_prior(ctx, lp, ba);
        cugo_k::launch_build(ctx->stream, *ev, d_poses, d_lms, rk, d_Hpp, d_bp, d_Hll, d_bl, d_Hpl,
                             cugo_k::ReduceScratch{ctx->scratch.data(), ctx->scratch.size()}, d_chi, -1.0, nullptr, nullptr,
                             nullptr, false, false, lp);
        if (d_chi)
        {
            cugo_k::launch_lm_prior_errors(ctx->stream, *lp, d_lms, d_wg);
            cugo_k::launch_pose_chi_total(ctx->stream, "k_lm_prior_chi_total", d_wg, cugo_k::lm_prior_workgroups(*lp), d_chi, true);
        }
        CUGO_HIP(hipGetLastError());
    });
}

int cugo_pose_edges_reject(cugo_ctx* ctx, int n, const double* d_edge_chi, const double* d_threshold, int n_threshold,
                           uint8_t* d_flags, int32_t* d_rejected, int* n_rejected)
{
    return guarded([&] {
        if (!ctx || !n_rejected || n < 0)
            throw std::runtime_error("cugo_pose_edges_reject: no context, no count or a negative edge count");
        *n_rejected = 0;
        if (n == 0)
            return;
        if (n > (1 << 26))
            throw std::runtime_error("cugo_pose_edges_reject: more than 2^26 edges");
        if (!d_edge_chi || !d_threshold || !d_flags || !d_rejected)
            throw std::runtime_error("cugo_pose_edges_reject: missing arrays");
        if (n_threshold != 1 && n_threshold != n)
            throw std::runtime_error("cugo_pose_edges_reject: n_threshold must be 1 or n");
        // (the counts of the workgroups live in the context's scratch, as ints)
        const cugo_k::ReduceScratch rs = pose_scratch_for(ctx, (cugo_k::pose_reject_work_ints(n) + 1) / 2);
        const int32_t* d_count = cugo_k::launch_pose_reject(ctx->stream, n, d_edge_chi, d_threshold, n_threshold == n && n > 1,
                                                            d_flags, d_rejected, reinterpret_cast<int32_t*>(rs.d_partials));
        CUGO_HIP(hipGetLastError());
        int32_t count = 0;
        CUGO_HIP(hipMemcpyAsync(&count, d_count, sizeof count, hipMemcpyDeviceToHost, ctx->stream));
        CUGO_HIP(hipStreamSynchronize(ctx->stream));
        *n_rejected = count;
    });
}

} // extern "C"

// the plan of a set of relative-pose edges: the host plan (relpose_plan.h) and, with a context, its copy on the device
struct cugo_relpose_plan
{
    cugo_host::RelPosePlanHost host;
    bool on_device = false;
    cugo_host::DevBuf<int32_t> pose_a, pose_b, inc_ptr, inc, off_blk;
    cugo_k::RelPosePlanDev dev() const
    {
        return {host.n, host.n_poses_free, pose_a.data(), pose_b.data(), inc_ptr.data(), inc.data(), off_blk.data()};
    }
};

// the plan of a batch of pose-landmark covariance queries (plcov_plan.h): host arrays only, the caller uploads them
struct cugo_plcov_plan
{
    cugo_host::PlCovPlanHost host;
};

namespace
{
// the layout is the plan's own, so nothing is checked on the device: counts against the plan, arrays, kernel code
cugo_k::ReduceScratch check_relpose(cugo_ctx* ctx, const cugo_relpose_edges* ev)
{
    if (!ev || !ev->plan)
        throw std::runtime_error("cugo_relpose: no edges or no plan (cugo_relpose_plan_create)");
    const cugo_host::RelPosePlanHost& h = ev->plan->host;
    if (ev->n != h.n || ev->n_poses_total != h.n_poses_total || ev->n_poses_free != h.n_poses_free)
        throw std::runtime_error("cugo_relpose: the pose or edge counts are not those of the plan");
    if (!ev->plan->on_device)
        throw std::runtime_error("cugo_relpose: the plan is host-only (created without a context)");
    check_se3_edges("cugo_relpose", ev);
    return pose_scratch_for(ctx, (size_t)cugo_k::relpose_workgroups(*ev));
}
void relpose_chi_total(cugo_ctx* ctx, const cugo_relpose_edges* ev, const cugo_k::ReduceScratch& rs, double* d_chi)
{
    if (!d_chi)
        return;
    const int wgs = cugo_k::relpose_workgroups(*ev);
    if (wgs)
        cugo_k::launch_pose_chi_total(ctx->stream, "k_relpose_chi_total", rs.d_partials, wgs, d_chi, false);
    else
        CUGO_HIP(hipMemsetAsync(d_chi, 0, sizeof(double), ctx->stream));
}
} // namespace

extern "C" {

int cugo_relpose_plan_create(cugo_ctx* ctx, int n, int n_poses_total, int n_poses_free, const int32_t* h_pose_a,
                             const int32_t* h_pose_b, const uint8_t* h_flags, const int32_t* h_rowptr,
                             const int32_t* h_colind, cugo_relpose_plan** out)
{
    return guarded([&] {
        if (!out)
            throw std::runtime_error("cugo_relpose_plan_create: null argument");
        *out = nullptr;
        if (n > (1 << 26))
            throw std::runtime_error("cugo_relpose_plan_create: more than 2^26 edges");
        auto p = std::make_unique<cugo_relpose_plan>();
        cugo_host::build_relpose_plan(n, n_poses_total, n_poses_free, h_pose_a, h_pose_b, h_flags, h_rowptr, h_colind, p->host);
        if (ctx)
        {
            p->pose_a.upload(h_pose_a, (size_t)n, ctx->stream);
            p->pose_b.upload(h_pose_b, (size_t)n, ctx->stream);
            p->inc_ptr.upload(p->host.inc_ptr, ctx->stream);
            p->inc.upload(p->host.inc, ctx->stream);
            p->off_blk.upload(p->host.off_blk, ctx->stream);
            CUGO_HIP(hipStreamSynchronize(ctx->stream)); // (the caller's index arrays are pageable and may go away)
            p->on_device = true;
        }
        *out = p.release();
    });
}
void cugo_relpose_plan_destroy(cugo_relpose_plan* plan) { delete plan; }

int cugo_relpose_plan_array(const cugo_relpose_plan* plan, const char* name, const int32_t** out)
{
    if (!plan || !name || !out)
        return CUGO_ERR_INVALID;
    const std::string n = name;
    const std::vector<int32_t>* v = n == "inc_ptr" ? &plan->host.inc_ptr : n == "inc" ? &plan->host.inc
                                    : n == "off_blk" ? &plan->host.off_blk : nullptr;
    if (!v)
    {
        set_last_error("cugo_relpose_plan_array: unknown array " + n);
        return CUGO_ERR_INVALID;
    }
    *out = v->data();
    return (int)v->size();
}

int cugo_relpose_pattern(int n, int n_poses_free, const int32_t* h_pose_a, const int32_t* h_pose_b,
                         const uint8_t* h_flags, int32_t* rowptr_out, int32_t* colind_out, int* nnzb)
{
    return guarded([&] {
        if (!nnzb)
            throw std::runtime_error("cugo_relpose_pattern: null argument");
        *nnzb = cugo_host::relpose_pattern(n, n_poses_free, h_pose_a, h_pose_b, h_flags, rowptr_out, colind_out);
    });
}

int cugo_relpose_compute_errors(cugo_ctx* ctx, const cugo_relpose_edges* ev, const double* d_poses, double* d_chi,
                                double* d_edge_chi)
{
    return guarded([&] {
        const cugo_k::ReduceScratch rs = check_relpose(ctx, ev);
        if (d_edge_chi && ev->n > 0) // (the kernel writes the edges that count)
            CUGO_HIP(hipMemsetAsync(d_edge_chi, 0, sizeof(double) * ev->n, ctx->stream));
        cugo_k::launch_relpose_errors(ctx->stream, *ev, ev->plan->dev(), d_poses, rs.d_partials, d_edge_chi);
        relpose_chi_total(ctx, ev, rs, d_chi);
        CUGO_HIP(hipGetLastError());
    });
}

int cugo_relpose_construct_quadratic_form(cugo_ctx* ctx, const cugo_relpose_edges* ev, const double* d_poses,
                                          double* d_Hpp, double* d_bp, double* d_Hoff, double* d_chi)
{
    return guarded([&] {
        const cugo_k::ReduceScratch rs = check_relpose(ctx, ev);
        if (ev->n > 0 && ev->n_poses_free > 0 && (!d_Hpp || !d_bp))
            throw std::runtime_error("cugo_relpose: missing Hpp or bp");
        if (!d_Hoff)
            for (int32_t k : ev->plan->host.off_blk)
                if (k >= 0)
                    throw std::runtime_error("cugo_relpose: missing Hoff (an edge joins two free poses)");
        cugo_k::launch_relpose_add(ctx->stream, *ev, ev->plan->dev(), d_poses, d_Hpp, d_bp, d_Hoff, rs.d_partials);
        relpose_chi_total(ctx, ev, rs, d_chi);
        CUGO_HIP(hipGetLastError());
    });
}

int cugo_relpose_construct_quadratic_form_schur(cugo_ctx* ctx, const cugo_relpose_edges* ev, const double* d_poses,
                                                const int32_t* d_rowptr, double* d_Hsc, double* d_bp, double* d_bsc,
                                                double* d_chi)
{
    return guarded([&] {
        const cugo_k::ReduceScratch rs = check_relpose(ctx, ev);
        if (!d_rowptr || !d_Hsc || !d_bp || !d_bsc)
            throw std::runtime_error("cugo_relpose: missing rowptr, Hsc, bp or bsc");
        cugo_k::launch_relpose_add_schur(ctx->stream, *ev, ev->plan->dev(), d_poses, d_rowptr, d_Hsc, d_bp, d_bsc, rs.d_partials);
        relpose_chi_total(ctx, ev, rs, d_chi);
        CUGO_HIP(hipGetLastError());
    });
}

int cugo_relpose_construct_quadratic_form_diag(cugo_ctx* ctx, const cugo_relpose_edges* ev, const double* d_poses,
                                               double* d_Hpp, double* d_bp, double* d_chi)
{
    return guarded([&] {
        const cugo_k::ReduceScratch rs = check_relpose(ctx, ev);
        if (ev->n > 0 && ev->n_poses_free > 0 && (!d_Hpp || !d_bp))
            throw std::runtime_error("cugo_relpose: missing Hpp or bp");
        cugo_k::launch_relpose_add(ctx->stream, *ev, ev->plan->dev(), d_poses, d_Hpp, d_bp, nullptr, rs.d_partials);
        relpose_chi_total(ctx, ev, rs, d_chi);
        CUGO_HIP(hipGetLastError());
    });
}

int cugo_relpose_add_offdiag_schur(cugo_ctx* ctx, const cugo_relpose_edges* ev, const double* d_poses, double* d_Hsc)
{
    return guarded([&] {
        (void)check_relpose(ctx, ev);
        if (!d_Hsc)
            throw std::runtime_error("cugo_relpose: missing Hsc");
        cugo_k::launch_relpose_add_offdiag(ctx->stream, *ev, ev->plan->dev(), d_poses, d_Hsc);
        CUGO_HIP(hipGetLastError());
    });
}

} // extern "C"

// the plan of a set of pose-pose point edges: the host plan (point_pair_plan.h) and, with a context, its copy on the
// device and the scratch of the set's passes (partials, chunk totals, the flag of the index check)
struct cugo_point_pair_plan
{
    cugo_host::PointPairPlanHost host;
    bool on_device = false, has_pattern = false;
    cugo_host::DevBuf<int32_t> edge_run, run_ptr, run_a, run_b, run_flags, inc_ptr, inc, blk_id, blk_ptr, blk_run;
    mutable cugo_host::DevBuf<double> scratch;
    mutable bool built = false; // the scratch holds the partials of a build pass
    int n_runs() const { return (int)host.run_a.size(); }
    cugo_k::PointPairPlanDev dev() const
    {
        return {host.n,         n_runs(),     host.n_poses_free, (int)host.blk_id.size(), edge_run.data(), run_ptr.data(),
                run_a.data(),   run_b.data(), run_flags.data(),  inc_ptr.data(),          inc.data(),      blk_id.data(),
                blk_ptr.data(), blk_run.data()};
    }
    cugo_k::ChunkScratch pair_scratch() const
    {
        return cugo_k::point_pair_scratch_in({scratch.data(), scratch.size()}, host.n, n_runs());
    }
};

namespace
{
// Both forms come here as a cugo_point_pair_edges view: the covariance form (cugo_gicp_pair_edges) with d_info = cov_p,
// n_info = n_cov and its cov_z beside it
struct PairView
{
    cugo_point_pair_edges ev;
    const double* d_cov_z; // nullptr: the information form
    bool cov;
    std::string who;
};
const cugo_point_pair_edges NO_PAIR_EDGES = {0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, 0.0, nullptr}; // (refused)
PairView view_of(const cugo_point_pair_edges* ev) { return {ev ? *ev : NO_PAIR_EDGES, nullptr, false, "cugo_point_pair"}; }
PairView view_of(const cugo_gicp_pair_edges* g)
{
    if (!g)
        return {NO_PAIR_EDGES, nullptr, true, "cugo_gicp_pair"};
    return {{g->n_poses_total, g->n_poses_free, g->n, g->d_pose_a, g->d_pose_b, g->d_p, g->d_z, g->d_cov_p, g->n_cov, g->d_flags,
             g->rk, g->delta, g->plan},
            g->d_cov_z, true, "cugo_gicp_pair"};
}
// counts against the plan, arrays, kernel code on the host; with check_indices, pose a / b of every edge against the
// plan's runs on the device
cugo_k::ChunkScratch check_point_pair(cugo_ctx* ctx, const PairView& v, bool check_indices = true)
{
    const cugo_point_pair_edges* ev = &v.ev;
    if (!ctx)
        throw std::runtime_error(v.who + ": no context");
    if (!ev->plan)
        throw std::runtime_error(v.who + ": no edges or no plan (cugo_point_pair_plan_create)");
    const cugo_host::PointPairPlanHost& h = ev->plan->host;
    if (ev->n != h.n || ev->n_poses_total != h.n_poses_total || ev->n_poses_free != h.n_poses_free)
        throw std::runtime_error(v.who + ": the pose or edge counts are not those of the plan");
    if (!ev->plan->on_device)
        throw std::runtime_error(v.who + ": the plan is host-only (created without a context)");
    if (!ev->plan->has_pattern)
        throw std::runtime_error(v.who + ": the plan was built without a pattern");
    if (ev->rk < CUGO_RK_NONE || ev->rk > CUGO_RK_HUBER || (ev->rk != CUGO_RK_NONE && !(ev->delta > 0.0 && std::isfinite(ev->delta))))
        throw std::runtime_error(v.who + ": unknown robust kernel or bad delta");
    if (ev->n > 0 && (!ev->d_pose_a || !ev->d_pose_b || !ev->d_p || !ev->d_z || !ev->d_info || (v.cov && !v.d_cov_z) ||
                      (ev->n_info != 1 && ev->n_info != ev->n)))
        throw std::runtime_error(v.who + (v.cov ? ": missing arrays, or n_cov is neither n nor 1" : ": missing arrays, or n_info is neither n nor 1"));
    const cugo_k::ChunkScratch rs = ev->plan->pair_scratch();
    if (check_indices &&
        cugo_k::point_pair_check_indices(ctx->stream, *ev, ev->plan->dev(),
                                         reinterpret_cast<int*>(ev->plan->scratch.data() + cugo_k::point_pair_scratch_doubles(h.n, ev->plan->n_runs()))))
        throw std::runtime_error(v.who + ": pose a or pose b of an edge is not that of its run: the edges are not in the plan's order");
    return rs;
}
void point_pair_build(cugo_ctx* ctx, const PairView& v, const double* d_poses, cugo_k::ChunkScratch rs)
{
    if (!d_poses)
        throw std::runtime_error(v.who + ": missing poses");
    v.ev.plan->built = false;
    cugo_k::launch_point_pair_chunks(ctx->stream, v.ev, v.ev.plan->dev(), d_poses, true, rs, nullptr, v.d_cov_z);
    v.ev.plan->built = true;
}
void point_pair_chi_total(cugo_ctx* ctx, const cugo_point_pair_edges* ev, cugo_k::ChunkScratch rs, double* d_chi)
{
    if (!d_chi)
        return;
    if (ev->n > 0)
        cugo_k::launch_point_pair_chi_total(ctx->stream, *ev, rs, d_chi, false);
    else
        CUGO_HIP(hipMemsetAsync(d_chi, 0, sizeof(double), ctx->stream));
}
bool joins_free_poses(const cugo_point_pair_edges* ev) { return !ev->plan->host.blk_id.empty(); }

// the five passes of the pair kind, for either form
int pair_errors(cugo_ctx* ctx, const PairView& v, const double* d_poses, double* d_chi, double* d_edge_chi)
{
    return guarded([&] {
        const cugo_point_pair_edges* ev = &v.ev;
        const cugo_k::ChunkScratch rs = check_point_pair(ctx, v);
        if (!d_poses)
            throw std::runtime_error(v.who + ": missing poses");
        cugo_k::launch_point_pair_chunks(ctx->stream, *ev, ev->plan->dev(), d_poses, false, rs, d_edge_chi, v.d_cov_z);
        point_pair_chi_total(ctx, ev, rs, d_chi);
        CUGO_HIP(hipGetLastError());
    });
}
int pair_form(cugo_ctx* ctx, const PairView& v, const double* d_poses, double* d_Hpp, double* d_bp, double* d_Hoff, double* d_chi)
{
    return guarded([&] {
        const cugo_point_pair_edges* ev = &v.ev;
        const cugo_k::ChunkScratch rs = check_point_pair(ctx, v);
        if (ev->n > 0 && ev->n_poses_free > 0 && (!d_Hpp || !d_bp))
            throw std::runtime_error(v.who + ": missing Hpp or bp");
        if (!d_Hoff && joins_free_poses(ev))
            throw std::runtime_error(v.who + ": missing Hoff (a counting run joins two free poses)");
        point_pair_build(ctx, v, d_poses, rs);
        cugo_k::launch_point_pair_add(ctx->stream, *ev, ev->plan->dev(), rs, d_Hpp, d_bp, d_Hoff);
        point_pair_chi_total(ctx, ev, rs, d_chi);
        CUGO_HIP(hipGetLastError());
    });
}
int pair_form_schur(cugo_ctx* ctx, const PairView& v, const double* d_poses, const int32_t* d_rowptr, double* d_Hsc, double* d_bp,
                    double* d_bsc, double* d_chi)
{
    return guarded([&] {
        const cugo_point_pair_edges* ev = &v.ev;
        const cugo_k::ChunkScratch rs = check_point_pair(ctx, v);
        if (!d_rowptr || !d_Hsc || !d_bp || !d_bsc)
            throw std::runtime_error(v.who + ": missing rowptr, Hsc, bp or bsc");
        point_pair_build(ctx, v, d_poses, rs);
        cugo_k::launch_point_pair_add_schur(ctx->stream, *ev, ev->plan->dev(), rs, d_rowptr, d_Hsc, d_bp, d_bsc);
        point_pair_chi_total(ctx, ev, rs, d_chi);
        CUGO_HIP(hipGetLastError());
    });
}
int pair_form_diag(cugo_ctx* ctx, const PairView& v, const double* d_poses, double* d_Hpp, double* d_bp, double* d_chi)
{
    return guarded([&] {
        const cugo_point_pair_edges* ev = &v.ev;
        const cugo_k::ChunkScratch rs = check_point_pair(ctx, v);
        if (ev->n > 0 && ev->n_poses_free > 0 && (!d_Hpp || !d_bp))
            throw std::runtime_error(v.who + ": missing Hpp or bp");
        point_pair_build(ctx, v, d_poses, rs);
        cugo_k::launch_point_pair_add_diag(ctx->stream, *ev, ev->plan->dev(), rs, d_Hpp, d_bp);
        point_pair_chi_total(ctx, ev, rs, d_chi);
        CUGO_HIP(hipGetLastError());
    });
}
int pair_add_offdiag_schur(cugo_ctx* ctx, const PairView& v, double* d_Hsc)
{
    return guarded([&] {
        const cugo_point_pair_edges* ev = &v.ev;
        const cugo_k::ChunkScratch rs = check_point_pair(ctx, v, false); // (the build pass checked the indices)
        if (!ev->plan->built)
            throw std::runtime_error(v.who + "_add_offdiag_schur: no build pass has left its partials in the plan's scratch");
        if (!d_Hsc)
            throw std::runtime_error(v.who + ": missing Hsc");
        cugo_k::launch_point_pair_add_offdiag(ctx->stream, *ev, ev->plan->dev(), rs, d_Hsc);
        CUGO_HIP(hipGetLastError());
    });
}
} // namespace

extern "C" {

int cugo_point_pair_plan_create(cugo_ctx* ctx, int n, int n_poses_total, int n_poses_free, const int32_t* h_pose_a,
                                const int32_t* h_pose_b, const uint8_t* h_flags, const int32_t* h_rowptr,
                                const int32_t* h_colind, cugo_point_pair_plan** out)
{
    return guarded([&] {
        if (!out)
            throw std::runtime_error("cugo_point_pair_plan_create: null argument");
        *out = nullptr;
        if (n > (1 << 26))
            throw std::runtime_error("cugo_point_pair_plan_create: more than 2^26 edges");
        auto p = std::make_unique<cugo_point_pair_plan>();
        cugo_host::build_point_pair_plan(n, n_poses_total, n_poses_free, h_pose_a, h_pose_b, h_flags, h_rowptr, h_colind, p->host);
        p->has_pattern = h_rowptr != nullptr;
        if (ctx)
        {
            const cugo_host::PointPairPlanHost& h = p->host;
            p->edge_run.upload(h.edge_run, ctx->stream);
            p->run_ptr.upload(h.run_ptr, ctx->stream);
            p->run_a.upload(h.run_a, ctx->stream);
            p->run_b.upload(h.run_b, ctx->stream);
            p->run_flags.upload(h.run_flags, ctx->stream);
            p->inc_ptr.upload(h.inc_ptr, ctx->stream);
            p->inc.upload(h.inc, ctx->stream);
            p->blk_id.upload(h.blk_id, ctx->stream);
            p->blk_ptr.upload(h.blk_ptr, ctx->stream);
            p->blk_run.upload(h.blk_run, ctx->stream);
            p->scratch.resize(cugo_k::point_pair_scratch_doubles(n, p->n_runs()) + 16); // (+ the flag of the index check)
            CUGO_HIP(hipStreamSynchronize(ctx->stream));
            p->on_device = true;
        }
        *out = p.release();
    });
}
void cugo_point_pair_plan_destroy(cugo_point_pair_plan* plan) { delete plan; }

int cugo_point_pair_plan_array(const cugo_point_pair_plan* plan, const char* name, const int32_t** out)
{
    if (!plan || !name || !out)
        return CUGO_ERR_INVALID;
    const cugo_host::PointPairPlanHost& h = plan->host;
    const std::pair<const char*, const std::vector<int32_t>*> arrays[] = {
        {"perm", &h.perm},       {"edge_run", &h.edge_run}, {"run_ptr", &h.run_ptr}, {"run_a", &h.run_a},   {"run_b", &h.run_b},
        {"run_flags", &h.run_flags}, {"run_blk", &h.run_blk}, {"inc_ptr", &h.inc_ptr}, {"inc", &h.inc},       {"blk_id", &h.blk_id},
        {"blk_ptr", &h.blk_ptr}, {"blk_run", &h.blk_run},   {"pair_lo", &h.pair_lo}, {"pair_hi", &h.pair_hi}};
    for (const auto& a : arrays)
        if (std::string(name) == a.first)
        {
            *out = a.second->data();
            return (int)a.second->size();
        }
    set_last_error(std::string("cugo_point_pair_plan_array: unknown array ") + name);
    return CUGO_ERR_INVALID;
}

int cugo_point_pair_compute_errors(cugo_ctx* ctx, const cugo_point_pair_edges* ev, const double* d_poses, double* d_chi,
                                   double* d_edge_chi)
{
    return pair_errors(ctx, view_of(ev), d_poses, d_chi, d_edge_chi);
}
int cugo_point_pair_construct_quadratic_form(cugo_ctx* ctx, const cugo_point_pair_edges* ev, const double* d_poses,
                                             double* d_Hpp, double* d_bp, double* d_Hoff, double* d_chi)
{
    return pair_form(ctx, view_of(ev), d_poses, d_Hpp, d_bp, d_Hoff, d_chi);
}
int cugo_point_pair_construct_quadratic_form_schur(cugo_ctx* ctx, const cugo_point_pair_edges* ev, const double* d_poses,
                                                   const int32_t* d_rowptr, double* d_Hsc, double* d_bp, double* d_bsc,
                                                   double* d_chi)
{
    return pair_form_schur(ctx, view_of(ev), d_poses, d_rowptr, d_Hsc, d_bp, d_bsc, d_chi);
}
int cugo_point_pair_construct_quadratic_form_diag(cugo_ctx* ctx, const cugo_point_pair_edges* ev, const double* d_poses,
                                                  double* d_Hpp, double* d_bp, double* d_chi)
{
    return pair_form_diag(ctx, view_of(ev), d_poses, d_Hpp, d_bp, d_chi);
}
int cugo_point_pair_add_offdiag_schur(cugo_ctx* ctx, const cugo_point_pair_edges* ev, double* d_Hsc)
{
    return pair_add_offdiag_schur(ctx, view_of(ev), d_Hsc);
}

int cugo_gicp_pair_compute_errors(cugo_ctx* ctx, const cugo_gicp_pair_edges* ev, const double* d_poses, double* d_chi,
                                  double* d_edge_chi)
{
    return pair_errors(ctx, view_of(ev), d_poses, d_chi, d_edge_chi);
}
int cugo_gicp_pair_construct_quadratic_form(cugo_ctx* ctx, const cugo_gicp_pair_edges* ev, const double* d_poses,
                                            double* d_Hpp, double* d_bp, double* d_Hoff, double* d_chi)
{
    return pair_form(ctx, view_of(ev), d_poses, d_Hpp, d_bp, d_Hoff, d_chi);
}
int cugo_gicp_pair_construct_quadratic_form_schur(cugo_ctx* ctx, const cugo_gicp_pair_edges* ev, const double* d_poses,
                                                  const int32_t* d_rowptr, double* d_Hsc, double* d_bp, double* d_bsc,
                                                  double* d_chi)
{
    return pair_form_schur(ctx, view_of(ev), d_poses, d_rowptr, d_Hsc, d_bp, d_bsc, d_chi);
}
int cugo_gicp_pair_construct_quadratic_form_diag(cugo_ctx* ctx, const cugo_gicp_pair_edges* ev, const double* d_poses,
                                                 double* d_Hpp, double* d_bp, double* d_chi)
{
    return pair_form_diag(ctx, view_of(ev), d_poses, d_Hpp, d_bp, d_chi);
}
int cugo_gicp_pair_add_offdiag_schur(cugo_ctx* ctx, const cugo_gicp_pair_edges* ev, double* d_Hsc)
{
    return pair_add_offdiag_schur(ctx, view_of(ev), d_Hsc);
}

int cugo_max_diagonal(cugo_ctx* ctx, const double* d_Hpp, int nP, const double* d_Hll, int nL,
                      double* d_out)
{
    return guarded([&] {
        cugo_k::launch_max_diagonal(ctx->stream, d_Hpp, nP, d_Hll, nL, scratch_for(ctx, nullptr),
                                    d_out);
        CUGO_HIP(hipGetLastError());
    });
}

int cugo_compute_schur(cugo_ctx* ctx, const cugo_edges* ev, const cugo_hsc_struct* hs, double lambda,
                       int damp_hsc_diag, const double* d_Hpp, const double* d_bp,
                       const double* d_Hll, const double* d_bl, const void* d_Hpl,
                       double* d_invHll, void* d_T, double* d_bsc, double* d_Hsc)
{
    return guarded([&] {
        if (!d_T && !hs->d_grp_ptr)
            throw std::runtime_error("cugo_compute_schur: d_T may only be NULL with a landmark-major plan "
                                     "(cugo_hsc_plan_create); the gather kernels read T from memory");
        cugo_k::SchurRows form;
        form.mfma = ctx->opt.hsc_mfma, form.xcd = ctx->opt.hsc_xcd;
        cugo_k::launch_schur(ctx->stream, *ev, *hs, lambda, damp_hsc_diag, d_Hpp, d_bp, d_Hll, d_bl,
                             d_Hpl, d_invHll, d_T, d_bsc, d_Hsc, false, form);
        CUGO_HIP(hipGetLastError());
    });
}

int cugo_backsubst_update(cugo_ctx* ctx, const cugo_edges* ev, double lambda,
                          const double* d_invHll, const double* d_bl, const double* d_bp,
                          const void* d_Hpl, const double* d_xp, double* d_xl,
                          const double* d_poses_in, const double* d_lms_in, double* d_poses_out,
                          double* d_lms_out, double* d_scale)
{
    return guarded([&] {
        cugo_k::launch_backsubst_update(ctx->stream, *ev, lambda, lambda, d_invHll, d_bl, d_bp, d_Hpl,
                                        d_xp, d_xl, d_poses_in, d_lms_in, d_poses_out, d_lms_out,
                                        scratch_for(ctx, ev), d_scale);
        CUGO_HIP(hipGetLastError());
    });
}

// ---------------------------------------------------------------- fused iteration ------
// The forms of the three passes that the LM loop runs from its second iteration on (engine.cpp: queue_build, queue_schur
// and the update of a trial), through the same launchers.  Every argument is checked before the context is touched.
int cugo_construct_quadratic_form_fused(cugo_ctx* ctx, const cugo_edges* ev, const int32_t* h_lm_ptr, const double* d_poses,
                                        const double* d_lms, cugo_robust rk, double lambda, int form, double* d_Hpp,
                                        double* d_bp, double* d_Hll, double* d_bl, void* d_Hpl, double* d_invHll,
                                        void* d_T, double* d_lmrec, double* d_chi)
{
    return guarded([&] {
        const char* who = "cugo_construct_quadratic_form_fused: ";
        auto refuse = [&](const char* what) { throw std::runtime_error(std::string(who) + what); };
        if (!ev || !h_lm_ptr)
            refuse("null ev or h_lm_ptr");
        if (form != 1 && form != 2)
            refuse("form must be 1 (two-stream) or 2 (one-stream)");
        if (!(lambda >= 0.0) || !std::isfinite(lambda))
            refuse("lambda must be finite and >= 0");
        if (!d_invHll || !d_T || !d_Hll || !d_bl)
            refuse("null d_invHll, d_T, d_Hll or d_bl (d_invHll is the launcher's fuse switch in either form)");
        if (form == 2 && !d_lmrec)
            refuse("form 2 needs d_lmrec");
        if (form == 1 && (!d_Hpl || (ev->n_poses_free > 0 && (!d_Hpp || !d_bp))))
            refuse("form 1 needs d_Hpl, d_Hpp and d_bp");
        check_edge_form(ev, "cugo_construct_quadratic_form_fused");
        // what the engine's slot layout guarantees and the fused kernel relies on: a landmark's slots in one group
        for (int l = 0; l < ev->n_landmarks_total; l++)
        {
            const int a = h_lm_ptr[l], b = h_lm_ptr[l + 1];
            if (a < 0 || b < a || b > ev->n_edges)
                refuse("h_lm_ptr is not a slot range list of ev");
            if (b > a && a / 256 != (b - 1) / 256)
                refuse("a landmark's edge slots lie in two 256-slot groups");
        }
        if (!ctx)
            refuse("null context");
        cugo_k::launch_build(ctx->stream, *ev, d_poses, d_lms, rk, d_Hpp, d_bp, d_Hll, d_bl, d_Hpl, scratch_for(ctx, ev),
                             d_chi, lambda, d_invHll, d_T, form == 2 ? d_lmrec : nullptr, form == 2);
        CUGO_HIP(hipGetLastError());
    });
}

int cugo_compute_schur_fused(cugo_ctx* ctx, const cugo_edges* ev, const cugo_hsc_struct* hs, double lambda,
                             int damp_hsc_diag, int form, const double* d_poses, const double* d_Hpp, const double* d_bp,
                             const double* d_Hll, const double* d_bl, const void* d_Hpl, double* d_invHll, void* d_T,
                             const double* d_lmrec, double* d_bp_out, double* d_bsc, double* d_Hsc)
{
    return guarded([&] {
        const char* who = "cugo_compute_schur_fused: ";
        auto refuse = [&](const char* what) { throw std::runtime_error(std::string(who) + what); };
        if (!ev || !hs)
            refuse("null ev or hs");
        if (form != 1 && form != 2)
            refuse("form must be 1 (two-stream) or 2 (one-stream)");
        if (!(lambda >= 0.0) || !std::isfinite(lambda))
            refuse("lambda must be finite and >= 0");
        if (hs->d_grp_ptr)
            refuse("hs carries a landmark-major plan: the fused forms run the gather kernels");
        if (!d_T || !d_bsc || !d_Hsc)
            refuse("null d_T, d_bsc or d_Hsc");
        if (form == 2 && (!d_lmrec || !d_poses || !d_bp_out || !hs->d_rowptr))
            refuse("form 2 needs d_lmrec, d_poses, d_bp_out and hs->d_rowptr");
        if (form == 1 && (!d_Hpl || !d_bl || (ev->n_poses_free > 0 && (!d_Hpp || !d_bp))))
            refuse("form 1 needs d_Hpl, d_bl, d_Hpp and d_bp");
        check_edge_form(ev, "cugo_compute_schur_fused");
        if (!ctx)
            refuse("null context");
        cugo_k::SchurRows rows;
        rows.mfma = ctx->opt.hsc_mfma, rows.xcd = ctx->opt.hsc_xcd;
        if (form == 2)
        {
            rows.d_lmrec = d_lmrec, rows.d_poses = d_poses, rows.d_bp_out = d_bp_out;
            rows.rs = scratch_for(ctx, ev); // the records of the fused build entry: same ev, same size, no resize
        }
        cugo_k::launch_schur(ctx->stream, *ev, *hs, lambda, damp_hsc_diag, d_Hpp, d_bp, d_Hll, d_bl, d_Hpl, d_invHll, d_T,
                             d_bsc, d_Hsc, true, rows);
        CUGO_HIP(hipGetLastError());
    });
}

int cugo_backsubst_update_fused(cugo_ctx* ctx, const cugo_edges* ev, double lambda, const double* d_lmrec,
                                const double* d_bl, const double* d_bp, const void* d_G, const double* d_xp, double* d_xl,
                                const double* d_poses_in, const double* d_lms_in, double* d_poses_out, double* d_lms_out,
                                double* d_scale, int from_records)
{
    return guarded([&] {
        const char* who = "cugo_backsubst_update_fused: ";
        auto refuse = [&](const char* what) { throw std::runtime_error(std::string(who) + what); };
        if (!ev)
            refuse("null ev");
        if (!(lambda >= 0.0) || !std::isfinite(lambda))
            refuse("lambda must be finite and >= 0");
        if (!d_lmrec)
            refuse(from_records ? "from_records without the landmarks' lines (d_lmrec)" : "null d_lmrec");
        if (!d_G || !d_bl || !d_bp || !d_xp || !d_xl || !d_poses_in || !d_lms_in || !d_poses_out || !d_lms_out)
            refuse("null argument");
        check_edge_form(ev, "cugo_backsubst_update_fused");
        if (!ctx)
            refuse("null context");
        cugo_k::launch_backsubst_update(ctx->stream, *ev, lambda, lambda, nullptr, d_bl, d_bp, d_G, d_xp, d_xl, d_poses_in,
                                        d_lms_in, d_poses_out, d_lms_out, scratch_for(ctx, ev), d_scale, d_lmrec,
                                        from_records != 0);
        CUGO_HIP(hipGetLastError());
    });
}

// ---------------------------------------------------------------- sparse LL^T ----------
int cugo_chol_create(cugo_ctx* ctx, cugo_chol** out)
{
    return guarded([&] {
        auto* s = new cugo_chol;
        s->ctx = ctx;
        *out = s;
    });
}
void cugo_chol_destroy(cugo_chol* s)
{
    if (s && s->ctx)
        (void)hipStreamSynchronize(s->ctx->stream);
    delete s;
}
int cugo_chol_analyze(cugo_chol* s, int n, const int32_t* rowptr, const int32_t* colind)
{
    return guarded([&] { s->analyze(n, rowptr, colind); });
}
int cugo_chol_factor_solve(cugo_chol* s, const double* d_Hsc, double lambda, const double* d_bsc,
                           double* d_x, int32_t* d_fail)
{
    return guarded([&] {
        if (!s->analyzed || !s->ctx)
            throw std::runtime_error("cugo_chol_factor_solve needs an analysed solver with a device context");
        s->factor_solve(d_Hsc, lambda, d_bsc, d_x, d_fail);
    });
}
int cugo_chol_selected_inverse(cugo_chol* s, double* d_sigma)
{
    bool ok = true;
    const int rc = guarded([&] {
        if (!s || !s->ctx || !s->analyzed || !s->factored)
            throw std::runtime_error("cugo_chol_selected_inverse needs a factorisation (cugo_chol_factor_solve) since the "
                                     "last analyze()");
        if (s->own_subtrees())
            throw std::runtime_error("cugo_chol_selected_inverse: not available when the solver factors rank-owned "
                                     "subtrees");
        ok = s->selected_inverse(d_sigma);
    });
    if (rc != CUGO_OK)
        return rc;
    if (!ok)
    {
        set_last_error("cugo_chol_selected_inverse: the factorisation hit a zero pivot");
        return CUGO_ERR_NUMERIC;
    }
    return CUGO_OK;
}
int cugo_chol_inverse_blocks(cugo_chol* s, int n_pairs, const int32_t* h_rows, const int32_t* h_cols, double* d_out)
{
    bool ok = true;
    const int rc = guarded([&] {
        if (!s || !s->analyzed)
            throw std::runtime_error("cugo_chol_inverse_blocks needs an analysed solver");
        if (n_pairs < 0)
            throw std::invalid_argument("cugo_chol_inverse_blocks: negative count");
        for (int k = 0; k < n_pairs; k++)
            if (h_rows[k] < 0 || h_rows[k] >= s->plan.n || h_cols[k] < 0 || h_cols[k] >= s->plan.n)
                throw std::invalid_argument("cugo_chol_inverse_blocks: pair " + std::to_string(k) + " names a block row "
                                            "outside [0, " + std::to_string(s->plan.n) + ")");
        if (!s->ctx || !s->factored)
            throw std::runtime_error("cugo_chol_inverse_blocks needs a factorisation (cugo_chol_factor_solve) since the "
                                     "last analyze()");
        if (s->own_subtrees())
            throw std::runtime_error("cugo_chol_inverse_blocks: not available when the solver factors rank-owned "
                                     "subtrees");
        ok = s->inverse_blocks(n_pairs, h_rows, h_cols, d_out);
    });
    if (rc != CUGO_OK)
        return rc;
    if (!ok)
    {
        set_last_error("cugo_chol_inverse_blocks: the factorisation hit a zero pivot");
        return CUGO_ERR_NUMERIC;
    }
    return CUGO_OK;
}
int cugo_landmark_covariances(cugo_ctx* ctx, const cugo_edges* ev, const cugo_hsc_struct* hs, const double* d_Hll,
                              const double* d_Hpl, const double* d_sigma, double* d_cov9, int32_t* d_fail)
{
    return guarded([&] {
        if (!ctx || !ev || !hs || !d_Hll || !d_Hpl || !d_sigma || !d_cov9 || !d_fail)
            throw std::invalid_argument("cugo_landmark_covariances: null argument");
        if (ev->block_f32)
            throw std::invalid_argument("cugo_landmark_covariances: the kernel reads Hpl as fp64 (ev->block_f32 is set)");
        if (ev->n_landmarks_free <= 0)
            return;
        if (!ev->d_lm_ptr || !ev->d_pose || !ev->d_flags || !hs->d_rowptr || !hs->d_colind)
            throw std::invalid_argument("cugo_landmark_covariances: null array in ev or hs");
        CUGO_HIP(hipMemsetAsync(d_fail, 0, sizeof(int32_t), ctx->stream));
        cugo_k::launch_lm_covariance(ctx->stream, ev->n_landmarks_free, ev->d_lm_ptr, ev->d_pose, ev->d_flags, d_Hll,
                                     d_Hpl, hs->d_rowptr, hs->d_colind, d_sigma, d_cov9, d_fail);
        CUGO_HIP(hipGetLastError());
    });
}
int cugo_plcov_plan_create(int n_poses_free, int n_landmarks, const int32_t* h_lm_ptr, const int32_t* h_slot_pose, int n,
                           const int32_t* h_q_pose, const int32_t* h_q_lm, cugo_plcov_plan** out)
{
    return guarded([&] {
        if (!out)
            throw std::invalid_argument("cugo_plcov_plan_create: null argument");
        *out = nullptr;
        auto p = std::make_unique<cugo_plcov_plan>();
        cugo_host::build_plcov_plan(n_poses_free, n_landmarks, h_lm_ptr, h_slot_pose, n, h_q_pose, h_q_lm, p->host);
        *out = p.release();
    });
}
void cugo_plcov_plan_destroy(cugo_plcov_plan* plan) { delete plan; }
int cugo_plcov_plan_array(const cugo_plcov_plan* plan, const char* name, const int32_t** out)
{
    if (!plan || !name || !out)
        return CUGO_ERR_INVALID;
    const std::string n = name;
    const cugo_host::PlCovPlanHost& h = plan->host;
    const std::vector<int32_t>* v = n == "rows" ? &h.rows : n == "cols" ? &h.cols : n == "q_ptr" ? &h.q_ptr
                                    : n == "q_slot" ? &h.q_slot : n == "q_aa" ? &h.q_aa : nullptr;
    if (!v)
    {
        set_last_error("cugo_plcov_plan_array: unknown array " + n);
        return CUGO_ERR_INVALID;
    }
    *out = v->data();
    return (int)v->size();
}
int cugo_pose_landmark_cross_covariances(cugo_ctx* ctx, const cugo_edges* ev, int n, const int32_t* d_q_pose,
                                         const int32_t* d_q_lm, const int32_t* d_q_ptr, const int32_t* d_q_slot,
                                         const double* d_Hll, const double* d_Hpl, const double* d_blocks,
                                         double* d_cov18, int32_t* d_fail)
{
    return guarded([&] {
        if (!ctx || !ev || !d_q_pose || !d_q_lm || !d_q_ptr || !d_q_slot || !d_Hll || !d_Hpl || !d_blocks || !d_cov18 ||
            !d_fail)
            throw std::invalid_argument("cugo_pose_landmark_cross_covariances: null argument");
        if (n < 0)
            throw std::invalid_argument("cugo_pose_landmark_cross_covariances: negative count");
        if (ev->block_f32)
            throw std::invalid_argument("cugo_pose_landmark_cross_covariances: the kernel reads Hpl as fp64 (ev->block_f32 "
                                        "is set)");
        if (n == 0)
            return;
        if (!ev->d_lm_ptr || !ev->d_flags)
            throw std::invalid_argument("cugo_pose_landmark_cross_covariances: null array in ev");
        CUGO_HIP(hipMemsetAsync(d_fail, 0, sizeof(int32_t), ctx->stream));
        cugo_k::launch_pose_lm_cross(ctx->stream, n, d_q_pose, d_q_lm, d_q_ptr, d_q_slot, ev->d_lm_ptr, ev->d_flags, d_Hll,
                                     d_Hpl, d_blocks, d_cov18, d_fail);
        CUGO_HIP(hipGetLastError());
    });
}
int cugo_reprojection_covariances(cugo_ctx* ctx, int n, int n_landmarks_free, const int32_t* d_q_pose,
                                  const int32_t* d_q_lm, const int32_t* d_q_dim, const int32_t* d_q_aa,
                                  const double* d_cam5, const double* d_poses, const double* d_lms,
                                  const double* d_blocks, const double* d_cross18, const double* d_lmcov9, double* d_cov9)
{
    return guarded([&] {
        if (!ctx || !d_q_pose || !d_q_lm || !d_q_dim || !d_q_aa || !d_cam5 || !d_poses || !d_lms || !d_blocks ||
            !d_cross18 || !d_lmcov9 || !d_cov9)
            throw std::invalid_argument("cugo_reprojection_covariances: null argument");
        if (n < 0 || n_landmarks_free < 0)
            throw std::invalid_argument("cugo_reprojection_covariances: negative count");
        if (n == 0)
            return;
        cugo_k::launch_reprojection_cov(ctx->stream, n, n_landmarks_free, d_q_pose, d_q_lm, d_q_dim, d_q_aa, d_cam5,
                                        d_poses, d_lms, d_blocks, d_cross18, d_lmcov9, d_cov9);
        CUGO_HIP(hipGetLastError());
    });
}
int cugo_predict_observations(cugo_ctx* ctx, int n, int n_landmarks_free, const int32_t* d_q_pose, const int32_t* d_q_lm,
                              const int32_t* d_q_kind, const int32_t* d_q_aa, const double* d_cam5, const double* d_cam_tab,
                              const double* d_poses, const double* d_lms, const double* d_blocks, const double* d_cross18,
                              const double* d_lmcov9, double* d_z3, double* d_cov9)
{
    return guarded([&] {
        if (!ctx || !d_q_pose || !d_q_lm || !d_q_kind || !d_q_aa || !d_cam5 || !d_poses || !d_lms || !d_blocks ||
            !d_cross18 || !d_lmcov9 || !d_z3 || !d_cov9)
            throw std::invalid_argument("cugo_predict_observations: null argument");
        if (n < 0 || n_landmarks_free < 0)
            throw std::invalid_argument("cugo_predict_observations: negative count");
        if (n == 0)
            return;
        cugo_k::launch_predict_obs(ctx->stream, n, n_landmarks_free, d_q_pose, d_q_lm, d_q_kind, d_q_aa, d_cam5, d_cam_tab,
                                   d_poses, d_lms, d_blocks, d_cross18, d_lmcov9, d_z3, d_cov9);
        CUGO_HIP(hipGetLastError());
    });
}
#ifdef CUGO_DEBUG_HOOKS // diagnosis entry points: only libcugo_hip_hooks.so exports them (csrc/host/cugo_debug.h)
int cugo_debug_pin_reference(void)
{
    return guarded([&] { cugo_debug_pin_reference_solver(); });
}
int cugo_debug_dump_call(int which, int call, const char* path)
{
    return guarded([&] {
        cugo_chol* s = cugo_debug_solver(which);
        if (!s)
            throw std::runtime_error("cugo_debug_dump_call: no solver has run with CUGO_DEBUG_KEEP");
        s->dump_slot(call, path);
    });
}
int cugo_debug_plan_array(int which, const char* name, const int32_t** out)
{
    cugo_chol* s = cugo_debug_solver(which);
    if (!s)
        return -1;
    return cugo_chol_plan_array(s, name, out);
}
int cugo_debug_dump(const char* dir, int* n_calls)
{
    return guarded([&] {
        const int n = cugo_debug_dump_last_solver(dir);
        if (n_calls)
            *n_calls = n;
    });
}
#endif
int cugo_chol_stats(const cugo_chol* s, double* nnzL, double* flops, int* n_super, int* n_stages,
                    double* front_bytes)
{
    if (nnzL)
        *nnzL = s->plan.nnzL;
    if (flops)
        *flops = s->plan.flops;
    if (n_super)
        *n_super = s->plan.n_super;
    if (n_stages)
        *n_stages = s->plan.n_stages;
    if (front_bytes)
        *front_bytes = 8.0 * (double)s->plan.front_doubles;
    return CUGO_OK;
}
int cugo_chol_plan_sizes(const cugo_chol* s, int* n, int* n_super, int* n_rows_total)
{
    *n = s->plan.n;
    *n_super = s->plan.n_super;
    *n_rows_total = (int)s->plan.rows.size();
    return CUGO_OK;
}
int cugo_chol_plan_get(const cugo_chol* s, int32_t* perm, int32_t* super_ptr, int32_t* rows_ptr,
                       int32_t* rows, int32_t* parent)
{
    const CholPlan& P = s->plan;
    std::memcpy(perm, P.perm.data(), sizeof(int32_t) * P.perm.size());
    std::memcpy(super_ptr, P.super_ptr.data(), sizeof(int32_t) * P.super_ptr.size());
    std::memcpy(rows_ptr, P.rows_ptr.data(), sizeof(int32_t) * P.rows_ptr.size());
    std::memcpy(rows, P.rows.data(), sizeof(int32_t) * P.rows.size());
    std::memcpy(parent, P.sparent.data(), sizeof(int32_t) * P.sparent.size());
    return CUGO_OK;
}

int cugo_chol_plan_array(cugo_chol* s, const char* name, const int32_t** out)
{
    const CholPlan& P = s->plan;
    const std::string n(name);
    const std::vector<int32_t>* v = nullptr;
#define CUGO_PLAN_FIELD(f) \
    if (n == #f)           \
    v = &P.f
    CUGO_PLAN_FIELD(perm);
    CUGO_PLAN_FIELD(super_ptr);
    CUGO_PLAN_FIELD(rows_ptr);
    CUGO_PLAN_FIELD(rows);
    CUGO_PLAN_FIELD(sparent);
    CUGO_PLAN_FIELD(child_ptr);
    CUGO_PLAN_FIELD(child);
    CUGO_PLAN_FIELD(rel_ptr);
    CUGO_PLAN_FIELD(rel);
    CUGO_PLAN_FIELD(ncb);
    CUGO_PLAN_FIELD(nb);
    CUGO_PLAN_FIELD(col0);
    CUGO_PLAN_FIELD(col_front);
    CUGO_PLAN_FIELD(stage_task_ptr);
    CUGO_PLAN_FIELD(stage_tile);
    CUGO_PLAN_FIELD(task_ptr);
    CUGO_PLAN_FIELD(task_fronts);
    CUGO_PLAN_FIELD(blk_front);
    CUGO_PLAN_FIELD(blk_row);
    CUGO_PLAN_FIELD(blk_col);
    CUGO_PLAN_FIELD(alias_of);
    CUGO_PLAN_FIELD(asm_map);
    CUGO_PLAN_FIELD(wl);
    CUGO_PLAN_FIELD(bc_front);
    CUGO_PLAN_FIELD(bc_seg_ptr);
    CUGO_PLAN_FIELD(bc_seg);
#undef CUGO_PLAN_FIELD
    if (n == "asm_info")
    { // [first assembly item in wl, items, then per front: offset of its map in asm_map or -1]
        s->asm_info.assign(1, P.asm0);
        s->asm_info.push_back(P.nasm);
        for (int64_t o : P.asm_off)
            s->asm_info.push_back((int32_t)o);
        v = &s->asm_info;
    }
    if (n == "blk_trans")
        v = &s->trans32;
    if (n == "ea1") // kernels.h: CholPlanDev::ea1, EA1_REC ints per child link, fronts in order, children in child order
        v = &s->ea1;
    if (!v)
    {
        set_last_error("cugo_chol_plan_array: unknown array " + n);
        return CUGO_ERR_INVALID;
    }
    *out = v->data();
    return (int)v->size();
}

int cugo_chol_plan_array64(cugo_chol* s, const char* name, const int64_t** out)
{
    const CholPlan& P = s->plan;
    const std::string n(name);
    const std::vector<int64_t>* v = n == "off" ? &P.off : n == "ldf" ? &P.ldf : n == "woff" ? &P.woff
                                  : n == "l21off" ? &P.l21off : nullptr;
    if (!v)
    {
        set_last_error("cugo_chol_plan_array64: unknown array " + n);
        return CUGO_ERR_INVALID;
    }
    *out = v->data();
    return (int)v->size();
}

int cugo_shard_range(int n_landmarks_total, const int32_t* edges_per_landmark, int rank, int world,
                     int* l0, int* l1)
{
    return guarded([&] {
        if (world < 1 || rank < 0 || rank >= world)
            throw std::runtime_error("cugo_shard_range: bad rank/world");
        std::vector<int32_t> cnt(n_landmarks_total + 1, 0);
        for (int l = 0; l < n_landmarks_total; l++)
            cnt[l + 1] = cnt[l] + edges_per_landmark[l];
        shard_range(cnt, rank, world, *l0, *l1);
    });
}

// ---------------------------------------------------------------- graph level ----------
struct cugo_graph
{
    cugo::GraphOptimisationOptions options;
    std::unique_ptr<cugo::CudaGraphOptimisationImpl> opt;
    cugo::PoseVertexSet poses{false};
    cugo::LandmarkVertexSet lms{true};
    cugo::MonoEdgeSet mono;
    cugo::StereoEdgeSet stereo;
    cugo::PlaneEdgeSet plane;
    cugo::LineEdgeSet line;
    cugo::PosePriorEdgeSet prior;
    std::deque<cugo::PosePriorEdge> prior_store;
    cugo::RelPoseEdgeSet relpose;
    std::deque<cugo::RelPoseEdge> relpose_store;
    cugo::LandmarkPriorEdgeSet lm_prior;
    std::deque<cugo::LandmarkPriorEdge> lm_prior_store;
    std::deque<cugo::PlaneEdge> plane_store;
    std::deque<cugo::LineEdge> line_store;
    std::deque<cugo::PoseVertex> pose_store;
    std::deque<cugo::LandmarkVertex> lm_store;
    std::deque<cugo::MonoEdge> mono_store;
    std::deque<cugo::StereoEdge> stereo_store;
    cugo::DepthEdgeSet depth;
    std::deque<cugo::DepthEdge> depth_store;
    cugo::PointEdgeSet point;
    std::deque<cugo::PointEdge> point_store;
    cugo::PointPairEdgeSet point_pair;
    std::deque<cugo::PointPairEdge> point_pair_store;
    cugo::GicpEdgeSet gicp;
    std::deque<cugo::GicpEdge> gicp_store;
    cugo::GicpPairEdgeSet gicp_pair;
    std::deque<cugo::GicpPairEdge> gicp_pair_store;
    bool attached = false;
    void attach()
    {
        if (attached)
            return;
        opt->addVertexSet(&poses);
        opt->addVertexSet(&lms);
        opt->addEdgeSet(&mono);
        opt->addEdgeSet(&stereo);
        opt->addEdgeSet(&plane);
        opt->addEdgeSet(&line);
        opt->addEdgeSet(&prior);
        opt->addEdgeSet(&relpose);
        opt->addEdgeSet(&lm_prior);
        opt->addEdgeSet(&depth); // (behind the others: the indices of the other sets in messages stay what they were)
        opt->addEdgeSet(&point); // (likewise)
        opt->addEdgeSet(&point_pair);
        opt->addEdgeSet(&gicp); // (gicp_types.h: empty sets count for nothing)
        opt->addEdgeSet(&gicp_pair);
        attached = true;
    }
};

int cugo_graph_create(int per_edge_information, int per_edge_camera, cugo_graph** out)
{
    return guarded([&] {
        auto g = std::make_unique<cugo_graph>();
        g->options.perEdgeInformation = per_edge_information != 0;
        g->options.perEdgeCamera = per_edge_camera != 0;
        g->options.relativePoseEdges = true; // (only cugo_graph_add_relpose_edges fills the set)
        g->opt = std::make_unique<cugo::CudaGraphOptimisationImpl>(g->options);
        *out = g.release();
    });
}
struct cugo_hsc_plan
{
    cugo_host::SchurPlanDevice dev;
};
int cugo_hsc_plan_create(cugo_ctx* ctx, int n_edges, int n_poses_free, const int32_t* h_pose, const int32_t* h_lm,
                         const uint8_t* h_flags, const int32_t* h_rowptr, const int32_t* h_colind,
                         cugo_hsc_struct* hs, cugo_hsc_plan** out)
{
    int rc = guarded([&] {
        if (!ctx || !hs || !out)
            throw std::runtime_error("cugo_hsc_plan_create: null argument");
        *out = nullptr;
        cugo_host::SchurPlanDevice::clear(*hs);
        cugo_host::SchurPlanHost h;
        cugo_host::build_schur_plan(n_edges, n_poses_free, h_pose, h_lm, h_flags, h_rowptr, h_colind, h);
        if (!h.usable)
            throw std::invalid_argument("cugo_hsc_plan_create: a landmark's active edges straddle two 256-slot groups");
        auto p = std::make_unique<cugo_hsc_plan>();
        p->dev.upload(h, ctx->stream);
        p->dev.fill(*hs);
        *out = p.release();
    });
    return rc;
}
void cugo_hsc_plan_destroy(cugo_hsc_plan* plan) { delete plan; }

int cugo_graph_create_plan_only(int per_edge_information, int per_edge_camera, cugo_graph** out)
{
    return guarded([&] {
        auto g = std::make_unique<cugo_graph>();
        g->options.perEdgeInformation = per_edge_information != 0;
        g->options.perEdgeCamera = per_edge_camera != 0;
        g->options.planOnly = true;
        g->options.relativePoseEdges = true; // (only cugo_graph_add_relpose_edges fills the set)
        g->opt = std::make_unique<cugo::CudaGraphOptimisationImpl>(g->options);
        *out = g.release();
    });
}
void cugo_graph_destroy(cugo_graph* g) { delete g; }

int cugo_graph_add_poses(cugo_graph* g, int n, const int32_t* ids, const double* qt, const uint8_t* fixed)
{
    return guarded([&] {
        for (int i = 0; i < n; i++)
        {
            g->pose_store.emplace_back(ids[i], cugo::Se3D(qt + 7 * (size_t)i, qt + 7 * (size_t)i + 4),
                                       fixed && fixed[i]);
            g->poses.addVertex(&g->pose_store.back());
        }
    });
}
int cugo_graph_add_landmarks(cugo_graph* g, int n, const int32_t* ids, const double* xyz,
                             const uint8_t* fixed)
{
    return guarded([&] {
        for (int i = 0; i < n; i++)
        {
            g->lm_store.emplace_back(ids[i], cugo::Vec3d(xyz + 3 * (size_t)i), fixed && fixed[i]);
            g->lms.addVertex(&g->lm_store.back());
        }
    });
}
// (k1, k2, k3, k4, model) -> CameraModel; who names the entry point in the message
static cugo::CameraModel camera_model_of(const char* who, const double* k4, double model)
{
    if (model != 0.0 && model != 1.0)
        throw std::runtime_error(std::string(who) + ": model must be 0 (pinhole) or 1 (Kannala-Brandt)");
    cugo::CameraModel m;
    m.type = model != 0.0 ? cugo::KannalaBrandt : cugo::Pinhole;
    for (int c = 0; c < 4; c++)
        m.k[c] = k4 ? k4[c] : 0.0;
    return m;
}
// mono / stereo edges; ext7 [n][7]: a sensor pose (q, t) per edge, or NULL (the set's applies); model5 [n][5]: a
// projection model (k1..k4, type) per edge, or NULL (likewise); dist5 [n][5]: a lens distortion (k1, k2, p1, p2, k3) per
// edge, or NULL (likewise)
static int add_ba_edges(cugo_graph* g, const char* who, int dim, int n, const int32_t* pose_ids, const int32_t* lm_ids,
                        const double* meas, const double* info, const double* cam5, const double* ext7,
                        const double* model5 = nullptr, const double* dist5 = nullptr)
{
    return guarded([&] {
        if (dim != 2 && dim != 3)
            throw std::runtime_error(std::string(who) + ": dim must be 2 or 3");
        for (int i = 0; i < n; i++)
        {
            cugo::PoseVertex* vp = g->poses.getVertex(pose_ids[i]);
            cugo::LandmarkVertex* vl = g->lms.getVertex(lm_ids[i]);
            cugo::Se3D ext;
            if (ext7)
                ext = cugo::Se3D(ext7 + 7 * (size_t)i, ext7 + 7 * (size_t)i + 4);
            cugo::CameraModel model;
            if (model5)
                model = camera_model_of(who, model5 + 5 * (size_t)i, model5[5 * (size_t)i + 4]);
            cugo::CameraDistortion dist;
            if (dist5)
            {
                const double* d = dist5 + 5 * (size_t)i;
                dist = cugo::CameraDistortion(d[0], d[1], d[2], d[3], d[4]);
            }
            cugo::Camera cam;
            if (cam5)
                cam = cugo::Camera(cam5[5 * (size_t)i], cam5[5 * (size_t)i + 1], cam5[5 * (size_t)i + 2],
                                   cam5[5 * (size_t)i + 3], cam5[5 * (size_t)i + 4]);
            if (dim == 2)
            {
                g->mono_store.emplace_back();
                cugo::MonoEdge& e = g->mono_store.back();
                e.setVertex(vp, 0), e.setVertex(vl, 1);
                e.setMeasurement(cugo::Vec2d(meas + 2 * (size_t)i));
                e.setInformation(info ? info[i] : 0.0);
                if (cam5)
                    e.setCamera(cam);
                if (ext7)
                    e.setSensorPose(ext);
                if (model5)
                    e.setCameraModel(model);
                if (dist5)
                    e.setDistortion(dist);
                g->mono.addEdge(&e);
            }
            else
            {
                g->stereo_store.emplace_back();
                cugo::StereoEdge& e = g->stereo_store.back();
                e.setVertex(vp, 0), e.setVertex(vl, 1);
                e.setMeasurement(cugo::Vec3d(meas + 3 * (size_t)i));
                e.setInformation(info ? info[i] : 0.0);
                if (cam5)
                    e.setCamera(cam);
                if (ext7)
                    e.setSensorPose(ext);
                if (model5)
                    e.setCameraModel(model);
                if (dist5)
                    e.setDistortion(dist);
                g->stereo.addEdge(&e);
            }
        }
    });
}
int cugo_graph_add_edges(cugo_graph* g, int dim, int n, const int32_t* pose_ids, const int32_t* lm_ids,
                         const double* meas, const double* info, const double* cam5)
{
    return add_ba_edges(g, "cugo_graph_add_edges", dim, n, pose_ids, lm_ids, meas, info, cam5, nullptr);
}
int cugo_graph_add_edges_rig(cugo_graph* g, int dim, int n, const int32_t* pose_ids, const int32_t* lm_ids,
                             const double* meas, const double* info, const double* cam5, const double* sensor_q_t7)
{
    return add_ba_edges(g, "cugo_graph_add_edges_rig", dim, n, pose_ids, lm_ids, meas, info, cam5, sensor_q_t7);
}
int cugo_graph_set_sensor_pose(cugo_graph* g, int dim, const double* q_t7)
{
    return guarded([&] {
        if ((dim != 2 && dim != 3) || !q_t7)
            throw std::runtime_error("cugo_graph_set_sensor_pose: dim must be 2 or 3 and q_t7 not NULL");
        const cugo::Se3D T(q_t7, q_t7 + 4);
        if (dim == 3)
            g->stereo.setSensorPose(T);
        else
            g->mono.setSensorPose(T);
    });
}
int cugo_graph_add_edges_model(cugo_graph* g, int dim, int n, const int32_t* pose_ids, const int32_t* lm_ids,
                               const double* meas, const double* info, const double* cam5, const double* sensor_q_t7,
                               const double* model_k5)
{
    return add_ba_edges(g, "cugo_graph_add_edges_model", dim, n, pose_ids, lm_ids, meas, info, cam5, sensor_q_t7, model_k5);
}
int cugo_graph_set_camera_model(cugo_graph* g, int dim, int model, const double* k4)
{
    return guarded([&] {
        if (dim != 2 && dim != 3)
            throw std::runtime_error("cugo_graph_set_camera_model: dim must be 2 or 3");
        const cugo::CameraModel m = camera_model_of("cugo_graph_set_camera_model", k4, (double)model);
        if (dim == 3)
            g->stereo.setCameraModel(m);
        else
            g->mono.setCameraModel(m);
    });
}
int cugo_graph_n_fisheye_cameras(cugo_graph* g)
{
    int n = -1;
    const int rc = guarded([&] { n = g->opt->nFisheyeCameras(); });
    return rc == CUGO_OK ? n : rc;
}
int cugo_graph_get_flat_camera_models(cugo_graph* g, int cap, double* model_k5)
{
    int n = -1;
    const int rc = guarded([&] {
        std::vector<double> m;
        g->opt->flatCameraModels(m);
        n = (int)(m.size() / 5);
        if (model_k5)
            std::copy(m.begin(), m.begin() + 5 * (size_t)std::min(n, std::max(cap, 0)), model_k5);
    });
    return rc == CUGO_OK ? n : rc;
}
int cugo_graph_add_edges_distorted(cugo_graph* g, int dim, int n, const int32_t* pose_ids, const int32_t* lm_ids,
                                   const double* meas, const double* info, const double* cam5, const double* sensor_q_t7,
                                   const double* dist5)
{
    return add_ba_edges(g, "cugo_graph_add_edges_distorted", dim, n, pose_ids, lm_ids, meas, info, cam5, sensor_q_t7,
                        nullptr, dist5);
}
int cugo_graph_set_camera_distortion(cugo_graph* g, int dim, const double* d5)
{
    return guarded([&] {
        if (dim != 2 && dim != 3)
            throw std::runtime_error("cugo_graph_set_camera_distortion: dim must be 2 or 3");
        const cugo::CameraDistortion d = d5 ? cugo::CameraDistortion(d5[0], d5[1], d5[2], d5[3], d5[4]) : cugo::CameraDistortion();
        if (dim == 3)
            g->stereo.setDistortion(d);
        else
            g->mono.setDistortion(d);
    });
}
int cugo_graph_n_distorted_cameras(cugo_graph* g)
{
    int n = -1;
    const int rc = guarded([&] { n = g->opt->nDistortedCameras(); });
    return rc == CUGO_OK ? n : rc;
}
int cugo_graph_get_flat_camera_distortions(cugo_graph* g, int cap, double* dist5)
{
    int n = -1;
    const int rc = guarded([&] {
        std::vector<double> d;
        g->opt->flatCameraDistortions(d);
        n = (int)(d.size() / 5);
        if (dist5)
            std::copy(d.begin(), d.begin() + 5 * (size_t)std::min(n, std::max(cap, 0)), dist5);
    });
    return rc == CUGO_OK ? n : rc;
}
int cugo_graph_n_rig_cameras(cugo_graph* g)
{
    int n = -1;
    const int rc = guarded([&] { n = g->opt->nRigCameras(); });
    return rc == CUGO_OK ? n : rc;
}
int cugo_graph_get_flat_cameras(cugo_graph* g, int cap, double* cam5, double* ext12, int* has_rig)
{
    int n = -1;
    const int rc = guarded([&] {
        std::vector<double> c, x;
        const bool rig = g->opt->flatCameras(c, x);
        n = (int)(c.size() / 5);
        for (int i = 0; i < n && i < cap; i++)
        {
            if (cam5)
                std::copy(c.begin() + 5 * (size_t)i, c.begin() + 5 * (size_t)i + 5, cam5 + 5 * (size_t)i);
            if (ext12)
                std::copy(x.begin() + 12 * (size_t)i, x.begin() + 12 * (size_t)i + 12, ext12 + 12 * (size_t)i);
        }
        if (has_rig)
            *has_rig = rig ? 1 : 0;
    });
    return rc == CUGO_OK ? n : rc;
}
int cugo_graph_add_depth_edges(cugo_graph* g, int n, const int32_t* pose_ids, const int32_t* lm_ids, const double* meas3,
                               const double* info, const double* cam5)
{
    return guarded([&] {
        if (n < 0 || (n > 0 && (!pose_ids || !lm_ids || !meas3)))
            throw std::invalid_argument("cugo_graph_add_depth_edges: missing arrays");
        for (int i = 0; i < n; i++)
        {
            cugo::PoseVertex* vp = g->poses.getVertex(pose_ids[i]);
            cugo::LandmarkVertex* vl = g->lms.getVertex(lm_ids[i]);
            g->depth_store.emplace_back();
            cugo::DepthEdge& e = g->depth_store.back();
            e.setVertex(vp, 0), e.setVertex(vl, 1);
            e.setMeasurement(cugo::Vec3d(meas3 + 3 * (size_t)i));
            e.setInformation(info ? info[i] : 0.0);
            if (cam5)
                e.setCamera(cugo::Camera(cam5[5 * (size_t)i], cam5[5 * (size_t)i + 1], cam5[5 * (size_t)i + 2],
                                         cam5[5 * (size_t)i + 3], cam5[5 * (size_t)i + 4]));
            g->depth.addEdge(&e);
        }
    });
}
static cugo::RobustKernelType rk_type_of(int type)
{
    return type == CUGO_RK_CAUCHY  ? cugo::RobustKernelType::Cauchy
           : type == CUGO_RK_TUKEY ? cugo::RobustKernelType::Tukey
           : type == CUGO_RK_HUBER ? cugo::RobustKernelType::Huber
                                   : cugo::RobustKernelType::None;
}
static cugo::PoseVertex* icp_pose(cugo_graph* g, int32_t id)
{
    try
    {
        return g->poses.getVertex(id);
    }
    catch (const std::out_of_range&)
    {
        throw std::invalid_argument("cugo_graph_add_*_edges: unknown pose id " + std::to_string(id));
    }
}
int cugo_graph_add_plane_edges(cugo_graph* g, int n, const int32_t* pose_ids, const double* pointP,
                               const double* normal, const double* origin_distance, const double* info)
{
    return guarded([&] {
        if (n < 0 || (n > 0 && (!pose_ids || !pointP || !normal || !origin_distance)))
            throw std::invalid_argument("cugo_graph_add_plane_edges: missing arrays");
        for (int i = 0; i < n; i++)
            (void)icp_pose(g, pose_ids[i]); // (all or nothing: an unknown id adds no edge)
        for (int i = 0; i < n; i++)
        {
            g->plane_store.emplace_back();
            cugo::PlaneEdge& e = g->plane_store.back();
            e.setVertex(icp_pose(g, pose_ids[i]), 0);
            e.setMeasurement(cugo::PointToPlaneMatch<double>(cugo::Vec3d(normal + 3 * (size_t)i), origin_distance[i],
                                                             cugo::Vec3d(pointP + 3 * (size_t)i)));
            e.setInformation(info ? info[i] : 0.0);
            g->plane.addEdge(&e);
        }
    });
}
int cugo_graph_add_line_edges(cugo_graph* g, int n, const int32_t* pose_ids, const double* pointP, const double* a,
                              const double* b, const double* info)
{
    return guarded([&] {
        if (n < 0 || (n > 0 && (!pose_ids || !pointP || !a || !b)))
            throw std::invalid_argument("cugo_graph_add_line_edges: missing arrays");
        for (int i = 0; i < n; i++)
            (void)icp_pose(g, pose_ids[i]);
        for (int i = 0; i < n; i++)
        {
            g->line_store.emplace_back();
            cugo::LineEdge& e = g->line_store.back();
            e.setVertex(icp_pose(g, pose_ids[i]), 0);
            cugo::PointToLineMatch<double> mz(cugo::Vec3d(a + 3 * (size_t)i), cugo::Vec3d(b + 3 * (size_t)i));
            mz.pointP = cugo::Vec3d(pointP + 3 * (size_t)i);
            e.setMeasurement(mz);
            e.setInformation(info ? info[i] : 0.0);
            g->line.addEdge(&e);
        }
    });
}
static cugo::BaseEdgeSet* icp_set(cugo_graph* g, int kind)
{
    if (kind == CUGO_ICP_PLANE)
        return &g->plane;
    if (kind == CUGO_ICP_LINE)
        return &g->line;
    throw std::invalid_argument("cugo: kind must be CUGO_ICP_PLANE (0) or CUGO_ICP_LINE (1)");
}
int cugo_graph_set_icp_information(cugo_graph* g, int kind, double info)
{
    return guarded([&] { icp_set(g, kind)->setInformation(info); });
}
int cugo_graph_set_icp_robust_kernel(cugo_graph* g, int kind, int type, double delta)
{
    return guarded([&] {
        icp_set(g, kind)->setRobustKernel(rk_type_of(type), delta);
    });
}
int cugo_graph_set_icp_outlier_threshold(cugo_graph* g, int kind, double threshold)
{
    return guarded([&] {
        if (kind == CUGO_ICP_PLANE)
            g->plane.setOutlierThreshold(threshold);
        else if (kind == CUGO_ICP_LINE)
            g->line.setOutlierThreshold(threshold);
        else
            icp_set(g, kind);
    });
}
int cugo_graph_n_icp_edges(cugo_graph* g, int kind)
{
    return kind == CUGO_ICP_PLANE || kind == CUGO_ICP_LINE ? g->opt->nIcpEdges(kind) : -1;
}
// the body of cugo_graph_add_pose_priors (binary false: no ids_b) and of cugo_graph_add_relpose_edges: all or nothing
extern "C++" {
template <class Edge, class Set>
static void add_se3_edges(cugo_graph* g, const char* who, std::deque<Edge>& store, Set& set, int n, const int32_t* ids_a,
                          const int32_t* ids_b, bool binary, const double* q_t7, const double* info36)
{
    if (n < 0 || (n > 0 && (!ids_a || (binary && !ids_b) || !q_t7)))
        throw std::invalid_argument(std::string(who) + ": missing arrays");
    for (int i = 0; i < n; i++) // (an unknown id adds no edge)
    {
        (void)icp_pose(g, ids_a[i]);
        if (binary)
            (void)icp_pose(g, ids_b[i]);
    }
    for (int i = 0; i < n; i++)
    {
        store.emplace_back();
        Edge& e = store.back();
        e.setVertex(icp_pose(g, ids_a[i]), 0);
        if (binary)
            e.setVertex(icp_pose(g, ids_b[i]), 1);
        const cugo::Se3D z(q_t7 + 7 * (size_t)i, q_t7 + 7 * (size_t)i + 4);
        e.setMeasurement(cugo::PosePriorMatch<double>(z, info36 ? info36 + 36 * (size_t)i : set.informationMatrix()));
        set.addEdge(&e);
    }
}
}
int cugo_graph_add_pose_priors(cugo_graph* g, int n, const int32_t* pose_ids, const double* q_t7, const double* info36)
{
    return guarded([&] {
        add_se3_edges(g, "cugo_graph_add_pose_priors", g->prior_store, g->prior, n, pose_ids, nullptr, false, q_t7, info36);
    });
}
int cugo_graph_add_relpose_edges(cugo_graph* g, int n, const int32_t* pose_ids_a, const int32_t* pose_ids_b,
                                 const double* q_t7, const double* info36)
{
    return guarded([&] {
        add_se3_edges(g, "cugo_graph_add_relpose_edges", g->relpose_store, g->relpose, n, pose_ids_a, pose_ids_b, true, q_t7,
                      info36);
    });
}
static cugo::BaseEdgeSet* pose_kind_set(cugo_graph* g, int kind)
{
    if (!g)
        throw std::invalid_argument("cugo: null graph");
    switch (kind)
    {
    case CUGO_POSE_KIND_PLANE: return &g->plane;
    case CUGO_POSE_KIND_LINE: return &g->line;
    case CUGO_POSE_KIND_PRIOR: return &g->prior;
    case CUGO_POSE_KIND_RELPOSE: return &g->relpose;
    }
    throw std::invalid_argument("cugo: kind must be one of CUGO_POSE_KIND_PLANE (0), _LINE (1), _PRIOR (2), _RELPOSE (3)");
}
int cugo_graph_set_prior_information(cugo_graph* g, const double* info36)
{
    return guarded([&] {
        if (!info36)
            throw std::invalid_argument("cugo_graph_set_prior_information: no matrix");
        g->prior.setInformationMatrix(info36);
    });
}
int cugo_graph_set_relpose_information(cugo_graph* g, const double* info36)
{
    return guarded([&] {
        if (!info36)
            throw std::invalid_argument("cugo_graph_set_relpose_information: no matrix");
        g->relpose.setInformationMatrix(info36);
    });
}
int cugo_graph_set_prior_robust_kernel(cugo_graph* g, int type, double delta)
{
    return guarded([&] { pose_kind_set(g, CUGO_POSE_KIND_PRIOR)->setRobustKernel(rk_type_of(type), delta); });
}
int cugo_graph_set_relpose_robust_kernel(cugo_graph* g, int type, double delta)
{
    return guarded([&] { pose_kind_set(g, CUGO_POSE_KIND_RELPOSE)->setRobustKernel(rk_type_of(type), delta); });
}
int cugo_graph_set_prior_outlier_threshold(cugo_graph* g, double threshold)
{
    return guarded([&] { g->prior.setOutlierThreshold(threshold); });
}
int cugo_graph_set_relpose_outlier_threshold(cugo_graph* g, double threshold)
{
    return guarded([&] { g->relpose.setOutlierThreshold(threshold); });
}
int cugo_graph_n_prior_edges(cugo_graph* g) { return g->opt->nPriorEdges(); }
int cugo_graph_set_relpose_active(cugo_graph* g, int first, int n, const uint8_t* active)
{
    return guarded([&] {
        if (first < 0 || n < 0 || (size_t)first + (size_t)n > g->relpose_store.size() || (n > 0 && !active))
            throw std::invalid_argument("cugo_graph_set_relpose_active: bad edge range or no flags");
        for (int i = 0; i < n; i++)
            active[i] ? g->relpose_store[(size_t)first + i].setActive() : g->relpose_store[(size_t)first + i].inactivate();
    });
}
int cugo_graph_n_relpose_edges(cugo_graph* g) { return g->opt->nRelPoseEdges(); }
int cugo_graph_add_landmark_priors(cugo_graph* g, int n, const int32_t* lm_ids, const double* xyz3, const double* info9)
{
    return guarded([&] {
        if (n < 0 || (n > 0 && (!lm_ids || !xyz3)))
            throw std::invalid_argument("cugo_graph_add_landmark_priors: missing arrays");
        auto landmark = [&](int32_t id) {
            try
            {
                return g->lms.getVertex(id);
            }
            catch (const std::out_of_range&)
            {
                throw std::invalid_argument("cugo_graph_add_landmark_priors: unknown landmark id " + std::to_string(id));
            }
        };
        for (int i = 0; i < n; i++) // (all or nothing: an unknown id adds no edge)
            (void)landmark(lm_ids[i]);
        for (int i = 0; i < n; i++)
        {
            g->lm_prior_store.emplace_back();
            cugo::LandmarkPriorEdge& e = g->lm_prior_store.back();
            e.setVertex(landmark(lm_ids[i]), 0);
            e.setMeasurement(cugo::LandmarkPriorMatch<double>(xyz3 + 3 * (size_t)i,
                                                              info9 ? info9 + 9 * (size_t)i : g->lm_prior.informationMatrix()));
            g->lm_prior.addEdge(&e);
        }
    });
}
int cugo_graph_set_landmark_prior_information(cugo_graph* g, const double* info9)
{
    return guarded([&] {
        if (!info9)
            throw std::invalid_argument("cugo_graph_set_landmark_prior_information: no matrix");
        g->lm_prior.setInformationMatrix(info9);
    });
}
int cugo_graph_set_landmark_prior_robust_kernel(cugo_graph* g, int type, double delta)
{
    return guarded([&] { g->lm_prior.setRobustKernel(rk_type_of(type), delta); });
}
int cugo_graph_n_landmark_prior_edges(cugo_graph* g) { return g->opt->nLandmarkPriorEdges(); }
int cugo_graph_add_point_edges(cugo_graph* g, int n, const int32_t* pose_ids, const double* pointP, const double* pointZ,
                               const double* info9)
{
    return guarded([&] {
        if (n < 0 || (n > 0 && (!pose_ids || !pointP || !pointZ)))
            throw std::invalid_argument("cugo_graph_add_point_edges: missing arrays");
        for (int i = 0; i < n; i++) // (all or nothing: an unknown id adds no edge)
            (void)icp_pose(g, pose_ids[i]);
        for (int i = 0; i < n; i++)
        {
            g->point_store.emplace_back();
            cugo::PointEdge& e = g->point_store.back();
            e.setVertex(icp_pose(g, pose_ids[i]), 0);
            e.setMeasurement(cugo::PointToPointMatch<double>(pointP + 3 * (size_t)i, pointZ + 3 * (size_t)i,
                                                             info9 ? info9 + 9 * (size_t)i : g->point.informationMatrix()));
            g->point.addEdge(&e);
        }
    });
}
int cugo_graph_set_point_information(cugo_graph* g, const double* info9)
{
    return guarded([&] {
        if (!info9)
            throw std::invalid_argument("cugo_graph_set_point_information: no matrix");
        g->point.setInformationMatrix(info9);
    });
}
int cugo_graph_set_point_robust_kernel(cugo_graph* g, int type, double delta)
{
    return guarded([&] { g->point.setRobustKernel(rk_type_of(type), delta); });
}
int cugo_graph_n_point_edges(cugo_graph* g) { return g->opt->nPointEdges(); }
int cugo_graph_get_flat_point_edges(cugo_graph* g, int cap, int32_t* pose, int32_t* src_edge, double* p, double* z,
                                    double* info, int* n_info)
{
    int n = -1;
    const int rc = guarded([&] {
        std::vector<int> q, s;
        std::vector<double> vp, vz, vi;
        const int ni = g->opt->flatPointEdges(q, s, vp, vz, vi);
        n = (int)q.size();
        if (n_info)
            *n_info = ni;
        if (cap < n)
            return;
        if (pose)
            std::copy(q.begin(), q.end(), pose);
        if (src_edge)
            std::copy(s.begin(), s.end(), src_edge);
        if (p)
            std::copy(vp.begin(), vp.end(), p);
        if (z)
            std::copy(vz.begin(), vz.end(), z);
        if (info && n > 0)
            std::copy(vi.begin(), vi.end(), info);
    });
    return rc == CUGO_OK ? n : rc;
}
int cugo_graph_add_point_pair_edges(cugo_graph* g, int n, const int32_t* pose_ids_a, const int32_t* pose_ids_b,
                                    const double* pointP, const double* pointZ, const double* info9)
{
    return guarded([&] {
        if (n < 0 || (n > 0 && (!pose_ids_a || !pose_ids_b || !pointP || !pointZ)))
            throw std::invalid_argument("cugo_graph_add_point_pair_edges: missing arrays");
        for (int i = 0; i < n; i++) // (all or nothing: an unknown id or a == b adds no edge)
        {
            (void)icp_pose(g, pose_ids_a[i]), (void)icp_pose(g, pose_ids_b[i]);
            if (pose_ids_a[i] == pose_ids_b[i])
                throw std::invalid_argument("cugo_graph_add_point_pair_edges: edge " + std::to_string(i) + " joins pose " +
                                            std::to_string(pose_ids_a[i]) + " to itself (a == b)");
        }
        for (int i = 0; i < n; i++)
        {
            g->point_pair_store.emplace_back();
            cugo::PointPairEdge& e = g->point_pair_store.back();
            e.setVertex(icp_pose(g, pose_ids_a[i]), 0);
            e.setVertex(icp_pose(g, pose_ids_b[i]), 1);
            e.setMeasurement(cugo::PointToPointMatch<double>(pointP + 3 * (size_t)i, pointZ + 3 * (size_t)i,
                                                             info9 ? info9 + 9 * (size_t)i : g->point_pair.informationMatrix()));
            g->point_pair.addEdge(&e);
        }
    });
}
int cugo_graph_set_point_pair_information(cugo_graph* g, const double* info9)
{
    return guarded([&] {
        if (!info9)
            throw std::invalid_argument("cugo_graph_set_point_pair_information: no matrix");
        g->point_pair.setInformationMatrix(info9);
    });
}
int cugo_graph_set_point_pair_robust_kernel(cugo_graph* g, int type, double delta)
{
    return guarded([&] { g->point_pair.setRobustKernel(rk_type_of(type), delta); });
}
int cugo_graph_set_point_pair_outlier_threshold(cugo_graph* g, double threshold)
{
    return guarded([&] { g->point_pair.setOutlierThreshold(threshold); });
}
int cugo_graph_set_point_pair_active(cugo_graph* g, int first, int n, const uint8_t* active)
{
    return guarded([&] {
        if (first < 0 || n < 0 || (size_t)first + (size_t)n > g->point_pair_store.size() || (n > 0 && !active))
            throw std::invalid_argument("cugo_graph_set_point_pair_active: bad edge range or no flags");
        for (int i = 0; i < n; i++)
            active[i] ? g->point_pair_store[(size_t)first + i].setActive() : g->point_pair_store[(size_t)first + i].inactivate();
    });
}
int cugo_graph_n_point_pair_edges(cugo_graph* g) { return g->opt->nPointPairEdges(); }
int cugo_graph_get_flat_point_pair_edges(cugo_graph* g, int cap, int32_t* pose_a, int32_t* pose_b, int32_t* src_edge, double* p,
                                         double* z, double* info, int* n_info)
{
    int n = -1;
    const int rc = guarded([&] {
        std::vector<int> a, b, s;
        std::vector<double> vp, vz, vi;
        const int ni = g->opt->flatPointPairEdges(a, b, s, vp, vz, vi);
        n = (int)a.size();
        if (n_info)
            *n_info = ni;
        if (cap < n)
            return;
        if (pose_a)
            std::copy(a.begin(), a.end(), pose_a);
        if (pose_b)
            std::copy(b.begin(), b.end(), pose_b);
        if (src_edge)
            std::copy(s.begin(), s.end(), src_edge);
        if (p)
            std::copy(vp.begin(), vp.end(), p);
        if (z)
            std::copy(vz.begin(), vz.end(), z);
        if (info && n > 0)
            std::copy(vi.begin(), vi.end(), info);
    });
    return rc == CUGO_OK ? n : rc;
}
int cugo_graph_add_gicp_edges(cugo_graph* g, int n, const int32_t* pose_ids, const double* pointP, const double* pointZ,
                              const double* covP9, const double* covZ9)
{
    return guarded([&] {
        if (n < 0 || (n > 0 && (!pose_ids || !pointP || !pointZ || !covP9 || !covZ9)))
            throw std::invalid_argument("cugo_graph_add_gicp_edges: missing arrays");
        for (int i = 0; i < n; i++) // (all or nothing: an unknown id adds no edge)
            (void)icp_pose(g, pose_ids[i]);
        for (int i = 0; i < n; i++)
        {
            g->gicp_store.emplace_back();
            cugo::GicpEdge& e = g->gicp_store.back();
            e.setVertex(icp_pose(g, pose_ids[i]), 0);
            e.setMeasurement(cugo::PointCovarianceMatch<double>(pointP + 3 * (size_t)i, pointZ + 3 * (size_t)i, covP9 + 9 * (size_t)i,
                                                                covZ9 + 9 * (size_t)i));
            g->gicp.addEdge(&e);
        }
    });
}
int cugo_graph_add_gicp_pair_edges(cugo_graph* g, int n, const int32_t* pose_ids_a, const int32_t* pose_ids_b, const double* pointP,
                                   const double* pointZ, const double* covP9, const double* covZ9)
{
    return guarded([&] {
        if (n < 0 || (n > 0 && (!pose_ids_a || !pose_ids_b || !pointP || !pointZ || !covP9 || !covZ9)))
            throw std::invalid_argument("cugo_graph_add_gicp_pair_edges: missing arrays");
        for (int i = 0; i < n; i++) // (all or nothing: an unknown id or a == b adds no edge)
        {
            (void)icp_pose(g, pose_ids_a[i]), (void)icp_pose(g, pose_ids_b[i]);
            if (pose_ids_a[i] == pose_ids_b[i])
                throw std::invalid_argument("cugo_graph_add_gicp_pair_edges: edge " + std::to_string(i) + " joins pose " +
                                            std::to_string(pose_ids_a[i]) + " to itself (a == b)");
        }
        for (int i = 0; i < n; i++)
        {
            g->gicp_pair_store.emplace_back();
            cugo::GicpPairEdge& e = g->gicp_pair_store.back();
            e.setVertex(icp_pose(g, pose_ids_a[i]), 0);
            e.setVertex(icp_pose(g, pose_ids_b[i]), 1);
            e.setMeasurement(cugo::PointCovarianceMatch<double>(pointP + 3 * (size_t)i, pointZ + 3 * (size_t)i, covP9 + 9 * (size_t)i,
                                                                covZ9 + 9 * (size_t)i));
            g->gicp_pair.addEdge(&e);
        }
    });
}
int cugo_graph_set_gicp_robust_kernel(cugo_graph* g, int type, double delta)
{
    return guarded([&] { g->gicp.setRobustKernel(rk_type_of(type), delta); });
}
int cugo_graph_set_gicp_pair_robust_kernel(cugo_graph* g, int type, double delta)
{
    return guarded([&] { g->gicp_pair.setRobustKernel(rk_type_of(type), delta); });
}
int cugo_graph_set_gicp_outlier_threshold(cugo_graph* g, double threshold)
{
    return guarded([&] { g->gicp.setOutlierThreshold(threshold); });
}
int cugo_graph_set_gicp_pair_outlier_threshold(cugo_graph* g, double threshold)
{
    return guarded([&] { g->gicp_pair.setOutlierThreshold(threshold); });
}
int cugo_graph_set_gicp_pair_active(cugo_graph* g, int first, int n, const uint8_t* active)
{
    return guarded([&] {
        if (first < 0 || n < 0 || (size_t)first + (size_t)n > g->gicp_pair_store.size() || (n > 0 && !active))
            throw std::invalid_argument("cugo_graph_set_gicp_pair_active: bad edge range or no flags");
        for (int i = 0; i < n; i++)
            active[i] ? g->gicp_pair_store[(size_t)first + i].setActive() : g->gicp_pair_store[(size_t)first + i].inactivate();
    });
}
int cugo_graph_n_gicp_edges(cugo_graph* g) { return g->opt->nGicpEdges(); }
int cugo_graph_n_gicp_pair_edges(cugo_graph* g) { return g->opt->nGicpPairEdges(); }
int cugo_graph_get_flat_gicp_edges(cugo_graph* g, int cap, int32_t* pose, int32_t* src_edge, double* p, double* z, double* cov_p,
                                   double* cov_z, int* n_cov)
{
    int n = -1;
    const int rc = guarded([&] {
        std::vector<int> q, s;
        std::vector<double> vp, vz, cp, cz;
        const int nc = g->opt->flatGicpEdges(q, s, vp, vz, cp, cz);
        n = (int)q.size();
        if (n_cov)
            *n_cov = nc;
        if (cap < n)
            return;
        if (pose)
            std::copy(q.begin(), q.end(), pose);
        if (src_edge)
            std::copy(s.begin(), s.end(), src_edge);
        if (p)
            std::copy(vp.begin(), vp.end(), p);
        if (z)
            std::copy(vz.begin(), vz.end(), z);
        if (cov_p)
            std::copy(cp.begin(), cp.end(), cov_p);
        if (cov_z)
            std::copy(cz.begin(), cz.end(), cov_z);
    });
    return rc == CUGO_OK ? n : rc;
}
int cugo_graph_get_flat_gicp_pair_edges(cugo_graph* g, int cap, int32_t* pose_a, int32_t* pose_b, int32_t* src_edge, double* p,
                                        double* z, double* cov_p, double* cov_z, int* n_cov)
{
    int n = -1;
    const int rc = guarded([&] {
        std::vector<int> a, b, s;
        std::vector<double> vp, vz, cp, cz;
        const int nc = g->opt->flatGicpPairEdges(a, b, s, vp, vz, cp, cz);
        n = (int)a.size();
        if (n_cov)
            *n_cov = nc;
        if (cap < n)
            return;
        if (pose_a)
            std::copy(a.begin(), a.end(), pose_a);
        if (pose_b)
            std::copy(b.begin(), b.end(), pose_b);
        if (src_edge)
            std::copy(s.begin(), s.end(), src_edge);
        if (p)
            std::copy(vp.begin(), vp.end(), p);
        if (z)
            std::copy(vz.begin(), vz.end(), z);
        if (cov_p)
            std::copy(cp.begin(), cp.end(), cov_p);
        if (cov_z)
            std::copy(cz.begin(), cz.end(), cov_z);
    });
    return rc == CUGO_OK ? n : rc;
}
int cugo_graph_set_camera(cugo_graph* g, int dim, const double* c)
{
    const cugo::Camera cam(c[0], c[1], c[2], c[3], c[4]);
    if (dim == 3)
        g->stereo.setCamera(cam);
    else
        g->mono.setCamera(cam);
    return CUGO_OK;
}
int cugo_graph_set_information(cugo_graph* g, int dim, double info)
{
    if (dim == 3)
        g->stereo.setInformation(info);
    else
        g->mono.setInformation(info);
    return CUGO_OK;
}
int cugo_graph_set_robust_kernel(cugo_graph* g, int dim, int type, double delta)
{
    if (dim == 3)
        g->stereo.setRobustKernel(rk_type_of(type), delta);
    else
        g->mono.setRobustKernel(rk_type_of(type), delta);
    return CUGO_OK;
}
int cugo_graph_set_outlier_threshold(cugo_graph* g, int dim, double threshold)
{
    if (dim == 3)
        g->stereo.setOutlierThreshold(threshold);
    else
        g->mono.setOutlierThreshold(threshold);
    return CUGO_OK;
}
int cugo_graph_n_outliers(cugo_graph* g, int dim)
{
    return (int)(dim == 3 ? g->stereo.getOutlierCount() : g->mono.getOutlierCount());
}
int cugo_graph_get_edge_active(cugo_graph* g, int dim, int n, uint8_t* active)
{
    return guarded([&] {
        if (dim == 3)
            for (int i = 0; i < n && i < (int)g->stereo_store.size(); i++)
                active[i] = g->stereo_store[i].isActive() ? 1 : 0;
        else
            for (int i = 0; i < n && i < (int)g->mono_store.size(); i++)
                active[i] = g->mono_store[i].isActive() ? 1 : 0;
    });
}
// the depth edge set: the dim-keyed functions above keep meaning mono (2) and stereo (3)
int cugo_graph_set_depth_camera(cugo_graph* g, const double* c)
{
    g->depth.setCamera(cugo::Camera(c[0], c[1], c[2], c[3], c[4]));
    return CUGO_OK;
}
int cugo_graph_set_depth_information(cugo_graph* g, double info)
{
    g->depth.setInformation(info);
    return CUGO_OK;
}
int cugo_graph_set_depth_robust_kernel(cugo_graph* g, int type, double delta)
{
    g->depth.setRobustKernel(rk_type_of(type), delta);
    return CUGO_OK;
}
int cugo_graph_set_depth_outlier_threshold(cugo_graph* g, double threshold)
{
    g->depth.setOutlierThreshold(threshold);
    return CUGO_OK;
}
int cugo_graph_set_depth_weight(cugo_graph* g, double weight)
{
    g->depth.setInverseDepthWeight(weight); // (checked by initialize())
    return CUGO_OK;
}
int cugo_graph_n_depth_outliers(cugo_graph* g) { return (int)g->depth.getOutlierCount(); }
int cugo_graph_get_depth_edge_active(cugo_graph* g, int n, uint8_t* active)
{
    return guarded([&] {
        for (int i = 0; i < n && i < (int)g->depth_store.size(); i++)
            active[i] = g->depth_store[i].isActive() ? 1 : 0;
    });
}
int cugo_graph_get_flat_edges(cugo_graph* g, int cap, int32_t* pose, int32_t* landmark, uint8_t* flags, double* meas3,
                              int* has_depth, double* depth_weight)
{
    int n = -1;
    const int rc = guarded([&] {
        std::vector<int> p, l;
        std::vector<unsigned char> f;
        std::vector<double> m;
        g->opt->flatEdges(p, l, f, m);
        n = (int)p.size();
        for (int i = 0; i < n && i < cap; i++)
        {
            if (pose)
                pose[i] = p[i];
            if (landmark)
                landmark[i] = l[i];
            if (flags)
                flags[i] = f[i];
            if (meas3)
                std::copy(m.begin() + 3 * (size_t)i, m.begin() + 3 * (size_t)i + 3, meas3 + 3 * (size_t)i);
        }
        double w = 1.0;
        const bool d = g->opt->flatDepth(w);
        if (has_depth)
            *has_depth = d ? 1 : 0;
        if (depth_weight)
            *depth_weight = w;
    });
    return rc == CUGO_OK ? n : rc;
}
int cugo_graph_n_pose_edge_outliers(cugo_graph* g, int kind)
{
    int n = -1;
    const int rc = guarded([&] { n = (int)pose_kind_set(g, kind)->getOutlierCount(); });
    return rc == CUGO_OK ? n : rc;
}
int cugo_graph_get_pose_edge_active(cugo_graph* g, int kind, int n, uint8_t* active)
{
    return guarded([&] {
        (void)pose_kind_set(g, kind);
        if (n < 0 || (n > 0 && !active))
            throw std::invalid_argument("cugo_graph_get_pose_edge_active: bad count or no array");
        auto fill = [&](const auto& store) {
            if ((size_t)n > store.size())
                throw std::invalid_argument("cugo_graph_get_pose_edge_active: the set holds fewer edges");
            for (int i = 0; i < n; i++)
                active[i] = store[(size_t)i].isActive() ? 1 : 0;
        };
        kind == CUGO_POSE_KIND_PLANE  ? fill(g->plane_store)
        : kind == CUGO_POSE_KIND_LINE ? fill(g->line_store)
        : kind == CUGO_POSE_KIND_PRIOR ? fill(g->prior_store)
                                       : fill(g->relpose_store);
    });
}
int cugo_graph_set_shard(cugo_graph* g, int rank, int world, cugo_exchange_fn fn, void* user)
{
    return guarded([&] { g->opt->setShard(rank, world, fn, user); });
}
int cugo_comm_unique_id(void* id128)
{
    return guarded([&] {
        if (!id128)
            throw std::runtime_error("cugo_comm_unique_id: null buffer");
        cugo_host::RcclComm::unique_id(id128);
    });
}
struct cugo_comm
{
    std::shared_ptr<cugo_host::RcclComm> c;
};
int cugo_comm_create(const void* id128, int rank, int world, cugo_comm** out)
{
    return guarded([&] {
        if (!id128 || !out || world < 1 || rank < 0 || rank >= world)
            throw std::runtime_error("cugo_comm_create: bad arguments");
        auto* h = new cugo_comm;
        try
        {
            h->c = std::make_shared<cugo_host::RcclComm>(id128, rank, world);
        }
        catch (...)
        {
            delete h;
            throw;
        }
        *out = h;
    });
}
void cugo_comm_destroy(cugo_comm* comm) { delete comm; }
int cugo_graph_set_comm(cugo_graph* g, cugo_comm* comm)
{
    return guarded([&] {
        if (!comm)
            throw std::runtime_error("cugo_graph_set_comm: null communicator");
        g->opt->setComm(comm->c);
    });
}
int cugo_graph_exchange_stats(cugo_graph* g, double* bytes, int32_t* calls)
{
    return guarded([&] {
        int c = 0;
        double b = 0;
        g->opt->exchangeStats(b, c);
        if (bytes)
            *bytes = b;
        if (calls)
            *calls = c;
    });
}
int cugo_set_device(int device)
{
    return guarded([&] { CUGO_HIP(hipSetDevice(device)); });
}
int cugo_graph_initialize(cugo_graph* g)
{
    return guarded([&] {
        g->attach();
        g->opt->initialize();
    });
}
int cugo_graph_flatten_reuses(cugo_graph* g)
{
    int n = -1;
    if (guarded([&] {
            if (!g)
                throw std::runtime_error("cugo_graph_flatten_reuses: null graph");
            n = g->opt->flattenReuses();
        }) != 0)
        return -1;
    return n;
}
int cugo_graph_set_option(cugo_graph* g, const char* name, int value)
{
    return guarded([&] {
        if (!g || !g->opt->setOption(name, value))
            throw std::invalid_argument(std::string("cugo_graph_set_option: unknown option ") + (name ? name : "(null)"));
    });
}
int cugo_graph_optimize(cugo_graph* g, int n_iters)
{
    return guarded([&] { g->opt->optimize(n_iters); });
}
int cugo_graph_n_stats(cugo_graph* g) { return (int)g->opt->batchStatistics().get().size(); }
int cugo_graph_get_stats(cugo_graph* g, int32_t* iteration, double* chi2, int cap)
{
    const auto& st = g->opt->batchStatistics().get();
    int n = 0;
    for (; n < (int)st.size() && n < cap; n++)
    {
        iteration[n] = st[n].iteration;
        chi2[n] = st[n].chi2;
    }
    return n;
}
int cugo_graph_get_trace(cugo_graph* g, double* lambda, double* rho, int32_t* trials, int cap)
{
    const auto& tr = g->opt->lmTrace();
    int n = 0;
    for (; n < (int)tr.size() && n < cap; n++)
    {
        lambda[n] = tr[n].lambda;
        rho[n] = tr[n].rho;
        trials[n] = tr[n].trials;
    }
    return n;
}
int cugo_graph_get_poses(cugo_graph* g, int n, const int32_t* ids, double* qt)
{
    return guarded([&] {
        for (int i = 0; i < n; i++)
        {
            const cugo::Se3D& e = g->poses.getVertex(ids[i])->getEstimate();
            e.copyTo(qt + 7 * (size_t)i, qt + 7 * (size_t)i + 4);
        }
    });
}
int cugo_graph_get_landmarks(cugo_graph* g, int n, const int32_t* ids, double* xyz)
{
    return guarded([&] {
        for (int i = 0; i < n; i++)
            g->lms.getVertex(ids[i])->getEstimate().copyTo(xyz + 3 * (size_t)i);
    });
}
int cugo_graph_compute_covariances(cugo_graph* g, int what)
{
    bool ok = true;
    const int rc = guarded([&] {
        if (what < 1 || what > 3)
            throw std::invalid_argument("cugo_graph_compute_covariances: what must be 1 (poses), 2 (landmarks) or 3 (both)");
        ok = g->opt->computeMarginals((what & 1) != 0, (what & 2) != 0);
    });
    if (rc != CUGO_OK)
        return rc;
    if (!ok)
    {
        set_last_error("cugo_graph_compute_covariances: zero pivot — H is singular at the current estimates (an "
                       "unconstrained gauge, a free pose without edges or a landmark seen too little)");
        return CUGO_ERR_NUMERIC;
    }
    return CUGO_OK;
}
int cugo_graph_get_pose_covariances(cugo_graph* g, int n, const int32_t* ids, double* cov36)
{
    return guarded([&] {
        for (int i = 0; i < n; i++)
            if (!g->opt->poseCovariance(g->poses.getVertex(ids[i]), cov36 + 36 * (size_t)i))
                throw std::runtime_error("cugo_graph_get_pose_covariances: no pose covariances were computed since the "
                                         "last initialize(), or the pose set changed since then");
    });
}
int cugo_graph_get_landmark_covariances(cugo_graph* g, int n, const int32_t* ids, double* cov9)
{
    return guarded([&] {
        for (int i = 0; i < n; i++)
            if (!g->opt->landmarkCovariance(g->lms.getVertex(ids[i]), cov9 + 9 * (size_t)i))
                throw std::runtime_error("cugo_graph_get_landmark_covariances: no landmark covariances were computed "
                                         "since the last initialize(), or the landmark set changed since then");
    });
}
namespace
{
// Sigma_ab of the pose pairs by caller id; CUGO_ERR_NUMERIC on a zero pivot
int pose_cross_blocks(cugo_graph* g, const char* who, int n, const int32_t* ids_a, const int32_t* ids_b, double* cov36)
{
    bool ok = true;
    const int rc = guarded([&] {
        if (n < 0)
            throw std::invalid_argument(std::string(who) + ": negative count");
        std::vector<const cugo::BaseVertex*> a(n), b(n);
        for (int i = 0; i < n; i++)
            a[i] = g->poses.getVertex(ids_a[i]), b[i] = g->poses.getVertex(ids_b[i]);
        ok = g->opt->poseCrossCovariances(n, a.data(), b.data(), cov36);
    });
    if (rc != CUGO_OK)
        return rc;
    if (!ok)
    {
        set_last_error(std::string(who) + ": zero pivot — H is singular at the current estimates");
        return CUGO_ERR_NUMERIC;
    }
    return CUGO_OK;
}

// Ad(A) of A = T_a T_b^-1 (row-major 6 x 6, tangent order [rotation, translation]): [ R 0 ; [t]x R  R ]
void relative_adjoint(const cugo::Se3D& Ta, const cugo::Se3D& Tb, double (&Ad)[6][6])
{
    auto rot = [](const cugo::Se3D& T, double (&R)[3][3]) {
        double q[4], t[3];
        T.copyTo(q, t);
        const double x = q[0], y = q[1], z = q[2], w = q[3];
        R[0][0] = 1 - 2 * (y * y + z * z), R[0][1] = 2 * (x * y - z * w), R[0][2] = 2 * (x * z + y * w);
        R[1][0] = 2 * (x * y + z * w), R[1][1] = 1 - 2 * (x * x + z * z), R[1][2] = 2 * (y * z - x * w);
        R[2][0] = 2 * (x * z - y * w), R[2][1] = 2 * (y * z + x * w), R[2][2] = 1 - 2 * (x * x + y * y);
    };
    double Ra[3][3], Rb[3][3], R[3][3], qa[4], ta[3], qb[4], tb[3], t[3];
    rot(Ta, Ra), rot(Tb, Rb);
    Ta.copyTo(qa, ta), Tb.copyTo(qb, tb);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            R[i][j] = Ra[i][0] * Rb[j][0] + Ra[i][1] * Rb[j][1] + Ra[i][2] * Rb[j][2]; // R_a R_b^T
    for (int i = 0; i < 3; i++)
        t[i] = ta[i] - (R[i][0] * tb[0] + R[i][1] * tb[1] + R[i][2] * tb[2]); // t_a - R t_b
    const double tx[3][3] = {{0, -t[2], t[1]}, {t[2], 0, -t[0]}, {-t[1], t[0], 0}};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
        {
            Ad[i][j] = Ad[3 + i][3 + j] = R[i][j];
            Ad[i][3 + j] = 0.0;
            Ad[3 + i][j] = tx[i][0] * R[0][j] + tx[i][1] * R[1][j] + tx[i][2] * R[2][j];
        }
}
} // namespace

int cugo_graph_compute_pose_cross_covariances(cugo_graph* g, int n, const int32_t* ids_a, const int32_t* ids_b,
                                              double* cov36)
{
    return pose_cross_blocks(g, "cugo_graph_compute_pose_cross_covariances", n, ids_a, ids_b, cov36);
}

namespace
{
// the two pose-landmark calls by caller id; CUGO_ERR_NUMERIC on a zero pivot or a queried landmark whose Hll fails
using PoseLandmarkFn = std::function<bool(const cugo::BaseVertex* const*, const cugo::BaseVertex* const*)>;
int pose_landmark_call(cugo_graph* g, const char* who, int n, const int32_t* pose_ids, const int32_t* lm_ids,
                       const PoseLandmarkFn& call)
{
    bool ok = true;
    const int rc = guarded([&] {
        if (!g)
            throw std::invalid_argument(std::string(who) + ": null argument");
        if (n < 0)
            throw std::invalid_argument(std::string(who) + ": negative count");
        if (n > 0 && (!pose_ids || !lm_ids))
            throw std::invalid_argument(std::string(who) + ": null argument");
        std::vector<const cugo::BaseVertex*> p(n), l(n);
        for (int i = 0; i < n; i++)
            p[i] = g->poses.getVertex(pose_ids[i]), l[i] = g->lms.getVertex(lm_ids[i]);
        ok = call(p.data(), l.data());
    });
    if (rc != CUGO_OK)
        return rc;
    if (!ok)
    {
        set_last_error(std::string(who) + ": zero pivot — H is singular at the current estimates, or a queried landmark "
                                          "has no active edge");
        return CUGO_ERR_NUMERIC;
    }
    return CUGO_OK;
}
} // namespace

int cugo_graph_compute_pose_landmark_cross_covariances(cugo_graph* g, int n, const int32_t* pose_ids,
                                                       const int32_t* lm_ids, double* cov18)
{
    return pose_landmark_call(g, "cugo_graph_compute_pose_landmark_cross_covariances", n, pose_ids, lm_ids,
                              [&](const cugo::BaseVertex* const* p, const cugo::BaseVertex* const* l) {
                                  return g->opt->poseLandmarkCrossCovariances(n, p, l, cov18);
                              });
}

int cugo_graph_reprojection_covariances(cugo_graph* g, int n, const int32_t* pose_ids, const int32_t* lm_ids, int dim,
                                        const double* cam5, double* cov)
{
    return pose_landmark_call(g, "cugo_graph_reprojection_covariances", n, pose_ids, lm_ids,
                              [&](const cugo::BaseVertex* const* p, const cugo::BaseVertex* const* l) {
                                  if (dim != 2 && dim != 3)
                                      throw std::invalid_argument("cugo_graph_reprojection_covariances: dim must be 2 "
                                                                  "(mono) or 3 (stereo)");
                                  if (cam5)
                                      return g->opt->reprojectionCovariances(n, p, l, dim, cam5, n, cov);
                                  // the camera of the edge set of that dim (cugo_graph_set_camera)
                                  const cugo::Camera& c = dim == 3 ? g->stereo.getCamera() : g->mono.getCamera();
                                  const double set5[5] = {c.fx, c.fy, c.cx, c.cy, c.bf};
                                  return g->opt->reprojectionCovariances(n, p, l, dim, set5, 1, cov);
                              });
}

int cugo_graph_predict_observations(cugo_graph* g, int n, const int32_t* pose_ids, const int32_t* lm_ids, int kind,
                                    const double* cam5, const double* sensor_q_t7, const double* model_k5, double* z,
                                    double* cov)
{
    const char* who = "cugo_graph_predict_observations";
    return pose_landmark_call(g, who, n, pose_ids, lm_ids,
                              [&](const cugo::BaseVertex* const* p, const cugo::BaseVertex* const* l) {
        if (kind != CUGO_OBS_MONO && kind != CUGO_OBS_STEREO && kind != CUGO_OBS_DEPTH)
            throw std::invalid_argument(std::string(who) + ": kind must be 2 (mono), 3 (stereo) or 4 (depth)");
        if (!cam5)
        {
            // the camera, sensor pose and model of the edge set of that kind
            if (sensor_q_t7 || model_k5)
                throw std::invalid_argument(std::string(who) + ": sensor_q_t7 and model_k5 must be NULL where cam5 is "
                                                               "(the set's camera brings its own)");
            const cugo::BaseEdgeSet& es = kind == CUGO_OBS_DEPTH    ? static_cast<const cugo::BaseEdgeSet&>(g->depth)
                                          : kind == CUGO_OBS_STEREO ? static_cast<const cugo::BaseEdgeSet&>(g->stereo)
                                                                    : static_cast<const cugo::BaseEdgeSet&>(g->mono);
            // (answering for the undistorted camera would be silently wrong; a distorted kind is a later step)
            if (!es.distortionData().isZero())
                throw std::invalid_argument(std::string(who) + ": the set's camera has lens distortion (radial-tangential), "
                                                               "which predicted observations do not model yet");
            const cugo::Camera& c = es.cameraData();
            const double set5[5] = {c.fx, c.fy, c.cx, c.cy, c.bf};
            const cugo::Se3D T = es.sensorPoseData();
            const cugo::CameraModel m = es.cameraModelData();
            return g->opt->predictObservations(n, p, l, kind, set5, 1, &T, &m, z, cov);
        }
        std::vector<cugo::Se3D> T;
        std::vector<cugo::CameraModel> m;
        for (int i = 0; sensor_q_t7 && i < n; i++)
            T.emplace_back(sensor_q_t7 + 7 * (size_t)i, sensor_q_t7 + 7 * (size_t)i + 4);
        for (int i = 0; model_k5 && i < n; i++)
        {
            // (the type travels as a double and is judged by predictObservations; the enum holds what it says)
            const double ty = model_k5[5 * (size_t)i + 4];
            if (ty != 0.0 && ty != 1.0)
                throw std::invalid_argument(std::string(who) + ": unknown model type (0 pinhole, 1 Kannala-Brandt)");
            cugo::CameraModel cm;
            cm.type = ty != 0.0 ? cugo::KannalaBrandt : cugo::Pinhole;
            for (int c = 0; c < 4; c++)
                cm.k[c] = model_k5[5 * (size_t)i + c];
            m.push_back(cm);
        }
        return g->opt->predictObservations(n, p, l, kind, cam5, n, sensor_q_t7 ? T.data() : nullptr,
                                           model_k5 ? m.data() : nullptr, z, cov);
    });
}

int cugo_graph_relative_pose_covariances(cugo_graph* g, int n, const int32_t* ids_a, const int32_t* ids_b, double* cov36)
{
    const char* who = "cugo_graph_relative_pose_covariances";
    std::vector<int32_t> qa, qb;
    std::vector<double> blk;
    int rc = guarded([&] {
        if (n < 0)
            throw std::invalid_argument(std::string(who) + ": negative count");
        for (int i = 0; i < n; i++)
        {
            if (ids_a[i] == ids_b[i])
                throw std::invalid_argument(std::string(who) + ": a == b (the relative pose of a pose to itself)");
            // Sigma_aa, Sigma_ab, Sigma_bb of every pair
            qa.insert(qa.end(), {ids_a[i], ids_a[i], ids_b[i]});
            qb.insert(qb.end(), {ids_a[i], ids_b[i], ids_b[i]});
        }
        blk.resize(36 * qa.size());
    });
    if (rc != CUGO_OK)
        return rc;
    rc = pose_cross_blocks(g, who, (int)qa.size(), qa.data(), qb.data(), blk.data());
    if (rc != CUGO_OK)
        return rc;
    return guarded([&] {
        for (int i = 0; i < n; i++)
        {
            double Ad[6][6];
            relative_adjoint(g->poses.getVertex(ids_a[i])->getEstimate(), g->poses.getVertex(ids_b[i])->getEstimate(), Ad);
            // column-major blocks: S(r, c) = S[r + 6 c]
            const double *Saa = blk.data() + 108 * (size_t)i, *Sab = Saa + 36, *Sbb = Saa + 72;
            double M[6][6], N[6][6]; // M = Ad Sigma_ba = Ad Sigma_ab^T, N = Ad Sigma_bb
            for (int r = 0; r < 6; r++)
                for (int c = 0; c < 6; c++)
                {
                    double m = 0.0, nn = 0.0;
                    for (int k = 0; k < 6; k++)
                        m += Ad[r][k] * Sab[c + 6 * k], nn += Ad[r][k] * Sbb[k + 6 * c];
                    M[r][c] = m, N[r][c] = nn;
                }
            double* out = cov36 + 36 * (size_t)i;
            for (int r = 0; r < 6; r++)
                for (int c = 0; c < 6; c++)
                {
                    double v = 0.0;
                    for (int k = 0; k < 6; k++)
                        v += N[r][k] * Ad[c][k];
                    out[r + 6 * c] = Saa[r + 6 * c] - M[c][r] - M[r][c] + v;
                }
        }
    });
}

int cugo_graph_set_poses(cugo_graph* g, int n, const int32_t* ids, const double* qt)
{
    return guarded([&] {
        for (int i = 0; i < n; i++)
            g->poses.getVertex(ids[i])->setEstimate(cugo::Se3D(qt + 7 * (size_t)i, qt + 7 * (size_t)i + 4));
    });
}
int cugo_graph_set_landmarks(cugo_graph* g, int n, const int32_t* ids, const double* xyz)
{
    return guarded([&] {
        for (int i = 0; i < n; i++)
            g->lms.getVertex(ids[i])->setEstimate(cugo::Vec3d(xyz + 3 * (size_t)i));
    });
}
int cugo_graph_n_active_edges(cugo_graph* g) { return g->opt->nActiveEdges(); }
int cugo_graph_time_profile(cugo_graph* g, char* names, int buf_len, double* ms, int cap)
{
    const auto& tp = g->opt->timeProfile();
    std::string all;
    int n = 0;
    for (const auto& kv : tp)
    {
        if (n >= cap)
            break;
        all += kv.first + "\n";
        ms[n++] = kv.second;
    }
    if (names && buf_len > 0)
    {
        std::strncpy(names, all.c_str(), buf_len - 1);
        names[buf_len - 1] = 0;
    }
    return n;
}
int cugo_graph_set_verbose(cugo_graph* g, int v)
{
    g->opt->setVerbose(v != 0);
    return CUGO_OK;
}
int cugo_graph_set_float32(cugo_graph* g, int on)
{
    g->opt->setUseFloat32(on != 0);
    return CUGO_OK;
}
int cugo_graph_set_kernel_timing(cugo_graph* g, int on)
{
    g->opt->setKernelTiming(on);
    return CUGO_OK;
}
int cugo_graph_kernel_times(cugo_graph* g, char* names, int buf_len, double* ms, int32_t* launches, int cap)
{
    std::vector<std::string> nm;
    std::vector<double> t;
    std::vector<int> c;
    g->opt->kernelTimes(nm, t, c);
    std::string all;
    int n = 0;
    for (; n < (int)nm.size() && n < cap; n++)
    {
        all += nm[n] + "\n";
        ms[n] = t[n];
        launches[n] = c[n];
    }
    if (names && buf_len > 0)
    {
        std::strncpy(names, all.c_str(), buf_len - 1);
        names[buf_len - 1] = 0;
    }
    return n;
}
int cugo_memcpy_d2d(cugo_ctx* ctx, void* d, const void* s, size_t bytes)
{
    return guarded([&] {
        CUGO_HIP(hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        CUGO_HIP(hipStreamSynchronize(ctx->stream));
    });
}
int cugo_graph_structure_stats(cugo_graph* g, double* out, int cap)
{
    const auto v = g->opt->structureStats();
    int n = 0;
    for (; n < (int)v.size() && n < cap; n++)
        out[n] = v[n];
    return n;
}

} // extern "C"
