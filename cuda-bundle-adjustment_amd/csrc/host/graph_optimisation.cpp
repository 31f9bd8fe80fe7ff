// CudaGraphOptimisationImpl: flatten the pointer graph, run the engine, write estimates back.
// ref: src/cuda_graph_optimisation.cpp:42-183 (class), src/block_solver.cpp:21-137
// (initialize), src/optimisable_graph.hpp:84-154, 474-572 (index / flag / activeness rules).
#include "../../include/cuda_graph_optimisation.h"
#include "../../include/icp_types.h"
#include "../../include/landmark_prior_types.h"
#include "../../include/point_edge_types.h"
#include "../../include/gicp_types.h"
#include "../../include/point_pair_types.h"
#include "../../include/prior_types.h"
#include "../../include/relpose_types.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <stdexcept>

#include "engine.h"
#include "options.h"
#include "thread_pool.h"

namespace cugo
{

namespace detail
{
unsigned hostPoolThreads()
{
    return cugo_host::pool_threads();
}
void hostPoolRun(unsigned chunks, void (*fn)(void*, unsigned), void* ctx)
{
    cugo_host::pool_run(chunks, fn, ctx);
}
} // namespace detail

using cugo_host::Engine;
using cugo_host::FlatGraph;

CudaGraphOptimisation::~CudaGraphOptimisation() {}

CudaGraphOptimisation::Ptr CudaGraphOptimisation::create()
{
    return std::make_unique<CudaGraphOptimisationImpl>();
}

CudaGraphOptimisationImpl::CudaGraphOptimisationImpl() : engine_(new Engine) {}

CudaGraphOptimisationImpl::CudaGraphOptimisationImpl(GraphOptimisationOptions& opts)
    : options(opts), engine_(new Engine(opts.planOnly))
{
}

CudaGraphOptimisationImpl::~CudaGraphOptimisationImpl() {}

void CudaGraphOptimisationImpl::setShard(int rank, int world, ExchangeFn fn, void* user)
{
    engine_->set_shard(rank, world, fn, user);
    flattenValid_ = false; // slot layout, landmark range and Hsc lists were built for the old rank / world
}

void CudaGraphOptimisationImpl::setComm(std::shared_ptr<cugo_host::RcclComm> comm)
{
    engine_->set_comm(std::move(comm));
    flattenValid_ = false;
}

void CudaGraphOptimisationImpl::exchangeStats(double& bytes, int& calls) const
{
    engine_->exchange_stats(bytes, calls);
}

int CudaGraphOptimisationImpl::nActiveEdges() const { return engine_->n_active_edges(); }
int CudaGraphOptimisationImpl::nIcpEdges(int kind) const { return engine_->n_icp_edges(kind); }
int CudaGraphOptimisationImpl::nPriorEdges() const { return engine_->n_prior_edges(); }
int CudaGraphOptimisationImpl::nRelPoseEdges() const { return engine_->n_relpose_edges(); }
int CudaGraphOptimisationImpl::nLandmarkPriorEdges() const { return engine_->n_lm_prior_edges(); }
int CudaGraphOptimisationImpl::nPointEdges() const { return engine_->point_edges_cov() ? 0 : engine_->n_point_edges(); }
int CudaGraphOptimisationImpl::nGicpEdges() const { return engine_->point_edges_cov() ? engine_->n_point_edges() : 0; }
int CudaGraphOptimisationImpl::nGicpPairEdges() const { return engine_->point_pair_edges_cov() ? engine_->n_point_pair_edges() : 0; }
// [12][n_cov] planar (cov_p, then cov_z) -> two [6][n_cov] arrays
static void splitCovariances(const std::vector<double>& w, int n_cov, std::vector<double>& covP, std::vector<double>& covZ)
{
    covP.assign(w.begin(), w.begin() + 6 * (size_t)n_cov);
    covZ.assign(w.begin() + 6 * (size_t)n_cov, w.begin() + 12 * (size_t)n_cov);
}
int CudaGraphOptimisationImpl::flatGicpEdges(std::vector<int>& pose, std::vector<int>& srcEdge, std::vector<double>& p,
                                             std::vector<double>& z, std::vector<double>& covP, std::vector<double>& covZ) const
{
    pose.clear(), srcEdge.clear(), p.clear(), z.clear(), covP.clear(), covZ.clear();
    if (!engine_->point_edges_cov())
        return 0;
    std::vector<int32_t> q, s;
    std::vector<double> w;
    const int n_cov = engine_->flat_point_edges(q, s, p, z, w);
    pose.assign(q.begin(), q.end()), srcEdge.assign(s.begin(), s.end());
    splitCovariances(w, n_cov, covP, covZ);
    return n_cov;
}
int CudaGraphOptimisationImpl::flatGicpPairEdges(std::vector<int>& poseA, std::vector<int>& poseB, std::vector<int>& srcEdge,
                                                 std::vector<double>& p, std::vector<double>& z, std::vector<double>& covP,
                                                 std::vector<double>& covZ) const
{
    poseA.clear(), poseB.clear(), srcEdge.clear(), p.clear(), z.clear(), covP.clear(), covZ.clear();
    if (!engine_->point_pair_edges_cov())
        return 0;
    std::vector<int32_t> a, b, s;
    std::vector<double> w;
    const int n_cov = engine_->flat_point_pair_edges(a, b, s, p, z, w);
    poseA.assign(a.begin(), a.end()), poseB.assign(b.begin(), b.end()), srcEdge.assign(s.begin(), s.end());
    splitCovariances(w, n_cov, covP, covZ);
    return n_cov;
}
int CudaGraphOptimisationImpl::flatPointEdges(std::vector<int>& pose, std::vector<int>& srcEdge, std::vector<double>& p,
                                              std::vector<double>& z, std::vector<double>& info) const
{
    pose.clear(), srcEdge.clear(), p.clear(), z.clear(), info.clear();
    if (engine_->point_edges_cov()) // (the kind holds covariances, [12][n_cov]: flatGicpEdges)
        return 0;
    std::vector<int32_t> q, s;
    const int n_info = engine_->flat_point_edges(q, s, p, z, info);
    pose.assign(q.begin(), q.end()), srcEdge.assign(s.begin(), s.end());
    return n_info;
}
int CudaGraphOptimisationImpl::nPointPairEdges() const { return engine_->point_pair_edges_cov() ? 0 : engine_->n_point_pair_edges(); }
int CudaGraphOptimisationImpl::flatPointPairEdges(std::vector<int>& poseA, std::vector<int>& poseB, std::vector<int>& srcEdge,
                                                  std::vector<double>& p, std::vector<double>& z, std::vector<double>& info) const
{
    poseA.clear(), poseB.clear(), srcEdge.clear(), p.clear(), z.clear(), info.clear();
    if (engine_->point_pair_edges_cov()) // (the kind holds covariances, [12][n_cov]: flatGicpPairEdges)
        return 0;
    std::vector<int32_t> a, b, s;
    const int n_info = engine_->flat_point_pair_edges(a, b, s, p, z, info);
    poseA.assign(a.begin(), a.end()), poseB.assign(b.begin(), b.end()), srcEdge.assign(s.begin(), s.end());
    return n_info;
}
void CudaGraphOptimisationImpl::flatEdges(std::vector<int>& pose, std::vector<int>& landmark,
                                          std::vector<unsigned char>& flags, std::vector<double>& meas3) const
{
    const FlatGraph& g = engine_->staging();
    pose.assign(g.e_pose.begin(), g.e_pose.end());
    landmark.assign(g.e_lm.begin(), g.e_lm.end());
    flags.assign(g.e_flags.begin(), g.e_flags.end());
    meas3 = g.e_meas;
}
bool CudaGraphOptimisationImpl::flatDepth(double& weight) const
{
    const FlatGraph& g = engine_->staging();
    weight = g.depth_weight;
    return g.has_depth;
}

bool CudaGraphOptimisationImpl::flatCameras(std::vector<double>& cam5, std::vector<double>& ext12) const
{
    const FlatGraph& g = engine_->staging();
    static const double I12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    cam5 = g.cams;
    ext12 = g.cam_ext;
    if (!g.has_rig)
        for (size_t k = 0; k < g.cams.size() / 5; k++)
            ext12.insert(ext12.end(), I12, I12 + 12);
    return g.has_rig;
}
bool CudaGraphOptimisationImpl::flatCameraModels(std::vector<double>& model_k5) const
{
    const FlatGraph& g = engine_->staging();
    model_k5 = g.cam_model;
    if (!g.has_models)
        model_k5.assign(5 * (g.cams.size() / 5), 0.0); // (k = 0, type Pinhole)
    return g.has_models;
}
int CudaGraphOptimisationImpl::nFisheyeCameras() const
{
    const FlatGraph& g = engine_->staging();
    int n = 0;
    if (g.has_models)
        for (size_t k = 0; k < g.cam_model.size() / 5; k++)
            n += g.cam_model[5 * k + 4] != 0.0 ? 1 : 0;
    return n;
}
bool CudaGraphOptimisationImpl::flatCameraDistortions(std::vector<double>& dist5) const
{
    const FlatGraph& g = engine_->staging();
    dist5 = g.cam_dist;
    if (!g.has_dist)
        dist5.assign(5 * (g.cams.size() / 5), 0.0);
    return g.has_dist;
}
int CudaGraphOptimisationImpl::nDistortedCameras() const
{
    const FlatGraph& g = engine_->staging();
    int n = 0;
    if (g.has_dist)
        for (size_t k = 0; k < g.cam_dist.size() / 5; k++)
            n += std::any_of(&g.cam_dist[5 * k], &g.cam_dist[5 * k] + 5, [](double c) { return c != 0.0; }) ? 1 : 0;
    return n;
}
int CudaGraphOptimisationImpl::nRigCameras() const
{
    std::vector<double> cams, x;
    if (!flatCameras(cams, x))
        return 0;
    static const double I12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    int n = 0;
    for (size_t k = 0; k < x.size() / 12; k++)
    {
        bool identity = true;
        for (int c = 0; c < 12; c++)
            identity = identity && x[12 * k + c] == I12[c];
        n += identity ? 0 : 1;
    }
    return n;
}

std::vector<double> CudaGraphOptimisationImpl::structureStats() const
{
    const auto& s = engine_->structure_stats();
    return {s.hsc_blocks,     s.products,      s.nnzL,          s.chol_flops,  s.supernodes,
            s.stages,         s.front_bytes,   s.offdiag_products, s.up_potrf_flops,
            s.up_trsm_flops,  s.up_syrk_flops, s.up_ea_bytes,   s.backward_bytes, s.schur_slots,
            s.chol_rank_flops, s.chol_top_flops, s.chol_bcast_bytes, s.chol_bcasts, s.trial_sync_retries,
            s.xchg_sys_bytes, s.xchg_sys_full_bytes};
}

void CudaGraphOptimisationImpl::setKernelTiming(int mode) { engine_->set_kernel_timing(mode); }

bool CudaGraphOptimisationImpl::setOption(const char* name, int value)
{
    cugo_host::Options& o = engine_->options();
    const std::string n = name ? name : "";
    if (n == "flatten_reuse")
        o.flatten_reuse = value != 0;
    else if (n == "structure_reuse")
        o.structure_reuse = value != 0;
    else if (n == "init_timing")
        o.init_timing = value != 0;
    else if (n == "pose_edge_outliers") // (an option of the graph, not of the engine: compared by the next initialize())
        options.poseEdgeOutlierRejection = value != 0;
    else
        return false;
    return true;
}

void CudaGraphOptimisationImpl::kernelTimes(std::vector<std::string>& names, std::vector<double>& ms,
                                            std::vector<int>& launches) const
{
    names.clear(), ms.clear(), launches.clear();
    for (const auto& k : engine_->kernel_times())
    {
        names.push_back(k.name);
        ms.push_back(k.ms);
        launches.push_back(k.launches);
    }
}

static int rk_code(RobustKernelType t)
{
    switch (t)
    {
    case RobustKernelType::Cauchy:
        return CUGO_RK_CAUCHY;
    case RobustKernelType::Tukey:
        return CUGO_RK_TUKEY;
    case RobustKernelType::Huber:
        return CUGO_RK_HUBER;
    default:
        return CUGO_RK_NONE;
    }
}

// smallest and largest eigenvalue of a symmetric N x N matrix by cyclic Jacobi sweeps
template <int N>
static void symEigenRange(const double* A, double& lo, double& hi)
{
    double a[N][N];
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++)
            a[i][j] = 0.5 * (A[N * i + j] + A[N * j + i]);
    for (int sweep = 0; sweep < 30; sweep++)
    {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < N; i++)
            for (int j = 0; j < N; j++)
                (i == j ? diag : off) += a[i][j] * a[i][j];
        if (off <= 1e-32 * diag || off == 0.0)
            break;
        for (int p = 0; p < N - 1; p++)
            for (int q = p + 1; q < N; q++)
            {
                if (a[p][q] == 0.0)
                    continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < N; k++)
                {
                    const double akp = a[k][p], akq = a[k][q];
                    a[k][p] = c * akp - sn * akq, a[k][q] = sn * akp + c * akq;
                }
                for (int k = 0; k < N; k++)
                {
                    const double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c * apk - sn * aqk, a[q][k] = sn * apk + c * aqk;
                }
            }
    }
    lo = hi = a[0][0];
    for (int i = 1; i < N; i++)
        lo = std::min(lo, a[i][i]), hi = std::max(hi, a[i][i]);
}

// nullptr if Omega [N x N] can serve as an information matrix, else what is wrong with it
template <int N>
static const char* checkInformation(const double* A)
{
    double mx = 0.0;
    for (int i = 0; i < N * N; i++)
    {
        if (!std::isfinite(A[i]))
            return "non-finite information";
        mx = std::max(mx, std::fabs(A[i]));
    }
    for (int i = 0; i < N; i++)
        for (int j = i + 1; j < N; j++)
            if (std::fabs(A[N * i + j] - A[N * j + i]) > 1e-12 * mx)
                return "the information matrix is not symmetric";
    double lo, hi;
    symEigenRange<N>(A, lo, hi);
    if (lo < -1e-12 * std::max(hi, 0.0) || hi < 0.0)
        return "the information matrix is not positive semi-definite";
    return nullptr;
}
static const char* checkInformation36(const double* A) { return checkInformation<6>(A); }

// What the pose edge kinds, unary and binary, share per set: the outlier threshold (refused unless
// GraphOptimisationOptions::poseEdgeOutlierRejection is on; returned: finite and > 0, or 0 = no rejection on this set), one
// robust kernel per kind (rk, delta, rk_seen: the kind's record), check_set()
template <class CheckSet>
static double settlePoseEdgeSet(BaseEdgeSet* es, int setIndex, const std::string& name, bool rejection, int& out_rk,
                                double& out_delta, bool& out_rk_seen, CheckSet check_set)
{
    const double set_threshold = es->getOutlierThreshold();
    if (set_threshold > 0.0 && !rejection)
        throw std::runtime_error("cugo: outlier rejection is not available on " + name +
                                 " edge sets yet (setOutlierThreshold must stay 0)");
    const RobustKernel& k = es->robustKernelData();
    const int rk = rk_code(k.type());
    const double delta = k.delta();
    if (es->nedges() > 0)
    {
        if (out_rk_seen && (rk != out_rk || (rk != CUGO_RK_NONE && delta != out_delta)))
            throw std::runtime_error("cugo: the " + name + " edge sets of one optimiser must use the same robust kernel");
        if (!std::isfinite(delta) || (rk != CUGO_RK_NONE && !(delta > 0.0)))
            throw std::runtime_error("cugo: bad robust kernel delta on a " + name + " edge set");
        out_rk = rk, out_delta = delta;
        out_rk_seen = true;
        if (const char* bad = check_set())
            throw std::runtime_error("cugo: " + name + " edge set " + std::to_string(setIndex) + ": " + bad);
    }
    es->setOutlierCount(0);
    return std::isfinite(set_threshold) && set_threshold > 0.0 ? set_threshold : 0.0;
}
// v is a pose vertex of one of the optimiser's pose vertex sets
static bool knownPoseVertex(const BaseVertex* v, const std::vector<BaseVertexSet*>& vertexSets)
{
    bool known = false;
    if (v && !v->isMarginilised())
        for (const BaseVertexSet* vs : vertexSets)
            known = known || (vs == v->ownerSet() && !vs->isMarginilised());
    return known;
}

// One edge set of pose edges (PlaneEdgeSet / LineEdgeSet of icp_types.h, PosePriorEdgeSet of prior_types.h: arity 1;
// RelPoseEdgeSet of relpose_types.h: arity 2, vertex 0 = a, vertex 1 = b) into the flat arrays of its kind, in container
// order.  This is the one place where these edges are checked (the kernels take the layout as given): every active edge
// must sit on pose vertices of the optimiser's pose vertex sets (arity 2: two different ones) and hold what
// payload(e, refuse, meas, weight) accepts; the callable writes the edge's meas_w / weight_w columns and refuses bad
// values through refuse(what).  Inactive edges and edges all of whose poses are fixed are dropped, as BA edges with two
// fixed ends are.  Several sets of a kind must agree on the robust kernel; once that is settled, check_set() returns
// what is wrong with a non-empty set as a whole, or nullptr.
template <class Payload, class CheckSet>
static void flattenPoseEdgeSet(BaseEdgeSet* es, int setIndex, int arity, const char* kind,
                               const std::vector<BaseVertexSet*>& vertexSets, bool rejection, cugo_host::FlatPoseKind& out,
                               std::vector<BaseEdge*>& setEdges, Payload payload, CheckSet check_set)
{
    const std::string name = kind;
    const double threshold = settlePoseEdgeSet(es, setIndex, name, rejection, out.rk, out.delta, out.rk_seen, check_set);
    if (threshold > 0.0) // (a set that can lose edges: where its flattened edges are, by position in the container)
        setEdges.assign(es->nedges(), nullptr);
    size_t i = 0, kept = 0;
    for (BaseEdge* e : es->get())
    {
        const size_t at = i++;
        if (!e->isActive())
            continue;
        auto refuse = [&](const char* what) {
            throw std::runtime_error("cugo: " + name + " edge " + std::to_string(at) + " of edge set " +
                                     std::to_string(setIndex) + ": " + what);
        };
        BaseVertex *v = e->getVertex(0), *vb = arity == 2 ? e->getVertex(1) : nullptr;
        if (!knownPoseVertex(v, vertexSets) || (arity == 2 && !knownPoseVertex(vb, vertexSets)))
            refuse(arity == 2 ? "one of its pose vertices is in no pose vertex set of this optimiser"
                              : "its pose vertex is in no pose vertex set of this optimiser");
        if (v == vb)
            refuse("it joins a pose to itself (a == b)");
        double meas[9], weight[21];
        payload(e, refuse, meas, weight);
        if (v->isFixed() && (arity == 1 || vb->isFixed()))
            continue;
        out.pose.push_back(v->getIndex());
        if (arity == 2)
            out.pose_b.push_back(vb->getIndex());
        out.meas.insert(out.meas.end(), meas, meas + out.meas_w);
        out.weight.insert(out.weight.end(), weight, weight + out.weight_w);
        out.src_set.push_back(setIndex), out.src_edge.push_back((int32_t)at);
        out.threshold.push_back(threshold);
        if (threshold > 0.0)
            setEdges[at] = e;
        kept++;
    }
    es->setActiveEdgeCount(kept);
    es->setDirtyState(false);
}

// The payloads of the kinds: an edge's columns, validated.
// plane / line: one information value, the edge's own or the set's
template <class Refuse>
static void icpInformation(BaseEdgeSet* es, BaseEdge* e, bool perInfo, Refuse& refuse, double* weight)
{
    weight[0] = perInfo ? (double)e->informationValue() : es->informationValue();
    if (!std::isfinite(weight[0]))
        refuse("non-finite information");
}
// plane: p, unit normal ("used as given": refused, not normalised silently), originDistance
template <class Refuse>
static void planePayload(BaseEdge* e, Refuse& refuse, double* m)
{
    const auto& mz = *static_cast<const PointToPlaneMatch<double>*>(e->measurementData());
    for (int c = 0; c < 3; c++)
        m[c] = mz.pointP[c], m[3 + c] = mz.normal[c];
    m[6] = mz.originDistance;
    for (int c = 0; c < 3; c++)
        if (!std::isfinite(m[c]) || !std::isfinite(m[3 + c]))
            refuse("non-finite point or normal");
    if (!std::isfinite(m[6]))
        refuse("non-finite originDistance");
    const double len = std::sqrt(m[3] * m[3] + m[4] * m[4] + m[5] * m[5]);
    if (!(std::fabs(len - 1.0) <= 1e-6))
        refuse("the plane normal is not of unit length (it is used as given)");
}
// line: p, a, unit direction of b - a (two distinct points)
template <class Refuse>
static void linePayload(BaseEdge* e, Refuse& refuse, double* m)
{
    const auto& mz = *static_cast<const PointToLineMatch<double>*>(e->measurementData());
    double d[3];
    for (int c = 0; c < 3; c++)
    {
        m[c] = mz.pointP[c], m[3 + c] = mz.a[c], d[c] = mz.b[c] - mz.a[c];
        if (!std::isfinite(m[c]) || !std::isfinite(mz.a[c]) || !std::isfinite(mz.b[c]))
            refuse("non-finite point or line end");
    }
    const double len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (!(len > 0.0) || !std::isfinite(len))
        refuse("the two points of the line coincide (a == b)");
    for (int c = 0; c < 3; c++)
        m[6 + c] = d[c] / len;
}
// prior and relative pose: measured pose with a unit quaternion | the upper triangle of the symmetric part of Omega (A:
// the edge's own matrix, checked here, or the set's, checked with the set)
template <class Refuse>
static void priorPayload(BaseEdge* e, const double* setInformation, Refuse& refuse, double* z, double* weight)
{
    const auto& mz = *static_cast<const PosePriorMatch<double>*>(e->measurementData());
    mz.pose.copyTo(z, z + 4);
    for (int c = 0; c < 7; c++)
        if (!std::isfinite(z[c]))
            refuse("non-finite measured pose");
    const double len = std::sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2] + z[3] * z[3]);
    if (!(std::fabs(len - 1.0) <= 1e-6))
        refuse("the quaternion of the measured pose is not of unit length (it is used as given)");
    const double* A = setInformation ? setInformation : mz.information;
    if (!setInformation)
        if (const char* bad = checkInformation36(A))
            refuse(bad);
    for (int r = 0, t = 0; r < 6; r++)
        for (int c = r; c < 6; c++)
            weight[t++] = 0.5 * (A[6 * r + c] + A[6 * c + r]);
}

// point-to-point: p, z | the upper triangle of the symmetric part of the 3 x 3 Omega (the edge's own matrix, checked here,
// or the set's, checked with the set)
template <class Refuse>
static void pointPayload(BaseEdge* e, const double* setInformation, Refuse& refuse, double* m, double* weight)
{
    const auto& mz = *static_cast<const PointToPointMatch<double>*>(e->measurementData());
    for (int c = 0; c < 3; c++)
    {
        m[c] = mz.pointP[c], m[3 + c] = mz.pointZ[c];
        if (!std::isfinite(m[c]) || !std::isfinite(m[3 + c]))
            refuse("non-finite point or measured point");
    }
    const double* A = setInformation ? setInformation : mz.information;
    if (!setInformation)
        if (const char* bad = checkInformation<3>(A))
            refuse(bad);
    for (int r = 0, t = 0; r < 3; r++)
        for (int c = r; c < 3; c++)
            weight[t++] = 0.5 * (A[3 * r + c] + A[3 * c + r]);
}

// covariance form (gicp_types.h): p, z | the upper triangles of the symmetric parts of C_p, then C_z.  Each covariance
// symmetric to 1e-12 max|C| and positive semi-definite to -1e-12 lambda_max; lambda_min(C_p) + lambda_min(C_z) >
// 1e-12 (lambda_max(C_p) + lambda_max(C_z)): by Weyl's inequality S = C_z + M C_p M^T is then positive definite for
// every rotation M
template <class Refuse>
static void gicpPayload(BaseEdge* e, Refuse& refuse, double* m, double* weight)
{
    const auto& mz = *static_cast<const PointCovarianceMatch<double>*>(e->measurementData());
    for (int c = 0; c < 3; c++)
    {
        m[c] = mz.pointP[c], m[3 + c] = mz.pointZ[c];
        if (!std::isfinite(m[c]) || !std::isfinite(m[3 + c]))
            refuse("non-finite point or measured point");
    }
    double lo[2], hi[2];
    const double* C[2] = {mz.covP, mz.covZ};
    for (int k = 0; k < 2; k++)
    {
        const double* A = C[k];
        double mx = 0.0;
        for (int i = 0; i < 9; i++)
        {
            if (!std::isfinite(A[i]))
                refuse(k ? "non-finite covariance covZ" : "non-finite covariance covP");
            mx = std::max(mx, std::fabs(A[i]));
        }
        for (int i = 0; i < 3; i++)
            for (int j = i + 1; j < 3; j++)
                if (std::fabs(A[3 * i + j] - A[3 * j + i]) > 1e-12 * mx)
                    refuse(k ? "the covariance covZ is not symmetric" : "the covariance covP is not symmetric");
        symEigenRange<3>(A, lo[k], hi[k]);
        if (lo[k] < -1e-12 * std::max(hi[k], 0.0) || hi[k] < 0.0)
            refuse(k ? "the covariance covZ is not positive semi-definite" : "the covariance covP is not positive semi-definite");
        for (int r = 0, t = 6 * k; r < 3; r++)
            for (int c = r; c < 3; c++)
                weight[t++] = 0.5 * (A[3 * r + c] + A[3 * c + r]);
    }
    if (!(lo[0] + lo[1] > 1e-12 * (hi[0] + hi[1])))
        refuse("covP and covZ are both singular: lambda_min(covP) + lambda_min(covZ) must exceed 1e-12 (lambda_max(covP) + "
               "lambda_max(covZ)) for C_z + M C_p M^T to be positive definite under every rotation");
}

// One LandmarkPriorEdgeSet (landmark_prior_types.h) into the flat arrays, in container order; the one place where these
// edges are checked, as flattenPoseEdgeSet is for the pose kinds.  Every active edge must sit on a landmark vertex of one
// of the optimiser's landmark sets and hold finite values and a symmetric positive semi-definite Omega (its own with
// perEdgeInformation, else the set's).  Inactive priors and priors on fixed landmarks are dropped.  Several sets must
// agree on the robust kernel.  Outlier rejection is not available on this kind.
static void flattenLandmarkPriorSet(LandmarkPriorEdgeSet* es, int setIndex, const std::vector<BaseVertexSet*>& vertexSets,
                                    bool perEdgeInformation, cugo_host::FlatLmPriors& out)
{
    const std::string name = "landmark prior";
    const double* setInformation = perEdgeInformation ? nullptr : es->informationMatrix();
    settlePoseEdgeSet(es, setIndex, name, false, out.rk, out.delta, out.rk_seen,
                      [&] { return setInformation ? checkInformation<3>(setInformation) : nullptr; });
    size_t at = 0, kept = 0;
    for (BaseEdge* e : es->get())
    {
        const size_t i = at++;
        if (!e->isActive())
            continue;
        auto refuse = [&](const char* what) {
            throw std::runtime_error("cugo: " + name + " edge " + std::to_string(i) + " of edge set " +
                                     std::to_string(setIndex) + ": " + what);
        };
        BaseVertex* v = e->getVertex(0);
        bool known = false;
        if (v && v->isMarginilised())
            for (const BaseVertexSet* vs : vertexSets)
                known = known || (vs == v->ownerSet() && vs->isMarginilised());
        if (!known)
            refuse("its landmark vertex is in no landmark vertex set of this optimiser");
        const auto& mz = *static_cast<const LandmarkPriorMatch<double>*>(e->measurementData());
        for (int c = 0; c < 3; c++)
            if (!std::isfinite(mz.point[c]))
                refuse("non-finite measured position");
        const double* A = setInformation ? setInformation : mz.information;
        if (!setInformation)
            if (const char* bad = checkInformation<3>(A))
                refuse(bad);
        if (v->isFixed())
            continue;
        out.lm.push_back(v->getIndex());
        out.meas.insert(out.meas.end(), mz.point, mz.point + 3);
        for (int r = 0; r < 3; r++)
            for (int c = r; c < 3; c++)
                out.info.push_back(0.5 * (A[3 * r + c] + A[3 * c + r]));
        kept++;
    }
    es->setActiveEdgeCount(kept);
    es->setDirtyState(false);
}

void CudaGraphOptimisationImpl::initialize()
{
    if (vertexSets.empty() || edgeSets.empty())
        throw std::runtime_error("cugo: initialize() needs at least one vertex set and one edge set");

    const cugo_host::Options& eopt = engine_->options();
    const bool timing = eopt.init_timing;
    auto lap_t = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!timing)
            return;
        const auto n = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[cugo init] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(n - lap_t).count());
        lap_t = n;
    };
    engine_->set_float32_blocks(options.useFloat32);
    engine_->clear_covariances();
    initialized_ = false;
    FlatGraph& g = engine_->staging();
    // ---- unchanged graph: only the estimates are refreshed -------------------------------
    // If no vertex set or edge set has counted a change since the last full flattening (see
    // "change tracking" in optimisable_graph.h: everything except vertex estimates counts), the
    // flattened, landmark-major graph on the device still is the graph held by these objects.
    // This is the reference fork's isDirty idea (src/block_solver.cpp:151-216 skips the structure
    // rebuild for clean edge sets) carried over to the flattening itself: SLAM back ends — and the
    // reference's own sample, main.cpp:168-190 — call initialize() again on an unchanged graph.
    // CUGO_NO_FLATTEN_REUSE=1 turns it off.
    {
        bool same = flattenValid_ && eopt.flatten_reuse && eopt.structure_reuse &&
                    flattenOptions_[0] == options.perEdgeInformation && flattenOptions_[1] == options.perEdgeCamera &&
                    flattenOptions_[2] == options.useFloat32 && flattenOptions_[3] == options.relativePoseEdges &&
                    flattenOptions_[4] == options.poseEdgeOutlierRejection &&
                    flattenCounts_.size() == vertexSets.size() + edgeSets.size();
        size_t q = 0;
        for (size_t i = 0; same && i < vertexSets.size(); i++, q++)
            same = flattenCounts_[q].first == vertexSets[i] && flattenCounts_[q].second == vertexSets[i]->changeCount();
        for (size_t i = 0; same && i < edgeSets.size(); i++, q++)
            same = flattenCounts_[q].first == edgeSets[i] && flattenCounts_[q].second == edgeSets[i]->changeCount();
        if (same)
        {
            // (straight into the engine's pinned staging: the copy to the device is then a DMA transfer nobody waits
            // for; a plan-only optimiser has no device and no pinned memory)
            double* hp = options.planOnly ? g.poses.data() : engine_->pinned_poses();
            double* hl = options.planOnly ? g.lms.data() : engine_->pinned_lms();
            for (BaseVertexSet* vs : vertexSets)
                vs->gatherEstimates(vs->isMarginilised() ? hl : hp);
            lap("graph: estimates only");
            for (BaseEdgeSet* es : edgeSets)
                es->setOutlierCount(0);
            if (options.planOnly)
                engine_->refresh_estimates(g);
            else
                engine_->refresh_estimates_pinned();
            flattenReuses_++;
            lap("graph: engine refresh");
            stats_.clear();
            trace_.clear();
            initialized_ = true;
            return;
        }
        flattenValid_ = false;
    }
    g.cams.clear();
    g.cam_ext.clear(), g.has_rig = false;
    g.cam_model.clear(), g.has_models = false;
    g.cam_dist.clear(), g.has_dist = false;
    // ---- vertex indices: free first (ascending id), fixed after -------------------------
    int nPfree = 0, nLfree = 0, nP = 0, nL = 0;
    for (BaseVertexSet* vs : vertexSets)
    {
        vs->clearEstimates();
        (vs->isMarginilised() ? nLfree : nPfree) += vs->countFree();
        (vs->isMarginilised() ? nL : nP) += (int)vs->size();
    }
    {
        int pf = 0, px = nPfree, lf = 0, lx = nLfree;
        for (BaseVertexSet* vs : vertexSets)
        {
            int a = 0, b = 0;
            if (!vs->isMarginilised())
            {
                if (vs->estimateDim() != 7)
                    throw std::runtime_error("cugo: pose vertex sets must hold Se3D estimates");
                vs->assignIndices(pf, px, a, b);
                pf += a, px += b;
            }
            else
            {
                if (vs->estimateDim() != 3)
                    throw std::runtime_error("cugo: landmark vertex sets must hold Vec3d estimates");
                vs->assignIndices(lf, lx, a, b);
                lf += a, lx += b;
            }
        }
    }
    g.Pall = nP, g.Lall = nL, g.P = nPfree, g.L = nLfree;
    g.poses.resize(7 * (size_t)nP);
    g.lms.resize(3 * (size_t)nL);
    for (BaseVertexSet* vs : vertexSets)
        vs->gatherEstimates(vs->isMarginilised() ? g.lms.data() : g.poses.data());

    lap("graph: vertices");
    // ---- edges: every edge with at least one free endpoint is active -------------------
    // Walking 561k edge objects through virtual getters is the bulk of initialize(); the walk of
    // each edge set is split over worker threads.  Every thread writes its contiguous chunk
    // straight into the final arrays (sized for all edges up front, so the first touch of the
    // pages is parallel too); chunks with skipped edges are compacted afterwards, in order, so
    // the flattened order is exactly the container order.
    size_t cap = 0;
    g.has_depth = false, g.rk_type_depth = CUGO_RK_NONE, g.rk_delta_depth = 1.0, g.depth_weight = 1.0;
    // (a LandmarkPriorEdgeSet, PointEdgeSet, PointPairEdgeSet, GicpEdgeSet or GicpPairEdgeSet is 3-d like a stereo set: the type
    //  tells them apart)
    for (BaseEdgeSet* es : edgeSets)
        if (es->dim() != 1 && es->dim() != 6 && !dynamic_cast<LandmarkPriorEdgeSet*>(es) && !dynamic_cast<PointEdgeSet*>(es) &&
            !dynamic_cast<PointPairEdgeSet*>(es) && !dynamic_cast<GicpEdgeSet*>(es) && !dynamic_cast<GicpPairEdgeSet*>(es))
            cap += es->nedges();
    for (cugo_host::FlatPoseKind& fk : g.kinds)
        fk.clear();
    g.lm_priors.clear();
    poseSetEdges_.assign(edgeSets.size(), {});
    int pointFormSeen[2] = {-1, -1}; // per arity: 0 information form, 1 covariance form
    const bool rejection = options.poseEdgeOutlierRejection;
    g.e_pose.resize(cap), g.e_lm.resize(cap), g.e_flags.resize(cap);
    g.e_meas.resize(3 * cap), g.e_omega.resize(cap), g.e_cam.resize(cap);
    g.e_outlier_threshold.resize(cap);
    flatEdges_.resize(cap), flatEdgeSets_.resize(cap);
    bool omega_uniform = true, any_threshold = false;
    cugo_robust rk{CUGO_RK_NONE, 1.0, CUGO_RK_NONE, 1.0};
    struct Chunk
    {
        size_t begin = 0, count = 0;  // slot range written: [begin, begin + count)
        std::vector<double> cams;     // distinct cameras of this chunk (CK each: see below), first-seen order
        bool uniform = true;
        bool too_many_cams = false;
        bool fisheye_3d = false;      // a Kannala-Brandt model met on a 3-d (stereo or depth) edge
        bool distorted_3d = false;    // a non-zero lens distortion met on a 3-d (stereo or depth) edge
    };
    // A camera-table entry is keyed on CK = 5 + 7 + 5 + 5 numbers: the intrinsics, the sensor pose (q, t) as the caller
    // gave it, the projection model (k1..k4, type; a pinhole's coefficients are not looked at and count as zeros) and the
    // lens distortion (k1, k2, p1, p2, k3; a zero of either sign counts as zero).  Two entries that differ in any of them
    // are different entries; the key table is split into g.cams, g.cam_ext, g.cam_model and g.cam_dist behind the walk.
    constexpr size_t CK = 22;
    std::vector<double> camKeys;
    const unsigned hw = cugo_host::pool_threads();
    lap("graph: edge array alloc");
    size_t out = 0; // slots filled so far (compacted)
    for (size_t si = 0; si < edgeSets.size(); si++)
    {
        BaseEdgeSet* es = edgeSets[si];
        const int dim = es->dim();
        if (auto* ls = dynamic_cast<LandmarkPriorEdgeSet*>(es))
        { // landmark_prior_types.h, an extension: by type, before the dispatch on dim() (stereo BA sets are 3-d as well)
            flattenLandmarkPriorSet(ls, (int)si, vertexSets, options.perEdgeInformation, g.lm_priors);
            continue;
        }
        const bool gicp1 = dynamic_cast<GicpEdgeSet*>(es) != nullptr, gicp2 = dynamic_cast<GicpPairEdgeSet*>(es) != nullptr;
        if (es->nedges() > 0 && (gicp1 || gicp2 || dynamic_cast<PointEdgeSet*>(es) || dynamic_cast<PointPairEdgeSet*>(es)))
        { // one kind has one payload width: the two forms of one arity cannot share an optimiser (empty sets aside)
            const bool pairKind = gicp2 || dynamic_cast<PointPairEdgeSet*>(es);
            int& seen = pointFormSeen[pairKind ? 1 : 0];
            const int form = gicp1 || gicp2 ? 1 : 0;
            if (seen >= 0 && seen != form)
                throw std::runtime_error(std::string("cugo: edge set ") + std::to_string(si) + " (" +
                                         (pairKind ? (form ? "GicpPairEdgeSet" : "PointPairEdgeSet") : (form ? "GicpEdgeSet" : "PointEdgeSet")) +
                                         "): a covariance-form set and an information-form set of the same arity (" +
                                         (pairKind ? "GicpPairEdgeSet with PointPairEdgeSet" : "GicpEdgeSet with PointEdgeSet") +
                                         ") cannot be combined in one optimiser yet");
            seen = form;
        }
        if (gicp1 || gicp2)
        { // gicp_types.h, an extension: the covariance form of the point kinds, by type as well
            const char* cls = gicp2 ? "GicpPairEdgeSet" : "GicpEdgeSet";
            if (es->getOutlierThreshold() > 0.0)
                throw std::runtime_error(std::string("cugo: covariance-form point edge set ") + std::to_string(si) +
                                         ": outlier rejection is not supported on " + cls + " yet (setOutlierThreshold "
                                         "must stay 0, whatever poseEdgeOutlierRejection says)");
            const int kind = gicp2 ? cugo_host::POSE_KIND_PAIR : cugo_host::POSE_KIND_POINT;
            if (es->nedges() == 0)
                continue;
            g.kinds[kind].set_covariance_form();
            flattenPoseEdgeSet(
                es, (int)si, gicp2 ? 2 : 1, cls, vertexSets, false, g.kinds[kind], poseSetEdges_[si],
                [&](BaseEdge* e, auto& refuse, double* meas, double* weight) { gicpPayload(e, refuse, meas, weight); },
                [] { return (const char*)nullptr; });
            continue;
        }
        if (auto* pts = dynamic_cast<PointEdgeSet*>(es))
        { // point_edge_types.h, an extension: by type as well.  Outlier rejection is not available on this kind
            if (pts->getOutlierThreshold() > 0.0)
                throw std::runtime_error("cugo: point-to-point edge set " + std::to_string(si) +
                                         ": outlier rejection is not supported on PointEdgeSet yet (setOutlierThreshold "
                                         "must stay 0, whatever poseEdgeOutlierRejection says)");
            const double* setInformation = options.perEdgeInformation ? nullptr : pts->informationMatrix();
            flattenPoseEdgeSet(
                es, (int)si, 1, cugo_host::pose_kind_name(cugo_host::POSE_KIND_POINT), vertexSets, false,
                g.kinds[cugo_host::POSE_KIND_POINT], poseSetEdges_[si],
                [&](BaseEdge* e, auto& refuse, double* meas, double* weight) {
                    pointPayload(e, setInformation, refuse, meas, weight);
                },
                [&] { return setInformation ? checkInformation<3>(setInformation) : nullptr; });
            continue;
        }
        if (auto* pps = dynamic_cast<PointPairEdgeSet*>(es))
        { // point_pair_types.h, an extension: by type as well; the point kind's payload and checks, two vertices
            if (pps->getOutlierThreshold() > 0.0)
                throw std::runtime_error("cugo: pose-pose point edge set " + std::to_string(si) +
                                         ": outlier rejection is not supported on PointPairEdgeSet yet (setOutlierThreshold "
                                         "must stay 0, whatever poseEdgeOutlierRejection says)");
            const double* setInformation = options.perEdgeInformation ? nullptr : pps->informationMatrix();
            flattenPoseEdgeSet(
                es, (int)si, 2, cugo_host::pose_kind_name(cugo_host::POSE_KIND_PAIR), vertexSets, false,
                g.kinds[cugo_host::POSE_KIND_PAIR], poseSetEdges_[si],
                [&](BaseEdge* e, auto& refuse, double* meas, double* weight) {
                    pointPayload(e, setInformation, refuse, meas, weight);
                },
                [&] { return setInformation ? checkInformation<3>(setInformation) : nullptr; });
            continue;
        }
        if (dim == 1)
        { // PlaneEdgeSet / LineEdgeSet (icp_types.h): both have dim() 1, the type tells them apart
            const bool line = dynamic_cast<LineEdgeSet*>(es) != nullptr;
            if (!line && !dynamic_cast<PlaneEdgeSet*>(es))
                throw std::runtime_error("cugo: a 1-d edge set must be a PlaneEdgeSet or a LineEdgeSet (icp_types.h)");
            const int kind = line ? cugo_host::POSE_KIND_LINE : cugo_host::POSE_KIND_PLANE;
            const bool perInfo = options.perEdgeInformation;
            flattenPoseEdgeSet(
                es, (int)si, 1, cugo_host::pose_kind_name(kind), vertexSets, rejection, g.kinds[kind], poseSetEdges_[si],
                [&](BaseEdge* e, auto& refuse, double* meas, double* weight) {
                    icpInformation(es, e, perInfo, refuse, weight);
                    line ? linePayload(e, refuse, meas) : planePayload(e, refuse, meas);
                },
                [] { return (const char*)nullptr; });
            continue;
        }
        if (dim == 6)
        { // RelPoseEdgeSet (relpose_types.h; opt-in) or PosePriorEdgeSet (prior_types.h), extensions: the type tells them apart
            auto* rs = dynamic_cast<RelPoseEdgeSet*>(es);
            auto* ps = dynamic_cast<PosePriorEdgeSet*>(es);
            if (rs && !options.relativePoseEdges)
                throw std::runtime_error("cugo: the optimiser does not take relative-pose edge sets unless "
                                         "GraphOptimisationOptions::relativePoseEdges is on "
                                         "(their terms alone: cugo_relpose_* in include/cugo_hip.h)");
            if (!rs && !ps)
                throw std::runtime_error("cugo: a 6-d edge set must be a PosePriorEdgeSet (prior_types.h)");
            const int kind = rs ? cugo_host::POSE_KIND_RELPOSE : cugo_host::POSE_KIND_PRIOR;
            const double* setInformation =
                options.perEdgeInformation ? nullptr : rs ? rs->informationMatrix() : ps->informationMatrix();
            flattenPoseEdgeSet(
                es, (int)si, rs ? 2 : 1, cugo_host::pose_kind_name(kind), vertexSets, rejection, g.kinds[kind],
                poseSetEdges_[si],
                [&](BaseEdge* e, auto& refuse, double* meas, double* weight) {
                    priorPayload(e, setInformation, refuse, meas, weight);
                },
                [&] { return setInformation ? checkInformation36(setInformation) : nullptr; });
            continue;
        }
        if (dim != 2 && dim != 3)
            throw std::runtime_error("cugo: only 2-d (mono) and 3-d (stereo, depth) BA edge sets are supported");
        // DepthEdgeSet (ba_types.h): by type — a stereo set is 3-d as well.  Same array, flag bit of its own
        auto* ds = dynamic_cast<DepthEdgeSet*>(es);
        if (ds && ds->nedges() == 0)
            continue; // (an empty depth set leaves the graph one without depth edges)
        const uint8_t stereo_bit = ds ? CUGO_EDGE_DEPTH : dim == 3 ? CUGO_EDGE_STEREO : 0;
        const RobustKernel& k = es->robustKernelData();
        if (ds)
        {
            const double w = ds->inverseDepthWeight();
            if (!(w > 0.0) || !std::isfinite(w))
                throw std::runtime_error("cugo: depth edge set: the inverse-depth weight must be finite and > 0 (edge set " +
                                         std::to_string(si) + ")");
            if (g.has_depth && w != g.depth_weight)
                throw std::runtime_error("cugo: depth edge sets disagree on the inverse-depth weight (edge set " +
                                         std::to_string(si) + "): one weight per optimiser");
            g.has_depth = true, g.depth_weight = w;
            g.rk_type_depth = rk_code(k.type()), g.rk_delta_depth = k.delta();
        }
        else if (dim == 3)
            rk.type_stereo = rk_code(k.type()), rk.delta_stereo = k.delta();
        else
            rk.type = rk_code(k.type()), rk.delta = k.delta();
        const double set_threshold = es->getOutlierThreshold();
        any_threshold = any_threshold || set_threshold > 0.0;
        es->setOutlierCount(0);
        const double set_info = es->informationValue();
        const Camera set_cam = es->cameraData();
        const Se3D set_ext = es->sensorPoseData();
        const CameraModel set_model = es->cameraModelData();
        const CameraDistortion set_dist = es->distortionData();
        const EdgeContainer& ec = es->get();
        const size_t n = ec.size();
        const unsigned nthreads = n < 20000 ? 1u : hw;
        std::vector<Chunk> chunks(nthreads);
        const bool perInfo = options.perEdgeInformation, perCam = options.perEdgeCamera;
        const size_t base = out; // this set's edges go to slots [base, base + n) before compaction
        auto work = [&](unsigned t) {
            Chunk& c = chunks[t];
            const size_t i0 = n * t / nthreads, i1 = n * (t + 1) / nthreads;
            c.begin = base + i0;
            size_t o = c.begin;
            auto it = ec.begin() + i0;
            uint16_t last_cam = 0;
            for (size_t i = i0; i < i1; ++i, ++it)
            {
                // the walk is a chain of cache misses (edge object, then its two vertices):
                // fetch the edge 16 ahead and the vertices of the edge 8 ahead
                if (i + 16 < i1)
                    __builtin_prefetch(*(it + 16));
                if (i + 8 < i1)
                {
                    BaseEdge* e8 = *(it + 8);
                    __builtin_prefetch(e8->getVertex(0));
                    __builtin_prefetch(e8->getVertex(1));
                }
                BaseEdge* e = *it;
                if (!e->isActive())
                    continue;
                BaseVertex* vp = e->getVertex(0);
                BaseVertex* vl = e->getVertex(1);
                const bool fp = vp->isFixed(), fl = vl->isFixed();
                if (fp && fl)
                    continue;
                flatEdges_[o] = e, flatEdgeSets_[o] = es;
                g.e_outlier_threshold[o] = set_threshold;
                g.e_pose[o] = vp->getIndex();
                g.e_lm[o] = vl->getIndex();
                g.e_flags[o] = (uint8_t)((fl ? CUGO_EDGE_FIXED_L : 0) | (fp ? CUGO_EDGE_FIXED_P : 0) | stereo_bit);
                const double* mz = static_cast<const double*>(e->measurementData());
                g.e_meas[3 * o] = mz[0];
                g.e_meas[3 * o + 1] = mz[1];
                g.e_meas[3 * o + 2] = dim == 3 ? mz[2] : 0.0;
                const double w = perInfo ? (double)e->informationValue() : set_info;
                if (o > c.begin && w != g.e_omega[c.begin])
                    c.uniform = false;
                g.e_omega[o] = w;
                const Camera& cm = perCam ? e->cameraData() : set_cam;
                const Se3D& sx = perCam ? e->sensorPoseData() : set_ext;
                const CameraModel& md = perCam ? e->cameraModelData() : set_model;
                const bool kb = md.type != Pinhole;
                if (kb && dim == 3)
                    c.fisheye_3d = true;
                const CameraDistortion& dd = perCam ? e->distortionData() : set_dist;
                if (dim == 3 && !dd.isZero())
                    c.distorted_3d = true;
                const double cv[CK] = {cm.fx,        cm.fy,        cm.cx,        cm.cy,        cm.bf,        sx.r.data[0],
                                       sx.r.data[1], sx.r.data[2], sx.r.data[3], sx.t.data[0], sx.t.data[1], sx.t.data[2],
                                       kb ? md.k[0] : 0.0, kb ? md.k[1] : 0.0, kb ? md.k[2] : 0.0, kb ? md.k[3] : 0.0,
                                       (double)(int)md.type,
                                       dd.k1 + 0.0,  dd.k2 + 0.0,  dd.p1 + 0.0,  dd.p2 + 0.0,  dd.k3 + 0.0}; // (-0 + 0 = +0)
                // deduplicate cameras: last-hit fast path, then a short linear scan
                int ci = -1;
                const size_t ncam = c.cams.size() / CK;
                if (ncam > 0 && std::memcmp(&c.cams[CK * (size_t)last_cam], cv, sizeof cv) == 0)
                    ci = last_cam;
                else
                    for (size_t k2 = 0; k2 < ncam; k2++)
                        if (std::memcmp(&c.cams[CK * k2], cv, sizeof cv) == 0)
                        {
                            ci = (int)k2;
                            break;
                        }
                if (ci < 0)
                {
                    if (ncam >= 65535)
                    {
                        c.too_many_cams = true;
                        ci = 0;
                    }
                    else
                    {
                        ci = (int)ncam;
                        c.cams.insert(c.cams.end(), cv, cv + CK);
                    }
                }
                last_cam = (uint16_t)ci;
                g.e_cam[o] = (uint16_t)ci; // chunk-local index, remapped below
                o++;
            }
            c.count = o - c.begin;
        };
        struct WorkCtx
        {
            decltype(work)* w;
        } wctx{&work};
        cugo_host::pool_run(
            nthreads, [](void* p, unsigned t) { (*static_cast<WorkCtx*>(p)->w)(t); }, &wctx);
        size_t nactive = 0;
        for (Chunk& c : chunks)
        {
            if (c.too_many_cams)
                throw std::runtime_error("cugo: more than 65535 distinct cameras");
            if (c.fisheye_3d)
                throw std::runtime_error(
                    ds ? "cugo: camera models (Kannala-Brandt) together with depth edge sets are not supported yet (edge set " +
                             std::to_string(si) + ")"
                       : "cugo: a Kannala-Brandt camera model on a stereo edge set is not defined: bf has no meaning there "
                         "(edge set " + std::to_string(si) + ")");
            if (c.distorted_3d)
                throw std::runtime_error(
                    ds ? "cugo: lens distortion (radial-tangential) together with depth edge sets is not supported yet (edge set " +
                             std::to_string(si) + ")"
                       : "cugo: lens distortion (radial-tangential) on a stereo edge set is not supported: bf describes a "
                         "rectified pair (edge set " + std::to_string(si) + ")");
            // merge this chunk's cameras into the global table (first-seen order is kept)
            std::vector<uint16_t> remap(c.cams.size() / CK);
            bool identity = true;
            for (size_t q = 0; q < remap.size(); q++)
            {
                int ci = -1;
                const size_t ncam = camKeys.size() / CK;
                for (size_t k2 = 0; k2 < ncam; k2++)
                    if (std::memcmp(&camKeys[CK * k2], &c.cams[CK * q], CK * sizeof(double)) == 0)
                    {
                        ci = (int)k2;
                        break;
                    }
                if (ci < 0)
                {
                    if (ncam >= 65535)
                        throw std::runtime_error("cugo: more than 65535 distinct cameras");
                    ci = (int)ncam;
                    camKeys.insert(camKeys.end(), c.cams.begin() + CK * q, c.cams.begin() + CK * q + CK);
                }
                remap[q] = (uint16_t)ci;
                identity = identity && ci == (int)q;
            }
            if (c.count > 0 && (!c.uniform || (out > 0 && g.e_omega[c.begin] != g.e_omega[0])))
                omega_uniform = false;
            if (!identity)
                for (size_t i = c.begin; i < c.begin + c.count; i++)
                    g.e_cam[i] = remap[g.e_cam[i]];
            if (c.begin != out && c.count > 0)
            { // edges were skipped in an earlier chunk: close the gap
                std::memmove(&g.e_pose[out], &g.e_pose[c.begin], c.count * sizeof(int32_t));
                std::memmove(&g.e_lm[out], &g.e_lm[c.begin], c.count * sizeof(int32_t));
                std::memmove(&g.e_flags[out], &g.e_flags[c.begin], c.count);
                std::memmove(&g.e_meas[3 * out], &g.e_meas[3 * c.begin], 3 * c.count * sizeof(double));
                std::memmove(&g.e_omega[out], &g.e_omega[c.begin], c.count * sizeof(double));
                std::memmove(&g.e_cam[out], &g.e_cam[c.begin], c.count * sizeof(uint16_t));
                std::memmove(&g.e_outlier_threshold[out], &g.e_outlier_threshold[c.begin], c.count * sizeof(double));
                std::memmove(&flatEdges_[out], &flatEdges_[c.begin], c.count * sizeof(BaseEdge*));
                std::memmove(&flatEdgeSets_[out], &flatEdgeSets_[c.begin], c.count * sizeof(BaseEdgeSet*));
            }
            out += c.count;
            nactive += c.count;
        }
        // the next set starts right behind the compacted edges of this one
        es->setActiveEdgeCount(nactive);
        es->setDirtyState(false);
    }
    g.e_pose.resize(out), g.e_lm.resize(out), g.e_flags.resize(out), g.e_meas.resize(3 * out);
    g.e_omega.resize(out), g.e_cam.resize(out), g.e_outlier_threshold.resize(out);
    flatEdges_.resize(out), flatEdgeSets_.resize(out);
    if (omega_uniform && !g.e_omega.empty())
        g.e_omega.resize(1);
    if (!any_threshold)
        g.e_outlier_threshold.clear();
    // the key table -> cameras and extrinsics: the quaternion normalised and expanded to M here, in fp64
    for (size_t k = 0; k < camKeys.size() / CK; k++)
    {
        const double* key = &camKeys[CK * k];
        g.cams.insert(g.cams.end(), key, key + 5);
        const double n2 = key[5] * key[5] + key[6] * key[6] + key[7] * key[7] + key[8] * key[8];
        bool finite = std::isfinite(n2) && n2 > 0.0;
        for (int c = 9; c < 12; c++)
            finite = finite && std::isfinite(key[c]);
        if (!finite)
            throw std::runtime_error("cugo: camera extrinsics (sensor pose) of camera-table entry " + std::to_string(k) +
                                     ": the quaternion must be finite with a norm > 0, the translation finite");
        const double in = 1.0 / std::sqrt(n2);
        const double x = key[5] * in, y = key[6] * in, z = key[7] * in, w = key[8] * in;
        const double M[12] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w),     2 * (x * z + y * w),
                              2 * (x * y + z * w),     1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                              2 * (x * z - y * w),     2 * (y * z + x * w),     1 - 2 * (x * x + y * y),
                              key[9],                  key[10],                 key[11]};
        static const double I12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
        for (int c = 0; c < 12; c++)
            g.has_rig = g.has_rig || M[c] != I12[c];
        g.cam_ext.insert(g.cam_ext.end(), M, M + 12);
        // the model: (k1, k2, k3, k4, type); has_models iff some entry is not a pinhole
        const int type = (int)key[16];
        if (type != (int)Pinhole && type != (int)KannalaBrandt)
            throw std::runtime_error("cugo: camera model of camera-table entry " + std::to_string(k) +
                                     ": unknown model type " + std::to_string(type));
        for (int c = 12; c < 16; c++)
            if (!std::isfinite(key[c]))
                throw std::runtime_error("cugo: camera model (Kannala-Brandt) of camera-table entry " + std::to_string(k) +
                                         ": the coefficients k1..k4 must be finite");
        g.has_models = g.has_models || type != (int)Pinhole;
        g.cam_model.insert(g.cam_model.end(), key + 12, key + 17);
        // the distortion: (k1, k2, p1, p2, k3); has_dist iff some entry's coefficients are not all zero
        bool distorted = false;
        for (int c = 17; c < 22; c++)
        {
            if (!std::isfinite(key[c]))
                throw std::runtime_error("cugo: lens distortion (radial-tangential) of camera-table entry " +
                                         std::to_string(k) + ": the coefficients k1, k2, p1, p2, k3 must be finite");
            distorted = distorted || key[c] != 0.0;
        }
        if (distorted && type != (int)Pinhole)
            throw std::runtime_error("cugo: lens distortion (radial-tangential) on a Kannala-Brandt camera (camera-table "
                                     "entry " + std::to_string(k) + ") is not defined: the fisheye model has its own "
                                     "coefficients");
        g.has_dist = g.has_dist || distorted;
        g.cam_dist.insert(g.cam_dist.end(), key + 17, key + 22);
    }
    if (g.has_dist && g.has_depth)
        throw std::runtime_error("cugo: lens distortion (radial-tangential) together with depth edge sets is not supported "
                                 "yet");
    if (g.has_dist && g.has_models)
        throw std::runtime_error("cugo: lens distortion (radial-tangential) and Kannala-Brandt cameras in one graph are "
                                 "not supported yet");
    if (!g.has_dist)
        g.cam_dist.clear(); // (no distortion: the graph runs the kernels it has always run)
    if (g.has_models && g.has_depth)
        throw std::runtime_error("cugo: camera models (Kannala-Brandt) together with depth edge sets are not supported "
                                 "yet");
    if (!g.has_models)
        g.cam_model.clear(); // (pinholes only: the graph runs the kernels it has always run)
    if (!g.has_rig)
        g.cam_ext.clear(); // (identities only: the graph runs the kernels it has always run)
    if (g.cams.empty())
    {
        const double z[5] = {1, 1, 0, 0, 0};
        g.cams.assign(z, z + 5);
    }
    g.rk = rk;
    for (cugo_host::FlatPoseKind& fk : g.kinds)
    { // one weight for the whole kind: a single entry, as for the BA edges
        bool uniform = fk.n() > 0;
        for (size_t i = fk.weight_w; uniform && i < fk.weight.size(); i++)
            uniform = fk.weight[i] == fk.weight[i % fk.weight_w];
        if (uniform)
            fk.weight.resize(fk.weight_w);
        cugo_host::collapse_thresholds(fk.threshold);
    }
    { // one matrix for all landmark priors: a single entry
        std::vector<double>& w = g.lm_priors.info;
        bool uniform = !w.empty();
        for (size_t i = 6; uniform && i < w.size(); i++)
            uniform = w[i] == w[i % 6];
        if (uniform)
            w.resize(6);
    }
    lap("graph: edge flatten");

    engine_->initialize(g);
    lap("graph: engine initialize");
    stats_.clear();
    trace_.clear();
    // what this flattening was made from (compared by the next initialize())
    flattenCounts_.clear();
    for (BaseVertexSet* vs : vertexSets)
        flattenCounts_.emplace_back(vs, vs->changeCount());
    for (BaseEdgeSet* es : edgeSets)
        flattenCounts_.emplace_back(es, es->changeCount());
    flattenOptions_[0] = options.perEdgeInformation, flattenOptions_[1] = options.perEdgeCamera;
    flattenOptions_[2] = options.useFloat32, flattenOptions_[3] = options.relativePoseEdges;
    flattenOptions_[4] = options.poseEdgeOutlierRejection;
    flattenValid_ = true;
    initialized_ = true;
}

void CudaGraphOptimisationImpl::optimize(int niterations)
{
    const bool timing = engine_->options().init_timing;
    auto lap_t = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!timing)
            return;
        const auto n = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[cugo optimize] %-24s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(n - lap_t).count());
        lap_t = n;
    };
    if (options.planOnly)
        throw std::runtime_error("cugo: no HIP device in use: this optimiser is plan-only (GraphOptimisationOptions::planOnly)");
    std::vector<cugo_host::IterRecord> rec;
    engine_->optimize(niterations, rec, verbose);
    // the walk that writes the estimates back into the vertex objects is ~0.1 ms away (behind the download): the
    // workers of the host pool, parked during the optimisation, start waking up now
    cugo_host::pool_prewake();
    lap("engine optimize");
    for (const auto& r : rec)
    {
        stats_.addStat({r.iteration, r.chi2});
        trace_.push_back({r.lambda, r.rho, r.trials});
    }
    if (shouldProfile_)
        for (const auto& kv : timeProfile())
            std::printf("%s:  %f\n", kv.first.c_str(), kv.second);
    // ref: solver_->updateEdges(edgeSets) (cuda_graph_optimisation.cpp:151): edges whose chi2
    // exceeds their set's outlier threshold are inactivated; the set becomes dirty
    for (int32_t id : engine_->reject_outliers())
    {
        flatEdges_[id]->inactivate();
        BaseEdgeSet* es = flatEdgeSets_[id];
        es->setOutlierCount(es->getOutlierCount() + 1);
        es->setDirtyState(true);
    }
    // the same on the pose edge sets (GraphOptimisationOptions::poseEdgeOutlierRejection): the engine has flagged them
    // on the device and hands back where each came from
    for (const auto& kind : engine_->reject_pose_outliers())
        for (const auto& se : kind)
        {
            BaseEdgeSet* es = edgeSets[se.first];
            poseSetEdges_[se.first][se.second]->inactivate();
            es->setOutlierCount(es->getOutlierCount() + 1);
            es->setDirtyState(true);
        }
    // ref: finalize(): estimates go back into the user's vertex objects
    const double *hp = nullptr, *hl = nullptr;
    if (!engine_->download_pinned(&hp, &hl))
    { // a landmark shard: the estimates are combined over the ranks first
        std::vector<double>&poses = downloadPoses_, &lms = downloadLms_; // (kept between calls: 24 MB of fresh pages
        engine_->download(poses, lms);                                    //  per call on the 1 M-landmark graph otherwise)
        hp = poses.data(), hl = lms.data();
    }
    lap("outliers + download");
    for (BaseVertexSet* vs : vertexSets)
        vs->scatterEstimates(vs->isMarginilised() ? hl : hp);
    lap("scatter estimates");
}

const TimeProfile& CudaGraphOptimisationImpl::timeProfile()
{
    timeProfile_.clear();
    for (int i = 0; i < cugo_host::PROF_COUNT; i++)
        timeProfile_[Engine::profile_name(i)] = engine_->profile_ms()[i];
    return timeProfile_;
}

bool CudaGraphOptimisationImpl::computeMarginals(bool poses, bool landmarks)
{
    if (!initialized_)
        throw std::runtime_error("cugo: computeMarginals() needs initialize() first");
    if (options.planOnly)
        throw std::runtime_error("cugo: computeMarginals(): this optimiser is plan-only (no HIP device in use)");
    if (options.useFloat32)
        throw std::runtime_error("cugo: computeMarginals() is not available in the fp32-internal mode");
    for (BaseVertexSet* vs : vertexSets)
        if (!flattenedUnchanged(vs))
            throw std::runtime_error("cugo: computeMarginals(): a vertex set changed since initialize() (vertex added, "
                                     "removed or fixed / freed); call initialize() again");
    const int what = (poses ? 1 : 0) | (landmarks ? 2 : 0);
    if (!what)
        return true;
    return engine_->compute_covariances(what);
}

// the vertex set is one the last full flattening was made from, and nothing but estimates changed in it since:
// the indices and fixed flags of its vertices are those the covariances were computed with
bool CudaGraphOptimisationImpl::flattenedUnchanged(const BaseVertexSet* vs) const
{
    for (const auto& fc : flattenCounts_)
        if (fc.first == vs)
            return fc.second == vs->changeCount();
    return false;
}

bool CudaGraphOptimisationImpl::poseCovariance(const BaseVertex* v, double cov[36]) const
{
    if (!(engine_->covariances_held() & 1) || !v || v->isMarginilised() || !flattenedUnchanged(v->ownerSet()))
        return false;
    const int i = v->getIndex();
    if (v->isFixed() || i < 0 || i >= engine_->n_poses_free())
        std::fill(cov, cov + 36, 0.0);
    else
        std::copy(engine_->cov_pose().begin() + 36 * (size_t)i, engine_->cov_pose().begin() + 36 * (size_t)i + 36, cov);
    return true;
}

bool CudaGraphOptimisationImpl::poseCrossCovariances(int n, const BaseVertex* const* a, const BaseVertex* const* b,
                                                     double* cov36)
{
    if (!initialized_)
        throw std::runtime_error("cugo: poseCrossCovariances() needs initialize() first");
    if (options.planOnly)
        throw std::runtime_error("cugo: poseCrossCovariances(): this optimiser is plan-only (no HIP device in use)");
    if (options.useFloat32)
        throw std::runtime_error("cugo: poseCrossCovariances() is not available in the fp32-internal mode");
    if (n < 0)
        throw std::invalid_argument("cugo: poseCrossCovariances(): negative count");
    for (BaseVertexSet* vs : vertexSets)
        if (!flattenedUnchanged(vs))
            throw std::runtime_error("cugo: poseCrossCovariances(): a vertex set changed since initialize() (vertex "
                                     "added, removed or fixed / freed); call initialize() again");
    // free pose index in the flattening, -1 for a fixed pose
    std::vector<int32_t> ia(n), ib(n);
    auto index_of = [this](const BaseVertex* v) {
        if (!v || v->isMarginilised() || !flattenedUnchanged(v->ownerSet()))
            throw std::invalid_argument("cugo: poseCrossCovariances(): a vertex is not a pose of the current flattening");
        const int i = v->getIndex();
        return v->isFixed() || i < 0 || i >= engine_->n_poses_free() ? -1 : i;
    };
    for (int k = 0; k < n; k++)
        ia[k] = index_of(a[k]), ib[k] = index_of(b[k]);
    return engine_->pose_cross_covariances(n, ia.data(), ib.data(), cov36);
}

// what the two pose-landmark calls refuse, and the indices of their vertices in the flattening (fixed vertices keep
// theirs: behind the free ones)
void CudaGraphOptimisationImpl::poseLandmarkIndices(const char* who, int n, const BaseVertex* const* poses,
                                                    const BaseVertex* const* landmarks, std::vector<int32_t>& ia,
                                                    std::vector<int32_t>& il) const
{
    const std::string w = std::string("cugo: ") + who;
    if (!initialized_)
        throw std::runtime_error(w + "() needs initialize() first");
    if (options.planOnly)
        throw std::runtime_error(w + "(): this optimiser is plan-only (no HIP device in use)");
    if (options.useFloat32)
        throw std::runtime_error(w + "() is not available in the fp32-internal mode");
    if (n < 0)
        throw std::invalid_argument(w + "(): negative count");
    if (n > 0 && (!poses || !landmarks))
        throw std::invalid_argument(w + "(): null argument");
    for (BaseVertexSet* vs : vertexSets)
        if (!flattenedUnchanged(vs))
            throw std::runtime_error(w + "(): a vertex set changed since initialize() (vertex added, removed or fixed / "
                                         "freed); call initialize() again");
    ia.resize((size_t)n), il.resize((size_t)n);
    for (int k = 0; k < n; k++)
    {
        const BaseVertex *p = poses[k], *l = landmarks[k];
        if (!p || p->isMarginilised() || !flattenedUnchanged(p->ownerSet()) || p->getIndex() < 0)
            throw std::invalid_argument(w + "(): a vertex is not a pose of the current flattening");
        if (!l || !l->isMarginilised() || !flattenedUnchanged(l->ownerSet()) || l->getIndex() < 0)
            throw std::invalid_argument(w + "(): a vertex is not a landmark of the current flattening");
        ia[k] = p->getIndex(), il[k] = l->getIndex();
    }
}

bool CudaGraphOptimisationImpl::poseLandmarkCrossCovariances(int n, const BaseVertex* const* poses,
                                                             const BaseVertex* const* landmarks, double* cov18)
{
    std::vector<int32_t> ia, il;
    poseLandmarkIndices("poseLandmarkCrossCovariances", n, poses, landmarks, ia, il);
    if (n > 0 && !cov18)
        throw std::invalid_argument("cugo: poseLandmarkCrossCovariances(): null argument");
    // free index, -1 for a fixed vertex
    for (int k = 0; k < n; k++)
    {
        if (poses[k]->isFixed() || ia[k] >= engine_->n_poses_free())
            ia[k] = -1;
        if (landmarks[k]->isFixed() || il[k] >= engine_->n_landmarks_free())
            il[k] = -1;
    }
    return engine_->pose_landmark_cross_covariances(n, ia.data(), il.data(), cov18);
}

bool CudaGraphOptimisationImpl::reprojectionCovariances(int n, const BaseVertex* const* poses,
                                                        const BaseVertex* const* landmarks, int dim, const double* cam5,
                                                        int nCams, double* cov)
{
    std::vector<int32_t> ia, il;
    poseLandmarkIndices("reprojectionCovariances", n, poses, landmarks, ia, il);
    if (dim != 2 && dim != 3)
        throw std::invalid_argument("cugo: reprojectionCovariances(): dim must be 2 (mono) or 3 (stereo)");
    if (n > 0 && (!cam5 || !cov || (nCams != 1 && nCams != n)))
        throw std::invalid_argument("cugo: reprojectionCovariances(): cam5 must hold one camera or one per query");
    std::vector<double> cams(5 * (size_t)n);
    for (int k = 0; k < n; k++)
        std::copy(cam5 + 5 * (size_t)(nCams == 1 ? 0 : k), cam5 + 5 * (size_t)(nCams == 1 ? 0 : k) + 5, cams.begin() + 5 * (size_t)k);
    return engine_->reprojection_covariances(n, ia.data(), il.data(), dim, cams.data(), cov);
}

bool CudaGraphOptimisationImpl::predictObservations(int n, const BaseVertex* const* poses,
                                                    const BaseVertex* const* landmarks, int kind, const double* cam5,
                                                    int nCams, const Se3D* sensorPoses, const CameraModel* models,
                                                    double* z, double* cov)
{
    const std::string w = "cugo: predictObservations(): ";
    std::vector<int32_t> ia, il;
    poseLandmarkIndices("predictObservations", n, poses, landmarks, ia, il);
    if (kind != CUGO_OBS_MONO && kind != CUGO_OBS_STEREO && kind != CUGO_OBS_DEPTH)
        throw std::invalid_argument(w + "kind must be 2 (mono), 3 (stereo) or 4 (depth)");
    if (n > 0 && (!cam5 || !z || !cov || (nCams != 1 && nCams != n)))
        throw std::invalid_argument(w + "cam5 must hold one camera or one per query (nCams 1 or n), z and cov not null");
    // the camera table of the batch, one entry per query: the quaternion normalised and expanded to M in fp64, as
    // initialize() does for the table of the graph
    // (neither sensor poses nor models: nothing to check and no table to form)
    const bool tabled = sensorPoses || models;
    std::vector<double> cams(5 * (size_t)n), tab(tabled ? 17 * (size_t)n : 0);
    bool plain = true; // every entry a pinhole at the pose: the kernel then runs without the table
    for (int k = 0; k < n; k++)
    {
        const size_t c = nCams == 1 ? 0 : (size_t)k;
        std::copy(cam5 + 5 * c, cam5 + 5 * c + 5, cams.begin() + 5 * (size_t)k);
        if (!tabled)
            continue;
        double* e = &tab[17 * (size_t)k];
        if (k > 0 && nCams == 1)
        {
            std::copy(tab.begin(), tab.begin() + 17, e);
            continue;
        }
        double q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0};
        if (sensorPoses)
            sensorPoses[c].copyTo(q, t);
        const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
        if (!std::isfinite(n2) || !(n2 > 0.0) || !std::isfinite(t[0]) || !std::isfinite(t[1]) || !std::isfinite(t[2]))
            throw std::invalid_argument(w + "sensor pose of query " + std::to_string(k) +
                                        ": the quaternion must be finite with a norm > 0, the translation finite");
        const double in = 1.0 / std::sqrt(n2);
        const double x = q[0] * in, y = q[1] * in, zq = q[2] * in, qw = q[3] * in;
        const double M[12] = {1 - 2 * (y * y + zq * zq), 2 * (x * y - zq * qw),     2 * (x * zq + y * qw),
                              2 * (x * y + zq * qw),     1 - 2 * (x * x + zq * zq), 2 * (y * zq - x * qw),
                              2 * (x * zq - y * qw),     2 * (y * zq + x * qw),     1 - 2 * (x * x + y * y),
                              t[0],                      t[1],                      t[2]};
        std::copy(M, M + 12, e);
        const CameraModel md = models ? models[c] : CameraModel();
        if ((int)md.type != (int)Pinhole && (int)md.type != (int)KannalaBrandt)
            throw std::invalid_argument(w + "camera model of query " + std::to_string(k) + ": unknown model type " +
                                        std::to_string((int)md.type));
        for (int j = 0; j < 4; j++)
        {
            if (!std::isfinite((double)md.k[j]))
                throw std::invalid_argument(w + "camera model of query " + std::to_string(k) +
                                            ": the coefficients k1..k4 must be finite");
            e[12 + j] = (double)md.k[j];
        }
        e[16] = md.type == KannalaBrandt ? 1.0 : 0.0;
        if (md.type == KannalaBrandt && kind != CUGO_OBS_MONO)
            throw std::invalid_argument(w + "a Kannala-Brandt camera has the rows (u, v) only: kind must be 2 (mono), "
                                            "query " + std::to_string(k));
        static const double I12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
        for (int j = 0; j < 12; j++)
            plain = plain && M[j] == I12[j];
        plain = plain && md.type == Pinhole;
    }
    return engine_->predict_observations(n, ia.data(), il.data(), kind, cams.data(), plain ? nullptr : tab.data(), z, cov);
}

bool CudaGraphOptimisationImpl::landmarkCovariance(const BaseVertex* v, double cov[9]) const
{
    if (!(engine_->covariances_held() & 2) || !v || !v->isMarginilised() || !flattenedUnchanged(v->ownerSet()))
        return false;
    const int i = v->getIndex();
    if (v->isFixed() || i < 0 || i >= engine_->n_landmarks_free())
        std::fill(cov, cov + 9, 0.0);
    else
        std::copy(engine_->cov_lm().begin() + 9 * (size_t)i, engine_->cov_lm().begin() + 9 * (size_t)i + 9, cov);
    return true;
}

} // namespace cugo
