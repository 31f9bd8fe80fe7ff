// Public optimiser class of the cugo API, MI355X build
// (ref: include/cuda_graph_optimisation.h:52-282 — same class / method names and semantics).
// The reference header leaks cuda_runtime.h through device_buffer.h / cuda_device.h; here
// the GPU runtime is hidden behind an opaque engine inside libcugo_hip.so.
#pragma once
#include <cassert>
#include <cmath>
#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "ba_types.h"

namespace cugo_host
{
class Engine;
class RcclComm;
}

namespace cugo
{

template <class T>
using UniquePtr = std::unique_ptr<T>;
using EdgeSetVec = std::vector<BaseEdgeSet*>;
using VertexSetVec = std::vector<BaseVertexSet*>;

/** one record per LM iteration */
struct CUGO_API BatchInfo
{
    int iteration; //!< iteration number
    double chi2;   //!< total chi2 after the iteration
};

class CUGO_API BatchStatistics
{
public:
    BatchInfo getStartStats() const { return stats.at(0); }
    BatchInfo getLastStats() const { return stats.at(stats.size() - 1); }
    BatchInfo getStatEntry(const int idx) const { return stats.at(idx); }
    void addStat(const BatchInfo& b) { stats.push_back(b); }
    const std::vector<BatchInfo>& get() { return stats; }
    void clear() { stats.clear(); }

private:
    std::vector<BatchInfo> stats;
};

using TimeProfile = std::map<std::string, double>;

/** per-iteration Levenberg-Marquardt trace (extension; the reference only printf's these) */
struct CUGO_API LmTrace
{
    double lambda, rho;
    int trials;
};

/** all-reduce hook for landmark-sharded multi-GPU runs (one process per GPU):
 *  must reduce `n` doubles at DEVICE address `d_buf` in place over all ranks
 *  (op 0 = sum, 1 = max) before returning. */
using ExchangeFn = void (*)(void* d_buf, std::size_t n, int op, void* user);

class CudaGraphOptimisationImpl;

class CUGO_API CudaGraphOptimisation
{
public:
    using Ptr = UniquePtr<CudaGraphOptimisationImpl>;
    virtual ~CudaGraphOptimisation();
    static Ptr create();

    virtual void initialize() = 0;
    virtual void optimize(int niterations) = 0;
    virtual BatchStatistics& batchStatistics() = 0;
    virtual const TimeProfile& timeProfile() = 0;
    virtual EdgeSetVec& getEdgeSets() = 0;
    virtual size_t nVertices(const int id) = 0;
    virtual void clearEdgeSets() = 0;
    virtual void clearVertexSets() = 0;
    virtual void setVerbose(bool status) = 0;
    virtual void setProfile(bool status) = 0;
};

/**
 * Levenberg-Marquardt bundle adjustment on one MI355X (or one landmark shard of a multi-GPU
 * run).  The optimiser never owns vertices, edges or sets — the caller frees them
 * (ref: include/cuda_graph_optimisation.h:129-130).  vertexSets: non-marginalised = poses,
 * marginalised = landmarks; edge vertex 0 = pose, 1 = landmark.
 */
class CUGO_API CudaGraphOptimisationImpl : public CudaGraphOptimisation
{
public:
    CudaGraphOptimisationImpl(GraphOptimisationOptions& options);
    CudaGraphOptimisationImpl();
    ~CudaGraphOptimisationImpl();

    template <typename T>
    bool addEdgeSet(T* edgeSet)
    {
        assert(edgeSet != nullptr);
        edgeSets.push_back(edgeSet);
        return true;
    }
    template <typename T>
    bool addVertexSet(T* vertexSet)
    {
        assert(vertexSet != nullptr);
        vertexSets.push_back(vertexSet);
        return true;
    }

    EdgeSetVec& getEdgeSets() override { return edgeSets; }
    void initialize() override;
    void optimize(int niterations) override;
    BatchStatistics& batchStatistics() override { return stats_; }
    const TimeProfile& timeProfile() override;
    size_t nVertices(const int id) override { return vertexSets.at(id)->size(); }
    void clearEdgeSets() override
    {
        edgeSets.clear();
        flattenValid_ = false;
    }
    void clearVertexSets() override
    {
        vertexSets.clear();
        flattenValid_ = false;
    }
    void setVerbose(bool status) override { verbose = status; }
    void setProfile(bool status) override { shouldProfile_ = status; }

    // ---- extensions (not in the reference) ----
    void setShard(int rank, int world, ExchangeFn fn, void* user);
    /** native exchange of a landmark-sharded run: the per-trial all-reduce of [Hsc | bsc] runs as an
     *  RCCL collective on the solver's stream (communicator: cugo_comm_create of include/cugo_hip.h) */
    void setComm(std::shared_ptr<cugo_host::RcclComm> comm);
    void exchangeStats(double& bytes, int& calls) const;
    const std::vector<LmTrace>& lmTrace() const { return trace_; }
    int nActiveEdges() const;
    /** active point-to-plane (kind 0) / point-to-line (kind 1) edges of the current flattening (icp_types.h) */
    int nIcpEdges(int kind) const;
    /** active SE(3) pose priors of the current flattening (prior_types.h, an extension) */
    int nPriorEdges() const;
    /** relative-pose edges of the current flattening that count: active, at least one free end (relpose_types.h, an
     *  extension; GraphOptimisationOptions::relativePoseEdges) */
    int nRelPoseEdges() const;
    /** landmark position priors of the current flattening that count: active, on a free landmark
     *  (landmark_prior_types.h, an extension) */
    int nLandmarkPriorEdges() const;
    /** point-to-point pose edges of the current flattening that count: active, on a free pose (point_edge_types.h, an
     *  extension) */
    int nPointEdges() const;
    /** the point edges of the current flattening as the kernels read them: sorted by pose (stable), planar — pose [n],
     *  position of each edge in its set's container, p [3][n], z [3][n], info [6][n_info] (upper triangle, row-major
     *  packed); returns n_info (n, or 1 when one matrix serves all; nothing and 0 for a kind in the covariance form:
     *  flatGicpEdges).  Diagnostic */
    int flatPointEdges(std::vector<int>& pose, std::vector<int>& srcEdge, std::vector<double>& p, std::vector<double>& z,
                       std::vector<double>& info) const;
    /** pose-pose point edges of the current flattening that count: active, at least one free end (point_pair_types.h, an
     *  extension) */
    int nPointPairEdges() const;
    /** the pose-pose point edges of the current flattening as the kernels read them: in the order of their plan (runs of
     *  one (a, b) orientation of a pair, ordered by (lo, hi, orientation); container order inside a run), planar — pose a
     *  and pose b [n], position of each edge in its set's container, p [3][n], z [3][n], info [6][n_info] (upper triangle,
     *  row-major packed); returns n_info (n, or 1 when one matrix serves all; nothing and 0 for a kind in the covariance
     *  form: flatGicpPairEdges).  Diagnostic */
    int flatPointPairEdges(std::vector<int>& poseA, std::vector<int>& poseB, std::vector<int>& srcEdge, std::vector<double>& p,
                           std::vector<double>& z, std::vector<double>& info) const;
    /** covariance-form point edges (GicpEdgeSet / GicpPairEdgeSet, gicp_types.h, an extension) of the current flattening
     *  that count; nPointEdges() / nPointPairEdges() are 0 for a kind in the covariance form */
    int nGicpEdges() const;
    int nGicpPairEdges() const;
    /** as flatPointEdges / flatPointPairEdges, with covP and covZ [6][n_cov] (upper triangles, row-major packed) in place
     *  of info; returns n_cov (n, or 1 when one covariance pair serves all; 0 without such edges).  Diagnostic */
    int flatGicpEdges(std::vector<int>& pose, std::vector<int>& srcEdge, std::vector<double>& p, std::vector<double>& z,
                      std::vector<double>& covP, std::vector<double>& covZ) const;
    int flatGicpPairEdges(std::vector<int>& poseA, std::vector<int>& poseB, std::vector<int>& srcEdge, std::vector<double>& p,
                          std::vector<double>& z, std::vector<double>& covP, std::vector<double>& covZ) const;
    /** the pose-landmark edges of the current flattening in flattening order (set by set, container order; mono,
     *  stereo and depth edges share the array): flattened pose and landmark index, CUGO_EDGE_* flags, measurement
     *  (3 per edge, the third 0 for a mono edge).  Diagnostic */
    void flatEdges(std::vector<int>& pose, std::vector<int>& landmark, std::vector<unsigned char>& flags,
                   std::vector<double>& meas3) const;
    /** whether the current flattening holds depth edges, and their inverse-depth weight */
    bool flatDepth(double& weight) const;
    /** the camera table of the current flattening: 5 intrinsics per entry, and the sensor pose body -> sensor of each
     *  entry as {M row-major, t_s} (12 per entry; identities where no sensor pose was set).  Returns whether any entry
     *  is not the identity: only then do the edge kernels see the extrinsics at all.  Diagnostic */
    bool flatCameras(std::vector<double>& cam5, std::vector<double>& ext12) const;
    /** entries of that table whose sensor pose is not the identity */
    int nRigCameras() const;
    /** the projection models of that table (camera_model.h), parallel to flatCameras(): (k1, k2, k3, k4, type) per entry,
     *  type 0 Pinhole / 1 KannalaBrandt.  Returns whether any entry is not a pinhole: only then do the edge kernels get
     *  the model table (cugo_edges.has_rig == CUGO_RIG_MODELS), sensor poses included even if all are identities */
    bool flatCameraModels(std::vector<double>& model_k5) const;
    /** entries of that table whose model is KannalaBrandt */
    int nFisheyeCameras() const;
    /** the radial-tangential distortions of that table (camera_distortion.h), parallel to flatCameras(): (k1, k2, p1, p2,
     *  k3) per entry.  Returns whether any entry's coefficients are not all zero: only then do the edge kernels get the
     *  distortion table (cugo_edges.has_rig == CUGO_RIG_DISTORTION), sensor poses included even if all are identities */
    bool flatCameraDistortions(std::vector<double>& dist5) const;
    /** entries of that table whose distortion is not all zero */
    int nDistortedCameras() const;
    /** B, M, nnz(L), flops, supernodes, stages, front bytes, off-diagonal products, then per
     *  factorisation: potrf / trsm / syrk flops, extend-add bytes, backward bytes */
    std::vector<double> structureStats() const;
    /** HIP-event timing on the solver's stream (diagnostic).  1: an event pair round every kernel group and every
     *  kernel (per-kernel figures; each pair adds a few microseconds to what it brackets); 2: one event per group
     *  boundary — group times that add up exactly to the device time of optimize(); 0: off */
    void setKernelTiming(int mode);
    void kernelTimes(std::vector<std::string>& names, std::vector<double>& ms, std::vector<int>& launches) const;
    /** GraphOptimisationOptions::useFloat32 after construction; takes effect at the next initialize() */
    void setUseFloat32(bool on) { options.useFloat32 = on; }
    /** initialize() calls that found the graph unchanged and refreshed only the estimates */
    int flattenReuses() const { return flattenReuses_; }
    bool useFloat32() const { return options.useFloat32; }
    /** a run-time switch of this optimiser ("flatten_reuse", "structure_reuse", "init_timing"; the optimiser took a
     *  snapshot of the CUGO_* environment variables when it was created), or "pose_edge_outliers"
     *  (GraphOptimisationOptions::poseEdgeOutlierRejection after construction; takes effect at the next
     *  initialize()); false: unknown name */
    bool setOption(const char* name, int value);
    /** marginal covariances at the current estimates (g2o SparseOptimizer::computeMarginals, Ceres Covariance):
     *  Sigma = H^-1 of the undamped J^T Omega J (robust weights included) over the free vertices, diagonal blocks
     *  only; kept until the next initialize().  false: a zero pivot (an unconstrained gauge, a free pose without
     *  edges, a landmark seen too little).  Throws std::runtime_error before initialize() and on plan-only,
     *  sharded or fp32-internal optimisers. */
    bool computeMarginals(bool poses = true, bool landmarks = true);
    /** the 6x6 block of a pose (column-major, tangent order [rotation, translation] of the left update
     *  T <- exp([w, v]) T); all zero for a fixed pose.  false: no pose blocks were computed since the last
     *  initialize(), v is not a pose vertex, or its set changed since (vertex added, removed, fixed / freed) */
    bool poseCovariance(const BaseVertex* v, double cov[36]) const;
    /** the 3x3 block of a landmark (column-major); all zero for a fixed landmark.  false: as poseCovariance */
    bool landmarkCovariance(const BaseVertex* v, double cov[9]) const;
    /** cross-covariances of ANY pose pairs (g2o computeMarginals(spinv, blockIndices)): cov36 [n][36], block k is
     *  Sigma_ab of (a[k], b[k]) at the current estimates, 6x6 column-major with rows a and columns b, tangent order as
     *  poseCovariance; a == b gives the diagonal block, a block with a fixed pose is zero.  The pairs need not be in
     *  the Hsc pattern: the joint uncertainty of a loop-closure candidate before its edge exists.  Runs what
     *  computeMarginals runs up to the factorisation and leaves the marginals stored by it untouched.  false: a zero
     *  pivot.  Throws as computeMarginals does, and for a vertex that is not a pose of the current flattening. */
    bool poseCrossCovariances(int n, const BaseVertex* const* a, const BaseVertex* const* b, double* cov36);
    /** pose-landmark blocks of the covariance (g2o computeMarginals / Ceres Covariance with mixed pairs): cov18
     *  [n][18], block k is Sigma_al of (poses[k], landmarks[k]) at the current estimates, 6x3 column-major with the rows
     *  in the tangent order of poseCovariance; zero where either vertex is fixed.  The pair needs no edge.  With
     *  poseCovariance and landmarkCovariance this gives the joint covariance of a camera and a map point.  The contract
     *  of poseCrossCovariances; false also when the Hll of a QUERIED landmark is not positive definite (a free landmark
     *  without an active edge) — other landmarks in that state do not matter. */
    bool poseLandmarkCrossCovariances(int n, const BaseVertex* const* poses, const BaseVertex* const* landmarks,
                                      double* cov18);
    /** covariance of the predicted reprojection of landmarks[k] in poses[k]: S = J Sigma J^T over the joint [pose;
     *  landmark] block with the Jacobians of the projection — the search ellipse of guided matching, the denominator
     *  of a normalised-innovation test.  cov [n][dim * dim] column-major, dim 2 (mono: u, v) or 3 (stereo: u, v,
     *  u_right); cam5 [nCams][5] = fx, fy, cx, cy, bf with nCams 1 (one camera for all) or n.  A fixed pose contributes
     *  no pose terms, a fixed landmark no landmark terms.  Contract and return value as above; throws
     *  std::invalid_argument for another dim or nCams.  cam5 describes a camera AT THE POSE: on a graph with sensor
     *  poses (setSensorPose: the pose vertex is then the body) this is the reprojection into a camera whose sensor
     *  pose is the identity.  Likewise it is a PINHOLE: on a graph with Kannala-Brandt models (setCameraModel) cam5
     *  is still read as fx, fy, cx, cy, bf of X / Z.  For a camera of a rig, a fisheye camera or a depth observation:
     *  predictObservations below. */
    bool reprojectionCovariances(int n, const BaseVertex* const* poses, const BaseVertex* const* landmarks, int dim,
                                 const double* cam5, int nCams, double* cov);
    /** the predicted observation z of landmarks[k] seen from poses[k] and its covariance S = J Sigma J^T, for every
     *  camera kind the optimiser accepts.  kind: 2 (mono, z = (u, v)), 3 (stereo, (u, v, u_right)) or 4 (depth,
     *  (u, v, 1 / Z_s)) — CUGO_OBS_MONO / _STEREO / _DEPTH of cugo_hip.h; dim = 2, 3, 3.  Camera of a query: cam5 as
     *  above; sensorPoses (null: identities) the pose body -> sensor in the convention of setSensorPose, its
     *  quaternion normalised in fp64 as initialize() does; models (null: pinholes) as setCameraModel.  nCams is 1 or
     *  n and counts for all three.  With Xb = R(q_a) X_l + t_a and Xs = M Xb + t_s, z is the projection of Xs and J
     *  the build pass's Jacobians of z - m.  The depth row is that of 1 / Z_s under unit weight: S is in measurement
     *  units, the inverse-depth weight of a DepthEdgeSet belongs to the caller's noise term.  A depth kind behind a
     *  sensor pose is defined here (the optimiser refuses such graphs; a query is not a graph).  z [n][dim] is
     *  computed for fixed vertices too; cov [n][dim * dim] column-major, exactly symmetric, fixed vertices as above.
     *  With identity sensor poses and pinhole models the kinds 2 / 3 give the bits of reprojectionCovariances.
     *  false (a zero pivot, or a queried free landmark whose Hll does not factor): z and cov zero-filled.  Throws as
     *  reprojectionCovariances does, and std::invalid_argument for another kind, a quaternion that is not finite or
     *  has norm 0, coefficients that are not finite, an unknown model type and a Kannala-Brandt model with kind 3 or
     *  4.  Nothing guards the projection itself: a pinhole query with Z_s = 0, or a Kannala-Brandt query on the
     *  negative optical axis, gives inf / NaN in its own z and S. */
    bool predictObservations(int n, const BaseVertex* const* poses, const BaseVertex* const* landmarks, int kind,
                             const double* cam5, int nCams, const Se3D* sensorPoses, const CameraModel* models, double* z,
                             double* cov);

private:
    void poseLandmarkIndices(const char* who, int n, const BaseVertex* const* poses, const BaseVertex* const* landmarks,
                             std::vector<int32_t>& ia, std::vector<int32_t>& il) const;
    bool verbose = false;
    bool shouldProfile_ = false;
    GraphOptimisationOptions options;
    VertexSetVec vertexSets;
    EdgeSetVec edgeSets;
    std::unique_ptr<cugo_host::Engine> engine_;
    BatchStatistics stats_;
    std::vector<LmTrace> trace_;
    TimeProfile timeProfile_;
    // change counts of the sets at the last full flattening (initialize() refreshes only the
    // estimates while they stand)
    std::vector<std::pair<const void*, unsigned long long>> flattenCounts_;
    bool flattenOptions_[5] = {false, false, false, false, false};
    bool flattenValid_ = false;
    bool initialized_ = false; // initialize() ran (computeMarginals needs it)
    bool flattenedUnchanged(const BaseVertexSet* vs) const;
    int flattenReuses_ = 0;
    // edges handed to the engine at initialize(), in that order (outlier rejection maps back)
    std::vector<BaseEdge*> flatEdges_;
    std::vector<BaseEdgeSet*> flatEdgeSets_;
    // the same for the pose edge sets that carry an outlier threshold: per edge set (position in edgeSets), the
    // flattened edge at every position of its container (nullptr: not flattened); empty for every other set
    std::vector<std::vector<BaseEdge*>> poseSetEdges_;
    std::vector<double> downloadPoses_, downloadLms_; // staging of the estimates that optimize() writes back
};

} // namespace cugo
