// vh.hpp -- C++ host classes of the MI355X voxel-hashing engine.
//
// Same class names, constructors and public methods as the reference's
// CUDASceneRepHashSDF (DSC/CUDASceneRepHashSDF.h:28-350), CUDARayCastSDF
// (DSC/CUDARayCastSDF.h:13-69) and CUDASceneRepChunkGrid
// (DSC/CUDASceneRepChunkGrid.h:152-753), so the reference's frame loop
// (DSC/DepthSensing.cpp:720-924) compiles against them after swapping the
// includes.  Differences, all forced by dropping Windows/D3D/mLib:
//   - mat4f / vec3f / vec3i are small PODs defined here (row-major 4x4);
//   - GlobalAppState is gone: the five flags it supplied are a VhSceneOptions;
//   - DepthCameraParams is passed explicitly where the reference read the
//     process-global __constant__ c_depthCameraParams;
//   - errors throw vh::Error (the reference aborts via cutilSafeCall/exit);
//   - a HIP stream can be given; all work of one instance is issued on it.
//
// This header needs no HIP headers; link against libvoxelhashing_amd.so.
//   DSC/ = /root/reference/DepthSensingCUDA/Source/
#ifndef VH_HPP
#define VH_HPP

#include <condition_variable>
#include <cstdint>
#include <memory>
#include <atomic>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>

#include "vh_api.h"
#include "vh_owners.hpp"

typedef VhHashEntry HashEntry;
typedef VhVoxel Voxel;
typedef VhHashParams HashParams;
typedef VhHashData HashData;
typedef VhDepthCameraParams DepthCameraParams;
typedef VhDepthCameraData DepthCameraData;
typedef VhRayCastParams RayCastParams;
typedef VhRayCastData RayCastData;
typedef VhSDFBlockDesc SDFBlockDesc;

namespace vh {

struct vec3f { float x, y, z; };
struct vec3i { int x, y, z; };

// Row-major 4x4, entries m[0..15] = m11,m12,...,m44 (the layout of the
// reference's float4x4 / mLib mat4f).
struct mat4f {
    float m[16];
    static mat4f identity();
    mat4f getInverse() const; // float4x4::getInverse, DSC/cuda_SimpleMatrixUtil.h:944-1069
    mat4f operator*(const mat4f& o) const;
    vec3f transformPoint(const vec3f& p) const; // float4x4 * float3, :900-907
    float& operator()(int r, int c) { return m[4 * r + c]; }
    float operator()(int r, int c) const { return m[4 * r + c]; }
};

struct SDFBlock { // DSC/CUDASceneRepChunkGrid.h:11-21
    Voxel data[VH_SDF_BLOCK_VOXELS];
};

// The plain projective-ICP solve (DSC/CUDACameraTrackingMultiRes.cpp:241-321) as its two hosts enqueue it:
// CUDACameraTrackingMultiRes::applyCT and Reconstruction's tracked frame (vh_tracking.cpp).
// The maps of one call, per level; owns nothing (level 0 is usually somebody else's: the sensor's, the ray caster's).
struct IcpPyramid {
    float* map[VH_TRACKING_MAX_LEVELS];
    float* normal[VH_TRACKING_MAX_LEVELS];
};
// level 0 as given, the levels from 1 on from their owners (whose element 0 is not looked at)
IcpPyramid icpPyramid(float* map0, float* normal0, const std::vector<DevicePtr<float>>& maps, const std::vector<DevicePtr<float>>& normals);
// the device scratch of a solve, and its enqueue
struct IcpSolver {
    IcpSolver(unsigned int imageWidth, unsigned int imageHeight, unsigned int levels, const char* who); // throws who + ": bad pyramid"
    std::vector<unsigned int> width, height;                            // per level
    std::vector<DevicePtr<float>> model, modelNormal;                   // levels >= 1 (element 0 stays empty)
    std::vector<DevicePtr<float>> correspondence, correspondenceNormal; // what a three-kernel level keeps between its kernels
    DevicePtr<float> partials;
    DevicePtr<float> estimate;     // the 4x4 delta a solve starts from: the caller writes it
    DevicePtr<VhIcpState> state;   // where a solve leaves its outcome
    DevicePtr<uint32_t> ticket;    // vh_icp_step's count of finished workgroups
    // level i + 1 of a pyramid from its level i (resampleFloat4Map + computeNormals, :256-263)
    void coarserLevel(const IcpPyramid& p, unsigned int i, vhStream_t stream) const;
    // Coarse to fine from `estimate` (:265-321, the loop exits taken on the device).  fusedStep: an iteration of a level
    // with s_maxInnerIter == 1 is one launch (vh_icp_step) instead of three.  d_result: the outcome is also published
    // there (mapped host memory) with `tag` stored behind it -- by the last step itself if that is a fused one, by
    // vh_icp_publish otherwise.
    void align(const IcpPyramid& input, const IcpPyramid& model, const VhTrackingState& settings, const DepthCameraParams& depthCameraParams,
               bool fusedStep, VhIcpResult* d_result, uint32_t tag, vhStream_t stream) const;
};

// The RGB-D solve (DSC/CUDACameraTrackingMultiResRGBD.cpp:239-353) as its two hosts enqueue it:
// CUDACameraTrackingMultiResRGBD::applyCT and Reconstruction's tracked frame (vh_tracking.cpp).
// The intensity maps the solve reads of the input, per level: the unfiltered map on level 0 (:267 copies it), the
// Gauss-filtered one above.  Owns nothing.
struct IcpIntensityPyramid {
    float* intensity[VH_TRACKING_MAX_LEVELS]; // level i from level i - 1 (resampleFloatMap)
    float* filtered[VH_TRACKING_MAX_LEVELS];  // levels >= 1 (element 0 is not looked at)
};
IcpIntensityPyramid icpIntensityPyramid(const std::vector<DevicePtr<float>>& intensity, const std::vector<DevicePtr<float>>& filtered);
// what of a solve does not depend on the frame, and its enqueue
struct IcpSolverRGBD {
    IcpSolverRGBD(unsigned int imageWidth, unsigned int imageHeight, unsigned int levels, const char* who); // throws who + ": bad pyramid"
    std::vector<unsigned int> width, height;                                        // per level
    std::vector<DevicePtr<float>> model, modelNormal;                               // levels >= 1 (element 0 stays empty)
    std::vector<DevicePtr<float>> modelIntensity, modelIntensityAndDerivatives;     // every level
    std::vector<DevicePtr<float>> modelIntensityFiltered;                           // levels >= 1
    DevicePtr<float> partials;
    DevicePtr<float> estimate;        // the 4x4 delta a solve starts from: the caller writes it
    DevicePtr<VhIcpStateRGBD> state;  // where a solve leaves its outcome
    DevicePtr<uint32_t> ticket;       // vh_icp_rgbd_step's count of finished workgroups
    // The input half of the pyramids (:264-284) on `stream`: level-0 intensity from the float4 colour map, then per level
    // resampleFloat4Map + computeNormals of the positions and resampleFloatMap + gaussFilterFloatMap (3, 1) of the intensity.
    void inputPyramid(const IcpPyramid& input, const float* d_inputColor, const IcpIntensityPyramid& intensity, vhStream_t stream) const;
    // The model half: intensity of the ray cast's colours and its derivatives, then per level the positions, normals,
    // intensity, Gauss filter and derivatives.
    void modelPyramid(const IcpPyramid& model, const float* d_modelColor, vhStream_t stream) const;
    // Coarse to fine from `estimate` (:289-353, the loop exits taken on the device).  fusedStep: an iteration is one launch
    // (vh_icp_rgbd_step) instead of two.  d_result: the outcome is also published there (mapped host memory) with `tag`
    // stored behind it -- by the last step itself if that is a fused one, by vh_icp_publish otherwise.
    void align(const IcpPyramid& input, const IcpIntensityPyramid& inputIntensity, const IcpPyramid& model, const VhTrackingStateRGBD& settings,
               const DepthCameraParams& depthCameraParams, bool fusedStep, VhIcpResult* d_result, uint32_t tag, vhStream_t stream) const;
};

} // namespace vh

struct VhStageTimer; // opaque: per-stage HIP event pairs

// ---------------------------------------------------------------------------
class CUDASceneRepHashSDF {
public:
    explicit CUDASceneRepHashSDF(const HashParams& params);
    CUDASceneRepHashSDF(const HashParams& params, const VhSceneOptions& options, vhStream_t stream = nullptr);
    ~CUDASceneRepHashSDF();
    CUDASceneRepHashSDF(const CUDASceneRepHashSDF&) = delete;
    CUDASceneRepHashSDF& operator=(const CUDASceneRepHashSDF&) = delete;

    static VhSceneOptions defaultOptions();

    // no-op kept for source compatibility (DSC/CUDASceneRepHashSDF.h:60-62)
    void bindDepthCameraTextures(const DepthCameraData&) {}

    // DSC/CUDASceneRepHashSDF.h:64-83
    void integrate(const vh::mat4f& lastRigidTransform, const DepthCameraData& depthCameraData,
                   const DepthCameraParams& depthCameraParams, const unsigned int* d_bitMask);
    void setLastRigidTransform(const vh::mat4f& lastRigidTransform);                       // :85
    void setLastRigidTransformAndCompactify(const vh::mat4f& lastRigidTransform,
                                            const DepthCameraParams& depthCameraParams);   // :90
    const vh::mat4f getLastRigidTransform() const;                                         // :96
    void reset();                                                                          // :101
    HashData& getHashData() { return m_hashData; }                                         // :112
    // m_numOccupiedBlocks is exact in offline mode; in online mode it is the
    // most recent count whose asynchronous read-back has completed.
    const HashParams& getHashParams();                                                     // :116
    unsigned int getHeapFreeCount();                                                       // :122 (blocking)
    unsigned int getNumOccupiedBlocks();                                                   // blocking, exact
    // :129-233; throws vh::Error on a violated invariant.  report = {numOccupied, numFree, duplicates, lockEntries}
    void debugHash(unsigned int report[4] = nullptr);

    // additions
    // The two halves of integrate() for a frame loop that knows the pose of a frame before it ray-casts the previous
    // one (a recorded trajectory: s_binaryDumpSensorUseTrajectory, DSC/DepthSensing.cpp:733-747).  integrateAhead()
    // sets the pose and returns the frame's alloc + compactify passes as a job; CUDARayCastSDF::render(..., job)
    // launches them INSIDE its own two launches (the alloc pass behind the ray caster's workgroups, where it fills the
    // tail the dearest tiles leave; the compactify pass behind computeNormals'); integrateFinish() launches whatever
    // of the job is still open and then the pass over the voxels.  The maps stay the same: a block allocated while
    // rays are marched holds only unobserved voxels (weight 0), which a sample treats exactly like an absent block
    // (DESIGN.md section 3).  Offline mode and the reference launch sequence need their blocking read-backs: there the
    // job is never handed out.
    VhFrameJob* integrateAhead(const vh::mat4f& lastRigidTransform, const DepthCameraData& depthCameraData,
                               const DepthCameraParams& depthCameraParams, const unsigned int* d_bitMask);
    void integrateFinish(const DepthCameraData& depthCameraData, const DepthCameraParams& depthCameraParams);
    // gives up a job of integrateAhead() that will not be finished (the caller is unwinding): the scene accepts
    // integrate() / integrateAhead() again.  Blocks an alloc pass that already ran has added stay: they are empty, and
    // garbage collection takes them like any other unobserved block.
    void abortAhead();
    // frames whose pass over the voxels has started on the device (read from mapped host memory: no synchronisation)
    unsigned int getNumFramesStartedOnDevice() const;
    // whoever edits the table outside integrate() (streaming) says so: work prepared from the table before is void
    void noteTableEdited() { m_tableEpoch++; }
    unsigned int getTableEpoch() const { return m_tableEpoch; }
    void setOptions(const VhSceneOptions& o) { m_options = o; }
    // How integrate() fuses colour (HashParams::m_colorIntegration): VH_COLOR_RUNNING_AVERAGE, the reference's running 50/50
    // average (a surface seen once has half its brightness), or VH_COLOR_WEIGHTED_AVERAGE, the average weighted by the
    // voxel weights the reference left commented out (DSC/VoxelUtilHashSDF.h:241), which lets the RGB-D tracker follow its
    // own reconstruction.  Holds from the next integrate() / integrateAhead() on (not between integrateAhead() and
    // integrateFinish(): the frame in progress has its parameters); a scene created from HashParams with the word set
    // starts with it.  Throws on any other mode.
    void setColorIntegration(unsigned int mode);
    unsigned int getColorIntegration() const { return m_hashParams.m_colorIntegration; }
    // Distance, colour, validity and (d_gradient != nullptr) gradient at n world points: vh_query_points (vh_api.h has the
    // semantics) on the scene's stream.  Device pointers.  Read-only, on the blocks resident on the device (blocks
    // streamed out to the host grid are absent); the caller must not run it beside an integrate on another stream.
    void queryPoints(const float* d_points, unsigned int n, float* d_sdf, uint32_t* d_color, float* d_gradient, uint8_t* d_valid);
    // Scene merge (DESIGN.md section 4 "Scene merge"; vh_api.h has the semantics of vh_merge_blocks): every block resident
    // in `other`'s table, shifted by a whole-block offset, is fused into this scene -- allocated where this scene lacks
    // the position, then merged voxel by voxel (unobserved source voxels change nothing, an unobserved voxel here takes
    // the source's with its weight capped, two observed ones go through combineVoxel with THIS scene's weight cap and
    // colour mode).  mergeBlocks takes a block list in device memory instead ({desc, 512 voxels} as the streaming
    // passes move them; d_leftOut: n device words or nullptr).  Both block until the merge is done, and leave the
    // compactified list stale as a stream-in does: compactify before the next ray cast.  Throw VH_ERR_BAD_ARGUMENT (and
    // do nothing) for two voxel sizes, other == this and a frame in flight in either scene (integrateAhead without
    // integrateFinish), VH_ERR_HEAP_EXHAUSTED (and do nothing) when the positions this scene lacks outnumber its free
    // blocks.  Blocks for which the table had no slot are left out whole and counted; *counts (may be nullptr) is
    // filled before any throw.  No block of this scene may be streamed out to a chunk grid (not checked here).
    struct MergeCounts {
        unsigned int c[VH_MERGE_NUM_COUNTS]; // indexed by VH_MERGE_*
        unsigned int status() const { return c[VH_MERGE_STATUS]; }
    };
    void mergeScene(const CUDASceneRepHashSDF& other, const int32_t blockOffset[3], MergeCounts* counts = nullptr);
    void mergeBlocks(const SDFBlockDesc* d_descs, const Voxel* d_blocks, unsigned int n, const int32_t blockOffset[3], uint32_t* d_leftOut = nullptr,
                     MergeCounts* counts = nullptr);
    // Resampled merge (DESIGN.md section 4 "Resampled merge"; vh_api.h has the rule of vh_resample_blocks): `other`, whose
    // world frame and voxel size may differ from this scene's, is sampled at this scene's voxel centres under the rigid
    // transform dstFromSrc (4x4 row-major, metres, this scene's frame from other's) and the resulting block list is fused
    // by the plain merge.  Only destination blocks with an observed voxel are listed: a source block of unobserved voxels
    // allocates nothing here, where mergeScene allocates its block.  Blocks; nothing of this scene is written before the
    // merge stage, so a refusal leaves it as it was: VH_ERR_BAD_ARGUMENT for a matrix that is not rigid, a ratio of voxel
    // sizes outside [1/2, 2], other == this, a frame in flight in either scene, and a block outside [-2^20, 2^20)
    // (VH_RESAMPLE_OUT_OF_RANGE); VH_ERR_HEAP_EXHAUSTED as mergeScene.  Both counts (may be nullptr) are filled before a throw.
    struct ResampleCounts {
        unsigned int c[VH_RESAMPLE_NUM_COUNTS]; // indexed by VH_RESAMPLE_*
        unsigned int status() const { return c[VH_RESAMPLE_STATUS]; }
    };
    void mergeSceneTransformed(const CUDASceneRepHashSDF& other, const double dstFromSrc[16], MergeCounts* counts = nullptr, ResampleCounts* resampled = nullptr);
    // Scene registration (DESIGN.md section 4 "Scene registration"; vh_api.h has the rule of vh_align_step): refines the
    // rigid transform `guess` (4x4 row-major, metres, this scene's frame from other's) so that `other`'s near-surface
    // voxels fall where this scene's field has their distance: direct SDF-to-SDF Gauss-Newton on the device, up to
    // options.maxIterations steps enqueued back to back and one read of the state at the end.  Neither scene is written.
    // result->status tells how it ended (VH_ALIGN_*): only with VH_ALIGN_CONVERGED is result->dstFromSrc an answer; a
    // scene that leaves a motion free (a lone plane, a lone sphere) ends with VH_ALIGN_ILL_CONDITIONED and the guess
    // unchanged.  The basin is a few voxels and a few degrees around the guess (the truncation band bounds it; there is
    // no pyramid); blocks streamed out to a chunk grid are absent; colours are not used.  Throws VH_ERR_BAD_ARGUMENT,
    // with nothing done, for other == this, a frame in flight in either scene, a guess or a ratio of voxel sizes that
    // vh_resample_voxel_transforms refuses, options that are not finite and positive or exceed their bounds, and a source
    // of more than VH_ALIGN_MOST_BLOCKS blocks.
    struct AlignOptions : VhAlignOptions {
        AlignOptions() { band = 2.0f; condThres = 1e4f; rotThres = 1e-5; transThres = 1e-3; minCount = 200u; maxIterations = 30u; }
    };
    typedef VhAlignState AlignResult;
    void alignScene(const CUDASceneRepHashSDF& other, const double guess[16], const AlignOptions& options, AlignResult* result);
    // Scene cut (DESIGN.md section 4 "Scene cut"; vh_api.h has the rule of vh_cut_blocks): the opposite of the merge, on
    // the blocks resident in this scene's table.  eraseRegion zeroes the voxels inside the region and frees the blocks
    // in which no observed voxel is left; cropToRegion does that to everything that is not inside.  extractRegion copies
    // the region out and writes nothing here: the blocks with an observed voxel in the region, the voxels outside it
    // zero, into d_descs / d_blocks (device memory with room for `capacity` blocks; block i at d_blocks[i * 512 ...]: a
    // list for mergeBlocks) -> their number; capacity 0 only counts, too little room throws VH_ERR_BAD_ARGUMENT with
    // counts->c[VH_CUT_LIFTED] what is needed.  moveRegionTo extracts, merges the list into `dst` shifted by whole blocks
    // and erases the region here only if the merge left no block out: VH_ERR_HEAP_EXHAUSTED is thrown with both scenes
    // as they were, and after a merge status that leaves blocks out (VH_MERGE_NO_SLOT, VH_MERGE_NOT_SETTLED, in *merged)
    // it returns with this scene untouched.  All block until done, leave the compactified list stale after a write
    // (compactify before the next ray cast) and throw VH_ERR_BAD_ARGUMENT, with nothing done, for a region
    // vh_cut_region_transform refuses, a frame in flight and, for the move, dst == this and two voxel sizes.  *counts
    // (may be nullptr) is filled before any throw.  No block of this scene may be streamed out to a chunk grid (not
    // checked here: such blocks are not seen).
    typedef VhCutRegion CutRegion;
    struct CutCounts {
        unsigned int c[VH_CUT_NUM_COUNTS]; // indexed by VH_CUT_*
        unsigned int status() const { return c[VH_CUT_STATUS]; }
    };
    void eraseRegion(const CutRegion& region, CutCounts* counts = nullptr);
    void cropToRegion(const CutRegion& region, CutCounts* counts = nullptr);
    unsigned int extractRegion(const CutRegion& region, SDFBlockDesc* d_descs, Voxel* d_blocks, unsigned int capacity, CutCounts* counts = nullptr);
    void moveRegionTo(CUDASceneRepHashSDF& dst, const CutRegion& region, const int32_t blockOffset[3], CutCounts* counts = nullptr,
                      MergeCounts* merged = nullptr);
    // Frame de-integration (DESIGN.md section 4 "Frame de-integration"; vh_api.h has the rule of vh_deintegrate_blocks):
    // deintegrate takes the frame that integrate() fused at `rigidTransform` back out of the blocks resident in this
    // scene's table -- same maps, same camera -- and frees the blocks left without an observed voxel.  It works on a copy
    // of the hash parameters that carries the frame's pose: the scene's last rigid transform is not changed, nor is
    // the number of integrated frames.  reintegrate is deintegrate(oldTransform) followed by integrate(newTransform),
    // which counts as a frame.  Both block until done, leave the compactified list stale (compactify before the next
    // ray cast) and throw VH_ERR_BAD_ARGUMENT, with nothing done, for a frame in flight, a null depth or colour map and
    // an image without pixels.  *counts (may be nullptr) is filled before any throw.  The take-out is the inverse below
    // the weight cap and without a starve pass in between, and never for colours in the running-average mode.  No
    // block of this scene may be streamed out to a chunk grid (not checked here: such blocks are not seen).
    struct DeintegrateCounts {
        unsigned int c[VH_DEINT_NUM_COUNTS]; // indexed by VH_DEINT_*
        unsigned int status() const { return c[VH_DEINT_STATUS]; }
    };
    void deintegrate(const vh::mat4f& rigidTransform, const DepthCameraData& depthCameraData, const DepthCameraParams& depthCameraParams,
                     DeintegrateCounts* counts = nullptr);
    void reintegrate(const vh::mat4f& oldTransform, const vh::mat4f& newTransform, const DepthCameraData& depthCameraData,
                     const DepthCameraParams& depthCameraParams, const unsigned int* d_bitMask, DeintegrateCounts* counts = nullptr);
    const VhSceneOptions& getOptions() const { return m_options; }
    vhStream_t getStream() const { return m_stream; }
    int32_t nextLockToken(); // fresh bucket-lock epoch (replaces resetHashBucketMutexCUDA)
    void getState(uint32_t out[VH_STATE_WORDS]);
    void getTimings(double out[4]); // ms: alloc, compactify, integrate(+gc), frames
    unsigned int getNumIntegratedFrames() const { return m_numIntegratedFrames; }
    // between integrateAhead() and integrateFinish(): what the editing calls above refuse, for a caller that must refuse too
    bool frameInFlight() const { return m_aheadPending != 0; }

private:
    void create(const HashParams& params);
    void cutRegion(const CutRegion& region, uint32_t flags, SDFBlockDesc* d_outDescs, Voxel* d_staging, unsigned int stagingBlocks, CutCounts& c,
                   const char* what);
    // what the scene operations start from: a table's entries as a block list, after another scene's stream
    struct BlockList {
        vh::DevicePtr<SDFBlockDesc> descs;
        vh::DevicePtr<uint32_t> counter; // the helper's own count word: lives as long as the list, as it always has
        uint32_t capacity, n;
    };
    BlockList gatherBlockList(const CUDASceneRepHashSDF& of, const char* what, uint32_t* d_counter = nullptr);
    void refuseOverfull(uint32_t n, uint32_t capacity, const CUDASceneRepHashSDF& of, const char* what) const;
    vh::Event waitForStreamOf(const CUDASceneRepHashSDF& other);
    void alloc(const DepthCameraData&, const DepthCameraParams&, const unsigned int* d_bitMask, bool jobPrepared); // :247
    void compactifyHashEntries(const DepthCameraParams&);                                        // :282
    void integrateFused(const DepthCameraData&, const DepthCameraParams&);
    void integrateDepthMap(const DepthCameraData&, const DepthCameraParams&);                    // :317
    void garbageCollect(const DepthCameraParams&);                                               // :327
    void pollOccupiedCount(bool block);

    HashParams m_hashParams;
    HashData m_hashData; // filled by the C ABI's allocator (vh_hash_data_alloc); m_hashDataOwner gives it back
    struct HashDataFree { void operator()(HashData* hd) const noexcept; };
    std::unique_ptr<HashData, HashDataFree> m_hashDataOwner;
    VhSceneOptions m_options;
    vhStream_t m_stream;
    unsigned int m_numIntegratedFrames;
    int32_t m_lockEpoch;
    vh::Mapped<uint32_t> m_occupied; // the fused integrate kernel mirrors {block count, frame number} here (DESIGN.md "What the device tells the host")
    bool m_occupiedPending;   // a frame was enqueued since the host value was last known exact
    bool m_counterCleared;    // d_hashCompactifiedCounter is known to be 0 (k_alloc clears it)
    std::unique_ptr<VhStageTimer> m_timer;
    unsigned int m_tableEpoch;
    VhFrameJob m_job;         // alloc + compactify of the frame in progress
    int m_aheadPending;       // 0 none, 1 job prepared by integrateAhead()
    vh::DevicePtr<unsigned char> d_packedFrame; // the frame as the alloc pass packs it for the pass over the voxels (8 bytes per pixel)
    size_t m_packedPixels;
    vh::DevicePtr<uint32_t> d_riderDone; // VH_RIDER_DONE_WORDS words (see VhFrameJob::d_riderDone)
    uint32_t m_riderTotals[2]; // VhFrameJob::listDoneTotal, listClassTotal as of the last launch
    void keepRiderTotals();
    unsigned int m_riderMostBlocks;
    uint32_t fusedFlags() const;
    void prepareJob(const DepthCameraData&, const DepthCameraParams&, const unsigned int* d_bitMask);
};

// ---------------------------------------------------------------------------
class CUDARayCastSDF {
public:
    explicit CUDARayCastSDF(const RayCastParams& params, vhStream_t stream = nullptr);
    ~CUDARayCastSDF();
    CUDARayCastSDF(const CUDARayCastSDF&) = delete;
    CUDARayCastSDF& operator=(const CUDARayCastSDF&) = delete;

    // DSC/CUDARayCastSDF.cpp:38-72.  The reference skips the view-matrix
    // update while hashParams.m_numOccupiedBlocks == 0 (stale matrices); here
    // the given transform is always used.
    // coLaunch (not in the reference): a job of CUDASceneRepHashSDF::integrateAhead, whose alloc and compactify
    // passes then ride in this call's two launches
    void render(const HashData& hashData, const HashParams& hashParams, const DepthCameraParams& cameraParams,
                const vh::mat4f& lastRigidTransform, VhFrameJob* coLaunch = nullptr);
    const RayCastData& getRayCastData() { return m_data; }        // :42
    const RayCastParams& getRayCastParams() const { return m_params; } // :45
    // n rays given in world space through the model: vh_query_rays (vh_api.h has the semantics) with this caster's
    // increment and thresholds, on its stream.  Device pointers; d_normals may be nullptr.  Read-only, on the blocks
    // resident on the device; the caller must not run it beside an integrate on another stream.
    void castRays(const HashData& hashData, const HashParams& hashParams, const float* d_origins, const float* d_directions,
                  const float* d_tMin, const float* d_tMax, unsigned int n, float* d_t, float* d_normals, uint32_t* d_color,
                  uint8_t* d_status);

    // marchOnly: events around the march kernel only; stride n: only every n-th render() is timed
    void setTiming(bool on, bool marchOnly = false, unsigned int stride = 1);
    void getTimings(double out[4]); // ms: raycast (the march kernel), normals, frames, interval splat
    double getEventPairOverheadMs(); // average reading of an empty HIP event pair (taken while every stage is timed)
    // ray-interval splatting (DSC/CUDARayCastSDF.cpp:84-100, disabled in the reference fork): on by default here,
    // as a conservative compute pass that leaves every output bit unchanged
    void setIntervalSplatting(bool on) { m_useIntervals = on; }
    // render() calls so far that ran on an interval splat made ahead (inside the previous call's computeNormals launch)
    unsigned int getNumSplatsMadeAheadUsed() const { return m_preSplatsUsed; }
    // entries per tile list of the latest render(): VH_TILE_LIST_CAPACITY, or VH_TILE_LIST_CAPACITY_LARGE while fine voxels ask for it
    uint32_t getTileCapacity() const { return m_tileCapacity; }

private:
    RayCastParams m_params;
    RayCastData m_data; // the four maps below, as the kernels and the callers take them
    vh::DevicePtr<float> d_depth, d_depth4, d_normals, d_colors;
    vhStream_t m_stream;
    std::unique_ptr<VhStageTimer> m_timer;
    bool m_timeMarchOnly;
    unsigned int m_timeStride, m_renderCalls;
    vh::DevicePtr<uint32_t> d_tileHeads;     // {min, max camera depth, block count, 0} per 8x8-pixel tile
    vh::DevicePtr<VhTileBlock> d_tileBlocks; // up to VH_TILE_LIST_CAPACITY_LARGE blocks per tile
    vh::Mapped<uint32_t> m_longestList;      // longest tile list the ray caster met lately
    bool m_largeTables;        // current choice of table size
    uint32_t m_quietFrames, m_tileCapacity;
    uint32_t chooseTileCapacity(); // large tables as soon as a list outgrew the small ones, back after 30 frames without one
    vh::DevicePtr<uint32_t> d_schedule; // tiles by cost class, for the launch order of the next render()
    uint32_t m_phase;          // render() calls with intervals so far
    unsigned int m_preSplatsUsed;
    bool m_useIntervals;
    // the interval splat of the next render, made ahead inside this render's computeNormals launch (vh_compute_normals_co2)
    struct PreSplat {
        bool valid;
        float pose[16];         // the pose it was made for
        const void* table;      // d_hash of the scene
        uint32_t frameNumber, tableEpoch, phase, capacity;
    } m_preSplat;
};

// ---------------------------------------------------------------------------
class ChunkDesc { // DSC/CUDASceneRepChunkGrid.h:68-121
public:
    explicit ChunkDesc(unsigned int initialChunkListSize)
    {
        m_SDFBlocks.reserve(initialChunkListSize);
        m_ChunkDesc.reserve(initialChunkListSize);
    }
    void addSDFBlock(const SDFBlockDesc& desc, const vh::SDFBlock& data)
    {
        m_ChunkDesc.push_back(desc);
        m_SDFBlocks.push_back(data);
    }
    unsigned int getNElements() const { return (unsigned int)m_SDFBlocks.size(); }
    void clear() { m_ChunkDesc.clear(); m_SDFBlocks.clear(); }
    bool isStreamedOut() const { return !m_SDFBlocks.empty(); }
    std::vector<SDFBlockDesc>& getSDFBlockDescs() { return m_ChunkDesc; }
    std::vector<vh::SDFBlock>& getSDFBlocks() { return m_SDFBlocks; }
    const std::vector<SDFBlockDesc>& getSDFBlockDescs() const { return m_ChunkDesc; }
    const std::vector<vh::SDFBlock>& getSDFBlocks() const { return m_SDFBlocks; }

private:
    std::vector<vh::SDFBlock> m_SDFBlocks;
    std::vector<SDFBlockDesc> m_ChunkDesc;
};

class CUDASceneRepChunkGrid {
public:
    // DSC/CUDASceneRepChunkGrid.h:155
    CUDASceneRepChunkGrid(CUDASceneRepHashSDF* sceneRepHashSDF, const vh::vec3f& voxelExtends,
                          const vh::vec3i& gridDimensions, const vh::vec3i& minGridPos,
                          unsigned int initialChunkListSize, bool streamingEnabled, unsigned int streamOutParts);
    ~CUDASceneRepChunkGrid();
    CUDASceneRepChunkGrid(const CUDASceneRepChunkGrid&) = delete;
    CUDASceneRepChunkGrid& operator=(const CUDASceneRepChunkGrid&) = delete;

    // stream out (GPU -> host), DSC/CUDASceneRepChunkGrid.cpp:31-153
    void streamOutToCPUAll();
    void streamOutToCPU(const vh::vec3f& posCamera, float radius, bool useParts, unsigned int& nStreamedBlocks);
    void streamOutToCPUPass0GPU(const vh::vec3f& posCamera, float radius, bool useParts, bool multiThreaded = true);
    void streamOutToCPUPass1CPU(bool multiThreaded = true);
    void integrateInChunkGrid(const SDFBlockDesc* desc, const vh::SDFBlock* block, unsigned int nSDFBlocks);

    // stream in (host -> GPU), DSC/CUDASceneRepChunkGrid.cpp:155-311
    void streamInToGPUAll();
    void streamInToGPUAll(const vh::vec3f& posCamera, float radius, bool useParts, unsigned int& nStreamedBlocks);
    void streamInToGPUChunk(const vh::vec3i& chunkPos);
    void streamInToGPUChunkNeighborhood(const vh::vec3i& chunkPos, int kernelRadius);
    void streamInToGPU(const vh::vec3f& posCamera, float radius, bool useParts, unsigned int& nStreamedBlocks);
    void streamInToGPUPass0CPU(const vh::vec3f& posCamera, float radius, bool useParts, bool multiThreaded = true);
    void streamInToGPUPass1GPU(bool multiThreaded = true);

    // ---- the streaming step of a frame in which nothing streams, kept out of the frame's launches (no reference twin;
    // used by Reconstruction when it knows the next frame's pose).  probeStreamOut() enqueues the scan the NEXT stream-out
    // pass will make, counting only; probeResult() waits for its answer.  With the answer 0, streamOutNothing() is that
    // pass without its launches (same protocol with the worker thread, same part counter), and streamInWait() /
    // streamInFinish() are the two halves of streamInToGPUPass1GPU(true): the worker's answer first, the launches -- if
    // any block comes in -- wherever the caller's launch order wants them.
    void probeStreamOut(const vh::vec3f& posCamera, float radius, bool useParts);
    unsigned int probeResult();
    void streamOutNothing(const vh::vec3f& posCamera, float radius, bool useParts);
    unsigned int streamInWait();
    void streamInFinish();
    // after streamInWait(), instead of streamInFinish(): the blocks the worker has staged go back into the host grid,
    // nothing is launched, the worker gets its buffers and its event (for a caller that is unwinding)
    void streamInAbort();
    bool bitMaskDirty() const { return m_bitMaskDirty; }
    unsigned int integrateInHash(const vh::vec3f& posCamera, float radius, bool useParts);

    // ---- the streaming step of a frame without a host wait (not in the reference; used by Reconstruction for a sequence
    // whose poses are known a frame ahead).  The reference's step is a chain of four host <-> device round trips: the
    // stream-out count is read back before the blocks are copied, the host puts the blocks into its grid and only then knows
    // the bit mask the frame's alloc pass needs, the worker picks the chunk that comes in, the heap counter is read back
    // before it is inserted.  Here
    //   * the counts stay on the device (vh_stream_out_device / vh_stream_in_device), and the stream-out pass writes the
    //     blocks straight into mapped host memory;
    //   * the DEVICE's copy of the bit mask is kept by the passes themselves (a block that leaves sets its chunk's bit, a
    //     chunk that comes in clears it): what the frame's alloc pass reads is in place without the host;
    //   * the chunk that comes in at frame k+1 is chosen and uploaded by a worker thread while the device is still working
    //     on frame k.  It may be chosen that early: a chunk gains blocks at frame k+1 only from blocks OUTSIDE that frame's
    //     sphere, and a chunk with such a block does not lie entirely inside the sphere, so what leaves in a frame cannot
    //     be what comes in in the same frame (isChunkInSphere is the conservative test of the chunk's bounding sphere);
    //   * the blocks that left at frame k are put into the host grid by that worker when their copy has arrived, before it
    //     chooses for frame k+1 -- the one order the choice does depend on.
    // Per frame: pipelineDecision() (the worker's answer for this frame) -> [the ray cast] -> pipelineStreamOut() ->
    // pipelineStreamIn() -> [integrate with getBitMaskDevice()] -> pipelineAsk() (the job for the next frame).
    // Every other entry point of this class drains the pipeline first (pipelineDrain()).
    struct StreamDecision {
        unsigned int nIn;      // blocks of the chunk that comes in (0: none)
        unsigned int chunkBit; // its bit in the bit mask
        int slot;              // which staging buffer holds them
    };
    bool pipelineHasDecision(const vh::vec3f& posCamera, float radius) const; // was pipelineAsk() called for this frame's sphere?
    StreamDecision pipelineDecision();  // waits for the worker (it has had most of a frame)
    // enqueues the frame's stream-out pass for at most `mostBlocks` blocks (vh_stream_out_probe's count; 0: nothing is
    // launched) and advances the part counter; false if mostBlocks exceeds the pipeline's staging (the caller then takes the
    // reference's order of calls: pipelineDrain() and the classic methods)
    bool pipelineStreamOut(const vh::vec3f& posCamera, float radius, bool useParts, unsigned int mostBlocks);
    void pipelineStreamIn(const StreamDecision& d); // enqueues the insert of what the worker has uploaded
    // the job for the worker: take in what this frame's stream-out pass copies, then (haveNext) choose for the next frame
    void pipelineAsk(bool haveNext, const vh::vec3f& nextPosCamera, float nextRadius);
    // waits for the worker's job and looks at the outcome of finished inserts (files failures back into the grid).  undo: a choice that has
    // been made for a coming frame is put back into the grid (whoever looks at the host grid or takes the reference's order
    // of calls next must find it as the reference would have it at this point; the next frame then chooses again)
    void pipelineDrain(bool undo = true);
    void pipelineReturn(const StreamDecision& d, const vh::vec3f& posCamera, float radius); // hands an unused pipelineDecision() back
    unsigned int pipelineCapacity() const { return (unsigned int)kPipelineBlocks; }
    unsigned int* getBitMaskDevice() { return d_bitMask.get(); } // (current while the pipeline runs: no upload)
    void pipelineTotals(unsigned long long* blocksOut, unsigned long long* blocksIn); // drains; blocks moved by the pipeline so far
    // blocks that stream-in passes could not insert and that went back to the host grid (not in the reference)
    unsigned int getNumFailedInserts() const { return m_numFailedInserts; }

    void debugCheckForDuplicates() const; // .cpp:313-341; throws vh::Error
    void startMultiThreading();           // .h:248
    void stopMultiThreading();            // .h:262
    void clearGrid();                     // .h:291
    void reset();                         // .h:297
    // .h:306 -- uploads the bit mask only if it changed since the last call
    unsigned int* getBitMaskGPU();
    // read-only, for tests: drains the pipeline, then copies out the host's copy of the bit mask and the device's as they
    // stand -- before any upload of the host's copy -- and says whether the host's copy was marked dirty
    // (DESIGN.md "Fragile by design": the two copies agree whenever the pipeline is drained)
    void debugDownloadBitMasks(std::vector<unsigned int>& hostCopy, std::vector<unsigned int>& deviceCopy, bool& hostDirty);
    bool containsSDFBlocksChunk(const vh::vec3i& chunk) const;                               // .h:311
    bool isChunkInSphere(const vh::vec3i& chunk, const vh::vec3f& center, float radius) const; // .h:317
    bool containsSDFBlocksChunkInRadius(const vh::vec3i& chunk, int chunkRadius) const;      // .h:348

    HashData& getHashData() { return m_sceneRepHashSDF->getHashData(); }               // .h:287
    const HashParams& getHashParams() { return m_sceneRepHashSDF->getHashParams(); }   // .h:283
    const vh::vec3i& getMinGridPos() const { return m_minGridPos; }
    const vh::vec3i& getMaxGridPos() const { return m_maxGridPos; }
    const vh::vec3f& getVoxelExtends() const { return m_voxelExtents; }
    vh::vec3f getWorldPosChunk(const vh::vec3i& chunk) const { return chunkToWorld(chunk); }
    void getStatistics(unsigned int out[3]) const; // chunks, blocks on host, bits set

    // .hashgrid version 1, DSC/CUDASceneRepChunkGrid.h:456-548 (mLib BinaryDataStreamFile layout)
    void saveToFile(const std::string& filename, const vh::vec3f& camPos, float radius);
    void loadFromFile(const std::string& filename, const vh::vec3f& camPos, float radius);

    unsigned int getNumStreamedOutBlocks() const { return s_nStreamdOutBlocks; } // of the last pass 0
    unsigned int getNumStreamedInBlocks() const { return s_nStreamdInBlocks; }   // of the last pass 1
    const vh::vec3f& getPosCamera() const { return s_posCamera; }
    float getRadius() const { return s_radius; }
    bool getTerminatedThread() const { return s_terminateThread; }
    static const bool s_useParts = true;

    // host-side content (sorted by chunk index, insertion order inside a chunk)
    void downloadHostBlocks(std::vector<SDFBlockDesc>& descs, std::vector<vh::SDFBlock>& blocks) const;

    // helpers (private in the reference, .h:560-640)
    bool isValidChunk(const vh::vec3i& chunk) const;
    vh::vec3i worldToChunks(const vh::vec3f& posWorld) const;
    vh::vec3f chunkToWorld(const vh::vec3i& posChunk) const;
    vh::vec3i delinearizeChunkIndex(unsigned int idx) const;
    unsigned int linearizeChunkPos(const vh::vec3i& chunkPos) const;
    vh::vec3i meterToNumberOfChunksCeil(float f) const;
    float getChunkRadiusInMeter() const;
    float getGridRadiusInMeter() const;

private:
    struct AutoResetEvent { // Win32 auto-reset event (CreateEvent(NULL, FALSE, initial, NULL))
        std::mutex mtx;
        std::condition_variable cv;
        std::atomic<bool> signaled{ false };
        void set();
        void wait();
        void reset(bool state);
    };
    void workerLoop();
    void create(const vh::vec3f& voxelExtends, const vh::vec3i& gridDimensions, const vh::vec3i& minGridPos,
                unsigned int initialChunkListSize, bool streamingEnabled);
    void setBit(unsigned int index);
    void resetBit(unsigned int index);
    bool refileFailedInserts(int slot, const SDFBlockDesc* descs, const vh::SDFBlock* blocks, unsigned int& nIn);
    unsigned int integrateInHash(const vh::vec3f& posCamera, float radius, bool useParts, SDFBlockDesc* hDescs, vh::SDFBlock* hBlocks,
                                 SDFBlockDesc* dDescs, vh::SDFBlock* dBlocks, unsigned int capacity, unsigned int* chunkBit);
    // the pipeline (see above)
    enum { kPipelineBlocks = 4096 }; // staging capacity of a pipelined pass (16 MB per buffer)
    struct PipelineJob {
        bool haveOut, haveNext;
        uint32_t outMost;
        int outSlot, inSlot;
        vh::vec3f nextPos;
        float nextRadius;
    };
    void pipelineStart();
    void pipelineStop();
    void pipelineWorker();
    void pipelineCheckInsert(int slot, bool block);
    void pipelineAwaitWorker(); // until the worker has finished every job posted so far; VH_ERR_TIMEOUT after 40 s
    std::thread m_plThread;
    std::mutex m_plMutex;
    std::condition_variable m_plCv;
    bool m_plStarted;
    std::atomic<bool> m_plQuit; // (the worker looks at it in its spin, without the mutex)
    PipelineJob m_plJob;
    std::atomic<unsigned int> m_plPosted, m_plDone; // jobs handed to / finished by the worker
    std::atomic<int> m_plError;                     // a vh error code the worker ran into (reported by the next call)
    StreamDecision m_plDecision;                    // the finished job's choice
    bool m_plDecisionValid;                         // ... if it was asked for
    vh::vec3f m_plDecisionPos;                      // ... and the sphere it was asked for
    float m_plDecisionRadius;
    unsigned int m_plFrame;                         // frames the pipeline has run (slot = frame & 1)
    bool m_plOutThisFrame;                          // pipelineStreamOut() of the current frame launched a pass
    uint32_t m_plOutMost;
    struct { bool pending; unsigned int nIn; } m_plInsert[2]; // per staging slot: an insert whose outcome has not been looked at
    std::atomic<unsigned long long> m_plBlocksOut, m_plBlocksIn;
    vh::DevicePtr<SDFBlockDesc> d_plOutDesc[2];  // pass 1 -> pass 2 (device)
    vh::Mapped<SDFBlockDesc> m_plOutDesc[2];     // pass 2 writes the blocks it moves straight to the host
    vh::Mapped<vh::SDFBlock> m_plOutBlocks[2];
    vh::Published m_plOut[2]; // {count, 0, tag}: drawn by the main thread, awaited by the worker (never both: pipelineDecision() / pipelineDrain() lie between)
    vh::PinnedPtr<SDFBlockDesc> h_plInDesc[2];   // pinned staging of the worker's upload
    vh::PinnedPtr<vh::SDFBlock> h_plInBlocks[2];
    vh::DevicePtr<SDFBlockDesc> d_plInDesc[2];
    vh::DevicePtr<vh::SDFBlock> d_plInBlocks[2];
    void streamInLaunches();
    unsigned int m_numFailedInserts;
    // the outcome of a stream-in pass (vh_stream_in_device), mapped pinned {failed, 0, tag, exhausted, failed indices ...}: one
    // per pipeline slot, and kSyncInSlot for the passes of streamInLaunches() (DESIGN.md "What the device tells the host")
    enum { kSyncInSlot = 2 };
    vh::Published m_in[3];

    unsigned int m_maxNumberOfSDFBlocksIntegrateFromGlobalHash;

    vh::PinnedPtr<SDFBlockDesc> h_SDFBlockDescOutput;
    vh::PinnedPtr<vh::SDFBlock> h_SDFBlockOutput;
    vh::PinnedPtr<SDFBlockDesc> h_SDFBlockDescInput; // staging for the worker's H2D
    vh::PinnedPtr<vh::SDFBlock> h_SDFBlockInput;
    vh::Published m_mirror;             // {word 0, word 1, tag} published by the device (vh_publish_words)
    vh::Published m_probe;              // {count, 0, tag} of the stream-out probe
    vh::DevicePtr<unsigned int> d_probeCounter;
    std::unique_lock<std::mutex> m_streamInLock; // held between streamInWait() and streamInFinish()
    // returns once the device has published `record`'s tag on the scene's stream (spinSeconds 0: synchronises at once); throws whatIfNot if it never does
    void awaitPublished(const vh::Published& record, const char* whatIfNot, double spinSeconds = vh::kPublishSyncSeconds);
    // values of up to two device words once the stream has reached this point, without a blocking driver call
    void readBack(const unsigned int* d_word0, const unsigned int* d_word1, unsigned int* out0, unsigned int* out1);
    vh::DevicePtr<SDFBlockDesc> d_SDFBlockDescOutput;
    vh::DevicePtr<SDFBlockDesc> d_SDFBlockDescInput;
    vh::DevicePtr<vh::SDFBlock> d_SDFBlockOutput;
    vh::DevicePtr<vh::SDFBlock> d_SDFBlockInput;
    vh::DevicePtr<unsigned int> d_SDFBlockCounter;
    vh::DevicePtr<unsigned int> d_insertFailed; // vh_stream_in_device's scratch: {count, {index, SDF block} ...} of the blocks that found no slot
    vh::DevicePtr<unsigned int> d_bitMask;
    vh::Stream m_copyStream; // of the worker thread; declared behind the staging buffers, so it goes before them
    int m_device;       // HIP device the scene lives on (the worker thread binds to it)

    vh::vec3f m_voxelExtents;
    vh::vec3i m_gridDimensions;
    vh::vec3i m_minGridPos;
    vh::vec3i m_maxGridPos;
    unsigned int m_initialChunkDescListSize;

    std::unordered_map<unsigned int, std::unique_ptr<ChunkDesc>> m_grid; // sparse: chunk index -> chunk
    std::vector<unsigned int> m_bitMask;                                 // BitArray<unsigned int>, DSC/BitArray.h
    bool m_bitMaskDirty;
    mutable std::mutex m_gridMutex;

    unsigned int m_currentPart;
    struct PartWindow { unsigned int threadsPerPart, start; }; // hash entries the NEXT stream-out pass scans: the same for the pass, its probe and the pipelined pass
    PartWindow nextPartWindow(const HashParams& hp, bool useParts) const;
    unsigned int m_streamOutParts;

    std::thread m_thread;
    std::mutex hMutexOut, hMutexIn;
    AutoResetEvent hEventOutProduce, hEventOutConsume, hEventInProduce, hEventInConsume;

    vh::vec3f s_posCamera;
    float s_radius;
    unsigned int s_nStreamdInBlocks;
    unsigned int s_nStreamdOutBlocks;
    volatile bool s_terminateThread;

    CUDASceneRepHashSDF* m_sceneRepHashSDF;
};


// ---------------------------------------------------------------------------
// The frame loop: reconstruction() of DSC/DepthSensing.cpp:720-924 for a recorded sequence at given poses, as a
// class over the three host classes above (the reference keeps them in globals: g_sceneRep, g_rayCast, g_chunkGrid).
typedef VhReconstructionOptions ReconstructionOptions;
typedef VhSequenceFrame SequenceFrame;
typedef VhReconstructionStats ReconstructionStats;
typedef VhRawFrameFormat RawFrameFormat;
typedef VhRawSequenceFrame RawSequenceFrame;

class Reconstruction {
public:
    Reconstruction(CUDASceneRepHashSDF* sceneRep, CUDARayCastSDF* rayCast, CUDASceneRepChunkGrid* chunkGrid,
                   const DepthCameraParams& depthCameraParams, const ReconstructionOptions& options);
    ~Reconstruction();
    Reconstruction(const Reconstruction&) = delete;
    Reconstruction& operator=(const Reconstruction&) = delete;

    static ReconstructionOptions defaultOptions();
    // next: the frame that will follow frames[n-1] in a later call, if the caller knows it (only its pose is read)
    void run(const SequenceFrame* frames, unsigned int n, const SequenceFrame* next = nullptr);
    // raw frames (VhRawFrameFormat): 16-bit depth + 8-bit colour at the sensor's sizes, on the host (s_framesOnHost) or on
    // the device; converted, resampled and filtered into a staging slot on the copy stream.  The format is set once,
    // before the first frame.
    void setRawFormat(const RawFrameFormat& format);
    void runRaw(const RawSequenceFrame* frames, unsigned int n, const RawSequenceFrame* next = nullptr);
    // Camera tracking inside the loop (plain projective ICP): once, before the first frame.  From then on run() / runRaw()
    // ignore the frames' rigidTransform and do what reconstruction() does with s_binaryDumpSensorUseTrajectory = false,
    // s_trackingEnabled = true (DSC/DepthSensing.cpp:750-879): frame 0 at the identity; later frames ray-cast the model at
    // the scene's last pose, align the input to it and integrate at lastRigidTransform * delta; a lost frame is not
    // integrated.  The host waits once per tracked frame, for the ICP result in mapped host memory.
    void setTracking(const VhTrackingState& settings);
    // The same with the RGB-D tracker (CUDACameraTrackingMultiResRGBD: depth + photometric ICP, one vh_icp_rgbd_step per
    // iteration) in place of the plain one; one of the two, once.  Every frame then needs a colour map.
    void setTrackingRGBD(const VhTrackingStateRGBD& settings);
    bool isTracking() const { return m_tracking; }
    // frames integrated at a pose the loop tracked itself / frames on which tracking was lost, since creation or reset
    unsigned long long getNumTrackedFrames() const { return m_trackedFrames; }
    unsigned long long getNumLostFrames() const { return m_lostFrames; }
    // the pose every frame fed since creation / reset was integrated at, 16 floats each; -inf for a frame that was not
    const std::vector<float>& getPoses() const { return m_poses; }
    void synchronize();
    void reset();
    const ReconstructionStats& getStats();
    // test hook: the n-th ray cast from now throws instead of running (0: off) -- the loop's unwinding is tested with it
    void debugFailRender(unsigned int nthRenderFromNow) { m_debugFailRender = nthRenderFromNow; }

private:
    unsigned int m_debugFailRender;
    unsigned long long m_pipelineOutSeen, m_pipelineInSeen; // the grid's pipeline totals already in m_stats
    void frame(const SequenceFrame& f, const SequenceFrame* next);
    bool m_probePending;        // a stream-out probe for the frame with pose m_probePose is in the stream
    float m_probePose[16];
    DepthCameraData upload(const SequenceFrame& f);

    CUDASceneRepHashSDF* m_sceneRep;
    CUDARayCastSDF* m_rayCast;
    CUDASceneRepChunkGrid* m_chunkGrid;
    DepthCameraParams m_cp;
    ReconstructionOptions m_opt;
    ReconstructionStats m_stats;
    unsigned int m_frameNumber;
    // frames on the host: a ring of staging slots fed by a copy stream
    enum { kStagingSlots = 4 };
    // (the destructor's body waits for all three streams before any member below goes)
    vh::Stream m_copyStream;
    vh::Stream m_copyStream2;                     // the depth copy runs on a stream (a copy engine) of its own
    vh::DevicePtr<float> d_stageDepth[kStagingSlots];
    vh::DevicePtr<unsigned char> d_stageColorRaw[kStagingSlots];
    vh::DevicePtr<float> d_stageColor[kStagingSlots];
    vh::Event m_slotReady[kStagingSlots];         // copy stream -> main stream
    vh::Event m_slotReady2[kStagingSlots];
    unsigned int m_slotSceneFrame[kStagingSlots]; // the scene's frame count when the slot's frame was enqueued, + 1 (0: never used)
    unsigned int m_uploads;                       // frames uploaded so far (the slot is m_uploads % kStagingSlots)
    std::vector<std::pair<vh::Event, vh::Event>> m_uploadTimers; // event pairs on the copy stream, not yet read
    std::vector<vh::Event> m_timerPool;
    // raw frames: the sensor's images of a slot (host-fed), and the maps the filters read (one pair: the copy stream runs
    // one frame at a time)
    bool m_raw, m_rawRun;
    RawFrameFormat m_rawFormat;
    vh::DevicePtr<unsigned short> d_rawDepth[kStagingSlots];
    vh::DevicePtr<float> d_unfilteredDepth;
    vh::DevicePtr<float> d_unfilteredColor;
    std::vector<SequenceFrame> m_rawFrames;
    // the streaming step in the reference's order of calls (:881-900) around p -> the bit mask for alloc
    const unsigned int* streamAround(const vh::vec3f& p);
    std::vector<float> m_poses;
    // tracking: the solve (m_icp->estimate holds the identity), and what is the loop's own: the input's camera-space
    // positions, normals and coarser levels per staging slot (they depend on the frame alone: made on the copy stream
    // behind the ingest), the solve's outcome in mapped host memory and the tag the host waits for
    bool m_tracking;
    unsigned long long m_trackedFrames, m_lostFrames;
    VhTrackingState m_trackingState;
    std::unique_ptr<vh::IcpSolver> m_icp;
    std::vector<vh::DevicePtr<float>> d_trkInput[kStagingSlots], d_trkInputNormal[kStagingSlots];
    vh::Mapped<VhIcpResult> m_trkResult;
    uint32_t m_trkTag;
    // the RGB-D tracker in place of m_icp (m_tracking is set for either): its solve, and the input's intensity levels per
    // staging slot beside the positions and normals above
    VhTrackingStateRGBD m_trackingStateRGBD;
    std::unique_ptr<vh::IcpSolverRGBD> m_icpRGBD;
    std::vector<vh::DevicePtr<float>> d_trkIntensity[kStagingSlots], d_trkIntensityFiltered[kStagingSlots];
    void checkCanTrack(const char* who) const;
    void inputPyramid(unsigned int slot, const float* d_depth, const float* d_color, vhStream_t stream);
    void frameTracked(const SequenceFrame& f);
};

// ---------------------------------------------------------------------------
// CUDAMarchingCubesHashSDF (DSC/CUDAMarchingCubesHashSDF.h:8-67, .cpp:16-224): iso-surface extraction of the
// voxel hash into a triangle mesh, and the mesh file.
typedef VhMarchingCubesParams MarchingCubesParams;
typedef VhMarchingCubesData MarchingCubesData;

namespace vh {
// what the reference keeps in an mLib MeshDataf: vertices, per-vertex colours (r,g,b,1), index triples
struct MeshData {
    std::vector<vec3f> m_Vertices;
    std::vector<float> m_Colors;                      // 4 per vertex
    std::vector<unsigned int> m_FaceIndicesVertices;  // 3 per face; empty = triangle soup (face i = 3i, 3i+1, 3i+2)
    std::vector<float> m_Normals;                     // 3 per vertex, or none (the indexed extraction with setIndexedNormals)
    void clear() { m_Vertices.clear(); m_Colors.clear(); m_FaceIndicesVertices.clear(); m_Normals.clear(); }
    bool hasNormals() const { return !m_Vertices.empty() && m_Normals.size() == 3 * m_Vertices.size(); }
    bool hasVertexIndices() const { return !m_FaceIndicesVertices.empty(); }
    void makeTriangleSoupIndices();
    // MeshData::mergeCloseVertices(thresh, approx = true) / removeDuplicateFaces() / merge() / applyTransform() of the
    // mLib revision the reference vendors (DepthSensingCUDA/Include/mLib/include/core-mesh/meshData.{h,cpp})
    void mergeCloseVertices(float thresh);
    void removeDuplicateFaces();
    void merge(const MeshData& other);
    // normals go by the cofactor matrix of the upper-left 3x3 times the sign of its determinant, renormalised in double
    // (mLib's own rule divides them by a w that holds the translation: DESIGN.md, fenced reference defects)
    void applyTransform(const mat4f& t);
    // binary little endian, x y z [nx ny nz] red green blue alpha + faces (MLIB/core-mesh/meshIO.cpp:485-556)
    void saveToPLY(const std::string& filename) const;
};
} // namespace vh

struct VhMeshFinish;     // opaque: the passes over a welded mesh and their buffers (csrc/vh_mesh_finish.hpp)
struct VhMeshView;       // opaque: an indexed mesh on the device

class CUDAMarchingCubesHashSDF {
public:
    explicit CUDAMarchingCubesHashSDF(const MarchingCubesParams& params, vhStream_t stream = nullptr);
    ~CUDAMarchingCubesHashSDF();
    CUDAMarchingCubesHashSDF(const CUDAMarchingCubesHashSDF&) = delete;
    CUDAMarchingCubesHashSDF& operator=(const CUDAMarchingCubesHashSDF&) = delete;

    // parametersFromGlobalAppState, .h:19-28: the four GlobalAppState values it reads, as arguments
    static MarchingCubesParams parameters(unsigned int marchingCubesMaxNumTriangles, float SDFMarchingCubeThreshFactor,
                                          float SDFVoxelSize, unsigned int hashNumBuckets);

    void clearMeshBuffer() { m_meshData.clear(); clearWeldedMark(); } // (MeshData::clear takes the normals with it)
    // copies the result of the last extraction to the host and appends it to the mesh (.cpp:31-86); throws when the
    // triangle buffer overflowed.  offlineProcessing (GlobalAppState::s_offlineProcessing): merge each batch first.
    void copyTrianglesToCPU();
    void setOfflineProcessing(bool on) { m_offline = on; }
    void saveMesh(const std::string& filename, const vh::mat4f* transform = nullptr, bool overwriteExistingFile = false);

    // per chunk of the grid: stream the chunk and its neighbours in, extract inside the chunk's box (.cpp:149-192)
    void extractIsoSurface(CUDASceneRepChunkGrid& chunkGrid, const vh::vec3f& camPos, float radius);
    void extractIsoSurface(const HashData& hashData, const HashParams& hashParams, const vh::vec3f& minCorner = { 0, 0, 0 },
                           const vh::vec3f& maxCorner = { 0, 0, 0 }, bool boxEnabled = false);
    void extractIsoSurfaceWithoutCopy(const HashData& hashData, const HashParams& hashParams, const vh::vec3f& minCorner = { 0, 0, 0 },
                                      const vh::vec3f& maxCorner = { 0, 0, 0 }, bool boxEnabled = false);

    // Not in the reference: the extraction with the soup welded on the device ("Indexed mesh").
    // Runs reset, pass 1, the sourced pass 2, the weld and the download; REPLACES the mesh buffer with the indexed mesh
    // and marks it welded, so that saveMesh skips mergeCloseVertices / removeDuplicateFaces.  Whatever appends to the
    // buffer afterwards (copyTrianglesToCPU) clears the mark.  Throws VH_ERR_STAGING_OVERFLOW when the triangle buffer
    // overflowed or the weld table was full and VH_ERR_BAD_ARGUMENT when a lattice coordinate left the key range; the
    // buffer is then empty.
    void extractIsoSurfaceIndexed(const HashData& hashData, const HashParams& hashParams, const vh::vec3f& minCorner = { 0, 0, 0 },
                                  const vh::vec3f& maxCorner = { 0, 0, 0 }, bool boxEnabled = false);
    // The same box by box, for several extractions that make one mesh ("Indexed mesh over several
    // extractions"): beginIndexed starts an accumulation, appendIndexed runs reset, pass 1, the sourced pass 2 and the
    // overflow test of copyTrianglesToCPU in its box and appends the soup to the accumulating weld
    // (vh_mesh_weld_accum_append), finishIndexed downloads, REPLACES the mesh buffer and marks it welded.  Boxes may
    // overlap: a cell is taken from the first box that has it.  Errors as extractIsoSurfaceIndexed, buffer empty.
    void beginIndexed();
    void appendIndexed(const HashData& hashData, const HashParams& hashParams, const vh::vec3f& minCorner = { 0, 0, 0 },
                       const vh::vec3f& maxCorner = { 0, 0, 0 }, bool boxEnabled = false);
    void finishIndexed();
    // the walk of extractIsoSurface(chunkGrid, ...) with the same boxes, every chunk appended to one accumulation.  When
    // a chunk throws, the scene is streamed back in around camPos and the streaming thread restarted as at the normal
    // end, the mesh buffer is empty, the indexed counts are 0, and the error goes on to the caller.
    void extractIsoSurfaceIndexed(CUDASceneRepChunkGrid& chunkGrid, const vh::vec3f& camPos, float radius);
    // of the last accumulated extraction: the VH_WELD_ACCUM_NUM_COUNTS counts of vh_types.h; 0 after a one-shot one
    void getIndexedStats(unsigned int out[6]) const { for (int i = 0; i < 6; i++) out[i] = m_indexed.accumulated ? m_indexed.counts[i] : 0u; }
    bool isWelded() const { return m_welded; }
    void getIndexedCounts(unsigned int out[3]) const { for (int i = 0; i < 3; i++) out[i] = i < 2 && m_indexed.filtered ? m_indexed.kept[i] : i < 2 && m_indexed.clustered ? m_indexed.clusterStats[i] : m_indexed.counts[i]; }
    void downloadIndexed(VhVertex* vertices, uint64_t* keys, uint32_t* faces); // device mesh of the last indexed extraction
    // Vertex normals of the indexed mesh ("Vertex normals"), off by default.  When on, the three
    // indexed extractions run vh_mesh_vertex_normals after the weld -- finishIndexed over the whole accumulation -- with
    // the default scale of hashParams' voxel size, and put them into the mesh buffer's m_Normals, which saveMesh
    // writes.  A status of the pass throws VH_ERR_BAD_ARGUMENT and leaves the buffer empty.
    void setIndexedNormals(bool on) { m_indexedNormals = on; }
    void downloadIndexedNormals(float* normals); // 3 per vertex, in downloadIndexed's order; throws if that extraction had none
    // The component filter of the indexed mesh ("Mesh components"), off by default (0, false).
    // When on, readBackIndexed -- the one-shot extraction, finishIndexed and the chunk-grid walk alike -- labels the
    // welded mesh's connected components after the weld and the normals and keeps those of at least minFaces faces, with
    // largestOnly the largest of them alone: getIndexedCounts, downloadIndexed, downloadIndexedNormals, the mesh buffer
    // and saveMesh then describe the FILTERED mesh; what the unfiltered one held is in the component stats.  A status of
    // the labelling throws VH_ERR_BAD_ARGUMENT and leaves the buffer empty.
    void setIndexedComponentFilter(unsigned int minFaces, bool largestOnly) { m_componentMinFaces = minFaces; m_componentLargestOnly = largestOnly; }
    // the VH_COMPONENTS_NUM_COUNTS counts of the mesh in the buffer; 0 when it was made with the filter off, or is no longer the weld's
    void getIndexedComponentStats(unsigned int out[6]) const { for (int i = 0; i < 6; i++) out[i] = m_indexed.componentStats[i]; }
    // Decimation of the indexed mesh by vertex clustering ("Mesh clustering"), off by default (0).
    // With cellsPerCluster = 1 ... 64, readBackIndexed -- the one-shot extraction, finishIndexed and the chunk-grid walk
    // alike -- runs vh_mesh_cluster after the weld and BEFORE normals and components, which then work on the clustered
    // mesh: getIndexedCounts, downloadIndexed, downloadIndexedNormals, the mesh buffer and saveMesh describe the
    // clustered mesh (the filtered one, when the component filter is on too).  A status of the pass throws and leaves
    // the buffer empty.  Throws VH_ERR_BAD_ARGUMENT above 64.
    void setIndexedClustering(unsigned int cellsPerCluster);
    // the VH_CLUSTER_NUM_COUNTS counts of the mesh in the buffer; 0 when it was made with clustering off, or is no longer the weld's
    void getIndexedClusterStats(unsigned int out[6]) const { for (int i = 0; i < 6; i++) out[i] = m_indexed.clusterStats[i]; }
    // Taubin smoothing of the indexed mesh ("Mesh smoothing"), off by default (0 iterations).  With
    // iterations = 1 ... 100, readBackIndexed -- the one-shot extraction, finishIndexed and the chunk-grid walk alike --
    // runs vh_mesh_smooth AFTER the clustering and BEFORE normals and components, at the clustering's default scale of
    // the voxel size: downloadIndexed, the mesh buffer and saveMesh carry the smoothed positions, and the normals are
    // those of the smoothed surface (at the scale of twice the edge bound used without smoothing).  lambda and mu go to
    // units of 2^-16 by rint.  A status of the pass throws and leaves the buffer empty.  Throws VH_ERR_BAD_ARGUMENT
    // above 100 iterations and for a factor above 1 in magnitude.
    void setIndexedSmoothing(unsigned int iterations, float lambda = 0.5f, float mu = -0.53f, bool keepBoundary = true);
    void setIndexedSmoothingQ16(unsigned int iterations, int32_t lambdaQ16, int32_t muQ16, bool keepBoundary); // the same, the factors as the launcher takes them
    // the VH_SMOOTH_NUM_COUNTS counts of the mesh in the buffer; 0 when it was made with smoothing off, or is no longer the weld's
    void getIndexedSmoothStats(unsigned int out[6]) const { for (int i = 0; i < 6; i++) out[i] = m_indexed.smoothStats[i]; }
    void downloadSources(VhTriangleSource* out, unsigned int n);               // source records of the last indexed extraction

    // Not in the reference: the live mesh ("Live mesh").  Between liveBegin and liveEnd the object's
    // triangle buffer and source records are a cache that liveUpdate brings to exactly what the sourced pass 2 of
    // extractIsoSurfaceIndexed without a box would give on the table now (as a set; buffer order is free), re-extracting
    // only the resident blocks within one block of a block that changed since the last update (vh_live_mesh_update).
    // liveBegin empties the mesh buffer and the cache; every extraction on the object is then refused with
    // VH_ERR_BAD_ARGUMENT, with nothing done, until liveEnd.  liveUpdate fills counts (may be null) with the
    // VH_LIVE_NUM_COUNTS counts and the status word; it throws VH_ERR_STAGING_OVERFLOW when the cache overflowed and
    // VH_ERR_BAD_ARGUMENT when a block is out of range or the table malformed -- the cache is then invalid and the next
    // update starts from nothing -- and VH_ERR_BAD_ARGUMENT without liveBegin, with boxEnabled, or for hash parameters
    // other than the earlier updates', the cache then as it was.  liveInvalidate makes the next update a full one (the
    // digests can collide).  liveIndexed welds the cache and runs the indexed passes that are on, as
    // extractIsoSurfaceIndexed does after its pass 2: it REPLACES the mesh buffer and marks it welded; the cache stays.
    void liveBegin();
    void liveUpdate(const HashData& hashData, const HashParams& hashParams, unsigned int counts[VH_LIVE_NUM_COUNTS + 1] = nullptr, bool boxEnabled = false);
    void liveInvalidate();
    void liveIndexed();
    void liveEnd();
    bool isLive() const { return m_live; }

    const vh::MeshData& getMeshData() const { return m_meshData; }
    const MarchingCubesData& getMarchingCubesData() const { return m_data; }
    unsigned int getNumTriangles();       // of the last extraction (blocks); may exceed m_maxNumTriangles on overflow
    unsigned int getNumOccupiedBlocks();  // of the last extraction
    void downloadTriangles(VhTriangle* out, unsigned int n); // the device triangle buffer of the last extraction

private:
    MarchingCubesParams m_params;
    MarchingCubesData m_data; // filled by the C ABI's allocator (vh_marching_cubes_data_alloc); m_dataOwner gives it back
    struct DataFree { void operator()(MarchingCubesData* d) const noexcept; };
    std::unique_ptr<MarchingCubesData, DataFree> m_dataOwner;
    vh::MeshData m_meshData;
    vhStream_t m_stream;
    bool m_offline;
    // the steps the extractions share: reset, the box into m_params, pass 1 and pass 2 -- or the sourced pass 2, whose
    // records go to d_sources; then the triangle count (and that of the records if sourced), which throws when the buffer overflowed
    void runPasses(const HashData& hashData, const HashParams& hashParams, const vh::vec3f& minCorner, const vh::vec3f& maxCorner, bool boxEnabled, bool sourced);
    unsigned int countTriangles(bool sourced);
    // the walk of .cpp:149-192: perChunk(hashData, hashParams, minCorner, maxCorner) for every chunk that has blocks, with
    // its neighbourhood streamed in.  restoreOnError: when a chunk throws, the scene goes back as the normal end puts it.
    template <class F> void walkChunks(CUDASceneRepChunkGrid& chunkGrid, const vh::vec3f& camPos, float radius, bool restoreOnError, F&& perChunk);
    // indexed extraction: made by its first call.  The finish is one chain of passes over the welded mesh -- clustering,
    // smoothing, normals, components (csrc/vh_mesh_finish.hpp; DESIGN.md section 4, "The finish as one chain") -- which
    // owns every pass's buffers, each made by the first run with its option on: m_finish for the one-shot weld, the
    // accumulation's own for m_accum
    bool m_welded = false;                      // m_meshData is the weld's mesh, untouched since
    vh::DevicePtr<VhTriangleSource> d_sources;  // m_maxNumTriangles records beside m_data.d_triangles
    VhMeshWeldData m_weld;                      // from vh_mesh_weld_data_alloc; m_weldOwner gives it back
    struct WeldFree { void operator()(VhMeshWeldData* d) const noexcept; };
    std::unique_ptr<VhMeshWeldData, WeldFree> m_weldOwner;
    // accumulated indexed extraction: made by the first beginIndexed
    struct AccumFree { void operator()(VhMeshWeldAccum* a) const noexcept; };
    std::unique_ptr<VhMeshWeldAccum, AccumFree> m_accum;
    std::unique_ptr<VhMeshFinish> m_finish;     // (complete where the constructor and the destructor are: vh_marching_cubes.cpp)
    // the options of the finish, in the chain's order
    unsigned int m_clusterCells = 0;
    unsigned int m_smoothIterations = 0;
    int32_t m_smoothLambdaQ16 = VH_SMOOTH_DEFAULT_LAMBDA_Q16, m_smoothMuQ16 = VH_SMOOTH_DEFAULT_MU_Q16;
    bool m_smoothKeepBoundary = true;
    bool m_indexedNormals = false;
    unsigned int m_componentMinFaces = 0;
    bool m_componentLargestOnly = false;
    struct IndexedResult {                      // what the last indexed extraction left; the empty one is the state after an error
        unsigned int counts[VH_WELD_ACCUM_NUM_COUNTS] = { 0, 0, 0, 0, 0, 0 }; // {vertices, faces, status}, then the accumulation's three
        unsigned int numSourced = 0;            // triangles of its last sourced pass 2 that are in the buffer
        bool accumulated = false;               // begun by beginIndexed: the mesh and the chain are m_accum's, not m_weld's and m_finish
        bool hasNormals = false;                // it computed them
        float voxelSize = 0.0f;                 // of the last appendIndexed: finishIndexed's scale
        bool filtered = false;                  // the component filter ran: the mesh is kept[] = {vertices, faces} of the filter's own buffers
        unsigned int kept[2] = { 0, 0 };
        unsigned int componentStats[VH_COMPONENTS_NUM_COUNTS] = { 0, 0, 0, 0, 0, 0 };
        bool clustered = false;                 // the clustering ran: normals and components are of ITS mesh, clusterStats[0 .. 1] vertices and faces
        unsigned int clusterStats[VH_CLUSTER_NUM_COUNTS] = { 0, 0, 0, 0, 0, 0 };
        bool smoothed = false;                  // the smoothing ran: the vertices are those of ITS buffers, over the clustered or the welded mesh
        unsigned int smoothStats[VH_SMOOTH_NUM_COUNTS] = { 0, 0, 0, 0, 0, 0 };
    } m_indexed;
    void clearWeldedMark() { m_welded = false; for (unsigned int& c : m_indexed.componentStats) c = 0; for (unsigned int& c : m_indexed.clusterStats) c = 0; for (unsigned int& c : m_indexed.smoothStats) c = 0; }
    void resetIndexed() { clearMeshBuffer(); m_indexed = IndexedResult(); }
    // the welded mesh on the device (m_accum's, or m_weld's) through the stages of its chain that are on, at the scales
    // of that voxel size; one download of the mesh after the last stage into the mesh buffer; then its counts and marks
    void readBackIndexed(unsigned int numVertices, unsigned int numFaces, bool accumulated, float voxelSize);
    VhMeshFinish& indexedChain(bool accumulated);
    VhMeshView indexedBase(bool accumulated, unsigned int numVertices, unsigned int numFaces) const;
    VhMeshView indexedView(const char* what);   // what downloadIndexed and downloadIndexedNormals read
    // the one-shot weld of the nTriangles triangles and records in the buffers, then readBackIndexed
    void weldAndReadBack(unsigned int nTriangles, float voxelSize);
    // live mesh: the buffers are made by the first liveBegin
    bool m_live = false, m_liveValid = false;   // between liveBegin and liveEnd; the last update ended without a status
    float m_liveVoxelSize = 0.0f;               // of the last update: liveIndexed's scale
    VhLiveMeshData m_liveData;                  // from vh_live_mesh_data_alloc; m_liveOwner gives it back
    struct LiveFree { void operator()(VhLiveMeshData* d) const noexcept; };
    std::unique_ptr<VhLiveMeshData, LiveFree> m_liveOwner;
    void refuseWhileLive(const char* what) const;
};


// ---------------------------------------------------------------------------
// Recorded sequences: ml::SensorData, the `.sens` container (DSC/sensorData/sensorData.h), and
// SensorDataReader (DSC/SensorDataReader.{h,cpp}).  Host side; see voxelhashing_amd/csrc/vh_sensor_data.cpp.
namespace vh {

class SensorData {
public:
    static const uint32_t kVersion = 4; // M_SENSOR_DATA_VERSION, sensorData.h:607
    enum COMPRESSION_TYPE_COLOR { TYPE_RAW = 0, TYPE_PNG = 1, TYPE_JPEG = 2 };                     // :217-221
    enum COMPRESSION_TYPE_DEPTH { TYPE_RAW_USHORT = 0, TYPE_ZLIB_USHORT = 1, TYPE_OCCI_USHORT = 2 }; // :222-226
    struct RGBDFrame { // :229-551
        std::vector<uint8_t> m_colorCompressed, m_depthCompressed;
        uint64_t m_timeStampColor = 0, m_timeStampDepth = 0; // microseconds by convention
        mat4f m_cameraToWorld;
    };
    struct IMUFrame { // :553-605: 15 doubles and a time stamp, 128 bytes in the file
        double rotationRate[3], acceleration[3], magneticField[3], attitude[3], gravity[3];
        uint64_t timeStamp;
    };

    SensorData();
    static mat4f makeIntrinsicMatrix(float fx, float fy, float mx, float my);
    void loadFromFile(const std::string& filename); // throws vh::Error: VH_ERR_IO, VH_ERR_VERSION_MISMATCH
    void saveToFile(const std::string& filename) const;
    // compresses with the file's compression types: depth raw / zlib; colour raw only (NULL = frame without colour)
    void addFrame(const uint8_t* colorRGB, const uint16_t* depth, const mat4f& cameraToWorld = mat4f::identity(),
                  uint64_t timeStampColor = 0, uint64_t timeStampDepth = 0);
    void decompressDepth(size_t frameIdx, uint16_t* out) const;   // depthWidth*depthHeight samples
    void decompressColor(size_t frameIdx, uint8_t* outRGB) const; // colorWidth*colorHeight*3 bytes; raw, PNG, baseline JPEG

    uint32_t m_versionNumber;
    std::string m_sensorName;
    mat4f m_colorIntrinsic, m_colorExtrinsic, m_depthIntrinsic, m_depthExtrinsic; // CalibrationData :150-215
    int32_t m_colorCompressionType, m_depthCompressionType;
    uint32_t m_colorWidth, m_colorHeight, m_depthWidth, m_depthHeight;
    float m_depthShift; // depth in metres = sample / m_depthShift
    std::vector<RGBDFrame> m_frames;
    std::vector<IMUFrame> m_IMUFrames;
};

class SensorDataReader { // the RGBDSensor the frame loop polls when s_sensorIdx selects a recorded sequence
public:
    SensorDataReader();
    void createFirstConnected(const std::string& filename);
    bool processDepth(); // decodes the next frame; false once the sequence is complete
    const float* getDepthFloat() const { return m_depthFloat.data(); }    // metres, 0 = no measurement
    const uint8_t* getColorRGBX() const { return m_colorRGBX.data(); }    // {r, g, b, 1}
    mat4f getRigidTransform(int offset = 0) const;                        // recorded pose of the frame last decoded
    unsigned int getNumFrames() const { return m_numFrames; }
    unsigned int getCurrFrame() const { return m_currFrame; }
    bool hasColorData() const { return m_bHasColorData; }
    const SensorData& getSensorData() const;

private:
    std::unique_ptr<SensorData> m_sensorData;
    std::vector<float> m_depthFloat;
    std::vector<uint8_t> m_colorRGBX, m_colorRGB;
    std::vector<uint16_t> m_depthShorts;
    unsigned int m_numFrames, m_currFrame;
    bool m_bHasColorData;
};

} // namespace vh

// ---------------------------------------------------------------------------
// CUDARGBDSensor over CUDARGBDAdapter (DSC/CUDARGBDSensor.{h,cpp}, DSC/CUDARGBDAdapter.{h,cpp}): the image path from
// a sensor frame (float depth in metres + RGBX bytes, host memory, as RGBDSensor::getDepthFloat / getColorRGBX
// deliver them) to the DepthCameraData that integrate() consumes, plus the camera-space and normal maps tracking uses.
class CUDARGBDSensor {
public:
    struct Config {
        unsigned int depthWidth, depthHeight, colorWidth, colorHeight; // sensor images
        unsigned int adapterWidth, adapterHeight;                      // s_adapterWidth / s_adapterHeight: working resolution
        float fx, fy, mx, my;                                          // depth intrinsics at sensor resolution
        float sensorDepthMin, sensorDepthMax;                          // s_sensorDepthMin / s_sensorDepthMax
        bool filterDepth; float sigmaD, sigmaR;                        // s_depthFilter, s_depthSigmaD, s_depthSigmaR
        bool filterIntensity; float sigmaDIntensity, sigmaRIntensity;  // s_colorFilter, s_colorSigmaD, s_colorSigmaR
    };
    explicit CUDARGBDSensor(const Config& config, vhStream_t stream = nullptr);
    ~CUDARGBDSensor();
    CUDARGBDSensor(const CUDARGBDSensor&) = delete;
    CUDARGBDSensor& operator=(const CUDARGBDSensor&) = delete;

    void process(const float* h_depthFloat, const unsigned char* h_colorRGBX); // CUDARGBDSensor::process :147 (blocks until done)
    void setFiterDepthValues(bool b = true, float sigmaD = 1.0f, float sigmaR = 1.0f);     // (sic) .h:37
    void setFiterIntensityValues(bool b = true, float sigmaD = 1.0f, float sigmaR = 1.0f); // (sic) .h:40
    // s_bUseCameraCalibration (CUDARGBDSensor.cpp:198-217): process() renders the depth map into the colour camera
    // (RenderDepthMap with the adapter's inverse depth intrinsics, depthExtrinsics as the modelview and the adapter's
    // colour intrinsics; render target 0 into d_depthData).  Colour intrinsics at the colour sensor's resolution.  An
    // identity extrinsic leaves it off ("already aligned", RGBDSensor.cpp:150-153).  The DepthCameraParams keep the depth
    // intrinsics, as in the reference (.cpp:133-140).
    void setCameraCalibration(bool enabled, float colorFx, float colorFy, float colorMx, float colorMy, const vh::mat4f& depthExtrinsics,
                              float thresOffset, float thresLin);
    bool getCameraCalibration() const { return m_bUseCameraCalibration; } // what took effect
    const VhViewParams& getRemapParams() const { return m_remapParams; }

    const DepthCameraData& getDepthCameraData() const { return m_depthCameraData; }       // .h:78
    const DepthCameraParams& getDepthCameraParams() const { return m_depthCameraParams; } // .h:82
    float* getCameraSpacePositionsFloat4() { return d_cameraSpaceFloat4.get(); }          // .h:50
    float* getNormalMapFloat4() { return d_normalMapFloat4.get(); }                       // .h:53
    float* getDepthMapColorSpaceFloat() { return d_depthData.get(); }                     // .h:44
    float* getColorMapFilteredFloat4() { return d_colorData.get(); }                      // .h:47
    float* getIntensityMapFilteredFloat() { return d_intensityMapFilteredFloat.get(); }
    unsigned int getDepthWidth() const { return m_cfg.adapterWidth; }
    unsigned int getDepthHeight() const { return m_cfg.adapterHeight; }
    unsigned int getFrameNumber() const { return m_frameNumber; }

private:
    Config m_cfg;
    vhStream_t m_stream;
    unsigned int m_frameNumber;
    bool m_bFilterDepthValues, m_bFilterIntensityValues;
    float m_fBilateralFilterSigmaD, m_fBilateralFilterSigmaR, m_fBilateralFilterSigmaDIntensity, m_fBilateralFilterSigmaRIntensity;
    DepthCameraParams m_depthCameraParams;
    DepthCameraData m_depthCameraData;
    vh::DevicePtr<float> d_depthMapFloat, d_depthMapResampledFloat, d_depthMapFilteredFloat, d_intensityMapFilteredFloat;
    vh::DevicePtr<unsigned char> d_colorMapRaw;
    vh::DevicePtr<float> d_colorMapFloat4, d_colorMapResampledFloat4, d_cameraSpaceFloat4, d_normalMapFloat4;
    vh::DevicePtr<float> d_depthData, d_colorData; // what m_depthCameraData points to
    bool m_bUseCameraCalibration = false;
    VhViewParams m_remapParams;               // the RenderDepthMap arguments of the remap
    vh::DevicePtr<uint64_t> d_remapKeys;      // adapter-size key buffer, all ones between frames
    vh::DevicePtr<uint32_t> d_remapLargeList; // vh_view_large_list_words(adapter size), counter 0 between frames
};


// ---------------------------------------------------------------------------
// CUDACameraTrackingMultiRes (DSC/CUDACameraTrackingMultiRes.{h,cpp}): coarse-to-fine projective point-to-plane ICP of
// the sensor frame (camera-space positions + normals) against the ray-cast model maps.  The per-level settings the
// reference takes from GlobalCameraTrackingState (and passes in five vectors) travel as one VhTrackingState.
class CUDACameraTrackingMultiRes {
public:
    CUDACameraTrackingMultiRes(unsigned int imageWidth, unsigned int imageHeight, unsigned int levels, vhStream_t stream = nullptr);
    ~CUDACameraTrackingMultiRes();
    CUDACameraTrackingMultiRes(const CUDACameraTrackingMultiRes&) = delete;
    CUDACameraTrackingMultiRes& operator=(const CUDACameraTrackingMultiRes&) = delete;

    // applyCT :241-289.  Returns lastTransform * delta; a matrix of -inf when tracking was lost (isTrackingLost).
    vh::mat4f applyCT(float* dInput, float* dInputNormals, float* dModel, float* dModelNormals, const vh::mat4f& lastTransform,
                      const VhTrackingState& settings, const vh::mat4f& deltaTransformEstimate, const DepthCameraParams& depthCameraParams);
    static bool isTrackingLost(const vh::mat4f& m);
    const VhIcpState& getLastState() const { return m_lastState; } // LinearSystemConfidence of the last solve + iteration count
    unsigned int getLevels() const { return m_levels; }

private:
    unsigned int m_levels;
    vhStream_t m_stream;
    vh::IcpSolver m_icp;
    std::vector<vh::DevicePtr<float>> d_input, d_inputNormal; // levels >= 1: the finest level is the caller's maps
    VhIcpState m_lastState;
};

// ---------------------------------------------------------------------------
// CUDACameraTrackingMultiResRGBD (DSC/CUDACameraTrackingMultiResRGBD.{h,cpp}): coarse-to-fine ICP with a point-to-plane
// and a photometric term per pixel, linearised in Euler angles.  Where the geometry leaves a motion unconstrained (a
// wall, a floor, a table top) the model's intensity gradients still pin it.  The per-level settings travel as one
// VhTrackingStateRGBD; the sensor's depth-range maximum comes from the DepthCameraParams.
class CUDACameraTrackingMultiResRGBD {
public:
    CUDACameraTrackingMultiResRGBD(unsigned int imageWidth, unsigned int imageHeight, unsigned int levels, vhStream_t stream = nullptr);
    ~CUDACameraTrackingMultiResRGBD();
    CUDACameraTrackingMultiResRGBD(const CUDACameraTrackingMultiResRGBD&) = delete;
    CUDACameraTrackingMultiResRGBD& operator=(const CUDACameraTrackingMultiResRGBD&) = delete;

    // applyCT :239-327.  dInputColor: the sensor's float4 colour map (getColorMapFilteredFloat4); dModel*: the ray
    // caster's d_depth4, d_normals and d_colors.  Returns lastTransform * delta; a matrix of -inf when tracking was lost.
    vh::mat4f applyCT(float* dInput, float* dInputNormals, float* dInputColor, float* dModel, float* dModelNormals, float* dModelColor,
                      const vh::mat4f& lastTransform, const VhTrackingStateRGBD& settings, const vh::mat4f& deltaTransformEstimate,
                      const DepthCameraParams& depthCameraParams);
    static bool isTrackingLost(const vh::mat4f& m);
    const VhIcpStateRGBD& getLastState() const { return m_lastState; }
    unsigned int getLevels() const { return m_levels; }

private:
    unsigned int m_levels;
    vhStream_t m_stream;
    vh::IcpSolverRGBD m_icp;
    std::vector<vh::DevicePtr<float>> d_input, d_inputNormal, d_inputIntensity, d_inputIntensityFiltered; // (levels >= 1 of all but the third)
    VhIcpStateRGBD m_lastState;
};

// ---------------------------------------------------------------------------
// DX11RGBDRenderer (DSC/DX11RGBDRenderer.h): a depth map drawn as a mesh, two triangles per pixel quad, into four
// screen-size maps.  The D3D pipeline becomes three compute passes (vh_view_raster / vh_view_resolve); the maps stay on
// the device and are overwritten by the next call.
class RGBDRenderer {
public:
    explicit RGBDRenderer(vhStream_t stream = nullptr);
    ~RGBDRenderer();
    RGBDRenderer(const RGBDRenderer&) = delete;
    RGBDRenderer& operator=(const RGBDRenderer&) = delete;

    // RenderDepthMap :197-275 minus the device context
    void RenderDepthMap(const float* d_depthMap, const float* d_colorMap, unsigned int width, unsigned int height, const vh::mat4f& intrinsicDepthToWorld,
                        const vh::mat4f& modelview, const vh::mat4f& intrinsicWorldToDepth, unsigned int screenWidth, unsigned int screenHeight,
                        float depthThreshOffset, float depthThreshLin);
    float* getDepth() const { return d_depth.get(); }
    float* getPositions() const { return d_positions.get(); }
    float* getNormals() const { return d_normals.get(); }
    float* getColors() const { return d_colors.get(); }
    unsigned int getWidth() const { return m_screenWidth; }
    unsigned int getHeight() const { return m_screenHeight; }

private:
    void resize(unsigned int width, unsigned int height, unsigned int screenWidth, unsigned int screenHeight);
    vhStream_t m_stream;
    unsigned int m_width = 0, m_height = 0, m_screenWidth = 0, m_screenHeight = 0;
    vh::DevicePtr<uint64_t> d_keys;
    vh::DevicePtr<uint32_t> d_largeList;
    vh::DevicePtr<float> d_depth, d_positions, d_normals, d_colors;
};

// DX11PhongLighting (DSC/DX11PhongLighting.h): PhongPS over three float4 maps into a float4 target, and on request its
// RGBA8 form as renderToFile writes it.  The light is the ConstantBufferLight (vh_phong_light_from_render_state).
class PhongLighting {
public:
    explicit PhongLighting(const VhPhongLight& light, vhStream_t stream = nullptr);
    ~PhongLighting();
    PhongLighting(const PhongLighting&) = delete;
    PhongLighting& operator=(const PhongLighting&) = delete;

    // render(float4* d_positions, float4* d_normals, float4* d_colors, useMaterial, width, height) :42
    void render(const float* d_positions, const float* d_normals, const float* d_colors, bool useMaterial, unsigned int width, unsigned int height,
                bool rgba8 = false);
    void setLight(const VhPhongLight& light) { m_light = light; }
    const VhPhongLight& getLight() const { return m_light; }
    float* getColors() const { return d_colors.get(); }
    uint8_t* getColorsRGBA8() const { return d_rgba8.get(); }

private:
    VhPhongLight m_light;
    vhStream_t m_stream;
    unsigned int m_numPixels = 0;
    vh::DevicePtr<float> d_colors;
    vh::DevicePtr<uint8_t> d_rgba8;
};

#endif // VH_HPP
