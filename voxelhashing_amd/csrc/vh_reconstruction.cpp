// vh_reconstruction.cpp -- the frame loop of the reference application, reconstruction()
// (DSC/DepthSensing.cpp:720-924), for a recorded sequence at given poses, behind the C ABI: one host call enqueues any
// number of frames (the build's headless driver).  DSC/ = /root/reference/DepthSensingCUDA/Source/.
//
// Per frame, in the reference's order:
//   render(pose of the previous frame)                         :750-763
//   [stream out around the camera; stream in]                  :881-900
//   integrate(pose, depth, colour, bit mask)                   :903
// What is not in the reference:
//   * s_allocAhead: the pose of frame k is known before pose k-1 is ray-cast (it comes from the file), so the frame's
//     alloc pass rides in the ray caster's launch (its last workgroups) and its compactify pass, with the next pose's
//     interval splat, in computeNormals' (CUDASceneRepHashSDF::integrateAhead hands out the job) -- and, up to 2048 blocks in view, the pass over the
//     voxels there too: two launches, else three, per
//     frame on ONE stream, no event.  With streaming on this happens in the frames whose streaming step is known a
//     frame ahead to be a no-op (vh_stream_out_probe; frame() below);
//   * s_framesOnHost: float depth + RGBX colour in host memory (what RGBDSensor::getDepthFloat / getColorRGBX hand
//     to CUDARGBDAdapter::process, DSC/CUDARGBDAdapter.cpp:107-131) are uploaded by two copy streams (one copy engine
//     each: depth, colour) into a ring of kStagingSlots = 4 staging slots, beside the previous frames' work, and the
//     colour is converted there (convertColorRawToFloat4);
//   * raw frames (setRawFormat / runRaw): 16-bit depth + RGB or RGBX bytes at the sensor's sizes, what a sensor or a
//     `.sens` file holds before SensorDataReader::processDepth and CUDARGBDAdapter::process.  From the host they travel
//     by the same two copy streams (5 or 6 bytes per sensor pixel instead of 8), from device memory they are read in
//     place; the copy stream then runs vh_ingest_frame (conversion + resampling to adapter size in one pass) and the
//     Gauss filters of CUDARGBDSensor::process that are on, into the staging slot;
//   * s_maxFramesInFlight: the host stays at most that many frames ahead of the device (polled through the mapped
//     frame counter the fused integrate pass writes: no event).
//   * setTracking: the pose of a frame comes from projective ICP against the ray cast of the model (:750-879 with
//     s_binaryDumpSensorUseTrajectory = false), enqueued on the loop's stream with one launch per iteration
//     (vh_icp_step); the host learns the pose from mapped host memory (frameTracked() below).
//   * setTrackingRGBD: the same frame with the RGB-D tracker (CUDACameraTrackingMultiResRGBD, vh_icp_rgbd_step): the
//     input's intensity pyramid is made per staging slot on the copy stream, the model's behind the ray cast.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>

#include "vh_handles.hpp"
#include "vh_host_util.hpp"

namespace {

inline double now()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

} // namespace

ReconstructionOptions Reconstruction::defaultOptions()
{
    ReconstructionOptions o;
    std::memset(&o, 0, sizeof(o));
    o.s_streamingEnabled = 0;
    o.s_integrationEnabled = 1;
    o.s_offlineProcessing = 0;
    o.s_renderEnabled = 1;
    o.s_allocAhead = 1;
    o.s_framesOnHost = 0;
    o.s_maxFramesInFlight = 16;
    o.s_streamingPos[0] = o.s_streamingPos[1] = 0.0f;
    o.s_streamingPos[2] = 3.0f; // zParametersDefault.txt: s_streamingPos
    o.s_streamingRadius = 4.0f;
    return o;
}

Reconstruction::Reconstruction(CUDASceneRepHashSDF* sceneRep, CUDARayCastSDF* rayCast, CUDASceneRepChunkGrid* chunkGrid,
                               const DepthCameraParams& cp, const ReconstructionOptions& options)
    : m_sceneRep(sceneRep), m_rayCast(rayCast), m_chunkGrid(chunkGrid), m_cp(cp), m_opt(options), m_frameNumber(0)
{
    m_debugFailRender = 0;
    m_pipelineOutSeen = m_pipelineInSeen = 0;
    if (chunkGrid) chunkGrid->pipelineTotals(&m_pipelineOutSeen, &m_pipelineInSeen);
    if (!sceneRep) throw vh::Error(VH_ERR_BAD_ARGUMENT, "Reconstruction: no scene");
    if (options.s_streamingEnabled && !chunkGrid) throw vh::Error(VH_ERR_BAD_ARGUMENT, "Reconstruction: streaming needs a chunk grid");
    if (options.s_renderEnabled && !rayCast) throw vh::Error(VH_ERR_BAD_ARGUMENT, "Reconstruction: rendering needs a ray caster");
    std::memset(&m_stats, 0, sizeof(m_stats));
    for (int i = 0; i < kStagingSlots; i++) m_slotSceneFrame[i] = 0;
    m_uploads = 0;
    m_raw = m_rawRun = false;
    std::memset(&m_rawFormat, 0, sizeof(m_rawFormat));
    m_probePending = false;
    std::memset(m_probePose, 0, sizeof(m_probePose));
    m_tracking = false;
    m_trackedFrames = m_lostFrames = 0;
    std::memset(&m_trackingState, 0, sizeof(m_trackingState));
    std::memset(&m_trackingStateRGBD, 0, sizeof(m_trackingStateRGBD));
    m_trkTag = 0;
    if (m_opt.s_framesOnHost) {
        const size_t n = (size_t)cp.m_imageWidth * cp.m_imageHeight;
        m_copyStream = vh::makeStream("hipStreamCreate");
        m_copyStream2 = vh::makeStream("hipStreamCreate");
        for (int i = 0; i < kStagingSlots; i++) {
            d_stageDepth[i] = vh::deviceAlloc<float>(n, "staging depth");
            d_stageColorRaw[i] = vh::deviceAlloc<unsigned char>(4 * (n ? n : 1), "staging colour (raw)");
            d_stageColor[i] = vh::deviceAlloc<float>(4 * (n ? n : 1), "staging colour");
            m_slotReady[i] = vh::makeEvent(false);
            m_slotReady2[i] = vh::makeEvent(false);
        }
        m_stats.uploadBytes = (sizeof(float) + 4) * n;
    }
}

// (synchronize() waits for the copy streams and the main stream: then the members go, buffers and events before the streams)
Reconstruction::~Reconstruction()
{
    try { synchronize(); } catch (...) {}
}

// Raw mode owns the copy streams and the staging ring in both residencies: the ingest kernel writes the slot's maps
// whether the sensor's images came over the link or were on the device already.
void Reconstruction::setRawFormat(const RawFrameFormat& f)
{
    if (m_raw) throw vh::Error(VH_ERR_BAD_ARGUMENT, "Reconstruction::setRawFormat: the format is already set");
    if (m_stats.frames || m_stats.invalidFrames || m_uploads) throw vh::Error(VH_ERR_BAD_ARGUMENT, "Reconstruction::setRawFormat: frames have been processed already");
    const unsigned int W = m_cp.m_imageWidth, H = m_cp.m_imageHeight;
    // the resampler's scale is (in - 1) / (out - 1)
    if (W < 2 || H < 2) throw vh::Error(VH_ERR_BAD_ARGUMENT, "Reconstruction::setRawFormat: the adapter size must be at least 2x2");
    if (f.depthWidth < 2 || f.depthHeight < 2) throw vh::Error(VH_ERR_BAD_ARGUMENT, "Reconstruction::setRawFormat: the depth size must be at least 2x2");
    if (f.colorChannels != 0 && f.colorChannels != 3 && f.colorChannels != 4) throw vh::Error(VH_ERR_BAD_ARGUMENT, "Reconstruction::setRawFormat: colorChannels must be 0, 3 or 4");
    if (m_icpRGBD && !f.colorChannels) throw vh::Error(VH_ERR_BAD_ARGUMENT, "Reconstruction::setRawFormat: the RGB-D tracker needs a colour image");
    if (f.colorChannels && (f.colorWidth < 2 || f.colorHeight < 2)) throw vh::Error(VH_ERR_BAD_ARGUMENT, "Reconstruction::setRawFormat: the colour size must be at least 2x2");
    if (!(f.depthShift > 0.0f) || !std::isfinite(f.depthShift)) throw vh::Error(VH_ERR_BAD_ARGUMENT, "Reconstruction::setRawFormat: depthShift must be positive and finite");
    auto sigmaOk = [](float s) { return s > 0.0f && std::isfinite(s); };
    if (f.s_depthFilter && !(sigmaOk(f.s_depthSigmaD) && sigmaOk(f.s_depthSigmaR))) throw vh::Error(VH_ERR_BAD_ARGUMENT, "Reconstruction::setRawFormat: the depth filter needs positive sigmas");
    if (f.s_colorFilter && !(sigmaOk(f.s_colorSigmaD) && sigmaOk(f.s_colorSigmaR))) throw vh::Error(VH_ERR_BAD_ARGUMENT, "Reconstruction::setRawFormat: the colour filter needs positive sigmas");
    const size_t n = (size_t)W * H, nDepth = (size_t)f.depthWidth * f.depthHeight;
    const size_t colorBytes = f.colorChannels ? (size_t)f.colorChannels * f.colorWidth * f.colorHeight : 0;
    // everything that is not there yet, into locals: a failure leaves the loop as it was
    vh::Stream cs, cs2;
    vh::DevicePtr<float> depth[kStagingSlots], color[kStagingSlots], unfilteredDepth, unfilteredColor;
    vh::Event ready[kStagingSlots], ready2[kStagingSlots];
    vh::DevicePtr<unsigned short> rawDepth[kStagingSlots];
    vh::DevicePtr<unsigned char> colorRaw[kStagingSlots];
    if (!m_copyStream) cs = vh::makeStream("hipStreamCreate");
    if (!m_copyStream2) cs2 = vh::makeStream("hipStreamCreate");
    for (int i = 0; i < kStagingSlots; i++) {
        if (!d_stageDepth[i]) depth[i] = vh::deviceAlloc<float>(n, "staging depth");
        if (!d_stageColor[i]) color[i] = vh::deviceAlloc<float>(4 * n, "staging colour");
        if (!m_slotReady[i]) ready[i] = vh::makeEvent(false);
        if (!m_slotReady2[i]) ready2[i] = vh::makeEvent(false);
        if (m_opt.s_framesOnHost) { // the sensor's images, as they come over the link
            rawDepth[i] = vh::deviceAlloc<unsigned short>(nDepth, "staging depth (raw)");
            colorRaw[i] = vh::deviceAlloc<unsigned char>(colorBytes, "staging colour (raw)");
        }
    }
    // what the filters read (vh_sensor.cpp: d_depthMapResampledFloat, d_colorMapResampledFloat4)
    if (f.s_depthFilter) unfilteredDepth = vh::deviceAlloc<float>(n, "unfiltered depth");
    if (f.s_colorFilter && f.colorChannels) unfilteredColor = vh::deviceAlloc<float>(4 * n, "unfiltered colour");
    if (cs) m_copyStream = std::move(cs);
    if (cs2) m_copyStream2 = std::move(cs2);
    for (int i = 0; i < kStagingSlots; i++) {
        if (depth[i]) d_stageDepth[i] = std::move(depth[i]);
        if (color[i]) d_stageColor[i] = std::move(color[i]);
        if (ready[i]) m_slotReady[i] = std::move(ready[i]);
        if (ready2[i]) m_slotReady2[i] = std::move(ready2[i]);
        if (m_opt.s_framesOnHost) {
            d_rawDepth[i] = std::move(rawDepth[i]);
            d_stageColorRaw[i] = std::move(colorRaw[i]); // (in place of the constructor's, which is sized for RGBX at adapter size)
        }
    }
    d_unfilteredDepth = std::move(unfilteredDepth);
    d_unfilteredColor = std::move(unfilteredColor);
    m_stats.uploadBytes = sizeof(uint16_t) * nDepth + colorBytes;
    m_rawFormat = f;
    m_raw = true;
}

// The tracker's buffers (CUDACameraTrackingMultiRes' constructor, vh_tracking.cpp): the input's levels once per staging
// slot, because they are made on the copy stream while the main stream still aligns the frame before.
void Reconstruction::checkCanTrack(const char* who) const
{
    if (m_tracking) throw vh::Error(VH_ERR_BAD_ARGUMENT, std::string(who) + ": tracking is already set");
    if (m_stats.frames || m_stats.invalidFrames || m_uploads || m_frameNumber) throw vh::Error(VH_ERR_BAD_ARGUMENT, std::string(who) + ": frames have been processed already");
    if (!m_rayCast || !m_opt.s_renderEnabled) throw vh::Error(VH_ERR_BAD_ARGUMENT, std::string(who) + ": tracking aligns to the ray cast (needs a ray caster and s_renderEnabled)");
}

void Reconstruction::setTracking(const VhTrackingState& ts)
{
    checkCanTrack("Reconstruction::setTracking");
    // into locals first: a failure leaves the loop without tracking and without half a set of buffers
    std::unique_ptr<vh::IcpSolver> icp(new vh::IcpSolver(m_cp.m_imageWidth, m_cp.m_imageHeight, ts.s_maxLevels, "Reconstruction::setTracking"));
    std::vector<vh::DevicePtr<float>> input[kStagingSlots], inputNormal[kStagingSlots];
    for (unsigned int i = 0; i < ts.s_maxLevels; i++) {
        const size_t n = 4 * (size_t)icp->width[i] * icp->height[i];
        for (int slot = 0; slot < (int)kStagingSlots; slot++) { // (frames read in place use the first set only)
            input[slot].push_back(vh::deviceAlloc<float>(n, "tracking input"));
            inputNormal[slot].push_back(vh::deviceAlloc<float>(n, "tracking input normals"));
        }
    }
    vh::Mapped<VhIcpResult> result(1, "tracking result");
    std::memset(result.host(), 0, sizeof(VhIcpResult));
    // the estimate every solve starts from (:816-826 pass the identity), once
    hipStream_t ms = (hipStream_t)m_sceneRep->getStream();
    const vh::mat4f I = vh::mat4f::identity();
    checkHip(hipMemcpyAsync(icp->estimate.get(), I.m, sizeof(I.m), hipMemcpyHostToDevice, ms), "deltaEstimate");
    checkHip(hipMemsetAsync(icp->ticket.get(), 0, sizeof(uint32_t), ms), "tracking ticket");
    checkHip(hipStreamSynchronize(ms), "Reconstruction::setTracking");
    m_icp = std::move(icp);
    for (int slot = 0; slot < (int)kStagingSlots; slot++) {
        d_trkInput[slot] = std::move(input[slot]);
        d_trkInputNormal[slot] = std::move(inputNormal[slot]);
    }
    m_trkResult = std::move(result);
    m_trackingState = ts;
    m_tracking = true;
}

// The same for CUDACameraTrackingMultiResRGBD: the input's intensity levels per staging slot as well.
void Reconstruction::setTrackingRGBD(const VhTrackingStateRGBD& ts)
{
    checkCanTrack("Reconstruction::setTrackingRGBD");
    if (m_raw && !m_rawFormat.colorChannels) throw vh::Error(VH_ERR_BAD_ARGUMENT, "Reconstruction::setTrackingRGBD: the RGB-D tracker needs a colour image (the raw format has none)");
    // into locals first: a failure leaves the loop without tracking and without half a set of buffers
    std::unique_ptr<vh::IcpSolverRGBD> icp(new vh::IcpSolverRGBD(m_cp.m_imageWidth, m_cp.m_imageHeight, ts.base.s_maxLevels, "Reconstruction::setTrackingRGBD"));
    std::vector<vh::DevicePtr<float>> input[kStagingSlots], inputNormal[kStagingSlots], intensity[kStagingSlots], filtered[kStagingSlots];
    for (unsigned int i = 0; i < ts.base.s_maxLevels; i++) {
        const size_t n = (size_t)icp->width[i] * icp->height[i];
        for (int slot = 0; slot < (int)kStagingSlots; slot++) { // (frames read in place use the first set only)
            input[slot].push_back(vh::deviceAlloc<float>(4 * n, "tracking input"));
            inputNormal[slot].push_back(vh::deviceAlloc<float>(4 * n, "tracking input normals"));
            intensity[slot].push_back(vh::deviceAlloc<float>(n, "tracking input intensity"));
            filtered[slot].push_back(i ? vh::deviceAlloc<float>(n, "tracking input intensity (filtered)") : nullptr);
        }
    }
    vh::Mapped<VhIcpResult> result(1, "tracking result");
    std::memset(result.host(), 0, sizeof(VhIcpResult));
    // the estimate every solve starts from (:816-826 pass the identity), once
    hipStream_t ms = (hipStream_t)m_sceneRep->getStream();
    const vh::mat4f I = vh::mat4f::identity();
    checkHip(hipMemcpyAsync(icp->estimate.get(), I.m, sizeof(I.m), hipMemcpyHostToDevice, ms), "deltaEstimate");
    checkHip(hipMemsetAsync(icp->ticket.get(), 0, sizeof(uint32_t), ms), "tracking ticket");
    checkHip(hipStreamSynchronize(ms), "Reconstruction::setTrackingRGBD");
    m_icpRGBD = std::move(icp);
    for (int slot = 0; slot < (int)kStagingSlots; slot++) {
        d_trkInput[slot] = std::move(input[slot]);
        d_trkInputNormal[slot] = std::move(inputNormal[slot]);
        d_trkIntensity[slot] = std::move(intensity[slot]);
        d_trkIntensityFiltered[slot] = std::move(filtered[slot]);
    }
    m_trkResult = std::move(result);
    m_trackingStateRGBD = ts;
    m_tracking = true;
}

void Reconstruction::synchronize()
{
    if (m_copyStream) checkHip(hipStreamSynchronize((hipStream_t)m_copyStream.get()), "hipStreamSynchronize");
    if (m_copyStream2) checkHip(hipStreamSynchronize((hipStream_t)m_copyStream2.get()), "hipStreamSynchronize");
    // the scene's side stream joins the main stream in integrateFinish(): the main stream is the last to finish
    checkHip(hipStreamSynchronize((hipStream_t)m_sceneRep->getStream()), "hipStreamSynchronize");
    if (m_chunkGrid) m_chunkGrid->pipelineDrain(false); // (the grid's worker has taken in what the last frame moved out; its choice for the next frame stands)
}

void Reconstruction::reset()
{
    synchronize();
    (void)getStats(); // returns the pending timer events to the pool
    const uint64_t bytes = m_stats.uploadBytes;
    std::memset(&m_stats, 0, sizeof(m_stats));
    m_stats.uploadBytes = bytes;
    m_frameNumber = 0;
    m_probePending = false;
    for (int i = 0; i < kStagingSlots; i++) m_slotSceneFrame[i] = 0;
    m_poses.clear();
    m_trackedFrames = m_lostFrames = 0;
}

const ReconstructionStats& Reconstruction::getStats()
{
    if (!m_uploadTimers.empty()) {
        checkHip(hipStreamSynchronize((hipStream_t)m_copyStream.get()), "hipStreamSynchronize");
        for (auto& p : m_uploadTimers) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, (hipEvent_t)p.first.get(), (hipEvent_t)p.second.get()) == hipSuccess) { m_stats.uploadMs += ms; m_stats.uploadsTimed++; }
            m_timerPool.push_back(std::move(p.first));
            m_timerPool.push_back(std::move(p.second));
        }
        m_uploadTimers.clear();
    }
    // the scene's status words: an empty voxel pool or a failed stream-in insert is raised on the device; this is where a
    // caller of the loop gets to see it (a blocking 64-byte read-back: get_stats() is not for the inside of a timed region)
    if (m_chunkGrid) { // what the streaming pipeline moved (its worker counts the blocks that left when they arrive)
        unsigned long long out = 0, in = 0;
        m_chunkGrid->pipelineTotals(&out, &in);
        m_stats.blocksStreamedOut += out - m_pipelineOutSeen;
        m_stats.blocksStreamedIn += in - m_pipelineInSeen;
        m_pipelineOutSeen = out;
        m_pipelineInSeen = in;
    }
    uint32_t state[VH_STATE_WORDS];
    m_sceneRep->getState(state);
    m_stats.heapUnderflows = state[VH_STATE_HEAP_UNDERFLOW];
    m_stats.failedInserts = state[VH_STATE_INSERT_FAILED];
    return m_stats;
}

// CUDARGBDAdapter::process :107-131 for a frame at adapter resolution: upload, colour bytes -> float4.  The copy
// stream runs beside the frame loop's stream; the only thing the main stream does for an upload is to wait for its
// "ready" event (a record on the main stream would idle it for ~6 us per frame).  A staging slot is reused once the
// frame that read it last has been integrated, which the host sees in the scene's mapped frame counter: the pass over
// the voxels of the NEXT frame has started.
DepthCameraData Reconstruction::upload(const SequenceFrame& f)
{
    const unsigned int slot = m_uploads % kStagingSlots;
    const size_t n = (size_t)m_cp.m_imageWidth * m_cp.m_imageHeight;
    hipStream_t cs = (hipStream_t)m_copyStream.get(), ms = (hipStream_t)m_sceneRep->getStream();
    // With tracking the host has seen the ICP result of the frame before this one, so that frame's ray cast has run, and
    // that is behind the integrate of the frame before it: every frame two or more back is done with its slot, and the
    // slot's last frame is four back.  (A lost frame uploads without integrating: the scene's counter does not count it.)
    if (m_slotSceneFrame[slot] != 0 && !m_tracking) {
        // the slot's last frame was the scene's frame number m_slotSceneFrame[slot]: done once a later frame's pass has started
        const unsigned int need = m_slotSceneFrame[slot] + 1u;
        const VhSceneOptions& so = m_sceneRep->getOptions();
        const bool mirrored = m_opt.s_integrationEnabled && !so.s_useReferenceLaunchSequence; // only the fused pass keeps the counter
        auto started = [&] { return m_sceneRep->getNumFramesStartedOnDevice() >= need; };
        if (!mirrored || m_sceneRep->getNumIntegratedFrames() < need) { // nothing later has been enqueued: only a synchronisation tells
            if (!started()) checkHip(hipStreamSynchronize(ms), "hipStreamSynchronize");
        } else {
            const vh::Waited w = vh::spinUntil(started, vh::kDeviceSilentSeconds, true);
            if (!w.ok) throw vh::Error(VH_ERR_TIMEOUT, "Reconstruction: the device made no progress for 30 s");
            m_stats.hostWaitSeconds += w.seconds;
        }
    }
    auto timerEvent = [&]() {
        if (m_timerPool.empty()) return vh::makeEvent(true);
        vh::Event e = std::move(m_timerPool.back());
        m_timerPool.pop_back();
        return e;
    };
    const bool timed = (m_uploads % 8u) == 0u; // (a timed pair idles the copy stream twice)
    vh::Event t0, t1;
    // The frame travels by the copy engines (hipMemcpyAsync: depth on one stream, colour on another, so that each gets
    // an engine), then the colour is converted as in the sensor path.  A kernel that read the pinned frame itself (one
    // pass, no raw-colour staging) was measured slower for the loop as a whole: while uncached reads of host memory are
    // in flight every other kernel's memory accesses queue behind them, and k_render took two to three times as long.
    if (timed) {
        t0 = timerEvent();
        t1 = timerEvent();
        checkHip(hipEventRecord((hipEvent_t)t0.get(), cs), "hipEventRecord");
    }
    const bool hasColor = m_rawRun ? (m_rawFormat.colorChannels != 0u && f.color != nullptr) : f.color != nullptr;
    if (m_rawRun) {
        // SensorDataReader::processDepth's conversion + CUDARGBDAdapter::process + the filters of CUDARGBDSensor::process
        // (vh_sensor.cpp:154-164), all on the copy stream: the main stream only waits for the slot's "ready" event
        const RawFrameFormat& rf = m_rawFormat;
        const unsigned int W = m_cp.m_imageWidth, H = m_cp.m_imageHeight;
        const uint16_t* depthRaw = reinterpret_cast<const uint16_t*>(f.depth);
        const uint8_t* colorRaw = hasColor ? static_cast<const uint8_t*>(f.color) : nullptr;
        if (m_opt.s_framesOnHost) { // two copies, two streams, as below
            hipStream_t cs2 = (hipStream_t)m_copyStream2.get();
            checkHip(hipMemcpyAsync(d_rawDepth[slot].get(), depthRaw, sizeof(uint16_t) * (size_t)rf.depthWidth * rf.depthHeight, hipMemcpyHostToDevice, cs2), "upload depth");
            checkHip(hipEventRecord((hipEvent_t)m_slotReady2[slot].get(), cs2), "hipEventRecord");
            if (colorRaw) checkHip(hipMemcpyAsync(d_stageColorRaw[slot].get(), colorRaw, (size_t)rf.colorChannels * rf.colorWidth * rf.colorHeight, hipMemcpyHostToDevice, cs), "upload colour");
            checkHip(hipStreamWaitEvent(cs, (hipEvent_t)m_slotReady2[slot].get(), 0), "hipStreamWaitEvent");
            depthRaw = d_rawDepth[slot].get();
            if (colorRaw) colorRaw = d_stageColorRaw[slot].get();
        }
        const bool filterColor = colorRaw && rf.s_colorFilter;
        float* depthOut = rf.s_depthFilter ? d_unfilteredDepth.get() : d_stageDepth[slot].get();
        float* colorOut = filterColor ? d_unfilteredColor.get() : d_stageColor[slot].get();
        check(vh_ingest_frame(depthOut, colorRaw ? colorOut : nullptr, W, H, depthRaw, rf.depthWidth, rf.depthHeight, colorRaw, rf.colorWidth, rf.colorHeight,
                              colorRaw ? rf.colorChannels : 0u, rf.depthShift, m_copyStream.get()), "vh_ingest_frame");
        if (filterColor) check(vh_gauss_filter_float4_map(d_stageColor[slot].get(), d_unfilteredColor.get(), rf.s_colorSigmaD, rf.s_colorSigmaR, W, H, m_copyStream.get()), "gaussFilterFloat4Map");
        if (rf.s_depthFilter) check(vh_gauss_filter_float_map(d_stageDepth[slot].get(), d_unfilteredDepth.get(), rf.s_depthSigmaD, rf.s_depthSigmaR, W, H, m_copyStream.get()), "gaussFilterFloatMap");
    } else {
        // two copies, two streams: each gets a copy engine of its own
        hipStream_t cs2 = (hipStream_t)m_copyStream2.get();
        checkHip(hipMemcpyAsync(d_stageDepth[slot].get(), f.depth, sizeof(float) * n, hipMemcpyHostToDevice, cs2), "upload depth");
        checkHip(hipEventRecord((hipEvent_t)m_slotReady2[slot].get(), cs2), "hipEventRecord");
        checkHip(hipStreamWaitEvent(ms, (hipEvent_t)m_slotReady2[slot].get(), 0), "hipStreamWaitEvent");
        if (f.color) {
            checkHip(hipMemcpyAsync(d_stageColorRaw[slot].get(), f.color, 4 * n, hipMemcpyHostToDevice, cs), "upload colour");
            check(vh_convert_color_raw_to_float4(d_stageColor[slot].get(), d_stageColorRaw[slot].get(), m_cp.m_imageWidth, m_cp.m_imageHeight, m_copyStream.get()), "convertColorRawToFloat4");
        }
    }
    if (timed) {
        // the pair spans the whole upload: the depth copy runs on the other stream, so this one waits for it first
        // (t0 was recorded before either copy was enqueued; both streams were idle or busy with earlier uploads)
        if (!m_rawRun) checkHip(hipStreamWaitEvent(cs, (hipEvent_t)m_slotReady2[slot].get(), 0), "hipStreamWaitEvent");
        checkHip(hipEventRecord((hipEvent_t)t1.get(), cs), "hipEventRecord");
        m_uploadTimers.emplace_back(std::move(t0), std::move(t1));
    }
    if (m_tracking) { // what the tracker needs of the input depends on the frame alone: here, beside the previous frame's work
        if (!m_rawRun) checkHip(hipStreamWaitEvent(cs, (hipEvent_t)m_slotReady2[slot].get(), 0), "hipStreamWaitEvent");
        inputPyramid(slot, d_stageDepth[slot].get(), hasColor ? d_stageColor[slot].get() : nullptr, m_copyStream.get()); // (the colour was made on this stream)
    }
    checkHip(hipEventRecord((hipEvent_t)m_slotReady[slot].get(), cs), "hipEventRecord");
    checkHip(hipStreamWaitEvent(ms, (hipEvent_t)m_slotReady[slot].get(), 0), "hipStreamWaitEvent");
    m_slotSceneFrame[slot] = m_sceneRep->getNumIntegratedFrames() + 1u; // the scene frame this upload feeds
    m_uploads++;
    DepthCameraData cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.d_depthData = d_stageDepth[slot].get();
    cam.d_colorData = hasColor ? d_stageColor[slot].get() : nullptr;
    return cam;
}

namespace {
bool poseValid(const float* m) { return !(m[0] == -std::numeric_limits<float>::infinity() || std::isnan(m[0])); }
}

void Reconstruction::frame(const SequenceFrame& f, const SequenceFrame* next)
{
    // :733-747
    vh::mat4f transformation;
    std::memcpy(transformation.m, f.rigidTransform, sizeof(transformation.m));
    if (!poseValid(transformation.m)) {
        m_stats.invalidFrames++;
        m_poses.insert(m_poses.end(), 16, -std::numeric_limits<float>::infinity());
        return; // "INVALID FRAME"
    }
    if (!f.depth) throw vh::Error(VH_ERR_BAD_ARGUMENT, "Reconstruction: frame without a depth map");

    DepthCameraData cam;
    if (m_opt.s_framesOnHost || m_rawRun) cam = upload(f);
    else {
        std::memset(&cam, 0, sizeof(cam));
        cam.d_depthData = const_cast<float*>(f.depth);
        cam.d_colorData = const_cast<float*>(static_cast<const float*>(f.color));
    }

    const bool streaming = m_opt.s_streamingEnabled && m_chunkGrid;
    const bool threaded = streaming && !m_opt.s_offlineProcessing && !m_chunkGrid->getTerminatedThread();
    const vh::vec3f p = transformation.transformPoint({ m_opt.s_streamingPos[0], m_opt.s_streamingPos[1], m_opt.s_streamingPos[2] });

    // The streaming step of this frame (:881-900).  The reference runs it between the ray cast of the previous pose and this
    // frame's alloc as a chain of host <-> device round trips (two counters read back, the blocks that left put into the host
    // grid before the bit mask for alloc is known, the chunk that comes in chosen after that), so alloc could not ride in the
    // ray caster's launch and the host could not enqueue past it.  With the next pose known a frame ahead (the sequence
    // comes from a file) the step runs without a host wait (CUDASceneRepChunkGrid's pipeline, vh.hpp):
    //   * how many blocks leave at most was asked of the device a frame early (a count-only run of the stream-out scan for
    //     THIS frame's sphere and part, behind the previous frame's alloc: nothing adds blocks between there and here);
    //   * the chunk that comes in was chosen and uploaded by the grid's worker while the device worked on the previous frame;
    //   * the counts stay on the device, the device keeps its own copy of the bit mask.
    // A frame in which nothing leaves and nothing comes in is then two or three launches, like a frame without streaming (alloc
    // rides in the ray caster's launch, reading the device's bit mask); a frame with traffic is the reference's order of
    // launches, enqueued without waiting.  Without the answers (first frame, next pose unknown, a pass too large for the
    // pipeline's staging) the frame takes the reference's order of calls.
    enum Step { kFull, kPipelined } step = kFull;
    unsigned int mostOut = 0;
    CUDASceneRepChunkGrid::StreamDecision choice = { 0u, 0xffffffffu, 0 };
    struct Unwind { // (integrateAhead() ... integrateFinish() with the ray cast in between: a throw must not leave the scene refusing every integrate())
        CUDASceneRepHashSDF* scene;
        bool ahead = false;
        ~Unwind() { if (ahead) scene->abortAhead(); }
    } unwind{ m_sceneRep };
    const bool pipelined = threaded && m_opt.s_allocAhead && m_opt.s_integrationEnabled;
    if (pipelined && m_probePending && std::memcmp(m_probePose, f.rigidTransform, sizeof(m_probePose)) == 0 &&
        m_chunkGrid->pipelineHasDecision(p, m_opt.s_streamingRadius)) {
        const double t0 = now();
        mostOut = m_chunkGrid->probeResult();
        if (mostOut <= m_chunkGrid->pipelineCapacity()) {
            choice = m_chunkGrid->pipelineDecision();
            step = kPipelined;
        }
        m_stats.hostWaitSeconds += now() - t0;
    }
    m_probePending = false;
    const bool quiet = step == kPipelined && mostOut == 0u && choice.nIn == 0u;

    const bool ahead = m_opt.s_allocAhead && m_opt.s_integrationEnabled && (!streaming || quiet);
    const unsigned int* d_bitMask = nullptr;
    if (streaming && step == kPipelined) d_bitMask = m_chunkGrid->getBitMaskDevice(); // (kept by the passes themselves: no upload)
    // :750-751 (the pose the scene holds is the previous frame's)
    const vh::mat4f renderTransform = m_sceneRep->getLastRigidTransform();
    VhFrameJob* job = nullptr;
    if (ahead) {
        job = m_sceneRep->integrateAhead(transformation, cam, m_cp, d_bitMask);
        unwind.ahead = true;
    }
    if (m_frameNumber > 0 && m_opt.s_renderEnabled) { // :750 "getFrameNumber() > 1" with frames counted from 1
        if (m_debugFailRender && --m_debugFailRender == 0) {
            // (the choice for this frame has been taken off the worker: hand it back before leaving)
            if (step == kPipelined) m_chunkGrid->pipelineReturn(choice, p, m_opt.s_streamingRadius);
            throw vh::Error(VH_ERR_BAD_ARGUMENT, "Reconstruction: injected failure of the ray cast (vh_reconstruction_debug_fail_render)");
        }
        const unsigned int used0 = m_rayCast->getNumSplatsMadeAheadUsed();
        try {
            m_rayCast->render(m_sceneRep->getHashData(), m_sceneRep->getHashParams(), m_cp, renderTransform, job); // :763
        } catch (...) {
            if (step == kPipelined) m_chunkGrid->pipelineReturn(choice, p, m_opt.s_streamingRadius);
            throw;
        }
        m_stats.splatsMadeAheadUsed += m_rayCast->getNumSplatsMadeAheadUsed() - used0;
        if (job && job->allocLaunched && job->compactifyLaunched) m_stats.framesWithRiders++;
        if (job && job->fusedLaunched) m_stats.framesInTwoLaunches++;
    }

    if (streaming && step == kPipelined) {
        try {
            (void)m_chunkGrid->pipelineStreamOut(p, m_opt.s_streamingRadius, CUDASceneRepChunkGrid::s_useParts, mostOut);
            m_chunkGrid->pipelineStreamIn(choice);
        } catch (...) { // (the chunk that was to come in is still in the worker's staging buffer: it goes back into the grid with the next drain)
            m_chunkGrid->pipelineReturn(choice, p, m_opt.s_streamingRadius);
            throw;
        }
        m_stats.streamingFramesPipelined++;
        if (quiet) m_stats.streamingStepsSkipped++;
    } else if (streaming) { // :881-900
        d_bitMask = streamAround(p);
    }

    // the question for the next frame, behind this frame's alloc
    const bool ask = pipelined && next && next->depth && poseValid(next->rigidTransform);
    vh::vec3f np = { 0.0f, 0.0f, 0.0f };
    if (ask) {
        vh::mat4f nt;
        std::memcpy(nt.m, next->rigidTransform, sizeof(nt.m));
        np = nt.transformPoint({ m_opt.s_streamingPos[0], m_opt.s_streamingPos[1], m_opt.s_streamingPos[2] });
    }
    auto askNow = [&]() {
        m_chunkGrid->probeStreamOut(np, m_opt.s_streamingRadius, CUDASceneRepChunkGrid::s_useParts);
        std::memcpy(m_probePose, next->rigidTransform, sizeof(m_probePose));
        m_probePending = true;
    };
    const bool allocIsIn = ahead && job && job->allocLaunched; // (it rode in the ray caster's launch)
    if (ask && allocIsIn) askNow();

    if (m_opt.s_integrationEnabled) { // :903
        unwind.ahead = false; // (integrateFinish() closes the job first thing)
        if (ahead) m_sceneRep->integrateFinish(cam, m_cp);
        else m_sceneRep->integrate(transformation, cam, m_cp, d_bitMask);
    } else {
        m_sceneRep->setLastRigidTransformAndCompactify(transformation, m_cp); // :907
    }
    if (ask && !allocIsIn) askNow();
    // the worker's job: take in what this frame's stream-out pass moves, choose and upload what comes in at the next frame
    if (pipelined && (ask || step == kPipelined)) m_chunkGrid->pipelineAsk(ask, np, m_opt.s_streamingRadius);
    m_frameNumber++;
    m_stats.frames++;
    m_poses.insert(m_poses.end(), transformation.m, transformation.m + 16);
}

// :881-900, the reference's order of calls: the host reads the streaming counters back
const unsigned int* Reconstruction::streamAround(const vh::vec3f& p)
{
    const bool threaded = !m_opt.s_offlineProcessing && !m_chunkGrid->getTerminatedThread();
    const double t0 = now();
    unsigned int nStreamedBlocks = 0;
    if (m_opt.s_offlineProcessing) {
        for (unsigned int i = 0; i < m_sceneRep->getOptions().s_streamingOutParts; i++) {
            m_chunkGrid->streamOutToCPU(p, m_opt.s_streamingRadius, CUDASceneRepChunkGrid::s_useParts, nStreamedBlocks);
            m_stats.blocksStreamedOut += nStreamedBlocks;
        }
        m_chunkGrid->streamInToGPUAll(p, m_opt.s_streamingRadius, CUDASceneRepChunkGrid::s_useParts, nStreamedBlocks);
        m_stats.blocksStreamedIn += nStreamedBlocks;
    } else if (threaded) {
        m_chunkGrid->streamOutToCPUPass0GPU(p, m_opt.s_streamingRadius, CUDASceneRepChunkGrid::s_useParts, true);
        m_stats.blocksStreamedOut += m_chunkGrid->getNumStreamedOutBlocks();
        m_chunkGrid->streamInToGPUPass1GPU(true);
        m_stats.blocksStreamedIn += m_chunkGrid->getNumStreamedInBlocks();
    } else {
        m_chunkGrid->streamOutToCPU(p, m_opt.s_streamingRadius, CUDASceneRepChunkGrid::s_useParts, nStreamedBlocks);
        m_stats.blocksStreamedOut += nStreamedBlocks;
        m_chunkGrid->streamInToGPU(p, m_opt.s_streamingRadius, CUDASceneRepChunkGrid::s_useParts, nStreamedBlocks);
        m_stats.blocksStreamedIn += nStreamedBlocks;
    }
    m_stats.hostWaitSeconds += now() - t0; // read-backs of the streaming counters: the host waits for the device here
    return m_chunkGrid->getBitMaskGPU();
}

// CUDARGBDSensor::process :173-174 (camera-space positions, normals) and the input half of applyCT's pyramids for one
// frame, on `stream`: DSC/CUDACameraTrackingMultiRes.cpp:256-263, or with the RGB-D tracker
// DSC/CUDACameraTrackingMultiResRGBD.cpp:264-284, which reads the frame's float4 colour map as well
void Reconstruction::inputPyramid(unsigned int slot, const float* d_depth, const float* d_color, vhStream_t stream)
{
    const vh::IcpPyramid in = vh::icpPyramid(d_trkInput[slot][0].get(), d_trkInputNormal[slot][0].get(), d_trkInput[slot], d_trkInputNormal[slot]);
    const unsigned int W = m_cp.m_imageWidth, H = m_cp.m_imageHeight;
    check(vh_convert_depth_float_to_camera_space_float4(in.map[0], d_depth, &m_cp, W, H, stream), "convertDepthFloatToCameraSpaceFloat4");
    check(vh_compute_normals(in.normal[0], in.map[0], W, H, stream), "computeNormals");
    if (m_icpRGBD) {
        m_icpRGBD->inputPyramid(in, d_color, vh::icpIntensityPyramid(d_trkIntensity[slot], d_trkIntensityFiltered[slot]), stream);
        return;
    }
    for (unsigned int i = 0; i + 1 < m_icp->width.size(); i++) m_icp->coarserLevel(in, i, stream);
}

// One frame with tracking: reconstruction() :750-879 with s_binaryDumpSensorUseTrajectory = false.  Everything is
// enqueued on the loop's stream without a blocking call; the host then waits once, for the tag the solve's last step
// stores into mapped host memory behind the result, because the pose decides what streaming and integrate are asked.
void Reconstruction::frameTracked(const SequenceFrame& f)
{
    if (!f.depth) throw vh::Error(VH_ERR_BAD_ARGUMENT, "Reconstruction: frame without a depth map");
    if (m_icpRGBD && !f.color) throw vh::Error(VH_ERR_BAD_ARGUMENT, "Reconstruction: the RGB-D tracker needs a colour map with every frame");
    vhStream_t stream = m_sceneRep->getStream();
    DepthCameraData cam;
    unsigned int slot = 0;
    if (m_opt.s_framesOnHost || m_rawRun) {
        cam = upload(f);
        slot = (m_uploads - 1u) % kStagingSlots;
    } else {
        std::memset(&cam, 0, sizeof(cam));
        cam.d_depthData = const_cast<float*>(f.depth);
        cam.d_colorData = const_cast<float*>(static_cast<const float*>(f.color));
        inputPyramid(0, cam.d_depthData, cam.d_colorData, stream);
    }
    const float minf = -std::numeric_limits<float>::infinity();
    vh::mat4f transformation = vh::mat4f::identity();
    if (m_frameNumber > 0) { // :750 "getFrameNumber() > 1" with frames counted from 1
        const vh::mat4f lastTransform = m_sceneRep->getLastRigidTransform();
        m_rayCast->render(m_sceneRep->getHashData(), m_sceneRep->getHashParams(), m_cp, lastTransform, nullptr); // :763
        const RayCastData& rd = m_rayCast->getRayCastData();
        const vh::IcpPyramid in = vh::icpPyramid(d_trkInput[slot][0].get(), d_trkInputNormal[slot][0].get(), d_trkInput[slot], d_trkInputNormal[slot]);
        const uint32_t tag = vh::nextTag(m_trkTag);
        // one launch per iteration where a level allows it; the last step stores the result and the tag into mapped memory
        if (m_icpRGBD) {
            const vh::IcpPyramid mdl = vh::icpPyramid(rd.d_depth4, rd.d_normals, m_icpRGBD->model, m_icpRGBD->modelNormal);
            m_icpRGBD->modelPyramid(mdl, rd.d_colors, stream); // the model half of the pyramids, RGBD.cpp:264-284
            m_icpRGBD->align(in, vh::icpIntensityPyramid(d_trkIntensity[slot], d_trkIntensityFiltered[slot]), mdl, m_trackingStateRGBD, m_cp, true,
                             m_trkResult.device(), tag, stream);
        } else {
            const vh::IcpPyramid mdl = vh::icpPyramid(rd.d_depth4, rd.d_normals, m_icp->model, m_icp->modelNormal);
            for (unsigned int i = 0; i + 1 < m_icp->width.size(); i++) m_icp->coarserLevel(mdl, i, stream); // the model half of the pyramids, :256-263
            m_icp->align(in, mdl, m_trackingState, m_cp, true, m_trkResult.device(), tag, stream);
        }
        // the one wait of the frame
        const vh::Waited w = vh::waitArrived(&m_trkResult.host()->tag, tag, vh::kDeviceSilentSeconds, true);
        if (!w.ok) throw vh::Error(VH_ERR_TIMEOUT, "Reconstruction: no tracking result from the device for 30 s");
        m_stats.hostWaitSeconds += w.seconds;
        if (m_trkResult.host()->lost) { // "!!! TRACKING LOST !!!": the frame is not integrated, the scene keeps its pose
            m_lostFrames++;
            m_frameNumber++;
            m_poses.insert(m_poses.end(), 16, minf);
            return;
        }
        vh::mat4f delta;
        std::memcpy(delta.m, m_trkResult.host()->delta, sizeof(delta.m));
        transformation = lastTransform * delta;
        m_trackedFrames++;
    }
    const unsigned int* d_bitMask = nullptr;
    if (m_opt.s_streamingEnabled && m_chunkGrid)
        d_bitMask = streamAround(transformation.transformPoint({ m_opt.s_streamingPos[0], m_opt.s_streamingPos[1], m_opt.s_streamingPos[2] }));
    // the pose is not known before the ray cast: alloc cannot ride in its launch, whatever s_allocAhead says
    if (m_opt.s_integrationEnabled) m_sceneRep->integrate(transformation, cam, m_cp, d_bitMask); // :903
    else m_sceneRep->setLastRigidTransformAndCompactify(transformation, m_cp);                   // :907
    m_frameNumber++;
    m_stats.frames++;
    m_poses.insert(m_poses.end(), transformation.m, transformation.m + 16);
}

void Reconstruction::run(const SequenceFrame* frames, unsigned int n, const SequenceFrame* after)
{
    if (n && !frames) throw vh::Error(VH_ERR_BAD_ARGUMENT, "Reconstruction::run: null frames");
    if (m_raw && !m_rawRun) throw vh::Error(VH_ERR_BAD_ARGUMENT, "Reconstruction::run: this loop takes raw frames (runRaw)");
    const double t0 = now();
    double waited = 0.0;
    const double streamWait0 = m_stats.hostWaitSeconds;
    // Run-ahead bound without an event (a record idles the queue for ~6 us on this machine): the pass over the voxels
    // mirrors the scene's frame counter into mapped host memory when it starts.  Only that (fused) pass does so.
    const VhSceneOptions& so = m_sceneRep->getOptions();
    const bool bounded = m_opt.s_maxFramesInFlight && m_opt.s_integrationEnabled && !so.s_useReferenceLaunchSequence;
    auto room = [&] { return m_sceneRep->getNumIntegratedFrames() - m_sceneRep->getNumFramesStartedOnDevice() < m_opt.s_maxFramesInFlight; };
    for (unsigned int i = 0; i < n; i++) {
        if (bounded) {
            const vh::Waited w = vh::spinUntil(room, vh::kDeviceSilentSeconds, true);
            if (!w.ok) throw vh::Error(VH_ERR_TIMEOUT, "Reconstruction::run: the device made no progress for 30 s");
            waited += w.seconds;
        }
        if (m_tracking) frameTracked(frames[i]); // (the pose of the next frame is not known ahead: nothing to look at)
        else frame(frames[i], i + 1 < n ? &frames[i + 1] : after);
    }
    const double total = now() - t0, streamWait = m_stats.hostWaitSeconds - streamWait0;
    m_stats.hostWaitSeconds += waited;
    m_stats.hostEnqueueSeconds += total - waited - streamWait;
}

void Reconstruction::runRaw(const RawSequenceFrame* frames, unsigned int n, const RawSequenceFrame* after)
{
    if (!m_raw) throw vh::Error(VH_ERR_BAD_ARGUMENT, "Reconstruction::runRaw: no raw format has been set (setRawFormat)");
    if (n && !frames) throw vh::Error(VH_ERR_BAD_ARGUMENT, "Reconstruction::runRaw: null frames");
    // frame() reads poses and pointers; upload() knows what the pointers are
    m_rawFrames.resize((size_t)n + 1);
    auto put = [](SequenceFrame& s, const RawSequenceFrame& r) {
        std::memcpy(s.rigidTransform, r.rigidTransform, sizeof(s.rigidTransform));
        s.depth = reinterpret_cast<const float*>(r.depth);
        s.color = r.color;
    };
    for (unsigned int i = 0; i < n; i++) put(m_rawFrames[i], frames[i]);
    if (after) put(m_rawFrames[n], *after);
    struct Mode {
        bool& on;
        ~Mode() { on = false; }
    } mode{ m_rawRun };
    m_rawRun = true;
    run(m_rawFrames.data(), n, after ? &m_rawFrames[n] : nullptr);
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

namespace {
template <class F> int guarded(F&& f) { return vh_guarded(static_cast<F&&>(f)); }
} // namespace

extern "C" {

void vh_reconstruction_default_options(VhReconstructionOptions* out)
{
    if (out) *out = Reconstruction::defaultOptions();
}

int vh_reconstruction_create(VhSceneRep* scene, VhRayCast* rayCast, VhChunkGrid* chunkGrid, const VhDepthCameraParams* cp,
                             const VhReconstructionOptions* opt, VhReconstruction** out)
{
    if (!scene || !cp || !out) return VH_ERR_BAD_ARGUMENT;
    *out = nullptr;
    return guarded([&] {
        const ReconstructionOptions o = opt ? *opt : Reconstruction::defaultOptions();
        *out = new VhReconstruction(&scene->impl, rayCast ? &rayCast->impl : nullptr, chunkGrid ? &chunkGrid->impl : nullptr, *cp, o);
    });
}
void vh_reconstruction_destroy(VhReconstruction* r) { delete r; }
int vh_reconstruction_run(VhReconstruction* r, const VhSequenceFrame* frames, uint32_t n)
{
    if (!r || (n && !frames)) return VH_ERR_BAD_ARGUMENT;
    return guarded([&] { r->impl.run(frames, n); });
}
int vh_reconstruction_run_ahead(VhReconstruction* r, const VhSequenceFrame* frames, uint32_t n, const VhSequenceFrame* next)
{
    if (!r || (n && !frames)) return VH_ERR_BAD_ARGUMENT;
    return guarded([&] { r->impl.run(frames, n, next); });
}
int vh_reconstruction_set_raw_format(VhReconstruction* r, const VhRawFrameFormat* format)
{
    if (!r || !format) return VH_ERR_BAD_ARGUMENT;
    return guarded([&] { r->impl.setRawFormat(*format); });
}
int vh_reconstruction_run_raw(VhReconstruction* r, const VhRawSequenceFrame* frames, uint32_t n)
{
    if (!r || (n && !frames)) return VH_ERR_BAD_ARGUMENT;
    return guarded([&] { r->impl.runRaw(frames, n); });
}
int vh_reconstruction_run_raw_ahead(VhReconstruction* r, const VhRawSequenceFrame* frames, uint32_t n, const VhRawSequenceFrame* next)
{
    if (!r || (n && !frames)) return VH_ERR_BAD_ARGUMENT;
    return guarded([&] { r->impl.runRaw(frames, n, next); });
}
int vh_reconstruction_set_tracking(VhReconstruction* r, const VhTrackingState* settings)
{
    if (!r || !settings) return VH_ERR_BAD_ARGUMENT;
    return guarded([&] { r->impl.setTracking(*settings); });
}
int vh_reconstruction_set_tracking_rgbd(VhReconstruction* r, const VhTrackingStateRGBD* settings)
{
    if (!r || !settings) return VH_ERR_BAD_ARGUMENT;
    return guarded([&] { r->impl.setTrackingRGBD(*settings); });
}
int vh_reconstruction_get_poses(VhReconstruction* r, uint32_t first, uint32_t n, float* out)
{
    if (!r || (n && !out)) return VH_ERR_BAD_ARGUMENT;
    return guarded([&] {
        const std::vector<float>& poses = r->impl.getPoses();
        if ((size_t)first + n > poses.size() / 16) throw vh::Error(VH_ERR_BAD_ARGUMENT, "vh_reconstruction_get_poses: frame range outside the frames fed");
        if (n) std::memcpy(out, poses.data() + 16 * (size_t)first, sizeof(float) * 16 * n);
    });
}
int vh_reconstruction_get_tracking_stats(VhReconstruction* r, uint64_t* trackedFrames, uint64_t* lostFrames)
{
    if (!r || !trackedFrames || !lostFrames) return VH_ERR_BAD_ARGUMENT;
    *trackedFrames = r->impl.getNumTrackedFrames();
    *lostFrames = r->impl.getNumLostFrames();
    return VH_OK;
}
int vh_reconstruction_synchronize(VhReconstruction* r)
{
    if (!r) return VH_ERR_BAD_ARGUMENT;
    return guarded([&] { r->impl.synchronize(); });
}
int vh_reconstruction_debug_fail_render(VhReconstruction* r, uint32_t nthRenderFromNow)
{
    if (!r) return VH_ERR_BAD_ARGUMENT;
    return guarded([&] { r->impl.debugFailRender(nthRenderFromNow); });
}
int vh_reconstruction_get_stats(VhReconstruction* r, VhReconstructionStats* out)
{
    if (!r || !out) return VH_ERR_BAD_ARGUMENT;
    return guarded([&] { *out = r->impl.getStats(); });
}
int vh_reconstruction_reset(VhReconstruction* r)
{
    if (!r) return VH_ERR_BAD_ARGUMENT;
    return guarded([&] { r->impl.reset(); });
}

} // extern "C"
