// vh_tracking.cpp -- CUDACameraTrackingMultiRes (DSC/CUDACameraTrackingMultiRes.{h,cpp}) over the vh_icp_* steps,
// CUDACameraTrackingMultiResRGBD (DSC/CUDACameraTrackingMultiResRGBD.{h,cpp}) over the vh_icp_rgbd_* steps, and the
// reader of zParametersTracking*.txt (GlobalCameraTrackingState).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>
#include <limits>
#include <map>
#include <sstream>

#include "../../include/vh.hpp"
#include "vh_host_util.hpp"
#include "vh_params.hpp"

// ---------------------------------------------------------------------------
// what the two solves share on the host
// ---------------------------------------------------------------------------

namespace {
void checkPyramid(unsigned int imageWidth, unsigned int imageHeight, unsigned int levels, const char* who)
{
    if (levels == 0 || levels > VH_TRACKING_MAX_LEVELS || (imageWidth >> (levels - 1)) < 2 || (imageHeight >> (levels - 1)) < 2)
        throw vh::Error(VH_ERR_BAD_ARGUMENT, std::string(who) + ": bad pyramid");
}
// The finest level that iterates: a coarse-to-fine solve ends with that level's last iteration.  -1: no level iterates.
int lastIteratingLevel(const VhTrackingState& ts, size_t levels)
{
    for (size_t level = 0; level < levels; level++)
        if (ts.s_maxOuterIter[level]) return (int)level;
    return -1;
}
// A fused step that is the solve's last publishes the result itself (d_result for it, null for every other): a publishing
// kernel behind it would be one more dependent launch, and the step's last wave holds the state in its hands anyway ...
VhIcpResult* publishedByStep(const VhTrackingState& ts, size_t levels, int level, unsigned int outer, VhIcpResult* d_result)
{
    return level == lastIteratingLevel(ts, levels) && outer + 1 == ts.s_maxOuterIter[level] ? d_result : nullptr;
}
// ... and a solve whose last iteration was not a fused step, or in which no level iterates, publishes afterwards
void publishAfterwards(const VhIcpState* state, VhIcpResult* d_result, bool published, uint32_t tag, vhStream_t stream)
{
    if (d_result && !published) check(vh_icp_publish(state, d_result, tag, stream), "vh_icp_publish");
}
// what applyCT returns: -inf everywhere when tracking was lost (isTrackingLost), lastTransform * delta otherwise
vh::mat4f trackedPose(const VhIcpState& state, const vh::mat4f& lastTransform)
{
    vh::mat4f delta;
    if (state.lost) {
        for (float& v : delta.m) v = -std::numeric_limits<float>::infinity();
        return delta;
    }
    std::memcpy(delta.m, state.delta, sizeof(delta.m));
    return lastTransform * delta;
}
} // namespace

// ---------------------------------------------------------------------------
// vh::IcpSolver: the plain solve, enqueued here for both its hosts
// ---------------------------------------------------------------------------

vh::IcpPyramid vh::icpPyramid(float* map0, float* normal0, const std::vector<DevicePtr<float>>& maps, const std::vector<DevicePtr<float>>& normals)
{
    IcpPyramid p = {};
    p.map[0] = map0;
    p.normal[0] = normal0;
    for (size_t i = 1; i < maps.size(); i++) { p.map[i] = maps[i].get(); p.normal[i] = normals[i].get(); }
    return p;
}

vh::IcpSolver::IcpSolver(unsigned int imageWidth, unsigned int imageHeight, unsigned int levels, const char* who)
{
    checkPyramid(imageWidth, imageHeight, levels, who);
    unsigned int fac = 1;
    for (unsigned int i = 0; i < levels; i++) { // :39-95
        width.push_back(imageWidth / fac);
        height.push_back(imageHeight / fac);
        const size_t n = 4 * (size_t)width[i] * height[i];
        correspondence.push_back(deviceAlloc<float>(n, "d_correspondence"));
        correspondenceNormal.push_back(deviceAlloc<float>(n, "d_correspondenceNormal"));
        model.push_back(i ? deviceAlloc<float>(n, "d_model") : nullptr); // the finest level is the caller's maps
        modelNormal.push_back(i ? deviceAlloc<float>(n, "d_modelNormal") : nullptr);
        fac *= 2;
    }
    partials = deviceAlloc<float>(30 * (size_t)vh_icp_num_partials(imageWidth, imageHeight), "d_partials");
    state = deviceAlloc<VhIcpState>(1, "VhIcpState");
    estimate = deviceAlloc<float>(16, "deltaEstimate");
    ticket = deviceAlloc<uint32_t>(1, "tracking ticket");
}

void vh::IcpSolver::coarserLevel(const IcpPyramid& p, unsigned int i, vhStream_t stream) const
{
    check(vh_resample_float4_map(p.map[i + 1], width[i + 1], height[i + 1], p.map[i], width[i], height[i], stream), "resampleFloat4Map");
    check(vh_compute_normals(p.normal[i + 1], p.map[i + 1], width[i + 1], height[i + 1], stream), "computeNormals");
}

void vh::IcpSolver::align(const IcpPyramid& in, const IcpPyramid& mdl, const VhTrackingState& ts, const DepthCameraParams& cp, bool fusedStep,
                          VhIcpResult* d_result, uint32_t tag, vhStream_t stream) const
{
    if (fusedStep) checkHip(hipMemsetAsync(ticket.get(), 0, sizeof(uint32_t), (hipStream_t)stream), "tracking ticket");
    check(vh_icp_begin(state.get(), estimate.get(), stream), "vh_icp_begin");
    bool published = false;
    for (int level = (int)width.size() - 1; level >= 0; level--) {
        const unsigned int W = width[level], H = height[level];
        const float levelFactor = std::pow(2.0f, (float)level);
        float *corr = correspondence[level].get(), *corrN = correspondenceNormal[level].get();
        check(vh_icp_begin_level(state.get(), stream), "vh_icp_begin_level");
        for (unsigned int outer = 0; outer < ts.s_maxOuterIter[level]; outer++) {
            const unsigned int inner = ts.s_maxInnerIter[level];
            if (fusedStep && inner == 1u) {
                VhIcpResult* const publish = publishedByStep(ts, width.size(), level, outer, d_result);
                check(vh_icp_step(in.map[level], in.normal[level], mdl.map[level], mdl.normal[level], W, H, ts.s_distThres[level], ts.s_normalThres[level],
                                  levelFactor, &cp, partials.get(), ticket.get(), state.get(), ts.s_angleTransThres[level], ts.s_distTransThres[level],
                                  ts.s_residualEarlyOut[level], publish, tag, stream), "vh_icp_step");
                published = published || publish;
                continue;
            }
            check(vh_icp_projective_correspondences(in.map[level], in.normal[level], mdl.map[level], mdl.normal[level], corr, corrN, W, H, ts.s_distThres[level],
                                                    ts.s_normalThres[level], levelFactor, state.get(), &cp, stream), "projectiveCorrespondences");
            for (unsigned int i = 0; i < inner; i++) {
                check(vh_icp_build_linear_system(W, H, partials.get(), in.map[level], corr, corrN, state.get(), stream), "buildLinearSystem");
                check(vh_icp_solve(state.get(), partials.get(), vh_icp_num_partials(W, H), ts.s_angleTransThres[level], ts.s_distTransThres[level],
                                   ts.s_residualEarlyOut[level], i + 1 == inner, stream), "vh_icp_solve");
            }
        }
    }
    publishAfterwards(state.get(), d_result, published, tag, stream);
}

// ---------------------------------------------------------------------------
// CUDACameraTrackingMultiRes
// ---------------------------------------------------------------------------

CUDACameraTrackingMultiRes::CUDACameraTrackingMultiRes(unsigned int imageWidth, unsigned int imageHeight, unsigned int levels, vhStream_t stream)
    : m_levels(levels), m_stream(stream), m_icp(imageWidth, imageHeight, levels, "CUDACameraTrackingMultiRes")
{
    std::memset(&m_lastState, 0, sizeof(m_lastState));
    for (unsigned int i = 0; i < levels; i++) {
        const size_t n = 4 * (size_t)m_icp.width[i] * m_icp.height[i];
        d_input.push_back(i ? vh::deviceAlloc<float>(n, "d_input") : nullptr);
        d_inputNormal.push_back(i ? vh::deviceAlloc<float>(n, "d_inputNormal") : nullptr);
    }
}

CUDACameraTrackingMultiRes::~CUDACameraTrackingMultiRes() { (void)hipStreamSynchronize((hipStream_t)m_stream); }

bool CUDACameraTrackingMultiRes::isTrackingLost(const vh::mat4f& m) { return m.m[0] == -std::numeric_limits<float>::infinity(); }

vh::mat4f CUDACameraTrackingMultiRes::applyCT(float* dInput, float* dInputNormals, float* dModel, float* dModelNormals, const vh::mat4f& lastTransform,
                                              const VhTrackingState& ts, const vh::mat4f& deltaTransformEstimate, const DepthCameraParams& cp)
{
    if (!dInput || !dInputNormals || !dModel || !dModelNormals) throw vh::Error(VH_ERR_BAD_ARGUMENT, "applyCT: null map");
    hipStream_t s = (hipStream_t)m_stream;
    const vh::IcpPyramid in = vh::icpPyramid(dInput, dInputNormals, d_input, d_inputNormal);
    const vh::IcpPyramid mdl = vh::icpPyramid(dModel, dModelNormals, m_icp.model, m_icp.modelNormal);
    for (unsigned int i = 0; i + 1 < m_levels; i++) { // the pyramids, :256-263
        m_icp.coarserLevel(in, i, m_stream);
        m_icp.coarserLevel(mdl, i, m_stream);
    }
    checkHip(hipMemcpyAsync(m_icp.estimate.get(), deltaTransformEstimate.m, sizeof(float) * 16, hipMemcpyHostToDevice, s), "deltaEstimate");
    m_icp.align(in, mdl, ts, cp, false, nullptr, 0u, m_stream); // three kernels an iteration; the outcome is copied back
    checkHip(hipMemcpyAsync(&m_lastState, m_icp.state.get(), sizeof(VhIcpState), hipMemcpyDeviceToHost, s), "VhIcpState");
    checkHip(hipStreamSynchronize(s), "applyCT");
    return trackedPose(m_lastState, lastTransform);
}

// ---------------------------------------------------------------------------
// vh::IcpSolverRGBD: the RGB-D solve, enqueued here for both its hosts
// ---------------------------------------------------------------------------

vh::IcpIntensityPyramid vh::icpIntensityPyramid(const std::vector<DevicePtr<float>>& intensity, const std::vector<DevicePtr<float>>& filtered)
{
    IcpIntensityPyramid p = {};
    for (size_t i = 0; i < intensity.size(); i++) { p.intensity[i] = intensity[i].get(); p.filtered[i] = filtered[i].get(); }
    return p;
}

vh::IcpSolverRGBD::IcpSolverRGBD(unsigned int imageWidth, unsigned int imageHeight, unsigned int levels, const char* who)
{
    checkPyramid(imageWidth, imageHeight, levels, who);
    unsigned int fac = 1;
    uint32_t nPartials = 0;
    for (unsigned int i = 0; i < levels; i++) { // :39-94
        width.push_back(imageWidth / fac);
        height.push_back(imageHeight / fac);
        const size_t n = (size_t)width[i] * height[i];
        model.push_back(i ? deviceAlloc<float>(4 * n, "d_model") : nullptr); // the finest level is the caller's maps
        modelNormal.push_back(i ? deviceAlloc<float>(4 * n, "d_modelNormal") : nullptr);
        modelIntensity.push_back(deviceAlloc<float>(n, "d_modelIntensity"));
        modelIntensityFiltered.push_back(i ? deviceAlloc<float>(n, "d_modelIntensityFiltered") : nullptr); // level 0: the unfiltered map (:267 copies it)
        modelIntensityAndDerivatives.push_back(deviceAlloc<float>(4 * n, "d_modelIntensityAndDerivatives"));
        nPartials = std::max(nPartials, vh_icp_rgbd_num_partials(width[i], height[i], i));
        fac *= 2;
    }
    partials = deviceAlloc<float>(30 * (size_t)nPartials, "d_partials");
    state = deviceAlloc<VhIcpStateRGBD>(1, "VhIcpStateRGBD");
    estimate = deviceAlloc<float>(16, "deltaEstimate");
    ticket = deviceAlloc<uint32_t>(1, "tracking ticket");
}

namespace {
const float kIntensitySigmaD = 3.0f, kIntensitySigmaR = 1.0f; // :262-263
}

void vh::IcpSolverRGBD::inputPyramid(const IcpPyramid& in, const float* dInputColor, const IcpIntensityPyramid& it, vhStream_t stream) const
{
    check(vh_convert_color_to_intensity_float(it.intensity[0], dInputColor, width[0], height[0], stream), "convertColorToIntensityFloat");
    for (unsigned int i = 0; i + 1 < width.size(); i++) {
        const unsigned int w = width[i], h = height[i], w1 = width[i + 1], h1 = height[i + 1];
        check(vh_resample_float4_map(in.map[i + 1], w1, h1, in.map[i], w, h, stream), "resampleFloat4Map");
        check(vh_compute_normals(in.normal[i + 1], in.map[i + 1], w1, h1, stream), "computeNormals");
        check(vh_resample_float_map(it.intensity[i + 1], w1, h1, it.intensity[i], w, h, stream), "resampleFloatMap");
        check(vh_gauss_filter_float_map(it.filtered[i + 1], it.intensity[i + 1], kIntensitySigmaD, kIntensitySigmaR, w1, h1, stream), "gaussFilterFloatMap");
    }
}

void vh::IcpSolverRGBD::modelPyramid(const IcpPyramid& mdl, const float* dModelColor, vhStream_t stream) const
{
    check(vh_convert_color_to_intensity_float(modelIntensity[0].get(), dModelColor, width[0], height[0], stream), "convertColorToIntensityFloat");
    check(vh_compute_intensity_and_derivatives(modelIntensity[0].get(), width[0], height[0], modelIntensityAndDerivatives[0].get(), stream), "computeIntensityAndDerivatives");
    for (unsigned int i = 0; i + 1 < width.size(); i++) {
        const unsigned int w = width[i], h = height[i], w1 = width[i + 1], h1 = height[i + 1];
        check(vh_resample_float4_map(mdl.map[i + 1], w1, h1, mdl.map[i], w, h, stream), "resampleFloat4Map");
        check(vh_compute_normals(mdl.normal[i + 1], mdl.map[i + 1], w1, h1, stream), "computeNormals");
        check(vh_resample_float_map(modelIntensity[i + 1].get(), w1, h1, modelIntensity[i].get(), w, h, stream), "resampleFloatMap");
        check(vh_gauss_filter_float_map(modelIntensityFiltered[i + 1].get(), modelIntensity[i + 1].get(), kIntensitySigmaD, kIntensitySigmaR, w1, h1, stream), "gaussFilterFloatMap");
        check(vh_compute_intensity_and_derivatives(modelIntensityFiltered[i + 1].get(), w1, h1, modelIntensityAndDerivatives[i + 1].get(), stream),
              "computeIntensityAndDerivatives");
    }
}

void vh::IcpSolverRGBD::align(const IcpPyramid& in, const IcpIntensityPyramid& it, const IcpPyramid& mdl, const VhTrackingStateRGBD& ts,
                              const DepthCameraParams& cp, bool fusedStep, VhIcpResult* d_result, uint32_t tag, vhStream_t stream) const
{
    if (fusedStep) checkHip(hipMemsetAsync(ticket.get(), 0, sizeof(uint32_t), (hipStream_t)stream), "tracking ticket");
    check(vh_icp_rgbd_begin(state.get(), estimate.get(), stream), "vh_icp_rgbd_begin");
    bool published = false;
    // coarse to fine, :289-321; align :329-353 with the loop exits taken on the device
    for (int level = (int)width.size() - 1; level >= 0; level--) {
        const unsigned int W = width[level], H = height[level];
        const float levelFactor = std::pow(2.0f, (float)level);
        VhIcpRGBDParams prm;
        prm.fx = cp.fx / levelFactor; prm.fy = cp.fy / levelFactor; prm.mx = cp.mx / levelFactor; prm.my = cp.my / levelFactor;
        prm.weightDepth = ts.s_weightsDepth[level];
        prm.weightColor = ts.s_weightsColor[level];
        prm.distThres = ts.base.s_distThres[level];
        prm.normalThres = ts.base.s_normalThres[level];
        prm.sensorMaxDepth = cp.m_sensorDepthWorldMax; // GlobalAppState::s_sensorDepthMax
        prm.colorGradientMin = ts.s_colorGradientMin[level];
        prm.colorThres = ts.s_colorThres[level];
        prm.level = (uint32_t)level;
        const float* inIntensity = level ? it.filtered[level] : it.intensity[0];
        const uint32_t nP = vh_icp_rgbd_num_partials(W, H, (uint32_t)level);
        check(vh_icp_begin_level(&state.get()->icp, stream), "vh_icp_begin_level");
        for (unsigned int outer = 0; outer < ts.base.s_maxOuterIter[level]; outer++) {
            if (fusedStep) {
                VhIcpResult* const publish = publishedByStep(ts.base, width.size(), level, outer, d_result);
                check(vh_icp_rgbd_step(W, H, partials.get(), ticket.get(), in.map[level], in.normal[level], inIntensity, mdl.map[level], mdl.normal[level],
                                       modelIntensityAndDerivatives[level].get(), &prm, state.get(), ts.base.s_angleTransThres[level],
                                       ts.base.s_distTransThres[level], ts.base.s_residualEarlyOut[level], publish, tag, stream),
                      "vh_icp_rgbd_step");
                published = published || publish;
                continue;
            }
            check(vh_icp_rgbd_build_linear_system(W, H, partials.get(), in.map[level], in.normal[level], inIntensity, mdl.map[level], mdl.normal[level],
                                                  modelIntensityAndDerivatives[level].get(), &prm, state.get(), stream), "computeNormalEquations");
            check(vh_icp_rgbd_solve(state.get(), partials.get(), nP, ts.base.s_angleTransThres[level], ts.base.s_distTransThres[level],
                                    ts.base.s_residualEarlyOut[level], stream), "vh_icp_rgbd_solve");
        }
    }
    publishAfterwards(&state.get()->icp, d_result, published, tag, stream);
}

// ---------------------------------------------------------------------------
// CUDACameraTrackingMultiResRGBD (DSC/CUDACameraTrackingMultiResRGBD.cpp) over the vh_icp_rgbd_* steps
// ---------------------------------------------------------------------------

CUDACameraTrackingMultiResRGBD::CUDACameraTrackingMultiResRGBD(unsigned int imageWidth, unsigned int imageHeight, unsigned int levels, vhStream_t stream)
    : m_levels(levels), m_stream(stream), m_icp(imageWidth, imageHeight, levels, "CUDACameraTrackingMultiResRGBD")
{
    std::memset(&m_lastState, 0, sizeof(m_lastState));
    for (unsigned int i = 0; i < levels; i++) {
        const size_t n = (size_t)m_icp.width[i] * m_icp.height[i];
        d_input.push_back(i ? vh::deviceAlloc<float>(4 * n, "d_input") : nullptr); // the finest level is the caller's maps
        d_inputNormal.push_back(i ? vh::deviceAlloc<float>(4 * n, "d_inputNormal") : nullptr);
        d_inputIntensity.push_back(vh::deviceAlloc<float>(n, "d_inputIntensity"));
        d_inputIntensityFiltered.push_back(i ? vh::deviceAlloc<float>(n, "d_inputIntensityFiltered") : nullptr);
    }
}

CUDACameraTrackingMultiResRGBD::~CUDACameraTrackingMultiResRGBD() { (void)hipStreamSynchronize((hipStream_t)m_stream); }

bool CUDACameraTrackingMultiResRGBD::isTrackingLost(const vh::mat4f& m) { return m.m[0] == -std::numeric_limits<float>::infinity(); }

vh::mat4f CUDACameraTrackingMultiResRGBD::applyCT(float* dInput, float* dInputNormals, float* dInputColor, float* dModel, float* dModelNormals,
                                                  float* dModelColor, const vh::mat4f& lastTransform, const VhTrackingStateRGBD& ts,
                                                  const vh::mat4f& deltaTransformEstimate, const DepthCameraParams& cp)
{
    if (!dInput || !dInputNormals || !dInputColor || !dModel || !dModelNormals || !dModelColor) throw vh::Error(VH_ERR_BAD_ARGUMENT, "applyCT: null map");
    hipStream_t s = (hipStream_t)m_stream;
    const vh::IcpPyramid in = vh::icpPyramid(dInput, dInputNormals, d_input, d_inputNormal);
    const vh::IcpPyramid mdl = vh::icpPyramid(dModel, dModelNormals, m_icp.model, m_icp.modelNormal);
    const vh::IcpIntensityPyramid it = vh::icpIntensityPyramid(d_inputIntensity, d_inputIntensityFiltered);
    m_icp.inputPyramid(in, dInputColor, it, m_stream); // the pyramids, :264-284
    m_icp.modelPyramid(mdl, dModelColor, m_stream);
    checkHip(hipMemcpyAsync(m_icp.estimate.get(), deltaTransformEstimate.m, sizeof(float) * 16, hipMemcpyHostToDevice, s), "deltaEstimate");
    m_icp.align(in, it, mdl, ts, cp, false, nullptr, 0u, m_stream); // two kernels an iteration; the outcome is copied back
    checkHip(hipMemcpyAsync(&m_lastState, m_icp.state.get(), sizeof(VhIcpStateRGBD), hipMemcpyDeviceToHost, s), "VhIcpStateRGBD");
    checkHip(hipStreamSynchronize(s), "applyCT");
    return trackedPose(m_lastState.icp, lastTransform);
}

// ---------------------------------------------------------------------------
// zParametersTracking*.txt: the ParameterFile rules of vh_params.cpp, members s_name[level]
// ---------------------------------------------------------------------------

namespace {
void parseTracking(const std::map<std::string, std::string>& values, VhTrackingState* out)
{
    std::memset(out, 0, sizeof(*out));
    auto u32 = [&](const std::string& k, uint32_t& v) { auto it = values.find(k); if (it == values.end()) return false; try { v = (uint32_t)std::stoi(it->second); } catch (...) { v = 0; } return true; };
    auto f32 = [&](const std::string& k, float& v) { auto it = values.find(k); if (it == values.end()) return false; try { v = std::stof(it->second); } catch (...) { v = 0.0f; } return true; };
    u32("s_maxLevels", out->s_maxLevels);
    for (unsigned int i = 0; i < VH_TRACKING_MAX_LEVELS; i++) { // readParameter(name, std::vector<U>&): name[0], name[1], ... until one is missing
        const std::string idx = "[" + std::to_string(i) + "]";
        if (!u32("s_maxOuterIter" + idx, out->s_maxOuterIter[i])) break;
        out->numLevelsFound = i + 1;
        u32("s_maxInnerIter" + idx, out->s_maxInnerIter[i]);
        f32("s_distThres" + idx, out->s_distThres[i]);
        f32("s_normalThres" + idx, out->s_normalThres[i]);
        f32("s_angleTransThres" + idx, out->s_angleTransThres[i]);
        f32("s_distTransThres" + idx, out->s_distTransThres[i]);
        f32("s_residualEarlyOut" + idx, out->s_residualEarlyOut[i]);
    }
}
// the f5 members as parseTracking reads them; s_weightsDepth, s_weightsColor, s_colorGradientMin and s_colorThres per
// level, setDefault's values (DSC/GlobalCameraTrackingState.h:67-71) where the file has no entry
void parseTrackingRGBD(const std::map<std::string, std::string>& values, VhTrackingStateRGBD* out)
{
    std::memset(out, 0, sizeof(*out));
    parseTracking(values, &out->base);
    auto f32 = [&](const std::string& k, float& v, float dflt) {
        auto it = values.find(k);
        if (it == values.end()) { v = dflt; return; }
        try { v = std::stof(it->second); } catch (...) { v = 0.0f; }
    };
    for (unsigned int i = 0; i < VH_TRACKING_MAX_LEVELS; i++) {
        const std::string idx = "[" + std::to_string(i) + "]";
        f32("s_weightsDepth" + idx, out->s_weightsDepth[i], 1.0f);
        f32("s_weightsColor" + idx, out->s_weightsColor[i], 1.0f);
        f32("s_colorGradientMin" + idx, out->s_colorGradientMin[i], 0.005f);
        f32("s_colorThres" + idx, out->s_colorThres[i], 0.1f);
    }
}
// the four C entry points below: a file or a text through parseTracking or parseTrackingRGBD
template <class State>
int parseWith(void (*parse)(const vh::ParamValues&, State*), std::istream& in, State* out)
{
    vh::ParamValues values;
    vh::parseStream(in, values);
    parse(values, out);
    return VH_OK;
}
template <class State>
int readWith(void (*parse)(const vh::ParamValues&, State*), const char* filename, State* out)
{
    if (!filename || !out) return VH_ERR_BAD_ARGUMENT;
    std::ifstream f(filename);
    return f.is_open() ? parseWith(parse, f, out) : VH_ERR_IO;
}
template <class State>
int parseTextWith(void (*parse)(const vh::ParamValues&, State*), const char* text, State* out)
{
    if (!text || !out) return VH_ERR_BAD_ARGUMENT;
    std::istringstream in(text);
    return parseWith(parse, in, out);
}
} // namespace

extern "C" {

int vh_tracking_state_read(const char* filename, VhTrackingState* out) { return readWith(parseTracking, filename, out); }
int vh_tracking_state_parse(const char* text, VhTrackingState* out) { return parseTextWith(parseTracking, text, out); }
int vh_tracking_state_rgbd_read(const char* filename, VhTrackingStateRGBD* out) { return readWith(parseTrackingRGBD, filename, out); }
int vh_tracking_state_rgbd_parse(const char* text, VhTrackingStateRGBD* out) { return parseTextWith(parseTrackingRGBD, text, out); }

} // extern "C"
