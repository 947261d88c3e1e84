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

namespace {
inline void check(int code, const char* what)
{
    if (code != 0) throw vh::Error(code, std::string(what) + ": " + vh_error_string(code));
}
inline void checkHip(hipError_t e, const char* what)
{
    if (e != hipSuccess) throw vh::Error(-(int)e, std::string(what) + ": " + hipGetErrorString(e));
}
float* allocFloats(size_t n, const char* what)
{
    float* p = nullptr;
    checkHip(hipMalloc((void**)&p, sizeof(float) * (n ? n : 1)), what);
    return p;
}
} // namespace

CUDACameraTrackingMultiRes::CUDACameraTrackingMultiRes(unsigned int imageWidth, unsigned int imageHeight, unsigned int levels, vhStream_t stream)
    : m_levels(levels), m_stream(stream), d_partials(nullptr), d_state(nullptr), d_deltaEstimate(nullptr)
{
    if (levels == 0 || levels > VH_TRACKING_MAX_LEVELS || (imageWidth >> (levels - 1)) < 2 || (imageHeight >> (levels - 1)) < 2)
        throw vh::Error(VH_ERR_BAD_ARGUMENT, "CUDACameraTrackingMultiRes: bad pyramid");
    std::memset(&m_lastState, 0, sizeof(m_lastState));
    unsigned int fac = 1;
    for (unsigned int i = 0; i < levels; i++) { // :39-95
        m_imageWidth.push_back(imageWidth / fac);
        m_imageHeight.push_back(imageHeight / fac);
        const size_t n = 4 * (size_t)m_imageWidth[i] * m_imageHeight[i];
        d_correspondence.push_back(allocFloats(n, "d_correspondence"));
        d_correspondenceNormal.push_back(allocFloats(n, "d_correspondenceNormal"));
        d_input.push_back(i ? allocFloats(n, "d_input") : nullptr); // the finest level is the caller's maps
        d_inputNormal.push_back(i ? allocFloats(n, "d_inputNormal") : nullptr);
        d_model.push_back(i ? allocFloats(n, "d_model") : nullptr);
        d_modelNormal.push_back(i ? allocFloats(n, "d_modelNormal") : nullptr);
        fac *= 2;
    }
    d_partials = allocFloats(30 * (size_t)vh_icp_num_partials(imageWidth, imageHeight), "d_partials");
    checkHip(hipMalloc((void**)&d_state, sizeof(VhIcpState)), "VhIcpState");
    d_deltaEstimate = allocFloats(16, "deltaEstimate");
}

CUDACameraTrackingMultiRes::~CUDACameraTrackingMultiRes()
{
    (void)hipStreamSynchronize((hipStream_t)m_stream);
    for (auto* v : { &d_correspondence, &d_correspondenceNormal, &d_input, &d_inputNormal, &d_model, &d_modelNormal })
        for (float* p : *v)
            if (p) (void)hipFree(p);
    if (d_partials) (void)hipFree(d_partials);
    if (d_state) (void)hipFree(d_state);
    if (d_deltaEstimate) (void)hipFree(d_deltaEstimate);
}

bool CUDACameraTrackingMultiRes::isTrackingLost(const vh::mat4f& m) { return m.m[0] == -std::numeric_limits<float>::infinity(); }

vh::mat4f CUDACameraTrackingMultiRes::applyCT(float* dInput, float* dInputNormals, float* dModel, float* dModelNormals, const vh::mat4f& lastTransform,
                                              const VhTrackingState& ts, const vh::mat4f& deltaTransformEstimate, const DepthCameraParams& cp)
{
    if (!dInput || !dInputNormals || !dModel || !dModelNormals) throw vh::Error(VH_ERR_BAD_ARGUMENT, "applyCT: null map");
    hipStream_t s = (hipStream_t)m_stream;
    d_input[0] = dInput; d_inputNormal[0] = dInputNormals;
    d_model[0] = dModel; d_modelNormal[0] = dModelNormals;
    // the pyramids, :256-263
    for (unsigned int i = 0; i + 1 < m_levels; i++) {
        check(vh_resample_float4_map(d_input[i + 1], m_imageWidth[i + 1], m_imageHeight[i + 1], d_input[i], m_imageWidth[i], m_imageHeight[i], m_stream), "resampleFloat4Map");
        check(vh_compute_normals(d_inputNormal[i + 1], d_input[i + 1], m_imageWidth[i + 1], m_imageHeight[i + 1], m_stream), "computeNormals");
        check(vh_resample_float4_map(d_model[i + 1], m_imageWidth[i + 1], m_imageHeight[i + 1], d_model[i], m_imageWidth[i], m_imageHeight[i], m_stream), "resampleFloat4Map");
        check(vh_compute_normals(d_modelNormal[i + 1], d_model[i + 1], m_imageWidth[i + 1], m_imageHeight[i + 1], m_stream), "computeNormals");
    }
    checkHip(hipMemcpyAsync(d_deltaEstimate, deltaTransformEstimate.m, sizeof(float) * 16, hipMemcpyHostToDevice, s), "deltaEstimate");
    check(vh_icp_begin(d_state, d_deltaEstimate, m_stream), "vh_icp_begin");
    // coarse to fine, :265-279; align :291-321 with the loop exits taken on the device
    for (int level = (int)m_levels - 1; level >= 0; level--) {
        const unsigned int W = m_imageWidth[level], H = m_imageHeight[level];
        const float levelFactor = std::pow(2.0f, (float)level);
        check(vh_icp_begin_level(d_state, m_stream), "vh_icp_begin_level");
        for (unsigned int outer = 0; outer < ts.s_maxOuterIter[level]; outer++) {
            check(vh_icp_projective_correspondences(d_input[level], d_inputNormal[level], d_model[level], d_modelNormal[level], d_correspondence[level],
                                                    d_correspondenceNormal[level], W, H, ts.s_distThres[level], ts.s_normalThres[level], levelFactor,
                                                    d_state, &cp, m_stream), "projectiveCorrespondences");
            const unsigned int inner = ts.s_maxInnerIter[level];
            for (unsigned int i = 0; i < inner; i++) {
                check(vh_icp_build_linear_system(W, H, d_partials, d_input[level], d_correspondence[level], d_correspondenceNormal[level], d_state, m_stream), "buildLinearSystem");
                check(vh_icp_solve(d_state, d_partials, vh_icp_num_partials(W, H), ts.s_angleTransThres[level], ts.s_distTransThres[level],
                                   ts.s_residualEarlyOut[level], i + 1 == inner, m_stream), "vh_icp_solve");
            }
        }
    }
    checkHip(hipMemcpyAsync(&m_lastState, d_state, sizeof(VhIcpState), hipMemcpyDeviceToHost, s), "VhIcpState");
    checkHip(hipStreamSynchronize(s), "applyCT");
    d_input[0] = d_inputNormal[0] = d_model[0] = d_modelNormal[0] = nullptr;
    vh::mat4f out;
    if (m_lastState.lost) {
        for (float& v : out.m) v = -std::numeric_limits<float>::infinity();
        return out;
    }
    vh::mat4f delta;
    std::memcpy(delta.m, m_lastState.delta, sizeof(delta.m));
    return lastTransform * delta;
}

// ---------------------------------------------------------------------------
// CUDACameraTrackingMultiResRGBD (DSC/CUDACameraTrackingMultiResRGBD.cpp) over the vh_icp_rgbd_* steps
// ---------------------------------------------------------------------------

CUDACameraTrackingMultiResRGBD::CUDACameraTrackingMultiResRGBD(unsigned int imageWidth, unsigned int imageHeight, unsigned int levels, vhStream_t stream)
    : m_levels(levels), m_stream(stream), d_partials(nullptr), d_state(nullptr), d_deltaEstimate(nullptr)
{
    if (levels == 0 || levels > VH_TRACKING_MAX_LEVELS || (imageWidth >> (levels - 1)) < 2 || (imageHeight >> (levels - 1)) < 2)
        throw vh::Error(VH_ERR_BAD_ARGUMENT, "CUDACameraTrackingMultiResRGBD: bad pyramid");
    std::memset(&m_lastState, 0, sizeof(m_lastState));
    unsigned int fac = 1;
    uint32_t partials = 0;
    for (unsigned int i = 0; i < levels; i++) { // :39-94
        m_imageWidth.push_back(imageWidth / fac);
        m_imageHeight.push_back(imageHeight / fac);
        const size_t n = (size_t)m_imageWidth[i] * m_imageHeight[i];
        d_input.push_back(i ? allocFloats(4 * n, "d_input") : nullptr); // the finest level is the caller's maps
        d_inputNormal.push_back(i ? allocFloats(4 * n, "d_inputNormal") : nullptr);
        d_inputIntensity.push_back(allocFloats(n, "d_inputIntensity"));
        d_inputIntensityFiltered.push_back(i ? allocFloats(n, "d_inputIntensityFiltered") : nullptr); // level 0: the unfiltered map (:267 copies it)
        d_model.push_back(i ? allocFloats(4 * n, "d_model") : nullptr);
        d_modelNormal.push_back(i ? allocFloats(4 * n, "d_modelNormal") : nullptr);
        d_modelIntensity.push_back(allocFloats(n, "d_modelIntensity"));
        d_modelIntensityFiltered.push_back(i ? allocFloats(n, "d_modelIntensityFiltered") : nullptr);
        d_modelIntensityAndDerivatives.push_back(allocFloats(4 * n, "d_modelIntensityAndDerivatives"));
        partials = std::max(partials, vh_icp_rgbd_num_partials(m_imageWidth[i], m_imageHeight[i], i));
        fac *= 2;
    }
    d_partials = allocFloats(30 * (size_t)partials, "d_partials");
    checkHip(hipMalloc((void**)&d_state, sizeof(VhIcpStateRGBD)), "VhIcpStateRGBD");
    d_deltaEstimate = allocFloats(16, "deltaEstimate");
}

CUDACameraTrackingMultiResRGBD::~CUDACameraTrackingMultiResRGBD()
{
    (void)hipStreamSynchronize((hipStream_t)m_stream);
    for (auto* v : { &d_input, &d_inputNormal, &d_inputIntensity, &d_inputIntensityFiltered, &d_model, &d_modelNormal, &d_modelIntensity,
                     &d_modelIntensityFiltered, &d_modelIntensityAndDerivatives })
        for (float* p : *v)
            if (p) (void)hipFree(p);
    if (d_partials) (void)hipFree(d_partials);
    if (d_state) (void)hipFree(d_state);
    if (d_deltaEstimate) (void)hipFree(d_deltaEstimate);
}

bool CUDACameraTrackingMultiResRGBD::isTrackingLost(const vh::mat4f& m) { return m.m[0] == -std::numeric_limits<float>::infinity(); }

vh::mat4f CUDACameraTrackingMultiResRGBD::applyCT(float* dInput, float* dInputNormals, float* dInputColor, float* dModel, float* dModelNormals,
                                                  float* dModelColor, const vh::mat4f& lastTransform, const VhTrackingStateRGBD& ts,
                                                  const vh::mat4f& deltaTransformEstimate, const DepthCameraParams& cp)
{
    if (!dInput || !dInputNormals || !dInputColor || !dModel || !dModelNormals || !dModelColor) throw vh::Error(VH_ERR_BAD_ARGUMENT, "applyCT: null map");
    hipStream_t s = (hipStream_t)m_stream;
    d_input[0] = dInput; d_inputNormal[0] = dInputNormals;
    d_model[0] = dModel; d_modelNormal[0] = dModelNormals;
    const unsigned int W0 = m_imageWidth[0], H0 = m_imageHeight[0];
    // the pyramids, :264-284
    check(vh_convert_color_to_intensity_float(d_inputIntensity[0], dInputColor, W0, H0, m_stream), "convertColorToIntensityFloat");
    check(vh_convert_color_to_intensity_float(d_modelIntensity[0], dModelColor, W0, H0, m_stream), "convertColorToIntensityFloat");
    check(vh_compute_intensity_and_derivatives(d_modelIntensity[0], W0, H0, d_modelIntensityAndDerivatives[0], m_stream), "computeIntensityAndDerivatives");
    const float sigmaD = 3.0f, sigmaR = 1.0f;
    for (unsigned int i = 0; i + 1 < m_levels; i++) {
        const unsigned int w = m_imageWidth[i], h = m_imageHeight[i], w1 = m_imageWidth[i + 1], h1 = m_imageHeight[i + 1];
        check(vh_resample_float4_map(d_input[i + 1], w1, h1, d_input[i], w, h, m_stream), "resampleFloat4Map");
        check(vh_compute_normals(d_inputNormal[i + 1], d_input[i + 1], w1, h1, m_stream), "computeNormals");
        check(vh_resample_float_map(d_inputIntensity[i + 1], w1, h1, d_inputIntensity[i], w, h, m_stream), "resampleFloatMap");
        check(vh_gauss_filter_float_map(d_inputIntensityFiltered[i + 1], d_inputIntensity[i + 1], sigmaD, sigmaR, w1, h1, m_stream), "gaussFilterFloatMap");
        check(vh_resample_float4_map(d_model[i + 1], w1, h1, d_model[i], w, h, m_stream), "resampleFloat4Map");
        check(vh_compute_normals(d_modelNormal[i + 1], d_model[i + 1], w1, h1, m_stream), "computeNormals");
        check(vh_resample_float_map(d_modelIntensity[i + 1], w1, h1, d_modelIntensity[i], w, h, m_stream), "resampleFloatMap");
        check(vh_gauss_filter_float_map(d_modelIntensityFiltered[i + 1], d_modelIntensity[i + 1], sigmaD, sigmaR, w1, h1, m_stream), "gaussFilterFloatMap");
        check(vh_compute_intensity_and_derivatives(d_modelIntensityFiltered[i + 1], w1, h1, d_modelIntensityAndDerivatives[i + 1], m_stream),
              "computeIntensityAndDerivatives");
    }
    checkHip(hipMemcpyAsync(d_deltaEstimate, deltaTransformEstimate.m, sizeof(float) * 16, hipMemcpyHostToDevice, s), "deltaEstimate");
    check(vh_icp_rgbd_begin(d_state, d_deltaEstimate, m_stream), "vh_icp_rgbd_begin");
    // coarse to fine, :289-321; align :329-353 with the loop exits taken on the device
    for (int level = (int)m_levels - 1; level >= 0; level--) {
        const unsigned int W = m_imageWidth[level], H = m_imageHeight[level];
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
        const float* inIntensity = level ? d_inputIntensityFiltered[level] : d_inputIntensity[0];
        const uint32_t nP = vh_icp_rgbd_num_partials(W, H, (uint32_t)level);
        check(vh_icp_begin_level(&d_state->icp, m_stream), "vh_icp_begin_level");
        for (unsigned int outer = 0; outer < ts.base.s_maxOuterIter[level]; outer++) {
            check(vh_icp_rgbd_build_linear_system(W, H, d_partials, d_input[level], d_inputNormal[level], inIntensity, d_model[level], d_modelNormal[level],
                                                  d_modelIntensityAndDerivatives[level], &prm, d_state, m_stream), "computeNormalEquations");
            check(vh_icp_rgbd_solve(d_state, d_partials, nP, ts.base.s_angleTransThres[level], ts.base.s_distTransThres[level],
                                    ts.base.s_residualEarlyOut[level], m_stream), "vh_icp_rgbd_solve");
        }
    }
    checkHip(hipMemcpyAsync(&m_lastState, d_state, sizeof(VhIcpStateRGBD), hipMemcpyDeviceToHost, s), "VhIcpStateRGBD");
    checkHip(hipStreamSynchronize(s), "applyCT");
    d_input[0] = d_inputNormal[0] = d_model[0] = d_modelNormal[0] = nullptr;
    vh::mat4f out;
    if (m_lastState.icp.lost) {
        for (float& v : out.m) v = -std::numeric_limits<float>::infinity();
        return out;
    }
    vh::mat4f delta;
    std::memcpy(delta.m, m_lastState.icp.delta, sizeof(delta.m));
    return lastTransform * delta;
}

// ---------------------------------------------------------------------------
// zParametersTracking*.txt: the ParameterFile rules of vh_params.cpp, members s_name[level]
// ---------------------------------------------------------------------------

namespace {
void stripT(std::string& s)
{
    const std::string junk = " \t\";";
    while (!s.empty() && junk.find(s.front()) != std::string::npos) s.erase(s.begin());
    while (!s.empty() && junk.find(s.back()) != std::string::npos) s.pop_back();
}
std::map<std::string, std::string> readValues(std::istream& in)
{
    std::map<std::string, std::string> values;
    std::string line;
    while (std::getline(in, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        for (const char* c : { "//", "#", ";" }) {
            const size_t at = line.find(c);
            if (at != std::string::npos) line = line.substr(0, at);
        }
        stripT(line);
        const size_t sep = line.find('=');
        if (line.empty() || sep == std::string::npos) continue;
        std::string name = line.substr(0, sep), value = line.substr(sep + 1);
        stripT(name); stripT(value);
        if (!name.empty()) values[name] = value;
    }
    return values;
}
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
} // namespace

extern "C" {

int vh_tracking_state_read(const char* filename, VhTrackingState* out)
{
    if (!filename || !out) return VH_ERR_BAD_ARGUMENT;
    std::ifstream f(filename);
    if (!f.is_open()) return VH_ERR_IO;
    parseTracking(readValues(f), out);
    return VH_OK;
}

int vh_tracking_state_parse(const char* text, VhTrackingState* out)
{
    if (!text || !out) return VH_ERR_BAD_ARGUMENT;
    std::istringstream in(text);
    parseTracking(readValues(in), out);
    return VH_OK;
}

int vh_tracking_state_rgbd_read(const char* filename, VhTrackingStateRGBD* out)
{
    if (!filename || !out) return VH_ERR_BAD_ARGUMENT;
    std::ifstream f(filename);
    if (!f.is_open()) return VH_ERR_IO;
    parseTrackingRGBD(readValues(f), out);
    return VH_OK;
}

int vh_tracking_state_rgbd_parse(const char* text, VhTrackingStateRGBD* out)
{
    if (!text || !out) return VH_ERR_BAD_ARGUMENT;
    std::istringstream in(text);
    parseTrackingRGBD(readValues(in), out);
    return VH_OK;
}

} // extern "C"
