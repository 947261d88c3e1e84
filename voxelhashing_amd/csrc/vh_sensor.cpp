// vh_sensor.cpp -- the per-frame image path between a depth sensor and integrate(): CUDARGBDAdapter::process
// (DSC/CUDARGBDAdapter.cpp:93-137) followed by CUDARGBDSensor::process (DSC/CUDARGBDSensor.cpp:147-257), as one
// host class over the kernels of vh_image.hip (sensor pre-processing).  The D3D11 remapping branch
// (s_bUseCameraCalibration, :198-217) is the depth map drawn into the colour camera by the view passes of vh_view.hip
// (vh_view_raster + vh_view_resolve_depth, render target 0 straight into d_depthData); setCameraCalibration switches it
// on.  The disabled erosion loop (:224-237) is not part of it.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/vh.hpp"
#include "vh_host_util.hpp"

extern "C" int vh_rgbd_sensor_remap_params(const uint32_t sizes[6], const float depthIntrinsics[4], const float colorIntrinsics[4],
                                           const float depthExtrinsics[16], float thresOffset, float thresLin, VhViewParams* out)
{
    if (!sizes || !depthIntrinsics || !colorIntrinsics || !depthExtrinsics || !out) return VH_ERR_BAD_ARGUMENT;
    for (int i = 0; i < 6; i++)
        if (sizes[i] < 2) return VH_ERR_BAD_ARGUMENT;
    const uint32_t dw = sizes[0], dh = sizes[1], cw = sizes[2], ch = sizes[3], W = sizes[4], H = sizes[5];
    // the adapter's intrinsics (DSC/CUDARGBDAdapter.cpp:54-66): the sensor's, rescaled to the adapter size.  The depth
    // ones are the constructor's DepthCameraParams, bit for bit.
    vh::mat4f depthK = vh::mat4f::identity(), colorK = vh::mat4f::identity();
    depthK.m[0] = depthIntrinsics[0] * ((float)W / (float)dw);
    depthK.m[5] = depthIntrinsics[1] * ((float)H / (float)dh);
    depthK.m[2] = depthIntrinsics[2] * ((float)(W - 1) / (float)(dw - 1));
    depthK.m[6] = depthIntrinsics[3] * ((float)(H - 1) / (float)(dh - 1));
    colorK.m[0] = colorIntrinsics[0] * ((float)W / (float)cw);
    colorK.m[5] = colorIntrinsics[1] * ((float)H / (float)ch);
    colorK.m[2] = colorIntrinsics[2] * ((float)(W - 1) / (float)(cw - 1));
    colorK.m[6] = colorIntrinsics[3] * ((float)(H - 1) / (float)(ch - 1));
    // getDepthIntrinsicsInv(): mLib's Matrix4x4::getInverse, the same cofactors in the same order as mat4f::getInverse
    const vh::mat4f depthKInv = depthK.getInverse();
    VhViewParams& p = *out;
    std::memset(&p, 0, sizeof(p));
    std::memcpy(p.intrinsicInverse, depthKInv.m, sizeof(p.intrinsicInverse));
    std::memcpy(p.modelview, depthExtrinsics, sizeof(p.modelview)); // getDepthExtrinsics(), not its inverse
    std::memcpy(p.intrinsicNew, colorK.m, sizeof(p.intrinsicNew));
    p.depthWidth = p.screenWidth = W; // the custom render target is the adapter size (CUDARGBDSensor.cpp:130-131)
    p.depthHeight = p.screenHeight = H;
    p.depthThreshOffset = thresOffset;
    p.depthThreshLin = thresLin;
    return VH_OK;
}

CUDARGBDSensor::CUDARGBDSensor(const Config& c, vhStream_t stream) : m_cfg(c), m_stream(stream), m_frameNumber(0)
{
    if (c.depthWidth < 2 || c.depthHeight < 2 || c.colorWidth < 2 || c.colorHeight < 2 || c.adapterWidth < 2 || c.adapterHeight < 2)
        throw vh::Error(VH_ERR_BAD_ARGUMENT, "CUDARGBDSensor: image sizes must be at least 2x2");
    m_bFilterDepthValues = c.filterDepth; m_fBilateralFilterSigmaD = c.sigmaD; m_fBilateralFilterSigmaR = c.sigmaR;
    m_bFilterIntensityValues = c.filterIntensity; m_fBilateralFilterSigmaDIntensity = c.sigmaDIntensity; m_fBilateralFilterSigmaRIntensity = c.sigmaRIntensity;
    // adapt intrinsics, DSC/CUDARGBDAdapter.cpp:56-62
    std::memset(&m_depthCameraParams, 0, sizeof(m_depthCameraParams));
    m_depthCameraParams.fx = c.fx * ((float)c.adapterWidth / (float)c.depthWidth);
    m_depthCameraParams.fy = c.fy * ((float)c.adapterHeight / (float)c.depthHeight);
    m_depthCameraParams.mx = c.mx * ((float)(c.adapterWidth - 1) / (float)(c.depthWidth - 1));
    m_depthCameraParams.my = c.my * ((float)(c.adapterHeight - 1) / (float)(c.depthHeight - 1));
    m_depthCameraParams.m_sensorDepthWorldMin = c.sensorDepthMin;
    m_depthCameraParams.m_sensorDepthWorldMax = c.sensorDepthMax;
    m_depthCameraParams.m_imageWidth = c.adapterWidth;
    m_depthCameraParams.m_imageHeight = c.adapterHeight;

    const size_t nDepthIn = (size_t)c.depthWidth * c.depthHeight, nColorIn = (size_t)c.colorWidth * c.colorHeight;
    const size_t nOut = (size_t)c.adapterWidth * c.adapterHeight;
    std::memset(&m_depthCameraData, 0, sizeof(m_depthCameraData));
    std::memset(&m_remapParams, 0, sizeof(m_remapParams));
    d_depthMapFloat = vh::deviceAlloc<float>(nDepthIn, "d_depthMapFloat");
    d_depthMapResampledFloat = vh::deviceAlloc<float>(nOut, "d_depthMapResampledFloat");
    d_colorMapRaw = vh::deviceAlloc<unsigned char>(4 * nColorIn, "d_colorMapRaw");
    d_colorMapFloat4 = vh::deviceAlloc<float>(4 * nColorIn, "d_colorMapFloat4");
    d_colorMapResampledFloat4 = vh::deviceAlloc<float>(4 * nOut, "d_colorMapResampledFloat4");
    d_depthMapFilteredFloat = vh::deviceAlloc<float>(nOut, "d_depthMapFilteredFloat");
    d_cameraSpaceFloat4 = vh::deviceAlloc<float>(4 * nOut, "d_cameraSpaceFloat4");
    d_normalMapFloat4 = vh::deviceAlloc<float>(4 * nOut, "d_normalMapFloat4");
    d_intensityMapFilteredFloat = vh::deviceAlloc<float>(nOut, "d_intensityMapFilteredFloat");
    d_depthData = vh::deviceAlloc<float>(nOut, "DepthCameraData::d_depthData");
    d_colorData = vh::deviceAlloc<float>(4 * nOut, "DepthCameraData::d_colorData");
    m_depthCameraData.d_depthData = d_depthData.get();
    m_depthCameraData.d_colorData = d_colorData.get();
    // a resampled pixel whose nearest source pixel is outside the source is left untouched by the reference:
    // start from "invalid" instead of from uninitialised memory
    check(vh_set_invalid_float_map(d_depthMapResampledFloat.get(), c.adapterWidth, c.adapterHeight, m_stream), "setInvalidFloatMap");
    checkHip(hipMemsetAsync(d_colorMapResampledFloat4.get(), 0, sizeof(float) * 4 * nOut, (hipStream_t)m_stream), "clear colour");
}

CUDARGBDSensor::~CUDARGBDSensor() { (void)hipStreamSynchronize((hipStream_t)m_stream); }

void CUDARGBDSensor::setFiterDepthValues(bool b, float sigmaD, float sigmaR)
{
    m_bFilterDepthValues = b; m_fBilateralFilterSigmaD = sigmaD; m_fBilateralFilterSigmaR = sigmaR;
}
void CUDARGBDSensor::setFiterIntensityValues(bool b, float sigmaD, float sigmaR)
{
    m_bFilterIntensityValues = b; m_fBilateralFilterSigmaDIntensity = sigmaD; m_fBilateralFilterSigmaRIntensity = sigmaR;
}

void CUDARGBDSensor::setCameraCalibration(bool enabled, float colorFx, float colorFy, float colorMx, float colorMy, const vh::mat4f& depthExtrinsics,
                                          float thresOffset, float thresLin)
{
    const Config& c = m_cfg;
    const unsigned int W = c.adapterWidth, H = c.adapterHeight;
    // mLib's operator==: entry by entry, exact.  Equal to the identity means already aligned: the remap stays off
    bool identity = true;
    const vh::mat4f I = vh::mat4f::identity();
    for (int i = 0; i < 16; i++) identity = identity && depthExtrinsics.m[i] == I.m[i];
    m_bUseCameraCalibration = false;
    if (!enabled || identity) return;
    const uint32_t sizes[6] = { c.depthWidth, c.depthHeight, c.colorWidth, c.colorHeight, W, H };
    const float depthIntrinsics[4] = { c.fx, c.fy, c.mx, c.my }, colorIntrinsics[4] = { colorFx, colorFy, colorMx, colorMy };
    check(vh_rgbd_sensor_remap_params(sizes, depthIntrinsics, colorIntrinsics, depthExtrinsics.m, thresOffset, thresLin, &m_remapParams), "remap params");
    // allocated once, all ones and a zero counter: every resolve leaves them so
    const hipStream_t s = (hipStream_t)m_stream;
    if (!d_remapKeys) {
        d_remapKeys = vh::deviceAlloc<uint64_t>((size_t)W * H, "remap keys");
        checkHip(hipMemsetAsync(d_remapKeys.get(), 0xff, sizeof(uint64_t) * (size_t)W * H, s), "remap keys");
    }
    if (!d_remapLargeList) {
        d_remapLargeList = vh::deviceAlloc<uint32_t>(vh_view_large_list_words(W, H), "remap list");
        checkHip(hipMemsetAsync(d_remapLargeList.get(), 0, sizeof(uint32_t), s), "remap list");
    }
    m_bUseCameraCalibration = true;
}

void CUDARGBDSensor::process(const float* h_depthFloat, const unsigned char* h_colorRGBX)
{
    if (!h_depthFloat || !h_colorRGBX) throw vh::Error(VH_ERR_BAD_ARGUMENT, "CUDARGBDSensor::process: null frame");
    const Config& c = m_cfg;
    const unsigned int W = c.adapterWidth, H = c.adapterHeight;
    hipStream_t s = (hipStream_t)m_stream;
    // ---- CUDARGBDAdapter::process :107-131
    checkHip(hipMemcpyAsync(d_colorMapRaw.get(), h_colorRGBX, 4 * (size_t)c.colorWidth * c.colorHeight, hipMemcpyHostToDevice, s), "upload colour");
    check(vh_convert_color_raw_to_float4(d_colorMapFloat4.get(), d_colorMapRaw.get(), c.colorWidth, c.colorHeight, m_stream), "convertColorRawToFloat4");
    if (c.colorWidth == W && c.colorHeight == H) check(vh_copy_float4_map(d_colorMapResampledFloat4.get(), d_colorMapFloat4.get(), W, H, m_stream), "copyFloat4Map");
    else check(vh_resample_float4_map(d_colorMapResampledFloat4.get(), W, H, d_colorMapFloat4.get(), c.colorWidth, c.colorHeight, m_stream), "resampleFloat4Map");
    checkHip(hipMemcpyAsync(d_depthMapFloat.get(), h_depthFloat, sizeof(float) * (size_t)c.depthWidth * c.depthHeight, hipMemcpyHostToDevice, s), "upload depth");
    check(vh_resample_float_map(d_depthMapResampledFloat.get(), W, H, d_depthMapFloat.get(), c.depthWidth, c.depthHeight, m_stream), "resampleFloatMap");
    // ---- CUDARGBDSensor::process :159-248
    if (m_bFilterIntensityValues) check(vh_gauss_filter_float4_map(d_colorData.get(), d_colorMapResampledFloat4.get(), m_fBilateralFilterSigmaDIntensity, m_fBilateralFilterSigmaRIntensity, W, H, m_stream), "gaussFilterFloat4Map");
    else check(vh_copy_float4_map(d_colorData.get(), d_colorMapResampledFloat4.get(), W, H, m_stream), "copyFloat4Map");
    if (m_bFilterDepthValues) check(vh_gauss_filter_float_map(d_depthMapFilteredFloat.get(), d_depthMapResampledFloat.get(), m_fBilateralFilterSigmaD, m_fBilateralFilterSigmaR, W, H, m_stream), "gaussFilterFloatMap");
    else check(vh_copy_float_map(d_depthMapFilteredFloat.get(), d_depthMapResampledFloat.get(), W, H, m_stream), "copyFloatMap");
    // (the reference also calls setInvalidFloatMap on d_depthData here and overwrites it right away, :188-219)
    if (m_bUseCameraCalibration) { // RenderDepthMap into the custom render target, then copyToCuda(d_depthData, 0)
        check(vh_view_raster(d_depthMapFilteredFloat.get(), &m_remapParams, d_remapKeys.get(), d_remapLargeList.get(), m_stream), "remap: raster");
        check(vh_view_resolve_depth(d_depthMapFilteredFloat.get(), &m_remapParams, d_remapKeys.get(), d_remapLargeList.get(), d_depthData.get(), m_stream), "remap: resolve");
    } else {
        check(vh_copy_float_map(d_depthData.get(), d_depthMapFilteredFloat.get(), W, H, m_stream), "copyFloatMap");
    }
    check(vh_convert_color_to_intensity_float(d_intensityMapFilteredFloat.get(), d_colorData.get(), W, H, m_stream), "convertColorToIntensityFloat");
    check(vh_convert_depth_float_to_camera_space_float4(d_cameraSpaceFloat4.get(), d_depthData.get(), &m_depthCameraParams, W, H, m_stream), "convertDepthFloatToCameraSpaceFloat4");
    check(vh_compute_normals(d_normalMapFloat4.get(), d_cameraSpaceFloat4.get(), W, H, m_stream), "computeNormals");
    // the source buffers are the caller's: they may be reused as soon as this returns
    checkHip(hipStreamSynchronize(s), "CUDARGBDSensor::process");
    m_frameNumber++;
}
