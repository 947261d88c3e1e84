// vh_image.hip -- sensor pre-processing (DSC/CameraUtil.cu): the image kernels
// CUDARGBDAdapter::process and CUDARGBDSensor::process run between the sensor and integrate(), and the raw-frame ingest,
// with their launcher-level C ABI (include/vh_api.h).  One pixel per lane, rows contiguous across the wave (the reference
// uses 16x16 tiles); all of them stream the image once.  The host side is vh_sensor.cpp.
// MUST be compiled with -ffp-contract=off (see vh_device.hpp).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/vh_api.h"
#include "vh_device.hpp"
#include "vh_host_util.hpp"

using namespace vhd;

namespace {

// convertColorRawToFloatDevice :137-152 (RGBX bytes; black means "no colour")
VHD float4 color_raw_to_float4(uint32_t c)
{
    const uint32_t r = c & 0xffu, g = (c >> 8) & 0xffu, b = (c >> 16) & 0xffu, w = c >> 24;
    const float mi = minf();
    return (r == 0u && g == 0u && b == 0u) ? make_float4(mi, mi, mi, mi)
                                           : make_float4((float)r / 255.0f, (float)g / 255.0f, (float)b / 255.0f, (float)(w / 255u));
}
__global__ __launch_bounds__(256) void k_convert_color_raw_to_float4(float4* out, const uint32_t* in, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = color_raw_to_float4(in[i]);
}

// bilinearInterpolationFloat :1071-1098 (invalid taps drop out of the weights).  fetch(i) is source pixel i: a load, or a
// load and a conversion (k_ingest_frame)
template <class Fetch>
VHD float bilinear_float_taps(float x, float y, Fetch fetch, uint32_t W, uint32_t H)
{
    const int px = (int)floorf(x), py = (int)floorf(y);
    const float alpha = x - (float)px, beta = y - (float)py;
    const float mi = minf();
    float s0 = 0.0f, w0 = 0.0f, s1 = 0.0f, w1 = 0.0f;
    if ((uint32_t)px < W && (uint32_t)py < H) { const float v = fetch((uint32_t)py * W + (uint32_t)px); if (v != mi) { s0 += (1.0f - alpha) * v; w0 += (1.0f - alpha); } }
    if ((uint32_t)(px + 1) < W && (uint32_t)py < H) { const float v = fetch((uint32_t)py * W + (uint32_t)(px + 1)); if (v != mi) { s0 += alpha * v; w0 += alpha; } }
    if ((uint32_t)px < W && (uint32_t)(py + 1) < H) { const float v = fetch((uint32_t)(py + 1) * W + (uint32_t)px); if (v != mi) { s1 += (1.0f - alpha) * v; w1 += (1.0f - alpha); } }
    if ((uint32_t)(px + 1) < W && (uint32_t)(py + 1) < H) { const float v = fetch((uint32_t)(py + 1) * W + (uint32_t)(px + 1)); if (v != mi) { s1 += alpha * v; w1 += alpha; } }
    const float p0 = s0 / w0, p1 = s1 / w1;
    float ss = 0.0f, ww = 0.0f;
    if (w0 > 0.0f) { ss += (1.0f - beta) * p0; ww += (1.0f - beta); }
    if (w1 > 0.0f) { ss += beta * p1; ww += beta; }
    return ww > 0.0f ? ss / ww : mi;
}
VHD float bilinear_float(float x, float y, const float* in, uint32_t W, uint32_t H)
{
    return bilinear_float_taps(x, y, [in](uint32_t i) { return in[i]; }, W, H);
}

// resampleFloatMapDevice :1100-1118 / resampleFloat4MapDevice :1168-1186 (pixels whose nearest source pixel lies
// outside the source keep their old value, as in the reference)
// the source coordinates of output pixel (x, y); false: the nearest source pixel lies outside the source
VHD bool resample_coords(int x, int y, uint32_t inW, uint32_t inH, uint32_t outW, uint32_t outH, float& sx, float& sy)
{
    const float scaleWidth = (float)(inW - 1) / (float)(outW - 1), scaleHeight = (float)(inH - 1) / (float)(outH - 1);
    const uint32_t xInput = (uint32_t)((float)x * scaleWidth + 0.5f), yInput = (uint32_t)((float)y * scaleHeight + 0.5f);
    sx = (float)x * scaleWidth;
    sy = (float)y * scaleHeight;
    return xInput < inW && yInput < inH;
}
template <class T>
__global__ __launch_bounds__(256) void k_resample(T* out, const T* in, uint32_t inW, uint32_t inH, uint32_t outW, uint32_t outH)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= outW * outH) return;
    float sx, sy;
    if (resample_coords((int)(i % outW), (int)(i / outW), inW, inH, outW, outH, sx, sy)) {
        if constexpr (sizeof(T) == 4) out[i] = bilinear_float(sx, sy, in, inW, inH);
        else out[i] = bilinear_float4(sx, sy, in, inW, inH);
    }
}

// Not in the reference: a raw sensor frame -- 16-bit depth in units of 1/depthShift m, 8-bit RGB or RGBX colour, at the
// sensor's sizes -- to integrate's input at adapter size in one pass: SensorDataReader::processDepth's conversion
// (DSC/SensorDataReader.cpp:125-140: u16 / depthShift, a 0 sample stays 0.0f; RGB -> RGBX with X = 1),
// convertColorRawToFloat4, resampleFloatMap and resampleFloat4Map (or the colour copy when the colour size is the
// adapter's, DSC/CUDARGBDAdapter.cpp:107-131), with the conversions inside the tap fetch of the bilinear functions
// above: the same operations in the same order, so the same bits.  For widths and heights from 2 up the nearest
// source pixel is always inside the source (resample_coords), so every output pixel is written.
// The output (20 B per adapter pixel) is most of the traffic; the taps come from L2.  A workgroup owns 1024 consecutive
// output pixels: lane t writes depth pixels 4t..4t+3 as one 16-byte store and colour pixels t, t+256, t+512, t+768
// (a float4 each), so every store instruction of a wave covers one contiguous kilobyte.
constexpr uint32_t kIngestPixelsPerGroup = 1024;
template <int CH, bool COPY_COLOR>
__global__ __launch_bounds__(256) void k_ingest_frame(float* __restrict__ outDepth, float4* __restrict__ outColor, const uint16_t* __restrict__ depth,
                                                      const uint8_t* __restrict__ color, uint32_t depthW, uint32_t depthH, uint32_t colorW, uint32_t colorH,
                                                      uint32_t outW, uint32_t outH, float depthShift)
{
    const uint32_t n = outW * outH, base = blockIdx.x * kIngestPixelsPerGroup;
    auto depthTap = [depth, depthShift](uint32_t i) { return (float)depth[i] / depthShift; };
    auto depthAt = [&](uint32_t i) {
        float sx, sy;
        (void)resample_coords((int)(i % outW), (int)(i / outW), depthW, depthH, outW, outH, sx, sy);
        return bilinear_float_taps(sx, sy, depthTap, depthW, depthH);
    };
    const uint32_t i0 = base + 4u * threadIdx.x;
    if (i0 + 4u <= n) {
        *reinterpret_cast<float4*>(outDepth + i0) = make_float4(depthAt(i0), depthAt(i0 + 1u), depthAt(i0 + 2u), depthAt(i0 + 3u));
    } else {
        for (uint32_t i = i0; i < n; i++) outDepth[i] = depthAt(i);
    }
    if constexpr (CH != 0) {
        auto colorTap = [color](uint32_t i, uint32_t = 0u) {
            if constexpr (CH == 4) return color_raw_to_float4(reinterpret_cast<const uint32_t*>(color)[i]);
            else return color_raw_to_float4((uint32_t)color[3u * i] | ((uint32_t)color[3u * i + 1u] << 8) | ((uint32_t)color[3u * i + 2u] << 16) | (1u << 24));
        };
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t i = base + k * 256u + threadIdx.x;
            if (i >= n) break;
            if constexpr (COPY_COLOR) outColor[i] = colorTap(i);
            else {
                float sx, sy;
                (void)resample_coords((int)(i % outW), (int)(i / outW), colorW, colorH, outW, outH, sx, sy);
                outColor[i] = bilinear_float4_taps(sx, sy, colorTap, colorW, colorH);
            }
        }
    }
}

// setInvalidFloatMapDevice :338-346
__global__ __launch_bounds__(256) void k_set_invalid_float(float* out, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = minf();
}

// convertColorToIntensityFloatDevice :258-267
__global__ __launch_bounds__(256) void k_color_to_intensity(float* out, const float4* in, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 c = in[i];
    out[i] = 0.299f * c.x + 0.587f * c.y + 0.114f * c.z;
}

// convertDepthFloatToCameraSpaceFloat4Device :390-407
__global__ __launch_bounds__(256) void k_depth_to_camera_space(float4* out, const float* in, VhDepthCameraParams cp, uint32_t W, uint32_t H)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= W * H) return;
    const float mi = minf();
    const float depth = in[i];
    float4 o = make_float4(mi, mi, mi, mi);
    if (depth != mi) {
        const F3 p = depth_to_skeleton(cp, i % W, i / W, depth);
        o = make_float4(p.x, p.y, p.z, 1.0f);
    }
    out[i] = o;
}

// gaussD :436-439 (float exp), gaussR :426-429 (double arithmetic as written)
VHD float gauss_d(float sigma, int x, int y) { return expf(-((float)(x * x + y * y) / (2.0f * sigma * sigma))); }
/* gaussR (DSC/CameraUtil.cu:426-429) evaluates in double and returns float: the bilateral weight is a float product */
VHD float gauss_r(float sigma, float dist) { return (float)exp(-(double)(dist * dist) / (2.0 * (double)sigma * (double)sigma)); }

// gaussFilterFloatMapDevice :555-593
__global__ __launch_bounds__(256) void k_gauss_filter_float(float* out, const float* in, float sigmaD, float sigmaR, uint32_t W, uint32_t H)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= W * H) return;
    const int x = (int)(i % W), y = (int)(i / W);
    const int kernelRadius = (int)ceil(2.0 * (double)sigmaD);
    const float mi = minf();
    float sum = 0.0f, sumWeight = 0.0f;
    const float center = in[i];
    if (center != mi) {
        for (int m = x - kernelRadius; m <= x + kernelRadius; m++)
            for (int n = y - kernelRadius; n <= y + kernelRadius; n++)
                if (m >= 0 && n >= 0 && m < (int)W && n < (int)H) {
                    const float cur = in[(uint32_t)n * W + (uint32_t)m];
                    if (cur != mi && fabsf(center - cur) < sigmaR) {
                        const float weight = gauss_d(sigmaD, m - x, n - y);
                        sumWeight += weight;
                        sum += weight * cur;
                    }
                }
    }
    out[i] = sumWeight > 0.0f ? sum / sumWeight : mi;
}

// The same filter for radii up to kGaussMaxRadius with the neighbourhood and the weights in LDS: a workgroup owns a
// 32x8 tile of pixels, stages the tile plus its halo once and computes the (2r+1)^2 weights once instead of once per
// pixel (the expf is most of the per-pixel kernel's work).  Same taps in the same order, same weights: same sums.
constexpr int kGaussMaxRadius = 8, kGaussTileW = 32, kGaussTileH = 8;

__global__ __launch_bounds__(256) void k_gauss_filter_float_tiled(float* out, const float* in, float sigmaD, float sigmaR, int W, int H, int r)
{
    extern __shared__ float sGauss[];
    const int tw = kGaussTileW + 2 * r, th = kGaussTileH + 2 * r, side = 2 * r + 1;
    float* sTile = sGauss;              // tw x th, rows contiguous
    float* sWeight = sGauss + tw * th;  // side x side, [dx + r][dy + r]
    const int x0 = (int)blockIdx.x * kGaussTileW, y0 = (int)blockIdx.y * kGaussTileH;
    const float mi = minf();
    for (int i = (int)threadIdx.x; i < tw * th; i += 256) {
        const int gx = x0 - r + i % tw, gy = y0 - r + i / tw;
        sTile[i] = (gx >= 0 && gy >= 0 && gx < W && gy < H) ? in[(size_t)gy * W + gx] : mi; // outside the image: skipped like an invalid pixel
    }
    for (int i = (int)threadIdx.x; i < side * side; i += 256) sWeight[i] = gauss_d(sigmaD, i / side - r, i % side - r);
    __syncthreads();
    const int lx = (int)threadIdx.x % kGaussTileW, ly = (int)threadIdx.x / kGaussTileW;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= W || y >= H) return;
    float sum = 0.0f, sumWeight = 0.0f;
    const float center = sTile[(ly + r) * tw + lx + r];
    if (center != mi) {
        for (int dx = -r; dx <= r; dx++)      // m = x + dx outer, n = y + dy inner: the reference's order of summation
            for (int dy = -r; dy <= r; dy++) {
                const float cur = sTile[(ly + r + dy) * tw + lx + r + dx];
                // a tap outside the image holds MINF here; the reference skips it by its bounds test
                if (cur != mi && fabsf(center - cur) < sigmaR) {
                    const float weight = sWeight[(dx + r) * side + dy + r];
                    sumWeight += weight;
                    sum += weight * cur;
                }
            }
    }
    out[(size_t)y * W + x] = sumWeight > 0.0f ? sum / sumWeight : mi;
}

// gaussFilterFloat4MapDevice :611-651
__global__ __launch_bounds__(256) void k_gauss_filter_float4(float4* out, const float4* in, float sigmaD, float sigmaR, uint32_t W, uint32_t H)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= W * H) return;
    const int x = (int)(i % W), y = (int)(i / W);
    const int kernelRadius = (int)ceil(2.0 * (double)sigmaD);
    const float mi = minf();
    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
    float sumWeight = 0.0f;
    const float4 center = in[i];
    if (center.x != mi) {
        for (int m = x - kernelRadius; m <= x + kernelRadius; m++)
            for (int n = y - kernelRadius; n <= y + kernelRadius; n++)
                if (m >= 0 && n >= 0 && m < (int)W && n < (int)H) {
                    const float4 cur = in[(uint32_t)n * W + (uint32_t)m];
                    if (cur.x != mi) {
                        const float dx = center.x - cur.x, dy = center.y - cur.y, dz = center.z - cur.z, dw = center.w - cur.w;
                        if (sqrtf(dx * dx + dy * dy + dz * dz + dw * dw) < sigmaR) { // length(float4), cutil_math.h
                            const float weight = gauss_d(sigmaD, m - x, n - y);
                            sumWeight += weight;
                            sum = f4_add(sum, f4_scale(weight, cur));
                        }
                    }
                }
    }
    out[i] = sumWeight > 0.0f ? f4_div(sum, sumWeight) : make_float4(mi, mi, mi, mi);
}

// bilateralFilterFloatMapDevice :446-483
__global__ __launch_bounds__(256) void k_bilateral_filter_float(float* out, const float* in, float sigmaD, float sigmaR, uint32_t W, uint32_t H)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= W * H) return;
    const int x = (int)(i % W), y = (int)(i / W);
    const int kernelRadius = (int)ceil(2.0 * (double)sigmaD);
    const float mi = minf();
    float sum = 0.0f, sumWeight = 0.0f;
    const float center = in[i];
    float o = mi;
    if (center != mi) {
        for (int m = x - kernelRadius; m <= x + kernelRadius; m++)
            for (int n = y - kernelRadius; n <= y + kernelRadius; n++)
                if (m >= 0 && n >= 0 && m < (int)W && n < (int)H) {
                    const float cur = in[(uint32_t)n * W + (uint32_t)m];
                    if (cur != mi) {
                        const float weight = gauss_d(sigmaD, m - x, n - y) * gauss_r(sigmaR, cur - center);
                        sumWeight += weight;
                        sum += weight * cur;
                    }
                }
        if (sumWeight > 0.0f) o = sum / sumWeight;
    }
    out[i] = o;
}

// erodeDepthMapDevice :1632-1670
__global__ __launch_bounds__(256) void k_erode_depth(float* out, const float* in, int structureSize, int W, int H, float dThresh, float fracReq)
{
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (uint32_t)(W * H)) return;
    const int x = (int)(idx % (uint32_t)W), y = (int)(idx / (uint32_t)W);
    const float mi = minf();
    uint32_t count = 0;
    const float oldDepth = in[idx];
    for (int i = -structureSize; i <= structureSize; i++)
        for (int j = -structureSize; j <= structureSize; j++)
            if (x + j >= 0 && x + j < W && y + i >= 0 && y + i < H) {
                const float depth = in[(y + i) * W + (x + j)];
                if (depth == mi || depth == 0.0f || fabsf(depth - oldDepth) > dThresh) count++;
            }
    const uint32_t sum = (uint32_t)((2 * structureSize + 1) * (2 * structureSize + 1));
    out[idx] = ((float)count / (float)sum >= fracReq) ? mi : oldDepth;
}

} // namespace

extern "C" {

#define VH_IMG_LAUNCH(n) cdiv((uint32_t)(n), 256u), 256, 0, (hipStream_t)stream

int vh_convert_color_raw_to_float4(float* d_output4, const uint8_t* d_inputRGBX, uint32_t width, uint32_t height, vhStream_t stream)
{
    if (!d_output4 || !d_inputRGBX) return VH_ERR_BAD_ARGUMENT;
    if (width * height == 0) return VH_OK;
    k_convert_color_raw_to_float4<<<VH_IMG_LAUNCH(width * height)>>>(reinterpret_cast<float4*>(d_output4), reinterpret_cast<const uint32_t*>(d_inputRGBX), width * height);
    return vh_last_launch_error();
}

int vh_ingest_frame(float* d_depth, float* d_color4, uint32_t width, uint32_t height, const uint16_t* d_depthRaw, uint32_t depthWidth, uint32_t depthHeight,
                    const uint8_t* d_colorRaw, uint32_t colorWidth, uint32_t colorHeight, uint32_t colorChannels, float depthShift, vhStream_t stream)
{
    if (!d_depth || !d_depthRaw || width < 2 || height < 2 || depthWidth < 2 || depthHeight < 2) return VH_ERR_BAD_ARGUMENT;
    if (!(depthShift > 0.0f) || !std::isfinite(depthShift)) return VH_ERR_BAD_ARGUMENT;
    if (colorChannels != 0 && colorChannels != 3 && colorChannels != 4) return VH_ERR_BAD_ARGUMENT;
    if (colorChannels != 0 && (!d_color4 || !d_colorRaw || colorWidth < 2 || colorHeight < 2)) return VH_ERR_BAD_ARGUMENT;
    // 16-byte stores; the 32-bit pixel index of the other image kernels
    if (((uintptr_t)d_depth | (uintptr_t)d_color4) % 16u || (uintptr_t)d_depthRaw % 2u || (colorChannels == 4 && (uintptr_t)d_colorRaw % 4u)) return VH_ERR_BAD_ARGUMENT;
    if ((uint64_t)width * height > 0x7fffffffull || (uint64_t)depthWidth * depthHeight > 0x7fffffffull || (uint64_t)colorWidth * colorHeight * 4ull > 0x7fffffffull) return VH_ERR_BAD_ARGUMENT;
    const bool copyColor = colorWidth == width && colorHeight == height;
    const uint32_t groups = cdiv(width * height, kIngestPixelsPerGroup);
    float4* c4 = reinterpret_cast<float4*>(d_color4);
#define VH_INGEST(CH, COPY) k_ingest_frame<CH, COPY><<<groups, 256, 0, (hipStream_t)stream>>>(d_depth, c4, d_depthRaw, d_colorRaw, depthWidth, depthHeight, colorWidth, colorHeight, width, height, depthShift)
    if (colorChannels == 0) VH_INGEST(0, false);
    else if (colorChannels == 3) { if (copyColor) VH_INGEST(3, true); else VH_INGEST(3, false); }
    else { if (copyColor) VH_INGEST(4, true); else VH_INGEST(4, false); }
#undef VH_INGEST
    return vh_last_launch_error();
}

int vh_resample_float_map(float* d_output, uint32_t outputWidth, uint32_t outputHeight, const float* d_input, uint32_t inputWidth, uint32_t inputHeight, vhStream_t stream)
{
    if (!d_output || !d_input || inputWidth == 0 || inputHeight == 0) return VH_ERR_BAD_ARGUMENT;
    if (outputWidth * outputHeight == 0) return VH_OK;
    k_resample<float><<<VH_IMG_LAUNCH(outputWidth * outputHeight)>>>(d_output, d_input, inputWidth, inputHeight, outputWidth, outputHeight);
    return vh_last_launch_error();
}
int vh_resample_float4_map(float* d_output4, uint32_t outputWidth, uint32_t outputHeight, const float* d_input4, uint32_t inputWidth, uint32_t inputHeight, vhStream_t stream)
{
    if (!d_output4 || !d_input4 || inputWidth == 0 || inputHeight == 0) return VH_ERR_BAD_ARGUMENT;
    if (outputWidth * outputHeight == 0) return VH_OK;
    k_resample<float4><<<VH_IMG_LAUNCH(outputWidth * outputHeight)>>>(reinterpret_cast<float4*>(d_output4), reinterpret_cast<const float4*>(d_input4), inputWidth, inputHeight, outputWidth, outputHeight);
    return vh_last_launch_error();
}
int vh_copy_float_map(float* d_output, const float* d_input, uint32_t width, uint32_t height, vhStream_t stream)
{
    if (!d_output || !d_input) return VH_ERR_BAD_ARGUMENT;
    VH_HIP(hipMemcpyAsync(d_output, d_input, sizeof(float) * (size_t)width * height, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return VH_OK;
}
int vh_copy_float4_map(float* d_output4, const float* d_input4, uint32_t width, uint32_t height, vhStream_t stream)
{
    if (!d_output4 || !d_input4) return VH_ERR_BAD_ARGUMENT;
    VH_HIP(hipMemcpyAsync(d_output4, d_input4, sizeof(float) * 4 * (size_t)width * height, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return VH_OK;
}
int vh_set_invalid_float_map(float* d_output, uint32_t width, uint32_t height, vhStream_t stream)
{
    if (!d_output) return VH_ERR_BAD_ARGUMENT;
    if (width * height == 0) return VH_OK;
    k_set_invalid_float<<<VH_IMG_LAUNCH(width * height)>>>(d_output, width * height);
    return vh_last_launch_error();
}
int vh_convert_color_to_intensity_float(float* d_output, const float* d_input4, uint32_t width, uint32_t height, vhStream_t stream)
{
    if (!d_output || !d_input4) return VH_ERR_BAD_ARGUMENT;
    if (width * height == 0) return VH_OK;
    k_color_to_intensity<<<VH_IMG_LAUNCH(width * height)>>>(d_output, reinterpret_cast<const float4*>(d_input4), width * height);
    return vh_last_launch_error();
}
int vh_convert_depth_float_to_camera_space_float4(float* d_output4, const float* d_input, const VhDepthCameraParams* cp, uint32_t width, uint32_t height, vhStream_t stream)
{
    if (!d_output4 || !d_input || !cp) return VH_ERR_BAD_ARGUMENT;
    if (width * height == 0) return VH_OK;
    k_depth_to_camera_space<<<VH_IMG_LAUNCH(width * height)>>>(reinterpret_cast<float4*>(d_output4), d_input, *cp, width, height);
    return vh_last_launch_error();
}
int vh_gauss_filter_float_map(float* d_output, const float* d_input, float sigmaD, float sigmaR, uint32_t width, uint32_t height, vhStream_t stream)
{
    if (!d_output || !d_input || d_output == d_input) return VH_ERR_BAD_ARGUMENT;
    if (width * height == 0) return VH_OK;
    const int r = (int)ceil(2.0 * (double)sigmaD);
    if (r >= 0 && r <= kGaussMaxRadius) {
        const size_t lds = sizeof(float) * ((size_t)(kGaussTileW + 2 * r) * (kGaussTileH + 2 * r) + (size_t)(2 * r + 1) * (2 * r + 1));
        const dim3 grid(cdiv(width, (uint32_t)kGaussTileW), cdiv(height, (uint32_t)kGaussTileH));
        k_gauss_filter_float_tiled<<<grid, 256, lds, (hipStream_t)stream>>>(d_output, d_input, sigmaD, sigmaR, (int)width, (int)height, r);
    } else {
        k_gauss_filter_float<<<VH_IMG_LAUNCH(width * height)>>>(d_output, d_input, sigmaD, sigmaR, width, height);
    }
    return vh_last_launch_error();
}
int vh_gauss_filter_float4_map(float* d_output4, const float* d_input4, float sigmaD, float sigmaR, uint32_t width, uint32_t height, vhStream_t stream)
{
    if (!d_output4 || !d_input4 || d_output4 == d_input4) return VH_ERR_BAD_ARGUMENT;
    if (width * height == 0) return VH_OK;
    k_gauss_filter_float4<<<VH_IMG_LAUNCH(width * height)>>>(reinterpret_cast<float4*>(d_output4), reinterpret_cast<const float4*>(d_input4), sigmaD, sigmaR, width, height);
    return vh_last_launch_error();
}
int vh_bilateral_filter_float_map(float* d_output, const float* d_input, float sigmaD, float sigmaR, uint32_t width, uint32_t height, vhStream_t stream)
{
    if (!d_output || !d_input || d_output == d_input) return VH_ERR_BAD_ARGUMENT;
    if (width * height == 0) return VH_OK;
    k_bilateral_filter_float<<<VH_IMG_LAUNCH(width * height)>>>(d_output, d_input, sigmaD, sigmaR, width, height);
    return vh_last_launch_error();
}
int vh_erode_depth_map(float* d_output, const float* d_input, int32_t structureSize, uint32_t width, uint32_t height, float dThresh, float fracReq, vhStream_t stream)
{
    if (!d_output || !d_input || d_output == d_input || structureSize < 0) return VH_ERR_BAD_ARGUMENT;
    if (width * height == 0) return VH_OK;
    k_erode_depth<<<VH_IMG_LAUNCH(width * height)>>>(d_output, d_input, structureSize, (int)width, (int)height, dThresh, fracReq);
    return vh_last_launch_error();
}
#undef VH_IMG_LAUNCH

} // extern "C"
