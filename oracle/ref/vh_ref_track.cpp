/*
 * vh_ref_track.cpp -- C ABI over the reference's two camera trackers' kernels, built for the CPU (oracle/ref/Makefile):
 * projectiveCorrespondences (CUDAImageHelper.cu), buildLinearSystem (CUDABuildLinearSystem.cu) and
 * computeNormalEquations (CUDABuildLinearSystemRGBD.cu), each through the reference's own launcher on host buffers.
 *
 * TEST INFRASTRUCTURE ONLY, like vh_ref_wrap.cpp, whose conventions hold here: the staged sources are compiled as host
 * C++ against the stand-ins in oracle/ref/include, kernels run through the launch emulator, and the reference's
 * functions are declared here by type only.
 *
 * THE BUILD KERNELS RUN WITH ONE THREAD PER BLOCK, AND WITH NOTHING ELSE.  Both end in a warp-synchronous tree
 * (warpReduce: six additions on volatile shared memory with no barrier between them), which an emulator that runs a
 * block's threads one after the other cannot execute as the hardware does.  With blockSizeInt = 1 thread 0 zeroes its
 * own 30 words of the static array, sums its window of pixels in order, and the tree then adds rows 32, 16, 8, 4, 2 and
 * 1 of that array -- rows that no launch has ever written, so they hold the zeros static storage starts with.  Output
 * row b is therefore lane b's in-order window sum exactly as the reference computes it (up to the sign of a zero).
 * That rests on one invariant: NO launch of these two kernels in this process ever uses a wider block.  So this file
 * offers no block size argument, and nothing else may call the two launchers.
 */
#include "cuda_runtime.h"
#include "cutil_math.h"
#include "cuda_SimpleMatrixUtil.h"
#include "DepthCameraUtil.h"
#include "CameraTrackingInput.h"

#include "../../include/vh_types.h"

extern "C" {
void updateConstantDepthCameraParams(const DepthCameraParams&);
void projectiveCorrespondences(float4*, float4*, float4*, float4*, float4*, float4*, float4*, float4*, unsigned int,
                               unsigned int, float, float, float, const float4x4*, const float4x4*, const DepthCameraData&);
void buildLinearSystem(unsigned int, unsigned int, float*, float4*, float4*, float4*, float*, unsigned int, unsigned int);
void computeNormalEquations(unsigned int, unsigned int, float*, CameraTrackingInput, float*, CameraTrackingParameters, float3,
                            float3, unsigned int, unsigned int);
}

static_assert(sizeof(DepthCameraParams) == sizeof(VhDepthCameraParams), "DepthCameraParams layout");
static_assert(sizeof(CameraTrackingParameters) == 7 * sizeof(float), "CameraTrackingParameters layout");

static float4* f4(const float* p) { return reinterpret_cast<float4*>(const_cast<float*>(p)); }

/* the one block size of the two build kernels in this process: see the head of the file */
static const unsigned int ONE_THREAD_PER_BLOCK = 1;

extern "C" {

/* projectiveCorrespondences.  transform: row-major 4x4, as the float4x4 the reference's host code hands over.  The
 * kernel reads its camera from c_depthCameraParams (and ignores its intrinsic argument and the colour maps). */
void vhr_icp_correspondences(const float* input, const float* inputNormals, const float* target, const float* targetNormals,
                             float* output, float* outputNormals, uint32_t w, uint32_t h, float distThres, float normalThres,
                             float levelFactor, const float transform[16], const VhDepthCameraParams* cp)
{
    DepthCameraParams p;
    memcpy(&p, cp, sizeof(p));
    updateConstantDepthCameraParams(p);
    const float4x4 t(transform);
    float4x4 intrinsic;
    intrinsic.setIdentity();
    DepthCameraData cam;
    projectiveCorrespondences(f4(input), f4(inputNormals), nullptr, f4(target), f4(targetNormals), nullptr, f4(output),
                              f4(outputNormals), w, h, distThres, normalThres, levelFactor, &t, &intrinsic, cam);
}

/* buildLinearSystem: out holds ceil(w h / window) rows of 30, row b = the in-order sum over pixels [b window,
 * (b + 1) window).  delta: the 16 floats the reference's host code passes, i.e. Eigen's column-major data() -- the
 * kernel reads them row-major and transposes. */
void vhr_icp_lane_sums(uint32_t w, uint32_t h, float* out, const float* input, const float* target,
                       const float* targetNormals, const float delta[16], uint32_t window)
{
    float d[16];
    memcpy(d, delta, sizeof(d));
    buildLinearSystem(w, h, out, f4(input), f4(target), f4(targetNormals), d, window, ONE_THREAD_PER_BLOCK);
}

/* computeNormalEquations, rows as above.  intrinsics: row-major 3x3 (what the host code's transposed Eigen matrix
 * holds); prm: weightDepth, weightColor, distThres, normalThres, sensorMaxDepth, colorGradiantMin, colorThres. */
void vhr_icp_rgbd_lane_sums(uint32_t w, uint32_t h, float* out, const float* inputPos, const float* inputNormal,
                            const float* inputIntensity, const float* targetPos, const float* targetNormal,
                            const float* targetIntensityAndDerivatives, const float intrinsics[9], const float prm[7],
                            const float angles[3], const float translation[3], uint32_t window)
{
    CameraTrackingInput in;
    in.d_inputPos = f4(inputPos);
    in.d_inputNormal = f4(inputNormal);
    in.d_inputIntensity = const_cast<float*>(inputIntensity);
    in.d_targetPos = f4(targetPos);
    in.d_targetNormal = f4(targetNormal);
    in.d_targetIntensityAndDerivatives = f4(targetIntensityAndDerivatives);
    CameraTrackingParameters p;
    p.weightDepth = prm[0];
    p.weightColor = prm[1];
    p.distThres = prm[2];
    p.normalThres = prm[3];
    p.sensorMaxDepth = prm[4];
    p.colorGradiantMin = prm[5];
    p.colorThres = prm[6];
    float k[9];
    memcpy(k, intrinsics, sizeof(k));
    computeNormalEquations(w, h, out, in, k, p, make_float3(angles[0], angles[1], angles[2]),
                           make_float3(translation[0], translation[1], translation[2]), window, ONE_THREAD_PER_BLOCK);
}

} /* extern "C" */
