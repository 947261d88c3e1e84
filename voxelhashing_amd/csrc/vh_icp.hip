// vh_icp.hip -- the two camera trackers (projective ICP and RGB-D ICP) and their launcher-level C ABI
// (include/vh_api.h).  Nothing here touches the hash, the riders or the ray caster.
//
// MUST be compiled with -ffp-contract=off (see vh_device.hpp): the fused step kernels and the unfused ones share their
// per-pixel arithmetic through inlined device functions, so the source expressions fix every bit of the result.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/vh_api.h"
#include "vh_device.hpp"
#include "vh_host_util.hpp"
#include "vh_solve_6x6.hpp"

using namespace vhd;

namespace {

// ---------------------------------------------------------------------------
// projective ICP camera tracking: projectiveCorrespondencesKernel (DSC/CUDAImageHelper.cu:70-125),
// scanScanElementsCS + reductionSystemCPU (DSC/CUDABuildLinearSystem.cu:130-188, .cpp:52-92) and the 6x6 solve /
// delinearisation the reference does on the host with Eigen (DSC/CUDACameraTrackingMultiRes.cpp:186-253).
//
// The reference copies every linear system to the host, solves it there and uploads the next transform: up to 18
// blocking round trips per frame.  Here the transform, the residual history and the lost / early-out flags live in
// a VhIcpState on the device; every step is a kernel on the stream that reads and updates it, a step whose level has
// finished returns at once, and the host reads the result once per frame.
// ---------------------------------------------------------------------------

constexpr uint32_t kIcpWindow = 12;   // pixels a lane sums before the wave reduces (localWindowSize, .cpp:41)
constexpr uint32_t kIcpTerms = 30;    // 21 upper-triangle terms of A^T A, 6 of A^T b, residual, weight, count (ARRAY_SIZE)

__global__ void k_icp_begin(VhIcpState* st, const float* d_deltaEstimate)
{
    const uint32_t t = threadIdx.x;
    if (t < 16u) st->delta[t] = d_deltaEstimate[t];
    if (t == 0u) { st->lost = 0u; st->done = 0u; st->lastError = -1.0f; st->iterations = 0u; st->sumRegError = 0.0f; st->sumRegWeight = 0.0f; st->numCorr = 0u; st->matrixCondition = 0.0f; }
}

__global__ void k_icp_begin_level(VhIcpState* st)
{
    if (threadIdx.x == 0u) { st->done = 0u; st->lastError = -1.0f; }
}

// The moving pixel of projectiveCorrespondencesKernel :70-125: the input point and normal under the delta D, and the
// model pixel the point lands on (getBestCorrespondence1x1 = that pixel itself).  False: no input, or off the image.
VHD bool icp_project(const float* D, float4 p, float4 n, const VhDepthCameraParams& cp, float levelFactor, uint32_t W, uint32_t H, F3& pt, F3& nt, uint32_t& at)
{
    if (p.x == minf() || n.x == minf()) return false;
    pt = mat_mul_p(D, mk3(p.x, p.y, p.z));
    nt = mat_mul_d(D, mk3(n.x, n.y, n.z));
    // cameraToKinectScreenInt, DSC/DepthCameraUtil.h:74-85, then the division by the level factor (both truncate)
    int sx = f2i((pt.x * cp.fx / pt.z + cp.mx) + 0.5f), sy = f2i((pt.y * cp.fy / pt.z + cp.my) + 0.5f);
    sx = f2i((float)sx / levelFactor); sy = f2i((float)sy / levelFactor);
    if (!(sx >= 0 && sy >= 0 && sx < (int)W && sy < (int)H)) return false;
    at = (uint32_t)sy * W + (uint32_t)sx;
    return true;
}

// The pair test of :70-125 on the model point tp and normal tn, and the weight of a pair that passes
VHD bool icp_pair(F3 pt, F3 nt, float4 tp, float4 tn, float distThres, float normalThres, const VhDepthCameraParams& cp, float& weight)
{
    if (tp.x == minf() || tn.x == minf()) return false;
    const float dx = pt.x - tp.x, dy = pt.y - tp.y, dz = pt.z - tp.z;
    const float d = sqrtf(dx * dx + dy * dy + dz * dz);
    const float dNormal = nt.x * tn.x + nt.y * tn.y + nt.z * tn.z;
    if (!(d <= distThres && dNormal >= normalThres)) return false;
    weight = fmaxf(0.0f, 0.5f * ((1.0f - d / distThres) + (1.0f - cam_to_proj_z(cp, pt.z))));
    return true;
}

// One pair into a lane's 30 terms: buildRowSystemMatrixPlane :70-82, buildRowRHSPlane :85-88 of the moving point q,
// the model point pT and its normal n; residual, weight and count behind them
VHD void icp_add_pair(float (&acc)[kIcpTerms], F3 q, F3 pT, F3 n, float weight)
{
    const float row[6] = { n.x * q.y - n.y * q.x, n.z * q.x - n.x * q.z, n.y * q.z - n.z * q.y, -n.x, -n.y, -n.z };
    const float b = n.x * (q.x - pT.x) + n.y * (q.y - pT.y) + n.z * (q.z - pT.z);
    uint32_t at = 0;
#pragma unroll
    for (uint32_t r = 0; r < 6u; r++) {
#pragma unroll
        for (uint32_t c = r; c < 6u; c++) acc[at + c - r] += weight * row[r] * row[c];
        at += 6u - r;
        acc[21u + r] += weight * row[r] * b;
    }
    const float dN = (pT.x - q.x) * n.x + (pT.y - q.y) * n.y + (pT.z - q.z) * n.z;
    acc[27] += weight * dN * dN;
    acc[28] += weight;
    acc[29] += 1.0f;
}

// The 64 lanes' terms into lane 0 by the reference's tree (+32, +16, ... +1; scanScanElementsCS :130-188, warpReduce)
VHD void icp_wave_sum(float (&acc)[kIcpTerms], uint32_t lane)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (uint32_t k = 0; k < kIcpTerms; k++) {
            const float other = __shfl_down(acc[k], off);
            if ((int)lane < off) acc[k] += other;
        }
    }
}

// The wave's 30 terms (lane 0 holds them) to its row of `partials`.  A workgroup is one wave.
VHD void icp_store_partials(float* partials, const float (&acc)[kIcpTerms])
{
#pragma unroll
    for (uint32_t k = 0; k < kIcpTerms; k++) partials[(size_t)blockIdx.x * kIcpTerms + k] = acc[k];
}

// projectiveCorrespondencesKernel :70-125
__global__ __launch_bounds__(256) void k_icp_correspondences(const float4* input, const float4* inputNormals, const float4* target, const float4* targetNormals,
                                                             float4* outCorr, float4* outCorrNormals, uint32_t W, uint32_t H, float distThres,
                                                             float normalThres, float levelFactor, const VhIcpState* st, VhDepthCameraParams cp)
{
    if (st->lost || st->done) return;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= W * H) return;
    const float mi = minf();
    float4 oc = make_float4(mi, mi, mi, mi), on = oc;
    F3 pt, nt;
    uint32_t at;
    if (icp_project(st->delta, input[i], inputNormals[i], cp, levelFactor, W, H, pt, nt, at)) {
        const float4 tp = target[at];
        float4 tn = targetNormals[at];
        if (icp_pair(pt, nt, tp, tn, distThres, normalThres, cp, tn.w)) { // (the weight travels in the normal's w)
            oc = tp;
            on = tn;
        }
    }
    outCorr[i] = oc;
    outCorrNormals[i] = on;
}

// scanScanElementsCS :130-188: lane x sums pixels [12x, 12x+12) in order, the wave is reduced and lane 0 writes its 30 terms
__global__ __launch_bounds__(64) void k_icp_build_system(uint32_t W, uint32_t H, float* partials, const float4* input, const float4* corr,
                                                         const float4* corrNormals, const VhIcpState* st)
{
    if (st->lost || st->done) return;
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    const float mi = minf();
    float acc[kIcpTerms];
#pragma unroll
    for (uint32_t k = 0; k < kIcpTerms; k++) acc[k] = 0.0f;
    for (uint32_t w = 0; w < kIcpWindow; w++) {
        const uint32_t idx = kIcpWindow * x + w;
        if (idx % W < W && idx / W < H) {
            const float4 tp = corr[idx], ip = input[idx], tn = corrNormals[idx];
            if (tp.x != mi && ip.x != mi && tn.x != mi)
                icp_add_pair(acc, mat_mul_p(st->delta, mk3(ip.x, ip.y, ip.z)), mk3(tp.x, tp.y, tp.z), mk3(tn.x, tn.y, tn.z), tn.w);
        }
    }
    const uint32_t lane = lane_id();
    icp_wave_sum(acc, lane);
    if (lane == 0u) icp_store_partials(partials, acc);
}

// reductionSystemCPU (.cpp:52-92) for term t: the wave partials summed in their order; eight loads in flight
VHD float icp_sum_term(const float* partials, uint32_t nPartials, uint32_t t)
{
    float sum = 0.0f;
    uint32_t k = 0;
    for (; k + 8u <= nPartials; k += 8u) {
        float v[8];
#pragma unroll
        for (uint32_t j = 0; j < 8u; j++) v[j] = partials[(size_t)(k + j) * kIcpTerms + t];
#pragma unroll
        for (uint32_t j = 0; j < 8u; j++) sum += v[j];
    }
    for (; k < nPartials; k++) sum += partials[(size_t)k * kIcpTerms + t];
    return sum;
}

// All 30 terms into shared memory, one term per lane, for the lane that solves.  The whole workgroup (one wave) calls it.
VHD void icp_sum_terms(const float* partials, uint32_t nPartials, uint32_t lane, float (&sTerms)[kIcpTerms])
{
    if (lane < kIcpTerms) sTerms[lane] = icp_sum_term(partials, nPartials, lane);
    __syncthreads();
}

// The end of a fused step's wave (a workgroup is ONE wave): its reduced terms (lane 0 holds them) go to `partials`, and the
// wave that draws the last ticket gets every wave's terms summed in `sTerms` and true; the others get false and are done.
//
// The hand-off crosses XCDs, whose L2s are not coherent with one another.  Lane 0 stores the partials with plain stores
// and waits until they have left the wave (vmcnt(0)); the agent-scope release fence writes them back to where every XCD
// sees them; only then is the ticket drawn, a relaxed agent-scope add.  So a wave that reads ticket value n knows that
// the partials of the n waves before it are visible at agent scope, and the one that reads gridDim.x - 1 knows it of all:
// it takes an agent-scope acquire (dropping its own stale lines) before its plain loads.  The ticket is broadcast with a
// shuffle, and no wave waits for another.  Every wave has read what it needs of the state before it draws its ticket, and
// only the last arriver's caller writes the state, after all tickets are drawn.  *ticket is 0 when the launch starts (the
// caller clears it on the stream where it begins the solve) and the last arriver leaves it 0 for the next launch.
VHD bool icp_hand_off(float* partials, uint32_t* ticket, const float (&acc)[kIcpTerms], uint32_t lane, float (&sTerms)[kIcpTerms])
{
    uint32_t drawn = 0u;
    if (lane == 0u) {
        icp_store_partials(partials, acc);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    drawn = (uint32_t)__shfl((int)drawn, 0);
    if (drawn != gridDim.x - 1u) return false;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0u) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    icp_sum_terms(partials, gridDim.x, lane, sTerms);
    return true;
}

// The 30 summed terms -> A (both triangles), b; false when ATA.isZero(): Eigen's DenseBase::isZero with the default
// dummy_precision of float (Core/CwiseNullaryOp.h:482-489, Core/MathFunctions.h:653-657, Core/NumTraits.h:94), i.e.
// |a_ij| <= 1e-5f for every entry.  A NaN entry is not "zero" (the comparison is false): the solve goes on and the
// rigidity check rejects the NaN step.
VHD bool icp_system_from_terms(const float* terms, double (&A)[6][6], double (&b)[6])
{
    uint32_t at = 0;
    bool zero = true;
    for (uint32_t r = 0; r < 6u; r++) {
        for (uint32_t c = r; c < 6u; c++) {
            A[r][c] = A[c][r] = (double)terms[at + c - r];
            if (!(fabsf(terms[at + c - r]) <= 1e-5f)) zero = false;
        }
        at += 6u - r;
        b[r] = (double)terms[21u + r];
    }
    return !zero;
}

// What computeBestRigidAlignment, delinearizeTransformation and align do with the summed system on the host
// (DSC/CUDACameraTrackingMultiRes.cpp:186-253, 306-318), the solve by icp_solve_6x6.  One lane; `terms` are the 30 sums.
VHD void icp_solve_step(VhIcpState* st, const float* terms, float angleThres, float distThres, float earlyOut, uint32_t lastInner)
{
    double A[6][6], b[6];
    {
        const bool nonzero = icp_system_from_terms(terms, A, b);
        st->sumRegError = terms[27];
        st->sumRegWeight = terms[28];
        st->numCorr = (uint32_t)terms[29];
        st->iterations += 1u;
        if (!nonzero) { st->lost = 1u; return; } // ATA.isZero(): every |a_ij| <= 1e-5
    }
    double xs[6];
    st->matrixCondition = icp_solve_6x6(A, b, xs);
    // delinearizeTransformation :186-207: R = Rz(x0) Ry(x1) Rx(x2), t = x[3..5]; mean 0, meanStDev 1
    const float x0 = (float)xs[0], x1 = (float)xs[1], x2 = (float)xs[2];
    const float tx = (float)xs[3], ty = (float)xs[4], tz = (float)xs[5];
    const float cz = cosf(x0), sz = sinf(x0), cy = cosf(x1), sy = sinf(x1), cx = cosf(x2), sx = sinf(x2);
    float R[9] = { cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx,
                   sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx,
                   -sy, cy * sx, cy * cx };
    // checkRigidTransformation :176-185: angle of the rotation (Eigen::AngleAxisf) and length of the translation
    const float trace = R[0] + R[4] + R[8];
    const float angle = acosf(fminf(1.0f, fmaxf(-1.0f, 0.5f * (trace - 1.0f))));
    const float tnorm = sqrtf(tx * tx + ty * ty + tz * tz);
    if (!(angle <= angleThres) || !(tnorm <= distThres)) { st->lost = 1u; return; }
    // deltaTransform = t * deltaTransform
    float M[16] = { R[0], R[1], R[2], tx, R[3], R[4], R[5], ty, R[6], R[7], R[8], tz, 0.0f, 0.0f, 0.0f, 1.0f };
    float D[16];
    for (int k = 0; k < 16; k++) D[k] = st->delta[k];
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            float acc = 0.0f;
            for (int k = 0; k < 4; k++) acc += M[4 * r + k] * D[4 * k + c];
            st->delta[4 * r + c] = acc;
        }
    // align :306-318, after the last inner iteration: leave the level when the residual stops changing
    if (lastInner) {
        if (fabsf(st->lastError - st->sumRegError) < earlyOut) st->done = 1u;
        st->lastError = st->sumRegError;
    }
}

// One wave: reductionSystemCPU (.cpp:52-92) over the wave partials in their order, then icp_solve_step.
__global__ __launch_bounds__(64) void k_icp_solve(VhIcpState* st, const float* partials, uint32_t nPartials, float angleThres, float distThres, float earlyOut, uint32_t lastInner)
{
    __shared__ float sTerms[kIcpTerms];
    if (st->lost || st->done) return;
    icp_sum_terms(partials, nPartials, threadIdx.x, sTerms);
    if (threadIdx.x == 0u) icp_solve_step(st, sTerms, angleThres, distThres, earlyOut, lastInner);
}

// The state's result into mapped host memory, the tag last (system-scope release: the host polls the tag and then reads
// the words before it; the idiom of k_publish_words).  One lane.
VHD void icp_publish(const VhIcpState* __restrict__ st, VhIcpResult* __restrict__ out, uint32_t tag)
{
    const VhIcpState s = *st; // (all loads in flight before the first store)
#pragma unroll
    for (int k = 0; k < 16; k++) out->delta[k] = s.delta[k];
    out->lost = s.lost;
    out->sumRegError = s.sumRegError;
    out->sumRegWeight = s.sumRegWeight;
    out->numCorr = s.numCorr;
    out->matrixCondition = s.matrixCondition;
    out->iterations = s.iterations;
    __atomic_thread_fence(__ATOMIC_RELEASE);
    __hip_atomic_store(&out->tag, tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ void k_icp_publish(const VhIcpState* st, VhIcpResult* out, uint32_t tag)
{
    if (blockIdx.x == 0u && threadIdx.x == 0u) icp_publish(st, out, tag);
}

// One outer iteration of a level whose s_maxInnerIter is 1, in one launch: k_icp_correspondences, k_icp_build_system and
// k_icp_solve.  A wave owns the 768 pixels k_icp_build_system gives it; for each it makes the pair with the functions
// k_icp_correspondences calls and adds it to the 30 running sums in the same order, so the correspondence maps are never
// written and the VhIcpState after the launch is the three kernels' bit for bit.  icp_hand_off gives the step to the
// wave that finishes last.
// publish (may be null): mapped host memory that receives the state after this step, under `tag`.  A step that is
// skipped (lost / done) changes nothing, so its first wave publishes the state as it stands.
__global__ __launch_bounds__(64) void k_icp_step(const float4* input, const float4* inputNormals, const float4* target, const float4* targetNormals,
                                                 uint32_t W, uint32_t H, float pairDistThres, float normalThres, float levelFactor, VhDepthCameraParams cp,
                                                 float* partials, uint32_t* ticket, VhIcpState* st, float angleThres, float distThres, float earlyOut,
                                                 VhIcpResult* publish, uint32_t tag)
{
    __shared__ float sTerms[kIcpTerms];
    const uint32_t lane = threadIdx.x;
    const uint32_t skip = st->lost | st->done;
    float D[16];
#pragma unroll
    for (int k = 0; k < 16; k++) D[k] = st->delta[k];
    if (skip) {
        if (publish && blockIdx.x == 0u && lane == 0u) icp_publish(st, publish, tag);
        return;
    }
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, nPixels = W * H;
    float acc[kIcpTerms];
#pragma unroll
    for (uint32_t k = 0; k < kIcpTerms; k++) acc[k] = 0.0f;
    // Six pixels at a time: their input loads go out together, then their model loads (a lane that took its 12 pixels one
    // after the other would wait for 24 dependent round trips); the sums take the pixels in their order all the same.
    constexpr uint32_t kBatch = 6u;
    for (uint32_t w0 = 0; w0 < kIcpWindow; w0 += kBatch) {
        float4 p[kBatch], n[kBatch], tp[kBatch], tn[kBatch];
        F3 pt[kBatch], nt[kBatch];
        bool ok[kBatch];
        uint32_t at[kBatch];
#pragma unroll
        for (uint32_t j = 0; j < kBatch; j++) {
            const uint32_t idx = kIcpWindow * x + w0 + j;
            ok[j] = idx < nPixels;
            at[j] = ok[j] ? idx : 0u; // (a pixel past the end reads pixel 0 and is dropped)
            p[j] = input[at[j]];
            n[j] = inputNormals[at[j]];
        }
#pragma unroll
        for (uint32_t j = 0; j < kBatch; j++) {
            at[j] = 0u;
            pt[j] = nt[j] = mk3(0.0f, 0.0f, 0.0f);
            ok[j] = ok[j] && icp_project(D, p[j], n[j], cp, levelFactor, W, H, pt[j], nt[j], at[j]);
        }
#pragma unroll
        for (uint32_t j = 0; j < kBatch; j++) { // (a pixel without a pair reads pixel 0 and is dropped)
            tp[j] = target[at[j]];
            tn[j] = targetNormals[at[j]];
        }
#pragma unroll
        for (uint32_t j = 0; j < kBatch; j++) {
            float weight;
            if (ok[j] && icp_pair(pt[j], nt[j], tp[j], tn[j], pairDistThres, normalThres, cp, weight)) // (the moving point is pt: the same product)
                icp_add_pair(acc, pt[j], mk3(tp[j].x, tp[j].y, tp[j].z), mk3(tn[j].x, tn[j].y, tn[j].z), weight);
        }
    }
    icp_wave_sum(acc, lane);
    if (!icp_hand_off(partials, ticket, acc, lane, sTerms) || lane != 0u) return;
    icp_solve_step(st, sTerms, angleThres, distThres, earlyOut, 1u);
    if (publish) icp_publish(st, publish, tag);
}

// ---------------------------------------------------------------------------
// RGB-D camera tracking: CUDACameraTrackingMultiResRGBD (DSC/CUDACameraTrackingMultiResRGBD.cpp) with
// scanNormalEquationsDevice (DSC/CUDABuildLinearSystemRGBD.cu:106-201).  One fused kernel per iteration projects the
// input pixels, looks the model up and sums a point-to-plane row and a photometric row; one wave then solves the
// system, takes the Gauss-Newton step in Euler angles and leaves the next linearisation point in the VhIcpStateRGBD.
// Like f5, the whole multi-level solve runs on the stream and the host reads the state once per frame.
// ---------------------------------------------------------------------------

// computeIntensityAndDerivativesDevice, DSC/CameraUtil.cu:1492-1529: (I, dI/du, dI/dv, 1) by the 3x3 Sobel stencil / 8;
// MINF on the border and wherever one of the nine taps is MINF.  Only exact products and one exact division: the
// result is the same bits as the reference's arithmetic in float.
__global__ __launch_bounds__(256) void k_intensity_and_derivatives(float4* out, const float* in, uint32_t W, uint32_t H)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= W * H) return;
    const uint32_t x = i % W, y = i / W;
    const float mi = minf();
    float4 o = make_float4(mi, mi, mi, mi);
    if (x > 0u && x + 1u < W && y > 0u && y + 1u < H) {
        float v[3][3]; // v[a][b] = pos_ab of the reference: pixel (x - 1 + a, y - 1 + b)
        bool ok = true;
#pragma unroll
        for (uint32_t a = 0; a < 3u; a++)
#pragma unroll
            for (uint32_t b = 0; b < 3u; b++) {
                v[a][b] = in[(y - 1u + b) * W + (x - 1u + a)];
                ok = ok && v[a][b] != mi;
            }
        if (ok) {
            float resU = (-1.0f) * v[0][0] + (1.0f) * v[2][0] + (-2.0f) * v[0][1] + (2.0f) * v[2][1] + (-1.0f) * v[0][2] + (1.0f) * v[2][2];
            resU /= 8.0f;
            float resV = (-1.0f) * v[0][0] + (-2.0f) * v[1][0] + (-1.0f) * v[2][0] + (1.0f) * v[0][2] + (2.0f) * v[1][2] + (1.0f) * v[2][2];
            resV /= 8.0f;
            o = make_float4(v[1][1], resU, resV, 1.0f);
        }
    }
    out[i] = o;
}

constexpr float kPiF = 3.14159265358979323846f; // Scalar(M_PI) in float

// MatrixBase::eulerAngles(2, 1, 0) of the Eigen the reference vendors (Geometry/EulerAngles.h, 3.2.2), restated for
// this axis triple on a row-major 3x3 R: R = Rz(e0) Ry(e1) Rx(e2) with e0 in [0, pi].  A negative first angle is moved
// up by pi and the other two follow (so a small negative z-rotation comes back near (pi, pi, pi)); the Gauss-Newton
// step is taken in these angles, so the branch matters, not only the rotation they stand for.
VHD void euler_angles_zyx(const float* R, float* e)
{
    float e0 = atan2f(R[3], R[0]);
    const float c2 = sqrtf(R[8] * R[8] + R[7] * R[7]);
    float e1;
    if (e0 < 0.0f) {
        e0 = e0 + kPiF;
        e1 = atan2f(-R[6], -c2);
    } else {
        e1 = atan2f(-R[6], c2);
    }
    const float s1 = sinf(e0), c1 = cosf(e0);
    e[0] = e0;
    e[1] = e1;
    e[2] = atan2f(s1 * R[2] - c1 * R[5], c1 * R[4] - s1 * R[1]);
}

// Eigen::AngleAxisf(R).angle() (Geometry/AngleAxis.h:159-189 over the quaternion of Quaternion.h:724-760, Shoemake's
// construction): 2 acos(w), 0 when the quaternion's vector part is below dummy_precision (1e-5)
VHD float angle_axis_angle(const float* R)
{
    const float tr = R[0] + R[4] + R[8];
    float q[4]; // x, y, z, w
    if (tr > 0.0f) {
        float t = sqrtf(tr + 1.0f);
        q[3] = 0.5f * t;
        t = 0.5f / t;
        q[0] = (R[7] - R[5]) * t;
        q[1] = (R[2] - R[6]) * t;
        q[2] = (R[3] - R[1]) * t;
    } else {
        // (entries are selected, not indexed, and the vector part is summed from named values: an index known only at
        // run time would put R and q into scratch memory)
        auto r = [&](int at) {
            float v = R[0];
#pragma unroll
            for (int n = 1; n < 9; n++) v = at == n ? R[n] : v;
            return v;
        };
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > r(4 * i)) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        float t = sqrtf(r(4 * i) - r(4 * j) - r(4 * k) + 1.0f);
        const float qi = 0.5f * t;
        t = 0.5f / t;
        q[3] = (r(3 * k + j) - r(3 * j + k)) * t;
        const float qj = (r(3 * j + i) + r(3 * i + j)) * t;
        const float qk = (r(3 * k + i) + r(3 * i + k)) * t;
        q[0] = i == 0 ? qi : j == 0 ? qj : qk;
        q[1] = i == 1 ? qi : j == 1 ? qj : qk;
        q[2] = i == 2 ? qi : j == 2 ? qj : qk;
    }
    const float n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
    if (n2 < 1e-5f * 1e-5f) return 0.0f;
    return 2.0f * acosf(fminf(fmaxf(-1.0f, q[3]), 1.0f));
}

// anglesOld / translationOld of computeBestRigidAlignment (:204-208) from a row-major 4x4
VHD void rgbd_linearisation_point(VhIcpStateRGBD* st, const float* m)
{
    const float R[9] = { m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10] };
    euler_angles_zyx(R, st->angles);
    st->translation[0] = m[3];
    st->translation[1] = m[7];
    st->translation[2] = m[11];
}

__global__ void k_icp_rgbd_begin(VhIcpStateRGBD* st, const float* d_deltaEstimate)
{
    const uint32_t t = threadIdx.x;
    if (t < 16u) st->icp.delta[t] = d_deltaEstimate[t];
    if (t == 0u) {
        VhIcpState& s = st->icp;
        s.lost = 0u; s.done = 0u; s.lastError = -1.0f; s.iterations = 0u; s.sumRegError = 0.0f; s.sumRegWeight = 0.0f; s.numCorr = 0u; s.matrixCondition = 0.0f;
        float m[16];
        for (int k = 0; k < 16; k++) m[k] = d_deltaEstimate[k];
        rgbd_linearisation_point(st, m);
    }
}

// evalRMat and its three derivatives, DSC/ICPUtil.h:30-126, with (alpha, beta, gamma) = (angles.z, angles.y, angles.x):
// R = Rz(gamma) Ry(beta) Rx(alpha).  Row-major 3x3.
VHD void eval_r(float ca, float cb, float cg, float sa, float sb, float sg, float* R)
{
    R[0] = cg * cb; R[1] = -sg * ca + cg * sb * sa; R[2] = sg * sa + cg * sb * ca;
    R[3] = sg * cb; R[4] = cg * ca + sg * sb * sa;  R[5] = -cg * sa + sg * sb * ca;
    R[6] = -sb;     R[7] = cb * sa;                 R[8] = cb * ca;
}
VHD void eval_r_dalpha(float ca, float cb, float cg, float sa, float sb, float sg, float* R)
{
    R[0] = 0.0f; R[1] = sg * sa + cg * sb * ca;  R[2] = sg * ca - cg * sb * sa;
    R[3] = 0.0f; R[4] = -cg * sa + sg * sb * ca; R[5] = -cg * ca - sg * sb * sa;
    R[6] = 0.0f; R[7] = cb * ca;                 R[8] = -cb * sa;
}
VHD void eval_r_dbeta(float ca, float cb, float cg, float sa, float sb, float sg, float* R)
{
    R[0] = -cg * sb; R[1] = cg * cb * sa; R[2] = cg * cb * ca;
    R[3] = -sg * sb; R[4] = sg * cb * sa; R[5] = sg * cb * ca;
    R[6] = -cb;      R[7] = -sb * sa;     R[8] = -sb * ca;
}
VHD void eval_r_dgamma(float ca, float cb, float cg, float sa, float sb, float sg, float* R)
{
    R[0] = -sg * cb; R[1] = -cg * ca - sg * sb * sa; R[2] = cg * sa - sg * sb * ca;
    R[3] = cg * cb;  R[4] = -sg * ca + cg * sb * sa; R[5] = sg * sa + cg * sb * ca;
    R[6] = 0.0f;     R[7] = 0.0f;                    R[8] = 0.0f;
}
VHD F3 mat3_mul(const float* M, F3 v)
{
    return mk3(M[0] * v.x + M[1] * v.y + M[2] * v.z, M[3] * v.x + M[4] * v.y + M[5] * v.z, M[6] * v.x + M[7] * v.y + M[8] * v.z);
}

// lane window of the RGB-D build step (CUDABuildLinearSystemRGBD.cpp:31-32)
__host__ __device__ inline uint32_t icp_rgbd_window(uint32_t level) { return level == 0u ? kIcpWindow : (kIcpWindow / (4u * level) > 1u ? kIcpWindow / (4u * level) : 1u); }

// addToLocalSystem (.cu:78-104): one row J (6) with residual r and weight w into the lane's 30 terms
VHD void rgbd_add_row(float (&acc)[kIcpTerms], const float (&J)[6], float r, float w)
{
    uint32_t at = 0;
#pragma unroll
    for (uint32_t i = 0; i < 6u; i++) {
#pragma unroll
        for (uint32_t j = i; j < 6u; j++) acc[at + j - i] += J[i] * J[j] * w;
        at += 6u - i;
        acc[21u + i] -= J[i] * r * w; // -J^T F
    }
    acc[27] += w * (r * r);
    acc[28] += w;
    acc[29] += 1.0f;
}

// The linearisation point of an iteration as every pixel uses it: evalRMat(anglesOld), its derivatives and translationOld
struct RgbdLin {
    float R[9], Ralpha[9], Rbeta[9], Rgamma[9];
    F3 tOld;
};
// angles as the state holds them: (.x, .y, .z) = (gamma, beta, alpha)
VHD void rgbd_linearise(float ga, float be, float al, F3 tOld, RgbdLin& L)
{
    const float ca = cosf(al), cb = cosf(be), cg = cosf(ga), sa = sinf(al), sb = sinf(be), sg = sinf(ga);
    eval_r(ca, cb, cg, sa, sb, sg, L.R);
    eval_r_dgamma(ca, cb, cg, sa, sb, sg, L.Ralpha); // the reference's assignment (:133-135): Ralpha = evalR_dGamma, ...
    eval_r_dbeta(ca, cb, cg, sa, sb, sg, L.Rbeta);
    eval_r_dalpha(ca, cb, cg, sa, sb, sg, L.Rgamma);
    L.tOld = tOld;
}

// An input pixel of scanNormalEquationsDevice :106-201 after its project stage: what the accumulate stage needs of it,
// and where the model is to be read for it (a pixel that is dropped, a tap outside the image: pixel 0, not looked at)
struct RgbdPixel {
    F3 pT, nT, pp;      // the transformed point and normal, I pT
    float u, v;         // pp dehomogenized
    float pz, iIn;      // z of the UNtransformed point, the input intensity
    uint32_t at;        // getValueNearestNeighbour's pixel (ICPUtil.h:188-197) for the model point and normal
    uint32_t tapAt[4];  // the taps of bilinear_float4_taps
};

// Project stage; false: the pixel is dropped.
//
// Fenced reference defect: the reference converts floor(u), floor(v) of the projection to int for the bilinear lookup
// whatever their size; a point projected far off screen makes that an out-of-range float -> int conversion.  Such a
// pixel can never pair up (its nearest-neighbour lookup, truncating u + 0.5, lies outside the image and returns MINF),
// so it is rejected before any conversion: u + 0.5 and v + 0.5 must lie in (-1, W) and (-1, H).
VHD bool rgbd_project(const RgbdLin& L, const VhIcpRGBDParams& prm, uint32_t W, uint32_t H, float4 p4, float4 n4, float iIn, RgbdPixel& px)
{
    const float mi = minf();
    px.at = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) px.tapAt[k] = 0u;
    px.u = px.v = 0.0f;
    px.pT = px.nT = px.pp = mk3(0.0f, 0.0f, 0.0f);
    px.pz = p4.z;
    px.iIn = iIn;
    if (p4.x == mi || p4.y == mi || p4.z == mi || n4.x == mi || n4.y == mi || n4.z == mi || iIn == mi) return false;
    const F3 rp = mat3_mul(L.R, mk3(p4.x, p4.y, p4.z));
    px.nT = mat3_mul(L.R, mk3(n4.x, n4.y, n4.z));
    px.pT = mk3(rp.x + L.tOld.x, rp.y + L.tOld.y, rp.z + L.tOld.z);
    // pProjTrans = I pInputTransformed, I = [fx 0 mx; 0 fy my; 0 0 1]
    px.pp = mk3(prm.fx * px.pT.x + 0.0f * px.pT.y + prm.mx * px.pT.z, 0.0f * px.pT.x + prm.fy * px.pT.y + prm.my * px.pT.z,
                0.0f * px.pT.x + 0.0f * px.pT.y + 1.0f * px.pT.z);
    if (!(px.pp.z > 0.0f)) return false;
    px.u = px.pp.x / px.pp.z; px.v = px.pp.y / px.pp.z; // dehomogenize
    const float un = px.u + 0.5f, vn = px.v + 0.5f;
    if (!(un > -1.0f && un < (float)W && vn > -1.0f && vn < (float)H)) return false; // the fence (above)
    const int ui = f2i(un), vi = f2i(vn);
    if (ui < 0 || ui >= (int)W || vi < 0 || vi >= (int)H) return false;
    px.at = (uint32_t)vi * W + (uint32_t)ui;
    const int bx = (int)floorf(px.u), by = (int)floorf(px.v);
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        const int tx = bx + (int)(k & 1u), ty = by + (int)(k >> 1);
        if ((uint32_t)tx < W && (uint32_t)ty < H) px.tapAt[k] = (uint32_t)ty * W + (uint32_t)tx;
    }
    return true;
}

// Accumulate stage: a projected pixel with its model point tp, normal tn and intensity taps into the lane's 30 terms, as a
// point-to-plane row (:156-168) and, where the colours allow it, a photometric row (:170-185)
VHD void rgbd_accumulate(float (&acc)[kIcpTerms], const RgbdLin& L, const VhIcpRGBDParams& prm, uint32_t W, uint32_t H, const RgbdPixel& px,
                         float4 tp, float4 tn, const float4 (&tap)[4])
{
    const float mi = minf();
    const float4 it = bilinear_float4_taps(px.u, px.v, [&tap](uint32_t, uint32_t k) { return tap[k]; }, W, H); // (the taps are loaded already)
    if (tp.x == mi || tp.y == mi || tp.z == mi || tn.x == mi || tn.y == mi || tn.z == mi || it.x == mi || it.y == mi || it.z == mi) return;
    const F3 pT = px.pT;
    const F3 phiA = mat3_mul(L.Ralpha, pT), phiB = mat3_mul(L.Rbeta, pT), phiG = mat3_mul(L.Rgamma, pT);
    const F3 diff = mk3(tp.x - pT.x, tp.y - pT.y, tp.z - pT.z);
    const float dDist = sqrtf(diff.x * diff.x + diff.y * diff.y + diff.z * diff.z);
    const float dNormal = tn.x * px.nT.x + tn.y * px.nT.y + tn.z * px.nT.z;
    if (!(dDist <= prm.distThres && dNormal >= prm.normalThres)) return; // both rows need it
    {   // point to plane (z of the UNtransformed input point in the weight)
        const float wD = fmaxf(0.0f, 0.5f * ((1.0f - dDist / prm.distThres) + (1.0f - px.pz / prm.sensorMaxDepth)));
        const float J[6] = { -(tn.x * phiA.x + tn.y * phiA.y + tn.z * phiA.z), -(tn.x * phiB.x + tn.y * phiB.y + tn.z * phiB.z),
                             -(tn.x * phiG.x + tn.y * phiG.y + tn.z * phiG.z), -tn.x, -tn.y, -tn.z };
        const float r = tn.x * diff.x + tn.y * diff.y + tn.z * diff.z;
        rgbd_add_row(acc, J, r, prm.weightDepth * wD);
    }
    // colour: J = dI (1x2) * dehomogenizeDerivative (2x3) * K (3x3) * phi
    const F3 pp = px.pp;
    const float dI = it.x - px.iIn;
    const float gu = it.y, gv = it.z;
    const float absDI = sqrtf(dI * dI); // norm1D of the 1x1 residual
    if (absDI <= prm.colorThres && sqrtf(gu * gu + gv * gv) > prm.colorGradientMin) {
        const float wC = fmaxf(0.0f, 1.0f - absDI / prm.colorThres);
        const float iz = 1.0f / pp.z, wSq = pp.z * pp.z;
        const float d0 = gu * iz, d1 = gv * iz, d2 = gu * (-pp.x / wSq) + gv * (-pp.y / wSq); // dI PI
        const F3 g = mk3(d0 * prm.fx, d1 * prm.fy, d0 * prm.mx + d1 * prm.my + d2);         // (dI PI) K
        const float J[6] = { g.x * phiA.x + g.y * phiA.y + g.z * phiA.z, g.x * phiB.x + g.y * phiB.y + g.z * phiB.z,
                             g.x * phiG.x + g.y * phiG.y + g.z * phiG.z, g.x, g.y, g.z };
        rgbd_add_row(acc, J, dI, prm.weightColor * wC);
    }
}

// scanNormalEquationsDevice :106-201.  Lane x sums pixels [win x, win x + win) in order, the wave is reduced and lane 0
// writes its 30 terms: the shape and order of k_icp_build_system.
__global__ __launch_bounds__(64) void k_icp_rgbd_build_system(uint32_t W, uint32_t H, uint32_t window, float* partials, const float4* inPos,
                                                              const float4* inNormal, const float* inIntensity, const float4* tgtPos,
                                                              const float4* tgtNormal, const float4* tgtIntensity4, VhIcpRGBDParams prm,
                                                              const VhIcpStateRGBD* st)
{
    if (st->icp.lost || st->icp.done) return;
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    RgbdLin L;
    rgbd_linearise(st->angles[0], st->angles[1], st->angles[2], mk3(st->translation[0], st->translation[1], st->translation[2]), L);
    float acc[kIcpTerms];
#pragma unroll
    for (uint32_t k = 0; k < kIcpTerms; k++) acc[k] = 0.0f;
    for (uint32_t w = 0; w < window; w++) {
        const uint32_t idx = window * x + w;
        if (!(idx % W < W && idx / W < H)) continue;
        RgbdPixel px;
        if (!rgbd_project(L, prm, W, H, inPos[idx], inNormal[idx], inIntensity[idx], px)) continue;
        const float4 tap[4] = { tgtIntensity4[px.tapAt[0]], tgtIntensity4[px.tapAt[1]], tgtIntensity4[px.tapAt[2]], tgtIntensity4[px.tapAt[3]] };
        rgbd_accumulate(acc, L, prm, W, H, px, tgtPos[px.at], tgtNormal[px.at], tap);
    }
    const uint32_t lane = lane_id();
    icp_wave_sum(acc, lane);
    if (lane == 0u) icp_store_partials(partials, acc);
}

// computeBestRigidAlignment, delinearizeTransformation and checkRigidTransformation
// (DSC/CUDACameraTrackingMultiResRGBD.cpp:166-237) and the residual early-out of align (:329-350) on the 30 summed terms.
// Unlike f5, the solution is an increment of the absolute Euler angles and translation of delta
// (xNew = [anglesOld; translationOld] + x), and the rigidity check is on the new delta itself.  ATA.isZero() and a failed
// check both set lost; the reference would go on iterating with a matrix of -inf there.  One lane.
VHD void icp_rgbd_solve_step(VhIcpStateRGBD* st, const float* terms, float angleThres, float distThres, float earlyOut)
{
    VhIcpState& s = st->icp;
    double A[6][6], b[6];
    const bool nonzero = icp_system_from_terms(terms, A, b);
    s.sumRegError = terms[27];
    s.sumRegWeight = terms[28];
    s.numCorr = (uint32_t)terms[29];
    s.iterations += 1u;
    if (!nonzero) { s.lost = 1u; return; }
    double xs[6];
    s.matrixCondition = icp_solve_6x6(A, b, xs);
    float x[6];
    for (int k = 0; k < 3; k++) x[k] = st->angles[k] + (float)xs[k];
    for (int k = 0; k < 3; k++) x[3 + k] = st->translation[k] + (float)xs[3 + k];
    // delinearizeTransformation :177-194: R = Rz(x0) Ry(x1) Rx(x2), t = x[3..5]; mean 0, meanStDev 1
    const float cz = cosf(x[0]), sz = sinf(x[0]), cy = cosf(x[1]), sy = sinf(x[1]), cx = cosf(x[2]), sx = sinf(x[2]);
    const float R[9] = { cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx,
                         sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx,
                         -sy, cy * sx, cy * cx };
    // checkRigidTransformation :166-175 (a NaN fails it, as in f5)
    const float angle = angle_axis_angle(R);
    const float tnorm = sqrtf(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]);
    if (!(angle <= angleThres) || !(tnorm <= distThres)) { s.lost = 1u; return; }
    const float M[16] = { R[0], R[1], R[2], x[3], R[3], R[4], R[5], x[4], R[6], R[7], R[8], x[5], 0.0f, 0.0f, 0.0f, 1.0f };
    for (int k = 0; k < 16; k++) s.delta[k] = M[k];
    rgbd_linearisation_point(st, M);
    // align :345-350, after every outer iteration
    if (fabsf(s.lastError - s.sumRegError) < earlyOut) s.done = 1u;
    s.lastError = s.sumRegError;
}

// One wave: reductionSystemCPU (CUDABuildLinearSystemRGBD.cpp:46-86) over the wave partials in their order, then
// icp_rgbd_solve_step.
__global__ __launch_bounds__(64) void k_icp_rgbd_solve(VhIcpStateRGBD* st, const float* partials, uint32_t nPartials, float angleThres, float distThres, float earlyOut)
{
    __shared__ float sTerms[kIcpTerms];
    if (st->icp.lost || st->icp.done) return;
    icp_sum_terms(partials, nPartials, threadIdx.x, sTerms);
    if (threadIdx.x == 0u) icp_rgbd_solve_step(st, sTerms, angleThres, distThres, earlyOut);
}

// One outer iteration of the RGB-D align in one launch: k_icp_rgbd_build_system and k_icp_rgbd_solve.  A wave owns the
// pixels k_icp_rgbd_build_system gives it (lane x: [kWindow x, kWindow x + kWindow)) and sums them in that order through
// the same two stages; icp_hand_off gives the step to the wave that finishes last: the VhIcpStateRGBD after the launch
// is the two kernels' bit for bit.
// publish (may be null): mapped host memory that receives st->icp after this step, under `tag`.  A step that is skipped
// (lost / done) changes nothing, so its first wave publishes the state as it stands.
//
// kBatch pixels of the window at a time: their input loads go out together, then their model loads (position, normal
// and the four bilinear taps), then the sums take them in their order.
template <uint32_t kWindow, uint32_t kBatch>
__global__ __launch_bounds__(64) void k_icp_rgbd_step(uint32_t W, uint32_t H, float* partials, uint32_t* ticket, const float4* inPos, const float4* inNormal,
                                                      const float* inIntensity, const float4* tgtPos, const float4* tgtNormal, const float4* tgtIntensity4,
                                                      VhIcpRGBDParams prm, VhIcpStateRGBD* st, float angleThres, float distThres, float earlyOut,
                                                      VhIcpResult* publish, uint32_t tag)
{
    static_assert(kWindow % kBatch == 0u, "whole batches");
    __shared__ float sTerms[kIcpTerms];
    const uint32_t lane = threadIdx.x;
    const uint32_t skip = st->icp.lost | st->icp.done;
    const float ga = st->angles[0], be = st->angles[1], al = st->angles[2];
    const F3 tOld = mk3(st->translation[0], st->translation[1], st->translation[2]);
    if (skip) {
        if (publish && blockIdx.x == 0u && lane == 0u) icp_publish(&st->icp, publish, tag);
        return;
    }
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, nPixels = W * H;
    RgbdLin L;
    rgbd_linearise(ga, be, al, tOld, L);
    float acc[kIcpTerms];
#pragma unroll
    for (uint32_t k = 0; k < kIcpTerms; k++) acc[k] = 0.0f;
    for (uint32_t w0 = 0; w0 < kWindow; w0 += kBatch) {
        float4 p4[kBatch], n4[kBatch], tp[kBatch], tn[kBatch], tap[kBatch][4];
        float iIn[kBatch];
        RgbdPixel px[kBatch];
        bool ok[kBatch];
#pragma unroll
        for (uint32_t j = 0; j < kBatch; j++) {
            const uint32_t idx = kWindow * x + w0 + j;
            ok[j] = idx < nPixels;
            const uint32_t at = ok[j] ? idx : 0u; // (a pixel past the end reads pixel 0 and is dropped)
            p4[j] = inPos[at];
            n4[j] = inNormal[at];
            iIn[j] = inIntensity[at];
        }
#pragma unroll
        for (uint32_t j = 0; j < kBatch; j++) {
            if (!ok[j]) iIn[j] = minf(); // (dropped: no input there)
            ok[j] = rgbd_project(L, prm, W, H, p4[j], n4[j], iIn[j], px[j]);
        }
#pragma unroll
        for (uint32_t j = 0; j < kBatch; j++) { // (a pixel without a pair, a tap outside the image: pixel 0, not looked at)
            tp[j] = tgtPos[px[j].at];
            tn[j] = tgtNormal[px[j].at];
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) tap[j][k] = tgtIntensity4[px[j].tapAt[k]];
        }
#pragma unroll
        for (uint32_t j = 0; j < kBatch; j++)
            if (ok[j]) rgbd_accumulate(acc, L, prm, W, H, px[j], tp[j], tn[j], tap[j]);
    }
    icp_wave_sum(acc, lane);
    if (!icp_hand_off(partials, ticket, acc, lane, sTerms) || lane != 0u) return;
    icp_rgbd_solve_step(st, sTerms, angleThres, distThres, earlyOut);
    if (publish) icp_publish(&st->icp, publish, tag);
}

} // namespace

extern "C" {

int vh_icp_begin(VhIcpState* d_state, const float* d_deltaEstimate, vhStream_t stream)
{
    if (!d_state || !d_deltaEstimate) return VH_ERR_BAD_ARGUMENT;
    k_icp_begin<<<1, 64, 0, (hipStream_t)stream>>>(d_state, d_deltaEstimate);
    return vh_last_launch_error();
}
int vh_icp_begin_level(VhIcpState* d_state, vhStream_t stream)
{
    if (!d_state) return VH_ERR_BAD_ARGUMENT;
    k_icp_begin_level<<<1, 64, 0, (hipStream_t)stream>>>(d_state);
    return vh_last_launch_error();
}
int vh_icp_projective_correspondences(const float* d_input4, const float* d_inputNormals4, const float* d_target4, const float* d_targetNormals4,
                                      float* d_output4, float* d_outputNormals4, uint32_t width, uint32_t height, float distThres, float normalThres,
                                      float levelFactor, const VhIcpState* d_state, const VhDepthCameraParams* cp, vhStream_t stream)
{
    if (!d_input4 || !d_inputNormals4 || !d_target4 || !d_targetNormals4 || !d_output4 || !d_outputNormals4 || !d_state || !cp) return VH_ERR_BAD_ARGUMENT;
    if (width * height == 0) return VH_OK;
    k_icp_correspondences<<<cdiv(width * height, 256u), 256, 0, (hipStream_t)stream>>>(
        reinterpret_cast<const float4*>(d_input4), reinterpret_cast<const float4*>(d_inputNormals4), reinterpret_cast<const float4*>(d_target4),
        reinterpret_cast<const float4*>(d_targetNormals4), reinterpret_cast<float4*>(d_output4), reinterpret_cast<float4*>(d_outputNormals4), width, height,
        distThres, normalThres, levelFactor, d_state, *cp);
    return vh_last_launch_error();
}
uint32_t vh_icp_num_partials(uint32_t width, uint32_t height) { return cdiv(width * height, 64u * kIcpWindow); }
int vh_icp_build_linear_system(uint32_t width, uint32_t height, float* d_partials, const float* d_input4, const float* d_corr4, const float* d_corrNormals4,
                               const VhIcpState* d_state, vhStream_t stream)
{
    if (!d_partials || !d_input4 || !d_corr4 || !d_corrNormals4 || !d_state) return VH_ERR_BAD_ARGUMENT;
    if (width * height == 0) return VH_OK;
    k_icp_build_system<<<vh_icp_num_partials(width, height), 64, 0, (hipStream_t)stream>>>(
        width, height, d_partials, reinterpret_cast<const float4*>(d_input4), reinterpret_cast<const float4*>(d_corr4),
        reinterpret_cast<const float4*>(d_corrNormals4), d_state);
    return vh_last_launch_error();
}
int vh_icp_solve(VhIcpState* d_state, const float* d_partials, uint32_t numPartials, float angleThres, float distThres, float earlyOutResidual,
                 int lastInnerIteration, vhStream_t stream)
{
    if (!d_state || !d_partials) return VH_ERR_BAD_ARGUMENT;
    k_icp_solve<<<1, 64, 0, (hipStream_t)stream>>>(d_state, d_partials, numPartials, angleThres, distThres, earlyOutResidual, lastInnerIteration ? 1u : 0u);
    return vh_last_launch_error();
}

int vh_icp_step(const float* d_input4, const float* d_inputNormals4, const float* d_target4, const float* d_targetNormals4, uint32_t width, uint32_t height,
                float distThres, float normalThres, float levelFactor, const VhDepthCameraParams* cp, float* d_partials, uint32_t* d_ticket,
                VhIcpState* d_state, float angleTransThres, float distTransThres, float earlyOutResidual, VhIcpResult* publish, uint32_t tag, vhStream_t stream)
{
    if (!d_input4 || !d_inputNormals4 || !d_target4 || !d_targetNormals4 || !cp || !d_partials || !d_ticket || !d_state) return VH_ERR_BAD_ARGUMENT;
    if (width * height == 0) return VH_ERR_BAD_ARGUMENT; // (no wave would draw the last ticket)
    k_icp_step<<<vh_icp_num_partials(width, height), 64, 0, (hipStream_t)stream>>>(
        reinterpret_cast<const float4*>(d_input4), reinterpret_cast<const float4*>(d_inputNormals4), reinterpret_cast<const float4*>(d_target4),
        reinterpret_cast<const float4*>(d_targetNormals4), width, height, distThres, normalThres, levelFactor, *cp, d_partials, d_ticket, d_state,
        angleTransThres, distTransThres, earlyOutResidual, publish, tag);
    return vh_last_launch_error();
}
int vh_icp_publish(const VhIcpState* d_state, VhIcpResult* publish, uint32_t tag, vhStream_t stream)
{
    if (!d_state || !publish) return VH_ERR_BAD_ARGUMENT;
    k_icp_publish<<<1, 64, 0, (hipStream_t)stream>>>(d_state, publish, tag);
    return vh_last_launch_error();
}

int vh_compute_intensity_and_derivatives(const float* d_intensity, uint32_t width, uint32_t height, float* d_intensityAndDerivatives4, vhStream_t stream)
{
    if (!d_intensity || !d_intensityAndDerivatives4) return VH_ERR_BAD_ARGUMENT;
    if (width * height == 0) return VH_OK;
    k_intensity_and_derivatives<<<cdiv(width * height, 256u), 256, 0, (hipStream_t)stream>>>(reinterpret_cast<float4*>(d_intensityAndDerivatives4), d_intensity, width, height);
    return vh_last_launch_error();
}
int vh_icp_rgbd_begin(VhIcpStateRGBD* d_state, const float* d_deltaEstimate, vhStream_t stream)
{
    if (!d_state || !d_deltaEstimate) return VH_ERR_BAD_ARGUMENT;
    k_icp_rgbd_begin<<<1, 64, 0, (hipStream_t)stream>>>(d_state, d_deltaEstimate);
    return vh_last_launch_error();
}
uint32_t vh_icp_rgbd_num_partials(uint32_t width, uint32_t height, uint32_t level) { return cdiv(width * height, 64u * icp_rgbd_window(level)); }
int vh_icp_rgbd_build_linear_system(uint32_t width, uint32_t height, float* d_partials, const float* d_input4, const float* d_inputNormals4,
                                    const float* d_inputIntensity, const float* d_target4, const float* d_targetNormals4,
                                    const float* d_targetIntensityAndDerivatives4, const VhIcpRGBDParams* params, const VhIcpStateRGBD* d_state,
                                    vhStream_t stream)
{
    if (!d_partials || !d_input4 || !d_inputNormals4 || !d_inputIntensity || !d_target4 || !d_targetNormals4 || !d_targetIntensityAndDerivatives4 ||
        !params || !d_state)
        return VH_ERR_BAD_ARGUMENT;
    if (width * height == 0) return VH_OK;
    const uint32_t window = icp_rgbd_window(params->level);
    k_icp_rgbd_build_system<<<vh_icp_rgbd_num_partials(width, height, params->level), 64, 0, (hipStream_t)stream>>>(
        width, height, window, d_partials, reinterpret_cast<const float4*>(d_input4), reinterpret_cast<const float4*>(d_inputNormals4), d_inputIntensity,
        reinterpret_cast<const float4*>(d_target4), reinterpret_cast<const float4*>(d_targetNormals4),
        reinterpret_cast<const float4*>(d_targetIntensityAndDerivatives4), *params, d_state);
    return vh_last_launch_error();
}
int vh_icp_rgbd_solve(VhIcpStateRGBD* d_state, const float* d_partials, uint32_t numPartials, float angleThres, float distThres, float earlyOutResidual,
                      vhStream_t stream)
{
    if (!d_state || !d_partials) return VH_ERR_BAD_ARGUMENT;
    k_icp_rgbd_solve<<<1, 64, 0, (hipStream_t)stream>>>(d_state, d_partials, numPartials, angleThres, distThres, earlyOutResidual);
    return vh_last_launch_error();
}
int vh_icp_rgbd_step(uint32_t width, uint32_t height, float* d_partials, uint32_t* d_ticket, const float* d_input4, const float* d_inputNormals4,
                     const float* d_inputIntensity, const float* d_target4, const float* d_targetNormals4, const float* d_targetIntensityAndDerivatives4,
                     const VhIcpRGBDParams* params, VhIcpStateRGBD* d_state, float angleThres, float distThres, float earlyOutResidual, VhIcpResult* publish,
                     uint32_t tag, vhStream_t stream)
{
    if (!d_partials || !d_ticket || !d_input4 || !d_inputNormals4 || !d_inputIntensity || !d_target4 || !d_targetNormals4 ||
        !d_targetIntensityAndDerivatives4 || !params || !d_state)
        return VH_ERR_BAD_ARGUMENT;
    if (width * height == 0) return VH_ERR_BAD_ARGUMENT; // (no wave would draw the last ticket)
    const uint32_t grid = vh_icp_rgbd_num_partials(width, height, params->level);
#define VH_RGBD_STEP(window, batch)                                                                                                                         \
    k_icp_rgbd_step<window, batch><<<grid, 64, 0, (hipStream_t)stream>>>(                                                                                   \
        width, height, d_partials, d_ticket, reinterpret_cast<const float4*>(d_input4), reinterpret_cast<const float4*>(d_inputNormals4), d_inputIntensity, \
        reinterpret_cast<const float4*>(d_target4), reinterpret_cast<const float4*>(d_targetNormals4),                                                      \
        reinterpret_cast<const float4*>(d_targetIntensityAndDerivatives4), *params, d_state, angleThres, distThres, earlyOutResidual, publish, tag)
    switch (icp_rgbd_window(params->level)) { // 12 / 3 / 1
    case kIcpWindow: VH_RGBD_STEP(kIcpWindow, 6u); break;
    case 3u: VH_RGBD_STEP(3u, 3u); break;
    default: VH_RGBD_STEP(1u, 1u); break;
    }
#undef VH_RGBD_STEP
    return vh_last_launch_error();
}
} // extern "C"
