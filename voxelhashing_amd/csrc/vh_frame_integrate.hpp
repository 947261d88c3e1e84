// vh_frame_integrate.hpp -- frame loop: the pass over the voxels.  The reference's separate kernels (k_integrate, k_starve,
// k_gc_identify, k_gc_free) and the fused pass (integrate + starve + GC: FusedArgs, integrate_fused_body,
// k_integrate_fused), with what a rider needs of it (rider_wait, integrate_block_by_workgroup).  Included by
// vh_kernels.hip, by vh_frame_normals.hpp (k_compute_normals carries the pass as a rider) and by vh_frame_checks.hpp (the
// checks of its arithmetic).
#pragma once

#include "../../include/vh_api.h"
#include "vh_device.hpp"
#include "vh_frame_alloc.hpp"
#include "vh_frame_compactify.hpp"

namespace {
using namespace vhd;

// ---------------------------------------------------------------------------
// integrate / starve / garbage collection
// (integrateDepthMapKernel :412-492, starveVoxelsKernel :512-521,
//  garbageCollectIdentifyKernel :543-590, garbageCollectFreeKernel :608-628)
//
// One 256-thread workgroup per SDF block, two x-adjacent voxels (16 B) per
// lane: a block is 4 waves x 1 KiB fully coalesced.  The fused kernel keeps the
// block in registers across integrate -> starve -> identify -> free, so every
// voxel is read once and written once per frame; min/max are reduced with
// wave64 shuffles and a 4-entry LDS combine.
// ---------------------------------------------------------------------------

VHD Vox integrate_voxel(const VhHashParams& hp, const VhDepthCameraParams& cp, const VhDepthCameraData& cam, I3 pi, Vox stored)
{
    F3 pf = mat_mul_p(hp.m_rigidTransformInverse, vvp_to_world(hp.m_virtualVoxelSize, pi));
    // cameraToKinectScreenInt, DSC/DepthCameraUtil.h:74-85 -> uint2
    const uint32_t sx = (uint32_t)f2i((pf.x * cp.fx / pf.z + cp.mx) + 0.5f);
    const uint32_t sy = (uint32_t)f2i((pf.y * cp.fy / pf.z + cp.my) + 0.5f);
    if (sx < cp.m_imageWidth && sy < cp.m_imageHeight) {
        const uint32_t pix = sy * cp.m_imageWidth + sx;
        const float depth = cam.d_depthData[pix];
        float cr = minf(), cg = minf(), cb = minf();
        if (cam.d_colorData) {
            const float4 c = reinterpret_cast<const float4*>(cam.d_colorData)[pix];
            cr = c.x; cg = c.y; cb = c.z;
        }
        if (cr != minf() && depth != minf()) {
            if (depth < hp.m_maxIntegrationDistance) {
                const float depthZeroOne = cam_to_proj_z(cp, depth);
                float sdf = depth - pf.z;
                const float truncation = get_truncation(hp, depth);
                if (sdf > -truncation) {
                    if (sdf >= 0.0f) sdf = fminf(truncation, sdf);
                    else sdf = fmaxf(-truncation, sdf);
                    const float weightUpdate = fmaxf((float)hp.m_integrationWeightSample * 1.5f * (1.0f - depthZeroOne), 1.0f);
                    Vox curr;
                    curr.sdf = sdf;
                    if (cam.d_colorData) curr.cw = pack_cw(f2uc(255.0f * cr), f2uc(255.0f * cg), f2uc(255.0f * cb), f2uc(weightUpdate));
                    else curr.cw = pack_cw(0, 255, 0, f2uc(weightUpdate));
                    return combine_voxel(hp, stored, curr);
                }
            }
        }
    }
    return stored;
}

VHD Vox starve_voxel(Vox v)
{
    uint32_t w = v.weight();
    w = (w > 0u) ? w - 1u : 0u;
    v.cw = (v.cw & 0x00ffffffu) | (w << 24);
    return v;
}

// block-wide min(|sdf| of weighted voxels) / max(weight): wave shuffle tree,
// then one LDS slot per wave.  Every lane returns the block result.
VHD void block_min_max(float& minSdf, uint32_t& maxW, float* sMin, uint32_t* sMax)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        minSdf = fminf(minSdf, __shfl_xor(minSdf, o));
        maxW = max(maxW, (uint32_t)__shfl_xor((int)maxW, o));
    }
    const uint32_t wave = threadIdx.x / kWave;
    if (lane_id() == 0) { sMin[wave] = minSdf; sMax[wave] = maxW; }
    __syncthreads();
    float m = sMin[0];
    uint32_t w = sMax[0];
    for (uint32_t i = 1; i < blockDim.x / kWave; i++) { m = fminf(m, sMin[i]); w = max(w, sMax[i]); }
    minSdf = m; maxW = w;
}

VHD float gc_key(Vox v) { return (v.weight() == 0u) ? pinf() : fabsf(v.sdf); }

template <bool FUSED>
__global__ __launch_bounds__(256) void k_integrate(VhHashData hd, VhHashParams hp, VhDepthCameraData cam,
                                                   VhDepthCameraParams cp, uint32_t flags, int32_t lockToken, uint32_t* countMirror)
{
    __shared__ float sMin[4];
    __shared__ uint32_t sMax[4];
    __shared__ int sFreed;

    const uint32_t count = FUSED ? (uint32_t)hd.d_hashCompactifiedCounter[0] : hp.m_numOccupiedBlocks;
    // host-visible copy of the block count (mapped pinned memory): replaces a per-frame device->host copy
    if (FUSED && countMirror && blockIdx.x == 0 && threadIdx.x == 0) *countMirror = count;
    const uint32_t t = threadIdx.x;
    // voxel pair (2t, 2t+1): x = (2t)%8 (+1), y = (2t%64)/8, z = 2t/64  (delinearizeVoxelIndex, DSC/VoxelUtilHashSDF.h:313-318)
    const int lx = (int)((2u * t) & 7u), ly = (int)(((2u * t) & 63u) >> 3), lz = (int)((2u * t) >> 6);

    for (uint32_t b = blockIdx.x; b < count; b += gridDim.x) {
        const int4 q = load_quad(&hd.d_hashCompactified[b]);
        const int ex = __builtin_amdgcn_readfirstlane(q.x), ey = __builtin_amdgcn_readfirstlane(q.y);
        const int ez = __builtin_amdgcn_readfirstlane(q.z), ptr = __builtin_amdgcn_readfirstlane(q.w);

        uint4* vp = reinterpret_cast<uint4*>(&hd.d_SDFBlocks[(uint32_t)ptr]) + t;
        const uint4 raw = *vp;
        Vox v0 = unpack_vox(make_uint2(raw.x, raw.y)), v1 = unpack_vox(make_uint2(raw.z, raw.w));

        const I3 p0 = mki3(ex * VH_SDF_BLOCK_SIZE + lx, ey * VH_SDF_BLOCK_SIZE + ly, ez * VH_SDF_BLOCK_SIZE + lz);
        v0 = integrate_voxel(hp, cp, cam, p0, v0);
        v1 = integrate_voxel(hp, cp, cam, mki3(p0.x + 1, p0.y, p0.z), v1);
        // Pin the four result words in VGPRs here.  Without this, hipcc (ROCm 7.2, gfx950, -O3) merges the
        // "not integrated" path of the second voxel with a register that the colour fetch has already
        // overwritten (found by the parity tests: sdf of skipped odd voxels came back as the colour's MINF).
        asm volatile("" : "+v"(v0.sdf), "+v"(v0.cw), "+v"(v1.sdf), "+v"(v1.cw));

        bool freed = false;
        if (FUSED && (flags & VH_FUSED_GC)) {
            if (flags & VH_FUSED_STARVE) { v0 = starve_voxel(v0); v1 = starve_voxel(v1); }
            float minSdf = fminf(gc_key(v0), gc_key(v1));
            uint32_t maxW = max(v0.weight(), v1.weight());
            __syncthreads(); // LDS slots of the previous block iteration are consumed
            block_min_max(minSdf, maxW, sMin, sMax);
            const float thr = get_truncation(hp, cp.m_sensorDepthWorldMax);
            const bool decide = (minSdf >= thr) || (maxW == 0u);
            if (t == 0) {
                hd.d_hashDecision[b] = decide ? 1 : 0;
                sFreed = (decide && delete_hash_entry_element(hd, hp, mki3(ex, ey, ez), lockToken)) ? 1 : 0;
            }
            __syncthreads();
            freed = sFreed != 0;
        }
        if (freed) {
            *vp = make_uint4(0u, 0u, 0u, 0u);
        } else {
            const uint2 a = pack_vox(v0), c = pack_vox(v1);
            *vp = make_uint4(a.x, a.y, c.x, c.y);
        }
    }
}

// integrate_voxel on a frame packed by alloc_tile / pack_pixel, in two steps: where the voxel projects to, and what
// the pixel found there makes of the stored voxel
VHD bool project_voxel(const VhHashParams& hp, const VhDepthCameraParams& cp, I3 pi, uint32_t& sx, uint32_t& sy, float& pz)
{
    F3 pf = mat_mul_p(hp.m_rigidTransformInverse, vvp_to_world(hp.m_virtualVoxelSize, pi));
    sx = (uint32_t)f2i((pf.x * cp.fx / pf.z + cp.mx) + 0.5f);
    sy = (uint32_t)f2i((pf.y * cp.fy / pf.z + cp.my) + 0.5f);
    pz = pf.z;
    return sx < cp.m_imageWidth && sy < cp.m_imageHeight;
}
VHD Vox apply_pixel(const VhHashParams& hp, uint2 px, float pz, Vox stored)
{
    // Without branches: every lane forms the blend, a select keeps or drops it (the lanes of a wave rarely agree, and
    // straight-line code lets the eight voxels of a lane overlap: measured 6 % on the dense scene).  The arithmetic of a
    // kept blend is integrateDepthMapKernel's (:447-472); a dropped one may be anything, NaN included.
    const float depth = __uint_as_float(px.x);
    float sdf = depth - pz;
    const float truncation = get_truncation(hp, depth);
    // a sample: valid depth within the integration distance, valid colour (weight byte, pack_pixel), not behind the band
    const bool use = ((px.y >> 24) != 0u) && (sdf > -truncation);
    const float lo = fmaxf(-truncation, sdf), hi = fminf(truncation, sdf);
    Vox curr;
    curr.sdf = (sdf >= 0.0f) ? hi : lo;
    curr.cw = px.y;
    const Vox c = combine_voxel(hp, stored, curr);
    Vox out;
    out.sdf = use ? c.sdf : stored.sdf;
    out.cw = use ? c.cw : stored.cw;
    return out;
}
VHD Vox integrate_voxel_packed(const VhHashParams& hp, const VhDepthCameraParams& cp, const uint2* packed, I3 pi, Vox stored)
{
    uint32_t sx, sy;
    float pz;
    if (project_voxel(hp, cp, pi, sx, sy, pz)) return apply_pixel(hp, packed[sy * cp.m_imageWidth + sx], pz, stored);
    return stored;
}

// The fused pass: integrate -> starve -> identify -> free with every voxel read once and written once.  The block count
// lives on the device (no host round trip), so the grid is fixed and the kernel picks its shape from the count:
//   * few blocks (count <= workgroups): one WORKGROUP per block, two x-adjacent voxels (16 B) per lane -- the frame is
//     a latency chain (entry -> voxels -> gather -> table edit), and four waves per block keep it short;
//   * many blocks: one WAVE per block (4 KB = four 16-byte loads per lane), at most 5120 waves (five per SIMD; the
//     active waves fill whole workgroups); wave w takes blocks w, w + 5120, ... -- dealt statically (a ticket counter
//     was measured: 165 us, agent-scope atomics on one address are served one after the other).  min |sdf| / max weight are a
//     wave reduction (no LDS, no barrier); lane 0 edits the table; the block's screen footprint is staged in LDS and
//     blocks whose corners pass a range certificate take the packed arithmetic of integrate_block_certified (below).
// Load j of lane l of a wave that holds a whole block: voxels 128 j + 2 l and + 1, i.e. x = 2l mod 8 (+1),
// y = (l / 4) mod 8, z = 2j + l / 32 (delinearizeVoxelIndex, DSC/VoxelUtilHashSDF.h:313-318).
template <bool PACKED>
VHD void integrate_pair(const VhHashParams& hp, const VhDepthCameraParams& cp, const VhDepthCameraData& cam, const uint2* packed,
                        uint32_t flags, I3 p0, uint4& raw, float& minSdf, uint32_t& maxW)
{
    Vox v0 = unpack_vox(make_uint2(raw.x, raw.y)), v1 = unpack_vox(make_uint2(raw.z, raw.w));
    if (PACKED) {
        v0 = integrate_voxel_packed(hp, cp, packed, p0, v0);
        v1 = integrate_voxel_packed(hp, cp, packed, mki3(p0.x + 1, p0.y, p0.z), v1);
    } else {
        v0 = integrate_voxel(hp, cp, cam, p0, v0);
        v1 = integrate_voxel(hp, cp, cam, mki3(p0.x + 1, p0.y, p0.z), v1);
    }
    // Pin the result words in VGPRs here.  Without this, hipcc (ROCm 7.2, gfx950, -O3) merges the "not integrated" path
    // of the second voxel with a register that the gather has already overwritten (found by the parity tests: sdf of
    // skipped odd voxels came back as the colour's MINF).
    asm volatile("" : "+v"(v0.sdf), "+v"(v0.cw), "+v"(v1.sdf), "+v"(v1.cw));
    if (flags & VH_FUSED_STARVE) { v0 = starve_voxel(v0); v1 = starve_voxel(v1); }
    minSdf = fminf(minSdf, fminf(gc_key(v0), gc_key(v1)));
    maxW = max(maxW, max(v0.weight(), v1.weight()));
    const uint2 a = pack_vox(v0), c = pack_vox(v1);
    raw = make_uint4(a.x, a.y, c.x, c.y);
}

// ---- the voxel pair of a lane as a two-vector (f32x2, both, fma2: vh_device.hpp)
// The reciprocal the compiler's own expansion of an fp32 division forms when v_div_scale_f32 leaves its operands alone:
// v_rcp_f32 and one Newton step.
VHD f32x2 rcp_refined2(f32x2 d)
{
    const f32x2 y0 = (f32x2){ __builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y) };
    const f32x2 e = fma2(-d, y0, both(1.0f));
    return fma2(e, y0, y0);
}
// n / d with y = rcp_refined2(d): the rest of that expansion (product, two residual corrections), instruction for
// instruction, minus v_div_scale / v_div_fmas' scaling / v_div_fixup.  Those three only act when an operand is zero,
// infinite, NaN or denormal, when |n| < 2^-103, when |d| >= 2^126 or when the exponents of n and d are 96 or more apart
// (the ISA's v_div_scale_f32 cases); outside of that the result is the division's, bit for bit.  Callers guard the range.
VHD f32x2 div_refined2(f32x2 n, f32x2 d, f32x2 y)
{
    f32x2 q = n * y;
    f32x2 r = fma2(-d, q, n);
    q = fma2(r, y, q);
    r = fma2(-d, q, n);
    return fma2(r, y, q);
}

// One block by one wave, the hot shape of the dense case: integrate_voxel_packed for the eight voxels of a lane (four
// x-adjacent pairs) with ~60 instead of ~110 vector instructions per voxel.  Only for blocks the caller has certified:
//   * the block's footprint is staged in LDS (tile, x0, y0, w, h);
//   * at all eight CORNER voxels 2^-20 <= pf.z <= 2^20 and |pf.x fx|, |pf.y fy| <= 2^60.  Every voxel of the block then
//     satisfies the same: each float operation of the transform is monotone in each of its operands, so pf.x, pf.y,
//     pf.z and the two products, as computed, take their extremes over the block at corner voxels;
//   * m_truncation > 0, m_truncScale >= 0 (so that a pixel that integrates has truncation > 0: the reference's
//     two-sided clamp is then the median of {sdf, -truncation, truncation}).
// What changes against the plain code, none of it in the results:
//   * the two divisions by pf.z share one refined reciprocal (div_refined2; a numerator below 2^-60, where the
//     argument above stops, gives a quotient below 2^-38 by either route, which the following "+ mx, + 0.5, truncate"
//     cannot see);
//   * the blend's division by the weight sum (1..510) takes the same route, with the exact division for any numerator
//     outside [2^-100, 2^90) (never seen with voxels this library wrote; a crafted .hashgrid could hold one);
//   * the pixel comes from the staged tile by an LDS read; a voxel that projects outside the staged box (not seen: the
//     box is the hull of the corners' pixels and a margin) is gathered from the frame as before;
//   * everything is written for the pair of a lane, so that the compiler can issue packed fp32.
VHD void integrate_block_certified(const VhHashParams& hp, const VhDepthCameraParams& cp, const uint2* packed, const uint2* tile, uint32_t tileStride,
                                   uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, int ex, int ey, int ez, uint32_t lane, uint32_t flags,
                                   uint4 (&raw)[4], float& minSdf, uint32_t& maxW)
{
    // (The transform as values of this function's own: packed instructions want their uniform operands in vector registers,
    // and copies shared with the kernel's other code paths live from the top of the kernel to its end -- the compiler
    // parks them in scratch memory, a store per lane of every wave of the launch.)
    float vs = hp.m_virtualVoxelSize;
    float m[12];
#pragma unroll
    for (int i = 0; i < 12; i++) m[i] = hp.m_rigidTransformInverse[i];
    asm volatile("" : "+s"(vs), "+s"(m[0]), "+s"(m[1]), "+s"(m[2]), "+s"(m[3]), "+s"(m[4]), "+s"(m[5]), "+s"(m[6]), "+s"(m[7]), "+s"(m[8]), "+s"(m[9]),
                      "+s"(m[10]), "+s"(m[11]));
    const int lx = (int)((2u * lane) & 7u), ly = (int)((lane >> 2) & 7u), lz0 = (int)(lane >> 5);
    // vvp_to_world, mat_mul_p: ((m0 x + m1 y) + m2 z) + m3 per row; the first sum does not depend on z
    const f32x2 xw = (f32x2){ (float)(ex * VH_SDF_BLOCK_SIZE + lx), (float)(ex * VH_SDF_BLOCK_SIZE + lx + 1) } * vs;
    const float yw = (float)(ey * VH_SDF_BLOCK_SIZE + ly) * vs;
    f32x2 ab[3];
#pragma unroll
    for (int r = 0; r < 3; r++) ab[r] = m[4 * r] * xw + both(m[4 * r + 1] * yw);
    uint32_t maxCw = 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float zw = (float)(ez * VH_SDF_BLOCK_SIZE + 2 * j + lz0) * vs;
        f32x2 pf[3];
#pragma unroll
        for (int r = 0; r < 3; r++) pf[r] = (ab[r] + both(m[4 * r + 2] * zw)) + both(m[4 * r + 3] * 1.0f);
        // cameraToKinectScreenInt: int((pf.x fx / pf.z + mx) + 0.5f), likewise y
        const f32x2 y = rcp_refined2(pf[2]);
        const f32x2 fsx = (div_refined2(pf[0] * cp.fx, pf[2], y) + cp.mx) + 0.5f;
        const f32x2 fsy = (div_refined2(pf[1] * cp.fy, pf[2], y) + cp.my) + 0.5f;
        uint2 px[2]; // the pixel of each voxel; weight byte 0: nothing to integrate (pack_pixel), or no pixel at all
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const uint32_t sx = (uint32_t)cvt_rz(fsx[k]), sy = (uint32_t)cvt_rz(fsy[k]);
            const uint32_t tx = sx - x0, ty = sy - y0; // unsigned: a pixel left of / above the box wraps to a huge number
            const bool inBox = (tx < w) & (ty < h);    // the box lies inside the image
            // (one ballot per comparison: the ballot of their conjunction goes through a register and back)
            const bool allInBox = (__builtin_amdgcn_ballot_w64(tx < w) & __builtin_amdgcn_ballot_w64(ty < h)) == ~0ull; // (every lane is active here)
            // (as one indivisible 8-byte read: left alone the compiler splits it in two)
            // (no clamp of the index: an LDS read beyond the workgroup's allocation returns zero, one inside it some other
            // pixel, and the weight byte of a voxel outside the box is cleared below either way)
            const unsigned long long t = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(&tile[__umul24(ty, tileStride) + tx]),
                                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            px[k] = make_uint2((uint32_t)t, inBox ? (uint32_t)(t >> 32) : 0u);
            if (__builtin_expect(!allInBox, 0)) {
                if (!inBox && sx < cp.m_imageWidth && sy < cp.m_imageHeight) px[k] = packed[sy * cp.m_imageWidth + sx];
            }
        }
        // integrateDepthMapKernel :447-472 and combineVoxel :229-250 (apply_pixel / combine_voxel above) for the pair
        const Vox s0 = unpack_vox(make_uint2(raw[j].x, raw[j].y)), s1 = unpack_vox(make_uint2(raw[j].z, raw[j].w));
        const f32x2 depth = (f32x2){ __uint_as_float(px[0].x), __uint_as_float(px[1].x) };
        const f32x2 sdf = depth - pf[2];
        const f32x2 truncation = both(hp.m_truncation) + hp.m_truncScale * depth;
        const bool use0 = ((px[0].y >> 24) != 0u) & (sdf.x > -truncation.x);
        const bool use1 = ((px[1].y >> 24) != 0u) & (sdf.y > -truncation.y);
        const f32x2 clamped = (f32x2){ __builtin_amdgcn_fmed3f(sdf.x, -truncation.x, truncation.x), __builtin_amdgcn_fmed3f(sdf.y, -truncation.y, truncation.y) };
        const f32x2 wOld = (f32x2){ (float)(s0.cw >> 24), (float)(s1.cw >> 24) }, wNew = (f32x2){ (float)(px[0].y >> 24), (float)(px[1].y >> 24) };
        const f32x2 num = (f32x2){ s0.sdf, s1.sdf } * wOld + clamped * wNew;
        const f32x2 den = wOld + wNew; // exact: integers up to 510
        const f32x2 yDen = rcp_refined2(den);
        f32x2 q = div_refined2(num, den, yDen);
        const bool odd0 = use0 & !((fabsf(num.x) >= 0x1p-100f) & (fabsf(num.x) < 0x1p90f));
        const bool odd1 = use1 & !((fabsf(num.y) >= 0x1p-100f) & (fabsf(num.y) < 0x1p90f));
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(odd0 | odd1) != 0ull, 0)) {
            if (odd0) q.x = num.x / den.x;
            if (odd1) q.y = num.y / den.y;
        }
        Vox v[2];
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const Vox st = k ? s1 : s0;
            // colour: the byte-wise average rounded up (combine_voxel) is v_lerp_u8 with the rounding bit set; the weight
            // byte comes in by v_perm_b32 (the top byte of the average is not used)
            // (m_colorIntegration: the average weighted by the voxel weights instead, with the reciprocal of the sdf's
            // division; the same for every voxel of the launch, a scalar branch)
            uint32_t rgb = __builtin_amdgcn_lerp(st.cw, px[k].y, 0x01010101u);
            if (hp.m_colorIntegration != VH_COLOR_RUNNING_AVERAGE) rgb = weighted_colour(st.cw, px[k].y, den[k], yDen[k]);
            const uint32_t wSum = min(hp.m_integrationWeightMax, (st.cw >> 24) + (px[k].y >> 24));
            const bool use = k ? use1 : use0;
            v[k].sdf = use ? q[k] : st.sdf;
            v[k].cw = use ? __builtin_amdgcn_perm(wSum, rgb, 0x04020100u) : st.cw;
        }
        if (flags & VH_FUSED_STARVE) { v[0] = starve_voxel(v[0]); v[1] = starve_voxel(v[1]); }
        minSdf = fminf(minSdf, fminf(gc_key(v[0]), gc_key(v[1])));
        maxCw = max(maxCw, max(v[0].cw, v[1].cw)); // the weight is the top byte: the largest word has the largest weight
        const uint2 a = pack_vox(v[0]), c = pack_vox(v[1]);
        raw[j] = make_uint4(a.x, a.y, c.x, c.y);
    }
    maxW = max(maxW, maxCw >> 24);
}

constexpr uint32_t kIntegrateWavesMost = 5120; // waves that take blocks when there are many: five per SIMD
// The kernel's one argument.  The pass that frees a block (a handful of blocks per frame, one lane each) wants a dozen
// table pointers and sizes that nothing else in the kernel needs; as ordinary kernel arguments they are loaded at the top
// of the kernel and kept in scalar registers throughout -- or, as measured, parked in scratch memory by every wave of
// the launch (4.5 MB of stores per launch at cfg2).  cold_args() hands that pass the argument block as memory the
// compiler knows nothing about, so it loads what it needs where it needs it.
struct FusedArgs {
    VhHashData hd;
    VhHashParams hp;
    VhDepthCameraData cam;
    VhDepthCameraParams cp;
    uint32_t flags;
    int32_t lockToken;
    uint32_t* countMirror;
    uint32_t mirrorTag;
    const uint2* packed;
};
// (host) the argument block from its parts: the launchers' scene arguments, or a VhFrameJob's
inline FusedArgs fused_args(const VhHashData& hd, const VhHashParams& hp, const VhDepthCameraData& cam, const VhDepthCameraParams& cp,
                            uint32_t flags, int32_t lockToken, uint32_t* countMirror, uint32_t mirrorTag, const void* packedFrame)
{
    FusedArgs a;
    a.hd = hd; a.hp = hp; a.cam = cam; a.cp = cp;
    a.flags = flags; a.lockToken = lockToken; a.countMirror = countMirror; a.mirrorTag = mirrorTag;
    a.packed = reinterpret_cast<const uint2*>(packedFrame);
    return a;
}
// A rider waits for a flag another rider of the launch raises (rider_done): VH_RIDER_DONE_COUNTERS copies 128 bytes apart, set
// to a number that only grows (compared modulo 2^32).  An exit every wave reaches: after ~1 s of polling the wait gives up
// (never seen; the caller says so in the status words and the grid drains whatever happens).  Every lane of the wave calls it.
VHD bool rider_wait(const uint32_t* flags, uint32_t expected)
{
    const uint32_t* const flag = flags + (blockIdx.x % VH_RIDER_DONE_COUNTERS) * 32u;
    for (uint32_t polls = 0; polls < (1u << 22); polls++) {
        const uint32_t v = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // (the same word for every lane: one request)
        if ((int32_t)(v - expected) >= 0) return true;
        __builtin_amdgcn_s_sleep(4);
    }
    return false;
}
template <uint32_t KERNARG_OFFSET> // where the kernel's argument block holds the FusedArgs (0: it is the kernel's only argument)
VHD const FusedArgs* cold_args()
{
    typedef const char __attribute__((address_space(4))) * KernargPtr;
    KernargPtr p = (KernargPtr)__builtin_amdgcn_kernarg_segment_ptr() + KERNARG_OFFSET;
    asm volatile("" : "+s"(p));
    return (const FusedArgs*)p;
}
template <uint32_t KERNARG_OFFSET>
VHD bool free_block_cold(int ex, int ey, int ez, uint32_t lane) // every lane of the wave calls it
{
    const FusedArgs* a = cold_args<KERNARG_OFFSET>();
    const VhHashData hd = a->hd;
    const VhHashParams hp = a->hp;
    // (As a rider of k_compute_normals the pass frees blocks while that launch's splat workgroups read the table.  That needs no
    // order: the delete never moves an entry -- it overwrites the freed one with one 16-byte store, clears counters and unlinks --
    // and the splat reads every slot once, so it lists every live block, and the freed one or not.  Either is what the splat made
    // BEFORE the pass, in a launch of its own, always was for the ray cast that uses it: a freed block that is still listed
    // has all-zero voxels by then (weight 0: no sample reads it), see CoSplat.)
    return delete_hash_entry_element_wave(hd, hp, mki3(ex, ey, ez), a->lockToken, lane);
}

// the fused pass's shared memory (a kernel that carries the pass as a rider overlays it with its other riders')
template <bool PACKED>
struct FusedShared {
    float sMin[4];
    uint32_t sMax[4];
    int sFreed;
    __attribute__((aligned(16))) uint2 sTile[PACKED ? 256 / kWave : 1][PACKED ? kIntegrateTileRows * kIntegrateTileStride : 2];
};

// One block by one workgroup, a voxel pair per thread: the pass's shape for up to 2048 blocks (integrate_fused_body), and the
// pass as a rider of k_compute_normals (pass_rider_group).  q: the block's entry, b: its place in the list.
template <bool PACKED, uint32_t KERNARG_OFFSET, class Shared> // Shared: a FusedShared (its sMin, sMax, sFreed)
VHD void integrate_block_by_workgroup(const FusedArgs& args, Shared& sh, const int4 q, const uint32_t b, const float thr)
{
    const VhHashData& hd = args.hd;
    const VhHashParams& hp = args.hp;
    const uint32_t flags = args.flags;
    const uint32_t lane = lane_id();
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
#if defined(VH_KNOCKOUT) && VH_KNOCKOUT == 43 // measurement build: every workgroup's life in this shape, read by tools/integrate_stamps.py
    const uint32_t stampA = (uint32_t)__builtin_amdgcn_s_memrealtime();
    uint32_t stampB = 0u, stampFreed = 0u;
#endif
    const uint32_t t = threadIdx.x;
    const int ex = __builtin_amdgcn_readfirstlane(q.x), ey = __builtin_amdgcn_readfirstlane(q.y);
    const int ez = __builtin_amdgcn_readfirstlane(q.z), ptr = __builtin_amdgcn_readfirstlane(q.w);
    uint4* vp = reinterpret_cast<uint4*>(&hd.d_SDFBlocks[(uint32_t)ptr]) + t;
    uint4 raw = *vp;
    // voxel pair (2t, 2t+1): x = (2t)%8 (+1), y = (2t%64)/8, z = 2t/64
    const I3 p0 = mki3(ex * VH_SDF_BLOCK_SIZE + (int)((2u * t) & 7u), ey * VH_SDF_BLOCK_SIZE + (int)(((2u * t) & 63u) >> 3), ez * VH_SDF_BLOCK_SIZE + (int)((2u * t) >> 6));
    float minSdf = pinf();
    uint32_t maxW = 0u;
    integrate_pair<PACKED>(hp, args.cp, args.cam, args.packed, flags, p0, raw, minSdf, maxW);
#if defined(VH_KNOCKOUT) && VH_KNOCKOUT == 43
    asm volatile("" : "+v"(raw.x));
    stampB = (uint32_t)__builtin_amdgcn_s_memrealtime();
#endif
    if (flags & VH_FUSED_GC) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            minSdf = fminf(minSdf, __shfl_xor(minSdf, o));
            maxW = max(maxW, (uint32_t)__shfl_xor((int)maxW, o));
        }
        if (lane == 0) { sh.sMin[wave] = minSdf; sh.sMax[wave] = maxW; }
        __syncthreads();
        minSdf = fminf(fminf(sh.sMin[0], sh.sMin[1]), fminf(sh.sMin[2], sh.sMin[3]));
        maxW = max(max(sh.sMax[0], sh.sMax[1]), max(sh.sMax[2], sh.sMax[3]));
        const bool decide = (minSdf >= thr) || (maxW == 0u); // the same in every thread of the workgroup
        if (t == 0) hd.d_hashDecision[b] = decide ? 1 : 0;
        if (decide) {
            if (wave == 0u) {
                const bool f = free_block_cold<KERNARG_OFFSET>(ex, ey, ez, lane);
                if (lane == 0u) sh.sFreed = f ? 1 : 0;
            }
            __syncthreads();
            if (sh.sFreed != 0) raw = make_uint4(0u, 0u, 0u, 0u);
#if defined(VH_KNOCKOUT) && VH_KNOCKOUT == 43
            stampFreed = 1u + (uint32_t)sh.sFreed;
#endif
        }
    }
    *vp = raw;
#if defined(VH_KNOCKOUT) && VH_KNOCKOUT == 43
    if (t == 0) reinterpret_cast<uint4*>(hd.d_hashCompactified)[(hp.m_hashNumBuckets * VH_HASH_BUCKET_SIZE) / 2u + b] = make_uint4(stampA, stampB, (uint32_t)__builtin_amdgcn_s_memrealtime(), 0x57430000u | stampFreed);
#endif
}

// The pass in a launch of its own (k_integrate_fused), as a function of (workgroup index, number of workgroups).  As a rider of
// k_compute_normals it is pass_rider_group (below), which shares the workgroup-per-block code above.
template <bool PACKED, uint32_t KERNARG_OFFSET>
VHD void integrate_fused_body(const FusedArgs& args, const uint32_t groupIdx, const uint32_t numGroups, FusedShared<PACKED>& sh)
{
    const VhHashData& hd = args.hd;
    const VhHashParams& hp = args.hp;
    const VhDepthCameraData& cam = args.cam;
    const VhDepthCameraParams& cp = args.cp;
    const uint32_t flags = args.flags;
    uint32_t* const countMirror = args.countMirror;
    const uint32_t mirrorTag = args.mirrorTag;
    const uint2* const packed = args.packed;
    float (&sMin)[4] = sh.sMin;
    uint32_t (&sMax)[4] = sh.sMax;
    int& sFreed = sh.sFreed;
    auto& sTile = sh.sTile;
    const uint32_t lane = lane_id();
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const uint32_t nEntries = hp.m_hashNumBuckets * VH_HASH_BUCKET_SIZE;
    // the count and the entry this workgroup / wave would start with in one trip (the list is Ne entries long: reading
    // beyond the count is reading stale entries, which are not used)
    const uint32_t count = (uint32_t)hd.d_hashCompactifiedCounter[0];
    // first block of this wave when waves take blocks: the active waves fill whole workgroups (the others leave at
    // once and free their slot: a workgroup's LDS and registers are held until its last wave is done)
    const uint32_t wFirst = groupIdx * (256u / kWave) + wave;
    int4 qg = make_int4(0, 0, 0, 0), qw = make_int4(0, 0, 0, 0);
    uint4 boxw = make_uint4(0u, 0u, 0u, 0u); // the entry's second half: {offset, box, box, tag} (compactify_group)
    if (groupIdx < nEntries) qg = load_quad(&hd.d_hashCompactified[groupIdx]);
    if (wFirst < nEntries) {
        qw = load_quad(&hd.d_hashCompactified[wFirst]);
        if (PACKED) boxw = list_box<false>(&hd.d_hashCompactified[wFirst]);
    }
    // host-visible copy of the block count and the caller's tag (mapped pinned memory): replaces a per-frame
    // device->host copy, and lets the host see how far the device has come
    if (countMirror && groupIdx == 0 && threadIdx.x == 0) *reinterpret_cast<uint2*>(countMirror) = make_uint2(count, mirrorTag);
    const float thr = get_truncation(hp, cp.m_sensorDepthWorldMax);

    if (count <= numGroups) {
        // ---- one workgroup per block
        if (groupIdx < count) integrate_block_by_workgroup<PACKED, KERNARG_OFFSET>(args, sh, qg, groupIdx, thr);
        return;
    }

    // ---- one wave per block: the first min(count, 5120) waves (five per SIMD; the hardware deals workgroups to the
    // compute units evenly) take blocks w, w + 5120, ...: no SIMD gets more than a block or two above the mean.
    // Measured and dropped: ceil(count / rounds) waves with `rounds` blocks each (SIMDs with five waves finished 3 us
    // after those with four: 27 us for 8 600 blocks), and a ticket counter (agent-scope atomics on one address are
    // served at the memory side of the eight L2s, ~12 ns each: 165 us).
    const uint32_t nActive = min(min(count, kIntegrateWavesMost), numGroups * (256u / kWave));
    if (wFirst >= nActive) return;
#if defined(VH_KNOCKOUT) && VH_KNOCKOUT == 9 // measurement build: shader clock over one wave's lifetime
    const uint64_t stampC0 = __builtin_amdgcn_s_memtime(), stampR0 = __builtin_amdgcn_s_memrealtime();
    uint32_t stamps[6] = { 0u, 0u, 0u, 0u, 0u, 0u }, stampN = 0u; // per block: staged, voxels arrived, computed (two blocks)
#endif
    uint32_t b = wFirst, round = 0u;
    // this wave's place in the later rounds: the SIMD it sits on (unit g mod 256, wave of the workgroup) bit-reversed, then
    // the workgroup's turn on that unit -- a permutation of 0 .. 5119 whose every prefix is spread evenly over the SIMDs
    // (used as is when all 5 120 waves are active; with fewer waves, which happens below 5 120 blocks, there is one round)
    const uint32_t simdOfMachine = ((groupIdx & 255u) << 2) | wave; // (as a rider the workgroups sit elsewhere: the order is then only a permutation)
    const uint32_t scattered = nActive == kIntegrateWavesMost ? (__brev(simdOfMachine) >> 22) + (groupIdx >> 8) * 1024u : wFirst;
    int4 q = qw;
    uint4 qbox = boxw;
    uint2* tile = sTile[wave];
    const uint32_t tagNow = frame_tag(hp, cp);
    for (;;) {
        // What depends on the lane alone is formed again for every block (a dozen cheap instructions): hoisted out of the
        // loop it is a dozen registers that live through everything, and the compiler parks them in scratch memory.
        uint32_t lane = lane_id();
        asm volatile("" : "+v"(lane));
        const int lx = (int)((2u * lane) & 7u), ly = (int)((lane >> 2) & 7u), lz0 = (int)(lane >> 5);
        const int ex = __builtin_amdgcn_readfirstlane(q.x), ey = __builtin_amdgcn_readfirstlane(q.y);
        const int ez = __builtin_amdgcn_readfirstlane(q.z), ptr = __builtin_amdgcn_readfirstlane(q.w);
        uint4* vp = reinterpret_cast<uint4*>(&hd.d_SDFBlocks[(uint32_t)ptr]) + lane;
        uint4 raw[4];
#pragma unroll
        for (int j = 0; j < 4; j++) raw[j] = vp[j * kWave];
        const uint32_t boxA = (uint32_t)__builtin_amdgcn_readfirstlane((int)qbox.y), boxB = (uint32_t)__builtin_amdgcn_readfirstlane((int)qbox.z);
        const uint32_t boxTag = (uint32_t)__builtin_amdgcn_readfirstlane((int)qbox.w);
        // The wave's next block.  Rounds of nActive blocks; within a round the blocks go to the waves in an order that
        // scatters a partial last round over the compute units (workgroup g sits on unit g mod 256: with the plain order
        // w + round * nActive the first units get all of the last round's blocks -- 36 blocks against 32 at 8 600).
        round += 1u;
        const uint32_t bNext = round * nActive + scattered;
        const bool hasNext = scattered < nActive && bNext < count;
        if (hasNext) { // its entry (both halves) behind this block's voxels
            q = load_quad(&hd.d_hashCompactified[bNext]);
            if (PACKED) qbox = list_box<false>(&hd.d_hashCompactified[bNext]);
        }
        // (Requesting the next block's voxels here as well was measured: slower.  The waves do not wait for the stream --
        // the kernel is bound by instruction issue, ~1000 vector instructions per block at 4 cycles each.)

        float minSdf = pinf();
        uint32_t maxW = 0u;
        bool wrote = false; // the plain code has put the block back itself
#if defined(VH_KNOCKOUT) && VH_KNOCKOUT == 1 // measurement build: the voxel stream alone (read, write back)
        if (false) {
#else
        if (PACKED) {
#endif
            // A voxel's gather from the frame is one cache access per LANE -- 64 tag look-ups per wave instruction, the
            // bound of this shape before staging (1 cm voxels: 13 us of a 33 us launch).  So the block's screen
            // footprint is staged in LDS first, four image rows per load instruction (whole lines), while the voxel
            // loads are in flight.  The box comes with the block's entry (block_box, worked out by the compactify pass
            // for this very transform: the tag says so; a list made for another one goes through the plain code, every
            // voxel gathered from the frame).  A voxel that projects outside the staged box all the same is gathered
            // from the frame itself: the box decides where a pixel is read, never which.
            BlockBox bb;
            bb.x0 = boxA & 0xffffu; bb.y0 = boxA >> 16;
            bb.w = boxB & 0xffu; bb.h = (boxB >> 8) & 0xffu;
            bb.flags = boxTag == tagNow ? boxB >> 16 : 0u; // a box made for another transform: neither staged nor certified
            // (a box that does not fit this image -- it cannot come from block_box for this frame -- is not used)
            const bool staged = (bb.flags & VH_BOX_STAGED) != 0u && bb.w <= kIntegrateTile && bb.h <= kIntegrateTileRows && (bb.x0 & 1u) == 0u &&
                                bb.x0 + bb.w <= cp.m_imageWidth && bb.y0 + bb.h <= cp.m_imageHeight && (cp.m_imageWidth & 1u) == 0u;
            const uint32_t x0 = bb.x0, y0 = bb.y0;
            const uint32_t w = staged ? bb.w : 0u, h = staged ? bb.h : 0u;
            if (staged) {
                // lane -> (row r + lane / 16, pixels 2 (lane % 16) and + 1): four rows per load instruction.  An even image
                // width and an even x0 keep a pixel pair inside its row.
                const uint32_t col2 = (lane & 15u) * 2u, rowInQuad = lane >> 4;
                const uint4* src = reinterpret_cast<const uint4*>(packed + (size_t)(y0 + rowInQuad) * cp.m_imageWidth + x0 + col2);
                uint4* dst = reinterpret_cast<uint4*>(tile + rowInQuad * kIntegrateTileStride + col2);
                __builtin_amdgcn_wave_barrier(); // the previous block's reads of the tile are done (they fed its stores)
#pragma unroll 4
                for (uint32_t r = 0; r < h; r += 4u) {
                    if (r + rowInQuad < h && col2 < w) dst[(size_t)r * (kIntegrateTileStride / 2u)] = src[(size_t)r * (cp.m_imageWidth / 2u)];
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
#if !defined(VH_INTEGRATE_PLAIN) // (measurement / test builds: every block through the plain code)
            const bool certified = staged && (bb.flags & VH_BOX_CERTIFIED) != 0u && hp.m_truncation > 0.0f && hp.m_truncScale >= 0.0f;
#else
            const bool certified = false;
#endif
#if defined(VH_KNOCKOUT) && VH_KNOCKOUT == 9
            if (stampN < 6u) stamps[stampN++] = (uint32_t)__builtin_amdgcn_s_memrealtime(); // staged
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (stampN < 6u) stamps[stampN++] = (uint32_t)__builtin_amdgcn_s_memrealtime(); // voxels here
#endif
            if (__builtin_amdgcn_readfirstlane(certified ? 1 : 0) != 0) {
                integrate_block_certified(hp, cp, packed, tile, kIntegrateTileStride, x0, y0, w, h, ex, ey, ez, lane, flags, raw, minSdf, maxW);
#if defined(VH_KNOCKOUT) && VH_KNOCKOUT == 9
                asm volatile("" : "+v"(raw[3].x), "+v"(raw[0].x));
                if (stampN < 6u) stamps[stampN++] = (uint32_t)__builtin_amdgcn_s_memrealtime(); // computed
#endif
            } else {
                // The plain code, for the blocks without a certificate or a staged footprint (near the camera, behind it,
                // on the image's edge): a compact loop that takes its voxels from memory again and puts them back itself.
                // Unrolled and on the registers of the loads above it costs the whole kernel 30 registers and its
                // fifth wave per SIMD (measured: 99 against 65); the voxels are in the cache.
                wrote = true;
#pragma unroll 1
                for (int j = 0; j < 4; j++) {
                    const uint4 r = vp[j * kWave];
                    Vox v[2] = { unpack_vox(make_uint2(r.x, r.y)), unpack_vox(make_uint2(r.z, r.w)) };
#pragma unroll
                    for (int k = 0; k < 2; k++) {
                        uint32_t sx, sy;
                        float pz;
                        if (project_voxel(hp, cp, mki3(ex * VH_SDF_BLOCK_SIZE + lx + k, ey * VH_SDF_BLOCK_SIZE + ly, ez * VH_SDF_BLOCK_SIZE + 2 * j + lz0), sx, sy, pz)) {
                            const uint32_t tx = sx - x0, ty = sy - y0; // unsigned: a pixel left of / above the box wraps to a huge number
#if defined(VH_KNOCKOUT) && VH_KNOCKOUT == 2 // measurement build: projection only
                            v[k].cw ^= (tx + ty + __float_as_uint(pz)) & 1u;
#elif defined(VH_KNOCKOUT) && VH_KNOCKOUT == 3 // measurement build: projection + the pixel, no blend
                            const uint2 px = (tx < w && ty < h) ? tile[ty * kIntegrateTileStride + tx] : packed[sy * cp.m_imageWidth + sx];
                            v[k].cw ^= (px.x + px.y + __float_as_uint(pz)) & 1u;
#else
                            const uint2 px = (tx < w && ty < h) ? tile[ty * kIntegrateTileStride + tx] : packed[sy * cp.m_imageWidth + sx];
                            v[k] = apply_pixel(hp, px, pz, v[k]);
#endif
                        }
                    }
                    asm volatile("" : "+v"(v[0].sdf), "+v"(v[0].cw), "+v"(v[1].sdf), "+v"(v[1].cw)); // see integrate_pair
                    if (flags & VH_FUSED_STARVE) { v[0] = starve_voxel(v[0]); v[1] = starve_voxel(v[1]); }
                    minSdf = fminf(minSdf, fminf(gc_key(v[0]), gc_key(v[1])));
                    maxW = max(maxW, max(v[0].weight(), v[1].weight()));
                    const uint2 a = pack_vox(v[0]), c = pack_vox(v[1]);
                    vp[j * kWave] = make_uint4(a.x, a.y, c.x, c.y);
                }
            }
        } else {
#if !(defined(VH_KNOCKOUT) && VH_KNOCKOUT == 1)
#pragma unroll
            for (int j = 0; j < 4; j++)
                integrate_pair<PACKED>(hp, cp, cam, packed, flags, mki3(ex * VH_SDF_BLOCK_SIZE + lx, ey * VH_SDF_BLOCK_SIZE + ly, ez * VH_SDF_BLOCK_SIZE + 2 * j + lz0),
                                       raw[j], minSdf, maxW);
#endif
        }
        bool freed = false;
        if (flags & VH_FUSED_GC) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                minSdf = fminf(minSdf, __shfl_xor(minSdf, o));
                maxW = max(maxW, (uint32_t)__shfl_xor((int)maxW, o));
            }
            const bool decide = (minSdf >= thr) || (maxW == 0u);
            if (lane == 0) hd.d_hashDecision[b] = decide ? 1 : 0;
            // (the same decision in every lane: the reduction left every lane with the block's minimum and maximum)
            if (__builtin_amdgcn_readfirstlane(decide ? 1 : 0) != 0) freed = free_block_cold<KERNARG_OFFSET>(ex, ey, ez, lane);
        }
        if (freed) {
#pragma unroll
            for (int j = 0; j < 4; j++) vp[j * kWave] = make_uint4(0u, 0u, 0u, 0u);
        } else if (!wrote) {
#pragma unroll
            for (int j = 0; j < 4; j++) vp[j * kWave] = raw[j];
        }
        if (!hasNext) break;
        b = bNext;
    }
#if defined(VH_KNOCKOUT) && VH_KNOCKOUT == 9
    if (wFirst == 0u && lane == 0u) {
        const uint64_t c = __builtin_amdgcn_s_memtime() - stampC0, r = __builtin_amdgcn_s_memrealtime() - stampR0;
        hd.d_state[8] = (uint32_t)c; hd.d_state[9] = (uint32_t)r; hd.d_state[10] = (count + nActive - 1u) / nActive; hd.d_state[11] = nActive;
    }
    if (lane == 0u) { // every wave's life in the unused upper half of the compactified list: {start, end (100 MHz ticks), hardware id, xcc id}
        const uint32_t hwid = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);
        reinterpret_cast<uint4*>(hd.d_hashCompactified)[nEntries / 2u + 3u * wFirst] =
            make_uint4((uint32_t)stampR0, (uint32_t)__builtin_amdgcn_s_memrealtime(), hwid, xcc);
        reinterpret_cast<uint4*>(hd.d_hashCompactified)[nEntries / 2u + 3u * wFirst + 1u] = make_uint4(stamps[0], stamps[1], stamps[2], stamps[3]);
        reinterpret_cast<uint4*>(hd.d_hashCompactified)[nEntries / 2u + 3u * wFirst + 2u] = make_uint4(stamps[4], stamps[5], 0u, 0u);
    }
#endif
}

template <bool PACKED>
__global__ __launch_bounds__(256)
void k_integrate_fused(FusedArgs args)
{
    __shared__ FusedShared<PACKED> sh;
    integrate_fused_body<PACKED, 0u>(args, blockIdx.x, gridDim.x, sh);
}
// the fused pass's grid for a pool (host).  Persistent: the count lives on the device, the kernel picks its shape from it
inline uint32_t fused_pass_groups(const VhHashParams& hp, uint32_t numCUs) { const uint32_t want = cdiv(hp.m_numSDFBlocks, 4), most = numCUs * 8u; return want < most ? want : most; }

__global__ __launch_bounds__(256) void k_starve(VhHashData hd, VhHashParams hp)
{
    const uint32_t b = blockIdx.x;
    if (b >= hp.m_numOccupiedBlocks) return;
    const int ptr = __builtin_amdgcn_readfirstlane(load_quad(&hd.d_hashCompactified[b]).w);
    uint4* vp = reinterpret_cast<uint4*>(&hd.d_SDFBlocks[(uint32_t)ptr]) + threadIdx.x;
    uint4 raw = *vp;
    Vox v0 = starve_voxel(unpack_vox(make_uint2(raw.x, raw.y))), v1 = starve_voxel(unpack_vox(make_uint2(raw.z, raw.w)));
    raw.y = v0.cw; raw.w = v1.cw;
    *vp = raw;
}

__global__ __launch_bounds__(256) void k_gc_identify(VhHashData hd, VhHashParams hp, VhDepthCameraParams cp)
{
    __shared__ float sMin[4];
    __shared__ uint32_t sMax[4];
    const uint32_t b = blockIdx.x;
    if (b >= hp.m_numOccupiedBlocks) return;
    const int ptr = __builtin_amdgcn_readfirstlane(load_quad(&hd.d_hashCompactified[b]).w);
    const uint4 raw = *(reinterpret_cast<const uint4*>(&hd.d_SDFBlocks[(uint32_t)ptr]) + threadIdx.x);
    const Vox v0 = unpack_vox(make_uint2(raw.x, raw.y)), v1 = unpack_vox(make_uint2(raw.z, raw.w));
    float minSdf = fminf(gc_key(v0), gc_key(v1));
    uint32_t maxW = max(v0.weight(), v1.weight());
    block_min_max(minSdf, maxW, sMin, sMax);
    if (threadIdx.x == 0) {
        const float thr = get_truncation(hp, cp.m_sensorDepthWorldMax);
        hd.d_hashDecision[b] = ((minSdf >= thr) || (maxW == 0u)) ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void k_gc_free(VhHashData hd, VhHashParams hp, int32_t lockToken)
{
    __shared__ int sFreed;
    const uint32_t b = blockIdx.x;
    if (b >= hp.m_numOccupiedBlocks) return;
    if (hd.d_hashDecision[b] == 0) return; // block-uniform
    const int4 q = load_quad(&hd.d_hashCompactified[b]);
    if (threadIdx.x == 0) sFreed = delete_hash_entry_element(hd, hp, mki3(q.x, q.y, q.z), lockToken) ? 1 : 0;
    __syncthreads();
    if (sFreed) {
        const int ptr = __builtin_amdgcn_readfirstlane(q.w);
        *(reinterpret_cast<uint4*>(&hd.d_SDFBlocks[(uint32_t)ptr]) + threadIdx.x) = make_uint4(0u, 0u, 0u, 0u);
    }
}

} // namespace
