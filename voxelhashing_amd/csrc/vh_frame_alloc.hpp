// vh_frame_alloc.hpp -- frame loop, first stage: the reset kernels, and alloc (alloc_tile, k_alloc) with the frame it
// packs for the integrate pass (pack_pixel).  Included by vh_frame_integrate.hpp (the pass reads the packed frame)
// and by vh_ray_tiles.hpp, where k_render carries alloc_tile as a rider (CoAlloc).
#pragma once

#include "vh_device.hpp"

namespace {
using namespace vhd;

// ---------------------------------------------------------------------------
// reset (resetHeapKernel / resetHashKernel / resetHashBucketMutexKernel,
// DSC/CUDASceneRepHashSDF.cu:23-61).  Voxels and summaries are cleared with
// hipMemsetAsync; these kernels write the non-zero patterns, 16 B per lane.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_reset_heap(uint32_t* heap, uint32_t* heapCounter, uint32_t n)
{
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx == 0) heapCounter[0] = n - 1;
    if (idx < n) heap[idx] = n - idx - 1;
}

__global__ __launch_bounds__(256) void k_reset_hash(VhHashEntry* a, VhHashEntry* b, uint32_t ne)
{
    // one 16-byte half-entry per lane: even lanes {0,0,0,FREE}, odd lanes {offset=0,pad}
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < 2ull * ne) {
        const int4 v = (idx & 1) ? make_int4(0, 0, 0, 0) : make_int4(0, 0, 0, VH_FREE_ENTRY);
        reinterpret_cast<int4*>(a)[idx] = v;
        reinterpret_cast<int4*>(b)[idx] = v;
    }
}

__global__ __launch_bounds__(256) void k_fill_i32(int32_t* p, int32_t v, uint32_t n)
{
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n) p[idx] = v;
}

// ---------------------------------------------------------------------------
// alloc (allocKernel, DSC/CUDASceneRepHashSDF.cu:158-243)
//
// One wave per 8x8 pixel tile.  Each lane walks its ray's SDF blocks with the
// reference's DDA; at every step the wave de-duplicates the block ids its
// lanes ask for (neighbouring rays hit the same 8^3 block) and ONE lane probes
// the table per distinct id, so the table sees ~1/64 of the reference's probes.
// ---------------------------------------------------------------------------

// What integrateDepthMapKernel reads of a pixel (DSC/CUDASceneRepHashSDF.cu:436-470), formed once per pixel instead
// of once per voxel that projects onto it: the depth, the colour as the bytes the kernel would make of it
// (uchar(255 * c), :466) and the weight of the sample (:463-464, a function of the depth alone).  Weight 0 marks a
// pixel that integrates nothing: invalid depth or colour, or beyond the integration distance (:443-445); a valid
// sample weighs at least 1.
VHD uint2 pack_pixel(const VhHashParams& hp, const VhDepthCameraParams& cp, float depth, bool hasColor, float4 c)
{
    uint32_t cw = 0u;
    if (hasColor && c.x != minf() && depth != minf() && depth < hp.m_maxIntegrationDistance) {
        const float depthZeroOne = cam_to_proj_z(cp, depth);
        const float weightUpdate = fmaxf((float)hp.m_integrationWeightSample * 1.5f * (1.0f - depthZeroOne), 1.0f);
        cw = pack_cw(f2uc(255.0f * c.x), f2uc(255.0f * c.y), f2uc(255.0f * c.z), f2uc(weightUpdate));
    }
    return make_uint2(__float_as_uint(depth), cw);
}

// one wave, one 8x8 pixel tile
VHD void alloc_tile(const VhHashData& hd, const VhHashParams& hp, const VhDepthCameraData& cam, const VhDepthCameraParams& cp,
                    const uint32_t* bitMask, int32_t lockToken, HashMod hm, uint2* packed, uint32_t tile)
{
    const uint32_t lane = lane_id();
    const uint32_t W = cp.m_imageWidth, H = cp.m_imageHeight;
    const uint32_t tilesX = (W + 7) / 8, tilesY = (H + 7) / 8;
    if (tile >= tilesX * tilesY) return; // wave-uniform
    const uint32_t x = (tile % tilesX) * 8 + (lane & 7), y = (tile / tilesX) * 8 + (lane >> 3);
    const float vs = hp.m_virtualVoxelSize;

    bool active = (x < W) && (y < H);
    float d = active ? cam.d_depthData[y * W + x] : minf();
    if (packed && active) { // the frame as the integrate pass reads it (a 128-byte row segment per 8 lanes)
        float4 c = make_float4(minf(), minf(), minf(), minf());
        if (cam.d_colorData) c = reinterpret_cast<const float4*>(cam.d_colorData)[y * W + x];
        packed[y * W + x] = pack_pixel(hp, cp, d, cam.d_colorData != nullptr, c);
    }
    if (d == minf() || d == 0.0f) active = false;
    if (d >= hp.m_maxIntegrationDistance) active = false;
    const float t = get_truncation(hp, d);
    const float minDepth = fminf(hp.m_maxIntegrationDistance, d - t);
    const float maxDepth = fminf(hp.m_maxIntegrationDistance, d + t);
    if (minDepth >= maxDepth) active = false;
    if (!__any(active)) return; // a tile without a measurement

    const F3 rayMin = mat_mul_p(hp.m_rigidTransform, depth_to_skeleton(cp, x, y, minDepth));
    const F3 rayMax = mat_mul_p(hp.m_rigidTransform, depth_to_skeleton(cp, x, y, maxDepth));
    const F3 rayDir = normalize3(mk3(rayMax.x - rayMin.x, rayMax.y - rayMin.y, rayMax.z - rayMin.z));

    // (world_to_block with the division by the voxel size as div_exact: five vector instructions instead of eleven, the same
    // quotient bit for bit -- tests/test_gpu_parity.py::test_exact_shortcuts; the ray caster's tap coordinates do the same)
    const float rvs = 1.0f / vs;
    I3 id = vvp_to_block(mki3(world_to_vvp1_rb(rayMin.x, vs, rvs), world_to_vvp1_rb(rayMin.y, vs, rvs), world_to_vvp1_rb(rayMin.z, vs, rvs)));
    const I3 idEnd = vvp_to_block(mki3(world_to_vvp1_rb(rayMax.x, vs, rvs), world_to_vvp1_rb(rayMax.y, vs, rvs), world_to_vvp1_rb(rayMax.z, vs, rvs)));

    const F3 step = mk3((float)signi(rayDir.x), (float)signi(rayDir.y), (float)signi(rayDir.z));
    const I3 cl = mki3(f2i(fmaxf(0.0f, fminf(step.x, 1.0f))), f2i(fmaxf(0.0f, fminf(step.y, 1.0f))), f2i(fmaxf(0.0f, fminf(step.z, 1.0f))));
    F3 boundaryPos = block_to_world(vs, mki3(id.x + cl.x, id.y + cl.y, id.z + cl.z));
    const float half = 0.5f * vs;
    boundaryPos.x -= half; boundaryPos.y -= half; boundaryPos.z -= half;
    F3 tMax = mk3((boundaryPos.x - rayMin.x) / rayDir.x, (boundaryPos.y - rayMin.y) / rayDir.y, (boundaryPos.z - rayMin.z) / rayDir.z);
    F3 tDelta = mk3((step.x * (float)VH_SDF_BLOCK_SIZE * vs) / rayDir.x, (step.y * (float)VH_SDF_BLOCK_SIZE * vs) / rayDir.y,
                    (step.z * (float)VH_SDF_BLOCK_SIZE * vs) / rayDir.z);
    const I3 idBound = mki3(f2i((float)idEnd.x + step.x), f2i((float)idEnd.y + step.y), f2i((float)idEnd.z + step.z));

    if (rayDir.x == 0.0f) { tMax.x = pinf(); tDelta.x = pinf(); }
    if (boundaryPos.x - rayMin.x == 0.0f) { tMax.x = pinf(); tDelta.x = pinf(); }
    if (rayDir.y == 0.0f) { tMax.y = pinf(); tDelta.y = pinf(); }
    if (boundaryPos.y - rayMin.y == 0.0f) { tMax.y = pinf(); tDelta.y = pinf(); }
    if (rayDir.z == 0.0f) { tMax.z = pinf(); tDelta.z = pinf(); }
    if (boundaryPos.z - rayMin.z == 0.0f) { tMax.z = pinf(); tDelta.z = pinf(); }

    uint32_t iter = 0;
    while (__any(active)) {
        // Steady state: the block exists and sits in the first slot of its bucket.  Every lane checks that for
        // its own block with ONE load (all lanes in flight together); only the rest -- new blocks and blocks
        // further down a bucket -- goes through the serial allocBlock below.  The reference asks "in the frustum?
        // not streamed out?" first; the tests are independent and a block that exists needs nothing, so the cheap
        // one goes first and the projection runs only for a block that is not where it is expected.
        bool want = active;
        if (want) {
            const int4 q0 = load_quad(&hd.d_hash[hash_pos_fast(hm, id) * VH_HASH_BUCKET_SIZE]);
            want = !quad_matches(q0, id);
        }
        if (want) want = block_in_frustum(hp, cp, id) && !block_streamed_out(hp, id, bitMask);
        // wave-level de-duplication of the requested block ids: one lane per distinct id, and those lanes allocate
        // side by side -- the chain lock -> heap counter -> heap slot -> entry is four trips to memory, walked once
        // for all the new blocks of this step instead of once per block
        uint64_t pending = __ballot(want);
        bool leads = false;
        while (pending) {
            const int leader = __ffsll((unsigned long long)pending) - 1;
            const int bx = __builtin_amdgcn_readlane(id.x, leader);
            const int by = __builtin_amdgcn_readlane(id.y, leader);
            const int bz = __builtin_amdgcn_readlane(id.z, leader);
            const bool same = want && id.x == bx && id.y == by && id.z == bz;
            pending &= ~__ballot(same);
            leads = leads || (int)lane == leader;
        }
        if (leads) alloc_block(hd, hp, id, lockToken);
        if (active) {
            if (tMax.x < tMax.y && tMax.x < tMax.z) {
                id.x = f2i((float)id.x + step.x);
                if (id.x == idBound.x) active = false;
                tMax.x += tDelta.x;
            } else if (tMax.z < tMax.y) {
                id.z = f2i((float)id.z + step.z);
                if (id.z == idBound.z) active = false;
                tMax.z += tDelta.z;
            } else {
                id.y = f2i((float)id.y + step.y);
                if (id.y == idBound.y) active = false;
                tMax.y += tDelta.y;
            }
            iter++;
            if (iter >= 1024u) active = false;
        }
    }
}

__global__ __launch_bounds__(512) void k_alloc(VhHashData hd, VhHashParams hp, VhDepthCameraData cam,
                                               VhDepthCameraParams cp, const uint32_t* bitMask, int32_t lockToken, HashMod hm, uint2* packed)
{
    // the compaction that follows needs its counter at zero: cleared here instead of by a separate memset
    if (blockIdx.x == 0 && threadIdx.x == 0) hd.d_hashCompactifiedCounter[0] = 0;
    alloc_tile(hd, hp, cam, cp, bitMask, lockToken, hm, packed, blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave));
}
constexpr uint32_t kAllocThreads = 512; // k_alloc's launch shape (host): eight tiles a workgroup (as a rider: co_alloc_groups)
inline uint32_t alloc_groups(uint32_t tiles) { return cdiv(tiles, kAllocThreads / kWave); }

} // namespace
