// vh_kernels.hip -- the frame loop's kernels: reset, alloc, compactify, integrate, garbage collection, the interval
// splat, the ray caster, the queries and normals, with their launcher-level C ABI (include/vh_api.h).  They are one
// translation unit because they ride on one another: k_render carries alloc, and k_compute_normals carries compactify,
// the splat and integrate, so those device functions must be visible together.  None of them is defined in this file:
// they are written a stage to a header (vh_frame_*.hpp) and the ray caster a part to a header (vh_ray_*.hpp: the block
// lookups, the sample, the march, the queries, the tile ray caster), included below in their order of definition; a
// header's includes say on whom it stands or rides.  What is here is host code: the device's compute units and the
// launchers.  The checks of integrate's arithmetic (k_check_refined_division, k_check_weighted_colour) stay with the
// functions they check, and k_debug_hash_ops with the kernels whose hash operations it runs one by one.  What shares only
// vh_device.hpp with the frame loop has a unit of its own: vh_image.hip, vh_streaming.hip, vh_mc.hip, vh_util.hip.
// A stage's launch shape is a host function beside its kernel; the launchers, whether they launch the stage alone or as
// a rider, call it.  The schedule buffer's size is such a function too (schedule_words, beside schedule_tiles).
//
// Reference behaviour: DSC/CUDASceneRepHashSDF.cu, DSC/CUDARayCastSDF.cu, DSC/RayCastSDFUtil.h, DSC/CameraUtil.cu:669-711
// (DSC/ = DepthSensingCUDA/Source/ of the reference).  Nothing here is derived from those kernels' structure: launch
// shapes, data movement and intra-wave cooperation are designed for CDNA4 (wave64, 16-byte lanes, no textures, no
// __constant__ singletons, no host round trips).
// MUST be compiled with -ffp-contract=off (see vh_device.hpp).
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/vh_api.h"
#include "vh_device.hpp"
#include "vh_host_util.hpp"

using namespace vhd;

#include "vh_frame_alloc.hpp"
#include "vh_frame_compactify.hpp"
#include "vh_frame_integrate.hpp"
#include "vh_frame_splat.hpp"
#include "vh_ray_lookup.hpp"
#include "vh_ray_sample.hpp"
#include "vh_ray_march.hpp"
#include "vh_ray_query.hpp"
#include "vh_ray_tiles.hpp"
#include "vh_frame_normals.hpp"
#include "vh_frame_checks.hpp"

// ---------------------------------------------------------------------------
// launcher-level C ABI
// ---------------------------------------------------------------------------

static uint32_t device_num_cus() // of the current device (one device per process: INTEGRATION.md)
{
    static int numCUs = 0;
    if (numCUs == 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&numCUs, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || numCUs <= 0)
            numCUs = 256;
    }
    return (uint32_t)numCUs;
}
static uint32_t schedule_num_cus(const uint32_t* d_schedule) { return d_schedule ? device_num_cus() : 256u; } // (no schedule: the device is not asked)

extern "C" {

int vh_reset(const VhHashData* hd, const VhHashParams* hp, vhStream_t stream)
{
    if (!hd || !hp || !hd->d_hash) return VH_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t nb = hp->m_hashNumBuckets, ne = nb * VH_HASH_BUCKET_SIZE, nblk = hp->m_numSDFBlocks;
    VH_HIP(hipMemsetAsync(hd->d_SDFBlocks, 0, sizeof(VhVoxel) * (size_t)nblk * VH_SDF_BLOCK_VOXELS, s));
    VH_HIP(hipMemsetAsync(hd->d_bucketCount, 0, sizeof(uint32_t) * nb, s));
    VH_HIP(hipMemsetAsync(hd->d_bucketBits, 0, sizeof(uint32_t) * ((nb + 31) / 32), s));
    VH_HIP(hipMemsetAsync(hd->d_state, 0, sizeof(uint32_t) * VH_STATE_WORDS, s));
    VH_HIP(hipMemsetAsync(hd->d_hashDecision, 0, sizeof(int32_t) * ne, s));
    VH_HIP(hipMemsetAsync(hd->d_hashCompactifiedCounter, 0, sizeof(int32_t), s));
    k_reset_heap<<<cdiv(nblk, 256), 256, 0, s>>>(hd->d_heap, hd->d_heapCounter, nblk);
    k_reset_hash<<<cdiv(2ull * ne, 256), 256, 0, s>>>(hd->d_hash, hd->d_hashCompactified, ne);
    k_fill_i32<<<cdiv(nb, 256), 256, 0, s>>>(hd->d_hashBucketMutex, VH_FREE_ENTRY, nb);
    return vh_last_launch_error();
}

int vh_reset_bucket_mutex(const VhHashData* hd, const VhHashParams* hp, vhStream_t stream)
{
    if (!hd || !hp) return VH_ERR_BAD_ARGUMENT;
    k_fill_i32<<<cdiv(hp->m_hashNumBuckets, 256), 256, 0, (hipStream_t)stream>>>(hd->d_hashBucketMutex, VH_FREE_ENTRY, hp->m_hashNumBuckets);
    return vh_last_launch_error();
}

int vh_alloc(const VhHashData* hd, const VhHashParams* hp, const VhDepthCameraData* cam,
             const VhDepthCameraParams* cp, const uint32_t* d_bitMask, int32_t lockToken, vhStream_t stream)
{
    if (!hd || !hp || !cam || !cp || !cam->d_depthData) return VH_ERR_BAD_ARGUMENT;
    const uint32_t tiles = image_tiles(cp->m_imageWidth, cp->m_imageHeight);
    if (tiles == 0) return VH_OK;
    if (hp->m_hashNumBuckets < 2) return VH_ERR_BAD_ARGUMENT;
    k_alloc<<<alloc_groups(tiles), kAllocThreads, 0, (hipStream_t)stream>>>(*hd, *hp, *cam, *cp, d_bitMask, lockToken, make_hash_mod(hp->m_hashNumBuckets), nullptr);
    return vh_last_launch_error();
}

int vh_alloc_job(VhFrameJob* job, vhStream_t stream)
{
    if (!job || !job->cam.d_depthData || !job->hashData.d_hash) return VH_ERR_BAD_ARGUMENT;
    const uint32_t tiles = image_tiles(job->cp.m_imageWidth, job->cp.m_imageHeight);
    if (job->hashParams.m_hashNumBuckets < 2) return VH_ERR_BAD_ARGUMENT;
    job->allocLaunched = 1;
    if (tiles == 0) return VH_OK;
    k_alloc<<<alloc_groups(tiles), kAllocThreads, 0, (hipStream_t)stream>>>(job->hashData, job->hashParams, job->cam, job->cp, job->d_bitMask, job->lockToken,
                                                                            make_hash_mod(job->hashParams.m_hashNumBuckets), reinterpret_cast<uint2*>(job->d_packedFrame));
    return vh_last_launch_error();
}

int vh_compactify_job(VhFrameJob* job, vhStream_t stream)
{
    if (!job || !job->hashData.d_hash) return VH_ERR_BAD_ARGUMENT;
    job->compactifyLaunched = 1;
    k_compactify<<<compactify_groups(job->hashParams), kCompactifyThreads, 0, (hipStream_t)stream>>>(job->hashData, job->hashParams, job->cp);
    return vh_last_launch_error();
}

int vh_compactify(const VhHashData* hd, const VhHashParams* hp, const VhDepthCameraParams* cp,
                  uint32_t* numOccupied, uint32_t flags, vhStream_t stream)
{
    if (!hd || !hp || !cp) return VH_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    if (!(flags & VH_COMPACT_COUNTER_IS_ZERO)) VH_HIP(hipMemsetAsync(hd->d_hashCompactifiedCounter, 0, sizeof(int32_t), s));
    k_compactify<<<compactify_groups(*hp), kCompactifyThreads, 0, s>>>(*hd, *hp, *cp);
    int err = vh_last_launch_error();
    if (err) return err;
    if (numOccupied) {
        VH_HIP(hipMemcpyAsync(numOccupied, hd->d_hashCompactifiedCounter, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        VH_HIP(hipStreamSynchronize(s));
    }
    return VH_OK;
}

int vh_integrate(const VhHashData* hd, const VhHashParams* hp, const VhDepthCameraData* cam,
                 const VhDepthCameraParams* cp, vhStream_t stream)
{
    if (!hd || !hp || !cam || !cp || !cam->d_depthData) return VH_ERR_BAD_ARGUMENT;
    if (hp->m_numOccupiedBlocks == 0) return VH_OK; // DSC/CUDASceneRepHashSDF.cu:501
    // (a timed launch: this kernel is the yardstick of tools/bench_deintegrate.py)
    VH_LAUNCH_TIMED(k_integrate<false>, hp->m_numOccupiedBlocks, 256, (hipStream_t)stream, *hd, *hp, *cam, *cp, 0u, VH_LOCK_ENTRY, nullptr);
    return vh_last_launch_error();
}

int vh_integrate_fused(const VhHashData* hd, const VhHashParams* hp, const VhDepthCameraData* cam,
                       const VhDepthCameraParams* cp, uint32_t flags, int32_t lockToken, uint32_t* d_countMirror, uint32_t mirrorTag,
                       const void* d_packedFrame, vhStream_t stream)
{
    if (!hd || !hp || !cam || !cp || !cam->d_depthData) return VH_ERR_BAD_ARGUMENT;
    if (cp->m_imageWidth > 0xffffu || cp->m_imageHeight > 0xffffu) return VH_ERR_BAD_ARGUMENT;
    const uint32_t grid = fused_pass_groups(*hp, device_num_cus());
    const FusedArgs args = fused_args(*hd, *hp, *cam, *cp, flags, lockToken, d_countMirror, mirrorTag, d_packedFrame);
    if (args.packed) VH_LAUNCH_TIMED(k_integrate_fused<true>, grid, 256, (hipStream_t)stream, args);
    else VH_LAUNCH_TIMED(k_integrate_fused<false>, grid, 256, (hipStream_t)stream, args);
    return vh_last_launch_error();
}

int vh_starve(const VhHashData* hd, const VhHashParams* hp, vhStream_t stream)
{
    if (!hd || !hp) return VH_ERR_BAD_ARGUMENT;
    if (hp->m_numOccupiedBlocks == 0) return VH_OK;
    k_starve<<<hp->m_numOccupiedBlocks, 256, 0, (hipStream_t)stream>>>(*hd, *hp);
    return vh_last_launch_error();
}

int vh_gc_identify(const VhHashData* hd, const VhHashParams* hp, const VhDepthCameraParams* cp, vhStream_t stream)
{
    if (!hd || !hp || !cp) return VH_ERR_BAD_ARGUMENT;
    if (hp->m_numOccupiedBlocks == 0) return VH_OK;
    k_gc_identify<<<hp->m_numOccupiedBlocks, 256, 0, (hipStream_t)stream>>>(*hd, *hp, *cp);
    return vh_last_launch_error();
}

int vh_gc_free(const VhHashData* hd, const VhHashParams* hp, int32_t lockToken, vhStream_t stream)
{
    if (!hd || !hp) return VH_ERR_BAD_ARGUMENT;
    if (hp->m_numOccupiedBlocks == 0) return VH_OK;
    k_gc_free<<<hp->m_numOccupiedBlocks, 256, 0, (hipStream_t)stream>>>(*hd, *hp, lockToken);
    return vh_last_launch_error();
}

int vh_bind_input_depth_color_textures(const VhDepthCameraData* cam)
{
    (void)cam;
    return VH_OK;
}

int vh_render(const VhHashData* hd, const VhHashParams* hp, const VhRayCastData* rd,
              const VhDepthCameraParams* cp, const VhRayCastParams* rp, vhStream_t stream)
{
    if (!hd || !hp || !rd || !cp || !rp || !rd->d_depth) return VH_ERR_BAD_ARGUMENT;
    const uint32_t tiles = image_tiles(rp->m_width, rp->m_height);
    if (tiles == 0) return VH_OK;
    if (hp->m_hashNumBuckets < 2) return VH_ERR_BAD_ARGUMENT;
    const HashMod hm = make_hash_mod(hp->m_hashNumBuckets);
    if (rp->m_useGradients) VH_LAUNCH_TIMED(k_render_hash<true>, render_hash_groups(tiles), 256, (hipStream_t)stream, *hd, *hp, *rd, *cp, *rp, hm);
    else VH_LAUNCH_TIMED(k_render_hash<false>, render_hash_groups(tiles), 256, (hipStream_t)stream, *hd, *hp, *rd, *cp, *rp, hm);
    return vh_last_launch_error();
}

int vh_query_points(const VhHashData* hd, const VhHashParams* hp, const float* d_points3, uint32_t n, float* d_sdf, uint32_t* d_color,
                    float* d_gradient3, uint8_t* d_valid, vhStream_t stream)
{
    if (!hd || !hp || !hd->d_hash || !d_points3 || !d_sdf || !d_color || !d_valid) return VH_ERR_BAD_ARGUMENT;
    if (hp->m_hashNumBuckets < 2) return VH_ERR_BAD_ARGUMENT;
    if (n == 0) return VH_OK;
    const HashMod hm = make_hash_mod(hp->m_hashNumBuckets);
    VH_LAUNCH_TIMED(k_query_points, cdiv(n, 256), 256, (hipStream_t)stream, *hd, *hp, d_points3, n, d_sdf, d_color, d_gradient3, d_valid, hm);
    return vh_last_launch_error();
}

int vh_query_rays(const VhHashData* hd, const VhHashParams* hp, const VhRayCastParams* rp, const float* d_origins3, const float* d_directions3,
                  const float* d_tMin, const float* d_tMax, uint32_t n, float* d_t, float* d_normals3, uint32_t* d_color, uint8_t* d_status,
                  vhStream_t stream)
{
    if (!hd || !hp || !rp || !hd->d_hash || !d_origins3 || !d_directions3 || !d_tMin || !d_tMax || !d_t || !d_color || !d_status)
        return VH_ERR_BAD_ARGUMENT;
    if (!std::isfinite(rp->m_rayIncrement) || !(rp->m_rayIncrement > 0.0f)) return VH_ERR_BAD_ARGUMENT;
    if (hp->m_hashNumBuckets < 2) return VH_ERR_BAD_ARGUMENT;
    if (n == 0) return VH_OK;
    const HashMod hm = make_hash_mod(hp->m_hashNumBuckets);
    VH_LAUNCH_TIMED(k_query_rays, cdiv(n, 256), 256, (hipStream_t)stream, *hd, *hp, rp->m_rayIncrement, rp->m_thresSampleDist, rp->m_thresDist,
                    d_origins3, d_directions3, d_tMin, d_tMax, n, d_t, d_normals3, d_color, d_status, hm);
    return vh_last_launch_error();
}

size_t vh_render_schedule_bytes(uint32_t width, uint32_t height)
{
    const uint32_t tiles = image_tiles(width, height);
    return schedule_words(tiles, render_groups_most(tiles)) * sizeof(uint32_t); // (slots for as many split tiles as any image has)
}

uint32_t vh_render_split_tiles(uint32_t width, uint32_t height) { return split_tiles(image_tiles(width, height)); }

static std::atomic<int> g_forceOffsets64{ 0 };

uint32_t vh_render_offsets32(uint32_t numSDFBlocks) { return (!g_forceOffsets64.load(std::memory_order_relaxed) && offsets32_ok(numSDFBlocks)) ? 1u : 0u; }

uint32_t vh_debug_render_force_offsets64(uint32_t on) { return (uint32_t)g_forceOffsets64.exchange(on ? 1 : 0, std::memory_order_relaxed); }

int vh_render_intervals_co(const VhHashData* hd, const VhHashParams* hp, const VhRayCastData* rd, const VhDepthCameraParams* cp,
                           const VhRayCastParams* rp, uint32_t* d_tileHeads, const VhTileBlock* d_tileBlocks, uint32_t tileCapacity,
                           uint32_t* d_schedule, uint32_t phase, VhFrameJob* fj, vhStream_t stream)
{
    if (!hd || !hp || !rd || !cp || !rp || !rd->d_depth || !d_tileHeads) return VH_ERR_BAD_ARGUMENT;
    const uint32_t tiles = image_tiles(rp->m_width, rp->m_height);
    if (tiles == 0) return VH_OK;
    uint4* h = reinterpret_cast<uint4*>(d_tileHeads);
    const int4* l = reinterpret_cast<const int4*>(d_tileBlocks);
    const uint32_t cap = d_tileBlocks ? tileCapacity : 0u;
    // the capacity of the lists picks the table size: up to VH_TILE_LIST_CAPACITY the small tables, beyond it the large ones
    const bool large = cap > (uint32_t)VH_TILE_LIST_CAPACITY;
    uint32_t groups = render_groups(tiles, d_schedule != nullptr);
    // Every ray-casting wave reads its launch slot, whatever phase the schedule holds -- a stale schedule's slots are read
    // too, and only then ignored.  The size of the caller's buffer is not known here: the contract is that d_schedule holds
    // vh_render_schedule_bytes(width, height), and this keeps the grid's slots inside that figure should split_tiles ever
    // exceed what the buffer is sized for.
    if (d_schedule && schedule_words(tiles, groups) * sizeof(uint32_t) > vh_render_schedule_bytes(rp->m_width, rp->m_height))
        return VH_ERR_BAD_ARGUMENT;
    CoAlloc job;
    std::memset(&job, 0, sizeof(job));
    if (fj && !fj->allocLaunched && fj->cam.d_depthData && fj->hashData.d_hash && fj->hashParams.m_hashNumBuckets >= 2) {
        job.hd = fj->hashData; job.hp = fj->hashParams; job.cam = fj->cam; job.cp = fj->cp;
        job.bitMask = fj->d_bitMask;
        job.packed = reinterpret_cast<uint2*>(fj->d_packedFrame);
        job.hm = make_hash_mod(fj->hashParams.m_hashNumBuckets);
        job.lockToken = fj->lockToken;
        job.firstGroup = groups;
        groups += co_alloc_groups(image_tiles(fj->cp.m_imageWidth, fj->cp.m_imageHeight));
        fj->allocLaunched = 1;
    }
    const dim3 grid(groups);
    hipStream_t st = (hipStream_t)stream;
    // 32-bit voxel offsets where the pool allows them (load_voxel)
    const bool o32 = vh_render_offsets32(hp->m_numSDFBlocks) != 0;
#define VH_RENDER_LAUNCH(G, O)                                                                                                                  \
    {                                                                                                                                           \
        auto* const kern = large ? &k_render_large<G, O> : &k_render<G, O>;                                                                     \
        VH_LAUNCH_TIMED(kern, grid, 256, st, *hd, *hp, *rd, *cp, *rp, h, l, cap, d_schedule, phase, job);                                       \
    }
    if (rp->m_useGradients) {
        if (o32) VH_RENDER_LAUNCH(true, true) else VH_RENDER_LAUNCH(true, false)
    } else {
        if (o32) VH_RENDER_LAUNCH(false, true) else VH_RENDER_LAUNCH(false, false)
    }
#undef VH_RENDER_LAUNCH
    return vh_last_launch_error();
}

int vh_render_intervals(const VhHashData* hd, const VhHashParams* hp, const VhRayCastData* rd, const VhDepthCameraParams* cp,
                        const VhRayCastParams* rp, uint32_t* d_tileHeads, const VhTileBlock* d_tileBlocks, uint32_t tileCapacity,
                        uint32_t* d_schedule, uint32_t phase, vhStream_t stream)
{
    return vh_render_intervals_co(hd, hp, rd, cp, rp, d_tileHeads, d_tileBlocks, tileCapacity, d_schedule, phase, nullptr, stream);
}

int vh_ray_interval_clear(uint32_t* d_tileHeads, uint32_t width, uint32_t height, vhStream_t stream)
{
    if (!d_tileHeads) return VH_ERR_BAD_ARGUMENT;
    const uint32_t tiles = image_tiles(width, height);
    if (tiles == 0) return VH_OK;
    k_interval_clear<<<cdiv(tiles, 256), 256, 0, (hipStream_t)stream>>>(reinterpret_cast<uint4*>(d_tileHeads), tiles);
    return vh_last_launch_error();
}

int vh_ray_interval_splat(const VhHashData* hd, const VhHashParams* hp, const VhDepthCameraParams* cp, const VhRayCastParams* rp,
                          uint32_t* d_tileHeads, VhTileBlock* d_tileBlocks, uint32_t tileCapacity, uint32_t* d_schedule, uint32_t phase,
                          uint32_t* d_longestList, vhStream_t stream)
{
    if (!hd || !hp || !cp || !rp || !d_tileHeads) return VH_ERR_BAD_ARGUMENT;
    if (rp->m_width == 0 || rp->m_height == 0) return VH_OK;
    const uint32_t groups = splat_groups(*hp);
    k_interval_splat<<<groups + splat_sched_groups(*rp, d_schedule), kSplatThreads, 0, (hipStream_t)stream>>>(
        *hd, *hp, *cp, *rp, reinterpret_cast<uint4*>(d_tileHeads), reinterpret_cast<int4*>(d_tileBlocks), d_tileBlocks ? tileCapacity : 0u,
        d_schedule, phase, schedule_num_cus(d_schedule), groups, d_longestList);
    return vh_last_launch_error();
}

int vh_compute_normals_co2(float* d_output4, const float* d_input4, uint32_t width, uint32_t height, VhFrameJob* fj,
                           const VhRayCastParams* nextView, uint32_t* d_tileHeads, VhTileBlock* d_tileBlocks, uint32_t tileCapacity,
                           uint32_t* d_schedule, uint32_t phase, uint32_t* d_longestList, vhStream_t stream)
{
    if (!d_output4 || !d_input4) return VH_ERR_BAD_ARGUMENT;
    if (width * height == 0) return VH_OK;
    uint32_t groups = cdiv((uint64_t)width * height, 256);
    CoCompactify job;
    std::memset(&job, 0, sizeof(job));
    CoSplat sp;
    std::memset(&sp, 0, sizeof(sp));
    if (fj && fj->allocLaunched && !fj->compactifyLaunched && fj->hashData.d_hash) {
        job.hd = fj->hashData; job.hp = fj->hashParams; job.cp = fj->cp;
        job.groups = compactify_groups(fj->hashParams);
        groups += job.groups;
        fj->compactifyLaunched = 1;
        if (nextView && d_tileHeads && nextView->m_width != 0 && nextView->m_height != 0) { // needs the job's table (job.hd / job.hp)
            sp.rp = *nextView; sp.cp = fj->cp;
            sp.heads = reinterpret_cast<uint4*>(d_tileHeads);
            sp.lists = reinterpret_cast<int4*>(d_tileBlocks);
            sp.sched = d_schedule; sp.feedback = d_longestList;
            sp.cap = d_tileBlocks ? tileCapacity : 0u;
            sp.phase = phase;
            sp.numCUs = schedule_num_cus(d_schedule);
            sp.nSplatGroups = splat_groups(fj->hashParams);
            sp.groups = sp.nSplatGroups + splat_sched_groups(*nextView, d_schedule);
            groups += sp.groups;
        }
    }
    // the frame's pass over the voxels as a third rider (the last workgroups of the grid), if the scene has prepared it and its
    // list is made in this very launch
    CoIntegrate integ;
    std::memset(&integ, 0, sizeof(integ));
    if (fj && job.groups != 0u &&
        fj->fusedPrepared && !fj->fusedLaunched && fj->d_riderDone && fj->d_packedFrame && fj->cam.d_depthData &&
        fj->cp.m_imageWidth <= 0xffffu && fj->cp.m_imageHeight <= 0xffffu) {
        integ.args = fused_args(fj->hashData, fj->hashParams, fj->cam, fj->cp, fj->fusedFlags, fj->fusedLockToken, fj->d_countMirror, fj->mirrorTag, fj->d_packedFrame);
        integ.done = fj->d_riderDone;
        integ.riderTag = 0x80000000u | fj->mirrorTag; // (rider_tag of the frame's number)
        rider_totals(job.groups, fj->listDoneTotal, fj->listClassTotal);
        integ.listExpected = fj->listDoneTotal;
        integ.listClassExpected = fj->listClassTotal;
        integ.first = groups;
        integ.groups = fused_pass_groups(fj->hashParams, device_num_cus());
        groups += integ.groups;
        fj->fusedLaunched = 1;
    }
    VH_LAUNCH_TIMED(k_compute_normals, groups, 256, (hipStream_t)stream, reinterpret_cast<float4*>(d_output4), reinterpret_cast<const float4*>(d_input4), width, height, job, sp, integ);
    return vh_last_launch_error();
}

int vh_compute_normals_co(float* d_output4, const float* d_input4, uint32_t width, uint32_t height, VhFrameJob* fj, vhStream_t stream)
{
    return vh_compute_normals_co2(d_output4, d_input4, width, height, fj, nullptr, nullptr, nullptr, 0u, nullptr, 0u, nullptr, stream);
}

int vh_compute_normals(float* d_output4, const float* d_input4, uint32_t width, uint32_t height, vhStream_t stream)
{
    return vh_compute_normals_co(d_output4, d_input4, width, height, nullptr, stream);
}

int vh_debug_hash_ops(const VhHashData* hd, const VhHashParams* hp, const int32_t* d_ops, int32_t* d_results,
                      uint32_t n, vhStream_t stream)
{
    if (!hd || !hp || !d_ops || !d_results) return VH_ERR_BAD_ARGUMENT;
    if (n == 0) return VH_OK;
    k_debug_hash_ops<<<1, 64, 0, (hipStream_t)stream>>>(*hd, *hp, d_ops, d_results, n);
    return vh_last_launch_error();
}

int vh_debug_check_refined_division(uint32_t n, uint32_t seed, uint32_t* d_mismatches, vhStream_t stream)
{
    if (!d_mismatches) return VH_ERR_BAD_ARGUMENT;
    VH_HIP(hipMemsetAsync(d_mismatches, 0, 2 * sizeof(uint32_t), (hipStream_t)stream));
    if (n == 0) return VH_OK;
    k_check_refined_division<<<cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(n, seed, d_mismatches);
    return vh_last_launch_error();
}

int vh_debug_check_weighted_colour(uint32_t* d_out, vhStream_t stream)
{
    if (!d_out) return VH_ERR_BAD_ARGUMENT;
    const uint32_t init[4] = { 0u, 0u, 0xffffffffu, 0u };
    VH_HIP(hipMemcpyAsync(d_out, init, sizeof(init), hipMemcpyHostToDevice, (hipStream_t)stream));
    VH_HIP(hipStreamSynchronize((hipStream_t)stream)); // (init is this call's own)
    k_check_weighted_colour<<<65536, 256, 0, (hipStream_t)stream>>>(d_out);
    return vh_last_launch_error();
}

} // extern "C"
