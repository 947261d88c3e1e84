/*
 * vh_api.h -- C ABI of the MI355X voxel-hashing TSDF fusion + raycast engine.
 *
 * Drop-in boundary: the reference's host classes call `extern "C"` launchers
 * defined in its .cu files (C++ references, by-value structs -- not C-ABI
 * clean).  This header is their pointer-based twin; every entry point cites the
 * reference interface it replaces.
 *
 *   DSC/ = /root/reference/DepthSensingCUDA/Source/
 *
 * Conventions
 *  - all pointers inside VhHashData / VhDepthCameraData / VhRayCastData are
 *    DEVICE pointers; parameter structs are host pointers, read at call time
 *    and passed to the kernels as arguments (no __constant__ singletons, so
 *    several scenes per process are possible);
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream); every
 *    launcher is asynchronous unless it documents a read-back;
 *  - return value: 0 ok, <0 = -(hipError_t), >0 = VH_ERR_* (vh_types.h);
 *  - `lockToken`: value written into d_hashBucketMutex to take a bucket for
 *    the rest of the pass.  VH_LOCK_ENTRY reproduces the reference (caller
 *    resets the mutex array before the pass with vh_reset_bucket_mutex); any
 *    other value that differs from every token used since the last reset
 *    makes that reset unnecessary (the host classes use a running epoch).
 */
#ifndef VH_API_H
#define VH_API_H

#include "vh_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vhStream_t;

/* ---- library -------------------------------------------------------------- */
const char* vh_version(void);
const char* vh_error_string(int code);
/* text of the last error raised by a handle-level call on this thread */
const char* vh_last_error_message(void);

/* ---- device memory helpers (thin hipMalloc/hipMemcpy wrappers for FFI users) */
int vh_malloc(void** devPtr, size_t bytes);
int vh_free(void* devPtr);
/* pinned, device-visible host memory (hipHostMalloc): what the frame loop's host-fed mode reads straight over the link */
int vh_malloc_host(void** hostPtr, size_t bytes);
int vh_free_host(void* hostPtr);
int vh_memcpy_h2d(void* dst, const void* src, size_t bytes, vhStream_t stream);
int vh_memcpy_d2h(void* dst, const void* src, size_t bytes, vhStream_t stream); /* synchronises the stream */
int vh_memset(void* dst, int value, size_t bytes, vhStream_t stream);
/* measurement: the next kernel the calling thread launches through vh_render, vh_render_intervals[_co], vh_compute_normals[_co, _co2],
 * vh_integrate_fused, vh_query_points or vh_query_rays is launched with hipExtLaunchKernel's start / stop events (two hipEvent_t created with timing):
 * hipEventElapsedTime(start, stop) is then that kernel's own duration -- the dispatch's begin and end time stamps, what
 * rocprofv3's kernel trace reports -- with no event record in the stream.  The launch consumes the pair. */
int vh_time_next_launch(void* startEvent, void* stopEvent);
/* the same for an entry point that launches several kernels: `skip` of the calling thread's timed launches pass first.
 * vh_extract_iso_surface_pass2[_sourced] launch one kernel; vh_mesh_weld launches insert, number, faces (skip 0, 1, 2),
 * vh_mesh_weld_accum_append insert, settle, faces; vh_mesh_vertex_normals and vh_mesh_weld_accum_normals faces, finish;
 * vh_mesh_components init, hook, flatten, count (init alone without faces); vh_mesh_components_filter stats, with
 * largestOnly pick by key and pick by index, compact vertices, compact faces (not without faces);
 * vh_mesh_weld_accum_components the launches of vh_mesh_components, then those of vh_mesh_components_filter;
 * vh_mesh_cluster and vh_mesh_weld_accum_cluster insert, faces, number, emit (insert and number alone without faces);
 * vh_mesh_smooth and vh_mesh_weld_accum_smooth edges, degree, prepare, then gather and step per half step (two half
 * steps an iteration), finish: 4 N + 4 launches (prepare and finish alone without faces);
 * vh_live_mesh_update digest, vanished, dilate, then drop (when something changed and the cache held triangles) and
 * pass 2 (when there is a block to re-mesh); vh_live_mesh_digest one kernel. */
int vh_time_launch_after(uint32_t skip, void* startEvent, void* stopEvent);
int vh_stream_create(vhStream_t* out);   /* a non-blocking HIP stream, for FFI users without a HIP binding */
int vh_stream_destroy(vhStream_t stream);
int vh_stream_synchronize(vhStream_t stream);
int vh_device_synchronize(void);

/* ---- HashData ownership: HashData::allocate / free, DSC/VoxelUtilHashSDF.h:113-181 */
int vh_hash_data_alloc(VhHashData* hd, const VhHashParams* hp);
int vh_hash_data_free(VhHashData* hd);

/* ---- scene-rep launchers: DSC/CUDASceneRepHashSDF.h:15-26 ------------------- */
/* resetCUDA(HashData&, const HashParams&)                       DSC/CUDASceneRepHashSDF.cu:63 */
int vh_reset(const VhHashData* hd, const VhHashParams* hp, vhStream_t stream);
/* resetHashBucketMutexCUDA(HashData&, const HashParams&)        DSC/CUDASceneRepHashSDF.cu:109 */
int vh_reset_bucket_mutex(const VhHashData* hd, const VhHashParams* hp, vhStream_t stream);
/* allocCUDA(HashData&, const HashParams&, const DepthCameraData&, const DepthCameraParams&,
 *           const unsigned int* d_bitMask)                      DSC/CUDASceneRepHashSDF.cu:245
 * d_bitMask may be NULL (streaming disabled).  Also clears d_hashCompactifiedCounter for the
 * compaction that follows. */
int vh_alloc(const VhHashData* hd, const VhHashParams* hp, const VhDepthCameraData* cam,
             const VhDepthCameraParams* cp, const uint32_t* d_bitMask, int32_t lockToken, vhStream_t stream);
/* unsigned compactifyHashAllInOneCUDA(HashData&, const HashParams&)  DSC/CUDASceneRepHashSDF.cu:361
 * The count lands in d_hashCompactifiedCounter.  numOccupied != NULL: blocking
 * read-back as the reference does; NULL: fully asynchronous.
 * flags: VH_COMPACT_COUNTER_IS_ZERO = the caller guarantees the counter is already 0 (vh_alloc leaves it
 * cleared), which saves the memset the reference issues (DSC/CUDASceneRepHashSDF.cu:367). */
enum { VH_COMPACT_COUNTER_IS_ZERO = 1 };
int vh_compactify(const VhHashData* hd, const VhHashParams* hp, const VhDepthCameraParams* cp,
                  uint32_t* numOccupied, uint32_t flags, vhStream_t stream);
/* integrateDepthMapCUDA(...)                                     DSC/CUDASceneRepHashSDF.cu:495
 * integrates hp->m_numOccupiedBlocks compactified blocks. */
int vh_integrate(const VhHashData* hd, const VhHashParams* hp, const VhDepthCameraData* cam,
                 const VhDepthCameraParams* cp, vhStream_t stream);
/* starveVoxelsKernelCUDA(HashData&, const HashParams&)          DSC/CUDASceneRepHashSDF.cu:523 */
int vh_starve(const VhHashData* hd, const VhHashParams* hp, vhStream_t stream);
/* garbageCollectIdentifyCUDA(HashData&, const HashParams&)      DSC/CUDASceneRepHashSDF.cu:592 */
int vh_gc_identify(const VhHashData* hd, const VhHashParams* hp, const VhDepthCameraParams* cp, vhStream_t stream);
/* garbageCollectFreeCUDA(HashData&, const HashParams&)          DSC/CUDASceneRepHashSDF.cu:631 */
int vh_gc_free(const VhHashData* hd, const VhHashParams* hp, int32_t lockToken, vhStream_t stream);
/* bindInputDepthColorTextures(const DepthCameraData&)           DSC/CUDASceneRepHashSDF.cu:15
 * images are read with plain loads: kept as a no-op for source compatibility. */
int vh_bind_input_depth_color_textures(const VhDepthCameraData* cam);

/* Fused integrate -> [starve] -> GC identify -> GC free in ONE pass over the
 * voxels (one read + one write per voxel instead of up to four kernels);
 * same results as the four launchers above in the reference's order
 * (CUDASceneRepHashSDF::integrateDepthMap + garbageCollect, DSC/CUDASceneRepHashSDF.h:317-339).
 * The block count is read on the device from d_hashCompactifiedCounter; if d_countMirror != NULL
 * (a device pointer, e.g. of mapped pinned host memory) the count is also stored there. */
enum { VH_FUSED_GC = 1, VH_FUSED_STARVE = 2 };
/* d_countMirror (may be NULL) receives two words: the block count and `mirrorTag`, a number of the caller's choice
 * (the host class passes its frame counter: a host that maps the words can follow the device without an event).
 * d_packedFrame (may be NULL): the frame as vh_alloc_job packed it, 8 bytes per pixel {depth, colour bytes + sample
 * weight}; the pass then gathers 8 bytes per voxel instead of 20 from the depth and colour maps (same results). */
int vh_integrate_fused(const VhHashData* hd, const VhHashParams* hp, const VhDepthCameraData* cam,
                       const VhDepthCameraParams* cp, uint32_t flags, int32_t lockToken, uint32_t* d_countMirror,
                       uint32_t mirrorTag, const void* d_packedFrame, vhStream_t stream);
/* the alloc / compactify pass of a prepared frame (VhFrameJob, vh_types.h); vh_alloc_job also packs the frame into
 * job->d_packedFrame when that is not NULL.  Each marks the job. */
int vh_alloc_job(VhFrameJob* job, vhStream_t stream);
int vh_compactify_job(VhFrameJob* job, vhStream_t stream);

/* ---- ray-cast launchers: DSC/CUDARayCastSDF.cpp:10-21 ----------------------- */
/* renderCS(const HashData&, const RayCastData&, const DepthCameraData&, const RayCastParams&)
 *                                                               DSC/CUDARayCastSDF.cu:59 */
/* d_normals of the VhRayCastData may be NULL for vh_render / vh_render_intervals: the map is then not written (the
 * host class does so when vh_compute_normals overwrites it right after). */
int vh_render(const VhHashData* hd, const VhHashParams* hp, const VhRayCastData* rd,
              const VhDepthCameraParams* cp, const VhRayCastParams* rp, vhStream_t stream);
/* ---- batch queries (not in the reference) --------------------------------------
 * Read-only questions to the blocks that are RESIDENT ON THE DEVICE: blocks streamed out to the host grid are absent,
 * as they are for the ray caster.  All arrays are device pointers; one thread per point / ray.  Nothing is written to
 * the scene, but the caller must not run a query beside an integrate (or streaming pass) on another stream.
 *
 * vh_query_points: per point p = d_points3[3i..3i+2] (world space)
 *   d_valid[i]      what trilinearInterpolationSimpleFastFast(p) returns (DSC/RayCastSDFUtil.h:97-116), one byte
 *   d_sdf[i]        its distance; -inf where valid is 0 (the reference's partial sum is not reported)
 *   d_color[i]      its colour, r | g << 8 | b << 16; 0 where valid is 0
 *   d_gradient3     (may be NULL) gradientForPoint(p) (:174-195) at EVERY point, valid or not: its six samples ignore
 *                   their own validity, partial sums included
 * A point with a non-finite coordinate is valid = 0 with gradient (0, 0, 0), decided before any lookup.
 *
 * vh_query_rays: per ray the body of traverseCoarseGridSimpleSampleAll (:198-262) with worldCamPos = origin,
 * worldDir = direction (used as given: the caller normalises), rayCurrent = tMin, rayEnd = tMax: the same samples
 * t += m_rayIncrement, sign-change test, three bisection steps and two thresholds; the march resumes after a rejected
 * crossing.  Of rp only m_rayIncrement (finite and > 0, else VH_ERR_BAD_ARGUMENT), m_thresSampleDist and m_thresDist
 * are read.
 *   d_status[i]  1 hit:     d_t = the bisection's alpha, d_color = the last bisection sample's colour (packed as
 *                           above), d_normals3 (may be NULL) = -gradientForPoint(origin + alpha * direction) in WORLD
 *                           space -- always from the gradient, whatever m_useGradients says
 *                0 miss:    d_t = -inf, normal (-inf, -inf, -inf), colour 0
 *                2 refused: outputs as for a miss, the ray is not marched: origin, direction, tMin or tMax not
 *                           finite; direction (0, 0, 0); (tMax - tMin) / m_rayIncrement > VH_QUERY_MAX_SAMPLES.
 * The march also counts its samples and stops at VH_QUERY_MAX_SAMPLES (t + increment == t cannot spin a wave).
 * A wave lasts as long as its longest ray: rays in a coherent order (neighbours next to each other) run faster.
 * n = 0 succeeds without a launch.  vh_time_next_launch applies to both, and to vh_render. */
int vh_query_points(const VhHashData* hd, const VhHashParams* hp, const float* d_points3, uint32_t n, float* d_sdf, uint32_t* d_color,
                    float* d_gradient3 /* may be NULL */, uint8_t* d_valid, vhStream_t stream);
int vh_query_rays(const VhHashData* hd, const VhHashParams* hp, const VhRayCastParams* rp, const float* d_origins3, const float* d_directions3,
                  const float* d_tMin, const float* d_tMax, uint32_t n, float* d_t, float* d_normals3 /* may be NULL */, uint32_t* d_color,
                  uint8_t* d_status, vhStream_t stream);
/* Ray-interval splatting as a compute pass: resetRayIntervalSplatCUDA / rayIntervalSplatCUDA
 * (DSC/CUDARayCastSDF.cu:88,169) + the D3D11 min/max rasterisation (DSC/DX11RayIntervalSplatting.cpp:150-220) that
 * this fork leaves disabled.  Per 8x8-pixel tile (ceil(W/8)*ceil(H/8) of them, row-major):
 *   d_tileHeads   4 words: {min, max} camera depth (float bits) of the allocated blocks the tile's rays can read --
 *                 kept only when no lists are (d_tileBlocks NULL); with lists the ray caster forms the range from the
 *                 listed blocks --, their number, 0;
 *   d_tileBlocks  tileCapacity entries: those blocks (may be NULL: intervals only).  tileCapacity also picks the
 *                 ray caster's table size: up to VH_TILE_LIST_CAPACITY (64) small tables, above it large ones
 *                 (VH_TILE_LIST_CAPACITY_LARGE, 128).  A longer list is used as far as it fits; the blocks it could
 *                 not hold are looked up in the hash table.
 *   d_longestList (splat, with a schedule; may be NULL) receives the longest list the previous render met if it came
 *                 within 16 of the small capacity, else 0: what a host needs to choose the capacity.
 * Both are conservative (every allocated block, grown by the reach of a sample), so rendering with them gives
 * bit-identical maps.  vh_render_intervals consumes and re-arms the heads; vh_ray_interval_clear arms them once. */
int vh_ray_interval_clear(uint32_t* d_tileHeads, uint32_t width, uint32_t height, vhStream_t stream);
int vh_ray_interval_splat(const VhHashData* hd, const VhHashParams* hp, const VhDepthCameraParams* cp, const VhRayCastParams* rp,
                          uint32_t* d_tileHeads, VhTileBlock* d_tileBlocks, uint32_t tileCapacity, uint32_t* d_schedule, uint32_t phase,
                          uint32_t* d_longestList, vhStream_t stream);
/* d_schedule (may be NULL) is vh_render_schedule_bytes() of device memory, zeroed once, that belongs to one sequence
 * of splat + render calls; phase is that sequence's call counter (1, 2, 3, ...; the same value for the splat and the
 * render of one frame).  The ray caster stores the cost every tile had; the next splat sorts the tiles by it and
 * deals them to the workgroups so that the compute units get even loads.  The maps do not depend on it, and a render
 * whose splat was given no schedule uses raster order. */
size_t vh_render_schedule_bytes(uint32_t width, uint32_t height);
/* how many tiles of an image of this size a scheduled render marches with two waves each (the dearest ones; 0 for
 * small images): lets a test make sure it exercises that path */
uint32_t vh_render_split_tiles(uint32_t width, uint32_t height);
/* Voxel addressing of the interval ray caster: 1 if, for a pool of numSDFBlocks blocks, it addresses voxels with 32-bit
 * byte offsets on the pool's base (numSDFBlocks * 4096 <= 2^32 bytes), 0 if with 64-bit addresses.  The maps are the same.
 * vh_debug_render_force_offsets64(1) makes every later render of the process take the 64-bit form (0: back to the rule)
 * and returns the setting it replaces: for tests that compare the two. */
uint32_t vh_render_offsets32(uint32_t numSDFBlocks);
uint32_t vh_debug_render_force_offsets64(uint32_t on);
int vh_render_intervals(const VhHashData* hd, const VhHashParams* hp, const VhRayCastData* rd, const VhDepthCameraParams* cp,
                        const VhRayCastParams* rp, uint32_t* d_tileHeads, const VhTileBlock* d_tileBlocks, uint32_t tileCapacity,
                        uint32_t* d_schedule, uint32_t phase, vhStream_t stream);
/* computeNormals(float4* d_output, float4* d_input, width, height)  DSC/CameraUtil.cu:699 */
int vh_compute_normals(float* d_output4, const float* d_input4, uint32_t width, uint32_t height, vhStream_t stream);
/* The same two launches with the passes of a frame job riding along as extra workgroups (job may be NULL, or already
 * launched: then they equal the plain calls): the alloc pass behind the ray caster's workgroups, where it fills the
 * tail the dearest tiles leave, and the compactify pass behind computeNormals'.  Legal because a block allocated while
 * rays are marched holds only unobserved voxels, which a sample treats like an absent block. */
int vh_render_intervals_co(const VhHashData* hd, const VhHashParams* hp, const VhRayCastData* rd, const VhDepthCameraParams* cp,
                           const VhRayCastParams* rp, uint32_t* d_tileHeads, const VhTileBlock* d_tileBlocks, uint32_t tileCapacity,
                           uint32_t* d_schedule, uint32_t phase, VhFrameJob* job, vhStream_t stream);
int vh_compute_normals_co(float* d_output4, const float* d_input4, uint32_t width, uint32_t height, VhFrameJob* job, vhStream_t stream);
/* ... and, when the job's compactify pass rides along and nextView != NULL, the interval splat of the NEXT render as
 * well (arguments as vh_ray_interval_splat; nextView holds that render's view matrices: the pose of the job's frame).
 * It lists the table as it stands BEFORE the job's frame is integrated: blocks that pass frees stay listed with all-zero
 * voxels (read like absent ones), blocks allocated later are empty.  Whoever uses it must make sure nothing else edits
 * the table in between (the host class CUDARayCastSDF checks the job's frame number and table epoch). */
int vh_compute_normals_co2(float* d_output4, const float* d_input4, uint32_t width, uint32_t height, VhFrameJob* job,
                           const VhRayCastParams* nextView, uint32_t* d_tileHeads, VhTileBlock* d_tileBlocks, uint32_t tileCapacity,
                           uint32_t* d_schedule, uint32_t phase, uint32_t* d_longestList, vhStream_t stream);

/* Read-back without a blocking call: one thread writes {*d_src0, *d_src1 (0 where NULL), tag} -- the tag last, with
 * system scope -- to d_mapped, the device alias of three words of mapped pinned host memory (vh_malloc_host memory is
 * mapped).  The host polls word 2 for the tag.  Replaces the reference's blocking cudaMemcpy of the streaming counters
 * (DSC/CUDASceneRepChunkGrid.cu:88, :140). */
int vh_publish_words(const uint32_t* d_src0, const uint32_t* d_src1, uint32_t* d_mapped, uint32_t tag, vhStream_t stream);

/* ---- streaming launchers: DSC/CUDASceneRepChunkGrid.h:142-146 --------------- */
/* integrateFromGlobalHashPass1CUDA(params, hashData, threadsPerPart, start, radius, camPos,
 *                                  d_outputCounter, d_output)   DSC/CUDASceneRepChunkGrid.cu:76 */
int vh_stream_out_pass1(const VhHashData* hd, const VhHashParams* hp, uint32_t threadsPerPart, uint32_t start,
                        float radius, const float camPos[3], uint32_t* d_outputCounter, VhSDFBlockDesc* d_output,
                        uint32_t outputCapacity, int32_t lockToken, vhStream_t stream);
/* The scan of vh_stream_out_pass1 without its deletes: the number of blocks the pass would move out, published as
 * {count, 0, tag} to d_mapped (device alias of mapped host memory, see vh_publish_words); *d_counter must be zero and is
 * zero again afterwards.  No reference twin: it lets a frame loop that knows its poses ahead skip the streaming step of a
 * frame in which nothing would stream (CUDASceneRepChunkGrid::probeStreamOut). */
int vh_stream_out_probe(const VhHashData* hd, const VhHashParams* hp, uint32_t threadsPerPart, uint32_t start, float radius,
                        const float camPos[3], uint32_t* d_counter, uint32_t* d_mapped, uint32_t tag, vhStream_t stream);
/* integrateFromGlobalHashPass2CUDA(params, hashData, threadsPerPart, descs, d_output, n)  :115 */
int vh_stream_out_pass2(const VhHashData* hd, const VhHashParams* hp, const VhSDFBlockDesc* d_descs,
                        VhVoxel* d_output, uint32_t nSDFBlocks, vhStream_t stream);
/* ---- the streaming passes for a caller that does not wait for the device (not in the reference: its host reads a counter back
 * before every second launch, DSC/CUDASceneRepChunkGrid.cu:88,140).
 * vh_stream_out_device: integrateFromGlobalHashPass1CUDA + Pass2CUDA in one call.  The counter is cleared, pass 1 lists at most
 * `mostBlocks` blocks (an upper bound the caller has from vh_stream_out_probe) and sets, in d_bitMask (may be NULL), the bit of
 * every listed block's chunk -- what the host's integrateInChunkGrid does when the block arrives; pass 2 is launched for
 * mostBlocks blocks and reads the count on the device.
 * vh_publish_count: {*d_counter, 0, tag} into mapped host memory (tag last, system scope), to be enqueued behind the copies of
 * the pass's output.
 * vh_stream_in_device: chunkToGlobalHashPass1CUDA + Pass2CUDA + the heap counter's update with the counter read on the device,
 * in three launches after which the device state is final.  Clears bit `chunkBit` of d_bitMask (d_bitMask may be NULL,
 * chunkBit 0xffffffff: none).  A block that finds no slot (its bucket and its list full, or a second overflow of one bucket
 * within the pass; the reference has no such case handling, DSC/VoxelUtilHashSDF.h:682-713) keeps no voxels: its SDF block
 * goes back onto the heap, cleared, and the chunk's bit is set again.  d_failed: device scratch of 1 + 2n words, zero on
 * entry and zero again afterwards.  Publishes {blocks that found no slot, 0, tag, 1 if the heap held too few free blocks --
 * then nothing was done, and d_state[VH_STATE_HEAP_UNDERFLOW] is raised -- then their indices into d_descs} to d_mapped
 * (room for 4 + n words; tag last, system scope). */
int vh_stream_out_device(const VhHashData* hd, const VhHashParams* hp, uint32_t threadsPerPart, uint32_t start, float radius,
                         const float camPos[3], uint32_t* d_outputCounter, VhSDFBlockDesc* d_descs, VhVoxel* d_blocks,
                         uint32_t mostBlocks, int32_t lockToken, uint32_t* d_bitMask, vhStream_t stream);
int vh_publish_count(const uint32_t* d_counter, uint32_t* d_mapped, uint32_t tag, vhStream_t stream);
int vh_stream_in_device(const VhHashData* hd, const VhHashParams* hp, uint32_t n, const VhSDFBlockDesc* d_descs, const VhVoxel* d_blocks,
                        int32_t lockToken, uint32_t* d_failed, uint32_t* d_bitMask, uint32_t chunkBit, uint32_t* d_mapped, uint32_t tag,
                        vhStream_t stream);
/* chunkToGlobalHashPass1CUDA(params, hashData, n, heapCountPrev, descs, blocks)           :162 */
int vh_stream_in_pass1(const VhHashData* hd, const VhHashParams* hp, uint32_t n, uint32_t heapCountPrev,
                       const VhSDFBlockDesc* d_descs, int32_t lockToken, vhStream_t stream);
/* chunkToGlobalHashPass2CUDA(params, hashData, n, heapCountPrev, descs, blocks)           :192 */
int vh_stream_in_pass2(const VhHashData* hd, const VhHashParams* hp, uint32_t n, uint32_t heapCountPrev,
                       const VhSDFBlockDesc* d_descs, const VhVoxel* d_blocks, vhStream_t stream);

/* ---- scene merge (not in the reference; DESIGN.md section 4 "Scene merge") -----
 * vh_merge_blocks fuses n source blocks into the table: block i, at d_descs[i].pos + blockOffset, is allocated if the
 * table does not hold that position, and its 512 voxels are merged voxel by voxel: a source voxel of weight 0 changes
 * nothing; onto a destination voxel of weight 0 the source voxel is copied with its weight capped at
 * m_integrationWeightMax; two observed voxels go through combineVoxel as integrate uses it (hp's m_integrationWeightMax
 * and m_colorIntegration).  The voxels are d_blocks[i * 512 ...] (a block list as the streaming passes move it), or
 * srcSDFBlocks[d_descs[i].ptr ...] (another scene's pool, its entries listed by vh_merge_gather): exactly one of the
 * two is given.  The positions must be distinct, and no block of the destination may be streamed out.
 * All or nothing on the heap: if the positions missing from the table outnumber its free blocks, nothing is changed
 * and the status word is VH_MERGE_HEAP_SHORT.  A block allocBlock finds no room for is left out whole
 * (VH_MERGE_NO_SLOT): no entry, no heap block, its index in d_leftOut (may be NULL; room for n words, the first
 * counts_out[VH_MERGE_LEFT_OUT] are written).  Alloc passes repeat, the bucket mutexes reset before each, while blocks
 * lose lock races, at most (missing + 8) times; what is pending then is left out too (VH_MERGE_NOT_SETTLED).
 * d_work: vh_merge_work_bytes(n) bytes of device scratch.  counts_out: VH_MERGE_NUM_COUNTS host words.  Returns VH_OK
 * with a status set: the caller looks at counts_out[VH_MERGE_STATUS].  One-shot and BLOCKING: the call reads a few
 * words back after the classification, after every alloc pass and at the end.  n = 0 launches nothing and reports zeros.
 * vh_time_launch_after: classify, decide, one launch per alloc pass, (give up), combine.
 * vh_merge_gather: every occupied entry of a table as {pos, ptr}, in no particular order, *d_counter = their number
 * (cleared first; entries beyond `capacity` are counted but not written).  Asynchronous. */
size_t vh_merge_work_bytes(uint32_t n);
int vh_merge_gather(const VhHashData* hd, const VhHashParams* hp, VhSDFBlockDesc* d_descs, uint32_t capacity, uint32_t* d_counter, vhStream_t stream);
int vh_merge_blocks(const VhHashData* hd, const VhHashParams* hp, uint32_t n, const VhSDFBlockDesc* d_descs, const VhVoxel* d_blocks /* or NULL */,
                    const VhVoxel* srcSDFBlocks /* or NULL */, const int32_t blockOffset[3], int32_t lockToken, uint32_t* d_work,
                    uint32_t* d_leftOut /* may be NULL */, uint32_t* counts_out, vhStream_t stream);

/* ---- resampled merge (not in the reference; DESIGN.md section 4 "Resampled merge") -----
 * A source scene sampled at the voxel centres of another lattice: the block list that vh_merge_blocks then fuses.
 * All geometry is in voxel index space.  vh_resample_voxel_transforms makes the two 3x4 row-major float matrices from a
 * rigid 4x4 row-major dstFromSrc (metres) and the two voxel sizes, in double, rounded once:
 *   srcVoxFromDstVox = [R^T (vsDst / vsSrc) | -R^T t / vsSrc]      dstVoxFromSrcVox = [R (vsSrc / vsDst) | t / vsDst]
 * and returns VH_ERR_BAD_ARGUMENT for a bottom row other than (0, 0, 0, 1), max |R^T R - I| > 1e-4, det R <= 0, a
 * non-finite entry or voxel size, or vsSrc / vsDst outside [1/2, 2].  Host only.
 * vh_resample_blocks, per destination voxel (i, j, k) of a candidate block: q_r = ((m_r0 i + m_r1 j) + m_r2 k) + m_r3
 * with m = srcVoxFromDstVox in float; b = floor(q), f = q - b, g = 1 - f; the eight taps b + (bit 0, bit 1, bit 2) of
 * t = 0..7 weigh w_t = (a_x a_y) a_z, a = f where the bit is set and g where not; a tap of weight 0 is not read.  The
 * voxel is unobserved (all zero) if some |q_r| is not below 2^24, or a used tap lies in a block the source does not
 * hold or has weight 0; otherwise its sdf and each colour channel are the used taps' w * value summed in tap order
 * from the first product, the colour rounded as (int)(sum + 0.5f) and capped at 255, its weight the least of the used
 * taps'.  Candidate blocks are those a source block d_srcDescs[i].pos may reach (a superset, made distinct in a table of
 * 2^slotsLog2 slots); the staged list holds exactly the candidates with an observed voxel, each once, in no order.
 * Two calls, both BLOCKING (each reads a few words back):
 *   count: d_staging NULL.  Finds the candidates; counts_out[VH_RESAMPLE_CANDIDATES] and the status are final.
 *   fill:  d_work as the count call left it, d_outDescs and d_staging with room for stagingBlocks >= candidates blocks.
 *          Block c is written whole to d_staging + c * 512; d_outDescs[0 .. staged) = {pos, ptr = c * 512}: a list for
 *          vh_merge_blocks with srcSDFBlocks = d_staging.  Staging needs no clearing: only listed blocks are read.
 * With a status bit set the fill call does nothing.  VH_ERR_BAD_ARGUMENT for a matrix that is not finite or stretches
 * beyond what ratio 2 allows (6 candidate blocks, 5 source blocks per axis), slotsLog2 outside [4, 28], staging too
 * small.  d_work: vh_resample_work_bytes(slotsLog2) bytes.  counts_out: VH_RESAMPLE_NUM_COUNTS host words.
 * vh_time_launch_after: count: candidates; fill: resample. */
int vh_resample_voxel_transforms(const double* dstFromSrc16, float vsSrc, float vsDst, float* srcVoxFromDstVox12, float* dstVoxFromSrcVox12);
size_t vh_resample_work_bytes(uint32_t slotsLog2);
int vh_resample_blocks(const VhHashData* srcHd, const VhHashParams* srcHp, uint32_t n, const VhSDFBlockDesc* d_srcDescs,
                       const float* srcVoxFromDstVox12, const float* dstVoxFromSrcVox12, uint32_t slotsLog2, uint32_t* d_work,
                       VhSDFBlockDesc* d_outDescs /* NULL: count */, VhVoxel* d_staging /* NULL: count */, uint32_t stagingBlocks,
                       uint32_t* counts_out, vhStream_t stream);

/* ---- scene registration (not in the reference; DESIGN.md section 4 "Scene registration") -----
 * The rigid motion that lays a source scene onto a destination scene, by direct SDF-to-SDF Gauss-Newton; neither scene
 * is written.  The estimate lives in a VhAlignState in device memory; a step is one kernel that reads and updates it.
 * All geometry is in the destination's voxel index space; the matrices are those of vh_resample_voxel_transforms.
 * Per voxel v = (i, j, k) of a listed source block with weight > 0 and |sdf_S(v)| <= band * vsSrc (one float product):
 *   q = dstVoxFromSrcVox v as vh_resample_blocks forms it; dropped unless every |q_r| < 2^24
 *   seven samples of the destination by the blend of vh_resample_blocks: at q and at q +- 1/2 along each axis
 *   (q_c + 0.5f, q_c - 0.5f); dropped unless every used tap of all seven is observed
 *   e = (phi(q) - sdf_S(v)) / vsDst        g_c = (phi(q + e_c / 2) - phi(q - e_c / 2)) / vsDst
 *   dropped unless |phi(q)| <= band * vsDst and every |g_c| <= 2
 *   u_c = (q_c - pivot_c) * invRadius; dropped unless every |u_c| <= 1 (pivot and radius are chosen so that this
 *   drops nothing; the gate is what bounds the terms whatever the estimate does)
 *   J = (u_y g_z - u_z g_y, u_z g_x - u_x g_z, u_x g_y - u_y g_x, g_x, g_y, g_z)
 *   29 terms in float, one rounding each: J_a J_b (a <= b, by rows), J_a e, e e, 1; each summed as the 64-bit integer
 *   rint(term * 2^26) (exact scaling, ties to even): the totals do not depend on the order of the sums.
 * The step, by one lane, in double: total / 2^26; (J^T J) y = -J^T e by the trackers' 6x6 solve; no step with
 * VH_ALIGN_TOO_FEW when the count is below minCount, with VH_ALIGN_ILL_CONDITIONED when the solve's condition number is
 * not <= condThres; otherwise w = y[0..3) * invRadius (radians), tau = y[3..6) (destination voxels),
 * R = exp([w]x) by Rodrigues, the motion q -> pivot + R (q - pivot) + tau of the destination's voxel space, in metres,
 * composed onto dstFromSrc from the left, and the voxel matrices derived again; VH_ALIGN_CONVERGED when |w| < rotThres
 * and |tau| < transThres.
 * vh_align_begin (BLOCKING): writes the whole state.  VH_ERR_BAD_ARGUMENT for a guess or voxel sizes that
 * vh_resample_voxel_transforms refuses, a pivot that is not finite, a radius that is not a positive power of two.
 * vh_align_step: one launch, max(n, 1) workgroups; *d_ticket must be 0 (it is left 0).  VH_ERR_BAD_ARGUMENT, with nothing
 * launched, for band outside (0, VH_ALIGN_MOST_BAND], thresholds that are not finite and positive, voxel sizes that are
 * not the state's; for n > VH_ALIGN_MOST_BLOCKS the state's status gets VH_ALIGN_TOO_MANY as well.
 * vh_time_next_launch applies to vh_align_step. */
int vh_align_begin(VhAlignState* d_state, const double* dstFromSrcGuess16, float vsSrc, float vsDst, const float pivot3[3], float radius, vhStream_t stream);
int vh_align_step(const VhHashData* dstHd, const VhHashParams* dstHp, const VhHashData* srcHd, const VhHashParams* srcHp, uint32_t n,
                  const VhSDFBlockDesc* d_srcDescs, float band, uint32_t minCount, float condThres, double rotThres, double transThres,
                  VhAlignState* d_state, uint32_t* d_ticket, vhStream_t stream);
/* The box of the listed blocks: d_box6 = {least x, y, z, greatest x, y, z} of the positions of the first
 * min(n, *d_count) blocks (d_count NULL: n; a device word, so that a list's length need not be read back first).
 * d_box6 must hold INT_MAX thrice and INT_MIN thrice before. */
int vh_align_bounds(uint32_t n, const VhSDFBlockDesc* d_descs, const uint32_t* d_count /* may be NULL */, int32_t* d_box6, vhStream_t stream);

/* ---- scene cut (not in the reference; DESIGN.md section 4 "Scene cut") -----
 * The opposite of the merge: the voxels of a region erased from the table, lifted out as a block list, or both.
 * All geometry is in voxel index space.  Voxel l of the block at pos is the integer triple (i, j, k) = 8 pos +
 * (l & 7, (l >> 3) & 7, l >> 6); with the float 3x4 row-major matrix m12 (regionFromVox), per row r
 *   u_r = ((m_r0 i + m_r1 j) + m_r2 k) + m_r3      in float32, in that order, no contraction.
 * VH_CUT_BOX: the voxel is inside iff |u_x| <= 1 && |u_y| <= 1 && |u_z| <= 1; VH_CUT_ELLIPSOID: iff (u_x u_x + u_y u_y) +
 * u_z u_z <= 1.  A comparison with a NaN is false: outside.  The selected voxels are the inside ones, with
 * VH_CUT_SELECT_OUTSIDE those that are not inside.  vh_cut_region_transform (host only, in double, each value rounded
 * once) makes m12 from a rigid 4x4 row-major worldFromRegion [R | t] in metres, three half extents h_r > 0 in metres and
 * the scene's voxel size: m[r][c] = (R[c][r] vs) / h_r, m[r][3] = -(((R[0][r] t_0 + R[1][r] t_1) + R[2][r] t_2) / h_r);
 * VH_ERR_BAD_ARGUMENT for what vh_resample_voxel_transforms refuses (bottom row, max |R^T R - I| > 1e-4, det R <= 0, a
 * non-finite entry) and a half extent or voxel size that is not finite and positive.
 *
 * vh_cut_blocks, per block i of the n listed: the block is touched iff one of its 512 voxels is selected, whatever its
 * weight; a block that is not touched is unchanged byte for byte.
 *   erase (default): every selected voxel of a touched block becomes 8 zero bytes; a touched block in which no unselected
 *          voxel has weight > 0 is freed: zeroed whole, then, in a later launch, its entry removed by
 *          deleteHashEntryElement (the block id back on the heap, which holds all-zero blocks only).
 *   lift (VH_CUT_LIFT): every touched block with a selected voxel of weight > 0 is written whole to d_staging at a slot c,
 *          each once, in no particular order -- selected voxels as they are, the others zero -- with d_outDescs[c] =
 *          {pos, c * 512}: a list vh_merge_blocks takes with d_blocks = d_staging or srcSDFBlocks = d_staging.
 *   keep (VH_CUT_KEEP, only with VH_CUT_LIFT): nothing in the table is written.
 *   count (VH_CUT_COUNT_ONLY): nothing is written anywhere but d_work; the counts are those the call without the flag gives.
 * The blocks are a table's entries (d_descs from vh_merge_gather, d_blocks NULL: the voxels are hd's pool at the descs'
 * ptr) or, with VH_CUT_KEEP only, a plain list d_blocks[i * 512 ...] (hd may be NULL).  All or nothing: when lifting
 * and stagingBlocks is less than the blocks to lift, nothing is written, the status is VH_CUT_STAGING_SHORT and the
 * call returns VH_ERR_BAD_ARGUMENT with the counts filled (the classification's: what a large enough pool would have
 * seen done; VH_CUT_LIFTED is the room needed).  Deletes that lose a bucket-lock race are run again, the
 * bucket mutexes reset before every pass but the first, at most (freed + 8) times; a block pending then stays
 * allocated, all zero (VH_CUT_NOT_SETTLED, counted in VH_CUT_UNSETTLED).  d_work: vh_cut_work_bytes(n) bytes of device
 * scratch.  counts_out: VH_CUT_NUM_COUNTS host words.  One-shot and BLOCKING: the call reads a few words back after its
 * first stage and after every delete pass.  n = 0 launches nothing and reports zeros.  The caller compactifies before
 * the next ray cast.  vh_time_launch_after: select (which erases too when nothing is lifted); when lifting: decide,
 * lift, (erase); then one launch per delete pass. */
int vh_cut_region_transform(const double* worldFromRegion16, const float* halfExtents3, float voxelSize, float* m12);
size_t vh_cut_work_bytes(uint32_t n);
int vh_cut_blocks(const VhHashData* hd, const VhHashParams* hp, uint32_t n, const VhSDFBlockDesc* d_descs, const VhVoxel* d_blocks /* or NULL */,
                  const float* m12, uint32_t shape, uint32_t flags, int32_t lockToken, uint32_t* d_work, VhSDFBlockDesc* d_outDescs,
                  VhVoxel* d_staging, uint32_t stagingBlocks, uint32_t* counts_out, vhStream_t stream);

/* ---- frame de-integration (not in the reference; DESIGN.md section 4 "Frame de-integration") -----
 * A fused depth frame taken back out of the table.  The frame is its float depth map and float4 colour map (cam), the
 * camera (cp) and its pose, in hp->m_rigidTransform / m_rigidTransformInverse.
 * The observation of voxel l of the block at pos, pi = 8 pos + (l & 7, (l >> 3) & 7, l >> 6) in wrapping int32, is what
 * the integrate pass hands to combineVoxel for it, the same float32 operations in the same order: pf = inverse * (pi *
 * voxelSize); the pixel (uint)cvt_rz((pf.x fx / pf.z + mx) + 0.5f), likewise y; it must lie inside the image; its colour
 * c (MINF without a colour map) must have c.x != MINF and its depth d must be != MINF, < m_maxIntegrationDistance and
 * have sdf = d - pf.z > -T, T = m_truncation + m_truncScale d.  Then o = sdf clamped to [-T, T], wo =
 * uchar(fmaxf(m_integrationWeightSample * 1.5f * (1 - (d - depthMin) / (depthMax - depthMin)), 1)), co = uchar(255 c)
 * per channel.  A voxel that fails a gate has no observation.  (As in the reference, a frame without a colour map puts
 * nothing in, so it has no observation to take out.)
 * The take-out of (o, co, wo) from the stored voxel (s, c, w):
 *   no observation, w == 0 or wo == 0: unchanged, byte for byte;
 *   wo >= w: 8 zero bytes;
 *   else w' = w - wo, s' = (s (float)w - o (float)wo) / (float)w' in float32, in that order, IEEE division, no contraction;
 *        colour with m_colorIntegration == VH_COLOR_RUNNING_AVERAGE: unchanged (a 50/50 average cannot be inverted);
 *        otherwise per channel n = c w - co wo (signed), c' = clamp(floor((2 n + w') / (2 w')), 0, 255).
 * A changed voxel whose w was m_integrationWeightMax is counted as at the cap: its weight was not the sum of what went
 * in, and the take-out is not the inverse there (nor after a starve pass).
 * vh_deintegrate_blocks, per block i of the n listed (d_descs from vh_merge_gather: the voxels are hd's pool at the
 * descs' ptr): the block is processed iff isSDFBlockInCameraFrustumApprox holds for it at the frame's pose (the test
 * compactify used when the frame went in); a block that is not processed is unchanged byte for byte.  A processed block
 * left without a voxel of weight > 0 is freed whether or not the call changed it: zeroed whole, then, in a later
 * launch, its entry removed by deleteHashEntryElement (the block id back on the heap, which holds all-zero blocks
 * only).  Deletes that lose a bucket-lock race are run again, the bucket mutexes reset before every pass but the
 * first, at most (freed + 8) times; a block pending then stays allocated, all zero (VH_DEINT_NOT_SETTLED, counted in
 * VH_DEINT_UNSETTLED).  VH_DEINT_COUNT_ONLY classifies and writes nothing but d_work; the counts are those of the call
 * without the flag.  d_work: vh_deintegrate_work_bytes(n) bytes of device scratch.  counts_out: VH_DEINT_NUM_COUNTS host
 * words.  The maps must hold cp->m_imageWidth * m_imageHeight pixels.  One-shot and BLOCKING: the call reads a few
 * words back after the apply launch and after every delete pass.  n = 0 launches nothing and reports zeros.  The
 * caller compactifies before the next ray cast.  vh_time_launch_after: apply; then one launch per delete pass
 * (vh_reset_bucket_mutex's launch between two passes is not a timed one and is not counted). */
size_t vh_deintegrate_work_bytes(uint32_t n);
int vh_deintegrate_blocks(const VhHashData* hd, const VhHashParams* hp, uint32_t n, const VhSDFBlockDesc* d_descs, const VhDepthCameraData* cam,
                          const VhDepthCameraParams* cp, uint32_t flags, int32_t lockToken, uint32_t* d_work, uint32_t* counts_out, vhStream_t stream);

/* ---- utilities that are not in the reference -------------------------------- */
/* Synthetic analytic-sphere depth+colour frame,
 * generated on the device so benchmark inputs are HBM-resident. */
int vh_synth_frame(const double* h_spheres, int nSpheres, int inside, const float camToWorld[16],
                   const VhDepthCameraParams* cp, float* d_depth, float* d_color4, vhStream_t stream);
/* Executes a list of hash operations one after the other in a single thread:
 * deterministic exercise of allocBlock / deleteHashEntryElement /
 * insertHashEntry / getHashEntryForSDFBlockPos including collision lists.
 * ops: n x {op, x, y, z, arg}; results: n ints.  op 0 = alloc, 1 = delete,
 * 2 = insert(ptr = arg), 3 = lookup (result = ptr), 4 = new lock pass. */
enum { VH_OP_ALLOC = 0, VH_OP_DELETE = 1, VH_OP_INSERT = 2, VH_OP_LOOKUP = 3, VH_OP_NEW_PASS = 4 };
int vh_debug_hash_ops(const VhHashData* hd, const VhHashParams* hp, const int32_t* d_ops, int32_t* d_results,
                      uint32_t n, vhStream_t stream);

/* Self-check of the two exact shortcuts the ray caster uses: division by the
 * voxel size through a reciprocal with two correction steps, and modulo by the
 * bucket count through a multiply-shift.  d_mismatches[0] / [1] = number of
 * operands (of n pseudo-random ones) where the shortcut differs from `/` / `%`.
 * The first 256 operands also check the ray caster's colour bytes: c / 255 for
 * every byte c through the same shortcut (counted in d_mismatches[0]). */
int vh_debug_check_fast_math(float divisor, uint32_t modulus, uint32_t n, uint32_t seed, uint32_t* d_mismatches, vhStream_t stream);

/* The ray caster's wave reductions (minimum and maximum of 64 floats, maximum of
 * 64 unsigned words) run by one wave on the 64 words of d_in64: d_out192[0..63] =
 * what each lane got back as the float minimum, [64..127] the float maximum,
 * [128..191] the unsigned maximum.  All 64 of a helper are the same word. */
int vh_debug_wave_reduce(const uint32_t* d_in64, uint32_t* d_out192, vhStream_t stream);

/* Self-check of the division the fused integrate pass uses for blocks it has certified (one refined reciprocal shared by
 * the two perspective divisions of a voxel; the same for the blend's division by the weight sum): n pseudo-random
 * operand pairs inside the certified ranges against `/`.  d_mismatches[0]: projection range, [1]: blend range. */
int vh_debug_check_refined_division(uint32_t n, uint32_t seed, uint32_t* d_mismatches, vhStream_t stream);
/* Self-check of the colour step of VhHashParams::m_colorIntegration = 1 (the average weighted by the voxel weights): one
 * launch runs the device function over every (c0, w0, c1, w1) with w1 >= 1, 256 * 256 * 256 * 255 cases, against the
 * integer formula floor((2 (c0 w0 + c1 w1) + d) / (2 d)), d = w0 + w1, once with each reciprocal its callers hand it.
 * d_out: four words.  [0] mismatches with 1.0f / d (combineVoxel), [1] with the refined reciprocal of the pass's
 * certified blocks, [2] the first mismatching case as c0 | w0 << 8 | c1 << 16 | w1 << 24 (0xffffffff: none), [3] 0. */
int vh_debug_check_weighted_colour(uint32_t* d_out, vhStream_t stream);
/* The take-out rule of vh_deintegrate_blocks alone, on arrays of voxels: d_out[i] = d_observed[i] taken out of
 * d_stored[i] under hp's colour mode (an observation of weight 0 is no observation).  No camera is needed. */
int vh_debug_deintegrate_rule(const VhVoxel* d_stored, const VhVoxel* d_observed, VhVoxel* d_out, uint32_t n, const VhHashParams* hp, vhStream_t stream);
/* The per-voxel rule of vh_align_step alone: per voxel l of listed block b, record (b * 512 + l) of d_out, 37 words:
 * [0] 1 if the voxel contributes, else 0 and the rest 0; [1..4) q; [4] e; [5..8) g; [8..37) the 29 float terms. */
int vh_debug_align_rule(const VhHashData* dstHd, const VhHashParams* dstHp, const VhHashData* srcHd, const VhHashParams* srcHp, uint32_t n,
                        const VhSDFBlockDesc* d_srcDescs, const float* dstVoxFromSrcVox12, const float pivot3[3], float invRadius, float band,
                        float* d_out, vhStream_t stream);
/* measurement, not part of the path: every SIMD of the device runs `wavesPerSimd` waves (1..8), each a chain-free stream of
 * 32 * iters vector instructions (mode 0 v_fma_f32, 1 v_pk_fma_f32, 2 v_add_u32, 3 v_mul_lo_u32); per wave
 * {start, end in 100 MHz ticks, s_memtime ticks spent, HW_ID[19:0] | XCC_ID << 20} into d_stamps (4 words per wave, *numWaves waves: room for
 * 8 * 4 * the device's compute units).  tools/valu_issue_probe.py turns that into cycles per wave-instruction per SIMD */
int vh_debug_valu_probe(uint32_t mode, uint32_t wavesPerSimd, uint32_t iters, uint32_t* d_stamps, uint32_t* numWaves, vhStream_t stream);

/* ---- host classes (opaque handles over the C++ classes of include/vh.hpp) ---- */
typedef struct VhSceneRep VhSceneRep;   /* CUDASceneRepHashSDF,   DSC/CUDASceneRepHashSDF.h:28 */
typedef struct VhRayCast VhRayCast;     /* CUDARayCastSDF,        DSC/CUDARayCastSDF.h:13 */
typedef struct VhChunkGrid VhChunkGrid; /* CUDASceneRepChunkGrid, DSC/CUDASceneRepChunkGrid.h:152 */

/* CUDASceneRepHashSDF(const HashParams&) :31 ; the five GlobalAppState flags arrive as options */
int vh_scene_rep_create(const VhHashParams* hp, const VhSceneOptions* opt, vhStream_t stream, VhSceneRep** out);
void vh_scene_rep_destroy(VhSceneRep* s);
/* integrate(lastRigidTransform, depthCameraData, depthCameraParams, d_bitMask) :64 */
int vh_scene_rep_integrate(VhSceneRep* s, const float rigidTransform[16], const VhDepthCameraData* cam,
                           const VhDepthCameraParams* cp, const uint32_t* d_bitMask);
/* setLastRigidTransformAndCompactify :90 */
int vh_scene_rep_set_last_rigid_transform_and_compactify(VhSceneRep* s, const float rigidTransform[16],
                                                         const VhDepthCameraParams* cp);
/* reset() :101 */
int vh_scene_rep_reset(VhSceneRep* s);
/* getHashData() :112 / getHashParams() :116 / getLastRigidTransform() :96 */
int vh_scene_rep_get_hash_data(VhSceneRep* s, VhHashData* out);
int vh_scene_rep_get_hash_params(VhSceneRep* s, VhHashParams* out);
/* getHeapFreeCount() :122 (blocking read-back) */
int vh_scene_rep_get_heap_free_count(VhSceneRep* s, uint32_t* out);
/* blocking, exact count of in-frustum blocks of the last compactify */
int vh_scene_rep_get_num_occupied_blocks(VhSceneRep* s, uint32_t* out);
/* debugHash() :129-233: 0 if every invariant holds; report = {numOccupied, numFree, duplicates, lockEntries} */
int vh_scene_rep_debug_hash(VhSceneRep* s, uint32_t report[4]);
/* device-side status words (heap underflow, failed inserts, lost lock races): copies VH_STATE_WORDS words */
int vh_scene_rep_get_state(VhSceneRep* s, uint32_t* out);
/* per-stage device time in ms accumulated while s_timingsDetailledEnabled:
 * {alloc, compactify, integrate(+gc), count} (TimingLog of the reference) */
int vh_scene_rep_get_timings(VhSceneRep* s, double out[4]);
int vh_scene_rep_set_options(VhSceneRep* s, const VhSceneOptions* opt);
/* setColorIntegration (include/vh.hpp): how the following integrate() calls fuse colour.  VH_COLOR_RUNNING_AVERAGE (0), the
 * reference's running 50/50 average, or VH_COLOR_WEIGHTED_AVERAGE (1), weighted by the voxel weights; any other mode is
 * VH_ERR_BAD_ARGUMENT.  The mode is VhHashParams::m_colorIntegration of vh_scene_rep_get_hash_params. */
int vh_scene_rep_set_color_integration(VhSceneRep* s, uint32_t mode);
/* queryPoints (include/vh.hpp): vh_query_points on the scene's table and stream; device pointers, d_gradient3 may be NULL */
int vh_scene_rep_query_points(VhSceneRep* s, const float* d_points3, uint32_t n, float* d_sdf, uint32_t* d_color, float* d_gradient3,
                              uint8_t* d_valid);

/* mergeScene / mergeBlocks (include/vh.hpp): vh_merge_blocks on the scene's table and stream with a lock token of the
 * scene's, after which the compactified list is stale as after a stream-in (compactify before the next ray cast).
 * merge_scene takes every block resident in src's table (vh_merge_gather; src's stream is ordered before dst's by an
 * event) and reads its voxels in place; merge_blocks takes a block list in device memory (d_leftOut: device, n words,
 * may be NULL).  VH_ERR_BAD_ARGUMENT, and nothing done, when the two voxel sizes differ (merge_scene), dst == src, or
 * either scene is between integrateAhead and integrateFinish; VH_ERR_HEAP_EXHAUSTED, and nothing done, on
 * VH_MERGE_HEAP_SHORT.  Every other status returns VH_OK: it is in counts[VH_MERGE_STATUS].  counts is filled in
 * either case.  Blocking. */
int vh_scene_rep_merge_scene(VhSceneRep* dst, VhSceneRep* src, const int32_t blockOffset[3], uint32_t counts[VH_MERGE_NUM_COUNTS]);
int vh_scene_rep_merge_blocks(VhSceneRep* dst, const VhSDFBlockDesc* d_descs, const VhVoxel* d_blocks, uint32_t n, const int32_t blockOffset[3],
                              uint32_t* d_leftOut /* may be NULL */, uint32_t counts[VH_MERGE_NUM_COUNTS]);
/* mergeSceneTransformed (include/vh.hpp): src, in another world frame and possibly at another voxel size, sampled at
 * dst's voxel centres under dstFromSrc16 (rigid, 4x4 row-major doubles, metres: a point of src's frame in dst's) and
 * fused by the plain merge: vh_merge_gather on src, vh_resample_blocks (count, with a table that grows while it fills;
 * fill into a staging pool), vh_merge_blocks with the staging pool as its source.  dst is not written before the last
 * stage.  Only destination blocks with an observed voxel are merged (merge_scene allocates a block of unobserved voxels
 * too).  VH_ERR_BAD_ARGUMENT, and nothing done, for a matrix vh_resample_voxel_transforms refuses, voxel sizes further
 * apart than a factor of 2, dst == src, a frame in flight in either scene, or a resample status
 * (VH_RESAMPLE_OUT_OF_RANGE); VH_ERR_HEAP_EXHAUSTED, and nothing done, on VH_MERGE_HEAP_SHORT.  Both counts are filled
 * in either case.  Blocking; compactify before the next ray cast. */
int vh_scene_rep_merge_scene_transformed(VhSceneRep* dst, VhSceneRep* src, const double* dstFromSrc16, uint32_t mergeCounts[VH_MERGE_NUM_COUNTS],
                                         uint32_t resampleCounts[VH_RESAMPLE_NUM_COUNTS]);
/* alignScene (include/vh.hpp): the rigid transform that lays src onto dst, refined from guess16 on the device:
 * vh_merge_gather on src, vh_align_bounds and one read-back for the pivot and the radius, vh_align_begin, up to
 * options->maxIterations vh_align_step launches back to back, one read of the state into *result.  src's stream is
 * ordered before dst's, as for the merge.  Neither scene is written.  VH_ERR_BAD_ARGUMENT, with nothing done, for
 * src == dst, a guess or voxel sizes that vh_resample_voxel_transforms refuses, options that are not finite and positive
 * or beyond their bounds, a frame in flight, more than VH_ALIGN_MOST_BLOCKS source blocks.  How the registration ended
 * is in result->status. */
int vh_scene_rep_align_scene(VhSceneRep* dst, VhSceneRep* src, const double* guess16, const VhAlignOptions* options, VhAlignState* result);
/* eraseRegion / cropToRegion / extractRegion / moveRegionTo (include/vh.hpp): vh_cut_blocks on the blocks resident in
 * the scene's table (vh_merge_gather), on the scene's stream, with a lock token of the scene's own.  erase_region zeroes
 * the region's voxels and frees the blocks that hold nothing any more; crop_to_region does that to everything outside.
 * extract_region copies the region out and leaves the scene as it is: the blocks with an observed voxel in the region,
 * the voxels outside it zero, as a list for vh_scene_rep_merge_blocks in d_descs / d_blocks (device memory, room for
 * capacity blocks; block i at d_blocks[i * 512 ...]); *numBlocks receives their number.  With capacity 0 it only
 * counts (the pointers may be NULL); with too little room it returns VH_ERR_BAD_ARGUMENT, *numBlocks what is needed.
 * move_region_to extracts, merges the list into dst shifted by whole blocks (vh_scene_rep_merge_blocks) and then
 * erases the region from src -- but only if the merge left no block out: VH_ERR_HEAP_EXHAUSTED on VH_MERGE_HEAP_SHORT
 * (both scenes untouched), and with VH_MERGE_NO_SLOT / VH_MERGE_NOT_SETTLED in mergeCounts the call returns VH_OK with
 * src untouched and cutCounts[VH_CUT_VOXELS_ERASED] == 0: the caller decides.  All: VH_ERR_BAD_ARGUMENT, and nothing
 * done, for a region vh_cut_region_transform refuses, a shape that is none, a frame in flight (integrateAhead without
 * integrateFinish), and for the move dst == src and differing voxel sizes.  The counts are filled in either case.
 * Blocking; compactify before the next ray cast. */
int vh_scene_rep_erase_region(VhSceneRep* s, const VhCutRegion* region, uint32_t counts[VH_CUT_NUM_COUNTS]);
int vh_scene_rep_crop_to_region(VhSceneRep* s, const VhCutRegion* region, uint32_t counts[VH_CUT_NUM_COUNTS]);
int vh_scene_rep_extract_region(VhSceneRep* s, const VhCutRegion* region, VhSDFBlockDesc* d_descs, VhVoxel* d_blocks, uint32_t capacity,
                                uint32_t* numBlocks, uint32_t counts[VH_CUT_NUM_COUNTS]);
int vh_scene_rep_move_region_to(VhSceneRep* src, VhSceneRep* dst, const VhCutRegion* region, const int32_t blockOffset[3],
                                uint32_t cutCounts[VH_CUT_NUM_COUNTS], uint32_t mergeCounts[VH_MERGE_NUM_COUNTS]);
/* getNumIntegratedFrames (include/vh.hpp): the frames integrate() has fused; a de-integration does not change it */
int vh_scene_rep_get_num_integrated_frames(VhSceneRep* s, uint32_t* out);
/* *out = 1 between vh_scene_rep_integrate_ahead and vh_scene_rep_integrate_finish (a frame in flight: what merge, cut and
 * de-integration refuse), else 0 */
int vh_scene_rep_frame_in_flight(VhSceneRep* s, int* out);
/* deintegrate / reintegrate (include/vh.hpp): vh_deintegrate_blocks on the blocks resident in the scene's table
 * (vh_merge_gather), on the scene's stream, with a lock token of the scene's own and a copy of the hash parameters that
 * carries the frame's pose: the scene's last rigid transform and its frame count are not changed.  cam / cp: the maps
 * and the camera the frame was integrated with.  reintegrate is deintegrate at oldTransform followed by
 * vh_scene_rep_integrate at newTransform (which counts as a frame; d_bitMask as there).  VH_ERR_BAD_ARGUMENT, and nothing
 * done, for a frame in flight (integrateAhead without integrateFinish), a null depth or colour map and an image
 * without pixels.  The counts are filled in either case.  Blocking; compactify before the next ray cast. */
int vh_scene_rep_deintegrate(VhSceneRep* s, const float rigidTransform[16], const VhDepthCameraData* cam, const VhDepthCameraParams* cp,
                             uint32_t counts[VH_DEINT_NUM_COUNTS]);
int vh_scene_rep_reintegrate(VhSceneRep* s, const float oldTransform[16], const float newTransform[16], const VhDepthCameraData* cam,
                             const VhDepthCameraParams* cp, const uint32_t* d_bitMask, uint32_t counts[VH_DEINT_NUM_COUNTS]);

/* integrateAhead / integrateFinish: the two halves of integrate() (include/vh.hpp).  *job receives the frame's alloc +
 * compactify passes for vh_raycast_render_co (NULL when the scene's options rule a co-launch out); it belongs to the
 * scene and is valid until vh_scene_rep_integrate_finish */
int vh_scene_rep_integrate_ahead(VhSceneRep* s, const float rigidTransform[16], const VhDepthCameraData* cam,
                                 const VhDepthCameraParams* cp, const uint32_t* d_bitMask, VhFrameJob** job);
int vh_scene_rep_integrate_finish(VhSceneRep* s, const VhDepthCameraData* cam, const VhDepthCameraParams* cp);

/* CUDARayCastSDF(const RayCastParams&) :16 */
int vh_raycast_create(const VhRayCastParams* rp, vhStream_t stream, VhRayCast** out);
void vh_raycast_destroy(VhRayCast* r);
/* render(hashData, hashParams, cameraData, lastRigidTransform), DSC/CUDARayCastSDF.cpp:38 */
int vh_raycast_render(VhRayCast* r, const VhHashData* hd, const VhHashParams* hp,
                      const VhDepthCameraParams* cp, const float lastRigidTransform[16]);
/* the same with a frame job riding along (may be NULL) */
int vh_raycast_render_co(VhRayCast* r, const VhHashData* hd, const VhHashParams* hp,
                         const VhDepthCameraParams* cp, const float lastRigidTransform[16], VhFrameJob* job);
/* castRays (include/vh.hpp): vh_query_rays with the caster's own parameters on its stream; device pointers, d_normals3 may be NULL */
int vh_ray_cast_cast_rays(VhRayCast* r, const VhHashData* hd, const VhHashParams* hp, const float* d_origins3, const float* d_directions3,
                          const float* d_tMin, const float* d_tMax, uint32_t n, float* d_t, float* d_normals3, uint32_t* d_color,
                          uint8_t* d_status);
/* getRayCastData() :42 / getRayCastParams() :45 */
int vh_raycast_get_data(VhRayCast* r, VhRayCastData* out);
int vh_raycast_get_params(VhRayCast* r, VhRayCastParams* out);
/* device time in ms of render() accumulated while timing is enabled: {raycast (march kernel), normals, count,
 * interval splat} */
int vh_raycast_get_timings(VhRayCast* r, double out[4]);
/* ms an event pair reads with nothing between its two records (sampled while every stage is timed): what a bracketed
 * launch's reading holds beside the kernel */
int vh_raycast_get_event_pair_overhead(VhRayCast* r, double* ms);
int vh_raycast_set_timing(VhRayCast* r, int enabled); /* 0 off, 1 every stage, 2 the march kernel only */
/* same, timing only every stride-th render() (an event record idles the queue for a few microseconds) */
int vh_raycast_set_timing_stride(VhRayCast* r, int enabled, uint32_t stride);
/* 1 (default): render() splats ray intervals first; 0: march the full depth range as this fork of the reference does */
int vh_raycast_set_interval_splatting(VhRayCast* r, int enabled);
/* entries per tile list of the latest render() (VH_TILE_LIST_CAPACITY before the first): large from the second render
 * after a list outgrew the small tables, small again after more than 30 renders without one.  Read-only. */
int vh_raycast_get_tile_capacity(VhRayCast* r, uint32_t* out);

/* CUDASceneRepChunkGrid(sceneRep, voxelExtends, gridDimensions, minGridPos, initialChunkListSize,
 *                       streamingEnabled, streamOutParts)         DSC/CUDASceneRepChunkGrid.h:155 */
int vh_chunk_grid_create(VhSceneRep* s, const float voxelExtents[3], const int32_t gridDimensions[3],
                         const int32_t minGridPos[3], uint32_t initialChunkListSize, int streamingEnabled,
                         uint32_t streamOutParts, VhChunkGrid** out);
void vh_chunk_grid_destroy(VhChunkGrid* g);
/* streamOutToCPUPass0GPU(posCamera, radius, useParts, multiThreaded)  DSC/CUDASceneRepChunkGrid.cpp:55 */
int vh_chunk_grid_stream_out_to_cpu_pass0_gpu(VhChunkGrid* g, const float posCamera[3], float radius, int useParts, int multiThreaded);
/* streamOutToCPUPass1CPU(multiThreaded) :107 */
int vh_chunk_grid_stream_out_to_cpu_pass1_cpu(VhChunkGrid* g, int multiThreaded);
/* streamInToGPUPass0CPU(posCamera, radius, useParts, multiThreaded) :208 */
int vh_chunk_grid_stream_in_to_gpu_pass0_cpu(VhChunkGrid* g, const float posCamera[3], float radius, int useParts, int multiThreaded);
/* streamInToGPUPass1GPU(multiThreaded) :227 */
int vh_chunk_grid_stream_in_to_gpu_pass1_gpu(VhChunkGrid* g, int multiThreaded);
/* streamOutToCPU / streamInToGPU (both passes, single-threaded) :44 / :197 ; nStreamedBlocks out */
int vh_chunk_grid_stream_out_to_cpu(VhChunkGrid* g, const float posCamera[3], float radius, int useParts, uint32_t* nStreamedBlocks);
int vh_chunk_grid_stream_in_to_gpu(VhChunkGrid* g, const float posCamera[3], float radius, int useParts, uint32_t* nStreamedBlocks);
/* streamOutToCPUAll() :31 / streamInToGPUAll(posCamera, radius, useParts, n) :164 */
int vh_chunk_grid_stream_out_to_cpu_all(VhChunkGrid* g);
int vh_chunk_grid_stream_in_to_gpu_all(VhChunkGrid* g, const float posCamera[3], float radius, int useParts, uint32_t* nStreamedBlocks);
/* getBitMaskGPU() DSC/CUDASceneRepChunkGrid.h:306 (uploads only when the mask changed) */
int vh_chunk_grid_get_bit_mask_gpu(VhChunkGrid* g, const uint32_t** d_bitMask);
/* Read-only, for tests: both copies of the bit mask as they stand once the streaming pipeline is drained and before any
 * upload of the host's copy.  hostCopy / deviceCopy: `words` words each (either may be NULL); *wordsOut: the mask's size
 * in words ((bits + 31) / 32), and nothing is copied if `words` is smaller; *hostDirty: 1 if the host's copy was marked
 * as changed since the last upload (getBitMaskGPU() would copy it to the device). */
int vh_chunk_grid_debug_download_bit_masks(VhChunkGrid* g, uint32_t* hostCopy, uint32_t* deviceCopy, uint32_t words,
                                           uint32_t* wordsOut, int32_t* hostDirty);
/* reset() :297 */
int vh_chunk_grid_reset(VhChunkGrid* g);
/* debugCheckForDuplicates() DSC/CUDASceneRepChunkGrid.cpp:313: 0 if no block is present twice */
int vh_chunk_grid_debug_check_for_duplicates(VhChunkGrid* g);
/* host-side statistics: {chunks allocated, blocks on the host, bits set} */
int vh_chunk_grid_get_statistics(VhChunkGrid* g, uint32_t out[3]);
/* blocks that stream-in passes could not insert (bucket and list full, or a second overflow of one bucket in a pass) and
 * that went back to the host grid for a later pass; not in the reference, which has no defined behaviour there */
int vh_chunk_grid_get_num_failed_inserts(VhChunkGrid* g, uint32_t* out);
/* copies the host chunk grid content: descs[n], blocks[n*512] (pass NULL to query n) */
int vh_chunk_grid_download_host_blocks(VhChunkGrid* g, VhSDFBlockDesc* descs, VhVoxel* blocks, uint32_t capacity, uint32_t* n);
/* saveToFile / loadFromFile (.hashgrid v1) DSC/CUDASceneRepChunkGrid.h:459-548 */
int vh_chunk_grid_save_to_file(VhChunkGrid* g, const char* filename, const float camPos[3], float radius);
int vh_chunk_grid_load_from_file(VhChunkGrid* g, const char* filename, const float camPos[3], float radius);

/* ---- the frame loop: reconstruction(), DSC/DepthSensing.cpp:720-924, headless over a recorded sequence at given
 * poses ("build's headless vh_bench / vh_replay driver").  Per frame, in the reference's order:
 * render(pose of the previous frame) -> [stream out / stream in around the camera] -> integrate(pose, depth, colour,
 * bit mask).  One call enqueues any number of frames; nothing in it waits for the device unless streaming is on (its
 * read-backs) or the run-ahead bound is reached.  The scene, the ray caster and the chunk grid stay the caller's. */
typedef struct VhReconstruction VhReconstruction;
void vh_reconstruction_default_options(VhReconstructionOptions* out);
int vh_reconstruction_create(VhSceneRep* scene, VhRayCast* rayCast, VhChunkGrid* chunkGrid /* may be NULL */,
                             const VhDepthCameraParams* cp, const VhReconstructionOptions* opt, VhReconstruction** out);
void vh_reconstruction_destroy(VhReconstruction* r);
/* processes frames[0..n): frame numbers continue from the previous call (the first frame of all is not ray-cast) */
int vh_reconstruction_run(VhReconstruction* r, const VhSequenceFrame* frames, uint32_t n);
/* the same for a caller that feeds the loop a few frames at a time and knows what comes next: `next` is the frame that
 * will follow frames[n-1] (only its pose is read; NULL: unknown).  With streaming on, the loop then asks the device
 * about that frame's streaming step behind the last frame's alloc pass, as it does inside a call (not in the reference) */
int vh_reconstruction_run_ahead(VhReconstruction* r, const VhSequenceFrame* frames, uint32_t n, const VhSequenceFrame* next);
/* raw frames (VhRawFrameFormat, VhRawSequenceFrame in vh_types.h): 16-bit depth and 8-bit colour at the sensor's sizes,
 * in host memory (s_framesOnHost = 1: copied by the loop's two copy streams) or in device memory (0: read in place).
 * The format is set once, before the first frame; the loop's copy stream turns every frame into float maps at adapter
 * size in a staging slot (vh_ingest_frame, then the Gauss filters that are on) beside the previous frames' work.
 * Raw and prepared frames may not be mixed in one loop. */
int vh_reconstruction_set_raw_format(VhReconstruction* r, const VhRawFrameFormat* format);
int vh_reconstruction_run_raw(VhReconstruction* r, const VhRawSequenceFrame* frames, uint32_t n);
int vh_reconstruction_run_raw_ahead(VhReconstruction* r, const VhRawSequenceFrame* frames, uint32_t n, const VhRawSequenceFrame* next);
/* Camera tracking inside the loop (plain projective ICP, CUDACameraTrackingMultiRes): once, before the first frame;
 * needs a ray caster, s_renderEnabled and a pyramid of settings->s_maxLevels levels that the adapter size can hold.
 * From then on the rigidTransform of the frames is ignored and every frame does what reconstruction() does with
 * s_binaryDumpSensorUseTrajectory = false, s_trackingEnabled = true (DSC/DepthSensing.cpp:750-879): frame 0 at the
 * identity; later frames ray-cast the model at the scene's last pose, align the input to it from the identity estimate
 * (one vh_icp_step per outer iteration on levels with s_maxInnerIter = 1) and integrate at lastRigidTransform * delta.  A
 * frame on which tracking is lost is not integrated (vh_reconstruction_get_tracking_stats).  The host waits once per tracked frame, for the ICP
 * result in mapped host memory; it makes no blocking HIP call. */
int vh_reconstruction_set_tracking(VhReconstruction* r, const VhTrackingState* settings);
/* The same with the RGB-D tracker (depth + photometric ICP, CUDACameraTrackingMultiResRGBD; one vh_icp_rgbd_step per
 * outer iteration) in place of the plain one: once, before the first frame, and one of the two only (either after the
 * other is VH_ERR_BAD_ARGUMENT).  Same preconditions.  The intensity pyramid of the input is made from the frame's float4
 * colour map (the staging slot's after ingest and the colour filter, or the caller's for resident frames) on the copy
 * stream, the model's from the ray cast's colours on the loop's stream.  Every frame needs a colour map: a frame without
 * one, or a raw format with colorChannels = 0, is VH_ERR_BAD_ARGUMENT. */
int vh_reconstruction_set_tracking_rgbd(VhReconstruction* r, const VhTrackingStateRGBD* settings);
/* the poses of frames [first, first + n) fed since creation / reset, 16 floats each: the pose the frame was integrated
 * at; every entry -inf for a frame that was not (tracking lost, invalid recorded pose).  Untracked loops report the
 * recorded poses.  Waits for nothing: the poses are the host's. */
int vh_reconstruction_get_poses(VhReconstruction* r, uint32_t first, uint32_t n, float* out);
/* trackedFrames: frames whose pose came from ICP inside the loop and that were integrated; lostFrames: frames on which
 * that tracking was lost (not integrated, the scene keeps its last pose).  Since creation / reset; both 0 without
 * tracking.  They are not members of VhReconstructionStats because its size is pinned (tests/test_raw_frames_host.py):
 * engine.Reconstruction.getStats() reports them beside its members. */
int vh_reconstruction_get_tracking_stats(VhReconstruction* r, uint64_t* trackedFrames, uint64_t* lostFrames);
/* waits for everything the loop has enqueued (all its streams) */
int vh_reconstruction_synchronize(VhReconstruction* r);
int vh_reconstruction_get_stats(VhReconstruction* r, VhReconstructionStats* out);
/* test hook: the n-th ray cast from now fails with an error instead of running (0: off); the loop must unwind cleanly */
int vh_reconstruction_debug_fail_render(VhReconstruction* r, uint32_t nthRenderFromNow);
/* frame counter and statistics back to zero (the scene is the caller's to reset) */
int vh_reconstruction_reset(VhReconstruction* r);

/* ---- sensor pre-processing: the image kernels of DSC/CameraUtil.cu that CUDARGBDAdapter::process
 * (DSC/CUDARGBDAdapter.cpp:93-137) and CUDARGBDSensor::process (DSC/CUDARGBDSensor.cpp:147-257) run on every frame.
 * Device pointers; float4 maps are passed as float* (4 per pixel); MINF marks an invalid pixel.  The filters read
 * their whole neighbourhood, so they do not work in place. */
int vh_convert_color_raw_to_float4(float* d_output4, const uint8_t* d_inputRGBX, uint32_t width, uint32_t height, vhStream_t stream); /* :154 */
/* not in the reference: a raw sensor frame in device memory (16-bit depth in units of 1/depthShift m; colorChannels = 3: RGB,
 * 4: RGBX, 0: no colour, then d_color4 / d_colorRaw may be NULL) to float depth + float4 colour at width x height in one
 * pass: SensorDataReader::processDepth's conversion, vh_convert_color_raw_to_float4, vh_resample_float_map and
 * vh_resample_float4_map (the colour is copied, not resampled, when its size is width x height), bit for bit.  All sizes
 * at least 2 x 2; d_depth and d_color4 16-byte aligned, RGBX colour 4-byte aligned. */
int vh_ingest_frame(float* d_depth, float* d_color4, uint32_t width, uint32_t height, const uint16_t* d_depthRaw, uint32_t depthWidth,
                    uint32_t depthHeight, const uint8_t* d_colorRaw, uint32_t colorWidth, uint32_t colorHeight, uint32_t colorChannels,
                    float depthShift, vhStream_t stream);
int vh_resample_float_map(float* d_output, uint32_t outputWidth, uint32_t outputHeight, const float* d_input,
                          uint32_t inputWidth, uint32_t inputHeight, vhStream_t stream);                                       /* :1120 */
int vh_resample_float4_map(float* d_output4, uint32_t outputWidth, uint32_t outputHeight, const float* d_input4,
                           uint32_t inputWidth, uint32_t inputHeight, vhStream_t stream);                                      /* :1188 */
int vh_copy_float_map(float* d_output, const float* d_input, uint32_t width, uint32_t height, vhStream_t stream);              /* :37  */
int vh_copy_float4_map(float* d_output4, const float* d_input4, uint32_t width, uint32_t height, vhStream_t stream);           /* :120 */
int vh_set_invalid_float_map(float* d_output, uint32_t width, uint32_t height, vhStream_t stream);                             /* :348 */
int vh_convert_color_to_intensity_float(float* d_output, const float* d_input4, uint32_t width, uint32_t height, vhStream_t stream); /* :269 */
int vh_convert_depth_float_to_camera_space_float4(float* d_output4, const float* d_input, const VhDepthCameraParams* cp,
                                                  uint32_t width, uint32_t height, vhStream_t stream);                         /* :409 */
int vh_gauss_filter_float_map(float* d_output, const float* d_input, float sigmaD, float sigmaR, uint32_t width, uint32_t height, vhStream_t stream);    /* :595 */
int vh_gauss_filter_float4_map(float* d_output4, const float* d_input4, float sigmaD, float sigmaR, uint32_t width, uint32_t height, vhStream_t stream); /* :653 */
int vh_bilateral_filter_float_map(float* d_output, const float* d_input, float sigmaD, float sigmaR, uint32_t width, uint32_t height, vhStream_t stream); /* :485 */
int vh_erode_depth_map(float* d_output, const float* d_input, int32_t structureSize, uint32_t width, uint32_t height, float dThresh,
                       float fracReq, vhStream_t stream);                                                                       /* :1672 */

/* ---- parameter files: zParameters*.txt as mLib's ParameterFile reads them
 * (DSCroot/Include/mLib/include/core-util/parameterFile.h:22-60,136-172: per line, cut at the first "//", "#" or ";",
 * strip blanks / quotes / semicolons, split at the first "="; numbers by stoi / stof, bool false iff "false", "False" or
 * "0") and the parametersFromGlobalAppState builders of the host classes. */
int vh_app_state_read(const char* filename, VhAppState* out);
int vh_app_state_parse(const char* text, VhAppState* out); /* the same on a string */
void vh_hash_params_from_app_state(const VhAppState* gas, VhHashParams* out);        /* DSC/CUDASceneRepHashSDF.h:38-58 */
void vh_raycast_params_from_app_state(const VhAppState* gas, const float intrinsics[16], const float intrinsicsInv[16],
                                      VhRayCastParams* out);                          /* DSC/CUDARayCastSDF.h:24-40 */
void vh_marching_cubes_params_from_app_state(const VhAppState* gas, VhMarchingCubesParams* out); /* DSC/CUDAMarchingCubesHashSDF.h:19-28 */
void vh_scene_options_from_app_state(const VhAppState* gas, VhSceneOptions* out);

/* handle level: CUDARGBDSensor over CUDARGBDAdapter (include/vh.hpp).  config = {depthW, depthH, colorW, colorH, adapterW,
 * adapterH} and {fx, fy, mx, my, sensorDepthMin, sensorDepthMax}. */
typedef struct VhRGBDSensor VhRGBDSensor;
int vh_rgbd_sensor_create(const uint32_t sizes[6], const float intrinsics[6], vhStream_t stream, VhRGBDSensor** out);
void vh_rgbd_sensor_destroy(VhRGBDSensor* s);
int vh_rgbd_sensor_set_filter_depth_values(VhRGBDSensor* s, int enabled, float sigmaD, float sigmaR);
int vh_rgbd_sensor_set_filter_intensity_values(VhRGBDSensor* s, int enabled, float sigmaD, float sigmaR);
int vh_rgbd_sensor_process(VhRGBDSensor* s, const float* h_depthFloat, const uint8_t* h_colorRGBX);
int vh_rgbd_sensor_get_depth_camera_data(VhRGBDSensor* s, VhDepthCameraData* out);
int vh_rgbd_sensor_get_depth_camera_params(VhRGBDSensor* s, VhDepthCameraParams* out);
/* device maps at adapter resolution: {camera space float4, normals float4, intensity float} */
int vh_rgbd_sensor_get_maps(VhRGBDSensor* s, float** d_cameraSpace4, float** d_normals4, float** d_intensity);
/* s_bUseCameraCalibration (DSC/CUDARGBDSensor.cpp:198-217): process() renders the (filtered) depth map into the colour
 * camera with vh_view_raster + vh_view_resolve_depth instead of copying it.  colorIntrinsics = {fx, fy, mx, my} at the
 * colour sensor's resolution; depthExtrinsics (row-major) is the modelview; the thresholds are
 * s_remappingDepthDiscontinuityThres{Offset,Lin}.  An identity extrinsic leaves it off (RGBDSensor.cpp:150-153). */
int vh_rgbd_sensor_set_camera_calibration(VhRGBDSensor* s, int enabled, const float colorIntrinsics[4], const float depthExtrinsics[16],
                                          float thresOffset, float thresLin);
/* host only: the VhViewParams of that remap.  sizes as vh_rgbd_sensor_create's; depthIntrinsics / colorIntrinsics =
 * {fx, fy, mx, my} at the sensors' resolutions.  The adapter rescales both to the adapter size; intrinsicInverse is
 * the inverse of the adapter's depth intrinsics (cofactors, mLib's order), modelview the extrinsic as given, screen =
 * depth map = adapter size. */
int vh_rgbd_sensor_remap_params(const uint32_t sizes[6], const float depthIntrinsics[4], const float colorIntrinsics[4], const float depthExtrinsics[16],
                                float thresOffset, float thresLin, VhViewParams* out);
/* whether the remap is on, and the VhViewParams process() draws with (adapter matrices; may be NULL) */
int vh_rgbd_sensor_get_camera_calibration(VhRGBDSensor* s, int* enabled, VhViewParams* params);

/* ---- recorded sequences: the `.sens` container and its reader.
 *   VhSensorData        ml::SensorData (load / save / frames)          DSC/sensorData/sensorData.h:608-830
 *   VhSensorDataReader  SensorDataReader (the sensor the loop polls)    DSC/SensorDataReader.cpp:39-179
 * Host side only; depth raw / zlib, colour raw / PNG / baseline JPEG are decoded (see vh_sensor_data.cpp). */
typedef struct VhSensorData VhSensorData;
int vh_sensor_data_create(const VhSensorDataInfo* header, VhSensorData** out); /* empty sequence with this header */
int vh_sensor_data_load(const char* filename, VhSensorData** out);             /* loadFromFile :789-830 */
void vh_sensor_data_destroy(VhSensorData* s);
int vh_sensor_data_save(const VhSensorData* s, const char* filename);          /* saveToFile :756-787 */
int vh_sensor_data_info(const VhSensorData* s, VhSensorDataInfo* out);
/* addFrame :657-667.  colorRGB (3 bytes / pixel) or depth may be NULL; stored with the header's compression types
 * (depth raw / zlib, colour raw). */
int vh_sensor_data_add_frame(VhSensorData* s, const uint8_t* colorRGB, const uint16_t* depth, const float cameraToWorld[16],
                             uint64_t timeStampColor, uint64_t timeStampDepth);
/* stores an already compressed colour frame (PNG / JPEG bytes as another tool produced them) with the frame's depth */
int vh_sensor_data_add_frame_compressed(VhSensorData* s, const uint8_t* colorBytes, uint64_t numColorBytes, const uint16_t* depth,
                                        const float cameraToWorld[16], uint64_t timeStampColor, uint64_t timeStampDepth);
int vh_sensor_data_add_imu_frame(VhSensorData* s, const double values15[15], uint64_t timeStamp);
/* decompressDepthAlloc / decompressColorAlloc :687-705 and the frame's pose and time stamps; any output may be NULL */
int vh_sensor_data_get_frame(const VhSensorData* s, uint64_t frameIdx, uint16_t* depth, uint8_t* colorRGB, float cameraToWorld[16],
                             uint64_t timeStamps[2]);

typedef struct VhSensorDataReader VhSensorDataReader;
int vh_sensor_data_reader_create(const char* filename, VhSensorDataReader** out); /* createFirstConnected */
void vh_sensor_data_reader_destroy(VhSensorDataReader* r);
int vh_sensor_data_reader_info(const VhSensorDataReader* r, VhSensorDataInfo* out);
/* processDepth: decodes the next frame.  *gotFrame = 0 once the sequence is complete.  The pointers stay valid until
 * the next call: depth in metres (depthWidth*depthHeight floats), colour {r, g, b, 1} (colorWidth*colorHeight*4). */
int vh_sensor_data_reader_process_depth(VhSensorDataReader* r, int* gotFrame, const float** depthFloat, const uint8_t** colorRGBX);
int vh_sensor_data_reader_get_rigid_transform(const VhSensorDataReader* r, int offset, float out[16]); /* getRigidTransform :172-179 */
int vh_sensor_data_reader_get_curr_frame(const VhSensorDataReader* r, uint32_t* currFrame, uint32_t* numFrames);

/* ---- projective ICP camera tracking.  Launcher level: the steps of one alignment, each a kernel
 * that reads and updates a VhIcpState in device memory (a step returns at once when the state says "lost" or "level
 * done"), so that a whole multi-resolution solve runs without a host round trip.
 *   vh_icp_projective_correspondences  projectiveCorrespondences           DSC/CUDAImageHelper.cu:70-145
 *   vh_icp_build_linear_system         buildLinearSystem (per-wave terms)  DSC/CUDABuildLinearSystem.cu:130-204
 *   vh_icp_solve                       reductionSystemCPU + computeBestRigidAlignment + delinearizeTransformation +
 *                                      the early-out of align               DSC/CUDABuildLinearSystem.cpp:52-92,
 *                                                                           DSC/CUDACameraTrackingMultiRes.cpp:186-253,306-318 */
int vh_icp_begin(VhIcpState* d_state, const float* d_deltaEstimate16, vhStream_t stream);
int vh_icp_begin_level(VhIcpState* d_state, vhStream_t stream);
int vh_icp_projective_correspondences(const float* d_input4, const float* d_inputNormals4, const float* d_target4, const float* d_targetNormals4,
                                      float* d_output4, float* d_outputNormals4, uint32_t width, uint32_t height, float distThres, float normalThres,
                                      float levelFactor, const VhIcpState* d_state, const VhDepthCameraParams* cp, vhStream_t stream);
uint32_t vh_icp_num_partials(uint32_t width, uint32_t height); /* rows of 30 floats vh_icp_build_linear_system writes */
int vh_icp_build_linear_system(uint32_t width, uint32_t height, float* d_partials, const float* d_input4, const float* d_corr4,
                               const float* d_corrNormals4, const VhIcpState* d_state, vhStream_t stream);
int vh_icp_solve(VhIcpState* d_state, const float* d_partials, uint32_t numPartials, float angleThres, float distThres, float earlyOutResidual,
                 int lastInnerIteration, vhStream_t stream);
/* One outer iteration of a level whose s_maxInnerIter is 1 in ONE launch: what vh_icp_projective_correspondences +
 * vh_icp_build_linear_system + vh_icp_solve(lastInnerIteration = 1) do, the VhIcpState afterwards equal to theirs bit
 * for bit; no correspondence maps.  d_partials: 30 * vh_icp_num_partials(width, height) floats.  d_ticket: a device word
 * of the caller's that is 0 before every launch -- clear it on the stream (vh_memset) where vh_icp_begin runs; the step
 * leaves it 0.  publish (may be NULL): mapped host memory that receives the state's result after this step, its tag
 * last (VhIcpResult); a step the state skips (lost / level done) publishes the state as it stands. */
int vh_icp_step(const float* d_input4, const float* d_inputNormals4, const float* d_target4, const float* d_targetNormals4, uint32_t width, uint32_t height,
                float distThres, float normalThres, float levelFactor, const VhDepthCameraParams* cp, float* d_partials, uint32_t* d_ticket,
                VhIcpState* d_state, float angleTransThres, float distTransThres, float earlyOutResidual, VhIcpResult* publish, uint32_t tag, vhStream_t stream);
/* the same publication by a one-wave kernel, for a solve whose last step is not a vh_icp_step */
int vh_icp_publish(const VhIcpState* d_state, VhIcpResult* publish, uint32_t tag, vhStream_t stream);
/* GlobalCameraTrackingState::readMembers on zParametersTracking*.txt (DSC/GlobalCameraTrackingState.h:14-60) */
int vh_tracking_state_read(const char* filename, VhTrackingState* out);
int vh_tracking_state_parse(const char* text, VhTrackingState* out);

/* handle level: CUDACameraTrackingMultiRes (DSC/CUDACameraTrackingMultiRes.h:17-78) */
typedef struct VhCameraTracking VhCameraTracking;
int vh_camera_tracking_create(uint32_t imageWidth, uint32_t imageHeight, uint32_t levels, vhStream_t stream, VhCameraTracking** out);
void vh_camera_tracking_destroy(VhCameraTracking* t);
/* applyCT(dInput, dInputNormals, -, dModel, dModelNormals, -, lastTransform, <per-level settings>, condThres, angleThres,
 * deltaTransformEstimate, ...) :241-289: returns lastTransform * delta in transformOut, every entry -inf if tracking was lost
 * (trackingLost = 1).  state (may be NULL) receives the final VhIcpState. */
int vh_camera_tracking_apply_ct(VhCameraTracking* t, float* d_input4, float* d_inputNormals4, float* d_model4, float* d_modelNormals4,
                                const float lastTransform[16], const VhTrackingState* settings, const float deltaTransformEstimate[16],
                                const VhDepthCameraParams* cp, float transformOut[16], int* trackingLost, VhIcpState* state);

/* ---- RGB-D camera tracking: depth + photometric multi-resolution ICP (CUDACameraTrackingMultiResRGBD).  Launcher
 * level, in the style of the f5 block above; a level starts with vh_icp_begin_level(&d_state->icp), and every
 * vh_icp_rgbd_solve is one outer iteration of align (the reference's RGB-D align has no inner loop).
 *   vh_compute_intensity_and_derivatives  computeIntensityAndDerivatives        DSC/CameraUtil.cu:1492-1538
 *   vh_icp_rgbd_build_linear_system       computeNormalEquations (per-wave terms) DSC/CUDABuildLinearSystemRGBD.cu:106-220
 *   vh_icp_rgbd_solve                     reductionSystemCPU + computeBestRigidAlignment + delinearizeTransformation +
 *                                         checkRigidTransformation + the early-out of align
 *                                                                        DSC/CUDABuildLinearSystemRGBD.cpp:46-86,
 *                                                                        DSC/CUDACameraTrackingMultiResRGBD.cpp:166-237,329-350 */
int vh_compute_intensity_and_derivatives(const float* d_intensity, uint32_t width, uint32_t height, float* d_intensityAndDerivatives4, vhStream_t stream);
int vh_icp_rgbd_begin(VhIcpStateRGBD* d_state, const float* d_deltaEstimate16, vhStream_t stream);
uint32_t vh_icp_rgbd_num_partials(uint32_t width, uint32_t height, uint32_t level); /* rows of 30 floats the build step writes */
int vh_icp_rgbd_build_linear_system(uint32_t width, uint32_t height, float* d_partials, const float* d_input4, const float* d_inputNormals4,
                                    const float* d_inputIntensity, const float* d_target4, const float* d_targetNormals4,
                                    const float* d_targetIntensityAndDerivatives4, const VhIcpRGBDParams* params, const VhIcpStateRGBD* d_state,
                                    vhStream_t stream);
int vh_icp_rgbd_solve(VhIcpStateRGBD* d_state, const float* d_partials, uint32_t numPartials, float angleThres, float distThres, float earlyOutResidual,
                      vhStream_t stream);
/* One outer iteration of the RGB-D align in ONE launch: what vh_icp_rgbd_build_linear_system + vh_icp_rgbd_solve do, the
 * VhIcpStateRGBD afterwards equal to theirs bit for bit.  d_partials: 30 * vh_icp_rgbd_num_partials(width, height,
 * params->level) floats.  d_ticket: a device word of the caller's that is 0 before every launch -- clear it on the stream
 * (vh_memset) where vh_icp_rgbd_begin runs; the step leaves it 0.  publish (may be NULL): mapped host memory that
 * receives d_state->icp's result after this step, its tag last (VhIcpResult); a step the state skips (lost / level done)
 * publishes the state as it stands.  A solve whose last step is not this one publishes with
 * vh_icp_publish(&d_state->icp, ...). */
int vh_icp_rgbd_step(uint32_t width, uint32_t height, float* d_partials, uint32_t* d_ticket, const float* d_input4, const float* d_inputNormals4,
                     const float* d_inputIntensity, const float* d_target4, const float* d_targetNormals4, const float* d_targetIntensityAndDerivatives4,
                     const VhIcpRGBDParams* params, VhIcpStateRGBD* d_state, float angleThres, float distThres, float earlyOutResidual, VhIcpResult* publish,
                     uint32_t tag, vhStream_t stream);
/* GlobalCameraTrackingState::readMembers with the four RGB-D keys (s_weightsDepth, s_weightsColor, s_colorGradientMin,
 * s_colorThres); the other members exactly as vh_tracking_state_read returns them */
int vh_tracking_state_rgbd_read(const char* filename, VhTrackingStateRGBD* out);
int vh_tracking_state_rgbd_parse(const char* text, VhTrackingStateRGBD* out);

/* handle level: CUDACameraTrackingMultiResRGBD (DSC/CUDACameraTrackingMultiResRGBD.h:23-75) */
typedef struct VhCameraTrackingRGBD VhCameraTrackingRGBD;
int vh_camera_tracking_rgbd_create(uint32_t imageWidth, uint32_t imageHeight, uint32_t levels, vhStream_t stream, VhCameraTrackingRGBD** out);
void vh_camera_tracking_rgbd_destroy(VhCameraTrackingRGBD* t);
/* applyCT(dInputPos, dInputNormal, dInputColor, dTargetPos, dTargetNormal, dTargetColor, lastTransform, <per-level
 * settings>, deltaTransformEstimate, ...) :239-327.  The input colour is the sensor's float4 colour map (what
 * integrate() reads), the target maps are the ray caster's d_depth4, d_normals and d_colors.  Returns
 * lastTransform * delta in transformOut, every entry -inf if tracking was lost (trackingLost = 1); state (may be NULL)
 * receives the final VhIcpStateRGBD. */
int vh_camera_tracking_rgbd_apply_ct(VhCameraTrackingRGBD* t, float* d_input4, float* d_inputNormals4, float* d_inputColor4, float* d_model4,
                                     float* d_modelNormals4, float* d_modelColor4, const float lastTransform[16], const VhTrackingStateRGBD* settings,
                                     const float deltaTransformEstimate[16], const VhDepthCameraParams* cp, float transformOut[16], int* trackingLost,
                                     VhIcpStateRGBD* state);

/* ---- marching cubes -------------------------------------------------------------------------
 * launcher level: resetMarchingCubesCUDA / extractIsoSurfacePass1CUDA / extractIsoSurfacePass2CUDA
 * (DSC/CUDAMarchingCubesSDF.cu:29-40, 94-105, 132-143).  The reference passes a RayCastData only for its member
 * function trilinearInterpolationSimpleFastFast; no buffer of it is read, so it is not a parameter here.
 * d_numTriangles counts every triangle produced; those beyond m_maxNumTriangles are dropped (the reference clamps
 * the counter instead). */
int vh_marching_cubes_data_alloc(VhMarchingCubesData* data, const VhMarchingCubesParams* params); /* MarchingCubesData::allocate */
void vh_marching_cubes_data_free(VhMarchingCubesData* data);
int vh_marching_cubes_update_params(const VhMarchingCubesData* data, const VhMarchingCubesParams* params, vhStream_t stream);
int vh_reset_marching_cubes(const VhMarchingCubesData* data, vhStream_t stream);
int vh_extract_iso_surface_pass1(const VhHashData* hd, const VhHashParams* hp, const VhMarchingCubesData* data, vhStream_t stream);
int vh_extract_iso_surface_pass2(const VhHashData* hd, const VhHashParams* hp, const VhMarchingCubesData* data,
                                 uint32_t numOccupiedBlocks, vhStream_t stream);
/* Pass 2 that also records where each triangle came from (not in the reference): the same triangles as
 * vh_extract_iso_surface_pass2, and beside triangle i of data->d_triangles the record d_sources[i].
 *   d_sources          device, m_maxNumTriangles records (triangles beyond that are dropped, and so are their records)
 *   numOccupiedBlocks  what pass 1 counted (0: nothing is launched) */
int vh_extract_iso_surface_pass2_sourced(const VhHashData* hd, const VhHashParams* hp, const VhMarchingCubesData* data,
                                         VhTriangleSource* d_sources, uint32_t numOccupiedBlocks, vhStream_t stream);

/* ---- live mesh: the sourced soup kept on the device and brought up to date (csrc/vh_live_mesh.hip; DESIGN.md section 4,
 * "Live mesh"; not in the reference).  The cache is data->d_triangles with the records *d_sources beside it and
 * data->d_numTriangles its count; one update makes it, as a set of (triangle, record) pairs, what reset, pass 1 and the
 * sourced pass 2 without a box would give on the same table, and runs pass 2 only over the resident blocks within one
 * block of a block whose voxels, position or presence changed since the last update.  What changed is found from the
 * table and the pool alone, by a 64-bit digest per block (vh_live_mesh_digest): a changed block is missed only where
 * two contents of one block share a digest; vh_live_mesh_reset makes the next update a full one.
 * Buffers for a pool of numSDFBlocks blocks (below 2^22) and a cache of maxNumTriangles: 64 B per block (record, two
 * positions, mark, list entry) and 88 B per triangle for the spare pair. */
int vh_live_mesh_data_alloc(VhLiveMeshData* live, uint32_t numSDFBlocks, uint32_t maxNumTriangles);
void vh_live_mesh_data_free(VhLiveMeshData* live);
/* invalidate: forgets every record and the cache, so that the next update re-extracts everything.  Asynchronous. */
int vh_live_mesh_reset(VhLiveMeshData* live, vhStream_t stream);
/* One update.  Waits once for the device, for the size of pass 2's grid.
 *   data       its d_params must hold the thresholds of the earlier updates, m_boxEnabled 0 and the m_maxNumTriangles of
 *              `live`; its block list and its counters are overwritten.  data->d_triangles and *d_sources are rewritten to
 *              name the buffers that hold the cache afterwards: the drop pass compacts into live's spare pair, which
 *              then changes places with them (all four are allocations of the same size, freed by whoever holds them)
 *   live       from vh_live_mesh_data_alloc with hp->m_numSDFBlocks and that m_maxNumTriangles
 * VH_ERR_BAD_ARGUMENT, with nothing launched and the cache as it was, when hp's bucket count, list limit or voxel size
 * differ from those of the updates since the last reset.  What the device finds -- an overflow, a block out of range --
 * is a status that vh_live_mesh_get_counts reports. */
int vh_live_mesh_update(const VhHashData* hd, const VhHashParams* hp, VhMarchingCubesData* data, VhTriangleSource** d_sources, VhLiveMeshData* live,
                        vhStream_t stream);
/* Waits for the update and reads the VH_LIVE_NUM_COUNTS counts and, in out[VH_LIVE_NUM_COUNTS], the status.  out is
 * filled whenever the copy succeeded; the return value restates the status: VH_ERR_STAGING_OVERFLOW for
 * VH_LIVE_OVERFLOW, VH_ERR_BAD_ARGUMENT for VH_LIVE_RANGE and VH_LIVE_BAD_TABLE.  After a status the cache and every
 * record are invalid (the device has seen to it): the next update starts from nothing. */
int vh_live_mesh_get_counts(const VhLiveMeshData* live, uint32_t out[9], vhStream_t stream);
/* The digest alone: d_out[i] for the block of hash entry d_entryIndices[i] (device arrays of n), 0 for a free entry or an
 * index outside the table.  With w_j the 8 bytes of voxel j (0 .. 511, memory order) as a little-endian 64-bit word:
 * the sum over j of fmix64(w_j + (j + 1) * 0x9E3779B97F4A7C15) modulo 2^64, fmix64 the finaliser of MurmurHash3. */
int vh_live_mesh_digest(const VhHashData* hd, const VhHashParams* hp, const uint32_t* d_entryIndices, uint32_t n, uint64_t* d_out, vhStream_t stream);

/* ---- indexed mesh: the soup welded on the device (csrc/vh_mesh.hip; DESIGN.md section 4, "Indexed mesh") -----------
 * The key a vertex is welded under: three 20-bit lattice coordinates biased by 2^19 (x in bits 0-19, y 20-39, z 40-59)
 * and a code in bits 60-61 (the lattice edge's axis, or 3 for a lattice point); bits 62-63 are 0.
 *   cell   voxel coordinates of the cell          edge  0..11, the order of vertlist
 *   snap   0 interpolated, 1 at the edge's first end point, 2 at its second
 * VH_ERR_BAD_ARGUMENT when edge > 11, snap > 2, or the lattice point is outside [-2^19, 2^19) in a coordinate. */
int vh_mesh_weld_key(const int32_t cell[3], uint32_t edge, uint32_t snap, uint64_t* key);
/* the number of slots vh_mesh_weld takes for numTriangles when told 0: the smallest power of two >= 6 numTriangles
 * (twice the 3 n distinct keys n triangles can have), 2^6 at least */
int vh_mesh_weld_default_slots_log2(uint32_t numTriangles, uint32_t* slotsLog2);
/* Buffers for welds of up to maxTriangles triangles in tables of up to 1 << slotsLog2 slots (0: the default for
 * maxTriangles).  Device memory: 16 B per slot and 40 B per possible vertex (3 maxTriangles of them). */
int vh_mesh_weld_data_alloc(VhMeshWeldData* data, uint32_t maxTriangles, uint32_t slotsLog2);
void vh_mesh_weld_data_free(VhMeshWeldData* data);
/* Welds a device soup: any triangles with their source records, not only pass 2's.  Asynchronous on `stream`.
 *   d_triangles, d_sources  numTriangles of each (may be NULL when numTriangles is 0: the mesh is then empty)
 *   data                    from vh_mesh_weld_data_alloc; numTriangles <= its m_maxTriangles
 *   slotsLog2               table size of this weld, <= data's; 0 = vh_mesh_weld_default_slots_log2(numTriangles)
 * Result in data: d_counts = {vertices, faces, status}, d_vertices / d_keys (one per welded vertex), d_faces (index
 * triples, winding kept, faces with a repeated index dropped).  A status other than 0 (VH_WELD_TABLE_FULL,
 * VH_WELD_KEY_RANGE) leaves both counts 0. */
int vh_mesh_weld(const VhTriangle* d_triangles, const VhTriangleSource* d_sources, uint32_t numTriangles, const VhMeshWeldData* data,
                 uint32_t slotsLog2, vhStream_t stream);
/* Waits for the weld and reads {vertices, faces, status}.  out is filled whenever the copy succeeded; the return value
 * then restates the status: VH_ERR_BAD_ARGUMENT for VH_WELD_KEY_RANGE, VH_ERR_STAGING_OVERFLOW for VH_WELD_TABLE_FULL. */
int vh_mesh_weld_get_counts(const VhMeshWeldData* data, uint32_t out[3], vhStream_t stream);
/* Copies the mesh to the host; each of vertices, keys and faces may be NULL.  numVertices / numFaces: from the counts. */
int vh_mesh_weld_download(const VhMeshWeldData* data, VhVertex* vertices, uint64_t* keys, uint32_t* faces, uint32_t numVertices,
                          uint32_t numFaces, vhStream_t stream);

/* ---- vertex normals of an indexed mesh (csrc/vh_mesh.hip; DESIGN.md section 4, "Vertex normals"): area-weighted, summed
 * per vertex in 64-bit fixed point, so that the result does not depend on the order of the faces, of the indices within
 * a face, or of the atomics.  Per face (one with a repeated index is skipped), rotated so that the vertex with the
 * smallest key comes first: a = p1 - p0, b = p2 - p0, c = a x b in float32 with one rounding per operation,
 * q = rint(c * 2^scaleLog2) added to the accumulators of the face's three vertices.  Per vertex: the sums as doubles,
 * normalised in double with correctly rounded sqrt and division, rounded to float; a zero sum gives (0, 0, 0).
 *   d_vertices, d_keys   numVertices of each        d_faces   numFaces index triples
 *   scaleLog2            in [-100, 100]; vh_mesh_normals_default_scale_log2 gives the one for a marching-cubes mesh
 *   d_acc                3 int64 per vertex (scratch; zeroed here)      d_normals   3 float per vertex
 *   d_status             one word: 0, or VH_NORMALS_RANGE | VH_NORMALS_BAD_INDEX, and then every normal is (0, 0, 0)
 * Asynchronous on `stream`: two memsets, k_mesh_normals_faces (not launched when numFaces is 0), k_mesh_normals_finish
 * (vh_time_launch_after skip 0, 1); numVertices = 0 launches nothing.  Callers map a status to VH_ERR_BAD_ARGUMENT. */
int vh_mesh_vertex_normals(const VhVertex* d_vertices, const uint64_t* d_keys, const uint32_t* d_faces, uint32_t numVertices, uint32_t numFaces,
                           int32_t scaleLog2, int64_t* d_acc, float* d_normals, uint32_t* d_status, vhStream_t stream);
/* 38 - ceil(log2(v)), v the double product of voxelSize with itself: a marching-cubes triangle lies in one cell, so
 * |a x b| <= 3 voxelSize^2 and the scaled components stay below 2^40.  VH_ERR_BAD_ARGUMENT for a voxel size that is
 * not finite or not positive. */
int vh_mesh_normals_default_scale_log2(float voxelSize, int32_t* scaleLog2);
/* ---- connected components of an indexed mesh (csrc/vh_mesh.hip; DESIGN.md section 4, "Mesh components").  Vertex a
 * comes before b when (key[a], a) < (key[b], b).  Two vertices are joined when a face names both; a component's root
 * is its first vertex.  A lock-free union-find: init, hook (one lane per face), flatten, count.
 *   d_keys        numVertices keys                  d_faces   numFaces index triples
 *   d_root        one per vertex: the index of its component's root (a vertex without a face is its own)
 *   d_faceCount   one per vertex: at a root the number of in-range faces whose first index lies in its component, else 0
 *   d_status      one word: 0, or VH_COMPONENTS_BAD_INDEX (a face with an index >= numVertices: it joins nothing and
 *                 counts nowhere) | VH_COMPONENTS_STEPS
 * A face with a repeated index joins its distinct vertices and counts as one face.  Asynchronous on `stream`;
 * numVertices = 0 launches nothing, numFaces = 0 the init alone.  Callers map a status to VH_ERR_BAD_ARGUMENT. */
int vh_mesh_components(const uint64_t* d_keys, const uint32_t* d_faces, uint32_t numVertices, uint32_t numFaces, uint32_t* d_root, uint32_t* d_faceCount,
                       uint32_t* d_status, vhStream_t stream);
/* Keeps the components of at least minFaces faces and, with largestOnly, of those only the largest (the greatest face
 * count; among equals the root that comes first), compacted into the caller's output arrays: nothing is compacted in
 * place.  Vertex and face order of the output come from atomics; winding and rotation of a face are left alone.
 *   d_vertices, d_keys, d_faces, numVertices, numFaces   the mesh that vh_mesh_components labelled
 *   d_normals / d_outNormals   3 floats per vertex, or NULL: normals ride along
 *   d_root, d_faceCount, d_status   what vh_mesh_components left; with a status set nothing is kept and all counts read 0
 *   d_newIndex   scratch, one word per vertex         d_best   scratch, two 64-bit words
 *   d_outVertices, d_outKeys   room for numVertices   d_outFaces   room for numFaces triples
 *   d_counts     VH_COMPONENTS_NUM_COUNTS words (vh_types.h)
 * minFaces = 0 and largestOnly = 0 keep everything.  With minFaces >= 1 the vertices without a face go. */
int vh_mesh_components_filter(const VhVertex* d_vertices, const uint64_t* d_keys, const float* d_normals, const uint32_t* d_faces, uint32_t numVertices,
                              uint32_t numFaces, const uint32_t* d_root, const uint32_t* d_faceCount, const uint32_t* d_status, uint32_t minFaces,
                              uint32_t largestOnly, uint32_t* d_newIndex, uint64_t* d_best, VhVertex* d_outVertices, uint64_t* d_outKeys,
                              float* d_outNormals, uint32_t* d_outFaces, uint32_t* d_counts, vhStream_t stream);
/* ---- decimation of an indexed mesh by vertex clustering (csrc/vh_mesh_cluster.hip; DESIGN.md section 4, "Mesh
 * clustering").  The lattice of voxel corners is cut into cubes of cellsPerCluster = m points a side (1 <= m <= 64).
 * A vertex belongs to the cube of its key's lattice point L, whatever the key's code: k = floor(L / m) per component
 * (floor, not truncation), and the cube's key is k packed as a lattice point with code 3.  All vertices of a cube
 * become one vertex, at the integer mean floor((2 sum + n) / (2 n)) of q = rint(p * 2^scaleLog2) (colours: 2^16),
 * turned back into a float with one rounding; its key is the cube's.  A face with two corners in one cube is dropped
 * (collapsed); of the faces over the same three cubes one is kept (the others: duplicates) -- if both windings occur,
 * the one which, rotated so that the smallest cube key comes first, has the smaller key second.  A cube that no kept
 * face names gives no vertex (unused).  No float is added anywhere: the result does not depend on the order of the
 * input or of the atomics; vertex and face order of the output do.
 * vh_mesh_cluster_key: the cube's key of a vertex key.  VH_ERR_BAD_ARGUMENT for m outside 1 ... 64 and for a key with
 * bit 62 or 63 set. */
int vh_mesh_cluster_key(uint64_t vertexKey, uint32_t cellsPerCluster, uint64_t* key);
/* 16 - floor(log2(voxelSize)): lattice positions within the key range, scaled, then stay under 2^36 and a quantum is
 * below 2^-16 voxel.  4 cm -> 21, 1 cm -> 23.  VH_ERR_BAD_ARGUMENT for a voxel size that is not finite or not positive. */
int vh_mesh_cluster_default_scale_log2(float voxelSize, int32_t* scaleLog2);
/* log2 of the table size the pass wants for `count` vertices (cluster table) or faces (face table): the smallest power
 * of two >= 2 count, 64 slots at least.  VH_ERR_BAD_ARGUMENT above 2^30. */
int vh_mesh_cluster_default_slots_log2(uint32_t count, uint32_t* slotsLog2);
/* The pass, over the caller's mesh and the caller's buffers (VhMeshClusterData, vh_types.h): insert (one lane per
 * vertex), faces (one lane per face; not without faces), number (one lane per cluster slot), emit (one lane per face
 * slot; not without faces).  data->m_clusterSlotsLog2 / m_faceSlotsLog2 say how much of the tables is used (a smaller
 * value than the default fills a table: VH_CLUSTER_TABLE_FULL).  data->d_counts: the VH_CLUSTER_NUM_COUNTS counts;
 * with a status set (VH_CLUSTER_*) the other five are 0 and nothing was written.  Callers map VH_CLUSTER_TABLE_FULL to
 * VH_ERR_STAGING_OVERFLOW and every other bit to VH_ERR_BAD_ARGUMENT.  Asynchronous on `stream`; numVertices = 0
 * launches nothing.  The mesh that went in stays as it is. */
int vh_mesh_cluster(const VhVertex* d_vertices, const uint64_t* d_keys, const uint32_t* d_faces, uint32_t numVertices, uint32_t numFaces,
                    uint32_t cellsPerCluster, int32_t scaleLog2, const VhMeshClusterData* data, vhStream_t stream);
/* ---- Taubin smoothing of an indexed mesh in fixed point (csrc/vh_mesh_smooth.hip; DESIGN.md section 4, "Mesh
 * smoothing").  Vertex count, keys, colours and faces stay; the positions are replaced by `iterations` = N (1 ... 100)
 * iterations of the lambda | mu scheme under the uniform umbrella operator, in 64-bit integers: the result does not
 * depend on the order of the input or of the atomics.
 * Edges: a face with an index >= numVertices sets VH_SMOOTH_BAD_INDEX and contributes nothing, a face with a repeated
 * index contributes no edge, every other face names three undirected edges; the distinct edges are the neighbour
 * relation, the faces that name an edge its use count, a vertex's distinct neighbours its degree n (above
 * VH_SMOOTH_MAX_DEGREE: VH_SMOOTH_DEGREE).  An edge of use count 1 is a boundary edge, its ends boundary vertices.
 * A vertex moves if n > 0 and, with keepBoundary = 1, it is no boundary vertex; every other vertex keeps its input
 * bits (and still lends its position to its neighbours).
 * q = rint(p * 2^scaleLog2) per component of every vertex (not finite or above 2^40: VH_SMOOTH_RANGE).  Half step
 * k = 0 ... 2 N - 1 with f = lambdaQ16 (k even) or muQ16 (k odd), for a moved vertex, from the q of the half step
 * before: d = sum over the neighbours of q_j - n q_i, u = floor((2 d + n) / (2 n)), q_i' = q_i + ((f u + 2^15) >> 16)
 * (arithmetic shift); |q'| > 2^40: VH_SMOOTH_RANGE.  A moved vertex comes back as (float)((double) q * 2^-scaleLog2).
 * vh_mesh_smooth_default_slots_log2: log2 of the edge table the pass wants for numFaces faces: the smallest power of
 * two >= 6 numFaces, 64 slots at least.  VH_ERR_BAD_ARGUMENT above 0x15555555 faces. */
int vh_mesh_smooth_default_slots_log2(uint32_t numFaces, uint32_t* slotsLog2);
/* The pass, over the caller's mesh and the caller's buffers (VhMeshSmoothData, vh_types.h): edges (one lane per face),
 * degree (one lane per edge slot), prepare (one lane per vertex), gather (one lane per edge slot) and step (one lane
 * per vertex) per half step, finish (one lane per vertex); prepare and finish alone without faces.  lambdaQ16, muQ16:
 * factors in units of 2^-16, |f| <= 65536.  data->m_edgeSlotsLog2 says how much of the table is used (a smaller value
 * than the default fills it: VH_SMOOTH_TABLE_FULL).  data->d_counts: the VH_SMOOTH_NUM_COUNTS counts; with a status set
 * (VH_SMOOTH_*) the other five are 0 and no vertex was written.  Callers map VH_SMOOTH_TABLE_FULL to
 * VH_ERR_STAGING_OVERFLOW and every other bit to VH_ERR_BAD_ARGUMENT.  Asynchronous on `stream`; numVertices = 0
 * launches nothing.  The mesh that went in stays as it is.  VH_ERR_BAD_ARGUMENT for iterations outside 1 ... 100, a
 * factor above 1 in magnitude, keepBoundary above 1 and scaleLog2 outside -100 ... 100. */
int vh_mesh_smooth(const VhVertex* d_vertices, const uint64_t* d_keys, const uint32_t* d_faces, uint32_t numVertices, uint32_t numFaces,
                   uint32_t iterations, int32_t lambdaQ16, int32_t muQ16, uint32_t keepBoundary, int32_t scaleLog2, const VhMeshSmoothData* data,
                   vhStream_t stream);
/* Host only: vh::MeshData::applyTransform (when transform is not NULL) and saveToPLY on the caller's arrays.
 *   vertices3, colors4 (may be NULL), normals3 (may be NULL)   numVertices rows each
 *   faceIndices   numFaceIndices = 3 per face; 0 = a triangle soup
 * With normals the file has nx, ny, nz between z and red, and 28-byte vertex records. */
int vh_mesh_save_ply(const float* vertices3, const float* colors4, const float* normals3, uint64_t numVertices, const uint32_t* faceIndices,
                     uint64_t numFaceIndices, const float transform[16], const char* filename);

/* ---- the accumulating weld: one indexed mesh out of several soups (csrc/vh_mesh.hip; DESIGN.md section 4, "Indexed
 * mesh over several extractions").  begin, then any number of appends, then get_counts / download.
 *   - a cell (VhTriangleSource::cell) belongs to the first append it occurs in: its triangles in a later append are
 *     dropped before they contribute a key, a bid or a face (and counted); within one append all are kept
 *   - a vertex key has one welded vertex for the whole accumulation, with the bits of the soup vertex of the smallest
 *     rank among all kept triangles (ties inside an append: the smallest soup index); its index never changes
 *   - faces are written as final index triples by the append that brings them; a face with a repeated index is dropped
 * The result is vh_mesh_weld of the kept triangles concatenated in append order.
 *   slotsLog2         the table's first size (0: 2^6 slots).  Before an append of n triangles the table is doubled until
 *                     it holds the keys it has plus 4 n (3 n vertex keys, n cell keys) at a load of at most 1/2
 *   reserveTriangles  the first size of the vertex and face arrays (0: the smallest); they grow as needed whatever
 *                     `fixed` says
 *   fixed             the table never grows: a probe that finds no slot sets VH_WELD_TABLE_FULL
 * Device memory: 20 B per slot, 33 B per welded vertex, 12 B per face, 12 B per triangle of the largest append. */
typedef struct VhMeshWeldAccum VhMeshWeldAccum;
int vh_mesh_weld_accum_create(uint32_t slotsLog2, uint32_t reserveTriangles, int fixed, VhMeshWeldAccum** out);
void vh_mesh_weld_accum_destroy(VhMeshWeldAccum* accum);
/* empties the table and the mesh (the buffers are kept at the size they have) */
int vh_mesh_weld_accum_begin(VhMeshWeldAccum* accum, vhStream_t stream);
/* One soup with its records, as the sourced pass 2 writes them.  Waits for the appends before it (it reads their
 * counts to size the table), then launches insert, settle, faces (vh_time_launch_after skip 0, 1, 2) and returns;
 * numTriangles = 0 launches nothing.  Once the status word is set nothing more is launched.  More than
 * VH_WELD_ACCUM_MAX_APPENDS appends: VH_ERR_BAD_ARGUMENT. */
int vh_mesh_weld_accum_append(VhMeshWeldAccum* accum, const VhTriangle* d_triangles, const VhTriangleSource* d_sources, uint32_t numTriangles,
                              vhStream_t stream);
/* Waits and reads the VH_WELD_ACCUM_NUM_COUNTS counts (vh_types.h).  The return value restates the status as
 * vh_mesh_weld_get_counts does; with a status set, vertices, faces, cells and dropped read 0. */
int vh_mesh_weld_accum_get_counts(VhMeshWeldAccum* accum, uint32_t out[6], vhStream_t stream);
/* as vh_mesh_weld_download */
int vh_mesh_weld_accum_download(VhMeshWeldAccum* accum, VhVertex* vertices, uint64_t* keys, uint32_t* faces, uint32_t numVertices,
                                uint32_t numFaces, vhStream_t stream);

/* Vertex normals of the accumulated mesh (vh_mesh_vertex_normals over ALL its faces with the vertex bits the appends
 * left: a pass at the end, never per append).  Waits for the appends, then launches and returns; the buffers are the
 * accumulator's own (36 B per welded vertex more).  A weld that failed returns its error here. */
int vh_mesh_weld_accum_normals(VhMeshWeldAccum* accum, int32_t scaleLog2, vhStream_t stream);
/* Waits and copies 3 floats per vertex.  VH_ERR_BAD_ARGUMENT when no pass has run since the last begin or append (its
 * result would be stale), when numVertices exceeds what the pass saw, or when the pass left a status (the normals are
 * then all zero). */
int vh_mesh_weld_accum_download_normals(VhMeshWeldAccum* accum, float* normals, uint32_t numVertices, vhStream_t stream);

/* The component filter over the accumulated mesh (vh_mesh_components, then vh_mesh_components_filter): a pass at the
 * end, never per append, because a component spans appends.  Waits for the appends, then launches and returns; the
 * buffers are the accumulator's own (44 B per welded vertex and 12 B per face more), and its own mesh, counts and
 * downloads stay what they are.  Normals ride along when vh_mesh_weld_accum_normals has run since the last append. */
int vh_mesh_weld_accum_components(VhMeshWeldAccum* accum, uint32_t minFaces, uint32_t largestOnly, vhStream_t stream);
/* Waits and reads the VH_COMPONENTS_NUM_COUNTS counts.  VH_ERR_BAD_ARGUMENT when no pass has run since the last begin
 * or append (its result would be stale), or when the labelling left a status (the counts are then 0). */
int vh_mesh_weld_accum_components_get_counts(VhMeshWeldAccum* accum, uint32_t out[6], vhStream_t stream);
/* The filtered mesh; each array may be NULL.  numVertices / numFaces: the kept ones of the counts.  Refused as above,
 * and when normals are asked for that the pass did not carry. */
int vh_mesh_weld_accum_components_download(VhMeshWeldAccum* accum, VhVertex* vertices, uint64_t* keys, float* normals, uint32_t* faces,
                                           uint32_t numVertices, uint32_t numFaces, vhStream_t stream);

/* The vertex clustering over the accumulated mesh (vh_mesh_cluster): a pass at the end, never per append, because a
 * cluster spans appends.  Waits for the appends, launches, and waits for the counts; the buffers are the
 * accumulator's own, and its welded mesh, counts and downloads stay what they are.  After a pass without a status,
 * vh_mesh_weld_accum_normals and vh_mesh_weld_accum_components work on the CLUSTERED mesh until the next begin or
 * append; a pass makes earlier normals and components stale.  cellsPerCluster = 0 launches nothing and forgets the last
 * pass: normals and components are of the welded mesh again, and the pass's reads are refused. */
int vh_mesh_weld_accum_cluster(VhMeshWeldAccum* accum, uint32_t cellsPerCluster, int32_t scaleLog2, vhStream_t stream);
/* Waits and reads the VH_CLUSTER_NUM_COUNTS counts.  VH_ERR_BAD_ARGUMENT when no pass has run since the last begin or
 * append (its result would be stale) or the pass left a status, VH_ERR_STAGING_OVERFLOW when that status is a full
 * table alone; the other five counts are then 0. */
int vh_mesh_weld_accum_cluster_get_counts(VhMeshWeldAccum* accum, uint32_t out[6], vhStream_t stream);
/* The clustered mesh; each array may be NULL.  numVertices / numFaces: at most those of the counts.  Refused as above. */
int vh_mesh_weld_accum_cluster_download(VhMeshWeldAccum* accum, VhVertex* vertices, uint64_t* keys, uint32_t* faces, uint32_t numVertices,
                                        uint32_t numFaces, vhStream_t stream);

/* The Taubin smoothing over the accumulated mesh (vh_mesh_smooth): a pass of the finish, never of an append, over the
 * clustered mesh if a cluster pass is current, else over the welded one, into buffers of the accumulator's own.  Waits
 * for the appends, launches, and waits for the counts.  After a pass without a status, vh_mesh_weld_accum_normals and
 * vh_mesh_weld_accum_components work on the SMOOTHED vertices; a pass makes earlier normals and components stale.  A
 * begin, an append or a later cluster pass makes it stale.  iterations = 0 launches nothing and forgets the last pass. */
int vh_mesh_weld_accum_smooth(VhMeshWeldAccum* accum, uint32_t iterations, int32_t lambdaQ16, int32_t muQ16, uint32_t keepBoundary, int32_t scaleLog2,
                              vhStream_t stream);
/* Waits and reads the VH_SMOOTH_NUM_COUNTS counts.  VH_ERR_BAD_ARGUMENT when no pass is current or the pass left a
 * status, VH_ERR_STAGING_OVERFLOW when that status is a full table alone; the other five counts are then 0. */
int vh_mesh_weld_accum_smooth_get_counts(VhMeshWeldAccum* accum, uint32_t out[6], vhStream_t stream);
/* The smoothed vertices (keys and faces are the source mesh's: the clustered one's, or the welded one's).  numVertices:
 * at most those of the source mesh.  Refused as above. */
int vh_mesh_weld_accum_smooth_download(VhMeshWeldAccum* accum, VhVertex* vertices, uint32_t numVertices, vhStream_t stream);

/* handle level: CUDAMarchingCubesHashSDF (DSC/CUDAMarchingCubesHashSDF.h:8-67) */
typedef struct VhMarchingCubes VhMarchingCubes;
int vh_marching_cubes_create(const VhMarchingCubesParams* params, vhStream_t stream, VhMarchingCubes** out);
void vh_marching_cubes_destroy(VhMarchingCubes* mc);
/* parametersFromGlobalAppState :19-28 */
int vh_marching_cubes_parameters(uint32_t maxNumTriangles, float threshFactor, float voxelSize, uint32_t hashNumBuckets,
                                 VhMarchingCubesParams* out);
int vh_marching_cubes_set_offline_processing(VhMarchingCubes* mc, int enabled);
/* extractIsoSurface(hashData, hashParams, rayCastData, minCorner, maxCorner, boxEnabled) .cpp:194-209 (copy = 1)
 * / extractIsoSurfaceWithoutCopy :211-224 (copy = 0) */
int vh_marching_cubes_extract_iso_surface(VhMarchingCubes* mc, const VhHashData* hd, const VhHashParams* hp,
                                          const float minCorner[3], const float maxCorner[3], int boxEnabled, int copy);
/* extractIsoSurface(chunkGrid, rayCastData, camPos, radius) .cpp:149-192 */
int vh_marching_cubes_extract_iso_surface_chunk_grid(VhMarchingCubes* mc, VhChunkGrid* grid, const float camPos[3], float radius);
/* extractIsoSurfaceIndexed (not in the reference): reset, pass 1, sourced pass 2, weld, download.  REPLACES the host
 * mesh with the indexed one and marks it welded, so that saveMesh writes it as it is.
 *   minCorner, maxCorner, boxEnabled   as vh_marching_cubes_extract_iso_surface (the corners may be NULL)
 * VH_ERR_STAGING_OVERFLOW when the triangle buffer overflowed (as copyTrianglesToCPU) or the weld table was full,
 * VH_ERR_BAD_ARGUMENT when a lattice coordinate left the key range; the host mesh is then empty. */
int vh_marching_cubes_extract_iso_surface_indexed(VhMarchingCubes* mc, const VhHashData* hd, const VhHashParams* hp,
                                                  const float minCorner[3], const float maxCorner[3], int boxEnabled);
/* The indexed extraction box by box (not in the reference): begin_indexed starts an accumulation, append_indexed runs
 * reset, pass 1, the sourced pass 2 and the overflow test of copyTrianglesToCPU in one box and appends the soup to the
 * accumulating weld, finish_indexed downloads and REPLACES the host mesh as vh_marching_cubes_extract_iso_surface_indexed
 * does.  Boxes may overlap: a cell is taken from the first box that has it.  An error leaves the host mesh empty. */
int vh_marching_cubes_begin_indexed(VhMarchingCubes* mc);
int vh_marching_cubes_append_indexed(VhMarchingCubes* mc, const VhHashData* hd, const VhHashParams* hp, const float minCorner[3],
                                     const float maxCorner[3], int boxEnabled);
int vh_marching_cubes_finish_indexed(VhMarchingCubes* mc);
/* The live mesh on the object (not in the reference; liveBegin ... liveEnd of include/vh.hpp).  Between live_begin and
 * live_end the object's triangle buffer and its source records are the cache of vh_live_mesh_update: get_counts,
 * download_triangles and download_sources read it, and every extraction is refused with VH_ERR_BAD_ARGUMENT, with nothing
 * done.  live_update brings the cache up to date with the table and fills counts_out (may be NULL) with the
 * VH_LIVE_NUM_COUNTS counts and the status; VH_ERR_STAGING_OVERFLOW / VH_ERR_BAD_ARGUMENT as vh_live_mesh_get_counts,
 * the cache then invalid until the next update; VH_ERR_BAD_ARGUMENT without live_begin, with boxEnabled, or for hash
 * parameters other than the earlier updates', the cache then as it was.  live_invalidate makes the next update a full
 * one.  live_indexed welds the cache and runs the passes that are on, as extract_iso_surface_indexed does after its
 * pass 2, and REPLACES the host mesh; VH_ERR_BAD_ARGUMENT when the cache is not valid. */
int vh_marching_cubes_live_begin(VhMarchingCubes* mc);
int vh_marching_cubes_live_update(VhMarchingCubes* mc, const VhHashData* hd, const VhHashParams* hp, int boxEnabled, uint32_t counts_out[9]);
int vh_marching_cubes_live_invalidate(VhMarchingCubes* mc);
int vh_marching_cubes_live_indexed(VhMarchingCubes* mc);
int vh_marching_cubes_live_end(VhMarchingCubes* mc);
/* The walk of vh_marching_cubes_extract_iso_surface_chunk_grid with the same boxes, every chunk appended to one
 * accumulation: the indexed mesh of a streamed scene.  When a chunk fails (VH_ERR_STAGING_OVERFLOW, VH_ERR_BAD_ARGUMENT
 * as above) the scene is streamed back in around camPos and the streaming thread restarted as at the normal end, the
 * host mesh is empty and the indexed counts are 0. */
int vh_marching_cubes_extract_iso_surface_indexed_chunk_grid(VhMarchingCubes* mc, VhChunkGrid* grid, const float camPos[3], float radius);
/* of the last accumulated extraction: the VH_WELD_ACCUM_NUM_COUNTS counts of vh_types.h (all 0 after a one-shot one) */
int vh_marching_cubes_get_indexed_stats(VhMarchingCubes* mc, uint32_t out[6]);
/* of the last indexed extraction: {vertices, faces, status} */
int vh_marching_cubes_get_indexed_counts(VhMarchingCubes* mc, uint32_t out[3]);
/* the device mesh of the last indexed extraction; each of vertices (position + colour), keys and faces may be NULL.
 * The arrays hold what vh_marching_cubes_get_indexed_counts reports. */
int vh_marching_cubes_download_indexed(VhMarchingCubes* mc, VhVertex* vertices, uint64_t* keys, uint32_t* faces);
/* Vertex normals for the indexed extractions (off by default): when on, the three indexed extractions run
 * vh_mesh_vertex_normals after the weld with the default scale of hp's voxel size, the host mesh holds them, and
 * save_mesh writes them.  A status of the pass: VH_ERR_BAD_ARGUMENT, the host mesh empty. */
int vh_marching_cubes_set_indexed_normals(VhMarchingCubes* mc, int enabled);
/* 3 floats per vertex of the last indexed extraction, in the order of vh_marching_cubes_download_indexed;
 * VH_ERR_BAD_ARGUMENT when that extraction ran without normals */
int vh_marching_cubes_download_indexed_normals(VhMarchingCubes* mc, float* normals);
/* the host mesh's normals: out = number of floats (3 per vertex, or 0), then the array */
int vh_marching_cubes_get_mesh_normals_size(VhMarchingCubes* mc, uint64_t* out);
int vh_marching_cubes_get_mesh_normals(VhMarchingCubes* mc, float* normals3);
/* The component filter for the indexed extractions (off by default: minFaces = 0 and largestOnly = 0).  When on, the
 * three indexed extractions run vh_mesh_components and vh_mesh_components_filter after the weld and the normals -- the
 * accumulated ones at the finish -- and get_indexed_counts, download_indexed, download_indexed_normals, the host mesh
 * and save_mesh all describe the FILTERED mesh.  A status of the labelling: VH_ERR_BAD_ARGUMENT, the host mesh empty. */
int vh_marching_cubes_set_indexed_component_filter(VhMarchingCubes* mc, uint32_t minFaces, uint32_t largestOnly);
/* of the last indexed extraction with the filter on: the VH_COMPONENTS_NUM_COUNTS counts, which say what the
 * unfiltered mesh held; all 0 when it ran with the filter off */
int vh_marching_cubes_get_indexed_component_stats(VhMarchingCubes* mc, uint32_t out[6]);
/* The vertex clustering for the indexed extractions (off by default: cellsPerCluster = 0; 1 ... 64 turn it on).  When
 * on, the three indexed extractions run vh_mesh_cluster after the weld and BEFORE normals and components -- the
 * accumulated ones at the finish -- at vh_mesh_cluster_default_scale_log2(voxelSize); normals (at the scale of
 * 2 cellsPerCluster voxelSize) and components are then of the clustered mesh, and get_indexed_counts, download_indexed,
 * download_indexed_normals, the host mesh and save_mesh all describe it.  A status of the pass: VH_ERR_BAD_ARGUMENT or
 * VH_ERR_STAGING_OVERFLOW, the host mesh empty.  VH_ERR_BAD_ARGUMENT for cellsPerCluster > 64. */
int vh_marching_cubes_set_indexed_clustering(VhMarchingCubes* mc, uint32_t cellsPerCluster);
/* of the last indexed extraction with clustering on: the VH_CLUSTER_NUM_COUNTS counts; all 0 when it ran with it off */
int vh_marching_cubes_get_indexed_cluster_stats(VhMarchingCubes* mc, uint32_t out[6]);
/* The Taubin smoothing for the indexed extractions (off by default: iterations = 0; 1 ... 100 turn it on).  When on, the
 * three indexed extractions run vh_mesh_smooth after the clustering and BEFORE normals and components -- the
 * accumulated ones at the finish -- at vh_mesh_cluster_default_scale_log2(voxelSize); normals (at the scale of twice
 * the edge bound used without smoothing: a margin, not a proof) and components are then of the smoothed mesh, and
 * download_indexed, the host mesh and save_mesh carry the smoothed positions.  A status of the pass:
 * VH_ERR_BAD_ARGUMENT or VH_ERR_STAGING_OVERFLOW, the host mesh empty.  VH_ERR_BAD_ARGUMENT for iterations > 100, a
 * factor above 1 in magnitude and keepBoundary above 1. */
int vh_marching_cubes_set_indexed_smoothing(VhMarchingCubes* mc, uint32_t iterations, int32_t lambdaQ16, int32_t muQ16, uint32_t keepBoundary);
/* of the last indexed extraction with smoothing on: the VH_SMOOTH_NUM_COUNTS counts; all 0 when it ran with it off */
int vh_marching_cubes_get_indexed_smooth_stats(VhMarchingCubes* mc, uint32_t out[6]);
/* the first n source records of the last indexed extraction (n <= min(triangles produced, m_maxNumTriangles)) */
int vh_marching_cubes_download_sources(VhMarchingCubes* mc, VhTriangleSource* out, uint32_t n);
int vh_marching_cubes_copy_triangles_to_cpu(VhMarchingCubes* mc);
int vh_marching_cubes_clear_mesh_buffer(VhMarchingCubes* mc);
/* counts of the last extraction: {triangles produced, occupied blocks} */
int vh_marching_cubes_get_counts(VhMarchingCubes* mc, uint32_t out[2]);
int vh_marching_cubes_download_triangles(VhMarchingCubes* mc, VhTriangle* out, uint32_t n);
/* the host mesh (getMetaDataf): sizes {vertices, face indices (3 per face; 0 = triangle soup)}, then the arrays */
int vh_marching_cubes_get_mesh_size(VhMarchingCubes* mc, uint64_t out[2]);
int vh_marching_cubes_get_mesh(VhMarchingCubes* mc, float* vertices3, float* colors4, uint32_t* faceIndices);
/* saveMesh(filename, transform, overwriteExistingFile) .cpp:89-145; transform may be NULL */
int vh_marching_cubes_save_mesh(VhMarchingCubes* mc, const char* filename, const float transform[16], int overwriteExistingFile);

/* ---- shaded view of the model: DX11RGBDRenderer::RenderDepthMap + DX11PhongLighting::render as compute passes
 * (csrc/vh_view.hip; DESIGN.md section 4, "Rendering").
 * launcher level.  A depth map (width x height, one quad per pixel, two triangles per quad, primitive id 2 quad + t) is
 * rasterised into a screen of 64-bit keys (float_bits(z) << 32 | primitive id, atomicMin = LESS with the first-drawn
 * primitive winning ties); vh_view_resolve turns the keys into the four maps of RGBDRendererRawDepthPS.
 *   d_keys       screenWidth * screenHeight uint64, all ones before the first raster (vh_memset 0xff); every resolve
 *                leaves them so
 *   d_largeList  vh_view_large_list_words(width, height) uint32, zero before the first raster; every resolve leaves it so
 *   outputs      screen-size maps: depth (f32, clear -inf), position / normal / colour (float4, clear (-inf, -inf, -inf, 1))
 * The colour map (float4, may be NULL for the raster) is the model's colours; both launchers must see the same depth map
 * and params.  Screens narrower or lower than 2 pixels are rejected (the shader divides by screen size - 1). */
uint32_t vh_view_large_list_words(uint32_t width, uint32_t height);
int vh_view_raster(const float* d_depth, const VhViewParams* params, uint64_t* d_keys, uint32_t* d_largeList, vhStream_t stream);
int vh_view_resolve(const float* d_depth, const float* d_color4, const VhViewParams* params, uint64_t* d_keys, uint32_t* d_largeList,
                    float* d_outDepth, float* d_outPosition4, float* d_outNormal4, float* d_outColor4, vhStream_t stream);
/* render target 0 alone: the depth map of vh_view_resolve (the source depth interpolated, -inf where nothing is drawn)
 * written into d_outDepth, with the same key / list reset.  CUDARGBDSensor's remap into the colour camera.  d_outDepth
 * is screen size and must not be the source depth map. */
int vh_view_resolve_depth(const float* d_depth, const VhViewParams* params, uint64_t* d_keys, uint32_t* d_largeList, float* d_outDepth, vhStream_t stream);
/* PhongPS (Shaders/PhongLighting.hlsl:49-86) on numPixels float4 maps.  out4 (float4) and/or outRGBA8 (D3D FLOAT->UNORM:
 * NaN -> 0, clamp to [0, 1], x 255, round to nearest even) may be NULL; alphaRule sets the RGBA8 alpha to 255 where any
 * of r, g, b is > 0 (renderToFile, DSC/DepthSensing.cpp:1199-1202). */
int vh_phong(const float* d_positions4, const float* d_normals4, const float* d_colors4, uint32_t numPixels, int useMaterial, const VhPhongLight* light,
             float* d_out4, uint8_t* d_outRGBA8, int alphaRule, vhStream_t stream);

/* the rendering keys of a zParameters*.txt (VhRenderState); vh_phong_light_from_render_state is ConstantBufferLight::SetDefault */
int vh_read_render_state(const char* filename, VhRenderState* out);
int vh_parse_render_state(const char* text, VhRenderState* out);
/* the camera-calibration keys of a zParameters*.txt (VhCalibrationState), read by the same rules */
int vh_read_calibration_state(const char* filename, VhCalibrationState* out);
int vh_parse_calibration_state(const char* text, VhCalibrationState* out);
void vh_phong_light_from_render_state(const VhRenderState* rs, VhPhongLight* out);

/* 8-bit RGBA, non-interlaced, lossless PNG of width x height pixels (row stride width * 4), deflated by the system zlib at
 * `level` (0-9, or -1 for zlib's default). */
int vh_write_png_rgba8(const char* filename, uint32_t width, uint32_t height, const uint8_t* rgba, int level);

/* handle level: DX11RGBDRenderer (DSC/DX11RGBDRenderer.h) and DX11PhongLighting (DSC/DX11PhongLighting.h) without the D3D
 * context.  The renderer owns its four screen maps and the key buffer; the Phong pass owns a float4 and an RGBA8 target. */
typedef struct VhRGBDRenderer VhRGBDRenderer;
int vh_rgbd_renderer_create(vhStream_t stream, VhRGBDRenderer** out);
void vh_rgbd_renderer_destroy(VhRGBDRenderer* r);
/* RenderDepthMap(d_depthMap, d_colorMap, width, height, intrinsicDepthToWorld, modelview, intrinsicWorldToDepth,
 * screenWidth, screenHeight, depthThreshOffset, depthThreshLin) :197-275 */
int vh_rgbd_renderer_render_depth_map(VhRGBDRenderer* r, const float* d_depthMap, const float* d_colorMap4, uint32_t width, uint32_t height,
                                      const float intrinsicDepthToWorld[16], const float modelview[16], const float intrinsicWorldToDepth[16],
                                      uint32_t screenWidth, uint32_t screenHeight, float depthThreshOffset, float depthThreshLin);
/* the maps of the last RenderDepthMap (device pointers) and their size */
int vh_rgbd_renderer_get_maps(VhRGBDRenderer* r, float** depth, float** positions4, float** normals4, float** colors4, uint32_t size[2]);
typedef struct VhPhongLighting VhPhongLighting;
int vh_phong_lighting_create(const VhPhongLight* light, vhStream_t stream, VhPhongLighting** out);
void vh_phong_lighting_destroy(VhPhongLighting* p);
/* render(d_positions, d_normals, d_colors, useMaterial, width, height) :42; the float4 target and, on request, its RGBA8
 * form with renderToFile's alpha rule */
int vh_phong_lighting_render(VhPhongLighting* p, const float* d_positions4, const float* d_normals4, const float* d_colors4, int useMaterial,
                             uint32_t width, uint32_t height, int rgba8);
int vh_phong_lighting_get_colors(VhPhongLighting* p, float** colors4, uint8_t** rgba8);

#ifdef __cplusplus
}
#endif
#endif /* VH_API_H */
