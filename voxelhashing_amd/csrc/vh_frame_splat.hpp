// vh_frame_splat.hpp -- frame loop: what the tile ray caster is handed.  The interval splat (tile heads and block lists:
// interval_splat_group, k_interval_splat, k_interval_clear) and the launch order of the next render (split_tiles,
// schedule_tiles; the schedule buffer's layout and size, schedule_words).  Included by vh_kernels.hip, by vh_ray_tiles.hpp
// (the tile ray caster reads the heads, the lists and the schedule, and leaves the cost classes) and by
// vh_frame_normals.hpp (k_compute_normals carries interval_splat_group as a rider).
#pragma once

#include "vh_device.hpp"

namespace {
using namespace vhd;

// ---------------------------------------------------------------------------
// ray-interval splatting as a compute pass (the reference rasterises block quads with D3D11 into min/max depth
// textures, DSC/DX11RayIntervalSplatting.cpp:150-220 + rayIntervalSplatKernel DSC/CUDARayCastSDF.cu:101-167, and
// this fork then ignores them: DSC/CUDARayCastSDF.cu:36-42).  Here every ALLOCATED block (not only the ones the
// approximate frustum test keeps) is projected, one wave per block, and folded into the 8x8-pixel tiles it can
// matter to:
//   * head {min depth, max depth, count}: camera-depth range of those blocks (positive float bits: uint order =
//     float order) and how many there are;
//   * list: their {block position, voxel pointer}, up to `cap` per tile.
// Both are conservative supersets, so rendering with them cannot change a result: a sample reads voxels within one
// voxel of its position (two for the gradient), the box of a block is grown by more than that, and a perspective
// projection maps a box in front of the camera into the hull of its projected corners.  A tile whose list is
// complete therefore knows every block its rays can read: k_render resolves block -> pointer in LDS instead of
// probing the hash table in HBM (and a block missing from the list is unallocated, as a failed probe would say).
// ---------------------------------------------------------------------------

constexpr uint32_t kSplatWordsPerGroup = 32; // occupancy words (x32 buckets) per workgroup
constexpr uint32_t kSplatQueue = 128;        // blocks a workgroup queues per round

// (i / nx, i % nx) for i < 2^22 without the integer-division sequence: float estimate, corrected by one step
VHD void divmod_small(uint32_t i, uint32_t nx, float rnx, uint32_t& q, uint32_t& r)
{
    q = (uint32_t)((float)i * rnx);
    int rem = (int)i - (int)(q * nx);
    if (rem < 0) { q--; rem += (int)nx; }
    if (rem >= (int)nx) { q++; rem -= (int)nx; }
    r = (uint32_t)rem;
}

// Three steps per workgroup, each one trip to memory: occupancy words -> bucket queue (LDS); slots of the queued
// buckets -> block queue (LDS); one wave per queued block folds it into its tiles.  The queues balance the waves: a
// block costs a wave a few thousand cycles, and the kernel is as long as its busiest wave.
// Cost of a tile in units of one empty-space step; a full sample (8 taps) weighs kCostSample of them (vh_ray_march.hpp,
// where they are counted).  The wave's cost is its busiest lane's: k_render stores the tile's cost class for the next
// frame's launch order.
constexpr uint32_t kCostClasses = 32;
constexpr uint32_t kCostClassWidth = 8;
// The dearest tiles of a frame are marched by TWO waves of one workgroup, each one half of the tile's depth interval:
// a wave alone on its SIMD runs at the pace of its own chain of dependent loads, and the few tiles with the longest
// rays (a silhouette grazing the truncation band) are the tail of the kernel.  A sample's state is the previous
// sample's alone, so the far half starts at the last sample before the middle with nothing remembered and arrives at
// the middle in the state the whole march would have; the near half's hit, if any, is the first along the ray.
#ifndef VH_SPLIT_TILES
#define VH_SPLIT_TILES 256
#endif
constexpr uint32_t kSplitTiles = VH_SPLIT_TILES;     // at most (even: two split tiles fill a workgroup); measured at 640x480: 64 -> 37.8 us, 256 -> 37.0, 512 -> 37.8
constexpr uint32_t kSplitMinTiles = 1024; // smaller images are not split
__host__ __device__ inline uint32_t split_tiles(uint32_t nTiles) // one tile in sixteen, dearest first
{
#ifndef VH_SPLIT_DIV
#define VH_SPLIT_DIV 16
#endif
    const uint32_t n = (nTiles / VH_SPLIT_DIV) & ~1u;
    return nTiles >= kSplitMinTiles ? (n < kSplitTiles ? n : kSplitTiles) : 0u;
}

// Launch order of the next k_render (one workgroup of k_interval_splat, beside the others): tiles sorted by the cost
// class the previous k_render stored, dearest first, dealt to the workgroups (4 tiles each) in rows of numCUs that
// alternate direction.  The hardware places workgroup g on compute unit g mod numCUs (all of them are resident), so
// a compute unit receives one workgroup of every row: the dearest of one row with the cheapest of the next.
// The sort was ONE workgroup's and the longest chain of its launch (per-workgroup time stamps, tools/riders_stamps.py: it
// ended at 8.4 us of a 9.9 us launch at 640x480, at 50 of 50 us at 1920x1080, everything else long done).  Now kSchedGroups
// workgroups sort a share of the tiles each -- the quads of four tiles q = part (mod parts): shares that look alike --
// and deal their sorted shares into the launch order in turns (the tile of rank i in share w comes after rank i of the
// shares before it): the dearest first as before, to within the difference between the shares.
constexpr uint32_t kSchedGroups = 8;
__host__ __device__ inline uint32_t sched_groups(uint32_t nTiles) { return nTiles >= kSplitMinTiles ? kSchedGroups : 1u; }

// The schedule buffer (host): {phase the slots were made for, longest list, -, -}, a cost class per tile padded to whole
// quads, then {tile | half << 24, phase} per launch slot -- a slot for each of the four waves of `renderGroups` workgroups
// of the tile ray caster (render_groups, vh_ray_tiles.hpp).  This is the layout's definition: schedule_tiles below and
// render_tile spell out where the slots begin.
inline size_t schedule_words(uint32_t nTiles, uint32_t renderGroups) { return 4u + 4u * (size_t)cdiv(nTiles, 4) + 2u * 4u * (size_t)renderGroups; }

__device__ void schedule_tiles(uint32_t* sched, uint32_t* feedback, uint32_t nTiles, uint32_t phase, uint32_t numCUs, uint32_t part, uint32_t parts,
                               uint32_t* sCount /*[2 * 256]*/)
{
    // layout: {phase the slots were made for, -, -, -}, cost class per tile, {tile, phase} per launch slot (schedule_words
    // defines it; where the slots begin is spelled out here and in render_tile, vh_ray_tiles.hpp)
    const uint32_t* cls = sched + 4;
    uint2* slots = reinterpret_cast<uint2*>(sched + 4 + 4u * ((nTiles + 3u) / 4u));
    const uint32_t nSplit = split_tiles(nTiles);
    if (threadIdx.x == 0 && part == 0u) {
        sched[0] = phase;
        if (feedback) *feedback = sched[1]; // longest tile list the previous k_render met (0: none near the small capacity)
        sched[1] = 0u;
    }
    // counting sort with kSub sub-bins per class (keyed by the thread): 64 lanes adding to one LDS word serialise
    constexpr uint32_t kSub = 8, kBins = kCostClasses * kSub;
    static_assert(kBins == 4u * kWave, "the scan below gives four bins to each lane of one wave");
    for (uint32_t i = threadIdx.x; i < 2u * kBins; i += blockDim.x) sCount[i] = 0u;
    __syncthreads();
    const uint32_t sub = threadIdx.x % kSub;
    // four tiles per load, kBatch loads in flight: this workgroup is alone with its trips to memory
    constexpr uint32_t kBatch = 5;
    const uint32_t nQuads = (nTiles + 3u) / 4u; // the cost array is padded to whole quads (vh_render_schedule_bytes)
    const uint4* cls4 = reinterpret_cast<const uint4*>(cls);
    const uint32_t myQuads = part < nQuads ? (nQuads - part + parts - 1u) / parts : 0u; // quads part, part + parts, ...
    // tiles in each share (the image's last quad may be short), for the turn-taking below
    uint32_t nShare[kSchedGroups];
#pragma unroll
    for (uint32_t w = 0; w < kSchedGroups; w++) {
        const uint32_t nq = (w < parts && w < nQuads) ? (nQuads - w + parts - 1u) / parts : 0u;
        nShare[w] = 4u * nq - ((nq != 0u && (nQuads - 1u) % parts == w) ? 4u * nQuads - nTiles : 0u);
    }
    for (uint32_t q0 = threadIdx.x; q0 < myQuads; q0 += blockDim.x * kBatch) {
        uint4 c[kBatch];
#pragma unroll
        for (uint32_t j = 0; j < kBatch; j++) {
            const uint32_t q = q0 + j * blockDim.x;
            c[j] = q < myQuads ? cls4[q * parts + part] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (uint32_t j = 0; j < kBatch; j++) {
            const uint32_t t = ((q0 + j * blockDim.x) * parts + part) * 4u;
            if (t + 0u < nTiles) atomicAdd(&sCount[min(c[j].x, kCostClasses - 1u) * kSub + sub], 1u);
            if (t + 1u < nTiles) atomicAdd(&sCount[min(c[j].y, kCostClasses - 1u) * kSub + sub], 1u);
            if (t + 2u < nTiles) atomicAdd(&sCount[min(c[j].z, kCostClasses - 1u) * kSub + sub], 1u);
            if (t + 3u < nTiles) atomicAdd(&sCount[min(c[j].w, kCostClasses - 1u) * kSub + sub], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < kWave) { // start of each bin in the sorted order, dearest class first: one wave scans the 256 bins
        const uint32_t lane = threadIdx.x;
        uint32_t n[4], mine = 0u;
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) { n[j] = sCount[kBins - 1u - (lane * 4u + j)]; mine += n[j]; } // bins in descending order
        uint32_t incl = mine;
#pragma unroll
        for (int off = 1; off < (int)kWave; off <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, off);
            if ((int)lane >= off) incl += up;
        }
        uint32_t start = incl - mine;
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) { sCount[kBins + kBins - 1u - (lane * 4u + j)] = start; start += n[j]; }
    }
    __syncthreads();
    // launch slots: the nSplit dearest tiles take two each (near half, far half; two tiles to a workgroup), the others one
    const uint32_t nGroups = (nTiles + nSplit + 3u) / 4u, fullRows = nGroups / numCUs;
    for (uint32_t q0 = threadIdx.x; q0 < myQuads; q0 += blockDim.x * kBatch) {
        uint4 c[kBatch];
#pragma unroll
        for (uint32_t j = 0; j < kBatch; j++) {
            const uint32_t q = q0 + j * blockDim.x;
            c[j] = q < myQuads ? cls4[q * parts + part] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (uint32_t j = 0; j < kBatch; j++) {
            const uint32_t cc[4] = { c[j].x, c[j].y, c[j].z, c[j].w };
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) {
                const uint32_t t = ((q0 + j * blockDim.x) * parts + part) * 4u + k;
                if (t < nTiles) {
                    const uint32_t mine = atomicAdd(&sCount[kBins + min(cc[k], kCostClasses - 1u) * kSub + sub], 1u); // rank of tile t in this share
                    // its rank overall: the shares take turns, a share that has run out is skipped
                    uint32_t i = 0u;
#pragma unroll
                    for (uint32_t w = 0; w < kSchedGroups; w++) i += min(mine, nShare[w]) + ((w < part && nShare[w] > mine) ? 1u : 0u);
                    if (i < nSplit) {
                        const uint32_t at = (i / 2u) * 4u + (i & 1u) * 2u;
                        slots[at] = make_uint2(t | (1u << 24), phase);
                        slots[at + 1u] = make_uint2(t | (2u << 24), phase);
                    } else {
                        const uint32_t j = i + nSplit;
                        uint32_t g = j / 4u;
                        const uint32_t row = g / numCUs, col = g % numCUs;
                        // (a row that also holds split tiles keeps its order: their slots are fixed)
                        if ((row & 1u) && row < fullRows && row * numCUs >= nSplit / 2u) g = row * numCUs + (numCUs - 1u - col);
                        slots[g * 4u + (j & 3u)] = make_uint2(t, phase);
                    }
                }
            }
        }
    }
}

struct SplatShared {
    uint32_t sBuckets[kSplatWordsPerGroup * 32];
    int4 sBlocks[kSplatQueue];
    uint32_t sNumBuckets, sNumBlocks;
};

// one workgroup of the splat: `group` < nSplatGroups takes 32 occupancy words, group == nSplatGroups makes the schedule
__device__ void interval_splat_group(const VhHashData& hd, const VhHashParams& hp, const VhDepthCameraParams& cp, const VhRayCastParams& rp,
                                     uint4* heads, int4* lists, uint32_t cap, uint32_t* sched, uint32_t phase, uint32_t numCUs,
                                     uint32_t nSplatGroups, uint32_t* feedback, uint32_t group, SplatShared& sh)
{
    uint32_t (&sBuckets)[kSplatWordsPerGroup * 32] = sh.sBuckets;
    int4 (&sBlocks)[kSplatQueue] = sh.sBlocks;
    uint32_t& sNumBuckets = sh.sNumBuckets;
    uint32_t& sNumBlocks = sh.sNumBlocks;
    const uint32_t nWords = (hp.m_hashNumBuckets + 31) / 32;
    const uint32_t lane = lane_id(), wave = threadIdx.x / kWave;
    const int tilesX = (int)((rp.m_width + 7) / 8), tilesY = (int)((rp.m_height + 7) / 8);
    const float vs = hp.m_virtualVoxelSize;
    // voxel indices a sample at p can read along one axis: floor(p/vs) and floor(p/vs)+1 (+-1/2 more for the
    // gradient's offset samples); block b holds indices 8b..8b+7  =>  p/vs in [8b-1, 8b+8) (+-1/2).  A quarter
    // voxel on top covers every rounding on the way (|p/vs| < 2^16 where the quotient is resolved to 2^-8).
    const float growLo = (rp.m_useGradients ? 1.75f : 1.25f) * vs, growHi = (rp.m_useGradients ? 0.75f : 0.25f) * vs;

    if (group >= nSplatGroups) { // the extra workgroups (launched only with a schedule)
        schedule_tiles(sched, feedback, (uint32_t)(tilesX * tilesY), phase, numCUs, group - nSplatGroups, sched_groups((uint32_t)(tilesX * tilesY)), sBuckets);
        return;
    }
    if (threadIdx.x == 0) { sNumBuckets = 0u; sNumBlocks = 0u; }
    __syncthreads();
    // 1: occupied buckets of this group's words
    if (threadIdx.x < kSplatWordsPerGroup) {
        const uint32_t wordIdx = group * kSplatWordsPerGroup + threadIdx.x;
        uint32_t bits = wordIdx < nWords ? hd.d_bucketBits[wordIdx] : 0u;
        while (bits) {
            const uint32_t bucket = wordIdx * 32u + (uint32_t)(__ffs((int)bits) - 1);
            bits &= bits - 1u;
            sBuckets[atomicAdd(&sNumBuckets, 1u)] = bucket;
        }
    }
    __syncthreads();
    const uint32_t nBuckets = sNumBuckets;
    // 2+3 in rounds of 12 buckets (120 slots, within the block queue)
    for (uint32_t b0 = 0; b0 < nBuckets; b0 += 12u) {
        const uint32_t bi = b0 + threadIdx.x / 16u, sl = threadIdx.x % 16u;
        if (threadIdx.x < 12u * 16u && bi < nBuckets && sl < VH_HASH_BUCKET_SIZE) {
            const int4 q = load_quad(&hd.d_hash[(uint64_t)sBuckets[bi] * VH_HASH_BUCKET_SIZE + sl]);
            if (q.w != VH_FREE_ENTRY) sBlocks[atomicAdd(&sNumBlocks, 1u)] = q;
        }
        __syncthreads();
        const uint32_t nBlocks = sNumBlocks;
        for (uint32_t k = wave; k < nBlocks; k += 256 / kWave) {
            const int4 q = sBlocks[k];
            const int bx = q.x, by = q.y, bz = q.z, ptr = q.w;
            const float lox = (float)(bx * VH_SDF_BLOCK_SIZE) * vs - growLo, hix = (float)(bx * VH_SDF_BLOCK_SIZE + VH_SDF_BLOCK_SIZE) * vs + growHi;
            const float loy = (float)(by * VH_SDF_BLOCK_SIZE) * vs - growLo, hiy = (float)(by * VH_SDF_BLOCK_SIZE + VH_SDF_BLOCK_SIZE) * vs + growHi;
            const float loz = (float)(bz * VH_SDF_BLOCK_SIZE) * vs - growLo, hiz = (float)(bz * VH_SDF_BLOCK_SIZE + VH_SDF_BLOCK_SIZE) * vs + growHi;
            float zmin = pinf(), zmax = minf(), xmin = pinf(), xmax = minf(), ymin = pinf(), ymax = minf();
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const F3 pc = mat_mul_p(rp.m_viewMatrix, mk3((c & 1) ? hix : lox, (c & 2) ? hiy : loy, (c & 4) ? hiz : loz));
                zmin = fminf(zmin, pc.z); zmax = fmaxf(zmax, pc.z);
                const float iz = 1.0f / fmaxf(pc.z, 1e-6f);
                const float sx = pc.x * cp.fx * iz + cp.mx, sy = pc.y * cp.fy * iz + cp.my;
                xmin = fminf(xmin, sx); xmax = fmaxf(xmax, sx);
                ymin = fminf(ymin, sy); ymax = fmaxf(ymax, sy);
            }
            if (!(zmax > 0.0f)) continue; // entirely behind the camera: no sample (depth > 0) lies in it
            int tx0 = 0, ty0 = 0, tx1 = tilesX - 1, ty1 = tilesY - 1;
            if (zmin > 0.05f) { // box in front of the camera; otherwise it may project anywhere: every tile
                const float slop = 1.0f + 1e-3f * fmaxf(fmaxf(fabsf(xmin), fabsf(xmax)), fmaxf(fabsf(ymin), fabsf(ymax)));
                // clamp in float first: the float -> int conversion of a huge coordinate is not defined
                tx0 = (int)fminf(fmaxf(floorf((xmin - slop) * 0.125f), 0.0f), (float)tilesX);
                ty0 = (int)fminf(fmaxf(floorf((ymin - slop) * 0.125f), 0.0f), (float)tilesY);
                tx1 = (int)fminf(fmaxf(floorf((xmax + slop) * 0.125f), -1.0f), (float)(tilesX - 1));
                ty1 = (int)fminf(fmaxf(floorf((ymax + slop) * 0.125f), -1.0f), (float)(tilesY - 1));
            }
            if (tx1 < tx0 || ty1 < ty0) continue; // off screen
            const float zs = 1e-3f * fabsf(zmax) + 0.5f * vs;
            const uint32_t lo = __float_as_uint(fmaxf(zmin - zs, 0.0f)), hi = __float_as_uint(fmaxf(zmax + zs, 0.0f));
            const uint32_t nx = (uint32_t)(tx1 - tx0 + 1), n = nx * (uint32_t)(ty1 - ty0 + 1);
            const float rnx = 1.0f / (float)nx;
            constexpr uint32_t kInFlight = 4; // tiles per lane in flight: the list slots come back from L2 together
            for (uint32_t base = 0; base < n; base += kInFlight * kWave) {
                uint32_t t[kInFlight], slot[kInFlight];
#pragma unroll
                for (uint32_t j = 0; j < kInFlight; j++) {
                    const uint32_t i = base + j * kWave + lane;
                    uint32_t qy, qx;
                    divmod_small(i, nx, rnx, qy, qx);
                    t[j] = (uint32_t)(ty0 + (int)qy) * (uint32_t)tilesX + (uint32_t)(tx0 + (int)qx);
                    slot[j] = 0xffffffffu;
                    if (i < n) {
                        slot[j] = atomicAdd(&heads[t[j]].z, 1u);
                    }
                }
#pragma unroll
                for (uint32_t j = 0; j < kInFlight; j++) {
                    if (slot[j] < cap) {
                        lists[(size_t)t[j] * cap + slot[j]] = make_int4(bx, by, bz, ptr);
                    } else if (slot[j] != 0xffffffffu) {
                        // the head's depth range covers the blocks that are NOT listed (all of them without lists);
                        // k_render forms the range of the listed ones itself: two atomics per tile and block less
                        atomicMin(&heads[t[j]].x, lo);
                        atomicMax(&heads[t[j]].y, hi);
                    }
                }
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) sNumBlocks = 0u;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_interval_splat(VhHashData hd, VhHashParams hp, VhDepthCameraParams cp,
                                                        VhRayCastParams rp, uint4* heads, int4* lists, uint32_t cap,
                                                        uint32_t* sched, uint32_t phase, uint32_t numCUs, uint32_t nSplatGroups, uint32_t* feedback)
{
    __shared__ SplatShared sh;
    interval_splat_group(hd, hp, cp, rp, heads, lists, cap, sched, phase, numCUs, nSplatGroups, feedback, blockIdx.x, sh);
}
constexpr uint32_t kSplatThreads = 256; // the splat's launch shape (host): a table's slices (nSplatGroups), then a view's schedule workgroups
inline uint32_t splat_groups(const VhHashParams& hp) { return cdiv((hp.m_hashNumBuckets + 31) / 32, kSplatWordsPerGroup); }
inline uint32_t splat_sched_groups(const VhRayCastParams& rp, const uint32_t* sched) { return sched ? sched_groups(image_tiles(rp.m_width, rp.m_height)) : 0u; }

__global__ __launch_bounds__(256) void k_interval_clear(uint4* heads, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) heads[i] = make_uint4(0x7f800000u, 0u, 0u, 0u); // empty: {+inf, 0, no blocks}
}

} // namespace
