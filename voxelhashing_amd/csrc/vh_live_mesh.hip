// vh_live_mesh.hip -- the live mesh ("Live mesh"; include/vh_api.h): a cache of the sourced pass 2's
// triangles that one update brings to what a full extraction of the table would give now, by re-extracting only the
// blocks whose 27-block neighbourhood changed.  Not in the reference.
//
// What changed is found from the model alone: a 64-bit digest of every resident block's 512 voxels is held against the
// record of the block's heap id (position, epoch, digest).  The passes of one update, all on one stream:
//   begin     zeroes the counts, reads the cache's triangle count (0 when the last update ended with a status)
//   pass 1    k_mc_pass1 of vh_mc.hip lists the resident entries
//   digest    a wave per four resident blocks: digest, compare, rewrite the record, append changed / moved-away positions
//   vanished  a lane per record: valid and not visited in this epoch -> its position is appended, the record invalidated
//   dilate    a lane per (position, one of 27 offsets): look the block up, stamp its id's mark with the epoch; the first
//             to stamp appends the entry to the re-mesh list R (and the first |C| lanes count the changed and the moved positions)
//   -- the one host wait: |C| and |R| --
//   drop      a lane per cached triangle: kept unless its owner is not resident or is in R; the kept ones are compacted
//             into the SPARE pair of buffers (reads and writes never share a buffer), which then becomes the cache
//   seal      the kept count into the triangle counter
//   pass 2    k_mc_pass2<true> of vh_mc.hip over R, appending behind the kept count
//   finish    total and status; with a status every record is invalidated
// No loop's length depends on data without a bound: the look-ups walk a bucket and at most
// m_hashMaxCollisionLinkedListSize links, the grid-stride loops run to a count the device holds.
//
// MUST be compiled with -ffp-contract=off like every unit (no float arithmetic is done here).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "../../include/vh_api.h"
#include "vh_device.hpp"
#include "vh_host_util.hpp"
#include "vh_mesh_table.hpp"

using namespace vhd;

namespace {

// words of VhLiveMeshData::d_counts behind the VH_LIVE_NUM_COUNTS counts
constexpr uint32_t kStatus = VH_LIVE_NUM_COUNTS, kNumPositions = VH_LIVE_NUM_COUNTS + 1, kOldTriangles = VH_LIVE_NUM_COUNTS + 2,
                   kCountWords = 16;
constexpr uint32_t kNoEntry = 0xffffffffu;
constexpr int kBlockRange = 1 << 16; // block coordinates of voxels in [-2^19, 2^19)

// fmix64, the finaliser weld_home applies (vh_mesh_table.hpp), whole
VHD uint64_t fmix64(uint64_t k)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// The digest of the block at voxel index `ptr` of the pool, in every lane of the calling wave (all 64 lanes call it):
// sum over the 512 voxels of fmix64(w_i + (i + 1) * golden) mod 2^64.  Lane l loads 16 bytes -- voxels 2 (l + 64 k) and the
// next -- at 16 l + 1024 k for k = 0 .. 3: each load instruction covers 1 KB of contiguous memory.
VHD uint64_t block_digest(const VhVoxel* pool, uint32_t ptr, uint32_t lane)
{
    constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;
    const uint4* src = reinterpret_cast<const uint4*>(pool + ptr); // ptr is a multiple of 512 voxels: 4 KB aligned
    uint4 v[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) v[k] = src[lane + 64u * k];
    uint64_t sum = 0ull;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        const uint64_t i = 2ull * (lane + 64u * k);
        const uint64_t w0 = (uint64_t)v[k].x | ((uint64_t)v[k].y << 32), w1 = (uint64_t)v[k].z | ((uint64_t)v[k].w << 32);
        sum += fmix64(w0 + (i + 1ull) * kGolden) + fmix64(w1 + (i + 2ull) * kGolden);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { // the sum commutes: a butterfly leaves the total in every lane
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)sum, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(sum >> 32), off);
        sum += (uint64_t)lo | ((uint64_t)hi << 32);
    }
    return sum;
}

// getHashEntryForSDFBlockPos (lookup_ptr of vh_device.hpp) returning the entry's index beside its ptr: pass 2's block
// list names entries.  Nothing allocates beside an update, so the stale-line retry of lookup_ptr is not needed.
VHD uint32_t lookup_entry(const VhHashData& hd, const VhHashParams& hp, I3 blk, int& ptr)
{
    ptr = VH_FREE_ENTRY;
    const uint32_t ne = hp.m_hashNumBuckets * VH_HASH_BUCKET_SIZE;
    const uint32_t h = hash_pos(hp.m_hashNumBuckets, blk);
    if (!bucket_maybe_occupied(hd, h)) return kNoEntry;
    const uint32_t base = h * VH_HASH_BUCKET_SIZE;
#pragma unroll 1
    for (uint32_t j = 0; j < VH_HASH_BUCKET_SIZE; j++) {
        const int4 q = load_quad(&hd.d_hash[base + j]);
        if (quad_matches(q, blk)) { ptr = q.w; return base + j; }
    }
    const uint32_t idxLast = base + VH_HASH_BUCKET_SIZE - 1;
    uint32_t i = idxLast, maxIter = 0;
#pragma unroll 1
    while (maxIter < hp.m_hashMaxCollisionLinkedListSize) {
        const int4 q = load_quad(&hd.d_hash[i]);
        if (quad_matches(q, blk)) { ptr = q.w; return i; }
        const uint32_t off = hd.d_hash[i].offset;
        if (off == 0) break;
        i = (idxLast + off) % ne;
        maxIter++;
    }
    return kNoEntry;
}

// the heap id of a resident entry's ptr, or kNoEntry for one that names no block of the pool (a table written by hand)
VHD uint32_t block_id(int ptr, uint32_t numSDFBlocks)
{
    if (ptr < 0 || ((uint32_t)ptr % VH_SDF_BLOCK_VOXELS) != 0u) return kNoEntry;
    const uint32_t id = (uint32_t)ptr / VH_SDF_BLOCK_VOXELS;
    return id < numSDFBlocks ? id : kNoEntry;
}

__global__ void k_live_begin(VhLiveMeshData live, const uint32_t* numTriangles, uint32_t* numOccupied, uint32_t fresh)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    // a cache that the last update left with a status holds nothing
    const uint32_t old = (fresh || live.d_counts[kStatus] != 0u) ? 0u : min(numTriangles[0], live.m_maxNumTriangles);
    for (uint32_t i = 0; i < kCountWords; i++) live.d_counts[i] = 0u;
    live.d_counts[kOldTriangles] = old;
    numOccupied[0] = 0u;
}

// blocks that one wave digests before it appends their positions: one atomic for up to 2 kDigestBatch positions.  (With an
// atomic a changed block, an update in which every block changed spent most of the kernel in line at one counter.)
constexpr uint32_t kDigestBatch = 4;
// tags of a position in d_positions[..].w: what the dilate pass counts it as
constexpr int kTagChanged = 0, kTagMoved = 1, kTagGone = 2;

// Step 1 of an update.  A wave per kDigestBatch resident blocks: for each the digest, then the comparison with the record
// of the block's heap id -- every lane reads the record and comes to the same verdict, lane 0 rewrites it -- and the
// changed block's position, and the position a moved id had, go into the registers of lanes 0, 1, ... until the wave
// appends them together.
__global__ __launch_bounds__(256) void k_live_digest(VhHashData hd, VhHashParams hp, const uint32_t* occupied, const uint32_t* numOccupied,
                                                     VhLiveMeshData live, uint32_t epoch)
{
    const uint32_t n = numOccupied[0], lane = lane_id();
    const uint32_t nWaves = (gridDim.x * blockDim.x) / kWave;
#pragma unroll 1
    for (uint32_t first = ((blockIdx.x * blockDim.x + threadIdx.x) / kWave) * kDigestBatch; first < n; first += nWaves * kDigestBatch) { // wave-uniform
        uint32_t cnt = 0u, status = 0u;
        int4 mine = make_int4(0, 0, 0, 0);
#pragma unroll 1
        for (uint32_t w = first; w < min(first + kDigestBatch, n); w++) {
            const int4 q = load_quad(&hd.d_hash[occupied[w]]);
            if (q.w == VH_FREE_ENTRY) continue;
            const uint32_t id = block_id(q.w, live.m_numSDFBlocks);
            if (id == kNoEntry) { status |= VH_LIVE_BAD_TABLE; continue; }
            const uint64_t d = block_digest(hd.d_SDFBlocks, (uint32_t)q.w, lane);
            VhLiveMeshRecord* rec = &live.d_records[id];
            const VhLiveMeshRecord r = *rec;
            if (r.epoch == epoch) { status |= VH_LIVE_BAD_TABLE; continue; } // a second entry with this block: a table written by hand
            if (q.x < -kBlockRange || q.x >= kBlockRange || q.y < -kBlockRange || q.y >= kBlockRange || q.z < -kBlockRange || q.z >= kBlockRange)
                status |= VH_LIVE_RANGE;
            const bool valid = r.epoch != 0u, moved = valid && (r.pos[0] != q.x || r.pos[1] != q.y || r.pos[2] != q.z);
            if (!valid || moved || r.digest != d) {
                if (lane == cnt) mine = make_int4(q.x, q.y, q.z, kTagChanged);
                cnt++;
                if (moved) {
                    if (lane == cnt) mine = make_int4(r.pos[0], r.pos[1], r.pos[2], kTagMoved);
                    cnt++;
                }
            }
            if (lane == 0u) {
                VhLiveMeshRecord out;
                out.pos[0] = q.x; out.pos[1] = q.y; out.pos[2] = q.z; out.epoch = epoch; out.digest = d;
                *rec = out;
            }
        }
        if (status != 0u && lane == 0u) atomicOr(&live.d_counts[kStatus], status);
        if (cnt == 0u) continue; // wave-uniform, as everything above
        uint32_t at = 0u;
        if (lane == 0u) at = atomicAdd(&live.d_counts[kNumPositions], cnt);
        at = (uint32_t)__builtin_amdgcn_readfirstlane((int)at);
        if (lane < cnt) {
            if (at + cnt <= 2u * live.m_numSDFBlocks) reinterpret_cast<int4*>(live.d_positions)[at + lane] = mine;
            else atomicOr(&live.d_counts[kStatus], VH_LIVE_BAD_TABLE);
        }
    }
}

// over the record array: numSDFBlocks records of 24 B, whatever the last update visited
__global__ __launch_bounds__(256) void k_live_vanished(VhLiveMeshData live, uint32_t epoch)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool gone = false;
    VhLiveMeshRecord r;
    if (i < live.m_numSDFBlocks) {
        r = live.d_records[i];
        gone = r.epoch != 0u && r.epoch != epoch;
    }
    const uint32_t at = wave_append(gone, &live.d_counts[kNumPositions]);
    wave_count(gone, &live.d_counts[VH_LIVE_VANISHED]);
    if (!gone) return;
    live.d_records[i].epoch = 0u;
    if (at < 2u * live.m_numSDFBlocks) reinterpret_cast<int4*>(live.d_positions)[at] = make_int4(r.pos[0], r.pos[1], r.pos[2], kTagGone);
    else atomicOr(&live.d_counts[kStatus], VH_LIVE_BAD_TABLE);
}

__global__ __launch_bounds__(256) void k_live_dilate(VhHashData hd, VhHashParams hp, VhLiveMeshData live, uint32_t epoch)
{
    const uint32_t numPositions = min(live.d_counts[kNumPositions], 2u * live.m_numSDFBlocks);
    const uint32_t total = numPositions * 27u; // < 2^32: numSDFBlocks < 2^22 (alloc)
    const uint32_t stride = gridDim.x * blockDim.x, lane = lane_id();
#pragma unroll 1
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i - lane < total; i += stride) { // wave-uniform
        bool first = false;
        uint32_t entry = kNoEntry;
        // the digest pass left the counting of its positions to this one: lane i < |C| counts position i, so that the
        // counters see an atomic for every 64 positions
        const int tag = i < numPositions ? live.d_positions[4u * i + 3u] : -1;
        if (i < total) {
            const int4 p = reinterpret_cast<const int4*>(live.d_positions)[i / 27u];
            const uint32_t o = i % 27u;
            // (wrapping sums: a position out of range has raised VH_LIVE_RANGE, and the look-up of whatever comes out is defined)
            const I3 blk = mki3((int)((uint32_t)p.x + (o % 3u) - 1u), (int)((uint32_t)p.y + ((o / 3u) % 3u) - 1u), (int)((uint32_t)p.z + (o / 9u) - 1u));
            int ptr;
            entry = lookup_entry(hd, hp, blk, ptr);
            const uint32_t id = entry != kNoEntry ? block_id(ptr, live.m_numSDFBlocks) : kNoEntry;
            if (id != kNoEntry) first = atomicMax(&live.d_marks[id], epoch) != epoch; // marks never exceed the epoch
        }
        wave_count(tag == kTagChanged, &live.d_counts[VH_LIVE_CHANGED]);
        wave_count(tag == kTagMoved, &live.d_counts[VH_LIVE_VANISHED]);
        const uint32_t at = wave_append(first, &live.d_counts[VH_LIVE_REMESHED]);
        if (first && at < live.m_numSDFBlocks) live.d_remesh[at] = entry; // (distinct ids: at most numSDFBlocks of them)
    }
}

// two dwords at a time: a VhTriangle is 72 B at a multiple of 8
VHD void copy_triangle(VhTriangle* dst, const VhTriangle* src)
{
    const uint2* s = reinterpret_cast<const uint2*>(src);
    uint2* d = reinterpret_cast<uint2*>(dst);
    uint2 v[9];
#pragma unroll
    for (int k = 0; k < 9; k++) v[k] = s[k];
#pragma unroll
    for (int k = 0; k < 9; k++) d[k] = v[k];
}

__global__ __launch_bounds__(256) void k_live_drop(VhHashData hd, VhHashParams hp, VhLiveMeshData live, uint32_t epoch, const VhTriangle* triangles,
                                                   const VhTriangleSource* sources, VhTriangle* outTriangles, VhTriangleSource* outSources)
{
    const uint32_t n = live.d_counts[kOldTriangles];
    const uint32_t stride = gridDim.x * blockDim.x, lane = lane_id();
#pragma unroll 1
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i - lane < n; i += stride) { // wave-uniform
        bool keep = false;
        int4 src = make_int4(0, 0, 0, 0);
        if (i < n) {
            src = *reinterpret_cast<const int4*>(&sources[i]);
            const int ptr = lookup_ptr(hd, hp, vvp_to_block(mki3(src.x, src.y, src.z))); // the owner: floor(cell / 8), as pass 2 deals cells
            const uint32_t id = block_id(ptr, live.m_numSDFBlocks);
            keep = id != kNoEntry && live.d_marks[id] != epoch;
        }
        const uint32_t at = wave_append(keep, &live.d_counts[VH_LIVE_KEPT]); // at < n <= m_maxNumTriangles
        if (keep) {
            copy_triangle(&outTriangles[at], &triangles[i]);
            *reinterpret_cast<int4*>(&outSources[at]) = src;
        }
    }
}

// skipped: nothing changed and nothing vanished, the drop pass did not run and the cache is where it was
__global__ void k_live_seal(VhLiveMeshData live, uint32_t* numTriangles, const uint32_t* numOccupied, uint32_t skipped)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint32_t old = live.d_counts[kOldTriangles];
    const uint32_t kept = skipped ? old : live.d_counts[VH_LIVE_KEPT];
    live.d_counts[VH_LIVE_KEPT] = kept;
    live.d_counts[VH_LIVE_DROPPED] = old - kept;
    live.d_counts[VH_LIVE_VISITED] = numOccupied[0];
    numTriangles[0] = kept;
}

__global__ __launch_bounds__(256) void k_live_finish(VhLiveMeshData live, const uint32_t* numTriangles)
{
    const uint32_t total = numTriangles[0]; // counts what pass 2 made, also what did not fit
    const bool over = total > live.m_maxNumTriangles;
    const bool bad = over || (live.d_counts[kStatus] & ~VH_LIVE_OVERFLOW) != 0u; // (thread 0 below adds that bit only when `over`)
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0u) {
        live.d_counts[VH_LIVE_TOTAL] = total;
        live.d_counts[VH_LIVE_ADDED] = total - live.d_counts[VH_LIVE_KEPT];
        if (over) live.d_counts[kStatus] |= VH_LIVE_OVERFLOW;
    }
    if (bad && i < live.m_numSDFBlocks) live.d_records[i].epoch = 0u; // the next update starts from nothing (k_live_begin)
}

__global__ __launch_bounds__(256) void k_live_digest_list(VhHashData hd, VhHashParams hp, const uint32_t* entries, uint32_t n, uint64_t* out)
{
    const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) / kWave, lane = lane_id();
    if (w >= n) return; // wave-uniform
    const uint32_t e = entries[w];
    uint64_t d = 0ull;
    if (e < hp.m_hashNumBuckets * VH_HASH_BUCKET_SIZE) {
        const int ptr = hd.d_hash[e].ptr;
        if (block_id(ptr, hp.m_numSDFBlocks) != kNoEntry) d = block_digest(hd.d_SDFBlocks, (uint32_t)ptr, lane);
    }
    if (lane == 0u) out[w] = d;
}

bool live_complete(const VhLiveMeshData* l)
{
    return l && l->d_records && l->d_positions && l->d_marks && l->d_remesh && l->d_spareTriangles && l->d_spareSources && l->d_counts &&
           l->m_numSDFBlocks != 0 && l->m_maxNumTriangles != 0;
}

} // namespace

extern "C" {

int vh_live_mesh_data_alloc(VhLiveMeshData* live, uint32_t numSDFBlocks, uint32_t maxNumTriangles)
{
    if (!live || numSDFBlocks == 0 || numSDFBlocks >= (1u << 22) || maxNumTriangles == 0) return VH_ERR_BAD_ARGUMENT;
    std::memset(live, 0, sizeof(*live));
    const size_t nb = numSDFBlocks;
    const int r = [&]() -> int {
        VH_HIP(hipMalloc((void**)&live->d_records, sizeof(VhLiveMeshRecord) * nb));
        VH_HIP(hipMalloc((void**)&live->d_positions, sizeof(int32_t) * 4 * 2 * nb));
        VH_HIP(hipMalloc((void**)&live->d_marks, sizeof(uint32_t) * nb));
        VH_HIP(hipMalloc((void**)&live->d_remesh, sizeof(uint32_t) * nb));
        VH_HIP(hipMalloc((void**)&live->d_spareTriangles, sizeof(VhTriangle) * (size_t)maxNumTriangles));
        VH_HIP(hipMalloc((void**)&live->d_spareSources, sizeof(VhTriangleSource) * (size_t)maxNumTriangles));
        VH_HIP(hipMalloc((void**)&live->d_counts, sizeof(uint32_t) * kCountWords));
        VH_HIP(hipMemset(live->d_records, 0, sizeof(VhLiveMeshRecord) * nb));
        VH_HIP(hipMemset(live->d_marks, 0, sizeof(uint32_t) * nb));
        VH_HIP(hipMemset(live->d_counts, 0, sizeof(uint32_t) * kCountWords));
        return VH_OK;
    }();
    if (r != VH_OK) {
        vh_live_mesh_data_free(live);
        return r;
    }
    live->m_numSDFBlocks = numSDFBlocks;
    live->m_maxNumTriangles = maxNumTriangles;
    live->m_fresh = 1;
    return VH_OK;
}

void vh_live_mesh_data_free(VhLiveMeshData* live)
{
    if (!live) return;
    if (live->d_records) (void)hipFree(live->d_records);
    if (live->d_positions) (void)hipFree(live->d_positions);
    if (live->d_marks) (void)hipFree(live->d_marks);
    if (live->d_remesh) (void)hipFree(live->d_remesh);
    if (live->d_spareTriangles) (void)hipFree(live->d_spareTriangles);
    if (live->d_spareSources) (void)hipFree(live->d_spareSources);
    if (live->d_counts) (void)hipFree(live->d_counts);
    std::memset(live, 0, sizeof(*live));
}

int vh_live_mesh_reset(VhLiveMeshData* live, vhStream_t stream)
{
    if (!live_complete(live)) return VH_ERR_BAD_ARGUMENT;
    VH_HIP(hipMemsetAsync(live->d_records, 0, sizeof(VhLiveMeshRecord) * (size_t)live->m_numSDFBlocks, (hipStream_t)stream));
    VH_HIP(hipMemsetAsync(live->d_counts, 0, sizeof(uint32_t) * kCountWords, (hipStream_t)stream));
    live->m_fresh = 1; // the next update takes the cache as empty, and the hash parameters as they come
    return VH_OK;
}

int vh_live_mesh_update(const VhHashData* hd, const VhHashParams* hp, VhMarchingCubesData* mcData, VhTriangleSource** d_sources, VhLiveMeshData* live,
                        vhStream_t stream)
{
    if (!hd || !hp || !mcData || !d_sources || !*d_sources || !live_complete(live)) return VH_ERR_BAD_ARGUMENT;
    if (!mcData->d_params || !mcData->d_triangles || !mcData->d_numTriangles || !mcData->d_numOccupiedBlocks || !mcData->d_occupiedBlocks) return VH_ERR_BAD_ARGUMENT;
    if (hp->m_numSDFBlocks != live->m_numSDFBlocks || hp->m_hashNumBuckets == 0 || hp->m_hashBucketSize != VH_HASH_BUCKET_SIZE) return VH_ERR_BAD_ARGUMENT;
    if (!live->m_fresh && (hp->m_hashNumBuckets != live->m_hashNumBuckets || hp->m_hashMaxCollisionLinkedListSize != live->m_hashMaxCollisionLinkedListSize ||
                           hp->m_virtualVoxelSize != live->m_virtualVoxelSize))
        return VH_ERR_BAD_ARGUMENT; // the cache was made under other parameters: nothing is done
    const hipStream_t s = (hipStream_t)stream;
    if (live->m_epoch == 0xffffffffu) { // the epoch wraps: forget every mark and record
        VH_HIP(hipMemsetAsync(live->d_marks, 0, sizeof(uint32_t) * (size_t)live->m_numSDFBlocks, s));
        VH_HIP(hipMemsetAsync(live->d_records, 0, sizeof(VhLiveMeshRecord) * (size_t)live->m_numSDFBlocks, s));
        live->m_epoch = 0;
        live->m_fresh = 1;
    }
    const uint32_t epoch = ++live->m_epoch, nb = live->m_numSDFBlocks;
    k_live_begin<<<1, 64, 0, s>>>(*live, mcData->d_numTriangles, mcData->d_numOccupiedBlocks, live->m_fresh);
    live->m_fresh = 0;
    live->m_hashNumBuckets = hp->m_hashNumBuckets;
    live->m_hashMaxCollisionLinkedListSize = hp->m_hashMaxCollisionLinkedListSize;
    live->m_virtualVoxelSize = hp->m_virtualVoxelSize;
    VH_TRY(vh_extract_iso_surface_pass1(hd, hp, mcData, stream));
    // grid-stride over counts the device holds; the grids cover the most there can be, up to a few waves per SIMD
    VH_LAUNCH_TIMED(k_live_digest, std::min(cdiv((uint64_t)cdiv(nb, kDigestBatch) * kWave, 256), 4096u), 256, s, *hd, *hp, mcData->d_occupiedBlocks, mcData->d_numOccupiedBlocks, *live, epoch);
    VH_LAUNCH_TIMED(k_live_vanished, cdiv(nb, 256), 256, s, *live, epoch);
    VH_LAUNCH_TIMED(k_live_dilate, std::min(cdiv((uint64_t)nb * 2 * 27, 256), 2048u), 256, s, *hd, *hp, *live, epoch);
    VH_TRY(vh_last_launch_error());
    uint32_t words[kCountWords];
    VH_HIP(hipMemcpyAsync(words, live->d_counts, sizeof(words), hipMemcpyDeviceToHost, s));
    VH_HIP(hipStreamSynchronize(s)); // the one wait of an update: pass 2's grid is |R|
    const uint32_t numRemesh = std::min(words[VH_LIVE_REMESHED], nb), numOld = words[kOldTriangles];
    const bool skip = words[kNumPositions] == 0u; // nothing changed, nothing vanished: R is empty and nothing is dropped
    if (!skip) {
        if (numOld != 0u)
            VH_LAUNCH_TIMED(k_live_drop, std::min(cdiv(numOld, 256), 4096u), 256, s, *hd, *hp, *live, epoch, mcData->d_triangles, *d_sources, live->d_spareTriangles,
                            live->d_spareSources);
        std::swap(mcData->d_triangles, live->d_spareTriangles);
        std::swap(*d_sources, live->d_spareSources);
    }
    k_live_seal<<<1, 64, 0, s>>>(*live, mcData->d_numTriangles, mcData->d_numOccupiedBlocks, skip ? 1u : 0u);
    VH_TRY(vh_last_launch_error());
    if (numRemesh != 0u) {
        VhMarchingCubesData over = *mcData;
        over.d_occupiedBlocks = live->d_remesh;
        VH_TRY(vh_extract_iso_surface_pass2_sourced(hd, hp, &over, *d_sources, numRemesh, stream));
    }
    k_live_finish<<<cdiv(nb, 256), 256, 0, s>>>(*live, mcData->d_numTriangles);
    return vh_last_launch_error();
}

int vh_live_mesh_get_counts(const VhLiveMeshData* live, uint32_t out[VH_LIVE_NUM_COUNTS + 1], vhStream_t stream)
{
    if (!live || !live->d_counts || !out) return VH_ERR_BAD_ARGUMENT;
    VH_HIP(hipMemcpyAsync(out, live->d_counts, sizeof(uint32_t) * (VH_LIVE_NUM_COUNTS + 1), hipMemcpyDeviceToHost, (hipStream_t)stream));
    VH_HIP(hipStreamSynchronize((hipStream_t)stream));
    const uint32_t status = out[VH_LIVE_NUM_COUNTS];
    if (status & (VH_LIVE_RANGE | VH_LIVE_BAD_TABLE)) return VH_ERR_BAD_ARGUMENT;
    if (status & VH_LIVE_OVERFLOW) return VH_ERR_STAGING_OVERFLOW;
    return VH_OK;
}

int vh_live_mesh_digest(const VhHashData* hd, const VhHashParams* hp, const uint32_t* d_entryIndices, uint32_t n, uint64_t* d_out, vhStream_t stream)
{
    if (!hd || !hp || !hd->d_hash || !hd->d_SDFBlocks || hp->m_hashNumBuckets == 0) return VH_ERR_BAD_ARGUMENT;
    if (n == 0) return VH_OK;
    if (!d_entryIndices || !d_out) return VH_ERR_BAD_ARGUMENT;
    VH_LAUNCH_TIMED(k_live_digest_list, cdiv((uint64_t)n * kWave, 256), 256, (hipStream_t)stream, *hd, *hp, d_entryIndices, n, d_out);
    return vh_last_launch_error();
}

} // extern "C"
