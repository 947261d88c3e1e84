// vh_frame_compactify.hpp -- frame loop: the list of allocated blocks with each block's box in the image (BlockBox,
// compactify_group, k_compactify).  Included by vh_kernels.hip, by vh_frame_integrate.hpp (the pass reads the list and
// its boxes) and by vh_frame_normals.hpp (k_compute_normals carries compactify_group as a rider).
#pragma once

#include "vh_device.hpp"

namespace {
using namespace vhd;

// ---------------------------------------------------------------------------
// compactify (compactifyHashAllInOneKernel, DSC/CUDASceneRepHashSDF.cu:317-359)
//
// The reference scans all Ne entries (32 B each) every frame.  Here the
// 1-bit-per-bucket summary is scanned instead (Nb/8 bytes) and only non-empty
// buckets are opened; kept entries queue up in LDS and the workgroup appends
// them to the list with ONE atomic (compactify_group below).
// ---------------------------------------------------------------------------

// v_cvt_i32_f32 truncates, saturates and sends NaN to 0 by itself: f2i() without the v_trunc_f32 the compiler puts in front
VHD int cvt_rz(float v)
{
    int r;
    asm("v_cvt_i32_f32 %0, %1" : "=v"(r) : "v"(v));
    return r;
}

constexpr uint32_t kIntegrateTile = 32;        // a block's screen footprint of up to 32 x 29 pixels is staged in LDS,
constexpr uint32_t kIntegrateTileRows = 29;    // rows 34 pixels apart (272 B: vertical neighbours fall into different banks):
constexpr uint32_t kIntegrateTileStride = 34;  // 31.6 KB per workgroup = 25 allocation units of 1280 B, five workgroups per compute
                                               // unit (30 rows are 26 units: per-wave time stamps showed four resident, the fifth waiting)

// What the fused integrate pass wants to know of a block before it touches a voxel, worked out once per block by the
// compactify pass (one lane per block there; in the integrate pass it would be ~160 instructions of every wave) and
// kept in the three spare words of the block's entry in the compactified list:
//   box: the block's screen footprint for the frame being integrated -- the hull of its eight corner voxels' pixels, one
//     pixel wider all round (a perspective projection maps the block into the hull of its corners when all of them lie
//     in front of the camera; the extra pixel covers rounding), clipped to the image, starting at an even pixel.  The
//     corners are projected with a hardware reciprocal: the box only decides WHERE a pixel is read from (the tile
//     staged in LDS or the frame itself), never which pixel;
//   VH_BOX_STAGED: the box is worth staging (in front of the camera, at most 32 x 29 pixels, even image width);
//   VH_BOX_CERTIFIED: the range certificate of integrate_block_certified holds at all eight corners (exact arithmetic,
//     the same expressions the voxels go through);
//   tag: which transform / camera / voxel size that was worked out for.  A pass that runs with another one works it
//     out again itself.
constexpr uint32_t VH_BOX_STAGED = 1u, VH_BOX_CERTIFIED = 2u;
struct BlockBox {
    uint32_t x0, y0, w, h, flags;
};
VHD uint32_t frame_tag(const VhHashParams& hp, const VhDepthCameraParams& cp)
{
    uint32_t t = 0x9E3779B9u;
#pragma unroll
    for (int i = 0; i < 12; i++) t = (t ^ __float_as_uint(hp.m_rigidTransformInverse[i])) * 0x01000193u + (t >> 15);
    const uint32_t more[7] = { __float_as_uint(hp.m_virtualVoxelSize), __float_as_uint(cp.fx), __float_as_uint(cp.fy), __float_as_uint(cp.mx),
                               __float_as_uint(cp.my), cp.m_imageWidth, cp.m_imageHeight };
#pragma unroll
    for (int i = 0; i < 7; i++) t = (t ^ more[i]) * 0x01000193u + (t >> 15);
    return (t & 0x7fffffffu) | 1u; // never 0: a zeroed entry carries no box; bit 31 is the mark of a rider_tag
}
// The tag of a list made and read within ONE launch (the pass over the voxels as a rider): the frame's number.  The reader
// takes an entry for this frame's when it carries this tag (CoIntegrate), so the tag must not repeat from one frame to the
// next as frame_tag does when the camera stands still, and must not collide with one by chance.
VHD uint32_t rider_tag(uint32_t frameNumber) { return 0x80000000u | frameNumber; }
struct BoxCorners { // what the eight corners add up to
    int bx0, bx1, by0, by1;
    float cz;
    bool fine;
};
VHD BoxCorners box_no_corner()
{
    BoxCorners a;
    a.bx0 = 0x7fffffff; a.bx1 = (int)0x80000000; a.by0 = 0x7fffffff; a.by1 = (int)0x80000000;
    a.cz = pinf();
    a.fine = true;
    return a;
}
VHD void box_add_corner(const VhHashParams& hp, const VhDepthCameraParams& cp, int ex, int ey, int ez, uint32_t c, BoxCorners& a)
{
    const I3 pc = mki3(ex * VH_SDF_BLOCK_SIZE + ((c & 1u) ? 7 : 0), ey * VH_SDF_BLOCK_SIZE + ((c & 2u) ? 7 : 0), ez * VH_SDF_BLOCK_SIZE + ((c & 4u) ? 7 : 0));
    const F3 pf = mat_mul_p(hp.m_rigidTransformInverse, vvp_to_world(hp.m_virtualVoxelSize, pc));
    const float rz = __builtin_amdgcn_rcpf(pf.z);
    const int cx = cvt_rz((pf.x * cp.fx * rz + cp.mx) + 0.5f), cy = cvt_rz((pf.y * cp.fy * rz + cp.my) + 0.5f); // (saturating; NaN -> 0)
    a.bx0 = min(a.bx0, cx); a.bx1 = max(a.bx1, cx);
    a.by0 = min(a.by0, cy); a.by1 = max(a.by1, cy);
    a.cz = fminf(a.cz, pf.z);
    a.fine = a.fine && pf.z >= 0x1p-20f && pf.z <= 0x1p20f && fabsf(pf.x * cp.fx) <= 0x1p60f && fabsf(pf.y * cp.fy) <= 0x1p60f;
}
VHD BlockBox box_of_corners(const VhDepthCameraParams& cp, const BoxCorners& a)
{
    const bool inFront = a.cz > 1e-3f;
    // (coordinates beyond +-2^30 would overflow the arithmetic below: such a block is simply not staged)
    const bool sane = a.bx0 > -(1 << 30) && a.bx1 < (1 << 30) && a.by0 > -(1 << 30) && a.by1 < (1 << 30);
    const int x0i = max(a.bx0 - 1, 0) & ~1, x1i = min(a.bx1 + 1, (int)cp.m_imageWidth - 1);
    const int y0i = max(a.by0 - 1, 0), y1i = min(a.by1 + 1, (int)cp.m_imageHeight - 1);
    const bool staged = inFront && sane && x0i <= x1i && y0i <= y1i && (x1i - x0i) < (int)kIntegrateTile && (y1i - y0i) < (int)kIntegrateTileRows &&
                        (cp.m_imageWidth & 1u) == 0u && cp.m_imageWidth <= 0xffffu && cp.m_imageHeight <= 0xffffu;
    BlockBox b;
    b.x0 = staged ? (uint32_t)x0i : 0u;
    b.y0 = staged ? (uint32_t)y0i : 0u;
    b.w = staged ? (uint32_t)(x1i - x0i + 1) : 0u;
    b.h = staged ? (uint32_t)(y1i - y0i + 1) : 0u;
    b.flags = (staged ? VH_BOX_STAGED : 0u) | (a.fine ? VH_BOX_CERTIFIED : 0u);
    return b;
}
VHD BlockBox block_box(const VhHashParams& hp, const VhDepthCameraParams& cp, int ex, int ey, int ez)
{
    BoxCorners a = box_no_corner();
#pragma unroll
    for (uint32_t c = 0; c < 8u; c++) box_add_corner(hp, cp, ex, ey, ez, c, a);
    return box_of_corners(cp, a);
}
// the same by eight neighbouring lanes, a corner each (every lane gets the box)
VHD BlockBox block_box_by_eight_lanes(const VhHashParams& hp, const VhDepthCameraParams& cp, int ex, int ey, int ez)
{
    BoxCorners a = box_no_corner();
    box_add_corner(hp, cp, ex, ey, ez, lane_id() & 7u, a);
    int fine = a.fine ? 1 : 0;
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
        a.bx0 = min(a.bx0, __shfl_xor(a.bx0, o)); a.bx1 = max(a.bx1, __shfl_xor(a.bx1, o));
        a.by0 = min(a.by0, __shfl_xor(a.by0, o)); a.by1 = max(a.by1, __shfl_xor(a.by1, o));
        a.cz = fminf(a.cz, __shfl_xor(a.cz, o));
        fine &= __shfl_xor(fine, o);
    }
    a.fine = fine != 0;
    return box_of_corners(cp, a);
}
// the spare words of a compactified entry: {x0 | y0 << 16, w | h << 8 | flags << 16, tag}
VHD uint4 pack_box(uint32_t offset, const BlockBox& b, uint32_t tag) { return make_uint4(offset, b.x0 | (b.y0 << 16), b.w | (b.h << 8) | (b.flags << 16), tag); }

// A workgroup takes 256 words of 32 occupancy bits.  It first gathers its non-empty buckets (a lane per word), then reads
// their slots a lane per slot, four slots in flight per lane: the loads do not depend on each other, so the workgroup's life
// is a few trips to memory -- with a lane per word and a loop over the word's bits it was one trip per set bit of the fullest
// word of the wave, 5-6 us where the launch's other riders need 2 (and the pass over the voxels, when it rides in the same
// launch, waits for the list).  What the workgroup keeps is queued in LDS and appended to the list with ONE atomic per
// workgroup (agent-scope atomics on one address are served one after the other at the memory side of the eight L2s, ~12 ns
// each: with one per wave and slot the dense scene's 8 700 blocks cost 40 us).  The queued entries then get their boxes, one
// lane each.  Entries beyond the queue's capacity take the list directly.
constexpr uint32_t kCompactQueue = 768;
struct CompactShared {
    int4 q[kCompactQueue];
    uint32_t off[kCompactQueue];
    uint32_t n, base, nBuckets;
    uint16_t buckets[256 * 32]; // the non-empty buckets, relative to the workgroup's first
};
// An entry of the compactified list, written and read within ONE launch (the pass over the voxels as a rider of the launch
// that makes its list, k_compute_normals): the L2s of the eight XCDs are not coherent with each other, so such an entry is
// written through and read at the agent's coherence point (relaxed agent-scope atomics: the sc1 forms of the instructions)
// instead of the writers writing their whole L2 back and the readers dropping theirs (a release / acquire pair at agent
// scope costs exactly that, buffer_wbl2 / buffer_inv: measured, +30 us a frame).
template <bool COHERENT> VHD void list_store(VhHashEntry* o, const int4 q, const uint4 box)
{
    if (COHERENT) {
        uint64_t* const w = reinterpret_cast<uint64_t*>(o);
        __hip_atomic_store(w + 0, (uint64_t)(uint32_t)q.x | ((uint64_t)(uint32_t)q.y << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(w + 1, (uint64_t)(uint32_t)q.z | ((uint64_t)(uint32_t)q.w << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(w + 2, (uint64_t)box.x | ((uint64_t)box.y << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // the word with the tag goes last, when the others have arrived: a reader that finds the tag finds the entry
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __hip_atomic_store(w + 3, (uint64_t)box.z | ((uint64_t)box.w << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        *(reinterpret_cast<uint4*>(o) + 1) = box;
        store_quad(o, q);
    }
}
template <bool COHERENT> VHD int4 list_quad(const VhHashEntry* e)
{
    if (COHERENT) {
        const uint64_t* const w = reinterpret_cast<const uint64_t*>(e);
        const uint64_t a = __hip_atomic_load(w + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), b = __hip_atomic_load(w + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return make_int4((int)(uint32_t)a, (int)(uint32_t)(a >> 32), (int)(uint32_t)b, (int)(uint32_t)(b >> 32));
    }
    return load_quad(e);
}
template <bool COHERENT> VHD uint4 list_box(const VhHashEntry* e)
{
    if (COHERENT) {
        const uint64_t* const w = reinterpret_cast<const uint64_t*>(e);
        const uint64_t a = __hip_atomic_load(w + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), b = __hip_atomic_load(w + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
    }
    return *(reinterpret_cast<const uint4*>(e) + 1);
}

template <bool COHERENT = false>
__device__ void compactify_group(const VhHashData& hd, const VhHashParams& hp, const VhDepthCameraParams& cp, uint32_t wordIdx, CompactShared& sh, const uint32_t riderTag = 0u)
{
    const uint32_t nWords = (hp.m_hashNumBuckets + 31) / 32;
    const uint32_t tag = COHERENT ? riderTag : frame_tag(hp, cp);
    const uint32_t lane = lane_id();
#if defined(VH_KNOCKOUT) && VH_KNOCKOUT == 42 // measurement build: the phases of a compactify workgroup (tools/riders_stamps.py)
    uint32_t phase[6];
    phase[0] = (uint32_t)__builtin_amdgcn_s_memrealtime();
#define VH_COMPACT_PHASE(I) phase[I] = (uint32_t)__builtin_amdgcn_s_memrealtime();
#define VH_COMPACT_PHASES_OUT { __syncthreads(); if (threadIdx.x == 0) { uint4* const at = reinterpret_cast<uint4*>(hd.d_hashCompactified) + (hp.m_hashNumBuckets * VH_HASH_BUCKET_SIZE) / 2u + 8192u + 2u * (wordIdx / 256u); \
        at[0] = make_uint4(phase[0], phase[1], phase[2], 0x5743u); at[1] = make_uint4(phase[3], phase[4], (uint32_t)__builtin_amdgcn_s_memrealtime(), sh.n | (sh.nBuckets << 16)); } }
#else
#define VH_COMPACT_PHASE(I)
#define VH_COMPACT_PHASES_OUT
#endif
    if (threadIdx.x == 0) { sh.n = 0u; sh.nBuckets = 0u; }
    __syncthreads();
    // the non-empty buckets, gathered (their order does not matter)
    uint32_t bits = (wordIdx < nWords) ? hd.d_bucketBits[wordIdx] : 0u;
    {
        const uint32_t mine = (uint32_t)__popc(bits);
        uint32_t incl = mine;
#pragma unroll
        for (uint32_t d = 1; d < kWave; d <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)incl, d);
            if (lane >= d) incl += t;
        }
        const uint32_t total = (uint32_t)__shfl((int)incl, kWave - 1);
        uint32_t at = 0;
        if (lane == 0 && total != 0u) at = atomicAdd(&sh.nBuckets, total);
        at = (uint32_t)__shfl((int)at, 0) + incl - mine;
        while (bits != 0u) {
            sh.buckets[at++] = (uint16_t)(threadIdx.x * 32u + (uint32_t)(__ffs((int)bits) - 1));
            bits &= bits - 1u;
        }
    }
    __syncthreads();
    VH_COMPACT_PHASE(1)
    const uint32_t nSlots = sh.nBuckets * VH_HASH_BUCKET_SIZE;
    const uint64_t firstBucket = (uint64_t)(wordIdx - threadIdx.x) * 32u;
    constexpr uint32_t kInFlight = 4; // (eight: 20 registers more for the launch's every wave, and no sooner done)
    for (uint32_t s0 = threadIdx.x; s0 < nSlots; s0 += 256u * kInFlight) { // (s0 < nSlots for all or none of a wave's lanes but in its last trip)
        int4 qs[kInFlight];
        uint32_t offs[kInFlight];
#pragma unroll
        for (uint32_t j = 0; j < kInFlight; j++) {
            const uint32_t slot = s0 + 256u * j;
            qs[j] = make_int4(0, 0, 0, VH_FREE_ENTRY);
            offs[j] = 0;
            if (slot < nSlots) {
                const VhHashEntry* e = &hd.d_hash[(firstBucket + sh.buckets[slot / VH_HASH_BUCKET_SIZE]) * VH_HASH_BUCKET_SIZE + slot % VH_HASH_BUCKET_SIZE];
                qs[j] = load_quad(e);
                offs[j] = e->offset;
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < kInFlight; j++) {
            const int4 q = qs[j];
            const bool keep = q.w != VH_FREE_ENTRY && block_in_frustum(hp, cp, mki3(q.x, q.y, q.z));
            const uint64_t kept = __ballot(keep); // one LDS atomic per wave
            if (kept == 0ull) continue;
            uint32_t at = 0;
            if (lane == 0) at = atomicAdd(&sh.n, (uint32_t)__popcll(kept));
            at = (uint32_t)__shfl((int)at, 0) + (uint32_t)__popcll(kept & lanemask_lt());
            if (keep) {
                if (at < kCompactQueue) {
                    sh.q[at] = q;
                    sh.off[at] = offs[j];
                } else { // the queue is full: straight to the list
                    VhHashEntry* o = &hd.d_hashCompactified[(uint32_t)atomicAdd(hd.d_hashCompactifiedCounter, 1)];
                    list_store<COHERENT>(o, q, pack_box(offs[j], block_box(hp, cp, q.x, q.y, q.z), tag));
                }
            }
        }
    }
    __syncthreads();
    VH_COMPACT_PHASE(2)
    const uint32_t n = min(sh.n, kCompactQueue);
    if (n == 0u) return; // (the same for every thread)
    // the workgroup's place in the list: asked for now, needed when the first boxes are done (a trip to memory)
    uint32_t place = 0;
    if (threadIdx.x == 0) place = (uint32_t)atomicAdd(hd.d_hashCompactifiedCounter, (int)n);
    if (COHERENT) {
        // (the pass that reads this list in the same launch gives a workgroup to every block and never looks at a box: the
        // entries go out as soon as the place is known, the tag in their last word)
        if (threadIdx.x == 0) sh.base = place;
        __syncthreads();
        VH_COMPACT_PHASE(3)
        const uint32_t base = sh.base;
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) list_store<true>(&hd.d_hashCompactified[base + i], sh.q[i], make_uint4(sh.off[i], 0u, 0u, tag));
        VH_COMPACT_PHASE(4)
        VH_COMPACT_PHASES_OUT
        return;
    }
    // the boxes, eight lanes per entry (a corner each: one lane per entry is ~300 instructions in a row, 1 us on a busy unit)
    constexpr uint32_t kBoxRounds = 2; // (rounds of 32 entries whose boxes wait in registers for the place; more entries: after it)
    uint4 boxes[kBoxRounds];
    const uint32_t mine = threadIdx.x >> 3;
#pragma unroll
    for (uint32_t r = 0; r < kBoxRounds; r++) {
        const uint32_t i = min(r * 32u + mine, n - 1u); // (whole groups of eight lanes compute or idle; an idle group repeats the last entry)
        if (r * 32u < n) {
            const int4 q = sh.q[i];
            boxes[r] = pack_box(sh.off[i], block_box_by_eight_lanes(hp, cp, q.x, q.y, q.z), tag);
        }
    }
    if (threadIdx.x == 0) sh.base = place;
    __syncthreads();
    VH_COMPACT_PHASE(3)
    const uint32_t base = sh.base;
#pragma unroll
    for (uint32_t r = 0; r < kBoxRounds; r++) {
        const uint32_t i = r * 32u + mine;
        if (i < n && (threadIdx.x & 7u) == 0u) list_store<COHERENT>(&hd.d_hashCompactified[base + i], sh.q[i], boxes[r]);
    }
    for (uint32_t r = kBoxRounds; r * 32u < n; r++) {
        const uint32_t i = r * 32u + mine;
        const int4 q = sh.q[min(i, n - 1u)];
        const BlockBox b = block_box_by_eight_lanes(hp, cp, q.x, q.y, q.z);
        if (i < n && (threadIdx.x & 7u) == 0u) list_store<COHERENT>(&hd.d_hashCompactified[base + i], q, pack_box(sh.off[i], b, tag));
    }
    VH_COMPACT_PHASE(4)
    VH_COMPACT_PHASES_OUT
}

__global__ __launch_bounds__(256) void k_compactify(VhHashData hd, VhHashParams hp, VhDepthCameraParams cp)
{
    __shared__ CompactShared sh;
    compactify_group(hd, hp, cp, blockIdx.x * blockDim.x + threadIdx.x, sh);
}
constexpr uint32_t kCompactifyThreads = 256; // compactify's launch shape for a table (host): a thread per occupancy word
inline uint32_t compactify_groups(const VhHashParams& hp) { return cdiv((hp.m_hashNumBuckets + 31) / 32, kCompactifyThreads); }

} // namespace
