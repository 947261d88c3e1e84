// vh_device.hpp -- device-side functions of the voxel-hash TSDF path (gfx950).
//
// Behavioural contract: DSC/VoxelUtilHashSDF.h, DSC/DepthCameraUtil.h
// (DSC/ = /root/reference/DepthSensingCUDA/Source/); each function cites the
// lines whose semantics it must reproduce.  Numerics are IEEE fp32 with one
// rounding per operation: this translation unit MUST be compiled with
// -ffp-contract=off and without fast-math (block ids and pixel ids are
// float->int cliffs; see DESIGN.md "Numerics").
//
// Parameters travel as kernel arguments (wave-uniform, SGPR-resident), not as
// process-global __constant__ symbols.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vh_types.h"

namespace vhd {

struct F3 { float x, y, z; };
struct I3 { int x, y, z; };

#define VHD __device__ __forceinline__

VHD float minf() { return __int_as_float((int)0xff800000u); }
VHD float pinf() { return __int_as_float((int)0x7f800000u); }

VHD F3 mk3(float x, float y, float z) { F3 r; r.x = x; r.y = y; r.z = z; return r; }
VHD I3 mki3(int x, int y, int z) { I3 r; r.x = x; r.y = y; r.z = z; return r; }
VHD float dot3(F3 a, F3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// float -> int, round toward zero, saturating, NaN -> 0: v_cvt_i32_f32 has
// exactly the semantics of the cvt.rzi.s32.f32 the reference executes.
VHD int f2i(float v) { return __float2int_rz(v); }
// float -> uchar, saturating (cvt.rzi.u8.f32)
VHD uint8_t f2uc(float v) { return (uint8_t)__float2int_rz(fminf(fmaxf(v, 0.0f), 255.0f)); }

// cutil_math.h:31-33
VHD int signi(float v) { return (0.0f < v) - (v < 0.0f); }

// normalize, cutil_math.h:1207-1211 with rsqrtf = 1/sqrtf (cutil_math.h:81-84)
VHD F3 normalize3(F3 v)
{
    float invLen = 1.0f / sqrtf(dot3(v, v));
    return mk3(v.x * invLen, v.y * invLen, v.z * invLen);
}

// float4x4 * float3 (w = 1), DSC/cuda_SimpleMatrixUtil.h:900-907
VHD F3 mat_mul_p(const float* m, F3 v)
{
    return mk3(m[0] * v.x + m[1] * v.y + m[2] * v.z + m[3] * 1.0f,
               m[4] * v.x + m[5] * v.y + m[6] * v.z + m[7] * 1.0f,
               m[8] * v.x + m[9] * v.y + m[10] * v.z + m[11] * 1.0f);
}
// xyz of float4x4 * float4(v, 0), DSC/cuda_SimpleMatrixUtil.h:888-896
VHD F3 mat_mul_d(const float* m, F3 v)
{
    const float w = 0.0f;
    return mk3(m[0] * v.x + m[1] * v.y + m[2] * v.z + m[3] * w,
               m[4] * v.x + m[5] * v.y + m[6] * v.z + m[7] * w,
               m[8] * v.x + m[9] * v.y + m[10] * v.z + m[11] * w);
}

// ---------------------------------------------------------------------------
// coordinate helpers (DSC/VoxelUtilHashSDF.h)
// ---------------------------------------------------------------------------

// computeHashPos :217-225 (wrapping int products, unsigned modulo)
VHD uint32_t hash_pos(uint32_t numBuckets, I3 p)
{
    const uint32_t p0 = 73856093u, p1 = 19349669u, p2 = 83492791u;
    uint32_t r = ((uint32_t)p.x * p0) ^ ((uint32_t)p.y * p1) ^ ((uint32_t)p.z * p2);
    return r % numBuckets;
}

// The reference's rounding of a quotient, (int)(p + sign(p) * 0.5f) with sign(p) in {-1, 0, 1} (:266-270, and
// worldToChunks), as p + copysignf(0.5f, p): a v_bfi_b32 and an add where the sign takes two compares, a select, a
// subtract, a conversion and a multiply.  The two differ only where sign(p) is 0: for p = +-0 the sum is +-0.5 here and
// 0 there, and both truncate to 0; for a NaN both sums are NaN, which converts to 0.  Every other p, the infinities
// included, gets the same sum.  k_check_fast_math (vh_util.hip) holds the two against each other on the device,
// tests/test_exact_voxel_coords.py in numpy.
VHD int round_half_away(float p) { return f2i(p + copysignf(0.5f, p)); }

// worldToVirtualVoxelPos :266-270, one component
VHD int world_to_vvp1(float pos, float voxelSize)
{
    return round_half_away(pos / voxelSize);
}
VHD I3 world_to_vvp(float voxelSize, F3 pos)
{
    return mki3(world_to_vvp1(pos.x, voxelSize), world_to_vvp1(pos.y, voxelSize), world_to_vvp1(pos.z, voxelSize));
}
// virtualVoxelPosToSDFBlock :273-282: (v < 0 ? v - 7 : v) / 8 with C's division, which is floor(v / 8), which is the
// arithmetic shift -- for every v >= INT_MIN + 7.  Below that the reference's v - 7 overflows (undefined in C; the
// wrapped value is a positive block no voxel of the scene is near), and such a v is only ever the saturated conversion
// of a position 2^31 voxels away.  (One instruction for seven; k_check_fast_math and tests/test_exact_voxel_coords.py.)
static_assert(VH_SDF_BLOCK_SIZE == 8, "vvp_to_block1");
VHD int vvp_to_block1(int v)
{
    return v >> 3;
}
VHD I3 vvp_to_block(I3 v) { return mki3(vvp_to_block1(v.x), vvp_to_block1(v.y), vvp_to_block1(v.z)); }
// SDFBlockToVirtualVoxelPos :286 / virtualVoxelPosToWorld :291 / SDFBlockToWorld :296
VHD F3 vvp_to_world(float voxelSize, I3 v) { return mk3((float)v.x * voxelSize, (float)v.y * voxelSize, (float)v.z * voxelSize); }
VHD F3 block_to_world(float voxelSize, I3 b)
{
    return vvp_to_world(voxelSize, mki3(b.x * VH_SDF_BLOCK_SIZE, b.y * VH_SDF_BLOCK_SIZE, b.z * VH_SDF_BLOCK_SIZE));
}
VHD I3 world_to_block(float voxelSize, F3 p) { return vvp_to_block(world_to_vvp(voxelSize, p)); }
// virtualVoxelPosToLocalSDFBlockIndex :330-341
VHD int local1(int v)
{
    int l = v % VH_SDF_BLOCK_SIZE;
    if (l < 0) l += VH_SDF_BLOCK_SIZE;
    return l;
}
VHD int vvp_to_local_index(I3 v)
{
    return local1(v.z) * VH_SDF_BLOCK_SIZE * VH_SDF_BLOCK_SIZE + local1(v.y) * VH_SDF_BLOCK_SIZE + local1(v.x);
}
// getTruncation :255-257
VHD float get_truncation(const VhHashParams& hp, float z) { return hp.m_truncation + hp.m_truncScale * z; }

// ---------------------------------------------------------------------------
// cheaper exact arithmetic for the hot loops
// ---------------------------------------------------------------------------

// a / b, correctly rounded, for a loop-invariant divisor b with rb = 1.0f / b
// (IEEE).  Two Markstein correction steps on q = a*rb, the same refinement the
// compiler's division expansion performs after its reciprocal -- 5 VALU ops
// instead of ~11.  Exact for finite operands whose quotient is a normal
// number (positions / voxel size); verified against `/` by
// vh_debug_check_fast_math and by the bit-exact raycast parity tests.
VHD float div_exact(float a, float b, float rb)
{
    float q = a * rb;
    float e = __fmaf_rn(-b, q, a);
    q = __fmaf_rn(e, rb, q);
    e = __fmaf_rn(-b, q, a);
    q = __fmaf_rn(e, rb, q);
    return q;
}
// ---- two fp32 values as a two-vector: packed fp32 instructions (v_pk_mul/add/fma_f32: two IEEE operations per issue
// slot; each component is the scalar instruction's result).  The frame-loop unit is compiled without the SLP vectorizer
// (build.py): what is packed there is what is written with these.
typedef float f32x2 __attribute__((ext_vector_type(2)));
VHD f32x2 both(float v) { return (f32x2){ v, v }; }
VHD f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
// div_exact for two dividends
VHD f32x2 div_exact2(f32x2 a, float b, float rb)
{
    const f32x2 b2 = both(b), rb2 = both(rb);
    f32x2 q = a * rb2;
    f32x2 e = fma2(-b2, q, a);
    q = fma2(e, rb2, q);
    e = fma2(-b2, q, a);
    q = fma2(e, rb2, q);
    return q;
}
VHD int world_to_vvp1_rb(float pos, float voxelSize, float rVoxelSize)
{
    return round_half_away(div_exact(pos, voxelSize, rVoxelSize));
}

// n % d for an invariant d through a host-computed multiply-shift
// (Granlund-Montgomery round-up method, exact for every 32-bit n; d >= 2)
struct HashMod {
    uint32_t d, m, sh;
};
// multiply-shift constants of umod_fast for divisor d >= 2
inline HashMod make_hash_mod(uint32_t d)
{
    HashMod k;
    k.d = d;
    uint32_t l = 0;
    while ((1ull << l) < (uint64_t)d) l++;
    k.m = (uint32_t)((((1ull << 32) * ((1ull << l) - (uint64_t)d)) / d) + 1ull);
    k.sh = l - 1;
    return k;
}
VHD uint32_t umod_fast(uint32_t n, HashMod k)
{
    const uint32_t q0 = __umulhi(k.m, n);
    const uint32_t t = ((n - q0) >> 1) + q0;
    const uint32_t q = t >> k.sh;
    return n - q * k.d;
}
VHD uint32_t hash_pos_fast(HashMod k, I3 p)
{
    const uint32_t p0 = 73856093u, p1 = 19349669u, p2 = 83492791u;
    return umod_fast(((uint32_t)p.x * p0) ^ ((uint32_t)p.y * p1) ^ ((uint32_t)p.z * p2), k);
}

// ---------------------------------------------------------------------------
// camera helpers (DSC/DepthCameraUtil.h)
// ---------------------------------------------------------------------------

// kinectDepthToSkeleton :117-122
VHD F3 depth_to_skeleton(const VhDepthCameraParams& cp, uint32_t ux, uint32_t uy, float depth)
{
    const float x = ((float)ux - cp.mx) / cp.fx;
    const float y = ((float)uy - cp.my) / cp.fy;
    return mk3(depth * x, depth * y, depth);
}
// cameraToKinectProjZ :94-96
VHD float cam_to_proj_z(const VhDepthCameraParams& cp, float z)
{
    return (z - cp.m_sensorDepthWorldMin) / (cp.m_sensorDepthWorldMax - cp.m_sensorDepthWorldMin);
}
// kinectProjToCameraZ :129-131
VHD float proj_to_cam_z(const VhDepthCameraParams& cp, float z)
{
    return z * (cp.m_sensorDepthWorldMax - cp.m_sensorDepthWorldMin) + cp.m_sensorDepthWorldMin;
}
// isInCameraFrustumApprox :141-147 over cameraToKinectProj :99-110
VHD bool in_frustum_approx(const VhDepthCameraParams& cp, const float* viewMatrixInverse, F3 pos)
{
    F3 pc = mat_mul_p(viewMatrixInverse, pos);
    float px = pc.x * cp.fx / pc.z + cp.mx;
    float py = pc.y * cp.fy / pc.z + cp.my;
    float wm1 = (float)cp.m_imageWidth - 1.0f, hm1 = (float)cp.m_imageHeight - 1.0f;
    float x = (2.0f * px - wm1) / wm1;
    float y = (hm1 - 2.0f * py) / hm1;
    float z = cam_to_proj_z(cp, pc.z);
    const float s = 0.95f;
    x *= s; y *= s; z *= s;
    return !(x < -1.0f || x > 1.0f || y < -1.0f || y > 1.0f || z < 0.0f || z > 1.0f);
}
// isSDFBlockInCameraFrustumApprox, DSC/VoxelUtilHashSDF.h:306-309
VHD bool block_in_frustum(const VhHashParams& hp, const VhDepthCameraParams& cp, I3 blk)
{
    F3 pw = block_to_world(hp.m_virtualVoxelSize, blk);
    float off = hp.m_virtualVoxelSize * 0.5f * ((float)VH_SDF_BLOCK_SIZE - 1.0f);
    pw.x += off; pw.y += off; pw.z += off;
    return in_frustum_approx(cp, hp.m_rigidTransformInverse, pw);
}

// The chunk of a block (worldToChunks of the block's world position, DSC/CUDASceneRepHashSDF.cu:133-146 and
// DSC/CUDASceneRepChunkGrid.cpp:126-153) and the index of its bit in the bit mask (linearizeChunkPos :124-130,
// .h:570-598), or 0xffffffff for a chunk outside the grid.  The one place that forms either: alloc's test
// (vh_kernels.hip) and the stream-out pass that keeps the device's copy of the mask (vh_streaming.hip) both go through it,
// as the host's isValidChunk does.
VHD uint32_t chunk_bit_of_block(const VhHashParams& hp, I3 blk)
{
    const F3 pw = block_to_world(hp.m_virtualVoxelSize, blk);
    const F3 p = mk3(pw.x / hp.m_streamingVoxelExtents[0], pw.y / hp.m_streamingVoxelExtents[1], pw.z / hp.m_streamingVoxelExtents[2]);
    const I3 c = mki3(round_half_away(p.x), round_half_away(p.y), round_half_away(p.z));
    const int qx = c.x - hp.m_streamingMinGridPos[0], qy = c.y - hp.m_streamingMinGridPos[1], qz = c.z - hp.m_streamingMinGridPos[2];
    if (qx < 0 || qy < 0 || qz < 0 || qx >= hp.m_streamingGridDimensions[0] || qy >= hp.m_streamingGridDimensions[1] || qz >= hp.m_streamingGridDimensions[2])
        return 0xffffffffu;
    return (uint32_t)(qz * hp.m_streamingGridDimensions[0] * hp.m_streamingGridDimensions[1] + qy * hp.m_streamingGridDimensions[0] + qx);
}

// isSDFBlockStreamedOut :149-156, fenced: the reference linearises the chunk without a bounds test
// and reads whatever word the index names -- another chunk's bit, or memory outside the mask.  The host can never set a
// bit for a chunk outside the grid (isValidChunk), so such a block is not streamed out, and nothing is read for it.
VHD bool block_streamed_out(const VhHashParams& hp, I3 blk, const uint32_t* bitMask)
{
    if (!bitMask) return false;
    const uint32_t index = chunk_bit_of_block(hp, blk);
    if (index == 0xffffffffu) return false;
    return (bitMask[index >> 5] & (1u << (index & 31))) != 0u;
}

// ---------------------------------------------------------------------------
// hash table access.  A VhHashEntry is 32 B: {pos.xyz, ptr} is one aligned
// 16-byte quad (a single dwordx4 load/store), offset is the dword behind it.
// ---------------------------------------------------------------------------

VHD int4 load_quad(const VhHashEntry* e) { return *reinterpret_cast<const int4*>(e); }
VHD void store_quad(VhHashEntry* e, int4 q) { *reinterpret_cast<int4*>(e) = q; }
VHD bool quad_matches(int4 q, I3 p) { return q.x == p.x && q.y == p.y && q.z == p.z && q.w != VH_FREE_ENTRY; }

// deleteHashEntry :365-369
VHD void delete_hash_entry(VhHashEntry* e)
{
    e->offset = 0;
    store_quad(e, make_int4(0, 0, 0, VH_FREE_ENTRY));
}
// HashEntry::operator= :64-73 (20-byte payload)
VHD void copy_entry(VhHashEntry* dst, const VhHashEntry* src)
{
    int4 q = load_quad(src);
    uint32_t o = src->offset;
    dst->offset = o;
    store_quad(dst, q);
}

// extension: per-bucket occupancy summary (count + 1 bit per bucket)
VHD void bucket_inc(const VhHashData& hd, uint32_t slotIdx)
{
    uint32_t b = slotIdx / VH_HASH_BUCKET_SIZE;
    uint32_t old = atomicAdd(&hd.d_bucketCount[b], 1u);
    if (old == 0u) atomicOr(&hd.d_bucketBits[b >> 5], 1u << (b & 31));
}
VHD void bucket_dec(const VhHashData& hd, uint32_t slotIdx)
{
    uint32_t b = slotIdx / VH_HASH_BUCKET_SIZE;
    uint32_t old = atomicSub(&hd.d_bucketCount[b], 1u);
    if (old == 1u) atomicAnd(&hd.d_bucketBits[b >> 5], ~(1u << (b & 31)));
}
VHD bool bucket_maybe_occupied(const VhHashData& hd, uint32_t h)
{
    return (hd.d_bucketBits[h >> 5] >> (h & 31)) & 1u;
}

// consumeHeap :519-523 (+ underflow guard the reference lacks: on an empty
// heap the counter is restored, the status word raised and block 0 returned
// is NOT handed out -- the caller must check `ok`)
VHD uint32_t consume_heap(const VhHashData& hd, uint32_t numSDFBlocks, bool& ok)
{
    uint32_t addr = atomicSub(&hd.d_heapCounter[0], 1u);
    if (addr >= numSDFBlocks) { // counter was already "-1": heap empty
        atomicAdd(&hd.d_heapCounter[0], 1u);
        atomicAdd(&hd.d_state[VH_STATE_HEAP_UNDERFLOW], 1u);
        ok = false;
        return 0;
    }
    ok = true;
    return hd.d_heap[addr];
}
// appendHeap :525-529
VHD void append_heap(const VhHashData& hd, uint32_t blockId)
{
    uint32_t addr = atomicAdd(&hd.d_heapCounter[0], 1u);
    hd.d_heap[addr + 1] = blockId;
}

// getHashEntryForSDFBlockPos :424-468, returning only what callers use:
// the ptr (VH_FREE_ENTRY on a miss).  The occupancy bit lets a miss in an
// empty bucket return without touching d_hash (an empty bucket has a free
// last slot with offset 0, so the list walk would stop at once).
VHD int lookup_ptr(const VhHashData& hd, const VhHashParams& hp, I3 blk)
{
    const uint32_t ne = hp.m_hashNumBuckets * VH_HASH_BUCKET_SIZE;
    const uint32_t h = hash_pos(hp.m_hashNumBuckets, blk);
    if (!bucket_maybe_occupied(hd, h)) return VH_FREE_ENTRY;
    const uint32_t base = h * VH_HASH_BUCKET_SIZE;
#pragma unroll 1
    for (uint32_t j = 0; j < VH_HASH_BUCKET_SIZE; j++) {
        int4 q = load_quad(&hd.d_hash[base + j]);
        if (quad_matches(q, blk)) return q.w;
    }
    const uint32_t idxLast = base + VH_HASH_BUCKET_SIZE - 1;
    uint32_t i = idxLast;
    uint32_t maxIter = 0;
#pragma unroll 1
    while (maxIter < hp.m_hashMaxCollisionLinkedListSize) {
        int4 q = load_quad(&hd.d_hash[i]);
        if (quad_matches(q, blk)) return q.w;
        if (q.w == VH_FREE_ENTRY && i != idxLast) {
            // A list never holds a free entry.  This one is a copy from before an alloc_block that runs beside this
            // kernel (CUDASceneRepHashSDF::integrateAhead) put a new head here: it stores the entry, fences, then
            // stores the link that led here, so the entry is in memory; drop this compute unit's stale lines and
            // read it again (what follows the new head is the list as it was).
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            q = load_quad(&hd.d_hash[i]);
            if (quad_matches(q, blk)) return q.w;
        }
        uint32_t off = hd.d_hash[i].offset;
        if (off == 0) break;
        i = (idxLast + off) % ne;
        maxIter++;
    }
    return VH_FREE_ENTRY;
}

// allocBlock :533-638.  Returns 0 = already there, 1 = allocated, 2 = lost a
// lock race (retry next pass), 3 = no room / heap empty.
VHD int alloc_block(const VhHashData& hd, const VhHashParams& hp, I3 pos, int32_t lockToken)
{
    const uint32_t ne = hp.m_hashNumBuckets * VH_HASH_BUCKET_SIZE;
    uint32_t h = hash_pos(hp.m_hashNumBuckets, pos);
    const uint32_t base = h * VH_HASH_BUCKET_SIZE;

    int firstEmpty = -1;
    const uint32_t idxLast = base + VH_HASH_BUCKET_SIZE - 1;
    const uint32_t maxLoop = hp.m_hashMaxCollisionLinkedListSize;
    uint32_t i = idxLast;
    uint32_t maxIter = 0;
    if (!bucket_maybe_occupied(hd, h)) {
        // empty bucket (no entry, hence no list hanging off its last slot): the first slot is the first free one.
        // A stale bit can only hide an entry written earlier in THIS pass, whose writer still holds the bucket
        // lock, so the lock attempt below fails exactly as it would after a full scan.
        firstEmpty = (int)base;
    } else {
        // the ten slots and the list head in flight together
        int4 qs[VH_HASH_BUCKET_SIZE];
#pragma unroll
        for (uint32_t j = 0; j < VH_HASH_BUCKET_SIZE; j++) qs[j] = load_quad(&hd.d_hash[base + j]);
        uint32_t off = hd.d_hash[idxLast].offset;
#pragma unroll
        for (uint32_t j = 0; j < VH_HASH_BUCKET_SIZE; j++) {
            if (quad_matches(qs[j], pos)) return 0;
            if (firstEmpty == -1 && qs[j].w == VH_FREE_ENTRY) firstEmpty = (int)(base + j);
        }
        // collision list (the reference's first hop re-reads the last slot: no match, see above)
#pragma unroll 1
        while (maxIter < maxLoop) {
            if (off == 0) break;
            i = (idxLast + off) % ne;
            maxIter++;
            if (!(maxIter < maxLoop)) break;
            int4 q = load_quad(&hd.d_hash[i]);
            if (quad_matches(q, pos)) return 0;
            off = hd.d_hash[i].offset;
        }
    }

    if (firstEmpty != -1) {
        int prev = atomicExch(&hd.d_hashBucketMutex[h], lockToken);
        if (prev != lockToken) {
            bool ok;
            uint32_t blk = consume_heap(hd, hp.m_numSDFBlocks, ok);
            if (!ok) return 3;
            VhHashEntry* e = &hd.d_hash[firstEmpty];
            e->offset = VH_NO_OFFSET;
            store_quad(e, make_int4(pos.x, pos.y, pos.z, (int)(blk * VH_SDF_BLOCK_VOXELS)));
            bucket_inc(hd, (uint32_t)firstEmpty);
            return 1;
        }
        atomicAdd(&hd.d_state[VH_STATE_ALLOC_LOCK_LOST], 1u);
        return 2;
    }

    int offset = 0;
    maxIter = 0;
#pragma unroll 1
    while (maxIter < maxLoop) {
        offset++;
        i = (idxLast + (uint32_t)offset) % ne;
        if ((offset % VH_HASH_BUCKET_SIZE) == 0) continue; // never a bucket's last slot
        int4 q = load_quad(&hd.d_hash[i]);
        if (q.w == VH_FREE_ENTRY) {
            int prev = atomicExch(&hd.d_hashBucketMutex[h], lockToken);
            if (prev != lockToken) {
                uint32_t lastOffset = hd.d_hash[idxLast].offset;
                uint32_t h2 = i / VH_HASH_BUCKET_SIZE;
                prev = atomicExch(&hd.d_hashBucketMutex[h2], lockToken);
                if (prev != lockToken) {
                    bool ok;
                    uint32_t blk = consume_heap(hd, hp.m_numSDFBlocks, ok);
                    if (!ok) return 3;
                    VhHashEntry* e = &hd.d_hash[i];
                    e->offset = lastOffset;
                    store_quad(e, make_int4(pos.x, pos.y, pos.z, (int)(blk * VH_SDF_BLOCK_VOXELS)));
                    // the new head is in memory before the link to it: a ray caster that runs beside this pass
                    // (integrateAhead) and follows the link finds the entry (lookup_ptr)
                    __threadfence();
                    hd.d_hash[idxLast].offset = (uint32_t)offset;
                    bucket_inc(hd, i);
                    return 1;
                }
            }
            atomicAdd(&hd.d_state[VH_STATE_ALLOC_LOCK_LOST], 1u);
            return 2;
        }
        maxIter++;
    }
    return 3;
}

// insertHashEntry :643-717.  In-bucket part as the reference (CAS on ptr).
// The reference's overflow branch (:682-713) is an unported HLSL remnant
// (3-int indexing) and undefined on this layout; defined behaviour here:
// take the home bucket, claim the first free non-last slot behind it by CAS
// and insert at the head of the home bucket's list.
VHD bool insert_hash_entry(const VhHashData& hd, const VhHashParams& hp, I3 pos, int ptr, int32_t lockToken)
{
    const uint32_t ne = hp.m_hashNumBuckets * VH_HASH_BUCKET_SIZE;
    const uint32_t h = hash_pos(hp.m_hashNumBuckets, pos);
    const uint32_t base = h * VH_HASH_BUCKET_SIZE;
#pragma unroll 1
    for (uint32_t j = 0; j < VH_HASH_BUCKET_SIZE; j++) {
        VhHashEntry* e = &hd.d_hash[base + j];
        int prev = atomicCAS(&e->ptr, VH_FREE_ENTRY, VH_LOCK_ENTRY);
        if (prev == VH_FREE_ENTRY) {
            // The offset is left alone: a free entry's is 0 (delete_hash_entry, reset), and the last slot's may
            // already be a link again -- a thread of this pass that found all ten slots claimed takes the list
            // branch below and may hang its element off the last slot before this thread has filled it in.  A
            // store of 0 here cut that element off: in the table, found by no walk from its home bucket.
            store_quad(e, make_int4(pos.x, pos.y, pos.z, ptr));
            bucket_inc(hd, base + j);
            return true;
        }
    }
    const uint32_t idxLast = base + VH_HASH_BUCKET_SIZE - 1;
    int prevLock = atomicExch(&hd.d_hashBucketMutex[h], lockToken);
    if (prevLock == lockToken) return false;
    uint32_t maxIter = 0;
    int offset = 0;
#pragma unroll 1
    while (maxIter < hp.m_hashMaxCollisionLinkedListSize) {
        offset++;
        uint32_t i = (idxLast + (uint32_t)offset) % ne;
        if ((offset % VH_HASH_BUCKET_SIZE) == 0) continue;
        VhHashEntry* e = &hd.d_hash[i];
        int prev = atomicCAS(&e->ptr, VH_FREE_ENTRY, VH_LOCK_ENTRY);
        if (prev == VH_FREE_ENTRY) {
            e->offset = hd.d_hash[idxLast].offset;
            store_quad(e, make_int4(pos.x, pos.y, pos.z, ptr));
            hd.d_hash[idxLast].offset = (uint32_t)offset;
            bucket_inc(hd, i);
            return true;
        }
        maxIter++;
    }
    return false;
}

// deleteHashEntryElement :723-809
VHD bool delete_hash_entry_element(const VhHashData& hd, const VhHashParams& hp, I3 blk, int32_t lockToken)
{
    const uint32_t ne = hp.m_hashNumBuckets * VH_HASH_BUCKET_SIZE;
    const uint32_t h = hash_pos(hp.m_hashNumBuckets, blk);
    const uint32_t base = h * VH_HASH_BUCKET_SIZE;

#pragma unroll 1
    for (uint32_t j = 0; j < VH_HASH_BUCKET_SIZE; j++) {
        const uint32_t i = base + j;
        int4 q = load_quad(&hd.d_hash[i]);
        if (quad_matches(q, blk)) {
            uint32_t off = hd.d_hash[i].offset;
            if (off != 0) {
                int prev = atomicExch(&hd.d_hashBucketMutex[h], lockToken);
                if (prev == lockToken) return false;
                append_heap(hd, (uint32_t)q.w / VH_SDF_BLOCK_VOXELS);
                uint32_t nextIdx = (i + off) % ne;
                copy_entry(&hd.d_hash[i], &hd.d_hash[nextIdx]);
                delete_hash_entry(&hd.d_hash[nextIdx]);
                bucket_dec(hd, nextIdx);
                return true;
            } else {
                append_heap(hd, (uint32_t)q.w / VH_SDF_BLOCK_VOXELS);
                delete_hash_entry(&hd.d_hash[i]);
                bucket_dec(hd, i);
                return true;
            }
        }
    }
    const uint32_t idxLast = base + VH_HASH_BUCKET_SIZE - 1;
    uint32_t prevIdx = idxLast;
    uint32_t i = (idxLast + hd.d_hash[idxLast].offset) % ne;
    uint32_t maxIter = 0;
#pragma unroll 1
    while (maxIter < hp.m_hashMaxCollisionLinkedListSize) {
        int4 q = load_quad(&hd.d_hash[i]);
        uint32_t off = hd.d_hash[i].offset;
        if (quad_matches(q, blk)) {
            int prev = atomicExch(&hd.d_hashBucketMutex[h], lockToken);
            if (prev == lockToken) return false;
            append_heap(hd, (uint32_t)q.w / VH_SDF_BLOCK_VOXELS);
            delete_hash_entry(&hd.d_hash[i]);
            bucket_dec(hd, i);
            hd.d_hash[prevIdx].offset = off;
            return true;
        }
        if (off == 0) return false;
        prevIdx = i;
        i = (idxLast + off) % ne;
        maxIter++;
    }
    return false;
}

// deleteHashEntryElement for a whole wave that frees ONE block (every lane calls it with the same block): ten lanes read
// the bucket's ten slots together instead of one lane reading them one after the other (up to ten dependent trips to
// memory at the end of a wave's life), and the lane that finds the block frees it with its two counter atomics in flight
// together.  An element of a collision list (a head with an offset, or a block that is not in its bucket) goes through
// the one-lane code.  Returns the same value in every lane.
VHD bool delete_hash_entry_element_wave(const VhHashData& hd, const VhHashParams& hp, I3 blk, int32_t lockToken, uint32_t lane)
{
    const uint32_t h = hash_pos(hp.m_hashNumBuckets, blk);
    const uint32_t i = h * VH_HASH_BUCKET_SIZE + lane;
    int4 q = make_int4(0, 0, 0, VH_FREE_ENTRY);
    uint32_t off = 0u;
    if (lane < VH_HASH_BUCKET_SIZE) { q = load_quad(&hd.d_hash[i]); off = hd.d_hash[i].offset; }
    const bool match = lane < VH_HASH_BUCKET_SIZE && quad_matches(q, blk);
    const unsigned long long m = __ballot(match);
    bool ok = false;
    if (m == 0ull || __ballot(match && off != 0u) != 0ull) {
        if (lane == 0u) ok = delete_hash_entry_element(hd, hp, blk, lockToken);
    } else if (match) { // (a block sits in at most one slot)
        const uint32_t addr = atomicAdd(&hd.d_heapCounter[0], 1u);          // append_heap
        const uint32_t old = atomicSub(&hd.d_bucketCount[h], 1u);           // bucket_dec
        hd.d_heap[addr + 1] = (uint32_t)q.w / VH_SDF_BLOCK_VOXELS;
        delete_hash_entry(&hd.d_hash[i]);
        if (old == 1u) atomicAnd(&hd.d_bucketBits[h >> 5], ~(1u << (h & 31)));
        ok = true;
    }
    return __ballot(ok) != 0ull;
}

// ---------------------------------------------------------------------------
// voxels.  A voxel is moved as one 64-bit word (DSC/VoxelUtilHashSDF.h:82-86):
// low dword = sdf bits, high dword = r | g<<8 | b<<16 | weight<<24.
// ---------------------------------------------------------------------------

struct Vox {
    float sdf;
    uint32_t cw; // colour + weight
    VHD uint32_t weight() const { return cw >> 24; }
    VHD uint32_t r() const { return cw & 0xffu; }
    VHD uint32_t g() const { return (cw >> 8) & 0xffu; }
    VHD uint32_t b() const { return (cw >> 16) & 0xffu; }
};
VHD Vox unpack_vox(uint2 w) { Vox v; v.sdf = __uint_as_float(w.x); v.cw = w.y; return v; }
VHD uint2 pack_vox(Vox v) { return make_uint2(__float_as_uint(v.sdf), v.cw); }
VHD uint32_t pack_cw(uint32_t r, uint32_t g, uint32_t b, uint32_t w) { return r | (g << 8) | (b << 16) | (w << 24); }

// The weighted colour average the reference left commented out (combineVoxel :241), per channel
//   uchar((c0 w0 + c1 w1) / (w0 + w1) + 0.5f)  =  floor((2 n + d) / (2 d)),  n = c0 w0 + c1 w1,  d = w0 + w1
// (the float32 formula and the integer one agree for every n <= 255 d, d in 1..510: tests/test_weighted_colour.py).
// cw0, cw1: the stored voxel's and the observation's colour + weight words; den = (float)(w0 + w1); y: a float within
// two ulp of 1 / den (the IEEE quotient, or the refined reciprocal the certified path holds for the sdf's division).
// Returns the three colour bytes with byte 3 clear.  A zero den gives bytes no caller keeps (and no trap).
//   * n by v_dot4_u32_u8 on {c0, c1, 0, 0} . {w0, w1, 0, 0}, accumulated onto the bit pattern of 2^23: the sum is the
//     float 2^23 + n as it stands (n <= 130 050), no conversion;
//   * t = 2 n + d by one fma (exact: an integer below 2^18);
//   * x = t / 2 d is a multiple of 1 / 2 d: an integer (the ties of n / d, which round up) or at least 1 / 2 d >= 2^-10
//     from one.  A product with a reciprocal that is an ulp low lands below the tie (thousands of pairs), so the
//     reciprocal is raised by 2^-21: with y's two ulp and the rounding of the constant's product the factor on x lies
//     in (1 + 0.37 * 2^-21, 1 + 1.63 * 2^-21) -- above the integer on a tie, and x < 256 moves by less than 2^-12
//     otherwise;
//   * floor(x) by the second fma: + (2^23 - 1/2) rounds x - 1/2 to the nearest integer, which is floor(x) for an x just
//     above an integer or that far below the next (x > 1/2, so the sum is at least 2^23, where floats are the
//     integers), and leaves it in the low mantissa bits: the low byte of the float is the colour byte.
// vh_debug_check_weighted_colour runs every (c0, w0, c1, w1) through it, with either reciprocal.
VHD uint32_t weighted_colour(uint32_t cw0, uint32_t cw1, float den, float y)
{
    const uint32_t ww = __builtin_amdgcn_perm(cw1, cw0, 0x0c0c0703u); // w0 | w1 << 8
    const float dOff = den - 0x1p24f;                                 // (exact)
    const float yh = y * (0.5f + 0x1p-22f);
    uint32_t byte[3];
#pragma unroll
    for (uint32_t ch = 0; ch < 3; ch++) {
        const uint32_t cc = __builtin_amdgcn_perm(cw1, cw0, 0x0c0c0400u + ch * 0x0101u);      // c0 | c1 << 8 of the channel
        const float nf = __uint_as_float(__builtin_amdgcn_udot4(cc, ww, 0x4b000000u, false)); // 2^23 + n
        const float t = __fmaf_rn(nf, 2.0f, dOff);                                            // 2 n + d
        byte[ch] = __float_as_uint(__fmaf_rn(t, yh, 0x1p23f - 0.5f));
    }
    return __builtin_amdgcn_perm(byte[2], __builtin_amdgcn_perm(byte[1], byte[0], 0x0c0c0400u), 0x0c040100u);
}

// combineVoxel :229-250
VHD Vox combine_voxel(const VhHashParams& hp, Vox v0, Vox v1)
{
    Vox out;
    // colour :236-240: uchar(0.5f * c0 + 0.5f * c1 + 0.5f) per channel.  For bytes c0, c1 every term and sum is exact in
    // fp32 (half-integers up to 255.5), so the value is floor((c0 + c1) / 2 + 1/2) = (c0 + c1 + 1) >> 1, the byte-wise
    // average rounded up: (a | b) - (((a ^ b) >> 1) & 0x7f7f7f7f) on the packed word, all channels at once
    // (tests/test_oracle_math.py checks the identity for all 65 536 pairs against the float formula).
    const uint32_t a = v0.cw & 0x00ffffffu, c = v1.cw & 0x00ffffffu;
    uint32_t rgb = (a | c) - (((a ^ c) >> 1) & 0x7f7f7f7fu);
    float w0 = (float)v0.weight(), w1 = (float)v1.weight();
    // (m_colorIntegration is the same for every voxel of a launch: a scalar branch)
    if (hp.m_colorIntegration != VH_COLOR_RUNNING_AVERAGE) rgb = weighted_colour(v0.cw, v1.cw, w0 + w1, 1.0f / (w0 + w1));
    out.sdf = (v0.sdf * w0 + v1.sdf * w1) / (w0 + w1);
    uint32_t w = min(hp.m_integrationWeightMax, v0.weight() + v1.weight());
    out.cw = rgb | ((w & 0xffu) << 24);
    return out;
}

// ---------------------------------------------------------------------------
// what more than one translation unit of kernels needs
// ---------------------------------------------------------------------------

constexpr int kWave = 64;
VHD uint32_t lane_id() { return threadIdx.x & (kWave - 1); }
VHD uint64_t lanemask_lt() { return (1ull << lane_id()) - 1ull; }

// Minimum / maximum over the 64 lanes of a wave, in a scalar register.  For a caller that runs with ALL 64 lanes enabled
// (a lane without data holds the identity): a disabled lane's register would be read as it stands.  The steps are DPP
// operands inside the vector unit -- row_shr 1, 2, 4, 8 gather each row of 16 into its lane 15, row_bcast:15 into rows 1
// and 3 and row_bcast:31 into rows 2 and 3 carry the rows' results on to lane 63, which is read -- one instruction per
// step where __shfl_xor takes four for the lane address, a trip through LDS and a wait.  A lane the step has no source
// for (the first lanes of a row, the rows the mask leaves out) is not written and keeps its value.  Written as
// instructions: from __builtin_amdgcn_update_dpp the compiler makes a copy, a v_mov_b32_dpp and a canonicalising
// v_max_f32 beside each min or max (four instructions a step).  It does not see into the text, so each step brings the
// two wait states a DPP operand needs behind the vector instruction that wrote it.  For min and max over values
// without NaN the order in which lanes meet changes nothing.
#define VH_WAVE_REDUCE(OP, CONSTRAINT)                                                                        \
    {                                                                                                         \
        asm("s_nop 1\n\t" OP " %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf" : CONSTRAINT(v));             \
        asm("s_nop 1\n\t" OP " %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf" : CONSTRAINT(v));             \
        asm("s_nop 1\n\t" OP " %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf" : CONSTRAINT(v));             \
        asm("s_nop 1\n\t" OP " %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf" : CONSTRAINT(v));             \
        asm("s_nop 1\n\t" OP " %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf" : CONSTRAINT(v));          \
        asm("s_nop 1\n\t" OP " %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf" : CONSTRAINT(v));          \
    }
VHD float wave_min_f32(float v)
{
    VH_WAVE_REDUCE("v_min_f32_dpp", "+v")
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), kWave - 1));
}
VHD float wave_max_f32(float v)
{
    VH_WAVE_REDUCE("v_max_f32_dpp", "+v")
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), kWave - 1));
}
VHD uint32_t wave_max_u32(uint32_t v)
{
    VH_WAVE_REDUCE("v_max_u32_dpp", "+v")
    return (uint32_t)__builtin_amdgcn_readlane((int)v, kWave - 1);
}
#undef VH_WAVE_REDUCE

// workgroups of b that cover a (host side: the launchers' grid sizes)
inline uint32_t cdiv(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }
// the 8x8-pixel tiles of an image: a wave each in alloc, the interval splat's heads and lists, the tile ray caster
inline uint32_t image_tiles(uint32_t width, uint32_t height) { return cdiv(width, 8) * cdiv(height, 8); }

VHD float4 f4_scale(float a, float4 v) { return make_float4(a * v.x, a * v.y, a * v.z, a * v.w); }
VHD float4 f4_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
VHD float4 f4_div(float4 a, float b) { return make_float4(a.x / b, a.y / b, a.z / b, a.w / b); }

// bilinearInterpolationFloat4, DSC/CameraUtil.cu:1136-1166 (and ICPUtil.h:129-156).  fetch(i, k): the pixel at index i,
// which is tap k of (px, py), (px + 1, py), (px, py + 1), (px + 1, py + 1); it is asked for taps inside the image only.
template <class Fetch>
VHD float4 bilinear_float4_taps(float x, float y, Fetch fetch, uint32_t W, uint32_t H)
{
    const int px = (int)floorf(x), py = (int)floorf(y);
    const float alpha = x - (float)px, beta = y - (float)py;
    const float mi = minf();
    float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
    float w0 = 0.0f, w1 = 0.0f;
    auto tap = [&](uint32_t k, int tx, int ty, float wgt, float4& s, float& w) {
        if ((uint32_t)tx < W && (uint32_t)ty < H) {
            const float4 v = fetch((uint32_t)ty * W + (uint32_t)tx, k);
            if (v.x != mi && v.y != mi && v.z != mi) { s = f4_add(s, f4_scale(wgt, v)); w += wgt; }
        }
    };
    tap(0u, px, py, 1.0f - alpha, s0, w0);
    tap(1u, px + 1, py, alpha, s0, w0);
    tap(2u, px, py + 1, 1.0f - alpha, s1, w1);
    tap(3u, px + 1, py + 1, alpha, s1, w1);
    const float4 p0 = f4_div(s0, w0), p1 = f4_div(s1, w1);
    float4 ss = make_float4(0.f, 0.f, 0.f, 0.f);
    float ww = 0.0f;
    if (w0 > 0.0f) { ss = f4_add(ss, f4_scale(1.0f - beta, p0)); ww += (1.0f - beta); }
    if (w1 > 0.0f) { ss = f4_add(ss, f4_scale(beta, p1)); ww += beta; }
    return ww > 0.0f ? f4_div(ss, ww) : make_float4(mi, mi, mi, mi);
}
VHD float4 bilinear_float4(float x, float y, const float4* in, uint32_t W, uint32_t H)
{
    return bilinear_float4_taps(x, y, [in](uint32_t i, uint32_t) { return in[i]; }, W, H);
}

} // namespace vhd
