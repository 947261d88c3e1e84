// vh_kernels.hip -- the frame loop's kernels: reset, alloc, compactify, integrate, garbage collection, the interval
// splat, the ray caster, the queries and normals, with their launcher-level C ABI (include/vh_api.h).  They are one
// translation unit because they ride on one another: k_render carries alloc, and k_compute_normals carries compactify,
// the splat and integrate, so those device functions must be visible together.  They are written a stage to a header
// (vh_frame_*.hpp, included in their order of definition; a header's includes say on whom its stage rides) but for the
// ray caster -- the march, the queries and the tile ray caster, which carries alloc -- which stands here, between the
// includes, until it is moved in a change of its own.  The checks of integrate's arithmetic (k_check_refined_division,
// k_check_weighted_colour) stay with the functions they check, and k_debug_hash_ops with the kernels whose hash
// operations it runs one by one.  What shares only vh_device.hpp with the frame loop has a unit of its own:
// vh_image.hip, vh_streaming.hip, vh_mc.hip, vh_util.hip.
// A stage's launch shape is a host function beside its kernel; the launchers, whether they launch the stage alone or as
// a rider, call it.
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

namespace {

// ---------------------------------------------------------------------------
// ray caster (renderKernel DSC/CUDARayCastSDF.cu:18-57,
// traverseCoarseGridSimpleSampleAll DSC/RayCastSDFUtil.h:198-262)
//
// One wave per 8x8 pixel tile (the rays of a tile stay in the same few blocks).  The reference's march is a chain
// of dependent gathers (8 hash probes x up to 11 entry loads + 8 voxel loads per sample, one after the other); here
// the work is re-ordered without changing an arithmetic operation, its order, or an early-out:
//   * k_render (with the tile heads / block lists of k_interval_splat): block -> pointer through a per-wave table in
//     LDS, the march confined to the tile's depth interval, one probe and one round of LDS reads per sample;
//   * k_render_hash (no intervals: the reference fork's behaviour): block -> pointer through the hash table behind
//     a 2-entry per-ray cache, empty space skipped on the bucket occupancy bit;
//   * both: division-free tap coordinates where they can be certified, the eight voxels of a sample in flight
//     together as 8-byte loads, march-until-sign-change / bisect / resume so that the lanes of a wave bisect together.
// ---------------------------------------------------------------------------

struct BlockCache {
    int bx0, by0, bz0, p0;
    int bx1, by1, bz1, p1;
    bool v0, v1;
};

VHD void cache_init(BlockCache& bc)
{
    bc.v0 = bc.v1 = false;
    bc.bx0 = bc.by0 = bc.bz0 = bc.bx1 = bc.by1 = bc.bz1 = 0;
    bc.p0 = bc.p1 = VH_FREE_ENTRY;
}

// getHashEntryForSDFBlockPos (DSC/VoxelUtilHashSDF.h:424-468) behind a 2-entry per-ray cache.  A miss loads the
// bucket's occupancy word and its first slot together (one round trip): a block sits in slot 0 unless two blocks
// share the bucket, and an empty bucket proves absence; only the remaining cases walk the bucket.
VHD int cached_lookup(const VhHashData& hd, const VhHashParams& hp, HashMod hm, BlockCache& bc, int bx, int by, int bz)
{
    if (bc.v0 && bc.bx0 == bx && bc.by0 == by && bc.bz0 == bz) return bc.p0;
    if (bc.v1 && bc.bx1 == bx && bc.by1 == by && bc.bz1 == bz) return bc.p1;
    const uint32_t h = hash_pos_fast(hm, mki3(bx, by, bz));
    const uint32_t word = hd.d_bucketBits[h >> 5];
    const int4 q = load_quad(&hd.d_hash[h * VH_HASH_BUCKET_SIZE]);
    int p;
    if (quad_matches(q, mki3(bx, by, bz))) p = q.w;
    else if (!((word >> (h & 31)) & 1u)) p = VH_FREE_ENTRY;
    else p = lookup_ptr(hd, hp, mki3(bx, by, bz));
    bc.bx1 = bc.bx0; bc.by1 = bc.by0; bc.bz1 = bc.bz0; bc.p1 = bc.p0; bc.v1 = bc.v0;
    bc.bx0 = bx; bc.by0 = by; bc.bz0 = bz; bc.p0 = p; bc.v0 = true;
    return p;
}

constexpr int kPtrUnknown = -3; // "first tap not resolved yet" (never a block pointer, VH_FREE_ENTRY or VH_LOCK_ENTRY)

// block -> voxel pointer through the hash table in HBM
struct HashLookup {
    const VhHashData& hd;
    const VhHashParams& hp;
    HashMod hm;
    BlockCache bc;
    static constexpr bool kOffsets32 = false; // (load_voxel)
    static constexpr bool kGeneral = true;    // a miss may end in the hash table (march_ray, split tiles)
    VHD int find(int bx, int by, int bz) { return cached_lookup(hd, hp, hm, bc, bx, by, bz); }
    // may the sample whose first tap lies in this block be valid?  (occupancy bit of the bucket: one cached dword)
    VHD bool first_tap(int bx, int by, int bz, int& handle)
    {
        handle = kPtrUnknown;
        return bucket_maybe_occupied(hd, hash_pos_fast(hm, mki3(bx, by, bz)));
    }
    // voxel pointers of the eight taps (p[j]: bit0 = x1, bit1 = y1, bit2 = z1), one probe per DISTINCT block;
    // false if one of the blocks does not exist.  bit a of `straddle`: the tap pair along axis a lies in two blocks.
    VHD bool resolve(int, int bxa, int bya, int bza, int bxb, int byb, int bzb, uint32_t straddle, int (&p)[8])
    {
        const int p0 = find(bxa, bya, bza);
        if (p0 == VH_FREE_ENTRY) return false; // the first tap reads the zero voxel (weight 0)
#pragma unroll
        for (int j = 0; j < 8; j++) p[j] = p0;
        if (straddle) {
            uint32_t need = 0xfeu; // combos whose block differs from combo 0 still need a pointer
#pragma unroll
            for (uint32_t j = 1; j < 8u; j++)
                if ((j & straddle) == 0u) need &= ~(1u << j);
#pragma unroll 1
            while (need) {
                const uint32_t k = (uint32_t)__ffs((int)need) - 1u;
                const int pk = find((k & 1u) ? bxb : bxa, (k & 2u) ? byb : bya, (k & 4u) ? bzb : bza);
                if (pk == VH_FREE_ENTRY) return false;
                const uint32_t km = k & straddle;
                uint32_t same = 0u;
#pragma unroll
                for (uint32_t j = 1; j < 8u; j++) {
                    const bool eq = (j & straddle) == km;
                    p[j] = eq ? pk : p[j];
                    same |= (eq ? 1u : 0u) << j;
                }
                need &= ~same;
            }
        }
        return true;
    }
};

// block -> voxel pointers through the tile's own table in LDS, built from the tile's block list (open addressing).
// A slot is kTileSlotWords words: {x, y, z, p000, p100, p010, p110, p001, p101, p011, p111, -}: the block, its voxel
// pointer and the pointers of its seven +x/+y/+z neighbours (VH_FREE_ENTRY where there is none), so that a sample
// resolves its eight taps with one probe and one round of LDS reads, however many blocks they straddle.
// k_interval_splat lists every block the tile's rays can read, so a block that is not in a COMPLETE table is not
// allocated; when the list overflowed, the table holds a part of it and a miss falls back to the hash table.
constexpr uint32_t kTileSlotWords = 12;

//
// Two lookups share the table.  TileLookupComplete serves a tile whose list took every block (all of them at 4 cm
// voxels): LDS only, nothing of the hash table is named in it, so the march instantiated on it keeps neither the table's
// pointers nor the bucket modulus nor the second block of a tap pair in registers.  TileLookup is the general one, for
// the tile whose list overflowed.  render_tile picks one per wave.
// OFFSETS32: voxel loads take a 32-bit byte offset on the pool's base (load_voxel).
// ONE_READ: a probe's four words are asked for together (slot_find).  For the kernels without gradients, where it was
// measured; with it k_render_large<true, *> takes 177 registers for 161 and loses a wave per SIMD.
template <uint32_t kTileTabSlots, bool OFFSETS32, bool ONE_READ> // 2 x the list capacity (load factor <= 1/2), a power of two
struct TileLookup {
    const int* tab;
    bool complete;
    const VhHashData& hd;
    const VhHashParams& hp;
    static constexpr bool kOffsets32 = OFFSETS32;
    static constexpr bool kGeneral = true;
    VHD static uint32_t slot_of(int bx, int by, int bz)
    {
        // Multiply-shift hash.  The blocks of a tile are a dense slab along its beam;
        // a linear form like x + 5y + 24z packs such a slab into ONE contiguous run of slots, and a probe for a block
        // that is not in the table (every empty-space step of a ray) then walks the whole run: 100 probes instead
        // of one on the long lists of fine voxels.
        // (The compiler makes three v_mul_lo_u32 of it, a quarter-rate instruction: only bits below 24 of the sum are used,
        // so it drops the 24-bit form and then cannot show that the operands have 24 bits.  v_mul_u32_u24 / v_mad_u32_u24
        // written as instructions are fewer issue cycles and were slower on the device: profiles/README.md.)
        return ((__umul24((uint32_t)bx, 0x9E3779u) + __umul24((uint32_t)by, 0x7F4A7Du) + __umul24((uint32_t)bz, 0x85EBCBu)) >> 10) & (kTileTabSlots - 1u);
    }
    VHD static int slot_find(const int* tab, int bx, int by, int bz)
    {
        uint32_t h = slot_of(bx, by, bz);
        for (;;) {
            int4 e = *reinterpret_cast<const int4*>(&tab[h * kTileSlotWords]);
            // one 16-byte LDS read, said so: left alone the compiler asks for e.w, waits, tests it and only then asks for
            // the other three words -- two trips in a row for every probe that finds its block
            if (ONE_READ) asm volatile("" : "+v"(e.x), "+v"(e.y), "+v"(e.z), "+v"(e.w));
            if (e.w == VH_FREE_ENTRY) return -1;
            if ((int)(e.x == bx) & (int)(e.y == by) & (int)(e.z == bz)) return (int)h;
            h = (h + 1u) & (kTileTabSlots - 1u);
        }
    }
    VHD int find_any(int bx, int by, int bz) const
    {
        const int sl = slot_find(tab, bx, by, bz);
        if (sl >= 0) return tab[(uint32_t)sl * kTileSlotWords + 3u];
        return complete ? VH_FREE_ENTRY : lookup_ptr(hd, hp, mki3(bx, by, bz));
    }
    // handle: the slot of the block (>= 0), or kPtrUnknown
    VHD bool first_tap(int bx, int by, int bz, int& handle) const
    {
        handle = slot_find(tab, bx, by, bz);
        if (handle >= 0) return true;
        handle = kPtrUnknown;
        return complete ? false : lookup_ptr(hd, hp, mki3(bx, by, bz)) != VH_FREE_ENTRY;
    }
    VHD bool resolve(int handle, int bxa, int bya, int bza, int bxb, int byb, int bzb, uint32_t straddle, int (&p)[8]) const
    {
        if (complete) {
            const int sl = handle >= 0 ? handle : slot_find(tab, bxa, bya, bza);
            if (sl < 0) return false; // the first tap reads the zero voxel (weight 0)
            // the tap pair of an axis lies in one block or in two adjacent ones: combo j reads neighbour (j & straddle)
            const int* e = &tab[(uint32_t)sl * kTileSlotWords + 3u];
            int all = 0;
#pragma unroll
            for (uint32_t j = 0; j < 8u; j++) {
                p[j] = e[j & straddle];
                all |= p[j];
            }
            return all >= 0; // voxel pointers are >= 0, VH_FREE_ENTRY is not
        }
#pragma unroll
        for (uint32_t k = 0; k < 8u; k++) p[k] = 0;
#pragma unroll 1
        for (uint32_t j = 0; j < 8u; j++) {
            const int pj = find_any((j & 1u) ? bxb : bxa, (j & 2u) ? byb : bya, (j & 4u) ? bzb : bza);
            if (pj == VH_FREE_ENTRY) return false;
#pragma unroll
            for (uint32_t k = 0; k < 8u; k++) p[k] = (k == j) ? pj : p[k];
        }
        return true;
    }
};

template <uint32_t kTileTabSlots, bool OFFSETS32, bool ONE_READ>
struct TileLookupComplete {
    const int* tab;
    static constexpr bool kOffsets32 = OFFSETS32;
    static constexpr bool kGeneral = false;
    // handle: the slot of the block (>= 0), or kPtrUnknown
    VHD bool first_tap(int bx, int by, int bz, int& handle) const
    {
        handle = TileLookup<kTileTabSlots, OFFSETS32, ONE_READ>::slot_find(tab, bx, by, bz);
        if (handle >= 0) return true;
        handle = kPtrUnknown;
        return false;
    }
    // (only the first tap's block and `straddle` are read: the second block's coordinates die where straddle is formed)
    VHD bool resolve(int handle, int bxa, int bya, int bza, int, int, int, uint32_t straddle, int (&p)[8]) const
    {
        const int sl = handle >= 0 ? handle : TileLookup<kTileTabSlots, OFFSETS32, ONE_READ>::slot_find(tab, bxa, bya, bza);
        if (sl < 0) return false; // the first tap reads the zero voxel (weight 0)
        // the tap pair of an axis lies in one block or in two adjacent ones: combo j reads neighbour (j & straddle)
        const int* e = &tab[(uint32_t)sl * kTileSlotWords + 3u];
        int all = 0;
#pragma unroll
        for (uint32_t j = 0; j < 8u; j++) {
            p[j] = e[j & straddle];
            all |= p[j];
        }
        return all >= 0; // voxel pointers are >= 0, VH_FREE_ENTRY is not
    }
};

// One 8-byte load per voxel.  As an (indivisible) relaxed atomic: an ordinary load is split by the compiler into its
// two words, and the sdf word is then fetched only after the weight test -- a second trip to memory per sample.
//
// OFFSETS32: the pool is at most 2^32 bytes (offsets32_ok), so the voxel's byte offset fits an unsigned 32-bit register
// and the load takes it beside the pool's base in scalar registers: one address register per tap instead of a 64-bit
// pair, and no 64-bit add.  The arithmetic is unsigned 32-bit on purpose (offsets with the top bit set are ordinary).
template <bool OFFSETS32 = false>
VHD uint2 load_voxel(const VhHashData& hd, int ptr, int lx, int ly, int lz)
{
    const unsigned long long* at;
    if constexpr (OFFSETS32) {
        const uint32_t off = ((uint32_t)ptr + (uint32_t)(lz * 64 + ly * 8 + lx)) * (uint32_t)sizeof(VhVoxel);
        at = reinterpret_cast<const unsigned long long*>(reinterpret_cast<const char*>(hd.d_SDFBlocks) + off);
    } else {
        at = reinterpret_cast<const unsigned long long*>(&hd.d_SDFBlocks[(uint32_t)ptr + (uint32_t)(lz * 64 + ly * 8 + lx)]);
    }
    const unsigned long long v = __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    return make_uint2((uint32_t)v, (uint32_t)(v >> 32));
}
static_assert(sizeof(VhVoxel) == 8, "load_voxel");
// may the ray caster address this pool's voxels with 32-bit byte offsets?
static bool offsets32_ok(uint32_t numSDFBlocks)
{
    return (uint64_t)numSDFBlocks * (VH_SDF_BLOCK_SIZE * VH_SDF_BLOCK_SIZE * VH_SDF_BLOCK_SIZE) * sizeof(VhVoxel) <= (1ull << 32);
}

struct Taps {
    int x0, y0, z0, x1, y1, z1;       // voxel coordinates of the lower / upper tap per axis
    int bxa, bya, bza, bxb, byb, bzb; // their SDF blocks (virtualVoxelPosToSDFBlock)
};

// The eight tap weights of trilinearInterpolationSimpleFastFast at `pos`, in the reference's tap order
// (000,100,010,001,110,011,101,111) and with its arithmetic: (wx' * wy') * wz' per tap, w = frac(pos / voxel), 1 - w.
// PACKED: x and y as f32x2 pairs, for the kernels that address voxels by 32-bit offsets (LK::kOffsets32).  With 64-bit
// addresses the packed form is ten instructions shorter per sample as well, adds no move -- and k_render<false, false> ran
// 2 % slower with it (the cfg3 frame 0.9 % below the scalar form's, profiles/README.md), so those kernels keep the scalar one.
template <bool PACKED>
VHD void tap_weights(F3 pos, float vs, float rvs, float (&s)[8])
{
    if constexpr (!PACKED) {
        const float fx = div_exact(pos.x, vs, rvs), fy = div_exact(pos.y, vs, rvs), fz = div_exact(pos.z, vs, rvs);
        const float wx = fx - floorf(fx), wy = fy - floorf(fy), wz = fz - floorf(fz);
        const float ux = 1.0f - wx, uy = 1.0f - wy, uz = 1.0f - wz;
        s[0] = (ux * uy) * uz; s[1] = (wx * uy) * uz; s[2] = (ux * wy) * uz; s[3] = (ux * uy) * wz;
        s[4] = (wx * wy) * uz; s[5] = (ux * wy) * wz; s[6] = (wx * uy) * wz; s[7] = (wx * wy) * wz;
        return;
    }
    // Packed where two operations find their operands side by side without a move (the unit is compiled without the SLP
    // vectorizer; what it packed here cost a v_mov or v_pk_mov per pair and a wait state before the next packed
    // instruction): the x and y divisions as one chain, then {ux, wx} -- which the two scalar subtractions write next to
    // each other -- times uy and times wy, and those two pairs times uz and times wz.  Each component is the scalar
    // instruction's result.  The eight products with the distances and their sum stay scalar in trilinear / taps_finish:
    // a voxel load returns {sdf, colour and weight}, so no two distances are neighbours, and the sum's order is the reference's.
    const f32x2 fxy = div_exact2((f32x2){ pos.x, pos.y }, vs, rvs);
    const float fz = div_exact(pos.z, vs, rvs);
    const float wx = fxy.x - floorf(fxy.x), wy = fxy.y - floorf(fxy.y), wz = fz - floorf(fz);
    const float uy = 1.0f - wy, uz = 1.0f - wz;
    const f32x2 xs = (f32x2){ 1.0f - wx, wx };
    const f32x2 xu = xs * both(uy), xw = xs * both(wy); // {ux uy, wx uy}, {ux wy, wx wy}
    const f32x2 a = xu * both(uz), b = xw * both(uz), c = xu * both(wz), d = xw * both(wz);
    s[0] = a.x; s[1] = a.y; s[2] = b.x; s[3] = c.x; s[4] = b.y; s[5] = d.x; s[6] = c.y; s[7] = d.y;
}

// The point cam + t dir of a ray, with the reference's arithmetic (a product and a sum per axis).  (x and y as one packed
// product and one packed sum were measured: 9 % off the cfg2 frame on top of the packed weights -- profiles/README.md.)
VHD F3 ray_point(F3 cam, F3 dir, float t)
{
    return mk3(cam.x + t * dir.x, cam.y + t * dir.y, cam.z + t * dir.z);
}

// trilinearInterpolationSimpleFastFast, DSC/RayCastSDFUtil.h:97-116, for tap
// voxel coordinates (x0..z1) the caller has already resolved.
// Returns false exactly when the reference does (some tap, in tap order, has
// weight 0 -- a missing block yields the zero voxel); `dist` is then undefined
// (the reference leaves a partial sum that only gradientForPoint can observe:
// see trilinear_partial below).  The colour is accumulated only on request:
// the reference computes it for every sample but reads it only from the last
// bisection sample (RayCastSDFUtil.h:231,241).
template <bool COLOR, class LK>
VHD bool trilinear(const VhHashData& hd, float vs, LK& lk, int p0in, const Taps& tp,
                   F3 pos, float rvs, float& dist, uint32_t& colorOut)
{
    const int x0 = tp.x0, y0 = tp.y0, z0 = tp.z0, x1 = tp.x1, y1 = tp.y1, z1 = tp.z1;
    const int bxa = tp.bxa, bya = tp.bya, bza = tp.bza, bxb = tp.bxb, byb = tp.byb, bzb = tp.bzb;
    // bit a of `straddle`: the tap pair along axis a lies in two different blocks
    const uint32_t straddle = (bxb != bxa ? 1u : 0u) | (byb != bya ? 2u : 0u) | (bzb != bza ? 4u : 0u);

    // voxel pointer per tap combo (bit0 = x1, bit1 = y1, bit2 = z1)
    int p[8];
    if (!lk.resolve(p0in, bxa, bya, bza, bxb, byb, bzb, straddle, p)) return false;
    const int p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3], p4 = p[4], p5 = p[5], p6 = p[6], p7 = p[7];

    const int lx0 = x0 & 7, ly0 = y0 & 7, lz0 = z0 & 7; // = local1(): two's complement & 7 is the non-negative remainder
    const int lx1 = x1 & 7, ly1 = y1 & 7, lz1 = z1 & 7;
    // the eight voxels, in flight together (reference tap order 000,100,010,001,110,011,101,111)
    constexpr bool O32 = LK::kOffsets32;
    uint2 r000 = load_voxel<O32>(hd, p0, lx0, ly0, lz0), r100 = load_voxel<O32>(hd, p1, lx1, ly0, lz0);
    uint2 r010 = load_voxel<O32>(hd, p2, lx0, ly1, lz0), r001 = load_voxel<O32>(hd, p4, lx0, ly0, lz1);
    uint2 r110 = load_voxel<O32>(hd, p3, lx1, ly1, lz0), r011 = load_voxel<O32>(hd, p6, lx0, ly1, lz1);
    uint2 r101 = load_voxel<O32>(hd, p5, lx1, ly0, lz1), r111 = load_voxel<O32>(hd, p7, lx1, ly1, lz1);
    // one trip to memory for the eight: left alone the compiler waits for the first pair before it issues the rest
    // (three trips), and the dearest waves of a frame run at the pace of their own chain of loads
    asm volatile("" : "+v"(r000.x), "+v"(r000.y), "+v"(r100.x), "+v"(r100.y), "+v"(r010.x), "+v"(r010.y), "+v"(r001.x), "+v"(r001.y),
                      "+v"(r110.x), "+v"(r110.y), "+v"(r011.x), "+v"(r011.y), "+v"(r101.x), "+v"(r101.y), "+v"(r111.x), "+v"(r111.y));
    const Vox v000 = unpack_vox(r000), v100 = unpack_vox(r100), v010 = unpack_vox(r010), v001 = unpack_vox(r001);
    const Vox v110 = unpack_vox(r110), v011 = unpack_vox(r011), v101 = unpack_vox(r101), v111 = unpack_vox(r111);
    // weight byte == 0 for any tap <=> min over the taps of (cw >> 24) == 0
    const uint32_t wmin = min(min(min(v000.cw, v100.cw), min(v010.cw, v001.cw)), min(min(v110.cw, v011.cw), min(v101.cw, v111.cw)));
    if ((wmin >> 24) == 0u) return false;

    float s[8];
    tap_weights<LK::kOffsets32>(pos, vs, rvs, s);
    float d = 0.0f, cr = 0.0f, cg = 0.0f, cb = 0.0f;
#define VH_ACC(V, S)                                                    \
    {                                                                   \
        d += (S) * (V).sdf;                                             \
        if (COLOR) { cr += (S) * (float)(V).r(); cg += (S) * (float)(V).g(); cb += (S) * (float)(V).b(); } \
    }
    VH_ACC(v000, s[0])
    VH_ACC(v100, s[1])
    VH_ACC(v010, s[2])
    VH_ACC(v001, s[3])
    VH_ACC(v110, s[4])
    VH_ACC(v011, s[5])
    VH_ACC(v101, s[6])
    VH_ACC(v111, s[7])
#undef VH_ACC
    dist = d;
    if (COLOR) colorOut = (uint32_t)f2uc(cr) | ((uint32_t)f2uc(cg) << 8) | ((uint32_t)f2uc(cb) << 16);
    return true;
}

// trilinear<false> in two steps, for a march that asks for the NEXT sample's voxels before it blends this one's
// (march_ray, PIPELINED): taps_issue resolves the eight pointers and puts the eight loads in flight (false: a block is
// missing, the sample is invalid and nothing was asked for), taps_finish is the weight test and the blend.
struct TapLoads {
    uint2 r000, r100, r010, r001, r110, r011, r101, r111;
};
template <class LK>
VHD bool taps_issue(const VhHashData& hd, LK& lk, int p0in, const Taps& tp, TapLoads& L)
{
    const uint32_t straddle = (tp.bxb != tp.bxa ? 1u : 0u) | (tp.byb != tp.bya ? 2u : 0u) | (tp.bzb != tp.bza ? 4u : 0u);
    int p[8];
    if (!lk.resolve(p0in, tp.bxa, tp.bya, tp.bza, tp.bxb, tp.byb, tp.bzb, straddle, p)) return false;
    const int lx0 = tp.x0 & 7, ly0 = tp.y0 & 7, lz0 = tp.z0 & 7;
    const int lx1 = tp.x1 & 7, ly1 = tp.y1 & 7, lz1 = tp.z1 & 7;
    constexpr bool O32 = LK::kOffsets32;
    L.r000 = load_voxel<O32>(hd, p[0], lx0, ly0, lz0); L.r100 = load_voxel<O32>(hd, p[1], lx1, ly0, lz0);
    L.r010 = load_voxel<O32>(hd, p[2], lx0, ly1, lz0); L.r001 = load_voxel<O32>(hd, p[4], lx0, ly0, lz1);
    L.r110 = load_voxel<O32>(hd, p[3], lx1, ly1, lz0); L.r011 = load_voxel<O32>(hd, p[6], lx0, ly1, lz1);
    L.r101 = load_voxel<O32>(hd, p[5], lx1, ly0, lz1); L.r111 = load_voxel<O32>(hd, p[7], lx1, ly1, lz1);
    return true;
}
template <bool PACKED>
VHD bool taps_finish(TapLoads& L, float vs, float rvs, F3 pos, float& dist)
{
    // (all eight have arrived together: see trilinear)
    asm volatile("" : "+v"(L.r000.x), "+v"(L.r000.y), "+v"(L.r100.x), "+v"(L.r100.y), "+v"(L.r010.x), "+v"(L.r010.y), "+v"(L.r001.x), "+v"(L.r001.y),
                      "+v"(L.r110.x), "+v"(L.r110.y), "+v"(L.r011.x), "+v"(L.r011.y), "+v"(L.r101.x), "+v"(L.r101.y), "+v"(L.r111.x), "+v"(L.r111.y));
    const Vox v000 = unpack_vox(L.r000), v100 = unpack_vox(L.r100), v010 = unpack_vox(L.r010), v001 = unpack_vox(L.r001);
    const Vox v110 = unpack_vox(L.r110), v011 = unpack_vox(L.r011), v101 = unpack_vox(L.r101), v111 = unpack_vox(L.r111);
    const uint32_t wmin = min(min(min(v000.cw, v100.cw), min(v010.cw, v001.cw)), min(min(v110.cw, v011.cw), min(v101.cw, v111.cw)));
    if ((wmin >> 24) == 0u) return false;
    float s[8];
    tap_weights<PACKED>(pos, vs, rvs, s);
    float d = 0.0f;
    // (the reference's tap order and arithmetic: trilinear)
    d += s[0] * v000.sdf;
    d += s[1] * v100.sdf;
    d += s[2] * v010.sdf;
    d += s[3] * v001.sdf;
    d += s[4] * v110.sdf;
    d += s[5] * v011.sdf;
    d += s[6] * v101.sdf;
    d += s[7] * v111.sdf;
    dist = d;
    return true;
}

// The same function with the reference's tap-by-tap early-out, leaving the
// partial sum in `dist` on failure: gradientForPoint (:174-195) ignores the
// return value and uses that partial sum.
__device__ __noinline__ float trilinear_partial(const VhHashData hd, const VhHashParams hp, float px, float py, float pz)
{
    const float vs = hp.m_virtualVoxelSize;
    const float oSet = vs;
    const float h = oSet / 2.0f;
    const F3 pd = mk3(px - h, py - h, pz - h);
    const float fx = px / vs, fy = py / vs, fz = pz / vs;
    const float wx = fx - floorf(fx), wy = fy - floorf(fy), wz = fz - floorf(fz);
    float d = 0.0f;
#pragma unroll 1
    for (uint32_t k = 0; k < 8u; k++) {
        // reference tap order 000,100,010,001,110,011,101,111 as (x,y,z) bit triples
        const uint32_t combo = (0x75634210u >> (4u * k)) & 7u; // k-th nibble: 0,1,2,4,3,6,5,7
        const bool bx = combo & 1u, by = combo & 2u, bz = combo & 4u;
        const int vx = world_to_vvp1(bx ? pd.x + oSet : pd.x, vs);
        const int vy = world_to_vvp1(by ? pd.y + oSet : pd.y, vs);
        const int vz = world_to_vvp1(bz ? pd.z + oSet : pd.z, vs);
        const int p = lookup_ptr(hd, hp, mki3(vvp_to_block1(vx), vvp_to_block1(vy), vvp_to_block1(vz)));
        if (p == VH_FREE_ENTRY) return d;
        const Vox v = unpack_vox(load_voxel(hd, p, local1(vx), local1(vy), local1(vz)));
        if (v.weight() == 0u) return d;
        const float s = (bx ? wx : 1.0f - wx) * (by ? wy : 1.0f - wy) * (bz ? wz : 1.0f - wz);
        d += s * v.sdf;
    }
    return d;
}

// gradientForPoint :174-195
VHD F3 gradient_for_point(const VhHashData& hd, const VhHashParams& hp, F3 pos)
{
    const float vs = hp.m_virtualVoxelSize;
    const float dp00 = trilinear_partial(hd, hp, pos.x - 0.5f * vs, pos.y - 0.0f, pos.z - 0.0f);
    const float d0p0 = trilinear_partial(hd, hp, pos.x - 0.0f, pos.y - 0.5f * vs, pos.z - 0.0f);
    const float d00p = trilinear_partial(hd, hp, pos.x - 0.0f, pos.y - 0.0f, pos.z - 0.5f * vs);
    const float d100 = trilinear_partial(hd, hp, pos.x + 0.5f * vs, pos.y + 0.0f, pos.z + 0.0f);
    const float d010 = trilinear_partial(hd, hp, pos.x + 0.0f, pos.y + 0.5f * vs, pos.z + 0.0f);
    const float d001 = trilinear_partial(hd, hp, pos.x + 0.0f, pos.y + 0.0f, pos.z + 0.5f * vs);
    const F3 g = mk3((dp00 - d100) / vs, (d0p0 - d010) / vs, (d00p - d001) / vs);
    const float l = sqrtf(dot3(g, g));
    if (l == 0.0f) return mk3(0.0f, 0.0f, 0.0f);
    return mk3(-g.x / l, -g.y / l, -g.z / l);
}

// Tap voxel coordinates of the sample at ray parameter t.
// Division-free when possible: q ~ pos/voxel is evaluated approximately (one fma per axis).  The lower tap
// of an axis is round_half_away((pos - voxel/2)/voxel) = floor(pos/voxel) and the upper tap is that + 1
// whenever pos/voxel is not within rounding distance of an integer: a fractional part further than the ray's
// margin (ray_setup, below) from 0 and 1 settles both taps.  Anything closer takes the exact path with the
// reference's arithmetic.  The decision is made per WAVE-iteration in practice (one uncertain lane sends the whole
// wave through the exact code), hence the tight margin: ~0.3 % per lane at Q = 256.
struct RayQ {
    F3 cam, dir;   // exact ray (world)
    F3 camq, dirq; // ~ cam/voxel, dir/voxel
    float vs, rvs, halfVoxel;
    float certLim; // 0.5 - margin, negative if the approximation must not be used
};

VHD void tap_coords(const RayQ& rq, float t, Taps& tp)
{
    // (x and y as a pair: the fma, the distance from the floor and from one half)
    const f32x2 qxy = fma2(both(t), (f32x2){ rq.dirq.x, rq.dirq.y }, (f32x2){ rq.camq.x, rq.camq.y });
    const float qz = __fmaf_rn(t, rq.dirq.z, rq.camq.z);
    const float gx = floorf(qxy.x), gy = floorf(qxy.y), gz = floorf(qz);
    const f32x2 dxy = (qxy - (f32x2){ gx, gy }) - both(0.5f);
    const float dev = fmaxf(fmaxf(fabsf(dxy.x), fabsf(dxy.y)), fabsf((qz - gz) - 0.5f));
    if (dev < rq.certLim) {
        tp.x0 = (int)gx; tp.y0 = (int)gy; tp.z0 = (int)gz;
        tp.x1 = tp.x0 + 1; tp.y1 = tp.y0 + 1; tp.z1 = tp.z0 + 1;
    } else {
        const F3 pd = mk3((rq.cam.x + t * rq.dir.x) - rq.halfVoxel, (rq.cam.y + t * rq.dir.y) - rq.halfVoxel, (rq.cam.z + t * rq.dir.z) - rq.halfVoxel);
        tp.x0 = world_to_vvp1_rb(pd.x, rq.vs, rq.rvs); tp.y0 = world_to_vvp1_rb(pd.y, rq.vs, rq.rvs); tp.z0 = world_to_vvp1_rb(pd.z, rq.vs, rq.rvs);
        tp.x1 = world_to_vvp1_rb(pd.x + rq.vs, rq.vs, rq.rvs); tp.y1 = world_to_vvp1_rb(pd.y + rq.vs, rq.vs, rq.rvs); tp.z1 = world_to_vvp1_rb(pd.z + rq.vs, rq.vs, rq.rvs);
    }
    tp.bxa = vvp_to_block1(tp.x0); tp.bya = vvp_to_block1(tp.y0); tp.bza = vvp_to_block1(tp.z0);
    tp.bxb = vvp_to_block1(tp.x1); tp.byb = vvp_to_block1(tp.y1); tp.bzb = vvp_to_block1(tp.z1);
}

// The constants of the ray cam + t dir, for samples at parameters |t| <= tFar (the caller's bound: march and bisection
// parameters lie inside the marched range).
VHD RayQ ray_setup(F3 cam, F3 dir, float voxel, float tFar)
{
    RayQ rq;
    rq.cam = cam; rq.dir = dir;
    rq.vs = voxel;
    rq.rvs = 1.0f / rq.vs; // IEEE reciprocal for div_exact
    rq.halfVoxel = rq.vs / 2.0f;
    rq.camq = mk3(cam.x * rq.rvs, cam.y * rq.rvs, cam.z * rq.rvs);
    rq.dirq = mk3(dir.x * rq.rvs, dir.y * rq.rvs, dir.z * rq.rvs);
    // Q bounds |pos/voxel| for every sample of this ray
    const float Q = 1.0f + (fabsf(rq.camq.x) + fabsf(rq.camq.y) + fabsf(rq.camq.z)) +
                    tFar * (fabsf(rq.dirq.x) + fabsf(rq.dirq.y) + fabsf(rq.dirq.z));
    // Margin: 16 u Q with u = 2^-24.  Per axis, with S = (|cam| + t |dir|) / voxel <= Q - 1: the fused route
    // q = fma(t, dir * r, cam * r), r = fl(1 / voxel), is within 3 u S of the real (cam + t dir) / voxel (r, the
    // two scaled operands, the fma); the reference's route -- fl(t dir), + cam, - half, / voxel, +- 0.5, and for
    // the upper tap + voxel before the division -- within u (6 S + 5.5) of the same number.  Both take the floor:
    // they agree when q is further than u (9 S + 5.5) < 16 u Q from an integer.
    const float margin = Q * (16.0f / 16777216.0f);
    rq.certLim = (Q < 65536.0f) ? 0.5f - margin : -1.0f; // NaN/inf Q compare false: exact path
    return rq;
}

// findIntersectionBisection :149-170 on [lastAlpha, t] -- the last valid sample (lastAlpha, lastSdf) and the march sample
// (t, dist) -- and the acceptance of its result (:227-229, the two thresholds).  `color` is the last bisection sample's.
// By value, `success = false; break;` kept: with reference outputs and an early return k_render_large<true, *> loses a wave per SIMD.
// (a -DVH_RENDER_STATS build counts the plain march only, which has this text in place)
//
// One step of the bisection, for a loop or a `do ... while (0)` around it (it leaves with `break` when the sample is invalid).
// COLOR: blend the sample's colour into COLOUR; STAT: the counters of a -DVH_RENDER_STATS build (the plain march's alone).  The reference reads the colour of the LAST sample alone (trilinear), and a
// bisection whose sample fails ends in "no hit": the first two steps blend none, the third is peeled off the loop.  (As a
// scalar branch on the step number inside one loop -- two copies of the blend, or one with the colour part behind a flag --
// k_render<false, *> went from 8 / 16 to 24..44 bytes of scratch: profiles/README.md.)
#ifdef VH_RENDER_STATS
#define VH_STAT_BISECT_SAMPLE statTri += 1.0f; statIter += 1.0f / (float)__popcll(__ballot(1));
#else
#define VH_STAT_BISECT_SAMPLE
#endif
// CAUTION: the step holds a `break`.  It has to stand directly in the loop (or `do ... while (0)`) it is to leave, never
// inside another loop or a switch, and `success` has to be tested before any step that follows the loop.
#define VH_BISECT_STEP(COLOR, CAM, DIR, COLOUR, STAT)                                                                               \
    {                                                                                                                               \
        STAT                                                                                                                        \
        cost += kCostSample;                                                                                                        \
        c = a + (aDist / (aDist - bDist)) * (b - a); /* findIntersectionLinear :140-143 */                                          \
        Taps ctp;                                                                                                                   \
        tap_coords(rq, c, ctp);                                                                                                     \
        const F3 cpos = ray_point(CAM, DIR, c);                                                                                     \
        float cDist = 0.0f;                                                                                                         \
        if (!trilinear<COLOR>(hd, rq.vs, lk, kPtrUnknown, ctp, cpos, rq.rvs, cDist, COLOUR)) { success = false; break; }            \
        if (aDist * cDist > 0.0f) { a = c; aDist = cDist; }                                                                         \
        else { b = c; bDist = cDist; }                                                                                              \
    }
struct Bisected {
    float alpha;
    uint32_t color;
    bool accepted;
};
template <class LK>
VHD Bisected bisect(LK& lk, const VhHashData& hd, const RayQ& rq, float lastAlpha, float lastSdf, float t, float dist,
                    float thresSampleDist, float thresDist, uint32_t& cost)
{
    float a = lastAlpha, aDist = lastSdf, b = t, bDist = dist, c = 0.0f;
    uint32_t color = 0u;
    bool success = true;
#pragma unroll 1
    for (int i = 0; i < 2; i++) VH_BISECT_STEP(false, rq.cam, rq.dir, color, )
    if (success) do VH_BISECT_STEP(true, rq.cam, rq.dir, color, ) while (0);
    Bisected r;
    r.alpha = c;
    r.color = color;
    r.accepted = success && fabsf(lastSdf - dist) < thresSampleDist && fabsf(dist) < thresDist;
    return r;
}

#ifndef VH_PIPELINE_SMALL // (measurement builds: the pipelined march with the small tables too)
#define VH_PIPELINE_SMALL 0
#endif

struct RayHit {
    float alpha;    // ray parameter of the accepted intersection; NaN-free flag in `hit`
    uint32_t color; // packed colour of the last bisection sample
    bool hit;
    float depthToRayLength;
    F3 normal;      // GRADIENTS only (camera space)
};

// traverseCoarseGridSimpleSampleAll, DSC/RayCastSDFUtil.h:198-262, for the ray of pixel (x, y), restricted to the
// tile's conservative depth interval [tileZmin, tileZmax].  Written as march-until-sign-change / bisect / resume so
// that the lanes of a wave run their bisections together instead of interleaving them with other lanes' marching;
// each ray's own sequence of samples is the reference's.
template <bool GRADIENTS, bool PIPELINED = false, class LK>
VHD void march_ray(LK& lk, const VhHashData& hd, const VhHashParams& hp, const VhDepthCameraParams& cp, const VhRayCastParams& rp,
                   uint32_t x, uint32_t y, float tileZmin, float tileZmax, uint32_t half, float zMid, RayHit& out, uint32_t& cost
#ifdef VH_RENDER_STATS
                   , float& statTri, float& statIter, float (&statCyc)[3]
#endif
)
{
    const float mi = minf();
    const F3 camDir = normalize3(depth_to_skeleton(cp, x, y, proj_to_cam_z(cp, 1.0f)));
    const F3 worldCamPos = mat_mul_p(rp.m_viewMatrixInverse, mk3(0.0f, 0.0f, 0.0f));
    const F3 worldDir = normalize3(mat_mul_d(rp.m_viewMatrixInverse, camDir));

    const float minInterval = rp.m_minDepth, maxInterval = rp.m_maxDepth;
    const bool run = !(minInterval == 0.0f || minInterval == mi) && !(maxInterval == 0.0f || maxInterval == mi);
    if (!run) return;
    const float depthToRayLength = 1.0f / camDir.z;
    out.depthToRayLength = depthToRayLength;
    const float rayEnd = depthToRayLength * fminf(rp.m_maxDepth, maxInterval);
    const float inc = rp.m_rayIncrement;
    const RayQ rq = ray_setup(worldCamPos, worldDir, hp.m_virtualVoxelSize, fabsf(rayEnd)); // (march and bisection parameters are <= rayEnd)

    float rcur = depthToRayLength * fmaxf(rp.m_minDepth, minInterval); // rayCurrent
    float lastSdf = 0.0f, lastAlpha = 0.0f;
    int lastValid = 0; // flags live in VGPRs: on this kernel the scalar unit (one per CU) is the scarce resource

    // Interval of the tile in ray-parameter units.  Samples before it have their first tap in no allocated block
    // (they are invalid: lastValid = 0), samples after it likewise, so nothing can be hit there.  rcur still
    // advances by the same sequence of additions, one VALU op per skipped sample.
    const float tSkip = depthToRayLength * tileZmin;
    float tStop = fminf(rayEnd, depthToRayLength * tileZmax);
#pragma unroll 1
    while (rcur < tSkip && rcur < rayEnd) rcur += inc;
    if (half != 0u) { // half of a split tile (wave-uniform): the near one samples before tMid, the far one from the last sample before it
        const float tMid = depthToRayLength * zMid;
        if (half == 1u) {
            tStop = fminf(tStop, tMid);
        } else {
#pragma unroll 1
            for (;;) {
                const float nxt = rcur + inc; // the same additions the march makes
                if (!(nxt < tMid) || !(nxt < rayEnd)) break;
                rcur = nxt;
            }
            // That sample is the near half's last, taken here again for its distance (a sign change across tMid) and paid
            // for there: what it will be charged below is taken off in advance, so that a lane's two parts add up to the
            // cost of its ray in a whole tile.  (The counter may wrap below 0: it is only ever added to the near half's.)
            // For tiles with complete lists and without gradients only: the general lookup's probe brings a copy of the hash
            // table walk (k_render<false, true> 76 -> 80 registers, the cfg2 frame 1 % slower), and with gradients it costs
            // k_render<true, *> 32 bytes of scratch and k_render_large<true, *> 14 registers; there a split tile stays dearer
            // by that one sample at most.
            if (!LK::kGeneral && !GRADIENTS && rcur < tMid && rcur < tStop) {
                // (the block of the sample's first tap by tap_coords' exact route alone: this runs once per ray)
                const F3 pd = mk3((rq.cam.x + rcur * rq.dir.x) - rq.halfVoxel, (rq.cam.y + rcur * rq.dir.y) - rq.halfVoxel, (rq.cam.z + rcur * rq.dir.z) - rq.halfVoxel);
                int h0 = kPtrUnknown;
                const bool there = lk.first_tap(vvp_to_block1(world_to_vvp1_rb(pd.x, rq.vs, rq.rvs)), vvp_to_block1(world_to_vvp1_rb(pd.y, rq.vs, rq.rvs)),
                                                vvp_to_block1(world_to_vvp1_rb(pd.z, rq.vs, rq.rvs)), h0);
                cost -= 1u + (there ? kCostSample : 0u);
            }
        }
    }

    if constexpr (PIPELINED) {
        // The same march with the NEXT sample's voxels asked for before this sample's are blended.  With three waves on a SIMD
        // (the large tables) and, in a frame's long tail, one, a wave otherwise runs at the pace of its own chain: probe,
        // eight loads, a trip to memory, blend, probe, ...  The next sample is the one the march would take next whatever this
        // one turns out to be (also after a bisection that did not end the ray: the march resumes one increment on), so what
        // is asked for early is never asked for in vain but at the end of the ray.  Every ray's sequence of samples, and what
        // is computed from each, is the plain march's.
        struct Pending {
            float r;      // the sample's ray parameter
            int skipped;  // samples without a block lay between the previous sample and this one
            int state;    // 0: the ray has left the range, 1: the eight voxels are in flight, 2: a block is missing (invalid)
            TapLoads L;
        };
        auto fetch = [&](float r0) -> Pending {
            Pending f;
            f.skipped = 0;
            float r = r0;
            Taps tp;
            int p0 = kPtrUnknown;
#pragma unroll 1
            while (r < tStop) { // (A: samples whose first tap has no block)
                cost += 1u;
                tap_coords(rq, r, tp);
                if (lk.first_tap(tp.bxa, tp.bya, tp.bza, p0)) break;
                f.skipped = 1;
                r += inc;
            }
            f.r = r;
            f.state = 0;
            if (r < tStop) {
                cost += kCostSample;
                f.state = taps_issue(hd, lk, p0, tp, f.L) ? 1 : 2;
            }
            return f;
        };
        Pending P = fetch(rcur);
#pragma unroll 1
        for (;;) {
            bool candidate = false;
            float dist = 0.0f;
            Pending N;
            N.state = 0; N.r = 0.0f; N.skipped = 0;
#pragma unroll 1
            for (;;) {
                if (P.state == 0) break; // ray left the depth range (or the range in which blocks exist)
                N = fetch(P.r + inc);
                rcur = P.r;
                lastValid = P.skipped ? 0 : lastValid;
                bool ok = false;
                if (P.state == 1) ok = taps_finish<LK::kOffsets32>(P.L, rq.vs, rq.rvs, ray_point(worldCamPos, worldDir, rcur), dist);
                if (ok & (lastValid != 0) & (lastSdf > 0.0f) & (dist < 0.0f)) { candidate = true; break; }
                lastSdf = ok ? dist : lastSdf;
                lastAlpha = ok ? rcur : lastAlpha;
                lastValid = ok ? 1 : 0;
                P = N;
            }
            if (!candidate) break;
            const Bisected bs = bisect(lk, hd, rq, lastAlpha, lastSdf, rcur, dist, rp.m_thresSampleDist, rp.m_thresDist, cost);
            if (bs.accepted) {
                out.hit = true;
                out.alpha = bs.alpha;
                out.color = bs.color;
                if (GRADIENTS) {
                    const F3 iso = mk3(worldCamPos.x + bs.alpha * worldDir.x, worldCamPos.y + bs.alpha * worldDir.y, worldCamPos.z + bs.alpha * worldDir.z);
                    const F3 g = gradient_for_point(hd, hp, iso);
                    out.normal = mat_mul_d(rp.m_viewMatrix, mk3(-g.x, -g.y, -g.z));
                }
                break;
            }
            // no accepted hit: the (valid) march sample becomes the last sample and the march goes on (:248-252) -- at N
            lastSdf = dist;
            lastAlpha = rcur;
            lastValid = 1;
            P = N;
        }
        return;
    }

#pragma unroll 1
    for (;;) {
        // ---- march until a sign change (or the end of the range).  The lanes of a wave leave this loop together:
        // whichever lane finds its sign change first waits here, so that the wave runs ONE bisection phase for all
        // of them instead of one per march step.  Each ray's own sequence of samples is the reference's.
        bool candidate = false;
        float dist = 0.0f;
#pragma unroll 1
        for (;;) {
            // ---- A: skip samples whose first tap has no block (they are invalid: weight 0 at the first tap)
            Taps tp;
            int p0 = kPtrUnknown;
            int skipped = 0;
#ifdef VH_RENDER_STATS
            const long long tA0 = clock64();
#endif
#pragma unroll 1
            while (rcur < tStop) {
#ifdef VH_RENDER_STATS
                statIter += 1024.0f / (float)__popcll(__ballot(1));
#endif
                cost += 1u;
                tap_coords(rq, rcur, tp);
                if (lk.first_tap(tp.bxa, tp.bya, tp.bza, p0)) break;
                skipped = 1;
                rcur += inc;
            }
#ifdef VH_RENDER_STATS
            statCyc[0] += (float)(clock64() - tA0);
            const long long tB0 = clock64();
#endif
            if (!(rcur < tStop)) break; // ray left the depth range (or the range in which blocks exist)
            lastValid = skipped ? 0 : lastValid;

            // ---- B: full sample at rcur
#ifdef VH_RENDER_STATS
            statTri += 1.0f;
            statIter += 1.0f / (float)__popcll(__ballot(1));
#endif
            cost += kCostSample;
            uint32_t colorUnused = 0u;
            const F3 pos = ray_point(worldCamPos, worldDir, rcur);
            const bool ok = trilinear<false>(hd, rq.vs, lk, p0, tp, pos, rq.rvs, dist, colorUnused);
#ifdef VH_RENDER_STATS
            statCyc[1] += (float)(clock64() - tB0);
#endif
            if (ok & (lastValid != 0) & (lastSdf > 0.0f) & (dist < 0.0f)) { candidate = true; break; }
            lastSdf = ok ? dist : lastSdf;
            lastAlpha = ok ? rcur : lastAlpha;
            lastValid = ok ? 1 : 0;
            rcur += inc;
        }
        if (!candidate) break;

        // ---- findIntersectionBisection :149-170 on [lastAlpha, rcur]: bisect()'s text, in place.  Called as bisect() it gives
        // k_render<false, true> fewer instructions and no scratch, and the cfg2 frame 1.7 % less (profiles/README.md)
        float a = lastAlpha, aDist = lastSdf, b = rcur, bDist = dist, c = 0.0f;
        uint32_t color2 = 0u;
        bool success = true;
#ifdef VH_RENDER_STATS
        const long long tC0 = clock64();
#endif
        // (with gradients the three steps stay one loop that blends the colour each time: peeled, k_render<true, *> spills more)
        if constexpr (GRADIENTS) {
#pragma unroll 1
            for (int i = 0; i < 3; i++) VH_BISECT_STEP(true, worldCamPos, worldDir, color2, VH_STAT_BISECT_SAMPLE)
        } else {
#pragma unroll 1
            for (int i = 0; i < 2; i++) VH_BISECT_STEP(false, worldCamPos, worldDir, color2, VH_STAT_BISECT_SAMPLE)
            if (success) do VH_BISECT_STEP(true, worldCamPos, worldDir, color2, VH_STAT_BISECT_SAMPLE) while (0);
        }
#ifdef VH_RENDER_STATS
        statCyc[2] += (float)(clock64() - tC0);
#endif
        if (success && fabsf(lastSdf - dist) < rp.m_thresSampleDist && fabsf(dist) < rp.m_thresDist) {
            out.hit = true;
            out.alpha = c;
            out.color = color2;
            if (GRADIENTS) {
                const F3 iso = mk3(worldCamPos.x + c * worldDir.x, worldCamPos.y + c * worldDir.y, worldCamPos.z + c * worldDir.z);
                const F3 g = gradient_for_point(hd, hp, iso);
                out.normal = mat_mul_d(rp.m_viewMatrix, mk3(-g.x, -g.y, -g.z));
            }
            break;
        }
        // no accepted hit: the (valid) march sample becomes the last sample and the march goes on (:248-252)
        lastSdf = dist;
        lastAlpha = rcur;
        lastValid = 1;
        rcur += inc;
    }
}

#undef VH_BISECT_STEP
#undef VH_STAT_BISECT_SAMPLE

// the maps of one pixel (renderKernel DSC/CUDARayCastSDF.cu:18-57; outputs of traverseCoarseGridSimpleSampleAll :236-247)
VHD void store_ray(const VhRayCastData& rd, const VhDepthCameraParams& cp, size_t pix, uint32_t x, uint32_t y, const RayHit& r, bool gradients)
{
    const float mi = minf();
    float depth = mi;
    float4 depth4 = make_float4(mi, mi, mi, mi), normal = depth4, color = depth4;
    if (r.hit) {
        depth = r.alpha / r.depthToRayLength;
        const F3 sk = depth_to_skeleton(cp, x, y, depth);
        depth4 = make_float4(sk.x, sk.y, sk.z, 1.0f);
        // (a byte over 255 through the constant's reciprocal: half the instructions of `/`, the same bits for all 256 -- vh_debug_check_fast_math)
        constexpr float r255 = 1.0f / 255.0f;
        color = make_float4(div_exact((float)(r.color & 0xffu), 255.0f, r255), div_exact((float)((r.color >> 8) & 0xffu), 255.0f, r255),
                            div_exact((float)((r.color >> 16) & 0xffu), 255.0f, r255), 1.0f);
        if (gradients) normal = make_float4(r.normal.x, r.normal.y, r.normal.z, 1.0f);
    }
    rd.d_depth[pix] = depth;
    reinterpret_cast<float4*>(rd.d_depth4)[pix] = depth4;
    if (rd.d_normals) reinterpret_cast<float4*>(rd.d_normals)[pix] = normal; // a null map is not written (vh_api.h)
    reinterpret_cast<float4*>(rd.d_colors)[pix] = color;
}

#ifdef VH_RENDER_STATS
#define VH_STAT_DECL const long long statT0 = clock64(); const long long statR0 = wall_clock64(); float statTri = 0.0f, statIter = 0.0f; float statCyc[3] = { 0.0f, 0.0f, 0.0f };
#define VH_STAT_ARGS , statTri, statIter, statCyc
#define VH_STAT_STORE                                                                                                                   \
    {                                                                                                                                   \
        const uint32_t hwid = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);              \
        reinterpret_cast<float4*>(rd.d_depth4)[pix] = make_float4(statCyc[0], statCyc[1], statCyc[2], 0.0f);                             \
        reinterpret_cast<float4*>(rd.d_normals)[pix] = make_float4((float)(clock64() - statT0), statTri, statIter, (float)(wall_clock64() - statR0)); \
        reinterpret_cast<float4*>(rd.d_colors)[pix] = make_float4((float)(uint32_t)(statR0 & 0xffffffll), (float)((hwid >> 8) & 0xfu),  \
            (float)((hwid >> 13) & 0x7u) + 8.0f * (float)((hwid >> 12) & 1u), (float)(xcc & 0xfu) * 4.0f + (float)((hwid >> 4) & 3u));   \
    }
#else
#define VH_STAT_DECL
#define VH_STAT_ARGS
#define VH_STAT_STORE
#endif

// One wave per 8x8-pixel tile, block pointers from the hash table: the reference fork's ray caster (no intervals).
template <bool GRADIENTS>
__global__ __launch_bounds__(256) void k_render_hash(VhHashData hd, VhHashParams hp, VhRayCastData rd,
                                                     VhDepthCameraParams cp, VhRayCastParams rp, HashMod hm)
{
    const uint32_t lane = lane_id();
    const uint32_t W = rp.m_width, H = rp.m_height;
    const uint32_t tilesX = (W + 7) / 8, tilesY = (H + 7) / 8;
    const uint32_t tile = blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
    if (tile >= tilesX * tilesY) return;
    const uint32_t x = (tile % tilesX) * 8 + (lane & 7), y = (tile / tilesX) * 8 + (lane >> 3);
    if (x >= W || y >= H) return;
    const size_t pix = (size_t)y * W + x;
    VH_STAT_DECL
    RayHit out;
    out.hit = false;
    HashLookup lk{ hd, hp, hm, {} };
    cache_init(lk.bc);
    uint32_t cost = 0u;
    march_ray<GRADIENTS>(lk, hd, hp, cp, rp, x, y, 0.0f, pinf(), 0u, 0.0f, out, cost VH_STAT_ARGS);
    store_ray(rd, cp, pix, x, y, out, GRADIENTS);
    VH_STAT_STORE
}

// ---------------------------------------------------------------------------
// batch queries (not in the reference: vh_query_points / vh_query_rays, DESIGN.md section 4 "Queries").  Read-only;
// one lane per point or ray, block pointers from the hash table behind the per-lane cache of k_render_hash.
// ---------------------------------------------------------------------------

VHD bool finite3(F3 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }

// trilinearInterpolationSimpleFastFast + gradientForPoint at given world points.  The taps come from tap_coords'
// exact route (the reference's arithmetic: a point is a ray of direction 0 sampled at 0).
__global__ __launch_bounds__(256) void k_query_points(VhHashData hd, VhHashParams hp, const float* __restrict__ points, uint32_t n,
                                                      float* __restrict__ sdf, uint32_t* __restrict__ color, float* __restrict__ gradient,
                                                      uint8_t* __restrict__ valid, HashMod hm)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const F3 p = mk3(points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]);
    float dist = minf();
    uint32_t col = 0u;
    bool ok = false;
    F3 g = mk3(0.0f, 0.0f, 0.0f);
    if (finite3(p)) { // decided before any lookup
        RayQ rq;
        rq.cam = p; rq.dir = mk3(0.0f, 0.0f, 0.0f);
        rq.camq = rq.dirq = mk3(0.0f, 0.0f, 0.0f);
        rq.vs = hp.m_virtualVoxelSize;
        rq.rvs = 1.0f / rq.vs;
        rq.halfVoxel = rq.vs / 2.0f;
        rq.certLim = -1.0f;
        Taps tp;
        tap_coords(rq, 0.0f, tp);
        HashLookup lk{ hd, hp, hm, {} };
        cache_init(lk.bc);
        float d = 0.0f;
        uint32_t c = 0u;
        ok = trilinear<true>(hd, rq.vs, lk, kPtrUnknown, tp, p, rq.rvs, d, c);
        if (ok) { dist = d; col = c; } // the reference's partial sum of an invalid sample is not reported
        if (gradient) g = gradient_for_point(hd, hp, p); // at every point: its six samples ignore their own validity
    }
    sdf[i] = dist;
    color[i] = col;
    valid[i] = ok ? 1 : 0;
    if (gradient) { gradient[3 * (size_t)i] = g.x; gradient[3 * (size_t)i + 1] = g.y; gradient[3 * (size_t)i + 2] = g.z; }
}

#ifdef VH_QUERY_RAYS_WAVES // (measurement builds: the waves per SIMD k_query_rays is compiled for; default: the compiler's choice)
#define VH_QUERY_RAYS_OCCUPANCY __attribute__((amdgpu_waves_per_eu(VH_QUERY_RAYS_WAVES, VH_QUERY_RAYS_WAVES)))
#else
#define VH_QUERY_RAYS_OCCUPANCY
#endif

// traverseCoarseGridSimpleSampleAll, DSC/RayCastSDFUtil.h:198-262, for rays given in world space: worldCamPos = origin,
// worldDir = direction (as given), rayCurrent = tMin, rayEnd = tMax.  The plain march of march_ray without its tile
// interval, its cost accounting and its camera.  Shared with it: ray_setup, tap_coords, trilinear and bisect (with the
// thresholds; its cost counter is thrown away here).  Restated here: the march loop with its limits (tMax and the sample
// count), the sign-change test and the carry of the last sample.  Lanes of a wave finish at different times (a wave lasts as long as its
// longest ray): rays in a coherent order -- neighbours in space next to each other -- are the caller's gain.
// The march counts its samples and stops at VH_QUERY_MAX_SAMPLES, so no caller data can spin a wave (t + inc == t).
__global__ __launch_bounds__(256) VH_QUERY_RAYS_OCCUPANCY void k_query_rays(VhHashData hd, VhHashParams hp, float inc, float thresSampleDist, float thresDist,
                                                    const float* __restrict__ origins, const float* __restrict__ directions,
                                                    const float* __restrict__ tMin, const float* __restrict__ tMax, uint32_t n,
                                                    float* __restrict__ tOut, float* __restrict__ normals, uint32_t* __restrict__ color,
                                                    uint8_t* __restrict__ status, HashMod hm)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float mi = minf();
    const F3 cam = mk3(origins[3 * (size_t)i], origins[3 * (size_t)i + 1], origins[3 * (size_t)i + 2]);
    const F3 dir = mk3(directions[3 * (size_t)i], directions[3 * (size_t)i + 1], directions[3 * (size_t)i + 2]);
    const float t0 = tMin[i], rayEnd = tMax[i];
    float alpha = mi;
    F3 nrm = mk3(mi, mi, mi);
    uint32_t col = 0u;
    uint32_t st = 0u;
    const bool refused = !(finite3(cam) && finite3(dir) && isfinite(t0) && isfinite(rayEnd)) ||
                         (dir.x == 0.0f && dir.y == 0.0f && dir.z == 0.0f) ||
                         (rayEnd - t0) / inc > (float)VH_QUERY_MAX_SAMPLES;
    if (refused) {
        st = 2u;
    } else {
        const RayQ rq = ray_setup(cam, dir, hp.m_virtualVoxelSize, fmaxf(fabsf(t0), fabsf(rayEnd))); // (parameters lie in [tMin, tMax))
        HashLookup lk{ hd, hp, hm, {} };
        cache_init(lk.bc);
        float rcur = t0;
        float lastSdf = 0.0f, lastAlpha = 0.0f;
        int lastValid = 0;
        uint32_t samples = 0u;
        uint32_t cost = 0u; // (bisect's accounting, thrown away here)
#pragma unroll 1
        for (;;) {
            // ---- march until a sign change, the end of the range or the sample cap
            bool candidate = false;
            float dist = 0.0f;
#pragma unroll 1
            for (;;) {
                // samples whose first tap has no block are invalid (weight 0 at the first tap)
                Taps tp;
                int p0 = kPtrUnknown;
                int skipped = 0;
#pragma unroll 1
                while (rcur < rayEnd && samples < (uint32_t)VH_QUERY_MAX_SAMPLES) {
                    tap_coords(rq, rcur, tp);
                    if (lk.first_tap(tp.bxa, tp.bya, tp.bza, p0)) break;
                    skipped = 1;
                    samples++;
                    rcur += inc;
                }
                if (!(rcur < rayEnd) || samples >= (uint32_t)VH_QUERY_MAX_SAMPLES) break;
                lastValid = skipped ? 0 : lastValid;
                samples++;
                uint32_t colorUnused = 0u;
                const F3 pos = mk3(cam.x + rcur * dir.x, cam.y + rcur * dir.y, cam.z + rcur * dir.z);
                const bool ok = trilinear<false>(hd, rq.vs, lk, p0, tp, pos, rq.rvs, dist, colorUnused);
                if (ok & (lastValid != 0) & (lastSdf > 0.0f) & (dist < 0.0f)) { candidate = true; break; }
                lastSdf = ok ? dist : lastSdf;
                lastAlpha = ok ? rcur : lastAlpha;
                lastValid = ok ? 1 : 0;
                rcur += inc;
            }
            if (!candidate) break;

            const Bisected bs = bisect(lk, hd, rq, lastAlpha, lastSdf, rcur, dist, thresSampleDist, thresDist, cost);
            if (bs.accepted) {
                st = 1u;
                alpha = bs.alpha;
                col = bs.color;
                if (normals) { // always from the gradient: there is no depth map to difference
                    const F3 g = gradient_for_point(hd, hp, mk3(cam.x + bs.alpha * dir.x, cam.y + bs.alpha * dir.y, cam.z + bs.alpha * dir.z));
                    nrm = mk3(-g.x, -g.y, -g.z);
                }
                break;
            }
            // no accepted hit: the (valid) march sample becomes the last sample and the march goes on (:248-252)
            lastSdf = dist;
            lastAlpha = rcur;
            lastValid = 1;
            rcur += inc;
        }
    }
    tOut[i] = alpha;
    color[i] = col;
    status[i] = (uint8_t)st;
    if (normals) { normals[3 * (size_t)i] = nrm.x; normals[3 * (size_t)i + 1] = nrm.y; normals[3 * (size_t)i + 2] = nrm.z; }
}

// One wave per 8x8-pixel tile with the tile's head and block list from k_interval_splat: the wave builds its block
// table in LDS, forms the tile's depth interval from the listed blocks and marches inside it.  The kernel is bound by
// VALU issue per SIMD: what counts is instructions per sample and even loads of the SIMDs.
// lane_id() from instructions the compiler does not merge with an earlier lane_id(): for code that would otherwise keep
// the number in a register across a long stretch that has none to spare
VHD uint32_t lane_id_again()
{
    uint32_t l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

template <bool GRADIENTS, uint32_t CAP, bool OFFSETS32>
VHD void render_tile(const VhHashData& hd, const VhHashParams& hp, const VhRayCastData& rd, const VhDepthCameraParams& cp, const VhRayCastParams& rp,
                     uint4* heads, const int4* lists, uint32_t cap, uint32_t* sched, uint32_t phase,
                     int (*tileTab)[2u * CAP * 12u])
{
    // CAP = blocks a tile's table takes: 64 (6 KB of LDS per wave, every tile of a 640x480 frame resident) or 128 (12 KB:
    // three workgroups per compute unit; for fine voxels, where a few tiles see more than 64 blocks and would
    // otherwise probe the hash table for every block the table could not hold)
    constexpr uint32_t kTileTabSlots = 2u * CAP;
    typedef TileLookup<kTileTabSlots, OFFSETS32, !GRADIENTS> Lookup;
    typedef TileLookupComplete<kTileTabSlots, OFFSETS32, !GRADIENTS> LookupComplete;
    static_assert(kTileSlotWords == 12u, "tileTab row size");
    const uint32_t lane = lane_id();
    const uint32_t W = rp.m_width, H = rp.m_height;
    const uint32_t tilesX = (W + 7) / 8, tilesY = (H + 7) / 8;
    const uint32_t nTiles = tilesX * tilesY;
    const uint32_t waveIdx = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (256u / kWave) + (threadIdx.x / kWave))); // (workgroups of 256: tileTab)
    // Launch order.  The kernel is as long as its busiest SIMD, and a SIMD's waves are the workgroups i, i+numCUs,
    // i+2 numCUs, ... in launch order.  k_interval_splat sorts the tiles by the cost the previous frame measured
    // (it differs little) and deals them to the workgroups so that the sums come out even.  The schedule carries the
    // phase it was made for: one that was not refreshed for this call is ignored (raster order).
    uint32_t tile = waveIdx, half = 0u; // half: 0 whole tile, 1 / 2 near / far half of a split tile (all four waves of a workgroup or none)
    if (sched) {
        // The wave's slot is asked for together with the schedule's phase, not behind it: where the slot lies depends on the
        // image and the wave alone (the launcher has seen to it that it lies inside the schedule for every wave of the grid,
        // whatever the schedule holds).  Both are used without a branch between them, so neither load waits for the other.
        const uint32_t made = sched[0];
        const unsigned long long ev = reinterpret_cast<const unsigned long long*>(sched + 4 + 4u * ((nTiles + 3u) / 4u))[waveIdx]; // {tile | half << 24, phase}
        const uint2 e = make_uint2((uint32_t)ev, (uint32_t)(ev >> 32));
        const bool fresh = made == phase, dealt = e.y == phase;
        tile = fresh ? (dealt ? (e.x & 0xffffffu) : nTiles) : waveIdx; // (nTiles: a slot the dealing left empty -- last, partial workgroup)
        half = fresh && dealt ? (e.x >> 24) : 0u;
    }
    if (tile >= nTiles) return;
#if defined(VH_KNOCKOUT) && VH_KNOCKOUT == 41 // measurement build: every wave's life, read by tools/render_stamps.py
    const uint32_t stamp0 = (uint32_t)__builtin_amdgcn_s_memrealtime();
    uint32_t stamp1 = 0u;
    uint4* const stampAt = reinterpret_cast<uint4*>(hd.d_hashCompactified) + (hp.m_hashNumBuckets * VH_HASH_BUCKET_SIZE) / 2u + 3u * waveIdx;
    uint32_t stampList = 0u;
#define VH_WAVE_STAMP(COST)                                                                                                                     \
    if (lane == 0) {                                                                                                                             \
        stampAt[0] = make_uint4(stamp0, stamp1, (uint32_t)__builtin_amdgcn_s_memrealtime(), tile | (half << 24));                               \
        stampAt[1] = make_uint4((COST), __builtin_amdgcn_s_getreg((31 << 11) | 4), __builtin_amdgcn_s_getreg((31 << 11) | 20), 0x57410000u | waveIdx); \
        stampAt[2] = make_uint4(stampList, 0u, 0u, 0u);                                                                                           \
    }
#else
#define VH_WAVE_STAMP(COST)
#endif
    // (in a scalar register: it is wanted again after the march, and a vector register held across the march is one spilled)
    const uint32_t waveInGroup = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    int* tab = tileTab[waveInGroup];
    // consume the head and re-arm it, so that no separate clear pass is needed
    const uint4 head = heads[tile];
    // With the large tables (three waves per SIMD: a trip to memory is not hidden by five other waves) the tile's list entries
    // are asked for at once, whatever the head will say of their number -- the list's CAP places exist whether they are used or
    // not: one trip instead of two before the table can be built (cfg3: 87.7 -> 84.6 us).  With the small tables the extra
    // 3 MB at the start of the launch cost more than the trip (cfg2 +1.0 us, cfg4 +1.3): there the entries wait for the head.
    constexpr uint32_t kPerLane = CAP / kWave; // list entries per lane
    constexpr bool kListAhead = CAP > (uint32_t)VH_TILE_LIST_CAPACITY;
    int4 ahead[kPerLane];
    if (kListAhead) {
#pragma unroll
        for (uint32_t k = 0; k < kPerLane; k++) {
            ahead[k] = make_int4(0, 0, 0, VH_FREE_ENTRY);
            if (lane + k * kWave < min(cap, CAP)) ahead[k] = lists[(size_t)tile * cap + lane + k * kWave];
        }
    }
    float tileZmin = __uint_as_float(head.x), tileZmax = __uint_as_float(head.y); // as splatted (lists == nullptr)
    if (lane == 0 && half == 0u) heads[tile] = make_uint4(0x7f800000u, 0u, 0u, 0u); // (a split tile: once both halves have read it)
    const uint32_t listed = min(head.z, min(cap, CAP));
    // wave-uniform, and said so: the two marches below are then the two sides of a scalar branch, and what the one for
    // overflowed lists needs does not have to outlive the other
    const bool complete = __builtin_amdgcn_readfirstlane(listed == head.z ? 1 : 0) != 0;
#if defined(VH_KNOCKOUT) && VH_KNOCKOUT == 41
    stampList = head.z | (complete ? 0u : 0x10000u);
#endif
    // feedback for the host's choice of CAP: the longest list of the frame (only lists near the small capacity report)
    if (sched && lane == 0 && head.z > (uint32_t)VH_TILE_LIST_CAPACITY - 16u) atomicMax(&sched[1], head.z);
    for (uint32_t i = lane; i < kTileTabSlots; i += kWave) tab[i * kTileSlotWords + 3u] = VH_FREE_ENTRY;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    int4 mine[kPerLane];
    uint32_t slot[kPerLane];
#pragma unroll
    for (uint32_t k = 0; k < kPerLane; k++) {
        const uint32_t i = lane + k * kWave;
        mine[k] = make_int4(0, 0, 0, VH_FREE_ENTRY);
        slot[k] = 0u;
        if (i < listed) {
            mine[k] = kListAhead ? ahead[k] : lists[(size_t)tile * cap + i];
            uint32_t h = Lookup::slot_of(mine[k].x, mine[k].y, mine[k].z);
            // claim a slot through its pointer word, then fill in the position (nobody reads it before the barrier)
            while (atomicCAS(&tab[h * kTileSlotWords + 3u], VH_FREE_ENTRY, mine[k].w) != VH_FREE_ENTRY) h = (h + 1u) & (kTileTabSlots - 1u);
            tab[h * kTileSlotWords + 0u] = mine[k].x; tab[h * kTileSlotWords + 1u] = mine[k].y; tab[h * kTileSlotWords + 2u] = mine[k].z;
            slot[k] = h;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // (a short list: its 7 x listed probes dealt to the lanes, a probe each per round, instead of seven in a row in the lanes that
    // hold an entry while the others idle -- two rounds for the median list of 13 blocks)
    constexpr uint32_t kSpreadRounds = 3;
    const bool spread = kPerLane == 1u && complete && listed * 7u <= kSpreadRounds * kWave;
    if (spread) {
#pragma unroll
        for (uint32_t r = 0; r < kSpreadRounds; r++) {
            if (r * kWave < listed * 7u) { // (wave-uniform)
                const uint32_t t = lane + r * kWave;
                const uint32_t e = (t * 9363u) >> 16; // t / 7 for t < 448
                const uint32_t j = t - 7u * e + 1u;
                const uint32_t src = min(e, kWave - 1u);
                const int bx = __shfl(mine[0].x, (int)src), by = __shfl(mine[0].y, (int)src), bz = __shfl(mine[0].z, (int)src);
                const uint32_t home = (uint32_t)__shfl((int)slot[0], (int)src);
                if (e < listed) {
                    const int sl = Lookup::slot_find(tab, bx + (int)(j & 1u), by + (int)((j >> 1) & 1u), bz + (int)((j >> 2) & 1u));
                    tab[home * kTileSlotWords + 3u + j] = sl >= 0 ? tab[(uint32_t)sl * kTileSlotWords + 3u] : VH_FREE_ENTRY;
                }
            }
        }
    } else if (complete) {
        // pointers of the seven neighbours a sample in this block can straddle into
#pragma unroll
        for (uint32_t k = 0; k < kPerLane; k++) {
            if (lane + k * kWave < listed) {
                // the seven first probes in flight together (the slots are scattered: one probe nearly always settles it)
                int nb[8];
#pragma unroll
                for (uint32_t j = 1; j < 8u; j++) {
                    const int sl = Lookup::slot_find(tab, mine[k].x + (int)(j & 1u), mine[k].y + (int)((j >> 1) & 1u), mine[k].z + (int)((j >> 2) & 1u));
                    nb[j] = sl >= 0 ? tab[(uint32_t)sl * kTileSlotWords + 3u] : VH_FREE_ENTRY;
                }
#pragma unroll
                for (uint32_t j = 1; j < 8u; j++) tab[slot[k] * kTileSlotWords + 3u + j] = nb[j];
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();

    if (cap != 0u) {
        // With lists the splat keeps the depth range of the blocks a full list could not take (head.x, head.y); the
        // range of the listed blocks is formed here (two atomics per tile and block less).  Camera depth is linear in
        // the world position, so over a (grown) box its extremes are sums of per-axis extremes; the same margins as
        // k_interval_splat.
        {
            const float vs = hp.m_virtualVoxelSize;
            const float growLo = (GRADIENTS ? 1.75f : 1.25f) * vs, growHi = (GRADIENTS ? 0.75f : 0.25f) * vs;
            const float* vm = rp.m_viewMatrix; // camera z of a world point: row 2
            float zlo = pinf(), zhi = minf();
#pragma unroll
            for (uint32_t k = 0; k < kPerLane; k++) {
                if (lane + k * kWave < listed) {
                    const int b3[3] = { mine[k].x, mine[k].y, mine[k].z };
                    float a = vm[11], b = vm[11];
#pragma unroll
                    for (int ax = 0; ax < 3; ax++) {
                        const float lo = (float)(b3[ax] * VH_SDF_BLOCK_SIZE) * vs - growLo, hi = (float)(b3[ax] * VH_SDF_BLOCK_SIZE + VH_SDF_BLOCK_SIZE) * vs + growHi;
                        const float p = vm[8 + ax] * lo, q = vm[8 + ax] * hi;
                        a += fminf(p, q);
                        b += fmaxf(p, q);
                    }
                    const float zs = 2e-3f * fmaxf(fabsf(a), fabsf(b)) + 0.5f * vs;
                    zlo = fminf(zlo, a - zs);
                    zhi = fmaxf(zhi, b + zs);
                }
            }
            if (!complete) { // {+inf, 0} if nothing overflowed
                zlo = fminf(zlo, __uint_as_float(head.x));
                zhi = fmaxf(zhi, __uint_as_float(head.y));
            }
            // (all 64 lanes are here, those without an entry with the identity.  The clamp at 0 comes before the reduction:
            // behind it, k_render<true, true> puts one more scalar register aside)
            tileZmin = wave_min_f32(fmaxf(zlo, 0.0f)); // an empty list leaves {+inf, -inf}: nothing to march
            tileZmax = wave_max_f32(zhi);
        }
    }
    // (the same in every lane: kept in scalar registers while the rays are set up)
    tileZmin = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(tileZmin)));
    tileZmax = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(tileZmax)));
#if defined(VH_KNOCKOUT) && VH_KNOCKOUT == 41
    stamp1 = (uint32_t)__builtin_amdgcn_s_memrealtime();
#endif
    const uint32_t tileX = (tile % tilesX) * 8, tileY = (tile / tilesX) * 8; // (scalar)
    VH_STAT_DECL
    RayHit out;
    out.hit = false;
    uint32_t cost = 0u;
    if (const uint32_t x = tileX + (lane & 7), y = tileY + (lane >> 3); x < W && y < H && tileZmin <= tileZmax) { // else: no allocated block can be read by this tile's rays, every sample is invalid
        // (complete is the same for the whole wave: one of the two marches runs)
        constexpr bool kPipelined = (CAP > (uint32_t)VH_TILE_LIST_CAPACITY) || VH_PIPELINE_SMALL;
        if (complete) {
            LookupComplete lk{ tab };
            march_ray<GRADIENTS, kPipelined>(lk, hd, hp, cp, rp, x, y, tileZmin, tileZmax, half, 0.5f * (tileZmin + tileZmax), out, cost VH_STAT_ARGS);
        } else {
            Lookup lk{ tab, false, hd, hp };
            march_ray<GRADIENTS, kPipelined>(lk, hd, hp, cp, rp, x, y, tileZmin, tileZmax, half, 0.5f * (tileZmin + tileZmax), out, cost VH_STAT_ARGS);
        }
    }
    // A tile's cost is its dearest ray's.  Without gradients a split tile's is formed below, per lane over both halves, so that
    // it leaves the same class whether it was split or not.  With gradients the halves' dearest rays are added up, as they
    // always were: formed per lane, k_render<true, true> spills 16 registers more (2 352 bytes of scratch against 2 336).
    if constexpr (GRADIENTS) cost = wave_max_u32(cost); // (all 64 lanes are here: those outside the image or the interval hold 0)
    // The pixel is worked out again rather than kept: every vector register that lives across the march is one the
    // march cannot use, and at this budget one it spills.  (lane_id_again: the same number from instructions of its own.)
    const uint32_t laneAfter = lane_id_again();
    const uint32_t x = tileX + (laneAfter & 7), y = tileY + (laneAfter >> 3);
    const bool inImage = x < W && y < H;
    const size_t pix = (size_t)y * W + x;
    if (half != 0u) {
        // the far half leaves its result in its (spent) table, the near half takes it where it found nothing itself
        int* mine = tab;
        int* other = tileTab[waveInGroup ^ 1u];
        if (half == 2u) {
            mine[laneAfter * 8u + 0u] = out.hit ? 1 : 0;
            mine[laneAfter * 8u + 1u] = __float_as_int(out.alpha);
            mine[laneAfter * 8u + 2u] = (int)out.color;
            if (GRADIENTS) { mine[laneAfter * 8u + 3u] = __float_as_int(out.normal.x); mine[laneAfter * 8u + 4u] = __float_as_int(out.normal.y); mine[laneAfter * 8u + 5u] = __float_as_int(out.normal.z); }
            if constexpr (GRADIENTS) { if (laneAfter == 0) mine[64u * 8u] = (int)cost; }
            else mine[laneAfter * 8u + 6u] = (int)cost;
        }
        __syncthreads(); // all four waves of this workgroup are halves of split tiles (schedule_tiles)
        if (half == 2u) { VH_WAVE_STAMP(cost) return; }
        // a lane adds the far half's part of its ray to its own, unless the ray ended in the near half (a whole tile would not
        // have marched it further)
        if constexpr (!GRADIENTS) { if (!out.hit) cost += (uint32_t)other[laneAfter * 8u + 6u]; }
        if (!out.hit && other[laneAfter * 8u + 0u] != 0) {
            out.hit = true;
            out.alpha = __int_as_float(other[laneAfter * 8u + 1u]);
            out.color = (uint32_t)other[laneAfter * 8u + 2u];
            if (GRADIENTS) out.normal = mk3(__int_as_float(other[laneAfter * 8u + 3u]), __int_as_float(other[laneAfter * 8u + 4u]), __int_as_float(other[laneAfter * 8u + 5u]));
        }
        if constexpr (GRADIENTS) cost += (uint32_t)other[64u * 8u];
        if (laneAfter == 0) heads[tile] = make_uint4(0x7f800000u, 0u, 0u, 0u);
    }
    if (inImage) {
        store_ray(rd, cp, pix, x, y, out, GRADIENTS);
        VH_STAT_STORE
    }
    if constexpr (!GRADIENTS) cost = wave_max_u32(cost); // (all 64 lanes again; the far half of a split tile has left)
    VH_WAVE_STAMP(cost)
    if (sched && laneAfter == 0) sched[4 + tile] = min(cost / kCostClassWidth, kCostClasses - 1u); // plain store: nobody waits for it
}
#undef VH_WAVE_STAMP
#undef VH_STAT_DECL
#undef VH_STAT_ARGS
#undef VH_STAT_STORE

// Co-launch (CUDASceneRepHashSDF::integrateAhead): the workgroups behind the ray caster's own, `firstGroup` onwards,
// run the alloc pass of the NEXT frame (four 8x8 pixel tiles each), and the workgroups behind computeNormals' own run
// its compactify pass.  One launch instead of two streams: the extra workgroups are dispatched as the ray caster's
// waves retire, so they fill the tail its few dearest tiles leave, and no event or second queue is involved.  A block
// allocated while rays are marched holds only unobserved voxels (weight 0), which a sample treats exactly like an
// absent block, and the ray caster reads the table through k_interval_splat's lists, made before this launch.
struct CoAlloc {
    VhHashData hd;
    VhHashParams hp; // of the frame being allocated (its pose)
    VhDepthCameraData cam;
    VhDepthCameraParams cp;
    const uint32_t* bitMask;
    uint2* packed;
    HashMod hm;
    int32_t lockToken;
    uint32_t firstGroup; // 0: nothing to co-launch
};

VHD bool co_alloc(const CoAlloc& job, uint32_t firstGroup)
{
    if (firstGroup == 0u || blockIdx.x < firstGroup) return false;
    const uint32_t g = blockIdx.x - firstGroup;
    if (g == 0u && threadIdx.x == 0) job.hd.d_hashCompactifiedCounter[0] = 0; // as k_alloc
    alloc_tile(job.hd, job.hp, job.cam, job.cp, job.bitMask, job.lockToken, job.hm, job.packed, g * (256u / kWave) + (threadIdx.x / kWave));
    return true;
}
// alloc's workgroups as a rider (host): the ray caster's workgroups of 256, four tiles each (on its own: alloc_groups)
inline uint32_t co_alloc_groups(uint32_t tiles) { return cdiv(tiles, 256u / kWave); }

// The kernel arguments a ray-casting wave reads before it knows its tile, asked for in one go at the kernel's entry, beside
// the one that tells a rider from a ray caster: left to the compiler each is loaded where it is first used, behind the
// branch before it, and the wave waits for one after the other (entry -> image size and schedule -> phase -> heads and
// lists -> capacity).  (An empty statement that names them as scalar-register operands: they have to be there by then.)
VHD uint32_t render_start(const VhRayCastParams& rp, uint4* heads, const int4* lists, uint32_t cap, uint32_t* sched, uint32_t phase, const CoAlloc& job)
{
    uint32_t firstGroup = job.firstGroup;
    asm("" : "+s"(firstGroup) : "s"(rp.m_width), "s"(rp.m_height), "s"(heads), "s"(lists), "s"(cap), "s"(sched), "s"(phase));
    return firstGroup;
}

// small tables: all tiles of a 640x480 frame resident at once (4800 + 256 waves <= 6 x 4 x 256) -- the march is a
// latency chain, and a second round of waves costs as much as the first -- and the riders behind them find free
// slots sooner.  Six waves per SIMD (80 registers, 16 bytes of spill) measured against five (96): +1.5 % frames/s at
// 640x480, +5 % at 1920x1080; four (128 registers): -9 %.
#ifndef VH_RENDER_WAVES
#define VH_RENDER_WAVES 6
#endif
template <bool GRADIENTS, bool OFFSETS32>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(VH_RENDER_WAVES, VH_RENDER_WAVES)))
void k_render(VhHashData hd, VhHashParams hp, VhRayCastData rd, VhDepthCameraParams cp, VhRayCastParams rp,
              uint4* heads, const int4* lists, uint32_t cap, uint32_t* sched, uint32_t phase, CoAlloc job)
{
    __shared__ int tileTab[256 / kWave][2u * VH_TILE_LIST_CAPACITY * kTileSlotWords];
    if (co_alloc(job, render_start(rp, heads, lists, cap, sched, phase, job))) return;
    render_tile<GRADIENTS, VH_TILE_LIST_CAPACITY, OFFSETS32>(hd, hp, rd, cp, rp, heads, lists, cap, sched, phase, tileTab);
}

// large tables (48 KB of LDS per workgroup: three workgroups per compute unit -- three waves per SIMD, said to the compiler
// as the least it has to leave room for: 168 registers.  Without gradients the kernel takes 113 either way; with them it
// took 161 of its own accord while the SLP vectorizer ran over this unit and takes 177 without it when not told)
template <bool GRADIENTS, bool OFFSETS32>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3)))
void k_render_large(VhHashData hd, VhHashParams hp, VhRayCastData rd, VhDepthCameraParams cp, VhRayCastParams rp,
                    uint4* heads, const int4* lists, uint32_t cap, uint32_t* sched, uint32_t phase, CoAlloc job)
{
    __shared__ int tileTab[256 / kWave][2u * VH_TILE_LIST_CAPACITY_LARGE * kTileSlotWords];
    if (co_alloc(job, render_start(rp, heads, lists, cap, sched, phase, job))) return;
    render_tile<GRADIENTS, VH_TILE_LIST_CAPACITY_LARGE, OFFSETS32>(hd, hp, rd, cp, rp, heads, lists, cap, sched, phase, tileTab);
}

} // namespace

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
    if (rp->m_useGradients) VH_LAUNCH_TIMED(k_render_hash<true>, cdiv(tiles, 4), 256, (hipStream_t)stream, *hd, *hp, *rd, *cp, *rp, hm);
    else VH_LAUNCH_TIMED(k_render_hash<false>, cdiv(tiles, 4), 256, (hipStream_t)stream, *hd, *hp, *rd, *cp, *rp, hm);
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
    const size_t tiles = image_tiles(width, height);
    // header, cost classes, launch slots (one per wave: the tiles, and a second one for each split tile)
    return (4u + 4u * ((tiles + 3u) / 4u) + 2u * 4u * ((tiles + kSplitTiles + 3u) / 4u)) * sizeof(uint32_t);
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
    uint32_t groups = cdiv(tiles + (d_schedule ? split_tiles(tiles) : 0u), 4);
    // Every ray-casting wave reads its launch slot, whatever phase the schedule holds -- a stale schedule's slots are read
    // too, and only then ignored.  The size of the caller's buffer is not known here: the contract is that d_schedule holds
    // vh_render_schedule_bytes(width, height), and this keeps the grid inside that figure should either formula change.
    if (d_schedule && (size_t)(4u + 4u * cdiv(tiles, 4) + 2u * 4u * groups) * sizeof(uint32_t) > vh_render_schedule_bytes(rp->m_width, rp->m_height))
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
