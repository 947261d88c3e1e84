// vh_ray_lookup.hpp -- ray caster, first part: from a block to its voxels.  The three lookups a march is instantiated on
// (HashLookup: the hash table behind a per-ray cache, getHashEntryForSDFBlockPos DSC/VoxelUtilHashSDF.h:424-468;
// TileLookup and TileLookupComplete: a tile's own table in LDS) and the one load per voxel (load_voxel, offsets32_ok).
// The ray caster is a chain of headers, each including the one it stands on: this one, vh_ray_sample.hpp (the eight
// taps), vh_ray_march.hpp (the march, k_render_hash), and on the march vh_ray_query.hpp (the queries: the hash lookup
// alone) and vh_ray_tiles.hpp (k_render: the tile tables, the schedule of vh_frame_splat.hpp, alloc as a rider).
#pragma once

#include "vh_device.hpp"

namespace {
using namespace vhd;

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
    // the eight pointers out of a complete table: the slot of the first tap's block holds them all (both lookups)
    VHD static bool resolve_complete(const int* tab, int handle, int bxa, int bya, int bza, uint32_t straddle, int (&p)[8])
    {
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
    VHD bool resolve(int handle, int bxa, int bya, int bza, int bxb, int byb, int bzb, uint32_t straddle, int (&p)[8]) const
    {
        if (complete) return resolve_complete(tab, handle, bxa, bya, bza, straddle, p);
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
        return TileLookup<kTileTabSlots, OFFSETS32, ONE_READ>::resolve_complete(tab, handle, bxa, bya, bza, straddle, p);
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

} // namespace
