// vh_ray_tiles.hpp -- ray caster: the tile ray caster k_render / k_render_large (renderKernel DSC/CUDARayCastSDF.cu:18-57
// on the heads, lists and schedule of vh_frame_splat.hpp): a wave builds its tile's table in LDS and marches its rays on
// it (render_tile), and the workgroups behind the ray caster's own run the next frame's alloc (CoAlloc, co_alloc:
// alloc_tile of vh_frame_alloc.hpp as a rider).  The launch shape (render_groups, co_alloc_groups) stands beside them.
#pragma once

#include "vh_frame_alloc.hpp"
#include "vh_frame_splat.hpp"
#include "vh_ray_march.hpp"

namespace {
using namespace vhd;

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
        // (The slots begin behind the header and the padded cost classes: schedule_words, vh_frame_splat.hpp, defines the layout.)
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

// The ray caster's own workgroups (host), of 256: a wave per launch slot -- one per tile, and with a schedule a second one
// for each split tile.  (The riders' workgroups come behind them: co_alloc_groups.)  render_groups_most: the most a
// schedule can make it, whatever split_tiles says of the image; the schedule buffer is sized for it.
inline uint32_t render_groups(uint32_t tiles, bool scheduled) { return cdiv((uint64_t)tiles + (scheduled ? split_tiles(tiles) : 0u), 256u / kWave); }
inline uint32_t render_groups_most(uint32_t tiles) { return cdiv((uint64_t)tiles + kSplitTiles, 256u / kWave); }

} // namespace
