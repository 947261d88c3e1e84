// vh_ray_march.hpp -- ray caster: one ray.  traverseCoarseGridSimpleSampleAll (DSC/RayCastSDFUtil.h:198-262) as
// march-until-sign-change / bisect / resume on any of the lookups (march_ray; bisect and VH_BISECT_STEP are
// findIntersectionBisection :149-170), the maps of a pixel (store_ray: renderKernel DSC/CUDARayCastSDF.cu:18-57), and the
// ray caster without intervals, k_render_hash, with its launch shape.  The VH_STAT_* macros of a -DVH_RENDER_STATS build
// are defined here and stay defined for vh_ray_tiles.hpp, their last user.
#pragma once

#include "vh_ray_sample.hpp"

namespace {
using namespace vhd;

// What a ray costs, in units of one empty-space step: a full sample (8 taps) weighs kCostSample of them.  (march_ray and
// bisect count; the tile ray caster turns the dearest ray's count into the tile's cost class, vh_frame_splat.hpp.)
constexpr uint32_t kCostSample = 6;

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
// k_render_hash's launch shape (host): workgroups of 256, a wave per tile
inline uint32_t render_hash_groups(uint32_t tiles) { return cdiv(tiles, 256u / kWave); }

} // namespace
