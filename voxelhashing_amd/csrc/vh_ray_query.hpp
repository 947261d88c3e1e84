// vh_ray_query.hpp -- the batch queries k_query_points and k_query_rays (not in the reference; they answer to its
// trilinearInterpolationSimpleFastFast, gradientForPoint and traverseCoarseGridSimpleSampleAll, DSC/RayCastSDFUtil.h).
// Of the ray caster they use the hash lookup, the sample and bisect: no tile table, no schedule, no rider.
#pragma once

#include "vh_ray_march.hpp"

namespace {
using namespace vhd;

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
        const RayQ rq = point_setup(p, hp.m_virtualVoxelSize);
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

} // namespace
