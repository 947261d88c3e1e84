// vh_ray_sample.hpp -- ray caster: one sample.  The eight-tap blend of trilinearInterpolationSimpleFastFast
// (DSC/RayCastSDFUtil.h:97-116) on any of the lookups, at once (trilinear) or in two steps (taps_issue, taps_finish);
// gradientForPoint (:174-195) with the reference's partial sums (trilinear_partial, gradient_for_point); and where a
// sample's taps lie: the constants of a ray or a point (RayQ, ray_setup, point_setup) and the tap coordinates (tap_coords).
#pragma once

#include "vh_ray_lookup.hpp"

namespace {
using namespace vhd;

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

// The constants of a point: a ray of direction 0, sampled at parameter 0, that must take tap_coords' exact route (the
// reference's arithmetic on the point itself).
VHD RayQ point_setup(F3 p, float voxel)
{
    RayQ rq;
    rq.cam = p; rq.dir = mk3(0.0f, 0.0f, 0.0f);
    rq.camq = rq.dirq = mk3(0.0f, 0.0f, 0.0f);
    rq.vs = voxel;
    rq.rvs = 1.0f / rq.vs;
    rq.halfVoxel = rq.vs / 2.0f;
    rq.certLim = -1.0f;
    return rq;
}

} // namespace
