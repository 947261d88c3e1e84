// vh_frame_checks.hpp -- kernels that only tests launch: k_debug_hash_ops (the hash operations one by one) and the checks
// of the integrate pass's arithmetic (k_check_refined_division, k_check_weighted_colour), which stay with the device
// functions they check.  Included by vh_kernels.hip.
#pragma once

#include "../../include/vh_api.h"
#include "vh_device.hpp"
#include "vh_frame_integrate.hpp"

namespace {
using namespace vhd;

// ---------------------------------------------------------------------------
// the hash operations one by one, and checks of integrate's arithmetic
// ---------------------------------------------------------------------------

// serial hash-operation interpreter (tests of the collision paths)
__global__ void k_debug_hash_ops(VhHashData hd, VhHashParams hp, const int32_t* ops, int32_t* results, uint32_t n)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int32_t token = 1;
    for (uint32_t i = 0; i < n; i++) {
        const int32_t op = ops[5 * i + 0];
        const I3 p = mki3(ops[5 * i + 1], ops[5 * i + 2], ops[5 * i + 3]);
        const int32_t arg = ops[5 * i + 4];
        int32_t r = 0;
        switch (op) {
        case VH_OP_ALLOC: r = alloc_block(hd, hp, p, token); break;
        case VH_OP_DELETE: r = delete_hash_entry_element(hd, hp, p, token) ? 1 : 0; break;
        case VH_OP_INSERT: r = insert_hash_entry(hd, hp, p, arg, token) ? 1 : 0; break;
        case VH_OP_LOOKUP: r = lookup_ptr(hd, hp, p); break;
        case VH_OP_NEW_PASS: token++; break;
        default: break;
        }
        // ops are "passes" of one launch here: drop this CU's L1 so that plain loads of the next op see what the
        // atomics of this one did at L2 (between real launches the hardware does that)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");
        results[i] = r;
    }
}

// checks div_refined2 (integrate_block_certified's division) against `/` inside the ranges its callers certify:
// [0] the projection: divisor in [2^-20, 2^20], |numerator| in [2^-100, 2^60] or zero; [1] the blend: divisor an integer
// in 1..510, |numerator| in [2^-100, 2^90)
__global__ __launch_bounds__(256) void k_check_refined_division(uint32_t n, uint32_t seed, uint32_t* mismatches)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t s = (i + 1u) * 2654435761u ^ seed;
    s ^= s >> 15; s *= 2246822519u; s ^= s >> 13; s *= 3266489917u; s ^= s >> 16;
    const uint32_t u = s * 747796405u + 2891336453u, t = u * 2654435761u + 40503u;
    // sign and mantissa from the random words, exponents spread evenly over the certified ranges
    const uint32_t dExp = 127u - 20u + (s >> 8) % 41u, nExpP = 127u - 100u + (u >> 8) % 161u, nExpB = 127u - 100u + (t >> 8) % 190u;
    float d = __uint_as_float((dExp << 23) | (s & 0x7fffffu));
    if (dExp == 127u + 20u) d = 0x1p20f; // the closed end of the range
    float nP = __uint_as_float((u & 0x80000000u) | (nExpP << 23) | (u & 0x7fffffu));
    if (nExpP == 127u + 60u) nP = copysignf(0x1p60f, nP);
    if ((i & 1023u) == 0u) nP = (i & 1024u) ? 0.0f : -0.0f;
    if ((i & 1023u) == 1u) { d = 1.0f + (float)(i >> 10) * 0x1p-23f; nP = __uint_as_float(0x3fffffffu - (s & 0xffu)); } // mantissas near all-ones
    const float dB = (float)(1u + (s >> 3) % 510u);
    const float nB = __uint_as_float((t & 0x80000000u) | (nExpB << 23) | (t & 0x7fffffu));
    const f32x2 dd = (f32x2){ d, dB }, nn = (f32x2){ nP, nB };
    const f32x2 q = div_refined2(nn, dd, rcp_refined2(dd));
    const float wantP = nP / d, wantB = nB / dB;
    // (a zero numerator: the projection takes either zero -- "+ mx, + 0.5" cannot tell them apart)
    if (__float_as_uint(q.x) != __float_as_uint(wantP) && !(wantP == 0.0f && q.x == 0.0f)) atomicAdd(&mismatches[0], 1u);
    if (__float_as_uint(q.y) != __float_as_uint(wantB)) atomicAdd(&mismatches[1], 1u);
}

// weighted_colour (combine_voxel's and integrate_block_certified's colour step with m_colorIntegration = 1) against the
// integer formula floor((2 n + d) / (2 d)), n = c0 w0 + c1 w1, d = w0 + w1, for EVERY (c0, w0, c1, w1) with w1 >= 1 of one
// channel (the channels share the arithmetic; the other two carry the value's complement and its swap with c1, so a
// mix-up of bytes shows too), with each reciprocal a caller hands it: [0] 1.0f / d (combine_voxel), [1] rcp_refined2
// (the certified path).  Workgroup (c0, c1), thread w0, a loop over w1.  out: {mismatches [0], [1], first mismatch as
// c0 | w0 << 8 | c1 << 16 | w1 << 24 (the smallest such word; 0xffffffff if none), 0}
__global__ __launch_bounds__(256) void k_check_weighted_colour(uint32_t* out)
{
    const uint32_t c0 = blockIdx.x & 255u, c1 = blockIdx.x >> 8, w0 = threadIdx.x;
    uint32_t bad0 = 0u, bad1 = 0u, first = 0xffffffffu;
    for (uint32_t w1 = 1u; w1 < 256u; w1++) {
        const uint32_t d = w0 + w1;
        const uint32_t want = (2u * (c0 * w0 + c1 * w1) + d) / (2u * d);
        const uint32_t o0 = 255u - c0, o1 = 255u - c1;
        const uint32_t wantO = (2u * (o0 * w0 + o1 * w1) + d) / (2u * d), wantX = (2u * (c1 * w0 + c0 * w1) + d) / (2u * d);
        const uint32_t cw0 = pack_cw(c0, o0, c1, w0), cw1 = pack_cw(c1, o1, c0, w1), wantRgb = pack_cw(want, wantO, wantX, 0u);
        const float den = (float)d;
        const f32x2 y = rcp_refined2(both(den));
        const bool m0 = weighted_colour(cw0, cw1, den, 1.0f / den) != wantRgb, m1 = weighted_colour(cw0, cw1, den, y.x) != wantRgb;
        bad0 += m0 ? 1u : 0u;
        bad1 += m1 ? 1u : 0u;
        if (m0 || m1) first = min(first, c0 | (w0 << 8) | (c1 << 16) | (w1 << 24));
    }
    if (bad0) atomicAdd(&out[0], bad0);
    if (bad1) atomicAdd(&out[1], bad1);
    if (first != 0xffffffffu) atomicMin(&out[2], first);
}

} // namespace
