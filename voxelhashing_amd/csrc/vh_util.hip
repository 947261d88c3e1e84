// vh_util.hip -- what tests and benchmark launch beside the frame loop and what needs nothing of it but vh_device.hpp:
// the synthetic scene and the check of that header's exact arithmetic, with their launchers (include/vh_api.h).
// MUST be compiled with -ffp-contract=off (see vh_device.hpp).
#include <hip/hip_runtime.h>
#include <limits.h>

#include "../../include/vh_api.h"
#include "vh_device.hpp"
#include "vh_host_util.hpp"

using namespace vhd;

namespace {

struct SynthArgs {
    double spheres[4 * 8];
    int nSpheres;
    int inside;
    float T[16];
};

// analytic sphere scene in double, rounded once to float
__global__ __launch_bounds__(256) void k_synth(SynthArgs a, VhDepthCameraParams cp, float* depth, float4* color)
{
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= cp.m_imageWidth * cp.m_imageHeight) return;
    const uint32_t u = idx % cp.m_imageWidth, v = idx / cp.m_imageWidth;
    const double ox = (double)a.T[3], oy = (double)a.T[7], oz = (double)a.T[11];
    const double dx = ((double)u - (double)cp.mx) / (double)cp.fx;
    const double dy = ((double)v - (double)cp.my) / (double)cp.fy;
    const double wx = (double)a.T[0] * dx + (double)a.T[1] * dy + (double)a.T[2];
    const double wy = (double)a.T[4] * dx + (double)a.T[5] * dy + (double)a.T[6];
    const double wz = (double)a.T[8] * dx + (double)a.T[9] * dy + (double)a.T[10];
    const double aa = wx * wx + wy * wy + wz * wz;
    double bestT = 0.0;
    int best = -1;
    for (int s = 0; s < a.nSpheres; s++) {
        const double cx = a.spheres[4 * s + 0], cy = a.spheres[4 * s + 1], cz = a.spheres[4 * s + 2], r = a.spheres[4 * s + 3];
        const double ocx = ox - cx, ocy = oy - cy, ocz = oz - cz;
        const double b = ocx * wx + ocy * wy + ocz * wz;
        const double c = ocx * ocx + ocy * ocy + ocz * ocz - r * r;
        const double disc = b * b - aa * c;
        if (disc < 0.0) continue;
        const double sq = sqrt(disc);
        const double t = a.inside ? (-b + sq) / aa : (-b - sq) / aa;
        if (t > 0.0 && (best < 0 || t < bestT)) { bestT = t; best = s; }
    }
    const float mi = minf();
    if (best < 0) {
        depth[idx] = mi;
        color[idx] = make_float4(mi, mi, mi, mi);
    } else {
        const double cx = a.spheres[4 * best + 0], cy = a.spheres[4 * best + 1], cz = a.spheres[4 * best + 2], r = a.spheres[4 * best + 3];
        const double px = ox + bestT * wx, py = oy + bestT * wy, pz = oz + bestT * wz;
        double nx = (px - cx) / r, ny = (py - cy) / r, nz = (pz - cz) / r;
        if (a.inside) { nx = -nx; ny = -ny; nz = -nz; }
        depth[idx] = (float)bestT;
        color[idx] = make_float4((float)(0.5 + 0.5 * nx), (float)(0.5 + 0.5 * ny), (float)(0.5 + 0.5 * nz), 1.0f);
    }
}

// the reference's own expressions (worldToVirtualVoxelPos, virtualVoxelPosToSDFBlock, DSC/VoxelUtilHashSDF.h:266-282) as
// they were written before round_half_away and the shift of vvp_to_block1: what k_check_fast_math holds those against
__device__ int round_by_sign(float p) { return f2i(p + (float)signi(p) * 0.5f); }
__device__ int block_by_division(int v)
{
    if (v < 0) v -= VH_SDF_BLOCK_SIZE - 1;
    return v / VH_SDF_BLOCK_SIZE;
}

// checks div_exact against `/`, round_half_away and vvp_to_block1 against the reference's expressions (word 0) and umod_fast
// against `%` (word 1) on pseudo-random operands
__global__ __launch_bounds__(256) void k_check_fast_math(float b, HashMod hm, uint32_t n, uint32_t seed, uint32_t* mismatches)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // xorshift-multiply scramble of (seed, i)
    uint32_t s = (i + 1u) * 2654435761u ^ seed;
    s ^= s >> 15; s *= 2246822519u; s ^= s >> 13; s *= 3266489917u; s ^= s >> 16;
    uint32_t u = s * 747796405u + 2891336453u;
    // dividend: mostly scene-scale positions, some raw bit patterns (any finite magnitude)
    float a;
    if ((i & 7u) == 7u) {
        a = __uint_as_float(u);
        const uint32_t ex = (u >> 23) & 0xffu;
        if (ex == 0xffu || ex < 0x10u || ex > 0xe8u) a = (float)(int)u * 1.0e-6f; // keep a and a/b normal
    } else {
        a = ((float)(int)u) * (1.0f / 2147483648.0f) * (((i >> 3) & 1u) ? 400.0f : 8.0f);
    }
    const float rb = 1.0f / b;
    const float q0 = a / b, q1 = div_exact(a, b, rb);
    if (__float_as_uint(q0) != __float_as_uint(q1) && !(q0 == 0.0f && q1 == 0.0f)) atomicAdd(&mismatches[0], 1u);
    // the quotient rounded to a voxel, the voxel's block, and the block of any 32-bit pattern (but the seven lowest,
    // where the reference's v - 7 overflows: of the voxels that is INT_MIN, what a quotient below -2^31 saturates to)
    const int v0 = round_by_sign(q0), v1 = round_half_away(q0);
    if (v0 != v1) atomicAdd(&mismatches[0], 1u);
    if (v0 > INT_MIN + 6 && block_by_division(v0) != vvp_to_block1(v0)) atomicAdd(&mismatches[0], 1u);
    if ((int)u > INT_MIN + 6 && block_by_division((int)u) != vvp_to_block1((int)u)) atomicAdd(&mismatches[0], 1u);
    if ((s % hm.d) != umod_fast(s, hm)) atomicAdd(&mismatches[1], 1u);
    if ((u % hm.d) != umod_fast(u, hm)) atomicAdd(&mismatches[1], 1u);
    if (i < 256u) { // every colour byte over 255 (store_ray)
        const float c = (float)i;
        if (__float_as_uint(c / 255.f) != __float_as_uint(div_exact(c, 255.0f, 1.0f / 255.0f))) atomicAdd(&mismatches[0], 1u);
    }
    if (i < 16u) { // the quotients where the sign is 0, the halves, and what the conversion saturates or sends to 0
        const uint32_t special[8] = { 0x00000000u, 0x3effffffu, 0x3f000000u, 0x3f000001u, 0x00000001u, 0x4f000000u, 0x7f800000u, 0x7fc00000u };
        const float p = __uint_as_float(special[i & 7u] | ((i & 8u) << 28));
        if (round_by_sign(p) != round_half_away(p)) atomicAdd(&mismatches[0], 1u);
    }
    if (i < 64u) { // extremes of the unsigned range
        const uint32_t e = 0xffffffffu - i;
        if ((e % hm.d) != umod_fast(e, hm)) atomicAdd(&mismatches[1], 1u);
        if ((i % hm.d) != umod_fast(i, hm)) atomicAdd(&mismatches[1], 1u);
    }
}

// the wave reductions of vh_device.hpp on one wave's 64 words: what each lane got back from each helper
__global__ __launch_bounds__(64) void k_wave_reduce(const uint32_t* __restrict__ in, uint32_t* __restrict__ out)
{
    const uint32_t lane = lane_id();
    const uint32_t w = in[lane];
    out[lane] = __float_as_uint(wave_min_f32(__uint_as_float(w)));
    out[kWave + lane] = __float_as_uint(wave_max_f32(__uint_as_float(w)));
    out[2 * kWave + lane] = wave_max_u32(w);
}

} // namespace

extern "C" {

int vh_synth_frame(const double* h_spheres, int nSpheres, int inside, const float camToWorld[16],
                   const VhDepthCameraParams* cp, float* d_depth, float* d_color4, vhStream_t stream)
{
    if (!h_spheres || !camToWorld || !cp || !d_depth || !d_color4 || nSpheres < 0 || nSpheres > 8) return VH_ERR_BAD_ARGUMENT;
    SynthArgs a;
    for (int i = 0; i < 4 * nSpheres; i++) a.spheres[i] = h_spheres[i];
    a.nSpheres = nSpheres;
    a.inside = inside;
    for (int i = 0; i < 16; i++) a.T[i] = camToWorld[i];
    const uint64_t n = (uint64_t)cp->m_imageWidth * cp->m_imageHeight;
    if (n == 0) return VH_OK;
    k_synth<<<cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(a, *cp, d_depth, reinterpret_cast<float4*>(d_color4));
    return vh_last_launch_error();
}

int vh_debug_check_fast_math(float divisor, uint32_t modulus, uint32_t n, uint32_t seed, uint32_t* d_mismatches, vhStream_t stream)
{
    if (!d_mismatches || modulus < 2 || !(divisor > 0.0f)) return VH_ERR_BAD_ARGUMENT;
    VH_HIP(hipMemsetAsync(d_mismatches, 0, 2 * sizeof(uint32_t), (hipStream_t)stream));
    if (n == 0) return VH_OK;
    k_check_fast_math<<<cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(divisor, make_hash_mod(modulus), n, seed, d_mismatches);
    return vh_last_launch_error();
}

int vh_debug_wave_reduce(const uint32_t* d_in64, uint32_t* d_out192, vhStream_t stream)
{
    if (!d_in64 || !d_out192) return VH_ERR_BAD_ARGUMENT;
    k_wave_reduce<<<1, kWave, 0, (hipStream_t)stream>>>(d_in64, d_out192);
    return vh_last_launch_error();
}

} // extern "C"
