// vh_resample_blend.hpp -- what the resampled merge (vh_resample.hip) and the scene registration (vh_align.hip) share:
// the position of a voxel of one lattice in another's voxel index space, the range of such positions over a box, the
// eight-tap blend of a scene at such a position, and the two float32 voxel matrices of a rigid transform.  Written once,
// so that the registration samples exactly the field the merge would write.  Float arithmetic held bit for bit: every
// unit that includes this MUST be compiled with -ffp-contract=off.
#pragma once

#include "vh_device.hpp"

namespace vhd {

constexpr int kMostReach = 5;          // blocks per axis the taps of one block's voxels reach in the other lattice (ratio 1/2)
constexpr float kMostCoord = 16777216.0f;

struct M34 { float m[12]; }; // row-major 3x4, voxel index space

// one row of the rule's position: ((m0 i + m1 j) + m2 k) + m3, one rounding per operation.  Every operation is monotone
// in its arguments, so the row is monotone in each of i, j, k: over a box of voxels it takes its least and its greatest
// value at corners of the box, in float as in exact arithmetic.
VHD float row(const float* r, float i, float j, float k) { return ((r[0] * i + r[1] * j) + r[2] * k) + r[3]; }

// the least and the greatest of a row over the eight corners of the box [lo, hi]^3 of voxel coordinates
VHD void row_range(const float* r, const float* lo, const float* hi, float& least, float& most)
{
    least = pinf();
    most = minf();
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const float q = row(r, (c & 1) ? hi[0] : lo[0], (c & 2) ? hi[1] : lo[1], (c & 4) ? hi[2] : lo[2]);
        least = fminf(least, q);
        most = fmaxf(most, q);
    }
}

// The eight-tap blend of a scene at the position (qx, qy, qz) of its voxel index space, every |q| at most 2^24.  s_ptr:
// the pointers of the scene's blocks [loB, loB + dim) the workgroup resolved.  A tap with a zero weight factor is not
// read; the sums start from the first product.  All zero unless every used tap is observed (a result's weight is at
// least 1 then).  The eight loads are issued before the first is used.
VHD uint2 blend_taps(const VhVoxel* __restrict__ pool, const int* s_ptr, I3 loB, I3 dim, float qx, float qy, float qz)
{
    const float bx = floorf(qx), by = floorf(qy), bz = floorf(qz);
    const float fx = qx - bx, fy = qy - by, fz = qz - bz;
    const float gx = 1.0f - fx, gy = 1.0f - fy, gz = 1.0f - fz;
    const int ix = (int)bx, iy = (int)by, iz = (int)bz;
    float wt[8];
    uint2 v[8];
#pragma unroll
    for (int t = 0; t < 8; t++) {
        wt[t] = (((t & 1) ? fx : gx) * ((t & 2) ? fy : gy)) * ((t & 4) ? fz : gz);
        v[t] = make_uint2(0u, 0u); // (a tap in a block the source does not hold reads as unobserved)
        if (wt[t] != 0.0f) {
            const int vx = ix + (t & 1), vy = iy + ((t >> 1) & 1), vz = iz + ((t >> 2) & 1);
            const int tx = (vx >> 3) - loB.x, ty = (vy >> 3) - loB.y, tz = (vz >> 3) - loB.z;
            int ptr = VH_FREE_ENTRY;
            if ((uint32_t)tx < (uint32_t)dim.x && (uint32_t)ty < (uint32_t)dim.y && (uint32_t)tz < (uint32_t)dim.z) ptr = s_ptr[(tz * dim.y + ty) * dim.x + tx];
            if (ptr != VH_FREE_ENTRY)
                v[t] = *reinterpret_cast<const uint2*>(&pool[(uint32_t)ptr + (uint32_t)(((vz & 7) * 8 + (vy & 7)) * 8 + (vx & 7))]);
        }
    }
    bool first = true, ok = true;
    float sdf = 0.0f, cr = 0.0f, cg = 0.0f, cb = 0.0f;
    uint32_t weight = 255u;
#pragma unroll
    for (int t = 0; t < 8; t++) {
        if (wt[t] != 0.0f) {
            const uint32_t cw = v[t].y;
            ok = ok && (cw >> 24) != 0u;
            weight = min(weight, cw >> 24);
            const float ps = wt[t] * __uint_as_float(v[t].x);
            const float pr = wt[t] * (float)(cw & 0xffu), pg = wt[t] * (float)((cw >> 8) & 0xffu), pb = wt[t] * (float)((cw >> 16) & 0xffu);
            // from the first product, not from 0: -0 stays -0
            sdf = first ? ps : sdf + ps;
            cr = first ? pr : cr + pr;
            cg = first ? pg : cg + pg;
            cb = first ? pb : cb + pb;
            first = false;
        }
    }
    if (!ok || first) return make_uint2(0u, 0u);
    const uint32_t r = (uint32_t)min(255, f2i(cr + 0.5f)), g = (uint32_t)min(255, f2i(cg + 0.5f)), bl = (uint32_t)min(255, f2i(cb + 0.5f));
    return make_uint2(__float_as_uint(sdf), pack_cw(r, g, bl, weight));
}

// The two voxel matrices of dstFromSrc = [R | t] (metres; T row-major 4x4, s and d the two voxel sizes): in double,
// rounded once.  On the host and on the device, the same operations in the same order.
__host__ __device__ inline void voxel_matrices(const double* T, double s, double d, float* srcVoxFromDstVox, float* dstVoxFromSrcVox)
{
    double R[3][3], t[3];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) R[r][c] = T[4 * r + c];
        t[r] = T[4 * r + 3];
    }
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) {
            srcVoxFromDstVox[4 * r + c] = (float)(R[c][r] * (d / s));
            dstVoxFromSrcVox[4 * r + c] = (float)(R[r][c] * (s / d));
        }
        srcVoxFromDstVox[4 * r + 3] = (float)(-((R[0][r] * t[0] + R[1][r] * t[1]) + R[2][r] * t[2]) / s);
        dstVoxFromSrcVox[4 * r + 3] = (float)(t[r] / d);
    }
}

} // namespace vhd
