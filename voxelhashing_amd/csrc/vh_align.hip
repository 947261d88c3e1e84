// vh_align.hip -- scene registration: the rigid motion that lays one scene onto another, found on the device by direct
// SDF-to-SDF Gauss-Newton (not in the reference; DESIGN.md section 4 "Scene registration" has the definition, the
// derivation of the fixed-point quantum and the limits).  Every near-surface observed voxel of the source goes through
// the current estimate into the destination, whose field and central-difference gradient are sampled there by the
// blend of the resampled merge (vh_resample_blend.hpp); each voxel adds one row of a 6-parameter least-squares problem
// as 29 terms in 64-bit fixed point, so the totals are the same to the bit whatever order the adds ran in.  The wave
// that draws the last ticket solves (vh_solve_6x6.hpp) and moves the estimate, which lives in a VhAlignState on the
// device.  Neither scene is written.  Three kernels -- the step, the rule alone for tests, the box of a block list --
// and their launcher-level C ABI (include/vh_api.h).  A unit of its own so that nothing is compiled beside k_render
// (DESIGN.md section 7 item 1); the rule is float arithmetic held bit for bit: MUST be compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>

#include "../../include/vh_api.h"
#include "vh_device.hpp"
#include "vh_host_util.hpp"
#include "vh_resample_blend.hpp"
#include "vh_solve_6x6.hpp"

using namespace vhd;

namespace {

constexpr int kBlockLimit = 1 << 20; // block coordinates in [-2^20, 2^20), as the resampled merge
constexpr uint32_t kTerms = VH_ALIGN_NUM_TERMS;
constexpr uint32_t kStripeWords = 32; // 29 totals in 256 bytes: a stripe has two cache lines to itself
constexpr float kQuantumInv = (float)(1u << VH_ALIGN_QUANTUM_LOG2);
constexpr float kMostGradient = 2.0f;

struct AlignArgs {
    float bandS, bandD; // band * vsSrc, band * vsDst: one float product each
    float vsD;
    float condThres;
    uint32_t minCount;
    double rotThres, transThres;
};

struct Rule {
    float q[3], e, g[3];
};

// The rule for one source voxel (include/vh_api.h): false when it is dropped.  s_ptr: the destination's blocks
// [loB, loB + dim) the workgroup resolved.  The six gradient samples are taken only where the centre passed its gates.
VHD bool align_voxel(uint2 src, const VhVoxel* __restrict__ pool, const int* s_ptr, I3 loB, I3 dim, const float* m, const float* pivot, float invRadius,
                     float bandS, float bandD, float vsD, float i, float j, float k, Rule& r, float (&t)[kTerms])
{
    const float s = __uint_as_float(src.x);
    if ((src.y >> 24) == 0u || !(fabsf(s) <= bandS)) return false;
    const float qx = row(&m[0], i, j, k), qy = row(&m[4], i, j, k), qz = row(&m[8], i, j, k);
    if (!(fabsf(qx) < kMostCoord) || !(fabsf(qy) < kMostCoord) || !(fabsf(qz) < kMostCoord)) return false;
    const float ux = (qx - pivot[0]) * invRadius, uy = (qy - pivot[1]) * invRadius, uz = (qz - pivot[2]) * invRadius;
    if (!(fabsf(ux) <= 1.0f) || !(fabsf(uy) <= 1.0f) || !(fabsf(uz) <= 1.0f)) return false;
    const uint2 c = blend_taps(pool, s_ptr, loB, dim, qx, qy, qz);
    const float phi = __uint_as_float(c.x);
    if ((c.y >> 24) == 0u || !(fabsf(phi) <= bandD)) return false;
    const uint2 xp = blend_taps(pool, s_ptr, loB, dim, qx + 0.5f, qy, qz), xm = blend_taps(pool, s_ptr, loB, dim, qx - 0.5f, qy, qz);
    const uint2 yp = blend_taps(pool, s_ptr, loB, dim, qx, qy + 0.5f, qz), ym = blend_taps(pool, s_ptr, loB, dim, qx, qy - 0.5f, qz);
    const uint2 zp = blend_taps(pool, s_ptr, loB, dim, qx, qy, qz + 0.5f), zm = blend_taps(pool, s_ptr, loB, dim, qx, qy, qz - 0.5f);
    if (((xp.y >> 24) == 0u) | ((xm.y >> 24) == 0u) | ((yp.y >> 24) == 0u) | ((ym.y >> 24) == 0u) | ((zp.y >> 24) == 0u) | ((zm.y >> 24) == 0u)) return false;
    const float e = (phi - s) / vsD;
    const float gx = (__uint_as_float(xp.x) - __uint_as_float(xm.x)) / vsD;
    const float gy = (__uint_as_float(yp.x) - __uint_as_float(ym.x)) / vsD;
    const float gz = (__uint_as_float(zp.x) - __uint_as_float(zm.x)) / vsD;
    if (!(fabsf(gx) <= kMostGradient) || !(fabsf(gy) <= kMostGradient) || !(fabsf(gz) <= kMostGradient)) return false;
    const float J[6] = { uy * gz - uz * gy, uz * gx - ux * gz, ux * gy - uy * gx, gx, gy, gz };
    uint32_t at = 0u;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = a; b < 6; b++) t[at++] = J[a] * J[b];
#pragma unroll
    for (int a = 0; a < 6; a++) t[VH_ALIGN_JTE + a] = J[a] * e;
    t[VH_ALIGN_EE] = e * e;
    t[VH_ALIGN_COUNT] = 1.0f;
    r.q[0] = qx; r.q[1] = qy; r.q[2] = qz;
    r.e = e;
    r.g[0] = gx; r.g[1] = gy; r.g[2] = gz;
    return true;
}

// a term in fixed point: the scaling by 2^26 is exact (|term| < 2^8, and the float's small end only gains), the
// conversion rounds to nearest, ties to even
VHD long long to_fixed(float term) { return __float2ll_rn(term * kQuantumInv); }

VHD bool block_in_range(I3 p)
{
    return p.x >= -kBlockLimit && p.x < kBlockLimit && p.y >= -kBlockLimit && p.y < kBlockLimit && p.z >= -kBlockLimit && p.z < kBlockLimit;
}

// The destination blocks that the samples of source block `pos` can reach, resolved into s_ptr by the whole workgroup
// (one lookup_ptr per block, none per tap); false when the block is out of range or reaches too far (uniform).
// The range is exact: by the monotonicity of row(), every voxel's q lies between the least and the greatest q of the
// box's corners, computed by the same operations; q - 0.5f and q + 0.5f are monotone in q too, so every tap of the
// seven samples lies in [floor(least - 0.5f), floor(most + 0.5f) + 1].  The corners' q differ by at most 7 * sum_c
// |m_rc| <= 7 * sqrt(3) * vsSrc / vsDst <= 24.3 per axis (ratio 2), with the half voxels 25.3: the two ends differ by
// at most 27, and an interval of L + 1 integers meets at most floor(L / 8) + 2 blocks: kMostReach = 5 per axis.
VHD bool resolve_reach(const VhHashData& hd, const VhHashParams& hp, I3 pos, const float* m, int* s_ptr, I3& loB, I3& dim, bool& any)
{
    any = false;
    if (!block_in_range(pos)) return false;
    const float bl[3] = { (float)(8 * pos.x), (float)(8 * pos.y), (float)(8 * pos.z) };
    const float bh[3] = { bl[0] + 7.0f, bl[1] + 7.0f, bl[2] + 7.0f };
    int l[3], d[3];
    bool fits = true;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        float least, most;
        row_range(&m[4 * r], bl, bh, least, most);
        // voxels whose q is not below 2^24 are dropped whatever the destination holds: the range need not cover them
        least = fminf(fmaxf(least, -kMostCoord), kMostCoord);
        most = fminf(fmaxf(most, -kMostCoord), kMostCoord);
        l[r] = (int)floorf(least - 0.5f) >> 3;
        d[r] = (((int)floorf(most + 0.5f) + 1) >> 3) - l[r] + 1;
        fits = fits && d[r] >= 1 && d[r] <= kMostReach; // (a NaN in the matrix gives no range at all)
    }
    if (!fits) return false;
    loB = mki3(l[0], l[1], l[2]);
    dim = mki3(d[0], d[1], d[2]);
    const uint32_t t = threadIdx.x;
    int ptr = VH_FREE_ENTRY;
    if (t < (uint32_t)(dim.x * dim.y * dim.z)) {
        ptr = lookup_ptr(hd, hp, mki3(loB.x + (int)(t % (uint32_t)dim.x), loB.y + (int)((t / (uint32_t)dim.x) % (uint32_t)dim.y), loB.z + (int)(t / (uint32_t)(dim.x * dim.y))));
        s_ptr[t] = ptr;
    }
    any = __syncthreads_or(ptr != VH_FREE_ENTRY) != 0;
    return true;
}

VHD long long wave_sum_i64(long long v)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Rodrigues' exponential of w (radians) in double: R = I + a K + b K K, a = sin(th) / th, b = 2 sin^2(th / 2) / th^2
VHD void rodrigues(const double* w, double* R)
{
    const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const double th = sqrt(th2);
    double a = 1.0, b = 0.5;
    if (th > 1e-8) {
        const double sh = sin(0.5 * th);
        a = sin(th) / th;
        b = 2.0 * (sh * sh) / th2;
    }
    const double K[9] = { 0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0 };
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            const double kk = (K[3 * r] * K[c] + K[3 * r + 1] * K[3 + c]) + K[3 * r + 2] * K[6 + c];
            R[3 * r + c] = ((r == c ? 1.0 : 0.0) + a * K[3 * r + c]) + b * kk;
        }
}

// What the last arriver does with the totals (include/vh_api.h has the step).  One lane.
VHD void align_take_step(VhAlignState* st, const long long (&tot)[kTerms], uint32_t raised, const AlignArgs& args)
{
    const uint32_t it = st->iterations;
    const double scale = 1.0 / (double)(1u << VH_ALIGN_QUANTUM_LOG2);
    double A[6][6], b[6], y[6];
    uint32_t at = 0u;
    for (int r = 0; r < 6; r++) {
        for (int c = r; c < 6; c++) A[r][c] = A[c][r] = (double)tot[at++] * scale;
        b[r] = -((double)tot[VH_ALIGN_JTE + r] * scale);
    }
    for (uint32_t k = 0; k < kTerms; k++) st->totals[k] = tot[k];
    const uint32_t count = (uint32_t)(tot[VH_ALIGN_COUNT] >> VH_ALIGN_QUANTUM_LOG2);
    st->count[it] = count;
    st->sumSquares[it] = (double)tot[VH_ALIGN_EE] * scale;
    st->condition[it] = 0.0f;
    st->stepRotation[it] = 0.0;
    st->stepTranslation[it] = 0.0;
    st->iterations = it + 1u;
    uint32_t status = raised;
    if (it + 1u == VH_ALIGN_MAX_ITERATIONS) status |= VH_ALIGN_ITERATIONS_SPENT;
    if (raised != 0u) { st->status = status; return; }
    if (count < args.minCount) { st->status = status | VH_ALIGN_TOO_FEW; return; }
    const float cond = icp_solve_6x6(A, b, y);
    st->condition[it] = cond;
    if (!(cond <= args.condThres)) { st->status = status | VH_ALIGN_ILL_CONDITIONED; return; }
    const double inv = (double)st->invRadius, vsD = (double)st->vsDst;
    const double w[3] = { y[0] * inv, y[1] * inv, y[2] * inv };
    const double p[3] = { (double)st->pivot[0], (double)st->pivot[1], (double)st->pivot[2] };
    double R[9];
    rodrigues(w, R);
    // q -> p + R (q - p) + tau in the destination's voxels; in metres the same rotation and (p - R p + tau) vsDst
    double S[12];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) S[4 * r + c] = R[3 * r + c];
        S[4 * r + 3] = ((p[r] - ((R[3 * r] * p[0] + R[3 * r + 1] * p[1]) + R[3 * r + 2] * p[2])) + y[3 + r]) * vsD;
    }
    double T[16];
    for (int k = 0; k < 16; k++) T[k] = st->dstFromSrc[k];
    double N[16];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) {
            const double v = (S[4 * r] * T[c] + S[4 * r + 1] * T[4 + c]) + S[4 * r + 2] * T[8 + c];
            N[4 * r + c] = c == 3 ? v + S[4 * r + 3] : v;
        }
    N[12] = 0.0; N[13] = 0.0; N[14] = 0.0; N[15] = 1.0;
    for (int k = 0; k < 16; k++) st->dstFromSrc[k] = N[k];
    float ma[12], mb[12];
    voxel_matrices(N, (double)st->vsSrc, vsD, ma, mb);
    for (int k = 0; k < 12; k++) { st->srcVoxFromDstVox[k] = ma[k]; st->dstVoxFromSrcVox[k] = mb[k]; }
    const double rot = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    const double trans = sqrt((y[3] * y[3] + y[4] * y[4]) + y[5] * y[5]);
    st->stepRotation[it] = rot;
    st->stepTranslation[it] = trans;
    if (rot < args.rotThres && trans < args.transThres) status |= VH_ALIGN_CONVERGED;
    st->status = status;
}

// The hot path: one workgroup of 256 per listed source block, one 16-byte pair of voxels per lane (voxels 2t and 2t + 1
// of the block: neighbours in x), as k_resample_blocks.  A block whose voxels contribute nothing goes straight to the
// ticket: no reduction, no add, no fence.  The others reduce their 29 fixed-point terms in the wave (shuffles), across
// the four waves through LDS, and lanes 0..28 add the block's sums to the stripe the block's index picks: one 232-byte
// wave-instruction of 64-bit integer adds.  The hand-off is icp_hand_off's (vh_icp.hip), for a workgroup of four
// waves of which the first goes on: the adds have left the wave (vmcnt(0)), the agent-scope release makes them visible
// to every XCD, then the ticket is drawn, a relaxed agent-scope add; the wave that reads gridDim.x - 1 takes an
// agent-scope acquire, leaves the ticket 0, sums the stripes, clears them for the next launch and takes the step.  Every
// workgroup has read what it needs of the state before its ticket is drawn, and only the last arriver writes the state.
// No loop's length depends on data.
__global__ __launch_bounds__(256) void k_align_step(VhHashData dstHd, VhHashParams dstHp, const VhVoxel* __restrict__ srcPool, uint32_t n,
                                                    const VhSDFBlockDesc* __restrict__ descs, AlignArgs args, VhAlignState* st, uint32_t* ticket)
{
    __shared__ int s_ptr[kMostReach * kMostReach * kMostReach];
    __shared__ long long s_part[256 / kWave][kTerms];
    __shared__ uint32_t s_has[256 / kWave];
    const uint32_t b = blockIdx.x, t = threadIdx.x, lane = lane_id(), wave = t / kWave;
    if (st->status != 0u || st->iterations >= VH_ALIGN_MAX_ITERATIONS) return; // (uniform in the grid: the state is written after the last ticket)
    float m[12], pivot[3];
#pragma unroll
    for (int k = 0; k < 12; k++) m[k] = st->dstVoxFromSrcVox[k];
#pragma unroll
    for (int k = 0; k < 3; k++) pivot[k] = st->pivot[k];
    const float invRadius = st->invRadius;

    bool wrote = false;
    if (b < n) { // (uniform in the workgroup, as every branch around a barrier below)
        const int4 d = *reinterpret_cast<const int4*>(&descs[b]);
        const I3 pos = mki3(__builtin_amdgcn_readfirstlane(d.x), __builtin_amdgcn_readfirstlane(d.y), __builtin_amdgcn_readfirstlane(d.z));
        const int ptr = __builtin_amdgcn_readfirstlane(d.w);
        I3 loB = mki3(0, 0, 0), dim = mki3(0, 0, 0);
        bool any = false;
        if (!resolve_reach(dstHd, dstHp, pos, m, s_ptr, loB, dim, any)) {
            if (t == 0u) {
                __hip_atomic_fetch_or(&st->raised, VH_ALIGN_OUT_OF_RANGE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                wrote = true;
            }
        } else if (any) { // (else the destination holds nothing here: an empty block)
            const uint4 raw = reinterpret_cast<const uint4*>(srcPool + (uint32_t)ptr)[t];
            const float i = (float)(8 * pos.x) + (float)((2u * t) & 7u), j = (float)(8 * pos.y) + (float)((t >> 2) & 7u), k = (float)(8 * pos.z) + (float)(t >> 5);
            long long acc[kTerms];
#pragma unroll
            for (uint32_t a = 0; a < kTerms; a++) acc[a] = 0;
            bool kept = false;
#pragma unroll 1
            for (int v = 0; v < 2; v++) {
                Rule r;
                float terms[kTerms];
                const uint2 src = v == 0 ? make_uint2(raw.x, raw.y) : make_uint2(raw.z, raw.w);
                if (align_voxel(src, dstHd.d_SDFBlocks, s_ptr, loB, dim, m, pivot, invRadius, args.bandS, args.bandD, args.vsD, i + (float)v, j, k, r, terms)) {
                    kept = true;
#pragma unroll
                    for (uint32_t a = 0; a < kTerms; a++) acc[a] += to_fixed(terms[a]);
                }
            }
            if (__syncthreads_or(kept) != 0) {
                const bool has = __ballot(kept) != 0ull; // (uniform in the wave)
                if (has) {
#pragma unroll
                    for (uint32_t a = 0; a < kTerms; a++) {
                        const long long sum = wave_sum_i64(acc[a]);
                        if (lane == 0u) s_part[wave][a] = sum;
                    }
                }
                if (lane == 0u) s_has[wave] = has ? 1u : 0u;
                __syncthreads();
                if (t < kTerms) {
                    long long sum = 0;
#pragma unroll
                    for (uint32_t w = 0; w < 256 / kWave; w++)
                        if (s_has[w] != 0u) sum += s_part[w][t];
                    __hip_atomic_fetch_add(&st->stripes[(b % VH_ALIGN_NUM_STRIPES) * kStripeWords + t], sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    wrote = true;
                }
            }
        }
    }
    if (wave != 0u) return; // (no barrier below)

    uint32_t drawn = 0u;
    if (__ballot(wrote) != 0ull) { // (uniform in the wave)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    if (lane == 0u) drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    drawn = (uint32_t)__shfl((int)drawn, 0);
    if (drawn != gridDim.x - 1u) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0u) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    long long total = 0;
    if (lane < kTerms) {
#pragma unroll 8
        for (uint32_t s = 0; s < VH_ALIGN_NUM_STRIPES; s++) {
            long long* at = &st->stripes[s * kStripeWords + lane];
            total += __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(at, 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    long long tot[kTerms];
#pragma unroll
    for (uint32_t a = 0; a < kTerms; a++) tot[a] = __shfl(total, (int)a);
    if (lane != 0u) return;
    const uint32_t raised = __hip_atomic_load(&st->raised, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&st->raised, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    align_take_step(st, tot, raised, args);
}

// the rule alone: a record of 37 words per voxel of every listed block (include/vh_api.h)
__global__ __launch_bounds__(256) void k_align_rule(VhHashData dstHd, VhHashParams dstHp, const VhVoxel* __restrict__ srcPool, uint32_t n,
                                                    const VhSDFBlockDesc* __restrict__ descs, M34 m, float px, float py, float pz, float invRadius, float bandS,
                                                    float bandD, float vsD, float* __restrict__ out)
{
    __shared__ int s_ptr[kMostReach * kMostReach * kMostReach];
    const uint32_t b = blockIdx.x, t = threadIdx.x;
    if (b >= n) return;
    const I3 pos = mki3(descs[b].pos[0], descs[b].pos[1], descs[b].pos[2]);
    const float pivot[3] = { px, py, pz };
    I3 loB = mki3(0, 0, 0), dim = mki3(0, 0, 0);
    bool any = false;
    const bool fits = resolve_reach(dstHd, dstHp, pos, m.m, s_ptr, loB, dim, any);
    const uint4 raw = reinterpret_cast<const uint4*>(srcPool + (uint32_t)descs[b].ptr)[t];
    const float i = (float)(8 * pos.x) + (float)((2u * t) & 7u), j = (float)(8 * pos.y) + (float)((t >> 2) & 7u), k = (float)(8 * pos.z) + (float)(t >> 5);
#pragma unroll 1
    for (int v = 0; v < 2; v++) {
        Rule r;
        float terms[kTerms];
        const uint2 src = v == 0 ? make_uint2(raw.x, raw.y) : make_uint2(raw.z, raw.w);
        const bool kept = fits && any && align_voxel(src, dstHd.d_SDFBlocks, s_ptr, loB, dim, m.m, pivot, invRadius, bandS, bandD, vsD, i + (float)v, j, k, r, terms);
        float* o = out + ((size_t)b * VH_SDF_BLOCK_VOXELS + 2u * t + (uint32_t)v) * 37u;
        o[0] = __uint_as_float(kept ? 1u : 0u);
        o[1] = kept ? r.q[0] : 0.0f; o[2] = kept ? r.q[1] : 0.0f; o[3] = kept ? r.q[2] : 0.0f;
        o[4] = kept ? r.e : 0.0f;
        o[5] = kept ? r.g[0] : 0.0f; o[6] = kept ? r.g[1] : 0.0f; o[7] = kept ? r.g[2] : 0.0f;
#pragma unroll
        for (uint32_t a = 0; a < kTerms; a++) o[8u + a] = kept ? terms[a] : 0.0f;
    }
}

// the box of a block list: a wave's least and greatest, then one atomic per wave and word
__global__ __launch_bounds__(256) void k_align_bounds(uint32_t n, const VhSDFBlockDesc* __restrict__ descs, const uint32_t* count, int* box)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (count) n = min(n, *count);
    int lo[3] = { INT_MAX, INT_MAX, INT_MAX }, hi[3] = { INT_MIN, INT_MIN, INT_MIN };
    if (i < n) {
#pragma unroll
        for (int c = 0; c < 3; c++) lo[c] = hi[c] = descs[i].pos[c];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
            lo[c] = min(lo[c], __shfl_xor(lo[c], o));
            hi[c] = max(hi[c], __shfl_xor(hi[c], o));
        }
        if (lane_id() == 0u && lo[c] <= hi[c]) {
            atomicMin(&box[c], lo[c]);
            atomicMax(&box[3 + c], hi[c]);
        }
    }
}

__global__ void k_align_raise(VhAlignState* st, uint32_t bits)
{
    if (threadIdx.x == 0u && st->status == 0u) st->status = bits;
}

bool power_of_two(float v)
{
    int e = 0;
    return std::isfinite(v) && v > 0.0f && std::frexp(v, &e) == 0.5f;
}

} // namespace

extern "C" {

int vh_align_begin(VhAlignState* d_state, const double* guess, float vsSrc, float vsDst, const float pivot3[3], float radius, vhStream_t stream)
{
    if (!d_state || !guess || !pivot3) return VH_ERR_BAD_ARGUMENT;
    if (!power_of_two(radius) || !std::isfinite(pivot3[0]) || !std::isfinite(pivot3[1]) || !std::isfinite(pivot3[2])) return VH_ERR_BAD_ARGUMENT;
    VhAlignState h;
    std::memset(&h, 0, sizeof(h));
    VH_TRY(vh_resample_voxel_transforms(guess, vsSrc, vsDst, h.srcVoxFromDstVox, h.dstVoxFromSrcVox));
    for (int k = 0; k < 16; k++) h.dstFromSrc[k] = guess[k];
    for (int k = 0; k < 3; k++) h.pivot[k] = pivot3[k];
    h.invRadius = 1.0f / radius;
    h.vsSrc = vsSrc;
    h.vsDst = vsDst;
    hipStream_t s = (hipStream_t)stream;
    VH_HIP(hipMemcpyAsync(d_state, &h, sizeof(h), hipMemcpyHostToDevice, s));
    VH_HIP(hipStreamSynchronize(s));
    return VH_OK;
}

static int align_check(const VhHashData* dstHd, const VhHashParams* dstHp, const VhHashData* srcHd, const VhHashParams* srcHp, uint32_t n,
                       const VhSDFBlockDesc* d_srcDescs, float band)
{
    if (!dstHd || !dstHp || !srcHd || !srcHp) return VH_ERR_BAD_ARGUMENT;
    if (!dstHd->d_SDFBlocks || !srcHd->d_SDFBlocks || dstHp->m_hashNumBuckets < 1) return VH_ERR_BAD_ARGUMENT;
    if (n != 0 && !d_srcDescs) return VH_ERR_BAD_ARGUMENT;
    if (!std::isfinite(band) || !(band > 0.0f) || !(band <= VH_ALIGN_MOST_BAND)) return VH_ERR_BAD_ARGUMENT;
    const double s = (double)srcHp->m_virtualVoxelSize, d = (double)dstHp->m_virtualVoxelSize;
    if (!std::isfinite(s) || !std::isfinite(d) || !(s > 0.0) || !(d > 0.0) || s / d < 0.5 || s / d > 2.0) return VH_ERR_BAD_ARGUMENT;
    // the reach per axis, from the ratio alone (the estimate stays rigid): the ends of a block's taps differ by at most
    // ceil(7 sqrt(3) s / d + 1) + 1
    const double ends = std::ceil(7.0 * std::sqrt(3.0) * (s / d) + 1.0 + 1e-3) + 1.0;
    if ((int)std::floor(ends / 8.0) + 2 > kMostReach) return VH_ERR_BAD_ARGUMENT;
    return VH_OK;
}

int vh_align_step(const VhHashData* dstHd, const VhHashParams* dstHp, const VhHashData* srcHd, const VhHashParams* srcHp, uint32_t n,
                  const VhSDFBlockDesc* d_srcDescs, float band, uint32_t minCount, float condThres, double rotThres, double transThres, VhAlignState* d_state,
                  uint32_t* d_ticket, vhStream_t stream)
{
    if (!d_state || !d_ticket) return VH_ERR_BAD_ARGUMENT;
    VH_TRY(align_check(dstHd, dstHp, srcHd, srcHp, n, d_srcDescs, band));
    if (!std::isfinite(condThres) || !(condThres > 0.0f) || !std::isfinite(rotThres) || !(rotThres > 0.0) || !std::isfinite(transThres) || !(transThres > 0.0))
        return VH_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    if (n > VH_ALIGN_MOST_BLOCKS) { // a total could wrap: refused in the state as well, so that the caller's one read shows it
        k_align_raise<<<1, 64, 0, s>>>(d_state, VH_ALIGN_TOO_MANY);
        VH_TRY(vh_last_launch_error());
        return VH_ERR_BAD_ARGUMENT;
    }
    AlignArgs args;
    args.bandS = band * srcHp->m_virtualVoxelSize;
    args.bandD = band * dstHp->m_virtualVoxelSize;
    args.vsD = dstHp->m_virtualVoxelSize;
    args.condThres = condThres;
    args.minCount = minCount;
    args.rotThres = rotThres;
    args.transThres = transThres;
    VH_LAUNCH_TIMED(k_align_step, n != 0 ? n : 1u, 256, s, *dstHd, *dstHp, srcHd->d_SDFBlocks, n, d_srcDescs, args, d_state, d_ticket);
    return vh_last_launch_error();
}

int vh_align_bounds(uint32_t n, const VhSDFBlockDesc* d_descs, const uint32_t* d_count, int32_t* d_box6, vhStream_t stream)
{
    if (!d_box6 || (n != 0 && !d_descs)) return VH_ERR_BAD_ARGUMENT;
    if (n == 0) return VH_OK;
    k_align_bounds<<<cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(n, d_descs, d_count, d_box6);
    return vh_last_launch_error();
}

int vh_debug_align_rule(const VhHashData* dstHd, const VhHashParams* dstHp, const VhHashData* srcHd, const VhHashParams* srcHp, uint32_t n,
                        const VhSDFBlockDesc* d_srcDescs, const float* dstVoxFromSrcVox, const float pivot3[3], float invRadius, float band, float* d_out,
                        vhStream_t stream)
{
    if (!dstVoxFromSrcVox || !pivot3 || !d_out) return VH_ERR_BAD_ARGUMENT;
    VH_TRY(align_check(dstHd, dstHp, srcHd, srcHp, n, d_srcDescs, band));
    if (n == 0) return VH_OK;
    M34 m;
    for (int k = 0; k < 12; k++) m.m[k] = dstVoxFromSrcVox[k];
    k_align_rule<<<n, 256, 0, (hipStream_t)stream>>>(*dstHd, *dstHp, srcHd->d_SDFBlocks, n, d_srcDescs, m, pivot3[0], pivot3[1], pivot3[2], invRadius,
                                                     band * srcHp->m_virtualVoxelSize, band * dstHp->m_virtualVoxelSize, dstHp->m_virtualVoxelSize, d_out);
    return vh_last_launch_error();
}

} // extern "C"
