// vh_resample.hip -- resampled merge: a source scene sampled at the voxel centres of another lattice, under a rigid
// transform and a ratio of voxel sizes (not in the reference; DESIGN.md section 4 "Resampled merge" has the definition).
// Two kernels -- the destination blocks the source may reach, made distinct; the blocks' voxels, blended from eight taps
// each -- and their launcher-level C ABI (include/vh_api.h).  What comes out is a block list for vh_merge_blocks
// (vh_merge.hip), which is unchanged.  A unit of its own so that nothing is compiled beside k_render (DESIGN.md section
// 7 item 1); the rule is float arithmetic held bit for bit: MUST be compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "vh_device.hpp"
#include "vh_host_util.hpp"
#include "vh_mesh_table.hpp"
#include "vh_resample_blend.hpp"
#include "vh_scene_ops.hpp"

using namespace vhd;

namespace {

// d_work: kHeader words, then per slot of the candidate table a key, a candidate (the list; at most one per slot) and a
// word that says whether the slot's key has been listed
enum {
    W_CANDIDATES = 0,
    W_STATUS = 1,
    W_STAGED = 2,
    W_OBSERVED = 16, // observed voxels, striped (vh_scene_ops.hpp)
    kHeader = W_OBSERVED + kStripes * kStripeWords
};

constexpr int kBlockLimit = 1 << 20;   // block coordinates in [-2^20, 2^20): voxel coordinates below 2^23, exact in a float
constexpr uint32_t kMostSpan = 6;      // candidate blocks per axis and source block (ratio 2)
// (kMostReach, the source blocks per axis a destination block's taps reach, kMostCoord and M34: vh_resample_blend.hpp)

struct Work {
    uint32_t* header;
    unsigned long long* keys;
    unsigned long long* cand;
    uint32_t* listed;
};
Work carve(uint32_t* d_work, uint32_t slotsLog2)
{
    const size_t S = (size_t)1 << slotsLog2;
    Work w;
    w.header = d_work;
    w.keys = reinterpret_cast<unsigned long long*>(d_work + kHeader);
    w.cand = w.keys + S;
    w.listed = reinterpret_cast<uint32_t*>(w.cand + S);
    return w;
}

VHD bool block_in_range(I3 p)
{
    return p.x >= -kBlockLimit && p.x < kBlockLimit && p.y >= -kBlockLimit && p.y < kBlockLimit && p.z >= -kBlockLimit && p.z < kBlockLimit;
}
// three biased 21-bit block coordinates; bit 63 stays 0, so the all-ones word (kMeshKeyEmpty) is no key
VHD unsigned long long block_key(I3 p)
{
    return (unsigned long long)(uint32_t)(p.x + kBlockLimit) | ((unsigned long long)(uint32_t)(p.y + kBlockLimit) << 21) |
           ((unsigned long long)(uint32_t)(p.z + kBlockLimit) << 42);
}
VHD I3 key_block(unsigned long long k)
{
    return mki3((int)(k & 0x1fffffull) - kBlockLimit, (int)((k >> 21) & 0x1fffffull) - kBlockLimit, (int)((k >> 42) & 0x1fffffull) - kBlockLimit);
}

// A wave per source block, a lane per candidate.  Positions with a tap in block b are those of [8b - 1, 8b + 8)^3; the
// box's corners go through dstVoxFromSrcVox, the range they span is widened by a voxel on either side and cut into
// blocks: at most `span` per axis (the host derives it from the matrix), span^3 candidates in `rounds` rounds of 64.
// A candidate claims its key's slot in the table; the lane that lists it is the one that finds the slot unlisted.
__global__ __launch_bounds__(256) void k_resample_candidates(uint32_t n, const VhSDFBlockDesc* descs, M34 m, uint32_t span, uint32_t rounds,
                                                             uint32_t slotsLog2, Work w)
{
    const uint32_t b = blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave; // (uniform in the wave)
    const uint32_t lane = lane_id();
    uint32_t status = 0u;
    bool live = b < n;
    I3 lo = mki3(0, 0, 0), hi = mki3(0, 0, 0);
    if (live) {
        const I3 pos = mki3(descs[b].pos[0], descs[b].pos[1], descs[b].pos[2]);
        if (!block_in_range(pos)) {
            status = VH_RESAMPLE_OUT_OF_RANGE;
            live = false;
        } else {
            const float bl[3] = { (float)(8 * pos.x - 1), (float)(8 * pos.y - 1), (float)(8 * pos.z - 1) };
            const float bh[3] = { (float)(8 * pos.x + 8), (float)(8 * pos.y + 8), (float)(8 * pos.z + 8) };
            int l[3], h[3];
#pragma unroll
            for (int r = 0; r < 3; r++) {
                float least, most;
                row_range(&m.m[4 * r], bl, bh, least, most);
                // (f2i saturates: a range far outside the lattice stays outside)
                l[r] = f2i(floorf(least) - 1.0f) >> 3;
                h[r] = f2i(ceilf(most) + 1.0f) >> 3;
            }
            lo = mki3(l[0], l[1], l[2]);
            hi = mki3(h[0], h[1], h[2]);
            const bool fits = (uint32_t)(hi.x - lo.x) < span && (uint32_t)(hi.y - lo.y) < span && (uint32_t)(hi.z - lo.z) < span;
            if (!block_in_range(lo) || !block_in_range(hi) || !fits) { // (!fits: coordinates so large that the corners' rounding adds blocks)
                status = VH_RESAMPLE_OUT_OF_RANGE;
                live = false;
            }
        }
    }
    const uint32_t cube = span * span * span;
#pragma unroll 1
    for (uint32_t r = 0; r < rounds; r++) {
        const uint32_t c = r * kWave + lane;
        bool take = false;
        unsigned long long key = 0ull;
        if (live && c < cube) {
            const I3 p = mki3(lo.x + (int)(c % span), lo.y + (int)((c / span) % span), lo.z + (int)(c / (span * span)));
            if (p.x <= hi.x && p.y <= hi.y && p.z <= hi.z) {
                key = block_key(p);
                const uint32_t slot = weld_find_or_claim(w.keys, key, slotsLog2);
                if (slot == kNoSlot) status = VH_RESAMPLE_TABLE_FULL;
                else take = atomicExch(&w.listed[slot], 1u) == 0u;
            }
        }
        const uint32_t at = wave_append(take, &w.header[W_CANDIDATES]); // (at most one candidate per slot: the list cannot overrun)
        if (take) w.cand[at] = key;
    }
    if (status != 0u) atomicOr(&w.header[W_STATUS], status);
}

// One destination voxel by the rule: its position in the source, then the blend the registration shares
// (vh_resample_blend.hpp).  s_ptr: the pointers of the source blocks [loB, loB + dim) the workgroup resolved.
VHD uint2 resample_voxel(const VhVoxel* __restrict__ pool, const int* s_ptr, I3 loB, I3 dim, const M34& m, float i, float j, float k)
{
    const float qx = row(&m.m[0], i, j, k), qy = row(&m.m[4], i, j, k), qz = row(&m.m[8], i, j, k);
    if (!(fabsf(qx) < kMostCoord) || !(fabsf(qy) < kMostCoord) || !(fabsf(qz) < kMostCoord)) return make_uint2(0u, 0u);
    return blend_taps(pool, s_ptr, loB, dim, qx, qy, qz);
}

// The hot path: one workgroup of 256 per candidate block, one 16-byte pair of voxels per lane (voxels 2t and 2t + 1 of
// the block: neighbours in x).  The source blocks the block's taps can reach are resolved into LDS first, one
// lookup_ptr per block and none per tap.  Their range is exact: by the monotonicity of row(), every voxel's q lies
// between the least and the greatest q of the box's corners, computed by the same operations, so every tap lies in
// [floor(least), floor(most) + 1].  A block is 7 voxels wide: the corners' q differ by at most 7 * sum_c |m_rc| <=
// 7 * sqrt(3) * vsDst / vsSrc per axis, that is <= 12.2 at equal sizes and <= 24.3 at ratio 1/2; floor(most) + 1 -
// floor(least) <= 14 resp. 26, and an interval of L + 1 integers meets at most floor(L / 8) + 2 blocks: 3 resp. 5 per
// axis, kMostReach^3 pointers at most.  (The launcher refuses a matrix that exceeds the bound; the kernel checks it
// again, since the translation's size adds rounding to the corners.)
__global__ __launch_bounds__(256) void k_resample_blocks(VhHashData hd, VhHashParams hp, M34 m, uint32_t numCandidates, Work w, VhVoxel* __restrict__ staging,
                                                  VhSDFBlockDesc* __restrict__ outDescs)
{
    __shared__ int s_ptr[kMostReach * kMostReach * kMostReach];
    __shared__ uint32_t s_observed[256 / kWave];
    const uint32_t c = blockIdx.x, t = threadIdx.x;
    if (c >= numCandidates) return; // (uniform in the workgroup, as every branch around a barrier below)
    const I3 blk = key_block(w.cand[c]);
    const float bl[3] = { (float)(8 * blk.x), (float)(8 * blk.y), (float)(8 * blk.z) };
    const float bh[3] = { bl[0] + 7.0f, bl[1] + 7.0f, bl[2] + 7.0f };
    int l[3], d[3];
    bool fits = true;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        float least, most;
        row_range(&m.m[4 * r], bl, bh, least, most);
        // voxels whose q is not below 2^24 are unobserved whatever the source holds: the range need not cover them
        least = fminf(fmaxf(least, -kMostCoord), kMostCoord);
        most = fminf(fmaxf(most, -kMostCoord), kMostCoord);
        l[r] = (int)floorf(least) >> 3;
        d[r] = (((int)floorf(most) + 1) >> 3) - l[r] + 1;
        fits = fits && d[r] <= kMostReach;
    }
    if (!fits) {
        if (t == 0u) atomicOr(&w.header[W_STATUS], VH_RESAMPLE_OUT_OF_RANGE);
        return;
    }
    const I3 loB = mki3(l[0], l[1], l[2]), dim = mki3(d[0], d[1], d[2]);
    int ptr = VH_FREE_ENTRY;
    if (t < (uint32_t)(dim.x * dim.y * dim.z)) {
        ptr = lookup_ptr(hd, hp, mki3(loB.x + (int)(t % (uint32_t)dim.x), loB.y + (int)((t / (uint32_t)dim.x) % (uint32_t)dim.y), loB.z + (int)(t / (uint32_t)(dim.x * dim.y))));
        s_ptr[t] = ptr;
    }
    if (__syncthreads_or(ptr != VH_FREE_ENTRY) == 0) return; // the source holds nothing here: an empty candidate

    const float i = bl[0] + (float)((2u * t) & 7u), j = bl[1] + (float)((t >> 2) & 7u), k = bl[2] + (float)(t >> 5);
    const uint2 r0 = resample_voxel(hd.d_SDFBlocks, s_ptr, loB, dim, m, i, j, k);
    const uint2 r1 = resample_voxel(hd.d_SDFBlocks, s_ptr, loB, dim, m, i + 1.0f, j, k);
    reinterpret_cast<uint4*>(staging + (size_t)c * VH_SDF_BLOCK_VOXELS)[t] = make_uint4(r0.x, r0.y, r1.x, r1.y);
    const uint32_t seen = (uint32_t)__popcll(__ballot((r0.y >> 24) != 0u)) + (uint32_t)__popcll(__ballot((r1.y >> 24) != 0u));
    if (lane_id() == 0u) {
        s_observed[t / kWave] = seen;
        if (seen != 0u) atomicAdd(stripe_of(&w.header[W_OBSERVED], c), seen); // one atomic per wave
    }
    __syncthreads();
    if (t == 0u && (s_observed[0] | s_observed[1] | s_observed[2] | s_observed[3]) != 0u) {
        const uint32_t at = atomicAdd(&w.header[W_STAGED], 1u); // (at < numCandidates: a candidate is listed once)
        VhSDFBlockDesc out;
        out.pos[0] = blk.x; out.pos[1] = blk.y; out.pos[2] = blk.z;
        out.ptr = (int)(c * VH_SDF_BLOCK_VOXELS);
        outDescs[at] = out;
    }
}

void fill_counts(uint32_t n, const uint32_t* h, uint32_t* counts_out)
{
    counts_out[VH_RESAMPLE_SOURCE_BLOCKS] = n;
    counts_out[VH_RESAMPLE_CANDIDATES] = h[W_CANDIDATES];
    counts_out[VH_RESAMPLE_STAGED] = h[W_STAGED];
    counts_out[VH_RESAMPLE_OBSERVED] = stripes_sum(h, W_OBSERVED, 0);
    counts_out[VH_RESAMPLE_STATUS] = h[W_STATUS];
}

// the blocks per axis an interval of voxel coordinates can meet when its ends differ by at most `length`
uint32_t blocks_met(double length) { return (uint32_t)std::floor(length / 8.0) + 2u; }

// What the kernels' loops and tables are sized by, from the matrices alone (data sets no bound).  A source block's box
// is 9 voxels wide, its image's range per axis at most e = 9 * sum_c |m_rc|; floor - 1 to ceil + 1 differ by at most
// ceil(e) + 3.  A destination block is 7 wide: floor(most) + 1 - floor(least) <= ceil(7 * sum_c |m_rc|) + 1.
bool spans(const float* srcFromDst, const float* dstFromSrc, uint32_t* span, uint32_t* reach)
{
    *span = *reach = 0u;
    for (int k = 0; k < 12; k++)
        if (!std::isfinite(srcFromDst[k]) || !std::isfinite(dstFromSrc[k])) return false;
    for (int r = 0; r < 3; r++) {
        const double fwd = std::fabs((double)dstFromSrc[4 * r]) + std::fabs((double)dstFromSrc[4 * r + 1]) + std::fabs((double)dstFromSrc[4 * r + 2]);
        const double back = std::fabs((double)srcFromDst[4 * r]) + std::fabs((double)srcFromDst[4 * r + 1]) + std::fabs((double)srcFromDst[4 * r + 2]);
        if (fwd > 4.0 || back > 4.0) return false;
        *span = std::max(*span, blocks_met(std::ceil(9.0 * fwd + 1e-3) + 3.0));
        *reach = std::max(*reach, blocks_met(std::ceil(7.0 * back + 1e-3) + 1.0));
    }
    return *span <= kMostSpan && *reach <= (uint32_t)kMostReach;
}

} // namespace

extern "C" {

int vh_resample_voxel_transforms(const double* T, float vsSrc, float vsDst, float* srcVoxFromDstVox, float* dstVoxFromSrcVox)
{
    if (!T || !srcVoxFromDstVox || !dstVoxFromSrcVox) return VH_ERR_BAD_ARGUMENT;
    if (!std::isfinite(vsSrc) || !std::isfinite(vsDst) || !(vsSrc > 0.0f) || !(vsDst > 0.0f)) return VH_ERR_BAD_ARGUMENT;
    VH_TRY(vh_rigid_or_refuse(T));
    const double s = (double)vsSrc, d = (double)vsDst;
    if (s / d < 0.5 || s / d > 2.0) return VH_ERR_BAD_ARGUMENT;
    voxel_matrices(T, s, d, srcVoxFromDstVox, dstVoxFromSrcVox);
    return VH_OK;
}

size_t vh_resample_work_bytes(uint32_t slotsLog2)
{
    if (slotsLog2 > 28u) return 0;
    return (size_t)kHeader * sizeof(uint32_t) + ((size_t)1 << slotsLog2) * (2u * sizeof(unsigned long long) + sizeof(uint32_t));
}

int vh_resample_blocks(const VhHashData* srcHd, const VhHashParams* srcHp, uint32_t n, const VhSDFBlockDesc* d_srcDescs, const float* srcVoxFromDstVox,
                       const float* dstVoxFromSrcVox, uint32_t slotsLog2, uint32_t* d_work, VhSDFBlockDesc* d_outDescs, VhVoxel* d_staging,
                       uint32_t stagingBlocks, uint32_t* counts_out, vhStream_t stream)
{
    if (!srcHd || !srcHp || !srcVoxFromDstVox || !dstVoxFromSrcVox || !d_work || !counts_out) return VH_ERR_BAD_ARGUMENT;
    if (srcHp->m_hashNumBuckets < 1 || slotsLog2 < 4u || slotsLog2 > 28u) return VH_ERR_BAD_ARGUMENT;
    if ((d_outDescs != nullptr) != (d_staging != nullptr)) return VH_ERR_BAD_ARGUMENT;
    for (int k = 0; k < VH_RESAMPLE_NUM_COUNTS; k++) counts_out[k] = 0u;
    uint32_t span = 0u, reach = 0u;
    if (!spans(srcVoxFromDstVox, dstVoxFromSrcVox, &span, &reach)) return VH_ERR_BAD_ARGUMENT;
    if (n != 0 && !d_srcDescs) return VH_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    const Work w = carve(d_work, slotsLog2);
    const size_t S = (size_t)1 << slotsLog2;
    uint32_t h[kHeader];
    M34 m;

    if (!d_staging) { // count: the candidates
        VH_HIP(hipMemsetAsync(w.header, 0, kHeader * sizeof(uint32_t), s));
        VH_HIP(hipMemsetAsync(w.keys, 0xff, S * sizeof(unsigned long long), s));
        VH_HIP(hipMemsetAsync(w.listed, 0, S * sizeof(uint32_t), s));
        if (n != 0) {
            for (int k = 0; k < 12; k++) m.m[k] = dstVoxFromSrcVox[k];
            const uint32_t wavesPerGroup = 256 / kWave;
            VH_LAUNCH_TIMED(k_resample_candidates, cdiv(n, wavesPerGroup), 256, s, n, d_srcDescs, m, span, cdiv(span * span * span, kWave), slotsLog2, w);
            VH_TRY(vh_last_launch_error());
        }
        VH_TRY(read_header(d_work, h, kHeader, s));
        fill_counts(n, h, counts_out);
        return VH_OK;
    }

    // fill: the voxels of the candidates the count call left in d_work
    VH_TRY(read_header(d_work, h, kHeader, s));
    const uint32_t numCandidates = h[W_CANDIDATES];
    if (numCandidates > S || numCandidates > stagingBlocks || (uint64_t)numCandidates * VH_SDF_BLOCK_VOXELS > 0x7fffffffull) return VH_ERR_BAD_ARGUMENT;
    if (h[W_STATUS] == 0u && numCandidates != 0u) {
        for (int k = 0; k < 12; k++) m.m[k] = srcVoxFromDstVox[k];
        VH_LAUNCH_TIMED(k_resample_blocks, numCandidates, 256, s, *srcHd, *srcHp, m, numCandidates, w, d_staging, d_outDescs);
        VH_TRY(vh_last_launch_error());
        VH_TRY(read_header(d_work, h, kHeader, s));
    }
    fill_counts(n, h, counts_out);
    return VH_OK;
}

} // extern "C"
