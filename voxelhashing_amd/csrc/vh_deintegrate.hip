// vh_deintegrate.hip -- frame de-integration: a fused depth frame taken back out of the voxel hash on the device (not in
// the reference; DESIGN.md section 4 "Frame de-integration" has the definition).  The observation a frame made of a voxel
// is formed again from the frame's maps and its pose, exactly as the integrate pass formed it, and subtracted from the
// running average; a block that is left without an observed voxel goes back to the heap.  Three kernels -- apply the
// rule and form the per-block facts, delete the entries of the blocks that hold nothing any more, the rule alone on
// arrays of voxels -- and their launcher-level C ABI (include/vh_api.h).  Reads the block lists of vh_merge_gather, as
// vh_cut.hip does, and like it shares only vh_device.hpp with the frame loop (vh_kernels.hip); a unit of its own so
// that nothing is compiled beside k_render.  The rule is float arithmetic held bit for bit:
// MUST be compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "../../include/vh_api.h"
#include "vh_device.hpp"
#include "vh_host_util.hpp"
#include "vh_scene_ops.hpp"

using namespace vhd;

namespace {

// d_work: kHeader words, then three arrays of n words (a state word per block, two pending lists: vh_scene_ops.hpp)
enum {
    W_STATUS = 0,
    W_PENDING = 1, // two words: the pending lists' lengths (a delete pass reads one list and fills the other)
    W_COUNTS = 16, // the counts, striped

    C_PROCESSED = 0,
    C_CHANGED = 1,
    C_FREED = 2,
    C_VOXELS_CHANGED = 3,
    C_VOXELS_RESET = 4,
    C_VOXELS_AT_CAP = 5,
    kHeader = W_COUNTS + kStripes * kStripeWords
};
// per listed block, in the first array behind the header
enum : uint32_t {
    kProcessed = 1u, // the block is in the frame's frustum
    kChanged = 2u,   // processed, and the take-out changed a voxel
    kFreed = 4u      // processed, and no voxel has weight > 0 afterwards
};
// per wave, in LDS
enum : uint32_t { kAnyLeft = 1u, kAnyChanged = 2u };

// The observation the frame makes of voxel pi: what integrate_voxel (vh_frame_integrate.hpp) hands to combine_voxel, the
// same operations in the same order.  A voxel that fails a gate has no observation: weight 0 (an observation's weight is
// at least 1).
VHD Vox observe(const VhHashParams& hp, const VhDepthCameraParams& cp, const VhDepthCameraData& cam, I3 pi)
{
    Vox o;
    o.sdf = 0.0f;
    o.cw = 0u;
    const F3 pf = mat_mul_p(hp.m_rigidTransformInverse, vvp_to_world(hp.m_virtualVoxelSize, pi));
    const uint32_t sx = (uint32_t)f2i((pf.x * cp.fx / pf.z + cp.mx) + 0.5f);
    const uint32_t sy = (uint32_t)f2i((pf.y * cp.fy / pf.z + cp.my) + 0.5f);
    if (sx < cp.m_imageWidth && sy < cp.m_imageHeight) {
        const uint32_t pix = sy * cp.m_imageWidth + sx;
        const float depth = cam.d_depthData[pix];
        // (as in the integrate pass, which is the reference's: without a colour map the colour is MINF, which fails the
        // gate below -- a frame without colours puts nothing in, so there is nothing of it to take out)
        float cr = minf(), cg = minf(), cb = minf();
        if (cam.d_colorData) {
            const float4 c = reinterpret_cast<const float4*>(cam.d_colorData)[pix];
            cr = c.x; cg = c.y; cb = c.z;
        }
        if (cr != minf() && depth != minf() && depth < hp.m_maxIntegrationDistance) {
            const float depthZeroOne = cam_to_proj_z(cp, depth);
            float sdf = depth - pf.z;
            const float truncation = get_truncation(hp, depth);
            if (sdf > -truncation) {
                if (sdf >= 0.0f) sdf = fminf(truncation, sdf);
                else sdf = fmaxf(-truncation, sdf);
                const float weightUpdate = fmaxf((float)hp.m_integrationWeightSample * 1.5f * (1.0f - depthZeroOne), 1.0f);
                o.sdf = sdf;
                if (cam.d_colorData) o.cw = pack_cw(f2uc(255.0f * cr), f2uc(255.0f * cg), f2uc(255.0f * cb), f2uc(weightUpdate));
                else o.cw = pack_cw(0, 255, 0, f2uc(weightUpdate));
            }
        }
    }
    return o;
}

// The take-out: observation o out of the stored voxel v (include/vh_api.h has the rule).  The weighted colour per
// channel is floor((2 n + w') / (2 w')) clamped to a byte, n = c w - co wo: the quotient through a float division.
// |2 n + w'| < 2^18 and 2 w' <= 508 are exact floats; a quotient that is no integer lies at least 1 / 508 from one,
// its rounding moves it by less than 2^-15 while it is below 512, and the conversion saturates: below 0 gives 0, from
// 256 on gives 255, and in between it truncates a positive number, which is the floor.
VHD Vox take_out(const VhHashParams& hp, Vox v, Vox o)
{
    const uint32_t w = v.weight(), wo = o.weight();
    if (w == 0u || wo == 0u) return v;
    Vox out;
    out.sdf = 0.0f;
    out.cw = 0u;
    if (wo >= w) return out;
    const uint32_t wn = w - wo;
    const float fw = (float)w, fwo = (float)wo, fwn = (float)wn;
    out.sdf = (v.sdf * fw - o.sdf * fwo) / fwn;
    uint32_t rgb = v.cw & 0x00ffffffu;
    // (m_colorIntegration is the same for every voxel of a launch: a scalar branch)
    if (hp.m_colorIntegration != VH_COLOR_RUNNING_AVERAGE) {
        rgb = 0u;
#pragma unroll
        for (uint32_t ch = 0; ch < 3; ch++) {
            const int c = (int)((v.cw >> (8u * ch)) & 0xffu), co = (int)((o.cw >> (8u * ch)) & 0xffu);
            const int num = 2 * (c * (int)w - co * (int)wo) + (int)wn;
            rgb |= (uint32_t)f2uc((float)num / (2.0f * fwn)) << (8u * ch);
        }
    }
    out.cw = rgb | (wn << 24);
    return out;
}

// One workgroup of 256 per listed block, one 16-byte pair of voxels per lane (the shape of k_integrate<false> and
// k_cut_select).  The frustum test comes first and is the same in every lane: a block outside returns before any voxel
// is loaded.  The pair is on its way while the lane projects its two voxels; depth and colour are gathered from the
// frame's plain float maps.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_deint_apply(VhHashData hd, VhHashParams hp, VhDepthCameraData cam, VhDepthCameraParams cp, uint32_t n,
                                                     const VhSDFBlockDesc* descs, uint32_t* work, uint32_t* blockState)
{
    __shared__ uint32_t s_facts[256 / kWave];
    const uint32_t b = blockIdx.x, t = threadIdx.x;
    if (b >= n) return; // (uniform in the workgroup)
    const int4 q = *reinterpret_cast<const int4*>(&descs[b]);
    const int ex = __builtin_amdgcn_readfirstlane(q.x), ey = __builtin_amdgcn_readfirstlane(q.y);
    const int ez = __builtin_amdgcn_readfirstlane(q.z), ptr = __builtin_amdgcn_readfirstlane(q.w);
    if (!block_in_frustum(hp, cp, mki3(ex, ey, ez))) { // (uniform in the workgroup)
        if (t == 0u) blockState[b] = 0u;
        return;
    }
    uint4* at = reinterpret_cast<uint4*>(hd.d_SDFBlocks + (uint32_t)ptr) + t;
    const uint4 raw = *at;
    // voxel pair (2t, 2t + 1), neighbours in x; the integer coordinates wrap as the table's hash does its products
    const I3 p0 = mki3((int)(8u * (uint32_t)ex + ((2u * t) & 7u)), (int)(8u * (uint32_t)ey + ((t >> 2) & 7u)), (int)(8u * (uint32_t)ez + (t >> 5)));
    const Vox o0 = observe(hp, cp, cam, p0), o1 = observe(hp, cp, cam, mki3((int)((uint32_t)p0.x + 1u), p0.y, p0.z));
    const Vox v0 = unpack_vox(make_uint2(raw.x, raw.y)), v1 = unpack_vox(make_uint2(raw.z, raw.w));
    const Vox r0 = take_out(hp, v0, o0), r1 = take_out(hp, v1, o1);
    const bool c0 = v0.weight() != 0u && o0.weight() != 0u, c1 = v1.weight() != 0u && o1.weight() != 0u;
    const bool z0 = c0 && o0.weight() >= v0.weight(), z1 = c1 && o1.weight() >= v1.weight();
    const bool k0 = c0 && v0.weight() == hp.m_integrationWeightMax, k1 = c1 && v1.weight() == hp.m_integrationWeightMax;
    const unsigned long long anyLeft = __ballot(r0.weight() != 0u || r1.weight() != 0u);
    const uint32_t nChanged = (uint32_t)__popcll(__ballot(c0)) + (uint32_t)__popcll(__ballot(c1));
    const uint32_t nReset = (uint32_t)__popcll(__ballot(z0)) + (uint32_t)__popcll(__ballot(z1));
    const uint32_t nCap = (uint32_t)__popcll(__ballot(k0)) + (uint32_t)__popcll(__ballot(k1));
    uint32_t* stripe = stripe_of(&work[W_COUNTS], b);
    if (lane_id() == 0u) {
        s_facts[t / kWave] = (anyLeft != 0ull ? kAnyLeft : 0u) | (nChanged != 0u ? kAnyChanged : 0u);
        // per wave: one atomic for the voxels it changed, and one each for the rare kinds among them
        if (nChanged != 0u) atomicAdd(&stripe[C_VOXELS_CHANGED], nChanged);
        if (nReset != 0u) atomicAdd(&stripe[C_VOXELS_RESET], nReset);
        if (nCap != 0u) atomicAdd(&stripe[C_VOXELS_AT_CAP], nCap);
    }
    __syncthreads();
    const uint32_t f = s_facts[0] | s_facts[1] | s_facts[2] | s_facts[3];
    const uint32_t state = kProcessed | ((f & kAnyChanged) ? kChanged : 0u) | ((f & kAnyLeft) ? 0u : kFreed);
    if (t == 0u) {
        blockState[b] = state;
        atomicAdd(&stripe[C_PROCESSED], 1u);
        if (state & kChanged) atomicAdd(&stripe[C_CHANGED], 1u);
        if (state & kFreed) atomicAdd(&stripe[C_FREED], 1u);
    }
    if (WRITE) {
        // a freed block is zeroed whole (a free block is all zero: weight-0 voxels may hold sdf bits)
        if (state & kFreed) *at = make_uint4(0u, 0u, 0u, 0u);
        else if (c0 || c1) {
            const uint2 w0 = pack_vox(r0), w1 = pack_vox(r1);
            *at = make_uint4(w0.x, w0.y, w1.x, w1.y);
        }
    }
}

// the delete pass (vh_scene_ops.hpp) over the freed blocks
__global__ __launch_bounds__(64) void k_deint_delete(VhHashData hd, VhHashParams hp, const VhSDFBlockDesc* descs, int32_t lockToken, uint32_t* work,
                                                     const uint32_t* blockState, const uint32_t* pendingIn, uint32_t nIn, uint32_t* pendingOut, uint32_t outSel)
{
    delete_listed(hd, hp, descs, lockToken, blockState, kFreed, pendingIn, nIn, pendingOut, &work[W_PENDING + outSel]);
}

// the rule alone: out[i] = observed[i] taken out of stored[i]
__global__ __launch_bounds__(256) void k_deint_rule(const uint2* stored, const uint2* observed, uint2* out, uint32_t n, VhHashParams hp)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = pack_vox(take_out(hp, unpack_vox(stored[i]), unpack_vox(observed[i])));
}

} // namespace

extern "C" {

size_t vh_deintegrate_work_bytes(uint32_t n) { return settle_work_bytes(kHeader, n); }

int vh_deintegrate_blocks(const VhHashData* hd, const VhHashParams* hp, uint32_t n, const VhSDFBlockDesc* d_descs, const VhDepthCameraData* cam,
                          const VhDepthCameraParams* cp, uint32_t flags, int32_t lockToken, uint32_t* d_work, uint32_t* counts_out, vhStream_t stream)
{
    if (!hd || !hp || !cam || !cp || !d_work || !counts_out) return VH_ERR_BAD_ARGUMENT;
    if ((flags & ~VH_DEINT_COUNT_ONLY) != 0u) return VH_ERR_BAD_ARGUMENT;
    if (!hd->d_SDFBlocks || hp->m_hashNumBuckets < 2 || !cam->d_depthData || cp->m_imageWidth == 0u || cp->m_imageHeight == 0u) return VH_ERR_BAD_ARGUMENT;
    for (int k = 0; k < VH_DEINT_NUM_COUNTS; k++) counts_out[k] = 0u;
    if (n == 0) return VH_OK;
    if (!d_descs) return VH_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    const bool countOnly = (flags & VH_DEINT_COUNT_ONLY) != 0u;
    const SettleArrays a = settle_arrays(d_work, kHeader, n);
    uint32_t* blockState = a.blockState;
    uint32_t h[kHeader];

    // Stage 1: the take-out, the state words and the counts
    VH_HIP(hipMemsetAsync(d_work, 0, kHeader * sizeof(uint32_t), s));
    if (countOnly) VH_LAUNCH_TIMED(k_deint_apply<false>, n, 256, s, *hd, *hp, *cam, *cp, n, d_descs, d_work, blockState);
    else VH_LAUNCH_TIMED(k_deint_apply<true>, n, 256, s, *hd, *hp, *cam, *cp, n, d_descs, d_work, blockState);
    VH_TRY(vh_last_launch_error());
    VH_TRY(read_header(d_work, h, kHeader, s));
    counts_out[VH_DEINT_BLOCKS_IN] = n;
    counts_out[VH_DEINT_PROCESSED] = stripes_sum(h, W_COUNTS, C_PROCESSED);
    counts_out[VH_DEINT_CHANGED] = stripes_sum(h, W_COUNTS, C_CHANGED);
    counts_out[VH_DEINT_FREED] = stripes_sum(h, W_COUNTS, C_FREED);
    counts_out[VH_DEINT_VOXELS_CHANGED] = stripes_sum(h, W_COUNTS, C_VOXELS_CHANGED);
    counts_out[VH_DEINT_VOXELS_RESET] = stripes_sum(h, W_COUNTS, C_VOXELS_RESET);
    counts_out[VH_DEINT_VOXELS_AT_CAP] = stripes_sum(h, W_COUNTS, C_VOXELS_AT_CAP);
    counts_out[VH_DEINT_STATUS] = h[W_STATUS];
    if (countOnly) return VH_OK;

    // Stage 2: delete passes while deletes lose their lock races.  The blocks were zeroed by an earlier launch; the first
    // pass walks every block's state word.
    const uint32_t freed = counts_out[VH_DEINT_FREED];
    Settled st;
    VH_TRY(settle_passes<kHeader>(hd, hp, stream, d_work, a, W_PENDING, freed != 0u ? n : 0u, freed + 8u,
                                  [&](const uint32_t* pendingIn, uint32_t nIn, uint32_t* pendingOut, uint32_t outSel, uint32_t pass) {
                                      VH_LAUNCH_TIMED(k_deint_delete, cdiv(nIn, 64), 64, s, *hd, *hp, d_descs, lockToken, d_work, blockState,
                                                      pass == 0u ? nullptr : pendingIn, nIn, pendingOut, outSel);
                                  }, &st));
    counts_out[VH_DEINT_DELETE_PASSES] = st.passes;
    counts_out[VH_DEINT_UNSETTLED] = st.nPending;
    if (st.nPending != 0u) counts_out[VH_DEINT_STATUS] |= VH_DEINT_NOT_SETTLED;
    return VH_OK;
}

int vh_debug_deintegrate_rule(const VhVoxel* d_stored, const VhVoxel* d_observed, VhVoxel* d_out, uint32_t n, const VhHashParams* hp, vhStream_t stream)
{
    if (!hp || (n != 0 && (!d_stored || !d_observed || !d_out))) return VH_ERR_BAD_ARGUMENT;
    if (n == 0) return VH_OK;
    k_deint_rule<<<cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(reinterpret_cast<const uint2*>(d_stored), reinterpret_cast<const uint2*>(d_observed),
                                                                reinterpret_cast<uint2*>(d_out), n, *hp);
    return vh_last_launch_error();
}

} // extern "C"
