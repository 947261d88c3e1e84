// vh_cut.hip -- scene cut: the voxels of a box or an ellipsoid (or of everything outside one) erased from the voxel hash
// on the device, lifted out as a block list, or both (not in the reference; DESIGN.md section 4 "Scene cut" has the
// definition).  Five kernels -- select the voxels and form the per-block facts, decide whether the staging pool is large
// enough, lift, erase, delete the entries of the blocks that hold nothing any more -- and their launcher-level C ABI
// (include/vh_api.h).  The opposite of vh_merge.hip, whose block lists it reads (vh_merge_gather) and writes (a lifted
// list is one for vh_merge_blocks).  Shares only vh_device.hpp with the frame loop (vh_kernels.hip), and is a unit of its
// own so that nothing is compiled beside k_render; the rule is float arithmetic held bit for
// bit: MUST be compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/vh_api.h"
#include "vh_device.hpp"
#include "vh_host_util.hpp"
#include "vh_resample_blend.hpp"
#include "vh_scene_ops.hpp"

using namespace vhd;

namespace {

// d_work: kHeader words, then three arrays of n words (a state word per block, two pending lists: vh_scene_ops.hpp)
enum {
    W_STATUS = 0,
    W_PENDING = 1,  // two words: the pending lists' lengths (a delete pass reads one list and fills the other)
    W_STAGED = 3,   // staging slots handed out
    W_LIFTABLE = 4, // the stripes' sum, by k_cut_decide
    // the counts, striped: {selected observed voxels, blocks touched, blocks freeable, blocks liftable}
    W_COUNTS = 16,
    C_VOXELS = 0,
    C_TOUCHED = 1,
    C_FREEABLE = 2,
    C_LIFTABLE = 3,
    kHeader = W_COUNTS + kStripes * kStripeWords
};
// per source block, in the first array behind the header
enum : uint32_t {
    kTouched = 1u,  // a voxel of the block is selected, whatever its weight
    kFreeable = 2u, // touched, and no unselected voxel has weight > 0
    kLiftable = 4u  // touched, and a selected voxel has weight > 0
};
// per wave, in LDS
enum : uint32_t { kAnySelected = 1u, kAnyUnselectedObserved = 2u, kAnySelectedObserved = 4u };

// (M34, here regionFromVox, and row(), one row of the rule with one rounding per operation: vh_resample_blend.hpp)

// the per-voxel rule: is voxel (i, j, k) selected?  A comparison with a NaN is false: such a voxel is not inside.
VHD bool selected(const M34& m, uint32_t shape, bool outside, float i, float j, float k)
{
    const float ux = row(&m.m[0], i, j, k), uy = row(&m.m[4], i, j, k), uz = row(&m.m[8], i, j, k);
    const bool inside = shape == VH_CUT_ELLIPSOID ? (ux * ux + uy * uy) + uz * uz <= 1.0f : fabsf(ux) <= 1.0f && fabsf(uy) <= 1.0f && fabsf(uz) <= 1.0f;
    return inside != outside;
}

// Lane t of a block's workgroup owns voxels 2t and 2t + 1 (neighbours in x): are they selected?  The voxel's integer
// coordinates wrap as the table's hash does its products.
VHD void selected_pair(const M34& m, uint32_t shape, bool outside, const VhSDFBlockDesc& d, uint32_t t, bool& s0, bool& s1)
{
    const float i = (float)(int)(8u * (uint32_t)d.pos[0] + ((2u * t) & 7u));
    const float i1 = (float)(int)(8u * (uint32_t)d.pos[0] + ((2u * t) & 7u) + 1u);
    const float j = (float)(int)(8u * (uint32_t)d.pos[1] + ((t >> 2) & 7u));
    const float k = (float)(int)(8u * (uint32_t)d.pos[2] + (t >> 5));
    s0 = selected(m, shape, outside, i, j, k);
    s1 = selected(m, shape, outside, i1, j, k);
}

VHD VhVoxel* voxels_of(const VhHashData& hd, VhVoxel* blocks, const VhSDFBlockDesc& d, uint32_t b)
{
    return blocks ? blocks + (size_t)b * VH_SDF_BLOCK_VOXELS : hd.d_SDFBlocks + (uint32_t)d.ptr;
}

// One workgroup of 256 per source block, one 16-byte pair of voxels per lane: the block's state word and the counts.
// The pair is on its way while the lane does the region's arithmetic.  kErase: the erase of a call that lifts nothing,
// which no later kernel of the call can refuse, is done here too (what k_cut_erase writes, from the pair in registers).
template <bool kErase>
__global__ __launch_bounds__(256) void k_cut_select(VhHashData hd, uint32_t n, const VhSDFBlockDesc* descs, VhVoxel* blocks, M34 m, uint32_t shape,
                                                    uint32_t outside, uint32_t* work, uint32_t* blockState)
{
    __shared__ uint32_t s_facts[256 / kWave];
    const uint32_t b = blockIdx.x, t = threadIdx.x;
    if (b >= n) return; // (uniform in the workgroup)
    const VhSDFBlockDesc dsc = descs[b];
    uint4* at = reinterpret_cast<uint4*>(voxels_of(hd, blocks, dsc, b)) + t;
    const uint4 v = *at;
    bool s0, s1;
    selected_pair(m, shape, outside != 0u, dsc, t, s0, s1);
    const bool o0 = (v.y >> 24) != 0u, o1 = (v.w >> 24) != 0u;
    const unsigned long long anySel = __ballot(s0 || s1), anyKept = __ballot((!s0 && o0) || (!s1 && o1));
    const uint32_t nGone = (uint32_t)__popcll(__ballot(s0 && o0)) + (uint32_t)__popcll(__ballot(s1 && o1));
    uint32_t* stripe = stripe_of(&work[W_COUNTS], b);
    if (lane_id() == 0u) {
        s_facts[t / kWave] = (anySel != 0ull ? kAnySelected : 0u) | (anyKept != 0ull ? kAnyUnselectedObserved : 0u) | (nGone != 0u ? kAnySelectedObserved : 0u);
        if (nGone != 0u) atomicAdd(&stripe[C_VOXELS], nGone); // one atomic per wave
    }
    __syncthreads();
    const uint32_t f = s_facts[0] | s_facts[1] | s_facts[2] | s_facts[3];
    uint32_t state = 0u;
    if (f & kAnySelected) state = kTouched | ((f & kAnyUnselectedObserved) ? 0u : kFreeable) | ((f & kAnySelectedObserved) ? kLiftable : 0u);
    if (t == 0u) {
        blockState[b] = state;
        if (state & kTouched) atomicAdd(&stripe[C_TOUCHED], 1u);
        if (state & kFreeable) atomicAdd(&stripe[C_FREEABLE], 1u);
        if (state & kLiftable) atomicAdd(&stripe[C_LIFTABLE], 1u);
    }
    if (kErase && (state & kTouched)) {
        const bool all = (state & kFreeable) != 0u;
        if (all || s0 || s1) *at = make_uint4(all || s0 ? 0u : v.x, all || s0 ? 0u : v.y, all || s1 ? 0u : v.z, all || s1 ? 0u : v.w);
    }
}

// All or nothing on the staging pool, decided before anything is written: more blocks to lift than it has room for, and
// every later kernel of the call does nothing (they read the status word; the host needs no round trip to refuse).
__global__ void k_cut_decide(uint32_t* work, uint32_t stagingBlocks)
{
    uint32_t liftable = 0u;
    for (uint32_t k = 0; k < kStripes; k++) liftable += work[W_COUNTS + k * kStripeWords + C_LIFTABLE];
    work[W_LIFTABLE] = liftable;
    if (liftable > stagingBlocks) work[W_STATUS] |= VH_CUT_STAGING_SHORT;
}

// A liftable block whole into the staging slot one lane draws: selected voxels as they are, the others as zero.
__global__ __launch_bounds__(256) void k_cut_lift(VhHashData hd, uint32_t n, const VhSDFBlockDesc* descs, VhVoxel* blocks, M34 m, uint32_t shape,
                                                  uint32_t outside, const uint32_t* work, uint32_t* staged, const uint32_t* blockState,
                                                  VhSDFBlockDesc* __restrict__ outDescs, VhVoxel* __restrict__ staging, uint32_t stagingBlocks)
{
    __shared__ uint32_t s_slot;
    const uint32_t b = blockIdx.x, t = threadIdx.x;
    if (b >= n || (work[W_STATUS] & VH_CUT_STAGING_SHORT) || !(blockState[b] & kLiftable)) return; // (uniform in the workgroup)
    const VhSDFBlockDesc dsc = descs[b];
    const uint4 v = reinterpret_cast<const uint4*>(voxels_of(hd, blocks, dsc, b))[t];
    if (t == 0u) s_slot = atomicAdd(staged, 1u);
    bool s0, s1;
    selected_pair(m, shape, outside != 0u, dsc, t, s0, s1);
    __syncthreads();
    const uint32_t slot = s_slot;
    if (slot >= stagingBlocks) return; // (k_cut_decide has seen to it: a liftable block is listed once)
    reinterpret_cast<uint4*>(staging + (size_t)slot * VH_SDF_BLOCK_VOXELS)[t] = make_uint4(s0 ? v.x : 0u, s0 ? v.y : 0u, s1 ? v.z : 0u, s1 ? v.w : 0u);
    if (t == 0u) {
        VhSDFBlockDesc out;
        out.pos[0] = dsc.pos[0]; out.pos[1] = dsc.pos[1]; out.pos[2] = dsc.pos[2];
        out.ptr = (int)(slot * VH_SDF_BLOCK_VOXELS);
        *reinterpret_cast<int4*>(&outDescs[slot]) = make_int4(out.pos[0], out.pos[1], out.pos[2], out.ptr);
    }
}

// Touched blocks only (an untouched block's workgroup returns after reading its state word): a freeable block is
// zeroed whole, of any other the selected voxels.  Nothing is read: a voxel is an 8-byte store.
__global__ __launch_bounds__(256) void k_cut_erase(VhHashData hd, uint32_t n, const VhSDFBlockDesc* descs, M34 m, uint32_t shape, uint32_t outside,
                                                   const uint32_t* work, const uint32_t* blockState)
{
    const uint32_t b = blockIdx.x, t = threadIdx.x;
    if (b >= n) return;
    const uint32_t state = blockState[b];
    if (!(state & kTouched) || (work[W_STATUS] & VH_CUT_STAGING_SHORT)) return; // (uniform in the workgroup)
    const VhSDFBlockDesc dsc = descs[b];
    uint2* at = reinterpret_cast<uint2*>(hd.d_SDFBlocks + (uint32_t)dsc.ptr) + 2u * t;
    if (state & kFreeable) {
        *reinterpret_cast<uint4*>(at) = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    bool s0, s1;
    selected_pair(m, shape, outside != 0u, dsc, t, s0, s1);
    if (s0) at[0] = make_uint2(0u, 0u);
    if (s1) at[1] = make_uint2(0u, 0u);
}

// the delete pass (vh_scene_ops.hpp) over the freeable blocks
__global__ __launch_bounds__(64) void k_cut_delete(VhHashData hd, VhHashParams hp, const VhSDFBlockDesc* descs, int32_t lockToken, uint32_t* work,
                                                   const uint32_t* blockState, const uint32_t* pendingIn, uint32_t nIn, uint32_t* pendingOut, uint32_t outSel)
{
    delete_listed(hd, hp, descs, lockToken, blockState, kFreeable, pendingIn, nIn, pendingOut, &work[W_PENDING + outSel]);
}

// what the classification says the call does (or, refused or only counting, would do)
void fill_counts(uint32_t n, uint32_t flags, const uint32_t* h, uint32_t* counts_out)
{
    const bool lift = (flags & VH_CUT_LIFT) != 0u, keep = (flags & VH_CUT_KEEP) != 0u;
    counts_out[VH_CUT_BLOCKS_IN] = n;
    counts_out[VH_CUT_TOUCHED] = stripes_sum(h, W_COUNTS, C_TOUCHED);
    counts_out[VH_CUT_FREED] = keep ? 0u : stripes_sum(h, W_COUNTS, C_FREEABLE);
    counts_out[VH_CUT_LIFTED] = lift ? stripes_sum(h, W_COUNTS, C_LIFTABLE) : 0u;
    counts_out[VH_CUT_VOXELS_ERASED] = keep ? 0u : stripes_sum(h, W_COUNTS, C_VOXELS);
    counts_out[VH_CUT_VOXELS_LIFTED] = lift ? stripes_sum(h, W_COUNTS, C_VOXELS) : 0u;
    counts_out[VH_CUT_STATUS] = h[W_STATUS];
}

} // namespace

extern "C" {

int vh_cut_region_transform(const double* T, const float* halfExtents3, float voxelSize, float* m12)
{
    if (!T || !halfExtents3 || !m12) return VH_ERR_BAD_ARGUMENT;
    if (!std::isfinite(voxelSize) || !(voxelSize > 0.0f)) return VH_ERR_BAD_ARGUMENT;
    for (int r = 0; r < 3; r++)
        if (!std::isfinite(halfExtents3[r]) || !(halfExtents3[r] > 0.0f)) return VH_ERR_BAD_ARGUMENT;
    VH_TRY(vh_rigid_or_refuse(T));
    double R[3][3], t[3];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) R[r][c] = T[4 * r + c];
        t[r] = T[4 * r + 3];
    }
    const double vs = (double)voxelSize;
    for (int r = 0; r < 3; r++) {
        const double h = (double)halfExtents3[r];
        for (int c = 0; c < 3; c++) m12[4 * r + c] = (float)((R[c][r] * vs) / h);
        m12[4 * r + 3] = (float)(-(((R[0][r] * t[0] + R[1][r] * t[1]) + R[2][r] * t[2]) / h));
    }
    return VH_OK;
}

size_t vh_cut_work_bytes(uint32_t n) { return settle_work_bytes(kHeader, n); }

int vh_cut_blocks(const VhHashData* hd, const VhHashParams* hp, uint32_t n, const VhSDFBlockDesc* d_descs, const VhVoxel* d_blocks, const float* m12,
                  uint32_t shape, uint32_t flags, int32_t lockToken, uint32_t* d_work, VhSDFBlockDesc* d_outDescs, VhVoxel* d_staging,
                  uint32_t stagingBlocks, uint32_t* counts_out, vhStream_t stream)
{
    if (!hp || !m12 || !d_work || !counts_out) return VH_ERR_BAD_ARGUMENT;
    const bool lift = (flags & VH_CUT_LIFT) != 0u, keep = (flags & VH_CUT_KEEP) != 0u, countOnly = (flags & VH_CUT_COUNT_ONLY) != 0u;
    if (shape > VH_CUT_ELLIPSOID || (flags & ~(VH_CUT_SELECT_OUTSIDE | VH_CUT_LIFT | VH_CUT_KEEP | VH_CUT_COUNT_ONLY)) != 0u) return VH_ERR_BAD_ARGUMENT;
    if (keep && !lift) return VH_ERR_BAD_ARGUMENT;
    if (d_blocks ? !keep : (!hd || !hd->d_SDFBlocks || hp->m_hashNumBuckets < 2)) return VH_ERR_BAD_ARGUMENT; // a list is only copied from
    if (lift && !countOnly && stagingBlocks != 0u && (!d_outDescs || !d_staging)) return VH_ERR_BAD_ARGUMENT;
    for (int k = 0; k < VH_CUT_NUM_COUNTS; k++) counts_out[k] = 0u;
    if (n == 0) return VH_OK;
    if (!d_descs) return VH_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    const VhHashData noTable = {};
    const VhHashData& table = hd ? *hd : noTable;
    VhVoxel* blocks = const_cast<VhVoxel*>(d_blocks); // (only read: nothing erases a list)
    const uint32_t outside = (flags & VH_CUT_SELECT_OUTSIDE) ? 1u : 0u;
    const SettleArrays a = settle_arrays(d_work, kHeader, n);
    uint32_t* blockState = a.blockState;
    uint32_t h[kHeader];
    M34 m;
    for (int k = 0; k < 12; k++) m.m[k] = m12[k];

    // Stage 1: the state words and the counts; a call that only erases erases here.
    const bool eraseInSelect = !countOnly && !lift;
    VH_HIP(hipMemsetAsync(d_work, 0, kHeader * sizeof(uint32_t), s));
    if (eraseInSelect) VH_LAUNCH_TIMED(k_cut_select<true>, n, 256, s, table, n, d_descs, blocks, m, shape, outside, d_work, blockState);
    else VH_LAUNCH_TIMED(k_cut_select<false>, n, 256, s, table, n, d_descs, blocks, m, shape, outside, d_work, blockState);
    if (lift && !countOnly) {
        VH_LAUNCH_TIMED(k_cut_decide, 1, 1, s, d_work, stagingBlocks);
        VH_LAUNCH_TIMED(k_cut_lift, n, 256, s, table, n, d_descs, blocks, m, shape, outside, d_work, &d_work[W_STAGED], blockState, d_outDescs, d_staging,
                        stagingBlocks);
        if (!keep) VH_LAUNCH_TIMED(k_cut_erase, n, 256, s, table, n, d_descs, m, shape, outside, d_work, blockState);
    }
    VH_TRY(vh_last_launch_error());
    VH_TRY(read_header(d_work, h, kHeader, s));
    fill_counts(n, flags, h, counts_out);
    if (countOnly || keep) return (h[W_STATUS] & VH_CUT_STAGING_SHORT) ? VH_ERR_BAD_ARGUMENT : VH_OK;
    if (h[W_STATUS] & VH_CUT_STAGING_SHORT) return VH_ERR_BAD_ARGUMENT; // nothing was written

    // Stage 2: delete passes while deletes lose their lock races.  The blocks were zeroed by an earlier launch; the first
    // pass walks every block's state word.
    const uint32_t freeable = counts_out[VH_CUT_FREED];
    Settled st;
    VH_TRY(settle_passes<kHeader>(hd, hp, stream, d_work, a, W_PENDING, freeable != 0u ? n : 0u, freeable + 8u,
                                  [&](const uint32_t* pendingIn, uint32_t nIn, uint32_t* pendingOut, uint32_t outSel, uint32_t pass) {
                                      VH_LAUNCH_TIMED(k_cut_delete, cdiv(nIn, 64), 64, s, table, *hp, d_descs, lockToken, d_work, blockState,
                                                      pass == 0u ? nullptr : pendingIn, nIn, pendingOut, outSel);
                                  }, &st));
    counts_out[VH_CUT_DELETE_PASSES] = st.passes;
    counts_out[VH_CUT_UNSETTLED] = st.nPending;
    if (st.nPending != 0u) counts_out[VH_CUT_STATUS] |= VH_CUT_NOT_SETTLED;
    return VH_OK;
}

} // extern "C"
