// vh_merge.hip -- scene merge: a second scene's blocks, or a list of blocks, fused into the voxel hash on the device
// (not in the reference; DESIGN.md section 4 "Scene merge" has the definition).  Four kernels -- gather the source's
// entries, classify them against the destination, allocate what is missing, combine the voxels -- and their launcher-level
// C ABI (include/vh_api.h).  Shares only vh_device.hpp with the frame loop (vh_kernels.hip), and is a unit of its own so
// that nothing is compiled beside k_render; like it, MUST be compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "../../include/vh_api.h"
#include "vh_device.hpp"
#include "vh_host_util.hpp"
#include "vh_scene_ops.hpp"

using namespace vhd;

namespace {

// d_work: kHeader words, then three arrays of n words (vh_scene_ops.hpp has the scheme)
enum {
    W_PRESENT = 0,
    W_MISSING = 1,
    W_STATUS = 2,
    W_PENDING = 3,   // two words: the pending lists' lengths (a pass reads one list and fills the other)
    W_LEFT_OUT = 5,
    W_ALLOCATED = 6,
    // The voxel counts, striped: 64-bit words {combined, copied << 32}.  (Fewer than 2^31 voxels can be merged -- a pool's
    // blocks are indexed by an int -- so the low half never carries into the high one.)
    W_VOXELS = 16,
    kHeader = W_VOXELS + kStripes * kStripeWords
};
// per source block, in the first array behind the header
enum : uint32_t { kBlockPresent = 0u, kBlockAllocated = 1u, kBlockPending = 2u, kBlockLeftOut = 3u };

VHD I3 shifted(const VhSDFBlockDesc& d, I3 o)
{
    // (wrapping, as the table's hash does its products)
    return mki3((int)((uint32_t)d.pos[0] + (uint32_t)o.x), (int)((uint32_t)d.pos[1] + (uint32_t)o.y), (int)((uint32_t)d.pos[2] + (uint32_t)o.z));
}

// The occupied entries of a table as a block list {pos, ptr}, in whatever order the atomics give (nothing downstream
// depends on it).  No frustum test: every block of the scene.  A lane whose bucket holds nothing (the occupancy bit, which
// counts the entries physically in the bucket, list elements of other buckets included) does not read its entry: of a
// table of 160 MB a scene of a few hundred blocks touches a few hundred lines.
__global__ __launch_bounds__(256) void k_merge_gather(VhHashData hd, uint32_t numEntries, VhSDFBlockDesc* out, uint32_t capacity, uint32_t* counter)
{
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    int4 q = make_int4(0, 0, 0, VH_FREE_ENTRY);
    if (idx < numEntries && bucket_maybe_occupied(hd, idx / VH_HASH_BUCKET_SIZE)) q = load_quad(&hd.d_hash[idx]);
    const bool take = q.w != VH_FREE_ENTRY;
    const uint64_t m = __ballot(take);
    if (m == 0ull) return;
    const uint32_t at = wave_run(m, counter);
    if (take && at < capacity) *reinterpret_cast<int4*>(&out[at]) = q;
}

// One lane per source block: is its position (shifted) in the destination?  Counts both answers and lists the missing
// blocks as the first alloc pass's work.
__global__ __launch_bounds__(256) void k_merge_classify(VhHashData hd, VhHashParams hp, uint32_t n, const VhSDFBlockDesc* descs, I3 offset,
                                                        uint32_t* work, uint32_t* blockState, uint32_t* pending)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool present = false, missing = false;
    if (i < n) {
        present = lookup_ptr(hd, hp, shifted(descs[i], offset)) != VH_FREE_ENTRY;
        missing = !present;
        blockState[i] = present ? kBlockPresent : kBlockPending;
    }
    wave_count(present, &work[W_PRESENT]);
    wave_count(missing, &work[W_MISSING]);
    wave_append(missing, i, &work[W_PENDING], pending);
}

// All or nothing on the heap, decided before anything is written: more missing positions than free blocks, and every
// later kernel of the call does nothing (they read the status word; the host needs no round trip to refuse).
__global__ void k_merge_decide(VhHashData hd, uint32_t* work)
{
    if (work[W_MISSING] > hd.d_heapCounter[0] + 1u) {
        work[W_STATUS] |= VH_MERGE_HEAP_SHORT;
        work[W_PENDING] = 0u;
    }
}

// One lane per block still pending: allocBlock.  0 / 1: done; 2 (lost a lock): pending for the next pass; 3 (no room by
// the table or list limit): left out whole -- allocBlock has then taken neither an entry nor a heap block.
__global__ __launch_bounds__(64) void k_merge_alloc(VhHashData hd, VhHashParams hp, const VhSDFBlockDesc* descs, I3 offset, int32_t lockToken,
                                                    uint32_t* work, uint32_t* blockState, const uint32_t* pendingIn, uint32_t nIn, uint32_t* pendingOut,
                                                    uint32_t outSel, uint32_t* leftOut)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    int r = -1;
    uint32_t i = 0u;
    if (t < nIn && !(work[W_STATUS] & VH_MERGE_HEAP_SHORT)) {
        i = pendingIn[t];
        r = alloc_block(hd, hp, shifted(descs[i], offset), lockToken);
    }
    if (r == 0 || r == 1) blockState[i] = r == 1 ? kBlockAllocated : kBlockPresent;
    wave_count(r == 1, &work[W_ALLOCATED]);
    wave_count(r == 0, &work[W_PRESENT]); // (only where two source blocks name one position: the second finds the first's block)
    wave_append(r == 2, i, &work[W_PENDING + outSel], pendingOut);
    if (r == 3) {
        blockState[i] = kBlockLeftOut;
        const uint32_t k = atomicAdd(&work[W_LEFT_OUT], 1u);
        if (leftOut) leftOut[k] = i;
        atomicOr(&work[W_STATUS], VH_MERGE_NO_SLOT);
    }
}

// what is still pending at the bound on passes is left out
__global__ __launch_bounds__(64) void k_merge_give_up(uint32_t* work, uint32_t* blockState, const uint32_t* pendingIn, uint32_t nIn, uint32_t* leftOut)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nIn) return;
    const uint32_t i = pendingIn[t];
    blockState[i] = kBlockLeftOut;
    const uint32_t k = atomicAdd(&work[W_LEFT_OUT], 1u);
    if (leftOut) leftOut[k] = i;
    if (t == 0u) atomicOr(&work[W_STATUS], VH_MERGE_NOT_SETTLED);
}

// the per-voxel rule; d and s as stored (sdf bits, colour + weight)
VHD uint2 merge_voxel(const VhHashParams& hp, uint2 d, uint2 s, bool& combined, bool& copied)
{
    const uint32_t wd = d.y >> 24, ws = s.y >> 24;
    combined = wd != 0u && ws != 0u;
    copied = wd == 0u && ws != 0u;
    if (combined) return pack_vox(combine_voxel(hp, unpack_vox(d), unpack_vox(s)));
    // not through combineVoxel: (s.sdf * w) / w is not always s.sdf, and the 50/50 colour would halve it against black
    if (copied) return make_uint2(s.x, (s.y & 0x00ffffffu) | (min(hp.m_integrationWeightMax, ws) << 24));
    return d;
}

// One workgroup of 256 per source block, one 16-byte pair of voxels per lane.  The source's voxels are the list's
// (blocks + b * 512) or, with srcSDFBlocks, the source scene's own pool at the block's ptr (no intermediate copy).
__global__ __launch_bounds__(256) void k_merge_combine(VhHashData hd, VhHashParams hp, uint32_t n, const VhSDFBlockDesc* descs, const VhVoxel* blocks,
                                                       const VhVoxel* srcSDFBlocks, I3 offset, uint32_t* work, const uint32_t* blockState)
{
    __shared__ int s_ptr;
    const uint32_t b = blockIdx.x;
    if (b >= n || (work[W_STATUS] & VH_MERGE_HEAP_SHORT) || blockState[b] >= kBlockPending) return; // (uniform in the workgroup)
    const VhSDFBlockDesc dsc = descs[b];
    // the source's pair is on its way while one lane walks the destination's bucket
    const VhVoxel* src = srcSDFBlocks ? srcSDFBlocks + (uint32_t)dsc.ptr : blocks + (size_t)b * VH_SDF_BLOCK_VOXELS;
    const uint4 s = reinterpret_cast<const uint4*>(src)[threadIdx.x];
    if (threadIdx.x == 0u) s_ptr = lookup_ptr(hd, hp, shifted(dsc, offset));
    __syncthreads();
    const int ptr = s_ptr;
    if (ptr == VH_FREE_ENTRY) return;
    uint4* dst = reinterpret_cast<uint4*>(&hd.d_SDFBlocks[(uint32_t)ptr]) + threadIdx.x;
    const uint4 d = *dst;
    bool comb0, copy0, comb1, copy1;
    const uint2 r0 = merge_voxel(hp, make_uint2(d.x, d.y), make_uint2(s.x, s.y), comb0, copy0);
    const uint2 r1 = merge_voxel(hp, make_uint2(d.z, d.w), make_uint2(s.z, s.w), comb1, copy1);
    if (comb0 || copy0 || comb1 || copy1) *dst = make_uint4(r0.x, r0.y, r1.x, r1.y);
    const uint32_t nComb = (uint32_t)__popcll(__ballot(comb0)) + (uint32_t)__popcll(__ballot(comb1));
    const uint32_t nCopy = (uint32_t)__popcll(__ballot(copy0)) + (uint32_t)__popcll(__ballot(copy1));
    if (lane_id() == 0u && (nComb | nCopy) != 0u) // one atomic per wave
        atomicAdd(reinterpret_cast<unsigned long long*>(stripe_of(&work[W_VOXELS], b)), (unsigned long long)nComb | ((unsigned long long)nCopy << 32));
}

} // namespace

extern "C" {

size_t vh_merge_work_bytes(uint32_t n) { return settle_work_bytes(kHeader, n); }

int vh_merge_gather(const VhHashData* hd, const VhHashParams* hp, VhSDFBlockDesc* d_descs, uint32_t capacity, uint32_t* d_counter, vhStream_t stream)
{
    if (!hd || !hp || !d_descs || !d_counter || capacity == 0) return VH_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    VH_HIP(hipMemsetAsync(d_counter, 0, sizeof(uint32_t), s));
    const uint64_t ne = (uint64_t)hp->m_hashNumBuckets * VH_HASH_BUCKET_SIZE;
    if (ne == 0 || ne > 0xffffffffull) return VH_ERR_BAD_ARGUMENT;
    VH_LAUNCH_TIMED(k_merge_gather, cdiv(ne, 256), 256, s, *hd, (uint32_t)ne, d_descs, capacity, d_counter);
    return vh_last_launch_error();
}

int vh_merge_blocks(const VhHashData* hd, const VhHashParams* hp, uint32_t n, const VhSDFBlockDesc* d_descs, const VhVoxel* d_blocks,
                    const VhVoxel* srcSDFBlocks, const int32_t blockOffset[3], int32_t lockToken, uint32_t* d_work, uint32_t* d_leftOut,
                    uint32_t* counts_out, vhStream_t stream)
{
    if (!hd || !hp || !blockOffset || !d_work || !counts_out) return VH_ERR_BAD_ARGUMENT;
    if (hp->m_hashNumBuckets < 2) return VH_ERR_BAD_ARGUMENT;
    for (int k = 0; k < VH_MERGE_NUM_COUNTS; k++) counts_out[k] = 0u;
    if (n == 0) return VH_OK;
    if (!d_descs || (d_blocks != nullptr) == (srcSDFBlocks != nullptr)) return VH_ERR_BAD_ARGUMENT; // exactly one source
    hipStream_t s = (hipStream_t)stream;
    I3 off;
    off.x = blockOffset[0]; off.y = blockOffset[1]; off.z = blockOffset[2];
    const SettleArrays a = settle_arrays(d_work, kHeader, n);
    uint32_t* blockState = a.blockState;
    uint32_t h[kHeader];

    VH_HIP(hipMemsetAsync(d_work, 0, kHeader * sizeof(uint32_t), s));
    VH_LAUNCH_TIMED(k_merge_classify, cdiv(n, 256), 256, s, *hd, *hp, n, d_descs, off, d_work, blockState, a.pending[0]);
    VH_LAUNCH_TIMED(k_merge_decide, 1, 1, s, *hd, d_work);
    VH_TRY(vh_last_launch_error());
    VH_TRY(read_header(d_work, h, kHeader, s));

    // alloc passes while blocks lose their lock races, starting from the list the classification left
    Settled st;
    VH_TRY(settle_passes<kHeader>(hd, hp, stream, d_work, a, W_PENDING, h[W_PENDING], h[W_MISSING] + 8u,
                                  [&](const uint32_t* pendingIn, uint32_t nIn, uint32_t* pendingOut, uint32_t outSel, uint32_t) {
                                      VH_LAUNCH_TIMED(k_merge_alloc, cdiv(nIn, 64), 64, s, *hd, *hp, d_descs, off, lockToken, d_work, blockState, pendingIn, nIn,
                                                      pendingOut, outSel, d_leftOut);
                                  }, &st));
    if (st.nPending != 0u) VH_LAUNCH_TIMED(k_merge_give_up, cdiv(st.nPending, 64), 64, s, d_work, blockState, a.pending[st.in], st.nPending, d_leftOut);
    if (!(h[W_STATUS] & VH_MERGE_HEAP_SHORT)) VH_LAUNCH_TIMED(k_merge_combine, n, 256, s, *hd, *hp, n, d_descs, d_blocks, srcSDFBlocks, off, d_work, blockState);
    VH_TRY(vh_last_launch_error());
    VH_TRY(read_header(d_work, h, kHeader, s));

    counts_out[VH_MERGE_SOURCE_BLOCKS] = n;
    counts_out[VH_MERGE_PRESENT] = h[W_PRESENT];
    counts_out[VH_MERGE_ALLOCATED] = h[W_ALLOCATED];
    counts_out[VH_MERGE_LEFT_OUT] = h[W_LEFT_OUT];
    counts_out[VH_MERGE_COMBINED] = stripes_sum(h, W_VOXELS, 0);
    counts_out[VH_MERGE_COPIED] = stripes_sum(h, W_VOXELS, 1);
    counts_out[VH_MERGE_ALLOC_PASSES] = st.passes;
    counts_out[VH_MERGE_STATUS] = h[W_STATUS];
    return VH_OK;
}

} // extern "C"
