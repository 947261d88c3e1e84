// vh_streaming.hip -- chunk streaming between the voxel hash and the host's chunk grid (DSC/CUDASceneRepChunkGrid.cu):
// the stream-out and stream-in passes, the probe and the kernels that publish a pass's result to mapped host memory, with
// their launcher-level C ABI (include/vh_api.h).  Shares only vh_device.hpp with the frame loop (vh_kernels.hip); like it,
// MUST be compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "../../include/vh_api.h"
#include "vh_device.hpp"
#include "vh_host_util.hpp"

using namespace vhd;

namespace {

// integrateFromGlobalHashPass1Kernel :27-74.  The double heap push of the reference's list branch (:58-64) is not
// reproduced: the element delete is the only push (DESIGN.md "Fenced reference defects").  With a bit mask the scan also
// keeps the DEVICE's copy of it: the bit of every block's chunk is set here, where the block leaves, instead of by the
// host a round trip later (the host sets the same bit in its own copy when the block arrives; the frame's alloc pass,
// which reads the mask, then need not wait for the host).
VHD void stream_out_scan(const VhHashData& hd, const VhHashParams& hp, uint32_t start, float radius, float cx, float cy, float cz,
                         uint32_t* outCounter, VhSDFBlockDesc* out, uint32_t capacity, int32_t lockToken, uint32_t* bitMask)
{
    const uint32_t ne = hp.m_hashNumBuckets * VH_HASH_BUCKET_SIZE;
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x + start;
    if (idx >= ne) return;
    VhHashEntry* e = &hd.d_hash[idx];
    const int4 q = load_quad(e);
    const uint32_t off = e->offset;
    const I3 pos = mki3(q.x, q.y, q.z);
    const F3 pw = block_to_world(hp.m_virtualVoxelSize, pos);
    const F3 df = mk3(pw.x - cx, pw.y - cy, pw.z - cz);
    const float d = sqrtf(dot3(df, df));
    if (q.w != VH_FREE_ENTRY && d >= radius) {
        bool emit = false;
        if (off != 0u || hash_pos(hp.m_hashNumBuckets, pos) != idx / VH_HASH_BUCKET_SIZE) {
            emit = delete_hash_entry_element(hd, hp, pos, lockToken);
        } else {
            append_heap(hd, (uint32_t)q.w / VH_SDF_BLOCK_VOXELS);
            delete_hash_entry(e);
            bucket_dec(hd, idx);
            emit = true;
        }
        if (emit) {
            const uint32_t addr = atomicAdd(outCounter, 1u);
            if (addr < capacity) {
                VhSDFBlockDesc dsc;
                dsc.pos[0] = q.x; dsc.pos[1] = q.y; dsc.pos[2] = q.z; dsc.ptr = q.w;
                out[addr] = dsc;
                const uint32_t bit = chunk_bit_of_block(hp, pos);
                if (bitMask && bit != 0xffffffffu) atomicOr(&bitMask[bit >> 5], 1u << (bit & 31u));
            }
        }
    }
}
__global__ __launch_bounds__(64) void k_stream_out_pass1(VhHashData hd, VhHashParams hp, uint32_t start, float radius, float cx, float cy, float cz,
                                                         uint32_t* outCounter, VhSDFBlockDesc* out, uint32_t capacity, int32_t lockToken)
{
    stream_out_scan(hd, hp, start, radius, cx, cy, cz, outCounter, out, capacity, lockToken, nullptr);
}
__global__ __launch_bounds__(64) void k_stream_out_pass1_bits(VhHashData hd, VhHashParams hp, uint32_t start, float radius, float cx, float cy, float cz,
                                                              uint32_t* outCounter, VhSDFBlockDesc* out, uint32_t capacity, int32_t lockToken, uint32_t* bitMask)
{
    stream_out_scan(hd, hp, start, radius, cx, cy, cz, outCounter, out, capacity, lockToken, bitMask);
}

// The same scan without the deletes: how many blocks of the part would the pass move out?  (A frame loop that knows its
// poses ahead asks this a frame early -- after that frame's alloc, the last pass that adds blocks -- and keeps the
// whole streaming step out of the next frame's launches when the answer is none: Reconstruction::frame.)
__global__ __launch_bounds__(256) void k_stream_out_probe(VhHashData hd, VhHashParams hp, uint32_t start, uint32_t n, float radius,
                                                          float cx, float cy, float cz, uint32_t* counter)
{
    const uint32_t ne = hp.m_hashNumBuckets * VH_HASH_BUCKET_SIZE;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, idx = t + start;
    bool would = false;
    if (t < n && idx < ne) {
        const int4 q = load_quad(&hd.d_hash[idx]);
        const F3 pw = block_to_world(hp.m_virtualVoxelSize, mki3(q.x, q.y, q.z));
        const F3 df = mk3(pw.x - cx, pw.y - cy, pw.z - cz);
        would = q.w != VH_FREE_ENTRY && sqrtf(dot3(df, df)) >= radius;
    }
    const unsigned long long m = __ballot(would);
    if (m != 0ull && lane_id() == 0u) atomicAdd(counter, (uint32_t)__popcll(m));
}

// after a message's words: a release fence, then the tag with system scope -- a host that sees the tag finds the words
VHD void publish_tag(uint32_t* mapped, uint32_t tag)
{
    __atomic_thread_fence(__ATOMIC_RELEASE);
    __hip_atomic_store(&mapped[2], tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// {*src, tag} into mapped host memory like k_publish_words, and the device word back to zero for the next use
__global__ void k_publish_and_clear(uint32_t* src, uint32_t* mapped, uint32_t tag)
{
    mapped[0] = *src;
    mapped[1] = 0u;
    *src = 0u;
    publish_tag(mapped, tag);
}

// integrateFromGlobalHashPass2Kernel :97-113 (copy block out, clear source)
VHD void stream_out_copy_and_clear(const VhHashData& hd, const VhSDFBlockDesc* descs, VhVoxel* out, uint32_t n)
{
    const uint32_t b = blockIdx.x;
    if (b >= n) return;
    const int ptr = __builtin_amdgcn_readfirstlane(descs[b].ptr);
    uint4* src = reinterpret_cast<uint4*>(&hd.d_SDFBlocks[(uint32_t)ptr]) + threadIdx.x;
    reinterpret_cast<uint4*>(out)[(size_t)b * 256 + threadIdx.x] = *src;
    *src = make_uint4(0u, 0u, 0u, 0u);
}
__global__ __launch_bounds__(256) void k_stream_out_pass2(VhHashData hd, const VhSDFBlockDesc* descs, VhVoxel* out, uint32_t n)
{
    stream_out_copy_and_clear(hd, descs, out, n);
}

// k_stream_out_pass2 for a caller that has not read the count: as many workgroups as blocks there can be at most, each
// looks the count up
__global__ __launch_bounds__(256) void k_stream_out_pass2_counted(VhHashData hd, const VhSDFBlockDesc* descs, VhVoxel* out, const uint32_t* counter, uint32_t capacity)
{
    stream_out_copy_and_clear(hd, descs, out, min(*counter, capacity));
}

// {count of the pass, 0, tag} into mapped host memory, behind the pass's copies in the stream: a host thread that sees the
// tag finds the copied blocks in its staging buffer
__global__ void k_publish_count(const uint32_t* counter, uint32_t* mapped, uint32_t tag)
{
    mapped[0] = *counter;
    mapped[1] = 0u;
    publish_tag(mapped, tag);
}

// The stream-in pass for a caller that does not read the heap counter back: chunkToGlobalHashPass1Kernel / Pass2Kernel
// with the counter looked up on the device, the chunk's bit cleared in the device's copy of the bit mask, and a third
// launch that settles the pass.  A block that finds no slot is listed as {index in the pass, SDF block it took} in
// failed[1 ..] and its heap slot is marked, so that pass 2 leaves the block zero; the commit returns those blocks to the
// heap and sets the chunk's bit again.  After the three launches the device state is final, and the host learns (mapped
// memory) which blocks of its staging copy to file back into its grid:
//   {blocks that found no slot, 0, tag, 1 if the heap held too few free blocks (nothing was done), their indices ...}
constexpr uint32_t kStreamInNoSlot = 0xffffffffu;
__global__ __launch_bounds__(64) void k_stream_in_pass1_dev(VhHashData hd, VhHashParams hp, uint32_t n, const VhSDFBlockDesc* descs, int32_t lockToken,
                                                            uint32_t* failed, uint32_t* bitMask, uint32_t chunkBit)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t heapCountPrev = hd.d_heapCounter[0];
    if (n > heapCountPrev + 1u) return; // (k_stream_in_commit reports it; the host puts the blocks back into its grid)
    if (i == 0u && bitMask && chunkBit != 0xffffffffu) atomicAnd(&bitMask[chunkBit >> 5], ~(1u << (chunkBit & 31u)));
    const uint32_t id = hd.d_heap[heapCountPrev - i];
    const VhSDFBlockDesc dsc = descs[i];
    if (!insert_hash_entry(hd, hp, mki3(dsc.pos[0], dsc.pos[1], dsc.pos[2]), (int)(id * VH_SDF_BLOCK_VOXELS), lockToken)) {
        atomicAdd(&hd.d_state[VH_STATE_INSERT_FAILED], 1u);
        const uint32_t k = atomicAdd(&failed[0], 1u);
        failed[1u + 2u * k] = i;
        failed[2u + 2u * k] = id;
        hd.d_heap[heapCountPrev - i] = kStreamInNoSlot; // (above the counter once the pass is committed)
    }
}
__global__ __launch_bounds__(256) void k_stream_in_pass2_dev(VhHashData hd, uint32_t n, const VhVoxel* blocks)
{
    const uint32_t b = blockIdx.x;
    if (b >= n) return;
    const uint32_t heapCountPrev = hd.d_heapCounter[0];
    if (n > heapCountPrev + 1u) return;
    const uint32_t id = hd.d_heap[heapCountPrev - b];
    if (id == kStreamInNoSlot) return; // (a free block: zero already)
    *(reinterpret_cast<uint4*>(&hd.d_SDFBlocks[id * VH_SDF_BLOCK_VOXELS]) + threadIdx.x) = reinterpret_cast<const uint4*>(blocks)[(size_t)b * 256 + threadIdx.x];
}
__global__ void k_stream_in_commit(VhHashData hd, uint32_t n, uint32_t* failed, uint32_t* bitMask, uint32_t chunkBit, uint32_t* mapped, uint32_t tag)
{
    const uint32_t heapCountPrev = hd.d_heapCounter[0];
    const bool exhausted = n > heapCountPrev + 1u;
    const uint32_t nFailed = failed[0];
    if (!exhausted) {
        // consumeHeap n times, then appendHeap (DSC/VoxelUtilHashSDF.h:525-529) of the blocks that found no slot
        const uint32_t counter = heapCountPrev - n;
        for (uint32_t k = 0; k < nFailed; k++) {
            hd.d_heap[counter + 1u + k] = failed[2u + 2u * k];
            mapped[4u + k] = failed[1u + 2u * k];
        }
        hd.d_heapCounter[0] = counter + nFailed;
        if (nFailed != 0u && bitMask && chunkBit != 0xffffffffu) atomicOr(&bitMask[chunkBit >> 5], 1u << (chunkBit & 31u));
    } else {
        atomicAdd(&hd.d_state[VH_STATE_HEAP_UNDERFLOW], 1u);
    }
    failed[0] = 0u; // (for the next pass)
    mapped[0] = nFailed;
    mapped[1] = 0u;
    mapped[3] = exhausted ? 1u : 0u;
    publish_tag(mapped, tag);
}

// chunkToGlobalHashPass1Kernel :143-160
__global__ __launch_bounds__(64) void k_stream_in_pass1(VhHashData hd, VhHashParams hp, uint32_t n, uint32_t heapCountPrev,
                                                        const VhSDFBlockDesc* descs, int32_t lockToken)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t ptr = hd.d_heap[heapCountPrev - i] * VH_SDF_BLOCK_VOXELS;
    const VhSDFBlockDesc dsc = descs[i];
    if (!insert_hash_entry(hd, hp, mki3(dsc.pos[0], dsc.pos[1], dsc.pos[2]), (int)ptr, lockToken)) atomicAdd(&hd.d_state[VH_STATE_INSERT_FAILED], 1u);
}

// chunkToGlobalHashPass2Kernel :181-189
__global__ __launch_bounds__(256) void k_stream_in_pass2(VhHashData hd, uint32_t n, uint32_t heapCountPrev, const VhVoxel* blocks)
{
    const uint32_t b = blockIdx.x;
    if (b >= n) return;
    const uint32_t ptr = hd.d_heap[heapCountPrev - b] * VH_SDF_BLOCK_VOXELS;
    *(reinterpret_cast<uint4*>(&hd.d_SDFBlocks[ptr]) + threadIdx.x) = reinterpret_cast<const uint4*>(blocks)[(size_t)b * 256 + threadIdx.x];
}

} // namespace

extern "C" {

int vh_stream_out_pass1(const VhHashData* hd, const VhHashParams* hp, uint32_t threadsPerPart, uint32_t start,
                        float radius, const float camPos[3], uint32_t* d_outputCounter, VhSDFBlockDesc* d_output,
                        uint32_t outputCapacity, int32_t lockToken, vhStream_t stream)
{
    if (!hd || !hp || !camPos || !d_outputCounter || !d_output) return VH_ERR_BAD_ARGUMENT;
    if (threadsPerPart == 0) return VH_OK; // DSC/CUDASceneRepChunkGrid.cu:81
    k_stream_out_pass1<<<cdiv(threadsPerPart, 64), 64, 0, (hipStream_t)stream>>>(*hd, *hp, start, radius, camPos[0], camPos[1], camPos[2],
                                                                                   d_outputCounter, d_output, outputCapacity, lockToken);
    return vh_last_launch_error();
}

int vh_stream_out_probe(const VhHashData* hd, const VhHashParams* hp, uint32_t threadsPerPart, uint32_t start, float radius,
                        const float camPos[3], uint32_t* d_counter, uint32_t* d_mapped, uint32_t tag, vhStream_t stream)
{
    if (!hd || !hp || !camPos || !d_counter || !d_mapped) return VH_ERR_BAD_ARGUMENT;
    if (threadsPerPart != 0) {
        // (the pass itself runs whole workgroups of 64: it looks at up to 63 entries beyond its part, and so must its probe --
        // the count is used as an upper bound)
        const uint32_t scanned = cdiv(threadsPerPart, 64) * 64u;
        k_stream_out_probe<<<cdiv(scanned, 256), 256, 0, (hipStream_t)stream>>>(*hd, *hp, start, scanned, radius, camPos[0], camPos[1], camPos[2], d_counter);
    }
    k_publish_and_clear<<<1, 1, 0, (hipStream_t)stream>>>(d_counter, d_mapped, tag);
    return vh_last_launch_error();
}

int vh_stream_out_pass2(const VhHashData* hd, const VhHashParams* hp, const VhSDFBlockDesc* d_descs,
                        VhVoxel* d_output, uint32_t nSDFBlocks, vhStream_t stream)
{
    (void)hp;
    if (!hd || !d_descs || !d_output) return VH_ERR_BAD_ARGUMENT;
    if (nSDFBlocks == 0) return VH_OK;
    k_stream_out_pass2<<<nSDFBlocks, 256, 0, (hipStream_t)stream>>>(*hd, d_descs, d_output, nSDFBlocks);
    return vh_last_launch_error();
}

int vh_stream_out_device(const VhHashData* hd, const VhHashParams* hp, uint32_t threadsPerPart, uint32_t start, float radius,
                         const float camPos[3], uint32_t* d_outputCounter, VhSDFBlockDesc* d_descs, VhVoxel* d_blocks,
                         uint32_t mostBlocks, int32_t lockToken, uint32_t* d_bitMask, vhStream_t stream)
{
    if (!hd || !hp || !camPos || !d_outputCounter || !d_descs || !d_blocks) return VH_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    VH_HIP(hipMemsetAsync(d_outputCounter, 0, sizeof(uint32_t), s));
    if (threadsPerPart == 0 || mostBlocks == 0) return VH_OK;
    k_stream_out_pass1_bits<<<cdiv(threadsPerPart, 64), 64, 0, s>>>(*hd, *hp, start, radius, camPos[0], camPos[1], camPos[2], d_outputCounter, d_descs,
                                                                     mostBlocks, lockToken, d_bitMask);
    k_stream_out_pass2_counted<<<mostBlocks, 256, 0, s>>>(*hd, d_descs, d_blocks, d_outputCounter, mostBlocks);
    return vh_last_launch_error();
}

int vh_publish_count(const uint32_t* d_counter, uint32_t* d_mapped, uint32_t tag, vhStream_t stream)
{
    if (!d_counter || !d_mapped) return VH_ERR_BAD_ARGUMENT;
    k_publish_count<<<1, 1, 0, (hipStream_t)stream>>>(d_counter, d_mapped, tag);
    return vh_last_launch_error();
}

int vh_stream_in_device(const VhHashData* hd, const VhHashParams* hp, uint32_t n, const VhSDFBlockDesc* d_descs, const VhVoxel* d_blocks,
                        int32_t lockToken, uint32_t* d_failed, uint32_t* d_bitMask, uint32_t chunkBit, uint32_t* d_mapped, uint32_t tag,
                        vhStream_t stream)
{
    if (!hd || !hp || !d_descs || !d_blocks || !d_failed || !d_mapped) return VH_ERR_BAD_ARGUMENT;
    if (hp->m_hashNumBuckets < 2) return VH_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    if (n != 0) {
        k_stream_in_pass1_dev<<<cdiv(n, 64), 64, 0, s>>>(*hd, *hp, n, d_descs, lockToken, d_failed, d_bitMask, chunkBit);
        k_stream_in_pass2_dev<<<n, 256, 0, s>>>(*hd, n, d_blocks);
    }
    k_stream_in_commit<<<1, 1, 0, s>>>(*hd, n, d_failed, d_bitMask, chunkBit, d_mapped, tag);
    return vh_last_launch_error();
}

int vh_stream_in_pass1(const VhHashData* hd, const VhHashParams* hp, uint32_t n, uint32_t heapCountPrev,
                       const VhSDFBlockDesc* d_descs, int32_t lockToken, vhStream_t stream)
{
    if (!hd || !hp || !d_descs) return VH_ERR_BAD_ARGUMENT;
    if (n == 0) return VH_OK;
    if (n > heapCountPrev + 1u) return VH_ERR_HEAP_EXHAUSTED;
    if (hp->m_hashNumBuckets < 2) return VH_ERR_BAD_ARGUMENT;
    k_stream_in_pass1<<<cdiv(n, 64), 64, 0, (hipStream_t)stream>>>(*hd, *hp, n, heapCountPrev, d_descs, lockToken);
    return vh_last_launch_error();
}

int vh_stream_in_pass2(const VhHashData* hd, const VhHashParams* hp, uint32_t n, uint32_t heapCountPrev,
                       const VhSDFBlockDesc* d_descs, const VhVoxel* d_blocks, vhStream_t stream)
{
    (void)hp; (void)d_descs;
    if (!hd || !d_blocks) return VH_ERR_BAD_ARGUMENT;
    if (n == 0) return VH_OK;
    if (n > heapCountPrev + 1u) return VH_ERR_HEAP_EXHAUSTED;
    k_stream_in_pass2<<<n, 256, 0, (hipStream_t)stream>>>(*hd, n, heapCountPrev, d_blocks);
    return vh_last_launch_error();
}

// {*src0, *src1, tag} into mapped host memory, the tag last and with system scope: a host that polls the tag reads
// the two words without a stream synchronisation or a copy (each costs a blocking driver call; the streaming passes of
// a frame need two such read-backs)
__global__ void k_publish_words(const uint32_t* src0, const uint32_t* src1, uint32_t* mapped, uint32_t tag)
{
    mapped[0] = src0 ? *src0 : 0u;
    mapped[1] = src1 ? *src1 : 0u;
    publish_tag(mapped, tag);
}

int vh_publish_words(const uint32_t* d_src0, const uint32_t* d_src1, uint32_t* d_mapped, uint32_t tag, vhStream_t stream)
{
    if (!d_mapped) return VH_ERR_BAD_ARGUMENT;
    k_publish_words<<<1, 1, 0, (hipStream_t)stream>>>(d_src0, d_src1, d_mapped, tag);
    return vh_last_launch_error();
}

} // extern "C"
