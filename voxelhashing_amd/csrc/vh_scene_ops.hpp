// vh_scene_ops.hpp -- what the scene operations (vh_merge.hip, vh_resample.hip, vh_cut.hip, vh_deintegrate.hip) and the
// mesh units (through vh_mesh_table.hpp) share around their rules: the one-atomic-per-wave list helpers, the striped
// counts of a work header, the passes that settle lost lock races, and the delete pass.  Each unit keeps its own enum of
// which header word means what; only the geometry is here.  Not for the frame loop (vh_kernels.hip includes none of it).
#pragma once

#include "vh_device.hpp"
#include "vh_host_util.hpp"

namespace {

// ---- wave-level lists

// this lane's position in the run that the lanes of the ballot `m` (not empty) append to a list that *counter counts: one
// atomic per wave.  Every lane of the wave calls it.
VHD uint32_t wave_run(uint64_t m, uint32_t* counter)
{
    const int leader = __ffsll((unsigned long long)m) - 1;
    uint32_t base = 0u;
    if ((int)vhd::lane_id() == leader) base = atomicAdd(counter, (uint32_t)__popcll(m));
    base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
    return base + (uint32_t)__popcll(m & vhd::lanemask_lt());
}

// base of `keep` lanes' run in a list that *counter counts.  Every lane of the wave calls it.
VHD uint32_t wave_append(bool keep, uint32_t* counter)
{
    const uint64_t m = __ballot(keep);
    return m == 0ull ? 0u : wave_run(m, counter);
}

// `v` appended to list[*counter ...] by every lane with `take`; every lane of the wave calls it.  (Not through the form
// above: that no lane stores after an empty ballot, which ends the wave's work here, the compiler does not see there.)
VHD void wave_append(bool take, uint32_t v, uint32_t* counter, uint32_t* list)
{
    const uint64_t m = __ballot(take);
    if (m == 0ull) return;
    const uint32_t at = wave_run(m, counter);
    if (take) list[at] = v;
}

// counts the lanes with `flag` into *counter: one atomic per wave.  Every lane of the wave calls it.
VHD void wave_count(bool flag, uint32_t* counter)
{
    const uint64_t m = __ballot(flag);
    if (m == 0ull) return;
    if ((int)vhd::lane_id() == __ffsll((unsigned long long)m) - 1) atomicAdd(counter, (uint32_t)__popcll(m));
}

// ---- the work header and its striped counts
//
// d_work starts with a header of a few single words and, from a word a unit names (W_VOXELS, W_COUNTS, ...), kStripes
// groups of kStripeWords words, each group in a cache line of its own.  A workgroup adds to the group its index picks;
// the host sums them.  (On one word the 35 000 atomics of a merge of 8 800 blocks queued up behind each other for
// 0.37 ms, twelve times what the voxels take: DESIGN.md section 6 "Scene merge".)
constexpr uint32_t kStripes = 32;
constexpr uint32_t kStripeWords = 16;

// the stripe of workgroup `group`; base: the header's first striped word
VHD uint32_t* stripe_of(uint32_t* base, uint32_t group) { return base + (group % kStripes) * kStripeWords; }

// word `which` of every stripe, summed; h: the header read back, base: the index of its first striped word
inline uint32_t stripes_sum(const uint32_t* h, uint32_t base, uint32_t which)
{
    uint32_t sum = 0u;
    for (uint32_t k = 0; k < kStripes; k++) sum += h[base + k * kStripeWords + which];
    return sum;
}

inline int read_header(const uint32_t* d_work, uint32_t* h, uint32_t words, hipStream_t s)
{
    VH_HIP(hipMemcpyAsync(h, d_work, words * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    VH_HIP(hipStreamSynchronize(s));
    return VH_OK;
}

// Behind the header of an operation that settles lock races: three arrays of n words, a state word per block and two
// pending lists (a pass reads one list and fills the other).
struct SettleArrays {
    uint32_t* blockState;
    uint32_t* pending[2];
};
inline SettleArrays settle_arrays(uint32_t* d_work, uint32_t headerWords, uint32_t n)
{
    uint32_t* blockState = d_work + headerWords;
    return { blockState, { blockState + n, blockState + 2u * (size_t)n } };
}
inline size_t settle_work_bytes(uint32_t headerWords, uint32_t n) { return ((size_t)headerWords + 3u * (size_t)n) * sizeof(uint32_t); }

// ---- the passes that settle lost lock races

struct Settled {
    uint32_t passes, nPending, in; // the passes run, and what was still pending when they stopped: pending[in] lists it
};

// Passes while blocks lose their lock races, the bucket mutexes reset before each but the first (resetHashBucketMutexCUDA:
// the caller's token is fresh again).  launchPass(pendingIn, nIn, pendingOut, outSel, passNumber) enqueues one pass over
// the nIn entries of pendingIn, which appends what lost to pendingOut and counts it in header word pendingWord + outSel;
// the first pass reads a.pending[0] with firstCount entries (or, the callback's choice by passNumber == 0, something
// else of that length).  One list element per bucket and pass gets through its bucket's mutex, and a pass may make no
// progress -- two list inserts each holding the other's second mutex -- so the bound is not one block per pass: the
// callers give the number of blocks + 8.
template <uint32_t kHeaderWords, class LaunchPass>
int settle_passes(const VhHashData* hd, const VhHashParams* hp, vhStream_t stream, uint32_t* d_work, const SettleArrays& a, uint32_t pendingWord,
                  uint32_t firstCount, uint32_t mostPasses, LaunchPass launchPass, Settled* out)
{
    hipStream_t s = (hipStream_t)stream;
    uint32_t h[kHeaderWords];
    uint32_t passes = 0u, in = 0u, nPending = firstCount;
    while (nPending != 0u && passes < mostPasses) {
        if (passes != 0u) VH_TRY(vh_reset_bucket_mutex(hd, hp, stream));
        VH_HIP(hipMemsetAsync(&d_work[pendingWord + (in ^ 1u)], 0, sizeof(uint32_t), s));
        launchPass(a.pending[in], nPending, a.pending[in ^ 1u], in ^ 1u, passes);
        VH_TRY(vh_last_launch_error());
        VH_TRY(read_header(d_work, h, kHeaderWords, s));
        in ^= 1u;
        nPending = h[pendingWord + in];
        passes++;
    }
    *out = { passes, nPending, in };
    return VH_OK;
}

// ---- the delete pass

// One lane per block still pending: deleteHashEntryElement on the listed blocks whose state word has a bit of `mask`,
// which puts the block (all zero since an earlier launch) back on the heap.  The first pass (pendingIn == nullptr) looks
// at every listed block's state word.  A delete that loses a bucket lock is pending for the next pass.
VHD void delete_listed(const VhHashData& hd, const VhHashParams& hp, const VhSDFBlockDesc* descs, int32_t lockToken, const uint32_t* blockState,
                       uint32_t mask, const uint32_t* pendingIn, uint32_t nIn, uint32_t* pendingOut, uint32_t* outCount)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    bool lost = false;
    uint32_t i = 0u;
    if (t < nIn) {
        i = pendingIn ? pendingIn[t] : t;
        if (blockState[i] & mask)
            lost = !vhd::delete_hash_entry_element(hd, hp, vhd::mki3(descs[i].pos[0], descs[i].pos[1], descs[i].pos[2]), lockToken);
    }
    wave_append(lost, i, outCount, pendingOut);
}

} // namespace
