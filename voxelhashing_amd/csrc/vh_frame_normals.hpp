// vh_frame_normals.hpp -- frame loop: k_compute_normals and its three riders -- compactify (CoCompactify), the interval
// splat of the next render (CoSplat) and the pass over the voxels (CoIntegrate, rider_done, pass_rider_group).
// Included by vh_kernels.hip.
#pragma once

#include <cstddef>

#include "vh_device.hpp"
#include "vh_frame_compactify.hpp"
#include "vh_frame_integrate.hpp"
#include "vh_frame_splat.hpp"

namespace {
using namespace vhd;

// Riders of computeNormals' launch.  They come FIRST in the grid (the schedule workgroup, the splat, the compactify
// pass, then the image): each of them is a chain of dependent trips to memory, and what starts first ends first.
struct CoCompactify {
    VhHashData hd;
    VhHashParams hp;
    VhDepthCameraParams cp;
    uint32_t groups; // 0: nothing to co-launch
};

// The interval splat of the NEXT render, for the pose of the frame being integrated.  It lists the table as it stands
// before that frame's pass over the voxels: what the pass frees stays listed with all-zero voxels (weight 0: read
// like an absent block), what the next alloc adds is not listed and is empty anyway.
struct CoSplat {
    VhRayCastParams rp; // view of the next render
    VhDepthCameraParams cp;
    uint4* heads;
    int4* lists;
    uint32_t* sched;
    uint32_t* feedback;
    uint32_t cap, phase, numCUs, nSplatGroups;
    uint32_t groups; // nSplatGroups (+ sched_groups() with a schedule); 0: nothing to co-launch
};

// The frame's pass over the voxels (integrate + starve + GC) as a third rider: the LAST workgroups of the launch, two launches
// a frame instead of three.  The pass needs the compactified list, which this launch's compactify workgroups make, and it
// frees blocks, which edits the table this launch's splat workgroups read.
//   * A workgroup of the pass polls ITS entry of the list (pass_rider_group): the entry is there as soon as the compactify
//     workgroup that found the block has written it, and its last word says so (rider_tag).  The compactify workgroups also
//     count themselves off when their part of the list is out (rider_done), and the last one raises flags (rider_wait): that
//     is how the pass learns that the list is complete -- for its length, which it needs afterwards -- and how a workgroup
//     beyond the end of the list learns that it has nothing to do.  (The first version waited for the flags before it read
//     anything: 1.4 us a frame more.)
//   * The frees and the splat need no order (free_block_cold): the splat lists every live block whatever happens, and a freed
//     one or not -- which is all the same to the ray cast it is made for.  (The first version had the splat workgroups count
//     themselves off too and the frees wait for them: 0.4 us a frame for nothing.)
// A wait cannot be in vain: the hardware starts a launch's workgroups in grid order, so what a workgroup of the pass waits
// for is running or done when it starts (and every wait gives up after ~1 s: VH_STATE_RIDER_GAVE_UP, never seen).
// Between workgroups of ONE launch the eight XCDs' L2s are not coherent, and a release / acquire pair at agent scope is the
// writer writing its whole L2 back and the reader dropping its own (buffer_wbl2 / buffer_inv per workgroup: measured, +30 us
// a frame).  The list is the only data that crosses: it is written through and read at the coherence point (list_store), the
// counters and flags are relaxed agent-scope atomics, and the writers wait for their stores before they count.
// What it buys (cfg2, tools/riders_stamps.py): the compactify workgroups are done 1.6 - 4.9 us into the launch (four trips to
// memory each, ~1 us on a busy machine), the pass's workgroups 6.4 - 8.9 us, beside the splat's 8.1; the launch alone ended at
// ~8 us and a launch of the pass would then ramp up and take its own ~6 us: 4.8 us less per frame at 640x480 (350 blocks in
// view), 5 us at 1080p (1200 blocks).  With more blocks than the launch has workgroups for the pass (2048) a workgroup takes
// several, one after the other: at 2500 - 5800 blocks (cfg3) that costs 1.4 us a frame more than it saves, at 8600 (the dense
// scene) it saves 2.3 -- the scene keeps the pass in a launch of its own, whose wave-per-block shape is made for such lists.
struct CoIntegrate {
    FusedArgs args;
    uint32_t* done;          // VH_RIDER_DONE_WORDS words: flags, class counters, top counter (rider_done; never reset)
    uint32_t listExpected, listClassExpected;   // what the compactify workgroups' top counter / class counters read once this launch's are done: the flags are set to the first then
    uint32_t riderTag;       // the tag of this launch's list entries (rider_tag)
    uint32_t first;          // the pass's first workgroup in the grid
    uint32_t groups;         // 0: nothing to co-launch
};
struct NormalsKernargs { // (the argument block of k_compute_normals, for the offset of the pass's arguments in it)
    float4* out; const float4* in; uint32_t width, height; CoCompactify job; CoSplat splat; CoIntegrate integ;
};
// A compactify workgroup, the i-th of n, has made its part of the list and counts itself off.  Counting on one word would
// not do: same-address atomics are served one after the other, ~12 ns each, and a launch has up to 1 000 of them (measured
// with the splat's 2 000 workgroups counting too: the launch twice as long).  So the workgroups count in
// VH_RIDER_DONE_COUNTERS classes (i mod 32, a counter each, 128 bytes apart), the last of a class counts the class off on a
// top counter, and the last class raises the flags.  Nothing is ever reset -- the host keeps what each word reads when all
// launches so far are done -- so every class must grow by the same amount in every launch: n rounded up to a multiple of 32,
// the workgroups whose i + 32 falls into the padding counting for two (n > 32 there).  A stage of few
// workgroups counts on the top counter alone.
constexpr uint32_t kRiderFewGroups = 128; // a stage of up to this many workgroups counts on one word (the launcher's totals follow: rider_totals)
VHD void rider_done(const CoIntegrate& integ, const uint32_t i, const uint32_t n)
{
    if (integ.groups == 0u) return;
    // every thread's stores to the list have arrived (written through, list_store: waiting for them is all a release has to
    // do here)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    if (threadIdx.x < kWave) {
        uint32_t* const words = integ.done; // flags, class counters, top counter
        const uint32_t padded = (n + VH_RIDER_DONE_COUNTERS - 1u) / VH_RIDER_DONE_COUNTERS * VH_RIDER_DONE_COUNTERS;
        const uint32_t add = (i + VH_RIDER_DONE_COUNTERS >= n && i + VH_RIDER_DONE_COUNTERS < padded) ? 2u : 1u;
        uint32_t last = 0;
        if (threadIdx.x == 0) {
            if (n <= kRiderFewGroups) { // few enough to count on the top counter itself: a trip to memory less before the flags go up
                last = __hip_atomic_fetch_add(&words[2u * VH_RIDER_DONE_COUNTERS * 32u], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == integ.listExpected ? 1u : 0u;
            } else {
                const uint32_t before = __hip_atomic_fetch_add(&words[(VH_RIDER_DONE_COUNTERS + i % VH_RIDER_DONE_COUNTERS) * 32u], add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (before + add == integ.listClassExpected)
                    last = __hip_atomic_fetch_add(&words[2u * VH_RIDER_DONE_COUNTERS * 32u], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == integ.listExpected ? 1u : 0u;
            }
        }
        last = (uint32_t)__shfl((int)last, 0);
        if (last && threadIdx.x < (uint32_t)VH_RIDER_DONE_COUNTERS)
            __hip_atomic_store(&words[threadIdx.x * 32u], integ.listExpected, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// (host) what a stage of g workgroups that counts itself off with rider_done adds to the totals the host keeps
// (VhFrameJob::listDoneTotal, listClassTotal): a class grows by g rounded up to 32s, over 32, and the top counter by 32
inline void rider_totals(uint32_t g, uint32_t& doneTotal, uint32_t& classTotal)
{
    if (g > kRiderFewGroups) classTotal += cdiv(g, VH_RIDER_DONE_COUNTERS);
    doneTotal += g > kRiderFewGroups ? VH_RIDER_DONE_COUNTERS : g; // (few workgroups count on the top counter alone)
}

// A workgroup of the pass as a rider: block `group` of the list, then (with more than `groups` blocks) group + groups, ...
// It does not wait for the list to be complete before it starts: it polls ITS entry, which is there as soon as the compactify
// workgroup that found the block has written it (the entry's tag says so: rider_tag, the last word list_store writes) -- on
// average a microsecond before the slowest compactify workgroup is done, and without the trip for the count and the flag's own
// way through memory (0.9 us).  The count it needs only afterwards: to know whether the list goes on beyond the launch's
// workgroups, and, in workgroup 0, for the host's mirror.
struct PassRiderShared {
    FusedShared<false> fused;
    int4 q;
    uint32_t have, count;
};
template <uint32_t KERNARG_OFFSET>
VHD void pass_rider_group(const CoIntegrate& integ, const uint32_t group, PassRiderShared& sh)
{
    const FusedArgs& args = integ.args;
    const VhHashEntry* const list = args.hd.d_hashCompactified;
    const uint32_t nEntries = args.hp.m_hashNumBuckets * VH_HASH_BUCKET_SIZE;
    const float thr = get_truncation(args.hp, args.cp.m_sensorDepthWorldMax);
    // 1. this workgroup's entry, or the end of the list (every lane of the wave reads the same words: one request each)
    if (threadIdx.x < kWave) {
        uint32_t have = 0u;
        if (group < nEntries) {
            const uint32_t* const flag = integ.done + (blockIdx.x % VH_RIDER_DONE_COUNTERS) * 32u;
            const uint64_t* const tagWord = reinterpret_cast<const uint64_t*>(&list[group]) + 3;
            for (uint32_t polls = 0; polls < (1u << 22); polls++) { // (an exit every wave reaches, as rider_wait)
                // both words in flight together: a poll is one trip to memory
                const uint64_t w = __hip_atomic_load(tagWord, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t f = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((uint32_t)(w >> 32) == integ.riderTag) { have = 1u; break; }
                if ((int32_t)(f - integ.listExpected) >= 0) break; // the list is complete (step 2 looks again)
                __builtin_amdgcn_s_sleep(2);
            }
        }
        int4 q = make_int4(0, 0, 0, 0);
        if (have) q = list_quad<true>(&list[group]);
        if (threadIdx.x == 0) { sh.q = q; sh.have = have; }
    }
    __syncthreads();
    const bool early = sh.have != 0u;
    if (early) integrate_block_by_workgroup<true, KERNARG_OFFSET>(args, sh.fused, sh.q, group, thr);
    // 2. the whole list
    if (threadIdx.x < kWave) {
        uint32_t count = 0u;
        if (rider_wait(integ.done, integ.listExpected)) count = (uint32_t)__hip_atomic_load(args.hd.d_hashCompactifiedCounter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if (threadIdx.x == 0) atomicAdd(&args.hd.d_state[VH_STATE_RIDER_GAVE_UP], 1u); // (what is left of its share stays undone)
        if (threadIdx.x == 0) sh.count = count;
    }
    __syncthreads();
    const uint32_t count = sh.count;
    // host-visible copy of the block count and the caller's tag (as integrate_fused_body)
    if (args.countMirror && group == 0u && threadIdx.x == 0) *reinterpret_cast<uint2*>(args.countMirror) = make_uint2(count, args.mirrorTag);
    for (uint32_t b = group; b < count; b += integ.groups) {
        if (b == group && early) continue;
        __syncthreads(); // (the previous block's reads of the shared words are done)
        integrate_block_by_workgroup<true, KERNARG_OFFSET>(args, sh.fused, list_quad<true>(&list[b]), b, thr);
    }
}

// computeNormalsDevice, DSC/CameraUtil.cu:669-697
__global__ __launch_bounds__(256) void k_compute_normals(float4* out, const float4* in, uint32_t width, uint32_t height, CoCompactify job, CoSplat splat, CoIntegrate integ)
{
    __shared__ union RiderShared { SplatShared splat; CompactShared compact; PassRiderShared pass; } shared;
    SplatShared& sh = shared.splat;
    uint32_t g = blockIdx.x;
    if (integ.groups != 0u && g >= integ.first) {
        static_assert(kRiderFewGroups >= VH_RIDER_DONE_COUNTERS && VH_RIDER_DONE_COUNTERS <= kWave, "one lane per flag");
#if defined(VH_KNOCKOUT) && VH_KNOCKOUT == 42
        const uint32_t riderStamp0 = (uint32_t)__builtin_amdgcn_s_memrealtime();
        uint4* const riderStampAt = reinterpret_cast<uint4*>(job.hd.d_hashCompactified) + (job.hp.m_hashNumBuckets * VH_HASH_BUCKET_SIZE) / 2u + blockIdx.x;
#endif
        pass_rider_group<(uint32_t)(offsetof(NormalsKernargs, integ) + offsetof(CoIntegrate, args))>(integ, g - integ.first, shared.pass);
#if defined(VH_KNOCKOUT) && VH_KNOCKOUT == 42
        __syncthreads();
        if (threadIdx.x == 0) *riderStampAt = make_uint4(riderStamp0, (uint32_t)__builtin_amdgcn_s_memrealtime(), 5u, 0x5742u);
#endif
        return;
    }
#if defined(VH_KNOCKOUT) && VH_KNOCKOUT == 42 // measurement build: every workgroup's life by kind, read by tools/riders_stamps.py
    const uint32_t stamp0 = (uint32_t)__builtin_amdgcn_s_memrealtime();
    uint4* const stampAt = reinterpret_cast<uint4*>(job.hd.d_hashCompactified) + (job.hp.m_hashNumBuckets * VH_HASH_BUCKET_SIZE) / 2u + blockIdx.x;
#define VH_GROUP_STAMP(KIND) { __syncthreads(); if (threadIdx.x == 0) *stampAt = make_uint4(stamp0, (uint32_t)__builtin_amdgcn_s_memrealtime(), (KIND), 0x5742u); }
#else
#define VH_GROUP_STAMP(KIND)
#endif
#if defined(VH_KNOCKOUT) && VH_KNOCKOUT >= 31 && VH_KNOCKOUT <= 34 // measurement builds: the riders of this launch, one at a time
    {
        const uint32_t nSchedK = splat.groups - splat.nSplatGroups;
        const bool isSched = g < nSchedK, isCompact = !isSched && g - nSchedK < job.groups, isSplat = !isSched && !isCompact && g < splat.groups + job.groups;
        if (VH_KNOCKOUT == 31 && isSched) return;               // no schedule workgroups
        if (VH_KNOCKOUT == 32 && (isSched || isSplat)) return;  // no splat at all
        if (VH_KNOCKOUT == 33 && isCompact) return;             // no compactify
        if (VH_KNOCKOUT == 34 && !isSched && !isCompact && !isSplat) return; // no normals
    }
#endif
    // the schedule workgroups first (the longest chains), then compactify (the pass over the voxels, if it rides, waits for
    // its list), then the table's slices
    const uint32_t nSched = splat.groups - splat.nSplatGroups;
    if (g >= nSched && g - nSched < job.groups) {
        g -= nSched;
        if (integ.groups != 0u) compactify_group<true>(job.hd, job.hp, job.cp, g * blockDim.x + threadIdx.x, shared.compact, integ.riderTag);
        else compactify_group<false>(job.hd, job.hp, job.cp, g * blockDim.x + threadIdx.x, shared.compact);
        VH_GROUP_STAMP(3u)
        rider_done(integ, g, job.groups);
        return;
    }
    if (g >= nSched) g -= job.groups;
    if (g < splat.groups) {
        const uint32_t group = g < nSched ? splat.nSplatGroups + g : g - nSched;
        interval_splat_group(job.hd, job.hp, splat.cp, splat.rp, splat.heads, splat.lists, splat.cap, splat.sched, splat.phase, splat.numCUs,
                             splat.nSplatGroups, splat.feedback, group, sh);
        VH_GROUP_STAMP(group >= splat.nSplatGroups ? 1u : 2u)
        return;
    }
    g -= splat.groups;
    const uint32_t idx = g * blockDim.x + threadIdx.x;
#if defined(VH_KNOCKOUT) && VH_KNOCKOUT == 42
    if (job.groups != 0u && idx < width * height) {
#else
    if (idx >= width * height) return;
    {
#endif
    const uint32_t x = idx % width, y = idx / width;
    const float mi = minf();
    float4 o = make_float4(mi, mi, mi, mi);
    if (x > 0 && x < width - 1 && y > 0 && y < height - 1) {
        const float4 CC = in[idx], PC = in[idx + width], CP = in[idx + 1], MC = in[idx - width], CM = in[idx - 1];
        if (CC.x != mi && PC.x != mi && CP.x != mi && MC.x != mi && CM.x != mi) {
            const F3 a = mk3(PC.x - MC.x, PC.y - MC.y, PC.z - MC.z), b = mk3(CP.x - CM.x, CP.y - CM.y, CP.z - CM.z);
            const F3 n = mk3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
            const float l = sqrtf(dot3(n, n));
            if (l > 0.0f) o = make_float4(n.x / -l, n.y / -l, n.z / -l, 1.0f);
        }
    }
    out[idx] = o;
    }
#if defined(VH_KNOCKOUT) && VH_KNOCKOUT == 42
    if (job.groups != 0u) VH_GROUP_STAMP(4u)
#endif
}
#undef VH_GROUP_STAMP

} // namespace
