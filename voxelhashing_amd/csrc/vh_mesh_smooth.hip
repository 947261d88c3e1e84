// vh_mesh_smooth.hip -- Taubin smoothing of an indexed mesh in fixed point on the device (not in the reference;
// DESIGN.md section 4, "Mesh smoothing").
//
// The distinct undirected edges of the faces are the neighbour relation (uniform umbrella operator).  Positions are
// rounded to integers once, q = rint(p * 2^scale), and every half step replaces a moved vertex's q by
// q + ((f u + 2^15) >> 16) with u the rounded mean of (q_j - q) over its neighbours j, f = lambda on even and mu on odd
// half steps, all from the q of the half step before (two arrays, never in place).  Sums are 64-bit integers, so the
// result does not depend on the order the atomics ran in.  Launches: edges (one lane per face), degree (one lane per
// edge slot), prepare (one lane per vertex), then per half step gather (one lane per edge slot) and step (one lane per
// vertex), finish (one lane per vertex).
//
// What the passes rely on inside a launch is the RESULT of an atomic and nothing else: an edge slot's key is written
// once, by the compare-and-swap that finds it empty; use counts, degrees, sums and counts are atomics, the boundary
// marks stores of the one value 1, and all of them are read only by a later launch.
#include <hip/hip_runtime.h>

#include <cmath>

#include "vh_device.hpp"
#include "vh_host_util.hpp"
#include "vh_mesh_key.hpp"
#include "vh_mesh_table.hpp"

using namespace vhd;

namespace {

// d_work: what the passes count, published by the finish pass if no launch has left a status
constexpr uint32_t kWorkEdges = 0u, kWorkBoundaryEdges = 1u, kWorkMoved = 2u, kWorkBoundary = 3u, kWorkIsolated = 4u, kWorkWords = 5u;
constexpr uint32_t kFlagBoundary = 1u, kFlagMoved = 2u; // d_flags
constexpr long long kLimit = 1ll << 40;

// the lanes' status bits into the word: one atomic per wave that has any.  Every lane of the wave calls it.
VHD void smooth_status(uint32_t status, uint32_t* statusWord)
{
    const uint64_t any = __ballot(status != 0u);
    if (any == 0ull) return;
    uint32_t bits = 0u;
    for (uint32_t b = 1u; b <= VH_SMOOTH_DEGREE; b <<= 1) bits |= __ballot((status & b) != 0u) != 0ull ? b : 0u;
    if ((int)lane_id() == __ffsll((unsigned long long)any) - 1) atomicOr(statusWord, bits);
}

// One lane per face.  An index >= numVertices is reported before anything is read through it.  A face without a
// repeated index puts its three edges into the table (lo | hi << 32, lo < hi: never all ones) and adds one to each
// slot's use count.
__global__ __launch_bounds__(256) void k_smooth_edges(const uint32_t* faces, uint32_t numVertices, uint32_t numFaces, VhMeshSmoothData d)
{
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t status = 0u;
    if (f < numFaces) {
        const uint32_t i0 = faces[3u * f], i1 = faces[3u * f + 1u], i2 = faces[3u * f + 2u];
        if (i0 >= numVertices || i1 >= numVertices || i2 >= numVertices) status = VH_SMOOTH_BAD_INDEX;
        else if (i0 != i1 && i1 != i2 && i0 != i2) {
            const uint32_t a[3] = { i0, i1, i2 }, b[3] = { i1, i2, i0 };
#pragma unroll 1
            for (int e = 0; e < 3; e++) { // (one copy of the probe loop)
                const uint64_t key = (uint64_t)min(a[e], b[e]) | ((uint64_t)max(a[e], b[e]) << 32);
                const uint32_t slot = weld_find_or_claim(reinterpret_cast<unsigned long long*>(d.d_edgeKeys), key, d.m_edgeSlotsLog2);
                if (slot == kNoSlot) status = VH_SMOOTH_TABLE_FULL;
                else atomicAdd(&d.d_edgeUses[slot], 1u);
            }
        }
    }
    smooth_status(status, &d.d_counts[VH_SMOOTH_STATUS]);
}

// One lane per edge slot; nothing happens once a launch before this one has left a status.  An occupied slot adds one
// to both ends' degree and marks both ends if one face alone names the edge; edges and boundary edges are counted with
// one atomic per wave.  (A dense list of the edges for the half steps to run over was measured and bought nothing:
// DESIGN.md section 6.)
__global__ __launch_bounds__(256) void k_smooth_degree(VhMeshSmoothData d)
{
    if (d.d_counts[VH_SMOOTH_STATUS] != 0u) return; // written by the launch before this one: uniform
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x, numSlots = 1u << d.m_edgeSlotsLog2;
    const uint64_t key = s < numSlots ? d.d_edgeKeys[s] : kMeshKeyEmpty;
    const bool edge = key != kMeshKeyEmpty;
    const bool boundary = edge && d.d_edgeUses[s] == 1u;
    wave_count(edge, &d.d_work[kWorkEdges]);
    wave_count(boundary, &d.d_work[kWorkBoundaryEdges]);
    if (!edge) return;
    const uint32_t lo = (uint32_t)key, hi = (uint32_t)(key >> 32);
    atomicAdd(&d.d_degree[lo], 1u);
    atomicAdd(&d.d_degree[hi], 1u);
    if (boundary) { d.d_flags[lo] = kFlagBoundary; d.d_flags[hi] = kFlagBoundary; }
}

// (int64) rint((double) x * scale) when that is finite and within 2^40; scale is a power of two, so the product is exact
VHD bool smooth_quantise(float x, double scale, long long* q)
{
    const double s = (double)x * scale;
    *q = 0ll;
    if (!(fabs(s) <= 1099511627776.0)) return false; // 2^40 (NaN fails the comparison)
    *q = (long long)rint(s);
    return true;
}

// One lane per vertex; nothing happens once a launch before this one has left a status.  The range and degree tests;
// the position in fixed point goes into both position arrays (a vertex that does not move is never written again), the
// sums become zero, and the flags say from here on whether the vertex moves.
__global__ __launch_bounds__(256) void k_smooth_prepare(const VhVertex* vertices, uint32_t numVertices, uint32_t keepBoundary, double scale, VhMeshSmoothData d)
{
    if (d.d_counts[VH_SMOOTH_STATUS] != 0u) return; // (as k_smooth_degree)
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t status = 0u;
    bool moved = false, boundary = false, isolated = false;
    if (v < numVertices) {
        const VhVertex r = vertices[v];
        long long q[3];
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 3; j++) ok = smooth_quantise(r.p[j], scale, &q[j]) && ok;
        if (!ok) status = VH_SMOOTH_RANGE;
        const uint32_t n = d.d_degree[v];
        if (n > VH_SMOOTH_MAX_DEGREE) status |= VH_SMOOTH_DEGREE;
        boundary = (d.d_flags[v] & kFlagBoundary) != 0u;
        isolated = n == 0u;
        moved = !isolated && !(keepBoundary != 0u && boundary);
        d.d_flags[v] = (boundary ? kFlagBoundary : 0u) | (moved ? kFlagMoved : 0u);
        int64_t* a = d.d_positions + 3ull * v;
        int64_t* b = d.d_positions + 3ull * numVertices + 3ull * v;
#pragma unroll
        for (int j = 0; j < 3; j++) { a[j] = q[j]; b[j] = q[j]; d.d_sums[3ull * v + j] = 0ll; }
    }
    wave_count(moved, &d.d_work[kWorkMoved]);
    wave_count(boundary, &d.d_work[kWorkBoundary]);
    wave_count(isolated, &d.d_work[kWorkIsolated]);
    smooth_status(status, &d.d_counts[VH_SMOOTH_STATUS]);
}

// One lane per edge slot: each end of an edge that moves gets the other end's position of the half step's input added
// to its sums.
__global__ __launch_bounds__(256) void k_smooth_gather(const long long* in, VhMeshSmoothData d)
{
    if (d.d_counts[VH_SMOOTH_STATUS] != 0u) return; // (as k_smooth_degree)
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= (1u << d.m_edgeSlotsLog2)) return;
    const uint64_t key = d.d_edgeKeys[s];
    if (key == kMeshKeyEmpty) return;
    const uint32_t lo = (uint32_t)key, hi = (uint32_t)(key >> 32);
    const bool toLo = (d.d_flags[lo] & kFlagMoved) != 0u, toHi = (d.d_flags[hi] & kFlagMoved) != 0u;
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(d.d_sums);
    if (toLo) {
#pragma unroll
        for (int j = 0; j < 3; j++) atomicAdd(&sums[3ull * lo + j], (unsigned long long)in[3ull * hi + j]);
    }
    if (toHi) {
#pragma unroll
        for (int j = 0; j < 3; j++) atomicAdd(&sums[3ull * hi + j], (unsigned long long)in[3ull * lo + j]);
    }
}

// floor((2 d + n) / (2 n)) on signed values: d / n rounded to the nearest integer, halves up -- the rule of the cluster
// mean (vh_mesh_cluster.hip keeps its own copy, so that its kernels stay what they are).  1 <= n <= 2^16, |d| < 2^57.
VHD long long smooth_mean(long long sum, uint32_t n)
{
    const long long a = 2ll * sum + (long long)n, b = 2ll * (long long)n;
    long long q = a / b;
    if (a % b != 0ll && a < 0ll) q--;
    return q;
}

// One lane per vertex.  A moved vertex's half step from `in` to `out`, and its sums back to zero for the next one.
// |f u| < 2^16 * 2^42: nothing overflows before the range test.
__global__ __launch_bounds__(256) void k_smooth_step(const long long* in, long long* out, uint32_t numVertices, int32_t factorQ16, VhMeshSmoothData d)
{
    if (d.d_counts[VH_SMOOTH_STATUS] != 0u) return; // (as k_smooth_degree)
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t status = 0u;
    if (v < numVertices && (d.d_flags[v] & kFlagMoved) != 0u) {
        const uint32_t n = d.d_degree[v];
#pragma unroll 1
        for (int j = 0; j < 3; j++) { // (one copy of the 64-bit division)
            const long long q = in[3ull * v + j];
            const long long u = smooth_mean(d.d_sums[3ull * v + j] - (long long)n * q, n);
            const long long moved = q + (((long long)factorQ16 * u + 32768ll) >> 16);
            if (moved > kLimit || moved < -kLimit) status = VH_SMOOTH_RANGE;
            out[3ull * v + j] = moved;
            d.d_sums[3ull * v + j] = 0ll;
        }
    }
    smooth_status(status, &d.d_counts[VH_SMOOTH_STATUS]);
}

// One lane per vertex; nothing happens once a launch before this one has left a status, so that a status writes no
// vertex.  A moved vertex's position from `in` (int64 -> double and the power of two are exact: one rounding, to
// float) with its colour, every other vertex as it came; the first lane publishes the counts.
__global__ __launch_bounds__(256) void k_smooth_finish(const VhVertex* vertices, const long long* in, uint32_t numVertices, double invScale, VhMeshSmoothData d)
{
    if (d.d_counts[VH_SMOOTH_STATUS] != 0u) return; // (as k_smooth_degree)
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v == 0u) {
        d.d_counts[VH_SMOOTH_MOVED] = d.d_work[kWorkMoved];
        d.d_counts[VH_SMOOTH_BOUNDARY] = d.d_work[kWorkBoundary];
        d.d_counts[VH_SMOOTH_ISOLATED] = d.d_work[kWorkIsolated];
        d.d_counts[VH_SMOOTH_EDGES] = d.d_work[kWorkEdges];
        d.d_counts[VH_SMOOTH_BOUNDARY_EDGES] = d.d_work[kWorkBoundaryEdges];
    }
    if (v >= numVertices) return;
    const VhVertex r = vertices[v];
    const bool moved = (d.d_flags[v] & kFlagMoved) != 0u;
    VhVertex w;
    w.p[0] = moved ? (float)((double)in[3ull * v] * invScale) : r.p[0];
    w.p[1] = moved ? (float)((double)in[3ull * v + 1u] * invScale) : r.p[1];
    w.p[2] = moved ? (float)((double)in[3ull * v + 2u] * invScale) : r.p[2];
    w.c[0] = r.c[0]; w.c[1] = r.c[1]; w.c[2] = r.c[2];
    d.d_vertices[v] = w;
}

// the smallest power of two >= 6 numFaces (twice the most edges), 64 slots at least
uint32_t smoothSlotsLog2(uint32_t numFaces)
{
    uint32_t l = 6;
    while (l < 31 && (1ull << l) < 6ull * numFaces) l++;
    return l;
}

} // namespace

extern "C" {

int vh_mesh_smooth_default_slots_log2(uint32_t numFaces, uint32_t* slotsLog2)
{
    if (!slotsLog2 || numFaces > 0x15555555u) return VH_ERR_BAD_ARGUMENT; // 6 F <= 2^31
    *slotsLog2 = smoothSlotsLog2(numFaces);
    return VH_OK;
}

int vh_mesh_smooth(const VhVertex* d_vertices, const uint64_t* d_keys, const uint32_t* d_faces, uint32_t numVertices, uint32_t numFaces, uint32_t iterations,
                   int32_t lambdaQ16, int32_t muQ16, uint32_t keepBoundary, int32_t scaleLog2, const VhMeshSmoothData* data, vhStream_t stream)
{
    (void)d_keys; // the keys stay the mesh's: the pass neither reads nor writes them
    if (!data || !data->d_counts || !data->d_work) return VH_ERR_BAD_ARGUMENT;
    if (iterations < 1u || iterations > VH_SMOOTH_MAX_ITERATIONS || keepBoundary > 1u || scaleLog2 < -100 || scaleLog2 > 100) return VH_ERR_BAD_ARGUMENT;
    if (lambdaQ16 < -VH_SMOOTH_MAX_FACTOR_Q16 || lambdaQ16 > VH_SMOOTH_MAX_FACTOR_Q16 || muQ16 < -VH_SMOOTH_MAX_FACTOR_Q16 || muQ16 > VH_SMOOTH_MAX_FACTOR_Q16)
        return VH_ERR_BAD_ARGUMENT;
    if (numVertices > 0x40000000u || numFaces > 0x15555555u || data->m_edgeSlotsLog2 > 31u) return VH_ERR_BAD_ARGUMENT; // 3 F face offsets and edges in 32 bits
    if (numVertices != 0 && (!d_vertices || !data->d_degree || !data->d_flags || !data->d_positions || !data->d_sums || !data->d_vertices)) return VH_ERR_BAD_ARGUMENT;
    if (numVertices != 0 && numFaces != 0 && (!d_faces || !data->d_edgeKeys || !data->d_edgeUses)) return VH_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    VH_HIP(hipMemsetAsync(data->d_counts, 0, sizeof(uint32_t) * VH_SMOOTH_NUM_COUNTS, s));
    if (numVertices == 0) return VH_OK; // an empty mesh, and no launch with an empty grid
    const size_t slots = (size_t)1 << data->m_edgeSlotsLog2;
    long long* q[2] = { reinterpret_cast<long long*>(data->d_positions), reinterpret_cast<long long*>(data->d_positions) + 3 * (size_t)numVertices };
    VH_HIP(hipMemsetAsync(data->d_work, 0, sizeof(uint32_t) * kWorkWords, s));
    VH_HIP(hipMemsetAsync(data->d_degree, 0, sizeof(uint32_t) * numVertices, s));
    VH_HIP(hipMemsetAsync(data->d_flags, 0, sizeof(uint32_t) * numVertices, s));
    if (numFaces != 0) {
        VH_HIP(hipMemsetAsync(data->d_edgeKeys, 0xff, sizeof(uint64_t) * slots, s));
        VH_HIP(hipMemsetAsync(data->d_edgeUses, 0, sizeof(uint32_t) * slots, s));
        VH_LAUNCH_TIMED(k_smooth_edges, cdiv(numFaces, 256), 256, s, d_faces, numVertices, numFaces, *data);
        VH_TRY(vh_last_launch_error());
        VH_LAUNCH_TIMED(k_smooth_degree, cdiv(slots, 256), 256, s, *data);
        VH_TRY(vh_last_launch_error());
    }
    VH_LAUNCH_TIMED(k_smooth_prepare, cdiv(numVertices, 256), 256, s, d_vertices, numVertices, keepBoundary, std::ldexp(1.0, scaleLog2), *data);
    VH_TRY(vh_last_launch_error());
    if (numFaces != 0) { // (without a face nothing moves)
        for (uint32_t k = 0; k < 2u * iterations; k++) {
            VH_LAUNCH_TIMED(k_smooth_gather, cdiv(slots, 256), 256, s, q[k & 1u], *data);
            VH_TRY(vh_last_launch_error());
            VH_LAUNCH_TIMED(k_smooth_step, cdiv(numVertices, 256), 256, s, q[k & 1u], q[(k & 1u) ^ 1u], numVertices, (k & 1u) ? muQ16 : lambdaQ16, *data);
            VH_TRY(vh_last_launch_error());
        }
    }
    VH_LAUNCH_TIMED(k_smooth_finish, cdiv(numVertices, 256), 256, s, d_vertices, q[0], numVertices, std::ldexp(1.0, -scaleLog2), *data); // 2 N half steps end in the first array
    return vh_last_launch_error();
}

} // extern "C"
