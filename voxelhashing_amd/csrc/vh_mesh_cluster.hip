// vh_mesh_cluster.hip -- decimates a welded mesh by vertex clustering on the device (Rossignac-Borrel; not in the
// reference; DESIGN.md section 4, "Mesh clustering").
//
// The lattice of voxel corners is cut into cubes of m points a side.  Every vertex falls into the cube of its key's
// lattice point (vh_mesh_cluster_key_of), a cube's vertices become one vertex at their integer mean, a face whose
// corners fall into fewer than three cubes goes, and of the faces over one set of three cubes one stays.  Grouping is by
// integer keys and the sums are integers, so the result does not depend on the order the atomics ran in.  Four
// launches: insert (one lane per vertex), faces (one lane per face), number (one lane per cluster slot), emit (one lane
// per face slot).
//
// What the passes rely on inside a launch is the RESULT of an atomic and nothing else: a slot word is written once, by
// the compare-and-swap that finds it empty, and never changes, so a plain load that sees a value sees the final one and
// a stale "empty" only sends the lane to the compare-and-swap, which returns the truth.  The sums, counts, winding bits
// and used marks are atomics (or stores of one value) whose results nobody reads before the next launch.
#include <hip/hip_runtime.h>

#include <cmath>

#include "vh_device.hpp"
#include "vh_host_util.hpp"
#include "vh_mesh_key.hpp"
#include "vh_mesh_table.hpp"

using namespace vhd;

namespace {

constexpr uint32_t kNoValue = 0xffffffffu;
constexpr uint32_t kWorkCollapsed = 0u, kWorkEntered = 1u; // d_work: the face pass's two counts, published by the number pass

// the lanes' status bits into the word: one atomic per wave that has any.  Every lane of the wave calls it.
VHD void cluster_status(uint32_t status, uint32_t* statusWord)
{
    const uint64_t any = __ballot(status != 0u);
    if (any == 0ull) return;
    uint32_t bits = 0u;
    for (uint32_t b = 1u; b <= VH_CLUSTER_BAD_INDEX; b <<= 1) bits |= __ballot((status & b) != 0u) != 0ull ? b : 0u;
    if ((int)lane_id() == __ffsll((unsigned long long)any) - 1) atomicOr(statusWord, bits);
}

// (int64) rint((double) x * scale) when that is finite and within 2^40; scale is a power of two, so the product is exact
VHD bool cluster_quantise(float x, double scale, long long* q)
{
    const double s = (double)x * scale;
    if (!(fabs(s) <= 1099511627776.0)) return false; // 2^40 (NaN fails the comparison)
    *q = (long long)rint(s);
    return true;
}

// One lane per vertex: the slot of its cluster's key, claimed if nobody has it; its position (times `scale`) and colour
// (times 2^16) rounded to integers and added to the slot's six sums, one to its count; the slot remembered.  A key that
// is no vertex key, a component out of range and a full table are reported, and the vertex then adds nothing.
__global__ __launch_bounds__(256) void k_cluster_insert(const VhVertex* vertices, const uint64_t* keys, uint32_t numVertices, uint32_t cellsPerCluster,
                                                        double scale, VhMeshClusterData c)
{
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t status = 0u;
    if (v < numVertices) {
        uint32_t slot = kNoSlot;
        uint64_t key = 0ull;
        long long q[6];
        if (!vh_mesh_cluster_key_of(keys[v], cellsPerCluster, &key)) status = VH_CLUSTER_BAD_KEY;
        else {
            const VhVertex r = vertices[v];
            bool ok = true;
#pragma unroll
            for (int j = 0; j < 3; j++) ok = cluster_quantise(r.p[j], scale, &q[j]) && ok;
#pragma unroll
            for (int j = 0; j < 3; j++) ok = cluster_quantise(r.c[j], 65536.0, &q[3 + j]) && ok;
            if (!ok) status = VH_CLUSTER_RANGE;
            else {
                slot = weld_find_or_claim(reinterpret_cast<unsigned long long*>(c.d_clusterKeys), key, c.m_clusterSlotsLog2);
                if (slot == kNoSlot) status = VH_CLUSTER_TABLE_FULL;
                else {
                    unsigned long long* sums = reinterpret_cast<unsigned long long*>(c.d_clusterSums) + 6ull * slot;
#pragma unroll
                    for (int j = 0; j < 6; j++) atomicAdd(&sums[j], (unsigned long long)q[j]);
                    atomicAdd(&c.d_clusterCount[slot], 1u);
                }
            }
        }
        c.d_vertexSlot[v] = slot;
    }
    cluster_status(status, &c.d_counts[VH_CLUSTER_STATUS]);
}

// the slot of the triple (pair, third) in the face table, claimed if nobody has it; kNoSlot after numSlots steps.  A
// slot is two words, each written once: the pair by a compare-and-swap from empty, then the third the same way.  Who
// finds either word set to something else probes on -- so does every other face over the same triple, at the same slot:
// they all end in one slot, and nobody waits for anybody.
VHD uint32_t cluster_face_slot(unsigned long long* pairs, uint32_t* thirds, uint64_t pair, uint32_t third, uint32_t slotsLog2)
{
    const uint32_t numSlots = 1u << slotsLog2, mask = numSlots - 1u;
    uint32_t slot = weld_home(pair ^ ((uint64_t)third * 0x9e3779b97f4a7c15ull), mask);
#pragma unroll 1
    for (uint32_t step = 0; step < numSlots; step++) {
        unsigned long long have = pairs[slot];
        if (have == kMeshKeyEmpty) have = atomicCAS(&pairs[slot], (unsigned long long)kMeshKeyEmpty, (unsigned long long)pair);
        if (have == kMeshKeyEmpty || have == pair) {
            uint32_t has = thirds[slot];
            if (has == kNoValue) has = atomicCAS(&thirds[slot], kNoValue, third);
            if (has == kNoValue || has == third) return slot;
        }
        slot = (slot + 1u) & mask;
    }
    return kNoSlot;
}

// One lane per face.  An index >= numVertices is reported before anything is read through it.  The three vertices'
// cluster slots; a face with two in one cluster is counted as collapsed and leaves; the others find the slot of their
// sorted slot triple in the face table, set the bit of their winding there and mark their three clusters as used.  The
// winding is read off the cluster keys: with the smallest key first, bit 0 if the second key is below the third.
__global__ __launch_bounds__(256) void k_cluster_faces(const uint32_t* faces, uint32_t numVertices, uint32_t numFaces, VhMeshClusterData c)
{
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t status = 0u;
    bool collapsed = false, entered = false;
    if (f < numFaces) {
        const uint32_t i0 = faces[3u * f], i1 = faces[3u * f + 1u], i2 = faces[3u * f + 2u];
        if (i0 >= numVertices || i1 >= numVertices || i2 >= numVertices) status = VH_CLUSTER_BAD_INDEX;
        else {
            const uint32_t s0 = c.d_vertexSlot[i0], s1 = c.d_vertexSlot[i1], s2 = c.d_vertexSlot[i2];
            if (s0 != kNoSlot && s1 != kNoSlot && s2 != kNoSlot) { // (a vertex without a slot has reported itself)
                collapsed = s0 == s1 || s1 == s2 || s0 == s2;
                if (!collapsed) {
                    const uint64_t k0 = c.d_clusterKeys[s0], k1 = c.d_clusterKeys[s1], k2 = c.d_clusterKeys[s2];
                    // rotated so that the smallest key comes first, the other two are (k1, k2), (k2, k0) or (k0, k1)
                    const bool ascending = (k0 < k1 && k0 < k2) ? k1 < k2 : (k1 < k2 ? k2 < k0 : k0 < k1);
                    const uint32_t lo = min(s0, min(s1, s2)), hi = max(s0, max(s1, s2)), mid = s0 ^ s1 ^ s2 ^ lo ^ hi;
                    const uint32_t slot = cluster_face_slot(reinterpret_cast<unsigned long long*>(c.d_facePairs), c.d_faceThirds,
                                                            ((uint64_t)lo << 32) | mid, hi, c.m_faceSlotsLog2);
                    if (slot == kNoSlot) status = VH_CLUSTER_TABLE_FULL;
                    else {
                        entered = true;
                        atomicOr(&c.d_faceWindings[slot], ascending ? 1u : 2u);
                        c.d_clusterIndex[s0] = 1u; c.d_clusterIndex[s1] = 1u; c.d_clusterIndex[s2] = 1u;
                    }
                }
            }
        }
    }
    wave_count(collapsed, &c.d_work[kWorkCollapsed]);
    wave_count(entered, &c.d_work[kWorkEntered]);
    cluster_status(status, &c.d_counts[VH_CLUSTER_STATUS]);
}

// floor((2 sum + n) / (2 n)) on signed values: the mean rounded to the nearest integer, halves up.  n >= 1, |sum| < 2^60.
VHD long long cluster_mean(long long sum, uint32_t n)
{
    const long long a = 2ll * sum + (long long)n, b = 2ll * (long long)n;
    long long q = a / b;
    if (a % b != 0ll && a < 0ll) q--;
    return q;
}

// One lane per cluster slot; nothing happens once a launch before this one has left a status.  A slot that a face
// marked takes the next vertex index (one atomic per wave), and its vertex is written: the integer mean of each sum
// times 2^-scale (int64 -> double and the power of two are exact: one rounding, to float), and the cluster key.  The
// slot's index word then holds the vertex index.  An occupied slot without a mark is counted as unused.  The first
// lane publishes the face pass's two counts; the emit pass takes the faces it writes off the second.
__global__ __launch_bounds__(256) void k_cluster_number(double invScale, VhMeshClusterData c)
{
    if (c.d_counts[VH_CLUSTER_STATUS] != 0u) return; // written by the launches before this one: uniform
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x, numSlots = 1u << c.m_clusterSlotsLog2;
    if (s == 0u) {
        c.d_counts[VH_CLUSTER_COLLAPSED] = c.d_work[kWorkCollapsed];
        c.d_counts[VH_CLUSTER_DUPLICATES] = c.d_work[kWorkEntered];
    }
    const uint64_t key = s < numSlots ? c.d_clusterKeys[s] : kMeshKeyEmpty;
    const bool used = key != kMeshKeyEmpty && c.d_clusterIndex[s] != 0u;
    const uint32_t at = wave_append(used, &c.d_counts[VH_CLUSTER_VERTICES]);
    wave_count(key != kMeshKeyEmpty && !used, &c.d_counts[VH_CLUSTER_UNUSED]);
    if (s >= numSlots) return;
    c.d_clusterIndex[s] = used ? at : kNoValue;
    if (!used) return;
    const uint32_t n = c.d_clusterCount[s];
    float* out = c.d_vertices[at].p; // p[3], then c[3]: six floats
#pragma unroll 1
    for (int j = 0; j < 6; j++) { // (one copy of the 64-bit division)
        const long long mean = n != 0u ? cluster_mean(c.d_clusterSums[6ull * s + j], n) : 0ll; // (a marked cluster has a member)
        out[j] = (float)((double)mean * (j < 3 ? invScale : 1.0 / 65536.0));
    }
    c.d_keys[at] = key;
}

// One lane per face slot; nothing happens once a launch before this one has left a status.  An occupied slot gives one
// face: its three clusters ordered by key, (first, second, third) if a face of that winding fell here, else (first,
// third, second), through the numbering, at the end of the face list (one atomic per wave).  What is written comes off
// the count of the faces that entered the table: the duplicates are left.
__global__ __launch_bounds__(256) void k_cluster_emit(VhMeshClusterData c)
{
    if (c.d_counts[VH_CLUSTER_STATUS] != 0u) return; // (as k_cluster_number)
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x, numSlots = 1u << c.m_faceSlotsLog2;
    const uint64_t pair = s < numSlots ? c.d_facePairs[s] : kMeshKeyEmpty;
    const bool keep = pair != kMeshKeyEmpty;
    uint32_t a = 0u, b = 0u, d = 0u;
    if (keep) {
        a = (uint32_t)(pair >> 32); b = (uint32_t)pair; d = c.d_faceThirds[s];
        uint64_t ka = c.d_clusterKeys[a], kb = c.d_clusterKeys[b], kd = c.d_clusterKeys[d];
        if (kb < ka) { const uint32_t t = a; a = b; b = t; const uint64_t k = ka; ka = kb; kb = k; }
        if (kd < kb) { const uint32_t t = b; b = d; d = t; const uint64_t k = kb; kb = kd; kd = k; }
        if (kb < ka) { const uint32_t t = a; a = b; b = t; }
        if ((c.d_faceWindings[s] & 1u) == 0u) { const uint32_t t = b; b = d; d = t; }
        a = c.d_clusterIndex[a]; b = c.d_clusterIndex[b]; d = c.d_clusterIndex[d];
    }
    const uint64_t m = __ballot(keep);
    if (m == 0ull) return; // wave-uniform
    const uint32_t at = wave_append(keep, &c.d_counts[VH_CLUSTER_FACES]);
    if ((int)lane_id() == __ffsll((unsigned long long)m) - 1) atomicSub(&c.d_counts[VH_CLUSTER_DUPLICATES], (uint32_t)__popcll(m));
    if (!keep) return;
    c.d_faces[3u * at] = a; c.d_faces[3u * at + 1u] = b; c.d_faces[3u * at + 2u] = d;
}

// the smallest power of two >= 2 n, 64 slots at least
uint32_t clusterSlotsLog2(uint32_t n)
{
    uint32_t l = 6;
    while (l < 31 && (1ull << l) < 2ull * n) l++;
    return l;
}

} // namespace

extern "C" {

int vh_mesh_cluster_key(uint64_t vertexKey, uint32_t cellsPerCluster, uint64_t* key)
{
    if (!key || cellsPerCluster < 1u || cellsPerCluster > VH_CLUSTER_MAX_CELLS) return VH_ERR_BAD_ARGUMENT;
    return vh_mesh_cluster_key_of(vertexKey, cellsPerCluster, key) ? VH_OK : VH_ERR_BAD_ARGUMENT;
}

int vh_mesh_cluster_default_scale_log2(float voxelSize, int32_t* scaleLog2)
{
    if (!scaleLog2 || !(voxelSize > 0.0f) || !std::isfinite(voxelSize)) return VH_ERR_BAD_ARGUMENT;
    // floor(log2(v)) from the exponent: v = m 2^e with m in [1/2, 1), so the floor is e - 1
    int e = 0;
    (void)std::frexp((double)voxelSize, &e);
    *scaleLog2 = 16 - (e - 1);
    return VH_OK;
}

int vh_mesh_cluster_default_slots_log2(uint32_t count, uint32_t* slotsLog2)
{
    if (!slotsLog2 || count > 0x40000000u) return VH_ERR_BAD_ARGUMENT;
    *slotsLog2 = clusterSlotsLog2(count);
    return VH_OK;
}

int vh_mesh_cluster(const VhVertex* d_vertices, const uint64_t* d_keys, const uint32_t* d_faces, uint32_t numVertices, uint32_t numFaces,
                    uint32_t cellsPerCluster, int32_t scaleLog2, const VhMeshClusterData* data, vhStream_t stream)
{
    if (!data || !data->d_counts || !data->d_work) return VH_ERR_BAD_ARGUMENT;
    if (cellsPerCluster < 1u || cellsPerCluster > VH_CLUSTER_MAX_CELLS || scaleLog2 < -100 || scaleLog2 > 100) return VH_ERR_BAD_ARGUMENT;
    if (numVertices > 0x40000000u || numFaces > 0x40000000u) return VH_ERR_BAD_ARGUMENT; // twice as many slots, and 3 F face offsets, in 32 bits
    if (data->m_clusterSlotsLog2 > 31u || data->m_faceSlotsLog2 > 31u) return VH_ERR_BAD_ARGUMENT;
    if (numVertices != 0 && (!d_vertices || !d_keys || !data->d_clusterKeys || !data->d_clusterSums || !data->d_clusterCount || !data->d_clusterIndex ||
                             !data->d_vertexSlot || !data->d_vertices || !data->d_keys))
        return VH_ERR_BAD_ARGUMENT;
    if (numFaces != 0 && (!d_faces || !data->d_facePairs || !data->d_faceThirds || !data->d_faceWindings || !data->d_faces)) return VH_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    VH_HIP(hipMemsetAsync(data->d_counts, 0, sizeof(uint32_t) * VH_CLUSTER_NUM_COUNTS, s));
    if (numVertices == 0) return VH_OK; // an empty mesh, and no launch with an empty grid
    const size_t clusterSlots = (size_t)1 << data->m_clusterSlotsLog2, faceSlots = (size_t)1 << data->m_faceSlotsLog2;
    VH_HIP(hipMemsetAsync(data->d_work, 0, sizeof(uint32_t) * 2, s));
    VH_HIP(hipMemsetAsync(data->d_clusterKeys, 0xff, sizeof(uint64_t) * clusterSlots, s));
    VH_HIP(hipMemsetAsync(data->d_clusterSums, 0, sizeof(int64_t) * 6 * clusterSlots, s));
    VH_HIP(hipMemsetAsync(data->d_clusterCount, 0, sizeof(uint32_t) * clusterSlots, s));
    VH_HIP(hipMemsetAsync(data->d_clusterIndex, 0, sizeof(uint32_t) * clusterSlots, s));
    VH_LAUNCH_TIMED(k_cluster_insert, cdiv(numVertices, 256), 256, s, d_vertices, d_keys, numVertices, cellsPerCluster, std::ldexp(1.0, scaleLog2), *data);
    VH_TRY(vh_last_launch_error());
    if (numFaces != 0) {
        VH_HIP(hipMemsetAsync(data->d_facePairs, 0xff, sizeof(uint64_t) * faceSlots, s));
        VH_HIP(hipMemsetAsync(data->d_faceThirds, 0xff, sizeof(uint32_t) * faceSlots, s));
        VH_HIP(hipMemsetAsync(data->d_faceWindings, 0, sizeof(uint32_t) * faceSlots, s));
        VH_LAUNCH_TIMED(k_cluster_faces, cdiv(numFaces, 256), 256, s, d_faces, numVertices, numFaces, *data);
        VH_TRY(vh_last_launch_error());
    }
    VH_LAUNCH_TIMED(k_cluster_number, cdiv(clusterSlots, 256), 256, s, std::ldexp(1.0, -scaleLog2), *data);
    VH_TRY(vh_last_launch_error());
    if (numFaces == 0) return VH_OK; // every cluster is unused
    VH_LAUNCH_TIMED(k_cluster_emit, cdiv(faceSlots, 256), 256, s, *data);
    return vh_last_launch_error();
}

} // extern "C"
