// vh_mesh.hip -- welds the marching-cubes triangle soup into an indexed mesh on the device (not in the reference, which
// downloads the soup and merges it on the host with mLib's mergeCloseVertices; DESIGN.md section 4, "Indexed mesh").
//
// Every vertex of the soup lies on an edge of the lattice of voxel corners, or on a lattice point when vertexInterp
// snapped it, and the sourced pass 2 (vh_mc.hip) says which.  Keyed by that (vh_mesh_key.hpp) the weld needs no
// distance search: an open-addressing table with linear probing takes one slot per key, the cell with the smallest
// (z, y, x) among those that share the key gives the vertex its bits, and the result does not depend on the order of
// the soup.  Three launches: insert (one lane per soup vertex), number (eight slots per lane), faces (one lane per
// triangle).  Vertex and face order come from atomics, as the soup's does.
#include <hip/hip_runtime.h>

#include <cstring>

#include "vh_device.hpp"
#include "vh_host_util.hpp"
#include "vh_mesh_key.hpp"

using namespace vhd;

namespace {

// the slot a key starts probing at (the 64-bit finaliser of MurmurHash3)
VHD uint32_t weld_home(uint64_t k, uint32_t mask)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (uint32_t)k & mask;
}

// base of `keep` lanes' run in a list that *counter counts: one atomic per wave.  Every lane of the wave calls it.
VHD uint32_t wave_append(bool keep, uint32_t* counter)
{
    const uint64_t m = __ballot(keep);
    if (m == 0ull) return 0u;
    const int leader = __ffsll((unsigned long long)m) - 1;
    uint32_t base = 0u;
    if ((int)lane_id() == leader) base = atomicAdd(counter, (uint32_t)__popcll(m));
    base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
    return base + (uint32_t)__popcll(m & lanemask_lt());
}

constexpr uint32_t kNoSlot = 0xffffffffu;

// One lane per soup vertex i = 3 * triangle + corner: claim the slot of its key, bid for the slot's vertex with
// rank << 32 | i (the smallest wins), remember the slot.  The probe walks at most numSlots steps.
__global__ __launch_bounds__(256) void k_weld_insert(const VhTriangleSource* sources, uint32_t numVertices, VhMeshWeldData w, uint32_t slotsLog2)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= numVertices) return;
    const uint32_t t = i / 3u, k = i - 3u * t;
    const VhTriangleSource src = sources[t];
    const uint32_t code = (src.edges >> (8u * k)) & 0xffu;
    uint64_t key = 0ull;
    uint32_t rank = 0u;
    // (bits 6-7 of a vertex's code are not defined: a record that sets them is malformed)
    if ((code >> 6) != 0u || !vh_mesh_key(src.cell[0], src.cell[1], src.cell[2], code & 0xfu, (code >> 4) & 3u, &key, &rank)) {
        atomicOr(&w.d_counts[2], VH_WELD_KEY_RANGE);
        w.d_vertexSlot[i] = kNoSlot;
        return;
    }
    const uint32_t numSlots = 1u << slotsLog2, mask = numSlots - 1u;
    uint32_t slot = weld_home(key, mask), found = kNoSlot;
    unsigned long long* slotKeys = reinterpret_cast<unsigned long long*>(w.d_slotKeys);
#pragma unroll 1
    for (uint32_t step = 0; step < numSlots; step++) {
        unsigned long long have = slotKeys[slot];
        if (have == kMeshKeyEmpty) have = atomicCAS(&slotKeys[slot], (unsigned long long)kMeshKeyEmpty, (unsigned long long)key);
        if (have == kMeshKeyEmpty || have == key) { found = slot; break; }
        slot = (slot + 1u) & mask;
    }
    if (found == kNoSlot) atomicOr(&w.d_counts[2], VH_WELD_TABLE_FULL);
    else atomicMin(reinterpret_cast<unsigned long long*>(&w.d_slotWinner[found]), ((unsigned long long)rank << 32) | i);
    w.d_vertexSlot[i] = found;
}

// Numbers the occupied slots: a wave takes 64 * kNumberPerLane consecutive slots (lane-strided, so its loads are
// contiguous), scans its lanes' counts and asks for its run of vertex indices with one atomic -- one per 512 slots: at
// the default table size most waves of one slot per lane would hold a key, and the atomics on the one counter would be
// the whole cost of the kernel.  An occupied slot writes its winner's vertex and its key; the slot's winner word then
// holds the vertex index.  Nothing is numbered once the status word is set.
constexpr uint32_t kNumberPerLane = 8;
__global__ __launch_bounds__(256) void k_weld_number(const VhTriangle* triangles, VhMeshWeldData w, uint32_t slotsLog2)
{
    if (w.d_counts[2] != 0u) return; // written by the launch before this one: uniform
    const uint32_t numSlots = 1u << slotsLog2, lane = lane_id();
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) / (uint32_t)kWave;
    const uint32_t first = wave * ((uint32_t)kWave * kNumberPerLane) + lane; // < numSlots + 2048: the grid covers numSlots once
    uint64_t keys[kNumberPerLane];
    uint32_t mine = 0u;
#pragma unroll
    for (uint32_t j = 0; j < kNumberPerLane; j++) {
        const uint32_t s = first + j * (uint32_t)kWave;
        keys[j] = s < numSlots ? w.d_slotKeys[s] : kMeshKeyEmpty;
        mine += keys[j] != kMeshKeyEmpty ? 1u : 0u;
    }
    uint32_t incl = mine;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, off);
        if ((int)lane >= off) incl += up;
    }
    const uint32_t total = (uint32_t)__shfl((int)incl, kWave - 1);
    if (total == 0u) return; // wave-uniform
    uint32_t base = 0u;
    if (lane == (uint32_t)kWave - 1u) base = atomicAdd(&w.d_counts[0], total);
    base = (uint32_t)__shfl((int)base, kWave - 1);
    uint32_t at = base + incl - mine;
#pragma unroll
    for (uint32_t j = 0; j < kNumberPerLane; j++) {
        if (keys[j] == kMeshKeyEmpty) continue;
        const uint32_t s = first + j * (uint32_t)kWave;
        const uint32_t i = (uint32_t)w.d_slotWinner[s];
        w.d_vertices[at] = reinterpret_cast<const VhVertex*>(triangles)[i];
        w.d_keys[at] = keys[j];
        w.d_slotWinner[s] = at;
        at++;
    }
}

// One lane per triangle: its three indices through the remembered slots; a face with a repeated index is dropped,
// the others keep their winding.
__global__ __launch_bounds__(256) void k_weld_faces(uint32_t numTriangles, VhMeshWeldData w)
{
    if (w.d_counts[2] != 0u) return; // (as k_weld_number)
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t a = 0u, b = 0u, c = 0u;
    if (t < numTriangles) {
        a = (uint32_t)w.d_slotWinner[w.d_vertexSlot[3u * t]];
        b = (uint32_t)w.d_slotWinner[w.d_vertexSlot[3u * t + 1u]];
        c = (uint32_t)w.d_slotWinner[w.d_vertexSlot[3u * t + 2u]];
    }
    const bool keep = t < numTriangles && a != b && b != c && a != c;
    const uint32_t at = wave_append(keep, &w.d_counts[1]);
    if (!keep) return;
    w.d_faces[3u * at] = a; w.d_faces[3u * at + 1u] = b; w.d_faces[3u * at + 2u] = c;
}

// the smallest power of two >= 6 n (twice the 3 n keys n triangles can have), 64 slots at least
uint32_t defaultSlotsLog2(uint32_t n)
{
    uint32_t l = 6;
    while (l < 63 && (1ull << l) < 6ull * n) l++;
    return l;
}

} // namespace

extern "C" {

int vh_mesh_weld_key(const int32_t cell[3], uint32_t edge, uint32_t snap, uint64_t* key)
{
    if (!cell || !key) return VH_ERR_BAD_ARGUMENT;
    uint32_t rank = 0;
    return vh_mesh_key(cell[0], cell[1], cell[2], edge, snap, key, &rank) ? VH_OK : VH_ERR_BAD_ARGUMENT;
}

int vh_mesh_weld_default_slots_log2(uint32_t numTriangles, uint32_t* slotsLog2)
{
    if (!slotsLog2) return VH_ERR_BAD_ARGUMENT;
    *slotsLog2 = defaultSlotsLog2(numTriangles);
    return VH_OK;
}

int vh_mesh_weld_data_alloc(VhMeshWeldData* data, uint32_t maxTriangles, uint32_t slotsLog2)
{
    if (!data || maxTriangles > 0x55555555u / 2u) return VH_ERR_BAD_ARGUMENT; // 3 n vertex indices and 6 n slots in 32 bits
    if (slotsLog2 == 0) slotsLog2 = defaultSlotsLog2(maxTriangles);
    if (slotsLog2 > 31) return VH_ERR_BAD_ARGUMENT;
    std::memset(data, 0, sizeof(*data));
    const size_t numSlots = (size_t)1 << slotsLog2, nv = 3 * (size_t)(maxTriangles ? maxTriangles : 1);
    const int r = [&]() -> int {
        VH_HIP(hipMalloc((void**)&data->d_slotKeys, sizeof(uint64_t) * numSlots));
        VH_HIP(hipMalloc((void**)&data->d_slotWinner, sizeof(uint64_t) * numSlots));
        VH_HIP(hipMalloc((void**)&data->d_vertexSlot, sizeof(uint32_t) * nv));
        VH_HIP(hipMalloc((void**)&data->d_counts, sizeof(uint32_t) * 4));
        VH_HIP(hipMalloc((void**)&data->d_vertices, sizeof(VhVertex) * nv));
        VH_HIP(hipMalloc((void**)&data->d_keys, sizeof(uint64_t) * nv));
        VH_HIP(hipMalloc((void**)&data->d_faces, sizeof(uint32_t) * nv));
        VH_HIP(hipMemset(data->d_counts, 0, sizeof(uint32_t) * 4));
        return VH_OK;
    }();
    if (r != VH_OK) {
        vh_mesh_weld_data_free(data);
        return r;
    }
    data->m_maxTriangles = maxTriangles;
    data->m_slotsLog2 = slotsLog2;
    return VH_OK;
}

void vh_mesh_weld_data_free(VhMeshWeldData* data)
{
    if (!data) return;
    if (data->d_slotKeys) (void)hipFree(data->d_slotKeys);
    if (data->d_slotWinner) (void)hipFree(data->d_slotWinner);
    if (data->d_vertexSlot) (void)hipFree(data->d_vertexSlot);
    if (data->d_counts) (void)hipFree(data->d_counts);
    if (data->d_vertices) (void)hipFree(data->d_vertices);
    if (data->d_keys) (void)hipFree(data->d_keys);
    if (data->d_faces) (void)hipFree(data->d_faces);
    std::memset(data, 0, sizeof(*data));
}

int vh_mesh_weld(const VhTriangle* d_triangles, const VhTriangleSource* d_sources, uint32_t numTriangles, const VhMeshWeldData* data,
                 uint32_t slotsLog2, vhStream_t stream)
{
    if (!data || !data->d_slotKeys || !data->d_counts) return VH_ERR_BAD_ARGUMENT;
    if (numTriangles > data->m_maxTriangles || (numTriangles != 0 && (!d_triangles || !d_sources))) return VH_ERR_BAD_ARGUMENT;
    if (slotsLog2 == 0) slotsLog2 = defaultSlotsLog2(numTriangles);
    if (slotsLog2 > data->m_slotsLog2) return VH_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    VH_HIP(hipMemsetAsync(data->d_counts, 0, sizeof(uint32_t) * 4, s));
    if (numTriangles == 0) return VH_OK; // an empty mesh, and no launch with an empty grid
    const size_t numSlots = (size_t)1 << slotsLog2;
    VH_HIP(hipMemsetAsync(data->d_slotKeys, 0xff, sizeof(uint64_t) * numSlots, s));
    VH_HIP(hipMemsetAsync(data->d_slotWinner, 0xff, sizeof(uint64_t) * numSlots, s));
    VH_LAUNCH_TIMED(k_weld_insert, cdiv(3ull * numTriangles, 256), 256, s, d_sources, 3u * numTriangles, *data, slotsLog2);
    VH_TRY(vh_last_launch_error());
    VH_LAUNCH_TIMED(k_weld_number, cdiv(numSlots, 256 * kNumberPerLane), 256, s, d_triangles, *data, slotsLog2);
    VH_TRY(vh_last_launch_error());
    VH_LAUNCH_TIMED(k_weld_faces, cdiv(numTriangles, 256), 256, s, numTriangles, *data);
    return vh_last_launch_error();
}

int vh_mesh_weld_get_counts(const VhMeshWeldData* data, uint32_t out[3], vhStream_t stream)
{
    if (!data || !data->d_counts || !out) return VH_ERR_BAD_ARGUMENT;
    VH_HIP(hipMemcpyAsync(out, data->d_counts, sizeof(uint32_t) * 3, hipMemcpyDeviceToHost, (hipStream_t)stream));
    VH_HIP(hipStreamSynchronize((hipStream_t)stream));
    if (out[2] & VH_WELD_KEY_RANGE) return VH_ERR_BAD_ARGUMENT;
    if (out[2] & VH_WELD_TABLE_FULL) return VH_ERR_STAGING_OVERFLOW;
    return VH_OK;
}

int vh_mesh_weld_download(const VhMeshWeldData* data, VhVertex* vertices, uint64_t* keys, uint32_t* faces, uint32_t numVertices,
                          uint32_t numFaces, vhStream_t stream)
{
    if (!data || !data->d_vertices) return VH_ERR_BAD_ARGUMENT;
    if (numVertices > 3ull * data->m_maxTriangles || numFaces > data->m_maxTriangles) return VH_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    if (vertices && numVertices) VH_HIP(hipMemcpyAsync(vertices, data->d_vertices, sizeof(VhVertex) * (size_t)numVertices, hipMemcpyDeviceToHost, s));
    if (keys && numVertices) VH_HIP(hipMemcpyAsync(keys, data->d_keys, sizeof(uint64_t) * (size_t)numVertices, hipMemcpyDeviceToHost, s));
    if (faces && numFaces) VH_HIP(hipMemcpyAsync(faces, data->d_faces, sizeof(uint32_t) * 3 * (size_t)numFaces, hipMemcpyDeviceToHost, s));
    VH_HIP(hipStreamSynchronize(s));
    return VH_OK;
}

} // extern "C"
