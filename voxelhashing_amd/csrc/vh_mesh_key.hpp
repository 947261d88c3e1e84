// vh_mesh_key.hpp -- the key under which the indexed extraction welds marching-cubes vertices (DESIGN.md section 4,
// "Indexed mesh").  Written once for the device (vh_mesh.hip) and the host (vh_mesh_weld_key).
//
// A cell at voxel coordinates `cell` has its corner (bx, by, bz) on the lattice point L = cell + (bx, by, bz), which
// sits at (L - 1/2) * voxelSize.  An interpolated vertex lies on a lattice edge and is named by the edge's lower end
// and its axis; a snapped vertex (vertexInterp returned one of the end points) is named by that lattice point.
//   bits  0-19  L.x + 2^19      bits 40-59  L.z + 2^19
//   bits 20-39  L.y + 2^19      bits 60-61  code: the edge's axis 0/1/2, or 3 for a lattice point
// Bits 62-63 are 0, so the all-ones word is no key: it marks an empty slot of the weld table.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define VH_KEY_FN __host__ __device__ inline
#else
#define VH_KEY_FN inline
#endif

constexpr uint64_t kMeshKeyEmpty = ~0ull;
constexpr int32_t kMeshKeyBias = 1 << 19;

// the 12 edges in the reference's vertlist order (DSC/MarchingCubesSDFUtil.h:217-228): corner bits x | y << 1 | z << 2
// of the first (p1) and second (p2) argument of vertexInterp, three bits per edge
constexpr uint64_t kMeshEdgeP1 = (2ull << 0) | (3ull << 3) | (1ull << 6) | (0ull << 9) | (6ull << 12) | (7ull << 15) | (5ull << 18) | (4ull << 21) | (2ull << 24) | (3ull << 27) | (1ull << 30) | (0ull << 33);
constexpr uint64_t kMeshEdgeP2 = (3ull << 0) | (1ull << 3) | (0ull << 6) | (2ull << 9) | (7ull << 12) | (5ull << 15) | (4ull << 18) | (6ull << 21) | (6ull << 24) | (7ull << 27) | (5ull << 30) | (4ull << 33);

// -> false when edge > 11, snap > 2 or a component of L is outside [-2^19, 2^19).  rank orders the cells that can hold
// the same key: the smaller rank belongs to the cell whose (z, y, x) voxel coordinates are lexicographically smaller.
VH_KEY_FN bool vh_mesh_key(int32_t cx, int32_t cy, int32_t cz, uint32_t edge, uint32_t snap, uint64_t* key, uint32_t* rank)
{
    if (edge > 11u || snap > 2u) return false;
    const uint32_t a = (uint32_t)(kMeshEdgeP1 >> (3u * edge)) & 7u, b = (uint32_t)(kMeshEdgeP2 >> (3u * edge)) & 7u;
    // the lower end of the edge is the corner without the axis bit; the axis bit is the one the end points differ in
    const uint32_t corner = snap == 0u ? (a & b) : (snap == 1u ? a : b);
    const uint32_t code = snap == 0u ? ((a ^ b) >> 1) : 3u; // 1, 2, 4 -> 0, 1, 2
    const int64_t lx = (int64_t)cx + (corner & 1u), ly = (int64_t)cy + ((corner >> 1) & 1u), lz = (int64_t)cz + ((corner >> 2) & 1u);
    if (lx < -kMeshKeyBias || lx >= kMeshKeyBias || ly < -kMeshKeyBias || ly >= kMeshKeyBias || lz < -kMeshKeyBias || lz >= kMeshKeyBias) return false;
    *key = (uint64_t)(lx + kMeshKeyBias) | ((uint64_t)(ly + kMeshKeyBias) << 20) | ((uint64_t)(lz + kMeshKeyBias) << 40) | ((uint64_t)code << 60);
    // cell = L - corner bits: among the sharers of a key the largest corner (z the most significant bit) is the
    // lexicographically smallest cell
    *rank = 7u - corner;
    return true;
}

// The key of a cell in the table of the accumulating weld (vh_mesh_weld_accum_*), which remembers the cells it has
// taken beside the vertex keys: the cell's voxel coordinates packed as a vertex key's lattice point, and bit 62 set,
// which no vertex key has.  Bit 63 stays 0, so the all-ones word is still no key.
constexpr uint64_t kMeshKeyCell = 1ull << 62;
// -> false when a coordinate is outside [-2^19, 2^19)
VH_KEY_FN bool vh_mesh_cell_key(int32_t cx, int32_t cy, int32_t cz, uint64_t* key)
{
    if (cx < -kMeshKeyBias || cx >= kMeshKeyBias || cy < -kMeshKeyBias || cy >= kMeshKeyBias || cz < -kMeshKeyBias || cz >= kMeshKeyBias) return false;
    *key = (uint64_t)(cx + kMeshKeyBias) | ((uint64_t)(cy + kMeshKeyBias) << 20) | ((uint64_t)(cz + kMeshKeyBias) << 40) | kMeshKeyCell;
    return true;
}

// The key of the cluster a vertex key falls into when the lattice is cut into cubes of m points a side (the vertex
// clustering of vh_mesh_cluster; DESIGN.md section 4, "Mesh clustering"): the key's lattice point L, whatever its code,
// gives k = floor(L / m) per component -- floor, not truncation: L = -1, m = 2 is k = -1 -- packed as a lattice point
// with code 3.  |k| <= |L|, so k is in range whenever L was.
// -> false when m is 0 or bit 62 or 63 of the key is set (a cell key, the empty word: no vertex key)
VH_KEY_FN bool vh_mesh_cluster_key_of(uint64_t vertexKey, uint32_t m, uint64_t* key)
{
    if (m == 0u || (vertexKey >> 62) != 0ull) return false;
    uint64_t out = 3ull << 60;
    for (uint32_t axis = 0; axis < 3u; axis++) {
        const int32_t l = (int32_t)((vertexKey >> (20u * axis)) & 0xfffffull) - kMeshKeyBias, d = (int32_t)m;
        const int32_t k = l >= 0 ? l / d : -((-l + d - 1) / d);
        out |= (uint64_t)(k + kMeshKeyBias) << (20u * axis);
    }
    *key = out;
    return true;
}
