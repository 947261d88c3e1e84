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

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

#include "vh_device.hpp"
#include "vh_host_util.hpp"
#include "vh_mesh_key.hpp"
#include "vh_mesh_table.hpp"
#include "vh_mesh_finish.hpp"

using namespace vhd;

namespace {

// One lane per soup vertex i = 3 * triangle + corner: claim the slot of its key, bid for the slot's vertex with
// rank << 32 | i (the smallest wins), remember the slot.
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
    const uint32_t found = weld_find_or_claim(reinterpret_cast<unsigned long long*>(w.d_slotKeys), key, slotsLog2);
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

// ---------------------------------------------------------------------------------------------------------------------
// The accumulating weld (vh_mesh_weld_accum_*; DESIGN.md section 4, "Indexed mesh over several extractions"): one table
// lives through several appends.  A slot is a key (a vertex key, or a cell key: bit 62), a value (the vertex's index,
// or the ordinal of the append that owns the cell; all ones = none yet) and a bid word.  A bid is
//   (VH_WELD_ACCUM_MAX_APPENDS - ordinal) << 35 | rank << 32 | soup vertex
// so that atomicMin keeps the smallest (rank, soup vertex) of the LATEST append that bid: what earlier appends left in
// the word never wins, and nothing has to be cleared between appends.  Three launches per append: insert (one lane
// per triangle), settle (one lane per soup vertex), faces (one lane per triangle).

struct WeldAccumView {
    uint64_t* slotKeys;    // numSlots; all ones = empty
    uint64_t* slotBids;    // numSlots
    uint32_t* slotVals;    // numSlots
    uint32_t* counts;      // VH_WELD_ACCUM_* (the rehash count is the host's)
    uint32_t* vertexSlot;  // 3 n of this append: the slot of each soup vertex
    VhVertex* vertices;    // one per welded vertex
    uint64_t* keys;
    uint8_t* ranks;        // the rank of the soup vertex whose bits the welded vertex has
    uint32_t* faces;
    uint32_t slotsLog2;
};

constexpr uint32_t kNoValue = 0xffffffffu;
constexpr uint32_t kDroppedSlot = 0xfffffffeu; // in vertexSlot: the triangle's cell belongs to an earlier append

// One lane per triangle.  Claims the cell for this append (a cell an earlier append owns drops the triangle here,
// before any of its keys is looked at), then for each of the three vertices the slot of its key, and bids for it.
__global__ __launch_bounds__(256) void k_weld_accum_insert(const VhTriangleSource* sources, uint32_t numTriangles, WeldAccumView w, uint32_t ordinal)
{
    if (__builtin_amdgcn_readfirstlane((int)w.counts[VH_WELD_ACCUM_STATUS]) != 0) return; // an earlier append failed (wave-uniform)
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = t < numTriangles;
    unsigned long long* slotKeys = reinterpret_cast<unsigned long long*>(w.slotKeys);
    uint64_t key[3] = { 0ull, 0ull, 0ull }, cellKey = 0ull;
    uint32_t rank[3] = { 0u, 0u, 0u }, status = 0u;
    if (valid) {
        const VhTriangleSource src = sources[t];
        bool ok = vh_mesh_cell_key(src.cell[0], src.cell[1], src.cell[2], &cellKey);
#pragma unroll
        for (uint32_t k = 0; k < 3u; k++) {
            const uint32_t code = (src.edges >> (8u * k)) & 0xffu;
            ok = ok && (code >> 6) == 0u && vh_mesh_key(src.cell[0], src.cell[1], src.cell[2], code & 0xfu, (code >> 4) & 3u, &key[k], &rank[k]);
        }
        if (!ok) status = VH_WELD_KEY_RANGE;
    }
    bool kept = false, first = false;
    uint32_t slots[3] = { kNoSlot, kNoSlot, kNoSlot };
    if (valid && status == 0u) {
        const uint32_t cellSlot = weld_find_or_claim(slotKeys, cellKey, w.slotsLog2);
        if (cellSlot == kNoSlot) status = VH_WELD_TABLE_FULL;
        else {
            const uint32_t owner = atomicCAS(&w.slotVals[cellSlot], kNoValue, ordinal);
            first = owner == kNoValue;
            kept = first || owner == ordinal;
        }
    }
    if (kept) {
        const uint64_t high = (uint64_t)(VH_WELD_ACCUM_MAX_APPENDS - ordinal) << 35;
#pragma unroll 1
        for (uint32_t k = 0; k < 3u; k++) {
            const uint32_t slot = weld_find_or_claim(slotKeys, key[k], w.slotsLog2);
            if (slot == kNoSlot) { status = VH_WELD_TABLE_FULL; break; }
            atomicMin(reinterpret_cast<unsigned long long*>(&w.slotBids[slot]), (unsigned long long)(high | ((uint64_t)rank[k] << 32) | (3u * t + k)));
            slots[k] = slot;
        }
    }
    if (status != 0u) atomicOr(&w.counts[VH_WELD_ACCUM_STATUS], status);
    if (valid) {
        const bool dropped = status == 0u && !kept;
#pragma unroll
        for (uint32_t k = 0; k < 3u; k++) w.vertexSlot[3u * t + k] = dropped ? kDroppedSlot : slots[k];
    }
    wave_count(first, &w.counts[VH_WELD_ACCUM_CELLS]);
}

// One lane per soup vertex; only the lane whose bid stands in its slot acts.  A key without a vertex gets the next
// index (one atomic per wave) and this soup vertex's bits; a key that has one keeps its index, and takes these bits
// only if their rank is strictly smaller than the rank of the bits it has.  One lane per key acts and the appends
// follow each other on the stream: nothing races.
__global__ __launch_bounds__(256) void k_weld_accum_settle(const VhTriangle* triangles, uint32_t numVertices, WeldAccumView w, uint32_t ordinal)
{
    if (w.counts[VH_WELD_ACCUM_STATUS] != 0u) return; // written by the launch before this one: uniform
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t slot = i < numVertices ? w.vertexSlot[i] : kNoSlot;
    bool mine = false;
    uint32_t rank = 0u, index = kNoValue;
    if (slot < kDroppedSlot) {
        const uint64_t bid = w.slotBids[slot];
        mine = (uint32_t)bid == i && (uint32_t)(bid >> 35) == VH_WELD_ACCUM_MAX_APPENDS - ordinal;
        rank = (uint32_t)(bid >> 32) & 7u;
        if (mine) index = w.slotVals[slot];
    }
    const bool fresh = mine && index == kNoValue;
    const uint32_t at = wave_append(fresh, &w.counts[VH_WELD_ACCUM_VERTICES]);
    if (!mine) return;
    if (fresh) {
        index = at;
        w.slotVals[slot] = index;
        w.keys[index] = w.slotKeys[slot];
    } else if (rank >= (uint32_t)w.ranks[index]) return;
    w.vertices[index] = reinterpret_cast<const VhVertex*>(triangles)[i];
    w.ranks[index] = (uint8_t)rank;
}

// One lane per triangle: a dropped one is counted; the others look their three indices up and, unless two are the same,
// go to the end of the one face list (one atomic per wave), winding kept.
__global__ __launch_bounds__(256) void k_weld_accum_faces(uint32_t numTriangles, WeldAccumView w)
{
    if (w.counts[VH_WELD_ACCUM_STATUS] != 0u) return; // (as k_weld_accum_settle)
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t a = 0u, b = 0u, c = 0u;
    bool dropped = false;
    if (t < numTriangles) {
        const uint32_t s0 = w.vertexSlot[3u * t], s1 = w.vertexSlot[3u * t + 1u], s2 = w.vertexSlot[3u * t + 2u];
        dropped = s0 == kDroppedSlot;
        if (!dropped) { a = w.slotVals[s0]; b = w.slotVals[s1]; c = w.slotVals[s2]; }
    }
    wave_count(dropped, &w.counts[VH_WELD_ACCUM_DROPPED]);
    const bool keep = t < numTriangles && !dropped && a != b && b != c && a != c;
    const uint32_t at = wave_append(keep, &w.counts[VH_WELD_ACCUM_FACES]);
    if (!keep) return;
    w.faces[3u * at] = a; w.faces[3u * at + 1u] = b; w.faces[3u * at + 2u] = c;
}

// One lane per slot of the old table: its key into the new, larger one (the keys are distinct, so the first empty slot
// of the probe is the key's), its value with it.  Bids are not carried: the next append's are smaller than any.
__global__ __launch_bounds__(256) void k_weld_rehash(const uint64_t* oldKeys, const uint32_t* oldVals, uint32_t oldSlotsLog2, WeldAccumView w)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= (1u << oldSlotsLog2)) return;
    const uint64_t key = oldKeys[s];
    if (key == kMeshKeyEmpty) return;
    const uint32_t slot = weld_find_or_claim(reinterpret_cast<unsigned long long*>(w.slotKeys), key, w.slotsLog2);
    if (slot == kNoSlot) atomicOr(&w.counts[VH_WELD_ACCUM_STATUS], VH_WELD_TABLE_FULL); // (a larger table always has room)
    else w.slotVals[slot] = oldVals[s];
}

// ---------------------------------------------------------------------------------------------------------------------
// Vertex normals of a welded mesh (vh_mesh_vertex_normals; DESIGN.md section 4, "Vertex normals"): area-weighted face
// normals summed per vertex in 64-bit fixed point, so that the sums do not depend on the order the atomics ran in.
// Two launches: faces (one lane per face), finish (one lane per vertex).

// One lane per face.  An index >= numVertices is reported before anything is read through it; a face with a repeated
// index adds nothing.  The triple is rotated, winding kept, so that the vertex with the smallest key comes first: face
// order and vertex numbers come from atomics, keys do not.  Then float32, one rounding per operation (the build has
// -ffp-contract=off): a = p1 - p0, b = p2 - p0, c = a x b, s = c * scale (a power of two), q = rint(s) added to the
// three accumulators of each of the three vertices -- nine atomics whose results nobody reads.  A component of s that is
// not finite or above 2^40 reports the face instead.  The lanes' reports go into the status word with one atomic per wave.
__global__ __launch_bounds__(256) void k_mesh_normals_faces(const VhVertex* vertices, const uint64_t* keys, const uint32_t* faces, uint32_t numVertices,
                                                            uint32_t numFaces, float scale, unsigned long long* acc, uint32_t* statusWord)
{
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t status = 0u;
    if (f < numFaces) {
        uint32_t i0 = faces[3u * f], i1 = faces[3u * f + 1u], i2 = faces[3u * f + 2u];
        if (i0 >= numVertices || i1 >= numVertices || i2 >= numVertices) status = VH_NORMALS_BAD_INDEX;
        else if (i0 != i1 && i1 != i2 && i0 != i2) {
            const uint64_t k0 = keys[i0], k1 = keys[i1], k2 = keys[i2];
            if (k1 < k0 && k1 <= k2) { const uint32_t t = i0; i0 = i1; i1 = i2; i2 = t; }
            else if (k2 < k0 && k2 < k1) { const uint32_t t = i0; i0 = i2; i2 = i1; i1 = t; }
            const VhVertex v0 = vertices[i0], v1 = vertices[i1], v2 = vertices[i2];
            const float ax = v1.p[0] - v0.p[0], ay = v1.p[1] - v0.p[1], az = v1.p[2] - v0.p[2];
            const float bx = v2.p[0] - v0.p[0], by = v2.p[1] - v0.p[1], bz = v2.p[2] - v0.p[2];
            const float sx = (ay * bz - az * by) * scale, sy = (az * bx - ax * bz) * scale, sz = (ax * by - ay * bx) * scale;
            const float limit = 1099511627776.0f; // 2^40
            if (!(fabsf(sx) <= limit && fabsf(sy) <= limit && fabsf(sz) <= limit)) status = VH_NORMALS_RANGE; // (NaN fails every comparison)
            else {
                const unsigned long long qx = (unsigned long long)(long long)rintf(sx), qy = (unsigned long long)(long long)rintf(sy),
                                         qz = (unsigned long long)(long long)rintf(sz);
                atomicAdd(&acc[3ull * i0], qx); atomicAdd(&acc[3ull * i0 + 1ull], qy); atomicAdd(&acc[3ull * i0 + 2ull], qz);
                atomicAdd(&acc[3ull * i1], qx); atomicAdd(&acc[3ull * i1 + 1ull], qy); atomicAdd(&acc[3ull * i1 + 2ull], qz);
                atomicAdd(&acc[3ull * i2], qx); atomicAdd(&acc[3ull * i2 + 1ull], qy); atomicAdd(&acc[3ull * i2 + 2ull], qz);
            }
        }
    }
    const uint64_t range = __ballot((status & VH_NORMALS_RANGE) != 0u), bad = __ballot((status & VH_NORMALS_BAD_INDEX) != 0u);
    if ((range | bad) == 0ull) return;
    if ((int)lane_id() == __ffsll((unsigned long long)(range | bad)) - 1)
        atomicOr(statusWord, (range != 0ull ? VH_NORMALS_RANGE : 0u) | (bad != 0ull ? VH_NORMALS_BAD_INDEX : 0u));
}

// One lane per vertex: the three sums as doubles, normalised with correctly rounded double arithmetic and rounded to
// float once.  A zero sum (no face, collapsed faces only, contributions that cancel) gives (0, 0, 0), and so does every
// vertex once the face pass, which ran before this launch on the stream, has left a status.
__global__ __launch_bounds__(256) void k_mesh_normals_finish(const unsigned long long* acc, uint32_t numVertices, const uint32_t* statusWord, float* normals)
{
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= numVertices) return;
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    if (*statusWord == 0u) { // uniform
        const double dx = (double)(long long)acc[3ull * v], dy = (double)(long long)acc[3ull * v + 1ull], dz = (double)(long long)acc[3ull * v + 2ull];
        const double l2 = (dx * dx + dy * dy) + dz * dz;
        if (l2 != 0.0) {
            const double l = __dsqrt_rn(l2);
            nx = (float)__ddiv_rn(dx, l); ny = (float)__ddiv_rn(dy, l); nz = (float)__ddiv_rn(dz, l);
        }
    }
    normals[3ull * v] = nx; normals[3ull * v + 1ull] = ny; normals[3ull * v + 2ull] = nz;
}

// ---------------------------------------------------------------------------------------------------------------------
// Connected components of a welded mesh (vh_mesh_components, vh_mesh_components_filter; DESIGN.md section 4, "Mesh
// components").  Vertices are ordered by (key, index); a component is named by its first vertex.  Labelling is a
// lock-free union-find: init, hook (one lane per face), flatten (one lane per vertex), count (one lane per face).  The
// filter then keeps the components of at least minFaces faces, or the largest one alone, and compacts vertices and
// faces into buffers of its own.
//
// parent[v] is v, or a vertex before v in the order: it leaves v once, by the one compare-and-swap that succeeds on
// it, and is afterwards only ever replaced by a proper ancestor.  So the parents never form a cycle, every chain ends
// in the first vertex of what has been joined, and once an ancestor is always an ancestor.  A load of parent[] inside
// the hook launch may be stale (the L2s of the XCDs are not coherent): a stale "I am a root" only makes the
// compare-and-swap fail, which returns the real parent, and a stale parent is still an ancestor.  Nothing but the
// results of the compare-and-swaps is relied on.

VHD uint32_t comp_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
VHD void comp_store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Moves c up to a vertex whose parent reads as itself, halving the path behind it: the grandparent that replaces a
// parent is a proper ancestor, and the word it goes into has left its own vertex for good, so no compare-and-swap can
// succeed on it any more.  false when the steps ran out.
VHD bool comp_walk(uint32_t* parent, uint32_t& c, uint32_t& steps, uint32_t limit)
{
#pragma unroll 1
    for (; steps < limit; steps++) {
        const uint32_t p = comp_load(&parent[c]);
        if (p == c) return true;
        const uint32_t g = comp_load(&parent[p]);
        if (g != p) comp_store(&parent[c], g);
        c = g;
    }
    return false;
}

// Joins the components of a and b: both cursors to what reads as a root, the later of the two under the earlier.  A
// compare-and-swap that fails returns y's real parent, and the walk goes on from there.  Every step and every failure
// moves one of the two cursors to a vertex strictly before it, so 2 V steps are never reached; false if they are.
// a comes back as the vertex the two ended under: a member of the joined component near its root, from which the
// face's next union starts instead of walking up again.
VHD bool comp_union(uint32_t* parent, const uint64_t* keys, uint32_t& a, uint32_t b, uint32_t limit)
{
    uint32_t x = a, y = b, steps = 0u;
#pragma unroll 1
    for (; steps < limit; steps++) {
        if (!comp_walk(parent, x, steps, limit) || !comp_walk(parent, y, steps, limit)) return false;
        a = x;
        if (x == y) return true;
        const uint64_t kx = keys[x], ky = keys[y];
        if (ky < kx || (ky == kx && y < x)) { const uint32_t t = x; x = y; y = t; }
        a = x;
        const uint32_t old = atomicCAS(&parent[y], y, x);
        if (old == y) return true;
        y = old;
    }
    return false;
}

// the lanes' status bits into the word: one atomic per wave that has any.  Every lane of the wave calls it.
VHD void wave_status(uint32_t status, uint32_t* statusWord)
{
    const uint64_t any = __ballot(status != 0u);
    if (any == 0ull) return;
    uint32_t bits = 0u;
    for (uint32_t b = 1u; b <= 2u; b <<= 1) bits |= __ballot((status & b) != 0u) != 0ull ? b : 0u;
    if ((int)lane_id() == __ffsll((unsigned long long)any) - 1) atomicOr(statusWord, bits);
}

__global__ __launch_bounds__(256) void k_components_init(uint32_t numVertices, uint32_t* parent)
{
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < numVertices) parent[v] = v;
}

// One lane per face: an index >= numVertices is reported before anything is read through it, and the face joins nothing;
// the others join (i0, i1) and then (where that ended, i2).
__global__ __launch_bounds__(256) void k_components_hook(const uint64_t* keys, const uint32_t* faces, uint32_t numVertices, uint32_t numFaces,
                                                         uint32_t* parent, uint32_t* statusWord)
{
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t status = 0u;
    if (f < numFaces) {
        const uint32_t i0 = faces[3u * f], i1 = faces[3u * f + 1u], i2 = faces[3u * f + 2u];
        if (i0 >= numVertices || i1 >= numVertices || i2 >= numVertices) status = VH_COMPONENTS_BAD_INDEX;
        else {
            const uint32_t limit = 2u * numVertices + 4u; // (numVertices <= 2^31 - 16: the launcher)
            uint32_t at = i0;
            if (!comp_union(parent, keys, at, i1, limit) || !comp_union(parent, keys, at, i2, limit)) status = VH_COMPONENTS_STEPS;
        }
    }
    wave_status(status, statusWord);
}

// One lane per vertex, in a launch of its own, so that what it reads is what the hook launch left: the end of v's chain
// over parent[v].  Lanes that pass through v meanwhile read its old parent or its root; both lead to the root.
__global__ __launch_bounds__(256) void k_components_flatten(uint32_t numVertices, uint32_t* parent, uint32_t* statusWord)
{
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t status = 0u;
    if (v < numVertices) {
        uint32_t c = v, p = comp_load(&parent[v]), steps = 0u;
#pragma unroll 1
        for (; p != c && steps < numVertices; steps++) { c = p; p = comp_load(&parent[c]); }
        if (p != c) status = VH_COMPONENTS_STEPS;
        else if (c != v) comp_store(&parent[v], c);
    }
    wave_status(status, statusWord);
}

// One lane per face: an in-range face counts for the root of its first index; the lanes of a wave that agree on the
// root share one atomic.
__global__ __launch_bounds__(256) void k_components_count(const uint32_t* faces, uint32_t numVertices, uint32_t numFaces, const uint32_t* root,
                                                          uint32_t* faceCount)
{
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    bool pending = false;
    uint32_t r = 0u;
    if (f < numFaces) {
        const uint32_t i0 = faces[3u * f], i1 = faces[3u * f + 1u], i2 = faces[3u * f + 2u];
        pending = i0 < numVertices && i1 < numVertices && i2 < numVertices;
        if (pending) r = root[i0];
    }
#pragma unroll 1
    for (int round = 0; round < kWave; round++) { // a round retires the leader's root: at most one per lane
        const uint64_t m = __ballot(pending);
        if (m == 0ull) break;
        const int leader = __ffsll((unsigned long long)m) - 1;
        const uint32_t lr = (uint32_t)__builtin_amdgcn_readlane((int)r, leader);
        const uint64_t same = __ballot(pending && r == lr);
        if ((int)lane_id() == leader) atomicAdd(&faceCount[lr], (uint32_t)__popcll(same));
        if (r == lr) pending = false;
    }
}

// One lane per vertex: the components with a face, the vertices without one, the largest face count (one atomic per
// wave each).  Nothing is counted once the labelling has left a status.
__global__ __launch_bounds__(256) void k_components_stats(uint32_t numVertices, const uint32_t* root, const uint32_t* faceCount, const uint32_t* statusWord,
                                                          uint32_t* counts)
{
    if (*statusWord != 0u) return; // written by a launch before this one: uniform
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    const bool isRoot = v < numVertices && root[v] == v;
    const uint32_t n = isRoot ? faceCount[v] : 0u;
    wave_count(isRoot && n != 0u, &counts[VH_COMPONENTS_WITH_FACES]);
    wave_count(isRoot && n == 0u, &counts[VH_COMPONENTS_FACELESS]);
    uint32_t most = n;
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) most = max(most, (uint32_t)__shfl_xor((int)most, off));
    if (most != 0u && lane_id() == 0u) atomicMax(&counts[VH_COMPONENTS_LARGEST_FACES], most);
}

// The largest component among equals: the root first in the order.  Two launches of one lane per vertex: the smallest
// key among the roots that reach the largest count into best[0], then the smallest index among those with that key
// into best[1] (welded keys are distinct; the index settles hand-made input).
__global__ __launch_bounds__(256) void k_components_pick(uint32_t numVertices, const uint64_t* keys, const uint32_t* root, const uint32_t* faceCount,
                                                         const uint32_t* statusWord, const uint32_t* counts, unsigned long long* best, uint32_t byIndex)
{
    if (*statusWord != 0u) return; // (as k_components_stats)
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t most = counts[VH_COMPONENTS_LARGEST_FACES];
    bool mine = most != 0u && v < numVertices && root[v] == v && faceCount[v] == most;
    if (byIndex != 0u) mine = mine && keys[v] == best[0];
    unsigned long long bid = !mine ? ~0ull : byIndex != 0u ? (unsigned long long)v : (unsigned long long)keys[v];
    if (__ballot(mine) == 0ull) return; // wave-uniform
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const unsigned long long other = (unsigned long long)__shfl_xor((long long)bid, off);
        bid = other < bid ? other : bid;
    }
    if (lane_id() == 0u) atomicMin(&best[byIndex], bid);
}

struct ComponentFilterView {
    const VhVertex* vertices;
    const uint64_t* keys;
    const float* normals;      // 3 per vertex, or null
    const uint32_t* faces;
    const uint32_t* root;
    const uint32_t* faceCount;
    const uint32_t* statusWord;
    const unsigned long long* best;
    uint32_t* counts;
    uint32_t* newIndex;        // one per vertex: its index in the output, or all ones
    VhVertex* outVertices;
    uint64_t* outKeys;
    float* outNormals;
    uint32_t* outFaces;
    uint32_t numVertices, numFaces, minFaces, largestOnly;
};

// One lane per vertex: kept when its component has minFaces faces and, with largestOnly, is the one picked.  The kept
// ones get their new indices by a wave scan and one atomic per wave, and go into the output with key and normal.
__global__ __launch_bounds__(256) void k_components_compact_vertices(ComponentFilterView c)
{
    if (*c.statusWord != 0u) return; // (as k_components_stats)
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    bool keep = false, keptRoot = false;
    if (v < c.numVertices) {
        const uint32_t r = c.root[v], n = c.faceCount[r];
        keep = n >= c.minFaces && (c.largestOnly == 0u || (unsigned long long)r == c.best[1]);
        keptRoot = keep && r == v && n != 0u;
    }
    const uint32_t at = wave_append(keep, &c.counts[VH_COMPONENTS_KEPT_VERTICES]);
    wave_count(keptRoot, &c.counts[VH_COMPONENTS_KEPT]);
    if (v >= c.numVertices) return;
    c.newIndex[v] = keep ? at : kNoValue;
    if (!keep) return;
    c.outVertices[at] = c.vertices[v];
    c.outKeys[at] = c.keys[v];
    if (c.normals) { c.outNormals[3ull * at] = c.normals[3ull * v]; c.outNormals[3ull * at + 1ull] = c.normals[3ull * v + 1ull]; c.outNormals[3ull * at + 2ull] = c.normals[3ull * v + 2ull]; }
}

// One lane per face: kept with its first vertex (all three are of one component), renumbered, winding and rotation left alone.
__global__ __launch_bounds__(256) void k_components_compact_faces(ComponentFilterView c)
{
    if (*c.statusWord != 0u) return; // (as k_components_stats)
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t a = kNoValue, b = kNoValue, d = kNoValue;
    if (f < c.numFaces) {
        const uint32_t i0 = c.faces[3u * f], i1 = c.faces[3u * f + 1u], i2 = c.faces[3u * f + 2u];
        if (i0 < c.numVertices && i1 < c.numVertices && i2 < c.numVertices) { a = c.newIndex[i0]; b = c.newIndex[i1]; d = c.newIndex[i2]; }
    }
    const bool keep = a != kNoValue && b != kNoValue && d != kNoValue;
    const uint32_t at = wave_append(keep, &c.counts[VH_COMPONENTS_KEPT_FACES]);
    if (!keep) return;
    c.outFaces[3u * at] = a; c.outFaces[3u * at + 1u] = b; c.outFaces[3u * at + 2u] = d;
}

// the smallest power of two >= 6 n (twice the 3 n keys n triangles can have), 64 slots at least
uint32_t defaultSlotsLog2(uint32_t n)
{
    uint32_t l = 6;
    while (l < 63 && (1ull << l) < 6ull * n) l++;
    return l;
}

// a weld's status word as the code the get_counts functions return
int weldStatusCode(uint32_t status)
{
    if (status & VH_WELD_KEY_RANGE) return VH_ERR_BAD_ARGUMENT;
    if (status & VH_WELD_TABLE_FULL) return VH_ERR_STAGING_OVERFLOW;
    return VH_OK;
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
    return weldStatusCode(out[2]);
}

int vh_mesh_weld_download(const VhMeshWeldData* data, VhVertex* vertices, uint64_t* keys, uint32_t* faces, uint32_t numVertices,
                          uint32_t numFaces, vhStream_t stream)
{
    if (!data || !data->d_vertices) return VH_ERR_BAD_ARGUMENT;
    if (numVertices > 3ull * data->m_maxTriangles || numFaces > data->m_maxTriangles) return VH_ERR_BAD_ARGUMENT;
    return VhMeshFinish::download(VhMeshView{ data->d_vertices, data->d_keys, data->d_faces, nullptr, numVertices, numFaces }, vertices, keys, nullptr, faces, stream);
}

int vh_mesh_normals_default_scale_log2(float voxelSize, int32_t* scaleLog2)
{
    if (!scaleLog2 || !(voxelSize > 0.0f) || !std::isfinite(voxelSize)) return VH_ERR_BAD_ARGUMENT;
    // ceil(log2(v)) from the exponent: v = m 2^e with m in [1/2, 1), so the ceiling is e unless v is the power of two 2^(e-1)
    int e = 0;
    const double m = std::frexp((double)voxelSize * (double)voxelSize, &e);
    *scaleLog2 = 38 - (m == 0.5 ? e - 1 : e);
    return VH_OK;
}

int vh_mesh_vertex_normals(const VhVertex* d_vertices, const uint64_t* d_keys, const uint32_t* d_faces, uint32_t numVertices, uint32_t numFaces,
                           int32_t scaleLog2, int64_t* d_acc, float* d_normals, uint32_t* d_status, vhStream_t stream)
{
    if (!d_status || scaleLog2 < -100 || scaleLog2 > 100) return VH_ERR_BAD_ARGUMENT;
    if (numVertices != 0 && (!d_vertices || !d_keys || !d_acc || !d_normals)) return VH_ERR_BAD_ARGUMENT;
    if (numFaces != 0 && !d_faces) return VH_ERR_BAD_ARGUMENT;
    if (numFaces > 0x55555555u) return VH_ERR_BAD_ARGUMENT; // 3 numFaces face offsets in 32 bits
    hipStream_t s = (hipStream_t)stream;
    VH_HIP(hipMemsetAsync(d_status, 0, sizeof(uint32_t), s));
    if (numVertices == 0) return VH_OK; // no vertex, no normal; and no launch with an empty grid
    VH_HIP(hipMemsetAsync(d_acc, 0, sizeof(int64_t) * 3 * (size_t)numVertices, s));
    if (numFaces != 0) {
        VH_LAUNCH_TIMED(k_mesh_normals_faces, cdiv(numFaces, 256), 256, s, d_vertices, d_keys, d_faces, numVertices, numFaces, std::ldexp(1.0f, scaleLog2),
                        reinterpret_cast<unsigned long long*>(d_acc), d_status);
        VH_TRY(vh_last_launch_error());
    }
    VH_LAUNCH_TIMED(k_mesh_normals_finish, cdiv(numVertices, 256), 256, s, reinterpret_cast<const unsigned long long*>(d_acc), numVertices, d_status, d_normals);
    return vh_last_launch_error();
}

int vh_mesh_components(const uint64_t* d_keys, const uint32_t* d_faces, uint32_t numVertices, uint32_t numFaces, uint32_t* d_root, uint32_t* d_faceCount,
                       uint32_t* d_status, vhStream_t stream)
{
    if (!d_status) return VH_ERR_BAD_ARGUMENT;
    if (numVertices != 0 && (!d_keys || !d_root || !d_faceCount)) return VH_ERR_BAD_ARGUMENT;
    if (numFaces != 0 && !d_faces) return VH_ERR_BAD_ARGUMENT;
    if (numVertices > 0x7ffffff0u || numFaces > 0x55555555u) return VH_ERR_BAD_ARGUMENT; // 2 V + 4 steps and 3 F face offsets in 32 bits
    hipStream_t s = (hipStream_t)stream;
    VH_HIP(hipMemsetAsync(d_status, 0, sizeof(uint32_t), s));
    if (numVertices == 0) return VH_OK; // nothing to label, and no launch with an empty grid
    VH_HIP(hipMemsetAsync(d_faceCount, 0, sizeof(uint32_t) * (size_t)numVertices, s));
    VH_LAUNCH_TIMED(k_components_init, cdiv(numVertices, 256), 256, s, numVertices, d_root);
    VH_TRY(vh_last_launch_error());
    if (numFaces == 0) return VH_OK; // every vertex is its own root
    VH_LAUNCH_TIMED(k_components_hook, cdiv(numFaces, 256), 256, s, d_keys, d_faces, numVertices, numFaces, d_root, d_status);
    VH_TRY(vh_last_launch_error());
    VH_LAUNCH_TIMED(k_components_flatten, cdiv(numVertices, 256), 256, s, numVertices, d_root, d_status);
    VH_TRY(vh_last_launch_error());
    VH_LAUNCH_TIMED(k_components_count, cdiv(numFaces, 256), 256, s, d_faces, numVertices, numFaces, d_root, d_faceCount);
    return vh_last_launch_error();
}

int vh_mesh_components_filter(const VhVertex* d_vertices, const uint64_t* d_keys, const float* d_normals, const uint32_t* d_faces, uint32_t numVertices,
                              uint32_t numFaces, const uint32_t* d_root, const uint32_t* d_faceCount, const uint32_t* d_status, uint32_t minFaces,
                              uint32_t largestOnly, uint32_t* d_newIndex, uint64_t* d_best, VhVertex* d_outVertices, uint64_t* d_outKeys,
                              float* d_outNormals, uint32_t* d_outFaces, uint32_t* d_counts, vhStream_t stream)
{
    if (!d_status || !d_counts || !d_best) return VH_ERR_BAD_ARGUMENT;
    if (numVertices != 0 && (!d_vertices || !d_keys || !d_root || !d_faceCount || !d_newIndex || !d_outVertices || !d_outKeys)) return VH_ERR_BAD_ARGUMENT;
    if (numVertices != 0 && d_normals && !d_outNormals) return VH_ERR_BAD_ARGUMENT;
    if (numFaces != 0 && (!d_faces || !d_outFaces)) return VH_ERR_BAD_ARGUMENT;
    if (numVertices > 0x7ffffff0u || numFaces > 0x55555555u) return VH_ERR_BAD_ARGUMENT; // (as vh_mesh_components)
    hipStream_t s = (hipStream_t)stream;
    VH_HIP(hipMemsetAsync(d_counts, 0, sizeof(uint32_t) * VH_COMPONENTS_NUM_COUNTS, s));
    if (numVertices == 0) return VH_OK; // nothing to keep, and no launch with an empty grid
    const uint32_t grid = cdiv(numVertices, 256);
    unsigned long long* best = reinterpret_cast<unsigned long long*>(d_best);
    VH_LAUNCH_TIMED(k_components_stats, grid, 256, s, numVertices, d_root, d_faceCount, d_status, d_counts);
    VH_TRY(vh_last_launch_error());
    if (largestOnly != 0) {
        VH_HIP(hipMemsetAsync(d_best, 0xff, sizeof(uint64_t) * 2, s));
        VH_LAUNCH_TIMED(k_components_pick, grid, 256, s, numVertices, d_keys, d_root, d_faceCount, d_status, d_counts, best, 0u);
        VH_TRY(vh_last_launch_error());
        VH_LAUNCH_TIMED(k_components_pick, grid, 256, s, numVertices, d_keys, d_root, d_faceCount, d_status, d_counts, best, 1u);
        VH_TRY(vh_last_launch_error());
    }
    const ComponentFilterView c = { d_vertices, d_keys, d_normals, d_faces, d_root, d_faceCount, d_status, best, d_counts, d_newIndex,
                                    d_outVertices, d_outKeys, d_outNormals, d_outFaces, numVertices, numFaces, minFaces, largestOnly != 0 ? 1u : 0u };
    VH_LAUNCH_TIMED(k_components_compact_vertices, grid, 256, s, c);
    VH_TRY(vh_last_launch_error());
    if (numFaces == 0) return VH_OK;
    VH_LAUNCH_TIMED(k_components_compact_faces, cdiv(numFaces, 256), 256, s, c);
    return vh_last_launch_error();
}

} // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// the accumulating weld, host side

struct VhMeshWeldAccum {
    vh::DevicePtr<uint64_t> slotKeys, slotBids;
    vh::DevicePtr<uint32_t> slotVals;
    vh::DevicePtr<uint32_t> counts;     // VH_WELD_ACCUM_NUM_COUNTS words; the rehash count is m_rehashes
    vh::DevicePtr<uint32_t> vertexSlot; // of the append in flight
    vh::DevicePtr<VhVertex> vertices;
    vh::DevicePtr<uint64_t> keys;
    vh::DevicePtr<uint8_t> ranks;
    vh::DevicePtr<uint32_t> faces;
    VhMeshFinish finish;                // the passes over the welded mesh, and what of them holds since the last begin or append
    size_t m_soupCapacity = 0, m_vertexCapacity = 0, m_faceCapacity = 0; // in soup vertices, welded vertices, faces
    uint32_t m_slotsLog2 = 6, m_firstSlotsLog2 = 6;
    bool m_fixed = false, m_begun = false;
    uint32_t m_appends = 0, m_rehashes = 0;

    WeldAccumView view() const
    {
        return WeldAccumView{ slotKeys.get(), slotBids.get(), slotVals.get(), counts.get(), vertexSlot.get(), vertices.get(), keys.get(), ranks.get(), faces.get(), m_slotsLog2 };
    }
};

namespace {

// errors of the owner types (vh::deviceAlloc throws) become codes, as at the handle level
template <class F> int accumGuarded(F&& f)
{
    try {
        return f();
    } catch (const vh::Error& e) {
        return e.code ? e.code : VH_ERR_BAD_ARGUMENT;
    } catch (const std::exception&) {
        return -(int)hipErrorOutOfMemory;
    }
}

// a new, empty table of 1 << slotsLog2 slots; the one it replaces comes back in oldKeys / oldVals.  Nothing of `a`
// changes when an allocation fails.
int accumAllocTable(VhMeshWeldAccum& a, uint32_t slotsLog2, hipStream_t s, vh::DevicePtr<uint64_t>* oldKeys = nullptr, vh::DevicePtr<uint32_t>* oldVals = nullptr)
{
    const size_t numSlots = (size_t)1 << slotsLog2;
    vh::DevicePtr<uint64_t> keys = vh::deviceAlloc<uint64_t>(numSlots, "weld table keys"), bids = vh::deviceAlloc<uint64_t>(numSlots, "weld table bids");
    vh::DevicePtr<uint32_t> vals = vh::deviceAlloc<uint32_t>(numSlots, "weld table values");
    VH_HIP(hipMemsetAsync(keys.get(), 0xff, sizeof(uint64_t) * numSlots, s));
    VH_HIP(hipMemsetAsync(bids.get(), 0xff, sizeof(uint64_t) * numSlots, s));
    VH_HIP(hipMemsetAsync(vals.get(), 0xff, sizeof(uint32_t) * numSlots, s));
    VH_HIP(hipStreamSynchronize(s)); // nothing uses the old bid words any more when they go
    a.slotKeys.swap(keys);
    a.slotBids.swap(bids);
    a.slotVals.swap(vals);
    a.m_slotsLog2 = slotsLog2;
    if (oldKeys) *oldKeys = std::move(keys);
    if (oldVals) *oldVals = std::move(vals);
    return VH_OK;
}

// a larger array with the first `used` elements of the old one; the stream is idle when the old one goes
template <class T> int accumGrow(vh::DevicePtr<T>& p, size_t used, size_t capacity, const char* what, hipStream_t s)
{
    vh::DevicePtr<T> next = vh::deviceAlloc<T>(capacity, what);
    if (used) VH_HIP(hipMemcpyAsync(next.get(), p.get(), sizeof(T) * used, hipMemcpyDeviceToDevice, s));
    VH_HIP(hipStreamSynchronize(s));
    p = std::move(next);
    return VH_OK;
}

// A pass of the finish over the welded mesh: run(base).  Waits for the appends and reads their counts.  A weld that
// failed has nothing to pass on: its code comes back, nothing runs, and what the pass held before is gone all the same.
template <class F> int accumStage(VhMeshWeldAccum* accum, VhFinishStage stage, vhStream_t stream, F&& run)
{
    return accumGuarded([&]() -> int {
        accum->finish.state.start(stage);
        uint32_t have[VH_WELD_ACCUM_NUM_COUNTS] = {};
        VH_TRY(vh_mesh_weld_accum_get_counts(accum, have, stream));
        return run(vh_mesh_weld_accum_base(accum, have[VH_WELD_ACCUM_VERTICES], have[VH_WELD_ACCUM_FACES]));
    });
}

} // namespace

VhMeshFinish& vh_mesh_weld_accum_finish(VhMeshWeldAccum* accum) { return accum->finish; }
VhMeshView vh_mesh_weld_accum_base(const VhMeshWeldAccum* accum, uint32_t numVertices, uint32_t numFaces)
{
    return VhMeshView{ accum->vertices.get(), accum->keys.get(), accum->faces.get(), nullptr, numVertices, numFaces };
}

extern "C" {

int vh_mesh_weld_accum_create(uint32_t slotsLog2, uint32_t reserveTriangles, int fixed, VhMeshWeldAccum** out)
{
    if (!out) return VH_ERR_BAD_ARGUMENT;
    *out = nullptr;
    if (slotsLog2 == 0) slotsLog2 = 6;
    if (slotsLog2 > 31 || reserveTriangles > 0x55555555u / 2u) return VH_ERR_BAD_ARGUMENT;
    return accumGuarded([&]() -> int {
        std::unique_ptr<VhMeshWeldAccum> a(new VhMeshWeldAccum);
        a->m_fixed = fixed != 0;
        a->m_firstSlotsLog2 = slotsLog2;
        a->counts = vh::deviceAlloc<uint32_t>(8, "weld counts");
        a->m_vertexCapacity = 3 * (size_t)reserveTriangles;
        a->m_faceCapacity = reserveTriangles;
        a->vertices = vh::deviceAlloc<VhVertex>(a->m_vertexCapacity, "welded vertices");
        a->keys = vh::deviceAlloc<uint64_t>(a->m_vertexCapacity, "welded vertex keys");
        a->ranks = vh::deviceAlloc<uint8_t>(a->m_vertexCapacity, "welded vertex ranks");
        a->faces = vh::deviceAlloc<uint32_t>(3 * a->m_faceCapacity, "welded faces");
        VH_TRY(accumAllocTable(*a, slotsLog2, nullptr));
        VH_HIP(hipMemsetAsync(a->counts.get(), 0, sizeof(uint32_t) * 8, nullptr));
        VH_HIP(hipStreamSynchronize(nullptr));
        a->m_begun = true;
        *out = a.release();
        return VH_OK;
    });
}

void vh_mesh_weld_accum_destroy(VhMeshWeldAccum* accum) { delete accum; }

int vh_mesh_weld_accum_begin(VhMeshWeldAccum* accum, vhStream_t stream)
{
    if (!accum) return VH_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    const size_t numSlots = (size_t)1 << accum->m_slotsLog2;
    VH_HIP(hipMemsetAsync(accum->counts.get(), 0, sizeof(uint32_t) * 8, s));
    VH_HIP(hipMemsetAsync(accum->slotKeys.get(), 0xff, sizeof(uint64_t) * numSlots, s));
    VH_HIP(hipMemsetAsync(accum->slotBids.get(), 0xff, sizeof(uint64_t) * numSlots, s));
    VH_HIP(hipMemsetAsync(accum->slotVals.get(), 0xff, sizeof(uint32_t) * numSlots, s));
    accum->m_appends = 0;
    accum->m_rehashes = 0;
    accum->m_begun = true;
    accum->finish.invalidateFrom(VH_FINISH_CLUSTER);
    return VH_OK;
}

int vh_mesh_weld_accum_append(VhMeshWeldAccum* accum, const VhTriangle* d_triangles, const VhTriangleSource* d_sources, uint32_t numTriangles,
                              vhStream_t stream)
{
    if (!accum || !accum->m_begun) return VH_ERR_BAD_ARGUMENT;
    if (numTriangles > 0x55555555u / 2u || (numTriangles != 0 && (!d_triangles || !d_sources))) return VH_ERR_BAD_ARGUMENT;
    // a cluster, a vertex's neighbours and a component span appends, and normals are of all faces with the final vertex
    // bits: every pass before this append is stale
    accum->finish.invalidateFrom(VH_FINISH_CLUSTER);
    if (numTriangles == 0) return VH_OK; // nothing to take, and no launch with an empty grid
    if (accum->m_appends >= VH_WELD_ACCUM_MAX_APPENDS - 1u) return VH_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    return accumGuarded([&]() -> int {
        VhMeshWeldAccum& a = *accum;
        // what the appends before this one left: sizes the table and the arrays
        uint32_t have[VH_WELD_ACCUM_NUM_COUNTS] = {};
        VH_HIP(hipMemcpyAsync(have, a.counts.get(), sizeof(uint32_t) * 5, hipMemcpyDeviceToHost, s));
        VH_HIP(hipStreamSynchronize(s));
        if (have[VH_WELD_ACCUM_STATUS] != 0u) return VH_OK; // the kernels would do nothing
        const uint64_t n = numTriangles;
        const uint64_t needKeys = (uint64_t)have[VH_WELD_ACCUM_VERTICES] + have[VH_WELD_ACCUM_CELLS] + 4ull * n;
        if ((uint64_t)have[VH_WELD_ACCUM_VERTICES] + 3ull * n >= kDroppedSlot || (uint64_t)have[VH_WELD_ACCUM_FACES] + n > 0x55555555ull)
            return VH_ERR_BAD_ARGUMENT; // vertex indices and face offsets are 32 bits
        if (!a.m_fixed) {
            uint32_t l = a.m_slotsLog2;
            while (l < 31u && (1ull << l) < 2ull * needKeys) l++;
            if ((1ull << l) < 2ull * needKeys) return VH_ERR_BAD_ARGUMENT;
            if (l != a.m_slotsLog2) {
                vh::DevicePtr<uint64_t> oldKeys;
                vh::DevicePtr<uint32_t> oldVals;
                const uint32_t oldLog2 = a.m_slotsLog2;
                VH_TRY(accumAllocTable(a, l, s, &oldKeys, &oldVals));
                if (have[VH_WELD_ACCUM_VERTICES] + have[VH_WELD_ACCUM_CELLS] != 0u) {
                    k_weld_rehash<<<cdiv((size_t)1 << oldLog2, 256), 256, 0, s>>>(oldKeys.get(), oldVals.get(), oldLog2, a.view());
                    VH_TRY(vh_last_launch_error());
                }
                VH_HIP(hipStreamSynchronize(s)); // the old table goes at the end of this block
                a.m_rehashes += l - oldLog2;
            }
        }
        const size_t needVertices = (size_t)have[VH_WELD_ACCUM_VERTICES] + 3 * (size_t)n, needFaces = (size_t)have[VH_WELD_ACCUM_FACES] + (size_t)n;
        if (needVertices > a.m_vertexCapacity) {
            const size_t cap = std::max(needVertices, 2 * a.m_vertexCapacity), used = have[VH_WELD_ACCUM_VERTICES];
            VH_TRY(accumGrow(a.vertices, used, cap, "welded vertices", s));
            VH_TRY(accumGrow(a.keys, used, cap, "welded vertex keys", s));
            VH_TRY(accumGrow(a.ranks, used, cap, "welded vertex ranks", s));
            a.m_vertexCapacity = cap;
        }
        if (needFaces > a.m_faceCapacity) {
            const size_t cap = std::max(needFaces, 2 * a.m_faceCapacity);
            VH_TRY(accumGrow(a.faces, 3 * (size_t)have[VH_WELD_ACCUM_FACES], 3 * cap, "welded faces", s));
            a.m_faceCapacity = cap;
        }
        if (3 * (size_t)n > a.m_soupCapacity) {
            VH_HIP(hipStreamSynchronize(s));
            a.vertexSlot = vh::deviceAlloc<uint32_t>(3 * (size_t)n, "weld vertex slots");
            a.m_soupCapacity = 3 * (size_t)n;
        }
        const uint32_t ordinal = ++a.m_appends; // 1 ..: all ones in a cell's value means no owner
        const WeldAccumView w = a.view();
        VH_LAUNCH_TIMED(k_weld_accum_insert, cdiv(n, 256), 256, s, d_sources, numTriangles, w, ordinal);
        VH_TRY(vh_last_launch_error());
        VH_LAUNCH_TIMED(k_weld_accum_settle, cdiv(3ull * n, 256), 256, s, d_triangles, 3u * numTriangles, w, ordinal);
        VH_TRY(vh_last_launch_error());
        VH_LAUNCH_TIMED(k_weld_accum_faces, cdiv(n, 256), 256, s, numTriangles, w);
        return vh_last_launch_error();
    });
}

int vh_mesh_weld_accum_get_counts(VhMeshWeldAccum* accum, uint32_t out[6], vhStream_t stream)
{
    if (!accum || !out) return VH_ERR_BAD_ARGUMENT;
    VH_HIP(hipMemcpyAsync(out, accum->counts.get(), sizeof(uint32_t) * 5, hipMemcpyDeviceToHost, (hipStream_t)stream));
    VH_HIP(hipStreamSynchronize((hipStream_t)stream));
    out[VH_WELD_ACCUM_REHASHES] = accum->m_rehashes;
    if (out[VH_WELD_ACCUM_STATUS] != 0u)
        out[VH_WELD_ACCUM_VERTICES] = out[VH_WELD_ACCUM_FACES] = out[VH_WELD_ACCUM_CELLS] = out[VH_WELD_ACCUM_DROPPED] = 0u; // nothing of it is a mesh
    return weldStatusCode(out[VH_WELD_ACCUM_STATUS]);
}

int vh_mesh_weld_accum_download(VhMeshWeldAccum* accum, VhVertex* vertices, uint64_t* keys, uint32_t* faces, uint32_t numVertices,
                                uint32_t numFaces, vhStream_t stream)
{
    if (!accum) return VH_ERR_BAD_ARGUMENT;
    if (numVertices > accum->m_vertexCapacity || numFaces > accum->m_faceCapacity) return VH_ERR_BAD_ARGUMENT;
    return VhMeshFinish::download(vh_mesh_weld_accum_base(accum, numVertices, numFaces), vertices, keys, nullptr, faces, stream);
}

int vh_mesh_weld_accum_normals(VhMeshWeldAccum* accum, int32_t scaleLog2, vhStream_t stream)
{
    if (!accum || !accum->m_begun || scaleLog2 < -100 || scaleLog2 > 100) return VH_ERR_BAD_ARGUMENT;
    return accumStage(accum, VH_FINISH_NORMALS, stream, [&](const VhMeshView& base) { return accum->finish.normals(base, scaleLog2, stream); });
}

int vh_mesh_weld_accum_download_normals(VhMeshWeldAccum* accum, float* normals, uint32_t numVertices, vhStream_t stream)
{
    if (!accum || !accum->finish.state.valid(VH_FINISH_NORMALS) || numVertices > accum->finish.state.vertices[VH_FINISH_NORMALS] || (numVertices != 0 && !normals))
        return VH_ERR_BAD_ARGUMENT;
    return accum->finish.m_normals.download(normals, numVertices, true, stream);
}

int vh_mesh_weld_accum_components(VhMeshWeldAccum* accum, uint32_t minFaces, uint32_t largestOnly, vhStream_t stream)
{
    if (!accum || !accum->m_begun) return VH_ERR_BAD_ARGUMENT;
    return accumStage(accum, VH_FINISH_COMPONENTS, stream, [&](const VhMeshView& base) { return accum->finish.components(base, minFaces, largestOnly, stream); });
}

int vh_mesh_weld_accum_cluster(VhMeshWeldAccum* accum, uint32_t cellsPerCluster, int32_t scaleLog2, vhStream_t stream)
{
    if (!accum || !accum->m_begun || cellsPerCluster > VH_CLUSTER_MAX_CELLS || scaleLog2 < -100 || scaleLog2 > 100) return VH_ERR_BAD_ARGUMENT;
    if (cellsPerCluster == 0u) { // forget the pass: the passes of the finish are of the welded mesh again
        accum->finish.forget(VH_FINISH_CLUSTER);
        return VH_OK;
    }
    // (a status the pass left is vh_mesh_weld_accum_cluster_get_counts' to report)
    return accumStage(accum, VH_FINISH_CLUSTER, stream, [&](const VhMeshView& base) { return accum->finish.cluster(base, cellsPerCluster, scaleLog2, stream); });
}

int vh_mesh_weld_accum_cluster_get_counts(VhMeshWeldAccum* accum, uint32_t out[6], vhStream_t stream)
{
    if (!accum || !out || !accum->finish.state.ran[VH_FINISH_CLUSTER]) return VH_ERR_BAD_ARGUMENT;
    return accum->finish.m_cluster.counts(out, stream);
}

int vh_mesh_weld_accum_cluster_download(VhMeshWeldAccum* accum, VhVertex* vertices, uint64_t* keys, uint32_t* faces, uint32_t numVertices, uint32_t numFaces,
                                        vhStream_t stream)
{
    if (!accum || !accum->finish.state.valid(VH_FINISH_CLUSTER)) return VH_ERR_BAD_ARGUMENT;
    const VhMeshFinish& f = accum->finish;
    if (numVertices > f.state.vertices[VH_FINISH_CLUSTER] || numFaces > f.state.faces[VH_FINISH_CLUSTER]) return VH_ERR_BAD_ARGUMENT;
    return VhMeshFinish::download(VhMeshView{ f.m_cluster.vertices.get(), f.m_cluster.keys.get(), f.m_cluster.faces.get(), nullptr, numVertices, numFaces }, vertices, keys,
                                  nullptr, faces, stream);
}

int vh_mesh_weld_accum_smooth(VhMeshWeldAccum* accum, uint32_t iterations, int32_t lambdaQ16, int32_t muQ16, uint32_t keepBoundary, int32_t scaleLog2,
                              vhStream_t stream)
{
    if (!accum || !accum->m_begun || iterations > VH_SMOOTH_MAX_ITERATIONS || keepBoundary > 1u || scaleLog2 < -100 || scaleLog2 > 100) return VH_ERR_BAD_ARGUMENT;
    if (lambdaQ16 < -VH_SMOOTH_MAX_FACTOR_Q16 || lambdaQ16 > VH_SMOOTH_MAX_FACTOR_Q16 || muQ16 < -VH_SMOOTH_MAX_FACTOR_Q16 || muQ16 > VH_SMOOTH_MAX_FACTOR_Q16)
        return VH_ERR_BAD_ARGUMENT;
    if (iterations == 0u) { // forget the pass: the passes of the finish take the vertices as they were again
        accum->finish.forget(VH_FINISH_SMOOTH);
        return VH_OK;
    }
    // (a status the pass left is vh_mesh_weld_accum_smooth_get_counts' to report)
    return accumStage(accum, VH_FINISH_SMOOTH, stream, [&](const VhMeshView& base) {
        return accum->finish.smooth(base, iterations, lambdaQ16, muQ16, keepBoundary, scaleLog2, stream);
    });
}

int vh_mesh_weld_accum_smooth_get_counts(VhMeshWeldAccum* accum, uint32_t out[6], vhStream_t stream)
{
    if (!accum || !out || !accum->finish.state.ran[VH_FINISH_SMOOTH]) return VH_ERR_BAD_ARGUMENT;
    return accum->finish.m_smooth.counts(out, stream);
}

int vh_mesh_weld_accum_smooth_download(VhMeshWeldAccum* accum, VhVertex* vertices, uint32_t numVertices, vhStream_t stream)
{
    if (!accum || !accum->finish.state.valid(VH_FINISH_SMOOTH) || numVertices > accum->finish.state.vertices[VH_FINISH_SMOOTH]) return VH_ERR_BAD_ARGUMENT;
    return VhMeshFinish::download(VhMeshView{ accum->finish.m_smooth.vertices.get(), nullptr, nullptr, nullptr, numVertices, 0u }, vertices, nullptr, nullptr, nullptr, stream);
}

int vh_mesh_weld_accum_components_get_counts(VhMeshWeldAccum* accum, uint32_t out[6], vhStream_t stream)
{
    if (!accum || !out || !accum->finish.state.valid(VH_FINISH_COMPONENTS)) return VH_ERR_BAD_ARGUMENT;
    return accum->finish.m_components.counts(out, stream);
}

int vh_mesh_weld_accum_components_download(VhMeshWeldAccum* accum, VhVertex* vertices, uint64_t* keys, float* normals, uint32_t* faces,
                                           uint32_t numVertices, uint32_t numFaces, vhStream_t stream)
{
    if (!accum || !accum->finish.state.valid(VH_FINISH_COMPONENTS)) return VH_ERR_BAD_ARGUMENT;
    const VhMeshComponents& c = accum->finish.m_components; // the caller has the kept counts; what bounds them here is the room there is
    if (numVertices > c.vertexCapacity || numFaces > c.faceCapacity) return VH_ERR_BAD_ARGUMENT;
    return VhMeshFinish::download(VhMeshView{ c.vertices.get(), c.keys.get(), c.faces.get(), c.hasNormals ? c.normals.get() : nullptr, numVertices, numFaces }, vertices, keys,
                                  normals, faces, stream);
}

} // extern "C"
