// vh_mesh_table.hpp -- what the indexed-mesh passes share on the device: the open-addressing table of 64-bit keys that the
// weld (vh_mesh.hip) and the clustering (vh_mesh_cluster.hip) probe; the one-atomic-per-wave list helpers they use come
// with vh_scene_ops.hpp.
#pragma once

#include "vh_device.hpp"
#include "vh_mesh_key.hpp"
#include "vh_scene_ops.hpp"

namespace {

// the slot a key starts probing at (the 64-bit finaliser of MurmurHash3)
VHD uint32_t weld_home(uint64_t k, uint32_t mask)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (uint32_t)k & mask;
}

constexpr uint32_t kNoSlot = 0xffffffffu;

// the slot of `key`, claimed if the table does not have it; kNoSlot after numSlots steps without one
VHD uint32_t weld_find_or_claim(unsigned long long* slotKeys, uint64_t key, uint32_t slotsLog2)
{
    const uint32_t numSlots = 1u << slotsLog2, mask = numSlots - 1u;
    uint32_t slot = weld_home(key, mask);
#pragma unroll 1
    for (uint32_t step = 0; step < numSlots; step++) {
        unsigned long long have = slotKeys[slot];
        if (have == kMeshKeyEmpty) have = atomicCAS(&slotKeys[slot], (unsigned long long)kMeshKeyEmpty, (unsigned long long)key);
        if (have == kMeshKeyEmpty || have == key) return slot;
        slot = (slot + 1u) & mask;
    }
    return kNoSlot;
}

} // namespace
