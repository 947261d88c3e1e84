// vh_mesh_smooth.hpp -- who owns the buffers of the Taubin smoothing (vh_mesh_smooth; DESIGN.md section 4, "Mesh
// smoothing").  A stage of the finish's chain (vh_mesh_finish.hpp), which owns one and downloads what it made.
#pragma once

#include <algorithm>

#include "vh_host_util.hpp"

struct VhMeshSmooth {
    vh::DevicePtr<uint64_t> edgeKeys;                          // the edge table: one per slot
    vh::DevicePtr<uint32_t> edgeUses;
    vh::DevicePtr<uint32_t> degree, flags;                     // one per vertex of the input
    vh::DevicePtr<int64_t> positions, sums;                    // 2 x 3 and 3 per vertex
    vh::DevicePtr<uint32_t> words;                             // the VH_SMOOTH_NUM_COUNTS counts, then the five work words
    vh::DevicePtr<VhVertex> vertices;                          // the smoothed vertices: the input stays as it is
    size_t vertexCapacity = 0, faceCapacity = 0;               // vertices and faces of the input there is room for
    uint32_t edgeSlotsLog2 = 0;                                // of the table there is

    // room for a mesh of nv vertices and nf faces, made by the first use; grows to max(n, 2 capacity), the table to the
    // power of two that is at least six times that.  Throws vh::Error.
    void ensure(uint32_t nv, uint32_t nf)
    {
        if (!words) words = vh::deviceAlloc<uint32_t>(VH_SMOOTH_NUM_COUNTS + 5, "smoothing counts");
        if (nv > vertexCapacity || !degree) {
            const size_t cap = std::max<size_t>(std::max((size_t)nv, 2 * vertexCapacity), 1);
            degree = vh::deviceAlloc<uint32_t>(cap, "smoothing degrees");
            flags = vh::deviceAlloc<uint32_t>(cap, "smoothing vertex flags");
            positions = vh::deviceAlloc<int64_t>(6 * cap, "smoothing fixed-point positions");
            sums = vh::deviceAlloc<int64_t>(3 * cap, "smoothing neighbour sums");
            vertices = vh::deviceAlloc<VhVertex>(cap, "smoothed vertices");
            vertexCapacity = cap;
        }
        if (nf > faceCapacity || !edgeKeys) {
            const size_t cap = std::min<size_t>(std::max((size_t)nf, 2 * faceCapacity), 0x15555555u);
            uint32_t log2 = 0;
            check(vh_mesh_smooth_default_slots_log2((uint32_t)cap, &log2), "vh_mesh_smooth_default_slots_log2");
            const size_t slots = (size_t)1 << log2;
            edgeKeys = vh::deviceAlloc<uint64_t>(slots, "smoothing edge table keys");
            edgeUses = vh::deviceAlloc<uint32_t>(slots, "smoothing edge use counts");
            faceCapacity = cap;
            edgeSlotsLog2 = log2;
        }
    }

    // the buffers as the launcher takes them, the table cut to what a mesh of nf faces needs
    VhMeshSmoothData data(uint32_t nf) const
    {
        VhMeshSmoothData d = { edgeKeys.get(), edgeUses.get(), degree.get(), flags.get(), positions.get(), sums.get(),
                               words.get() + VH_SMOOTH_NUM_COUNTS, vertices.get(), words.get(), 0u, 0u };
        (void)vh_mesh_smooth_default_slots_log2(nf, &d.m_edgeSlotsLog2);
        return d;
    }

    // smooth an indexed mesh on the device into these buffers
    int run(const VhVertex* d_vertices, const uint64_t* d_keys, const uint32_t* d_faces, uint32_t nv, uint32_t nf, uint32_t iterations, int32_t lambdaQ16,
            int32_t muQ16, uint32_t keepBoundary, int32_t scaleLog2, vhStream_t stream)
    {
        if (nv > 0x40000000u || nf > 0x15555555u) return VH_ERR_BAD_ARGUMENT;
        ensure(nv, nf);
        const VhMeshSmoothData d = data(nf);
        return vh_mesh_smooth(d_vertices, d_keys, d_faces, nv, nf, iterations, lambdaQ16, muQ16, keepBoundary, scaleLog2, &d, stream);
    }

    // waits and reads the six counts of the last run.  A status leaves the other five 0: a full table is
    // VH_ERR_STAGING_OVERFLOW, as for the weld, every other bit VH_ERR_BAD_ARGUMENT.
    int counts(uint32_t out[VH_SMOOTH_NUM_COUNTS], vhStream_t stream) const
    {
        VH_HIP(hipMemcpyAsync(out, words.get(), sizeof(uint32_t) * VH_SMOOTH_NUM_COUNTS, hipMemcpyDeviceToHost, (hipStream_t)stream));
        VH_HIP(hipStreamSynchronize((hipStream_t)stream));
        const uint32_t status = out[VH_SMOOTH_STATUS];
        if (status & ~VH_SMOOTH_TABLE_FULL) return VH_ERR_BAD_ARGUMENT;
        return status != 0u ? VH_ERR_STAGING_OVERFLOW : VH_OK;
    }
};
