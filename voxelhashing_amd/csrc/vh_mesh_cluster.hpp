// vh_mesh_cluster.hpp -- who owns the buffers of the vertex clustering (vh_mesh_cluster; DESIGN.md section 4, "Mesh
// clustering").  A stage of the finish's chain (vh_mesh_finish.hpp), which owns one and downloads what it made.
#pragma once

#include <algorithm>

#include "vh_host_util.hpp"

struct VhMeshCluster {
    vh::DevicePtr<uint64_t> clusterKeys;                       // the cluster table: one per slot
    vh::DevicePtr<int64_t> clusterSums;                        // 6 per slot
    vh::DevicePtr<uint32_t> clusterCount, clusterIndex;
    vh::DevicePtr<uint32_t> vertexSlot;                        // one per vertex of the input
    vh::DevicePtr<uint64_t> facePairs;                         // the face table: one per slot
    vh::DevicePtr<uint32_t> faceThirds, faceWindings;
    vh::DevicePtr<uint32_t> words;                             // the VH_CLUSTER_NUM_COUNTS counts, then the two work words
    vh::DevicePtr<VhVertex> vertices;                          // the clustered mesh: nothing is compacted in place
    vh::DevicePtr<uint64_t> keys;
    vh::DevicePtr<uint32_t> faces;
    size_t vertexCapacity = 0, faceCapacity = 0;               // vertices and faces of the input there is room for
    uint32_t clusterSlotsLog2 = 0, faceSlotsLog2 = 0;          // of the tables there are

    // room for a mesh of nv vertices and nf faces, made by the first use; grows to max(n, 2 capacity), the tables to
    // the power of two that is at least twice that.  Throws vh::Error.
    void ensure(uint32_t nv, uint32_t nf)
    {
        if (!words) words = vh::deviceAlloc<uint32_t>(VH_CLUSTER_NUM_COUNTS + 2, "cluster counts");
        if (nv > vertexCapacity || !clusterKeys) {
            const size_t cap = std::max((size_t)nv, 2 * vertexCapacity);
            uint32_t log2 = 0;
            check(vh_mesh_cluster_default_slots_log2((uint32_t)std::min<size_t>(cap, 0x40000000u), &log2), "vh_mesh_cluster_default_slots_log2");
            const size_t slots = (size_t)1 << log2;
            clusterKeys = vh::deviceAlloc<uint64_t>(slots, "cluster table keys");
            clusterSums = vh::deviceAlloc<int64_t>(6 * slots, "cluster sums");
            clusterCount = vh::deviceAlloc<uint32_t>(slots, "cluster member counts");
            clusterIndex = vh::deviceAlloc<uint32_t>(slots, "cluster vertex numbers");
            vertexSlot = vh::deviceAlloc<uint32_t>(cap, "cluster slots of the vertices");
            vertices = vh::deviceAlloc<VhVertex>(cap, "clustered vertices");
            keys = vh::deviceAlloc<uint64_t>(cap, "clustered vertex keys");
            vertexCapacity = cap;
            clusterSlotsLog2 = log2;
        }
        if (nf > faceCapacity || !facePairs) {
            const size_t cap = std::max((size_t)nf, 2 * faceCapacity);
            uint32_t log2 = 0;
            check(vh_mesh_cluster_default_slots_log2((uint32_t)std::min<size_t>(cap, 0x40000000u), &log2), "vh_mesh_cluster_default_slots_log2");
            const size_t slots = (size_t)1 << log2;
            facePairs = vh::deviceAlloc<uint64_t>(slots, "cluster face table pairs");
            faceThirds = vh::deviceAlloc<uint32_t>(slots, "cluster face table thirds");
            faceWindings = vh::deviceAlloc<uint32_t>(slots, "cluster face table windings");
            faces = vh::deviceAlloc<uint32_t>(3 * cap, "clustered faces");
            faceCapacity = cap;
            faceSlotsLog2 = log2;
        }
    }

    // the buffers as the launcher takes them, the tables cut to what a mesh of nv vertices and nf faces needs
    VhMeshClusterData data(uint32_t nv, uint32_t nf) const
    {
        VhMeshClusterData d = { clusterKeys.get(), clusterSums.get(), clusterCount.get(), clusterIndex.get(), vertexSlot.get(), facePairs.get(), faceThirds.get(),
                                faceWindings.get(), words.get() + VH_CLUSTER_NUM_COUNTS, vertices.get(), keys.get(), faces.get(), words.get(), 0u, 0u };
        (void)vh_mesh_cluster_default_slots_log2(nv, &d.m_clusterSlotsLog2);
        (void)vh_mesh_cluster_default_slots_log2(nf, &d.m_faceSlotsLog2);
        return d;
    }

    // cluster a welded mesh on the device into these buffers
    int run(const VhVertex* d_vertices, const uint64_t* d_keys, const uint32_t* d_faces, uint32_t nv, uint32_t nf, uint32_t cellsPerCluster, int32_t scaleLog2,
            vhStream_t stream)
    {
        if (nv > 0x40000000u || nf > 0x40000000u) return VH_ERR_BAD_ARGUMENT;
        ensure(nv, nf);
        const VhMeshClusterData d = data(nv, nf);
        return vh_mesh_cluster(d_vertices, d_keys, d_faces, nv, nf, cellsPerCluster, scaleLog2, &d, stream);
    }

    // waits and reads the six counts of the last run.  A status leaves the other five 0: a full table is
    // VH_ERR_STAGING_OVERFLOW, as for the weld, every other bit VH_ERR_BAD_ARGUMENT.
    int counts(uint32_t out[VH_CLUSTER_NUM_COUNTS], vhStream_t stream) const
    {
        VH_HIP(hipMemcpyAsync(out, words.get(), sizeof(uint32_t) * VH_CLUSTER_NUM_COUNTS, hipMemcpyDeviceToHost, (hipStream_t)stream));
        VH_HIP(hipStreamSynchronize((hipStream_t)stream));
        const uint32_t status = out[VH_CLUSTER_STATUS];
        if (status & ~VH_CLUSTER_TABLE_FULL) return VH_ERR_BAD_ARGUMENT;
        return status != 0u ? VH_ERR_STAGING_OVERFLOW : VH_OK;
    }
};
