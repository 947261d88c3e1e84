// vh_mesh_components.hpp -- who owns the buffers of the component pass (vh_mesh_components, vh_mesh_components_filter;
// DESIGN.md section 4, "Mesh components").  A stage of the finish's chain (vh_mesh_finish.hpp), which owns one and downloads
// what it made.
#pragma once

#include <algorithm>

#include "vh_host_util.hpp"

struct VhMeshComponents {
    vh::DevicePtr<uint32_t> root, faceCount, newIndex; // one per vertex of the input
    vh::DevicePtr<uint32_t> words;                     // the status word, then the VH_COMPONENTS_NUM_COUNTS counts
    vh::DevicePtr<uint64_t> best;                      // two words of the pick of the largest component
    vh::DevicePtr<VhVertex> vertices;                  // the filtered mesh: nothing is compacted in place
    vh::DevicePtr<uint64_t> keys;
    vh::DevicePtr<float> normals;                      // 3 per vertex; made by the first run that carries normals
    vh::DevicePtr<uint32_t> faces;
    size_t vertexCapacity = 0, normalCapacity = 0, faceCapacity = 0; // vertices, vertices, faces
    bool hasNormals = false;                           // the last run carried them

    // room for a mesh of nv vertices and nf faces, made by the first use; grows to max(n, 2 capacity).  Throws vh::Error.
    void ensure(uint32_t nv, uint32_t nf, bool withNormals)
    {
        if (!words) {
            words = vh::deviceAlloc<uint32_t>(1 + VH_COMPONENTS_NUM_COUNTS, "component status and counts");
            best = vh::deviceAlloc<uint64_t>(2, "component pick");
        }
        if (nv > vertexCapacity) {
            const size_t cap = std::max((size_t)nv, 2 * vertexCapacity);
            root = vh::deviceAlloc<uint32_t>(cap, "component roots");
            faceCount = vh::deviceAlloc<uint32_t>(cap, "component face counts");
            newIndex = vh::deviceAlloc<uint32_t>(cap, "component vertex numbers");
            vertices = vh::deviceAlloc<VhVertex>(cap, "filtered vertices");
            keys = vh::deviceAlloc<uint64_t>(cap, "filtered vertex keys");
            vertexCapacity = cap;
        }
        if (withNormals && vertexCapacity > normalCapacity) {
            normals = vh::deviceAlloc<float>(3 * vertexCapacity, "filtered vertex normals");
            normalCapacity = vertexCapacity;
        }
        if (nf > faceCapacity) {
            const size_t cap = std::max((size_t)nf, 2 * faceCapacity);
            faces = vh::deviceAlloc<uint32_t>(3 * cap, "filtered faces");
            faceCapacity = cap;
        }
    }

    // label, then filter, a welded mesh on the device into these buffers; d_normals may be null
    int run(const VhVertex* d_vertices, const uint64_t* d_keys, const float* d_normals, const uint32_t* d_faces, uint32_t nv, uint32_t nf, uint32_t minFaces,
            uint32_t largestOnly, vhStream_t stream)
    {
        ensure(nv, nf, d_normals != nullptr);
        hasNormals = d_normals != nullptr;
        VH_TRY(vh_mesh_components(d_keys, d_faces, nv, nf, root.get(), faceCount.get(), words.get(), stream));
        return vh_mesh_components_filter(d_vertices, d_keys, d_normals, d_faces, nv, nf, root.get(), faceCount.get(), words.get(), minFaces, largestOnly,
                                         newIndex.get(), best.get(), vertices.get(), keys.get(), normals.get(), faces.get(), words.get() + 1, stream);
    }

    // waits and reads the six counts of the last run: VH_ERR_BAD_ARGUMENT when the labelling left a status (they are then 0)
    int counts(uint32_t out[VH_COMPONENTS_NUM_COUNTS], vhStream_t stream) const
    {
        uint32_t w[1 + VH_COMPONENTS_NUM_COUNTS] = {};
        VH_HIP(hipMemcpyAsync(w, words.get(), sizeof(w), hipMemcpyDeviceToHost, (hipStream_t)stream));
        VH_HIP(hipStreamSynchronize((hipStream_t)stream));
        std::copy(w + 1, w + 1 + VH_COMPONENTS_NUM_COUNTS, out);
        return w[0] != 0u ? VH_ERR_BAD_ARGUMENT : VH_OK;
    }
};
