// vh_mesh_normals.hpp -- who owns the buffers of the vertex-normal pass (vh_mesh_vertex_normals; DESIGN.md section 4,
// "Vertex normals").  A stage of the finish's chain (vh_mesh_finish.hpp), which owns one.
#pragma once

#include <algorithm>

#include "vh_host_util.hpp"

struct VhMeshNormals {
    vh::DevicePtr<int64_t> acc;     // 3 per vertex
    vh::DevicePtr<float> normals;   // 3 per vertex
    vh::DevicePtr<uint32_t> status; // one word
    size_t capacity = 0;            // vertices

    // room for nv vertices, made by the first use; grows to max(nv, 2 capacity).  Throws vh::Error.
    void ensure(uint32_t nv)
    {
        if (!status) status = vh::deviceAlloc<uint32_t>(1, "vertex normal status");
        if (nv <= capacity) return;
        const size_t cap = std::max((size_t)nv, 2 * capacity);
        acc = vh::deviceAlloc<int64_t>(3 * cap, "vertex normal accumulators");
        normals = vh::deviceAlloc<float>(3 * cap, "vertex normals");
        capacity = cap;
    }

    // the pass over a welded mesh on the device, into these buffers
    int run(const VhVertex* d_vertices, const uint64_t* d_keys, const uint32_t* d_faces, uint32_t nv, uint32_t nf, int32_t scaleLog2, vhStream_t stream)
    {
        ensure(nv);
        return vh_mesh_vertex_normals(d_vertices, d_keys, d_faces, nv, nf, scaleLog2, acc.get(), normals.get(), status.get(), stream);
    }

    // 3 nv floats of the last run, and with them its status word if asked: VH_ERR_BAD_ARGUMENT when the pass left one
    int download(float* out, uint32_t nv, bool withStatus, vhStream_t stream) const
    {
        hipStream_t s = (hipStream_t)stream;
        uint32_t word = 0u;
        if (withStatus) VH_HIP(hipMemcpyAsync(&word, status.get(), sizeof(word), hipMemcpyDeviceToHost, s));
        if (nv) VH_HIP(hipMemcpyAsync(out, normals.get(), sizeof(float) * 3 * (size_t)nv, hipMemcpyDeviceToHost, s));
        VH_HIP(hipStreamSynchronize(s));
        return word != 0u ? VH_ERR_BAD_ARGUMENT : VH_OK;
    }
};
