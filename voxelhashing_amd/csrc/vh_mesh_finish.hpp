// vh_mesh_finish.hpp -- the finish of the indexed mesh as one chain ("The finish as one chain"):
// clustering, smoothing, normals, components, in that order, over a welded mesh that stays where it is.  The accumulating
// weld (vh_mesh.hip) holds one chain for its appends, the one-shot indexed extraction (vh_marching_cubes.cpp) one for
// its weld; vh_mesh_weld_accum_* and readBackIndexed are calls on it.
//
// The first part is the bookkeeping alone -- which stage has run, which holds a mesh, what a later stage takes from the
// earlier ones -- in plain integers: with VH_MESH_FINISH_STATE_ONLY defined nothing else is compiled, and
// tests/test_mesh_finish_state.py walks it without a device.
#pragma once

#include <cstdint>

enum VhFinishStage { VH_FINISH_CLUSTER = 0, VH_FINISH_SMOOTH, VH_FINISH_NORMALS, VH_FINISH_COMPONENTS, VH_FINISH_NUM_STAGES };

struct VhMeshFinishState {
    bool ran[VH_FINISH_NUM_STAGES] = {};  // since the last begin or append, and since the last run of a stage it takes from
    int code[VH_FINISH_NUM_STAGES] = {};  // what its counts read back as at the run (0: VH_OK).  Nobody reads those of the
                                          // normals and the components then, so theirs is 0: their queries report the status
    uint32_t vertices[VH_FINISH_NUM_STAGES] = {}, faces[VH_FINISH_NUM_STAGES] = {}; // cluster: of its mesh; smooth, normals: of the
                                          // mesh it ran over; components: of the kept mesh, once its counts were read

    bool valid(int stage) const { return ran[stage] && code[stage] == 0; }

    void reset(int s) { ran[s] = false; code[s] = 0; vertices[s] = faces[s] = 0u; }
    // `stage` and every stage after it: not run
    void invalidateFrom(int stage) { for (int s = stage; s < VH_FINISH_NUM_STAGES; s++) reset(s); }
    // a stage runs anew: what the stages after it hold is of the mesh before.  Irregular, and kept as it always was: new
    // normals leave the components valid, because the filter keeps its own copy of the normals it was given.
    void start(int stage) { if (stage == VH_FINISH_NORMALS) reset(stage); else invalidateFrom(stage); }
    // a stage is switched off: as its start, if it has run
    void forget(int stage) { if (ran[stage]) start(stage); }
    void finish(int stage, int statusCode, uint32_t numVertices, uint32_t numFaces)
    {
        ran[stage] = true;
        code[stage] = statusCode;
        vertices[stage] = statusCode == 0 ? numVertices : 0u; // (behind a status there is no mesh)
        faces[stage] = statusCode == 0 ? numFaces : 0u;
    }

    // The mesh after `stage` (the input of the stage that follows) is the base taken through the stages up to `stage` that
    // are valid: bit s is set when it takes what stage s made.  The clustering replaces the mesh, the smoothing its
    // vertices -- it never runs over smoothed ones: a smoothing invalidates itself first --, the normals ride along when
    // they are of as many vertices as the mesh has, and the components replace all of it.
    unsigned passes(int stage, uint32_t baseVertices) const
    {
        if (stage >= VH_FINISH_COMPONENTS && valid(VH_FINISH_COMPONENTS)) return 1u << VH_FINISH_COMPONENTS;
        unsigned mask = 0u;
        if (stage >= VH_FINISH_CLUSTER && valid(VH_FINISH_CLUSTER)) mask |= 1u << VH_FINISH_CLUSTER;
        if (stage >= VH_FINISH_SMOOTH && valid(VH_FINISH_SMOOTH)) mask |= 1u << VH_FINISH_SMOOTH;
        const uint32_t numVertices = (mask & 1u << VH_FINISH_CLUSTER) ? vertices[VH_FINISH_CLUSTER] : baseVertices;
        if (stage >= VH_FINISH_NORMALS && valid(VH_FINISH_NORMALS) && vertices[VH_FINISH_NORMALS] == numVertices) mask |= 1u << VH_FINISH_NORMALS;
        return mask;
    }
};

#ifndef VH_MESH_FINISH_STATE_ONLY

#include "vh_host_util.hpp"
#include "vh_mesh_cluster.hpp"
#include "vh_mesh_components.hpp"
#include "vh_mesh_normals.hpp"
#include "vh_mesh_smooth.hpp"

// an indexed mesh on the device; normals (3 floats per vertex) may be null
struct VhMeshView {
    const VhVertex* vertices;
    const uint64_t* keys;
    const uint32_t* faces;
    const float* normals;
    uint32_t numVertices, numFaces;
};

struct VhMeshFinish {
    VhMeshCluster m_cluster;       // the four owners in the pipeline's order; each makes its buffers at its first run
    VhMeshSmooth m_smooth;
    VhMeshNormals m_normals;
    VhMeshComponents m_components;
    VhMeshFinishState state;

    void invalidateFrom(VhFinishStage stage) { state.invalidateFrom(stage); }
    void forget(VhFinishStage stage) { state.forget(stage); }

    // `base` through the valid stages up to `stage` (state.passes)
    VhMeshView after(VhFinishStage stage, VhMeshView m) const
    {
        const unsigned mask = state.passes(stage, m.numVertices);
        if (mask & 1u << VH_FINISH_COMPONENTS)
            return VhMeshView{ m_components.vertices.get(), m_components.keys.get(), m_components.faces.get(), m_components.hasNormals ? m_components.normals.get() : nullptr,
                               state.vertices[VH_FINISH_COMPONENTS], state.faces[VH_FINISH_COMPONENTS] };
        m.normals = nullptr;
        if (mask & 1u << VH_FINISH_CLUSTER)
            m = VhMeshView{ m_cluster.vertices.get(), m_cluster.keys.get(), m_cluster.faces.get(), nullptr, state.vertices[VH_FINISH_CLUSTER], state.faces[VH_FINISH_CLUSTER] };
        if (mask & 1u << VH_FINISH_SMOOTH) m.vertices = m_smooth.vertices.get();
        if (mask & 1u << VH_FINISH_NORMALS) m.normals = m_normals.normals.get();
        return m;
    }

    // The stages.  Each returns what the launches returned and may throw vh::Error (an owner's allocation); a status the
    // pass left is state.code[stage] for the first two, which wait and read their counts (into `counts` too, if given),
    // and is read by normalsStatus / componentsCounts for the other two, which do not wait.
    int cluster(const VhMeshView& base, uint32_t cellsPerCluster, int32_t scaleLog2, vhStream_t stream, uint32_t counts[VH_CLUSTER_NUM_COUNTS] = nullptr)
    {
        uint32_t own[VH_CLUSTER_NUM_COUNTS] = {};
        if (!counts) counts = own;
        state.start(VH_FINISH_CLUSTER);
        VH_TRY(m_cluster.run(base.vertices, base.keys, base.faces, base.numVertices, base.numFaces, cellsPerCluster, scaleLog2, stream));
        const int status = m_cluster.counts(counts, stream);
        state.finish(VH_FINISH_CLUSTER, status, counts[VH_CLUSTER_VERTICES], counts[VH_CLUSTER_FACES]);
        return VH_OK;
    }
    int smooth(const VhMeshView& base, uint32_t iterations, int32_t lambdaQ16, int32_t muQ16, uint32_t keepBoundary, int32_t scaleLog2, vhStream_t stream,
               uint32_t counts[VH_SMOOTH_NUM_COUNTS] = nullptr)
    {
        uint32_t own[VH_SMOOTH_NUM_COUNTS] = {};
        if (!counts) counts = own;
        state.start(VH_FINISH_SMOOTH);
        const VhMeshView m = after(VH_FINISH_CLUSTER, base);
        VH_TRY(m_smooth.run(m.vertices, m.keys, m.faces, m.numVertices, m.numFaces, iterations, lambdaQ16, muQ16, keepBoundary, scaleLog2, stream));
        const int status = m_smooth.counts(counts, stream);
        state.finish(VH_FINISH_SMOOTH, status, m.numVertices, m.numFaces);
        return VH_OK;
    }
    int normals(const VhMeshView& base, int32_t scaleLog2, vhStream_t stream)
    {
        state.start(VH_FINISH_NORMALS);
        const VhMeshView m = after(VH_FINISH_SMOOTH, base);
        VH_TRY(m_normals.run(m.vertices, m.keys, m.faces, m.numVertices, m.numFaces, scaleLog2, stream));
        state.finish(VH_FINISH_NORMALS, 0, m.numVertices, m.numFaces);
        return VH_OK;
    }
    int components(const VhMeshView& base, uint32_t minFaces, uint32_t largestOnly, vhStream_t stream)
    {
        state.start(VH_FINISH_COMPONENTS);
        const VhMeshView m = after(VH_FINISH_NORMALS, base); // the normals it leaves behind a status are zeros, not garbage
        VH_TRY(m_components.run(m.vertices, m.keys, m.normals, m.faces, m.numVertices, m.numFaces, minFaces, largestOnly, stream));
        state.finish(VH_FINISH_COMPONENTS, 0, 0u, 0u); // the kept mesh has no size until componentsCounts has read it
        return VH_OK;
    }
    // waits; VH_ERR_BAD_ARGUMENT when the normals left a status
    int normalsStatus(vhStream_t stream) const { return m_normals.download(nullptr, 0u, true, stream); }
    // waits and reads the filter's six counts; without a status, after(VH_FINISH_COMPONENTS) is then the kept mesh
    int componentsCounts(uint32_t out[VH_COMPONENTS_NUM_COUNTS], vhStream_t stream)
    {
        const int status = m_components.counts(out, stream);
        if (status == VH_OK && state.valid(VH_FINISH_COMPONENTS))
            state.finish(VH_FINISH_COMPONENTS, 0, out[VH_COMPONENTS_KEPT_VERTICES], out[VH_COMPONENTS_KEPT_FACES]);
        return status;
    }

    // a mesh on the device to the host, then the wait; an array that is not asked for is not copied, and normals that
    // are asked for have to be there
    static int download(const VhMeshView& m, VhVertex* vertices, uint64_t* keys, float* normals, uint32_t* faces, vhStream_t stream)
    {
        hipStream_t s = (hipStream_t)stream;
        if (normals && m.numVertices && !m.normals) return VH_ERR_BAD_ARGUMENT;
        if (vertices && m.numVertices) VH_HIP(hipMemcpyAsync(vertices, m.vertices, sizeof(VhVertex) * (size_t)m.numVertices, hipMemcpyDeviceToHost, s));
        if (keys && m.numVertices) VH_HIP(hipMemcpyAsync(keys, m.keys, sizeof(uint64_t) * (size_t)m.numVertices, hipMemcpyDeviceToHost, s));
        if (normals && m.numVertices) VH_HIP(hipMemcpyAsync(normals, m.normals, sizeof(float) * 3 * (size_t)m.numVertices, hipMemcpyDeviceToHost, s));
        if (faces && m.numFaces) VH_HIP(hipMemcpyAsync(faces, m.faces, sizeof(uint32_t) * 3 * (size_t)m.numFaces, hipMemcpyDeviceToHost, s));
        VH_HIP(hipStreamSynchronize(s));
        return VH_OK;
    }
};

// How the extraction class reaches an accumulation's chain and its welded mesh (vh_mesh.hip): not part of the C ABI.
// numVertices and numFaces are the accumulation's counts as vh_mesh_weld_accum_get_counts has just read them.
struct VhMeshWeldAccum;
VhMeshFinish& vh_mesh_weld_accum_finish(VhMeshWeldAccum* accum);
VhMeshView vh_mesh_weld_accum_base(const VhMeshWeldAccum* accum, uint32_t numVertices, uint32_t numFaces);

#endif // VH_MESH_FINISH_STATE_ONLY
