// vh_marching_cubes.cpp -- host side of the iso-surface extraction: CUDAMarchingCubesHashSDF
// (DSC/CUDAMarchingCubesHashSDF.{h,cpp}), MarchingCubesData::allocate/free/copyToCPU
// (DSC/MarchingCubesSDFUtil.h:57-147) and the mesh container the reference takes from mLib (MeshDataf, MeshIOf).
//
// The mesh functions restate the mLib revision the reference vendors (DepthSensingCUDA/Include/mLib/include/
// core-mesh/meshData.{h,cpp}, meshIO.cpp, cited as MLIB/ below).  No reference output exists for them, so they are
// pinned by that source only ("parity unpinned" as far as outputs go).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <unordered_map>
#include <set>

#include "../../include/vh.hpp"
#include "vh_host_util.hpp"
#include "vh_mesh_finish.hpp"

// ---------------------------------------------------------------------------
// launcher-level buffers
// ---------------------------------------------------------------------------

extern "C" {

// MarchingCubesData::allocate (GPU side), DSC/MarchingCubesSDFUtil.h:57-83
int vh_marching_cubes_data_alloc(VhMarchingCubesData* data, const VhMarchingCubesParams* params)
{
    if (!data || !params || params->m_maxNumTriangles == 0) return VH_ERR_BAD_ARGUMENT;
    std::memset(data, 0, sizeof(*data));
    const size_t maxBlocks = (size_t)params->m_hashNumBuckets * params->m_hashBucketSize;
    const int r = [&]() -> int {
        VH_HIP(hipMalloc((void**)&data->d_params, sizeof(VhMarchingCubesParams)));
        VH_HIP(hipMalloc((void**)&data->d_numOccupiedBlocks, sizeof(uint32_t)));
        VH_HIP(hipMalloc((void**)&data->d_occupiedBlocks, sizeof(uint32_t) * (maxBlocks ? maxBlocks : 1)));
        VH_HIP(hipMalloc((void**)&data->d_triangles, sizeof(VhTriangle) * (size_t)params->m_maxNumTriangles));
        VH_HIP(hipMalloc((void**)&data->d_numTriangles, sizeof(uint32_t)));
        VH_HIP(hipMemcpy(data->d_params, params, sizeof(*params), hipMemcpyHostToDevice));
        return VH_OK;
    }();
    if (r != VH_OK) { // (what was allocated before the failure goes back)
        vh_marching_cubes_data_free(data);
        return r;
    }
    data->m_bIsOnGPU = 1;
    return VH_OK;
}

void vh_marching_cubes_data_free(VhMarchingCubesData* data)
{
    if (!data) return;
    if (data->d_params) (void)hipFree(data->d_params);
    if (data->d_numOccupiedBlocks) (void)hipFree(data->d_numOccupiedBlocks);
    if (data->d_occupiedBlocks) (void)hipFree(data->d_occupiedBlocks);
    if (data->d_triangles) (void)hipFree(data->d_triangles);
    if (data->d_numTriangles) (void)hipFree(data->d_numTriangles);
    std::memset(data, 0, sizeof(*data));
}

// MarchingCubesData::updateParams :85-93
int vh_marching_cubes_update_params(const VhMarchingCubesData* data, const VhMarchingCubesParams* params, vhStream_t stream)
{
    if (!data || !data->d_params || !params) return VH_ERR_BAD_ARGUMENT;
    VH_HIP(hipMemcpyAsync(data->d_params, params, sizeof(*params), hipMemcpyHostToDevice, (hipStream_t)stream));
    VH_HIP(hipStreamSynchronize((hipStream_t)stream)); // params is the caller's stack object
    return VH_OK;
}

} // extern "C"

// ---------------------------------------------------------------------------
// vh::MeshData
// ---------------------------------------------------------------------------

void vh::MeshData::makeTriangleSoupIndices()
{
    m_FaceIndicesVertices.resize(m_Vertices.size() / 3 * 3);
    for (size_t i = 0; i < m_FaceIndicesVertices.size(); i++) m_FaceIndicesVertices[i] = (unsigned int)i;
}

namespace {
struct CellKey {
    int x, y, z;
    bool operator==(const CellKey& o) const { return x == o.x && y == o.y && z == o.z; }
};
struct CellHash {
    size_t operator()(const CellKey& k) const
    {
        return ((size_t)(unsigned int)k.x * 73856093u) ^ ((size_t)(unsigned int)k.y * 19349669u) ^ ((size_t)(unsigned int)k.z * 83492791u);
    }
};
inline int signf(float v) { return (0.0f < v) - (v < 0.0f); }
} // namespace

// MLIB/core-mesh/meshData.cpp:216-289 with approx = true (the only mode the reference calls): a vertex goes to the
// cell int(v / thresh + 0.5 sign(v)) (meshData.h:732-734); the 27 cells around it are searched in x-major order and
// the first one that holds a vertex wins (meshData.cpp:197-212, no distance test); otherwise the vertex founds its
// cell.  Faces are re-indexed and those left with a repeated index are dropped (removeDegeneratedFaces :293-318).
void vh::MeshData::mergeCloseVertices(float thresh)
{
    if (thresh <= 0.0f) throw vh::Error(VH_ERR_BAD_ARGUMENT, "mergeCloseVertices: invalid thresh");
    if (m_Vertices.empty()) return;
    std::unordered_map<CellKey, unsigned int, CellHash> grid;
    grid.reserve(2 * m_Vertices.size());
    std::vector<unsigned int> lookUp(m_Vertices.size());
    std::vector<vec3f> verts;
    std::vector<float> cols;
    verts.reserve(m_Vertices.size());
    const bool hasColors = m_Colors.size() == 4 * m_Vertices.size();
    unsigned int cnt = 0;
    for (size_t v = 0; v < m_Vertices.size(); v++) {
        const vec3f& p = m_Vertices[v];
        const CellKey c = { (int)(p.x / thresh + 0.5f * (float)signf(p.x)), (int)(p.y / thresh + 0.5f * (float)signf(p.y)),
                            (int)(p.z / thresh + 0.5f * (float)signf(p.z)) };
        unsigned int nn = (unsigned int)-1;
        for (int i = -1; i <= 1 && nn == (unsigned int)-1; i++)
            for (int j = -1; j <= 1 && nn == (unsigned int)-1; j++)
                for (int k = -1; k <= 1 && nn == (unsigned int)-1; k++) {
                    auto it = grid.find(CellKey{ c.x + i, c.y + j, c.z + k });
                    if (it != grid.end()) nn = it->second;
                }
        if (nn == (unsigned int)-1) {
            grid[c] = cnt;
            verts.push_back(p);
            if (hasColors) cols.insert(cols.end(), m_Colors.begin() + 4 * v, m_Colors.begin() + 4 * v + 4);
            lookUp[v] = cnt++;
        } else {
            lookUp[v] = nn;
        }
    }
    for (auto& f : m_FaceIndicesVertices) f = lookUp[f];
    if (verts.size() != m_Vertices.size()) {
        m_Vertices.swap(verts);
        if (hasColors) m_Colors.swap(cols);
    }
    std::vector<unsigned int> faces;
    faces.reserve(m_FaceIndicesVertices.size());
    for (size_t f = 0; f + 2 < m_FaceIndicesVertices.size(); f += 3) {
        const unsigned int a = m_FaceIndicesVertices[f], b = m_FaceIndicesVertices[f + 1], c = m_FaceIndicesVertices[f + 2];
        if (a == b || b == c || a == c) continue;
        faces.push_back(a); faces.push_back(b); faces.push_back(c);
    }
    m_FaceIndicesVertices.swap(faces);
}

// MLIB/core-mesh/meshData.cpp:36-105: of the faces over one vertex set the first is kept, in its own winding
void vh::MeshData::removeDuplicateFaces()
{
    std::set<std::array<unsigned int, 3>> seen;
    std::vector<unsigned int> faces;
    faces.reserve(m_FaceIndicesVertices.size());
    for (size_t f = 0; f + 2 < m_FaceIndicesVertices.size(); f += 3) {
        std::array<unsigned int, 3> key = { m_FaceIndicesVertices[f], m_FaceIndicesVertices[f + 1], m_FaceIndicesVertices[f + 2] };
        std::sort(key.begin(), key.end());
        if (!seen.insert(key).second) continue;
        faces.push_back(m_FaceIndicesVertices[f]); faces.push_back(m_FaceIndicesVertices[f + 1]); faces.push_back(m_FaceIndicesVertices[f + 2]);
    }
    m_FaceIndicesVertices.swap(faces);
}

// MLIB/core-mesh/meshData.cpp:473-556.  The vendored revision returns without doing anything when *this is empty
// (the assignment is commented out, :479-482), which would leave the reference's offline path with an empty mesh
// for ever; here an empty mesh takes the other one over (fenced reference defects).
void vh::MeshData::merge(const MeshData& other)
{
    if (other.m_Vertices.empty()) return;
    if (m_Vertices.empty()) { *this = other; return; }
    if (hasVertexIndices() != other.hasVertexIndices()) throw vh::Error(VH_ERR_BAD_ARGUMENT, "invalid mesh conversion");
    if (hasNormals() && other.hasNormals()) m_Normals.insert(m_Normals.end(), other.m_Normals.begin(), other.m_Normals.end());
    else m_Normals.clear(); // normals for a part of the vertices are none
    const unsigned int base = (unsigned int)m_Vertices.size();
    m_Vertices.insert(m_Vertices.end(), other.m_Vertices.begin(), other.m_Vertices.end());
    m_Colors.insert(m_Colors.end(), other.m_Colors.begin(), other.m_Colors.end());
    for (unsigned int f : other.m_FaceIndicesVertices) m_FaceIndicesVertices.push_back(base + f);
}

// MLIB/core-mesh/meshData.h:471-479 with Matrix4x4 * point3d = implicit w = 1 and de-homogenisation
// (MLIB/core-math/matrix4x4.h:459-468).  mLib sends normals through the same operator with the inverse transpose, whose
// fourth row holds the translation: it ends up in w, and the normal is divided by it (fenced reference
// defects); here a normal
// goes by the cofactor matrix of the upper-left 3x3 -- det(A) times the inverse transpose of A -- times the sign of the
// determinant, renormalised in double; zero stays zero.  The normal then stays on the side of the surface it was on:
// it turns with a rotation and is mirrored by a mirror.  (The faces keep their index order, so after a mirror the
// winding gives the opposite side: a x b of the transformed edges is cof(A) (a x b), without the sign.)
void vh::MeshData::applyTransform(const mat4f& t)
{
    if (hasNormals()) {
        const double a[3][3] = { { t.m[0], t.m[1], t.m[2] }, { t.m[4], t.m[5], t.m[6] }, { t.m[8], t.m[9], t.m[10] } };
        double c[3][3];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
                c[i][j] = a[i1][j1] * a[i2][j2] - a[i1][j2] * a[i2][j1];
            }
        const double det = a[0][0] * c[0][0] + a[0][1] * c[0][1] + a[0][2] * c[0][2];
        const double sign = det < 0.0 ? -1.0 : 1.0;
        for (size_t v = 0; v < m_Vertices.size(); v++) {
            const double n[3] = { m_Normals[3 * v], m_Normals[3 * v + 1], m_Normals[3 * v + 2] };
            double r[3];
            for (int i = 0; i < 3; i++) r[i] = sign * (c[i][0] * n[0] + c[i][1] * n[1] + c[i][2] * n[2]);
            const double l = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
            for (int i = 0; i < 3; i++) m_Normals[3 * v + i] = l > 0.0 ? (float)(r[i] / l) : 0.0f;
        }
    }
    for (auto& v : m_Vertices) {
        const float x = t.m[0] * v.x + t.m[1] * v.y + t.m[2] * v.z + t.m[3];
        const float y = t.m[4] * v.x + t.m[5] * v.y + t.m[6] * v.z + t.m[7];
        const float z = t.m[8] * v.x + t.m[9] * v.y + t.m[10] * v.z + t.m[11];
        const float w = t.m[12] * v.x + t.m[13] * v.y + t.m[14] * v.z + t.m[15];
        v = { x / w, y / w, z / w };
    }
}

// MeshIO::saveToPLY, MLIB/core-mesh/meshIO.cpp:485-556
void vh::MeshData::saveToPLY(const std::string& filename) const
{
    std::ofstream f(filename, std::ios::binary);
    if (!f) throw vh::Error(VH_ERR_IO, "cannot write " + filename);
    const bool hasColors = m_Colors.size() == 4 * m_Vertices.size(), withNormals = hasNormals();
    const size_t nFaces = hasVertexIndices() ? m_FaceIndicesVertices.size() / 3 : m_Vertices.size() / 3;
    f << "ply\nformat binary_little_endian 1.0\ncomment MLIB generated\nelement vertex " << m_Vertices.size() << "\nproperty float x\nproperty float y\nproperty float z\n";
    if (withNormals) f << "property float nx\nproperty float ny\nproperty float nz\n"; // meshIO.cpp:499-503
    if (hasColors) f << "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n";
    f << "element face " << nFaces << "\nproperty list uchar int vertex_indices\nend_header\n";
    for (size_t i = 0; i < m_Vertices.size(); i++) {
        f.write((const char*)&m_Vertices[i], 12);
        if (withNormals) f.write((const char*)&m_Normals[3 * i], 12); // meshIO.cpp:527-538
        if (hasColors) {
            unsigned char c[4];
            for (int k = 0; k < 4; k++) c[k] = (unsigned char)(int)std::min(255.0f, std::max(0.0f, m_Colors[4 * i + k] * 255)); // vec4uc(c * 255)
            f.write((const char*)c, 4);
        }
    }
    for (size_t i = 0; i < nFaces; i++) {
        const unsigned char three = 3;
        int idx[3];
        for (int k = 0; k < 3; k++) idx[k] = hasVertexIndices() ? (int)m_FaceIndicesVertices[3 * i + k] : (int)(3 * i + k);
        f.write((const char*)&three, 1);
        f.write((const char*)idx, 12);
    }
    if (!f) throw vh::Error(VH_ERR_IO, "write failed: " + filename);
}

// ---------------------------------------------------------------------------
// CUDAMarchingCubesHashSDF
// ---------------------------------------------------------------------------

MarchingCubesParams CUDAMarchingCubesHashSDF::parameters(unsigned int marchingCubesMaxNumTriangles, float SDFMarchingCubeThreshFactor,
                                                         float SDFVoxelSize, unsigned int hashNumBuckets)
{
    MarchingCubesParams p;
    std::memset(&p, 0, sizeof(p));
    p.m_maxNumTriangles = marchingCubesMaxNumTriangles;
    p.m_threshMarchingCubes = SDFMarchingCubeThreshFactor * SDFVoxelSize;
    p.m_threshMarchingCubes2 = SDFMarchingCubeThreshFactor * SDFVoxelSize;
    p.m_sdfBlockSize = VH_SDF_BLOCK_SIZE;
    p.m_hashBucketSize = VH_HASH_BUCKET_SIZE;
    p.m_hashNumBuckets = hashNumBuckets;
    return p;
}

CUDAMarchingCubesHashSDF::CUDAMarchingCubesHashSDF(const MarchingCubesParams& params, vhStream_t stream)
    : m_params(params), m_stream(stream), m_offline(false)
{
    std::memset(&m_data, 0, sizeof(m_data));
    std::memset(&m_weld, 0, sizeof(m_weld));
    std::memset(&m_liveData, 0, sizeof(m_liveData));
    check(vh_marching_cubes_data_alloc(&m_data, &m_params), "MarchingCubesData::allocate");
    m_dataOwner.reset(&m_data);
    check(vh_reset_marching_cubes(&m_data, m_stream), "resetMarchingCubesCUDA");
}

CUDAMarchingCubesHashSDF::~CUDAMarchingCubesHashSDF() { (void)hipStreamSynchronize((hipStream_t)m_stream); }
void CUDAMarchingCubesHashSDF::DataFree::operator()(MarchingCubesData* d) const noexcept { vh_marching_cubes_data_free(d); }
void CUDAMarchingCubesHashSDF::WeldFree::operator()(VhMeshWeldData* d) const noexcept { vh_mesh_weld_data_free(d); }
void CUDAMarchingCubesHashSDF::LiveFree::operator()(VhLiveMeshData* d) const noexcept { vh_live_mesh_data_free(d); }

unsigned int CUDAMarchingCubesHashSDF::getNumTriangles()
{
    unsigned int n = 0;
    checkHip(hipMemcpyAsync(&n, m_data.d_numTriangles, sizeof(n), hipMemcpyDeviceToHost, (hipStream_t)m_stream), "numTriangles");
    checkHip(hipStreamSynchronize((hipStream_t)m_stream), "numTriangles");
    return n;
}

unsigned int CUDAMarchingCubesHashSDF::getNumOccupiedBlocks()
{
    unsigned int n = 0;
    checkHip(hipMemcpyAsync(&n, m_data.d_numOccupiedBlocks, sizeof(n), hipMemcpyDeviceToHost, (hipStream_t)m_stream), "numOccupiedBlocks");
    checkHip(hipStreamSynchronize((hipStream_t)m_stream), "numOccupiedBlocks");
    return n;
}

void CUDAMarchingCubesHashSDF::downloadTriangles(VhTriangle* out, unsigned int n)
{
    if (n == 0) return;
    if (!out || n > m_params.m_maxNumTriangles) throw vh::Error(VH_ERR_BAD_ARGUMENT, "downloadTriangles");
    checkHip(hipMemcpyAsync(out, m_data.d_triangles, sizeof(VhTriangle) * (size_t)n, hipMemcpyDeviceToHost, (hipStream_t)m_stream), "triangles");
    checkHip(hipStreamSynchronize((hipStream_t)m_stream), "triangles");
}

// reset, the box, pass 1, pass 2 (.cpp:194-224) -- or the sourced pass 2, which says where every vertex came from
void CUDAMarchingCubesHashSDF::runPasses(const HashData& hashData, const HashParams& hashParams, const vh::vec3f& minCorner, const vh::vec3f& maxCorner,
                                         bool boxEnabled, bool sourced)
{
    if (sourced && !d_sources) d_sources = vh::deviceAlloc<VhTriangleSource>(m_params.m_maxNumTriangles, "triangle sources");
    check(vh_reset_marching_cubes(&m_data, m_stream), "resetMarchingCubesCUDA");
    m_params.m_maxCorner[0] = maxCorner.x; m_params.m_maxCorner[1] = maxCorner.y; m_params.m_maxCorner[2] = maxCorner.z;
    m_params.m_minCorner[0] = minCorner.x; m_params.m_minCorner[1] = minCorner.y; m_params.m_minCorner[2] = minCorner.z;
    m_params.m_boxEnabled = boxEnabled ? 1u : 0u;
    check(vh_marching_cubes_update_params(&m_data, &m_params, m_stream), "MarchingCubesData::updateParams");
    check(vh_extract_iso_surface_pass1(&hashData, &hashParams, &m_data, m_stream), "extractIsoSurfacePass1CUDA");
    if (sourced)
        check(vh_extract_iso_surface_pass2_sourced(&hashData, &hashParams, &m_data, d_sources.get(), getNumOccupiedBlocks(), m_stream),
              "extractIsoSurfacePass2CUDA (sourced)");
    else
        check(vh_extract_iso_surface_pass2(&hashData, &hashParams, &m_data, getNumOccupiedBlocks(), m_stream), "extractIsoSurfacePass2CUDA");
}

// the overflow test of copyTrianglesToCPU (.cpp:35-38); after a sourced pass 2 the records in the buffer are counted first
unsigned int CUDAMarchingCubesHashSDF::countTriangles(bool sourced)
{
    const unsigned int nTriangles = getNumTriangles();
    if (sourced) m_indexed.numSourced = std::min(nTriangles, m_params.m_maxNumTriangles);
    if (nTriangles >= m_params.m_maxNumTriangles)
        throw vh::Error(VH_ERR_STAGING_OVERFLOW, "not enough memory to store triangles for chunk; increase s_marchingCubesMaxNumTriangles");
    return nTriangles;
}

void CUDAMarchingCubesHashSDF::extractIsoSurfaceWithoutCopy(const HashData& hashData, const HashParams& hashParams, const vh::vec3f& minCorner,
                                                            const vh::vec3f& maxCorner, bool boxEnabled)
{
    refuseWhileLive("extractIsoSurface");
    runPasses(hashData, hashParams, minCorner, maxCorner, boxEnabled, false);
}

void CUDAMarchingCubesHashSDF::extractIsoSurface(const HashData& hashData, const HashParams& hashParams, const vh::vec3f& minCorner,
                                                 const vh::vec3f& maxCorner, bool boxEnabled)
{
    extractIsoSurfaceWithoutCopy(hashData, hashParams, minCorner, maxCorner, boxEnabled);
    copyTrianglesToCPU();
}

namespace {
// a weld's get_counts code as the exception the indexed extractions throw
void checkWeld(int rc, const char* what)
{
    if (rc == VH_ERR_STAGING_OVERFLOW) throw vh::Error(rc, "mesh weld: the table is full");
    if (rc == VH_ERR_BAD_ARGUMENT) throw vh::Error(rc, "mesh weld: a voxel coordinate is outside the key range of +-2^19");
    check(rc, what);
}

// What a stage of the finish left as the exception the indexed extractions throw: a launch that failed, or the status the
// pass wrote (a text of null: that code has none of its own)
struct StageTexts { const char* launch; const char* pass; const char* overflow; const char* badArgument; };
const StageTexts kStageTexts[VH_FINISH_NUM_STAGES] = {
    { "vh_mesh_cluster", "mesh clustering", "mesh clustering: a table is full",
      "mesh clustering: a key that is no vertex key, a value out of the fixed-point range, or a face index out of bounds" },
    { "vh_mesh_smooth", "mesh smoothing", "mesh smoothing: the edge table is full",
      "mesh smoothing: a value out of the fixed-point range, a face index out of bounds, or a vertex of more than 65536 neighbours" },
    { "vh_mesh_vertex_normals", "vertex normals", nullptr, "vertex normals: a face normal is out of the fixed-point range, or a face index out of bounds" },
    { "vh_mesh_components", "mesh components", nullptr, "mesh components: a face index out of bounds" },
};
void checkStage(VhFinishStage stage, int launched, int status)
{
    const StageTexts& t = kStageTexts[stage];
    check(launched, t.launch);
    if (status == VH_ERR_STAGING_OVERFLOW && t.overflow) throw vh::Error(status, t.overflow);
    if (status == VH_ERR_BAD_ARGUMENT && t.badArgument) throw vh::Error(status, t.badArgument);
    check(status, t.pass);
}

// n vertex records as the mesh container has them: positions, and rgb with alpha 1
void recordsToMeshData(const VhVertex* v, size_t n, vh::MeshData& md)
{
    md.m_Vertices.resize(n);
    md.m_Colors.resize(4 * n);
    for (size_t i = 0; i < n; i++) {
        md.m_Vertices[i] = { v[i].p[0], v[i].p[1], v[i].p[2] };
        md.m_Colors[4 * i + 0] = v[i].c[0]; md.m_Colors[4 * i + 1] = v[i].c[1]; md.m_Colors[4 * i + 2] = v[i].c[2]; md.m_Colors[4 * i + 3] = 1.0f;
    }
}
} // namespace

void CUDAMarchingCubesHashSDF::setIndexedClustering(unsigned int cellsPerCluster)
{
    if (cellsPerCluster > VH_CLUSTER_MAX_CELLS) throw vh::Error(VH_ERR_BAD_ARGUMENT, "setIndexedClustering: at most 64 cells per cluster");
    m_clusterCells = cellsPerCluster;
}

void CUDAMarchingCubesHashSDF::setIndexedSmoothing(unsigned int iterations, float lambda, float mu, bool keepBoundary)
{
    if (iterations > VH_SMOOTH_MAX_ITERATIONS) throw vh::Error(VH_ERR_BAD_ARGUMENT, "setIndexedSmoothing: at most 100 iterations");
    if (!(std::fabs(lambda) <= 1.0f) || !(std::fabs(mu) <= 1.0f)) throw vh::Error(VH_ERR_BAD_ARGUMENT, "setIndexedSmoothing: factors in [-1, 1]");
    setIndexedSmoothingQ16(iterations, (int32_t)std::rint((double)lambda * 65536.0), (int32_t)std::rint((double)mu * 65536.0), keepBoundary);
}

void CUDAMarchingCubesHashSDF::setIndexedSmoothingQ16(unsigned int iterations, int32_t lambdaQ16, int32_t muQ16, bool keepBoundary)
{
    if (iterations > VH_SMOOTH_MAX_ITERATIONS) throw vh::Error(VH_ERR_BAD_ARGUMENT, "setIndexedSmoothing: at most 100 iterations");
    if (lambdaQ16 < -VH_SMOOTH_MAX_FACTOR_Q16 || lambdaQ16 > VH_SMOOTH_MAX_FACTOR_Q16 || muQ16 < -VH_SMOOTH_MAX_FACTOR_Q16 || muQ16 > VH_SMOOTH_MAX_FACTOR_Q16)
        throw vh::Error(VH_ERR_BAD_ARGUMENT, "setIndexedSmoothing: factors in [-1, 1]");
    m_smoothIterations = iterations; m_smoothLambdaQ16 = lambdaQ16; m_smoothMuQ16 = muQ16; m_smoothKeepBoundary = keepBoundary;
}

// the chain of the last indexed extraction, and the welded mesh it runs over
VhMeshFinish& CUDAMarchingCubesHashSDF::indexedChain(bool accumulated)
{
    if (accumulated) return vh_mesh_weld_accum_finish(m_accum.get());
    if (!m_finish) m_finish.reset(new VhMeshFinish);
    return *m_finish;
}

VhMeshView CUDAMarchingCubesHashSDF::indexedBase(bool accumulated, unsigned int nv, unsigned int nf) const
{
    if (accumulated) return vh_mesh_weld_accum_base(m_accum.get(), nv, nf);
    return VhMeshView{ m_weld.d_vertices, m_weld.d_keys, m_weld.d_faces, nullptr, nv, nf };
}

void CUDAMarchingCubesHashSDF::readBackIndexed(unsigned int nv, unsigned int nf, bool accumulated, float voxelSize)
{
    const bool filter = m_componentMinFaces != 0 || m_componentLargestOnly, cluster = m_clusterCells != 0, smooth = m_smoothIterations != 0;
    // (an accumulation without an append has no voxel size, and no vertex either: any scale serves)
    const bool sized = voxelSize > 0.0f || !accumulated;
    VhMeshFinish& chain = indexedChain(accumulated);
    const VhMeshView base = indexedBase(accumulated, nv, nf);
    // A stage that is off is forgotten -- a finish of these appends with it on may have gone before --, so that the mesh
    // after the last stage is the mesh of THIS finish.  The welded mesh stays where it is.
    unsigned int clusterStats[VH_CLUSTER_NUM_COUNTS] = { 0, 0, 0, 0, 0, 0 }, smoothStats[VH_SMOOTH_NUM_COUNTS] = { 0, 0, 0, 0, 0, 0 };
    int32_t meshScale = 0; // of the clustering, and of the smoothing over the mesh as it then stands
    if ((cluster || smooth) && sized) check(vh_mesh_cluster_default_scale_log2(voxelSize, &meshScale), "vh_mesh_cluster_default_scale_log2");
    if (cluster) { // a cluster spans chunks: a pass of the finish
        const int launched = chain.cluster(base, m_clusterCells, meshScale, m_stream, clusterStats);
        checkStage(VH_FINISH_CLUSTER, launched, chain.state.code[VH_FINISH_CLUSTER]);
    } else chain.forget(VH_FINISH_CLUSTER);
    if (smooth) { // and so do a vertex's neighbours
        const int launched = chain.smooth(base, m_smoothIterations, m_smoothLambdaQ16, m_smoothMuQ16, m_smoothKeepBoundary ? 1u : 0u, meshScale, m_stream, smoothStats);
        checkStage(VH_FINISH_SMOOTH, launched, chain.state.code[VH_FINISH_SMOOTH]);
    } else chain.forget(VH_FINISH_SMOOTH);
    if (m_indexedNormals) {
        // the vertices of a welded face lie in adjacent clusters and inside their clusters' boxes: an edge of a clustered
        // face stays under 2 m voxels in every component, and the normals' scale is that of a voxel of 2 m voxelSize.
        // Smoothing can lengthen an edge: twice that bound again, which is a margin and not a proof (VH_NORMALS_RANGE says so)
        int32_t scaleLog2 = 0;
        if (sized)
            check(vh_mesh_normals_default_scale_log2((smooth ? 2.0f : 1.0f) * (cluster ? 2.0f * (float)m_clusterCells * voxelSize : voxelSize), &scaleLog2),
                  "vh_mesh_normals_default_scale_log2");
        // over all the faces, with the bits the last append left: a pass of the finish, never of an append.  Only its
        // status comes back here: the normals come with the mesh
        const int launched = chain.normals(base, scaleLog2, m_stream);
        checkStage(VH_FINISH_NORMALS, launched, launched == VH_OK ? chain.normalsStatus(m_stream) : VH_OK);
    } else chain.forget(VH_FINISH_NORMALS);
    unsigned int stats[VH_COMPONENTS_NUM_COUNTS] = { 0, 0, 0, 0, 0, 0 };
    if (filter) { // a component spans chunks
        const int launched = chain.components(base, m_componentMinFaces, m_componentLargestOnly ? 1u : 0u, m_stream);
        checkStage(VH_FINISH_COMPONENTS, launched, launched == VH_OK ? chain.componentsCounts(stats, m_stream) : VH_OK);
    } else chain.forget(VH_FINISH_COMPONENTS);
    const VhMeshView mesh = chain.after(VH_FINISH_COMPONENTS, base); // the mesh that goes to the host
    vh::MeshData md;
    std::vector<VhVertex> verts(mesh.numVertices);
    md.m_FaceIndicesVertices.resize(3 * (size_t)mesh.numFaces);
    if (m_indexedNormals) md.m_Normals.resize(3 * (size_t)mesh.numVertices);
    check(VhMeshFinish::download(mesh, verts.data(), nullptr, m_indexedNormals ? md.m_Normals.data() : nullptr, md.m_FaceIndicesVertices.data(), m_stream), "indexed mesh download");
    recordsToMeshData(verts.data(), verts.size(), md);
    m_meshData = std::move(md);
    m_indexed.counts[0] = nv; m_indexed.counts[1] = nf;
    m_indexed.clustered = cluster;
    std::copy(clusterStats, clusterStats + VH_CLUSTER_NUM_COUNTS, m_indexed.clusterStats);
    m_indexed.smoothed = smooth;
    std::copy(smoothStats, smoothStats + VH_SMOOTH_NUM_COUNTS, m_indexed.smoothStats);
    m_indexed.hasNormals = m_indexedNormals;
    m_indexed.filtered = filter;
    m_indexed.kept[0] = mesh.numVertices; m_indexed.kept[1] = mesh.numFaces;
    std::copy(stats, stats + VH_COMPONENTS_NUM_COUNTS, m_indexed.componentStats);
    m_welded = true;
}

// Not in the reference.  The soup stays on the device; what comes back is the welded mesh.
void CUDAMarchingCubesHashSDF::extractIsoSurfaceIndexed(const HashData& hashData, const HashParams& hashParams, const vh::vec3f& minCorner,
                                                        const vh::vec3f& maxCorner, bool boxEnabled)
{
    refuseWhileLive("extractIsoSurfaceIndexed");
    resetIndexed(); // nothing partial is left behind by an error
    runPasses(hashData, hashParams, minCorner, maxCorner, boxEnabled, true);
    weldAndReadBack(countTriangles(true), hashParams.m_virtualVoxelSize);
}

void CUDAMarchingCubesHashSDF::weldAndReadBack(unsigned int nTriangles, float voxelSize)
{
    // the table is sized by the triangles there are, not by the buffer: it grows, and is kept for the next call
    if (!m_weldOwner || m_weld.m_maxTriangles < nTriangles) {
        m_weldOwner.reset();
        check(vh_mesh_weld_data_alloc(&m_weld, nTriangles + nTriangles / 4u, 0), "vh_mesh_weld_data_alloc");
        m_weldOwner.reset(&m_weld);
    }
    indexedChain(false).invalidateFrom(VH_FINISH_CLUSTER); // a new weld: what the stages made of the last one is stale
    check(vh_mesh_weld(m_data.d_triangles, d_sources.get(), nTriangles, &m_weld, 0, m_stream), "vh_mesh_weld");
    unsigned int counts[3] = { 0, 0, 0 };
    const int rc = vh_mesh_weld_get_counts(&m_weld, counts, m_stream);
    m_indexed.counts[2] = counts[2];
    checkWeld(rc, "vh_mesh_weld_get_counts");
    readBackIndexed(counts[0], counts[1], false, voxelSize);
}

// ---------------------------------------------------------------------------
// live mesh
// ---------------------------------------------------------------------------

void CUDAMarchingCubesHashSDF::refuseWhileLive(const char* what) const
{
    if (m_live) throw vh::Error(VH_ERR_BAD_ARGUMENT, std::string(what) + ": the object holds a live mesh (liveEnd first)");
}

void CUDAMarchingCubesHashSDF::liveBegin()
{
    refuseWhileLive("liveBegin");
    if (!d_sources) d_sources = vh::deviceAlloc<VhTriangleSource>(m_params.m_maxNumTriangles, "triangle sources");
    resetIndexed();
    m_params.m_boxEnabled = 0u;
    check(vh_marching_cubes_update_params(&m_data, &m_params, m_stream), "MarchingCubesData::updateParams");
    check(vh_reset_marching_cubes(&m_data, m_stream), "resetMarchingCubesCUDA");
    if (m_liveOwner) check(vh_live_mesh_reset(&m_liveData, m_stream), "vh_live_mesh_reset");
    m_live = true;
    m_liveValid = false;
}

void CUDAMarchingCubesHashSDF::liveUpdate(const HashData& hashData, const HashParams& hashParams, unsigned int counts[VH_LIVE_NUM_COUNTS + 1], bool boxEnabled)
{
    if (!m_live) throw vh::Error(VH_ERR_BAD_ARGUMENT, "liveUpdate: no liveBegin");
    if (boxEnabled) throw vh::Error(VH_ERR_BAD_ARGUMENT, "liveUpdate: a live mesh has no box");
    if (m_liveOwner && m_liveData.m_numSDFBlocks != hashParams.m_numSDFBlocks) {
        if (!m_liveData.m_fresh) throw vh::Error(VH_ERR_BAD_ARGUMENT, "liveUpdate: the hash parameters are not those of the earlier updates");
        m_liveOwner.reset();
    }
    if (!m_liveOwner) { // the records are sized by the pool, which only the hash parameters name
        check(vh_live_mesh_data_alloc(&m_liveData, hashParams.m_numSDFBlocks, m_params.m_maxNumTriangles), "vh_live_mesh_data_alloc");
        m_liveOwner.reset(&m_liveData);
    }
    VhTriangleSource* sources = d_sources.get();
    const int rc = vh_live_mesh_update(&hashData, &hashParams, &m_data, &sources, &m_liveData, m_stream);
    if (sources != d_sources.get()) { (void)d_sources.release(); d_sources.reset(sources); } // the cache changed places with the spare pair
    if (rc == VH_ERR_BAD_ARGUMENT) throw vh::Error(rc, "liveUpdate: the hash parameters are not those of the earlier updates");
    m_liveValid = false;
    check(rc, "vh_live_mesh_update");
    unsigned int stats[VH_LIVE_NUM_COUNTS + 1] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    const int st = vh_live_mesh_get_counts(&m_liveData, stats, m_stream);
    if (counts) std::copy(stats, stats + VH_LIVE_NUM_COUNTS + 1, counts);
    if (st == VH_ERR_STAGING_OVERFLOW) throw vh::Error(st, "live mesh: not enough memory to store the triangles; increase s_marchingCubesMaxNumTriangles");
    if (st == VH_ERR_BAD_ARGUMENT) throw vh::Error(st, "live mesh: a block outside the range of +-2^16, or a table that names a block twice or none of the pool");
    check(st, "vh_live_mesh_get_counts");
    m_liveVoxelSize = hashParams.m_virtualVoxelSize;
    m_liveValid = true;
}

void CUDAMarchingCubesHashSDF::liveInvalidate()
{
    if (!m_live) throw vh::Error(VH_ERR_BAD_ARGUMENT, "liveInvalidate: no liveBegin");
    if (m_liveOwner) check(vh_live_mesh_reset(&m_liveData, m_stream), "vh_live_mesh_reset");
    check(vh_reset_marching_cubes(&m_data, m_stream), "resetMarchingCubesCUDA");
    m_liveValid = false;
}

void CUDAMarchingCubesHashSDF::liveIndexed()
{
    if (!m_live || !m_liveValid) throw vh::Error(VH_ERR_BAD_ARGUMENT, "liveIndexed: no valid live mesh (liveBegin, liveUpdate)");
    resetIndexed();
    const unsigned int nTriangles = getNumTriangles(); // the cache's count: within the buffer after an update without a status
    m_indexed.numSourced = nTriangles;
    weldAndReadBack(nTriangles, m_liveVoxelSize);
}

void CUDAMarchingCubesHashSDF::liveEnd()
{
    if (!m_live) throw vh::Error(VH_ERR_BAD_ARGUMENT, "liveEnd: no liveBegin");
    m_live = false;
    m_liveValid = false;
    check(vh_reset_marching_cubes(&m_data, m_stream), "resetMarchingCubesCUDA");
}

void CUDAMarchingCubesHashSDF::AccumFree::operator()(VhMeshWeldAccum* a) const noexcept { vh_mesh_weld_accum_destroy(a); }

void CUDAMarchingCubesHashSDF::beginIndexed()
{
    refuseWhileLive("beginIndexed");
    resetIndexed();
    m_indexed.accumulated = true;
    if (!m_accum) {
        VhMeshWeldAccum* a = nullptr;
        check(vh_mesh_weld_accum_create(0, 0, 0, &a), "vh_mesh_weld_accum_create");
        m_accum.reset(a);
    }
    check(vh_mesh_weld_accum_begin(m_accum.get(), m_stream), "vh_mesh_weld_accum_begin");
}

void CUDAMarchingCubesHashSDF::appendIndexed(const HashData& hashData, const HashParams& hashParams, const vh::vec3f& minCorner,
                                             const vh::vec3f& maxCorner, bool boxEnabled)
{
    refuseWhileLive("appendIndexed");
    if (!m_accum || !m_indexed.accumulated) throw vh::Error(VH_ERR_BAD_ARGUMENT, "appendIndexed: no beginIndexed");
    m_indexed.voxelSize = hashParams.m_virtualVoxelSize;
    try {
        runPasses(hashData, hashParams, minCorner, maxCorner, boxEnabled, true);
        const unsigned int nTriangles = countTriangles(true);
        check(vh_mesh_weld_accum_append(m_accum.get(), m_data.d_triangles, d_sources.get(), nTriangles, m_stream), "vh_mesh_weld_accum_append");
    } catch (...) {
        // the accumulation is over: finishIndexed wants a new beginIndexed.  The records in the buffer stay readable.
        const unsigned int sourced = m_indexed.numSourced;
        resetIndexed();
        m_indexed.numSourced = sourced;
        throw;
    }
}

void CUDAMarchingCubesHashSDF::finishIndexed()
{
    if (!m_accum || !m_indexed.accumulated) throw vh::Error(VH_ERR_BAD_ARGUMENT, "finishIndexed: no beginIndexed");
    clearMeshBuffer();
    unsigned int stats[VH_WELD_ACCUM_NUM_COUNTS] = { 0, 0, 0, 0, 0, 0 };
    const int rc = vh_mesh_weld_accum_get_counts(m_accum.get(), stats, m_stream);
    for (unsigned int& c : m_indexed.counts) c = 0;
    m_indexed.counts[VH_WELD_ACCUM_STATUS] = stats[VH_WELD_ACCUM_STATUS];
    m_indexed.hasNormals = false;
    m_indexed.filtered = false;
    m_indexed.clustered = false;
    m_indexed.smoothed = false;
    checkWeld(rc, "vh_mesh_weld_accum_get_counts");
    readBackIndexed(stats[VH_WELD_ACCUM_VERTICES], stats[VH_WELD_ACCUM_FACES], true, m_indexed.voxelSize);
    std::copy(stats, stats + VH_WELD_ACCUM_NUM_COUNTS, m_indexed.counts);
}

// .cpp:149-192; the box of a chunk is padded by one block
template <class F>
void CUDAMarchingCubesHashSDF::walkChunks(CUDASceneRepChunkGrid& chunkGrid, const vh::vec3f& camPos, float radius, bool restoreOnError, F&& perChunk)
{
    chunkGrid.stopMultiThreading();
    const vh::vec3i minGridPos = chunkGrid.getMinGridPos(), maxGridPos = chunkGrid.getMaxGridPos();
    unsigned int nStreamedBlocks = 0;
    bool walking = false;
    try {
        chunkGrid.streamOutToCPUAll();
        walking = true;
        for (int x = minGridPos.x; x < maxGridPos.x; x++)
            for (int y = minGridPos.y; y < maxGridPos.y; y++)
                for (int z = minGridPos.z; z < maxGridPos.z; z++) {
                    const vh::vec3i chunk = { x, y, z };
                    if (!chunkGrid.containsSDFBlocksChunk(chunk)) continue;
                    chunkGrid.streamInToGPUChunkNeighborhood(chunk, 1);
                    const vh::vec3f c = chunkGrid.getWorldPosChunk(chunk), e = chunkGrid.getVoxelExtends();
                    const HashParams hp = chunkGrid.getHashParams();
                    const float pad = hp.m_virtualVoxelSize * (float)hp.m_SDFBlockSize;
                    const vh::vec3f minCorner = { c.x - e.x / 2.0f - pad, c.y - e.y / 2.0f - pad, c.z - e.z / 2.0f - pad };
                    const vh::vec3f maxCorner = { c.x + e.x / 2.0f + pad, c.y + e.y / 2.0f + pad, c.z + e.z / 2.0f + pad };
                    perChunk(chunkGrid.getHashData(), hp, minCorner, maxCorner);
                    chunkGrid.streamOutToCPUAll();
                }
        walking = false;
        chunkGrid.streamInToGPUAll(camPos, radius, true, nStreamedBlocks);
    } catch (...) {
        if (!restoreOnError) throw; // the reference's walk leaves the scene where the error found it
        if (walking) { // a chunk failed with its neighbourhood on the device
            chunkGrid.streamOutToCPUAll();
            chunkGrid.streamInToGPUAll(camPos, radius, true, nStreamedBlocks);
        }
        chunkGrid.startMultiThreading();
        throw;
    }
    chunkGrid.startMultiThreading();
}

void CUDAMarchingCubesHashSDF::extractIsoSurface(CUDASceneRepChunkGrid& chunkGrid, const vh::vec3f& camPos, float radius)
{
    refuseWhileLive("extractIsoSurface");
    clearMeshBuffer();
    walkChunks(chunkGrid, camPos, radius, false, [this](const HashData& hd, const HashParams& hp, const vh::vec3f& lo, const vh::vec3f& hi) {
        extractIsoSurface(hd, hp, lo, hi, true);
    });
}

// the same walk, every chunk appended to one accumulation
void CUDAMarchingCubesHashSDF::extractIsoSurfaceIndexed(CUDASceneRepChunkGrid& chunkGrid, const vh::vec3f& camPos, float radius)
{
    refuseWhileLive("extractIsoSurfaceIndexed");
    try {
        beginIndexed();
        walkChunks(chunkGrid, camPos, radius, true, [this](const HashData& hd, const HashParams& hp, const vh::vec3f& lo, const vh::vec3f& hi) {
            appendIndexed(hd, hp, lo, hi, true);
        });
        finishIndexed();
    } catch (...) {
        resetIndexed(); // the one reset of the walk: also of the records' count, which a failed appendIndexed alone keeps
        throw;
    }
}

// The device mesh of the last indexed extraction, of the size getIndexedCounts reports: its welded mesh through its chain,
// which has to stand as that extraction left it (an appendIndexed after the finishIndexed makes every stage stale).
VhMeshView CUDAMarchingCubesHashSDF::indexedView(const char* what)
{
    unsigned int n[3];
    getIndexedCounts(n);
    if (n[0] == 0 && n[1] == 0) return VhMeshView{ nullptr, nullptr, nullptr, nullptr, 0u, 0u };
    if (!m_indexed.accumulated && !m_weldOwner) throw vh::Error(VH_ERR_BAD_ARGUMENT, std::string(what) + ": no indexed extraction");
    const VhMeshFinish& chain = indexedChain(m_indexed.accumulated);
    const VhMeshView m = chain.after(VH_FINISH_COMPONENTS, indexedBase(m_indexed.accumulated, m_indexed.counts[0], m_indexed.counts[1]));
    const unsigned ran = m_indexed.filtered ? 1u << VH_FINISH_COMPONENTS
                                            : (m_indexed.clustered ? 1u << VH_FINISH_CLUSTER : 0u) | (m_indexed.smoothed ? 1u << VH_FINISH_SMOOTH : 0u) |
                                                  (m_indexed.hasNormals ? 1u << VH_FINISH_NORMALS : 0u);
    if (chain.state.passes(VH_FINISH_COMPONENTS, m_indexed.counts[0]) != ran || m.numVertices != n[0] || m.numFaces != n[1])
        throw vh::Error(VH_ERR_BAD_ARGUMENT, std::string(what) + ": the mesh of the last indexed extraction is no longer on the device");
    return m;
}

void CUDAMarchingCubesHashSDF::downloadIndexed(VhVertex* vertices, uint64_t* keys, uint32_t* faces)
{
    const VhMeshView m = indexedView("downloadIndexed");
    if (m.numVertices == 0 && m.numFaces == 0) return;
    check(VhMeshFinish::download(m, vertices, keys, nullptr, faces, m_stream), "downloadIndexed");
}

void CUDAMarchingCubesHashSDF::downloadIndexedNormals(float* normals)
{
    if (!m_indexed.hasNormals) throw vh::Error(VH_ERR_BAD_ARGUMENT, "downloadIndexedNormals: the last indexed extraction computed none (setIndexedNormals)");
    const VhMeshView m = indexedView("downloadIndexedNormals");
    if (m.numVertices == 0) return;
    if (!normals) throw vh::Error(VH_ERR_BAD_ARGUMENT, "downloadIndexedNormals");
    check(VhMeshFinish::download(m, nullptr, nullptr, normals, nullptr, m_stream), "downloadIndexedNormals");
}

void CUDAMarchingCubesHashSDF::downloadSources(VhTriangleSource* out, unsigned int n)
{
    if (n == 0) return;
    // (while live the records are the cache's: as many as it holds triangles)
    const unsigned int have = m_live ? std::min(getNumTriangles(), m_params.m_maxNumTriangles) : m_indexed.numSourced;
    if (!out || !d_sources || n > have) throw vh::Error(VH_ERR_BAD_ARGUMENT, "downloadSources");
    checkHip(hipMemcpyAsync(out, d_sources.get(), sizeof(VhTriangleSource) * (size_t)n, hipMemcpyDeviceToHost, (hipStream_t)m_stream), "sources");
    checkHip(hipStreamSynchronize((hipStream_t)m_stream), "sources");
}

// .cpp:31-86
void CUDAMarchingCubesHashSDF::copyTrianglesToCPU()
{
    const unsigned int nTriangles = countTriangles(false);
    if (nTriangles == 0) return;
    clearWeldedMark(); // the buffer is about to hold something the weld did not make
    m_meshData.m_Normals.clear(); // (and the soup that joins it has no normals)
    std::vector<VhTriangle> tris(nTriangles);
    downloadTriangles(tris.data(), nTriangles);
    vh::MeshData md;
    recordsToMeshData(reinterpret_cast<const VhVertex*>(tris.data()), 3 * (size_t)nTriangles, md);
    if (!m_offline) {
        // triangle soup appended as it is
        if (m_meshData.hasVertexIndices()) { md.makeTriangleSoupIndices(); m_meshData.merge(md); }
        else {
            m_meshData.m_Vertices.insert(m_meshData.m_Vertices.end(), md.m_Vertices.begin(), md.m_Vertices.end());
            m_meshData.m_Colors.insert(m_meshData.m_Colors.end(), md.m_Colors.begin(), md.m_Colors.end());
        }
    } else {
        // "some sequences exhaust cpu memory... -> merge first"
        md.makeTriangleSoupIndices();
        md.mergeCloseVertices(0.0001f);
        md.removeDuplicateFaces();
        if (!md.m_FaceIndicesVertices.empty()) m_meshData.merge(md);
    }
}

// .cpp:89-145 (the reference appends a numeric suffix instead of overwriting unless told to)
void CUDAMarchingCubesHashSDF::saveMesh(const std::string& filename, const vh::mat4f* transform, bool overwriteExistingFile)
{
    std::string actual = filename;
    if (!overwriteExistingFile) {
        unsigned int num = 0;
        for (;;) {
            std::ifstream probe(actual, std::ios::binary);
            if (!probe) break;
            const size_t dot = filename.find_last_of('.');
            const std::string stem = dot == std::string::npos ? filename : filename.substr(0, dot);
            const std::string ext = dot == std::string::npos ? "" : filename.substr(dot);
            actual = stem + std::to_string(++num) + ext;
        }
    }
    if (!m_welded) { // the indexed extraction's mesh is merged already, exactly
        if (!m_meshData.hasVertexIndices()) m_meshData.makeTriangleSoupIndices();
        m_meshData.mergeCloseVertices(0.0001f);
        m_meshData.removeDuplicateFaces();
    }
    if (transform) m_meshData.applyTransform(*transform);
    m_meshData.saveToPLY(actual);
    clearMeshBuffer();
}
