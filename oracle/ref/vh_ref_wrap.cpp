/*
 * vh_ref_wrap.cpp -- C ABI over the reference's own voxel-hashing code, built for the CPU (oracle/ref/Makefile).
 *
 * TEST INFRASTRUCTURE ONLY, like the oracle.  The reference's headers and .cu files are staged into oracle/_ref/src
 * at build time (oracle/ref/stage.py) and compiled as host C++ against the stand-ins in oracle/ref/include; this
 * file sets the reference's __constant__ parameter blocks from the project's structs (include/vh_types.h, the same
 * layouts, asserted below) and calls its device functions and kernels -- with barriers or without -- on host buffers.  The arguments
 * mirror the oracle's vho_* functions so that a test can run both on two copies of one state.
 *
 * Kernels run through the launch emulator (vhr_launch): every thread of a launch in order, blocks z-y-x then
 * threads z-y-x; a workgroup that reaches __syncthreads (compactify, GC identify) runs barrier by barrier on fibers
 * (oracle/ref/vhr_launch.cpp).
 */
#include "cuda_runtime.h"
#include "cutil_math.h"
#include "cuda_SimpleMatrixUtil.h"
#include "VoxelUtilHashSDF.h"
#include "DepthCameraUtil.h"
#include "RayCastSDFUtil.h"
#include "MarchingCubesSDFUtil.h"

#include <cstddef>
#include <vector>

#include "../../include/vh_types.h"

thread_local uint3 threadIdx, blockIdx;
thread_local dim3 blockDim, gridDim;

HashParams c_hashParams;
RayCastParams c_rayCastParams;
DepthCameraParams c_depthCameraParams;

extern "C" void updateConstantHashParams(const HashParams& p) { c_hashParams = p; }
extern "C" void updateConstantRayCastParams(const RayCastParams& p) { c_rayCastParams = p; }
extern "C" void updateConstantDepthCameraParams(const DepthCameraParams& p) { c_depthCameraParams = p; }

/* CUDASceneRepChunkGrid.cu defines this in the .cu file itself; the same declaration, asserted below */
struct SDFBlockDesc {
    int3 pos;
    int ptr;
};

/* Defined in the staged .cu files: two kernels, and launchers with C linkage.  Our declarations, by type only. */
__global__ void allocKernel(HashData, DepthCameraData, const unsigned int*);
__global__ void computeNormalsDevice(float4*, float4*, unsigned int, unsigned int);
extern "C" {
void bindInputDepthColorTextures(const DepthCameraData&);
void resetCUDA(HashData&, const HashParams&);
void resetHashBucketMutexCUDA(HashData&, const HashParams&);
void allocCUDA(HashData&, const HashParams&, const DepthCameraData&, const DepthCameraParams&, const unsigned int*);
void integrateDepthMapCUDA(HashData&, const HashParams&, const DepthCameraData&, const DepthCameraParams&);
void starveVoxelsKernelCUDA(HashData&, const HashParams&);
void garbageCollectFreeCUDA(HashData&, const HashParams&);
void renderCS(const HashData&, const RayCastData&, const DepthCameraData&, const RayCastParams&);
unsigned int compactifyHashAllInOneCUDA(HashData&, const HashParams&);
void garbageCollectIdentifyCUDA(HashData&, const HashParams&);
void integrateFromGlobalHashPass1CUDA(const HashParams&, const HashData&, uint, uint, float, const float3&, uint*,
                                      SDFBlockDesc*);
void integrateFromGlobalHashPass2CUDA(const HashParams&, const HashData&, uint, const SDFBlockDesc*, Voxel*, unsigned int);
void chunkToGlobalHashPass1CUDA(const HashParams&, const HashData&, uint, uint, const SDFBlockDesc*, const Voxel*);
void chunkToGlobalHashPass2CUDA(const HashParams&, const HashData&, uint, uint, const SDFBlockDesc*, const Voxel*);
void resetMarchingCubesCUDA(MarchingCubesData&);
void extractIsoSurfaceCUDA(const HashData&, const RayCastData&, const MarchingCubesParams&, MarchingCubesData&);
void extractIsoSurfacePass1CUDA(const HashData&, const RayCastData&, const MarchingCubesParams&, MarchingCubesData&);
void extractIsoSurfacePass2CUDA(const HashData&, const RayCastData&, const MarchingCubesParams&, MarchingCubesData&,
                                unsigned int);
void convertColorRawToFloat4(float4*, unsigned char*, unsigned int, unsigned int);
void resampleFloatMap(float*, unsigned int, unsigned int, float*, unsigned int, unsigned int);
void resampleFloat4Map(float4*, unsigned int, unsigned int, float4*, unsigned int, unsigned int);
void convertColorToIntensityFloat(float*, float4*, unsigned int, unsigned int);
void convertDepthFloatToCameraSpaceFloat4(float4*, float*, float4x4, unsigned int, unsigned int, const DepthCameraData&);
void gaussFilterFloatMap(float*, float*, float, float, unsigned int, unsigned int);
void gaussFilterFloat4Map(float4*, float4*, float, float, unsigned int, unsigned int);
void bilateralFilterFloatMap(float*, float*, float, float, unsigned int, unsigned int);
void erodeDepthMap(float*, float*, int, unsigned int, unsigned int, float, float);
void computeIntensityAndDerivatives(float*, unsigned int, unsigned int, float4*);
}

/* the project's structs are the reference's, byte for byte */
static_assert(sizeof(HashEntry) == sizeof(VhHashEntry), "HashEntry layout");
static_assert(offsetof(HashEntry, ptr) == offsetof(VhHashEntry, ptr), "HashEntry layout");
static_assert(offsetof(HashEntry, offset) == offsetof(VhHashEntry, offset), "HashEntry layout");
static_assert(sizeof(Voxel) == sizeof(VhVoxel), "Voxel layout");
static_assert(offsetof(Voxel, weight) == offsetof(VhVoxel, weight), "Voxel layout");
static_assert(sizeof(HashParams) == sizeof(VhHashParams), "HashParams layout");
static_assert(offsetof(HashParams, m_numOccupiedBlocks) == offsetof(VhHashParams, m_numOccupiedBlocks), "HashParams layout");
static_assert(offsetof(HashParams, m_streamingInitialChunkListSize) == offsetof(VhHashParams, m_streamingInitialChunkListSize), "HashParams layout");
static_assert(sizeof(RayCastParams) == sizeof(VhRayCastParams), "RayCastParams layout");
static_assert(offsetof(RayCastParams, m_useGradients) == offsetof(VhRayCastParams, m_useGradients), "RayCastParams layout");
static_assert(sizeof(DepthCameraParams) == sizeof(VhDepthCameraParams), "DepthCameraParams layout");
static_assert(offsetof(DepthCameraParams, m_sensorDepthWorldMax) == offsetof(VhDepthCameraParams, m_sensorDepthWorldMax), "DepthCameraParams layout");
static_assert(sizeof(SDFBlockDesc) == sizeof(VhSDFBlockDesc), "SDFBlockDesc layout");
static_assert(offsetof(SDFBlockDesc, ptr) == offsetof(VhSDFBlockDesc, ptr), "SDFBlockDesc layout");
static_assert(sizeof(MarchingCubesParams) == sizeof(VhMarchingCubesParams), "MarchingCubesParams layout");
static_assert(offsetof(MarchingCubesParams, m_maxNumTriangles) == offsetof(VhMarchingCubesParams, m_maxNumTriangles), "MarchingCubesParams layout");
static_assert(offsetof(MarchingCubesParams, m_threshMarchingCubes2) == offsetof(VhMarchingCubesParams, m_threshMarchingCubes2), "MarchingCubesParams layout");
static_assert(sizeof(MarchingCubesData::Triangle) == sizeof(VhTriangle), "Triangle layout");
static_assert(offsetof(MarchingCubesData::Vertex, c) == offsetof(VhVertex, c), "Vertex layout");

static void set_hash_params(const VhHashParams* hp) { memcpy(&c_hashParams, hp, sizeof(c_hashParams)); }
static void set_camera_params(const VhDepthCameraParams* cp) { memcpy(&c_depthCameraParams, cp, sizeof(c_depthCameraParams)); }
static void set_raycast_params(const VhRayCastParams* rp) { memcpy(&c_rayCastParams, rp, sizeof(c_rayCastParams)); }

static HashData hash_data(const VhHashData* hd)
{
    HashData h;
    h.d_heap = hd->d_heap;
    h.d_heapCounter = hd->d_heapCounter;
    h.d_hashDecision = hd->d_hashDecision;
    h.d_hashDecisionPrefix = hd->d_hashDecisionPrefix;
    h.d_hash = reinterpret_cast<HashEntry*>(hd->d_hash);
    h.d_hashCompactified = reinterpret_cast<HashEntry*>(hd->d_hashCompactified);
    h.d_hashCompactifiedCounter = hd->d_hashCompactifiedCounter;
    h.d_SDFBlocks = reinterpret_cast<Voxel*>(hd->d_SDFBlocks);
    h.d_hashBucketMutex = hd->d_hashBucketMutex;
    h.m_bIsOnGPU = true;
    return h;
}

static float3 f3(const float p[3]) { return make_float3(p[0], p[1], p[2]); }
static int3 i3(const int32_t p[3]) { return make_int3(p[0], p[1], p[2]); }
static void put3(float* o, float3 v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }
static void put3(int32_t* o, int3 v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }

/* A depth frame as the reference's textures see it: two cudaArrays over the caller's host images. */
struct Frame {
    cudaArray depth{}, color{};
    DepthCameraData cam;
    Frame(const VhDepthCameraData* c, const VhDepthCameraParams* cp)
    {
        depth.data = c->d_depthData; depth.width = cp->m_imageWidth; depth.height = cp->m_imageHeight; depth.elemBytes = 4;
        color.data = c->d_colorData; color.width = cp->m_imageWidth; color.height = cp->m_imageHeight; color.elemBytes = 16;
        cam.d_depthData = const_cast<float*>(c->d_depthData);
        cam.d_colorData = reinterpret_cast<float4*>(const_cast<float*>(c->d_colorData));
        cam.d_depthArray = &depth;
        cam.d_colorArray = c->d_colorData ? &color : nullptr;
        cam.h_depthChannelDesc = cudaCreateChannelDesc(32, 0, 0, 0, cudaChannelFormatKindFloat);
        cam.h_colorChannelDesc = cudaCreateChannelDesc(32, 32, 32, 32, cudaChannelFormatKindFloat);
        bindInputDepthColorTextures(cam);
    }
};

extern "C" {

/* ---- HashData device functions (VoxelUtilHashSDF.h) ---- */
uint32_t vhr_compute_hash_pos(const VhHashParams* hp, const int32_t pos[3])
{
    set_hash_params(hp);
    return HashData().computeHashPos(i3(pos));
}

void vhr_world_to_virtual_voxel_pos(const VhHashParams* hp, const float p[3], int32_t out[3])
{
    set_hash_params(hp);
    put3(out, HashData().worldToVirtualVoxelPos(f3(p)));
}

void vhr_virtual_voxel_pos_to_sdf_block(const int32_t v[3], int32_t out[3])
{
    put3(out, HashData().virtualVoxelPosToSDFBlock(i3(v)));
}

void vhr_world_to_sdf_block(const VhHashParams* hp, const float p[3], int32_t out[3])
{
    set_hash_params(hp);
    put3(out, HashData().worldToSDFBlock(f3(p)));
}

void vhr_sdf_block_to_world(const VhHashParams* hp, const int32_t b[3], float out[3])
{
    set_hash_params(hp);
    put3(out, HashData().SDFBlockToWorld(i3(b)));
}

void vhr_virtual_voxel_pos_to_world(const VhHashParams* hp, const int32_t v[3], float out[3])
{
    set_hash_params(hp);
    put3(out, HashData().virtualVoxelPosToWorld(i3(v)));
}

int vhr_virtual_voxel_pos_to_local_index(const int32_t v[3])
{
    return HashData().virtualVoxelPosToLocalSDFBlockIndex(i3(v));
}

uint32_t vhr_linearize_voxel_pos(const int32_t v[3])
{
    return HashData().linearizeVoxelPos(i3(v));
}

void vhr_delinearize_voxel_index(uint32_t idx, int32_t out[3])
{
    uint3 d = HashData().delinearizeVoxelIndex(idx);
    out[0] = (int32_t)d.x; out[1] = (int32_t)d.y; out[2] = (int32_t)d.z;
}

int vhr_is_block_in_frustum(const VhHashParams* hp, const VhDepthCameraParams* cp, const int32_t blk[3])
{
    set_hash_params(hp);
    set_camera_params(cp);
    return HashData().isSDFBlockInCameraFrustumApprox(i3(blk)) ? 1 : 0;
}

float vhr_get_truncation(const VhHashParams* hp, float z)
{
    set_hash_params(hp);
    return HashData().getTruncation(z);
}

VhVoxel vhr_combine_voxel(const VhHashParams* hp, VhVoxel v0, VhVoxel v1)
{
    set_hash_params(hp);
    Voxel a, b, o;
    memcpy(&a, &v0, sizeof(a));
    memcpy(&b, &v1, sizeof(b));
    memset(&o, 0, sizeof(o));
    HashData().combineVoxel(a, b, o);
    VhVoxel r;
    memcpy(&r, &o, sizeof(r));
    return r;
}

/* ---- DepthCameraData (DepthCameraUtil.h) ---- */
void vhr_camera_to_screen_float(const VhDepthCameraParams* cp, const float p[3], float out[2])
{
    set_camera_params(cp);
    float2 s = DepthCameraData::cameraToKinectScreenFloat(f3(p));
    out[0] = s.x; out[1] = s.y;
}

void vhr_camera_to_screen_int(const VhDepthCameraParams* cp, const float p[3], int32_t out[2])
{
    set_camera_params(cp);
    int2 s = DepthCameraData::cameraToKinectScreenInt(f3(p));
    out[0] = s.x; out[1] = s.y;
}

void vhr_camera_to_proj(const VhDepthCameraParams* cp, const float p[3], float out[3])
{
    set_camera_params(cp);
    put3(out, DepthCameraData::cameraToKinectProj(f3(p)));
}

float vhr_camera_to_proj_z(const VhDepthCameraParams* cp, float z)
{
    set_camera_params(cp);
    return DepthCameraData::cameraToKinectProjZ(z);
}

void vhr_depth_to_skeleton(const VhDepthCameraParams* cp, uint32_t ux, uint32_t uy, float depth, float out[3])
{
    set_camera_params(cp);
    put3(out, DepthCameraData::kinectDepthToSkeleton(ux, uy, depth));
}

float vhr_proj_to_camera_z(const VhDepthCameraParams* cp, float z)
{
    set_camera_params(cp);
    return DepthCameraData::kinectProjToCameraZ(z);
}

/* ---- hash table operations ---- */
VhHashEntry vhr_get_hash_entry(const VhHashData* hd, const VhHashParams* hp, const int32_t pos[3])
{
    set_hash_params(hp);
    HashEntry e = hash_data(hd).getHashEntryForSDFBlockPos(i3(pos));
    VhHashEntry r;
    memset(&r, 0, sizeof(r));
    memcpy(&r, &e, sizeof(r));
    return r;
}

void vhr_alloc_block(VhHashData* hd, const VhHashParams* hp, const int32_t pos[3])
{
    set_hash_params(hp);
    hash_data(hd).allocBlock(i3(pos));
}

int vhr_delete_hash_entry_element(VhHashData* hd, const VhHashParams* hp, const int32_t pos[3])
{
    set_hash_params(hp);
    return hash_data(hd).deleteHashEntryElement(i3(pos)) ? 1 : 0;
}

/* The bucket part only: the reference's list branch is a fenced defect, so a call that would
 * reach it returns -1 and leaves the table alone. */
int vhr_insert_hash_entry_bucket(VhHashData* hd, const VhHashParams* hp, const VhHashEntry* e)
{
    set_hash_params(hp);
    HashData h = hash_data(hd);
    uint32_t b = h.computeHashPos(i3(e->pos));
    bool room = false;
    for (uint32_t j = 0; j < HASH_BUCKET_SIZE; j++) room |= h.d_hash[b * HASH_BUCKET_SIZE + j].ptr == FREE_ENTRY;
    if (!room) return -1;
    HashEntry x;
    memcpy(&x, e, sizeof(x));
    return h.insertHashEntry(x) ? 1 : 0;
}

/* ---- kernels through the launch emulator ---- */

/* resetCUDA: heap, table, mutexes */
void vhr_reset(VhHashData* hd, const VhHashParams* hp)
{
    set_hash_params(hp);
    HashData h = hash_data(hd);
    HashParams p = c_hashParams;
    resetCUDA(h, p);
}

void vhr_reset_bucket_mutex(VhHashData* hd, const VhHashParams* hp)
{
    set_hash_params(hp);
    HashData h = hash_data(hd);
    HashParams p = c_hashParams;
    resetHashBucketMutexCUDA(h, p);
}

/* float4x4::getInverse (cuda_SimpleMatrixUtil.h), row-major */
void vhr_mat4_inverse(const float m[16], float out[16])
{
    float4x4 a(m);
    float4x4 r = a.getInverse();
    memcpy(out, &r, sizeof(float) * 16);
}

/* allocKernel.  raster != 0: one row of threads per block row (threads in raster order, the oracle's order);
 * raster == 0: the reference's own launcher allocCUDA (8x8 tiles).  bitMask NULL = an all-zero chunk mask. */
void vhr_alloc(VhHashData* hd, const VhHashParams* hp, const VhDepthCameraData* c, const VhDepthCameraParams* cp,
               const uint32_t* bitMask, int raster)
{
    set_hash_params(hp);
    set_camera_params(cp);
    std::vector<uint32_t> zero;
    if (!bitMask) {
        const size_t chunks = (size_t)hp->m_streamingGridDimensions[0] * hp->m_streamingGridDimensions[1] *
                              hp->m_streamingGridDimensions[2];
        zero.assign(chunks / 32 + 1, 0u);
        bitMask = zero.data();
    }
    Frame f(c, cp);
    HashData h = hash_data(hd);
    HashParams p = c_hashParams;
    DepthCameraParams q = c_depthCameraParams;
    if (raster) vhr_launch(dim3(1, cp->m_imageHeight), dim3(cp->m_imageWidth, 1), allocKernel, h, f.cam, bitMask);
    else allocCUDA(h, p, f.cam, q, bitMask);
}

/* integrateDepthMapCUDA over hd->d_hashCompactified[0 .. hp->m_numOccupiedBlocks) */
void vhr_integrate(VhHashData* hd, const VhHashParams* hp, const VhDepthCameraData* c, const VhDepthCameraParams* cp)
{
    set_hash_params(hp);
    set_camera_params(cp);
    Frame f(c, cp);
    HashData h = hash_data(hd);
    HashParams p = c_hashParams;
    DepthCameraParams q = c_depthCameraParams;
    integrateDepthMapCUDA(h, p, f.cam, q);
}

void vhr_starve(VhHashData* hd, const VhHashParams* hp)
{
    set_hash_params(hp);
    HashData h = hash_data(hd);
    HashParams p = c_hashParams;
    starveVoxelsKernelCUDA(h, p);
}

/* garbageCollectFreeCUDA on the decisions in hd->d_hashDecision */
void vhr_gc_free(VhHashData* hd, const VhHashParams* hp)
{
    set_hash_params(hp);
    HashData h = hash_data(hd);
    HashParams p = c_hashParams;
    garbageCollectFreeCUDA(h, p);
}

/* renderCS: the four maps of rd, from rp's view (no ray intervals: the reference's kernel ignores them) */
void vhr_render(const VhHashData* hd, const VhHashParams* hp, const VhRayCastData* rd, const VhDepthCameraParams* cp,
                const VhRayCastParams* rp)
{
    set_hash_params(hp);
    set_camera_params(cp);
    set_raycast_params(rp);
    RayCastData r;
    r.d_depth = rd->d_depth;
    r.d_depth4 = reinterpret_cast<float4*>(rd->d_depth4);
    r.d_normals = reinterpret_cast<float4*>(rd->d_normals);
    r.d_colors = reinterpret_cast<float4*>(rd->d_colors);
    DepthCameraData cam;
    RayCastParams p = c_rayCastParams;
    renderCS(hash_data(hd), r, cam, p);
}

void vhr_compute_normals(float* out4, const float* in4, uint32_t width, uint32_t height)
{
    vhr_launch(dim3((width + 7) / 8, (height + 7) / 8), dim3(8, 8), computeNormalsDevice,
               reinterpret_cast<float4*>(out4), reinterpret_cast<float4*>(const_cast<float*>(in4)), width, height);
}

/* ---- RayCastData device functions (RayCastSDFUtil.h) ---- */
int vhr_trilinear(const VhHashData* hd, const VhHashParams* hp, const float pos[3], float* dist, uint8_t color[3])
{
    set_hash_params(hp);
    RayCastData r;
    uchar3 c = make_uchar3(0, 0, 0);
    float d = 0.0f;
    bool ok = r.trilinearInterpolationSimpleFastFast(hash_data(hd), f3(pos), d, c);
    *dist = d;
    color[0] = c.x; color[1] = c.y; color[2] = c.z;
    return ok ? 1 : 0;
}

int vhr_intersect_bisection(const VhHashData* hd, const VhHashParams* hp, const float camPos[3], const float dir[3],
                            float d0, float r0, float d1, float r1, float* alpha, uint8_t color[3])
{
    set_hash_params(hp);
    RayCastData r;
    uchar3 c = make_uchar3(0, 0, 0);
    float a = 0.0f;
    bool ok = r.findIntersectionBisection(hash_data(hd), f3(camPos), f3(dir), d0, r0, d1, r1, a, c);
    *alpha = a;
    color[0] = c.x; color[1] = c.y; color[2] = c.z;
    return ok ? 1 : 0;
}

void vhr_gradient_for_point(const VhHashData* hd, const VhHashParams* hp, const float pos[3], float out[3])
{
    set_hash_params(hp);
    RayCastData r;
    put3(out, r.gradientForPoint(hash_data(hd), f3(pos)));
}

/* ---- kernels with barriers ---- */

/* compactifyHashAllInOneCUDA: the count, also left in hp->m_numOccupiedBlocks */
uint32_t vhr_compactify(VhHashData* hd, VhHashParams* hp, const VhDepthCameraParams* cp)
{
    set_hash_params(hp);
    set_camera_params(cp);
    HashData h = hash_data(hd);
    HashParams p = c_hashParams;
    const unsigned int n = compactifyHashAllInOneCUDA(h, p);
    hp->m_numOccupiedBlocks = n;
    return n;
}

/* garbageCollectIdentifyCUDA over hd->d_hashCompactified[0 .. hp->m_numOccupiedBlocks); the threshold reads cp */
void vhr_gc_identify(VhHashData* hd, const VhHashParams* hp, const VhDepthCameraParams* cp)
{
    set_hash_params(hp);
    set_camera_params(cp);
    HashData h = hash_data(hd);
    HashParams p = c_hashParams;
    garbageCollectIdentifyCUDA(h, p);
}

/* ---- streaming (CUDASceneRepChunkGrid.cu) ---- */

/* integrateFromGlobalHashPass1CUDA: returns the number of descriptors; out must hold every one the pass writes */
uint32_t vhr_stream_out_pass1(VhHashData* hd, const VhHashParams* hp, uint32_t threadsPerPart, uint32_t start,
                              float radius, const float camPos[3], VhSDFBlockDesc* out, uint32_t outCapacity)
{
    set_hash_params(hp);
    HashData h = hash_data(hd);
    HashParams p = c_hashParams;
    uint32_t counter = 0;
    const float3 c = f3(camPos);
    /* room for every thread of the launch: threadsPerPart rounded up to whole workgroups of 64 */
    std::vector<SDFBlockDesc> buf(((size_t)threadsPerPart + 63) / 64 * 64 + 1);
    integrateFromGlobalHashPass1CUDA(p, h, threadsPerPart, start, radius, c, &counter, buf.data());
    memcpy(out, buf.data(), sizeof(SDFBlockDesc) * (counter < outCapacity ? counter : outCapacity));
    return counter;
}

void vhr_stream_out_pass2(VhHashData* hd, const VhHashParams* hp, const VhSDFBlockDesc* descs, VhVoxel* out, uint32_t n)
{
    set_hash_params(hp);
    HashData h = hash_data(hd);
    HashParams p = c_hashParams;
    integrateFromGlobalHashPass2CUDA(p, h, n, reinterpret_cast<const SDFBlockDesc*>(descs), reinterpret_cast<Voxel*>(out), n);
}

/* chunkToGlobalHashPass1CUDA.  Its insertHashEntry's list branch is a fenced defect: callers
 * give it only entries whose bucket has room. */
void vhr_stream_in_pass1(VhHashData* hd, const VhHashParams* hp, uint32_t n, uint32_t heapCountPrev,
                         const VhSDFBlockDesc* descs)
{
    set_hash_params(hp);
    HashData h = hash_data(hd);
    HashParams p = c_hashParams;
    chunkToGlobalHashPass1CUDA(p, h, n, heapCountPrev, reinterpret_cast<const SDFBlockDesc*>(descs), nullptr);
}

void vhr_stream_in_pass2(VhHashData* hd, const VhHashParams* hp, uint32_t n, uint32_t heapCountPrev,
                         const VhSDFBlockDesc* descs, const VhVoxel* blocks)
{
    set_hash_params(hp);
    HashData h = hash_data(hd);
    HashParams p = c_hashParams;
    chunkToGlobalHashPass2CUDA(p, h, n, heapCountPrev, reinterpret_cast<const SDFBlockDesc*>(descs),
                               reinterpret_cast<const Voxel*>(blocks));
}

/* ---- marching cubes (CUDAMarchingCubesSDF.cu) ----
 * resetMarchingCubesCUDA, then extractIsoSurfacePass1CUDA + Pass2CUDA (twoPass != 0) or the one-kernel
 * extractIsoSurfaceCUDA, with room for maxTriangles triangles (mp->m_maxNumTriangles is replaced by it).  Returns the
 * reference's triangle counter, which it clamps to the capacity. */
uint32_t vhr_extract_iso_surface(const VhHashData* hd, const VhHashParams* hp, const VhMarchingCubesParams* mp,
                                 VhTriangle* out, uint32_t maxTriangles, int twoPass)
{
    set_hash_params(hp);
    MarchingCubesParams params;
    memcpy(&params, mp, sizeof(params));
    params.m_maxNumTriangles = maxTriangles;
    const uint32_t entries = hp->m_hashNumBuckets * HASH_BUCKET_SIZE;
    std::vector<uint> occupied(entries ? entries : 1);
    uint numOccupied = 0, numTriangles = 0;
    MarchingCubesData d;
    d.d_params = &params;
    d.d_numOccupiedBlocks = &numOccupied;
    d.d_occupiedBlocks = occupied.data();
    d.d_numTriangles = &numTriangles;
    d.d_triangles = reinterpret_cast<MarchingCubesData::Triangle*>(out);
    d.m_bIsOnGPU = true;
    HashData h = hash_data(hd);
    RayCastData r;
    resetMarchingCubesCUDA(d);
    if (twoPass) {
        extractIsoSurfacePass1CUDA(h, r, params, d);
        extractIsoSurfacePass2CUDA(h, r, params, d, numOccupied);
    } else {
        extractIsoSurfaceCUDA(h, r, params, d);
    }
    return numTriangles;
}

/* ---- sensor maps (CameraUtil.cu) ---- */
void vhr_convert_color_raw_to_float4(float* out4, const uint8_t* rgbx, uint32_t w, uint32_t h)
{
    convertColorRawToFloat4(reinterpret_cast<float4*>(out4), const_cast<uint8_t*>(rgbx), w, h);
}

void vhr_resample_float_map(float* out, uint32_t ow, uint32_t oh, const float* in, uint32_t w, uint32_t h)
{
    resampleFloatMap(out, ow, oh, const_cast<float*>(in), w, h);
}

void vhr_resample_float4_map(float* out4, uint32_t ow, uint32_t oh, const float* in4, uint32_t w, uint32_t h)
{
    resampleFloat4Map(reinterpret_cast<float4*>(out4), ow, oh, reinterpret_cast<float4*>(const_cast<float*>(in4)), w, h);
}

void vhr_convert_color_to_intensity_float(float* out, const float* in4, uint32_t w, uint32_t h)
{
    convertColorToIntensityFloat(out, reinterpret_cast<float4*>(const_cast<float*>(in4)), w, h);
}

/* the kernel ignores its intrinsicsInv argument (it back-projects through c_depthCameraParams) */
void vhr_convert_depth_float_to_camera_space_float4(float* out4, const float* in, const VhDepthCameraParams* cp,
                                                    uint32_t w, uint32_t h)
{
    set_camera_params(cp);
    DepthCameraData cam;
    convertDepthFloatToCameraSpaceFloat4(reinterpret_cast<float4*>(out4), const_cast<float*>(in), float4x4(), w, h, cam);
}

void vhr_gauss_filter_float_map(float* out, const float* in, float sigmaD, float sigmaR, uint32_t w, uint32_t h)
{
    gaussFilterFloatMap(out, const_cast<float*>(in), sigmaD, sigmaR, w, h);
}

void vhr_gauss_filter_float4_map(float* out4, const float* in4, float sigmaD, float sigmaR, uint32_t w, uint32_t h)
{
    gaussFilterFloat4Map(reinterpret_cast<float4*>(out4), reinterpret_cast<float4*>(const_cast<float*>(in4)), sigmaD,
                         sigmaR, w, h);
}

void vhr_bilateral_filter_float_map(float* out, const float* in, float sigmaD, float sigmaR, uint32_t w, uint32_t h)
{
    bilateralFilterFloatMap(out, const_cast<float*>(in), sigmaD, sigmaR, w, h);
}

void vhr_erode_depth_map(float* out, const float* in, int structureSize, uint32_t w, uint32_t h, float dThresh,
                         float fracReq)
{
    erodeDepthMap(out, const_cast<float*>(in), structureSize, w, h, dThresh, fracReq);
}

void vhr_compute_intensity_and_derivatives(float* out4, const float* in, uint32_t w, uint32_t h)
{
    computeIntensityAndDerivatives(const_cast<float*>(in), w, h, reinterpret_cast<float4*>(out4));
}

} /* extern "C" */
