/*
 * vh_types.h -- plain-old-data types of the voxel-hashing TSDF hot path.
 *
 * C-compatible (included by the HIP library, by the C oracle and by FFI users).
 * Every struct names the reference type it replaces.  Field names and field
 * order follow the reference so that a maintainer can memcpy between the two.
 *
 *   DSC/ = /root/reference/DepthSensingCUDA/Source/
 */
#ifndef VH_TYPES_H
#define VH_TYPES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Compile-time constants of the reference (DSC/VoxelUtilHashSDF.h:39-54). */
#define VH_SDF_BLOCK_SIZE 8
#define VH_SDF_BLOCK_VOXELS 512 /* 8*8*8 */
#define VH_HASH_BUCKET_SIZE 10
#define VH_LOCK_ENTRY (-1)
#define VH_FREE_ENTRY (-2)
#define VH_NO_OFFSET 0

/* HashEntry, DSC/VoxelUtilHashSDF.h:56-74.  20 B payload; 32 B stride is what
 * __align__(16) yields on the reference toolchain and gives 16 B-aligned
 * {pos,ptr} quads for single dwordx4 probes on gfx950. */
typedef struct VhHashEntry {
    int32_t pos[3];   /* SDF-block coordinates (x,y,z) */
    int32_t ptr;      /* first voxel index (= block id * 512), or FREE/LOCK */
    uint32_t offset;  /* collision-list hop, relative to the home bucket's last slot */
    uint32_t _pad[3];
} VhHashEntry;

/* Voxel, DSC/VoxelUtilHashSDF.h:76-88.  8 B, moved as one 64-bit word. */
typedef struct VhVoxel {
    float sdf;
    uint8_t color[3];
    uint8_t weight;
} VhVoxel;

/* HashParams, DSC/CUDAHashParams.h:8-38 (224 B). Matrices are row-major
 * (DSC/cuda_SimpleMatrixUtil.h:1127-1137: entries[16] = m11,m12,...,m44). */
typedef struct VhHashParams {
    float m_rigidTransform[16];
    float m_rigidTransformInverse[16];

    uint32_t m_hashNumBuckets;
    uint32_t m_hashBucketSize;
    uint32_t m_hashMaxCollisionLinkedListSize;
    uint32_t m_numSDFBlocks;

    int32_t m_SDFBlockSize;
    float m_virtualVoxelSize;
    uint32_t m_numOccupiedBlocks; /* occupied blocks in the viewing frustum */

    float m_maxIntegrationDistance;
    float m_truncScale;
    float m_truncation;
    uint32_t m_integrationWeightSample;
    uint32_t m_integrationWeightMax;

    float m_streamingVoxelExtents[3];
    int32_t m_streamingGridDimensions[3];
    int32_t m_streamingMinGridPos[3];
    uint32_t m_streamingInitialChunkListSize;
    /* The reference's two spare words (m_dummy[2]); the first is a switch the reference does not have.
     * 0: combineVoxel's colour as the reference computes it, a running 50/50 average (DSC/VoxelUtilHashSDF.h:236-240);
     * 1: the average weighted by the voxel weights that the reference left commented out at :241,
     *    uchar((c0 w0 + c1 w1) / (w0 + w1) + 0.5f) per channel.  Set by CUDASceneRepHashSDF::setColorIntegration. */
    uint32_t m_colorIntegration;
    uint32_t m_dummy;
} VhHashParams;

enum { VH_COLOR_RUNNING_AVERAGE = 0, VH_COLOR_WEIGHTED_AVERAGE = 1 };

/* DepthCameraParams, DSC/CUDADepthCameraParams.h:8-19 (32 B). */
typedef struct VhDepthCameraParams {
    float fx, fy, mx, my;
    uint32_t m_imageWidth;
    uint32_t m_imageHeight;
    float m_sensorDepthWorldMin;
    float m_sensorDepthWorldMax;
} VhDepthCameraParams;

/* RayCastParams, DSC/CUDARayCastParams.h:7-28 (304 B). */
typedef struct VhRayCastParams {
    float m_viewMatrix[16];
    float m_viewMatrixInverse[16];
    float m_intrinsics[16];
    float m_intrinsicsInverse[16];

    uint32_t m_width;
    uint32_t m_height;

    uint32_t m_numOccupiedSDFBlocks;
    uint32_t m_maxNumVertices;
    int32_t m_splatMinimum;

    float m_minDepth;
    float m_maxDepth;
    float m_rayIncrement;
    float m_thresSampleDist;
    float m_thresDist;
    uint8_t m_useGradients; /* bool in the reference */
    uint8_t _pad0[3];

    uint32_t dummy0;
} VhRayCastParams;

/* HashData, DSC/VoxelUtilHashSDF.h:813-823: the nine device buffers, in the
 * reference's order.  Two extension buffers follow (not in the reference):
 * a per-bucket occupancy count and a 1-bit-per-bucket summary that let the
 * compaction and the ray caster skip empty buckets without touching d_hash.
 * They are owned by vh_hash_data_alloc()/vh_hash_data_free() like the rest. */
typedef struct VhHashData {
    uint32_t* d_heap;                  /* [numSDFBlocks] free-list of block ids */
    uint32_t* d_heapCounter;           /* [1] index of the top free element */
    int32_t* d_hashDecision;           /* [numEntries] GC decisions (first No used) */
    int32_t* d_hashDecisionPrefix;     /* [numEntries] kept for layout parity; unused */
    VhHashEntry* d_hash;               /* [numEntries] */
    VhHashEntry* d_hashCompactified;   /* [numEntries] in-frustum occupied entries */
    int32_t* d_hashCompactifiedCounter;/* [1] */
    VhVoxel* d_SDFBlocks;              /* [numSDFBlocks*512] */
    int32_t* d_hashBucketMutex;        /* [numBuckets] */
    uint8_t m_bIsOnGPU;
    uint8_t _pad0[7];
    /* --- extensions --- */
    uint32_t* d_bucketCount;           /* [numBuckets] occupied slots physically in bucket */
    uint32_t* d_bucketBits;            /* [ceil(numBuckets/32)] bit b = (d_bucketCount[b] != 0) */
    uint32_t* d_state;                 /* [VH_STATE_WORDS] device-side status words */
} VhHashData;

/* words of VhHashData::d_state */
enum {
    VH_STATE_HEAP_UNDERFLOW = 0, /* consumeHeap found the heap empty */
    VH_STATE_INSERT_FAILED = 1,  /* stream-in: insertHashEntry returned false */
    VH_STATE_ALLOC_LOCK_LOST = 2,/* alloc requests that lost a bucket lock this pass */
    VH_STATE_RIDER_GAVE_UP = 3,  /* workgroups of a co-launched pass over the voxels that gave up waiting for the launch's other riders (must stay 0) */
    VH_STATE_WORDS = 16
};

/* Scene merge (vh_merge_blocks): bits of its status word, and what the call counts.  Any status leaves the scene a
 * scene; VH_MERGE_HEAP_SHORT leaves it untouched. */
#define VH_MERGE_HEAP_SHORT 1u  /* the source names more absent positions than the heap has free blocks: nothing was done */
#define VH_MERGE_NO_SLOT 2u     /* allocBlock found no room for a block (bucket and list limit): that block was left out whole */
#define VH_MERGE_NOT_SETTLED 4u /* blocks still lost their lock races at the bound on alloc passes: they were left out whole */
enum {
    VH_MERGE_SOURCE_BLOCKS = 0, /* n */
    VH_MERGE_PRESENT = 1,       /* source blocks whose position the destination already held */
    VH_MERGE_ALLOCATED = 2,     /* source blocks the call allocated */
    VH_MERGE_LEFT_OUT = 3,      /* source blocks left out whole (depends on the order the allocs ran in) */
    VH_MERGE_COMBINED = 4,      /* voxels with both weights > 0: combineVoxel */
    VH_MERGE_COPIED = 5,        /* voxels with destination weight 0 and source weight > 0: the source's, weight capped */
    VH_MERGE_ALLOC_PASSES = 6,  /* alloc passes run (depends on the order the allocs ran in) */
    VH_MERGE_STATUS = 7,
    VH_MERGE_NUM_COUNTS = 8
};

/* Resampled merge (vh_resample_blocks): bits of its status word, and what the call counts.  Any status bit means that
 * nothing was staged: there is nothing to merge and the destination is untouched.  No count depends on the order in
 * which the device's atomics ran. */
#define VH_RESAMPLE_OUT_OF_RANGE 1u /* a source block, or a destination block it reaches, lies outside [-2^20, 2^20) */
#define VH_RESAMPLE_TABLE_FULL 2u   /* the table that makes the candidates distinct had no slot left: call again with more slots */
enum {
    VH_RESAMPLE_SOURCE_BLOCKS = 0, /* n */
    VH_RESAMPLE_CANDIDATES = 1,    /* distinct destination blocks some source block may reach */
    VH_RESAMPLE_STAGED = 2,        /* candidates with an observed voxel: the blocks handed to the merge */
    VH_RESAMPLE_OBSERVED = 3,      /* observed voxels in the staged blocks */
    VH_RESAMPLE_STATUS = 4,
    VH_RESAMPLE_NUM_COUNTS = 5
};

/* Scene cut (vh_cut_blocks): the region's shape, the call's flags, bits of its status word, and what the call counts.
 * VH_CUT_STAGING_SHORT means that nothing was written anywhere; VH_CUT_NOT_SETTLED leaves a valid table in which some
 * blocks that were to be freed are still allocated, all zero. */
#define VH_CUT_BOX 0u       /* inside: |u_x| <= 1 && |u_y| <= 1 && |u_z| <= 1 */
#define VH_CUT_ELLIPSOID 1u /* inside: (u_x u_x + u_y u_y) + u_z u_z <= 1 */
#define VH_CUT_SELECT_OUTSIDE 1u /* the selected voxels are those that are not inside */
#define VH_CUT_LIFT 2u           /* blocks with a selected observed voxel are written to the staging pool */
#define VH_CUT_KEEP 4u           /* (with VH_CUT_LIFT) nothing in the table is written: the region is copied out */
#define VH_CUT_COUNT_ONLY 8u     /* classify and count; write nothing to table, pool or staging */
#define VH_CUT_STAGING_SHORT 1u /* more blocks to lift than the staging pool has room for: nothing was done */
#define VH_CUT_NOT_SETTLED 2u   /* freed blocks still lost their lock races at the bound on delete passes: they stay allocated, all zero */
enum {
    VH_CUT_BLOCKS_IN = 0,     /* n */
    VH_CUT_TOUCHED = 1,       /* blocks with a selected voxel, whatever its weight */
    VH_CUT_FREED = 2,         /* touched blocks without an unselected observed voxel: their entries are removed (0 with VH_CUT_KEEP) */
    VH_CUT_LIFTED = 3,        /* touched blocks with a selected observed voxel: written to the staging pool (0 without VH_CUT_LIFT) */
    VH_CUT_VOXELS_ERASED = 4, /* selected voxels of weight > 0 (0 with VH_CUT_KEEP) */
    VH_CUT_VOXELS_LIFTED = 5, /* selected voxels of weight > 0 (0 without VH_CUT_LIFT) */
    VH_CUT_DELETE_PASSES = 6, /* delete passes run (depends on the order the deletes ran in) */
    VH_CUT_UNSETTLED = 7,     /* freed blocks still pending at the bound on passes (depends on that order too) */
    VH_CUT_STATUS = 8,
    VH_CUT_NUM_COUNTS = 9
};
/* A region in the world: a box or an ellipsoid with the given half extents along the axes of its own frame (a sphere
 * is an ellipsoid with three equal extents, an axis-aligned box has R = I). */
typedef struct VhCutRegion {
    double worldFromRegion[16]; /* rigid 4x4 row-major [R | t], metres */
    float halfExtents[3];       /* > 0, metres */
    uint32_t shape;             /* VH_CUT_BOX / VH_CUT_ELLIPSOID */
} VhCutRegion;

/* Frame de-integration (vh_deintegrate_blocks): the call's flag, the bit of its status word, and what the call counts.
 * VH_DEINT_NOT_SETTLED leaves a valid table in which some blocks that were to be freed are still allocated, all zero. */
#define VH_DEINT_COUNT_ONLY 1u  /* classify and count; write nothing but the work buffer */
#define VH_DEINT_NOT_SETTLED 1u /* freed blocks still lost their lock races at the bound on delete passes: they stay allocated, all zero */
enum {
    VH_DEINT_BLOCKS_IN = 0,      /* n */
    VH_DEINT_PROCESSED = 1,      /* listed blocks in the frame's frustum */
    VH_DEINT_CHANGED = 2,        /* processed blocks in which the take-out changed a voxel */
    VH_DEINT_FREED = 3,          /* processed blocks left without a voxel of weight > 0, changed or not: their entries are removed */
    VH_DEINT_VOXELS_CHANGED = 4, /* voxels of weight > 0 with an observation: the take-out applied (the next two are among them) */
    VH_DEINT_VOXELS_RESET = 5,   /* ... whose observation weighs at least what the voxel does: 8 zero bytes now */
    VH_DEINT_VOXELS_AT_CAP = 6,  /* ... whose weight was m_integrationWeightMax before the call: the take-out is not the inverse there */
    VH_DEINT_DELETE_PASSES = 7,  /* delete passes run (depends on the order the deletes ran in) */
    VH_DEINT_UNSETTLED = 8,      /* freed blocks still pending at the bound on passes (depends on that order too) */
    VH_DEINT_STATUS = 9,
    VH_DEINT_NUM_COUNTS = 10
};

/* Scene registration (vh_align_begin / vh_align_step; DESIGN.md section 4 "Scene registration"): bits of the state's
 * status word, the places of the 29 totals, and the state itself.  A state whose status has any bit set takes no
 * further step: a launch that finds it so returns at once and changes no word of it. */
#define VH_ALIGN_CONVERGED 1u        /* the last step's rotation and translation were below the thresholds (the step was taken) */
#define VH_ALIGN_TOO_FEW 2u          /* fewer than minCount voxels contributed: no step */
#define VH_ALIGN_ILL_CONDITIONED 4u  /* the condition number of J^T J exceeds condThres (or is not a number): no step */
#define VH_ALIGN_OUT_OF_RANGE 8u     /* a listed block lies outside [-2^20, 2^20), or its samples reach more destination blocks than the bound: no step */
#define VH_ALIGN_TOO_MANY 16u        /* more than VH_ALIGN_MOST_BLOCKS listed blocks: nothing was launched (a total could wrap) */
#define VH_ALIGN_ITERATIONS_SPENT 32u /* VH_ALIGN_MAX_ITERATIONS steps were taken */
#define VH_ALIGN_MAX_ITERATIONS 64u
#define VH_ALIGN_MOST_BLOCKS (1u << 19)
#define VH_ALIGN_MOST_BAND 4.0f      /* the band in voxels: bounds the residual, and with it every term */
#define VH_ALIGN_QUANTUM_LOG2 26     /* a term t is summed as the integer rint(t * 2^26) */
#define VH_ALIGN_NUM_STRIPES 32u
enum {
    VH_ALIGN_JTJ = 0,    /* 21 words: the upper triangle of J^T J by rows (00 01 .. 05 11 12 ..) */
    VH_ALIGN_JTE = 21,   /* 6 words: J^T e */
    VH_ALIGN_EE = 27,    /* e e */
    VH_ALIGN_COUNT = 28, /* the contributing voxels (each adds 1.0, that is 2^26) */
    VH_ALIGN_NUM_TERMS = 29
};
typedef struct VhAlignState {
    double dstFromSrc[16];      /* the current estimate, metres, row-major [R | t] */
    float srcVoxFromDstVox[12]; /* the two voxel matrices of the estimate, by the formulas of vh_resample_voxel_transforms */
    float dstVoxFromSrcVox[12];
    float pivot[3];             /* destination voxel index space */
    float invRadius;            /* a power of two */
    float vsSrc, vsDst;
    uint32_t iterations;        /* steps attempted (a refused one counts) */
    uint32_t status;
    uint32_t raised;            /* status bits raised by the workgroups of the launch in flight; 0 between launches */
    uint32_t reserved;
    /* per attempted step k < iterations */
    uint32_t count[VH_ALIGN_MAX_ITERATIONS];          /* contributing voxels */
    float condition[VH_ALIGN_MAX_ITERATIONS];         /* of J^T J, as vh's 6x6 solve reports it */
    double sumSquares[VH_ALIGN_MAX_ITERATIONS];       /* sum of e e, voxels squared */
    double stepRotation[VH_ALIGN_MAX_ITERATIONS];     /* radians (0 for a refused step) */
    double stepTranslation[VH_ALIGN_MAX_ITERATIONS];  /* destination voxels */
    long long totals[32];       /* the last attempted step's 29 integer totals */
    long long stripes[VH_ALIGN_NUM_STRIPES * 32]; /* where the launch in flight adds; all zero between launches */
} VhAlignState;
/* what vh_scene_rep_align_scene takes: every field finite and positive, band <= VH_ALIGN_MOST_BAND, maxIterations <=
 * VH_ALIGN_MAX_ITERATIONS */
typedef struct VhAlignOptions {
    float band;             /* voxels: a voxel contributes while |sdf| <= band * voxel size, in both scenes (default 2) */
    float condThres;        /* the largest condition number of J^T J that is answered with a step (default 1e4) */
    double rotThres;        /* radians: converged when a step turns by less ... (default 1e-5) */
    double transThres;      /* destination voxels: ... and moves by less (default 1e-3) */
    uint32_t minCount;      /* the fewest contributing voxels that are answered with a step (default 200) */
    uint32_t maxIterations; /* launches enqueued (default 30) */
} VhAlignOptions;

/* DepthCameraData, DSC/DepthCameraUtil.h:17-159: the two image buffers the
 * path reads (the cudaArray/texture twins of the reference are not needed:
 * images are read with plain cached loads). */
typedef struct VhDepthCameraData {
    const float* d_depthData; /* [H*W] metres; invalid = -inf (MINF) or 0 */
    const float* d_colorData; /* [H*W*4] float4 rgba in [0,1]; invalid = MINF in .x; may be NULL */
} VhDepthCameraData;

/* RayCastData, DSC/RayCastSDFUtil.h:266-274: the four output maps. */
typedef struct VhRayCastData {
    float* d_depth;   /* [H*W]   */
    float* d_depth4;  /* [H*W*4] camera-space position, w=1 */
    float* d_normals; /* [H*W*4] */
    float* d_colors;  /* [H*W*4] */
} VhRayCastData;

/* SDFBlockDesc, DSC/CUDASceneRepChunkGrid.cu:13-16 / .h:24-51 (16 B):
 * streaming wire/disk unit, together with a 4096 B block of 512 voxels. */
/* ray-interval splatting (vh_ray_interval_splat): one entry of a tile's block list */
#define VH_TILE_LIST_CAPACITY 64        /* small tile tables (default) */
#define VH_TILE_LIST_CAPACITY_LARGE 128 /* large tile tables: fine voxels */
/* vh_query_rays: the most samples one ray may take; a ray that asks for more is refused (status 2) */
#define VH_QUERY_MAX_SAMPLES 65536
typedef struct VhTileBlock {
    int32_t pos[3]; /* SDF block position */
    int32_t ptr;    /* its voxel pointer (HashEntry::ptr) */
} VhTileBlock;

typedef struct VhSDFBlockDesc {
    int32_t pos[3];
    int32_t ptr;
} VhSDFBlockDesc;

/* MarchingCubesParams, DSC/MarchingCubesSDFUtil.h:9-23 (64 B; the reference's leading `bool` is the low byte of
 * m_boxEnabled, its padding the rest). */
typedef struct VhMarchingCubesParams {
    uint32_t m_boxEnabled;
    float m_minCorner[3];
    uint32_t m_maxNumTriangles;
    float m_maxCorner[3];
    uint32_t m_sdfBlockSize;
    uint32_t m_hashNumBuckets;
    uint32_t m_hashBucketSize;
    float m_threshMarchingCubes;
    float m_threshMarchingCubes2;
    float dummy[3];
} VhMarchingCubesParams;

/* MarchingCubesData::Vertex / ::Triangle, DSC/MarchingCubesSDFUtil.h:33-44 (24 B / 72 B) */
typedef struct VhVertex {
    float p[3];
    float c[3];
} VhVertex;
typedef struct VhTriangle {
    VhVertex v0, v1, v2;
} VhTriangle;

/* MarchingCubesData, DSC/MarchingCubesSDFUtil.h:27-326 (device buffers) */
typedef struct VhMarchingCubesData {
    VhMarchingCubesParams* d_params;
    uint32_t* d_numOccupiedBlocks;
    uint32_t* d_occupiedBlocks; /* hash entry indices, Ne of them */
    uint32_t* d_numTriangles;
    VhTriangle* d_triangles;    /* m_maxNumTriangles */
    uint8_t m_bIsOnGPU;
} VhMarchingCubesData;

/* Where a triangle of the soup came from (not in the reference; DESIGN.md section 4, "Indexed mesh"): the cell's voxel
 * coordinates and, for each of its three vertices, 8 bits of `edges`: bits 0-3 the edge 0..11 in the order of
 * vertlist (DSC/MarchingCubesSDFUtil.h:217-228), bits 4-5 the snap code of vertexInterp: 0 = interpolated,
 * 1 = returned at its first end point, 2 = at its second.  16 B. */
typedef struct VhTriangleSource {
    int32_t cell[3];
    uint32_t edges;
} VhTriangleSource;

/* status word of a weld (VhMeshWeldData::d_counts[2]) */
#define VH_WELD_TABLE_FULL 1u /* a vertex found no slot: the table has fewer slots than there are distinct keys */
#define VH_WELD_KEY_RANGE 2u  /* a lattice coordinate outside [-2^19, 2^19), or a malformed source record */

/* status word of the vertex-normal pass (vh_mesh_vertex_normals); either bit leaves every normal (0, 0, 0) */
#define VH_NORMALS_RANGE 1u     /* a scaled face normal is not finite or exceeds 2^40 in a component: scaleLog2 is too large */
#define VH_NORMALS_BAD_INDEX 2u /* a face index >= numVertices (nothing was read through it) */

/* status word of the component labelling (vh_mesh_components); either bit makes the filter keep nothing */
#define VH_COMPONENTS_BAD_INDEX 1u /* a face index >= numVertices (nothing was read through it; the face joins nothing) */
#define VH_COMPONENTS_STEPS 2u     /* a walk to a root took more steps than there are vertices (unreachable; defended) */
/* what vh_mesh_components_filter counts */
enum {
    VH_COMPONENTS_WITH_FACES = 0,     /* components of at least one face */
    VH_COMPONENTS_FACELESS = 1,       /* vertices that no in-range face names */
    VH_COMPONENTS_KEPT = 2,           /* components with a face that the filter kept */
    VH_COMPONENTS_KEPT_VERTICES = 3,
    VH_COMPONENTS_KEPT_FACES = 4,
    VH_COMPONENTS_LARGEST_FACES = 5,  /* faces of the largest component */
    VH_COMPONENTS_NUM_COUNTS = 6
};

/* status word of the vertex clustering (vh_mesh_cluster); any bit leaves the output empty and the other counts 0 */
#define VH_CLUSTER_TABLE_FULL 1u /* the cluster table or the face table has no free slot left */
#define VH_CLUSTER_BAD_KEY 2u    /* a vertex key with bit 62 or 63 set: no vertex key */
#define VH_CLUSTER_RANGE 4u      /* a scaled position or colour is not finite or exceeds 2^40 in a component: scaleLog2 is too large */
#define VH_CLUSTER_BAD_INDEX 8u  /* a face index >= numVertices (nothing was read through it; the face contributes nothing) */
#define VH_CLUSTER_MAX_CELLS 64u /* cellsPerCluster is 1 ... 64: a cluster then holds at most 2^20 keys and its sums stay below 2^60 */
/* what vh_mesh_cluster counts */
enum {
    VH_CLUSTER_VERTICES = 0,   /* vertices of the clustered mesh: the clusters that a kept face names */
    VH_CLUSTER_FACES = 1,      /* faces of the clustered mesh */
    VH_CLUSTER_STATUS = 2,
    VH_CLUSTER_COLLAPSED = 3,  /* faces dropped because two of their vertices fell into one cluster */
    VH_CLUSTER_DUPLICATES = 4, /* faces dropped because another face over the same three clusters was kept */
    VH_CLUSTER_UNUSED = 5,     /* clusters that no kept face names: they give no vertex */
    VH_CLUSTER_NUM_COUNTS = 6
};
/* Device buffers of the vertex clustering (vh_mesh_cluster): the caller's, sized for the mesh that goes in.  The
 * cluster table has 1 << m_clusterSlotsLog2 slots (at least twice the vertices), the face table 1 << m_faceSlotsLog2
 * (at least twice the faces); the launcher empties what it uses of them. */
typedef struct VhMeshClusterData {
    uint64_t* d_clusterKeys;   /* per cluster slot: the cluster key, all ones = empty */
    int64_t* d_clusterSums;    /* 6 per cluster slot: position and colour of the members in fixed point */
    uint32_t* d_clusterCount;  /* per cluster slot: its members */
    uint32_t* d_clusterIndex;  /* per cluster slot: named by a kept face (0 / 1), then its vertex in the output or all ones */
    uint32_t* d_vertexSlot;    /* per vertex of the input: its cluster's slot */
    uint64_t* d_facePairs;     /* per face slot: the two smaller cluster slots of the triple, all ones = empty */
    uint32_t* d_faceThirds;    /* per face slot: the largest cluster slot of the triple, all ones = empty */
    uint32_t* d_faceWindings;  /* per face slot: bit 0 / bit 1 = a face of this / the other winding fell here */
    uint32_t* d_work;          /* 2 words */
    VhVertex* d_vertices;      /* out: room for as many vertices as go in */
    uint64_t* d_keys;          /* out: the cluster keys of d_vertices */
    uint32_t* d_faces;         /* out: room for as many faces as go in */
    uint32_t* d_counts;        /* VH_CLUSTER_NUM_COUNTS words */
    uint32_t m_clusterSlotsLog2, m_faceSlotsLog2;
} VhMeshClusterData;

/* status word of the Taubin smoothing (vh_mesh_smooth); any bit leaves the output unwritten and the other counts 0 */
#define VH_SMOOTH_TABLE_FULL 1u /* the edge table has no free slot left */
#define VH_SMOOTH_RANGE 2u      /* a scaled position is not finite or exceeds 2^40 in a component, before or after a half step */
#define VH_SMOOTH_BAD_INDEX 4u  /* a face index >= numVertices (nothing was read through it; the face contributes nothing) */
#define VH_SMOOTH_DEGREE 8u     /* a vertex with more than VH_SMOOTH_MAX_DEGREE distinct neighbours */
#define VH_SMOOTH_MAX_DEGREE 65536u   /* 2^16 neighbours of at most 2^40 each: a sum stays below 2^56, sum - n q below 2^57 */
#define VH_SMOOTH_MAX_ITERATIONS 100u /* iterations are 1 ... 100; each is two half steps */
#define VH_SMOOTH_MAX_FACTOR_Q16 65536 /* |lambdaQ16|, |muQ16| <= 2^16: factors in [-1, 1] */
#define VH_SMOOTH_DEFAULT_LAMBDA_Q16 32768   /* 0.5 */
#define VH_SMOOTH_DEFAULT_MU_Q16 (-34734)    /* rint(-0.53 * 2^16) */
/* what vh_mesh_smooth counts */
enum {
    VH_SMOOTH_MOVED = 0,          /* vertices that the pass moves */
    VH_SMOOTH_BOUNDARY = 1,       /* vertices at an end of an edge that exactly one face names */
    VH_SMOOTH_ISOLATED = 2,       /* vertices without an edge */
    VH_SMOOTH_STATUS = 3,
    VH_SMOOTH_EDGES = 4,          /* distinct undirected edges */
    VH_SMOOTH_BOUNDARY_EDGES = 5, /* of them, those that exactly one face names */
    VH_SMOOTH_NUM_COUNTS = 6
};
/* Device buffers of the Taubin smoothing (vh_mesh_smooth): the caller's, sized for the mesh that goes in.  The edge
 * table has 1 << m_edgeSlotsLog2 slots (at least six times the faces: twice the edges at worst); the launcher empties
 * what it uses of it. */
typedef struct VhMeshSmoothData {
    uint64_t* d_edgeKeys;      /* per edge slot: lo | hi << 32 with lo < hi, all ones = empty */
    uint32_t* d_edgeUses;      /* per edge slot: the faces that name the edge */
    uint32_t* d_degree;        /* per vertex: its distinct neighbours */
    uint32_t* d_flags;         /* per vertex: a boundary vertex (0 / 1) from the degree pass; bit 1 = moves, from the prepare pass on */
    int64_t* d_positions;      /* 2 x 3 per vertex: the fixed-point positions, half step in and half step out */
    int64_t* d_sums;           /* 3 per vertex: the neighbours' positions summed */
    uint32_t* d_work;          /* 5 words */
    VhVertex* d_vertices;      /* out: as many vertices as go in */
    uint32_t* d_counts;        /* VH_SMOOTH_NUM_COUNTS words */
    uint32_t m_edgeSlotsLog2, m_pad;
} VhMeshSmoothData;

/* Device buffers of the weld (vh_mesh_weld): an open-addressing table of numSlots = 1 << m_slotsLog2 slots, and the
 * indexed mesh it produces.  Sized for m_maxTriangles triangles, that is 3 * m_maxTriangles vertices at worst. */
typedef struct VhMeshWeldData {
    uint64_t* d_slotKeys;    /* numSlots; all ones = empty */
    uint64_t* d_slotWinner;  /* numSlots; rank << 32 | soup vertex while inserting, then the slot's vertex index */
    uint32_t* d_vertexSlot;  /* 3 * m_maxTriangles: the slot of each soup vertex */
    uint32_t* d_counts;      /* {vertices, faces, status} */
    VhVertex* d_vertices;    /* 3 * m_maxTriangles */
    uint64_t* d_keys;        /* 3 * m_maxTriangles: the key of each welded vertex */
    uint32_t* d_faces;       /* 3 * m_maxTriangles: index triples */
    uint32_t m_maxTriangles;
    uint32_t m_slotsLog2;
} VhMeshWeldData;

/* What the accumulating weld (vh_mesh_weld_accum_*) reports: vertices, faces and the status word as the one-shot weld,
 * then the cells it took, the triangles it dropped because an earlier append had their cell, and the number of times
 * its table doubled (every doubling moves the keys: one rehash launch covers the doublings of one append). */
enum {
    VH_WELD_ACCUM_VERTICES = 0,
    VH_WELD_ACCUM_FACES = 1,
    VH_WELD_ACCUM_STATUS = 2,
    VH_WELD_ACCUM_CELLS = 3,
    VH_WELD_ACCUM_DROPPED = 4,
    VH_WELD_ACCUM_REHASHES = 5,
    VH_WELD_ACCUM_NUM_COUNTS = 6
};
/* appends between two vh_mesh_weld_accum_begin: a bid carries the append's ordinal above the rank and the soup index */
#define VH_WELD_ACCUM_MAX_APPENDS (1u << 28)

/* ---- live mesh (not in the reference; DESIGN.md section 4, "Live mesh") ----
 * status word of an update (vh_live_mesh_get_counts: out[VH_LIVE_NUM_COUNTS]); any bit leaves the cache and every record
 * invalid, so that the next update starts from nothing */
#define VH_LIVE_OVERFLOW 1u  /* more triangles than m_maxNumTriangles */
#define VH_LIVE_RANGE 2u     /* a resident block outside [-2^16, 2^16) in a coordinate: voxels outside [-2^19, 2^19) */
#define VH_LIVE_BAD_TABLE 4u /* an entry whose ptr names no block of the pool, or two entries with one block */
/* what an update counts */
enum {
    VH_LIVE_VISITED = 0,  /* resident entries */
    VH_LIVE_CHANGED = 1,  /* of them: no valid record, another position than the record's, or another digest */
    VH_LIVE_VANISHED = 2, /* positions that a valid record held and no longer holds: moved ids and ids not visited */
    VH_LIVE_REMESHED = 3, /* |R|: resident blocks within Chebyshev distance 1 of a changed or vanished position */
    VH_LIVE_DROPPED = 4,  /* cached triangles whose owner is not resident or lies in R */
    VH_LIVE_KEPT = 5,
    VH_LIVE_ADDED = 6,    /* triangles of the sourced pass 2 over R */
    VH_LIVE_TOTAL = 7,    /* kept + added */
    VH_LIVE_NUM_COUNTS = 8
};
/* one per heap block id (ptr / 512); epoch 0 = invalid.  24 B. */
typedef struct VhLiveMeshRecord {
    int32_t pos[3];
    uint32_t epoch;
    uint64_t digest;
} VhLiveMeshRecord;
/* Device buffers of the live mesh (vh_live_mesh_data_alloc) and, in the m_ fields, what the host remembers between
 * updates.  The cache itself is the VhMarchingCubesData's d_triangles and the records beside it; the spare pair is what
 * the drop pass compacts into, and changes places with them. */
typedef struct VhLiveMeshData {
    VhLiveMeshRecord* d_records;      /* m_numSDFBlocks */
    int32_t* d_positions;             /* C: {x, y, z, tag} per changed (0), moved-from (1) or abandoned (2) position, 2 m_numSDFBlocks of them */
    uint32_t* d_marks;                /* per heap block id: the epoch of the last update that had the block in R */
    uint32_t* d_remesh;               /* R: hash entry indices, m_numSDFBlocks */
    VhTriangle* d_spareTriangles;     /* m_maxNumTriangles */
    VhTriangleSource* d_spareSources; /* m_maxNumTriangles */
    uint32_t* d_counts;               /* 16 words: the VH_LIVE_NUM_COUNTS counts, the status, |C|, the triangles that went in */
    uint32_t m_numSDFBlocks, m_maxNumTriangles;
    uint32_t m_epoch;                 /* of the last update */
    uint32_t m_fresh;                 /* no update since the allocation or the last reset */
    uint32_t m_hashNumBuckets, m_hashMaxCollisionLinkedListSize; /* of the updates since then */
    float m_virtualVoxelSize;
    uint32_t m_pad;
} VhLiveMeshData;

/* The five GlobalAppState flags the reference host classes read
 * (DSC/CUDASceneRepHashSDF.h:249,251,329,331; DSC/CUDASceneRepChunkGrid.cpp:13). */
typedef struct VhSceneOptions {
    uint8_t s_offlineProcessing;        /* alloc until fixed point (host loop) */
    uint8_t s_garbageCollectionEnabled;
    uint8_t s_timingsDetailledEnabled;  /* record per-stage HIP events */
    uint8_t s_useReferenceLaunchSequence; /* not in the reference: 1 = run integrate / starve / identify /
                                             mutex reset / free as separate launches with host-side counts
                                             (the reference's sequence) instead of the fused kernel */
    uint32_t s_garbageCollectionStarve; /* starve every n-th frame */
    uint32_t s_streamingOutParts;
} VhSceneOptions;

/* alloc + compactify of one frame as a job (CUDASceneRepHashSDF::integrateAhead prepares it): whoever holds it may
 * launch the two passes -- CUDARayCastSDF::render does so INSIDE its own two launches (vh_render_intervals_co,
 * vh_compute_normals_co), CUDASceneRepHashSDF::integrateFinish launches whatever is still open. */
typedef struct VhFrameJob {
    VhHashData hashData;
    VhHashParams hashParams; /* with the frame's pose */
    VhDepthCameraData cam;
    VhDepthCameraParams cp;
    const uint32_t* d_bitMask;
    void* d_packedFrame;     /* width*height*8 bytes, written by the alloc pass (see vh_alloc_job), or NULL */
    int32_t lockToken;
    uint8_t allocLaunched, compactifyLaunched, pad0[2];
    uint32_t frameNumber; /* frames the scene had integrated when the job was made */
    uint32_t tableEpoch;  /* bumped by everything that edits the table outside integrate(): reset, streaming */
    /* The frame's pass over the voxels (integrate + starve + GC, vh_integrate_fused) as a third rider of computeNormals' launch:
     * its workgroups come last in the grid; they start when the launch's compactify workgroups have counted themselves off
     * (vh_compute_normals_co2).  Prepared by integrateAhead(); integrateFinish()
     * launches the pass itself if nobody did. */
    uint32_t* d_riderDone;   /* VH_RIDER_DONE_WORDS words (the scene's): the flags and counters of the compactify workgroups */
    uint32_t listDoneTotal, listClassTotal;   /* what their top counter / class counters read when every launch enqueued so far has finished (kept by the launcher) */
    uint32_t fusedFlags;     /* VH_FUSED_* of the frame's pass */
    int32_t fusedLockToken;
    uint32_t* d_countMirror; /* the scene's mapped {block count, frame number} words, or NULL */
    uint32_t mirrorTag;
    uint8_t fusedPrepared, fusedLaunched, pad1[2];
} VhFrameJob;
#define VH_RIDER_DONE_COUNTERS 32 /* copies of a flag, 128 bytes apart */
#define VH_RIDER_DONE_WORDS ((2 * VH_RIDER_DONE_COUNTERS + 1) * 32) /* flags, class counters, top counter */

/* The switches reconstruction() reads (DSC/DepthSensing.cpp:720-924) when it runs headless over a recorded sequence at
 * given poses (s_binaryDumpSensorUseTrajectory = true, s_binaryDumpSensorUseTrajectoryOnlyInit = false), plus what is
 * not in the reference: how far the host may run ahead of the device, and where the frames live. */
typedef struct VhReconstructionOptions {
    uint8_t s_streamingEnabled;   /* :881-900: stream out / in around the camera every frame (needs a chunk grid) */
    uint8_t s_integrationEnabled; /* :903-908: 0 = setLastRigidTransformAndCompactify instead of integrate */
    uint8_t s_offlineProcessing;  /* :885-891: streaming moves every part out and everything in range in, each frame */
    uint8_t s_renderEnabled;      /* 0 = skip the ray cast of the previous pose (:763) */
    uint8_t s_allocAhead;         /* not in the reference: alloc of frame k rides in the launch of the ray cast of pose k-1, compactify
                                     and the next pose's interval splat in computeNormals' (CUDASceneRepHashSDF::integrateAhead).
                                     With streaming on: in the frames whose streaming step is known a frame ahead to be a no-op
                                     (vh_stream_out_probe), and in frames where blocks only LEAVE (the pass runs behind the ray cast) */
    uint8_t s_framesOnHost;       /* not in the reference: VhSequenceFrame pointers are HOST memory (pinned for an
                                     asynchronous copy): float depth + RGBX bytes as a sensor delivers them
                                     (RGBDSensor::getDepthFloat / getColorRGBX); uploaded by two copy streams (depth, colour) into
                                     a ring of four staging slots, beside the previous frames' work */
    uint8_t pad0[2];
    uint32_t s_maxFramesInFlight; /* frames the host may enqueue ahead of the device (0 = no bound) */
    float s_streamingPos[3];      /* DSC/DepthSensing.cpp:1340-1355: in camera space */
    float s_streamingRadius;
} VhReconstructionOptions;

/* one frame of a recorded sequence */
typedef struct VhSequenceFrame {
    float rigidTransform[16]; /* camera-to-world pose of the trajectory; [0] = -inf or NaN marks an invalid frame (:738) */
    const float* depth;       /* width*height floats (device pointer, or host pointer with s_framesOnHost) */
    const void* color;        /* device: float4 per pixel (may be NULL); host: RGBX bytes, 4 per pixel */
} VhSequenceFrame;

/* Raw frames: what a sensor or a `.sens` recording delivers before SensorDataReader::processDepth and
 * CUDARGBDAdapter::process have touched it.  Set once, before the first frame (vh_reconstruction_set_raw_format); the
 * loop then makes d_depthData / d_colorData at adapter size (the VhDepthCameraParams it was created with) on the device
 * with vh_ingest_frame, and, when a filter is on, vh_gauss_filter_float_map / vh_gauss_filter_float4_map behind it, as
 * CUDARGBDSensor::process does (DSC/CUDARGBDSensor.cpp:159-186). */
typedef struct VhRawFrameFormat {
    uint32_t depthWidth, depthHeight; /* the sensor's depth image */
    uint32_t colorWidth, colorHeight; /* the sensor's colour image (ignored when colorChannels = 0) */
    float depthShift;                 /* depth in metres = sample / depthShift (ml::SensorData::m_depthShift: 1000 = millimetres) */
    uint32_t colorChannels;           /* 0: no colour, 3: RGB, 4: RGBX; bytes per pixel */
    uint8_t s_depthFilter, s_colorFilter, pad0[2];
    float s_depthSigmaD, s_depthSigmaR, s_colorSigmaD, s_colorSigmaR;
} VhRawFrameFormat;

/* one raw frame: s_framesOnHost says where the images live (host memory, pinned for an asynchronous copy; or device memory) */
typedef struct VhRawSequenceFrame {
    float rigidTransform[16]; /* as VhSequenceFrame's */
    const uint16_t* depth;    /* depthWidth*depthHeight samples; 0 = no measurement, which becomes 0.0f as in the reference */
    const uint8_t* color;     /* colorWidth*colorHeight*colorChannels bytes; may be NULL */
} VhRawSequenceFrame;

typedef struct VhReconstructionStats {
    uint64_t frames;             /* frames processed since creation / reset */
    uint64_t invalidFrames;      /* skipped: invalid pose */
    uint64_t blocksStreamedOut, blocksStreamedIn;
    double hostEnqueueSeconds;   /* host time inside run() spent enqueueing work (waits for the device excluded) */
    double hostWaitSeconds;      /* host time inside run() spent waiting: run-ahead bound, streaming read-backs */
    double uploadMs;             /* device time of the timed frame uploads: depth copy, colour copy and conversion (HIP events; the pair
                                    spans both copy streams) */
    uint64_t uploadsTimed;
    uint64_t uploadBytes;        /* bytes per frame upload */
    uint64_t streamingStepsSkipped; /* frames whose streaming step was known ahead to move nothing and that ran like a frame without streaming */
    uint64_t heapUnderflows;     /* the scene's status words as get_stats() found them (VH_STATE_*): alloc requests that found */
    uint64_t failedInserts;      /* the voxel pool empty; stream-in inserts that found no slot (the blocks went back to the host grid) */
    uint64_t framesWithRiders;   /* frames whose alloc pass rode in the ray caster's launch and whose compactify pass rode in computeNormals' */
    uint64_t splatsMadeAheadUsed; /* ray casts that ran on an interval splat made ahead (inside the previous computeNormals launch): such a
                                     frame is three launches -- k_render, k_compute_normals, k_integrate_fused -- or two (framesInTwoLaunches) */
    uint64_t streamingFramesPipelined; /* frames whose streaming step ran without a host wait (CUDASceneRepChunkGrid's pipeline: counts on the
                                          device, the chunk that comes in chosen a frame ahead); streamingStepsSkipped of them moved nothing */
    uint64_t framesInTwoLaunches; /* frames whose pass over the voxels rode in computeNormals' launch too (VhFrameJob::fusedLaunched): k_render and
                                     k_compute_normals are all the frame launches */
} VhReconstructionStats;

/* The GlobalAppState members (DSC/GlobalAppState.h:28-101) that the path reads, as filled from a zParameters*.txt
 * file by vh_app_state_read.  A key the file does not hold is value-initialised (0 / false), as readMembers() does
 * (DSC/GlobalAppState.h:139-142). */
typedef struct VhAppState {
    uint32_t s_adapterWidth, s_adapterHeight;
    float s_sensorDepthMax, s_sensorDepthMin;
    float s_SDFVoxelSize, s_SDFMarchingCubeThreshFactor, s_SDFTruncation, s_SDFTruncationScale, s_SDFMaxIntegrationDistance;
    uint32_t s_SDFIntegrationWeightSample, s_SDFIntegrationWeightMax;
    uint32_t s_hashNumBuckets, s_hashNumSDFBlocks, s_hashMaxCollisionLinkedListSize;
    float s_SDFRayIncrementFactor, s_SDFRayThresSampleDistFactor, s_SDFRayThresDistFactor;
    uint32_t s_SDFUseGradients;
    float s_depthSigmaD, s_depthSigmaR;
    uint32_t s_depthFilter;
    float s_colorSigmaD, s_colorSigmaR;
    uint32_t s_colorFilter;
    uint32_t s_integrationEnabled, s_trackingEnabled, s_timingsDetailledEnabled, s_timingsTotalEnabled;
    uint32_t s_garbageCollectionEnabled, s_garbageCollectionStarve;
    uint32_t s_marchingCubesMaxNumTriangles;
    uint32_t s_streamingEnabled;
    float s_streamingVoxelExtents[3];
    int32_t s_streamingGridDimensions[3];
    int32_t s_streamingMinGridPos[3];
    uint32_t s_streamingInitialChunkListSize;
    float s_streamingRadius;
    float s_streamingPos[3];
    uint32_t s_streamingOutParts;
    uint32_t s_offlineProcessing;
    uint32_t s_sensorIdx;
    /* recorded sequences: played when s_sensorIdx selects the SensorDataReader (DSC/GlobalAppState.h:51-53,80,95-98) */
    uint32_t s_binaryDumpSensorUseTrajectory, s_binaryDumpSensorUseTrajectoryOnlyInit;
    uint32_t s_playData, s_recordData, s_recordCompression, s_reconstructionEnabled;
    uint32_t s_numBinaryDumpSensorFiles; /* entries s_binaryDumpSensorFile[0..n) the file held, at most 8 kept */
    char s_binaryDumpSensorFile[8][256];
    char s_recordDataFile[256];
    uint32_t numKeysFound; /* how many of the members above the file held (the file list counts once) */
} VhAppState;

/* GlobalCameraTrackingState (DSC/GlobalCameraTrackingState.h:14-25), per pyramid level; from zParametersTracking*.txt */
#define VH_TRACKING_MAX_LEVELS 8
typedef struct VhTrackingState {
    uint32_t s_maxLevels;
    uint32_t s_maxOuterIter[VH_TRACKING_MAX_LEVELS];
    uint32_t s_maxInnerIter[VH_TRACKING_MAX_LEVELS];
    float s_distThres[VH_TRACKING_MAX_LEVELS];
    float s_normalThres[VH_TRACKING_MAX_LEVELS];
    float s_angleTransThres[VH_TRACKING_MAX_LEVELS];
    float s_distTransThres[VH_TRACKING_MAX_LEVELS];
    float s_residualEarlyOut[VH_TRACKING_MAX_LEVELS];
    uint32_t numLevelsFound; /* how many levels of s_maxOuterIter the file held */
} VhTrackingState;

/* The same plus the four per-level keys of the RGB-D tracker (DSC/GlobalCameraTrackingState.h:17-20); a key the file
 * does not hold takes setDefault's value (:67-71) on every level. */
typedef struct VhTrackingStateRGBD {
    VhTrackingState base;
    float s_weightsDepth[VH_TRACKING_MAX_LEVELS];
    float s_weightsColor[VH_TRACKING_MAX_LEVELS];
    float s_colorGradientMin[VH_TRACKING_MAX_LEVELS];
    float s_colorThres[VH_TRACKING_MAX_LEVELS];
} VhTrackingStateRGBD;

/* What one RGB-D build step needs besides the maps: CameraTrackingParameters (DSC/CameraTrackingInput.h:5-15) and the
 * level's intrinsics (fx, fy, mx, my divided by 2^level, DSC/CUDACameraTrackingMultiResRGBD.cpp:295-297). */
typedef struct VhIcpRGBDParams {
    float fx, fy, mx, my;
    float weightDepth, weightColor, distThres, normalThres;
    float sensorMaxDepth, colorGradientMin, colorThres;
    uint32_t level; /* picks the lane window: 12 at level 0, max(1, 12 / (4 level)) above (CUDABuildLinearSystemRGBD.cpp:31-32) */
} VhIcpRGBDParams;

/* Header of a recorded sequence (`.sens`, ml::SensorData, DSC/sensorData/sensorData.h:608-830): what
 * SensorDataReader::createFirstConnected hands to RGBDSensor::init and the intrinsics / extrinsics setters. */
typedef struct VhSensorDataInfo {
    uint32_t m_versionNumber;
    int32_t m_colorCompressionType; /* 0 raw, 1 PNG, 2 JPEG */
    int32_t m_depthCompressionType; /* 0 raw u16, 1 zlib u16, 2 uplink (refused) */
    uint32_t m_colorWidth, m_colorHeight, m_depthWidth, m_depthHeight;
    float m_depthShift; /* metres = sample / m_depthShift */
    uint64_t m_numFrames, m_numIMUFrames;
    float m_colorIntrinsic[16], m_colorExtrinsic[16], m_depthIntrinsic[16], m_depthExtrinsic[16];
    char m_sensorName[64];
} VhSensorDataInfo;

/* Device-resident state of one camera-tracking solve (vh_icp_*): the delta transform being refined and what the
 * reference keeps in LinearSystemConfidence (DSC/ICPErrorLog.h:16-58). */
typedef struct VhIcpState {
    float delta[16];        /* row-major; input points are moved by it */
    float lastError;        /* lastICPError of the current level (-1 at its start) */
    uint32_t done;          /* current level left its outer loop early (residual early-out) */
    uint32_t lost;          /* tracking lost: singular system or a step beyond the level's thresholds */
    float sumRegError;
    float sumRegWeight;
    uint32_t numCorr;
    float matrixCondition;
    uint32_t iterations;    /* linear systems solved so far */
    uint32_t pad[8];
} VhIcpState;

/* What the last vh_icp_step of a solve leaves in mapped host memory for a host that polls instead of copying: the
 * VhIcpState's result, then `tag` with a system-scope release store. */
typedef struct VhIcpResult {
    float delta[16];
    uint32_t lost;
    float sumRegError;
    float sumRegWeight;
    uint32_t numCorr;
    float matrixCondition;
    uint32_t iterations;
    uint32_t pad;
    uint32_t tag;
} VhIcpResult;

/* Device-resident state of one RGB-D solve (vh_icp_rgbd_*): a VhIcpState with the same meaning, plus the point the next
 * build step linearises at.  The reference recomputes both from deltaTransform before every build
 * (DSC/CUDACameraTrackingMultiResRGBD.cpp:204-208); here the solve step leaves them behind. */
typedef struct VhIcpStateRGBD {
    VhIcpState icp;
    float angles[3];      /* anglesOld = delta's rotation as eulerAngles(2, 1, 0): R = Rz(a0) Ry(a1) Rx(a2) */
    float translation[3]; /* translationOld = delta's translation column */
    uint32_t pad[2];
} VhIcpStateRGBD;

/* The rendering block of a zParameters*.txt (DSC/GlobalAppState.h:60-100, zParametersDefault.txt:69-109) as filled by
 * vh_read_render_state.  A key the file does not hold is value-initialised (0 / false / ""), as in VhAppState. */
typedef struct VhRenderState {
    float s_materialShininess;
    float s_materialAmbient[4], s_materialDiffuse[4], s_materialSpecular[4];
    float s_lightAmbient[4], s_lightDiffuse[4], s_lightSpecular[4];
    float s_lightDirection[3];
    uint32_t s_useColorForRendering;
    float s_renderingDepthDiscontinuityThresOffset, s_renderingDepthDiscontinuityThresLin;
    uint32_t s_renderToFile;
    char s_renderToFileDir[256];
    uint32_t numKeysFound; /* how many of the 13 members above the file held */
} VhRenderState;

/* The camera-calibration keys of a zParameters*.txt (DSC/GlobalAppState.h:82-85, zParametersDefault.txt:86-89) as
 * filled by vh_read_calibration_state.  Absent keys are value-initialised, as in VhAppState. */
typedef struct VhCalibrationState {
    uint32_t s_bUseCameraCalibration;
    float s_remappingDepthDiscontinuityThresOffset, s_remappingDepthDiscontinuityThresLin;
    uint32_t numKeysFound; /* how many of the 3 members above the file held */
} VhCalibrationState;

/* DX11PhongLighting::ConstantBufferLight (DSC/DX11PhongLighting.h:12-37), the light and material of k_phong. */
typedef struct VhPhongLight {
    float lightAmbient[4], lightDiffuse[4], lightSpecular[4];
    float lightDirection[3];
    float materialShininess;
    float materialAmbient[4], materialSpecular[4], materialDiffuse[4];
} VhPhongLight;

/* One RenderDepthMap call (DSC/DX11RGBDRenderer.h:197-275, cbRGBDRenderer of Shaders/RGBDRenderer.hlsl): the matrices
 * row-major as the host holds them (the shader's mul(v, M) is M v). */
typedef struct VhViewParams {
    float intrinsicInverse[16]; /* depth pixel * d -> camera */
    float modelview[16];        /* camera -> view */
    float intrinsicNew[16];     /* view -> screen pixels */
    uint32_t depthWidth, depthHeight, screenWidth, screenHeight;
    float depthThreshOffset, depthThreshLin;
    uint32_t pad[2];
} VhViewParams;

/* Error codes of the C ABI: 0 ok; <0 = -(hipError_t); >0 logical. */
enum {
    VH_OK = 0,
    VH_ERR_HEAP_EXHAUSTED = 1,
    VH_ERR_STAGING_OVERFLOW = 2,
    VH_ERR_INSERT_FAILED = 3,
    VH_ERR_BAD_ARGUMENT = 4,
    VH_ERR_VERSION_MISMATCH = 5,
    VH_ERR_IO = 6,
    VH_ERR_TIMEOUT = 7 /* the device made no progress for 30 s (hung or faulted): not a misuse.  Work may still be enqueued against the
                          caller's frame buffers: synchronize() or destroy the loop before freeing them */
};

#ifdef __cplusplus
}
#endif

#endif /* VH_TYPES_H */
