"""ctypes mirrors of include/vh_types.h plus the parameter builders of the
reference host classes.

Reference: HashParams  <- CUDASceneRepHashSDF::parametersFromGlobalAppState
           (DepthSensingCUDA/Source/CUDASceneRepHashSDF.h:38-58),
           RayCastParams <- CUDARayCastSDF::parametersFromGlobalAppState
           (DepthSensingCUDA/Source/CUDARayCastSDF.h:24-40),
           DepthCameraParams <- CUDARGBDSensor (CUDARGBDSensor.cpp:133-142).
"""
import ctypes as C

import numpy as np

SDF_BLOCK_SIZE = 8
SDF_BLOCK_VOXELS = 512
HASH_BUCKET_SIZE = 10
LOCK_ENTRY = -1
FREE_ENTRY = -2
STATE_WORDS = 16
STATE_HEAP_UNDERFLOW = 0
STATE_INSERT_FAILED = 1
STATE_ALLOC_LOCK_LOST = 2
STATE_RIDER_GAVE_UP = 3
QUERY_MAX_SAMPLES = 65536  # VH_QUERY_MAX_SAMPLES: the most samples one ray of vh_query_rays may take
QUERY_MISS, QUERY_HIT, QUERY_REFUSED = 0, 1, 2  # status bytes of vh_query_rays

MINF = np.float32(-np.inf)


class HashEntry(C.Structure):
    _fields_ = [("pos", C.c_int32 * 3), ("ptr", C.c_int32), ("offset", C.c_uint32), ("_pad", C.c_uint32 * 3)]


class Voxel(C.Structure):
    _fields_ = [("sdf", C.c_float), ("color", C.c_uint8 * 3), ("weight", C.c_uint8)]


class HashParams(C.Structure):
    _fields_ = [
        ("m_rigidTransform", C.c_float * 16),
        ("m_rigidTransformInverse", C.c_float * 16),
        ("m_hashNumBuckets", C.c_uint32),
        ("m_hashBucketSize", C.c_uint32),
        ("m_hashMaxCollisionLinkedListSize", C.c_uint32),
        ("m_numSDFBlocks", C.c_uint32),
        ("m_SDFBlockSize", C.c_int32),
        ("m_virtualVoxelSize", C.c_float),
        ("m_numOccupiedBlocks", C.c_uint32),
        ("m_maxIntegrationDistance", C.c_float),
        ("m_truncScale", C.c_float),
        ("m_truncation", C.c_float),
        ("m_integrationWeightSample", C.c_uint32),
        ("m_integrationWeightMax", C.c_uint32),
        ("m_streamingVoxelExtents", C.c_float * 3),
        ("m_streamingGridDimensions", C.c_int32 * 3),
        ("m_streamingMinGridPos", C.c_int32 * 3),
        ("m_streamingInitialChunkListSize", C.c_uint32),
        ("m_colorIntegration", C.c_uint32),   # 0: running 50/50 colour average (the reference), 1: weighted by the voxel weights
        ("m_dummy", C.c_uint32),
    ]


class DepthCameraParams(C.Structure):
    _fields_ = [
        ("fx", C.c_float), ("fy", C.c_float), ("mx", C.c_float), ("my", C.c_float),
        ("m_imageWidth", C.c_uint32), ("m_imageHeight", C.c_uint32),
        ("m_sensorDepthWorldMin", C.c_float), ("m_sensorDepthWorldMax", C.c_float),
    ]


class RayCastParams(C.Structure):
    _fields_ = [
        ("m_viewMatrix", C.c_float * 16),
        ("m_viewMatrixInverse", C.c_float * 16),
        ("m_intrinsics", C.c_float * 16),
        ("m_intrinsicsInverse", C.c_float * 16),
        ("m_width", C.c_uint32), ("m_height", C.c_uint32),
        ("m_numOccupiedSDFBlocks", C.c_uint32), ("m_maxNumVertices", C.c_uint32),
        ("m_splatMinimum", C.c_int32),
        ("m_minDepth", C.c_float), ("m_maxDepth", C.c_float), ("m_rayIncrement", C.c_float),
        ("m_thresSampleDist", C.c_float), ("m_thresDist", C.c_float),
        ("m_useGradients", C.c_uint8), ("_pad0", C.c_uint8 * 3),
        ("dummy0", C.c_uint32),
    ]


class HashData(C.Structure):
    _fields_ = [
        ("d_heap", C.c_void_p),
        ("d_heapCounter", C.c_void_p),
        ("d_hashDecision", C.c_void_p),
        ("d_hashDecisionPrefix", C.c_void_p),
        ("d_hash", C.c_void_p),
        ("d_hashCompactified", C.c_void_p),
        ("d_hashCompactifiedCounter", C.c_void_p),
        ("d_SDFBlocks", C.c_void_p),
        ("d_hashBucketMutex", C.c_void_p),
        ("m_bIsOnGPU", C.c_uint8), ("_pad0", C.c_uint8 * 7),
        ("d_bucketCount", C.c_void_p),
        ("d_bucketBits", C.c_void_p),
        ("d_state", C.c_void_p),
    ]


class DepthCameraData(C.Structure):
    _fields_ = [("d_depthData", C.c_void_p), ("d_colorData", C.c_void_p)]


class RayCastData(C.Structure):
    _fields_ = [("d_depth", C.c_void_p), ("d_depth4", C.c_void_p), ("d_normals", C.c_void_p), ("d_colors", C.c_void_p)]


class SDFBlockDesc(C.Structure):
    _fields_ = [("pos", C.c_int32 * 3), ("ptr", C.c_int32)]


class MarchingCubesParams(C.Structure):
    _fields_ = [
        ("m_boxEnabled", C.c_uint32), ("m_minCorner", C.c_float * 3),
        ("m_maxNumTriangles", C.c_uint32), ("m_maxCorner", C.c_float * 3),
        ("m_sdfBlockSize", C.c_uint32), ("m_hashNumBuckets", C.c_uint32), ("m_hashBucketSize", C.c_uint32),
        ("m_threshMarchingCubes", C.c_float), ("m_threshMarchingCubes2", C.c_float), ("dummy", C.c_float * 3),
    ]


class MarchingCubesData(C.Structure):
    _fields_ = [
        ("d_params", C.c_void_p), ("d_numOccupiedBlocks", C.c_void_p), ("d_occupiedBlocks", C.c_void_p),
        ("d_numTriangles", C.c_void_p), ("d_triangles", C.c_void_p), ("m_bIsOnGPU", C.c_uint8),
    ]


# MarchingCubesData::Triangle = 3 x {float3 p, float3 c} (72 B)
TRIANGLE_DTYPE = np.dtype([("v", [("p", np.float32, 3), ("c", np.float32, 3)], 3)])
VERTEX_DTYPE = np.dtype([("p", np.float32, 3), ("c", np.float32, 3)])


class TriangleSource(C.Structure):
    """VhTriangleSource: where a triangle of the soup came from (16 B)"""
    _fields_ = [("cell", C.c_int32 * 3), ("edges", C.c_uint32)]


# edges: 8 bits per vertex, bits 0-3 the edge 0..11 (vertlist order), bits 4-5 the snap code 0 / 1 / 2
TRIANGLE_SOURCE_DTYPE = np.dtype([("cell", np.int32, 3), ("edges", np.uint32)])
WELD_TABLE_FULL, WELD_KEY_RANGE = 1, 2  # bits of the weld's status word
NORMALS_RANGE, NORMALS_BAD_INDEX = 1, 2  # bits of the vertex-normal pass's status word (VH_NORMALS_*)
COMPONENTS_BAD_INDEX, COMPONENTS_STEPS = 1, 2  # bits of the component labelling's status word (VH_COMPONENTS_*)
# VH_COMPONENTS_*: what the component filter counts
COMPONENTS_COUNTS = ("components", "faceless_vertices", "kept_components", "kept_vertices", "kept_faces", "largest_faces")
# VH_CLUSTER_*: bits of the vertex clustering's status word, the limit of cellsPerCluster, what the pass counts
CLUSTER_TABLE_FULL, CLUSTER_BAD_KEY, CLUSTER_RANGE, CLUSTER_BAD_INDEX = 1, 2, 4, 8
CLUSTER_MAX_CELLS = 64
CLUSTER_COUNTS = ("vertices", "faces", "status", "collapsed", "duplicates", "unused_clusters")


class MeshClusterData(C.Structure):  # VhMeshClusterData
    _fields_ = [(n, C.c_void_p) for n in ("d_clusterKeys", "d_clusterSums", "d_clusterCount", "d_clusterIndex", "d_vertexSlot", "d_facePairs", "d_faceThirds",
                                         "d_faceWindings", "d_work", "d_vertices", "d_keys", "d_faces", "d_counts")] + \
               [("m_clusterSlotsLog2", C.c_uint32), ("m_faceSlotsLog2", C.c_uint32)]


# VH_SMOOTH_*: bits of the Taubin smoothing's status word, its limits and defaults, what the pass counts
SMOOTH_TABLE_FULL, SMOOTH_RANGE, SMOOTH_BAD_INDEX, SMOOTH_DEGREE = 1, 2, 4, 8
SMOOTH_MAX_DEGREE, SMOOTH_MAX_ITERATIONS, SMOOTH_MAX_FACTOR_Q16 = 1 << 16, 100, 1 << 16
SMOOTH_DEFAULT_LAMBDA_Q16, SMOOTH_DEFAULT_MU_Q16 = 32768, -34734
SMOOTH_COUNTS = ("moved", "boundary_vertices", "isolated_vertices", "status", "edges", "boundary_edges")
# VH_MERGE_*: bits of the scene merge's status word, what the call counts
MERGE_HEAP_SHORT, MERGE_NO_SLOT, MERGE_NOT_SETTLED = 1, 2, 4
MERGE_COUNTS = ("source_blocks", "present", "allocated", "left_out", "combined", "copied", "alloc_passes", "status")
# VH_RESAMPLE_*: bits of the resampled merge's status word, what vh_resample_blocks counts
RESAMPLE_OUT_OF_RANGE, RESAMPLE_TABLE_FULL = 1, 2
RESAMPLE_COUNTS = ("source_blocks", "candidates", "staged", "observed", "status")
# VH_CUT_*: the scene cut's shapes, flags, bits of its status word, what vh_cut_blocks counts
CUT_BOX, CUT_ELLIPSOID = 0, 1
CUT_SELECT_OUTSIDE, CUT_LIFT, CUT_KEEP, CUT_COUNT_ONLY = 1, 2, 4, 8
CUT_STAGING_SHORT, CUT_NOT_SETTLED = 1, 2
CUT_COUNTS = ("blocks_in", "touched", "freed", "lifted", "voxels_erased", "voxels_lifted", "delete_passes", "unsettled", "status")

# VH_DEINT_*: the frame de-integration's flag, the bit of its status word, what vh_deintegrate_blocks counts
DEINT_COUNT_ONLY = 1
DEINT_NOT_SETTLED = 1
DEINT_COUNTS = ("blocks_in", "processed", "changed", "freed", "voxels_changed", "voxels_reset", "voxels_at_cap", "delete_passes", "unsettled", "status")

# VH_ALIGN_*: bits of the scene registration's status word, its limits, the places of its 29 totals
ALIGN_CONVERGED, ALIGN_TOO_FEW, ALIGN_ILL_CONDITIONED, ALIGN_OUT_OF_RANGE, ALIGN_TOO_MANY, ALIGN_ITERATIONS_SPENT = 1, 2, 4, 8, 16, 32
ALIGN_MAX_ITERATIONS, ALIGN_MOST_BLOCKS, ALIGN_MOST_BAND, ALIGN_QUANTUM_LOG2, ALIGN_NUM_STRIPES = 64, 1 << 19, 4.0, 26, 32
ALIGN_JTJ, ALIGN_JTE, ALIGN_EE, ALIGN_COUNT, ALIGN_NUM_TERMS = 0, 21, 27, 28, 29
ALIGN_RULE_WORDS = 37  # vh_debug_align_rule's record: kept, q[3], e, g[3], the 29 float terms


class AlignState(C.Structure):  # VhAlignState
    _fields_ = [
        ("dstFromSrc", C.c_double * 16), ("srcVoxFromDstVox", C.c_float * 12), ("dstVoxFromSrcVox", C.c_float * 12),
        ("pivot", C.c_float * 3), ("invRadius", C.c_float), ("vsSrc", C.c_float), ("vsDst", C.c_float),
        ("iterations", C.c_uint32), ("status", C.c_uint32), ("raised", C.c_uint32), ("reserved", C.c_uint32),
        ("count", C.c_uint32 * ALIGN_MAX_ITERATIONS), ("condition", C.c_float * ALIGN_MAX_ITERATIONS),
        ("sumSquares", C.c_double * ALIGN_MAX_ITERATIONS), ("stepRotation", C.c_double * ALIGN_MAX_ITERATIONS),
        ("stepTranslation", C.c_double * ALIGN_MAX_ITERATIONS),
        ("totals", C.c_longlong * 32), ("stripes", C.c_longlong * (ALIGN_NUM_STRIPES * 32)),
    ]


class AlignOptions(C.Structure):  # VhAlignOptions
    _fields_ = [("band", C.c_float), ("condThres", C.c_float), ("rotThres", C.c_double), ("transThres", C.c_double),
                ("minCount", C.c_uint32), ("maxIterations", C.c_uint32)]


def make_align_options(band=2.0, cond_thres=1e4, rot_thres=1e-5, trans_thres=1e-3, min_count=200, max_iterations=30):
    """the defaults of CUDASceneRepHashSDF::AlignOptions (include/vh.hpp)"""
    return AlignOptions(float(band), float(cond_thres), float(rot_thres), float(trans_thres), int(min_count), int(max_iterations))


def align_state_dict(st):
    """an AlignState as plain Python: the pose [4, 4], the matrices [3, 4], the status, and the per-step records cut to
    the steps attempted"""
    import numpy as np
    k = int(st.iterations)
    return dict(
        dst_from_src=np.array(st.dstFromSrc[:], np.float64).reshape(4, 4),
        src_vox_from_dst_vox=np.array(st.srcVoxFromDstVox[:], np.float32).reshape(3, 4),
        dst_vox_from_src_vox=np.array(st.dstVoxFromSrcVox[:], np.float32).reshape(3, 4),
        pivot=np.array(st.pivot[:], np.float32), inv_radius=float(st.invRadius), iterations=k, status=int(st.status),
        converged=bool(st.status & ALIGN_CONVERGED),
        count=[int(v) for v in st.count[:k]], condition=[float(v) for v in st.condition[:k]], sum_squares=[float(v) for v in st.sumSquares[:k]],
        step_rotation=[float(v) for v in st.stepRotation[:k]], step_translation=[float(v) for v in st.stepTranslation[:k]],
        totals=np.array(st.totals[:ALIGN_NUM_TERMS], np.int64), raw=bytes(st))


class CutRegion(C.Structure):  # VhCutRegion
    _fields_ = [("worldFromRegion", C.c_double * 16), ("halfExtents", C.c_float * 3), ("shape", C.c_uint32)]


def make_cut_region(centre=(0.0, 0.0, 0.0), half_extents=(1.0, 1.0, 1.0), rotation=None, shape=CUT_BOX, world_from_region=None):
    """a box or an ellipsoid in the world: its centre and half extents in metres, its axes the columns of `rotation`
    (3x3, default the world's); or its whole frame as a rigid 4x4 world_from_region"""
    import numpy as np
    m = np.eye(4)
    if world_from_region is not None:
        m = np.asarray(world_from_region, np.float64).reshape(4, 4)
    else:
        if rotation is not None:
            m[:3, :3] = np.asarray(rotation, np.float64).reshape(3, 3)
        m[:3, 3] = centre
    r = CutRegion()
    r.worldFromRegion[:] = [float(v) for v in m.reshape(16)]
    r.halfExtents[:] = [float(v) for v in half_extents]
    r.shape = int(shape)
    return r


class MeshSmoothData(C.Structure):  # VhMeshSmoothData
    _fields_ = [(n, C.c_void_p) for n in ("d_edgeKeys", "d_edgeUses", "d_degree", "d_flags", "d_positions", "d_sums", "d_work", "d_vertices", "d_counts")] + \
               [("m_edgeSlotsLog2", C.c_uint32), ("m_pad", C.c_uint32)]


def smooth_factor_q16(f):
    """a smoothing factor in units of 2^-16, by rint; ValueError above 1 in magnitude"""
    if not abs(float(f)) <= 1.0:
        raise ValueError("a smoothing factor lies in [-1, 1]")
    return int(np.rint(np.float64(np.float32(f)) * 65536.0))


WELD_ACCUM_COUNTS = ("vertices", "faces", "status", "cells", "dropped", "rehashes")  # VH_WELD_ACCUM_*: what the accumulating weld reports
WELD_ACCUM_MAX_APPENDS = 1 << 28


class MeshWeldData(C.Structure):
    _fields_ = [
        ("d_slotKeys", C.c_void_p), ("d_slotWinner", C.c_void_p), ("d_vertexSlot", C.c_void_p), ("d_counts", C.c_void_p),
        ("d_vertices", C.c_void_p), ("d_keys", C.c_void_p), ("d_faces", C.c_void_p),
        ("m_maxTriangles", C.c_uint32), ("m_slotsLog2", C.c_uint32),
    ]


# VH_LIVE_*: what an update of the live mesh counts (the status word follows them), and the bits of that word
LIVE_COUNTS = ("visited", "changed", "vanished", "remeshed", "dropped", "kept", "added", "total")
LIVE_OVERFLOW, LIVE_RANGE, LIVE_BAD_TABLE = 1, 2, 4
LIVE_RECORD_DTYPE = np.dtype([("pos", np.int32, 3), ("epoch", np.uint32), ("digest", np.uint64)])  # VhLiveMeshRecord, 24 B


class LiveMeshData(C.Structure):  # VhLiveMeshData
    _fields_ = [
        ("d_records", C.c_void_p), ("d_positions", C.c_void_p), ("d_marks", C.c_void_p), ("d_remesh", C.c_void_p),
        ("d_spareTriangles", C.c_void_p), ("d_spareSources", C.c_void_p), ("d_counts", C.c_void_p),
        ("m_numSDFBlocks", C.c_uint32), ("m_maxNumTriangles", C.c_uint32), ("m_epoch", C.c_uint32), ("m_fresh", C.c_uint32),
        ("m_hashNumBuckets", C.c_uint32), ("m_hashMaxCollisionLinkedListSize", C.c_uint32), ("m_virtualVoxelSize", C.c_float),
        ("m_pad", C.c_uint32),
    ]


class AppState(C.Structure):
    _fields_ = [
        ("s_adapterWidth", C.c_uint32), ("s_adapterHeight", C.c_uint32),
        ("s_sensorDepthMax", C.c_float), ("s_sensorDepthMin", C.c_float),
        ("s_SDFVoxelSize", C.c_float), ("s_SDFMarchingCubeThreshFactor", C.c_float), ("s_SDFTruncation", C.c_float),
        ("s_SDFTruncationScale", C.c_float), ("s_SDFMaxIntegrationDistance", C.c_float),
        ("s_SDFIntegrationWeightSample", C.c_uint32), ("s_SDFIntegrationWeightMax", C.c_uint32),
        ("s_hashNumBuckets", C.c_uint32), ("s_hashNumSDFBlocks", C.c_uint32), ("s_hashMaxCollisionLinkedListSize", C.c_uint32),
        ("s_SDFRayIncrementFactor", C.c_float), ("s_SDFRayThresSampleDistFactor", C.c_float), ("s_SDFRayThresDistFactor", C.c_float),
        ("s_SDFUseGradients", C.c_uint32),
        ("s_depthSigmaD", C.c_float), ("s_depthSigmaR", C.c_float), ("s_depthFilter", C.c_uint32),
        ("s_colorSigmaD", C.c_float), ("s_colorSigmaR", C.c_float), ("s_colorFilter", C.c_uint32),
        ("s_integrationEnabled", C.c_uint32), ("s_trackingEnabled", C.c_uint32), ("s_timingsDetailledEnabled", C.c_uint32),
        ("s_timingsTotalEnabled", C.c_uint32), ("s_garbageCollectionEnabled", C.c_uint32), ("s_garbageCollectionStarve", C.c_uint32),
        ("s_marchingCubesMaxNumTriangles", C.c_uint32), ("s_streamingEnabled", C.c_uint32),
        ("s_streamingVoxelExtents", C.c_float * 3), ("s_streamingGridDimensions", C.c_int32 * 3), ("s_streamingMinGridPos", C.c_int32 * 3),
        ("s_streamingInitialChunkListSize", C.c_uint32), ("s_streamingRadius", C.c_float), ("s_streamingPos", C.c_float * 3),
        ("s_streamingOutParts", C.c_uint32), ("s_offlineProcessing", C.c_uint32), ("s_sensorIdx", C.c_uint32),
        ("s_binaryDumpSensorUseTrajectory", C.c_uint32), ("s_binaryDumpSensorUseTrajectoryOnlyInit", C.c_uint32),
        ("s_playData", C.c_uint32), ("s_recordData", C.c_uint32), ("s_recordCompression", C.c_uint32), ("s_reconstructionEnabled", C.c_uint32),
        ("s_numBinaryDumpSensorFiles", C.c_uint32), ("s_binaryDumpSensorFile", (C.c_char * 256) * 8), ("s_recordDataFile", C.c_char * 256),
        ("numKeysFound", C.c_uint32),
    ]


class SensorDataInfo(C.Structure):
    """VhSensorDataInfo: the header of a `.sens` sequence"""
    _fields_ = [
        ("m_versionNumber", C.c_uint32), ("m_colorCompressionType", C.c_int32), ("m_depthCompressionType", C.c_int32),
        ("m_colorWidth", C.c_uint32), ("m_colorHeight", C.c_uint32), ("m_depthWidth", C.c_uint32), ("m_depthHeight", C.c_uint32),
        ("m_depthShift", C.c_float), ("m_numFrames", C.c_uint64), ("m_numIMUFrames", C.c_uint64),
        ("m_colorIntrinsic", C.c_float * 16), ("m_colorExtrinsic", C.c_float * 16),
        ("m_depthIntrinsic", C.c_float * 16), ("m_depthExtrinsic", C.c_float * 16), ("m_sensorName", C.c_char * 64),
    ]


class TrackingState(C.Structure):
    _fields_ = [
        ("s_maxLevels", C.c_uint32), ("s_maxOuterIter", C.c_uint32 * 8), ("s_maxInnerIter", C.c_uint32 * 8),
        ("s_distThres", C.c_float * 8), ("s_normalThres", C.c_float * 8), ("s_angleTransThres", C.c_float * 8),
        ("s_distTransThres", C.c_float * 8), ("s_residualEarlyOut", C.c_float * 8), ("numLevelsFound", C.c_uint32),
    ]


class IcpState(C.Structure):
    _fields_ = [
        ("delta", C.c_float * 16), ("lastError", C.c_float), ("done", C.c_uint32), ("lost", C.c_uint32),
        ("sumRegError", C.c_float), ("sumRegWeight", C.c_float), ("numCorr", C.c_uint32), ("matrixCondition", C.c_float),
        ("iterations", C.c_uint32), ("pad", C.c_uint32 * 8),
    ]


class IcpResult(C.Structure):
    """VhIcpResult: what the last vh_icp_step of a solve leaves in mapped host memory, the tag last"""
    _fields_ = [
        ("delta", C.c_float * 16), ("lost", C.c_uint32), ("sumRegError", C.c_float), ("sumRegWeight", C.c_float), ("numCorr", C.c_uint32),
        ("matrixCondition", C.c_float), ("iterations", C.c_uint32), ("pad", C.c_uint32), ("tag", C.c_uint32),
    ]


class TrackingStateRGBD(C.Structure):
    """VhTrackingStateRGBD: the f5 settings plus the four per-level keys of the RGB-D tracker"""
    _fields_ = [
        ("base", TrackingState), ("s_weightsDepth", C.c_float * 8), ("s_weightsColor", C.c_float * 8),
        ("s_colorGradientMin", C.c_float * 8), ("s_colorThres", C.c_float * 8),
    ]


class IcpRGBDParams(C.Structure):
    _fields_ = [
        ("fx", C.c_float), ("fy", C.c_float), ("mx", C.c_float), ("my", C.c_float),
        ("weightDepth", C.c_float), ("weightColor", C.c_float), ("distThres", C.c_float), ("normalThres", C.c_float),
        ("sensorMaxDepth", C.c_float), ("colorGradientMin", C.c_float), ("colorThres", C.c_float), ("level", C.c_uint32),
    ]


class IcpStateRGBD(C.Structure):
    _fields_ = [("icp", IcpState), ("angles", C.c_float * 3), ("translation", C.c_float * 3), ("pad", C.c_uint32 * 2)]


class RenderState(C.Structure):
    """VhRenderState: the rendering block of a zParameters*.txt"""
    _fields_ = [
        ("s_materialShininess", C.c_float), ("s_materialAmbient", C.c_float * 4), ("s_materialDiffuse", C.c_float * 4),
        ("s_materialSpecular", C.c_float * 4), ("s_lightAmbient", C.c_float * 4), ("s_lightDiffuse", C.c_float * 4),
        ("s_lightSpecular", C.c_float * 4), ("s_lightDirection", C.c_float * 3), ("s_useColorForRendering", C.c_uint32),
        ("s_renderingDepthDiscontinuityThresOffset", C.c_float), ("s_renderingDepthDiscontinuityThresLin", C.c_float),
        ("s_renderToFile", C.c_uint32), ("s_renderToFileDir", C.c_char * 256), ("numKeysFound", C.c_uint32),
    ]


class CalibrationState(C.Structure):
    """VhCalibrationState: the camera-calibration keys of a zParameters*.txt"""
    _fields_ = [
        ("s_bUseCameraCalibration", C.c_uint32), ("s_remappingDepthDiscontinuityThresOffset", C.c_float),
        ("s_remappingDepthDiscontinuityThresLin", C.c_float), ("numKeysFound", C.c_uint32),
    ]


class PhongLight(C.Structure):
    """VhPhongLight: DX11PhongLighting::ConstantBufferLight"""
    _fields_ = [
        ("lightAmbient", C.c_float * 4), ("lightDiffuse", C.c_float * 4), ("lightSpecular", C.c_float * 4),
        ("lightDirection", C.c_float * 3), ("materialShininess", C.c_float),
        ("materialAmbient", C.c_float * 4), ("materialSpecular", C.c_float * 4), ("materialDiffuse", C.c_float * 4),
    ]


class ViewParams(C.Structure):
    """VhViewParams: one RenderDepthMap call (matrices row-major)"""
    _fields_ = [
        ("intrinsicInverse", C.c_float * 16), ("modelview", C.c_float * 16), ("intrinsicNew", C.c_float * 16),
        ("depthWidth", C.c_uint32), ("depthHeight", C.c_uint32), ("screenWidth", C.c_uint32), ("screenHeight", C.c_uint32),
        ("depthThreshOffset", C.c_float), ("depthThreshLin", C.c_float), ("pad", C.c_uint32 * 2),
    ]


def make_view_params(intrinsic_inverse, modelview, intrinsic_new, depth_size, screen_size, thres_offset=0.012, thres_lin=0.001):
    p = ViewParams()
    for name, m in (("intrinsicInverse", intrinsic_inverse), ("modelview", modelview), ("intrinsicNew", intrinsic_new)):
        getattr(p, name)[:] = [float(v) for v in np.asarray(m, dtype=np.float32).reshape(16)]
    p.depthWidth, p.depthHeight = depth_size
    p.screenWidth, p.screenHeight = screen_size
    p.depthThreshOffset, p.depthThreshLin = thres_offset, thres_lin
    return p


def make_tracking_state(levels=3, outer=(8, 6, 4), inner=(1, 1, 1), dist=0.15, normal=0.97, angle_trans=1.0, dist_trans=1.0, early_out=0.01):
    """the reference's zParametersTrackingDefault.txt"""
    t = TrackingState()
    t.s_maxLevels = levels
    for i in range(levels):
        t.s_maxOuterIter[i] = outer[i]
        t.s_maxInnerIter[i] = inner[i]
        t.s_distThres[i], t.s_normalThres[i] = dist, normal
        t.s_angleTransThres[i], t.s_distTransThres[i], t.s_residualEarlyOut[i] = angle_trans, dist_trans, early_out
    t.numLevelsFound = levels
    return t


def make_tracking_state_rgbd(levels=3, weights_depth=(1.0, 0.5, 0.5), weights_color=(0.0, 0.5, 0.5), color_gradient_min=0.005, color_thres=0.1, **f5):
    """the reference's zParametersTrackingDefault.txt with its colour keys (colour weight 0 on level 0, 0.5 above);
    the f5 keys as make_tracking_state takes them"""
    t = TrackingStateRGBD()
    t.base = make_tracking_state(levels, **f5)
    for i in range(8):  # VH_TRACKING_MAX_LEVELS; setDefault (DSC/GlobalCameraTrackingState.h:67-71) beyond the levels given
        t.s_weightsDepth[i], t.s_weightsColor[i], t.s_colorGradientMin[i], t.s_colorThres[i] = 1.0, 1.0, 0.005, 0.1
    for i in range(levels):
        t.s_weightsDepth[i], t.s_weightsColor[i] = weights_depth[i], weights_color[i]
        t.s_colorGradientMin[i], t.s_colorThres[i] = color_gradient_min, color_thres
    return t


class SceneOptions(C.Structure):
    _fields_ = [
        ("s_offlineProcessing", C.c_uint8),
        ("s_garbageCollectionEnabled", C.c_uint8),
        ("s_timingsDetailledEnabled", C.c_uint8),
        ("s_useReferenceLaunchSequence", C.c_uint8),
        ("s_garbageCollectionStarve", C.c_uint32),
        ("s_streamingOutParts", C.c_uint32),
    ]


class FrameJob(C.Structure):
    _fields_ = [
        ("hashData", HashData),
        ("hashParams", HashParams),
        ("cam", DepthCameraData),
        ("cp", DepthCameraParams),
        ("d_bitMask", C.c_void_p),
        ("d_packedFrame", C.c_void_p),
        ("lockToken", C.c_int32),
        ("allocLaunched", C.c_uint8),
        ("compactifyLaunched", C.c_uint8),
        ("pad0", C.c_uint8 * 2),
        ("frameNumber", C.c_uint32),
        ("tableEpoch", C.c_uint32),
        ("d_riderDone", C.c_void_p),
        ("listDoneTotal", C.c_uint32),
        ("listClassTotal", C.c_uint32),
        ("fusedFlags", C.c_uint32),
        ("fusedLockToken", C.c_int32),
        ("d_countMirror", C.c_void_p),
        ("mirrorTag", C.c_uint32),
        ("fusedPrepared", C.c_uint8),
        ("fusedLaunched", C.c_uint8),
        ("pad1", C.c_uint8 * 2),
    ]


class ReconstructionOptions(C.Structure):
    _fields_ = [
        ("s_streamingEnabled", C.c_uint8),
        ("s_integrationEnabled", C.c_uint8),
        ("s_offlineProcessing", C.c_uint8),
        ("s_renderEnabled", C.c_uint8),
        ("s_allocAhead", C.c_uint8),
        ("s_framesOnHost", C.c_uint8),
        ("pad0", C.c_uint8 * 2),
        ("s_maxFramesInFlight", C.c_uint32),
        ("s_streamingPos", C.c_float * 3),
        ("s_streamingRadius", C.c_float),
    ]


class SequenceFrame(C.Structure):
    _fields_ = [("rigidTransform", C.c_float * 16), ("depth", C.c_void_p), ("color", C.c_void_p)]


class RawFrameFormat(C.Structure):
    """VhRawFrameFormat: what the raw frames of a native loop look like (set once, before the first frame)"""
    _fields_ = [
        ("depthWidth", C.c_uint32), ("depthHeight", C.c_uint32),
        ("colorWidth", C.c_uint32), ("colorHeight", C.c_uint32),
        ("depthShift", C.c_float),
        ("colorChannels", C.c_uint32),
        ("s_depthFilter", C.c_uint8), ("s_colorFilter", C.c_uint8), ("pad0", C.c_uint8 * 2),
        ("s_depthSigmaD", C.c_float), ("s_depthSigmaR", C.c_float), ("s_colorSigmaD", C.c_float), ("s_colorSigmaR", C.c_float),
    ]


class RawSequenceFrame(C.Structure):
    """VhRawSequenceFrame: pose, u16 depth, RGB / RGBX bytes"""
    _fields_ = [("rigidTransform", C.c_float * 16), ("depth", C.c_void_p), ("color", C.c_void_p)]


class ReconstructionStats(C.Structure):
    _fields_ = [
        ("frames", C.c_uint64),
        ("invalidFrames", C.c_uint64),
        ("blocksStreamedOut", C.c_uint64),
        ("blocksStreamedIn", C.c_uint64),
        ("hostEnqueueSeconds", C.c_double),
        ("hostWaitSeconds", C.c_double),
        ("uploadMs", C.c_double),
        ("uploadsTimed", C.c_uint64),
        ("uploadBytes", C.c_uint64),
        ("streamingStepsSkipped", C.c_uint64),
        ("heapUnderflows", C.c_uint64),
        ("failedInserts", C.c_uint64),
        ("framesWithRiders", C.c_uint64),
        ("splatsMadeAheadUsed", C.c_uint64),
        ("streamingFramesPipelined", C.c_uint64),
        ("framesInTwoLaunches", C.c_uint64),
    ]


assert C.sizeof(HashEntry) == 32
assert C.sizeof(Voxel) == 8
assert C.sizeof(HashParams) == 224
assert C.sizeof(DepthCameraParams) == 32
assert C.sizeof(RayCastParams) == 304
assert C.sizeof(SDFBlockDesc) == 16

# numpy views of the same layouts (for downloads)
HASH_ENTRY_DTYPE = np.dtype([("pos", np.int32, 3), ("ptr", np.int32), ("offset", np.uint32), ("_pad", np.uint32, 3)])
VOXEL_DTYPE = np.dtype([("sdf", np.float32), ("color", np.uint8, 3), ("weight", np.uint8)])
DESC_DTYPE = np.dtype([("pos", np.int32, 3), ("ptr", np.int32)])
assert HASH_ENTRY_DTYPE.itemsize == 32 and VOXEL_DTYPE.itemsize == 8 and DESC_DTYPE.itemsize == 16

IDENTITY16 = (1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0)


def mat16(m):
    """row-major 4x4 -> (c_float*16)"""
    a = np.asarray(m, dtype=np.float32).reshape(16)
    return (C.c_float * 16)(*a.tolist())


COLOR_RUNNING_AVERAGE = 0    # HashParams.m_colorIntegration
COLOR_WEIGHTED_AVERAGE = 1


def make_hash_params(num_buckets, num_sdf_blocks, voxel_size, truncation=None, trunc_scale=None,
                     max_integration_distance=4.0, weight_sample=10, weight_max=255,
                     max_collision_list=7, streaming_extents=(1.0, 1.0, 1.0),
                     streaming_dims=(257, 257, 257), streaming_min=(-128, -128, -128),
                     streaming_list_size=2000, weighted_colour=False):
    """HashParams as parametersFromGlobalAppState builds it.  truncation defaults
    to 5*voxel and trunc_scale to 2.5*voxel (zParametersManolisScan.txt:31-32).
    weighted_colour: fuse colours weighted by the voxel weights (m_colorIntegration = 1) instead of the reference's
    running 50/50 average."""
    p = HashParams()
    p.m_rigidTransform = (C.c_float * 16)(*IDENTITY16)
    p.m_rigidTransformInverse = (C.c_float * 16)(*IDENTITY16)
    p.m_hashNumBuckets = num_buckets
    p.m_hashBucketSize = HASH_BUCKET_SIZE
    p.m_hashMaxCollisionLinkedListSize = max_collision_list
    p.m_numSDFBlocks = num_sdf_blocks
    p.m_SDFBlockSize = SDF_BLOCK_SIZE
    p.m_virtualVoxelSize = voxel_size
    p.m_numOccupiedBlocks = 0
    p.m_maxIntegrationDistance = max_integration_distance
    p.m_truncation = float(np.float32(5.0) * np.float32(voxel_size)) if truncation is None else truncation
    p.m_truncScale = float(np.float32(2.5) * np.float32(voxel_size)) if trunc_scale is None else trunc_scale
    p.m_integrationWeightSample = weight_sample
    p.m_integrationWeightMax = weight_max
    p.m_streamingVoxelExtents = (C.c_float * 3)(*streaming_extents)
    p.m_streamingGridDimensions = (C.c_int32 * 3)(*streaming_dims)
    p.m_streamingMinGridPos = (C.c_int32 * 3)(*streaming_min)
    p.m_streamingInitialChunkListSize = streaming_list_size
    p.m_colorIntegration = COLOR_WEIGHTED_AVERAGE if weighted_colour else COLOR_RUNNING_AVERAGE
    return p


def make_depth_camera_params(width, height, depth_min=0.5, depth_max=5.0, fx=None, fy=None, mx=None, my=None):
    """Intrinsics of SURVEY.md section 8(d): fx = fy = 525*W/640, principal point
    at the image centre."""
    p = DepthCameraParams()
    p.fx = 525.0 * width / 640.0 if fx is None else fx
    p.fy = 525.0 * width / 640.0 if fy is None else fy
    p.mx = (width - 1) / 2.0 if mx is None else mx
    p.my = (height - 1) / 2.0 if my is None else my
    p.m_imageWidth = width
    p.m_imageHeight = height
    p.m_sensorDepthWorldMin = depth_min
    p.m_sensorDepthWorldMax = depth_max
    return p


def make_raycast_params(hash_params, cam_params, ray_increment_factor=0.8, thres_sample_dist_factor=50.5,
                        thres_dist_factor=50.0, use_gradients=False):
    """RayCastParams as CUDARayCastSDF::parametersFromGlobalAppState builds it
    (float32 arithmetic as in the reference)."""
    p = RayCastParams()
    p.m_viewMatrix = (C.c_float * 16)(*IDENTITY16)
    p.m_viewMatrixInverse = (C.c_float * 16)(*IDENTITY16)
    fx, fy, mx, my = cam_params.fx, cam_params.fy, cam_params.mx, cam_params.my
    p.m_intrinsics = mat16([[fx, 0, mx, 0], [0, fy, my, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    p.m_intrinsicsInverse = mat16([[1 / fx, 0, -mx / fx, 0], [0, 1 / fy, -my / fy, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    p.m_width = cam_params.m_imageWidth
    p.m_height = cam_params.m_imageHeight
    p.m_numOccupiedSDFBlocks = 0
    p.m_maxNumVertices = hash_params.m_numSDFBlocks * 6
    p.m_splatMinimum = 0
    p.m_minDepth = cam_params.m_sensorDepthWorldMin
    p.m_maxDepth = cam_params.m_sensorDepthWorldMax
    inc = np.float32(ray_increment_factor) * np.float32(hash_params.m_truncation)
    p.m_rayIncrement = float(inc)
    p.m_thresSampleDist = float(np.float32(thres_sample_dist_factor) * inc)
    p.m_thresDist = float(np.float32(thres_dist_factor) * inc)
    p.m_useGradients = 1 if use_gradients else 0
    return p


def make_marching_cubes_params(hash_params, max_num_triangles=1 << 20, thresh_factor=10.0):
    """parametersFromGlobalAppState, DSC/CUDAMarchingCubesHashSDF.h:19-28 (s_SDFMarchingCubeThreshFactor = 10 in
    the reference's zParameters files)"""
    p = MarchingCubesParams()
    p.m_maxNumTriangles = max_num_triangles
    p.m_threshMarchingCubes = np.float32(thresh_factor) * np.float32(hash_params.m_virtualVoxelSize)
    p.m_threshMarchingCubes2 = np.float32(thresh_factor) * np.float32(hash_params.m_virtualVoxelSize)
    p.m_sdfBlockSize = 8
    p.m_hashBucketSize = 10
    p.m_hashNumBuckets = hash_params.m_hashNumBuckets
    return p


def make_scene_options(offline=True, gc=True, starve=15, timings=False, streaming_out_parts=80,
                       reference_launch_sequence=False):
    o = SceneOptions()
    o.s_offlineProcessing = 1 if offline else 0
    o.s_garbageCollectionEnabled = 1 if gc else 0
    o.s_timingsDetailledEnabled = 1 if timings else 0
    o.s_useReferenceLaunchSequence = 1 if reference_launch_sequence else 0
    o.s_garbageCollectionStarve = starve
    o.s_streamingOutParts = streaming_out_parts
    return o
