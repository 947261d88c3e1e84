"""Python mirror of the reference host classes over the C ABI:

    CUDASceneRepHashSDF   (DepthSensingCUDA/Source/CUDASceneRepHashSDF.h:28)
    CUDARayCastSDF        (DepthSensingCUDA/Source/CUDARayCastSDF.h:13)
    CUDASceneRepChunkGrid (DepthSensingCUDA/Source/CUDASceneRepChunkGrid.h:152)

Same method names and argument meaning as the reference (camelCase kept), so
tests read like the reference's frame loop (DepthSensing.cpp:720-924).  All
compute happens in libvoxelhashing_amd.so on the GPU; this file only marshals.
"""
import ctypes as C

import numpy as np

from . import canonical
from . import vhtypes as T
from .lib import DeviceBuffer, VhError, check, download, f16, load


def _copy_struct(s):
    out = type(s)()
    C.memmove(C.byref(out), C.byref(s), C.sizeof(s))
    return out


def _unpack_rgb(packed):
    """r | g << 8 | b << 16 -> [n, 3] u8"""
    p = np.asarray(packed, dtype=np.uint32)
    return np.stack([p & 0xff, (p >> 8) & 0xff, (p >> 16) & 0xff], axis=-1).astype(np.uint8)


class DepthFrame:
    """Device-resident depth + colour image pair (DepthCameraData,
    DepthSensingCUDA/Source/DepthCameraUtil.h:17)."""

    def __init__(self, cam_params, depth=None, color=None, depth_ptr=None, color_ptr=None, stream=None):
        self.cp = cam_params
        n = cam_params.m_imageWidth * cam_params.m_imageHeight
        self._own = []
        if depth_ptr is None:
            buf = DeviceBuffer(4 * n)
            self._own.append(buf)
            depth_ptr = buf.ptr
            if depth is not None:
                buf.upload(np.ascontiguousarray(depth, dtype=np.float32), stream)
        if color_ptr is None and color is not False:
            buf = DeviceBuffer(16 * n)
            self._own.append(buf)
            color_ptr = buf.ptr
            if color is not None:
                buf.upload(np.ascontiguousarray(color, dtype=np.float32), stream)
        self.depth_ptr = depth_ptr
        self.color_ptr = color_ptr if color is not False else None
        self.data = T.DepthCameraData(self.depth_ptr, self.color_ptr)

    def download(self):
        H, W = self.cp.m_imageHeight, self.cp.m_imageWidth
        d = download(self.depth_ptr, np.float32, H * W).reshape(H, W)
        c = download(self.color_ptr, np.float32, H * W * 4).reshape(H, W, 4) if self.color_ptr else None
        return d, c


def synth_frame(spheres, inside, cam_to_world, cam_params, out=None, stream=None):
    """generate a synthetic frame on the device (vh_synth_frame)"""
    fr = out if out is not None else DepthFrame(cam_params)
    sp = np.ascontiguousarray(spheres, dtype=np.float64)
    check(load().vh_synth_frame(sp.ctypes.data, sp.shape[0], int(inside), f16(cam_to_world), C.byref(cam_params),
                                fr.depth_ptr, fr.color_ptr, stream), "vh_synth_frame")
    return fr


def _merge_upload(descs, blocks, stream):
    """-> (descs, blocks) in device memory and n; numpy arrays are checked for repeated positions first"""
    if isinstance(descs, DeviceBuffer):
        return descs, blocks, descs.nbytes // T.DESC_DTYPE.itemsize
    descs = np.ascontiguousarray(descs, dtype=T.DESC_DTYPE)
    n = len(descs)
    blocks = np.ascontiguousarray(blocks, dtype=T.VOXEL_DTYPE).reshape(n, T.SDF_BLOCK_VOXELS)
    if n and len(np.unique(descs["pos"].reshape(n, 3), axis=0)) != n:
        raise ValueError("merge: the block list names a position more than once")
    if n == 0:
        return DeviceBuffer(16), DeviceBuffer(8), 0
    return DeviceBuffer.from_numpy(descs, stream), DeviceBuffer.from_numpy(blocks, stream), n


def _counts_result(names, code, counts, what, extra=None):
    """the counts by name (a list of vhtypes: MERGE_COUNTS, CUT_COUNTS, DEINT_COUNTS) plus `extra`; with `what`, an
    error code raises VhError with .counts"""
    out = {k: int(v) for k, v in zip(names, counts)}
    out.update(extra or {})
    if what is not None and code != 0:
        try:
            check(code, what)
        except Exception as e:
            e.counts = out
            raise
    return out


def _merge_result(code, counts, left, what):
    """the merge's counts plus left_out_indices, read from (buffer, stream), or None"""
    idx = None
    if left is not None:
        idx = np.sort(left[0].download(np.uint32, int(counts[T.MERGE_COUNTS.index("left_out")]), left[1]).astype(np.int64))
    return _counts_result(T.MERGE_COUNTS, code, counts, what, {"left_out_indices": idx})


def resample_voxel_transforms(dst_from_src, vs_src, vs_dst):
    """vh_resample_voxel_transforms: a rigid 4x4 (metres, the destination's frame from the source's) and the two voxel
    sizes -> (srcVoxFromDstVox, dstVoxFromSrcVox), float32 [3, 4] in voxel index space.  Raises VhError
    (VH_ERR_BAD_ARGUMENT) for a matrix that is not rigid or sizes further apart than a factor of 2.  No device is needed."""
    m = np.ascontiguousarray(dst_from_src, dtype=np.float64).reshape(16)
    a, b = np.zeros(12, np.float32), np.zeros(12, np.float32)
    check(load().vh_resample_voxel_transforms(m.ctypes.data, C.c_float(vs_src), C.c_float(vs_dst), a.ctypes.data, b.ctypes.data),
          "vh_resample_voxel_transforms")
    return a.reshape(3, 4), b.reshape(3, 4)


def cut_region_transform(world_from_region, half_extents, voxel_size):
    """vh_cut_region_transform: a region's rigid frame (4x4, metres), its three half extents (metres) and a scene's voxel
    size -> regionFromVox, float32 [3, 4] in voxel index space (a voxel is inside a box iff every |row . (i, j, k, 1)| <=
    1).  Raises VhError (VH_ERR_BAD_ARGUMENT) for a frame that is not rigid or an extent that is not positive.  No
    device is needed."""
    m = np.ascontiguousarray(world_from_region, dtype=np.float64).reshape(16)
    h = np.ascontiguousarray(half_extents, dtype=np.float32).reshape(3)
    out = np.zeros(12, np.float32)
    check(load().vh_cut_region_transform(m.ctypes.data, h.ctypes.data, C.c_float(voxel_size), out.ctypes.data), "vh_cut_region_transform")
    return out.reshape(3, 4)


def _cut_result(code, counts, what, extra=None):
    return _counts_result(T.CUT_COUNTS, code, counts, what, extra)


def _staged_list(d_descs, d_blocks, n, stream):
    """a lifted list read back: (descs DESC_DTYPE [n], voxels VOXEL_DTYPE [n, 512]), block i of the list at slot i"""
    if n == 0:
        return np.zeros(0, T.DESC_DTYPE), np.zeros((0, T.SDF_BLOCK_VOXELS), T.VOXEL_DTYPE)
    descs = d_descs.download(T.DESC_DTYPE, n, stream)
    pool = d_blocks.download(T.VOXEL_DTYPE, n * T.SDF_BLOCK_VOXELS, stream).reshape(n, T.SDF_BLOCK_VOXELS)
    return descs, np.ascontiguousarray(pool[descs["ptr"] // T.SDF_BLOCK_VOXELS])


def extract_from_block_list(descs, blocks, region_from_vox, shape, select_outside=False, stream=None):
    """vh_cut_blocks in its list form (count, then lift with keep): the region copied out of a plain block list -- a
    streamed scene's host blocks, say -- which is uploaded and left as it is -> the counts by name plus "descs" and
    "voxels", the blocks with an observed voxel in the region, the voxels outside it zero"""
    L = load()
    m = np.ascontiguousarray(region_from_vox, dtype=np.float32).reshape(12)
    descs = np.ascontiguousarray(descs, dtype=T.DESC_DTYPE)
    n = len(descs)
    blocks = np.ascontiguousarray(blocks, dtype=T.VOXEL_DTYPE).reshape(n, T.SDF_BLOCK_VOXELS)
    counts = (C.c_uint32 * len(T.CUT_COUNTS))()
    if n == 0:
        return _cut_result(0, counts, "vh_cut_blocks", dict(zip(("descs", "voxels"), _staged_list(None, None, 0, stream))))
    d_desc, d_blocks = DeviceBuffer.from_numpy(descs, stream), DeviceBuffer.from_numpy(blocks, stream)
    d_work = DeviceBuffer(L.vh_cut_work_bytes(n))
    hp = T.HashParams()
    flags = T.CUT_LIFT | T.CUT_KEEP | (T.CUT_SELECT_OUTSIDE if select_outside else 0)
    check(L.vh_cut_blocks(None, C.byref(hp), n, d_desc.ptr, d_blocks.ptr, m.ctypes.data, int(shape), flags | T.CUT_COUNT_ONLY, 0, d_work.ptr, None, None, 0,
                          counts, stream), "vh_cut_blocks")
    room = int(counts[T.CUT_COUNTS.index("lifted")])
    d_out, d_staging = DeviceBuffer(16 * max(room, 1)), DeviceBuffer(8 * T.SDF_BLOCK_VOXELS * max(room, 1))
    check(L.vh_cut_blocks(None, C.byref(hp), n, d_desc.ptr, d_blocks.ptr, m.ctypes.data, int(shape), flags, 0, d_work.ptr, d_out.ptr, d_staging.ptr, room,
                          counts, stream), "vh_cut_blocks")
    return _cut_result(0, counts, "vh_cut_blocks", dict(zip(("descs", "voxels"), _staged_list(d_out, d_staging, room, stream))))


def _deint_result(code, counts, what):
    return _counts_result(T.DEINT_COUNTS, code, counts, what)


def _frame_data(frame, cp, what):
    """a DepthFrame's DepthCameraData, refused (VH_ERR_BAD_ARGUMENT) when the frame's image size is not cp's"""
    if not isinstance(frame, DepthFrame):
        return frame
    if (frame.cp.m_imageWidth, frame.cp.m_imageHeight) != (cp.m_imageWidth, cp.m_imageHeight):
        e = VhError(4, f"{what}: the frame is {frame.cp.m_imageWidth}x{frame.cp.m_imageHeight}, the camera {cp.m_imageWidth}x{cp.m_imageHeight}")
        e.counts = {k: 0 for k in T.DEINT_COUNTS}
        raise e
    return frame.data


def deintegrate_rule(stored, observed, hp, stream=None):
    """vh_debug_deintegrate_rule: the take-out rule of the frame de-integration on two VOXEL_DTYPE arrays of one shape
    (an observation of weight 0 is no observation) -> the voxels afterwards"""
    stored = np.ascontiguousarray(stored, dtype=T.VOXEL_DTYPE)
    observed = np.ascontiguousarray(observed, dtype=T.VOXEL_DTYPE)
    assert stored.shape == observed.shape
    n = stored.size
    if n == 0:
        return stored.copy()
    d_s, d_o, d_out = DeviceBuffer.from_numpy(stored, stream), DeviceBuffer.from_numpy(observed, stream), DeviceBuffer(8 * n)
    check(load().vh_debug_deintegrate_rule(d_s.ptr, d_o.ptr, d_out.ptr, n, C.byref(hp), stream), "vh_debug_deintegrate_rule")
    return d_out.download(T.VOXEL_DTYPE, n, stream).reshape(stored.shape)


class CUDASceneRepHashSDF:
    def __init__(self, params, options=None, stream=None):
        self.L = load()
        self.stream = stream
        self._params = _copy_struct(params)
        self._options = _copy_struct(options) if options is not None else T.make_scene_options(offline=False)
        h = C.c_void_p()
        check(self.L.vh_scene_rep_create(C.byref(self._params), C.byref(self._options), stream, C.byref(h)), "vh_scene_rep_create")
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self.L.vh_scene_rep_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- reference API -------------------------------------------------------
    def integrate(self, lastRigidTransform, depthCameraData, depthCameraParams, d_bitMask=None):
        data = depthCameraData.data if isinstance(depthCameraData, DepthFrame) else depthCameraData
        check(self.L.vh_scene_rep_integrate(self.handle, f16(lastRigidTransform), C.byref(data), C.byref(depthCameraParams), d_bitMask),
              "CUDASceneRepHashSDF::integrate")

    def integrateAhead(self, lastRigidTransform, depthCameraData, depthCameraParams, d_bitMask=None):
        """-> the frame's alloc + compactify job (a pointer for CUDARayCastSDF.render(..., coLaunch=job)) or None"""
        data = depthCameraData.data if isinstance(depthCameraData, DepthFrame) else depthCameraData
        job = C.POINTER(T.FrameJob)()
        check(self.L.vh_scene_rep_integrate_ahead(self.handle, f16(lastRigidTransform), C.byref(data), C.byref(depthCameraParams), d_bitMask,
                                                  C.byref(job)), "CUDASceneRepHashSDF::integrateAhead")
        return job if job else None

    def integrateFinish(self, depthCameraData, depthCameraParams):
        data = depthCameraData.data if isinstance(depthCameraData, DepthFrame) else depthCameraData
        check(self.L.vh_scene_rep_integrate_finish(self.handle, C.byref(data), C.byref(depthCameraParams)), "CUDASceneRepHashSDF::integrateFinish")

    def setLastRigidTransformAndCompactify(self, lastRigidTransform, depthCameraParams):
        check(self.L.vh_scene_rep_set_last_rigid_transform_and_compactify(self.handle, f16(lastRigidTransform), C.byref(depthCameraParams)),
              "setLastRigidTransformAndCompactify")

    def reset(self):
        check(self.L.vh_scene_rep_reset(self.handle), "reset")

    def getHashData(self):
        hd = T.HashData()
        check(self.L.vh_scene_rep_get_hash_data(self.handle, C.byref(hd)), "getHashData")
        return hd

    def getHashParams(self):
        hp = T.HashParams()
        check(self.L.vh_scene_rep_get_hash_params(self.handle, C.byref(hp)), "getHashParams")
        return hp

    def getLastRigidTransform(self):
        return np.array(self.getHashParams().m_rigidTransform, dtype=np.float32).reshape(4, 4)

    def getHeapFreeCount(self):
        n = C.c_uint32()
        check(self.L.vh_scene_rep_get_heap_free_count(self.handle, C.byref(n)), "getHeapFreeCount")
        return n.value

    def getNumOccupiedBlocks(self):
        n = C.c_uint32()
        check(self.L.vh_scene_rep_get_num_occupied_blocks(self.handle, C.byref(n)), "getNumOccupiedBlocks")
        return n.value

    def debugHash(self):
        rep = (C.c_uint32 * 4)()
        check(self.L.vh_scene_rep_debug_hash(self.handle, rep), "debugHash")
        return dict(numOccupied=rep[0], numFree=rep[1], duplicates=rep[2], lockEntries=rep[3])

    # ---- additions ---------------------------------------------------------------
    def setOptions(self, options):
        self._options = _copy_struct(options)
        check(self.L.vh_scene_rep_set_options(self.handle, C.byref(self._options)), "setOptions")

    def setColorIntegration(self, mode):
        """T.COLOR_RUNNING_AVERAGE (the reference's 50/50 colour average) or T.COLOR_WEIGHTED_AVERAGE (weighted by the
        voxel weights), from the next integrate() on"""
        check(self.L.vh_scene_rep_set_color_integration(self.handle, int(mode)), "setColorIntegration")

    def getColorIntegration(self):
        return int(self.getHashParams().m_colorIntegration)

    def queryPoints(self, points, gradient=True):
        """distance, colour and gradient of the model at world points [n, 3] (vh_query_points: include/vh_api.h has the
        semantics) -> dict sdf [n] f32 (-inf where invalid), color [n, 3] u8, gradient [n, 3] f32 (None without), valid [n] bool"""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n, s = len(pts), self.stream
        d_pts, d_sdf, d_col, d_val = DeviceBuffer.from_numpy(pts, s), DeviceBuffer(4 * n), DeviceBuffer(4 * n), DeviceBuffer(n)
        d_grad = DeviceBuffer(12 * n) if gradient else None
        check(self.L.vh_scene_rep_query_points(self.handle, d_pts.ptr, n, d_sdf.ptr, d_col.ptr, d_grad.ptr if gradient else None, d_val.ptr),
              "CUDASceneRepHashSDF::queryPoints")
        return dict(sdf=d_sdf.download(np.float32, n, s), color=_unpack_rgb(d_col.download(np.uint32, n, s)),
                    gradient=d_grad.download(np.float32, 3 * n, s).reshape(n, 3) if gradient else None,
                    valid=d_val.download(np.uint8, n, s).astype(bool))

    # ---- scene merge (DESIGN.md section 4 "Scene merge") ----------------------------------------------------------
    def mergeScene(self, other, block_offset=(0, 0, 0)):
        """Fuses every block resident in `other`'s table into this scene, shifted by whole blocks (vh_api.h has the
        semantics of vh_merge_blocks) -> the counts by name (vhtypes.MERGE_COUNTS), left_out_indices None.  Raises VhError:
        VH_ERR_BAD_ARGUMENT for two voxel sizes, other is self, a frame in flight; VH_ERR_HEAP_EXHAUSTED when the new
        positions outnumber the free blocks -- nothing was done then, and the exception carries the counts (.counts).
        Compactify before the next ray cast."""
        counts = (C.c_uint32 * len(T.MERGE_COUNTS))()
        off = (C.c_int32 * 3)(*[int(v) for v in block_offset])
        return _merge_result(self.L.vh_scene_rep_merge_scene(self.handle, other.handle, off, counts), counts, None, "CUDASceneRepHashSDF::mergeScene")

    def mergeBlocks(self, descs, blocks, block_offset=(0, 0, 0)):
        """mergeScene for a block list: descs (DESC_DTYPE [n], ptr ignored) and blocks (VOXEL_DTYPE [n, 512]) as numpy
        arrays -- repeated positions raise ValueError before anything is uploaded -- or as DeviceBuffers with n =
        descs.nbytes / 16 -> the counts by name plus left_out_indices, the indices of the blocks the table had no slot for"""
        off = (C.c_int32 * 3)(*[int(v) for v in block_offset])
        d_desc, d_blocks, n = _merge_upload(descs, blocks, self.stream)
        d_left = DeviceBuffer(4 * max(n, 1))
        counts = (C.c_uint32 * len(T.MERGE_COUNTS))()
        rc = self.L.vh_scene_rep_merge_blocks(self.handle, d_desc.ptr, d_blocks.ptr, n, off, d_left.ptr, counts)
        return _merge_result(rc, counts, (d_left, self.stream), "CUDASceneRepHashSDF::mergeBlocks")

    def mergeSceneTransformed(self, other, dst_from_src):
        """Fuses `other`, in another world frame and possibly at another voxel size, into this scene: other is sampled at
        this scene's voxel centres under the rigid 4x4 dst_from_src (metres; a point of other's frame in this scene's) and
        the blocks with an observed voxel are merged as mergeScene merges (DESIGN.md section 4 "Resampled merge")
        -> the merge's counts by name, with "resample": the counts of vhtypes.RESAMPLE_COUNTS.  Raises VhError with
        .counts: VH_ERR_BAD_ARGUMENT (nothing done) for a matrix that is not rigid, voxel sizes further apart than a
        factor of 2, other is self, a frame in flight, a block outside the lattice's range; VH_ERR_HEAP_EXHAUSTED
        (nothing done) as mergeScene.  Compactify before the next ray cast."""
        m = np.ascontiguousarray(dst_from_src, dtype=np.float64).reshape(16)
        counts = (C.c_uint32 * len(T.MERGE_COUNTS))()
        resampled = (C.c_uint32 * len(T.RESAMPLE_COUNTS))()
        rc = self.L.vh_scene_rep_merge_scene_transformed(self.handle, other.handle, m.ctypes.data, counts, resampled)
        extra = {"resample": {k: int(v) for k, v in zip(T.RESAMPLE_COUNTS, resampled)}}
        try:
            out = _merge_result(rc, counts, None, "CUDASceneRepHashSDF::mergeSceneTransformed")
        except Exception as e:
            e.counts.update(extra)
            raise
        out.update(extra)
        return out

    # ---- scene registration (DESIGN.md section 4 "Scene registration") ----------------------------------------------
    def alignScene(self, other, guess=None, options=None, **overrides):
        """Refines the rigid 4x4 `guess` (metres; a point of other's frame in this scene's; default the identity) so that
        other's near-surface voxels fall where this scene's field has their distance: direct SDF-to-SDF Gauss-Newton on
        the device (vh_api.h has the rule of vh_align_step).  Neither scene is written.  options: a vhtypes.AlignOptions
        (make_align_options), or its fields by keyword -> vhtypes.align_state_dict of the state: "dst_from_src" is an
        answer only where "converged"; "status" tells how it ended otherwise (vhtypes.ALIGN_*).  The basin is a few
        voxels and a few degrees around the guess.  Raises VhError (VH_ERR_BAD_ARGUMENT, nothing done) for other is
        self, a guess that is not rigid, voxel sizes further apart than a factor of 2, options that are not finite and
        positive or beyond their bounds, a frame in flight."""
        m = np.ascontiguousarray(np.eye(4) if guess is None else guess, dtype=np.float64).reshape(16)
        o = options if options is not None else T.make_align_options(**overrides)
        st = T.AlignState()
        check(self.L.vh_scene_rep_align_scene(self.handle, other.handle, m.ctypes.data, C.byref(o), C.byref(st)), "CUDASceneRepHashSDF::alignScene")
        return T.align_state_dict(st)

    # ---- scene cut (DESIGN.md section 4 "Scene cut") ---------------------------------------------------------------
    def eraseRegion(self, region):
        """Zeroes the voxels inside `region` (a vhtypes.CutRegion: make_cut_region) and frees the blocks in which no
        observed voxel is left (vh_api.h has the rule of vh_cut_blocks) -> the counts by name (vhtypes.CUT_COUNTS).
        Raises VhError (VH_ERR_BAD_ARGUMENT, nothing done) for a region that is not rigid or has no size and for a frame
        in flight.  Compactify before the next ray cast."""
        counts = (C.c_uint32 * len(T.CUT_COUNTS))()
        return _cut_result(self.L.vh_scene_rep_erase_region(self.handle, C.byref(region), counts), counts, "CUDASceneRepHashSDF::eraseRegion")

    def cropToRegion(self, region):
        """eraseRegion of everything that is not inside `region`"""
        counts = (C.c_uint32 * len(T.CUT_COUNTS))()
        return _cut_result(self.L.vh_scene_rep_crop_to_region(self.handle, C.byref(region), counts), counts, "CUDASceneRepHashSDF::cropToRegion")

    def extractRegion(self, region, download=True):
        """Copies the region out and leaves the scene as it is: the blocks with an observed voxel in the region, the
        voxels outside it zero -> the counts by name plus "descs" and "voxels", a list for mergeBlocks: numpy arrays
        (DESC_DTYPE [n], VOXEL_DTYPE [n, 512]) or, with download=False, DeviceBuffers and "n"."""
        counts = (C.c_uint32 * len(T.CUT_COUNTS))()
        n = C.c_uint32()
        what = "CUDASceneRepHashSDF::extractRegion"
        _cut_result(self.L.vh_scene_rep_extract_region(self.handle, C.byref(region), None, None, 0, C.byref(n), counts), counts, what)
        room = n.value
        d_descs, d_blocks = DeviceBuffer(16 * max(room, 1)), DeviceBuffer(8 * T.SDF_BLOCK_VOXELS * max(room, 1))
        if room:
            _cut_result(self.L.vh_scene_rep_extract_region(self.handle, C.byref(region), d_descs.ptr, d_blocks.ptr, room, C.byref(n), counts), counts, what)
        if not download:
            return _cut_result(0, counts, what, dict(descs=d_descs, voxels=d_blocks, n=room))
        descs, voxels = _staged_list(d_descs, d_blocks, room, self.stream)
        return _cut_result(0, counts, what, dict(descs=descs, voxels=voxels))

    def moveRegionTo(self, dst, region, block_offset=(0, 0, 0)):
        """Moves the region's voxels into `dst`, shifted by whole blocks: extractRegion, dst.mergeBlocks of the list,
        eraseRegion here -- the erase only if the merge left no block out -> the cut's counts by name, with "merge":
        the merge's.  Raises VhError with .counts: VH_ERR_HEAP_EXHAUSTED when dst's pool is too small (both scenes
        untouched), VH_ERR_BAD_ARGUMENT for dst is self, two voxel sizes, a frame in flight.  A merge status that leaves
        blocks out (MERGE_NO_SLOT, MERGE_NOT_SETTLED) is in "merge"; this scene is then untouched (voxels_erased 0)."""
        counts = (C.c_uint32 * len(T.CUT_COUNTS))()
        merged = (C.c_uint32 * len(T.MERGE_COUNTS))()
        off = (C.c_int32 * 3)(*[int(v) for v in block_offset])
        rc = self.L.vh_scene_rep_move_region_to(self.handle, dst.handle, C.byref(region), off, counts, merged)
        return _cut_result(rc, counts, "CUDASceneRepHashSDF::moveRegionTo", {"merge": {k: int(v) for k, v in zip(T.MERGE_COUNTS, merged)}})

    # ---- frame de-integration (DESIGN.md section 4 "Frame de-integration") ------------------------------------------
    def deintegrate(self, rigidTransform, depthCameraData, depthCameraParams):
        """Takes the frame that integrate() fused at `rigidTransform` -- the same maps, the same camera -- back out of
        the blocks resident in the table and frees the blocks left without an observed voxel (vh_api.h has the rule of
        vh_deintegrate_blocks) -> the counts by name (vhtypes.DEINT_COUNTS).  The scene's last rigid transform and its
        frame count stay.  Raises VhError (VH_ERR_BAD_ARGUMENT, nothing done) for a frame in flight, a null map and a
        frame whose image size is not the camera's.  Compactify before the next ray cast."""
        what = "CUDASceneRepHashSDF::deintegrate"
        data = _frame_data(depthCameraData, depthCameraParams, what)
        counts = (C.c_uint32 * len(T.DEINT_COUNTS))()
        return _deint_result(self.L.vh_scene_rep_deintegrate(self.handle, f16(rigidTransform), C.byref(data), C.byref(depthCameraParams), counts), counts, what)

    def getNumIntegratedFrames(self):
        """the frames integrate() has fused; a de-integration does not change it"""
        n = C.c_uint32()
        check(self.L.vh_scene_rep_get_num_integrated_frames(self.handle, C.byref(n)), "getNumIntegratedFrames")
        return n.value

    def frameInFlight(self):
        """True between integrateAhead() and integrateFinish(): what merge, cut and de-integration refuse"""
        out = C.c_int()
        check(self.L.vh_scene_rep_frame_in_flight(self.handle, C.byref(out)), "frameInFlight")
        return bool(out.value)

    def reintegrate(self, oldTransform, newTransform, depthCameraData, depthCameraParams, d_bitMask=None):
        """deintegrate(oldTransform) followed by integrate(newTransform), which counts as a frame -> the take-out's counts"""
        what = "CUDASceneRepHashSDF::reintegrate"
        data = _frame_data(depthCameraData, depthCameraParams, what)
        counts = (C.c_uint32 * len(T.DEINT_COUNTS))()
        return _deint_result(self.L.vh_scene_rep_reintegrate(self.handle, f16(oldTransform), f16(newTransform), C.byref(data), C.byref(depthCameraParams),
                                                             d_bitMask, counts), counts, what)

    def getState(self):
        out = (C.c_uint32 * T.STATE_WORDS)()
        check(self.L.vh_scene_rep_get_state(self.handle, out), "getState")
        return np.array(out, dtype=np.uint32)

    def getTimings(self):
        out = (C.c_double * 4)()
        check(self.L.vh_scene_rep_get_timings(self.handle, out), "getTimings")
        return dict(alloc_ms=out[0], compactify_ms=out[1], integrate_ms=out[2], frames=int(out[3]))

    def synchronize(self):
        check(self.L.vh_stream_synchronize(self.stream), "synchronize")

    # ---- downloads (test support) ---------------------------------------------------
    def download(self, with_voxels=True):
        """-> dict with the raw tables (hash, heap, counters, optionally voxels)"""
        hp = self.getHashParams()
        hd = self.getHashData()
        ne = hp.m_hashNumBuckets * T.HASH_BUCKET_SIZE
        s = self.stream
        out = dict(
            params=hp,
            hash=download(hd.d_hash, T.HASH_ENTRY_DTYPE, ne, s),
            heap=download(hd.d_heap, np.uint32, hp.m_numSDFBlocks, s),
            heap_counter=int(download(hd.d_heapCounter, np.uint32, 1, s)[0]),
            bucket_count=download(hd.d_bucketCount, np.uint32, hp.m_hashNumBuckets, s),
            bucket_bits=download(hd.d_bucketBits, np.uint32, (hp.m_hashNumBuckets + 31) // 32, s),
            compact_count=int(download(hd.d_hashCompactifiedCounter, np.int32, 1, s)[0]),
        )
        out["compactified"] = download(hd.d_hashCompactified, T.HASH_ENTRY_DTYPE, out["compact_count"], s)
        out["decisions"] = download(hd.d_hashDecision, np.int32, out["compact_count"], s)
        if with_voxels:
            out["sdf_blocks"] = download(hd.d_SDFBlocks, T.VOXEL_DTYPE, hp.m_numSDFBlocks * T.SDF_BLOCK_VOXELS, s)
        return out

    def state(self, with_voxels=True, check_invariants=True):
        """canonical snapshot (voxelhashing_amd.canonical) + invariant checks"""
        d = self.download(with_voxels)
        hp = d["params"]
        if check_invariants:
            canonical.check_invariants(d["hash"], d["heap"], d["heap_counter"], hp, d.get("sdf_blocks"))
            canonical.check_bucket_summary(d["hash"], d["bucket_count"], d["bucket_bits"], hp)
        snap = canonical.snapshot(d["hash"], d.get("sdf_blocks"), d["heap"], d["heap_counter"], hp, with_voxels)
        snap["compactified"] = d["compactified"]
        snap["decisions"] = d["decisions"]
        return snap


class CUDARayCastSDF:
    def __init__(self, params, stream=None):
        self.L = load()
        self.stream = stream
        self._params = _copy_struct(params)
        h = C.c_void_p()
        check(self.L.vh_raycast_create(C.byref(self._params), stream, C.byref(h)), "vh_raycast_create")
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self.L.vh_raycast_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def render(self, hashData, hashParams, depthCameraParams, lastRigidTransform, coLaunch=None):
        if coLaunch is not None:
            check(self.L.vh_raycast_render_co(self.handle, C.byref(hashData), C.byref(hashParams), C.byref(depthCameraParams),
                                              f16(lastRigidTransform), coLaunch), "CUDARayCastSDF::render")
            return
        check(self.L.vh_raycast_render(self.handle, C.byref(hashData), C.byref(hashParams), C.byref(depthCameraParams),
                                       f16(lastRigidTransform)), "CUDARayCastSDF::render")

    def castRays(self, hashData, hashParams, origins, directions, t_min, t_max, normals=True):
        """rays given in world space through the model (vh_query_rays: include/vh_api.h has the semantics); origins and
        directions [n, 3], t_min / t_max [n] or scalars -> dict t [n] f32 (-inf without a hit), normal [n, 3] f32 (world;
        None without), color [n, 3] u8, status [n] u8 (T.QUERY_MISS / QUERY_HIT / QUERY_REFUSED)"""
        org = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        n, s = len(org), self.stream
        dirs = np.ascontiguousarray(np.broadcast_to(np.asarray(directions, dtype=np.float32).reshape(-1, 3), (n, 3)))
        t0 = np.ascontiguousarray(np.broadcast_to(np.asarray(t_min, dtype=np.float32).reshape(-1), (n,)))
        t1 = np.ascontiguousarray(np.broadcast_to(np.asarray(t_max, dtype=np.float32).reshape(-1), (n,)))
        ins = [DeviceBuffer.from_numpy(a, s) for a in (org, dirs, t0, t1)]
        d_t, d_col, d_st = DeviceBuffer(4 * n), DeviceBuffer(4 * n), DeviceBuffer(n)
        d_nrm = DeviceBuffer(12 * n) if normals else None
        check(self.L.vh_ray_cast_cast_rays(self.handle, C.byref(hashData), C.byref(hashParams), ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, n,
                                           d_t.ptr, d_nrm.ptr if normals else None, d_col.ptr, d_st.ptr), "CUDARayCastSDF::castRays")
        return dict(t=d_t.download(np.float32, n, s), normal=d_nrm.download(np.float32, 3 * n, s).reshape(n, 3) if normals else None,
                    color=_unpack_rgb(d_col.download(np.uint32, n, s)), status=d_st.download(np.uint8, n, s))

    def getRayCastData(self):
        rd = T.RayCastData()
        check(self.L.vh_raycast_get_data(self.handle, C.byref(rd)), "getRayCastData")
        return rd

    def getRayCastParams(self):
        rp = T.RayCastParams()
        check(self.L.vh_raycast_get_params(self.handle, C.byref(rp)), "getRayCastParams")
        return rp

    def setTiming(self, on, march_only=False, stride=1):
        check(self.L.vh_raycast_set_timing_stride(self.handle, (2 if march_only else 1) if on else 0, stride), "setTiming")

    def setIntervalSplatting(self, on):
        check(self.L.vh_raycast_set_interval_splatting(self.handle, 1 if on else 0), "setIntervalSplatting")

    def getTileCapacity(self):
        """entries per tile list of the latest render(): 64, or 128 while fine voxels ask for large tile tables"""
        n = C.c_uint32()
        check(self.L.vh_raycast_get_tile_capacity(self.handle, C.byref(n)), "getTileCapacity")
        return n.value

    def getTimings(self):
        out = (C.c_double * 4)()
        check(self.L.vh_raycast_get_timings(self.handle, out), "getTimings")
        return dict(raycast_ms=out[0], normals_ms=out[1], frames=int(out[2]), splat_ms=out[3])

    def getEventPairOverheadMs(self):
        out = C.c_double(0.0)
        check(self.L.vh_raycast_get_event_pair_overhead(self.handle, C.byref(out)), "getEventPairOverhead")
        return out.value

    def download(self):
        rd = self.getRayCastData()
        W, H = self._params.m_width, self._params.m_height
        s = self.stream
        return dict(
            depth=download(rd.d_depth, np.float32, H * W, s).reshape(H, W),
            depth4=download(rd.d_depth4, np.float32, H * W * 4, s).reshape(H, W, 4),
            normals=download(rd.d_normals, np.float32, H * W * 4, s).reshape(H, W, 4),
            colors=download(rd.d_colors, np.float32, H * W * 4, s).reshape(H, W, 4),
        )


class CUDASceneRepChunkGrid:
    def __init__(self, sceneRepHashSDF, voxelExtends, gridDimensions, minGridPos, initialChunkListSize,
                 streamingEnabled, streamOutParts):
        self.L = load()
        self.scene = sceneRepHashSDF
        h = C.c_void_p()
        ext = np.asarray(voxelExtends, dtype=np.float32)
        dims = (C.c_int32 * 3)(*[int(v) for v in gridDimensions])
        mn = (C.c_int32 * 3)(*[int(v) for v in minGridPos])
        check(self.L.vh_chunk_grid_create(sceneRepHashSDF.handle, f16(ext), dims, mn, initialChunkListSize,
                                          1 if streamingEnabled else 0, streamOutParts, C.byref(h)), "vh_chunk_grid_create")
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self.L.vh_chunk_grid_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def streamOutToCPUPass0GPU(self, posCamera, radius, useParts=True, multiThreaded=True):
        check(self.L.vh_chunk_grid_stream_out_to_cpu_pass0_gpu(self.handle, f16(posCamera), radius, int(useParts), int(multiThreaded)),
              "streamOutToCPUPass0GPU")

    def streamOutToCPUPass1CPU(self, multiThreaded=True):
        check(self.L.vh_chunk_grid_stream_out_to_cpu_pass1_cpu(self.handle, int(multiThreaded)), "streamOutToCPUPass1CPU")

    def streamInToGPUPass0CPU(self, posCamera, radius, useParts=True, multiThreaded=True):
        check(self.L.vh_chunk_grid_stream_in_to_gpu_pass0_cpu(self.handle, f16(posCamera), radius, int(useParts), int(multiThreaded)),
              "streamInToGPUPass0CPU")

    def streamInToGPUPass1GPU(self, multiThreaded=True):
        check(self.L.vh_chunk_grid_stream_in_to_gpu_pass1_gpu(self.handle, int(multiThreaded)), "streamInToGPUPass1GPU")

    def streamOutToCPU(self, posCamera, radius, useParts=True):
        n = C.c_uint32()
        check(self.L.vh_chunk_grid_stream_out_to_cpu(self.handle, f16(posCamera), radius, int(useParts), C.byref(n)), "streamOutToCPU")
        return n.value

    def streamInToGPU(self, posCamera, radius, useParts=True):
        n = C.c_uint32()
        check(self.L.vh_chunk_grid_stream_in_to_gpu(self.handle, f16(posCamera), radius, int(useParts), C.byref(n)), "streamInToGPU")
        return n.value

    def streamOutToCPUAll(self):
        check(self.L.vh_chunk_grid_stream_out_to_cpu_all(self.handle), "streamOutToCPUAll")

    def streamInToGPUAll(self, posCamera, radius, useParts=True):
        n = C.c_uint32()
        check(self.L.vh_chunk_grid_stream_in_to_gpu_all(self.handle, f16(posCamera), radius, int(useParts), C.byref(n)), "streamInToGPUAll")
        return n.value

    def getBitMaskGPU(self):
        p = C.c_void_p()
        check(self.L.vh_chunk_grid_get_bit_mask_gpu(self.handle, C.byref(p)), "getBitMaskGPU")
        return p

    def downloadBitMasks(self):
        """-> (host copy, device copy, host copy marked dirty): both copies of the bit mask with the pipeline drained and
        before any upload of the host's copy (read-only; for tests)"""
        n, dirty = C.c_uint32(), C.c_int32()
        check(self.L.vh_chunk_grid_debug_download_bit_masks(self.handle, None, None, 0, C.byref(n), C.byref(dirty)), "downloadBitMasks")
        host, dev = np.zeros(n.value, dtype=np.uint32), np.zeros(n.value, dtype=np.uint32)
        check(self.L.vh_chunk_grid_debug_download_bit_masks(self.handle, host.ctypes.data, dev.ctypes.data, n.value, C.byref(n), C.byref(dirty)),
              "downloadBitMasks")
        return host, dev, bool(dirty.value)

    def reset(self):
        check(self.L.vh_chunk_grid_reset(self.handle), "reset")

    def debugCheckForDuplicates(self):
        check(self.L.vh_chunk_grid_debug_check_for_duplicates(self.handle), "debugCheckForDuplicates")

    def getStatistics(self):
        out = (C.c_uint32 * 3)()
        check(self.L.vh_chunk_grid_get_statistics(self.handle, out), "getStatistics")
        return dict(chunks=out[0], blocks=out[1], bits=out[2])

    def getNumFailedInserts(self):
        out = C.c_uint32(0)
        check(self.L.vh_chunk_grid_get_num_failed_inserts(self.handle, C.byref(out)), "getNumFailedInserts")
        return out.value

    def downloadHostBlocks(self):
        n = C.c_uint32()
        check(self.L.vh_chunk_grid_download_host_blocks(self.handle, None, None, 0, C.byref(n)), "downloadHostBlocks")
        descs = np.zeros(n.value, dtype=T.DESC_DTYPE)
        blocks = np.zeros((n.value, T.SDF_BLOCK_VOXELS), dtype=T.VOXEL_DTYPE)
        if n.value:
            check(self.L.vh_chunk_grid_download_host_blocks(self.handle, descs.ctypes.data, blocks.ctypes.data, n.value, C.byref(n)),
                  "downloadHostBlocks")
        return descs, blocks

    def saveToFile(self, filename, camPos, radius):
        check(self.L.vh_chunk_grid_save_to_file(self.handle, filename.encode(), f16(camPos), radius), "saveToFile")

    def loadFromFile(self, filename, camPos, radius):
        check(self.L.vh_chunk_grid_load_from_file(self.handle, filename.encode(), f16(camPos), radius), "loadFromFile")


class Reconstruction:
    """The frame loop reconstruction() (DepthSensingCUDA/Source/DepthSensing.cpp:720-924) for a recorded sequence at
    given poses, native behind the C ABI: run() enqueues any number of frames with one call."""

    def __init__(self, sceneRep, rayCast, chunkGrid, depthCameraParams, options=None):
        self.L = load()
        self.scene, self.ray, self.grid = sceneRep, rayCast, chunkGrid  # kept alive as long as the loop
        self._cp = _copy_struct(depthCameraParams)
        self._options = _copy_struct(options) if options is not None else self.defaultOptions()
        h = C.c_void_p()
        check(self.L.vh_reconstruction_create(sceneRep.handle, rayCast.handle if rayCast is not None else None,
                                              chunkGrid.handle if chunkGrid is not None else None, C.byref(self._cp),
                                              C.byref(self._options), C.byref(h)), "vh_reconstruction_create")
        self.handle = h

    @staticmethod
    def defaultOptions(**overrides):
        o = T.ReconstructionOptions()
        load().vh_reconstruction_default_options(C.byref(o))
        for k, v in overrides.items():
            if k in ("s_streamingPos",):
                o.s_streamingPos[:] = [float(x) for x in v]
            else:
                setattr(o, k, v)
        return o

    @staticmethod
    def makeFrames(poses, depth_ptrs, color_ptrs):
        """-> ctypes array of VhSequenceFrame (device pointers, or host pointers for s_framesOnHost)"""
        n = len(poses)
        arr = (T.SequenceFrame * n)()
        for k in range(n):
            arr[k].rigidTransform[:] = [float(v) for v in np.asarray(poses[k], dtype=np.float32).reshape(-1)]
            arr[k].depth = depth_ptrs[k]
            arr[k].color = color_ptrs[k] if color_ptrs is not None else None
        return arr

    def close(self):
        if getattr(self, "handle", None):
            self.L.vh_reconstruction_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, frames, first=0, count=None, lookahead=False):
        """frames: a VhSequenceFrame array (makeFrames); processes frames[first:first+count].  lookahead: the loop may
        read the pose of frames[first+count], the frame a later call will bring (vh_reconstruction_run_ahead)"""
        n = len(frames) - first if count is None else count
        if n <= 0:
            return
        ptr = C.cast(C.byref(frames, first * C.sizeof(T.SequenceFrame)), C.POINTER(T.SequenceFrame))
        if lookahead and first + n < len(frames):
            nxt = C.cast(C.byref(frames, (first + n) * C.sizeof(T.SequenceFrame)), C.POINTER(T.SequenceFrame))
            check(self.L.vh_reconstruction_run_ahead(self.handle, ptr, n, nxt), "Reconstruction::run")
        else:
            check(self.L.vh_reconstruction_run(self.handle, ptr, n), "Reconstruction::run")

    # ---- raw frames: 16-bit depth + 8-bit colour at the sensor's sizes -------------------------------------------
    def setRawFormat(self, depth_size, color_size=None, depth_shift=1000.0, color_channels=3, depth_filter=None, color_filter=None):
        """Once, before the first frame.  depth_size / color_size: (width, height) of the sensor's images;
        color_channels: 3 (RGB), 4 (RGBX) or 0 (no colour); depth_filter / color_filter: None, or (sigmaD, sigmaR) of the
        Gauss filter CUDARGBDSensor::process applies (s_depthFilter / s_colorFilter of the parameter file)"""
        f = T.RawFrameFormat()
        f.depthWidth, f.depthHeight = int(depth_size[0]), int(depth_size[1])
        if color_size is not None:
            f.colorWidth, f.colorHeight = int(color_size[0]), int(color_size[1])
        f.depthShift = depth_shift
        f.colorChannels = int(color_channels)
        if depth_filter is not None:
            f.s_depthFilter, (f.s_depthSigmaD, f.s_depthSigmaR) = 1, depth_filter
        if color_filter is not None:
            f.s_colorFilter, (f.s_colorSigmaD, f.s_colorSigmaR) = 1, color_filter
        check(self.L.vh_reconstruction_set_raw_format(self.handle, C.byref(f)), "Reconstruction::setRawFormat")
        self._raw_format = f

    @staticmethod
    def makeRawFrames(poses, depth_ptrs, color_ptrs):
        """-> ctypes array of VhRawSequenceFrame (host pointers for s_framesOnHost, else device pointers)"""
        n = len(poses)
        arr = (T.RawSequenceFrame * n)()
        for k in range(n):
            arr[k].rigidTransform[:] = [float(v) for v in np.asarray(poses[k], dtype=np.float32).reshape(-1)]
            arr[k].depth = depth_ptrs[k]
            arr[k].color = color_ptrs[k] if color_ptrs is not None else None
        return arr

    def runRaw(self, frames, first=0, count=None, lookahead=False):
        """run() for a VhRawSequenceFrame array (makeRawFrames); needs setRawFormat"""
        n = len(frames) - first if count is None else count
        if n <= 0:
            return
        ptr = C.cast(C.byref(frames, first * C.sizeof(T.RawSequenceFrame)), C.POINTER(T.RawSequenceFrame))
        if lookahead and first + n < len(frames):
            nxt = C.cast(C.byref(frames, (first + n) * C.sizeof(T.RawSequenceFrame)), C.POINTER(T.RawSequenceFrame))
            check(self.L.vh_reconstruction_run_raw_ahead(self.handle, ptr, n, nxt), "Reconstruction::runRaw")
        else:
            check(self.L.vh_reconstruction_run_raw(self.handle, ptr, n), "Reconstruction::runRaw")

    # ---- camera tracking inside the loop ----------------------------------------------------------------------------
    def setTracking(self, tracking_state):
        """Once, before the first frame: from then on run() / runRaw() ignore the frames' poses; every frame after the first
        is aligned to the ray cast of the model by projective ICP (tracking_state: a TrackingState) and integrated at
        lastRigidTransform * delta, a frame on which tracking is lost is not integrated.  Needs a ray caster."""
        check(self.L.vh_reconstruction_set_tracking(self.handle, C.byref(tracking_state)), "Reconstruction::setTracking")

    def setTrackingRGBD(self, tracking_state_rgbd):
        """setTracking with the RGB-D tracker (depth + photometric ICP; tracking_state_rgbd: a TrackingStateRGBD) in place
        of the plain one: one of the two, once.  Every frame then needs a colour map."""
        check(self.L.vh_reconstruction_set_tracking_rgbd(self.handle, C.byref(tracking_state_rgbd)), "Reconstruction::setTrackingRGBD")

    def getPoses(self, first=0, count=None):
        """-> [count, 4, 4] float32: the pose each frame fed since creation / reset was integrated at, all -inf for a frame
        that was not (tracking lost, invalid recorded pose).  count=None: up to the last frame fed (asks getStats)."""
        if count is None:
            st = self.getStats()
            count = st["frames"] + st["invalidFrames"] + st["lostFrames"] - first
        out = np.empty((max(int(count), 0), 4, 4), dtype=np.float32)
        if len(out):
            check(self.L.vh_reconstruction_get_poses(self.handle, int(first), len(out), out.ctypes.data_as(C.POINTER(C.c_float))), "Reconstruction::getPoses")
        return out

    def synchronize(self):
        check(self.L.vh_reconstruction_synchronize(self.handle), "Reconstruction::synchronize")

    def reset(self):
        check(self.L.vh_reconstruction_reset(self.handle), "Reconstruction::reset")

    def debugFailRender(self, nth_render_from_now):
        check(self.L.vh_reconstruction_debug_fail_render(self.handle, int(nth_render_from_now)), "Reconstruction::debugFailRender")

    def getStats(self):
        st = T.ReconstructionStats()
        check(self.L.vh_reconstruction_get_stats(self.handle, C.byref(st)), "Reconstruction::getStats")
        out = {k: getattr(st, k) for k, _ in T.ReconstructionStats._fields_}
        out["trackedFrames"], out["lostFrames"] = self.getTrackingStats()
        return out

    def getTrackingStats(self):
        """-> (trackedFrames, lostFrames): frames integrated at a pose the loop tracked itself, frames on which tracking was
        lost; both 0 without setTracking.  Waits for nothing."""
        a, b = C.c_uint64(), C.c_uint64()
        check(self.L.vh_reconstruction_get_tracking_stats(self.handle, C.byref(a), C.byref(b)), "Reconstruction::getTrackingStats")
        return a.value, b.value


class LauncherScene:
    """HashData + the launcher-level C ABI (the twins of the reference's
    extern "C" launchers, DepthSensingCUDA/Source/CUDASceneRepHashSDF.h:15-26 and
    CUDASceneRepChunkGrid.h:142-146), one call per kernel, for tests that pin
    each launcher on its own."""

    def __init__(self, params, stream=None):
        self.L = load()
        self.stream = stream
        self.hp = _copy_struct(params)
        self.hd = T.HashData()
        check(self.L.vh_hash_data_alloc(C.byref(self.hd), C.byref(self.hp)), "vh_hash_data_alloc")
        self.reset()

    def close(self):
        if getattr(self, "hd", None) is not None and self.hd.d_hash:
            self.L.vh_stream_synchronize(self.stream)
            self.L.vh_hash_data_free(C.byref(self.hd))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_transform(self, transform, inverse):
        self.hp.m_rigidTransform = T.mat16(transform)
        self.hp.m_rigidTransformInverse = T.mat16(inverse)

    def reset(self):
        check(self.L.vh_reset(C.byref(self.hd), C.byref(self.hp), self.stream), "vh_reset")

    def reset_mutex(self):
        check(self.L.vh_reset_bucket_mutex(C.byref(self.hd), C.byref(self.hp), self.stream), "vh_reset_bucket_mutex")

    def alloc(self, frame, cp, bitmask_ptr=None, lock_token=T.LOCK_ENTRY):
        check(self.L.vh_alloc(C.byref(self.hd), C.byref(self.hp), C.byref(frame.data), C.byref(cp), bitmask_ptr, lock_token, self.stream), "vh_alloc")

    def compactify(self, cp):
        n = C.c_uint32()
        check(self.L.vh_compactify(C.byref(self.hd), C.byref(self.hp), C.byref(cp), C.byref(n), 0, self.stream), "vh_compactify")
        self.hp.m_numOccupiedBlocks = n.value
        return n.value

    def integrate(self, frame, cp):
        check(self.L.vh_integrate(C.byref(self.hd), C.byref(self.hp), C.byref(frame.data), C.byref(cp), self.stream), "vh_integrate")

    def integrate_fused(self, frame, cp, flags, lock_token, packed_ptr=None):
        check(self.L.vh_integrate_fused(C.byref(self.hd), C.byref(self.hp), C.byref(frame.data), C.byref(cp), flags, lock_token, None, 0,
                                        packed_ptr, self.stream), "vh_integrate_fused")

    def frame_job(self, frame, cp, bitmask_ptr=None, lock_token=T.LOCK_ENTRY, packed_ptr=None):
        """the alloc + compactify passes of a frame as a VhFrameJob (vh_alloc_job / vh_compactify_job / the co-launches)"""
        job = T.FrameJob()
        C.memmove(C.byref(job.hashData), C.byref(self.hd), C.sizeof(self.hd))
        C.memmove(C.byref(job.hashParams), C.byref(self.hp), C.sizeof(self.hp))
        C.memmove(C.byref(job.cam), C.byref(frame.data), C.sizeof(frame.data))
        C.memmove(C.byref(job.cp), C.byref(cp), C.sizeof(cp))
        job.d_bitMask = bitmask_ptr
        job.d_packedFrame = packed_ptr
        job.lockToken = lock_token
        return job

    def alloc_job(self, job):
        check(self.L.vh_alloc_job(C.byref(job), self.stream), "vh_alloc_job")

    def compactify_job(self, job):
        check(self.L.vh_compactify_job(C.byref(job), self.stream), "vh_compactify_job")

    def starve(self):
        check(self.L.vh_starve(C.byref(self.hd), C.byref(self.hp), self.stream), "vh_starve")

    def gc_identify(self, cp):
        check(self.L.vh_gc_identify(C.byref(self.hd), C.byref(self.hp), C.byref(cp), self.stream), "vh_gc_identify")

    def gc_free(self, lock_token=T.LOCK_ENTRY):
        check(self.L.vh_gc_free(C.byref(self.hd), C.byref(self.hp), lock_token, self.stream), "vh_gc_free")

    def hash_ops(self, ops):
        """ops: [n,5] int32 {op, x, y, z, arg} executed serially by one thread -> results[n]"""
        ops = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1, 5)
        d_ops = DeviceBuffer.from_numpy(ops, self.stream)
        d_res = DeviceBuffer(4 * len(ops))
        check(self.L.vh_debug_hash_ops(C.byref(self.hd), C.byref(self.hp), d_ops.ptr, d_res.ptr, len(ops), self.stream), "vh_debug_hash_ops")
        return d_res.download(np.int32, len(ops), self.stream)

    def stream_out(self, threads_per_part, start, radius, cam_pos, lock_token, capacity=4096):
        """pass 1 + pass 2 -> (descs, blocks)"""
        cnt = DeviceBuffer(4)
        check(self.L.vh_memset(cnt.ptr, 0, 4, self.stream), "memset")
        d_desc = DeviceBuffer(16 * capacity)
        check(self.L.vh_stream_out_pass1(C.byref(self.hd), C.byref(self.hp), threads_per_part, start, C.c_float(radius), f16(cam_pos),
                                         cnt.ptr, d_desc.ptr, capacity, lock_token, self.stream), "vh_stream_out_pass1")
        n = int(cnt.download(np.uint32, 1, self.stream)[0])
        assert n <= capacity
        d_blocks = DeviceBuffer(4096 * max(n, 1))
        check(self.L.vh_stream_out_pass2(C.byref(self.hd), C.byref(self.hp), d_desc.ptr, d_blocks.ptr, n, self.stream), "vh_stream_out_pass2")
        descs = d_desc.download(T.DESC_DTYPE, n, self.stream)
        blocks = d_blocks.download(T.VOXEL_DTYPE, n * T.SDF_BLOCK_VOXELS, self.stream).reshape(n, T.SDF_BLOCK_VOXELS)
        return descs, blocks

    def stream_in(self, descs, blocks, lock_token):
        descs = np.ascontiguousarray(descs, dtype=T.DESC_DTYPE)
        blocks = np.ascontiguousarray(blocks, dtype=T.VOXEL_DTYPE)
        n = len(descs)
        if n == 0:
            return
        d_desc, d_blocks = DeviceBuffer.from_numpy(descs, self.stream), DeviceBuffer.from_numpy(blocks, self.stream)
        prev = int(download(self.hd.d_heapCounter, np.uint32, 1, self.stream)[0])
        check(self.L.vh_stream_in_pass1(C.byref(self.hd), C.byref(self.hp), n, prev, d_desc.ptr, lock_token, self.stream), "vh_stream_in_pass1")
        check(self.L.vh_stream_in_pass2(C.byref(self.hd), C.byref(self.hp), n, prev, d_desc.ptr, d_blocks.ptr, self.stream), "vh_stream_in_pass2")
        new = np.array([prev - n], dtype=np.uint32)
        check(self.L.vh_memcpy_h2d(self.hd.d_heapCounter, new.ctypes.data, 4, self.stream), "heapCounter")

    def stream_in_settled(self, descs, blocks, lock_token):
        """vh_stream_in_device: the pass that reads the heap counter on the device and settles itself -- a block that
        finds no slot keeps no voxels and its SDF block is back on the heap when the call returns
        -> (indices into descs of the blocks that found no slot, whether the heap held too few free blocks)"""
        descs = np.ascontiguousarray(descs, dtype=T.DESC_DTYPE)
        blocks = np.ascontiguousarray(blocks, dtype=T.VOXEL_DTYPE)
        n = len(descs)
        d_desc, d_blocks = DeviceBuffer.from_numpy(descs, self.stream), DeviceBuffer.from_numpy(blocks, self.stream)
        d_failed, d_out = DeviceBuffer(4 * (1 + 2 * n)), DeviceBuffer(4 * (4 + n))
        check(self.L.vh_memset(d_failed.ptr, 0, d_failed.nbytes, self.stream), "memset")
        check(self.L.vh_memset(d_out.ptr, 0, d_out.nbytes, self.stream), "memset")
        check(self.L.vh_stream_in_device(C.byref(self.hd), C.byref(self.hp), n, d_desc.ptr, d_blocks.ptr, lock_token, d_failed.ptr, None, 0xFFFFFFFF,
                                         d_out.ptr, 1, self.stream), "vh_stream_in_device")
        out = d_out.download(np.uint32, 4 + n, self.stream)
        if out[2] != 1 or d_failed.download(np.uint32, 1 + 2 * n, self.stream)[0] != 0:
            raise RuntimeError("vh_stream_in_device: the pass did not settle (no tag published, or the scratch words were not cleared)")
        return out[4:4 + int(out[0])].astype(np.int64), bool(out[3])

    def merge_gather(self):
        """vh_merge_gather -> (descs in device memory, n): every occupied entry of this table as {pos, ptr}"""
        cap = int(self.hp.m_numSDFBlocks)
        d_desc, cnt = DeviceBuffer(16 * cap), DeviceBuffer(4)
        check(self.L.vh_merge_gather(C.byref(self.hd), C.byref(self.hp), d_desc.ptr, cap, cnt.ptr, self.stream), "vh_merge_gather")
        return d_desc, int(cnt.download(np.uint32, 1, self.stream)[0])

    def merge_blocks(self, descs, blocks, lock_token, block_offset=(0, 0, 0), source=None, n=None):
        """vh_merge_blocks: descs / blocks as numpy arrays (or DeviceBuffers); with source (a LauncherScene) the voxels
        are read from that scene's pool at descs' ptr and blocks is ignored (n: how many of a DeviceBuffer's descs count) -> the counts by name plus left_out_indices
        (the status is in the counts: nothing raises for it)"""
        off = (C.c_int32 * 3)(*[int(v) for v in block_offset])
        n_given = n
        if source is not None:
            d_desc, n = (descs, descs.nbytes // 16) if isinstance(descs, DeviceBuffer) else (DeviceBuffer.from_numpy(np.ascontiguousarray(descs, dtype=T.DESC_DTYPE), self.stream), len(descs))
            d_blocks, n = None, n_given if n_given is not None else n
        else:
            d_desc, d_blocks, n = _merge_upload(descs, blocks, self.stream)
        d_work = DeviceBuffer(self.L.vh_merge_work_bytes(n))
        d_left = DeviceBuffer(4 * max(n, 1))
        counts = (C.c_uint32 * len(T.MERGE_COUNTS))()
        check(self.L.vh_merge_blocks(C.byref(self.hd), C.byref(self.hp), n, d_desc.ptr, d_blocks.ptr if d_blocks is not None else None,
                                     source.hd.d_SDFBlocks if source is not None else None, off, lock_token, d_work.ptr, d_left.ptr, counts, self.stream),
              "vh_merge_blocks")
        return _merge_result(0, counts, (d_left, self.stream), "vh_merge_blocks")

    def cut_blocks(self, region_from_vox, shape, flags, lock_token, descs=None, blocks=None, staging_blocks=None, poison=None):
        """vh_cut_blocks on this table's entries (vh_merge_gather) or, with descs / blocks (numpy arrays, VH_CUT_KEEP
        only), on a plain block list.  region_from_vox: float32 [3, 4] (cut_region_transform).  A lifting call counts
        first and sizes the staging pool by the count unless staging_blocks says otherwise; poison: a byte the staging
        pool and its list are filled with before.  -> the counts by name (vhtypes.CUT_COUNTS) plus "code" (the call's
        return code: nothing raises), "descs" / "voxels" (the lifted list; empty unless the call lifted) and
        "staging_raw" (the list's and the pool's bytes after the call, or None)"""
        m = np.ascontiguousarray(region_from_vox, dtype=np.float32).reshape(12)
        if descs is None:
            (d_desc, n), d_blocks = self.merge_gather(), None
        else:
            descs = np.ascontiguousarray(descs, dtype=T.DESC_DTYPE)
            n = len(descs)
            blocks = np.ascontiguousarray(blocks, dtype=T.VOXEL_DTYPE).reshape(n, T.SDF_BLOCK_VOXELS)
            d_desc = DeviceBuffer.from_numpy(descs, self.stream) if n else DeviceBuffer(16)
            d_blocks = DeviceBuffer.from_numpy(blocks, self.stream) if n else DeviceBuffer(8)
        d_work = DeviceBuffer(self.L.vh_cut_work_bytes(n))
        counts = (C.c_uint32 * len(T.CUT_COUNTS))()

        def call(fl, d_out, d_staging, room):
            rc = self.L.vh_cut_blocks(C.byref(self.hd), C.byref(self.hp), n, d_desc.ptr, d_blocks.ptr if d_blocks is not None else None, m.ctypes.data,
                                      int(shape), int(fl), lock_token, d_work.ptr, d_out.ptr if d_out else None, d_staging.ptr if d_staging else None,
                                      room, counts, self.stream)
            return _counts_result(T.CUT_COUNTS, rc, counts, None, dict(code=rc, descs=np.zeros(0, T.DESC_DTYPE),
                                                                       voxels=np.zeros((0, T.SDF_BLOCK_VOXELS), T.VOXEL_DTYPE), staging_raw=None))

        if not (flags & T.CUT_LIFT) or (flags & T.CUT_COUNT_ONLY):
            return call(flags, None, None, 0)
        if staging_blocks is None:
            staging_blocks = call(flags | T.CUT_COUNT_ONLY, None, None, 0)["lifted"]
        room = int(staging_blocks)
        d_out, d_staging = DeviceBuffer(16 * max(room, 1)), DeviceBuffer(8 * T.SDF_BLOCK_VOXELS * max(room, 1))
        if poison is not None:
            check(self.L.vh_memset(d_out.ptr, int(poison), d_out.nbytes, self.stream), "memset")
            check(self.L.vh_memset(d_staging.ptr, int(poison), d_staging.nbytes, self.stream), "memset")
        out = call(flags, d_out, d_staging, room)
        out["staging_raw"] = (d_out.download(np.uint8, None, self.stream), d_staging.download(np.uint8, None, self.stream))
        if out["code"] == 0:
            out["descs"], out["voxels"] = _staged_list(d_out, d_staging, out["lifted"], self.stream)
        return out

    def deintegrate_blocks(self, frame, cp, transform, inverse, lock_token, flags=0):
        """vh_merge_gather on this table, then vh_deintegrate_blocks with the frame's pose and its inverse in a copy of the
        hash parameters -> the counts by name (vhtypes.DEINT_COUNTS) plus "code" (the call's return code: nothing raises)"""
        d_desc, n = self.merge_gather()
        hp = T.HashParams()
        C.memmove(C.byref(hp), C.byref(self.hp), C.sizeof(hp))
        hp.m_rigidTransform = T.mat16(transform)
        hp.m_rigidTransformInverse = T.mat16(inverse)
        d_work = DeviceBuffer(self.L.vh_deintegrate_work_bytes(n))
        counts = (C.c_uint32 * len(T.DEINT_COUNTS))()
        rc = self.L.vh_deintegrate_blocks(C.byref(self.hd), C.byref(hp), n, d_desc.ptr, C.byref(frame.data), C.byref(cp), int(flags), lock_token, d_work.ptr,
                                          counts, self.stream)
        return _counts_result(T.DEINT_COUNTS, rc, counts, None, {"code": rc})

    def align_begin(self, source, guess, pivot, radius):
        """vh_align_begin for `source` (a LauncherScene) against this scene -> (the state in device memory, the ticket
        word, the call's return code)"""
        m = np.ascontiguousarray(guess, dtype=np.float64).reshape(16)
        p = np.ascontiguousarray(pivot, dtype=np.float32).reshape(3)
        d_state, d_ticket = DeviceBuffer(C.sizeof(T.AlignState)), DeviceBuffer(4)
        check(self.L.vh_memset(d_state.ptr, 0, d_state.nbytes, self.stream), "memset")
        check(self.L.vh_memset(d_ticket.ptr, 0, 4, self.stream), "memset")
        rc = self.L.vh_align_begin(d_state.ptr, m.ctypes.data, float(source.hp.m_virtualVoxelSize), float(self.hp.m_virtualVoxelSize), p.ctypes.data,
                                   float(radius), self.stream)
        return d_state, d_ticket, rc

    def align_state(self, d_state, d_ticket=None):
        """the state read back -> vhtypes.align_state_dict, with "ticket" where the word is given"""
        st = T.AlignState.from_buffer_copy(d_state.download(np.uint8, C.sizeof(T.AlignState), self.stream).tobytes())
        out = T.align_state_dict(st)
        out["stripes"] = np.array(st.stripes[:], np.int64)
        out["raised"] = int(st.raised)
        if d_ticket is not None:
            out["ticket"] = int(d_ticket.download(np.uint32, 1, self.stream)[0])
        return out

    def align_step(self, source, d_state, d_ticket, descs=None, n=None, band=2.0, min_count=200, cond_thres=1e4, rot_thres=1e-5, trans_thres=1e-3,
                   steps=1):
        """vh_align_step, `steps` launches back to back: `source`'s blocks (vh_merge_gather on it, or descs: a
        DESC_DTYPE array or a DeviceBuffer with n) against this scene -> (align_state afterwards, the last return code)"""
        if descs is None:
            d_desc, n = source.merge_gather()
        elif isinstance(descs, DeviceBuffer):
            d_desc, n = descs, (descs.nbytes // 16 if n is None else n)
        else:
            descs = np.ascontiguousarray(descs, dtype=T.DESC_DTYPE)
            d_desc, n = (DeviceBuffer.from_numpy(descs, self.stream) if len(descs) else DeviceBuffer(16)), len(descs)
        rc = 0
        for _ in range(steps):
            rc = self.L.vh_align_step(C.byref(self.hd), C.byref(self.hp), C.byref(source.hd), C.byref(source.hp), n, d_desc.ptr, float(band), int(min_count),
                                      float(cond_thres), float(rot_thres), float(trans_thres), d_state.ptr, d_ticket.ptr, self.stream)
        return self.align_state(d_state, d_ticket), rc

    def align_rule(self, source, dst_vox_from_src_vox, pivot, inv_radius, band=2.0, descs=None):
        """vh_debug_align_rule: the per-voxel rule on `source`'s blocks (descs: DESC_DTYPE with the blocks' ptr, default
        vh_merge_gather on it) against this scene -> dict descs, kept [n, 512] bool, q [n, 512, 3], e [n, 512],
        g [n, 512, 3], terms [n, 512, 29] (float32; all zero where not kept)"""
        b = np.ascontiguousarray(dst_vox_from_src_vox, dtype=np.float32).reshape(12)
        p = np.ascontiguousarray(pivot, dtype=np.float32).reshape(3)
        if descs is None:
            d_desc, n = source.merge_gather()
        else:
            descs = np.ascontiguousarray(descs, dtype=T.DESC_DTYPE)
            d_desc, n = DeviceBuffer.from_numpy(descs, self.stream), len(descs)
        W, V = T.ALIGN_RULE_WORDS, T.SDF_BLOCK_VOXELS
        d_out = DeviceBuffer(4 * W * V * max(n, 1))
        check(self.L.vh_debug_align_rule(C.byref(self.hd), C.byref(self.hp), C.byref(source.hd), C.byref(source.hp), n, d_desc.ptr, b.ctypes.data, p.ctypes.data,
                                         float(inv_radius), float(band), d_out.ptr, self.stream), "vh_debug_align_rule")
        rec = d_out.download(np.float32, W * V * n, self.stream).reshape(n, V, W)
        return dict(descs=d_desc.download(T.DESC_DTYPE, n, self.stream), kept=rec[:, :, 0].view(np.uint32) != 0, q=rec[:, :, 1:4], e=rec[:, :, 4],
                    g=rec[:, :, 5:8], terms=rec[:, :, 8:])

    def resample_blocks(self, src_vox_from_dst_vox, dst_vox_from_src_vox, slots_log2=None):
        """vh_merge_gather on this table, then vh_resample_blocks, count and fill: this scene sampled on another lattice
        (the matrices of resample_voxel_transforms) -> the counts by name (vhtypes.RESAMPLE_COUNTS) plus "descs"
        (DESC_DTYPE [staged], ptr = 512 * the block's place in the staging pool) and "voxels" (VOXEL_DTYPE [staged, 512],
        in the descs' order): a list for merge_blocks.  slots_log2: the candidate table's size (default: 16 slots per
        source block).  A status is in the counts, with nothing staged: nothing raises for it."""
        a = np.ascontiguousarray(src_vox_from_dst_vox, dtype=np.float32).reshape(12)
        b = np.ascontiguousarray(dst_vox_from_src_vox, dtype=np.float32).reshape(12)
        d_src, n = self.merge_gather()
        counts = (C.c_uint32 * len(T.RESAMPLE_COUNTS))()

        def call(d_out, d_staging, room):
            check(self.L.vh_resample_blocks(C.byref(self.hd), C.byref(self.hp), n, d_src.ptr, a.ctypes.data, b.ctypes.data, slots_log2, d_work.ptr,
                                            d_out.ptr if d_out else None, d_staging.ptr if d_staging else None, room, counts, self.stream), "vh_resample_blocks")
            return {k: int(v) for k, v in zip(T.RESAMPLE_COUNTS, counts)}

        # without a size: as mergeSceneTransformed, 16 slots per source block, four times as many while the table fills, up
        # to two for each of the 6^3 candidates a source block can name
        grow = slots_log2 is None
        most = max(4, int(2 * 216 * max(n, 1) - 1).bit_length())
        if grow:
            slots_log2 = min(most, max(4, int(16 * max(n, 1) - 1).bit_length()))
        for _ in range(4):
            d_work = DeviceBuffer(self.L.vh_resample_work_bytes(slots_log2))
            out = call(None, None, 0)
            if not grow or not (out["status"] & T.RESAMPLE_TABLE_FULL) or slots_log2 == most:
                break
            slots_log2 = min(most, slots_log2 + 2)
        out.update(descs=np.zeros(0, T.DESC_DTYPE), voxels=np.zeros((0, T.SDF_BLOCK_VOXELS), T.VOXEL_DTYPE))
        room = out["candidates"]
        if out["status"] != 0 or room == 0:
            return out
        d_out, d_staging = DeviceBuffer(16 * room), DeviceBuffer(8 * T.SDF_BLOCK_VOXELS * room)
        out = call(d_out, d_staging, room)
        descs = d_out.download(T.DESC_DTYPE, out["staged"], self.stream)
        pool = d_staging.download(T.VOXEL_DTYPE, room * T.SDF_BLOCK_VOXELS, self.stream).reshape(room, T.SDF_BLOCK_VOXELS)
        out.update(descs=descs, voxels=np.ascontiguousarray(pool[descs["ptr"] // T.SDF_BLOCK_VOXELS]))
        return out

    def download(self, with_voxels=True):
        hp, hd, s = self.hp, self.hd, self.stream
        ne = hp.m_hashNumBuckets * T.HASH_BUCKET_SIZE
        out = dict(
            params=hp,
            hash=download(hd.d_hash, T.HASH_ENTRY_DTYPE, ne, s),
            heap=download(hd.d_heap, np.uint32, hp.m_numSDFBlocks, s),
            heap_counter=int(download(hd.d_heapCounter, np.uint32, 1, s)[0]),
            bucket_count=download(hd.d_bucketCount, np.uint32, hp.m_hashNumBuckets, s),
            bucket_bits=download(hd.d_bucketBits, np.uint32, (hp.m_hashNumBuckets + 31) // 32, s),
            state=download(hd.d_state, np.uint32, T.STATE_WORDS, s),
            compactified=download(hd.d_hashCompactified, T.HASH_ENTRY_DTYPE, hp.m_numOccupiedBlocks, s),
            decisions=download(hd.d_hashDecision, np.int32, hp.m_numOccupiedBlocks, s),
        )
        if with_voxels:
            out["sdf_blocks"] = download(hd.d_SDFBlocks, T.VOXEL_DTYPE, hp.m_numSDFBlocks * T.SDF_BLOCK_VOXELS, s)
        return out

    def state(self, with_voxels=True):
        d = self.download(with_voxels)
        canonical.check_invariants(d["hash"], d["heap"], d["heap_counter"], self.hp, d.get("sdf_blocks"))
        canonical.check_bucket_summary(d["hash"], d["bucket_count"], d["bucket_bits"], self.hp)
        snap = canonical.snapshot(d["hash"], d.get("sdf_blocks"), d["heap"], d["heap_counter"], self.hp, with_voxels)
        snap.update(compactified=d["compactified"], decisions=d["decisions"], raw=d)
        return snap


class CUDAMarchingCubesHashSDF:
    """Mirror of DSC/CUDAMarchingCubesHashSDF.h:8-67 over the C ABI."""

    def __init__(self, params, stream=None):
        self.L = load()
        self._params = params
        self.stream = stream
        h = C.c_void_p()
        check(self.L.vh_marching_cubes_create(C.byref(params), stream, C.byref(h)), "vh_marching_cubes_create")
        self.handle = h
        self._indexed_normals = False

    def close(self):
        if getattr(self, "handle", None):
            self.L.vh_marching_cubes_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def setOfflineProcessing(self, on):
        check(self.L.vh_marching_cubes_set_offline_processing(self.handle, 1 if on else 0), "setOfflineProcessing")

    def setIndexedNormals(self, on):
        """vertex normals for the indexed extractions (off by default): computed on the device after the weld; indexed()
        and mesh() then have a "normals" entry and saveMesh writes nx, ny, nz"""
        check(self.L.vh_marching_cubes_set_indexed_normals(self.handle, 1 if on else 0), "setIndexedNormals")
        self._indexed_normals = bool(on)

    def setIndexedComponentFilter(self, minFaces=0, largestOnly=False):
        """the component filter for the indexed extractions (off by default: 0, False): after the weld and the normals
        the mesh's connected components are labelled on the device and those of fewer than minFaces faces dropped, with
        largestOnly all but the largest; indexed_counts(), indexed(), mesh() and saveMesh then describe the filtered
        mesh, and indexed_component_stats() says what the unfiltered one held"""
        check(self.L.vh_marching_cubes_set_indexed_component_filter(self.handle, int(minFaces), 1 if largestOnly else 0), "setIndexedComponentFilter")

    def setIndexedClustering(self, cellsPerCluster=0):
        """decimation by vertex clustering for the indexed extractions (off by default: 0; 1 ... 64 turn it on): after
        the weld, and before normals and components, the vertices that fall into one cube of cellsPerCluster lattice
        points a side become one vertex at their mean; indexed_counts(), indexed(), mesh() and saveMesh then describe the
        clustered mesh, and indexed_cluster_stats() says what the pass did"""
        check(self.L.vh_marching_cubes_set_indexed_clustering(self.handle, int(cellsPerCluster)), "setIndexedClustering")

    def indexed_cluster_stats(self):
        """of the last indexed extraction: vertices, faces, status, collapsed, duplicates, unused_clusters; all 0 when
        it ran with clustering off"""
        out = (C.c_uint32 * 6)()
        check(self.L.vh_marching_cubes_get_indexed_cluster_stats(self.handle, out), "get_indexed_cluster_stats")
        return {k: int(out[i]) for i, k in enumerate(T.CLUSTER_COUNTS)}

    def setIndexedSmoothing(self, iterations=0, lam=0.5, mu=-0.53, keepBoundary=True):
        """Taubin smoothing for the indexed extractions (off by default: 0; 1 ... 100 iterations turn it on): after the
        clustering, and before normals and components, the positions are replaced by that many lambda | mu iterations
        in fixed point; indexed(), mesh() and saveMesh then carry the smoothed positions, and indexed_smooth_stats()
        says what the pass did.  The factors go to units of 2^-16 by rint; ValueError above 1 in magnitude"""
        check(self.L.vh_marching_cubes_set_indexed_smoothing(self.handle, int(iterations), T.smooth_factor_q16(lam), T.smooth_factor_q16(mu), 1 if keepBoundary else 0),
              "setIndexedSmoothing")

    def indexed_smooth_stats(self):
        """of the last indexed extraction: moved, boundary_vertices, isolated_vertices, status, edges, boundary_edges;
        all 0 when it ran with smoothing off"""
        out = (C.c_uint32 * 6)()
        check(self.L.vh_marching_cubes_get_indexed_smooth_stats(self.handle, out), "get_indexed_smooth_stats")
        return {k: int(out[i]) for i, k in enumerate(T.SMOOTH_COUNTS)}

    def indexed_component_stats(self):
        """of the last indexed extraction: components (with a face), faceless_vertices, kept_components, kept_vertices,
        kept_faces, largest_faces; all 0 when it ran with the filter off"""
        out = (C.c_uint32 * 6)()
        check(self.L.vh_marching_cubes_get_indexed_component_stats(self.handle, out), "get_indexed_component_stats")
        return {k: int(out[i]) for i, k in enumerate(T.COMPONENTS_COUNTS)}

    def extractIsoSurface(self, hashData, hashParams, minCorner=(0, 0, 0), maxCorner=(0, 0, 0), boxEnabled=False, copy=True):
        check(self.L.vh_marching_cubes_extract_iso_surface(self.handle, C.byref(hashData), C.byref(hashParams), f16(minCorner),
                                                           f16(maxCorner), int(boxEnabled), int(copy)), "extractIsoSurface")

    def extractIsoSurfaceWithoutCopy(self, hashData, hashParams, minCorner=(0, 0, 0), maxCorner=(0, 0, 0), boxEnabled=False):
        self.extractIsoSurface(hashData, hashParams, minCorner, maxCorner, boxEnabled, copy=False)

    def extractIsoSurfaceChunkGrid(self, chunkGrid, camPos, radius):
        check(self.L.vh_marching_cubes_extract_iso_surface_chunk_grid(self.handle, chunkGrid.handle, f16(camPos), radius),
              "extractIsoSurface(chunkGrid)")

    def extractIsoSurfaceIndexed(self, hashData, hashParams, minCorner=(0, 0, 0), maxCorner=(0, 0, 0), boxEnabled=False):
        """the extraction with the soup welded on the device: REPLACES the mesh buffer with the indexed mesh (mesh(),
        saveMesh write it as it is); indexed() has it with the keys, sources() the records it was welded by"""
        check(self.L.vh_marching_cubes_extract_iso_surface_indexed(self.handle, C.byref(hashData), C.byref(hashParams), f16(minCorner),
                                                                   f16(maxCorner), int(boxEnabled)), "extractIsoSurfaceIndexed")

    def beginIndexed(self):
        """starts an indexed extraction that is made box by box: appendIndexed any number of times, then finishIndexed"""
        check(self.L.vh_marching_cubes_begin_indexed(self.handle), "beginIndexed")

    def appendIndexed(self, hashData, hashParams, minCorner=(0, 0, 0), maxCorner=(0, 0, 0), boxEnabled=False):
        """one extraction in a box, appended to the accumulation; boxes may overlap: a cell is taken from the first box
        that has it"""
        check(self.L.vh_marching_cubes_append_indexed(self.handle, C.byref(hashData), C.byref(hashParams), f16(minCorner), f16(maxCorner),
                                                      int(boxEnabled)), "appendIndexed")

    def finishIndexed(self):
        """downloads the accumulated mesh and REPLACES the mesh buffer with it, as extractIsoSurfaceIndexed does"""
        check(self.L.vh_marching_cubes_finish_indexed(self.handle), "finishIndexed")

    def extractIsoSurfaceIndexedChunkGrid(self, chunkGrid, camPos, radius):
        """the walk of extractIsoSurfaceChunkGrid with every chunk appended to one accumulation: the indexed mesh of a
        streamed scene"""
        check(self.L.vh_marching_cubes_extract_iso_surface_indexed_chunk_grid(self.handle, chunkGrid.handle, f16(camPos), radius),
              "extractIsoSurfaceIndexed(chunkGrid)")

    def liveBegin(self):
        """starts a live mesh: until liveEnd the object's triangles() and sources() are a cache that liveUpdate brings
        up to date with the table, and every extraction on the object raises VhError (VH_ERR_BAD_ARGUMENT)"""
        check(self.L.vh_marching_cubes_live_begin(self.handle), "liveBegin")

    def liveUpdate(self, hashData, hashParams, boxEnabled=False, raise_on_status=True):
        """one update of the live mesh: re-extracts the resident blocks within one block of a block that changed since
        the last update -> the counts of T.LIVE_COUNTS and `status`.  An overflow or a block out of range raises VhError
        and leaves the cache invalid (the next update is a full one); with raise_on_status=False it comes back as `code`"""
        out = (C.c_uint32 * 9)()
        code = self.L.vh_marching_cubes_live_update(self.handle, C.byref(hashData), C.byref(hashParams), int(boxEnabled), out)
        if code != 0 and (raise_on_status or out[8] == 0):
            check(code, "liveUpdate")
        return dict({k: int(out[i]) for i, k in enumerate(T.LIVE_COUNTS)}, status=int(out[8]), code=int(code))

    def liveInvalidate(self):
        """forgets every record and the cache: the next liveUpdate is a full extraction (the digests can collide)"""
        check(self.L.vh_marching_cubes_live_invalidate(self.handle), "liveInvalidate")

    def liveIndexed(self):
        """welds the cache and runs the indexed passes that are on: REPLACES the mesh buffer as extractIsoSurfaceIndexed
        does (indexed(), mesh(), saveMesh); the cache stays"""
        check(self.L.vh_marching_cubes_live_indexed(self.handle), "liveIndexed")

    def liveEnd(self):
        check(self.L.vh_marching_cubes_live_end(self.handle), "liveEnd")

    def indexed_stats(self):
        """of the last accumulated extraction: vertices, faces, status, cells, dropped (triangles of cells an earlier
        append had), rehashes (doublings of the table); all 0 after a one-shot extraction"""
        out = (C.c_uint32 * 6)()
        check(self.L.vh_marching_cubes_get_indexed_stats(self.handle, out), "get_indexed_stats")
        return {k: int(out[i]) for i, k in enumerate(T.WELD_ACCUM_COUNTS)}

    def indexed_counts(self):
        out = (C.c_uint32 * 3)()
        check(self.L.vh_marching_cubes_get_indexed_counts(self.handle, out), "get_indexed_counts")
        return dict(vertices=int(out[0]), faces=int(out[1]), status=int(out[2]))

    def indexed(self):
        """device mesh of the last indexed extraction -> vertices (V,3) f32, colors (V,3) f32, keys (V,) u64, faces (F,3) u32;
        with setIndexedNormals(True), and an extraction made since, also normals (V,3) f32"""
        n = self.indexed_counts()
        out = _welded_arrays(n["vertices"], n["faces"], "download_indexed",
                             lambda v, k, f, nv, nf: self.L.vh_marching_cubes_download_indexed(self.handle, v, k, f))
        if self._indexed_normals:
            out["normals"] = np.zeros((n["vertices"], 3), dtype=np.float32)
            check(self.L.vh_marching_cubes_download_indexed_normals(self.handle, out["normals"].ctypes.data), "download_indexed_normals")
        return out

    def sources(self):
        """source records of the last indexed extraction, beside triangles() -> numpy array of T.TRIANGLE_SOURCE_DTYPE"""
        n = min(self.counts()["triangles"], self._params.m_maxNumTriangles)
        out = np.zeros(n, dtype=T.TRIANGLE_SOURCE_DTYPE)
        if n:
            check(self.L.vh_marching_cubes_download_sources(self.handle, out.ctypes.data, n), "download_sources")
        return out

    def copyTrianglesToCPU(self):
        check(self.L.vh_marching_cubes_copy_triangles_to_cpu(self.handle), "copyTrianglesToCPU")

    def clearMeshBuffer(self):
        check(self.L.vh_marching_cubes_clear_mesh_buffer(self.handle), "clearMeshBuffer")

    def counts(self):
        out = (C.c_uint32 * 2)()
        check(self.L.vh_marching_cubes_get_counts(self.handle, out), "get_counts")
        return dict(triangles=int(out[0]), occupied_blocks=int(out[1]))

    def triangles(self):
        """device triangle buffer of the last extraction -> numpy array of T.TRIANGLE_DTYPE"""
        n = min(self.counts()["triangles"], self._params.m_maxNumTriangles)
        out = np.zeros(n, dtype=T.TRIANGLE_DTYPE)
        if n:
            check(self.L.vh_marching_cubes_download_triangles(self.handle, out.ctypes.data, n), "download_triangles")
        return out

    def mesh(self):
        sz = (C.c_uint64 * 2)()
        check(self.L.vh_marching_cubes_get_mesh_size(self.handle, sz), "get_mesh_size")
        v = np.zeros((int(sz[0]), 3), dtype=np.float32)
        c = np.zeros((int(sz[0]), 4), dtype=np.float32)
        f = np.zeros(int(sz[1]), dtype=np.uint32)
        check(self.L.vh_marching_cubes_get_mesh(self.handle, v.ctypes.data, c.ctypes.data, f.ctypes.data), "get_mesh")
        out = dict(vertices=v, colors=c, faces=f.reshape(-1, 3))
        if self._indexed_normals:  # (3 per vertex, or none: whatever appended to the buffer since has dropped them)
            nn = C.c_uint64()
            check(self.L.vh_marching_cubes_get_mesh_normals_size(self.handle, C.byref(nn)), "get_mesh_normals_size")
            out["normals"] = np.zeros((int(nn.value) // 3, 3), dtype=np.float32)
            check(self.L.vh_marching_cubes_get_mesh_normals(self.handle, out["normals"].ctypes.data), "get_mesh_normals")
        return out

    def saveMesh(self, filename, transform=None, overwriteExistingFile=False):
        t = f16(transform) if transform is not None else None
        check(self.L.vh_marching_cubes_save_mesh(self.handle, filename.encode(), t, int(overwriteExistingFile)), "saveMesh")


def live_mesh_digest(hashData, hashParams, entry_indices, stream=None):
    """vh_live_mesh_digest: the 64-bit digests of the blocks of the listed hash entries (0 for a free entry) -> (n,) u64"""
    idx = np.ascontiguousarray(entry_indices, dtype=np.uint32).ravel()
    if len(idx) == 0:
        return np.zeros(0, dtype=np.uint64)
    d_idx, d_out = DeviceBuffer.from_numpy(idx, stream), DeviceBuffer(8 * len(idx))
    try:
        check(load().vh_live_mesh_digest(C.byref(hashData), C.byref(hashParams), d_idx.ptr, len(idx), d_out.ptr, stream), "vh_live_mesh_digest")
        return d_out.download(np.uint64, len(idx), stream)
    finally:
        d_idx.free()
        d_out.free()


class LiveMesh:
    """The live mesh at launcher level: vh_live_mesh_* over buffers of its own (vh_marching_cubes_data_alloc, the source
    records, vh_live_mesh_data_alloc).  params: T.MarchingCubesParams with the box off."""

    def __init__(self, params, numSDFBlocks, stream=None):
        self.L = load()
        self.stream = stream
        self._params = _copy_struct(params)
        self._params.m_boxEnabled = 0
        self.data, self.live, self.d_sources = T.MarchingCubesData(), T.LiveMeshData(), C.c_void_p()
        check(self.L.vh_marching_cubes_data_alloc(C.byref(self.data), C.byref(self._params)), "vh_marching_cubes_data_alloc")
        check(self.L.vh_reset_marching_cubes(C.byref(self.data), stream), "vh_reset_marching_cubes")
        check(self.L.vh_malloc(C.byref(self.d_sources), 16 * int(self._params.m_maxNumTriangles)), "vh_malloc")
        check(self.L.vh_live_mesh_data_alloc(C.byref(self.live), int(numSDFBlocks), int(self._params.m_maxNumTriangles)), "vh_live_mesh_data_alloc")

    def close(self):
        if getattr(self, "live", None) is not None:
            self.L.vh_live_mesh_data_free(C.byref(self.live))
            self.L.vh_marching_cubes_data_free(C.byref(self.data))
            self.L.vh_free(self.d_sources)
            self.live = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        check(self.L.vh_live_mesh_reset(C.byref(self.live), self.stream), "vh_live_mesh_reset")
        check(self.L.vh_reset_marching_cubes(C.byref(self.data), self.stream), "vh_reset_marching_cubes")

    def enqueue(self, hashData, hashParams):
        """vh_live_mesh_update alone: the counts are read by counts()"""
        check(self.L.vh_live_mesh_update(C.byref(hashData), C.byref(hashParams), C.byref(self.data), C.byref(self.d_sources), C.byref(self.live), self.stream),
              "vh_live_mesh_update")

    def counts(self, raise_on_status=True):
        out = (C.c_uint32 * 9)()
        code = self.L.vh_live_mesh_get_counts(C.byref(self.live), out, self.stream)
        if code != 0 and (raise_on_status or out[8] == 0):
            check(code, "vh_live_mesh_get_counts")
        return dict({k: int(out[i]) for i, k in enumerate(T.LIVE_COUNTS)}, status=int(out[8]), code=int(code))

    def update(self, hashData, hashParams, raise_on_status=True):
        self.enqueue(hashData, hashParams)
        return self.counts(raise_on_status)

    def soup(self, n):
        """the first n triangles of the cache and their records (n: the last update's total)"""
        tris, srcs = np.zeros(int(n), dtype=T.TRIANGLE_DTYPE), np.zeros(int(n), dtype=T.TRIANGLE_SOURCE_DTYPE)
        if n:
            check(self.L.vh_memcpy_d2h(tris.ctypes.data, self.data.d_triangles, tris.nbytes, self.stream), "vh_memcpy_d2h")
            check(self.L.vh_memcpy_d2h(srcs.ctypes.data, self.d_sources, srcs.nbytes, self.stream), "vh_memcpy_d2h")
        return tris, srcs

    def records(self):
        out = np.zeros(int(self.live.m_numSDFBlocks), dtype=T.LIVE_RECORD_DTYPE)
        check(self.L.vh_memcpy_d2h(out.ctypes.data, self.live.d_records, out.nbytes, self.stream), "vh_memcpy_d2h")
        return out


def mesh_weld_key(cell, edge, snap):
    """vh_mesh_weld_key: the 64-bit key of a vertex (host side, no GPU); raises VhError when it has none"""
    key = C.c_uint64()
    check(load().vh_mesh_weld_key((C.c_int32 * 3)(*[int(v) for v in cell]), int(edge), int(snap), C.byref(key)), "vh_mesh_weld_key")
    return int(key.value)


def _upload_soup(triangles, sources, stream):
    """a soup (T.TRIANGLE_DTYPE) and its records (T.TRIANGLE_SOURCE_DTYPE) on the device -> the two buffers and the triangle count"""
    tris = np.ascontiguousarray(triangles, dtype=T.TRIANGLE_DTYPE).ravel()
    srcs = np.ascontiguousarray(sources, dtype=T.TRIANGLE_SOURCE_DTYPE).ravel()
    if len(tris) != len(srcs):
        raise ValueError("one source record per triangle")
    return DeviceBuffer.from_numpy(tris, stream), DeviceBuffer.from_numpy(srcs, stream), len(tris)


def _check_weld(code, status, raise_on_status, what):
    """what a weld's get_counts returned: a HIP error always raises; a status raises if asked to, and a code without one always"""
    if code < 0 or (code != 0 and (raise_on_status or status == 0)):
        check(code, what)


def _welded_arrays(nv, nf, what, download):
    """the arrays of a welded mesh of nv vertices and nf faces, filled by download(vertices, keys, faces, nv, nf) -> dict"""
    v = np.zeros(int(nv), dtype=T.VERTEX_DTYPE)
    k = np.zeros(int(nv), dtype=np.uint64)
    f = np.zeros((int(nf), 3), dtype=np.uint32)
    check(download(v.ctypes.data, k.ctypes.data, f.ctypes.data, len(v), len(f)), what)
    return dict(vertices=np.ascontiguousarray(v["p"]), colors=np.ascontiguousarray(v["c"]), keys=k, faces=f)


def mesh_weld(triangles, sources, slots_log2=0, raise_on_status=True, stream=None):
    """vh_mesh_weld on hand-made input: a soup (T.TRIANGLE_DTYPE) and its records (T.TRIANGLE_SOURCE_DTYPE) ->
    vertices, colors, keys, faces as CUDAMarchingCubesHashSDF.indexed(), and counts / status / code of the weld.  A full
    table or a key out of range raises VhError, or with raise_on_status=False comes back as `code` beside empty arrays."""
    L = load()
    d_tris, d_srcs, n = _upload_soup(triangles, sources, stream)
    w = T.MeshWeldData()
    check(L.vh_mesh_weld_data_alloc(C.byref(w), n, slots_log2), "vh_mesh_weld_data_alloc")
    slots = int(w.m_slotsLog2)
    try:
        check(L.vh_mesh_weld(d_tris.ptr, d_srcs.ptr, n, C.byref(w), slots_log2, stream), "vh_mesh_weld")
        counts = (C.c_uint32 * 3)()
        code = L.vh_mesh_weld_get_counts(C.byref(w), counts, stream)
        _check_weld(code, counts[2], raise_on_status, "vh_mesh_weld")
        out = _welded_arrays(counts[0], counts[1], "vh_mesh_weld_download",
                             lambda v, k, f, nv, nf: L.vh_mesh_weld_download(C.byref(w), v, k, f, nv, nf, stream))
    finally:
        L.vh_mesh_weld_data_free(C.byref(w))
        d_tris.free()
        d_srcs.free()
    return dict(out, counts=(int(counts[0]), int(counts[1])), status=int(counts[2]), code=int(code), slots_log2=slots)


def mesh_normals_default_scale_log2(voxel_size):
    """vh_mesh_normals_default_scale_log2 (host side, no GPU); raises VhError for a voxel size it refuses"""
    out = C.c_int32()
    check(load().vh_mesh_normals_default_scale_log2(float(voxel_size), C.byref(out)), "vh_mesh_normals_default_scale_log2")
    return int(out.value)


def mesh_vertex_normals(vertices, keys, faces, scale_log2, raise_on_status=True, stream=None):
    """vh_mesh_vertex_normals on hand-made input: vertices (V,3) f32 positions, or T.VERTEX_DTYPE records; keys (V,) u64;
    faces (F,3) u32 -> normals (V,3) f32, acc (V,3) i64 (the fixed-point sums), status, code.  A status raises VhError
    (VH_ERR_BAD_ARGUMENT), or with raise_on_status=False comes back as `code` beside the all-zero normals."""
    L = load()
    v = np.asarray(vertices)
    if v.dtype != T.VERTEX_DTYPE:
        p = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3)
        v = np.zeros(len(p), dtype=T.VERTEX_DTYPE)
        v["p"] = p
    v = np.ascontiguousarray(v).ravel()
    k = np.ascontiguousarray(keys, dtype=np.uint64).ravel()
    f = np.ascontiguousarray(faces, dtype=np.uint32).reshape(-1, 3)
    if len(k) != len(v):
        raise ValueError("one key per vertex")
    nv, nf = len(v), len(f)
    bufs = [DeviceBuffer.from_numpy(v, stream), DeviceBuffer.from_numpy(k, stream), DeviceBuffer.from_numpy(f, stream),
            DeviceBuffer(24 * nv), DeviceBuffer(12 * nv), DeviceBuffer(4)]
    try:
        d_v, d_k, d_f, d_acc, d_n, d_st = bufs
        check(L.vh_mesh_vertex_normals(d_v.ptr, d_k.ptr, d_f.ptr, nv, nf, int(scale_log2), d_acc.ptr, d_n.ptr, d_st.ptr, stream), "vh_mesh_vertex_normals")
        status = int(d_st.download(np.uint32, 1, stream)[0])
        normals = d_n.download(np.float32, 3 * nv, stream).reshape(-1, 3)
        acc = d_acc.download(np.int64, 3 * nv, stream).reshape(-1, 3)
    finally:
        for b in bufs:
            b.free()
    code = 4 if status else 0  # VH_ERR_BAD_ARGUMENT for either bit, as for the weld's key range
    if code and raise_on_status:
        check(code, f"vh_mesh_vertex_normals (status {status})")
    return dict(normals=normals, acc=acc, status=status, code=code)


def _vertex_records(vertices, colors=None):
    """(V,3) positions with (V,3) colours or none, or T.VERTEX_DTYPE records -> contiguous records"""
    v = np.asarray(vertices)
    if v.dtype != T.VERTEX_DTYPE:
        p = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3)
        v = np.zeros(len(p), dtype=T.VERTEX_DTYPE)
        v["p"] = p
        if colors is not None:
            v["c"] = np.ascontiguousarray(colors, dtype=np.float32).reshape(len(p), 3)
    return np.ascontiguousarray(v).ravel()


def mesh_components(keys, faces, stream=None, guard=0):
    """vh_mesh_components on hand-made input: keys (V,) u64, faces (F,3) u32 -> root (V,) u32 (the index of each
    vertex's component's first vertex by (key, index)), face_count (V,) u32 (at the roots), status, code (4 =
    VH_ERR_BAD_ARGUMENT for either status bit).  guard: the last `guard` keys are not vertices but room behind them, with
    that many words of 0xa5a5a5a5 behind root and face_count on the device, returned as root_guard / count_guard."""
    L = load()
    k = np.ascontiguousarray(keys, dtype=np.uint64).ravel()
    f = np.ascontiguousarray(faces, dtype=np.uint32).reshape(-1, 3)
    nv, nf = len(k) - guard, len(f)
    fill = np.full(nv + guard, 0xa5a5a5a5, dtype=np.uint32)
    bufs = [DeviceBuffer.from_numpy(k, stream), DeviceBuffer.from_numpy(f, stream), DeviceBuffer.from_numpy(fill, stream), DeviceBuffer.from_numpy(fill, stream),
            DeviceBuffer(4)]
    try:
        d_k, d_f, d_root, d_cnt, d_st = bufs
        check(L.vh_mesh_components(d_k.ptr, d_f.ptr, nv, nf, d_root.ptr, d_cnt.ptr, d_st.ptr, stream), "vh_mesh_components")
        status = int(d_st.download(np.uint32, 1, stream)[0])
        root = d_root.download(np.uint32, nv + guard, stream)
        cnt = d_cnt.download(np.uint32, nv + guard, stream)
    finally:
        for b in bufs:
            b.free()
    return dict(root=root[:nv], face_count=cnt[:nv], root_guard=root[nv:], count_guard=cnt[nv:], status=status, code=4 if status else 0)


def mesh_components_filter(vertices, colors, keys, faces, min_faces=0, largest_only=False, normals=None, raise_on_status=True, stream=None):
    """vh_mesh_components, then vh_mesh_components_filter, on hand-made input: vertices (V,3) f32 with colors (V,3) f32
    or None, or T.VERTEX_DTYPE records; keys (V,) u64; faces (F,3) u32; normals (V,3) f32 or None -> the filtered
    vertices, colors, keys, faces (and normals) as mesh_weld(), root and face_count of the labelling, counts (the six by
    name), status, code.  A status raises VhError (VH_ERR_BAD_ARGUMENT), or with raise_on_status=False comes back as
    `code` beside an empty mesh."""
    L = load()
    v = _vertex_records(vertices, colors)
    k = np.ascontiguousarray(keys, dtype=np.uint64).ravel()
    f = np.ascontiguousarray(faces, dtype=np.uint32).reshape(-1, 3)
    if len(k) != len(v):
        raise ValueError("one key per vertex")
    nv, nf = len(v), len(f)
    n = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(nv, 3)
    bufs = [DeviceBuffer.from_numpy(v, stream), DeviceBuffer.from_numpy(k, stream), DeviceBuffer.from_numpy(f, stream),
            DeviceBuffer(4 * nv), DeviceBuffer(4 * nv), DeviceBuffer(4), DeviceBuffer(4 * nv), DeviceBuffer(16),
            DeviceBuffer(24 * nv), DeviceBuffer(8 * nv), DeviceBuffer(12 * nf), DeviceBuffer(24)]
    if n is not None:
        bufs += [DeviceBuffer.from_numpy(n, stream), DeviceBuffer(12 * nv)]
    try:
        d_v, d_k, d_f, d_root, d_cnt, d_st, d_new, d_best, d_ov, d_ok, d_of, d_counts = bufs[:12]
        d_n, d_on = (bufs[12].ptr, bufs[13].ptr) if n is not None else (None, None)
        check(L.vh_mesh_components(d_k.ptr, d_f.ptr, nv, nf, d_root.ptr, d_cnt.ptr, d_st.ptr, stream), "vh_mesh_components")
        check(L.vh_mesh_components_filter(d_v.ptr, d_k.ptr, d_n, d_f.ptr, nv, nf, d_root.ptr, d_cnt.ptr, d_st.ptr, int(min_faces), 1 if largest_only else 0,
                                          d_new.ptr, d_best.ptr, d_ov.ptr, d_ok.ptr, d_on, d_of.ptr, d_counts.ptr, stream), "vh_mesh_components_filter")
        status = int(d_st.download(np.uint32, 1, stream)[0])
        counts = d_counts.download(np.uint32, 6, stream)
        kv, kf = int(counts[3]), int(counts[4])
        ov = d_ov.download(T.VERTEX_DTYPE, kv, stream)
        out = dict(vertices=np.ascontiguousarray(ov["p"]), colors=np.ascontiguousarray(ov["c"]), keys=d_ok.download(np.uint64, kv, stream),
                   faces=d_of.download(np.uint32, 3 * kf, stream).reshape(-1, 3),
                   root=d_root.download(np.uint32, nv, stream), face_count=d_cnt.download(np.uint32, nv, stream))
        if n is not None:
            out["normals"] = bufs[13].download(np.float32, 3 * kv, stream).reshape(-1, 3)
    finally:
        for b in bufs:
            b.free()
    code = 4 if status else 0  # VH_ERR_BAD_ARGUMENT for either bit, as for the normals
    if code and raise_on_status:
        check(code, f"vh_mesh_components (status {status})")
    return dict(out, counts={name: int(counts[i]) for i, name in enumerate(T.COMPONENTS_COUNTS)}, status=status, code=code)


def mesh_cluster_key(vertex_key, cells_per_cluster):
    """vh_mesh_cluster_key (host side, no GPU): the key of the cluster a vertex key falls into"""
    out = C.c_uint64()
    check(load().vh_mesh_cluster_key(int(vertex_key), int(cells_per_cluster), C.byref(out)), "vh_mesh_cluster_key")
    return int(out.value)


def mesh_cluster_default_scale_log2(voxel_size):
    """vh_mesh_cluster_default_scale_log2 (host side, no GPU)"""
    out = C.c_int32()
    check(load().vh_mesh_cluster_default_scale_log2(float(voxel_size), C.byref(out)), "vh_mesh_cluster_default_scale_log2")
    return int(out.value)


def mesh_cluster(vertices, colors, keys, faces, cells_per_cluster, scale_log2, cluster_slots_log2=0, face_slots_log2=0, raise_on_status=True,
                 stream=None, guard=0):
    """vh_mesh_cluster on hand-made input: vertices (V,3) f32 with colors (V,3) f32 or None, or T.VERTEX_DTYPE records;
    keys (V,) u64; faces (F,3) u32 -> the clustered vertices, colors, keys, faces as mesh_weld(), counts (the six by
    name), status, code.  cluster_slots_log2 / face_slots_log2: the tables' sizes (0: the default, twice the vertices
    and faces); smaller ones fill.  A status raises VhError (VH_ERR_STAGING_OVERFLOW for a full table alone, else
    VH_ERR_BAD_ARGUMENT), or with raise_on_status=False comes back as `code` beside an empty mesh.  guard: that many
    words of 0xa5a5a5a5 behind the per-vertex slot array on the device, returned as slot_guard: where a face index >= V
    would lead."""
    L = load()
    v = _vertex_records(vertices, colors)
    k = np.ascontiguousarray(keys, dtype=np.uint64).ravel()
    f = np.ascontiguousarray(faces, dtype=np.uint32).reshape(-1, 3)
    if len(k) != len(v):
        raise ValueError("one key per vertex")
    nv, nf = len(v), len(f)

    def log2_for(n, given):
        out = C.c_uint32()
        check(L.vh_mesh_cluster_default_slots_log2(n, C.byref(out)), "vh_mesh_cluster_default_slots_log2")
        return int(given) if given else int(out.value)
    cl, fl = log2_for(nv, cluster_slots_log2), log2_for(nf, face_slots_log2)
    cs, fs = 1 << cl, 1 << fl
    sizes = [8 * cs, 48 * cs, 4 * cs, 4 * cs, 4 * max(nv, 1), 8 * fs, 4 * fs, 4 * fs, 8, 24 * max(nv, 1), 8 * max(nv, 1), 12 * max(nf, 1), 24]
    bufs = [DeviceBuffer.from_numpy(v, stream), DeviceBuffer.from_numpy(k, stream), DeviceBuffer.from_numpy(f if nf else np.zeros((1, 3), np.uint32), stream)]
    bufs += [DeviceBuffer(n) for n in sizes]
    try:
        d_v, d_k, d_f = bufs[:3]
        if guard:
            bufs[7].free()
            bufs[7] = DeviceBuffer.from_numpy(np.full(nv + guard, 0xa5a5a5a5, dtype=np.uint32), stream)
        data = T.MeshClusterData(*[b.ptr for b in bufs[3:]], cl, fl)
        check(L.vh_mesh_cluster(d_v.ptr, d_k.ptr, d_f.ptr, nv, nf, int(cells_per_cluster), int(scale_log2), C.byref(data), stream), "vh_mesh_cluster")
        counts = bufs[15].download(np.uint32, 6, stream)
        status = int(counts[2])
        ov = bufs[12].download(T.VERTEX_DTYPE, int(counts[0]), stream)
        out = dict(vertices=np.ascontiguousarray(ov["p"]), colors=np.ascontiguousarray(ov["c"]), keys=bufs[13].download(np.uint64, int(counts[0]), stream),
                   faces=bufs[14].download(np.uint32, 3 * int(counts[1]), stream).reshape(-1, 3))
        if guard:
            out["slot_guard"] = bufs[7].download(np.uint32, nv + guard, stream)[nv:]
    finally:
        for b in bufs:
            b.free()
    code = 0 if status == 0 else 2 if status == T.CLUSTER_TABLE_FULL else 4  # VH_ERR_STAGING_OVERFLOW, VH_ERR_BAD_ARGUMENT
    if code and raise_on_status:
        check(code, f"vh_mesh_cluster (status {status})")
    return dict(out, counts={name: int(counts[i]) for i, name in enumerate(T.CLUSTER_COUNTS)}, status=status, code=code)


def mesh_smooth(vertices, colors, keys, faces, iterations, lam=0.5, mu=-0.53, keep_boundary=True, scale_log2=21, edge_slots_log2=None, raise_on_status=True,
                stream=None, guard=0, factors_q16=None):
    """vh_mesh_smooth on hand-made input: vertices (V,3) f32 with colors (V,3) f32 or None, or T.VERTEX_DTYPE records;
    keys (V,) u64; faces (F,3) u32 -> the mesh with the smoothed vertices (vertices, colors, keys, faces as mesh_weld();
    keys and faces are the input's), counts (the six by name), status, code.  lam, mu go to units of 2^-16 by rint, or
    factors_q16 = (lambdaQ16, muQ16) gives them as they are.  edge_slots_log2: the edge table's size (None: the
    default, six times the faces); a smaller one fills.  A status raises VhError (VH_ERR_STAGING_OVERFLOW for a full
    table alone, else VH_ERR_BAD_ARGUMENT), or with raise_on_status=False comes back as `code` beside an empty mesh.
    guard: that many words of 0xa5a5a5a5 behind the per-vertex degree, flag, position and sum arrays on the device,
    returned as guards: where a face index >= V would lead."""
    L = load()
    v = _vertex_records(vertices, colors)
    k = np.ascontiguousarray(keys, dtype=np.uint64).ravel()
    f = np.ascontiguousarray(faces, dtype=np.uint32).reshape(-1, 3)
    if len(k) != len(v):
        raise ValueError("one key per vertex")
    nv, nf = len(v), len(f)
    lq, mq = (int(factors_q16[0]), int(factors_q16[1])) if factors_q16 is not None else (T.smooth_factor_q16(lam), T.smooth_factor_q16(mu))
    log2 = C.c_uint32()
    check(L.vh_mesh_smooth_default_slots_log2(nf, C.byref(log2)), "vh_mesh_smooth_default_slots_log2")
    el = int(log2.value) if edge_slots_log2 is None else int(edge_slots_log2)
    es = 1 << el
    per_vertex = [4, 4, 48, 24]  # degree, flags, positions, sums: bytes per vertex
    sizes = [8 * es, 4 * es] + [b * max(nv, 1) for b in per_vertex] + [20, 24 * max(nv, 1), 24]
    bufs = [DeviceBuffer.from_numpy(v, stream), DeviceBuffer.from_numpy(k, stream), DeviceBuffer.from_numpy(f if nf else np.zeros((1, 3), np.uint32), stream)]
    bufs += [DeviceBuffer(n) for n in sizes]
    try:
        d_v, d_k, d_f = bufs[:3]
        if guard:
            for i, b in zip(range(5, 9), per_vertex):
                bufs[i].free()
                bufs[i] = DeviceBuffer.from_numpy(np.full(b // 4 * nv + guard, 0xa5a5a5a5, dtype=np.uint32), stream)
        data = T.MeshSmoothData(*[b.ptr for b in bufs[3:]], el, 0)
        check(L.vh_mesh_smooth(d_v.ptr, d_k.ptr, d_f.ptr, nv, nf, int(iterations), lq, mq, 1 if keep_boundary else 0, int(scale_log2), C.byref(data), stream),
              "vh_mesh_smooth")
        counts = bufs[11].download(np.uint32, 6, stream)
        status = int(counts[3])
        n_out = nv if status == 0 else 0
        ov = bufs[10].download(T.VERTEX_DTYPE, n_out, stream)
        out = dict(vertices=np.ascontiguousarray(ov["p"]), colors=np.ascontiguousarray(ov["c"]), keys=k[:n_out].copy(), faces=f.copy() if status == 0 else f[:0].copy())
        if guard:
            out["guards"] = [bufs[i].download(np.uint32, b // 4 * nv + guard, stream)[b // 4 * nv:] for i, b in zip(range(5, 9), per_vertex)]
    finally:
        for b in bufs:
            b.free()
    code = 0 if status == 0 else 2 if status == T.SMOOTH_TABLE_FULL else 4  # VH_ERR_STAGING_OVERFLOW, VH_ERR_BAD_ARGUMENT
    if code and raise_on_status:
        check(code, f"vh_mesh_smooth (status {status})")
    return dict(out, counts={name: int(counts[i]) for i, name in enumerate(T.SMOOTH_COUNTS)}, status=status, code=code)


def mesh_save_ply(filename, vertices, colors=None, normals=None, faces=None, transform=None):
    """vh_mesh_save_ply (host side, no GPU): the mesh container's applyTransform (when a transform is given) and
    saveToPLY on numpy arrays: vertices (V,3), colors (V,4) or None, normals (V,3) or None, faces (F,3) or None"""
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    c = None if colors is None else np.ascontiguousarray(colors, dtype=np.float32).reshape(len(v), 4)
    n = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(len(v), 3)
    f = np.zeros(0, dtype=np.uint32) if faces is None else np.ascontiguousarray(faces, dtype=np.uint32).ravel()
    check(load().vh_mesh_save_ply(v.ctypes.data, None if c is None else c.ctypes.data, None if n is None else n.ctypes.data, len(v),
                                  f.ctypes.data if len(f) else None, len(f), f16(transform) if transform is not None else None,
                                  str(filename).encode()), "vh_mesh_save_ply")


def mesh_weld_appends(parts, slots_log2=0, fixed=False, reserve_triangles=0, raise_on_status=True, stream=None, normals_scale_log2=None,
                      min_component_faces=0, largest_component=False, append_after_components=None, cluster_cells=0, cluster_scale_log2=0,
                      append_after_cluster=None, smooth_iterations=0, smooth_lambda=0.5, smooth_mu=-0.53, keep_boundary=True, smooth_scale_log2=21,
                      append_after_smooth=None):
    """vh_mesh_weld_accum_* on hand-made input: parts is a sequence of (soup, records), appended in order to one
    accumulation -> vertices, colors, keys, faces as mesh_weld(), counts (vertices, faces), stats (the six counts by
    name), status and code.  slots_log2 is the table's FIRST size (0: the smallest), reserve_triangles that of the
    vertex and face arrays; fixed keeps the table from growing.  Errors as mesh_weld().
    normals_scale_log2: run the vertex-normal pass over the finished accumulation -> also normals (V,3) f32 and
    normals_code (what the download returned: 4 when the pass left a status).
    min_component_faces, largest_component: run the component filter over the finished accumulation (after the normals,
    which then ride along) -> also `filtered` (vertices, colors, keys, faces, normals if any) and component_counts (the
    six by name); the unfiltered mesh comes back as without.  append_after_components: one more (soup, records) appended
    after the pass -> stale_code, what the filter's download then returns (4: refused).
    cluster_cells (1 ... 64), cluster_scale_log2: run the vertex clustering over the finished accumulation, BEFORE the
    normals and the components, which are then of the clustered mesh -> also `clustered` (vertices, colors, keys, faces),
    cluster_counts (the six by name) and cluster_code (what the counts' read returned: 4 or 2 when the pass left a
    status).  append_after_cluster: one more (soup, records) appended after the pass -> stale_cluster_code, what the
    counts' read then returns (4: refused); not with the normals or the filter.
    smooth_iterations (1 ... 100), smooth_lambda, smooth_mu, keep_boundary, smooth_scale_log2: run the Taubin smoothing
    over the finished accumulation, AFTER the clustering and before the normals and the components, which then take the
    smoothed vertices -> also `smoothed` (the vertices and colors; keys and faces of the clustered mesh if there is one,
    else the welded one's), smooth_counts (the six by name) and smooth_code.  append_after_smooth: one more (soup,
    records) appended after the pass -> stale_smooth_code, what the counts' read then returns (4: refused)."""
    L = load()
    h = C.c_void_p()
    check(L.vh_mesh_weld_accum_create(slots_log2, reserve_triangles, int(fixed), C.byref(h)), "vh_mesh_weld_accum_create")
    buffers = []
    try:
        check(L.vh_mesh_weld_accum_begin(h, stream), "vh_mesh_weld_accum_begin")
        for triangles, sources in parts:
            d_tris, d_srcs, n = _upload_soup(triangles, sources, stream)
            buffers += [d_tris, d_srcs]
            check(L.vh_mesh_weld_accum_append(h, d_tris.ptr, d_srcs.ptr, n, stream), "vh_mesh_weld_accum_append")
        counts = (C.c_uint32 * 6)()
        code = L.vh_mesh_weld_accum_get_counts(h, counts, stream)
        _check_weld(code, counts[2], raise_on_status, "vh_mesh_weld_accum")
        out = _welded_arrays(counts[0], counts[1], "vh_mesh_weld_accum_download",
                             lambda v, k, f, nv, nf: L.vh_mesh_weld_accum_download(h, v, k, f, nv, nf, stream))
        extra = {}
        mesh_vertices = int(counts[0])  # of the mesh the normals are of
        if cluster_cells and counts[2] == 0:
            check(L.vh_mesh_weld_accum_cluster(h, int(cluster_cells), int(cluster_scale_log2), stream), "vh_mesh_weld_accum_cluster")
            kc = (C.c_uint32 * 6)()
            ccode = L.vh_mesh_weld_accum_cluster_get_counts(h, kc, stream)
            if ccode < 0 or (ccode != 0 and raise_on_status):
                check(ccode, f"vh_mesh_weld_accum_cluster (status {kc[2]})")
            extra.update(cluster_counts={name: int(kc[i]) for i, name in enumerate(T.CLUSTER_COUNTS)}, cluster_code=int(ccode))
            if ccode == 0:
                extra["clustered"] = _welded_arrays(kc[0], kc[1], "vh_mesh_weld_accum_cluster_download",
                                                    lambda v, k, f, nv, nf: L.vh_mesh_weld_accum_cluster_download(h, v, k, f, nv, nf, stream))
                mesh_vertices = int(kc[0])
            if append_after_cluster is not None:
                d_tris, d_srcs, n = _upload_soup(*append_after_cluster, stream)
                buffers += [d_tris, d_srcs]
                check(L.vh_mesh_weld_accum_append(h, d_tris.ptr, d_srcs.ptr, n, stream), "vh_mesh_weld_accum_append")
                extra["stale_cluster_code"] = int(L.vh_mesh_weld_accum_cluster_get_counts(h, kc, stream))
        if smooth_iterations and counts[2] == 0:
            check(L.vh_mesh_weld_accum_smooth(h, int(smooth_iterations), T.smooth_factor_q16(smooth_lambda), T.smooth_factor_q16(smooth_mu), 1 if keep_boundary else 0,
                                              int(smooth_scale_log2), stream), "vh_mesh_weld_accum_smooth")
            sc = (C.c_uint32 * 6)()
            scode = L.vh_mesh_weld_accum_smooth_get_counts(h, sc, stream)
            if scode < 0 or (scode != 0 and raise_on_status):
                check(scode, f"vh_mesh_weld_accum_smooth (status {sc[3]})")
            extra.update(smooth_counts={name: int(sc[i]) for i, name in enumerate(T.SMOOTH_COUNTS)}, smooth_code=int(scode))
            if scode == 0:
                base = extra.get("clustered", out)
                sv = np.zeros(mesh_vertices, dtype=T.VERTEX_DTYPE)
                check(L.vh_mesh_weld_accum_smooth_download(h, sv.ctypes.data, mesh_vertices, stream), "vh_mesh_weld_accum_smooth_download")
                extra["smoothed"] = dict(vertices=np.ascontiguousarray(sv["p"]), colors=np.ascontiguousarray(sv["c"]), keys=base["keys"], faces=base["faces"])
            if append_after_smooth is not None:
                d_tris, d_srcs, n = _upload_soup(*append_after_smooth, stream)
                buffers += [d_tris, d_srcs]
                check(L.vh_mesh_weld_accum_append(h, d_tris.ptr, d_srcs.ptr, n, stream), "vh_mesh_weld_accum_append")
                extra["stale_smooth_code"] = int(L.vh_mesh_weld_accum_smooth_get_counts(h, sc, stream))
        if normals_scale_log2 is not None and counts[2] == 0:
            check(L.vh_mesh_weld_accum_normals(h, int(normals_scale_log2), stream), "vh_mesh_weld_accum_normals")
            nrm = np.zeros((mesh_vertices, 3), dtype=np.float32)
            ncode = L.vh_mesh_weld_accum_download_normals(h, nrm.ctypes.data, len(nrm), stream)
            if ncode < 0 or (ncode != 0 and raise_on_status):
                check(ncode, "vh_mesh_weld_accum_download_normals")
            extra.update(normals=nrm, normals_code=int(ncode))
        if (min_component_faces or largest_component) and counts[2] == 0:
            check(L.vh_mesh_weld_accum_components(h, int(min_component_faces), 1 if largest_component else 0, stream), "vh_mesh_weld_accum_components")
            cc = (C.c_uint32 * 6)()
            check(L.vh_mesh_weld_accum_components_get_counts(h, cc, stream), "vh_mesh_weld_accum_components_get_counts")
            with_n = "normals" in extra and extra["normals_code"] == 0
            fn = np.zeros((int(cc[3]), 3), dtype=np.float32)
            filtered = _welded_arrays(cc[3], cc[4], "vh_mesh_weld_accum_components_download",
                                      lambda v, k, f, nv, nf: L.vh_mesh_weld_accum_components_download(h, v, k, fn.ctypes.data if with_n else None, f, nv, nf, stream))
            if with_n:
                filtered["normals"] = fn
            extra.update(filtered=filtered, component_counts={name: int(cc[i]) for i, name in enumerate(T.COMPONENTS_COUNTS)})
            if append_after_components is not None:
                d_tris, d_srcs, n = _upload_soup(*append_after_components, stream)
                buffers += [d_tris, d_srcs]
                check(L.vh_mesh_weld_accum_append(h, d_tris.ptr, d_srcs.ptr, n, stream), "vh_mesh_weld_accum_append")
                extra["stale_code"] = int(L.vh_mesh_weld_accum_components_download(h, None, None, None, None, 0, 0, stream))
    finally:
        L.vh_mesh_weld_accum_destroy(h)
        for b in buffers:
            b.free()
    return dict(out, counts=(int(counts[0]), int(counts[1])), stats={n: int(counts[i]) for i, n in enumerate(T.WELD_ACCUM_COUNTS)},
                status=int(counts[2]), code=int(code), **extra)


# ---- sensor pre-processing (DSC/CameraUtil.cu) over the C ABI: numpy in, numpy out (tests, tools) ----

def image_op(name, src, width, height, *args, out_channels=1, out_size=None, prefill=None):
    """run vh_<name> on one source image; -> float32 array (height, width[, 4]) of the output size"""
    L = load()
    src = np.ascontiguousarray(src)
    d_in = DeviceBuffer.from_numpy(src)
    ow, oh = out_size if out_size else (width, height)
    n_out = ow * oh * out_channels
    d_out = DeviceBuffer(n_out * 4)
    if prefill is not None:
        d_out.upload(np.ascontiguousarray(prefill, dtype=np.float32))
    fn = getattr(L, "vh_" + name)
    if name in ("resample_float_map", "resample_float4_map"):
        check(fn(d_out.ptr, ow, oh, d_in.ptr, width, height, None), name)
    elif name == "convert_depth_float_to_camera_space_float4":
        check(fn(d_out.ptr, d_in.ptr, C.byref(args[0]), width, height, None), name)
    elif name == "erode_depth_map":
        check(fn(d_out.ptr, d_in.ptr, int(args[0]), width, height, float(args[1]), float(args[2]), None), name)
    elif name in ("gauss_filter_float_map", "gauss_filter_float4_map", "bilateral_filter_float_map"):
        check(fn(d_out.ptr, d_in.ptr, float(args[0]), float(args[1]), width, height, None), name)
    elif name == "set_invalid_float_map":
        check(fn(d_out.ptr, width, height, None), name)
    else:
        check(fn(d_out.ptr, d_in.ptr, width, height, None), name)
    out = d_out.download(np.float32, n_out)
    return out.reshape((oh, ow, out_channels)) if out_channels > 1 else out.reshape((oh, ow))


def ingest_frame(depth_u16, color_u8, adapter_size, depth_shift=1000.0, stream=None):
    """vh_ingest_frame on host arrays: depth [h, w] u16, colour [h', w', 3 or 4] u8 or None, adapter_size (width, height)
    -> (depth [H, W] f32, colour [H, W, 4] f32 or None) as the device made them"""
    W, H = int(adapter_size[0]), int(adapter_size[1])
    d = np.ascontiguousarray(depth_u16, dtype=np.uint16)
    d_in = DeviceBuffer.from_numpy(d, stream)
    d_out = DeviceBuffer(4 * W * H)
    c_in = c_out = None
    cw = ch = channels = 0
    if color_u8 is not None:
        c = np.ascontiguousarray(color_u8, dtype=np.uint8)
        ch, cw, channels = c.shape
        c_in = DeviceBuffer.from_numpy(c, stream)
        c_out = DeviceBuffer(16 * W * H)
    check(load().vh_ingest_frame(d_out.ptr, c_out.ptr if c_out else None, W, H, d_in.ptr, d.shape[1], d.shape[0], c_in.ptr if c_in else None, cw, ch,
                                 channels, depth_shift, stream), "vh_ingest_frame")
    depth = d_out.download(np.float32, W * H, stream).reshape(H, W)
    color = c_out.download(np.float32, 4 * W * H, stream).reshape(H, W, 4) if c_out else None
    return depth, color


class CUDARGBDSensor:
    """Mirror of CUDARGBDSensor over CUDARGBDAdapter (include/vh.hpp) over the C ABI."""

    def __init__(self, depth_size, color_size, adapter_size, fx, fy, mx, my, depth_min, depth_max, stream=None):
        self.L = load()
        self.size = tuple(adapter_size)
        sizes = (C.c_uint32 * 6)(depth_size[0], depth_size[1], color_size[0], color_size[1], adapter_size[0], adapter_size[1])
        intr = (C.c_float * 6)(fx, fy, mx, my, depth_min, depth_max)
        h = C.c_void_p()
        check(self.L.vh_rgbd_sensor_create(sizes, intr, stream, C.byref(h)), "vh_rgbd_sensor_create")
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self.L.vh_rgbd_sensor_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def setFiterDepthValues(self, b=True, sigmaD=1.0, sigmaR=1.0):
        check(self.L.vh_rgbd_sensor_set_filter_depth_values(self.handle, int(b), sigmaD, sigmaR), "setFiterDepthValues")

    def setFiterIntensityValues(self, b=True, sigmaD=1.0, sigmaR=1.0):
        check(self.L.vh_rgbd_sensor_set_filter_intensity_values(self.handle, int(b), sigmaD, sigmaR), "setFiterIntensityValues")

    def setCameraCalibration(self, enabled, colorFx, colorFy, colorMx, colorMy, depthExtrinsics, thresOffset, thresLin):
        """s_bUseCameraCalibration: remap the depth map into the colour camera (colour intrinsics at the colour sensor's
        resolution, the depth extrinsic as the modelview); an identity extrinsic leaves it off"""
        ci = (C.c_float * 4)(colorFx, colorFy, colorMx, colorMy)
        check(self.L.vh_rgbd_sensor_set_camera_calibration(self.handle, int(bool(enabled)), ci, f16(depthExtrinsics), thresOffset, thresLin),
              "setCameraCalibration")

    def getCameraCalibration(self):
        """-> (whether the remap took effect, the ViewParams process() draws with)"""
        on, p = C.c_int(), T.ViewParams()
        check(self.L.vh_rgbd_sensor_get_camera_calibration(self.handle, C.byref(on), C.byref(p)), "getCameraCalibration")
        return bool(on.value), p

    def process(self, depth_float, color_rgbx):
        d = np.ascontiguousarray(depth_float, dtype=np.float32)
        c = np.ascontiguousarray(color_rgbx, dtype=np.uint8)
        check(self.L.vh_rgbd_sensor_process(self.handle, d.ctypes.data, c.ctypes.data), "process")

    def getDepthCameraData(self):
        out = T.DepthCameraData()
        check(self.L.vh_rgbd_sensor_get_depth_camera_data(self.handle, C.byref(out)), "getDepthCameraData")
        return out

    def getDepthCameraParams(self):
        out = T.DepthCameraParams()
        check(self.L.vh_rgbd_sensor_get_depth_camera_params(self.handle, C.byref(out)), "getDepthCameraParams")
        return out

    def download(self):
        W, H = self.size
        cam = self.getDepthCameraData()
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(self.L.vh_rgbd_sensor_get_maps(self.handle, C.byref(a), C.byref(b), C.byref(c)), "get_maps")
        return dict(
            depth=download(cam.d_depthData, np.float32, W * H).reshape(H, W),
            color=download(cam.d_colorData, np.float32, W * H * 4).reshape(H, W, 4),
            camera_space=download(a.value, np.float32, W * H * 4).reshape(H, W, 4),
            normals=download(b.value, np.float32, W * H * 4).reshape(H, W, 4),
            intensity=download(c.value, np.float32, W * H).reshape(H, W),
        )


def view_resolve_depth(d_depth, params, d_keys, d_large_list, d_out_depth, stream=None):
    """vh_view_resolve_depth: render target 0 of the keys vh_view_raster left (device pointers; params a ViewParams)"""
    check(load().vh_view_resolve_depth(d_depth, C.byref(params), d_keys, d_large_list, d_out_depth, stream), "vh_view_resolve_depth")


class CUDACameraTrackingMultiRes:
    """Mirror of DSC/CUDACameraTrackingMultiRes.h:17-78 over the C ABI (device pointers in, 4x4 pose out)."""

    def __init__(self, imageWidth, imageHeight, levels, stream=None):
        self.L = load()
        h = C.c_void_p()
        check(self.L.vh_camera_tracking_create(imageWidth, imageHeight, levels, stream, C.byref(h)), "vh_camera_tracking_create")
        self.handle = h
        self.state = T.IcpState()

    def close(self):
        if getattr(self, "handle", None):
            self.L.vh_camera_tracking_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def applyCT(self, d_input, d_inputNormals, d_model, d_modelNormals, lastTransform, settings, deltaTransformEstimate, cameraParams):
        """-> (4x4 float32 pose = lastTransform * delta, lost flag); the final VhIcpState is kept in self.state"""
        out = (C.c_float * 16)()
        lost = C.c_int(0)
        est = f16(deltaTransformEstimate) if deltaTransformEstimate is not None else None
        check(self.L.vh_camera_tracking_apply_ct(self.handle, d_input, d_inputNormals, d_model, d_modelNormals, f16(lastTransform), C.byref(settings),
                                                 est, C.byref(cameraParams), out, C.byref(lost), C.byref(self.state)), "applyCT")
        return np.array(out, dtype=np.float32).reshape(4, 4), bool(lost.value)


class CUDACameraTrackingMultiResRGBD:
    """Mirror of DSC/CUDACameraTrackingMultiResRGBD.h:23-75 over the C ABI (device pointers in, 4x4 pose out)."""

    def __init__(self, imageWidth, imageHeight, levels, stream=None):
        self.L = load()
        h = C.c_void_p()
        check(self.L.vh_camera_tracking_rgbd_create(imageWidth, imageHeight, levels, stream, C.byref(h)), "vh_camera_tracking_rgbd_create")
        self.handle = h
        self.state = T.IcpStateRGBD()

    def close(self):
        if getattr(self, "handle", None):
            self.L.vh_camera_tracking_rgbd_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def applyCT(self, d_input, d_inputNormals, d_inputColor, d_model, d_modelNormals, d_modelColor, lastTransform, settings, deltaTransformEstimate,
                cameraParams):
        """-> (4x4 float32 pose = lastTransform * delta, lost flag); the final VhIcpStateRGBD is kept in self.state.
        d_inputColor: the sensor's float4 colour map; d_model*: the ray cast's d_depth4, d_normals, d_colors."""
        out = (C.c_float * 16)()
        lost = C.c_int(0)
        est = f16(deltaTransformEstimate) if deltaTransformEstimate is not None else None
        check(self.L.vh_camera_tracking_rgbd_apply_ct(self.handle, d_input, d_inputNormals, d_inputColor, d_model, d_modelNormals, d_modelColor,
                                                      f16(lastTransform), C.byref(settings), est, C.byref(cameraParams), out, C.byref(lost),
                                                      C.byref(self.state)), "applyCT")
        return np.array(out, dtype=np.float32).reshape(4, 4), bool(lost.value)


class RGBDRenderer:
    """Mirror of DX11RGBDRenderer (DSC/DX11RGBDRenderer.h) over the C ABI: RenderDepthMap draws a depth map as a mesh into
    four screen-size device maps (depth f32, position / normal / colour float4)."""

    def __init__(self, stream=None):
        self.L = load()
        self.stream = stream
        h = C.c_void_p()
        check(self.L.vh_rgbd_renderer_create(stream, C.byref(h)), "vh_rgbd_renderer_create")
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self.L.vh_rgbd_renderer_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def RenderDepthMap(self, d_depthMap, d_colorMap, width, height, intrinsicDepthToWorld, modelview, intrinsicWorldToDepth, screenWidth, screenHeight,
                       depthThreshOffset, depthThreshLin):
        check(self.L.vh_rgbd_renderer_render_depth_map(self.handle, d_depthMap, d_colorMap, width, height, f16(intrinsicDepthToWorld), f16(modelview),
                                                       f16(intrinsicWorldToDepth), screenWidth, screenHeight, depthThreshOffset, depthThreshLin),
              "RenderDepthMap")

    def getMaps(self):
        """-> dict of device pointers (depth, positions, normals, colors) and the screen size (width, height)"""
        ptrs = [C.c_void_p() for _ in range(4)]
        size = (C.c_uint32 * 2)()
        check(self.L.vh_rgbd_renderer_get_maps(self.handle, *[C.byref(p) for p in ptrs], size), "getMaps")
        return dict(depth=ptrs[0].value, positions=ptrs[1].value, normals=ptrs[2].value, colors=ptrs[3].value, size=(size[0], size[1]))

    def download(self):
        m = self.getMaps()
        W, H = m["size"]
        s = self.stream
        return dict(depth=download(m["depth"], np.float32, H * W, s).reshape(H, W),
                    positions=download(m["positions"], np.float32, H * W * 4, s).reshape(H, W, 4),
                    normals=download(m["normals"], np.float32, H * W * 4, s).reshape(H, W, 4),
                    colors=download(m["colors"], np.float32, H * W * 4, s).reshape(H, W, 4))


class PhongLighting:
    """Mirror of DX11PhongLighting (DSC/DX11PhongLighting.h): PhongPS over three float4 device maps; the light is a
    PhongLight (phong_light_from_render_state)."""

    def __init__(self, light, stream=None):
        self.L = load()
        self.stream = stream
        self.light = _copy_struct(light)
        h = C.c_void_p()
        check(self.L.vh_phong_lighting_create(C.byref(self.light), stream, C.byref(h)), "vh_phong_lighting_create")
        self.handle = h
        self.size = (0, 0)

    def close(self):
        if getattr(self, "handle", None):
            self.L.vh_phong_lighting_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def render(self, d_positions, d_normals, d_colors, useMaterial, width, height, rgba8=False):
        check(self.L.vh_phong_lighting_render(self.handle, d_positions, d_normals, d_colors, 1 if useMaterial else 0, width, height, 1 if rgba8 else 0),
              "PhongLighting::render")
        self.size = (width, height)

    def getColors(self):
        """-> (float4 target, RGBA8 target) device pointers"""
        a, b = C.c_void_p(), C.c_void_p()
        check(self.L.vh_phong_lighting_get_colors(self.handle, C.byref(a), C.byref(b)), "getColors")
        return a.value, b.value

    def download(self, rgba8=False):
        W, H = self.size
        a, b = self.getColors()
        if rgba8:
            return download(b, np.uint8, H * W * 4, self.stream).reshape(H, W, 4)
        return download(a, np.float32, H * W * 4, self.stream).reshape(H, W, 4)


def phong_light_from_render_state(render_state):
    light = T.PhongLight()
    load().vh_phong_light_from_render_state(C.byref(render_state), C.byref(light))
    return light


def write_png_rgba8(filename, rgba, level=-1):
    """an [H, W, 4] uint8 array -> 8-bit RGBA PNG (vh_write_png_rgba8)"""
    a = np.ascontiguousarray(rgba, dtype=np.uint8)
    H, W = a.shape[:2]
    check(load().vh_write_png_rgba8(str(filename).encode(), W, H, a.ctypes.data, level), f"vh_write_png_rgba8 {filename}")
