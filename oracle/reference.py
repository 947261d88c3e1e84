"""ctypes wrapper of oracle/_ref/libvh_ref.so: the reference's own voxel-hashing code, compiled for the CPU.

TEST INFRASTRUCTURE ONLY, like oracle.py.  `__graft_entry__.build()` makes the library (oracle/ref/Makefile) when the
reference tree is present; nothing here reads that tree.  Every function takes the same structs as its vho_* twin in
oracle/vh_oracle.c, so a test runs both on two copies of one state (`RefScene` shares an OracleScene's buffers).
"""
import ctypes as C
import os

import numpy as np

from voxelhashing_amd import vhtypes as T

_HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(_HERE, "_ref", "libvh_ref.so")
_LIB = []


def available():
    return os.path.exists(PATH)


def lib():
    if _LIB:
        return _LIB[0]
    L = C.CDLL(PATH)
    P, f, i32, u32, vp = C.POINTER, C.c_float, C.c_int32, C.c_uint32, C.c_void_p
    HD, HP, CP, RP = P(T.HashData), P(T.HashParams), P(T.DepthCameraParams), P(T.RayCastParams)
    sig = {
        "vhr_compute_hash_pos": ([HP, P(i32)], u32),
        "vhr_world_to_virtual_voxel_pos": ([HP, P(f), P(i32)], None),
        "vhr_virtual_voxel_pos_to_sdf_block": ([P(i32), P(i32)], None),
        "vhr_world_to_sdf_block": ([HP, P(f), P(i32)], None),
        "vhr_sdf_block_to_world": ([HP, P(i32), P(f)], None),
        "vhr_virtual_voxel_pos_to_world": ([HP, P(i32), P(f)], None),
        "vhr_virtual_voxel_pos_to_local_index": ([P(i32)], C.c_int),
        "vhr_linearize_voxel_pos": ([P(i32)], u32),
        "vhr_delinearize_voxel_index": ([u32, P(i32)], None),
        "vhr_is_block_in_frustum": ([HP, CP, P(i32)], C.c_int),
        "vhr_get_truncation": ([HP, f], f),
        "vhr_combine_voxel": ([HP, T.Voxel, T.Voxel], T.Voxel),
        "vhr_camera_to_screen_float": ([CP, P(f), P(f)], None),
        "vhr_camera_to_screen_int": ([CP, P(f), P(i32)], None),
        "vhr_camera_to_proj": ([CP, P(f), P(f)], None),
        "vhr_camera_to_proj_z": ([CP, f], f),
        "vhr_depth_to_skeleton": ([CP, u32, u32, f, P(f)], None),
        "vhr_proj_to_camera_z": ([CP, f], f),
        "vhr_get_hash_entry": ([HD, HP, P(i32)], T.HashEntry),
        "vhr_alloc_block": ([HD, HP, P(i32)], None),
        "vhr_delete_hash_entry_element": ([HD, HP, P(i32)], C.c_int),
        "vhr_insert_hash_entry_bucket": ([HD, HP, P(T.HashEntry)], C.c_int),
        "vhr_reset": ([HD, HP], None),
        "vhr_reset_bucket_mutex": ([HD, HP], None),
        "vhr_mat4_inverse": ([P(f), P(f)], None),
        "vhr_alloc": ([HD, HP, P(T.DepthCameraData), CP, vp, C.c_int], None),
        "vhr_integrate": ([HD, HP, P(T.DepthCameraData), CP], None),
        "vhr_starve": ([HD, HP], None),
        "vhr_gc_free": ([HD, HP], None),
        "vhr_render": ([HD, HP, P(T.RayCastData), CP, RP], None),
        "vhr_compute_normals": ([vp, vp, u32, u32], None),
        "vhr_trilinear": ([HD, HP, P(f), P(f), P(C.c_uint8)], C.c_int),
        "vhr_intersect_bisection": ([HD, HP, P(f), P(f), f, f, f, f, P(f), P(C.c_uint8)], C.c_int),
        "vhr_gradient_for_point": ([HD, HP, P(f), P(f)], None),
        "vhr_compactify": ([HD, HP, CP], u32),
        "vhr_gc_identify": ([HD, HP, CP], None),
        "vhr_stream_out_pass1": ([HD, HP, u32, u32, f, P(f), vp, u32], u32),
        "vhr_stream_out_pass2": ([HD, HP, vp, vp, u32], None),
        "vhr_stream_in_pass1": ([HD, HP, u32, u32, vp], None),
        "vhr_stream_in_pass2": ([HD, HP, u32, u32, vp, vp], None),
        "vhr_extract_iso_surface": ([HD, HP, P(T.MarchingCubesParams), vp, u32, C.c_int], u32),
        "vhr_convert_color_raw_to_float4": ([vp, vp, u32, u32], None),
        "vhr_resample_float_map": ([vp, u32, u32, vp, u32, u32], None),
        "vhr_resample_float4_map": ([vp, u32, u32, vp, u32, u32], None),
        "vhr_convert_color_to_intensity_float": ([vp, vp, u32, u32], None),
        "vhr_convert_depth_float_to_camera_space_float4": ([vp, vp, CP, u32, u32], None),
        "vhr_gauss_filter_float_map": ([vp, vp, f, f, u32, u32], None),
        "vhr_gauss_filter_float4_map": ([vp, vp, f, f, u32, u32], None),
        "vhr_bilateral_filter_float_map": ([vp, vp, f, f, u32, u32], None),
        "vhr_erode_depth_map": ([vp, vp, C.c_int, u32, u32, f, f], None),
        "vhr_compute_intensity_and_derivatives": ([vp, vp, u32, u32], None),
        "vhr_icp_correspondences": ([vp, vp, vp, vp, vp, vp, u32, u32, f, f, f, P(f), CP], None),
        "vhr_icp_lane_sums": ([u32, u32, vp, vp, vp, vp, P(f), u32], None),
        "vhr_icp_rgbd_lane_sums": ([u32, u32, vp, vp, vp, vp, vp, vp, vp, P(f), P(f), P(f), P(f), u32], None),
        "vhr_icp_solve": ([P(f), P(f), P(f), P(C.c_int)], C.c_int),
        "vhr_rotation_angle": ([P(f)], f),
    }
    for name, (args, res) in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    _LIB.append(L)
    return L


def compute_normals(depth4):
    H, W, _ = depth4.shape
    d4 = np.ascontiguousarray(depth4, dtype=np.float32)
    out = np.empty_like(d4)
    lib().vhr_compute_normals(out.ctypes.data, d4.ctypes.data, W, H)
    return out


def image_op(name, src, width, height, *args, out_channels=1, out_size=None, prefill=None):
    """the reference's CameraUtil.cu map `name`, with oracle.image_op's signature (vhr_<name> here, vho_<name> there)"""
    from oracle import oracle as O
    return O.call_image_op(lib(), "vhr_", name, src, width, height, *args, out_channels=out_channels,
                           out_size=out_size, prefill=prefill)


def compute_intensity_and_derivatives(intensity):
    """computeIntensityAndDerivatives: (H, W) intensity -> (H, W, 4) intensity, d/du, d/dv, 1"""
    H, W = intensity.shape
    src = np.ascontiguousarray(intensity, dtype=np.float32)
    out = np.empty((H, W, 4), dtype=np.float32)
    lib().vhr_compute_intensity_and_derivatives(out.ctypes.data, src.ctypes.data, W, H)
    return out


# ---- the camera trackers (oracle/ref/vh_ref_track.cpp): the same arrays as their twins in oracle/icp.py and
# tests/rgbd_icp.py.  A 4x4 transform is row-major everywhere in this project, and so it is here.

def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _map(a, channels):
    a = np.ascontiguousarray(a, dtype=np.float32)
    assert a.shape[-1] == channels if channels > 1 else a.ndim == 2, a.shape
    return a


def icp_correspondences(inp, inp_n, tgt, tgt_n, delta, dist_thres, normal_thres, level_factor, cp):
    """projectiveCorrespondences -> (positions, normals with the pair weight in .w), as oracle.icp.correspondences.  The
    launcher takes a float4x4, which is row-major: delta goes in as it is."""
    inp, inp_n, tgt, tgt_n = (_map(a, 4) for a in (inp, inp_n, tgt, tgt_n))
    h, w = inp.shape[:2]
    corr, corr_n = np.empty_like(inp), np.empty_like(inp)
    m = np.ascontiguousarray(delta, dtype=np.float32).reshape(16)
    lib().vhr_icp_correspondences(inp.ctypes.data, inp_n.ctypes.data, tgt.ctypes.data, tgt_n.ctypes.data, corr.ctypes.data,
                                  corr_n.ctypes.data, w, h, dist_thres, normal_thres, level_factor, _fp(m), C.byref(cp))
    return corr, corr_n


def _lanes(n, window):
    return -(-n // window)


def icp_lane_sums(inp, corr, corr_n, delta, window=1):
    """buildLinearSystem with one thread per block -> (ceil(H W / window), 30) float32: row b is the in-order sum of the
    30 terms over pixels [b window, (b + 1) window), as a lane of the reference's kernel sums them; with window 1, one
    pixel's terms, as oracle.icp.pixel_terms.

    THE TRANSFORM'S STORAGE ORDER is settled here and nowhere else: the reference's host code hands the launcher
    Eigen::Matrix4f::data(), which is column-major, and the kernel reads those 16 floats as a row-major float4x4 and
    multiplies by its transpose.  `delta` is row-major like every transform of this project, so it is transposed here
    into what data() would hold."""
    inp, corr, corr_n = (_map(a, 4) for a in (inp, corr, corr_n))
    h, w = inp.shape[:2]
    out = np.empty((_lanes(w * h, window), 30), dtype=np.float32)
    col_major = np.ascontiguousarray(np.asarray(delta, dtype=np.float32).reshape(4, 4).T).reshape(16)
    lib().vhr_icp_lane_sums(w, h, out.ctypes.data, inp.ctypes.data, corr.ctypes.data, corr_n.ctypes.data, _fp(col_major), window)
    return out


def icp_rgbd_lane_sums(inp, inp_n, inp_i, tgt, tgt_n, tgt_iad, angles, trans, prm, window=1):
    """computeNormalEquations with one thread per block -> (ceil(H W / window), 30) float32 lane sums (depth row, then
    colour row per pixel), arguments as tests/rgbd_icp.pixel_terms.  The intrinsics go in as the row-major 3x3 the
    host code makes by transposing its Eigen matrix."""
    inp, inp_n, tgt, tgt_n, tgt_iad = (_map(a, 4) for a in (inp, inp_n, tgt, tgt_n, tgt_iad))
    inp_i = _map(inp_i, 1)
    h, w = inp.shape[:2]
    out = np.empty((_lanes(w * h, window), 30), dtype=np.float32)
    k = np.array([prm["fx"], 0, prm["mx"], 0, prm["fy"], prm["my"], 0, 0, 1], dtype=np.float32)
    p = np.array([prm[n] for n in ("weightDepth", "weightColor", "distThres", "normalThres", "sensorMaxDepth",
                                   "colorGradientMin", "colorThres")], dtype=np.float32)
    a, t = np.ascontiguousarray(angles, dtype=np.float32), np.ascontiguousarray(trans, dtype=np.float32)
    lib().vhr_icp_rgbd_lane_sums(w, h, out.ctypes.data, inp.ctypes.data, inp_n.ctypes.data, inp_i.ctypes.data, tgt.ctypes.data,
                                 tgt_n.ctypes.data, tgt_iad.ctypes.data, _fp(k), _fp(p), _fp(a), _fp(t), window)
    return out


def icp_solve(terms):
    """the reference's solve step in its own float32 Eigen on a row of 30 summed terms -> (x (6,) float32, condition
    s_0 / s_5 (float32), rank, ATA.isZero())"""
    t = np.ascontiguousarray(terms, dtype=np.float32).reshape(30)
    x = np.empty(6, dtype=np.float32)
    cond, zero = C.c_float(), C.c_int()
    rank = lib().vhr_icp_solve(_fp(t), _fp(x), C.byref(cond), C.byref(zero))
    return x, np.float32(cond.value), int(rank), bool(zero.value)


def rotation_angle(R):
    """Eigen::AngleAxisf(R).angle() of a 3x3 rotation"""
    m = np.ascontiguousarray(R, dtype=np.float32).reshape(9)
    return np.float32(lib().vhr_rotation_angle(_fp(m)))


def mat4_inverse(m):
    m = np.ascontiguousarray(m, dtype=np.float32).reshape(16)
    out = np.empty(16, dtype=np.float32)
    lib().vhr_mat4_inverse(m.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


class RefScene:
    """The reference's kernels on the buffers and parameters of an oracle.OracleScene (which owns them)."""

    def __init__(self, scene):
        self.s = scene
        self.L = lib()

    # -- a scene run by the reference's code alone: reset, transform, mutex, offline alloc, compactify ----------
    def reset(self):
        self.s.hp.m_numOccupiedBlocks = 0
        self.L.vhr_reset(C.byref(self.s.hd), C.byref(self.s.hp))

    def set_transform(self, transform):
        m = np.ascontiguousarray(transform, dtype=np.float32).reshape(16)
        self.s.hp.m_rigidTransform = (C.c_float * 16)(*m.tolist())
        self.s.hp.m_rigidTransformInverse = (C.c_float * 16)(*mat4_inverse(m).tolist())

    def reset_mutex(self):
        self.L.vhr_reset_bucket_mutex(C.byref(self.s.hd), C.byref(self.s.hp))

    def alloc_offline(self, depth, color, raster=False):
        """CUDASceneRepHashSDF::alloc with offline processing: passes until the heap stops moving"""
        prev = None
        while prev != self.s.heap_free_count():
            prev = self.s.heap_free_count()
            self.reset_mutex()
            self.alloc(depth, color, raster=raster)

    def compactify(self):
        """compactifyHashAllInOneCUDA: the live entries whose block passes the frustum test, in table order (serial
        workgroups); the count is also left in m_numOccupiedBlocks"""
        s = self.s
        n = int(self.L.vhr_compactify(C.byref(s.hd), C.byref(s.hp), C.byref(s.cp)))
        # the kernel's set is the frustum rule applied to the live entries
        table = s.hash_table()
        live = np.nonzero(table["ptr"] != T.FREE_ENTRY)[0]
        keep = [i for i in live if self.L.vhr_is_block_in_frustum(
            C.byref(s.hp), C.byref(s.cp), np.ascontiguousarray(table["pos"][i]).ctypes.data_as(C.POINTER(C.c_int32)))]
        assert n == len(keep) and int(s.array("d_hashCompactifiedCounter", np.int32, 1)[0]) == n
        assert np.array_equal(s.array("d_hashCompactified", T.HASH_ENTRY_DTYPE, n), table[keep])
        return n

    def integrate(self, transform, depth, color, bitmask=None):
        """CUDASceneRepHashSDF::integrate with the reference's kernels, on the OracleScene's options and frame counter:
        alloc (in raster order, the oracle's thread order; offline: passes until the heap stops moving), compactify,
        integrate, and with GC on: starve every opt.s_garbageCollectionStarve frames, GC identify, GC free.  Returns
        the number of blocks GC freed."""
        s = self.s
        freed = 0
        self.set_transform(transform)
        if s.opt.s_offlineProcessing:
            prev = None
            while prev != s.heap_free_count():
                prev = s.heap_free_count()
                self.reset_mutex()
                self.alloc(depth, color, bitmask, raster=True)
        else:
            self.reset_mutex()
            self.alloc(depth, color, bitmask, raster=True)
        self.compactify()
        self.integrate_depth_map(depth, color)
        if s.opt.s_garbageCollectionEnabled:
            k, starve = s.frames.value, s.opt.s_garbageCollectionStarve
            if k > 0 and starve != 0 and k % starve == 0:
                self.starve()
            self.gc_identify()
            self.reset_mutex()
            live = int((s.hash_table()["ptr"] != T.FREE_ENTRY).sum())
            self.gc_free()
            freed = live - int((s.hash_table()["ptr"] != T.FREE_ENTRY).sum())
        s.frames.value += 1
        return freed

    def gc_identify(self):
        self.L.vhr_gc_identify(C.byref(self.s.hd), C.byref(self.s.hp), C.byref(self.s.cp))

    def stream_out_pass1(self, threads_per_part, start, radius, cam_pos, capacity=100000):
        out = np.zeros(capacity, dtype=T.DESC_DTYPE)
        cpv = np.ascontiguousarray(cam_pos, dtype=np.float32)
        n = self.L.vhr_stream_out_pass1(C.byref(self.s.hd), C.byref(self.s.hp), threads_per_part, start,
                                        C.c_float(radius), cpv.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data,
                                        capacity)
        return out[:n].copy()

    def stream_out_pass2(self, descs):
        descs = np.ascontiguousarray(descs, dtype=T.DESC_DTYPE)
        out = np.zeros((len(descs), T.SDF_BLOCK_VOXELS), dtype=T.VOXEL_DTYPE)
        self.L.vhr_stream_out_pass2(C.byref(self.s.hd), C.byref(self.s.hp), descs.ctypes.data, out.ctypes.data,
                                    len(descs))
        return out

    def stream_in(self, descs, blocks):
        """chunkToGlobalHashPass1CUDA + Pass2CUDA, then the heap counter moved down by len(descs) as
        CUDASceneRepChunkGrid::streamInToGPUChunk does.  Only for entries whose bucket has room: the reference's
        insertHashEntry corrupts the table in its list branch.  Returns 0 (the reference's pass
        reports no failed insert)."""
        s = self.s
        descs = np.ascontiguousarray(descs, dtype=T.DESC_DTYPE)
        blocks = np.ascontiguousarray(blocks, dtype=T.VOXEL_DTYPE)
        n = len(descs)
        table = s.hash_table()
        for d in descs:
            b = int(self.L.vhr_compute_hash_pos(C.byref(s.hp), np.ascontiguousarray(d["pos"], dtype=np.int32)
                                                .ctypes.data_as(C.POINTER(C.c_int32))))
            bucket = table[b * T.HASH_BUCKET_SIZE:(b + 1) * T.HASH_BUCKET_SIZE]
            assert (bucket["ptr"] == T.FREE_ENTRY).any(), f"stream in: bucket {b} is full (the reference's list branch)"
        hc = s.array("d_heapCounter", np.uint32, 1)
        prev = int(hc[0])
        self.L.vhr_stream_in_pass1(C.byref(s.hd), C.byref(s.hp), n, prev, descs.ctypes.data)
        self.L.vhr_stream_in_pass2(C.byref(s.hd), C.byref(s.hp), n, prev, descs.ctypes.data, blocks.ctypes.data)
        hc[0] = prev - n
        return 0

    def extract_iso_surface(self, mc_params, max_triangles=None, two_pass=True):
        """resetMarchingCubesCUDA + extractIsoSurfacePass1/2CUDA (two_pass) or extractIsoSurfaceCUDA -> triangles
        (T.TRIANGLE_DTYPE) and the reference's counter (clamped to the capacity)"""
        cap = int(max_triangles if max_triangles is not None else mc_params.m_maxNumTriangles)
        out = np.zeros(max(cap, 1), dtype=T.TRIANGLE_DTYPE)
        n = int(self.L.vhr_extract_iso_surface(C.byref(self.s.hd), C.byref(self.s.hp), C.byref(mc_params),
                                               out.ctypes.data, cap, int(two_pass)))
        return out[:min(n, cap)].copy(), n

    def alloc(self, depth, color=None, bitmask=None, raster=True):
        cam = self.s._cam(depth, color)
        bm = None if bitmask is None else bitmask.ctypes.data
        self.L.vhr_alloc(C.byref(self.s.hd), C.byref(self.s.hp), C.byref(cam), C.byref(self.s.cp), bm, int(raster))

    def integrate_depth_map(self, depth, color):
        cam = self.s._cam(depth, color)
        self.L.vhr_integrate(C.byref(self.s.hd), C.byref(self.s.hp), C.byref(cam), C.byref(self.s.cp))

    def starve(self):
        self.L.vhr_starve(C.byref(self.s.hd), C.byref(self.s.hp))

    def gc_free(self):
        self.L.vhr_gc_free(C.byref(self.s.hd), C.byref(self.s.hp))

    def render(self, ray_params):
        s = self.s
        self.L.vhr_render(C.byref(s.hd), C.byref(s.hp), C.byref(s.rd), C.byref(s.cp), C.byref(ray_params))
        return dict(depth=s.rc_depth.copy(), depth4=s.rc_depth4.copy(), normals=s.rc_normals.copy(),
                    colors=s.rc_colors.copy())

    def alloc_block(self, pos):
        p = np.asarray(pos, dtype=np.int32)
        self.L.vhr_alloc_block(C.byref(self.s.hd), C.byref(self.s.hp), p.ctypes.data_as(C.POINTER(C.c_int32)))

    def delete_block(self, pos):
        p = np.asarray(pos, dtype=np.int32)
        return self.L.vhr_delete_hash_entry_element(C.byref(self.s.hd), C.byref(self.s.hp),
                                                    p.ctypes.data_as(C.POINTER(C.c_int32)))

    def insert_entry_bucket(self, pos, ptr):
        e = T.HashEntry()
        e.pos = (C.c_int32 * 3)(*[int(v) for v in pos])
        e.ptr = int(ptr)
        e.offset = 0
        return self.L.vhr_insert_hash_entry_bucket(C.byref(self.s.hd), C.byref(self.s.hp), C.byref(e))

    def get_entry(self, pos):
        p = np.asarray(pos, dtype=np.int32)
        e = self.L.vhr_get_hash_entry(C.byref(self.s.hd), C.byref(self.s.hp), p.ctypes.data_as(C.POINTER(C.c_int32)))
        return (tuple(e.pos), e.ptr, e.offset)
