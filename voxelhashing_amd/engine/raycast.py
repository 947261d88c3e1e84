"""CUDARayCastSDF (DepthSensingCUDA/Source/CUDARayCastSDF.h:13) over the C ABI."""
import ctypes as C

import numpy as np

from .. import vhtypes as T
from ..lib import DeviceBuffer, check, download, f16
from ._common import _Handle, _copy_struct, _scalar_out, _struct_out, _unpack_rgb


class CUDARayCastSDF(_Handle):
    _destroy = "vh_raycast_destroy"

    def __init__(self, params, stream=None):
        self.stream = stream
        self._params = _copy_struct(params)
        self._create("vh_raycast_create", C.byref(self._params), stream)

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
        d_org, d_dirs, d_t0, d_t1 = [DeviceBuffer.from_numpy(a, s) for a in (org, dirs, t0, t1)]
        d_t, d_col, d_st = DeviceBuffer(4 * n), DeviceBuffer(4 * n), DeviceBuffer(n)
        d_nrm = DeviceBuffer(12 * n) if normals else None
        check(self.L.vh_ray_cast_cast_rays(self.handle, C.byref(hashData), C.byref(hashParams), d_org.ptr, d_dirs.ptr, d_t0.ptr, d_t1.ptr, n,
                                           d_t.ptr, d_nrm.ptr if normals else None, d_col.ptr, d_st.ptr), "CUDARayCastSDF::castRays")
        return dict(t=d_t.download(np.float32, n, s), normal=d_nrm.download(np.float32, 3 * n, s).reshape(n, 3) if normals else None,
                    color=_unpack_rgb(d_col.download(np.uint32, n, s)), status=d_st.download(np.uint8, n, s))

    def getRayCastData(self):
        return _struct_out(T.RayCastData, "getRayCastData", self.L.vh_raycast_get_data, self.handle)

    def getRayCastParams(self):
        return _struct_out(T.RayCastParams, "getRayCastParams", self.L.vh_raycast_get_params, self.handle)

    def setTiming(self, on, march_only=False, stride=1):
        check(self.L.vh_raycast_set_timing_stride(self.handle, (2 if march_only else 1) if on else 0, stride), "setTiming")

    def setIntervalSplatting(self, on):
        check(self.L.vh_raycast_set_interval_splatting(self.handle, 1 if on else 0), "setIntervalSplatting")

    def getTileCapacity(self):
        """entries per tile list of the latest render(): 64, or 128 while fine voxels ask for large tile tables"""
        return _scalar_out(C.c_uint32, "getTileCapacity", self.L.vh_raycast_get_tile_capacity, self.handle)

    def getTimings(self):
        out = (C.c_double * 4)()
        check(self.L.vh_raycast_get_timings(self.handle, out), "getTimings")
        return dict(raycast_ms=out[0], normals_ms=out[1], frames=int(out[2]), splat_ms=out[3])

    def getEventPairOverheadMs(self):
        return _scalar_out(C.c_double, "getEventPairOverhead", self.L.vh_raycast_get_event_pair_overhead, self.handle)

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
