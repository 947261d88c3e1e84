"""CUDARGBDSensor over CUDARGBDAdapter (include/vh.hpp) over the C ABI."""
import ctypes as C

import numpy as np

from .. import vhtypes as T
from ..lib import check, download, f16
from ._common import _Handle, _struct_out


class CUDARGBDSensor(_Handle):
    """Mirror of CUDARGBDSensor over CUDARGBDAdapter (include/vh.hpp) over the C ABI."""

    _destroy = "vh_rgbd_sensor_destroy"

    def __init__(self, depth_size, color_size, adapter_size, fx, fy, mx, my, depth_min, depth_max, stream=None):
        self.size = tuple(adapter_size)
        sizes = (C.c_uint32 * 6)(depth_size[0], depth_size[1], color_size[0], color_size[1], adapter_size[0], adapter_size[1])
        intr = (C.c_float * 6)(fx, fy, mx, my, depth_min, depth_max)
        self._create("vh_rgbd_sensor_create", sizes, intr, stream)

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
        return _struct_out(T.DepthCameraData, "getDepthCameraData", self.L.vh_rgbd_sensor_get_depth_camera_data, self.handle)

    def getDepthCameraParams(self):
        return _struct_out(T.DepthCameraParams, "getDepthCameraParams", self.L.vh_rgbd_sensor_get_depth_camera_params, self.handle)

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
