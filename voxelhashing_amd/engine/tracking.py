"""The two camera trackers (DSC/CUDACameraTrackingMultiRes.h, CUDACameraTrackingMultiResRGBD.h) over the C ABI."""
import ctypes as C

import numpy as np

from .. import vhtypes as T
from ..lib import check, f16
from ._common import _Handle


class CUDACameraTrackingMultiRes(_Handle):
    """Mirror of DSC/CUDACameraTrackingMultiRes.h:17-78 over the C ABI (device pointers in, 4x4 pose out)."""

    _destroy = "vh_camera_tracking_destroy"

    def __init__(self, imageWidth, imageHeight, levels, stream=None):
        self._create("vh_camera_tracking_create", imageWidth, imageHeight, levels, stream)
        self.state = T.IcpState()

    def applyCT(self, d_input, d_inputNormals, d_model, d_modelNormals, lastTransform, settings, deltaTransformEstimate, cameraParams):
        """-> (4x4 float32 pose = lastTransform * delta, lost flag); the final VhIcpState is kept in self.state"""
        out = (C.c_float * 16)()
        lost = C.c_int(0)
        est = f16(deltaTransformEstimate) if deltaTransformEstimate is not None else None
        check(self.L.vh_camera_tracking_apply_ct(self.handle, d_input, d_inputNormals, d_model, d_modelNormals, f16(lastTransform), C.byref(settings),
                                                 est, C.byref(cameraParams), out, C.byref(lost), C.byref(self.state)), "applyCT")
        return np.array(out, dtype=np.float32).reshape(4, 4), bool(lost.value)


class CUDACameraTrackingMultiResRGBD(_Handle):
    """Mirror of DSC/CUDACameraTrackingMultiResRGBD.h:23-75 over the C ABI (device pointers in, 4x4 pose out)."""

    _destroy = "vh_camera_tracking_rgbd_destroy"

    def __init__(self, imageWidth, imageHeight, levels, stream=None):
        self._create("vh_camera_tracking_rgbd_create", imageWidth, imageHeight, levels, stream)
        self.state = T.IcpStateRGBD()

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
