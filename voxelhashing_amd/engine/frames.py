"""Frames on the device: the depth + colour pair the scene integrates, synthetic frames, and the sensor
pre-processing (DSC/CameraUtil.cu) over the C ABI with numpy in and numpy out (tests, tools)."""
import ctypes as C

import numpy as np

from .. import vhtypes as T
from ..lib import DeviceBuffer, check, download, f16, load


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
