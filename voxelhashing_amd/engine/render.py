"""Shaded rendering: RGBDRenderer (DSC/DX11RGBDRenderer.h), PhongLighting (DSC/DX11PhongLighting.h) and what goes
with them over the C ABI."""
import ctypes as C

import numpy as np

from .. import vhtypes as T
from ..lib import check, download, f16, load
from ._common import _Handle, _copy_struct


def view_resolve_depth(d_depth, params, d_keys, d_large_list, d_out_depth, stream=None):
    """vh_view_resolve_depth: render target 0 of the keys vh_view_raster left (device pointers; params a ViewParams)"""
    check(load().vh_view_resolve_depth(d_depth, C.byref(params), d_keys, d_large_list, d_out_depth, stream), "vh_view_resolve_depth")


class RGBDRenderer(_Handle):
    """Mirror of DX11RGBDRenderer (DSC/DX11RGBDRenderer.h) over the C ABI: RenderDepthMap draws a depth map as a mesh into
    four screen-size device maps (depth f32, position / normal / colour float4)."""

    _destroy = "vh_rgbd_renderer_destroy"

    def __init__(self, stream=None):
        self.stream = stream
        self._create("vh_rgbd_renderer_create", stream)

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
        depth, positions, normals, colors = [p.value for p in ptrs]
        return dict(depth=depth, positions=positions, normals=normals, colors=colors, size=(size[0], size[1]))

    def download(self):
        m = self.getMaps()
        W, H = m["size"]
        s = self.stream
        return dict(depth=download(m["depth"], np.float32, H * W, s).reshape(H, W),
                    positions=download(m["positions"], np.float32, H * W * 4, s).reshape(H, W, 4),
                    normals=download(m["normals"], np.float32, H * W * 4, s).reshape(H, W, 4),
                    colors=download(m["colors"], np.float32, H * W * 4, s).reshape(H, W, 4))


class PhongLighting(_Handle):
    """Mirror of DX11PhongLighting (DSC/DX11PhongLighting.h): PhongPS over three float4 device maps; the light is a
    PhongLight (phong_light_from_render_state)."""

    _destroy = "vh_phong_lighting_destroy"

    def __init__(self, light, stream=None):
        self.stream = stream
        self.light = _copy_struct(light)
        self._create("vh_phong_lighting_create", C.byref(self.light), stream)
        self.size = (0, 0)

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
