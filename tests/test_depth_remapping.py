"""Depth-to-colour remapping (s_bUseCameraCalibration, DSC/CUDARGBDSensor.cpp:198-217): the depth map drawn into the
colour camera by the view passes (vh_view_raster + vh_view_resolve_depth), render target 0 into d_depthData.

CPU: the calibration keys of a parameter file; VhCalibrationState against its ctypes mirror; the identity rule
("already aligned"); the adapter matrices of the remap, the inverse depth intrinsics among them, against float32 and
float64 restatements.
GPU: the depth-only resolve bit for bit against tests/view_render.py and against vh_view_resolve's depth map; the sensor
with calibration on against the restatement chain (resample, remap, back-projection, normals), and bit-identical to
an untouched sensor when calibration is off or the extrinsic is the identity; end to end, a `.sens` from a rig whose
depth camera sits 5 cm beside the colour camera, replayed with --camera-calibration: the stripes of the final ray cast
lie where the colour camera saw them."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import view_render as V
from voxelhashing_amd import vhtypes as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINF = np.float32(-np.inf)
f32 = np.float32

# the calibration block of DepthSensingCUDA's zParametersDefault.txt (data only), with the switch turned on
CALIB_BLOCK = b"""s_remappingDepthDiscontinuityThresOffset = 0.012f;	// discontinuity offset in meter
s_remappingDepthDiscontinuityThresLin	 = 0.01f;	// additional discontinuity threshold per meter

s_bUseCameraCalibration = true;
"""


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def ordered(a):
    """float32 -> integers in the order of the floats, so that a difference is a count of ulps"""
    i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def remap_params(sizes, depth_k, color_k, extrinsic=np.eye(4), thres=(0.012, 0.01)):
    from voxelhashing_amd import lib
    p = T.ViewParams()
    lib.check(lib.load().vh_rgbd_sensor_remap_params((C.c_uint32 * 6)(*sizes), (C.c_float * 4)(*depth_k), (C.c_float * 4)(*color_k),
                                                     lib.f16(extrinsic), thres[0], thres[1], C.byref(p)), "vh_rgbd_sensor_remap_params")
    return p


def as_dict(p):
    return V.view_params(p.intrinsicInverse[:], p.modelview[:], p.intrinsicNew[:], (p.depthWidth, p.depthHeight), (p.screenWidth, p.screenHeight),
                         p.depthThreshOffset, p.depthThreshLin)


def adapter_intrinsics(k, size, adapter):
    """CUDARGBDAdapter.cpp:54-66 in float32: _m00 *= W / w, _m11 *= H / h, _m02 *= (W-1)/(w-1), _m12 *= (H-1)/(h-1)"""
    (w, h), (W, H) = size, adapter
    m = np.eye(4, dtype=np.float32)
    m[0, 0], m[1, 1] = f32(k[0]) * (f32(W) / f32(w)), f32(k[1]) * (f32(H) / f32(h))
    m[0, 2], m[1, 2] = f32(k[2]) * (f32(W - 1) / f32(w - 1)), f32(k[3]) * (f32(H - 1) / f32(h - 1))
    return m


# mLib's Matrix4x4::getInverse (core-math/matrix4x4.h:567-695), float32: entry n is six signed triple products summed
# left to right, then times 1 / det with det = m0 inv0 + m1 inv4 + m2 inv8 + m3 inv12
_COFACTORS = [
    "+5,10,15 -5,11,14 -9,6,15 +9,7,14 +13,6,11 -13,7,10", "-1,10,15 +1,11,14 +9,2,15 -9,3,14 -13,2,11 +13,3,10",
    "+1,6,15 -1,7,14 -5,2,15 +5,3,14 +13,2,7 -13,3,6", "-1,6,11 +1,7,10 +5,2,11 -5,3,10 -9,2,7 +9,3,6",
    "-4,10,15 +4,11,14 +8,6,15 -8,7,14 -12,6,11 +12,7,10", "+0,10,15 -0,11,14 -8,2,15 +8,3,14 +12,2,11 -12,3,10",
    "-0,6,15 +0,7,14 +4,2,15 -4,3,14 -12,2,7 +12,3,6", "+0,6,11 -0,7,10 -4,2,11 +4,3,10 +8,2,7 -8,3,6",
    "+4,9,15 -4,11,13 -8,5,15 +8,7,13 +12,5,11 -12,7,9", "-0,9,15 +0,11,13 +8,1,15 -8,3,13 -12,1,11 +12,3,9",
    "+0,5,15 -0,7,13 -4,1,15 +4,3,13 +12,1,7 -12,3,5", "-0,5,11 +0,7,9 +4,1,11 -4,3,9 -8,1,7 +8,3,5",
    "-4,9,14 +4,10,13 +8,5,14 -8,6,13 -12,5,10 +12,6,9", "+0,9,14 -0,10,13 -8,1,14 +8,2,13 +12,1,10 -12,2,9",
    "-0,5,14 +0,6,13 +4,1,14 -4,2,13 -12,1,6 +12,2,5", "+0,5,10 -0,6,9 -4,1,10 +4,2,9 +8,1,6 -8,2,5",
]


def mlib_inverse(m):
    m = np.asarray(m, np.float32).reshape(16)
    inv = np.zeros(16, np.float32)
    for n, terms in enumerate(_COFACTORS):
        acc = None
        for t in terms.split():
            a, b, c = (int(x) for x in t[1:].split(","))
            p = (m[a] * m[b]) * m[c]
            acc = (p if t[0] == "+" else -p) if acc is None else (acc + p if t[0] == "+" else acc - p)
        inv[n] = acc
    det = ((m[0] * inv[0] + m[1] * inv[4]) + m[2] * inv[8]) + m[3] * inv[12]
    return (inv * (f32(1) / det)).reshape(4, 4)


# ---------------------------------------------------------------------------------------------------------- CPU

def test_calibration_state_reader():
    from voxelhashing_amd import reconstruction as R
    cs = R.read_calibration_state(CALIB_BLOCK)
    assert cs.numKeysFound == 3 and cs.s_bUseCameraCalibration == 1
    assert cs.s_remappingDepthDiscontinuityThresOffset == f32(0.012) and cs.s_remappingDepthDiscontinuityThresLin == f32(0.01)
    # absent keys read as 0; ParameterFile's bool: only false / False / 0 are false
    cs = R.read_calibration_state(b"s_bUseCameraCalibration = 1;\ns_adapterWidth = 640;\n")
    assert cs.numKeysFound == 1 and cs.s_bUseCameraCalibration == 1
    assert cs.s_remappingDepthDiscontinuityThresOffset == 0.0 and cs.s_remappingDepthDiscontinuityThresLin == 0.0
    assert R.read_calibration_state(b"s_bUseCameraCalibration = False;").s_bUseCameraCalibration == 0
    assert R.read_calibration_state(b"// s_bUseCameraCalibration = true;\n").numKeysFound == 0
    # the file form: the reference's default file holds all three, with the switch off
    cs = R.read_calibration_state(os.path.join(ROOT, "tests", "golden", "reference", "zParametersDefault.txt"))
    assert cs.numKeysFound == 3 and cs.s_bUseCameraCalibration == 0 and cs.s_remappingDepthDiscontinuityThresLin == f32(0.01)
    # the other readers are unchanged by the block
    assert R.read_render_state(CALIB_BLOCK).numKeysFound == 0 and R.read_app_state(CALIB_BLOCK).numKeysFound == 0


def test_calibration_struct_layout():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "vh_types.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(VhCalibrationState), offsetof(VhCalibrationState, s_bUseCameraCalibration),
         offsetof(VhCalibrationState, s_remappingDepthDiscontinuityThresOffset), offsetof(VhCalibrationState, s_remappingDepthDiscontinuityThresLin),
         offsetof(VhCalibrationState, numKeysFound));
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = list(map(int, subprocess.check_output([exe]).decode().split()))
    S = T.CalibrationState
    assert got == [C.sizeof(S), S.s_bUseCameraCalibration.offset, S.s_remappingDepthDiscontinuityThresOffset.offset,
                   S.s_remappingDepthDiscontinuityThresLin.offset, S.numKeysFound.offset]


def _header(extrinsic):
    from voxelhashing_amd import sensor_data as SD
    return SD.SensorData.create((640, 480), (1280, 960), SD.make_intrinsic_matrix(570, 571, 319.5, 239.5), SD.make_intrinsic_matrix(1050, 1049, 640, 480),
                                depth_extrinsic=extrinsic).info()


def test_identity_rule(capsys):
    """RGBDSensor::initializeDepthExtrinsics: an identity depth extrinsic switches the key off, with the warning"""
    from voxelhashing_amd import reconstruction as R
    on = R.read_calibration_state(CALIB_BLOCK)
    assert R.camera_calibration(_header(np.eye(4)), on) is None
    assert R.IDENTITY_EXTRINSICS_WARNING in capsys.readouterr().err
    ext = np.eye(4, dtype=np.float32)
    ext[0, 3] = 0.025
    got = R.camera_calibration(_header(ext), on)
    assert got[:4] == (1050.0, 1049.0, 640.0, 480.0) and np.array_equal(got[4], ext)
    assert got[5:] == (f32(0.012), f32(0.01))
    assert capsys.readouterr().err == ""
    # the key off, or no state at all: nothing to do, nothing said
    assert R.camera_calibration(_header(ext), R.read_calibration_state(b"s_bUseCameraCalibration = false;")) is None
    assert R.camera_calibration(_header(ext), None) is None
    assert capsys.readouterr().err == ""
    # the comparison is exact: a rounding-level rotation is not "already aligned"
    ext = np.eye(4, dtype=np.float32)
    ext[0, 0] = np.nextafter(f32(1), f32(0))
    assert R.camera_calibration(_header(ext), on) is not None


def test_remap_params_on_the_host():
    rng = np.random.default_rng(7)
    ext = np.eye(4, dtype=np.float32)
    ext[:3, :3] = [[0.999, -0.02, 0.03], [0.021, 0.998, -0.01], [-0.03, 0.011, 0.999]]
    ext[:3, 3] = (0.052, -0.003, 0.001)
    # (depth size, colour size, adapter size, depth intrinsics, colour intrinsics)
    realistic = [((640, 480), (640, 480), (640, 480), (525, 525, 319.5, 239.5), (525, 525, 319.5, 239.5)),
                 ((640, 480), (1280, 960), (640, 480), (583.1, 579.4, 321.7, 238.2), (1049.9, 1050.3, 639.1, 481.7)),
                 ((640, 480), (640, 480), (1280, 960), (525, 525, 319.5, 239.5), (517.3, 516.5, 318.6, 255.3)),
                 ((512, 424), (1920, 1080), (640, 480), (365.5, 365.5, 257.3, 205.1), (1081.4, 1081.4, 959.5, 539.5)),
                 ((320, 240), (640, 480), (320, 240), (262.5, 262.5, 159.5, 119.5), (525, 525, 319.5, 239.5))]
    random = []
    for _ in range(300):
        dw, dh, cw, ch, W, H = (int(v) for v in rng.integers(2, 2000, 6))
        random.append(((dw, dh), (cw, ch), (W, H), tuple(rng.uniform(0.3, 2.0, 4) * (dw, dh, dw / 2, dh / 2)),
                       tuple(rng.uniform(0.3, 2.0, 4) * (cw, ch, cw / 2, ch / 2))))
    worst = {"realistic": 0, "random": 0}
    for kind, cases in (("realistic", realistic), ("random", random)):
        for dsize, csize, asize, dk, ck in cases:
            p = remap_params(dsize + csize + asize, dk, ck, ext, (0.012, 0.01))
            Kd, Kc = adapter_intrinsics(dk, dsize, asize), adapter_intrinsics(ck, csize, asize)
            inv = np.array(p.intrinsicInverse[:], np.float32).reshape(4, 4)
            assert np.array_equal(np.array(p.intrinsicNew[:], np.float32).reshape(4, 4), Kc)
            assert np.array_equal(np.array(p.modelview[:], np.float32).reshape(4, 4), ext)  # the extrinsic itself, not its inverse
            assert (p.depthWidth, p.depthHeight, p.screenWidth, p.screenHeight) == asize + asize
            assert (p.depthThreshOffset, p.depthThreshLin) == (f32(0.012), f32(0.01))
            # mLib's cofactor inverse, bit for bit
            assert np.array_equal(inv.view(np.uint32), mlib_inverse(Kd).view(np.uint32)), (dsize, asize, dk)
            # and close to the float64 inverse
            want = np.linalg.inv(Kd.astype(np.float64)).astype(np.float32)
            worst[kind] = max(worst[kind], int(np.abs(ordered(inv) - ordered(want)).max()))
    # the colour half agrees with the loop's own restatement (renderToFile's colour intrinsics)
    from voxelhashing_amd import reconstruction as R
    for dsize, csize, asize, dk, ck in realistic + random[:20]:
        p = remap_params(dsize + csize + asize, dk, ck)
        assert np.array_equal(np.array(p.intrinsicNew[:], np.float32).reshape(4, 4),
                              R.adapter_color_intrinsics(V.intrinsics(*ck), csize, asize))
    # the cofactor form rounds five times on the way to an entry (-mx fy, fx fy, 1 / det, the product): on real cameras
    # every entry is within one ulp of the float64 inverse; over arbitrary intrinsics within two
    assert worst["realistic"] <= 1, worst
    assert worst["random"] <= 2, worst
    # the same checks as the sensor's constructor
    from voxelhashing_amd import lib
    bad = lib.load().vh_rgbd_sensor_remap_params((C.c_uint32 * 6)(640, 480, 1, 480, 640, 480), (C.c_float * 4)(1, 1, 1, 1), (C.c_float * 4)(1, 1, 1, 1),
                                                lib.f16(np.eye(4)), 0.0, 0.0, C.byref(T.ViewParams()))
    assert bad != 0


# ---------------------------------------------------------------------------------------------------------- GPU

def scenes(W=640, H=480):
    """plane, a depth step, a sphere, noise with -inf holes (all at the 525/640 camera)"""
    rng = np.random.default_rng(5)
    K = V.intrinsics(525 * W / 640, 525 * W / 640, (W - 1) / 2, (H - 1) / 2)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    rx, ry = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
    a, b, c = rx * rx + ry * ry + 1, -2 * (0.1 * rx + 2.0), 0.01 + 4.0 - 0.49
    disc = b * b - 4 * a * c
    noise = (1.3 + 0.004 * rng.standard_normal((H, W))).astype(np.float32)
    noise[rng.random((H, W)) < 0.05] = MINF
    return K, dict(plane=np.full((H, W), 1.5, np.float32),
                   step=np.where(u < W * 0.55, 1.2 + 0.0005 * v, 2.0 + 0.0008 * u).astype(np.float32),
                   sphere=np.where(disc >= 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), -np.inf).astype(np.float32),
                   noise=noise)


def rig_extrinsic():
    """a depth camera 5 cm beside the colour camera, turned by a few degrees"""
    cx, sx, cy, sy = np.cos(0.03), np.sin(0.03), np.cos(-0.05), np.sin(-0.05)
    m = np.eye(4)
    m[:3, :3] = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    m[:3, 3] = (0.05, -0.004, 0.002)
    return m.astype(np.float32)


class GpuRemap:
    """vh_view_raster + vh_view_resolve_depth on device buffers of one adapter size"""

    def __init__(self, vh, lib, W, H):
        self.vh, self.lib, self.W, self.H = vh, lib, W, H
        self.keys = lib.DeviceBuffer(8 * W * H)
        lib.check(vh.vh_memset(self.keys.ptr, 0xFF, 8 * W * H, None), "memset")
        self.large = lib.DeviceBuffer(4 * vh.vh_view_large_list_words(W, H))
        lib.check(vh.vh_memset(self.large.ptr, 0, 4, None), "memset")
        self.out = lib.DeviceBuffer(4 * W * H)
        self.full = [lib.DeviceBuffer(4 * W * H)] + [lib.DeviceBuffer(16 * W * H) for _ in range(3)]
        self.colour = lib.DeviceBuffer.from_numpy(np.zeros((H, W, 4), np.float32))

    def assert_clean(self):
        assert np.all(self.keys.download(np.uint64, self.W * self.H) == V.EMPTY)
        assert self.large.download(np.uint32, 1)[0] == 0

    def remap(self, d_depth, params):
        """-> (depth map, keys between the passes, large-list count)"""
        from voxelhashing_amd import engine as E
        W, H = self.W, self.H
        self.lib.check(self.vh.vh_view_raster(d_depth, C.byref(params), self.keys.ptr, self.large.ptr, None), "vh_view_raster")
        keys = self.keys.download(np.uint64, W * H).reshape(H, W)
        n_large = int(self.large.download(np.uint32, 1)[0])
        E.view_resolve_depth(d_depth, params, self.keys.ptr, self.large.ptr, self.out.ptr)
        self.assert_clean()
        return self.out.download(np.float32, W * H).reshape(H, W), keys, n_large

    def full_resolve_depth(self, d_depth, params):
        """vh_view_resolve's depth map on the same raster"""
        vh, lib = self.vh, self.lib
        lib.check(vh.vh_view_raster(d_depth, C.byref(params), self.keys.ptr, self.large.ptr, None), "vh_view_raster")
        lib.check(vh.vh_view_resolve(d_depth, self.colour.ptr, C.byref(params), self.keys.ptr, self.large.ptr, *[b.ptr for b in self.full], None),
                  "vh_view_resolve")
        self.assert_clean()
        return self.full[0].download(np.float32, self.W * self.H).reshape(self.H, self.W)


@pytest.mark.gpu
def test_gpu_resolve_depth_bit_exact(vh):
    from voxelhashing_amd import lib
    W, H = 640, 480
    K, maps = scenes(W, H)
    Kinv = np.array(mlib_inverse(K), np.float32)
    close = np.eye(4, dtype=np.float32)
    close[2, 3] = -0.9
    views = [("rig", rig_extrinsic(), V.intrinsics(548.2, 546.9, 324.1, 251.6)),
             ("magnified", close, V.intrinsics(6000, 6000, (W - 1) / 2, (H - 1) / 2))]
    g = GpuRemap(vh, lib, W, H)
    for scene, depth in maps.items():
        d_depth = lib.DeviceBuffer.from_numpy(depth)
        for name, mv, Knew in views:
            p = V.view_params(Kinv, mv, Knew, (W, H), (W, H), 0.012, 0.01)
            want_keys, want = V.render_depth_map(depth, None, p)
            got, keys, n_large = g.remap(d_depth.ptr, T.make_view_params(Kinv, mv, Knew, (W, H), (W, H), 0.012, 0.01))
            what = f"{scene}/{name}"
            assert np.array_equal(keys, want_keys), f"{what}: {int((keys != want_keys).sum())} keys differ"
            assert same_bits(got, want["depth"]), f"{what}: {int((got.view(np.uint32) != want['depth'].view(np.uint32)).sum())} pixels differ"
            covered = int((want_keys != V.EMPTY).sum())
            assert covered > (1000 if (scene, name) != ("sphere", "magnified") else 0), (what, covered)
            assert np.all(got[want_keys == V.EMPTY] == MINF)
            if name == "magnified" and scene in ("plane", "step"):
                assert n_large > 100, (what, n_large)  # the large-triangle list was used
            # the full resolve's target 0 on the same raster is the same map
            assert same_bits(g.full_resolve_depth(d_depth.ptr, T.make_view_params(Kinv, mv, Knew, (W, H), (W, H), 0.012, 0.01)), got), what
    # two remaps of different inputs in a row, each right (no state carried over)
    p = V.view_params(Kinv, rig_extrinsic(), K, (W, H), (W, H), 0.012, 0.01)
    for scene in ("sphere", "step", "sphere"):
        got, _, _ = g.remap(lib.DeviceBuffer.from_numpy(maps[scene]).ptr, T.make_view_params(Kinv, rig_extrinsic(), K, (W, H), (W, H), 0.012, 0.01))
        assert same_bits(got, V.render_depth_map(maps[scene], None, p)[1]["depth"]), scene
    # argument checks: those of vh_view_resolve, and the output may not be the source
    d = lib.DeviceBuffer.from_numpy(maps["plane"])
    pp = T.make_view_params(Kinv, np.eye(4), K, (W, H), (W, H))
    assert vh.vh_view_resolve_depth(d.ptr, C.byref(pp), g.keys.ptr, g.large.ptr, d.ptr, None) != 0
    assert vh.vh_view_resolve_depth(d.ptr, C.byref(pp), g.keys.ptr, g.large.ptr, None, None) != 0
    assert vh.vh_view_resolve_depth(d.ptr, C.byref(T.make_view_params(Kinv, np.eye(4), K, (W, H), (1, H))), g.keys.ptr, g.large.ptr, g.out.ptr, None) != 0


def sensor_inputs(w, h, seed, cw=None, ch=None):
    """depth at the depth sensor's size, RGBX at the colour sensor's (cw x ch, default the same)"""
    cw, ch = cw or w, ch or h
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    d = (1.4 + 0.3 * np.sin(xx / 37.0) * np.cos(yy / 23.0) + 0.002 * rng.standard_normal((h, w))).astype(np.float32)
    d[:, int(0.6 * w):] += f32(0.5)  # a depth step, for the discontinuity threshold
    d[rng.random((h, w)) < 0.03] = 0.0  # no measurement
    c = rng.integers(1, 256, size=(ch, cw, 4), dtype=np.uint8)
    c[..., 3] = 255
    return d, c


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [(640, 480, 640, 480, 640, 480), (320, 240, 640, 480, 640, 480)])
def test_gpu_sensor_remap(vh, oracle_lib, sizes):
    from voxelhashing_amd import engine as E
    O = oracle_lib
    dw, dh, cw, ch, W, H = sizes
    dk = (525 * dw / 640, 525 * dw / 640, (dw - 1) / 2, (dh - 1) / 2)
    ck = (531.7, 530.2, 322.4, 244.9)
    ext = rig_extrinsic()

    def make(calibrate=None):
        s = E.CUDARGBDSensor((dw, dh), (cw, ch), (W, H), *dk, 0.5, 5.0)
        if calibrate is not None:
            s.setCameraCalibration(calibrate[0], *ck, calibrate[1], 0.012, 0.01)
        return s

    on, untouched = make((True, ext)), make()
    assert on.getCameraCalibration()[0] and not untouched.getCameraCalibration()[0]
    params = on.getCameraCalibration()[1]
    assert same_bits(params.intrinsicInverse[:], np.array(remap_params(sizes, dk, ck, ext).intrinsicInverse[:], np.float32))
    cp = on.getDepthCameraParams()  # the depth intrinsics, as in the reference (CUDARGBDSensor.cpp:133-140)
    assert bytes(cp) == bytes(untouched.getDepthCameraParams())
    for frame in range(2):  # the second frame reuses the keys the first left behind
        depth, colour = sensor_inputs(dw, dh, 10 + frame, cw, ch)
        on.process(depth, colour)
        got = on.download()
        resampled = O.image_op("resample_float_map", depth, dw, dh, out_size=(W, H), prefill=np.full((H, W), MINF, np.float32))
        _, maps = V.render_depth_map(resampled, None, as_dict(params))
        want = maps["depth"]
        assert same_bits(got["depth"], want), f"frame {frame}: {int((got['depth'].view(np.uint32) != want.view(np.uint32)).sum())} pixels differ"
        assert (want != MINF).mean() > 0.5
        cam = E.image_op("convert_depth_float_to_camera_space_float4", want, W, H, cp, out_channels=4)
        assert same_bits(got["camera_space"], cam)
        assert same_bits(got["normals"], E.image_op("compute_normals", cam, W, H, out_channels=4))
        untouched.process(depth, colour)
        ref = untouched.download()
        assert same_bits(got["color"], ref["color"]) and same_bits(got["intensity"], ref["intensity"])  # colour is not remapped
        assert not same_bits(got["depth"], ref["depth"])

    # with the depth filter on: the filtered map is remapped (the filter itself is held to 1e-5 elsewhere)
    for s in (on, untouched):
        s.setFiterDepthValues(True, 2.0, 0.1)
    depth, colour = sensor_inputs(dw, dh, 20, cw, ch)
    on.process(depth, colour)
    got = on.download()["depth"]
    resampled = O.image_op("resample_float_map", depth, dw, dh, out_size=(W, H), prefill=np.full((H, W), MINF, np.float32))
    filtered = O.image_op("gauss_filter_float_map", resampled, W, H, 2.0, 0.1)
    want = V.render_depth_map(filtered, None, as_dict(params))[1]["depth"]
    both = (got != MINF) & (want != MINF)
    assert both.sum() > 0.98 * max((got != MINF).sum(), (want != MINF).sum())  # coverage: a drop rule may flip on a filter ulp
    assert np.allclose(got[both], want[both], rtol=1e-5, atol=0)

    # calibration off, or an identity extrinsic: every map bit-identical to a sensor whose setter was never called
    for state in ((False, ext), (True, np.eye(4, dtype=np.float32))):
        s, ref = make(state), make()
        assert not s.getCameraCalibration()[0]
        for seed in (30, 31):
            depth, colour = sensor_inputs(dw, dh, seed, cw, ch)
            s.process(depth, colour)
            ref.process(depth, colour)
            a, b = s.download(), ref.download()
            for k in a:
                assert same_bits(a[k], b[k]), (state[0], k)
    # switched off again after being on: the copy path is back
    on.setFiterDepthValues(False)
    untouched.setFiterDepthValues(False)
    on.setCameraCalibration(False, *ck, ext, 0.012, 0.01)
    depth, colour = sensor_inputs(dw, dh, 40, cw, ch)
    on.process(depth, colour)
    untouched.process(depth, colour)
    a, b = on.download(), untouched.download()
    assert all(same_bits(a[k], b[k]) for k in a)


# ------------------------------------------------------------------------------------------------- end to end

F, BASELINE, Z = 510.0, 0.05, 1.5  # f b / z = 17 px of disparity
STRIPES = [(-0.50, -0.38), (-0.30, -0.18), (-0.10, 0.02), (0.10, 0.22), (0.30, 0.42)]  # boards on the plane z = 1.5 (world x)
E2E_PARAMS = """
s_sensorIdx = 8;
s_adapterWidth = 640;
s_adapterHeight = 480;
s_sensorDepthMax = 4.0f;
s_sensorDepthMin = 0.5f;
s_hashNumBuckets = 262144;
s_hashNumSDFBlocks = 131072;
s_hashMaxCollisionLinkedListSize = 7;
s_SDFVoxelSize = 0.002f;
s_SDFMarchingCubeThreshFactor = 10.0f;
s_SDFTruncation = 0.012f;
s_SDFTruncationScale = 0.004f;
s_SDFMaxIntegrationDistance = 4.0f;
s_SDFIntegrationWeightSample = 10;
s_SDFIntegrationWeightMax = 255;
s_SDFRayIncrementFactor = 0.8f;
s_SDFRayThresSampleDistFactor = 50.5f;
s_SDFRayThresDistFactor = 50.0f;
s_SDFUseGradients = false;
s_integrationEnabled = true;
s_trackingEnabled = true;
s_garbageCollectionEnabled = false;
s_marchingCubesMaxNumTriangles = 400000;
s_streamingEnabled = false;
s_offlineProcessing = true;
s_playData = true;
s_reconstructionEnabled = true;
s_binaryDumpSensorUseTrajectory = true;
s_remappingDepthDiscontinuityThresOffset = 0.012f;
s_remappingDepthDiscontinuityThresLin = 0.01f;
s_bUseCameraCalibration = false;
"""


def on_board(x):
    return np.any([(x >= a) & (x < b) for a, b in STRIPES], axis=0)


def rig_frames(poses, W=640, H=480):
    """(depth u16 mm, colour rgb) per colour-camera pose (a translation in x, y): the depth camera sits BASELINE to the
    right of the colour camera, both look down +z at the boards of the plane z = Z; outside the boards nothing is seen"""
    c = ((W - 1) / 2, (H - 1) / 2)
    u = np.arange(W, dtype=np.float64)
    frames = []
    for pose in poses:
        tx = float(pose[0, 3])
        colour = np.zeros((H, W, 3), np.uint8)
        colour[:, on_board(tx + Z * (u - c[0]) / F)] = (255, 230, 40)
        depth = np.zeros((H, W), np.uint16)
        depth[:, on_board(tx + BASELINE + Z * (u - c[0]) / F)] = int(round(1000 * Z))
        frames.append((depth, colour))
    return frames


def true_edges(tx, W=640):
    """the first and last colour-camera column whose pixel centre lies on each board"""
    c = (W - 1) / 2
    return [(int(np.ceil(c + F * (a - tx) / Z)), int(np.ceil(c + F * (b - tx) / Z)) - 1) for a, b in STRIPES]


def measured_edges(colors, rows):
    """per board, the median over rows of the first and last column where the ray cast is bright"""
    bright = (colors[rows, :, 0] > 0.5) & (colors[rows, :, 1] > 0.5) & (colors[rows, :, 2] < 0.5)
    out = []
    for k in range(len(STRIPES)):
        firsts, lasts = [], []
        for r in bright:
            cols = np.nonzero(r)[0]
            runs = np.split(cols, np.nonzero(np.diff(cols) > 1)[0] + 1) if len(cols) else []
            if len(runs) == len(STRIPES):
                firsts.append(runs[k][0])
                lasts.append(runs[k][-1])
        out.append((float(np.median(firsts)), float(np.median(lasts))) if firsts else (np.nan, np.nan))
    return out


@pytest.mark.gpu
def test_gpu_replay_colour_lands_on_the_geometry(vh, tmp_path, capsys):
    from voxelhashing_amd import reconstruction as R, sensor_data as SD
    W, H = 640, 480
    K = SD.make_intrinsic_matrix(F, F, (W - 1) / 2, (H - 1) / 2)
    ext = np.eye(4, dtype=np.float32)
    ext[0, 3] = BASELINE  # depth camera -> colour camera
    poses = []
    for k in range(3):
        p = np.eye(4, dtype=np.float32)
        p[0, 3], p[1, 3] = 0.004 * k, -0.002 * k
        poses.append(p)
    sens = {}
    for name, e in (("rig", ext), ("aligned", np.eye(4, dtype=np.float32))):
        sd = SD.SensorData.create((W, H), (W, H), K, K, 1000.0, "synthetic rig", SD.TYPE_RAW, SD.TYPE_ZLIB_USHORT, e)
        for (depth, colour), p in zip(rig_frames(poses), poses):
            sd.addFrame(np.ascontiguousarray(colour), depth, p)
        sens[name] = str(tmp_path / f"{name}.sens")
        sd.saveToFile(sens[name])
    params = str(tmp_path / "params.txt")
    open(params, "w").write(E2E_PARAMS)

    cmd = [sys.executable, os.path.join(ROOT, "tools", "replay.py"), "--params", params, "--sens", sens["rig"]]
    out = json.loads(subprocess.check_output(cmd + ["--camera-calibration"], timeout=600).decode().strip().splitlines()[-1])
    assert out["frames"] == 3 and out["camera_calibration"] is True and out["lost_frames"] == 0, out
    out = json.loads(subprocess.check_output(cmd, timeout=600).decode().strip().splitlines()[-1])
    assert out["frames"] == 3 and "camera_calibration" not in out, out

    g = R.read_app_state(params)
    rows = np.arange(H // 2 - 60, H // 2 + 60)
    edges = {}
    for key in (1, 0):
        cs = R.read_calibration_state(params)
        cs.s_bUseCameraCalibration = key
        rec = R.Reconstruction(g, None, [sens["rig"]], calibration_state=cs)
        assert rec.camera_calibration == bool(key)
        assert rec.run() == 3
        last = rec.scene.getLastRigidTransform().reshape(4, 4)
        assert np.array_equal(last, poses[-1])
        rec.ray.render(rec.scene.getHashData(), rec.scene.getHashParams(), rec.cp, last)
        edges[key] = measured_edges(rec.ray.download()["colors"], rows)
    want = true_edges(float(poses[-1][0, 3]))
    err_on = np.abs(np.array(edges[1]) - np.array(want))
    err_off = np.array(edges[0]) - np.array(want)
    print("true", want, "\ncalibrated", edges[1], "\nuncalibrated", edges[0])
    # with the remap every edge is where the colour camera saw it, up to the model's own resolution: a 2 mm voxel is 0.7 px
    # at 1.5 m, and the ray cast needs all eight voxels of a sample integrated, so a board's surface may end a voxel or
    # two inside its edge (measured: 0-2 px in, never out)
    assert np.all(err_on <= 2.0), (want, edges[1])
    assert np.abs(err_on).mean() <= 1.0, (want, edges[1])
    # without the remap the geometry sits where the depth camera saw it, f b / z = 17 px to the left: the right edge
    # of every board moves in by that much (its left edge is cut by the colour, which is right)
    disparity = F * BASELINE / Z
    assert np.all(np.abs(err_off[:, 1] + disparity) <= 2.0), (want, edges[0])
    assert np.all(np.abs(err_off[:, 0]) <= 2.0), (want, edges[0])

    # an aligned rig (identity extrinsic) with the key set: the reference's warning, and the remap stays off
    capsys.readouterr()
    cs = R.read_calibration_state(params)
    cs.s_bUseCameraCalibration = 1
    rec = R.Reconstruction(g, None, [sens["aligned"]], calibration_state=cs)
    assert not rec.camera_calibration and R.IDENTITY_EXTRINSICS_WARNING in capsys.readouterr().err
