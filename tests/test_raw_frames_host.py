"""Raw frames for the native frame loop (16-bit depth, RGB / RGBX bytes at the sensor's sizes), the parts that need no
device: the layout of the two new structs and the unchanged layout of the old ones, the argument checks of
vh_ingest_frame (made before anything touches the device), and the two host-only pieces of
reconstruction.Reconstruction.run_native: the refusal rule and the batch decoder."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from voxelhashing_amd import lib, vhtypes as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_structs_match_the_c_header_and_old_ones_keep_their_layout():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "vh_types.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(VhRawFrameFormat), sizeof(VhRawSequenceFrame), offsetof(VhRawFrameFormat, depthShift),
         offsetof(VhRawFrameFormat, s_colorFilter), offsetof(VhRawFrameFormat, s_colorSigmaR), offsetof(VhRawSequenceFrame, depth),
         offsetof(VhRawSequenceFrame, color));
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(VhReconstructionOptions), sizeof(VhSequenceFrame), sizeof(VhReconstructionStats), sizeof(VhFrameJob),
         sizeof(VhDepthCameraParams), sizeof(VhDepthCameraData));
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    new = [int(v) for v in out[0].split()]
    F, R = T.RawFrameFormat, T.RawSequenceFrame
    assert new == [C.sizeof(F), C.sizeof(R), F.depthShift.offset, F.s_colorFilter.offset, F.s_colorSigmaR.offset, R.depth.offset, R.color.offset]
    assert new == [44, 80, 16, 25, 40, 64, 72]
    old = [int(v) for v in out[1].split()]
    # the sizes at the parent commit
    assert old == [28, 80, 128, 448, 32, 16]
    assert old == [C.sizeof(t) for t in (T.ReconstructionOptions, T.SequenceFrame, T.ReconstructionStats, T.FrameJob, T.DepthCameraParams, T.DepthCameraData)]


def test_ingest_frame_checks_its_arguments_before_the_device():
    L = lib.load()
    BAD = 4  # VH_ERR_BAD_ARGUMENT
    p = 4096  # an aligned non-NULL "device pointer": never dereferenced, the call returns before any launch

    def call(depth=p, color=p + 4096, w=8, h=6, raw=p + 8192, dw=8, dh=6, craw=p + 12288, cw=8, ch=6, channels=3, shift=1000.0):
        return L.vh_ingest_frame(depth, color, w, h, raw, dw, dh, craw, cw, ch, channels, shift, None)

    assert call(depth=None) == BAD and call(raw=None) == BAD
    assert call(color=None) == BAD and call(craw=None) == BAD  # colour asked for, no colour map
    for size in (dict(w=1), dict(h=1), dict(w=0), dict(h=0), dict(dw=1), dict(dh=1), dict(cw=1), dict(ch=0)):
        assert call(**size) == BAD, size
    for channels in (1, 2, 5, 255):
        assert call(channels=channels) == BAD, channels
    for shift in (0.0, -1000.0, float("inf"), float("nan")):
        assert call(shift=shift) == BAD, shift
    assert call(depth=p + 4) == BAD and call(color=p + 8) == BAD  # 16-byte stores
    assert call(raw=p + 1) == BAD and call(channels=4, craw=p + 2) == BAD
    # the loop's entry points without a loop
    assert L.vh_reconstruction_set_raw_format(None, C.byref(T.RawFrameFormat())) == BAD
    assert L.vh_reconstruction_set_raw_format(None, None) == BAD
    assert L.vh_reconstruction_run_raw(None, None, 0) == BAD
    assert L.vh_reconstruction_run_raw_ahead(None, None, 3, None) == BAD


PARAMS = b"""
s_adapterWidth = 160;
s_adapterHeight = 120;
s_trackingEnabled = true;
s_integrationEnabled = true;
s_binaryDumpSensorUseTrajectory = true;
s_binaryDumpSensorUseTrajectoryOnlyInit = false;
"""


def test_run_native_refuses_what_the_native_loop_cannot_do():
    from voxelhashing_amd import reconstruction as R
    plain = R.read_app_state(PARAMS)
    assert R.native_refusal(plain) is None
    assert R.native_refusal(plain, R.read_render_state(b""), False, False) is None
    icp = R.read_app_state(PARAMS.replace(b"s_binaryDumpSensorUseTrajectory = true", b"s_binaryDumpSensorUseTrajectory = false"))
    assert "ICP" in R.native_refusal(icp)
    assert "ICP" in R.native_refusal(plain, use_rgbd_tracking=True)
    init = R.read_app_state(PARAMS.replace(b"OnlyInit = false", b"OnlyInit = true"))
    assert "s_binaryDumpSensorUseTrajectoryOnlyInit" in R.native_refusal(init)
    rec = R.read_app_state(PARAMS + b"s_recordData = true;\n")
    assert "s_recordData" in R.native_refusal(rec)
    rs = R.read_render_state(b"s_renderToFile = true;\n")
    assert rs.s_renderToFile and "s_renderToFile" in R.native_refusal(plain, rs)
    assert "s_bUseCameraCalibration" in R.native_refusal(plain, None, True)
    off = R.read_app_state(PARAMS.replace(b"s_trackingEnabled = true", b"s_trackingEnabled = false"))
    assert "s_trackingEnabled" in R.native_refusal(off)


def test_batch_decoder_returns_what_the_file_holds(tmp_path):
    from voxelhashing_amd import reconstruction as R, sensor_data as SD
    (dw, dh), (cw, ch), n = (24, 18), (30, 20), 7
    rng = np.random.default_rng(5)
    intr = SD.make_intrinsic_matrix(20.0, 20.0, 11.5, 8.5)
    sd = SD.SensorData.create((dw, dh), (cw, ch), intr, depth_shift=5000.0, depth_type=SD.TYPE_ZLIB_USHORT, color_type=SD.TYPE_RAW)
    depth = rng.integers(0, 65536, size=(n, dh, dw), dtype=np.uint16)
    depth[:, ::5, ::3] = 0
    color = rng.integers(0, 256, size=(n, ch, cw, 3), dtype=np.uint8)
    poses = rng.standard_normal((n, 16)).astype(np.float32)
    poses[3] = -np.inf  # an invalid pose is a pose like any other to the decoder
    for k in range(n):
        sd.addFrame(color[k], depth[k], poses[k], 10 + k, 20 + k)
    path = str(tmp_path / "t.sens")
    sd.saveToFile(path)
    back = SD.SensorData.loadFromFile(path)
    d, c, p = R.decode_batch(back, 0, n)
    assert d.dtype == np.uint16 and c.dtype == np.uint8 and p.dtype == np.float32
    assert np.array_equal(d, depth) and np.array_equal(c, color) and p.tobytes() == poses.tobytes()
    # a range in the middle, into buffers of the caller's (larger than the range)
    d_out, c_out = np.zeros((5, dh, dw), np.uint16), np.zeros((5, ch, cw, 3), np.uint8)
    d, c, p = R.decode_batch(back, 2, 3, d_out, c_out)
    assert np.array_equal(d, depth[2:5]) and np.array_equal(c, color[2:5]) and p.tobytes() == poses[2:5].tobytes()
    assert np.shares_memory(d, d_out) and np.shares_memory(c, c_out) and not d_out[3:].any()
    for bad in ((5, 3), (-1, 2), (0, n + 1)):
        try:
            R.decode_batch(back, *bad)
        except IndexError:
            continue
        raise AssertionError(f"range {bad} was accepted")
    try:
        R.decode_batch(back, 0, 2, np.zeros((2, dh, dw + 1), np.uint16))
    except ValueError:
        pass
    else:
        raise AssertionError("a depth buffer of the wrong shape was accepted")
