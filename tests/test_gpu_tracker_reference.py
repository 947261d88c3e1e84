"""The trackers' HIP kernels against the reference's own kernels, compiled for the CPU (oracle/_ref/libvh_ref.so, which
travels with the tree; nothing here reads the reference's sources).  tests/test_tracker_pinning.py holds the numpy
restatements to that library on the CPU; here the device is held to it directly, on the inputs where a rule shows: the
crafted 37x29 maps of tests/tracker_edges.py (levelFactor 1, 2 and 4) and the 50x38 level of the 202x154 pyramids, under
the cameras `tum` and `offcentre`.

- vh_icp_projective_correspondences: positions, normals and the pair weight bit for bit.  (The older tests grant the
  weight 1e-5 relative; the device's division, its cameraToKinectProjZ and its fmaxf stand in the reference's order and
  each rounds once, so nothing less than equality is asked here.)
- vh_icp_build_linear_system / vh_icp_rgbd_build_linear_system, and the fused vh_icp_step / vh_icp_rgbd_step, whose
  partials are the same rows: per-wave row counts equal to the reference's per-pixel counts summed over the wave's
  pixels, and EACH of the 30 sums within the float32 summation bound (assert_sums_within_float32_bound) of the float64
  sum of the reference's per-pixel terms.  The RGB-D kernels run at angles (0, 0, 0) (identity and a translation),
  where sin and cos are exact on both sides, and under two small rotations, where the reference is evaluated at the
  device's own angles: which rows are made is asserted exactly there too (no input sits within the trig slack of a
  threshold: the crafted threshold pixels are moved 6e-4 off it by the rotation).
"""
import ctypes as C

import numpy as np
import pytest

import icp_reference as S
import test_tracker_pinning as P
import tracker_edges as E
from oracle import icp
from oracle import reference as R
from test_camera_tracking import assert_sums_within_float32_bound, padded
from voxelhashing_amd import vhtypes as T

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.available(), reason="oracle/_ref/libvh_ref.so is not built")]

MINF = np.float32(-np.inf)
WINDOW = 12  # the depth tracker's lane window on every level
# delta estimates of the RGB-D cases as (rz, ry, rx, tx, ty, tz): angles 0 are exact on both sides; under the two small
# rotations the device's sin / cos meet the host libm's, and the crafted map's two normal-threshold pixels make both
# rows (+y) or none (-y) only if the input normal is rotated
RGBD_ESTIMATES = {"identity": (0, 0, 0, 0, 0, 0), "translation": (0, 0, 0, 0.006, 0.003, 0.001),
                  "rotation +y": (0.004, 0.003, 0.002, 0.003, -0.001, 0.002), "rotation -y": (0.004, -0.003, 0.002, 0.003, -0.001, 0.002)}
WANT_NORMAL_PIXELS = {"identity": [2, 0], "rotation +y": [2, 2], "rotation -y": [0, 0]}


def depth_cases(cam):
    """the crafted maps at levelFactor 1, 2, 4 and the 50x38 level of the sphere pyramid"""
    return [c for c in P.depth_cases(cam) if c[0].startswith("crafted") or c[0] == "spheres level 2"]


def rgbd_cases(cam):
    return [c for c in P.rgbd_cases(cam) if c[0] in ("crafted", "plane level 2")]


def wave_counts(rows, pixels_per_wave, nP):
    c = np.zeros(nP * pixels_per_wave, np.float64)
    c[:len(rows)] = rows[:, 29]
    return c.reshape(nP, pixels_per_wave).sum(1).astype(np.float32)


def assert_partials_against_reference_rows(part, rows, window, what):
    """part: the device's (nP, 30) wave partials; rows: the reference's (W H, 30) per-pixel terms"""
    nP = len(part)
    assert np.array_equal(part[:, 29], wave_counts(rows, 64 * window, nP)), (what, "rows per wave")
    r64 = rows.astype(np.float64)
    assert_sums_within_float32_bound(S.reduce_partials(part), r64.sum(0), np.abs(r64).sum(0), window, nP, what)


class DepthDevice:
    def __init__(self, vh, lib, delta):
        self.vh, self.lib = vh, lib
        self.up = lambda a: lib.DeviceBuffer.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        self.state, self.delta = lib.DeviceBuffer(C.sizeof(T.IcpState)), self.up(delta)
        self.ticket = lib.DeviceBuffer(4)
        self.begin()

    def begin(self):
        lib, vh = self.lib, self.vh
        lib.check(vh.vh_memset(self.state.ptr, 0, C.sizeof(T.IcpState), None))
        lib.check(vh.vh_memset(self.ticket.ptr, 0, 4, None))
        lib.check(vh.vh_icp_begin(self.state.ptr, self.delta.ptr, None))
        lib.check(vh.vh_icp_begin_level(self.state.ptr, None))


@pytest.mark.parametrize("cam", P.CAMERAS)
def test_gpu_depth_tracker_kernels_against_the_reference(vh, cam):
    from voxelhashing_amd import lib
    for what, i, inn, t, tn, lf, cp, _ in depth_cases(cam):
        h, w = i.shape[:2]
        nP = vh.vh_icp_num_partials(w, h)
        assert nP == -(-(w * h) // (64 * WINDOW))
        npx = nP * 64 * WINDOW
        for name, d in P.deltas().items():
            tag = f"{cam}, {what}, {name}"
            rc, rn = R.icp_correspondences(i, inn, t, tn, d.reshape(16), P.DIST_THRES, P.NORMAL_THRES, lf, cp)
            rows = R.icp_lane_sums(i, rc, rn, d.reshape(16), 1)
            ok = rc[..., 0] != MINF
            assert ok.sum() > 0.1 * w * h, tag
            dev = DepthDevice(vh, lib, d)
            up = dev.up
            # past the image the padded maps hold a pixel that pairs: a kernel reading there would add rows
            d_in, d_inn, d_t, d_tn = up(padded(i, npx, i[ok][0])), up(padded(inn, npx, inn[ok][0])), up(t), up(tn)
            d_c, d_cn = up(padded(rc, npx, rc[ok][0])), up(padded(rn, npx, rn[ok][0]))
            lib.check(vh.vh_icp_projective_correspondences(d_in.ptr, d_inn.ptr, d_t.ptr, d_tn.ptr, d_c.ptr, d_cn.ptr, w, h, P.DIST_THRES,
                                                           P.NORMAL_THRES, lf, dev.state.ptr, C.byref(cp), None))
            corr = d_c.download(np.float32, npx * 4).reshape(npx, 4)[:w * h].reshape(h, w, 4)
            corr_n = d_cn.download(np.float32, npx * 4).reshape(npx, 4)[:w * h].reshape(h, w, 4)
            assert np.array_equal(P.bits(corr), P.bits(rc)), (tag, "positions")
            assert np.array_equal(P.bits(corr_n), P.bits(rn)), (tag, "normals and pair weight")
            # the build step on the reference's own correspondences
            d_c, d_cn = up(padded(rc, npx, rc[ok][0])), up(padded(rn, npx, rn[ok][0]))
            d_part = lib.DeviceBuffer(nP * 30 * 4)
            lib.check(vh.vh_icp_build_linear_system(w, h, d_part.ptr, d_in.ptr, d_c.ptr, d_cn.ptr, dev.state.ptr, None))
            assert_partials_against_reference_rows(d_part.download(np.float32, nP * 30).reshape(nP, 30), rows, WINDOW, tag + ", build")
            # the fused step: its partials are the rows of its own correspondences
            d_part = lib.DeviceBuffer(nP * 30 * 4)
            lib.check(vh.vh_memset(d_part.ptr, 0xff, nP * 30 * 4, None))
            dev.begin()
            lib.check(vh.vh_icp_step(d_in.ptr, d_inn.ptr, d_t.ptr, d_tn.ptr, w, h, P.DIST_THRES, P.NORMAL_THRES, lf, C.byref(cp), d_part.ptr,
                                     dev.ticket.ptr, dev.state.ptr, 1.0, 1.0, 0.01, None, 0, None), "vh_icp_step")
            assert_partials_against_reference_rows(d_part.download(np.float32, nP * 30).reshape(nP, 30), rows, WINDOW, tag + ", fused step")


@pytest.mark.parametrize("cam", P.CAMERAS)
def test_gpu_rgbd_tracker_kernels_against_the_reference(vh, cam):
    from voxelhashing_amd import lib
    up = lambda a: lib.DeviceBuffer.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    for what, maps, prm, window in rgbd_cases(cam):
        pi, pn, pii, pm, pmn, pmiad = maps
        h, w = pi.shape[:2]
        level = {12: 0, 3: 1, 1: 2}[window]
        nP = vh.vh_icp_rgbd_num_partials(w, h, level)
        assert nP == -(-(w * h) // (64 * window))
        npx = nP * 64 * window
        dprm = T.IcpRGBDParams(fx=prm["fx"], fy=prm["fy"], mx=prm["mx"], my=prm["my"], weightDepth=prm["weightDepth"], weightColor=prm["weightColor"],
                               distThres=prm["distThres"], normalThres=prm["normalThres"], sensorMaxDepth=prm["sensorMaxDepth"],
                               colorGradientMin=prm["colorGradientMin"], colorThres=prm["colorThres"], level=level)
        for name, x in RGBD_ESTIMATES.items():
            tag = f"{cam}, {what}, {name}"
            delta = icp.delinearize(np.array(x, np.float32), 1.0, 1.0)
            d_state, d_delta, d_ticket = lib.DeviceBuffer(C.sizeof(T.IcpStateRGBD)), up(delta), lib.DeviceBuffer(4)

            def begin():
                lib.check(vh.vh_memset(d_state.ptr, 0, C.sizeof(T.IcpStateRGBD), None))
                lib.check(vh.vh_memset(d_ticket.ptr, 0, 4, None))
                lib.check(vh.vh_icp_rgbd_begin(d_state.ptr, d_delta.ptr, None))
                lib.check(vh.vh_icp_begin_level(d_state.ptr, None))

            begin()
            # the reference is evaluated at the device's own linearisation point
            st = T.IcpStateRGBD.from_buffer_copy(d_state.download(np.uint8, C.sizeof(T.IcpStateRGBD)).tobytes())
            angles, trans = np.array(st.angles, np.float32), np.array(st.translation, np.float32)
            assert np.array_equal(trans, delta[:3, 3]), tag
            if max(np.abs(x[:3])) == 0.0:
                assert np.abs(angles).max() == 0.0, tag
            else:  # eulerAngles(2, 1, 0) of Rz(x0) Ry(x1) Rx(x2), through float32 products, atan2 and sqrt
                assert np.abs(angles - np.array(x[:3], np.float32)).max() < 1e-6, (tag, angles)
            rows = R.icp_rgbd_lane_sums(*maps, angles, trans, prm, 1)
            assert rows[:, 29].sum() > 0.3 * w * h, tag
            if what == "crafted" and name in WANT_NORMAL_PIXELS:  # ROld turns the input normals over / under normalThres
                assert [int(rows[16 * E.W + px, 29]) for px in (31, 33)] == WANT_NORMAL_PIXELS[name], tag
            k = int(np.nonzero(rows[:, 29])[0][0])  # past the image the inputs hold a pixel that makes a row
            pad = lambda a, c: np.concatenate([a.reshape(-1, c), np.repeat(a.reshape(-1, c)[k:k + 1], npx - w * h, 0)])
            bufs = [up(pad(pi, 4)), up(pad(pn, 4)), up(pad(pii, 1)), up(pm), up(pmn), up(pmiad)]
            d_part = lib.DeviceBuffer(nP * 30 * 4)
            lib.check(vh.vh_icp_rgbd_build_linear_system(w, h, d_part.ptr, *[b.ptr for b in bufs], C.byref(dprm), d_state.ptr, None))
            assert_partials_against_reference_rows(d_part.download(np.float32, nP * 30).reshape(nP, 30), rows, window, tag + ", build")
            d_part = lib.DeviceBuffer(nP * 30 * 4)
            lib.check(vh.vh_memset(d_part.ptr, 0xff, nP * 30 * 4, None))
            begin()
            lib.check(vh.vh_icp_rgbd_step(w, h, d_part.ptr, d_ticket.ptr, *[b.ptr for b in bufs], C.byref(dprm), d_state.ptr, 1.0, 1.0, 0.01, None, 0,
                                          None), "vh_icp_rgbd_step")
            assert_partials_against_reference_rows(d_part.download(np.float32, nP * 30).reshape(nP, 30), rows, window, tag + ", fused step")
