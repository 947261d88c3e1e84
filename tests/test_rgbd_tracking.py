"""RGB-D camera tracking (CUDACameraTrackingMultiResRGBD): depth + photometric multi-resolution ICP.

The scene is a fronto-parallel textured plane (tests/rgbd_icp.py): an in-plane camera motion leaves every
point-to-plane residual at zero, so the geometric tracker (f5) cannot see it, while the texture pins it for the
photometric term.

CPU: the tracking parameter file with the four colour keys; the new structs against their ctypes mirrors; the numpy
restatement recovers an in-plane motion that oracle.icp (f5) misses, also from a delta estimate whose Euler angles sit
on the far branch (near (pi, pi, pi)).
GPU: k_intensity_and_derivatives bit for bit; one build step (which rows pair up: exactly; the 30 sums: 1e-5 of the
largest term); applyCT on an integrated, ray-cast plane against the restatement (1e-4 absolute per pose entry, same
iterations, numCorr, lost flag) and against the true motion; lost tracking; tools/replay.py --rgbd-tracking."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import rgbd_icp as G
from voxelhashing_amd import synth, vhtypes as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINF = np.float32(-np.inf)

# DepthSensingCUDA's zParametersTrackingDefault.txt, inlined (data only)
TRACKING_DEFAULT = b"""//Default Tracking Parameters
s_maxLevels = 3;

s_maxOuterIter[0] = 8;
s_maxInnerIter[0] = 1;
s_distThres[0] = 0.15f;
s_normalThres[0] = 0.97f;
s_angleTransThres[0] = 1.0f;// radians
s_distTransThres[0] = 1.0f; // meters
s_residualEarlyOut[0] = 0.01f;	//causes an early out if residual is smaller than this number (no early out if set to zero)
s_weightsDepth[0] = 1.0f;
s_weightsColor[0] = 0.0f;
s_colorGradientMin[0] = 0.005f;
s_colorThres[0] = 0.1f;

s_maxOuterIter[1] = 6;
s_maxInnerIter[1] = 1;
s_distThres[1] = 0.15f;
s_normalThres[1] = 0.97f;
s_angleTransThres[1] = 1.0f;// radians
s_distTransThres[1] = 1.0f; // meters
s_residualEarlyOut[1] = 0.01f;	//causes an early out if residual is smaller than this number (no early out if set to zero)
s_weightsDepth[1] = 0.5f;
s_weightsColor[1] = 0.5f;
s_colorGradientMin[1] = 0.005f;
s_colorThres[1] = 0.1f;

s_maxOuterIter[2] = 4;
s_maxInnerIter[2] = 1;
s_distThres[2] = 0.15f;
s_normalThres[2] = 0.97f;
s_angleTransThres[2] = 1.0f;// radians
s_distTransThres[2] = 1.0f; // meters
s_residualEarlyOut[2] = 0.01;	//causes an early out if residual is smaller than this number (no early out if set to zero)
s_weightsDepth[2] = 0.5f;
s_weightsColor[2] = 0.5f;
s_colorGradientMin[2] = 0.005f;
s_colorThres[2] = 0.1f;

s_maxOuterIter[3] = 4;
s_maxInnerIter[3] = 1;
s_distThres[3] = 0.15f;
s_normalThres[3] = 0.97f;
s_angleTransThres[3] = 1.0f;// radians
s_distTransThres[3] = 1.0f; // meters
s_residualEarlyOut[3] = 0.01f;	//causes an early out if residual is smaller than this number (no early out if set to zero)
s_weightsDepth[3] = 0.5f;
s_weightsColor[3] = 0.5f;
s_colorGradientMin[3] = 0.005f;
s_colorThres[3] = 0.1f;
"""


def pose_error(a, b):
    a, b = np.asarray(a, np.float64).reshape(4, 4), np.asarray(b, np.float64).reshape(4, 4)
    rel = np.linalg.inv(a) @ b
    ang = np.degrees(np.arccos(np.clip(0.5 * (np.trace(rel[:3, :3]) - 1.0), -1, 1)))
    return float(np.linalg.norm(rel[:3, 3])), float(ang)


def all_colour_settings(**kw):
    """a non-zero colour weight on every level"""
    return T.make_tracking_state_rgbd(weights_depth=(1.0, 0.5, 0.5), weights_color=(0.5, 0.5, 0.5), **kw)


# ---------------------------------------------------------------------------- CPU

def test_rgbd_tracking_parameter_file():
    from voxelhashing_amd import lib
    L = lib.load()
    ts, f5 = T.TrackingStateRGBD(), T.TrackingState()
    lib.check(L.vh_tracking_state_rgbd_parse(TRACKING_DEFAULT, C.byref(ts)), "rgbd parse")
    lib.check(L.vh_tracking_state_parse(TRACKING_DEFAULT, C.byref(f5)), "parse")
    assert list(ts.s_weightsDepth)[:4] == [1.0, 0.5, 0.5, 0.5]
    assert list(ts.s_weightsColor)[:4] == [0.0, 0.5, 0.5, 0.5]
    assert all(ts.s_colorGradientMin[i] == np.float32(0.005) and ts.s_colorThres[i] == np.float32(0.1) for i in range(4))
    assert bytes(ts.base) == bytes(f5)  # the f5 members exactly as the f5 reader returns them
    for i in range(4, 8):  # levels the file does not name: setDefault's values
        assert (ts.s_weightsDepth[i], ts.s_weightsColor[i]) == (1.0, 1.0)
        assert ts.s_colorGradientMin[i] == np.float32(0.005) and ts.s_colorThres[i] == np.float32(0.1)
    # a file without any colour key: the defaults on every level, the f5 keys untouched
    plain = b"s_maxLevels = 1;\ns_maxOuterIter[0] = 3;\ns_weightsColor[1] = 0.25;\n"
    lib.check(L.vh_tracking_state_rgbd_parse(plain, C.byref(ts)), "rgbd parse")
    lib.check(L.vh_tracking_state_parse(plain, C.byref(f5)), "parse")
    assert bytes(ts.base) == bytes(f5) and ts.base.s_maxOuterIter[0] == 3 and ts.base.numLevelsFound == 1
    assert ts.s_weightsColor[0] == 1.0 and ts.s_weightsColor[1] == 0.25 and ts.s_weightsDepth[0] == 1.0
    # the file reader agrees with the text parser
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "t.txt")
        open(path, "wb").write(TRACKING_DEFAULT)
        rd = T.TrackingStateRGBD()
        lib.check(L.vh_tracking_state_rgbd_read(path.encode(), C.byref(rd)), "rgbd read")
        lib.check(L.vh_tracking_state_rgbd_parse(TRACKING_DEFAULT, C.byref(ts)), "rgbd parse")
        assert bytes(rd) == bytes(ts)
    assert L.vh_tracking_state_rgbd_read(b"/nonexistent/file.txt", C.byref(rd)) != 0


def test_rgbd_struct_layouts():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "vh_types.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(VhTrackingStateRGBD), offsetof(VhTrackingStateRGBD, s_weightsDepth),
         offsetof(VhTrackingStateRGBD, s_weightsColor), offsetof(VhTrackingStateRGBD, s_colorGradientMin),
         offsetof(VhTrackingStateRGBD, s_colorThres), sizeof(VhTrackingState));
  printf("%zu %zu %zu %zu\n", sizeof(VhIcpStateRGBD), offsetof(VhIcpStateRGBD, angles), offsetof(VhIcpStateRGBD, translation), sizeof(VhIcpState));
  printf("%zu %zu %zu %zu\n", sizeof(VhIcpRGBDParams), offsetof(VhIcpRGBDParams, weightDepth), offsetof(VhIcpRGBDParams, sensorMaxDepth),
         offsetof(VhIcpRGBDParams, level));
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [list(map(int, line.split())) for line in subprocess.check_output([exe]).decode().split("\n") if line.strip()]
    S, I, P = T.TrackingStateRGBD, T.IcpStateRGBD, T.IcpRGBDParams
    assert got[0] == [C.sizeof(S), S.s_weightsDepth.offset, S.s_weightsColor.offset, S.s_colorGradientMin.offset, S.s_colorThres.offset,
                      C.sizeof(T.TrackingState)]
    assert got[1] == [C.sizeof(I), I.angles.offset, I.translation.offset, C.sizeof(T.IcpState)]
    assert got[2] == [C.sizeof(P), P.weightDepth.offset, P.sensorMaxDepth.offset, P.level.offset]


def plane_maps(cp, tx_prev, tx_cur):
    prev, cur = G.plane_pose(tx_prev), G.plane_pose(tx_cur)
    model = G.sensor_maps(*G.plane_frame(prev, cp), cp)
    inp = G.sensor_maps(*G.plane_frame(cur, cp), cp)
    return prev, cur, inp, model


def test_restatement_tracks_in_plane_motion_that_geometry_misses(oracle_lib):
    restatement_tracks_in_plane_motion(T.make_depth_camera_params(160, 120))


def restatement_tracks_in_plane_motion(cp, tx=0.02):
    from oracle import icp
    prev, cur, (i, inn, ic), (m, mn, mc) = plane_maps(cp, 0.0, tx)
    eye = np.eye(4, dtype=np.float32)
    got, info = G.apply_ct(i, inn, ic, m, mn, mc, prev, all_colour_settings(), eye, cp, 3)
    assert got is not None and info["numCorr"] > 10000
    dt, da = pose_error(got, cur)
    assert dt < 0.003 and da < 0.1, (dt, da)
    f5, _ = icp.apply_ct(i, inn, m, mn, prev, T.make_tracking_state(), eye, cp, 3)
    assert f5 is None or pose_error(f5, cur)[0] > 0.01
    # the reference's own default settings (no colour on level 0) still beat the geometry
    got, _ = G.apply_ct(i, inn, ic, m, mn, mc, prev, T.make_tracking_state_rgbd(), eye, cp, 3)
    assert got is not None and pose_error(got, cur)[0] < 0.01


def test_restatement_euler_branch_near_identity(oracle_lib):
    """eulerAngles(2, 1, 0) returns its first angle in [0, pi]: a small negative z-rotation comes back near
    (pi, pi, pi), and the Gauss-Newton steps taken in those angles still converge"""
    R = np.asarray(G.plane_pose(0.0, rz_deg=-0.3), np.float32).reshape(4, 4)[:3, :3]
    e = G.euler_angles_zyx(R)
    assert np.all(np.abs(np.abs(e) - np.pi) < 0.01), e
    assert np.abs(G.delinearize(e).reshape(3, 3) - R).max() < 1e-6
    assert np.abs(G.euler_angles_zyx(np.eye(3, dtype=np.float32))).max() == 0.0
    cp = T.make_depth_camera_params(160, 120)
    prev, cur, (i, inn, ic), (m, mn, mc) = plane_maps(cp, 0.0, 0.015)
    est = np.asarray(G.plane_pose(0.004, rz_deg=-0.3), np.float32).reshape(4, 4)
    got, info = G.apply_ct(i, inn, ic, m, mn, mc, prev, all_colour_settings(), est, cp, 3)
    assert got is not None
    dt, da = pose_error(got, cur)
    assert dt < 0.003 and da < 0.1, (dt, da)


# ---------------------------------------------------------------------------- GPU

class PlaneRig:
    """scene at 1 cm voxels + ray caster + sensor + both trackers on the GPU, fed with the textured plane"""

    def __init__(self, E, cp, levels=3):
        self.E, self.cp = E, cp
        self.hp = T.make_hash_params(1 << 15, 1 << 14, **synth.PARAM_SETS["P1"])
        self.scene = E.CUDASceneRepHashSDF(self.hp, T.make_scene_options(offline=True, gc=False))
        self.ray = E.CUDARayCastSDF(T.make_raycast_params(self.hp, cp))
        W, H = cp.m_imageWidth, cp.m_imageHeight
        self.sensor = E.CUDARGBDSensor((W, H), (W, H), (W, H), cp.fx, cp.fy, cp.mx, cp.my, cp.m_sensorDepthWorldMin, cp.m_sensorDepthWorldMax)
        self.rgbd = E.CUDACameraTrackingMultiResRGBD(W, H, levels)
        self.f5 = E.CUDACameraTrackingMultiRes(W, H, levels)

    def feed(self, pose):
        self.sensor.process(*G.plane_frame(pose, self.cp))

    def integrate(self, pose):
        cam = self.sensor.getDepthCameraData()
        self.scene.integrate(pose, self.E.DepthFrame(self.cp, depth_ptr=cam.d_depthData, color_ptr=cam.d_colorData), self.cp, None)

    def render(self, pose):
        self.ray.render(self.scene.getHashData(), self.scene.getHashParams(), self.cp, pose)
        return self.ray.getRayCastData()

    def maps(self):
        from voxelhashing_amd import lib
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        lib.check(lib.load().vh_rgbd_sensor_get_maps(self.sensor.handle, C.byref(a), C.byref(b), C.byref(c)), "maps")
        return a, b, self.sensor.getDepthCameraData().d_colorData

    def track_rgbd(self, last_pose, ts, estimate=None):
        rd = self.render(last_pose)
        a, b, col = self.maps()
        return self.rgbd.applyCT(a, b, col, rd.d_depth4, rd.d_normals, rd.d_colors, last_pose, ts, estimate, self.cp)

    def track_f5(self, last_pose, ts):
        rd = self.render(last_pose)
        a, b, _ = self.maps()
        return self.f5.applyCT(a, b, rd.d_depth4, rd.d_normals, last_pose, ts, None, self.cp)


@pytest.mark.gpu
def test_gpu_intensity_and_derivatives_bit_exact(vh):
    from voxelhashing_amd import lib
    rng = np.random.default_rng(5)
    for W, H in ((160, 120), (37, 23), (3, 3), (2, 5)):
        img = rng.random((H, W), dtype=np.float32)
        img[rng.random((H, W)) < 0.05] = MINF  # holes
        d_in = lib.DeviceBuffer.from_numpy(img)
        d_out = lib.DeviceBuffer(W * H * 16)
        lib.check(vh.vh_compute_intensity_and_derivatives(d_in.ptr, W, H, d_out.ptr, None), "intensity_and_derivatives")
        got = d_out.download(np.float32, W * H * 4).reshape(H, W, 4)
        want = G.intensity_and_derivatives(img)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (W, H)
        if W > 2 and H > 2 and W * H > 100:
            valid = want[..., 0] != MINF
            assert 0 < valid.sum() < W * H and np.all(want[0, :, 0] == MINF) and np.all(want[:, -1, 0] == MINF)


def _one_build_step(vh, lib, cp, inp, model, delta):
    """vh_icp_rgbd_begin + one build on level 0 -> (wave partials, device state, the restatement's partials)"""
    W, H = cp.m_imageWidth, cp.m_imageHeight
    (i, inn, ic), (m, mn, mc) = inp, model
    ii, miad = G.intensity(ic), G.intensity_and_derivatives(G.intensity(mc))
    up = lambda a: lib.DeviceBuffer.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    bufs = [up(a) for a in (i, inn, ii, m, mn, miad)]
    d_state, d_delta = lib.DeviceBuffer(C.sizeof(T.IcpStateRGBD)), up(delta)
    ts = all_colour_settings()
    p = G.level_params(ts, 0, cp)
    prm = T.IcpRGBDParams(fx=p["fx"], fy=p["fy"], mx=p["mx"], my=p["my"], weightDepth=p["weightDepth"], weightColor=p["weightColor"],
                          distThres=p["distThres"], normalThres=p["normalThres"], sensorMaxDepth=p["sensorMaxDepth"],
                          colorGradientMin=p["colorGradientMin"], colorThres=p["colorThres"], level=0)
    nP = vh.vh_icp_rgbd_num_partials(W, H, 0)
    assert nP == -(-(W * H) // (64 * 12))
    d_part = lib.DeviceBuffer(nP * 30 * 4)
    lib.check(vh.vh_icp_rgbd_begin(d_state.ptr, d_delta.ptr, None))
    lib.check(vh.vh_icp_rgbd_build_linear_system(W, H, d_part.ptr, *[b.ptr for b in bufs], C.byref(prm), d_state.ptr, None))
    part = d_part.download(np.float32, nP * 30).reshape(nP, 30)
    st = T.IcpStateRGBD.from_buffer_copy(d_state.download(np.uint8, C.sizeof(T.IcpStateRGBD)).tobytes())
    angles = G.euler_angles_zyx(np.asarray(delta, np.float32).reshape(4, 4)[:3, :3])
    trans = np.asarray(delta, np.float32).reshape(4, 4)[:3, 3]
    return part, st, (i, inn, ii, m, mn, miad), p, angles, trans


@pytest.mark.gpu
def test_gpu_rgbd_build_step_matches_restatement(vh, oracle_lib):
    """which rows pair up: exactly; EACH of the 30 sums within the float32 bound of its summation (a wrong small term --
    an ATb entry, a colour row's Jacobian column -- does not hide behind the largest one).  On the far Euler branch the
    restatement is evaluated at the device's own angles; tests/test_tracker_pinning.py holds that evaluation to the
    reference's kernel."""
    import icp_reference as R
    from test_camera_tracking import assert_sums_within_float32_bound
    from voxelhashing_amd import lib
    cp = T.make_depth_camera_params(160, 120)
    W, H = cp.m_imageWidth, cp.m_imageHeight
    _, _, inp, model = plane_maps(cp, 0.0, 0.02)
    for delta, exact in ((np.eye(4, dtype=np.float32), True), (np.asarray(G.plane_pose(0.006, 0.002, rz_deg=-0.4), np.float32).reshape(4, 4), False)):
        part, st, maps, p, angles, trans = _one_build_step(vh, lib, cp, inp, model, delta)
        if exact:
            assert np.abs(np.array(st.angles)).max() == 0.0
        else:  # the far Euler branch: the kernel linearises at (pi, +-pi, +-pi), as the reference's Eigen does
            assert np.all(np.abs(np.abs(np.array(st.angles)) - np.pi) < 0.02), list(st.angles)
            assert np.abs(np.array(st.angles) - angles).max() < 1e-5
        at = np.array(st.angles, np.float32)
        dterm, cterm, dmask, cmask = G.pixel_terms(*maps, at, trans, p)
        assert dmask.sum() > 5000 and cmask.sum() > 1000
        want = G.build_partials(H, W, 0, dterm, cterm)
        # which rows pair up: the per-wave row counts are exact
        assert np.array_equal(part[:, 29], want[:, 29]), np.abs(part[:, 29] - want[:, 29]).max()
        sign = np.ones(30)
        sign[21:27] = -1.0  # the kernel subtracts the J^T F products
        want_sum = ((dterm.astype(np.float64) + cterm.astype(np.float64)) * sign).sum(0)
        abs_sum = np.abs(dterm.astype(np.float64)).sum(0) + np.abs(cterm.astype(np.float64)).sum(0)
        assert_sums_within_float32_bound(R.reduce_partials(part), want_sum, abs_sum, 12, len(part), f"exact angles: {exact}")


@pytest.mark.gpu
def test_gpu_apply_ct_equals_restatement(vh, oracle_lib):
    apply_ct_equals_restatement(160, 120)


@pytest.mark.gpu
@pytest.mark.slow
def test_gpu_apply_ct_at_sensor_size(vh, oracle_lib):
    """the same bar at 640x480, the size tools/bench_tracking.py --rgbd measures"""
    apply_ct_equals_restatement(640, 480)


def apply_ct_equals_restatement(W, H):
    from voxelhashing_amd import engine as E
    cp = T.make_depth_camera_params(W, H)
    rig = PlaneRig(E, cp)
    poses = [G.plane_pose(0.01 * k) for k in range(3)]
    # a voxel's colour is a running 50/50 average that starts from black (combineVoxel), so the model is integrated
    # six times at the pose it is ray-cast from: its colours are then within 2 % of the texture's
    for _ in range(6):
        rig.feed(poses[1])
        rig.integrate(poses[1])
    cur = G.plane_pose(0.035)
    rig.feed(cur)
    ts = all_colour_settings()
    got, lost = rig.track_rgbd(poses[1], ts)
    assert not lost
    model, inp = rig.ray.download(), rig.sensor.download()
    want, info = G.apply_ct(inp["camera_space"], inp["normals"], inp["color"], model["depth4"], model["normals"], model["colors"], poses[1], ts,
                            np.eye(4, dtype=np.float32), cp, 3)
    assert want is not None
    assert np.abs(got - want).max() < 1e-4, np.abs(got - want).max()
    st = rig.rgbd.state.icp
    # the linearisation point goes through atan2 / sin / cos, whose device and numpy results may differ in the last bit
    # once the estimate is no longer the identity: a row sitting exactly at a threshold can flip (measured: 2 of 35 767)
    assert st.iterations == info["iterations"] and st.lost == 0
    assert abs(st.numCorr - info["numCorr"]) <= 1e-3 * info["numCorr"], (st.numCorr, info["numCorr"])
    # (a flipped colour row moves the residual sum by up to weight * colorThres^2 = 0.005)
    assert abs(st.sumRegError - info["sumRegError"]) <= 1e-3 * max(1.0, info["sumRegError"])
    dt, da = pose_error(got, cur)
    assert dt < 0.003 and da < 0.1, (dt, da)


@pytest.mark.gpu
def test_gpu_rgbd_lost_tracking(vh, oracle_lib):
    from voxelhashing_amd import engine as E
    cp = T.make_depth_camera_params(160, 120)
    rig = PlaneRig(E, cp)
    p0 = G.plane_pose(0.0)
    rig.feed(p0)
    rig.integrate(p0)
    rig.feed(G.plane_pose(0.01))
    _, lost = rig.track_rgbd(p0, all_colour_settings(dist_trans=1e-4))
    assert lost and rig.rgbd.state.icp.lost == 1
    W, H = cp.m_imageWidth, cp.m_imageHeight
    rig.sensor.process(np.full((H, W), MINF, np.float32), np.zeros((H, W, 4), np.uint8))
    got, lost = rig.track_rgbd(p0, all_colour_settings())
    assert lost and np.all(got == MINF) and rig.rgbd.state.icp.numCorr == 0 and rig.rgbd.state.icp.lost == 1


REPLAY_PARAMS = """
s_sensorIdx = 8;
s_adapterWidth = 160;
s_adapterHeight = 120;
s_sensorDepthMax = 5.0f;
s_sensorDepthMin = 0.5f;
s_hashNumBuckets = 32768;
s_hashNumSDFBlocks = 16384;
s_hashMaxCollisionLinkedListSize = 7;
s_SDFVoxelSize = 0.01f;
s_SDFMarchingCubeThreshFactor = 10.0f;
s_SDFTruncation = 0.05f;
s_SDFTruncationScale = 0.025f;
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
s_binaryDumpSensorUseTrajectory = false;
"""

REPLAY_TRACKING = TRACKING_DEFAULT.replace(b"s_weightsColor[0] = 0.0f;", b"s_weightsColor[0] = 0.5f;")


@pytest.mark.gpu
def test_gpu_replay_with_rgbd_tracking(vh, oracle_lib, tmp_path):
    """a synthetic `.sens` of the textured plane through tools/replay.py --rgbd-tracking, end to end: every frame
    read, the RGB-D tracker used, a mesh written"""
    import json
    import sys
    from voxelhashing_amd import sensor_data as SD
    cp = T.make_depth_camera_params(160, 120)
    truth = [G.plane_pose(0.012 * k, -0.003 * k) for k in range(8)]
    sd = SD.SensorData.create((160, 120), (160, 120), SD.make_intrinsic_matrix(cp.fx, cp.fy, cp.mx, cp.my), depth_shift=1000.0,
                              sensor_name="synthetic textured plane", depth_type=SD.TYPE_ZLIB_USHORT)
    for k, p in enumerate(truth):
        d, rgbx = G.plane_frame(p, cp)
        sd.addFrame(np.ascontiguousarray(rgbx[..., :3]), np.floor(1000.0 * d.astype(np.float64) + 0.5).astype(np.uint16), p, k, k)
    sens, params, tracking, mesh = (str(tmp_path / n) for n in ("plane.sens", "params.txt", "tracking.txt", "plane.ply"))
    sd.saveToFile(sens)
    open(params, "w").write(REPLAY_PARAMS)
    open(tracking, "wb").write(REPLAY_TRACKING)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "replay.py"), "--params", params, "--tracking", tracking, "--rgbd-tracking", "--sens", sens,
           "--mesh", mesh]
    out = json.loads(subprocess.check_output(cmd, timeout=600).decode().strip().splitlines()[-1])
    assert out["frames"] == len(truth) and out["pose_source"] == "RGB-D ICP", out
    assert out["mesh"]["faces"] > 1000 and os.path.getsize(mesh) > 10000
    # the switch is off by default: the same files without it run the depth-only tracker
    out = json.loads(subprocess.check_output(cmd[:6] + cmd[7:9], timeout=600).decode().strip().splitlines()[-1])
    assert out["frames"] == len(truth) and out["pose_source"] == "projective ICP", out


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(640, 480), (202, 154)])
def test_gpu_rgbd_build_step_on_every_level(vh, oracle_lib, W, H):
    """vh_icp_rgbd_build_linear_system on levels 0, 1, 2 (lane windows 12, 3, 1) of the restatement's pyramids, as applyCT
    builds them: the number of waves against the reference's formula, the per-wave row counts exactly, every one of the
    30 sums within the float32 error bound of its summation.  202x154 gives 101x77 and 50x38: odd widths, and no level
    a whole number of waves.  The identity and a translation-only estimate keep the Euler angles exactly 0, so which
    rows pair up is exact."""
    rgbd_build_step_on_every_level(vh, T.make_depth_camera_params(W, H))


def rgbd_build_step_on_every_level(vh, cp):
    """test_gpu_rgbd_build_step_on_every_level under the camera `cp` (tests/test_gpu_camera_models.py runs it under
    cameras with fx != fy and an off-centre principal point)"""
    from voxelhashing_amd import lib
    from test_camera_tracking import assert_sums_within_float32_bound
    W, H = cp.m_imageWidth, cp.m_imageHeight
    _, _, (i, inn, ic), (m, mn, mc) = plane_maps(cp, 0.0, 0.02)
    pyr = G.pyramids(i, inn, ic, m, mn, mc, 3)
    ts = all_colour_settings()
    up = lambda a: lib.DeviceBuffer.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    for tx in (0.0, 0.006):
        delta = np.eye(4, dtype=np.float32)
        delta[:3, 3] = [tx, 0.5 * tx, 0.0]
        d_state = lib.DeviceBuffer(C.sizeof(T.IcpStateRGBD))
        lib.check(vh.vh_icp_rgbd_begin(d_state.ptr, up(delta).ptr, None))
        for level in range(3):
            pi, pn, pii, pm, pmn, pmiad = pyr[level]
            h, w = pi.shape[:2]
            assert (w, h) == (W >> level, H >> level)
            win = G.window(level)
            assert win == (12, 3, 1)[level]
            nP = vh.vh_icp_rgbd_num_partials(w, h, level)
            # CUDABuildLinearSystemRGBD.cpp:31-35: max(1, 12 / (4 level)) above level 0, ceil(W H / (window 64)) in float
            assert nP == int(np.ceil(np.float32(w * h) / np.float32(win * 64))), (level, nP)
            npx = nP * 64 * win
            p = G.level_params(ts, level, cp)
            prm = T.IcpRGBDParams(fx=p["fx"], fy=p["fy"], mx=p["mx"], my=p["my"], weightDepth=p["weightDepth"], weightColor=p["weightColor"],
                                  distThres=p["distThres"], normalThres=p["normalThres"], sensorMaxDepth=p["sensorMaxDepth"],
                                  colorGradientMin=p["colorGradientMin"], colorThres=p["colorThres"], level=level)
            dterm, cterm, dmask, cmask = G.pixel_terms(pi, pn, pii, pm, pmn, pmiad, np.zeros(3, np.float32), delta[:3, 3].copy(), p)
            # at 50x38 the Gauss-filtered texture is too smooth for colour rows: there the depth rows carry the test
            assert dmask.sum() > 0.3 * w * h and (cmask.sum() > 0.05 * w * h or w * h < 2000), (level, dmask.sum(), cmask.sum())
            # past the image the inputs hold a pixel that pairs up: a kernel reading there would add rows
            k = int(np.nonzero(dmask)[0][0])
            pad = lambda a, c: np.concatenate([a.reshape(-1, c), np.repeat(a.reshape(-1, c)[k:k + 1], npx - w * h, 0)]) if npx > w * h else a.reshape(-1, c)
            bufs = [up(pad(pi, 4)), up(pad(pn, 4)), up(pad(pii, 1)), up(pm), up(pmn), up(pmiad)]
            d_part = lib.DeviceBuffer(nP * 30 * 4)
            lib.check(vh.vh_icp_rgbd_build_linear_system(w, h, d_part.ptr, *[b.ptr for b in bufs], C.byref(prm), d_state.ptr, None))
            part = d_part.download(np.float32, nP * 30).reshape(nP, 30)
            want = G.build_partials(h, w, level, dterm, cterm)
            what = f"{W}x{H} level {level} tx {tx}"
            assert np.array_equal(part[:, 29], want[:, 29]), what
            contrib = dterm.astype(np.float64) + cterm.astype(np.float64)
            sign = np.ones(30)
            sign[21:27] = -1.0  # the kernel subtracts the J^T F products
            want_sum = (contrib * sign).sum(0)
            abs_sum = np.abs(dterm.astype(np.float64)).sum(0) + np.abs(cterm.astype(np.float64)).sum(0)
            import icp_reference as R
            assert_sums_within_float32_bound(R.reduce_partials(part), want_sum, abs_sum, win, nP, what)
