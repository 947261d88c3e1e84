"""The RGB-D tracker inside the native frame loop (engine.Reconstruction.setTrackingRGBD,
Reconstruction.run_native(tracking=True, tracking_rgbd=True)).

A. vh_icp_rgbd_step (one launch per iteration) against vh_icp_rgbd_build_linear_system + vh_icp_rgbd_solve: the whole
   VhIcpStateRGBD, as bytes, after every iteration of the applyCT schedule -- the same arithmetic in the same order, so no
   tolerance; the latches; the publication.
B. The native RGB-D loop against the Python RGB-D loop: poses, scene, ray-cast maps and counts equal; a lost frame;
   resident frames; streaming; misuse; tools/replay.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rgbd_icp as G
from test_gpu_native_tracking import ICP, STREAMING, assert_on_the_true_trajectory, assert_same_raycast, write_sequence
from test_rgbd_tracking import REPLAY_PARAMS, REPLAY_TRACKING, PlaneRig, all_colour_settings
from voxelhashing_amd import canonical, synth, vhtypes as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINF = np.float32(-np.inf)
STATE_BYTES = C.sizeof(T.IcpStateRGBD)


# ---------------------------------------------------------------------------- A. the fused step

class LevelsRGBD:
    """the maps of one RGB-D alignment on the device, on every pyramid level, made with the launchers applyCT uses:
    (w, h, input, input normals, input intensity as the solve reads it, model, model normals, model intensity and
    derivatives), and the buffers both schedules work in"""

    def __init__(self, L, lib, W, H, levels, d_in, d_inn, d_incol, d_model, d_modeln, d_modelcol):
        self.L, self.lib = L, lib
        self.keep = []

        def buf(n):
            b = lib.DeviceBuffer(n)
            self.keep.append(b)
            return b.ptr

        ii, mi, miad = buf(W * H * 4), buf(W * H * 4), buf(W * H * 16)
        lib.check(L.vh_convert_color_to_intensity_float(ii, d_incol, W, H, None))
        lib.check(L.vh_convert_color_to_intensity_float(mi, d_modelcol, W, H, None))
        lib.check(L.vh_compute_intensity_and_derivatives(mi, W, H, miad, None))
        self.lv = [(W, H, d_in, d_inn, ii, d_model, d_modeln, miad)]
        raw = (ii, mi)  # the unfiltered intensities the next level is resampled from
        for i in range(1, levels):
            w0, h0, a, _, _, m, _, _ = self.lv[-1]
            w, h = W >> i, H >> i
            a1, an1, m1, mn1, miad1 = (buf(w * h * 16) for _ in range(5))
            ii1, iif1, mi1, mif1 = (buf(w * h * 4) for _ in range(4))
            lib.check(L.vh_resample_float4_map(a1, w, h, a, w0, h0, None))
            lib.check(L.vh_compute_normals(an1, a1, w, h, None))
            lib.check(L.vh_resample_float_map(ii1, w, h, raw[0], w0, h0, None))
            lib.check(L.vh_gauss_filter_float_map(iif1, ii1, 3.0, 1.0, w, h, None))
            lib.check(L.vh_resample_float4_map(m1, w, h, m, w0, h0, None))
            lib.check(L.vh_compute_normals(mn1, m1, w, h, None))
            lib.check(L.vh_resample_float_map(mi1, w, h, raw[1], w0, h0, None))
            lib.check(L.vh_gauss_filter_float_map(mif1, mi1, 3.0, 1.0, w, h, None))
            lib.check(L.vh_compute_intensity_and_derivatives(mif1, w, h, miad1, None))
            self.lv.append((w, h, a1, an1, iif1, m1, mn1, miad1))
            raw = (ii1, mi1)
        n_part = max(L.vh_icp_rgbd_num_partials(w, h, i) for i, (w, h, *_) in enumerate(self.lv))
        self.part = lib.DeviceBuffer(n_part * 30 * 4)
        self.state = lib.DeviceBuffer(STATE_BYTES)
        self.ticket = lib.DeviceBuffer(4)
        self.result = lib.DeviceBuffer(C.sizeof(T.IcpResult))
        lib.check(L.vh_memset(self.ticket.ptr, 0xff, 4, None))  # not zero by luck: every run clears it where it begins

    def params(self, ts, level, cp):
        p = G.level_params(ts, level, cp)
        return T.IcpRGBDParams(fx=p["fx"], fy=p["fy"], mx=p["mx"], my=p["my"], weightDepth=p["weightDepth"], weightColor=p["weightColor"],
                               distThres=p["distThres"], normalThres=p["normalThres"], sensorMaxDepth=p["sensorMaxDepth"],
                               colorGradientMin=p["colorGradientMin"], colorThres=p["colorThres"], level=level)

    def run(self, cp, ts, delta, fused, model=None, publish_tag=None):
        """the schedule of applyCT -> [(level, iteration, state bytes)] after every iteration.  publish_tag: the last step
        of level 0 publishes into self.result under it (fused only)."""
        L, lib = self.L, self.lib
        d_delta = lib.DeviceBuffer.from_numpy(np.ascontiguousarray(delta, dtype=np.float32))
        lib.check(L.vh_memset(self.state.ptr, 0, STATE_BYTES, None))
        lib.check(L.vh_memset(self.ticket.ptr, 0, 4, None))
        lib.check(L.vh_memset(self.result.ptr, 0, C.sizeof(T.IcpResult), None))
        lib.check(L.vh_icp_rgbd_begin(self.state.ptr, d_delta.ptr, None))
        b = ts.base
        out = []
        for level in reversed(range(b.s_maxLevels)):
            w, h, a, an, ai, m, mn, miad = self.lv[level]
            if model is not None:
                m, mn, miad = model[level]
            prm = self.params(ts, level, cp)
            lib.check(L.vh_icp_begin_level(self.state.ptr, None))  # (&state->icp: the first member)
            for it in range(b.s_maxOuterIter[level]):
                if fused:
                    last = publish_tag is not None and level == 0 and it + 1 == b.s_maxOuterIter[0]
                    lib.check(L.vh_icp_rgbd_step(w, h, self.part.ptr, self.ticket.ptr, a, an, ai, m, mn, miad, C.byref(prm), self.state.ptr,
                                                 b.s_angleTransThres[level], b.s_distTransThres[level], b.s_residualEarlyOut[level],
                                                 self.result.ptr if last else None, publish_tag if last else 0, None), "vh_icp_rgbd_step")
                else:
                    lib.check(L.vh_icp_rgbd_build_linear_system(w, h, self.part.ptr, a, an, ai, m, mn, miad, C.byref(prm), self.state.ptr, None))
                    lib.check(L.vh_icp_rgbd_solve(self.state.ptr, self.part.ptr, L.vh_icp_rgbd_num_partials(w, h, level), b.s_angleTransThres[level],
                                                  b.s_distTransThres[level], b.s_residualEarlyOut[level], None))
                out.append((level, it, self.state.download(np.uint8).tobytes()))
        if fused:
            assert self.ticket.download(np.uint32)[0] == 0, "the last arriver left the ticket counter dirty"
        return out

    def published(self):
        return T.IcpResult.from_buffer_copy(self.result.download(np.uint8).tobytes())


def describe(b):
    s = T.IcpStateRGBD.from_buffer_copy(b)
    out = {k: (list(getattr(s.icp, k)) if k in ("delta", "pad") else getattr(s.icp, k)) for k, _ in T.IcpState._fields_}
    out.update(angles=list(s.angles), translation=list(s.translation), pad2=list(s.pad))
    return out


def assert_same_states(got, want, what):
    assert len(got) == len(want)
    for (level, it, g), (_, _, w) in zip(got, want):
        if g != w:
            dg, dw = describe(g), describe(w)
            diff = {k: (dg[k], dw[k]) for k in dg if dg[k] != dw[k]}
            raise AssertionError(f"{what}: level {level} iteration {it}: fused vs two kernels differ in {diff}")


@pytest.mark.parametrize("W,H", [(160, 120), (640, 480), (202, 154)])
def test_fused_rgbd_step_equals_two_kernels_bit_for_bit(vh, oracle_lib, W, H):
    from voxelhashing_amd import engine as E, lib
    L = lib.load()
    cp = T.make_depth_camera_params(W, H)
    rig = PlaneRig(E, cp)
    at = G.plane_pose(0.01)
    for _ in range(6):  # (the model's colours: see apply_ct_equals_restatement)
        rig.feed(at)
        rig.integrate(at)
    rig.feed(G.plane_pose(0.035))
    rd = rig.render(at)
    a, b, col = rig.maps()
    lv = LevelsRGBD(L, lib, W, H, 3, a.value, b.value, col, rd.d_depth4, rd.d_normals, rd.d_colors)
    eye = np.eye(4, dtype=np.float32)
    state = lambda raw: T.IcpStateRGBD.from_buffer_copy(raw)

    def two_kernels(ts, delta, model=None):
        return lv.run(cp, ts, delta, False, model)

    def both(ts, delta, what, model=None, want=None):
        want = want if want is not None else two_kernels(ts, delta, model)
        got = lv.run(cp, ts, delta, True, model)
        assert_same_states(got, want, what)
        again = lv.run(cp, ts, delta, True, model)
        assert [s for _, _, s in again] == [s for _, _, s in got], f"{what}: the fused schedule is not repeatable"
        return [state(s) for _, _, s in got], [s for _, _, s in got]

    # 1. a colour weight on every level, identity estimate: tracks
    ts = all_colour_settings()
    want_colour = two_kernels(ts, eye)
    states, _ = both(ts, eye, "colour on every level", want=want_colour)
    assert len(states) == 18 and not states[-1].icp.lost and states[-1].icp.numCorr > 0
    print(f"{W}x{H}: {states[-1].icp.iterations} systems, {states[-1].icp.numCorr} rows on level 0")

    # 2. the far Euler branch: the estimate's angles sit near +-pi
    far = np.asarray(G.plane_pose(0.006, 0.002, rz_deg=-0.4), np.float32).reshape(4, 4)
    want_far = two_kernels(ts, far)
    first = state(want_far[0][2])
    assert first.icp.iterations == 1  # (the first step ran: what follows is a linearisation point it computed)
    states, _ = both(ts, far, "far Euler branch", want=want_far)
    assert not states[-1].icp.lost and states[-1].icp.numCorr > 0

    # 3. the photometric rows are in the sums: without them the two-kernel states differ, by the first step of level 1 at the latest
    ts_depth = all_colour_settings()
    for i in range(3):
        ts_depth.s_weightsColor[i] = 0.0
    want_depth = two_kernels(ts_depth, eye)
    differs = [k for k, ((_, _, x), (_, _, y)) in enumerate(zip(want_depth, want_colour)) if x != y]
    assert differs and differs[0] <= 4, differs  # (iterations 0-3 are level 2, 4 is the first of level 1)
    both(ts_depth, eye, "no colour weight", want=want_depth)

    # 4. latches.  Early-out: every level done after its first step, its other steps leave the bytes untouched
    ts_done = all_colour_settings(early_out=1e9)
    states, raw = both(ts_done, eye, "early-out")
    k = 0
    for level in (2, 1, 0):
        n = ts_done.base.s_maxOuterIter[level]
        assert states[k].icp.done == 1 and not states[k].icp.lost
        assert all(raw[k + j] == raw[k] for j in range(1, n)), level
        k += n
    assert states[-1].icp.iterations == 3
    # a model of -inf on every level: lost with the first step, nothing changes afterwards
    empty = []
    for w, h, *_ in lv.lv:
        e = lib.DeviceBuffer.from_numpy(np.full((h, w, 4), MINF, dtype=np.float32))
        lv.keep.append(e)
        empty.append((e.ptr, e.ptr, e.ptr))
    states, raw = both(ts, eye, "empty model", empty)
    assert states[0].icp.lost == 1 and states[0].icp.numCorr == 0 and states[0].icp.iterations == 1
    assert all(r == raw[0] for r in raw)
    # a step beyond the rigidity thresholds: lost with rows in the system, nothing changes afterwards.  (Not asked of the
    # very first step: level 2 may hold no photometric row, and the plane's depth rows do not see the in-plane motion.)
    states, raw = both(all_colour_settings(dist_trans=1e-4), eye, "rigidity check")
    lost = [k for k, s in enumerate(states) if s.icp.lost]
    assert lost and states[lost[0]].icp.numCorr > 0 and all(r == raw[lost[0]] for r in raw[lost[0]:]), lost[:1]
    print(f"{W}x{H}: the rigidity check fails at step {lost[0]}")

    # 5. publication by the last step: one that works, and ones that are skipped (done; lost)
    def published(ts, delta, tag, model=None):
        got = lv.run(cp, ts, delta, True, model, publish_tag=tag)
        final, res = state(got[-1][2]).icp, lv.published()
        assert res.tag == tag
        assert list(res.delta) == list(final.delta) and res.lost == final.lost and res.numCorr == final.numCorr and res.iterations == final.iterations
        assert (res.sumRegError, res.sumRegWeight, res.matrixCondition) == (final.sumRegError, final.sumRegWeight, final.matrixCondition)
        return got, final

    got, final = published(ts, eye, 0x1234)
    assert [s for _, _, s in got] == [s for _, _, s in want_colour]  # publishing changes nothing in the state
    assert not final.lost
    _, final = published(ts_done, eye, 7)
    assert final.done == 1 and final.iterations == 3      # the last step of level 0 was a skipped one
    _, final = published(ts, eye, 0xfffffffe, empty)
    assert final.lost == 1 and final.iterations == 1


@pytest.mark.parametrize("axis", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (3, 1, 2), (1, 3, 2), (1, 2, 3), (-3, 1, 2), (1, -3, -2), (-1, 2, -3)])
@pytest.mark.parametrize("angle", [2.3, 2.8, 3.1])
def test_rigidity_angle_of_a_rotation_beyond_120_degrees(vh, axis, angle):
    """angle_axis_angle's branch for a rotation whose trace is not positive (Shoemake's construction from the largest
    diagonal entry, each of the three; the quaternion's w of either sign): a state whose delta is such a rotation, a
    system whose solution is zero, and the level's angle threshold a little above and a little below what the
    restatement (tests/rgbd_icp.py) gives for the delta the step arrives at.  float32 rounding of the sines, cosines and
    the arc cosine is some 1e-6 here; the margin is 1e-3 rad."""
    from test_icp_solve import Solver, terms_of
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)  # Rodrigues
    assert np.trace(R) <= 0
    delta = np.eye(4, dtype=np.float32)
    delta[:3, :3] = R.astype(np.float32)
    arrived = G.delinearize(G.euler_angles_zyx(delta[:3, :3])).reshape(3, 3)  # x = anglesOld + 0
    assert np.abs(arrived - delta[:3, :3]).max() < 1e-5
    want = float(G.angle_axis_angle(arrived))
    assert min(abs(want - angle), abs(want - (2 * np.pi - angle))) < 1e-4, (want, angle)
    system = terms_of(np.eye(6), np.zeros(6))
    above = Solver(vh, True, delta).solve(system, angle=want + 1e-3, dist=1.0)
    assert not above.lost and above.iterations == 1, (axis, angle, want)
    below = Solver(vh, True, delta).solve(system, angle=want - 1e-3, dist=1.0)
    assert below.lost == 1 and below.iterations == 1, (axis, angle, want)


# ---------------------------------------------------------------------------- B. the loop

def write_plane_sequence(tmp_path):
    """the 8-frame textured-plane `.sens`, parameter file and tracking file of test_gpu_replay_with_rgbd_tracking"""
    from voxelhashing_amd import sensor_data as SD
    cp = T.make_depth_camera_params(160, 120)
    truth = [G.plane_pose(0.012 * k, -0.003 * k) for k in range(8)]
    sd = SD.SensorData.create((160, 120), (160, 120), SD.make_intrinsic_matrix(cp.fx, cp.fy, cp.mx, cp.my), depth_shift=1000.0,
                              sensor_name="synthetic textured plane", depth_type=SD.TYPE_ZLIB_USHORT)
    for k, p in enumerate(truth):
        d, rgbx = G.plane_frame(p, cp)
        sd.addFrame(np.ascontiguousarray(rgbx[..., :3]), np.floor(1000.0 * d.astype(np.float64) + 0.5).astype(np.uint16), p, k, k)
    sens, params, tracking = (str(tmp_path / n) for n in ("plane.sens", "params.txt", "tracking.txt"))
    sd.saveToFile(sens)
    open(params, "w").write(REPLAY_PARAMS)
    open(tracking, "wb").write(REPLAY_TRACKING)
    return truth, sens, params, tracking


def assert_same_run(nat, py, n, what):
    """poses (getPoses() and trajectory), lost frames, scene, the last ray cast"""
    nat.native.synchronize()
    got = nat.native.getPoses()
    assert len(got) == n
    assert nat.lost_frames == py.lost_frames and len(nat.trajectory) == len(py.trajectory) == n - py.lost_frames
    for k, (a, b) in enumerate(zip(nat.trajectory, py.trajectory)):
        assert np.array_equal(a, b), (what, k)
    assert np.array_equal(np.stack([p for p in got if p[0, 0] != MINF]), np.stack(py.trajectory)), what
    canonical.assert_same_scene(nat.scene.state(), py.scene.state(), what)
    assert_same_raycast(nat.ray, py.ray, what + ": last ray cast")
    st = nat.native.getStats()
    assert st["lostFrames"] == py.lost_frames and st["trackedFrames"] == n - 1 - py.lost_frames and st["frames"] == n - py.lost_frames
    return got


def test_native_rgbd_loop_equals_python_loop_on_the_textured_plane(vh, oracle_lib, tmp_path):
    from voxelhashing_amd import reconstruction as R
    truth, sens, params, tracking = write_plane_sequence(tmp_path)
    n = len(truth)
    make = lambda rgbd: R.Reconstruction(R.read_app_state(params), R.read_tracking_state_rgbd(tracking) if rgbd else R.read_tracking_state(tracking),
                                         [sens], use_rgbd_tracking=rgbd)
    py = make(True)
    want = []
    for _ in range(n):
        want.append(py.frame())
    assert py.frame() is None
    print("Python RGB-D loop: lost frames", [k for k in range(n) if want[k][0, 0] == MINF])
    nat = make(True)
    with pytest.raises(ValueError, match="RGB-D"):
        nat.run_native(tracking=True, batch=4)  # as before without tracking_rgbd=True
    assert nat.run_native(tracking=True, tracking_rgbd=True, batch=4) == n
    got = assert_same_run(nat, py, n, "native RGB-D loop vs Python RGB-D loop, textured plane")
    for k in range(n):  # a frame the Python loop lost is lost here too, all -inf
        assert np.array_equal(got[k], want[k]), k
    # the switch does something: the plain tracker inside the native loop gives other poses on the same file
    plain = make(False)
    assert plain.run_native(tracking=True, batch=4) == n
    plain.native.synchronize()
    other = plain.native.getPoses()
    assert any(not np.array_equal(other[k], got[k]) for k in range(n))


def test_native_rgbd_loop_equals_python_loop_on_s3(vh, oracle_lib, tmp_path):
    import test_reconstruction as TR
    from voxelhashing_amd import reconstruction as R
    path = str(tmp_path / "s3.sens")
    poses, _ = TR.make_sequence(path, oracle_lib)
    py = R.Reconstruction(TR.app_state(ICP), sens_files=[path], use_rgbd_tracking=True)
    assert bytes(py.tracking_rgbd) == bytes(T.make_tracking_state_rgbd())
    assert py.run() == TR.N
    # the conditions of this test, asked of the Python loop alone first
    assert py.lost_frames == 0
    f5 = R.Reconstruction(TR.app_state(ICP), sens_files=[path])
    assert f5.run() == TR.N and f5.lost_frames == 0
    assert any(not np.array_equal(a, b) for a, b in zip(py.trajectory, f5.trajectory)), "the RGB-D tracker gives the plain tracker's poses here"
    nat = R.Reconstruction(TR.app_state(ICP), sens_files=[path], use_rgbd_tracking=True)
    assert nat.run_native(tracking=True, tracking_rgbd=True, batch=4) == TR.N
    assert_same_run(nat, py, TR.N, "native RGB-D loop vs Python RGB-D loop, S3")
    assert np.array_equal(py.trajectory[0], np.eye(4, dtype=np.float32))
    assert_on_the_true_trajectory(nat.trajectory, poses, range(1, TR.N))


def test_native_rgbd_loop_on_resident_float_frames(vh, oracle_lib, tmp_path):
    """through run(): device copies of the depth and colour maps CUDARGBDSensor handed the Python loop"""
    import test_reconstruction as TR
    from voxelhashing_amd import engine as E, lib, reconstruction as R
    path = str(tmp_path / "s3.sens")
    TR.make_sequence(path, oracle_lib)
    py = R.Reconstruction(TR.app_state(ICP), sens_files=[path], use_rgbd_tracking=True)
    want, depth, color = [], [], []
    for k in range(TR.N):
        want.append(py.frame())
        maps = py.sensor.download()
        depth.append(lib.DeviceBuffer.from_numpy(np.ascontiguousarray(maps["depth"], dtype=np.float32)))
        color.append(lib.DeviceBuffer.from_numpy(np.ascontiguousarray(maps["color"], dtype=np.float32)))
    assert py.lost_frames == 0
    other = R.Reconstruction(TR.app_state(ICP), sens_files=[path], use_rgbd_tracking=True)  # a second scene and ray caster with the same parameters
    loop = E.Reconstruction(other.scene, other.ray, None, other.cp, E.Reconstruction.defaultOptions(s_offlineProcessing=1))
    loop.setTrackingRGBD(other.tracking_rgbd)
    frames = E.Reconstruction.makeFrames([np.full(16, 7.0, np.float32)] * TR.N, [d.ptr for d in depth], [c.ptr for c in color])  # (the poses are ignored)
    loop.run(frames)
    loop.synchronize()
    got = loop.getPoses()
    for k in range(TR.N):
        assert np.array_equal(got[k], want[k]), k
    canonical.assert_same_scene(other.scene.state(), py.scene.state(), "resident float frames")
    assert_same_raycast(other.ray, py.ray, "last ray cast, resident float frames")
    st = loop.getStats()
    assert st["trackedFrames"] == TR.N - 1 and st["lostFrames"] == 0
    # a frame without a colour map is refused
    bare = E.Reconstruction.makeFrames([np.eye(4, dtype=np.float32)], [depth[0].ptr], None)
    with pytest.raises(lib.VhError) as e:
        loop.run(bare)
    assert e.value.code == 4


def test_rgbd_lost_frame_is_skipped_and_tracking_goes_on(vh, oracle_lib, tmp_path):
    import test_reconstruction as TR
    from voxelhashing_amd import reconstruction as R
    path = str(tmp_path / "s3_blank5.sens")
    poses = write_sequence(path, oracle_lib, TR.W, TR.H, TR.N, blank=5)
    py = R.Reconstruction(TR.app_state(ICP), sens_files=[path], use_rgbd_tracking=True)
    want = [py.frame() for _ in range(TR.N)]
    lost = [k for k in range(TR.N) if want[k][0, 0] == MINF]
    # the condition of this test, asked of the Python loop alone first: exactly one lost frame, frame 5
    assert lost == [5] and py.lost_frames == 1 and np.all(want[5] == MINF), lost
    nat = R.Reconstruction(TR.app_state(ICP), sens_files=[path], use_rgbd_tracking=True)
    assert nat.run_native(tracking=True, tracking_rgbd=True, batch=4) == TR.N
    got = assert_same_run(nat, py, TR.N, "RGB-D, sequence with a lost frame")
    assert np.all(got[5] == MINF)
    for k in range(TR.N):
        assert np.array_equal(got[k], want[k]), k
    st = nat.native.getStats()
    assert st["lostFrames"] == 1 and st["trackedFrames"] == TR.N - 2 and st["frames"] == TR.N - 1


def test_rgbd_tracking_with_streaming(vh, oracle_lib, tmp_path):
    """as test_tracking_with_streaming: no bit equality with the Python loop (different stream-in entry points)"""
    import test_reconstruction as TR
    from voxelhashing_amd import reconstruction as R
    path = str(tmp_path / "s3.sens")
    TR.make_sequence(path, oracle_lib)
    nat = R.Reconstruction(TR.app_state(STREAMING + ICP), sens_files=[path], use_rgbd_tracking=True)
    assert nat.run_native(tracking=True, tracking_rgbd=True, batch=4) == TR.N
    nat.native.synchronize()
    nat.chunk_grid.debugCheckForDuplicates()
    assert nat.scene.debugHash()["duplicates"] == 0
    st = nat.native.getStats()
    assert st["trackedFrames"] + st["lostFrames"] == TR.N - 1
    assert nat.chunk_grid.getStatistics()["blocks"] > 0 and nat.scene.state()["num_occupied"] > 100


def test_rgbd_misuse_is_refused_and_the_default_is_left_alone(vh, oracle_lib, tmp_path):
    import test_reconstruction as TR
    from test_camera_tracking import setup_small
    from voxelhashing_amd import engine as E, lib, reconstruction as R
    L = lib.load()
    assert L.vh_icp_rgbd_step(160, 120, None, None, None, None, None, None, None, None, None, None, 1.0, 1.0, 0.01, None, 0, None) == 4
    hp, cp, rp = setup_small()
    ts, plain = T.make_tracking_state_rgbd(), T.make_tracking_state()

    def refused(call, *args):
        with pytest.raises(lib.VhError) as e:
            call(*args)
        assert e.value.code == 4, e.value

    scene, ray = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=True, gc=False)), E.CUDARayCastSDF(rp)
    refused(E.Reconstruction(scene, None, None, cp, E.Reconstruction.defaultOptions(s_renderEnabled=0)).setTrackingRGBD, ts)   # no ray caster
    refused(E.Reconstruction(scene, ray, None, cp, E.Reconstruction.defaultOptions(s_renderEnabled=0)).setTrackingRGBD, ts)    # never ray-casts
    loop = E.Reconstruction(scene, ray, None, cp)
    refused(loop.setTrackingRGBD, T.make_tracking_state_rgbd(levels=0, weights_depth=(), weights_color=(), outer=(), inner=()))
    refused(loop.setTrackingRGBD, T.make_tracking_state_rgbd(levels=8, weights_depth=(1.0,) * 8, weights_color=(0.5,) * 8, outer=(1,) * 8, inner=(1,) * 8))
    # one of the two trackers, once
    a = E.Reconstruction(scene, ray, None, cp)
    a.setTracking(plain)
    refused(a.setTrackingRGBD, ts)
    b = E.Reconstruction(scene, ray, None, cp)
    b.setTrackingRGBD(ts)
    refused(b.setTracking, plain)
    refused(b.setTrackingRGBD, ts)
    # a raw format without colour, whichever call comes second
    refused(b.setRawFormat, (160, 120), None, 1000.0, 0)
    c = E.Reconstruction(scene, ray, None, cp)
    c.setRawFormat((160, 120), None, 1000.0, 0)
    refused(c.setTrackingRGBD, ts)
    frame = E.synth_frame(synth.S3_SPHERES, 0, synth.orbit_pose(0, 400), cp)
    seq = E.Reconstruction.makeFrames([synth.orbit_pose(0, 400)], [frame.depth_ptr], [frame.color_ptr])
    loop.run(seq)
    loop.synchronize()
    refused(loop.setTrackingRGBD, ts)  # after a frame
    assert loop.getStats()["trackedFrames"] == 0 and loop.getStats()["lostFrames"] == 0

    # a loop whose setTrackingRGBD was refused plays the recorded poses as it always did
    path = str(tmp_path / "s3.sens")
    poses, _ = TR.make_sequence(path, oracle_lib)
    recorded = "s_binaryDumpSensorUseTrajectory = true;\ns_binaryDumpSensorUseTrajectoryOnlyInit = false;\n"
    py = R.Reconstruction(TR.app_state(recorded), sens_files=[path])
    assert py.run() == TR.N
    nat = R.Reconstruction(TR.app_state(recorded), sens_files=[path])
    nat.prepare_native(batch=4)
    refused(nat.native.setTrackingRGBD, T.make_tracking_state_rgbd(levels=0, weights_depth=(), weights_color=(), outer=(), inner=()))
    assert nat.run_native(batch=4) == TR.N
    nat.native.synchronize()
    got = nat.native.getPoses()
    for k in range(TR.N):
        assert np.array_equal(got[k], np.asarray(poses[k], np.float32).reshape(4, 4)) and np.array_equal(nat.trajectory[k], py.trajectory[k]), k
    canonical.assert_same_scene(nat.scene.state(), py.scene.state(), "untracked native loop vs Python loop")
    st = nat.native.getStats()
    assert st["trackedFrames"] == 0 and st["lostFrames"] == 0 and st["frames"] == TR.N


def test_replay_tool_with_native_rgbd_tracking(vh, oracle_lib, tmp_path):
    truth, sens, params, tracking = write_plane_sequence(tmp_path)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "replay.py"), "--params", params, "--tracking", tracking, "--rgbd-tracking", "--sens", sens,
           "--native", "--native-tracking", "--batch", "4"]
    out = json.loads(subprocess.check_output(cmd, timeout=600).decode().strip().splitlines()[-1])
    assert out["frames"] == len(truth) and out["pose_source"] == "RGB-D ICP" and out["loop"] == "native", out
    assert out["trackedFrames"] + out["lostFrames"] == len(truth) - 1, out
