"""Camera tracking inside the native frame loop (engine.Reconstruction.setTracking, Reconstruction.run_native(tracking=True)).

1. vh_icp_step (one launch per ICP iteration) against the three kernels it replaces: the whole VhIcpState, as bytes, after
   every iteration of the default schedule -- it is the same arithmetic in the same order, so no tolerance.
2. The native tracked loop against the Python loop (reconstruction.Reconstruction.run with
   s_binaryDumpSensorUseTrajectory = false): poses, scene and ray-cast maps equal, then the accuracy bounds
   tests/test_reconstruction.py uses for the sequence.
3. A frame without a measurement: lost, not integrated, the loop goes on.
4. Tracking with streaming.
5. Misuse, and a loop whose setTracking was refused plays recorded poses as before."""
import ctypes as C

import numpy as np
import pytest

from voxelhashing_amd import canonical, synth, vhtypes as T

pytestmark = pytest.mark.gpu

MINF = np.float32(-np.inf)
STATE_BYTES = C.sizeof(T.IcpState)


# ---------------------------------------------------------------------------- 1. the fused step

class Levels:
    """the maps of one alignment on the device: input and model, positions and normals, on every pyramid level (made with
    the launchers applyCT uses), and the buffers both schedules work in"""

    def __init__(self, L, lib, W, H, levels, d_in, d_inn, d_model, d_modeln):
        self.L, self.lib = L, lib
        self.keep = []
        self.lv = [(W, H, d_in, d_inn, d_model, d_modeln)]
        for i in range(1, levels):
            w0, h0, a, _, m, _ = self.lv[-1]
            w, h = W >> i, H >> i
            bufs = [lib.DeviceBuffer(w * h * 16) for _ in range(4)]
            self.keep += bufs
            lib.check(L.vh_resample_float4_map(bufs[0].ptr, w, h, a, w0, h0, None))
            lib.check(L.vh_compute_normals(bufs[1].ptr, bufs[0].ptr, w, h, None))
            lib.check(L.vh_resample_float4_map(bufs[2].ptr, w, h, m, w0, h0, None))
            lib.check(L.vh_compute_normals(bufs[3].ptr, bufs[2].ptr, w, h, None))
            self.lv.append((w, h, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr))
        self.corr, self.corrn = lib.DeviceBuffer(W * H * 16), lib.DeviceBuffer(W * H * 16)
        self.part = lib.DeviceBuffer(L.vh_icp_num_partials(W, H) * 30 * 4)
        self.state = lib.DeviceBuffer(STATE_BYTES)
        self.ticket = lib.DeviceBuffer(4)
        lib.check(L.vh_memset(self.ticket.ptr, 0xff, 4, None))  # not zero by luck: every run clears it where it begins

    def run(self, cp, ts, delta, fused, model=None):
        """the schedule of applyCT -> [(level, iteration, state bytes)] after every iteration"""
        L, lib = self.L, self.lib
        d_delta = lib.DeviceBuffer.from_numpy(np.ascontiguousarray(delta, dtype=np.float32))
        lib.check(L.vh_memset(self.state.ptr, 0, STATE_BYTES, None))
        lib.check(L.vh_memset(self.ticket.ptr, 0, 4, None))
        lib.check(L.vh_icp_begin(self.state.ptr, d_delta.ptr, None))
        out = []
        for level in reversed(range(ts.s_maxLevels)):
            w, h, a, an, m, mn = self.lv[level]
            if model is not None:
                m, mn = model[level]
            lib.check(L.vh_icp_begin_level(self.state.ptr, None))
            for it in range(ts.s_maxOuterIter[level]):
                assert ts.s_maxInnerIter[level] == 1
                if fused:
                    lib.check(L.vh_icp_step(a, an, m, mn, w, h, ts.s_distThres[level], ts.s_normalThres[level], float(2 ** level), C.byref(cp),
                                            self.part.ptr, self.ticket.ptr, self.state.ptr, ts.s_angleTransThres[level], ts.s_distTransThres[level],
                                            ts.s_residualEarlyOut[level], None, 0, None), "vh_icp_step")
                else:
                    lib.check(L.vh_icp_projective_correspondences(a, an, m, mn, self.corr.ptr, self.corrn.ptr, w, h, ts.s_distThres[level],
                                                                  ts.s_normalThres[level], float(2 ** level), self.state.ptr, C.byref(cp), None))
                    lib.check(L.vh_icp_build_linear_system(w, h, self.part.ptr, a, self.corr.ptr, self.corrn.ptr, self.state.ptr, None))
                    lib.check(L.vh_icp_solve(self.state.ptr, self.part.ptr, L.vh_icp_num_partials(w, h), ts.s_angleTransThres[level],
                                             ts.s_distTransThres[level], ts.s_residualEarlyOut[level], 1, None))
                out.append((level, it, self.state.download(np.uint8).tobytes()))
        assert self.ticket.download(np.uint32)[0] == 0 or not fused, "the last arriver left the ticket counter dirty"
        return out


def describe(b):
    s = T.IcpState.from_buffer_copy(b)
    return {k: (list(getattr(s, k)) if k in ("delta", "pad") else getattr(s, k)) for k, _ in T.IcpState._fields_}


def assert_same_states(got, want, what):
    assert len(got) == len(want)
    for (level, it, g), (_, _, w) in zip(got, want):
        if g != w:
            dg, dw = describe(g), describe(w)
            diff = {k: (dg[k], dw[k]) for k in dg if dg[k] != dw[k]}
            raise AssertionError(f"{what}: level {level} iteration {it}: fused vs three kernels differ in {diff}")


@pytest.mark.parametrize("W,H", [(160, 120), (640, 480), (100, 76)])
def test_fused_step_equals_three_kernels_bit_for_bit(vh, oracle_lib, W, H):
    from test_camera_tracking import GpuRig, TRACK_SPHERES, setup_small
    from voxelhashing_amd import engine as E, lib
    O, L = oracle_lib, lib.load()
    hp, cp, rp = setup_small(W, H)
    poses = [synth.orbit_pose(k, n_frames=400) for k in range(2)]
    rig = GpuRig(E, hp, cp, rp)
    rig.feed(O, TRACK_SPHERES, poses[0])
    rig.integrate(poses[0])
    rig.feed(O, TRACK_SPHERES, poses[1])
    rig.ray.render(rig.scene.getHashData(), rig.scene.getHashParams(), cp, poses[0])
    rd = rig.ray.getRayCastData()
    a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
    lib.check(L.vh_rgbd_sensor_get_maps(rig.sensor.handle, C.byref(a), C.byref(b), C.byref(c)), "maps")
    lv = Levels(L, lib, W, H, 3, a.value, b.value, rd.d_depth4, rd.d_normals)
    eye = np.eye(4, dtype=np.float32)

    def both(ts, delta, what, model=None):
        want = lv.run(cp, ts, delta, False, model)
        got = lv.run(cp, ts, delta, True, model)
        assert_same_states(got, want, what)
        again = lv.run(cp, ts, delta, True, model)
        assert [s for _, _, s in again] == [s for _, _, s in got], f"{what}: the fused schedule is not repeatable"
        return [T.IcpState.from_buffer_copy(s) for _, _, s in got], [s for _, _, s in got]

    # the default schedule: tracks
    ts = T.make_tracking_state()
    states, _ = both(ts, eye, "default schedule")
    assert len(states) == 18 and not states[-1].lost and states[-1].numCorr > 0
    assert states[-1].iterations >= 3

    # a level that reaches its early-out: done latches, the level's other steps leave the state untouched
    ts_done = T.make_tracking_state(early_out=1e9)
    states, raw = both(ts_done, eye, "early-out")
    at = 0
    for level in (2, 1, 0):
        n = ts_done.s_maxOuterIter[level]
        assert states[at].done == 1 and not states[at].lost
        assert all(raw[at + k] == raw[at] for k in range(1, n)), level
        at += n
    assert states[-1].iterations == 3

    # an empty model: no pair, ATA.isZero() -> lost latches with the first step, nothing changes afterwards
    empty = []
    for w, h, *_ in lv.lv:
        e = lib.DeviceBuffer.from_numpy(np.full((h, w, 4), MINF, dtype=np.float32))
        lv.keep.append(e)
        empty.append((e.ptr, e.ptr))
    states, raw = both(ts, eye, "empty model", empty)
    assert states[0].lost == 1 and states[0].numCorr == 0 and states[0].iterations == 1
    assert all(r == raw[0] for r in raw)

    # a model moved out of reach (no pair within the distance threshold), and a step beyond the rigidity thresholds
    far = eye.copy()
    far[0, 3] = 3.0
    states, raw = both(ts, far, "model out of reach")
    assert states[0].lost == 1 and all(r == raw[0] for r in raw)
    states, raw = both(T.make_tracking_state(dist_trans=1e-4), eye, "rigidity check")
    assert states[0].lost == 1 and states[0].numCorr > 0 and all(r == raw[0] for r in raw)


# ---------------------------------------------------------------------------- 2.-5. the loop

def write_sequence(path, O, w, h, n, blank=None):
    """tests/test_reconstruction.py's make_sequence at any size; frame `blank` holds no measurement (depth 0 everywhere)"""
    from voxelhashing_amd import sensor_data as SD
    cp = T.make_depth_camera_params(w, h)
    intr = SD.make_intrinsic_matrix(cp.fx, cp.fy, cp.mx, cp.my)
    sd = SD.SensorData.create((w, h), (w, h), intr, depth_shift=1000.0, sensor_name="synthetic S3", depth_type=SD.TYPE_ZLIB_USHORT)
    poses = [synth.orbit_pose(k, n_frames=400) for k in range(n)]
    for k, p in enumerate(poses):
        d, c = O.synth_frame(synth.S3_SPHERES, 0, p, cp)
        mm = np.where(np.isfinite(d), np.floor(1000.0 * d.astype(np.float64) + 0.5), 0).astype(np.uint16)
        if k == blank:
            mm[:] = 0
        rgb = np.clip(np.where(np.isfinite(c[..., :3]), c[..., :3], 0) * 255.0, 0, 255).astype(np.uint8)
        sd.addFrame(rgb, mm, p, 100 + k, 200 + k)
    sd.saveToFile(path)
    return poses


ICP = "s_binaryDumpSensorUseTrajectory = false;\n"


def assert_on_the_true_trajectory(trajectory, poses, frames):
    """the bounds of test_tracked_replay_recording_and_second_generation: without a trajectory the world frame is the first
    camera frame, so compare with inv(T0) * Tk"""
    t0_inv = np.linalg.inv(np.asarray(poses[0], np.float64).reshape(4, 4))
    for k in frames:
        rel = np.linalg.inv(trajectory[k].astype(np.float64)) @ (t0_inv @ np.asarray(poses[k], np.float64).reshape(4, 4))
        ang = np.degrees(np.arccos(np.clip(0.5 * (np.trace(rel[:3, :3]) - 1.0), -1, 1)))
        print(f"frame {k}: {np.linalg.norm(rel[:3, 3]):.5f} m, {ang:.4f} deg")
        assert np.linalg.norm(rel[:3, 3]) < 0.006 and ang < 0.15, (k, np.linalg.norm(rel[:3, 3]), ang)


def assert_same_raycast(a, b, what):
    got, want = a.download(), b.download()
    for m in ("depth", "depth4", "normals", "colors"):
        assert got[m].tobytes() == want[m].tobytes(), (what, m)


def test_native_tracked_loop_equals_python_loop(vh, oracle_lib, tmp_path):
    import test_reconstruction as TR
    from voxelhashing_amd import reconstruction as R
    path = str(tmp_path / "s3.sens")
    poses, _ = TR.make_sequence(path, oracle_lib)
    py = R.Reconstruction(TR.app_state(ICP), sens_files=[path])
    assert py.run() == TR.N and py.lost_frames == 0
    nat = R.Reconstruction(TR.app_state(ICP), sens_files=[path])
    with pytest.raises(ValueError, match="ICP"):
        nat.run_native(batch=4)  # as before without tracking=True
    assert nat.run_native(tracking=True, batch=4) == TR.N
    nat.native.synchronize()
    assert nat.lost_frames == 0 and len(nat.trajectory) == len(py.trajectory) == TR.N
    for k in range(TR.N):
        assert np.array_equal(nat.trajectory[k], py.trajectory[k]), k
    assert np.array_equal(nat.native.getPoses(), np.stack(py.trajectory))
    canonical.assert_same_scene(nat.scene.state(), py.scene.state(), "native tracked loop vs Python loop")
    assert_same_raycast(nat.ray, py.ray, "last ray cast")
    st = nat.native.getStats()
    assert st["trackedFrames"] == TR.N - 1 and st["lostFrames"] == 0 and st["frames"] == TR.N
    assert np.array_equal(py.trajectory[0], np.eye(4, dtype=np.float32))
    assert_on_the_true_trajectory(nat.trajectory, poses, (1, TR.N - 1))


def test_native_tracked_loop_on_resident_float_frames_at_sensor_size(vh, oracle_lib, tmp_path):
    """640x480, 4 frames, through run(): device copies of the depth and colour maps CUDARGBDSensor handed the Python loop"""
    import test_reconstruction as TR
    from voxelhashing_amd import engine as E, lib, reconstruction as R
    W, H, n = 640, 480, 4
    path = str(tmp_path / "s3_640.sens")
    write_sequence(path, oracle_lib, W, H, n)
    params = TR.PARAMS.replace("s_adapterWidth = 160", "s_adapterWidth = 640").replace("s_adapterHeight = 120", "s_adapterHeight = 480") + ICP
    state = lambda: R.read_app_state(params.encode())
    py = R.Reconstruction(state(), sens_files=[path])
    assert (py.cp.m_imageWidth, py.cp.m_imageHeight) == (W, H)
    want, depth, color = [], [], []
    for k in range(n):
        want.append(py.frame())
        maps = py.sensor.download()
        depth.append(lib.DeviceBuffer.from_numpy(np.ascontiguousarray(maps["depth"], dtype=np.float32)))
        color.append(lib.DeviceBuffer.from_numpy(np.ascontiguousarray(maps["color"], dtype=np.float32)))
    assert py.lost_frames == 0
    other = R.Reconstruction(state(), sens_files=[path])  # a second scene and ray caster with the same parameters
    loop = E.Reconstruction(other.scene, other.ray, None, other.cp, E.Reconstruction.defaultOptions(s_offlineProcessing=1))
    loop.setTracking(other.tracking)
    frames = E.Reconstruction.makeFrames([np.full(16, 7.0, np.float32)] * n, [d.ptr for d in depth], [c.ptr for c in color])  # (the poses are ignored)
    loop.run(frames)
    loop.synchronize()
    got = loop.getPoses()
    for k in range(n):
        assert np.array_equal(got[k], want[k]), k
    canonical.assert_same_scene(other.scene.state(), py.scene.state(), "resident float frames, 640x480")
    assert_same_raycast(other.ray, py.ray, "last ray cast, 640x480")
    st = loop.getStats()
    assert st["trackedFrames"] == n - 1 and st["lostFrames"] == 0 and st["framesWithRiders"] == 0


def test_lost_frame_is_skipped_and_tracking_goes_on(vh, oracle_lib, tmp_path):
    import test_reconstruction as TR
    from voxelhashing_amd import reconstruction as R
    path = str(tmp_path / "s3_blank5.sens")
    poses = write_sequence(path, oracle_lib, TR.W, TR.H, TR.N, blank=5)
    py = R.Reconstruction(TR.app_state(ICP), sens_files=[path])
    want = [py.frame() for _ in range(TR.N)]
    lost = [k for k in range(TR.N) if want[k][0, 0] == MINF]
    # the condition of this test, asked of the Python loop alone first: exactly one lost frame, frame 5
    assert lost == [5] and py.lost_frames == 1 and np.all(want[5] == MINF), lost
    nat = R.Reconstruction(TR.app_state(ICP), sens_files=[path])
    assert nat.run_native(tracking=True, batch=4) == TR.N
    nat.native.synchronize()
    got = nat.native.getPoses()
    assert len(got) == TR.N and np.all(got[5] == MINF)
    for k in range(TR.N):
        assert np.array_equal(got[k], want[k]), k
    assert nat.lost_frames == 1 and len(nat.trajectory) == len(py.trajectory) == TR.N - 1
    for a, b in zip(nat.trajectory, py.trajectory):
        assert np.array_equal(a, b)
    canonical.assert_same_scene(nat.scene.state(), py.scene.state(), "sequence with a lost frame")
    assert_same_raycast(nat.ray, py.ray, "last ray cast")
    st = nat.native.getStats()
    assert st["lostFrames"] == 1 and st["trackedFrames"] == TR.N - 2 and st["frames"] == TR.N - 1
    assert_on_the_true_trajectory(got, poses, (1, TR.N - 1))


STREAMING = """s_streamingEnabled = true;
s_streamingVoxelExtents = 0.5f 0.5f 0.5f;
s_streamingGridDimensions = 65 65 65;
s_streamingMinGridPos = -32 -32 -32;
s_streamingInitialChunkListSize = 16;
s_streamingRadius = 1.3f;
s_streamingPos = 0.0f 0.0f 1.8f;
s_streamingOutParts = 4;
"""


def test_tracking_with_streaming(vh, oracle_lib, tmp_path):
    """test_replay_with_streaming's streaming block with tracking instead of the trajectory.  No bit equality with the
    Python loop here: the two loops call different stream-in entry points."""
    import test_reconstruction as TR
    from voxelhashing_amd import reconstruction as R
    path = str(tmp_path / "s3.sens")
    poses, _ = TR.make_sequence(path, oracle_lib)
    nat = R.Reconstruction(TR.app_state(STREAMING + ICP), sens_files=[path])
    assert nat.run_native(tracking=True, batch=4) == TR.N
    nat.native.synchronize()
    assert nat.lost_frames == 0 and len(nat.trajectory) == TR.N
    nat.chunk_grid.debugCheckForDuplicates()
    assert nat.scene.debugHash()["duplicates"] == 0
    assert nat.chunk_grid.getStatistics()["blocks"] > 0 and nat.scene.state()["num_occupied"] > 100
    assert nat.native.getStats()["trackedFrames"] == TR.N - 1
    assert_on_the_true_trajectory(nat.trajectory, poses, (1, TR.N - 1))


def test_misuse_is_refused_and_the_default_is_left_alone(vh, oracle_lib, tmp_path):
    import test_reconstruction as TR
    from test_camera_tracking import setup_small
    from voxelhashing_amd import engine as E, lib, reconstruction as R
    L = lib.load()
    assert L.vh_icp_step(None, None, None, None, 160, 120, 0.15, 0.97, 1.0, None, None, None, None, 1.0, 1.0, 0.01, None, 0, None) == 4
    hp, cp, rp = setup_small()
    ts = T.make_tracking_state()

    def refused(loop, settings):
        with pytest.raises(lib.VhError) as e:
            loop.setTracking(settings)
        assert e.value.code == 4, e.value

    scene, ray = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=True, gc=False)), E.CUDARayCastSDF(rp)
    refused(E.Reconstruction(scene, None, None, cp, E.Reconstruction.defaultOptions(s_renderEnabled=0)), ts)   # no ray caster
    refused(E.Reconstruction(scene, ray, None, cp, E.Reconstruction.defaultOptions(s_renderEnabled=0)), ts)    # never ray-casts
    loop = E.Reconstruction(scene, ray, None, cp)
    refused(loop, T.make_tracking_state(levels=0, outer=(), inner=()))
    refused(loop, T.make_tracking_state(levels=8, outer=(1,) * 8, inner=(1,) * 8))  # 160 >> 7 < 2
    frame = E.synth_frame(synth.S3_SPHERES, 0, synth.orbit_pose(0, 400), cp)
    seq = E.Reconstruction.makeFrames([synth.orbit_pose(0, 400)], [frame.depth_ptr], [frame.color_ptr])
    loop.run(seq)
    loop.synchronize()
    refused(loop, ts)  # after a frame
    assert loop.getStats()["trackedFrames"] == 0 and loop.getStats()["lostFrames"] == 0

    # a loop whose setTracking was refused plays the recorded poses as it always did
    path = str(tmp_path / "s3.sens")
    poses, _ = TR.make_sequence(path, oracle_lib)
    recorded = "s_binaryDumpSensorUseTrajectory = true;\ns_binaryDumpSensorUseTrajectoryOnlyInit = false;\n"
    py = R.Reconstruction(TR.app_state(recorded), sens_files=[path])
    assert py.run() == TR.N
    nat = R.Reconstruction(TR.app_state(recorded), sens_files=[path])
    nat.prepare_native(batch=4)
    refused(nat.native, T.make_tracking_state(levels=0, outer=(), inner=()))
    assert nat.run_native(batch=4) == TR.N
    nat.native.synchronize()
    got = nat.native.getPoses()
    for k in range(TR.N):
        assert np.array_equal(got[k], np.asarray(poses[k], np.float32).reshape(4, 4)) and np.array_equal(nat.trajectory[k], py.trajectory[k]), k
    canonical.assert_same_scene(nat.scene.state(), py.scene.state(), "untracked native loop vs Python loop")
    st = nat.native.getStats()
    assert st["trackedFrames"] == 0 and st["lostFrames"] == 0 and st["frames"] == TR.N
