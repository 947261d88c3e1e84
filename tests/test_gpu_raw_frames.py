"""Raw frames through the native frame loop: 16-bit depth and RGB / RGBX bytes at the sensor's sizes, turned into
integrate's input on the device (vh_ingest_frame, then the Gauss filters that are on).

Everything is compared bit for bit: the kernel against the oracle's twins of the functions it fuses, against the class
path (CUDARGBDSensor.process on the host-converted frame), and the loop against the existing native loop fed with the
device maps the class path produced for the same frames, and against the oracle scene integrated with those maps."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_maps_equal, bits, small_config
from voxelhashing_amd import canonical, synth, vhtypes as T

pytestmark = pytest.mark.gpu

GAUSS = (2.0, 0.1)  # s_depthSigmaD / s_depthSigmaR and s_colorSigmaD / s_colorSigmaR of zParametersDefault.txt


@pytest.fixture(scope="module")
def E(vh):
    from voxelhashing_amd import engine
    return engine


def raw_images(depth_size, color_size, channels, seed):
    """seeded u16 depth with holes (0) and the extreme samples 1 and 65535; RGB / RGBX bytes with black pixels"""
    rng = np.random.default_rng(seed)
    (dw, dh) = depth_size
    depth = rng.integers(300, 6000, size=(dh, dw), dtype=np.uint16)
    depth[rng.random((dh, dw)) < 0.15] = 0
    depth[rng.random((dh, dw)) < 0.02] = 1
    depth[rng.random((dh, dw)) < 0.02] = 65535
    depth[0, 0], depth[0, 1], depth[-1, -1] = 0, 1, 65535
    color = None
    if channels:
        (cw, ch) = color_size
        color = rng.integers(0, 256, size=(ch, cw, channels), dtype=np.uint8)
        color[rng.random((ch, cw)) < 0.1, :3] = 0
        if channels == 4:
            color[..., 3] = rng.choice(np.array([0, 1, 128, 255], dtype=np.uint8), size=(ch, cw))
    return depth, color


def host_conversion(depth, color, shift):
    """SensorDataReader::processDepth (DSC/SensorDataReader.cpp:125-140): u16 / depthShift, RGB -> RGBX with X = 1"""
    d = depth.astype(np.float32) / np.float32(shift)
    if color is None:
        return d, None
    if color.shape[-1] == 4:
        return d, np.ascontiguousarray(color)
    rgbx = np.empty(color.shape[:2] + (4,), dtype=np.uint8)
    rgbx[..., :3] = color
    rgbx[..., 3] = 1
    return d, rgbx


def oracle_ingest(O, depth, color, adapter, shift):
    d, rgbx = host_conversion(depth, color, shift)
    (W, H), (dh, dw) = adapter, depth.shape
    want_d = O.image_op("resample_float_map", d, dw, dh, out_size=(W, H), prefill=np.full((H, W), np.nan, np.float32))
    want_c = None
    if rgbx is not None:
        ch, cw = rgbx.shape[:2]
        want_c = O.image_op("convert_color_raw_to_float4", rgbx, cw, ch, out_channels=4)
        if (cw, ch) != (W, H):  # CUDARGBDAdapter.cpp:113-118: a colour image of the adapter's size is copied
            want_c = O.image_op("resample_float4_map", want_c, cw, ch, out_channels=4, out_size=(W, H), prefill=np.full((H, W, 4), np.nan, np.float32))
    return want_d, want_c


SHAPES = [((160, 120), (160, 120), (160, 120)),      # equal sizes: depth resampled all the same, colour copied
          ((640, 480), (1296, 968), (640, 480)),     # ScanNet
          ((512, 424), (1920, 1080), (640, 480)),    # Kinect v2
          ((80, 60), (80, 60), (160, 120)),          # an upsample
          ((37, 23), (41, 29), (19, 11))]            # ragged: the last workgroup, the last quad


@pytest.mark.parametrize("shift", [1000.0, 5000.0])
@pytest.mark.parametrize("channels", [3, 4, 0])
@pytest.mark.parametrize("depth_size,color_size,adapter", SHAPES)
def test_ingest_kernel_equals_the_oracle(E, oracle_lib, depth_size, color_size, adapter, channels, shift):
    depth, color = raw_images(depth_size, color_size, channels, seed=depth_size[0] + channels)
    got_d, got_c = E.ingest_frame(depth, color, adapter, shift)
    want_d, want_c = oracle_ingest(oracle_lib, depth, color, adapter, shift)
    assert not np.isnan(want_d).any(), "the resampler left a pixel unwritten"
    assert np.array_equal(bits(got_d), bits(want_d)), f"depth differs at {(bits(got_d) != bits(want_d)).sum()} pixels"
    assert (got_d == 0).sum() > 0 and np.isfinite(got_d).all()  # a hole is 0.0f, not -inf
    if channels:
        assert np.array_equal(bits(got_c), bits(want_c)), f"colour differs at {(bits(got_c) != bits(want_c)).any(axis=-1).sum()} pixels"
        assert (got_c[..., 0] == -np.inf).sum() > 0
    else:
        assert got_c is None


def class_path(E, depth, color, adapter, shift, filters, cp_sensor=None):
    """the existing code: host conversion + CUDARGBDSensor.process -> (depth, colour, the sensor's DepthCameraParams)"""
    d, rgbx = host_conversion(depth, color, shift)
    (dh, dw), (ch, cw) = depth.shape, rgbx.shape[:2]
    cs = cp_sensor if cp_sensor is not None else T.make_depth_camera_params(dw, dh)
    sensor = E.CUDARGBDSensor((dw, dh), (cw, ch), adapter, cs.fx, cs.fy, cs.mx, cs.my, cs.m_sensorDepthWorldMin, cs.m_sensorDepthWorldMax)
    if filters:
        sensor.setFiterDepthValues(True, *GAUSS)
        sensor.setFiterIntensityValues(True, *GAUSS)
    sensor.process(d, rgbx)
    m = sensor.download()
    cp = sensor.getDepthCameraParams()
    sensor.close()
    return m["depth"], m["color"], cp


@pytest.mark.parametrize("filters", [False, True])
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("depth_size,color_size,adapter", SHAPES)
def test_ingest_kernel_equals_the_class_path(E, depth_size, color_size, adapter, channels, filters):
    depth, color = raw_images(depth_size, color_size, channels, seed=7 + depth_size[0])
    want_d, want_c, _ = class_path(E, depth, color, adapter, 1000.0, filters)
    got_d, got_c = E.ingest_frame(depth, color, adapter, 1000.0)
    if filters:  # the launchers the loop runs behind the ingest kernel, on the ingest kernel's output
        W, H = adapter
        got_d = E.image_op("gauss_filter_float_map", got_d, W, H, *GAUSS)
        got_c = E.image_op("gauss_filter_float4_map", got_c, W, H, *GAUSS, out_channels=4)
    assert np.array_equal(bits(got_d), bits(want_d)) and np.array_equal(bits(got_c), bits(want_c))


# ---- the loop ---------------------------------------------------------------------------------------------------------

OFFSET = np.array([7.3, 5.1, 3.7])  # away from the origin an online alloc pass is schedule-independent (test_gpu_frame_loop.py)
SHIFTED_S3 = synth.S3_SPHERES.copy()
SHIFTED_S3[:, :3] += OFFSET


def shifted_pose(k, n_frames):
    q = np.array(synth.orbit_pose(k, n_frames=n_frames), dtype=np.float32).copy()
    q[3] += np.float32(OFFSET[0])
    q[7] += np.float32(OFFSET[1])
    q[11] += np.float32(OFFSET[2])
    return q


class Sequence:
    """a synthetic S3 sequence as a sensor would record it (u16 millimetres, RGB bytes), and what the class path makes
    of every frame: host maps for the oracle, device maps for the existing native loop"""

    def __init__(self, E, O, n, depth_size, color_size, adapter, filters=False, invalid=None, n_orbit=100, spheres=SHIFTED_S3, pose=shifted_pose):
        cd, cc = T.make_depth_camera_params(*depth_size), T.make_depth_camera_params(*color_size)
        self.poses = [pose(k, n_orbit) for k in range(n)]
        self.depth, self.color, self.maps, self.frames = [], [], [], []
        self.format = dict(depth_size=depth_size, color_size=color_size, depth_shift=1000.0, color_channels=3,
                           depth_filter=GAUSS if filters else None, color_filter=GAUSS if filters else None)
        for p in self.poses:
            d, _ = O.synth_frame(spheres, 0, p, cd)
            _, c = O.synth_frame(spheres, 0, p, cc)
            self.depth.append(np.where(np.isfinite(d), np.floor(1000.0 * d.astype(np.float64) + 0.5), 0).astype(np.uint16))
            self.color.append(np.clip(np.where(np.isfinite(c[..., :3]), c[..., :3], 0) * 255.0, 0, 255).astype(np.uint8))
            md, mc, self.cp = class_path(E, self.depth[-1], self.color[-1], adapter, 1000.0, filters, cd)
            self.maps.append((md, mc))
            self.frames.append(E.DepthFrame(self.cp, depth=md, color=mc))
        if invalid is not None:
            self.poses[invalid] = self.poses[invalid].copy()
            self.poses[invalid][0] = -np.inf
        self.valid = [k for k in range(n) if k != invalid]

    def float_frames(self, E):
        return E.Reconstruction.makeFrames(self.poses, [f.depth_ptr for f in self.frames], [f.color_ptr for f in self.frames])

    def raw_frames(self, E, on_host):
        from voxelhashing_amd.lib import DeviceBuffer, PinnedArray
        make = PinnedArray.from_numpy if on_host else DeviceBuffer.from_numpy
        self._keep = [(make(d), make(c)) for d, c in zip(self.depth, self.color)]
        E.load().vh_device_synchronize()
        return E.Reconstruction.makeRawFrames(self.poses, [d.ptr for d, _ in self._keep], [c.ptr for _, c in self._keep])


def raycast_bits(ray):
    m = ray.download()
    return {k: bits(m[k]).copy() for k in ("depth", "depth4", "colors", "normals")}


@pytest.mark.parametrize("depth_size,color_size", [((160, 120), (160, 120)), ((320, 240), (400, 300))])
def test_raw_loop_equals_the_float_loop_and_the_oracle(E, oracle_lib, depth_size, color_size):
    O = oracle_lib
    n, adapter = 12, (160, 120)
    seq = Sequence(E, O, n, depth_size, color_size, adapter, invalid=5)
    cp = seq.cp
    assert (cp.m_imageWidth, cp.m_imageHeight) == adapter
    hp, _, _ = small_config(160, 120, num_buckets=1 << 17, num_sdf_blocks=1 << 12)
    rp = T.make_raycast_params(hp, cp)
    opt = T.make_scene_options(offline=False, gc=True, starve=5)
    # the oracle, and that alloc does not depend on the schedule for these frames
    ref = O.OracleScene(hp, cp, rp, opt)
    off = O.OracleScene(hp, cp, rp, T.make_scene_options(offline=True, gc=True, starve=5))
    for k in seq.valid:
        ref.integrate(seq.poses[k], *seq.maps[k])
        off.integrate(seq.poses[k], *seq.maps[k])
        assert np.array_equal(canonical.block_positions(ref.hash_table()), canonical.block_positions(off.hash_table())), "pick a scene without same-pass bucket sharing"
    want_state = ref.state()
    assert want_state["num_occupied"] > 50
    # the existing loop on the class path's device maps
    scene, ray = E.CUDASceneRepHashSDF(hp, opt), E.CUDARayCastSDF(rp)
    recon = E.Reconstruction(scene, ray, None, cp)
    recon.run(seq.float_frames(E))
    recon.synchronize()
    canonical.assert_same_scene(scene.state(), want_state, "float loop")
    want_maps = raycast_bits(ray)
    assert (want_maps["depth"] != bits(np.float32(-np.inf))).sum() > 2000
    recon.close()
    for on_host in (True, False):
        raw = seq.raw_frames(E, on_host)
        for ahead in (1, 0):
            for in_flight in (2, 16):
                for split in (False, True):
                    what = f"host={on_host} ahead={ahead} in flight={in_flight} split={split}"
                    scene, ray = E.CUDASceneRepHashSDF(hp, opt), E.CUDARayCastSDF(rp)
                    recon = E.Reconstruction(scene, ray, None, cp, E.Reconstruction.defaultOptions(s_framesOnHost=1 if on_host else 0, s_allocAhead=ahead,
                                                                                                  s_maxFramesInFlight=in_flight))
                    recon.setRawFormat(**seq.format)
                    if split:
                        for k0 in range(0, n, 3):
                            recon.runRaw(raw, k0, 3, lookahead=True)
                    else:
                        recon.runRaw(raw)
                    recon.synchronize()
                    canonical.assert_same_scene(scene.state(), want_state, what)
                    got = raycast_bits(ray)
                    for m in want_maps:
                        assert np.array_equal(got[m], want_maps[m]), f"{what}: ray-cast map {m}"
                    st = recon.getStats()
                    assert st["frames"] == n - 1 and st["invalidFrames"] == 1, what
                    assert st["uploadBytes"] == 2 * depth_size[0] * depth_size[1] + 3 * color_size[0] * color_size[1]
                    assert st["uploadsTimed"] >= 1 and st["uploadMs"] > 0
                    recon.close()
                    ray.close()
                    scene.close()


def test_raw_loop_with_the_filters_on(E, oracle_lib):
    """s_depthFilter / s_colorFilter: the Gauss filters run behind the ingest kernel on the copy stream"""
    O = oracle_lib
    n, adapter = 10, (160, 120)
    seq = Sequence(E, O, n, (320, 240), (400, 300), adapter, filters=True)
    cp = seq.cp
    hp, _, _ = small_config(160, 120, num_buckets=1 << 17, num_sdf_blocks=1 << 12)
    rp = T.make_raycast_params(hp, cp)
    opt = T.make_scene_options(offline=True, gc=True, starve=5)
    ref = O.OracleScene(hp, cp, rp, opt)
    for k in range(n):
        ref.integrate(seq.poses[k], *seq.maps[k])
    for on_host in (True, False):
        scene, ray = E.CUDASceneRepHashSDF(hp, opt), E.CUDARayCastSDF(rp)
        recon = E.Reconstruction(scene, ray, None, cp, E.Reconstruction.defaultOptions(s_framesOnHost=1 if on_host else 0))
        recon.setRawFormat(**seq.format)
        recon.runRaw(seq.raw_frames(E, on_host))
        recon.synchronize()
        canonical.assert_same_scene(scene.state(), ref.state(), f"filters on, host={on_host}")
        ray.render(scene.getHashData(), scene.getHashParams(), cp, seq.poses[-1])
        assert_maps_equal(ray.download(), ref.render(seq.poses[-1]), "render after the filtered sequence")
        recon.close()


def test_staging_slots_are_not_overwritten_early(E, oracle_lib):
    """more than three times as many frames as staging slots (4), no run-ahead bound, every frame's depth different:
    a slot reused before its frame was integrated shows as a wrong scene"""
    O = oracle_lib
    n, adapter = 14, (160, 120)
    seq = Sequence(E, O, n, (160, 120), (160, 120), adapter, n_orbit=60)
    assert len({d.tobytes() for d in seq.depth}) == n
    cp = seq.cp
    hp, _, _ = small_config(160, 120, num_buckets=1 << 17, num_sdf_blocks=1 << 12)
    rp = T.make_raycast_params(hp, cp)
    opt = T.make_scene_options(offline=True, gc=True, starve=5)
    ref = O.OracleScene(hp, cp, rp, opt)
    for k in range(n):
        ref.integrate(seq.poses[k], *seq.maps[k])
    for on_host in (True, False):
        scene, ray = E.CUDASceneRepHashSDF(hp, opt), E.CUDARayCastSDF(rp)
        recon = E.Reconstruction(scene, ray, None, cp, E.Reconstruction.defaultOptions(s_framesOnHost=1 if on_host else 0, s_maxFramesInFlight=0))
        recon.setRawFormat(**seq.format)
        recon.runRaw(seq.raw_frames(E, on_host))
        recon.synchronize()
        canonical.assert_same_scene(scene.state(), ref.state(), f"slot reuse, host={on_host}")
        assert recon.getStats()["frames"] == n
        recon.close()


def test_loop_checks_the_format_and_the_order_of_calls(E):
    hp, cp, rp = small_config(160, 120)
    scene, ray = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=True, gc=False)), E.CUDARayCastSDF(rp)
    recon = E.Reconstruction(scene, ray, None, cp)
    raw = E.Reconstruction.makeRawFrames([np.eye(4, dtype=np.float32)], [4096], [8192])
    with pytest.raises(Exception, match="no raw format"):
        recon.runRaw(raw)
    ok = dict(depth_size=(160, 120), color_size=(160, 120), depth_shift=1000.0, color_channels=3)
    for bad in (dict(depth_size=(1, 120)), dict(depth_size=(160, 0)), dict(color_size=(1, 1)), dict(color_channels=2), dict(color_channels=5),
                dict(depth_shift=0.0), dict(depth_shift=-1.0), dict(depth_shift=float("inf")), dict(depth_shift=float("nan")),
                dict(depth_filter=(0.0, 0.1)), dict(color_filter=(2.0, float("nan")))):
        with pytest.raises(Exception, match="bad argument"):
            recon.setRawFormat(**{**ok, **bad})
    recon.setRawFormat(**ok)
    with pytest.raises(Exception, match="already set"):
        recon.setRawFormat(**ok)
    flt = E.Reconstruction.makeFrames([np.eye(4, dtype=np.float32)], [4096], [8192])
    with pytest.raises(Exception, match="raw frames"):
        recon.run(flt)
    recon.close()
    tiny = T.make_depth_camera_params(1, 120)  # an adapter the resampler cannot serve
    recon = E.Reconstruction(scene, None, None, tiny, E.Reconstruction.defaultOptions(s_renderEnabled=0))
    with pytest.raises(Exception, match="bad argument"):
        recon.setRawFormat(**ok)
    recon.close()


# ---- streaming ----------------------------------------------------------------------------------------------------------

EXT, DIMS, MINP, PARTS = (0.5, 0.5, 0.5), (65, 65, 65), (-32, -32, -32), 4
STREAM_POS = (0.0, 0.0, 1.6)
RADIUS = 1.2


def sorted_blocks(descs, blocks):
    order = canonical.lexsort_pos(np.ascontiguousarray(descs["pos"]))
    return np.ascontiguousarray(descs["pos"][order]), np.ascontiguousarray(blocks[order])


def test_raw_loop_with_streaming_equals_the_float_loop(E, oracle_lib):
    """blocks leave and come back along the orbit (test_gpu_streaming.py's set-up): the raw loop moves the same blocks as
    the float loop fed with the class path's maps"""
    n, adapter = 60, (160, 120)
    spheres = synth.S1_SPHERES.copy()
    spheres[:, :3] += OFFSET
    seq = Sequence(E, oracle_lib, n, (160, 120), (200, 150), adapter, n_orbit=120, spheres=spheres)
    cp = seq.cp
    hp, _, _ = small_config(160, 120, num_buckets=1 << 15, num_sdf_blocks=1 << 13, streaming_extents=EXT, streaming_dims=DIMS, streaming_min=MINP)
    rp = T.make_raycast_params(hp, cp)

    def run(raw, on_host):
        opt = T.make_scene_options(offline=False, gc=True, starve=15, streaming_out_parts=PARTS)
        scene, ray = E.CUDASceneRepHashSDF(hp, opt), E.CUDARayCastSDF(rp)
        grid = E.CUDASceneRepChunkGrid(scene, EXT, DIMS, MINP, 64, True, PARTS)
        recon = E.Reconstruction(scene, ray, grid, cp, E.Reconstruction.defaultOptions(s_streamingEnabled=1, s_streamingPos=STREAM_POS, s_streamingRadius=RADIUS,
                                                                                      s_allocAhead=1, s_maxFramesInFlight=4, s_framesOnHost=1 if on_host else 0))
        if raw:
            recon.setRawFormat(**seq.format)
            frames = seq.raw_frames(E, on_host)
        else:
            frames = seq.float_frames(E)
        for k0 in range(0, n, 20):
            (recon.runRaw if raw else recon.run)(frames, k0, 20)
            recon.synchronize()
        stats = recon.getStats()
        maps = raycast_bits(ray)
        host = sorted_blocks(*grid.downloadHostBlocks())
        grid.debugCheckForDuplicates()
        grid.reset()
        state = scene.state()
        recon.close()
        grid.close()
        return state, host, maps, stats

    sf, hf, mf, tf = run(False, False)
    assert tf["blocksStreamedOut"] > 20 and tf["blocksStreamedIn"] > 0, tf
    for on_host in (True, False):
        sr, hr, mr, tr = run(True, on_host)
        canonical.assert_same_scene(sr, sf, f"streaming, raw frames, host={on_host}")
        assert np.array_equal(hr[0], hf[0]) and hr[1].tobytes() == hf[1].tobytes(), "host chunk grids differ"
        for m in mf:
            assert np.array_equal(mr[m], mf[m]), m
        assert (tr["blocksStreamedOut"], tr["blocksStreamedIn"], tr["frames"]) == (tf["blocksStreamedOut"], tf["blocksStreamedIn"], n)


# ---- a ray cast that fails in the middle of a raw run ----------------------------------------------------------------------

@pytest.mark.parametrize("on_host", [True, False])
def test_a_failing_ray_cast_in_a_raw_run(E, oracle_lib, on_host):
    O = oracle_lib
    n, adapter = 12, (160, 120)
    seq = Sequence(E, O, n, (320, 240), (400, 300), adapter)
    cp = seq.cp
    hp, _, _ = small_config(160, 120, num_buckets=1 << 17, num_sdf_blocks=1 << 12)
    rp = T.make_raycast_params(hp, cp)
    opt = T.make_scene_options(offline=False, gc=True, starve=5)
    raw = seq.raw_frames(E, on_host)
    options = E.Reconstruction.defaultOptions(s_framesOnHost=1 if on_host else 0, s_allocAhead=1, s_maxFramesInFlight=4)
    # a run that nothing disturbs
    scene0, ray0 = E.CUDASceneRepHashSDF(hp, opt), E.CUDARayCastSDF(rp)
    fresh = E.Reconstruction(scene0, ray0, None, cp, options)
    fresh.setRawFormat(**seq.format)
    fresh.runRaw(raw)
    fresh.synchronize()
    want, want_maps = scene0.state(), raycast_bits(ray0)
    for nth in (1, 3, 6):
        scene, ray = E.CUDASceneRepHashSDF(hp, opt), E.CUDARayCastSDF(rp)
        recon = E.Reconstruction(scene, ray, None, cp, options)
        recon.setRawFormat(**seq.format)
        recon.runRaw(raw, 0, 2)
        recon.debugFailRender(nth)
        with pytest.raises(Exception, match="injected"):
            recon.runRaw(raw, 2, n - 2)
        recon.synchronize()
        done = recon.getStats()["frames"]
        assert done == 2 + nth - 1
        recon.runRaw(raw, done, n - done)  # the frame that failed is run again
        recon.synchronize()
        assert recon.getStats()["frames"] == n
        canonical.assert_same_scene(scene.state(), want, f"after a failure at render {nth}")
        got = raycast_bits(ray)
        for m in want_maps:
            assert np.array_equal(got[m], want_maps[m]), m
        recon.close()
    fresh.close()


# ---- a `.sens` file through the native loop -------------------------------------------------------------------------------

PARAMS = """
s_sensorIdx = 8;
s_adapterWidth = 160;
s_adapterHeight = 120;
s_sensorDepthMax = 5.0f;
s_sensorDepthMin = 0.5f;
s_hashNumBuckets = 16384;
s_hashNumSDFBlocks = 8192;
s_hashMaxCollisionLinkedListSize = 7;
s_SDFVoxelSize = 0.02f;
s_SDFMarchingCubeThreshFactor = 10.0f;
s_SDFTruncation = 0.10f;
s_SDFTruncationScale = 0.05f;
s_SDFMaxIntegrationDistance = 4.0f;
s_SDFIntegrationWeightSample = 10;
s_SDFIntegrationWeightMax = 255;
s_SDFRayIncrementFactor = 0.8f;
s_SDFRayThresSampleDistFactor = 50.5f;
s_SDFRayThresDistFactor = 50.0f;
s_SDFUseGradients = false;
s_depthSigmaD = 2.0f;
s_depthSigmaR = 0.1f;
s_depthFilter = true;
s_colorSigmaD = 2.0f;
s_colorSigmaR = 0.1f;
s_colorFilter = false;
s_integrationEnabled = true;
s_trackingEnabled = true;
s_garbageCollectionEnabled = false;
s_garbageCollectionStarve = 15;
s_marchingCubesMaxNumTriangles = 400000;
s_streamingEnabled = false;
s_offlineProcessing = true;
s_playData = true;
s_reconstructionEnabled = true;
s_binaryDumpSensorUseTrajectory = true;
s_binaryDumpSensorUseTrajectoryOnlyInit = false;
"""


def write_sens(path, O, n, depth_size, color_size, first=0):
    from voxelhashing_amd import sensor_data as SD
    cd, cc = T.make_depth_camera_params(*depth_size), T.make_depth_camera_params(*color_size)
    sd = SD.SensorData.create(depth_size, color_size, SD.make_intrinsic_matrix(cd.fx, cd.fy, cd.mx, cd.my), SD.make_intrinsic_matrix(cc.fx, cc.fy, cc.mx, cc.my),
                              depth_shift=1000.0, sensor_name="synthetic S3", depth_type=SD.TYPE_ZLIB_USHORT)
    for k in range(first, first + n):
        p = synth.orbit_pose(k, n_frames=400)
        d, _ = O.synth_frame(synth.S3_SPHERES, 0, p, cd)
        _, c = O.synth_frame(synth.S3_SPHERES, 0, p, cc)
        mm = np.where(np.isfinite(d), np.floor(1000.0 * d.astype(np.float64) + 0.5), 0).astype(np.uint16)
        rgb = np.clip(np.where(np.isfinite(c[..., :3]), c[..., :3], 0) * 255.0, 0, 255).astype(np.uint8)
        sd.addFrame(rgb, mm, p, 100 + k, 200 + k)
    sd.saveToFile(path)


def sorted_rows(tris):
    flat = np.ascontiguousarray(tris).view(np.uint8).reshape(len(tris), -1)
    return flat[np.lexsort(flat.T[::-1])]


def test_run_native_equals_the_python_loop_on_a_sens_file(E, oracle_lib, tmp_path):
    from voxelhashing_amd import reconstruction as R
    files = [str(tmp_path / "a.sens"), str(tmp_path / "b.sens")]
    write_sens(files[0], oracle_lib, 9, (320, 240), (400, 300))
    write_sens(files[1], oracle_lib, 5, (320, 240), (400, 300), first=9)
    g = R.read_app_state(PARAMS.encode())
    py = R.Reconstruction(g, sens_files=files)
    assert py.run() == 14
    py.scene.synchronize()
    nat = R.Reconstruction(g, sens_files=files)
    for f in ("fx", "fy", "mx", "my", "m_imageWidth", "m_imageHeight", "m_sensorDepthWorldMin", "m_sensorDepthWorldMax"):
        assert getattr(nat.cp, f) == getattr(py.cp, f)
    assert nat.run_native(batch=4) == 14  # batches that end inside a file and at its end
    st = nat.native.getStats()
    assert st["frames"] == 14 and st["invalidFrames"] == 0
    canonical.assert_same_scene(nat.scene.state(), py.scene.state(), "native loop vs Python loop")
    assert len(nat.trajectory) == len(py.trajectory) == 14
    for a, b in zip(nat.trajectory, py.trajectory):
        assert np.array_equal(a, b)
    tris = []
    for rec in (nat, py):
        mc = E.CUDAMarchingCubesHashSDF(rec.mp)
        mc.extractIsoSurface(rec.scene.getHashData(), rec.scene.getHashParams())
        tris.append(sorted_rows(mc.triangles()))
    assert len(tris[0]) > 200 and np.array_equal(tris[0], tris[1])
    out = str(tmp_path / "native.ply")
    mesh = nat.extractIsoSurface(out)
    assert len(mesh["vertices"]) > 100 and len(mesh["faces"]) > 100
    import os
    assert os.path.getsize(out) > 1000 and b"element face" in open(out, "rb").read(600)
    with pytest.raises(RuntimeError, match="native loop"):
        nat.frame()
    # what the native loop cannot do is refused with the reason
    icp = R.Reconstruction(R.read_app_state(PARAMS.replace("s_binaryDumpSensorUseTrajectory = true", "s_binaryDumpSensorUseTrajectory = false").encode()),
                           sens_files=files[:1])
    with pytest.raises(ValueError, match="ICP"):
        icp.run_native()
    with pytest.raises(ValueError, match="Python loop"):
        py.run_native()
