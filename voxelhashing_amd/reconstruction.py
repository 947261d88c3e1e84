"""The reference's frame loop for a recorded sequence, over the C ABI: `reconstruction()`
(DepthSensingCUDA/Source/DepthSensing.cpp:720-924) with the SensorDataReader as the sensor, plus the two things
the application does around it -- recording what was processed (RGBDSensor::recordFrame / recordTrajectory /
saveRecordedFramesToFile, RGBDSensor.cpp:275-389) and StopScanningAndExtractIsoSurfaceMC (DepthSensing.cpp:284-373).

Everything is configured the way the application is: a GlobalAppState parameter file (zParameters*.txt) and a
tracking parameter file.  The D3D window, the GUI and the live sensors are out of scope."""
import ctypes as C
import os
import sys

import numpy as np

from . import engine as E
from . import sensor_data as SD
from . import vhtypes as T
from .lib import check, load

MINF = np.float32(-np.inf)


def read_app_state(path_or_text):
    """zParameters*.txt (a path, or the text itself as bytes) -> AppState"""
    L = load()
    g = T.AppState()
    if isinstance(path_or_text, bytes):
        check(L.vh_app_state_parse(path_or_text, C.byref(g)), "vh_app_state_parse")
    else:
        check(L.vh_app_state_read(str(path_or_text).encode(), C.byref(g)), "vh_app_state_read")
    return g


def read_tracking_state(path_or_text):
    L = load()
    t = T.TrackingState()
    if isinstance(path_or_text, bytes):
        check(L.vh_tracking_state_parse(path_or_text, C.byref(t)), "vh_tracking_state_parse")
    else:
        check(L.vh_tracking_state_read(str(path_or_text).encode(), C.byref(t)), "vh_tracking_state_read")
    return t


def read_tracking_state_rgbd(path_or_text):
    """the tracking parameter file with the RGB-D tracker's four colour keys (VhTrackingStateRGBD)"""
    L = load()
    t = T.TrackingStateRGBD()
    if isinstance(path_or_text, bytes):
        check(L.vh_tracking_state_rgbd_parse(path_or_text, C.byref(t)), "vh_tracking_state_rgbd_parse")
    else:
        check(L.vh_tracking_state_rgbd_read(str(path_or_text).encode(), C.byref(t)), "vh_tracking_state_rgbd_read")
    return t


def read_render_state(path_or_text):
    """the rendering keys of a zParameters*.txt (RenderState: light, material, discontinuity thresholds, s_renderToFile)"""
    L = load()
    r = T.RenderState()
    if isinstance(path_or_text, bytes):
        check(L.vh_parse_render_state(path_or_text, C.byref(r)), "vh_parse_render_state")
    else:
        check(L.vh_read_render_state(str(path_or_text).encode(), C.byref(r)), "vh_read_render_state")
    return r


def read_calibration_state(path_or_text):
    """the camera-calibration keys of a zParameters*.txt (CalibrationState: s_bUseCameraCalibration and the two remapping
    discontinuity thresholds)"""
    L = load()
    c = T.CalibrationState()
    if isinstance(path_or_text, bytes):
        check(L.vh_parse_calibration_state(path_or_text, C.byref(c)), "vh_parse_calibration_state")
    else:
        check(L.vh_read_calibration_state(str(path_or_text).encode(), C.byref(c)), "vh_read_calibration_state")
    return c


IDENTITY_EXTRINSICS_WARNING = ("Warning: forcing s_bUseCameraCalibration to be false because the m_depthExtrinsics are the identity "
                               "(i.e., already aligned)")


def camera_calibration(header, calibration_state):
    """RGBDSensor::initializeDepthExtrinsics (RGBDSensor.cpp:146-156) for a `.sens` header: None when the key is off or
    the depth extrinsic is the identity (then with the reference's warning, on stderr), else the arguments of
    CUDARGBDSensor.setCameraCalibration: the colour intrinsics (fx, fy, mx, my) at the colour sensor's resolution, the
    depth extrinsic and the two thresholds"""
    if calibration_state is None or not calibration_state.s_bUseCameraCalibration:
        return None
    ext = np.array(header.m_depthExtrinsic[:], dtype=np.float32).reshape(4, 4)
    if np.array_equal(ext, np.eye(4, dtype=np.float32)):  # mLib's operator==: exact, entry by entry
        print(IDENTITY_EXTRINSICS_WARNING, file=sys.stderr)
        return None
    ci = np.array(header.m_colorIntrinsic[:], dtype=np.float32).reshape(4, 4)
    return (float(ci[0, 0]), float(ci[1, 1]), float(ci[0, 2]), float(ci[1, 2]), ext,
            calibration_state.s_remappingDepthDiscontinuityThresOffset, calibration_state.s_remappingDepthDiscontinuityThresLin)


def adapter_color_intrinsics(color_intrinsic, color_size, adapter_size):
    """CUDARGBDAdapter's colour intrinsics (DSC/CUDARGBDAdapter.cpp:61-66): the sensor's, rescaled to the adapter size"""
    m = np.array(color_intrinsic, dtype=np.float32).reshape(4, 4).copy()
    (cw, ch), (W, H) = color_size, adapter_size
    f = np.float32
    m[0, 0] *= f(W) / f(cw)
    m[1, 1] *= f(H) / f(ch)
    m[0, 2] *= f(W - 1) / f(cw - 1) if cw > 1 else f(1)
    m[1, 2] *= f(H - 1) / f(ch - 1) if ch > 1 else f(1)
    return m


def rgbx_alpha_rule(rgbx):
    """renderToFile's alpha rule (DSC/DepthSensing.cpp:1199-1202): alpha = 255 where any of r, g, b is > 0"""
    out = np.array(rgbx, dtype=np.uint8, copy=True)
    out[(out[..., :3] > 0).any(axis=-1), 3] = 255
    return out


def depth_image_rgba8(depth):
    """renderToFile's input_depth image: mLib's ColorImageR32G32B32A32(DepthImage) (baseImage.h:822-845; per-image min / max
    over the values that are not -inf, hue 240 (1 - x), S = 1, V = 0.5, baseImageHelper.h:68-115), the alpha rule, 0 where
    the depth is 0 or -inf, then FreeImageWrapper's (unsigned char)(255 c) per channel.  A NaN hue (every valid depth
    equal) is taken as 0."""
    f = np.float32
    d = np.asarray(depth, dtype=np.float32)
    valid = d != -np.inf
    out = np.zeros(d.shape + (4,), dtype=np.float32)
    if valid.any():
        lo, hi = d[valid].min(), d[valid].max()
        with np.errstate(divide="ignore", invalid="ignore"):
            x = f(1) - (d - lo) / (hi - lo)
        x = np.where(x < 0, f(0), np.where(x > 1, f(1), x))
        x = np.where(np.isnan(x), f(0), x).astype(np.float32)
        hd = (f(240) * x) / f(60)
        h = hd.astype(np.uint32)
        fr = hd - h.astype(np.float32)
        V = f(0.5)
        p = V * (f(1) - f(1))
        q = V * (f(1) - fr)
        t = V * (f(1) - (f(1) - fr))
        pp = np.full_like(q, p)
        vv = np.full_like(q, V)
        # convertHSVtoRGB: sector h of six, h > 4 (never reached for a hue <= 240) is (V, p, q)
        cases = [((h == 0) | (h == 6), (vv, t, pp)), (h == 1, (q, vv, pp)), (h == 2, (pp, vv, t)), (h == 3, (pp, q, vv)), (h == 4, (t, pp, vv))]
        rgb = np.stack((vv, pp, q), -1)
        for cond, c in cases:
            rgb = np.where(cond[..., None], np.stack(c, -1), rgb)
        out[..., :3] = rgb
        out[..., 3] = 1.0
        out[~valid] = 0.0
    out[(d == 0) | (d == -np.inf)] = 0.0
    return (out * f(255)).astype(np.uint8)


def native_refusal(app_state, render_state=None, camera_calibration=False, use_rgbd_tracking=False, tracking=False, tracking_rgbd=False):
    """Why the native frame loop cannot play this configuration, as text, or None when it can.  The native loop
    (engine.Reconstruction) integrates every frame at the pose the file holds: s_binaryDumpSensorUseTrajectory = true,
    s_binaryDumpSensorUseTrajectoryOnlyInit = false.  tracking=True: the caller lets the loop track the camera itself
    (engine.Reconstruction.setTracking), which admits s_binaryDumpSensorUseTrajectory = false with the plain ICP tracker.
    tracking_rgbd=True (with tracking=True): the caller lets it do so with the RGB-D tracker as well
    (engine.Reconstruction.setTrackingRGBD), which admits use_rgbd_tracking.  Both keywords only permit.  Needs no device."""
    g = app_state
    rgbd_allowed = bool(tracking and tracking_rgbd)
    if tracking and use_rgbd_tracking and not rgbd_allowed:
        return "the poses come from the RGB-D tracker: the native loop tracks with plain projective ICP only"
    if (not g.s_binaryDumpSensorUseTrajectory and not tracking) or (use_rgbd_tracking and not rgbd_allowed):
        return "the poses come from ICP tracking (s_binaryDumpSensorUseTrajectory = false): the native loop has no tracker"
    if g.s_binaryDumpSensorUseTrajectory and g.s_binaryDumpSensorUseTrajectoryOnlyInit:  # (without the trajectory the key means nothing)
        return "s_binaryDumpSensorUseTrajectoryOnlyInit = true tracks from the recorded pose: the native loop has no tracker"
    if not g.s_trackingEnabled:
        return "s_trackingEnabled = false integrates every frame at the identity, not at the recorded pose"
    if g.s_recordData:
        return "s_recordData = true records the float frames of the Python loop"
    if render_state is not None and render_state.s_renderToFile:
        return "s_renderToFile = true draws every frame between two frames of the loop"
    if camera_calibration:
        return "s_bUseCameraCalibration = true remaps depth into the colour camera, which the native loop's ingest does not"
    return None


def decode_batch(sensor_data, first, count, depth_out=None, color_out=None):
    """Frames [first, first + count) of a SensorData as the file holds them -> (depth [count, h, w] u16, colour
    [count, h', w', 3] u8 or None when the file has no colour, poses [count, 16] f32).  depth_out / color_out: arrays
    of at least these shapes to decode into (pinned memory for the native loop).  Needs no device."""
    i = sensor_data.info()
    if first < 0 or count < 0 or first + count > i.m_numFrames:
        raise IndexError("frame range outside the sequence")
    has_color = i.m_colorWidth * i.m_colorHeight > 0
    depth = depth_out[:count] if depth_out is not None else np.empty((count, i.m_depthHeight, i.m_depthWidth), dtype=np.uint16)
    color = None
    if has_color:
        color = color_out[:count] if color_out is not None else np.empty((count, i.m_colorHeight, i.m_colorWidth, 3), dtype=np.uint8)
    if depth.shape[1:] != (i.m_depthHeight, i.m_depthWidth) or depth.dtype != np.uint16 or not depth.flags.c_contiguous:
        raise ValueError("depth_out does not fit the sequence")
    if color is not None and (color.shape[1:] != (i.m_colorHeight, i.m_colorWidth, 3) or color.dtype != np.uint8 or not color.flags.c_contiguous):
        raise ValueError("color_out does not fit the sequence")
    poses = np.empty((count, 16), dtype=np.float32)
    for k in range(count):
        check(sensor_data.L.vh_sensor_data_get_frame(sensor_data.handle, first + k, depth[k].ctypes.data, color[k].ctypes.data if color is not None else None,
                                                     poses[k].ctypes.data_as(C.POINTER(C.c_float)), None), "vh_sensor_data_get_frame")
    return depth, color, poses


class Reconstruction:
    """One scene fed from `.sens` files.  `frame()` is one pass of the reference's render callback with
    reconstruction enabled: read a frame, pre-process it, ray-cast the model at the last pose, find the new pose
    (recorded trajectory or projective ICP), stream, integrate.

    use_rgbd_tracking (off by default) is the reference's useRGBDTracking (DSC/DepthSensing.cpp:816): the pose comes
    from CUDACameraTrackingMultiResRGBD, fed with the sensor's colour map and the ray cast's colours as well.  Its
    tracking_state is then a TrackingStateRGBD (read_tracking_state_rgbd); a plain TrackingState keeps the colour keys'
    defaults.

    render_state (a RenderState, read_render_state; None by default) carries the rendering keys.  When its
    s_renderToFile is set, every frame read ends with the reference's renderToFile (DSC/DepthSensing.cpp:1150-1255):
    the model ray-cast at the last pose, drawn as a mesh and lit, into s_renderToFileDir/reconstruction/%06d.png
    (material) and reconstruction_color/%06d.png (colour), plus the input as input_color/ and input_depth/ images.

    calibration_state (a CalibrationState, read_calibration_state; None by default) carries s_bUseCameraCalibration.  When
    it is set and the `.sens` depth extrinsic is not the identity, the sensor renders every depth map into the colour
    camera before anything uses it (CUDARGBDSensor.cpp:198-217); an identity extrinsic leaves it off with the reference's
    warning.  camera_calibration tells which took effect.

    weighted_colour (off by default; not a key of the parameter file) fuses colours weighted by the voxel weights instead
    of the reference's running 50/50 average (CUDASceneRepHashSDF.setColorIntegration): the ray cast then shows a surface
    at the brightness it was seen at, which the RGB-D tracker needs to follow its own reconstruction.  It belongs to the
    scene, so frame() and run_native() integrate alike."""

    def __init__(self, app_state, tracking_state=None, sens_files=None, stream=None, use_rgbd_tracking=False, render_state=None,
                 calibration_state=None, weighted_colour=False):
        self.L = load()
        self.gas = app_state
        self.tracking_rgbd = None
        if use_rgbd_tracking:
            if isinstance(tracking_state, T.TrackingStateRGBD):
                self.tracking_rgbd = tracking_state
            else:
                self.tracking_rgbd = T.make_tracking_state_rgbd()
                if tracking_state is not None:
                    self.tracking_rgbd.base = tracking_state
            tracking_state = self.tracking_rgbd.base
        self.tracking = tracking_state if tracking_state is not None else T.make_tracking_state()
        if sens_files is None:
            sens_files = [bytes(app_state.s_binaryDumpSensorFile[i].value).decode() for i in range(app_state.s_numBinaryDumpSensorFiles)]
        if not sens_files:
            raise ValueError("need to specify s_binaryDumpSensorFile[0]")  # SensorDataReader.cpp:43
        self.sens_files = list(sens_files)
        self.file_idx = 0
        self.reader = SD.SensorDataReader(self.sens_files[0])
        h = self.reader.header
        g = app_state
        self.adapter_size = (g.s_adapterWidth, g.s_adapterHeight)
        di = np.array(h.m_depthIntrinsic[:], dtype=np.float32).reshape(4, 4)
        # RGBDSensor::init + initializeDepthIntrinsics (SensorDataReader.cpp:56-58); the adapter rescales them
        self.sensor = E.CUDARGBDSensor((h.m_depthWidth, h.m_depthHeight), (max(h.m_colorWidth, 1), max(h.m_colorHeight, 1)), self.adapter_size,
                                       float(di[0, 0]), float(di[1, 1]), float(di[0, 2]), float(di[1, 2]), g.s_sensorDepthMin, g.s_sensorDepthMax, stream=stream)
        if g.s_depthFilter:
            self.sensor.setFiterDepthValues(True, g.s_depthSigmaD, g.s_depthSigmaR)
        if g.s_colorFilter:
            self.sensor.setFiterIntensityValues(True, g.s_colorSigmaD, g.s_colorSigmaR)
        calib = camera_calibration(h, calibration_state)
        if calib is not None:
            self.sensor.setCameraCalibration(True, *calib)
        self.camera_calibration = self.sensor.getCameraCalibration()[0]
        self.cp = self.sensor.getDepthCameraParams()
        hp, opt, rp, mp = T.HashParams(), T.SceneOptions(), T.RayCastParams(), T.MarchingCubesParams()
        self.L.vh_hash_params_from_app_state(C.byref(g), C.byref(hp))
        self.L.vh_scene_options_from_app_state(C.byref(g), C.byref(opt))
        intr = np.eye(4, dtype=np.float32)
        intr[0, 0], intr[1, 1], intr[0, 2], intr[1, 2] = self.cp.fx, self.cp.fy, self.cp.mx, self.cp.my
        inv = np.linalg.inv(intr.astype(np.float64)).astype(np.float32)
        fp = lambda a: np.ascontiguousarray(a, dtype=np.float32).reshape(16).ctypes.data_as(C.POINTER(C.c_float))
        self.L.vh_raycast_params_from_app_state(C.byref(g), fp(intr), fp(inv), C.byref(rp))
        self.L.vh_marching_cubes_params_from_app_state(C.byref(g), C.byref(mp))
        self.hp, self.rp, self.mp = hp, rp, mp
        self.scene = E.CUDASceneRepHashSDF(hp, opt, stream=stream)
        self.weighted_colour = bool(weighted_colour)
        if self.weighted_colour:
            self.scene.setColorIntegration(T.COLOR_WEIGHTED_AVERAGE)
        self.ray = E.CUDARayCastSDF(rp, stream=stream)
        self.chunk_grid = None
        if g.s_streamingEnabled:
            self.chunk_grid = E.CUDASceneRepChunkGrid(self.scene, tuple(g.s_streamingVoxelExtents), tuple(g.s_streamingGridDimensions),
                                                      tuple(g.s_streamingMinGridPos), g.s_streamingInitialChunkListSize, False, g.s_streamingOutParts)
        self.tracker = E.CUDACameraTrackingMultiRes(self.adapter_size[0], self.adapter_size[1], self.tracking.s_maxLevels, stream=stream)
        self.tracker_rgbd = None
        if self.tracking_rgbd is not None:
            self.tracker_rgbd = E.CUDACameraTrackingMultiResRGBD(self.adapter_size[0], self.adapter_size[1], self.tracking.s_maxLevels, stream=stream)
        self.marching_cubes = None
        self.live_marching_cubes = None  # the extractor that holds the live mesh, once liveMeshBegin has made it
        cam = self.sensor.getDepthCameraData()
        self.frame_data = E.DepthFrame(self.cp, depth_ptr=cam.d_depthData, color_ptr=cam.d_colorData)
        self.calibration_state = calibration_state
        self.use_rgbd_tracking = bool(use_rgbd_tracking)
        self.native = None     # the native frame loop, once run_native has played frames
        self.frame_number = 0  # g_RGBDAdapter.getFrameNumber()
        self.trajectory = []   # the pose every processed frame was integrated at (recordTrajectory)
        self.frame_poses = []  # per frame read: the pose it was integrated at, or None (invalid, lost): for reintegrateCorrected
        self.recorded = None
        self.lost_frames = 0
        self.render_state = render_state
        self.renderer = self.phong = None
        if render_state is not None and render_state.s_renderToFile:
            self.renderer = E.RGBDRenderer(stream=stream)
            self.phong = E.PhongLighting(E.phong_light_from_render_state(render_state), stream=stream)
            self.render_color_intrinsics = adapter_color_intrinsics(h.m_colorIntrinsic[:], (max(h.m_colorWidth, 1), max(h.m_colorHeight, 1)),
                                                                    self.adapter_size)

    # -- the sensor side ------------------------------------------------------------------------------------------
    def _next_frame(self):
        """processDepth + loadNextSensFile (SensorDataReader.cpp:79-165)"""
        got = self.reader.processDepth()
        while got is None and self.file_idx + 1 < len(self.sens_files):
            self.file_idx += 1
            self.reader.close()
            self.reader = SD.SensorDataReader(self.sens_files[self.file_idx])
            got = self.reader.processDepth()
        return got

    def _record(self, depth, color):
        """recordFrame, RGBDSensor.cpp:275-323.  The reference stores JPEG colour; no encoder is built in, so the
        colour goes in raw (a reader of either side opens both)."""
        h = self.reader.header
        if self.recorded is None:
            self.recorded = SD.SensorData.create((h.m_depthWidth, h.m_depthHeight), (max(h.m_colorWidth, 1), max(h.m_colorHeight, 1)),
                                                 np.array(h.m_depthIntrinsic[:]), np.array(h.m_colorIntrinsic[:]), 1000.0,
                                                 bytes(h.m_sensorName).decode(), SD.TYPE_RAW, SD.TYPE_ZLIB_USHORT,
                                                 np.array(h.m_depthExtrinsic[:]), np.array(h.m_colorExtrinsic[:]))
        d = np.where(np.isfinite(depth), depth, 0.0).astype(np.float64)
        self.recorded.addFrame(color[..., :3], np.floor(1000.0 * d + 0.5).clip(0, 65535).astype(np.uint16))

    # -- reconstruction(), DepthSensing.cpp:720-924 ---------------------------------------------------------------
    def frame(self):
        """-> the camera-to-world pose the frame was integrated at, or None when the input is exhausted"""
        if self.native is not None:
            raise RuntimeError("this sequence is being played by the native loop (run_native)")
        got = self._next_frame()
        if got is None:
            return None
        depth, color = got
        pose = self._reconstruct(depth, color)
        if self.renderer is not None:
            self.renderToFile(depth, color)
        return pose

    def _reconstruct(self, depth, color):
        g = self.gas
        self.sensor.process(depth, color)
        self.frame_number += 1
        if g.s_recordData:
            self._record(depth, color)
        use_trajectory = bool(g.s_binaryDumpSensorUseTrajectory)
        only_init = bool(g.s_binaryDumpSensorUseTrajectoryOnlyInit)
        transformation = np.eye(4, dtype=np.float32)
        if use_trajectory:
            transformation = self.reader.getRigidTransform().reshape(4, 4)
            if transformation[0, 0] == MINF or np.isnan(transformation[0, 0]):
                return self._done(None)  # "INVALID FRAME"
        if self.frame_number > 1:
            render_transform = self.scene.getLastRigidTransform().reshape(4, 4)
            if use_trajectory and only_init:
                delta = np.linalg.inv(self.reader.getRigidTransform(-1).reshape(4, 4).astype(np.float64)).astype(np.float32) @ transformation
                render_transform = render_transform @ delta
                self.scene.setLastRigidTransformAndCompactify(render_transform, self.cp)
            self.ray.render(self.scene.getHashData(), self.scene.getHashParams(), self.cp, render_transform)
            if not g.s_trackingEnabled:
                transformation = np.eye(4, dtype=np.float32)
            elif use_trajectory and not only_init:
                pass  # the recorded pose is the pose
            else:
                a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
                check(self.L.vh_rgbd_sensor_get_maps(self.sensor.handle, C.byref(a), C.byref(b), C.byref(c)), "maps")
                rd = self.ray.getRayCastData()
                if self.tracker_rgbd is not None:
                    transformation, lost = self.tracker_rgbd.applyCT(a, b, self.sensor.getDepthCameraData().d_colorData, rd.d_depth4, rd.d_normals, rd.d_colors,
                                                                     self.scene.getLastRigidTransform(), self.tracking_rgbd, None, self.cp)
                else:
                    transformation, lost = self.tracker.applyCT(a, b, rd.d_depth4, rd.d_normals, self.scene.getLastRigidTransform(), self.tracking, None, self.cp)
                if lost:
                    self.lost_frames += 1
                    return self._done(None)  # "!!! TRACKING LOST !!!": the frame is not integrated
        if self.chunk_grid is not None:
            p = (transformation.reshape(4, 4) @ np.array(list(g.s_streamingPos) + [1.0], dtype=np.float32))[:3]
            if g.s_offlineProcessing:
                for _ in range(g.s_streamingOutParts):
                    self.chunk_grid.streamOutToCPUPass0GPU(p, g.s_streamingRadius, True, False)
                    self.chunk_grid.streamOutToCPUPass1CPU(False)
                self.chunk_grid.streamInToGPUAll(p, g.s_streamingRadius, True)
            else:
                self.chunk_grid.streamOutToCPU(p, g.s_streamingRadius, True)
                self.chunk_grid.streamInToGPU(p, g.s_streamingRadius, True)
        mask = self.chunk_grid.getBitMaskGPU() if self.chunk_grid is not None else None
        if g.s_integrationEnabled:
            self.scene.integrate(transformation, self.frame_data, self.cp, mask)
        else:
            self.scene.setLastRigidTransformAndCompactify(transformation, self.cp)
        return self._done(np.ascontiguousarray(transformation, dtype=np.float32).reshape(4, 4))

    def renderToFile(self, depth, color):
        """DSC/DepthSensing.cpp:1159-1255 for the frame just processed: one raster of the ray cast, shaded twice"""
        base = bytes(self.render_state.s_renderToFileDir).decode() or "."
        dirs = {k: os.path.join(base, k) for k in ("input_color", "input_depth", "reconstruction", "reconstruction_color")}
        for d in dirs.values():
            os.makedirs(d, exist_ok=True)
        last = self.scene.getLastRigidTransform()
        self.scene.setLastRigidTransformAndCompactify(last, self.cp)
        self.ray.render(self.scene.getHashData(), self.scene.getHashParams(), self.cp, last)
        rd, rp = self.ray.getRayCastData(), self.ray.getRayCastParams()
        W, H = self.adapter_size
        rs = self.render_state
        self.renderer.RenderDepthMap(rd.d_depth, rd.d_colors, rp.m_width, rp.m_height, np.array(rp.m_intrinsicsInverse[:], dtype=np.float32),
                                     np.eye(4, dtype=np.float32), self.render_color_intrinsics, W, H, rs.s_renderingDepthDiscontinuityThresOffset,
                                     rs.s_renderingDepthDiscontinuityThresLin)
        m = self.renderer.getMaps()
        name = "%06d.png" % self.frame_number
        for colored, sub in ((False, "reconstruction"), (True, "reconstruction_color")):
            self.phong.render(m["positions"], m["normals"], m["colors"], colored, W, H, rgba8=True)
            E.write_png_rgba8(os.path.join(dirs[sub], name), self.phong.download(rgba8=True))
        E.write_png_rgba8(os.path.join(dirs["input_color"], name), rgbx_alpha_rule(color))
        E.write_png_rgba8(os.path.join(dirs["input_depth"], name), depth_image_rgba8(depth))

    def _done(self, pose):
        self.frame_poses.append(pose if pose is not None and self.gas.s_integrationEnabled else None)
        if self.gas.s_recordData:
            self.trajectory.append(pose if pose is not None else np.full((4, 4), MINF, dtype=np.float32))
        elif pose is not None:
            self.trajectory.append(pose)
        return pose if pose is not None else np.full((4, 4), MINF, dtype=np.float32)

    def run(self, max_frames=None):
        """-> number of frames read"""
        n = 0
        while max_frames is None or n < max_frames:
            if self.frame() is None:
                break
            n += 1
        return n

    # -- the same sequence through the native frame loop ------------------------------------------------------------
    def prepare_native(self, batch=64, tracking=False, tracking_rgbd=False):
        """what run_native needs before its first frame: the native loop with the raw format of the first file, two sets of
        pinned buffers of `batch` frames, the file loaded.  run_native calls it; a caller that times the frames alone
        calls it first (the Python loop's reader loads its file in the constructor too)."""
        from .lib import PinnedArray
        if self.native is not None:
            return
        why = native_refusal(self.gas, self.render_state, self.camera_calibration, self.use_rgbd_tracking, tracking=tracking, tracking_rgbd=tracking_rgbd)
        if why is None and self.frame_number:
            why = "frames of this sequence have been played by the Python loop already"
        if why is not None:
            raise ValueError("run_native: " + why)
        g, h = self.gas, self.reader.header
        batch = max(int(batch), 1)
        has_color = h.m_colorWidth * h.m_colorHeight > 0
        opt = E.Reconstruction.defaultOptions(s_framesOnHost=1, s_streamingEnabled=1 if self.chunk_grid is not None else 0,
                                              s_integrationEnabled=1 if g.s_integrationEnabled else 0, s_offlineProcessing=1 if g.s_offlineProcessing else 0,
                                              s_streamingPos=list(g.s_streamingPos), s_streamingRadius=g.s_streamingRadius)
        native = E.Reconstruction(self.scene, self.ray, self.chunk_grid, self.cp, opt)
        native.setRawFormat((h.m_depthWidth, h.m_depthHeight), (h.m_colorWidth, h.m_colorHeight) if has_color else None, h.m_depthShift,
                            3 if has_color else 0, (g.s_depthSigmaD, g.s_depthSigmaR) if g.s_depthFilter else None,
                            (g.s_colorSigmaD, g.s_colorSigmaR) if g.s_colorFilter else None)
        self._native_sets = [(PinnedArray((batch, h.m_depthHeight, h.m_depthWidth), np.uint16),
                              PinnedArray((batch, h.m_colorHeight, h.m_colorWidth, 3), np.uint8) if has_color else None) for _ in range(2)]
        # the loop tracks where the Python loop would (_reconstruct): the file's poses are not used
        self._native_tracked = bool(tracking) and not g.s_binaryDumpSensorUseTrajectory
        if self._native_tracked and self.tracker_rgbd is not None:  # (as _reconstruct picks its tracker)
            native.setTrackingRGBD(self.tracking_rgbd)
        elif self._native_tracked:
            native.setTracking(self.tracking)
        self._native_sens = SD.SensorData.loadFromFile(self.sens_files[self.file_idx])
        self._native_at = 0
        self.native = native

    def run_native(self, max_frames=None, batch=64, tracking=False, tracking_rgbd=False):
        """Plays the `.sens` files through the native frame loop (engine.Reconstruction) fed with raw frames: a batch of
        frames is decoded into pinned memory (16-bit depth, RGB) while the device works on the batch before, and handed
        over with one call, the next frame's pose as look-ahead.  The device converts, resamples and filters them
        (vh_ingest_frame) as CUDARGBDSensor.process does for the Python loop.  For recorded poses, and with tracking=True
        for poses from the plain ICP tracker (s_binaryDumpSensorUseTrajectory = false: the loop tracks the camera itself,
        trajectory and lost_frames are filled as the Python loop fills them), with tracking_rgbd=True as well from the RGB-D
        tracker of a use_rgbd_tracking configuration; raises ValueError with the reason otherwise
        (native_refusal).  -> number of frames read"""
        h = self.reader.header
        batch = max(int(batch), 1)
        has_color = h.m_colorWidth * h.m_colorHeight > 0
        self.prepare_native(batch, tracking, tracking_rgbd)
        if self._native_sets[0][0].shape[0] < batch:
            raise ValueError("run_native: the batch size is fixed by the first call")

        def same_format(i):
            return ((i.m_depthWidth, i.m_depthHeight, i.m_colorWidth, i.m_colorHeight, i.m_depthShift) ==
                    (h.m_depthWidth, h.m_depthHeight, h.m_colorWidth, h.m_colorHeight, h.m_depthShift))

        def advance():
            """-> False when the input is exhausted (loadNextSensFile, SensorDataReader.cpp:147-165)"""
            while self._native_at >= self._native_sens.info().m_numFrames:
                if self.file_idx + 1 >= len(self.sens_files):
                    return False
                self.file_idx += 1
                self._native_sens.close()
                self._native_sens = SD.SensorData.loadFromFile(self.sens_files[self.file_idx])
                self._native_at = 0
                if not same_format(self._native_sens.info()):
                    raise ValueError("run_native: " + self.sens_files[self.file_idx] + " has another frame format than the first file")
            return True

        def decode(which, budget):
            """the next frames, at most a batch and `budget`, of the current file into buffer set `which` -> frame array or None"""
            if budget <= 0 or not advance():
                return None
            n = min(batch, budget, self._native_sens.info().m_numFrames - self._native_at)
            d, c = self._native_sets[which]
            _, _, poses = decode_batch(self._native_sens, self._native_at, n, d.array, c.array if c is not None else None)
            self._native_at += n
            ds, cs = d.array[0].nbytes, (c.array[0].nbytes if c is not None else 0)
            return poses, E.Reconstruction.makeRawFrames(list(poses) + [poses[-1]], [d.ptr + k * ds for k in range(n)] + [d.ptr],
                                                         [c.ptr + k * cs for k in range(n)] + [c.ptr] if c is not None else None)

        def peek_pose(budget):
            """the pose of the frame decode() would bring next, or None"""
            if budget <= 0 or not advance():
                return None
            pose = np.empty(16, dtype=np.float32)
            check(self.L.vh_sensor_data_get_frame(self._native_sens.handle, self._native_at, None, None, pose.ctypes.data_as(C.POINTER(C.c_float)), None),
                  "vh_sensor_data_get_frame")
            return pose

        read, which = 0, 0
        left = lambda: (max_frames - read) if max_frames is not None else batch
        cur = decode(which, left())
        while cur is not None:
            poses, frames = cur
            n = len(poses)
            read += n
            ahead = peek_pose(left())
            if ahead is not None:
                frames[n].rigidTransform[:] = [float(v) for v in ahead]
            self.native.runRaw(frames, 0, n, lookahead=ahead is not None)
            if self._native_tracked:  # the poses are the loop's own (the host has them when runRaw returns)
                for p in self.native.getPoses(self.frame_number, n):
                    if p[0, 0] == MINF:
                        self.lost_frames += 1
                    else:
                        self.trajectory.append(p.copy())
                poses = ()
            for p in poses:
                if not (p[0] == MINF or np.isnan(p[0])):
                    self.trajectory.append(p.reshape(4, 4).copy())
            self.frame_number += n
            which = 1 - which
            cur = decode(which, left())  # while the device works on the batch just handed over
            self.native.synchronize()    # whose buffers are free after this
        return read

    # -- around the loop ------------------------------------------------------------------------------------------
    def alignTo(self, other, guess=None, **options):
        """The rigid transform that lays this reconstruction's model onto `other`'s (not in the reference; DESIGN.md
        section 4 "Scene registration"): other.scene.alignScene(self.scene, guess) -> its result: "dst_from_src" (4x4,
        metres: a point of this world frame in other's) is an answer only where "converged".  Neither model is written.
        guess: a rough transform (odometry, a marker, an earlier session's pose; default the identity): the basin is a few
        voxels and a few degrees around it.  Blocks either chunk grid holds on the host are absent, as for every query.
        options: the fields of vhtypes.make_align_options.  A native loop of either side is synchronised first."""
        for r in (self, other):
            if r.native is not None:
                r.native.synchronize()
        return other.scene.alignScene(self.scene, guess, **options)

    def mergeFrom(self, other, block_offset=(0, 0, 0), transform=None, align=False, **align_options):
        """Fuses another reconstruction's model into this one (not in the reference; DESIGN.md section 4 "Scene merge"):
        the blocks resident in other's table (CUDASceneRepHashSDF.mergeScene) and, if other streams, the blocks its chunk
        grid holds on the host (downloadHostBlocks, upload, mergeBlocks), all shifted by whole blocks.  This scene must
        hold every block of its own on the device: stream everything in first (ValueError otherwise).  A native loop of
        either side is synchronised first.  -> [the counts of each merge]; compactify before the next ray cast.
        With transform (a rigid 4x4, metres: a point of other's world frame in this one's) other is resampled onto this
        scene's lattice instead (mergeSceneTransformed; DESIGN.md section 4 "Resampled merge"; the voxel sizes may differ by
        up to a factor of 2, block_offset must be zero).  Then other, too, must hold every block on the device
        (ValueError otherwise): a tap that crosses from a device block into a host block would read as unobserved.
        With align=True the transform (default the identity) is only a guess: it is refined first (other.alignTo(self,
        transform); DESIGN.md section 4 "Scene registration") and other is merged under the result, which is appended to
        the returned list under "align"; a registration that does not converge raises ValueError with nothing merged."""
        for r in (self, other):
            if r.native is not None:
                r.native.synchronize()
        if self.chunk_grid is not None and self.chunk_grid.getStatistics()["blocks"] != 0:
            raise ValueError("mergeFrom: the destination's chunk grid holds blocks on the host; stream them in first")
        if align and transform is None:
            transform = np.eye(4)
        if transform is not None:
            if tuple(int(v) for v in block_offset) != (0, 0, 0):
                raise ValueError("mergeFrom: a transform and a block offset exclude each other; put the shift into the transform")
            if other.chunk_grid is not None and other.chunk_grid.getStatistics()["blocks"] != 0:
                raise ValueError("mergeFrom: with a transform the source's chunk grid must hold no blocks on the host; stream them in first")
            if align:
                found = self.scene.alignScene(other.scene, transform, **align_options)
                if not found["converged"]:
                    raise ValueError(f"mergeFrom: the registration did not converge (status {found['status']}, {found['iterations']} steps); nothing was merged")
                return [self.scene.mergeSceneTransformed(other.scene, found["dst_from_src"]), {"align": found}]
            return [self.scene.mergeSceneTransformed(other.scene, transform)]
        out = [self.scene.mergeScene(other.scene, block_offset)]
        if other.chunk_grid is not None:
            descs, blocks = other.chunk_grid.downloadHostBlocks()
            if len(descs):
                out.append(self.scene.mergeBlocks(descs, blocks, block_offset))
        return out

    def _before_cut(self, what, modifies, others=()):
        for r in (self,) + tuple(others):
            if r.native is not None:
                r.native.synchronize()
        if modifies and self.chunk_grid is not None and self.chunk_grid.getStatistics()["blocks"] != 0:
            raise ValueError(f"{what}: the chunk grid holds blocks on the host; stream them in first")

    def eraseRegion(self, region):
        """Takes the voxels inside a region (vhtypes.make_cut_region: a box or an ellipsoid in the world) out of the
        model (not in the reference; DESIGN.md section 4 "Scene cut"; CUDASceneRepHashSDF.eraseRegion) -> the counts.
        This scene must hold every block on the device: stream everything in first (ValueError otherwise).  A native
        loop is synchronised first; compactify before the next ray cast."""
        self._before_cut("eraseRegion", True)
        return self.scene.eraseRegion(region)

    def cropToRegion(self, region):
        """eraseRegion of everything that is not inside the region: what is left is the region's content"""
        self._before_cut("cropToRegion", True)
        return self.scene.cropToRegion(region)

    def extractRegion(self, region):
        """Copies a region out and leaves the model as it is -> [the block lists, each a dict with "descs", "voxels" and
        the counts]: the one of the blocks resident on the device (CUDASceneRepHashSDF.extractRegion) and, if this scene
        streams and its chunk grid holds blocks on the host, the one of those (downloadHostBlocks through vh_cut_blocks'
        list form).  A block is on the device or on the host, never both: the lists name no position twice."""
        self._before_cut("extractRegion", False)
        out = [self.scene.extractRegion(region)]
        if self.chunk_grid is not None:
            descs, blocks = self.chunk_grid.downloadHostBlocks()
            if len(descs):
                m = E.cut_region_transform(list(region.worldFromRegion), list(region.halfExtents), self.scene.getHashParams().m_virtualVoxelSize)
                out.append(E.extract_from_block_list(descs, blocks, m, region.shape, stream=self.scene.stream))
        return out

    def moveRegionTo(self, other, region, block_offset=(0, 0, 0)):
        """Moves a region's voxels into another reconstruction's model, shifted by whole blocks
        (CUDASceneRepHashSDF.moveRegionTo: nothing is erased here unless everything arrived there) -> the counts.  Both
        scenes must hold every block on the device (ValueError otherwise)."""
        self._before_cut("moveRegionTo", True, (other,))
        if other.chunk_grid is not None and other.chunk_grid.getStatistics()["blocks"] != 0:
            raise ValueError("moveRegionTo: the destination's chunk grid holds blocks on the host; stream them in first")
        return self.scene.moveRegionTo(other.scene, region, block_offset)

    def deintegrateFrame(self, depth, color, pose):
        """Takes a frame back out of the model (not in the reference; DESIGN.md section 4 "Frame de-integration";
        CUDASceneRepHashSDF.deintegrate) -> the counts.  depth, color: the frame as the reader gave it when it was
        integrated at `pose`; it goes through the sensor's pre-processing again, so that the maps are the ones that
        were integrated (the sensor's maps hold this frame afterwards).  This scene must hold every block on the device:
        stream everything in first (ValueError otherwise).  A native loop is synchronised first; compactify before the
        next ray cast.  The take-out is the inverse below the weight cap and without a starve pass in between."""
        self._before_cut("deintegrateFrame", True)
        self.sensor.process(depth, color)
        return self.scene.deintegrate(pose, self.frame_data, self.cp)

    def reintegrateFrame(self, depth, color, old_pose, new_pose):
        """deintegrateFrame at old_pose, then the frame integrated again at new_pose (CUDASceneRepHashSDF.reintegrate;
        counts as a frame) -> the take-out's counts"""
        self._before_cut("reintegrateFrame", True)
        self.sensor.process(depth, color)
        return self.scene.reintegrate(old_pose, new_pose, self.frame_data, self.cp)

    def reintegrateCorrected(self, corrected_poses):
        """A second pass over the recording with a corrected trajectory (one 4x4 camera-to-world pose per frame read, in
        order): every frame that was integrated and whose corrected pose differs from the pose it went in at is taken
        out and integrated again at the corrected one (reintegrateFrame) -> dict(frames, reintegrated, voxels_changed,
        voxels_reset, voxels_at_cap, blocks_freed).  For a sequence played by the Python loop without streaming
        (ValueError otherwise)."""
        if self.native is not None:
            raise ValueError("reintegrateCorrected: this sequence was played by the native loop")
        if self.chunk_grid is not None:
            raise ValueError("reintegrateCorrected: not with streaming")
        corrected = np.asarray(corrected_poses, dtype=np.float32).reshape(-1, 4, 4)
        out = dict(frames=len(self.frame_poses), reintegrated=0, voxels_changed=0, voxels_reset=0, voxels_at_cap=0, blocks_freed=0)
        files = iter(self.sens_files)
        reader = SD.SensorDataReader(next(files))
        try:
            for i, pose in enumerate(self.frame_poses):
                got = reader.processDepth()
                while got is None:
                    reader.close()
                    reader = SD.SensorDataReader(next(files))
                    got = reader.processDepth()
                if pose is None or i >= len(corrected) or np.array_equal(corrected[i], np.asarray(pose, np.float32).reshape(4, 4)):
                    continue
                c = self.reintegrateFrame(got[0], got[1], pose, corrected[i])
                self.frame_poses[i] = corrected[i].copy()
                out["reintegrated"] += 1
                out["blocks_freed"] += c["freed"]
                for k in ("voxels_changed", "voxels_reset", "voxels_at_cap"):
                    out[k] += c[k]
        finally:
            reader.close()
        return out

    def saveRecordedFramesToFile(self, filename=None):
        """RGBDSensor.cpp:339-389: poses from the run, time stamps and IMU records from the input"""
        if self.recorded is None:
            return None
        filename = filename or bytes(self.gas.s_recordDataFile).decode()
        d = os.path.dirname(filename)
        if d:
            os.makedirs(d, exist_ok=True)
        n = self.recorded.info().m_numFrames
        if n != len(self.trajectory):
            raise RuntimeError("num frames and trajectory size doesn't match")
        src = SD.SensorData.loadFromFile(self.sens_files[0]) if len(self.sens_files) == 1 else None
        out = SD.SensorData.create(*self._recorded_header())
        for i in range(n):
            f = self.recorded.frame(i)
            ts = src.frame(i, depth=False, color=False)["timeStamps"] if src is not None and i < src.info().m_numFrames else (0, 0)
            out.addFrame(f["color"], f["depth"], self.trajectory[i], ts[0], ts[1])
        out.saveToFile(filename)
        return filename

    def _recorded_header(self):
        h = self.recorded.info()
        return ((h.m_depthWidth, h.m_depthHeight), (h.m_colorWidth, h.m_colorHeight), np.array(h.m_depthIntrinsic[:]), np.array(h.m_colorIntrinsic[:]),
                h.m_depthShift, bytes(h.m_sensorName).decode(), h.m_colorCompressionType, h.m_depthCompressionType,
                np.array(h.m_depthExtrinsic[:]), np.array(h.m_colorExtrinsic[:]))

    # -- live mesh (not in the reference; DESIGN.md section 4 "Live mesh") --------------------------------------------
    def _live_check(self, what):
        if self.chunk_grid is not None:
            raise ValueError(f"{what}: not with streaming (a live mesh is of what is resident; the chunk-grid walk is not covered)")
        if self.native is not None:  # frames the native loop still has in flight, as deintegrateFrame treats them
            self.native.synchronize()
        if self.scene.frameInFlight():  # the model is about to change under an update: refused, as a de-integration is
            raise ValueError(f"{what}: a frame is in flight (between integrateAhead and integrateFinish)")

    def liveMeshBegin(self):
        """Starts a live mesh on an extractor of its own (live_marching_cubes): liveMeshUpdate then brings it up to date
        with the model at the cost of what changed, and liveMesh reads it.  ValueError with streaming on."""
        self._live_check("liveMeshBegin")
        if self.live_marching_cubes is None:
            self.live_marching_cubes = E.CUDAMarchingCubesHashSDF(self.mp)
        else:
            self.live_marching_cubes.liveEnd()
        self.live_marching_cubes.liveBegin()

    def liveMeshUpdate(self):
        """One update of the live mesh (CUDAMarchingCubesHashSDF.liveUpdate) -> its counts.  A native loop is
        synchronised first.  ValueError, with the cache as it was, without liveMeshBegin, with streaming on and with a
        frame in flight (the scene between integrateAhead and integrateFinish)."""
        self._live_check("liveMeshUpdate")
        if self.live_marching_cubes is None:
            raise ValueError("liveMeshUpdate: no liveMeshBegin")
        return self.live_marching_cubes.liveUpdate(self.scene.getHashData(), self.scene.getHashParams())

    def liveMesh(self, filename=None, normals=False, min_component_faces=0, largest_component=False, cluster_cells=0, smooth_iterations=0,
                 smooth_lambda=0.5, smooth_mu=-0.53, keep_boundary=True):
        """The live mesh as it stands after the last update, welded on the device and through the indexed passes asked
        for (as extractIsoSurface(indexed=True) describes them) -> the mesh; written as a PLY when a file name is given"""
        if self.live_marching_cubes is None:
            raise ValueError("liveMesh: no liveMeshBegin")
        mc = self.live_marching_cubes
        mc.setIndexedNormals(bool(normals))
        mc.setIndexedComponentFilter(int(min_component_faces), bool(largest_component))
        mc.setIndexedClustering(int(cluster_cells))
        mc.setIndexedSmoothing(int(smooth_iterations), smooth_lambda, smooth_mu, bool(keep_boundary))
        mc.liveIndexed()
        mesh = mc.mesh()
        if min_component_faces or largest_component:
            mesh["components"] = mc.indexed_component_stats()
        if cluster_cells:
            mesh["clustering"] = mc.indexed_cluster_stats()
        if smooth_iterations:
            mesh["smoothing"] = mc.indexed_smooth_stats()
        if filename:
            mc.saveMesh(filename, None, True)
        return mesh

    def extractIsoSurface(self, filename=None, indexed=False, normals=False, min_component_faces=0, largest_component=False, cluster_cells=0,
                          smooth_iterations=0, smooth_lambda=0.5, smooth_mu=-0.53, keep_boundary=True):
        """StopScanningAndExtractIsoSurfaceMC: marching cubes over the whole scene (through the chunk grid when
        streaming is on) -> (vertices, colours, faces); written as a PLY when a file name is given.  indexed (not in the
        reference): weld the triangles on the device instead of merging them on the host.  With streaming on that is
        refused here before any GPU work: extractIsoSurfaceIndexed() is the indexed extraction that also walks the
        chunk grid.  normals (with indexed): vertex normals computed on the device after the weld, returned as
        "normals" and written into the PLY.  min_component_faces, largest_component (with indexed): the mesh's
        connected components are labelled on the device after the weld and those of fewer faces dropped, or all but the
        largest; what is returned and written is the filtered mesh, and its "components" entry (indexed_component_stats)
        says what the unfiltered one held.  cluster_cells (with indexed; 1 ... 64): the welded mesh is decimated on the
        device by vertex clustering -- the vertices in one cube of that many lattice points a side become one -- before
        the normals and the filter; what is returned and written is the clustered mesh, and its "clustering" entry
        (indexed_cluster_stats) says what the pass did.  smooth_iterations (with indexed; 1 ... 100), smooth_lambda,
        smooth_mu, keep_boundary: that many iterations of Taubin smoothing in fixed point on the device, after the
        clustering and before the normals and the filter; what is returned and written carries the smoothed positions,
        and its "smoothing" entry (indexed_smooth_stats) says what the pass did."""
        if smooth_iterations and not indexed:
            raise ValueError("smoothing needs the indexed extraction: a triangle soup has no neighbours")
        if cluster_cells and not indexed:
            raise ValueError("clustering needs the indexed extraction: it works on the welded mesh's vertex keys")
        if (min_component_faces or largest_component) and not indexed:
            raise ValueError("the component filter needs the indexed extraction: a triangle soup has no connectivity")
        if normals and not indexed:
            raise ValueError("vertex normals need the indexed extraction: only the welded mesh has vertices that faces share")
        if indexed and self.chunk_grid is not None:
            raise ValueError("indexed extraction is not available with streaming enabled (the chunk grid extracts per chunk)")
        if self.marching_cubes is None:
            self.marching_cubes = E.CUDAMarchingCubesHashSDF(self.mp)
            # offline: every batch is merged and de-duplicated as it arrives; otherwise the buffer holds the triangle
            # soup (three vertices per triangle, no indices) until saveMesh merges it (.cpp:31-86)
            self.marching_cubes.setOfflineProcessing(bool(self.gas.s_offlineProcessing))
        mc = self.marching_cubes
        mc.clearMeshBuffer()
        mc.setIndexedNormals(bool(normals))
        mc.setIndexedComponentFilter(int(min_component_faces), bool(largest_component))
        mc.setIndexedClustering(int(cluster_cells))
        mc.setIndexedSmoothing(int(smooth_iterations), smooth_lambda, smooth_mu, bool(keep_boundary))
        if self.chunk_grid is not None:
            pos = (self.scene.getLastRigidTransform().reshape(4, 4) @ np.array(list(self.gas.s_streamingPos) + [1.0], dtype=np.float32))[:3]
            mc.extractIsoSurfaceChunkGrid(self.chunk_grid, pos, self.gas.s_streamingRadius)
        elif indexed:
            mc.extractIsoSurfaceIndexed(self.scene.getHashData(), self.scene.getHashParams())
        else:
            mc.extractIsoSurface(self.scene.getHashData(), self.scene.getHashParams())
        mesh = mc.mesh()
        if min_component_faces or largest_component:
            mesh["components"] = mc.indexed_component_stats()  # (saveMesh clears them with the buffer)
        if cluster_cells:
            mesh["clustering"] = mc.indexed_cluster_stats()
        if smooth_iterations:
            mesh["smoothing"] = mc.indexed_smooth_stats()
        if filename:
            mc.saveMesh(filename, None, True)  # merges close vertices, writes the PLY and clears the buffer (.cpp:126-144)
        return mesh

    def extractIsoSurfaceIndexed(self, filename=None, normals=False, min_component_faces=0, largest_component=False, cluster_cells=0,
                                 smooth_iterations=0, smooth_lambda=0.5, smooth_mu=-0.53, keep_boundary=True):
        """The indexed extraction with and without streaming (not in the reference): marching cubes with the triangles
        welded on the device -> (vertices, colours, faces); written as a PLY when a file name is given.  Without
        streaming this is extractIsoSurface(indexed=True); with streaming it walks the chunk grid as extractIsoSurface()
        does and welds every chunk's triangles into one mesh (the overlap of the chunks' boxes is taken once), so
        nothing is merged on the host.  marching_cubes.indexed() has the mesh with its keys, indexed_stats() the counts.
        normals: vertex normals computed on the device over the finished mesh, returned as "normals" and written into
        the PLY.  min_component_faces, largest_component: the component filter, over the finished mesh (a component
        spans chunks), as extractIsoSurface describes it.  cluster_cells: the vertex clustering, over the finished mesh
        too, before the other two.  smooth_iterations, smooth_lambda, smooth_mu, keep_boundary: the Taubin smoothing,
        over the finished mesh after the clustering and before the other two."""
        if self.chunk_grid is None:
            return self.extractIsoSurface(filename, indexed=True, normals=normals, min_component_faces=min_component_faces, largest_component=largest_component,
                                          cluster_cells=cluster_cells, smooth_iterations=smooth_iterations, smooth_lambda=smooth_lambda, smooth_mu=smooth_mu,
                                          keep_boundary=keep_boundary)
        if self.marching_cubes is None:
            self.marching_cubes = E.CUDAMarchingCubesHashSDF(self.mp)
            self.marching_cubes.setOfflineProcessing(bool(self.gas.s_offlineProcessing))
        mc = self.marching_cubes
        mc.setIndexedNormals(bool(normals))
        mc.setIndexedComponentFilter(int(min_component_faces), bool(largest_component))
        mc.setIndexedClustering(int(cluster_cells))
        mc.setIndexedSmoothing(int(smooth_iterations), smooth_lambda, smooth_mu, bool(keep_boundary))
        pos = (self.scene.getLastRigidTransform().reshape(4, 4) @ np.array(list(self.gas.s_streamingPos) + [1.0], dtype=np.float32))[:3]
        mc.extractIsoSurfaceIndexedChunkGrid(self.chunk_grid, pos, self.gas.s_streamingRadius)
        mesh = mc.mesh()
        if min_component_faces or largest_component:
            mesh["components"] = mc.indexed_component_stats()  # (saveMesh clears them with the buffer)
        if cluster_cells:
            mesh["clustering"] = mc.indexed_cluster_stats()
        if smooth_iterations:
            mesh["smoothing"] = mc.indexed_smooth_stats()
        if filename:
            mc.saveMesh(filename, None, True)  # the mesh is welded: written as it is, and the buffer cleared
        return mesh
