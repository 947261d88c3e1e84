"""The native frame loop: Reconstruction, reconstruction() of DepthSensingCUDA/Source/DepthSensing.cpp:720-924 behind
the C ABI."""
import ctypes as C

import numpy as np

from .. import vhtypes as T
from ..lib import check, load
from ._common import _Handle, _copy_struct


class Reconstruction(_Handle):
    """The frame loop reconstruction() (DepthSensingCUDA/Source/DepthSensing.cpp:720-924) for a recorded sequence at
    given poses, native behind the C ABI: run() enqueues any number of frames with one call."""

    _destroy = "vh_reconstruction_destroy"

    def __init__(self, sceneRep, rayCast, chunkGrid, depthCameraParams, options=None):
        self.scene, self.ray, self.grid = sceneRep, rayCast, chunkGrid  # kept alive as long as the loop
        self._cp = _copy_struct(depthCameraParams)
        self._options = _copy_struct(options) if options is not None else self.defaultOptions()
        self._create("vh_reconstruction_create", sceneRep.handle, rayCast.handle if rayCast is not None else None,
                     chunkGrid.handle if chunkGrid is not None else None, C.byref(self._cp), C.byref(self._options))

    @staticmethod
    def defaultOptions(**overrides):
        o = T.ReconstructionOptions()
        load().vh_reconstruction_default_options(C.byref(o))
        for k, v in overrides.items():
            if k in ("s_streamingPos",):
                o.s_streamingPos[:] = [float(x) for x in v]
            else:
                setattr(o, k, v)
        return o

    @staticmethod
    def _frames(ctype, poses, depth_ptrs, color_ptrs):
        n = len(poses)
        arr = (ctype * n)()
        for k in range(n):
            arr[k].rigidTransform[:] = [float(v) for v in np.asarray(poses[k], dtype=np.float32).reshape(-1)]
            arr[k].depth = depth_ptrs[k]
            arr[k].color = color_ptrs[k] if color_ptrs is not None else None
        return arr

    def _run(self, ctype, run, run_ahead, what, frames, first, count, lookahead):
        """frames[first:first+count], an array of `ctype`, through L.<run>, or L.<run_ahead> with the frame behind them"""
        n = len(frames) - first if count is None else count
        if n <= 0:
            return
        ptr = C.cast(C.byref(frames, first * C.sizeof(ctype)), C.POINTER(ctype))
        if lookahead and first + n < len(frames):
            nxt = C.cast(C.byref(frames, (first + n) * C.sizeof(ctype)), C.POINTER(ctype))
            check(getattr(self.L, run_ahead)(self.handle, ptr, n, nxt), what)
        else:
            check(getattr(self.L, run)(self.handle, ptr, n), what)

    @staticmethod
    def makeFrames(poses, depth_ptrs, color_ptrs):
        """-> ctypes array of VhSequenceFrame (device pointers, or host pointers for s_framesOnHost)"""
        return Reconstruction._frames(T.SequenceFrame, poses, depth_ptrs, color_ptrs)

    def run(self, frames, first=0, count=None, lookahead=False):
        """frames: a VhSequenceFrame array (makeFrames); processes frames[first:first+count].  lookahead: the loop may
        read the pose of frames[first+count], the frame a later call will bring (vh_reconstruction_run_ahead)"""
        self._run(T.SequenceFrame, "vh_reconstruction_run", "vh_reconstruction_run_ahead", "Reconstruction::run", frames, first, count, lookahead)

    # ---- raw frames: 16-bit depth + 8-bit colour at the sensor's sizes -------------------------------------------
    def setRawFormat(self, depth_size, color_size=None, depth_shift=1000.0, color_channels=3, depth_filter=None, color_filter=None):
        """Once, before the first frame.  depth_size / color_size: (width, height) of the sensor's images;
        color_channels: 3 (RGB), 4 (RGBX) or 0 (no colour); depth_filter / color_filter: None, or (sigmaD, sigmaR) of the
        Gauss filter CUDARGBDSensor::process applies (s_depthFilter / s_colorFilter of the parameter file)"""
        f = T.RawFrameFormat()
        f.depthWidth, f.depthHeight = int(depth_size[0]), int(depth_size[1])
        if color_size is not None:
            f.colorWidth, f.colorHeight = int(color_size[0]), int(color_size[1])
        f.depthShift = depth_shift
        f.colorChannels = int(color_channels)
        if depth_filter is not None:
            f.s_depthFilter, (f.s_depthSigmaD, f.s_depthSigmaR) = 1, depth_filter
        if color_filter is not None:
            f.s_colorFilter, (f.s_colorSigmaD, f.s_colorSigmaR) = 1, color_filter
        check(self.L.vh_reconstruction_set_raw_format(self.handle, C.byref(f)), "Reconstruction::setRawFormat")
        self._raw_format = f

    @staticmethod
    def makeRawFrames(poses, depth_ptrs, color_ptrs):
        """-> ctypes array of VhRawSequenceFrame (host pointers for s_framesOnHost, else device pointers)"""
        return Reconstruction._frames(T.RawSequenceFrame, poses, depth_ptrs, color_ptrs)

    def runRaw(self, frames, first=0, count=None, lookahead=False):
        """run() for a VhRawSequenceFrame array (makeRawFrames); needs setRawFormat"""
        self._run(T.RawSequenceFrame, "vh_reconstruction_run_raw", "vh_reconstruction_run_raw_ahead", "Reconstruction::runRaw", frames, first, count, lookahead)

    # ---- camera tracking inside the loop ----------------------------------------------------------------------------
    def setTracking(self, tracking_state):
        """Once, before the first frame: from then on run() / runRaw() ignore the frames' poses; every frame after the first
        is aligned to the ray cast of the model by projective ICP (tracking_state: a TrackingState) and integrated at
        lastRigidTransform * delta, a frame on which tracking is lost is not integrated.  Needs a ray caster."""
        check(self.L.vh_reconstruction_set_tracking(self.handle, C.byref(tracking_state)), "Reconstruction::setTracking")

    def setTrackingRGBD(self, tracking_state_rgbd):
        """setTracking with the RGB-D tracker (depth + photometric ICP; tracking_state_rgbd: a TrackingStateRGBD) in place
        of the plain one: one of the two, once.  Every frame then needs a colour map."""
        check(self.L.vh_reconstruction_set_tracking_rgbd(self.handle, C.byref(tracking_state_rgbd)), "Reconstruction::setTrackingRGBD")

    def getPoses(self, first=0, count=None):
        """-> [count, 4, 4] float32: the pose each frame fed since creation / reset was integrated at, all -inf for a frame
        that was not (tracking lost, invalid recorded pose).  count=None: up to the last frame fed (asks getStats)."""
        if count is None:
            st = self.getStats()
            count = st["frames"] + st["invalidFrames"] + st["lostFrames"] - first
        out = np.empty((max(int(count), 0), 4, 4), dtype=np.float32)
        if len(out):
            check(self.L.vh_reconstruction_get_poses(self.handle, int(first), len(out), out.ctypes.data_as(C.POINTER(C.c_float))), "Reconstruction::getPoses")
        return out

    def synchronize(self):
        check(self.L.vh_reconstruction_synchronize(self.handle), "Reconstruction::synchronize")

    def reset(self):
        check(self.L.vh_reconstruction_reset(self.handle), "Reconstruction::reset")

    def debugFailRender(self, nth_render_from_now):
        check(self.L.vh_reconstruction_debug_fail_render(self.handle, int(nth_render_from_now)), "Reconstruction::debugFailRender")

    def getStats(self):
        st = T.ReconstructionStats()
        check(self.L.vh_reconstruction_get_stats(self.handle, C.byref(st)), "Reconstruction::getStats")
        out = {k: getattr(st, k) for k, _ in T.ReconstructionStats._fields_}
        out["trackedFrames"], out["lostFrames"] = self.getTrackingStats()
        return out

    def getTrackingStats(self):
        """-> (trackedFrames, lostFrames): frames integrated at a pose the loop tracked itself, frames on which tracking was
        lost; both 0 without setTracking.  Waits for nothing."""
        a, b = C.c_uint64(), C.c_uint64()
        check(self.L.vh_reconstruction_get_tracking_stats(self.handle, C.byref(a), C.byref(b)), "Reconstruction::getTrackingStats")
        return a.value, b.value
