#!/usr/bin/env python3
"""Plays `.sens` sequences through the frame loop the way the reference application does (parameter file, tracking
parameter file, optional mesh at the end) and prints one JSON line with the timing.

    python tools/replay.py --params zParameters.txt [--tracking zParametersTracking.txt] [--rgbd-tracking] [--sens a.sens b.sens]
                           [--mesh scan.ply [--indexed-mesh [--mesh-normals] [--mesh-min-component N] [--mesh-largest-component] [--mesh-cluster M]
                           [--mesh-smooth N [--mesh-smooth-lambda L] [--mesh-smooth-mu M] [--mesh-smooth-free-boundary]] [--live-mesh-every N]]] [--max-frames N] [--record out.sens] [--render-to DIR] [--camera-calibration]
                           [--native [--batch N] [--native-tracking]] [--weighted-colour]
                           [--crop-box CX CY CZ HX HY HZ [RX RY RZ]] [--erase-box CX CY CZ HX HY HZ [RX RY RZ]]
                           [--corrected-trajectory FILE]

Without --sens the files named by s_binaryDumpSensorFile[i] in the parameter file are played.  The rendering keys
(light, material, discontinuity thresholds, s_renderToFile, s_renderToFileDir) come from --params; --render-to switches
s_renderToFile on and writes the images under DIR.  The camera-calibration keys (s_bUseCameraCalibration and the
remapping thresholds) come from --params too; --camera-calibration switches s_bUseCameraCalibration on, so the depth
map is rendered into the colour camera with the `.sens` file's extrinsic (unless that is the identity).

--native plays the files through the native frame loop fed with raw frames (Reconstruction.run_native): batches of
16-bit depth + RGB frames decoded into pinned memory, converted, resampled and filtered on the device, no host wait per
frame.  It is for recorded poses (s_binaryDumpSensorUseTrajectory = true, ...OnlyInit = false) and says why when the
configuration needs the Python loop (ICP tracking, --record, --render-to, camera calibration).  With --native-tracking the
native loop tracks the camera itself where the parameter file asks for it (s_binaryDumpSensorUseTrajectory = false): one
host wait per frame, for the pose; with plain projective ICP, or with --rgbd-tracking with the RGB-D tracker.

--weighted-colour fuses colours weighted by the voxel weights (CUDASceneRepHashSDF::setColorIntegration) instead of the
reference's running 50/50 average, in either loop: what the RGB-D tracker needs to follow its own reconstruction.  It is
not a key of the parameter file; the JSON line names the rule as "colour_rule".

--erase-box takes a box out of the model after the last frame and before --mesh (Reconstruction.eraseRegion), --crop-box
everything but a box (cropToRegion): the centre and the half extents in metres and, optionally, a rotation vector in
radians (axis times angle) that turns the box's axes.  The erase runs first when both are given.  With s_streamingEnabled
the blocks on the host must be streamed in first: the tool says so and stops.  The JSON line has the counts as "cut".

--corrected-trajectory FILE: FILE holds one camera-to-world pose per frame as text, 16 numbers per line (4x4, row-major).
After the replay a second pass over the recording takes every frame whose corrected pose differs from the pose it went in
at back out of the model and integrates it again at the corrected one (Reconstruction.reintegrateCorrected; DESIGN.md
section 4 "Frame de-integration" has what the take-out is worth), before any cut, mesh or record.  Not with
s_streamingEnabled and not with --native.  The JSON line has the tally as "reintegrated"."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def box_region(values):
    """centre, half extents and an optional rotation vector (Rodrigues) -> vhtypes.CutRegion"""
    import numpy as np
    from voxelhashing_amd import vhtypes as T
    R = np.eye(3)
    if len(values) == 9:
        w = np.asarray(values[6:9], np.float64)
        th = float(np.linalg.norm(w))
        if th > 0.0:
            k = w / th
            K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
            R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    return T.make_cut_region(values[0:3], values[3:6], R, T.CUT_BOX)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", required=True)
    ap.add_argument("--tracking", default=None)
    ap.add_argument("--rgbd-tracking", action="store_true", help="track with depth + colour (CUDACameraTrackingMultiResRGBD) instead of depth alone")
    ap.add_argument("--sens", nargs="*", default=None)
    ap.add_argument("--mesh", default=None)
    ap.add_argument("--indexed-mesh", action="store_true", help="--mesh: weld the triangles on the device instead of merging them on the host; with s_streamingEnabled the chunks' triangles are welded into one mesh as the chunk grid is walked")
    ap.add_argument("--mesh-normals", action="store_true", help="--indexed-mesh: compute vertex normals on the device after the weld and write nx, ny, nz into the PLY")
    ap.add_argument("--mesh-min-component", type=int, default=0, metavar="N", help="--indexed-mesh: drop the connected components of fewer than N faces on the device before the mesh is written")
    ap.add_argument("--mesh-largest-component", action="store_true", help="--indexed-mesh: keep only the connected component with the most faces")
    ap.add_argument("--mesh-cluster", type=int, default=0, metavar="M", help="--indexed-mesh: decimate the mesh on the device before it is written: the vertices in one cube of M (2 ... 64) voxel-lattice points a side become one")
    ap.add_argument("--mesh-smooth", type=int, default=None, metavar="N", help="--indexed-mesh: N (1 ... 100) iterations of Taubin smoothing on the device, after the clustering and before the normals")
    ap.add_argument("--mesh-smooth-lambda", type=float, default=0.5, metavar="L", help="--mesh-smooth: the shrinking factor (0.5)")
    ap.add_argument("--mesh-smooth-mu", type=float, default=-0.53, metavar="M", help="--mesh-smooth: the inflating factor (-0.53)")
    ap.add_argument("--mesh-smooth-free-boundary", action="store_true", help="--mesh-smooth: move the vertices of the mesh's open boundary too")
    ap.add_argument("--live-mesh-every", type=int, default=0, metavar="N", help="--mesh --indexed-mesh: keep a live mesh, update it every N frames at the cost of what the frames changed, and write the final mesh from it")
    ap.add_argument("--record", default=None, help="write what was processed, with the poses used, to this .sens file")
    ap.add_argument("--max-frames", type=int, default=None)
    ap.add_argument("--render-to", default=None, help="renderToFile: the shaded model and the input of every frame as PNGs under this directory")
    ap.add_argument("--camera-calibration", action="store_true", help="s_bUseCameraCalibration: remap depth into the colour camera")
    ap.add_argument("--native", action="store_true", help="play through the native frame loop, fed with raw frames")
    ap.add_argument("--batch", type=int, default=64, help="--native: frames decoded and handed over per call")
    ap.add_argument("--native-tracking", action="store_true", help="--native: let the native loop track the camera (plain ICP, or RGB-D ICP with --rgbd-tracking) when the poses are not recorded")
    ap.add_argument("--crop-box", type=float, nargs="+", default=None, metavar="V", help="keep only a box of the model before --mesh: centre x y z, half extents x y z (metres) and optionally a rotation vector (radians)")
    ap.add_argument("--erase-box", type=float, nargs="+", default=None, metavar="V", help="take a box out of the model before --mesh: centre, half extents and optionally a rotation vector, as --crop-box")
    ap.add_argument("--corrected-trajectory", default=None, metavar="FILE", help="after the replay, re-integrate every frame whose pose in FILE (one 4x4 row-major pose per frame, 16 numbers per line) differs from the pose it went in at")
    ap.add_argument("--weighted-colour", action="store_true", help="fuse colours weighted by the voxel weights instead of the reference's running 50/50 average")
    args = ap.parse_args()
    if args.mesh_normals and not args.indexed_mesh:
        ap.error("--mesh-normals needs --indexed-mesh: only the welded mesh has vertices that faces share")
    if args.mesh_min_component and not args.indexed_mesh:
        ap.error("--mesh-min-component needs --indexed-mesh: a triangle soup has no connectivity")
    if args.mesh_largest_component and not args.indexed_mesh:
        ap.error("--mesh-largest-component needs --indexed-mesh: a triangle soup has no connectivity")
    if args.mesh_cluster and not args.indexed_mesh:
        ap.error("--mesh-cluster needs --indexed-mesh: clustering works on the welded mesh's vertex keys")
    if args.mesh_cluster and not 2 <= args.mesh_cluster <= 64:
        ap.error("--mesh-cluster: 2 ... 64 lattice points a side")
    if args.mesh_smooth is not None and not args.indexed_mesh:
        ap.error("--mesh-smooth needs --indexed-mesh: a triangle soup has no neighbours")
    if args.mesh_smooth is not None and not 1 <= args.mesh_smooth <= 100:
        ap.error("--mesh-smooth: 1 ... 100 iterations")
    args.mesh_smooth = args.mesh_smooth or 0  # (not given: off)
    if not (abs(args.mesh_smooth_lambda) <= 1.0 and abs(args.mesh_smooth_mu) <= 1.0):
        ap.error("--mesh-smooth-lambda, --mesh-smooth-mu: factors in [-1, 1]")
    if args.mesh_min_component < 0:
        ap.error("--mesh-min-component: a number of faces")
    for name, box in (("--crop-box", args.crop_box), ("--erase-box", args.erase_box)):
        if box is not None and (len(box) not in (6, 9) or not all(h > 0 for h in box[3:6])):
            ap.error(name + ": centre x y z, half extents x y z (> 0) and optionally a rotation vector x y z")
    if args.live_mesh_every < 0 or (args.live_mesh_every and not (args.mesh and args.indexed_mesh)):
        ap.error("--live-mesh-every: a number of frames, with --mesh and --indexed-mesh")
    if args.live_mesh_every and args.native:
        ap.error("--live-mesh-every: not with --native (the update is not part of the native loop)")
    if args.corrected_trajectory and args.native:
        ap.error("--corrected-trajectory: not with --native")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU (there is no CPU fallback)")
    from voxelhashing_amd import reconstruction as R
    g = R.read_app_state(args.params)
    if args.record:
        g.s_recordData = 1
    read = R.read_tracking_state_rgbd if args.rgbd_tracking else R.read_tracking_state
    t = read(args.tracking) if args.tracking else None
    rs = R.read_render_state(args.params)
    if args.render_to:
        rs.s_renderToFile = 1
        rs.s_renderToFileDir = args.render_to.encode()
    cs = R.read_calibration_state(args.params)
    if args.camera_calibration:
        cs.s_bUseCameraCalibration = 1
    rec = R.Reconstruction(g, t, args.sens or None, use_rgbd_tracking=args.rgbd_tracking, render_state=rs, calibration_state=cs,
                           weighted_colour=args.weighted_colour)
    if args.native:  # the loop, its pinned buffers and the file, before the clock (the Python loop's reader has loaded its file above)
        try:
            rec.prepare_native(args.batch, tracking=args.native_tracking, tracking_rgbd=args.native_tracking and args.rgbd_tracking)
        except ValueError as e:
            raise SystemExit(str(e))
    t0 = time.perf_counter()
    if args.native:
        n = rec.run_native(args.max_frames, batch=args.batch, tracking=args.native_tracking, tracking_rgbd=args.native_tracking and args.rgbd_tracking)
        rec.native.synchronize()
    elif args.live_mesh_every:
        try:
            rec.liveMeshBegin()
        except ValueError as e:
            raise SystemExit(str(e))
        n, live_updates = 0, []
        while (args.max_frames is None or n < args.max_frames) and rec.frame() is not None:
            n += 1
            if n % args.live_mesh_every == 0:
                live_updates.append(dict(frame=n, **rec.liveMeshUpdate()))
        rec.scene.synchronize()
    else:
        n = rec.run(args.max_frames)
        rec.scene.synchronize()
    dt = time.perf_counter() - t0
    out = dict(frames=n, seconds=round(dt, 3), frames_per_s=round(n / dt, 1) if dt > 0 else None, lost_frames=rec.lost_frames,
               blocks=rec.scene.getNumOccupiedBlocks(), heap_free=rec.scene.getHeapFreeCount(),
               pose_source="recorded trajectory" if g.s_binaryDumpSensorUseTrajectory and not g.s_binaryDumpSensorUseTrajectoryOnlyInit else ("RGB-D ICP" if args.rgbd_tracking else "projective ICP"),
               colour_rule="weighted" if rec.scene.getColorIntegration() else "running average")
    if args.native:  # the loop's statistics ("frames" above is frames read; the loop's own count leaves out invalidFrames)
        out["loop"] = "native"
        out.update({k: (round(v, 6) if isinstance(v, float) else v) for k, v in rec.native.getStats().items() if k != "frames"})
    if cs.s_bUseCameraCalibration:
        out["camera_calibration"] = rec.camera_calibration
    if rs.s_renderToFile:
        out["render_to"] = bytes(rs.s_renderToFileDir).decode()
    if args.record:
        out["recorded"] = rec.saveRecordedFramesToFile(args.record)
    if args.corrected_trajectory:
        import numpy as np
        poses = np.loadtxt(args.corrected_trajectory, dtype=np.float64, ndmin=2)
        if poses.shape[1] != 16:
            raise SystemExit("--corrected-trajectory: 16 numbers per line")
        try:
            out["reintegrated"] = rec.reintegrateCorrected(poses.reshape(-1, 4, 4))
        except ValueError as e:
            raise SystemExit(str(e))
        out["blocks_after_reintegration"] = rec.scene.getNumOccupiedBlocks()
    cuts = {}
    for name, box, cut in (("erase", args.erase_box, rec.eraseRegion), ("crop", args.crop_box, rec.cropToRegion)):
        if box is not None:
            try:
                cuts[name] = cut(box_region(box))
            except ValueError as e:
                raise SystemExit(str(e))
    if cuts:
        out["cut"] = cuts
        out["blocks_after_cut"] = rec.scene.getNumOccupiedBlocks()
    if args.mesh:
        mesh_options = dict(normals=args.mesh_normals, min_component_faces=args.mesh_min_component, largest_component=args.mesh_largest_component,
                            cluster_cells=args.mesh_cluster, smooth_iterations=args.mesh_smooth, smooth_lambda=args.mesh_smooth_lambda,
                            smooth_mu=args.mesh_smooth_mu, keep_boundary=not args.mesh_smooth_free_boundary)
        if args.live_mesh_every:  # whatever happened since the last update (frames, a cut, a re-integration) is picked up by one more
            live_updates.append(dict(frame=n, **rec.liveMeshUpdate()))
            out["live_mesh"] = dict(every=args.live_mesh_every, updates=live_updates)
            m = rec.liveMesh(args.mesh, **mesh_options)
        elif args.indexed_mesh:
            m = rec.extractIsoSurfaceIndexed(args.mesh, **mesh_options)
        else:
            m = rec.extractIsoSurface(args.mesh)
        out["mesh"] = dict(file=args.mesh, indexed=bool(args.indexed_mesh), vertices=int(len(m["vertices"])), faces=int(len(m["faces"])))
        if args.mesh_normals:
            out["mesh"]["normals"] = int(len(m["normals"]))
        if args.mesh_min_component or args.mesh_largest_component:
            out["mesh"]["components"] = m["components"]
        if args.mesh_cluster:
            out["mesh"]["clustering"] = m["clustering"]
        if args.mesh_smooth:
            out["mesh"]["smoothing"] = m["smoothing"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
