#!/usr/bin/env python3
"""Measures the closed loop with camera tracking on: sensor pre-processing -> raycast at the last
pose -> projective ICP (3 levels, the reference's default settings) -> integrate at the tracked pose, on the S3 scene
at 640x480 / 4 cm voxels (cfg2's sizes).  Wall time per frame including the one read-back of the pose, HIP-event time of
applyCT alone, and the drift against the true trajectory.  One JSON line; with --rgbd a second one for the RGB-D
tracker (CUDACameraTrackingMultiResRGBD, the reference's default settings with their colour keys) on the same frames.

    python tools/bench_tracking.py [--frames 120] [--width 640 --height 480] [--rgbd] [--weighted-colour]

--weighted-colour: every scene fuses colours weighted by the voxel weights (HashParams.m_colorIntegration = 1) instead of
the reference's running 50/50 average; each line names the rule as "colour_rule".

--native: the same loop against the native frame loop with tracking on (engine.Reconstruction.setTracking), in ONE process,
the two legs alternating --repeats times (tools/bench_ingest.py's scheme): (a) the Python loop exactly as timed above,
(b) the native tracked loop fed raw frames from pinned host memory.  Both legs see the same measurements: the frames are
quantised to what a sensor records (16-bit millimetres, 0 = no measurement; RGB bytes), leg (a) gets them as the float
depth + RGBX a SensorDataReader would hand over.  One JSON line: medians and ranges of both, icp_ms_per_frame of (a), the
drift of both, the largest difference between the two legs' poses; exit status 1 when (b)'s median is below (a)'s.
--native --rgbd: the same two legs with the RGB-D tracker (CUDACameraTrackingMultiResRGBD.applyCT against
engine.Reconstruction.setTrackingRGBD), default RGB-D settings.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--rgbd", action="store_true", help="also measure the RGB-D tracker on the same frames (second line)")
    ap.add_argument("--trajectory", action="store_true", help="poses from the true trajectory, no ICP: the host-fed (PCIe-inclusive) rate of the plain loop")
    ap.add_argument("--native", action="store_true", help="the Python loop against the native tracked loop, legs alternating (one line)")
    ap.add_argument("--repeats", type=int, default=5, help="--native: how often each leg runs")
    ap.add_argument("--only", default=None, choices=("python", "native"), help="--native: one leg alone (for a profiler run)")
    ap.add_argument("--weighted-colour", action="store_true", help="fuse colours weighted by the voxel weights instead of the running 50/50 average")
    args = ap.parse_args()
    import torch
    from oracle import oracle as O
    from voxelhashing_amd import synth, vhtypes as T
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    W, H = args.width, args.height
    hp = T.make_hash_params(500000, 1 << 18, weighted_colour=args.weighted_colour, **synth.PARAM_SETS["P4"])
    cp = T.make_depth_camera_params(W, H)
    rp = T.make_raycast_params(hp, cp)
    spheres, inside, radius = synth.scene("S3")
    truth = [synth.orbit_pose(k, 1000, radius) for k in range(args.frames)]
    frames = []
    for p in truth:  # the "sensor": depth in metres + RGBX bytes on the host
        d, c = O.synth_frame(spheres, inside, p, cp)
        rgbx = np.ascontiguousarray(np.clip(c * 255.0, 0, 255).astype(np.uint8))
        rgbx[..., 3] = 255
        frames.append((d, rgbx))
    if args.native:
        return native_against_python(args, frames, truth, hp, cp, rp, W, H)
    for kind in (["f5", "rgbd"] if args.rgbd and not args.trajectory else ["f5"]):
        run(args, kind, frames, truth, hp, cp, rp, W, H)


def colour_rule(hp):
    return "weighted" if hp.m_colorIntegration else "running average"


def spread(values):
    return dict(median=round(statistics.median(values), 1), min=round(min(values), 1), max=round(max(values), 1), runs=[round(v, 1) for v in values])


def drift(pose, want):
    rel = np.linalg.inv(np.asarray(pose, np.float64).reshape(4, 4)) @ np.asarray(want, np.float64).reshape(4, 4)
    return (round(float(np.linalg.norm(rel[:3, 3])), 5),
            round(float(np.degrees(np.arccos(np.clip(0.5 * (np.trace(rel[:3, :3]) - 1), -1, 1)))), 4))


def native_against_python(args, frames, truth, hp, cp, rp, W, H):
    from voxelhashing_amd import engine as E, lib, vhtypes as T
    n = args.frames
    # what a sensor records, and what a SensorDataReader makes of it for the Python loop
    d16 = lib.PinnedArray((n, H, W), np.uint16)
    rgb = lib.PinnedArray((n, H, W, 3), np.uint8)
    quantised = []
    for k, (d, rgbx) in enumerate(frames):
        d16.array[k] = np.where(np.isfinite(d), np.floor(1000.0 * d.astype(np.float64) + 0.5), 0).clip(0, 65535).astype(np.uint16)
        rgb.array[k] = rgbx[..., :3]
        quantised.append((d16.array[k].astype(np.float32) / np.float32(1000.0), rgbx))
    scene = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=False, gc=False))
    ray = E.CUDARayCastSDF(rp)
    loop = E.Reconstruction(scene, ray, None, cp, E.Reconstruction.defaultOptions(s_framesOnHost=1))
    loop.setRawFormat((W, H), (W, H), 1000.0, 3)
    kind = "rgbd" if args.rgbd else "f5"
    if args.rgbd:
        loop.setTrackingRGBD(T.make_tracking_state_rgbd())
    else:
        loop.setTracking(T.make_tracking_state())
    ds, cs = d16.array[0].nbytes, rgb.array[0].nbytes
    seq = E.Reconstruction.makeRawFrames([np.eye(4, dtype=np.float32)] * n, [d16.ptr + k * ds for k in range(n)], [rgb.ptr + k * cs for k in range(n)])

    def native_leg():
        loop.synchronize()
        scene.reset()
        loop.reset()
        loop.runRaw(seq, 0, 1)  # the first frame, as the Python leg integrates it, before the clock
        loop.synchronize()
        t0 = time.perf_counter()
        loop.runRaw(seq, 1, n - 1)
        loop.synchronize()
        return (n - 1) / (time.perf_counter() - t0)

    both = args.only is None
    if args.only != "python":
        native_leg()  # warm-up: code objects, the pinned pages once over the link
    py, nat = [], []
    for _ in range(args.repeats):  # alternating
        if args.only != "native":
            py.append(run(args, kind, quantised, truth, hp, cp, rp, W, H, quiet=True))
        if args.only != "python":
            nat.append(native_leg())
    out = dict(bench="tracking, Python loop against the native tracked loop", tracker="RGB-D ICP" if args.rgbd else "projective ICP", unit="frames/s",
               frames=n - 1, repeats=args.repeats, colour_rule=colour_rule(hp))
    t0 = np.asarray(truth[0], np.float64).reshape(4, 4)
    if py:
        last = py[-1]
        out["python_loop"] = dict(frames_per_s=spread([r["value"] for r in py]), icp_ms_per_frame=last["icp_ms_per_frame"],
                                  icp_systems_per_frame=last["icp_systems_per_frame"], lost_frames=last["lost_frames"], drift_m=last["drift_m"],
                                  drift_deg=last["drift_deg"], path_m=last["path_m"])
    if nat:
        st = loop.getStats()
        in_world = [(t0 @ p.astype(np.float64)) if p[0, 0] != -np.inf else None for p in loop.getPoses()]  # the native loop's world is the first camera
        b = spread(nat)
        out["native_tracked_loop"] = dict(frames_per_s=b, ms_per_frame=round(1e3 / b["median"], 3), lost_frames=st["lostFrames"], tracked_frames=st["trackedFrames"],
                                          host_wait_s=round(st["hostWaitSeconds"], 4), host_enqueue_s=round(st["hostEnqueueSeconds"], 4),
                                          upload_bytes=st["uploadBytes"], drift_m=drift(in_world[-1], truth[-1])[0], drift_deg=drift(in_world[-1], truth[-1])[1])
    out["gate_native_not_slower"] = True
    if both:
        a, b = out["python_loop"]["frames_per_s"], out["native_tracked_loop"]["frames_per_s"]
        out["native_over_python"] = round(b["median"] / a["median"], 2)
        out["largest_pose_difference"] = max(float(np.abs(x - np.asarray(y, np.float64).reshape(4, 4)).max())
                                             for x, y in zip(in_world, py[-1]["poses"]) if x is not None and y is not None)
        out["gate_native_not_slower"] = bool(b["median"] >= a["median"])
    settings = "reference default tracking settings" + (" with their colour keys" if args.rgbd else "")
    out["config"] = dict(workload=f"S3 orbit, {W}x{H}, P4 voxels, 3 pyramid levels, {settings}, frames quantised to 16-bit "
                                  "millimetres + RGB bytes; Python loop: float depth + RGBX from pageable host memory, native loop: raw frames from pinned "
                                  "host memory; online alloc")
    print(json.dumps(out))
    loop.close()
    return 0 if out["gate_native_not_slower"] else 1


def run(args, kind, frames, truth, hp, cp, rp, W, H, quiet=False):
    import torch
    from voxelhashing_amd import engine as E, lib, vhtypes as T
    L = lib.load()
    scene = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=False, gc=False))
    ray = E.CUDARayCastSDF(rp)
    sensor = E.CUDARGBDSensor((W, H), (W, H), (W, H), cp.fx, cp.fy, cp.mx, cp.my, cp.m_sensorDepthWorldMin, cp.m_sensorDepthWorldMax)
    if kind == "rgbd":
        tracker = E.CUDACameraTrackingMultiResRGBD(W, H, 3)
        ts = T.make_tracking_state_rgbd()
    else:
        tracker = E.CUDACameraTrackingMultiRes(W, H, 3)
        ts = T.make_tracking_state()
    a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
    lib.check(L.vh_rgbd_sensor_get_maps(sensor.handle, C.byref(a), C.byref(b), C.byref(c)), "maps")
    cam = sensor.getDepthCameraData()
    frame = E.DepthFrame(cp, depth_ptr=cam.d_depthData, color_ptr=cam.d_colorData)
    pose = truth[0]
    sensor.process(*frames[0])
    scene.integrate(pose, frame, cp, None)
    icp_ms, lost_frames, iters = 0.0, 0, 0
    poses = [pose]  # the pose every frame was integrated at (None: tracking lost)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(1, args.frames):
        sensor.process(*frames[k])
        ray.render(scene.getHashData(), scene.getHashParams(), cp, pose)
        rd = ray.getRayCastData()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if args.trajectory:
            pose = truth[k]
            scene.integrate(pose, frame, cp, None)
            continue
        e0.record()
        if kind == "rgbd":
            new_pose, lost = tracker.applyCT(a, b, cam.d_colorData, rd.d_depth4, rd.d_normals, rd.d_colors, pose, ts, None, cp)
        else:
            new_pose, lost = tracker.applyCT(a, b, rd.d_depth4, rd.d_normals, pose, ts, None, cp)
        e1.record()
        e1.synchronize()
        icp_ms += e0.elapsed_time(e1)
        iters += tracker.state.icp.iterations if kind == "rgbd" else tracker.state.iterations
        if lost:
            lost_frames += 1
        else:
            pose = new_pose
        poses.append(None if lost else pose)
        scene.integrate(pose, frame, cp, None)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rel = np.linalg.inv(np.asarray(pose, np.float64).reshape(4, 4)) @ np.asarray(truth[-1], np.float64).reshape(4, 4)
    path = sum(np.linalg.norm(np.asarray(truth[k], np.float64).reshape(4, 4)[:3, 3] - np.asarray(truth[k - 1], np.float64).reshape(4, 4)[:3, 3]) for k in range(1, args.frames))
    n = args.frames - 1
    if args.trajectory:
        print(json.dumps(dict(metric="host-fed frames/sec: upload + sensor pre-processing + raycast + integrate, poses given", value=round(n / dt, 1), unit="frames/s",
                              ms_per_frame=round(1e3 * dt / n, 3), upload_bytes_per_frame=int(frames[0][0].nbytes + frames[0][1].nbytes),
                              config=dict(workload=f"S3 orbit, {W}x{H}, P4 voxels, float depth + RGBX bytes from pageable host memory every frame"))))
        return
    what = "RGB-D ICP (depth + photometric)" if kind == "rgbd" else "ICP"
    settings = "reference default tracking settings with their colour keys" if kind == "rgbd" else "reference default tracking settings"
    line = (dict(metric=f"tracked frames/sec: sensor pre-processing + raycast + {what} + integrate", value=round(n / dt, 1), unit="frames/s",
                          ms_per_frame=round(1e3 * dt / n, 3), icp_ms_per_frame=round(icp_ms / n, 3), icp_systems_per_frame=round(iters / n, 2), lost_frames=lost_frames,
                          drift_m=round(float(np.linalg.norm(rel[:3, 3])), 5),
                          drift_deg=round(float(np.degrees(np.arccos(np.clip(0.5 * (np.trace(rel[:3, :3]) - 1), -1, 1)))), 4), path_m=round(float(path), 3),
                          colour_rule=colour_rule(hp),
                          config=dict(workload=f"S3 orbit, {W}x{H}, P4 voxels, 3 pyramid levels, {settings}, host-fed frames", **({"tracker": "rgbd"} if kind == "rgbd" else {}))))
    if not quiet:
        print(json.dumps(line))
    return dict(line, poses=poses)

if __name__ == "__main__":
    sys.exit(main())
