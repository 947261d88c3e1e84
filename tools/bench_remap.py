#!/usr/bin/env python3
"""Measures the sensor's depth-to-colour remap (s_bUseCameraCalibration): per-launch time of k_view_raster,
k_view_raster_large and k_view_resolve_depth from rocprofv3 --kernel-trace --stats, against k_view_resolve plus the
copy of its depth map on the same input; CUDARGBDSensor::process per frame with and without the remap; tools/replay.py's
frames/s without it.  Prints one JSON line.

    python tools/bench_remap.py [--reps 200] [--frames 30] [--out DIR]

Cases: a 640x480 sensor frame (a wavy surface 1.1-1.7 m away with a depth step and 3 % holes) at an adapter size of
640x480 and of 1280x960, the depth camera 5 cm beside the colour camera.  Each case is one child process under the
profiler; the process() wall times come from a child of their own, without the profiler."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = {"640x480": (640, 480), "1280x960": (1280, 960)}
KERNELS = ("k_view_raster", "k_view_raster_large", "k_view_resolve_depth", "k_view_resolve")


def setup(case):
    import ctypes as C
    import numpy as np
    from voxelhashing_amd import engine as E, lib, vhtypes as T
    W, H = CASES[case]
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:480, 0:640].astype(np.float32)
    depth = (1.4 + 0.3 * np.sin(xx / 37.0) * np.cos(yy / 23.0)).astype(np.float32)
    depth[:, 384:] += np.float32(0.3)
    depth[rng.random((480, 640)) < 0.03] = 0.0
    colour = rng.integers(1, 256, size=(480, 640, 4), dtype=np.uint8)
    ext = np.eye(4, dtype=np.float32)
    ext[0, 3] = 0.05
    ck = (531.7, 530.2, 322.4, 244.9)
    sensor = E.CUDARGBDSensor((640, 480), (640, 480), (W, H), 525.0, 525.0, 319.5, 239.5, 0.5, 5.0)
    plain = E.CUDARGBDSensor((640, 480), (640, 480), (W, H), 525.0, 525.0, 319.5, 239.5, 0.5, 5.0)
    sensor.setCameraCalibration(True, *ck, ext, 0.012, 0.01)
    assert sensor.getCameraCalibration()[0]
    return C, np, E, lib, T, W, H, depth, colour, sensor, plain


def inner(case, reps):
    """the remap inside process(), then the full resolve + copy on the same filtered map, reps times each"""
    C, np, E, lib, T, W, H, depth, colour, sensor, plain = setup(case)
    L = lib.load()
    params = sensor.getCameraCalibration()[1]
    for _ in range(reps):
        sensor.process(depth, colour)
    # the full resolve writes depth, position, normal and colour; its depth map then has to be copied to d_depthData
    plain.process(depth, colour)
    src = lib.DeviceBuffer.from_numpy(plain.download()["depth"])  # the map the remap draws: the resampled frame
    keys = lib.DeviceBuffer(8 * W * H)
    lib.check(L.vh_memset(keys.ptr, 0xFF, 8 * W * H, None), "memset")
    large = lib.DeviceBuffer(4 * L.vh_view_large_list_words(W, H))
    lib.check(L.vh_memset(large.ptr, 0, 4, None), "memset")
    colour4 = lib.DeviceBuffer(16 * W * H)
    outs = [lib.DeviceBuffer(4 * W * H)] + [lib.DeviceBuffer(16 * W * H) for _ in range(3)]
    dst = lib.DeviceBuffer(4 * W * H)
    for _ in range(reps):
        lib.check(L.vh_view_raster(src.ptr, C.byref(params), keys.ptr, large.ptr, None), "raster")
        lib.check(L.vh_view_resolve(src.ptr, colour4.ptr, C.byref(params), keys.ptr, large.ptr, *[b.ptr for b in outs], None), "resolve")
        lib.check(L.vh_copy_float_map(dst.ptr, outs[0].ptr, W, H, None), "copy")
    lib.check(L.vh_device_synchronize(), "sync")
    covered = int((sensor.download()["depth"] != -np.inf).sum())
    print(json.dumps(dict(case=case, adapter=[W, H], covered_pixels=covered)))


def inner_wall(case, reps):
    """process() per frame, wall clock, with and without the remap"""
    C, np, E, lib, T, W, H, depth, colour, sensor, plain = setup(case)
    out = {}
    for name, s in (("process_ms_calibrated", sensor), ("process_ms_plain", plain)):
        for _ in range(10):
            s.process(depth, colour)
        t0 = time.perf_counter()
        for _ in range(reps):
            s.process(depth, colour)
        out[name] = round(1e3 * (time.perf_counter() - t0) / reps, 3)
    print(json.dumps(dict(case=case, **out)))


def kernel_stats(d):
    out = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            m = re.search(r"(k_\w+)", r["Name"])
            name = m.group(1) if m and m.group(1) in KERNELS else ("copy (blit)" if "opy" in r["Name"] else None)
            if name:
                out[name] = dict(calls=int(r["Calls"]), avg_us=round(float(r["AverageNs"]) / 1e3, 2), min_us=round(float(r["MinNs"]) / 1e3, 2),
                                 max_us=round(float(r["MaxNs"]) / 1e3, 2))
    return out


def child(args, timeout=600):
    log = subprocess.run(args, capture_output=True, timeout=timeout, text=True)
    if log.returncode != 0:
        raise SystemExit(f"rc {log.returncode}\n{log.stdout[-2000:]}\n{log.stderr[-2000:]}")
    return json.loads([ln for ln in log.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", choices=tuple(CASES), default=None)
    ap.add_argument("--inner-wall", choices=tuple(CASES), default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--out", default=None, help="keep the profiler's files here")
    args = ap.parse_args()
    if args.inner:
        return inner(args.inner, args.reps)
    if args.inner_wall:
        return inner_wall(args.inner_wall, args.reps)
    out_root = args.out or tempfile.mkdtemp(prefix="bench_remap_")
    res = dict(kernels={}, process={})
    me = [sys.executable, os.path.abspath(__file__)]
    for case in CASES:
        d = os.path.join(out_root, case)
        res["kernels"][case] = dict(child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "p", "--"] + me +
                                          ["--inner", case, "--reps", str(args.reps)]), **kernel_stats(d))
        res["process"][case] = child(me + ["--inner-wall", case, "--reps", str(args.reps)])
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_view
    t0 = time.perf_counter()
    res["replay_frames_per_s"] = bench_view.replay_fps(args.frames, False)
    res["replay_frames"] = args.frames
    res["seconds"] = round(time.perf_counter() - t0, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
