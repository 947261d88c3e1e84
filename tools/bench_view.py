#!/usr/bin/env python3
"""Measures the shaded view (csrc/vh_view.hip): per-kernel time of raster, large-triangle raster, resolve and Phong from
rocprofv3 --kernel-trace --stats, and tools/replay.py's frames/s with and without --render-to.  Prints one JSON line.

    python tools/bench_view.py [--reps 200] [--frames 30] [--out DIR]

Cases (the model: S1 integrated at 640x480 and ray-cast at the last pose, as tests/test_view_rendering.py builds it):
  640x480     the ray cast drawn at its own view and size (what renderToFile does)
  1920x1080   the same view on a 1080p screen (intrinsics scaled by 3)
  magnified   a close novel view (0.9 m nearer, fx = fy = 6000 at 640x480): most triangles take the second phase
Each case is one child process under the profiler: per repetition one RenderDepthMap and two Phong passes (material
and colour, RGBA8)."""
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
CASES = ("640x480", "1920x1080", "magnified")
KERNELS = ("k_view_raster", "k_view_raster_large", "k_view_resolve", "k_phong")
PARAMS = """
s_adapterWidth = 640
s_adapterHeight = 480
s_sensorDepthMax = 5.0f
s_sensorDepthMin = 0.5f
s_hashNumBuckets = 262144
s_hashNumSDFBlocks = 65536
s_hashMaxCollisionLinkedListSize = 7
s_SDFVoxelSize = 0.01f
s_SDFMarchingCubeThreshFactor = 10.0f
s_SDFTruncation = 0.05f
s_SDFTruncationScale = 0.025f
s_SDFMaxIntegrationDistance = 4.0f
s_SDFIntegrationWeightSample = 10
s_SDFIntegrationWeightMax = 255
s_SDFRayIncrementFactor = 0.8f
s_SDFRayThresSampleDistFactor = 50.5f
s_SDFRayThresDistFactor = 50.0f
s_integrationEnabled = true
s_trackingEnabled = true
s_offlineProcessing = true
s_binaryDumpSensorUseTrajectory = true
s_materialShininess = 16.0f
s_materialAmbient = 0.75f 0.65f 0.5f 1.0f
s_materialDiffuse = 1.0f 0.9f 0.7f 1.0f
s_materialSpecular = 1.0f 1.0f 1.0f 1.0f
s_lightAmbient = 0.4f 0.4f 0.4f 1.0f
s_lightDiffuse = 0.6f 0.52944f 0.4566f 0.6f
s_lightSpecular = 0.3f 0.3f 0.3f 1.0f
s_lightDirection = 0.0f -1.0f 2.0f
s_renderingDepthDiscontinuityThresOffset = 0.012f
s_renderingDepthDiscontinuityThresLin = 0.001f
"""


def inner(case, reps):
    import numpy as np
    from voxelhashing_amd import engine as E, synth, vhtypes as T
    W, H = 640, 480
    hp = T.make_hash_params(1 << 18, 1 << 16, **synth.PARAM_SETS["P4"])
    cp = T.make_depth_camera_params(W, H)
    scene, ray = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=True, gc=False)), E.CUDARayCastSDF(T.make_raycast_params(hp, cp))
    poses = [np.array(synth.orbit_pose(k, 90), dtype=np.float32) for k in range(3)]
    for p in poses:
        scene.integrate(p, E.synth_frame(synth.S1_SPHERES, 0, p, cp), cp, None)
    ray.render(scene.getHashData(), scene.getHashParams(), cp, poses[-1])
    rp, rd = ray.getRayCastParams(), ray.getRayCastData()
    Kinv = np.array(rp.m_intrinsicsInverse[:], np.float32)
    K = np.array(rp.m_intrinsics[:], np.float32).reshape(4, 4)
    view, Knew, (SW, SH) = np.eye(4, dtype=np.float32), K.copy(), (W, H)
    if case == "1920x1080":
        Knew[0, 0], Knew[1, 1], Knew[0, 2], Knew[1, 2], SW, SH = K[0, 0] * 3, K[1, 1] * 3, 959.5, 539.5, 1920, 1080
    elif case == "magnified":
        view[2, 3] = -0.9
        Knew[0, 0] = Knew[1, 1] = 6000.0
    renderer = E.RGBDRenderer()
    light = T.PhongLight()
    for k, v in dict(lightAmbient=(0.4, 0.4, 0.4, 1), lightDiffuse=(0.6, 0.52944, 0.4566, 0.6), lightSpecular=(0.3, 0.3, 0.3, 1),
                     lightDirection=(0, -1, 2), materialAmbient=(0.75, 0.65, 0.5, 1), materialSpecular=(1, 1, 1, 1),
                     materialDiffuse=(1, 0.9, 0.7, 1)).items():
        getattr(light, k)[:] = v
    light.materialShininess = 16.0
    phong = E.PhongLighting(light)
    for _ in range(reps):
        renderer.RenderDepthMap(rd.d_depth, rd.d_colors, W, H, Kinv, view, Knew, SW, SH, 0.012, 0.001)
        m = renderer.getMaps()
        for colored in (False, True):
            phong.render(m["positions"], m["normals"], m["colors"], colored, SW, SH, rgba8=True)
    scene.synchronize()
    covered = int((renderer.download()["depth"] != -np.inf).sum())
    print(json.dumps(dict(case=case, screen=[SW, SH], covered_pixels=covered)))


def kernel_stats(d):
    out = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            m = re.search(r"(k_\w+)", r["Name"])
            if m and m.group(1) in KERNELS:
                out[m.group(1)] = dict(calls=int(r["Calls"]), avg_us=round(float(r["AverageNs"]) / 1e3, 2),
                                       min_us=round(float(r["MinNs"]) / 1e3, 2), max_us=round(float(r["MaxNs"]) / 1e3, 2))
    return out


def replay_fps(frames, render_to):
    """frames/s of tools/replay.py on a synthetic S1 sequence at 640x480 (recorded trajectory)"""
    import numpy as np
    from voxelhashing_amd import engine as E, sensor_data as SD, synth, vhtypes as T
    cp = T.make_depth_camera_params(640, 480)
    with tempfile.TemporaryDirectory() as tmp:
        sens, params = os.path.join(tmp, "s1.sens"), os.path.join(tmp, "params.txt")
        sd = SD.SensorData.create((640, 480), (640, 480), SD.make_intrinsic_matrix(cp.fx, cp.fy, cp.mx, cp.my), depth_shift=1000.0,
                                  sensor_name="synthetic S1", depth_type=SD.TYPE_ZLIB_USHORT)
        fr = E.DepthFrame(cp)
        for k in range(frames):
            p = np.array(synth.orbit_pose(k, 90), dtype=np.float32)
            d, c = E.synth_frame(synth.S1_SPHERES, 0, p, cp, out=fr).download()
            d = np.where(np.isfinite(d), d, 0.0)
            rgb = np.clip(np.nan_to_num(c[..., :3], neginf=0.0) * 255.0 + 0.5, 0, 255).astype(np.uint8)
            sd.addFrame(np.ascontiguousarray(rgb), np.floor(1000.0 * d + 0.5).astype(np.uint16), p, k, k)
        sd.saveToFile(sens)
        open(params, "w").write(PARAMS)
        cmd = [sys.executable, os.path.join(ROOT, "tools", "replay.py"), "--params", params, "--sens", sens]
        if render_to:
            cmd += ["--render-to", os.path.join(tmp, "render")]
        out = json.loads(subprocess.check_output(cmd, timeout=600).decode().strip().splitlines()[-1])
        return out["frames_per_s"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", choices=CASES, default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--out", default=None, help="keep the profiler's files here")
    args = ap.parse_args()
    if args.inner:
        return inner(args.inner, args.reps)
    out_root = args.out or tempfile.mkdtemp(prefix="bench_view_")
    res = dict(kernels={})
    for case in CASES:
        d = os.path.join(out_root, case)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "p", "--",
               sys.executable, os.path.abspath(__file__), "--inner", case, "--reps", str(args.reps)]
        log = subprocess.run(cmd, capture_output=True, timeout=600, text=True)
        if log.returncode != 0:
            raise SystemExit(f"{case}: rc {log.returncode}\n{log.stdout[-2000:]}\n{log.stderr[-2000:]}")
        line = [ln for ln in log.stdout.splitlines() if ln.startswith("{")][-1]
        res["kernels"][case] = dict(json.loads(line), **kernel_stats(d))
    t0 = time.perf_counter()
    res["replay_frames_per_s"] = replay_fps(args.frames, False)
    res["replay_render_to_frames_per_s"] = replay_fps(args.frames, True)
    res["replay_frames"] = args.frames
    res["seconds"] = round(time.perf_counter() - t0, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
