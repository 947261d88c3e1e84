#!/usr/bin/env python3
"""What raw frames cost and save in the native frame loop: cfg2's orbit at 640x480, the same frames fed in every form
the loop takes, alternating, several repeats each, the host clock around a run that ends in synchronize().

    A  float depth + RGBX bytes in pinned host memory (s_framesOnHost = 1): the loop as it was, the baseline
    B  raw frames in pinned host memory, sensor size = adapter size: u16 depth + RGB, and u16 depth + RGBX
    C  raw frames in pinned host memory, 640x480 depth + 1296x968 RGB -> 640x480
    D  raw frames resident in device memory (u16 + RGB), against the resident float loop
    E  tools/replay.py on a synthetic `.sens` file written from a seed: the Python loop against --native

Needs a GPU; prints one JSON line.  `--only B_rgb --repeats 1` runs one leg alone (for a kernel trace of k_ingest_frame)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPLAY_PARAMS = """
s_sensorIdx = 8;
s_adapterWidth = 640;
s_adapterHeight = 480;
s_sensorDepthMax = 5.0f;
s_sensorDepthMin = 0.5f;
s_hashNumBuckets = 500000;
s_hashNumSDFBlocks = 1000000;
s_hashMaxCollisionLinkedListSize = 7;
s_SDFVoxelSize = 0.04f;
s_SDFMarchingCubeThreshFactor = 10.0f;
s_SDFTruncation = 0.20f;
s_SDFTruncationScale = 0.10f;
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
s_colorFilter = false;
s_integrationEnabled = true;
s_trackingEnabled = true;
s_garbageCollectionEnabled = true;
s_garbageCollectionStarve = 15;
s_marchingCubesMaxNumTriangles = 2500000;
s_streamingEnabled = false;
s_offlineProcessing = false;
s_binaryDumpSensorUseTrajectory = true;
s_binaryDumpSensorUseTrajectoryOnlyInit = false;
"""


def spread(values):
    return dict(median=round(statistics.median(values), 1), min=round(min(values), 1), max=round(max(values), 1), runs=[round(v, 1) for v in values])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sens-frames", type=int, default=300)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--only", default=None, help="one leg alone: A, B_rgb, B_rgbx, C, D_raw, D_float, E")
    ap.add_argument("--no-replay", action="store_true", help="skip leg E")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU (there is no CPU fallback)")
    from voxelhashing_amd import engine as E, synth, vhtypes as T
    n = args.frames if args.only != "E" else min(args.frames, args.sens_frames)
    hp, cp, rp = synth.config_params("cfg2")
    W, H = cp.m_imageWidth, cp.m_imageHeight
    spheres, inside, radius = synth.scene("S1")
    poses = [synth.orbit_pose(k, 1000, radius) for k in range(n)]
    dev = torch.device("cuda", 0)
    want = (lambda leg: args.only is None or args.only == leg)
    depth = torch.empty((n, H, W), dtype=torch.float32, device=dev)
    color = torch.empty((n, H, W, 4), dtype=torch.float32, device=dev)
    for k in range(n):
        E.synth_frame(spheres, inside, poses[k], cp, out=E.DepthFrame(cp, depth_ptr=depth[k].data_ptr(), color_ptr=color[k].data_ptr()))
    torch.cuda.synchronize()
    # what a sensor records: millimetres (0 = no measurement; below 2^15, so int16 holds the u16 bit pattern), RGB(X) bytes
    d16 = torch.where(torch.isfinite(depth), torch.floor(1000.0 * depth + 0.5), torch.zeros_like(depth)).clamp(0, 32767).to(torch.int16)
    rgbx = (color.clamp(0.0, 1.0) * 255.0).to(torch.uint8)
    rgbx[..., 3] = 255
    rgbx[(rgbx[..., :3] == 0).all(dim=-1)] = 0
    rgb = rgbx[..., :3].contiguous()

    def pinned(t):
        out = torch.empty(t.shape, dtype=t.dtype).pin_memory()
        out.copy_(t)
        return out

    scene = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=False, gc=True, starve=15, timings=False))
    ray = E.CUDARayCastSDF(rp)
    keep, legs = [], {}

    def leg(name, on_host, fmt, d, c, bytes_per_frame):
        keep.append((d, c))
        recon = E.Reconstruction(scene, ray, None, cp, E.Reconstruction.defaultOptions(s_framesOnHost=1 if on_host else 0))
        dp, cptr = [d[k].data_ptr() for k in range(n)], [c[k].data_ptr() for k in range(n)]
        if fmt is not None:
            recon.setRawFormat(**fmt)
            frames, run = E.Reconstruction.makeRawFrames(poses, dp, cptr), recon.runRaw
        else:
            frames, run = E.Reconstruction.makeFrames(poses, dp, cptr), recon.run
        legs[name] = dict(recon=recon, frames=frames, run=run, bytes_per_frame=bytes_per_frame, fps=[])

    same = dict(depth_size=(W, H), color_size=(W, H), depth_shift=1000.0)
    if want("A"):
        leg("A", True, None, pinned(depth), pinned(rgbx), 8 * W * H)
    if want("B_rgb"):
        leg("B_rgb", True, dict(same, color_channels=3), pinned(d16), pinned(rgb), 5 * W * H)
    if want("B_rgbx"):
        leg("B_rgbx", True, dict(same, color_channels=4), pinned(d16), pinned(rgbx), 6 * W * H)
    if want("C"):
        cw, ch = 1296, 968
        yi = (torch.arange(ch, device=dev) * H // ch).long()
        xi = (torch.arange(cw, device=dev) * W // cw).long()
        big = torch.empty((n, ch, cw, 3), dtype=torch.uint8).pin_memory()
        for k in range(n):  # nearest neighbour: the content does not matter to the clock, the size does
            big[k].copy_(rgb[k][yi][:, xi])
        leg("C", True, dict(depth_size=(W, H), color_size=(cw, ch), depth_shift=1000.0, color_channels=3), pinned(d16), big, 2 * W * H + 3 * cw * ch)
    if want("D_raw"):
        leg("D_raw", False, dict(same, color_channels=3), d16, rgb, 0)
    if want("D_float"):
        leg("D_float", False, None, depth, color, 0)
    torch.cuda.synchronize()

    def restart(L):
        L["recon"].synchronize()
        scene.reset()
        L["recon"].reset()

    for L in legs.values():  # warm-up: code objects, the pinned pages once over the link, clocks
        restart(L)
        L["run"](L["frames"], 0, min(args.warmup, n))
        L["recon"].synchronize()
    for _ in range(args.repeats):  # alternating
        for L in legs.values():
            restart(L)
            t0 = time.perf_counter()
            L["run"](L["frames"], 0, n)
            L["recon"].synchronize()
            L["fps"].append(n / (time.perf_counter() - t0))
    out = dict(bench="ingest", config="cfg2", width=W, height=H, frames=n, warmup=args.warmup, repeats=args.repeats, legs={})
    for name, L in legs.items():
        st = L["recon"].getStats()
        out["legs"][name] = dict(frames_per_s=spread(L["fps"]), bytes_per_frame=L["bytes_per_frame"], upload_bytes=st["uploadBytes"],
                                 upload_us=round(1e3 * st["uploadMs"] / st["uploadsTimed"], 1) if st["uploadsTimed"] else None,
                                 host_wait_s=round(st["hostWaitSeconds"], 3))
        restart(L)
        L["recon"].close()
    if "A" in legs and "B_rgb" in legs:
        a, b = out["legs"]["A"]["frames_per_s"], out["legs"]["B_rgb"]["frames_per_s"]
        out["B_rgb_over_A"] = round(b["median"] / a["median"], 3)
        out["A_spread"] = round((a["max"] - a["min"]) / a["median"], 3)
    ray.close()
    scene.close()

    if args.only in (None, "E") and not args.no_replay:
        # E: a `.sens` file from the same synthetic scene, played by tools/replay.py with and without --native
        from voxelhashing_amd import sensor_data as SD
        m = min(args.sens_frames, n)
        tmp = tempfile.mkdtemp(prefix="bench_ingest_")
        sens, params = os.path.join(tmp, "orbit.sens"), os.path.join(tmp, "zParameters.txt")
        open(params, "w").write(REPLAY_PARAMS)
        sd = SD.SensorData.create((W, H), (W, H), SD.make_intrinsic_matrix(cp.fx, cp.fy, cp.mx, cp.my), depth_shift=1000.0, sensor_name="synthetic S1",
                                  depth_type=SD.TYPE_ZLIB_USHORT)
        rng = np.random.default_rng(args.seed)  # sensor noise of +-1 mm, so that the zlib stream is not trivially small
        for k in range(m):
            d = d16[k].cpu().numpy().view(np.uint16).copy()
            noise = rng.integers(-1, 2, size=d.shape)
            d = np.where(d > 0, np.clip(d.astype(np.int64) + noise, 1, 65535), 0).astype(np.uint16)
            sd.addFrame(rgb[k].cpu().numpy(), d, poses[k], k, k)
        sd.saveToFile(sens)
        sd.close()
        # what the host's decoder alone can deliver (zlib depth, raw colour, one thread): the ceiling of both loops
        from voxelhashing_amd import reconstruction as R
        back = SD.SensorData.loadFromFile(sens)
        d_buf, c_buf = np.empty((64, H, W), np.uint16), np.empty((64, H, W, 3), np.uint8)
        t0 = time.perf_counter()
        for k0 in range(0, m, 64):
            R.decode_batch(back, k0, min(64, m - k0), d_buf, c_buf)
        decode_fps = m / (time.perf_counter() - t0)
        back.close()
        del depth, color, d16, rgbx, rgb, keep
        torch.cuda.empty_cache()
        replay = dict(python=[], native=[])
        for _ in range(args.repeats):
            for kind in ("python", "native"):
                cmd = [sys.executable, os.path.join(ROOT, "tools", "replay.py"), "--params", params, "--sens", sens] + (["--native"] if kind == "native" else [])
                line = subprocess.run(cmd, check=True, capture_output=True, timeout=300).stdout.decode().strip().splitlines()[-1]
                replay[kind].append(json.loads(line)["frames_per_s"])
        out["replay"] = dict(frames=m, sens_bytes=os.path.getsize(sens), decode_only_frames_per_s=round(decode_fps, 1), python=spread(replay["python"]), native=spread(replay["native"]))
        os.remove(sens)
        os.remove(params)
        os.rmdir(tmp)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
