#!/usr/bin/env python3
"""Measures the batch queries (vh_query_points / vh_query_rays) on a cfg2 scene (S1, 640x480, 4 cm voxels) and prints one
JSON line:

  points_per_s            1 M points near the surface (ray-cast hits + N(0, voxel) noise), with gradients
  rays_per_s_tile_order   the 640x480 rays of the last pose's view, ordered so that a wave holds an 8x8-pixel tile
  rays_per_s_permuted     the same rays in a fixed random permutation
  render_hash_us          k_render_hash (vh_render, gradients on) on the same view, for scale: the same march per pixel

Every figure is a kernel's own duration (vh_time_next_launch: the dispatch's time stamps), the median of --reps launches
after --warmup; uploads and downloads are not in it.

    python tools/bench_query.py [--frames 24] [--reps 30] [--warmup 5] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
f32 = np.float32


def camera_rays(cp, rp, pose):
    """the rays renderKernel casts for the view (float32, vectorised: a workload, not a bit-exact restatement)"""
    W, H = rp.m_width, rp.m_height
    yy, xx = np.mgrid[0:H, 0:W]
    cam = np.stack([(xx.astype(f32) - f32(cp.mx)) / f32(cp.fx), (yy.astype(f32) - f32(cp.my)) / f32(cp.fy), np.ones((H, W), f32)], axis=-1).reshape(-1, 3)
    cam /= np.linalg.norm(cam, axis=1, keepdims=True).astype(f32)
    m = np.asarray(pose, f32).reshape(4, 4)
    world = cam @ m[:3, :3].T
    world /= np.linalg.norm(world, axis=1, keepdims=True).astype(f32)
    d2r = f32(1) / cam[:, 2]
    return (np.broadcast_to(m[:3, 3], world.shape).astype(f32), world.astype(f32), (d2r * f32(rp.m_minDepth)).astype(f32),
            (d2r * f32(rp.m_maxDepth)).astype(f32))


def tile_order(W, H):
    """raster index of every pixel, tile by tile (8x8, row-major inside): 64 consecutive rays are one tile"""
    idx = np.arange(W * H).reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3)
    return idx.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    from voxelhashing_amd import engine as E, lib, synth, vhtypes as T
    L = lib.load()
    hip = C.CDLL("libamdhip64.so")  # the runtime the library already has open: events for vh_time_next_launch
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0

    hp, cp, rp = synth.config_params("cfg2")
    rp.m_useGradients = 1
    spheres, inside, radius = synth.scene("S1")
    scene = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=False, gc=True, starve=15))
    frame = E.DepthFrame(cp)
    for k in range(a.frames):
        pose = synth.orbit_pose(k, 1000, radius)
        E.synth_frame(spheres, inside, pose, cp, out=frame)
        scene.integrate(pose, frame, cp, None)
    scene.synchronize()
    hd, hpp = scene.getHashData(), scene.getHashParams()
    pose = np.array(pose, f32)
    ray = E.CUDARayCastSDF(rp)
    ray.setIntervalSplatting(False)
    ray.render(hd, hpp, cp, pose)  # sets the view matrices of the caster's parameters
    rpv, rd = ray.getRayCastParams(), ray.getRayCastData()
    W, H = rp.m_width, rp.m_height
    n = W * H

    def timed(launch):
        """median and least kernel time in us over the repetitions"""
        us = []
        for i in range(a.warmup + a.reps):
            lib.check(L.vh_time_next_launch(e0, e1), "vh_time_next_launch")
            launch()
            lib.check(L.vh_stream_synchronize(None), "synchronize")
            ms = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0, "the launch did not take the events"
            if i >= a.warmup:
                us.append(1e3 * ms.value)
        return float(np.median(us)), float(np.min(us))

    org, dirs, t0, t1 = camera_rays(cp, rpv, pose)
    out_t, out_n, out_c, out_s = lib.DeviceBuffer(4 * n), lib.DeviceBuffer(12 * n), lib.DeviceBuffer(4 * n), lib.DeviceBuffer(n)
    res = dict(lib=os.path.basename(lib.LIB_PATH), frames=a.frames, blocks=scene.getNumOccupiedBlocks(), reps=a.reps, rays=n)
    orders = dict(tile_order=tile_order(W, H), permuted=np.random.default_rng(1).permutation(n), raster=np.arange(n))
    for name, order in orders.items():
        ins = [lib.DeviceBuffer.from_numpy(np.ascontiguousarray(v[order])) for v in (org, dirs, t0, t1)]
        med, least = timed(lambda: lib.check(L.vh_query_rays(C.byref(hd), C.byref(hpp), C.byref(rpv), ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, n,
                                                                out_t.ptr, out_n.ptr, out_c.ptr, out_s.ptr, None), "vh_query_rays"))
        res[f"rays_{name}_us"] = [round(med, 1), round(least, 1)]
        res[f"rays_per_s_{name}"] = round(n / med * 1e6)
        if name == "raster":
            t = out_t.download(f32, n)
            hit = out_s.download(np.uint8, n) == T.QUERY_HIT
    res["hits"] = int(hit.sum())
    med, least = timed(lambda: lib.check(L.vh_render(C.byref(hd), C.byref(hpp), C.byref(rd), C.byref(cp), C.byref(rpv), None), "vh_render"))
    res["render_hash_us"] = [round(med, 1), round(least, 1)]
    res["render_hash_pixels_per_s"] = round(n / med * 1e6)
    depth = ray.download()["depth"].reshape(n)
    res["render_hash_hits"] = int((depth != -np.inf).sum())

    # points near the surface: the hits' positions with N(0, voxel) noise, repeated up to --points
    surface = org[hit] + dirs[hit] * t[hit, None]
    rng = np.random.default_rng(2)
    pts = (surface[rng.integers(0, len(surface), a.points)] + rng.normal(0.0, hpp.m_virtualVoxelSize, (a.points, 3))).astype(f32)
    d_pts = lib.DeviceBuffer.from_numpy(pts)
    p_sdf, p_col, p_grad, p_val = lib.DeviceBuffer(4 * a.points), lib.DeviceBuffer(4 * a.points), lib.DeviceBuffer(12 * a.points), lib.DeviceBuffer(a.points)
    for name, grad in (("points", p_grad.ptr), ("points_no_gradient", None)):
        med, least = timed(lambda: lib.check(L.vh_query_points(C.byref(hd), C.byref(hpp), d_pts.ptr, a.points, p_sdf.ptr, p_col.ptr, grad, p_val.ptr, None),
                                             "vh_query_points"))
        res[f"{name}_us"] = [round(med, 1), round(least, 1)]
        res[f"{name}_per_s"] = round(a.points / med * 1e6)
    res["points"] = a.points
    res["points_valid"] = int(p_val.download(np.uint8, a.points).sum())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
