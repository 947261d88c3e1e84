#!/usr/bin/env python3
"""Measures the scene merge (vh_merge.hip) on cfg2 (S1, 640x480, 4 cm voxels): two scenes are built from the two halves
of an orbit of --frames frames, the second is merged into the first (CUDASceneRepHashSDF.mergeScene), and one JSON line
is printed:

  blocks                  source blocks, of them present in the destination / allocated by the merge / left out
  alloc_passes            alloc passes the merge ran
  gather_us ... combine_us   each kernel's own duration [median, least]; alloc_us is the sum over the passes' medians
  call_ms                 the whole blocking call on the host clock (its read-backs included)
  combine_bytes, combine_tb_per_s, combine_of_hbm_peak
                          the combine kernel moves 12 KB per shared block (source and destination read, destination
                          written) and 8 KB per new one (the destination's zeros need no read to give the result), against
                          the 8 TB/s HBM peak DESIGN.md section 6 uses

A kernel's duration is the dispatch's own time stamps (vh_time_launch_after: the merge launches gather, classify, decide,
one kernel per alloc pass, combine).  The merge changes its destination, so every sample rebuilds the destination first;
a sample whose merge took another number of alloc passes than the first one is dropped (the skip count would name
another kernel).

With --transform the second scene is resampled into the first under a rigid motion (0.6 rad about (1, 2, 3) through the
world's origin, which the orbit circles, and a shift of a few voxels and a fraction: CUDASceneRepHashSDF.mergeSceneTransformed,
vh_resample.hip).
The call launches gather, candidates, resample and then the merge's kernels on the staged list; added to the line are

  resample                candidates, staged blocks, observed voxels
  candidates_us, resample_us   the two new kernels' own durations [median, least]
  stage_us                the three stages the issue names: candidates, resample, merge (classify + alloc + combine)
  bytes                   the source read once by the resample kernel (4 KB per source block), the staging pool written
                          (4 KB per staged block; an empty candidate leaves before it writes) and read again by the
                          combine, the destination read and written (8 KB per shared block, 4 KB per new one)

    python tools/bench_merge.py [--frames 24] [--reps 7] [--config cfg2] [--scene S1] [--transform] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--config", default="cfg2", choices=["cfg1", "cfg2", "cfg3", "cfg4"])
    ap.add_argument("--scene", default="S1", help="S1, or the dense S2 (thousands of blocks: the combine kernel's rate with the device filled)")
    ap.add_argument("--transform", action="store_true", help="resample the second scene into the first under a rigid motion (mergeSceneTransformed)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    from voxelhashing_amd import engine as E, lib, synth, vhtypes as T
    L = lib.load()
    hip = C.CDLL("libamdhip64.so")  # the runtime the library already has open: events for vh_time_launch_after
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0

    hp, cp, rp = synth.config_params(a.config)
    spheres, inside, radius = synth.scene(a.scene)
    opt = T.make_scene_options(offline=False, gc=True, starve=15)
    dst, src = E.CUDASceneRepHashSDF(hp, opt), E.CUDASceneRepHashSDF(hp, opt)
    frame = E.DepthFrame(cp)
    half = a.frames // 2

    def build(scene, first, last):
        scene.reset()
        for k in range(first, last):
            pose = synth.orbit_pose(k, 1000, radius)
            E.synth_frame(spheres, inside, pose, cp, out=frame)
            scene.integrate(pose, frame, cp, None)
        scene.synchronize()

    build(src, half, a.frames)
    motion = None
    if a.transform:
        # about the origin, which the orbit circles, so that the two halves still overlap
        th, ax = 0.6, np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
        vs = float(hp.m_virtualVoxelSize)
        motion = np.eye(4)
        motion[:3, :3] = R
        motion[:3, 3] = np.array([3.3, -5.4, 10.7]) * vs

    def merge(skip=None):
        """a fresh destination, one merge -> (counts, the armed kernel's us or None, the call's ms)"""
        build(dst, 0, half)
        if skip is not None:
            lib.check(L.vh_time_launch_after(skip, e0, e1), "vh_time_launch_after")
        t0 = time.perf_counter()
        counts = dst.mergeSceneTransformed(src, motion) if a.transform else dst.mergeScene(src)
        ms_call = 1e3 * (time.perf_counter() - t0)
        us = None
        if skip is not None:
            ms = C.c_float()
            if hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0:
                us = 1e3 * ms.value
        return counts, us, ms_call

    first, _, _ = merge()
    passes = first["alloc_passes"]
    assert first["status"] == 0, first
    phases = [("gather", 0), ("classify", 1)] + [(f"alloc{p}", 3 + p) for p in range(passes)] + [("combine", 3 + passes)]
    if a.transform:
        rs = first["resample"]
        # (a table that filled and grew would have run the candidates kernel again and shifted every later launch)
        assert rs["candidates"] <= 16 * rs["source_blocks"], rs
        phases = [("gather", 0), ("candidates", 1), ("resample", 2), ("classify", 3)] + [(f"alloc{p}", 5 + p) for p in range(passes)] + [("combine", 5 + passes)]
    res = dict(lib=os.path.basename(lib.LIB_PATH), config=a.config, scene=a.scene, frames=a.frames, reps=a.reps,
               blocks=dict(source=first["source_blocks"], present=first["present"], allocated=first["allocated"], left_out=first["left_out"]),
               voxels=dict(combined=first["combined"], copied=first["copied"]), alloc_passes=passes)
    calls, dropped = [], 0
    for name, skip in phases:
        us = []
        for _ in range(3 * a.reps):
            counts, t, ms_call = merge(skip)
            if counts["alloc_passes"] != passes or t is None:
                dropped += 1
                continue
            us.append(t)
            calls.append(ms_call)
            if len(us) == a.reps:
                break
        res[name + "_us"] = [round(float(np.median(us)), 1), round(float(np.min(us)), 1)] if us else None
    alloc = [res.pop(f"alloc{p}_us") for p in range(passes)]
    res["alloc_pass_us"] = alloc
    res["alloc_us"] = round(sum(m[0] for m in alloc if m), 1)
    res["samples_dropped"] = dropped
    res["call_ms"] = [round(float(np.median(calls)), 3), round(float(np.min(calls)), 3)] if calls else None
    nbytes = 12288 * first["present"] + 8192 * first["allocated"]
    if a.transform:
        res["transform"] = [[float(v) for v in row] for row in motion]
        res["resample"] = dict(candidates=rs["candidates"], staged=rs["staged"], observed=rs["observed"])
        merge_us = sum(res[k][0] for k in ("classify_us", "combine_us") if res[k]) + res["alloc_us"]
        res["stage_us"] = dict(candidates=res["candidates_us"] and res["candidates_us"][0], resample=res["resample_us"] and res["resample_us"][0],
                               merge=round(merge_us, 1))
        res["bytes"] = dict(source_read=4096 * rs["source_blocks"], staging_written=4096 * rs["staged"], staging_read=4096 * rs["staged"],
                            destination_read=4096 * first["present"], destination_written=4096 * (first["present"] + first["allocated"]))
    res["combine_bytes"] = nbytes
    if res["combine_us"]:
        rate = nbytes / (res["combine_us"][0] * 1e-6)
        res["combine_tb_per_s"] = round(rate / 1e12, 3)
        res["combine_of_hbm_peak"] = round(rate / HBM_PEAK, 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
