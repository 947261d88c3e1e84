#!/usr/bin/env python3
"""Measures the scene cut (vh_cut.hip) on the scene tools/bench_merge.py uses: cfg2 (S1, 640x480, 4 cm voxels), an orbit of
--frames frames fused into one scene.  The region is a box with one face through the median of the blocks' x
coordinates and the others far away: about half the blocks.  Four cases, one JSON line each:

  erase        CUDASceneRepHashSDF.eraseRegion: gather, select (which erases: nothing is lifted), delete passes
  crop         cropToRegion: the same launches with the complement selected
  move         moveRegionTo into an empty scene: count (gather, select), lift (gather, select, decide, lift), the merge
               (classify, decide, alloc passes, combine), erase (gather, select, delete passes)
  lift_erase   vh_cut_blocks with VH_CUT_LIFT alone, at the launcher level: select, decide, lift, erase, delete passes
               (the one call in which k_cut_erase runs)

  blocks                  blocks in, touched, freed, lifted; voxels erased
  *_us                    each kernel's own duration [median, least] (vh_time_launch_after: the dispatch's time stamps)
  call_ms                 the whole blocking call on the host clock (its read-backs included)
  select_bytes, select_tb_per_s
                          the select kernel reads every listed block once: 4 KB per block in.  Where it erases too it
                          writes 4 KB per freed block and the selected pairs of the other touched blocks, which are not
                          counted: the rate of an erasing select is a lower bound.
  erase_bytes, erase_tb_per_s
                          k_cut_erase reads nothing: 4 KB written per freed block (the selected voxels of the other
                          touched blocks are not counted: a lower bound)

The cut changes its scene, so every sample rebuilds it first; a sample whose call took another number of delete or
alloc passes than the first one is dropped (the skip count would name another kernel).

    python tools/bench_cut.py [--frames 24] [--reps 7] [--config cfg2] [--scene S1] [--out FILE]"""
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
    ap.add_argument("--scene", default="S1")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
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
    scene, other = E.CUDASceneRepHashSDF(hp, opt), E.CUDASceneRepHashSDF(hp, opt)
    frame = E.DepthFrame(cp)

    def build():
        scene.reset()
        for k in range(a.frames):
            pose = synth.orbit_pose(k, 1000, radius)
            E.synth_frame(spheres, inside, pose, cp, out=frame)
            scene.integrate(pose, frame, cp, None)
        scene.synchronize()

    build()
    positions = scene.state(with_voxels=False)["positions"]
    vs = float(hp.m_virtualVoxelSize)
    centre = (np.median(positions, axis=0) * 8.0 + 4.0) * vs
    centre[0] += 500.0
    region = T.make_cut_region(centre, (500.0, 500.0, 500.0))
    m = E.cut_region_transform(list(region.worldFromRegion), list(region.halfExtents), hp.m_virtualVoxelSize)
    n_blocks = len(positions)
    token = [1 << 30]

    def launcher_lift_erase():
        """vh_cut_blocks with VH_CUT_LIFT on the scene's own table (count first, untimed, to size the staging pool)"""
        hd, shp = scene.getHashData(), scene.getHashParams()
        d_desc, cnt = lib.DeviceBuffer(16 * shp.m_numSDFBlocks), lib.DeviceBuffer(4)
        lib.check(L.vh_merge_gather(C.byref(hd), C.byref(shp), d_desc.ptr, shp.m_numSDFBlocks, cnt.ptr, None), "vh_merge_gather")
        n = int(cnt.download(np.uint32, 1)[0])
        d_work = lib.DeviceBuffer(L.vh_cut_work_bytes(n))
        counts = (C.c_uint32 * len(T.CUT_COUNTS))()
        room = n
        d_out, d_staging = lib.DeviceBuffer(16 * room), lib.DeviceBuffer(4096 * room)
        token[0] += 1
        lib.check(L.vh_cut_blocks(C.byref(hd), C.byref(shp), n, d_desc.ptr, None, m.ctypes.data, T.CUT_BOX, T.CUT_LIFT, token[0], d_work.ptr, d_out.ptr,
                                  d_staging.ptr, room, counts, None), "vh_cut_blocks")
        return {k: int(v) for k, v in zip(T.CUT_COUNTS, counts)}

    cases = {
        "erase": lambda: scene.eraseRegion(region),
        "crop": lambda: scene.cropToRegion(region),
        "move": lambda: scene.moveRegionTo(other, region),
        "lift_erase": launcher_lift_erase,
    }

    def run(case, skip=None):
        """a fresh scene, one call -> (counts, the armed kernel's us or None, the call's ms)"""
        build()
        other.reset()
        other.synchronize()
        if skip is not None:
            lib.check(L.vh_time_launch_after(skip, e0, e1), "vh_time_launch_after")
        t0 = time.perf_counter()
        counts = cases[case]()
        ms_call = 1e3 * (time.perf_counter() - t0)
        us = None
        if skip is not None:
            ms = C.c_float()
            if hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0:
                us = 1e3 * ms.value
        return counts, us, ms_call

    def shape_of(counts):
        return (counts["delete_passes"], counts.get("merge", {}).get("alloc_passes", 0))

    lines = []
    for case in cases:
        first, _, _ = run(case)
        assert first["status"] == 0 and first["unsettled"] == 0, first
        dp, apasses = shape_of(first)
        if case in ("erase", "crop"):
            phases = [("gather", 0), ("select", 1)] + [(f"delete{p}", 2 + p) for p in range(dp)]
        elif case == "lift_erase":  # (its gather is the first timed launch of the case)
            phases = [("gather", 0), ("select", 1), ("decide", 2), ("lift", 3), ("erase", 4)] + [(f"delete{p}", 5 + p) for p in range(dp)]
        else:
            k = 8 + apasses
            phases = [("count_gather", 0), ("count_select", 1), ("lift_gather", 2), ("select", 3), ("decide", 4), ("lift", 5), ("merge_classify", 6)] + \
                     [(f"merge_alloc{p}", 8 + p) for p in range(apasses)] + [("merge_combine", k), ("erase_gather", k + 1), ("erase_select", k + 2)] + \
                     [(f"delete{p}", k + 3 + p) for p in range(dp)]
        res = dict(case=case, lib=os.path.basename(lib.LIB_PATH), config=a.config, scene=a.scene, frames=a.frames, reps=a.reps,
                   blocks={k: first[k] for k in ("blocks_in", "touched", "freed", "lifted")}, voxels_erased=first["voxels_erased"],
                   voxels_lifted=first["voxels_lifted"], delete_passes=dp)
        if case == "move":
            res["merge"] = first["merge"]
        calls, dropped = [], 0
        for name, skip in phases:
            us = []
            for _ in range(3 * a.reps):
                counts, t, ms_call = run(case, skip)
                if shape_of(counts) != (dp, apasses) or t is None:
                    dropped += 1
                    continue
                us.append(t)
                calls.append(ms_call)
                if len(us) == a.reps:
                    break
            res[name + "_us"] = [round(float(np.median(us)), 1), round(float(np.min(us)), 1)] if us else None
        res["samples_dropped"] = dropped
        res["call_ms"] = [round(float(np.median(calls)), 3), round(float(np.min(calls)), 3)] if calls else None
        res["select_bytes"] = 4096 * first["blocks_in"]
        if res.get("select_us"):
            rate = res["select_bytes"] / (res["select_us"][0] * 1e-6)
            res["select_tb_per_s"] = round(rate / 1e12, 3)
            res["select_of_hbm_peak"] = round(rate / HBM_PEAK, 3)
            res["select_erases"] = case in ("erase", "crop")
        if res.get("erase_us"):
            res["erase_bytes"] = 4096 * first["freed"]
            res["erase_tb_per_s"] = round(res["erase_bytes"] / (res["erase_us"][0] * 1e-6) / 1e12, 3)
        assert first["blocks_in"] == n_blocks
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
