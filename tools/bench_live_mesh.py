#!/usr/bin/env python3
"""Measures the live mesh (vh_live_mesh.hip) on the scenes tools/bench_mesh.py uses: the S1 orbit at cfg2 (4 cm voxels)
and at cfg3 (1 cm voxels).  --warm frames are fused first and one full update made; then, for each of --reps further
frames of the orbit: the frame is integrated, the live mesh updated, and the same state extracted in full (reset, pass 1,
the sourced pass 2) in the same process.  One JSON line a configuration:

  blocks, triangles        resident blocks and cached triangles after the last frame
  counts                   medians over the frames of what an update counted (vhtypes.LIVE_COUNTS)
  *_us                     each kernel's own duration [median, least] over the frames (vh_time_launch_after: the dispatch's
                           time stamps).  One launch can be armed per call, so there is a live mesh per kernel, all fed
                           the same frames; a frame in which that kernel did not run gives no sample
  update_ms                the whole update on the host clock: vh_live_mesh_update and vh_live_mesh_get_counts, its one
                           wait and the read-back of the counts included
  full_ms, full_pass2_us   the full sourced extraction of the same state on the host clock (its blocking block count
                           and the read-back of the triangle count included), and its pass 2 alone
  update_over_full         update_ms / full_ms, medians
  digest_share             digest_us / the sum of the update's kernel medians
  idle_update_ms, idle_digest_us
                           an update with nothing changed: digest, vanished and dilate run, nothing else
  digest_bytes, digest_tb_s, of_hbm_peak
                           4 KB a resident block over idle_digest_us, against the 8 TB/s DESIGN.md section 6 uses

    python tools/bench_live_mesh.py [--configs cfg2 cfg3] [--warm 40] [--reps 20] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_TB_S = 8.0
PHASES = ("digest", "vanished", "dilate", "drop", "pass2")


def med_min(v, digits=1):
    return [round(float(np.median(v)), digits), round(float(np.min(v)), digits)] if len(v) else None


def measure(config, warm, reps, max_triangles):
    from voxelhashing_amd import engine as E, lib, synth, vhtypes as T
    L = lib.load()
    hip = C.CDLL("libamdhip64.so")  # the runtime the library already has open: events for vh_time_launch_after
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0

    cfg = dict(synth.CONFIGS[config])
    cfg["num_sdf_blocks"] = min(cfg["num_sdf_blocks"], 1 << 18)
    hp, cp, _ = synth.config_params(cfg)
    spheres, inside, radius = synth.scene(cfg["scene"])
    scene = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=True, gc=True))  # as tools/bench_mesh.py
    frame = E.DepthFrame(cp)

    def integrate(k):
        pose = synth.orbit_pose(k, 1000, radius)
        E.synth_frame(spheres, inside, pose, cp, out=frame)
        scene.integrate(pose, frame, cp, None)
        scene.synchronize()

    for k in range(warm):
        integrate(k)
    mp = T.make_marching_cubes_params(hp, max_triangles)
    lives = {name: E.LiveMesh(mp, hp.m_numSDFBlocks) for name in PHASES + ("whole",)}
    full = E.LiveMesh(mp, hp.m_numSDFBlocks)  # its buffers serve the full extraction

    def armed(skip, call):
        """call() with its launch number `skip` timed -> (what call returned, us or None if that launch did not happen)"""
        lib.check(L.vh_time_launch_after(skip, e0, e1), "vh_time_launch_after")
        out = call()
        scene.synchronize()
        ms = C.c_float()
        ok = hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        return out, (1e3 * ms.value if ok else None)

    def update(name, hd, hpp):
        """-> (counts, the armed kernel's us, the whole update's ms)"""
        live = lives[name]
        if name == "whole":
            t0 = time.perf_counter()
            c = live.update(hd, hpp)
            return c, None, 1e3 * (time.perf_counter() - t0)
        skip = PHASES.index(name)
        probe = lives["whole"].last  # the whole-update instance went first: it says which launches this frame has
        ran = dict(digest=True, vanished=True, dilate=True, drop=probe["changed"] + probe["vanished"] > 0 and probe["dropped"] + probe["kept"] > 0,
                   pass2=probe["remeshed"] > 0)
        if not ran[name]:
            return live.update(hd, hpp), None, None
        if name == "pass2" and not ran["drop"]:
            skip -= 1
        c, us = armed(skip, lambda: live.update(hd, hpp))
        return c, us, None

    def full_extraction(hd, hpp, arm):
        def run():
            t0 = time.perf_counter()
            lib.check(L.vh_reset_marching_cubes(C.byref(full.data), None), "vh_reset_marching_cubes")
            lib.check(L.vh_extract_iso_surface_pass1(C.byref(hd), C.byref(hpp), C.byref(full.data), None), "pass 1")
            n = np.zeros(1, np.uint32)
            lib.check(L.vh_memcpy_d2h(n.ctypes.data, full.data.d_numOccupiedBlocks, 4, None), "block count")
            lib.check(L.vh_extract_iso_surface_pass2_sourced(C.byref(hd), C.byref(hpp), C.byref(full.data), full.d_sources, int(n[0]), None), "pass 2")
            lib.check(L.vh_memcpy_d2h(n.ctypes.data, full.data.d_numTriangles, 4, None), "triangle count")
            return 1e3 * (time.perf_counter() - t0), int(n[0])
        if arm:
            (ms, n), us = armed(0, run)
            return ms, n, us
        ms, n = run()
        return ms, n, None

    hd, hpp = scene.getHashData(), scene.getHashParams()
    for name in ("whole",) + PHASES:  # the first update: the full one
        lives[name].last = lives[name].update(hd, hpp)
    full_extraction(hd, hpp, False)

    kernel_us = {p: [] for p in PHASES}
    update_ms, full_ms, full_pass2_us, counts = [], [], [], []
    for k in range(warm, warm + reps):
        integrate(k)
        hd, hpp = scene.getHashData(), scene.getHashParams()
        c, _, ms = update("whole", hd, hpp)
        lives["whole"].last = c
        update_ms.append(ms)
        counts.append(c)
        for p in PHASES:
            cp_, us, _ = update(p, hd, hpp)
            assert {n: cp_[n] for n in T.LIVE_COUNTS} == {n: c[n] for n in T.LIVE_COUNTS}, (p, cp_, c)
            if us is not None:
                kernel_us[p].append(us)
        ms, n, us = full_extraction(hd, hpp, True)
        assert n == c["total"], (n, c)
        full_ms.append(ms)
        ms, _, _ = full_extraction(hd, hpp, False)
        full_ms.append(ms)
        if us is not None:
            full_pass2_us.append(us)

    idle_ms, idle_digest = [], []
    for _ in range(reps):
        c, _, ms = update("whole", hd, hpp)
        assert c["changed"] == c["vanished"] == c["remeshed"] == 0 and c["total"] == counts[-1]["total"], c
        lives["whole"].last = c
        idle_ms.append(ms)
        _, us = armed(0, lambda: lives["digest"].update(hd, hpp))
        if us is not None:
            idle_digest.append(us)

    res = dict(config=config, lib=os.path.basename(lib.LIB_PATH), scene=cfg["scene"], voxel_size=hp.m_virtualVoxelSize, warm_frames=warm, frames=reps,
               blocks=counts[-1]["visited"], triangles=counts[-1]["total"],
               counts={n: int(np.median([c[n] for c in counts])) for n in T.LIVE_COUNTS})
    for p in PHASES:
        res[p + "_us"] = med_min(kernel_us[p])
        res[p + "_samples"] = len(kernel_us[p])
    res["update_ms"] = med_min(update_ms, 3)
    res["full_ms"] = med_min(full_ms, 3)
    res["full_pass2_us"] = med_min(full_pass2_us)
    res["update_over_full"] = round(res["update_ms"][0] / res["full_ms"][0], 3)
    total = sum(res[p + "_us"][0] for p in PHASES if res[p + "_us"])
    res["digest_share"] = round(res["digest_us"][0] / total, 3) if total > 0 else None
    res["idle_update_ms"] = med_min(idle_ms, 3)
    res["idle_digest_us"] = med_min(idle_digest)
    res["digest_bytes"] = 4096 * res["blocks"]
    if res["idle_digest_us"]:
        res["digest_tb_s"] = round(res["digest_bytes"] / (res["idle_digest_us"][0] * 1e-6) / 1e12, 3)
        res["of_hbm_peak"] = round(res["digest_tb_s"] / HBM_PEAK_TB_S, 3)
    for live in list(lives.values()) + [full]:
        live.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["cfg2", "cfg3"], choices=["cfg1", "cfg2", "cfg3", "cfg4"])
    ap.add_argument("--warm", type=int, default=40)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--max-triangles", type=int, default=1 << 22)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    text = []
    for config in a.configs:
        text.append(json.dumps(measure(config, a.warm, a.reps, a.max_triangles)))
        print(text[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
