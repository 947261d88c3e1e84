#!/usr/bin/env python3
"""Measures the frame de-integration (vh_deintegrate.hip) on the scene tools/bench_cut.py uses: cfg2 (S1, 640x480, 4 cm
voxels), an orbit of --frames frames fused into one scene.  The frame taken out is the middle one of the orbit.  Three
JSON lines:

  deintegrate  CUDASceneRepHashSDF.deintegrate: gather, apply, delete passes
  reintegrate  CUDASceneRepHashSDF.reintegrate to a pose 1 cm away: the same launches, then an ordinary integrate
  yardstick    vh_integrate (the unfused k_integrate<false>) of the same frame at the same pose on the same scene, after
               the compactify that lists the blocks in its frustum: it moves the same voxels through the same
               projection, and writes every one of them back

  blocks                  blocks in, processed, changed, freed; voxels changed
  *_us                    each kernel's own duration [median, least] (vh_time_launch_after: the dispatch's time stamps)
  call_ms                 the whole blocking call on the host clock (its read-backs included)
  apply_bytes             4 KB read per processed block, 4 KB written per changed block (a lane writes its pair only if
                          it changed: an upper bound on the writes)
  apply_over_integrate    apply_us / the yardstick's integrate_us, medians
  gather_share, delete_share
                          of the sum of the call's kernel times

The call changes its scene, so every sample rebuilds it first; a sample whose call took another number of delete passes
than the first one is dropped (the skip count would name another kernel).

    python tools/bench_deintegrate.py [--frames 24] [--reps 20] [--config cfg2] [--scene S1] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--reps", type=int, default=20)
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
    scene = E.CUDASceneRepHashSDF(hp, opt)
    frame = E.DepthFrame(cp)
    k0 = a.frames // 2
    pose = np.asarray(synth.orbit_pose(k0, 1000, radius), np.float32).reshape(4, 4)
    moved = pose.copy()
    moved[:3, 3] += np.float32(0.01)

    def build():
        scene.reset()
        for k in range(a.frames):
            p = synth.orbit_pose(k, 1000, radius)
            E.synth_frame(spheres, inside, p, cp, out=frame)
            scene.integrate(p, frame, cp, None)
        E.synth_frame(spheres, inside, pose, cp, out=frame)
        scene.synchronize()

    prepared = {}

    def yardstick_prepare():
        """the compactify that lists the blocks in the frame's frustum, before the launch is armed"""
        scene.setLastRigidTransformAndCompactify(pose, cp)
        n = scene.getNumOccupiedBlocks()
        prepared.update(hd=scene.getHashData(), hp=scene.getHashParams(), n=n)
        assert prepared["hp"].m_numOccupiedBlocks == n
        scene.synchronize()

    def yardstick():
        lib.check(L.vh_integrate(C.byref(prepared["hd"]), C.byref(prepared["hp"]), C.byref(frame.data), C.byref(cp), scene.stream), "vh_integrate")
        return dict(blocks_in=prepared["n"], delete_passes=0, status=0, unsettled=0)

    cases = {
        "deintegrate": lambda: scene.deintegrate(pose, frame, cp),
        "reintegrate": lambda: scene.reintegrate(pose, moved, frame, cp),
        "yardstick": yardstick,
    }

    def run(case, skip=None):
        """a fresh scene, one call -> (counts, the armed kernel's us or None, the call's ms)"""
        build()
        if case == "yardstick":
            yardstick_prepare()
        if skip is not None:
            lib.check(L.vh_time_launch_after(skip, e0, e1), "vh_time_launch_after")
        t0 = time.perf_counter()
        counts = cases[case]()
        scene.synchronize()
        ms_call = 1e3 * (time.perf_counter() - t0)
        us = None
        if skip is not None:
            ms = C.c_float()
            if hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0:
                us = 1e3 * ms.value
        return counts, us, ms_call

    lines, medians = [], {}
    for case in cases:
        first, _, _ = run(case)
        assert first["status"] == 0 and first["unsettled"] == 0, first
        dp = first["delete_passes"]
        if case == "yardstick":
            phases = [("integrate", 0)]
        else:
            phases = [("gather", 0), ("apply", 1)] + [(f"delete{p}", 2 + p) for p in range(dp)]
        res = dict(case=case, lib=os.path.basename(lib.LIB_PATH), config=a.config, scene=a.scene, frames=a.frames, frame=k0, reps=a.reps,
                   blocks={k: first[k] for k in ("blocks_in", "processed", "changed", "freed") if k in first}, delete_passes=dp)
        if "voxels_changed" in first:
            res.update(voxels_changed=first["voxels_changed"], voxels_reset=first["voxels_reset"], voxels_at_cap=first["voxels_at_cap"])
        calls, dropped = [], 0
        for name, skip in phases:
            us = []
            for _ in range(3 * a.reps):
                counts, t, ms_call = run(case, skip)
                if counts["delete_passes"] != dp or t is None:
                    dropped += 1
                    continue
                us.append(t)
                calls.append(ms_call)
                if len(us) == a.reps:
                    break
            res[name + "_us"] = [round(float(np.median(us)), 1), round(float(np.min(us)), 1)] if us else None
            res[name + "_samples"] = len(us)
        res["samples_dropped"] = dropped
        res["call_ms"] = [round(float(np.median(calls)), 3), round(float(np.min(calls)), 3)] if calls else None
        if case == "yardstick":
            res["integrate_bytes"] = 2 * 4096 * first["blocks_in"]
            medians["integrate"] = res["integrate_us"][0] if res["integrate_us"] else None
            medians["integrate_blocks"] = first["blocks_in"]
        else:
            res["apply_bytes"] = 4096 * (first["processed"] + first["changed"])
            kernel_us = {n: res[n + "_us"][0] for n, _ in phases if res.get(n + "_us")}
            total = sum(kernel_us.values())
            if total > 0:
                res["gather_share"] = round(kernel_us.get("gather", 0.0) / total, 3)
                res["delete_share"] = round(sum(v for n, v in kernel_us.items() if n.startswith("delete")) / total, 3)
            medians[case] = res["apply_us"][0] if res["apply_us"] else None
        lines.append(res)
    for res in lines:
        if res["case"] != "yardstick" and medians.get("integrate") and medians.get(res["case"]):
            res["apply_over_integrate"] = round(medians[res["case"]] / medians["integrate"], 3)
            res["integrate_us"] = medians["integrate"]
            res["integrate_blocks"] = medians["integrate_blocks"]
    text = [json.dumps(r) for r in lines]
    for t in text:
        print(t, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
