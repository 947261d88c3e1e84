#!/usr/bin/env python3
"""Measures the scene registration (vh_align.hip) on cfg2 (S1, 640x480, 4 cm voxels): a scene is built from an orbit of
--frames frames, a second one from the same frames at displaced poses (so the truth is known: 1 degree about (1, 2, 3)
through the origin the orbit circles, and 1.5 voxels), and the second is registered to the first from identity.  One
JSON line is printed:

  blocks                  source blocks (one workgroup each), destination blocks
  step_us                 every step launch's own duration, in order (vh_time_next_launch: the dispatch's time stamps)
  count                   contributing voxels per step
  voxels_per_us           contributing voxels per microsecond of step kernel, [median, best] over the steps
  step_ns_per_block       the median step's duration per source block
  iterations, status      steps to VH_ALIGN_CONVERGED; error_deg / error_voxel against the truth
  call_ms                 CUDASceneRepHashSDF.alignScene as a whole on the host clock, [median, least]
  resample_us, resample_ns_per_block
                          the yardstick: k_resample_blocks on the same source list under the found transform, in this
                          process: the same block lookups and one eight-tap sample per voxel against seven here
  step_over_resample      step_ns_per_block / resample_ns_per_block
  accumulate_us           the step kernel with a count gate that no scene passes: everything but the one-lane 6x6 solve
                          and the pose update, [median, least]; accumulate_ns_per_block and accumulate_over_resample
                          as above (the question DESIGN.md section 6 answers: more than 7?)

    python tools/bench_align.py [--frames 24] [--reps 7] [--config cfg2] [--scene S1] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--config", default="cfg2", choices=["cfg1", "cfg2", "cfg3", "cfg4"])
    ap.add_argument("--scene", default="S1")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = ap.parse_args()
    from voxelhashing_amd import engine as E, lib, synth, vhtypes as T
    from voxelhashing_amd.lib import DeviceBuffer
    L = lib.load()
    hip = C.CDLL("libamdhip64.so")  # the runtime the library already has open: events for vh_time_next_launch
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0

    hp, cp, rp = synth.config_params(a.config)
    vs = float(hp.m_virtualVoxelSize)
    spheres, inside, radius = synth.scene(a.scene)
    opt = T.make_scene_options(offline=False, gc=True, starve=15)
    dst, src = E.CUDASceneRepHashSDF(hp, opt), E.CUDASceneRepHashSDF(hp, opt)
    frame = E.DepthFrame(cp)
    truth = np.eye(4)
    truth[:3, :3] = rotation((1, 2, 3), np.radians(1.0))
    truth[:3, 3] = np.array([2.0, -1.0, 1.5]) / np.linalg.norm([2.0, -1.0, 1.5]) * 1.5 * vs
    back = np.linalg.inv(truth)
    for k in range(a.frames):
        pose = synth.orbit_pose(k, 1000, radius)
        E.synth_frame(spheres, inside, pose, cp, out=frame)
        dst.integrate(pose, frame, cp, None)
        # the same depth map seen from the pose as the source's world has it: dstFromSrc = truth
        moved = (back @ np.asarray(pose, np.float64).reshape(4, 4)).astype(np.float32).reshape(16)
        src.integrate(moved, frame, cp, None)
    dst.synchronize()
    src.synchronize()

    def timed():
        ms = C.c_float()
        return 1e3 * ms.value if hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0 else None

    # the handle level: the whole call
    calls = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        found = dst.alignScene(src)
        calls.append(1e3 * (time.perf_counter() - t0))
    P = found["dst_from_src"]
    c = (np.trace(P[:3, :3] @ truth[:3, :3].T) - 1.0) / 2.0
    err_deg, err_vox = float(np.degrees(np.arccos(np.clip(c, -1, 1)))), float(np.linalg.norm(P[:3, 3] - truth[:3, 3]) / vs)

    # the launcher level: every step launch timed
    dhd, dhp, shd, shp = dst.getHashData(), dst.getHashParams(), src.getHashData(), src.getHashParams()
    cap = int(shp.m_numSDFBlocks)
    d_desc, d_cnt = DeviceBuffer(16 * cap), DeviceBuffer(4)
    lib.check(L.vh_merge_gather(C.byref(shd), C.byref(shp), d_desc.ptr, cap, d_cnt.ptr, None), "vh_merge_gather")
    n = int(d_cnt.download(np.uint32, 1)[0])
    d_state, d_ticket = DeviceBuffer(C.sizeof(T.AlignState)), DeviceBuffer(4)
    lib.check(L.vh_memset(d_ticket.ptr, 0, 4, None), "memset")
    guess = np.ascontiguousarray(np.eye(4), np.float64)
    pivot = np.ascontiguousarray(found["pivot"], np.float32)
    o = T.make_align_options()
    step_us, counts, status = [], [], 0
    lib.check(L.vh_align_begin(d_state.ptr, guess.ctypes.data, vs, vs, pivot.ctypes.data, 1.0 / found["inv_radius"], None), "vh_align_begin")
    for _ in range(o.maxIterations):
        lib.check(L.vh_time_next_launch(e0, e1), "vh_time_next_launch")
        lib.check(L.vh_align_step(C.byref(dhd), C.byref(dhp), C.byref(shd), C.byref(shp), n, d_desc.ptr, o.band, o.minCount, o.condThres, o.rotThres,
                                  o.transThres, d_state.ptr, d_ticket.ptr, None), "vh_align_step")
        lib.check(L.vh_stream_synchronize(None), "synchronize")
        st = T.AlignState.from_buffer_copy(d_state.download(np.uint8, C.sizeof(T.AlignState)).tobytes())
        step_us.append(timed())
        counts.append(int(st.count[st.iterations - 1]))
        status = int(st.status)
        if status:
            break

    # the step kernel without its solve: a count gate no scene passes refuses the step once the totals are summed, so
    # this is the lookups, the samples, the reduction, the adds and the hand-off, under the found transform
    m = np.ascontiguousarray(P, np.float64)
    accumulate_us = []
    for _ in range(a.reps):
        lib.check(L.vh_align_begin(d_state.ptr, m.ctypes.data, vs, vs, pivot.ctypes.data, 1.0 / found["inv_radius"], None), "vh_align_begin")
        lib.check(L.vh_time_next_launch(e0, e1), "vh_time_next_launch")
        lib.check(L.vh_align_step(C.byref(dhd), C.byref(dhp), C.byref(shd), C.byref(shp), n, d_desc.ptr, o.band, 0xFFFFFFFF, o.condThres, o.rotThres,
                                  o.transThres, d_state.ptr, d_ticket.ptr, None), "vh_align_step")
        lib.check(L.vh_stream_synchronize(None), "synchronize")
        accumulate_us.append(timed())

    # the yardstick: the resampler on the same list, under the found transform
    ma, mb = np.zeros(12, np.float32), np.zeros(12, np.float32)
    lib.check(L.vh_resample_voxel_transforms(m.ctypes.data, vs, vs, ma.ctypes.data, mb.ctypes.data), "vh_resample_voxel_transforms")
    slots = max(4, int(16 * max(n, 1) - 1).bit_length())
    d_work = DeviceBuffer(L.vh_resample_work_bytes(slots))
    rc = (C.c_uint32 * len(T.RESAMPLE_COUNTS))()

    def count_call():
        lib.check(L.vh_resample_blocks(C.byref(shd), C.byref(shp), n, d_desc.ptr, ma.ctypes.data, mb.ctypes.data, slots, d_work.ptr, None, None, 0, rc, None),
                  "vh_resample_blocks")
        assert int(rc[4]) == 0 and int(rc[1]) > 0, list(rc)
        return int(rc[1])

    cand = count_call()
    d_out, d_staging = DeviceBuffer(16 * cand), DeviceBuffer(8 * T.SDF_BLOCK_VOXELS * cand)
    resample_us = []
    for _ in range(a.reps):
        # a fill call appends to the staged list from where the header's count stands: the count call, which clears
        # the header, comes before every fill (it finds the same candidates)
        assert count_call() == cand
        lib.check(L.vh_time_next_launch(e0, e1), "vh_time_next_launch")
        lib.check(L.vh_resample_blocks(C.byref(shd), C.byref(shp), n, d_desc.ptr, ma.ctypes.data, mb.ctypes.data, slots, d_work.ptr, d_out.ptr, d_staging.ptr,
                                       cand, rc, None), "vh_resample_blocks")
        assert int(rc[2]) <= cand, list(rc)
        resample_us.append(timed())

    per_us = [c / t for c, t in zip(counts, step_us) if t]
    med_step = float(np.median(step_us))
    res = dict(lib=os.path.basename(lib.LIB_PATH), config=a.config, scene=a.scene, frames=a.frames, reps=a.reps,
               blocks=dict(source=n),
               step_us=[round(t, 1) for t in step_us], count=counts,
               voxels_per_us=[round(float(np.median(per_us)), 1), round(float(np.max(per_us)), 1)],
               step_ns_per_block=round(1e3 * med_step / max(n, 1), 2),
               iterations=found["iterations"], status=found["status"], launcher_status=status, error_deg=round(err_deg, 5), error_voxel=round(err_vox, 5),
               condition=[round(v, 1) for v in found["condition"]],
               call_ms=[round(float(np.median(calls)), 3), round(float(np.min(calls)), 3)],
               resample=dict(candidates=cand, staged=int(rc[2])),
               resample_us=[round(float(np.median(resample_us)), 1), round(float(np.min(resample_us)), 1)],
               resample_ns_per_block=round(1e3 * float(np.median(resample_us)) / cand, 2))
    res["step_over_resample"] = round(res["step_ns_per_block"] / res["resample_ns_per_block"], 2)
    res["accumulate_us"] = [round(float(np.median(accumulate_us)), 1), round(float(np.min(accumulate_us)), 1)]
    res["accumulate_ns_per_block"] = round(1e3 * float(np.median(accumulate_us)) / max(n, 1), 2)
    res["accumulate_over_resample"] = round(res["accumulate_ns_per_block"] / res["resample_ns_per_block"], 2)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "a").write(line + "\n")


if __name__ == "__main__":
    main()
