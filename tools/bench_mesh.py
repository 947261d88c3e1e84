#!/usr/bin/env python3
"""Measures the marching-cubes extraction on the bench scene: cfg2 after `--frames` frames of the
S1 orbit (or cfg3's 1 cm voxels with --config cfg3), `--reps` extractions, HIP-event time of pass 1 + pass 2 on the
stream, and the CPU oracle on the same scene for comparison.  One JSON line.

    python tools/bench_mesh.py [--config cfg2] [--frames 100] [--reps 20] [--no-cpu]

--indexed measures the indexed extraction instead ("Indexed mesh") at the launcher level, on the same
scene: each kernel's own duration (vh_time_launch_after: the dispatch's time stamps; median of --reps) for the plain
pass 2, the sourced pass 2 and the three weld kernels, the bytes each route downloads, and the wall time of the host
merge (mergeCloseVertices + removeDuplicateFaces inside saveMesh) on the same soup.

    python tools/bench_mesh.py --indexed [--config cfg3] [--frames 100] [--reps 20]

--indexed --streamed puts the same scene behind a chunk grid (the config's 1 m chunks) and measures the two routes of a
streamed scene ("Indexed mesh over several extractions") in one process: the wall time of the soup
walk (extractIsoSurface(chunkGrid)) and of saveMesh's merge of that soup, the wall time of the indexed walk
(extractIsoSurfaceIndexed(chunkGrid)), the bytes each downloads, and -- at the launcher level, over the same boxes on
the resident scene -- each append's three kernels by vh_time_launch_after (one accumulation per kernel; --reps of them).

    python tools/bench_mesh.py --indexed --streamed [--config cfg3] [--frames 100] [--reps 5]

--normals (with --indexed, also with --streamed) adds the vertex-normal pass ("Vertex normals"): the
two kernels' own durations over the welded mesh (over the finished accumulation with --streamed), the bytes the normals
add to the download, and the wall time of the extraction (of the indexed walk) with the option on beside the one with it
off.

    python tools/bench_mesh.py --indexed --normals [--streamed] [--config cfg3]

--components (with --indexed) adds the component pass ("Mesh components"): each of its kernels by
vh_time_launch_after, the pass as a share of the indexed extraction's kernels, the serial alternative it replaces (the
download of the welded mesh and the labelling of tests/mesh_components.py on the host), and the wall time of the
extraction with the filter on beside the one with it off.

    python tools/bench_mesh.py --indexed --components [--normals] [--config cfg3]

--cluster M (with --indexed) adds the vertex clustering ("Mesh clustering") at M lattice points a
side: each of its four kernels by vh_time_launch_after, the pass as a share of the indexed extraction's kernels,
vertices, faces and download size before and after, and the wall time of the extraction with clustering on beside the
one with it off.  With --streamed: the pass over the finished accumulation, and the indexed walk with it on.

    python tools/bench_mesh.py --indexed --cluster 2 [--streamed] [--config cfg3]

--smooth N (with --indexed) adds N iterations of the Taubin smoothing ("Mesh smoothing"), over the
clustered mesh with --cluster M and else over the welded one: its edge, degree, prepare and finish kernels and the
first half step's gather and step by vh_time_launch_after, the whole pass of 4 N + 4 launches between two events and
what that makes per launch, the edge table's slots beside the edges there are, and the wall time of the extraction
with smoothing on beside the one with it off.  With --streamed: the pass over the finished accumulation (wall clock,
the wait for the counts included), and the indexed walk with it on.

    python tools/bench_mesh.py --indexed --smooth 10 [--cluster 2] [--streamed] [--config cfg3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def indexed_report(args, scene, hp):
    """the two routes from the scene to a mesh, stage by stage"""
    import tempfile
    from voxelhashing_amd import engine as E, lib, vhtypes as T
    L = lib.load()
    hip = C.CDLL("libamdhip64.so")  # the runtime the library already has open: events for vh_time_launch_after
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    hd, hpp = scene.getHashData(), scene.getHashParams()
    mp = T.make_marching_cubes_params(hp, 1 << 22)
    data = T.MarchingCubesData()
    lib.check(L.vh_marching_cubes_data_alloc(C.byref(data), C.byref(mp)), "vh_marching_cubes_data_alloc")
    sources = lib.DeviceBuffer(T.TRIANGLE_SOURCE_DTYPE.itemsize * mp.m_maxNumTriangles)
    lib.check(L.vh_reset_marching_cubes(C.byref(data), None), "reset")
    lib.check(L.vh_extract_iso_surface_pass1(C.byref(hd), C.byref(hpp), C.byref(data), None), "pass1")
    nblk = int(lib.download(data.d_numOccupiedBlocks, np.uint32, 1)[0])

    def timed(skip, launch, before=None):
        us = []
        for i in range(3 + args.reps):
            if before:
                before()
            lib.check(L.vh_time_launch_after(skip, e0, e1), "vh_time_launch_after")
            launch()
            lib.check(L.vh_stream_synchronize(None), "synchronize")
            ms = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0, "the launch did not take the events"
            if i >= 3:
                us.append(1e3 * ms.value)
        return round(float(np.median(us)), 2)

    reset = lambda: lib.check(L.vh_reset_marching_cubes(C.byref(data), None), "reset")  # the triangle counter
    out = dict(blocks=nblk)
    out["pass2_plain_us"] = timed(0, lambda: lib.check(L.vh_extract_iso_surface_pass2(C.byref(hd), C.byref(hpp), C.byref(data), nblk, None), "pass2"), reset)
    out["pass2_sourced_us"] = timed(0, lambda: lib.check(L.vh_extract_iso_surface_pass2_sourced(C.byref(hd), C.byref(hpp), C.byref(data), sources.ptr, nblk, None), "pass2 sourced"), reset)
    n = int(lib.download(data.d_numTriangles, np.uint32, 1)[0])
    assert n < mp.m_maxNumTriangles
    w = T.MeshWeldData()
    lib.check(L.vh_mesh_weld_data_alloc(C.byref(w), n, 0), "vh_mesh_weld_data_alloc")
    weld = lambda: lib.check(L.vh_mesh_weld(data.d_triangles, sources.ptr, n, C.byref(w), 0, None), "vh_mesh_weld")
    for skip, name in enumerate(("weld_insert_us", "weld_number_us", "weld_faces_us")):
        out[name] = timed(skip, weld)
    counts = (C.c_uint32 * 3)()
    lib.check(L.vh_mesh_weld_get_counts(C.byref(w), counts, None), "vh_mesh_weld_get_counts")
    V, F = int(counts[0]), int(counts[1])
    out.update(triangles=n, vertices=V, faces=F, slots_log2=int(w.m_slotsLog2),
               weld_device_bytes=16 * (1 << w.m_slotsLog2) + 40 * 3 * n + 16 * n,
               download_bytes_soup=72 * n, download_bytes_indexed=24 * V + 12 * F)
    if args.normals:
        scale = E.mesh_normals_default_scale_log2(hp.m_virtualVoxelSize)
        acc, nrm, st = lib.DeviceBuffer(24 * V), lib.DeviceBuffer(12 * V), lib.DeviceBuffer(4)
        normals = lambda: lib.check(L.vh_mesh_vertex_normals(w.d_vertices, w.d_keys, w.d_faces, V, F, scale, acc.ptr, nrm.ptr, st.ptr, None), "vh_mesh_vertex_normals")
        for skip, name in enumerate(("normals_faces_us", "normals_finish_us")):
            out[name] = timed(skip, normals)
        assert int(st.download(np.uint32, 1)[0]) == 0, "the default scale left a status"
        out.update(normals_scale_log2=scale, normals_device_bytes=36 * V + 4, download_bytes_normals=12 * V)
        for b in (acc, nrm, st):
            b.free()
    if args.components:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import mesh_components as MC  # the numpy restatement: the host pass a user would run on the downloaded mesh
        bufs = [lib.DeviceBuffer(4 * V), lib.DeviceBuffer(4 * V), lib.DeviceBuffer(4), lib.DeviceBuffer(4 * V), lib.DeviceBuffer(16),
                lib.DeviceBuffer(24 * V), lib.DeviceBuffer(8 * V), lib.DeviceBuffer(12 * F), lib.DeviceBuffer(24)]
        root, cnt, st, newi, best, ov, ok, of, cc = bufs
        label = lambda: lib.check(L.vh_mesh_components(w.d_keys, w.d_faces, V, F, root.ptr, cnt.ptr, st.ptr, None), "vh_mesh_components")
        names = ["components_init_us", "components_hook_us", "components_flatten_us", "components_count_us"]
        for skip, name in enumerate(names):
            out[name] = timed(skip, label)
        filt = lambda: lib.check(L.vh_mesh_components_filter(w.d_vertices, w.d_keys, None, w.d_faces, V, F, root.ptr, cnt.ptr, st.ptr, args.min_component, 1, newi.ptr,
                                                             best.ptr, ov.ptr, ok.ptr, None, of.ptr, cc.ptr, None), "vh_mesh_components_filter")
        more = ["components_stats_us", "components_pick_key_us", "components_pick_index_us", "components_compact_vertices_us", "components_compact_faces_us"]
        for skip, name in enumerate(more):
            out[name] = timed(skip, filt)
        assert int(st.download(np.uint32, 1)[0]) == 0, "the labelling left a status"
        stats = {k: int(v) for k, v in zip(T.COMPONENTS_COUNTS, cc.download(np.uint32, 6))}
        total = sum(out[k] for k in names + more)
        kernels = out["pass2_sourced_us"] + out["weld_insert_us"] + out["weld_number_us"] + out["weld_faces_us"] + out.get("normals_faces_us", 0.0) + out.get("normals_finish_us", 0.0)
        out.update(components=stats, components_min_faces=args.min_component, components_pass_us=round(total, 2),
                   components_share_of_indexed_kernels=round(total / (kernels + total), 4), components_device_bytes=44 * V + 12 * F + 44)
        # the serial alternative: the welded mesh to the host, labelled there
        keys, faces = np.zeros(V, dtype=np.uint64), np.zeros((F, 3), dtype=np.uint32)
        t0 = time.perf_counter()
        lib.check(L.vh_mesh_weld_download(C.byref(w), None, keys.ctypes.data, faces.ctypes.data, V, F, None), "vh_mesh_weld_download")
        t_down = time.perf_counter() - t0
        t0 = time.perf_counter()
        h_root, h_count, h_status = MC.components(keys, faces)
        t_host = time.perf_counter() - t0
        assert h_status == 0 and np.array_equal(h_root, root.download(np.uint32, V)) and np.array_equal(h_count, cnt.download(np.uint32, V))
        out.update(host_labelling_download_s=round(t_down, 5), host_labelling_s=round(t_host, 5))
        for b in bufs:
            b.free()
    if args.cluster:
        scale = E.mesh_cluster_default_scale_log2(hp.m_virtualVoxelSize)
        logs = [C.c_uint32(), C.c_uint32()]
        for count, log in zip((V, F), logs):
            lib.check(L.vh_mesh_cluster_default_slots_log2(count, C.byref(log)), "vh_mesh_cluster_default_slots_log2")
        logs = [int(log.value) for log in logs]
        cs, fs = 1 << logs[0], 1 << logs[1]
        bufs = [lib.DeviceBuffer(n) for n in (8 * cs, 48 * cs, 4 * cs, 4 * cs, 4 * V, 8 * fs, 4 * fs, 4 * fs, 8, 24 * V, 8 * V, 12 * F, 24)]
        cd = T.MeshClusterData(*[b.ptr for b in bufs], logs[0], logs[1])
        run = lambda: lib.check(L.vh_mesh_cluster(w.d_vertices, w.d_keys, w.d_faces, V, F, args.cluster, scale, C.byref(cd), None), "vh_mesh_cluster")
        names = ["cluster_insert_us", "cluster_faces_us", "cluster_number_us", "cluster_emit_us"]
        for skip, name in enumerate(names):
            out[name] = timed(skip, run)
        stats = {k: int(v) for k, v in zip(T.CLUSTER_COUNTS, bufs[12].download(np.uint32, 6))}
        assert stats["status"] == 0, "the clustering left a status"
        total = sum(out[k] for k in names)
        kernels = out["pass2_sourced_us"] + out["weld_insert_us"] + out["weld_number_us"] + out["weld_faces_us"]
        out.update(cluster=stats, cluster_cells=args.cluster, cluster_scale_log2=scale, cluster_pass_us=round(total, 2),
                   cluster_share_of_indexed_kernels=round(total / (kernels + total), 4),
                   cluster_device_bytes=sum(b.nbytes for b in bufs), download_bytes_clustered=24 * stats["vertices"] + 12 * stats["faces"])
        if args.smooth:  # the smoothing below runs over the clustered mesh
            clustered = (bufs[9].ptr, bufs[10].ptr, bufs[11].ptr, stats["vertices"], stats["faces"])
            held = bufs
        else:
            for b in bufs:
                b.free()
    if args.smooth:
        sv, sk, sf, SV, SF = clustered if args.cluster else (w.d_vertices, w.d_keys, w.d_faces, V, F)
        scale = E.mesh_cluster_default_scale_log2(hp.m_virtualVoxelSize)
        log = C.c_uint32()
        lib.check(L.vh_mesh_smooth_default_slots_log2(SF, C.byref(log)), "vh_mesh_smooth_default_slots_log2")
        es = 1 << int(log.value)
        bufs = [lib.DeviceBuffer(n) for n in (8 * es, 4 * es, 4 * SV, 4 * SV, 48 * SV, 24 * SV, 20, 24 * SV, 24)]
        sd = T.MeshSmoothData(*[b.ptr for b in bufs], int(log.value), 0)
        lam, mu = T.SMOOTH_DEFAULT_LAMBDA_Q16, T.SMOOTH_DEFAULT_MU_Q16
        run = lambda: lib.check(L.vh_mesh_smooth(sv, sk, sf, SV, SF, args.smooth, lam, mu, 1, scale, C.byref(sd), None), "vh_mesh_smooth")
        launches = 4 * args.smooth + 4
        for skip, name in ((0, "smooth_edges_us"), (1, "smooth_degree_us"), (2, "smooth_prepare_us"), (3, "smooth_gather_us"), (4, "smooth_step_us"),
                           (launches - 1, "smooth_finish_us")):
            out[name] = timed(skip, run)
        hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        whole = []
        for i in range(3 + args.reps):  # the pass between two events on the null stream, the launches' gaps included
            assert hip.hipEventRecord(e0, None) == 0
            run()
            assert hip.hipEventRecord(e1, None) == 0
            lib.check(L.vh_stream_synchronize(None), "synchronize")
            ms = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
            if i >= 3:
                whole.append(1e3 * ms.value)
        stats = {k: int(v) for k, v in zip(T.SMOOTH_COUNTS, bufs[8].download(np.uint32, 6))}
        assert stats["status"] == 0, "the smoothing left a status"
        total = round(float(np.median(whole)), 2)
        kernels = out["pass2_sourced_us"] + out["weld_insert_us"] + out["weld_number_us"] + out["weld_faces_us"] + out.get("cluster_pass_us", 0.0)
        out.update(smooth=stats, smooth_iterations=args.smooth, smooth_scale_log2=scale, smooth_vertices=SV, smooth_faces=SF, smooth_launches=launches,
                   smooth_pass_us=total, smooth_pass_us_range=[round(min(whole), 2), round(max(whole), 2)], smooth_us_per_launch=round(total / launches, 2),
                   smooth_half_step_kernels_us=round(out["smooth_gather_us"] + out["smooth_step_us"], 2),
                   smooth_share_of_indexed=round(total / (kernels + total), 4), smooth_edge_slots=es, smooth_device_bytes=sum(b.nbytes for b in bufs))
        for b in bufs + (held if args.cluster else []):
            b.free()
    L.vh_mesh_weld_data_free(C.byref(w))
    L.vh_marching_cubes_data_free(C.byref(data))
    # the host merge on the same soup: saveMesh = merge + PLY; the PLY alone is timed on the indexed mesh and taken off
    mc = E.CUDAMarchingCubesHashSDF(mp)
    with tempfile.TemporaryDirectory() as d:
        mc.extractIsoSurface(hd, hpp)
        t0 = time.perf_counter()
        mc.saveMesh(os.path.join(d, "soup.ply"), None, True)
        t_soup = time.perf_counter() - t0
        t0 = time.perf_counter()
        mc.extractIsoSurfaceIndexed(hd, hpp)
        t_indexed = time.perf_counter() - t0
        t0 = time.perf_counter()
        mc.saveMesh(os.path.join(d, "indexed.ply"), None, True)
        t_ply = time.perf_counter() - t0
        if args.normals:  # the whole extraction, option off and on, alternating (the first pair sizes the buffers)
            walls = {False: [], True: []}
            for rep in range(1 + max(args.reps, 3)):
                for on in (False, True):
                    mc.setIndexedNormals(on)
                    t0 = time.perf_counter()
                    mc.extractIsoSurfaceIndexed(hd, hpp)
                    if rep > 0:
                        walls[on].append(time.perf_counter() - t0)
            out.update(extract_indexed_off_wall_s=round(float(np.median(walls[False])), 5), extract_indexed_normals_wall_s=round(float(np.median(walls[True])), 5))
        if args.components:  # the whole extraction, filter off and on, alternating (the first pair sizes the buffers)
            mc.setIndexedNormals(bool(args.normals))
            walls = {False: [], True: []}
            for rep in range(1 + max(args.reps, 3)):
                for on in (False, True):
                    mc.setIndexedComponentFilter(args.min_component if on else 0, False)
                    t0 = time.perf_counter()
                    mc.extractIsoSurfaceIndexed(hd, hpp)
                    if rep > 0:
                        walls[on].append(time.perf_counter() - t0)
            spread = lambda v: [round(float(np.min(v)), 5), round(float(np.median(v)), 5), round(float(np.max(v)), 5)]
            out.update(extract_indexed_filter_off_wall_s=spread(walls[False]), extract_indexed_filter_on_wall_s=spread(walls[True]))
        if args.cluster:  # the whole extraction, clustering off and on, alternating (the first pair sizes the buffers)
            mc.setIndexedNormals(bool(args.normals))
            walls = {False: [], True: []}
            for rep in range(1 + max(args.reps, 3)):
                for on in (False, True):
                    mc.setIndexedClustering(args.cluster if on else 0)
                    t0 = time.perf_counter()
                    mc.extractIsoSurfaceIndexed(hd, hpp)
                    if rep > 0:
                        walls[on].append(time.perf_counter() - t0)
            mc.setIndexedClustering(0)
            spread = lambda v: [round(float(np.min(v)), 5), round(float(np.median(v)), 5), round(float(np.max(v)), 5)]
            out.update(extract_indexed_cluster_off_wall_s=spread(walls[False]), extract_indexed_cluster_on_wall_s=spread(walls[True]))
        if args.smooth:  # the whole extraction (clustered with --cluster), smoothing off and on, alternating (the first pair sizes the buffers)
            mc.setIndexedNormals(bool(args.normals))
            mc.setIndexedClustering(args.cluster)
            walls = {False: [], True: []}
            for rep in range(1 + max(args.reps, 3)):
                for on in (False, True):
                    mc.setIndexedSmoothing(args.smooth if on else 0)
                    t0 = time.perf_counter()
                    mc.extractIsoSurfaceIndexed(hd, hpp)
                    if rep > 0:
                        walls[on].append(time.perf_counter() - t0)
            mc.setIndexedSmoothing(0)
            mc.setIndexedClustering(0)
            spread = lambda v: [round(float(np.min(v)), 5), round(float(np.median(v)), 5), round(float(np.max(v)), 5)]
            out.update(extract_indexed_smooth_off_wall_s=spread(walls[False]), extract_indexed_smooth_on_wall_s=spread(walls[True]))
    out.update(host_merge_s=round(t_soup - t_ply, 4), ply_write_s=round(t_ply, 4), extract_indexed_wall_s=round(t_indexed, 4))
    return out


def streamed_report(args, scene, hp):
    """a streamed scene to a mesh: soup walk + host merge (what there was) against the indexed walk"""
    import tempfile
    from voxelhashing_amd import engine as E, lib, vhtypes as T
    L = lib.load()
    hd, hpp = scene.getHashData(), scene.getHashParams()
    mp = T.make_marching_cubes_params(hp, 1 << 22)
    ext = [hp.m_streamingVoxelExtents[i] for i in range(3)]
    out = dict(chunk_extent_m=ext[0])

    # ---- the appends' kernels, box by box on the resident scene (the boxes of the walk: chunk +- one block)
    hip = C.CDLL("libamdhip64.so")
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    data = T.MarchingCubesData()
    lib.check(L.vh_marching_cubes_data_alloc(C.byref(data), C.byref(mp)), "vh_marching_cubes_data_alloc")
    sources = lib.DeviceBuffer(T.TRIANGLE_SOURCE_DTYPE.itemsize * mp.m_maxNumTriangles)
    f32 = np.float32
    pad = f32(hp.m_virtualVoxelSize) * f32(hp.m_SDFBlockSize)
    reach = 3  # chunks each way from the origin: the S1 scene lies within 1.5 m of it

    def extract_box(chunk):
        c = np.array(chunk, dtype=np.float32) * np.array(ext, dtype=np.float32)
        half = np.array(ext, dtype=np.float32) / f32(2.0)
        mp.m_boxEnabled = 1
        mp.m_minCorner[:] = [float(v) for v in c - half - pad]
        mp.m_maxCorner[:] = [float(v) for v in c + half + pad]
        lib.check(L.vh_reset_marching_cubes(C.byref(data), None), "reset")
        lib.check(L.vh_marching_cubes_update_params(C.byref(data), C.byref(mp), None), "update_params")
        lib.check(L.vh_extract_iso_surface_pass1(C.byref(hd), C.byref(hpp), C.byref(data), None), "pass1")
        nblk = int(lib.download(data.d_numOccupiedBlocks, np.uint32, 1)[0])
        lib.check(L.vh_extract_iso_surface_pass2_sourced(C.byref(hd), C.byref(hpp), C.byref(data), sources.ptr, nblk, None), "pass2 sourced")
        return int(lib.download(data.d_numTriangles, np.uint32, 1)[0])

    chunks = [(x, y, z) for x in range(-reach, reach + 1) for y in range(-reach, reach + 1) for z in range(-reach, reach + 1)]
    chunks = [c for c in chunks if extract_box(c) > 0]
    accum = C.c_void_p()
    lib.check(L.vh_mesh_weld_accum_create(0, 0, 0, C.byref(accum)), "vh_mesh_weld_accum_create")
    names = ("append_insert_us", "append_settle_us", "append_faces_us")
    per_append = {n: [] for n in names}
    counts = (C.c_uint32 * 6)()
    for skip, name in enumerate(names):
        for rep in range(1 + args.reps):  # the first accumulation grows the table and the arrays; the later ones reuse them
            lib.check(L.vh_mesh_weld_accum_begin(accum, None), "vh_mesh_weld_accum_begin")
            us = []
            for c in chunks:
                n = extract_box(c)
                lib.check(L.vh_time_launch_after(skip, e0, e1), "vh_time_launch_after")
                lib.check(L.vh_mesh_weld_accum_append(accum, data.d_triangles, sources.ptr, n, None), "vh_mesh_weld_accum_append")
                lib.check(L.vh_stream_synchronize(None), "synchronize")
                ms = C.c_float()
                assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0, "the launch did not take the events"
                us.append(1e3 * ms.value)
            if rep == 0:
                lib.check(L.vh_mesh_weld_accum_get_counts(accum, counts, None), "vh_mesh_weld_accum_get_counts")
                out.setdefault("doublings_first_accumulation", int(counts[5]))
            else:
                per_append[name].append(us)
    lib.check(L.vh_mesh_weld_accum_get_counts(accum, counts, None), "vh_mesh_weld_accum_get_counts")
    if args.normals:  # over the finished accumulation (the last one above); the first pass makes the buffers
        scale = E.mesh_normals_default_scale_log2(hp.m_virtualVoxelSize)
        for skip, name in enumerate(("normals_faces_us", "normals_finish_us")):
            us = []
            for rep in range(3 + args.reps):
                lib.check(L.vh_time_launch_after(skip, e0, e1), "vh_time_launch_after")
                lib.check(L.vh_mesh_weld_accum_normals(accum, scale, None), "vh_mesh_weld_accum_normals")
                lib.check(L.vh_stream_synchronize(None), "synchronize")
                ms = C.c_float()
                assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0, "the launch did not take the events"
                if rep >= 3:
                    us.append(1e3 * ms.value)
            out[name] = round(float(np.median(us)), 2)
        out.update(normals_scale_log2=scale, download_bytes_normals=12 * int(counts[0]))
    if args.cluster:  # over the finished accumulation (the last one above); the first pass makes the buffers
        scale = E.mesh_cluster_default_scale_log2(hp.m_virtualVoxelSize)
        for skip, name in enumerate(("cluster_insert_us", "cluster_faces_us", "cluster_number_us", "cluster_emit_us")):
            us = []
            for rep in range(3 + args.reps):
                lib.check(L.vh_time_launch_after(skip, e0, e1), "vh_time_launch_after")
                lib.check(L.vh_mesh_weld_accum_cluster(accum, args.cluster, scale, None), "vh_mesh_weld_accum_cluster")
                lib.check(L.vh_stream_synchronize(None), "synchronize")
                ms = C.c_float()
                assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0, "the launch did not take the events"
                if rep >= 3:
                    us.append(1e3 * ms.value)
            out[name] = round(float(np.median(us)), 2)
        kc = (C.c_uint32 * 6)()
        lib.check(L.vh_mesh_weld_accum_cluster_get_counts(accum, kc, None), "vh_mesh_weld_accum_cluster_get_counts")
        out.update(cluster={k: int(kc[i]) for i, k in enumerate(T.CLUSTER_COUNTS)}, cluster_cells=args.cluster, cluster_scale_log2=scale,
                   download_bytes_clustered=24 * int(kc[0]) + 12 * int(kc[1]))
    if args.smooth:  # over the finished accumulation (clustered above with --cluster); the first pass makes the buffers
        scale = E.mesh_cluster_default_scale_log2(hp.m_virtualVoxelSize)
        us = []
        for rep in range(3 + args.reps):
            lib.check(L.vh_stream_synchronize(None), "synchronize")
            t0 = time.perf_counter()
            lib.check(L.vh_mesh_weld_accum_smooth(accum, args.smooth, T.SMOOTH_DEFAULT_LAMBDA_Q16, T.SMOOTH_DEFAULT_MU_Q16, 1, scale, None), "vh_mesh_weld_accum_smooth")
            if rep >= 3:
                us.append(1e6 * (time.perf_counter() - t0))
        sc = (C.c_uint32 * 6)()
        lib.check(L.vh_mesh_weld_accum_smooth_get_counts(accum, sc, None), "vh_mesh_weld_accum_smooth_get_counts")
        out.update(smooth={k: int(sc[i]) for i, k in enumerate(T.SMOOTH_COUNTS)}, smooth_iterations=args.smooth, smooth_scale_log2=scale,
                   smooth_launches=4 * args.smooth + 4, accum_smooth_wall_us=round(float(np.median(us)), 1))
    L.vh_mesh_weld_accum_destroy(accum)
    L.vh_marching_cubes_data_free(C.byref(data))
    for name in names:
        med = np.median(np.array(per_append[name]), axis=0)  # per append, over the accumulations
        out[name] = dict(sum=round(float(med.sum()), 1), largest=round(float(med.max()), 1), median=round(float(np.median(med)), 1))
    out.update(appends_timed=len(chunks), boxes_vertices=int(counts[0]), boxes_faces=int(counts[1]), boxes_dropped=int(counts[4]))

    # ---- the two walks
    pos, radius = (0.0, 0.0, 0.0), 100.0  # everything comes back in at the end of a walk
    dims = [hp.m_streamingGridDimensions[i] for i in range(3)]
    mn = [hp.m_streamingMinGridPos[i] for i in range(3)]
    grid = E.CUDASceneRepChunkGrid(scene, ext, dims, mn, hp.m_streamingInitialChunkListSize, True, 4)
    mc = E.CUDAMarchingCubesHashSDF(mp)
    try:
        with tempfile.TemporaryDirectory() as d:
            walls = dict(soup_walk_s=[], soup_save_s=[], indexed_walk_s=[], indexed_save_s=[])
            normal_walks, cluster_walks, smooth_walks = [], [], []
            for rep in range(1 + max(args.reps, 3)):  # the first pair of walks sizes every buffer
                t0 = time.perf_counter()
                mc.extractIsoSurfaceChunkGrid(grid, pos, radius)
                t1 = time.perf_counter()
                soup_vertices = len(mc.mesh()["vertices"])
                t2 = time.perf_counter()
                mc.saveMesh(os.path.join(d, "soup.ply"), None, True)
                t3 = time.perf_counter()
                mc.extractIsoSurfaceIndexedChunkGrid(grid, pos, radius)
                t4 = time.perf_counter()
                stats = mc.indexed_stats()
                t5 = time.perf_counter()
                mc.saveMesh(os.path.join(d, "indexed.ply"), None, True)
                t6 = time.perf_counter()
                if rep > 0:
                    for k, v in zip(walls, (t1 - t0, t3 - t2, t4 - t3, t6 - t5)):
                        walls[k].append(v)
                if args.normals:
                    mc.setIndexedNormals(True)
                    t7 = time.perf_counter()
                    mc.extractIsoSurfaceIndexedChunkGrid(grid, pos, radius)
                    if rep > 0:
                        normal_walks.append(time.perf_counter() - t7)
                    mc.setIndexedNormals(False)
                    mc.clearMeshBuffer()
                if args.cluster:
                    mc.setIndexedClustering(args.cluster)
                    t8 = time.perf_counter()
                    mc.extractIsoSurfaceIndexedChunkGrid(grid, pos, radius)
                    if rep > 0:
                        cluster_walks.append(time.perf_counter() - t8)
                    mc.setIndexedClustering(0)
                    mc.clearMeshBuffer()
                if args.smooth:
                    mc.setIndexedClustering(args.cluster)
                    mc.setIndexedSmoothing(args.smooth)
                    t9 = time.perf_counter()
                    mc.extractIsoSurfaceIndexedChunkGrid(grid, pos, radius)
                    if rep > 0:
                        smooth_walks.append(time.perf_counter() - t9)
                    mc.setIndexedSmoothing(0)
                    mc.setIndexedClustering(0)
                    mc.clearMeshBuffer()
    finally:
        grid.close()
    w = {k: float(np.median(v)) for k, v in walls.items()}
    out.update(walk_pairs=len(walls["soup_walk_s"]), soup_walk_min_s=round(min(walls["soup_walk_s"]), 4), indexed_walk_min_s=round(min(walls["indexed_walk_s"]), 4))
    n_soup = soup_vertices // 3
    out.update(soup_walk_s=round(w["soup_walk_s"], 4), soup_merge_s=round(w["soup_save_s"] - w["indexed_save_s"], 4),
               ply_write_s=round(w["indexed_save_s"], 4), indexed_walk_s=round(w["indexed_walk_s"], 4),
               soup_route_s=round(w["soup_walk_s"] + w["soup_save_s"] - w["indexed_save_s"], 4),
               soup_triangles=n_soup, download_bytes_soup=72 * n_soup,
               download_bytes_indexed=24 * stats["vertices"] + 12 * stats["faces"], walk=stats)
    if args.normals:
        out.update(indexed_walk_normals_s=round(float(np.median(normal_walks)), 4), indexed_walk_normals_min_s=round(min(normal_walks), 4))
    if args.cluster:
        out.update(indexed_walk_cluster_s=round(float(np.median(cluster_walks)), 4), indexed_walk_cluster_min_s=round(min(cluster_walks), 4))
    if args.smooth:
        out.update(indexed_walk_smooth_s=round(float(np.median(smooth_walks)), 4), indexed_walk_smooth_min_s=round(min(smooth_walks), 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--indexed", action="store_true", help="measure the indexed extraction stage by stage instead")
    ap.add_argument("--streamed", action="store_true", help="--indexed: the scene behind a chunk grid; soup walk + host merge against the indexed walk")
    ap.add_argument("--normals", action="store_true", help="--indexed: add the vertex-normal pass: its two kernels, its download, the extraction with it on and off")
    ap.add_argument("--components", action="store_true", help="--indexed: add the component pass: its kernels, its share of the extraction, the labelling on the host beside it")
    ap.add_argument("--min-component", type=int, default=100, help="--components: the filter's minFaces")
    ap.add_argument("--cluster", type=int, default=0, metavar="M", help="--indexed: add the vertex clustering at M (1 ... 64) lattice points a side: its kernels, the mesh before and after, the extraction with it on and off")
    ap.add_argument("--smooth", type=int, default=0, metavar="N", help="--indexed: add N (1 ... 100) iterations of the Taubin smoothing, over the clustered mesh with --cluster: its kernels, the pass, the extraction with it on and off")
    args = ap.parse_args()
    if args.smooth and (not args.indexed or not 1 <= args.smooth <= 100):
        ap.error("--smooth needs --indexed, and 1 ... 100 iterations")
    if args.cluster and (not args.indexed or not 1 <= args.cluster <= 64):
        ap.error("--cluster needs --indexed, and 1 ... 64 lattice points a side")
    if args.normals and not args.indexed:
        ap.error("--normals needs --indexed")
    if args.components and (not args.indexed or args.streamed):
        ap.error("--components needs --indexed, without --streamed")

    import torch
    from voxelhashing_amd import engine as E, synth, vhtypes as T
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    cfg = dict(synth.CONFIGS[args.config])
    cfg["num_sdf_blocks"] = min(cfg["num_sdf_blocks"], 1 << 18)
    hp, cp, rp = synth.config_params(cfg)
    spheres, inside, radius = synth.scene(cfg["scene"])
    scene = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=True, gc=True))  # offline: a reproducible block set
    frame = E.DepthFrame(cp)
    poses = [synth.orbit_pose(k, 1000, radius) for k in range(args.frames)]
    for pose in poses:
        E.synth_frame(spheres, inside, pose, cp, out=frame)
        scene.integrate(pose, frame, cp, None)
    if args.indexed and args.streamed:
        out = dict(metric="indexed mesh of a streamed scene: walls (s), per-append kernel times (us), download sizes (bytes)",
                   config=dict(workload=f"{args.config} after {args.frames} frames of the S1 orbit, behind its chunk grid", voxel_size=hp.m_virtualVoxelSize))
        out.update(streamed_report(args, scene, hp))
        print(json.dumps(out))
        return
    if args.indexed:
        out = dict(metric="indexed mesh: kernel times (us), download sizes (bytes) and the host merge (s)",
                   config=dict(workload=f"{args.config} after {args.frames} frames of the S1 orbit", voxel_size=hp.m_virtualVoxelSize))
        out.update(indexed_report(args, scene, hp))
        print(json.dumps(out))
        return
    mp = T.make_marching_cubes_params(hp, 1 << 22)
    mc = E.CUDAMarchingCubesHashSDF(mp)
    hd, hpp = scene.getHashData(), scene.getHashParams()
    mc.extractIsoSurfaceWithoutCopy(hd, hpp)  # warm-up
    torch.cuda.synchronize()
    counts = mc.counts()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)  # default stream = the engine's
    ev0.record()
    for _ in range(args.reps):
        mc.extractIsoSurfaceWithoutCopy(hd, hpp)
    ev1.record()
    torch.cuda.synchronize()
    ms = ev0.elapsed_time(ev1) / args.reps
    nblk, ntri = counts["occupied_blocks"], counts["triangles"]
    # algorithmic bytes: every voxel of every allocated block once (8 B) + its entry (20 B) + the triangles written (72 B)
    alg = nblk * (512 * 8 + 20) + ntri * 72
    out = dict(metric="marching cubes: allocated blocks/s (extractIsoSurface pass1+pass2, incl. the blocking block count)",
               value=round(nblk / (ms * 1e-3), 1), unit="blocks/s", ms_per_extraction=round(ms, 4), blocks=nblk, triangles=ntri,
               voxels_per_s=round(nblk * 512 / (ms * 1e-3)), algorithmic_bytes=alg,
               config=dict(workload=f"{args.config} after {args.frames} frames of the S1 orbit", voxel_size=hp.m_virtualVoxelSize))
    if not args.no_cpu:
        from oracle import oracle as O
        o = O.OracleScene(hp, cp, None, T.make_scene_options(offline=True, gc=True))
        n_cpu = min(args.frames, 12)  # a bounded sample of the same orbit: the oracle integrates at ~2.5 frames/s
        for pose in poses[:n_cpu]:
            d, c = O.synth_frame(spheres, inside, pose, cp)
            o.integrate(pose, d, c)
        t0 = time.perf_counter()
        tris, n = o.extract_iso_surface(mp)
        dt = time.perf_counter() - t0
        nb = len(o.state()["positions"])
        out["cpu_baseline"] = dict(value=round(nb / dt, 1), unit="blocks/s", cores=1, kind="port",
                                   sample=f"oracle scene after {n_cpu} frames: {nb} blocks, {n} triangles, {dt:.2f} s")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
