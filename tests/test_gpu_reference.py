"""The HIP kernels against the reference's own code compiled for the CPU (oracle/_ref/libvh_ref.so), with no oracle
in between: the host side runs the reference's kernels through its launch emulator (oracle/reference.py) -- reset,
alloc, compactifyHashAllInOneKernel and GC identify (on fibers, barrier by barrier), integrate, starve, GC free,
render, the streaming passes, marching cubes and the CameraUtil.cu maps.  Only oracle/_ref/ is read, never the
reference tree.

The reference's compactify is serial on the CPU: about 12 s per call at cfg2's 500 k buckets (5 M entries), so
test_integrate_and_ray_cast_at_cfg2_size (three calls) and the launcher test at cfg2's table (one) spend most of their
time there; the GC sequence uses 2^16 buckets (about 1.5 s per call)."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_maps_equal
from oracle import oracle as O
from oracle import reference as R
from voxelhashing_amd import canonical, synth, vhtypes as T

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not R.available(), reason="oracle/_ref/libvh_ref.so is not built")]

OFF = np.array([7.3, 5.1, 3.7])


def _poses(n, radius):
    out = []
    for k in range(n):
        q = np.array(synth.orbit_pose(k, 200, radius), dtype=np.float32).copy()
        q[3] += np.float32(OFF[0]); q[7] += np.float32(OFF[1]); q[11] += np.float32(OFF[2])
        out.append(q)
    return out


def _bits_equal(a, b, what):
    for k in ("depth", "depth4", "colors"):
        assert np.array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32)), f"{what}: {k}"


def test_integrate_and_ray_cast_at_cfg2_size(vh):
    """640x480, 4 cm voxels, cfg2's 500 k buckets; S1 moved off the origin; three frames offline"""
    from voxelhashing_amd import engine as E
    c = dict(synth.CONFIGS["cfg2"])
    c.update(num_sdf_blocks=1 << 16)
    hp, cp, rp = synth.config_params(c)
    spheres, inside, radius = synth.scene("S1")
    spheres = spheres.copy()
    spheres[:, :3] += OFF
    poses = _poses(3, radius)
    scene, ray = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=True, gc=False)), E.CUDARayCastSDF(rp)
    frame = E.DepthFrame(cp)
    host = O.OracleScene(hp, cp, rp)  # host buffers only: every step below is the reference's code
    ref = R.RefScene(host)
    ref.reset()
    for k, pose in enumerate(poses):
        E.synth_frame(spheres, inside, pose, cp, out=frame)
        scene.integrate(pose, frame, cp, None)
        depth, color = O.synth_frame(spheres, inside, pose, cp)
        ref.set_transform(pose)
        ref.alloc_offline(depth, color)
        ref.compactify()
        ref.integrate_depth_map(depth, color)
        canonical.assert_same_scene(scene.state(), host.state(), f"frame {k}: GPU vs reference")
    ray.render(scene.getHashData(), scene.getHashParams(), cp, poses[-1])
    got = ray.download()
    want = ref.render(ray.getRayCastParams())
    want["normals"] = R.compute_normals(want["depth4"])
    assert_maps_equal(got, want, "ray cast: GPU vs reference")
    assert (want["depth"] != -np.inf).sum() > 20000


def test_render_large_at_cfg3_tables(vh):
    """k_render_large (tile lists of the large capacity) at cfg3's tables -- 2 M buckets, 1 cm voxels -- against the
    reference's renderKernel on the GPU's own table and voxels"""
    from voxelhashing_amd import engine as E, lib
    c = dict(synth.CONFIGS["cfg3"])
    c.update(num_sdf_blocks=1 << 16)
    hp, cp, rp = synth.config_params(c)
    spheres, inside, radius = synth.scene("S1")
    spheres = spheres.copy()
    spheres[:, :3] += OFF
    poses = _poses(2, radius)
    scene, full = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=True, gc=False)), E.CUDARayCastSDF(rp)
    frame = E.DepthFrame(cp)
    for pose in poses:
        E.synth_frame(spheres, inside, pose, cp, out=frame)
        scene.integrate(pose, frame, cp, None)
    full.setIntervalSplatting(False)
    full.render(scene.getHashData(), scene.getHashParams(), cp, poses[-1])
    L = lib.load()
    n_tiles = ((cp.m_imageWidth + 7) // 8) * ((cp.m_imageHeight + 7) // 8)
    heads, lists = lib.DeviceBuffer(n_tiles * 16), lib.DeviceBuffer(n_tiles * 128 * 16)
    lib.check(L.vh_ray_interval_clear(heads.ptr, cp.m_imageWidth, cp.m_imageHeight, None))
    hd, hpp, rpp, rd = scene.getHashData(), scene.getHashParams(), full.getRayCastParams(), full.getRayCastData()
    lib.check(L.vh_ray_interval_splat(C.byref(hd), C.byref(hpp), C.byref(cp), C.byref(rpp), heads.ptr, lists.ptr, 128,
                                      None, 0, None, None))
    lib.check(L.vh_render_intervals(C.byref(hd), C.byref(hpp), C.byref(rd), C.byref(cp), C.byref(rpp), heads.ptr,
                                    lists.ptr, 128, None, 0, None))
    got = full.download()
    # the reference renders the GPU's table and voxels, copied to the host as they are
    d = scene.download()
    table = np.ascontiguousarray(d["hash"])
    voxels = np.ascontiguousarray(d["sdf_blocks"])
    h = T.HashData()
    h.d_hash, h.d_SDFBlocks = table.ctypes.data, voxels.ctypes.data
    H, W = cp.m_imageHeight, cp.m_imageWidth
    want = dict(depth=np.empty((H, W), np.float32), depth4=np.empty((H, W, 4), np.float32),
                normals=np.empty((H, W, 4), np.float32), colors=np.empty((H, W, 4), np.float32))
    out = T.RayCastData(want["depth"].ctypes.data, want["depth4"].ctypes.data, want["normals"].ctypes.data,
                        want["colors"].ctypes.data)
    R.lib().vhr_render(C.byref(h), C.byref(hpp), C.byref(out), C.byref(cp), C.byref(rpp))
    _bits_equal(got, want, "k_render_large vs reference")
    assert (want["depth"] != -np.inf).sum() > 20000


def test_sensor_maps_against_the_reference(vh):
    """engine.image_op against reference.image_op on one call each: bit for bit, except the exp filters, where validity
    matches exactly and values to 1e-5 relative (the device's expf / exp against the host libm); and
    vh_compute_intensity_and_derivatives bit for bit"""
    from voxelhashing_amd import engine as E, lib
    from helpers import make_color_rgbx, make_depth
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    for w, h in ((1, 1), (7, 5), (33, 9), (101, 77), (640, 480)):
        rgbx, depth = make_color_rgbx(w, h, 3), make_depth(w, h, 4, holes=0.1 if w * h > 1 else 0.0)
        cp = T.make_depth_camera_params(w, h)
        exact = [("convert_color_raw_to_float4", (rgbx, w, h), dict(out_channels=4))]
        colf = R.image_op("convert_color_raw_to_float4", rgbx, w, h, out_channels=4)
        for ow, oh in ((w, h), (max(w // 2, 1), max(h // 2, 1)), (2 * w - 1, 2 * h - 1), (w + 13, max(h - 7, 1))):
            exact.append(("resample_float_map", (depth, w, h), dict(out_size=(ow, oh), prefill=np.full((oh, ow), 7.0, np.float32))))
            exact.append(("resample_float4_map", (colf, w, h), dict(out_channels=4, out_size=(ow, oh),
                                                                     prefill=np.full((oh, ow, 4), 7.0, np.float32))))
        exact.append(("convert_color_to_intensity_float", (colf, w, h), {}))
        exact.append(("convert_depth_float_to_camera_space_float4", (depth, w, h, cp), dict(out_channels=4)))
        for size, thr, frac in ((1, 0.05, 0.3), (5, 0.05, 0.3), (2, 0.01, 0.9)):
            exact.append(("erode_depth_map", (depth, w, h, size, thr, frac), {}))
        for name, args, kw in exact:
            assert np.array_equal(bits(E.image_op(name, *args, **kw)), bits(R.image_op(name, *args, **kw))), (name, w, h)
        for sigma_d, sigma_r in ((1.0, 0.05), (2.5, 0.1), (0.7, 1.0), (4.5, 0.2)):
            for name, src, ch, sr in (("gauss_filter_float_map", depth, 1, sigma_r), ("bilateral_filter_float_map", depth, 1, sigma_r),
                                      ("gauss_filter_float4_map", colf, 4, 10.0 * sigma_r)):
                a = E.image_op(name, src, w, h, sigma_d, sr, out_channels=ch)
                b = R.image_op(name, src, w, h, sigma_d, sr, out_channels=ch)
                assert np.array_equal(a == -np.inf, b == -np.inf), (name, w, h)
                ok = b != -np.inf
                assert np.allclose(a[ok], b[ok], rtol=1e-5, atol=0.0), (name, w, h)
        inten = R.image_op("convert_color_to_intensity_float", colf, w, h)
        d_in = lib.DeviceBuffer.from_numpy(np.ascontiguousarray(inten))
        d_out = lib.DeviceBuffer(w * h * 16)
        lib.check(vh.vh_compute_intensity_and_derivatives(d_in.ptr, w, h, d_out.ptr, None), "intensity_and_derivatives")
        got = d_out.download(np.float32, w * h * 4).reshape(h, w, 4)
        assert np.array_equal(bits(got), bits(R.compute_intensity_and_derivatives(inten))), (w, h)


def _host_copy(d, hp, cp, rp=None):
    """an OracleScene (host buffers only) holding a downloaded device state: table, heap, counter, voxels"""
    host = O.OracleScene(hp, cp, rp)
    for field, key, dt in (("d_hash", "hash", T.HASH_ENTRY_DTYPE), ("d_heap", "heap", np.uint32),
                           ("d_SDFBlocks", "sdf_blocks", T.VOXEL_DTYPE)):
        host.array(field, dt, len(d[key]))[:] = d[key]
    host.array("d_heapCounter", np.uint32, 1)[0] = d["heap_counter"]
    return host


def _sorted_rows(a):
    if a.dtype == T.HASH_ENTRY_DTYPE:  # the device keeps words of its own in the padding
        b = np.zeros(len(a), [("pos", np.int32, 3), ("ptr", np.int32), ("offset", np.uint32)])
        for f in ("pos", "ptr", "offset"):
            b[f] = a[f]
        a = b
    a = np.ascontiguousarray(a)
    return np.sort(a.view(np.dtype((np.void, a.dtype.itemsize))).ravel())


def test_gc_sequence_through_the_frame_loop(vh):
    """cfg2's image and voxel size (640x480, 4 cm), 2^16 buckets, S1 off the origin, online alloc, GC on and starving
    every second frame, through the native frame loop (fused integrate + GC pass, riders): after every frame the
    scene equals the one the reference's alloc, compactify, integrate, starve, GC identify and GC free make, and the
    ray cast of the previous pose equals the reference's renderKernel; blocks are freed"""
    from voxelhashing_amd import engine as E
    hp, cp, rp = synth.config_params("cfg2", num_buckets=1 << 16, num_sdf_blocks=1 << 15)
    opt = T.make_scene_options(offline=False, gc=True, starve=2)
    spheres, inside, radius = synth.scene("S1")
    spheres = spheres.copy()
    spheres[:, :3] += OFF
    poses = _poses(7, radius)
    scene, ray = E.CUDASceneRepHashSDF(hp, opt), E.CUDARayCastSDF(rp)
    host = O.OracleScene(hp, cp, rp, opt)  # host buffers and the loop's options; every step is the reference's code
    ref = R.RefScene(host)
    ref.reset()
    frames = [E.synth_frame(spheres, inside, p, cp) for p in poses]
    recon = E.Reconstruction(scene, ray, None, cp)
    seq = E.Reconstruction.makeFrames(poses, [f.depth_ptr for f in frames], [f.color_ptr for f in frames])
    freed = hits = 0
    for k, pose in enumerate(poses):
        recon.run(seq, k, 1)
        recon.synchronize()
        if k > 0:
            host.render(poses[k - 1])  # sets the view of host.rp as CUDARayCastSDF::render does
            want = ref.render(host.rp)
            want["normals"] = R.compute_normals(want["depth4"])
            assert_maps_equal(ray.download(), want, f"frame {k}: ray cast vs reference")
            hits = max(hits, int((want["depth"] != -np.inf).sum()))
        depth, color = O.synth_frame(spheres, inside, pose, cp)
        freed += ref.integrate(pose, depth, color)
        canonical.assert_same_scene(scene.state(), host.state(), f"frame {k}: GPU vs reference")
    assert freed > 0 and hits > 20000


def test_compactify_and_gc_identify_launchers_at_cfg2_table(vh):
    """vh_compactify at cfg2's full table (500 k buckets) on an integrated state seen from another pose, against
    compactifyHashAllInOneKernel on the downloaded state: count and set; then vh_starve + vh_gc_identify against
    starveVoxelsKernel + garbageCollectIdentifyKernel on the GPU's own compactified list: the decision array"""
    from voxelhashing_amd import engine as E, lib
    hp, cp, rp = synth.config_params("cfg2", num_sdf_blocks=1 << 15)
    spheres, inside, radius = synth.scene("S1")
    spheres = spheres.copy()
    spheres[:, :3] += OFF
    poses = _poses(3, radius)
    g = E.LauncherScene(hp)
    frame = E.DepthFrame(cp)
    for pose in poses[:2]:
        E.synth_frame(spheres, inside, pose, cp, out=frame)
        g.set_transform(pose, R.mat4_inverse(pose))
        counter = lambda: int(lib.download(g.hd.d_heapCounter, np.uint32, 1, g.stream)[0])
        prev = None
        while prev != counter():  # offline alloc: passes until the heap stops moving
            prev = counter()
            g.reset_mutex()
            g.alloc(frame, cp)
        g.compactify(cp)
        g.integrate(frame, cp)
    view = poses[2].copy()
    view[3] += np.float32(2.0)  # moved sideways: part of the scene leaves the frustum
    g.set_transform(view, R.mat4_inverse(view))
    n = g.compactify(cp)
    d = g.download()
    host = _host_copy(d, g.hp, cp)
    ref = R.RefScene(host)
    ref.set_transform(view)
    assert ref.compactify() == n
    live = int((d["hash"]["ptr"] != T.FREE_ENTRY).sum())
    assert 0 < n < live
    assert np.array_equal(_sorted_rows(d["compactified"]), _sorted_rows(host.compactified()))
    # GC identify on the GPU's own list (its order is the device's); weights starved once so that some blocks go
    host.array("d_hashCompactified", T.HASH_ENTRY_DTYPE, n)[:] = d["compactified"]
    g.starve()
    ref.starve()
    g.gc_identify(cp)
    ref.gc_identify()
    got = g.download(with_voxels=False)["decisions"]
    want = host.decisions()
    assert np.array_equal(got, want)
    assert 0 < int((want != 0).sum()) < n


def _launcher_state(hp, positions, seed):
    """a LauncherScene whose blocks are allocated one serial pass each (vh_debug_hash_ops) and whose voxels are
    random, with weights 0 .. 3"""
    from voxelhashing_amd import engine as E, lib
    g = E.LauncherScene(hp)
    ops = []
    for p in positions:
        ops += [(0, *p, 0), (4, 0, 0, 0, 0)]  # alloc, new pass
    g.hash_ops(np.array(ops, dtype=np.int32))
    rng = np.random.default_rng(seed)
    vox = np.zeros(hp.m_numSDFBlocks * T.SDF_BLOCK_VOXELS, T.VOXEL_DTYPE)
    vox["sdf"] = rng.uniform(-0.3, 0.3, len(vox)).astype(np.float32)
    vox["color"] = rng.integers(0, 256, (len(vox), 3))
    vox["weight"] = rng.integers(0, 4, len(vox))
    used = np.zeros(hp.m_numSDFBlocks, bool)  # free blocks stay cleared (deleteVoxel's values), as the table requires
    t = g.download(with_voxels=False)["hash"]
    used[t["ptr"][t["ptr"] != T.FREE_ENTRY] // T.SDF_BLOCK_VOXELS] = True
    free = np.repeat(~used, T.SDF_BLOCK_VOXELS)
    vox[free] = np.zeros(1, T.VOXEL_DTYPE)
    vox["sdf"][free] = 0.0
    lib.check(g.L.vh_memcpy_h2d(g.hd.d_SDFBlocks, vox.ctypes.data, vox.nbytes, g.stream), "voxels")
    return g


def _by_pos(descs, blocks):
    order = np.lexsort((descs["pos"][:, 2], descs["pos"][:, 1], descs["pos"][:, 0]))
    return descs["pos"][order], blocks[order]


def test_stream_out_and_in_launchers(vh):
    """vh_stream_out_pass1/2 and vh_stream_in_pass1/2 against integrateFromGlobalHashPass1/2Kernel and
    chunkToGlobalHashPass1/2Kernel on the same state: descriptors as a set, voxel payloads, the resulting tables;
    stream-in into buckets with room only (the reference's list branch corrupts the table)"""
    from voxelhashing_amd import engine as E
    hp = T.make_hash_params(1 << 12, 1 << 10, **synth.PARAM_SETS["P4"])
    cp = T.make_depth_camera_params(64, 48)
    rng = np.random.default_rng(21)
    pos = np.unique(rng.integers(-12, 13, size=(600, 3)), axis=0)[:500]
    g = _launcher_state(hp, pos, 22)
    d0 = g.download()
    assert np.all(d0["hash"]["offset"] == 0)
    host = _host_copy(d0, g.hp, cp)
    ref = R.RefScene(host)
    cam = np.array([0.3, -0.2, 0.1], np.float32)
    dist = []
    for p in pos:
        w = np.zeros(3, np.float32)
        R.lib().vhr_sdf_block_to_world(C.byref(hp), np.ascontiguousarray(p, np.int32).ctypes.data_as(C.POINTER(C.c_int32)),
                                       w.ctypes.data_as(C.POINTER(C.c_float)))
        v = w - cam
        dist.append(np.sqrt(np.float32(v[0] * v[0] + v[1] * v[1]) + np.float32(v[2] * v[2]), dtype=np.float32))
    radius = float(np.sort(np.array(dist, np.float32))[len(dist) // 2])
    ne = g.hp.m_hashNumBuckets * T.HASH_BUCKET_SIZE
    g.reset_mutex()
    descs, blocks = g.stream_out(ne, 0, radius, cam, T.LOCK_ENTRY, capacity=ne)
    rd = ref.stream_out_pass1(ne, 0, radius, cam)
    rv = ref.stream_out_pass2(rd)
    assert 0 < len(descs) == len(rd) < len(pos)
    assert np.array_equal(_sorted_rows(descs), _sorted_rows(rd))
    gp, gb = _by_pos(descs, blocks)
    hp_, hb = _by_pos(rd, rv)
    assert np.array_equal(gp, hp_) and np.array_equal(gb.view(np.uint8), hb.view(np.uint8))
    canonical.assert_same_scene(g.state(), host.state(), "after stream out")
    # back in, in two parts, the same blocks on both sides
    order = np.random.default_rng(23).permutation(len(rd))
    for part in (order[:9], order[9:]):
        g.reset_mutex()
        ref.reset_mutex()
        g.stream_in(rd[part], rv[part], T.LOCK_ENTRY)
        ref.stream_in(rd[part], rv[part])
        canonical.assert_same_scene(g.state(), host.state(), "after stream in")
    before = _host_copy(d0, g.hp, cp)
    canonical.assert_same_scene(g.state(), before.state(), "out and back in")


def test_marching_cubes_triangle_set(vh):
    """vh_extract_iso_surface_pass1/2 (through CUDAMarchingCubesHashSDF) against the reference's
    extractIsoSurfacePass1/2Kernel on the downloaded state: the triangle set, with and without the box"""
    from voxelhashing_amd import engine as E
    hp, cp, rp = synth.config_params("cfg2", num_buckets=1 << 15, num_sdf_blocks=1 << 14, width=160, height=120)
    spheres, inside, radius = synth.scene("S1")
    spheres = spheres.copy()
    spheres[:, :3] += OFF
    scene = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=True, gc=False))
    frame = E.DepthFrame(cp)
    for pose in _poses(2, radius):
        E.synth_frame(spheres, inside, pose, cp, out=frame)
        scene.integrate(pose, frame, cp, None)
    host = _host_copy(scene.download(), scene.getHashParams(), cp)
    ref = R.RefScene(host)
    mp = T.make_marching_cubes_params(hp, 1 << 19)
    mc = E.CUDAMarchingCubesHashSDF(mp)
    mc.extractIsoSurface(scene.getHashData(), scene.getHashParams())
    want, n = ref.extract_iso_surface(mp)
    assert mc.counts()["triangles"] == n > 200
    assert np.array_equal(_sorted_rows(mc.triangles()), _sorted_rows(want))
    cx = float(np.median(want["v"]["p"][..., 0]))
    mpb = T.make_marching_cubes_params(hp, 1 << 19)
    mpb.m_boxEnabled = 1
    mpb.m_minCorner[:] = [cx, -100.0, -100.0]
    mpb.m_maxCorner[:] = [100.0, 100.0, 100.0]
    mc.extractIsoSurfaceWithoutCopy(scene.getHashData(), scene.getHashParams(), (cx, -100, -100), (100, 100, 100), True)
    want_b, nb = ref.extract_iso_surface(mpb)
    assert 0 < nb < n and mc.counts()["triangles"] == nb
    assert np.array_equal(_sorted_rows(mc.triangles()), _sorted_rows(want_b))

