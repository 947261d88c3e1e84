"""The HIP kernels against the reference's own code compiled for the CPU (oracle/_ref/libvh_ref.so), with no oracle
in between: the host side runs the reference's reset, alloc (offline passes), integrate and render kernels through
its serial launch emulator, and takes compactify's set from the reference's frustum test (oracle/reference.py).
Only oracle/_ref/ is read, never the reference tree."""
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
