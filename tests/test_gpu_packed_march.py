"""The march's hand-packed fp32 (tap_weights, tap_coords: x and y of a sample as one f32x2) through
every path that casts rays, bit for bit against the oracle and against each other.

A packed instruction's two components are the scalar instructions' results, so nothing may move.  What can go wrong is
the pairing itself -- a y value in the x half, a weight taken from the wrong half, a pair formed on one route of
tap_coords and not on the other -- and that shows on any scene, so the scenes are the two smallest committed ones: S1 at
64x48 with 4 cm voxels (tests/golden/s1_64x48_p4.npz) and at 48x36 with 2 cm voxels and gradients
(s1_48x36_p2_gradients.npz), fused offline (alloc run to its fixed point).  Each is rendered from three poses: a pose of
its orbit, a pose beside the orbit, and a voxel-aligned one -- the camera on the voxel lattice with the grid's axes, so
that rows and columns of rays lie on voxel boundaries and lanes on tap_coords' exact route sit beside lanes on the
certified one -- by

  * k_render with complete tile lists (the LDS-only lookup),
  * k_render with lists of four entries, which overflow (the general lookup),
  * k_render_large (the pipelined march: taps_issue / taps_finish),
  * k_render_hash,
  * k_query_rays on the view's camera rays,

and by k_render and k_render_large once more with 64-bit voxel addresses: those kernels keep the scalar weights (the
scenes' pools are small, so all of the above address voxels by 32-bit offsets and run the packed ones).

The paths are forced as tests/test_gpu_render_lookups.py and tests/test_gpu_query.py force them."""
import ctypes as C
import os

import numpy as np
import pytest

import ray_query as RQ
import tile_intervals as TI
from helpers import assert_maps_equal, bits
from test_golden import GOLDEN, setup
from test_gpu_query import query_rays
from test_gpu_render_lookups import render_hash, render_intervals
from voxelhashing_amd import canonical, synth, vhtypes as T

pytestmark = pytest.mark.gpu
f32 = np.float32
CAP_OVERFLOW = 4
SCENES = {"p4": "s1_64x48_p4", "p2_gradients": "s1_48x36_p2_gradients"}
POSES = ("orbit", "beside", "aligned")


def aligned_pose(voxel, eye_voxels):
    """camera -> world: the grid's axes, the eye a whole number of voxels from the origin on every axis"""
    m = np.eye(4)
    m[:3, 3] = np.asarray(eye_voxels, np.float64) * voxel
    return m.astype(f32).reshape(16)


_rigs = {}


def rig(E, O, name):
    """the scene on the device and in the oracle, the three poses and the oracle's maps for each; built once"""
    if name not in _rigs:
        g = np.load(os.path.join(GOLDEN, SCENES[name] + ".npz"))
        hp, cp, rp, opt, spheres, inside, radius = setup(g)
        g_scene, o_scene = E.CUDASceneRepHashSDF(hp, opt), O.OracleScene(hp, cp, rp, opt)
        frame = E.DepthFrame(cp)
        frames = [int(k) for k in g["frames"]]
        for k in frames:
            pose = synth.orbit_pose(k, 100, radius)
            E.synth_frame(spheres, inside, pose, cp, out=frame)
            g_scene.integrate(pose, frame, cp, None)
            o_scene.integrate(pose, *O.synth_frame(spheres, inside, pose, cp))
        canonical.assert_same_scene(g_scene.state(), o_scene.state(), name)
        voxel = float(hp.m_virtualVoxelSize)
        # the voxel-aligned camera looks along +z at the part of the big sphere the orbit's frames saw, from about 2.5 m
        # before z = 0 (off the sphere's axis: from a lattice point on it no sample of the 4 cm scene comes within the
        # margin of a voxel boundary near the surface -- test_the_aligned_pose_takes_both_routes counts them)
        eye = (7, -3, -64) if name == "p4" else (round(0.6 / voxel), 0, -round(2.52 / voxel))
        poses = dict(orbit=synth.orbit_pose(frames[0], 100, radius), beside=synth.orbit_pose(frames[-1] + 2, 100, radius),
                     aligned=aligned_pose(voxel, eye))
        want = {k: o_scene.render(p) for k, p in poses.items()}
        _rigs[name] = dict(hp=hp, cp=cp, rp=rp, gradients=bool(rp.m_useGradients), poses=poses, want=want, g_scene=g_scene, o_scene=o_scene)
    return _rigs[name]


@pytest.fixture(scope="module")
def E(vh):
    from voxelhashing_amd import engine
    yield engine
    for r in _rigs.values():
        r["g_scene"].close()
        r["o_scene"].close()
    _rigs.clear()


def finish(vh, lib, ray, gradients, W, H):
    """the maps of a launcher-level render as CUDARayCastSDF::render leaves them: without gradients the normals come
    from the depth map"""
    if not gradients:
        rd = ray.getRayCastData()
        lib.check(vh.vh_compute_normals(rd.d_normals, rd.d_depth4, W, H, None))
    return ray.download()


def tiles_hit(maps, W, H):
    hit = maps["depth"] != -np.inf
    out = np.zeros(((H + 7) // 8) * ((W + 7) // 8), bool)
    ys, xs = np.nonzero(hit)
    out[(ys // 8) * ((W + 7) // 8) + xs // 8] = True
    return out


@pytest.mark.parametrize("which", POSES)
@pytest.mark.parametrize("name", list(SCENES))
def test_every_ray_casting_path_equals_the_oracle(vh, E, oracle_lib, name, which):
    from voxelhashing_amd import lib
    r = rig(E, oracle_lib, name)
    hp, cp, gradients, pose, want = r["hp"], r["cp"], r["gradients"], r["poses"][which], r["want"][which]
    W, H = cp.m_imageWidth, cp.m_imageHeight
    n_hit = int((want["depth"] != -np.inf).sum())
    print(f"\n{name}, {which}: the oracle's render has {n_hit} hit pixels of {W * H}")
    assert n_hit >= 300, "the oracle's render is all but empty"
    hd, hpp = r["g_scene"].getHashData(), r["g_scene"].getHashParams()
    rp = RQ.view_params(oracle_lib, r["rp"], pose)
    ray = E.CUDARayCastSDF(rp)
    try:
        got = {}
        # the object's own render (the splat's lists, the launch the frame loop makes)
        ray.render(hd, hpp, cp, pose)
        got["CUDARayCastSDF::render"] = ray.download()
        render_hash(vh, lib, ray, hd, hpp, cp, rp, W, H)
        got["k_render_hash"] = finish(vh, lib, ray, gradients, W, H)
        _, heads, _ = render_intervals(vh, lib, ray, hd, hpp, cp, rp, W, H, TI.CAP_SMALL)
        got["k_render, complete lists"] = finish(vh, lib, ray, gradients, W, H)
        count = heads[:, 2]
        complete = (count > 0) & (count <= TI.CAP_SMALL)
        assert (complete & tiles_hit(want, W, H)).any(), "no tile with a complete list hits the surface"
        if name == "p4":
            assert (count <= TI.CAP_SMALL).all(), f"every list was meant to be complete at 4 cm: longest {count.max()}"
        _, heads, _ = render_intervals(vh, lib, ray, hd, hpp, cp, rp, W, H, CAP_OVERFLOW)
        got["k_render, overflowed lists"] = finish(vh, lib, ray, gradients, W, H)
        over = heads[:, 2] > CAP_OVERFLOW
        assert (over & tiles_hit(want, W, H)).sum() >= 4, "the tiles that hit the surface were meant to have overflowed lists"
        _, heads, _ = render_intervals(vh, lib, ray, hd, hpp, cp, rp, W, H, TI.CAP_LARGE)
        got["k_render_large"] = finish(vh, lib, ray, gradients, W, H)
        assert ((heads[:, 2] > 0) & (heads[:, 2] <= TI.CAP_LARGE) & tiles_hit(want, W, H)).any()
        # the same two kernels with 64-bit voxel addresses, whose weights are the scalar code: pair against scalar directly
        try:
            assert vh.vh_debug_render_force_offsets64(1) == 0
            render_intervals(vh, lib, ray, hd, hpp, cp, rp, W, H, TI.CAP_SMALL)
            got["k_render, 64-bit addresses (scalar weights)"] = finish(vh, lib, ray, gradients, W, H)
            render_intervals(vh, lib, ray, hd, hpp, cp, rp, W, H, TI.CAP_LARGE)
            got["k_render_large, 64-bit addresses (scalar weights)"] = finish(vh, lib, ray, gradients, W, H)
        finally:
            vh.vh_debug_render_force_offsets64(0)
    finally:
        ray.close()
    for path, maps in got.items():
        assert np.array_equal(maps["depth"] != -np.inf, want["depth"] != -np.inf), f"{name}, {which}: {path}: validity"
        assert_maps_equal(maps, want, f"{name}, {which}: {path} against the oracle")
    paths = list(got)
    for a in range(len(paths)):
        for b in range(a + 1, len(paths)):
            assert_maps_equal(got[paths[a]], got[paths[b]], f"{name}, {which}: {paths[a]} against {paths[b]}")

    # k_query_rays on the camera rays: what the maps hold for its results (the identities of tests/test_query_reference.py)
    cam = RQ.camera_rays(r["o_scene"].L, cp, rp)
    q = query_rays(hd, hpp, rp, cam["origins"], cam["directions"], cam["t_min"], cam["t_max"], normals=gradients)
    n = W * H
    hit = q["status"] == RQ.HIT
    assert np.array_equal(hit, want["depth"].reshape(n) != -np.inf), f"{name}, {which}: k_query_rays: validity"
    with np.errstate(all="ignore"):
        depth = q["t"] / cam["depth_to_ray_length"]
    assert np.array_equal(bits(depth[hit]), bits(want["depth"].reshape(n)[hit])), f"{name}, {which}: k_query_rays: depth bits"
    rgb = np.stack([q["color"] & 0xff, (q["color"] >> 8) & 0xff, (q["color"] >> 16) & 0xff], axis=-1).astype(f32) / f32(255)
    assert np.array_equal(bits(rgb[hit]), bits(want["colors"].reshape(n, 4)[hit, :3])), f"{name}, {which}: k_query_rays: colour bits"
    if gradients:
        normals = np.stack([RQ.mat_mul_d(rp.m_viewMatrix, v) for v in q["normal"][hit]])
        assert np.array_equal(bits(normals), bits(want["normals"].reshape(n, 4)[hit, :3])), f"{name}, {which}: k_query_rays: normal bits"


def test_the_aligned_pose_takes_both_routes(E, oracle_lib):
    """tap_coords' decision in numpy for the voxel-aligned pose's rays, at the march samples within ten increments before
    each ray's hit (samples the device takes whatever the tile's interval): some tile -- the 64 lanes of a wave -- has, in
    the same march step, a lane within the ray's margin of a voxel boundary (the exact route) beside lanes that are not"""
    for name in SCENES:
        r = rig(E, oracle_lib, name)
        cp, hp, pose = r["cp"], r["hp"], r["poses"]["aligned"]
        rp = RQ.view_params(oracle_lib, r["rp"], pose)
        cam = RQ.camera_rays(r["o_scene"].L, cp, rp)
        W, H = cp.m_imageWidth, cp.m_imageHeight
        rvs = f32(1) / f32(hp.m_virtualVoxelSize)
        inc = f32(rp.m_rayIncrement)
        want = r["want"]["aligned"]
        hit = (want["depth"] != -np.inf).reshape(-1)
        o, d = cam["origins"].astype(f32), cam["directions"].astype(f32)
        t_hit = np.where(hit, want["depth"].reshape(-1) * cam["depth_to_ray_length"], f32(np.inf)).astype(f32)
        oq, dq = (o * rvs).astype(f32), (d * rvs).astype(f32)
        Q = f32(1) + np.abs(oq).sum(axis=1) + np.abs(cam["t_max"]) * np.abs(dq).sum(axis=1)
        lim = (f32(0.5) - Q * f32(16.0 / 16777216.0)).astype(f32)
        tiles = ((np.arange(H)[:, None] // 8) * ((W + 7) // 8) + np.arange(W)[None, :] // 8).reshape(-1)
        t = cam["t_min"].astype(f32).copy()
        both, n_exact = 0, 0
        for _ in range(int(np.ceil(float((cam["t_max"] - cam["t_min"]).max()) / float(inc))) + 1):
            near = hit & (t <= t_hit) & (t_hit - t <= f32(10) * inc)
            if near.any():
                q = (t[:, None].astype(np.float64) * dq.astype(np.float64) + oq.astype(np.float64)).astype(f32)  # the fma
                dev = np.abs((q - np.floor(q)) - f32(0.5)).max(axis=1)
                exact = near & ~(dev < lim)
                n_exact += int(exact.sum())
                for tile in np.unique(tiles[exact]):
                    both += bool((near & ~exact & (tiles == tile)).any())
            t = (t + inc).astype(f32)
        print(f"\n{name}: {n_exact} samples on the exact route, {both} (tile, step) pairs with lanes on both routes")
        assert both >= 1, f"{name}: no wave of the aligned pose has lanes on both routes in one step"
