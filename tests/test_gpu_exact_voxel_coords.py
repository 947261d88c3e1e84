"""The ray march on its exact route, and the voxel and block coordinates every kernel forms, against the oracle bit for bit.

tap_coords (vh_ray_sample.hpp) takes the fused route for a sample whose position is certainly not within rounding distance of a
voxel boundary, and the reference's own arithmetic -- world_to_vvp1_rb, vvp_to_block1 -- for the others; one uncertain lane
sends its whole wave there.  The scenes below put the camera where that happens all the time:

  * `aligned`:  the camera a whole number of voxels from the origin on every axis, looking down -z, +x and -y (the image
                plane's axes are the grid's: rows and columns of rays start on voxel boundaries);
  * `negative`: the same, camera and scene moved so that every block has negative indices on all three axes (the
                rounding's sign, the block's floor division);
  * `far`:      camera and scene about 3 000 m from the origin: |position / voxel| is beyond 65 536, ray_setup gives the fused
                route up (certLim = -1) and every sample of every ray is exact.

Each scene: 64x48, 4 cm voxels, the three views integrated (alloc and integrate compared through the canonical snapshot),
then each view rendered without and with gradients.  Plus vh_debug_check_fast_math, whose kernel holds round_half_away and
vvp_to_block1 against the reference's expressions.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_maps_equal, small_config
from voxelhashing_amd import canonical, synth, vhtypes as T

pytestmark = pytest.mark.gpu

VOXEL = synth.PARAM_SETS["P4"]["voxel_size"]
DISTANCE = 63  # voxels between camera and the big sphere's centre: 2.52 m

# camera axes as columns (right, down, forward), right x down = forward
VIEWS = {
    "-z": ((-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, -1.0)),
    "+x": ((0.0, 0.0, -1.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)),
    "-y": ((1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, -1.0, 0.0)),
}
# where the scene's centre lies, in voxels
CENTRES = {
    "aligned": (0, 0, 0),
    "negative": (-184, -128, -92),       # (-7.36, -5.12, -3.68) m: scene and cameras in the all-negative octant
    "far": (50000, -40000, 40000),       # (2000, -1600, 1600) m, 3 020 m from the origin; sum |position / voxel| = 130 000
}


def scene_of(name):
    """-> (spheres, [camera-to-world float32[16] per view]): S1 about the centre, a camera DISTANCE voxels before it per view"""
    centre = np.array(CENTRES[name], dtype=np.float64) * VOXEL
    spheres = synth.S1_SPHERES.copy()
    spheres[:, :3] += centre
    poses = []
    for right, down, fwd in VIEWS.values():
        at = (np.array(CENTRES[name], dtype=np.float64) - DISTANCE * np.array(fwd)) * VOXEL
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, down, fwd, at
        poses.append(m.astype(np.float32).reshape(16))
    return spheres, poses


_rigs = {}


def rig(E, O, name):
    """the scene integrated on the device and in the oracle, once per module"""
    if name not in _rigs:
        hp, cp, rp = small_config(64, 48, "P4")
        opt = T.make_scene_options(offline=True, gc=False)
        spheres, poses = scene_of(name)
        g_scene, o_scene = E.CUDASceneRepHashSDF(hp, opt), O.OracleScene(hp, cp, rp, opt)
        frame = E.DepthFrame(cp)
        for pose in poses:
            E.synth_frame(spheres, 0, pose, cp, out=frame)
            depth, color = O.synth_frame(spheres, 0, pose, cp)
            g_scene.integrate(pose, frame, cp, None)
            o_scene.integrate(pose, depth, color)
        _rigs[name] = dict(hp=hp, cp=cp, poses=poses, g_scene=g_scene, o_scene=o_scene)
    return _rigs[name]


@pytest.fixture(scope="module")
def E(vh):
    from voxelhashing_amd import engine
    yield engine
    for r in _rigs.values():
        r["g_scene"].close()
        r["o_scene"].close()
    _rigs.clear()


@pytest.mark.parametrize("voxel,buckets", [(0.04, 500000), (0.01, 2000000)])
def test_rounding_and_block_division_on_the_device(vh, voxel, buckets):
    """k_check_fast_math at 1 M operands: round_half_away == (int)(p + sign(p) / 2) on every quotient, vvp_to_block1 == the
    reference's division on the rounded voxel and on raw 32-bit patterns (word 0, with div_exact); umod_fast (word 1)"""
    from voxelhashing_amd.lib import DeviceBuffer, check
    buf = DeviceBuffer(8)
    check(vh.vh_debug_check_fast_math(C.c_float(voxel), buckets, 1 << 20, 424242, buf.ptr, None), "check")
    mism = buf.download(np.uint32)
    assert mism[0] == 0, f"division, rounding or block division differs from the reference's on {mism[0]} operands"
    assert mism[1] == 0, f"umod_fast differs from % on {mism[1]} operands"


@pytest.mark.parametrize("name", list(CENTRES))
def test_alloc_and_integrate(E, oracle_lib, name):
    """alloc's DDA and the integrate pass form their voxels and blocks with the same helpers: canonical snapshot == oracle"""
    r = rig(E, oracle_lib, name)
    gs, os_ = r["g_scene"].state(), r["o_scene"].state()
    assert gs["num_occupied"] > 40
    canonical.assert_same_scene(gs, os_, name)
    if name == "negative":
        pos = np.asarray(canonical.compactified_set(gs["compactified"]))
        assert (pos.reshape(len(pos), -1)[:, :3] < 0).all(), "a block with a non-negative index"


@pytest.mark.parametrize("gradients", [False, True])
@pytest.mark.parametrize("name", list(CENTRES))
def test_march_on_the_exact_route(E, oracle_lib, name, gradients):
    r = rig(E, oracle_lib, name)
    rp = T.make_raycast_params(r["hp"], r["cp"], use_gradients=gradients)
    ray = E.CUDARayCastSDF(rp)
    r["o_scene"].rp = rp
    try:
        for view, pose in zip(VIEWS, r["poses"]):
            want = r["o_scene"].render(pose)
            assert (want["depth"] != -np.inf).sum() >= 100, f"{name} {view}: the oracle's render is all but empty"
            for again in range(2):  # (the second render runs on the schedule the first one left)
                ray.render(r["g_scene"].getHashData(), r["g_scene"].getHashParams(), r["cp"], pose)
                assert_maps_equal(ray.download(), want, f"{name}, view {view}, gradients {gradients}, render {again}")
    finally:
        ray.close()
