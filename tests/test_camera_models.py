"""The oracle, and the numpy restatements the GPU tests lean on, under cameras other than the default one: fx != fy, a
principal point off the image centre (and off the image), other depth limits, truncations and weight caps
(tests/camera_models.py).  With fx == fy and a centred principal point an fx where an fy belongs, a sign error in the
principal point's offset or a cut-off taken from the wrong parameter leaves every bit of the rest of the suite unchanged.

The oracle against the reference's own code compiled for the CPU (oracle/_ref/libvh_ref.so), bit for bit, through the
comparisons of tests/test_reference_pinning.py and tests/test_reference_pinning_kernels.py; the restatements through
the checks of their own test files.  No case passes empty: the lower bounds on blocks, voxels and ray hits are literal
numbers read off the oracle's own run on the CPU (two thirds of what it gave, rounded down), never off the device.
"""
import numpy as np
import pytest

import camera_models as CM
import test_reference_pinning as PIN
import test_reference_pinning_kernels as PINK
from helpers import make_depth
from oracle import oracle as O
from oracle import reference as R
from test_gpu_parity import general_poses
from voxelhashing_amd import synth, vhtypes as T

pytestmark = pytest.mark.skipif(not R.available(), reason="oracle/_ref/libvh_ref.so is not built (build() makes it "
                                "where the reference tree is present)")

SIZE = (96, 72)
RESTATED = ["tum", "tall", "offcentre"]


@pytest.fixture(scope="module")
def libs():
    O.build()
    return O.lib(), R.lib()


def integrated_voxels(scene):
    return int((scene.state()["voxels"]["weight"] > 0).sum())


# ------------------------------------------------------------------------------------------------ device functions

@pytest.mark.parametrize("name", list(CM.CAMERAS))
def test_projection_unprojection_and_frustum(libs, name):
    hp, cp, _ = CM.config(name, (64, 48))
    PIN.check_projection_and_back_projection(libs, cp, n=4000)
    inside = PIN.check_block_in_frustum(libs, hp, cp, seed=len(name), stride=2)
    assert inside > 300  # the oracle's count is 1 900 (tall) to 9 700 (fisheyeish)
    # the cameras are what they are named for
    k = CM.intrinsics(name, 640, 480)
    assert (k["fx"], k["fy"], k["mx"], k["my"]) == pytest.approx(CM.CAMERAS[name])
    assert cp.fx != cp.fy
    if name == "crop":
        assert cp.mx > cp.m_imageWidth


# ------------------------------------------------------------------------------------------------ kernels

# per camera: (live blocks after the last frame, integrated voxels, most ray hits of a frame) of the oracle's own run
# of test_kernels_under_a_camera's frames, times 2/3
KERNEL_COUNTS = {"tum": (150, 33000, 2000), "tall": (131, 29000, 2300), "wide": (134, 31000, 2800),   # oracle: 226 / 49 550 / 3 101, 197 / 43 938 / 3 528, 202 / 46 603 / 4 202
                 "offcentre": (146, 33000, 2300), "crop": (131, 31000, 2800), "fisheyeish": (163, 36000, 980)}  # 219 / 50 046 / 3 565, 197 / 47 180 / 4 326, 245 / 54 902 / 1 477


def frames_for(cp, n, seed, pset=None):
    back = CM.parameter_set(pset)["back"] if pset else 0.0
    return CM.place(general_poses(n, seed), cp, back)


def kernels_under(hp, cp, poses, what):
    """alloc, integrate, starve, GC free, render and normals one by one on the oracle's state; then the online frame
    loop with the reference's compactify and GC identify in it; then the ray cast with gradients of that scene
    -> (live blocks, integrated voxels, most ray hits, the frame loop's oracle scene)"""
    hits = PIN.check_kernels_on_one_state(hp, cp, CM.SPHERES, poses)
    _, a, b = PINK.check_frame_loop_with_gc(hp, cp, CM.SPHERES, poses)
    n = PINK._assert_same_compactify(a, b, R.RefScene(b), f"{what}: compactify")
    assert n > 0
    a.rp.m_useGradients = 1
    want = a.render(poses[-2])
    got = R.RefScene(b).render(a.rp)
    PIN._maps_equal(want, got, f"{what}: ray cast with gradients")
    assert (want["normals"][want["depth"] != -np.inf][:, :3] != -np.inf).any()
    return a.state()["num_occupied"], integrated_voxels(a), hits, a


@pytest.mark.parametrize("name", list(CM.CAMERAS))
def test_kernels_under_a_camera(libs, name):
    hp, cp, _ = CM.config(name, SIZE, buckets=1 << 14, blocks=1 << 12)
    blocks, voxels, hits, _ = kernels_under(hp, cp, frames_for(cp, 4, 1), name)
    print(f"{name}: {blocks} blocks, {voxels} voxels, {hits} hits")
    want = KERNEL_COUNTS[name]
    assert blocks >= want[0] and voxels >= want[1] and hits >= want[2], (blocks, voxels, hits)


# per parameter set under tum: the same three counts, times 2/3
PSET_COUNTS = {"near": (66, 17000, 1600), "thin": (92, 17000, 1800),               # oracle: 100 / 25 840 / 2 516, 138 / 25 941 / 2 792
               "thin_scaled": (158, 34000, 2100), "saturating": (150, 33000, 2000)}  # 237 / 52 376 / 3 160, 226 / 49 550 / 3 101


@pytest.mark.parametrize("pset", list(CM.PARAMETER_SETS))
def test_kernels_under_a_parameter_set(libs, pset):
    hp, cp, _ = CM.config("tum", SIZE, pset=pset, buckets=1 << 14, blocks=1 << 12)
    poses = frames_for(cp, 4, 1, pset)
    blocks, voxels, hits, _ = kernels_under(hp, cp, poses, pset)
    print(f"{pset}: {blocks} blocks, {voxels} voxels, {hits} hits")
    want = PSET_COUNTS[pset]
    assert blocks >= want[0] and voxels >= want[1] and hits >= want[2], (blocks, voxels, hits)
    cuts = cuts_taking_effect(pset, SIZE, poses)
    print(f"{pset}: {cuts}")
    if pset == "near":
        # the oracle, same frames: 19 361 more voxels with the default integration distance, 140 more ray hits with the
        # default depth range
        assert cuts["voxels_refused_by_max_integration_distance"] >= 12000 and cuts["pixels_refused_by_depth_max"] >= 90, cuts
    if pset == "saturating":
        assert cuts["voxels_at_weight_max"] >= 450, cuts  # the oracle: 682 after the last frame
    # the truncation band is 3.2 voxels, and 4 voxels more per metre in thin_scaled, where the default is 5 voxels and 2.5
    # more per metre: the oracle integrates 25 941 (thin) and 52 376 (thin_scaled) voxels, 49 550 with the default band
    if pset == "thin":
        assert cuts["voxels_with_default_truncation"] - cuts["voxels"] >= 15000, cuts
    if pset == "thin_scaled":
        assert cuts["voxels"] - cuts["voxels_with_default_truncation"] >= 1800, cuts


def oracle_run(hp, cp, rp, poses):
    """the online frame loop on the oracle alone -> (scene, ray hits of every render of the previous pose)"""
    sc = O.OracleScene(hp, cp, rp, T.make_scene_options(offline=False, gc=True, starve=2))
    hits = []
    for k, q in enumerate(poses):
        if k > 0:
            hits.append(int((sc.render(poses[k - 1])["depth"] != -np.inf).sum()))
        sc.integrate(q, *O.synth_frame(CM.SPHERES, 0, q, cp))
    return sc, hits


def cuts_taking_effect(pset, size, poses, voxels="P4", camera="tum", **table):
    """what a parameter set's cuts do, by the oracle alone: the same frames with one limit at a time put back to its
    default"""
    hp, cp, rp = CM.config(camera, size, voxels, pset, **table)
    sc, hits = oracle_run(hp, cp, rp, poses)
    out = dict(voxels=integrated_voxels(sc), hits=sum(hits),
               voxels_at_weight_max=int((sc.state()["voxels"]["weight"] == hp.m_integrationWeightMax).sum()))
    if pset == "near":
        far = T.make_hash_params(hp.m_hashNumBuckets, hp.m_numSDFBlocks, **synth.PARAM_SETS[voxels])  # integration distance 4 m
        out["voxels_refused_by_max_integration_distance"] = integrated_voxels(oracle_run(far, cp, rp, poses)[0]) - out["voxels"]
        deep = CM.camera(camera, *size, depth_min=cp.m_sensorDepthWorldMin)  # depth_max 5 m
        out["pixels_refused_by_depth_max"] = sum(oracle_run(hp, deep, T.make_raycast_params(hp, deep), poses)[1]) - out["hits"]
    if pset in ("thin", "thin_scaled"):
        plain = T.make_hash_params(hp.m_hashNumBuckets, hp.m_numSDFBlocks, **synth.PARAM_SETS[voxels])
        out["voxels_with_default_truncation"] = integrated_voxels(oracle_run(plain, cp, T.make_raycast_params(plain, cp), poses)[0])
    return out


# ------------------------------------------------------------------------------------------------ sensor maps

@pytest.mark.parametrize("name", list(CM.CAMERAS))
@pytest.mark.parametrize("w,h", [(33, 9), (101, 77)])
def test_depth_to_camera_space(libs, name, w, h):
    depth = make_depth(w, h, 4, holes=0.1)
    cp = CM.camera(name, w, h)
    out = PINK._same("convert_depth_float_to_camera_space_float4", depth, w, h, cp, out_channels=4)
    ok = depth != -np.inf
    assert ok.sum() > 0.8 * w * h and np.array_equal(PIN.bits(out[..., 2][ok]), PIN.bits(depth[ok]))
    # x and y carry the two focal lengths: the same pixel offset from the principal point gives x / y = fy / fx
    assert np.isfinite(out[..., :2][ok]).all()


# ------------------------------------------------------------------------------------------------ restatements

def ray_query_model(name):
    """tests/test_query_reference.py's model under a named camera: S1 at 64x48 (P4), three offline frames, rendered with
    gradients from a fourth pose"""
    hp, cp, rp = CM.config(name, (64, 48), gradients=True)
    o = O.OracleScene(hp, cp, rp, T.make_scene_options(offline=True))
    # (crop's aimed view is filled by the sphere: from 0.7 m further back a third of its rays miss)
    poses = CM.place([synth.orbit_pose(k, n_frames=100) for k in (0, 1, 2, 5)], cp, back=0.7 if name == "crop" else 0.0, offset=0.0)
    for pose in poses[:3]:
        o.integrate(pose, *O.synth_frame(synth.S1_SPHERES, 0, pose, cp))
    maps = o.render(poses[3])
    return dict(O=O, o=o, cp=cp, rp=o.rp, maps=maps, view=poses[3], poses=poses[:3])


@pytest.mark.parametrize("name", RESTATED + ["crop"])
def test_ray_query_restatement(libs, name):
    """tests/ray_query.py's camera rays and march reproduce the oracle's render (at least 1000 hits and 1000 misses)"""
    import test_query_reference as TQ
    TQ.test_camera_rays_reproduce_the_oracle_render(ray_query_model(name))


@pytest.fixture(scope="module")
def tile_blocks():
    import tile_intervals as TI
    return {t: TI.oracle_blocks(O, t) for t in ("A", "P8")}


@pytest.mark.parametrize("gradients", [False, True])
@pytest.mark.parametrize("view", ["orbit_2cm", "tilted_8cm"])
@pytest.mark.parametrize("name", RESTATED)
def test_tile_interval_rule(libs, tile_blocks, name, view, gradients):
    """tests/tile_intervals.py: the splat's rule (float32, the kernel's order) lists every (tile, block) pair the float64
    slab test needs, and its depth ranges hold the needed ones (more than 500 needed pairs)"""
    import test_tile_intervals as TT
    import tile_intervals as TI
    table, W, H, pose = TI.VIEWS[view]
    cp = CM.camera(name, W, H)
    pose = CM.place([pose], cp, offset=0.0)[0]
    v = TI.View(view, TI.table_frames(table)[0], (table, W, H, pose))
    v.cp = cp
    blocks = tile_blocks[table]
    case = dict(view=v, blocks=blocks, need=TI.needed_for(v, blocks, gradients), model=TI.model_for(v, blocks, gradients))
    TT.test_the_rule_lists_every_needed_pair({(view, gradients): case}, view, gradients)


@pytest.mark.parametrize("name", RESTATED)
def test_icp_restatement_recovers_a_known_motion(libs, name):
    """oracle/icp.py (and tests/icp_reference.py's solve in it) at the bounds of tests/test_camera_tracking.py"""
    import test_camera_tracking as TC
    hp, cp, rp = CM.config(name, (160, 120), "P2", buckets=1 << 14, blocks=1 << 13)
    TC.oracle_icp_recovers_a_known_motion(O, hp, cp, rp, CM.aim(cp))


@pytest.mark.parametrize("name", RESTATED)
def test_rgbd_restatement_tracks_in_plane_motion(libs, name):
    """tests/rgbd_icp.py at the bounds of tests/test_rgbd_tracking.py"""
    import test_rgbd_tracking as TR
    TR.restatement_tracks_in_plane_motion(CM.camera(name, 160, 120))


@pytest.mark.parametrize("name", RESTATED)
def test_view_render_restatement(libs, name, monkeypatch):
    """tests/view_render.py: the plane covers the screen, a depth step leaves a gap -- under the named camera's K"""
    import test_view_rendering as TV
    import view_render as V
    W, H = 64, 48
    k = CM.intrinsics(name, W, H)
    K = V.intrinsics(k["fx"] * 50.0 / 52.5, k["fy"] * 50.0 / 52.5, k["mx"], k["my"])  # (the test's own plane case has f = 50 at 64x48)
    monkeypatch.setattr(TV, "_plane_case", lambda: (np.full((H, W), 1.0, np.float32), K))
    TV.test_restatement_plane_covers_the_screen()
    TV.test_restatement_depth_step_leaves_a_gap()
