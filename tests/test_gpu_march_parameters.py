"""The ray casters on the device under the march sets and the wide band of tests/camera_models.py: thresholds at which
the two comparisons that accept a zero crossing are false for most crossings, so that the march resumes behind a
rejected one (the plain march, the pipelined march of the large tile tables, the halves of split tiles and their merge,
the hash-table ray caster, the alloc riders' launch); ray increments of a quarter of the truncation and of two and a
half truncations; and a truncation band wider than a block through alloc, the splat and both shapes of the fused pass.
Under the builders' defaults neither comparison can be false: a k_render without them passes every other test.

The expectation is always the oracle's own render or the oracle's own scene, bit for bit, and
tests/test_march_parameters.py holds the oracle to the reference under the same sets and shows, by the oracle alone,
that these views cross the cuts.  The lower bounds on hits, pixels and blocks are literal numbers read off the oracle's
own run on the CPU (two thirds of what it gave), never off the device; which tiles a schedule splits is the device's
choice, and the split-tile case says where it reports what the device chose."""
import numpy as np
import pytest

import camera_models as CM
import test_march_parameters as M
from helpers import assert_maps_equal, bits, small_config
from voxelhashing_amd import canonical, vhtypes as T

pytestmark = pytest.mark.gpu
B = T.SDF_BLOCK_SIZE


@pytest.fixture(scope="module")
def E(vh):
    from voxelhashing_amd import engine
    return engine


# ------------------------------------------------------------------------------------------------ (a) every ray caster

@pytest.fixture(scope="module")
def all_round_scenes(E, oracle_lib):
    """(camera, voxels) -> (device scene, oracle scene) of tests/test_march_parameters.py's all-round S1, made when first
    asked for and compared once"""
    O = oracle_lib

    class Scenes(dict):
        def __missing__(self, key):
            camera, voxels = key
            hp, cp, _, poses, _ = M.all_round(camera, voxels)
            scene = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=True, gc=False))
            for p in poses:
                scene.integrate(p, E.synth_frame(CM.SPHERES, 0, p, cp), cp, None)
            ref = M.all_round_scene(O, camera, voxels)
            canonical.assert_same_scene(scene.state(), ref.state(), f"{key}: the scene to render")
            self[key] = (scene, ref)
            return self[key]

    scenes = Scenes()
    yield scenes
    for scene, ref in scenes.values():
        scene.close()
        ref.close()


# hits of the four views under the coarse step by the oracle alone, times 2/3 (the gated sets: M.CUTS_VIEWS' third column)
COARSE_HITS = {(None, "P4"): 5980, ("offcentre", "P4"): 6789, (None, "P2"): 19688, ("offcentre", "P2"): 21513}  # oracle: 8 971 / 10 184 / 29 533 / 32 270

RAY_CAST_CASES = ([(c, v, m) for c in (None, "offcentre") for v in ("P4", "P2") for m in CM.MARCH_SETS]
                  + [(c, "P1", m) for c in (None, "offcentre") for m in ("dist_gate", "fine")])


def expected_hits(camera, voxels, march):
    return COARSE_HITS[(camera, voxels)] if march == "coarse" else M.CUTS_VIEWS[(camera, voxels)][march][2]


@pytest.mark.parametrize("camera,voxels,march", RAY_CAST_CASES, ids=lambda v: str(v))
def test_ray_casters_under_a_march_set(E, oracle_lib, vh, all_round_scenes, camera, voxels, march):
    """four views of the all-round scene, with and without gradients, through every ray caster: the engine's own choice,
    the full-range march without the interval splat, the large-tile tables (k_render_large), the small ones, tile lists of
    four entries that overflow into the general lookup, and the hash-table ray caster -- each against the oracle's render,
    bit for bit.  test_ray_cast_paths of tests/test_gpu_camera_models.py, under a march set."""
    from test_gpu_render_lookups import render_hash, render_intervals
    from voxelhashing_amd import lib
    import tile_intervals as TI
    scene, ref = all_round_scenes[(camera, voxels)]
    hp, cp, _, _, views = M.all_round(camera, voxels)
    hd, hpp = scene.getHashData(), scene.getHashParams()
    W, H = cp.m_imageWidth, cp.m_imageHeight
    keep = ref.rp
    try:
        for gradients in (False, True):
            rpg = M.all_round(camera, voxels, march=march, gradients=gradients)[2]
            ref.rp = rpg
            ray = E.CUDARayCastSDF(rpg)
            full = E.CUDARayCastSDF(rpg)
            full.setIntervalSplatting(False)
            hits, longest = 0, 0
            for v in M.VIEWS:
                what = f"{camera} {voxels} {march} gradients={gradients} view {v}"
                want = ref.render(views[v])
                hits += int((want["depth"] != -np.inf).sum())
                ray.render(hd, hpp, cp, views[v])
                assert_maps_equal(ray.download(), want, f"{what}: interval splat")
                full.render(hd, hpp, cp, views[v])
                assert_maps_equal(full.download(), want, f"{what}: full-range march")
                rpv = ray.getRayCastParams()  # (with the view's matrices)
                maps = ("depth", "depth4", "colors") + (("normals",) if gradients else ())  # (computeNormals is not part of the launchers)
                got = render_hash(vh, lib, ray, hd, hpp, cp, rpv, W, H)
                for m in maps:
                    assert np.array_equal(bits(got[m]), bits(want[m])), f"{what}: hash-table ray caster, map {m}"
                for cap in (TI.CAP_LARGE, TI.CAP_SMALL, 4):
                    got, heads, _ = render_intervals(vh, lib, ray, hd, hpp, cp, rpv, W, H, cap)
                    longest = max(longest, int(heads[:, 2].max()))
                    for m in maps:
                        assert np.array_equal(bits(got[m]), bits(want[m])), f"{what}: tile lists of {cap} entries, map {m}"
            print(f"{camera} {voxels} {march} gradients={gradients}: {hits} hits, longest tile list {longest}")
            assert hits >= expected_hits(camera, voxels, march), hits
            assert longest > 4, "no tile list overflowed four entries"
            if voxels == "P1":
                assert longest > TI.CAP_SMALL, f"the longest tile list has {longest} entries: the large tables were not needed"
            ray.close()
            full.close()
    finally:
        ref.rp = keep


# ------------------------------------------------------------------------------------------------ (b) split tiles

# set -> pixels that end on the near wall, on the far wall, nowhere, 8x8 tiles with pixels of both walls: the oracle's, times 2/3
WALLS = {"dist_gate": (26336, 9701, 7653, 93), "fine": (24960, 9693, 9037, 450)}  # oracle: 39 504 / 14 552 / 11 480 / 140, 37 440 / 14 540 / 13 556 / 676 of 1024


@pytest.mark.parametrize("gradients", [False, True])
@pytest.mark.parametrize("march", list(WALLS))
def test_split_tiles_with_a_rejected_near_crossing(vh, E, oracle_lib, march, gradients):
    """256x256, two walls behind one another: under these sets a ray's crossing of the near wall is rejected for a third
    of the pixels and the ray goes on to the far wall, where it is accepted or not.  In a split tile that is the near
    half finding nothing and taking the far half's result.  Rendered without a schedule, along a fresh schedule (64 tiles
    split, at least 8 of them with pixels of both walls), beside a stale one, along a schedule made from the cost classes
    those renders left (the dearest tiles split), and along one made from classes set here that put the tiles with both
    walls first: each the oracle's, bit for bit."""
    import test_gpu_render_wave_work as WW
    from voxelhashing_amd import lib
    O = oracle_lib
    W = H = 256
    hp, cp, _ = small_config(W, H, "P4", num_buckets=1 << 11, num_sdf_blocks=1024)
    vs, trunc = float(hp.m_virtualVoxelSize), float(hp.m_truncation)
    near_z, far_z = 4.9 * B * vs, 8.9 * B * vs
    fields = [WW.plane_field((-7, -7, 4), (14, 14, 2), vs, near_z, trunc, seed=3), WW.plane_field((-7, -7, 8), (14, 14, 2), vs, far_z, trunc, seed=4)]
    descs, blocks = np.concatenate([f[0] for f in fields]), np.concatenate([f[1] for f in fields])
    assert len(descs) == 784
    pose = WW.eye_pose(0.013, -0.021, 0.0)
    # with the default thresholds every pixel ends on the near wall
    rp0 = T.make_raycast_params(hp, cp, use_gradients=gradients)
    o = O.OracleScene(hp, cp, rp0)
    assert o.stream_in(descs, blocks) == 0
    first = WW.oracle_render(o, WW.view_of(rp0, pose), pose)["depth"]
    assert (first != -np.inf).all() and (first < 0.5 * (near_z + far_z)).all()
    o.close()
    rp = T.make_raycast_params(hp, cp, use_gradients=gradients, **CM.march_factors(march))
    g, o = WW.both_scenes(E, O, hp, cp, rp, descs, blocks)
    rpv = WW.view_of(rp, pose)
    want = WW.oracle_render(o, rpv, pose)
    d = want["depth"]
    hit = d != -np.inf
    near, far = hit & (d < 0.5 * (near_z + far_z)), hit & (d >= 0.5 * (near_z + far_z))
    both = (near.reshape(H // 8, 8, W // 8, 8).any(axis=(1, 3)) & far.reshape(H // 8, 8, W // 8, 8).any(axis=(1, 3))).reshape(-1)
    counts = (int(near.sum()), int(far.sum()), int((~hit).sum()), int(both.sum()))
    print(f"\n{march} gradients={gradients}: near wall / far wall / nothing / tiles with both: {counts}")
    assert all(c >= w for c, w in zip(counts, WALLS[march])), counts
    r = WW.Renderer(vh, E, g, cp, rpv)
    assert vh.vh_render_split_tiles(W, H) == 64
    words = vh.vh_render_schedule_bytes(W, H) // 4
    n_launched = 4 * ((r.n_tiles + 64 + 3) // 4)

    def split_tiles_of(sched, phase):
        after = sched.download(np.uint32)
        assert after[0] == phase
        slots = after[4 + 4 * ((r.n_tiles + 3) // 4):].reshape(-1, 2)[:n_launched]
        halves = slots[:, 0] >> 24
        assert (slots[:, 1] == phase).sum() == r.n_tiles + 64 and (halves != 0).sum() == 128, "64 tiles were meant to be split"
        return np.unique(slots[halves != 0, 0] & 0xffffff)

    sched = lib.DeviceBuffer(4 * words)
    sched.upload(np.zeros(words, np.uint32))
    plain, _ = r.render()
    assert_maps_equal(plain, want, f"{march}: no schedule against the oracle")
    fresh, _ = r.render(splat_sched=sched.ptr, render_sched=sched.ptr, phase=1)
    split = split_tiles_of(sched, 1)
    assert_maps_equal(fresh, want, f"{march}: schedule of this phase against the oracle")
    stale, _ = r.render(splat_sched=None, render_sched=sched.ptr, phase=2)  # the splat made no schedule for phase 2
    assert sched.download(np.uint32)[0] == 1, "the schedule was meant to be stale"
    assert_maps_equal(stale, want, f"{march}: stale schedule against the oracle")
    print(f"split tiles that hold pixels of both walls: {int(both[split].sum())} of {len(split)} along the fresh schedule (tile rows {np.unique(split // (W // 8)).tolist()})")
    assert len(split) == 64
    # The fresh schedule is dealt from cost classes that are all 0, where a tile's rank is the order in which one wave's lanes
    # are served at one LDS word (schedule_tiles, vh_frame_splat.hpp): the first two tiles of every quad of the tile rows 7,
    # 15, 23 and 31 whenever it was run.  The oracle's walls meet in 13 (dist_gate) and 41 (fine) of those 64 tiles.
    assert both[split].sum() >= 8, "fewer than 8 of the tiles the fresh run split hold pixels of both walls"
    # a schedule made from the cost classes those two renders left (sched[4 + tile], schedule_tiles in vh_frame_splat.hpp):
    # the dearest tiles are split
    costed, _ = r.render(splat_sched=sched.ptr, render_sched=sched.ptr, phase=3)
    costed_split = split_tiles_of(sched, 3)
    assert_maps_equal(costed, want, f"{march}: schedule from the previous render's cost classes against the oracle")
    # and one from classes set here (the same words), dearest the tiles that hold pixels of both walls: an extra, on top of
    # the runs above, in which nearly every split tile merges a rejected near half with a far half
    seeded = np.zeros(words, np.uint32)
    seeded[4:4 + r.n_tiles] = np.where(both, 31, 0)
    steered_sched = lib.DeviceBuffer(4 * words)
    steered_sched.upload(seeded)
    steered, _ = r.render(splat_sched=steered_sched.ptr, render_sched=steered_sched.ptr, phase=1)
    steered_split = split_tiles_of(steered_sched, 1)
    assert_maps_equal(steered, want, f"{march}: schedule that splits the tiles with both walls against the oracle")
    print(f"along the schedule from the previous render's costs: {int(both[costed_split].sum())} of {len(costed_split)}; along the steered one: "
          f"{int(both[steered_split].sum())} of {len(steered_split)}")
    assert len(costed_split) == 64 and len(steered_split) == 64
    # the dearest rays pass both walls, so the dearest tiles hold such pixels: the device split 23 (dist_gate) and 61 (fine)
    # tiles in which the oracle's walls meet, and 60 and 64 of the steered ones (the sort deals from eight shares in turns)
    assert both[costed_split].sum() >= 8 and both[steered_split].sum() >= 8, "fewer than 8 split tiles hold pixels of both walls"
    g.close()
    o.close()


# ------------------------------------------------------------------------------------------------ (c) the frame loop

# (parameter set, march set) -> (buckets, seed of the poses, blocks after the last frame and ray hits of all frames by the
# oracle alone, times 2/3) for tum at 160x120, 4 cm: the layout of tests/test_gpu_camera_models.py's LOOP
LOOP_SETS = {(None, "dist_gate"): (1 << 14, 1, 149, 7342), (None, "fine"): (1 << 14, 1, 149, 7605),  # oracle: 224 / 11 013, 224 / 11 408 (21 717 hits with the defaults)
             ("thick", None): (1 << 14, 1, 214, 14442)}                                              # 322 / 21 664


@pytest.mark.parametrize("pset,march", list(LOOP_SETS), ids=lambda v: str(v))
def test_native_loop_under_a_set(E, oracle_lib, pset, march):
    """vh_reconstruction_run frame by frame with its riders -- alloc in the ray caster's launch, compactify and the next
    frame's splat in computeNormals' -- against the oracle after every frame: test_native_loop_under_a_camera's body"""
    from test_gpu_camera_models import native_loop_under_a_camera
    key = ("tum", (160, 120), "P4", pset)
    native_loop_under_a_camera(E, oracle_lib, key, {key: LOOP_SETS[(pset, march)]}, march)


# ------------------------------------------------------------------------------------------------ (d) integrate's shapes

# voxels -> (pool, blocks in view in the last frame, voxels integrated over the default band's: the oracle's, times 2/3)
THICK_SEQUENCES = {"P4": (4096, 200, 18658), "P2": (2048, 736, 79811)}  # oracle: 300 in view, 77 382 - 49 394 voxels; 1 104 in view, 347 554 - 227 837


@pytest.mark.parametrize("reference_sequence", [False, True])
@pytest.mark.parametrize("voxels", list(THICK_SEQUENCES))
def test_launch_sequences_under_the_thick_band(E, oracle_lib, voxels, reference_sequence):
    """test_launch_sequences_under_a_camera's body with a band of 9.6 voxels + 4 per metre, wider than a block: the fused
    pass in a launch of its own -- a workgroup per block at 4 cm, a wave per block at 2 cm -- and the reference's launch
    sequence, both against the oracle after every frame"""
    from test_camera_models import integrated_voxels
    from test_gpu_parity import general_poses, run_pair
    O = oracle_lib
    pool, want_in_view, want_extra = THICK_SEQUENCES[voxels]
    hp, cp, rp = CM.config("tum", (160, 120), voxels, "thick", buckets=1 << 14, blocks=pool)
    poses = CM.place(general_poses(4, 1), cp)
    nearest = min(float(d[d != -np.inf].min()) for d in (O.synth_frame(CM.SPHERES, 0, p, cp)[0] for p in poses))
    assert hp.m_truncation + hp.m_truncScale * nearest > B * hp.m_virtualVoxelSize, "the band was meant to be wider than a block"
    opt = T.make_scene_options(offline=True, gc=True, starve=2, reference_launch_sequence=reference_sequence)
    g_scene, g_ray, o_scene = run_pair(E, O, hp, cp, rp, opt, poses, CM.SPHERES)
    in_view = o_scene.hp.m_numOccupiedBlocks  # the oracle's count for the last frame
    plain = CM.config("tum", (160, 120), voxels, buckets=1 << 14, blocks=pool)
    o_plain = O.OracleScene(*plain, opt)
    for p in poses:
        o_plain.integrate(p, *O.synth_frame(CM.SPHERES, 0, p, cp))
    extra = integrated_voxels(o_scene) - integrated_voxels(o_plain)
    print(f"thick {voxels}: {in_view} blocks in view of a pool of {pool}, {extra} voxels more than with the default band")
    assert in_view >= want_in_view and extra >= want_extra, (in_view, extra)
    if voxels == "P4":
        assert in_view <= pool // 4, in_view       # a workgroup per block
    else:
        assert in_view > pool // 4 + 64, in_view   # a wave per block
    st = g_scene.getState()
    assert st[T.STATE_HEAP_UNDERFLOW] == 0 and st[T.STATE_INSERT_FAILED] == 0
    g_ray.close()
    g_scene.close()
    o_plain.close()
