"""The oracle under the ray caster's other parameters (tests/camera_models.py's MARCH_SETS and BAND_SETS): thresholds at
which the two comparisons that accept a zero crossing -- fabsf(lastSdf - dist) < m_thresSampleDist and fabsf(dist) <
m_thresDist -- are false for most crossings, ray increments of a quarter of the truncation and of two and a half
truncations, and a truncation band wider than a block.  Under the builders' defaults both thresholds lie at forty
truncations and a stored distance never passes three and a half: neither comparison can be false, and what follows a
rejected crossing (the march resumes with the rejected sample as its last one) never runs.

The oracle against the reference's own code compiled for the CPU (oracle/_ref/libvh_ref.so), bit for bit, through the
comparisons of tests/test_reference_pinning.py and tests/test_camera_models.py; then, by the oracle alone, that the sets
do what they are named for on the views tests/test_gpu_march_parameters.py renders on the device.  The lower bounds are
literal numbers read off the oracle's own run (two thirds of what it gave, rounded down), never off the device.

The scene is S1 seen from all round -- integrated offline from eight poses of the orbit, rendered from twenty-four -- so
that there is a surface behind the first one: where a crossing is rejected the ray goes on through the sphere and may
meet, and accept, the far side's band.  Three neighbouring poses leave nothing behind the first surface, and no hit
ever moves."""
import numpy as np
import pytest

import camera_models as CM
import test_reference_pinning as PIN
from oracle import oracle as O
from oracle import reference as R
from test_camera_models import frames_for, integrated_voxels, kernels_under, oracle_run
from voxelhashing_amd import synth, vhtypes as T

pytestmark = pytest.mark.skipif(not R.available(), reason="oracle/_ref/libvh_ref.so is not built (build() makes it "
                                "where the reference tree is present)")

GATED = [m for m in CM.MARCH_SETS if not m.startswith("coarse")] + ["coarse_dist_gate"]
# the views of the orbit of 24 the device tests render (a quarter turn apart would see the small sphere alike: these do not)
VIEWS = (7, 9, 18, 23)


@pytest.fixture(scope="module")
def libs():
    O.build()
    return O.lib(), R.lib()


# ------------------------------------------------------------------------------------------------ the all-round scene

# voxels -> image size, block pool, metres the views stand further back.  1 cm from 3.4 m, as test_ray_cast_paths of
# tests/test_gpu_camera_models.py has it: there the tile lists pass 64 entries and k_render_large's pipelined march runs
SHAPES = {"P4": ((96, 72), 1 << 13, 0.0), "P2": ((160, 120), 1 << 13, 0.0), "P1": ((64, 48), 1 << 14, 0.9)}


def all_round(camera, voxels, march=None, gradients=False):
    """-> hp, cp, rp, the 8 poses S1 is integrated from, the 24 views it is rendered from"""
    size, blocks, back = SHAPES[voxels]
    hp, cp, rp = CM.config(camera, size, voxels, buckets=1 << 14, blocks=blocks, gradients=gradients, march=march)
    poses = CM.place([synth.orbit_pose(k, n_frames=8) for k in range(8)], cp)
    views = CM.place([synth.orbit_pose(v, n_frames=24) for v in range(24)], cp, back)
    return hp, cp, rp, poses, views


def all_round_scene(O, camera, voxels):
    """the oracle's scene of all_round (offline, no GC)"""
    hp, cp, rp, poses, _ = all_round(camera, voxels)
    sc = O.OracleScene(hp, cp, rp, T.make_scene_options(offline=True, gc=False))
    for p in poses:
        sc.integrate(p, *O.synth_frame(CM.SPHERES, 0, p, cp))
    return sc


def gate_effects(sc, march, views):
    """what a march set's thresholds do over `views`, by the oracle alone: against the same increment with the default
    thresholds -> (hits at the default thresholds, pixels whose hit is lost, pixels whose hit moved deeper -- a crossing
    was rejected and a later one accepted --, hits that remain).  No hit is gained and none moves nearer: asserted."""
    inc = CM.MARCH_SETS[march][0]
    keep = sc.rp
    total = np.zeros(4, np.int64)
    try:
        for v in views:
            sc.rp = T.make_raycast_params(sc.hp, sc.cp, ray_increment_factor=inc)
            base = sc.render(v)["depth"]
            sc.rp = T.make_raycast_params(sc.hp, sc.cp, **CM.march_factors(march))
            d = sc.render(v)["depth"]
            hb, hd = base != -np.inf, d != -np.inf
            assert not (hd & ~hb).any() and not (hb & hd & (d < base)).any(), f"{march}: a tighter threshold gave a hit or brought one nearer"
            total += (int(hb.sum()), int((hb & ~hd).sum()), int((hb & hd & (d > base)).sum()), int(hd.sum()))
    finally:
        sc.rp = keep
    return tuple(int(t) for t in total)


@pytest.fixture(scope="module")
def scenes():
    class Scenes(dict):
        def __missing__(self, key):
            self[key] = all_round_scene(O, *key)
            return self[key]
    return Scenes()


# ------------------------------------------------------------------------------------------------ against the reference

# default-camera hits of VIEWS under the set (without gradients) at 4 cm, times 2/3
RENDER_HITS = {"sample_gate": 2426, "dist_gate": 3828, "both_gates": 1256, "fine": 3355, "fine_sample_gate": 1200,  # oracle: 3 640 / 5 743 / 1 885 / 5 033 / 1 801
               "coarse": 5980, "coarse_dist_gate": 1863}                                                                # 8 971 / 2 795


@pytest.mark.parametrize("gradients", [False, True])
@pytest.mark.parametrize("march", list(CM.MARCH_SETS))
def test_oracle_render_equals_the_reference_under_a_march_set(libs, scenes, march, gradients):
    """OracleScene.render against the reference's renderKernel on one state, under every march set: the four maps"""
    key = (None, "P4")
    sc = scenes[key]
    _, _, rp, _, views = all_round(*key, march=march, gradients=gradients)
    a, b = O.OracleScene(sc.hp, sc.cp, ray_params=rp), O.OracleScene(sc.hp, sc.cp, ray_params=rp)
    PIN._copy_state(sc, a)
    PIN._copy_state(sc, b)
    hits = 0
    for v in VIEWS:
        want = a.render(views[v])
        got = R.RefScene(b).render(a.rp)
        if not gradients:  # (the reference leaves computeNormals to a separate call, as PIN.check_kernels_on_one_state makes it)
            got["normals"] = R.compute_normals(got["depth4"])
        PIN._maps_equal(want, got, f"{march} gradients={gradients} view {v}")
        hits += int((want["depth"] != -np.inf).sum())
    print(f"{march} gradients={gradients}: {hits} hits")
    assert hits >= RENDER_HITS[march], hits


# per voxel size under tum and thick: (live blocks after the last frame, integrated voxels, most ray hits of a frame) of
# the oracle's run of kernels_under's frames, times 2/3; then the voxels the online loop integrates over the default band's
THICK_COUNTS = {"P4": (216, 51706, 2052, 18672), "P2": (751, 231909, 2191, 80408)}  # oracle: 324 / 77 559 / 3 078, 77 559 - 49 550; 1 127 / 347 864 / 3 287, 347 864 - 227 252


@pytest.mark.parametrize("voxels", ["P4", "P2"])
def test_kernels_under_the_thick_band(libs, voxels):
    """tests/test_camera_models.py's kernels_under -- alloc, integrate, starve, GC, render and normals one by one, the
    online frame loop, the ray cast with gradients -- with a band of 9.6 voxels + 4 per metre"""
    hp, cp, rp = CM.config("tum", (96, 72), voxels, pset="thick", buckets=1 << 14, blocks=1 << 12)
    poses = frames_for(cp, 4, 1)
    assert hp.m_truncation > T.SDF_BLOCK_SIZE * hp.m_virtualVoxelSize, "the band was meant to be wider than a block"
    blocks, voxels_in, hits, _ = kernels_under(hp, cp, poses, f"thick {voxels}")
    plain = CM.config("tum", (96, 72), voxels, buckets=1 << 14, blocks=1 << 12)
    extra = integrated_voxels(oracle_run(hp, cp, rp, poses)[0]) - integrated_voxels(oracle_run(*plain, poses)[0])
    print(f"thick {voxels}: {blocks} blocks, {voxels_in} voxels, {hits} hits, {extra} voxels more than with the default band")
    want = THICK_COUNTS[voxels]
    assert blocks >= want[0] and voxels_in >= want[1] and hits >= want[2] and extra >= want[3], (blocks, voxels_in, hits, extra)


# ------------------------------------------------------------------------------------------------ the cuts are crossed

# (camera, voxels) -> set -> (lost, moved, remaining) over the 24 views by the oracle alone, times 2/3
CUTS_ALL_ROUND = {
    (None, "P4"): {"sample_gate": (46746, 202, 13052), "dist_gate": (37036, 118, 22762), "both_gates": (53192, 138, 6606),  # oracle: 70 119 / 304 / 19 578, 55 554 / 177 / 34 143, 79 788 / 208 / 9 909
                   "fine": (41322, 672, 20148), "fine_sample_gate": (55012, 896, 6458), "coarse_dist_gate": (25413, 20, 10634)},  # 61 984 / 1 009 / 30 223, 82 519 / 1 345 / 9 688, 38 120 / 31 / 15 952
}


@pytest.mark.parametrize("march", GATED)
@pytest.mark.parametrize("camera,voxels", list(CUTS_ALL_ROUND), ids=lambda v: str(v))
def test_thresholds_reject_crossings_and_the_march_resumes(libs, scenes, camera, voxels, march):
    """in the style of cuts_taking_effect: each set against the same increment with the default thresholds"""
    sc = scenes[(camera, voxels)]
    views = all_round(camera, voxels)[4]
    default_hits, lost, moved, remaining = gate_effects(sc, march, views)
    print(f"{camera} {voxels} {march}: {default_hits} hits at the default thresholds, {lost} lost, {moved} moved deeper, {remaining} remain")
    want = CUTS_ALL_ROUND[(camera, voxels)][march]
    assert lost >= want[0] and moved >= want[1] and remaining >= want[2], (lost, moved, remaining)
    assert lost >= 1000 and remaining >= 1000, "a set that rejects or keeps fewer than 1000 crossings is vacuous"


# (camera, voxels) -> set -> (lost, moved, remaining) over VIEWS, the four views the device renders, times 2/3.  1 cm
# only under the two sets the device renders there.
CUTS_VIEWS = {
    # oracle: 11 098 / 130 / 3 640, 8 995 / 81 / 5 743, 12 853 / 80 / 1 885, 10 263 / 235 / 5 033, 13 495 / 310 / 1 801, 6 176 / 13 / 2 795
    (None, "P4"): {"sample_gate": (7398, 86, 2426), "dist_gate": (5996, 54, 3828), "both_gates": (8568, 53, 1256),
                   "fine": (6842, 156, 3355), "fine_sample_gate": (8996, 206, 1200), "coarse_dist_gate": (4117, 8, 1863)},
    # 11 091 / 61 / 4 014, 8 839 / 31 / 6 266, 12 878 / 43 / 2 227, 9 638 / 244 / 5 932, 13 284 / 368 / 2 286, 6 002 / 7 / 4 182
    ("offcentre", "P4"): {"sample_gate": (7394, 40, 2676), "dist_gate": (5892, 20, 4177), "both_gates": (8585, 28, 1484),
                          "fine": (6425, 162, 3954), "fine_sample_gate": (8856, 245, 1524), "coarse_dist_gate": (4001, 4, 2788)},
    # 31 939 / 413 / 10 109, 24 973 / 273 / 17 075, 36 755 / 298 / 5 293, 27 229 / 432 / 15 025, 36 619 / 511 / 5 635, 18 109 / 95 / 11 424
    (None, "P2"): {"sample_gate": (21292, 275, 6739), "dist_gate": (16648, 182, 11383), "both_gates": (24503, 198, 3528),
                   "fine": (18152, 288, 10016), "fine_sample_gate": (24412, 340, 3756), "coarse_dist_gate": (12072, 63, 7616)},
    # 32 386 / 467 / 12 589, 26 855 / 356 / 18 120, 38 442 / 391 / 6 533, 28 239 / 578 / 17 094, 38 615 / 698 / 6 718, 17 798 / 112 / 14 472
    ("offcentre", "P2"): {"sample_gate": (21590, 311, 8392), "dist_gate": (17903, 237, 12080), "both_gates": (25628, 260, 4355),
                          "fine": (18826, 385, 11396), "fine_sample_gate": (25743, 465, 4478), "coarse_dist_gate": (11865, 74, 9648)},
    (None, "P1"): {"dist_gate": (1204, 19, 974), "fine": (1282, 30, 903)},         # 1 806 / 29 / 1 461, 1 923 / 46 / 1 355
    ("offcentre", "P1"): {"dist_gate": (1236, 18, 1066), "fine": (1389, 42, 943)},  # 1 854 / 27 / 1 600, 2 084 / 64 / 1 415
}


@pytest.mark.parametrize("camera,voxels,march", [(c, v, m) for (c, v), sets in CUTS_VIEWS.items() for m in sets], ids=lambda v: str(v))
def test_the_views_of_the_device_tests_cross_the_cuts(libs, scenes, camera, voxels, march):
    """the same over the four views tests/test_gpu_march_parameters.py renders, so that the device is held to rejected
    crossings and resumed marches and not to the sets' names"""
    sc = scenes[(camera, voxels)]
    views = all_round(camera, voxels)[4]
    default_hits, lost, moved, remaining = gate_effects(sc, march, [views[v] for v in VIEWS])
    print(f"{camera} {voxels} {march}: {default_hits} hits at the default thresholds, {lost} lost, {moved} moved deeper, {remaining} remain")
    want = CUTS_VIEWS[(camera, voxels)][march]
    assert lost >= want[0] and moved >= want[1] and remaining >= want[2], (lost, moved, remaining)
    assert lost >= 1000 and remaining >= 1000, "a set that rejects or keeps fewer than 1000 crossings is vacuous"


def step_effects(sc, views):
    """the coarse step against the 0.8 step, default thresholds -> (hits at 0.8, hits at 2.5, pixels hit by either, pixels of those whose depth differs)"""
    keep = sc.rp
    out = np.zeros(4, np.int64)
    try:
        for v in views:
            sc.rp = T.make_raycast_params(sc.hp, sc.cp)
            base = sc.render(v)["depth"]
            sc.rp = T.make_raycast_params(sc.hp, sc.cp, **CM.march_factors("coarse"))
            d = sc.render(v)["depth"]
            either = (base != -np.inf) | (d != -np.inf)
            out += (int((base != -np.inf).sum()), int((d != -np.inf).sum()), int(either.sum()), int((PIN.bits(base) != PIN.bits(d)).sum()))
    finally:
        sc.rp = keep
    return tuple(int(t) for t in out)


@pytest.mark.parametrize("camera,voxels", list(CUTS_ALL_ROUND), ids=lambda v: str(v))
def test_the_coarse_step_passes_over_the_band(libs, scenes, camera, voxels):
    """an increment of 2.5 truncations: a ray can step from in front of the band to behind it and see no sign change.
    The oracle, 24 views: 54 072 hits against 89 697 at the 0.8 step; of the 90 365 pixels either march hits, 90 327 differ."""
    sc = scenes[(camera, voxels)]
    fine_hits, coarse_hits, either, differ = step_effects(sc, all_round(camera, voxels)[4])
    print(f"{camera} {voxels}: {coarse_hits} hits at the coarse step, {fine_hits} at 0.8; {differ} of {either} pixels differ")
    assert 1000 <= coarse_hits <= 0.8 * fine_hits, (coarse_hits, fine_hits)
    assert coarse_hits >= 36048  # two thirds of 54 072
    assert differ > 0.8 * either, (differ, either)


# ------------------------------------------------------------------------------------------------ the ray-query restatement

def ray_query_model(march):
    """tests/test_query_reference.py's model -- S1 at 64x48 (P4), three offline frames, rendered with gradients from a
    fourth pose -- with the march set in its RayCastParams.  The view stands 0.7 m nearer, where the sphere fills the image:
    half of the crossings rejected still leaves 1000 hits (the oracle: 2 929 hits at the default thresholds, 1 547 under
    dist_gate, 1 101 under fine_sample_gate).  Rays end at 2.6 m, behind the sphere's rim."""
    hp = T.make_hash_params(1 << 14, 1 << 13, **synth.PARAM_SETS["P4"])
    cp = CM.camera(None, 64, 48, depth_max=2.6)
    rp = T.make_raycast_params(hp, cp, use_gradients=True, **CM.march_factors(march))
    o = O.OracleScene(hp, cp, rp, T.make_scene_options(offline=True))
    poses = [synth.orbit_pose(k, n_frames=100) for k in (0, 1, 2)]
    for pose in poses:
        o.integrate(pose, *O.synth_frame(synth.S1_SPHERES, 0, pose, cp))
    view = CM.place([synth.orbit_pose(5, n_frames=100)], cp, -0.7, offset=0.0)[0]
    maps = o.render(view)
    return dict(O=O, o=o, cp=cp, rp=o.rp, maps=maps, view=view, poses=poses)


# set -> (hits at least, hits at most) of the model's view by the oracle alone: two thirds of what it gave, and the middle
# between that and the 2 929 hits of the default thresholds and step
QUERY_HITS = {"dist_gate": (1031, 2238), "fine_sample_gate": (734, 2015)}  # oracle: 1 547, 1 101


@pytest.mark.parametrize("march", list(QUERY_HITS))
def test_ray_query_restatement_under_a_march_set(libs, march):
    """tests/ray_query.py's march reproduces the oracle's render where most crossings are rejected (at least 1000 hits
    and 1000 misses, and far fewer hits than under the default thresholds): the GPU query tests lean on it"""
    import test_query_reference as TQ
    m = ray_query_model(march)
    TQ.test_camera_rays_reproduce_the_oracle_render(m)
    hits = int((m["maps"]["depth"] != -np.inf).sum())
    print(f"{march}: {hits} hits")
    assert QUERY_HITS[march][0] <= hits <= QUERY_HITS[march][1], hits


def test_ray_query_model_at_the_default_thresholds(libs):
    """the same view with the builders' defaults: the sphere fills the image"""
    hits = int((ray_query_model(None)["maps"]["depth"] != -np.inf).sum())
    assert hits >= 1952, hits  # oracle: 2 929 of 3 072 pixels
