"""The numpy restatement of the scene merge (tests/scene_merge.py) against the definition's own consequences: merging
into nothing gives the source, merging nothing changes nothing, the block set is the union, the merge commutes for two
scenes built under one weight cap, and a heap too short for the new blocks leaves everything as it was.  No GPU."""
import numpy as np
import pytest

import scene_merge as SM
from helpers import small_config
from voxelhashing_amd import vhtypes as T

V = T.SDF_BLOCK_VOXELS


def params(cap=255, colour_mode=0):
    hp, _, _ = small_config(64, 48, "P4")
    hp.m_integrationWeightMax = cap
    hp.m_colorIntegration = colour_mode
    return hp


def random_scene(seed, n, most_weight=255, span=4, unobserved=0.4):
    """n blocks at distinct positions in [-span, span)^3; a share of the voxels unobserved and all zero, as a scene's own
    unobserved voxels are; the rest with a seeded sdf, colour and a weight in 1 ... most_weight"""
    rng = np.random.default_rng(seed)
    cells = rng.permutation((2 * span) ** 3)[:n]
    pos = np.stack([cells % (2 * span), (cells // (2 * span)) % (2 * span), cells // (2 * span) ** 2], axis=-1).astype(np.int32) - span
    vox = np.zeros((n, V), T.VOXEL_DTYPE)
    vox["sdf"] = rng.uniform(-0.2, 0.2, (n, V)).astype(np.float32)
    vox["color"] = rng.integers(0, 256, (n, V, 3), dtype=np.uint8)
    vox["weight"] = rng.integers(1, most_weight + 1, (n, V)).astype(np.uint8)
    vox[rng.random((n, V)) < unobserved] = np.zeros((), T.VOXEL_DTYPE)
    return SM.sort_scene(pos, vox)


def test_merge_into_empty_is_the_source_with_weights_capped():
    src = random_scene(1, 12)
    got = SM.merge(SM.empty_scene(), src, params(cap=20))
    want = src[1].copy()
    want["weight"] = np.minimum(want["weight"], 20)
    assert np.array_equal(got["positions"], src[0]) and got["voxels"].tobytes() == want.tobytes()
    seen = int((src[1]["weight"] > 0).sum())
    assert got["counts"] == dict(source_blocks=12, present=0, allocated=12, combined=0, copied=seen, status=0)
    # under a cap no weight exceeds, bit for bit
    full = SM.merge(SM.empty_scene(), src, params())
    assert SM.same_scene((full["positions"], full["voxels"]), src)


def test_merge_of_an_empty_source_is_the_identity():
    dst = random_scene(2, 9)
    got = SM.merge(dst, SM.empty_scene(), params(cap=20))
    assert SM.same_scene((got["positions"], got["voxels"]), dst)
    assert got["counts"] == dict(source_blocks=0, present=0, allocated=0, combined=0, copied=0, status=0)


def test_a_block_of_unobserved_voxels_still_allocates():
    dst = random_scene(3, 5)
    pos = np.array([[40, 41, 42]], np.int32)
    got = SM.merge(dst, (pos, np.zeros((1, V), T.VOXEL_DTYPE)), params())
    assert len(got["positions"]) == 6 and got["counts"]["allocated"] == 1 and got["counts"]["copied"] == 0
    k = int(np.nonzero((got["positions"] == pos[0]).all(axis=1))[0][0])
    assert not got["voxels"][k].view(np.uint64).any()


@pytest.mark.parametrize("offset", [(0, 0, 0), (1, -2, 3)])
def test_the_block_set_is_the_union(offset):
    a, b = random_scene(4, 40), random_scene(5, 40)
    got = SM.merge(a, b, params(), offset)
    shifted = b[0] + np.array(offset, np.int32)
    both = np.unique(np.concatenate([a[0], shifted]), axis=0)
    assert np.array_equal(np.unique(got["positions"], axis=0), both) and len(got["positions"]) == len(both)
    shared = len(a[0]) + len(b[0]) - len(both)
    assert shared > 0, "the two scenes were meant to share blocks"
    assert got["counts"]["present"] == shared and got["counts"]["allocated"] == len(b[0]) - shared
    # blocks the source does not name are untouched
    named = {tuple(p) for p in shifted.tolist()}
    for p, v in zip(*a):
        if tuple(p.tolist()) not in named:
            k = int(np.nonzero((got["positions"] == p).all(axis=1))[0][0])
            assert got["voxels"][k].tobytes() == v.tobytes()


@pytest.mark.parametrize("colour_mode", [0, 1])
def test_merge_commutes_under_one_cap(colour_mode):
    """both scenes hold weights up to the cap they were built under, and unobserved voxels are zero: then D <- S and
    S <- D are the same scene bit for bit (a sum and a product of two floats commute, both colour rules are symmetric,
    and the copy rule hands over whichever of the two voxels was observed)"""
    cap = 30
    a, b = random_scene(6, 30, most_weight=cap, span=2), random_scene(7, 30, most_weight=cap, span=2)
    hp = params(cap, colour_mode)
    ab, ba = SM.merge(a, b, hp), SM.merge(b, a, hp)
    assert ab["counts"]["combined"] > 1000 and ab["counts"]["copied"] > 1000
    assert SM.same_scene((ab["positions"], ab["voxels"]), (ba["positions"], ba["voxels"]))
    assert ab["counts"]["combined"] == ba["counts"]["combined"]
    assert int(ab["voxels"]["weight"].max()) == cap, "the cap was meant to bind"


def test_the_two_colour_rules_differ_only_in_colour():
    a, b = random_scene(8, 6, most_weight=40), random_scene(12, 6, most_weight=3)
    b = (a[0], b[1])  # the same positions: every block shared
    run, wgt = SM.merge(a, b, params(255, 0)), SM.merge(a, b, params(255, 1))
    assert np.array_equal(run["voxels"]["sdf"].view(np.uint32), wgt["voxels"]["sdf"].view(np.uint32))
    assert np.array_equal(run["voxels"]["weight"], wgt["voxels"]["weight"])
    assert not np.array_equal(run["voxels"]["color"], wgt["voxels"]["color"])


def test_heap_short_changes_nothing():
    a, b = random_scene(9, 20), random_scene(10, 20)
    new = len(np.unique(np.concatenate([a[0], b[0]]), axis=0)) - len(a[0])
    assert new > 1
    short = SM.merge(a, b, params(), free_blocks=new - 1)
    assert short["counts"]["status"] == T.MERGE_HEAP_SHORT and short["counts"]["allocated"] == 0
    assert short["counts"]["combined"] == 0 and short["counts"]["copied"] == 0
    assert SM.same_scene((short["positions"], short["voxels"]), a)
    enough = SM.merge(a, b, params(), free_blocks=new)
    assert enough["counts"]["status"] == 0 and enough["counts"]["allocated"] == new


def test_repeated_source_positions_are_refused():
    a = random_scene(11, 4)
    pos = np.concatenate([a[0][:2], a[0][:1]])
    with pytest.raises(AssertionError):
        SM.merge(SM.empty_scene(), (pos, a[1][:3]), params())
