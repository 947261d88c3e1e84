"""Scene cut without a GPU (DESIGN.md section 4 "Scene cut"): vh_cut_region_transform against a float64 statement of its
expressions, and the properties of the numpy restatement (tests/scene_cut.py) the GPU is held to."""
import ctypes as C

import numpy as np
import pytest

import scene_cut as SC
import scene_merge as SM
from voxelhashing_amd import vhtypes as T

V = T.SDF_BLOCK_VOXELS
VS = 0.04


@pytest.fixture(scope="module")
def E():
    from voxelhashing_amd import engine
    return engine


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the region matrix

GENERAL = SC.rotation([(0, 0.3), (2, -1.1), (1, 0.7)])
CASES = {
    "identity": (SC.frame(), (0.5, 0.5, 0.5)),
    "quarter turn": (SC.frame(SC.rotation([(2, np.pi / 2)]), (0.1, -0.2, 1.5)), (0.3, 0.3, 0.3)),
    "general rotation, unequal extents": (SC.frame(GENERAL, (0.37, -1.21, 2.05)), (0.11, 0.72, 1.9)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_region_matrix_equals_the_float64_statement(E, name):
    frame, half = CASES[name]
    for vs in (VS, 0.02, 0.013):
        got = E.cut_region_transform(frame, half, vs)
        want = SC.region_matrix(frame, half, vs)
        assert got.dtype == np.float32 and got.shape == (3, 4)
        assert np.array_equal(bits(got), bits(want)), (name, vs, got, want)
    if name == "identity":  # an axis-aligned box: a voxel at h / vs voxels from the centre has |u| = 1
        m = E.cut_region_transform(frame, half, 0.02)
        assert np.array_equal(m[:, :3], np.eye(3, dtype=np.float32) * np.float32(0.02 / 0.5)) and not m[:, 3].any()


def test_region_matrix_refusals(E):
    ok_frame, ok_half = CASES["general rotation, unequal extents"]

    def refused(frame, half=ok_half, vs=VS):
        with pytest.raises(Exception) as err:
            E.cut_region_transform(frame, half, vs)
        assert getattr(err.value, "code", None) == 4, err.value  # VH_ERR_BAD_ARGUMENT

    E.cut_region_transform(ok_frame, ok_half, VS)
    bottom = ok_frame.copy()
    bottom[3] = (0, 0, 0.001, 1)
    refused(bottom)
    bottom[3] = (0, 0, 0, 2)
    refused(bottom)
    scaled = ok_frame.copy()
    scaled[:3, :3] *= 1.001
    refused(scaled)
    sheared = ok_frame.copy()
    sheared[0, 1] += 0.01
    refused(sheared)
    mirrored = ok_frame.copy()
    mirrored[:3, 0] *= -1.0
    refused(mirrored)
    for bad in (np.nan, np.inf):
        f = ok_frame.copy()
        f[1, 3] = bad
        refused(f)
        f = ok_frame.copy()
        f[1, 1] = bad
        refused(f)
        refused(ok_frame, (0.1, bad, 0.1))
        refused(ok_frame, vs=bad)
    refused(ok_frame, (0.1, 0.0, 0.1))
    refused(ok_frame, (0.1, 0.1, -0.2))
    refused(ok_frame, vs=0.0)
    refused(ok_frame, vs=-0.04)
    # within the tolerance of 1e-4 a nearly rigid frame is taken
    nearly = ok_frame.copy()
    nearly[:3, :3] *= 1.00001
    E.cut_region_transform(nearly, ok_half, VS)
    L = E.load()
    out = np.zeros(12, np.float32)
    assert L.vh_cut_region_transform(None, None, C.c_float(VS), out.ctypes.data) == 4


# ------------------------------------------------------------------------------------------------ the restatement

def seeded_scene(seed, n=60, most_weight=40):
    """n blocks around the origin, 40 % of the voxels unobserved, some of those with sdf bits left in them"""
    rng = np.random.default_rng(seed)
    cand = np.unique(rng.integers(-3, 3, (4 * n, 3)).astype(np.int32), axis=0)
    pos = cand[rng.permutation(len(cand))[:n]]
    vox = np.zeros((len(pos), V), T.VOXEL_DTYPE)
    vox["sdf"] = rng.uniform(-0.1, 0.1, vox.shape).astype(np.float32)
    vox["color"] = rng.integers(0, 256, vox.shape + (3,), dtype=np.uint8)
    vox["weight"] = rng.integers(1, most_weight + 1, vox.shape).astype(np.uint8)
    hole = rng.random(vox.shape) < 0.4
    vox["weight"][hole] = 0
    vox["color"][hole] = 0
    vox["sdf"][hole & (rng.random(vox.shape) < 0.5)] = 0
    return SM.sort_scene(pos, vox)


REGIONS = {
    "box": (SC.frame(None, (0.1, -0.05, 0.2)), (0.5, 0.33, 0.41), T.CUT_BOX),
    "rotated box": (SC.frame(SC.rotation([(0, 0.5), (1, -0.8)]), (-0.1, 0.1, 0.0)), (0.7, 0.45, 0.6), T.CUT_BOX),
    "ellipsoid": (SC.frame(SC.rotation([(2, 0.4)]), (0.0, 0.0, 0.1)), (0.9, 0.6, 0.75), T.CUT_ELLIPSOID),
}


def by_position(scene):
    return {tuple(int(v) for v in p): v for p, v in zip(*scene)}


@pytest.mark.parametrize("outside", [0, T.CUT_SELECT_OUTSIDE])
@pytest.mark.parametrize("name", sorted(REGIONS))
def test_lifted_and_remainder_partition_the_observed_voxels(name, outside):
    frame, half, shape = REGIONS[name]
    m = SC.region_matrix(frame, half, VS)
    scene = seeded_scene(5)
    out = SC.cut(scene, m, shape, outside | T.CUT_LIFT)
    c = out["counts"]
    assert 0 < c["freed"] < c["touched"] <= c["blocks_in"] and 0 < c["lifted"] and (outside or c["touched"] < c["blocks_in"]), c
    before, rest, lifted = by_position(scene), by_position((out["positions"], out["voxels"])), by_position(out["lifted"])
    seen = 0
    for p, v in before.items():
        obs = v["weight"] > 0
        r = rest.get(p, np.zeros(V, T.VOXEL_DTYPE))
        l = lifted.get(p, np.zeros(V, T.VOXEL_DTYPE))
        in_r, in_l = r["weight"] > 0, l["weight"] > 0
        assert not (in_r & in_l).any() and np.array_equal(in_r | in_l, obs), f"block {p}: the observed voxels are not partitioned"
        assert r[in_r].tobytes() == v[in_r].tobytes() and l[in_l].tobytes() == v[in_l].tobytes()
        seen += int(in_l.sum())
    assert seen == c["voxels_lifted"] == c["voxels_erased"]
    assert set(rest) | SC_positions(out["freed"]) == set(before) and not (set(rest) & SC_positions(out["freed"]))
    assert set(lifted) <= set(before)


def SC_positions(positions):
    return {tuple(int(v) for v in p) for p in np.asarray(positions).reshape(-1, 3)}


@pytest.mark.parametrize("name", sorted(REGIONS))
def test_merging_the_lifted_list_back_restores_every_observed_voxel(name):
    frame, half, shape = REGIONS[name]
    m = SC.region_matrix(frame, half, VS)
    scene = seeded_scene(6, most_weight=40)
    hp = T.make_hash_params(1 << 10, 1 << 10, 0.04)
    hp.m_integrationWeightMax = 40  # a cap the weights do not exceed
    out = SC.cut(scene, m, shape, T.CUT_LIFT)
    back = SM.merge((out["positions"], out["voxels"]), out["lifted"], hp)
    assert back["counts"]["combined"] == 0 and back["counts"]["copied"] == out["counts"]["voxels_lifted"]
    assert back["counts"]["allocated"] <= out["counts"]["freed"]
    got, want = by_position((back["positions"], back["voxels"])), by_position(scene)
    for p, v in want.items():
        obs = v["weight"] > 0
        if obs.any():
            assert p in got, f"block {p} with observed voxels did not come back"
            assert got[p][obs].tobytes() == v[obs].tobytes(), f"block {p}: an observed voxel differs"
            assert not (got[p]["weight"][~obs] > 0).any()


@pytest.mark.parametrize("name", sorted(REGIONS))
def test_select_outside_is_the_complement(name):
    frame, half, shape = REGIONS[name]
    m = SC.region_matrix(frame, half, VS)
    pos, vox = seeded_scene(7)
    a, b = SC.selected(m, shape, 0, pos), SC.selected(m, shape, T.CUT_SELECT_OUTSIDE, pos)
    assert a.any() and b.any() and np.array_equal(a, ~b)
    # a NaN is not inside: selected by the complement
    nan = m.copy()
    nan[1, 3] = np.nan
    assert not SC.selected(nan, shape, 0, pos).any() and SC.selected(nan, shape, T.CUT_SELECT_OUTSIDE, pos).all()
    # crop then holds what erase takes: the observed voxels of the two results partition the scene's
    erased, cropped = SC.cut((pos, vox), m, shape, 0), SC.cut((pos, vox), m, shape, T.CUT_SELECT_OUTSIDE)
    total = int((vox["weight"] > 0).sum())
    assert int((erased["voxels"]["weight"] > 0).sum()) + int((cropped["voxels"]["weight"] > 0).sum()) == total
    assert erased["counts"]["voxels_erased"] + cropped["counts"]["voxels_erased"] == total


@pytest.mark.parametrize("flags", [0, T.CUT_LIFT, T.CUT_LIFT | T.CUT_KEEP, T.CUT_SELECT_OUTSIDE])
def test_an_untouched_block_is_the_same_byte_for_byte(flags):
    frame, half, shape = REGIONS["rotated box"]
    m = SC.region_matrix(frame, half, VS)
    scene = seeded_scene(8)
    out = SC.cut(scene, m, shape, flags)
    touched = SC.selected(m, shape, flags, scene[0]).any(axis=1)
    assert touched.any() and not touched.all()
    before, after = by_position(scene), by_position((out["positions"], out["voxels"]))
    for p, hit in zip(scene[0], touched):
        p = tuple(int(v) for v in p)
        if not hit or flags & T.CUT_KEEP:
            assert after[p].tobytes() == before[p].tobytes(), f"block {p} changed"
    if flags & T.CUT_KEEP:
        assert out["counts"]["freed"] == 0 and out["counts"]["voxels_erased"] == 0 and len(out["freed"]) == 0
    # count only and a staging pool one block short change nothing
    for same in (SC.cut(scene, m, shape, flags | T.CUT_COUNT_ONLY),
                 SC.cut(scene, m, shape, T.CUT_LIFT, staging_blocks=SC.cut(scene, m, shape, T.CUT_LIFT)["counts"]["lifted"] - 1)):
        assert SM.same_scene((same["positions"], same["voxels"]), scene) and len(same["lifted"][0]) == 0


# ------------------------------------------------------------------------------------------------ tools/replay.py's boxes

def test_replay_box_arguments():
    """--erase-box / --crop-box: centre, half extents and an optional rotation vector make the region's frame"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import replay
    r = replay.box_region([0.1, -0.2, 1.5, 0.3, 0.4, 0.5])
    assert np.array_equal(np.array(r.worldFromRegion[:]).reshape(4, 4), SC.frame(None, (0.1, -0.2, 1.5)))
    assert [np.float32(v) for v in r.halfExtents] == [np.float32(0.3), np.float32(0.4), np.float32(0.5)] and r.shape == T.CUT_BOX
    r = replay.box_region([0.0, 0.0, 1.0, 0.3, 0.4, 0.5, 0.0, 0.0, np.pi / 2])  # a quarter turn about z
    assert np.allclose(np.array(r.worldFromRegion[:]).reshape(4, 4), SC.frame(SC.rotation([(2, np.pi / 2)]), (0, 0, 1)), atol=1e-15)
    w = np.array([0.3, -0.5, 0.2])
    R = np.array(replay.box_region([0, 0, 0, 1, 1, 1, *w]).worldFromRegion[:]).reshape(4, 4)[:3, :3]
    assert np.allclose(R.T @ R, np.eye(3), atol=1e-14) and np.isclose(np.linalg.det(R), 1.0) and np.allclose(R @ w, w)
