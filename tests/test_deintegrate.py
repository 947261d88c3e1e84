"""Frame de-integration without a GPU (DESIGN.md section 4 "Frame de-integration"): the numpy restatement
(tests/deintegrate.py) the device is held to.  Its observation is pinned to the oracle's integrate pass, its take-out is
shown to invert combineVoxel within the stated bounds over every pair of weights below the cap, and the rule's boundary
cases are spelled out."""
import numpy as np
import pytest

import deintegrate as DI
import scene_merge as SM
import weighted_colour as WC
from helpers import small_config
from voxelhashing_amd import synth, vhtypes as T

V = T.SDF_BLOCK_VOXELS
f32 = np.float32


def config(weighted=False, **over):
    hp, cp, rp = small_config(64, 48, "P4", num_sdf_blocks=1 << 11, **over)
    hp.m_colorIntegration = T.COLOR_WEIGHTED_AVERAGE if weighted else 0
    return hp, cp, rp


def options():
    return T.make_scene_options(offline=True, gc=False)


def voxels(sdf, colour, weight):
    n = len(np.atleast_1d(weight))
    v = np.zeros(n, T.VOXEL_DTYPE)
    v["sdf"], v["color"], v["weight"] = sdf, colour, weight
    return v


def combine_numpy(hp, a, b):
    """combineVoxel in numpy (both weights > 0, the sum below the cap): pinned to the oracle's by the test below"""
    out = np.zeros(len(a), T.VOXEL_DTYPE)
    w0, w1 = a["weight"].astype(np.float32), b["weight"].astype(np.float32)
    out["sdf"] = (a["sdf"] * w0 + b["sdf"] * w1) / (w0 + w1)
    out["weight"] = np.minimum(a["weight"].astype(np.int64) + b["weight"].astype(np.int64), int(hp.m_integrationWeightMax)).astype(np.uint8)
    if hp.m_colorIntegration != 0:
        out["color"] = WC.rule_weighted(a["color"], a["weight"][:, None], b["color"], b["weight"][:, None])
    else:
        out["color"] = ((a["color"].astype(np.int64) + b["color"].astype(np.int64) + 1) >> 1).astype(np.uint8)
    return out


# ------------------------------------------------------------------------------------------------ the observation

@pytest.mark.parametrize("weighted", [False, True], ids=["running average", "weighted"])
def test_observe_is_what_the_oracle_integrates(oracle_lib, weighted):
    """S1 at 64x48: frame A through the oracle, then frame B launcher by launcher -- the voxels after B's integrate pass
    are combineVoxel(the voxels before it, observe(B)) where there is an observation and unchanged elsewhere, and the
    blocks the pass visited are the restatement's frustum test"""
    O = oracle_lib
    hp, cp, rp = config(weighted)
    o = O.OracleScene(hp, cp, rp, options())
    pose_a, pose_b = synth.orbit_pose(0, 40), synth.orbit_pose(2, 40)
    o.integrate(pose_a, *O.synth_frame(synth.S1_SPHERES, 0, pose_a, cp))
    depth, colour = O.synth_frame(synth.S1_SPHERES, 0, pose_b, cp)
    o.set_transform(pose_b)
    prev = -1
    while o.heap_free_count() != prev:
        prev = o.heap_free_count()
        o.reset_mutex()
        o.alloc(depth, colour)
    o.compactify()
    before = o.state()
    visited = {tuple(int(v) for v in p) for p in o.compactified()["pos"].reshape(-1, 3)}
    o.integrate_depth_map(depth, colour)
    after = o.state()
    pos = before["positions"]
    assert np.array_equal(pos, after["positions"]) and 100 < len(pos)
    processed = DI.block_in_frustum(pose_b, hp, cp, pos)
    assert {tuple(int(v) for v in p) for p in pos[processed]} == visited and 0 < len(visited) < len(pos)
    obs = DI.observe((depth, colour), pose_b, hp, cp, pos)
    obs[~processed] = np.zeros((), T.VOXEL_DTYPE)
    seen = obs["weight"] > 0
    assert seen.any() and (seen & (before["voxels"]["weight"] > 0)).any() and (seen & (before["voxels"]["weight"] == 0)).any()
    want = before["voxels"].copy()
    want[seen] = SM.combine_voxels(hp, before["voxels"][seen], obs[seen])
    got = after["voxels"]
    assert np.array_equal(got["sdf"].view(np.uint32), want["sdf"].view(np.uint32)), "sdf"
    assert np.array_equal(got["weight"], want["weight"]), "weight"
    if not weighted:  # (the oracle fuses colours by the running average only; the weighted rule is tests/weighted_colour.py's)
        assert got.tobytes() == want.tobytes()
    # without a colour map nothing is integrated, so nothing is observed
    assert not DI.observe((depth, None), pose_b, hp, cp, pos)["weight"].any()


# ------------------------------------------------------------------------------------------------ the inverse

def weight_pairs():
    wa, wo = np.meshgrid(np.arange(1, 255), np.arange(1, 255), indexing="ij")
    keep = wa + wo <= 255
    return wa[keep].astype(np.uint8), wo[keep].astype(np.uint8)


@pytest.mark.parametrize("weighted", [False, True], ids=["running average", "weighted"])
def test_take_out_inverts_combine_within_the_bounds(oracle_lib, weighted):
    hp = config(weighted)[0]
    assert hp.m_integrationWeightMax == 255
    depth = 3.0
    trunc = f32(f32(hp.m_truncation) + f32(hp.m_truncScale) * f32(depth))
    wa, wo = weight_pairs()
    assert len(wa) == 254 * 255 // 2
    rng = np.random.default_rng(5)
    reps = 24
    wa, wo = np.repeat(wa, reps), np.repeat(wo, reps)
    n = len(wa)
    extremes = np.array([trunc, -trunc, 0.0, -0.0, 1e-38, -1e-41, np.nextafter(trunc, f32(0)), 0.5 * trunc], np.float32)
    s = rng.uniform(-trunc, trunc, n).astype(np.float32)
    ob = rng.uniform(-trunc, trunc, n).astype(np.float32)
    s[0::reps], ob[0::reps] = trunc, -trunc
    s[1::reps], ob[1::reps] = -trunc, trunc
    s[2::reps], ob[2::reps] = extremes[rng.integers(0, len(extremes), n // reps)], extremes[rng.integers(0, len(extremes), n // reps)]
    c = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    co = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    c[0::reps], co[0::reps] = 255, 0
    c[1::reps], co[1::reps] = 0, 255
    c[3::reps], co[3::reps] = 255, 255
    c[4::reps], co[4::reps] = 0, 0
    a, obs = voxels(s, c, wa), voxels(ob, co, wo)
    fused = combine_numpy(hp, a, obs)
    some = rng.choice(n, 3000, replace=False)
    assert fused[some].tobytes() == SM.combine_voxels(hp, a[some], obs[some]).tobytes(), "the numpy combineVoxel is not the oracle's"
    back = DI.take_out(hp, fused, obs)
    assert np.array_equal(back["weight"], wa), "the weight does not come back exactly"
    W = wa.astype(np.float64) + wo.astype(np.float64)
    err = np.abs(back["sdf"].astype(np.float64) - s.astype(np.float64))
    bound = DI.sdf_bound(hp, depth, W, wa)
    print("sdf: largest error / bound", float((err / bound).max()))
    assert (err <= bound).all(), f"sdf error {err.max()} over its bound at {np.argmax(err / bound)}"
    if weighted:
        cerr = np.abs(back["color"].astype(np.int64) - c.astype(np.int64))
        cbound = np.floor(W / (2.0 * wa) + 0.5).astype(np.int64)[:, None]
        print("colour: largest error", int(cerr.max()), "largest bound", int(cbound.max()))
        assert (cerr <= cbound).all()
        assert (cerr[cbound[:, 0] == 0] == 0).all()
    else:
        assert np.array_equal(back["color"], fused["color"]), "the running average's colour is left alone"


# ------------------------------------------------------------------------------------------------ the boundary cases

@pytest.mark.parametrize("weighted", [False, True], ids=["running average", "weighted"])
def test_boundary_cases_of_the_rule(weighted):
    hp = config(weighted)[0]
    zero = np.zeros(1, T.VOXEL_DTYPE)
    v = voxels(f32(0.125), [[10, 200, 30]], 7)
    # wo == w and wo > w reset the voxel
    for wo in (7, 8, 255):
        assert DI.take_out(hp, v, voxels(f32(-0.3), [[1, 2, 3]], wo)).tobytes() == zero.tobytes()
    # no observation, or a voxel of weight 0 (with sdf bits and colours): the bytes stay
    assert DI.take_out(hp, v, zero).tobytes() == v.tobytes()
    assert DI.take_out(hp, v, voxels(f32(0.5), [[9, 9, 9]], 0)).tobytes() == v.tobytes()
    empty = voxels(f32(1.5), [[4, 5, 6]], 0)
    assert DI.take_out(hp, empty, voxels(f32(0.1), [[1, 2, 3]], 3)).tobytes() == empty.tobytes()
    # an ordinary case by hand: (0.125 * 7 - (-0.25) * 3) / 4
    out = DI.take_out(hp, v, voxels(f32(-0.25), [[10, 0, 255]], 3))
    assert out["weight"][0] == 4 and out["sdf"][0] == f32((0.125 * 7 + 0.25 * 3) / 4)
    if weighted:
        # n = c w - co wo: 10 * 7 - 10 * 3 = 40 -> 10; 200 * 7 - 0 = 1400 -> 350 clamps to 255; 30 * 7 - 255 * 3 = -555 floors below 0 -> 0
        assert out["color"][0].tolist() == [10, 255, 0]
        # round half up, and floor for a negative n: (2 n + w') // (2 w') with w' = 2: n = 5 -> 3 (2.5 rounds up), n = -1 -> -1 -> 0, n = -5 -> -2 -> 0
        got = DI.take_out(hp, voxels(f32(0), [[1, 0, 0]], 5), voxels(f32(0), [[0, 1, 5]], 3))
        assert got["weight"][0] == 2 and got["color"][0].tolist() == [3, 0, 0]
        assert (2 * -1 + 2) // 4 == 0 and (2 * -5 + 2) // 4 == -2
    else:
        assert out["color"][0].tolist() == [10, 200, 30]


# ------------------------------------------------------------------------------------------------ a whole frame

@pytest.mark.parametrize("weighted", [False, True], ids=["running average", "weighted"])
def test_integrate_then_deintegrate_on_an_empty_scene_is_the_empty_scene(oracle_lib, weighted):
    O = oracle_lib
    hp, cp, rp = config(weighted)
    pose = synth.orbit_pose(0, 40)
    frame = O.synth_frame(synth.S1_SPHERES, 0, pose, cp)
    o = O.OracleScene(hp, cp, rp, options())
    o.integrate(pose, *frame)
    scene = SM.scene_of(o.state())
    assert len(scene[0]) > 100 and (scene[1]["weight"] > 0).any()
    got = DI.deintegrate(scene, frame, pose, hp, cp)
    c = got["counts"]
    assert len(got["positions"]) == 0 and c["freed"] == c["processed"] == c["blocks_in"] == len(scene[0])
    assert c["voxels_changed"] == c["voxels_reset"] == int((scene[1]["weight"] > 0).sum()) and c["voxels_at_cap"] == 0
    assert c["changed"] <= c["freed"]
    # counting alone leaves the scene
    counted = DI.deintegrate(scene, frame, pose, hp, cp, count_only=True)
    assert counted["counts"] == c and SM.same_scene((counted["positions"], counted["voxels"]), scene)
    # from another pose the frame's observations are not the ones that went in: something is left, nothing is wrong
    other = synth.orbit_pose(3, 40)
    left = DI.deintegrate(scene, O.synth_frame(synth.S1_SPHERES, 0, other, cp), other, hp, cp)
    assert 0 < len(left["positions"]) <= len(scene[0])
