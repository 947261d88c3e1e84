"""Pins the yardstick of the batch queries (tests/ray_query.py): the restatement of traverseCoarseGridSimpleSampleAll for
given rays, fed the rays renderKernel builds for the pixels of a view, must reproduce OracleScene.render bit for bit;
and each of its refusal rules holds.  No device: these tests pass with or without the queries themselves."""
import numpy as np
import pytest

import ray_query as RQ
from helpers import bits, small_config
from voxelhashing_amd import synth, vhtypes as T

f32 = np.float32


@pytest.fixture(scope="module")
def model(oracle_lib):
    """S1 at 64x48 (P4), three offline frames, rendered with gradients from a fourth pose"""
    O = oracle_lib
    hp, cp, rp = small_config(64, 48)
    rp.m_useGradients = 1
    o = O.OracleScene(hp, cp, rp, T.make_scene_options(offline=True))
    for k in range(3):
        pose = synth.orbit_pose(k, n_frames=100)
        o.integrate(pose, *O.synth_frame(synth.S1_SPHERES, 0, pose, cp))
    view = synth.orbit_pose(5, n_frames=100)
    maps = o.render(view)
    return dict(O=O, o=o, cp=cp, rp=o.rp, maps=maps, view=view)


def test_camera_rays_reproduce_the_oracle_render(model):
    o, rp, maps = model["o"], model["rp"], model["maps"]
    cam = RQ.camera_rays(o.L, model["cp"], rp)
    got = RQ.rays(o.L, o.hd, o.hp, rp, cam["origins"], cam["directions"], cam["t_min"], cam["t_max"])
    n = rp.m_width * rp.m_height
    depth, colors, normals = maps["depth"].reshape(n), maps["colors"].reshape(n, 4), maps["normals"].reshape(n, 4)
    hit = got["status"] == RQ.HIT
    assert np.array_equal(hit, depth != -np.inf), "a miss is a miss"
    assert not (got["status"] == RQ.REFUSED).any()
    assert hit.sum() >= 1000 and (~hit).sum() >= 1000, (hit.sum(), (~hit).sum())
    with np.errstate(all="ignore"):
        assert np.array_equal(bits(got["t"][hit] / cam["depth_to_ray_length"][hit]), bits(depth[hit])), "t / depthToRayLength = depth"
    rgb = np.stack([got["color"] & 0xff, (got["color"] >> 8) & 0xff, (got["color"] >> 16) & 0xff], axis=-1).astype(f32) / f32(255)
    assert np.array_equal(bits(rgb[hit]), bits(colors[hit, :3])), "colour / 255 = colors"
    cam_normals = np.stack([RQ.mat_mul_d(rp.m_viewMatrix, v) for v in got["normal"][hit]])
    assert np.array_equal(bits(cam_normals), bits(normals[hit, :3])), "viewMatrix * normal = normals"
    miss = ~hit
    assert np.all(got["t"][miss] == -np.inf) and np.all(got["normal"][miss] == -np.inf) and np.all(got["color"][miss] == 0)
    assert np.all(colors[miss] == -np.inf) and np.all(normals[miss] == -np.inf)


def test_refusal_rules_of_the_restatement(model):
    o, rp = model["o"], model["rp"]
    m = RQ.Model(o.L, o.hd, o.hp)
    inc = f32(rp.m_rayIncrement)
    o3, d3 = np.array([0, 0, -2.5], f32), np.array([0, 0, 1], f32)

    def cast(o=o3, d=d3, t0=0.5, t1=5.0):
        return RQ.cast(m, inc, rp.m_thresSampleDist, rp.m_thresDist, o, d, f32(t0), f32(t1))

    status, t, normal, color, samples = cast()
    assert status == RQ.HIT and samples > 1 and np.isfinite(t) and np.all(np.isfinite(normal))
    for bad in (np.nan, np.inf, -np.inf):
        for what in (dict(o=np.array([0, bad, -2.5], f32)), dict(d=np.array([bad, 0, 1], f32)), dict(t0=bad), dict(t1=bad)):
            got = cast(**what)
            assert got[0] == RQ.REFUSED and got[1] == -np.inf and np.all(got[2] == -np.inf) and got[3] == 0 and got[4] == 0, (bad, what)
    assert cast(d=np.zeros(3, f32))[0] == RQ.REFUSED
    assert cast(d=np.array([0, -0.0, 0], f32))[0] == RQ.REFUSED
    # the interval: 65536 increments are marched, 65537 are not
    assert cast(t0=0.0, t1=f32(65537) * inc)[0] == RQ.REFUSED
    assert cast(t0=0.0, t1=f32(65536) * inc)[0] != RQ.REFUSED
    # an empty interval takes no sample
    assert cast(t0=5.0, t1=5.0)[::4] == (RQ.MISS, 0) and cast(t0=5.0, t1=0.5)[::4] == (RQ.MISS, 0)


def test_sample_cap_stops_a_stalled_march(model):
    """t + increment == t: the interval passes the refusal rule (it is short) but the march cannot advance; the count of
    samples ends it"""
    o, rp = model["o"], model["rp"]
    m = RQ.Model(o.L, o.hd, o.hp)
    inc = f32(rp.m_rayIncrement)
    t0 = f32(2.0 ** 24) * inc * f32(4)  # the increment is below half an ulp of t
    assert t0 + inc == t0
    t1 = np.nextafter(t0, f32(np.inf))
    status, _, _, _, samples = RQ.cast(m, inc, rp.m_thresSampleDist, rp.m_thresDist, np.array([0, 0, -2.5], f32), np.array([0, 0, 1e-9], f32), t0, t1)
    assert status == RQ.MISS and samples == RQ.MAX_SAMPLES


def test_point_reference_reports_invalid_points_as_minus_infinity(model):
    o = model["o"]
    pts = np.array([[0, 0, -1.0], [50, 50, 50], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], f32)
    got = RQ.points(o.L, o.hd, o.hp, pts)
    assert got["valid"].tolist() == [1, 0, 0, 0, 0]
    assert np.isfinite(got["sdf"][0]) and np.all(got["sdf"][1:] == -np.inf) and np.all(got["color"][1:] == 0)
    assert np.any(got["gradient"][0] != 0) and np.all(got["gradient"][2:] == 0)
