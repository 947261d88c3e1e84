"""The weighted colour average (HashParams.m_colorIntegration = 1) on the device: the colour step over every input, every
shape of the pass over the voxels, the certified blocks' pair code on crafted payloads, the switch, the native frame loop,
and what the rule is for -- an RGB-D tracker that follows its own reconstruction.  Block set, sdf, weights and heap are
held against the oracle, colours against the rule in numpy (tests/weighted_colour.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rgbd_icp as G
import weighted_colour as WC
from helpers import small_config
from test_gpu_native_rgbd_tracking import assert_same_run, write_plane_sequence
from test_rgbd_tracking import PlaneRig, all_colour_settings, pose_error
from voxelhashing_amd import canonical, synth, vhtypes as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINF = np.float32(-np.inf)


@pytest.fixture(scope="module")
def E(vh):
    from voxelhashing_amd import engine
    return engine


def weighted(hp):
    hp.m_colorIntegration = T.COLOR_WEIGHTED_AVERAGE
    return hp


def test_colour_step_on_every_input(vh):
    """vh_debug_check_weighted_colour: the device function over all 256 * 256 * 256 * 255 (c0, w0, c1, w1), w1 >= 1, with
    the reciprocal of combine_voxel (1.0f / d) and with the certified path's (rcp_refined2), against
    floor((2 n + d) / (2 d))"""
    from voxelhashing_amd.lib import DeviceBuffer, check
    buf = DeviceBuffer(16)
    check(vh.vh_debug_check_weighted_colour(buf.ptr, None), "check")
    out = buf.download(np.uint32)
    first = int(out[2])
    where = dict(c0=first & 255, w0=(first >> 8) & 255, c1=(first >> 16) & 255, w1=first >> 24)
    assert out[0] == 0 and out[1] == 0, f"mismatches: {out[0]} with 1.0f / d, {out[1]} with the refined reciprocal; first at {where}"
    assert first == 0xFFFFFFFF


def run(E, hp, cp, rp, scene_name, n_frames, n_orbit, opt):
    """tests/test_gpu_integrate_shapes.py's run with the rule on -> most blocks in view"""
    from oracle import oracle as O
    spheres, inside, radius = synth.scene(scene_name)
    scene, ref = E.CUDASceneRepHashSDF(weighted(hp), opt), WC.WeightedColourScene(hp, cp, rp, opt)
    assert scene.getColorIntegration() == 1
    frame = E.DepthFrame(cp)
    most = 0
    for k in range(n_frames):
        pose = synth.orbit_pose(k, n_orbit, radius)
        E.synth_frame(spheres, inside, pose, cp, out=frame)
        d, c = O.synth_frame(spheres, inside, pose, cp)
        scene.integrate(pose, frame, cp, None)
        ref.integrate(pose, d, c)
        most = max(most, scene.getNumOccupiedBlocks())
        canonical.assert_same_scene(scene.state(), ref.state(), f"{scene_name} frame {k}")
    # the rule is not the running average here: the oracle's own colours differ
    assert any(not np.array_equal(ref.colours[p], c) for p, c in ref.last["oracle_colours"].items() if p in ref.colours)
    assert scene.getState()[T.STATE_HEAP_UNDERFLOW] == 0
    ref.close()
    return most


def test_workgroup_per_block_shape(E, oracle_lib):
    hp, cp, rp = small_config(160, 120, params="P4")
    most = run(E, hp, cp, rp, "S3", 5, 100, T.make_scene_options(offline=True, gc=False))
    assert 50 < most < 2048


@pytest.mark.parametrize("width,height,what", [(160, 120, "footprints of ~17 pixels: staged"), (320, 240, "footprints of ~34 pixels: gathered")])
def test_wave_per_block_shape_small_pool(E, oracle_lib, width, height, what):
    hp, cp, rp = small_config(width, height, params="P4", num_buckets=1 << 14, num_sdf_blocks=512)
    most = run(E, hp, cp, rp, "S1", 7, 150, T.make_scene_options(offline=True, gc=True, starve=3))
    assert 128 < most <= 512, most


def test_wave_per_block_shape_many_rounds(E, oracle_lib):
    hp, cp, rp = small_config(320, 240, params="P1", num_buckets=1 << 17, num_sdf_blocks=1 << 14)
    most = run(E, hp, cp, rp, "S2", 2, 400, T.make_scene_options(offline=True, gc=True, starve=2))
    assert most > 5120 + 64, most  # more than one round (kIntegrateWavesMost = 5120)


def test_reference_launch_sequence(E, oracle_lib):
    """s_useReferenceLaunchSequence: k_integrate<false>, then starve and the two garbage collection kernels"""
    hp, cp, rp = small_config(160, 120, params="P4")
    most = run(E, hp, cp, rp, "S1", 4, 150, T.make_scene_options(offline=True, gc=True, starve=2, reference_launch_sequence=True))
    assert most > 50


@pytest.mark.parametrize("weight_sample", [1, 10, 170])
def test_certified_blocks_with_crafted_voxels(E, oracle_lib, weight_sample):
    """tests/test_gpu_integrate_shapes.py's rig (a wall at 2.5 m seen from an oblique pose, blocks streamed into the free
    space in front of it, where every voxel integrates, 512 < blocks <= 2048: the wave-per-block shape and its certified
    pair code) with stored colours and weights over the full byte range, 0 and 255 included, and observation weights of 1
    (m_integrationWeightSample = 1), 8 (10) and 140..142 (170) at the wall's depth: denominators 1..397, half of them
    even, with their ties."""
    from voxelhashing_amd.lib import DeviceBuffer
    hp, cp, rp = small_config(160, 120, params="P2", num_buckets=1 << 12, num_sdf_blocks=2048, weight_sample=weight_sample)
    weighted(hp)
    rng = np.random.default_rng(20260 + weight_sample)
    W, H = cp.m_imageWidth, cp.m_imageHeight
    depth = np.full((H, W), 2.5, np.float32) + rng.uniform(-0.02, 0.02, (H, W)).astype(np.float32)
    depth[rng.random((H, W)) < 0.03] = -np.inf
    color = np.concatenate([rng.random((H, W, 3), dtype=np.float32), np.ones((H, W, 1), np.float32)], axis=2)
    color[rng.random((H, W)) < 0.02, :3] = -np.inf
    a, b, c = np.radians([17.0, -23.0, 9.0])
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    pose = np.eye(4)
    pose[:3, :3] = rz @ ry @ rx
    pose[:3, 3] = [3.1, -1.7, 2.3]
    pose = pose.astype(np.float32).reshape(16)
    z = rng.uniform(0.9, 2.1, 600)
    pts = np.stack([rng.uniform(-0.4, 0.4, 600) * z, rng.uniform(-0.3, 0.3, 600) * z, z, np.ones(600)], axis=1)
    ids = np.unique(np.floor((pts @ pose.reshape(4, 4).astype(np.float64).T)[:, :3] / (8 * hp.m_virtualVoxelSize)).astype(np.int32), axis=0)[:200]
    assert len(ids) > 150, len(ids)
    blocks = np.zeros((len(ids), T.SDF_BLOCK_VOXELS), T.VOXEL_DTYPE)
    blocks["sdf"] = rng.normal(0, 0.2, blocks.shape).astype(np.float32)
    blocks["weight"] = rng.integers(0, 256, blocks.shape, dtype=np.uint8)
    blocks["weight"][rng.random(blocks.shape) < 0.1] = 0
    blocks["weight"][rng.random(blocks.shape) < 0.1] = 255
    blocks["color"] = rng.integers(0, 256, blocks.shape + (3,), dtype=np.uint8)
    descs = np.zeros(len(ids), T.DESC_DTYPE)
    descs["pos"] = ids

    g = E.LauncherScene(hp)
    # (the oracle starves on frames k > 0 with k % s_garbageCollectionStarve == 0: frame 1 of starve = 1 is the pass below, flags 3)
    ref = WC.WeightedColourScene(hp, cp, rp, T.make_scene_options(offline=True, gc=True, starve=1))
    o = ref.o
    g.set_transform(pose, oracle_lib.mat4_inverse(pose))
    o.set_transform(pose)
    g.reset_mutex()
    g.stream_in(descs, blocks, T.LOCK_ENTRY)
    assert o.stream_in(descs, blocks) == 0
    ref.set_colours(ids, blocks["color"])
    o.frames.value = 1
    frame = E.DepthFrame(cp, depth, color)
    packed = DeviceBuffer(8 * W * H)
    job = g.frame_job(frame, cp, packed_ptr=packed.ptr)
    prev = -1
    while True:  # alloc until the heap stops changing; every pass packs the frame as well
        g.reset_mutex()
        g.alloc_job(job)
        cur = g.download(with_voxels=False)["heap_counter"]
        if cur == prev:
            break
        prev = cur
    n = g.compactify(cp)
    assert 512 < n <= 2048, n  # 512 workgroups: the wave-per-block shape
    g.reset_mutex()
    g.integrate_fused(frame, cp, 3, T.LOCK_ENTRY, packed.ptr)  # VH_FUSED_GC | VH_FUSED_STARVE
    ref.integrate(pose, depth, color)
    assert ref.last["starved"] and o.hp.m_numOccupiedBlocks == n
    canonical.assert_same_scene(g.state(), ref.state(), "after the fused pass")
    # the crafted voxels were blended, with every kind of denominator
    hit = np.concatenate([(ref.last["w1"][bid] > 0) & (ref.last["w0"][bid] > 0) for pos, bid in ref.last["before"].items()])
    d = np.concatenate([ref.last["w1"][bid] + ref.last["w0"][bid] for pos, bid in ref.last["before"].items()])[hit]
    assert hit.sum() > 30000 and (d % 2 == 0).sum() > 10000 and d.max() >= 256, (hit.sum(), d.max())
    ref.close()


def test_off_means_off_and_a_switch_takes_effect_on_the_next_frame(E, oracle_lib):
    """word 0: the oracle bit for bit (the helper under combineVoxel's own rule is the oracle: test_weighted_colour.py);
    setColorIntegration between frames changes the frames that follow and nothing else; a mode other than 0 and 1 is
    refused and leaves the mode alone"""
    from voxelhashing_amd.lib import VhError
    O = oracle_lib
    hp, cp, rp = small_config(160, 120, params="P4")
    opt = T.make_scene_options(offline=True, gc=True, starve=2)
    scene, ref, plain = E.CUDASceneRepHashSDF(hp, opt), WC.WeightedColourScene(hp, cp, rp, opt), O.OracleScene(hp, cp, rp, opt)
    assert scene.getColorIntegration() == 0
    spheres, inside, radius = synth.scene("S1")
    frame = E.DepthFrame(cp)
    modes = [0, 0, 1, 1, 0, 1]
    for k, mode in enumerate(modes):
        pose = synth.orbit_pose(k, 150, radius)
        E.synth_frame(spheres, inside, pose, cp, out=frame)
        d, c = O.synth_frame(spheres, inside, pose, cp)
        scene.setColorIntegration(mode)
        assert scene.getColorIntegration() == mode
        with pytest.raises(VhError):
            scene.setColorIntegration(2)
        assert scene.getColorIntegration() == mode
        scene.integrate(pose, frame, cp, None)
        ref.rule = WC.rule_weighted if mode else WC.rule_running
        ref.integrate(pose, d, c)
        canonical.assert_same_scene(scene.state(), ref.state(), f"frame {k}, mode {mode}")
        if k < 2:  # nothing but the running average so far: the oracle itself
            plain.integrate(pose, d, c)
            canonical.assert_same_scene(scene.state(), plain.state(), f"frame {k}, rule off, against the oracle")
    ref.close()


def test_native_loop_with_riders(E, oracle_lib):
    """the native frame loop in online mode (alloc rides in the ray caster's launch, compactify and -- with few blocks --
    the pass over the voxels in computeNormals'), rule on: the scene after every frame equals the class-by-class path's
    and the reference's"""
    O = oracle_lib
    hp, cp, rp = small_config(160, 120, params="P4", num_buckets=1 << 16, num_sdf_blocks=1 << 12)
    weighted(hp)
    opt = T.make_scene_options(offline=False, gc=True, starve=2)
    # S1 away from the origin: the hash sends (x, y, z) and (-x, -y, z) to one bucket, and which of the two an online
    # alloc pass serves first is a matter of scheduling (tests/test_gpu_frame_loop.py)
    off = np.array([7.3, 5.1, 3.7])
    spheres = synth.S1_SPHERES.copy()
    spheres[:, :3] += off
    poses = []
    for k in range(6):
        q = np.array(synth.orbit_pose(k, 90), dtype=np.float32).copy()
        q[3] += np.float32(off[0]); q[7] += np.float32(off[1]); q[11] += np.float32(off[2])
        poses.append(q)
    scene, ray, ref = E.CUDASceneRepHashSDF(hp, opt), E.CUDARayCastSDF(rp), WC.WeightedColourScene(hp, cp, rp, opt)
    by_class = E.CUDASceneRepHashSDF(hp, opt)
    frames = [E.synth_frame(spheres, 0, p, cp) for p in poses]
    recon = E.Reconstruction(scene, ray, None, cp)
    seq = E.Reconstruction.makeFrames(poses, [f.depth_ptr for f in frames], [f.color_ptr for f in frames])
    for k, pose in enumerate(poses):
        recon.run(seq, k, 1)
        recon.synchronize()
        if k > 0:  # the ray cast shows the weighted colours
            got, want = ray.download(), ref.render(poses[k - 1])
            for m in ("depth", "depth4", "colors", "normals"):
                assert np.array_equal(got[m].view(np.uint32), want[m].view(np.uint32)), f"frame {k}: ray-cast map {m} differs"
        by_class.integrate(pose, frames[k], cp, None)
        ref.integrate(pose, *O.synth_frame(spheres, 0, pose, cp))
        canonical.assert_same_scene(scene.state(), by_class.state(), f"frame {k}: native loop against integrate()")
        canonical.assert_same_scene(scene.state(), ref.state(), f"frame {k}: native loop against the reference")
    ref.close()


@pytest.fixture(scope="module")
def plane_runs(vh, oracle_lib, tmp_path_factory):
    """the 8-frame textured-plane `.sens` without recorded poses, RGB-D tracker, rule on: through the Python loop and
    through run_native with the tracker inside the loop"""
    from voxelhashing_amd import reconstruction as R
    truth, sens, params, tracking = write_plane_sequence(tmp_path_factory.mktemp("plane"))
    make = lambda: R.Reconstruction(R.read_app_state(params), R.read_tracking_state_rgbd(tracking), [sens], use_rgbd_tracking=True, weighted_colour=True)
    py = make()
    assert py.scene.getColorIntegration() == 1
    want = [py.frame() for _ in truth]
    assert py.frame() is None
    nat = make()
    assert nat.run_native(tracking=True, tracking_rgbd=True, batch=4) == len(truth)
    return dict(truth=truth, py=py, nat=nat, want=want, files=(sens, params, tracking))


def test_run_native_equals_the_python_loop_with_the_rgbd_tracker(plane_runs):
    py, nat, n = plane_runs["py"], plane_runs["nat"], len(plane_runs["truth"])
    got = assert_same_run(nat, py, n, "native RGB-D loop vs Python RGB-D loop, weighted colours")
    for k in range(n):
        assert np.array_equal(got[k], plane_runs["want"][k]), k


def assert_loop_closed(poses, truth, what):
    for k in range(1, len(truth)):
        assert poses[k] is not None and np.asarray(poses[k]).reshape(-1)[0] != MINF, f"{what}: frame {k} lost"
        dt, da = pose_error(poses[k], truth[k])
        print(f"{what}: frame {k}: {1e3 * dt:.3f} mm, {da:.4f} degrees")
        assert dt < 0.003 and da < 0.1, (what, k, dt, da)


def test_rgbd_tracker_follows_its_own_reconstruction(E, oracle_lib, plane_runs):
    """The capability.  The camera moves 12 mm / -3 mm a frame in the textured plane's own plane; every frame is tracked
    by the RGB-D tracker (colour on every level) against the ray cast of what has been integrated so far, and integrated
    at the tracked pose.  With the weighted average every frame stays within 3 mm and 0.1 degrees of the truth and none
    is lost -- class by class (CUDACameraTrackingMultiResRGBD.applyCT), and inside the native loop (setTrackingRGBD,
    through Reconstruction.run_native on the same frames as a `.sens`).  Under the running average the first tracked
    frame is already 60 mm off (tests/test_weighted_colour.py)."""
    cp = T.make_depth_camera_params(160, 120)
    truth = [G.plane_pose(0.012 * k, -0.003 * k) for k in range(8)]
    rig = PlaneRig(E, cp)
    rig.scene.setColorIntegration(T.COLOR_WEIGHTED_AVERAGE)
    ts = all_colour_settings()
    pose, poses = truth[0], [truth[0]]
    rig.feed(pose)
    rig.integrate(pose)
    for k in range(1, len(truth)):
        rig.feed(truth[k])
        got, lost = rig.track_rgbd(pose, ts)
        poses.append(None if lost else got)
        assert not lost, k
        pose = np.asarray(got, np.float32).reshape(16)
        rig.integrate(pose)
    assert_loop_closed(poses, truth, "class by class")
    # the native loop (the file's tracking settings: colour on every level as well; its world is the first camera, the identity here)
    nat = plane_runs["nat"]
    assert nat.lost_frames == 0 and nat.native.getStats()["trackedFrames"] == len(truth) - 1
    assert_loop_closed(list(nat.native.getPoses()), plane_runs["truth"], "native loop")


@pytest.mark.parametrize("extra", [[], ["--native", "--native-tracking"]])
def test_replay_tool_with_weighted_colour(plane_runs, extra):
    sens, params, tracking = plane_runs["files"]
    cmd = [sys.executable, os.path.join(ROOT, "tools", "replay.py"), "--params", params, "--tracking", tracking, "--rgbd-tracking", "--sens", sens,
           "--weighted-colour"] + extra
    out = json.loads(subprocess.check_output(cmd, timeout=600).decode().strip().splitlines()[-1])
    assert out["frames"] == len(plane_runs["truth"]) and out["pose_source"] == "RGB-D ICP" and out["colour_rule"] == "weighted", out
    assert out["lost_frames"] == 0, out
