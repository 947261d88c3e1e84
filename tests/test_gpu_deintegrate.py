"""Frame de-integration on the device (vh_deintegrate.hip) against the numpy restatement of its definition
(tests/deintegrate.py), applied to the table downloaded before the call: block set, voxel bytes, heap and counts.  The
rule alone on crafted pairs; S1 at 64x48 from two poses, taken out again in both colour modes; the weight cap; count
only; a frustum that holds nothing; a camera with fx != fy and an off-centre principal point; the crowded-table
sequences A and B (tests/crowded.py), every frame of which is taken out again until the last one frees whole collision
lists; a ray cast and an integrate afterwards; reintegrate; the refusals and Reconstruction's methods.  Every downloaded
state goes through state(), which checks the invariants (a free block is all zero among them), follows every list
(canonical.check_chains) and compares the bucket summary."""

import numpy as np
import pytest

import camera_models as CM
import crowded as CR
import deintegrate as DI
import scene_merge as SM
from helpers import assert_maps_equal, small_config
from voxelhashing_amd import canonical, synth, vhtypes as T

pytestmark = pytest.mark.gpu
V = T.SDF_BLOCK_VOXELS
POOL = 1 << 11
A_POSE, B_POSE = 0, 2  # frames A and B: the orbit's poses 0 and 2 of 40


@pytest.fixture(scope="module")
def E(vh):
    from voxelhashing_amd import engine
    return engine


def config(weighted=False, pool=POOL, **over):
    hp, cp, rp = small_config(64, 48, "P4", num_sdf_blocks=pool, **over)
    hp.m_colorIntegration = T.COLOR_WEIGHTED_AVERAGE if weighted else 0
    return hp, cp, rp


def options():
    return T.make_scene_options(offline=True, gc=False)


def frame_at(E, cp, pose, spheres=synth.S1_SPHERES):
    """-> (the frame on the device, (depth, colour) as the device holds them)"""
    frame = E.synth_frame(spheres, 0, pose, cp)
    return frame, frame.download()


def new_scene(E, hp, weighted=False, opt=None):
    scene = E.CUDASceneRepHashSDF(hp, opt or options())
    if weighted:
        scene.setColorIntegration(T.COLOR_WEIGHTED_AVERAGE)
    return scene


def raw_equal(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a if k != "params")


def assert_is(snap, want, what):
    assert np.array_equal(snap["positions"], want["positions"]), f"{what}: block position sets differ"
    assert snap["voxels"].tobytes() == want["voxels"].tobytes(), f"{what}: voxel bytes differ"


def deintegrate_checked(scene, frame, maps, pose, cp, what):
    """scene.deintegrate, everything against the restatement applied to the table before the call -> (counts, restatement)"""
    hp = scene.getHashParams()
    before = scene.state()
    last = scene.getLastRigidTransform().copy()
    want = DI.deintegrate(SM.scene_of(before), maps, pose, hp, cp)
    got = scene.deintegrate(pose, frame, cp)
    print(what, got)
    DI.assert_counts(got, want["counts"], what)
    assert got["unsettled"] == 0 and got["delete_passes"] <= got["freed"] + 8 and (got["delete_passes"] == 0) == (got["freed"] == 0)
    after = scene.state()
    assert_is(after, want, what)
    assert after["heap_free"] == hp.m_numSDFBlocks - len(want["positions"])
    assert np.array_equal(scene.getLastRigidTransform().view(np.uint32), last.view(np.uint32)), f"{what}: the scene's last rigid transform was changed"
    return got, want


# ------------------------------------------------------------------------------------------------ 1. the rule alone

@pytest.mark.parametrize("weighted", [False, True], ids=["running average", "weighted"])
def test_rule_on_crafted_pairs(E, weighted):
    hp = config(weighted)[0]
    w, wo = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    colours = np.array([(0, 0), (0, 255), (255, 0), (255, 255), (1, 0), (0, 1), (254, 255), (255, 254), (128, 127), (127, 128), (17, 201), (201, 17),
                        (100, 100), (3, 250), (250, 3), (64, 192)], np.uint8)
    sdf_bits = np.array([0x00000000, 0x80000000, 0x3e000000, 0xbe000000, 0x3e4ccccd, 0xbe4ccccd, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff,
                         0x00800000, 0x3dcccccd, 0xbdcccccd, 0x3f000000, 0xbf000000, 0x33d6bf95], np.uint32)
    n = 256 * 256 * 16
    k = np.arange(n)
    pair, col = k // 16, k % 16
    stored, obs = np.zeros(n, T.VOXEL_DTYPE), np.zeros(n, T.VOXEL_DTYPE)
    stored["weight"], obs["weight"] = w.reshape(-1)[pair], wo.reshape(-1)[pair]
    stored["color"] = np.stack([colours[col, 0], colours[(col + 5) % 16, 0], colours[(col + 11) % 16, 0]], axis=-1)
    obs["color"] = np.stack([colours[col, 1], colours[(col + 5) % 16, 1], colours[(col + 11) % 16, 1]], axis=-1)
    stored["sdf"] = sdf_bits[(col + pair) % 16].view(np.float32)          # (a weight-0 voxel with sdf bits among them)
    obs["sdf"] = sdf_bits[(3 * col + 7 * pair + 1) % 16].view(np.float32)
    assert ((stored["weight"] == 0) & (stored["sdf"].view(np.uint32) != 0)).any()
    want = DI.take_out(hp, stored, obs)
    got = E.deintegrate_rule(stored, obs, hp)
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    assert len(bad) == 0, f"{len(bad)} of {n} differ, first: stored {stored[bad[0]]} observed {obs[bad[0]]} -> {got[bad[0]]}, the rule says {want[bad[0]]}"
    if weighted:
        assert (want["color"] != stored["color"]).any()


# ------------------------------------------------------------------------------------------------ 2. S1, frames A and B

@pytest.fixture(scope="module")
def s1(E):
    """frames A and B of S1 at 64x48 (the device's maps, downloaded once), only read"""
    cp = config()[1]
    out = {}
    for name, k in (("A", A_POSE), ("B", B_POSE)):
        pose = synth.orbit_pose(k, 40)
        frame, maps = frame_at(E, cp, pose)
        out[name] = dict(pose=pose, frame=frame, maps=maps)
    return out


@pytest.mark.parametrize("weighted", [False, True], ids=["running average", "weighted"])
def test_a_then_b_then_b_taken_out(E, s1, weighted):
    hp, cp, _ = config(weighted)
    a, b = s1["A"], s1["B"]
    alone = new_scene(E, hp, weighted)
    alone.integrate(a["pose"], a["frame"], cp, None)
    only_a = alone.state()
    scene = new_scene(E, hp, weighted)
    scene.integrate(a["pose"], a["frame"], cp, None)
    scene.integrate(b["pose"], b["frame"], cp, None)
    both = SM.scene_of(scene.state())
    got, want = deintegrate_checked(scene, b["frame"], b["maps"], b["pose"], cp, "A + B - B")
    assert 0 < got["freed"] < got["processed"] <= got["blocks_in"] and got["voxels_reset"] > 0 and got["voxels_changed"] > got["voxels_reset"]
    assert scene.getNumIntegratedFrames() == 2, "a de-integration is not a frame"
    # against A alone: nothing was at the cap, so the comparison leaves nothing out
    assert got["voxels_at_cap"] == 0
    after = scene.state()
    va, vb = CR.voxels_by_position(only_a), CR.voxels_by_position(after)
    observed = lambda vox: {p for p, v in vox.items() if np.frombuffer(v, T.VOXEL_DTYPE)["weight"].any()}
    assert observed(va) == observed(vb), "A + B - B and A do not hold the same observed blocks"
    pos = np.array(sorted(observed(va)), np.int32)
    xa = np.stack([np.frombuffer(va[tuple(p)], T.VOXEL_DTYPE) for p in pos.tolist()])
    xb = np.stack([np.frombuffer(vb[tuple(p)], T.VOXEL_DTYPE) for p in pos.tolist()])
    assert np.array_equal(xa["weight"], xb["weight"]), "the weights did not come back"
    obs, depth = DI.observe(b["maps"], b["pose"], hp, cp, pos, with_depth=True)
    obs[~DI.block_in_frustum(b["pose"], hp, cp, pos)] = np.zeros((), T.VOXEL_DTYPE)
    seen = (obs["weight"] > 0) & (xa["weight"] > 0)
    assert seen.sum() > 1000
    assert xa[~seen].tobytes() == xb[~seen].tobytes(), "a voxel B did not observe changed"
    wa, wo = xa["weight"][seen].astype(np.float64), obs["weight"][seen].astype(np.float64)
    trunc = np.float64(hp.m_truncation) + np.float64(hp.m_truncScale) * depth[seen].astype(np.float64)
    bound = 8.0 * 2.0 ** -24 * trunc * (wa + wo) / wa
    err = np.abs(xa["sdf"][seen].astype(np.float64) - xb["sdf"][seen].astype(np.float64))
    print("sdf: largest error / bound", float((err / bound).max()))
    assert (err <= bound).all()
    if weighted:
        cerr = np.abs(xa["color"][seen].astype(np.int64) - xb["color"][seen].astype(np.int64))
        assert (cerr <= np.floor((wa + wo) / (2.0 * wa) + 0.5).astype(np.int64)[:, None]).all()
    assert len(both[0]) > len(after["positions"])


def test_a_then_a_taken_out_is_the_empty_table(E, s1):
    hp, cp, _ = config()
    a = s1["A"]
    scene = new_scene(E, hp)
    scene.integrate(a["pose"], a["frame"], cp, None)
    n = scene.state()["num_occupied"]
    got, _ = deintegrate_checked(scene, a["frame"], a["maps"], a["pose"], cp, "A - A")
    assert got["freed"] == got["processed"] == n and got["voxels_changed"] == got["voxels_reset"] > 0
    d = scene.download()
    assert not (d["hash"]["ptr"] != T.FREE_ENTRY).any() and not d["bucket_count"].any() and not d["bucket_bits"].any()
    assert d["heap_counter"] == hp.m_numSDFBlocks - 1
    assert np.array_equal(np.sort(d["heap"]), np.arange(hp.m_numSDFBlocks, dtype=np.uint32)), "the heap is not a permutation of all block ids"
    assert not d["sdf_blocks"].view(np.uint64).any()
    # n = 0: the empty table launches nothing and reports zeros
    assert all(v == 0 for v in scene.deintegrate(a["pose"], a["frame"], cp).values())


# ------------------------------------------------------------------------------------------------ 3. the cap, 4. count only, 5. nothing in view

def launcher(E, scene, hp):
    g = E.LauncherScene(hp)
    descs = np.zeros(len(scene[0]), T.DESC_DTYPE)
    descs["pos"] = scene[0]
    g.stream_in(descs, scene[1], 1)
    return g


def test_weight_cap(E, oracle_lib, s1):
    """three integrations of one frame under a cap the third one reaches"""
    a = s1["A"]
    hp, cp, _ = config(weight_max=30)
    scene = new_scene(E, hp)
    for _ in range(3):
        scene.integrate(a["pose"], a["frame"], cp, None)
    w = scene.state()["voxels"]["weight"]
    assert w.max() == 30 and ((w > 0) & (w < 30)).any(), "the cap was meant to be reached by some voxels and not by others"
    got, want = deintegrate_checked(scene, a["frame"], a["maps"], a["pose"], cp, "under the cap")
    assert 0 < got["voxels_at_cap"] < got["voxels_changed"] and got["voxels_at_cap"] == int(want["at_cap"].sum())
    assert got["voxels_reset"] == 0 and got["freed"] < got["processed"]


def test_count_only_and_nothing_in_view(E, oracle_lib, s1):
    hp, cp, _ = config()
    a, b = s1["A"], s1["B"]
    probe = new_scene(E, hp)
    probe.integrate(a["pose"], a["frame"], cp, None)
    probe.integrate(b["pose"], b["frame"], cp, None)
    scene = SM.scene_of(probe.state())
    inv = oracle_lib.mat4_inverse(b["pose"])
    g = launcher(E, scene, hp)
    before = g.download()
    counted = g.deintegrate_blocks(b["frame"], cp, b["pose"], inv, 2, T.DEINT_COUNT_ONLY)
    assert counted["code"] == 0 and raw_equal(before, g.download()), "counting wrote to the table"
    done = g.deintegrate_blocks(b["frame"], cp, b["pose"], inv, 3)
    want = DI.deintegrate(scene, b["maps"], b["pose"], hp, cp)
    assert done["code"] == 0
    DI.assert_counts(done, want["counts"], "the launcher")
    DI.assert_counts(counted, want["counts"], "count only")
    assert counted["delete_passes"] == 0 and done["delete_passes"] > 0 and done["unsettled"] == 0
    after = g.state()
    assert_is(after, want, "the launcher")
    assert after["heap_free"] == hp.m_numSDFBlocks - len(want["positions"])
    # a camera that looks away from the scene: no block is in its frustum
    away = np.asarray(synth.orbit_pose(A_POSE, 40), np.float32).reshape(4, 4).copy()
    away[:3, 3] += away[:3, 2] * np.float32(-20.0)
    assert not DI.block_in_frustum(away, hp, cp, scene[0]).any()
    g = launcher(E, scene, hp)
    before = g.download()
    got = g.deintegrate_blocks(b["frame"], cp, away, oracle_lib.mat4_inverse(away), 2)
    assert got["code"] == 0 and got["blocks_in"] == len(scene[0])
    assert [got[k] for k in T.DEINT_COUNTS[1:]] == [0] * (len(T.DEINT_COUNTS) - 1), got
    assert raw_equal(before, g.download()), "a frame that sees nothing changed the table"
    # flags that are none are refused
    assert g.deintegrate_blocks(b["frame"], cp, away, oracle_lib.mat4_inverse(away), 2, 6)["code"] == 4


# ------------------------------------------------------------------------------------------------ 6. another camera

def test_off_centre_camera_with_unequal_focal_lengths(E):
    hp, cp, _ = CM.config("offcentre", (64, 48), blocks=POOL)
    assert cp.fx != cp.fy and abs(cp.mx - 31.5) > 5 and abs(cp.my - 23.5) > 5
    poses = CM.place([synth.orbit_pose(k, 40) for k in (A_POSE, B_POSE)], cp)
    scene = new_scene(E, hp)
    frames = [frame_at(E, cp, p, CM.SPHERES) for p in poses]
    for p, (f, _) in zip(poses, frames):
        scene.integrate(p, f, cp, None)
    got, _ = deintegrate_checked(scene, frames[1][0], frames[1][1], poses[1], cp, "offcentre: A + B - B")
    assert got["voxels_changed"] > 1000 and got["freed"] > 0
    got, _ = deintegrate_checked(scene, frames[0][0], frames[0][1], poses[0], cp, "offcentre: - A")
    assert scene.state()["num_occupied"] == 0


# ------------------------------------------------------------------------------------------------ 7. crowded tables

def list_head_middle_tail(table, hp, freed):
    """a bucket whose list's head (the bucket's last slot, carrying an offset), a middle element and tail are all freed"""
    freed = CR.position_set(freed)
    for b, slots in sorted(CR.lists_of(table, hp).items()):
        chain = [b * T.HASH_BUCKET_SIZE + T.HASH_BUCKET_SIZE - 1] + [int(s) for s in slots]
        if len(chain) < 3 or table["offset"][chain[0]] == 0 or table["ptr"][chain[0]] == T.FREE_ENTRY:
            continue
        is_freed = [tuple(int(v) for v in table["pos"][s]) in freed for s in chain]
        if is_freed[0] and is_freed[-1] and any(is_freed[1:-1]):
            return b
    return None


@pytest.mark.parametrize("name", ["A", "B"])
def test_crowded_tables(E, name):
    """Every frame of the sequence is taken out again, in the order they went in.  The frames before the last leave what
    the later ones saw; the last one finds voxels that weigh no more than its observations (the sequence starves), so
    it frees every block in its view, whole collision lists among them: chosen on the table before that call."""
    s = CR.SCENARIOS[name]
    cp = CR.config(name)[1]
    poses = CR.poses(name)
    frames = [frame_at(E, cp, p) for p in poses]
    results = {}
    for buckets in (s["buckets"], CR.ROOMY):
        hp = CR.config(name, buckets)[0]
        scene = E.CUDASceneRepHashSDF(hp, CR.options())
        for p, (f, _) in zip(poses, frames):
            scene.integrate(p, f, cp, None)
        if buckets != CR.ROOMY:
            assert canonical.check_chains(scene.download()["hash"], scene.getHashParams())["listed"] >= 3
        for k, (p, (f, maps)) in enumerate(zip(poses, frames)):
            label = f"{name}, {buckets} buckets, frame {k}"
            last = k == len(poses) - 1
            if last and buckets != CR.ROOMY:
                # asserted on the table before the call: the delete passes are exercised
                table = scene.download()["hash"]
                want = DI.deintegrate(SM.scene_of(scene.state()), maps, p, scene.getHashParams(), cp)
                assert list_head_middle_tail(table, scene.getHashParams(), want["freed"]) is not None, f"{label}: no list loses its head, a middle element and its tail"
                assert CR.list_involved(table, scene.getHashParams()).sum() >= 3
            got, want = deintegrate_checked(scene, f, maps, p, cp, label)
            assert got["status"] == 0
            if last and buckets != CR.ROOMY:
                assert got["delete_passes"] >= 3, "three deletes of one list take its bucket's mutex in three passes"
            results[(buckets, k)] = scene.state()
        assert scene.debugHash()["duplicates"] == 0 and scene.getState()[T.STATE_HEAP_UNDERFLOW] == 0
    for k in range(len(poses)):
        assert_is(results[(s["buckets"], k)], results[(CR.ROOMY, k)], f"{name}, frame {k}: crowded vs roomy")


# ------------------------------------------------------------------------------------------------ 8. the scene is a scene

def test_ray_cast_reallocation_and_reintegrate(E, oracle_lib, s1):
    hp, cp, rp = config()
    a, b = s1["A"], s1["B"]
    scene = new_scene(E, hp)
    scene.integrate(a["pose"], a["frame"], cp, None)
    scene.integrate(b["pose"], b["frame"], cp, None)
    with_b = CR.position_set(scene.state()["positions"])
    got = scene.deintegrate(b["pose"], b["frame"], cp)
    assert got["freed"] > 0
    without_b = CR.position_set(scene.state()["positions"])
    view = synth.orbit_pose(1, 40)
    scene.setLastRigidTransformAndCompactify(view, cp)
    d = scene.download()
    host = CR.host_copy(oracle_lib, d, scene.getHashParams(), cp, rp, options())
    ray = E.CUDARayCastSDF(rp)
    ray.render(scene.getHashData(), scene.getHashParams(), cp, view)
    assert_maps_equal(ray.download(), host.render(view), "ray cast after the de-integration")
    # the frame again: freed positions are allocated again, and the table is a table
    scene.integrate(b["pose"], b["frame"], cp, None)
    after = scene.state()
    assert (CR.position_set(after["positions"]) - without_b) & (with_b - without_b), "no freed position was allocated again"
    rep = scene.debugHash()
    assert rep["duplicates"] == 0 and rep["lockEntries"] == 0 and scene.getState()[T.STATE_HEAP_UNDERFLOW] == 0
    # reintegrate(old, new) is deintegrate(old) followed by integrate(new)
    new_pose = synth.orbit_pose(3, 40)
    one, two = new_scene(E, hp), new_scene(E, hp)
    for sc in (one, two):
        sc.integrate(a["pose"], a["frame"], cp, None)
        sc.integrate(b["pose"], b["frame"], cp, None)
    c1 = one.reintegrate(b["pose"], new_pose, b["frame"], cp)
    c2 = two.deintegrate(b["pose"], b["frame"], cp)
    two.integrate(new_pose, b["frame"], cp, None)
    assert {k: c1[k] for k in DI.COUNT_KEYS} == {k: c2[k] for k in DI.COUNT_KEYS}
    assert_is(one.state(), two.state(), "reintegrate")
    assert np.array_equal(one.getLastRigidTransform().reshape(16), np.asarray(new_pose, np.float32).reshape(16))


# ------------------------------------------------------------------------------------------------ 9. refusals, Reconstruction

def test_refusals_leave_the_table_alone(E, s1):
    hp, cp, _ = config()
    a = s1["A"]
    scene = new_scene(E, hp)
    scene.integrate(a["pose"], a["frame"], cp, None)
    before = scene.download()

    def refused(call):
        with pytest.raises(Exception) as err:
            call()
        assert getattr(err.value, "code", None) == 4, err.value  # VH_ERR_BAD_ARGUMENT
        assert raw_equal(before, scene.download()), "a refused de-integration changed the table"

    other_cp = T.make_depth_camera_params(32, 24)
    refused(lambda: scene.deintegrate(a["pose"], E.DepthFrame(other_cp), cp))
    refused(lambda: scene.reintegrate(a["pose"], a["pose"], E.DepthFrame(other_cp), cp))
    refused(lambda: scene.deintegrate(a["pose"], T.DepthCameraData(None, a["frame"].color_ptr), cp))
    refused(lambda: scene.deintegrate(a["pose"], T.DepthCameraData(a["frame"].depth_ptr, None), cp))
    refused(lambda: scene.reintegrate(a["pose"], a["pose"], T.DepthCameraData(None, None), cp))
    no_pixels = T.make_depth_camera_params(64, 48)
    no_pixels.m_imageWidth = 0
    refused(lambda: scene.deintegrate(a["pose"], a["frame"].data, no_pixels))
    # a frame in flight (integrateAhead without integrateFinish)
    busy = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=False, gc=True, starve=2))
    busy.integrateAhead(a["pose"], a["frame"], cp, None)
    for call in (lambda: busy.deintegrate(a["pose"], a["frame"], cp), lambda: busy.reintegrate(a["pose"], a["pose"], a["frame"], cp)):
        with pytest.raises(Exception) as err:
            call()
        assert err.value.code == 4
    busy.integrateFinish(a["frame"], cp)
    assert busy.deintegrate(a["pose"], a["frame"], cp)["status"] == 0
    # and the scene still takes the frame out
    deintegrate_checked(scene, a["frame"], a["maps"], a["pose"], cp, "after the refusals")


MF_W, MF_H, MF_N = 64, 48, 3
MF_PARAMS = """
s_sensorIdx = 8;
s_adapterWidth = 64;
s_adapterHeight = 48;
s_sensorDepthMax = 5.0f;
s_sensorDepthMin = 0.5f;
s_hashNumBuckets = 16384;
s_hashNumSDFBlocks = 8192;
s_hashMaxCollisionLinkedListSize = 7;
s_SDFVoxelSize = 0.02f;
s_SDFMarchingCubeThreshFactor = 10.0f;
s_SDFTruncation = 0.10f;
s_SDFTruncationScale = 0.05f;
s_SDFMaxIntegrationDistance = 4.0f;
s_SDFIntegrationWeightSample = 10;
s_SDFIntegrationWeightMax = 255;
s_SDFRayIncrementFactor = 0.8f;
s_SDFRayThresSampleDistFactor = 50.5f;
s_SDFRayThresDistFactor = 50.0f;
s_SDFUseGradients = false;
s_integrationEnabled = true;
s_trackingEnabled = true;
s_garbageCollectionEnabled = false;
s_garbageCollectionStarve = 15;
s_marchingCubesMaxNumTriangles = 400000;
s_offlineProcessing = true;
s_playData = true;
s_reconstructionEnabled = true;
s_binaryDumpSensorUseTrajectory = true;
"""
MF_STREAMING = """s_streamingEnabled = true;
s_streamingVoxelExtents = 0.5f 0.5f 0.5f;
s_streamingGridDimensions = 65 65 65;
s_streamingMinGridPos = -32 -32 -32;
s_streamingInitialChunkListSize = 16;
s_streamingRadius = 1.3f;
s_streamingPos = 0.0f 0.0f 1.8f;
s_streamingOutParts = 4;
"""


def test_reconstruction_takes_frames_out(E, oracle_lib, tmp_path):
    """Reconstruction's methods: a streaming scene with blocks on the host refuses; a scene without streaming takes its
    last frame out (what is left is the scene of the frames before it, within the rule) and puts it back elsewhere"""
    from voxelhashing_amd import reconstruction as R, sensor_data as SD
    cp = T.make_depth_camera_params(MF_W, MF_H)
    sd = SD.SensorData.create((MF_W, MF_H), (MF_W, MF_H), SD.make_intrinsic_matrix(cp.fx, cp.fy, cp.mx, cp.my), depth_shift=1000.0,
                              sensor_name="synthetic S3", depth_type=SD.TYPE_ZLIB_USHORT)
    raw = []
    for k in range(MF_N):
        p = synth.orbit_pose(k, n_frames=400)
        d, c = oracle_lib.synth_frame(synth.S3_SPHERES, 0, p, cp)
        mm = np.where(np.isfinite(d), np.floor(1000.0 * d.astype(np.float64) + 0.5), 0).astype(np.uint16)
        rgb = np.clip(np.where(np.isfinite(c[..., :3]), c[..., :3], 0) * 255.0, 0, 255).astype(np.uint8)
        sd.addFrame(rgb, mm, p, 100 + k, 200 + k)
    path = str(tmp_path / "s3.sens")
    sd.saveToFile(path)
    reader = SD.SensorDataReader(path)
    for k in range(MF_N):
        raw.append(reader.processDepth())
    reader.close()
    streaming = R.Reconstruction(R.read_app_state((MF_PARAMS + MF_STREAMING).encode()), sens_files=[path])
    assert streaming.run() == MF_N and streaming.chunk_grid.getStatistics()["blocks"] != 0
    pose = streaming.trajectory[-1]
    before = streaming.scene.download()
    for call in (lambda: streaming.deintegrateFrame(*raw[-1], pose), lambda: streaming.reintegrateFrame(*raw[-1], pose, pose)):
        with pytest.raises(ValueError):
            call()
    assert raw_equal(before, streaming.scene.download())
    plain = R.Reconstruction(R.read_app_state((MF_PARAMS + "s_streamingEnabled = false;\n").encode()), sens_files=[path])
    assert plain.run() == MF_N
    poses = [np.asarray(p, np.float32) for p in plain.trajectory]
    whole = SM.scene_of(plain.scene.state())
    frames_before = plain.scene.getNumIntegratedFrames()
    got = plain.deintegrateFrame(*raw[-1], poses[-1])
    maps = plain.frame_data.download()
    want = DI.deintegrate(whole, maps, poses[-1], plain.scene.getHashParams(), plain.cp)
    DI.assert_counts(got, want["counts"], "Reconstruction.deintegrateFrame")
    assert got["voxels_changed"] > 0 and got["voxels_at_cap"] == 0
    assert_is(plain.scene.state(), want, "Reconstruction.deintegrateFrame")
    assert plain.scene.getNumIntegratedFrames() == frames_before, "a de-integration is not a frame"
    # the frame back at its pose, then moved to another: reintegrateFrame against the two steps on a twin
    plain.scene.integrate(poses[-1], plain.frame_data, plain.cp, None)
    twin = R.Reconstruction(R.read_app_state((MF_PARAMS + "s_streamingEnabled = false;\n").encode()), sens_files=[path])
    assert twin.run() == MF_N
    twin.deintegrateFrame(*raw[-1], poses[-1])
    twin.scene.integrate(poses[-1], twin.frame_data, twin.cp, None)
    corrected = poses[-1].copy()
    corrected[:3, 3] += np.float32(0.01)
    got = plain.reintegrateFrame(*raw[-1], poses[-1], corrected)
    twin.deintegrateFrame(*raw[-1], poses[-1])
    twin.scene.integrate(corrected, twin.frame_data, twin.cp, None)
    assert got["voxels_changed"] > 0
    assert_is(plain.scene.state(), twin.scene.state(), "Reconstruction.reintegrateFrame")
    # a corrected trajectory: the second pass over the recording re-integrates the one frame whose pose differs
    params = (MF_PARAMS + "s_streamingEnabled = false;\n").encode()
    third, fourth = R.Reconstruction(R.read_app_state(params), sens_files=[path]), R.Reconstruction(R.read_app_state(params), sens_files=[path])
    assert third.run() == MF_N and fourth.run() == MF_N
    tally = third.reintegrateCorrected(np.stack(poses[:-1] + [corrected]))
    want = fourth.reintegrateFrame(*raw[-1], poses[-1], corrected)
    assert tally["frames"] == MF_N and tally["reintegrated"] == 1 and tally["voxels_changed"] == want["voxels_changed"] > 0
    assert_is(third.scene.state(), fourth.scene.state(), "Reconstruction.reintegrateCorrected")
    assert third.reintegrateCorrected(np.stack(poses[:-1] + [corrected]))["reintegrated"] == 0, "the corrected poses are the poses now"
    with pytest.raises(ValueError):
        streaming.reintegrateCorrected(np.stack(poses))
