"""Scene merge on the device (vh_merge.hip) against the numpy restatement of its definition (tests/scene_merge.py), which
takes combineVoxel from the oracle: every pair of weights, the two halves of the crowded-table sequences A and B
(tests/crowded.py) on roomy and crowded tables, merge into empty and commutativity, the block offset, the list source
and Reconstruction.mergeFrom, the heap-short refusal, a table too small for the union, a ray cast of the merged scene,
and the refusals.  Every downloaded state goes through state(), which checks the invariants and follows every list."""

import numpy as np
import pytest

import crowded as CR
import scene_merge as SM
from helpers import assert_maps_equal, small_config
from voxelhashing_amd import canonical, synth, vhtypes as T

pytestmark = pytest.mark.gpu
V = T.SDF_BLOCK_VOXELS
COUNT_KEYS = ("source_blocks", "present", "allocated", "left_out", "combined", "copied", "alloc_passes", "status")


@pytest.fixture(scope="module")
def E(vh):
    from voxelhashing_amd import engine
    return engine


def split(name):
    n = CR.SCENARIOS[name]["frames"]
    return range(0, n // 2), range(n // 2, n)


@pytest.fixture(scope="module")
def ref(oracle_lib):
    """The oracle's two half scenes of A and B, each from an empty roomy table, and the restatement's merge of the
    second into the first.  Computed once; the tests only read it."""
    O = oracle_lib
    out = {}
    for name in CR.SCENARIOS:
        hp, cp, rp = CR.config(name, CR.ROOMY)
        frames = CR.frames(O, name)
        halves = []
        for part in split(name):
            o = O.OracleScene(hp, cp, rp, CR.options())
            for k in part:
                o.integrate(*frames[k])
            halves.append(o.state())
        merged = SM.merge(SM.scene_of(halves[0]), SM.scene_of(halves[1]), hp)
        out[name] = dict(halves=halves, merged=merged, union=CR.union(halves[0]["positions"], halves[1]["positions"]))
    return out


def build_half(E, name, which, buckets=None):
    """half `which` of the sequence through CUDASceneRepHashSDF from an empty table"""
    hp, cp, rp = CR.config(name, buckets)
    scene = E.CUDASceneRepHashSDF(hp, CR.options())
    frame = E.DepthFrame(cp)
    poses = CR.poses(name)
    for k in split(name)[which]:
        E.synth_frame(synth.S1_SPHERES, 0, poses[k], cp, out=frame)
        scene.integrate(poses[k], frame, cp, None)
    return scene


def same(a, b, what):
    canonical.assert_same_scene(a, b, what, bucket_counts=False)
    assert a["voxels"].tobytes() == b["voxels"].tobytes(), f"{what}: voxel bytes differ"


def assert_is(snap, want, what):
    """a device snapshot holds the restatement's scene"""
    assert np.array_equal(snap["positions"], want["positions"]), f"{what}: block position sets differ"
    assert snap["voxels"].tobytes() == want["voxels"].tobytes(), f"{what}: voxel bytes differ"


def check_counts(got, want, what):
    SM.assert_counts(got, want["counts"], what)
    assert got["left_out"] == 0 and got["present"] + got["allocated"] == got["source_blocks"], (what, got)


# ------------------------------------------------------------------------------------------------ 1. every weight pair

def weight_pair_blocks(seed, truncation):
    """128 blocks at the same positions for both sides: voxel v of the 65 536 has destination weight v >> 8 and source
    weight v & 255; seeded sdfs within +- the truncation with 0, -0 and values at the float's small end among them,
    seeded colours (also on the unobserved voxels, whose bytes the merge must leave alone)"""
    rng = np.random.default_rng(seed)
    n = 128
    pos = np.stack([np.arange(n) % 8 - 4, (np.arange(n) // 8) % 4 - 2, np.arange(n) // 32 - 2], axis=-1).astype(np.int32)
    v = np.arange(n * V).reshape(n, V)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754944e-38, -1.1754944e-38, 1e-30, truncation, -truncation], np.float32)
    sides = []
    for weights in (v >> 8, v & 255):
        vox = np.zeros((n, V), T.VOXEL_DTYPE)
        sdf = rng.uniform(-truncation, truncation, (n, V)).astype(np.float32)
        pick = rng.random((n, V)) < 0.05
        sdf[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
        vox["sdf"], vox["weight"] = sdf, weights.astype(np.uint8)
        vox["color"] = rng.integers(0, 256, (n, V, 3), dtype=np.uint8)
        sides.append(vox)
    return pos, sides[0], sides[1]


@pytest.mark.parametrize("colour_mode", [T.COLOR_RUNNING_AVERAGE, T.COLOR_WEIGHTED_AVERAGE])
@pytest.mark.parametrize("cap", [255, 20])
def test_every_weight_pair(E, oracle_lib, cap, colour_mode):
    """all (w_d, w_s) in [0, 255]^2 with the cap at 255 and at 20, which most sums exceed, under both colour rules:
    voxels and counts bit for bit"""
    hp, _, _ = small_config(64, 48, "P4", num_sdf_blocks=256)
    hp.m_integrationWeightMax, hp.m_colorIntegration = cap, colour_mode
    pos, d_vox, s_vox = weight_pair_blocks(17, np.float32(hp.m_truncation))
    descs = np.zeros(len(pos), T.DESC_DTYPE)
    descs["pos"] = pos
    g = E.LauncherScene(hp)
    g.stream_in(descs, d_vox, 1)
    before = g.state()
    assert_is(before, dict(zip(("positions", "voxels"), SM.sort_scene(pos, d_vox))), "the destination as streamed in")
    want = SM.merge((pos, d_vox), (pos, s_vox), hp)
    got = g.merge_blocks(descs, s_vox, 2)
    print({k: got[k] for k in COUNT_KEYS})
    check_counts(got, want, f"cap {cap} colour mode {colour_mode}")
    assert got["present"] == 128 and got["combined"] == 255 * 255 and got["copied"] == 255
    after = g.state()
    assert_is(after, want, f"cap {cap} colour mode {colour_mode}")
    assert after["heap_free"] == before["heap_free"]


# ------------------------------------------------------------------------------------------------ 2. two halves of a sequence

@pytest.fixture(scope="module")
def merged_a(E, ref):
    """what test 2 leaves for test 8: the merged scene of A on its crowded table"""
    return {}


@pytest.mark.parametrize("name", ["A", "B"])
def test_two_halves_on_roomy_and_crowded_tables(E, ref, name, merged_a):
    r, s = ref[name], CR.SCENARIOS[name]
    hp = CR.config(name)[0]
    # what makes the outcome the same on every schedule, on the union the merge asks the table for
    pre = CR.assert_precondition_a if name == "A" else CR.assert_precondition_b
    over, fullest = pre(r["union"], s["buckets"], s["limit"])
    assert over >= 3 and fullest > T.HASH_BUCKET_SIZE
    assert len(r["union"]) < CR.POOL
    states = {}
    for buckets in (CR.ROOMY, s["buckets"]):
        what = f"{name} on {buckets} buckets"
        dst, src = build_half(E, name, 0, buckets), build_half(E, name, 1, buckets)
        same(dst.state(), r["halves"][0], what + ": first half vs oracle")
        src_before = src.state()
        same(src_before, r["halves"][1], what + ": second half vs oracle")
        got = dst.mergeScene(src)
        print(what, {k: got[k] for k in COUNT_KEYS})
        check_counts(got, r["merged"], what)
        st = dst.state()
        assert_is(st, r["merged"], what + ": merged vs restatement")
        assert st["heap_free"] == hp.m_numSDFBlocks - len(r["union"])
        assert dst.getState()[T.STATE_HEAP_UNDERFLOW] == 0
        same(src.state(), src_before, what + ": the source afterwards")
        assert dst.debugHash()["duplicates"] == 0
        states[buckets] = st
        if buckets != CR.ROOMY:
            chains = canonical.check_chains(dst.download(False)["hash"], dst.getHashParams())
            assert chains["listed"] >= 3, f"{what}: the table was meant to hold collision lists: {chains}"
            if name == "A":
                merged_a["scene"] = dst
    same(states[s["buckets"]], states[CR.ROOMY], f"{name}: crowded vs roomy")


# ------------------------------------------------------------------------------------------------ 3. empty, commutativity

def test_merge_into_empty_and_commutativity(E, ref):
    r = ref["A"]
    hp = CR.config("A", CR.ROOMY)[0]
    src = build_half(E, "A", 1, CR.ROOMY)
    empty = E.CUDASceneRepHashSDF(hp, CR.options())
    got = empty.mergeScene(src)
    n = len(r["halves"][1]["positions"])
    assert (got["present"], got["allocated"], got["left_out"], got["combined"], got["status"]) == (0, n, 0, 0, 0)
    assert got["copied"] == int((r["halves"][1]["voxels"]["weight"] > 0).sum())
    same(empty.state(), src.state(), "merge into a freshly reset scene vs the source")
    # D <- S and S <- D
    d1, s1 = build_half(E, "A", 0, CR.ROOMY), build_half(E, "A", 1, CR.ROOMY)
    d1.mergeScene(s1)
    d2, s2 = build_half(E, "A", 0, CR.ROOMY), build_half(E, "A", 1, CR.ROOMY)
    s2.mergeScene(d2)
    same(d1.state(), s2.state(), "D <- S vs S <- D")


# ------------------------------------------------------------------------------------------------ 4. block offset

def test_block_offset(E, ref):
    r = ref["B"]
    hp = CR.config("B", CR.ROOMY)[0]
    off = (1, -2, 3)
    want = SM.merge(SM.scene_of(r["halves"][0]), SM.scene_of(r["halves"][1]), hp, off)
    assert 0 < want["counts"]["present"] < r["merged"]["counts"]["present"], "the shift was meant to change which blocks are shared"
    dst, src = build_half(E, "B", 0, CR.ROOMY), build_half(E, "B", 1, CR.ROOMY)
    got = dst.mergeScene(src, off)
    check_counts(got, want, "offset (1, -2, 3)")
    assert_is(dst.state(), want, "offset (1, -2, 3)")
    zero, plain = build_half(E, "B", 0, CR.ROOMY), build_half(E, "B", 0, CR.ROOMY)
    zero.mergeScene(src, (0, 0, 0))
    plain.mergeScene(src)
    same(zero.state(), plain.state(), "offset (0, 0, 0) vs the plain call")
    assert_is(zero.state(), r["merged"], "offset (0, 0, 0)")


# ------------------------------------------------------------------------------------------------ 5. list source

def test_list_source_equals_scene_source(E, ref):
    r = ref["B"]
    src = build_half(E, "B", 1, CR.ROOMY)
    snap = src.state()
    descs = np.zeros(len(snap["positions"]), T.DESC_DTYPE)
    descs["pos"], descs["ptr"] = snap["positions"], -7  # (the ptr of a list's desc is not read)
    by_list, by_scene = build_half(E, "B", 0, CR.ROOMY), build_half(E, "B", 0, CR.ROOMY)
    a = by_list.mergeBlocks(descs, snap["voxels"])
    b = by_scene.mergeScene(src)
    assert a["left_out_indices"] is not None and len(a["left_out_indices"]) == 0
    for k in ("source_blocks", "present", "allocated", "left_out", "combined", "copied", "status"):
        assert a[k] == b[k], (k, a, b)
    same(by_list.state(), by_scene.state(), "list source vs scene source")
    assert_is(by_list.state(), r["merged"], "list source")


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


def test_merge_from_a_streaming_reconstruction(E, oracle_lib, tmp_path):
    """Reconstruction.mergeFrom: the source streams, part of its model sits in the host grid; merged into an empty
    reconstruction, the destination holds the source's device blocks and its host blocks, bit for bit"""
    from voxelhashing_amd import reconstruction as R, sensor_data as SD
    cp = T.make_depth_camera_params(MF_W, MF_H)
    sd = SD.SensorData.create((MF_W, MF_H), (MF_W, MF_H), SD.make_intrinsic_matrix(cp.fx, cp.fy, cp.mx, cp.my), depth_shift=1000.0,
                              sensor_name="synthetic S3", depth_type=SD.TYPE_ZLIB_USHORT)
    for k in range(MF_N):
        p = synth.orbit_pose(k, n_frames=400)
        d, c = oracle_lib.synth_frame(synth.S3_SPHERES, 0, p, cp)
        mm = np.where(np.isfinite(d), np.floor(1000.0 * d.astype(np.float64) + 0.5), 0).astype(np.uint16)
        rgb = np.clip(np.where(np.isfinite(c[..., :3]), c[..., :3], 0) * 255.0, 0, 255).astype(np.uint8)
        sd.addFrame(rgb, mm, p, 100 + k, 200 + k)
    path = str(tmp_path / "s3.sens")
    sd.saveToFile(path)
    src = R.Reconstruction(R.read_app_state((MF_PARAMS + MF_STREAMING).encode()), sens_files=[path])
    assert src.run() == MF_N
    on_gpu, (h_descs, h_blocks) = src.scene.state(), src.chunk_grid.downloadHostBlocks()
    assert on_gpu["num_occupied"] > 20 and len(h_descs) > 20, "the source was meant to hold blocks on the device and on the host"
    want = SM.sort_scene(np.concatenate([on_gpu["positions"], h_descs["pos"]]), np.concatenate([on_gpu["voxels"], h_blocks]))
    dst = R.Reconstruction(R.read_app_state((MF_PARAMS + "s_streamingEnabled = false;\n").encode()), sens_files=[path])
    out = dst.mergeFrom(src)
    assert len(out) == 2 and out[0]["allocated"] == on_gpu["num_occupied"] and out[1]["allocated"] == len(h_descs)
    assert all(o["status"] == 0 and o["present"] == 0 and o["left_out"] == 0 for o in out)
    assert_is(dst.scene.state(), dict(positions=want[0], voxels=want[1]), "mergeFrom")
    # a destination whose own grid holds blocks on the host refuses
    with pytest.raises(ValueError):
        src.mergeFrom(dst)


# ------------------------------------------------------------------------------------------------ 6. heap short

def list_of(snap):
    descs = np.zeros(len(snap["positions"]), T.DESC_DTYPE)
    descs["pos"] = snap["positions"]
    return descs, snap["voxels"]


def raw_equal(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a if k != "params")


def test_heap_short_changes_nothing(E, ref):
    r = ref["B"]
    missing = r["merged"]["counts"]["allocated"]
    held = len(r["halves"][0]["positions"])
    assert missing > 1
    hp = CR.config("B", CR.ROOMY)[0]
    hp.m_numSDFBlocks = held + missing - 1  # one block short
    # launcher level: the status word
    g = E.LauncherScene(hp)
    g.stream_in(*list_of(r["halves"][0]), 1)
    before = g.download()
    got = g.merge_blocks(*list_of(r["halves"][1]), 2)
    print({k: got[k] for k in COUNT_KEYS})
    assert got["status"] == T.MERGE_HEAP_SHORT
    assert (got["source_blocks"], got["present"], got["allocated"], got["left_out"], got["combined"], got["copied"], got["alloc_passes"]) == \
        (len(r["halves"][1]["positions"]), r["merged"]["counts"]["present"], 0, 0, 0, 0, 0)
    assert raw_equal(before, g.download()), "a refused merge changed the destination"
    g.state()
    # scene level: the return code, and one more free block is enough
    for pool, fits in ((held + missing - 1, False), (held + missing, True)):
        hp.m_numSDFBlocks = pool
        scene = E.CUDASceneRepHashSDF(hp, CR.options())
        first = scene.mergeBlocks(*list_of(r["halves"][0]))
        assert first["allocated"] == held and first["status"] == 0
        before = scene.download()
        if fits:
            check_counts(scene.mergeBlocks(*list_of(r["halves"][1])), r["merged"], "a pool that just fits")
            st = scene.state()
            assert_is(st, r["merged"], "a pool that just fits")
            assert st["heap_free"] == 0
        else:
            with pytest.raises(Exception) as err:
                scene.mergeBlocks(*list_of(r["halves"][1]))
            assert err.value.code == 1 and err.value.counts["status"] == T.MERGE_HEAP_SHORT, err.value  # VH_ERR_HEAP_EXHAUSTED
            assert raw_equal(before, scene.download()), "a refused merge changed the destination"
            assert scene.getState()[T.STATE_HEAP_UNDERFLOW] == 0


# ------------------------------------------------------------------------------------------------ 7. no slot

NO_SLOT_ROOMY = (2, 7, 12, 17, 21)  # buckets of the destination that hold 8 blocks; every other bucket holds its 10


def positions_by_bucket(buckets, per_bucket, seed):
    """{bucket: per_bucket distinct positions whose home it is}"""
    rng = np.random.default_rng(seed)
    cand = np.unique(rng.integers(-200, 200, (40 * buckets * per_bucket, 3)).astype(np.int32), axis=0)
    cand = cand[rng.permutation(len(cand))]
    home = canonical.hash_buckets(cand, buckets)
    out = {b: cand[home == b][:per_bucket] for b in range(buckets)}
    assert all(len(v) == per_bucket for v in out.values())
    return out


def seeded_blocks(n, seed, most_weight=30):
    rng = np.random.default_rng(seed)
    vox = np.zeros((n, V), T.VOXEL_DTYPE)
    vox["sdf"] = rng.uniform(-0.1, 0.1, (n, V)).astype(np.float32)
    vox["color"] = rng.integers(0, 256, (n, V, 3), dtype=np.uint8)
    vox["weight"] = rng.integers(1, most_weight + 1, (n, V)).astype(np.uint8)
    vox[rng.random((n, V)) < 0.4] = np.zeros((), T.VOXEL_DTYPE)
    return vox


def test_no_slot_leaves_blocks_out_whole(E):
    """A table too small for the union: 23 buckets with the default list limit of 7.  The destination fills every
    bucket's ten slots, but for five buckets that are not neighbours and hold eight.  allocBlock then answers `no room`
    by its limits, never by the heap, and no list ever forms (a list longer than the walk would hide entries: the
    precondition of tests/crowded.py).  The source names 40 of the destination's blocks and, as new positions:
      - four in each bucket of eight: two find a slot, two do not -- which two depends on the schedule;
      - three in the full bucket in front of each: its own slots and the seven it may probe behind it are taken;
      - one in every other full bucket: no room.
    Asserted is what every schedule gives."""
    hp = CR.config("B")[0]
    hp.m_hashMaxCollisionLinkedListSize = 7
    nb = hp.m_hashNumBuckets
    assert nb == 23 and all((b + 1) % nb not in NO_SLOT_ROOMY for b in NO_SLOT_ROOMY)
    by = positions_by_bucket(nb, 14, 3)
    d_pos = np.concatenate([by[b][:8 if b in NO_SLOT_ROOMY else 10] for b in range(nb)])
    d_vox = seeded_blocks(len(d_pos), 4)
    g = E.LauncherScene(hp)
    d_descs = np.zeros(len(d_pos), T.DESC_DTYPE)
    d_descs["pos"] = d_pos
    first = g.merge_blocks(d_descs, d_vox, 1)
    assert (first["allocated"], first["left_out"], first["status"]) == (len(d_pos), 0, 0), first
    before = g.state()
    assert canonical.check_chains(before["raw"]["hash"], hp)["listed"] == 0
    had = CR.voxels_by_position(before)

    rng = np.random.default_rng(6)
    shared = d_pos[rng.permutation(len(d_pos))[:40]]
    new, fits = [], 0
    for b in range(nb):
        if b in NO_SLOT_ROOMY:
            new.append(by[b][10:14])
            fits += 2
        elif (b + 1) % nb in NO_SLOT_ROOMY:
            new.append(by[b][10:13])
        else:
            new.append(by[b][10:11])
    new = np.concatenate(new)
    pos = np.concatenate([shared, new])
    pos = pos[rng.permutation(len(pos))]
    n = len(pos)
    vox = seeded_blocks(n, 8)
    assert len(np.unique(pos, axis=0)) == n
    assert len(had) + len(new) < hp.m_numSDFBlocks, "alloc was meant to run out by its list limit, not by the heap"
    assert len(CR.union(d_pos, pos)) > nb * T.HASH_BUCKET_SIZE, "the union was meant to outnumber the table's slots"
    descs = np.zeros(n, T.DESC_DTYPE)
    descs["pos"] = pos
    got = g.merge_blocks(descs, vox, 2)
    print({k: got[k] for k in COUNT_KEYS})
    after = g.state()  # (the invariants hold)
    now = CR.voxels_by_position(after)
    assert got["present"] + got["allocated"] + got["left_out"] == n
    assert (got["present"], got["allocated"], got["left_out"]) == (40, fits, len(new) - fits)
    assert got["status"] == T.MERGE_NO_SLOT
    left = got["left_out_indices"]
    assert len(left) == got["left_out"] == len(np.unique(left))
    src_pos = [tuple(int(v) for v in p) for p in pos]
    left_pos = {src_pos[i] for i in left}
    for p in left_pos:
        assert p not in now and p not in had, f"the left-out block {p} has an entry"
    merged = {p: k for k, p in enumerate(src_pos) if p not in left_pos}
    assert set(now) == set(had) | set(merged)
    for p, bytes_now in now.items():
        if p not in merged:
            assert bytes_now == had[p], f"block {p}, which no merged source block names, changed"
        else:
            d = np.frombuffer(had[p], T.VOXEL_DTYPE) if p in had else np.zeros(V, T.VOXEL_DTYPE)
            want, _, _ = SM.merge_voxels(hp, d, vox[merged[p]])
            assert bytes_now == want.tobytes(), f"block {p}: merged voxels differ from the rule"
    assert after["heap_free"] == hp.m_numSDFBlocks - after["num_occupied"]
    assert after["raw"]["state"][T.STATE_HEAP_UNDERFLOW] == 0


# ------------------------------------------------------------------------------------------------ 8. the merged scene is a scene

def test_the_merged_scene_ray_casts(E, oracle_lib, ref, merged_a):
    """A's merged scene on its crowded table, compactified and ray cast from one of the scenario's poses, against the
    oracle's ray cast on a host copy of the table the device built"""
    r = ref["A"]
    hp, cp, rp = CR.config("A")
    scene = merged_a.get("scene")
    if scene is None:  # (run on its own)
        scene, src = build_half(E, "A", 0), build_half(E, "A", 1)
        scene.mergeScene(src)
    assert_is(scene.state(), r["merged"], "the scene to render")
    pose = CR.poses("A")[1]
    scene.setLastRigidTransformAndCompactify(pose, cp)
    assert scene.getNumOccupiedBlocks() > 100
    d = scene.download()
    host = CR.host_copy(oracle_lib, d, scene.getHashParams(), cp, rp, CR.options())
    want = host.render(pose)
    ray = E.CUDARayCastSDF(rp)
    ray.render(scene.getHashData(), scene.getHashParams(), cp, pose)
    got = ray.download()
    assert_maps_equal(got, want, "ray cast of the merged scene")
    W, H = cp.m_imageWidth, cp.m_imageHeight
    assert int((got["depth"] != -np.inf).sum()) > 0.3 * W * H, "the maps were meant to show the model"


# ------------------------------------------------------------------------------------------------ 9. refusals

def test_refusals_leave_the_destination_alone(E, ref):
    r = ref["B"]
    hp, cp, _ = CR.config("B", CR.ROOMY)
    dst, src = build_half(E, "B", 0, CR.ROOMY), build_half(E, "B", 1, CR.ROOMY)
    before = dst.download()

    def refused(call, code=4):  # VH_ERR_BAD_ARGUMENT
        with pytest.raises(Exception) as err:
            call()
        assert getattr(err.value, "code", None) == code, err.value
        assert raw_equal(before, dst.download()), "a refused merge changed the destination"

    other_hp = CR.config("B", CR.ROOMY)[0]
    other_hp.m_virtualVoxelSize = np.float32(0.05)
    refused(lambda: dst.mergeScene(E.CUDASceneRepHashSDF(other_hp, CR.options())))
    refused(lambda: dst.mergeScene(dst))
    # repeated positions: refused by the Python mirror before anything is uploaded
    descs, vox = list_of(r["halves"][1])
    descs[1]["pos"] = descs[0]["pos"]
    with pytest.raises(ValueError):
        dst.mergeBlocks(descs, vox)
    assert raw_equal(before, dst.download())
    # a frame in flight (integrateAhead without integrateFinish), in the destination and in the source
    online = T.make_scene_options(offline=False, gc=True, starve=2)
    busy = E.CUDASceneRepHashSDF(hp, online)
    frame = E.DepthFrame(cp)
    pose = CR.poses("B")[0]
    E.synth_frame(synth.S1_SPHERES, 0, pose, cp, out=frame)
    busy.integrateAhead(pose, frame, cp, None)
    refused(lambda: dst.mergeScene(busy))
    with pytest.raises(Exception) as err:
        busy.mergeScene(src)
    assert err.value.code == 4
    with pytest.raises(Exception) as err:
        busy.mergeBlocks(*list_of(r["halves"][1]))
    assert err.value.code == 4
    busy.integrateFinish(frame, cp)
    # and the scene still merges
    check_counts(dst.mergeScene(src), r["merged"], "after the refusals")
    assert_is(dst.state(), r["merged"], "after the refusals")
