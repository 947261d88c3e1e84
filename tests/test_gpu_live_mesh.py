"""The live mesh on the GPU ("Live mesh"; vh_live_mesh.hip).  After every update the cache's
(triangle || record) pairs are held, as a set, against a fresh extractIsoSurfaceIndexed on a second object, and every
count against the numpy restatement (tests/live_mesh.py) run on the downloaded table and voxel pool.

Scenes: S1 64x48 P2 and S2 80x60 P4, three orbit frames, built as build_scene of tests/test_gpu_mesh_weld.py builds
them (the helper is copied here, a frame at a time)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import live_mesh as LM
import mesh_weld as MW
from helpers import small_config
from voxelhashing_amd import synth, vhtypes as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = {"S1": (64, 48, "P2", "S1"), "S2": (80, 60, "P4", "S2")}
MAX_TRIANGLES = 1 << 19
BAD_ARGUMENT, STAGING_OVERFLOW = 4, 2


class Scene:
    """build_scene of tests/test_gpu_mesh_weld.py, a frame at a time"""

    def __init__(self, E, name, frames=3, options=None, orbit=100, first=0, **config):
        width, height, params, scene_name = SCENES[name]
        self.E = E
        self.hp, self.cp, _ = small_config(width, height, params=params, **config)
        self.spheres, self.inside, radius = synth.scene(scene_name)
        self.poses = [synth.orbit_pose(first + k, orbit, radius) for k in range(max(frames, 3))]
        self.scene = E.CUDASceneRepHashSDF(self.hp, options if options is not None else T.make_scene_options(offline=True, gc=False))
        self.frame = E.DepthFrame(self.cp)
        for k in range(frames):
            self.integrate(k)

    def integrate(self, k, pose=None):
        pose = self.poses[k] if pose is None else pose
        self.E.synth_frame(self.spheres, self.inside, pose, self.cp, out=self.frame)
        self.scene.integrate(pose, self.frame, self.cp, None)

    def tables(self):
        return self.scene.getHashData(), self.scene.getHashParams()


class Session:
    """a live mesh on `scene`, a second object for the fresh extraction, and the restatement's records beside them"""

    def __init__(self, E, scene, max_triangles=MAX_TRIANGLES):
        self.scene = scene
        self.mc = E.CUDAMarchingCubesHashSDF(T.make_marching_cubes_params(scene.hp, max_triangles))
        self.ref = E.CUDAMarchingCubesHashSDF(T.make_marching_cubes_params(scene.hp, MAX_TRIANGLES))
        self.mc.liveBegin()
        self.forget()

    def forget(self):
        self.records, self.epoch = LM.new_records(self.scene.hp.m_numSDFBlocks), 0
        self.sources = np.zeros(0, dtype=T.TRIANGLE_SOURCE_DTYPE)

    def fresh(self):
        hd, hp = self.scene.tables()
        self.ref.extractIsoSurfaceIndexed(hd, hp)
        return self.ref.triangles(), self.ref.sources()

    def plan(self):
        d = self.scene.scene.download()
        self.epoch += 1
        return LM.update(self.records, self.epoch, d["hash"], d["sdf_blocks"]), d

    def update(self):
        """one update, held against the restatement and the fresh extraction -> the plan, the counts, the downloaded tables"""
        hd, hp = self.scene.tables()
        plan, d = self.plan()
        drop = LM.dropped(self.sources, plan)
        got = self.mc.liveUpdate(hd, hp)
        tris, srcs = self.mc.triangles(), self.mc.sources()
        want_tris, want_srcs = self.fresh()
        kept = len(self.sources) - int(drop.sum())
        want = LM.counts(plan, len(self.sources), int(drop.sum()), len(want_tris) - kept)
        print({k: got[k] for k in LM.COUNTS}, "status", got["status"])
        assert got["status"] == 0 and got["code"] == 0 and {k: got[k] for k in LM.COUNTS} == want
        assert len(tris) == len(srcs) == got["total"] == len(want_tris)
        assert LM.pair_set(tris, srcs).tobytes() == LM.pair_set(want_tris, want_srcs).tobytes()
        self.sources = srcs
        return dict(plan=plan, counts=got, tables=d)


@pytest.fixture(scope="module")
def E(vh):
    from voxelhashing_amd import engine
    return engine


def poke(vh, base, offset, data):
    """vh_memcpy_h2d of a few bytes into a device buffer"""
    a = np.ascontiguousarray(data).view(np.uint8).ravel().copy()
    assert vh.vh_memcpy_h2d(C.c_void_p(int(base) + int(offset)), a.ctypes.data, a.nbytes, None) == 0


# ---------------------------------------------------------------------------- 1, 2. an update per frame; nothing changed

@pytest.mark.parametrize("name", ["S1", "S2"])
def test_update_after_every_frame_and_with_nothing_changed(E, name):
    x = Scene(E, name, frames=0)
    s = Session(E, x)
    first = s.update()["counts"]  # nothing resident: an empty cache, nothing launched over a list
    assert first["visited"] == first["total"] == first["remeshed"] == 0
    for k in range(3):
        x.integrate(k)
        c = s.update()["counts"]
        assert c["total"] > 100 and c["changed"] > 0
        if k == 0:
            assert c["changed"] == c["visited"] == c["remeshed"] and c["dropped"] == 0  # the first update is the full extraction
    before = (s.mc.triangles().tobytes(), s.mc.sources().tobytes())
    u = s.update()
    again = u["counts"]
    assert again["visited"] == len(LM.resident(u["tables"]["hash"])) > 0
    assert again["changed"] == again["vanished"] == again["remeshed"] == again["dropped"] == again["added"] == 0
    assert (s.mc.triangles().tobytes(), s.mc.sources().tobytes()) == before  # byte for byte, order included


# ---------------------------------------------------------------------------- 3. one voxel written into the pool

def test_one_voxel_written_through_memcpy(E, vh):
    x = Scene(E, "S1")
    s = Session(E, x)
    u = s.update()
    where, table, pool = u["plan"]["resident"], u["tables"]["hash"], u["tables"]["sdf_blocks"]

    def neighbours(p):
        return sum((p[0] + o[0], p[1] + o[1], p[2] + o[2]) in where for o in LM.OFFSETS)

    by_count = sorted(where, key=lambda p: (neighbours(p), p))
    blocks = [by_count[0]]  # a block with missing neighbours
    assert neighbours(blocks[0]) < 27
    if neighbours(by_count[-1]) == 27:  # and one with all 26, if the scene has one (a surface shell two blocks thick has few)
        blocks.append(by_count[-1])
    print("neighbour counts", [neighbours(p) for p in blocks])
    hd, _ = x.tables()
    for p in blocks:
        ptr = int(table["ptr"][where[p]])
        vox = pool[ptr:ptr + T.SDF_BLOCK_VOXELS].copy()
        i = int(np.argmax(vox["weight"]))  # an observed voxel if the block has one
        j = next(k for k in range(T.SDF_BLOCK_VOXELS) if vox[k].tobytes() != vox[i].tobytes())
        edits = []
        w = vox[i:i + 1].copy()
        w["weight"] += 1
        edits.append({i: w})  # its weight
        c = w.copy()
        c["color"][0, 2] ^= 0x10
        edits.append({i: c})  # only a colour byte
        edits.append({i: vox[j:j + 1].copy(), j: c})  # two unlike voxels of the block change places
        for edit in edits:
            for k, v in edit.items():
                poke(vh, hd.d_SDFBlocks, 8 * (ptr + k), v)
            got = s.update()["counts"]
            assert got["changed"] == 1 and got["vanished"] == 0
            assert got["remeshed"] == neighbours(p) < got["visited"]


# ---------------------------------------------------------------------------- 4, 5. blocks freed, ids reused

def small_sphere_region():
    return T.make_cut_region(tuple(synth.S1_SPHERES[1, :3]), (0.45, 0.45, 0.45), shape=T.CUT_ELLIPSOID)


def test_erase_region_frees_blocks(E):
    x = Scene(E, "S1")
    s = Session(E, x)
    before = s.update()["counts"]["visited"]
    x.scene.eraseRegion(small_sphere_region())
    got = s.update()["counts"]
    assert 0 < got["visited"] < before  # the ellipsoid frees at least one block and leaves at least one
    assert got["vanished"] > 0 and got["dropped"] > 0 and 0 < got["remeshed"] < got["visited"]


def test_freed_ids_come_back_at_other_positions(E):
    x = Scene(E, "S1")
    s = Session(E, x)
    u = s.update()
    t0 = u["tables"]["hash"]
    x.scene.eraseRegion(small_sphere_region())
    x.integrate(0, synth.orbit_pose(40, 100, synth.S1_ORBIT_RADIUS))  # another pose, no update in between
    u = s.update()
    t1 = u["tables"]["hash"]

    def by_id(t):
        r = LM.resident(t)
        return {int(t["ptr"][i]) // T.SDF_BLOCK_VOXELS: tuple(int(v) for v in t["pos"][i]) for i in r}

    a, b = by_id(t0), by_id(t1)
    moved = [i for i in a if i in b and a[i] != b[i]]
    print("ids at another position:", len(moved))
    assert moved, "no freed id came back at another position"
    assert u["counts"]["vanished"] >= len(moved)


# ---------------------------------------------------------------------------- 6. garbage collection

def test_update_per_frame_with_garbage_collection(E):
    """The frames of the golden s1_64x48_p1_gc set-up (1 cm voxels, GC every frame, the starve pass at frame 15), with
    an update per frame; the frames around the starve pass, where blocks are freed, are held against the restatement
    and the fresh extraction, the others update only.  No block that one update saw is gone at the next in this
    sequence -- what GC frees here was allocated by the same frame, and vanished is 0 in every update -- so the freed
    path is test_erase_region_frees_blocks' and test_freed_ids_come_back_at_other_positions'; what this one adds is the
    starve pass, which rewrites the weight byte of every observed voxel."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "s1_64x48_p1_gc.npz"))
    width, height, params = int(g["width"]), int(g["height"]), str(g["params"])
    hp = T.make_hash_params(int(g["num_buckets"]), int(g["num_sdf_blocks"]), **synth.PARAM_SETS[params])

    class Gc:
        pass

    x = Gc()
    x.hp, x.cp = hp, T.make_depth_camera_params(width, height)
    x.scene = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=True, gc=True, starve=int(g["starve"])))
    x.tables = lambda: (x.scene.getHashData(), x.scene.getHashParams())
    frame = E.DepthFrame(x.cp)
    s = Session(E, x)
    checked = (0, 1, int(g["starve"]) - 1, int(g["starve"]), int(g["starve"]) + 1, int(g["frames"]) - 1)
    vanished = 0
    for k in range(int(g["frames"])):
        pose = synth.orbit_pose(k, int(g["orbit"]))
        E.synth_frame(synth.S1_SPHERES, 0, pose, x.cp, out=frame)
        x.scene.integrate(pose, frame, x.cp, None)
        if k in checked:
            vanished += s.update()["counts"]["vanished"]
        else:  # the device's update alone; the restatement's records follow so that the next checked frame compares
            hd, hpp = x.tables()
            got = s.mc.liveUpdate(hd, hpp)
            assert got["status"] == 0
            s.plan()
            s.sources = s.mc.sources()
            vanished += got["vanished"]
    print("vanished over the sequence:", vanished)


# ---------------------------------------------------------------------------- 7. merge, de-integration

def test_merge_scene_and_deintegrate(E):
    x = Scene(E, "S1")
    s = Session(E, x)
    s.update()
    other = Scene(E, "S1", first=30)  # the same spheres seen from a third of the way round
    x.scene.mergeScene(other.scene)
    got = s.update()["counts"]
    assert got["changed"] > 0 and got["added"] > 0
    E.synth_frame(x.spheres, x.inside, x.poses[2], x.cp, out=x.frame)
    x.scene.deintegrate(x.poses[2], x.frame, x.cp)
    got = s.update()["counts"]
    assert got["changed"] > 0


# ---------------------------------------------------------------------------- 8. a crowded table

def test_crowded_table(E):
    x = Scene(E, "S1", frames=0, num_buckets=64, num_sdf_blocks=1 << 11)
    s = Session(E, x)
    for k in range(3):
        x.integrate(k)
        u = s.update()
    on_lists = LM.entries_on_lists(u["tables"]["hash"], 64)
    print("entries on collision lists:", len(on_lists), "of", u["counts"]["visited"])
    assert len(on_lists) > 0  # neighbours and owners are found through the lists
    x.scene.eraseRegion(small_sphere_region())
    assert s.update()["counts"]["vanished"] > 0


# ---------------------------------------------------------------------------- 9. overflow; the coordinate range

def test_overflow_invalidates_and_recovers(E):
    from voxelhashing_amd import lib
    x = Scene(E, "S1")
    probe = Session(E, x)
    n = probe.update()["counts"]["total"]
    s = Session(E, x, max_triangles=n - 100)
    hd, hp = x.tables()
    got = s.mc.liveUpdate(hd, hp, raise_on_status=False)
    assert got["status"] == T.LIVE_OVERFLOW and got["code"] == STAGING_OVERFLOW and got["total"] == n
    with pytest.raises(lib.VhError) as e:
        s.mc.liveIndexed()  # the cache is not valid
    assert e.value.code == BAD_ARGUMENT
    with pytest.raises(lib.VhError) as e:
        s.mc.liveUpdate(hd, hp)  # still too many: the same status again, as an exception
    assert e.value.code == STAGING_OVERFLOW
    x.scene.eraseRegion(small_sphere_region())  # now there is room
    got = s.update()["counts"]  # the next update starts from nothing: the device forgot every record
    assert got["changed"] == got["visited"] and got["dropped"] == 0 and got["total"] <= n - 100
    s.mc.liveEnd()
    s.mc.liveBegin()
    s.forget()
    got = s.update()["counts"]
    assert got["changed"] == got["visited"] and got["kept"] == 0


def test_block_out_of_range_is_refused(E, vh):
    """update refuses a resident block outside [-2^16, 2^16) (voxels outside the weld's key range) with
    VH_ERR_BAD_ARGUMENT; the cache is then invalid, and right again after the table is"""
    from voxelhashing_amd import lib
    x = Scene(E, "S1")
    s = Session(E, x)
    u = s.update()
    hd, hp = x.tables()
    idx = int(LM.resident(u["tables"]["hash"])[0])
    pos = u["tables"]["hash"]["pos"][idx].copy()
    poke(vh, hd.d_hash, 32 * idx, np.array([1 << 16, 0, 0], dtype=np.int32))
    got = s.mc.liveUpdate(hd, hp, raise_on_status=False)
    assert got["status"] == T.LIVE_RANGE and got["code"] == BAD_ARGUMENT
    with pytest.raises(lib.VhError):
        s.mc.liveIndexed()
    poke(vh, hd.d_hash, 32 * idx, pos)
    s.forget()
    got = s.update()["counts"]
    assert got["changed"] == got["visited"]


# ---------------------------------------------------------------------------- 10. the indexed mesh of the cache

@pytest.mark.parametrize("normals", [False, True])
def test_live_indexed_equals_the_indexed_extraction(E, normals):
    x = Scene(E, "S2", frames=2)
    s = Session(E, x)
    s.update()
    x.integrate(2)
    s.update()
    hd, hp = x.tables()
    for mc in (s.mc, s.ref):
        mc.setIndexedNormals(normals)
    s.mc.liveIndexed()
    s.ref.extractIsoSurfaceIndexed(hd, hp)
    got, want = s.mc.indexed(), s.ref.indexed()
    assert len(want["faces"]) > 100 and MW.same_mesh(MW.canonical(got), MW.canonical(want))
    if normals:
        a, b = np.argsort(got["keys"], kind="stable"), np.argsort(want["keys"], kind="stable")
        assert got["normals"][a].tobytes() == want["normals"][b].tobytes() and np.any(want["normals"] != 0)
    m = s.mc.mesh()
    assert m["vertices"].shape[0] == len(got["keys"]) and m["faces"].shape[0] == len(got["faces"])
    assert s.update()["counts"]["changed"] == 0  # the cache stays


# ---------------------------------------------------------------------------- 11. the digest alone; the launcher level

def test_digest_equals_the_restatement(E):
    x = Scene(E, "S1")
    d = x.scene.download()
    r = LM.resident(d["hash"])
    free = np.flatnonzero(d["hash"]["ptr"] == T.FREE_ENTRY)[:3]
    idx = np.concatenate([r, free, [len(d["hash"]) + 5]]).astype(np.uint32)
    hd, hp = x.tables()
    got = E.live_mesh_digest(hd, hp, idx)
    want = np.concatenate([LM.digests(d["sdf_blocks"], d["hash"]["ptr"][r]), np.zeros(4, dtype=np.uint64)])
    assert len(r) > 100 and np.array_equal(got, want)


def test_launcher_level_update(E):
    """vh_live_mesh_* over buffers of the caller's own: the same cache as the host class's"""
    x = Scene(E, "S1", frames=2)
    hd, hp = x.tables()
    live = E.LiveMesh(T.make_marching_cubes_params(x.hp, MAX_TRIANGLES), x.hp.m_numSDFBlocks)
    s = Session(E, x)
    for k in (None, 2):
        if k is not None:
            x.integrate(k)
        want = s.update()["counts"]
        got = live.update(hd, hp)
        assert {n: got[n] for n in LM.COUNTS} == {n: want[n] for n in LM.COUNTS} and got["status"] == 0
        assert LM.pair_set(*live.soup(got["total"])).tobytes() == LM.pair_set(s.mc.triangles(), s.mc.sources()).tobytes()
    rec = live.records()
    assert int((rec["epoch"] != 0).sum()) == want["visited"]
    live.reset()
    got = live.update(hd, hp)
    assert got["changed"] == got["visited"] and got["kept"] == 0 and got["total"] == want["total"]
    live.close()


# ---------------------------------------------------------------------------- 12. refusals

def test_refusals_leave_the_cache_as_it_was(E):
    from voxelhashing_amd import lib
    x = Scene(E, "S1")
    s = Session(E, x)
    s.update()
    hd, hp = x.tables()
    before = (s.mc.triangles().tobytes(), s.mc.sources().tobytes())

    def refused(call):
        with pytest.raises(lib.VhError) as e:
            call()
        assert e.value.code == BAD_ARGUMENT
        assert (s.mc.triangles().tobytes(), s.mc.sources().tobytes()) == before

    refused(lambda: s.mc.extractIsoSurface(hd, hp))  # an extraction while live
    refused(lambda: s.mc.extractIsoSurfaceWithoutCopy(hd, hp))
    refused(lambda: s.mc.extractIsoSurfaceIndexed(hd, hp))
    refused(lambda: s.mc.beginIndexed())
    refused(lambda: s.mc.liveBegin())
    refused(lambda: s.mc.liveUpdate(hd, hp, boxEnabled=True))  # a box
    for field, value in (("m_virtualVoxelSize", 0.03), ("m_hashNumBuckets", hp.m_hashNumBuckets // 2), ("m_numSDFBlocks", hp.m_numSDFBlocks // 2),
                         ("m_hashMaxCollisionLinkedListSize", 3)):
        other = type(hp).from_buffer_copy(hp)
        setattr(other, field, value)
        refused(lambda: s.mc.liveUpdate(hd, other))  # changed hash parameters
    idle = E.CUDAMarchingCubesHashSDF(T.make_marching_cubes_params(x.hp, MAX_TRIANGLES))
    for call in (lambda: idle.liveUpdate(hd, hp), idle.liveInvalidate, idle.liveIndexed, idle.liveEnd):  # without liveBegin
        with pytest.raises(lib.VhError) as e:
            call()
        assert e.value.code == BAD_ARGUMENT
    got = s.update()["counts"]  # and the records are as they were: nothing has changed
    assert got["changed"] == got["remeshed"] == 0
    s.mc.liveInvalidate()
    s.forget()
    got = s.update()["counts"]
    assert got["changed"] == got["visited"]
    s.mc.liveEnd()
    s.mc.extractIsoSurfaceIndexed(hd, hp)  # after liveEnd the object extracts again
    assert s.mc.indexed_counts()["faces"] > 100


# ---------------------------------------------------------------------------- 13, 14. Reconstruction, the replay tool

RW, RH, RN = 80, 60, 3
PARAMS = """
s_sensorIdx = 8;
s_adapterWidth = 80;
s_adapterHeight = 60;
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
STREAMING = """s_streamingEnabled = true;
s_streamingVoxelExtents = 0.5f 0.5f 0.5f;
s_streamingGridDimensions = 65 65 65;
s_streamingMinGridPos = -32 -32 -32;
s_streamingInitialChunkListSize = 16;
s_streamingRadius = 1.3f;
s_streamingPos = 0.0f 0.0f 1.8f;
s_streamingOutParts = 4;
"""


@pytest.fixture(scope="module")
def sens_file(vh, oracle_lib, tmp_path_factory):
    from voxelhashing_amd import sensor_data as SD
    cp = T.make_depth_camera_params(RW, RH)
    sd = SD.SensorData.create((RW, RH), (RW, RH), SD.make_intrinsic_matrix(cp.fx, cp.fy, cp.mx, cp.my), depth_shift=1000.0,
                              sensor_name="synthetic S3", depth_type=SD.TYPE_ZLIB_USHORT)
    for k in range(RN):
        p = synth.orbit_pose(k, n_frames=400)
        d, c = oracle_lib.synth_frame(synth.S3_SPHERES, 0, p, cp)
        mm = np.where(np.isfinite(d), np.floor(1000.0 * d.astype(np.float64) + 0.5), 0).astype(np.uint16)
        rgb = np.clip(np.where(np.isfinite(c[..., :3]), c[..., :3], 0) * 255.0, 0, 255).astype(np.uint8)
        sd.addFrame(rgb, mm, p, 100 + k, 200 + k)
    path = str(tmp_path_factory.mktemp("live") / "s3.sens")
    sd.saveToFile(path)
    return path


def test_reconstruction_keeps_a_live_mesh(sens_file):
    from voxelhashing_amd import reconstruction as R
    rec = R.Reconstruction(R.read_app_state((PARAMS + "s_streamingEnabled = false;\n").encode()), sens_files=[sens_file])
    with pytest.raises(ValueError):
        rec.liveMeshUpdate()  # no liveMeshBegin
    rec.liveMeshBegin()
    updates = []
    while rec.frame() is not None:
        updates.append(rec.liveMeshUpdate())
    assert len(updates) == RN and all(u["status"] == 0 and u["changed"] > 0 for u in updates)
    assert updates[0]["changed"] == updates[0]["visited"] and updates[-1]["dropped"] > 0  # (neighbouring frames: each touches nearly every block)
    # a frame in flight: refused, the cache as it was
    rec.scene.integrateAhead(rec.frame_poses[-1], rec.frame_data, rec.cp)
    before = (rec.live_marching_cubes.triangles().tobytes(), rec.live_marching_cubes.sources().tobytes())
    with pytest.raises(ValueError):
        rec.liveMeshUpdate()
    assert (rec.live_marching_cubes.triangles().tobytes(), rec.live_marching_cubes.sources().tobytes()) == before
    rec.scene.integrateFinish(rec.frame_data, rec.cp)
    again = rec.liveMeshUpdate()  # the frame went in a second time: the model changed, and the update follows it
    assert again["status"] == 0 and again["changed"] > 0
    mesh = rec.liveMesh()
    live = rec.live_marching_cubes.indexed()
    plain = rec.extractIsoSurface(indexed=True)
    want = rec.marching_cubes.indexed()
    assert len(plain["faces"]) == len(mesh["faces"]) > 500 and MW.same_mesh(MW.canonical(live), MW.canonical(want))
    # with streaming a live mesh is refused before any GPU work
    streamed = R.Reconstruction(R.read_app_state((PARAMS + STREAMING).encode()), sens_files=[sens_file])
    for call in (streamed.liveMeshBegin, streamed.liveMeshUpdate):
        with pytest.raises(ValueError):
            call()
    assert streamed.live_marching_cubes is None


def read_ply_sets(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    nv = int(re.search(rb"element vertex (\d+)", head).group(1))
    nf = int(re.search(rb"element face (\d+)", head).group(1))
    assert len(body) == nv * 16 + nf * 13
    verts = [body[16 * i:16 * i + 16] for i in range(nv)]
    faces = np.frombuffer(body[nv * 16:], dtype=np.dtype([("n", "u1"), ("i", "<i4", 3)]))["i"]
    out = set()
    for f in faces:  # a face as its three vertex records, the smallest first: independent of the vertex order
        t = [verts[i] for i in f]
        r = t.index(min(t))
        out.add(tuple(t[r:] + t[:r]))
    return set(verts), out


def test_replay_tool_writes_the_same_mesh_from_the_live_cache(sens_file, tmp_path):
    """tools/replay.py --live-mesh-every 1 on the sample parameters of the indexed-mesh tests (PARAMS above): the PLY's
    vertex and face sets are those of the run without it"""
    params = str(tmp_path / "params.txt")
    open(params, "w").write(PARAMS + "s_streamingEnabled = false;\n")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "replay.py"), "--params", params, "--sens", sens_file, "--indexed-mesh"]
    plain = json.loads(subprocess.check_output(cmd + ["--mesh", str(tmp_path / "plain.ply")], timeout=600).decode().strip().splitlines()[-1])
    live = json.loads(subprocess.check_output(cmd + ["--mesh", str(tmp_path / "live.ply"), "--live-mesh-every", "1"], timeout=600).decode().strip().splitlines()[-1])
    assert live["frames"] == plain["frames"] == RN and "live_mesh" not in plain
    ups = live["live_mesh"]["updates"]
    assert [u["frame"] for u in ups] == [1, 2, 3, 3] and all(u["status"] == 0 for u in ups) and ups[-1]["changed"] == 0
    assert live["mesh"]["vertices"] == plain["mesh"]["vertices"] > 100 and live["mesh"]["faces"] == plain["mesh"]["faces"] > 100
    assert read_ply_sets(str(tmp_path / "live.ply")) == read_ply_sets(str(tmp_path / "plain.ply"))
