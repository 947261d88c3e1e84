"""The accumulating weld on the GPU ("Indexed mesh over several extractions"): vh_mesh_weld_accum_*
on hand-made and random parts against the numpy restatement (tests/mesh_weld_appends.py) bit for bit, growth of the
table and the arrays, the fixed table, the key range; then the host path: two overlapping boxes, the walk of the chunk
grid against the direct indexed extraction, an overflow inside the walk, and Reconstruction.extractIsoSurfaceIndexed
with streaming."""
import re

import numpy as np
import pytest

import mesh_weld as MW
import mesh_weld_appends as MA
from helpers import small_config
from voxelhashing_amd import synth, vhtypes as T

pytestmark = pytest.mark.gpu

STAGING_OVERFLOW, BAD_ARGUMENT = 2, 4  # VH_ERR_*


def assert_same_mesh(got, want, what=""):
    for k in ("keys", "vertices", "colors", "faces"):
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), f"{what}: {k}"


# ---------------------------------------------------------------------------- 1. launcher, hand-made

@pytest.mark.parametrize("name", ["shared_edge", "snapped_meet", "snapped_meet_reversed", "repeated_cell"])
def test_appends_hand_made_cases(vh, name):
    from voxelhashing_amd import engine as E
    parts = MA.split_cases()[name]
    want = MA.weld_appends(parts)
    got = E.mesh_weld_appends(parts)
    assert got["status"] == 0 and got["code"] == 0 and got["counts"] == (len(want["keys"]), len(want["faces"]))
    m = MW.canonical(got)
    assert_same_mesh(m, want, name)
    assert got["stats"]["dropped"] == MA.dropped(parts) and got["stats"]["cells"] == MA.num_cells(parts)
    if name == "shared_edge":
        # numbered by the first append, overwritten by the second: the bits of cell (0, 0, 0)
        i = int(np.searchsorted(m["keys"], np.uint64(MW.pack_key((0, 0, 1), 0, 0))))
        assert m["vertices"][i].tobytes() == parts[1][0]["v"]["p"][0, 0].tobytes()
        assert m["colors"][i].tobytes() == parts[1][0]["v"]["c"][0, 0].tobytes()
    if name == "repeated_cell":
        gone = np.array([MW.pack_key((2, 2, 2), e, 0) for e in (4, 5, 6)], dtype=np.uint64)
        assert got["stats"]["dropped"] == 1 and not np.isin(gone, got["keys"]).any()


def test_appends_of_nothing(vh):
    from voxelhashing_amd import engine as E
    empty = (np.zeros(0, dtype=T.TRIANGLE_DTYPE), np.zeros(0, dtype=T.TRIANGLE_SOURCE_DTYPE))
    got = E.mesh_weld_appends([])
    assert got["counts"] == (0, 0) and got["status"] == 0 and set(got["stats"].values()) == {0}
    soup, srcs = MW.random_soup(21, 4)
    got = E.mesh_weld_appends([empty, (soup, srcs), empty])  # n = 0 launches nothing and changes nothing
    assert_same_mesh(MW.canonical(got), MW.weld(soup, srcs), "empty appends around one")


# ---------------------------------------------------------------------------- 2. launcher, random

@pytest.fixture(scope="module")
def random_parts():
    """random_soup(2000, seed, spread=3) by cell into 5 appends, about a third of the cells repeated whole in a later
    append; the restatement's results, computed once"""
    soup, srcs = MW.random_soup(2000, 11, spread=3)
    parts = MA.deal(soup, srcs, 5, 11)
    other = MA.deal(soup, srcs, 5, 11, identical=False)
    return dict(soup=soup, srcs=srcs, parts=parts, other=other, whole=MW.weld(soup, srcs), want=MA.weld_appends(parts),
                want_other=MA.weld_appends(other), dropped=MA.dropped(parts), cells=MA.num_cells(parts))


def test_appends_random_soup(vh, random_parts):
    from voxelhashing_amd import engine as E
    r = random_parts
    assert r["dropped"] > 300 and r["dropped"] == sum(len(s) for s, _ in r["parts"]) - 2000
    got = E.mesh_weld_appends(r["parts"])
    assert got["status"] == 0 and got["counts"] == (len(r["want"]["keys"]), len(r["want"]["faces"]))
    assert_same_mesh(MW.canonical(got), r["want"], "against weld_appends")
    assert_same_mesh(MW.canonical(got), r["whole"], "against the weld of the whole soup")  # the repeats are identical copies
    assert got["stats"]["dropped"] == r["dropped"] and got["stats"]["cells"] == r["cells"]
    # repeats with other bits: the first append that has a cell gives it its triangles
    got = E.mesh_weld_appends(r["other"])
    assert_same_mesh(MW.canonical(got), r["want_other"], "repeats with other bits")
    assert_same_mesh(MW.canonical(got), r["whole"], "repeats with other bits against the whole")
    assert got["stats"]["dropped"] == r["dropped"]


@pytest.mark.parametrize("order", [(4, 3, 2, 1, 0), (2, 0, 4, 1, 3)])
def test_appends_in_any_order_give_the_same_mesh(vh, random_parts, order):
    from voxelhashing_amd import engine as E
    parts = [random_parts["parts"][i] for i in order]
    got = E.mesh_weld_appends(parts)
    assert_same_mesh(MW.canonical(got), random_parts["want"], f"order {order}")
    assert got["stats"]["dropped"] == random_parts["dropped"] == MA.dropped(parts)


@pytest.mark.parametrize("sizes", [(63, 1), (64, 65), (257, 22, 256)])
def test_appends_around_a_wave_and_a_workgroup(vh, sizes):
    """consecutive slices of one random soup: cells repeat between them with other triangles, which are dropped"""
    from voxelhashing_amd import engine as E
    soup, srcs = MW.random_soup(sum(sizes), 20 + len(sizes))
    cuts = np.cumsum((0,) + sizes)
    parts = [(soup[a:b], srcs[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    want = MA.weld_appends(parts)
    got = E.mesh_weld_appends(parts)
    assert_same_mesh(MW.canonical(got), want, str(sizes))
    assert got["stats"]["dropped"] == MA.dropped(parts) and (MA.dropped(parts) > 0 or sum(sizes) < 100)


# ---------------------------------------------------------------------------- 3. growth

def test_table_and_arrays_grow(vh, random_parts):
    from voxelhashing_amd import engine as E
    roomy = E.mesh_weld_appends(random_parts["parts"], slots_log2=16, reserve_triangles=4096)
    assert roomy["stats"]["rehashes"] == 0
    tight = E.mesh_weld_appends(random_parts["parts"], slots_log2=6, reserve_triangles=0)
    print("rehashes", tight["stats"]["rehashes"])
    assert tight["stats"]["rehashes"] >= 3 and tight["status"] == 0
    assert_same_mesh(MW.canonical(tight), MW.canonical(roomy), "tight against roomy")
    assert_same_mesh(MW.canonical(tight), random_parts["want"], "tight against the restatement")
    assert {k: v for k, v in tight["stats"].items() if k != "rehashes"} == {k: v for k, v in roomy["stats"].items() if k != "rehashes"}


# ---------------------------------------------------------------------------- 4. fixed table

def test_fixed_table_fills_up_and_says_so(vh, random_parts):
    from voxelhashing_amd import engine as E, lib
    full = E.mesh_weld_appends(random_parts["parts"], slots_log2=6, fixed=True, raise_on_status=False)
    assert full["status"] == T.WELD_TABLE_FULL and full["code"] == STAGING_OVERFLOW and full["counts"] == (0, 0)
    assert len(full["keys"]) == 0 and len(full["faces"]) == 0 and full["stats"]["rehashes"] == 0
    assert full["stats"]["cells"] == 0 and full["stats"]["dropped"] == 0
    with pytest.raises(lib.VhError) as e:
        E.mesh_weld_appends(random_parts["parts"], slots_log2=6, fixed=True)
    assert e.value.code == STAGING_OVERFLOW
    # a fixed table that is large enough is a table like any other
    ok = E.mesh_weld_appends(random_parts["parts"], slots_log2=13, fixed=True)
    assert ok["stats"]["rehashes"] == 0
    assert_same_mesh(MW.canonical(ok), random_parts["want"], "fixed, 2^13 slots")


# ---------------------------------------------------------------------------- 5. key range

@pytest.mark.parametrize("cell", [((1 << 19) - 1, 0, 0), (0, 1 << 19, 0), (0, 0, -(1 << 19) - 1)])
def test_appends_refuse_a_cell_outside_the_key_range(vh, cell):
    from voxelhashing_amd import engine as E, lib
    soup, srcs = MW.random_soup(44, 6)
    # edges 1, 5, 9 lie on the cell's x = 1 face: at 2^19 - 1 their lattice points are one past the range, the cell's
    # own coordinates are not
    srcs["cell"][35] = cell
    srcs["edges"][35] = MW.source_record(cell, [(1, 0), (5, 0), (9, 0)])["edges"][0]
    parts = [(soup[:22], srcs[:22]), (soup[22:], srcs[22:])]  # the first append is fine
    out = E.mesh_weld_appends(parts, raise_on_status=False)
    assert out["status"] == T.WELD_KEY_RANGE and out["code"] == BAD_ARGUMENT and out["counts"] == (0, 0) and len(out["keys"]) == 0
    with pytest.raises(lib.VhError) as e:
        E.mesh_weld_appends(parts)
    assert e.value.code == BAD_ARGUMENT
    with pytest.raises(MW.KeyRange):
        MA.weld_appends(parts)


# ---------------------------------------------------------------------------- 6. two boxes

def read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    nv = int(re.search(rb"element vertex (\d+)", head).group(1))
    nf = int(re.search(rb"element face (\d+)", head).group(1))
    assert len(body) == nv * 16 + nf * 13
    verts = np.frombuffer(body[:nv * 16], dtype=np.dtype([("p", "<f4", 3), ("c", "u1", 4)]))
    faces = np.frombuffer(body[nv * 16:], dtype=np.dtype([("n", "u1"), ("i", "<i4", 3)]))
    assert np.all(faces["n"] == 3)
    return verts, faces["i"]


def gpu_scene(E, hp, cp, poses, spheres):
    scene = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=True, gc=False))
    frame = E.DepthFrame(cp)
    for pose in poses:
        E.synth_frame(spheres, 0, pose, cp, out=frame)
        scene.integrate(pose, frame, cp, None)
    return scene


def test_two_overlapping_boxes_give_the_direct_mesh(vh):
    from voxelhashing_amd import engine as E
    hp, cp, _ = small_config(64, 48, params="P2")
    poses = [synth.orbit_pose(k, 100) for k in range(2)]
    scene = gpu_scene(E, hp, cp, poses, synth.S1_SPHERES)
    hd, hpp = scene.getHashData(), scene.getHashParams()
    mc = E.CUDAMarchingCubesHashSDF(T.make_marching_cubes_params(hp, 1 << 19))
    mc.extractIsoSurfaceIndexed(hd, hpp)
    direct, soup = MW.canonical(mc.indexed()), mc.triangles()
    assert len(direct["faces"]) > 500 and set(mc.indexed_stats().values()) == {0}
    # split along x at the median, one block of overlap
    cx, half = float(np.median(soup["v"]["p"][..., 0])), 0.5 * hp.m_virtualVoxelSize * T.SDF_BLOCK_SIZE
    boxes = [((-10.0, -10.0, -10.0), (cx + half, 10.0, 10.0)), ((cx - half, -10.0, -10.0), (10.0, 10.0, 10.0))]
    for order in (boxes, boxes[::-1]):
        mc.beginIndexed()
        for lo, hi in order:
            mc.appendIndexed(hd, hpp, lo, hi, True)
            assert 0 < mc.counts()["triangles"] < len(soup)
        mc.finishIndexed()
        got = mc.indexed()
        assert_same_mesh(MW.canonical(got), direct, "two boxes")
        stats = mc.indexed_stats()
        print(stats)
        assert stats["dropped"] > 0 and stats["status"] == 0
        assert stats["vertices"] == len(direct["keys"]) and stats["faces"] == len(direct["faces"])
        assert mc.indexed_counts() == dict(vertices=stats["vertices"], faces=stats["faces"], status=0)
        m = mc.mesh()
        assert m["vertices"].tobytes() == got["vertices"].tobytes() and np.array_equal(m["faces"], got["faces"])
    # a one-shot extraction afterwards is served by the one-shot weld again
    mc.extractIsoSurfaceIndexed(hd, hpp)
    assert_same_mesh(MW.canonical(mc.indexed()), direct, "one-shot after accumulated")
    assert set(mc.indexed_stats().values()) == {0}


# ---------------------------------------------------------------------------- 7. / 8. the chunk grid

SMALL_BUFFER = 200  # triangles: fewer than the fullest chunk's


@pytest.fixture(scope="module")
def chunk_walk(vh):
    """The scene of test_gpu_chunkwise_extraction_covers_the_direct_one (tests/test_marching_cubes.py): 96x72, three S1
    orbit frames, 1 m chunks, a 9^3 grid from -4, radius 100.  On the CPU the oracle gives 4005 triangles for it and,
    box by box over this grid, 18 chunks with triangles and 18858 triangles in all: more than one chunk appends and
    cells repeat, so the chunk extent stays at 1 m.  The indexed walk, then a walk that overflows in a chunk."""
    from voxelhashing_amd import engine as E, lib
    hp, cp, _ = small_config(96, 72, streaming_extents=(1.0, 1.0, 1.0), streaming_dims=(9, 9, 9), streaming_min=(-4, -4, -4))
    poses = [synth.orbit_pose(k, n_frames=100) for k in range(3)]
    scene = gpu_scene(E, hp, cp, poses, synth.S1_SPHERES)
    mp = T.make_marching_cubes_params(hp, 1 << 19)
    direct = E.CUDAMarchingCubesHashSDF(mp)
    direct.extractIsoSurfaceIndexed(scene.getHashData(), scene.getHashParams())
    out = dict(direct=MW.canonical(direct.indexed()), direct_triangles=direct.counts()["triangles"], before=scene.state())
    grid = E.CUDASceneRepChunkGrid(scene, (1.0, 1.0, 1.0), (9, 9, 9), (-4, -4, -4), 64, True, 4)
    try:
        mc = E.CUDAMarchingCubesHashSDF(mp)
        mc.extractIsoSurfaceIndexedChunkGrid(grid, (0.0, 0.0, 0.0), 100.0)
        out.update(mc=mc, indexed=mc.indexed(), stats=mc.indexed_stats(), counts=mc.indexed_counts(), mesh=mc.mesh(), after=scene.state())
        small = E.CUDAMarchingCubesHashSDF(T.make_marching_cubes_params(hp, SMALL_BUFFER))
        try:
            small.extractIsoSurfaceIndexedChunkGrid(grid, (0.0, 0.0, 0.0), 100.0)
            out["overflow_code"] = 0
        except lib.VhError as e:
            out["overflow_code"] = e.code
        out.update(small_mesh=small.mesh(), small_counts=small.indexed_counts(), small_stats=small.indexed_stats(),
                   small_indexed=small.indexed(), after_overflow=scene.state())
        # and the grid still walks: the soup walk of the parent on the same grid
        again = E.CUDAMarchingCubesHashSDF(mp)
        again.extractIsoSurfaceChunkGrid(grid, (0.0, 0.0, 0.0), 100.0)
        out.update(soup_vertices=again.mesh()["vertices"], after_again=scene.state())
    finally:
        grid.close()
    return out


def test_chunk_grid_walk_gives_the_direct_indexed_mesh(chunk_walk, tmp_path):
    from voxelhashing_amd import canonical
    x = chunk_walk
    assert x["direct_triangles"] == 4005 and len(x["direct"]["faces"]) > 1000
    assert_same_mesh(MW.canonical(x["indexed"]), x["direct"], "chunk grid against direct")
    s = x["stats"]
    print(s)
    # (at least two chunks appended: the kept triangles are the direct extraction's, the dropped ones come on top, and
    # no box but the whole scene's holds them all; the oracle's count of the boxes is in the fixture's docstring)
    assert s["dropped"] > 0 and s["status"] == 0 and s["cells"] > 0
    assert s["dropped"] <= 18858 - 4005  # (the walk skips a chunk without blocks of its own, the oracle's count did not)
    assert x["counts"] == dict(vertices=len(x["direct"]["keys"]), faces=len(x["direct"]["faces"]), status=0)
    m, ind = x["mesh"], x["indexed"]
    assert m["vertices"].tobytes() == ind["vertices"].tobytes() and m["colors"][:, :3].tobytes() == ind["colors"].tobytes()
    assert np.all(m["colors"][:, 3] == 1.0) and np.array_equal(m["faces"], ind["faces"])
    path = str(tmp_path / "streamed.ply")
    x["mc"].saveMesh(path, None, True)
    verts, faces = read_ply(path)
    assert len(verts) == len(ind["keys"]) and verts["p"].tobytes() == ind["vertices"].tobytes()
    assert np.array_equal(faces.astype(np.uint32), ind["faces"])
    assert x["mc"].mesh()["vertices"].shape[0] == 0  # saveMesh clears the buffer
    canonical.assert_same_scene(x["before"], x["after"], "scene after the indexed chunk-wise extraction")
    # the soup the parent's walk downloads over the same boxes: the kept triangles and the dropped ones
    assert len(x["soup_vertices"]) == 3 * (4005 + s["dropped"]) and len(ind["keys"]) < len(x["soup_vertices"]) // 10


def test_overflow_in_a_chunk_leaves_nothing_behind(chunk_walk):
    from voxelhashing_amd import canonical
    x = chunk_walk
    assert x["overflow_code"] == STAGING_OVERFLOW
    assert x["small_mesh"]["vertices"].shape[0] == 0 and x["small_mesh"]["faces"].shape[0] == 0
    assert x["small_counts"] == dict(vertices=0, faces=0, status=0) and set(x["small_stats"].values()) == {0}
    assert len(x["small_indexed"]["keys"]) == 0 and len(x["small_indexed"]["faces"]) == 0
    canonical.assert_same_scene(x["before"], x["after_overflow"], "scene after the walk that overflowed")
    canonical.assert_same_scene(x["before"], x["after_again"], "scene after the walk that followed it")


# ---------------------------------------------------------------------------- 9. Reconstruction

RW, RH, RN = 80, 60, 3
# PARAMS and STREAMING of test_reconstruction_extracts_an_indexed_mesh (tests/test_gpu_mesh_weld.py)
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


def test_reconstruction_extracts_an_indexed_mesh_with_streaming(vh, oracle_lib, tmp_path):
    from voxelhashing_amd import reconstruction as R, sensor_data as SD
    cp = T.make_depth_camera_params(RW, RH)
    sd = SD.SensorData.create((RW, RH), (RW, RH), SD.make_intrinsic_matrix(cp.fx, cp.fy, cp.mx, cp.my), depth_shift=1000.0,
                              sensor_name="synthetic S3", depth_type=SD.TYPE_ZLIB_USHORT)
    for k in range(RN):
        p = synth.orbit_pose(k, n_frames=400)
        d, c = oracle_lib.synth_frame(synth.S3_SPHERES, 0, p, cp)
        mm = np.where(np.isfinite(d), np.floor(1000.0 * d.astype(np.float64) + 0.5), 0).astype(np.uint16)
        rgb = np.clip(np.where(np.isfinite(c[..., :3]), c[..., :3], 0) * 255.0, 0, 255).astype(np.uint8)
        sd.addFrame(rgb, mm, p, 100 + k, 200 + k)
    path = str(tmp_path / "s3.sens")
    sd.saveToFile(path)

    rec = R.Reconstruction(R.read_app_state((PARAMS + STREAMING).encode()), sens_files=[path])
    assert rec.run() == RN and rec.chunk_grid is not None
    mesh = rec.extractIsoSurfaceIndexed()
    ind = rec.marching_cubes.indexed()
    stats = rec.marching_cubes.indexed_stats()
    print(stats)
    assert len(ind["faces"]) > 500 and stats["dropped"] > 0 and stats["status"] == 0
    assert mesh["vertices"].tobytes() == ind["vertices"].tobytes() and np.array_equal(mesh["faces"], ind["faces"])
    assert mesh["colors"][:, :3].tobytes() == ind["colors"].tobytes()
    m = MW.canonical(ind)
    f = m["faces"].astype(np.int64)
    assert not ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).any()
    assert len(np.unique(np.sort(f, axis=1), axis=0)) == len(f)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    assert np.unique(e, axis=0, return_counts=True)[1].max() <= 2
    # The soup of the same object.  PARAMS has s_offlineProcessing on, with which the soup walk merges every chunk's
    # batch on the host before it appends it, and what comes back is no soup; for this comparison the extractor appends
    # the chunks' triangles as they are.
    rec.marching_cubes.setOfflineProcessing(False)
    soup = rec.extractIsoSurface()
    assert soup["faces"].shape[0] == 0 and len(soup["vertices"]) % 3 == 0  # three vertices per triangle, no indices
    row = np.dtype((np.void, 12))
    soup_rows = np.unique(np.ascontiguousarray(soup["vertices"]).view(row).ravel())
    assert np.isin(np.ascontiguousarray(ind["vertices"]).view(row).ravel(), soup_rows).all()
    tri = np.dtype((np.void, 36))
    unique_triangles = len(np.unique(np.ascontiguousarray(soup["vertices"]).reshape(-1, 9).view(tri).ravel()))
    assert unique_triangles < len(soup["vertices"]) // 3  # the chunks' boxes overlap
    assert len(ind["faces"]) <= unique_triangles
    # written as a PLY, the file is the indexed mesh
    ply = str(tmp_path / "streamed.ply")
    again = rec.extractIsoSurfaceIndexed(ply)
    verts, faces = read_ply(ply)
    assert len(verts) == len(again["vertices"]) and len(faces) == len(again["faces"]) == len(ind["faces"])
    assert_same_mesh(MW.canonical(rec.marching_cubes.indexed()), m, "a second streamed extraction")

    # without streaming the new method is extractIsoSurface(indexed=True)
    plain = R.Reconstruction(R.read_app_state((PARAMS + "s_streamingEnabled = false;\n").encode()), sens_files=[path])
    assert plain.run() == RN
    a = plain.extractIsoSurfaceIndexed()
    via_new = MW.canonical(plain.marching_cubes.indexed())
    b = plain.extractIsoSurface(indexed=True)
    via_old = MW.canonical(plain.marching_cubes.indexed())
    assert_same_mesh(via_new, via_old, "non-streamed")
    assert len(a["vertices"]) == len(b["vertices"]) == len(via_old["keys"]) and len(a["faces"]) == len(b["faces"]) > 500
    assert set(plain.marching_cubes.indexed_stats().values()) == {0}
