"""The indexed mesh on the GPU ("Indexed mesh"): the sourced pass 2 (same triangles as the plain
pass, records that name the lattice edge of every vertex), the weld (vh_mesh.hip) against the numpy restatement
(tests/mesh_weld.py) bit for bit, the properties of the welded mesh, vh_mesh_weld on hand-made input, the host path
(mesh buffer, saveMesh, errors) and Reconstruction.extractIsoSurface(indexed=True).

Scenes: S1 64x48 P2 and S2 80x60 P4 (the one with snapped vertices), three orbit frames, as gpu_scene of
tests/test_marching_cubes.py."""
import re

import numpy as np
import pytest

import mesh_weld as MW
from helpers import small_config
from voxelhashing_amd import synth, vhtypes as T

pytestmark = pytest.mark.gpu

SCENES = {"S1": (64, 48, "P2", "S1"), "S2": (80, 60, "P4", "S2")}
MAX_TRIANGLES = 1 << 19


def sorted_triangles(tris):
    v = np.ascontiguousarray(tris).view(np.dtype((np.void, T.TRIANGLE_DTYPE.itemsize))).ravel()
    return np.ascontiguousarray(tris)[np.argsort(v, kind="stable")]


def same_triangle_set(a, b):
    a, b = sorted_triangles(a), sorted_triangles(b)
    return len(a) == len(b) and a.tobytes() == b.tobytes()


def build_scene(E, name):
    width, height, params, scene_name = SCENES[name]
    hp, cp, _ = small_config(width, height, params=params)
    spheres, inside, radius = synth.scene(scene_name)
    poses = [synth.orbit_pose(k, 100, radius) for k in range(3)]
    scene = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=True, gc=False))
    frame = E.DepthFrame(cp)
    for pose in poses:
        E.synth_frame(spheres, inside, pose, cp, out=frame)
        scene.integrate(pose, frame, cp, None)
    return scene, hp, cp, poses, spheres, inside


@pytest.fixture(scope="module")
def extractions(vh):
    """name -> what the plain and the indexed extraction gave on that scene, with and without the box; made once"""
    from voxelhashing_amd import engine as E
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        scene, hp, cp, poses, spheres, inside = build_scene(E, name)
        hd, hpp = scene.getHashData(), scene.getHashParams()
        mc = E.CUDAMarchingCubesHashSDF(T.make_marching_cubes_params(hp, MAX_TRIANGLES))
        mc.extractIsoSurfaceWithoutCopy(hd, hpp)
        plain = mc.triangles()
        cx = float(np.median(plain["v"]["p"][..., 0]))  # the box of tests/test_marching_cubes.py
        box = ((cx, -10.0, -10.0), (10.0, 10.0, 10.0))
        mc.extractIsoSurfaceWithoutCopy(hd, hpp, box[0], box[1], True)
        plain_box = mc.triangles()
        mc.extractIsoSurfaceIndexed(hd, hpp, box[0], box[1], True)
        boxed = dict(triangles=mc.triangles(), sources=mc.sources(), indexed=mc.indexed(), plain=plain_box)
        mc.extractIsoSurfaceIndexed(hd, hpp)
        full = dict(triangles=mc.triangles(), sources=mc.sources(), indexed=mc.indexed(), plain=plain, mesh=mc.mesh(),
                    counts=mc.indexed_counts())
        cache[name] = dict(scene=scene, hp=hp, cp=cp, poses=poses, spheres=spheres, inside=inside, mc=mc, full=full, boxed=boxed, box=box)
        return cache[name]

    return get


# ---------------------------------------------------------------------------- 1. the sourced pass 2

@pytest.mark.parametrize("name", ["S1", "S2"])
def test_sourced_pass_writes_the_same_triangles_and_names_their_edges(extractions, oracle_lib, name):
    x = extractions(name)
    O = oracle_lib
    o = O.OracleScene(x["hp"], x["cp"], None, T.make_scene_options(offline=True, gc=False))
    for pose in x["poses"]:
        depth, color = O.synth_frame(x["spheres"], x["inside"], pose, x["cp"])
        o.integrate(pose, depth, color)
    mp = T.make_marching_cubes_params(x["hp"], MAX_TRIANGLES)
    want, n = o.extract_iso_surface(mp)
    assert n > 200 and len(x["full"]["triangles"]) == n == len(x["full"]["sources"])
    assert same_triangle_set(x["full"]["triangles"], x["full"]["plain"]) and same_triangle_set(x["full"]["triangles"], want)
    mp.m_boxEnabled = 1
    mp.m_minCorner[:] = x["box"][0]
    mp.m_maxCorner[:] = x["box"][1]
    want_b, nb = o.extract_iso_surface(mp)
    assert 0 < nb < n and same_triangle_set(x["boxed"]["triangles"], x["boxed"]["plain"]) and same_triangle_set(x["boxed"]["triangles"], want_b)

    for part in (x["full"], x["boxed"]):
        snap = MW.assert_sources_name_their_edges(part["triangles"], part["sources"], x["hp"].m_virtualVoxelSize)
        if name == "S2" and part is x["full"]:
            assert (snap != 0).sum() > 0  # the scene that is here for its snapped vertices


# ---------------------------------------------------------------------------- 2. the weld against the restatement

@pytest.mark.parametrize("name", ["S1", "S2"])
@pytest.mark.parametrize("part", ["full", "boxed"])
def test_weld_equals_the_restatement(extractions, name, part):
    x = extractions(name)[part]
    want = MW.weld(x["triangles"], x["sources"])
    got = MW.canonical(x["indexed"])
    assert len(want["keys"]) > 100 and len(want["faces"]) > 100
    for k in ("keys", "vertices", "colors", "faces"):
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k


# ---------------------------------------------------------------------------- 3. the mesh

@pytest.mark.parametrize("name", ["S1", "S2"])
def test_welded_mesh_properties(extractions, name):
    x = extractions(name)["full"]
    n = len(x["triangles"])
    got = MW.canonical(x["indexed"])
    props = MW.properties(got, x["triangles"], x["sources"])
    V, F = len(got["keys"]), len(got["faces"])
    print(name, dict(triangles=n, vertices=V, faces=F, reduction=round(3 * n / V, 2), **props))
    assert props["repeated"] == 0
    assert props["faces_per_edge"] == 2
    assert props["duplicates"] == 0
    assert 3 * n / V >= 4
    assert props["spread"] < 1e-4  # the threshold of the host merge this replaces
    assert x["counts"] == dict(vertices=V, faces=F, status=0)


# ---------------------------------------------------------------------------- 4. vh_mesh_weld on hand-made input

@pytest.mark.parametrize("name", ["shared_edge", "snapped_meet", "snap_disagreement", "collapsing_face"])
def test_mesh_weld_hand_made_cases(vh, name):
    from voxelhashing_amd import engine as E
    soup, srcs, nv, nf = MW.hand_made_cases()[name]
    got = E.mesh_weld(soup, srcs)
    assert got["counts"] == (nv, nf) and got["status"] == 0
    assert MW.same_mesh(MW.canonical(got), MW.weld(soup, srcs))


@pytest.mark.parametrize("n", [0, 1, 21, 22, 257])
def test_mesh_weld_sizes_around_a_wave_and_a_workgroup(vh, n):
    """3 n lanes insert: 63 and 66 straddle a wave, 257 triangles a workgroup of the face pass"""
    from voxelhashing_amd import engine as E
    soup, srcs = MW.random_soup(n, 10 + n)
    got = E.mesh_weld(soup, srcs)
    want = MW.weld(soup, srcs)
    assert got["counts"] == (len(want["keys"]), len(want["faces"])) and got["status"] == 0
    assert MW.same_mesh(MW.canonical(got), want)
    if n == 0:
        assert got["counts"] == (0, 0)
    if n == 257:
        assert want["dropped_faces"] > 0 and len(want["keys"]) < 3 * n  # the random soup shares keys and collapses faces


def test_mesh_weld_crowded_and_full_tables(vh):
    from voxelhashing_amd import engine as E, lib
    soup, srcs = MW.random_soup(160, 5, isolated=True)
    want = MW.weld(soup, srcs)
    assert len(want["keys"]) == 480
    got = E.mesh_weld(soup, srcs, slots_log2=9)  # 480 keys in 512 slots: load 0.94
    assert got["slots_log2"] == 9 and MW.same_mesh(MW.canonical(got), want)
    # one power of two too small: the probe gives up after as many steps as there are slots
    full = E.mesh_weld(soup, srcs, slots_log2=8, raise_on_status=False)
    assert full["code"] == 2 and full["status"] == T.WELD_TABLE_FULL and full["counts"] == (0, 0)  # VH_ERR_STAGING_OVERFLOW
    assert len(full["keys"]) == 0 and len(full["faces"]) == 0
    with pytest.raises(lib.VhError) as e:
        E.mesh_weld(soup, srcs, slots_log2=8)
    assert e.value.code == 2


def test_mesh_weld_refuses_a_cell_outside_the_key_range(vh):
    from voxelhashing_amd import engine as E, lib
    soup, srcs = MW.random_soup(22, 6)
    srcs["cell"][13] = (1 << 19, 0, 0)
    out = E.mesh_weld(soup, srcs, raise_on_status=False)
    assert out["code"] == 4 and out["status"] == T.WELD_KEY_RANGE and out["counts"] == (0, 0)  # VH_ERR_BAD_ARGUMENT
    with pytest.raises(lib.VhError) as e:
        E.mesh_weld(soup, srcs)
    assert e.value.code == 4


def test_mesh_weld_does_not_depend_on_the_order_of_the_soup(extractions):
    from voxelhashing_amd import engine as E
    x = extractions("S2")["full"]
    perm = np.random.default_rng(7).permutation(len(x["triangles"]))
    got = E.mesh_weld(x["triangles"][perm], x["sources"][perm])
    assert MW.same_mesh(MW.canonical(got), MW.canonical(x["indexed"]))


# ---------------------------------------------------------------------------- 5. the host path

def read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    nv = int(re.search(rb"element vertex (\d+)", head).group(1))
    nf = int(re.search(rb"element face (\d+)", head).group(1))
    assert len(body) == nv * 16 + nf * 13
    faces = np.frombuffer(body[nv * 16:], dtype=np.dtype([("n", "u1"), ("i", "<i4", 3)]))
    assert np.all(faces["n"] == 3)
    return nv, nf, faces["i"]


def test_host_mesh_and_ply_are_the_indexed_mesh(extractions, tmp_path):
    x = extractions("S1")
    mc, hd, hpp = x["mc"], x["scene"].getHashData(), x["scene"].getHashParams()
    mc.extractIsoSurfaceIndexed(hd, hpp)
    ind = mc.indexed()
    V, F = len(ind["keys"]), len(ind["faces"])
    m = mc.mesh()
    assert m["vertices"].shape == (V, 3) and m["faces"].shape == (F, 3) and V > 100 and F > 100
    assert m["vertices"].tobytes() == ind["vertices"].tobytes() and m["colors"][:, :3].tobytes() == ind["colors"].tobytes()
    assert np.all(m["colors"][:, 3] == 1.0) and np.array_equal(m["faces"], ind["faces"])
    path = str(tmp_path / "indexed.ply")
    mc.saveMesh(path, None, True)
    nv, nf, faces = read_ply(path)
    assert nv == V and nf == F and np.array_equal(faces.astype(np.uint32), ind["faces"])
    assert mc.mesh()["vertices"].shape[0] == 0  # saveMesh clears the buffer

    # copyTrianglesToCPU after an indexed extraction appends the soup and clears the mark: saveMesh merges on the host
    # again (were the mark still set, the file would hold V + 3 n vertices and F + n faces)
    mc.extractIsoSurfaceIndexed(hd, hpp)
    n = mc.counts()["triangles"]
    mc.copyTrianglesToCPU()
    assert mc.mesh()["vertices"].shape[0] == V + 3 * n and mc.mesh()["faces"].shape[0] == F + n
    path2 = str(tmp_path / "merged.ply")
    mc.saveMesh(path2, None, True)
    nv2, nf2, _ = read_ply(path2)
    assert nv2 < V + 3 * n and nf2 < F + n and nv2 < 3 * n // 2


def test_indexed_extraction_refuses_an_overflowed_triangle_buffer(extractions):
    from voxelhashing_amd import engine as E, lib
    x = extractions("S1")
    n = len(x["full"]["triangles"])
    small = E.CUDAMarchingCubesHashSDF(T.make_marching_cubes_params(x["hp"], n // 2))
    with pytest.raises(lib.VhError) as e:
        small.extractIsoSurfaceIndexed(x["scene"].getHashData(), x["scene"].getHashParams())
    assert e.value.code == 2  # VH_ERR_STAGING_OVERFLOW, as copyTrianglesToCPU
    assert small.counts()["triangles"] == n
    m = small.mesh()
    assert m["vertices"].shape[0] == 0 and m["faces"].shape[0] == 0
    assert small.indexed_counts() == dict(vertices=0, faces=0, status=0) and len(small.indexed()["keys"]) == 0


# ---------------------------------------------------------------------------- 6. Reconstruction

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


def test_reconstruction_extracts_an_indexed_mesh(vh, oracle_lib, tmp_path):
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
    rec = R.Reconstruction(R.read_app_state((PARAMS + "s_streamingEnabled = false;\n").encode()), sens_files=[path])
    assert rec.run() == RN
    mesh = rec.extractIsoSurface(indexed=True)
    ind = rec.marching_cubes.indexed()
    assert len(mesh["faces"]) == len(ind["faces"]) > 500 and len(mesh["vertices"]) == len(ind["keys"])
    # with streaming the extraction walks the chunk grid, which has no indexed path: refused before any GPU work
    streamed = R.Reconstruction(R.read_app_state((PARAMS + STREAMING).encode()), sens_files=[path])
    launched = streamed.marching_cubes
    with pytest.raises(ValueError):
        streamed.extractIsoSurface(indexed=True)
    assert streamed.marching_cubes is launched is None  # not even the extractor was made
