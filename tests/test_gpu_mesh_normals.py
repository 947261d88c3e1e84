"""Vertex normals of the indexed mesh on the GPU ("Vertex normals"): vh_mesh_vertex_normals against
the numpy restatement (tests/mesh_normals.py), accumulators and normals bit for bit, on random and hand-made meshes; the
indexed extractions with setIndexedNormals on the scenes of tests/test_gpu_mesh_weld.py; the accumulating weld's pass
against the one-shot one; the chunk-grid walk against the direct extraction; the host path (mesh buffer, PLY); and
Reconstruction with normals=True, resident and streamed."""
import ctypes as C
import re

import numpy as np
import pytest

import mesh_normals as MN
import mesh_weld as MW
import mesh_weld_appends as MA
from helpers import small_config
from voxelhashing_amd import synth, vhtypes as T

pytestmark = pytest.mark.gpu

BAD_ARGUMENT = 4  # VH_ERR_BAD_ARGUMENT
SCALE = 30
MAX_TRIANGLES = 1 << 19


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def by_key(mesh):
    """normals of a mesh as the library returns it, in the order of MW.canonical(mesh)"""
    return np.ascontiguousarray(mesh["normals"][np.argsort(mesh["keys"], kind="stable")])


def restated(canonical_mesh, scale):
    return MN.vertex_normals(canonical_mesh["vertices"], canonical_mesh["keys"], canonical_mesh["faces"], scale)


# ---------------------------------------------------------------------------- 1. the launcher against the restatement

@pytest.mark.parametrize("n", [0, 1, 21, 22, 257])
def test_launcher_equals_the_restatement(vh, n):
    """random_soup(n, 10 + n) welded on the host: 63 / 66 soup vertices straddle a wave, 257 faces a workgroup"""
    from voxelhashing_amd import engine as E
    m = MW.weld(*MW.random_soup(n, 10 + n))
    want = MN.vertex_normals(m["vertices"], m["keys"], m["faces"], SCALE)
    got = E.mesh_vertex_normals(m["vertices"], m["keys"], m["faces"], SCALE)
    assert got["status"] == 0 == want["status"] and got["code"] == 0
    assert same_bits(got["acc"], want["acc"]) and same_bits(got["normals"], want["normals"])
    if n == 0:
        assert got["normals"].shape == (0, 3)
    if n == 257:
        assert len(m["faces"]) > 200 and np.any(want["normals"] != 0, axis=1).sum() > 400
    # the same faces in another order, every triple rotated: identical bytes
    rng = np.random.default_rng(n)
    f = m["faces"][rng.permutation(len(m["faces"]))]
    r = rng.integers(0, 3, len(f))
    f = np.stack([f[np.arange(len(f)), (r + k) % 3] for k in range(3)], axis=1).astype(np.uint32).reshape(-1, 3)
    again = E.mesh_vertex_normals(m["vertices"], m["keys"], f, SCALE)
    assert again["status"] == 0 and same_bits(again["acc"], got["acc"]) and same_bits(again["normals"], got["normals"])


def test_vertices_without_faces_still_get_their_zero_normals(vh):
    """F = 0 launches nothing that reads a face, and still leaves V zero normals"""
    from voxelhashing_amd import engine as E
    m = MW.weld(*MW.random_soup(22, 32))
    got = E.mesh_vertex_normals(m["vertices"], m["keys"], np.zeros((0, 3), dtype=np.uint32), SCALE)
    assert got["status"] == 0 and got["normals"].shape == (len(m["keys"]), 3) and not got["normals"].any() and not got["acc"].any()


# ---------------------------------------------------------------------------- 2. hand-made cases

def square():
    """a unit square in the plane z = 0 and a point above it; keys in the order of the vertices"""
    p = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0.5, 0.5, 1)], dtype=np.float32)
    return p, np.arange(10, 15, dtype=np.uint64)


def test_a_face_with_a_repeated_index_adds_nothing(vh):
    from voxelhashing_amd import engine as E
    p, keys = square()
    got = E.mesh_vertex_normals(p, keys, [(0, 1, 2), (0, 2, 2), (3, 3, 3), (4, 0, 4)], 20)
    want = MN.vertex_normals(p, keys, [(0, 1, 2), (0, 2, 2), (3, 3, 3), (4, 0, 4)], 20)
    assert got["status"] == 0 and same_bits(got["acc"], want["acc"]) and same_bits(got["normals"], want["normals"])
    assert np.array_equal(got["acc"][:3], np.tile([0, 0, 1 << 20], (3, 1))) and not got["acc"][3:].any()
    assert np.array_equal(got["normals"], np.array([(0, 0, 1)] * 3 + [(0, 0, 0)] * 2, dtype=np.float32))


def test_two_faces_that_cancel_give_zero(vh):
    from voxelhashing_amd import engine as E
    p, keys = square()
    faces = [(0, 1, 2), (2, 1, 0), (0, 2, 3)]  # the first two are one triangle in both windings
    got = E.mesh_vertex_normals(p, keys, faces, 20)
    want = MN.vertex_normals(p, keys, faces, 20)
    assert got["status"] == 0 and same_bits(got["acc"], want["acc"]) and same_bits(got["normals"], want["normals"])
    assert not got["acc"][1].any() and not got["normals"][1].any()  # vertex 1 has the two cancelling faces only
    assert np.array_equal(got["normals"][[0, 2, 3]], np.tile(np.float32([0, 0, 1]), (3, 1)))


def test_a_face_index_out_of_bounds_is_a_status(vh):
    """An index equal to V, in a face in the middle of the list, with the V vertices in the middle of larger buffers: a
    launcher that gathered through the index before testing it would stay inside the test's buffers, add to the
    accumulators behind the V-th vertex and show here as a missing status or a changed guard -- not as a fault."""
    from voxelhashing_amd import engine as E, lib
    m = MW.weld(*MW.random_soup(257, 267))
    V, guard = len(m["keys"]), 16
    f = m["faces"].copy()
    f[len(f) // 2, 1] = V
    assert MN.vertex_normals(m["vertices"], m["keys"], f, SCALE)["status"] == MN.BAD_INDEX
    v = np.zeros(V + guard, dtype=T.VERTEX_DTYPE)
    v["p"][:V] = m["vertices"]
    v["p"][V:] = np.random.default_rng(5).standard_normal((guard, 3)).astype(np.float32)  # finite: a face through them is in range
    k = np.concatenate([m["keys"], np.arange(1, guard + 1, dtype=np.uint64)])              # smaller than every real key
    acc0 = np.full(3 * (V + guard), 0x5555555555555555, dtype=np.int64)
    n0 = np.full(3 * (V + guard), 7.0, dtype=np.float32)
    bufs = [lib.DeviceBuffer.from_numpy(a) for a in (v, k, f, acc0, n0, np.array([9], dtype=np.uint32))]
    try:
        d_v, d_k, d_f, d_acc, d_n, d_st = bufs
        lib.check(vh.vh_mesh_vertex_normals(d_v.ptr, d_k.ptr, d_f.ptr, V, len(f), SCALE, d_acc.ptr, d_n.ptr, d_st.ptr, None), "vh_mesh_vertex_normals")
        status = int(d_st.download(np.uint32, 1)[0])
        acc, normals = d_acc.download(np.int64), d_n.download(np.float32)
    finally:
        for b in bufs:
            b.free()
    assert status == T.NORMALS_BAD_INDEX
    assert not normals[:3 * V].any() and np.all(normals[3 * V:] == 7.0)  # V zero normals, and nothing behind them
    assert np.all(acc[3 * V:] == 0x5555555555555555)                     # nothing was added through the index
    # the other faces did add: the refusal is the status word's, not an early exit of the launch
    want = MN.vertex_normals(m["vertices"], m["keys"], f, SCALE)
    assert np.array_equal(acc[:3 * V].reshape(-1, 3), want["acc"]) and want["acc"].any()
    # and through the mirror: both bits map to VH_ERR_BAD_ARGUMENT
    got = E.mesh_vertex_normals(m["vertices"], m["keys"], f, SCALE, raise_on_status=False)
    assert got["status"] == T.NORMALS_BAD_INDEX and got["code"] == BAD_ARGUMENT and not got["normals"].any()
    with pytest.raises(lib.VhError) as e:
        E.mesh_vertex_normals(m["vertices"], m["keys"], f, SCALE)
    assert e.value.code == BAD_ARGUMENT


def test_a_scale_that_leaves_the_range_is_a_status(vh):
    from voxelhashing_amd import engine as E
    m = MW.weld(*MW.random_soup(257, 267))
    # the restatement picks the scale: the first at which it reports a face out of range
    scale = next(s for s in range(SCALE, 101) if MN.vertex_normals(m["vertices"], m["keys"], m["faces"], s)["status"] & MN.RANGE)
    assert scale > 36 and MN.vertex_normals(m["vertices"], m["keys"], m["faces"], scale - 1)["status"] == 0
    got = E.mesh_vertex_normals(m["vertices"], m["keys"], m["faces"], scale, raise_on_status=False)
    assert got["status"] == T.NORMALS_RANGE and got["code"] == BAD_ARGUMENT and not got["normals"].any()
    below = E.mesh_vertex_normals(m["vertices"], m["keys"], m["faces"], scale - 1)
    want = MN.vertex_normals(m["vertices"], m["keys"], m["faces"], scale - 1)
    assert below["status"] == 0 and same_bits(below["acc"], want["acc"]) and same_bits(below["normals"], want["normals"])
    # an infinite and a NaN position: not finite is out of range too
    p = m["vertices"].copy()
    p[m["faces"][3, 0]] = (np.inf, 0, 0)
    p[m["faces"][90, 1]] = (np.nan, 1, 1)
    assert MN.vertex_normals(p, m["keys"], m["faces"], SCALE)["status"] == MN.RANGE
    got = E.mesh_vertex_normals(p, m["keys"], m["faces"], SCALE, raise_on_status=False)
    assert got["status"] == T.NORMALS_RANGE and not got["normals"].any()


# ---------------------------------------------------------------------------- 3. the scenes of test_gpu_mesh_weld.py

SCENES = {"S1": (64, 48, "P2", "S1"), "S2": (80, 60, "P4", "S2")}


def read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    props = [p.decode() for p in re.findall(rb"property (?:float|uchar) (\w+)", head.split(b"element face")[0])]
    nv = int(re.search(rb"element vertex (\d+)", head).group(1))
    nf = int(re.search(rb"element face (\d+)", head).group(1))
    dt = np.dtype([("p", "<f4", 3)] + ([("n", "<f4", 3)] if "nx" in props else []) + [("c", "u1", 4)])
    assert len(body) == nv * dt.itemsize + nf * 13
    verts = np.frombuffer(body[:nv * dt.itemsize], dtype=dt)
    faces = np.frombuffer(body[nv * dt.itemsize:], dtype=np.dtype([("k", "u1"), ("i", "<i4", 3)]))
    assert np.all(faces["k"] == 3)
    return props, verts, faces["i"]


@pytest.fixture(scope="module")
def extractions(vh):
    """name -> the indexed extraction of that scene (three orbit frames) with normals, whole and in the box of
    tests/test_gpu_mesh_weld.py, and with the option off; made once"""
    from voxelhashing_amd import engine as E
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        width, height, params, scene_name = SCENES[name]
        hp, cp, _ = small_config(width, height, params=params)
        spheres, inside, radius = synth.scene(scene_name)
        scene = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=True, gc=False))
        frame = E.DepthFrame(cp)
        for pose in [synth.orbit_pose(k, 100, radius) for k in range(3)]:
            E.synth_frame(spheres, inside, pose, cp, out=frame)
            scene.integrate(pose, frame, cp, None)
        hd, hpp = scene.getHashData(), scene.getHashParams()
        mc = E.CUDAMarchingCubesHashSDF(T.make_marching_cubes_params(hp, MAX_TRIANGLES))
        mc.extractIsoSurfaceIndexed(hd, hpp)
        off = dict(indexed=mc.indexed(), mesh=mc.mesh())
        cx = float(np.median(mc.triangles()["v"]["p"][..., 0]))
        box = ((cx, -10.0, -10.0), (10.0, 10.0, 10.0))
        mc.setIndexedNormals(True)
        mc.extractIsoSurfaceIndexed(hd, hpp, box[0], box[1], True)
        boxed = dict(indexed=mc.indexed(), mesh=mc.mesh())
        mc.extractIsoSurfaceIndexed(hd, hpp)
        full = dict(indexed=mc.indexed(), mesh=mc.mesh())
        cache[name] = dict(scene=scene, hp=hp, mc=mc, off=off, full=full, boxed=boxed, scale=E.mesh_normals_default_scale_log2(hp.m_virtualVoxelSize))
        return cache[name]

    return get


@pytest.mark.parametrize("name", ["S1", "S2"])
@pytest.mark.parametrize("part", ["full", "boxed"])
def test_extraction_normals_equal_the_restatement(extractions, name, part):
    x = extractions(name)
    ind = x[part]["indexed"]
    m = MW.canonical(ind)
    want = restated(m, x["scale"])
    got = by_key(ind)
    assert want["status"] == 0 and len(m["keys"]) > 100 and len(m["faces"]) > 100
    assert same_bits(got, want["normals"])
    # ... and the restatement, and so the device, stays within the float64 bound of tests/test_mesh_normals.py
    ratio, unit = MN.check_against_reference(got, m["vertices"], m["faces"], x["scale"])
    print(name, part, "scale", x["scale"], "error / bound", ratio, "| |n| - 1 |", unit)
    # no normal is zero at a vertex with a face, unless the restatement says so
    _, _, valence = MN.reference(m["vertices"], m["faces"], x["scale"])
    zero = ~np.any(got != 0, axis=1)
    print("vertices", len(zero), "without a face", int((valence == 0).sum()), "zero normals", int(zero.sum()))
    assert np.array_equal(zero, ~np.any(want["normals"] != 0, axis=1)) and np.all(zero[valence == 0])
    assert (zero & (valence > 0)).sum() <= len(zero) // 100  # (faces without an area: two keys at one position)
    # the mesh buffer has them in the download's order
    assert same_bits(x[part]["mesh"]["normals"], ind["normals"]) and x[part]["mesh"]["vertices"].tobytes() == ind["vertices"].tobytes()


def test_option_off_leaves_every_output_as_it_was(extractions, tmp_path):
    x = extractions("S1")
    assert set(x["off"]["indexed"]) == {"vertices", "colors", "keys", "faces"} and set(x["off"]["mesh"]) == {"vertices", "colors", "faces"}
    # the same mesh with and without the option
    a, b = MW.canonical(x["off"]["indexed"]), MW.canonical(x["full"]["indexed"])
    assert MW.same_mesh(a, b)
    mc, hd, hpp = x["mc"], x["scene"].getHashData(), x["scene"].getHashParams()
    mc.setIndexedNormals(False)
    try:
        mc.extractIsoSurfaceIndexed(hd, hpp)
        V, F = len(mc.indexed()["keys"]), len(mc.indexed()["faces"])
        assert "normals" not in mc.indexed() and "normals" not in mc.mesh()
        path = str(tmp_path / "plain.ply")
        mc.saveMesh(path, None, True)
        props, verts, faces = read_ply(path)
        assert props == ["x", "y", "z", "red", "green", "blue", "alpha"] and verts.dtype.itemsize == 16 and len(verts) == V and len(faces) == F
        from voxelhashing_amd import lib
        with pytest.raises(lib.VhError) as e:  # an extraction without normals has none to download
            lib.check(mc.L.vh_marching_cubes_download_indexed_normals(mc.handle, None), "download_indexed_normals")
        assert e.value.code == BAD_ARGUMENT
    finally:
        mc.setIndexedNormals(True)


def test_ply_has_the_normals_and_a_soup_drops_them(extractions, tmp_path):
    x = extractions("S2")
    mc, hd, hpp = x["mc"], x["scene"].getHashData(), x["scene"].getHashParams()
    mc.extractIsoSurfaceIndexed(hd, hpp)
    ind = mc.indexed()
    V, F = len(ind["keys"]), len(ind["faces"])
    path = str(tmp_path / "normals.ply")
    mc.saveMesh(path, None, True)
    props, verts, faces = read_ply(path)
    assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "alpha"]
    assert verts.dtype.itemsize == 28 and len(verts) == V and len(faces) == F
    assert verts["p"].tobytes() == ind["vertices"].tobytes() and verts["n"].tobytes() == ind["normals"].tobytes()
    assert np.array_equal(faces.astype(np.uint32), ind["faces"])
    assert mc.mesh()["normals"].shape == (0, 3)  # saveMesh clears the buffer
    # copyTrianglesToCPU afterwards appends the soup, clears the welded mark and drops the normals
    mc.extractIsoSurfaceIndexed(hd, hpp)
    assert mc.mesh()["normals"].shape == (V, 3)
    n = mc.counts()["triangles"]
    mc.copyTrianglesToCPU()
    m = mc.mesh()
    assert m["vertices"].shape[0] == V + 3 * n and m["normals"].shape == (0, 3)
    path2 = str(tmp_path / "merged.ply")
    mc.saveMesh(path2, None, True)
    props2, verts2, _ = read_ply(path2)
    assert "nx" not in props2 and verts2.dtype.itemsize == 16
    mc.extractIsoSurfaceIndexed(hd, hpp)
    mc.clearMeshBuffer()
    assert mc.mesh()["normals"].shape == (0, 3) and mc.mesh()["vertices"].shape == (0, 3)


# ---------------------------------------------------------------------------- 4. the accumulating weld

@pytest.fixture(scope="module")
def dealt(vh):
    """the 2 000-triangle soup of tests/test_gpu_mesh_weld_appends.py dealt into 5 appends (a third of the cells repeated
    whole, as identical copies), and the one-shot weld of the whole with its normals"""
    from voxelhashing_amd import engine as E
    soup, srcs = MW.random_soup(2000, 11, spread=3)
    parts = MA.deal(soup, srcs, 5, 11)
    whole = E.mesh_weld(soup, srcs)
    whole["normals"] = E.mesh_vertex_normals(whole["vertices"], whole["keys"], whole["faces"], SCALE)["normals"]
    m = MW.canonical(whole)
    want = restated(m, SCALE)
    assert want["status"] == 0 and same_bits(by_key(whole), want["normals"])
    return dict(parts=parts, mesh=m, normals=want["normals"])


@pytest.mark.parametrize("order, slots_log2", [((0, 1, 2, 3, 4), 0), ((4, 3, 2, 1, 0), 0), ((2, 0, 4, 1, 3), 0), ((0, 1, 2, 3, 4), 6)])
def test_accumulated_normals_are_the_one_shot_welds(vh, dealt, order, slots_log2):
    """over all the faces with the final vertex bits: whatever the order of the appends, and from a table that starts at
    2^6 slots and is rehashed on the way"""
    from voxelhashing_amd import engine as E
    got = E.mesh_weld_appends([dealt["parts"][i] for i in order], slots_log2=slots_log2, normals_scale_log2=SCALE)
    assert got["status"] == 0 and got["normals_code"] == 0
    assert MW.same_mesh(MW.canonical(got), dealt["mesh"])
    assert same_bits(by_key(got), dealt["normals"])
    if slots_log2 == 6:
        assert got["stats"]["rehashes"] >= 3


def test_a_pass_is_stale_after_an_append(vh, dealt):
    from voxelhashing_amd import lib
    L = vh
    h = C.c_void_p()
    lib.check(L.vh_mesh_weld_accum_create(0, 0, 0, C.byref(h)), "create")
    bufs = []
    try:
        def append(part):
            tris = np.ascontiguousarray(part[0], dtype=T.TRIANGLE_DTYPE).ravel()
            srcs = np.ascontiguousarray(part[1], dtype=T.TRIANGLE_SOURCE_DTYPE).ravel()
            bufs.extend([lib.DeviceBuffer.from_numpy(tris), lib.DeviceBuffer.from_numpy(srcs)])
            lib.check(L.vh_mesh_weld_accum_append(h, bufs[-2].ptr, bufs[-1].ptr, len(tris), None), "append")

        def download():
            counts = (C.c_uint32 * 6)()
            lib.check(L.vh_mesh_weld_accum_get_counts(h, counts, None), "get_counts")
            out = np.full((int(counts[0]), 3), 7.0, dtype=np.float32)
            return L.vh_mesh_weld_accum_download_normals(h, out.ctypes.data, len(out), None), out

        lib.check(L.vh_mesh_weld_accum_begin(h, None), "begin")
        assert download()[0] == BAD_ARGUMENT  # no pass yet
        for part in dealt["parts"][:4]:
            append(part)
        lib.check(L.vh_mesh_weld_accum_normals(h, SCALE, None), "normals")
        code, first = download()
        assert code == 0 and np.any(first != 0, axis=1).sum() > 500
        assert L.vh_mesh_weld_accum_download_normals(h, first.ctypes.data, len(first) + 1, None) == BAD_ARGUMENT  # more than the pass saw
        append(dealt["parts"][4])
        code, untouched = download()
        assert code == BAD_ARGUMENT and np.all(untouched == 7.0)  # refused, and nothing copied
        lib.check(L.vh_mesh_weld_accum_normals(h, SCALE, None), "normals")
        code, last = download()
        assert code == 0
        counts = (C.c_uint32 * 6)()
        lib.check(L.vh_mesh_weld_accum_get_counts(h, counts, None), "get_counts")
        keys = np.zeros(int(counts[0]), dtype=np.uint64)
        lib.check(L.vh_mesh_weld_accum_download(h, None, keys.ctypes.data, None, len(keys), 0, None), "download")
        assert same_bits(np.ascontiguousarray(last[np.argsort(keys, kind="stable")]), dealt["normals"])
        lib.check(L.vh_mesh_weld_accum_begin(h, None), "begin")
        assert download()[0] == BAD_ARGUMENT  # a begin makes it stale as well
        assert L.vh_mesh_weld_accum_normals(h, 101, None) == BAD_ARGUMENT
    finally:
        L.vh_mesh_weld_accum_destroy(h)
        for b in bufs:
            b.free()


# ---------------------------------------------------------------------------- 5. the chunk grid

def test_chunk_grid_walk_normals_are_the_direct_extractions(vh):
    """the 96x72 scene of tests/test_gpu_mesh_weld_appends.py: three S1 orbit frames, 1 m chunks, a 9^3 grid from -4"""
    from voxelhashing_amd import engine as E
    hp, cp, _ = small_config(96, 72, streaming_extents=(1.0, 1.0, 1.0), streaming_dims=(9, 9, 9), streaming_min=(-4, -4, -4))
    scene = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=True, gc=False))
    frame = E.DepthFrame(cp)
    for pose in [synth.orbit_pose(k, n_frames=100) for k in range(3)]:
        E.synth_frame(synth.S1_SPHERES, 0, pose, cp, out=frame)
        scene.integrate(pose, frame, cp, None)
    mp = T.make_marching_cubes_params(hp, MAX_TRIANGLES)
    direct = E.CUDAMarchingCubesHashSDF(mp)
    direct.setIndexedNormals(True)
    direct.extractIsoSurfaceIndexed(scene.getHashData(), scene.getHashParams())
    want = direct.indexed()
    assert direct.counts()["triangles"] == 4005
    grid = E.CUDASceneRepChunkGrid(scene, (1.0, 1.0, 1.0), (9, 9, 9), (-4, -4, -4), 64, True, 4)
    try:
        mc = E.CUDAMarchingCubesHashSDF(mp)
        mc.setIndexedNormals(True)
        mc.extractIsoSurfaceIndexedChunkGrid(grid, (0.0, 0.0, 0.0), 100.0)
        got, stats, mesh = mc.indexed(), mc.indexed_stats(), mc.mesh()
        # the walk with the option off: the mesh it always gave
        mc.setIndexedNormals(False)
        mc.extractIsoSurfaceIndexedChunkGrid(grid, (0.0, 0.0, 0.0), 100.0)
        off, off_mesh = mc.indexed(), mc.mesh()
    finally:
        grid.close()
    assert stats["dropped"] > 0 and stats["status"] == 0
    assert MW.same_mesh(MW.canonical(got), MW.canonical(want)) and same_bits(by_key(got), by_key(want))
    m = MW.canonical(got)
    assert same_bits(by_key(got), restated(m, E.mesh_normals_default_scale_log2(hp.m_virtualVoxelSize))["normals"])
    assert same_bits(mesh["normals"], got["normals"])
    assert "normals" not in off and "normals" not in off_mesh and MW.same_mesh(MW.canonical(off), m)


def test_one_object_switches_between_one_shot_and_accumulated_with_normals(vh):
    """The scene of test_two_overlapping_boxes_give_the_direct_mesh (tests/test_gpu_mesh_weld_appends.py): a few hundred
    faces.  The one-shot extraction and the accumulation have normals buffers of their own behind one read-back: one
    object that goes from one to the other and back gives the same mesh and the same normals each time, and turning the
    option off afterwards leaves the mesh and takes only the normals away."""
    from voxelhashing_amd import engine as E, lib
    hp, cp, _ = small_config(64, 48, params="P2")
    scene = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=True, gc=False))
    frame = E.DepthFrame(cp)
    for pose in [synth.orbit_pose(k, 100) for k in range(2)]:
        E.synth_frame(synth.S1_SPHERES, 0, pose, cp, out=frame)
        scene.integrate(pose, frame, cp, None)
    hd, hpp = scene.getHashData(), scene.getHashParams()
    mc = E.CUDAMarchingCubesHashSDF(T.make_marching_cubes_params(hp, MAX_TRIANGLES))
    empty = dict(vertices=0, faces=0, status=0)
    with pytest.raises(lib.VhError) as e:  # an append without a begin
        mc.appendIndexed(hd, hpp)
    assert e.value.code == BAD_ARGUMENT and mc.indexed_counts() == empty and set(mc.indexed_stats().values()) == {0}
    mc.setIndexedNormals(True)

    def accumulated():
        mc.beginIndexed()
        mc.appendIndexed(hd, hpp)
        mc.finishIndexed()

    seen = []
    for extract in (lambda: mc.extractIsoSurfaceIndexed(hd, hpp), accumulated, lambda: mc.extractIsoSurfaceIndexed(hd, hpp)):
        extract()
        ind, mesh = mc.indexed(), mc.mesh()
        assert same_bits(mesh["normals"], ind["normals"]) and mesh["vertices"].tobytes() == ind["vertices"].tobytes()
        seen.append((MW.canonical(ind), by_key(ind), mc.indexed_counts(), mc.indexed_stats()))
    first, normals, counts, _ = seen[0]
    assert len(first["faces"]) > 500 and counts == dict(vertices=len(first["keys"]), faces=len(first["faces"]), status=0)
    assert same_bits(normals, restated(first, E.mesh_normals_default_scale_log2(hp.m_virtualVoxelSize))["normals"]) and normals.any()
    for m, n, c, _ in seen[1:]:
        assert MW.same_mesh(m, first) and same_bits(n, normals) and c == counts
    # the stats are the accumulation's alone
    assert set(seen[0][3].values()) == {0} == set(seen[2][3].values()) and seen[1][3]["vertices"] == counts["vertices"] and seen[1][3]["cells"] > 0
    mc.setIndexedNormals(False)
    mc.extractIsoSurfaceIndexed(hd, hpp)
    ind = mc.indexed()
    assert "normals" not in ind and "normals" not in mc.mesh() and MW.same_mesh(MW.canonical(ind), first)
    with pytest.raises(lib.VhError) as e:
        lib.check(mc.L.vh_marching_cubes_download_indexed_normals(mc.handle, None), "download_indexed_normals")
    assert e.value.code == BAD_ARGUMENT
    with pytest.raises(lib.VhError) as e:  # still no begin: refused before anything is touched
        mc.appendIndexed(hd, hpp)
    assert e.value.code == BAD_ARGUMENT and mc.indexed_counts() == counts and set(mc.indexed_stats().values()) == {0}


# ---------------------------------------------------------------------------- 6. Reconstruction

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


def test_reconstruction_extracts_normals_resident_and_streamed(vh, oracle_lib, tmp_path):
    from voxelhashing_amd import engine as E, reconstruction as R, sensor_data as SD
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
    scale = E.mesh_normals_default_scale_log2(0.02)
    assert scale == 49
    for name, extra in (("resident", "s_streamingEnabled = false;\n"), ("streamed", STREAMING)):
        rec = R.Reconstruction(R.read_app_state((PARAMS + extra).encode()), sens_files=[path])
        assert rec.run() == RN and (rec.chunk_grid is not None) == (name == "streamed")
        ply = str(tmp_path / (name + ".ply"))
        mesh = rec.extractIsoSurfaceIndexed(ply, normals=True) if name == "streamed" else rec.extractIsoSurface(ply, indexed=True, normals=True)
        ind = rec.marching_cubes.indexed()
        assert len(ind["faces"]) > 500 and same_bits(mesh["normals"], ind["normals"]) and mesh["normals"].shape == (len(ind["keys"]), 3)
        m = MW.canonical(ind)
        want = restated(m, scale)
        assert want["status"] == 0 and same_bits(by_key(ind), want["normals"])
        MN.check_against_reference(by_key(ind), m["vertices"], m["faces"], scale)
        props, verts, faces = read_ply(ply)
        assert props[3:6] == ["nx", "ny", "nz"] and verts["n"].tobytes() == ind["normals"].tobytes() and len(faces) == len(ind["faces"])
        with pytest.raises(ValueError):
            rec.extractIsoSurface(normals=True)  # normals need the welded mesh
        plain = rec.extractIsoSurfaceIndexed()   # and the default is without them
        assert set(plain) == {"vertices", "colors", "faces"} and "normals" not in rec.marching_cubes.indexed()
