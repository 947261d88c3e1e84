"""Connected components of the indexed mesh on the GPU ("Mesh components"): vh_mesh_components and
vh_mesh_components_filter against the numpy restatement (tests/mesh_components.py) -- roots, face counts, the six
counts and the canonical filtered mesh bit for bit -- on random and hand-made meshes; the indexed extractions with
setIndexedComponentFilter on the scenes of tests/test_gpu_mesh_weld.py; the accumulating weld's pass against the
one-shot one; the chunk-grid walk against the direct extraction; the host path (mesh buffer, PLY); and Reconstruction,
resident and streamed."""
import ctypes as C
import re

import numpy as np
import pytest

import mesh_components as MC
import mesh_weld as MW
import mesh_weld_appends as MA
from helpers import small_config
from voxelhashing_amd import synth, vhtypes as T

pytestmark = pytest.mark.gpu

BAD_ARGUMENT = 4  # VH_ERR_BAD_ARGUMENT
SCALE = 30
MAX_TRIANGLES = 1 << 19
MESH_KEYS = ("vertices", "colors", "keys", "faces")


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_against_restatement(E, mesh, min_faces=0, largest_only=False):
    """the launchers on `mesh` (vertices, colors, keys, faces, optionally normals) against MC.filter, bit for bit -> both"""
    want = MC.filter(mesh, min_faces, largest_only)
    got = E.mesh_components_filter(mesh["vertices"], mesh["colors"], mesh["keys"], mesh["faces"], min_faces, largest_only, normals=mesh.get("normals"))
    assert got["status"] == 0 == want["status"] and got["code"] == 0
    assert same_bits(got["root"], want["root"]) and same_bits(got["face_count"], want["face_count"])
    assert same_bits(MC.root_keys(mesh["keys"], got["root"]), MC.root_keys(mesh["keys"], want["root"]))
    assert got["counts"] == want["counts"]
    g = MC.canonical(got)
    assert MW.same_mesh(g, want["mesh"])
    if "normals" in mesh:
        assert same_bits(g["normals"], want["mesh"]["normals"])
    return got, want


def shuffled_faces(faces, seed):
    """the same faces in another order, every triple rotated"""
    rng = np.random.default_rng(seed)
    f = faces[rng.permutation(len(faces))]
    r = rng.integers(0, 3, len(f))
    return np.stack([f[np.arange(len(f)), (r + k) % 3] for k in range(3)], axis=1).astype(np.uint32).reshape(-1, 3)


# ---------------------------------------------------------------------------- 1. the launchers against the restatement

@pytest.mark.parametrize("isolated", [False, True])
@pytest.mark.parametrize("n", [0, 1, 21, 22, 257])
def test_launchers_equal_the_restatement(vh, n, isolated):
    """random_soup(n, 10 + n) welded on the host: 63 / 66 vertices straddle a wave, 257 faces a workgroup; isolated: n
    components of one face"""
    from voxelhashing_amd import engine as E
    m = MW.weld(*MW.random_soup(n, 10 + n, isolated=isolated))
    got, want = check_against_restatement(E, m)
    assert got["counts"]["kept_vertices"] == len(m["keys"]) and got["counts"]["kept_faces"] == len(m["faces"])  # the filter off: the identity
    if isolated:
        assert want["counts"]["components"] == n and want["counts"]["largest_faces"] == min(n, 1)
    check_against_restatement(E, m, 2)
    check_against_restatement(E, m, 0, True)
    # the same faces permuted, with every triple rotated, give identical labels and the same mesh
    again = E.mesh_components_filter(m["vertices"], m["colors"], m["keys"], shuffled_faces(m["faces"], n), 2)
    first = E.mesh_components_filter(m["vertices"], m["colors"], m["keys"], m["faces"], 2)
    assert same_bits(again["root"], first["root"]) and same_bits(again["face_count"], first["face_count"]) and again["counts"] == first["counts"]
    assert MW.same_mesh(MC.canonical(again), MC.canonical(first))


@pytest.fixture(scope="module")
def archipelago():
    m = MW.weld(*MC.archipelago())
    base = MC.filter(m)
    assert base["counts"]["components"] >= 6 and base["counts"]["largest_faces"] > 200
    return m, base


def test_archipelago(vh, archipelago):
    from voxelhashing_amd import engine as E
    m, base = archipelago
    check_against_restatement(E, m)
    check_against_restatement(E, dict(m, faces=shuffled_faces(m["faces"], 9)), 3)


@pytest.mark.parametrize("how", ["ascending", "descending", "shuffled"])
def test_a_long_strip_stays_within_the_step_bound(vh, how):
    """4 096 triangles in a row: the long chains; the status stays 0"""
    from voxelhashing_amd import engine as E
    m = MC.strip(4096, how, seed=4)
    got, want = check_against_restatement(E, m, 0, True)
    assert want["counts"] == dict(components=1, faceless_vertices=0, kept_components=1, kept_vertices=4098, kept_faces=4096, largest_faces=4096)
    assert np.all(got["root"] == np.argmin(m["keys"]))


def test_a_fan_round_one_hub(vh):
    """4 096 faces that all name vertex 0: every compare-and-swap contends on a few words"""
    from voxelhashing_amd import engine as E
    m = MC.fan(4096, seed=6)
    got, want = check_against_restatement(E, m, 1)
    assert want["counts"]["components"] == 1 and want["counts"]["kept_faces"] == 4096 and np.all(got["root"] == np.argmin(m["keys"]))


def test_hand_made_meshes(vh):
    from voxelhashing_amd import engine as E
    cases = [(np.array([80, 70, 60, 50, 40, 30, 20, 10], dtype=np.uint64), [(0, 1, 2), (2, 1, 3), (4, 5, 6)]),  # a shared edge, a separate triangle, a faceless vertex
             (np.array([5, 9, 7, 3, 8], dtype=np.uint64), [(0, 1, 2), (3, 0, 4)]),                                  # a bow-tie
             (np.array([4, 3, 2, 1], dtype=np.uint64), [(0, 0, 1), (2, 3, 2)]),                                     # repeated indices
             (np.array([4, 3, 2, 1], dtype=np.uint64), [(0, 0, 0)])]
    for keys, faces in cases:
        m = MC.plain_mesh(keys, faces)
        for min_faces, largest in ((0, False), (1, False), (2, False), (0, True)):
            check_against_restatement(E, m, min_faces, largest)
    # equal keys are settled by the index (the canonical form sorts by key alone: compare labels and counts)
    keys = np.full(6, 42, dtype=np.uint64)
    faces = np.array([(5, 4, 3), (2, 1, 0)], dtype=np.uint32)
    got = E.mesh_components_filter(np.zeros((6, 3), dtype=np.float32), None, keys, faces, 0, True)
    assert got["root"].tolist() == [0, 0, 0, 3, 3, 3] and got["face_count"].tolist() == [1, 0, 0, 1, 0, 0]
    assert got["counts"] == MC.filter(MC.plain_mesh(keys, faces), 0, True)["counts"] and got["faces"].shape == (1, 3)
    assert sorted(got["faces"][0].tolist()) == [0, 1, 2] and got["counts"]["kept_vertices"] == 3


def test_a_face_index_out_of_bounds_is_a_status(vh):
    """An index equal to V, in a face in the middle of the list, with the V vertices in the middle of larger buffers: a
    launcher that gathered through the index before testing it would stay inside the test's buffers, and show here as
    a missing status, a changed guard or a vertex joined to the guard -- not as a fault."""
    from voxelhashing_amd import engine as E, lib
    m = MW.weld(*MW.random_soup(257, 267))
    V, guard = len(m["keys"]), 16
    f = m["faces"].copy()
    f[len(f) // 2, 1] = V
    want = MC.filter(dict(m, faces=f))
    assert want["status"] == MC.BAD_INDEX
    k = np.concatenate([m["keys"], np.arange(1, guard + 1, dtype=np.uint64)])  # smaller than every real key: a root, if it were joined
    got = E.mesh_components(k, f, guard=guard)
    assert got["status"] == T.COMPONENTS_BAD_INDEX and got["code"] == BAD_ARGUMENT
    assert np.all(got["root_guard"] == 0xa5a5a5a5) and np.all(got["count_guard"] == 0xa5a5a5a5)  # nothing is written behind V
    # the other faces still joined: the refusal is the status word's, not an early exit of the launch
    assert same_bits(got["root"], want["root"]) and same_bits(got["face_count"], want["face_count"])
    assert int(got["face_count"].sum()) == len(f) - 1 and len(np.unique(got["root"])) < V - 100
    # the filter then keeps nothing, and all its counts read 0
    out = E.mesh_components_filter(m["vertices"], m["colors"], m["keys"], f, 0, False, raise_on_status=False)
    assert out["status"] == T.COMPONENTS_BAD_INDEX and out["code"] == BAD_ARGUMENT and set(out["counts"].values()) == {0}
    assert len(out["keys"]) == 0 and out["faces"].shape == (0, 3) and out["counts"] == want["counts"]
    with pytest.raises(lib.VhError) as e:
        E.mesh_components_filter(m["vertices"], m["colors"], m["keys"], f, 1)
    assert e.value.code == BAD_ARGUMENT


def test_without_faces_every_vertex_is_its_own_root(vh):
    from voxelhashing_amd import engine as E
    m = MW.weld(*MW.random_soup(22, 32))
    m = dict(m, faces=np.zeros((0, 3), dtype=np.uint32))
    got, want = check_against_restatement(E, m)
    V = len(m["keys"])
    assert got["root"].tolist() == list(range(V)) and not got["face_count"].any() and want["counts"]["faceless_vertices"] == V == want["counts"]["kept_vertices"]
    check_against_restatement(E, m, 1)
    got, _ = check_against_restatement(E, m, 0, True)  # without a face nothing is the largest
    assert got["counts"]["kept_vertices"] == 0


# ---------------------------------------------------------------------------- 2. the filter

def test_filter_edges(vh, archipelago):
    from voxelhashing_amd import engine as E
    m, base = archipelago
    sizes = MC.sizes(base["face_count"])
    second = int(sizes[1])
    at, _ = check_against_restatement(E, m, second)          # minFaces equal to a component's size keeps it ...
    above, _ = check_against_restatement(E, m, second + 1)   # ... one more drops it
    assert at["counts"]["kept_components"] == above["counts"]["kept_components"] + int((sizes == second).sum()) == int((sizes >= second).sum())
    largest, _ = check_against_restatement(E, m, 0, True)
    assert largest["counts"]["kept_components"] == 1 and largest["counts"]["kept_faces"] == int(sizes[0])
    nothing, _ = check_against_restatement(E, m, int(sizes[0]) + 1)  # a threshold above everything gives an empty mesh
    assert nothing["counts"]["kept_vertices"] == 0 == nothing["counts"]["kept_faces"] and nothing["faces"].shape == (0, 3)
    check_against_restatement(E, m, int(sizes[0]) + 1, True)
    check_against_restatement(E, m, second, True)


def test_a_tie_for_the_largest_goes_to_the_earlier_root(vh):
    from voxelhashing_amd import engine as E
    m = MW.weld(*MW.random_soup(257, 267, isolated=True))  # 257 components of one face: ties in every wave and across workgroups
    got, want = check_against_restatement(E, m, 0, True)
    assert want["counts"]["kept_components"] == 1 and want["counts"]["kept_vertices"] == 3 and got["keys"].min() == m["keys"].min()


def test_normals_ride_along(vh, archipelago):
    """the normals of the kept vertices are the unfiltered normals at the kept keys"""
    from voxelhashing_amd import engine as E
    m, _ = archipelago
    normals = E.mesh_vertex_normals(m["vertices"], m["keys"], m["faces"], SCALE)["normals"]
    assert np.any(normals != 0, axis=1).sum() > 300
    got, _ = check_against_restatement(E, dict(m, normals=normals), 5)
    at = np.searchsorted(m["keys"], got["keys"])  # (a welded mesh in canonical form: keys ascending)
    assert np.array_equal(m["keys"][at], got["keys"]) and same_bits(got["normals"], np.ascontiguousarray(normals[at])) and 0 < len(at) < len(m["keys"])


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
def scenes(vh):
    """name -> the scene (three orbit frames), an extractor, and its unfiltered indexed mesh with normals; made once"""
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
        off = dict(indexed=mc.indexed(), mesh=mc.mesh(), counts=mc.indexed_counts(), stats=mc.indexed_component_stats())
        cx = float(np.median(mc.triangles()["v"]["p"][..., 0]))
        box = ((cx, -10.0, -10.0), (10.0, 10.0, 10.0))
        mc.setIndexedNormals(True)
        mc.extractIsoSurfaceIndexed(hd, hpp)
        full = mc.indexed()
        mc.extractIsoSurfaceIndexed(hd, hpp, box[0], box[1], True)
        boxed = mc.indexed()
        cache[name] = dict(scene=scene, hp=hp, mc=mc, off=off, full=full, boxed=boxed, box=box)
        return cache[name]

    return get


def extract_filtered(x, part, min_faces, largest_only):
    mc, hd, hpp = x["mc"], x["scene"].getHashData(), x["scene"].getHashParams()
    mc.setIndexedComponentFilter(min_faces, largest_only)
    try:
        if part == "boxed":
            mc.extractIsoSurfaceIndexed(hd, hpp, x["box"][0], x["box"][1], True)
        else:
            mc.extractIsoSurfaceIndexed(hd, hpp)
        return dict(indexed=mc.indexed(), mesh=mc.mesh(), counts=mc.indexed_counts(), stats=mc.indexed_component_stats())
    finally:
        mc.setIndexedComponentFilter(0, False)


def assert_is_the_restatements(got, want):
    """an extraction with the filter on against MC.filter of the device's own unfiltered mesh"""
    assert got["stats"] == want["counts"]
    assert got["counts"] == dict(vertices=want["counts"]["kept_vertices"], faces=want["counts"]["kept_faces"], status=0)
    g = MC.canonical(got["indexed"])
    assert MW.same_mesh(g, want["mesh"]) and same_bits(g["normals"], want["mesh"]["normals"])
    # the mesh buffer has the filtered mesh in the download's order
    assert got["mesh"]["vertices"].tobytes() == got["indexed"]["vertices"].tobytes() and same_bits(got["mesh"]["normals"], got["indexed"]["normals"])
    assert np.array_equal(got["mesh"]["faces"], got["indexed"]["faces"])


@pytest.mark.parametrize("part", ["full", "boxed"])
def test_s1_extraction_drops_its_crumbs(scenes, part):
    """S1 64x48 P2: against the restatement on the device's own welded mesh.  Against a vacuous scene: at least 50
    components, minFaces = 100 keeps exactly two and largestOnly one of more than 20 000 faces (the whole scene; the CPU
    oracle's soup of this scene welds into components of 20 715 and 188 faces and 102 of 17 faces or fewer)."""
    x = scenes("S1")
    plain = x[part]
    base = MC.filter(plain)
    print(part, "vertices", len(plain["keys"]), "faces", len(plain["faces"]), base["counts"], "sizes", MC.sizes(base["face_count"])[:12])
    want = MC.filter(plain, 100)
    got = extract_filtered(x, part, 100, False)
    assert_is_the_restatements(got, want)
    one = extract_filtered(x, part, 0, True)
    assert_is_the_restatements(one, MC.filter(plain, 0, True))
    assert one["stats"]["kept_components"] == 1 and one["stats"]["kept_faces"] == one["stats"]["largest_faces"]
    if part == "full":
        assert base["counts"]["components"] >= 50 and want["counts"]["kept_components"] == 2 and one["stats"]["kept_faces"] > 20000
        assert 0 < want["counts"]["kept_faces"] < len(plain["faces"])
    else:
        assert base["counts"]["components"] >= 2 and 0 < want["counts"]["kept_faces"] < len(plain["faces"])


def test_s2_is_one_component_and_the_filter_the_identity(scenes):
    x = scenes("S2")
    plain = x["full"]
    want = MC.filter(plain, 100)
    assert want["counts"]["components"] == 1 and want["counts"]["faceless_vertices"] == 0
    got = extract_filtered(x, "full", 100, False)
    assert_is_the_restatements(got, want)
    c = MC.canonical(plain)
    assert MW.same_mesh(MC.canonical(got["indexed"]), c) and same_bits(MC.canonical(got["indexed"])["normals"], c["normals"])


def test_option_off_leaves_every_output_as_it_was(scenes, tmp_path):
    x = scenes("S1")
    off = x["off"]
    assert set(off["indexed"]) == set(MESH_KEYS) and set(off["mesh"]) == {"vertices", "colors", "faces"} and set(off["stats"].values()) == {0}
    assert set(off["counts"]) == {"vertices", "faces", "status"}
    mc, hd, hpp = x["mc"], x["scene"].getHashData(), x["scene"].getHashParams()
    mc.setIndexedNormals(False)
    try:
        filtered = extract_filtered(x, "full", 100, False)  # on, then off again: nothing of it stays behind
        assert filtered["stats"]["kept_components"] >= 1 and "normals" not in filtered["indexed"]
        mc.extractIsoSurfaceIndexed(hd, hpp)
        ind, mesh = mc.indexed(), mc.mesh()
        assert set(mc.indexed_component_stats().values()) == {0} and mc.indexed_counts() == off["counts"]
        assert set(ind) == set(MESH_KEYS) and set(mesh) == {"vertices", "colors", "faces"}
        assert MW.same_mesh(MW.canonical(ind), MW.canonical(off["indexed"]))
        assert mesh["vertices"].tobytes() == ind["vertices"].tobytes() and np.array_equal(mesh["faces"], ind["faces"])
        path = str(tmp_path / "plain.ply")
        mc.saveMesh(path, None, True)
        props, verts, faces = read_ply(path)
        assert props == ["x", "y", "z", "red", "green", "blue", "alpha"] and len(verts) == len(ind["keys"]) and len(faces) == len(ind["faces"])
        assert verts["p"].tobytes() == ind["vertices"].tobytes() and np.array_equal(faces.astype(np.uint32), ind["faces"])
    finally:
        mc.setIndexedNormals(True)


@pytest.mark.parametrize("with_normals", [True, False])
def test_ply_holds_the_filtered_mesh(scenes, tmp_path, with_normals):
    x = scenes("S1")
    mc, hd, hpp = x["mc"], x["scene"].getHashData(), x["scene"].getHashParams()
    mc.setIndexedNormals(with_normals)
    mc.setIndexedComponentFilter(100, False)
    try:
        mc.extractIsoSurfaceIndexed(hd, hpp)
        ind, stats = mc.indexed(), mc.indexed_component_stats()
        path = str(tmp_path / "filtered.ply")
        mc.saveMesh(path, None, True)
        props, verts, faces = read_ply(path)
        assert ("nx" in props) == with_normals and len(verts) == stats["kept_vertices"] == len(ind["keys"]) and len(faces) == stats["kept_faces"]
        assert 0 < len(verts) < len(x["full"]["keys"])
        assert verts["p"].tobytes() == ind["vertices"].tobytes() and np.array_equal(faces.astype(np.uint32), ind["faces"])
        if with_normals:
            assert verts["n"].tobytes() == ind["normals"].tobytes()
        assert set(mc.indexed_component_stats().values()) == {0}  # saveMesh clears the buffer, the welded mark and the stats
        # copyTrianglesToCPU clears the mark, and the stats with it
        mc.extractIsoSurfaceIndexed(hd, hpp)
        assert mc.indexed_component_stats() == stats
        mc.copyTrianglesToCPU()
        assert set(mc.indexed_component_stats().values()) == {0}
    finally:
        mc.setIndexedNormals(True)
        mc.setIndexedComponentFilter(0, False)
        mc.clearMeshBuffer()


# ---------------------------------------------------------------------------- 4. the accumulating weld

@pytest.fixture(scope="module")
def dealt(vh):
    """the 2 000-triangle soup of tests/test_gpu_mesh_weld_appends.py, and the archipelago, each dealt into 5 appends, with
    the one-shot weld of the whole and its normals"""
    from voxelhashing_amd import engine as E
    out = {}
    for name, (soup, srcs) in (("soup", MW.random_soup(2000, 11, spread=3)), ("archipelago", MC.archipelago())):
        whole = E.mesh_weld(soup, srcs)
        whole["normals"] = E.mesh_vertex_normals(whole["vertices"], whole["keys"], whole["faces"], SCALE)["normals"]
        out[name] = dict(parts=MA.deal(soup, srcs, 5, 11), whole={k: whole[k] for k in MESH_KEYS + ("normals",)}, soup=(soup, srcs))
    return out


@pytest.mark.parametrize("order", [(0, 1, 2, 3, 4), (4, 3, 2, 1, 0), (2, 0, 4, 1, 3)])
@pytest.mark.parametrize("name, min_faces, largest", [("soup", 3, False), ("archipelago", 5, False), ("archipelago", 0, True)])
def test_accumulated_components_are_the_one_shot_welds(vh, dealt, name, min_faces, largest, order):
    """a component split over appends is counted whole, whatever their order"""
    from voxelhashing_amd import engine as E
    d = dealt[name]
    one_shot, want = check_against_restatement(E, d["whole"], min_faces, largest)
    got = E.mesh_weld_appends([d["parts"][i] for i in order], normals_scale_log2=SCALE, min_component_faces=min_faces, largest_component=largest)
    assert got["status"] == 0 and got["component_counts"] == want["counts"] == one_shot["counts"]
    g = MC.canonical(got["filtered"])
    assert MW.same_mesh(g, want["mesh"]) and same_bits(g["normals"], want["mesh"]["normals"])
    assert MW.same_mesh(MW.canonical(got), MW.canonical(d["whole"]))  # the accumulator's own mesh is what it was
    assert 0 < want["counts"]["kept_faces"] <= len(d["whole"]["faces"])


def test_a_component_split_over_two_appends_is_counted_whole(vh):
    from voxelhashing_amd import engine as E
    soup, srcs = MW.random_soup(257, 45, spread=2)  # the archipelago's largest island, its cells dealt to two appends
    parts = MA.deal(soup, srcs, 2, 5, repeat=0.0)
    whole = MC.filter(MW.weld(soup, srcs), 0, True)
    got = E.mesh_weld_appends(parts, min_component_faces=0, largest_component=True)
    halves = [MC.filter(MW.weld(*p), 0, True)["counts"]["largest_faces"] for p in parts]
    assert got["component_counts"] == whole["counts"] and whole["counts"]["largest_faces"] > max(halves) > 0
    assert MW.same_mesh(MC.canonical(got["filtered"]), whole["mesh"]) and "normals" not in got["filtered"]


def test_a_pass_is_stale_after_an_append(vh, dealt):
    from voxelhashing_amd import engine as E
    parts = dealt["soup"]["parts"]
    got = E.mesh_weld_appends(parts[:4], min_component_faces=3, append_after_components=parts[4])
    assert got["component_counts"]["kept_faces"] > 0 and got["stale_code"] == BAD_ARGUMENT
    h = C.c_void_p()
    from voxelhashing_amd import lib
    lib.check(vh.vh_mesh_weld_accum_create(0, 0, 0, C.byref(h)), "create")
    try:
        counts = (C.c_uint32 * 6)(*([7] * 6))
        assert vh.vh_mesh_weld_accum_components_get_counts(h, counts, None) == BAD_ARGUMENT and list(counts) == [7] * 6  # no pass yet
        lib.check(vh.vh_mesh_weld_accum_components(h, 1, 0, None), "components")  # an empty accumulation: nothing launched
        assert vh.vh_mesh_weld_accum_components_get_counts(h, counts, None) == 0 and list(counts) == [0] * 6
        lib.check(vh.vh_mesh_weld_accum_begin(h, None), "begin")
        assert vh.vh_mesh_weld_accum_components_get_counts(h, counts, None) == BAD_ARGUMENT  # a begin makes it stale as well
    finally:
        vh.vh_mesh_weld_accum_destroy(h)


# ---------------------------------------------------------------------------- 5. the chunk grid

def test_chunk_grid_walk_is_the_direct_extraction_filter_on(vh):
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
    plain = direct.indexed()
    sizes = MC.sizes(MC.filter(plain)["face_count"])
    print("96x72: sizes", sizes[:12], "of", len(sizes))
    assert len(sizes) >= 2
    min_faces = int(sizes[1]) + 1  # drops all but the largest: a threshold taken from the restatement of this very mesh
    want = MC.filter(plain, min_faces)
    direct.setIndexedComponentFilter(min_faces, False)
    direct.extractIsoSurfaceIndexed(scene.getHashData(), scene.getHashParams())
    assert direct.indexed_component_stats() == want["counts"] and want["counts"]["kept_components"] >= 1
    grid = E.CUDASceneRepChunkGrid(scene, (1.0, 1.0, 1.0), (9, 9, 9), (-4, -4, -4), 64, True, 4)
    try:
        mc = E.CUDAMarchingCubesHashSDF(mp)
        mc.setIndexedNormals(True)
        mc.setIndexedComponentFilter(min_faces, False)
        mc.extractIsoSurfaceIndexedChunkGrid(grid, (0.0, 0.0, 0.0), 100.0)
        got = dict(indexed=mc.indexed(), mesh=mc.mesh(), counts=mc.indexed_counts(), stats=mc.indexed_component_stats())
        accumulated = mc.indexed_stats()
    finally:
        grid.close()
    assert_is_the_restatements(got, want)
    # the accumulation's own figures stay the unfiltered ones
    assert accumulated["dropped"] > 0 and accumulated["vertices"] == len(plain["keys"]) and accumulated["faces"] == len(plain["faces"])
    assert want["counts"]["kept_faces"] < len(plain["faces"])


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


def test_reconstruction_filters_resident_and_streamed(vh, oracle_lib, tmp_path):
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
    for name, extra in (("resident", "s_streamingEnabled = false;\n"), ("streamed", STREAMING)):
        rec = R.Reconstruction(R.read_app_state((PARAMS + extra).encode()), sens_files=[path])
        assert rec.run() == RN and (rec.chunk_grid is not None) == (name == "streamed")
        extract = rec.extractIsoSurfaceIndexed if name == "streamed" else (lambda *a, **k: rec.extractIsoSurface(*a, indexed=True, **k))
        plain = extract(normals=True)
        assert set(plain) == {"vertices", "colors", "faces", "normals"}  # the option off: the keys it always had
        unfiltered = rec.marching_cubes.indexed()
        base = MC.filter(unfiltered)
        sizes = MC.sizes(base["face_count"])
        print(name, "sizes", sizes[:12], "of", len(sizes))
        ply = str(tmp_path / (name + ".ply"))
        mesh = extract(ply, normals=True, largest_component=True)
        want = MC.filter(unfiltered, 0, True)
        assert mesh["components"] == want["counts"] and want["counts"]["kept_faces"] == int(sizes[0]) > 500
        props, verts, faces = read_ply(ply)
        assert len(verts) == want["counts"]["kept_vertices"] == len(mesh["vertices"]) and len(faces) == want["counts"]["kept_faces"]
        assert verts["p"].tobytes() == mesh["vertices"].tobytes() and verts["n"].tobytes() == mesh["normals"].tobytes()
        # the filtered mesh of the file, by position (the PLY has no keys): the kept vertices of the restatement
        rows = lambda a: np.unique(np.ascontiguousarray(a, dtype="<f4").view("<u4").reshape(-1, 3), axis=0)
        assert np.array_equal(rows(verts["p"]), rows(want["mesh"]["vertices"]))
        with pytest.raises(ValueError):
            rec.extractIsoSurface(min_component_faces=10)  # a soup has no connectivity
        with pytest.raises(ValueError):
            rec.extractIsoSurface(largest_component=True)
        again = extract()  # and the default is without the filter
        assert set(again) == {"vertices", "colors", "faces"} and len(again["vertices"]) == len(unfiltered["keys"])
