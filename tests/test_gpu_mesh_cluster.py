"""Vertex clustering of the indexed mesh on the device ("Mesh clustering"): the launcher, the pass
inside the indexed extractions, the accumulating weld, the chunk-grid walk, the files and the replay -- the six counts
and the canonical clustered mesh against the numpy restatement (tests/mesh_cluster.py), bit for bit."""
import ctypes as C

import numpy as np
import pytest

import mesh_cluster as MK
import mesh_normals as MN
import mesh_components as MC
import mesh_weld as MW
import mesh_weld_appends as MA
from helpers import small_config
from test_gpu_mesh_components import PARAMS, STREAMING, RW, RH, RN, read_ply, same_bits, shuffled_faces
from voxelhashing_amd import synth, vhtypes as T

pytestmark = pytest.mark.gpu

BAD_ARGUMENT, STAGING_OVERFLOW = 4, 2  # VH_ERR_*
SCALE = 21
MAX_TRIANGLES = 1 << 19
MESH_KEYS = ("vertices", "colors", "keys", "faces")
K = lambda L, code=3: int(MK.pack_point(np.array(L, dtype=np.int64), code))


def run(E, mesh, m, scale=SCALE, **kw):
    return E.mesh_cluster(mesh["vertices"], mesh["colors"], mesh["keys"], mesh["faces"], m, scale, **kw)


def check_against_restatement(E, mesh, m, scale=SCALE):
    """the launcher on `mesh` against MK.cluster, bit for bit -> both"""
    want = MK.cluster(mesh, m, scale)
    got = run(E, mesh, m, scale)
    assert got["status"] == 0 == want["status"] and got["code"] == 0
    assert got["counts"] == want["counts"], (got["counts"], want["counts"])
    assert MW.same_mesh(MW.canonical(got), want["mesh"])
    return got, want


# ---------------------------------------------------------------------------- 1. the launcher against the restatement

@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("n", [0, 1, 21, 22, 257])
def test_launcher_equals_the_restatement(vh, n, m):
    """random_soup(n, 10 + n) welded on the host: its cells lie in [-3, 3)^3, so the lattice straddles the origin and
    negative L meets floor division; 63 / 66 vertices straddle a wave, 257 faces a workgroup"""
    from voxelhashing_amd import engine as E
    mesh = MW.weld(*MW.random_soup(n, 10 + n))
    got, want = check_against_restatement(E, mesh, m)
    if n >= 21:
        assert MK.lattice(mesh["keys"]).min() < 0 < MK.lattice(mesh["keys"]).max()
        assert want["counts"]["faces"] + want["counts"]["collapsed"] + want["counts"]["duplicates"] == len(mesh["faces"])
    if n == 257 and m > 1:
        assert want["counts"]["collapsed"] > 0 and want["counts"]["duplicates"] > 0 and 0 < want["counts"]["faces"] < len(mesh["faces"])
    # the same faces permuted, with every triple rotated: the same mesh
    again = run(E, dict(mesh, faces=shuffled_faces(mesh["faces"], n)), m)
    assert again["counts"] == got["counts"] and MW.same_mesh(MW.canonical(again), MW.canonical(got))


def test_order_independence_is_shown(vh):
    """the 257-triangle case twice: vertices renumbered and faces permuted and rotated the second time, so that every
    atomic runs in another order -- the canonical results are identical"""
    from voxelhashing_amd import engine as E
    m = MW.weld(*MW.random_soup(257, 267))
    first = run(E, m, 2)
    rng = np.random.default_rng(5)
    p = rng.permutation(len(m["keys"]))
    inv = np.empty_like(p)
    inv[p] = np.arange(len(p))
    other = dict(vertices=m["vertices"][p], colors=m["colors"][p], keys=m["keys"][p], faces=shuffled_faces(inv[m["faces"].astype(np.int64)].astype(np.uint32), 9))
    second = run(E, other, 2)
    assert first["counts"] == second["counts"] and first["counts"]["vertices"] > 0
    assert MW.same_mesh(MW.canonical(first), MW.canonical(second))


def test_a_larger_soup_at_m_4(vh):
    from voxelhashing_amd import engine as E
    got, want = check_against_restatement(E, MW.weld(*MW.random_soup(2000, 12, spread=6)), 4)
    assert want["counts"]["vertices"] > 20 and want["counts"]["duplicates"] > 0


def test_keys_at_both_ends_of_the_range(vh):
    from voxelhashing_amd import engine as E
    B = 1 << 19
    keys = [K((-B, -B, -B)), K((-B + 1, -B, -B), 0), K((B - 1, B - 1, B - 1)), K((B - 2, B - 1, B - 1), 1), K((0, 0, 0)), K((-1, -1, -1), 2), K((B - 1, -B, 0))]
    v = MK.lattice(np.array(keys, dtype=np.uint64)).astype(np.float32) * np.float32(0.04)
    mesh = MK.plain_mesh(keys, [(0, 2, 4), (1, 3, 5), (4, 5, 6), (0, 6, 2)], vertices=v)
    for m in (1, 2, 3, 64):
        got, want = check_against_restatement(E, mesh, m)
        assert want["counts"]["vertices"] >= 3


# ---------------------------------------------------------------------------- 2. hand-made duplicates and collapses

def test_hand_made_cases(vh):
    from voxelhashing_amd import engine as E
    from test_mesh_cluster import hand_made
    for name, (mesh, m, counts, _) in hand_made().items():
        got, want = check_against_restatement(E, mesh, m, 16)
        assert got["counts"] == dict(counts, status=0), name


def test_64_copies_of_one_face_in_one_wave(vh):
    from voxelhashing_amd import engine as E
    keys = [K((0, 0, 0)), K((2, 0, 0)), K((0, 2, 0))]
    faces = [[(0, 1, 2), (1, 2, 0), (2, 0, 1)][i % 3] for i in range(64)]
    got, want = check_against_restatement(E, MK.plain_mesh(keys, faces), 2, 16)
    assert got["counts"] == dict(vertices=3, faces=1, status=0, collapsed=0, duplicates=63, unused_clusters=0)
    mixed = [(0, 1, 2) if i % 2 else (0, 2, 1) for i in range(64)]  # both windings, many times: (A, B, C) stays
    got, want = check_against_restatement(E, MK.plain_mesh(keys, mixed), 2, 16)
    a, b, c = K((0, 0, 0)), K((1, 0, 0)), K((0, 1, 0))  # the three clusters' keys, ascending
    assert got["counts"]["duplicates"] == 63 and got["keys"][got["faces"][0].astype(np.int64)].tolist() in ([a, b, c], [b, c, a], [c, a, b])


def test_a_fan_whose_faces_share_two_clusters(vh):
    """every face is (A, B, rim): the pair word of the face table is the same for all, the third word tells them apart"""
    from voxelhashing_amd import engine as E
    rim = [K((2 * i, 10, 4)) for i in range(100)]
    keys = [K((0, 0, 0)), K((2, 0, 0))] + rim
    faces = [(0, 1, 2 + i) for i in range(100)] + [(1, 0, 2 + i) for i in range(0, 100, 2)]
    got, want = check_against_restatement(E, MK.plain_mesh(keys, faces), 2, 16)
    assert got["counts"] == dict(vertices=102, faces=100, status=0, collapsed=0, duplicates=50, unused_clusters=0)


# ---------------------------------------------------------------------------- 3. statuses

@pytest.fixture(scope="module")
def soup257():
    return MW.weld(*MW.random_soup(257, 267))


def assert_refused(got, want, status, code):
    assert got["status"] == status == want["status"] and got["code"] == code
    assert got["counts"] == dict(dict.fromkeys(MK.COUNTS, 0), status=status) == want["counts"]
    assert len(got["keys"]) == 0 and len(got["faces"]) == 0


def test_a_face_index_out_of_bounds_is_a_status(vh, soup257):
    from voxelhashing_amd import engine as E
    f = soup257["faces"].copy()
    f[len(f) // 2, 1] = len(soup257["keys"])  # an index equal to V in the middle of the list
    mesh = dict(soup257, faces=f)
    got = run(E, mesh, 2, raise_on_status=False, guard=64)
    assert_refused(got, MK.cluster(mesh, 2, SCALE), MK.BAD_INDEX, BAD_ARGUMENT)
    assert np.all(got["slot_guard"] == 0xa5a5a5a5)
    with pytest.raises(Exception):
        run(E, mesh, 2)


def test_a_key_that_is_no_vertex_key_is_a_status(vh, soup257):
    from voxelhashing_amd import engine as E
    k = soup257["keys"].copy()
    k[len(k) // 2] |= np.uint64(1 << 62)
    mesh = dict(soup257, keys=k)
    assert_refused(run(E, mesh, 2, raise_on_status=False), MK.cluster(mesh, 2, SCALE), MK.BAD_KEY, BAD_ARGUMENT)


def test_range_status_at_the_first_scale_the_restatement_reports(vh, soup257):
    from voxelhashing_amd import engine as E
    first = next(s for s in range(20, 60) if MK.cluster(soup257, 2, s)["status"] != 0)
    assert MK.cluster(soup257, 2, first - 1)["status"] == 0
    check_against_restatement(E, soup257, 2, first - 1)
    assert_refused(run(E, soup257, 2, first, raise_on_status=False), MK.cluster(soup257, 2, first), MK.RANGE, BAD_ARGUMENT)
    for bad in (np.nan, np.inf, -np.inf):
        v = soup257["vertices"].copy()
        v[7, 1] = bad
        mesh = dict(soup257, vertices=v)
        assert_refused(run(E, mesh, 2, raise_on_status=False), MK.cluster(mesh, 2, SCALE), MK.RANGE, BAD_ARGUMENT)
    c = soup257["colors"].copy()
    c[3, 2] = np.nan
    assert_refused(run(E, dict(soup257, colors=c), 2, raise_on_status=False), MK.cluster(dict(soup257, colors=c), 2, SCALE), MK.RANGE, BAD_ARGUMENT)


def test_full_tables_are_a_status_and_the_run_ends(vh, soup257):
    from voxelhashing_amd import engine as E
    base = MK.cluster(soup257, 2, SCALE)
    clusters = base["counts"]["vertices"] + base["counts"]["unused_clusters"]
    log2 = int(np.floor(np.log2(clusters - 1)))  # fewer slots than clusters
    assert (1 << log2) < clusters
    got = run(E, soup257, 2, cluster_slots_log2=log2, raise_on_status=False)
    assert_refused(got, MK.cluster(soup257, 2, SCALE, cluster_slots_log2=log2), MK.TABLE_FULL, STAGING_OVERFLOW)
    distinct = base["counts"]["faces"]
    log2 = int(np.floor(np.log2(distinct - 1)))  # fewer face slots than distinct faces
    got = run(E, soup257, 2, face_slots_log2=log2, raise_on_status=False)
    assert_refused(got, MK.cluster(soup257, 2, SCALE, face_slots_log2=log2), MK.TABLE_FULL, STAGING_OVERFLOW)
    # a table of exactly as many slots as there are keys fills to the last slot, and works
    keys = [K((2 * i, 0, 0)) for i in range(64)]
    faces = [(i, i + 1, i + 2) for i in range(62)] + [(62, 63, 0), (63, 0, 1)]
    check = run(E, MK.plain_mesh(keys, faces), 2, 16, cluster_slots_log2=6, face_slots_log2=6)
    assert check["counts"] == MK.cluster(MK.plain_mesh(keys, faces), 2, 16, 6, 6)["counts"] and check["counts"]["faces"] == 64


def test_no_vertex_and_no_face(vh, soup257):
    from voxelhashing_amd import engine as E
    nothing = dict(vertices=np.zeros((0, 3), np.float32), colors=np.zeros((0, 3), np.float32), keys=np.zeros(0, np.uint64), faces=np.zeros((0, 3), np.uint32))
    got = run(E, nothing, 2)
    assert got["counts"] == dict.fromkeys(MK.COUNTS, 0) and len(got["keys"]) == 0
    faceless = dict(soup257, faces=np.zeros((0, 3), np.uint32))
    got, want = check_against_restatement(E, faceless, 2)
    assert got["counts"]["vertices"] == 0 and got["counts"]["unused_clusters"] > 0


# ---------------------------------------------------------------------------- 4. through setIndexedClustering

SCENES = {"S1": (64, 48, "P2", "S1"), "S2": (80, 60, "P4", "S2")}


@pytest.fixture(scope="module")
def scenes(vh):
    """name -> the scene (three orbit frames), an extractor, its welded mesh whole and boxed with the option off"""
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
        off = dict(indexed=mc.indexed(), mesh=mc.mesh(), counts=mc.indexed_counts(), stats=mc.indexed_cluster_stats(), accumulated=mc.indexed_stats(),
                   components=mc.indexed_component_stats())
        cx = float(np.median(mc.triangles()["v"]["p"][..., 0]))
        box = ((cx, -10.0, -10.0), (10.0, 10.0, 10.0))
        mc.extractIsoSurfaceIndexed(hd, hpp, box[0], box[1], True)
        boxed = mc.indexed()
        cache[name] = dict(scene=scene, vs=float(hpp.m_virtualVoxelSize), mc=mc, off=off, full=off["indexed"], boxed=boxed, box=box)
        return cache[name]

    return get


def extract_clustered(x, part, m, normals=False, min_faces=0):
    mc, hd, hpp = x["mc"], x["scene"].getHashData(), x["scene"].getHashParams()
    mc.setIndexedClustering(m)
    mc.setIndexedNormals(normals)
    mc.setIndexedComponentFilter(min_faces, False)
    try:
        if part == "boxed":
            mc.extractIsoSurfaceIndexed(hd, hpp, x["box"][0], x["box"][1], True)
        else:
            mc.extractIsoSurfaceIndexed(hd, hpp)
        return dict(indexed=mc.indexed(), mesh=mc.mesh(), counts=mc.indexed_counts(), stats=mc.indexed_cluster_stats(), components=mc.indexed_component_stats())
    finally:
        mc.setIndexedClustering(0)
        mc.setIndexedNormals(False)
        mc.setIndexedComponentFilter(0, False)


@pytest.mark.parametrize("part", ["full", "boxed"])
@pytest.mark.parametrize("m", [2, 4])
@pytest.mark.parametrize("name", ["S1", "S2"])
def test_extraction_clusters_the_scene(scenes, name, m, part):
    """against the restatement run on the device's own welded mesh, at the default scale of the voxel size"""
    x = scenes(name)
    plain = x[part]
    want = MK.cluster(plain, m, MK.default_scale_log2(x["vs"]))
    got = extract_clustered(x, part, m)
    print(name, part, "m", m, "vertices", len(plain["keys"]), "->", want["counts"]["vertices"], "faces", len(plain["faces"]), "->", want["counts"]["faces"], want["counts"])
    assert got["stats"] == want["counts"] and want["status"] == 0
    assert got["counts"] == dict(vertices=want["counts"]["vertices"], faces=want["counts"]["faces"], status=0)
    assert MW.same_mesh(MW.canonical(got["indexed"]), want["mesh"])
    assert got["mesh"]["vertices"].tobytes() == got["indexed"]["vertices"].tobytes() and np.array_equal(got["mesh"]["faces"], got["indexed"]["faces"])
    assert set(got["components"].values()) == {0} and set(got["indexed"]) == set(MESH_KEYS)
    # a decimation: a surface crosses about m^2 cells of a cluster's m^3, so about 1 / m^2 <= 1 / 4 of the faces stay; half is generous
    assert 0 < want["counts"]["faces"] < len(plain["faces"]) // 2 and 0 < want["counts"]["vertices"] < len(plain["keys"]) // 2
    # every representative lies in its cluster's box (the extraction's vertices lie on their lattice edges)
    k, r = MK.lattice(want["mesh"]["keys"]).astype(np.float64), want["mesh"]["vertices"].astype(np.float64)
    slack = 2.0 ** -MK.default_scale_log2(x["vs"]) + 2.0 ** -22 * (np.abs(r) + x["vs"] * m)
    assert np.all(r >= (k * m - 0.5) * x["vs"] - slack) and np.all(r <= (k * m + m - 0.5) * x["vs"] + slack)


@pytest.mark.parametrize("m", [2, 4])
def test_normals_are_of_the_clustered_mesh(scenes, m):
    from voxelhashing_amd import engine as E
    x = scenes("S1")
    got = extract_clustered(x, "full", m, normals=True)
    ind = got["indexed"]
    want = MK.cluster(x["full"], m, MK.default_scale_log2(x["vs"]))
    assert MW.same_mesh(MW.canonical(ind), want["mesh"])
    scale = E.mesh_normals_default_scale_log2(2.0 * m * np.float32(x["vs"]))
    host = MN.vertex_normals(ind["vertices"], ind["keys"], ind["faces"], scale)
    assert host["status"] == 0 and same_bits(ind["normals"], host["normals"]) and same_bits(got["mesh"]["normals"], ind["normals"])


def test_the_component_filter_works_on_the_clustered_mesh(scenes):
    x = scenes("S1")
    clustered = extract_clustered(x, "full", 2)["indexed"]
    want = MC.filter(clustered, 20)
    got = extract_clustered(x, "full", 2, min_faces=20)
    assert got["components"] == want["counts"] and 0 < want["counts"]["kept_faces"] < len(clustered["faces"])
    assert got["counts"] == dict(vertices=want["counts"]["kept_vertices"], faces=want["counts"]["kept_faces"], status=0)
    assert MW.same_mesh(MW.canonical(got["indexed"]), MW.canonical(want["mesh"]))
    assert got["stats"]["faces"] == len(clustered["faces"])  # the clustering's own figures stay those of its pass


def test_option_off_leaves_every_output_as_it_was(scenes, tmp_path):
    x = scenes("S1")
    off = x["off"]
    assert set(off["indexed"]) == set(MESH_KEYS) and set(off["mesh"]) == {"vertices", "colors", "faces"}
    assert set(off["stats"].values()) == {0} and set(off["components"].values()) == {0} and set(off["accumulated"].values()) == {0}
    mc, hd, hpp = x["mc"], x["scene"].getHashData(), x["scene"].getHashParams()
    on = extract_clustered(x, "full", 2)  # on, then off again: nothing of it stays behind
    assert on["stats"]["faces"] > 0
    mc.extractIsoSurfaceIndexed(hd, hpp)
    ind, mesh = mc.indexed(), mc.mesh()
    assert set(mc.indexed_cluster_stats().values()) == {0} and mc.indexed_counts() == off["counts"]
    assert set(ind) == set(MESH_KEYS) and set(mesh) == {"vertices", "colors", "faces"}
    assert MW.same_mesh(MW.canonical(ind), MW.canonical(off["indexed"]))
    path = str(tmp_path / "plain.ply")
    mc.saveMesh(path, None, True)
    props, verts, faces = read_ply(path)
    assert props == ["x", "y", "z", "red", "green", "blue", "alpha"] and len(verts) == len(ind["keys"]) and len(faces) == len(ind["faces"])
    assert verts["p"].tobytes() == ind["vertices"].tobytes() and np.array_equal(faces.astype(np.uint32), ind["faces"])
    with pytest.raises(Exception):
        mc.setIndexedClustering(65)


def test_ply_holds_the_clustered_mesh(scenes, tmp_path):
    x = scenes("S1")
    mc, hd, hpp = x["mc"], x["scene"].getHashData(), x["scene"].getHashParams()
    mc.setIndexedClustering(2)
    mc.setIndexedNormals(True)
    try:
        mc.extractIsoSurfaceIndexed(hd, hpp)
        ind, stats = mc.indexed(), mc.indexed_cluster_stats()
        path = str(tmp_path / "clustered.ply")
        mc.saveMesh(path, None, True)
        props, verts, faces = read_ply(path)
        assert "nx" in props and len(verts) == stats["vertices"] == len(ind["keys"]) and len(faces) == stats["faces"] == len(ind["faces"])
        assert verts["p"].tobytes() == ind["vertices"].tobytes() and verts["n"].tobytes() == ind["normals"].tobytes()
        assert np.array_equal(faces.astype(np.uint32), ind["faces"])
        assert set(mc.indexed_cluster_stats().values()) == {0}  # saveMesh clears the buffer, the welded mark and the stats
    finally:
        mc.setIndexedClustering(0)
        mc.setIndexedNormals(False)
        mc.clearMeshBuffer()


# ---------------------------------------------------------------------------- 5. the accumulating weld

@pytest.fixture(scope="module")
def dealt(vh):
    """the 2 000-triangle soup of tests/test_gpu_mesh_weld_appends.py dealt into 5 appends, and the one-shot weld of the whole"""
    from voxelhashing_amd import engine as E
    soup, srcs = MW.random_soup(2000, 11, spread=3)
    whole = E.mesh_weld(soup, srcs)
    return dict(parts=MA.deal(soup, srcs, 5, 11), whole={k: whole[k] for k in MESH_KEYS})


@pytest.mark.parametrize("order", [(0, 1, 2, 3, 4), (4, 3, 2, 1, 0), (2, 0, 4, 1, 3)])
def test_accumulated_clustering_is_the_one_shot_welds(vh, dealt, order):
    from voxelhashing_amd import engine as E
    one_shot, want = check_against_restatement(E, dealt["whole"], 2)
    got = E.mesh_weld_appends([dealt["parts"][i] for i in order], cluster_cells=2, cluster_scale_log2=SCALE, normals_scale_log2=30)
    assert got["status"] == 0 and got["cluster_code"] == 0 and got["cluster_counts"] == want["counts"] and want["counts"]["faces"] > 0
    assert MW.same_mesh(MW.canonical(got["clustered"]), want["mesh"])
    assert MW.same_mesh(MW.canonical(got), MW.canonical(dealt["whole"]))  # the accumulator's own mesh is what it was
    c = got["clustered"]  # the normals that follow are of the clustered mesh, in its order
    host = MN.vertex_normals(c["vertices"], c["keys"], c["faces"], 30)
    assert host["status"] == 0 and got["normals_code"] == 0 and same_bits(got["normals"], host["normals"])


def test_a_pass_is_stale_after_an_append(vh, dealt):
    from voxelhashing_amd import engine as E, lib
    parts = dealt["parts"]
    got = E.mesh_weld_appends(parts[:4], cluster_cells=2, cluster_scale_log2=SCALE, append_after_cluster=parts[4])
    assert got["cluster_counts"]["faces"] > 0 and got["stale_cluster_code"] == BAD_ARGUMENT
    h = C.c_void_p()
    lib.check(vh.vh_mesh_weld_accum_create(0, 0, 0, C.byref(h)), "create")
    try:
        counts = (C.c_uint32 * 6)(*([7] * 6))
        assert vh.vh_mesh_weld_accum_cluster_get_counts(h, counts, None) == BAD_ARGUMENT and list(counts) == [7] * 6  # no pass yet
        assert vh.vh_mesh_weld_accum_cluster(h, 65, SCALE, None) == BAD_ARGUMENT and vh.vh_mesh_weld_accum_cluster(h, 2, 101, None) == BAD_ARGUMENT
        lib.check(vh.vh_mesh_weld_accum_cluster(h, 2, SCALE, None), "cluster")  # an empty accumulation: nothing launched
        assert vh.vh_mesh_weld_accum_cluster_get_counts(h, counts, None) == 0 and list(counts) == [0] * 6
        lib.check(vh.vh_mesh_weld_accum_cluster(h, 0, 0, None), "forget")  # m = 0 forgets the pass
        assert vh.vh_mesh_weld_accum_cluster_get_counts(h, counts, None) == BAD_ARGUMENT
        lib.check(vh.vh_mesh_weld_accum_cluster(h, 2, SCALE, None), "cluster")
        lib.check(vh.vh_mesh_weld_accum_begin(h, None), "begin")
        assert vh.vh_mesh_weld_accum_cluster_get_counts(h, counts, None) == BAD_ARGUMENT  # a begin makes it stale as well
        assert vh.vh_mesh_weld_accum_cluster_download(h, None, None, None, 0, 0, None) == BAD_ARGUMENT
    finally:
        vh.vh_mesh_weld_accum_destroy(h)


def test_two_finishes_of_one_accumulation_with_the_option_changed_between(scenes):
    """finishIndexed with clustering on, then off, then on again, without an append between: each describes its own mesh"""
    x = scenes("S1")
    mc, hd, hpp = x["mc"], x["scene"].getHashData(), x["scene"].getHashParams()
    want = MK.cluster(x["full"], 2, MK.default_scale_log2(x["vs"]))
    mc.setIndexedNormals(True)
    try:
        mc.beginIndexed()
        mc.appendIndexed(hd, hpp)
        for m in (2, 0, 2):
            mc.setIndexedClustering(m)
            mc.finishIndexed()
            ind = mc.indexed()
            if m:
                assert mc.indexed_cluster_stats() == want["counts"] and MW.same_mesh(MW.canonical(ind), want["mesh"])
            else:
                assert set(mc.indexed_cluster_stats().values()) == {0} and MW.same_mesh(MW.canonical(ind), MW.canonical(x["full"]))
            assert len(ind["normals"]) == len(ind["keys"]) == mc.indexed_counts()["vertices"]
            host = MN.vertex_normals(ind["vertices"], ind["keys"], ind["faces"], E_scale(x["vs"], m))
            assert host["status"] == 0 and same_bits(ind["normals"], host["normals"])
    finally:
        mc.setIndexedClustering(0)
        mc.setIndexedNormals(False)
        mc.clearMeshBuffer()


def E_scale(vs, m):
    """the normals' scale of an extraction at that voxel size, clustering at m or off"""
    from voxelhashing_amd import engine as E
    return E.mesh_normals_default_scale_log2(np.float32(vs) * np.float32(2 * m if m else 1))


# ---------------------------------------------------------------------------- 6. the chunk grid

def test_chunk_grid_walk_is_the_direct_extraction_clustering_on(vh):
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
    direct.extractIsoSurfaceIndexed(scene.getHashData(), scene.getHashParams())
    plain = direct.indexed()
    want = MK.cluster(plain, 2, MK.default_scale_log2(float(hp.m_virtualVoxelSize)))
    direct.setIndexedClustering(2)
    direct.setIndexedNormals(True)
    direct.extractIsoSurfaceIndexed(scene.getHashData(), scene.getHashParams())
    one = direct.indexed()
    assert direct.indexed_cluster_stats() == want["counts"] and MW.same_mesh(MW.canonical(one), want["mesh"])
    grid = E.CUDASceneRepChunkGrid(scene, (1.0, 1.0, 1.0), (9, 9, 9), (-4, -4, -4), 64, True, 4)
    try:
        mc = E.CUDAMarchingCubesHashSDF(mp)
        mc.setIndexedClustering(2)
        mc.setIndexedNormals(True)
        mc.extractIsoSurfaceIndexedChunkGrid(grid, (0.0, 0.0, 0.0), 100.0)
        got = dict(indexed=mc.indexed(), mesh=mc.mesh(), counts=mc.indexed_counts(), stats=mc.indexed_cluster_stats())
        accumulated = mc.indexed_stats()
    finally:
        grid.close()
    assert got["stats"] == want["counts"] and got["counts"] == dict(vertices=want["counts"]["vertices"], faces=want["counts"]["faces"], status=0)
    assert MW.same_mesh(MW.canonical(got["indexed"]), want["mesh"])
    order = lambda m: np.argsort(m["keys"], kind="stable")
    assert same_bits(got["indexed"]["normals"][order(got["indexed"])], one["normals"][order(one)])
    assert got["mesh"]["vertices"].tobytes() == got["indexed"]["vertices"].tobytes() and same_bits(got["mesh"]["normals"], got["indexed"]["normals"])
    # the accumulation's own figures stay the welded ones
    assert accumulated["dropped"] > 0 and accumulated["vertices"] == len(plain["keys"]) and accumulated["faces"] == len(plain["faces"])


# ---------------------------------------------------------------------------- 7. Reconstruction

def test_reconstruction_clusters_resident_and_streamed(vh, oracle_lib, tmp_path):
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
        plain = extract()
        assert set(plain) == {"vertices", "colors", "faces"}  # the option off: the keys it always had
        welded = rec.marching_cubes.indexed()
        want = MK.cluster(welded, 3, MK.default_scale_log2(0.02))
        ply = str(tmp_path / (name + ".ply"))
        mesh = extract(ply, cluster_cells=3)
        assert set(mesh) == {"vertices", "colors", "faces", "clustering"} and mesh["clustering"] == want["counts"]
        assert 0 < want["counts"]["faces"] < len(welded["faces"]) // 3
        props, verts, faces = read_ply(ply)
        assert len(verts) == want["counts"]["vertices"] == len(mesh["vertices"]) and len(faces) == want["counts"]["faces"]
        assert verts["p"].tobytes() == mesh["vertices"].tobytes() and np.array_equal(faces.astype(np.uint32), mesh["faces"])
        rows = lambda a: np.unique(np.ascontiguousarray(a, dtype="<f4").view("<u4").reshape(-1, 3), axis=0)
        assert np.array_equal(rows(verts["p"]), rows(want["mesh"]["vertices"]))
        with pytest.raises(ValueError):
            rec.extractIsoSurface(cluster_cells=2)  # a soup has no keys
        again = extract()  # and the default is without it
        assert set(again) == {"vertices", "colors", "faces"} and len(again["vertices"]) == len(welded["keys"])
