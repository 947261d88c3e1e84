"""Taubin smoothing of the indexed mesh on the device ("Mesh smoothing"): the launcher, the pass
inside the indexed extractions, the accumulating weld, the chunk-grid walk, the files and the replay -- the six counts
and the canonical smoothed mesh against the numpy restatement (tests/mesh_smooth.py), bit for bit."""
import ctypes as C

import numpy as np
import pytest

import mesh_cluster as MK
import mesh_components as MC
import mesh_normals as MN
import mesh_smooth as MS
import mesh_weld as MW
import mesh_weld_appends as MA
from helpers import small_config
from test_gpu_mesh_components import PARAMS, STREAMING, RW, RH, RN, read_ply, same_bits
from voxelhashing_amd import synth, vhtypes as T

pytestmark = pytest.mark.gpu

BAD_ARGUMENT, STAGING_OVERFLOW = 4, 2  # VH_ERR_*
SCALE = 21
MAX_TRIANGLES = 1 << 19
MESH_KEYS = ("vertices", "colors", "keys", "faces")
ONE_MINUS_ONE = (65536, -65536)  # lambda | mu = 1 | -1


def run(E, mesh, n, factors=(MS.DEFAULT_LAMBDA_Q16, MS.DEFAULT_MU_Q16), keep=True, scale=SCALE, **kw):
    return E.mesh_smooth(mesh["vertices"], mesh["colors"], mesh["keys"], mesh["faces"], n, keep_boundary=keep, scale_log2=scale, factors_q16=factors, **kw)


def check_against_restatement(E, mesh, n, factors=(MS.DEFAULT_LAMBDA_Q16, MS.DEFAULT_MU_Q16), keep=True, scale=SCALE, **kw):
    """the launcher on `mesh` against MS.smooth, bit for bit -> both"""
    want = MS.smooth(mesh, n, factors[0], factors[1], keep, scale)
    got = run(E, mesh, n, factors, keep, scale, **kw)
    assert got["status"] == 0 == want["status"] and got["code"] == 0
    assert got["counts"] == want["counts"], (got["counts"], want["counts"])
    assert MW.same_mesh(MW.canonical(got), want["mesh"])
    return got, want


@pytest.fixture(scope="module")
def shapes():
    patch, rim = MS.open_patch()
    return dict(sphere=MS.uv_sphere(), patch=patch, rim=rim, soup257=MW.weld(*MW.random_soup(257, 267)))


# ---------------------------------------------------------------------------- 1. the launcher against the restatement

@pytest.mark.parametrize("factors", [(MS.DEFAULT_LAMBDA_Q16, MS.DEFAULT_MU_Q16), ONE_MINUS_ONE])
@pytest.mark.parametrize("n", [0, 1, 21, 22, 257])
def test_launcher_equals_the_restatement(vh, n, factors):
    """random_soup(n, 10 + n) welded on the host: its positions straddle the origin, so d and u take both signs; 63 /
    66 vertices straddle a wave, 257 faces a workgroup.  Nearly every edge of a soup has one face, so the boundary is
    kept once and freed otherwise; then the same faces permuted, every triple rotated, the vertices renumbered."""
    from voxelhashing_amd import engine as E
    mesh = MW.weld(*MW.random_soup(n, 10 + n))
    for iterations in (1, 2, 5):
        for keep in (True, False):
            got, want = check_against_restatement(E, mesh, iterations, factors, keep)
            if n >= 21 and not keep:
                assert want["counts"]["moved"] > len(mesh["keys"]) // 2 and want["counts"]["edges"] > 0
            if iterations == 2:
                again = run(E, MS.renumbered(mesh, n), iterations, factors, keep)
                assert again["counts"] == got["counts"] and MW.same_mesh(MW.canonical(again), want["mesh"])
    if n >= 21:
        assert mesh["vertices"].min() < 0 < mesh["vertices"].max()


def test_a_larger_soup_at_ten_iterations(vh):
    from voxelhashing_amd import engine as E
    mesh = MW.weld(*MW.random_soup(2000, 12, spread=6))
    got, want = check_against_restatement(E, mesh, 10, keep=False)
    assert want["counts"]["moved"] > 1000 and 0 < want["counts"]["boundary_edges"] < want["counts"]["edges"]
    check_against_restatement(E, mesh, 10)


@pytest.mark.parametrize("keep", [True, False])
def test_sphere_and_patch(vh, shapes, keep):
    from voxelhashing_amd import engine as E
    got, want = check_against_restatement(E, shapes["sphere"], 10, keep=keep)
    assert got["counts"]["moved"] == len(shapes["sphere"]["keys"]) and got["counts"]["boundary_edges"] == 0
    patch, rim = shapes["patch"], shapes["rim"]
    got, want = check_against_restatement(E, patch, 10, keep=keep)
    assert got["counts"]["moved"] == (100 if keep else 144) and got["counts"]["boundary_vertices"] == 44
    same = np.all(got["vertices"].view(np.uint32) == patch["vertices"].view(np.uint32), axis=1)  # in the input's order
    assert np.array_equal(same, rim) if keep else not same.any()
    assert got["colors"].tobytes() == patch["colors"].tobytes() and np.array_equal(got["faces"], patch["faces"])


# ---------------------------------------------------------------------------- 2. hand-made cases

def test_hand_made_cases(vh):
    from voxelhashing_amd import engine as E
    from test_mesh_smooth import hand_made
    for name, (mesh, kw, counts, positions) in hand_made().items():
        got, want = check_against_restatement(E, mesh, 1, (kw["lambda_q16"], kw["mu_q16"]), kw.get("keep_boundary", True), kw["scale_log2"])
        if counts is not None:
            assert got["counts"] == dict(counts, status=0), name
        if positions is not None:
            assert got["vertices"].tolist() == [list(map(float, p)) for p in positions], name


def test_64_copies_of_one_face_in_one_wave(vh):
    from voxelhashing_amd import engine as E
    faces = [[(0, 1, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)][i % 4] for i in range(64)]
    mesh = MS.plain_mesh([(0, 0, 0), (4, 0, 0), (0, 4, 0), (9, 9, 9)], faces)
    got, want = check_against_restatement(E, mesh, 3, scale=8)
    assert got["counts"] == dict(moved=3, boundary_vertices=0, isolated_vertices=1, status=0, edges=3, boundary_edges=0)


def test_a_hub_of_exactly_the_largest_degree_and_one_more(vh):
    from voxelhashing_amd import engine as E
    fan = MS.closed_fan(MS.MAX_DEGREE)
    got, want = check_against_restatement(E, fan, 1, ONE_MINUS_ONE, scale=30)
    assert got["counts"] == dict(moved=1, boundary_vertices=MS.MAX_DEGREE, isolated_vertices=0, status=0, edges=2 * MS.MAX_DEGREE, boundary_edges=MS.MAX_DEGREE)
    check_against_restatement(E, fan, 2, keep=False, scale=30)
    fan = MS.closed_fan(MS.MAX_DEGREE + 1)
    assert_refused(run(E, fan, 1, raise_on_status=False), MS.smooth(fan, 1), MS.DEGREE, BAD_ARGUMENT)


# ---------------------------------------------------------------------------- 3. statuses

def assert_refused(got, want, status, code):
    assert got["status"] == status == want["status"] and got["code"] == code
    assert got["counts"] == dict(dict.fromkeys(MS.COUNTS, 0), status=status) == want["counts"]
    assert len(got["keys"]) == 0 and len(got["vertices"]) == 0


def test_a_face_index_out_of_bounds_is_a_status(vh, shapes):
    from voxelhashing_amd import engine as E
    soup = shapes["soup257"]
    f = soup["faces"].copy()
    f[len(f) // 2, 1] = len(soup["keys"])  # an index equal to V in the middle of the list
    mesh = dict(soup, faces=f)
    got = run(E, mesh, 2, raise_on_status=False, guard=64)
    assert_refused(got, MS.smooth(mesh, 2), MS.BAD_INDEX, BAD_ARGUMENT)
    assert len(got["guards"]) == 4 and all(np.all(g == 0xa5a5a5a5) for g in got["guards"])
    with pytest.raises(Exception):
        run(E, mesh, 2)


def test_range_status_at_the_first_scale_the_restatement_reports(vh, shapes):
    from voxelhashing_amd import engine as E
    soup = shapes["soup257"]
    for factors, keep in (((MS.DEFAULT_LAMBDA_Q16, MS.DEFAULT_MU_Q16), True), (ONE_MINUS_ONE, False), ((-65536, -65536), False)):
        first = next(s for s in range(20, 60) if MS.smooth(soup, 2, factors[0], factors[1], keep, s)["status"] != 0)
        print(factors, "first scale with a status", first)
        check_against_restatement(E, soup, 2, factors, keep, first - 1)
        assert_refused(run(E, soup, 2, factors, keep, first, raise_on_status=False), MS.smooth(soup, 2, factors[0], factors[1], keep, first), MS.RANGE, BAD_ARGUMENT)
    # the last pair leaves the range in a half step, not going in
    assert MS.quantise(soup["vertices"], first)[1].all()
    for bad in (np.nan, np.inf, -np.inf):
        v = soup["vertices"].copy()
        v[7, 1] = bad
        mesh = dict(soup, vertices=v)
        assert_refused(run(E, mesh, 2, raise_on_status=False), MS.smooth(mesh, 2), MS.RANGE, BAD_ARGUMENT)


def test_a_full_edge_table_is_a_status_and_the_run_ends(vh, shapes):
    from voxelhashing_amd import engine as E
    soup = shapes["soup257"]
    edges = MS.smooth(soup, 1)["counts"]["edges"]
    log2 = int(np.floor(np.log2(edges - 1)))  # fewer slots than edges
    assert (1 << log2) < edges
    got = run(E, soup, 1, edge_slots_log2=log2, raise_on_status=False)
    assert_refused(got, MS.smooth(soup, 1, edge_slots_log2=log2), MS.TABLE_FULL, STAGING_OVERFLOW)
    # a table of exactly as many slots as there are edges fills to the last slot, and works: a closed strip of 64 edges
    n = 32
    ring = MS.plain_mesh([(np.cos(2 * np.pi * i / n), np.sin(2 * np.pi * i / n), 0.1 * (i % 3)) for i in range(n)], [(i, (i + 1) % n, (i + 2) % n) for i in range(n)])
    assert MS.smooth(ring, 2, keep_boundary=False)["counts"]["edges"] == 64
    check_against_restatement(E, ring, 2, keep=False, edge_slots_log2=6)
    assert_refused(run(E, ring, 2, edge_slots_log2=5, raise_on_status=False), MS.smooth(ring, 2, edge_slots_log2=5), MS.TABLE_FULL, STAGING_OVERFLOW)


def test_no_vertex_and_no_face(vh, shapes):
    from voxelhashing_amd import engine as E
    nothing = dict(vertices=np.zeros((0, 3), np.float32), colors=np.zeros((0, 3), np.float32), keys=np.zeros(0, np.uint64), faces=np.zeros((0, 3), np.uint32))
    got = run(E, nothing, 2)
    assert got["counts"] == dict.fromkeys(MS.COUNTS, 0) and len(got["keys"]) == 0
    faceless = dict(shapes["soup257"], faces=np.zeros((0, 3), np.uint32))
    got, want = check_against_restatement(E, faceless, 2)
    assert got["counts"]["isolated_vertices"] == len(faceless["keys"]) and got["counts"]["moved"] == 0
    assert got["vertices"].tobytes() == faceless["vertices"].tobytes()


# ---------------------------------------------------------------------------- 4. through setIndexedSmoothing

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
        off = dict(indexed=mc.indexed(), mesh=mc.mesh(), counts=mc.indexed_counts(), stats=mc.indexed_smooth_stats(), cluster=mc.indexed_cluster_stats(),
                   accumulated=mc.indexed_stats(), components=mc.indexed_component_stats())
        cx = float(np.median(mc.triangles()["v"]["p"][..., 0]))
        box = ((cx, -10.0, -10.0), (10.0, 10.0, 10.0))
        mc.extractIsoSurfaceIndexed(hd, hpp, box[0], box[1], True)
        boxed = mc.indexed()
        cache[name] = dict(scene=scene, vs=float(hpp.m_virtualVoxelSize), mc=mc, off=off, full=off["indexed"], boxed=boxed, box=box)
        return cache[name]

    return get


def extract_smoothed(x, part, n, m=0, normals=False, min_faces=0, keep=True):
    mc, hd, hpp = x["mc"], x["scene"].getHashData(), x["scene"].getHashParams()
    mc.setIndexedSmoothing(n, keepBoundary=keep)
    mc.setIndexedClustering(m)
    mc.setIndexedNormals(normals)
    mc.setIndexedComponentFilter(min_faces, False)
    try:
        if part == "boxed":
            mc.extractIsoSurfaceIndexed(hd, hpp, x["box"][0], x["box"][1], True)
        else:
            mc.extractIsoSurfaceIndexed(hd, hpp)
        return dict(indexed=mc.indexed(), mesh=mc.mesh(), counts=mc.indexed_counts(), stats=mc.indexed_smooth_stats(), cluster=mc.indexed_cluster_stats(),
                    components=mc.indexed_component_stats())
    finally:
        mc.setIndexedSmoothing(0)
        mc.setIndexedClustering(0)
        mc.setIndexedNormals(False)
        mc.setIndexedComponentFilter(0, False)


def expected(x, part, n, m=0, keep=True):
    """the restatement on the device's own welded mesh: clustered at m first, then smoothed, at the voxel size's scale"""
    scale = MK.default_scale_log2(x["vs"])
    base = MK.cluster(x[part], m, scale)["mesh"] if m else MW.canonical(x[part])
    return base, MS.smooth(base, n, keep_boundary=keep, scale_log2=scale)


@pytest.mark.parametrize("m", [0, 2])
@pytest.mark.parametrize("part", ["full", "boxed"])
@pytest.mark.parametrize("name", ["S1", "S2"])
def test_extraction_smooths_the_scene(scenes, name, part, m):
    x = scenes(name)
    base, want = expected(x, part, 5, m)
    got = extract_smoothed(x, part, 5, m)
    print(name, part, "m", m, want["counts"])
    assert want["status"] == 0 and got["stats"] == want["counts"] and 0 < want["counts"]["moved"] <= len(base["keys"])
    assert MW.same_mesh(MW.canonical(got["indexed"]), want["mesh"])
    assert got["counts"] == dict(vertices=len(base["keys"]), faces=len(base["faces"]), status=0)
    assert got["mesh"]["vertices"].tobytes() == got["indexed"]["vertices"].tobytes() and np.array_equal(got["mesh"]["faces"], got["indexed"]["faces"])
    assert set(got["components"].values()) == {0} and set(got["indexed"]) == set(MESH_KEYS) and (got["cluster"]["faces"] > 0) == bool(m)
    assert not MW.same_mesh(want["mesh"], base)  # something moved


@pytest.mark.parametrize("m", [0, 2])
def test_normals_are_of_the_smoothed_mesh(scenes, m):
    from voxelhashing_amd import engine as E
    x = scenes("S1")
    got = extract_smoothed(x, "full", 5, m, normals=True)
    ind = got["indexed"]
    assert MW.same_mesh(MW.canonical(ind), expected(x, "full", 5, m)[1]["mesh"])
    scale = E.mesh_normals_default_scale_log2(np.float32(2.0) * (np.float32(2 * m) * np.float32(x["vs"]) if m else np.float32(x["vs"])))  # the doubled edge bound
    host = MN.vertex_normals(ind["vertices"], ind["keys"], ind["faces"], scale)
    assert host["status"] == 0 and same_bits(ind["normals"], host["normals"]) and same_bits(got["mesh"]["normals"], ind["normals"])


def test_the_component_filter_works_on_the_smoothed_mesh(scenes):
    x = scenes("S1")
    smoothed = extract_smoothed(x, "full", 5)["indexed"]
    want = MC.filter(smoothed, 20)
    got = extract_smoothed(x, "full", 5, min_faces=20)
    assert got["components"] == want["counts"] and 0 < want["counts"]["kept_faces"] < len(smoothed["faces"])
    assert got["counts"] == dict(vertices=want["counts"]["kept_vertices"], faces=want["counts"]["kept_faces"], status=0)
    assert MW.same_mesh(MW.canonical(got["indexed"]), MW.canonical(want["mesh"]))
    assert got["stats"]["moved"] > 0


def test_option_off_leaves_every_output_as_it_was(scenes, tmp_path):
    x = scenes("S1")
    off = x["off"]
    assert set(off["indexed"]) == set(MESH_KEYS) and set(off["mesh"]) == {"vertices", "colors", "faces"}
    assert set(off["stats"].values()) == {0} and set(off["cluster"].values()) == {0} and set(off["components"].values()) == {0} and set(off["accumulated"].values()) == {0}
    mc, hd, hpp = x["mc"], x["scene"].getHashData(), x["scene"].getHashParams()
    on = extract_smoothed(x, "full", 3)  # on, then off again: nothing of it stays behind
    assert on["stats"]["moved"] > 0
    mc.extractIsoSurfaceIndexed(hd, hpp)
    ind, mesh = mc.indexed(), mc.mesh()
    assert set(mc.indexed_smooth_stats().values()) == {0} and mc.indexed_counts() == off["counts"]
    assert set(ind) == set(MESH_KEYS) and set(mesh) == {"vertices", "colors", "faces"}
    assert MW.same_mesh(MW.canonical(ind), MW.canonical(off["indexed"])) and mesh["vertices"].tobytes() == ind["vertices"].tobytes()
    path = str(tmp_path / "plain.ply")
    mc.saveMesh(path, None, True)
    props, verts, faces = read_ply(path)
    assert props == ["x", "y", "z", "red", "green", "blue", "alpha"] and verts["p"].tobytes() == ind["vertices"].tobytes()
    for bad in (dict(iterations=101), dict(iterations=1, lam=1.5), dict(iterations=1, mu=-1.01)):
        with pytest.raises(Exception):
            mc.setIndexedSmoothing(**bad)


def test_ply_holds_the_smoothed_mesh(scenes, tmp_path):
    x = scenes("S1")
    mc, hd, hpp = x["mc"], x["scene"].getHashData(), x["scene"].getHashParams()
    mc.setIndexedSmoothing(5)
    mc.setIndexedNormals(True)
    try:
        mc.extractIsoSurfaceIndexed(hd, hpp)
        ind, stats = mc.indexed(), mc.indexed_smooth_stats()
        assert stats["moved"] > 0 and MW.same_mesh(MW.canonical(ind), expected(x, "full", 5)[1]["mesh"])
        path = str(tmp_path / "smoothed.ply")
        mc.saveMesh(path, None, True)
        props, verts, faces = read_ply(path)
        assert "nx" in props and len(verts) == len(ind["keys"]) and len(faces) == len(ind["faces"])
        assert verts["p"].tobytes() == ind["vertices"].tobytes() and verts["n"].tobytes() == ind["normals"].tobytes()
        assert np.array_equal(faces.astype(np.uint32), ind["faces"])
        assert set(mc.indexed_smooth_stats().values()) == {0}  # saveMesh clears the buffer, the welded mark and the stats
    finally:
        mc.setIndexedSmoothing(0)
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
def test_accumulated_smoothing_is_the_one_shot_welds(vh, dealt, order):
    from voxelhashing_amd import engine as E
    one_shot, want = check_against_restatement(E, dealt["whole"], 3, keep=False)
    got = E.mesh_weld_appends([dealt["parts"][i] for i in order], smooth_iterations=3, keep_boundary=False, smooth_scale_log2=SCALE, normals_scale_log2=30)
    assert got["status"] == 0 and got["smooth_code"] == 0 and got["smooth_counts"] == want["counts"] and want["counts"]["moved"] > 0
    assert MW.same_mesh(MW.canonical(got["smoothed"]), want["mesh"])
    assert MW.same_mesh(MW.canonical(got), MW.canonical(dealt["whole"]))  # the accumulator's own mesh is what it was
    s = got["smoothed"]  # the normals that follow are of the smoothed mesh, in its order
    host = MN.vertex_normals(s["vertices"], s["keys"], s["faces"], 30)
    assert host["status"] == 0 and got["normals_code"] == 0 and same_bits(got["normals"], host["normals"])
    if order == (0, 1, 2, 3, 4):  # over the clustered mesh when a cluster pass is current
        both = E.mesh_weld_appends([dealt["parts"][i] for i in order], cluster_cells=2, cluster_scale_log2=SCALE, smooth_iterations=3, keep_boundary=False,
                                   smooth_scale_log2=SCALE)
        base = MK.cluster(dealt["whole"], 2, SCALE)["mesh"]
        after = MS.smooth(base, 3, keep_boundary=False, scale_log2=SCALE)
        assert both["smooth_counts"] == after["counts"] and MW.same_mesh(MW.canonical(both["smoothed"]), after["mesh"])


def test_a_pass_is_stale_after_an_append(vh, dealt):
    from voxelhashing_amd import engine as E, lib
    parts = dealt["parts"]
    lam, mu = MS.DEFAULT_LAMBDA_Q16, MS.DEFAULT_MU_Q16
    got = E.mesh_weld_appends(parts[:4], smooth_iterations=2, keep_boundary=False, append_after_smooth=parts[4])
    assert got["smooth_counts"]["moved"] > 0 and got["stale_smooth_code"] == BAD_ARGUMENT
    h = C.c_void_p()
    lib.check(vh.vh_mesh_weld_accum_create(0, 0, 0, C.byref(h)), "create")
    try:
        counts = (C.c_uint32 * 6)(*([7] * 6))
        assert vh.vh_mesh_weld_accum_smooth_get_counts(h, counts, None) == BAD_ARGUMENT and list(counts) == [7] * 6  # no pass yet
        assert vh.vh_mesh_weld_accum_smooth(h, 101, lam, mu, 1, SCALE, None) == BAD_ARGUMENT and vh.vh_mesh_weld_accum_smooth(h, 2, lam, mu, 1, 101, None) == BAD_ARGUMENT
        assert vh.vh_mesh_weld_accum_smooth(h, 2, 65537, mu, 1, SCALE, None) == BAD_ARGUMENT and vh.vh_mesh_weld_accum_smooth(h, 2, lam, mu, 2, SCALE, None) == BAD_ARGUMENT
        lib.check(vh.vh_mesh_weld_accum_smooth(h, 2, lam, mu, 1, SCALE, None), "smooth")  # an empty accumulation: nothing launched
        assert vh.vh_mesh_weld_accum_smooth_get_counts(h, counts, None) == 0 and list(counts) == [0] * 6
        lib.check(vh.vh_mesh_weld_accum_smooth(h, 0, 0, 0, 0, 0, None), "forget")  # N = 0 forgets the pass
        assert vh.vh_mesh_weld_accum_smooth_get_counts(h, counts, None) == BAD_ARGUMENT
        lib.check(vh.vh_mesh_weld_accum_smooth(h, 2, lam, mu, 1, SCALE, None), "smooth")
        lib.check(vh.vh_mesh_weld_accum_cluster(h, 2, SCALE, None), "cluster")  # a later cluster pass makes it stale
        assert vh.vh_mesh_weld_accum_smooth_get_counts(h, counts, None) == BAD_ARGUMENT
        lib.check(vh.vh_mesh_weld_accum_smooth(h, 2, lam, mu, 1, SCALE, None), "smooth")
        lib.check(vh.vh_mesh_weld_accum_begin(h, None), "begin")
        assert vh.vh_mesh_weld_accum_smooth_get_counts(h, counts, None) == BAD_ARGUMENT  # a begin as well
        assert vh.vh_mesh_weld_accum_smooth_download(h, None, 0, None) == BAD_ARGUMENT
    finally:
        vh.vh_mesh_weld_accum_destroy(h)


def test_two_finishes_of_one_accumulation_with_the_option_changed_between(scenes):
    """finishIndexed with smoothing on, then off, then on again, without an append between: each describes its own mesh"""
    from voxelhashing_amd import engine as E
    x = scenes("S1")
    mc, hd, hpp = x["mc"], x["scene"].getHashData(), x["scene"].getHashParams()
    want = expected(x, "full", 4)[1]
    mc.setIndexedNormals(True)
    try:
        mc.beginIndexed()
        mc.appendIndexed(hd, hpp)
        for n in (4, 0, 4):
            mc.setIndexedSmoothing(n)
            mc.finishIndexed()
            ind = mc.indexed()
            if n:
                assert mc.indexed_smooth_stats() == want["counts"] and MW.same_mesh(MW.canonical(ind), want["mesh"])
            else:
                assert set(mc.indexed_smooth_stats().values()) == {0} and MW.same_mesh(MW.canonical(ind), MW.canonical(x["full"]))
            assert len(ind["normals"]) == len(ind["keys"]) == mc.indexed_counts()["vertices"]
            scale = E.mesh_normals_default_scale_log2(np.float32(x["vs"]) * np.float32(2 if n else 1))
            host = MN.vertex_normals(ind["vertices"], ind["keys"], ind["faces"], scale)
            assert host["status"] == 0 and same_bits(ind["normals"], host["normals"])
    finally:
        mc.setIndexedSmoothing(0)
        mc.setIndexedNormals(False)
        mc.clearMeshBuffer()


# ---------------------------------------------------------------------------- 6. the chunk grid

def test_chunk_grid_walk_is_the_direct_extraction_smoothing_on(vh):
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
    want = MS.smooth(plain, 5, scale_log2=MK.default_scale_log2(float(hp.m_virtualVoxelSize)))
    direct.setIndexedSmoothing(5)
    direct.setIndexedNormals(True)
    direct.extractIsoSurfaceIndexed(scene.getHashData(), scene.getHashParams())
    one = direct.indexed()
    assert direct.indexed_smooth_stats() == want["counts"] and MW.same_mesh(MW.canonical(one), want["mesh"])
    grid = E.CUDASceneRepChunkGrid(scene, (1.0, 1.0, 1.0), (9, 9, 9), (-4, -4, -4), 64, True, 4)
    try:
        mc = E.CUDAMarchingCubesHashSDF(mp)
        mc.setIndexedSmoothing(5)
        mc.setIndexedNormals(True)
        mc.extractIsoSurfaceIndexedChunkGrid(grid, (0.0, 0.0, 0.0), 100.0)
        got = dict(indexed=mc.indexed(), mesh=mc.mesh(), counts=mc.indexed_counts(), stats=mc.indexed_smooth_stats())
        accumulated = mc.indexed_stats()
    finally:
        grid.close()
    assert got["stats"] == want["counts"] and got["counts"] == dict(vertices=len(plain["keys"]), faces=len(plain["faces"]), status=0)
    assert MW.same_mesh(MW.canonical(got["indexed"]), want["mesh"])
    order = lambda m: np.argsort(m["keys"], kind="stable")
    assert same_bits(got["indexed"]["normals"][order(got["indexed"])], one["normals"][order(one)])
    assert got["mesh"]["vertices"].tobytes() == got["indexed"]["vertices"].tobytes() and same_bits(got["mesh"]["normals"], got["indexed"]["normals"])
    assert accumulated["dropped"] > 0 and accumulated["vertices"] == len(plain["keys"]) and accumulated["faces"] == len(plain["faces"])


# ---------------------------------------------------------------------------- 7. Reconstruction

def test_reconstruction_smooths_resident_and_streamed(vh, oracle_lib, tmp_path):
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
        scale = MK.default_scale_log2(0.02)
        base = MK.cluster(welded, 3, scale)["mesh"]
        want = MS.smooth(base, 5, scale_log2=scale)
        ply = str(tmp_path / (name + ".ply"))
        mesh = extract(ply, cluster_cells=3, smooth_iterations=5)
        assert set(mesh) == {"vertices", "colors", "faces", "clustering", "smoothing"} and mesh["smoothing"] == want["counts"] and want["counts"]["moved"] > 0
        props, verts, faces = read_ply(ply)
        assert len(verts) == len(base["keys"]) == len(mesh["vertices"]) and len(faces) == len(base["faces"])
        assert verts["p"].tobytes() == mesh["vertices"].tobytes() and np.array_equal(faces.astype(np.uint32), mesh["faces"])
        rows = lambda a: np.unique(np.ascontiguousarray(a, dtype="<f4").view("<u4").reshape(-1, 3), axis=0)
        assert np.array_equal(rows(verts["p"]), rows(want["mesh"]["vertices"]))
        with pytest.raises(ValueError):
            rec.extractIsoSurface(smooth_iterations=2)  # a soup has no neighbours
        again = extract()  # and the default is without it
        assert set(again) == {"vertices", "colors", "faces"} and len(again["vertices"]) == len(welded["keys"])
