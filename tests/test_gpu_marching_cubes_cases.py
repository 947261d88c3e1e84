"""Marching cubes on crafted voxel fields (tests/mc_fields.py), GPU side: k_mc_pass2, plain and sourced, the weld and
the vertex normals against the oracle and the numpy restatements on fields that reach all 254 cube cases, the
edge-mask-255 rule, threshold decisions at their rounding edge, the 2^20 cut-off of the own-voxel short cut, blocks
with missing neighbours, unobserved taps, snapped vertices, neighbour look-ups off collision lists, box faces through
cell centres and triangle buffers that end anywhere.

State comes from LauncherScene.stream_in beside OracleScene.stream_in and is compared first; every field is 64 blocks
or fewer.  tests/test_marching_cubes_cases.py holds the oracle to a float64 restatement on the same fields."""
import ctypes as C

import numpy as np
import pytest

import mc_fields as F
import mesh_normals as MN
import mesh_weld as MW
from voxelhashing_amd import canonical, vhtypes as T

pytestmark = pytest.mark.gpu

f32 = np.float32
PATTERN = 0xA5


@pytest.fixture(scope="module")
def E(vh):
    from voxelhashing_amd import engine
    return engine


def rows(tris):
    return np.sort(np.ascontiguousarray(tris).view(np.dtype((np.void, T.TRIANGLE_DTYPE.itemsize))).ravel())


def same_set(a, b):
    return len(a) == len(b) and np.array_equal(rows(a), rows(b))


def counted(tris):
    """{the bytes of a triangle: how often the soup has it}"""
    from collections import Counter
    b, size = np.ascontiguousarray(tris).tobytes(), T.TRIANGLE_DTYPE.itemsize
    return Counter(b[i:i + size] for i in range(0, len(b), size))


def stream_both(g, o, descs, blocks, what):
    g.reset_mutex()
    g.stream_in(descs, blocks, T.LOCK_ENTRY)
    assert o.stream_in(descs, blocks) == 0
    canonical.assert_same_scene(g.state(), o.state(), what)


def scenes(E, O, name, descs, blocks, what, **cfg):
    """the field on the device and in the oracle -> (LauncherScene, OracleScene, marching-cubes params, voxel size)"""
    hp, cp, mp, vs = F.config(name, **cfg)
    g, o = E.LauncherScene(hp), O.OracleScene(hp, cp)
    stream_both(g, o, descs, blocks, what)
    return g, o, mp, vs


def assert_extraction(mc, g, want, n, what):
    mc.extractIsoSurfaceWithoutCopy(g.hd, g.hp)
    assert mc.counts()["triangles"] == n, f"{what}: {mc.counts()['triangles']} triangles, the oracle has {n}"
    assert same_set(mc.triangles(), want), f"{what}: the triangle sets differ"


def case_lists():
    import gen_mc_tables as G
    tri, edge = G.tables()
    out = []
    for c in range(256):
        e = [(tri[c] >> (4 * k)) & 0xF for k in range(16)]
        out.append(tuple(e[:e.index(0xF)] if 0xF in e else e))
    return out, edge


def edges_by_cell(srcs):
    """{cell: its triangles' edges in buffer order} (a cell's triangles are written one after the other)"""
    out = {}
    code8 = (srcs["edges"][:, None] >> (8 * np.arange(3, dtype=np.uint32))[None, :]) & 0xf
    for cell, e in zip(map(tuple, srcs["cell"].tolist()), code8.tolist()):
        out.setdefault(cell, []).extend(e)
    return {k: tuple(v) for k, v in out.items()}


# ---------------------------------------------------------------------------- 1. all cases, plain and sourced

@pytest.mark.parametrize("name", ["P2", "P4"])
def test_all_cases_plain_and_sourced(E, oracle_lib, name):
    """the planted field astride the origin in all three axes"""
    vs = f32(F.config(name)[0].m_virtualVoxelSize)
    descs, blocks = F.planted(F.NEAR, vs, f32(10.0) * vs)
    g, o, mp, vs = scenes(E, oracle_lib, name, descs, blocks, f"{name} planted")
    want, n = o.extract_iso_surface(mp)
    assert n == 18626
    mc = E.CUDAMarchingCubesHashSDF(mp)
    mc.extractIsoSurface(g.hd, g.hp)
    assert mc.counts() == dict(triangles=n, occupied_blocks=len(descs)) and same_set(mc.triangles(), want)
    assert mc.mesh()["vertices"].tobytes() == mc.triangles()["v"]["p"].reshape(-1, 3).tobytes()
    mc.extractIsoSurfaceIndexed(g.hd, g.hp)
    tris, srcs = mc.triangles(), mc.sources()
    assert mc.counts()["triangles"] == n == len(tris) == len(srcs) and same_set(tris, want)
    snap = MW.assert_sources_name_their_edges(tris, srcs, vs)
    assert not snap.any()  # every sample is 1.25 voxels from zero
    # cell by cell: the ordered edge list is the table's for the cell's case (the float64 reference names the case)
    lists, edge_mask = case_lists()
    ref = F.reference(descs, blocks, vs, mp)
    assert ref["decided"].all()
    got = edges_by_cell(srcs)
    emitting = {tuple(c): lists[k] for c, k in zip(ref["cell"][ref["emits"]].tolist(), ref["case"][ref["emits"]].tolist())}
    assert got == emitting
    distinct = {l for c, l in enumerate(lists) if l and edge_mask[c] != 255}
    assert len(distinct) == 252 and set(got.values()) == distinct
    # cases 85 and 170 (edge mask 255): planted once each by the builder, reached by neighbour cells too, never emitted
    dropped = ref["valid"] & np.isin(ref["case"], (85, 170))
    assert dropped.sum() == 226 and not any(tuple(c) in got for c in ref["cell"][dropped].tolist())
    for p in range(256):
        if F.case_of_pattern(p) in (85, 170):
            assert tuple((np.array(F.NEAR) * F.B + F.pattern_voxel(p)).tolist()) not in got


# ---------------------------------------------------------------------------- 2. threshold sweep

@pytest.mark.parametrize("name", ["P2", "P4"])
@pytest.mark.parametrize("origin", [F.NEAR, F.FAR])
def test_threshold_sweep(E, oracle_lib, name, origin):
    """|d_k| + |d_l| stepped over thres ulp by ulp: a summation order other than the reference's in the trilinear
    sample, or a pair left out of the threshold loops, changes hundreds of cells; one object, nine extractions"""
    hp, cp, mp, vs = F.config(name)
    g = E.LauncherScene(hp)
    mc = E.CUDAMarchingCubesHashSDF(mp)
    for k, count in zip(F.SWEEP_KS, F.SWEEP_COUNTS[origin]):
        descs, blocks = F.planted(origin, vs, F.sweep_amplitude(mp.m_threshMarchingCubes, k))
        g.reset()
        o = oracle_lib.OracleScene(hp, cp)
        stream_both(g, o, descs, blocks, f"{name} {origin} k = {k}")
        want, n = o.extract_iso_surface(mp)
        assert n == count
        assert_extraction(mc, g, want, n, f"{name} {origin} k = {k}")


# ---------------------------------------------------------------------------- 3. random fields, missing neighbours

@pytest.mark.parametrize("name,seed", F.RANDOM_SEEDS)
@pytest.mark.parametrize("left_out", [False, True])
def test_random_fields_with_holes_and_missing_neighbours(E, oracle_lib, name, seed, left_out):
    """27 blocks at (-1..1)^3 with unobserved voxels, values either side of vertexInterp's 1e-5 and values at the size
    of the thresholds; then without 9 of them, so that the 18 others miss neighbours of every kind"""
    hp, cp, mp, vs = F.config(name, max_triangles=1 << 15)
    descs, blocks = F.random_field(F.block_ids(), seed, float(mp.m_threshMarchingCubes), **F.RANDOM)
    if left_out:
        descs, blocks = F.without(descs, blocks, F.LEFT_OUT)
        assert len(descs) == 18
    g, o, mp, vs = scenes(E, oracle_lib, name, descs, blocks, f"{name} random {seed}", max_triangles=1 << 15)
    want, n = o.extract_iso_surface(mp)
    # what the field is here for, counted without the GPU: the float64 reference on the cells rounding cannot change
    # (tests/test_marching_cubes_cases.py holds the oracle to it)
    ref = F.reference(descs, blocks, vs, mp)
    dec = ref["decided"][ref["tri_cell"]][:, None]
    first, second = int(((ref["tri_snap"] == 1) & dec).sum()), int(((ref["tri_snap"] == 2) & dec).sum())
    skipped = int((ref["holed"] & ~ref["valid"]).sum())
    missing = int((~ref["holed"] & ~ref["valid"]).sum())
    print(f"{name} seed {seed} left_out {left_out}: {n} triangles, snapped {first} / {second}, skipped for a weight-0 tap {skipped}, "
          f"for a missing block only {missing}")
    assert n > 2000 and first > 0 and second > 0 and skipped > 1000 and missing > 0
    mc = E.CUDAMarchingCubesHashSDF(mp)
    assert_extraction(mc, g, want, n, "plain")
    mc.extractIsoSurfaceIndexed(g.hd, g.hp)
    tris, srcs = mc.triangles(), mc.sources()
    assert mc.counts()["triangles"] == n and same_set(tris, want)
    snap = MW.assert_sources_name_their_edges(tris, srcs, vs)
    assert (snap == 1).sum() >= first and (snap == 2).sum() >= second


# ---------------------------------------------------------------------------- 4. the own-voxel short cut's boundary

@pytest.mark.parametrize("name,origin,axis", [("P2", (131070, -2, -1), 0), ("P4", (-2, -131074, -1), 1), ("P2", (3, 4, 131071), 2)])
def test_own_voxel_short_cut_at_its_coordinate_limit(E, oracle_lib, name, origin, axis):
    """Blocks +-131071 / +-131072 along one axis hold voxels 2^20 - 8 .. 2^20 + 7: below 2^20 an unobserved own voxel
    skips the cell before any sample is taken, from 2^20 on the eight samples decide.  3 % of the voxels are
    unobserved, on both sides."""
    vs = f32(F.config(name)[0].m_virtualVoxelSize)
    descs, blocks = F.planted(origin, vs, f32(10.0) * vs, holes=0.03, seed=axis)
    local = (np.arange(T.SDF_BLOCK_VOXELS) >> (3 * axis)) & 7  # voxel index = x + 8 y + 64 z
    coord = np.abs(descs["pos"][:, axis].astype(np.int64)[:, None] * F.B + local[None, :])
    holes = blocks["weight"] == 0
    assert (holes & (coord < (1 << 20))).sum() > 50 and (holes & (coord >= (1 << 20))).sum() > 50
    g, o, mp, vs = scenes(E, oracle_lib, name, descs, blocks, f"{name} planted at {origin}")
    want, n = o.extract_iso_surface(mp)
    print(name, origin, n, "triangles")
    assert n > 1000
    assert_extraction(E.CUDAMarchingCubesHashSDF(mp), g, want, n, f"{name} at {origin}")


# ---------------------------------------------------------------------------- 5. neighbour look-ups off collision lists

def test_neighbours_found_on_collision_lists(E, oracle_lib):
    """The random field in a table of 8 buckets with a list limit of 256.  The 27 blocks of (-1..1)^3 put at most 5 in a
    bucket of ten slots, so the field here is the 64 blocks of (-2..1)^3: four buckets are asked for 12 blocks each,
    lists form, and lookup_ptr_wide's walk serves neighbour look-ups whose voxels decide triangles.  Blocks go in one
    by one on both sides (several list inserts into one bucket in one pass may fail, on the device and in the oracle)."""
    from test_gpu_crowded_tables import lists_formed
    name, seed = F.RANDOM_SEEDS[0]
    hp, cp, mp, vs = F.config(name, num_buckets=8, num_sdf_blocks=128, max_triangles=1 << 16, max_collision_list=256)
    ids = F.block_ids(-2, 1)
    demand = np.bincount(canonical.hash_buckets(ids, 8), minlength=8)
    assert (demand > T.HASH_BUCKET_SIZE).sum() >= 2, demand
    descs, blocks = F.random_field(ids, seed, float(mp.m_threshMarchingCubes), **F.RANDOM)
    g, o = E.LauncherScene(hp), oracle_lib.OracleScene(hp, cp)
    for k in range(len(descs)):
        g.reset_mutex()
        failed, exhausted = g.stream_in_settled(descs[k:k + 1], blocks[k:k + 1], T.LOCK_ENTRY)
        assert len(failed) == 0 and not exhausted
        o.reset_mutex()
        assert o.stream_in(descs[k:k + 1], blocks[k:k + 1]) == 0
    canonical.assert_same_scene(g.state(), o.state(), "64 blocks in 8 buckets")
    print(lists_formed(g.download(False)["hash"], g.hp))
    want, n = o.extract_iso_surface(mp)
    assert n > 10000
    assert_extraction(E.CUDAMarchingCubesHashSDF(mp), g, want, n, "crowded table")


# ---------------------------------------------------------------------------- 6. box faces through cell centres

@pytest.mark.parametrize("lo,hi", [((1, 2, 1), (9, 10, 5)), ((-11, -12, -5), (-2, 3, 2))])
def test_box_faces_through_cell_centres(E, oracle_lib, lo, hi):
    """box corners float(i) * voxel: the centres of the cells i lie exactly on the six faces; both ends are inclusive"""
    name = "P2"
    vs = f32(F.config(name)[0].m_virtualVoxelSize)
    descs, blocks = F.planted(F.NEAR, vs, f32(10.0) * vs)
    g, o, mp, vs = scenes(E, oracle_lib, name, descs, blocks, "planted")
    lo_w, hi_w = [f32(i) * vs for i in lo], [f32(i) * vs for i in hi]
    mp.m_boxEnabled = 1
    mp.m_minCorner[:] = [float(v) for v in lo_w]
    mp.m_maxCorner[:] = [float(v) for v in hi_w]
    want, n = o.extract_iso_surface(mp)
    mc = E.CUDAMarchingCubesHashSDF(T.make_marching_cubes_params(g.hp, 1 << 16))
    mc.extractIsoSurfaceWithoutCopy(g.hd, g.hp, lo_w, hi_w, True)
    assert mc.counts()["triangles"] == n and 500 < n < 18626 and same_set(mc.triangles(), want)
    mc.extractIsoSurfaceIndexed(g.hd, g.hp, lo_w, hi_w, True)
    cells = mc.sources()["cell"]
    assert mc.counts()["triangles"] == n and same_set(mc.triangles(), want)
    # cells on all six faces are in, their neighbours one voxel out are not -- though they give triangles without the box
    assert cells.min(axis=0).tolist() == list(lo) and cells.max(axis=0).tolist() == list(hi)
    mc.extractIsoSurfaceIndexed(g.hd, g.hp)
    every = mc.sources()["cell"]
    for axis in range(3):
        inside = np.all((every >= np.array(lo)) & (every <= np.array(hi)) | (np.arange(3) == axis), axis=1)
        assert (inside & (every[:, axis] == lo[axis] - 1)).any() and (inside & (every[:, axis] == hi[axis] + 1)).any()
    assert int(np.all((every >= np.array(lo)) & (every <= np.array(hi)), axis=1).sum()) == n


# ---------------------------------------------------------------------------- 7. capacity cuts, launcher level

def test_triangle_buffer_that_ends_anywhere(E, oracle_lib, vh):
    """m_maxNumTriangles = cap in a buffer with room for everything, prefilled: the count is the full one, the first
    cap triangles are triangles of the full set, and nothing is written past cap -- with the buffer ending inside a
    wave's run of the counter and inside one lane's list (n - 1, n - 3), at 0 and at 1.  Plain and sourced."""
    from voxelhashing_amd import lib
    name = "P2"
    vs = f32(F.config(name)[0].m_virtualVoxelSize)
    descs, blocks = F.planted(F.NEAR, vs, f32(10.0) * vs)
    g, o, mp, vs = scenes(E, oracle_lib, name, descs, blocks, "planted")
    full, n = o.extract_iso_surface(mp)
    assert n == 18626
    full_count = counted(full)
    room = n + 64
    tsize, ssize = T.TRIANGLE_DTYPE.itemsize, T.TRIANGLE_SOURCE_DTYPE.itemsize
    d_params = lib.DeviceBuffer(C.sizeof(T.MarchingCubesParams))
    d_nblocks, d_ntris = lib.DeviceBuffer(4), lib.DeviceBuffer(4)
    d_blocks = lib.DeviceBuffer(4 * g.hp.m_hashNumBuckets * T.HASH_BUCKET_SIZE)
    d_tris, d_srcs = lib.DeviceBuffer(tsize * room), lib.DeviceBuffer(ssize * room)
    data = T.MarchingCubesData(d_params.ptr, d_nblocks.ptr, d_blocks.ptr, d_ntris.ptr, d_tris.ptr, 1)
    for sourced in (False, True):
        for cap in (0, 1, n - 1, n - 3, n // 2 + 1):
            what = f"cap {cap}, sourced {sourced}"
            mp.m_maxNumTriangles = cap
            d_params.upload(np.frombuffer(bytes(mp), np.uint8))
            lib.check(vh.vh_memset(d_tris.ptr, PATTERN, d_tris.nbytes, None), "memset")
            lib.check(vh.vh_memset(d_srcs.ptr, PATTERN, d_srcs.nbytes, None), "memset")
            lib.check(vh.vh_reset_marching_cubes(C.byref(data), None), "reset")
            lib.check(vh.vh_extract_iso_surface_pass1(C.byref(g.hd), C.byref(g.hp), C.byref(data), None), "pass1")
            nblk = int(d_nblocks.download(np.uint32, 1)[0])
            assert nblk == len(descs)
            if sourced:
                lib.check(vh.vh_extract_iso_surface_pass2_sourced(C.byref(g.hd), C.byref(g.hp), C.byref(data), d_srcs.ptr, nblk, None), "pass2 sourced")
            else:
                lib.check(vh.vh_extract_iso_surface_pass2(C.byref(g.hd), C.byref(g.hp), C.byref(data), nblk, None), "pass2")
            assert int(d_ntris.download(np.uint32, 1)[0]) == n, what
            raw = d_tris.download(np.uint8)
            assert np.all(raw[tsize * cap:] == PATTERN), f"{what}: a triangle written past the capacity"
            kept = raw[:tsize * cap].view(T.TRIANGLE_DTYPE)
            for tri, times in counted(kept).items():
                assert times <= full_count.get(tri, 0), f"{what}: a triangle the full set has not, or has less often"
            raw_s = d_srcs.download(np.uint8)
            if sourced:
                assert np.all(raw_s[ssize * cap:] == PATTERN), f"{what}: a source record written past the capacity"
                if cap:
                    MW.assert_sources_name_their_edges(kept, raw_s[:ssize * cap].view(T.TRIANGLE_SOURCE_DTYPE), vs)
            else:
                assert np.all(raw_s == PATTERN), f"{what}: the plain pass wrote source records"


# ---------------------------------------------------------------------------- 8. weld and normals on the all-case mesh

def by_key(mesh):
    return np.ascontiguousarray(mesh["normals"][np.argsort(mesh["keys"], kind="stable")])


def assert_welded_with_normals(E, mc, g, vs, what):
    mc.extractIsoSurfaceIndexed(g.hd, g.hp)
    tris, srcs, ind = mc.triangles(), mc.sources(), mc.indexed()
    want = MW.weld(tris, srcs)
    got = MW.canonical(ind)
    for k in ("keys", "vertices", "colors", "faces"):
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), f"{what}: {k}"
    assert mc.indexed_counts() == dict(vertices=len(want["keys"]), faces=len(want["faces"]), status=0)
    scale = E.mesh_normals_default_scale_log2(vs)
    restated = MN.vertex_normals(got["vertices"], got["keys"], got["faces"], scale)
    normals = by_key(ind)
    assert restated["status"] == 0 and normals.tobytes() == restated["normals"].tobytes() and normals.any(), f"{what}: normals"
    ratio, unit = MN.check_against_reference(normals, got["vertices"], got["faces"], scale)
    props = MW.properties(got, tris, srcs)
    # (Bourke's tables leave cracks on ambiguous faces, and these fields have them on purpose: no two-faces-per-edge here)
    print(what, dict(triangles=len(tris), vertices=len(got["keys"]), faces=len(got["faces"]), dropped_faces=want["dropped_faces"],
                     normals_error_over_bound=ratio, **props))
    assert props["repeated"] == 0 and len(got["faces"]) > 1000
    return got


@pytest.mark.parametrize("name,origin", [("P2", F.NEAR), ("P4", F.NEAR), ("P2", F.FAR)])
def test_weld_and_normals_on_the_all_case_mesh(E, oracle_lib, name, origin):
    vs = f32(F.config(name)[0].m_virtualVoxelSize)
    descs, blocks = F.planted(origin, vs, f32(10.0) * vs)
    assert F.weld_inputs_in_range(descs)
    g, o, mp, vs = scenes(E, oracle_lib, name, descs, blocks, f"{name} planted at {origin}")
    mc = E.CUDAMarchingCubesHashSDF(mp)
    mc.setIndexedNormals(True)
    assert_welded_with_normals(E, mc, g, vs, f"{name} planted at {origin}")
    want, n = o.extract_iso_surface(mp)
    assert n == 18626 and same_set(mc.triangles(), want)


@pytest.mark.parametrize("name,seed", F.RANDOM_SEEDS)
def test_weld_and_normals_on_the_random_field(E, oracle_lib, name, seed):
    hp, cp, mp, vs = F.config(name)
    descs, blocks = F.random_field(F.block_ids(), seed, float(mp.m_threshMarchingCubes), **F.RANDOM)
    g, o, mp, vs = scenes(E, oracle_lib, name, descs, blocks, f"{name} random {seed}")
    mc = E.CUDAMarchingCubesHashSDF(mp)
    mc.setIndexedNormals(True)
    got = assert_welded_with_normals(E, mc, g, vs, f"{name} random {seed}")
    assert ((got["keys"] >> np.uint64(60)) == MW.POINT).sum() > 0  # snapped vertices, keyed by their lattice point
    want, n = o.extract_iso_surface(mp)
    assert same_set(mc.triangles(), want)


def test_last_lattice_point_with_a_key_and_the_first_without(E, oracle_lib):
    """Blocks 65532..65535 end at voxel 2^19 - 1.  Its cells are skipped (their neighbours lie in the missing block
    65536), so the last cell with triangles is 2^19 - 2 and its upper corners are the lattice points L.x = 2^19 - 1, the
    last that vh_mesh_key accepts: the extraction welds, status 0.  One block further, cells from 2^19 - 1 on give
    triangles: VH_WELD_KEY_RANGE, reported as vh_mesh_weld reports it, and nothing is left behind; the same object then
    serves the in-range field again."""
    from voxelhashing_amd import lib
    name = "P2"
    hp, cp, mp, vs = F.config(name)
    inside, outside = F.planted((65532, -2, -1), vs, f32(10.0) * vs), F.planted((65533, -2, -1), vs, f32(10.0) * vs)
    assert (inside[0]["pos"][:, 0].max() + 1) * F.B == 1 << 19 and (outside[0]["pos"][:, 0].max() + 1) * F.B == (1 << 19) + F.B
    g, o, mp, vs = scenes(E, oracle_lib, name, *inside, "planted at 65532")
    mc = E.CUDAMarchingCubesHashSDF(mp)
    mc.setIndexedNormals(True)
    first = assert_welded_with_normals(E, mc, g, vs, "planted at 65532")
    assert int((first["keys"] & np.uint64((1 << 20) - 1)).max()) == (1 << 20) - 1  # L.x + 2^19
    want, n = o.extract_iso_surface(mp)
    assert same_set(mc.triangles(), want)
    g2, o2, _, _ = scenes(E, oracle_lib, name, *outside, "planted at 65533")
    with pytest.raises(lib.VhError) as e:
        mc.extractIsoSurfaceIndexed(g2.hd, g2.hp)
    assert e.value.code == 4  # VH_ERR_BAD_ARGUMENT
    assert mc.indexed_counts() == dict(vertices=0, faces=0, status=T.WELD_KEY_RANGE)
    want2, n2 = o2.extract_iso_surface(mp)
    assert mc.counts()["triangles"] == n2 and same_set(mc.triangles(), want2)  # the soup is whole, only the weld refused
    assert (mc.sources()["cell"][:, 0] >= (1 << 19) - 1).any()
    again = assert_welded_with_normals(E, mc, g, vs, "planted at 65532, after the refusal")
    assert MW.same_mesh(again, first)


# ---------------------------------------------------------------------------- 9. the chunk-grid walk

def test_chunk_grid_walk_over_the_all_case_field(E, oracle_lib, vh):
    """The planted field (P2) in a scene with a 3 x 3 x 3 grid of 0.64 m chunks: blocks -2 of x and y belong to chunk
    -1, the others to chunk 0, so four chunks are appended and their boxes meet at voxel -8, between the patterns at
    -11 and -7.  The accumulated mesh is the direct indexed extraction's."""
    from voxelhashing_amd import lib
    name = "P2"
    ext, dims, low = (0.64, 0.64, 0.64), (3, 3, 3), (-1, -1, -1)
    hp, cp, mp, vs = F.config(name, streaming_extents=ext, streaming_dims=dims, streaming_min=low)
    descs, blocks = F.planted(F.NEAR, vs, f32(10.0) * vs)
    scene = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=True, gc=False))
    hd, hpp = scene.getHashData(), scene.getHashParams()
    d_desc, d_blocks = lib.DeviceBuffer.from_numpy(descs), lib.DeviceBuffer.from_numpy(blocks)
    prev = int(lib.download(hd.d_heapCounter, np.uint32, 1)[0])
    lib.check(vh.vh_reset_bucket_mutex(C.byref(hd), C.byref(hpp), None), "vh_reset_bucket_mutex")
    lib.check(vh.vh_stream_in_pass1(C.byref(hd), C.byref(hpp), len(descs), prev, d_desc.ptr, T.LOCK_ENTRY, None), "vh_stream_in_pass1")
    lib.check(vh.vh_stream_in_pass2(C.byref(hd), C.byref(hpp), len(descs), prev, d_desc.ptr, d_blocks.ptr, None), "vh_stream_in_pass2")
    lib.check(vh.vh_memcpy_h2d(hd.d_heapCounter, np.array([prev - len(descs)], np.uint32).ctypes.data, 4, None), "heapCounter")
    o = oracle_lib.OracleScene(hp, cp)
    assert o.stream_in(descs, blocks) == 0
    before = scene.state()
    canonical.assert_same_scene(before, o.state(), "planted, in the scene class")
    want, n = o.extract_iso_surface(mp)
    direct = E.CUDAMarchingCubesHashSDF(mp)
    direct.extractIsoSurfaceIndexed(hd, hpp)
    assert direct.counts()["triangles"] == n == 18626 and same_set(direct.triangles(), want)
    grid = E.CUDASceneRepChunkGrid(scene, ext, dims, low, 64, True, 4)
    try:
        mc = E.CUDAMarchingCubesHashSDF(mp)
        mc.extractIsoSurfaceIndexedChunkGrid(grid, (0.0, 0.0, 0.0), 100.0)
        got, stats = mc.indexed(), mc.indexed_stats()
        after = scene.state()
    finally:
        grid.close()
    print(stats)
    assert stats["status"] == 0 and stats["dropped"] > 0 and stats["cells"] == 7912  # the cells that give triangles, each kept once
    assert MW.same_mesh(MW.canonical(got), MW.canonical(direct.indexed()))
    canonical.assert_same_scene(before, after, "scene after the walk")
