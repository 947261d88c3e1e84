"""The finish of the indexed mesh as one chain ("The finish as one chain"): clustering, smoothing,
normals and the component filter in every on/off combination, at the launcher level (vh_mesh_weld_accum_*) and through
CUDAMarchingCubesHashSDF (finishIndexed and the one-shot extraction, the options switched one at a time on ONE object),
against the chain of the numpy restatements done by hand: MW.weld -> MK.cluster -> MS.smooth -> MN.vertex_normals ->
MC.filter.  Meshes canonical and bit for bit, counts by name, normals bit for bit in key order.

The launcher level runs two inputs.  random_soup(2000, 11, spread=3) welds to ONE component (every cell of its cube is
full), so no min_faces can drop a component of it and keep another: on it the filter is held to the restatement all the
same, and the condition "drops one, keeps one" is asserted on the second input, the same soup with five small islands
beside it."""
import itertools

import numpy as np
import pytest

import mesh_cluster as MK
import mesh_components as MC
import mesh_normals as MN
import mesh_smooth as MS
import mesh_weld as MW
import mesh_weld_appends as MA
from helpers import small_config
from test_gpu_mesh_components import same_bits
from test_gpu_mesh_weld_appends import gpu_scene
from voxelhashing_amd import synth, vhtypes as T

pytestmark = pytest.mark.gpu

CELLS, ITERATIONS = 2, 3          # clustering at 2 cells a side, 3 Taubin iterations without keep_boundary
SCALE, NORMALS_SCALE = 21, 30     # the launcher level's fixed-point scales, as the tests of the single passes have them
MIN_FACES = 10                    # of the launcher level's filter
COMBINATIONS = list(itertools.product((False, True), repeat=4))  # (cluster, smooth, normals, filter)
GRAY = [tuple(bool((i ^ (i >> 1)) >> b & 1) for b in range(4)) for i in range(16)]  # one option switches per step


class HandChain:
    """the chain of the restatements over one welded mesh; the four (cluster, smooth) variants are computed once"""

    def __init__(self, welded, scale, normals_scale, min_faces=0, largest_only=False):
        self.scale, self.normals_scale, self.min_faces, self.largest_only = scale, normals_scale, min_faces, largest_only
        self.variants = {}
        for cluster, smooth in itertools.product((False, True), repeat=2):
            mesh, counts = MW.canonical(welded), {}
            if cluster:
                r = MK.cluster(mesh, CELLS, scale)
                assert r["status"] == 0
                mesh, counts["cluster"] = r["mesh"], r["counts"]
            if smooth:
                before = mesh
                r = MS.smooth(mesh, ITERATIONS, keep_boundary=False, scale_log2=scale)
                assert r["status"] == 0
                mesh, counts["smooth"] = r["mesh"], r["counts"]
                assert r["counts"]["moved"] > 0 and not MW.same_mesh(mesh, before)  # smoothing moves a vertex
            self.variants[cluster, smooth] = (mesh, counts)
        assert self.variants[True, False][1]["cluster"]["collapsed"] > 0  # clustering collapses a face

    def normals_scale_of(self, cluster, smooth):
        return self.normals_scale(cluster, smooth) if callable(self.normals_scale) else self.normals_scale

    def expected(self, cluster, smooth, normals, filt):
        """-> the canonical mesh of the combination (with normals if on) and the counts of the passes that ran, by name"""
        mesh, counts = self.variants[cluster, smooth]
        counts = dict(counts)
        if normals:
            n = MN.vertex_normals(mesh["vertices"], mesh["keys"], mesh["faces"], self.normals_scale_of(cluster, smooth))
            assert n["status"] == 0
            mesh = dict(mesh, normals=n["normals"])
        if filt:
            r = MC.filter(mesh, self.min_faces, self.largest_only)
            assert r["status"] == 0
            mesh, counts["components"] = r["mesh"], r["counts"]
        return mesh, counts

    def filter_drops_and_keeps(self):
        """the filter's condition, over each of the four variants it can meet"""
        return all(0 < MC.filter(m, self.min_faces, self.largest_only)["counts"]["kept_components"] < MC.filter(m, 0)["counts"]["components"]
                   for m, _ in self.variants.values())


def assert_same(got, want, what):
    g = MC.canonical(got)
    assert MW.same_mesh(g, want), what
    assert ("normals" in g) == ("normals" in want), what
    if "normals" in want:
        assert same_bits(g["normals"], want["normals"]), what


# ---------------------------------------------------------------------------- (a) the launcher level

def island_soup():
    soup, srcs = MW.random_soup(2000, 11, spread=3)
    islands, records = MC.archipelago((1, 2, 5, 22, 64))
    records = records.copy()
    records["cell"][:, 0] += 20  # clear of the soup's cube, and of one another
    return np.concatenate([soup, islands]), np.concatenate([srcs, records])


@pytest.fixture(scope="module")
def dealt():
    """name -> the soup dealt into 5 appends as in the tests of the single passes, and the hand chain over its weld"""
    out = {}
    for name, (soup, srcs) in (("soup", MW.random_soup(2000, 11, spread=3)), ("islands", island_soup())):
        out[name] = dict(parts=MA.deal(soup, srcs, 5, 11), chain=HandChain(MW.weld(soup, srcs), SCALE, NORMALS_SCALE, MIN_FACES))
    assert out["islands"]["chain"].filter_drops_and_keeps()
    return out


@pytest.mark.parametrize("name", ["soup", "islands"])
def test_launcher_level_every_combination(vh, dealt, name):
    from voxelhashing_amd import engine as E
    parts, chain = dealt[name]["parts"], dealt[name]["chain"]
    for cluster, smooth, normals, filt in COMBINATIONS:
        what = f"{name}: cluster {cluster} smooth {smooth} normals {normals} filter {filt}"
        want, counts = chain.expected(cluster, smooth, normals, filt)
        got = E.mesh_weld_appends(parts, cluster_cells=CELLS if cluster else 0, cluster_scale_log2=SCALE, smooth_iterations=ITERATIONS if smooth else 0,
                                  keep_boundary=False, smooth_scale_log2=SCALE, normals_scale_log2=NORMALS_SCALE if normals else None,
                                  min_component_faces=MIN_FACES if filt else 0)
        assert got["status"] == 0, what
        assert {k: got[k + "_counts"] for k in ("cluster", "smooth") if k + "_counts" in got} == {k: v for k, v in counts.items() if k != "components"}, what
        assert got.get("component_counts") == counts.get("components"), what
        assert got.get("normals_code", 0) == 0 and ("normals" in got) == normals, what
        last = got["filtered"] if filt else dict(got["smoothed"] if smooth else got["clustered"] if cluster else got)
        if normals and not filt:
            last["normals"] = got["normals"]
        assert_same({k: last[k] for k in ("vertices", "colors", "keys", "faces", "normals") if k in last}, want, what)
        # the stages before the last hold what they made, and the accumulator's own mesh is what it was
        assert MW.same_mesh(MW.canonical(got), chain.variants[False, False][0]), what
        if cluster:
            assert MW.same_mesh(MW.canonical(got["clustered"]), chain.variants[True, False][0]), what
        if smooth:
            assert MW.same_mesh(MW.canonical(got["smoothed"]), chain.variants[cluster, True][0]), what


# ---------------------------------------------------------------------------- (b) the class level

@pytest.fixture(scope="module")
def scene(vh):
    """the 96x72 scene of three S1 orbit frames, an extractor, two overlapping boxes, and the hand chain over the direct
    extraction's welded mesh; the filter is min_faces where one up to a quarter of the faces drops and keeps a component
    in every variant, else largest_only"""
    from voxelhashing_amd import engine as E
    hp, cp, _ = small_config(96, 72)
    s = gpu_scene(E, hp, cp, [synth.orbit_pose(k, 100) for k in range(3)], synth.S1_SPHERES)
    hd, hpp = s.getHashData(), s.getHashParams()
    mc = E.CUDAMarchingCubesHashSDF(T.make_marching_cubes_params(hp, 1 << 19))
    mc.extractIsoSurfaceIndexed(hd, hpp)
    welded, soup = mc.indexed(), mc.triangles()
    vs = np.float32(hpp.m_virtualVoxelSize)
    cx, half = float(np.median(soup["v"]["p"][..., 0])), 0.5 * float(vs) * T.SDF_BLOCK_SIZE
    boxes = [((-10.0, -10.0, -10.0), (cx + half, 10.0, 10.0)), ((cx - half, -10.0, -10.0), (10.0, 10.0, 10.0))]

    def normals_scale(cluster, smooth):  # the edge bound of readBackIndexed, doubled under smoothing
        return E.mesh_normals_default_scale_log2(np.float32(2.0 if smooth else 1.0) * (np.float32(2 * CELLS) * vs if cluster else vs))

    chain = HandChain(welded, MK.default_scale_log2(float(vs)), normals_scale)
    for chain.min_faces in (m for m in (5, 10, 20, 50, 100, 200, 500) if m <= len(welded["faces"]) // 4):
        if chain.filter_drops_and_keeps():
            break
    else:
        chain.min_faces, chain.largest_only = 0, True
        assert chain.filter_drops_and_keeps()
    print("class level: filter", dict(min_faces=chain.min_faces, largest_only=chain.largest_only), "welded faces", len(welded["faces"]))
    return dict(scene=s, mc=mc, hd=hd, hpp=hpp, boxes=boxes, chain=chain)


def set_options(mc, chain, cluster, smooth, normals, filt):
    mc.setIndexedClustering(CELLS if cluster else 0)
    mc.setIndexedSmoothing(ITERATIONS if smooth else 0, keepBoundary=False)
    mc.setIndexedNormals(normals)
    mc.setIndexedComponentFilter(chain.min_faces if filt else 0, chain.largest_only if filt else False)


def check_extraction(mc, chain, combination, what):
    cluster, smooth, normals, filt = combination
    want, counts = chain.expected(*combination)
    nothing = lambda stats: set(stats.values()) == {0}
    assert mc.indexed_cluster_stats() == counts["cluster"] if cluster else nothing(mc.indexed_cluster_stats()), what
    assert mc.indexed_smooth_stats() == counts["smooth"] if smooth else nothing(mc.indexed_smooth_stats()), what
    assert mc.indexed_component_stats() == counts["components"] if filt else nothing(mc.indexed_component_stats()), what
    assert mc.indexed_counts() == dict(vertices=len(want["keys"]), faces=len(want["faces"]), status=0), what
    ind, mesh = mc.indexed(), mc.mesh()
    assert_same(ind, want, what)
    assert mesh["vertices"].tobytes() == ind["vertices"].tobytes() and np.array_equal(mesh["faces"], ind["faces"]), what
    assert ("normals" in mesh) == normals and (not normals or same_bits(mesh["normals"], ind["normals"])), what


def test_sixteen_finishes_of_one_accumulation_in_gray_code_order(scene):
    """two appendIndexed of overlapping boxes, then finishIndexed sixteen times with no append between: each step
    switches one option, and each result is the hand chain's for that combination"""
    mc, chain = scene["mc"], scene["chain"]
    try:
        mc.beginIndexed()
        for lo, hi in scene["boxes"]:
            mc.appendIndexed(scene["hd"], scene["hpp"], lo, hi, True)
        for combination in GRAY:
            set_options(mc, chain, *combination)
            mc.finishIndexed()
            check_extraction(mc, chain, combination, f"finishIndexed {combination}")
            stats = mc.indexed_stats()
            assert stats["dropped"] > 0 and stats["status"] == 0 and stats["vertices"] == len(chain.variants[False, False][0]["keys"])
    finally:
        set_options(mc, chain, False, False, False, False)
        mc.clearMeshBuffer()


def test_sixteen_one_shot_extractions_on_one_object_in_gray_code_order(scene):
    """the same sixteen through extractIsoSurfaceIndexed on one object: what a stage held for the extraction before is stale"""
    mc, chain = scene["mc"], scene["chain"]
    try:
        for combination in GRAY:
            set_options(mc, chain, *combination)
            mc.extractIsoSurfaceIndexed(scene["hd"], scene["hpp"])
            check_extraction(mc, chain, combination, f"extractIsoSurfaceIndexed {combination}")
            assert set(mc.indexed_stats().values()) == {0}
    finally:
        set_options(mc, chain, False, False, False, False)
        mc.clearMeshBuffer()


def test_gray_code_order_switches_one_option_per_step_and_visits_all():
    assert sorted(GRAY) == sorted(COMBINATIONS) and GRAY[0] == (False, False, False, False)
    assert all(sum(a != b for a, b in zip(GRAY[i], GRAY[i + 1])) == 1 for i in range(15))
