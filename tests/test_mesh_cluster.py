"""Vertex clustering of the indexed mesh, without a GPU ("Mesh clustering"): the cluster key against
floor division written out, the default scales, the numpy restatement (tests/mesh_cluster.py) against a float64 mean
and its clusters' boxes, its independence of face order, rotation and vertex numbers, hand-made duplicates and
collapses, the constants and prototypes, the refusals through the library, the option's defaults, what the kernels
cost, and the replay tool's usage errors."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mesh_cluster as MK
import mesh_weld as MW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARGUMENT = 4  # VH_ERR_BAD_ARGUMENT
B = 1 << 19


def key_of(L, code=3):
    return int(MK.pack_point(np.array(L, dtype=np.int64), code))


# ---------------------------------------------------------------------------- 1. the cluster key

@pytest.mark.parametrize("m", [1, 2, 3, 4, 7, 64])
def test_cluster_key_is_floor_division(vh, m):
    """the library's key (host side of csrc/vh_mesh_key.hpp) and the restatement's against math.floor, at the values
    where truncation would differ and at both ends of the key range"""
    out = C.c_uint64()
    for l in (-1, -m, -m - 1, m - 1, m, 0, 1, -B, -B + 1, B - 1, B - 2, 5 * m, -5 * m, -5 * m + 1):
        k = math.floor(l / m)
        assert k * m <= l < (k + 1) * m
        for code in range(4):
            key = key_of((l, -l - 1, (l % 7) - 3), code)
            want = key_of((k, math.floor((-l - 1) / m), math.floor(((l % 7) - 3) / m)))
            assert vh.vh_mesh_cluster_key(key, m, C.byref(out)) == 0 and out.value == want == MK.cluster_key(key, m), (l, m, code)
    assert key_of((-1, -1, -1)) == MK.cluster_key(key_of((-1, -2, -1), 0), 2)  # L = -1, m = 2: k = -1, not 0


def test_cluster_key_refusals(vh):
    out = C.c_uint64(7)
    good = key_of((1, 2, 3), 1)
    assert vh.vh_mesh_cluster_key(good, 0, C.byref(out)) == BAD_ARGUMENT and vh.vh_mesh_cluster_key(good, 65, C.byref(out)) == BAD_ARGUMENT
    assert vh.vh_mesh_cluster_key(good, 2, None) == BAD_ARGUMENT
    for bad in (good | 1 << 62, good | 1 << 63, (1 << 64) - 1):
        assert vh.vh_mesh_cluster_key(bad, 2, C.byref(out)) == BAD_ARGUMENT and MK.cluster_key(bad, 2) is None
    assert out.value == 7


def test_default_scales_and_refusals(vh):
    out = C.c_int32(99)
    for vs, want in ((0.04, 21), (0.01, 23), (0.004, 24), (1.0, 16), (0.5, 17), (0.25, 18), (0.26, 18), (2.0, 15), (3.9, 15)):
        assert vh.vh_mesh_cluster_default_scale_log2(vs, C.byref(out)) == 0 and out.value == want == MK.default_scale_log2(vs) == 16 - math.floor(math.log2(np.float32(vs))), vs
        assert (B * vs) * 2.0 ** want < 2.0 ** 36  # lattice positions within the key range stay under 2^36
    out.value = 99
    for vs in (0.0, -0.04, float("inf"), float("nan")):
        assert vh.vh_mesh_cluster_default_scale_log2(vs, C.byref(out)) == BAD_ARGUMENT
    assert vh.vh_mesh_cluster_default_scale_log2(0.04, None) == BAD_ARGUMENT and out.value == 99


# ---------------------------------------------------------------------------- 2. the restatement's arithmetic

@pytest.fixture(scope="module")
def soups():
    """the two welded random soups of the issue, and one whose vertices lie on their lattice edges"""
    return {257: MW.weld(*MW.random_soup(257, 11)), 2000: MW.weld(*MW.random_soup(2000, 12, spread=6)), "lattice": MW.weld(*MK.lattice_soup(2000, 13, 0.04))}


@pytest.mark.parametrize("n, m", [(257, 2), (257, 4), (2000, 2), (2000, 4)])
def test_representative_against_a_float64_mean(soups, n, m):
    """|r - mean64| <= 1/S + 2^-24 |r| per component: half a quantum per member, averaged; half a quantum for the
    division; the rounding to float32"""
    mesh, scale = soups[n], 21
    out = MK.cluster(mesh, m, scale)
    assert out["status"] == 0 and 0 < out["counts"]["vertices"] < len(mesh["keys"])
    ukeys, mean64, members = MK.float64_means(mesh, m)
    assert out["counts"]["vertices"] + out["counts"]["unused_clusters"] == len(ukeys) and members.max() > 1
    at = np.searchsorted(ukeys, out["mesh"]["keys"])
    assert np.array_equal(ukeys[at], out["mesh"]["keys"])
    r = out["mesh"]["vertices"].astype(np.float64)
    err = np.abs(r - mean64[at])
    bound = 2.0 ** -scale + 2.0 ** -24 * np.abs(r)
    print("largest error / bound", float((err / bound).max()))
    assert np.all(err <= bound)


@pytest.mark.parametrize("m", [1, 2, 4])
def test_representative_lies_in_its_clusters_box(soups, m):
    """vertices of an extraction lie on their lattice edges, so a cluster's mean lies in the closed box
    [(k m - 1/2) vs, (k m + m - 1/2) vs]; the float32 positions and the mean's quantum are allowed for"""
    mesh, vs, scale = soups["lattice"], 0.04, 21
    out = MK.cluster(mesh, m, scale)
    assert out["status"] == 0
    k = MK.lattice(out["mesh"]["keys"]).astype(np.float64)
    r = out["mesh"]["vertices"].astype(np.float64)
    slack = 2.0 ** -scale + 2.0 ** -23 * np.abs(r)  # the members' own float32 rounding, the quantum, the final rounding
    assert np.all(r >= (k * m - 0.5) * vs - slack) and np.all(r <= (k * m + m - 0.5) * vs + slack)
    assert np.all((out["mesh"]["keys"] >> np.uint64(60)) == 3)


def test_restatement_does_not_depend_on_face_order_rotation_or_vertex_numbers(soups):
    m = soups[2000]
    want = MK.cluster(m, 2, 21)
    assert want["counts"]["collapsed"] > 0 and want["counts"]["duplicates"] > 0
    rng = np.random.default_rng(3)
    f = m["faces"][rng.permutation(len(m["faces"]))]
    r = rng.integers(0, 3, len(f))
    f = np.stack([f[np.arange(len(f)), (r + k) % 3] for k in range(3)], axis=1)
    other = MK.cluster(dict(m, faces=f), 2, 21)
    assert other["counts"] == want["counts"] and MW.same_mesh(other["mesh"], want["mesh"])
    p = rng.permutation(len(m["keys"]))
    inv = np.empty_like(p)
    inv[p] = np.arange(len(p))
    renumbered = dict(vertices=m["vertices"][p], colors=m["colors"][p], keys=m["keys"][p], faces=inv[m["faces"].astype(np.int64)].astype(np.uint32))
    again = MK.cluster(renumbered, 2, 21)
    assert again["counts"] == want["counts"] and MW.same_mesh(again["mesh"], want["mesh"])


# ---------------------------------------------------------------------------- 3. hand-made cases

def hand_made():
    """name -> (mesh, m, expected counts, expected faces as cluster-key triples)"""
    K = key_of
    out = {}
    # clusters at m = 2: A = (0,0,0), B = (1,0,0), C = (0,1,0), D = (1,1,0); two vertices in each of A, B, C
    keys = [K((0, 0, 0)), K((1, 1, 1), 0), K((2, 0, 0)), K((3, 1, 0), 1), K((0, 2, 0)), K((1, 3, 1), 2), K((2, 2, 0))]
    A, Bc, Cc = K((0, 0, 0)), K((1, 0, 0)), K((0, 1, 0))
    # the same winding twice: one stays, one duplicate
    out["same_winding"] = (MK.plain_mesh(keys, [(0, 2, 4), (3, 5, 1)]), 2, dict(vertices=3, faces=1, collapsed=0, duplicates=1, unused_clusters=1), [(A, Bc, Cc)])
    # opposite windings: rotated to A first they are (A, B, C) and (A, C, B); B < C, so (A, B, C) stays whichever comes first
    out["opposite_windings"] = (MK.plain_mesh(keys, [(4, 2, 0), (0, 2, 4)]), 2, dict(vertices=3, faces=1, collapsed=0, duplicates=1, unused_clusters=1), [(A, Bc, Cc)])
    out["opposite_windings_swapped"] = (MK.plain_mesh(keys, [(1, 3, 5), (5, 3, 1)]), 2, dict(vertices=3, faces=1, collapsed=0, duplicates=1, unused_clusters=1), [(A, Bc, Cc)])
    # only the other winding: it stays as it is
    out["one_odd_winding"] = (MK.plain_mesh(keys, [(2, 0, 4)]), 2, dict(vertices=3, faces=1, collapsed=0, duplicates=0, unused_clusters=1), [(A, Cc, Bc)])
    # a face with two corners in A collapses; the other stays
    out["collapse"] = (MK.plain_mesh(keys, [(0, 1, 2), (0, 2, 6)]), 2, dict(vertices=3, faces=1, collapsed=1, duplicates=0, unused_clusters=1), [(A, Bc, K((1, 1, 0)))])
    # a small component that falls into one cluster whole: its faces collapse, its cluster is unused, the mesh loses it
    far = [K((40, 40, 40)), K((41, 40, 40)), K((40, 41, 40)), K((41, 41, 41))]
    out["component_collapses_whole"] = (MK.plain_mesh(keys + far, [(0, 2, 4), (7, 8, 9), (8, 10, 9)]), 2,
                                        dict(vertices=3, faces=1, collapsed=2, duplicates=0, unused_clusters=2), [(A, Bc, Cc)])
    # m = 1: every lattice point is its own cluster, but the codes fall together: vertices 0 and 1' share point (0,0,0)
    k1 = [K((0, 0, 0)), K((0, 0, 0), 0), K((1, 0, 0), 1), K((0, 1, 0), 2), K((5, 5, 5))]
    out["m_1"] = (MK.plain_mesh(k1, [(0, 2, 3), (1, 2, 3), (0, 1, 2)]), 1, dict(vertices=3, faces=1, collapsed=1, duplicates=1, unused_clusters=1),
                  [(K((0, 0, 0)), K((1, 0, 0)), K((0, 1, 0)))])
    return out


@pytest.mark.parametrize("name", sorted(hand_made()))
def test_hand_made_cases(name):
    mesh, m, counts, faces = hand_made()[name]
    out = MK.cluster(mesh, m, 16)
    assert out["counts"] == dict(counts, status=0), name
    got = out["mesh"]["keys"][out["mesh"]["faces"].astype(np.int64)]
    rot = lambda t: min((t[i:] + t[:i] for i in range(3)))  # smallest key first, winding kept
    assert sorted(rot(tuple(int(k) for k in t)) for t in got) == sorted(rot(t) for t in faces), name
    # every vertex of a cluster counts, with or without a face: the mean of cluster A's members in "same_winding"
    if name == "same_winding":
        a = out["mesh"]["vertices"][0]  # keys ascend: A first
        assert a.tolist() == [0.5, 0.5, 0.5]  # lattice points (0,0,0) and (1,1,1)


def test_the_mean_rounds_halves_up_on_signed_values():
    K = key_of
    keys = [K((-2, 0, 0)), K((-1, 0, 0)), K((2, 0, 0)), K((0, 2, 0))]
    v = np.array([[-1, 0, 0], [-2, 0, 0], [2, 0, 0], [0, 2, 0]], np.float32)
    out = MK.cluster(MK.plain_mesh(keys, [(0, 2, 3)], vertices=v), 2, 0)  # S = 1: the mean of -1 and -2 is floor((2 * -3 + 2) / 4) = -1
    assert out["mesh"]["vertices"][np.argmin(out["mesh"]["keys"])].tolist() == [-1.0, 0.0, 0.0]
    out = MK.cluster(MK.plain_mesh(keys, [(0, 2, 3)], vertices=-v), 2, 0)  # of 1 and 2: floor((6 + 2) / 4) = 2
    assert out["mesh"]["vertices"][np.argmin(out["mesh"]["keys"])].tolist() == [2.0, 0.0, 0.0]


def test_statuses_of_the_restatement():
    K = key_of
    keys = [K((0, 0, 0)), K((2, 0, 0)), K((0, 2, 0))]
    ok = MK.plain_mesh(keys, [(0, 1, 2)])
    assert MK.cluster(ok, 2, 16)["counts"] == dict(vertices=3, faces=1, status=0, collapsed=0, duplicates=0, unused_clusters=0)
    bad = MK.cluster(dict(ok, faces=np.array([[0, 1, 3]], np.uint32)), 2, 16)
    assert bad["status"] == MK.BAD_INDEX and set(bad["counts"].values()) == {0, MK.BAD_INDEX} and len(bad["mesh"]["keys"]) == 0
    assert MK.cluster(dict(ok, keys=np.array([keys[0], keys[1] | 1 << 62, keys[2]], np.uint64)), 2, 16)["status"] == MK.BAD_KEY
    far = dict(ok, vertices=np.array([[0, 0, 0], [1024.5, 0, 0], [0, 2, 0]], np.float32))
    assert MK.cluster(far, 2, 29)["status"] == 0 and MK.cluster(far, 2, 30)["status"] == MK.RANGE  # 1024.5 * 2^30 > 2^40
    assert MK.cluster(dict(ok, vertices=np.array([[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0]], np.float32)), 2, 16)["status"] == MK.RANGE
    assert MK.cluster(ok, 2, 16, cluster_slots_log2=1)["status"] == MK.TABLE_FULL and MK.cluster(ok, 2, 16, cluster_slots_log2=2)["status"] == 0
    two = MK.plain_mesh(keys + [K((2, 2, 0)), K((4, 4, 0))], [(0, 1, 2), (1, 3, 2), (1, 4, 3)])
    assert MK.cluster(two, 2, 16, face_slots_log2=1)["status"] == MK.TABLE_FULL and MK.cluster(two, 2, 16, face_slots_log2=2)["status"] == 0
    none = MK.cluster(dict(ok, faces=np.zeros((0, 3), np.uint32)), 2, 16)  # without a face every cluster is unused
    assert none["counts"] == dict(vertices=0, faces=0, status=0, collapsed=0, duplicates=0, unused_clusters=3)


# ---------------------------------------------------------------------------- 4. constants, prototypes, refusals, defaults

def test_constants_are_the_headers():
    from voxelhashing_amd import lib, vhtypes as T
    head = open(os.path.join(ROOT, "include", "vh_types.h")).read()
    for name, mine, theirs in (("TABLE_FULL", MK.TABLE_FULL, T.CLUSTER_TABLE_FULL), ("BAD_KEY", MK.BAD_KEY, T.CLUSTER_BAD_KEY), ("RANGE", MK.RANGE, T.CLUSTER_RANGE),
                               ("BAD_INDEX", MK.BAD_INDEX, T.CLUSTER_BAD_INDEX), ("MAX_CELLS", MK.MAX_CELLS, T.CLUSTER_MAX_CELLS)):
        assert int(re.search(r"#define VH_CLUSTER_%s (\d+)u" % name, head).group(1)) == mine == theirs
    enum = re.findall(r"VH_CLUSTER_(\w+) = (\d+)", head)
    assert [int(v) for _, v in enum] == list(range(7)) and [n for n, _ in enum] == ["VERTICES", "FACES", "STATUS", "COLLAPSED", "DUPLICATES", "UNUSED", "NUM_COUNTS"]
    assert T.CLUSTER_COUNTS == MK.COUNTS and len(T.CLUSTER_COUNTS) == 6
    for name in ("vh_mesh_cluster_key", "vh_mesh_cluster_default_scale_log2", "vh_mesh_cluster", "vh_mesh_weld_accum_cluster", "vh_mesh_weld_accum_cluster_get_counts",
                 "vh_mesh_weld_accum_cluster_download", "vh_marching_cubes_set_indexed_clustering", "vh_marching_cubes_get_indexed_cluster_stats"):
        assert name in lib.PROTOTYPES and lib.PROTOTYPES[name][0] is C.c_int
    # the ctypes mirror of the launcher's buffers against the C compiler's layout
    fields = re.search(r"typedef struct VhMeshClusterData \{(.*?)\} VhMeshClusterData;", head, re.S).group(1)
    names = re.findall(r"\b([dm]_\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [f[0] for f in T.MeshClusterData._fields_] and C.sizeof(T.MeshClusterData) == 13 * 8 + 8


def test_launchers_refuse_before_they_touch_the_device(vh):
    from voxelhashing_amd import vhtypes as T
    word = (C.c_uint32 * 8)(7)
    st = C.addressof(word)
    full = T.MeshClusterData(*([st] * 13), 6, 6)
    f = vh.vh_mesh_cluster
    assert f(None, None, None, 0, 0, 0, 0, None, None) == BAD_ARGUMENT
    assert f(st, st, st, 3, 1, 2, 21, None, None) == BAD_ARGUMENT                         # no buffers
    assert f(st, st, st, 3, 1, 0, 21, C.byref(full), None) == BAD_ARGUMENT                # m = 0
    assert f(st, st, st, 3, 1, 65, 21, C.byref(full), None) == BAD_ARGUMENT               # m = 65
    assert f(st, st, st, 3, 1, 2, 101, C.byref(full), None) == BAD_ARGUMENT and f(st, st, st, 3, 1, 2, -101, C.byref(full), None) == BAD_ARGUMENT
    assert f(None, st, st, 3, 1, 2, 21, C.byref(full), None) == BAD_ARGUMENT              # vertices without an array
    assert f(st, st, None, 3, 1, 2, 21, C.byref(full), None) == BAD_ARGUMENT              # faces without an array
    assert f(st, st, st, (1 << 30) + 1, 1, 2, 21, C.byref(full), None) == BAD_ARGUMENT
    assert f(st, st, st, 3, 1, 2, 21, C.byref(T.MeshClusterData(*([st] * 13), 32, 6)), None) == BAD_ARGUMENT
    holes = [st] * 13
    holes[0] = None
    assert f(st, st, st, 3, 1, 2, 21, C.byref(T.MeshClusterData(*holes, 6, 6)), None) == BAD_ARGUMENT  # no cluster table
    assert word[0] == 7
    assert vh.vh_mesh_weld_accum_cluster(None, 2, 21, None) == BAD_ARGUMENT
    assert vh.vh_mesh_weld_accum_cluster_get_counts(None, word, None) == BAD_ARGUMENT
    assert vh.vh_mesh_weld_accum_cluster_download(None, None, None, None, 0, 0, None) == BAD_ARGUMENT
    assert vh.vh_marching_cubes_set_indexed_clustering(None, 2) == BAD_ARGUMENT
    assert vh.vh_marching_cubes_get_indexed_cluster_stats(None, word) == BAD_ARGUMENT


def test_the_option_is_off_by_default_and_the_ply_has_no_new_property(tmp_path):
    """nothing of a mesh's file or dictionary changes unless the option is asked for"""
    from voxelhashing_amd import engine as E, reconstruction as R
    for fn in (R.Reconstruction.extractIsoSurface, R.Reconstruction.extractIsoSurfaceIndexed):
        assert inspect.signature(fn).parameters["cluster_cells"].default == 0
    assert inspect.signature(E.mesh_weld_appends).parameters["cluster_cells"].default == 0
    assert inspect.signature(E.CUDAMarchingCubesHashSDF.setIndexedClustering).parameters["cellsPerCluster"].default == 0
    # a clustered mesh is written like any indexed mesh: the same properties, its own counts
    m = MK.cluster(MW.weld(*MW.random_soup(257, 11)), 2, 21)["mesh"]
    colors = np.concatenate([m["colors"], np.ones((len(m["colors"]), 1), np.float32)], axis=1)
    E.mesh_save_ply(tmp_path / "c.ply", m["vertices"], colors, None, m["faces"])
    E.mesh_save_ply(tmp_path / "w.ply", m["vertices"][:3], colors[:3], None, m["faces"][:0])
    head = lambda p: open(p, "rb").read().split(b"end_header\n")[0].decode().split("\n")
    a, b = head(tmp_path / "c.ply"), head(tmp_path / "w.ply")
    assert "element vertex %d" % len(m["keys"]) in a and "element face %d" % len(m["faces"]) in a
    assert [l for l in a if l.startswith("property")] == [l for l in b if l.startswith("property")]


# ---------------------------------------------------------------------------- 5. what the kernels cost

def test_cluster_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    from voxelhashing_amd import lib
    rows = {r["kernel"].split("(")[0]: r for r in KR.library_resources(lib.LIB_PATH)}
    for name in ("k_cluster_insert", "k_cluster_faces", "k_cluster_number", "k_cluster_emit"):
        assert name in rows, sorted(k for k in rows if "mesh" in k or "weld" in k or "cluster" in k)
        r = rows[name]
        print(name, r)
        assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r["lds_bytes"] == 0
        assert r["vgprs"] <= 64  # eight waves per SIMD


# ---------------------------------------------------------------------------- 6. the replay tool

@pytest.mark.parametrize("flag, message", [(["--mesh-cluster", "2"], "--mesh-cluster needs --indexed-mesh"),
                                           (["--indexed-mesh", "--mesh-cluster", "1"], "--mesh-cluster: 2 ... 64"),
                                           (["--indexed-mesh", "--mesh-cluster", "65"], "--mesh-cluster: 2 ... 64"),
                                           (["--indexed-mesh", "--mesh-cluster", "-2"], "--mesh-cluster: 2 ... 64")])
def test_replay_refuses_bad_clustering_options(tmp_path, flag, message):
    """a usage error, before the tool looks for a GPU"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "replay.py"), "--params", str(tmp_path / "none.txt"), "--mesh", str(tmp_path / "m.ply")] + flag,
                       capture_output=True, text=True)
    assert r.returncode == 2 and message in r.stderr and not (tmp_path / "m.ply").exists()
