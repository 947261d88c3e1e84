"""Connected components of the indexed mesh, without a GPU ("Mesh components"): the numpy
restatement (tests/mesh_components.py) on hand-made meshes, its independence of face order, of the rotation of a triple
and of the vertex numbers, the edges of the filter, the constants and prototypes, the refusals through the library,
what the kernels cost, and the replay tool's usage errors."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mesh_components as MC
import mesh_weld as MW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARGUMENT = 4  # VH_ERR_BAD_ARGUMENT


# ---------------------------------------------------------------------------- 1. hand-made meshes

def test_two_triangles_on_an_edge_a_separate_one_and_a_faceless_vertex():
    # vertices 0-3: two triangles on the edge (1, 2); 4-6: one triangle; 7: no face.  Keys descend, so roots are the LAST indices
    keys = np.array([80, 70, 60, 50, 40, 30, 20, 10], dtype=np.uint64)
    faces = [(0, 1, 2), (2, 1, 3), (4, 5, 6)]
    root, count, status = MC.components(keys, faces)
    assert status == 0 and root.tolist() == [3, 3, 3, 3, 6, 6, 6, 7] and count.tolist() == [0, 0, 0, 2, 0, 0, 1, 0]
    out = MC.filter(MC.plain_mesh(keys, faces))
    assert out["counts"] == dict(components=2, faceless_vertices=1, kept_components=2, kept_vertices=8, kept_faces=3, largest_faces=2)
    out = MC.filter(MC.plain_mesh(keys, faces), 1)  # with minFaces >= 1 the faceless vertex goes
    assert out["counts"]["kept_vertices"] == 7 and out["counts"]["kept_faces"] == 3 and 10 not in out["mesh"]["keys"]


def test_a_bow_tie_is_one_component():
    keys = np.array([5, 9, 7, 3, 8], dtype=np.uint64)  # two triangles that share vertex 0 alone
    root, count, status = MC.components(keys, [(0, 1, 2), (3, 0, 4)])
    assert status == 0 and root.tolist() == [3] * 5 and count.tolist() == [0, 0, 0, 2, 0]


def test_equal_keys_are_settled_by_the_index():
    keys = np.full(6, 42, dtype=np.uint64)
    root, count, _ = MC.components(keys, [(5, 4, 3), (2, 1, 0)])
    assert root.tolist() == [0, 0, 0, 3, 3, 3] and count.tolist() == [1, 0, 0, 1, 0, 0]
    # a tie for the largest goes to the earlier root: index 0
    out = MC.filter(MC.plain_mesh(keys, [(5, 4, 3), (2, 1, 0)]), 0, True)
    assert out["counts"]["kept_vertices"] == 3 and out["counts"]["kept_faces"] == 1 and out["counts"]["kept_components"] == 1
    assert out["mesh"]["faces"].tolist() == [[0, 2, 1]]  # (2, 1, 0) renumbered by itself and rotated by canonical()


def test_a_repeated_index_joins_and_counts_once():
    keys = np.array([4, 3, 2, 1], dtype=np.uint64)
    root, count, status = MC.components(keys, [(0, 0, 1), (2, 3, 2)])
    assert status == 0 and root.tolist() == [1, 1, 3, 3] and count.tolist() == [0, 1, 0, 1]
    root, count, status = MC.components(keys, [(0, 0, 0)])  # joins nothing, counts as one face
    assert root.tolist() == [0, 1, 2, 3] and count.tolist() == [1, 0, 0, 0]


def test_a_bad_index_is_a_status_and_the_face_joins_nothing():
    keys = np.array([4, 3, 2, 1], dtype=np.uint64)
    root, count, status = MC.components(keys, [(0, 1, 4), (2, 3, 3)])
    assert status == MC.BAD_INDEX and root.tolist() == [0, 1, 3, 3] and count.tolist() == [0, 0, 0, 1]
    out = MC.filter(MC.plain_mesh(keys, [(0, 1, 4), (2, 3, 3)]))
    assert set(out["counts"].values()) == {0} and len(out["mesh"]["keys"]) == 0 and len(out["mesh"]["faces"]) == 0


# ---------------------------------------------------------------------------- 2. what the restatement does not depend on

@pytest.fixture(scope="module")
def welded():
    m = MW.weld(*MC.archipelago())
    return m, MC.filter(m)


def test_restatement_does_not_depend_on_face_order_rotation_or_vertex_numbers(welded):
    m, base = welded
    assert base["counts"]["components"] >= 6 and base["counts"]["largest_faces"] > 200
    rng = np.random.default_rng(3)
    f = m["faces"][rng.permutation(len(m["faces"]))]
    r = rng.integers(0, 3, len(f))
    f = np.stack([f[np.arange(len(f)), (r + k) % 3] for k in range(3)], axis=1)
    assert len(np.unique(r)) == 3
    other = MC.filter(dict(m, faces=f), 5)
    want = MC.filter(m, 5)
    assert np.array_equal(other["root"], want["root"]) and np.array_equal(other["face_count"], want["face_count"])
    assert other["counts"] == want["counts"] and MW.same_mesh(other["mesh"], want["mesh"])
    # other vertex numbers: roots are compared by key
    p = rng.permutation(len(m["keys"]))
    inv = np.empty_like(p)
    inv[p] = np.arange(len(p))
    renumbered = dict(vertices=m["vertices"][p], colors=m["colors"][p], keys=m["keys"][p], faces=inv[m["faces"].astype(np.int64)].astype(np.uint32))
    again = MC.filter(renumbered, 5)
    assert np.array_equal(MC.root_keys(renumbered["keys"], again["root"])[inv], MC.root_keys(m["keys"], want["root"]))
    assert np.array_equal(again["face_count"][inv], want["face_count"])
    assert again["counts"] == want["counts"] and MW.same_mesh(again["mesh"], want["mesh"])


def test_a_root_is_the_smallest_key_of_its_component_and_counts_add_up(welded):
    m, base = welded
    root, count = base["root"].astype(np.int64), base["face_count"]
    assert np.all(m["keys"][root] <= m["keys"]) and np.all(root[root] == root)
    assert np.all(root[m["faces"][:, 0]] == root[m["faces"][:, 1]]) and np.all(root[m["faces"][:, 1]] == root[m["faces"][:, 2]])
    assert int(count.sum()) == len(m["faces"]) and not count[root != np.arange(len(root))].any()
    assert base["counts"]["components"] + base["counts"]["faceless_vertices"] == len(np.unique(root))


# ---------------------------------------------------------------------------- 3. the filter's edges

def test_filter_edges(welded):
    m, base = welded
    sizes = MC.sizes(base["face_count"])
    second = int(sizes[1])
    assert sizes[0] > second > sizes[-1]
    at = MC.filter(m, second)  # minFaces equal to a component's size keeps it ...
    above = MC.filter(m, second + 1)  # ... one more drops it
    n_second = int((sizes == second).sum())
    assert at["counts"]["kept_components"] == int((sizes >= second).sum()) == above["counts"]["kept_components"] + n_second
    assert at["counts"]["kept_faces"] == int(sizes[sizes >= second].sum()) == above["counts"]["kept_faces"] + n_second * second
    largest = MC.filter(m, 0, True)
    assert largest["counts"]["kept_components"] == 1 and largest["counts"]["kept_faces"] == int(sizes[0]) == largest["counts"]["largest_faces"]
    nothing = MC.filter(m, int(sizes[0]) + 1)  # a threshold above everything gives an empty mesh
    assert nothing["counts"]["kept_vertices"] == 0 == nothing["counts"]["kept_faces"] and nothing["counts"]["components"] == base["counts"]["components"]
    assert len(nothing["mesh"]["keys"]) == 0 and nothing["mesh"]["faces"].shape == (0, 3)
    both = MC.filter(m, int(sizes[0]) + 1, True)  # the largest must also reach the threshold
    assert both["counts"]["kept_vertices"] == 0
    # the filter off keeps everything, the faceless vertices too
    assert base["counts"]["kept_vertices"] == len(m["keys"]) and base["counts"]["kept_faces"] == len(m["faces"]) and MW.same_mesh(base["mesh"], MW.canonical(m))
    # without a face nothing is the largest
    assert MC.filter(dict(m, faces=np.zeros((0, 3), dtype=np.uint32)), 0, True)["counts"]["kept_vertices"] == 0


def test_a_tie_for_the_largest_goes_to_the_earlier_root():
    m = MW.weld(*MW.random_soup(22, 32, isolated=True))  # 22 components of one face
    out = MC.filter(m, 0, True)
    assert out["counts"] == dict(components=22, faceless_vertices=0, kept_components=1, kept_vertices=3, kept_faces=1, largest_faces=1)
    assert out["mesh"]["keys"][0] == m["keys"].min()


# ---------------------------------------------------------------------------- 4. constants, prototypes, refusals

def test_constants_are_the_headers():
    from voxelhashing_amd import lib, vhtypes as T
    head = open(os.path.join(ROOT, "include", "vh_types.h")).read()
    assert int(re.search(r"#define VH_COMPONENTS_BAD_INDEX (\d+)u", head).group(1)) == T.COMPONENTS_BAD_INDEX == MC.BAD_INDEX == 1
    assert int(re.search(r"#define VH_COMPONENTS_STEPS (\d+)u", head).group(1)) == T.COMPONENTS_STEPS == MC.STEPS == 2
    enum = re.findall(r"VH_COMPONENTS_(\w+) = (\d+)", head)
    assert [int(v) for _, v in enum] == list(range(7)) and enum[-1][0] == "NUM_COUNTS"
    assert len(T.COMPONENTS_COUNTS) == 6 and T.COMPONENTS_COUNTS == MC.COUNTS
    for name in ("vh_mesh_components", "vh_mesh_components_filter", "vh_mesh_weld_accum_components", "vh_mesh_weld_accum_components_get_counts",
                 "vh_mesh_weld_accum_components_download", "vh_marching_cubes_set_indexed_component_filter", "vh_marching_cubes_get_indexed_component_stats"):
        assert name in lib.PROTOTYPES and lib.PROTOTYPES[name][0] is C.c_int


def test_launchers_refuse_before_they_touch_the_device(vh):
    word = (C.c_uint32 * 8)(7)
    st = C.addressof(word)
    assert vh.vh_mesh_components(None, None, 0, 0, None, None, None, None) == BAD_ARGUMENT          # no status word
    assert vh.vh_mesh_components(None, None, 3, 0, None, None, st, None) == BAD_ARGUMENT            # vertices without arrays
    assert vh.vh_mesh_components(st, None, 3, 1, st, st, st, None) == BAD_ARGUMENT                  # faces without an array
    assert vh.vh_mesh_components(st, st, 0x7ffffff1, 1, st, st, st, None) == BAD_ARGUMENT           # 2 V + 4 steps in 32 bits
    assert vh.vh_mesh_components(st, st, 3, 0x55555556, st, st, st, None) == BAD_ARGUMENT
    f = vh.vh_mesh_components_filter
    assert f(None, None, None, None, 0, 0, None, None, None, 0, 0, None, None, None, None, None, None, None, None) == BAD_ARGUMENT
    assert f(None, None, None, None, 3, 0, None, None, st, 1, 0, None, st, None, None, None, None, st, None) == BAD_ARGUMENT   # vertices without arrays
    assert f(st, st, st, None, 3, 0, st, st, st, 1, 0, st, st, st, st, None, None, st, None) == BAD_ARGUMENT                 # normals in, none out
    assert f(st, st, None, st, 3, 1, st, st, st, 1, 0, st, st, st, st, None, None, st, None) == BAD_ARGUMENT                 # faces in, none out
    assert word[0] == 7
    assert vh.vh_mesh_weld_accum_components(None, 1, 0, None) == BAD_ARGUMENT
    assert vh.vh_mesh_weld_accum_components_get_counts(None, word, None) == BAD_ARGUMENT
    assert vh.vh_mesh_weld_accum_components_download(None, None, None, None, None, 0, 0, None) == BAD_ARGUMENT
    assert vh.vh_marching_cubes_set_indexed_component_filter(None, 100, 1) == BAD_ARGUMENT
    assert vh.vh_marching_cubes_get_indexed_component_stats(None, word) == BAD_ARGUMENT


# ---------------------------------------------------------------------------- 5. what the kernels cost

def test_component_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    from voxelhashing_amd import lib
    rows = {r["kernel"].split("(")[0]: r for r in KR.library_resources(lib.LIB_PATH)}
    for name in ("k_components_init", "k_components_hook", "k_components_flatten", "k_components_count", "k_components_stats", "k_components_pick",
                 "k_components_compact_vertices", "k_components_compact_faces"):
        assert name in rows, sorted(k for k in rows if "mesh" in k or "weld" in k or "components" in k)
        r = rows[name]
        print(name, r)
        assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r["lds_bytes"] == 0
        assert r["vgprs"] <= 64  # eight waves per SIMD


# ---------------------------------------------------------------------------- 6. the replay tool

@pytest.mark.parametrize("flag, message", [(["--mesh-min-component", "100"], "--mesh-min-component needs --indexed-mesh"),
                                           (["--mesh-largest-component"], "--mesh-largest-component needs --indexed-mesh")])
def test_replay_refuses_the_component_filter_without_an_indexed_mesh(tmp_path, flag, message):
    """a usage error, before the tool looks for a GPU"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "replay.py"), "--params", str(tmp_path / "none.txt"), "--mesh", str(tmp_path / "m.ply")] + flag,
                       capture_output=True, text=True)
    assert r.returncode == 2 and message in r.stderr and not (tmp_path / "m.ply").exists()
