"""The indexed mesh without a GPU: the numpy restatement (tests/mesh_weld.py) on hand-made soups, its canonical form,
and the library's key packing (vh_mesh_weld_key) against the restatement's."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mesh_weld as MW
from voxelhashing_amd import vhtypes as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = (1 << 19) - 1


def key_of(cell, edge, snap):
    from voxelhashing_amd import engine as E, lib
    try:
        return E.mesh_weld_key(cell, edge, snap)
    except lib.VhError as e:
        assert e.code == 4  # VH_ERR_BAD_ARGUMENT
        return None


# ---------------------------------------------------------------------------- the restatement

@pytest.mark.parametrize("name", ["shared_edge", "snapped_meet", "snap_disagreement", "collapsing_face"])
def test_restatement_on_hand_made_soups(name):
    soup, srcs, nv, nf = MW.hand_made_cases()[name]
    m = MW.weld(soup, srcs)
    assert len(m["vertices"]) == nv and len(m["faces"]) == nf and len(m["keys"]) == nv
    assert np.all(np.diff(m["keys"].astype(np.int64)) > 0)  # sorted, distinct (bit 63 is never set)
    if name == "shared_edge":
        # the lattice edge both cells touch: one vertex, with the bits of the lower cell (z first) = the second triangle
        k = MW.pack_key((0, 0, 1), 0, 0)
        assert k == MW.pack_key((0, 0, 0), 4, 0)
        i = int(np.searchsorted(m["keys"], np.uint64(k)))
        assert m["vertices"][i].tobytes() == soup["v"]["p"][1, 0].tobytes() and m["colors"][i].tobytes() == soup["v"]["c"][1, 0].tobytes()
    if name == "snapped_meet":
        k = MW.pack_key((0, 0, 0), 5, 1)
        assert k == MW.pack_key((1, 1, 1), 3, 1) == MW.pack_key((0, 1, 0), 10, 2) and k >> 60 == MW.POINT
        i = int(np.searchsorted(m["keys"], np.uint64(k)))
        assert m["colors"][i].tobytes() == soup["v"]["c"][0, 0].tobytes()  # cell (0, 0, 0) is the smallest
        assert all(i in f for f in m["faces"])
    if name == "snap_disagreement":
        assert MW.pack_key((0, 0, 0), 4, 1) != MW.pack_key((0, 0, 1), 0, 0)
    if name == "collapsing_face":
        assert m["dropped_faces"] == 1


def test_winding_is_kept_and_the_smallest_index_leads():
    f = MW.canonical_faces([[5, 2, 9], [7, 8, 1], [3, 4, 6]])
    assert f.tolist() == [[1, 7, 8], [2, 9, 5], [3, 4, 6]]  # rotations, never a swap


@pytest.mark.parametrize("n,seed", [(1, 0), (22, 1), (257, 2)])
def test_canonical_form_does_not_depend_on_triangle_order(n, seed):
    soup, srcs = MW.random_soup(n, seed)
    # (vertices of one cell under one key carry the same bits in a real soup; the random one gets that by copying)
    keys, _ = MW.vertex_keys(srcs)
    cell = np.repeat(srcs["cell"], 3, axis=0)
    tag = np.concatenate([keys[:, None].view(np.uint32).reshape(-1, 2), cell.view(np.uint32)], axis=1)
    _, first, inv = np.unique(tag, axis=0, return_index=True, return_inverse=True)
    flat_p, flat_c = soup["v"]["p"].reshape(-1, 3), soup["v"]["c"].reshape(-1, 3)
    soup["v"]["p"] = flat_p[first[inv.ravel()]].reshape(n, 3, 3)
    soup["v"]["c"] = flat_c[first[inv.ravel()]].reshape(n, 3, 3)
    want = MW.weld(soup, srcs)
    perm = np.random.default_rng(seed + 100).permutation(n)
    assert MW.same_mesh(MW.weld(soup[perm], srcs[perm]), want)
    # and a mesh whose vertices and faces come in another order has the same canonical form
    vperm = np.random.default_rng(seed + 200).permutation(len(want["keys"]))
    inv_v = np.argsort(vperm)
    shuffled = dict(vertices=want["vertices"][vperm], colors=want["colors"][vperm], keys=want["keys"][vperm],
                    faces=np.roll(inv_v[want["faces"].astype(np.int64)][::-1], 1, axis=1))
    assert MW.same_mesh(MW.canonical(shuffled), want)


def test_restatement_refuses_a_vertex_without_key():
    soup, srcs = MW.random_soup(4, 3)
    srcs["cell"][2] = (1 << 19, 0, 0)
    with pytest.raises(MW.KeyRange):
        MW.weld(soup, srcs)


# ---------------------------------------------------------------------------- the library's packing

CELLS = [(0, 0, 0), (-3, 7, 11), (5, -9, -1), (-120000, 250000, -7), (LIMIT, LIMIT, LIMIT), (-LIMIT, -LIMIT, -LIMIT),
         (LIMIT, -LIMIT, 0), (-(1 << 19), -(1 << 19), -(1 << 19))]


def test_key_equals_the_restatement():
    seen, refused = set(), 0
    for cell in CELLS:
        for edge in range(12):
            for snap in range(3):
                want = MW.pack_key(cell, edge, snap)
                assert key_of(cell, edge, snap) == want, (cell, edge, snap)
                if want is None:
                    refused += 1
                else:
                    assert want >> 62 == 0
                    seen.add(want)
    # a cell at 2^19 - 1 has keys only on the lattice points that are its own coordinates: the others are one past the range
    assert refused > 0 and len(seen) > 100
    assert MW.pack_key((LIMIT,) * 3, 3, 1) is not None and MW.pack_key((LIMIT,) * 3, 5, 1) is None
    # the layout the header documents
    assert MW.pack_key((1, 2, 3), 11, 0) == (1 + (1 << 19)) | (2 + (1 << 19)) << 20 | (3 + (1 << 19)) << 40 | 2 << 60
    assert key_of((1, 2, 3), 11, 0) == MW.pack_key((1, 2, 3), 11, 0)


def test_key_is_refused_one_step_beyond_the_range():
    for axis in range(3):
        hi, lo = [0, 0, 0], [0, 0, 0]
        hi[axis], lo[axis] = 1 << 19, -(1 << 19) - 2
        for edge in range(12):
            for snap in range(3):
                assert key_of(hi, edge, snap) is None and MW.pack_key(hi, edge, snap) is None
                assert key_of(lo, edge, snap) is None and MW.pack_key(lo, edge, snap) is None
        # -(2^19) - 1: the lattice points one up are in range again, the cell's own are not
        edge_lo = [0, 0, 0]
        edge_lo[axis] = -(1 << 19) - 1
        got = [key_of(edge_lo, e, s) for e in range(12) for s in range(3)]
        assert got == [MW.pack_key(edge_lo, e, s) for e in range(12) for s in range(3)]
        assert any(k is None for k in got) and any(k is not None for k in got)


def test_key_refuses_bad_edge_and_snap():
    for edge, snap in [(12, 0), (15, 1), (255, 0), (0, 3), (11, 7), (1 << 31, 0)]:
        assert key_of((0, 0, 0), edge, snap) is None and MW.pack_key((0, 0, 0), edge, snap) is None
    from voxelhashing_amd import lib
    L = lib.load()
    key = C.c_uint64()
    assert L.vh_mesh_weld_key(None, 0, 0, C.byref(key)) == 4 and L.vh_mesh_weld_key((C.c_int32 * 3)(0, 0, 0), 0, 0, None) == 4


def test_default_table_size():
    """the smallest power of two >= 6 n"""
    from voxelhashing_amd import lib
    L = lib.load()
    out = C.c_uint32()
    for n, want in [(0, 6), (10, 6), (11, 7), (257, 11), (341, 11), (342, 12), (2500000, 24)]:
        assert L.vh_mesh_weld_default_slots_log2(n, C.byref(out)) == 0 and out.value == want, n
        assert (1 << want) >= 6 * n and (want == 6 or (1 << (want - 1)) < 6 * n)


def test_new_struct_layouts_match_the_c_header():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "vh_types.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(VhTriangleSource), offsetof(VhTriangleSource, edges), sizeof(VhMeshWeldData),
         offsetof(VhMeshWeldData, d_counts), offsetof(VhMeshWeldData, d_faces), offsetof(VhMeshWeldData, m_maxTriangles),
         offsetof(VhMeshWeldData, m_slotsLog2), sizeof(VhVertex));
  printf("%u %u\n", VH_WELD_TABLE_FULL, VH_WELD_KEY_RANGE);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    assert [int(v) for v in out[0].split()] == [
        C.sizeof(T.TriangleSource), T.TriangleSource.edges.offset, C.sizeof(T.MeshWeldData), T.MeshWeldData.d_counts.offset,
        T.MeshWeldData.d_faces.offset, T.MeshWeldData.m_maxTriangles.offset, T.MeshWeldData.m_slotsLog2.offset, T.VERTEX_DTYPE.itemsize]
    assert C.sizeof(T.TriangleSource) == 16 == T.TRIANGLE_SOURCE_DTYPE.itemsize and T.TRIANGLE_SOURCE_DTYPE.fields["edges"][1] == 12
    assert [int(v) for v in out[1].split()] == [T.WELD_TABLE_FULL, T.WELD_KEY_RANGE]
