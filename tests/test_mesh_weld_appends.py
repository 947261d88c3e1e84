"""The accumulating weld without a GPU ("Indexed mesh over several extractions"): its numpy
restatement (tests/mesh_weld_appends.py) on hand-made soups split over appends and on random ones, the argument checks
of the new entry points, and what the new kernels cost in the built library."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import mesh_weld as MW
import mesh_weld_appends as MA
from voxelhashing_amd import vhtypes as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402


def vertex_of(mesh, key):
    i = int(np.searchsorted(mesh["keys"], np.uint64(key)))
    assert mesh["keys"][i] == key
    return i


# ---------------------------------------------------------------------------- the restatement

def test_shared_edge_takes_the_bits_of_the_second_append():
    parts = MA.split_cases()["shared_edge"]
    m = MA.weld_appends(parts)
    assert len(m["keys"]) == 5 and len(m["faces"]) == 2 and MA.dropped(parts) == 0
    late = parts[1][0]
    i = vertex_of(m, MW.pack_key((0, 0, 1), 0, 0))
    assert m["vertices"][i].tobytes() == late["v"]["p"][0, 0].tobytes() and m["colors"][i].tobytes() == late["v"]["c"][0, 0].tobytes()
    whole = MW.hand_made_cases()["shared_edge"]
    assert MW.same_mesh(m, MW.weld(whole[0], whole[1]))


@pytest.mark.parametrize("name", ["snapped_meet", "snapped_meet_reversed"])
def test_snapped_meet_one_triangle_per_append(name):
    parts = MA.split_cases()[name]
    assert [len(s) for s, _ in parts] == [1, 1, 1]
    m = MA.weld_appends(parts)
    whole = MW.hand_made_cases()["snapped_meet"]
    assert len(m["keys"]) == 7 and len(m["faces"]) == 3 and MW.same_mesh(m, MW.weld(whole[0], whole[1]))
    i = vertex_of(m, MW.pack_key((0, 0, 0), 5, 1))
    assert m["colors"][i].tobytes() == whole[0]["v"]["c"][0, 0].tobytes()  # cell (0, 0, 0), whichever append brings it


def test_a_cell_that_comes_back_with_other_triangles_vanishes():
    parts = MA.split_cases()["repeated_cell"]
    kept = MA.kept(parts)
    assert [len(s) for s, _ in kept] == [2, 1] and MA.dropped(parts) == 1
    assert kept[1][1]["cell"].tolist() == [[3, 2, 2]]
    m = MA.weld_appends(parts)
    gone = [MW.pack_key((2, 2, 2), e, 0) for e in (4, 5, 6)]  # the keys only the dropped triangle had
    assert not np.isin(np.array(gone, dtype=np.uint64), m["keys"]).any()
    # what is left: the first append's mesh (one face collapses) and the new cell's triangle, which shares the lattice
    # edge (3, 2..3, 2) with cell (2, 2, 2) and takes that cell's bits there
    first = MW.weld(*parts[0])
    assert len(m["faces"]) == len(first["faces"]) + 1 == 2 and len(m["keys"]) == len(first["keys"]) + 2 == 7
    shared = MW.pack_key((3, 2, 2), 3, 0)
    assert shared == MW.pack_key((2, 2, 2), 1, 0)
    assert m["vertices"][vertex_of(m, shared)].tobytes() == parts[0][0]["v"]["p"][1, 1].tobytes()


@pytest.mark.parametrize("n,seed,num_parts", [(1, 0, 1), (64, 1, 2), (500, 2, 5), (2000, 3, 5)])
def test_random_soup_split_by_cell_welds_as_the_whole(n, seed, num_parts):
    soup, srcs = MW.random_soup(n, seed, spread=3)
    want = MW.weld(soup, srcs)
    split = MA.deal(soup, srcs, num_parts, seed, repeat=0.0)
    assert sum(len(s) for s, _ in split) == n and MA.dropped(split) == 0
    assert MW.same_mesh(MA.weld_appends(split), want)
    # cells that come back whole as identical copies change nothing, in whatever order the appends come
    parts = MA.deal(soup, srcs, num_parts, seed)
    repeated = sum(len(s) for s, _ in parts) - n
    assert MA.dropped(parts) == repeated and (repeated > 0 or num_parts == 1 or n < 10)
    assert MW.same_mesh(MA.weld_appends(parts), want) and MW.same_mesh(MA.weld_appends(parts[::-1]), want)
    assert MA.num_cells(parts) == len(np.unique(srcs["cell"], axis=0))
    # copies with other bits lose: the first append that has the cell gives it its triangles
    other = MA.deal(soup, srcs, num_parts, seed, identical=False)
    assert MW.same_mesh(MA.weld_appends(other), want)
    if n >= 500:
        assert not MW.same_mesh(MA.weld_appends(other[::-1]), want)


def test_restatement_of_nothing():
    m = MA.weld_appends([])
    assert len(m["keys"]) == 0 and len(m["faces"]) == 0 and MA.dropped([]) == 0


# ---------------------------------------------------------------------------- the library, no GPU

def test_new_entry_points_refuse_bad_arguments():
    from voxelhashing_amd import lib
    L = lib.load()
    bad = 4  # VH_ERR_BAD_ARGUMENT
    h = C.c_void_p()
    assert L.vh_mesh_weld_accum_create(0, 0, 0, None) == bad
    assert L.vh_mesh_weld_accum_create(32, 0, 0, C.byref(h)) == bad and not h.value      # more than 2^31 slots
    assert L.vh_mesh_weld_accum_create(0, 0x55555555 // 2 + 1, 0, C.byref(h)) == bad and not h.value  # 3 n indices in 32 bits
    assert L.vh_mesh_weld_accum_begin(None, None) == bad
    assert L.vh_mesh_weld_accum_append(None, None, None, 0, None) == bad
    assert L.vh_mesh_weld_accum_get_counts(None, None, None) == bad
    assert L.vh_mesh_weld_accum_download(None, None, None, None, 0, 0, None) == bad
    L.vh_mesh_weld_accum_destroy(None)  # as free(NULL)
    assert L.vh_marching_cubes_begin_indexed(None) == bad
    assert L.vh_marching_cubes_append_indexed(None, None, None, None, None, 0) == bad
    assert L.vh_marching_cubes_finish_indexed(None) == bad
    assert L.vh_marching_cubes_extract_iso_surface_indexed_chunk_grid(None, None, None, 0.0) == bad
    assert L.vh_marching_cubes_get_indexed_stats(None, None) == bad
    for name in ("vh_mesh_weld_accum_create", "vh_mesh_weld_accum_destroy", "vh_mesh_weld_accum_begin", "vh_mesh_weld_accum_append",
                 "vh_mesh_weld_accum_get_counts", "vh_mesh_weld_accum_download", "vh_marching_cubes_begin_indexed",
                 "vh_marching_cubes_append_indexed", "vh_marching_cubes_finish_indexed",
                 "vh_marching_cubes_extract_iso_surface_indexed_chunk_grid", "vh_marching_cubes_get_indexed_stats"):
        assert name in lib.PROTOTYPES
    assert len(T.WELD_ACCUM_COUNTS) == 6 and T.WELD_ACCUM_COUNTS[2] == "status"


def test_count_indices_match_the_c_header():
    import subprocess
    import tempfile
    prog = r'''
#include <stdio.h>
#include "vh_types.h"
int main(void) {
  printf("%d %d %d %d %d %d %d %u\n", VH_WELD_ACCUM_VERTICES, VH_WELD_ACCUM_FACES, VH_WELD_ACCUM_STATUS, VH_WELD_ACCUM_CELLS,
         VH_WELD_ACCUM_DROPPED, VH_WELD_ACCUM_REHASHES, VH_WELD_ACCUM_NUM_COUNTS, VH_WELD_ACCUM_MAX_APPENDS);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    names = ("vertices", "faces", "status", "cells", "dropped", "rehashes")
    assert out[:6] == [T.WELD_ACCUM_COUNTS.index(n) for n in names] and out[6] == len(T.WELD_ACCUM_COUNTS)
    assert out[7] == T.WELD_ACCUM_MAX_APPENDS


def test_new_kernels_use_no_scratch_and_spill_nothing():
    from voxelhashing_amd import lib
    rows = {r["kernel"].split("(")[0]: r for r in KR.library_resources(lib.LIB_PATH)}
    for name in ("k_weld_accum_insert", "k_weld_accum_settle", "k_weld_accum_faces", "k_weld_rehash"):
        assert name in rows, f"{name} is not in the library: {sorted(k for k in rows if 'weld' in k)}"
        r = rows[name]
        print(name, r)
        assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r["lds_bytes"] == 0, (name, r)
