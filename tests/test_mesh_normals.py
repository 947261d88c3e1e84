"""Vertex normals of the indexed mesh, without a GPU ("Vertex normals"): the default scale and the
refusals through the library, the numpy restatement (tests/mesh_normals.py) against a float64 area-weighted reference
within a derived bound, its independence of face order and of the rotation of a triple, the mesh container's PLY
layout and its rule for normals under a transform, and what the two kernels cost."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import mesh_normals as MN
import mesh_weld as MW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARGUMENT = 4  # VH_ERR_BAD_ARGUMENT
SCALE = 30


# ---------------------------------------------------------------------------- 1. the default scale, the refusals

@pytest.mark.parametrize("voxel_size, want", [(0.004, 53), (0.01, 51), (0.02, 49), (0.04, 47), (0.05, 46), (0.25, 42), (0.5, 40), (1.0, 38)])
def test_default_scale_known_answers(vh, voxel_size, want):
    from voxelhashing_amd import engine as E
    assert E.mesh_normals_default_scale_log2(voxel_size) == want
    # 38 - ceil(log2(v)) with v the double product of the float32 voxel size with itself
    vs = float(np.float32(voxel_size))
    m, e = np.frexp(vs * vs)
    assert want == 38 - (e - 1 if m == 0.5 else e)


def test_default_scale_keeps_a_cell_sized_triangle_in_range(vh):
    """|a x b| <= 3 vs^2 for a triangle inside one cell, so every scaled component stays below 2^40"""
    from voxelhashing_amd import engine as E
    for vs in (0.004, 0.01, 0.0123, 0.02, 0.05, 0.3, 1.0, 7.5):
        s = E.mesh_normals_default_scale_log2(vs)
        v = float(np.float32(vs)) ** 2
        assert 2.0 ** 37 < v * 2.0 ** s <= 2.0 ** 38 and 3 * v * 2.0 ** s < 2.0 ** 40


@pytest.mark.parametrize("voxel_size", [0.0, -0.02, float("inf"), float("-inf"), float("nan")])
def test_default_scale_refuses_a_voxel_size_that_is_none(vh, voxel_size):
    from voxelhashing_amd import engine as E, lib
    out = C.c_int32(12345)
    assert vh.vh_mesh_normals_default_scale_log2(voxel_size, C.byref(out)) == BAD_ARGUMENT and out.value == 12345
    assert vh.vh_mesh_normals_default_scale_log2(0.02, None) == BAD_ARGUMENT
    with pytest.raises(lib.VhError) as e:
        E.mesh_normals_default_scale_log2(voxel_size)
    assert e.value.code == BAD_ARGUMENT


def test_launcher_refuses_before_it_touches_the_device(vh):
    """scaleLog2 outside [-100, 100], and missing arrays: refused by the argument checks, which come before any HIP call"""
    word = (C.c_uint32 * 1)(7)
    st = C.addressof(word)
    for scale in (101, -101, 1 << 20, -(1 << 31)):
        assert vh.vh_mesh_vertex_normals(None, None, None, 0, 0, scale, None, None, st, None) == BAD_ARGUMENT
    assert vh.vh_mesh_vertex_normals(None, None, None, 0, 0, 30, None, None, None, None) == BAD_ARGUMENT   # no status word
    assert vh.vh_mesh_vertex_normals(None, None, None, 3, 0, 30, None, None, st, None) == BAD_ARGUMENT     # vertices without arrays
    assert vh.vh_mesh_vertex_normals(st, st, None, 3, 1, 30, st, st, st, None) == BAD_ARGUMENT             # faces without an array
    assert word[0] == 7
    assert vh.vh_mesh_weld_accum_normals(None, 30, None) == BAD_ARGUMENT
    assert vh.vh_mesh_weld_accum_download_normals(None, None, 0, None) == BAD_ARGUMENT
    assert vh.vh_marching_cubes_set_indexed_normals(None, 1) == BAD_ARGUMENT
    assert vh.vh_marching_cubes_download_indexed_normals(None, None) == BAD_ARGUMENT


def test_status_bits_are_the_headers():
    from voxelhashing_amd import vhtypes as T
    head = open(os.path.join(ROOT, "include", "vh_types.h")).read()
    assert int(re.search(r"#define VH_NORMALS_RANGE (\d+)u", head).group(1)) == T.NORMALS_RANGE == MN.RANGE == 1
    assert int(re.search(r"#define VH_NORMALS_BAD_INDEX (\d+)u", head).group(1)) == T.NORMALS_BAD_INDEX == MN.BAD_INDEX == 2


# ---------------------------------------------------------------------------- 2. the restatement against float64

@pytest.fixture(scope="module")
def welded():
    """(n, seed) -> the welded random soup and the restatement's normals at SCALE; made once"""
    out = {}
    for n, seed in ((257, 267), (2000, 3)):
        m = MW.weld(*MW.random_soup(n, seed))
        out[n] = dict(mesh=m, got=MN.vertex_normals(m["vertices"], m["keys"], m["faces"], SCALE))
    return out


@pytest.mark.parametrize("n, without_face, valence", [(257, 6, 4), (2000, 1, 16)])
def test_restatement_stays_within_the_derived_bound(welded, n, without_face, valence):
    """|n - A / |A|| <= 2 E / |A| + 2^-22 with E = sum over the vertex's faces of 2^-20 |a| |b| + sqrt(3) / S: float32
    rounding of two subtractions and a two-term product difference, half a unit of quantisation per component, the final
    rounding to float.  Derived, not measured; both soups use about 4 % of it."""
    m, got = welded[n]["mesh"], welded[n]["got"]
    assert got["status"] == 0
    assert MN.vertex_normals(m["vertices"], m["keys"], m["faces"], 36)["status"] == 0  # no face out of range at 30 or at 36
    ratio, unit = MN.check_against_reference(got["normals"], m["vertices"], m["faces"], SCALE)
    print(n, "error / bound", ratio, "| |n| - 1 |", unit)
    A, _, val = MN.reference(m["vertices"], m["faces"], SCALE)
    assert int((val == 0).sum()) == without_face and int(val.max()) == valence
    zero = ~np.any(got["normals"] != 0, axis=1)
    assert np.array_equal(zero, val == 0)  # vertices all of whose faces collapsed, and no others
    assert np.all(got["acc"][val == 0] == 0)


@pytest.mark.parametrize("n", [257, 2000])
def test_restatement_does_not_depend_on_order(welded, n):
    m, got = welded[n]["mesh"], welded[n]["got"]
    rng = np.random.default_rng(n)
    f = m["faces"][rng.permutation(len(m["faces"]))]
    permuted = MN.vertex_normals(m["vertices"], m["keys"], f, SCALE)
    rows = np.arange(len(f))
    r = rng.integers(0, 3, len(f))
    rotated = np.stack([f[rows, (r + k) % 3] for k in range(3)], axis=1)
    assert len(np.unique(r)) == 3
    turned = MN.vertex_normals(m["vertices"], m["keys"], rotated, SCALE)
    for other in (permuted, turned):
        assert other["acc"].tobytes() == got["acc"].tobytes() and other["normals"].tobytes() == got["normals"].tobytes()
    # the winding is not a rotation: it turns every normal round
    flipped = MN.vertex_normals(m["vertices"], m["keys"], f[:, ::-1], SCALE)
    assert np.array_equal(flipped["acc"], -got["acc"])


def test_restatement_reports_range_and_index():
    m = MW.weld(*MW.random_soup(257, 267))
    V = len(m["keys"])
    out = MN.vertex_normals(m["vertices"], m["keys"], m["faces"], 60)
    assert out["status"] == MN.RANGE and not out["normals"].any()
    f = m["faces"].copy()
    f[100, 1] = V
    out = MN.vertex_normals(m["vertices"], m["keys"], f, SCALE)
    assert out["status"] == MN.BAD_INDEX and not out["normals"].any()
    assert MN.vertex_normals(m["vertices"], m["keys"], f, 60)["status"] == MN.RANGE | MN.BAD_INDEX


# ---------------------------------------------------------------------------- 3. the PLY, and normals under a transform

def read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    props = re.findall(rb"property (?:float|uchar) (\w+)", head.split(b"element face")[0])
    nv = int(re.search(rb"element vertex (\d+)", head).group(1))
    nf = int(re.search(rb"element face (\d+)", head).group(1))
    fields = [("p", "<f4", 3)] + ([("n", "<f4", 3)] if b"nx" in props else []) + ([("c", "u1", 4)] if b"red" in props else [])
    dt = np.dtype(fields)
    assert len(body) == nv * dt.itemsize + nf * 13
    verts = np.frombuffer(body[:nv * dt.itemsize], dtype=dt)
    faces = np.frombuffer(body[nv * dt.itemsize:], dtype=np.dtype([("k", "u1"), ("i", "<i4", 3)]))
    return [p.decode() for p in props], verts, faces["i"]


@pytest.fixture(scope="module")
def small_mesh():
    m = MW.weld(*MW.random_soup(257, 267))
    n = MN.vertex_normals(m["vertices"], m["keys"], m["faces"], SCALE)["normals"]
    colors = np.concatenate([m["colors"], np.ones((len(n), 1), dtype=np.float32)], axis=1)
    return dict(m, normals=n, colors4=colors)


def test_ply_layout_with_and_without_normals(vh, small_mesh, tmp_path):
    from voxelhashing_amd import engine as E
    m = small_mesh
    V, F = len(m["keys"]), len(m["faces"])
    with_n, without = str(tmp_path / "n.ply"), str(tmp_path / "plain.ply")
    E.mesh_save_ply(with_n, m["vertices"], m["colors4"], m["normals"], m["faces"])
    E.mesh_save_ply(without, m["vertices"], m["colors4"], None, m["faces"])
    props, verts, faces = read_ply(with_n)
    assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "alpha"]
    assert verts.dtype.itemsize == 28 and len(verts) == V and len(faces) == F
    assert verts["p"].tobytes() == m["vertices"].tobytes() and verts["n"].tobytes() == m["normals"].tobytes()
    assert np.array_equal(faces.astype(np.uint32), m["faces"])
    props0, verts0, faces0 = read_ply(without)
    assert props0 == ["x", "y", "z", "red", "green", "blue", "alpha"] and verts0.dtype.itemsize == 16
    assert verts0["p"].tobytes() == verts["p"].tobytes() and verts0["c"].tobytes() == verts["c"].tobytes()
    assert np.array_equal(faces0, faces)
    # an index list that is no list of triples is refused
    assert vh.vh_mesh_save_ply(m["vertices"].ctypes.data, None, None, V, None, 1, None, with_n.encode()) == BAD_ARGUMENT  # 1 index is no face


def rotation(axis, angle):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def transformed(E, m, A, t, path):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = A, t
    E.mesh_save_ply(path, m["vertices"], m["colors4"], m["normals"], m["faces"], transform=M.astype(np.float32))
    _, verts, faces = read_ply(path)
    assert np.array_equal(faces.astype(np.uint32), m["faces"])  # the faces keep their index order
    return M.astype(np.float32).astype(np.float64), verts


def test_rigid_transform_with_a_translation_turns_the_normals(vh, small_mesh, tmp_path):
    """mLib sends normals through the point operator of the inverse transpose, which divides them by a w that holds the
    translation; here a translation does nothing to a normal, and a rotation turns it"""
    from voxelhashing_amd import engine as E
    m = small_mesh
    R = rotation((1.0, -2.0, 0.5), 0.9)
    M, verts = transformed(E, m, R, (3.5, -120.0, 41.0), str(tmp_path / "rigid.ply"))
    n0, n1 = m["normals"].astype(np.float64), verts["n"].astype(np.float64)
    has = np.any(n0 != 0, axis=1)
    assert has.sum() == len(n0) - 6 and not n1[~has].any()  # zero stays zero
    assert np.abs(np.linalg.norm(n1[has], axis=1) - 1.0).max() <= 2.0 ** -23
    # M is a rotation only up to its rounding to float32 (2^-24 per entry), and the result is rounded to float32
    assert np.abs(n1 - n0 @ M[:3, :3].T).max() <= 2.0 ** -21
    # and they are the normals of the transformed mesh: the same faces over the file's positions
    again = MN.vertex_normals(verts["p"], m["keys"], m["faces"], 24)["normals"].astype(np.float64)
    assert np.abs(np.einsum("ij,ij->i", again[has], n1[has]) - 1.0).max() < 1e-6


def test_mirror_keeps_the_normals_on_their_side_of_the_surface(vh, small_mesh, tmp_path):
    """cofactor matrix times the sign of the determinant: under a mirror a normal is mirrored, so it stays on the side of
    the surface it was on.  The faces keep their index order, and the winding rule (a x b of the transformed edges is
    cof(A) (a x b)) then gives the other side: every normal of the file is the opposite of the one recomputed from it."""
    from voxelhashing_amd import engine as E
    m = small_mesh
    mirror = np.diag([-1.0, 1.0, 1.0])
    M, verts = transformed(E, m, mirror, (0.25, 0.0, -7.0), str(tmp_path / "mirror.ply"))
    n0, n1 = m["normals"].astype(np.float64), verts["n"].astype(np.float64)
    has = np.any(n0 != 0, axis=1)
    # a sign, and the renormalisation in double of a vector whose length is 1 to 2^-23: at most an ulp of float32
    assert np.abs(n1 - n0 * np.array([-1.0, 1.0, 1.0])).max() <= 2.0 ** -23 and not n1[~has].any()
    again = MN.vertex_normals(verts["p"], m["keys"], m["faces"], 24)["normals"].astype(np.float64)
    assert np.abs(np.einsum("ij,ij->i", again[has], n1[has]) + 1.0).max() < 1e-6
    # a mirror with a rotation and a scale: unit length, and the same rule
    A = 1.7 * rotation((0.2, 0.3, -1.0), 2.1) @ mirror
    M, verts = transformed(E, m, A, (1.0, 2.0, 3.0), str(tmp_path / "mirror2.ply"))
    n2 = verts["n"].astype(np.float64)
    assert np.abs(np.linalg.norm(n2[has], axis=1) - 1.0).max() <= 2.0 ** -23 and not n2[~has].any()
    cof = np.linalg.det(M[:3, :3]) * np.linalg.inv(M[:3, :3]).T
    want = -(n0 @ cof.T)
    want[has] /= np.linalg.norm(want[has], axis=1)[:, None]
    assert np.abs(n2 - want).max() <= 2.0 ** -21


# ---------------------------------------------------------------------------- 4. what the kernels cost

def test_normal_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    from voxelhashing_amd import lib
    rows = {r["kernel"].split("(")[0]: r for r in KR.library_resources(lib.LIB_PATH)}
    for name in ("k_mesh_normals_faces", "k_mesh_normals_finish"):
        assert name in rows, sorted(k for k in rows if "mesh" in k or "weld" in k)
        r = rows[name]
        print(name, r)
        assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r["lds_bytes"] == 0
        assert r["vgprs"] <= 64  # eight waves per SIMD


# ---------------------------------------------------------------------------- 5. the replay tool

def test_replay_refuses_mesh_normals_without_an_indexed_mesh(tmp_path):
    """a usage error, before the tool looks for a GPU"""
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "replay.py"), "--params", str(tmp_path / "none.txt"), "--mesh", str(tmp_path / "m.ply"),
                        "--mesh-normals"], capture_output=True, text=True)
    assert r.returncode == 2 and "--mesh-normals needs --indexed-mesh" in r.stderr and not (tmp_path / "m.ply").exists()
