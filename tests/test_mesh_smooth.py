"""Taubin smoothing of the indexed mesh, without a GPU ("Mesh smoothing"): the numpy restatement
(tests/mesh_smooth.py) against a float64 Taubin under a derived bound, what smoothing does to a noisy sphere and an open
patch, its independence of face order, rotation and vertex numbers, hand-made cases, each status, the constants,
prototypes and the struct's layout, the refusals through the library, the option's defaults, what the kernels cost, and
the replay tool's usage errors."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import mesh_smooth as MS
import mesh_weld as MW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARGUMENT = 4  # VH_ERR_BAD_ARGUMENT
SCALE = 21


@pytest.fixture(scope="module")
def meshes():
    """the welded random soups of the issue, the closed noisy sphere and the open patch with its rim"""
    patch, rim = MS.open_patch()
    return {257: MW.weld(*MW.random_soup(257, 11)), 2000: MW.weld(*MW.random_soup(2000, 12, spread=6)), "sphere": MS.uv_sphere(), "patch": patch, "rim": rim}


# ---------------------------------------------------------------------------- 1. against a float64 Taubin

@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("name", [257, 2000, "sphere"])
def test_restatement_against_a_float64_taubin(meshes, name, n):
    """|r - r64| <= e_2N / S + 2^-24 |r| per component, e from mesh_smooth.error_bound_quanta: the worst-case
    amplification of a half step, half a quantum for u and half for the shift, then the rounding to float32.  The bound
    grows like 3^k: this is not a test for large N."""
    mesh = meshes[name]
    # nearly every edge of a random soup has one face: its vertices move only with the boundary free
    keep = name == "sphere"
    out = MS.smooth(mesh, n, keep_boundary=keep, scale_log2=SCALE)
    assert out["status"] == 0 and out["counts"]["moved"] > len(mesh["keys"]) // 2
    order = np.argsort(mesh["keys"], kind="stable")
    r = out["mesh"]["vertices"].astype(np.float64)
    r64 = MS.float64_taubin(mesh, n, 0.5, MS.DEFAULT_MU_Q16 / 65536.0, keep_boundary=keep)[order]
    e = MS.error_bound_quanta(n, MS.DEFAULT_LAMBDA_Q16, MS.DEFAULT_MU_Q16)
    assert abs(e - (5.12 if n == 1 else 24.1544)) < 1e-3
    bound = e * 2.0 ** -SCALE + 2.0 ** -24 * np.abs(r)
    err = np.abs(r - r64)
    print(name, "N", n, "largest error in quanta", float(err.max() * 2.0 ** SCALE), "bound in quanta", e)
    assert np.all(err <= bound)
    still = ~out["moved"][order]
    assert r[still].tobytes() == mesh["vertices"][order][still].astype(np.float64).tobytes()


# ---------------------------------------------------------------------------- 2. what smoothing does

def radial(mesh):
    r = np.linalg.norm(mesh["vertices"].astype(np.float64), axis=1)
    return float(r.std()), float(r.mean())


def test_taubin_smooths_the_sphere_and_shrinks_it_less_than_a_laplacian(meshes):
    """comparisons only: the radial standard deviation falls, and the mean radius moves less under lambda | mu than
    under lambda | lambda"""
    sphere = meshes["sphere"]
    std0, mean0 = radial(sphere)
    taubin = MS.smooth(sphere, 10, scale_log2=SCALE)
    laplace = MS.smooth(sphere, 10, MS.DEFAULT_LAMBDA_Q16, MS.DEFAULT_LAMBDA_Q16, scale_log2=SCALE)
    assert taubin["counts"] == dict(moved=len(sphere["keys"]), boundary_vertices=0, isolated_vertices=0, status=0, edges=3 * len(sphere["faces"]) // 2, boundary_edges=0)
    std1, mean1 = radial(taubin["mesh"])
    std2, mean2 = radial(laplace["mesh"])
    print("radial std", std0, "->", std1, "(Laplacian", std2, ") mean radius", mean0, "->", mean1, "(Laplacian", mean2, ")")
    assert std1 < std0 and abs(mean1 - mean0) < abs(mean2 - mean0)


def test_the_rim_of_an_open_patch_keeps_its_bits(meshes):
    patch, rim = meshes["patch"], meshes["rim"]
    kept = MS.smooth(patch, 10, scale_log2=SCALE)
    assert kept["counts"]["moved"] == 100 and kept["counts"]["boundary_vertices"] == 44 == int(rim.sum()) and kept["counts"]["boundary_edges"] == 44
    assert np.array_equal(kept["moved"], ~rim)
    same = np.all(kept["mesh"]["vertices"].view(np.uint32) == patch["vertices"].view(np.uint32), axis=1)  # (the keys ascend: canonical order is the input's)
    assert np.array_equal(same, rim)
    free = MS.smooth(patch, 10, keep_boundary=False, scale_log2=SCALE)
    assert free["counts"]["moved"] == 144 and free["counts"]["boundary_vertices"] == 44
    for axis in (0, 1):
        assert np.ptp(free["mesh"]["vertices"][:, axis]) < np.ptp(patch["vertices"][:, axis])
        assert np.ptp(kept["mesh"]["vertices"][:, axis]) == np.ptp(patch["vertices"][:, axis])


def test_restatement_does_not_depend_on_face_order_rotation_or_vertex_numbers(meshes):
    for name, n in ((2000, 3), ("sphere", 2), ("patch", 2)):
        want = MS.smooth(meshes[name], n, scale_log2=SCALE)
        for seed in (3, 4):
            other = MS.smooth(MS.renumbered(meshes[name], seed), n, scale_log2=SCALE)
            assert other["counts"] == want["counts"] and MW.same_mesh(other["mesh"], want["mesh"])


# ---------------------------------------------------------------------------- 3. hand-made cases

def hand_made():
    """name -> (mesh, keyword arguments of MS.smooth, expected counts without the status, expected positions or None);
    scale 0 unless said: positions are integers and a quantum is 1"""
    P = MS.plain_mesh
    tri = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]
    quad = tri + [(4, 4, 4)]
    one = dict(lambda_q16=65536, mu_q16=0, scale_log2=0)  # lambda = 1: the first half step goes to the rounded mean, the second does nothing
    out = {}
    out["one_triangle"] = (P(tri, [(0, 1, 2)]), one, dict(moved=0, boundary_vertices=3, isolated_vertices=0, edges=3, boundary_edges=3), tri)
    # a tetrahedron is closed: every vertex goes to the mean of the other three, rounded, halves up: 8/3 -> 3, 4/3 -> 1
    tet = [(0, 1, 2), (0, 3, 1), (1, 3, 2), (0, 2, 3)]
    out["tetrahedron"] = (P(quad, tet), one, dict(moved=4, boundary_vertices=0, isolated_vertices=0, edges=6, boundary_edges=0),
                          [(3, 3, 1), (1, 3, 1), (3, 1, 1), (1, 1, 0)])
    # two faces over the edge {0, 1}: it has two faces, the other four one each -- all four vertices are boundary
    two = dict(moved=0, boundary_vertices=4, isolated_vertices=0, edges=5, boundary_edges=4)
    out["two_faces_opposite_windings"] = (P(quad, [(0, 1, 2), (1, 0, 3)]), one, two, quad)
    out["two_faces_same_winding"] = (P(quad, [(0, 1, 2), (0, 1, 3)]), one, two, quad)
    free = dict(one, keep_boundary=False)  # 0 and 1 have three neighbours, 2 and 3 two
    out["two_faces_free_boundary"] = (P(quad, [(0, 1, 2), (1, 0, 3)]), free, dict(two, moved=4), [(3, 3, 1), (1, 3, 1), (2, 0, 0), (2, 0, 0)])
    # a duplicate face: every edge has two faces, so nothing is boundary by the rule
    out["duplicate_face"] = (P(tri, [(0, 1, 2), (2, 0, 1)]), one, dict(moved=3, boundary_vertices=0, isolated_vertices=0, edges=3, boundary_edges=0),
                             [(2, 2, 0), (0, 2, 0), (2, 0, 0)])
    # a face with a repeated index names no edge, and vertex 3 is named by no face at all
    out["repeated_index"] = (P(quad, [(0, 0, 1), (2, 1, 2)]), one, dict(moved=0, boundary_vertices=0, isolated_vertices=4, edges=0, boundary_edges=0), quad)
    out["unnamed_vertex"] = (P(quad, [(0, 1, 2), (0, 1, 2)]), one, dict(moved=3, boundary_vertices=0, isolated_vertices=1, edges=3, boundary_edges=0),
                             [(2, 2, 0), (0, 2, 0), (2, 0, 0), (4, 4, 4)])
    # halves round up on signed values: d = -3 and 3 over n = 2 give u = -1 and 2 (truncation: -1 and 1, floor: -2 and 1)
    dup = [(0, 1, 2), (0, 1, 2)]
    out["halves_up_negative_d"] = (P([(0, 0, 0), (-1, 0, 0), (-2, 0, 0)], dup), one, None, [(-1, 0, 0), (-1, 0, 0), (0, 0, 0)])  # -3/2, -2/2 - (-1) = 0, -1/2 - (-2) = 3/2
    out["halves_up_positive_d"] = (P([(0, 0, 0), (1, 0, 0), (2, 0, 0)], dup), one, None, [(2, 0, 0), (1, 0, 0), (1, 0, 0)])  # 3/2 -> 2; 0; 2 + floor(-3/2 + 1/2) = 1
    # a negative f u under the arithmetic shift, in the second half step (the first, with lambda = 0, changes nothing):
    # vertex 0 has d = 6, n = 2, u = 3; f = -1/2: (-98304 + 32768) >> 16 = -1; vertex 1 has d = 3, u = 2: (-65536 + 32768) >> 16 = -1
    # (-1/2 goes down, as a floor does); vertex 2 has d = -9, u = floor(-16 / 4) = -4: (131072 + 32768) >> 16 = 2
    out["negative_f_u"] = (P([(0, 0, 0), (1, 0, 0), (5, 0, 0)], dup), dict(lambda_q16=0, mu_q16=-32768, scale_log2=0), None, [(-1, 0, 0), (0, 0, 0), (7, 0, 0)])
    # f = -32769, u = 1 (vertex 1: d = 2, n = 2): (-32769 + 32768) >> 16 = -1, which a logical shift or a division would not give
    out["arithmetic_shift"] = (P([(0, 0, 0), (3, 0, 0), (8, 0, 0)], dup), dict(lambda_q16=0, mu_q16=-32769, scale_log2=0), None, None)
    return out


@pytest.mark.parametrize("name", sorted(hand_made()))
def test_hand_made_cases(name):
    mesh, kw, counts, positions = hand_made()[name]
    out = MS.smooth(mesh, 1, **kw)
    assert out["status"] == 0
    if counts is not None:
        assert out["counts"] == dict(counts, status=0), name
    if positions is not None:
        assert out["mesh"]["vertices"].tolist() == [list(map(float, p)) for p in positions], name
    if name == "arithmetic_shift":  # u = 6, 1, -6 (d = 11, 2, -13 over n = 2): (f u + 2^15) >> 16 = -3, -1, 3
        assert out["mesh"]["vertices"][:, 0].tolist() == [-3.0, 2.0, 11.0]
    assert out["mesh"]["colors"].tobytes() == mesh["colors"].tobytes() and np.array_equal(out["mesh"]["keys"], mesh["keys"])


def test_statuses_of_the_restatement():
    tet = MS.plain_mesh([(0, 0, 0), (4, 0, 0), (0, 4, 0), (4, 4, 4)], [(0, 1, 2), (0, 3, 1), (1, 3, 2), (0, 2, 3)])
    assert MS.smooth(tet, 1)["status"] == 0
    bad = MS.smooth(dict(tet, faces=np.array([[0, 1, 2], [0, 4, 1]], np.uint32)), 1)
    assert bad["status"] == MS.BAD_INDEX and set(bad["counts"].values()) == {0, MS.BAD_INDEX} and len(bad["mesh"]["keys"]) == 0
    assert MS.smooth(tet, 1, scale_log2=37)["status"] == 0 and MS.smooth(tet, 1, scale_log2=39)["status"] == MS.RANGE  # 4 * 2^39 > 2^40
    for v in (np.nan, np.inf, -np.inf):
        p = tet["vertices"].copy()
        p[2, 1] = v
        assert MS.smooth(dict(tet, vertices=p), 1)["status"] == MS.RANGE
    # within range going in, out of it after a half step: lambda = -1 doubles the distance to the neighbours' mean
    far = MS.plain_mesh([(-1, 0, 0), (1, 0, 0), (0, 1, 0), (0, -1, 0)], tet["faces"])
    assert MS.smooth(far, 1, -65536, -65536, scale_log2=40)["status"] == MS.RANGE and MS.smooth(far, 1, -65536, -65536, scale_log2=37)["status"] == 0  # (7/3)^2 * 2^37 < 2^40
    assert MS.smooth(tet, 1, edge_slots_log2=2)["status"] == MS.TABLE_FULL and MS.smooth(tet, 1, edge_slots_log2=3)["status"] == 0  # six edges
    assert MS.smooth(MS.closed_fan(MS.MAX_DEGREE), 1)["status"] == 0 and MS.smooth(MS.closed_fan(MS.MAX_DEGREE + 1), 1)["status"] == MS.DEGREE
    none = MS.smooth(dict(tet, faces=np.zeros((0, 3), np.uint32)), 1)
    assert none["counts"] == dict(moved=0, boundary_vertices=0, isolated_vertices=4, status=0, edges=0, boundary_edges=0)
    assert none["mesh"]["vertices"].tobytes() == tet["vertices"].tobytes()


# ---------------------------------------------------------------------------- 4. constants, prototypes, refusals, defaults

def test_constants_are_the_headers():
    from voxelhashing_amd import lib, vhtypes as T
    head = open(os.path.join(ROOT, "include", "vh_types.h")).read()
    for name, mine, theirs in (("TABLE_FULL", MS.TABLE_FULL, T.SMOOTH_TABLE_FULL), ("RANGE", MS.RANGE, T.SMOOTH_RANGE), ("BAD_INDEX", MS.BAD_INDEX, T.SMOOTH_BAD_INDEX),
                               ("DEGREE", MS.DEGREE, T.SMOOTH_DEGREE), ("MAX_DEGREE", MS.MAX_DEGREE, T.SMOOTH_MAX_DEGREE),
                               ("MAX_ITERATIONS", MS.MAX_ITERATIONS, T.SMOOTH_MAX_ITERATIONS)):
        assert int(re.search(r"#define VH_SMOOTH_%s (\d+)u" % name, head).group(1)) == mine == theirs
    assert int(re.search(r"#define VH_SMOOTH_DEFAULT_LAMBDA_Q16 (\d+)", head).group(1)) == MS.DEFAULT_LAMBDA_Q16 == T.SMOOTH_DEFAULT_LAMBDA_Q16 == MS.q16(0.5) == 32768
    assert int(re.search(r"#define VH_SMOOTH_DEFAULT_MU_Q16 \((-\d+)\)", head).group(1)) == MS.DEFAULT_MU_Q16 == T.SMOOTH_DEFAULT_MU_Q16 == MS.q16(-0.53) == -34734
    assert int(re.search(r"#define VH_SMOOTH_MAX_FACTOR_Q16 (\d+)", head).group(1)) == MS.MAX_FACTOR_Q16 == T.SMOOTH_MAX_FACTOR_Q16
    assert T.smooth_factor_q16(0.5) == 32768 and T.smooth_factor_q16(-0.53) == -34734 and T.smooth_factor_q16(-1) == -65536
    with pytest.raises(ValueError):
        T.smooth_factor_q16(1.0001)
    enum = re.findall(r"VH_SMOOTH_(\w+) = (\d+)", head)
    assert [int(v) for _, v in enum] == list(range(7)) and [n for n, _ in enum] == ["MOVED", "BOUNDARY", "ISOLATED", "STATUS", "EDGES", "BOUNDARY_EDGES", "NUM_COUNTS"]
    assert T.SMOOTH_COUNTS == MS.COUNTS and len(T.SMOOTH_COUNTS) == 6 and T.SMOOTH_COUNTS.index("status") == 3
    for name in ("vh_mesh_smooth", "vh_mesh_smooth_default_slots_log2", "vh_mesh_weld_accum_smooth", "vh_mesh_weld_accum_smooth_get_counts",
                 "vh_mesh_weld_accum_smooth_download", "vh_marching_cubes_set_indexed_smoothing", "vh_marching_cubes_get_indexed_smooth_stats"):
        assert name in lib.PROTOTYPES and lib.PROTOTYPES[name][0] is C.c_int


def test_struct_layout_is_the_compiled_headers():
    """the ctypes mirror of the launcher's buffers against the C compiler's layout"""
    from voxelhashing_amd import vhtypes as T
    head = open(os.path.join(ROOT, "include", "vh_types.h")).read()
    fields = re.search(r"typedef struct VhMeshSmoothData \{(.*?)\} VhMeshSmoothData;", head, re.S).group(1)
    names = re.findall(r"\b([dm]_\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [f[0] for f in T.MeshSmoothData._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "vh_types.h"\nint main(void) { printf("%zu", sizeof(VhMeshSmoothData));\n' + \
           "".join('printf(" %%zu", offsetof(VhMeshSmoothData, %s));\n' % n for n in names) + "return 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    assert got == [C.sizeof(T.MeshSmoothData)] + [getattr(T.MeshSmoothData, n).offset for n in names] and got[0] == 9 * 8 + 8


def test_default_slots(vh):
    out = C.c_uint32(99)
    for faces, want in ((0, 6), (1, 6), (10, 6), (11, 7), (21, 7), (22, 8), (257, 11), (2000, 14), (0x15555555, 31)):
        assert vh.vh_mesh_smooth_default_slots_log2(faces, C.byref(out)) == 0 and out.value == want and (1 << want) >= max(6 * faces, 64), faces
        assert want == 6 or (1 << (want - 1)) < 6 * faces
    out.value = 99
    assert vh.vh_mesh_smooth_default_slots_log2(0x15555556, C.byref(out)) == BAD_ARGUMENT and vh.vh_mesh_smooth_default_slots_log2(4, None) == BAD_ARGUMENT
    assert out.value == 99


def test_launchers_refuse_before_they_touch_the_device(vh):
    from voxelhashing_amd import vhtypes as T
    word = (C.c_uint32 * 8)(7)
    st = C.addressof(word)
    full = T.MeshSmoothData(*([st] * 9), 6, 0)
    f = vh.vh_mesh_smooth
    lam, mu = MS.DEFAULT_LAMBDA_Q16, MS.DEFAULT_MU_Q16
    assert f(None, None, None, 0, 0, 0, 0, 0, 0, 0, None, None) == BAD_ARGUMENT
    assert f(st, st, st, 3, 1, 1, lam, mu, 1, 21, None, None) == BAD_ARGUMENT                       # no buffers
    assert f(st, st, st, 3, 1, 0, lam, mu, 1, 21, C.byref(full), None) == BAD_ARGUMENT              # N = 0
    assert f(st, st, st, 3, 1, 101, lam, mu, 1, 21, C.byref(full), None) == BAD_ARGUMENT            # N = 101
    for bad in (65537, -65537):
        assert f(st, st, st, 3, 1, 1, bad, mu, 1, 21, C.byref(full), None) == BAD_ARGUMENT and f(st, st, st, 3, 1, 1, lam, bad, 1, 21, C.byref(full), None) == BAD_ARGUMENT
    assert f(st, st, st, 3, 1, 1, lam, mu, 2, 21, C.byref(full), None) == BAD_ARGUMENT              # keepBoundary is 0 or 1
    assert f(st, st, st, 3, 1, 1, lam, mu, 1, 101, C.byref(full), None) == BAD_ARGUMENT and f(st, st, st, 3, 1, 1, lam, mu, 1, -101, C.byref(full), None) == BAD_ARGUMENT
    assert f(None, st, st, 3, 1, 1, lam, mu, 1, 21, C.byref(full), None) == BAD_ARGUMENT            # vertices without an array
    assert f(st, st, None, 3, 1, 1, lam, mu, 1, 21, C.byref(full), None) == BAD_ARGUMENT            # faces without an array
    assert f(st, st, st, (1 << 30) + 1, 1, 1, lam, mu, 1, 21, C.byref(full), None) == BAD_ARGUMENT
    assert f(st, st, st, 3, 0x15555556, 1, lam, mu, 1, 21, C.byref(full), None) == BAD_ARGUMENT
    assert f(st, st, st, 3, 1, 1, lam, mu, 1, 21, C.byref(T.MeshSmoothData(*([st] * 9), 32, 0)), None) == BAD_ARGUMENT
    holes = [st] * 9
    holes[0] = None
    assert f(st, st, st, 3, 1, 1, lam, mu, 1, 21, C.byref(T.MeshSmoothData(*holes, 6, 0)), None) == BAD_ARGUMENT  # no edge table
    assert word[0] == 7
    assert vh.vh_mesh_weld_accum_smooth(None, 1, lam, mu, 1, 21, None) == BAD_ARGUMENT
    assert vh.vh_mesh_weld_accum_smooth_get_counts(None, word, None) == BAD_ARGUMENT
    assert vh.vh_mesh_weld_accum_smooth_download(None, None, 0, None) == BAD_ARGUMENT
    assert vh.vh_marching_cubes_set_indexed_smoothing(None, 1, lam, mu, 1) == BAD_ARGUMENT
    assert vh.vh_marching_cubes_get_indexed_smooth_stats(None, word) == BAD_ARGUMENT


def test_the_option_is_off_by_default():
    """nothing of a mesh's file or dictionary changes unless the option is asked for"""
    from voxelhashing_amd import engine as E, reconstruction as R
    for fn in (R.Reconstruction.extractIsoSurface, R.Reconstruction.extractIsoSurfaceIndexed):
        p = inspect.signature(fn).parameters
        assert p["smooth_iterations"].default == 0 and p["smooth_lambda"].default == 0.5 and p["smooth_mu"].default == -0.53 and p["keep_boundary"].default is True
    p = inspect.signature(E.mesh_weld_appends).parameters
    assert p["smooth_iterations"].default == 0 and p["keep_boundary"].default is True
    p = inspect.signature(E.CUDAMarchingCubesHashSDF.setIndexedSmoothing).parameters
    assert p["iterations"].default == 0 and p["lam"].default == 0.5 and p["mu"].default == -0.53 and p["keepBoundary"].default is True
    p = inspect.signature(E.mesh_smooth).parameters
    assert p["lam"].default == 0.5 and p["mu"].default == -0.53 and p["keep_boundary"].default is True and p["edge_slots_log2"].default is None
    head = open(os.path.join(ROOT, "include", "vh.hpp")).read()
    assert "void setIndexedSmoothing(unsigned int iterations, float lambda = 0.5f, float mu = -0.53f, bool keepBoundary = true);" in head
    assert "unsigned int m_smoothIterations = 0;" in head


# ---------------------------------------------------------------------------- 5. what the kernels cost

def test_smooth_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    from voxelhashing_amd import lib
    rows = {r["kernel"].split("(")[0]: r for r in KR.library_resources(lib.LIB_PATH)}
    for name in ("k_smooth_edges", "k_smooth_degree", "k_smooth_prepare", "k_smooth_gather", "k_smooth_step", "k_smooth_finish"):
        assert name in rows, sorted(k for k in rows if "mesh" in k or "weld" in k or "smooth" in k)
        r = rows[name]
        print(name, r)
        assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r["lds_bytes"] == 0
        assert r["vgprs"] <= 64  # eight waves per SIMD


# ---------------------------------------------------------------------------- 6. the replay tool

@pytest.mark.parametrize("flag, message", [(["--mesh-smooth", "5"], "--mesh-smooth needs --indexed-mesh"),
                                           (["--indexed-mesh", "--mesh-smooth", "0"], "--mesh-smooth: 1 ... 100"),
                                           (["--indexed-mesh", "--mesh-smooth", "101"], "--mesh-smooth: 1 ... 100"),
                                           (["--indexed-mesh", "--mesh-smooth", "-3"], "--mesh-smooth: 1 ... 100"),
                                           (["--indexed-mesh", "--mesh-smooth", "5", "--mesh-smooth-mu", "-1.5"], "factors in [-1, 1]")])
def test_replay_refuses_bad_smoothing_options(tmp_path, flag, message):
    """a usage error, before the tool looks for a GPU"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "replay.py"), "--params", str(tmp_path / "none.txt"), "--mesh", str(tmp_path / "m.ply")] + flag,
                       capture_output=True, text=True)
    assert r.returncode == 2 and message in r.stderr and not (tmp_path / "m.ply").exists()
