"""The numpy restatement of the scene registration (tests/scene_align.py) held to what it restates, and what of the
feature needs no GPU: its Jacobian row against a finite difference of its own residual, the totals' independence of
the order, the conditions of the fixture that tests/test_gpu_scene_align.py runs on the device, the refusals, and the
declarations."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scene_align as SA
import scene_resample as SR
from voxelhashing_amd import lib, vhtypes as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def fix():
    """the fixture of the issue: a ball, a floor and two walls in 64^3 voxels = 512 blocks, cut off at 4 voxels; the
    source turned by 2 degrees and moved by 1.9 voxels"""
    dst, src, truth, vs_src, vs_dst = SA.fixture()
    assert len(dst[0]) == len(src[0]) == 512
    return dst, src, truth, vs_src, vs_dst


def test_the_jacobian_row_is_the_derivative_of_the_residual():
    """On a plane the blend is exact and the gradient constant, so the residual is linear in q and a finite difference
    under a small twist y meets J y up to the float32 rounding of the positions and the blend (about 1e-5 voxel at these
    coordinates) and the twist's second order (|w|^2 |q - pivot| < 1e-6).  A wrong sign or a lever arm that is not
    (q - pivot) / radius misses by the size of J y itself, 1e-2."""
    vs = float(F(0.01))
    field = SA.plane_field((0.3, -0.5, 0.81), 0.002)
    dst = SA.field_scene(vs, np.eye(4), field=field, scale=1.0)
    pose = SR.rigid(SR.rotation((1, 2, 3), 0.05), (0.013, -0.008, 0.004))
    # the source holds the same plane a third of a voxel off, so that no residual is zero
    src = SA.field_scene(vs, pose, side=4, field=SA.plane_field((0.3, -0.5, 0.81), 0.002 + vs / 3.0), scale=1.0)
    pivot, radius = np.array([3.0, -2.0, 1.0], F), 64.0
    b0 = SR.voxel_transforms(pose, vs, vs)[1]
    r0 = SA.rule(dst, src, b0, pivot, 1.0 / radius, 2.0, vs, vs)
    assert r0["kept"].sum() > 2000
    with np.errstate(all="ignore"):
        J = r0["terms"][..., T.ALIGN_JTE:T.ALIGN_JTE + 6].astype(np.float64) / r0["e"].astype(np.float64)[..., None]
    assert (np.abs(r0["e"][r0["kept"]]) > 0.2).all()
    for a in range(6):
        y = np.zeros(6)
        y[a] = 1e-2
        moved, _, _ = SA.moved(pose, y, pivot, 1.0 / radius, vs)
        r1 = SA.rule(dst, src, SR.voxel_transforms(moved, vs, vs)[1], pivot, 1.0 / radius, 2.0, vs, vs)
        both = r0["kept"] & r1["kept"]
        assert both.sum() > 2000
        diff = r1["e"][both].astype(np.float64) - r0["e"][both].astype(np.float64)
        want = J[both][:, a] * y[a]
        assert np.abs(want).max() > 2e-3, (a, np.abs(want).max())
        err = np.abs(diff - want).max()
        print(f"twist {a}: |J y| up to {np.abs(want).max():.3e}, finite difference off by {err:.3e}")
        assert err < 1e-4, (a, err)
    # and the 21 products are those of the same row
    k = r0["kept"]
    at = 0
    for a in range(6):
        for c in range(a, 6):
            assert np.allclose(r0["terms"][k][:, at], J[k][:, a] * J[k][:, c], rtol=1e-5, atol=1e-6)
            at += 1


def test_the_totals_do_not_depend_on_the_order(fix):
    dst, src, truth, vs_src, vs_dst = fix
    b = SR.voxel_transforms(np.eye(4), vs_src, vs_dst)[1]
    pivot, radius = SA.pivot_and_radius(src[0], b)
    ruled = SA.rule(dst, src, b, pivot, 1.0 / radius, 2.0, vs_src, vs_dst)
    want = SA.totals(ruled)
    assert want[T.ALIGN_COUNT] >> T.ALIGN_QUANTUM_LOG2 == ruled["kept"].sum() > 10000
    rng = np.random.default_rng(5)
    order = rng.permutation(len(src[0]))
    assert np.array_equal(SA.totals(ruled, order), want)
    assert np.array_equal(SA.totals(ruled, order[::-1]), want)
    parts = sum(SA.totals(ruled, part) for part in np.array_split(order, 7))
    assert np.array_equal(parts, want)
    # the largest total is far from the end of 64 bits at this size, and the bound on a term holds
    assert np.abs(ruled["terms"]).max() < 256.0
    assert np.abs(want).max() < 2 ** 62


def test_the_fixture_converges_from_identity(fix):
    """the conditions of the issue, asserted of the restatement alone: within 8 iterations, and within 0.02 degree and
    0.05 voxel of the truth (reached: 4 iterations, 0.0004 degree, 0.0035 voxel)"""
    dst, src, truth, vs_src, vs_dst = fix
    assert np.allclose(SA.pose_error(np.eye(4), truth, vs_dst), (2.0, 1.9))
    out = SA.align(dst, src, np.eye(4), vs_src, vs_dst)
    deg, vox = SA.pose_error(out["pose"], truth, vs_dst)
    print(f"{out['iterations']} iterations, {deg:.5f} degree, {vox:.5f} voxel; condition {out['steps'][-1]['condition']:.1f}, "
          f"{out['steps'][-1]['count']} voxels")
    assert out["status"] == T.ALIGN_CONVERGED and out["iterations"] <= 8
    assert deg <= 0.02 and vox <= 0.05
    for s in out["steps"]:
        assert s["condition"] < 1000.0 and s["count"] > 10000


def test_a_coarser_destination_converges_too():
    dst, src, truth, vs_src, vs_dst = SA.fixture(ratio=2.0)
    out = SA.align(dst, src, np.eye(4), vs_src, vs_dst)
    deg, vox = SA.pose_error(out["pose"], truth, vs_dst)
    print(f"{out['iterations']} iterations, {deg:.5f} degree, {vox:.5f} voxel")
    assert out["status"] == T.ALIGN_CONVERGED and out["iterations"] <= 8 and deg <= 0.02 and vox <= 0.05


def test_gates_of_the_step():
    """a lone plane leaves three motions free: the condition gate; too few voxels: the count gate; neither moves the pose"""
    vs = float(F(0.01))
    plane = SA.plane_field((0.3, -0.5, 0.81), 0.002)
    dst = SA.field_scene(vs, np.eye(4), side=4, field=plane, scale=1.0)
    src = SA.field_scene(vs, SR.rigid(None, (0.004, 0.0, 0.0)), side=4, field=plane, scale=1.0)
    out = SA.align(dst, src, np.eye(4), vs, vs)
    assert out["status"] == T.ALIGN_ILL_CONDITIONED and out["iterations"] == 1 and np.array_equal(out["pose"], np.eye(4))
    assert out["steps"][0]["count"] > 1000
    far = SA.field_scene(vs, np.eye(4), side=2, field=plane, scale=1.0, corner=40)
    out = SA.align(far, src, np.eye(4), vs, vs)
    assert out["status"] == T.ALIGN_TOO_FEW and out["steps"][0]["count"] == 0 and np.array_equal(out["pose"], np.eye(4))


def test_refusals_agree_with_the_transform_function(fix):
    dst, src, truth, vs_src, vs_dst = fix
    L = lib.load()
    R = SR.rotation((1, 2, 3), 0.6)
    good = SR.rigid(R, (0.4, -0.2, 0.3))
    scaled, sheared, mirrored, nan = (good.copy() for _ in range(4))
    scaled[:3, :3] *= 1.01
    sheared[0, 1] += 0.01
    mirrored[:3, :3] = R @ np.diag([1.0, 1.0, -1.0])
    nan[1, 3] = np.nan
    a, b = np.zeros(12, F), np.zeros(12, F)
    small = (src[0][:1], src[1][:1])
    for M, s, d in [(good, 0.01, 0.01), (scaled, 0.01, 0.01), (sheared, 0.01, 0.01), (mirrored, 0.01, 0.01), (nan, 0.01, 0.01), (good, 0.025, 0.01),
                    (good, 0.01, 0.025), (good, 0.02, 0.01), (good, 0.01, 0.0), (good, np.inf, 0.01)]:
        refuses = SR.voxel_transforms(M, s, d) is None
        m = np.ascontiguousarray(M, np.float64)
        rc = L.vh_resample_voxel_transforms(m.ctypes.data, C.c_float(s), C.c_float(d), a.ctypes.data, b.ctypes.data)
        assert (rc != 0) == refuses
        assert (SA.align(small, small, M, s, d, max_iterations=1) is None) == refuses
    # the matrices the step derives are the transform function's of the moved pose: still rigid after ten steps
    pose = np.eye(4)
    for k in range(10):
        pose, _, _ = SA.moved(pose, np.array([0.3, -0.2, 0.1, 0.5, -0.4, 0.3]), (1.0, 2.0, 3.0), 1.0 / 64.0, 0.01)
    assert SR.voxel_transforms(pose, 0.01, 0.01) is not None


def test_the_fixed_point_conversion():
    t = np.array([0.0, -0.0, 1.0, -1.0, 2.0 ** -27, 3 * 2.0 ** -27, -(2.0 ** -27), 2.0 ** -28, 255.99998, 1e-45], F)
    want = np.array([0, 0, 1 << 26, -(1 << 26), 0, 2, 0, 0, int(round(255.99998474121094 * 2 ** 26)), 0], np.int64)
    assert np.array_equal(SA.to_fixed(t), want)  # (ties to even: a half goes to 0, three halves to 2)
    # the bound of DESIGN.md: the most blocks, every voxel contributing the largest term, stays inside 64 bits
    assert T.ALIGN_MOST_BLOCKS * 512 * (256 << T.ALIGN_QUANTUM_LOG2) < 2 ** 63


def test_the_new_symbols_are_declared_exported_and_mirrored():
    L = lib.load()
    api = open(os.path.join(ROOT, "include", "vh_api.h")).read()
    for name in ("vh_align_begin", "vh_align_step", "vh_align_bounds", "vh_debug_align_rule", "vh_scene_rep_align_scene"):
        assert hasattr(L, name) and re.search(r"\b" + name + r"\(", api), name
    types = open(os.path.join(ROOT, "include", "vh_types.h")).read()
    for name, value in [("CONVERGED", T.ALIGN_CONVERGED), ("TOO_FEW", T.ALIGN_TOO_FEW), ("ILL_CONDITIONED", T.ALIGN_ILL_CONDITIONED),
                        ("OUT_OF_RANGE", T.ALIGN_OUT_OF_RANGE), ("TOO_MANY", T.ALIGN_TOO_MANY), ("ITERATIONS_SPENT", T.ALIGN_ITERATIONS_SPENT),
                        ("MAX_ITERATIONS", T.ALIGN_MAX_ITERATIONS), ("QUANTUM_LOG2", T.ALIGN_QUANTUM_LOG2)]:
        m = re.search(r"#define VH_ALIGN_" + name + r" (\d+)", types)
        assert m and int(m.group(1)) == value, name
    assert re.search(r"#define VH_ALIGN_MOST_BLOCKS \(1u << 19\)", types) and T.ALIGN_MOST_BLOCKS == 1 << 19
    assert "alignScene" in open(os.path.join(ROOT, "include", "vh.hpp")).read()
    # the state's layout: 10760 bytes, the totals behind the per-step records
    assert C.sizeof(T.AlignState) == 10760 and T.AlignState.totals.offset == 2312 and T.AlignState.stripes.offset == 2568
    assert C.sizeof(T.AlignOptions) == 32
