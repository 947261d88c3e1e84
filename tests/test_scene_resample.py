"""The numpy restatement of the resampled merge (tests/scene_resample.py) against the rule's own consequences -- the
identity is the plain merge, whole-voxel motions and the factor 2 permute voxels, half a voxel blends two neighbours --
and what of the feature needs no GPU: vh_resample_voxel_transforms through the C ABI, and the declarations."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scene_merge as SM
import scene_resample as SR
from helpers import small_config
from voxelhashing_amd import lib, vhtypes as T

V = T.SDF_BLOCK_VOXELS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0.04, 0.01, 0.004, 0.05, 2.0 ** -5]


def params(cap=255):
    hp, _, _ = small_config(64, 48, "P4")
    hp.m_integrationWeightMax = cap
    return hp


def observed_blocks(scene):
    pos, vox = scene
    keep = (vox["weight"] > 0).any(axis=1)
    return pos[keep], vox[keep]


@pytest.fixture(scope="module")
def source():
    return SR.crafted_source(5, side=3, corner=(-2, -1, -2))


def transforms(L, M, vs_src, vs_dst):
    """vh_resample_voxel_transforms -> (rc, a, b)"""
    m = np.ascontiguousarray(M, np.float64).reshape(16)
    a, b = np.zeros(12, np.float32), np.zeros(12, np.float32)
    rc = L.vh_resample_voxel_transforms(m.ctypes.data, C.c_float(vs_src), C.c_float(vs_dst), a.ctypes.data, b.ctypes.data)
    return rc, a.reshape(3, 4), b.reshape(3, 4)


# ------------------------------------------------------------------------------------------------ the restatement

@pytest.mark.parametrize("vs", SIZES)
def test_exact_transforms_permute_the_voxels(source, vs):
    """identity, whole-voxel shift, quarter turn, factor 2: every observed source voxel arrives bit for bit, -0 and
    denormals included, border voxels too; nothing else is observed"""
    for name, M, vs_src, vs_dst, where in SR.exact_cases(vs):
        a, b = SR.voxel_transforms(M, vs_src, vs_dst)
        got = SR.resample(source, a, b)
        want = SR.permuted(source, where)
        assert SM.same_scene((got["positions"], got["voxels"]), want), f"{name} at voxel size {vs}"
        assert got["counts"]["observed"] == int((want[1]["weight"] > 0).sum()) > 1000


def test_identity_is_the_plain_merge_without_the_unobserved_blocks(source):
    hp = params(cap=20)
    a, b = SR.voxel_transforms(SR.rigid(), 0.04, 0.04)
    dst = SR.crafted_source(6, side=3, corner=(-1, -1, -1))
    assert len(observed_blocks(source)[0]) == len(source[0]) - 3
    for d in (SM.empty_scene(), dst):
        got, staged = SR.merge_transformed(d, source, hp, a, b)
        want = SM.merge(d, observed_blocks(source), hp)
        assert SM.same_scene((got["positions"], got["voxels"]), (want["positions"], want["voxels"]))
        assert got["counts"] == want["counts"]
        assert staged["counts"]["staged"] == len(source[0]) - 3


def test_half_a_voxel_along_x_blends_two_neighbours(source):
    vs = float(np.float32(0.04))
    a, b = SR.voxel_transforms(SR.rigid(None, (0.5 * vs, 0, 0)), vs, vs)
    assert np.array_equal(a, np.array([[1, 0, 0, -0.5], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32))
    got = SR.resample(source, a, b)
    SR.assert_half_voxel_blend(source, got["positions"], got["voxels"])


def test_the_staged_list_does_not_depend_on_the_box(source):
    """more blocks evaluated, the same blocks kept"""
    M = SR.rigid(SR.rotation((1, 2, 3), 0.6), (0.17, -0.23, 0.31))
    a, b = SR.voxel_transforms(M, 0.04, 0.04)
    got = SR.resample(source, a, b)
    box = SR.block_box(source[0], b)
    wider = np.unique(np.concatenate([box + np.array(o) for o in ((0, 0, 0), (2, 0, 0), (-2, 0, 0), (0, 2, -2))]), axis=0)
    again = SR.resample(source, a, b, wider)
    assert SM.same_scene((got["positions"], got["voxels"]), (again["positions"], again["voxels"]))
    assert 0 < got["counts"]["staged"] < len(box)
    # a blend is no better observed than its least observed tap
    assert int(got["voxels"]["weight"].max()) <= int(source[1]["weight"].max())


# ------------------------------------------------------------------------------------------------ the transform function

def test_voxel_transforms_are_exact_where_the_motion_is(vh):
    for vs in SIZES:
        for name, M, vs_src, vs_dst, where in SR.exact_cases(vs):
            rc, a, b = transforms(vh, M, vs_src, vs_dst)
            assert rc == 0, (name, vs)
            v = np.array([[6, -14, 22], [-8, 0, 2], [2, 4, -6], [1800, -1798, 750]], np.int64)  # (even: the factor 2 has them all)
            p, has = where(v)
            assert has.all()
            # integers through the forward matrix, and back, with nothing to round
            assert np.array_equal(SR.rule_positions(b, v), p.astype(np.float32)), (name, vs)
            assert np.array_equal(SR.rule_positions(a, p), v.astype(np.float32)), (name, vs)
            ra, rb = SR.voxel_transforms(M, vs_src, vs_dst)
            assert a.tobytes() == ra.tobytes() and b.tobytes() == rb.tobytes(), (name, vs)


@pytest.mark.parametrize("ratio", [1.0, 2.0, 0.5, 1.3])
def test_voxel_transforms_round_the_double_value_once(vh, ratio):
    for k, (axis, angle, t) in enumerate([((1, 2, 3), 0.6, (1.7, -2.3, 3.1)), ((-2, 1, -0.5), -2.1, (-0.4, 5.0, -1.9))]):
        M = SR.rigid(SR.rotation(axis, angle), t)
        vs_dst = 0.01
        vs_src = float(np.float32(vs_dst)) * ratio
        rc, a, b = transforms(vh, M, vs_src, vs_dst)
        assert rc == 0
        ra, rb = SR.voxel_transforms(M, vs_src, vs_dst)
        assert a.tobytes() == ra.tobytes() and b.tobytes() == rb.tobytes(), (k, ratio)
        # the two are each other's inverse to float precision
        s, d = float(np.float32(vs_src)), float(np.float32(vs_dst))
        assert np.allclose(a[:, :3].astype(np.float64) @ b[:, :3].astype(np.float64), np.eye(3), atol=1e-6)
        assert np.allclose(b[:, :3], M[:3, :3] * (s / d), atol=1e-6)


def test_voxel_transforms_refuse_what_is_not_rigid(vh):
    R = SR.rotation((1, 2, 3), 0.6)
    good = SR.rigid(R, (1.0, 2.0, 3.0))
    assert transforms(vh, good, 0.04, 0.04)[0] == 0
    scaled, sheared, mirrored, nan, row, inf = (good.copy() for _ in range(6))
    scaled[:3, :3] *= 1.01
    sheared[0, 1] += 0.01
    mirrored[:3, :3] = R @ np.diag([1.0, 1.0, -1.0])
    nan[1, 3] = np.nan
    inf[0, 0] = np.inf
    row[3, 0] = 1e-3
    for name, M in dict(scaled=scaled, sheared=sheared, mirrored=mirrored, nan=nan, inf=inf, row=row).items():
        assert transforms(vh, M, 0.04, 0.04)[0] == 4, name  # VH_ERR_BAD_ARGUMENT
        assert SR.voxel_transforms(M, 0.04, 0.04) is None, name
    for vs_src, vs_dst in ((0.025, 0.01), (0.01, 0.025), (0.0, 0.01), (0.01, -0.01), (np.nan, 0.01), (0.01, np.inf)):
        assert transforms(vh, good, vs_src, vs_dst)[0] == 4, (vs_src, vs_dst)
    assert transforms(vh, good, 0.02, 0.01)[0] == 0 and transforms(vh, good, 0.01, 0.02)[0] == 0  # the ends of [1/2, 2]
    # within the tolerance of a matrix that came through float32
    assert transforms(vh, SR.rigid(R.astype(np.float32).astype(np.float64), (1, 2, 3)), 0.04, 0.04)[0] == 0
    a, b = np.zeros(12, np.float32), np.zeros(12, np.float32)
    assert vh.vh_resample_voxel_transforms(None, C.c_float(0.04), C.c_float(0.04), a.ctypes.data, b.ctypes.data) == 4


# ------------------------------------------------------------------------------------------------ declarations

def test_the_new_symbols_are_declared_exported_and_mirrored(vh):
    header = open(os.path.join(ROOT, "include", "vh_api.h")).read()
    types = open(os.path.join(ROOT, "include", "vh_types.h")).read()
    for name in ("vh_resample_voxel_transforms", "vh_resample_work_bytes", "vh_resample_blocks", "vh_scene_rep_merge_scene_transformed"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in lib.PROTOTYPES and hasattr(vh, name), name
    enum = {k: int(v) for k, v in re.findall(r"\b(VH_RESAMPLE_[A-Z_]+) = (\d+)", types)}
    assert enum["VH_RESAMPLE_NUM_COUNTS"] == len(T.RESAMPLE_COUNTS)
    for k, name in enumerate(T.RESAMPLE_COUNTS):
        assert enum["VH_RESAMPLE_" + {"source_blocks": "SOURCE_BLOCKS"}.get(name, name.upper())] == k
    bits = {k: int(v) for k, v in re.findall(r"#define (VH_RESAMPLE_[A-Z_]+) (\d+)u", types)}
    assert bits == dict(VH_RESAMPLE_OUT_OF_RANGE=T.RESAMPLE_OUT_OF_RANGE, VH_RESAMPLE_TABLE_FULL=T.RESAMPLE_TABLE_FULL)
    assert "VH_MERGE_NUM_COUNTS = 8" in types
    # the scratch: a header, then 20 bytes per slot
    assert vh.vh_resample_work_bytes(11) - vh.vh_resample_work_bytes(10) == 20 << 10
    # null arguments and sizes out of range are refused before anything touches a device
    assert vh.vh_resample_blocks(None, None, 0, None, None, None, 10, None, None, None, 0, None, None) == 4
    assert vh.vh_scene_rep_merge_scene_transformed(None, None, None, None, None) == 4
