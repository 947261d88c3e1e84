"""The scene merge restated in numpy on canonical forms (DESIGN.md section 4 "Scene merge").  TEST INFRASTRUCTURE ONLY.

A scene is (positions [n, 3] int32, voxels [n, 512] VOXEL_DTYPE) -- what canonical.snapshot gives as "positions" and
"voxels".  merge() fuses a source into a destination and returns the merged scene in the same form, sorted by position,
with the counts that do not depend on the order in which the device's atomics ran.

  * the block set is the union of the destination's positions and the source's, shifted by a whole-block offset; a
    source block allocates its block whatever its voxels hold;
  * per voxel: a source voxel of weight 0 changes nothing; onto a destination voxel of weight 0 the source voxel is
    copied, its weight capped at m_integrationWeightMax; two observed voxels are combineVoxel's, which is the ORACLE's
    vho_combine_voxel (pinned to the reference's own function by tests/test_reference_pinning.py), with the colour of
    tests/weighted_colour.py's rule when the destination has m_colorIntegration = 1;
  * all or nothing on the heap: more new positions than free blocks, and the destination comes back as it went in with
    the status MERGE_HEAP_SHORT.
"""
import ctypes as C

import numpy as np

import weighted_colour as WC
from oracle import oracle as O
from voxelhashing_amd import canonical, vhtypes as T

V = T.SDF_BLOCK_VOXELS


def empty_scene():
    return np.zeros((0, 3), np.int32), np.zeros((0, V), T.VOXEL_DTYPE)


def sort_scene(positions, voxels):
    positions = np.ascontiguousarray(positions, np.int32).reshape(-1, 3)
    order = canonical.lexsort_pos(positions)
    return np.ascontiguousarray(positions[order]), np.ascontiguousarray(np.asarray(voxels, T.VOXEL_DTYPE).reshape(-1, V)[order])


def scene_of(snap):
    """(positions, voxels) of a canonical snapshot"""
    return snap["positions"], snap["voxels"]


def combine_voxels(hp, d, s):
    """combineVoxel of two flat VOXEL_DTYPE arrays (every weight > 0) through the oracle, one voxel at a time; the
    colour by the weighted rule when hp says so"""
    L = O.lib()
    out = np.zeros(len(d), T.VOXEL_DTYPE)
    v0, v1 = T.Voxel(), T.Voxel()
    hpp = C.byref(hp)
    for k in range(len(d)):
        C.memmove(C.byref(v0), d[k:k + 1].ctypes.data, 8)
        C.memmove(C.byref(v1), s[k:k + 1].ctypes.data, 8)
        r = L.vho_combine_voxel(hpp, v0, v1)
        C.memmove(out[k:k + 1].ctypes.data, C.byref(r), 8)
    if hp.m_colorIntegration != 0:
        out["color"] = WC.rule_weighted(d["color"], d["weight"][:, None], s["color"], s["weight"][:, None])
    return out


def merge_voxels(hp, d, s):
    """the per-voxel rule on two arrays of one shape -> (result, voxels combined, voxels copied)"""
    d, s = np.ascontiguousarray(d, T.VOXEL_DTYPE), np.ascontiguousarray(s, T.VOXEL_DTYPE)
    out = d.copy()
    both = (d["weight"] > 0) & (s["weight"] > 0)
    copy = (d["weight"] == 0) & (s["weight"] > 0)
    out[copy] = s[copy]
    w = out["weight"]
    w[copy] = np.minimum(s["weight"][copy].astype(np.int64), int(hp.m_integrationWeightMax)).astype(np.uint8)
    out["weight"] = w
    if both.any():
        out[both] = combine_voxels(hp, d[both], s[both])
    return out, int(both.sum()), int(copy.sum())


def merge(dst, src, hp, offset=(0, 0, 0), free_blocks=None):
    """dst, src: (positions, voxels); hp: the DESTINATION's parameters (weight cap, colour mode); free_blocks: the
    destination's free heap blocks (None: enough)
    -> dict(positions, voxels, counts = {source_blocks, present, allocated, combined, copied, status})"""
    dpos, dvox = sort_scene(*dst)
    spos, svox = sort_scene(*src)
    spos = (spos.astype(np.int64) + np.asarray(offset, np.int64)).astype(np.int32)
    assert len(np.unique(spos, axis=0)) == len(spos), "the source positions are not distinct"
    where = {tuple(int(v) for v in p): k for k, p in enumerate(dpos)}
    at = np.array([where.get(tuple(int(v) for v in p), -1) for p in spos], np.int64)
    present = at >= 0
    counts = dict(source_blocks=len(spos), present=int(present.sum()), allocated=0, combined=0, copied=0, status=0)
    missing = int((~present).sum())
    if free_blocks is not None and missing > free_blocks:
        counts["status"] = T.MERGE_HEAP_SHORT
        return dict(positions=dpos, voxels=dvox, counts=counts)
    counts["allocated"] = missing
    pos = np.concatenate([dpos, spos[~present]])
    vox = np.concatenate([dvox, np.zeros((missing, V), T.VOXEL_DTYPE)])
    at[~present] = len(dpos) + np.arange(missing)
    if len(spos):
        vox[at], counts["combined"], counts["copied"] = merge_voxels(hp, vox[at], svox)
    pos, vox = sort_scene(pos, vox)
    return dict(positions=pos, voxels=vox, counts=counts)


def same_scene(a, b):
    """two (positions, voxels) scenes hold the same blocks with the same bytes"""
    (pa, va), (pb, vb) = sort_scene(*a), sort_scene(*b)
    return np.array_equal(pa, pb) and va.tobytes() == vb.tobytes()


def assert_counts(got, want, what=""):
    """the device's counts against the restatement's, on the fields no schedule changes"""
    for k in ("source_blocks", "present", "allocated", "combined", "copied", "status"):
        assert got[k] == want[k], f"{what}: {k} is {got[k]}, the restatement says {want[k]} ({got} vs {want})"
