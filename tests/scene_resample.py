"""The resampled merge restated in numpy (DESIGN.md section 4 "Resampled merge").  TEST INFRASTRUCTURE ONLY.

A scene is (positions [n, 3] int32, voxels [n, 512] VOXEL_DTYPE), as in tests/scene_merge.py.  resample() samples a
source scene at the voxel centres of another lattice by the rule of include/vh_api.h (vh_resample_blocks), in float32
with one rounding per operation, and keeps the blocks with an observed voxel; merge_transformed() hands them to
scene_merge.merge.  The rule is evaluated on every block of a generous box -- the source's box of voxels taken through
the transform, plus a block all round -- so nothing here knows the device's candidate rule.

voxel_transforms() restates vh_resample_voxel_transforms in float64, rounded once.
"""
import numpy as np

import scene_merge as SM
from voxelhashing_amd import vhtypes as T

V = T.SDF_BLOCK_VOXELS
F = np.float32
MOST_COORD = F(2.0 ** 24)


def voxel_transforms(dst_from_src, vs_src, vs_dst):
    """-> (srcVoxFromDstVox, dstVoxFromSrcVox) float32 [3, 4], or None where the C function refuses"""
    M = np.asarray(dst_from_src, np.float64).reshape(4, 4)
    s, d = float(F(vs_src)), float(F(vs_dst))
    if not (np.isfinite(M).all() and np.isfinite([s, d]).all() and s > 0 and d > 0):
        return None
    if not np.array_equal(M[3], [0, 0, 0, 1]) or s / d < 0.5 or s / d > 2.0:
        return None
    R, t = M[:3, :3], M[:3, 3]
    if np.abs(R.T @ R - np.eye(3)).max() > 1e-4 or np.linalg.det(R) <= 0:
        return None
    a, b = np.zeros((3, 4), np.float64), np.zeros((3, 4), np.float64)
    for r in range(3):
        for c in range(3):
            a[r, c] = R[c, r] * (d / s)
            b[r, c] = R[r, c] * (s / d)
        a[r, 3] = -((R[0, r] * t[0] + R[1, r] * t[1]) + R[2, r] * t[2]) / s
        b[r, 3] = t[r] / d
    return a.astype(F), b.astype(F)


def rule_positions(m, ijk):
    """q = ((m0 i + m1 j) + m2 k) + m3 per row, float32 -> [n, 3]"""
    m = np.asarray(m, F).reshape(3, 4)
    i, j, k = (ijk[:, a].astype(F) for a in range(3))
    return np.stack([((m[r, 0] * i + m[r, 1] * j) + m[r, 2] * k) + m[r, 3] for r in range(3)], axis=-1)


class Dense:
    """a scene's voxels in one array over its box of blocks: a tap outside, or in a block the scene lacks, has weight 0"""

    def __init__(self, positions, voxels):
        positions = np.asarray(positions, np.int64).reshape(-1, 3)
        self.lo = positions.min(axis=0) * 8
        shape = (positions.max(axis=0) + 1) * 8 - self.lo
        self.vox = np.zeros(tuple(int(v) for v in shape[::-1]), T.VOXEL_DTYPE)  # [z, y, x]
        for p, v in zip(positions, np.asarray(voxels).reshape(-1, 8, 8, 8)):
            o = p * 8 - self.lo
            self.vox[o[2]:o[2] + 8, o[1]:o[1] + 8, o[0]:o[0] + 8] = v

    def at(self, v):
        """voxels at global voxel coordinates v [n, 3] (int64)"""
        r = v - self.lo
        inside = ((r >= 0) & (r < np.array(self.vox.shape[::-1]))).all(axis=1)
        out = np.zeros(len(v), T.VOXEL_DTYPE)
        ri = r[inside]
        out[inside] = self.vox[ri[:, 2], ri[:, 1], ri[:, 0]]
        return out


def rule_voxels(dense, m, ijk):
    """the rule at destination voxels ijk [n, 3] -> VOXEL_DTYPE [n] (all zero where unobserved)"""
    q = rule_positions(m, ijk)
    with np.errstate(invalid="ignore"):
        valid = (np.abs(q) < MOST_COORD).all(axis=1)
    q = np.where(valid[:, None], q, F(0))
    b = np.floor(q)
    f = q - b
    g = F(1) - f
    bi = b.astype(np.int64)
    n = len(ijk)
    ok = valid.copy()
    first = np.ones(n, bool)
    acc = np.zeros((n, 4), F)  # sdf, r, g, b
    weight = np.full(n, 255, np.int64)
    for t in range(8):
        bits = np.array([t & 1, (t >> 1) & 1, (t >> 2) & 1])
        a = [np.where(bits[c] == 1, f[:, c], g[:, c]).astype(F) for c in range(3)]
        w = (a[0] * a[1]) * a[2]
        used = w != 0
        tap = dense.at(bi + bits)
        ok &= ~used | (tap["weight"] > 0)
        weight = np.where(used, np.minimum(weight, tap["weight"]), weight)
        vals = np.concatenate([tap["sdf"][:, None], tap["color"].astype(F)], axis=1).astype(F)
        with np.errstate(all="ignore"):
            prod = w[:, None] * vals
            acc = np.where((used & first)[:, None], prod, np.where(used[:, None], acc + prod, acc)).astype(F)
        first &= ~used
    ok &= ~first
    out = np.zeros(n, T.VOXEL_DTYPE)
    sdf = acc[:, 0].copy()
    with np.errstate(all="ignore"):
        colour = np.minimum(255, (acc[:, 1:] + F(0.5)).astype(np.int64)).astype(np.uint8)
    out["sdf"] = np.where(ok, sdf, F(0))
    # (np.where keeps the sign of -0 where ok; an unobserved voxel is +0)
    out["color"] = np.where(ok[:, None], colour, 0)
    out["weight"] = np.where(ok, weight, 0).astype(np.uint8)
    return out


LOCAL = np.stack([np.arange(V) % 8, (np.arange(V) // 8) % 8, np.arange(V) // 64], axis=-1).astype(np.int64)


def block_box(src_positions, dst_vox_from_src_vox):
    """every destination block in the box that the source's voxels (a tap's width added) span under the transform, plus
    a block all round"""
    p = np.asarray(src_positions, np.int64).reshape(-1, 3)
    lo, hi = p.min(axis=0) * 8 - 1, p.max(axis=0) * 8 + 9
    corners = np.array([[(hi if (c >> a) & 1 else lo)[a] for a in range(3)] for c in range(8)], np.float64)
    m = np.asarray(dst_vox_from_src_vox, np.float64).reshape(3, 4)
    img = corners @ m[:, :3].T + m[:, 3]
    blo = np.floor(img.min(axis=0) / 8).astype(np.int64) - 1
    bhi = np.floor(img.max(axis=0) / 8).astype(np.int64) + 1
    axes = [np.arange(blo[a], bhi[a] + 1) for a in range(3)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)


def resample(src, src_vox_from_dst_vox, dst_vox_from_src_vox, blocks=None):
    """src: (positions, voxels) -> dict(positions, voxels: the staged blocks sorted by position; counts =
    {source_blocks, staged, observed, status})"""
    spos, svox = SM.sort_scene(*src)
    counts = dict(source_blocks=len(spos), staged=0, observed=0, status=0)
    if len(spos) == 0:
        return dict(positions=spos, voxels=svox, counts=counts)
    dense = Dense(spos, svox)
    blocks = block_box(spos, dst_vox_from_src_vox) if blocks is None else np.asarray(blocks, np.int64).reshape(-1, 3)
    keep_pos, keep_vox = [], []
    for start in range(0, len(blocks), 256):
        part = blocks[start:start + 256]
        ijk = (part[:, None, :] * 8 + LOCAL[None]).reshape(-1, 3)
        vox = rule_voxels(dense, src_vox_from_dst_vox, ijk).reshape(len(part), V)
        seen = (vox["weight"] > 0).any(axis=1)
        keep_pos.append(part[seen])
        keep_vox.append(vox[seen])
    pos, vox = SM.sort_scene(np.concatenate(keep_pos).astype(np.int32), np.concatenate(keep_vox))
    counts["staged"], counts["observed"] = len(pos), int((vox["weight"] > 0).sum())
    return dict(positions=pos, voxels=vox, counts=counts)


def merge_transformed(dst, src, hp, src_vox_from_dst_vox, dst_vox_from_src_vox, free_blocks=None):
    """-> (scene_merge.merge's result for the staged list, resample's result)"""
    staged = resample(src, src_vox_from_dst_vox, dst_vox_from_src_vox)
    return SM.merge(dst, (staged["positions"], staged["voxels"]), hp, free_blocks=free_blocks), staged


def crafted_source(seed, side=4, corner=(-2, -2, -2), truncation=0.2):
    """side^3 blocks from `corner` on (straddling the origin by default, so that floor differs from truncation): random
    sdf and colour, weights 1 ... 30 with a quarter of the voxels unobserved and all zero, three blocks unobserved
    throughout, and -0, denormals and the float's small end among the sdfs"""
    rng = np.random.default_rng(seed)
    n = side ** 3
    k = np.arange(n)
    pos = (np.stack([k % side, (k // side) % side, k // side ** 2], axis=-1) + np.array(corner)).astype(np.int32)
    vox = np.zeros((n, V), T.VOXEL_DTYPE)
    sdf = rng.uniform(-truncation, truncation, (n, V)).astype(F)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 3e-39, 1.1754944e-38, -1.1754944e-38], F)
    pick = rng.random((n, V)) < 0.03
    sdf[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    vox["sdf"] = sdf
    vox["color"] = rng.integers(0, 256, (n, V, 3), dtype=np.uint8)
    vox["weight"] = rng.integers(1, 31, (n, V)).astype(np.uint8)
    vox[rng.random((n, V)) < 0.25] = np.zeros((), T.VOXEL_DTYPE)
    vox[rng.permutation(n)[:3]] = np.zeros((), T.VOXEL_DTYPE)
    return SM.sort_scene(pos, vox)


def random_blocks(positions, seed, truncation=0.2):
    """blocks at the given positions: seeded sdf, colour and weights 1 ... 30, two fifths of the voxels unobserved"""
    rng = np.random.default_rng(seed)
    n = len(positions)
    vox = np.zeros((n, V), T.VOXEL_DTYPE)
    vox["sdf"] = rng.uniform(-truncation, truncation, (n, V)).astype(F)
    vox["color"] = rng.integers(0, 256, (n, V, 3), dtype=np.uint8)
    vox["weight"] = rng.integers(1, 31, (n, V)).astype(np.uint8)
    vox[rng.random((n, V)) < 0.4] = np.zeros((), T.VOXEL_DTYPE)
    return SM.sort_scene(np.asarray(positions, np.int32), vox)


def ball_of_blocks(n):
    """the n block positions nearest the origin (ties by position): a solid lump"""
    k = np.arange(-6, 7)
    p = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)
    order = np.lexsort((p[:, 0], p[:, 1], p[:, 2], (p * p).sum(axis=1)))
    return p[order[:n]].astype(np.int32)


def linear_field(vs, qmax, normal, seed=0):
    """64^3 voxels, the box [qmax - 64, qmax)^3, holding float32(n . x - d) at x = v * vs metres, d such that the field
    is 0 at the box's centre; every voxel observed -> (scene, n, d)"""
    vs = float(F(vs))
    n = np.asarray(normal, np.float64)
    n = n / np.linalg.norm(n)
    assert qmax % 8 == 0
    first = qmax // 8 - 8
    k = np.arange(8)
    pos = (np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3) + first).astype(np.int32)
    d = float(n @ (np.full(3, qmax - 32.0) * vs))
    v = (pos.astype(np.int64)[:, None, :] * 8 + LOCAL[None]).astype(np.float64)
    rng = np.random.default_rng(seed)
    vox = np.zeros((len(pos), V), T.VOXEL_DTYPE)
    vox["sdf"] = ((v * vs) @ n - d).astype(F)
    vox["color"] = rng.integers(0, 256, (len(pos), V, 3), dtype=np.uint8)
    vox["weight"] = rng.integers(1, 31, (len(pos), V)).astype(np.uint8)
    return SM.sort_scene(pos, vox), n, d


def over_the_box(src_positions, dst_vox_from_src_vox, staged_positions, staged_voxels):
    """the staged blocks laid into the generous box of block_box, every other block of it unobserved"""
    box = block_box(src_positions, dst_vox_from_src_vox)
    where = {tuple(int(c) for c in p): k for k, p in enumerate(box)}
    vox = np.zeros((len(box), V), T.VOXEL_DTYPE)
    for p, v in zip(np.asarray(staged_positions), np.asarray(staged_voxels)):
        vox[where[tuple(int(c) for c in p)]] = v  # (KeyError: a staged block outside the box)
    return box, vox


def linear_field_errors(staged_positions, staged_voxels, M, vs_src, vs_dst, qmax, n, d):
    """the staged blocks of a linear field against the analytic field under dstFromSrc = M
    -> (the largest error over the observed voxels in metres, probed voxels observed, probed voxels, max |sdf|): probed
    are the staged blocks' voxels whose exact sample position has all eight taps in the source's box (a block with such a
    voxel is staged unless the device dropped it, which the comparison with the restatement rules out)"""
    vs_src, vs_dst = float(F(vs_src)), float(F(vs_dst))
    R, t = M[:3, :3], M[:3, 3]
    p = (np.asarray(staged_positions, np.int64)[:, None, :] * 8 + LOCAL[None]).reshape(-1, 3)
    x = (p * vs_dst - t) @ R  # R^T (y - t), per row
    out = np.asarray(staged_voxels).reshape(-1)
    seen = out["weight"] > 0
    err = np.abs(out["sdf"][seen].astype(np.float64) - (x[seen] @ n - d))
    # the probed voxels: over the whole box of candidate blocks, not only the staged ones
    q = x / vs_src
    inside = ((q >= qmax - 64) & (q <= qmax - 1)).all(axis=1)
    return float(err.max()), int((seen & inside).sum()), int(inside.sum()), float(np.abs(out["sdf"][seen]).max())


def rotation(axis, angle):
    """Rodrigues' formula in float64"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def rigid(R=None, t=(0, 0, 0)):
    M = np.eye(4)
    if R is not None:
        M[:3, :3] = R
    M[:3, 3] = t
    return M


def assert_half_voxel_blend(source, positions, voxels):
    """the staged blocks of `source` moved by half a voxel along x: sdf 0.5 a + 0.5 b to the bit, the colour's mean
    rounded, the lesser weight, and unobserved where either neighbour is"""
    dense = Dense(*source)
    p = (np.asarray(positions, np.int64)[:, None, :] * 8 + LOCAL[None]).reshape(-1, 3)
    left, right = dense.at(p - np.array([1, 0, 0])), dense.at(p)
    both = (left["weight"] > 0) & (right["weight"] > 0)
    out = np.asarray(voxels).reshape(-1)
    assert np.array_equal(out["weight"] > 0, both) and both.sum() > 1000
    h = F(0.5)
    assert np.array_equal((h * left["sdf"][both] + h * right["sdf"][both]).view(np.uint32), out["sdf"][both].view(np.uint32))
    assert np.array_equal(out["weight"][both], np.minimum(left["weight"], right["weight"])[both])
    mean = ((h * left["color"][both].astype(F) + h * right["color"][both].astype(F)) + h).astype(np.int64)
    assert np.array_equal(out["color"][both], mean.astype(np.uint8))
    assert not out[~both].view(np.uint64).any()
    # every block with a blended voxel is listed, and no other
    every = np.unique(np.concatenate([np.asarray(source[0], np.int64), np.asarray(source[0], np.int64) + np.array([1, 0, 0])]), axis=0)
    q = (every[:, None, :] * 8 + LOCAL[None]).reshape(-1, 3)
    seen = ((dense.at(q - np.array([1, 0, 0]))["weight"] > 0) & (dense.at(q)["weight"] > 0)).reshape(len(every), V).any(axis=1)
    want = every[seen]
    assert np.array_equal(want[np.lexsort(want.T[::-1])], np.asarray(positions, np.int64)[np.lexsort(np.asarray(positions, np.int64).T[::-1])])


SHIFT = np.array([3, -5, 10], np.int64)


def exact_cases(vs):
    """The transforms under which every sample falls on a source voxel: (name, dstFromSrc, vs_src, vs_dst, the map from a
    source voxel to its destination voxel -> (p, which voxels have one)).  The translation is whole voxels of float32(vs),
    built in float64."""
    vs = float(F(vs))
    t = SHIFT * vs
    turn = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    everyone = lambda v: np.ones(len(v), bool)  # noqa: E731
    return [
        ("identity", rigid(), vs, vs, lambda v: (v, everyone(v))),
        ("shift", rigid(None, t), vs, vs, lambda v: (v + SHIFT, everyone(v))),
        ("turn and shift", rigid(turn, t), vs, vs, lambda v: (np.stack([-v[:, 1], v[:, 0], v[:, 2]], axis=-1) + SHIFT, everyone(v))),
        ("coarser by 2", rigid(), vs, float(F(2.0 * vs)), lambda v: (v >> 1, (v & 1).sum(axis=1) == 0)),
    ]


def permuted(src, dst_voxel_of):
    """The scene whose voxel at p is the source's observed voxel at v, for (p, has) = dst_voxel_of(v) (global voxel
    coordinates, int64 [n, 3]; one-to-one on the voxels that have one), every other voxel unobserved and all zero: what
    an exact transform gives.  Blocks without an observed voxel are left out."""
    spos, svox = SM.sort_scene(*src)
    v = (spos.astype(np.int64)[:, None, :] * 8 + LOCAL[None]).reshape(-1, 3)
    flat = svox.reshape(-1)
    p, has = dst_voxel_of(v)
    seen = (flat["weight"] > 0) & has
    p = np.asarray(p, np.int64)[seen]
    blk = p >> 3
    pos, inv = np.unique(blk, axis=0, return_inverse=True)
    vox = np.zeros((len(pos), V), T.VOXEL_DTYPE)
    loc = p & 7
    vox[inv.reshape(-1), loc[:, 2] * 64 + loc[:, 1] * 8 + loc[:, 0]] = flat[seen]
    return SM.sort_scene(pos.astype(np.int32), vox)
