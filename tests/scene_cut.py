"""The scene cut restated in numpy on canonical forms (DESIGN.md section 4 "Scene cut").  TEST INFRASTRUCTURE ONLY.

A scene is (positions [n, 3] int32, voxels [n, 512] VOXEL_DTYPE) -- what canonical.snapshot gives as "positions" and
"voxels", and what tests/scene_merge.py takes.  cut() returns the cut scene and the lifted list in the same form, sorted
by position, the positions of the freed blocks and the counts that do not depend on the order in which the device's
deletes ran.

  * voxel l of the block at pos is the integer triple 8 pos + (l & 7, (l >> 3) & 7, l >> 6), in wrapping int32, converted
    to float32; per row r of the float32 3x4 matrix m: u_r = ((m_r0 i + m_r1 j) + m_r2 k) + m_r3, one float32 rounding
    per operation;
  * box: inside iff every |u_r| <= 1; ellipsoid: iff (u_x u_x + u_y u_y) + u_z u_z <= 1; a NaN compares false; the
    selected voxels are the inside ones, with CUT_SELECT_OUTSIDE those that are not inside;
  * a block is touched iff one of its voxels is selected; an untouched block is returned as it came in;
  * erase: the selected voxels of a touched block become zero bytes, and a touched block without an unselected voxel of
    weight > 0 leaves the scene; lift: every touched block with a selected voxel of weight > 0, its unselected voxels
    zero; keep: the scene comes back as it went in;
  * all or nothing: lifting into fewer staging blocks than there are blocks to lift changes nothing
    (CUT_STAGING_SHORT).
"""
import numpy as np

from scene_merge import sort_scene
from voxelhashing_amd import vhtypes as T

V = T.SDF_BLOCK_VOXELS
COUNT_KEYS = ("blocks_in", "touched", "freed", "lifted", "voxels_erased", "voxels_lifted", "status")


def region_matrix(world_from_region, half_extents, voxel_size):
    """vh_cut_region_transform's expressions in float64, each value rounded once to float32 -> [3, 4]"""
    T4 = np.asarray(world_from_region, np.float64).reshape(4, 4)
    R, t = T4[:3, :3], T4[:3, 3]
    h = np.asarray(half_extents, np.float32).astype(np.float64)
    vs = np.float64(np.float32(voxel_size))
    m = np.zeros((3, 4), np.float64)
    for r in range(3):
        for c in range(3):
            m[r, c] = (R[c, r] * vs) / h[r]
        m[r, 3] = -(((R[0, r] * t[0] + R[1, r] * t[1]) + R[2, r] * t[2]) / h[r])
    return m.astype(np.float32)


def voxel_coords(positions):
    """[n, 512, 3] int32: the integer triples of every voxel of the blocks"""
    l = np.arange(V)
    local = np.stack([l & 7, (l >> 3) & 7, l >> 6], axis=-1).astype(np.uint32)
    base = np.ascontiguousarray(positions, np.int32).reshape(-1, 3).view(np.uint32)
    return (base[:, None, :] * np.uint32(8) + local[None]).view(np.int32)


def region_u(m, positions):
    """[n, 512, 3] float32: u of every voxel"""
    m = np.ascontiguousarray(m, np.float32).reshape(3, 4)
    f = voxel_coords(positions).astype(np.float32)
    i, j, k = f[..., 0], f[..., 1], f[..., 2]
    with np.errstate(over="ignore", invalid="ignore"):
        u = [((m[r, 0] * i + m[r, 1] * j) + m[r, 2] * k) + m[r, 3] for r in range(3)]
    assert all(x.dtype == np.float32 for x in u)
    return np.stack(u, axis=-1)


def inside(m, shape, positions):
    u = region_u(m, positions)
    with np.errstate(over="ignore", invalid="ignore"):
        if shape == T.CUT_ELLIPSOID:
            return (u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2] <= np.float32(1)
        return (np.abs(u[..., 0]) <= np.float32(1)) & (np.abs(u[..., 1]) <= np.float32(1)) & (np.abs(u[..., 2]) <= np.float32(1))


def selected(m, shape, flags, positions):
    """[n, 512] bool"""
    ins = inside(m, shape, positions)
    return ~ins if flags & T.CUT_SELECT_OUTSIDE else ins


def cut(scene, m, shape, flags=0, staging_blocks=None):
    """scene: (positions, voxels) -> dict(positions, voxels: the scene afterwards; lifted: (positions, voxels);
    freed: positions; counts: COUNT_KEYS by name).  flags: CUT_SELECT_OUTSIDE, CUT_LIFT, CUT_KEEP, CUT_COUNT_ONLY."""
    pos, vox = sort_scene(*scene)
    lift, keep, count_only = bool(flags & T.CUT_LIFT), bool(flags & T.CUT_KEEP), bool(flags & T.CUT_COUNT_ONLY)
    assert lift or not keep
    sel = selected(m, shape, flags, pos) if len(pos) else np.zeros((0, V), bool)
    observed = vox["weight"] > 0
    touched = sel.any(axis=1)
    freeable = touched & ~(~sel & observed).any(axis=1)
    liftable = (sel & observed).any(axis=1)
    gone = int((sel & observed).sum())
    counts = dict(blocks_in=len(pos), touched=int(touched.sum()), freed=0 if keep else int(freeable.sum()), lifted=int(liftable.sum()) if lift else 0,
                  voxels_erased=0 if keep else gone, voxels_lifted=gone if lift else 0, status=0)
    nothing = (np.zeros((0, 3), np.int32), np.zeros((0, V), T.VOXEL_DTYPE))
    out = dict(positions=pos, voxels=vox, lifted=nothing, freed=nothing[0], counts=counts)
    if lift and not count_only and staging_blocks is not None and staging_blocks < counts["lifted"]:
        counts["status"] = T.CUT_STAGING_SHORT
        return out
    if count_only:
        return out
    if lift:
        lv = vox[liftable].copy()
        lv[~sel[liftable]] = np.zeros((), T.VOXEL_DTYPE)
        out["lifted"] = (pos[liftable], lv)
    if not keep:
        cv = vox.copy()
        cv[sel] = np.zeros((), T.VOXEL_DTYPE)
        # an untouched block is the block that came in
        cv[~touched] = vox[~touched]
        out.update(positions=np.ascontiguousarray(pos[~freeable]), voxels=np.ascontiguousarray(cv[~freeable]), freed=pos[freeable])
    return out


def assert_counts(got, want, what=""):
    """the device's counts against the restatement's, on the fields no schedule changes"""
    for k in COUNT_KEYS:
        assert got[k] == want[k], f"{what}: {k} is {got[k]}, the restatement says {want[k]} ({ {q: got[q] for q in COUNT_KEYS} } vs {want})"


def rotation(axis_angles):
    """a product of rotations about coordinate axes: [(axis 0/1/2, radians), ...] -> 3x3 float64"""
    R = np.eye(3)
    for axis, a in axis_angles:
        c, s = np.cos(a), np.sin(a)
        i, j = [(1, 2), (2, 0), (0, 1)][axis]
        M = np.eye(3)
        M[i, i], M[i, j], M[j, i], M[j, j] = c, -s, s, c
        R = R @ M
    return R


def frame(R=None, t=(0.0, 0.0, 0.0)):
    m = np.eye(4)
    if R is not None:
        m[:3, :3] = R
    m[:3, 3] = t
    return m
