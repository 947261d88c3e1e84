"""A chunk grid smaller than the scene: the numpy float32 restatement of block -> world -> chunk -> (inside the grid?,
bit index) that alloc's streamed-out test, the device's stream-out pass and the host's integrateInChunkGrid all compute
(DSC/CUDASceneRepHashSDF.cu:124-156, DSC/CUDASceneRepChunkGrid.h:560-598), the index the reference's unguarded formula
would form for a chunk outside the grid, and the scene and grids of tests/test_streaming_grid_edges.py and
tests/test_gpu_streaming_grid_edges.py.

The scene is S1 seen from three poses of the 40-frame orbit.  The grid has chunks of two blocks (0.64 m at P4's 0.32 m
blocks), so every odd block coordinate sits on a rounding tie of worldToChunks, and it is smaller than the scene past
four of its faces: blocks of the scene lie in chunks that do not exist."""
import numpy as np

from helpers import small_config
from voxelhashing_amd import synth, vhtypes as T

f32 = np.float32

WIDTH, HEIGHT, PARAMS = 64, 48, "P4"
EXT = (0.64, 0.64, 0.64)
DIMS = (4, 3, 5)
MINP = (-1, -1, -3)
N_BITS = DIMS[0] * DIMS[1] * DIMS[2]  # 60: two words, the second one partial
ALLOC_POSES = (0, 5, 10)  # of the 40-frame orbit
ORBIT = 40

# The copy the online tests use: S1 and its poses moved away from the origin (the reference's hash sends (x, y, z) and
# (-x, -y, z) to one bucket; which of the two an online alloc pass serves first is a matter of scheduling).  The grid
# moves with it by whole chunks -- SHIFT / 0.64 = (11.4, 7.97, 5.78), the grid by (12, 8, 5) -- chosen so that
# check_conditions() holds for the moved scene too: blocks past x-low, y-low, y-high and z-high.
SHIFT = np.array([7.3, 5.1, 3.7])
SHIFTED_MINP = (11, 7, 2)
SHIFTED_S1 = synth.S1_SPHERES.copy()
SHIFTED_S1[:, :3] += SHIFT

# words of all ones on either side of a crafted mask: what an unguarded index reads instead of another buffer
GUARD_WORDS = 4


def orbit_pose(k, shifted=False):
    q = np.array(synth.orbit_pose(k, ORBIT), dtype=np.float32).copy()
    if shifted:
        q[3] += f32(SHIFT[0]); q[7] += f32(SHIFT[1]); q[11] += f32(SHIFT[2])
    return q


def block_to_world(blocks, voxel_size):
    """SDFBlockToWorld: (float)(block * 8) * voxelSize, in float32"""
    b = np.asarray(blocks, dtype=np.int64).reshape(-1, 3)
    return ((b * T.SDF_BLOCK_SIZE).astype(np.float32) * f32(voxel_size)).astype(np.float32)


def world_to_chunks(world, ext=EXT):
    """worldToChunks: p = world / extents; int(p + sign(p) * 0.5), the conversion truncating towards zero"""
    p = (np.asarray(world, dtype=np.float32).reshape(-1, 3) / np.asarray(ext, dtype=np.float32)).astype(np.float32)
    return np.trunc((p + np.sign(p).astype(np.float32) * f32(0.5)).astype(np.float32)).astype(np.int64)


def chunk_inside(chunks, dims=DIMS, minp=MINP):
    q = np.asarray(chunks, dtype=np.int64).reshape(-1, 3) - np.asarray(minp, dtype=np.int64)
    return ((q >= 0) & (q < np.asarray(dims, dtype=np.int64))).all(axis=1)


def unguarded_index(chunks, dims=DIMS, minp=MINP):
    """linearizeChunkPos as the reference's isSDFBlockStreamedOut applies it to any chunk: 32-bit integer arithmetic,
    the result taken as unsigned -> int64 in [0, 2^32)"""
    q = np.asarray(chunks, dtype=np.int64).reshape(-1, 3) - np.asarray(minp, dtype=np.int64)
    return (q[:, 2] * dims[0] * dims[1] + q[:, 1] * dims[0] + q[:, 0]) & 0xFFFFFFFF


def signed_unguarded_index(chunks, dims=DIMS, minp=MINP):
    """the same before the conversion to unsigned: negative for an index in front of the mask"""
    q = np.asarray(chunks, dtype=np.int64).reshape(-1, 3) - np.asarray(minp, dtype=np.int64)
    return q[:, 2] * dims[0] * dims[1] + q[:, 1] * dims[0] + q[:, 0]


def classify(blocks, voxel_size, ext=EXT, dims=DIMS, minp=MINP):
    """-> dict over blocks [n, 3]: chunk [n, 3], inside [n] bool, bit [n] (the bit index; -1 outside the grid),
    unguarded [n] (signed), face [n, 6] bool (past x-low, x-high, y-low, y-high, z-low, z-high)"""
    chunk = world_to_chunks(block_to_world(blocks, voxel_size), ext)
    inside = chunk_inside(chunk, dims, minp)
    raw = signed_unguarded_index(chunk, dims, minp)
    q = chunk - np.asarray(minp, dtype=np.int64)
    d = np.asarray(dims, dtype=np.int64)
    face = np.stack([q[:, 0] < 0, q[:, 0] >= d[0], q[:, 1] < 0, q[:, 1] >= d[1], q[:, 2] < 0, q[:, 2] >= d[2]], axis=1)
    return dict(chunk=chunk, inside=inside, bit=np.where(inside, raw, -1), unguarded=raw, face=face)


def near_ties(blocks, voxel_size, ext=EXT, eps=1e-3):
    """how many block coordinates lie within eps of a rounding tie of worldToChunks: |world / extents| = k + 1/2"""
    p = np.abs(block_to_world(blocks, voxel_size).astype(np.float64) / np.asarray(ext, dtype=np.float64))
    return int((np.abs(p - np.floor(p) - 0.5) < eps).sum())


def mask_of_bits(bits, n_bits=N_BITS):
    m = np.zeros((n_bits + 31) // 32, dtype=np.uint32)
    for b in np.asarray(bits, dtype=np.int64).ravel():
        assert 0 <= b < n_bits
        m[b // 32] |= np.uint32(1 << (b % 32))
    return m


def guarded_mask(mask):
    """-> (whole array, offset in words of the mask inside it): all-ones guard words on either side of the mask, so that
    an unguarded index stays inside an array this module made and reads 'streamed out'"""
    whole = np.full(len(mask) + 2 * GUARD_WORDS, 0xFFFFFFFF, dtype=np.uint32)
    whole[GUARD_WORDS:GUARD_WORDS + len(mask)] = mask
    return whole, GUARD_WORDS


def check_conditions(blocks, voxel_size, ext=EXT, dims=DIMS, minp=MINP):
    """Conditions on the inputs, asserted before anything is launched: the scene reaches past the grid, sits on the
    rounding ties, and an unguarded index stays within the guard words of guarded_mask().  -> classify()'s dict plus the
    counts the tests print."""
    c = classify(blocks, voxel_size, ext, dims, minp)
    n_in, n_out = int(c["inside"].sum()), int((~c["inside"]).sum())
    faces = c["face"][~c["inside"]].any(axis=0)
    ties = near_ties(blocks, voxel_size, ext)
    n_bits = dims[0] * dims[1] * dims[2]
    words = (n_bits + 31) // 32
    lo, hi = int(c["unguarded"].min()), int(c["unguarded"].max())
    assert n_in >= 50, n_in
    assert n_out >= 20, n_out
    assert faces.sum() >= 3, faces
    assert ties >= 50, ties
    assert lo >= 0, lo  # nothing in front of the mask: even an unguarded read starts at the mask's first word
    assert hi < 32 * (words + GUARD_WORDS), hi  # and ends before the guard words do
    aliased = int(((c["unguarded"] >= 0) & (c["unguarded"] < n_bits) & ~c["inside"]).sum())
    c.update(n_inside=n_in, n_outside=n_out, faces=faces, ties=ties, unguarded_range=(lo, hi), aliased=aliased)
    return c


def pos_set(positions):
    return set(map(tuple, np.asarray(positions, dtype=np.int64).reshape(-1, 3).tolist()))


# ---- the scene's blocks on the oracle, and alloc's three mask cases --------------------------------------------------

# chunks whose bit the third mask sets (bit indices of the grid at the origin): 12 lies on the x-low and y-low faces, 59 is
# the last chunk, 20 and 23 are the indices that most outside-grid blocks of the scene alias
CRAFTED_BITS = (12, 20, 23, 59)
MASK_CASES = ("none", "all", "crafted")


def alloc_to_fixed_point(o, depth, color, mask):
    prev = -1
    while True:  # CUDASceneRepHashSDF::alloc, offline branch
        o.reset_mutex()
        o.alloc(depth, color, mask)
        cur = o.heap_free_count()
        if cur == prev:
            return
        prev = cur


def oracle_blocks(O, mask=None, shifted=False, minp=MINP):
    """the blocks the oracle allocates for the scene's three poses under `mask` (a numpy view: its address is passed on)"""
    hp, cp, rp = small_config(WIDTH, HEIGHT, PARAMS, streaming_extents=EXT, streaming_dims=DIMS, streaming_min=minp)
    o = O.OracleScene(hp, cp, rp, T.make_scene_options(offline=True, gc=False))
    for k in ALLOC_POSES:
        pose = orbit_pose(k, shifted)
        depth, color = O.synth_frame(SHIFTED_S1 if shifted else synth.S1_SPHERES, 0, pose, cp)
        o.set_transform(pose)
        alloc_to_fixed_point(o, depth, color, mask)
    return o, hp


def case_mask(case):
    bits = dict(none=(), all=range(N_BITS), crafted=CRAFTED_BITS)[case]
    whole, at = guarded_mask(mask_of_bits(bits))
    return whole, whole[at:at + (N_BITS + 31) // 32]


def expected_blocks(case, positions, info):
    """what alloc must leave under the case's mask, from the restatement applied to the unmasked block set: a block is
    suppressed iff its chunk is inside the grid and that chunk's bit is set"""
    bits = dict(none=(), all=range(N_BITS), crafted=CRAFTED_BITS)[case]
    suppressed = info["inside"] & np.isin(info["bit"], np.array(list(bits), dtype=np.int64))
    return pos_set(positions[~suppressed])
