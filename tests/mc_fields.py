"""Crafted voxel fields for marching cubes, and a float64 restatement of the extraction (plain numpy, no GPU).

planted():      a 32 x 32 x 16 voxel field (4 x 4 x 2 blocks) in which every one of the 256 corner-sign patterns is
                planted once; its neighbour cells bring every cube case more than once.
random_field(): blocks of small random distances with unobserved voxels, values at the snapping threshold of
                vertexInterp and values at the size of the marching-cubes thresholds strewn in.
reference():    marching cubes in float64 on such a field, with a flag per cell that says whether float32 rounding
                could change any of its decisions.

The geometry (DSC/MarchingCubesSDFUtil.h:154-235, DSC/RayCastSDFUtil.h:97-116): the cell of voxel v is the cube
v - 1/2 .. v + 1/2 (in voxels); its corner (bx, by, bz) is the lattice point v - 1/2 + (bx, by, bz), and the sample
there is a trilinear interpolation with all three weights 1/2: the mean of the eight voxels v - 1 + b + {0, 1}^3.
"""
import os
import sys

import numpy as np

from voxelhashing_amd import vhtypes as T

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

B = T.SDF_BLOCK_SIZE
PLANTED_BLOCKS = (4, 4, 2)
SNAP = float(np.float32(0.00001))  # vertexInterp's threshold
SPECIAL = np.array([0.0, -0.0, 9e-6, -9e-6, 1.1e-5, -1.1e-5, 1e-30, -1e-30], dtype=np.float32)

# bit b of the cube index <- the corner x | y << 1 | z << 2 (the reference's order 010,110,100,000,011,111,101,001)
CASE_BIT_CORNER = (2, 3, 1, 0, 6, 7, 5, 4)
# the 12 edges as pairs of corners x | y << 1 | z << 2, in vertlist order (first end, second end)
EDGE_ENDS = ((2, 3), (3, 1), (1, 0), (0, 2), (6, 7), (7, 5), (5, 4), (4, 6), (2, 6), (3, 7), (1, 5), (0, 4))


# ---------------------------------------------------------------------------- builders

def _to_blocks(origin_block, nblocks, sdf, weight, color):
    """dense [x, y, z] voxel arrays -> (descs, blocks): blocks in x-fastest order, voxels x fastest inside a block"""
    nx, ny, nz = nblocks
    descs = np.zeros(nx * ny * nz, T.DESC_DTYPE)
    blocks = np.zeros((len(descs), T.SDF_BLOCK_VOXELS), T.VOXEL_DTYPE)
    n = 0
    for bz in range(nz):
        for by in range(ny):
            for bx in range(nx):
                descs["pos"][n] = (origin_block[0] + bx, origin_block[1] + by, origin_block[2] + bz)
                sl = (slice(B * bx, B * bx + B), slice(B * by, B * by + B), slice(B * bz, B * bz + B))
                blocks["sdf"][n] = sdf[sl].transpose(2, 1, 0).ravel()
                blocks["weight"][n] = weight[sl].transpose(2, 1, 0).ravel()
                blocks["color"][n] = color[sl].transpose(2, 1, 0, 3).reshape(-1, 3)
                n += 1
    return descs, blocks


def pattern_voxel(p):
    """field-local voxel that carries sign pattern p"""
    return np.array([4 * (p & 7) + 1, 4 * ((p >> 3) & 7) + 1, 4 * (p >> 6) + 1])


def case_of_pattern(p):
    """the reference's cube index of the cell whose corner x | y << 1 | z << 2 is negative where that bit of p is set"""
    return sum(1 << b for b, c in enumerate(CASE_BIT_CORNER) if (p >> c) & 1)


def planted(origin_block, voxel_size, amplitude, holes=0.0, seed=0):
    """-> (descs, blocks) of 4 x 4 x 2 blocks at origin_block.  Pattern p sits at voxel c = pattern_voxel(p); the eight
    diagonal neighbours c + (+-1, +-1, +-1) hold -amplitude where bit x | y << 1 | z << 2 of p is set (x = 1: +1) and
    +amplitude otherwise.  Every other voxel holds 0, every weight is 1, colours are random bytes.  A lattice point
    then has at most one non-zero voxel among its eight: every corner sample is +-amplitude / 8 (or 0 between the
    outermost patterns and the field's border, where the cells are skipped for their missing neighbours anyway).
    holes: that share of the voxels gets weight 0 (the planted ones included).  voxel_size is not used: amplitude is
    in metres already."""
    nx, ny, nz = (B * n for n in PLANTED_BLOCKS)
    rng = np.random.default_rng(1000 + seed)
    sdf = np.zeros((nx, ny, nz), np.float32)
    for p in range(256):
        c = pattern_voxel(p)
        for b in range(8):
            d = np.array([(b & 1) * 2 - 1, ((b >> 1) & 1) * 2 - 1, ((b >> 2) & 1) * 2 - 1])
            sdf[tuple(c + d)] = -amplitude if (p >> b) & 1 else amplitude
    weight = np.ones((nx, ny, nz), np.uint8)
    color = rng.integers(0, 256, (nx, ny, nz, 3), dtype=np.uint8)
    if holes > 0.0:
        weight[rng.random((nx, ny, nz)) < holes] = 0
    return _to_blocks(origin_block, PLANTED_BLOCKS, sdf, weight, color)


def block_ids(lo=-1, hi=1):
    """the (hi - lo + 1)^3 blocks of the cube lo..hi, x fastest"""
    r = range(lo, hi + 1)
    return np.array([(x, y, z) for z in r for y in r for x in r], np.int32)


# 9 of the 27 blocks of (-1..1)^3: the centre, three face, three edge and two corner neighbours of it.  The 18 blocks
# that stay then miss neighbours of every kind.
LEFT_OUT = np.array([(0, 0, 0), (1, 0, 0), (0, -1, 0), (0, 0, 1), (1, 1, 0), (-1, 0, 1), (0, -1, -1), (1, 1, 1), (-1, -1, 1)], np.int32)


def without(descs, blocks, ids):
    keep = ~np.array([any(tuple(p) == tuple(q) for q in ids) for p in descs["pos"]])
    return descs[keep], blocks[keep]


def random_field(ids, seed, thres, holes=0.0, special=0.0, large=0.0):
    """-> (descs, blocks) for the blocks `ids`: magnitudes 0.45 * thres * u^3 (u uniform in [0, 1)) with random signs,
    so that most cells pass the thresholds and small values are common; then a share `special` of the voxels takes a
    value of SPECIAL (zeros of both signs, values either side of vertexInterp's 1e-5, a value whose products
    underflow), a share `large` a value of +-(0.5 .. 1.2) * thres (cells at and over the thresholds), and a share
    `holes` weight 0.  Other weights are 1..255, colours random bytes."""
    ids = np.asarray(ids, np.int32).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    shape = (len(ids), T.SDF_BLOCK_VOXELS)
    u = rng.random(shape)
    sdf = (0.45 * thres * u ** 3 * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    pick = rng.random(shape)
    sdf = np.where(pick < special, SPECIAL[rng.integers(0, len(SPECIAL), shape)], sdf)
    big = (rng.uniform(0.5, 1.2, shape) * thres * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    sdf = np.where((pick >= special) & (pick < special + large), big, sdf).astype(np.float32)
    blocks = np.zeros(shape, T.VOXEL_DTYPE)
    blocks["sdf"] = sdf
    blocks["weight"] = rng.integers(1, 256, shape, dtype=np.uint8)
    blocks["weight"][rng.random(shape) < holes] = 0
    blocks["color"] = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    descs = np.zeros(len(ids), T.DESC_DTYPE)
    descs["pos"] = ids
    return descs, blocks


# ---------------------------------------------------------------------------- float64 restatement

def sample_error_bound(max_sdf, q):
    """eps_d: how far a float32 corner sample can lie from the float64 one, for voxel values up to max_sdf in
    magnitude and voxel coordinates up to q in magnitude.

      margin = 64 * 2^-24 * (1 + q / 2^4) * max|sdf|

    The sample is sum_k s_k v_k over eight taps with s_k = wx' wy' wz', w' = w or 1 - w (RayCastSDFUtil.h:97-116).
    * Arithmetic, with the weights as they are (u = 2^-24, the largest relative error of one rounding): 1 - w costs
      at most one rounding, s_k two more, s_k v_k one more: 4 u |s_k v_k| per tap, in all 4 u max|sdf| since the s_k
      sum to 1.  Each of the seven sums rounds a partial sum no larger than max|sdf|: 7 u max|sdf|.  11 u max|sdf|
      together; 64 u leaves room for the second-order terms and for the few ulps by which the weights move the taps.
    * The weights themselves: w = frac(pos / voxel) where pos = fl(fl(v * voxel) +- voxel / 2) is three roundings
      away from (v +- 1/2) voxel, so pos / voxel is off by up to 3 (q + 1) u and so is each w (the true value is
      1/2).  d(sample)/dw along one axis is the difference of the two face means of the eight taps weighted 1/4 each:
      on the planted field, where one tap of eight is non-zero, 1/4 max|sdf|, over the three axes
      3/4 * 3 (q + 1) u max|sdf| < 4 q u max|sdf| = 64 u (q / 2^4) max|sdf| for q >= 2.  On a general field the face
      means can differ by up to 2 max|sdf| (eight times as much); the random fields here have q <= 16 and values
      far below their max|sdf| nearly everywhere, and the formula is used as it stands.
    """
    return 64.0 * 2.0 ** -24 * (1.0 + q / 16.0) * max_sdf


def reference(descs, blocks, voxel_size, mp):
    """Marching cubes in float64 over every voxel of the blocks given.  -> dict, one entry per cell unless said:
      cell        (N, 3) voxel coordinates
      color       (N, 3) the own voxel's colour bytes
      valid       all eight corner samples exist (no tap of weight 0 or in a missing block)
      holed       some tap is a voxel of an existing block with weight 0
      d           (N, 8) corner samples, corner x | y << 1 | z << 2 (0 where not valid)
      case        the reference's cube index
      emits       valid, passes both threshold rules, edge mask neither 0 nor 255
      ntri        triangles the cell gives
      decided     no float32 rounding within `margin` can change `emits`, `case` or a snap decision of the cell
      margin      sample_error_bound(max|sdf|, Q), Q the largest voxel coordinate magnitude
      tri_cell    (M,) index of the cell of every triangle, cells in order
      tri_edges   (M, 3) its three edges
      tri_pos     (M, 3, 3) float64 vertex positions
      tri_gap     (M, 3) |d2 - d1| of each vertex's edge
      tri_snap    (M, 3) 0 interpolated, 1 / 2 snapped to the first / second end (|d| < 1e-5)
    """
    import gen_mc_tables as G
    tri_table, edge_table = G.tables()
    vs = float(np.float32(voxel_size))
    pos = descs["pos"].astype(np.int64)
    lo = pos.min(axis=0)
    ext = pos.max(axis=0) - lo + 1
    # dense volume with a one-voxel rim of absent voxels (weight 0)
    shape = tuple(int(e) * B + 2 for e in ext)
    sdf = np.zeros(shape, np.float64)
    wgt = np.zeros(shape, np.int64)
    own = np.zeros(shape, bool)
    col = np.zeros(shape + (3,), np.uint8)
    for p, blk in zip(pos, blocks):
        o = (p - lo) * B + 1
        sl = (slice(o[0], o[0] + B), slice(o[1], o[1] + B), slice(o[2], o[2] + B))
        sdf[sl] = blk["sdf"].astype(np.float64).reshape(B, B, B).transpose(2, 1, 0)
        wgt[sl] = blk["weight"].reshape(B, B, B).transpose(2, 1, 0)
        col[sl] = blk["color"].reshape(B, B, B, 3).transpose(2, 1, 0, 3)
        own[sl] = True
    # lattice point i (per axis) lies between voxels i and i + 1 of the dense volume
    n = [s - 1 for s in shape]
    lat = np.zeros(n, np.float64)
    seen = np.ones(n, bool)
    hole = np.zeros(n, bool)  # a tap that exists and has weight 0
    for b in range(8):
        sl = tuple(slice(k, k + m) for k, m in zip((b & 1, (b >> 1) & 1, b >> 2), n))
        lat += sdf[sl]
        seen &= wgt[sl] > 0
        hole |= own[sl] & (wgt[sl] == 0)
    lat /= 8.0
    idx = np.argwhere(own)  # dense indices, z slowest is not needed: order is ours
    idx = idx[np.lexsort((idx[:, 0], idx[:, 1], idx[:, 2]))]
    cell = idx - 1 + lo * B
    d = np.zeros((len(idx), 8))
    valid = np.ones(len(idx), bool)
    holed = np.zeros(len(idx), bool)
    for c in range(8):
        at = (idx[:, 0] - 1 + (c & 1), idx[:, 1] - 1 + ((c >> 1) & 1), idx[:, 2] - 1 + (c >> 2))
        d[:, c] = lat[at]
        valid &= seen[at]
        holed |= hole[at]
    d[~valid] = 0.0
    q = float(np.abs(cell).max())
    max_sdf = float(np.abs(blocks["sdf"].astype(np.float64)).max())
    margin = sample_error_bound(max_sdf, q)

    case = np.zeros(len(idx), np.int64)
    for b, c in enumerate(CASE_BIT_CORNER):
        case += (d[:, c] < 0.0).astype(np.int64) << b
    thres, thres2 = float(mp.m_threshMarchingCubes), float(mp.m_threshMarchingCubes2)
    ok = valid.copy()
    near = np.zeros(len(idx), bool)  # some comparison lies within reach of rounding
    for k in range(8):
        for l in range(8):
            opposite = d[:, k] * d[:, l] < 0.0
            expr = np.where(opposite, np.abs(d[:, k]) + np.abs(d[:, l]), np.abs(d[:, k] - d[:, l]))
            ok &= ~(expr > thres)
            near |= np.abs(expr - thres) <= 2.0 * margin  # two samples, each off by up to margin
    for k in range(8):
        ok &= ~(np.abs(d[:, k]) > thres2)
        near |= np.abs(np.abs(d[:, k]) - thres2) <= margin
        near |= np.abs(d[:, k]) <= margin
        near |= np.abs(np.abs(d[:, k]) - SNAP) <= margin
    edges = np.array(edge_table)[case]
    emits = ok & (edges != 0) & (edges != 255)
    decided = ~near | ~valid  # a cell with a missing tap is skipped whatever its samples are
    lists = []
    for c in range(256):
        e = [(tri_table[c] >> (4 * k)) & 0xF for k in range(16)]
        e = e[:e.index(0xF)] if 0xF in e else e
        lists.append(np.array(e, np.int64).reshape(-1, 3))
    ntri = np.where(emits, np.array([len(l) for l in lists])[case], 0)

    tri_cell = np.repeat(np.arange(len(idx)), ntri)
    tri_edges = np.concatenate([lists[c] for c in case[emits]] + [np.zeros((0, 3), np.int64)])
    ends = np.array(EDGE_ENDS)
    a, b = ends[tri_edges, 0], ends[tri_edges, 1]  # (M, 3) corners
    d1 = np.take_along_axis(d[tri_cell], a, axis=1)
    d2 = np.take_along_axis(d[tri_cell], b, axis=1)
    world = cell[tri_cell].astype(np.float64) * vs  # (M, 3)
    half = vs / 2.0

    def corner_pos(c):  # (M, 3) corners -> (M, 3, 3)
        bits = np.stack([c & 1, (c >> 1) & 1, c >> 2], axis=-1)
        return world[:, None, :] + np.where(bits == 1, half, -half)

    p1, p2 = corner_pos(a), corner_pos(b)
    snap = np.where(np.abs(d1) < SNAP, 1, np.where(np.abs(d2) < SNAP, 2, 0))
    gap = np.abs(d2 - d1)
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = np.where(snap == 0, -d1 / (d2 - d1), np.where(snap == 1, 0.0, 1.0))
    tri_pos = p1 + mu[..., None] * (p2 - p1)
    return dict(cell=cell, color=col[idx[:, 0], idx[:, 1], idx[:, 2]], holed=holed, valid=valid, d=d, case=case, emits=emits, ntri=ntri, decided=decided, margin=margin,
                tri_cell=tri_cell, tri_edges=tri_edges, tri_pos=tri_pos, tri_gap=gap, tri_snap=snap, max_sdf=max_sdf, q=q)


def cell_keys(cells, lo):
    """one integer per voxel coordinate triple (coordinates within 2^20 of lo)"""
    c = np.asarray(cells, np.int64) - np.asarray(lo, np.int64) + 4
    return (c[..., 0] << 42) | (c[..., 1] << 21) | c[..., 2]


def group_by_cell(tris, ref, voxel_size):
    """the cell of every triangle of a soup, from its vertices: the voxel v whose cube v +- 1/2 holds all three
    positions.  A triangle that lies in a face of its cube (it has a snapped vertex, as a rule) fits the cell on
    either side; the colour decides then: every vertex carries the colour of its cell's own voxel, and the fields
    here have random colours.  -> (index into ref["cell"] per triangle, -1 where no cell or more than one fits;
    how many triangles needed the colour)"""
    vs = float(np.float32(voxel_size))
    x = tris["v"]["p"].astype(np.float64) / vs  # (n, 3 vertices, 3 axes)
    eps = 1e-3 + ref["q"] * 2.0 ** -20
    lo = np.ceil(x.max(axis=1) - 0.5 - eps).astype(np.int64)
    hi = np.floor(x.min(axis=1) + 0.5 + eps).astype(np.int64)
    assert np.all(lo <= hi) and np.all(hi - lo <= 1), "a triangle larger than a cell"
    base = ref["cell"].min(axis=0)
    keys = cell_keys(ref["cell"], base)
    order = np.argsort(keys)
    col = tris["v"]["c"][:, 0, :]  # v.color / 255.f, the same for the three vertices
    want = (ref["color"].astype(np.float32) / np.float32(255.0))
    found = np.full(len(tris), -1, np.int64)
    hits = np.zeros(len(tris), np.int64)
    for b in range(8):
        off = np.array([b & 1, (b >> 1) & 1, b >> 2])
        take = np.all((off == 0) | (hi > lo), axis=1)  # each candidate once
        cand = lo + off
        k = cell_keys(cand, base)
        at = np.clip(np.searchsorted(keys[order], k), 0, len(keys) - 1)
        idx = order[at]
        ok = take & (keys[idx] == k) & np.all(want[idx] == col, axis=1)
        found = np.where(ok, idx, found)
        hits += ok
    found[hits != 1] = -1
    return found, int(np.any(lo < hi, axis=1).sum())


def weld_inputs_in_range(descs):
    """whether every lattice point of every cell of the blocks has a key (vh_mesh_key: -2^19 <= L < 2^19); the cells
    of the outermost voxels count, though they give no triangle while their neighbour blocks are missing"""
    v = descs["pos"].astype(np.int64) * B
    return bool(v.min() >= -(1 << 19) and v.max() + B - 1 + 1 < (1 << 19))


# ---------------------------------------------------------------------------- the cases the tests share

NEAR, FAR = (-2, -2, -1), (65530, -2, -1)  # FAR: voxel coordinates just under 2^19, every lattice point still has a weld key
SWEEP_KS = (-64, -8, -2, -1, 0, 1, 2, 8, 64)
# triangles the oracle extracts from planted(origin, amplitude = sweep_amplitude(thres, k)), P2 and P4 alike; the
# reference's own code gives the same (tests/test_reference_pinning_kernels.py)
SWEEP_COUNTS = {NEAR: (18626, 18282, 14972, 12893, 12893, 3759, 3759, 22, 0),
                FAR: (12644, 12610, 11473, 10651, 10651, 4857, 4857, 3168, 3168)}
RANDOM = dict(holes=0.03, special=0.05, large=0.01)
RANDOM_SEEDS = (("P4", 1), ("P2", 5))  # fields with snapped vertices of both kinds (counted by the tests)


def sweep_amplitude(thres, k):
    """4 * thres * (1 + k * 2^-22) in float32: corner samples of thres / 2 * (1 + k 2^-22), so that the sum over a
    crossing edge steps over thres ulp by ulp"""
    return np.float32(4.0) * np.float32(thres) * np.float32(1.0 + k * 2.0 ** -22)


def config(name, num_buckets=1 << 10, num_sdf_blocks=256, max_triangles=1 << 16, **kw):
    """-> (hash params, camera params, marching-cubes params, voxel size as float32) for parameter set `name`"""
    from voxelhashing_amd import synth
    hp = T.make_hash_params(num_buckets, num_sdf_blocks, **synth.PARAM_SETS[name], **kw)
    return hp, T.make_depth_camera_params(64, 48), T.make_marching_cubes_params(hp, max_triangles), np.float32(hp.m_virtualVoxelSize)
