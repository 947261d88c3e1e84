"""What k_interval_splat decides for every 8x8-pixel tile, restated twice in numpy and once for its schedule
(tests/test_tile_intervals.py checks the models against each other on the CPU, tests/test_gpu_tile_intervals.py checks
the kernel against them):

  needed_pairs    float64, independent of the kernel's reasoning: the (tile, block) pairs for which a pixel ray of the
                  tile, between the two depth limits, passes through the block's reach box -- a slab test per pixel ray
                  and box, no projection of corners;
  splat_model     float32, the kernel's rule operation by operation (the library is built with -ffp-contract=off, so
                  every multiply and add is rounded once, as numpy's float32 arithmetic is): the pairs it lists, the
                  count per tile, the depth range {lo, hi} of every block as float bits;
  schedule_model  schedule_tiles' deal: for every launch slot the cost class of the tile it holds and its half.

TABLES and VIEWS are the scenes both test files use; a table is built by the oracle on the CPU and by the engine on
the GPU from the same frames."""
import numpy as np

import crowded as CR
from helpers import small_config
from voxelhashing_amd import synth, vhtypes as T

F = np.float32
BLOCK = T.SDF_BLOCK_SIZE
TIE_SHRINK = 1e-4  # voxels taken off every face of the reach box: float32-against-float64 ties are never asserted
CAP_SMALL, CAP_LARGE = 64, 128  # VH_TILE_LIST_CAPACITY, VH_TILE_LIST_CAPACITY_LARGE
COST_CLASSES = 32
SPLIT_MIN_TILES, SPLIT_MAX, SPLIT_DIV, SCHED_GROUPS = 1024, 256, 16, 8


# ------------------------------------------------------------------------------------------------ scenes and views

def rigid_inverse(pose):
    """world -> camera of a rigid camera -> world matrix, in double, rounded once -> float32 [4, 4]"""
    m = np.asarray(pose, np.float64).reshape(4, 4)
    out = np.eye(4)
    out[:3, :3] = m[:3, :3].T
    out[:3, 3] = -m[:3, :3].T @ m[:3, 3]
    return out.astype(F)


def look_pose(eye, yaw=0.0, pitch=0.0, roll=0.0):
    """camera -> world, float32[16]: at `eye`, looking along +z turned by yaw (about y), pitch (about x), roll (about z)"""
    cy, sy, cx, sx, cz, sz = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    m = np.eye(4)
    m[:3, :3] = ry @ rx @ rz
    m[:3, 3] = eye
    return m.astype(F).reshape(16)


def _orbit(n, of=40):
    return [synth.orbit_pose(k, of) for k in range(n)]


# table name -> how it is made: (HashParams, DepthCameraParams, RayCastParams) of the frames, scene options, poses
TABLES = {
    "A": lambda: dict(cfg=CR.config("A"), opt=CR.options(), poses=CR.poses("A")),  # crowded scenario A: 2 cm, 180 buckets
    "P4": lambda: dict(cfg=small_config(96, 72, "P4", num_buckets=1 << 12), opt=T.make_scene_options(offline=True, gc=False), poses=_orbit(3)),
    "P8": lambda: dict(cfg=small_config(96, 72, "P4", num_buckets=1 << 12, voxel_size=0.08, truncation=0.40, trunc_scale=0.20),
                       opt=T.make_scene_options(offline=True, gc=False), poses=_orbit(4)),
    "P1": lambda: dict(cfg=small_config(96, 72, "P1", num_buckets=1 << 12), opt=T.make_scene_options(offline=True, gc=False), poses=_orbit(3)),
}

# view name -> (table, width, height, camera -> world).  S1's big sphere is centred on the origin with radius 1.
VIEWS = {
    "orbit_2cm": ("A", 96, 72, CR.poses("A")[-1]),                 # the 2 cm orbit view of crowded scenario A, 2.5 m away
    "close_8cm": ("P8", 96, 72, look_pose((0.3, 0.0, -1.8))),       # a voxel spans about ten pixels
    "ragged_2cm": ("A", 91, 67, CR.poses("A")[0]),                  # no multiple of the tile in either direction
    "tilted_8cm": ("P8", 96, 72, look_pose((0.3, 0.0, -1.8), yaw=0.4, roll=0.1)),  # blocks straddle the border
    "inside_4cm": ("P4", 96, 72, look_pose((0.05, 0.02, -1.01), yaw=1.2, pitch=0.1)),  # in the block band: blocks behind, across z = 0.05
    "fine_1cm": ("P1", 48, 36, look_pose((0.0, 0.0, -3.4))),        # counts beyond 64 and beyond 128
}


def table_frames(name):
    """-> (hp, cp, rp, options, poses) of a table"""
    t = TABLES[name]()
    hp, cp, rp = t["cfg"]
    return hp, cp, rp, t["opt"], t["poses"]


def oracle_blocks(O, name):
    """the table's block positions [n, 3] int32 as the oracle builds it (the GPU test compares its own table with this)"""
    from voxelhashing_amd import canonical
    hp, cp, rp, opt, poses = table_frames(name)
    o = O.OracleScene(hp, cp, rp, opt)
    for pose in poses:
        o.integrate(pose, *O.synth_frame(synth.S1_SPHERES, 0, pose, cp))
    return canonical.block_positions(o.hash_table()).reshape(-1, 3).astype(np.int32)


class View:
    """what the splat is given for one view: intrinsics, image size, the two view matrices, depth limits, voxel size"""

    def __init__(self, name, hp, spec=None):
        table, W, H, pose = spec or VIEWS[name]
        self.name, self.table, self.W, self.H = name, table, W, H
        self.pose = np.asarray(pose, F).reshape(16)
        self.cp = T.make_depth_camera_params(W, H)
        self.view = rigid_inverse(self.pose)
        self.vs = float(hp.m_virtualVoxelSize)
        self.min_depth, self.max_depth = float(self.cp.m_sensorDepthWorldMin), float(self.cp.m_sensorDepthWorldMax)
        self.tiles_x, self.tiles_y = (W + 7) // 8, (H + 7) // 8
        self.n_tiles = self.tiles_x * self.tiles_y

    def raycast_params(self, hp, gradients):
        rp = T.make_raycast_params(hp, self.cp, use_gradients=gradients)
        rp.m_viewMatrix = T.mat16(self.view)
        rp.m_viewMatrixInverse = T.mat16(self.pose.reshape(4, 4))
        return rp

    def intrinsics(self):
        return tuple(float(F(v)) for v in (self.cp.fx, self.cp.fy, self.cp.mx, self.cp.my))


# ------------------------------------------------------------------------------------------------ (a) what the rays need

def reach_box(blocks, vs, gradients, shrink=TIE_SHRINK):
    """per block the positions whose sample can read one of its voxels, float64 -> (lo [n, 3], hi [n, 3]): along each
    axis p / vs in [8b - 1, 8b + 8), half a voxel more on both sides with gradients, shrunk by `shrink` voxels"""
    b = np.asarray(blocks, np.float64).reshape(-1, 3)
    extra = 0.5 if gradients else 0.0
    return (BLOCK * b - 1.0 - extra + shrink) * vs, (BLOCK * b + BLOCK + extra - shrink) * vs


def needed_pairs(blocks, vs, cam_to_world, intrinsics, width, height, min_depth, max_depth, gradients, chunk=128):
    """-> (need [tiles, blocks] bool, zlo, zhi [tiles, blocks] float64): the pixel rays of tile t pass through the reach
    box of block b at camera depths zlo .. zhi (their union over the tile's pixels; +inf / -inf where need is False).
    The ray of pixel (x, y) is camera + z ((x - mx) / fx, (y - my) / fy, 1) for min_depth <= z <= max_depth, taken to
    the world by cam_to_world in float64; every ray is tested against every box (slab test)."""
    fx, fy, mx, my = intrinsics
    m = np.asarray(cam_to_world, np.float64).reshape(4, 4)
    tx, ty = (width + 7) // 8, (height + 7) // 8
    # pixels tile by tile: [tiles, 64]
    t = np.arange(tx * ty)
    lane = np.arange(64)
    px = (t[:, None] % tx) * 8 + (lane[None, :] & 7)
    py = (t[:, None] // tx) * 8 + (lane[None, :] >> 3)
    inside = (px < width) & (py < height)
    d_cam = np.stack([(px - mx) / fx, (py - my) / fy, np.ones(px.shape)], axis=-1)  # [tiles, 64, 3]
    d = d_cam @ m[:3, :3].T
    o = m[:3, 3]
    lo, hi = reach_box(blocks, vs, gradients)
    n = len(lo)
    need = np.zeros((tx * ty, n), bool)
    zlo = np.full((tx * ty, n), np.inf)
    zhi = np.full((tx * ty, n), -np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d  # +-inf where a ray runs along a slab
        for c0 in range(0, n, chunk):
            l, h = lo[c0:c0 + chunk], hi[c0:c0 + chunk]
            near = np.full(d.shape[:2] + (len(l),), min_depth)
            far = np.full(d.shape[:2] + (len(l),), max_depth)
            for ax in range(3):
                a = (l[None, None, :, ax] - o[ax]) * inv[:, :, None, ax]
                b = (h[None, None, :, ax] - o[ax]) * inv[:, :, None, ax]
                along = (d[:, :, None, ax] == 0.0)
                within = (o[ax] >= l[:, ax]) & (o[ax] <= h[:, ax])
                # a ray that runs along the slab is in it for every z or for none
                a = np.where(along, np.where(within, -np.inf, np.inf)[None, None, :], a)
                b = np.where(along, np.inf, b)
                near = np.maximum(near, np.minimum(a, b))
                far = np.minimum(far, np.maximum(a, b))
            hit = (near <= far) & inside[:, :, None]
            need[:, c0:c0 + chunk] = hit.any(axis=1)
            zlo[:, c0:c0 + chunk] = np.where(hit, near, np.inf).min(axis=1)
            zhi[:, c0:c0 + chunk] = np.where(hit, far, -np.inf).max(axis=1)
    return need, zlo, zhi


def needed_for(view, blocks, gradients):
    return needed_pairs(blocks, view.vs, view.pose, view.intrinsics(), view.W, view.H, view.min_depth, view.max_depth, gradients)


# ------------------------------------------------------------------------------------------------ (b) the kernel's rule

def splat_model(blocks, vs, view_matrix, intrinsics, width, height, gradients, margins=None, slop=True):
    """interval_splat_group in float32, one rounding per operation, in the kernel's order.
    margins: (low, high) growth of the box in voxels instead of the kernel's 1.25 / 0.25 (1.75 / 0.75 with gradients);
    slop=False drops the screen rectangle's slop -- both only for the mutation table.
    -> dict listed [tiles, blocks] bool, count [tiles], lo / hi [blocks] uint32 (float bits of the block's depth range),
       rect [blocks, 4] (tx0, ty0, tx1, ty1; an empty rectangle for a block that is given to no tile)"""
    fx, fy, mx, my = (F(v) for v in intrinsics)
    m = np.asarray(view_matrix, F).reshape(16)
    b = np.asarray(blocks, np.int32).reshape(-1, 3)
    vs = F(vs)
    tx, ty = (width + 7) // 8, (height + 7) // 8
    g_lo, g_hi = margins if margins is not None else ((1.75, 0.75) if gradients else (1.25, 0.25))
    grow_lo, grow_hi = F(g_lo) * vs, F(g_hi) * vs
    lo3 = (b * BLOCK).astype(F) * vs - grow_lo
    hi3 = (b * BLOCK + BLOCK).astype(F) * vs + grow_hi
    inf = F(np.inf)
    n = len(b)
    zmin, xmin, ymin = np.full(n, inf), np.full(n, inf), np.full(n, inf)
    zmax, xmax, ymax = np.full(n, -inf), np.full(n, -inf), np.full(n, -inf)
    one = F(1.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(8):
            x = hi3[:, 0] if c & 1 else lo3[:, 0]
            y = hi3[:, 1] if c & 2 else lo3[:, 1]
            z = hi3[:, 2] if c & 4 else lo3[:, 2]
            pcx = m[0] * x + m[1] * y + m[2] * z + m[3] * one  # mat_mul_p: left to right
            pcy = m[4] * x + m[5] * y + m[6] * z + m[7] * one
            pcz = m[8] * x + m[9] * y + m[10] * z + m[11] * one
            zmin, zmax = np.minimum(zmin, pcz), np.maximum(zmax, pcz)
            iz = one / np.maximum(pcz, F(1e-6))
            sx = pcx * fx * iz + mx
            sy = pcy * fy * iz + my
            xmin, xmax = np.minimum(xmin, sx), np.maximum(xmax, sx)
            ymin, ymax = np.minimum(ymin, sy), np.maximum(ymax, sy)
        assert all(a.dtype == F for a in (zmin, zmax, xmin, xmax, ymin, ymax))
        sl = one + F(1e-3) * np.maximum(np.maximum(np.abs(xmin), np.abs(xmax)), np.maximum(np.abs(ymin), np.abs(ymax)))
        if not slop:
            sl = np.zeros(n, F)
        eighth = F(0.125)
        # the clamp in float comes before the conversion to int
        tx0 = np.minimum(np.maximum(np.floor((xmin - sl) * eighth), F(0.0)), F(tx)).astype(np.int32)
        ty0 = np.minimum(np.maximum(np.floor((ymin - sl) * eighth), F(0.0)), F(ty)).astype(np.int32)
        tx1 = np.minimum(np.maximum(np.floor((xmax + sl) * eighth), F(-1.0)), F(tx - 1)).astype(np.int32)
        ty1 = np.minimum(np.maximum(np.floor((ymax + sl) * eighth), F(-1.0)), F(ty - 1)).astype(np.int32)
    front = zmin > F(0.05)  # otherwise the box may project anywhere: every tile
    tx0, ty0 = np.where(front, tx0, 0), np.where(front, ty0, 0)
    tx1, ty1 = np.where(front, tx1, tx - 1), np.where(front, ty1, ty - 1)
    behind = ~(zmax > F(0.0))  # entirely behind the camera: no tile
    tx1 = np.where(behind, -1, tx1)
    zs = F(1e-3) * np.abs(zmax) + F(0.5) * vs
    lo = np.maximum(zmin - zs, F(0.0)).astype(F).view(np.uint32)
    hi = np.maximum(zmax + zs, F(0.0)).astype(F).view(np.uint32)
    tcol, trow = np.arange(tx * ty) % tx, np.arange(tx * ty) // tx
    listed = ((tcol[:, None] >= tx0[None, :]) & (tcol[:, None] <= tx1[None, :]) &
              (trow[:, None] >= ty0[None, :]) & (trow[:, None] <= ty1[None, :]))
    return dict(listed=listed, count=listed.sum(axis=1).astype(np.uint32), lo=lo, hi=hi, every_tile=~front & ~behind,
                rect=np.stack([tx0, ty0, tx1, ty1], axis=1))


def model_for(view, blocks, gradients, **mutation):
    return splat_model(blocks, view.vs, view.view, view.intrinsics(), view.W, view.H, gradients, **mutation)


# the mutation table of DESIGN.md section 2: what is changed in splat_model, by name
def mutations(gradients):
    lo, hi = (1.75, 0.75) if gradients else (1.25, 0.25)
    return {
        "low margin - 0.5 voxel": dict(margins=(lo - 0.5, hi)),
        "low margin - 1 voxel": dict(margins=(lo - 1.0, hi)),
        "margins swapped": dict(margins=(hi, lo)),
        "no-gradient margins with gradients": dict(margins=(1.25, 0.25)),  # (the rule itself without gradients)
        "slop removed": dict(slop=False),
    }


# ------------------------------------------------------------------------------------------------ (c) the deal

def class_patterns(n_tiles, seed):
    """the crafted cost classes both test files deal: all equal, a ramp, random 0 .. 40 (so that the clamp to 31 is used),
    one dear tile at the very end (in the short last quad, where the image has one)"""
    rng = np.random.default_rng(seed)
    last = np.zeros(n_tiles, np.int64)
    last[-1] = 31
    return {"equal": np.full(n_tiles, 7, np.int64), "ramp": np.arange(n_tiles, dtype=np.int64) % 40,
            "random": rng.integers(0, 41, n_tiles).astype(np.int64), "dear_last": last}


def split_tiles(n_tiles):
    n = (n_tiles // SPLIT_DIV) & ~1
    return min(n, SPLIT_MAX) if n_tiles >= SPLIT_MIN_TILES else 0


def sched_parts(n_tiles):
    return SCHED_GROUPS if n_tiles >= SPLIT_MIN_TILES else 1


def share_of(tile, n_tiles):
    """the share (sorting workgroup) of a tile: its quad of four tiles q = share (mod shares)"""
    return (np.asarray(tile) // 4) % sched_parts(n_tiles)


def slot_of_rank(i, n_tiles, num_cus, n_split):
    """the launch slot (the first of the two, for a split tile) of the tile of overall rank i"""
    if i < n_split:
        return (i // 2) * 4 + (i & 1) * 2
    n_groups = (n_tiles + n_split + 3) // 4
    full_rows = n_groups // num_cus
    j = i + n_split
    g = j // 4
    row, col = divmod(g, num_cus)
    if (row & 1) and row < full_rows and row * num_cus >= n_split // 2:  # odd full rows run backwards, unless they hold split tiles
        g = row * num_cus + (num_cus - 1 - col)
    return g * 4 + (j & 3)


def schedule_model(classes, n_tiles, num_cus, n_split):
    """-> dict over the 4 * ceil((n_tiles + n_split) / 4) launch slots:
         cls    the cost class (clamped to 31) of the tile the slot holds, -1 for a slot that stays empty
         half   0 whole tile, 1 / 2 near / far half of a split tile
         rank   the overall rank of that tile (-1 if empty), share: the share it came from
         tile   ONE deal that obeys the rule: equal classes of a share in ascending tile order (the kernel's order among
                them is the order of its atomics)
         writes how often the slot was written
    The class in a slot does not depend on the order of the atomics: a share's ranks run over its classes in
    descending order, whatever the sub-bins do."""
    cls = np.minimum(np.asarray(classes[:n_tiles], np.int64), COST_CLASSES - 1)
    parts = sched_parts(n_tiles)
    shares = []
    for w in range(parts):
        tiles = np.array([t for t in range(n_tiles) if (t // 4) % parts == w], np.int64)
        order = np.argsort(-cls[tiles], kind="stable") if len(tiles) else np.zeros(0, np.int64)
        shares.append(tiles[order])
    n_share = [len(s) for s in shares]
    n_slots = 4 * ((n_tiles + n_split + 3) // 4)
    out = dict(cls=np.full(n_slots, -1, np.int64), half=np.zeros(n_slots, np.int64), rank=np.full(n_slots, -1, np.int64),
               share=np.full(n_slots, -1, np.int64), tile=np.full(n_slots, -1, np.int64), writes=np.zeros(n_slots, np.int64))

    def put(at, tile, half, i, w):
        out["cls"][at], out["half"][at], out["rank"][at], out["share"][at], out["tile"][at] = cls[tile], half, i, w, tile
        out["writes"][at] += 1

    for w, tiles in enumerate(shares):
        for mine, tile in enumerate(tiles):
            # the shares take turns: rank `mine` of share w comes after rank `mine` of the shares before it; a share
            # that has run out is skipped
            i = sum(min(mine, n_share[v]) + (1 if v < w and n_share[v] > mine else 0) for v in range(parts))
            at = slot_of_rank(i, n_tiles, num_cus, n_split)
            if i < n_split:
                put(at, tile, 1, i, w)
                put(at + 1, tile, 2, i, w)
            else:
                put(at, tile, 0, i, w)
    return out


def check_deal(tile, half, n_tiles, n_split, what=""):
    """the properties every deal must have, on the accepted slots of a launch (tile < 0: empty): every tile once, or as
    one (1, 2) pair in adjacent slots of one workgroup; exactly n_split pairs.  -> the tiles that are split"""
    tile, half = np.asarray(tile), np.asarray(half)
    used = np.nonzero(tile >= 0)[0]
    assert ((half[used] >= 0) & (half[used] <= 2)).all(), f"{what}: a half other than 0, 1, 2"
    assert (tile[used] < n_tiles).all(), f"{what}: a tile beyond the image"
    whole = used[half[used] == 0]
    near = used[half[used] == 1]
    far = used[half[used] == 2]
    assert len(near) == len(far) == n_split, f"{what}: {len(near)} near and {len(far)} far halves for {n_split} split tiles"
    assert (near % 2 == 0).all() and np.array_equal(far, near + 1), f"{what}: the halves of a split tile are not an aligned pair of slots (so not in one workgroup)"
    assert np.array_equal(tile[near], tile[far]), f"{what}: a pair of halves holds two different tiles"
    seen = np.bincount(np.concatenate([tile[whole], tile[near]]), minlength=n_tiles)
    assert (seen == 1).all(), f"{what}: tiles dealt {np.unique(seen).tolist()} times; first wrong: tile {int(np.argmax(seen != 1))} ({int(seen[np.argmax(seen != 1)])} times)"
    return tile[near]
