"""What a wave of the tile ray caster does around its march, held to numpy and to the oracle on crafted fields:

  * the wave reductions of vh_device.hpp (DPP steps, one scalar result) through vh_debug_wave_reduce;
  * the tile's depth range and the table build at the list lengths where the code takes another path (0, 1, 27 | 28: the
    last list whose neighbour probes are spread over the lanes and the first that probes seven in a row; 64 | 65: the last
    complete list and the first that overflows into the general lookup), on whole and on partial tiles;
  * a wave's launch slot: no schedule, a schedule of this phase, a schedule of another phase;
  * the colour of a hit, which is the last bisection sample's alone, with bisections that fail half way;
  * a colour byte over 255 through the reciprocal (vh_debug_check_fast_math, all 256 bytes).

The fields are planes in columns or slabs of blocks, streamed into the device's table and into the oracle's."""
import ctypes as C

import numpy as np
import pytest

import mc_fields as MF
import ray_query as RQ
import tile_intervals as TI
from helpers import assert_maps_equal, bits, small_config
from voxelhashing_amd import vhtypes as T

pytestmark = pytest.mark.gpu
F = np.float32
B = T.SDF_BLOCK_SIZE
CAP_SMALL = 64


@pytest.fixture(scope="module")
def E(vh):
    from voxelhashing_amd import engine
    return engine


# ------------------------------------------------------------------------------------------------ 1. the reductions

PINF, MINF = F(np.inf).view(np.uint32), F(-np.inf).view(np.uint32)


def reduction_inputs():
    """name -> 64 words.  The float helpers read them as floats (no NaN among them), the unsigned one as they are."""
    rng = np.random.default_rng(11)
    out = {"identity of min": np.full(64, PINF, np.uint32), "identity of max": np.full(64, MINF, np.uint32), "zeros": np.zeros(64, np.uint32)}
    for lane in (0, 15, 16, 31, 32, 47, 48, 63):  # the row and half boundaries the DPP steps cross
        for name, ident, value in (("min", PINF, F(-3.25)), ("max", MINF, F(7.5)), ("u32", 0, None)):
            w = np.full(64, ident, np.uint32)
            w[lane] = value.view(np.uint32) if value is not None else 0x80000001 + lane
            out[f"one {name} value in lane {lane}"] = w
    out["64 distinct values"] = rng.permutation(np.arange(64)).astype(F) * F(0.37) - F(9.0)
    out["64 distinct values"] = out["64 distinct values"].view(np.uint32)
    mixed = np.array([0.0, -0.0, np.inf, -np.inf], F).view(np.uint32)
    out["+-0 and +-inf mixed"] = mixed[rng.integers(0, 4, 64)]
    # all four are there, so the extremes are the infinities: which of +0 and -0 numpy's min / max would return for zeros
    # alone is not specified, and a case without the infinities would hang on that
    out["+-0 and +-inf mixed"][[5, 21, 40, 63]] = mixed
    return out


@pytest.mark.parametrize("name", list(reduction_inputs()))
def test_wave_reductions_against_numpy(vh, name):
    from voxelhashing_amd import lib
    words = reduction_inputs()[name]
    d_in, d_out = lib.DeviceBuffer.from_numpy(words), lib.DeviceBuffer(4 * 192)
    lib.check(vh.vh_memset(d_out.ptr, 0xa5, 4 * 192, None))
    lib.check(vh.vh_debug_wave_reduce(d_in.ptr, d_out.ptr, None), "vh_debug_wave_reduce")
    got = d_out.download(np.uint32, 192).reshape(3, 64)
    f = words.view(F)
    want = (f.min().view(np.uint32), f.max().view(np.uint32), words.max())
    for row, w, helper in zip(got, want, ("wave_min_f32", "wave_max_f32", "wave_max_u32")):
        assert (row == row[0]).all(), f"{name}: {helper} gave the lanes {np.unique(row)}"
        assert row[0] == w, f"{name}: {helper} gave {row[0]:#x}, numpy {w:#x}"


# ------------------------------------------------------------------------------------------------ crafted fields

def plane_field(origin_block, nblocks, vs, z_plane, trunc, seed, holes=None):
    """blocks origin_block .. + nblocks with sdf = z_plane - z clipped to +-trunc, weight 1, colours independent random
    bytes per voxel; holes(ix, iy, iz voxel index arrays) -> bool: voxels whose weight is 0 -> (descs, blocks)"""
    rng = np.random.default_rng(seed)
    n = tuple(B * k for k in nblocks)
    iz = (B * origin_block[2] + np.arange(n[2])).astype(np.float64) * vs
    sdf = np.broadcast_to(np.clip(z_plane - iz, -trunc, trunc).astype(F)[None, None, :], n).copy()
    weight = np.ones(n, np.uint8)
    if holes is not None:
        gx, gy, gz = np.meshgrid(*(np.arange(k) for k in n), indexing="ij")
        weight[holes(gx, gy, gz)] = 0
    color = rng.integers(0, 256, n + (3,), dtype=np.uint8)
    return MF._to_blocks(origin_block, nblocks, sdf, weight, color)


def both_scenes(E, O, hp, cp, rp, descs, blocks):
    g, o = E.LauncherScene(hp), O.OracleScene(hp, cp, rp)
    if len(descs):
        g.stream_in(descs, blocks, T.LOCK_ENTRY)
        assert o.stream_in(descs, blocks) == 0
    return g, o


def view_of(rp, pose):
    out = type(rp)()
    C.memmove(C.byref(out), C.byref(rp), C.sizeof(rp))
    pose = np.asarray(pose, F).reshape(4, 4)
    inv = np.eye(4)
    inv[:3, :3] = pose[:3, :3].astype(np.float64).T
    inv[:3, 3] = -inv[:3, :3] @ pose[:3, 3].astype(np.float64)
    out.m_viewMatrix = T.mat16(inv.astype(F))
    out.m_viewMatrixInverse = T.mat16(pose)
    return out


def oracle_render(o, rpv, pose):
    """the oracle's four maps for the view rpv.  OracleScene.render takes the view from the pose only once the scene has
    counted its blocks (as the reference does); a streamed-in table has not, so the matrices are set here."""
    o.rp.m_viewMatrix, o.rp.m_viewMatrixInverse = rpv.m_viewMatrix, rpv.m_viewMatrixInverse
    return o.render(pose)


def eye_pose(x, y, z):
    m = np.eye(4, dtype=F)
    m[:3, 3] = (x, y, z)
    return m.reshape(16)


class Renderer:
    """splat + vh_render_intervals + vh_compute_normals (CUDARayCastSDF::render's steps: the normals from the depth map only
    without gradients, with them the march has written them) on a launcher scene -> maps, heads"""

    def __init__(self, vh, E, g, cp, rpv):
        from voxelhashing_amd import lib
        self.vh, self.lib, self.g, self.cp, self.rp = vh, lib, g, cp, rpv
        self.W, self.H = rpv.m_width, rpv.m_height
        self.n_tiles = ((self.W + 7) // 8) * ((self.H + 7) // 8)
        self.ray = E.CUDARayCastSDF(rpv)
        self.rd = self.ray.getRayCastData()
        self.heads, self.lists = lib.DeviceBuffer(self.n_tiles * 16), lib.DeviceBuffer(self.n_tiles * CAP_SMALL * 16)
        lib.check(vh.vh_ray_interval_clear(self.heads.ptr, self.W, self.H, None))

    def render(self, splat_sched=None, render_sched=None, phase=0):
        vh, lib, g = self.vh, self.lib, self.g
        for ptr, words in ((self.rd.d_depth, 1), (self.rd.d_depth4, 4), (self.rd.d_colors, 4), (self.rd.d_normals, 4)):
            lib.check(vh.vh_memset(ptr, 0, 4 * words * self.W * self.H, None))
        lib.check(vh.vh_ray_interval_splat(C.byref(g.hd), C.byref(g.hp), C.byref(self.cp), C.byref(self.rp), self.heads.ptr, self.lists.ptr, CAP_SMALL,
                                           splat_sched, phase, None, None))
        heads = self.heads.download(np.uint32).reshape(self.n_tiles, 4)
        lib.check(vh.vh_render_intervals(C.byref(g.hd), C.byref(g.hp), C.byref(self.rd), C.byref(self.cp), C.byref(self.rp), self.heads.ptr, self.lists.ptr,
                                         CAP_SMALL, render_sched, phase, None))
        if not self.rp.m_useGradients:  # (no gradients: normals from the depth map)
            lib.check(vh.vh_compute_normals(self.rd.d_normals, self.rd.d_depth4, self.W, self.H, None))
        return self.ray.download(), heads


# ------------------------------------------------------------------------------------------------ 2. list lengths

COLUMN_VS, COLUMN_TRUNC, COLUMN_FIRST = 0.005, 0.01, 25  # blocks of 4 cm along z from 1 m on, the camera looks along them


@pytest.fixture(scope="module")
def columns(E, oracle_lib):
    """n -> (device scene, oracle scene factory inputs) of a column of n blocks along z with a plane in its middle block;
    made when first asked for"""
    class Columns(dict):
        def __missing__(self, n):
            hp, _, _ = small_config(64, 48, "P4", num_buckets=1 << 10, num_sdf_blocks=256, voxel_size=COLUMN_VS, truncation=COLUMN_TRUNC, trunc_scale=0.0)
            if n:
                z_plane = (COLUMN_FIRST + n // 2 + 0.5) * B * COLUMN_VS
                descs, blocks = plane_field((0, 0, COLUMN_FIRST), (1, 1, n), COLUMN_VS, z_plane, COLUMN_TRUNC, seed=n)
            else:
                descs, blocks = np.zeros(0, T.DESC_DTYPE), np.zeros((0, T.SDF_BLOCK_VOXELS), T.VOXEL_DTYPE)
            self[n] = (hp, descs, blocks)
            return self[n]
    return Columns()


@pytest.mark.parametrize("size", [(64, 48, 35, 19), (20, 12, 17, 9)], ids=["64x48", "20x12"])
@pytest.mark.parametrize("n", [0, 1, 27, 28, 64, 65])
def test_depth_range_and_list_lengths(vh, E, oracle_lib, columns, n, size):
    """the ray of pixel (px, py) runs down the middle of the column: its tile lists the n blocks, and the pixel hits the
    plane where there is one.  20x12: the tile is a partial one on both edges."""
    W, H, px, py = size
    hp, descs, blocks = columns[n]
    cp = T.make_depth_camera_params(W, H, mx=float(px), my=float(py))
    rp = T.make_raycast_params(hp, cp)
    g, o = both_scenes(E, oracle_lib, hp, cp, rp, descs, blocks)
    pose = eye_pose(0.0213, 0.0187, 0.0)  # inside the column's 4 cm x 4 cm, off the voxel lattice
    rpv = view_of(rp, pose)
    want = oracle_render(o, rpv, pose)
    got, heads = Renderer(vh, E, g, cp, rpv).render()
    tile = (py // 8) * ((W + 7) // 8) + px // 8
    print(f"\n{n} blocks at {W}x{H}: the tile lists {heads[tile, 2]}, longest list {heads[:, 2].max()}, {int((want['depth'] != -np.inf).sum())} pixels hit")
    assert heads[tile, 2] == n, f"the tile of pixel ({px}, {py}) was meant to list {n} blocks, it lists {heads[tile, 2]}"
    assert heads[:, 2].max() == n
    if n:
        assert want["depth"][py, px] != -np.inf, "the ray down the column was meant to hit the plane"
    else:
        assert (want["depth"] == -np.inf).all()
    assert_maps_equal(got, want, f"{n} blocks at {W}x{H} against the oracle")
    g.close()
    o.close()


# ------------------------------------------------------------------------------------------------ 3. launch slots

@pytest.fixture(scope="module")
def slot_renders(vh, E, oracle_lib):
    """256x256, 1024 tiles, the smallest image whose tiles are split: the same wall rendered without a schedule, along a
    schedule made for this phase and beside one made for another phase (raster order; every wave still reads a slot).
    -> dict want, plain, fresh, stale (maps), c_fresh, c_stale (cost classes per tile), split (the tiles the fresh run split)"""
    from voxelhashing_amd import lib
    W = H = 256
    hp, cp, rp = small_config(W, H, "P4", num_buckets=1 << 11, num_sdf_blocks=1024)
    vs = float(hp.m_virtualVoxelSize)
    descs, blocks = plane_field((-7, -7, 5), (14, 14, 2), vs, 6.3 * B * vs, float(hp.m_truncation), seed=3)  # a wall around z = 2 m
    g, o = both_scenes(E, oracle_lib, hp, cp, rp, descs, blocks)
    pose = eye_pose(0.013, -0.021, 0.0)
    rpv = view_of(rp, pose)
    want = oracle_render(o, rpv, pose)
    r = Renderer(vh, E, g, cp, rpv)
    assert vh.vh_render_split_tiles(W, H) == 64
    words = vh.vh_render_schedule_bytes(W, H) // 4
    sched = lib.DeviceBuffer(4 * words)
    sched.upload(np.zeros(words, np.uint32))
    plain, _ = r.render()
    fresh, _ = r.render(splat_sched=sched.ptr, render_sched=sched.ptr, phase=1)
    after_fresh = sched.download(np.uint32)
    assert after_fresh[0] == 1
    n_launched = 4 * ((r.n_tiles + 64 + 3) // 4)
    slots = after_fresh[4 + 4 * ((r.n_tiles + 3) // 4):].reshape(-1, 2)[:n_launched]
    halves = slots[:, 0] >> 24
    assert (slots[:, 1] == 1).sum() == r.n_tiles + 64 and (halves != 0).sum() == 128, "64 tiles were meant to be split"
    split = np.unique(slots[halves != 0, 0] & 0xffffff)
    stale, _ = r.render(splat_sched=None, render_sched=sched.ptr, phase=2)  # the splat made no schedule for phase 2
    after_stale = sched.download(np.uint32)
    assert after_stale[0] == 1, "the schedule was meant to be stale"
    g.close()
    o.close()
    return dict(want=want, plain=plain, fresh=fresh, stale=stale, split=split,
                c_fresh=after_fresh[4:4 + r.n_tiles].copy(), c_stale=after_stale[4:4 + r.n_tiles].copy())


def test_launch_slots_with_no_fresh_and_stale_schedule(slot_renders):
    """the three renders are the oracle's bit for bit, and so each other's"""
    w = slot_renders
    assert (w["want"]["depth"] != -np.inf).sum() > 30000
    assert_maps_equal(w["plain"], w["want"], "no schedule against the oracle")
    assert_maps_equal(w["fresh"], w["want"], "schedule of this phase against the oracle")
    assert_maps_equal(w["stale"], w["want"], "stale schedule against the oracle")


def test_cost_classes_of_scheduled_and_stale_run_are_the_same(slot_renders):
    """the classes written to sched[4 + tile] are the same in the scheduled run, which splits 64 tiles, and in the stale
    one, which splits none: a tile's cost is its dearest ray's, a split tile's the dearest sum of a ray's two parts (the
    sample the halves share counted once, nothing behind a hit in the near half).
    The property is partial, and this wall is inside it: it holds for tiles with complete lists rendered without gradients.
    A tile whose list overflowed still pays the shared sample twice, and with gradients a split tile's cost is the sum of
    its halves' dearest rays as before (vh_ray_march.hpp and vh_ray_tiles.hpp say why); neither case is asserted here."""
    w = slot_renders
    differ = np.nonzero(w["c_fresh"] != w["c_stale"])[0]
    print(f"\ncost classes {np.unique(w['c_fresh']).tolist()}; {len(differ)} tiles differ, {int(np.isin(differ, w['split']).sum())} of them split tiles")
    assert w["c_fresh"].max() > 0 and len(np.unique(w["c_fresh"][w["split"]])) > 0
    assert np.array_equal(w["c_fresh"], w["c_stale"]), f"cost classes differ at {len(differ)} tiles, first {differ[:8]}"


# ------------------------------------------------------------------------------------------------ 4. bisection colour

def failing_iterations(m, rp, cam):
    """per ray of cam (ray_query.camera_rays): at which bisection iteration (0, 1, 2) its bisections failed -- the
    bisection restated over the oracle's trilinear sample, float32, one rounding per operation -> counts [3]"""
    f = F
    counts = np.zeros(3, np.int64)
    inc = f(rp.m_rayIncrement)
    with np.errstate(all="ignore"):
        for o, d, t0, t1 in zip(cam["origins"], cam["directions"], cam["t_min"], cam["t_max"]):
            t, last_sdf, last_alpha, last_w = f(t0), f(0), f(0), 0
            while t < t1:
                ok, dist = m.trilinear(o[0] + d[0] * t, o[1] + d[1] * t, o[2] + d[2] * t)
                dist = f(dist)
                if ok:
                    if last_w > 0 and last_sdf > 0 and dist < 0:
                        a, a_dist, b, b_dist = last_alpha, last_sdf, t, dist
                        failed = False
                        for i in range(3):
                            c = a + (a_dist / (a_dist - b_dist)) * (b - a)
                            okc, c_dist = m.trilinear(o[0] + d[0] * c, o[1] + d[1] * c, o[2] + d[2] * c)
                            c_dist = f(c_dist)
                            if not okc:
                                counts[i] += 1
                                failed = True
                                break
                            if a_dist * c_dist > 0:
                                a, a_dist = c, c_dist
                            else:
                                b, b_dist = c, c_dist
                        if not failed:
                            break  # (accepted here: the thresholds are far away)
                    last_sdf, last_alpha, last_w = dist, t, 1
                else:
                    last_w = 0
                t = t + inc
    return counts


def test_colour_of_the_last_bisection_sample(vh, E, oracle_lib):
    """a wall, seen at an angle, with independent random colours per voxel (the three bisection samples blend different bytes in every
    channel) and unobserved voxels sprinkled next to the surface, so that bisections fail at iterations 1 and 2: colours and
    hit masks of k_render and of vh_query_rays against the oracle's"""
    W, H = 64, 48
    hp, cp, rp = small_config(W, H, "P4", num_buckets=1 << 10, num_sdf_blocks=256)
    vs, trunc = float(hp.m_virtualVoxelSize), float(hp.m_truncation)
    z_plane = 6.37 * B * vs
    k_plane = z_plane / vs - 5 * B  # the plane in voxel indices of the field

    def holes(gx, gy, gz):
        rng = np.random.default_rng(5)
        return (np.abs(gz - k_plane) < 1.6) & (rng.random(gx.shape) < 0.1)

    descs, blocks = plane_field((-4, -3, 5), (8, 6, 2), vs, z_plane, trunc, seed=4, holes=holes)
    # the distance bent to a parabola through the same zero: on a linear field the first bisection sample is the root and
    # the other two sit on it, reading the same eight voxels; on this one they move by a fraction of a voxel and meet others
    s = blocks["sdf"].astype(np.float64) / trunc
    blocks["sdf"] = (trunc * np.sign(s) * s * s).astype(F)
    g, o = both_scenes(E, oracle_lib, hp, cp, rp, descs, blocks)
    pose = TI.look_pose((0.311, 0.007, 0.0), yaw=-0.15, pitch=0.05)
    rpv = view_of(rp, pose)
    want = oracle_render(o, rpv, pose)
    hit = want["depth"] != -np.inf
    cam = RQ.camera_rays(o.L, cp, rpv)
    fails = failing_iterations(RQ.Model(o.L, o.hd, o.hp), rpv, cam)
    print(f"\n{int(hit.sum())} of {W * H} pixels hit; bisections failed at iteration 0 / 1 / 2: {fails.tolist()}")
    assert hit.sum() > 500 and (~hit).sum() > 100
    assert fails[1] > 0 and fails[2] > 0, "bisections were meant to fail at iteration 1 and at iteration 2"
    got, _ = Renderer(vh, E, g, cp, rpv).render()
    assert np.array_equal(got["depth"] != -np.inf, hit), "k_render: the hit mask differs from the oracle's"
    assert np.array_equal(bits(got["colors"]), bits(want["colors"])), "k_render: colours differ from the oracle's"
    assert_maps_equal(got, want, "k_render against the oracle")
    # the colours of neighbouring samples differ: a colour taken from another bisection sample would show
    col = want["colors"][hit][:, :3]
    assert len(np.unique(bits(col), axis=0)) > 0.9 * hit.sum()
    ref = RQ.rays(o.L, o.hd, o.hp, rpv, cam["origins"], cam["directions"], cam["t_min"], cam["t_max"])
    assert np.array_equal(ref["status"].reshape(H, W) == RQ.HIT, hit), "the query's restatement and the oracle's render disagree on the hits"
    q = E.CUDARayCastSDF(rpv).castRays(g.hd, g.hp, cam["origins"], cam["directions"], cam["t_min"], cam["t_max"], normals=False)
    assert np.array_equal(q["status"], ref["status"]), "vh_query_rays: the hit mask differs from the oracle's"
    assert np.array_equal(RQ.pack_rgb(q["color"]), ref["color"]), "vh_query_rays: colours differ from the oracle's"
    assert np.array_equal(bits(q["t"]), bits(ref["t"]))
    g.close()
    o.close()


# ------------------------------------------------------------------------------------------------ 5. a byte over 255

def test_every_colour_byte_over_255(vh):
    """vh_debug_check_fast_math's first 256 operands are the bytes: c / 255 through div_exact against `/`"""
    from voxelhashing_amd import lib
    buf = lib.DeviceBuffer(8)
    lib.check(vh.vh_debug_check_fast_math(C.c_float(0.04), 1000, 256, 1, buf.ptr, None), "check")
    assert buf.download(np.uint32, 2).tolist() == [0, 0]
