"""k_interval_splat read back directly: the tile heads, the tile lists and the launch schedule, which the rest of the
suite only sees through finished maps (a list that is too wide, a tile dealt twice or a margin that is too narrow by
less than a pixel changes no map).  The heads and lists are held to tests/tile_intervals.py's float32 restatement of
the rule bit for bit and to its float64 ray/box reference as a superset; the schedule to its restatement of the deal and
to the properties every deal must have; the host's switch between the small and the large tile tables to its rule."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

import tile_intervals as TI
from helpers import assert_maps_equal, small_config
from voxelhashing_amd import canonical, synth, vhtypes as T

pytestmark = pytest.mark.gpu
PINF = 0x7f800000
CAPACITIES = (128, 64, 3, None)  # large tables, small tables, lists that nearly always overflow, no lists


@pytest.fixture(scope="module")
def E(vh):
    from voxelhashing_amd import engine
    return engine


@pytest.fixture(scope="module")
def tables(E, oracle_lib):
    """the scenes of tile_intervals.TABLES on the device: {name: dict(scene, hd, hp, blocks [n, 3], ptr [n])}; the blocks
    are the oracle's, so what tests/test_tile_intervals.py shows for the model holds for these tables"""
    out = {}
    for name in TI.TABLES:
        hp, cp, rp, opt, poses = TI.table_frames(name)
        scene = E.CUDASceneRepHashSDF(hp, opt)
        frame = E.DepthFrame(cp)
        for pose in poses:
            E.synth_frame(synth.S1_SPHERES, 0, pose, cp, out=frame)
            scene.integrate(pose, frame, cp, None)
        table = scene.download(False)["hash"]
        occ = table["ptr"] != T.FREE_ENTRY
        pos = np.ascontiguousarray(table["pos"][occ]).reshape(-1, 3).astype(np.int32)
        order = canonical.lexsort_pos(pos)
        blocks, ptr = pos[order], table["ptr"][occ][order]
        assert np.array_equal(blocks, TI.oracle_blocks(oracle_lib, name)), f"table {name}: the device and the oracle hold different blocks"
        out[name] = dict(scene=scene, hd=scene.getHashData(), hp=scene.getHashParams(), blocks=blocks, ptr=ptr,
                         index={tuple(int(v) for v in p): i for i, p in enumerate(blocks)})
    return out


@pytest.fixture(scope="module")
def truth(tables):
    """per (view, gradients), computed once and only read: the view, what its rays need (float64) and the rule (float32)"""
    out = {}
    for name, (table, *_rest) in TI.VIEWS.items():
        view = TI.View(name, tables[table]["hp"])
        for g in (False, True):
            out[name, g] = dict(view=view, need=TI.needed_for(view, tables[table]["blocks"], g), model=TI.model_for(view, tables[table]["blocks"], g))
    return out


def splat(vh, lib, tab, view, gradients, cap, sched=None, phase=0, longest=None, heads=None, lists=None):
    """vh_ray_interval_clear + vh_ray_interval_splat into test-owned buffers -> (heads [tiles, 4] u32, lists [tiles, cap, 4] i32 or None)"""
    n = view.n_tiles
    heads = heads or lib.DeviceBuffer(n * 16)
    if cap is not None and lists is None:
        lists = lib.DeviceBuffer(n * cap * 16)
        lists.upload(np.full(n * cap * 4, -77, np.int32))  # what the splat does not write must not look like an entry
    rp = view.raycast_params(tab["hp"], gradients)
    lib.check(vh.vh_ray_interval_clear(heads.ptr, view.W, view.H, None))
    lib.check(vh.vh_ray_interval_splat(C.byref(tab["hd"]), C.byref(tab["hp"]), C.byref(view.cp), C.byref(rp), heads.ptr,
                                       lists.ptr if cap is not None else None, cap or 0, sched.ptr if sched else None, phase,
                                       longest.ptr if longest else None, None))
    h = heads.download(np.uint32).reshape(n, 4)
    l = lists.download(np.int32).reshape(n, cap, 4) if cap is not None else None
    return h, l, (heads, lists, rp)


def tiles_of(mask):
    return np.nonzero(np.asarray(mask).reshape(len(mask), -1).any(axis=1))[0].tolist()


def check_lists(heads, lists, cap, tab, model, need, zlo, zhi, what):
    """one splat's heads [tiles, 4] and lists [tiles, cap, 4] (None without lists) against the rule and the rays' needs,
    every tile at once -> the kinds of tile met: none (no block), complete, overflow"""
    listed, count = model["listed"], heads[:, 2].astype(np.int64)
    n_tiles, n_blocks = listed.shape
    assert (heads[:, 3] == 0).all(), f"{what}: the fourth word of the heads of tiles {tiles_of(heads[:, 3] != 0)} is not 0"
    n_listed = np.minimum(count, cap or 0)
    got = np.zeros((n_tiles, n_blocks), np.int64)  # how often tile t lists block b
    if cap is not None:
        t, k = np.nonzero(np.arange(cap)[None, :] < n_listed[:, None])
        e = lists[t, k].astype(np.int64)
        keys = (tab["blocks"].astype(np.int64) + (1 << 15)) @ np.array([1 << 32, 1 << 16, 1], np.int64)  # (blocks are lexsorted: ascending keys)
        key = (e[:, :3] + (1 << 15)) @ np.array([1 << 32, 1 << 16, 1], np.int64)
        b = np.minimum(np.searchsorted(keys, key), n_blocks - 1)
        known = keys[b] == key
        assert known.all(), f"{what}: tiles {sorted(set(t[~known].tolist()))} list positions that are not allocated, first {e[~known][0, :3].tolist()}"
        wrong = e[:, 3] != tab["ptr"][b]
        assert not wrong.any(), f"{what}: tiles {sorted(set(t[wrong].tolist()))} list a pointer other than the hash table's, first {e[wrong][0].tolist()} against {int(tab['ptr'][b[wrong][0]])}"
        np.add.at(got, (t, b), 1)
    complete = count == n_listed
    lost = need & complete[:, None] & (got == 0)
    assert not lost.any(), f"{what}: tiles {tiles_of(lost)} need blocks (float64 ray/box test) that their complete lists do not hold: they would be read as unallocated; first: tile {np.argwhere(lost)[0][0]}, block {tab['blocks'][np.argwhere(lost)[0][1]].tolist()}"
    bad = np.nonzero(count != model["count"])[0]
    assert len(bad) == 0, f"{what}: the counts of tiles {bad.tolist()} differ from the rule's: {count[bad].tolist()} against {model['count'][bad].tolist()}"
    assert got.max(initial=0) <= 1, f"{what}: tiles {tiles_of(got > 1)} list a block twice"
    got = got.astype(bool)
    assert not (got & ~listed).any(), f"{what}: tiles {tiles_of(got & ~listed)} list blocks the rule does not give them"
    assert not (complete[:, None] & (listed != got)).any(), f"{what}: the complete lists of tiles {tiles_of(complete[:, None] & (listed != got))} are not the rule's sets"
    lost = need & ~listed
    assert not lost.any(), f"{what}: tiles {tiles_of(lost)} need blocks that the splat gave them neither a list entry nor a range for"
    # the head's range stands for exactly the blocks that are not listed (all of them without lists): {+inf, 0} if none
    rest = listed & ~got
    want = np.stack([np.where(rest, model["lo"][None, :], PINF).min(axis=1, initial=PINF), np.where(rest, model["hi"][None, :], 0).max(axis=1, initial=0)], axis=1)
    bad = np.nonzero((heads[:, :2] != want).any(axis=1))[0]
    assert len(bad) == 0, (f"{what}: the head ranges of tiles {bad.tolist()} are not the min / max over the blocks that are not listed; first "
                           f"{heads[bad[0], :2].view(np.float32)} against {want[bad[0]].astype(np.uint32).view(np.float32)}")
    h = np.ascontiguousarray(heads[:, :2]).view(np.float32).astype(np.float64)
    stood = need & rest
    outside = stood & ((h[:, :1] > zlo) | (h[:, 1:] < zhi))
    assert not outside.any(), f"{what}: the head ranges of tiles {tiles_of(outside)} do not hold the depths at which their rays need the blocks they stand for"
    return {("none", "complete", "overflow")[i] for i in np.unique(np.where(count == 0, 0, np.where(complete, 1, 2)))}


@pytest.mark.parametrize("gradients", [False, True])
@pytest.mark.parametrize("name", list(TI.VIEWS))
def test_tile_lists_and_heads(vh, tables, truth, name, gradients):
    """Counts, lists and head ranges of every tile for the four capacities, against the float32 rule; needed pairs
    (float64) are listed, and a head's range holds the depths of the needed pairs it stands for.

    Measured on an MI355X (DESIGN.md section 6 has the table): no (tile, block) pair of any view had to be excluded as a
    tie; the kernel and the restatement agree on every count, entry and range bit."""
    from voxelhashing_amd import lib
    t = truth[name, gradients]
    view, model, (need, zlo, zhi) = t["view"], t["model"], t["need"]
    tab = tables[view.table]
    print(f"\n{name} gradients={gradients}: {int(model['listed'].sum())} pairs listed by the rule, {int(need.sum())} needed, "
          f"over-coverage {model['listed'].sum() / need.sum():.2f}, longest list {int(model['count'].max())}")
    seen = {}
    for cap in CAPACITIES:
        heads, lists, _ = splat(vh, lib, tab, view, gradients, cap)
        seen[cap] = check_lists(heads, lists, cap, tab, model, need, zlo, zhi, f"{name}, gradients={gradients}, capacity {cap}")
    assert "overflow" in seen[3] and "overflow" in seen[None], f"lists of three entries were meant to overflow: {seen}"
    if name == "fine_1cm":
        for cap in (128, 64):
            assert seen[cap] == {"none", "complete", "overflow"}, f"capacity {cap}: the three count cases were meant to occur: {seen[cap]}"
    if name == "close_8cm":
        nearest = zlo[need].min()
        assert view.intrinsics()[0] * view.vs / nearest >= 8.0, "a voxel of the nearest needed block was meant to span 8 pixels"


# ------------------------------------------------------------------------------------------------ the schedule

SIZES = {300: (160, 120), 1024: (256, 256), 1073: (291, 227), 1056: (264, 256)}


@pytest.fixture(scope="module")
def num_cus():
    """the device's compute units as PyTorch reports them; asked in a fresh process, because PyTorch cannot initialise
    its HIP runtime in a process in which the library has already initialised its own"""
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    return int(out.stdout.split()[-1])


class Schedule:
    """a test-owned schedule buffer: {phase, longest list, -, -}, cost classes padded to whole quads, {tile | half << 24, phase} per slot"""

    def __init__(self, vh, lib, W, H):
        self.n_tiles = ((W + 7) // 8) * ((H + 7) // 8)
        self.words = vh.vh_render_schedule_bytes(W, H) // 4
        self.first_slot = 4 + 4 * ((self.n_tiles + 3) // 4)
        self.buf = lib.DeviceBuffer(4 * self.words)
        self.host = np.zeros(self.words, np.uint32)
        self.buf.upload(self.host)
        self.n_split = vh.vh_render_split_tiles(W, H)
        self.n_launched = 4 * ((self.n_tiles + self.n_split + 3) // 4)

    def set_classes(self, classes):
        """as k_render leaves them; the padding of the last quad is filled with the dearest class, which no tile has"""
        self.host = self.buf.download(np.uint32)
        self.host[4:self.first_slot] = 31
        self.host[4:4 + self.n_tiles] = classes
        self.buf.upload(self.host)

    def read(self):
        self.host = self.buf.download(np.uint32)
        slots = self.host[self.first_slot:].reshape(-1, 2)
        return self.host[:4], slots[:, 0] & 0xffffff, slots[:, 0] >> 24, slots[:, 1]


def check_schedule(s, classes, phase, num_cus, what):
    head, tile, half, stamp = s.read()
    assert head[0] == phase, f"{what}: the schedule says phase {head[0]}"
    assert (stamp[s.n_launched:] != phase).all(), f"{what}: a slot beyond the {s.n_launched} launched ones was written"
    accepted = stamp[:s.n_launched] == phase  # what k_render takes; every other slot is an empty one to it
    dealt = np.where(accepted, tile[:s.n_launched].astype(np.int64), -1)
    halves = np.where(accepted, half[:s.n_launched].astype(np.int64), 0)
    TI.check_deal(dealt, halves, s.n_tiles, s.n_split, what)
    model = TI.schedule_model(classes, s.n_tiles, num_cus, s.n_split)
    assert np.array_equal(accepted, model["cls"] >= 0), f"{what}: other slots are filled than the rule fills: {np.nonzero(accepted != (model['cls'] >= 0))[0][:8]}"
    got = np.where(accepted, np.minimum(classes, 31)[np.maximum(dealt, 0)].astype(np.int64), -1)
    bad = np.nonzero(got != model["cls"])[0]
    assert len(bad) == 0, f"{what}: {len(bad)} slots hold a tile of another cost class than the rule deals, first: slot {bad[0]} holds class {got[bad[0]]}, the rule {model['cls'][bad[0]]}"
    assert np.array_equal(halves, model["half"]), f"{what}: the halves differ from the rule's"
    assert np.array_equal(TI.share_of(dealt[accepted], s.n_tiles), model["share"][accepted]), f"{what}: a slot holds a tile of another share than the rule deals"


@pytest.mark.parametrize("n_tiles", list(SIZES))
def test_schedule_deal(vh, E, num_cus, n_tiles):
    """phase 1 with crafted cost classes, then phase 2 with others, on an empty table (no render is needed)"""
    from voxelhashing_amd import lib
    W, H = SIZES[n_tiles]
    hp, cp, rp = small_config(W, H, "P4", num_buckets=1 << 10, num_sdf_blocks=1 << 8)
    scene = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=True, gc=False))
    hd, hpp = scene.getHashData(), scene.getHashParams()
    s = Schedule(vh, lib, W, H)
    assert s.n_tiles == n_tiles and s.n_split == TI.split_tiles(n_tiles) == vh.vh_render_split_tiles(W, H)
    heads = lib.DeviceBuffer(n_tiles * 16)
    lib.check(vh.vh_ray_interval_clear(heads.ptr, W, H, None))
    patterns = TI.class_patterns(n_tiles, n_tiles)
    phase = 0
    for pattern, classes in patterns.items():
        phase += 1
        s.set_classes(classes)
        lib.check(vh.vh_ray_interval_splat(C.byref(hd), C.byref(hpp), C.byref(cp), C.byref(rp), heads.ptr, None, 0, s.buf.ptr, phase, None, None))
        check_schedule(s, classes, phase, num_cus, f"{n_tiles} tiles, phase {phase} ({pattern}), {num_cus} CUs")
        # Nothing of an earlier phase is left where this phase's k_render would look for a tile.  k_render takes a slot only
        # if its stamp is the current phase, so any other stamp would do; this asks for more, that every launched slot is
        # either rewritten or still 0, which holds because schedule_tiles rewrites every slot it fills in every phase and
        # never touches the padding slots of the last workgroup.  A change that pre-stamps the padding is no defect:
        # relax this line then, not the deal.
        _, _, _, stamp = s.read()
        stale = (stamp[:s.n_launched] != phase) & (stamp[:s.n_launched] != 0)
        assert not stale.any(), f"phase {phase}: slots {np.nonzero(stale)[0][:8]} still carry an earlier phase"
    assert (heads.download(np.uint32).reshape(n_tiles, 4) == np.array([PINF, 0, 0, 0], np.uint32)).all(), "an empty table gives no tile a block"


@pytest.mark.parametrize("name,expect", [("fine_1cm", "long"), ("orbit_2cm", "long"), ("close_8cm", "short")])
def test_longest_list_feedback(vh, E, tables, truth, name, expect):
    """splat(1) -> render(1) -> splat(2): the second splat publishes the longest list render 1 met, if it came within 16
    of the small capacity, and render 1 leaves a cost class of at most 31 for every tile"""
    from voxelhashing_amd import lib
    view = truth[name, False]["view"]
    tab = tables[view.table]
    s = Schedule(vh, lib, view.W, view.H)
    word = lib.DeviceBuffer(4)
    word.upload(np.array([0xdead], np.uint32))
    heads, lists, (d_heads, d_lists, rp) = splat(vh, lib, tab, view, False, TI.CAP_SMALL, sched=s.buf, phase=1, longest=word)
    assert word.download(np.uint32)[0] == 0, "no render has reported yet"
    counts = heads[:, 2]
    ray = E.CUDARayCastSDF(rp)
    rd = ray.getRayCastData()
    lib.check(vh.vh_render_intervals(C.byref(tab["hd"]), C.byref(tab["hp"]), C.byref(rd), C.byref(view.cp), C.byref(rp), d_heads.ptr, d_lists.ptr,
                                     TI.CAP_SMALL, s.buf.ptr, 1, None))
    maps = ray.download()
    assert (maps["depth"] != -np.inf).sum() > 50
    head, *_ = s.read()
    want = int(counts.max()) if counts.max() > TI.CAP_SMALL - 16 else 0
    assert (want != 0) == (expect == "long")
    assert head[1] == want, f"render 1 met lists of up to {counts.max()} blocks and left {head[1]} in the schedule"
    assert (s.host[4:4 + view.n_tiles] <= 31).all(), "a stored cost class beyond the last one"
    assert (d_heads.download(np.uint32).reshape(-1, 4) == np.array([PINF, 0, 0, 0], np.uint32)).all(), "the render re-arms the heads"
    splat(vh, lib, tab, view, False, TI.CAP_SMALL, sched=s.buf, phase=2, longest=word, heads=d_heads, lists=d_lists)
    assert word.download(np.uint32)[0] == want
    head, *_ = s.read()
    assert head[0] == 2 and head[1] == 0, "the word starts again for render 2"


def test_scheduled_render_with_a_short_last_quad(vh, E, tables, num_cus):
    """291x227 (1073 tiles: 66 split tiles, a last quad of one tile): renders along a schedule, the second one in the
    order and the halves render 1's costs give, against the same view without a schedule (raster order)"""
    from voxelhashing_amd import lib
    W, H = SIZES[1073]
    tab = tables["P4"]
    view = TI.View("wide_4cm", tab["hp"], ("P4", W, H, synth.orbit_pose(1, 40)))
    rp = view.raycast_params(tab["hp"], False)
    ray = E.CUDARayCastSDF(rp)
    rd = ray.getRayCastData()
    s = Schedule(vh, lib, W, H)
    assert s.n_split == 66
    heads, lists = lib.DeviceBuffer(view.n_tiles * 16), lib.DeviceBuffer(view.n_tiles * TI.CAP_SMALL * 16)
    lib.check(vh.vh_ray_interval_clear(heads.ptr, W, H, None))

    def render(sched, phase):
        for ptr, words in ((rd.d_depth, 1), (rd.d_depth4, 4), (rd.d_colors, 4), (rd.d_normals, 4)):
            lib.check(vh.vh_memset(ptr, 0, 4 * words * W * H, None))
        lib.check(vh.vh_ray_interval_splat(C.byref(tab["hd"]), C.byref(tab["hp"]), C.byref(view.cp), C.byref(rp), heads.ptr, lists.ptr, TI.CAP_SMALL,
                                           sched, phase, None, None))
        lib.check(vh.vh_render_intervals(C.byref(tab["hd"]), C.byref(tab["hp"]), C.byref(rd), C.byref(view.cp), C.byref(rp), heads.ptr, lists.ptr,
                                         TI.CAP_SMALL, sched, phase, None))
        return ray.download()

    want = render(None, 0)
    assert (want["depth"] != -np.inf).sum() > 10000
    assert_maps_equal(render(s.buf.ptr, 1), want, "scheduled render 1 (every class 0)")
    classes = s.buf.download(np.uint32)[4:4 + view.n_tiles].copy()
    assert classes.max() <= 31 and len(np.unique(classes)) > 1, "render 1 was meant to leave more than one cost class"
    assert_maps_equal(render(s.buf.ptr, 2), want, "scheduled render 2 (in the order of render 1's costs, 66 tiles split)")
    # (render 2 has rewritten the classes; the deal it ran on was made from render 1's)
    _, tile, half, stamp = s.read()
    accepted = stamp[:s.n_launched] == 2
    TI.check_deal(np.where(accepted, tile[:s.n_launched].astype(np.int64), -1), np.where(accepted, half[:s.n_launched].astype(np.int64), 0), view.n_tiles, 66, "the deal of render 2")
    model = TI.schedule_model(classes, view.n_tiles, num_cus, 66)
    assert np.array_equal(np.where(accepted, classes[np.minimum(tile[:s.n_launched], view.n_tiles - 1)].astype(np.int64), -1), model["cls"])


# ------------------------------------------------------------------------------------------------ the host's choice of tables

def capacity_rule(longest_per_render):
    """vh_host.cpp: render k reads the word render k - 2 left (a render's longest list, if above 48, is published by the
    next render's splat and has arrived once that render is synchronised); large tables as soon as the word exceeds 64,
    small ones again after more than 30 renders in a row that read no such word"""
    large, quiet, out = False, 0, []
    for k in range(len(longest_per_render)):
        word = 0 if k < 2 else (longest_per_render[k - 2] if longest_per_render[k - 2] > TI.CAP_SMALL - 16 else 0)
        if word > TI.CAP_SMALL:
            large, quiet = True, 0
        elif large:
            quiet += 1
            if quiet > 30:
                large = False
        out.append(TI.CAP_LARGE if large else TI.CAP_SMALL)
    return out


def test_tile_capacity_follows_the_longest_list(E, tables, truth):
    """CUDARayCastSDF::render over the fine-voxel scene: 128 from the second render after a list outgrew 64, back to
    64 after more than 30 renders without one; every render is synchronised, so the frames are exact"""
    t = truth["fine_1cm", False]
    view, longest = t["view"], int(t["model"]["count"].max())
    assert longest > 2 * TI.CAP_SMALL
    tab = tables[view.table]
    away = TI.look_pose(view.pose.reshape(4, 4)[:3, 3], yaw=np.pi)  # every block behind the camera: no list at all
    ray = E.CUDARayCastSDF(view.raycast_params(tab["hp"], False))
    assert ray.getTileCapacity() == TI.CAP_SMALL
    sequence = [(view.pose, longest)] * 4 + [(away, 0)] * 34 + [(view.pose, longest)] * 3
    got = []
    for pose, _ in sequence:
        ray.render(tab["hd"], tab["hp"], view.cp, pose)
        maps = ray.download()  # synchronises the stream: the mapped word has arrived
        got.append(ray.getTileCapacity())
        assert ((maps["depth"] != -np.inf).sum() > 50) == (pose is view.pose)
    want = [64, 64] + [128] * 34 + [64, 64] + [64, 64, 128]
    assert capacity_rule([n for _, n in sequence]) == want
    assert got == want, f"capacities per render: {got}"
