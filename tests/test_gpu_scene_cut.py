"""Scene cut on the device (vh_cut.hip) against the numpy restatement of its definition (tests/scene_cut.py): boxes whose
faces pass through lattice points, rotated boxes and ellipsoids, inside and outside, erased, lifted and copied out; the
region that holds everything and the one that holds nothing; the crowded-table sequences A and B (tests/crowded.py),
where freed blocks sit on collision lists; a crafted block list; count only; a staging pool one block short;
moveRegionTo; a ray cast and an integrate after a cut; the refusals and Reconstruction's methods.  Every downloaded
state goes through state(), which checks the invariants (a free block is all zero among them), follows every list and
compares the bucket summary."""

import numpy as np
import pytest

import crowded as CR
import scene_cut as SC
import scene_merge as SM
from helpers import assert_maps_equal, small_config
from voxelhashing_amd import canonical, synth, vhtypes as T

pytestmark = pytest.mark.gpu
V = T.SDF_BLOCK_VOXELS
POOL = 1 << 11
LIFT, KEEP, OUTSIDE, COUNT_ONLY = T.CUT_LIFT, T.CUT_KEEP, T.CUT_SELECT_OUTSIDE, T.CUT_COUNT_ONLY


@pytest.fixture(scope="module")
def E(vh):
    from voxelhashing_amd import engine
    return engine


def config(pool=POOL):
    return small_config(64, 48, "P4", num_sdf_blocks=pool)


def options():
    return T.make_scene_options(offline=True, gc=False)


def fused_scene(E, frames=range(3), pool=POOL):
    """S1 at 64x48, the given frames of the orbit fused through CUDASceneRepHashSDF"""
    hp, cp, _ = config(pool)
    scene = E.CUDASceneRepHashSDF(hp, options())
    frame = E.DepthFrame(cp)
    for k in frames:
        pose = synth.orbit_pose(k, 40)
        E.synth_frame(synth.S1_SPHERES, 0, pose, cp, out=frame)
        scene.integrate(pose, frame, cp, None)
    return scene


@pytest.fixture(scope="module")
def base(E):
    """The scene every launcher-level test starts from, as (positions, voxels), with the regions cut out of it: computed
    once, only read."""
    snap = fused_scene(E).state()
    pos, vox = snap["positions"], snap["voxels"]
    assert 100 < len(pos) < POOL // 2
    hp = config()[0]
    vs = np.float32(hp.m_virtualVoxelSize)
    coords = SC.voxel_coords(pos)[vox["weight"] > 0]
    centre = np.round(np.median(coords, axis=0)).astype(np.int64)
    c_world = centre.astype(np.float64) * np.float64(vs)
    regions = {
        # half extents of 16, 8 and 16 voxels about a lattice point: m_rr = 1 / 16, 1 / 8, exactly
        "lattice box": (E.cut_region_transform(SC.frame(None, c_world), (16 * vs, 8 * vs, 16 * vs), vs), T.CUT_BOX),
        "rotated box": (E.cut_region_transform(SC.frame(SC.rotation([(0, 0.5), (1, -0.8)]), c_world + (0.03, -0.02, 0.05)), (0.7, 0.4, 0.55), vs), T.CUT_BOX),
        "ellipsoid": (E.cut_region_transform(SC.frame(SC.rotation([(2, 0.4)]), c_world + (0.01, 0.02, -0.03)), (0.8, 0.5, 0.7), vs), T.CUT_ELLIPSOID),
    }
    return dict(scene=(pos, vox), regions=regions, centre=centre, c_world=c_world, vs=vs)


def launcher(E, scene, hp=None):
    """a LauncherScene that holds the scene (streamed in as a block list)"""
    hp = hp or config()[0]
    g = E.LauncherScene(hp)
    descs = np.zeros(len(scene[0]), T.DESC_DTYPE)
    descs["pos"] = scene[0]
    g.stream_in(descs, scene[1], 1)
    return g


def raw_equal(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a if k != "params")


def assert_is(snap, want, what):
    """a device snapshot holds the restatement's scene"""
    assert np.array_equal(snap["positions"], want["positions"]), f"{what}: block position sets differ"
    assert snap["voxels"].tobytes() == want["voxels"].tobytes(), f"{what}: voxel bytes differ"


def assert_list_is(descs, voxels, want, what):
    """a lifted list holds the restatement's blocks, as a set of {pos, 512 voxels}"""
    assert len(descs) == len(np.unique(descs["pos"].reshape(-1, 3), axis=0)) == len(want[0]), f"{what}: {len(descs)} lifted blocks, {len(want[0])} wanted"
    assert sorted(int(p) for p in descs["ptr"]) == [V * k for k in range(len(descs))], f"{what}: the list's ptrs are not the staging slots"
    got = SM.sort_scene(descs["pos"].reshape(-1, 3), voxels)
    assert np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes(), f"{what}: the lifted blocks differ"


def check_cut(E, scene, m, shape, flags, what, hp=None):
    """one vh_cut_blocks on a table that holds `scene`, everything against the restatement -> (counts, restatement)"""
    hp = hp or config()[0]
    want = SC.cut(scene, m, shape, flags)
    g = launcher(E, scene, hp)
    before = g.download()
    got = g.cut_blocks(m, shape, flags, 2)
    print(what, {k: got[k] for k in T.CUT_COUNTS})
    assert got["code"] == 0
    SC.assert_counts(got, want["counts"], what)
    assert got["unsettled"] == 0 and got["delete_passes"] <= got["freed"] + 8
    assert (got["delete_passes"] == 0) == (got["freed"] == 0)
    if flags & (KEEP | COUNT_ONLY):
        assert raw_equal(before, g.download()), f"{what}: a call that keeps or only counts wrote to the table"
    after = g.state()
    assert_is(after, want, what)
    assert after["heap_free"] == hp.m_numSDFBlocks - len(want["positions"])
    assert_list_is(got["descs"], got["voxels"], want["lifted"], what)
    return got, want


# ------------------------------------------------------------------------------------------------ 1. regions x modes

@pytest.mark.parametrize("outside", [0, OUTSIDE], ids=["inside", "outside"])
@pytest.mark.parametrize("name", ["lattice box", "rotated box", "ellipsoid"])
def test_regions_erased_lifted_and_copied_out(E, base, name, outside):
    m, shape = base["regions"][name]
    pos, vox = base["scene"]
    if name == "lattice box":
        # the faces pass through voxels: |u| == 1 occurs on an observed voxel, and such a voxel is inside
        u = SC.region_u(m, pos)
        on_face = (np.abs(u) == np.float32(1)).any(axis=-1) & (vox["weight"] > 0)
        assert on_face.any(), "no observed voxel lies on a face of the box"
        assert (on_face & SC.inside(m, shape, pos)).any(), "no observed voxel on a face is inside"
        assert np.array_equal(m[:, :3], np.diag(np.array([1 / 16, 1 / 8, 1 / 16], np.float32)))
    for flags in (0, LIFT, LIFT | KEEP):
        got, want = check_cut(E, base["scene"], m, shape, flags | outside, f"{name}, flags {flags | outside}")
        c = want["counts"]
        assert 0 < c["touched"] <= c["blocks_in"] and c["voxels_erased"] + c["voxels_lifted"] > 0
        if not flags & KEEP:
            assert 0 < c["freed"] < c["blocks_in"], "the region was meant to free some blocks and keep others"
            assert c["freed"] < c["touched"], "the region was meant to cut through blocks"
        if flags & LIFT:
            assert 0 < c["lifted"]


# ------------------------------------------------------------------------------------------------ 2. everything, nothing

def test_everything_and_nothing(E, base):
    hp = config()[0]
    everything = np.zeros((3, 4), np.float32)              # u = 0: inside
    nothing = np.zeros((3, 4), np.float32)
    nothing[:, 3] = 2.0                                    # u = 2: outside
    n = len(base["scene"][0])
    got, _ = check_cut(E, base["scene"], everything, T.CUT_BOX, 0, "everything")
    assert (got["touched"], got["freed"]) == (n, n)
    g = launcher(E, base["scene"], hp)
    g.cut_blocks(everything, T.CUT_ELLIPSOID, 0, 2)
    d = g.download()
    assert not (d["hash"]["ptr"] != T.FREE_ENTRY).any() and not d["bucket_count"].any() and not d["bucket_bits"].any()
    assert d["heap_counter"] == hp.m_numSDFBlocks - 1
    assert np.array_equal(np.sort(d["heap"]), np.arange(hp.m_numSDFBlocks, dtype=np.uint32)), "the heap is not a permutation of all block ids"
    assert not d["sdf_blocks"].view(np.uint64).any()
    # nothing: every array as it was, for every mode
    for flags in (0, LIFT, LIFT | KEEP, OUTSIDE | COUNT_ONLY):
        m = everything if flags & OUTSIDE else nothing
        g = launcher(E, base["scene"], hp)
        before = g.download()
        got = g.cut_blocks(m, T.CUT_BOX, flags, 2)
        assert got["code"] == 0 and got["blocks_in"] == n
        assert [got[k] for k in T.CUT_COUNTS[1:]] == [0] * (len(T.CUT_COUNTS) - 1), got
        assert raw_equal(before, g.download()), f"flags {flags}: a region that selects nothing changed the table"
    # the host class: a box far larger than the scene, and what vh_scene_rep_debug_hash says afterwards
    scene = fused_scene(E)
    occupied = scene.state()["num_occupied"]
    got = scene.eraseRegion(T.make_cut_region(base["c_world"], (1000.0, 1000.0, 1000.0)))
    assert (got["touched"], got["freed"], got["status"], got["unsettled"]) == (occupied, occupied, 0, 0)
    rep = scene.debugHash()
    assert (rep["numOccupied"], rep["duplicates"], rep["lockEntries"]) == (0, 0, 0)
    assert scene.state()["num_occupied"] == 0
    # n = 0: the empty table launches nothing and reports zeros
    got = scene.eraseRegion(T.make_cut_region(base["c_world"], (1.0, 1.0, 1.0)))
    assert all(got[k] == 0 for k in T.CUT_COUNTS)


# ------------------------------------------------------------------------------------------------ 3. crowded tables

def crowded_scene(E, name, buckets=None):
    hp, cp, _ = CR.config(name, buckets)
    scene = E.CUDASceneRepHashSDF(hp, CR.options())
    frame = E.DepthFrame(cp)
    for pose in CR.poses(name):
        E.synth_frame(synth.S1_SPHERES, 0, pose, cp, out=frame)
        scene.integrate(pose, frame, cp, None)
    return scene


def list_head_middle_tail(table, hp, freed):
    """a bucket whose list's head (the bucket's last slot, carrying an offset), a middle element and tail are all freed"""
    freed = CR.position_set(freed)
    for b, slots in sorted(CR.lists_of(table, hp).items()):
        chain = [b * T.HASH_BUCKET_SIZE + T.HASH_BUCKET_SIZE - 1] + [int(s) for s in slots]
        if len(chain) < 3 or table["offset"][chain[0]] == 0 or table["ptr"][chain[0]] == T.FREE_ENTRY:
            continue
        is_freed = [tuple(int(v) for v in table["pos"][s]) in freed for s in chain]
        if is_freed[0] and is_freed[-1] and any(is_freed[1:-1]):
            return b
    return None


def half_spaces(snap, vs):
    """boxes that hold about a half, a quarter or three quarters of the scene: one face through it, the others far away"""
    coords = SC.voxel_coords(snap["positions"])[snap["voxels"]["weight"] > 0].astype(np.float64) * float(vs)
    mid = np.median(coords, axis=0)
    for q in (50, 25, 75):
        for axis in range(3):
            for side in (1.0, -1.0):
                centre = mid.copy()
                centre[axis] = np.percentile(coords[:, axis], q) + side * 50.0
                yield T.make_cut_region(centre, (50.0, 50.0, 50.0)), (q, axis, side)


@pytest.mark.parametrize("name", ["A", "B"])
def test_crowded_tables(E, name):
    s = CR.SCENARIOS[name]
    hp = CR.config(name)[0]
    vs = np.float32(hp.m_virtualVoxelSize)
    everything = T.make_cut_region((0.0, 0.0, 0.0), (1000.0, 1000.0, 1000.0))
    # the half space is chosen on the crowded table as it is before the cut: one that frees a whole stretch of a list
    probe = crowded_scene(E, name)
    table, snap = probe.download()["hash"], probe.state()
    assert canonical.check_chains(table, hp)["listed"] >= 3
    scene0 = SM.scene_of(snap)
    half = None
    for region, which in half_spaces(snap, vs):
        m = E.cut_region_transform(list(region.worldFromRegion), list(region.halfExtents), vs)
        want = SC.cut(scene0, m, T.CUT_BOX, 0)
        if 0 < len(want["freed"]) < len(scene0[0]) and list_head_middle_tail(table, hp, want["freed"]) is not None:
            half = (region, m, which)
            break
    assert half is not None, "no half space frees the head, a middle element and the tail of one list"
    print(name, "half space", half[2])
    m_all = E.cut_region_transform(list(everything.worldFromRegion), list(everything.halfExtents), vs)
    for what, region, m in (("everything", everything, m_all), ("half space", half[0], half[1])):
        results = {}
        for buckets in (s["buckets"], CR.ROOMY):
            label = f"{name}, {what}, {buckets} buckets"
            scene = crowded_scene(E, name, buckets)
            before, table = scene.state(), scene.download()["hash"]
            want = SC.cut(SM.scene_of(before), m, T.CUT_BOX, 0)
            if buckets != CR.ROOMY:
                # asserted on the table before the cut: the delete passes are exercised
                assert list_head_middle_tail(table, scene.getHashParams(), want["freed"]) is not None, label
                assert CR.list_involved(table, scene.getHashParams()).sum() >= 3
            got = scene.eraseRegion(region)
            print(label, got)
            SC.assert_counts(got, want["counts"], label)
            assert got["unsettled"] == 0 and got["status"] == 0
            assert got["delete_passes"] <= got["freed"] + 8
            if buckets != CR.ROOMY:
                assert got["delete_passes"] >= 3, "three deletes of one list take its bucket's mutex in three passes"
            after = scene.state()
            assert_is(after, want, label)
            assert after["heap_free"] == scene.getHashParams().m_numSDFBlocks - len(want["positions"])
            assert scene.debugHash()["duplicates"] == 0 and scene.getState()[T.STATE_HEAP_UNDERFLOW] == 0
            results[buckets] = after
        assert_is(results[s["buckets"]], results[CR.ROOMY], f"{name}, {what}: crowded vs roomy")


# ------------------------------------------------------------------------------------------------ 4. a crafted list

def crafted(m, shape, flags, base_block):
    """four blocks, three of them around a corner of base_block + 1 that the region's centre lies on: A keeps observed voxels
    and holds one selected voxel of weight 0 with sdf bits; B's only observed voxels are selected; C is B with one
    unselected observed voxel; D, far away, is full: untouched by the box, all selected by its complement"""
    rng = np.random.default_rng(11)
    pos = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [40, 0, 0]], np.int64) + np.asarray(base_block, np.int64)).astype(np.int32)
    sel = SC.selected(m, shape, flags, pos)
    vox = np.zeros((len(pos), V), T.VOXEL_DTYPE)
    full = np.zeros((len(pos), V), T.VOXEL_DTYPE)
    full["sdf"] = rng.uniform(-0.1, 0.1, full.shape).astype(np.float32)
    full["color"] = rng.integers(0, 256, full.shape + (3,), dtype=np.uint8)
    full["weight"] = rng.integers(1, 200, full.shape).astype(np.uint8)
    for k in range(3):
        assert sel[k].any() and not sel[k].all(), "A, B and C were meant to straddle a face"
    assert sel[3].all() if flags & OUTSIDE else not sel[3].any(), "D was meant to lie wholly outside the box"
    a_sel = np.nonzero(sel[0])[0][0]
    vox[0][~sel[0]] = full[0][~sel[0]]
    vox[0]["sdf"][a_sel] = np.float32(1.5)              # weight 0, sdf bits != 0
    vox[1][sel[1]] = full[1][sel[1]]
    vox[2][sel[2]] = full[2][sel[2]]
    c_keep = np.nonzero(~sel[2])[0][-1]
    vox[2][c_keep] = full[2][c_keep]
    vox[3] = full[3]
    return pos, vox, sel


@pytest.mark.parametrize("outside", [0, OUTSIDE], ids=["inside", "outside"])
def test_crafted_block_list(E, outside):
    hp = config()[0]
    # voxel coordinates near 2^19, a matrix that is no power of two: the products round
    base_block = (1 << 16, 1 << 16, 1 << 16)
    c = np.array([(1 << 19) + 8, (1 << 19) + 8, (1 << 19) + 8], np.float64)
    a = np.array([0.16, 0.19, 0.23], np.float32)
    m = np.zeros((3, 4), np.float32)
    m[:, :3] = np.diag(a)
    m[:, 3] = (-(a.astype(np.float64) * c)).astype(np.float32)
    pos, vox, sel = crafted(m, T.CUT_BOX, outside, base_block)
    u = SC.region_u(m, pos)
    exact = np.float64(m[0, 0]) * SC.voxel_coords(pos)[..., 0].astype(np.float64)
    assert (exact.astype(np.float32).astype(np.float64) != exact).any(), "no product rounds"
    assert np.isfinite(u).all()
    # the list form: counts and the lifted list
    want = SC.cut((pos, vox), m, T.CUT_BOX, outside | LIFT | KEEP)
    descs = np.zeros(len(pos), T.DESC_DTYPE)
    descs["pos"], descs["ptr"] = pos, -7  # (the ptr of a list's desc is not read)
    g = E.LauncherScene(hp)
    before = g.download()
    got = g.cut_blocks(m, T.CUT_BOX, outside | LIFT | KEEP, 2, descs=descs, blocks=vox)
    print({k: got[k] for k in T.CUT_COUNTS})
    assert got["code"] == 0
    SC.assert_counts(got, want["counts"], "crafted list")
    assert_list_is(got["descs"], got["voxels"], want["lifted"], "crafted list")
    assert raw_equal(before, g.download())
    lifted = CR.position_set(want["lifted"][0])
    touched = sel.any(axis=1)
    assert touched[0] and tuple(int(v) for v in pos[0]) not in lifted, "A: touched, not lifted"
    assert tuple(int(v) for v in pos[1]) in lifted and tuple(int(v) for v in pos[2]) in lifted
    assert got["touched"] == int(touched.sum()) and touched[3] == bool(outside)
    assert E.extract_from_block_list(descs, vox, m, T.CUT_BOX, bool(outside))["lifted"] == got["lifted"]
    # a list is only copied from: without VH_CUT_KEEP the call is refused
    assert g.cut_blocks(m, T.CUT_BOX, outside, 2, descs=descs, blocks=vox)["code"] == 4
    assert g.cut_blocks(m, T.CUT_BOX, outside | KEEP, 2, descs=descs, blocks=vox)["code"] == 4
    # the erase form on a table that holds the same blocks
    got, want = check_cut(E, (pos, vox), m, T.CUT_BOX, outside, "crafted blocks on a table")
    freed = CR.position_set(want["freed"])
    left = CR.voxels_by_position(dict(positions=want["positions"], voxels=want["voxels"]))
    pa, pb, pc, pd = (tuple(int(v) for v in p) for p in pos[:4])
    assert pa in left and pb in freed and pc in left and (pd in freed if outside else pd in left)
    a_after = np.frombuffer(left[pa], T.VOXEL_DTYPE)
    assert not a_after[sel[0]].view(np.uint64).any() and a_after[~sel[0]].tobytes() == vox[0][~sel[0]].tobytes(), "A: its selected voxel is zeroed"
    assert outside or left[pd] == vox[3].tobytes()


def test_rows_that_overflow(E):
    """m_x0 = -m_x1 so large that the products of some voxels overflow: +inf + -inf is a NaN, which is not inside.  On the
    diagonal i == j of the others u_x is 0."""
    hp = config()[0]
    big = np.float32(3.4028234e38 / ((1 << 19) + 3.5))
    m = np.zeros((3, 4), np.float32)
    m[0, 0], m[0, 1] = big, -big
    pos = np.array([[1 << 16, 1 << 16, 0], [1 << 16, (1 << 16) + 1, 0], [(1 << 16) - 1, (1 << 16) - 1, 0]], np.int32)
    u = SC.region_u(m, pos)
    ins = SC.inside(m, T.CUT_BOX, pos)
    assert np.isnan(u[..., 0]).any() and np.isinf(u[..., 0]).any() and (u[..., 0] == 0).any()
    assert ins[0].any() and not ins[0].all() and not ins[1].any() and ins[2].any()
    coords = SC.voxel_coords(pos)
    diag = coords[..., 0] == coords[..., 1]
    assert (np.isnan(u[..., 0]) & diag).any() and np.array_equal(ins, diag & ~np.isnan(u[..., 0]))
    rng = np.random.default_rng(12)
    vox = np.zeros((len(pos), V), T.VOXEL_DTYPE)
    vox["sdf"] = rng.uniform(-0.1, 0.1, vox.shape).astype(np.float32)
    vox["weight"] = rng.integers(0, 3, vox.shape).astype(np.uint8)
    for outside in (0, OUTSIDE):
        for flags in (0, LIFT):
            check_cut(E, (pos, vox), m, T.CUT_BOX, flags | outside, f"overflowing rows, flags {flags | outside}")


# ------------------------------------------------------------------------------------------------ 5. count only, 6. staging short

def test_count_only_writes_nothing_and_counts_the_same(E, base):
    for name, (m, shape) in base["regions"].items():
        for flags in (0, LIFT, LIFT | KEEP, OUTSIDE, OUTSIDE | LIFT):
            g = launcher(E, base["scene"])
            before = g.download()
            counted = g.cut_blocks(m, shape, flags | COUNT_ONLY, 2)
            assert counted["code"] == 0 and raw_equal(before, g.download()), f"{name}, flags {flags}: counting wrote to the table"
            done = g.cut_blocks(m, shape, flags, 3)
            SC.assert_counts(counted, {k: done[k] for k in SC.COUNT_KEYS}, f"{name}, flags {flags}: count vs do")
            assert counted["delete_passes"] == 0


@pytest.mark.parametrize("flags", [LIFT, LIFT | KEEP, LIFT | OUTSIDE])
def test_staging_one_block_short_changes_nothing(E, base, flags):
    m, shape = base["regions"]["rotated box"]
    want = SC.cut(base["scene"], m, shape, flags)
    need = want["counts"]["lifted"]
    assert need > 1
    g = launcher(E, base["scene"])
    before = g.download()
    got = g.cut_blocks(m, shape, flags, 2, staging_blocks=need - 1, poison=0xA5)
    print({k: got[k] for k in T.CUT_COUNTS})
    assert got["code"] == 4 and got["status"] == T.CUT_STAGING_SHORT  # VH_ERR_BAD_ARGUMENT
    assert got["lifted"] == need and got["delete_passes"] == 0
    assert raw_equal(before, g.download()), "a refused cut changed the table"
    for raw in got["staging_raw"]:
        assert (raw == 0xA5).all(), "a refused cut wrote to the staging pool or its list"
    g.state()
    # one block more is enough, and a pool larger than needed is written only where blocks are listed
    got = g.cut_blocks(m, shape, flags, 3, staging_blocks=need + 2, poison=0xA5)
    assert got["code"] == 0 and got["status"] == 0
    assert_list_is(got["descs"], got["voxels"], want["lifted"], "a pool with room to spare")
    assert (got["staging_raw"][1][need * V * 8:] == 0xA5).all() and (got["staging_raw"][0][need * 16:] == 0xA5).all()
    assert_is(g.state(), want, "after the refusal")


# ------------------------------------------------------------------------------------------------ 7. moveRegionTo

def region_of(base, name="rotated"):
    if name == "rotated":
        return T.make_cut_region(base["c_world"] + (0.03, -0.02, 0.05), (0.7, 0.4, 0.55), SC.rotation([(0, 0.5), (1, -0.8)]))
    return T.make_cut_region(base["c_world"] + (0.01, 0.02, -0.03), (0.8, 0.5, 0.7), SC.rotation([(2, 0.4)]), T.CUT_ELLIPSOID)


def matrix_of(E, region, vs):
    return E.cut_region_transform(list(region.worldFromRegion), list(region.halfExtents), vs)


def test_move_region_to(E, oracle_lib, base):
    hp = config()[0]
    region = region_of(base)
    m = matrix_of(E, region, base["vs"])
    assert np.array_equal(m.view(np.uint32), base["regions"]["rotated box"][0].view(np.uint32))
    src, dst = fused_scene(E), fused_scene(E, range(5, 6))
    s0, d0 = SM.scene_of(src.state()), SM.scene_of(dst.state())
    assert SM.same_scene(s0, base["scene"])
    erased = SC.cut(s0, m, T.CUT_BOX, 0)
    lifted = SC.cut(s0, m, T.CUT_BOX, LIFT | KEEP)["lifted"]
    merged = SM.merge(d0, lifted, hp)
    assert merged["counts"]["present"] > 0 and merged["counts"]["allocated"] > 0 and merged["counts"]["combined"] > 0
    got = src.moveRegionTo(dst, region)
    print(got)
    SC.assert_counts(got, dict(erased["counts"], lifted=len(lifted[0]), voxels_lifted=erased["counts"]["voxels_erased"]), "move")
    SM.assert_counts(got["merge"], merged["counts"], "move: the merge")
    assert got["unsettled"] == 0 and got["merge"]["left_out"] == 0
    assert_is(src.state(), erased, "the source after the move")
    assert_is(dst.state(), merged, "the destination after the move")
    # extractRegion at the scene level is the list the move merged, and writes nothing
    probe = fused_scene(E)
    before = probe.download()
    ex = probe.extractRegion(region)
    assert_list_is(ex["descs"], ex["voxels"], lifted, "extractRegion")
    assert raw_equal(before, probe.download())
    # out and back: every observed voxel is restored to the bit
    a, b = fused_scene(E), E.CUDASceneRepHashSDF(hp, options())
    a.moveRegionTo(b, region)
    assert_is(b.state(), SM.merge(SM.empty_scene(), lifted, hp), "the region in an empty scene")
    b.moveRegionTo(a, region)
    assert b.state()["num_occupied"] == 0
    back = CR.voxels_by_position(a.state())
    for p, v in zip(*s0):
        obs = v["weight"] > 0
        if obs.any():
            now = np.frombuffer(back[tuple(int(x) for x in p)], T.VOXEL_DTYPE)
            assert now[obs].tobytes() == v[obs].tobytes(), f"block {p}: an observed voxel did not come back"
    # a destination pool too small: refused, both scenes as they were
    small_hp = config(pool=len(lifted[0]) - 1)[0]
    src2, small = fused_scene(E), E.CUDASceneRepHashSDF(small_hp, options())
    before_s, before_d = src2.download(), small.download()
    with pytest.raises(Exception) as err:
        src2.moveRegionTo(small, region)
    assert err.value.code == 1 and err.value.counts["merge"]["status"] == T.MERGE_HEAP_SHORT, err.value  # VH_ERR_HEAP_EXHAUSTED
    assert err.value.counts["voxels_erased"] == 0
    assert raw_equal(before_s, src2.download()) and raw_equal(before_d, small.download()), "a refused move changed a scene"


# ------------------------------------------------------------------------------------------------ 8. the cut scene is a scene

def test_the_cut_scene_ray_casts_and_integrates(E, oracle_lib, base):
    hp, cp, rp = config()
    region = region_of(base, "ellipsoid")
    scene = fused_scene(E)
    got = scene.eraseRegion(region)
    assert got["freed"] > 0 and got["voxels_erased"] > 0
    pose = synth.orbit_pose(1, 40)
    scene.setLastRigidTransformAndCompactify(pose, cp)
    d = scene.download()
    host = CR.host_copy(oracle_lib, d, scene.getHashParams(), cp, rp, options())
    want = host.render(pose)
    ray = E.CUDARayCastSDF(rp)
    ray.render(scene.getHashData(), scene.getHashParams(), cp, pose)
    maps = ray.download()
    assert_maps_equal(maps, want, "ray cast of the cut scene")
    full = fused_scene(E)
    full.setLastRigidTransformAndCompactify(pose, cp)
    ray.render(full.getHashData(), full.getHashParams(), cp, pose)
    assert not np.array_equal(ray.download()["depth"].view(np.uint32), maps["depth"].view(np.uint32)), "the cut was meant to show in the depth map"
    # crop, then the next frame: freed positions are allocated again
    crop = fused_scene(E)
    before = CR.position_set(crop.state()["positions"])
    got = crop.cropToRegion(region)
    assert got["freed"] > 0
    kept = CR.position_set(crop.state()["positions"])
    frame = E.DepthFrame(cp)
    pose = synth.orbit_pose(3, 40)
    E.synth_frame(synth.S1_SPHERES, 0, pose, cp, out=frame)
    crop.integrate(pose, frame, cp, None)
    after = crop.state()
    now = CR.position_set(after["positions"])
    assert (now - kept) & (before - kept), "no freed position was allocated again"
    rep = crop.debugHash()
    assert rep["duplicates"] == 0 and rep["lockEntries"] == 0
    assert crop.getState()[T.STATE_HEAP_UNDERFLOW] == 0


# ------------------------------------------------------------------------------------------------ 9. refusals, Reconstruction

def test_refusals_leave_the_scenes_alone(E, base):
    hp, cp, _ = config()
    region = region_of(base)
    src, dst = fused_scene(E), fused_scene(E, range(5, 6))
    before_s, before_d = src.download(), dst.download()

    def refused(call, code=4):  # VH_ERR_BAD_ARGUMENT
        with pytest.raises(Exception) as err:
            call()
        assert getattr(err.value, "code", None) == code, err.value
        assert raw_equal(before_s, src.download()) and raw_equal(before_d, dst.download()), "a refused cut changed a scene"

    refused(lambda: src.moveRegionTo(src, region))
    other_hp = config()[0]
    other_hp.m_virtualVoxelSize = np.float32(0.05)
    refused(lambda: src.moveRegionTo(E.CUDASceneRepHashSDF(other_hp, options()), region))
    not_rigid = T.make_cut_region(base["c_world"], (0.5, 0.5, 0.5), 1.01 * np.eye(3))
    flat = T.make_cut_region(base["c_world"], (0.5, 0.0, 0.5))
    no_shape = T.make_cut_region(base["c_world"], (0.5, 0.5, 0.5), shape=7)
    for bad in (not_rigid, flat, no_shape):
        refused(lambda: src.eraseRegion(bad))
        refused(lambda: src.cropToRegion(bad))
        refused(lambda: src.extractRegion(bad))
        refused(lambda: src.moveRegionTo(dst, bad))
    # a frame in flight (integrateAhead without integrateFinish), in the source and in the destination
    busy = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=False, gc=True, starve=2))
    frame = E.DepthFrame(cp)
    pose = synth.orbit_pose(0, 40)
    E.synth_frame(synth.S1_SPHERES, 0, pose, cp, out=frame)
    busy.integrateAhead(pose, frame, cp, None)
    refused(lambda: src.moveRegionTo(busy, region))
    for call in (lambda: busy.eraseRegion(region), lambda: busy.cropToRegion(region), lambda: busy.extractRegion(region), lambda: busy.moveRegionTo(dst, region)):
        with pytest.raises(Exception) as err:
            call()
        assert err.value.code == 4
    busy.integrateFinish(frame, cp)
    assert raw_equal(before_d, dst.download())
    # and the scenes still cut
    m = matrix_of(E, region, base["vs"])
    got = src.eraseRegion(region)
    want = SC.cut(base["scene"], m, T.CUT_BOX, 0)
    SC.assert_counts(got, want["counts"], "after the refusals")
    assert_is(src.state(), want, "after the refusals")
    assert busy.eraseRegion(region)["status"] == 0


MF_W, MF_H, MF_N = 64, 48, 3
MF_PARAMS = """
s_sensorIdx = 8;
s_adapterWidth = 64;
s_adapterHeight = 48;
s_sensorDepthMax = 5.0f;
s_sensorDepthMin = 0.5f;
s_hashNumBuckets = 16384;
s_hashNumSDFBlocks = 8192;
s_hashMaxCollisionLinkedListSize = 7;
s_SDFVoxelSize = 0.02f;
s_SDFMarchingCubeThreshFactor = 10.0f;
s_SDFTruncation = 0.10f;
s_SDFTruncationScale = 0.05f;
s_SDFMaxIntegrationDistance = 4.0f;
s_SDFIntegrationWeightSample = 10;
s_SDFIntegrationWeightMax = 255;
s_SDFRayIncrementFactor = 0.8f;
s_SDFRayThresSampleDistFactor = 50.5f;
s_SDFRayThresDistFactor = 50.0f;
s_SDFUseGradients = false;
s_integrationEnabled = true;
s_trackingEnabled = true;
s_garbageCollectionEnabled = false;
s_garbageCollectionStarve = 15;
s_marchingCubesMaxNumTriangles = 400000;
s_offlineProcessing = true;
s_playData = true;
s_reconstructionEnabled = true;
s_binaryDumpSensorUseTrajectory = true;
"""
MF_STREAMING = """s_streamingEnabled = true;
s_streamingVoxelExtents = 0.5f 0.5f 0.5f;
s_streamingGridDimensions = 65 65 65;
s_streamingMinGridPos = -32 -32 -32;
s_streamingInitialChunkListSize = 16;
s_streamingRadius = 1.3f;
s_streamingPos = 0.0f 0.0f 1.8f;
s_streamingOutParts = 4;
"""


def test_reconstruction_cuts(E, oracle_lib, tmp_path):
    """Reconstruction's methods: a streaming scene with blocks on the host refuses a modifying cut and extracts from its
    device blocks and its host blocks; a scene without streaming erases, crops and moves"""
    from voxelhashing_amd import reconstruction as R, sensor_data as SD
    cp = T.make_depth_camera_params(MF_W, MF_H)
    sd = SD.SensorData.create((MF_W, MF_H), (MF_W, MF_H), SD.make_intrinsic_matrix(cp.fx, cp.fy, cp.mx, cp.my), depth_shift=1000.0,
                              sensor_name="synthetic S3", depth_type=SD.TYPE_ZLIB_USHORT)
    for k in range(MF_N):
        p = synth.orbit_pose(k, n_frames=400)
        d, c = oracle_lib.synth_frame(synth.S3_SPHERES, 0, p, cp)
        mm = np.where(np.isfinite(d), np.floor(1000.0 * d.astype(np.float64) + 0.5), 0).astype(np.uint16)
        rgb = np.clip(np.where(np.isfinite(c[..., :3]), c[..., :3], 0) * 255.0, 0, 255).astype(np.uint8)
        sd.addFrame(rgb, mm, p, 100 + k, 200 + k)
    path = str(tmp_path / "s3.sens")
    sd.saveToFile(path)
    src = R.Reconstruction(R.read_app_state((MF_PARAMS + MF_STREAMING).encode()), sens_files=[path])
    assert src.run() == MF_N
    on_gpu, (h_descs, h_blocks) = src.scene.state(), src.chunk_grid.downloadHostBlocks()
    assert on_gpu["num_occupied"] > 20 and len(h_descs) > 20, "the source was meant to hold blocks on the device and on the host"
    vs = np.float32(src.scene.getHashParams().m_virtualVoxelSize)
    everywhere = SM.sort_scene(np.concatenate([on_gpu["positions"], h_descs["pos"].reshape(-1, 3)]), np.concatenate([on_gpu["voxels"], h_blocks]))
    coords = SC.voxel_coords(everywhere[0])[everywhere[1]["weight"] > 0].astype(np.float64) * float(vs)
    region = T.make_cut_region(np.median(coords, axis=0), (1.2, 0.6, 1.0), SC.rotation([(1, 0.3)]), T.CUT_ELLIPSOID)
    m = matrix_of(E, region, vs)
    for call in (src.eraseRegion, src.cropToRegion):
        with pytest.raises(ValueError):
            call(region)
    plain = R.Reconstruction(R.read_app_state((MF_PARAMS + "s_streamingEnabled = false;\n").encode()), sens_files=[path])
    with pytest.raises(ValueError):
        plain.moveRegionTo(src, region)
    with pytest.raises(ValueError):
        src.moveRegionTo(plain, region)
    before = src.scene.download()
    lists = src.extractRegion(region)
    assert raw_equal(before, src.scene.download())
    assert len(lists) == 2 and lists[0]["lifted"] > 0 and lists[1]["lifted"] > 0, "the region was meant to reach blocks on the device and on the host"
    want = SC.cut(everywhere, m, T.CUT_ELLIPSOID, LIFT | KEEP)
    got = SM.sort_scene(np.concatenate([l["descs"]["pos"].reshape(-1, 3) for l in lists]), np.concatenate([l["voxels"] for l in lists]))
    assert np.array_equal(got[0], want["lifted"][0]) and got[1].tobytes() == want["lifted"][1].tobytes(), "extractRegion of a streaming scene"
    assert lists[0]["voxels_lifted"] + lists[1]["voxels_lifted"] == want["counts"]["voxels_lifted"]
    # without streaming: erase, crop and move against the restatement
    assert plain.run() == MF_N
    whole = SM.scene_of(plain.scene.state())
    other = R.Reconstruction(R.read_app_state((MF_PARAMS + "s_streamingEnabled = false;\n").encode()), sens_files=[path])
    moved = plain.moveRegionTo(other, region)
    erased = SC.cut(whole, m, T.CUT_ELLIPSOID, 0)
    assert moved["status"] == 0 and moved["merge"]["status"] == 0
    assert_is(plain.scene.state(), erased, "Reconstruction.moveRegionTo: the source")
    assert_is(other.scene.state(), SM.merge(SM.empty_scene(), SC.cut(whole, m, T.CUT_ELLIPSOID, LIFT | KEEP)["lifted"], other.scene.getHashParams()),
              "Reconstruction.moveRegionTo: the destination")
    got = other.cropToRegion(region)
    assert got["voxels_erased"] == 0 and got["freed"] == 0, "what was moved lies inside the region"
    got = other.eraseRegion(region)
    assert got["voxels_erased"] == moved["voxels_lifted"] and other.scene.state()["num_occupied"] == 0
