"""The oracle against the reference's own kernels that need a barrier, stream, mesh or filter images, compiled for the
CPU (oracle/_ref/libvh_ref.so; see tests/test_reference_pinning.py for the rest).

Compactify and GC identify run through the emulator's fibers (oracle/ref/vhr_launch.cpp); the streaming, marching
cubes and CameraUtil.cu kernels through its plain serial path.  Every comparison is bit for bit.  The one fenced
reference defect these kernels reach -- stream-out's list branch pushes the heap a second time -- is run on the
reference anyway and held to its exact difference; stream-in's list branch, which corrupts the
table, is not run on the reference.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from oracle import reference as R
from helpers import make_color_rgbx, make_depth, stream_out_replay
from voxelhashing_amd import canonical, synth, vhtypes as T

pytestmark = pytest.mark.skipif(not R.available(), reason="oracle/_ref/libvh_ref.so is not built (build() makes it "
                                "where the reference tree is present)")

f32 = np.float32
FP, IP = C.POINTER(C.c_float), C.POINTER(C.c_int32)
MINF = f32(-np.inf)


@pytest.fixture(scope="module")
def libs():
    O.build()
    return O.lib(), R.lib()


def ip(a):
    return np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(IP)


def fp(a):
    return np.ascontiguousarray(a, dtype=np.float32).ctypes.data_as(FP)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _pose(k, off, step=90):
    q = np.array(synth.orbit_pose(k, step), dtype=np.float32).copy()
    q[3] += f32(off[0]); q[7] += f32(off[1]); q[11] += f32(off[2])
    return q


def _spheres(off):
    s = synth.S1_SPHERES.copy()
    s[:, :3] += np.array(off)
    return s


def _alloc(s, pos):
    """one block, the bucket mutex released first (allocBlock takes it and leaves it taken)"""
    s.reset_mutex()
    s.alloc_block(pos)


def _copy_state(src, dst):
    for field, dt, n in (("d_hash", T.HASH_ENTRY_DTYPE, src.num_entries()),
                         ("d_SDFBlocks", T.VOXEL_DTYPE, src.hp.m_numSDFBlocks * 512),
                         ("d_heap", np.uint32, src.hp.m_numSDFBlocks), ("d_heapCounter", np.uint32, 1),
                         ("d_hashBucketMutex", np.int32, src.hp.m_hashNumBuckets)):
        dst.array(field, dt, n)[:] = src.array(field, dt, n)
    C.memmove(C.byref(dst.hp), C.byref(src.hp), C.sizeof(src.hp))


def _assert_same_scene(a, b, what):
    assert np.array_equal(a.hash_table().view(np.uint8), b.hash_table().view(np.uint8)), f"{what}: table"
    assert np.array_equal(a.heap(), b.heap()), f"{what}: heap"
    assert np.array_equal(a.array("d_heapCounter", np.uint32, 1), b.array("d_heapCounter", np.uint32, 1)), what
    assert np.array_equal(a.sdf_blocks().view(np.uint8), b.sdf_blocks().view(np.uint8)), f"{what}: voxels"


def _scene(off, name="P4", size=(160, 120), frames=2, buckets=1 << 15, blocks=1 << 13):
    """two copies of one integrated state: the oracle's (a) and the one the reference runs on (b)"""
    hp = T.make_hash_params(buckets, blocks, **synth.PARAM_SETS[name])
    cp = T.make_depth_camera_params(*size)
    a = O.OracleScene(hp, cp, options=T.make_scene_options(offline=True, gc=False))
    spheres = _spheres(off)
    poses = [_pose(k, off) for k in range(frames)]
    for q in poses:
        d, c = O.synth_frame(spheres, 0, q, cp)
        a.integrate(q, d, c)
    b = O.OracleScene(hp, cp)
    _copy_state(a, b)
    return a, b, R.RefScene(b), poses


# ---------------------------------------------------------------------------------------------------------- compactify

def _assert_same_compactify(a, b, rb, what):
    n_a = a.compactify()
    n_b = rb.compactify()
    assert n_a == n_b == b.hp.m_numOccupiedBlocks, f"{what}: count {n_a} != {n_b}"
    assert int(b.array("d_hashCompactifiedCounter", np.int32, 1)[0]) == n_b, what
    assert np.array_equal(a.compactified().view(np.uint8), b.compactified().view(np.uint8)), f"{what}: list"
    return n_b


@pytest.mark.parametrize("off", [(7.3, 5.1, 3.7), (-7.3, -5.1, -3.7)])
def test_compactify_on_integrated_states(libs, off):
    a, b, rb, poses = _scene(off)
    for k, q in enumerate(poses + [_pose(5, off)]):
        a.set_transform(q); b.set_transform(q)
        n = _assert_same_compactify(a, b, rb, f"pose {k}")
        assert 0 < n
    live = int((a.hash_table()["ptr"] != T.FREE_ENTRY).sum())
    assert n < live  # the last pose leaves blocks outside the frustum


def test_compactify_at_image_border_and_depth_limits(libs):
    """blocks around the rays through the image border, at both depth limits: some in, some out"""
    Lo, Lr = libs
    hp = T.make_hash_params(1 << 14, 1 << 14, **synth.PARAM_SETS["P4"])
    cp = T.make_depth_camera_params(64, 48, depth_min=0.5, depth_max=3.0)
    a, b = O.OracleScene(hp, cp), O.OracleScene(hp, cp)
    rb = R.RefScene(b)
    W, H = cp.m_imageWidth, cp.m_imageHeight
    border = [(x, y) for x in (0, W - 1) for y in range(0, H, 5)] + [(x, y) for y in (0, H - 1) for x in range(0, W, 5)]
    blocks = set()
    for (x, y) in border + [(W // 2, H // 2)]:
        for z in (cp.m_sensorDepthWorldMin, cp.m_sensorDepthWorldMax):
            p = np.zeros(3, np.float32)
            Lr.vhr_depth_to_skeleton(C.byref(cp), x, y, f32(z), p.ctypes.data_as(FP))
            blk = np.zeros(3, np.int32)
            Lr.vhr_world_to_sdf_block(C.byref(hp), p.ctypes.data_as(FP), blk.ctypes.data_as(IP))
            for d in np.ndindex(3, 3, 3):
                blocks.add(tuple(int(v) for v in blk + np.array(d) - 1))
    for pos in sorted(blocks):
        _alloc(a, pos)
    _copy_state(a, b)
    table = a.hash_table()
    live = table["pos"][table["ptr"] != T.FREE_ENTRY]
    assert len(live) == len(blocks)
    inside = sum(Lr.vhr_is_block_in_frustum(C.byref(hp), C.byref(cp), ip(p)) for p in live)
    assert 0 < inside < len(blocks)
    assert _assert_same_compactify(a, b, rb, "border and depth limits") == inside


def test_compactify_empty_table(libs):
    hp = T.make_hash_params(1000, 64, **synth.PARAM_SETS["P4"])
    cp = T.make_depth_camera_params(64, 48)
    a, b = O.OracleScene(hp, cp), O.OracleScene(hp, cp)
    b.array("d_hashCompactifiedCounter", np.int32, 1)[0] = 77
    assert _assert_same_compactify(a, b, R.RefScene(b), "empty") == 0


def test_compactify_across_many_workgroups(libs):
    """2^16 buckets: 2 560 workgroups of 256, a scattered set of blocks"""
    hp = T.make_hash_params(1 << 16, 1 << 14, **synth.PARAM_SETS["P4"])
    cp = T.make_depth_camera_params(160, 120)
    a, b = O.OracleScene(hp, cp), O.OracleScene(hp, cp)
    rng = np.random.default_rng(11)
    for pos in rng.integers(-16, 17, size=(6000, 3)):
        _alloc(a, (pos[0], pos[1], abs(pos[2])))
    _copy_state(a, b)
    n = _assert_same_compactify(a, b, R.RefScene(b), "many workgroups")
    assert n > 256


# ---------------------------------------------------------------------------------------------------------- GC identify

def _gc_tables(nblocks):
    hp = T.make_hash_params(1 << 12, nblocks, **synth.PARAM_SETS["P4"])
    cp = T.make_depth_camera_params(64, 48)
    a, b = O.OracleScene(hp, cp), O.OracleScene(hp, cp)
    for k in range(nblocks):
        _alloc(a, (k, 0, 0))
    return a, b


def _gc_compare(a, b, what):
    table = a.hash_table()
    live = table[table["ptr"] != T.FREE_ENTRY]
    for s in (a, b):
        s.array("d_hashCompactified", T.HASH_ENTRY_DTYPE, len(live))[:] = live
        s.hp.m_numOccupiedBlocks = len(live)
    _copy_state(a, b)
    b.array("d_hashCompactified", T.HASH_ENTRY_DTYPE, len(live))[:] = live
    a.array("d_hashDecision", np.int32, len(live))[:] = -7
    b.array("d_hashDecision", np.int32, len(live))[:] = -7
    a.gc_identify()
    R.RefScene(b).gc_identify()
    got, want = b.decisions().copy(), a.decisions().copy()
    assert np.array_equal(got, want), f"{what}: decisions {got} != {want}"
    return got, live


def test_gc_identify_on_crafted_voxels(libs):
    Lo, Lr = libs
    cases = []
    hp0 = T.make_hash_params(1 << 12, 64, **synth.PARAM_SETS["P4"])
    cp0 = T.make_depth_camera_params(64, 48)
    t = f32(Lr.vhr_get_truncation(C.byref(hp0), f32(cp0.m_sensorDepthWorldMax)))
    up, down = np.nextafter(t, f32(np.inf)), np.nextafter(t, f32(-np.inf))

    def one(sdf, at=100, w=1, rest_w=0, rest_sdf=0.0):
        def f(v):
            v["weight"] = rest_w
            v["sdf"] = rest_sdf
            v["sdf"][at] = sdf
            v["weight"][at] = w
        return f

    def want_of(sdf, w=1):
        return int(not (w > 0 and np.abs(f32(sdf)) < t))

    cases.append(("all weights 0", one(0.0, w=0), 1))
    for name, s in (("t", t), ("-t", -t), ("t+ulp", up), ("t-ulp", down), ("-(t-ulp)", -down), ("-(t+ulp)", -up),
                    ("+0", f32(0.0)), ("-0", f32(-0.0))):
        cases.append((f"one voxel at |sdf| {name}", one(s), want_of(s)))
    cases.append(("NaN sdf", one(np.nan), None))
    cases.append(("NaN beside a near voxel", one(np.nan, at=7, rest_w=1, rest_sdf=0.01), None))
    cases.append(("weight 255, far", one(2.0 * t, w=255, rest_w=255, rest_sdf=2.0 * t), 1))
    cases.append(("weight 255, near", one(0.0, w=255, rest_w=255, rest_sdf=2.0 * t), 0))
    for at in (0, 1, 510, 511):
        cases.append((f"only live voxel {at}", one(0.0, at=at), 0))
        cases.append((f"only live voxel {at}, far", one(up, at=at), 1))
        cases.append((f"only live voxel {at}, near, others far", one(down, at=at, rest_w=3, rest_sdf=up), 0))
    a, b = _gc_tables(len(cases) + 8)
    table = a.hash_table()
    ptrs = table["ptr"][table["ptr"] != T.FREE_ENTRY]
    vox = a.sdf_blocks()
    rng = np.random.default_rng(3)
    for (name, f, want), p in zip(cases, ptrs):
        v = vox[p:p + 512]
        f(v)
    for p in ptrs[len(cases):]:  # random blocks
        v = vox[p:p + 512]
        v["weight"] = rng.integers(0, 3, 512)
        v["sdf"] = rng.uniform(-2 * t, 2 * t, 512).astype(np.float32)
    got, live = _gc_compare(a, b, "crafted")
    for (name, f, want), p, g in zip(cases, ptrs, got):
        if want is not None:
            assert g == want, f"{name}: decision {g}, expected {want}"


# ------------------------------------------------------------------------------------------ a frame loop with GC

@pytest.mark.parametrize("off", [(7.3, 5.1, 3.7), (-7.3, -5.1, -3.7)])
def test_frame_loop_with_gc_run_by_the_reference(libs, off):
    """alloc, compactify, integrate, starve every other frame, GC identify and GC free: the reference's kernels alone
    against the oracle's frame loop, after every frame"""
    hp = T.make_hash_params(1 << 14, 1 << 13, **synth.PARAM_SETS["P4"])
    cp = T.make_depth_camera_params(160, 120)
    freed, _, _ = check_frame_loop_with_gc(hp, cp, _spheres(off), [_pose(k, off, step=12) for k in range(7)])
    assert freed > 0


def check_frame_loop_with_gc(hp, cp, spheres, poses, starve=2):
    """the online frame loop with GC by the reference's kernels (b) and by the oracle (a), compared after every frame
    -> (blocks GC freed, a, b)"""
    opt = T.make_scene_options(offline=False, gc=True, starve=starve)
    a, b = O.OracleScene(hp, cp, options=opt), O.OracleScene(hp, cp, options=opt)
    rb = R.RefScene(b)
    freed = 0
    for k, q in enumerate(poses):
        d, c = O.synth_frame(spheres, 0, q, cp)
        a.integrate(q, d, c)
        freed += rb.integrate(q, d, c)
        canonical.assert_same_scene(a.state(), b.state(), f"frame {k}")
        _assert_same_scene(a, b, f"frame {k}")
    return freed, a, b


# ------------------------------------------------------------------------------------------------------- stream out

def _block_distance(Lr, hp, pos, cam):
    w = np.zeros(3, np.float32)
    Lr.vhr_sdf_block_to_world(C.byref(hp), ip(pos), w.ctypes.data_as(FP))
    v = (w - cam).astype(np.float32)
    return np.sqrt(f32(v[0] * v[0] + v[1] * v[1]) + f32(v[2] * v[2]), dtype=np.float32)


def _bucket_only(a, b):
    """free every collision-list entry in both copies (the oracle's delete), so that stream-out meets buckets only"""
    table = a.hash_table()
    lst = [tuple(e["pos"]) for i, e in enumerate(table) if e["ptr"] != T.FREE_ENTRY and
           O.lib().vho_compute_hash_pos(C.byref(a.hp), ip(e["pos"])) != i // T.HASH_BUCKET_SIZE]
    for p in lst:
        a.delete_block(p)
    _copy_state(a, b)
    return len(lst)


@pytest.mark.parametrize("off", [(7.3, 5.1, 3.7), (-7.3, -5.1, -3.7)])
def test_stream_out_and_back_in(libs, off):
    Lo, Lr = libs
    a, b, rb, poses = _scene(off, buckets=1 << 12, blocks=1 << 13)
    _bucket_only(a, b)
    cam = np.array([poses[0][3], poses[0][7], poses[0][11]], np.float32)
    table = a.hash_table()
    live = table[table["ptr"] != T.FREE_ENTRY]
    dist = np.array([_block_distance(Lr, a.hp, e["pos"], cam) for e in live], np.float32)
    radius = np.sort(dist)[len(dist) // 2]
    # blocks at exactly the radius and one ulp either side of it
    # blocks lie exactly at the radius: one ulp above it, fewer leave
    assert (dist >= radius).sum() > (dist >= np.nextafter(radius, f32(np.inf))).sum()
    ne = a.num_entries()
    for r in (radius, np.nextafter(radius, f32(np.inf)), np.nextafter(radius, f32(-np.inf))):
        a2, b2 = O.OracleScene(a.hp, a.cp), O.OracleScene(a.hp, a.cp)
        _copy_state(a, a2); _copy_state(a, b2)
        rb2 = R.RefScene(b2)
        descs_a, descs_b = [], []
        for start, part in ((0, 1000), (1000, 64), (1064, 1), (1065, 3000), (4065, ne - 4065 + 100)):
            descs_a.append(a2.stream_out_pass1(part, start, float(r), cam))
            descs_b.append(rb2.stream_out_pass1(part, start, float(r), cam))
            assert np.array_equal(descs_a[-1].view(np.uint8), descs_b[-1].view(np.uint8)), f"radius {r}: pass 1 part {start}"
            _assert_same_scene(a2, b2, f"radius {r}: pass 1 part {start}")
            va, vb = a2.stream_out_pass2(descs_a[-1]), rb2.stream_out_pass2(descs_b[-1])
            assert np.array_equal(va.view(np.uint8), vb.view(np.uint8)), f"radius {r}: pass 2 part {start}"
            _assert_same_scene(a2, b2, f"radius {r}: pass 2 part {start}")
        assert sum(len(d) for d in descs_a) == int((dist >= r).sum())
    # stream in: the blocks streamed out at the radius, back into a copy of the state they left
    a3, b3 = O.OracleScene(a.hp, a.cp), O.OracleScene(a.hp, a.cp)
    _copy_state(a, a3); _copy_state(a, b3)
    rb3 = R.RefScene(b3)
    da = a3.stream_out_pass1(ne, 0, float(radius), cam)
    va = a3.stream_out_pass2(da)
    db = rb3.stream_out_pass1(ne, 0, float(radius), cam)
    vb = rb3.stream_out_pass2(db)
    assert np.array_equal(va.view(np.uint8), vb.view(np.uint8))
    order = np.random.default_rng(5).permutation(len(da))
    for lo, hi in ((0, 7), (7, len(da))):
        sel = order[lo:hi]
        assert a3.stream_in(da[sel], va[sel]) == 0
        assert rb3.stream_in(db[sel], vb[sel]) == 0
        _assert_same_scene(a3, b3, f"stream in {lo}:{hi}")
    canonical.assert_same_scene(a3.state(), a.state(), "out and back in")


def test_stream_out_list_entries_hold_the_fenced_difference(libs):
    """Entries in collision lists: the reference's list branch pushes the heap again after deleteHashEntryElement
    (DESIGN.md section 2).  Everything equals the oracle except the reference's heap, which has one extra push after
    each listed entry streamed out; the extra id is ptr / 512 of what the entry's slot holds after the delete -- a
    live block that moved up the list, or FREE_ENTRY's quotient."""
    Lo, Lr = libs
    hp = T.make_hash_params(16, 256, **synth.PARAM_SETS["P4"], max_collision_list=7)
    cp = T.make_depth_camera_params(64, 48)
    a, b = O.OracleScene(hp, cp), O.OracleScene(hp, cp)
    rng = np.random.default_rng(9)  # a state whose list deletes leave both a moved-up block and a free slot
    for pos in rng.integers(-30, 31, size=(400, 3)):
        _alloc(a, pos)
    _copy_state(a, b)
    rb = R.RefScene(b)
    ne = a.num_entries()
    table0 = a.hash_table().copy()
    hash_of = lambda pos: int(Lo.vho_compute_hash_pos(C.byref(hp), ip(pos)))
    listed = [i for i, e in enumerate(table0) if e["ptr"] != T.FREE_ENTRY and (e["offset"] != 0 or
                                                                             hash_of(e["pos"]) != i // T.HASH_BUCKET_SIZE)]
    assert len(listed) > 5
    # the extra ids, by replaying the pass slot by slot on a third copy with the oracle's single operations
    c = O.OracleScene(hp, cp)
    _copy_state(a, c)
    want_a, want_b, extras = stream_out_replay(c, hash_of)
    assert (2 ** 32 - 2) // 512 in extras and any(x < 256 for x in extras)
    counter0 = int(a.array("d_heapCounter", np.uint32, 1)[0])
    da = a.stream_out_pass1(ne, 0, 0.0, np.zeros(3, np.float32))
    db = rb.stream_out_pass1(ne, 0, 0.0, np.zeros(3, np.float32))
    assert np.array_equal(da.view(np.uint8), db.view(np.uint8))
    assert np.array_equal(a.hash_table().view(np.uint8), b.hash_table().view(np.uint8))
    assert np.array_equal(a.sdf_blocks().view(np.uint8), b.sdf_blocks().view(np.uint8))
    ca, cb = int(a.array("d_heapCounter", np.uint32, 1)[0]), int(b.array("d_heapCounter", np.uint32, 1)[0])
    assert cb - ca == len(extras)
    pushed_a, pushed_b = list(a.heap()[counter0 + 1:ca + 1]), list(b.heap()[counter0 + 1:cb + 1])
    assert pushed_a == want_a
    assert pushed_b == want_b
    assert np.array_equal(a.heap()[:counter0 + 1], b.heap()[:counter0 + 1])


# --------------------------------------------------------------------------------------------------- marching cubes

def _mc_sorted(tris):
    return np.sort(np.ascontiguousarray(tris).view(np.dtype((np.void, tris.dtype.itemsize))).ravel())


@pytest.mark.parametrize("name,off", [("P4", (7.3, 5.1, 3.7)), ("P2", (-7.3, -5.1, -3.7))])
def test_marching_cubes(libs, name, off):
    a, b, rb, poses = _scene(off, name=name, size=(160, 120), buckets=1 << 15, blocks=1 << 14)
    mp = T.make_marching_cubes_params(a.hp, 1 << 19)
    variants = [("default", mp)]
    thr = T.make_marching_cubes_params(a.hp, 1 << 19, thresh_factor=1.5)
    variants.append(("thresholds", thr))
    box = T.make_marching_cubes_params(a.hp, 1 << 19)
    box.m_boxEnabled = 1
    v = a.extract_iso_surface(mp)[0]["v"]["p"].reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    box.m_minCorner = (C.c_float * 3)(*lo.tolist())
    box.m_maxCorner = (C.c_float * 3)(*((lo + hi) / 2).tolist())
    variants.append(("box", box))
    full = None
    for what, p in variants:
        want, n = a.extract_iso_surface(p)
        assert n > 100, what
        for two in (True, False):
            got, m = rb.extract_iso_surface(p, two_pass=two)
            assert m == n, f"{what}: {m} != {n} triangles"
            if two:  # serial order is the oracle's: entries in table order, voxels x fastest
                assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), what
            assert np.array_equal(_mc_sorted(got), _mc_sorted(want)), what
        if what == "default":
            full = n
        else:
            assert n < full, what
    cap = full // 3
    want, n = a.extract_iso_surface(mp, max_triangles=cap)
    got, m = rb.extract_iso_surface(mp, max_triangles=cap)
    assert n >= cap and m == cap and len(want) == cap
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))


def test_marching_cubes_on_crafted_fields(libs):
    """The fields of tests/mc_fields.py: every cube case with the edge-mask-255 rule, far coordinates, the threshold
    comparison stepped over its rounding edge, unobserved taps and snapped vertices.  The state is the oracle's after
    its stream-in, copied; the reference's own extraction on it against the oracle's, bit for bit."""
    import mc_fields as F

    def compare(name, descs, blocks, what, count=None):
        hp, cp, mp, vs = F.config(name)
        a, b = O.OracleScene(hp, cp), O.OracleScene(hp, cp)
        assert a.stream_in(descs, blocks) == 0
        _copy_state(a, b)
        rb = R.RefScene(b)
        want, n = a.extract_iso_surface(mp)
        assert count is None or n == count, f"{what}: {n} triangles, {count} expected"
        for two in (True, False):
            got, m = rb.extract_iso_surface(mp, two_pass=two)
            assert m == n, f"{what}: {m} != {n} triangles"
            if two:
                assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), what
            assert np.array_equal(_mc_sorted(got), _mc_sorted(want)), what
        return n

    for name in ("P2", "P4"):
        vs = f32(synth.PARAM_SETS[name]["voxel_size"])
        thres = f32(10.0) * vs
        for origin in (F.NEAR, (131070, -2, -1)):
            n = compare(name, *F.planted(origin, vs, f32(10.0) * vs), f"{name} planted at {origin}")
            assert n > 10000
        for origin in (F.NEAR, F.FAR):
            for k, count in zip(F.SWEEP_KS, F.SWEEP_COUNTS[origin]):
                compare(name, *F.planted(origin, vs, F.sweep_amplitude(thres, k)), f"{name} sweep {k} at {origin}", count)
    for name, seed in F.RANDOM_SEEDS:
        thres = f32(10.0) * f32(synth.PARAM_SETS[name]["voxel_size"])
        descs, blocks = F.random_field(F.block_ids(), seed, float(thres), **F.RANDOM)
        assert compare(name, descs, blocks, f"{name} random {seed}") > 5000
        assert compare(name, *F.without(descs, blocks, F.LEFT_OUT), f"{name} random {seed}, 18 blocks") > 2000


# ------------------------------------------------------------------------------------------------------ sensor maps

SIZES = [(1, 1), (7, 5), (33, 9), (101, 77), (640, 480)]


def _same(op, *args, **kw):
    a = O.image_op(op, *args, **kw)
    b = R.image_op(op, *args, **kw)
    assert np.array_equal(bits(a), bits(b)), f"{op} {args[1:3]} {args[3:]} {kw.get('out_size')}"
    return a


@pytest.mark.parametrize("w,h", SIZES)
def test_sensor_maps(libs, w, h):
    rgbx, depth = make_color_rgbx(w, h, 3), make_depth(w, h, 4, holes=0.1 if w * h > 1 else 0.0)
    cp = T.make_depth_camera_params(w, h)
    colf = _same("convert_color_raw_to_float4", rgbx, w, h, out_channels=4)
    for ow, oh in ((w, h), (max(w // 2, 1), max(h // 2, 1)), (2 * w - 1, 2 * h - 1), (w + 13, max(h - 7, 1))):
        pre = np.full((oh, ow), 7.0, dtype=np.float32)
        _same("resample_float_map", depth, w, h, out_size=(ow, oh), prefill=pre)
        pre4 = np.full((oh, ow, 4), 7.0, dtype=np.float32)
        _same("resample_float4_map", colf, w, h, out_channels=4, out_size=(ow, oh), prefill=pre4)
    inten = _same("convert_color_to_intensity_float", colf, w, h)
    _same("convert_depth_float_to_camera_space_float4", depth, w, h, cp, out_channels=4)
    for size, thr, frac in ((1, 0.05, 0.3), (5, 0.05, 0.3), (2, 0.01, 0.9)):
        _same("erode_depth_map", depth, w, h, size, thr, frac)
    for sigma_d, sigma_r in ((1.0, 0.05), (2.5, 0.1), (0.7, 1.0), (4.5, 0.2), (0.5, 0.1), (3.0, 10.0), (4.0, 0.1)):
        _same("gauss_filter_float_map", depth, w, h, sigma_d, sigma_r)
        _same("bilateral_filter_float_map", depth, w, h, sigma_d, sigma_r)
        _same("gauss_filter_float4_map", colf, w, h, sigma_d, 10.0 * sigma_r, out_channels=4)
    # computeIntensityAndDerivatives against the restatement the tracking tests use
    from rgbd_icp import intensity_and_derivatives
    got = R.compute_intensity_and_derivatives(inten)
    assert np.array_equal(bits(got), bits(intensity_and_derivatives(inten)))
