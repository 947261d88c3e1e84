"""vh_query_points / vh_query_rays on the device against the reference's functions applied to the same points and rays
(tests/ray_query.py, pinned by tests/test_query_reference.py), always on the device's own table: the state is
downloaded into an OracleScene (crowded.host_copy) and the oracle's primitives run on that.  Tolerance 0 throughout."""
import ctypes as C

import numpy as np
import pytest

import crowded as CR
import ray_query as RQ
from helpers import bits, small_config
from voxelhashing_amd import canonical, lib, synth, vhtypes as T

pytestmark = pytest.mark.gpu
f32 = np.float32
FILL = 0xCD  # what the output buffers hold before a launch


@pytest.fixture(scope="module")
def E(vh):
    from voxelhashing_amd import engine
    return engine


# ---- launcher-level calls ---------------------------------------------------------------------------------------------

def query_points(hd, hp, pts, gradient=True, n=None, room=None):
    """vh_query_points on the first n of pts -> dict of whole output buffers (room entries, FILL bytes beyond n)"""
    L = lib.load()
    pts = np.ascontiguousarray(pts, dtype=f32).reshape(-1, 3)
    n = len(pts) if n is None else n
    room = len(pts) if room is None else room
    d_pts = lib.DeviceBuffer.from_numpy(pts)
    bufs = dict(sdf=lib.DeviceBuffer(4 * room), color=lib.DeviceBuffer(4 * room), gradient=lib.DeviceBuffer(12 * room), valid=lib.DeviceBuffer(room))
    for b in bufs.values():
        lib.check(L.vh_memset(b.ptr, FILL, b.nbytes, None))
    lib.check(L.vh_query_points(C.byref(hd), C.byref(hp), d_pts.ptr, n, bufs["sdf"].ptr, bufs["color"].ptr,
                                bufs["gradient"].ptr if gradient else None, bufs["valid"].ptr, None), "vh_query_points")
    return dict(sdf=bufs["sdf"].download(f32, room), color=bufs["color"].download(np.uint32, room),
                gradient=bufs["gradient"].download(f32, 3 * room).reshape(room, 3), valid=bufs["valid"].download(np.uint8, room))


def query_rays(hd, hp, rp, origins, directions, t_min, t_max, normals=True, n=None):
    L = lib.load()
    origins = np.ascontiguousarray(origins, dtype=f32).reshape(-1, 3)
    room = len(origins)
    n = room if n is None else n
    directions = np.ascontiguousarray(np.broadcast_to(np.asarray(directions, f32).reshape(-1, 3), (room, 3)))
    t_min, t_max = (np.ascontiguousarray(np.broadcast_to(np.asarray(a, f32).reshape(-1), (room,))) for a in (t_min, t_max))
    ins = [lib.DeviceBuffer.from_numpy(a) for a in (origins, directions, t_min, t_max)]
    bufs = dict(t=lib.DeviceBuffer(4 * room), normal=lib.DeviceBuffer(12 * room), color=lib.DeviceBuffer(4 * room), status=lib.DeviceBuffer(room))
    for b in bufs.values():
        lib.check(L.vh_memset(b.ptr, FILL, b.nbytes, None))
    lib.check(L.vh_query_rays(C.byref(hd), C.byref(hp), C.byref(rp), ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, n, bufs["t"].ptr,
                              bufs["normal"].ptr if normals else None, bufs["color"].ptr, bufs["status"].ptr, None), "vh_query_rays")
    return dict(t=bufs["t"].download(f32, room), normal=bufs["normal"].download(f32, 3 * room).reshape(room, 3),
                color=bufs["color"].download(np.uint32, room), status=bufs["status"].download(np.uint8, room))


def untouched(a, n):
    return bool(np.all(np.ascontiguousarray(a[n:]).view(np.uint8) == FILL))


def assert_points(got, want, what, n=None, gradient=True):
    n = len(want["valid"]) if n is None else n
    assert np.array_equal(got["valid"][:n], want["valid"][:n]), f"{what}: valid"
    assert np.array_equal(bits(got["sdf"][:n]), bits(want["sdf"][:n])), f"{what}: sdf bits"
    assert np.array_equal(got["color"][:n], want["color"][:n]), f"{what}: colour"
    if gradient:
        assert np.array_equal(bits(got["gradient"][:n]), bits(want["gradient"][:n])), f"{what}: gradient bits"
    else:
        assert untouched(got["gradient"], 0), f"{what}: a NULL gradient array is not written"
    for k in ("valid", "sdf", "color", "gradient"):
        assert untouched(got[k], n), f"{what}: {k} written beyond n"


def assert_rays(got, want, what, n=None, normals=True):
    n = len(want["status"]) if n is None else n
    bad = np.nonzero(got["status"][:n] != want["status"][:n])[0]
    assert len(bad) == 0, f"{what}: status differs at {len(bad)} rays, first {bad[:4]}: {got['status'][bad[:4]]} want {want['status'][bad[:4]]}"
    assert np.array_equal(bits(got["t"][:n]), bits(want["t"][:n])), f"{what}: t bits"
    assert np.array_equal(got["color"][:n], want["color"][:n]), f"{what}: colour"
    if normals:
        assert np.array_equal(bits(got["normal"][:n]), bits(want["normal"][:n])), f"{what}: normal bits"
    else:
        assert untouched(got["normal"], 0), f"{what}: a NULL normal array is not written"
    for k in ("status", "t", "color", "normal"):
        assert untouched(got[k], n), f"{what}: {k} written beyond n"


def point_sets(hits, vs, seed, uniform=2000):
    """(a) hit positions + N(0, voxel) noise, (b) uniform points in the hits' box grown by 0.3 m, (c) the set (a) on the
    voxel lattice, (d) on the block lattice"""
    rng = np.random.default_rng(seed)
    a = (hits + rng.normal(0.0, vs, size=hits.shape)).astype(f32)
    lo, hi = hits.min(axis=0) - 0.3, hits.max(axis=0) + 0.3
    b = rng.uniform(lo, hi, size=(uniform, 3)).astype(f32)
    c = (np.round(a / f32(vs)) * f32(vs)).astype(f32)
    d = (np.round(a / f32(8 * vs)) * f32(8 * vs)).astype(f32)
    return a, b, c, d


# ---- the scene of the issue: S1, 64x48 (P4), three offline frames, the view of a fourth pose ------------------------------

@pytest.fixture(scope="module")
def world(E, oracle_lib):
    """the device scene, its table in an OracleScene, the view's camera rays and point sets with their references
    (computed once; the tests only read them)"""
    O = oracle_lib
    hp, cp, rp = small_config(64, 48)
    rp.m_useGradients = 1
    scene = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=True))
    frame = E.DepthFrame(cp)
    for k in range(3):
        pose = synth.orbit_pose(k, n_frames=100)
        E.synth_frame(synth.S1_SPHERES, 0, pose, cp, out=frame)
        scene.integrate(pose, frame, cp, None)
    hd, hp = scene.getHashData(), scene.getHashParams()
    host = CR.host_copy(O, scene.download(), hp, cp, rp)
    view = np.array(synth.orbit_pose(5, n_frames=100), f32)
    rpv = RQ.view_params(O, rp, view)
    cam = RQ.camera_rays(host.L, cp, rpv)
    ref = RQ.rays(host.L, host.hd, host.hp, rpv, cam["origins"], cam["directions"], cam["t_min"], cam["t_max"])
    hit = ref["status"] == RQ.HIT
    assert hit.sum() >= 1000 and (ref["status"] == RQ.MISS).sum() >= 1000, "the camera set must hold 1000 hits and 1000 misses"
    hits = cam["origins"][hit].astype(np.float64) + cam["directions"][hit].astype(np.float64) * ref["t"][hit, None].astype(np.float64)
    vs = hp.m_virtualVoxelSize
    a, b, c, d = point_sets(hits, vs, seed=11)
    far = hits[0] + np.array([1e6, 0, 0])
    special = np.array([far, [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan], hits[1]], f32)
    special[5, 2] = np.inf
    pts = np.concatenate([a, b, c, d, special])
    pref = RQ.points(host.L, host.hd, host.hp, pts)
    assert pref["valid"].sum() >= 1000 and (pref["valid"] == 0).sum() >= 1000, "the point set must hold 1000 valid and 1000 invalid points"
    return dict(O=O, scene=scene, hd=hd, hp=hp, cp=cp, rp=rpv, host=host, view=view, cam=cam, ref=ref, hit=hit, hits=hits, pts=pts, pref=pref,
                n_special=len(special))


def test_points_match_the_reference(world):
    w = world
    got = query_points(w["hd"], w["hp"], w["pts"])
    assert_points(got, w["pref"], "all points")
    tail = slice(len(w["pts"]) - w["n_special"], None)
    assert not got["valid"][tail].any() and np.all(got["sdf"][tail] == -np.inf) and np.all(got["color"][tail] == 0)
    assert np.all(bits(got["gradient"][tail][1:]) == 0), "a non-finite point has gradient (0, 0, 0)"
    invalid = w["pref"]["valid"] == 0
    assert np.all(got["sdf"][invalid] == -np.inf) and np.all(got["color"][invalid] == 0)
    assert np.any(w["pref"]["gradient"][invalid] != 0), "the reference's gradient is observable at invalid points too"
    assert_points(query_points(w["hd"], w["hp"], w["pts"], gradient=False), w["pref"], "without a gradient array", gradient=False)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_points_prefixes(world, n):
    w = world
    assert_points(query_points(w["hd"], w["hp"], w["pts"][:128], n=n), w["pref"], f"n = {n}", n=n)


def test_camera_rays_match_the_restatement(world):
    w = world
    cam = w["cam"]
    got = query_rays(w["hd"], w["hp"], w["rp"], cam["origins"], cam["directions"], cam["t_min"], cam["t_max"])
    assert_rays(got, w["ref"], "camera rays in raster order")
    miss = got["status"] == RQ.MISS
    assert np.all(got["t"][miss] == -np.inf) and np.all(got["normal"][miss] == -np.inf) and np.all(got["color"][miss] == 0)
    # a fixed random permutation gives the permuted results
    perm = np.random.default_rng(3).permutation(len(cam["t_min"]))
    shuffled = query_rays(w["hd"], w["hp"], w["rp"], cam["origins"][perm], cam["directions"][perm], cam["t_min"][perm], cam["t_max"][perm])
    assert_rays(shuffled, {k: v[perm] for k, v in w["ref"].items()}, "camera rays permuted")
    assert_rays(query_rays(w["hd"], w["hp"], w["rp"], cam["origins"], cam["directions"], cam["t_min"], cam["t_max"], normals=False), w["ref"],
                "without a normal array", normals=False)


def maps_of_rays(got, cam, rp):
    """what the render's maps hold for query results `got` of the view's camera rays (the identities of
    tests/test_query_reference.py) -> (hit [n], depth [n], rgb [n, 3], camera-space normals of the hits)"""
    hit = got["status"] == RQ.HIT
    with np.errstate(all="ignore"):
        depth = got["t"] / cam["depth_to_ray_length"]
    rgb = np.stack([got["color"] & 0xff, (got["color"] >> 8) & 0xff, (got["color"] >> 16) & 0xff], axis=-1).astype(f32) / f32(255)
    normals = np.stack([RQ.mat_mul_d(rp.m_viewMatrix, v) for v in got["normal"][hit]])
    return hit, depth, rgb, normals


def assert_maps_match_rays(maps, want, n, what):
    hit, depth, rgb, normals = want
    assert np.array_equal(hit, maps["depth"].reshape(n) != -np.inf), f"{what}: a miss is a miss"
    assert np.array_equal(bits(depth[hit]), bits(maps["depth"].reshape(n)[hit])), f"{what}: depth bits"
    assert np.array_equal(bits(rgb[hit]), bits(maps["colors"].reshape(n, 4)[hit, :3])), f"{what}: colour bits"
    assert np.array_equal(bits(normals), bits(maps["normals"].reshape(n, 4)[hit, :3])), f"{what}: normal bits"


def test_camera_rays_match_the_device_render(world, E):
    """the identities of tests/test_query_reference.py against the device's own maps (full-range march and tile tables)"""
    w = world
    cam, rp = w["cam"], w["rp"]
    got = query_rays(w["hd"], w["hp"], rp, cam["origins"], cam["directions"], cam["t_min"], cam["t_max"])
    want = maps_of_rays(got, cam, rp)
    for intervals in (False, True):
        ray = E.CUDARayCastSDF(rp)
        ray.setIntervalSplatting(intervals)
        ray.render(w["hd"], w["hp"], w["cp"], w["view"])
        assert_maps_match_rays(ray.download(), want, rp.m_width * rp.m_height, f"intervals={intervals}")


def test_rejected_sign_changes_resume_the_march(world, E, vh):
    """Both acceptance thresholds tightened to the scale of one ray increment (the defaults, 50.5 and 50 increments,
    accept practically every sign change): a sample pair further apart than one increment (rays that meet the surface
    head-on) or a sample deeper than half an increment behind the surface is rejected, the march sample becomes the last
    sample and the march goes on.  The query and the three marches of the render must all do so as the restatement does."""
    import tile_intervals as TI
    from test_gpu_render_lookups import render_hash, render_intervals
    w = world
    cam, host = w["cam"], w["host"]
    rp = type(w["rp"]).from_buffer_copy(w["rp"])
    inc = f32(rp.m_rayIncrement)
    rp.m_thresSampleDist, rp.m_thresDist = float(inc), float(f32(0.5) * inc)
    want = RQ.rays(host.L, host.hd, host.hp, rp, cam["origins"], cam["directions"], cam["t_min"], cam["t_max"])
    moved = (want["status"] != w["ref"]["status"]) | (bits(want["t"]) != bits(w["ref"]["t"]))
    n_moved, n_hit = int(moved.sum()), int((want["status"] == RQ.HIT).sum())
    print(f"\ntightened thresholds: {n_moved} rays changed status or t, {n_hit} still hit")
    assert n_moved >= 100 and n_hit >= 100
    got = query_rays(w["hd"], w["hp"], rp, cam["origins"], cam["directions"], cam["t_min"], cam["t_max"])
    assert_rays(got, want, "tightened thresholds")
    maps = maps_of_rays(got, cam, rp)
    W, H = rp.m_width, rp.m_height
    ray = E.CUDARayCastSDF(rp)
    assert_maps_match_rays(render_hash(vh, lib, ray, w["hd"], w["hp"], w["cp"], rp, W, H), maps, W * H, "hash-table render")
    for cap, what in ((TI.CAP_SMALL, "small tables"), (TI.CAP_LARGE, "large tables (pipelined march)")):
        assert_maps_match_rays(render_intervals(vh, lib, ray, w["hd"], w["hp"], w["cp"], rp, W, H, cap)[0], maps, W * H, what)


def test_rays_with_differing_sample_phases(world):
    """a per-ray tMin offset from [0, increment): the lanes of a wave sample at different phases"""
    w = world
    cam, host = w["cam"], w["host"]
    off = (np.random.default_rng(5).random(len(cam["t_min"])) * w["rp"].m_rayIncrement).astype(f32)
    t_min = cam["t_min"] + off
    want = RQ.rays(host.L, host.hd, host.hp, w["rp"], cam["origins"], cam["directions"], t_min, cam["t_max"])
    assert (want["status"] == RQ.HIT).sum() >= 1000
    assert np.any(want["t"] != w["ref"]["t"]), "the offsets were meant to move the samples"
    assert_rays(query_rays(w["hd"], w["hp"], w["rp"], cam["origins"], cam["directions"], t_min, cam["t_max"]), want, "offset tMin")


def test_special_rays(world):
    w = world
    cam, host, rp, hit = w["cam"], w["host"], w["rp"], w["hit"]
    inc, vs = f32(rp.m_rayIncrement), f32(w["hp"].m_virtualVoxelSize)
    pick = np.nonzero(hit)[0][:: max(1, hit.sum() // 64)][:64]
    o, d, t0, t1 = cam["origins"][pick], cam["directions"][pick], cam["t_min"][pick], cam["t_max"][pick]
    groups = {}

    def add(name, origins, directions, t_min, t_max):
        n = len(origins)
        groups[name] = (np.asarray(origins, f32), np.broadcast_to(np.asarray(directions, f32), (n, 3)),
                        np.broadcast_to(np.asarray(t_min, f32), (n,)), np.broadcast_to(np.asarray(t_max, f32), (n,)))

    add("empty interval", o[:8], d[:8], t1[:8], np.concatenate([t1[:4], t0[:4]]))
    surface = o.astype(np.float64) + d.astype(np.float64) * w["ref"]["t"][pick, None].astype(np.float64)
    behind = (surface + 1.5 * float(vs) * d.astype(np.float64)).astype(f32)  # 1.5 voxels behind the surface, looking on
    add("from behind the surface", behind, d, 0.0, 2.0)
    t_far = f32(3000.0)
    add("from 3000 m away", (o.astype(np.float64) - 3000.0 * d.astype(np.float64)).astype(f32), d, t_far, t_far + f32(6.0))
    add("zero direction", o[:2], np.array([[0, 0, 0], [0, -0.0, 0]], f32), t0[:2], t1[:2])
    add("non-finite", np.array([[np.nan, 0, 0], o[0], o[0], o[0]], f32), np.array([d[0], [0, np.inf, 1], d[0], d[0]], f32),
        np.array([t0[0], t0[0], -np.inf, t0[0]], f32), np.array([t1[0], t1[0], t1[0], np.nan], f32))
    add("too long", o[:2], d[:2], 0.0, np.array([f32(65537) * inc, f32(3e38)], f32))
    stall = f32(2.0 ** 24) * inc * f32(4)  # t + increment == t: the sample count ends the march
    add("stalled", o[:1], d[:1] * f32(1e-9), stall, np.nextafter(stall, f32(np.inf)))
    add("unnormalised direction", o, d * f32(0.75), t0 / f32(0.75), t1 / f32(0.75))
    add("negative parameters", o + d * f32(8.0), d, t0 - f32(8.0), t1 - f32(8.0))  # |tMin| > |tMax|
    origins, directions, t_min, t_max = (np.concatenate([g[k] for g in groups.values()]) for k in range(4))
    want = RQ.rays(host.L, host.hd, host.hp, rp, origins, directions, t_min, t_max)
    at, start = {}, 0
    for name, g in groups.items():
        at[name] = slice(start, start + len(g[0]))
        start += len(g[0])
    # what the reference says of each group (conditions on the test's own inputs)
    assert np.all(want["status"][at["empty interval"]] == RQ.MISS) and np.all(want["samples"][at["empty interval"]] == 0)
    assert np.all(want["status"][at["zero direction"]] == RQ.REFUSED) and np.all(want["status"][at["non-finite"]] == RQ.REFUSED)
    assert np.all(want["status"][at["too long"]] == RQ.REFUSED)
    assert want["status"][at["stalled"]][0] == RQ.MISS and want["samples"][at["stalled"]][0] == RQ.MAX_SAMPLES
    assert (want["status"][at["from 3000 m away"]] == RQ.HIT).sum() >= 32
    assert (want["status"][at["unnormalised direction"]] == RQ.HIT).sum() >= 32
    assert (want["status"][at["negative parameters"]] == RQ.HIT).sum() >= 32 and np.all(t_max[at["negative parameters"]] < 0)
    assert np.all(want["status"][at["from behind the surface"]] != RQ.REFUSED)
    assert (want["status"][at["from behind the surface"]] == RQ.HIT).sum() < 32, "a ray that starts inside meets no positive sample first"
    q = (np.abs(origins[at["from 3000 m away"]]).sum(axis=1) + t_max[at["from 3000 m away"]] * np.abs(directions[at["from 3000 m away"]]).sum(axis=1)) / vs
    assert np.all(q >= 65536), "these rays were meant to take the uncertified tap path"
    got = query_rays(w["hd"], w["hp"], rp, origins, directions, t_min, t_max)
    for name, sl in at.items():
        assert_rays({k: v[sl] for k, v in got.items()}, {k: v[sl] for k, v in want.items()}, name)
    first = at["from behind the surface"].start  # n = 1 and 65 on a slice that starts with ordinary rays
    sub = [a[first:first + 96] for a in (origins, directions, t_min, t_max)]
    for n in (1, 65):
        assert_rays(query_rays(w["hd"], w["hp"], rp, *sub, n=n), {k: v[first:first + 96] for k, v in want.items()}, f"n = {n}", n=n)
    assert_rays(query_rays(w["hd"], w["hp"], rp, *sub, normals=False), {k: v[first:first + 96] for k, v in want.items()}, "no normals", normals=False)


def test_queries_leave_the_scene_alone(world):
    w = world
    scene, cam = w["scene"], w["cam"]
    before, words = scene.state(), scene.getState()
    query_points(w["hd"], w["hp"], w["pts"])
    query_rays(w["hd"], w["hp"], w["rp"], cam["origins"], cam["directions"], cam["t_min"], cam["t_max"])
    after = scene.state()
    canonical.assert_same_scene(before, after, "before and after a pair of queries")
    assert before["voxels"].tobytes() == after["voxels"].tobytes()
    assert np.array_equal(words, scene.getState())


def test_python_wrappers_return_the_launcher_results(world, E):
    w = world
    cam = w["cam"]
    pts = w["pts"][-700:]
    want = query_points(w["hd"], w["hp"], pts)
    got = w["scene"].queryPoints(pts)
    assert np.array_equal(got["valid"], want["valid"].astype(bool)) and np.array_equal(bits(got["sdf"]), bits(want["sdf"]))
    assert np.array_equal(bits(got["gradient"]), bits(want["gradient"]))
    assert got["color"].shape == (len(pts), 3) and got["color"].dtype == np.uint8
    assert np.array_equal(RQ.pack_rgb(got["color"]), want["color"])
    assert w["scene"].queryPoints(pts, gradient=False)["gradient"] is None
    ray = E.CUDARayCastSDF(w["rp"])
    want = query_rays(w["hd"], w["hp"], w["rp"], cam["origins"], cam["directions"], cam["t_min"], cam["t_max"])
    got = ray.castRays(w["hd"], w["hp"], cam["origins"], cam["directions"], cam["t_min"], cam["t_max"])
    assert np.array_equal(got["status"], want["status"]) and np.array_equal(bits(got["t"]), bits(want["t"]))
    assert np.array_equal(bits(got["normal"]), bits(want["normal"])) and np.array_equal(RQ.pack_rgb(got["color"]), want["color"])
    assert ray.castRays(w["hd"], w["hp"], cam["origins"], cam["directions"], cam["t_min"], cam["t_max"], normals=False)["normal"] is None
    # scalars broadcast: every ray with the widest interval of the set
    lo, hi = float(cam["t_min"].min()), float(cam["t_max"].max())
    wide = ray.castRays(w["hd"], w["hp"], cam["origins"][:256], cam["directions"][:256], lo, hi)
    want = query_rays(w["hd"], w["hp"], w["rp"], cam["origins"][:256], cam["directions"][:256], lo, hi)
    assert np.array_equal(wide["status"], want["status"]) and np.array_equal(bits(wide["t"]), bits(want["t"]))
    empty = w["scene"].queryPoints(np.zeros((0, 3), f32))
    assert len(empty["sdf"]) == 0 and len(empty["valid"]) == 0


# ---- a crowded table: scenario B of tests/crowded.py (23 buckets: look-ups walk collision lists) ------------------------

def test_queries_through_collision_lists(E, oracle_lib):
    from test_gpu_crowded_tables import lists_formed, run_launchers
    O = oracle_lib
    poses = CR.poses("B")
    # (`new` bounds the alloc passes of a frame: the loop ends at the fixed point)
    g, _ = run_launchers(E, O, "B", dict(frames=[dict(pose=p, new=64) for p in poses]), None, True)
    lists_formed(g.download(False)["hash"], g.hp)
    hp, cp, rp = CR.config("B")
    host = CR.host_copy(O, g.download(), g.hp, cp, rp, CR.options())
    rpv = RQ.view_params(O, rp, poses[-1])
    cam = RQ.camera_rays(host.L, cp, rpv)
    want = RQ.rays(host.L, host.hd, host.hp, rpv, cam["origins"], cam["directions"], cam["t_min"], cam["t_max"])
    hit = want["status"] == RQ.HIT
    assert hit.sum() >= 300 and (~hit).sum() >= 300
    assert_rays(query_rays(g.hd, g.hp, rpv, cam["origins"], cam["directions"], cam["t_min"], cam["t_max"]), want, "camera rays on table B")
    hits = cam["origins"][hit].astype(np.float64) + cam["directions"][hit].astype(np.float64) * want["t"][hit, None].astype(np.float64)
    a, b, c, _ = point_sets(hits, g.hp.m_virtualVoxelSize, seed=13, uniform=1000)
    pts = np.concatenate([a, b, c])
    pref = RQ.points(host.L, host.hd, host.hp, pts)
    assert pref["valid"].sum() >= 500 and (pref["valid"] == 0).sum() >= 500
    assert_points(query_points(g.hd, g.hp, pts), pref, "points on table B")
