"""The resampled merge on the device (vh_resample.hip) against the numpy restatement of its rule
(tests/scene_resample.py): the transforms that permute voxels, half a voxel along x, general rigid motions at ratios 1, 2
and 1/2 bit for bit, a linear field against the analytic one, sources on crowded tables, the table's integrity and a ray
cast of the result, and the refusals.  Sources are crafted blocks merged into an empty table."""

import numpy as np
import pytest

import crowded as CR
import scene_merge as SM
import scene_resample as SR
from helpers import assert_maps_equal
from voxelhashing_amd import canonical, synth, vhtypes as T

pytestmark = pytest.mark.gpu
V = T.SDF_BLOCK_VOXELS
ROOMY = 1 << 14


@pytest.fixture(scope="module")
def E(vh):
    from voxelhashing_amd import engine
    return engine


def params(vs, buckets=ROOMY, pool=4096, limit=7):
    return T.make_hash_params(buckets, pool, float(np.float32(vs)), max_collision_list=limit)


def descs_of(positions):
    d = np.zeros(len(positions), T.DESC_DTYPE)
    d["pos"] = positions
    return d


def launcher_with(E, hp, scene):
    """a LauncherScene holding the blocks of a (positions, voxels) scene"""
    g = E.LauncherScene(hp)
    if len(scene[0]):
        got = g.merge_blocks(descs_of(scene[0]), scene[1], 1)
        assert (got["allocated"], got["left_out"], got["status"]) == (len(scene[0]), 0, 0), got
    return g


def scene_with(E, hp, scene):
    s = E.CUDASceneRepHashSDF(hp, CR.options())
    if len(scene[0]):
        got = s.mergeBlocks(descs_of(scene[0]), scene[1])
        assert (got["allocated"], got["left_out"], got["status"]) == (len(scene[0]), 0, 0), got
    return s


def scene_of(snap):
    return snap["positions"], snap["voxels"]


def raw_equal(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a if k != "params")


def assert_is(snap, want, what):
    assert np.array_equal(snap["positions"], want["positions"]), f"{what}: block position sets differ"
    assert snap["voxels"].tobytes() == want["voxels"].tobytes(), f"{what}: voxel bytes differ"


def staged_scene(out):
    return SM.sort_scene(out["descs"]["pos"], out["voxels"])


MOTIONS = {
    "first": (SR.rotation((1, 2, 3), 0.6), (1.7, -2.3, 3.1)),
    "second": (SR.rotation((-2, 1, -0.5), -2.1), (-0.9, 1.4, -2.2)),
}
GENERAL = [("first", 1.0), ("second", 1.0), ("first", 2.0), ("second", 0.5)]  # (motion, vs_dst / vs_src)


@pytest.fixture(scope="module")
def S():
    """the crafted source: 64 blocks straddling the origin"""
    src = SR.crafted_source(11)
    assert len(src[0]) == 64 and (src[1]["weight"] > 0).any(axis=1).sum() == 61
    return src


@pytest.fixture(scope="module")
def general(S):
    """the restatement of the general motions, computed once: {case: (M, vs_src, vs_dst, a, b, staged)}"""
    out = {}
    for name, ratio in GENERAL:
        R, t = MOTIONS[name]
        vs_src = float(np.float32(0.04))
        vs_dst = float(np.float32(vs_src * ratio))
        M = SR.rigid(R, t)
        a, b = SR.voxel_transforms(M, vs_src, vs_dst)
        out[(name, ratio)] = (M, vs_src, vs_dst, a, b, SR.resample(S, a, b))
    return out


# ------------------------------------------------------------------------------------------------ 1. exact cases

@pytest.mark.parametrize("vs", [0.04, 0.01])
def test_exact_transforms_permute_the_voxels(E, S, vs):
    """identity, a shift of whole voxels, a quarter turn with the shift, a destination twice as coarse: into an empty
    destination and into one that overlaps the source, the merged bytes are scene_merge.merge's of the permuted voxels"""
    D = SR.random_blocks(SR.crafted_source(12, corner=(0, -2, -2))[0], 13)
    for name, M, vs_src, vs_dst, where in SR.exact_cases(vs):
        want_staged = SR.permuted(S, where)
        for d_name, d in (("empty", SM.empty_scene()), ("overlapping", D)):
            what = f"{name} at {vs} into an {d_name} destination"
            hp_d = params(vs_dst)
            src, dst = scene_with(E, params(vs_src), S), scene_with(E, hp_d, d)
            want = SM.merge(d, want_staged, hp_d)
            got = dst.mergeSceneTransformed(src, M)
            SM.assert_counts(got, want["counts"], what)
            assert got["left_out"] == 0
            assert got["resample"]["staged"] == len(want_staged[0]) and got["resample"]["status"] == 0, (what, got)
            assert got["resample"]["observed"] == int((want_staged[1]["weight"] > 0).sum())
            assert got["resample"]["candidates"] >= got["resample"]["staged"]
            assert_is(dst.state(), want, what)
            if d_name == "overlapping":
                assert 0 < want["counts"]["present"] and want["counts"]["combined"] > 0, "the destination was meant to overlap"
            if name == "identity":
                # the plain merge, but for the blocks without an observed voxel, which allocate there and not here
                plain = scene_with(E, hp_d, d)
                keep = (S[1]["weight"] > 0).any(axis=1)
                plain.mergeBlocks(descs_of(S[0][keep]), S[1][keep])
                assert_is(dst.state(), plain.state(), what + " vs mergeBlocks")
                if d_name == "empty":
                    every = E.CUDASceneRepHashSDF(hp_d, CR.options())
                    every.mergeScene(src)
                    assert every.state()["num_occupied"] == dst.state()["num_occupied"] + int((~keep).sum())


# ------------------------------------------------------------------------------------------------ 2. half a voxel

def test_half_a_voxel_along_x(E, S):
    vs = float(np.float32(0.04))
    a, b = E.resample_voxel_transforms(SR.rigid(None, (0.5 * vs, 0, 0)), vs, vs)
    g = launcher_with(E, params(vs), S)
    out = g.resample_blocks(a, b)
    assert out["status"] == 0 and out["source_blocks"] == 64
    pos, vox = staged_scene(out)
    SR.assert_half_voxel_blend(S, pos, vox)
    assert out["observed"] == int((vox["weight"] > 0).sum())


# ------------------------------------------------------------------------------------------------ 3. general rigid motions

@pytest.mark.parametrize("case", GENERAL, ids=[f"{n}-{r}" for n, r in GENERAL])
def test_general_motions_bit_for_bit(E, S, general, case):
    M, vs_src, vs_dst, a, b, want = general[case]
    assert want["counts"]["staged"] > 20 and want["counts"]["observed"] > 300
    da, db = E.resample_voxel_transforms(M, vs_src, vs_dst)
    assert da.tobytes() == a.tobytes() and db.tobytes() == b.tobytes()
    # the staged list, twice
    g = launcher_with(E, params(vs_src), S)
    runs = [g.resample_blocks(a, b) for _ in range(2)]
    for out in runs:
        for k in ("source_blocks", "staged", "observed", "status"):
            assert out[k] == want["counts"][k], (k, out[k], want["counts"])
        assert out["candidates"] >= out["staged"]
        assert len(np.unique(out["descs"]["pos"], axis=0)) == out["staged"], "a block is listed twice"
        assert len(np.unique(out["descs"]["ptr"])) == out["staged"] and (out["descs"]["ptr"] % V == 0).all()
        assert SM.same_scene(staged_scene(out), (want["positions"], want["voxels"])), "the staged list differs from the restatement"
    assert runs[0]["candidates"] == runs[1]["candidates"]
    # the merged destination: half of the staged positions are there already, and blocks that nothing names
    far = want["positions"][:5] + np.array([100, 0, 0], np.int32)
    D = SR.random_blocks(np.concatenate([want["positions"][::2], far]), 21)
    hp_d = params(vs_dst)
    merged = SM.merge(D, (want["positions"], want["voxels"]), hp_d)
    states = []
    for _ in range(2):
        src, dst = scene_with(E, params(vs_src), S), scene_with(E, hp_d, D)
        got = dst.mergeSceneTransformed(src, M)
        SM.assert_counts(got, merged["counts"], str(case))
        assert got["left_out"] == 0 and got["present"] == len(want["positions"][::2])
        for k in ("source_blocks", "staged", "observed", "status"):
            assert got["resample"][k] == want["counts"][k], (k, got["resample"], want["counts"])
        st = dst.state()
        assert_is(st, merged, str(case))
        states.append(st)
        assert_is(src.state(), dict(zip(("positions", "voxels"), S)), "the source afterwards")
    assert states[0]["voxels"].tobytes() == states[1]["voxels"].tobytes()
    now, had = CR.voxels_by_position(states[0]), CR.voxels_by_position(dict(zip(("positions", "voxels"), D)))
    for p in far:
        assert now[tuple(int(v) for v in p)] == had[tuple(int(v) for v in p)], "a block no staged block names changed"


# ------------------------------------------------------------------------------------------------ 4. linear field

@pytest.mark.parametrize("vs, qmax", [(0.04, 152), (0.01, 752), (0.004, 1800)])
def test_a_linear_field_stays_linear(E, vs, qmax):
    """Blending a linear field is exact in real numbers, so what is left is rounding: of the sample position (three
    products and three sums at coordinates up to qmax, and three rounded matrix entries times a coordinate: 8 ulp(qmax)
    voxels between them) and of the eight-term blend and the stored field (16 * 2^-24 relative).
    Measured on the restatement, which the device equals bit for bit: 1.10 / 1.38 / 1.39 micrometres against bounds of
    6.82 / 5.37 / 4.10, and every probed voxel observed."""
    (pos, vox), n, d = SR.linear_field(vs, qmax, (0.3, -0.5, 0.81))
    vs = float(np.float32(vs))
    centre = np.full(3, qmax - 32.0) * vs
    R = SR.rotation((1, 2, 3), 0.6)
    M = SR.rigid(R, centre - R @ centre + np.array([0.013, -0.021, 0.017]))  # a turn about the box's centre, and a bit
    a, b = E.resample_voxel_transforms(M, vs, vs)
    g = launcher_with(E, params(vs, pool=1024), (pos, vox))
    out = g.resample_blocks(a, b)
    assert out["status"] == 0 and out["source_blocks"] == 512
    box, laid = SR.over_the_box(pos, b, out["descs"]["pos"], out["voxels"])
    err, seen, probed, most = SR.linear_field_errors(box, laid, M, vs, vs, qmax, n, d)
    bound = 8.0 * float(np.spacing(np.float32(qmax))) * vs + 16.0 * 2.0 ** -24 * most
    print(f"vs {vs} qmax {qmax}: error {err * 1e6:.2f} um, bound {bound * 1e6:.2f} um, {seen} of {probed} probed voxels observed")
    assert probed > 100000
    assert seen >= 0.9 * probed
    assert err <= bound


# ------------------------------------------------------------------------------------------------ 5. crowded source

def crowded_source(buckets):
    """a lump of blocks whose table of `buckets` buckets overflows into lists, under the precondition of
    tests/crowded.py that makes alloc's outcome the same on every schedule"""
    if buckets == 23:
        pos = SR.ball_of_blocks(190)
        over, fullest = CR.assert_precondition_b(pos, 23, 256)
    else:
        # a lump, and thirteen blocks each in three buckets that are not neighbours
        lump = SR.ball_of_blocks(60)
        k = np.arange(-8, 8)
        cube = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int32)
        cube = cube[np.abs(cube).max(axis=1) > 4]
        home, have = canonical.hash_buckets(cube, buckets), CR.bucket_demand(lump, buckets)
        chosen, extra = [], []
        for bkt in range(buckets):
            near = [(bkt + o) % buckets for o in (-2, -1, 0, 1, 2)]
            if have[near].sum() == 0 and not any(c in near for c in chosen) and (home == bkt).sum() >= 13:
                chosen.append(bkt)
                extra.append(cube[home == bkt][:13])
            if len(chosen) == 3:
                break
        assert len(chosen) == 3
        pos = np.concatenate([lump] + extra)
        over, fullest = CR.assert_precondition_a(pos, buckets, 7)
    assert over >= 3 and fullest > T.HASH_BUCKET_SIZE
    return SR.random_blocks(pos, 31)


@pytest.mark.parametrize("name", ["B", "A"])
def test_a_crowded_source_gives_the_roomy_result(E, name):
    s = CR.SCENARIOS[name]
    src = crowded_source(s["buckets"])
    vs = 0.04
    M = SR.rigid(*MOTIONS["first"])
    a, b = E.resample_voxel_transforms(M, vs, vs)
    outs = {}
    for buckets in (ROOMY, s["buckets"]):
        hp = params(vs, buckets, pool=CR.POOL, limit=s["limit"])
        g = launcher_with(E, hp, src)
        st = g.state()
        chains = canonical.check_chains(st["raw"]["hash"], hp)
        if buckets != ROOMY:
            assert chains["listed"] >= 3, f"the source's table was meant to hold collision lists: {chains}"
        outs[buckets] = g.resample_blocks(a, b)
        assert outs[buckets]["status"] == 0 and outs[buckets]["staged"] > 50
        assert raw_equal(st["raw"], g.download()), "resampling changed its source"
    roomy, tight = outs[ROOMY], outs[s["buckets"]]
    for k in T.RESAMPLE_COUNTS:
        assert roomy[k] == tight[k], (k, roomy[k], tight[k])
    assert SM.same_scene(staged_scene(roomy), staged_scene(tight))


# ------------------------------------------------------------------------------------------------ 6. the result is a scene

def test_the_resampled_scene_is_a_scene_and_ray_casts(E, oracle_lib, S):
    """into a crowded destination: the invariants and every list hold, and a ray cast equals the oracle's on a host copy of
    the table the device built"""
    hp, cp, rp = CR.config("A")
    hp_s = params(hp.m_virtualVoxelSize)
    M = SR.rigid(SR.rotation((1, 2, 3), 0.6), (0.0, 0.0, 1.2))
    # a surface to see: a plane through the source's blocks, truncated, every voxel observed, positive towards the camera
    # (the ray march looks for a change from positive to negative)
    vs = float(hp.m_virtualVoxelSize)
    x = (S[0].astype(np.int64)[:, None, :] * 8 + SR.LOCAL[None]) * vs
    plane = S[1].copy()
    plane["sdf"] = np.clip(-(x @ np.array([0.2, -0.1, 0.97])) / np.linalg.norm([0.2, -0.1, 0.97]), -hp.m_truncation, hp.m_truncation).astype(np.float32)
    plane["weight"] = 10
    src = scene_with(E, hp_s, (S[0], plane))
    dst = E.CUDASceneRepHashSDF(hp, CR.options())
    got = dst.mergeSceneTransformed(src, M)
    assert got["status"] == 0 and got["left_out"] == 0 and got["allocated"] == got["resample"]["staged"] > 50
    st = dst.state()  # (check_invariants, the bucket summary)
    assert st["num_occupied"] == got["allocated"]
    assert dst.debugHash()["duplicates"] == 0
    canonical.check_chains(dst.download(False)["hash"], dst.getHashParams())
    pose = np.eye(4, dtype=np.float32).reshape(16)
    dst.setLastRigidTransformAndCompactify(pose, cp)
    assert dst.getNumOccupiedBlocks() > 20
    d = dst.download()
    host = CR.host_copy(oracle_lib, d, dst.getHashParams(), cp, rp, CR.options())
    want = host.render(pose)
    ray = E.CUDARayCastSDF(rp)
    ray.render(dst.getHashData(), dst.getHashParams(), cp, pose)
    have = ray.download()
    assert_maps_equal(have, want, "ray cast of the resampled scene")
    assert int((have["depth"] != -np.inf).sum()) > 0, "the maps were meant to show the model"


# ------------------------------------------------------------------------------------------------ 7. refusals and limits

def test_refusals_leave_the_destination_alone(E, S, general):
    vs = float(np.float32(0.04))
    hp = params(vs)
    D = SR.random_blocks(SR.crafted_source(12, corner=(0, -2, -2))[0], 13)
    src, dst = scene_with(E, hp, S), scene_with(E, hp, D)
    before = dst.download()
    R = SR.rotation((1, 2, 3), 0.6)
    good = SR.rigid(R, (0.4, -0.2, 0.3))

    def refused(call, code=4, status=None):
        with pytest.raises(Exception) as err:
            call()
        assert getattr(err.value, "code", None) == code, err.value
        if status is not None:
            assert err.value.counts["resample"]["status"] == status, err.value.counts
        assert raw_equal(before, dst.download()), "a refused merge changed the destination"

    scaled, sheared, mirrored, nan = (good.copy() for _ in range(4))
    scaled[:3, :3] *= 1.01
    sheared[0, 1] += 0.01
    mirrored[:3, :3] = R @ np.diag([1.0, 1.0, -1.0])
    nan[1, 3] = np.nan
    for M in (scaled, sheared, mirrored, nan):
        refused(lambda: dst.mergeSceneTransformed(src, M))
    coarse = scene_with(E, params(np.float32(2.5) * np.float32(vs)), S)
    refused(lambda: dst.mergeSceneTransformed(coarse, good))  # a ratio of 2.5
    refused(lambda: dst.mergeSceneTransformed(dst, good))
    # a frame in flight, in the source and in the destination
    _, cp, _ = CR.config("B", ROOMY)
    busy = E.CUDASceneRepHashSDF(CR.config("B", ROOMY)[0], T.make_scene_options(offline=False, gc=True, starve=2))
    frame = E.DepthFrame(cp)
    pose = CR.poses("B")[0]
    E.synth_frame(synth.S1_SPHERES, 0, pose, cp, out=frame)
    busy.integrateAhead(pose, frame, cp, None)
    refused(lambda: dst.mergeSceneTransformed(busy, good))
    with pytest.raises(Exception) as err:
        busy.mergeSceneTransformed(src, good)
    assert err.value.code == 4
    busy.integrateFinish(frame, cp)
    # a block at 2^20: outside the lattice's range
    edge = SR.random_blocks(np.array([[1 << 20, 0, 0], [0, 0, 0]], np.int32), 41)
    refused(lambda: dst.mergeSceneTransformed(scene_with(E, hp, edge), good), status=T.RESAMPLE_OUT_OF_RANGE)
    g = launcher_with(E, hp, edge)
    out = g.resample_blocks(*E.resample_voxel_transforms(good, vs, vs))
    assert out["status"] == T.RESAMPLE_OUT_OF_RANGE and out["staged"] == 0 and len(out["descs"]) == 0
    # ... and a block inside it whose image is not
    inner = SR.random_blocks(np.array([[(1 << 20) - 1, 0, 0]], np.int32), 42)
    refused(lambda: dst.mergeSceneTransformed(scene_with(E, hp, inner), SR.rigid(None, (16 * vs, 0, 0))), status=T.RESAMPLE_OUT_OF_RANGE)
    # the heap one block short
    M, vs_src, vs_dst, a, b, want = general[("first", 1.0)]
    short = params(vs, pool=len(D[0]) + want["counts"]["staged"] - 1)
    tight = scene_with(E, short, D)
    assert len(CR.union(D[0], want["positions"])) == len(D[0]) + want["counts"]["staged"], "the image was meant to miss the destination"
    before_tight = tight.download()
    with pytest.raises(Exception) as err:
        tight.mergeSceneTransformed(src, M)
    assert err.value.code == 1 and err.value.counts["status"] == T.MERGE_HEAP_SHORT, err.value  # VH_ERR_HEAP_EXHAUSTED
    assert raw_equal(before_tight, tight.download()), "a refused merge changed the destination"
    # and the scene still merges
    got = dst.mergeSceneTransformed(src, M)
    assert_is(dst.state(), SM.merge(D, (want["positions"], want["voxels"]), hp), "after the refusals")
    assert got["status"] == 0


def test_a_full_candidate_table_is_reported_and_grown(E):
    """eight blocks far from each other, turned: each reaches more than 16 destination blocks, the slots the scene-level
    call starts with.  At the launcher level the status says so and nothing is staged; the scene-level call grows the
    table and gives the restatement's scene."""
    vs = float(np.float32(0.04))
    hp = params(vs)
    k = np.arange(8)
    pos = np.stack([10 * (k & 1), 10 * ((k >> 1) & 1), 10 * (k >> 2)], axis=-1).astype(np.int32) - 5
    src = SR.random_blocks(pos, 51)
    M = SR.rigid(SR.rotation((1, 2, 3), 0.6), (0.1, 0.2, 0.3))
    a, b = E.resample_voxel_transforms(M, vs, vs)
    g = launcher_with(E, hp, src)
    roomy = g.resample_blocks(a, b, slots_log2=12)
    assert roomy["status"] == 0 and roomy["candidates"] > 16 * 8, roomy["candidates"]
    full = g.resample_blocks(a, b, slots_log2=7)  # 16 slots per source block
    assert full["status"] == T.RESAMPLE_TABLE_FULL and full["staged"] == 0 and len(full["descs"]) == 0
    want = SR.resample(src, a, b)
    assert SM.same_scene(staged_scene(roomy), (want["positions"], want["voxels"]))
    dst = E.CUDASceneRepHashSDF(hp, CR.options())
    got = dst.mergeSceneTransformed(scene_with(E, hp, src), M)
    assert got["resample"]["status"] == 0 and got["resample"]["candidates"] == roomy["candidates"]
    assert_is(dst.state(), SM.merge(SM.empty_scene(), (want["positions"], want["voxels"]), hp), "after growing the table")


def test_merge_from_with_a_transform(E, oracle_lib, tmp_path):
    """Reconstruction.mergeFrom(other, transform=): a whole-voxel shift of a reconstruction gives its voxels moved; a
    streaming source with blocks on the host is refused before anything is done"""
    from test_gpu_scene_merge import MF_H, MF_N, MF_PARAMS, MF_STREAMING, MF_W
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
    plain = MF_PARAMS + "s_streamingEnabled = false;\n"
    src = R.Reconstruction(R.read_app_state(plain.encode()), sens_files=[path])
    assert src.run() == MF_N
    have = src.scene.state()
    assert have["num_occupied"] > 20
    vs = float(np.float32(0.02))
    M = SR.rigid(None, SR.SHIFT * vs)
    dst = R.Reconstruction(R.read_app_state(plain.encode()), sens_files=[path])
    out = dst.mergeFrom(src, transform=M)
    assert len(out) == 1 and out[0]["status"] == 0 and out[0]["resample"]["status"] == 0
    want = SR.permuted(scene_of(have), lambda v: (v + SR.SHIFT, np.ones(len(v), bool)))
    assert_is(dst.scene.state(), dict(positions=want[0], voxels=want[1]), "mergeFrom with a shift")
    with pytest.raises(ValueError):
        dst.mergeFrom(src, block_offset=(1, 0, 0), transform=M)
    # a streaming source with blocks on the host
    streamed = R.Reconstruction(R.read_app_state((MF_PARAMS + MF_STREAMING).encode()), sens_files=[path])
    assert streamed.run() == MF_N
    assert streamed.chunk_grid.getStatistics()["blocks"] > 0, "the source was meant to hold blocks on the host"
    fresh = R.Reconstruction(R.read_app_state(plain.encode()), sens_files=[path])
    before = fresh.scene.download()
    with pytest.raises(ValueError):
        fresh.mergeFrom(streamed, transform=M)
    assert raw_equal(before, fresh.scene.download())
