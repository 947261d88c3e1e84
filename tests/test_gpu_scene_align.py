"""The scene registration on the device (vh_align.hip) against the numpy restatement of its rule (tests/scene_align.py):
the per-voxel rule and the 29 integer totals bit for bit, the totals' independence of the order and of the table, one
step against the float64 step from the same totals, convergence on the analytic fixture against the truth and the
restatement, the gates, the scenes left as they were, and the refusals.  Scenes are crafted blocks merged into an empty
table."""

import ctypes as C

import numpy as np
import pytest

import crowded as CR
import scene_align as SA
import scene_resample as SR
from voxelhashing_amd import canonical, vhtypes as T

pytestmark = pytest.mark.gpu
V = T.SDF_BLOCK_VOXELS
F = np.float32
ROOMY = 1 << 14
VS = float(F(0.04))


@pytest.fixture(scope="module")
def E(vh):
    from voxelhashing_amd import engine
    return engine


def params(vs, buckets=ROOMY, pool=4096, limit=7):
    return T.make_hash_params(buckets, pool, float(F(vs)), max_collision_list=limit)


def pool_for(scene):
    return max(4096, 1 << int(len(scene[0]) + 64).bit_length())


def descs_of(positions):
    d = np.zeros(len(positions), T.DESC_DTYPE)
    d["pos"] = positions
    return d


def launcher_with(E, hp, scene):
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


def raw_equal(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a if k != "params")


def in_order_of(positions, descs):
    """for every position (the restatement's block order) its index in the device's list"""
    where = {tuple(int(c) for c in p): k for k, p in enumerate(descs["pos"])}
    return np.array([where[tuple(int(c) for c in p)] for p in positions])


MOTIONS = {
    "first": (SR.rotation((1, 2, 3), 0.6), (1.7, -2.3, 3.1)),
    "second": (SR.rotation((-2, 1, -0.5), -2.1), (-0.9, 1.4, -2.2)),
}
GENERAL = [("first", 1.0), ("second", 1.0), ("first", 2.0), ("second", 0.5)]  # (motion, vs_dst / vs_src), as test_gpu_scene_resample.py


@pytest.fixture(scope="module")
def S():
    """the crafted source: 64 blocks straddling the origin"""
    src = SR.crafted_source(11)
    assert len(src[0]) == 64
    return src


@pytest.fixture(scope="module")
def general(S):
    """the restatement of the rule under the general motions, computed once: {case: dict}"""
    out = {}
    for name, ratio in GENERAL:
        R, t = MOTIONS[name]
        vs_dst = float(F(VS * ratio))
        M = SR.rigid(R, t)
        b = SR.voxel_transforms(M, VS, vs_dst)[1]
        D = SA.crafted_destination(S[0], b, vs_dst, 17)
        pivot, radius = SA.pivot_and_radius(S[0], b)
        out[(name, ratio)] = dict(M=M, vs_dst=vs_dst, b=b, D=D, pivot=pivot, radius=radius, rule=SA.rule(D, S, b, pivot, 1.0 / radius, 2.0, VS, vs_dst))
    return out


@pytest.fixture(scope="module")
def room():
    """the analytic fixture at 4 cm voxels, and the restatement's registration from identity, computed once"""
    out = {}
    for ratio in (1.0, 2.0):
        dst, src, truth, vs_src, vs_dst = SA.fixture(vs_src=VS, ratio=ratio)
        ref = SA.align(dst, src, np.eye(4), vs_src, vs_dst)
        assert ref["status"] == T.ALIGN_CONVERGED and ref["iterations"] <= 8
        out[ratio] = dict(dst=dst, src=src, truth=truth, vs_src=vs_src, vs_dst=vs_dst, ref=ref, ref_error=SA.pose_error(ref["pose"], truth, vs_dst))
    return out


# ------------------------------------------------------------------------------------------------ 1. the rule

@pytest.mark.parametrize("case", GENERAL, ids=[f"{n}-{r}" for n, r in GENERAL])
def test_the_rule_bit_for_bit(E, S, general, case):
    c = general[case]
    want = c["rule"]
    reasons = np.bincount(want["reason"].ravel(), minlength=9)
    assert reasons[SA.KEPT] > 3000 and reasons[SA.CENTRE_TAP] > 100 and reasons[SA.OFFSET_TAP] > 100, reasons  # an unobserved tap
    assert reasons[SA.DST_BAND] > 100 and reasons[SA.GRADIENT] > 100 and reasons[SA.SRC_BAND] > 100 and reasons[SA.SRC_UNOBSERVED] > 100, reasons
    gS, gD = launcher_with(E, params(VS), S), launcher_with(E, params(c["vs_dst"], pool=pool_for(c["D"])), c["D"])
    db = E.resample_voxel_transforms(c["M"], VS, c["vs_dst"])[1]
    assert db.tobytes() == c["b"].tobytes()
    got = gD.align_rule(gS, c["b"], c["pivot"], 1.0 / c["radius"], band=2.0)
    o = in_order_of(S[0], got["descs"])
    assert np.array_equal(got["kept"][o], want["kept"]), f"kept flags differ at {(got['kept'][o] != want['kept']).sum()} voxels"
    for k in ("q", "e", "g", "terms"):
        assert np.ascontiguousarray(got[k][o]).tobytes() == want[k].tobytes(), f"{k} differs from the restatement"


def test_the_rule_drops_positions_from_2_to_the_24(E, S):
    shift = float(2 ** 24 - 12)
    M = SR.rigid(None, (shift * VS, 0.0, 0.0))
    b = SR.voxel_transforms(M, VS, VS)[1]
    assert b[0, 3] == F(shift)
    D = SR.random_blocks(SR.crafted_source(12)[0], 13)
    pivot = np.array([shift, 0.0, 0.0], F)
    want = SA.rule(D, S, b, pivot, 1.0 / 64.0, 2.0, VS, VS)
    reasons = np.bincount(want["reason"].ravel(), minlength=9)
    assert reasons[SA.Q_RANGE] > 1000 and reasons[SA.CENTRE_TAP] > 1000 and reasons[SA.KEPT] == 0, reasons
    gS, gD = launcher_with(E, params(VS), S), launcher_with(E, params(VS), D)
    got = gD.align_rule(gS, b, pivot, 1.0 / 64.0, band=2.0)
    assert not got["kept"].any() and not got["terms"].any() and not got["q"].any()


# ------------------------------------------------------------------------------------------------ 2. the totals

def one_step(gD, gS, M, pivot, radius, **kw):
    d_state, d_ticket, rc = gD.align_begin(gS, M, pivot, radius)
    assert rc == 0
    st, rc = gD.align_step(gS, d_state, d_ticket, **kw)
    assert rc == 0 and st["ticket"] == 0 and st["raised"] == 0 and not st["stripes"].any() and st["iterations"] == 1, st
    return st


@pytest.mark.parametrize("case", [GENERAL[0], GENERAL[3]], ids=["first-1.0", "second-0.5"])
def test_the_totals_bit_for_bit_in_any_order(E, S, general, case):
    c = general[case]
    want = SA.totals(c["rule"])
    assert want[T.ALIGN_COUNT] >> T.ALIGN_QUANTUM_LOG2 == c["rule"]["kept"].sum()
    gS, gD = launcher_with(E, params(VS), S), launcher_with(E, params(c["vs_dst"], pool=pool_for(c["D"])), c["D"])
    st = one_step(gD, gS, c["M"], c["pivot"], c["radius"])
    assert np.array_equal(st["totals"], want), (st["totals"], want)
    assert st["count"] == [int(c["rule"]["kept"].sum())]
    d_desc, n = gS.merge_gather()
    descs = d_desc.download(T.DESC_DTYPE, n, None)
    rng = np.random.default_rng(3)
    for order in (np.arange(n)[::-1], rng.permutation(n), rng.permutation(n)):
        again = one_step(gD, gS, c["M"], c["pivot"], c["radius"], descs=descs[order])
        assert np.array_equal(again["totals"], want), "the totals depend on the order of the list"
        assert again["raw"] == st["raw"], "the state depends on the order of the list"


def test_the_totals_of_a_source_on_a_crowded_table(E):
    pos = SR.ball_of_blocks(190)
    over, fullest = CR.assert_precondition_b(pos, 23, 256)
    assert over >= 3 and fullest > T.HASH_BUCKET_SIZE
    src = SR.random_blocks(pos, 31)
    M = SR.rigid(*MOTIONS["first"])
    b = SR.voxel_transforms(M, VS, VS)[1]
    D = SA.crafted_destination(src[0], b, VS, 19)
    pivot, radius = SA.pivot_and_radius(src[0], b)
    want = SA.totals(SA.rule(D, src, b, pivot, 1.0 / radius, 2.0, VS, VS))
    assert want[T.ALIGN_COUNT] >> T.ALIGN_QUANTUM_LOG2 > 3000
    gD = launcher_with(E, params(VS, pool=pool_for(D)), D)
    for buckets, limit in ((ROOMY, 7), (23, 256)):
        hp = params(VS, buckets, pool=CR.POOL, limit=limit)
        gS = launcher_with(E, hp, src)
        before = gS.download()
        if buckets != ROOMY:
            assert canonical.check_chains(before["hash"], hp)["listed"] >= 3, "the source's table was meant to hold collision lists"
        st = one_step(gD, gS, M, pivot, radius)
        assert np.array_equal(st["totals"], want), buckets
        assert raw_equal(before, gS.download())
    # ... and the destination on one: the crafted source, under no motion, against the lump
    S = SR.crafted_source(11)
    lump = SA.crafted_destination(None, None, VS, 23, positions=pos)
    bI = SR.voxel_transforms(np.eye(4), VS, VS)[1]
    pivot, radius = SA.pivot_and_radius(S[0], bI)
    want = SA.totals(SA.rule(lump, S, bI, pivot, 1.0 / radius, 2.0, VS, VS))
    assert want[T.ALIGN_COUNT] >> T.ALIGN_QUANTUM_LOG2 > 3000
    hp = params(VS, 23, pool=CR.POOL, limit=256)
    tight = launcher_with(E, hp, lump)
    assert canonical.check_chains(tight.download(False)["hash"], hp)["listed"] >= 3
    assert np.array_equal(one_step(tight, launcher_with(E, params(VS), S), np.eye(4), pivot, radius)["totals"], want)


# ------------------------------------------------------------------------------------------------ 3. one step

def test_one_step_against_the_float64_step(E, room):
    """The device solves by a Jacobi sweep and turns by its own sin / cos; the restatement by LAPACK and numpy's.  Both
    solves are backward stable, so the twists differ by at most some eps kappa max|y|: 100 * 2^-52 * kappa * max|y|, kappa
    as the state reports it.  The pose's entries are the twist's, scaled by at most 1 (1 / radius for the rotation, the
    voxel size for the translation): the same bound."""
    r = room[1.0]
    gS, gD = launcher_with(E, params(r["vs_src"]), r["src"]), launcher_with(E, params(r["vs_dst"]), r["dst"])
    b = SR.voxel_transforms(np.eye(4), r["vs_src"], r["vs_dst"])[1]
    pivot, radius = SA.pivot_and_radius(r["src"][0], b)
    assert np.array_equal(pivot, r["ref"]["pivot"]) and radius == r["ref"]["radius"]
    st = one_step(gD, gS, np.eye(4), pivot, radius)
    want_totals = SA.totals(SA.rule(r["dst"], r["src"], b, pivot, 1.0 / radius, 2.0, r["vs_src"], r["vs_dst"]))
    assert np.array_equal(st["totals"], want_totals)
    ref = SA.step(st["totals"], np.eye(4), pivot, 1.0 / radius, r["vs_dst"])
    assert st["status"] == ref["status"] == 0 and st["count"] == [ref["count"]]
    kappa = st["condition"][0]
    assert abs(kappa - ref["condition"]) <= 1e-5 * ref["condition"]
    assert st["sum_squares"] == [ref["sum_squares"]]
    bound = 100.0 * 2.0 ** -52 * kappa * np.abs(ref["y"]).max()
    print(f"kappa {kappa:.2f}, max|y| {np.abs(ref['y']).max():.4f}, bound {bound:.3e}: rotation off by {abs(st['step_rotation'][0] - ref['rotation']):.3e}, "
          f"translation by {abs(st['step_translation'][0] - ref['translation']):.3e}, pose by {np.abs(st['dst_from_src'] - ref['pose']).max():.3e}")
    assert abs(st["step_rotation"][0] - ref["rotation"]) <= np.sqrt(3.0) * bound
    assert abs(st["step_translation"][0] - ref["translation"]) <= np.sqrt(3.0) * bound
    assert np.abs(st["dst_from_src"] - ref["pose"]).max() <= bound
    # the matrices are the transform function's of the device's own pose, to the bit
    a2, b2 = SR.voxel_transforms(st["dst_from_src"], r["vs_src"], r["vs_dst"])
    assert st["src_vox_from_dst_vox"].tobytes() == a2.tobytes() and st["dst_vox_from_src_vox"].tobytes() == b2.tobytes()


# ------------------------------------------------------------------------------------------------ 4. convergence

def look_at(eye, target):
    """camera-to-world, row-major float32[16]: right, down, forward as columns (synth.orbit_pose's convention)"""
    f = np.asarray(target, np.float64) - np.asarray(eye, np.float64)
    f /= np.linalg.norm(f)
    right = np.cross([0.0, 1.0, 0.0], f)
    right /= np.linalg.norm(right)
    down = np.cross(f, right)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, down, f, eye
    return m.astype(F).reshape(16)


@pytest.mark.parametrize("ratio", [1.0, 2.0])
def test_convergence_on_the_fixture(E, room, ratio):
    """from identity to the 2 degree / 1.9 voxel motion: converged within the restatement's iterations plus one, and at
    most twice the restatement's own error plus 1e-3 voxel and 1e-3 degree from the truth; merged under the result, the
    destination's ray cast has no hole where it had none before"""
    r = room[ratio]
    hp_d = params(r["vs_dst"])
    src, dst = scene_with(E, params(r["vs_src"]), r["src"]), scene_with(E, hp_d, r["dst"])
    got = dst.alignScene(src)
    deg, vox = SA.pose_error(got["dst_from_src"], r["truth"], r["vs_dst"])
    ref_deg, ref_vox = r["ref_error"]
    print(f"device: {got['iterations']} steps, {deg:.5f} degree, {vox:.5f} voxel; restatement: {r['ref']['iterations']} steps, {ref_deg:.5f} degree, "
          f"{ref_vox:.5f} voxel; counts {got['count']}, conditions {[round(c, 1) for c in got['condition']]}")
    assert got["status"] == T.ALIGN_CONVERGED, got["status"]
    assert got["iterations"] <= r["ref"]["iterations"] + 1
    assert deg <= 2.0 * ref_deg + 1e-3 and vox <= 2.0 * ref_vox + 1e-3
    assert np.array_equal(got["pivot"], r["ref"]["pivot"]) and 1.0 / got["inv_radius"] == r["ref"]["radius"]
    # the merge under the result
    _, cp, _ = CR.config("B", ROOMY)
    rp = T.make_raycast_params(hp_d, cp)
    unit = 32.0 * r["vs_src"]
    pose = look_at(np.array([0.75, 0.7, 0.75]) * unit, np.array([0.12, 0.06, -0.2]) * unit)
    ray = E.CUDARayCastSDF(rp)

    def depth():
        dst.setLastRigidTransformAndCompactify(pose, cp)
        ray.render(dst.getHashData(), dst.getHashParams(), cp, pose)
        return ray.download()["depth"]

    before = depth()
    seen = before != -np.inf
    assert seen.sum() > 0.5 * seen.size, f"the camera was meant to see the room: {seen.sum()} of {seen.size} pixels"
    merged = dst.mergeSceneTransformed(src, got["dst_from_src"])
    assert merged["status"] == 0 and merged["left_out"] == 0 and merged["combined"] > 10000
    after = depth()
    assert (after[seen] != -np.inf).all(), f"{(after[seen] == -np.inf).sum()} holes where the destination had none"


# ------------------------------------------------------------------------------------------------ 5. the gates

def test_a_lone_plane_is_refused_and_disjoint_scenes_are_too_few(E):
    plane = SA.plane_field((0.3, -0.5, 0.81), 0.002)
    hp = params(VS)
    dst_s = SA.field_scene(VS, np.eye(4), side=4, field=plane, scale=1.0)
    src_s = SA.field_scene(VS, SR.rigid(None, (0.4 * VS, 0.0, 0.0)), side=4, field=plane, scale=1.0)
    dst, src = scene_with(E, hp, dst_s), scene_with(E, hp, src_s)
    guess = SR.rigid(SR.rotation((1, 2, 3), 0.01), (0.3 * VS, 0.0, -0.2 * VS))
    got = dst.alignScene(src, guess)
    assert got["status"] == T.ALIGN_ILL_CONDITIONED and got["iterations"] == 1 and got["count"][0] > 1000, got
    assert not got["condition"][0] <= 1e4
    assert got["dst_from_src"].tobytes() == np.ascontiguousarray(guess, np.float64).tobytes(), "a refused step moved the pose"
    far = scene_with(E, hp, SA.field_scene(VS, np.eye(4), side=2, field=plane, scale=1.0, corner=40))
    got = far.alignScene(src, guess)
    assert got["status"] == T.ALIGN_TOO_FEW and got["count"] == [0] and got["dst_from_src"].tobytes() == np.ascontiguousarray(guess, np.float64).tobytes()
    empty = E.CUDASceneRepHashSDF(hp, CR.options())
    assert dst.alignScene(empty)["status"] == T.ALIGN_TOO_FEW and empty.alignScene(src)["status"] == T.ALIGN_TOO_FEW


def test_a_guess_far_off_never_converges_to_a_wrong_pose(E, room):
    r = room[1.0]
    src, dst = scene_with(E, params(r["vs_src"]), r["src"]), scene_with(E, params(r["vs_dst"]), r["dst"])
    t = np.array([2.0, -1.0, 1.5])
    guess = r["truth"].copy()
    guess[:3, 3] += t / np.linalg.norm(t) * 20.0 * r["vs_dst"]
    got = dst.alignScene(src, guess)
    deg, vox = SA.pose_error(got["dst_from_src"], r["truth"], r["vs_dst"])
    print(f"20 voxels off: status {got['status']}, {got['iterations']} steps, {deg:.4f} degree and {vox:.4f} voxel from the truth")
    assert got["status"] != 0 or got["iterations"] == 30, "neither a verdict nor the iterations spent"
    if got["status"] & T.ALIGN_CONVERGED:
        assert deg <= 0.02 and vox <= 0.05, "converged, says the status, at a wrong pose"
    else:
        assert not got["converged"]


def test_a_launch_after_convergence_changes_nothing(E, room):
    r = room[1.0]
    gS, gD = launcher_with(E, params(r["vs_src"]), r["src"]), launcher_with(E, params(r["vs_dst"]), r["dst"])
    d_state, d_ticket, rc = gD.align_begin(gS, np.eye(4), r["ref"]["pivot"], r["ref"]["radius"])
    assert rc == 0
    st, rc = gD.align_step(gS, d_state, d_ticket, steps=r["ref"]["iterations"] + 1)
    assert rc == 0 and st["status"] == T.ALIGN_CONVERGED and st["ticket"] == 0 and not st["stripes"].any()
    again, rc = gD.align_step(gS, d_state, d_ticket, steps=2)
    assert rc == 0 and again["raw"] == st["raw"] and again["ticket"] == 0


# ------------------------------------------------------------------------------------------------ 6. read-only

def test_both_scenes_are_left_as_they_were(E, room):
    r = room[1.0]
    hp_s, hp_d = params(r["vs_src"]), params(r["vs_dst"])
    src, dst = scene_with(E, hp_s, r["src"]), scene_with(E, hp_d, r["dst"])
    before = [s.download() for s in (src, dst)]
    states = [s.state() for s in (src, dst)]
    got = dst.alignScene(src)
    assert got["converged"]
    for s, raw, st, hp in zip((src, dst), before, states, (hp_s, hp_d)):
        assert raw_equal(raw, s.download()), "the registration wrote to a scene"
        now = s.state()
        assert now["positions"].tobytes() == st["positions"].tobytes() and now["voxels"].tobytes() == st["voxels"].tobytes()
        canonical.check_chains(s.download(False)["hash"], s.getHashParams())


# ------------------------------------------------------------------------------------------------ 7. refusals

def test_refusals_change_nothing(E, S):
    hp = params(VS)
    D = SR.random_blocks(SR.crafted_source(12, corner=(0, -2, -2))[0], 13)
    src, dst = scene_with(E, hp, S), scene_with(E, hp, D)
    before = [s.download() for s in (src, dst)]
    R = SR.rotation((1, 2, 3), 0.6)
    good = SR.rigid(R, (0.4, -0.2, 0.3))

    def refused(call):
        with pytest.raises(Exception) as err:
            call()
        assert getattr(err.value, "code", None) == 4, err.value
        for s, raw in zip((src, dst), before):
            assert raw_equal(raw, s.download()), "a refused registration changed a scene"

    refused(lambda: dst.alignScene(dst, good))
    scaled, sheared, nan = (good.copy() for _ in range(3))
    scaled[:3, :3] *= 1.01
    sheared[0, 1] += 0.01
    nan[1, 3] = np.nan
    for M in (scaled, sheared, nan):
        refused(lambda: dst.alignScene(src, M))
    coarse = scene_with(E, params(F(2.5) * F(VS)), S)
    refused(lambda: dst.alignScene(coarse, good))  # a ratio of 2.5
    for bad in (dict(band=np.nan), dict(band=0.0), dict(band=4.5), dict(cond_thres=np.inf), dict(cond_thres=-1.0), dict(rot_thres=np.nan),
                dict(rot_thres=0.0), dict(trans_thres=np.inf), dict(trans_thres=-1e-3), dict(min_count=0), dict(max_iterations=0),
                dict(max_iterations=T.ALIGN_MAX_ITERATIONS + 1)):
        refused(lambda: dst.alignScene(src, good, **bad))
    # a list longer than the overflow bound: VH_ALIGN_MOST_BLOCKS + 1 blocks, refused before anything is read
    gS, gD = launcher_with(E, hp, S), launcher_with(E, hp, D)
    d_state, d_ticket, rc = gD.align_begin(gS, good, (0.0, 0.0, 0.0), 64.0)
    assert rc == 0
    fresh = gD.align_state(d_state, d_ticket)
    long_list = E.DeviceBuffer(16 * (T.ALIGN_MOST_BLOCKS + 1))
    st, rc = gD.align_step(gS, d_state, d_ticket, descs=long_list, n=T.ALIGN_MOST_BLOCKS + 1)
    assert rc == 4 and st["status"] == T.ALIGN_TOO_MANY and st["iterations"] == 0 and st["ticket"] == 0
    assert st["dst_from_src"].tobytes() == fresh["dst_from_src"].tobytes() and not st["totals"].any()
    st, rc = gD.align_step(gS, d_state, d_ticket)  # the state is refused for good
    assert rc == 0 and st["status"] == T.ALIGN_TOO_MANY and st["iterations"] == 0
    # the launcher's own refusals
    d_state, d_ticket, rc = gD.align_begin(gS, good, (0.0, 0.0, 0.0), 48.0)  # a radius that is no power of two
    assert rc == 4
    assert gD.align_begin(gS, scaled, (0.0, 0.0, 0.0), 64.0)[2] == 4
    d_state, d_ticket, rc = gD.align_begin(gS, good, (0.0, 0.0, 0.0), 64.0)
    for bad in (dict(band=5.0), dict(band=np.nan), dict(cond_thres=np.inf), dict(rot_thres=0.0), dict(trans_thres=np.nan)):
        st, rc = gD.align_step(gS, d_state, d_ticket, **bad)
        assert rc == 4 and st["iterations"] == 0 and st["status"] == 0, bad
    for s, raw in zip((src, dst), before):
        assert raw_equal(raw, s.download())


# ------------------------------------------------------------------------------------------------ 8. Reconstruction

def test_reconstruction_align_to_and_merge_from(E, oracle_lib, tmp_path):
    """Reconstruction.alignTo and mergeFrom(align=True) on the fixture at 2 cm voxels: the transform found is the scene
    level's, the merge runs under it, and a guess that does not converge merges nothing"""
    from test_gpu_scene_merge import MF_H, MF_PARAMS, MF_W
    from voxelhashing_amd import reconstruction as R, sensor_data as SD, synth
    cp = T.make_depth_camera_params(MF_W, MF_H)
    sd = SD.SensorData.create((MF_W, MF_H), (MF_W, MF_H), SD.make_intrinsic_matrix(cp.fx, cp.fy, cp.mx, cp.my), depth_shift=1000.0,
                              sensor_name="synthetic S3", depth_type=SD.TYPE_ZLIB_USHORT)
    p = synth.orbit_pose(0, n_frames=400)
    d, c = oracle_lib.synth_frame(synth.S3_SPHERES, 0, p, cp)
    mm = np.where(np.isfinite(d), np.floor(1000.0 * d.astype(np.float64) + 0.5), 0).astype(np.uint16)
    rgb = np.clip(np.where(np.isfinite(c[..., :3]), c[..., :3], 0) * 255.0, 0, 255).astype(np.uint8)
    sd.addFrame(rgb, mm, p, 100, 200)
    path = str(tmp_path / "one.sens")
    sd.saveToFile(path)
    plain = MF_PARAMS + "s_streamingEnabled = false;\n"
    dst_s, src_s, truth, vs_src, vs_dst = SA.fixture(vs_src=0.02)
    dst, src = (R.Reconstruction(R.read_app_state(plain.encode()), sens_files=[path]) for _ in range(2))
    for rec, scene in ((dst, dst_s), (src, src_s)):
        got = rec.scene.mergeBlocks(descs_of(scene[0]), scene[1])
        assert (got["allocated"], got["left_out"], got["status"]) == (512, 0, 0), got
    found = src.alignTo(dst)
    assert found["converged"] and found["iterations"] <= 5
    deg, vox = SA.pose_error(found["dst_from_src"], truth, vs_dst)
    assert deg <= 0.02 and vox <= 0.05, (deg, vox)
    assert src.alignTo(dst, guess=found["dst_from_src"], max_iterations=3)["converged"]
    before = dst.scene.download()
    off = truth.copy()
    off[:3, 3] += np.array([20.0, 0.0, 0.0]) * vs_dst
    with pytest.raises(ValueError):
        dst.mergeFrom(src, transform=off, align=True)
    assert raw_equal(before, dst.scene.download()), "a registration that did not converge merged something"
    out = dst.mergeFrom(src, align=True)
    assert len(out) == 2 and out[0]["status"] == 0 and out[0]["combined"] > 10000
    assert out[1]["align"]["dst_from_src"].tobytes() == found["dst_from_src"].tobytes()
