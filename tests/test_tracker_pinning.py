"""Both camera trackers' per-pixel rules against the reference's own kernels, compiled for the CPU (oracle/_ref/libvh_ref.so
through oracle/reference.py: projectiveCorrespondences, buildLinearSystem and computeNormalEquations, the build kernels
with one thread per block so that an output row is one lane's in-order window sum; oracle/ref/vh_ref_track.cpp).

oracle/icp.py (depth tracker) and tests/rgbd_icp.py (RGB-D tracker) restate those kernels in numpy and the HIP kernels are
held to them; these tests close the other link.  Float32 arithmetic with one rounding per operation on both sides and
sqrt as the only function, so every comparison is bit for bit (after `+ 0.0`: a sum that starts from +0 and a product
never added differ in the sign of a zero).  Only the RGB-D rows at angles other than 0 go through sin and cos (host libm
there, numpy here), and are held to a measured bound.

Inputs: the sphere scene and the textured plane at 202x154 with their pyramids (101x77, 50x38), and the crafted 37x29
maps of tests/tracker_edges.py, under the cameras `tum` and `offcentre` (fx != fy, principal point off the centre) and
under the identity, a translation and a general small motion.  The last tests hold tests/icp_reference.py, the float64
restatement of the 6x6 solve, to the float32 Eigen the reference vendors and runs.
"""
import numpy as np
import pytest

import camera_models as CM
import icp_reference as S
import rgbd_icp as G
import tracker_edges as E
from oracle import icp
from oracle import oracle as O
from oracle import reference as R
from test_camera_tracking import TRACK_SPHERES, maps_for
from test_icp_solve import SYSTEMS, terms_of
from test_rgbd_tracking import all_colour_settings, plane_maps
from voxelhashing_amd import synth

pytestmark = pytest.mark.skipif(not R.available(), reason="oracle/_ref/libvh_ref.so is not built (build() makes it "
                                "where the reference tree is present)")

f32 = np.float32
MINF = f32(-np.inf)
CAMERAS = ("tum", "offcentre")
W0, H0 = 202, 154
DIST_THRES, NORMAL_THRES = 0.15, 0.97


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    """bit for bit, the sign of a zero aside"""
    return np.array_equal(bits(np.asarray(a, np.float32) + f32(0.0)), bits(np.asarray(b, np.float32) + f32(0.0)))


def general_motion():
    return icp.delinearize(np.array([0.004, -0.003, 0.002, 0.003, -0.001, 0.002], np.float32), 1.0, 1.0)


def deltas():
    t = np.eye(4, dtype=np.float32)
    t[:3, 3] = [0.004, -0.002, 0.001]
    return {"identity": np.eye(4, dtype=np.float32), "translation": t, "general": general_motion()}


_CACHE = {}


def sphere_levels(cam):
    """[(input, input normals, target, target normals)] for levels 0, 1, 2 and the full-resolution camera"""
    if ("s", cam) not in _CACHE:
        O.build()
        cp = CM.camera(cam, W0, H0)
        A = CM.aim(cp)
        poses = [(np.asarray(synth.orbit_pose(k, n_frames=400), np.float64).reshape(4, 4) @ A).astype(np.float32).reshape(16)
                 for k in range(3)]
        _, c, n = maps_for(O, TRACK_SPHERES, poses[2], cp)
        _, tc, tn = maps_for(O, TRACK_SPHERES, poses[1], cp)
        ins, tgs = [(c, n)] + icp.pyramid(c, 3), [(tc, tn)] + icp.pyramid(tc, 3)
        _CACHE["s", cam] = [ins[lv] + tgs[lv] for lv in range(3)], cp
    return _CACHE["s", cam]


def plane_levels(cam):
    if ("p", cam) not in _CACHE:
        O.build()
        cp = CM.camera(cam, W0, H0)
        _, _, (i, inn, ic), (m, mn, mc) = plane_maps(cp, 0.0, 0.02)
        _CACHE["p", cam] = G.pyramids(i, inn, ic, m, mn, mc, 3), cp
    return _CACHE["p", cam]


def crafted_depth(cam, lf):
    cp = CM.camera(cam, E.W * lf, E.H * lf)
    return E.depth_maps(cp, lf, DIST_THRES, NORMAL_THRES), cp


def depth_cases(cam):
    """(what, input, input normals, target, target normals, levelFactor, full-resolution camera, lane window)"""
    levels, cp = sphere_levels(cam)
    for lv, maps in enumerate(levels):
        assert maps[0].shape[:2] == (H0 >> lv, W0 >> lv)
        yield (f"spheres level {lv}",) + maps + (float(2 ** lv), cp, (12, 3, 1)[lv])
    for lf in (1, 2, 4):
        m, cp = crafted_depth(cam, lf)
        yield (f"crafted levelFactor {lf}", m["inp"], m["inp_n"], m["tgt"], m["tgt_n"], float(lf), cp, 12)


# ------------------------------------------------------------------------------------------------- the depth tracker

@pytest.mark.parametrize("cam", CAMERAS)
def test_correspondences(cam):
    for what, i, inn, t, tn, lf, cp, _ in depth_cases(cam):
        for name, d in deltas().items():
            wc, wn = icp.correspondences(i, inn, t, tn, d.reshape(16), DIST_THRES, NORMAL_THRES, lf, cp)
            rc, rn = R.icp_correspondences(i, inn, t, tn, d.reshape(16), DIST_THRES, NORMAL_THRES, lf, cp)
            assert (rc[..., 0] != MINF).sum() > 0.1 * rc.shape[0] * rc.shape[1], (what, name)
            assert np.array_equal(bits(wc), bits(rc)), (what, name, "positions")
            # the pair weight included: max(0.0, 0.5f * ...) takes nvcc's max(double, float), whose result converted back
            # to float is the float maximum
            assert np.array_equal(bits(wn), bits(rn)), (what, name, "normals and pair weight")


@pytest.mark.parametrize("cam", CAMERAS)
def test_depth_rows_and_lane_sums(cam):
    for what, i, inn, t, tn, lf, cp, window in depth_cases(cam):
        for name, d in deltas().items():
            rc, rn = R.icp_correspondences(i, inn, t, tn, d.reshape(16), DIST_THRES, NORMAL_THRES, lf, cp)
            terms = icp.pixel_terms(i, rc, rn, d.reshape(16), dtype=np.float32)
            assert terms[:, 29].sum() == (rc[..., 0] != MINF).sum()
            assert same_bits(terms, R.icp_lane_sums(i, rc, rn, d.reshape(16), 1)), (what, name, "per pixel")
            for win in {window, 12}:
                assert same_bits(icp.lane_sums(terms, win), R.icp_lane_sums(i, rc, rn, d.reshape(16), win)), (what, name, win)


def paired_with(rc, tgt, x, y):
    """the target pixel whose position the reference wrote into correspondence (x, y), or None"""
    if rc[y, x, 0] == MINF:
        return None
    hit = np.nonzero(np.all(bits(tgt) == bits(rc[y, x]), axis=-1))
    assert len(hit[0]) == 1, "the crafted targets are all different"
    return int(hit[1][0]), int(hit[0][0])


@pytest.mark.parametrize("lf", [1, 2, 4])
@pytest.mark.parametrize("cam", CAMERAS)
def test_crafted_depth_edge_classes_occur(cam, lf):
    """each rule the crafted map was made for shows in the REFERENCE's output, under the identity"""
    m, cp = crafted_depth(cam, lf)
    eye = np.eye(4, dtype=np.float32)
    rc, rn = R.icp_correspondences(m["inp"], m["inp_n"], m["tgt"], m["tgt_n"], eye.reshape(16), DIST_THRES, NORMAL_THRES, float(lf), cp)
    rows = R.icp_lane_sums(m["inp"], rc, rn, eye.reshape(16), 1)
    cls = m["classes"]
    got = {name: [paired_with(rc, m["tgt"], x, y) for x, y in c["pixels"]] for name, c in cls.items()}
    screen = lambda x, y: (m["inp"][y, x, 0].astype(np.float64) * cp.fx / m["inp"][y, x, 2] + cp.mx + 0.5,
                           m["inp"][y, x, 1].astype(np.float64) * cp.fy / m["inp"][y, x, 2] + cp.my + 0.5)
    # a projection in (-1, 0) truncates to column / row 0 and pairs there
    assert -1 < screen(5, 3)[0] < 0 and got["neg_x"] == [(0, 3)]
    assert -1 < screen(7, 5)[1] < 0 and got["neg_y"] == [(7, 0)]
    # the last column and row pair; the first screen position past them does not
    assert got["last_col"] == [(E.W - 1, 4)] and got["last_row"] == [(13, E.H - 1)]
    assert got["past_the_image"] == [None, None]
    # z = 0 pairs with nothing; z < 0 pairs (the reference's z test is commented out)
    assert got["z_zero"] == [None] and got["z_negative"] == [(21, 10)] and m["inp"][8, 19, 2] == -1.0
    assert got["target_half_valid"] == [None, None] and got["input_invalid"] == [None, None]
    # at the thresholds: <= and >= hold with equality, and fail one ulp further
    assert got["dist_at_thres"] == [(27, 14)] and got["dist_one_ulp_above"] == [None]
    assert got["normal_at_thres"] == [(31, 16)] and got["normal_one_ulp_below"] == [None]
    # beyond the sensor's depth range the weight clamps to 0, and the build step still counts the row
    assert got["weight_zero"] == [(4, 20)] and rn[20, 4, 3] == 0.0 and rows[20 * E.W + 4, 29] == 1.0 and rows[20 * E.W + 4, 28] == 0.0
    # every untouched pixel pairs with itself: screenPos / levelFactor drops the fraction of an odd coordinate
    touched = {p for c in cls.values() for p in c["pixels"]} | {(21, 10)}
    own = [(x, y) for y in range(E.H) for x in range(E.W) if (x, y) not in touched]
    assert len(own) == 1055 and all(paired_with(rc, m["tgt"], x, y) == (x, y) for x, y in own)
    assert int((rc[..., 0] != MINF).sum()) == 1063 and int(rows[:, 29].sum()) == 1063


# ------------------------------------------------------------------------------------------------- the RGB-D tracker

def rgbd_cases(cam):
    """(what, the six maps, level parameters, lane window)"""
    ts = all_colour_settings()
    pyr, cp = plane_levels(cam)
    for lv, maps in enumerate(pyr):
        yield f"plane level {lv}", maps, G.level_params(ts, lv, cp), G.window(lv)
    prm = G.level_params(ts, 0, CM.camera(cam, E.W, E.H))
    m = E.rgbd_maps(prm)
    yield "crafted", (m["inp"], m["inp_n"], m["inp_i"], m["tgt"], m["tgt_n"], m["tgt_iad"]), prm, 12


def restated_rows(maps, angles, trans, prm):
    dterm, cterm, dmask, cmask = G.pixel_terms(*maps, angles, trans, prm)
    return dterm, cterm, dmask.astype(np.float32) + cmask.astype(np.float32)


@pytest.mark.parametrize("cam", CAMERAS)
def test_rgbd_rows_at_angles_zero(cam):
    """sin(0) and cos(0) are exact in every libm: bit for bit"""
    zero = np.zeros(3, np.float32)
    for what, maps, prm, window in rgbd_cases(cam):
        for trans in (zero, np.array([0.006, 0.003, 0.001], np.float32)):
            dterm, cterm, made = restated_rows(maps, zero, trans, prm)
            ref = R.icp_rgbd_lane_sums(*maps, zero, trans, prm, 1)
            assert made.sum() > 0.3 * len(made), (what, trans)
            assert np.array_equal(ref[:, 29], made), (what, trans, "which rows are made")
            assert same_bits(G.lane_sums(dterm, cterm, 1), ref), (what, trans, "per pixel")
            for win in {window, 12}:
                assert same_bits(G.lane_sums(dterm, cterm, win), R.icp_rgbd_lane_sums(*maps, zero, trans, prm, win)), (what, trans, win)


# Measured here: the six sin / cos values come from the host libm on one side and from numpy's
# float32 functions on the other.  At `small` and `far` the two libraries return the same bits for all six and the rows
# agree bit for bit; at `far, a sine differs` sin(3.1372294) differs in its last bit, and the largest
# |reference - restatement| / sum |per-pixel products| over the 29 value terms, both cameras and all four inputs, is
# 8.36e-8 (offcentre, crafted map).  Asserted: twice that.
RGBD_TRIG_MEASURED = 8.36e-8


def far_euler_branch(tx=0.006, ty=0.002, rz_deg=-0.4):
    """the linearisation point test_gpu_rgbd_build_step_matches_restatement uses: eulerAngles near (pi, -pi, pi)"""
    d = np.asarray(G.plane_pose(tx, ty, rz_deg=rz_deg), np.float32).reshape(4, 4)
    return G.euler_angles_zyx(d[:3, :3]), d[:3, 3].copy()


@pytest.mark.parametrize("cam", CAMERAS)
def test_rgbd_rows_at_general_angles(cam):
    small = (np.array([0.004, -0.003, 0.002], np.float32), np.array([0.006, 0.003, 0.001], np.float32))
    far, far_b = far_euler_branch(), far_euler_branch(0.004, -0.002, -0.25)
    assert np.all(np.abs(np.abs(far[0]) - np.pi) < 0.02) and np.all(np.abs(np.abs(far_b[0]) - np.pi) < 0.02)
    for what, maps, prm, window in rgbd_cases(cam):
        for name, (angles, trans) in (("small", small), ("far", far), ("far, a sine differs", far_b)):
            dterm, cterm, made = restated_rows(maps, angles, trans, prm)
            ref = R.icp_rgbd_lane_sums(*maps, angles, trans, prm, 1)
            assert np.array_equal(ref[:, 29], made), (what, name, "which rows are made", int((ref[:, 29] != made).sum()))
            mine = G.lane_sums(dterm, cterm, 1).astype(np.float64)
            scale = (np.abs(dterm.astype(np.float64)) + np.abs(cterm.astype(np.float64))).sum(0)[:29]
            err = np.abs(mine - ref).sum(0)[:29]
            worst = float((err / np.maximum(scale, 1e-300)).max())
            print(f"rgbd rows, {cam}, {what}, {name}: |reference - restatement| / sum |products| = {worst:.3g}")
            assert worst <= 2 * RGBD_TRIG_MEASURED, (what, name, worst)


@pytest.mark.parametrize("cam", CAMERAS)
def test_crafted_rgbd_edge_classes_occur(cam):
    prm = G.level_params(all_colour_settings(), 0, CM.camera(cam, E.W, E.H))
    m = E.rgbd_maps(prm)
    maps = (m["inp"], m["inp_n"], m["inp_i"], m["tgt"], m["tgt_n"], m["tgt_iad"])
    zero = np.zeros(3, np.float32)
    ref = R.icp_rgbd_lane_sums(*maps, zero, zero, prm, 1)
    rows = {name: [int(ref[y * E.W + x, 29]) for x, y in c["pixels"]] for name, c in m["classes"].items()}
    assert rows["input_invalid"] == [0, 0, 0]
    assert rows["z_not_positive"] == [0, 0]                      # pProjTrans(2) <= 0, also onto a target holding the same point
    assert rows["taps_1_minf"] == [2] and rows["taps_2_minf"] == [2] and rows["taps_3_minf"] == [2] and rows["taps_4_minf"] == [0]
    assert rows["taps_over_the_border"] == [2, 2, 2, 2]
    assert rows["colour_at_thres"] == [2] and rows["colour_one_ulp_above"] == [1]      # a depth row without a colour row
    assert rows["gradient_at_min"] == [1] and rows["gradient_one_ulp_above"] == [2]    # `>`: at the minimum there is no colour row
    # the geometric gate, which this kernel states for itself: u + 0.5 / v + 0.5 in (-1, 0) truncate onto column / row 0
    # (the one on row 0 makes its depth row only), the last column and row make rows, the first position past them none
    u = m["inp"][3, 5, 0].astype(np.float64) * prm["fx"] / m["inp"][3, 5, 2] + prm["mx"] + 0.5
    v = m["inp"][5, 7, 1].astype(np.float64) * prm["fy"] / m["inp"][5, 7, 2] + prm["my"] + 0.5
    assert -1 < u < 0 and -1 < v < 0 and rows["neg_x_neg_y"] == [2, 1]
    assert rows["last_col_last_row"] == [2, 2] and rows["past_the_image"] == [0, 0]
    # <= distThres and >= normalThres hold with equality and fail one ulp further
    assert rows["dist_at_thres"] == [2] and rows["dist_one_ulp_above"] == [0]
    assert rows["normal_at_thres"] == [2] and rows["normal_one_ulp_below"] == [0]
    # under a small rotation ROld turns the input normals: about +y it lifts both normal pixels over the threshold, about
    # -y it drops both below it (a kernel that left the normal unrotated would keep [2] and [0])
    for beta, want in ((0.003, [2, 2]), (-0.003, [0, 0])):
        turned = R.icp_rgbd_lane_sums(*maps, np.array([0.004, beta, 0.002], np.float32), zero, prm, 1)
        assert [int(turned[16 * E.W + x, 29]) for x in (31, 33)] == want, beta
    # pixels with no row, a depth row only, both rows
    assert tuple(int((ref[:, 29] == k).sum()) for k in range(3)) == {"tum": (19, 6, 1048), "offcentre": (18, 6, 1049)}[cam]
    # the reverse, a colour row without a depth row, cannot be: the colour row's condition repeats the depth row's.  The
    # restatement's two masks, which add up to the reference's count on every pixel, say which single rows are which.
    _, _, dmask, cmask = G.pixel_terms(*maps, zero, zero, prm)
    assert np.array_equal(ref[:, 29], dmask.astype(np.float32) + cmask.astype(np.float32)) and not np.any(cmask & ~dmask)
    # the intensity those exact pixels saw is the texel's own: dI = colorThres exactly makes the colour weight 0, so the
    # pixel's summed weight is the depth row's alone although it made two rows
    x, y = m["classes"]["colour_at_thres"]["pixels"][0]
    xa, ya = m["classes"]["colour_one_ulp_above"]["pixels"][0]
    assert ref[y * E.W + x, 28] == ref[ya * E.W + xa, 28]


def test_depth_and_rgbd_kernels_share_one_process():
    """the two build-system units define helpers of one name differently (oracle/ref/Makefile renames them per unit): each
    must run its own.  Depth, RGB-D, depth again, RGB-D again, each held to its restatement.  This is a check of the
    result, NOT the proof that the rename rule works: at -O2 the compiler inlines every call of those helpers, so the
    library passes this test without the renames too (tried).  What it would catch is a build in which the calls are
    not inlined and the linker's one copy serves both kernels."""
    cam = "tum"
    what, i, inn, t, tn, lf, cp, _ = next(c for c in depth_cases(cam) if c[0] == "crafted levelFactor 1")
    d = general_motion()
    rc, rn = R.icp_correspondences(i, inn, t, tn, d.reshape(16), DIST_THRES, NORMAL_THRES, lf, cp)
    _, maps, prm, _ = next(c for c in rgbd_cases(cam) if c[0] == "crafted")
    zero = np.zeros(3, np.float32)
    a1 = R.icp_lane_sums(i, rc, rn, d.reshape(16), 12)
    b1 = R.icp_rgbd_lane_sums(*maps, zero, zero, prm, 12)
    a2 = R.icp_lane_sums(i, rc, rn, d.reshape(16), 12)
    b2 = R.icp_rgbd_lane_sums(*maps, zero, zero, prm, 12)
    assert np.array_equal(bits(a1), bits(a2)) and np.array_equal(bits(b1), bits(b2))
    assert a1[:, 29].sum() > 900 and b1[:, 29].sum() > 900 and not np.array_equal(a1, b1)
    assert same_bits(a1, icp.lane_sums(icp.pixel_terms(i, rc, rn, d.reshape(16), dtype=np.float32), 12))
    dterm, cterm, _ = restated_rows(maps, zero, zero, prm)
    assert same_bits(b1, G.lane_sums(dterm, cterm, 12))


# ------------------------------------------------------------------------------------------------- the 6x6 solve

# Measured against the compiled float32 Eigen on the SYSTEMS of tests/test_icp_solve.py: the float64
# restatement's x differs from JacobiSVD<Matrix6x6f>::solve's by at most SOLVE_X_MEASURED * cond * max|x| per component,
# its condition number s_0 / s_5 by SOLVE_COND_MEASURED * cond relative where s_5 is resolved (cond < 1e6) -- float32's
# absolute error on s_5 is a fraction of 2^-24 s_0, which is that fraction times cond of s_5 itself.  Asserted: twice that.
SOLVE_X_MEASURED = 3.72e-8
SOLVE_COND_MEASURED = 2.22e-8


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_solve_restatement_against_eigen(name):
    A, b = SYSTEMS[name]()
    t = terms_of(A, b)
    x, s, rank, cond = S.jacobi_svd_solve(*S.system(t))
    ex, econd, erank, ezero = R.icp_solve(t)
    assert rank == erank and S.is_zero(t) == ezero and not ezero, (name, rank, erank)
    live = s[:rank]
    kappa = live[0] / live[-1]  # the conditioning of the part that is solved
    err = float(np.abs(ex.astype(np.float64) - x).max() / (kappa * np.abs(x).max()))
    print(f"solve {name}: rank {rank}, cond {cond:.6g} / {econd:.6g}, |x - x_eigen| / (kappa max|x|) = {err:.3g}")
    assert err <= 2 * SOLVE_X_MEASURED, (name, err)
    if np.isinf(cond):
        assert np.isinf(econd), name
    elif cond < 1e6:
        cerr = abs(float(econd) / cond - 1.0) / cond
        print(f"solve {name}: condition relative difference / cond = {cerr:.3g}")
        assert cerr <= 2 * SOLVE_COND_MEASURED, (name, cerr)
    else:  # s_5 of a singular matrix is rounding noise on both sides
        assert econd > 1e6, (name, econd)


def test_solve_decisions_against_eigen():
    """isZero at its boundary, a NaN entry, exact zeros; AngleAxisf(R).angle() against both restatements"""
    eps = f32(1e-5)
    t = np.zeros(30, np.float32)
    assert R.icp_solve(t)[3] and S.is_zero(t)
    t[:21] = -eps * f32(0.5)
    t[7] = -eps
    assert R.icp_solve(t)[3] and S.is_zero(t)
    t[7] = -np.nextafter(eps, f32(1))
    assert not R.icp_solve(t)[3] and not S.is_zero(t)
    t[7] = eps
    t[3] = np.nan
    assert not R.icp_solve(t)[3] and not S.is_zero(t)
    # A NaN system is where the restatement leaves Eigen ON PURPOSE (fenced defects), so its rank and
    # x are not among the equalities above.  The compiled Eigen never looks at a NaN entry of ATA -- every comparison of
    # its Jacobi sweeps is false -- and returns rank 6 with a finite x, which the reference's `>` tests then accept; a NaN
    # in ATb gives a NaN x that those tests accept as well.  The restatement, like the kernels, answers NaN, rank 0, lost.
    A, b = SYSTEMS["spd"]()
    for at in (3, 23):
        t = terms_of(A, b)
        t[at] = np.nan
        ex, _, erank, ezero = R.icp_solve(t)
        assert erank == 6 and not ezero and np.all(np.isfinite(ex)) == (at == 3), at
        x, _, rank, _ = S.jacobi_svd_solve(*S.system(t))
        assert rank == 0 and np.all(np.isnan(x)) and not S.is_zero(t), at
        st = S.new_state()
        S.f5_step(st, t[None], 1.0, 1.0, 0.0, True)
        assert st["lost"], at
    for x in ([0.01, -0.02, 0.015], [0.3, 0.2, -0.4], [0.0, 0.0, 0.0], [1e-7, 0.0, 0.0], [3.1, 0.02, -0.01]):
        Rm = S.rot_zyx(np.array(x + [0, 0, 0], np.float64))
        want = S.angle_axis_angle(Rm)
        got = float(R.rotation_angle(Rm))
        # float32 acos near w = 1: d(angle) = 2 d(w) / sin(angle / 2), d(w) = 2^-24: 4 2^-24 / angle, plus float32's own ulp
        assert abs(got - want) <= 4 * 2.0 ** -24 / max(want, 2e-5) + 2.0 ** -22, (x, got, want)
        assert abs(float(G.angle_axis_angle(Rm)) - got) <= 4 * 2.0 ** -24 / max(want, 2e-5) + 2.0 ** -22, x
