"""The 6x6 solve step of both trackers (k_icp_solve, k_icp_rgbd_solve) on crafted systems, against tests/icp_reference.py,
a float64 statement of the reference's rules written apart from the kernels (Eigen's isZero, JacobiSVD's rank and
minimum-norm solve, delinearisation, the rigidity check, align's early-out).

CPU: known answers of icp_reference itself.
GPU: the kernels driven through the C ABI (vh_icp_begin, vh_icp_begin_level, vh_icp_solve, vh_icp_rgbd_begin,
vh_icp_rgbd_solve) on wave partials written from numpy: the in-order float32 sum for 1 ... 400 partials, well- and
ill-conditioned, rank-deficient and threshold systems, lost / done decisions on both sides of every threshold, the
latching of lost and done (also in the correspondence and build kernels), and the order of composition."""
import ctypes as C
import math

import numpy as np
import pytest

import icp_reference as R
import rgbd_icp as G
from voxelhashing_amd import vhtypes as T

f32 = np.float32
MINF = np.float32(-np.inf)
THR = 6.0 * 2.0 ** -23  # JacobiSVD's threshold() for a 6x6 float matrix, relative to s_0
TINY_STEP = np.array([1e-3, -2e-3, 1.5e-3, 4e-3, -1e-3, 2.5e-3])


def terms_of(ata, atb, err=1.0, weight=1.0, count=100.0):
    """(6x6, 6) -> the 30 float32 terms of one wave, in the kernels' order"""
    ata = np.asarray(ata, np.float64)
    t = np.zeros(R.TERMS, np.float32)
    t[:21] = [ata[r, c] for r, c in R.UPPER]
    t[21:27] = atb
    t[27:] = err, weight, count
    return t


def integer_system(rows, x0):
    """A = J^T J of an integer J (exact in float32: every entry is an integer below 2^24) and b = A x0, rounded to float32
    once; the reference and the kernel then solve the very same float32 system"""
    J = np.asarray(rows, np.float64)
    A = J.T @ J
    assert np.all(np.abs(A) < 2 ** 24)
    return A, (A @ x0).astype(np.float32).astype(np.float64)


def plane_rows(n, pts):
    """buildRowSystemMatrixPlane (CUDABuildLinearSystem.cu:70-82) for integer points on a plane with integer normal"""
    n = np.asarray(n, np.float64)
    return [[n[0] * q[1] - n[1] * q[0], n[2] * q[0] - n[0] * q[2], n[1] * q[2] - n[2] * q[1], -n[0], -n[1], -n[2]] for q in pts]


def rotated_plane_system():
    # plane x + 2y + 2z = 6, normal (1, 2, 2): rank 3 (two in-plane translations and the rotation about the normal are free)
    pts = [(6 - 2 * y - 2 * z, y, z) for y in range(-3, 4) for z in range(-3, 4)]
    return integer_system(plane_rows((1, 2, 2), pts), TINY_STEP)


def axis_plane_system():
    # plane z = 5, normal (0, 0, 1): columns 0, 3 and 4 of A are exactly zero
    pts = [(x, y, 5) for x in range(-4, 5) for y in range(-3, 4)]
    return integer_system(plane_rows((0, 0, 1), pts), TINY_STEP)


def rank5_system():
    rng = np.random.default_rng(11)
    J = rng.integers(-4, 5, size=(12, 6)).astype(np.float64)
    J[:, 5] = J[:, 0] - J[:, 2] + J[:, 3]  # null vector (1, 0, -1, 1, 0, -1): not axis-aligned
    return integer_system(J, TINY_STEP)


def spd_system(cond, scale=1.0, seed=3):
    """Q diag(s) Q^T with eigenvalues from `scale` down to scale / cond, rounded to float32; b = A x0"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    s = scale * np.logspace(0.0, -math.log10(cond), 6)
    A = ((Q * s) @ Q.T).astype(np.float32).astype(np.float64)
    A = 0.5 * (A + A.T)
    return A, (A @ TINY_STEP).astype(np.float32).astype(np.float64)


def threshold_diag(below=False):
    """diag(1, 1, 1, 1, 1, 6 * 2^-23): the last value sits exactly on JacobiSVD's rank threshold (kept); one float32 ulp
    below, it is dropped"""
    last = np.float32(THR)
    if below:
        last = np.nextafter(last, np.float32(0))
    A = np.diag([1.0, 1.0, 1.0, 1.0, 1.0, float(last)])
    b = np.array([1e-3, 2e-3, -1e-3, 3e-3, 1e-3, 0.0])
    b[5] = float(np.float32(0.02 * float(last)))
    return A, b


# ---------------------------------------------------------------------------- CPU: known answers of the statement

def test_reference_diagonal_and_threshold():
    A = np.diag([4.0, 2.0, 1.0, 0.5, 0.25, 0.125])
    b = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    x, s, rank, cond = R.jacobi_svd_solve(A, b)
    assert np.array_equal(x, 1.0 / np.diag(A)) and rank == 6 and cond == 32.0 and list(s) == sorted(np.diag(A), reverse=True)
    A, b = threshold_diag()
    x, _, rank, _ = R.jacobi_svd_solve(A, b)
    assert rank == 6 and abs(x[5] - b[5] / A[5, 5]) <= 1e-15 and abs(x[5] - 0.02) < 1e-8  # Eigen solves all six components
    A, b = threshold_diag(below=True)
    x, _, rank, _ = R.jacobi_svd_solve(A, b)
    assert rank == 5 and x[5] == 0.0


def test_reference_rank3_rotated_plane():
    A, b = rotated_plane_system()
    x, s, rank, cond = R.jacobi_svd_solve(A, b)
    assert rank == 3
    w, V = np.linalg.eigh(A)
    null = V[:, w < 1e-9 * w.max()]
    proj = null @ null.T
    assert null.shape[1] == 3 and np.abs(proj - np.diag(np.diag(proj))).max() > 0.1  # the null space is not axis-aligned
    assert np.abs(null.T @ x).max() < 1e-12 * np.abs(x).max()           # x is orthogonal to the null space
    P = np.eye(6) - null @ null.T
    assert np.allclose(A @ x, P @ b, rtol=0, atol=1e-10 * np.abs(b).max())  # A x = P_range b
    assert cond > 1e12  # s_5 is rounding noise of a singular matrix: inf in exact arithmetic


def test_reference_rank3_axis_plane_is_inf_condition():
    A, b = axis_plane_system()
    assert np.all(A[[0, 3, 4]] == 0.0)
    x, s, rank, cond = R.jacobi_svd_solve(A, b)
    assert rank == 3 and cond == math.inf and np.all(x[[0, 3, 4]] == 0.0) and np.all(s[3:] == 0.0)


def test_reference_is_zero_boundary_and_nan():
    eps = np.float32(1e-5)
    t = np.zeros(30, np.float32)
    t[:21] = -eps * 0.5
    t[7] = -eps
    assert R.is_zero(t)  # max |a| = 1e-5f: lost
    t[7] = -np.nextafter(eps, np.float32(1))
    assert not R.is_zero(t)  # one ulp above: solved
    t[21:] = 123.0  # ATb and the statistics do not count
    t[7] = eps
    assert R.is_zero(t)
    t[3] = np.nan
    assert not R.is_zero(t)  # NaN is not zero ...
    st = R.new_state()
    R.f5_step(st, t[None], 1.0, 1.0, 0.0, True)
    assert st["lost"]        # ... and the NaN step fails the rigidity check


def test_reference_steps_compose_and_stop():
    A = np.eye(6)
    x = np.array([0.01, 0.0, 0.0, 0.02, 0.0, 0.0])
    t = terms_of(A, x, err=5.0)
    D = np.eye(4)
    D[:3, :3] = R.rot_zyx([0.2, -0.1, 0.3])
    D[:3, 3] = [0.1, 0.2, -0.3]
    st = R.new_state(D)
    R.f5_step(st, t[None], 1.0, 1.0, 0.5, False)
    assert np.allclose(st["delta"], R.transform(x) @ D, atol=1e-7) and not np.allclose(st["delta"], D @ R.transform(x), atol=1e-3)
    assert not st["done"] and st["lastError"] == -1.0
    R.f5_step(st, t[None], 1.0, 1.0, 0.5, True)
    assert not st["done"] and st["lastError"] == 5.0
    R.f5_step(st, t[None], 1.0, 1.0, 0.5, True)
    assert st["done"] and st["iterations"] == 3
    assert R.angle_axis_angle(R.rot_zyx([0.3, 0.0, 0.0])) == pytest.approx(0.3, abs=1e-12)
    assert R.angle_axis_angle(np.eye(3)) == 0.0


# ---------------------------------------------------------------------------- GPU

class Solver:
    """one VhIcpState or VhIcpStateRGBD on the device, driven through the C ABI"""

    def __init__(self, vh, rgbd, delta=None):
        from voxelhashing_amd import lib
        self.vh, self.lib, self.rgbd = vh, lib, rgbd
        self.cls = T.IcpStateRGBD if rgbd else T.IcpState
        self.d_state = lib.DeviceBuffer(C.sizeof(self.cls))
        d = lib.DeviceBuffer.from_numpy(np.eye(4, dtype=np.float32) if delta is None else np.asarray(delta, np.float32).reshape(16))
        lib.check((vh.vh_icp_rgbd_begin if rgbd else vh.vh_icp_begin)(self.d_state.ptr, d.ptr, None), "begin")

    def solve(self, partials, angle=1.0, dist=1.0, early_out=0.0, last_inner=True):
        p = np.ascontiguousarray(np.asarray(partials, np.float32).reshape(-1, R.TERMS))
        d_p = self.lib.DeviceBuffer.from_numpy(p)
        if self.rgbd:
            self.lib.check(self.vh.vh_icp_rgbd_solve(self.d_state.ptr, d_p.ptr, len(p), angle, dist, early_out, None), "rgbd_solve")
        else:
            self.lib.check(self.vh.vh_icp_solve(self.d_state.ptr, d_p.ptr, len(p), angle, dist, early_out, 1 if last_inner else 0, None), "solve")
        return self.state()

    def begin_level(self):
        self.lib.check(self.vh.vh_icp_begin_level(self.d_state.ptr, None), "begin_level")
        return self.state()

    def raw(self):
        return self.d_state.download(np.uint8, C.sizeof(self.cls)).tobytes()

    def state(self):
        st = self.cls.from_buffer_copy(self.raw())
        return st.icp if self.rgbd else st

    def full(self):
        return self.cls.from_buffer_copy(self.raw())


def assert_state(got, want, what, delta_tol=None):
    assert bool(got.lost) == want["lost"] and bool(got.done) == want["done"], (what, got.lost, got.done, want["lost"], want["done"])
    assert got.iterations == want["iterations"], what
    # the sums are the reference's in-order float32 sums: bit for bit
    assert f32(got.sumRegError).tobytes() == f32(want["sumRegError"]).tobytes(), (what, got.sumRegError, want["sumRegError"])
    assert f32(got.sumRegWeight).tobytes() == f32(want["sumRegWeight"]).tobytes(), what
    assert got.numCorr == want["numCorr"], what
    assert f32(got.lastError) == f32(want["lastError"]), what
    if delta_tol is not None:
        d = np.array(got.delta, np.float64).reshape(4, 4)
        assert np.abs(d - want["delta"]).max() <= delta_tol, (what, np.abs(d - want["delta"]).max())


@pytest.mark.gpu
@pytest.mark.parametrize("rgbd", [False, True])
def test_gpu_solve_sums_partials_in_order(vh, rgbd):
    """reductionSystemCPU: the kernel's 8-wide loop plus remainder must add the partials one after the other"""
    rng = np.random.default_rng(7)
    for nP in (1, 7, 8, 9, 17, 400):
        p = np.zeros((nP, R.TERMS), np.float32)
        # magnitudes over eight decades: a float32 sum in any other order (pairwise, reversed, 8 interleaved
        # accumulators) comes out different
        p[:, 27] = 10.0 ** rng.uniform(-4, 4, nP)
        p[:, 28] = 10.0 ** rng.uniform(-4, 4, nP)
        p[:, 29] = rng.integers(0, 2 ** 20, nP) + 0.5 * rng.integers(0, 2, nP) + 2.0 ** 22 * (rng.random(nP) < 0.3)
        p[0, :21] = terms_of(np.eye(6), np.zeros(6))[:21]  # a solvable system: the step is zero
        if nP >= 17:  # the data can tell the orders apart: the reversed order gives other bits
            seq, rev = R.reduce_partials(p), R.reduce_partials(p[::-1])
            assert np.any(seq[27:] != rev[27:])
        sv = Solver(vh, rgbd)
        got = sv.solve(p)
        want = R.new_state()
        (R.rgbd_step(want, p, 1.0, 1.0, 0.0) if rgbd else R.f5_step(want, p, 1.0, 1.0, 0.0, True))
        assert_state(got, want, f"nP={nP}", delta_tol=1e-7)


SYSTEMS = {
    "spd": lambda: spd_system(10.0),
    "cond1e5": lambda: spd_system(1e5, seed=4),
    "big_terms": lambda: spd_system(30.0, scale=3e5, seed=5),  # terms ~1e5, the magnitude of a 640x480 level-0 system
    "rank5": rank5_system,
    "rank3_axis": axis_plane_system,
    "rank3_rotated": rotated_plane_system,
    "threshold": threshold_diag,
    "below_threshold": lambda: threshold_diag(below=True),
}


@pytest.mark.gpu
@pytest.mark.parametrize("rgbd", [False, True])
@pytest.mark.parametrize("name", list(SYSTEMS))
def test_gpu_solve_systems(vh, rgbd, name):
    A, b = SYSTEMS[name]()
    p = terms_of(A, b)[None]
    x, s, rank, cond = R.jacobi_svd_solve(*R.system(p[0]))
    sv = Solver(vh, rgbd)
    st = sv.solve(p)
    want = R.new_state()
    (R.rgbd_step(want, p, 1.0, 1.0, 0.0) if rgbd else R.f5_step(want, p, 1.0, 1.0, 0.0, True))
    assert not want["lost"]
    # Tolerance.  The kernel solves the same float32 system in double (cyclic Jacobi) and casts x to float: the
    # double error is ~cond * 1e-16 relative, the cast 6e-8 relative per component.  For cond <= 1e5 that is below
    # 1e-6 of max|x|.  The rank-deficient systems are solved on their range, where they are well-conditioned.
    # From the identity, the delta's translation is the cast x[3:6] itself; its rotation is Rz Ry Rx of the cast angles
    # in float32 (cosf / sinf, products of three): 1e-6 absolute.
    d = np.array(st.delta, np.float64).reshape(4, 4)
    assert np.abs(d[:3, 3] - x[3:6]).max() <= 1e-6 * np.abs(x).max(), (name, d[:3, 3], x[3:6])
    assert np.abs(d[:3, :3] - R.rot_zyx(x)).max() <= 1e-6, name
    if rgbd:  # the linearisation point left for the next step: the new delta's Euler angles (near 0 here) and translation
        full = sv.full()
        assert np.abs(np.array(full.angles) - x[:3]).max() <= 1e-6 * np.abs(x).max() + 1e-7, (name, list(full.angles), x[:3])
        assert np.array_equal(np.array(full.translation, np.float32), d[:3, 3].astype(np.float32))
    if math.isinf(cond):
        assert st.matrixCondition == math.inf, name
    elif cond < 1e12:  # matrixCondition is float: s_0 / s_5 to 1e-5 relative where the singular values are resolved
        assert abs(st.matrixCondition / cond - 1.0) <= 1e-5, (name, st.matrixCondition, cond)
    else:  # a rank-deficient matrix whose null values are rounding noise: only the size says something
        assert st.matrixCondition > 1e10, (name, st.matrixCondition)
    assert_state(st, want, name)
    if name == "threshold":  # Eigen keeps the value on the threshold and solves for all six components
        assert abs(x[5] - 0.02) < 1e-8 and abs(st.delta[11] - 0.02) < 1e-8, st.delta[11]
    if name == "below_threshold":  # one ulp below, the component is dropped
        assert x[5] == 0.0 and st.delta[11] == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("rgbd", [False, True])
def test_gpu_lost_decisions(vh, rgbd):
    eps = np.float32(1e-5)

    def run(p, **kw):
        sv = Solver(vh, rgbd)
        st = sv.solve(p, **{k: v for k, v in kw.items() if k != "what" and not (rgbd and k == "last_inner")})
        want = R.new_state()
        args = (kw.get("angle", 1.0), kw.get("dist", 1.0), kw.get("early_out", 0.0))
        (R.rgbd_step(want, p, *args) if rgbd else R.f5_step(want, p, *args, kw.get("last_inner", True)))
        assert_state(st, want, kw.get("what", ""))
        return st, want

    # ATA.isZero(): every |a_ij| <= 1e-5f is lost, one ulp more is solved
    for top, lost in ((eps, True), (np.nextafter(eps, np.float32(1)), False)):
        A = np.eye(6) * float(top)
        A[0, 1] = A[1, 0] = 0.5 * float(eps)
        t = terms_of(A, A @ TINY_STEP)
        st, want = run(t[None], what=f"isZero {top!r}")
        assert bool(st.lost) == lost == want["lost"]
    # NaN terms: lost (the reference would let the NaN step through its `>` tests)
    t = terms_of(np.eye(6), TINY_STEP)
    t[4] = np.nan
    st, _ = run(t[None], what="nan")
    assert st.lost == 1
    # a step at 0.99x / 1.01x of the angle threshold and of the distance threshold
    for x, key in ((np.array([0.2, 0, 0, 0, 0, 0.0]), "angle"), (np.array([0, 0, 0, 0.03, -0.04, 0.0]), "dist")):
        size = 0.2 if key == "angle" else 0.05
        for f, lost in ((0.99, False), (1.01, True)):
            st, _ = run(terms_of(np.eye(6), x)[None], what=f"{key} {f}", **{key: size / f})
            assert bool(st.lost) == lost, (key, f)


@pytest.mark.gpu
def test_gpu_early_out(vh):
    t = terms_of(np.eye(6), TINY_STEP * 0.1, err=5.0)[None]
    # f5: only after the last inner iteration of an outer iteration
    sv = Solver(vh, False)
    st = sv.solve(t, early_out=100.0, last_inner=False)
    assert st.done == 0 and st.lastError == -1.0
    st = sv.solve(t, early_out=100.0, last_inner=True)
    assert st.done == 1 and st.lastError == 5.0 and st.iterations == 2
    sv = Solver(vh, False)
    st = sv.solve(t, early_out=1e-3, last_inner=True)
    assert st.done == 0 and st.lastError == 5.0
    st = sv.solve(t, early_out=1e-3, last_inner=True)
    assert st.done == 1
    # RGB-D: after every call
    sv = Solver(vh, True)
    st = sv.solve(t, early_out=1e-3)
    assert st.done == 0 and st.lastError == 5.0
    st = sv.solve(t, early_out=1e-3)
    assert st.done == 1 and st.iterations == 2
    want = R.new_state()
    for _ in range(2):
        R.rgbd_step(want, t, 1.0, 1.0, 1e-3)
    assert_state(st, want, "rgbd early out", delta_tol=2e-6)


def _sentinel(n):
    return np.full(n, 0x7FBADBAD, np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("rgbd", [False, True])
@pytest.mark.parametrize("how", ["lost", "done"])
def test_gpu_lost_and_done_latch(vh, rgbd, how):
    from voxelhashing_amd import lib
    sv = Solver(vh, rgbd)
    good = terms_of(np.eye(6), TINY_STEP, err=5.0)[None]
    if how == "lost":
        st = sv.solve(terms_of(np.zeros((6, 6)), np.zeros(6))[None])
        assert st.lost == 1
    else:
        st = sv.solve(good, early_out=100.0)
        assert st.done == 1 and st.lost == 0
    before = sv.raw()
    other = terms_of(2.0 * np.eye(6), TINY_STEP, err=9.0)[None]
    sv.solve(other, early_out=100.0)
    assert sv.raw() == before, "a solve after lost / done changed the state"
    # the correspondence and build kernels of a finished level leave their outputs alone
    W, H = 64, 24
    rng = np.random.default_rng(1)
    pos = np.concatenate([rng.uniform(-0.3, 0.3, (H, W, 2)), rng.uniform(0.8, 1.2, (H, W, 1)), np.ones((H, W, 1))], -1).astype(np.float32)
    nrm = np.zeros((H, W, 4), np.float32)
    nrm[..., 2] = -1.0
    up = lambda a: lib.DeviceBuffer.from_numpy(np.ascontiguousarray(a))
    d_pos, d_nrm = up(pos), up(nrm)
    cp = T.make_depth_camera_params(W, H)
    if rgbd:
        inten = np.full((H, W), 0.5, np.float32)
        iad = np.concatenate([np.full((H, W, 1), 0.5), np.full((H, W, 2), 0.1), np.ones((H, W, 1))], -1).astype(np.float32)
        d_i, d_iad = up(inten), up(iad)
        nP = vh.vh_icp_rgbd_num_partials(W, H, 0)
        d_part = up(_sentinel(nP * 30))
        prm = T.IcpRGBDParams(fx=cp.fx, fy=cp.fy, mx=cp.mx, my=cp.my, weightDepth=1.0, weightColor=1.0, distThres=0.15, normalThres=0.9,
                              sensorMaxDepth=4.0, colorGradientMin=0.0, colorThres=1.0, level=0)
        lib.check(vh.vh_icp_rgbd_build_linear_system(W, H, d_part.ptr, d_pos.ptr, d_nrm.ptr, d_i.ptr, d_pos.ptr, d_nrm.ptr, d_iad.ptr,
                                                     C.byref(prm), sv.d_state.ptr, None))
        outs = [d_part]
    else:
        d_c, d_cn = up(_sentinel(W * H * 4)), up(_sentinel(W * H * 4))
        lib.check(vh.vh_icp_projective_correspondences(d_pos.ptr, d_nrm.ptr, d_pos.ptr, d_nrm.ptr, d_c.ptr, d_cn.ptr, W, H, 0.15, 0.5, 1.0,
                                                       sv.d_state.ptr, C.byref(cp), None))
        nP = vh.vh_icp_num_partials(W, H)
        d_part = up(_sentinel(nP * 30))
        d_cc, d_ccn = up(pos), up(np.concatenate([nrm[..., :3], np.ones((H, W, 1), np.float32)], -1))
        lib.check(vh.vh_icp_build_linear_system(W, H, d_part.ptr, d_pos.ptr, d_cc.ptr, d_ccn.ptr, sv.d_state.ptr, None))
        outs = [d_c, d_cn, d_part]
    for o in outs:
        assert np.all(o.download(np.uint32) == 0x7FBADBAD), f"{how}: a launch after {how} wrote its output"
    # vh_icp_begin_level clears done (and lastError), not lost
    st = sv.begin_level()
    if how == "lost":
        assert st.lost == 1
    else:
        assert st.done == 0 and st.lost == 0 and st.lastError == -1.0
        st = sv.solve(other, early_out=0.0)
        assert st.iterations == 2  # the next level solves again


@pytest.mark.gpu
def test_gpu_sentinel_control_builds_write(vh):
    """the control for test_gpu_lost_and_done_latch: with a live state the same launches do write their outputs"""
    from voxelhashing_amd import lib
    sv = Solver(vh, False)
    W, H = 64, 24
    pos = np.zeros((H, W, 4), np.float32)
    pos[..., 2] = 1.0
    pos[..., 3] = 1.0
    nrm = np.zeros((H, W, 4), np.float32)
    nrm[..., 2] = -1.0
    nrm[..., 3] = 1.0
    up = lambda a: lib.DeviceBuffer.from_numpy(np.ascontiguousarray(a))
    d_pos, d_nrm = up(pos), up(nrm)
    nP = vh.vh_icp_num_partials(W, H)
    d_part = up(_sentinel(nP * 30))
    lib.check(vh.vh_icp_build_linear_system(W, H, d_part.ptr, d_pos.ptr, d_pos.ptr, d_nrm.ptr, sv.d_state.ptr, None))
    assert not np.any(d_part.download(np.uint32) == 0x7FBADBAD)


@pytest.mark.gpu
def test_gpu_order_of_composition(vh):
    x = np.array([0.01, -0.02, 0.015, 0.01, 0.02, -0.005])
    t = terms_of(np.eye(6), x)[None]
    # f5: the new step multiplies the delta from the left
    D = np.eye(4, dtype=np.float32)
    D[:3, :3] = R.rot_zyx([0.2, -0.1, 0.3])
    D[:3, 3] = [0.1, 0.2, -0.3]
    st = Solver(vh, False, D).solve(t)
    want = R.new_state(D)
    R.f5_step(want, t, 1.0, 1.0, 0.0, True)
    got = np.array(st.delta, np.float64).reshape(4, 4)
    # float32 products of float32 factors, 4-term sums: 2e-6 absolute on entries of size <= 1
    assert np.abs(got - want["delta"]).max() <= 2e-6, np.abs(got - want["delta"]).max()
    assert np.abs(got - D.astype(np.float64) @ R.transform(x)).max() > 1e-3
    # RGB-D: from the far Euler branch (rz = -0.3 degrees: linearised near (pi, +-pi, +-pi)) the increment is added to
    # those angles and the state holds the new delta's angles and translation
    E = np.asarray(G.plane_pose(0.004, 0.002, rz_deg=-0.3), np.float32).reshape(4, 4)
    sv = Solver(vh, True, E)
    a0 = np.array(sv.full().angles)
    assert np.all(np.abs(np.abs(a0) - np.pi) < 0.01), a0
    st = sv.solve(t)
    full = sv.full()
    want = R.new_state(E)
    x_new = R.rgbd_step(want, t, 1.0, 1.0, 0.0)
    got = np.array(st.delta, np.float64).reshape(4, 4)
    # the angles near pi carry 2.4e-7 of float32 rounding each, and the state's angles are eulerAngles of the new
    # float32 delta: 2e-6 absolute
    assert np.abs(got - want["delta"]).max() <= 2e-6, np.abs(got - want["delta"]).max()
    ang = np.array(full.angles, np.float64)
    assert np.abs(R.rot_zyx(ang) - want["delta"][:3, :3]).max() <= 2e-6
    assert np.array_equal(np.array(full.translation, np.float32), np.array(st.delta, np.float32).reshape(4, 4)[:3, 3])
    assert np.abs(np.array(full.translation) - x_new[3:6]).max() <= 1e-6
