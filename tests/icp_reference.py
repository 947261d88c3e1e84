"""The reference's 6x6 solve step of both trackers, restated in float64 from the sources it runs: the Eigen 3.2.2 the
reference vendors (DepthSensingCUDA/Include/Eigen) and DepthSensingCUDA's CUDABuildLinearSystem*.cpp /
CUDACameraTrackingMultiRes*.cpp.  TEST INFRASTRUCTURE ONLY.

It is written apart from the kernels and from their restatements (oracle/icp.py, tests/rgbd_icp.py), which were written
next to the kernels and share their rules, so that a wrong rule in both shows up: it imports none of their rules, only
rgbd_icp.euler_angles_zyx (a float32 helper for the linearisation point, tested in tests/test_rgbd_tracking.py).

The rules, each as the reference states it:
- reductionSystemCPU (CUDABuildLinearSystem.cpp:52-92, CUDABuildLinearSystemRGBD.cpp:46-86): the wave partials summed in
  their order in float32, sumRegError / sumRegWeight / numCorr included, numCorr converted to unsigned at the end.
- ATA.isZero() (CUDACameraTrackingMultiRes.cpp:228, CUDACameraTrackingMultiResRGBD.cpp:215) of a Matrix6x6f:
  DenseBase::isZero (Core/CwiseNullaryOp.h:482-489) with isMuchSmallerThan (Core/MathFunctions.h:653-657) and
  NumTraits<float>::dummy_precision() = 1e-5f (Core/NumTraits.h:94): lost when every |a_ij| <= 1e-5f.  NaN <= x is
  false, so a NaN entry is not zero.
- JacobiSVD::solve (SVD/JacobiSVD.h:925-941) through rank() (:683-691) and threshold() (:733-738): the minimum-norm
  solution over the singular values with s >= s_0 * 6 * 2^-23; exact zeros are never counted
  (m_nonzeroSingularValues, :895-904).  The condition number is s_0 / s_5 (CUDACameraTrackingMultiRes.cpp:237).
- delinearizeTransformation (CUDACameraTrackingMultiRes.cpp:193-211) with mean 0 and stddev 1: R = Rz(x0) Ry(x1) Rx(x2),
  t = x[3..5]; checkRigidTransformation (:182-191): lost when AngleAxisf(R).angle() > angleThres or |t| > distThres.
  AngleAxis from a rotation matrix goes through the quaternion (Geometry/Quaternion.h:724-760,
  Geometry/AngleAxis.h:159-175): angle 2 acos(w), 0 when |vec|^2 < dummy_precision^2.  A NaN step passes the
  reference's `>` tests; the project fails it (fenced defects), and so does this statement.
- f5 (CUDACameraTrackingMultiRes.cpp:226-251, 306-318): delta = T(x) * delta; align's early-out compares the residual
  after the last inner iteration of an outer iteration with the previous one: |lastError - sumRegError| < earlyOut.
- RGB-D (CUDACameraTrackingMultiResRGBD.cpp:203-237, 329-350): xNew = [eulerAngles(2,1,0) of delta; t of delta] + x,
  delta = T(xNew) after the check on T(xNew) itself; the early-out after every outer iteration (one solve each).
"""
import math

import numpy as np

from rgbd_icp import euler_angles_zyx

f32 = np.float32
EPS_F32 = 2.0 ** -23                    # NumTraits<float>::epsilon()
DUMMY_PRECISION = np.float32(1e-5)      # NumTraits<float>::dummy_precision()
TERMS = 30
UPPER = [(r, c) for r in range(6) for c in range(r, 6)]  # the order of the 21 ATA terms in a wave's row


def reduce_partials(partials):
    """reductionSystemCPU: (nP, 30) float32 -> (30,) float32, summed from the first partial to the last"""
    p = np.asarray(partials, np.float32).reshape(-1, TERMS)
    if len(p) == 0:
        return np.zeros(TERMS, np.float32)
    return np.cumsum(p, axis=0, dtype=np.float32)[-1]


def system(terms):
    """the 30 summed float32 terms -> (ATA 6x6, ATb 6) in float64 (both exact copies of the float32 values)"""
    t = np.asarray(terms, np.float32)
    ata = np.zeros((6, 6))
    for k, (r, c) in enumerate(UPPER):
        ata[r, c] = ata[c, r] = t[k]
    return ata, t[21:27].astype(np.float64)


def is_zero(terms):
    """ATA.isZero() on the float32 terms: every |a_ij| <= 1e-5f (a NaN is not <=, so not zero)"""
    return bool(np.all(np.abs(np.asarray(terms, np.float32)[:21]) <= DUMMY_PRECISION))


def jacobi_svd_solve(ata, atb):
    """-> (x, singular values in descending order, rank, condition s_0 / s_5).

    Rows / columns of ATA that are exactly zero are never rotated by Eigen's two-sided Jacobi sweeps (the off-diagonal
    entry is 0, below any threshold), so their singular values come out as exact zeros; numpy's SVD would give values
    of order 1e-17 there, so those columns are split off before it runs.  The rest is decomposed in float64."""
    ata, atb = np.asarray(ata, np.float64), np.asarray(atb, np.float64)
    if not (np.all(np.isfinite(ata)) and np.all(np.isfinite(atb))):
        return np.full(6, np.nan), np.full(6, np.nan), 0, float("nan")  # NaN in, NaN out: the rigidity check fails it
    live = np.any(ata != 0.0, axis=1)
    s = np.zeros(6)
    x = np.zeros(6)
    rank = 0
    if live.any():
        sub = ata[np.ix_(live, live)]
        u, sv, vt = np.linalg.svd(sub)
        s[:len(sv)] = sv
        keep = (sv >= sv[0] * 6.0 * EPS_F32) & (sv != 0.0)
        rank = int(keep.sum())
        x[live] = vt.T[:, keep] @ ((u.T[keep] @ atb[live]) / sv[keep])
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = s[0] / s[5]
    return x, s, rank, float(cond)


def rot_zyx(x):
    """Rz(x0) Ry(x1) Rx(x2) in float64"""
    cz, sz, cy, sy, cx, sx = (f(float(a)) for a in (x[0], x[1], x[2]) for f in (math.cos, math.sin))
    return np.array([[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx],
                     [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx],
                     [-sy, cy * sx, cy * cx]])


def angle_axis_angle(R):
    """AngleAxis(R).angle(): the quaternion by Shoemake's construction, then 2 acos(w), 0 below dummy_precision"""
    R = np.asarray(R, np.float64)
    tr = np.trace(R)
    q = np.zeros(4)  # x, y, z, w
    if tr > 0.0:
        t = math.sqrt(tr + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = math.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
    if q[0] ** 2 + q[1] ** 2 + q[2] ** 2 < float(DUMMY_PRECISION) ** 2:
        return 0.0
    return 2.0 * math.acos(min(max(-1.0, q[3]), 1.0))


def rigid_ok(R, t, angle_thres, dist_thres):
    """checkRigidTransformation, with a NaN failing it (the project's fence)"""
    if not (np.all(np.isfinite(R)) and np.all(np.isfinite(t))):
        return False
    return bool(angle_axis_angle(R) <= angle_thres and np.linalg.norm(t) <= dist_thres)


def transform(x):
    m = np.eye(4)
    m[:3, :3] = rot_zyx(x)
    m[:3, 3] = np.asarray(x[3:6], np.float64)
    return m


def new_state(delta=None):
    """the part of VhIcpState the solve step reads and writes, as after vh_icp_begin"""
    return dict(delta=np.eye(4) if delta is None else np.asarray(delta, np.float64).reshape(4, 4).copy(), lastError=-1.0,
                done=False, lost=False, sumRegError=0.0, sumRegWeight=0.0, numCorr=0, matrixCondition=0.0, iterations=0)


def _sum_into(st, partials):
    t = reduce_partials(partials)
    st.update(sumRegError=t[27], sumRegWeight=t[28], numCorr=int(t[29]) if np.isfinite(t[29]) else 0, iterations=st["iterations"] + 1)
    return t


def f5_step(st, partials, angle_thres, dist_thres, early_out, last_inner):
    """one inner iteration of computeBestRigidAlignment plus, when last_inner, align's early-out; updates st in place
    and returns the solve's x (None when no solve ran)"""
    if st["lost"] or st["done"]:
        return None
    t = _sum_into(st, partials)
    if is_zero(t):
        st["lost"] = True
        return None
    x, _, _, st["matrixCondition"] = jacobi_svd_solve(*system(t))
    if not rigid_ok(rot_zyx(x), x[3:6], angle_thres, dist_thres):
        st["lost"] = True
        return x
    st["delta"] = transform(x) @ st["delta"]
    if last_inner:
        if abs(f32(st["lastError"]) - f32(st["sumRegError"])) < f32(early_out):
            st["done"] = True
        st["lastError"] = st["sumRegError"]
    return x


def rgbd_step(st, partials, angle_thres, dist_thres, early_out):
    """one outer iteration of the RGB-D align (computeBestRigidAlignment, then the early-out); the linearisation point
    is eulerAngles(2, 1, 0) of delta's rotation (float32, as the reference computes it on a Matrix3f) and its
    translation.  Returns xNew (None when no solve ran)."""
    if st["lost"] or st["done"]:
        return None
    t = _sum_into(st, partials)
    if is_zero(t):
        st["lost"] = True
        return None
    x, _, _, st["matrixCondition"] = jacobi_svd_solve(*system(t))
    old = np.asarray(st["delta"], np.float32)
    x_new = np.concatenate([euler_angles_zyx(old[:3, :3]).astype(np.float64), old[:3, 3].astype(np.float64)]) + x
    if not rigid_ok(rot_zyx(x_new), x_new[3:6], angle_thres, dist_thres):
        st["lost"] = True
        return x_new
    st["delta"] = transform(x_new)
    if abs(f32(st["lastError"]) - f32(st["sumRegError"])) < f32(early_out):
        st["done"] = True
    st["lastError"] = st["sumRegError"]
    return x_new
