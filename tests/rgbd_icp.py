"""numpy restatement of the RGB-D camera tracker (CUDACameraTrackingMultiResRGBD, DSC/CUDACameraTrackingMultiResRGBD.cpp
with scanNormalEquationsDevice, DSC/CUDABuildLinearSystemRGBD.cu:106-201), in the style of oracle/icp.py: per-pixel
arithmetic in float32 in the kernels' order, each lane's window summed in order, the +32 ... +1 wave tree, the wave
partials summed in order in float32 (reductionSystemCPU), the 6x6 solve by oracle.icp.solve.  TEST INFRASTRUCTURE ONLY.
pixel_terms and lane_sums are pinned to the reference's own kernel, compiled for the CPU (tests/test_tracker_pinning.py).

Also the textured-plane scene the RGB-D tests use: a fronto-parallel plane with a smooth procedural texture, where a
geometric tracker cannot see an in-plane motion and the photometric term can.
"""
import numpy as np

from oracle import icp
from oracle import oracle as O

MINF = np.float32(-np.inf)
f32 = np.float32
PI_F = np.float32(np.pi)
TERMS = 30


# ---------------------------------------------------------------------------------------------------------- scene

def plane_frame(pose, cp, z0=1.0, period=0.15):
    """depth (H, W) and RGBX bytes (H, W, 4) of the plane world z = z0 seen from the camera-to-world `pose` (16,
    row-major; the camera must look along world +z with no rotation about x or y).  The texture is
    0.5 + 0.3 sin(2 pi X / period) cos(2 pi Y / period) in three phases, so no pixel is black."""
    W, H = cp.m_imageWidth, cp.m_imageHeight
    m = np.asarray(pose, np.float64).reshape(4, 4)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    # camera ray (x, y, 1) scaled to hit the plane; the camera's z axis is world z
    z = z0 - m[2, 3]
    xc, yc = (u - cp.mx) / cp.fx * z, (v - cp.my) / cp.fy * z
    X = m[0, 0] * xc + m[0, 1] * yc + m[0, 2] * z + m[0, 3]
    Y = m[1, 0] * xc + m[1, 1] * yc + m[1, 2] * z + m[1, 3]
    k = 2.0 * np.pi / period
    rgbx = np.empty((H, W, 4), np.uint8)
    for c, ph in enumerate((0.0, 0.9, 2.1)):
        val = 0.5 + 0.3 * np.sin(k * X + ph) * np.cos(k * 0.8 * Y - ph)
        rgbx[..., c] = np.clip(np.floor(val * 255.0 + 0.5), 1, 255).astype(np.uint8)
    rgbx[..., 3] = 255
    depth = np.full((H, W), z, np.float32)
    return depth, rgbx


def plane_pose(tx, ty=0.0, rz_deg=0.0):
    m = np.eye(4, dtype=np.float64)
    a = np.radians(rz_deg)
    m[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    m[0, 3], m[1, 3] = tx, ty
    return m.astype(np.float32).reshape(16)


def sensor_maps(depth, rgbx, cp):
    """what CUDARGBDSensor hands over for an unfiltered frame: positions, normals, float4 colour"""
    W, H = cp.m_imageWidth, cp.m_imageHeight
    cam = O.image_op("convert_depth_float_to_camera_space_float4", depth, W, H, cp, out_channels=4)
    c = rgbx.astype(np.float32)
    col = np.stack([c[..., 0] / f32(255.0), c[..., 1] / f32(255.0), c[..., 2] / f32(255.0), np.ones_like(c[..., 0])], -1).astype(np.float32)
    return cam, O.compute_normals(cam), col


# ---------------------------------------------------------------------------------------------------------- kernels

def intensity(color4):
    """convertColorToIntensityFloatDevice"""
    c = color4.astype(np.float32)
    return (f32(0.299) * c[..., 0] + f32(0.587) * c[..., 1] + f32(0.114) * c[..., 2]).astype(np.float32)


def intensity_and_derivatives(img):
    """computeIntensityAndDerivativesDevice, DSC/CameraUtil.cu:1492-1529"""
    img = np.asarray(img, np.float32)
    H, W = img.shape
    out = np.full((H, W, 4), MINF, np.float32)
    if W < 3 or H < 3:
        return out
    p = lambda a, b: img[b:H - 2 + b, a:W - 2 + a]  # pos_ab = pixel (x - 1 + a, y - 1 + b)
    ok = np.ones((H - 2, W - 2), bool)
    for a in range(3):
        for b in range(3):
            ok &= p(a, b) != MINF
    with np.errstate(invalid="ignore"):
        ru = f32(-1.0) * p(0, 0) + f32(1.0) * p(2, 0) + f32(-2.0) * p(0, 1) + f32(2.0) * p(2, 1) + f32(-1.0) * p(0, 2) + f32(1.0) * p(2, 2)
        ru = ru / f32(8.0)
        rv = f32(-1.0) * p(0, 0) + f32(-2.0) * p(1, 0) + f32(-1.0) * p(2, 0) + f32(1.0) * p(0, 2) + f32(2.0) * p(1, 2) + f32(1.0) * p(2, 2)
        rv = rv / f32(8.0)
    inner = np.stack([p(1, 1), ru, rv, np.ones_like(ru)], -1).astype(np.float32)
    out[1:H - 1, 1:W - 1] = np.where(ok[..., None], inner, MINF)
    return out


def bilinear_float4(x, y, img):
    """bilinearInterpolationFloat4, DSC/ICPUtil.h:129-156 (x, y inside the fence: floor fits an int)"""
    H, W = img.shape[:2]
    px, py = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    alpha, beta = (x - px.astype(np.float32)).astype(np.float32), (y - py.astype(np.float32)).astype(np.float32)
    one = f32(1.0)

    def tap(tx, ty):
        inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        v = img[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)]
        return inside & (v[:, 0] != MINF) & (v[:, 1] != MINF) & (v[:, 2] != MINF), v

    n = len(x)
    with np.errstate(invalid="ignore", divide="ignore"):
        def row(ty):
            s, w = np.zeros((n, 4), np.float32), np.zeros(n, np.float32)
            ok, v = tap(px, ty)
            s = np.where(ok[:, None], s + (one - alpha)[:, None] * v, s)
            w = np.where(ok, w + (one - alpha), w)
            ok, v = tap(px + 1, ty)
            s = np.where(ok[:, None], s + alpha[:, None] * v, s)
            w = np.where(ok, w + alpha, w)
            return s, w
        s0, w0 = row(py)
        s1, w1 = row(py + 1)
        p0, p1 = s0 / w0[:, None], s1 / w1[:, None]
        ss, ww = np.zeros((n, 4), np.float32), np.zeros(n, np.float32)
        ss = np.where((w0 > 0)[:, None], ss + (one - beta)[:, None] * p0, ss)
        ww = np.where(w0 > 0, ww + (one - beta), ww)
        ss = np.where((w1 > 0)[:, None], ss + beta[:, None] * p1, ss)
        ww = np.where(w1 > 0, ww + beta, ww)
        return np.where((ww > 0)[:, None], ss / ww[:, None], MINF).astype(np.float32)


def euler_angles_zyx(R):
    """eulerAngles(2, 1, 0) of the reference's vendored Eigen (Geometry/EulerAngles.h), float32: e0 in [0, pi]"""
    R = np.asarray(R, np.float32).reshape(3, 3)
    e0 = np.arctan2(R[1, 0], R[0, 0])
    c2 = np.sqrt(R[2, 2] * R[2, 2] + R[2, 1] * R[2, 1])
    if e0 < 0:
        e0 = f32(e0 + PI_F)
        e1 = np.arctan2(-R[2, 0], -c2)
    else:
        e1 = np.arctan2(-R[2, 0], c2)
    s1, c1 = np.sin(e0), np.cos(e0)
    e2 = np.arctan2(s1 * R[0, 2] - c1 * R[1, 2], c1 * R[1, 1] - s1 * R[0, 1])
    return np.array([e0, e1, e2], np.float32)


def angle_axis_angle(R):
    """Eigen::AngleAxisf(R).angle() through the quaternion (AngleAxis.h / Quaternion.h), float32"""
    R = np.asarray(R, np.float32).reshape(3, 3)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4, np.float32)  # x y z w
    if tr > 0:
        t = np.sqrt(tr + f32(1.0))
        q[3] = f32(0.5) * t
        t = f32(0.5) / t
        q[0], q[1], q[2] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + f32(1.0))
        q[i] = f32(0.5) * t
        t = f32(0.5) / t
        q[3] = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
    if q[0] * q[0] + q[1] * q[1] + q[2] * q[2] < f32(1e-5) * f32(1e-5):
        return f32(0.0)
    return f32(2.0) * np.arccos(np.clip(q[3], f32(-1.0), f32(1.0)))


def _rmats(angles):
    """evalRMat and the three derivatives of DSC/ICPUtil.h:30-126 -> R, Ralpha (= dGamma), Rbeta, Rgamma (= dAlpha)"""
    g, b, a = [f32(v) for v in angles]
    ca, cb, cg, sa, sb, sg = np.cos(a), np.cos(b), np.cos(g), np.sin(a), np.sin(b), np.sin(g)
    z = f32(0.0)
    R = [cg * cb, -sg * ca + cg * sb * sa, sg * sa + cg * sb * ca, sg * cb, cg * ca + sg * sb * sa, -cg * sa + sg * sb * ca, -sb, cb * sa, cb * ca]
    dA = [z, sg * sa + cg * sb * ca, sg * ca - cg * sb * sa, z, -cg * sa + sg * sb * ca, -cg * ca - sg * sb * sa, z, cb * ca, -cb * sa]
    dB = [-cg * sb, cg * cb * sa, cg * cb * ca, -sg * sb, sg * cb * sa, sg * cb * ca, -cb, -sb * sa, -sb * ca]
    dG = [-sg * cb, -cg * ca - sg * sb * sa, cg * sa - sg * sb * ca, cg * cb, -sg * ca + cg * sb * sa, sg * sa + cg * sb * ca, z, z, z]
    m = lambda v: np.array(v, np.float32)
    return m(R), m(dG), m(dB), m(dA)


def _mul3(M, p):  # row-major 3x3 (9,) times (N, 3), float32, ((a + b) + c)
    return np.stack([M[3 * r] * p[:, 0] + M[3 * r + 1] * p[:, 1] + M[3 * r + 2] * p[:, 2] for r in range(3)], -1).astype(np.float32)


def window(level):
    """CUDABuildLinearSystemRGBD.cpp:31-32"""
    return 12 if level == 0 else max(1, 12 // (4 * level))


def pixel_terms(inp, inp_n, inp_i, tgt, tgt_n, tgt_iad, angles, trans, prm):
    """per-pixel contributions of both rows -> (depth terms (N, 30), colour terms (N, 30), depth row mask, colour row
    mask); the 21 ATA and 6 JTF products are stored positive (the kernel subtracts the JTF ones)"""
    H, W = inp.shape[:2]
    N = H * W
    p, n, ii = inp.reshape(N, 4)[:, :3], inp_n.reshape(N, 4)[:, :3], inp_i.reshape(N)
    R, Ra, Rb, Rg = _rmats(angles)
    t = np.asarray(trans, np.float32)
    fx, fy, mx, my = f32(prm["fx"]), f32(prm["fy"]), f32(prm["mx"]), f32(prm["my"])
    valid = np.all(p != MINF, 1) & np.all(n != MINF, 1) & (ii != MINF)
    dmask, cmask = np.zeros(N, bool), np.zeros(N, bool)
    dterm, cterm = np.zeros((N, TERMS), np.float32), np.zeros((N, TERMS), np.float32)
    idx = np.nonzero(valid)[0]
    with np.errstate(all="ignore"):
        rp = _mul3(R, p[idx])
        nT = _mul3(R, n[idx])
        pT = (rp + t).astype(np.float32)
        z0 = f32(0.0)
        pp = np.stack([fx * pT[:, 0] + z0 * pT[:, 1] + mx * pT[:, 2], z0 * pT[:, 0] + fy * pT[:, 1] + my * pT[:, 2],
                       z0 * pT[:, 0] + z0 * pT[:, 1] + f32(1.0) * pT[:, 2]], -1).astype(np.float32)
        u, v = pp[:, 0] / pp[:, 2], pp[:, 1] / pp[:, 2]
        un, vn = u + f32(0.5), v + f32(0.5)
        ok = (pp[:, 2] > 0) & (un > -1) & (un < W) & (vn > -1) & (vn < H)
    idx, pT, nT, pp, u, v, un, vn = idx[ok], pT[ok], nT[ok], pp[ok], u[ok], v[ok], un[ok], vn[ok]
    ui, vi = np.trunc(un).astype(np.int64), np.trunc(vn).astype(np.int64)
    tp, tn = tgt[vi, ui][:, :3], tgt_n[vi, ui][:, :3]
    it = bilinear_float4(u, v, tgt_iad)
    good = np.all(tp != MINF, 1) & np.all(tn != MINF, 1) & np.all(it[:, :3] != MINF, 1)
    idx, pT, nT, pp, tp, tn, it = idx[good], pT[good], nT[good], pp[good], tp[good], tn[good], it[good]
    p_in = p[idx]
    with np.errstate(all="ignore"):
        diff = (tp - pT).astype(np.float32)
        dDist = np.sqrt(diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1] + diff[:, 2] * diff[:, 2])
        dNormal = tn[:, 0] * nT[:, 0] + tn[:, 1] * nT[:, 1] + tn[:, 2] * nT[:, 2]
        geo = (dDist <= f32(prm["distThres"])) & (dNormal >= f32(prm["normalThres"]))
        idx, pT, pp, tp, tn, it, diff, dDist, p_in = idx[geo], pT[geo], pp[geo], tp[geo], tn[geo], it[geo], diff[geo], dDist[geo], p_in[geo]
        phis = [_mul3(M, pT) for M in (Ra, Rb, Rg)]
        dot = lambda a, b: (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]).astype(np.float32)
        one, half = f32(1.0), f32(0.5)
        # point to plane
        wD = np.maximum(f32(0.0), half * ((one - dDist / f32(prm["distThres"])) + (one - p_in[:, 2] / f32(prm["sensorMaxDepth"])))).astype(np.float32)
        J = np.stack([-dot(tn, phis[0]), -dot(tn, phis[1]), -dot(tn, phis[2]), -tn[:, 0], -tn[:, 1], -tn[:, 2]], -1).astype(np.float32)
        r = dot(tn, diff)
        dterm[idx] = _row_terms(J, r, f32(prm["weightDepth"]) * wD)
        dmask[idx] = True
        # colour
        dI = (it[:, 0] - inp_i.reshape(N)[idx]).astype(np.float32)
        gu, gv = it[:, 1], it[:, 2]
        absDI = np.sqrt(dI * dI)
        csel = (absDI <= f32(prm["colorThres"])) & (np.sqrt(gu * gu + gv * gv) > f32(prm["colorGradientMin"]))
        wC = np.maximum(f32(0.0), one - absDI / f32(prm["colorThres"])).astype(np.float32)
        iz, wSq = one / pp[:, 2], pp[:, 2] * pp[:, 2]
        d0, d1 = gu * iz, gv * iz
        d2 = gu * (-pp[:, 0] / wSq) + gv * (-pp[:, 1] / wSq)
        g = np.stack([d0 * fx, d1 * fy, d0 * mx + d1 * my + d2], -1).astype(np.float32)
        Jc = np.stack([dot(g, phis[0]), dot(g, phis[1]), dot(g, phis[2]), g[:, 0], g[:, 1], g[:, 2]], -1).astype(np.float32)
        cterm[idx[csel]] = _row_terms(Jc[csel], dI[csel], (f32(prm["weightColor"]) * wC)[csel])
        cmask[idx[csel]] = True
    return dterm, cterm, dmask, cmask


def _row_terms(J, r, w):
    """addToLocalSystem (.cu:78-104) for one row per pixel"""
    out = np.zeros((len(J), TERMS), np.float32)
    at = 0
    for i in range(6):
        for j in range(i, 6):
            out[:, at + j - i] = J[:, i] * J[:, j] * w
        at += 6 - i
        out[:, 21 + i] = J[:, i] * r * w
    out[:, 27] = w * (r * r)
    out[:, 28] = w
    out[:, 29] = 1.0
    return out


def lane_sums(dterm, cterm, win, lanes=None):
    """each lane's window of `win` pixels summed in order from zero, per pixel the depth row and then the colour row, the
    J^T F products subtracted (.cu:92-103) -> (lanes, 30) float32; lanes defaults to ceil(N / win)"""
    N = len(dterm)
    lanes = -(-N // win) if lanes is None else lanes
    D = np.zeros((lanes * win, TERMS), np.float32)
    Cc = np.zeros((lanes * win, TERMS), np.float32)
    D[:N], Cc[:N] = dterm, cterm
    D, Cc = D.reshape(lanes, win, TERMS), Cc.reshape(lanes, win, TERMS)
    acc = np.zeros((lanes, TERMS), np.float32)
    for w in range(win):
        for T in (D, Cc):
            acc[:, :21] += T[:, w, :21]
            acc[:, 21:27] -= T[:, w, 21:27]
            acc[:, 27:] += T[:, w, 27:]
    return acc


def build_partials(H, W, level, dterm, cterm):
    """the lanes' windows in order (depth row, then colour row per pixel), the wave tree -> (nP, 30) float32"""
    win = window(level)
    nP = -(-(W * H) // (64 * win))
    acc = lane_sums(dterm, cterm, win, lanes=nP * 64).reshape(nP, 64, TERMS)
    off = 32
    while off > 0:
        acc[:, :off] += acc[:, off:2 * off]
        off //= 2
    return acc[:, 0].copy()


def sum_partials(partials):
    """reductionSystemCPU: in order, float32"""
    return np.cumsum(partials.astype(np.float32), axis=0, dtype=np.float32)[-1] if len(partials) else np.zeros(TERMS, np.float32)


def terms_to_system(t):
    ata = np.zeros((6, 6))
    at = 0
    for r in range(6):
        for c in range(r, 6):
            ata[r, c] = ata[c, r] = t[at + c - r]
        at += 6 - r
    return ata, t[21:27].astype(np.float64)


def delinearize(x):
    """R = Rz(x0) Ry(x1) Rx(x2) in the closed form the kernel uses"""
    cz, sz, cy, sy, cx, sx = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    return np.array([cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx,
                     sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx,
                     -sy, cy * sx, cy * cx], np.float32)


def level_params(ts, level, cp):
    lf = f32(2.0 ** level)
    return dict(fx=f32(cp.fx) / lf, fy=f32(cp.fy) / lf, mx=f32(cp.mx) / lf, my=f32(cp.my) / lf,
                weightDepth=ts.s_weightsDepth[level], weightColor=ts.s_weightsColor[level], distThres=ts.base.s_distThres[level],
                normalThres=ts.base.s_normalThres[level], sensorMaxDepth=cp.m_sensorDepthWorldMax,
                colorGradientMin=ts.s_colorGradientMin[level], colorThres=ts.s_colorThres[level])


def pyramids(inp, inp_n, inp_col, model, model_n, model_col, levels):
    """applyCT :264-284 -> per level (input pos, normals, intensity (filtered above 0), model pos, normals, I+dI)"""
    ins = [(np.ascontiguousarray(inp, np.float32), np.ascontiguousarray(inp_n, np.float32))] + icp.pyramid(inp, levels)
    mods = [(np.ascontiguousarray(model, np.float32), np.ascontiguousarray(model_n, np.float32))] + icp.pyramid(model, levels)
    ii, mi = [intensity(inp_col)], [intensity(model_col)]
    iif, miad = [ii[0]], [intensity_and_derivatives(mi[0])]
    for lv in range(levels - 1):
        h, w = ii[lv].shape
        w1, h1 = w // 2, h // 2
        ii.append(O.image_op("resample_float_map", ii[lv], w, h, out_size=(w1, h1)))
        iif.append(O.image_op("gauss_filter_float_map", ii[-1], w1, h1, 3.0, 1.0))
        mi.append(O.image_op("resample_float_map", mi[lv], w, h, out_size=(w1, h1)))
        miad.append(intensity_and_derivatives(O.image_op("gauss_filter_float_map", mi[-1], w1, h1, 3.0, 1.0)))
    return [(ins[lv][0], ins[lv][1], iif[lv], mods[lv][0], mods[lv][1], miad[lv]) for lv in range(levels)]


def apply_ct(inp, inp_n, inp_col, model, model_n, model_col, last_transform, ts, delta_estimate, cp, levels):
    """-> (4x4 pose or None if lost, info dict)"""
    pyr = pyramids(inp, inp_n, inp_col, model, model_n, model_col, levels)
    delta = np.asarray(delta_estimate, np.float32).reshape(4, 4).copy()
    info = dict(iterations=0, numCorr=0)
    for level in range(levels - 1, -1, -1):
        maps = pyr[level]
        H, W = maps[0].shape[:2]
        prm = level_params(ts, level, cp)
        last_err = f32(-1.0)
        for _ in range(int(ts.base.s_maxOuterIter[level])):
            angles = euler_angles_zyx(delta[:3, :3])
            trans = delta[:3, 3].copy()
            dterm, cterm, _, _ = pixel_terms(*maps, angles, trans, prm)
            t = sum_partials(build_partials(H, W, level, dterm, cterm))
            info["iterations"] += 1
            info.update(sumRegError=float(t[27]), sumRegWeight=float(t[28]), numCorr=int(t[29]))
            ata, atb = terms_to_system(t)
            if icp.is_zero(t[:21]):  # ATA.isZero(): the 21 distinct entries of the symmetric ATA
                return None, info
            x, cond = icp.solve(ata, atb)
            info["matrixCondition"] = cond
            xn = np.concatenate([angles, trans]).astype(np.float32) + x.astype(np.float32)
            R = delinearize(xn)
            tn = np.sqrt(xn[3] * xn[3] + xn[4] * xn[4] + xn[5] * xn[5])
            if not (angle_axis_angle(R) <= f32(ts.base.s_angleTransThres[level])) or not (tn <= f32(ts.base.s_distTransThres[level])):
                return None, info
            delta = np.eye(4, dtype=np.float32)
            delta[:3, :3] = R.reshape(3, 3)
            delta[:3, 3] = xn[3:6]
            err = f32(t[27])
            done = abs(last_err - err) < f32(ts.base.s_residualEarlyOut[level])
            last_err = err
            if done:
                break
    info["delta"] = delta
    return (np.asarray(last_transform, np.float32).reshape(4, 4) @ delta).astype(np.float32), info
