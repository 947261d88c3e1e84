"""Crafted 37x29 maps for the two camera trackers' per-pixel rules (tests/test_tracker_pinning.py on the CPU,
tests/test_gpu_tracker_reference.py on the device).  numpy only; everything is built by the code below.

37x29 has no side that is a multiple of a 16x16 tile and is 1.4 waves of 64 * 12 pixels.  The base is a slanted plane
seen from the camera, every pixel its own depth, the target equal to the input -- so under the identity every base pixel
pairs with itself, and which target a pixel took can be read off the position it was given.  On top of it single
pixels are placed by hand, one per rule that a kernel and its restatement could misread together; `classes` names them:

    name -> dict(pixels=[(x, y) of input pixels], expect=...)

What `expect` means is up to the test, which reads it off the REFERENCE's output (paired with which target pixel, not
paired, how many rows).  All of it is stated for the identity estimate; under another estimate the maps are still a
37x29 input with holes, points behind the camera and pixels that project off the image.
"""
import numpy as np

MINF = np.float32(-np.inf)
f32 = np.float32
W, H = 37, 29


def _bp(k, sx, sy, z):
    """the camera-space point (float32 x, y, z, 1) that projects to screen (sx, sy) at depth z; k = (fx, fy, mx, my)"""
    fx, fy, mx, my = (float(v) for v in k)
    return np.array([(sx - mx) / fx * z, (sy - my) / fy * z, z, 1.0], dtype=np.float32)


def _base(k, lf):
    """target = input: pixel (x, y) of the level holds the point behind full-resolution screen pixel
    (lf x + lf - 1, lf y + lf - 1) -- odd for lf 2 and 4, so that screenPos / levelFactor has a fraction to drop"""
    tgt = np.empty((H, W, 4), np.float32)
    for y in range(H):
        for x in range(W):
            tgt[y, x] = _bp(k, lf * x + lf - 1, lf * y + lf - 1, 1.0 + 0.01 * x + 0.003 * y)
    nrm = np.zeros((H, W, 4), np.float32)
    nrm[..., 2] = -1.0
    return tgt, nrm


def depth_maps(cp, lf, dist_thres, normal_thres):
    """-> dict(inp, inp_n, tgt, tgt_n, classes) for projectiveCorrespondences at levelFactor lf under the full-resolution
    camera cp (the maps are the 37x29 level), and for buildLinearSystem on its output"""
    k = (cp.fx, cp.fy, cp.mx, cp.my)
    tgt, tgt_n = _base(k, lf)
    inp, inp_n = tgt.copy(), tgt_n.copy()
    centre = lambda x, y: (lf * x + lf - 1, lf * y + lf - 1)
    cls = {}
    # holes, as a sensor leaves them
    inp[2, 2] = MINF
    inp_n[2, 3] = MINF
    cls["input_invalid"] = dict(pixels=[(2, 2), (3, 2)], expect=None)
    # a projection in (-1, 0): cameraToKinectScreenInt truncates it to 0, which is inside the image
    inp[3, 5] = _bp(k, -0.9, centre(0, 3)[1], tgt[3, 0, 2])
    cls["neg_x"] = dict(pixels=[(5, 3)], expect=(0, 3))
    inp[5, 7] = _bp(k, centre(7, 0)[0], -0.9, tgt[0, 7, 2])
    cls["neg_y"] = dict(pixels=[(7, 5)], expect=(7, 0))
    # the last column and row, and the first screen position past them
    inp[4, 9] = _bp(k, lf * W - 0.6, centre(0, 4)[1], tgt[4, W - 1, 2])
    cls["last_col"] = dict(pixels=[(9, 4)], expect=(W - 1, 4))
    inp[4, 11] = _bp(k, lf * W - 0.4, centre(0, 4)[1], tgt[4, W - 1, 2])
    inp[6, 13] = _bp(k, centre(13, 0)[0], lf * H - 0.6, tgt[H - 1, 13, 2])
    cls["last_row"] = dict(pixels=[(13, 6)], expect=(13, H - 1))
    inp[6, 15] = _bp(k, centre(15, 0)[0], lf * H - 0.4, tgt[H - 1, 15, 2])
    cls["past_the_image"] = dict(pixels=[(11, 4), (15, 6)], expect=None)
    # pTransInput.z <= 0: z = 0 divides by zero; z < 0 projects through the pinhole onto a target that holds the very
    # same point -- the reference has no z > 0 test here (it is commented out), so that pixel pairs
    inp[8, 17] = [0.1, 0.1, 0.0, 1.0]
    cls["z_zero"] = dict(pixels=[(17, 8)], expect=None)
    inp[8, 19] = _bp(k, *centre(21, 10), -1.0)
    tgt[10, 21] = inp[8, 19]
    cls["z_negative"] = dict(pixels=[(19, 8)], expect=(21, 10))
    # a valid target position under an invalid target normal, and the reverse
    tgt_n[12, 23] = MINF
    tgt[12, 25] = MINF
    cls["target_half_valid"] = dict(pixels=[(23, 12), (25, 12)], expect=None)
    # d == distThres exactly, and one ulp above: same x and y, depths whose float32 difference is exact
    thr = f32(dist_thres)
    zt = f32(0.1875)
    zi = f32(zt + thr)
    zt_above = np.nextafter(zt, f32(0.0))
    assert f32(zi - zt) == thr and f32(zi - zt_above) == np.nextafter(thr, f32(np.inf)), "no exact pair for this distThres"
    for (x, y), z in (((27, 14), zt), ((29, 14), zt_above)):
        inp[y, x] = _bp(k, *centre(x, y), zi)
        tgt[y, x] = inp[y, x]
        tgt[y, x, 2] = z
    cls["dist_at_thres"] = dict(pixels=[(27, 14)], expect=(27, 14))
    cls["dist_one_ulp_above"] = dict(pixels=[(29, 14)], expect=None)
    # dNormal == normalThres exactly, and one ulp below: the target normal is (0, 0, -1), so the dot is -n.z
    nthr = f32(normal_thres)
    inp_n[16, 31] = [0.2, 0.0, -nthr, 0.0]
    inp_n[16, 33] = [0.2, 0.0, -np.nextafter(nthr, f32(0.0)), 0.0]
    cls["normal_at_thres"] = dict(pixels=[(31, 16)], expect=(31, 16))
    cls["normal_one_ulp_below"] = dict(pixels=[(33, 16)], expect=None)
    # beyond m_sensorDepthWorldMax: the pair weight clamps to 0, and the row still counts
    inp[20, 4] = _bp(k, *centre(4, 20), 2.5 * cp.m_sensorDepthWorldMax)
    tgt[20, 4] = inp[20, 4]
    cls["weight_zero"] = dict(pixels=[(4, 20)], expect=(4, 20))
    return dict(inp=inp, inp_n=inp_n, tgt=tgt, tgt_n=tgt_n, classes=cls)


def _on_the_pixel(k, x, y):
    """a point at depth 1 whose float32 projection (fx X + 0 Y + mx z) / z is EXACTLY (x, y): the bilinear weights are
    then 0 and 1 and the interpolated value is the texel's own bits"""
    fx, fy, mx, my = (f32(v) for v in k)
    out = []
    for f, m, s in ((fx, mx, x), (fy, my, y)):
        c = f32((s - float(m)) / float(f))
        for _ in range(4000):
            u = f32(f32(f * c) + f32(m * f32(1.0)))
            if u == f32(s):
                break
            c = np.nextafter(c, f32(np.inf) if u < s else f32(-np.inf))
        assert u == f32(s), "no float32 coordinate projects exactly onto the pixel"
        out.append(c)
    return np.array([out[0], out[1], 1.0, 1.0], np.float32)


def rgbd_maps(prm):
    """-> dict(inp, inp_n, inp_i, tgt, tgt_n, tgt_iad, classes) for computeNormalEquations on level 0; prm as
    rgbd_icp.level_params gives it.  `expect` is the number of rows (depth + colour) the pixel makes."""
    k = (prm["fx"], prm["fy"], prm["mx"], prm["my"])
    tgt, tgt_n = _base(k, 1)
    inp, inp_n = tgt.copy(), tgt_n.copy()
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    img = 0.5 + 0.2 * np.sin(0.5 * xs) * np.cos(0.4 * ys)
    tgt_iad = np.stack([img, 0.1 * np.cos(0.5 * xs) * np.cos(0.4 * ys), -0.08 * np.sin(0.5 * xs) * np.sin(0.4 * ys), np.ones_like(img)],
                       -1).astype(np.float32)
    inp_i = (img + 0.01).astype(np.float32)
    cls = {}
    inp[2, 2] = MINF
    inp_n[2, 3] = MINF
    inp_i[2, 4] = MINF
    cls["input_invalid"] = dict(pixels=[(2, 2), (3, 2), (4, 2)], expect=0)
    # pProjTrans(2) <= 0: no row, also where the target holds the very same point (the depth tracker pairs that one)
    inp[8, 17] = [0.1, 0.1, 0.0, 1.0]
    inp[8, 19] = _bp(k, 21, 10, -1.0)
    tgt[10, 21] = inp[8, 19]
    cls["z_not_positive"] = dict(pixels=[(17, 8), (19, 8)], expect=0)
    # the bilinear taps of the intensity map: one, two, three and four of them MINF (the nearest neighbour's position and
    # normal stay valid), and a tap set that hangs over each image border
    gone = {1: [(1, 1)], 2: [(1, 0), (1, 1)], 3: [(1, 0), (0, 1), (1, 1)], 4: [(0, 0), (1, 0), (0, 1), (1, 1)]}
    for n, tx in ((1, 5), (2, 10), (3, 15), (4, 20)):
        ty = 22
        inp[ty, tx] = _bp(k, tx + 0.3, ty + 0.4, tgt[ty, tx, 2])
        for dx, dy in gone[n]:
            tgt_iad[ty + dy, tx + dx] = MINF
        cls[f"taps_{n}_minf"] = dict(pixels=[(tx, ty)], expect=None if n < 4 else 0)
    inp[12, 1] = _bp(k, -0.3, 12.4, tgt[12, 0, 2])
    inp[1, 12] = _bp(k, 12.4, -0.3, tgt[0, 12, 2])
    inp[14, W - 2] = _bp(k, W - 1 + 0.3, 14.4, tgt[14, W - 1, 2])
    inp[H - 2, 14] = _bp(k, 14.4, H - 1 + 0.3, tgt[H - 1, 14, 2])
    cls["taps_over_the_border"] = dict(pixels=[(1, 12), (12, 1), (W - 2, 14), (14, H - 2)], expect=None)
    # |dI| at colorThres and one ulp above; the gradient norm at colorGradiantMin and one ulp above.  The input intensity
    # is 0 and the projection exact, so dI and the gradient are the texel's own numbers.
    cthr, gmin = f32(prm["colorThres"]), f32(prm["colorGradientMin"])
    up = lambda v: np.nextafter(f32(v), f32(np.inf))
    for name, (x, y), texel, rows in (("colour_at_thres", (26, 6), (cthr, 0.05, 0.0, 1.0), 2),
                                      ("colour_one_ulp_above", (29, 6), (up(cthr), 0.05, 0.0, 1.0), 1),
                                      ("gradient_at_min", (26, 10), (0.02, gmin, 0.0, 1.0), 1),
                                      ("gradient_one_ulp_above", (29, 10), (0.02, 0.0, up(gmin), 1.0), 2)):
        inp[y, x] = _on_the_pixel(k, x, y)
        tgt[y, x] = inp[y, x]
        inp_i[y, x] = 0.0
        tgt_iad[y, x] = texel
        cls[name] = dict(pixels=[(x, y)], expect=rows)
    # The geometric gate, which this kernel states for itself (.cu:131-157), with the constructions of depth_maps:
    # u + 0.5 or v + 0.5 in (-1, 0), which (int) truncates onto column / row 0; the last column and row, and the first
    # position past them
    inp[3, 5] = _bp(k, -0.9, 3, tgt[3, 0, 2])
    inp[5, 7] = _bp(k, 7, -0.9, tgt[0, 7, 2])
    cls["neg_x_neg_y"] = dict(pixels=[(5, 3), (7, 5)], expect=None)
    inp[4, 9] = _bp(k, W - 0.6, 4, tgt[4, W - 1, 2])
    inp[6, 13] = _bp(k, 13, H - 0.6, tgt[H - 1, 13, 2])
    cls["last_col_last_row"] = dict(pixels=[(9, 4), (13, 6)], expect=None)
    inp[4, 11] = _bp(k, W - 0.4, 4, tgt[4, W - 1, 2])
    inp[6, 15] = _bp(k, 15, H - 0.4, tgt[H - 1, 15, 2])
    cls["past_the_image"] = dict(pixels=[(11, 4), (15, 6)], expect=0)
    # dDist == distThres exactly and one ulp above; dNormal == normalThres exactly and one ulp below.  Under a rotation
    # the two normal pixels also show whether the input normal is rotated: ROld moves their dot product off the threshold.
    thr = f32(prm["distThres"])
    zt = f32(0.1875)
    zi = f32(zt + thr)
    zt_above = np.nextafter(zt, f32(0.0))
    assert f32(zi - zt) == thr and f32(zi - zt_above) == np.nextafter(thr, f32(np.inf)), "no exact pair for this distThres"
    for (x, y), z in (((27, 14), zt), ((29, 14), zt_above)):
        inp[y, x] = _bp(k, x, y, zi)
        tgt[y, x] = inp[y, x]
        tgt[y, x, 2] = z
    cls["dist_at_thres"] = dict(pixels=[(27, 14)], expect=None)
    cls["dist_one_ulp_above"] = dict(pixels=[(29, 14)], expect=0)
    nthr = f32(prm["normalThres"])
    inp_n[16, 31] = [0.2, 0.0, -nthr, 0.0]
    inp_n[16, 33] = [0.2, 0.0, -np.nextafter(nthr, f32(0.0)), 0.0]
    cls["normal_at_thres"] = dict(pixels=[(31, 16)], expect=None)
    cls["normal_one_ulp_below"] = dict(pixels=[(33, 16)], expect=0)
    return dict(inp=inp, inp_n=inp_n, inp_i=inp_i, tgt=tgt, tgt_n=tgt_n, tgt_iad=tgt_iad, classes=cls)
