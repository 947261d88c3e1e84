"""numpy restatement of the shaded view ("Rendering"): RenderDepthMap of DX11RGBDRenderer
(Shaders/RGBDRenderer.hlsl: RGBDRendererGS, ComputeQuadVertex, RGBDRendererRawDepthPS under D3D11's default rasterizer
state) and PhongPS of DX11PhongLighting (Shaders/PhongLighting.hlsl).  Every step is float32 in the kernels' order (no
fused multiply-add), coverage is int64 on the 1/256-pixel grid, so the raster keys and the four maps are bit-exact
against csrc/vh_view.hip.  TEST INFRASTRUCTURE ONLY.

Also a minimal PNG reader (zlib only) for the files renderToFile writes.
"""
import struct
import zlib

import numpy as np

f32 = np.float32
MINF = f32(-np.inf)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
DEPTH_WORLD_MIN, DEPTH_WORLD_MAX = f32(0.1), f32(8.0)
GUARD = f32(2.0 ** 28)  # 2^20 px on the 1/256 grid
CHUNK = 1 << 22         # candidate pixels per vectorised batch


# ------------------------------------------------------------------------------------------------------ vertices

def _load(img, x, y):
    """Texture2D::Load: 0 outside the image (x, y int64; -1 stands for the shader's wrapped uint)"""
    h, w = img.shape[:2]
    ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    v = img[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]
    if v.ndim > ok.ndim:
        return np.where(ok[..., None], v, f32(0))
    return np.where(ok, v, f32(0))


def _uint_as_float(x):
    """(float)x of the shader's uint (x - 1 at 0 is 2^32 - 1)"""
    return (np.asarray(x, np.int64) % (1 << 32)).astype(np.float32)


def _mat_vec(M, v):
    """mul(v, M) with M read column-major = M v, the sum over j = 0..3 left to right"""
    M = np.asarray(M, np.float32).reshape(4, 4)
    return [((M[i, 0] * v[0] + M[i, 1] * v[1]) + M[i, 2] * v[2]) + M[i, 3] * v[3] for i in range(4)]


def world_position(depth, p, x, y):
    """getWorldSpacePosition, hlsl:67-77 -> 4 arrays"""
    d = _load(depth, x, y)
    c = _mat_vec(p["intrinsicInverse"], (_uint_as_float(x) * d, _uint_as_float(y) * d, d, d))
    c = (c[0], c[1], c[3], np.ones_like(d))
    w = _mat_vec(p["modelview"], c)
    return [w[0] / w[3], w[1] / w[3], w[2] / w[3], w[3] / w[3]]


def vertex(depth, color, p, x, y):
    """ComputeQuadVertex, hlsl:79-111, and the viewport -> dict of arrays: X, Y (screen px), z, depth, pos, normal, color"""
    sw, sh = p["screenWidth"], p["screenHeight"]
    cc = world_position(depth, p, x, y)
    mc, cm = world_position(depth, p, x - 1, y), world_position(depth, p, x, y - 1)
    cp, pc = world_position(depth, p, x, y + 1), world_position(depth, p, x + 1, y)
    a = [cp[k] - cm[k] for k in range(3)]
    b = [pc[k] - mc[k] for k in range(3)]
    n = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    with np.errstate(divide="ignore", invalid="ignore"):
        ln = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        normal = [n[0] / ln, n[1] / ln, n[2] / ln, np.ones_like(ln)]
        clip = _mat_vec(p["intrinsicNew"], (cc[0], cc[1], cc[2], np.ones_like(cc[0])))
        px, py = clip[0] / clip[2], clip[1] / clip[2]
        fx = (px / f32(sw - 1)) * f32(2) - f32(1)
        fy = f32(1) - (py / f32(sh - 1)) * f32(2)
        z = (clip[2] - DEPTH_WORLD_MIN) / (DEPTH_WORLD_MAX - DEPTH_WORLD_MIN)
        X = ((fx + f32(1)) * f32(0.5)) * f32(sw)
        Y = ((f32(1) - fy) * f32(0.5)) * f32(sh)
    col = _load(color, x, y) if color is not None else np.zeros(np.shape(x) + (4,), np.float32)
    return dict(X=X, Y=Y, z=z, depth=_load(depth, x, y), pos=cc, normal=normal, color=[col[..., k] for k in range(4)])


def triangle_vertices(depth, color, p, prim):
    """the strip of quad prim // 2: (x, y+1), (x, y), (x+1, y+1), (x+1, y); triangle 0 = (v0, v1, v2), 1 = (v2, v1, v3)"""
    prim = np.asarray(prim, np.int64)
    q, t = prim >> 1, prim & 1
    w = p["depthWidth"]
    x, y = q % w, q // w
    return (vertex(depth, color, p, np.where(t == 1, x + 1, x), y + 1),
            vertex(depth, color, p, x, y),
            vertex(depth, color, p, x + 1, np.where(t == 1, y, y + 1)))


def quad_kept(depth, p, x, y):
    """RGBDRendererGS's drop rules, hlsl:122-137"""
    d = [_load(depth, x, y), _load(depth, x, y + 1), _load(depth, x + 1, y), _load(depth, x + 1, y + 1)]
    bad = np.zeros(np.shape(x), bool)
    for di in d:
        bad |= (di <= DEPTH_WORLD_MIN) | (di == MINF)
    dmax = np.fmax(np.fmax(d[0], d[1]), np.fmax(d[2], d[3]))
    dmin = np.fmin(np.fmin(d[0], d[1]), np.fmin(d[2], d[3]))
    dm = f32(0.5) * (dmax + dmin)
    with np.errstate(invalid="ignore"):
        far = (dmax - dmin) > (f32(p["depthThreshOffset"]) + f32(p["depthThreshLin"]) * dm)
    return ~bad & ~far


# ------------------------------------------------------------------------------------------------------ raster

def setup(v0, v1, v2):
    """snap to 1/256 px, guard band, back-face cull -> (kept, x (3, n) int64, y (3, n) int64, area)"""
    xs, ys, ok = [], [], None
    with np.errstate(invalid="ignore", over="ignore"):
        for v in (v0, v1, v2):
            sx, sy = np.rint(v["X"] * f32(256)), np.rint(v["Y"] * f32(256))
            good = (np.abs(sx) <= GUARD) & (np.abs(sy) <= GUARD)
            ok = good if ok is None else ok & good
            xs.append(np.where(good, sx, 0).astype(np.int64))
            ys.append(np.where(good, sy, 0).astype(np.int64))
    x, y = np.stack(xs), np.stack(ys)
    area = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
    return ok & (area > 0), x, y, area


def cover(x, y, px, py):
    """edge functions with the top-left rule -> (covered, e (3, n)); e[k] is the weight of vertex k"""
    es, cov = [], None
    for k, (a, b) in enumerate(((1, 2), (2, 0), (0, 1))):
        dx, dy = x[b] - x[a], y[b] - y[a]
        e = dx * (py - y[a]) - dy * (px - x[a])
        tl = (dy < 0) | ((dy == 0) & (dx > 0))
        c = (e > 0) | ((e == 0) & tl)
        cov = c if cov is None else cov & c
        es.append(e)
    return cov, np.stack(es)


def bary(e, area):
    a = area.astype(np.float32)
    return [e[k].astype(np.float32) / a for k in range(3)]


def interp(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def box(x, y, sw, sh):
    """pixels whose centre i * 256 + 128 may lie in the triangle, clipped to the screen"""
    lx = np.maximum(0, -((128 - x.min(0)) >> 8))
    hx = np.minimum(sw - 1, (x.max(0) - 128) >> 8)
    ly = np.maximum(0, -((128 - y.min(0)) >> 8))
    hy = np.minimum(sh - 1, (y.max(0) - 128) >> 8)
    return lx, hx, ly, hy


def rasterize(x, y, area, z3, prim, sw, sh, keys):
    """atomicMin of (float_bits(z) << 32 | prim) into keys (sw * sh uint64) for every covered pixel with 0 <= z < 1"""
    lx, hx, ly, hy = box(x, y, sw, sh)
    bw, bh = np.maximum(hx - lx + 1, 0), np.maximum(hy - ly + 1, 0)
    n = bw * bh
    live = np.nonzero(n > 0)[0]
    start = 0
    while start < len(live):
        # a batch of triangles whose boxes hold at most CHUNK pixels (at least one triangle)
        cs = np.cumsum(n[live[start:]])
        stop = start + max(1, int(np.searchsorted(cs, CHUNK, side="right")))
        t = live[start:stop]
        cnt = n[t]
        ti = np.repeat(np.arange(len(t)), cnt)
        local = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        tt = t[ti]
        i = lx[tt] + local % bw[tt]
        j = ly[tt] + local // bw[tt]
        cov, e = cover(x[:, tt], y[:, tt], i * 256 + 128, j * 256 + 128)
        b = bary(e, area[tt])
        z = interp([z3[k][tt] for k in range(3)], b) + f32(0)
        keep = cov & (z >= 0) & (z < 1)
        key = (z[keep].view(np.uint32).astype(np.uint64) << np.uint64(32)) | prim[tt][keep].astype(np.uint64)
        np.minimum.at(keys, (j[keep] * sw + i[keep]).astype(np.int64), key)
        start = stop
    return keys


def raster(depth, p):
    """k_view_raster + k_view_raster_large: the key buffer (screenHeight, screenWidth) uint64"""
    h, w = depth.shape
    sw, sh = p["screenWidth"], p["screenHeight"]
    q = np.arange(w * h, dtype=np.int64)
    q = q[quad_kept(depth, p, q % w, q // w)]
    prim = np.concatenate([2 * q, 2 * q + 1])
    v = triangle_vertices(depth, None, p, prim)
    ok, x, y, area = setup(*v)
    keys = np.full(sw * sh, EMPTY, np.uint64)
    z3 = [vi["z"][ok] for vi in v]
    rasterize(x[:, ok], y[:, ok], area[ok], z3, prim[ok], sw, sh, keys)
    return keys.reshape(sh, sw)


def resolve(depth, color, p, keys):
    """k_view_resolve: -> dict depth (H, W), positions / normals / colors (H, W, 4) with the reference's clear values"""
    sw, sh = p["screenWidth"], p["screenHeight"]
    keys = keys.reshape(-1)
    out_d = np.full(sw * sh, MINF, np.float32)
    clear = np.array([MINF, MINF, MINF, 1], np.float32)
    maps = {k: np.tile(clear, (sw * sh, 1)) for k in ("positions", "normals", "colors")}
    pix = np.nonzero(keys != EMPTY)[0]
    if len(pix):
        prim = (keys[pix] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        v = triangle_vertices(depth, color, p, prim)
        _, x, y, area = setup(*v)
        _, e = cover(x, y, (pix % sw) * 256 + 128, (pix // sw) * 256 + 128)
        b = bary(e, area)
        out_d[pix] = interp([vi["depth"] for vi in v], b)
        for name, attr in (("positions", "pos"), ("normals", "normal"), ("colors", "color")):
            maps[name][pix] = np.stack([interp([vi[attr][c] for vi in v], b) for c in range(4)], -1)
    out = {k: m.reshape(sh, sw, 4) for k, m in maps.items()}
    out["depth"] = out_d.reshape(sh, sw)
    return out


def render_depth_map(depth, color, p):
    """RenderDepthMap -> (keys, maps)"""
    depth = np.asarray(depth, np.float32)
    color = np.asarray(color, np.float32) if color is not None else None
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):  # -inf depths and colours propagate as in the kernels
        keys = raster(depth, p)
        return keys, resolve(depth, color, p, keys)


def view_params(intrinsic_inverse, modelview, intrinsic_new, depth_size, screen_size, thres_offset=0.012, thres_lin=0.001):
    """the dict form of VhViewParams this module reads"""
    return dict(intrinsicInverse=np.asarray(intrinsic_inverse, np.float32).reshape(4, 4),
                modelview=np.asarray(modelview, np.float32).reshape(4, 4),
                intrinsicNew=np.asarray(intrinsic_new, np.float32).reshape(4, 4),
                depthWidth=int(depth_size[0]), depthHeight=int(depth_size[1]), screenWidth=int(screen_size[0]),
                screenHeight=int(screen_size[1]), depthThreshOffset=f32(thres_offset), depthThreshLin=f32(thres_lin))


def intrinsics(fx, fy, mx, my):
    m = np.eye(4, dtype=np.float32)
    m[0, 0], m[1, 1], m[0, 2], m[1, 2] = fx, fy, mx, my
    return m


def inverse(m):
    return np.linalg.inv(np.asarray(m, np.float64)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------ Phong

def _normalize(v):
    ln = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    return [v[0] / ln, v[1] / ln, v[2] / ln]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def phong(positions, normals, colors, use_material, light):
    """PhongPS, PhongLighting.hlsl:49-86 -> float4 (..., 4); light: a PhongLight (or anything with its fields)"""
    L = {k: np.asarray(getattr(light, k)[:] if hasattr(getattr(light, k), "__len__") else getattr(light, k), np.float32)
         for k in ("lightAmbient", "lightDiffuse", "lightSpecular", "lightDirection", "materialShininess", "materialAmbient",
                   "materialSpecular", "materialDiffuse")}
    P, N, Cc = (np.asarray(a, np.float32) for a in (positions, normals, colors))
    valid = (P[..., 0] != MINF) & (Cc[..., 0] != MINF) & (N[..., 0] != MINF)
    with np.errstate(all="ignore"):
        position = [P[..., k] for k in range(3)]
        normal = [N[..., k] for k in range(3)]
        ld = _normalize([L["lightDirection"][k] for k in range(3)])
        eye = _normalize(position)
        i = [-ld[k] for k in range(3)]
        t = f32(2) * _dot(normal, i)
        R = _normalize([i[k] - t * normal[k] for k in range(3)])
        diff = np.fmax(_dot(normal, i), f32(0))
        spec = np.power(np.fmax(_dot(R, eye), f32(0)), L["materialShininess"]).astype(np.float32)
        out = np.empty(P.shape[:-1] + (4,), np.float32)
        for k in range(4):
            if use_material:
                material = Cc[..., k] if k < 3 else f32(1)
                out[..., k] = (L["lightDiffuse"][k] * material * diff + L["lightSpecular"][k] * L["materialSpecular"][k] * spec) * f32(2)
            else:
                out[..., k] = (L["lightAmbient"][k] * L["materialAmbient"][k] + L["lightDiffuse"][k] * L["materialDiffuse"][k] * diff) \
                    + L["lightSpecular"][k] * L["materialSpecular"][k] * spec
    out[~valid] = MINF
    return out


def unorm8(c):
    """D3D FLOAT -> UNORM8: NaN -> 0, clamp to [0, 1], x 255, round to nearest even"""
    c = np.asarray(c, np.float32)
    c = np.where(np.isnan(c), f32(0), np.clip(c, f32(0), f32(1)))
    return np.rint(c * f32(255)).astype(np.uint8)


def rgba8(out4, alpha_rule=True):
    b = unorm8(out4)
    if alpha_rule:
        b[(b[..., :3] > 0).any(-1), 3] = 255
    return b


def rgba8_boundary(out4, tol=1e-5):
    """where a channel's float value lies within tol of a rounding boundary of the x 255 grid (an RGBA8 value may then
    differ by one between two pow implementations)"""
    c = np.where(np.isnan(out4), f32(0), np.clip(out4, 0, 1)).astype(np.float64) * 255.0
    return np.abs(c - np.floor(c) - 0.5) <= tol * 255.0


# ------------------------------------------------------------------------------------------------------ PNG

def read_png_rgba8(path):
    """an 8-bit RGBA, non-interlaced PNG -> (H, W, 4) uint8; every filter type of the specification"""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "not a PNG"
    pos, idat, hdr = 8, [], None
    while pos < len(data):
        n, typ = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        crc = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]
        assert zlib.crc32(typ + body) & 0xFFFFFFFF == crc, typ
        if typ == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif typ == b"IDAT":
            idat.append(body)
        elif typ == b"IEND":
            break
        pos += 12 + n
    W, H, depth, ctype, comp, filt, inter = hdr
    assert (depth, ctype, comp, filt, inter) == (8, 6, 0, 0, 0), hdr
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8).reshape(H, W * 4 + 1)
    out = np.zeros((H, W * 4), np.int32)
    for r in range(H):
        ft, line = raw[r, 0], raw[r, 1:].astype(np.int32)
        prev = out[r - 1] if r else np.zeros(W * 4, np.int32)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 255
        else:  # 1 (sub), 3 (average), 4 (Paeth) depend on the pixel to the left
            cur = np.zeros(W * 4, np.int32)
            for k in range(W * 4):
                a = cur[k - 4] if k >= 4 else 0
                b, c = prev[k], (prev[k - 4] if k >= 4 else 0)
                if ft == 1:
                    pred = a
                elif ft == 3:
                    pred = (a + b) // 2
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cur[k] = (line[k] + pred) & 255
        out[r] = cur
    return out.astype(np.uint8).reshape(H, W, 4)
