"""The shaded view of the model: RenderDepthMap (DX11RGBDRenderer), PhongPS (DX11PhongLighting) and renderToFile.

CPU: the rendering keys of a parameter file; the new structs against their ctypes mirrors; the PNG writer read back by
an independent decoder (Python's zlib); the numpy restatement's own cases (tests/view_render.py).
GPU: the key buffer and the four maps bit for bit against the restatement, on synthetic depth maps and on a ray cast of
S1, from several views (one of them magnified, so the large-triangle path runs); Phong in both modes; the handle-level
classes; tools/replay.py --render-to end to end."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import view_render as V
from voxelhashing_amd import synth, vhtypes as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINF = np.float32(-np.inf)

# the rendering block of DepthSensingCUDA's zParametersDefault.txt, inlined (data only)
RENDER_BLOCK = b"""// rendering
s_materialShininess 	= 16.0f;
s_materialAmbient   	= 0.75f 0.65f 0.5f 1.0f;
s_materialDiffuse 		= 1.0f 0.9f 0.7f 1.0f;
s_materialSpecular 		= 1.0f 1.0f 1.0f 1.0f;
s_lightAmbient 			= 0.4f 0.4f 0.4f 1.0f;
s_lightDiffuse 			= 0.6f 0.52944f 0.4566f 0.6f;
s_lightSpecular 		= 0.3f 0.3f 0.3f 1.0f;
s_lightDirection 		= 0.0f -1.0f 2.0f;

s_RenderMode = 1;

s_useColorForRendering = false;
s_playData = true;

s_renderingDepthDiscontinuityThresOffset = 0.012f;	// discontinuity offset in meter
s_renderingDepthDiscontinuityThresLin	 = 0.001f;	// additional discontinuity threshold per meter
s_remappingDepthDiscontinuityThresOffset = 0.012f;	// discontinuity offset in meter
s_remappingDepthDiscontinuityThresLin	 = 0.01f;	// additional discontinuity threshold per meter
s_renderToFile = false;				//for making paper videos: renders all input/raycasts etc. to images
s_renderToFileDir = "./output/";
"""


def default_light():
    from voxelhashing_amd import engine as E, reconstruction as R
    return E.phong_light_from_render_state(R.read_render_state(RENDER_BLOCK))


def same_bits(a, b):
    """bit-equal float arrays, any NaN equal to any NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


# ---------------------------------------------------------------------------------------------------------- CPU

def test_render_state_reader():
    from voxelhashing_amd import reconstruction as R
    rs = R.read_render_state(RENDER_BLOCK)
    assert rs.numKeysFound == 13
    assert rs.s_materialShininess == 16.0
    assert list(rs.s_materialAmbient) == [np.float32(v) for v in (0.75, 0.65, 0.5, 1.0)]
    assert list(rs.s_lightDiffuse) == [np.float32(v) for v in (0.6, 0.52944, 0.4566, 0.6)]
    assert list(rs.s_lightDirection) == [0.0, -1.0, 2.0]
    assert rs.s_useColorForRendering == 0 and rs.s_renderToFile == 0
    assert rs.s_renderingDepthDiscontinuityThresOffset == np.float32(0.012) and rs.s_renderingDepthDiscontinuityThresLin == np.float32(0.001)
    assert bytes(rs.s_renderToFileDir) == b"./output/"
    # missing keys are value-initialised, as VhAppState's are
    rs = R.read_render_state(b"s_renderToFile = true;\ns_lightAmbient = 0.1f 0.2f 0.3f 0.4f;\n")
    assert rs.numKeysFound == 2 and rs.s_renderToFile == 1 and list(rs.s_lightAmbient) == [np.float32(v) for v in (0.1, 0.2, 0.3, 0.4)]
    assert rs.s_materialShininess == 0.0 and list(rs.s_materialDiffuse) == [0.0] * 4 and bytes(rs.s_renderToFileDir) == b""
    # the file form, and the reference's full default file (the block is there in the same form)
    rs = R.read_render_state(os.path.join(ROOT, "tests", "golden", "reference", "zParametersDefault.txt"))
    assert rs.numKeysFound == 13 and rs.s_materialShininess == 16.0
    light = default_light()
    assert list(light.lightDirection) == [0.0, -1.0, 2.0] and light.materialShininess == 16.0
    assert list(light.materialAmbient) == list(R.read_render_state(RENDER_BLOCK).s_materialAmbient)


def test_render_struct_layouts():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "vh_types.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(VhRenderState), offsetof(VhRenderState, s_lightDirection),
         offsetof(VhRenderState, s_useColorForRendering), offsetof(VhRenderState, s_renderingDepthDiscontinuityThresLin),
         offsetof(VhRenderState, s_renderToFile), offsetof(VhRenderState, s_renderToFileDir), offsetof(VhRenderState, numKeysFound));
  printf("%zu %zu %zu %zu\n", sizeof(VhPhongLight), offsetof(VhPhongLight, lightDirection), offsetof(VhPhongLight, materialShininess),
         offsetof(VhPhongLight, materialDiffuse));
  printf("%zu %zu %zu %zu %zu\n", sizeof(VhViewParams), offsetof(VhViewParams, modelview), offsetof(VhViewParams, depthWidth),
         offsetof(VhViewParams, screenHeight), offsetof(VhViewParams, depthThreshLin));
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [list(map(int, line.split())) for line in subprocess.check_output([exe]).decode().split("\n") if line.strip()]
    R, P, Q = T.RenderState, T.PhongLight, T.ViewParams
    assert got[0] == [C.sizeof(R), R.s_lightDirection.offset, R.s_useColorForRendering.offset, R.s_renderingDepthDiscontinuityThresLin.offset,
                      R.s_renderToFile.offset, R.s_renderToFileDir.offset, R.numKeysFound.offset]
    assert got[1] == [C.sizeof(P), P.lightDirection.offset, P.materialShininess.offset, P.materialDiffuse.offset]
    assert got[2] == [C.sizeof(Q), Q.modelview.offset, Q.depthWidth.offset, Q.screenHeight.offset, Q.depthThreshLin.offset]


def test_png_round_trip(tmp_path):
    from voxelhashing_amd import engine as E
    rng = np.random.default_rng(3)
    for W, H, level in ((1, 1, -1), (37, 23, 1), (160, 120, 9), (5, 200, 0)):
        img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
        img[: H // 2, : W // 2] = (10, 20, 30, 255)  # runs that deflate
        path = str(tmp_path / f"{W}x{H}.png")
        E.write_png_rgba8(path, img, level)
        assert np.array_equal(V.read_png_rgba8(path), img)
    from voxelhashing_amd import lib
    assert lib.load().vh_write_png_rgba8(str(tmp_path / "x.png").encode(), 0, 4, img.ctypes.data, -1) != 0  # an empty image is refused
    assert not os.path.exists(tmp_path / "x.png")


def test_input_images_on_the_host():
    from voxelhashing_amd import reconstruction as R
    rgbx = np.array([[[0, 0, 0, 7], [1, 0, 0, 0], [0, 0, 200, 9]]], np.uint8)
    assert R.rgbx_alpha_rule(rgbx).tolist() == [[[0, 0, 0, 7], [1, 0, 0, 255], [0, 0, 200, 255]]]
    d = np.array([[1.0, 2.0, 3.0, MINF, 0.0]], np.float32)
    img = R.depth_image_rgba8(d)
    # min 0 (0 is a value, not -inf), max 3: x = 1 - d / 3; hue 240 x; 0 and -inf become black and transparent
    assert img[0, 3].tolist() == [0, 0, 0, 0] and img[0, 4].tolist() == [0, 0, 0, 0]
    assert img[0, 2].tolist() == [127, 0, 0, 255]           # x = 0: hue 0, red
    assert img[0, 1, 3] == 255 and img[0, 0, 2] > img[0, 0, 0]  # nearer is bluer


def _plane_case(W=64, H=48, depth=1.0):
    K = V.intrinsics(50, 50, (W - 1) / 2, (H - 1) / 2)
    return np.full((H, W), depth, np.float32), K


def test_restatement_plane_covers_the_screen():
    d, K = _plane_case()
    H, W = d.shape
    col = np.random.default_rng(0).random((H, W, 4)).astype(np.float32)
    keys, m = V.render_depth_map(d, col, V.view_params(V.inverse(K), np.eye(4), K, (W, H), (W, H)))
    # the mesh spans vertex 0 .. W-1, which the shader's viewport maps to 0 .. W px: every pixel centre is covered
    assert np.all(keys != V.EMPTY)
    assert np.allclose(m["depth"], 1.0, atol=1e-6) and np.allclose(m["positions"][..., 2], 1.0, atol=1e-6)
    assert np.allclose(m["normals"][5:-5, 5:-5], [0, 0, -1, 1], atol=1e-6)
    z = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    assert np.allclose(z, (np.float32(1.0) - np.float32(0.1)) / (np.float32(8.0) - np.float32(0.1)), rtol=0, atol=1e-7)
    # the winner is the pixel's own quad (x, y) = floor(centre * (W - 1) / W)
    prim = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    j, i = np.mgrid[0:H, 0:W]
    assert np.array_equal(prim // 2, ((j + 0.5) * (H - 1) / H).astype(int) * W + ((i + 0.5) * (W - 1) / W).astype(int))


def test_restatement_depth_step_leaves_a_gap():
    d, K = _plane_case()
    H, W = d.shape
    d[:, W // 2:] = 1.5
    p = V.view_params(V.inverse(K), np.eye(4), K, (W, H), (W, H))
    keys, m = V.render_depth_map(d, None, p)
    gap = np.nonzero(np.all(keys == V.EMPTY, axis=0))[0]
    assert len(gap) and np.all(np.abs(gap - (W // 2 - 0.5)) < 2), gap
    assert np.all(m["depth"][:, gap] == MINF) and np.all(m["positions"][:, gap] == [MINF, MINF, MINF, 1])
    # under the threshold the step is drawn
    keys, _ = V.render_depth_map(d, None, V.view_params(V.inverse(K), np.eye(4), K, (W, H), (W, H), thres_offset=1.0))
    assert np.all(keys != V.EMPTY)


def test_restatement_back_faces_are_culled():
    d, K = _plane_case()
    H, W = d.shape
    behind = np.diag([-1.0, 1.0, -1.0, 1.0]).astype(np.float32)  # turned about y and moved so that the plane is 1 m ahead
    behind[2, 3] = 2.0
    keys, m = V.render_depth_map(d, None, V.view_params(V.inverse(K), behind, K, (W, H), (W, H)))
    assert np.all(keys == V.EMPTY) and np.all(m["depth"] == MINF)
    # the same geometry mirrored back is drawn: it is the winding, not the depth range, that removes it
    mirror = np.diag([-1.0, 1.0, 1.0, 1.0]).astype(np.float32)
    keys, _ = V.render_depth_map(d, None, V.view_params(V.inverse(K), mirror, K, (W, H), (W, H)))
    assert np.all(keys == V.EMPTY)
    keys, _ = V.render_depth_map(d, None, V.view_params(V.inverse(K), np.eye(4), K, (W, H), (W, H)))
    assert np.all(keys != V.EMPTY)


def test_restatement_equal_z_goes_to_the_lower_primitive():
    W, H = 16, 16
    x = np.array([[2, 2], [2, 2], [12, 12]], np.int64) * 256  # one triangle twice, clockwise on screen
    y = np.array([[12, 12], [2, 2], [12, 12]], np.int64) * 256
    area = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
    z3 = [np.full(2, 0.5, np.float32)] * 3
    for order in ((7, 3), (3, 7)):
        keys = np.full(W * H, V.EMPTY, np.uint64)
        V.rasterize(x, y, area, z3, np.array(order, np.int64), W, H, keys)
        hit = keys[keys != V.EMPTY]
        assert len(hit) > 20 and np.all((hit & np.uint64(0xFFFFFFFF)) == 3)
    # a nearer fragment wins whatever its id
    z3 = [np.array([0.5, 0.25], np.float32)] * 3
    keys = np.full(W * H, V.EMPTY, np.uint64)
    V.rasterize(x, y, area, z3, np.array([3, 7], np.int64), W, H, keys)
    assert np.all((keys[keys != V.EMPTY] & np.uint64(0xFFFFFFFF)) == 7)


def test_restatement_top_left_rule_shares_an_edge():
    """two triangles of one quad cover every pixel centre on their shared diagonal exactly once"""
    W, H = 8, 8
    x = np.array([[0, 8], [0, 0], [8, 8]], np.int64) * 256  # (0,8) (0,0) (8,8) and (8,8) (0,0) (8,0)
    y = np.array([[8, 8], [0, 0], [8, 0]], np.int64) * 256
    area = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
    assert np.all(area > 0)
    j, i = np.mgrid[0:H, 0:W]
    px, py = (i * 256 + 128).ravel(), (j * 256 + 128).ravel()
    c0, _ = V.cover(x[:, :1], y[:, :1], px, py)
    c1, _ = V.cover(x[:, 1:], y[:, 1:], px, py)
    assert np.all(c0 ^ c1)


# ---------------------------------------------------------------------------------------------------------- GPU

def depth_maps(W=640, H=480):
    """plane, two planes with a discontinuity, a sphere, noise with -inf holes (all at the 525/640 camera)"""
    rng = np.random.default_rng(11)
    K = V.intrinsics(525 * W / 640, 525 * W / 640, (W - 1) / 2, (H - 1) / 2)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    plane = np.full((H, W), 1.5, np.float32)
    two = np.where(u < W * 0.55, 1.2 + 0.0005 * v, 2.0 + 0.0008 * u).astype(np.float32)
    rx, ry = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
    # ray (rx, ry, 1) against a sphere at (0.1, 0, 2), radius 0.7
    a, b, c = rx * rx + ry * ry + 1, -2 * (0.1 * rx + 2.0), 0.01 + 4.0 - 0.49
    disc = b * b - 4 * a * c
    sphere = np.where(disc >= 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), -np.inf).astype(np.float32)
    noise = (1.3 + 0.004 * rng.standard_normal((H, W))).astype(np.float32)
    noise[rng.random((H, W)) < 0.05] = MINF
    colour = rng.random((H, W, 4)).astype(np.float32)
    colour[rng.random((H, W)) < 0.01] = MINF
    return K, dict(plane=plane, two_planes=two, sphere=sphere, noise=noise), colour


def rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def views(K, W, H):
    """(name, modelview, intrinsicNew, screen size)"""
    moved = np.eye(4)
    moved[:3, :3] = rot(0.08, -0.15, 0.05)
    moved[:3, 3] = (0.12, -0.05, 0.2)
    close = np.eye(4)
    close[2, 3] = -0.9
    return [
        ("identity", np.eye(4), K, (W, H)),
        ("moved", moved, V.intrinsics(600, 580, 330, 250), (W, H)),
        ("screen_320x240", np.eye(4), V.intrinsics(K[0, 0] / 2, K[1, 1] / 2, (320 - 1) / 2, (240 - 1) / 2), (320, 240)),
        ("screen_800x600", moved, V.intrinsics(K[0, 0] * 1.25, K[1, 1] * 1.25, (800 - 1) / 2, (600 - 1) / 2), (800, 600)),
        ("magnified", close, V.intrinsics(6000, 6000, (W - 1) / 2, (H - 1) / 2), (W, H)),
    ]


class GpuView:
    """the launcher-level passes on device buffers, with the keys read back between raster and resolve"""

    def __init__(self, vh, lib, W, H, SW, SH):
        self.vh, self.lib = vh, lib
        self.keys = lib.DeviceBuffer(8 * SW * SH)
        lib.check(vh.vh_memset(self.keys.ptr, 0xFF, 8 * SW * SH, None), "memset")
        self.words = vh.vh_view_large_list_words(W, H)
        self.large = lib.DeviceBuffer(4 * self.words)
        lib.check(vh.vh_memset(self.large.ptr, 0, 4 * self.words, None), "memset")
        self.out = [lib.DeviceBuffer(4 * SW * SH)] + [lib.DeviceBuffer(16 * SW * SH) for _ in range(3)]
        self.SW, self.SH = SW, SH

    def run(self, d_depth, d_color, params):
        vh, lib, SW, SH = self.vh, self.lib, self.SW, self.SH
        lib.check(vh.vh_view_raster(d_depth, C.byref(params), self.keys.ptr, self.large.ptr, None), "vh_view_raster")
        keys = self.keys.download(np.uint64, SW * SH).reshape(SH, SW)
        n_large = int(self.large.download(np.uint32, 1)[0])
        lib.check(vh.vh_view_resolve(d_depth, d_color, C.byref(params), self.keys.ptr, self.large.ptr, *[b.ptr for b in self.out], None), "resolve")
        maps = dict(depth=self.out[0].download(np.float32, SW * SH).reshape(SH, SW))
        for name, b in zip(("positions", "normals", "colors"), self.out[1:]):
            maps[name] = b.download(np.float32, SW * SH * 4).reshape(SH, SW, 4)
        # the resolve leaves the buffers ready for the next view
        assert np.all(self.keys.download(np.uint64, SW * SH) == V.EMPTY) and self.large.download(np.uint32, 1)[0] == 0
        return keys, maps, n_large


def to_params(p):
    return T.make_view_params(p["intrinsicInverse"], p["modelview"], p["intrinsicNew"], (p["depthWidth"], p["depthHeight"]),
                              (p["screenWidth"], p["screenHeight"]), p["depthThreshOffset"], p["depthThreshLin"])


def assert_maps_equal(got, want, what):
    for k in ("depth", "positions", "normals", "colors"):
        assert same_bits(got[k], want[k]), f"{what}: map {k} differs at {np.argwhere(got[k].view(np.uint32) != want[k].view(np.uint32))[:5].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["plane", "two_planes", "sphere", "noise"])
def test_gpu_render_depth_map_bit_exact(vh, scene):
    from voxelhashing_amd import lib
    W, H = 640, 480
    K, maps, colour = depth_maps(W, H)
    depth = maps[scene]
    d_depth, d_colour = lib.DeviceBuffer.from_numpy(depth), lib.DeviceBuffer.from_numpy(colour)
    for name, mv, Knew, (SW, SH) in views(K, W, H):
        p = V.view_params(V.inverse(K), mv, Knew, (W, H), (SW, SH))
        want_keys, want = V.render_depth_map(depth, colour, p)
        keys, got, n_large = GpuView(vh, lib, W, H, SW, SH).run(d_depth.ptr, d_colour.ptr, to_params(p))
        assert np.array_equal(keys, want_keys), f"{scene}/{name}: {int((keys != want_keys).sum())} keys differ"
        assert_maps_equal(got, want, f"{scene}/{name}")
        covered = int((want_keys != V.EMPTY).sum())
        assert covered > (1000 if scene != "sphere" or name != "magnified" else 0), (scene, name, covered)
        if name == "magnified" and scene in ("plane", "two_planes"):
            assert n_large > 100, (scene, n_large)  # the second phase ran


def s1_raycast(W=320, H=240):
    """S1 integrated from a few orbit poses and ray-cast at the last one -> (camera params, ray caster, ray maps)"""
    from voxelhashing_amd import engine as E
    hp = T.make_hash_params(1 << 16, 1 << 14, **synth.PARAM_SETS["P4"])
    cp = T.make_depth_camera_params(W, H)
    scene, ray = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=True, gc=False)), E.CUDARayCastSDF(T.make_raycast_params(hp, cp))
    poses = [np.array(synth.orbit_pose(k, 90), dtype=np.float32) for k in range(3)]
    frames = [E.synth_frame(synth.S1_SPHERES, 0, p, cp) for p in poses]
    for p, f in zip(poses, frames):
        scene.integrate(p, f, cp, None)
    ray.render(scene.getHashData(), scene.getHashParams(), cp, poses[-1])
    return cp, scene, ray


@pytest.mark.gpu
def test_gpu_render_s1_raycast_bit_exact(vh):
    from voxelhashing_amd import engine as E, lib
    cp, scene, ray = s1_raycast()
    W, H = cp.m_imageWidth, cp.m_imageHeight
    rm = ray.download()
    assert (rm["depth"] != MINF).sum() > 5000
    rp = ray.getRayCastParams()
    Kinv = np.array(rp.m_intrinsicsInverse[:], np.float32).reshape(4, 4)
    K = np.array(rp.m_intrinsics[:], np.float32).reshape(4, 4)
    rd = ray.getRayCastData()
    renderer = E.RGBDRenderer()
    moved = np.eye(4)
    moved[:3, :3] = rot(0.0, 0.2, 0.0)
    moved[:3, 3] = (0.3, 0.0, 0.3)
    for name, mv, Knew, (SW, SH) in [("identity", np.eye(4), K, (W, H)), ("640x480", np.eye(4), V.intrinsics(K[0, 0] * 2, K[1, 1] * 2, 319.5, 239.5), (640, 480)),
                                     ("1920x1080", moved, V.intrinsics(K[0, 0] * 4, K[1, 1] * 4, 959.5, 539.5), (1920, 1080))]:
        p = V.view_params(Kinv, mv, Knew, (W, H), (SW, SH))
        want_keys, want = V.render_depth_map(rm["depth"], rm["colors"], p)
        keys, got, _ = GpuView(vh, lib, W, H, SW, SH).run(rd.d_depth, rd.d_colors, to_params(p))
        assert np.array_equal(keys, want_keys), f"S1/{name}: {int((keys != want_keys).sum())} keys differ"
        assert_maps_equal(got, want, f"S1/{name}")
        # the handle-level class runs the same passes
        renderer.RenderDepthMap(rd.d_depth, rd.d_colors, W, H, Kinv, mv, Knew, SW, SH, 0.012, 0.001)
        assert_maps_equal(renderer.download(), want, f"S1/{name} (RGBDRenderer)")


def assert_rgba8_close(got, want4, alpha_rule=True):
    want = V.rgba8(want4, alpha_rule)
    diff = got.astype(int) - want.astype(int)
    near = V.rgba8_boundary(want4)
    rgb_bad = (diff[..., :3] != 0) & ~((np.abs(diff[..., :3]) == 1) & near[..., :3])
    assert not rgb_bad.any(), np.argwhere(rgb_bad)[:5].tolist()
    a_ok = (diff[..., 3] == 0) | ((np.abs(diff[..., 3]) == 1) & near[..., 3]) | (diff[..., :3] != 0).any(-1)
    assert a_ok.all()


@pytest.mark.gpu
def test_gpu_phong_both_modes(vh):
    from voxelhashing_amd import engine as E, lib
    cp, scene, ray = s1_raycast(160, 120)
    rm, rd = ray.download(), ray.getRayCastData()
    light = default_light()
    W, H = cp.m_imageWidth, cp.m_imageHeight
    n = W * H
    out4, out8 = lib.DeviceBuffer(16 * n), lib.DeviceBuffer(4 * n)
    # the ray caster's own maps (render(float4*...)), with -inf where nothing was hit, and a hand-made invalid-pixel set
    pos, nrm, col = rm["depth4"].copy(), rm["normals"].copy(), rm["colors"].copy()
    pos[0, :8, 0], nrm[1, :8, 0], col[2, :8, 0] = MINF, MINF, MINF
    nrm[3, :8, 1] = MINF  # only x is tested
    bufs = [lib.DeviceBuffer.from_numpy(a) for a in (pos, nrm, col)]
    phong = E.PhongLighting(light)
    for use_material in (0, 1):
        for alpha_rule in (0, 1):
            lib.check(vh.vh_phong(*[b.ptr for b in bufs], n, use_material, C.byref(light), out4.ptr, out8.ptr, alpha_rule, None), "vh_phong")
            got4 = out4.download(np.float32, n * 4).reshape(H, W, 4)
            got8 = out8.download(np.uint8, n * 4).reshape(H, W, 4)
            want4 = V.phong(pos, nrm, col, use_material, light)
            invalid = (pos[..., 0] == MINF) | (nrm[..., 0] == MINF) | (col[..., 0] == MINF)
            assert invalid.sum() > 24 and (~invalid).sum() > 2000
            assert np.all(got4[invalid] == MINF) and np.all(got8[invalid] == 0)
            assert np.allclose(got4[~invalid], want4[~invalid], rtol=1e-5, atol=1e-7), np.abs(got4 - want4)[~invalid].max()
            assert_rgba8_close(got8, want4, bool(alpha_rule))
        # the handle-level class: float4 and its RGBA8 form with the alpha rule
        phong.render(*[b.ptr for b in bufs], bool(use_material), W, H, rgba8=True)
        assert same_bits(phong.download(), out4.download(np.float32, n * 4).reshape(H, W, 4))
        assert_rgba8_close(phong.download(rgba8=True), V.phong(pos, nrm, col, use_material, light), True)


REPLAY_PARAMS = """
s_sensorIdx = 8;
s_adapterWidth = 160;
s_adapterHeight = 120;
s_sensorDepthMax = 5.0f;
s_sensorDepthMin = 0.5f;
s_hashNumBuckets = 32768;
s_hashNumSDFBlocks = 16384;
s_hashMaxCollisionLinkedListSize = 7;
s_SDFVoxelSize = 0.01f;
s_SDFMarchingCubeThreshFactor = 10.0f;
s_SDFTruncation = 0.05f;
s_SDFTruncationScale = 0.025f;
s_SDFMaxIntegrationDistance = 4.0f;
s_SDFIntegrationWeightSample = 10;
s_SDFIntegrationWeightMax = 255;
s_SDFRayIncrementFactor = 0.8f;
s_SDFRayThresSampleDistFactor = 50.5f;
s_SDFRayThresDistFactor = 50.0f;
s_SDFUseGradients = false;
s_integrationEnabled = true;
s_trackingEnabled = true;
s_garbageCollectionEnabled = false;
s_marchingCubesMaxNumTriangles = 400000;
s_streamingEnabled = false;
s_offlineProcessing = true;
s_playData = true;
s_reconstructionEnabled = true;
s_binaryDumpSensorUseTrajectory = true;
""" + RENDER_BLOCK.decode()


@pytest.mark.gpu
def test_gpu_replay_render_to_file(vh, tmp_path):
    """a synthetic `.sens` of S1 through tools/replay.py --render-to, end to end: three frames, four image directories;
    then the same loop in process, whose last reconstruction image is the restatement applied to its ray cast"""
    import json
    from voxelhashing_amd import engine as E, reconstruction as R, sensor_data as SD
    cp = T.make_depth_camera_params(160, 120)
    poses = [np.array(synth.orbit_pose(k, 90), dtype=np.float32) for k in range(4)]
    sd = SD.SensorData.create((160, 120), (160, 120), SD.make_intrinsic_matrix(cp.fx, cp.fy, cp.mx, cp.my), depth_shift=1000.0,
                              sensor_name="synthetic S1", depth_type=SD.TYPE_ZLIB_USHORT)
    for k, p in enumerate(poses):
        d, c = E.synth_frame(synth.S1_SPHERES, 0, p, cp).download()
        d = np.where(np.isfinite(d), d, 0.0).astype(np.float64)
        rgb = np.clip(np.nan_to_num(c[..., :3], neginf=0.0) * 255.0 + 0.5, 0, 255).astype(np.uint8)
        sd.addFrame(np.ascontiguousarray(rgb), np.floor(1000.0 * d + 0.5).astype(np.uint16), p, k, k)
    sens, params = str(tmp_path / "s1.sens"), str(tmp_path / "params.txt")
    sd.saveToFile(sens)
    open(params, "w").write(REPLAY_PARAMS)
    out_dir = str(tmp_path / "render")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "replay.py"), "--params", params, "--sens", sens, "--render-to", out_dir, "--max-frames", "3"]
    out = json.loads(subprocess.check_output(cmd, timeout=600).decode().strip().splitlines()[-1])
    assert out["frames"] == 3 and out["render_to"] == out_dir, out
    names = ["%06d.png" % k for k in (1, 2, 3)]
    for sub in ("reconstruction", "reconstruction_color", "input_color", "input_depth"):
        assert sorted(os.listdir(os.path.join(out_dir, sub))) == names, sub
    last = V.read_png_rgba8(os.path.join(out_dir, "reconstruction", names[-1]))
    assert last.shape == (120, 160, 4) and (last[..., 3] == 255).sum() > 1000

    # in process, so that the last ray cast can be read back
    g = R.read_app_state(params)
    rs = R.read_render_state(params)
    rs.s_renderToFile, rs.s_renderToFileDir = 1, str(tmp_path / "again").encode()
    rec = R.Reconstruction(g, None, [sens], render_state=rs)
    assert rec.run(3) == 3
    rec.scene.synchronize()
    rm, rp = rec.ray.download(), rec.ray.getRayCastParams()
    p = V.view_params(np.array(rp.m_intrinsicsInverse[:], np.float32), np.eye(4), rec.render_color_intrinsics, (rp.m_width, rp.m_height), (160, 120),
                      rs.s_renderingDepthDiscontinuityThresOffset, rs.s_renderingDepthDiscontinuityThresLin)
    _, maps = V.render_depth_map(rm["depth"], rm["colors"], p)
    light = E.phong_light_from_render_state(rs)
    for sub, use_material in (("reconstruction", False), ("reconstruction_color", True)):
        got = V.read_png_rgba8(str(tmp_path / "again" / sub / names[-1]))
        assert_rgba8_close(got, V.phong(maps["positions"], maps["normals"], maps["colors"], use_material, light), True)
    reader = SD.SensorDataReader(sens)
    d3, c3 = [reader.processDepth() for _ in range(3)][-1]
    assert np.array_equal(V.read_png_rgba8(str(tmp_path / "again" / "input_color" / names[-1])), R.rgbx_alpha_rule(c3))
    assert np.array_equal(V.read_png_rgba8(str(tmp_path / "again" / "input_depth" / names[-1])), R.depth_image_rgba8(d3))
    # off unless asked for: the same files without --render-to write nothing
    out = json.loads(subprocess.check_output(cmd[:-4] + cmd[-2:], timeout=600).decode().strip().splitlines()[-1])
    assert out["frames"] == 3 and "render_to" not in out
