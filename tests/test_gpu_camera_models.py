"""The camera-model kernels on the device under cameras other than the default one (tests/camera_models.py): fx != fy, a
principal point off the image centre and off the image, other depth limits, truncations and weight caps.  With
fx == fy and a centred principal point an fx where an fy belongs, a dropped cp.fy or a sign error in the principal
point's offset leaves every bit of the rest of the suite unchanged; here it does not.

Everything is compared as the kernel's own test compares it -- bit for bit against the oracle and the numpy
restatements, the ICP sums within the float32 bound of their summation -- and tests/test_camera_models.py holds the
oracle and the restatements to the reference under the same cameras.  No case passes empty: the lower bounds on blocks
and ray hits are literal numbers read off the oracle's own run on the CPU (two thirds of what it gave), never off the
device.  160x120 has an even width, so block footprints are staged; 101x77 an odd one, so every block takes the plain
path."""
import ctypes as C

import numpy as np
import pytest

import camera_models as CM
from helpers import assert_maps_equal, bits
from test_gpu_parity import general_poses
from voxelhashing_amd import canonical, synth, vhtypes as T

pytestmark = pytest.mark.gpu
f32 = np.float32
MINF = f32(-np.inf)


@pytest.fixture(scope="module")
def E(vh):
    from voxelhashing_amd import engine
    return engine


def frames_for(cp, n, seed, pset=None):
    back = CM.parameter_set(pset)["back"] if pset else 0.0
    return CM.place(general_poses(n, seed), cp, back)


# ------------------------------------------------------------------------------------------------ the frame loop

# (camera, size, voxels, parameter set) -> (buckets, seed of the poses, blocks after the last frame and ray hits of all
# frames by the oracle alone, times 2/3).  2 cm voxels put several new blocks of one frame into one of 2^14 buckets, and
# which of them an online pass serves is a matter of scheduling (tests/test_gpu_frame_loop.py): they get 2^16 buckets and
# poses under which the oracle's online pass allocates what its offline passes do (asserted in the test).
LOOP = {
    ("tum", (160, 120), "P4", None): (1 << 14, 1, 149, 14478), ("tum", (101, 77), "P4", None): (1 << 14, 1, 149, 5844),
    ("tall", (160, 120), "P4", None): (1 << 14, 1, 133, 15946), ("tall", (101, 77), "P4", None): (1 << 14, 1, 134, 6456),
    ("wide", (160, 120), "P4", None): (1 << 14, 1, 134, 18613), ("wide", (101, 77), "P4", None): (1 << 14, 1, 134, 7526),
    ("offcentre", (160, 120), "P4", None): (1 << 14, 1, 146, 16153), ("offcentre", (101, 77), "P4", None): (1 << 14, 1, 146, 6545),
    ("crop", (160, 120), "P4", None): (1 << 14, 1, 131, 19344), ("crop", (101, 77), "P4", None): (1 << 14, 1, 131, 7830),
    ("fisheyeish", (160, 120), "P4", None): (1 << 14, 1, 164, 7370), ("fisheyeish", (101, 77), "P4", None): (1 << 14, 1, 163, 2976),
    ("tum", (160, 120), "P2", None): (1 << 16, 2, 590, 14365), ("tum", (101, 77), "P2", None): (1 << 16, 2, 578, 5777),
    ("tall", (160, 120), "P2", None): (1 << 16, 2, 498, 15948), ("tall", (101, 77), "P2", None): (1 << 16, 2, 488, 6448),
    ("tum", (160, 120), "P4", "near"): (1 << 14, 1, 67, 8543), ("tum", (160, 120), "P4", "thin"): (1 << 14, 1, 91, 13112),
    ("tum", (160, 120), "P4", "thin_scaled"): (1 << 14, 1, 158, 14680), ("tum", (160, 120), "P4", "saturating"): (1 << 14, 1, 149, 14476),
}


def loop_inputs(O, key, cases=None, march=None):
    """-> hp, cp, rp, poses, the oracle's frames of a LOOP case (or of a case of another table of that layout, under a
    march set of tests/camera_models.py)"""
    name, size, voxels, pset = key
    buckets, seed = (LOOP if cases is None else cases)[key][:2]
    blocks = 1 << 12 if voxels == "P2" else 1 << 11
    hp, cp, rp = CM.config(name, size, voxels, pset, buckets=buckets, blocks=blocks, march=march)
    poses = frames_for(cp, 4, seed, pset)
    return hp, cp, rp, poses, [O.synth_frame(CM.SPHERES, 0, p, cp) for p in poses]


def oracle_loop(O, hp, cp, rp, poses, host):
    """the online frame loop on the oracle alone -> (scene, ray hits of all renders)"""
    ref = O.OracleScene(hp, cp, rp, T.make_scene_options(offline=False, gc=True, starve=2))
    hits = 0
    for k, p in enumerate(poses):
        if k > 0:
            hits += int((ref.render(poses[k - 1])["depth"] != -np.inf).sum())
        ref.integrate(p, *host[k])
    return ref, hits


@pytest.mark.parametrize("key", list(LOOP), ids=lambda k: "-".join(str(v) for v in (k[0], k[1][0], k[2], k[3]) if v is not None))
def test_native_loop_under_a_camera(E, oracle_lib, key):
    """vh_reconstruction_run frame by frame with its riders -- alloc in the ray caster's launch, compactify and the next
    frame's splat in computeNormals', the pass over the voxels with GC behind them -- against the oracle after every
    frame: the canonical scene and the four ray-cast maps"""
    native_loop_under_a_camera(E, oracle_lib, key)


def native_loop_under_a_camera(E, O, key, cases=None, march=None):
    """test_native_loop_under_a_camera's body, for a case of LOOP or of another table of its layout"""
    from test_gpu_frame_loop import oracle_online_is_deterministic
    hp, cp, rp, poses, host = loop_inputs(O, key, cases, march)
    n = len(poses)
    assert oracle_online_is_deterministic(O, hp, cp, rp, poses, host, True, 2), "pick poses without same-pass bucket sharing"
    frames = [E.synth_frame(CM.SPHERES, 0, p, cp) for p in poses]
    for k, f in enumerate(frames):  # k_synth under this camera
        gd, gc = f.download()
        assert np.array_equal(bits(gd), bits(host[k][0])) and np.array_equal(bits(gc), bits(host[k][1])), f"synthetic frame {k}"
    opt = T.make_scene_options(offline=False, gc=True, starve=2)
    scene, ray, ref = E.CUDASceneRepHashSDF(hp, opt), E.CUDARayCastSDF(rp), O.OracleScene(hp, cp, rp, opt)
    recon = E.Reconstruction(scene, ray, None, cp)
    seq = E.Reconstruction.makeFrames(poses, [f.depth_ptr for f in frames], [f.color_ptr for f in frames])
    hits = 0
    for k in range(n):
        recon.run(seq, k, 1)
        recon.synchronize()
        if k > 0:
            want = ref.render(poses[k - 1])
            assert_maps_equal(ray.download(), want, f"{key} frame {k}: ray cast of pose {k - 1}")
            hits += int((want["depth"] != -np.inf).sum())
        ref.integrate(poses[k], *host[k])
        canonical.assert_same_scene(scene.state(), ref.state(), f"{key} frame {k}")
    blocks = ref.state()["num_occupied"]
    print(f"{key} {march or ''}: {blocks} blocks, {hits} hits")
    want = (LOOP if cases is None else cases)[key]
    assert blocks >= want[2] and hits >= want[3], (blocks, hits)
    st = recon.getStats()
    assert st["frames"] == n and st["invalidFrames"] == 0
    assert st["framesWithRiders"] == n - 1 and st["splatsMadeAheadUsed"] == n - 2, st
    sw = scene.getState()
    assert sw[T.STATE_HEAP_UNDERFLOW] == 0 and sw[T.STATE_INSERT_FAILED] == 0 and sw[T.STATE_RIDER_GAVE_UP] == 0
    recon.close()
    ray.close()
    scene.close()


def test_parameter_sets_take_effect_in_the_oracle(oracle_lib):
    """the cuts of the parameter sets really are crossed by test_native_loop_under_a_camera's frames: by the oracle
    alone, the same frames with one limit at a time put back to its default (no device in this test)"""
    from test_camera_models import cuts_taking_effect
    O = oracle_lib
    size = (160, 120)
    cuts = {}
    for pset in CM.PARAMETER_SETS:
        key = ("tum", size, "P4", pset)
        hp, cp, rp, poses, host = loop_inputs(O, key)
        cuts[pset] = cuts_taking_effect(pset, size, poses, buckets=LOOP[key][0], blocks=1 << 11)
        print(pset, cuts[pset])
    # the oracle: 19 289 voxels more with the default integration distance, 424 ray hits more with the default depth range
    assert cuts["near"]["voxels_refused_by_max_integration_distance"] >= 12000 and cuts["near"]["pixels_refused_by_depth_max"] >= 280
    assert cuts["saturating"]["voxels_at_weight_max"] >= 1  # the oracle: 713
    assert cuts["thin"]["voxels_with_default_truncation"] - cuts["thin"]["voxels"] >= 15000  # the oracle: 49 394 - 25 841
    assert cuts["thin_scaled"]["voxels"] - cuts["thin_scaled"]["voxels_with_default_truncation"] >= 1800  # 52 206 - 49 394


# (camera, size, voxels, pool): the fused pass takes one workgroup per block while the blocks in view are at most a quarter
# of the pool, and one wave per block beyond -- where a staged block with a certificate goes through
# integrate_block_certified (tests/test_gpu_integrate_shapes.py)
SEQUENCES = [("tum", (160, 120), "P4", 2048), ("tall", (160, 120), "P4", 2048), ("offcentre", (101, 77), "P4", 2048),
             ("tum", (160, 120), "P2", 1024), ("tall", (160, 120), "P2", 1024), ("wide", (160, 120), "P2", 1024),
             ("offcentre", (160, 120), "P2", 1024), ("crop", (160, 120), "P2", 1024), ("tall", (101, 77), "P2", 1024)]


def sequence_inputs(name, size, voxels, pool):
    hp, cp, rp = CM.config(name, size, voxels, buckets=1 << 14, blocks=pool)
    return hp, cp, rp, frames_for(cp, 4, 1)


@pytest.mark.parametrize("reference_sequence", [False, True])
@pytest.mark.parametrize("name,size,voxels,pool", SEQUENCES, ids=[f"{c[0]}-{c[1][0]}-{c[2]}-{c[3]}" for c in SEQUENCES])
def test_launch_sequences_under_a_camera(E, oracle_lib, name, size, voxels, pool, reference_sequence):
    """the same kind of frames through CUDASceneRepHashSDF::integrate: the fused pass in a launch of its own, in both of
    its shapes, and the reference's launch sequence (plain kernels) -- so that a difference between the fused and the
    plain paths shows up apart from a difference to the oracle"""
    from test_gpu_parity import run_pair
    O = oracle_lib
    hp, cp, rp, poses = sequence_inputs(name, size, voxels, pool)
    opt = T.make_scene_options(offline=True, gc=True, starve=2, reference_launch_sequence=reference_sequence)
    g_scene, g_ray, o_scene = run_pair(E, O, hp, cp, rp, opt, poses, CM.SPHERES)
    in_view = o_scene.hp.m_numOccupiedBlocks  # the oracle's count for the last frame
    if voxels == "P4":
        assert 100 <= in_view <= pool // 4, in_view  # a workgroup per block (the oracle: 171 to 212 in view)
    else:
        assert in_view > pool // 4 + 64, in_view     # a wave per block (the oracle: 595 to 793 in view)
    st = g_scene.getState()
    assert st[T.STATE_HEAP_UNDERFLOW] == 0 and st[T.STATE_INSERT_FAILED] == 0


# ------------------------------------------------------------------------------------------------ block boxes

def box_expectations(O, hp, cp, blocks):
    """per block of a compactified list, from the oracle's projection of its eight corner voxels (the expressions of
    integrateDepthMap: float32, one rounding per operation, an IEEE division): the pixel hull, whether every corner
    passes the range certificate, and the box vh_frame_compactify.hpp describes -- the hull one pixel wider all round,
    clipped to the image, starting at an even pixel"""
    import ray_query as RQ
    L = O.lib()
    W, H = cp.m_imageWidth, cp.m_imageHeight
    vs = f32(hp.m_virtualVoxelSize)
    out = []
    for b in blocks:
        xs, ys, zs, fine = [], [], [], True
        for c in range(8):
            v = np.array([b[0] * 8 + (7 if c & 1 else 0), b[1] * 8 + (7 if c & 2 else 0), b[2] * 8 + (7 if c & 4 else 0)], np.int32)
            pf = RQ.mat_mul_p(hp.m_rigidTransformInverse, v.astype(f32) * vs)
            px = np.zeros(2, np.int32)
            L.vho_camera_to_screen_int(C.byref(cp), pf.ctypes.data_as(C.POINTER(C.c_float)), px.ctypes.data_as(C.POINTER(C.c_int32)))
            xs.append(int(px[0])); ys.append(int(px[1])); zs.append(float(pf[2]))
            fine = fine and 2.0 ** -20 <= pf[2] <= 2.0 ** 20 and abs(pf[0] * f32(cp.fx)) <= 2.0 ** 60 and abs(pf[1] * f32(cp.fy)) <= 2.0 ** 60
        x0, x1 = max(min(xs) - 1, 0) & ~1, min(max(xs) + 1, W - 1)
        y0, y1 = max(min(ys) - 1, 0), min(max(ys) + 1, H - 1)
        out.append(dict(hull=(min(xs), max(xs), min(ys), max(ys)), in_front=min(zs) > 1e-3, fine=bool(fine), cols=x1 - x0 + 1, rows=y1 - y0 + 1))
    return out


def box_scene(O, name, E=None):
    """four frames of S1 under `name` with a near limit of 5 cm; in the last one a patch in the middle of the image reads
    10 to 20 cm, as if something were held in front of the sensor, and the camera stands 10 cm in front of a block's
    centre: the blocks allocated there have corners behind the camera (no certificate) and footprints far beyond the tile
    (no staging), beside the scene's ordinary blocks
    -> the oracle scene, the device scene (with E), (hp, cp, rp), poses"""
    hp = T.make_hash_params(1 << 12, 1 << 11, **synth.PARAM_SETS["P4"])
    cp = CM.camera(name, 160, 120, depth_min=0.05)
    rp = T.make_raycast_params(hp, cp)
    opt = T.make_scene_options(offline=True, gc=True, starve=2)
    ref = O.OracleScene(hp, cp, rp, opt)
    scene = E.CUDASceneRepHashSDF(hp, opt) if E is not None else None
    poses = frames_for(cp, 4, 1)
    # the last camera is moved by less than a block, to 10 cm in front of the centre of the block ahead of it
    m = np.asarray(poses[3], np.float64).reshape(4, 4).copy()
    ahead = m[:3, 3] + m[:3, :3] @ np.array([0.0, 0.0, 0.1])
    centre = (np.floor(ahead / (8 * hp.m_virtualVoxelSize) + 0.5 / 8) * 8 + 3.5) * hp.m_virtualVoxelSize
    m[:3, 3] = centre - m[:3, :3] @ np.array([0.0, 0.0, 0.1])
    poses[3] = m.astype(np.float32).reshape(16)
    for k, p in enumerate(poses):
        d, c = O.synth_frame(CM.SPHERES, 0, p, cp)
        if k == 3:
            yy, xx = np.mgrid[50:70, 70:90]
            d[50:70, 70:90] = (0.10 + 0.005 * ((xx + yy) % 20)).astype(np.float32)
            c[50:70, 70:90] = (0.5, 0.25, 0.75, 1.0)
        ref.integrate(p, d, c)
        if scene is not None:
            scene.integrate(p, E.DepthFrame(cp, depth=d, color=c), cp, None)
            canonical.assert_same_scene(scene.state(), ref.state(), f"{name} frame {k}")
    return ref, scene, (hp, cp, rp), poses


# per camera, by the oracle's projection alone (box_expectations on the oracle's list): blocks that fit the tile, blocks
# refused for their rows alone, for their columns alone, blocks without a certificate -- each times 2/3 (None: not asked for)
BOX_KINDS = {"tall": (68, 28, None, 1), "wide": (78, None, 22, 1)}  # oracle: 103 / 43 / 0 / 1 of 185 in view, 118 / 3 / 33 / 1 of 203


def box_kinds(exp):
    fits = sum(e["in_front"] and e["cols"] <= 31 and e["rows"] <= 28 for e in exp)  # clear of the limits by a pixel
    rows_alone = sum(e["in_front"] and e["cols"] <= 31 and e["rows"] >= 31 for e in exp)
    cols_alone = sum(e["in_front"] and e["cols"] >= 34 and e["rows"] <= 28 for e in exp)
    return fits, rows_alone, cols_alone, sum(not e["fine"] for e in exp)


@pytest.mark.parametrize("name", ["tall", "wide"])
def test_block_boxes(E, oracle_lib, name):
    """the boxes in the spare words of the compactified list: the limit is 32 columns by 29 rows, so under `tall` blocks
    are refused for their rows alone and under `wide` for their columns alone.  Which blocks those are comes from the
    oracle's projection of the eight corners; the device's box must contain that hull and agree on the clear cases."""
    O = oracle_lib
    ref, scene, (hp, cp, rp), poses = box_scene(O, name, E)
    raw = scene.download(with_voxels=False)
    comp = raw["compactified"]
    assert np.array_equal(canonical.compactified_set(comp), canonical.compactified_set(ref.compactified()))
    exp = box_expectations(O, ref.hp, cp, comp["pos"])
    kinds = box_kinds(exp)
    print(f"{name}: {len(comp)} blocks in view; fit / rows alone / columns alone / no certificate: {kinds}")
    assert all(k >= w for k, w in zip(kinds, BOX_KINDS[name]) if w is not None), kinds
    if name == "tall":
        assert kinds[1] >= 1, "no block is refused for its rows alone"
    else:
        assert kinds[2] >= 1, "no block is refused for its columns alone"
    pad = comp["_pad"].view(np.uint32)
    x0, y0 = (pad[:, 0] & 0xFFFF).astype(int), (pad[:, 0] >> 16).astype(int)
    w, h, flags = (pad[:, 1] & 0xFF).astype(int), ((pad[:, 1] >> 8) & 0xFF).astype(int), pad[:, 1] >> 16
    staged, certified = (flags & 1) != 0, (flags & 2) != 0
    assert len(np.unique(pad[:, 2])) == 1 and pad[0, 2] != 0, "one tag, not zero, on every entry"
    assert staged.any() and (~staged).any() and certified.any() and (~certified).any(), "the frame was meant to hold all four kinds of block"
    W, H = cp.m_imageWidth, cp.m_imageHeight
    for i, e in enumerate(exp):
        what = f"{name}: block {comp['pos'][i]} hull {e['hull']} box {(x0[i], y0[i], w[i], h[i])} flags {flags[i]}"
        assert bool(certified[i]) == e["fine"], what
        clear_fit = e["in_front"] and e["cols"] <= 31 and e["rows"] <= 28
        clear_miss = not e["in_front"] or e["cols"] >= 34 or e["rows"] >= 31
        if clear_fit:
            assert staged[i], what
        if clear_miss and min(e["hull"][0], e["hull"][2]) > -(1 << 29):
            assert not staged[i], what
        if staged[i]:
            hx0, hx1, hy0, hy1 = e["hull"]
            assert x0[i] % 2 == 0 and 1 <= w[i] <= 32 and 1 <= h[i] <= 29 and x0[i] + w[i] <= W and y0[i] + h[i] <= H, what
            # the part of the hull that lies in the image
            assert x0[i] <= max(hx0, 0) and x0[i] + w[i] - 1 >= min(hx1, W - 1) and y0[i] <= max(hy0, 0) and y0[i] + h[i] - 1 >= min(hy1, H - 1), what
        else:
            assert w[i] == 0 and h[i] == 0, what


# ------------------------------------------------------------------------------------------------ ray cast paths

# camera -> ray hits of the two views by the oracle alone (2 cm voxels, then 1 cm), times 2/3
RAY_HITS = {"tum": (2746, 422), "offcentre": (2762, 514), "crop": (813, 190), "fisheyeish": (3312, 244)}  # oracle: 4 119 / 634, 4 143 / 772, 1 220 / 285, 4 969 / 366


def ray_cast_inputs(name, voxels):
    size = (160, 120) if voxels == "P2" else (64, 48)
    hp, cp, rp = CM.config(name, size, voxels, buckets=1 << 14, blocks=1 << 13 if voxels == "P2" else 1 << 14, gradients=True)
    poses = frames_for(cp, 3, 5)
    back = 0.0 if voxels == "P2" else 0.9   # 1 cm voxels from 3.4 m: tile lists beyond 64 and beyond 128 (tile_intervals' fine_1cm)
    view = CM.place(general_poses(1, 105), cp, back)[0]
    return hp, cp, rp, poses, view


@pytest.mark.parametrize("voxels", ["P2", "P1"])
@pytest.mark.parametrize("name", list(RAY_HITS))
def test_ray_cast_paths(E, oracle_lib, vh, name, voxels):
    """one scene, one novel view, with and without gradients, through every ray caster: the engine's own choice (interval
    splat, small tables), the large-tile tables (k_render_large), tile lists of four entries that overflow into the
    general lookup, and the hash-table ray caster -- each against the oracle's render, bit for bit"""
    from test_gpu_render_lookups import render_hash, render_intervals
    from voxelhashing_amd import lib
    import tile_intervals as TI
    O = oracle_lib
    hp, cp, rp, poses, view = ray_cast_inputs(name, voxels)
    opt = T.make_scene_options(offline=True, gc=False)
    scene, ref = E.CUDASceneRepHashSDF(hp, opt), O.OracleScene(hp, cp, rp, opt)
    for p in poses:
        scene.integrate(p, E.synth_frame(CM.SPHERES, 0, p, cp), cp, None)
        ref.integrate(p, *O.synth_frame(CM.SPHERES, 0, p, cp))
    canonical.assert_same_scene(scene.state(), ref.state(), f"{name} {voxels}: the scene to render")
    hd, hpp = scene.getHashData(), scene.getHashParams()
    W, H = cp.m_imageWidth, cp.m_imageHeight
    for gradients in (True, False):
        rpg = T.make_raycast_params(hp, cp, use_gradients=gradients)
        ref.rp.m_useGradients = 1 if gradients else 0
        want = ref.render(view)
        hits = int((want["depth"] != -np.inf).sum())
        print(f"{name} {voxels} gradients={gradients}: {hits} hits")
        assert hits >= max(RAY_HITS[name][voxels == "P1"], 1), hits
        what = f"{name} {voxels} gradients={gradients}"
        ray = E.CUDARayCastSDF(rpg)
        ray.render(hd, hpp, cp, view)
        assert_maps_equal(ray.download(), want, f"{what}: interval splat")
        rpv = ray.getRayCastParams()  # (with the view's matrices)
        got = render_hash(vh, lib, ray, hd, hpp, cp, rpv, W, H)
        for m in ("depth", "depth4", "colors") + (("normals",) if gradients else ()):  # (computeNormals is not part of the launchers)
            assert np.array_equal(bits(got[m]), bits(want[m])), f"{what}: hash-table ray caster, map {m}"
        longest = 0
        for cap in (TI.CAP_LARGE, TI.CAP_SMALL, 4):
            got, heads, _ = render_intervals(vh, lib, ray, hd, hpp, cp, rpv, W, H, cap)
            longest = max(longest, int(heads[:, 2].max()))
            for m in ("depth", "depth4", "colors") + (("normals",) if gradients else ()):
                assert np.array_equal(bits(got[m]), bits(want[m])), f"{what}: tile lists of {cap} entries, map {m}"
        assert longest > 4, "no tile list overflowed four entries"
        if voxels == "P1":
            assert longest > TI.CAP_SMALL, f"{what}: the longest tile list has {longest} entries: the large tables were not needed"
        ray.close()
    scene.close()


# ------------------------------------------------------------------------------------------------ ICP

@pytest.mark.parametrize("W,H", [(202, 154), (160, 120)])
@pytest.mark.parametrize("name", ["tum", "tall", "offcentre"])
def test_icp_steps_on_every_level(vh, oracle_lib, name, W, H):
    """the depth tracker's correspondences (bit for bit) and linear system (row counts exactly, sums within the float32
    bound) on levels 0, 1, 2 against oracle/icp.py: tests/test_camera_tracking.py's comparison, unchanged"""
    from test_camera_tracking import icp_steps_on_every_level
    cp = CM.camera(name, W, H)
    icp_steps_on_every_level(vh, oracle_lib, cp, CM.aim(cp))


@pytest.mark.parametrize("W,H", [(202, 154), (160, 120)])
@pytest.mark.parametrize("name", ["tum", "tall", "offcentre"])
def test_rgbd_build_step_on_every_level(vh, oracle_lib, name, W, H):
    """the RGB-D tracker's build step on levels 0, 1, 2 against tests/rgbd_icp.py: tests/test_rgbd_tracking.py's
    comparison, unchanged (the per-level fx / 2^level, fy / 2^level and the (dI PI) K row)"""
    from test_rgbd_tracking import rgbd_build_step_on_every_level
    rgbd_build_step_on_every_level(vh, CM.camera(name, W, H))


@pytest.mark.parametrize("W,H", [(202, 154), (160, 120)])
@pytest.mark.parametrize("name", ["tum", "tall", "offcentre"])
def test_fused_icp_steps_equal_the_separate_kernels(vh, oracle_lib, name, W, H):
    """vh_icp_step against correspondences + build + solve, and vh_icp_rgbd_step against build + solve: the whole state
    as bytes after every iteration of the default schedule, as tests/test_gpu_native_tracking.py and
    tests/test_gpu_native_rgbd_tracking.py compare them"""
    import rgbd_icp as G
    import test_gpu_native_rgbd_tracking as NR
    import test_gpu_native_tracking as NT
    from test_camera_tracking import GpuRig, TRACK_SPHERES
    from test_rgbd_tracking import PlaneRig, all_colour_settings
    from voxelhashing_amd import engine as E, lib
    O, L = oracle_lib, lib.load()
    hp, cp, rp = CM.config(name, (W, H), "P2", buckets=1 << 14, blocks=1 << 13)
    eye = np.eye(4, dtype=np.float32)
    # the depth tracker on S3
    poses = CM.place([synth.orbit_pose(k, n_frames=400) for k in range(2)], cp, offset=0.0)
    rig = GpuRig(E, hp, cp, rp)
    rig.feed(O, TRACK_SPHERES, poses[0])
    rig.integrate(poses[0])
    rig.feed(O, TRACK_SPHERES, poses[1])
    rig.ray.render(rig.scene.getHashData(), rig.scene.getHashParams(), cp, poses[0])
    rd = rig.ray.getRayCastData()
    a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
    lib.check(L.vh_rgbd_sensor_get_maps(rig.sensor.handle, C.byref(a), C.byref(b), C.byref(c)), "maps")
    lv = NT.Levels(L, lib, W, H, 3, a.value, b.value, rd.d_depth4, rd.d_normals)
    ts = T.make_tracking_state()
    want = lv.run(cp, ts, eye, False)
    NT.assert_same_states(lv.run(cp, ts, eye, True), want, f"{name} {W}x{H}: depth tracker")
    last = T.IcpState.from_buffer_copy(want[-1][2])
    assert len(want) == 18 and not last.lost and last.numCorr > 0.1 * W * H, (last.lost, last.numCorr)
    # the RGB-D tracker on the textured plane
    prig = PlaneRig(E, cp)
    at = G.plane_pose(0.01)
    for _ in range(6):  # (the model's colours: see tests/test_rgbd_tracking.py's apply_ct_equals_restatement)
        prig.feed(at)
        prig.integrate(at)
    prig.feed(G.plane_pose(0.035))
    prd = prig.render(at)
    pa, pb, pcol = prig.maps()
    plv = NR.LevelsRGBD(L, lib, W, H, 3, pa.value, pb.value, pcol, prd.d_depth4, prd.d_normals, prd.d_colors)
    pts = all_colour_settings()
    pwant = plv.run(cp, pts, eye, False)
    NR.assert_same_states(plv.run(cp, pts, eye, True), pwant, f"{name} {W}x{H}: RGB-D tracker")
    plast = T.IcpStateRGBD.from_buffer_copy(pwant[-1][2])
    assert not plast.icp.lost and plast.icp.numCorr > 0.1 * W * H, (plast.icp.lost, plast.icp.numCorr)


# ------------------------------------------------------------------------------------------------ queries

@pytest.mark.parametrize("name", ["offcentre", "crop"])
def test_queries_under_a_camera(E, oracle_lib, name):
    """vh_query_rays on the view's camera rays against tests/ray_query.py (on the device's own table) and against the
    device's render of that view, and vh_query_points around the hit points: tests/test_gpu_query.py's comparisons"""
    import crowded as CR
    import ray_query as RQ
    import test_gpu_query as TQ
    from test_camera_models import ray_query_model
    O = oracle_lib
    m = ray_query_model(name)  # the oracle's model and view of tests/test_camera_models.py: 1000 hits and 1000 misses there
    cp, view = m["cp"], m["view"]
    hp, _, rp = CM.config(name, (64, 48), gradients=True)
    scene = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=True))
    for pose in m["poses"]:
        scene.integrate(pose, E.synth_frame(synth.S1_SPHERES, 0, pose, cp), cp, None)
    canonical.assert_same_scene(scene.state(), m["o"].state(), f"{name}: the model")
    hd, hpp = scene.getHashData(), scene.getHashParams()
    host = CR.host_copy(O, scene.download(), hpp, cp, rp)
    rpv = RQ.view_params(O, rp, view)
    cam = RQ.camera_rays(host.L, cp, rpv)
    want = RQ.rays(host.L, host.hd, host.hp, rpv, cam["origins"], cam["directions"], cam["t_min"], cam["t_max"])
    hit = want["status"] == RQ.HIT
    assert hit.sum() >= 1000 and (want["status"] == RQ.MISS).sum() >= 1000, (hit.sum(), (~hit).sum())
    got = TQ.query_rays(hd, hpp, rpv, cam["origins"], cam["directions"], cam["t_min"], cam["t_max"])
    TQ.assert_rays(got, want, f"{name}: camera rays")
    maps = TQ.maps_of_rays(got, cam, rpv)
    for intervals in (False, True):
        ray = E.CUDARayCastSDF(rpv)
        ray.setIntervalSplatting(intervals)
        ray.render(hd, hpp, cp, view)
        TQ.assert_maps_match_rays(ray.download(), maps, rpv.m_width * rpv.m_height, f"{name}: intervals={intervals}")
        ray.close()
    hits = cam["origins"][hit].astype(np.float64) + cam["directions"][hit].astype(np.float64) * want["t"][hit, None].astype(np.float64)
    pts = np.concatenate(TQ.point_sets(hits, hpp.m_virtualVoxelSize, seed=11, uniform=1000))
    pref = RQ.points(host.L, host.hd, host.hp, pts)
    assert pref["valid"].sum() >= 1000 and (pref["valid"] == 0).sum() >= 500
    TQ.assert_points(TQ.query_points(hd, hpp, pts), pref, f"{name}: points")
    scene.close()


# ------------------------------------------------------------------------------------------------ sensor side, view

@pytest.mark.parametrize("w,h", [(160, 120), (101, 77)])
@pytest.mark.parametrize("name", ["tum", "tall"])
def test_depth_to_camera_space(E, oracle_lib, name, w, h):
    from helpers import make_depth
    O = oracle_lib
    cp = CM.camera(name, w, h)
    depth = make_depth(w, h, 4, holes=0.1)
    want = O.image_op("convert_depth_float_to_camera_space_float4", depth, w, h, cp, out_channels=4)
    got = E.image_op("convert_depth_float_to_camera_space_float4", depth, w, h, cp, out_channels=4)
    assert np.array_equal(bits(got), bits(want))
    assert (want[..., 2] != MINF).sum() > 0.8 * w * h


@pytest.mark.parametrize("name", ["tum", "tall"])
def test_sensor_remap_between_unlike_cameras(vh, oracle_lib, name):
    """the depth-to-colour remap with a depth camera `name` at 160x120 and a colour camera of another size and another
    fx / fy ratio: tests/test_depth_remapping.py's comparison of test_gpu_sensor_remap (the remapped depth against
    tests/view_render.py bit for bit, camera space and normals from it)"""
    import view_render as V
    from test_depth_remapping import as_dict, remap_params, rig_extrinsic, same_bits, sensor_inputs
    from voxelhashing_amd import engine as E
    O = oracle_lib
    sizes = dw, dh, cw, ch, W, H = 160, 120, 202, 154, 160, 120
    k = CM.intrinsics(name, dw, dh)
    dk = (k["fx"], k["fy"], k["mx"], k["my"])
    other = CM.intrinsics("wide" if name == "tall" else "offcentre", cw, ch)
    ck = (other["fx"], other["fy"], other["mx"], other["my"])
    assert abs(dk[0] / dk[1] - ck[0] / ck[1]) > 0.05
    ext = rig_extrinsic()
    on = E.CUDARGBDSensor((dw, dh), (cw, ch), (W, H), *dk, 0.5, 5.0)
    on.setCameraCalibration(True, *ck, ext, 0.012, 0.01)
    assert on.getCameraCalibration()[0]
    params = on.getCameraCalibration()[1]
    assert same_bits(params.intrinsicInverse[:], np.array(remap_params(sizes, dk, ck, ext).intrinsicInverse[:], np.float32))
    cp = on.getDepthCameraParams()
    assert cp.fx != cp.fy and abs(cp.fx - dk[0]) < 1e-3 and abs(cp.fy - dk[1]) < 1e-3  # the depth intrinsics, as in the reference
    for frame in range(2):
        depth, colour = sensor_inputs(dw, dh, 10 + frame, cw, ch)
        on.process(depth, colour)
        got = on.download()
        resampled = O.image_op("resample_float_map", depth, dw, dh, out_size=(W, H), prefill=np.full((H, W), MINF, np.float32))
        want = V.render_depth_map(resampled, None, as_dict(params))[1]["depth"]
        assert same_bits(got["depth"], want), f"frame {frame}: {int((got['depth'].view(np.uint32) != want.view(np.uint32)).sum())} pixels differ"
        assert (want != MINF).mean() > 0.5
        cam = O.image_op("convert_depth_float_to_camera_space_float4", want, W, H, cp, out_channels=4)
        assert same_bits(got["camera_space"], cam)
        assert same_bits(got["normals"], O.compute_normals(cam))


def test_view_render_under_tall(vh):
    """RenderDepthMap (raster keys and the four maps) against tests/view_render.py bit for bit: a sphere seen by `tall`,
    re-rendered from a moved view by a camera with yet another fx / fy ratio"""
    import view_render as V
    from test_view_rendering import GpuView, assert_maps_equal as assert_view_maps_equal, rot, to_params
    from voxelhashing_amd import lib
    W, H = 160, 120
    k = CM.intrinsics("tall", W, H)
    K = V.intrinsics(k["fx"], k["fy"], k["mx"], k["my"])
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    rx, ry = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
    a, b, c = rx * rx + ry * ry + 1, -2 * (0.1 * rx + 2.0), 0.01 + 4.0 - 0.49  # the ray (rx, ry, 1) against a sphere at (0.1, 0, 2), r = 0.7
    disc = b * b - 4 * a * c
    depth = np.where(disc >= 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), 2.6).astype(np.float32)  # in front of a wall
    rng = np.random.default_rng(11)
    colour = rng.random((H, W, 4)).astype(np.float32)
    colour[rng.random((H, W)) < 0.01] = MINF
    d_depth, d_colour = lib.DeviceBuffer.from_numpy(depth), lib.DeviceBuffer.from_numpy(colour)
    moved = np.eye(4)
    moved[:3, :3] = rot(0.08, -0.15, 0.05)
    moved[:3, 3] = (0.12, -0.05, 0.2)
    o = CM.intrinsics("offcentre", 202, 154)
    for what, mv, Knew, (SW, SH) in (("identity", np.eye(4), K, (W, H)),
                                     ("moved", moved, V.intrinsics(o["fx"], o["fy"], o["mx"], o["my"]), (202, 154))):
        p = V.view_params(V.inverse(K), mv, Knew, (W, H), (SW, SH))
        want_keys, want = V.render_depth_map(depth, colour, p)
        keys, got, _ = GpuView(vh, lib, W, H, SW, SH).run(d_depth.ptr, d_colour.ptr, to_params(p))
        assert np.array_equal(keys, want_keys), f"tall/{what}: {int((keys != want_keys).sum())} keys differ"
        assert_view_maps_equal(got, want, f"tall/{what}")
        assert int((want_keys != V.EMPTY).sum()) > 0.2 * SW * SH  # the restatement covers 83 % and 31 % of the screen
