"""The interval ray caster's two block lookups and its two voxel addressings, bit for bit against each other and
against the hash-table ray caster (k_render_hash), which shares none of them:

  * a launch that holds tiles with complete lists (LDS-only lookup) beside tiles whose lists overflowed (general lookup,
    which falls back to the hash table), with the small and with the large tables, with and without gradients;
  * voxel byte offsets with the top bit set, where the 32-bit form must not sign-extend or wrap, against the 64-bit form;
  * views whose samples have negative block coordinates and taps at local index 7, and one in which a wave has lanes on
    both sides of a block face in the same sample."""
import ctypes as C

import numpy as np
import pytest

import tile_intervals as TI
from helpers import assert_maps_equal, small_config
from voxelhashing_amd import synth, vhtypes as T

pytestmark = pytest.mark.gpu
BLOCK_BYTES = 8 * 512  # sizeof(VhVoxel) * voxels per block


@pytest.fixture(scope="module")
def E(vh):
    from voxelhashing_amd import engine
    return engine


@pytest.fixture(scope="module")
def tables(E):
    """the scenes of tile_intervals.TABLES on the device, each built when first asked for and then only read:
    name -> dict(scene, hd, hp, blocks [n, 3])"""
    class Tables(dict):
        def __missing__(self, name):
            hp, cp, rp, opt, poses = TI.table_frames(name)
            scene = E.CUDASceneRepHashSDF(hp, opt)
            frame = E.DepthFrame(cp)
            for pose in poses:
                E.synth_frame(synth.S1_SPHERES, 0, pose, cp, out=frame)
                scene.integrate(pose, frame, cp, None)
            table = scene.download(False)["hash"]
            blocks = np.ascontiguousarray(table["pos"][table["ptr"] != T.FREE_ENTRY]).reshape(-1, 3).astype(np.int32)
            self[name] = dict(scene=scene, hd=scene.getHashData(), hp=scene.getHashParams(), blocks=blocks)
            return self[name]
    return Tables()


def clear_maps(vh, lib, rd, W, H):
    for ptr, words in ((rd.d_depth, 1), (rd.d_depth4, 4), (rd.d_colors, 4), (rd.d_normals, 4)):
        lib.check(vh.vh_memset(ptr, 0, 4 * words * W * H, None))


def render_hash(vh, lib, ray, hd, hp, cp, rp, W, H):
    rd = ray.getRayCastData()
    clear_maps(vh, lib, rd, W, H)
    lib.check(vh.vh_render(C.byref(hd), C.byref(hp), C.byref(rd), C.byref(cp), C.byref(rp), None))
    return ray.download()


def render_intervals(vh, lib, ray, hd, hp, cp, rp, W, H, cap):
    """splat + render with lists of `cap` entries -> (maps, heads [tiles, 4], lists [tiles, cap, 4])"""
    n = ((W + 7) // 8) * ((H + 7) // 8)
    d_heads, d_lists = lib.DeviceBuffer(n * 16), lib.DeviceBuffer(n * cap * 16)
    lib.check(vh.vh_ray_interval_clear(d_heads.ptr, W, H, None))
    lib.check(vh.vh_ray_interval_splat(C.byref(hd), C.byref(hp), C.byref(cp), C.byref(rp), d_heads.ptr, d_lists.ptr, cap, None, 0, None, None))
    heads, lists = d_heads.download(np.uint32).reshape(n, 4), d_lists.download(np.int32).reshape(n, cap, 4)
    rd = ray.getRayCastData()
    clear_maps(vh, lib, rd, W, H)
    lib.check(vh.vh_render_intervals(C.byref(hd), C.byref(hp), C.byref(rd), C.byref(cp), C.byref(rp), d_heads.ptr, d_lists.ptr, cap, None, 0, None))
    return ray.download(), heads, lists


@pytest.mark.parametrize("gradients", [False, True])
def test_complete_and_overflowed_tiles_in_one_launch(vh, E, tables, gradients):
    """fine_1cm (48x36, 1 cm voxels, longest list 466): the small-table launch marches tiles of both kinds"""
    from voxelhashing_amd import lib
    tab = tables["P1"]
    view = TI.View("fine_1cm", tab["hp"])
    rp = view.raycast_params(tab["hp"], gradients)
    ray = E.CUDARayCastSDF(rp)
    want = render_hash(vh, lib, ray, tab["hd"], tab["hp"], view.cp, rp, view.W, view.H)
    assert (want["depth"] != -np.inf).sum() > 50
    small, heads, _ = render_intervals(vh, lib, ray, tab["hd"], tab["hp"], view.cp, rp, view.W, view.H, TI.CAP_SMALL)
    count = heads[:, 2]
    n_complete, n_over = int(((count > 0) & (count <= TI.CAP_SMALL)).sum()), int((count > TI.CAP_SMALL).sum())
    print(f"\ngradients={gradients}: {n_complete} tiles with complete lists, {n_over} with overflowed ones, longest {count.max()}")
    assert n_complete > 0 and n_over > 0, "the launch was meant to hold complete and overflowed tile lists"
    # the general lookup must have found something (a lookup that found nothing would still agree on empty tiles); the
    # complete one is held to hits by test_block_borders_against_the_hash_table_ray_caster, whose lists are all complete
    hit = (want["depth"] != -np.inf)
    tile_hit = np.zeros(view.n_tiles, bool)
    ys, xs = np.nonzero(hit)
    tile_hit[(ys // 8) * view.tiles_x + xs // 8] = True
    assert (tile_hit & (count > TI.CAP_SMALL)).any(), "no tile with an overflowed list hits the surface"
    print(f"tiles that hit the surface: {int((tile_hit & (count > TI.CAP_SMALL)).sum())} overflowed, {int((tile_hit & (count <= TI.CAP_SMALL)).sum())} complete")
    assert_maps_equal(small, want, f"small tables against the hash-table ray caster, gradients={gradients}")
    large, heads, _ = render_intervals(vh, lib, ray, tab["hd"], tab["hp"], view.cp, rp, view.W, view.H, TI.CAP_LARGE)
    assert (heads[:, 2] > TI.CAP_LARGE).any() and ((heads[:, 2] > 0) & (heads[:, 2] <= TI.CAP_LARGE)).any()
    assert_maps_equal(large, want, f"large tables against the hash-table ray caster, gradients={gradients}")
    assert_maps_equal(small, large, "small tables against large tables")


@pytest.mark.parametrize("gradients", [False, True])
def test_voxel_offsets_with_the_top_bit_set(vh, E, gradients):
    """one 64x48 frame on a pool of 2^20 blocks whose heap hands out the upper half: every byte offset is >= 2^31"""
    from voxelhashing_amd import lib
    n_blocks = 1 << 20
    hp, cp, rp = small_config(64, 48, "P4", num_buckets=1 << 12, num_sdf_blocks=n_blocks)
    assert vh.vh_render_offsets32(n_blocks) == 1
    scene = E.CUDASceneRepHashSDF(hp, T.make_scene_options(offline=True, gc=False))
    hd = scene.getHashData()
    # The heap is {n-1, ..., 1, 0} with the counter on its last place: blocks come out lowest first.  Half of the pool is
    # taken as if allocated, so that what the frame gets is block 2^19 and above.
    assert lib.download(hd.d_heapCounter, np.uint32, 1)[0] == n_blocks - 1
    taken = np.array([n_blocks // 2 - 1], np.uint32)
    lib.check(vh.vh_memcpy_h2d(hd.d_heapCounter, taken.ctypes.data, 4, None))
    pose = synth.orbit_pose(0, 40)
    frame = E.DepthFrame(cp)
    E.synth_frame(synth.S1_SPHERES, 0, pose, cp, out=frame)
    scene.integrate(pose, frame, cp, None)
    hd, hpp = scene.getHashData(), scene.getHashParams()
    rp = T.make_raycast_params(hp, cp, use_gradients=gradients)
    rp.m_viewMatrix = T.mat16(TI.rigid_inverse(pose))
    rp.m_viewMatrixInverse = T.mat16(np.asarray(pose, np.float32).reshape(4, 4))
    ray = E.CUDARayCastSDF(rp)
    try:
        got32, heads, lists = render_intervals(vh, lib, ray, hd, hpp, cp, rp, 64, 48, TI.CAP_SMALL)
        count = np.minimum(heads[:, 2], TI.CAP_SMALL)
        listed = np.arange(TI.CAP_SMALL)[None, :] < count[:, None]
        offsets = lists[:, :, 3][listed].astype(np.int64) * 8  # a list entry's pointer is the block's first voxel
        assert len(offsets) > 0 and (offsets % BLOCK_BYTES == 0).all()
        print(f"\n{len(offsets)} listed blocks, byte offsets {offsets.min():#x} .. {offsets.max():#x}")
        assert (offsets >= 1 << 31).any(), "no listed block lies in the upper half of the pool"
        assert offsets.max() + BLOCK_BYTES <= 1 << 32
        assert (got32["depth"] != -np.inf).sum() > 200
        assert vh.vh_debug_render_force_offsets64(1) == 0
        assert vh.vh_render_offsets32(n_blocks) == 0
        got64, _, _ = render_intervals(vh, lib, ray, hd, hpp, cp, rp, 64, 48, TI.CAP_SMALL)
    finally:
        vh.vh_debug_render_force_offsets64(0)
    assert_maps_equal(got32, got64, f"32-bit offsets against 64-bit addresses, gradients={gradients}")
    assert_maps_equal(got32, render_hash(vh, lib, ray, hd, hpp, cp, rp, 64, 48), "against the hash-table ray caster")


def face_view(hp):
    """A camera 2 cm beside the block face x = 0 that looks along +z at S1's big sphere, unrotated: the image's columns
    run along world x, and the rays of the columns left and right of the one that looks along the face stay on their own
    side of it.  The tile that holds those columns -- the lanes of one wave -- has, in every march step, samples on both
    sides of the face, and samples that straddle it beside samples that do not."""
    return TI.View("face_4cm", hp, ("P4", 96, 72, TI.look_pose((0.02, 0.01, -1.9))))


@pytest.mark.parametrize("name", ["orbit_2cm", "close_8cm", "tilted_8cm", "face_4cm"])
def test_block_borders_against_the_hash_table_ray_caster(vh, E, tables, name):
    """negative block coordinates, taps at local index 7 and waves that sit on a block face: small tables, complete lists"""
    from voxelhashing_amd import lib
    view = face_view(tables["P4"]["hp"]) if name == "face_4cm" else TI.View(name, tables[TI.VIEWS[name][0]]["hp"])
    tab = tables[view.table]
    assert (tab["blocks"] < 0).any(), "the table was meant to hold blocks with negative coordinates"
    rp = view.raycast_params(tab["hp"], False)
    ray = E.CUDARayCastSDF(rp)
    want = render_hash(vh, lib, ray, tab["hd"], tab["hp"], view.cp, rp, view.W, view.H)
    assert (want["depth"] != -np.inf).sum() > 500
    if name == "face_4cm":
        # of the hit points of one tile (the 64 lanes of a wave), some lie in one block along x and some in the next
        vs = float(tab["hp"].m_virtualVoxelSize)
        hit = want["depth"] != -np.inf
        cam = np.where(hit[..., None], want["depth4"][..., :3], 0).astype(np.float64)
        world = cam @ view.pose.reshape(4, 4)[:3, :3].astype(np.float64).T + view.pose.reshape(4, 4)[:3, 3].astype(np.float64)
        xblock = np.floor(world[..., 0] / vs / 8.0)
        both = 0
        for ty in range(view.tiles_y):
            for tx in range(view.tiles_x):
                sl = (slice(8 * ty, 8 * ty + 8), slice(8 * tx, 8 * tx + 8))
                b = xblock[sl][hit[sl]]
                both += len(b) > 0 and b.min() != b.max()
        print(f"\n{both} tiles whose rays end in two blocks along x")
        assert both >= 4, "the view was meant to put the lanes of a wave on both sides of a block face"
    got, heads, _ = render_intervals(vh, lib, ray, tab["hd"], tab["hp"], view.cp, rp, view.W, view.H, TI.CAP_SMALL)
    if name != "orbit_2cm":
        assert (heads[:, 2] <= TI.CAP_SMALL).all(), "every list was meant to be complete"
    assert_maps_equal(got, want, f"{name}: small tables against the hash-table ray caster")
