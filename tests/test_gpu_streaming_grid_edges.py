"""World-chunk streaming at the edges of the chunk grid, on the GPU (tests/grid_edges.py has the scene, the grid and the
restatement; tests/test_streaming_grid_edges.py the same checks on the oracle alone).

The grid is smaller than the scene, so blocks lie in chunks that do not exist.  For alloc such a block is not streamed
out, whatever the bit mask holds at the index its chunk would linearise to (the reference reads that word: DESIGN.md
section 2); when it streams out it is dropped, as in the reference.  Held here to the oracle pair (oracle/vh_oracle.c +
oracle/chunk_grid.py) and to the restatement: vh_alloc and the alloc rider under crafted masks, the frame-by-frame
streaming calls, the pipelined streaming step of the native loop, and both copies of the bit mask word for word."""
import ctypes as C

import numpy as np
import pytest

import grid_edges as G
from grid_edges import MASK_CASES, case_mask, expected_blocks, oracle_blocks
from helpers import assert_maps_equal, small_config
from voxelhashing_amd import canonical, synth, vhtypes as T

pytestmark = pytest.mark.gpu

STREAM_POS = np.array([0.0, 0.0, 1.6, 1.0], dtype=np.float32)
RADIUS = 1.2  # small enough for blocks to leave: on the oracle pair 166 drops over the 24 frames, 180 blocks back at the end
WORDS = (G.N_BITS + 31) // 32


@pytest.fixture(scope="module")
def E(vh):
    from voxelhashing_amd import engine
    return engine


@pytest.fixture(scope="module")
def scene(oracle_lib):
    o, hp = oracle_blocks(oracle_lib)
    positions = o.state()["positions"].copy()
    return positions, G.check_conditions(positions, hp.m_virtualVoxelSize), hp


def sorted_blocks(descs, blocks):
    order = canonical.lexsort_pos(np.ascontiguousarray(descs["pos"]))
    return np.ascontiguousarray(descs["pos"][order]), np.ascontiguousarray(blocks[order])


def device_mask(case):
    """the case's mask in the middle of a device buffer whose other words are all ones -> (buffer, pointer to the mask,
    the same on the host for the oracle)"""
    from voxelhashing_amd.lib import DeviceBuffer
    whole, view = case_mask(case)
    buf = DeviceBuffer.from_numpy(whole)
    return buf, C.c_void_p(buf.ptr + 4 * G.GUARD_WORDS), whole, view


def missing_message(case, got, want, info, positions):
    outside = G.pos_set(positions[~info["inside"]])
    return (f"mask '{case}': {len(want - got)} of {len(want)} blocks missing ({len((want - got) & outside)} of them in chunks "
            f"outside the grid), {len(got - want)} unexpected")


@pytest.mark.parametrize("case", MASK_CASES)
def test_alloc_launcher_under_a_crafted_mask(E, oracle_lib, scene, case):
    """vh_alloc, one call per pass until the heap stops changing, for the scene's three poses.  An unguarded kernel stays
    inside this test's own buffer and fails by leaving out blocks whose chunk is outside the grid."""
    O = oracle_lib
    positions, info, _ = scene
    hp, cp, rp = small_config(G.WIDTH, G.HEIGHT, G.PARAMS, streaming_extents=G.EXT, streaming_dims=G.DIMS, streaming_min=G.MINP)
    want = expected_blocks(case, positions, info)
    buf, mask_ptr, whole, view = device_mask(case)
    o, _ = oracle_blocks(O, view)
    g = E.LauncherScene(hp)
    frame = E.DepthFrame(cp)
    for k in G.ALLOC_POSES:
        pose = G.orbit_pose(k)
        E.synth_frame(synth.S1_SPHERES, 0, pose, cp, out=frame)
        g.set_transform(pose, O.mat4_inverse(pose))
        prev = -1
        for _ in range(16):
            g.reset_mutex()
            g.alloc(frame, cp, mask_ptr, T.LOCK_ENTRY)
            cur = g.download(with_voxels=False)["heap_counter"]
            if cur == prev:
                break
            prev = cur
        else:
            raise AssertionError("alloc did not reach a fixed point in 16 passes")
    gs = g.state(with_voxels=False)
    got = G.pos_set(gs["positions"])
    print(f"vh_alloc, mask '{case}': {len(got)} blocks, {len(got & G.pos_set(positions[~info['inside']]))} outside the grid")
    assert got == want, "vh_alloc, " + missing_message(case, got, want, info, positions)
    assert got == G.pos_set(o.state()["positions"]) and gs["heap_free"] == o.state()["heap_free"]
    assert np.array_equal(buf.download(np.uint32), whole), "alloc only reads the mask"


@pytest.mark.parametrize("case", MASK_CASES)
def test_alloc_rider_under_a_crafted_mask(E, oracle_lib, scene, case):
    """The same masks through the alloc rider inside the ray caster's launch (integrateAhead -> render(coLaunch) ->
    integrateFinish, online alloc: one pass per frame, so every pose is given four frames).  The first frame has no ray
    cast to ride in and allocates through its own launch, as in the native loop.  Same table as vh_alloc's."""
    O = oracle_lib
    positions, info, _ = scene
    hp, cp, rp = small_config(G.WIDTH, G.HEIGHT, G.PARAMS, streaming_extents=G.EXT, streaming_dims=G.DIMS, streaming_min=G.MINP)
    opt = T.make_scene_options(offline=False, gc=False)
    want = expected_blocks(case, positions, info)
    buf, mask_ptr, whole, view = device_mask(case)
    order = [k for k in G.ALLOC_POSES for _ in range(4)]
    poses = {k: G.orbit_pose(k) for k in G.ALLOC_POSES}
    ref = O.OracleScene(hp, cp, rp, opt)
    for k in order:
        ref.integrate(poses[k], *O.synth_frame(synth.S1_SPHERES, 0, poses[k], cp), view)
    assert G.pos_set(ref.state()["positions"]) == want, "four online passes per pose must reach alloc's fixed point"
    gs, ray = E.CUDASceneRepHashSDF(hp, opt), E.CUDARayCastSDF(rp)
    frames = {k: E.synth_frame(synth.S1_SPHERES, 0, poses[k], cp) for k in G.ALLOC_POSES}
    rode = 0
    for i, k in enumerate(order):
        if i == 0:
            gs.integrate(poses[k], frames[k], cp, mask_ptr)
            continue
        job = gs.integrateAhead(poses[k], frames[k], cp, mask_ptr)
        assert job is not None
        ray.render(gs.getHashData(), gs.getHashParams(), cp, poses[order[i - 1]], coLaunch=job)
        rode += int(job.contents.allocLaunched == 1)
        gs.integrateFinish(frames[k], cp)
    assert rode == len(order) - 1, "every frame but the first allocates inside the ray caster's launch"
    st = gs.state(with_voxels=False)
    got = G.pos_set(st["positions"])
    assert got == want, "alloc rider, " + missing_message(case, got, want, info, positions)
    assert st["heap_free"] == ref.state()["heap_free"]
    sw = gs.getState()
    assert not sw[[T.STATE_HEAP_UNDERFLOW, T.STATE_INSERT_FAILED, T.STATE_RIDER_GAVE_UP]].any(), sw
    assert np.array_equal(buf.download(np.uint32), whole)
    ray.close()
    gs.close()


def make_pair(E, O, parts, gc=True):
    from oracle.chunk_grid import OracleChunkGrid
    hp, cp, rp = small_config(G.WIDTH, G.HEIGHT, G.PARAMS, streaming_extents=G.EXT, streaming_dims=G.DIMS, streaming_min=G.MINP)
    opt = T.make_scene_options(offline=True, gc=gc, starve=15, streaming_out_parts=parts)
    gs = E.CUDASceneRepHashSDF(hp, opt)
    gg = E.CUDASceneRepChunkGrid(gs, G.EXT, G.DIMS, G.MINP, 16, False, parts)
    os_ = O.OracleScene(hp, cp, rp, opt)
    og = OracleChunkGrid(os_, G.EXT, G.DIMS, G.MINP, parts)
    return hp, cp, rp, gs, gg, os_, og


def compare(gs, gg, os_, og, what):
    canonical.assert_same_scene(gs.state(), os_.state(), what)
    gd, gb = sorted_blocks(*gg.downloadHostBlocks())
    od, ob = sorted_blocks(*og.host_blocks())
    assert np.array_equal(gd, od), f"{what}: host chunk grid holds different blocks"
    assert gb.tobytes() == ob.tobytes(), f"{what}: host voxel payloads differ"
    st = gg.getStatistics()
    assert st["blocks"] == len(od) and st["bits"] == og.statistics()["bits"]
    gg.debugCheckForDuplicates()


def assert_masks(gg, og, what, uploaded=True):
    """both copies of the bit mask against the oracle's, word for word.  uploaded: getBitMaskGPU() has been called since
    the host's copy last changed, so the device's copy must hold it too and nothing is left to upload."""
    host, dev, dirty = gg.downloadBitMasks()
    assert len(host) == len(dev) == WORDS == len(og.bitmask)
    assert np.array_equal(host, og.bitmask), f"{what}: host copy {host} != oracle {og.bitmask}"
    if uploaded:
        assert not dirty, f"{what}: the host's copy is still marked dirty"
        assert np.array_equal(dev, og.bitmask), f"{what}: device copy {dev} != oracle {og.bitmask}"
    assert not (host[-1] >> (G.N_BITS % 32)) and not (dev[-1] >> (G.N_BITS % 32)), f"{what}: a bit past the grid's last chunk is set"
    return host, dev, dirty


def test_frame_by_frame_streaming_on_a_grid_smaller_than_the_scene(E, oracle_lib, scene):
    """streamOutToCPU / streamInToGPU / integrate(getBitMaskGPU()) per frame, offline alloc, against the oracle pair:
    blocks whose chunk is outside the grid are dropped when they leave -- counted by the pass, then in neither the
    table nor the host grid, their heap slots free -- and alloc brings them back whatever the mask holds elsewhere."""
    O = oracle_lib
    hp, cp, rp, gs, gg, os_, og = make_pair(E, O, 4)
    vs = hp.m_virtualVoxelSize
    frame = E.DepthFrame(cp)
    dropped = moved_out = moved_in = 0
    for k in range(24):
        pose = synth.orbit_pose(k, G.ORBIT)
        p = (pose.reshape(4, 4) @ STREAM_POS)[:3]
        E.synth_frame(synth.S1_SPHERES, 0, pose, cp, out=frame)
        depth, color = O.synth_frame(synth.S1_SPHERES, 0, pose, cp)
        before = G.pos_set(gs.state(with_voxels=False)["positions"])
        n_out = gg.streamOutToCPU(p, RADIUS, True)
        assert n_out == og.stream_out_to_cpu(p, RADIUS, True), f"frame {k}: blocks streamed out"
        st = gs.state(with_voxels=False)
        left = before - G.pos_set(st["positions"])
        assert len(left) == n_out, f"frame {k}: the pass counts every block that left, dropped ones included"
        if left:
            arr = np.array(sorted(left))
            gone = G.pos_set(arr[~G.classify(arr, vs)["inside"]])
            on_host = G.pos_set(gg.downloadHostBlocks()[0]["pos"])
            assert not (gone & on_host) and left - gone <= on_host, f"frame {k}: dropped blocks on the host, or kept ones missing"
            dropped += len(gone)
        assert st["heap_free"] == hp.m_numSDFBlocks - st["num_occupied"], f"frame {k}: a heap slot was lost"
        n_in = gg.streamInToGPU(p, RADIUS, True)
        assert n_in == og.stream_in_to_gpu(p, RADIUS, True), f"frame {k}: blocks streamed in"
        moved_out += n_out
        moved_in += n_in
        mask = gg.getBitMaskGPU()
        assert_masks(gg, og, f"frame {k}")
        gs.integrate(pose, frame, cp, mask)
        os_.integrate(pose, depth, color, og.bitmask)
        compare(gs, gg, os_, og, f"frame {k}")
    sw = gs.getState()
    assert not sw[[T.STATE_HEAP_UNDERFLOW, T.STATE_INSERT_FAILED]].any(), sw  # (the other words count, they do not report)
    # everything out, everything the grid holds back in
    held = gs.state()
    inside = G.classify(held["positions"], vs)["inside"]
    host_pos, host_vox = sorted_blocks(*gg.downloadHostBlocks())
    gg.streamOutToCPUAll()
    og.stream_out_to_cpu_all()
    assert gs.state(with_voxels=False)["num_occupied"] == 0
    gg.getBitMaskGPU()
    assert_masks(gg, og, "everything streamed out")
    centre, big = np.zeros(3, np.float32), 1000.0
    back = gg.streamInToGPUAll(centre, big, True)
    assert back == og.stream_in_to_gpu_all(centre, big, True)
    gg.getBitMaskGPU()
    host, dev, _ = assert_masks(gg, og, "everything streamed back in")
    assert not host.any() and not dev.any()
    after = gs.state()
    canonical.assert_same_scene(after, os_.state(), "out and back in")
    want_pos = np.concatenate([held["positions"][inside], host_pos])
    want_vox = np.concatenate([held["voxels"][inside], host_vox])
    order = canonical.lexsort_pos(want_pos)
    assert np.array_equal(after["positions"], want_pos[order]), "exactly the blocks inside the grid come back"
    assert after["voxels"].tobytes() == want_vox[order].tobytes(), "and bit for bit"
    assert after["heap_free"] == hp.m_numSDFBlocks - back == os_.state()["heap_free"]
    assert gg.getStatistics()["blocks"] == 0
    print(f"frame by frame: {moved_out} blocks out ({dropped} dropped), {moved_in} in, {int((~inside).sum())} of {len(inside)} "
          f"blocks outside the grid at the end, {back} back after streaming everything out and in")
    assert dropped >= 10 and back >= 20, (dropped, back)
    gg.close()
    gs.close()


def test_pipelined_streaming_on_a_grid_smaller_than_the_scene(E, oracle_lib):
    """The native loop with the worker thread, s_allocAhead = 1 and the streaming step decided a frame ahead (the device
    keeps its own copy of the bit mask: k_stream_out_pass1_bits sets no bit for a chunk outside the grid), the scene and
    grid moved away from the origin, online alloc.  After every call of three frames: scene, host grid, ray-cast maps and
    both copies of the mask equal the oracle pair's."""
    from oracle.chunk_grid import OracleChunkGrid
    O = oracle_lib
    parts, n, batch = 8, 12, 3
    hp, cp, rp = small_config(160, 120, G.PARAMS, num_buckets=1 << 15, num_sdf_blocks=1 << 13, streaming_extents=G.EXT,
                              streaming_dims=G.DIMS, streaming_min=G.SHIFTED_MINP)
    vs = hp.m_virtualVoxelSize
    poses = [G.orbit_pose(k, shifted=True) for k in range(n)]
    host = [O.synth_frame(G.SHIFTED_S1, 0, p, cp) for p in poses]
    # the oracle pair first (and its shadow with offline alloc: an online pass must not depend on scheduling), in the
    # reference's order of calls: the conditions on the inputs are known before anything is launched
    opt = T.make_scene_options(offline=False, gc=True, starve=4, streaming_out_parts=parts)
    ref = O.OracleScene(hp, cp, rp, opt)
    og = OracleChunkGrid(ref, G.EXT, G.DIMS, G.SHIFTED_MINP, parts)
    shadow = O.OracleScene(hp, cp, rp, T.make_scene_options(offline=True, gc=True, starve=4, streaming_out_parts=parts))
    sg = OracleChunkGrid(shadow, G.EXT, G.DIMS, G.SHIFTED_MINP, parts)
    want = []
    out = inn = dropped = 0
    deterministic = True
    for k in range(n):
        maps = ref.render(poses[k - 1]) if k > 0 else None
        p = (poses[k].reshape(4, 4) @ STREAM_POS)[:3]
        before = G.pos_set(ref.state()["positions"])
        out += og.stream_out_to_cpu(p, RADIUS, True)
        left = before - G.pos_set(ref.state()["positions"])
        if left:
            arr = np.array(sorted(left))
            dropped += int((~G.classify(arr, vs, minp=G.SHIFTED_MINP)["inside"]).sum())
        inn += og.stream_in_to_gpu(p, RADIUS, True)
        ref.integrate(poses[k], host[k][0], host[k][1], og.bitmask)
        sg.stream_out_to_cpu(p, RADIUS, True)
        sg.stream_in_to_gpu(p, RADIUS, True)
        shadow.integrate(poses[k], host[k][0], host[k][1], sg.bitmask)
        deterministic = deterministic and np.array_equal(canonical.block_positions(ref.hash_table()), canonical.block_positions(shadow.hash_table()))
        if (k + 1) % batch == 0:
            want.append(dict(maps=maps, scene=ref.state(), grid=sorted_blocks(*og.host_blocks()), mask=og.bitmask.copy(), totals=(out, inn)))
    assert deterministic, "pick poses without same-pass bucket sharing"
    info = G.classify(ref.state()["positions"], vs, minp=G.SHIFTED_MINP)
    print(f"pipelined: {out} blocks out ({dropped} dropped), {inn} in, {int((~info['inside']).sum())} of {len(info['inside'])} blocks "
          "outside the grid at the end")
    assert dropped > 0 and out > dropped and inn > 0, (out, dropped, inn)

    frames = [E.synth_frame(G.SHIFTED_S1, 0, p, cp) for p in poses]
    scene, ray = E.CUDASceneRepHashSDF(hp, opt), E.CUDARayCastSDF(rp)
    grid = E.CUDASceneRepChunkGrid(scene, G.EXT, G.DIMS, G.SHIFTED_MINP, 2000, True, parts)  # worker thread running
    recon = E.Reconstruction(scene, ray, grid, cp, E.Reconstruction.defaultOptions(
        s_streamingEnabled=1, s_streamingPos=STREAM_POS[:3], s_streamingRadius=RADIUS, s_allocAhead=1, s_maxFramesInFlight=16))
    seq = E.Reconstruction.makeFrames(poses, [f.depth_ptr for f in frames], [f.color_ptr for f in frames])
    for b, w in enumerate(want):
        k = (b + 1) * batch - 1
        recon.run(seq, b * batch, batch, lookahead=True)
        recon.synchronize()
        # both copies as the loop left them: the pipelined frames keep the device's copy themselves, nothing was uploaded
        hostm, devm, _ = grid.downloadBitMasks()
        assert np.array_equal(hostm, w["mask"]), f"frame {k}: host copy of the mask {hostm} != oracle {w['mask']}"
        assert np.array_equal(devm, w["mask"]), f"frame {k}: device copy of the mask {devm} != oracle {w['mask']}"
        assert_maps_equal(ray.download(), w["maps"], f"frame {k}: ray cast of pose {k - 1}")
        canonical.assert_same_scene(scene.state(), w["scene"], f"frame {k}")
        gd, gb = sorted_blocks(*grid.downloadHostBlocks())
        assert np.array_equal(gd, w["grid"][0]), f"frame {k}: host chunk grid holds different blocks"
        assert gb.tobytes() == w["grid"][1].tobytes(), f"frame {k}: host voxel payloads differ"
        grid.debugCheckForDuplicates()
        st = recon.getStats()
        assert (st["blocksStreamedOut"], st["blocksStreamedIn"]) == w["totals"], (k, st, w["totals"])
    st = recon.getStats()
    assert st["frames"] == n
    assert st["streamingFramesPipelined"] == n - n // batch, st  # all but the first frame of every call
    sw = scene.getState()
    assert not sw[[T.STATE_HEAP_UNDERFLOW, T.STATE_INSERT_FAILED]].any(), sw
    recon.close()
    grid.close()
    ray.close()
    scene.close()


def test_last_chunk_and_a_ragged_mask(E, oracle_lib, scene):
    """60 chunks: two words, the second one partial.  The scene has a block in the last chunk; streaming that chunk in and
    out clears and sets bit 59 in both copies of the mask and touches nothing else."""
    O = oracle_lib
    positions, info, _ = scene
    last = G.N_BITS - 1
    n_last = int((info["bit"] == last).sum())
    assert n_last >= 1 and WORDS == 2 and G.N_BITS % 32 != 0
    hp, cp, rp, gs, gg, os_, og = make_pair(E, O, 1, gc=False)  # (without GC the table is alloc's fixed point: the scene fixture's blocks)
    frame = E.DepthFrame(cp)
    for k in G.ALLOC_POSES:
        pose = G.orbit_pose(k)
        E.synth_frame(synth.S1_SPHERES, 0, pose, cp, out=frame)
        gs.integrate(pose, frame, cp, gg.getBitMaskGPU())
        os_.integrate(pose, *O.synth_frame(synth.S1_SPHERES, 0, pose, cp), og.bitmask)
    assert G.pos_set(gs.state(with_voxels=False)["positions"]) == G.pos_set(positions)
    gg.streamOutToCPUAll()
    og.stream_out_to_cpu_all()
    full = G.mask_of_bits(np.unique(info["bit"][info["inside"]]))
    assert full[1] >> (last % 32) == 1
    # before any upload: the host's copy has the bits and says so, the device's copy has none yet
    hostm, devm, dirty = assert_masks(gg, og, "everything out", uploaded=False)
    assert np.array_equal(hostm, full) and dirty and not devm.any()
    gg.getBitMaskGPU()
    assert_masks(gg, og, "everything out, uploaded")
    # the last chunk alone comes back: a sphere around its centre that holds no other chunk's centre
    chunk = np.array(G.MINP) + np.array(G.DIMS) - 1
    centre = (chunk.astype(np.float32) * np.float32(G.EXT[0])).astype(np.float32)
    n_in = gg.streamInToGPU(centre, 0.6, True)
    assert n_in == og.stream_in_to_gpu(centre, 0.6, True) == n_last
    cleared = full.copy()
    cleared[1] &= np.uint32(~np.uint32(1 << (last % 32)))
    hostm, _, dirty = assert_masks(gg, og, "last chunk in", uploaded=False)
    assert np.array_equal(hostm, cleared) and dirty
    gg.getBitMaskGPU()
    _, devm, _ = assert_masks(gg, og, "last chunk in, uploaded")
    assert np.array_equal(devm, cleared) and devm[0] == full[0]
    got = gs.state(with_voxels=False)["positions"]
    assert G.pos_set(got) == G.pos_set(positions[info["bit"] == last])
    # and leaves again: the table holds nothing else, so radius 0 moves just this chunk
    n_out = gg.streamOutToCPU(np.zeros(3, np.float32), 0.0, False)
    assert n_out == og.stream_out_to_cpu(np.zeros(3, np.float32), 0.0, False) == n_last
    gg.getBitMaskGPU()
    hostm, devm, _ = assert_masks(gg, og, "last chunk out again")
    assert np.array_equal(hostm, full) and np.array_equal(devm, full)
    compare(gs, gg, os_, og, "last chunk out again")
    gg.close()
    gs.close()
