"""World-chunk streaming at the edges of the chunk grid, on the CPU: the restatement of tests/grid_edges.py against the
oracle twin of the host grid, the oracle's alloc under crafted bit masks whose neighbouring words are all ones, and
the drop of blocks whose chunk does not exist.  tests/test_gpu_streaming_grid_edges.py holds the GPU to the same sets."""
import numpy as np
import pytest

import grid_edges as G
from grid_edges import CRAFTED_BITS, MASK_CASES, case_mask, expected_blocks, oracle_blocks

@pytest.fixture(scope="module")
def scene(oracle_lib):
    """the unmasked block set of the scene at the origin, classified; the conditions on it asserted"""
    o, hp = oracle_blocks(oracle_lib)
    positions = o.state()["positions"].copy()
    info = G.check_conditions(positions, hp.m_virtualVoxelSize)
    print(f"grid edges, scene at the origin: {len(positions)} blocks, {info['n_inside']} inside / {info['n_outside']} outside "
          f"(past x-low, x-high, y-low, y-high, z-low, z-high: {info['face'][~info['inside']].sum(axis=0).tolist()}), "
          f"{info['ties']} near-tie coordinates, unguarded index {info['unguarded_range']}, {info['aliased']} alias a real bit")
    return positions, info, hp


def test_conditions_hold_for_both_copies_of_the_scene(scene, oracle_lib):
    positions, info, hp = scene
    # the figures of the scene this suite was designed on (they are inputs: a change of synth or of P4 must be noticed)
    assert (len(positions), info["n_inside"], info["n_outside"]) == (219, 156, 63)
    assert info["face"][~info["inside"]].sum(axis=0).tolist() == [21, 0, 30, 5, 0, 10]
    assert info["ties"] == 333 and info["aliased"] == 54
    assert (int(info["unguarded"][~info["inside"]].min()), int(info["unguarded"][~info["inside"]].max())) == (8, 69)
    # the crafted chunks are what their comment says
    ins = np.bincount(info["bit"][info["inside"]], minlength=G.N_BITS)
    u = info["unguarded"][~info["inside"]]
    alias = np.bincount(u[u < G.N_BITS], minlength=G.N_BITS)
    assert all(ins[b] > 0 for b in CRAFTED_BITS), ins
    assert CRAFTED_BITS[-1] == G.N_BITS - 1 and alias[20] >= 4 and alias[23] >= 4 and alias[59] >= 1
    assert (u >= G.N_BITS).sum() >= 3, "some unguarded indices must land in the guard words"
    # the shifted copy (online tests): same conditions with its own grid
    o, hp2 = oracle_blocks(oracle_lib, shifted=True, minp=G.SHIFTED_MINP)
    shifted = G.check_conditions(o.state()["positions"], hp2.m_virtualVoxelSize, minp=G.SHIFTED_MINP)
    print(f"grid edges, shifted scene: {shifted['n_inside']} inside / {shifted['n_outside']} outside, {shifted['ties']} near-tie "
          f"coordinates, unguarded index {shifted['unguarded_range']}")
    assert shifted["faces"].sum() >= 3


def test_restatement_equals_the_oracle_twin(scene, oracle_lib):
    from oracle.chunk_grid import OracleChunkGrid
    positions, info, hp = scene
    og = OracleChunkGrid(None, G.EXT, G.DIMS, G.MINP, 1)
    world = G.block_to_world(positions, hp.m_virtualVoxelSize)
    for w, chunk, inside, raw in zip(world, info["chunk"], info["inside"], info["unguarded"]):
        c = og.world_to_chunks(w)
        assert c == chunk.tolist()
        assert og.is_valid_chunk(c) == bool(inside)
        assert og.linearize(c) == int(raw) & 0xFFFFFFFF
    # one ulp either side of the rounding ties +-(k + 1/2) extents, and the ties themselves
    ext = np.float32(G.EXT[0])
    coords = []
    for k in range(0, 6):
        t = np.float32(np.float32(k + 0.5) * ext)
        for s in (1.0, -1.0):
            v = np.float32(s) * t
            coords += [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]
    coords = np.array(coords, dtype=np.float32)
    pts = np.stack([coords, coords[::-1], np.roll(coords, 7)], axis=1)
    got = G.world_to_chunks(pts)
    assert len(set(got[:, 0].tolist())) >= 12, "the points must straddle the ties"
    for p, c in zip(pts, got):
        twin = og.world_to_chunks(p)
        assert twin == c.tolist(), (p, twin, c)
        assert og.is_valid_chunk(twin) == bool(G.chunk_inside(c)[0])
        assert og.linearize(twin) == int(G.unguarded_index(c)[0])


@pytest.mark.parametrize("case", MASK_CASES)
def test_oracle_alloc_under_a_crafted_mask(scene, oracle_lib, case):
    """The mask is a slice from the middle of an array whose other words are all ones: a read through an unguarded
    index finds 'streamed out' there (or another chunk's bit inside the mask) and the outside-grid block goes missing."""
    positions, info, hp = scene
    whole, mask = case_mask(case)
    o, _ = oracle_blocks(oracle_lib, mask)
    got = G.pos_set(o.state()["positions"])
    want = expected_blocks(case, positions, info)
    assert got == want, f"mask '{case}': {len(want - got)} blocks missing, {len(got - want)} unexpected (of {len(want)})"
    outside = G.pos_set(positions[~info["inside"]])
    assert outside <= got, "a block whose chunk is outside the grid is never streamed out"
    if case == "all":
        assert got == outside
    if case == "crafted":
        assert len(want) == len(positions) - sum(int((info["bit"] == b).sum()) for b in CRAFTED_BITS) < len(positions)
    assert (whole[:G.GUARD_WORDS] == 0xFFFFFFFF).all() and (whole[-G.GUARD_WORDS:] == 0xFFFFFFFF).all()


def test_blocks_outside_the_grid_are_dropped_on_stream_out(scene, oracle_lib):
    """integrateInChunkGrid ("Chunk out of bounds", the reference's behaviour): a block that streams out while its chunk
    is outside the grid leaves the table, its heap slot returns, and it is gone -- no entry on the host, no bit"""
    from oracle.chunk_grid import OracleChunkGrid
    positions, info, hp = scene
    o, _ = oracle_blocks(oracle_lib)
    og = OracleChunkGrid(o, G.EXT, G.DIMS, G.MINP, 1)
    n = og.stream_out_to_cpu(np.zeros(3, np.float32), 0.0, False)  # radius 0: every block leaves
    assert n == len(positions), "the count of a pass includes the dropped blocks"
    st = o.state()
    assert st["num_occupied"] == 0 and st["heap_free"] == hp.m_numSDFBlocks
    descs, _ = og.host_blocks()
    assert G.pos_set(descs["pos"]) == G.pos_set(positions[info["inside"]])
    assert len(descs) == info["n_inside"]
    assert np.array_equal(og.bitmask, G.mask_of_bits(np.unique(info["bit"][info["inside"]])))
    assert og.statistics()["bits"] == len(np.unique(info["bit"][info["inside"]]))
