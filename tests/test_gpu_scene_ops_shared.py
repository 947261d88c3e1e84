"""The scene operations' shared scaffolding (vh_scene_ops.hpp: striped counts, the passes that settle lost lock races,
the delete pass) driven by three operations in a row on ONE tiny table: a merge that needs several alloc passes, a cut
that needs several delete passes, a de-integration that frees blocks.  Each operation's counts and the table after it
are what the numpy restatements give (tests/scene_merge.py, tests/scene_cut.py, tests/deintegrate.py).

The blocks are a few dozen of one fused frame of S1 (2 cm voxels), chosen by their home bucket in a table of 13 buckets: 13 that the
cut frees and that share one bucket -- three more than its slots, so a collision list hangs off it -- and 27 from the
other buckets, freed, cut through and untouched ones among them.  How many passes an operation needs at least follows
from the mutexes: an alloc takes its home bucket's, a delete of a list's head or element takes its home bucket's, and a
mutex is granted once per pass."""

import numpy as np
import pytest

import crowded as CR
import deintegrate as DI
import scene_cut as SC
import scene_merge as SM
from helpers import small_config
from voxelhashing_amd import canonical, synth, vhtypes as T

pytestmark = pytest.mark.gpu
BUCKETS = 13
IN_ONE_BUCKET, OTHERS = 13, 27


def test_merge_then_cut_then_deintegrate_on_one_table(vh, oracle_lib):
    from voxelhashing_amd import engine as E
    hp, cp, _ = small_config(64, 48, "P2", num_buckets=BUCKETS, num_sdf_blocks=1 << 7, max_collision_list=256)
    roomy = small_config(64, 48, "P2", num_sdf_blocks=1 << 11)[0]
    vs = np.float32(hp.m_virtualVoxelSize)
    assert vs == np.float32(roomy.m_virtualVoxelSize)

    # one frame of S1 fused in a roomy table: the blocks to choose from, and the frame to take out again
    pose = synth.orbit_pose(0, 40)
    frame = E.synth_frame(synth.S1_SPHERES, 0, pose, cp)
    maps = frame.download()
    fused = E.CUDASceneRepHashSDF(roomy, T.make_scene_options(offline=True, gc=False))
    fused.integrate(pose, frame, cp, None)
    pos, vox = SM.scene_of(fused.state())

    # the region: a rotated box with one face through the median of the observed voxels, the others far away
    coords = SC.voxel_coords(pos)[vox["weight"] > 0].astype(np.float64) * float(vs)
    R = SC.rotation([(2, 0.3), (1, -0.2)])
    m = E.cut_region_transform(SC.frame(R, np.median(coords, axis=0) + R @ np.array([50.0, 0.0, 0.0])), (50.0, 50.0, 50.0), vs)
    whole = SC.cut((pos, vox), m, T.CUT_BOX, 0)
    freed_by_cut = CR.position_set(whole["freed"])
    is_freed = np.array([tuple(int(v) for v in p) in freed_by_cut for p in pos])
    home = canonical.hash_buckets(pos, BUCKETS)
    b = int(np.argmax(np.bincount(home[is_freed], minlength=BUCKETS)))
    one = np.nonzero(is_freed & (home == b))[0][:IN_ONE_BUCKET]
    assert len(one) == IN_ONE_BUCKET, f"bucket {b} is home to only {len(one)} blocks the cut frees"
    rest = np.nonzero(home != b)[0]
    rest = rest[np.random.default_rng(5).permutation(len(rest))[:OTHERS]]
    pick = np.concatenate([one, rest])
    scene = SM.sort_scene(pos[pick], vox[pick])
    n = len(pick)
    assert n == IN_ONE_BUCKET + OTHERS
    demand = CR.bucket_demand(scene[0], BUCKETS)
    assert demand[b] == IN_ONE_BUCKET > T.HASH_BUCKET_SIZE + 2

    # 1. the merge into the empty table: every block is new, every observed voxel copied
    g = E.LauncherScene(hp)
    descs = np.zeros(n, T.DESC_DTYPE)
    descs["pos"] = scene[0]
    want = SM.merge(SM.empty_scene(), scene, hp, free_blocks=hp.m_numSDFBlocks)
    got = g.merge_blocks(descs, scene[1], 1)
    print("merge", {k: v for k, v in got.items() if k != "left_out_indices"})
    SM.assert_counts(got, want["counts"], "merge")
    assert (got["allocated"], got["left_out"], got["combined"]) == (n, 0, 0) and got["copied"] == int((scene[1]["weight"] > 0).sum())
    assert len(got["left_out_indices"]) == 0
    assert demand.max() <= got["alloc_passes"] <= n + 8, "a bucket's mutex is granted to one alloc per pass"
    after = g.state()
    assert np.array_equal(after["positions"], want["positions"]) and after["voxels"].tobytes() == want["voxels"].tobytes(), "merge: the table differs"
    assert after["heap_free"] == hp.m_numSDFBlocks - n

    # 2. the cut: the blocks of bucket b all go, the head of its list and the list's elements through b's mutex
    table = after["raw"]["hash"]
    assert canonical.check_chains(table, hp)["listed"] >= IN_ONE_BUCKET - T.HASH_BUCKET_SIZE
    through_b = int((CR.list_involved(table, hp) & (canonical.hash_buckets(table["pos"], BUCKETS) == b)).sum())
    assert through_b >= 3
    want = SC.cut(scene, m, T.CUT_BOX, 0)
    assert CR.position_set(scene[0][canonical.hash_buckets(scene[0], BUCKETS) == b]) <= CR.position_set(want["freed"])
    assert 0 < len(want["freed"]) < n and want["counts"]["touched"] > want["counts"]["freed"], "the region was meant to cut through blocks"
    got = g.cut_blocks(m, T.CUT_BOX, 0, 2)
    print("cut", {k: got[k] for k in T.CUT_COUNTS})
    assert got["code"] == 0
    SC.assert_counts(got, want["counts"], "cut")
    assert got["unsettled"] == 0 and through_b <= got["delete_passes"] <= got["freed"] + 8
    after = g.state()
    assert np.array_equal(after["positions"], want["positions"]) and after["voxels"].tobytes() == want["voxels"].tobytes(), "cut: the table differs"
    assert after["heap_free"] == hp.m_numSDFBlocks - len(want["positions"])

    # 3. the frame taken out of what the cut left: blocks it leaves without an observed voxel go back to the heap
    left = SM.scene_of(after)
    want = DI.deintegrate(left, maps, pose, hp, cp)
    assert len(want["freed"]) > 0
    got = g.deintegrate_blocks(frame, cp, pose, oracle_lib.mat4_inverse(pose), 3)
    print("de-integration", got)
    assert got["code"] == 0
    DI.assert_counts(got, want["counts"], "de-integration")
    assert got["unsettled"] == 0 and 0 < got["delete_passes"] <= got["freed"] + 8
    after = g.state()
    assert np.array_equal(after["positions"], want["positions"]) and after["voxels"].tobytes() == want["voxels"].tobytes(), "de-integration: the table differs"
    assert after["heap_free"] == hp.m_numSDFBlocks - len(want["positions"])
    assert after["raw"]["state"][T.STATE_HEAP_UNDERFLOW] == 0

