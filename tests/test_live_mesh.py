"""The live mesh's definition ("Live mesh") on the CPU: the numpy restatement's digest on hand-made
blocks, the claim that a block's triangles depend on its 27-block neighbourhood alone -- on the oracle -- and the
restatement's update of a cache against the oracle's full extraction.  No GPU.

Scene: S1 64x48 P2, three frames of its orbit (the third from further round than the GPU tests of
tests/test_gpu_live_mesh.py take it: OracleFrames says why).  A block's triangles are the oracle's extraction in the box
that spans the block's voxel centres."""
import numpy as np
import pytest

import live_mesh as LM
from helpers import small_config
from voxelhashing_amd import synth, vhtypes as T


# ---------------------------------------------------------------------------- the digest

def hand_made_block(seed=7):
    rng = np.random.default_rng(seed)
    v = np.zeros(T.SDF_BLOCK_VOXELS, dtype=T.VOXEL_DTYPE)
    v["sdf"] = rng.standard_normal(T.SDF_BLOCK_VOXELS).astype(np.float32) * np.float32(0.05)
    v["color"] = rng.integers(0, 256, size=(T.SDF_BLOCK_VOXELS, 3), dtype=np.uint8)
    v["weight"] = rng.integers(1, 200, size=T.SDF_BLOCK_VOXELS, dtype=np.uint8)
    return v


def test_digest_is_the_salted_sum_of_mixed_words():
    v = hand_made_block()
    w = v.view("<u8")
    assert int(w[5]) == int(v["sdf"][5:6].view(np.uint32)[0]) | (int(v["color"][5, 0]) << 32) | (int(v["color"][5, 1]) << 40) | \
        (int(v["color"][5, 2]) << 48) | (int(v["weight"][5]) << 56)
    want = 0
    for i in range(T.SDF_BLOCK_VOXELS):  # in Python integers
        k = (int(w[i]) + (i + 1) * 0x9E3779B97F4A7C15) % (1 << 64)
        k ^= k >> 33
        k = (k * 0xff51afd7ed558ccd) % (1 << 64)
        k ^= k >> 33
        k = (k * 0xc4ceb9fe1a85ec53) % (1 << 64)
        k ^= k >> 33
        want = (want + k) % (1 << 64)
    assert LM.digest(v) == want
    pool = np.concatenate([hand_made_block(1), v, hand_made_block(2)])
    assert [int(d) for d in LM.digests(pool, [512, 0, 1024])] == [want, LM.digest(hand_made_block(1)), LM.digest(hand_made_block(2))]
    assert LM.digest(np.zeros(T.SDF_BLOCK_VOXELS, dtype=T.VOXEL_DTYPE)) != 0  # the salt: an empty block is not digest 0


def test_digest_sees_every_kind_of_edit():
    v = hand_made_block()
    base = LM.digest(v)
    s = v.copy()
    assert s[3].tobytes() != s[200].tobytes()
    s[[3, 200]] = s[[200, 3]]  # two different voxels change places: the same multiset of words
    assert LM.digest(s) != base
    c = v.copy()
    c["color"][100, 1] ^= 1  # a colour byte alone
    assert LM.digest(c) != base
    w = v.copy()
    w["weight"][511] += 1  # the weight byte alone
    assert LM.digest(w) != base
    z = v.copy()
    z["sdf"][0] = np.float32(0.0)
    plus = LM.digest(z)
    z["sdf"][0] = np.float32(-0.0)  # equal as floats, another bit pattern
    assert z["sdf"][0] == np.float32(0.0) and LM.digest(z) != plus
    assert LM.digest(v.copy()) == base


# ---------------------------------------------------------------------------- on the oracle

NUM_BUCKETS, NUM_BLOCKS = 1 << 12, 1 << 12
THIRD_POSE = 33


class OracleFrames:
    """the S1 64x48 P2 oracle scene, a frame at a time"""

    def __init__(self, O):
        self.hp, self.cp, _ = small_config(64, 48, params="P2", num_buckets=NUM_BUCKETS, num_sdf_blocks=NUM_BLOCKS)
        self.spheres, self.inside, radius = synth.scene("S1")
        # The third frame looks from a third of the way round the orbit: from the next orbit position (as the GPU tests
        # take it) it changes 438 of the scene's 462 blocks and R is every block, which leaves the claim nothing to say.
        self.poses = [synth.orbit_pose(k, 100, radius) for k in (0, 1, THIRD_POSE)]
        self.O = O
        self.scene = O.OracleScene(self.hp, self.cp, options=T.make_scene_options(offline=True, gc=False))
        self.vs = np.float32(self.hp.m_virtualVoxelSize)

    def integrate(self, k):
        depth, color = self.O.synth_frame(self.spheres, self.inside, self.poses[k], self.cp)
        self.scene.integrate(self.poses[k], depth, color)

    def tables(self):
        return self.scene.hash_table().copy(), self.scene.sdf_blocks().copy()

    def extract(self, block=None):
        """the oracle's triangles, sorted: of the whole scene, or in the box that spans `block`'s voxel centres"""
        mp = T.make_marching_cubes_params(self.hp, 1 << 18)
        if block is not None:
            mp.m_boxEnabled = 1
            for a in range(3):
                mp.m_minCorner[a] = np.float32(8 * block[a]) * self.vs  # vvp_to_world of the first and the last voxel
                mp.m_maxCorner[a] = np.float32(8 * block[a] + 7) * self.vs
        tris, n = self.scene.extract_iso_surface(mp)
        assert n == len(tris)
        return np.sort(np.ascontiguousarray(tris).view(np.dtype((np.void, T.TRIANGLE_DTYPE.itemsize))).ravel())


@pytest.fixture(scope="module")
def walk(oracle_lib):
    """the scene integrated frame by frame with an update of the restatement's cache after each -> per frame the plan,
    the counts of blocks dropped and added, and whether the cache equalled the oracle's full extraction; then, for the
    dependency claim, the boxed extractions before and after the third frame"""
    F = OracleFrames(oracle_lib)
    records, cache, steps = LM.new_records(NUM_BLOCKS), {}, []
    before = {}
    for k in range(3):
        F.integrate(k)
        table, pool = F.tables()
        plan = LM.update(records, k + 1, table, pool)
        gone, added = LM.apply(cache, plan, F.extract)
        full = F.extract()
        mine = np.sort(np.concatenate([v for v in cache.values()] + [full[:0]]))
        steps.append(dict(plan=plan, gone=gone, added=added, equal=len(mine) == len(full) and mine.tobytes() == full.tobytes(), triangles=len(full)))
        if k == 1:  # every resident block's own triangles in the state before the third frame, extracted afresh
            before = {p: F.extract(p) for p in plan["resident"]}
    return dict(F=F, steps=steps, before=before, cache=cache)


def test_update_of_the_cache_equals_the_full_extraction_after_every_frame(walk):
    for k, s in enumerate(walk["steps"]):
        print(k, {n: len(s["plan"][n]) for n in ("resident", "changed", "vanished", "R")}, s["gone"], s["added"], s["triangles"])
        assert s["triangles"] > 100 and s["equal"], f"frame {k + 1}"
    first = walk["steps"][0]["plan"]
    assert len(first["changed"]) == len(first["resident"]) == len(first["R"]) > 50 and not first["vanished"]  # the first update is the full one
    third = walk["steps"][2]["plan"]
    assert 0 < len(third["R"]) < len(third["resident"])  # and a later one is not


def test_a_blocks_triangles_depend_on_its_27_blocks_alone(walk):
    """frame 3 changes the blocks of C; the 8 resident blocks outside R nearest to C give bit-identical boxed extractions
    before and after it, and a block of R does not"""
    F, plan, before = walk["F"], walk["steps"][2]["plan"], walk["before"]
    C = np.array(sorted(plan["C"]), dtype=np.int64)
    outside = [p for p in plan["resident"] if p not in plan["R"]]
    assert len(outside) >= 8 and len(C) > 0
    dist = {p: int(np.min(np.max(np.abs(C - np.array(p, dtype=np.int64)), axis=1))) for p in outside}
    nearest = sorted(outside, key=lambda p: (dist[p], p))[:8]
    assert all(dist[p] >= 2 for p in nearest) and dist[nearest[0]] == 2  # just outside the neighbourhood
    for p in nearest:
        assert p in before, p  # not changed, so resident before the frame too
        now = F.extract(p)
        assert len(now) == len(before[p]) and now.tobytes() == before[p].tobytes(), p
    assert sum(len(before[p]) for p in nearest) > 0  # (they are not all empty blocks)
    differing = [p for p in sorted(plan["R"]) if p not in before or F.extract(p).tobytes() != before[p].tobytes()]
    assert differing, "no block of R changed its triangles"
    assert any(p in before for p in differing)


# ---------------------------------------------------------------------------- the replay tool

@pytest.mark.parametrize("flags, message", [(["--live-mesh-every", "2"], "--live-mesh-every: a number of frames, with --mesh and --indexed-mesh"),
                                            (["--indexed-mesh", "--live-mesh-every", "-1"], "--live-mesh-every: a number of frames"),
                                            (["--indexed-mesh", "--live-mesh-every", "2", "--native"], "--live-mesh-every: not with --native")])
def test_replay_refuses_bad_live_mesh_options(tmp_path, flags, message):
    """a usage error, before the tool looks for a GPU"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "replay.py"), "--params", str(tmp_path / "none.txt"), "--mesh", str(tmp_path / "m.ply")] + flags,
                       capture_output=True, text=True)
    assert r.returncode == 2 and message in r.stderr and not (tmp_path / "m.ply").exists()
