"""Crowded hash tables: the two sequences of tests/test_hash_chains.py and tests/test_gpu_crowded_tables.py, in which
buckets overflow into collision lists, and the preconditions under which their outcome cannot depend on the order in
which concurrent allocs ran.

Both are S1 seen from synth.orbit_pose(k, 40), offline, with garbage collection starving every second frame:

  A  96x72, 2 cm voxels, 180 buckets, the default list limit 7, 4 frames: three buckets overflow, none of them next to
     another;
  B  64x48, 4 cm voxels, 23 buckets, a list limit of 256, 8 frames: every bucket is nearly full and eight of them
     overflow, their elements spilling through several neighbours.

ROOMY is the table the rest of the suite uses (2^14 buckets): no bucket overflows in it."""
import numpy as np

from helpers import small_config
from voxelhashing_amd import canonical, synth, vhtypes as T

ROOMY = 1 << 14
POOL = 1 << 11
SCENARIOS = {
    "A": dict(size=(96, 72), params="P2", buckets=180, limit=7, frames=4),
    "B": dict(size=(64, 48), params="P4", buckets=23, limit=256, frames=8),
}


def config(name, buckets=None):
    s = SCENARIOS[name]
    return small_config(s["size"][0], s["size"][1], s["params"], num_buckets=buckets or s["buckets"], num_sdf_blocks=POOL,
                        max_collision_list=s["limit"])


def options(offline=True):
    return T.make_scene_options(offline=offline, gc=True, starve=2)


def poses(name):
    return [synth.orbit_pose(k, 40) for k in range(SCENARIOS[name]["frames"])]


def frames(O, name):
    """-> [(pose, depth, colour)] from the oracle's generator"""
    _, cp, _ = config(name)
    return [(p, *O.synth_frame(synth.S1_SPHERES, 0, p, cp)) for p in poses(name)]


def frame_demand(O, name, depth, color, pose):
    """the blocks a frame's alloc asks for: what alloc to fixed point leaves in an empty roomy table (alloc looks at
    the depth map and the pose only, never at the table)"""
    hp, cp, rp = config(name, ROOMY)
    o = O.OracleScene(hp, cp, rp, options())
    o.set_transform(pose)
    prev = -1
    while o.heap_free_count() != prev:
        prev = o.heap_free_count()
        o.reset_mutex()
        o.alloc(depth, color)
    return canonical.block_positions(o.hash_table())


def union(a, b):
    both = np.unique(np.concatenate([a.reshape(-1, 3), b.reshape(-1, 3)]), axis=0)
    return both[canonical.lexsort_pos(both)]


def bucket_demand(positions, buckets):
    return np.bincount(canonical.hash_buckets(positions, buckets), minlength=buckets)


def assert_precondition_a(positions, buckets, limit):
    """Around every bucket b that holds more than its ten slots: at most 16 blocks (the list walk's `limit` iterations
    reach its 6th element), the bucket behind it has room for what spills over (so no probe of alloc's runs out),
    and the bucket in front does not overflow (its elements would take b's slots).  Overflowing buckets are then never
    neighbours: each takes its two mutexes alone, so every pass in which something is still missing allocates."""
    d = bucket_demand(positions, buckets)
    over = np.nonzero(d > T.HASH_BUCKET_SIZE)[0]
    for b in over:
        nxt, prv = d[(b + 1) % buckets], d[(b - 1) % buckets]
        assert d[b] <= 16, f"bucket {b} is asked for {d[b]} blocks"
        assert d[b] - T.HASH_BUCKET_SIZE < limit, f"bucket {b}: the list walk does not reach its last element"
        assert nxt + d[b] - T.HASH_BUCKET_SIZE <= 7, f"bucket {b} spills {d[b] - 10} blocks into a bucket asked for {nxt}"
        assert prv <= T.HASH_BUCKET_SIZE, f"buckets {(b - 1) % buckets} and {b} both overflow"
    return len(over), int(d.max())


def assert_precondition_b(positions, buckets, limit):
    """The list limit is at least the number of blocks (no walk or probe of alloc's ends early) and the blocks are
    fewer than the table's non-last slots (a probe finds a free one): alloc never answers `no room`."""
    n = len(positions)
    assert limit >= n, f"{n} blocks with a list limit of {limit}"
    assert n < (T.HASH_BUCKET_SIZE - 1) * buckets, f"{n} blocks in {buckets} buckets"
    d = bucket_demand(positions, buckets)
    return int((d > T.HASH_BUCKET_SIZE).sum()), int(d.max())


def oracle_run(O, name, buckets=None, each=None):
    """the sequence through OracleScene.integrate; each(k, scene, pose) after every frame -> the scene"""
    hp, cp, rp = config(name, buckets)
    o = O.OracleScene(hp, cp, rp, options())
    for k, (pose, depth, color) in enumerate(frames(O, name)):
        o.integrate(pose, depth, color)
        if each is not None:
            each(k, o, pose)
    return o


def chains(scene_or_table, hp=None):
    """check_chains of an OracleScene, or of a table with its parameters"""
    if hp is None:
        return canonical.check_chains(scene_or_table.hash_table(), scene_or_table.hp)
    return canonical.check_chains(scene_or_table, hp)


def list_involved(table, hp):
    """per slot: the entry's delete goes through its home bucket's mutex (deleteHashEntryElement: an entry with an
    offset, or one that sits outside its home bucket)"""
    occ = table["ptr"] != T.FREE_ENTRY
    home = canonical.hash_buckets(table["pos"], hp.m_hashNumBuckets)
    slots = np.arange(len(table))
    return occ & ((table["offset"] != 0) | (home != slots // T.HASH_BUCKET_SIZE))


def flagged_positions(scene):
    """positions GC identify flagged, from an OracleScene's compactified list and decisions"""
    return scene.compactified()["pos"][scene.decisions() != 0].reshape(-1, 3)


def lists_of(table, hp):
    """{bucket: [slots of the collision list that hangs off its last slot, in list order]}"""
    bs = T.HASH_BUCKET_SIZE
    last = np.arange(bs - 1, len(table), bs)
    return {int(b): canonical.chain_of(table, hp, int(b)) for b in last[table["offset"][last] != 0] // bs}


def oracle_frame(o, k, pose, depth, color, before_free=None):
    """CUDASceneRepHashSDF::integrate of frame k (offline, GC starving every second frame) launcher by launcher on an
    OracleScene; before_free(scene) runs between GC identify and GC free.  Equal to OracleScene.integrate, which
    test_hash_chains.py checks."""
    o.set_transform(pose)
    prev = -1
    while o.heap_free_count() != prev:
        prev = o.heap_free_count()
        o.reset_mutex()
        o.alloc(depth, color)
    o.compactify()
    o.integrate_depth_map(depth, color)
    if k > 0 and k % 2 == 0:
        o.starve()
    o.gc_identify()
    if before_free is not None:
        before_free(o)
    o.reset_mutex()
    o.gc_free()


def assert_gc_precondition(flagged, ever_over, buckets):
    """GC free lets one delete per pass through a home bucket's mutex, and which of a bucket's blocks are on its list
    depends on the order the allocs ran in: so that one pass frees the same blocks in any order, no bucket that has ever
    overflowed (`ever_over`) is the home of two flagged blocks"""
    if len(flagged):
        per = bucket_demand(flagged, buckets)
        for b in ever_over:
            assert per[b] <= 1, f"bucket {b} has overflowed and is the home of {per[b]} flagged blocks"


class Tokens:
    """lock tokens as CUDASceneRepHashSDF hands them out: positive, a new one for every pass"""

    def __init__(self):
        self.last = 0

    def next(self):
        self.last += 1
        return self.last


def host_copy(O, d, hp, cp, rp=None, opt=None):
    """an OracleScene holding a downloaded device state (table, heap, counter, voxels): the oracle's functions then run
    on the table the device built"""
    host = O.OracleScene(hp, cp, rp, opt)
    for field, key, dt in (("d_hash", "hash", T.HASH_ENTRY_DTYPE), ("d_heap", "heap", np.uint32), ("d_SDFBlocks", "sdf_blocks", T.VOXEL_DTYPE)):
        host.array(field, dt, len(d[key]))[:] = d[key]
    host.array("d_heapCounter", np.uint32, 1)[0] = d["heap_counter"]
    # (CUDARayCastSDF::render leaves the view alone while the count of compactified blocks is 0)
    host.hp.m_numOccupiedBlocks = d["compact_count"] if "compact_count" in d else len(d["compactified"])
    return host


def rows(a):
    """the records of a structured array as sortable byte strings (for comparing sets of them)"""
    a = np.ascontiguousarray(a)
    return np.sort(a.view(np.dtype((np.void, a.dtype.itemsize))).ravel())


def position_set(positions):
    return {tuple(int(v) for v in p) for p in np.asarray(positions).reshape(-1, 3)}


def voxels_by_position(snap):
    """{position: the block's 4096 bytes} of a canonical snapshot"""
    return {tuple(int(v) for v in p): v.tobytes() for p, v in zip(snap["positions"], snap["voxels"])}
