"""The collision lists of the hash table on the CPU: canonical.check_chains on tables the oracle built and on copies of
them broken by hand, one thing at a time; and that the size of the table cannot be seen in what the oracle computes --
a table so crowded that buckets overflow into lists against the 2^14 buckets of the rest of the suite."""
import ctypes as C

import numpy as np
import pytest

import crowded as CR
from helpers import bits
from voxelhashing_amd import canonical, synth, vhtypes as T

BS = T.HASH_BUCKET_SIZE


def _serial_scenario(O):
    """the table of test_gpu_launchers.py::test_collision_lists_match_oracle_slot_by_slot: 7 buckets, 16 blocks of
    bucket 3 and 8 of bucket 4, deletes of a head, list elements and plain slots, re-allocs; one op per lock pass"""
    rng = np.random.default_rng(5)
    nb = 7
    hp = T.make_hash_params(nb, 64, **synth.PARAM_SETS["P4"])
    o = O.OracleScene(hp, T.make_depth_camera_params(8, 8))

    def in_bucket(bucket, count):
        out = []
        while len(out) < count:
            p = rng.integers(-40, 40, 3)
            if canonical.hash_buckets(p, nb)[0] == bucket and not any((p == q).all() for q in out):
                out.append(p)
        return out

    a, b = in_bucket(3, 16), in_bucket(4, 8)
    for p in a[:12] + b[:8] + a[12:]:
        o.alloc_block(p)
        o.reset_mutex()
    for p in [a[9], a[13], a[0], a[11], a[15], b[2]]:
        o.delete_block(p)
        o.reset_mutex()
    for p in [a[9], a[0], a[13]]:
        o.alloc_block(p)
        o.reset_mutex()
    return o


@pytest.fixture(scope="module")
def tables(oracle_lib):
    """{name: (a copy of the oracle's table, its parameters)} -- the copies are never written; tests break copies of them"""
    out = {}
    o = _serial_scenario(oracle_lib)
    out["serial"] = (o.hash_table().copy(), o.hp)
    for name in CR.SCENARIOS:
        o = CR.oracle_run(oracle_lib, name)
        out[name] = (o.hash_table().copy(), o.hp)
    return out


@pytest.mark.parametrize("name,listed,longest,heads", [("serial", 2, 2, 1), ("A", 7, 4, 3), ("B", 20, 5, 8)])
def test_the_oracles_lists_pass(tables, name, listed, longest, heads):
    table, hp = tables[name]
    got = canonical.check_chains(table, hp)
    assert got == dict(listed=listed, longest=longest, heads=heads)
    assert sum(len(c) for c in CR.lists_of(table, hp).values()) == listed
    # counted another way: the entries that sit outside their home bucket are the listed ones
    slots = np.nonzero(table["ptr"] != T.FREE_ENTRY)[0]
    assert int((canonical.hash_buckets(table["pos"][slots], hp.m_hashNumBuckets) != slots // BS).sum()) == listed


def test_hash_buckets_is_the_oracles_hash(oracle_lib):
    rng = np.random.default_rng(2)
    pos = np.concatenate([rng.integers(-2000, 2000, (500, 3)), rng.integers(-2 ** 31, 2 ** 31, (500, 3))]).astype(np.int32)
    for nb in (7, 23, 180, 1 << 14, 500000):
        hp = T.make_hash_params(nb, 64, **synth.PARAM_SETS["P4"])
        want = [oracle_lib.lib().vho_compute_hash_pos(C.byref(hp), p.ctypes.data_as(C.POINTER(C.c_int32))) for p in pos]
        assert np.array_equal(canonical.hash_buckets(pos, nb), want)


def _offset_to(slot, bucket, ne):
    return (slot - (bucket * BS + BS - 1)) % ne


def _break(table, hp, what):
    """one defect in a copy of the table -> the message check_chains must give"""
    t = table.copy()
    ne = len(t)
    lists = CR.lists_of(t, hp)
    occ = t["ptr"] != T.FREE_ENTRY
    b, chain = max(lists.items(), key=lambda kv: len(kv[1]))  # the longest list
    last = b * BS + BS - 1
    links = [last] + chain  # links[k] links to chain[k]
    if what == "zero the link to the last element":
        t["offset"][links[len(chain) - 1]] = 0
        return t, "not found from their home bucket"
    if what == "zero the link of the head":
        assert len(chain) >= 2
        t["offset"][last] = 0
        return t, "neither a bucket's last slot nor on a list"
    if what == "link to a free slot":
        free = [i for i in np.nonzero(~occ)[0] if i % BS != BS - 1]
        t["offset"][links[len(chain) - 1]] = _offset_to(free[0], b, ne)
        return t, "lands on the free slot"
    if what == "link to another bucket's last slot":
        other = [i for i in range(BS - 1, ne, BS) if occ[i] and i != last]
        t["offset"][links[len(chain) - 1]] = _offset_to(other[0], b, ne)
        return t, "the last slot of bucket"
    if what == "swap two lists' tails":
        (b1, c1), (b2, c2) = sorted(lists.items())[:2]
        t["offset"][b1 * BS + BS - 1] = _offset_to(c2[0], b1, ne)
        t["offset"][b2 * BS + BS - 1] = _offset_to(c1[0], b2, ne)
        return t, "whose entry belongs to bucket"
    if what == "two lists share a tail":
        (b1, c1), (b2, c2) = sorted(lists.items())[:2]
        t["offset"][c2[-1]] = _offset_to(c1[-1], b2, ne)
        return t, "is on the lists of buckets"
    if what == "close a cycle":
        assert len(chain) >= 2
        t["offset"][chain[-1]] = _offset_to(chain[0], b, ne)
        return t, "a cycle"
    if what == "offset on a plain slot":
        home = canonical.hash_buckets(t["pos"], hp.m_hashNumBuckets)
        on_list = {i for c in lists.values() for i in c}
        plain = [i for i in np.nonzero(occ)[0] if i % BS != BS - 1 and home[i] == i // BS and i not in on_list]
        t["offset"][plain[0]] = 3
        return t, "an entry in its own bucket"
    if what == "entry moved out of its bucket":
        home = canonical.hash_buckets(t["pos"], hp.m_hashNumBuckets)
        on_list = {i for c in lists.values() for i in c}
        plain = [i for i in np.nonzero(occ)[0] if i % BS != BS - 1 and home[i] == i // BS and i not in on_list]
        free = [i for i in np.nonzero(~occ)[0] if i % BS != BS - 1 and i // BS != home[plain[0]]]
        t[free[0]] = t[plain[0]]
        t[plain[0]]["ptr"], t[plain[0]]["pos"] = T.FREE_ENTRY, 0
        return t, "not found from their home bucket"
    raise KeyError(what)


BREAKS = ["zero the link to the last element", "zero the link of the head", "link to a free slot", "link to another bucket's last slot",
          "swap two lists' tails", "two lists share a tail", "close a cycle", "offset on a plain slot", "entry moved out of its bucket"]


@pytest.mark.parametrize("what", BREAKS)
@pytest.mark.parametrize("name", ["A", "B"])
def test_each_clause_fires_on_a_broken_table(tables, name, what):
    table, hp = tables[name]
    broken, message = _break(table, hp, what)
    assert int((broken != table).sum()) in (1, 2), "break one thing at a time"
    with pytest.raises(AssertionError, match=message):
        canonical.check_chains(broken, hp)
    canonical.check_chains(table, hp)  # (the fixture's table is as it was)


@pytest.mark.parametrize("what", ["zero the link to the last element", "zero the link of the head", "link to a free slot",
                                  "link to another bucket's last slot", "close a cycle", "offset on a plain slot"])
def test_each_clause_fires_on_the_serial_scenarios_table(tables, what):
    """(one list only: the breaks that need two are left to A and B)"""
    table, hp = tables["serial"]
    broken, message = _break(table, hp, what)
    with pytest.raises(AssertionError, match=message):
        canonical.check_chains(broken, hp)


def test_an_element_beyond_the_walks_limit_is_not_found(tables):
    """getHashEntryForSDFBlockPos looks at the last slot and then at limit - 1 elements: A's list of four elements is
    within the limit 7 and beyond a limit of 4"""
    table, hp = tables["A"]
    short = type(hp)()
    C.memmove(C.byref(short), C.byref(hp), C.sizeof(hp))
    short.m_hashMaxCollisionLinkedListSize = 5
    canonical.check_chains(table, short)
    short.m_hashMaxCollisionLinkedListSize = 4
    with pytest.raises(AssertionError, match="not found from their home bucket"):
        canonical.check_chains(table, short)


def test_check_invariants_runs_the_chain_check(tables, oracle_lib):
    o = CR.oracle_run(oracle_lib, "B")
    counter = int(o.array("d_heapCounter", np.uint32, 1)[0])
    got = canonical.check_invariants(o.hash_table(), o.heap(), counter, o.hp, o.sdf_blocks())
    assert got["listed"] == 20 and got["heads"] == 8
    broken, message = _break(o.hash_table(), o.hp, "zero the link to the last element")
    with pytest.raises(AssertionError, match=message):
        canonical.check_invariants(broken, o.heap(), counter, o.hp, o.sdf_blocks())


def test_assert_same_scene_without_bucket_counts(tables, oracle_lib):
    """bucket_counts=False drops the per-bucket occupancy and nothing else"""
    crowded, roomy = CR.oracle_run(oracle_lib, "B").state(), CR.oracle_run(oracle_lib, "B", CR.ROOMY).state()
    with pytest.raises(AssertionError, match="per-bucket occupancy"):
        canonical.assert_same_scene(crowded, dict(crowded, bucket_counts=crowded["bucket_counts"][::-1].copy()), "reversed")
    canonical.assert_same_scene(crowded, dict(crowded, bucket_counts=crowded["bucket_counts"][::-1].copy()), "reversed", bucket_counts=False)
    for field, message in (("positions", "position sets"), ("heap_free", "heap free"), ("voxels", "voxel")):
        other = dict(crowded)
        if field == "heap_free":
            other[field] = crowded[field] + 1
        else:
            other[field] = crowded[field].copy()
            other[field].view(np.uint8).reshape(-1)[-1] ^= 1
        with pytest.raises(AssertionError, match=message):
            canonical.assert_same_scene(crowded, other, field, bucket_counts=False)
    assert len(roomy["bucket_counts"]) != len(crowded["bucket_counts"])


@pytest.mark.parametrize("name,blocks,listed,heads,longest", [("A", 575, 7, 3, 4), ("B", 199, 20, 8, 5)])
def test_table_size_is_invisible_to_the_oracle(oracle_lib, name, blocks, listed, heads, longest):
    """after every frame: the same positions, heap count, voxel bytes and the four ray-cast maps bit for bit on the
    crowded table and on 2^14 buckets; and the sequence meets the precondition the GPU tests rely on"""
    O = oracle_lib
    s = CR.SCENARIOS[name]
    roomy = []
    CR.oracle_run(O, name, CR.ROOMY, lambda k, o, pose: roomy.append((o.state(), o.render(pose))))
    fr = CR.frames(O, name)
    seen = dict(prev=np.zeros((0, 3), np.int32), over=0)

    def each(k, o, pose):
        st = o.state()
        counter = int(o.array("d_heapCounter", np.uint32, 1)[0])
        canonical.check_invariants(o.hash_table(), o.heap(), counter, o.hp, o.sdf_blocks())
        canonical.assert_same_scene(st, roomy[k][0], f"{name} frame {k}", bucket_counts=False)
        assert st["voxels"].tobytes() == roomy[k][0]["voxels"].tobytes()
        maps = o.render(pose)
        for key in ("depth", "depth4", "normals", "colors"):
            assert np.array_equal(bits(maps[key]), bits(roomy[k][1][key])), f"{name} frame {k}: map {key}"
        assert (maps["depth"] != -np.inf).sum() > 1000
        demand = CR.union(seen["prev"], CR.frame_demand(O, name, fr[k][1], fr[k][2], fr[k][0]))
        pre = CR.assert_precondition_a if name == "A" else CR.assert_precondition_b
        seen["over"], _ = pre(demand, s["buckets"], s["limit"])
        seen["prev"] = st["positions"]

    o = CR.oracle_run(O, name, None, each)
    assert o.state()["num_occupied"] == blocks
    assert CR.chains(o) == dict(listed=listed, longest=longest, heads=heads)
    assert seen["over"] >= 3
