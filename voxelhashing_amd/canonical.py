"""Canonical forms and structural invariants of a voxel-hash scene.

The reference's block->heap-slot assignment, slot order inside a bucket and
compactified order depend on thread scheduling
(DepthSensingCUDA/Source/VoxelUtilHashSDF.h:587-595), so parity is defined on
canonical forms: the sorted set of block positions, voxel payloads keyed by
position, per-bucket occupancy counts and the heap free count.

check_invariants() restates CUDASceneRepHashSDF::debugHash
(DepthSensingCUDA/Source/CUDASceneRepHashSDF.h:129-233) and
CUDASceneRepChunkGrid::debugCheckForDuplicates (CUDASceneRepChunkGrid.cpp:313-341).
"""
import numpy as np

from . import vhtypes as T


def lexsort_pos(pos):
    """order that sorts [n,3] int positions by (x, y, z)"""
    if len(pos) == 0:
        return np.zeros(0, dtype=np.int64)
    return np.lexsort((pos[:, 2], pos[:, 1], pos[:, 0]))


def block_positions(hash_table):
    """sorted positions of the allocated blocks of a hash table"""
    occ = hash_table["ptr"] != T.FREE_ENTRY
    pos = np.ascontiguousarray(hash_table["pos"][occ])
    return pos[lexsort_pos(pos)]


def snapshot(hash_table, sdf_blocks, heap, heap_counter, hp, with_voxels=True):
    occ = hash_table["ptr"] != T.FREE_ENTRY
    idx = np.nonzero(occ)[0]
    pos = hash_table["pos"][idx]
    ptr = hash_table["ptr"][idx]
    order = lexsort_pos(pos)
    pos = np.ascontiguousarray(pos[order])
    ptr = ptr[order]
    bucket_counts = np.bincount(idx // T.HASH_BUCKET_SIZE, minlength=hp.m_hashNumBuckets).astype(np.uint32)
    snap = dict(
        positions=pos,
        ptrs=ptr,
        slots=idx[order],
        bucket_counts=bucket_counts,
        heap_free=(int(heap_counter) + 1) & 0xFFFFFFFF,  # the counter is the top index: -1 (wrapped) when empty
        num_occupied=int(len(idx)),
    )
    if with_voxels:
        if len(ptr):
            vox = sdf_blocks.reshape(-1, T.SDF_BLOCK_VOXELS)[ptr // T.SDF_BLOCK_VOXELS]
        else:
            vox = np.zeros((0, T.SDF_BLOCK_VOXELS), dtype=T.VOXEL_DTYPE)
        snap["voxels"] = np.ascontiguousarray(vox)
    return snap


def check_invariants(hash_table, heap, heap_counter, hp, sdf_blocks=None):
    """debugHash: free-list has no duplicates; no block is both free and
    allocated; every block is free or allocated; no duplicate positions; no
    LOCK_ENTRY left behind.  With sdf_blocks: every free block is all-zero.  Plus check_chains: the collision lists."""
    n_blocks = hp.m_numSDFBlocks
    n_free = (int(heap_counter) + 1) & 0xFFFFFFFF  # the counter is the top index: -1 (wrapped) when empty
    assert 0 <= n_free <= n_blocks, f"heap counter out of range: {heap_counter}"
    free_ids = heap[:n_free].astype(np.int64)
    assert free_ids.min(initial=0) >= 0 and free_ids.max(initial=0) < n_blocks
    assert len(np.unique(free_ids)) == n_free, "duplicate free pointers in heap array"
    occ = hash_table["ptr"] != T.FREE_ENTRY
    ptrs = hash_table["ptr"][occ].astype(np.int64)
    assert np.all(ptrs != T.LOCK_ENTRY), "LOCK_ENTRY left in the table"
    assert np.all(ptrs % T.SDF_BLOCK_VOXELS == 0)
    used_ids = ptrs // T.SDF_BLOCK_VOXELS
    assert len(np.unique(used_ids)) == len(used_ids), "two entries share one SDF block"
    state = np.zeros(n_blocks, dtype=np.int8)
    state[free_ids] += 1
    state[used_ids] += 2
    assert not np.any(state == 3), "ptr is on the free heap but also marked as an allocated entry"
    assert not np.any(state == 0), "memory leak: block neither free nor allocated"
    pos = hash_table["pos"][occ]
    if len(pos):
        assert len(np.unique(pos, axis=0)) == len(pos), "duplicate block positions in hash"
    # free entries are fully reset (deleteHashEntry, VoxelUtilHashSDF.h:365-369)
    free_e = hash_table[~occ]
    assert not free_e["offset"].any() and not free_e["pos"].any(), "free entry not reset"
    if sdf_blocks is not None and n_free:
        raw = sdf_blocks.view(np.uint64).reshape(n_blocks, T.SDF_BLOCK_VOXELS)
        assert not raw[free_ids].any(), "free SDF block is not cleared"
    chains = check_chains(hash_table, hp)
    return dict(num_occupied=int(occ.sum()), heap_free=n_free, **chains)


def hash_buckets(pos, num_buckets):
    """computeHashPos (VoxelUtilHashSDF.h:217-225) of [n,3] int positions: the int products wrap, the modulo is unsigned"""
    p = np.asarray(pos).astype(np.int64).reshape(-1, 3) & 0xFFFFFFFF
    h = ((p[:, 0] * 73856093) ^ (p[:, 1] * 19349669) ^ (p[:, 2] * 83492791)) & 0xFFFFFFFF
    return (h % int(num_buckets)).astype(np.int64)


def chain_of(hash_table, hp, bucket):
    """slots of the collision list that hangs off a bucket's last slot, in list order, as far as it can be followed
    (it stops in front of a link that leaves the table's rules: check_chains says which)"""
    ne = hp.m_hashNumBuckets * T.HASH_BUCKET_SIZE
    last = bucket * T.HASH_BUCKET_SIZE + T.HASH_BUCKET_SIZE - 1
    out, i = [], last
    while hash_table["offset"][i] != 0 and len(out) < ne:
        i = (last + int(hash_table["offset"][i])) % ne
        if i in out or i == last or hash_table["ptr"][i] == T.FREE_ENTRY:
            break
        out.append(i)
    return out


def check_chains(hash_table, hp):
    """The collision lists, which debugHash does not look at: every occupied entry is where
    getHashEntryForSDFBlockPos (VoxelUtilHashSDF.h:424-468) finds it -- in one of the ten slots of its home bucket, or
    on the list that starts at that bucket's last slot (an element's offset counts from the HOME bucket's last slot,
    :447, :601-606) within the walk's m_hashMaxCollisionLinkedListSize iterations, the first of which looks at the last
    slot itself -- and the lists are lists: a link leads to an occupied entry of the list's own bucket that is no
    bucket's last slot (allocBlock :585 skips those), no entry is on two lists or twice on one, and an offset sits
    only where a link can start.  -> dict(listed = entries on lists, longest = elements of the longest list,
    heads = buckets with a list)."""
    nb, bs = hp.m_hashNumBuckets, T.HASH_BUCKET_SIZE
    ne = nb * bs
    ptr, off = hash_table["ptr"], hash_table["offset"]
    slots = np.nonzero(ptr != T.FREE_ENTRY)[0]
    home_of = dict(zip(slots.tolist(), hash_buckets(hash_table["pos"][slots], nb).tolist()))  # occupied slot -> home bucket
    place = {}  # slot on a list -> (the list's bucket, its place on it: 1 = the element the last slot links to)
    heads = np.nonzero(off[bs - 1::bs])[0]
    longest = 0
    for b in heads.tolist():
        last = b * bs + bs - 1
        i, n = last, 0
        while off[i] != 0:
            j = (last + int(off[i])) % ne
            assert j in home_of, f"bucket {b}: the link of slot {i} (offset {off[i]}) lands on the free slot {j}"
            assert j % bs != bs - 1, f"bucket {b}: the link of slot {i} lands on slot {j}, the last slot of bucket {j // bs}"
            assert j not in place or place[j][0] != b, f"bucket {b}: its list comes back to slot {j}: a cycle"
            assert j not in place, f"slot {j} is on the lists of buckets {place.get(j, (0,))[0]} and {b}"
            assert home_of[j] == b, f"bucket {b}: the link of slot {i} lands on slot {j}, whose entry belongs to bucket {home_of[j]}"
            n += 1
            place[j] = (b, n)
            i = j
        longest = max(longest, n)
    for i in np.nonzero(off)[0].tolist():
        if i % bs == bs - 1 or i in place:
            continue
        assert home_of.get(i) != i // bs, f"slot {i}: an entry in its own bucket, not its last slot and on no list, has offset {off[i]}"
        assert False, f"slot {i}: offset {off[i]} on an entry that is neither a bucket's last slot nor on a list"
    # the walk: iteration 0 looks at the last slot, iteration k at the k-th element, k < m_hashMaxCollisionLinkedListSize
    homes = np.fromiter(home_of.values(), dtype=np.int64, count=len(home_of))
    lost = [i for i in slots[slots // bs != homes].tolist()
            if i not in place or place[i][0] != home_of[i] or place[i][1] >= hp.m_hashMaxCollisionLinkedListSize]
    assert not lost, (f"{len(lost)} entries are not found from their home bucket, first: slot {lost[0]} pos {hash_table['pos'][lost[0]]} "
                      f"home {home_of[lost[0]]} list and place {place.get(lost[0])}")
    return dict(listed=len(place), longest=int(longest), heads=int(len(heads)))


def check_bucket_summary(hash_table, bucket_count, bucket_bits, hp):
    """extension buffers: d_bucketCount[b] = occupied slots physically in
    bucket b; bit b of d_bucketBits = (count != 0)"""
    occ = hash_table["ptr"] != T.FREE_ENTRY
    want = np.bincount(np.nonzero(occ)[0] // T.HASH_BUCKET_SIZE, minlength=hp.m_hashNumBuckets).astype(np.uint32)
    assert np.array_equal(bucket_count, want), "d_bucketCount out of sync with d_hash"
    bits = np.unpackbits(bucket_bits.view(np.uint8), bitorder="little")[: hp.m_hashNumBuckets].astype(bool)
    assert np.array_equal(bits, want != 0), "d_bucketBits out of sync with d_bucketCount"


def assert_same_scene(a, b, what="", bucket_counts=True):
    """exact equality of two snapshots on the canonical forms.  bucket_counts=False: without the per-bucket occupancy --
    which neighbouring slot a collision-list element takes depends on the order in which concurrent allocs ran"""
    assert a["num_occupied"] == b["num_occupied"], f"{what}: occupied {a['num_occupied']} != {b['num_occupied']}"
    assert np.array_equal(a["positions"], b["positions"]), f"{what}: block position sets differ"
    assert a["heap_free"] == b["heap_free"], f"{what}: heap free {a['heap_free']} != {b['heap_free']}"
    if bucket_counts:
        assert np.array_equal(a["bucket_counts"], b["bucket_counts"]), f"{what}: per-bucket occupancy differs"
    if "voxels" in a and "voxels" in b:
        va, vb = a["voxels"], b["voxels"]
        assert np.array_equal(va["weight"], vb["weight"]), f"{what}: voxel weights differ"
        assert np.array_equal(va["color"], vb["color"]), f"{what}: voxel colours differ"
        assert np.array_equal(va["sdf"].view(np.uint32), vb["sdf"].view(np.uint32)), f"{what}: voxel sdf bits differ"


def compactified_set(entries):
    """sorted positions of a compactified entry list (its order is arbitrary)"""
    pos = np.ascontiguousarray(entries["pos"])
    return pos[lexsort_pos(pos)]
