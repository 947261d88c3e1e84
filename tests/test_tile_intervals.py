"""The models of tests/tile_intervals.py against each other, without a GPU: the float64 ray/box reference on hand cases,
the float32 restatement of the splat's rule as a superset of it on every view the GPU test uses, the mutation table of
DESIGN.md section 2 (what the reference would catch if the rule were narrower), and the properties of the deal."""
import numpy as np
import pytest

import tile_intervals as TI

F = np.float32


# ------------------------------------------------------------------------------------------------ needed_pairs by hand

def one_ray(blocks, eye_x, gradients, vs=1.0, min_depth=0.5, max_depth=100.0):
    """a 1x1 image whose only ray runs from (eye_x, 0.5, 0) along +z (mx = my = 0: the ray is the optical axis)"""
    pose = np.eye(4)
    pose[:3, 3] = (eye_x, 0.5, 0.0)
    need, zlo, zhi = TI.needed_pairs(np.array(blocks), vs, pose, (10.0, 10.0, 0.0, 0.0), 1, 1, min_depth, max_depth, gradients)
    return need[0], zlo[0], zhi[0]


def test_needed_pairs_one_block_dead_ahead():
    """16x16 pixels (four tiles), focal length 10, the optical axis through pixel (8, 8): block (0, 0, 3) of 4 cm voxels
    reaches x, y in [-0.04, 0.32) and z in [0.92, 1.28), so only rays with x, y >= 8 - 0.3125 meet it: the fourth tile"""
    need, zlo, zhi = TI.needed_pairs(np.array([[0, 0, 3]]), 0.04, np.eye(4), (10.0, 10.0, 8.0, 8.0), 16, 16, 0.5, 5.0, False)
    assert need[:, 0].tolist() == [False, False, False, True]
    assert zlo[3, 0] == pytest.approx(0.92, abs=1e-5) and zhi[3, 0] == pytest.approx(1.28, abs=1e-5)
    assert np.isinf(zlo[:3, 0]).all()
    # with gradients the box is half a voxel larger: the axis ray is in it from 0.90 to 1.30
    need, zlo, zhi = TI.needed_pairs(np.array([[0, 0, 3]]), 0.04, np.eye(4), (10.0, 10.0, 8.0, 8.0), 16, 16, 0.5, 5.0, True)
    assert need[:, 0].tolist() == [False, False, False, True]
    assert zlo[3, 0] == pytest.approx(0.90, abs=1e-5) and zhi[3, 0] == pytest.approx(1.30, abs=1e-5)


@pytest.mark.parametrize("eye_x,plain,with_gradients", [
    (7.3, True, True),     # in the last voxel of reach below the block (8b - 1 = 7 .. 8)
    (6.7, False, True),    # in the half voxel the gradient adds
    (6.3, False, False),
    (15.9, True, True),    # the last voxel of the block itself: reach ends at 8b + 8 = 16
    (16.3, False, True),
    (16.7, False, False),
])
def test_needed_pairs_grazing_ray(eye_x, plain, with_gradients):
    """block (1, 0, 3) of unit voxels reaches x in [7, 16) ([6.5, 16.5) with gradients); a ray parallel to its faces"""
    assert one_ray([[1, 0, 3]], eye_x, False)[0][0] == plain
    assert one_ray([[1, 0, 3]], eye_x, True)[0][0] == with_gradients
    if plain:
        _, zlo, zhi = one_ray([[1, 0, 3]], eye_x, False)
        assert zlo[0] == pytest.approx(23.0, abs=1e-3) and zhi[0] == pytest.approx(32.0, abs=1e-3)


def test_needed_pairs_behind_and_beyond():
    blocks = [[1, 0, -3], [1, 0, 3], [1, 0, 0]]
    need, zlo, zhi = one_ray(blocks, 9.0, False, max_depth=20.0)
    assert need.tolist() == [False, False, True], "a block behind the camera, one beyond the far limit, one across the near limit"
    assert zlo[2] == 0.5 and zhi[2] == pytest.approx(8.0, abs=1e-3), "the range is cut at the near limit"
    need, _, zhi = one_ray(blocks, 9.0, False, max_depth=25.0)
    assert need.tolist() == [False, True, True] and zhi[1] == 25.0


# ------------------------------------------------------------------------------------------------ the model on the scenes

@pytest.fixture(scope="module")
def blocks(oracle_lib):
    return {name: TI.oracle_blocks(oracle_lib, name) for name in TI.TABLES}


@pytest.fixture(scope="module")
def cases(blocks):
    """per (view, gradients): the view, its blocks, what the rays need and what the rule lists; computed once"""
    out = {}
    for name, (table, *_rest) in TI.VIEWS.items():
        view = TI.View(name, TI.table_frames(table)[0])
        for g in (False, True):
            out[name, g] = dict(view=view, blocks=blocks[table], need=TI.needed_for(view, blocks[table], g), model=TI.model_for(view, blocks[table], g))
    return out


@pytest.mark.parametrize("gradients", [False, True])
@pytest.mark.parametrize("name", list(TI.VIEWS))
def test_the_rule_lists_every_needed_pair(cases, name, gradients):
    c = cases[name, gradients]
    (need, zlo, zhi), m = c["need"], c["model"]
    assert need.sum() > 500, "the view was meant to need many blocks"
    missing = np.argwhere(need & ~m["listed"])
    assert len(missing) == 0, f"{len(missing)} needed (tile, block) pairs are not listed, first: tile {missing[0][0]}, block {c['blocks'][missing[0][1]]}"
    # the block's depth range holds the depths at which the tile's rays are in its reach
    lo, hi = m["lo"].view(F).astype(np.float64), m["hi"].view(F).astype(np.float64)
    t, b = np.nonzero(need)
    assert (lo[b] <= zlo[t, b]).all() and (hi[b] >= zhi[t, b]).all()
    print(f"{name} gradients={gradients}: {int(need.sum())} needed, {int(m['listed'].sum())} listed, ratio {m['listed'].sum() / need.sum():.2f}")


def test_the_scenes_are_what_they_were_chosen_for(cases):
    c = cases["close_8cm", False]
    nearest = c["need"][1][c["need"][0]].min()
    assert c["view"].intrinsics()[0] * c["view"].vs / nearest >= 8.0, "a voxel of the nearest needed block spans at least 8 pixels"
    for g in (False, True):
        count = cases["fine_1cm", g]["model"]["count"]
        for cap in (TI.CAP_SMALL, TI.CAP_LARGE):
            assert (count == 0).any() and ((count > 0) & (count <= cap)).any() and (count > cap).any(), f"capacity {cap}: not all three count cases"
        m = cases["inside_4cm", g]["model"]
        assert m["every_tile"].sum() > 10 and (m["rect"][:, 2] < 0).sum() > 10, "blocks across z = 0.05 and blocks behind the camera"
        r = cases["tilted_8cm", g]["model"]["rect"]
        v = cases["tilted_8cm", g]["view"]
        partly = (r[:, 2] >= r[:, 0]) & ((r[:, 0] == 0) | (r[:, 1] == 0) | (r[:, 2] == v.tiles_x - 1) | (r[:, 3] == v.tiles_y - 1))
        assert partly.sum() > 10, "blocks that straddle the image border"
    assert cases["ragged_2cm", False]["view"].W % 8 and cases["ragged_2cm", False]["view"].H % 8


# "slop removed" can lose no needed pair: a perspective projection maps a box in front of the camera into the hull of
# its projected corners, so the rule without the slop is still a superset in exact arithmetic; the slop (at least one
# pixel) only guards the float32 roundings of the projection, which are far smaller than the quarter voxel of margin.
NOT_CAUGHT = {"slop removed"}


def mutation_table(cases):
    """{mutation: {view: needed pairs lost with / without gradients}}"""
    table = {}
    for (name, g), c in cases.items():
        for mutation, change in TI.mutations(g).items():
            if mutation.startswith("no-gradient") and not g:
                continue
            lost = int((c["need"][0] & ~TI.model_for(c["view"], c["blocks"], g, **change)["listed"]).sum())
            table.setdefault(mutation, {}).setdefault(name, {})[g] = lost
    return table


def test_mutations_of_the_rule_lose_needed_pairs(cases):
    """every narrower rule must lose a needed pair in some view, or the reference could not tell it from the right one"""
    table = mutation_table(cases)
    views = list(TI.VIEWS)
    print("\n| mutation | " + " | ".join(views) + " |")
    print("|---|" + "---|" * len(views))
    for mutation, row in table.items():
        print(f"| {mutation} | " + " | ".join(" / ".join(str(row[v][g]) for g in (False, True) if g in row[v]) for v in views) + " |")
    caught = {m for m, row in table.items() if any(n > 0 for per in row.values() for n in per.values())}
    assert set(table) - caught == NOT_CAUGHT, f"caught: {sorted(caught)}"


# ------------------------------------------------------------------------------------------------ the deal

def turns(n_share):
    """the order in which the shares' ranks are dealt, told literally: round after round, a share that has run out is skipped"""
    order = []
    for mine in range(max(n_share)):
        order += [(w, mine) for w in range(len(n_share)) if mine < n_share[w]]
    return order


@pytest.mark.parametrize("num_cus", [256, 37])
@pytest.mark.parametrize("n_tiles", [300, 1023, 1024, 1056, 1073])
def test_schedule_model_properties(n_tiles, num_cus):
    n_split = TI.split_tiles(n_tiles)
    assert n_split == {300: 0, 1023: 0, 1024: 64, 1056: 66, 1073: 66}[n_tiles]
    parts = TI.sched_parts(n_tiles)
    for pattern, classes in TI.class_patterns(n_tiles, n_tiles + num_cus).items():
        what = f"{n_tiles} tiles, {num_cus} CUs, {pattern}"
        s = TI.schedule_model(classes, n_tiles, num_cus, n_split)
        assert s["writes"].max() == 1, f"{what}: a slot written twice"
        assert (s["tile"] >= 0).sum() == n_tiles + n_split
        TI.check_deal(s["tile"], s["half"], n_tiles, n_split, what)
        # the pairs are the first ranks, in slot order
        paired = s["half"] != 0
        assert sorted(set(s["rank"][paired].tolist())) == list(range(n_split)), f"{what}: the split tiles are not ranks 0 .. {n_split - 1}"
        assert (s["rank"][~paired & (s["tile"] >= 0)] >= n_split).all()
        clamped = np.minimum(classes, 31)
        assert np.array_equal(s["cls"][s["tile"] >= 0], clamped[s["tile"][s["tile"] >= 0]])
        # classes do not increase along a share, and the shares take turns
        used = np.nonzero((s["tile"] >= 0) & (s["half"] != 2))[0]
        by_rank = used[np.argsort(s["rank"][used])]
        assert np.array_equal(s["rank"][by_rank], np.arange(n_tiles))
        n_share = [int((TI.share_of(np.arange(n_tiles), n_tiles) == w).sum()) for w in range(parts)]
        assert s["share"][by_rank].tolist() == [w for w, _ in turns(n_share)], f"{what}: the shares do not take turns"
        assert np.array_equal(TI.share_of(s["tile"][by_rank], n_tiles), s["share"][by_rank])
        for w in range(parts):
            along = s["cls"][by_rank][s["share"][by_rank] == w]
            assert (np.diff(along) <= 0).all(), f"{what}: share {w} is not sorted dearest first"
        if parts == 1:  # one share: the whole image dearest first
            assert (np.diff(s["cls"][by_rank]) <= 0).all()
