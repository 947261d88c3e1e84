"""A numpy restatement of the accumulating weld ("Indexed mesh over several extractions"), on top
of the restatement of the one-shot weld (tests/mesh_weld.py), which it leaves as it is.

parts is a sequence of (soup, records), one per append.  A cell belongs to the first append it occurs in; every
triangle of it in a later append is dropped.  What the accumulation has to give is the one-shot weld of the kept
triangles concatenated in append order."""
import numpy as np

import mesh_weld as MW
from voxelhashing_amd import vhtypes as T


def _arrays(parts):
    return [(np.ascontiguousarray(s, dtype=T.TRIANGLE_DTYPE).ravel(), np.ascontiguousarray(r, dtype=T.TRIANGLE_SOURCE_DTYPE).ravel())
            for s, r in parts]


def kept(parts):
    """-> [(soup, records)] per append: the triangles whose cell occurs in no earlier append"""
    seen, out = set(), []
    for soup, srcs in _arrays(parts):
        cells = [tuple(int(v) for v in c) for c in srcs["cell"]]
        keep = np.array([c not in seen for c in cells], dtype=bool)
        seen.update(cells)
        out.append((soup[keep], srcs[keep]))
    return out


def dropped(parts):
    """the number of triangles that kept() leaves out"""
    return sum(len(s) for s, _ in _arrays(parts)) - sum(len(s) for s, _ in kept(parts))


def concatenate(parts):
    parts = _arrays(parts)
    if not parts:
        return np.zeros(0, dtype=T.TRIANGLE_DTYPE), np.zeros(0, dtype=T.TRIANGLE_SOURCE_DTYPE)
    return np.concatenate([s for s, _ in parts]), np.concatenate([r for _, r in parts])


def weld_appends(parts):
    """the canonical mesh of the accumulation (as mesh_weld.weld)"""
    return MW.weld(*concatenate(kept(parts)))


def num_cells(parts):
    _, srcs = concatenate(parts)
    return len(np.unique(srcs["cell"], axis=0)) if len(srcs) else 0


# ---------------------------------------------------------------------------- input

def split_cases():
    """name -> parts: the hand-made soups of mesh_weld.hand_made_cases() split over appends"""
    cases = MW.hand_made_cases()
    out = {}
    # the winning cell (0, 0, 0) -- the smaller (z, y, x) -- comes in the SECOND append: the vertex on the shared edge,
    # numbered by the first append, has to take the second one's bits
    soup, srcs, _, _ = cases["shared_edge"]
    out["shared_edge"] = [(soup[:1], srcs[:1]), (soup[1:], srcs[1:])]
    soup, srcs, _, _ = cases["snapped_meet"]
    out["snapped_meet"] = [(soup[i:i + 1], srcs[i:i + 1]) for i in range(3)]
    # the same, the winning cell (0, 0, 0) last
    out["snapped_meet_reversed"] = [(soup[i:i + 1], srcs[i:i + 1]) for i in (2, 1, 0)]
    # cell (2, 2, 2) comes back in a later append with DIFFERENT triangles, over edges nobody else has: they vanish,
    # keys and all
    soup, srcs, _, _ = cases["collapsing_face"]
    grey = (0.5, 0.5, 0.5)
    late, late_srcs = MW.make_soup([
        ((2, 2, 2), [(4, 0, (2.3, 2.5, 3.0), grey), (5, 0, (3.0, 2.3, 3.0), grey), (6, 0, (2.6, 2.0, 3.0), grey)]),
        ((3, 2, 2), [(0, 0, (3.3, 2.5, 2.0), grey), (3, 0, (3.0, 2.2, 2.0), grey), (11, 0, (3.0, 2.0, 2.4), grey)])])
    out["repeated_cell"] = [(soup, srcs), (late, late_srcs)]
    return out


def by_cell(soup, srcs):
    """-> the groups of triangle indices that share a cell, buffer order kept inside a group, groups in order of their
    first triangle"""
    _, first, inv = np.unique(srcs["cell"], axis=0, return_index=True, return_inverse=True)
    inv = np.asarray(inv).ravel()
    order = np.argsort(first, kind="stable")
    return [np.flatnonzero(inv == g) for g in order]


def deal(soup, srcs, num_parts, seed, repeat=1.0 / 3.0, identical=True):
    """a soup dealt into num_parts appends cell by cell (round robin); about `repeat` of the cells come back WHOLE in a
    later append -- as bit-identical copies, or (identical=False) with other positions and colours"""
    rng = np.random.default_rng(seed)
    groups = by_cell(soup, srcs)
    idx = [[] for _ in range(num_parts)]
    again = [[] for _ in range(num_parts)]
    for g, tris in enumerate(groups):
        p = g % num_parts
        idx[p].append(tris)
        if p + 1 < num_parts and rng.random() < repeat * num_parts / (num_parts - 1):
            again[int(rng.integers(p + 1, num_parts))].append(tris)
    parts = []
    for p in range(num_parts):
        own = np.concatenate(idx[p]) if idx[p] else np.zeros(0, dtype=np.int64)
        rep = np.concatenate(again[p]) if again[p] else np.zeros(0, dtype=np.int64)
        # the repeats first, so that they do not sit at the end of their append; the order inside a cell stays the
        # soup's, which decides ties between two vertices of one cell under one key
        s, r = np.concatenate([soup[rep], soup[own]]), np.concatenate([srcs[rep], srcs[own]])
        if not identical and len(rep):
            s["v"]["p"][:len(rep)] += np.float32(0.25)
            s["v"]["c"][:len(rep)] *= np.float32(0.5)
        parts.append((s, r))
    return parts
