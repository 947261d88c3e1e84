"""A numpy restatement of the indexed mesh ("Indexed mesh"): what welding a marching-cubes soup
by lattice edge has to give, written without the library -- its own key packing, its own table of the 12 edges.

A cell at voxel coordinates c has corner (bx, by, bz) on the lattice point L = c + (bx, by, bz).  An interpolated
vertex (snap code 0) is keyed by the lower end of its edge and the edge's axis; a snapped vertex (code 1 / 2:
vertexInterp returned its first / second end point) by that lattice point and code 3.  Of the soup vertices under one
key, the one from the cell with the lexicographically smallest (z, y, x) gives the welded vertex its bits (ties: the
first in the buffer; vertices of one cell under one key carry the same bits in a real extraction).

weld() returns the canonical form: vertices sorted by key, faces renumbered, each face rotated so that its smallest
index comes first (winding kept), faces sorted."""
import numpy as np

from voxelhashing_amd import vhtypes as T

# the end points of the 12 edges as (x, y, z) corner bits, read off the vertlist lines of the reference
# (DSC/MarchingCubesSDFUtil.h:217-228: vertlist[e] = vertexInterp(isolevel, p<xyz>, p<xyz>, ...))
EDGE_P1 = np.array([(0, 1, 0), (1, 1, 0), (1, 0, 0), (0, 0, 0), (0, 1, 1), (1, 1, 1), (1, 0, 1), (0, 0, 1),
                    (0, 1, 0), (1, 1, 0), (1, 0, 0), (0, 0, 0)], dtype=np.int64)
EDGE_P2 = np.array([(1, 1, 0), (1, 0, 0), (0, 0, 0), (0, 1, 0), (1, 1, 1), (1, 0, 1), (0, 0, 1), (0, 1, 1),
                    (0, 1, 1), (1, 1, 1), (1, 0, 1), (0, 0, 1)], dtype=np.int64)
BIAS = 1 << 19
POINT = 3  # the code of a lattice-point key


class KeyRange(ValueError):
    pass


def pack_key(cell, edge, snap):
    """-> the 64-bit key of one vertex, or None where it has none (bad edge / snap, lattice point out of range)"""
    if not (0 <= edge <= 11 and 0 <= snap <= 2):
        return None
    p1, p2 = EDGE_P1[edge], EDGE_P2[edge]
    if snap == 0:
        corner, code = np.minimum(p1, p2), int(np.argmax(p1 != p2))
    else:
        corner, code = (p1 if snap == 1 else p2), POINT
    L = np.asarray(cell, dtype=np.int64) + corner
    if np.any(L < -BIAS) or np.any(L >= BIAS):
        return None
    return int(L[0] + BIAS) | int(L[1] + BIAS) << 20 | int(L[2] + BIAS) << 40 | code << 60


def vertex_keys(sources):
    """keys of the 3 n soup vertices (uint64) and which of them are valid"""
    s = np.ascontiguousarray(sources, dtype=T.TRIANGLE_SOURCE_DTYPE).ravel()
    code8 = (s["edges"][:, None] >> (8 * np.arange(3, dtype=np.uint32))[None, :]) & 0xff
    edge, snap = (code8 & 0xf).astype(np.int64), ((code8 >> 4) & 3).astype(np.int64)
    ok = (edge <= 11) & (snap <= 2) & ((code8 >> 6) == 0)
    e = np.where(ok, edge, 0)
    p1, p2 = EDGE_P1[e], EDGE_P2[e]  # (n, 3, 3)
    corner = np.where((snap == 0)[..., None], np.minimum(p1, p2), np.where((snap == 1)[..., None], p1, p2))
    code = np.where(snap == 0, np.argmax(p1 != p2, axis=-1), POINT).astype(np.uint64)
    L = s["cell"].astype(np.int64)[:, None, :] + corner
    ok &= np.all((L >= -BIAS) & (L < BIAS), axis=-1)
    Lb = np.where(ok[..., None], L + BIAS, 0).astype(np.uint64)
    keys = Lb[..., 0] | (Lb[..., 1] << np.uint64(20)) | (Lb[..., 2] << np.uint64(40)) | (code << np.uint64(60))
    return keys.ravel(), ok.ravel()


def canonical_faces(faces):
    f = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
    if len(f) == 0:
        return f.astype(np.uint32)
    r = np.argmin(f, axis=1)
    f = np.stack([f[np.arange(len(f)), (r + k) % 3] for k in range(3)], axis=1)
    return f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))].astype(np.uint32)


def canonical(mesh):
    """a mesh as the library returns it (vertices, colors, keys, faces in any order) -> the canonical form"""
    order = np.argsort(mesh["keys"], kind="stable")
    new = np.empty(len(order), dtype=np.int64)
    new[order] = np.arange(len(order))
    faces = np.asarray(mesh["faces"], dtype=np.int64).reshape(-1, 3)
    return dict(vertices=np.ascontiguousarray(mesh["vertices"][order]), colors=np.ascontiguousarray(mesh["colors"][order]),
                keys=np.ascontiguousarray(mesh["keys"][order]), faces=canonical_faces(new[faces]))


def weld(soup, sources):
    soup = np.ascontiguousarray(soup, dtype=T.TRIANGLE_DTYPE).ravel()
    sources = np.ascontiguousarray(sources, dtype=T.TRIANGLE_SOURCE_DTYPE).ravel()
    assert len(soup) == len(sources)
    keys, ok = vertex_keys(sources)
    if not np.all(ok):
        raise KeyRange("a vertex has no key")
    p, c = soup["v"]["p"].reshape(-1, 3), soup["v"]["c"].reshape(-1, 3)
    cell = np.repeat(sources["cell"].astype(np.int64), 3, axis=0)
    idx = np.arange(len(keys))
    order = np.lexsort((idx, cell[:, 0], cell[:, 1], cell[:, 2], keys))  # by key, then (z, y, x), then buffer order
    sk = keys[order]
    first = np.ones(len(sk), dtype=bool)
    first[1:] = sk[1:] != sk[:-1]
    winners = order[first]            # one soup vertex per key, keys ascending
    ukeys = sk[first]
    of_vertex = np.searchsorted(ukeys, keys)
    faces = of_vertex.reshape(-1, 3)
    keep = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    return dict(vertices=np.ascontiguousarray(p[winners]), colors=np.ascontiguousarray(c[winners]), keys=ukeys.astype(np.uint64),
                faces=canonical_faces(faces[keep]), dropped_faces=int((~keep).sum()))


def same_mesh(a, b):
    """bit for bit: vertices, colours, keys and faces of two canonical meshes"""
    return all(a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in ("vertices", "colors", "keys", "faces"))


def properties(mesh, soup, sources):
    """of a canonical mesh: faces with a repeated index, faces over a vertex set that an earlier face has, the largest
    number of faces on one undirected edge, and the largest distance from a soup vertex to the vertex it was welded to"""
    f = mesh["faces"].astype(np.int64)
    repeated = int(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).sum())
    duplicates = len(f) - len(np.unique(np.sort(f, axis=1), axis=0)) if len(f) else 0
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    per_edge = int(np.unique(e, axis=0, return_counts=True)[1].max()) if len(e) else 0
    keys, _ = vertex_keys(sources)
    at = np.searchsorted(mesh["keys"], keys)
    assert np.array_equal(mesh["keys"][at], keys), "a soup vertex whose key the mesh does not have"
    p = np.ascontiguousarray(soup, dtype=T.TRIANGLE_DTYPE).ravel()["v"]["p"].reshape(-1, 3).astype(np.float64)
    spread = float(np.linalg.norm(p - mesh["vertices"][at].astype(np.float64), axis=1).max()) if len(p) else 0.0
    snapped = int(((mesh["keys"] >> np.uint64(60)) == POINT).sum())
    return dict(repeated=repeated, duplicates=duplicates, faces_per_edge=per_edge, spread=spread, snapped_vertices=snapped)


def assert_sources_name_their_edges(tris, srcs, voxel_size):
    """every vertex of a sourced extraction against the end points of the edge its record names, recomputed in float32
    the way the kernel does: worldPos = float(cell) * voxelSize, corner = worldPos +- voxelSize / 2
    -> the snap codes (n, 3)"""
    vs = np.float32(voxel_size)
    P = vs / np.float32(2.0)
    world = srcs["cell"].astype(np.float32) * vs  # (n, 3)
    code8 = (srcs["edges"][:, None] >> (8 * np.arange(3, dtype=np.uint32))[None, :]) & 0xff
    edge, snap = (code8 & 0xf).astype(np.int64), (code8 >> 4).astype(np.int64)
    assert edge.max() <= 11 and snap.max() <= 2
    p1 = world[:, None, :] + np.where(EDGE_P1[edge] == 1, P, -P).astype(np.float32)
    p2 = world[:, None, :] + np.where(EDGE_P2[edge] == 1, P, -P).astype(np.float32)
    assert p1.dtype == np.float32
    pos = tris["v"]["p"]  # (n, 3, 3)
    on_axis = EDGE_P1[edge] != EDGE_P2[edge]
    assert np.all(on_axis.sum(axis=-1) == 1)
    b = lambda a: np.ascontiguousarray(a).view(np.uint32)
    assert np.array_equal(b(pos)[~on_axis], b(p1)[~on_axis]) and np.array_equal(b(pos)[~on_axis], b(p2)[~on_axis])
    lo, hi = np.minimum(p1, p2)[on_axis], np.maximum(p1, p2)[on_axis]
    assert np.all((pos[on_axis] >= lo) & (pos[on_axis] <= hi))
    at1, at2 = np.all(b(pos) == b(p1), axis=-1), np.all(b(pos) == b(p2), axis=-1)
    assert np.array_equal(snap == 1, at1) and np.array_equal(snap == 2, at2)
    return snap


# ---------------------------------------------------------------------------- hand-made input

def source_record(cell, codes):
    """codes: three (edge, snap)"""
    s = np.zeros(1, dtype=T.TRIANGLE_SOURCE_DTYPE)
    s["cell"] = cell
    s["edges"] = sum((e | sn << 4) << (8 * k) for k, (e, sn) in enumerate(codes))
    return s


def make_soup(tris):
    """tris: a list of (cell, [(edge, snap, position, colour)] * 3) -> soup, sources"""
    soup = np.zeros(len(tris), dtype=T.TRIANGLE_DTYPE)
    srcs = np.zeros(len(tris), dtype=T.TRIANGLE_SOURCE_DTYPE)
    for i, (cell, verts) in enumerate(tris):
        srcs[i] = source_record(cell, [(e, sn) for e, sn, _, _ in verts])[0]
        for k, (_, _, p, c) in enumerate(verts):
            soup["v"]["p"][i, k] = p
            soup["v"]["c"][i, k] = c
    return soup, srcs


def random_soup(n, seed, spread=3, isolated=False):
    """n triangles over three distinct edges each; cells drawn from a cube of `spread` cells a side (so keys are
    shared across cells), or one cell per triangle two cells apart (isolated: 3 n distinct keys); random bits for
    positions and colours; about one vertex in eight snapped"""
    rng = np.random.default_rng(seed)
    soup = np.zeros(n, dtype=T.TRIANGLE_DTYPE)
    srcs = np.zeros(n, dtype=T.TRIANGLE_SOURCE_DTYPE)
    soup["v"]["p"] = rng.standard_normal((n, 3, 3)).astype(np.float32)
    soup["v"]["c"] = rng.random((n, 3, 3)).astype(np.float32)
    for i in range(n):
        if isolated:
            srcs["cell"][i] = (2 * i - n, 5, -7)
            codes = [(0, 0), (3, 0), (8, 0)]
        else:
            srcs["cell"][i] = rng.integers(-spread, spread, 3)
            codes = [(int(e), int(rng.choice([0, 0, 0, 0, 0, 0, 1, 2]))) for e in rng.choice(12, 3, replace=False)]
        srcs["edges"][i] = sum((e | sn << 4) << (8 * k) for k, (e, sn) in enumerate(codes))
    return soup, srcs


def hand_made_cases():
    """name -> (soup, sources, expected vertex count, expected face count): the cases of the issue"""
    red, blue, grey = (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.5, 0.5, 0.5)
    out = {}
    # two cells share the x edge through lattice point (0, 1, 1): edge 0 of cell (0,0,1) is edge 4 of cell (0,0,0);
    # the lower cell (z first) gives the bits
    a = ((0, 0, 1), [(0, 0, (0.31, 0.5, 0.5), red), (3, 0, (0.0, 0.2, 0.5), red), (8, 0, (0.0, 0.5, 0.8), red)])
    b = ((0, 0, 0), [(4, 0, (0.30, 0.5, 0.5), blue), (5, 0, (1.0, 0.2, 0.4), blue), (8, 0, (0.0, 0.5, 0.3), blue)])
    out["shared_edge"] = make_soup([a, b]) + (5, 2)
    # snapped vertices from different edges and cells meet at lattice point (1, 1, 1): one vertex
    c = ((0, 0, 0), [(5, 1, (0.5, 0.5, 0.5), red), (6, 0, (0.2, 0.0, 0.5), red), (10, 0, (0.5, 0.0, 0.2), red)])
    d = ((1, 1, 1), [(3, 1, (0.5, 0.5, 0.5), blue), (2, 0, (0.9, 0.5, 0.5), blue), (11, 0, (0.5, 0.5, 0.9), blue)])
    e = ((0, 1, 0), [(10, 2, (0.5, 0.5, 0.5), grey), (1, 0, (0.5, 1.3, 0.0), grey), (0, 0, (0.4, 1.5, 0.0), grey)])
    out["snapped_meet"] = make_soup([c, d, e]) + (7, 3)
    # a snap disagreement: cell (0,0,0) snapped its edge 4 to the first end point, cell (0,0,1) interpolated the same
    # lattice edge: two vertices
    f = ((0, 0, 0), [(4, 1, (0.0, 0.5, 0.5), red), (5, 0, (1.0, 0.2, 0.4), red), (8, 0, (0.0, 0.5, 0.3), red)])
    g = ((0, 0, 1), [(0, 0, (0.00001, 0.5, 0.5), blue), (3, 0, (0.0, 0.2, 0.5), blue), (8, 0, (0.0, 0.5, 0.8), blue)])
    out["snap_disagreement"] = make_soup([f, g]) + (6, 2)
    # a face that collapses: edges 0 and 3 both snapped onto corner (0, 1, 0) -> a repeated index, dropped
    h = ((2, 2, 2), [(0, 1, (2.0, 2.5, 2.0), grey), (3, 2, (2.0, 2.5, 2.0), grey), (8, 0, (2.0, 2.5, 2.3), grey)])
    k = ((2, 2, 2), [(0, 0, (2.3, 2.5, 2.0), grey), (1, 0, (2.5, 2.3, 2.0), grey), (9, 0, (2.5, 2.5, 2.3), grey)])
    out["collapsing_face"] = make_soup([h, k]) + (5, 1)
    return out
