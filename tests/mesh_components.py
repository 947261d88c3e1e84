"""A numpy restatement of the component pass of the indexed mesh ("Mesh components"), written
without the library and deliberately not as a union-find: labels are spread over the faces until nothing changes.

Order of vertices: a comes before b when (key[a], a) < (key[b], b).  Two vertices are joined when a face names both.
A face with an index >= V sets BAD_INDEX, joins nothing and counts nowhere; a face with a repeated index joins its
distinct vertices and counts as one face.  A component's root is its first vertex; root[v] is the root's index (a
vertex without a face is its own root); face_count[r] is the number of in-range faces whose first index lies in r's
component, 0 at vertices that are no root.

filter(): a component is kept when face_count >= min_faces; with largest_only it must also be THE largest (the greatest
face_count; among equals the root that comes first; with no face at all nothing).  The output is the kept vertices with
keys (and normals), and the kept faces renumbered, winding and rotation left alone, in mesh_weld.canonical form.
Counts: components with a face, faceless vertices, kept components (with a face), kept vertices, kept faces, faces of
the largest component.  A status keeps nothing and all counts read 0."""
import numpy as np

import mesh_weld as MW

BAD_INDEX, STEPS = 1, 2
COUNTS = ("components", "faceless_vertices", "kept_components", "kept_vertices", "kept_faces", "largest_faces")


def vertex_order(keys):
    """-> order (the vertices, first to last) and rank (the place of each vertex)"""
    k = np.ascontiguousarray(keys, dtype=np.uint64).ravel()
    order = np.lexsort((np.arange(len(k)), k))
    rank = np.empty(len(k), dtype=np.int64)
    rank[order] = np.arange(len(k))
    return order, rank


def components(keys, faces):
    """-> root (V,) u32, face_count (V,) u32, status"""
    k = np.ascontiguousarray(keys, dtype=np.uint64).ravel()
    f = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
    V = len(k)
    ok = np.all((f >= 0) & (f < V), axis=1)
    status = 0 if np.all(ok) else BAD_INDEX
    g = f[ok]
    order, rank = vertex_order(k)
    label = rank.copy()  # the smallest place known in the vertex's component
    while True:
        new = label.copy()
        if len(g):
            np.minimum.at(new, g.ravel(), np.repeat(new[g].min(axis=1), 3))  # every face spreads its smallest label
        new = new[order[new]]  # pointer jump: the vertex at that place may know a smaller one
        if np.array_equal(new, label):
            break
        label = new
    root = order[label] if V else np.zeros(0, dtype=np.int64)
    count = np.bincount(root[g[:, 0]], minlength=V) if len(g) else np.zeros(V, dtype=np.int64)
    return root.astype(np.uint32), count.astype(np.uint32), status


def canonical(mesh):
    """MW.canonical, with the normals (if any) in the same order"""
    out = MW.canonical(mesh)
    if "normals" in mesh:
        out["normals"] = np.ascontiguousarray(np.asarray(mesh["normals"])[np.argsort(mesh["keys"], kind="stable")])
    return out


def filter(mesh, min_faces=0, largest_only=False):
    """mesh: vertices (V,3), colors (V,3), keys (V,), faces (F,3), optionally normals (V,3) -> dict(mesh=the canonical
    filtered mesh, counts=the six by name, root, face_count, status)"""
    k = np.ascontiguousarray(mesh["keys"], dtype=np.uint64).ravel()
    f = np.ascontiguousarray(mesh["faces"], dtype=np.int64).reshape(-1, 3)
    V = len(k)
    root, count, status = components(k, f)
    _, rank = vertex_order(k)
    is_root = root == np.arange(V)
    keep_root = np.zeros(V, dtype=bool)
    counts = dict.fromkeys(COUNTS, 0)
    if status == 0:
        keep_root = is_root & (count >= min_faces)
        largest = int(count.max()) if V else 0
        if largest_only:
            tied = np.flatnonzero(is_root & (count == largest)) if largest > 0 else np.zeros(0, dtype=np.int64)
            best = np.zeros(V, dtype=bool)
            if len(tied):
                best[tied[np.argmin(rank[tied])]] = True
            keep_root &= best
        counts = dict(components=int((is_root & (count > 0)).sum()), faceless_vertices=int((is_root & (count == 0)).sum()),
                      kept_components=int((keep_root & (count > 0)).sum()), largest_faces=largest)
    keep_v = keep_root[root] if V else np.zeros(0, dtype=bool)
    in_range = np.all((f >= 0) & (f < V), axis=1)
    keep_f = in_range & (status == 0)
    keep_f[keep_f] = keep_v[f[keep_f, 0]]
    new = np.cumsum(keep_v) - 1
    out = dict(vertices=np.asarray(mesh["vertices"])[keep_v], colors=np.asarray(mesh["colors"])[keep_v], keys=k[keep_v], faces=new[f[keep_f]].astype(np.uint32).reshape(-1, 3))
    if "normals" in mesh:
        out["normals"] = np.asarray(mesh["normals"])[keep_v]
    counts.update(kept_vertices=int(keep_v.sum()), kept_faces=int(keep_f.sum()))
    return dict(mesh=canonical(out), counts={n: counts[n] for n in COUNTS}, root=root, face_count=count, status=status)


def root_keys(keys, root):
    """the key of every vertex's root: what two labellings of one mesh under different vertex numbers agree on"""
    return np.ascontiguousarray(keys, dtype=np.uint64).ravel()[np.asarray(root, dtype=np.int64)]


def sizes(face_count):
    """the face counts of the components with a face, largest first"""
    c = np.asarray(face_count)
    return np.sort(c[c > 0])[::-1]


# ---------------------------------------------------------------------------- hand-made meshes

def plain_mesh(keys, faces, seed=0):
    """keys and faces with random positions and colours"""
    rng = np.random.default_rng(seed)
    k = np.ascontiguousarray(keys, dtype=np.uint64).ravel()
    return dict(vertices=rng.standard_normal((len(k), 3)).astype(np.float32), colors=rng.random((len(k), 3)).astype(np.float32), keys=k,
                faces=np.ascontiguousarray(faces, dtype=np.uint32).reshape(-1, 3))


def strip(n, how, seed=0):
    """a strip of n triangles (i, i + 1, i + 2) over n + 2 vertices whose keys ascend, descend or are shuffled along it"""
    keys = np.arange(100, 100 + n + 2, dtype=np.uint64) * np.uint64(7)
    if how == "descending":
        keys = keys[::-1]
    elif how == "shuffled":
        keys = np.random.default_rng(seed).permutation(keys)
    else:
        assert how == "ascending"
    i = np.arange(n, dtype=np.uint32)
    return plain_mesh(keys, np.stack([i, i + 1, i + 2], axis=1), seed)


def fan(n, seed=0):
    """n faces (hub, i, i + 1) round one hub whose key is in the middle of the others"""
    keys = np.random.default_rng(seed).permutation(np.arange(1, n + 3, dtype=np.uint64) * np.uint64(3))
    i = np.arange(1, n + 1, dtype=np.uint32)
    return plain_mesh(keys, np.stack([np.zeros(n, dtype=np.uint32), i, i + 1], axis=1), seed)


def archipelago(sizes_=(1, 2, 5, 22, 64, 257), seed=40):
    """soups of those many triangles in cubes of 4 cells a side (so that the large ones hang together), the cells of each
    shifted 10 further in x so that no two share a key -> soup, sources"""
    soups, srcs = [], []
    for j, n in enumerate(sizes_):
        s, r = MW.random_soup(n, seed + j, spread=2)
        r = r.copy()
        r["cell"][:, 0] += 10 * j
        soups.append(s)
        srcs.append(r)
    return np.concatenate(soups), np.concatenate(srcs)
