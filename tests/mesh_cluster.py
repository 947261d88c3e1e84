"""A numpy restatement of the vertex clustering ("Mesh clustering"): what decimating a welded mesh
by clusters of m lattice points a side has to give, written without the library and without a hash table -- sorting and
np.unique do the grouping, int64 arrays the sums.

A vertex key holds a lattice point L (three 20-bit components biased by 2^19; bits 60-61 are a code that does not
matter here; bit 62 or 63 set: no vertex key).  Its cluster is k = floor(L / m) per component, named by k packed like a
lattice point with code 3.  A cluster's vertex is the integer mean floor((2 sum + n) / (2 n)) of q = rint(p * 2^scale)
over ALL its vertices (colours: scale 16), as float32((float64) mean * 2^-scale).  A face with two corners in one
cluster is dropped (collapsed); of the faces over one set of three clusters one is kept (the others: duplicates): with
the smallest cluster key rotated to the front, the one whose second key is the smaller if both windings occur.  A
cluster that no kept face names gives no vertex (unused).

cluster() returns the mesh in mesh_weld.canonical form."""
import numpy as np

import mesh_weld as MW

TABLE_FULL, BAD_KEY, RANGE, BAD_INDEX = 1, 2, 4, 8
MAX_CELLS = 64
COUNTS = ("vertices", "faces", "status", "collapsed", "duplicates", "unused_clusters")
BIAS = 1 << 19
LIMIT = float(1 << 40)


def lattice(keys):
    """(V, 3) int64 lattice points of vertex keys"""
    k = np.asarray(keys, dtype=np.uint64)
    return np.stack([((k >> np.uint64(20 * a)) & np.uint64(0xfffff)).astype(np.int64) - BIAS for a in range(3)], axis=1)


def pack_point(L, code=3):
    L = np.asarray(L, dtype=np.int64)
    b = (L + BIAS).astype(np.uint64)
    return b[..., 0] | (b[..., 1] << np.uint64(20)) | (b[..., 2] << np.uint64(40)) | (np.uint64(code) << np.uint64(60))


def cluster_key(key, m):
    """the cluster key of one vertex key, or None for a key that is none"""
    if int(key) >> 62:
        return None
    return int(pack_point(np.floor_divide(lattice(np.array([key], dtype=np.uint64)), m))[0])


def default_scale_log2(voxel_size):
    """16 - floor(log2(voxel_size))"""
    v = np.float32(voxel_size)
    if not (np.isfinite(v) and v > 0):
        raise ValueError("voxel size")
    mant, e = np.frexp(np.float64(v))  # v = mant 2^e, mant in [1/2, 1): floor(log2 v) = e - 1
    return 16 - (int(e) - 1)


def quantise(x, scale_log2):
    """float32 (..) -> int64 rint(x * 2^scale) and where that is in range"""
    s = np.asarray(x, dtype=np.float32).astype(np.float64) * np.ldexp(1.0, scale_log2)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(s) & (np.abs(s) <= LIMIT)
    return np.rint(np.where(ok, s, 0.0)).astype(np.int64), ok


def empty(status):
    mesh = dict(vertices=np.zeros((0, 3), np.float32), colors=np.zeros((0, 3), np.float32), keys=np.zeros(0, np.uint64), faces=np.zeros((0, 3), np.uint32))
    return dict(mesh=mesh, counts=dict(dict.fromkeys(COUNTS, 0), status=status), status=status)


def cluster(mesh, m, scale_log2, cluster_slots_log2=None, face_slots_log2=None):
    """mesh: vertices (V,3) f32, colors (V,3) f32, keys (V,) u64, faces (F,3) -> dict(mesh=canonical clustered mesh,
    counts=the six by name, status).  *_slots_log2: the sizes of the device's tables, for the full-table status."""
    assert 1 <= m <= MAX_CELLS
    p, c = np.asarray(mesh["vertices"], np.float32).reshape(-1, 3), np.asarray(mesh["colors"], np.float32).reshape(-1, 3)
    keys = np.asarray(mesh["keys"], dtype=np.uint64).ravel()
    faces = np.asarray(mesh["faces"], dtype=np.int64).reshape(-1, 3)
    V = len(keys)
    if V == 0:
        return empty(0)
    status = 0
    good_key = (keys >> np.uint64(62)) == 0
    if not good_key.all():
        status |= BAD_KEY
    qp, okp = quantise(p, scale_log2)
    qc, okc = quantise(c, 16)
    in_range = okp.all(axis=1) & okc.all(axis=1)
    if not in_range[good_key].all():
        status |= RANGE
    good_face = np.all((faces >= 0) & (faces < V), axis=1)
    if not good_face.all():
        status |= BAD_INDEX
    member = good_key & in_range  # the vertices that reach the cluster table
    ckeys = pack_point(np.floor_divide(lattice(keys), m))
    ukeys, of_vertex = np.unique(ckeys[member], return_inverse=True)
    cluster_of = np.full(V, -1, dtype=np.int64)  # clusters are numbered by ascending key
    cluster_of[member] = of_vertex
    full = cluster_slots_log2 is not None and len(ukeys) > (1 << cluster_slots_log2)
    f = cluster_of[faces[good_face]]
    f = f[np.all(f >= 0, axis=1)]
    collapsed = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])
    f = f[~collapsed]
    # smallest cluster (key) first, winding kept
    r = np.argmin(f, axis=1) if len(f) else np.zeros(0, dtype=np.int64)
    f = np.stack([f[np.arange(len(f)), (r + j) % 3] for j in range(3)], axis=1) if len(f) else f
    ascending = f[:, 1] < f[:, 2]
    triple = np.sort(f, axis=1)
    utriple, group = np.unique(triple, axis=0, return_inverse=True) if len(f) else (triple, np.zeros(0, dtype=np.int64))
    group = np.asarray(group).ravel()
    if not full and face_slots_log2 is not None and len(utriple) > (1 << face_slots_log2):
        full = True
    if full:
        status |= TABLE_FULL
    if status:
        return empty(status)
    has_ascending = np.zeros(len(utriple), dtype=bool)
    has_ascending[group[ascending]] = True
    kept = np.where(has_ascending[:, None], utriple, utriple[:, [0, 2, 1]])
    used = np.zeros(len(ukeys), dtype=bool)
    used[kept.ravel()] = True
    n = np.bincount(of_vertex, minlength=len(ukeys)).astype(np.int64)
    sums = np.zeros((len(ukeys), 6), dtype=np.int64)
    np.add.at(sums, of_vertex, np.concatenate([qp[member], qc[member]], axis=1))
    mean = np.floor_divide(2 * sums + n[:, None], 2 * n[:, None])
    pos = (mean[:, :3].astype(np.float64) * np.ldexp(1.0, -scale_log2)).astype(np.float32)
    col = (mean[:, 3:].astype(np.float64) * np.ldexp(1.0, -16)).astype(np.float32)
    new = np.cumsum(used) - 1
    out = dict(vertices=pos[used], colors=col[used], keys=ukeys[used], faces=new[kept].astype(np.uint32).reshape(-1, 3))
    counts = dict(vertices=int(used.sum()), faces=len(kept), status=0, collapsed=int(collapsed.sum()), duplicates=len(f) - len(kept),
                  unused_clusters=int((~used).sum()))
    return dict(mesh=MW.canonical(out), counts=counts, status=0)


def float64_means(mesh, m):
    """cluster key -> (float64 mean position, members) over all the vertices of a mesh with good keys"""
    ckeys = pack_point(np.floor_divide(lattice(mesh["keys"]), m))
    ukeys, inv = np.unique(ckeys, return_inverse=True)
    n = np.bincount(inv, minlength=len(ukeys))
    s = np.zeros((len(ukeys), 3))
    np.add.at(s, inv, np.asarray(mesh["vertices"], np.float32).astype(np.float64))
    return ukeys, s / n[:, None], n


def plain_mesh(keys, faces, vertices=None, colors=None):
    """a hand-made mesh: positions default to the lattice points themselves, colours to 1/2"""
    keys = np.asarray(keys, dtype=np.uint64)
    v = lattice(keys).astype(np.float32) if vertices is None else np.asarray(vertices, np.float32).reshape(-1, 3)
    c = np.full((len(keys), 3), 0.5, np.float32) if colors is None else np.asarray(colors, np.float32).reshape(-1, 3)
    return dict(vertices=v, colors=c, keys=keys, faces=np.asarray(faces, dtype=np.uint32).reshape(-1, 3))


def lattice_soup(n, seed, voxel_size, spread=6):
    """a random soup as mesh_weld.random_soup's, but every vertex ON the lattice edge (or point) its record names, as a
    real extraction's are: position (L - 1/2 + t axis) * voxel_size"""
    from voxelhashing_amd import vhtypes as T
    rng = np.random.default_rng(seed)
    soup, srcs = MW.random_soup(n, seed, spread)
    keys, ok = MW.vertex_keys(srcs)
    assert ok.all()
    L = lattice(keys).astype(np.float64)
    code = ((keys >> np.uint64(60)) & np.uint64(3)).astype(np.int64)
    t = rng.random(len(keys))
    for a in range(3):
        L[:, a] += np.where(code == a, t, 0.0)
    soup["v"]["p"] = ((L - 0.5) * voxel_size).astype(np.float32).reshape(n, 3, 3)
    return np.ascontiguousarray(soup, dtype=T.TRIANGLE_DTYPE), srcs
