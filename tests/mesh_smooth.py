"""A numpy restatement of the Taubin smoothing ("Mesh smoothing"): what N iterations of the
lambda | mu scheme under the uniform umbrella operator have to give on an indexed mesh, written without the library and
without a hash table -- np.unique finds the distinct edges, np.add.at on int64 sums the neighbours.

Edges: a face with an index >= V sets BAD_INDEX and contributes nothing, a face with a repeated index contributes no
edge, every other face names three undirected edges {lo, hi}; the distinct edges are the neighbour relation, the number
of faces that name an edge its use count, a vertex's distinct neighbours its degree n (above MAX_DEGREE: DEGREE).  An
edge of use count 1 is a boundary edge, both its ends boundary vertices.  A vertex moves if n > 0 and, with
keep_boundary, it is no boundary vertex; every other vertex keeps its input bits.

q = rint(p * 2^scale) per component of every vertex (not finite, or above 2^40: RANGE).  Half step k = 0 ... 2 N - 1,
f = lambdaQ16 for even k and muQ16 for odd k, for a moved vertex from the q of the half step before:
d = sum of the neighbours' q - n q, u = floor((2 d + n) / (2 n)), q' = q + ((f u + 2^15) >> 16); |q'| > 2^40: RANGE.
A moved vertex comes back as float32((float64) q * 2^-scale).

The statuses come in stages, and the first stage that leaves one ends the run: the faces (BAD_INDEX, TABLE_FULL), the
vertices (RANGE of the input, DEGREE), each half step (RANGE).

smooth() returns the mesh in mesh_weld.canonical form."""
import numpy as np

import mesh_weld as MW

TABLE_FULL, RANGE, BAD_INDEX, DEGREE = 1, 2, 4, 8
MAX_DEGREE, MAX_ITERATIONS, MAX_FACTOR_Q16 = 1 << 16, 100, 1 << 16
DEFAULT_LAMBDA_Q16, DEFAULT_MU_Q16 = 32768, -34734
COUNTS = ("moved", "boundary_vertices", "isolated_vertices", "status", "edges", "boundary_edges")
LIMIT = 1 << 40


def q16(f):
    """a factor in units of 2^-16, by rint of the float32"""
    return int(np.rint(np.float64(np.float32(f)) * 65536.0))


def quantise(x, scale_log2):
    """float32 (..) -> int64 rint(x * 2^scale) and where that is in range"""
    s = np.asarray(x, dtype=np.float32).astype(np.float64) * np.ldexp(1.0, scale_log2)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(s) & (np.abs(s) <= float(LIMIT))
    return np.rint(np.where(ok, s, 0.0)).astype(np.int64), ok


def edges_of(faces, V):
    """faces (F,3) -> status bits of the faces, the distinct edges (E,2) int64 with lo < hi, their use counts"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    good = np.all((faces >= 0) & (faces < V), axis=1)
    status = 0 if good.all() else BAD_INDEX
    f = faces[good]
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    if len(e) == 0:
        return status, np.zeros((0, 2), np.int64), np.zeros(0, np.int64)
    edges, uses = np.unique(e, axis=0, return_counts=True)
    return status, edges, uses


def empty(status):
    mesh = dict(vertices=np.zeros((0, 3), np.float32), colors=np.zeros((0, 3), np.float32), keys=np.zeros(0, np.uint64), faces=np.zeros((0, 3), np.uint32))
    return dict(mesh=mesh, counts=dict(dict.fromkeys(COUNTS, 0), status=status), status=status)


def half_step(q, edges, n, moved, f):
    """one Jacobi half step on int64 positions (V,3) -> the new array"""
    sums = np.zeros_like(q)
    np.add.at(sums, edges[:, 0], q[edges[:, 1]])
    np.add.at(sums, edges[:, 1], q[edges[:, 0]])
    nn = np.maximum(n, 1)[:, None]
    d = sums - nn * q
    u = np.floor_divide(2 * d + nn, 2 * nn)
    return np.where(moved[:, None], q + ((f * u + (1 << 15)) >> 16), q)


def smooth(mesh, iterations, lambda_q16=DEFAULT_LAMBDA_Q16, mu_q16=DEFAULT_MU_Q16, keep_boundary=True, scale_log2=21, edge_slots_log2=None):
    """mesh: vertices (V,3) f32, colors (V,3) f32, keys (V,) u64, faces (F,3) -> dict(mesh=canonical smoothed mesh,
    counts=the six by name, status, moved=which vertices of the INPUT's numbering move).  edge_slots_log2: the size of the device's edge table, for the
    full-table status."""
    assert 1 <= iterations <= MAX_ITERATIONS and abs(lambda_q16) <= MAX_FACTOR_Q16 and abs(mu_q16) <= MAX_FACTOR_Q16
    p, c = np.asarray(mesh["vertices"], np.float32).reshape(-1, 3), np.asarray(mesh["colors"], np.float32).reshape(-1, 3)
    keys = np.asarray(mesh["keys"], dtype=np.uint64).ravel()
    V = len(keys)
    if V == 0:
        return dict(empty(0), moved=np.zeros(0, bool))
    status, edges, uses = edges_of(mesh["faces"], V)
    if edge_slots_log2 is not None and len(edges) > (1 << edge_slots_log2):
        status |= TABLE_FULL
    if status:
        return empty(status)
    n = np.bincount(edges.ravel(), minlength=V).astype(np.int64)
    boundary = np.zeros(V, dtype=bool)
    boundary[edges[uses == 1].ravel()] = True
    q, ok = quantise(p, scale_log2)
    if not ok.all():
        status |= RANGE
    if (n > MAX_DEGREE).any():
        status |= DEGREE
    if status:
        return empty(status)
    moved = (n > 0) & ~(boundary & bool(keep_boundary))
    for k in range(2 * iterations):
        q = half_step(q, edges, n, moved, int(mu_q16 if k & 1 else lambda_q16))
        if (np.abs(q) > LIMIT).any():
            return empty(RANGE)
    pos = np.where(moved[:, None], (q.astype(np.float64) * np.ldexp(1.0, -scale_log2)).astype(np.float32), p)
    out = dict(vertices=pos, colors=c, keys=keys, faces=np.asarray(mesh["faces"], dtype=np.uint32).reshape(-1, 3))
    counts = dict(moved=int(moved.sum()), boundary_vertices=int(boundary.sum()), isolated_vertices=int((n == 0).sum()), status=0, edges=len(edges),
                  boundary_edges=int((uses == 1).sum()))
    return dict(mesh=MW.canonical(out), counts=counts, status=0, moved=moved)


def float64_taubin(mesh, iterations, lam, mu, keep_boundary=True):
    """the same scheme on float64 positions, nothing rounded -> (V,3) float64 in the input's numbering"""
    p = np.asarray(mesh["vertices"], np.float32).astype(np.float64)
    _, edges, uses = edges_of(mesh["faces"], len(p))
    n = np.bincount(edges.ravel(), minlength=len(p)).astype(np.float64)
    boundary = np.zeros(len(p), dtype=bool)
    boundary[edges[uses == 1].ravel()] = True
    moved = (n > 0) & ~(boundary & bool(keep_boundary))
    for k in range(2 * iterations):
        sums = np.zeros_like(p)
        np.add.at(sums, edges[:, 0], p[edges[:, 1]])
        np.add.at(sums, edges[:, 1], p[edges[:, 0]])
        step = (mu if k & 1 else lam) * (sums / np.maximum(n, 1)[:, None] - p)
        p = np.where(moved[:, None], p + step, p)
    return p


def error_bound_quanta(iterations, lambda_q16, mu_q16):
    """e_0 = 1/2 (the quantisation), e_{k+1} = (1 + 2 |f_k|) e_k + 1: a half step maps an error e of every position to
    at most (1 + 2 |f|) e -- |f| e through the neighbours' mean, |f| e through the vertex's own term, e carried -- and
    adds half a quantum for u (times |f| <= 1) and half for the shift"""
    e = 0.5
    for k in range(2 * iterations):
        e = (1.0 + 2.0 * abs(mu_q16 if k & 1 else lambda_q16) / 65536.0) * e + 1.0
    return e


# ---------------------------------------------------------------------------- meshes

def plain_mesh(vertices, faces, keys=None, colors=None):
    """a hand-made mesh: keys default to 1000 + the vertex number (distinct, ascending), colours to a ramp"""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    k = 1000 + np.arange(len(v), dtype=np.uint64) if keys is None else np.asarray(keys, dtype=np.uint64)
    c = (np.arange(3 * len(v), dtype=np.float32).reshape(-1, 3) % 7) / 8 if colors is None else np.asarray(colors, np.float32).reshape(-1, 3)
    return dict(vertices=v, colors=c, keys=k, faces=np.asarray(faces, dtype=np.uint32).reshape(-1, 3))


def uv_sphere(n_lon=24, n_lat=16, radius=0.5, noise=0.004, seed=1):
    """a closed UV sphere: two poles and n_lat - 1 rings of n_lon vertices, radial noise of that standard deviation"""
    rng = np.random.default_rng(seed)
    v = [(0.0, 0.0, 1.0)]
    for i in range(1, n_lat):
        t = np.pi * i / n_lat
        for j in range(n_lon):
            a = 2 * np.pi * j / n_lon
            v.append((np.sin(t) * np.cos(a), np.sin(t) * np.sin(a), np.cos(t)))
    v.append((0.0, 0.0, -1.0))
    v = np.array(v)
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon
    south = len(v) - 1
    f = [(0, ring(1, j), ring(1, j + 1)) for j in range(n_lon)]
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            f += [(ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)), (ring(i, j), ring(i + 1, j + 1), ring(i, j + 1))]
    f += [(south, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)) for j in range(n_lon)]
    r = radius + noise * rng.standard_normal(len(v))
    return plain_mesh(v * r[:, None], f)


def open_patch(n=12, spacing=0.04, noise=0.004, seed=2):
    """an open n x n grid of vertices in the plane z = 0 with noise in z, two faces a cell: 4 n - 4 rim vertices"""
    rng = np.random.default_rng(seed)
    ij = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), axis=-1).reshape(-1, 2)
    v = np.concatenate([(ij - (n - 1) / 2) * spacing, noise * rng.standard_normal((n * n, 1))], axis=1)
    at = lambda i, j: i * n + j
    f = []
    for i in range(n - 1):
        for j in range(n - 1):
            f += [(at(i, j), at(i + 1, j), at(i + 1, j + 1)), (at(i, j), at(i + 1, j + 1), at(i, j + 1))]
    rim = (ij[:, 0] == 0) | (ij[:, 0] == n - 1) | (ij[:, 1] == 0) | (ij[:, 1] == n - 1)
    return plain_mesh(v, f), rim


def closed_fan(spokes):
    """a hub (vertex 0) with `spokes` neighbours on a unit circle below it and one face between every two next to each
    other, all the way round: the hub's edges have two faces each, the rim's one"""
    a = 2 * np.pi * np.arange(spokes) / spokes
    v = np.concatenate([[(0.0, 0.0, 0.25)], np.stack([np.cos(a), np.sin(a), np.zeros(spokes)], axis=1)])
    i = np.arange(spokes)
    f = np.stack([np.zeros(spokes, np.int64), 1 + i, 1 + (i + 1) % spokes], axis=1)
    return plain_mesh(v, f, keys=np.arange(len(v), dtype=np.uint64))


def renumbered(mesh, seed):
    """the same mesh with the vertices in another order, the faces permuted and every triple rotated"""
    rng = np.random.default_rng(seed)
    p = rng.permutation(len(mesh["keys"]))
    inv = np.empty_like(p)
    inv[p] = np.arange(len(p))
    f = inv[np.asarray(mesh["faces"], dtype=np.int64).reshape(-1, 3)]
    f = f[rng.permutation(len(f))]
    r = rng.integers(0, 3, len(f))
    f = np.stack([f[np.arange(len(f)), (r + k) % 3] for k in range(3)], axis=1) if len(f) else f
    return dict(vertices=mesh["vertices"][p], colors=mesh["colors"][p], keys=mesh["keys"][p], faces=f.astype(np.uint32).reshape(-1, 3))
