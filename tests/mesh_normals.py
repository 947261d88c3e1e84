"""A numpy restatement of the vertex normals of an indexed mesh ("Vertex normals"), written without
the library and with its own arithmetic: float32 arrays for the face pass (numpy rounds every operation once and fuses
nothing), np.rint for the quantisation, np.add.at on int64 for the sums, float64 for the vertex pass.

Per face: skip one with a repeated index; rotate the triple, winding kept, so that the vertex with the smallest key comes
first; a = p1 - p0, b = p2 - p0, c = a x b, s = c * 2^scale_log2; a component of s that is not finite or exceeds 2^40
sets RANGE and the face adds nothing; otherwise q = rint(s) goes to the three sums of each of the face's three vertices.
Per vertex: d = the sums as float64, n = float32(d / sqrt((dx dx + dy dy) + dz dz)), zero where the sum is zero.  Any
status leaves every normal zero.

reference() is the yardstick of the restatement itself: the area-weighted sums in float64, and the error budget of
every vertex."""
import numpy as np

RANGE, BAD_INDEX = 1, 2
LIMIT = np.float32(2.0 ** 40)


def rotate_to_smallest_key(faces, keys):
    """index triples (F,3) rotated, winding kept, so that the vertex with the smallest key comes first"""
    f = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
    if len(f) == 0:
        return f
    r = np.argmin(np.asarray(keys, dtype=np.uint64)[f], axis=1)
    rows = np.arange(len(f))
    return np.stack([f[rows, (r + k) % 3] for k in range(3)], axis=1)


def face_terms(vertices, keys, faces, scale_log2):
    """-> the faces that add something (rotated), their quantised normals q (int64), and the status word"""
    p = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
    status = 0
    inside = np.all(f < len(p), axis=1) if len(f) else np.zeros(0, dtype=bool)
    if not np.all(inside):
        status |= BAD_INDEX
    f = f[inside]
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    f = rotate_to_smallest_key(f, keys)
    p0, p1, p2 = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    with np.errstate(over="ignore", invalid="ignore"):
        a, b = p1 - p0, p2 - p0
        assert a.dtype == np.float32 and b.dtype == np.float32
        c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
        s = c * np.float32(2.0 ** int(scale_log2))
        assert s.dtype == np.float32
        ok = np.all(np.abs(s) <= LIMIT, axis=1) if len(s) else np.zeros(0, dtype=bool)  # (a NaN fails the comparison)
    if not np.all(ok):
        status |= RANGE
    q = np.rint(s[ok]).astype(np.int64)
    return f[ok], q, status


def vertex_normals(vertices, keys, faces, scale_log2):
    """-> normals (V,3) float32, acc (V,3) int64 (the fixed-point sums), status"""
    p = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    f, q, status = face_terms(p, keys, faces, scale_log2)
    acc = np.zeros((len(p), 3), dtype=np.int64)
    for k in range(3):
        np.add.at(acc, f[:, k], q)
    normals = np.zeros((len(p), 3), dtype=np.float32)
    if status == 0:
        d = acc.astype(np.float64)
        l2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        nz = l2 != 0.0
        normals[nz] = (d[nz] / np.sqrt(l2[nz])[:, None]).astype(np.float32)
    return dict(normals=normals, acc=acc, status=status)


def reference(vertices, faces, scale_log2):
    """float64, no quantisation -> A (V,3): the sums of a x b over every vertex's faces (those without a repeated index);
    E (V,): the error budget of the fixed-point sum, 2^-20 |a| |b| + sqrt(3) / S summed over the vertex's faces (the
    float32 rounding of two subtractions and a two-term product difference, then half a unit of quantisation per
    component); valence (V,)"""
    p = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    f = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    a, b = p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]
    c = np.cross(a, b) if len(f) else np.zeros((0, 3))
    e = 2.0 ** -20 * np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1) + np.sqrt(3.0) / 2.0 ** int(scale_log2)
    A, E, valence = np.zeros((len(p), 3)), np.zeros(len(p)), np.zeros(len(p), dtype=np.int64)
    for k in range(3):
        np.add.at(A, f[:, k], c)
        np.add.at(E, f[:, k], e)
        np.add.at(valence, f[:, k], 1)
    return A, E, valence


def check_against_reference(normals, vertices, faces, scale_log2):
    """For every vertex with a non-zero float64 sum A: |n - A / |A|| <= 2 E / |A| + 2^-22 (a perturbation of A by at most
    E turns its direction by at most 2 E / |A|; the last term is the rounding of the components to float32).  -> the
    largest ratio of error to bound, and the largest | |n| - 1 | over the non-zero normals."""
    A, E, valence = reference(vertices, faces, scale_log2)
    n = np.asarray(normals, dtype=np.float64)
    la = np.linalg.norm(A, axis=1)
    has = la > 0
    err = np.linalg.norm(n[has] - A[has] / la[has, None], axis=1)
    bound = 2.0 * E[has] / la[has] + 2.0 ** -22
    assert np.all(err <= bound), f"{int((err > bound).sum())} normals off their bound, worst ratio {float((err / bound).max())}"
    assert np.all(n[valence == 0] == 0.0), "a vertex without a face has a normal"
    length = np.linalg.norm(n[np.any(n != 0, axis=1)], axis=1)
    unit = float(np.abs(length - 1.0).max()) if len(length) else 0.0
    assert unit <= 2.0 ** -23, unit
    return (float((err / bound).max()) if len(err) else 0.0), unit
