"""The indexed-mesh passes at launcher level, on hand-made input: weld, accumulating weld, vertex normals, connected
components, vertex clustering, Taubin smoothing, and the PLY writer."""
import ctypes as C

import numpy as np

from .. import vhtypes as T
from ..lib import check, f16, load
from ._common import _Buffers, _counts_by_name, _int3, _scalar_out

GUARD_WORD = 0xa5a5a5a5  # what the `guard` options fill the room behind an array with


def mesh_weld_key(cell, edge, snap):
    """vh_mesh_weld_key: the 64-bit key of a vertex (host side, no GPU); raises VhError when it has none"""
    return int(_scalar_out(C.c_uint64, "vh_mesh_weld_key", load().vh_mesh_weld_key, _int3(cell), int(edge), int(snap)))


def _upload_soup(dev, tag, triangles, sources):
    """a soup (T.TRIANGLE_DTYPE) and its records (T.TRIANGLE_SOURCE_DTYPE) into `dev` under `tag` -> the two device pointers and the triangle count"""
    tris = np.ascontiguousarray(triangles, dtype=T.TRIANGLE_DTYPE).ravel()
    srcs = np.ascontiguousarray(sources, dtype=T.TRIANGLE_SOURCE_DTYPE).ravel()
    if len(tris) != len(srcs):
        raise ValueError("one source record per triangle")
    return dev.upload(tag + ".triangles", tris).ptr, dev.upload(tag + ".sources", srcs).ptr, len(tris)


def _check_weld(code, raise_on_status, what, status=None):
    """what a read of a weld's counts returned: a HIP error always raises; a status raises if asked to, and, where the
    status word is given, a code without one always"""
    if code < 0 or (code != 0 and (raise_on_status or status == 0)):
        check(code, what)


def _welded_arrays(nv, nf, what, download):
    """the arrays of a welded mesh of nv vertices and nf faces, filled by download(vertices, keys, faces, nv, nf) -> dict"""
    v = np.zeros(int(nv), dtype=T.VERTEX_DTYPE)
    k = np.zeros(int(nv), dtype=np.uint64)
    f = np.zeros((int(nf), 3), dtype=np.uint32)
    check(download(v.ctypes.data, k.ctypes.data, f.ctypes.data, len(v), len(f)), what)
    return dict(vertices=np.ascontiguousarray(v["p"]), colors=np.ascontiguousarray(v["c"]), keys=k, faces=f)


def _vertex_arrays(records):
    """T.VERTEX_DTYPE records -> their positions and colours as the entries `vertices`, `colors` of a mesh"""
    return dict(vertices=np.ascontiguousarray(records["p"]), colors=np.ascontiguousarray(records["c"]))


def mesh_weld(triangles, sources, slots_log2=0, raise_on_status=True, stream=None):
    """vh_mesh_weld on hand-made input: a soup (T.TRIANGLE_DTYPE) and its records (T.TRIANGLE_SOURCE_DTYPE) ->
    vertices, colors, keys, faces as CUDAMarchingCubesHashSDF.indexed(), and counts / status / code of the weld.  A full
    table or a key out of range raises VhError, or with raise_on_status=False comes back as `code` beside empty arrays."""
    L = load()
    with _Buffers(stream) as dev:
        d_tris, d_srcs, n = _upload_soup(dev, "soup", triangles, sources)
        w = T.MeshWeldData()
        check(L.vh_mesh_weld_data_alloc(C.byref(w), n, slots_log2), "vh_mesh_weld_data_alloc")
        slots = int(w.m_slotsLog2)
        try:
            check(L.vh_mesh_weld(d_tris, d_srcs, n, C.byref(w), slots_log2, stream), "vh_mesh_weld")
            counts = (C.c_uint32 * 3)()
            code = L.vh_mesh_weld_get_counts(C.byref(w), counts, stream)
            _check_weld(code, raise_on_status, "vh_mesh_weld", counts[2])
            out = _welded_arrays(counts[0], counts[1], "vh_mesh_weld_download",
                                 lambda v, k, f, nv, nf: L.vh_mesh_weld_download(C.byref(w), v, k, f, nv, nf, stream))
        finally:
            L.vh_mesh_weld_data_free(C.byref(w))
    return dict(out, counts=(int(counts[0]), int(counts[1])), status=int(counts[2]), code=int(code), slots_log2=slots)


def mesh_normals_default_scale_log2(voxel_size):
    """vh_mesh_normals_default_scale_log2 (host side, no GPU); raises VhError for a voxel size it refuses"""
    return int(_scalar_out(C.c_int32, "vh_mesh_normals_default_scale_log2", load().vh_mesh_normals_default_scale_log2, float(voxel_size)))


def _vertex_records(vertices, colors=None):
    """(V,3) positions with (V,3) colours or none, or T.VERTEX_DTYPE records -> contiguous records"""
    v = np.asarray(vertices)
    if v.dtype != T.VERTEX_DTYPE:
        p = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3)
        v = np.zeros(len(p), dtype=T.VERTEX_DTYPE)
        v["p"] = p
        if colors is not None:
            v["c"] = np.ascontiguousarray(colors, dtype=np.float32).reshape(len(p), 3)
    return np.ascontiguousarray(v).ravel()


def _mesh_inputs(vertices, colors, keys, faces):
    """a hand-made indexed mesh -> (records T.VERTEX_DTYPE [V], keys u64 [V], faces u32 [F, 3], V, F)"""
    v = _vertex_records(vertices, colors)
    k = np.ascontiguousarray(keys, dtype=np.uint64).ravel()
    f = np.ascontiguousarray(faces, dtype=np.uint32).reshape(-1, 3)
    if len(k) != len(v):
        raise ValueError("one key per vertex")
    return v, k, f, len(v), len(f)


def _upload_mesh(dev, v, k, f):
    """the inputs of a pass into `dev` as "in.vertices", "in.keys", "in.faces"; a mesh without faces gets room for one"""
    dev.upload("in.vertices", v)
    dev.upload("in.keys", k)
    dev.upload("in.faces", f if len(f) else np.zeros((1, 3), np.uint32))


def _alloc_pass_data(dev, sizes, nv, guard, guarded):
    """the arrays of a pass's data struct into `dev` under their field names (sizes: bytes by name) -> their device
    pointers by name.  With guard, each of the per-vertex arrays `guarded` (words per vertex by name) is filled with
    GUARD_WORD and has that many words of room behind its nv vertices"""
    for name, nbytes in sizes.items():
        if guard and name in guarded:
            dev.alloc(name, 4 * (guarded[name] * nv + guard), fill=GUARD_WORD)
        else:
            dev.alloc(name, nbytes)
    return {name: dev[name].ptr for name in sizes}


def _mesh_result(what, status, raise_on_status, table_full=None, counts=None):
    """what a pass's status word comes to: code 0 without one, VH_ERR_STAGING_OVERFLOW (2) for the bit `table_full`
    alone, else VH_ERR_BAD_ARGUMENT (4), raised as VhError if asked to -> dict of status and code and, given (names,
    values), the counts by name"""
    code = 0 if status == 0 else 2 if status == table_full else 4
    if code and raise_on_status:
        check(code, f"{what} (status {status})")
    out = {} if counts is None else dict(counts=_counts_by_name(*counts))
    return dict(out, status=status, code=code)


def mesh_vertex_normals(vertices, keys, faces, scale_log2, raise_on_status=True, stream=None):
    """vh_mesh_vertex_normals on hand-made input: vertices (V,3) f32 positions, or T.VERTEX_DTYPE records; keys (V,) u64;
    faces (F,3) u32 -> normals (V,3) f32, acc (V,3) i64 (the fixed-point sums), status, code.  A status raises VhError
    (VH_ERR_BAD_ARGUMENT), or with raise_on_status=False comes back as `code` beside the all-zero normals."""
    v, k, f, nv, nf = _mesh_inputs(vertices, None, keys, faces)
    with _Buffers(stream) as dev:
        _upload_mesh(dev, v, k, f)
        dev.alloc("sums", 24 * nv)
        dev.alloc("normals", 12 * nv)
        dev.alloc("status", 4)
        check(load().vh_mesh_vertex_normals(dev["in.vertices"].ptr, dev["in.keys"].ptr, dev["in.faces"].ptr, nv, nf, int(scale_log2), dev["sums"].ptr,
                                            dev["normals"].ptr, dev["status"].ptr, stream), "vh_mesh_vertex_normals")
        status = int(dev.download("status", np.uint32, 1)[0])
        normals = dev.download("normals", np.float32, 3 * nv).reshape(-1, 3)
        acc = dev.download("sums", np.int64, 3 * nv).reshape(-1, 3)
    return dict(normals=normals, acc=acc, **_mesh_result("vh_mesh_vertex_normals", status, raise_on_status))


def _label_components(L, dev, nv, nf):
    """vh_mesh_components on "in.keys" and "in.faces" into "root", "face_count" and "status" of `dev`"""
    check(L.vh_mesh_components(dev["in.keys"].ptr, dev["in.faces"].ptr, nv, nf, dev["root"].ptr, dev["face_count"].ptr, dev["status"].ptr, dev.stream),
          "vh_mesh_components")


def mesh_components(keys, faces, stream=None, guard=0):
    """vh_mesh_components on hand-made input: keys (V,) u64, faces (F,3) u32 -> root (V,) u32 (the index of each
    vertex's component's first vertex by (key, index)), face_count (V,) u32 (at the roots), status, code (4 =
    VH_ERR_BAD_ARGUMENT for either status bit).  guard: the last `guard` keys are not vertices but room behind them, with
    that many words of 0xa5a5a5a5 behind root and face_count on the device, returned as root_guard / count_guard."""
    k = np.ascontiguousarray(keys, dtype=np.uint64).ravel()
    f = np.ascontiguousarray(faces, dtype=np.uint32).reshape(-1, 3)
    nv, nf = len(k) - guard, len(f)
    with _Buffers(stream) as dev:
        dev.upload("in.keys", k)
        dev.upload("in.faces", f)
        dev.alloc("root", 4 * (nv + guard), fill=GUARD_WORD)
        dev.alloc("face_count", 4 * (nv + guard), fill=GUARD_WORD)
        dev.alloc("status", 4)
        _label_components(load(), dev, nv, nf)
        status = int(dev.download("status", np.uint32, 1)[0])
        root = dev.download("root", np.uint32, nv + guard)
        cnt = dev.download("face_count", np.uint32, nv + guard)
    return dict(root=root[:nv], face_count=cnt[:nv], root_guard=root[nv:], count_guard=cnt[nv:], **_mesh_result("vh_mesh_components", status, False))


def mesh_components_filter(vertices, colors, keys, faces, min_faces=0, largest_only=False, normals=None, raise_on_status=True, stream=None):
    """vh_mesh_components, then vh_mesh_components_filter, on hand-made input: vertices (V,3) f32 with colors (V,3) f32
    or None, or T.VERTEX_DTYPE records; keys (V,) u64; faces (F,3) u32; normals (V,3) f32 or None -> the filtered
    vertices, colors, keys, faces (and normals) as mesh_weld(), root and face_count of the labelling, counts (the six by
    name), status, code.  A status raises VhError (VH_ERR_BAD_ARGUMENT), or with raise_on_status=False comes back as
    `code` beside an empty mesh."""
    L = load()
    v, k, f, nv, nf = _mesh_inputs(vertices, colors, keys, faces)
    n = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(nv, 3)
    with _Buffers(stream) as dev:
        _upload_mesh(dev, v, k, f)
        for name, nbytes in (("root", 4 * nv), ("face_count", 4 * nv), ("status", 4), ("new_index", 4 * nv), ("best", 16),
                             ("out.vertices", 24 * nv), ("out.keys", 8 * nv), ("out.faces", 12 * nf), ("counts", 24)):
            dev.alloc(name, nbytes)
        if n is not None:
            dev.upload("in.normals", n)
            dev.alloc("out.normals", 12 * nv)
        _label_components(L, dev, nv, nf)
        check(L.vh_mesh_components_filter(dev["in.vertices"].ptr, dev["in.keys"].ptr, dev["in.normals"].ptr if n is not None else None, dev["in.faces"].ptr,
                                          nv, nf, dev["root"].ptr, dev["face_count"].ptr, dev["status"].ptr, int(min_faces), 1 if largest_only else 0,
                                          dev["new_index"].ptr, dev["best"].ptr, dev["out.vertices"].ptr, dev["out.keys"].ptr,
                                          dev["out.normals"].ptr if n is not None else None, dev["out.faces"].ptr, dev["counts"].ptr, stream),
              "vh_mesh_components_filter")
        status = int(dev.download("status", np.uint32, 1)[0])
        counts = dev.download("counts", np.uint32, 6)
        kv, kf = int(counts[3]), int(counts[4])
        out = dict(_vertex_arrays(dev.download("out.vertices", T.VERTEX_DTYPE, kv)), keys=dev.download("out.keys", np.uint64, kv),
                   faces=dev.download("out.faces", np.uint32, 3 * kf).reshape(-1, 3),
                   root=dev.download("root", np.uint32, nv), face_count=dev.download("face_count", np.uint32, nv))
        if n is not None:
            out["normals"] = dev.download("out.normals", np.float32, 3 * kv).reshape(-1, 3)
    return dict(out, **_mesh_result("vh_mesh_components", status, raise_on_status, counts=(T.COMPONENTS_COUNTS, counts)))


def mesh_cluster_key(vertex_key, cells_per_cluster):
    """vh_mesh_cluster_key (host side, no GPU): the key of the cluster a vertex key falls into"""
    return int(_scalar_out(C.c_uint64, "vh_mesh_cluster_key", load().vh_mesh_cluster_key, int(vertex_key), int(cells_per_cluster)))


def mesh_cluster_default_scale_log2(voxel_size):
    """vh_mesh_cluster_default_scale_log2 (host side, no GPU)"""
    return int(_scalar_out(C.c_int32, "vh_mesh_cluster_default_scale_log2", load().vh_mesh_cluster_default_scale_log2, float(voxel_size)))


def mesh_cluster(vertices, colors, keys, faces, cells_per_cluster, scale_log2, cluster_slots_log2=0, face_slots_log2=0, raise_on_status=True,
                 stream=None, guard=0):
    """vh_mesh_cluster on hand-made input: vertices (V,3) f32 with colors (V,3) f32 or None, or T.VERTEX_DTYPE records;
    keys (V,) u64; faces (F,3) u32 -> the clustered vertices, colors, keys, faces as mesh_weld(), counts (the six by
    name), status, code.  cluster_slots_log2 / face_slots_log2: the tables' sizes (0: the default, twice the vertices
    and faces); smaller ones fill.  A status raises VhError (VH_ERR_STAGING_OVERFLOW for a full table alone, else
    VH_ERR_BAD_ARGUMENT), or with raise_on_status=False comes back as `code` beside an empty mesh.  guard: that many
    words of 0xa5a5a5a5 behind the per-vertex slot array on the device, returned as slot_guard: where a face index >= V
    would lead."""
    L = load()
    v, k, f, nv, nf = _mesh_inputs(vertices, colors, keys, faces)

    def log2_for(n, given):
        default = _scalar_out(C.c_uint32, "vh_mesh_cluster_default_slots_log2", L.vh_mesh_cluster_default_slots_log2, n)
        return int(given) if given else int(default)
    cl, fl = log2_for(nv, cluster_slots_log2), log2_for(nf, face_slots_log2)
    cs, fs = 1 << cl, 1 << fl
    sizes = dict(d_clusterKeys=8 * cs, d_clusterSums=48 * cs, d_clusterCount=4 * cs, d_clusterIndex=4 * cs, d_vertexSlot=4 * max(nv, 1),
                 d_facePairs=8 * fs, d_faceThirds=4 * fs, d_faceWindings=4 * fs, d_work=8, d_vertices=24 * max(nv, 1), d_keys=8 * max(nv, 1),
                 d_faces=12 * max(nf, 1), d_counts=24)
    with _Buffers(stream) as dev:
        _upload_mesh(dev, v, k, f)
        data = T.MeshClusterData(m_clusterSlotsLog2=cl, m_faceSlotsLog2=fl, **_alloc_pass_data(dev, sizes, nv, guard, dict(d_vertexSlot=1)))
        check(L.vh_mesh_cluster(dev["in.vertices"].ptr, dev["in.keys"].ptr, dev["in.faces"].ptr, nv, nf, int(cells_per_cluster), int(scale_log2),
                                C.byref(data), stream), "vh_mesh_cluster")
        counts = dev.download("d_counts", np.uint32, 6)
        status = int(counts[2])
        out = dict(_vertex_arrays(dev.download("d_vertices", T.VERTEX_DTYPE, int(counts[0]))), keys=dev.download("d_keys", np.uint64, int(counts[0])),
                   faces=dev.download("d_faces", np.uint32, 3 * int(counts[1])).reshape(-1, 3))
        if guard:
            out["slot_guard"] = dev.download("d_vertexSlot", np.uint32, nv + guard)[nv:]
    return dict(out, **_mesh_result("vh_mesh_cluster", status, raise_on_status, T.CLUSTER_TABLE_FULL, (T.CLUSTER_COUNTS, counts)))


def mesh_smooth(vertices, colors, keys, faces, iterations, lam=0.5, mu=-0.53, keep_boundary=True, scale_log2=21, edge_slots_log2=None, raise_on_status=True,
                stream=None, guard=0, factors_q16=None):
    """vh_mesh_smooth on hand-made input: vertices (V,3) f32 with colors (V,3) f32 or None, or T.VERTEX_DTYPE records;
    keys (V,) u64; faces (F,3) u32 -> the mesh with the smoothed vertices (vertices, colors, keys, faces as mesh_weld();
    keys and faces are the input's), counts (the six by name), status, code.  lam, mu go to units of 2^-16 by rint, or
    factors_q16 = (lambdaQ16, muQ16) gives them as they are.  edge_slots_log2: the edge table's size (None: the
    default, six times the faces); a smaller one fills.  A status raises VhError (VH_ERR_STAGING_OVERFLOW for a full
    table alone, else VH_ERR_BAD_ARGUMENT), or with raise_on_status=False comes back as `code` beside an empty mesh.
    guard: that many words of 0xa5a5a5a5 behind the per-vertex degree, flag, position and sum arrays on the device,
    returned as guards: where a face index >= V would lead."""
    L = load()
    v, k, f, nv, nf = _mesh_inputs(vertices, colors, keys, faces)
    lq, mq = (int(factors_q16[0]), int(factors_q16[1])) if factors_q16 is not None else (T.smooth_factor_q16(lam), T.smooth_factor_q16(mu))
    default = _scalar_out(C.c_uint32, "vh_mesh_smooth_default_slots_log2", L.vh_mesh_smooth_default_slots_log2, nf)
    el = int(default if edge_slots_log2 is None else edge_slots_log2)
    es = 1 << el
    per_vertex = dict(d_degree=1, d_flags=1, d_positions=12, d_sums=6)  # the guarded arrays: words per vertex
    sizes = dict(d_edgeKeys=8 * es, d_edgeUses=4 * es, **{name: 4 * w * max(nv, 1) for name, w in per_vertex.items()}, d_work=20, d_vertices=24 * max(nv, 1),
                 d_counts=24)
    with _Buffers(stream) as dev:
        _upload_mesh(dev, v, k, f)
        data = T.MeshSmoothData(m_edgeSlotsLog2=el, m_pad=0, **_alloc_pass_data(dev, sizes, nv, guard, per_vertex))
        check(L.vh_mesh_smooth(dev["in.vertices"].ptr, dev["in.keys"].ptr, dev["in.faces"].ptr, nv, nf, int(iterations), lq, mq, 1 if keep_boundary else 0,
                               int(scale_log2), C.byref(data), stream), "vh_mesh_smooth")
        counts = dev.download("d_counts", np.uint32, 6)
        status = int(counts[3])
        n_out = nv if status == 0 else 0
        out = dict(_vertex_arrays(dev.download("d_vertices", T.VERTEX_DTYPE, n_out)), keys=k[:n_out].copy(), faces=f.copy() if status == 0 else f[:0].copy())
        if guard:
            out["guards"] = [dev.download(name, np.uint32, w * nv + guard)[w * nv:] for name, w in per_vertex.items()]
    return dict(out, **_mesh_result("vh_mesh_smooth", status, raise_on_status, T.SMOOTH_TABLE_FULL, (T.SMOOTH_COUNTS, counts)))


def mesh_save_ply(filename, vertices, colors=None, normals=None, faces=None, transform=None):
    """vh_mesh_save_ply (host side, no GPU): the mesh container's applyTransform (when a transform is given) and
    saveToPLY on numpy arrays: vertices (V,3), colors (V,4) or None, normals (V,3) or None, faces (F,3) or None"""
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    c = None if colors is None else np.ascontiguousarray(colors, dtype=np.float32).reshape(len(v), 4)
    n = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(len(v), 3)
    f = np.zeros(0, dtype=np.uint32) if faces is None else np.ascontiguousarray(faces, dtype=np.uint32).ravel()
    check(load().vh_mesh_save_ply(v.ctypes.data, None if c is None else c.ctypes.data, None if n is None else n.ctypes.data, len(v),
                                  f.ctypes.data if len(f) else None, len(f), f16(transform) if transform is not None else None,
                                  str(filename).encode()), "vh_mesh_save_ply")


def mesh_weld_appends(parts, slots_log2=0, fixed=False, reserve_triangles=0, raise_on_status=True, stream=None, normals_scale_log2=None,
                      min_component_faces=0, largest_component=False, append_after_components=None, cluster_cells=0, cluster_scale_log2=0,
                      append_after_cluster=None, smooth_iterations=0, smooth_lambda=0.5, smooth_mu=-0.53, keep_boundary=True, smooth_scale_log2=21,
                      append_after_smooth=None):
    """vh_mesh_weld_accum_* on hand-made input: parts is a sequence of (soup, records), appended in order to one
    accumulation -> vertices, colors, keys, faces as mesh_weld(), counts (vertices, faces), stats (the six counts by
    name), status and code.  slots_log2 is the table's FIRST size (0: the smallest), reserve_triangles that of the
    vertex and face arrays; fixed keeps the table from growing.  Errors as mesh_weld().
    normals_scale_log2: run the vertex-normal pass over the finished accumulation -> also normals (V,3) f32 and
    normals_code (what the download returned: 4 when the pass left a status).
    min_component_faces, largest_component: run the component filter over the finished accumulation (after the normals,
    which then ride along) -> also `filtered` (vertices, colors, keys, faces, normals if any) and component_counts (the
    six by name); the unfiltered mesh comes back as without.  append_after_components: one more (soup, records) appended
    after the pass -> stale_code, what the filter's download then returns (4: refused).
    cluster_cells (1 ... 64), cluster_scale_log2: run the vertex clustering over the finished accumulation, BEFORE the
    normals and the components, which are then of the clustered mesh -> also `clustered` (vertices, colors, keys, faces),
    cluster_counts (the six by name) and cluster_code (what the counts' read returned: 4 or 2 when the pass left a
    status).  append_after_cluster: one more (soup, records) appended after the pass -> stale_cluster_code, what the
    counts' read then returns (4: refused); not with the normals or the filter.
    smooth_iterations (1 ... 100), smooth_lambda, smooth_mu, keep_boundary, smooth_scale_log2: run the Taubin smoothing
    over the finished accumulation, AFTER the clustering and before the normals and the components, which then take the
    smoothed vertices -> also `smoothed` (the vertices and colors; keys and faces of the clustered mesh if there is one,
    else the welded one's), smooth_counts (the six by name) and smooth_code.  append_after_smooth: one more (soup,
    records) appended after the pass -> stale_smooth_code, what the counts' read then returns (4: refused)."""
    L = load()
    h = C.c_void_p()
    check(L.vh_mesh_weld_accum_create(slots_log2, reserve_triangles, int(fixed), C.byref(h)), "vh_mesh_weld_accum_create")
    with _Buffers(stream) as dev:
        def append(tag, part):
            d_tris, d_srcs, n = _upload_soup(dev, tag, *part)
            check(L.vh_mesh_weld_accum_append(h, d_tris, d_srcs, n, stream), "vh_mesh_weld_accum_append")

        def stale_code(part, tag, read):
            """one more soup appended after a pass, where the test asks for it: {tag: what `read` then returns}"""
            if part is None:
                return {}
            append(tag, part)
            return {tag: int(read())}

        try:
            check(L.vh_mesh_weld_accum_begin(h, stream), "vh_mesh_weld_accum_begin")
            for i, part in enumerate(parts):
                append(f"part{i}", part)
            counts = (C.c_uint32 * 6)()
            code = L.vh_mesh_weld_accum_get_counts(h, counts, stream)
            _check_weld(code, raise_on_status, "vh_mesh_weld_accum", counts[2])
            out = _welded_arrays(counts[0], counts[1], "vh_mesh_weld_accum_download",
                                 lambda v, k, f, nv, nf: L.vh_mesh_weld_accum_download(h, v, k, f, nv, nf, stream))
            extra = {}
            mesh_vertices = int(counts[0])  # of the mesh the normals are of
            if cluster_cells and counts[2] == 0:
                check(L.vh_mesh_weld_accum_cluster(h, int(cluster_cells), int(cluster_scale_log2), stream), "vh_mesh_weld_accum_cluster")
                kc = (C.c_uint32 * 6)()
                ccode = L.vh_mesh_weld_accum_cluster_get_counts(h, kc, stream)
                _check_weld(ccode, raise_on_status, f"vh_mesh_weld_accum_cluster (status {kc[2]})")
                extra.update(cluster_counts=_counts_by_name(T.CLUSTER_COUNTS, kc), cluster_code=int(ccode))
                if ccode == 0:
                    extra["clustered"] = _welded_arrays(kc[0], kc[1], "vh_mesh_weld_accum_cluster_download",
                                                        lambda v, k, f, nv, nf: L.vh_mesh_weld_accum_cluster_download(h, v, k, f, nv, nf, stream))
                    mesh_vertices = int(kc[0])
                extra.update(stale_code(append_after_cluster, "stale_cluster_code", lambda: L.vh_mesh_weld_accum_cluster_get_counts(h, kc, stream)))
            if smooth_iterations and counts[2] == 0:
                check(L.vh_mesh_weld_accum_smooth(h, int(smooth_iterations), T.smooth_factor_q16(smooth_lambda), T.smooth_factor_q16(smooth_mu), 1 if keep_boundary else 0,
                                                  int(smooth_scale_log2), stream), "vh_mesh_weld_accum_smooth")
                sc = (C.c_uint32 * 6)()
                scode = L.vh_mesh_weld_accum_smooth_get_counts(h, sc, stream)
                _check_weld(scode, raise_on_status, f"vh_mesh_weld_accum_smooth (status {sc[3]})")
                extra.update(smooth_counts=_counts_by_name(T.SMOOTH_COUNTS, sc), smooth_code=int(scode))
                if scode == 0:
                    base = extra.get("clustered", out)
                    sv = np.zeros(mesh_vertices, dtype=T.VERTEX_DTYPE)
                    check(L.vh_mesh_weld_accum_smooth_download(h, sv.ctypes.data, mesh_vertices, stream), "vh_mesh_weld_accum_smooth_download")
                    extra["smoothed"] = dict(_vertex_arrays(sv), keys=base["keys"], faces=base["faces"])
                extra.update(stale_code(append_after_smooth, "stale_smooth_code", lambda: L.vh_mesh_weld_accum_smooth_get_counts(h, sc, stream)))
            if normals_scale_log2 is not None and counts[2] == 0:
                check(L.vh_mesh_weld_accum_normals(h, int(normals_scale_log2), stream), "vh_mesh_weld_accum_normals")
                nrm = np.zeros((mesh_vertices, 3), dtype=np.float32)
                ncode = L.vh_mesh_weld_accum_download_normals(h, nrm.ctypes.data, len(nrm), stream)
                _check_weld(ncode, raise_on_status, "vh_mesh_weld_accum_download_normals")
                extra.update(normals=nrm, normals_code=int(ncode))
            if (min_component_faces or largest_component) and counts[2] == 0:
                check(L.vh_mesh_weld_accum_components(h, int(min_component_faces), 1 if largest_component else 0, stream), "vh_mesh_weld_accum_components")
                cc = (C.c_uint32 * 6)()
                check(L.vh_mesh_weld_accum_components_get_counts(h, cc, stream), "vh_mesh_weld_accum_components_get_counts")
                with_n = "normals" in extra and extra["normals_code"] == 0
                fn = np.zeros((int(cc[3]), 3), dtype=np.float32)
                filtered = _welded_arrays(cc[3], cc[4], "vh_mesh_weld_accum_components_download",
                                          lambda v, k, f, nv, nf: L.vh_mesh_weld_accum_components_download(h, v, k, fn.ctypes.data if with_n else None, f, nv, nf, stream))
                if with_n:
                    filtered["normals"] = fn
                extra.update(filtered=filtered, component_counts=_counts_by_name(T.COMPONENTS_COUNTS, cc))
                extra.update(stale_code(append_after_components, "stale_code",
                                        lambda: L.vh_mesh_weld_accum_components_download(h, None, None, None, None, 0, 0, stream)))
        finally:
            L.vh_mesh_weld_accum_destroy(h)
    return dict(out, counts=(int(counts[0]), int(counts[1])), stats=_counts_by_name(T.WELD_ACCUM_COUNTS, counts), status=int(counts[2]), code=int(code), **extra)
