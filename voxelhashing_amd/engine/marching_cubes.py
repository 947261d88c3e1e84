"""CUDAMarchingCubesHashSDF (DSC/CUDAMarchingCubesHashSDF.h) with its indexed and live extractions, and the live mesh
at launcher level."""
import ctypes as C

import numpy as np

from .. import vhtypes as T
from ..lib import check, f16, load
from ._common import _Buffers, _Handle, _copy_struct, _counts_by_name, _scalar_out
from .mesh import _welded_arrays


def _live_counts(code, out, raise_on_status, what):
    """what an update of a live mesh returned (the eight counts, then the status word) -> the counts by name, status and
    code; a code raises VhError if asked to, and a code without a status always"""
    if code != 0 and (raise_on_status or out[8] == 0):
        check(code, what)
    return dict(_counts_by_name(T.LIVE_COUNTS, out), status=int(out[8]), code=int(code))


class CUDAMarchingCubesHashSDF(_Handle):
    """Mirror of DSC/CUDAMarchingCubesHashSDF.h:8-67 over the C ABI."""

    _destroy = "vh_marching_cubes_destroy"

    def __init__(self, params, stream=None):
        self._params = params
        self.stream = stream
        self._create("vh_marching_cubes_create", C.byref(params), stream)
        self._indexed_normals = False

    def _stats(self, words, names, fn, what):
        """the `words` words that fn(handle, out) fills -- the C function writes that many, whatever the names say -- by name"""
        assert len(names) == words
        out = (C.c_uint32 * words)()
        check(fn(self.handle, out), what)
        return _counts_by_name(names, out)

    def setOfflineProcessing(self, on):
        check(self.L.vh_marching_cubes_set_offline_processing(self.handle, 1 if on else 0), "setOfflineProcessing")

    def setIndexedNormals(self, on):
        """vertex normals for the indexed extractions (off by default): computed on the device after the weld; indexed()
        and mesh() then have a "normals" entry and saveMesh writes nx, ny, nz"""
        check(self.L.vh_marching_cubes_set_indexed_normals(self.handle, 1 if on else 0), "setIndexedNormals")
        self._indexed_normals = bool(on)

    def setIndexedComponentFilter(self, minFaces=0, largestOnly=False):
        """the component filter for the indexed extractions (off by default: 0, False): after the weld and the normals
        the mesh's connected components are labelled on the device and those of fewer than minFaces faces dropped, with
        largestOnly all but the largest; indexed_counts(), indexed(), mesh() and saveMesh then describe the filtered
        mesh, and indexed_component_stats() says what the unfiltered one held"""
        check(self.L.vh_marching_cubes_set_indexed_component_filter(self.handle, int(minFaces), 1 if largestOnly else 0), "setIndexedComponentFilter")

    def setIndexedClustering(self, cellsPerCluster=0):
        """decimation by vertex clustering for the indexed extractions (off by default: 0; 1 ... 64 turn it on): after
        the weld, and before normals and components, the vertices that fall into one cube of cellsPerCluster lattice
        points a side become one vertex at their mean; indexed_counts(), indexed(), mesh() and saveMesh then describe the
        clustered mesh, and indexed_cluster_stats() says what the pass did"""
        check(self.L.vh_marching_cubes_set_indexed_clustering(self.handle, int(cellsPerCluster)), "setIndexedClustering")

    def indexed_cluster_stats(self):
        """of the last indexed extraction: vertices, faces, status, collapsed, duplicates, unused_clusters; all 0 when
        it ran with clustering off"""
        return self._stats(6, T.CLUSTER_COUNTS, self.L.vh_marching_cubes_get_indexed_cluster_stats, "get_indexed_cluster_stats")

    def setIndexedSmoothing(self, iterations=0, lam=0.5, mu=-0.53, keepBoundary=True):
        """Taubin smoothing for the indexed extractions (off by default: 0; 1 ... 100 iterations turn it on): after the
        clustering, and before normals and components, the positions are replaced by that many lambda | mu iterations
        in fixed point; indexed(), mesh() and saveMesh then carry the smoothed positions, and indexed_smooth_stats()
        says what the pass did.  The factors go to units of 2^-16 by rint; ValueError above 1 in magnitude"""
        check(self.L.vh_marching_cubes_set_indexed_smoothing(self.handle, int(iterations), T.smooth_factor_q16(lam), T.smooth_factor_q16(mu), 1 if keepBoundary else 0),
              "setIndexedSmoothing")

    def indexed_smooth_stats(self):
        """of the last indexed extraction: moved, boundary_vertices, isolated_vertices, status, edges, boundary_edges;
        all 0 when it ran with smoothing off"""
        return self._stats(6, T.SMOOTH_COUNTS, self.L.vh_marching_cubes_get_indexed_smooth_stats, "get_indexed_smooth_stats")

    def indexed_component_stats(self):
        """of the last indexed extraction: components (with a face), faceless_vertices, kept_components, kept_vertices,
        kept_faces, largest_faces; all 0 when it ran with the filter off"""
        return self._stats(6, T.COMPONENTS_COUNTS, self.L.vh_marching_cubes_get_indexed_component_stats, "get_indexed_component_stats")

    def extractIsoSurface(self, hashData, hashParams, minCorner=(0, 0, 0), maxCorner=(0, 0, 0), boxEnabled=False, copy=True):
        check(self.L.vh_marching_cubes_extract_iso_surface(self.handle, C.byref(hashData), C.byref(hashParams), f16(minCorner),
                                                           f16(maxCorner), int(boxEnabled), int(copy)), "extractIsoSurface")

    def extractIsoSurfaceWithoutCopy(self, hashData, hashParams, minCorner=(0, 0, 0), maxCorner=(0, 0, 0), boxEnabled=False):
        self.extractIsoSurface(hashData, hashParams, minCorner, maxCorner, boxEnabled, copy=False)

    def extractIsoSurfaceChunkGrid(self, chunkGrid, camPos, radius):
        check(self.L.vh_marching_cubes_extract_iso_surface_chunk_grid(self.handle, chunkGrid.handle, f16(camPos), radius),
              "extractIsoSurface(chunkGrid)")

    def extractIsoSurfaceIndexed(self, hashData, hashParams, minCorner=(0, 0, 0), maxCorner=(0, 0, 0), boxEnabled=False):
        """the extraction with the soup welded on the device: REPLACES the mesh buffer with the indexed mesh (mesh(),
        saveMesh write it as it is); indexed() has it with the keys, sources() the records it was welded by"""
        check(self.L.vh_marching_cubes_extract_iso_surface_indexed(self.handle, C.byref(hashData), C.byref(hashParams), f16(minCorner),
                                                                   f16(maxCorner), int(boxEnabled)), "extractIsoSurfaceIndexed")

    def beginIndexed(self):
        """starts an indexed extraction that is made box by box: appendIndexed any number of times, then finishIndexed"""
        check(self.L.vh_marching_cubes_begin_indexed(self.handle), "beginIndexed")

    def appendIndexed(self, hashData, hashParams, minCorner=(0, 0, 0), maxCorner=(0, 0, 0), boxEnabled=False):
        """one extraction in a box, appended to the accumulation; boxes may overlap: a cell is taken from the first box
        that has it"""
        check(self.L.vh_marching_cubes_append_indexed(self.handle, C.byref(hashData), C.byref(hashParams), f16(minCorner), f16(maxCorner),
                                                      int(boxEnabled)), "appendIndexed")

    def finishIndexed(self):
        """downloads the accumulated mesh and REPLACES the mesh buffer with it, as extractIsoSurfaceIndexed does"""
        check(self.L.vh_marching_cubes_finish_indexed(self.handle), "finishIndexed")

    def extractIsoSurfaceIndexedChunkGrid(self, chunkGrid, camPos, radius):
        """the walk of extractIsoSurfaceChunkGrid with every chunk appended to one accumulation: the indexed mesh of a
        streamed scene"""
        check(self.L.vh_marching_cubes_extract_iso_surface_indexed_chunk_grid(self.handle, chunkGrid.handle, f16(camPos), radius),
              "extractIsoSurfaceIndexed(chunkGrid)")

    def liveBegin(self):
        """starts a live mesh: until liveEnd the object's triangles() and sources() are a cache that liveUpdate brings
        up to date with the table, and every extraction on the object raises VhError (VH_ERR_BAD_ARGUMENT)"""
        check(self.L.vh_marching_cubes_live_begin(self.handle), "liveBegin")

    def liveUpdate(self, hashData, hashParams, boxEnabled=False, raise_on_status=True):
        """one update of the live mesh: re-extracts the resident blocks within one block of a block that changed since
        the last update -> the counts of T.LIVE_COUNTS and `status`.  An overflow or a block out of range raises VhError
        and leaves the cache invalid (the next update is a full one); with raise_on_status=False it comes back as `code`"""
        out = (C.c_uint32 * 9)()
        code = self.L.vh_marching_cubes_live_update(self.handle, C.byref(hashData), C.byref(hashParams), int(boxEnabled), out)
        return _live_counts(code, out, raise_on_status, "liveUpdate")

    def liveInvalidate(self):
        """forgets every record and the cache: the next liveUpdate is a full extraction (the digests can collide)"""
        check(self.L.vh_marching_cubes_live_invalidate(self.handle), "liveInvalidate")

    def liveIndexed(self):
        """welds the cache and runs the indexed passes that are on: REPLACES the mesh buffer as extractIsoSurfaceIndexed
        does (indexed(), mesh(), saveMesh); the cache stays"""
        check(self.L.vh_marching_cubes_live_indexed(self.handle), "liveIndexed")

    def liveEnd(self):
        check(self.L.vh_marching_cubes_live_end(self.handle), "liveEnd")

    def indexed_stats(self):
        """of the last accumulated extraction: vertices, faces, status, cells, dropped (triangles of cells an earlier
        append had), rehashes (doublings of the table); all 0 after a one-shot extraction"""
        return self._stats(6, T.WELD_ACCUM_COUNTS, self.L.vh_marching_cubes_get_indexed_stats, "get_indexed_stats")

    def indexed_counts(self):
        return self._stats(3, ("vertices", "faces", "status"), self.L.vh_marching_cubes_get_indexed_counts, "get_indexed_counts")

    def indexed(self):
        """device mesh of the last indexed extraction -> vertices (V,3) f32, colors (V,3) f32, keys (V,) u64, faces (F,3) u32;
        with setIndexedNormals(True), and an extraction made since, also normals (V,3) f32"""
        n = self.indexed_counts()
        out = _welded_arrays(n["vertices"], n["faces"], "download_indexed",
                             lambda v, k, f, nv, nf: self.L.vh_marching_cubes_download_indexed(self.handle, v, k, f))
        if self._indexed_normals:
            out["normals"] = np.zeros((n["vertices"], 3), dtype=np.float32)
            check(self.L.vh_marching_cubes_download_indexed_normals(self.handle, out["normals"].ctypes.data), "download_indexed_normals")
        return out

    def _soup_part(self, dtype, fn, what):
        """the triangles the last extraction counted, as far as the buffer holds them, filled by fn(handle, out, n)"""
        n = min(self.counts()["triangles"], self._params.m_maxNumTriangles)
        out = np.zeros(n, dtype=dtype)
        if n:
            check(fn(self.handle, out.ctypes.data, n), what)
        return out

    def sources(self):
        """source records of the last indexed extraction, beside triangles() -> numpy array of T.TRIANGLE_SOURCE_DTYPE"""
        return self._soup_part(T.TRIANGLE_SOURCE_DTYPE, self.L.vh_marching_cubes_download_sources, "download_sources")

    def copyTrianglesToCPU(self):
        check(self.L.vh_marching_cubes_copy_triangles_to_cpu(self.handle), "copyTrianglesToCPU")

    def clearMeshBuffer(self):
        check(self.L.vh_marching_cubes_clear_mesh_buffer(self.handle), "clearMeshBuffer")

    def counts(self):
        return self._stats(2, ("triangles", "occupied_blocks"), self.L.vh_marching_cubes_get_counts, "get_counts")

    def triangles(self):
        """device triangle buffer of the last extraction -> numpy array of T.TRIANGLE_DTYPE"""
        return self._soup_part(T.TRIANGLE_DTYPE, self.L.vh_marching_cubes_download_triangles, "download_triangles")

    def mesh(self):
        sz = (C.c_uint64 * 2)()
        check(self.L.vh_marching_cubes_get_mesh_size(self.handle, sz), "get_mesh_size")
        v = np.zeros((int(sz[0]), 3), dtype=np.float32)
        c = np.zeros((int(sz[0]), 4), dtype=np.float32)
        f = np.zeros(int(sz[1]), dtype=np.uint32)
        check(self.L.vh_marching_cubes_get_mesh(self.handle, v.ctypes.data, c.ctypes.data, f.ctypes.data), "get_mesh")
        out = dict(vertices=v, colors=c, faces=f.reshape(-1, 3))
        if self._indexed_normals:  # (3 per vertex, or none: whatever appended to the buffer since has dropped them)
            nn = _scalar_out(C.c_uint64, "get_mesh_normals_size", self.L.vh_marching_cubes_get_mesh_normals_size, self.handle)
            out["normals"] = np.zeros((int(nn) // 3, 3), dtype=np.float32)
            check(self.L.vh_marching_cubes_get_mesh_normals(self.handle, out["normals"].ctypes.data), "get_mesh_normals")
        return out

    def saveMesh(self, filename, transform=None, overwriteExistingFile=False):
        t = f16(transform) if transform is not None else None
        check(self.L.vh_marching_cubes_save_mesh(self.handle, filename.encode(), t, int(overwriteExistingFile)), "saveMesh")


def live_mesh_digest(hashData, hashParams, entry_indices, stream=None):
    """vh_live_mesh_digest: the 64-bit digests of the blocks of the listed hash entries (0 for a free entry) -> (n,) u64"""
    idx = np.ascontiguousarray(entry_indices, dtype=np.uint32).ravel()
    if len(idx) == 0:
        return np.zeros(0, dtype=np.uint64)
    with _Buffers(stream) as dev:
        dev.upload("entries", idx)
        dev.alloc("digests", 8 * len(idx))
        check(load().vh_live_mesh_digest(C.byref(hashData), C.byref(hashParams), dev["entries"].ptr, len(idx), dev["digests"].ptr, stream), "vh_live_mesh_digest")
        return dev.download("digests", np.uint64, len(idx))


class LiveMesh(_Handle):
    """The live mesh at launcher level: vh_live_mesh_* over buffers of its own (vh_marching_cubes_data_alloc, the source
    records, vh_live_mesh_data_alloc).  params: T.MarchingCubesParams with the box off."""

    def __init__(self, params, numSDFBlocks, stream=None):
        self.L = load()
        self.stream = stream
        self._params = _copy_struct(params)
        self._params.m_boxEnabled = 0
        self.data, self.live, self.d_sources = T.MarchingCubesData(), T.LiveMeshData(), C.c_void_p()
        check(self.L.vh_marching_cubes_data_alloc(C.byref(self.data), C.byref(self._params)), "vh_marching_cubes_data_alloc")
        check(self.L.vh_reset_marching_cubes(C.byref(self.data), stream), "vh_reset_marching_cubes")
        check(self.L.vh_malloc(C.byref(self.d_sources), 16 * int(self._params.m_maxNumTriangles)), "vh_malloc")
        check(self.L.vh_live_mesh_data_alloc(C.byref(self.live), int(numSDFBlocks), int(self._params.m_maxNumTriangles)), "vh_live_mesh_data_alloc")

    def close(self):
        if getattr(self, "live", None) is not None:
            self.L.vh_live_mesh_data_free(C.byref(self.live))
            self.L.vh_marching_cubes_data_free(C.byref(self.data))
            self.L.vh_free(self.d_sources)
            self.live = None

    def reset(self):
        check(self.L.vh_live_mesh_reset(C.byref(self.live), self.stream), "vh_live_mesh_reset")
        check(self.L.vh_reset_marching_cubes(C.byref(self.data), self.stream), "vh_reset_marching_cubes")

    def enqueue(self, hashData, hashParams):
        """vh_live_mesh_update alone: the counts are read by counts()"""
        check(self.L.vh_live_mesh_update(C.byref(hashData), C.byref(hashParams), C.byref(self.data), C.byref(self.d_sources), C.byref(self.live), self.stream),
              "vh_live_mesh_update")

    def counts(self, raise_on_status=True):
        out = (C.c_uint32 * 9)()
        code = self.L.vh_live_mesh_get_counts(C.byref(self.live), out, self.stream)
        return _live_counts(code, out, raise_on_status, "vh_live_mesh_get_counts")

    def update(self, hashData, hashParams, raise_on_status=True):
        self.enqueue(hashData, hashParams)
        return self.counts(raise_on_status)

    def soup(self, n):
        """the first n triangles of the cache and their records (n: the last update's total)"""
        tris, srcs = np.zeros(int(n), dtype=T.TRIANGLE_DTYPE), np.zeros(int(n), dtype=T.TRIANGLE_SOURCE_DTYPE)
        if n:
            check(self.L.vh_memcpy_d2h(tris.ctypes.data, self.data.d_triangles, tris.nbytes, self.stream), "vh_memcpy_d2h")
            check(self.L.vh_memcpy_d2h(srcs.ctypes.data, self.d_sources, srcs.nbytes, self.stream), "vh_memcpy_d2h")
        return tris, srcs

    def records(self):
        out = np.zeros(int(self.live.m_numSDFBlocks), dtype=T.LIVE_RECORD_DTYPE)
        check(self.L.vh_memcpy_d2h(out.ctypes.data, self.live.d_records, out.nbytes, self.stream), "vh_memcpy_d2h")
        return out
