"""What the modules of the engine share, each written once: the lifetime of a handle behind the C ABI, out-parameters,
counts by name, block lists in device memory, and the device buffers of one driver call by name."""
import ctypes as C

import numpy as np

from .. import canonical
from .. import vhtypes as T
from ..lib import DeviceBuffer, check, download, load


def _copy_struct(s):
    out = type(s)()
    C.memmove(C.byref(out), C.byref(s), C.sizeof(s))
    return out


def _int3(v):
    return (C.c_int32 * 3)(*[int(x) for x in v])


def _unpack_rgb(packed):
    """r | g << 8 | b << 16 -> [n, 3] u8"""
    p = np.asarray(packed, dtype=np.uint32)
    return np.stack([p & 0xff, (p >> 8) & 0xff, (p >> 16) & 0xff], axis=-1).astype(np.uint8)


# Owner of one object behind the C ABI.  A subclass names its destroy function in `_destroy` and makes the object with
# `_create`; close() destroys it once, however often it is called, and __del__ closes without ever raising.  A create call
# that fails raises VhError and leaves `handle` unset, so that close() and __del__ then do nothing.  (Comments, not
# docstrings: a subclass without a docstring of its own would show this one's.)
class _Handle:
    _destroy = None
    handle = None

    def _create(self, create, *args):
        # self.L, then self.handle from L.<create>(*args, &handle)
        self.L = load()
        h = C.c_void_p()
        check(getattr(self.L, create)(*args, C.byref(h)), create)
        self.handle = h

    def close(self):
        if self.handle:
            getattr(self.L, self._destroy)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _struct_out(ctype, what, fn, *args):
    """fn(*args, &out), checked -> out, a `ctype`"""
    out = ctype()
    check(fn(*args, C.byref(out)), what)
    return out


def _scalar_out(ctype, what, fn, *args):
    return _struct_out(ctype, what, fn, *args).value


def _counts_by_name(names, counts):
    return {k: int(v) for k, v in zip(names, counts)}


def _counts_result(names, code, counts, what, extra=None):
    """the counts by name (a list of vhtypes: MERGE_COUNTS, CUT_COUNTS, DEINT_COUNTS) plus `extra`; with `what`, an
    error code raises VhError with .counts"""
    out = _counts_by_name(names, counts)
    out.update(extra or {})
    if what is not None and code != 0:
        try:
            check(code, what)
        except Exception as e:
            e.counts = out
            raise
    return out


# ---- block lists: descs (DESC_DTYPE [n]) and blocks (VOXEL_DTYPE [n, 512]) ---------------------------------------------

def _device_descs(descs, stream, n=None):
    """descs as a numpy array or a DeviceBuffer -> (descs in device memory, n); an empty list is a 16-byte dummy.
    n: how many count, where that is not all of them"""
    if isinstance(descs, DeviceBuffer):
        count = descs.nbytes // T.DESC_DTYPE.itemsize
    else:
        descs = np.ascontiguousarray(descs, dtype=T.DESC_DTYPE)
        count = len(descs)
        descs = DeviceBuffer.from_numpy(descs, stream) if count else DeviceBuffer(16)
    return descs, count if n is None else n


def _device_blocks(blocks, n, stream):
    """the n blocks of a list as a numpy array -> in device memory; an 8-byte dummy for none"""
    blocks = np.ascontiguousarray(blocks, dtype=T.VOXEL_DTYPE).reshape(n, T.SDF_BLOCK_VOXELS)
    return DeviceBuffer.from_numpy(blocks, stream) if n else DeviceBuffer(8)


def _staging_pair(room):
    """what a lift of up to `room` blocks writes: (the list, the pool) in device memory"""
    return DeviceBuffer(16 * max(room, 1)), DeviceBuffer(8 * T.SDF_BLOCK_VOXELS * max(room, 1))


def _staged_list(d_descs, d_blocks, n, stream, pool_blocks=None):
    """a lifted list read back: (descs DESC_DTYPE [n], voxels VOXEL_DTYPE [n, 512]), block i of the list at slot i; its
    voxels are at the desc's ptr in a pool of pool_blocks blocks (default n)"""
    if n == 0:
        return np.zeros(0, T.DESC_DTYPE), np.zeros((0, T.SDF_BLOCK_VOXELS), T.VOXEL_DTYPE)
    room = n if pool_blocks is None else pool_blocks
    descs = d_descs.download(T.DESC_DTYPE, n, stream)
    pool = d_blocks.download(T.VOXEL_DTYPE, room * T.SDF_BLOCK_VOXELS, stream).reshape(room, T.SDF_BLOCK_VOXELS)
    return descs, np.ascontiguousarray(pool[descs["ptr"] // T.SDF_BLOCK_VOXELS])


# ---- a scene's tables read back (test support) ------------------------------------------------------------------------

def _download_tables(hd, hp, s, with_voxels):
    """-> dict with the raw tables (params, hash, heap, heap_counter, bucket_count, bucket_bits, optionally sdf_blocks)"""
    out = dict(
        params=hp,
        hash=download(hd.d_hash, T.HASH_ENTRY_DTYPE, hp.m_hashNumBuckets * T.HASH_BUCKET_SIZE, s),
        heap=download(hd.d_heap, np.uint32, hp.m_numSDFBlocks, s),
        heap_counter=int(download(hd.d_heapCounter, np.uint32, 1, s)[0]),
        bucket_count=download(hd.d_bucketCount, np.uint32, hp.m_hashNumBuckets, s),
        bucket_bits=download(hd.d_bucketBits, np.uint32, (hp.m_hashNumBuckets + 31) // 32, s),
    )
    if with_voxels:
        out["sdf_blocks"] = download(hd.d_SDFBlocks, T.VOXEL_DTYPE, hp.m_numSDFBlocks * T.SDF_BLOCK_VOXELS, s)
    return out


def _canonical_state(d, hp, with_voxels, check_invariants=True):
    """the canonical snapshot (voxelhashing_amd.canonical) of downloaded tables `d`, with their compactified list and
    decisions, after the invariant checks"""
    if check_invariants:
        canonical.check_invariants(d["hash"], d["heap"], d["heap_counter"], hp, d.get("sdf_blocks"))
        canonical.check_bucket_summary(d["hash"], d["bucket_count"], d["bucket_bits"], hp)
    snap = canonical.snapshot(d["hash"], d.get("sdf_blocks"), d["heap"], d["heap_counter"], hp, with_voxels)
    snap.update(compactified=d["compactified"], decisions=d["decisions"])
    return snap


class _Buffers:
    """The device buffers of one driver call, by name: `with _Buffers(stream) as b:` frees every one of them on the way
    out, also when the body raises."""

    def __init__(self, stream=None):
        self.stream = stream
        self._by_name = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self._by_name.values():
            b.free()
        self._by_name = {}

    def _add(self, name, buf):
        if name in self._by_name:
            buf.free()
            raise KeyError(f"a buffer named {name} is there already")
        self._by_name[name] = buf
        return buf

    def upload(self, name, a):
        return self._add(name, DeviceBuffer.from_numpy(a, self.stream))

    def alloc(self, name, nbytes, fill=None):
        """nbytes of device memory; fill: a 32-bit pattern for every word of it"""
        if fill is None:
            return self._add(name, DeviceBuffer(nbytes))
        return self.upload(name, np.full(nbytes // 4, fill, dtype=np.uint32))

    def __getitem__(self, name):
        return self._by_name[name]

    def download(self, name, dtype, count=None):
        return self._by_name[name].download(dtype, count, self.stream)
