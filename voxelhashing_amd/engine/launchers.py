"""LauncherScene: a hash table of its own under the launcher-level C ABI, one call per kernel, for the tests that pin
each launcher on its own."""
import ctypes as C

import numpy as np

from .. import vhtypes as T
from ..lib import DeviceBuffer, check, download, f16, load
from ._common import (_Handle, _canonical_state, _copy_struct, _counts_by_name, _counts_result, _device_blocks, _device_descs, _download_tables, _int3,
                      _staged_list, _staging_pair)
from .scene import _merge_result, _merge_upload


class LauncherScene(_Handle):
    """HashData + the launcher-level C ABI (the twins of the reference's
    extern "C" launchers, DepthSensingCUDA/Source/CUDASceneRepHashSDF.h:15-26 and
    CUDASceneRepChunkGrid.h:142-146), one call per kernel, for tests that pin
    each launcher on its own."""

    def __init__(self, params, stream=None):
        self.L = load()
        self.stream = stream
        self.hp = _copy_struct(params)
        self.hd = T.HashData()
        check(self.L.vh_hash_data_alloc(C.byref(self.hd), C.byref(self.hp)), "vh_hash_data_alloc")
        self.reset()

    def close(self):
        if getattr(self, "hd", None) is not None and self.hd.d_hash:
            self.L.vh_stream_synchronize(self.stream)
            self.L.vh_hash_data_free(C.byref(self.hd))

    def set_transform(self, transform, inverse):
        self.hp.m_rigidTransform = T.mat16(transform)
        self.hp.m_rigidTransformInverse = T.mat16(inverse)

    def reset(self):
        check(self.L.vh_reset(C.byref(self.hd), C.byref(self.hp), self.stream), "vh_reset")

    def reset_mutex(self):
        check(self.L.vh_reset_bucket_mutex(C.byref(self.hd), C.byref(self.hp), self.stream), "vh_reset_bucket_mutex")

    def alloc(self, frame, cp, bitmask_ptr=None, lock_token=T.LOCK_ENTRY):
        check(self.L.vh_alloc(C.byref(self.hd), C.byref(self.hp), C.byref(frame.data), C.byref(cp), bitmask_ptr, lock_token, self.stream), "vh_alloc")

    def compactify(self, cp):
        n = C.c_uint32()
        check(self.L.vh_compactify(C.byref(self.hd), C.byref(self.hp), C.byref(cp), C.byref(n), 0, self.stream), "vh_compactify")
        self.hp.m_numOccupiedBlocks = n.value
        return n.value

    def integrate(self, frame, cp):
        check(self.L.vh_integrate(C.byref(self.hd), C.byref(self.hp), C.byref(frame.data), C.byref(cp), self.stream), "vh_integrate")

    def integrate_fused(self, frame, cp, flags, lock_token, packed_ptr=None):
        check(self.L.vh_integrate_fused(C.byref(self.hd), C.byref(self.hp), C.byref(frame.data), C.byref(cp), flags, lock_token, None, 0,
                                        packed_ptr, self.stream), "vh_integrate_fused")

    def frame_job(self, frame, cp, bitmask_ptr=None, lock_token=T.LOCK_ENTRY, packed_ptr=None):
        """the alloc + compactify passes of a frame as a VhFrameJob (vh_alloc_job / vh_compactify_job / the co-launches)"""
        job = T.FrameJob()
        C.memmove(C.byref(job.hashData), C.byref(self.hd), C.sizeof(self.hd))
        C.memmove(C.byref(job.hashParams), C.byref(self.hp), C.sizeof(self.hp))
        C.memmove(C.byref(job.cam), C.byref(frame.data), C.sizeof(frame.data))
        C.memmove(C.byref(job.cp), C.byref(cp), C.sizeof(cp))
        job.d_bitMask = bitmask_ptr
        job.d_packedFrame = packed_ptr
        job.lockToken = lock_token
        return job

    def alloc_job(self, job):
        check(self.L.vh_alloc_job(C.byref(job), self.stream), "vh_alloc_job")

    def compactify_job(self, job):
        check(self.L.vh_compactify_job(C.byref(job), self.stream), "vh_compactify_job")

    def starve(self):
        check(self.L.vh_starve(C.byref(self.hd), C.byref(self.hp), self.stream), "vh_starve")

    def gc_identify(self, cp):
        check(self.L.vh_gc_identify(C.byref(self.hd), C.byref(self.hp), C.byref(cp), self.stream), "vh_gc_identify")

    def gc_free(self, lock_token=T.LOCK_ENTRY):
        check(self.L.vh_gc_free(C.byref(self.hd), C.byref(self.hp), lock_token, self.stream), "vh_gc_free")

    def hash_ops(self, ops):
        """ops: [n,5] int32 {op, x, y, z, arg} executed serially by one thread -> results[n]"""
        ops = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1, 5)
        d_ops = DeviceBuffer.from_numpy(ops, self.stream)
        d_res = DeviceBuffer(4 * len(ops))
        check(self.L.vh_debug_hash_ops(C.byref(self.hd), C.byref(self.hp), d_ops.ptr, d_res.ptr, len(ops), self.stream), "vh_debug_hash_ops")
        return d_res.download(np.int32, len(ops), self.stream)

    def stream_out(self, threads_per_part, start, radius, cam_pos, lock_token, capacity=4096):
        """pass 1 + pass 2 -> (descs, blocks)"""
        cnt = DeviceBuffer(4)
        check(self.L.vh_memset(cnt.ptr, 0, 4, self.stream), "memset")
        d_desc = DeviceBuffer(16 * capacity)
        check(self.L.vh_stream_out_pass1(C.byref(self.hd), C.byref(self.hp), threads_per_part, start, C.c_float(radius), f16(cam_pos),
                                         cnt.ptr, d_desc.ptr, capacity, lock_token, self.stream), "vh_stream_out_pass1")
        n = int(cnt.download(np.uint32, 1, self.stream)[0])
        assert n <= capacity
        d_blocks = DeviceBuffer(4096 * max(n, 1))
        check(self.L.vh_stream_out_pass2(C.byref(self.hd), C.byref(self.hp), d_desc.ptr, d_blocks.ptr, n, self.stream), "vh_stream_out_pass2")
        descs = d_desc.download(T.DESC_DTYPE, n, self.stream)
        blocks = d_blocks.download(T.VOXEL_DTYPE, n * T.SDF_BLOCK_VOXELS, self.stream).reshape(n, T.SDF_BLOCK_VOXELS)
        return descs, blocks

    def stream_in(self, descs, blocks, lock_token):
        descs = np.ascontiguousarray(descs, dtype=T.DESC_DTYPE)
        blocks = np.ascontiguousarray(blocks, dtype=T.VOXEL_DTYPE)
        n = len(descs)
        if n == 0:
            return
        d_desc, d_blocks = DeviceBuffer.from_numpy(descs, self.stream), DeviceBuffer.from_numpy(blocks, self.stream)
        prev = int(download(self.hd.d_heapCounter, np.uint32, 1, self.stream)[0])
        check(self.L.vh_stream_in_pass1(C.byref(self.hd), C.byref(self.hp), n, prev, d_desc.ptr, lock_token, self.stream), "vh_stream_in_pass1")
        check(self.L.vh_stream_in_pass2(C.byref(self.hd), C.byref(self.hp), n, prev, d_desc.ptr, d_blocks.ptr, self.stream), "vh_stream_in_pass2")
        new = np.array([prev - n], dtype=np.uint32)
        check(self.L.vh_memcpy_h2d(self.hd.d_heapCounter, new.ctypes.data, 4, self.stream), "heapCounter")

    def stream_in_settled(self, descs, blocks, lock_token):
        """vh_stream_in_device: the pass that reads the heap counter on the device and settles itself -- a block that
        finds no slot keeps no voxels and its SDF block is back on the heap when the call returns
        -> (indices into descs of the blocks that found no slot, whether the heap held too few free blocks)"""
        descs = np.ascontiguousarray(descs, dtype=T.DESC_DTYPE)
        blocks = np.ascontiguousarray(blocks, dtype=T.VOXEL_DTYPE)
        n = len(descs)
        d_desc, d_blocks = DeviceBuffer.from_numpy(descs, self.stream), DeviceBuffer.from_numpy(blocks, self.stream)
        d_failed, d_out = DeviceBuffer(4 * (1 + 2 * n)), DeviceBuffer(4 * (4 + n))
        check(self.L.vh_memset(d_failed.ptr, 0, d_failed.nbytes, self.stream), "memset")
        check(self.L.vh_memset(d_out.ptr, 0, d_out.nbytes, self.stream), "memset")
        check(self.L.vh_stream_in_device(C.byref(self.hd), C.byref(self.hp), n, d_desc.ptr, d_blocks.ptr, lock_token, d_failed.ptr, None, 0xFFFFFFFF,
                                         d_out.ptr, 1, self.stream), "vh_stream_in_device")
        out = d_out.download(np.uint32, 4 + n, self.stream)
        if out[2] != 1 or d_failed.download(np.uint32, 1 + 2 * n, self.stream)[0] != 0:
            raise RuntimeError("vh_stream_in_device: the pass did not settle (no tag published, or the scratch words were not cleared)")
        return out[4:4 + int(out[0])].astype(np.int64), bool(out[3])

    def merge_gather(self):
        """vh_merge_gather -> (descs in device memory, n): every occupied entry of this table as {pos, ptr}"""
        cap = int(self.hp.m_numSDFBlocks)
        d_desc, cnt = DeviceBuffer(16 * cap), DeviceBuffer(4)
        check(self.L.vh_merge_gather(C.byref(self.hd), C.byref(self.hp), d_desc.ptr, cap, cnt.ptr, self.stream), "vh_merge_gather")
        return d_desc, int(cnt.download(np.uint32, 1, self.stream)[0])

    def merge_blocks(self, descs, blocks, lock_token, block_offset=(0, 0, 0), source=None, n=None):
        """vh_merge_blocks: descs / blocks as numpy arrays (or DeviceBuffers); with source (a LauncherScene) the voxels
        are read from that scene's pool at descs' ptr and blocks is ignored (n: how many of a DeviceBuffer's descs count) -> the counts by name plus left_out_indices
        (the status is in the counts: nothing raises for it)"""
        off = _int3(block_offset)
        if source is not None:
            (d_desc, n), d_blocks = _device_descs(descs, self.stream, n), None
        else:
            d_desc, d_blocks, n = _merge_upload(descs, blocks, self.stream)
        d_work = DeviceBuffer(self.L.vh_merge_work_bytes(n))
        d_left = DeviceBuffer(4 * max(n, 1))
        counts = (C.c_uint32 * len(T.MERGE_COUNTS))()
        check(self.L.vh_merge_blocks(C.byref(self.hd), C.byref(self.hp), n, d_desc.ptr, d_blocks.ptr if d_blocks is not None else None,
                                     source.hd.d_SDFBlocks if source is not None else None, off, lock_token, d_work.ptr, d_left.ptr, counts, self.stream),
              "vh_merge_blocks")
        return _merge_result(0, counts, "vh_merge_blocks", d_left, self.stream)

    def cut_blocks(self, region_from_vox, shape, flags, lock_token, descs=None, blocks=None, staging_blocks=None, poison=None):
        """vh_cut_blocks on this table's entries (vh_merge_gather) or, with descs / blocks (numpy arrays, VH_CUT_KEEP
        only), on a plain block list.  region_from_vox: float32 [3, 4] (cut_region_transform).  A lifting call counts
        first and sizes the staging pool by the count unless staging_blocks says otherwise; poison: a byte the staging
        pool and its list are filled with before.  -> the counts by name (vhtypes.CUT_COUNTS) plus "code" (the call's
        return code: nothing raises), "descs" / "voxels" (the lifted list; empty unless the call lifted) and
        "staging_raw" (the list's and the pool's bytes after the call, or None)"""
        m = np.ascontiguousarray(region_from_vox, dtype=np.float32).reshape(12)
        d_desc, n = self.merge_gather() if descs is None else _device_descs(descs, self.stream)
        d_blocks = None if descs is None else _device_blocks(blocks, n, self.stream)
        d_work = DeviceBuffer(self.L.vh_cut_work_bytes(n))
        counts = (C.c_uint32 * len(T.CUT_COUNTS))()

        def call(fl, d_out, d_staging, room):
            rc = self.L.vh_cut_blocks(C.byref(self.hd), C.byref(self.hp), n, d_desc.ptr, d_blocks.ptr if d_blocks is not None else None, m.ctypes.data,
                                      int(shape), int(fl), lock_token, d_work.ptr, d_out.ptr if d_out else None, d_staging.ptr if d_staging else None,
                                      room, counts, self.stream)
            return _counts_result(T.CUT_COUNTS, rc, counts, None, dict(code=rc, descs=np.zeros(0, T.DESC_DTYPE),
                                                                       voxels=np.zeros((0, T.SDF_BLOCK_VOXELS), T.VOXEL_DTYPE), staging_raw=None))

        if not (flags & T.CUT_LIFT) or (flags & T.CUT_COUNT_ONLY):
            return call(flags, None, None, 0)
        if staging_blocks is None:
            staging_blocks = call(flags | T.CUT_COUNT_ONLY, None, None, 0)["lifted"]
        room = int(staging_blocks)
        d_out, d_staging = _staging_pair(room)
        if poison is not None:
            check(self.L.vh_memset(d_out.ptr, int(poison), d_out.nbytes, self.stream), "memset")
            check(self.L.vh_memset(d_staging.ptr, int(poison), d_staging.nbytes, self.stream), "memset")
        out = call(flags, d_out, d_staging, room)
        out["staging_raw"] = (d_out.download(np.uint8, None, self.stream), d_staging.download(np.uint8, None, self.stream))
        if out["code"] == 0:
            out["descs"], out["voxels"] = _staged_list(d_out, d_staging, out["lifted"], self.stream)
        return out

    def deintegrate_blocks(self, frame, cp, transform, inverse, lock_token, flags=0):
        """vh_merge_gather on this table, then vh_deintegrate_blocks with the frame's pose and its inverse in a copy of the
        hash parameters -> the counts by name (vhtypes.DEINT_COUNTS) plus "code" (the call's return code: nothing raises)"""
        d_desc, n = self.merge_gather()
        hp = _copy_struct(self.hp)
        hp.m_rigidTransform = T.mat16(transform)
        hp.m_rigidTransformInverse = T.mat16(inverse)
        d_work = DeviceBuffer(self.L.vh_deintegrate_work_bytes(n))
        counts = (C.c_uint32 * len(T.DEINT_COUNTS))()
        rc = self.L.vh_deintegrate_blocks(C.byref(self.hd), C.byref(hp), n, d_desc.ptr, C.byref(frame.data), C.byref(cp), int(flags), lock_token, d_work.ptr,
                                          counts, self.stream)
        return _counts_result(T.DEINT_COUNTS, rc, counts, None, {"code": rc})

    def align_begin(self, source, guess, pivot, radius):
        """vh_align_begin for `source` (a LauncherScene) against this scene -> (the state in device memory, the ticket
        word, the call's return code)"""
        m = np.ascontiguousarray(guess, dtype=np.float64).reshape(16)
        p = np.ascontiguousarray(pivot, dtype=np.float32).reshape(3)
        d_state, d_ticket = DeviceBuffer(C.sizeof(T.AlignState)), DeviceBuffer(4)
        check(self.L.vh_memset(d_state.ptr, 0, d_state.nbytes, self.stream), "memset")
        check(self.L.vh_memset(d_ticket.ptr, 0, 4, self.stream), "memset")
        rc = self.L.vh_align_begin(d_state.ptr, m.ctypes.data, float(source.hp.m_virtualVoxelSize), float(self.hp.m_virtualVoxelSize), p.ctypes.data,
                                   float(radius), self.stream)
        return d_state, d_ticket, rc

    def align_state(self, d_state, d_ticket=None):
        """the state read back -> vhtypes.align_state_dict, with "ticket" where the word is given"""
        st = T.AlignState.from_buffer_copy(d_state.download(np.uint8, C.sizeof(T.AlignState), self.stream).tobytes())
        out = T.align_state_dict(st)
        out["stripes"] = np.array(st.stripes[:], np.int64)
        out["raised"] = int(st.raised)
        if d_ticket is not None:
            out["ticket"] = int(d_ticket.download(np.uint32, 1, self.stream)[0])
        return out

    def align_step(self, source, d_state, d_ticket, descs=None, n=None, band=2.0, min_count=200, cond_thres=1e4, rot_thres=1e-5, trans_thres=1e-3,
                   steps=1):
        """vh_align_step, `steps` launches back to back: `source`'s blocks (vh_merge_gather on it, or descs: a
        DESC_DTYPE array or a DeviceBuffer with n) against this scene -> (align_state afterwards, the last return code)"""
        d_desc, n = source.merge_gather() if descs is None else _device_descs(descs, self.stream, n if isinstance(descs, DeviceBuffer) else None)
        rc = 0
        for _ in range(steps):
            rc = self.L.vh_align_step(C.byref(self.hd), C.byref(self.hp), C.byref(source.hd), C.byref(source.hp), n, d_desc.ptr, float(band), int(min_count),
                                      float(cond_thres), float(rot_thres), float(trans_thres), d_state.ptr, d_ticket.ptr, self.stream)
        return self.align_state(d_state, d_ticket), rc

    def align_rule(self, source, dst_vox_from_src_vox, pivot, inv_radius, band=2.0, descs=None):
        """vh_debug_align_rule: the per-voxel rule on `source`'s blocks (descs: DESC_DTYPE with the blocks' ptr, default
        vh_merge_gather on it) against this scene -> dict descs, kept [n, 512] bool, q [n, 512, 3], e [n, 512],
        g [n, 512, 3], terms [n, 512, 29] (float32; all zero where not kept)"""
        b = np.ascontiguousarray(dst_vox_from_src_vox, dtype=np.float32).reshape(12)
        p = np.ascontiguousarray(pivot, dtype=np.float32).reshape(3)
        d_desc, n = source.merge_gather() if descs is None else _device_descs(descs, self.stream)
        W, V = T.ALIGN_RULE_WORDS, T.SDF_BLOCK_VOXELS
        d_out = DeviceBuffer(4 * W * V * max(n, 1))
        check(self.L.vh_debug_align_rule(C.byref(self.hd), C.byref(self.hp), C.byref(source.hd), C.byref(source.hp), n, d_desc.ptr, b.ctypes.data, p.ctypes.data,
                                         float(inv_radius), float(band), d_out.ptr, self.stream), "vh_debug_align_rule")
        rec = d_out.download(np.float32, W * V * n, self.stream).reshape(n, V, W)
        return dict(descs=d_desc.download(T.DESC_DTYPE, n, self.stream), kept=rec[:, :, 0].view(np.uint32) != 0, q=rec[:, :, 1:4], e=rec[:, :, 4],
                    g=rec[:, :, 5:8], terms=rec[:, :, 8:])

    def resample_blocks(self, src_vox_from_dst_vox, dst_vox_from_src_vox, slots_log2=None):
        """vh_merge_gather on this table, then vh_resample_blocks, count and fill: this scene sampled on another lattice
        (the matrices of resample_voxel_transforms) -> the counts by name (vhtypes.RESAMPLE_COUNTS) plus "descs"
        (DESC_DTYPE [staged], ptr = 512 * the block's place in the staging pool) and "voxels" (VOXEL_DTYPE [staged, 512],
        in the descs' order): a list for merge_blocks.  slots_log2: the candidate table's size (default: 16 slots per
        source block).  A status is in the counts, with nothing staged: nothing raises for it."""
        a = np.ascontiguousarray(src_vox_from_dst_vox, dtype=np.float32).reshape(12)
        b = np.ascontiguousarray(dst_vox_from_src_vox, dtype=np.float32).reshape(12)
        d_src, n = self.merge_gather()
        counts = (C.c_uint32 * len(T.RESAMPLE_COUNTS))()

        def call(d_out, d_staging, room):
            check(self.L.vh_resample_blocks(C.byref(self.hd), C.byref(self.hp), n, d_src.ptr, a.ctypes.data, b.ctypes.data, slots_log2, d_work.ptr,
                                            d_out.ptr if d_out else None, d_staging.ptr if d_staging else None, room, counts, self.stream), "vh_resample_blocks")
            return _counts_by_name(T.RESAMPLE_COUNTS, counts)

        # without a size: as mergeSceneTransformed, 16 slots per source block, four times as many while the table fills, up
        # to two for each of the 6^3 candidates a source block can name
        grow = slots_log2 is None
        most = max(4, int(2 * 216 * max(n, 1) - 1).bit_length())
        if grow:
            slots_log2 = min(most, max(4, int(16 * max(n, 1) - 1).bit_length()))
        for _ in range(4):
            d_work = DeviceBuffer(self.L.vh_resample_work_bytes(slots_log2))
            out = call(None, None, 0)
            if not grow or not (out["status"] & T.RESAMPLE_TABLE_FULL) or slots_log2 == most:
                break
            slots_log2 = min(most, slots_log2 + 2)
        out.update(zip(("descs", "voxels"), _staged_list(None, None, 0, self.stream)))
        room = out["candidates"]
        if out["status"] != 0 or room == 0:
            return out
        d_out, d_staging = _staging_pair(room)
        out = call(d_out, d_staging, room)
        out.update(zip(("descs", "voxels"), _staged_list(d_out, d_staging, out["staged"], self.stream, pool_blocks=room)))
        return out

    def download(self, with_voxels=True):
        hp, hd, s = self.hp, self.hd, self.stream
        return dict(_download_tables(hd, hp, s, with_voxels), state=download(hd.d_state, np.uint32, T.STATE_WORDS, s),
                    compactified=download(hd.d_hashCompactified, T.HASH_ENTRY_DTYPE, hp.m_numOccupiedBlocks, s),
                    decisions=download(hd.d_hashDecision, np.int32, hp.m_numOccupiedBlocks, s))

    def state(self, with_voxels=True):
        d = self.download(with_voxels)
        return dict(_canonical_state(d, self.hp, with_voxels), raw=d)
