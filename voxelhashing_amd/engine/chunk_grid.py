"""CUDASceneRepChunkGrid (DepthSensingCUDA/Source/CUDASceneRepChunkGrid.h:152) over the C ABI."""
import ctypes as C

import numpy as np

from .. import vhtypes as T
from ..lib import check, f16
from ._common import _Handle, _int3, _scalar_out, _struct_out


class CUDASceneRepChunkGrid(_Handle):
    _destroy = "vh_chunk_grid_destroy"

    def __init__(self, sceneRepHashSDF, voxelExtends, gridDimensions, minGridPos, initialChunkListSize,
                 streamingEnabled, streamOutParts):
        self.scene = sceneRepHashSDF
        ext = np.asarray(voxelExtends, dtype=np.float32)
        self._create("vh_chunk_grid_create", sceneRepHashSDF.handle, f16(ext), _int3(gridDimensions), _int3(minGridPos), initialChunkListSize,
                     1 if streamingEnabled else 0, streamOutParts)

    def streamOutToCPUPass0GPU(self, posCamera, radius, useParts=True, multiThreaded=True):
        check(self.L.vh_chunk_grid_stream_out_to_cpu_pass0_gpu(self.handle, f16(posCamera), radius, int(useParts), int(multiThreaded)),
              "streamOutToCPUPass0GPU")

    def streamOutToCPUPass1CPU(self, multiThreaded=True):
        check(self.L.vh_chunk_grid_stream_out_to_cpu_pass1_cpu(self.handle, int(multiThreaded)), "streamOutToCPUPass1CPU")

    def streamInToGPUPass0CPU(self, posCamera, radius, useParts=True, multiThreaded=True):
        check(self.L.vh_chunk_grid_stream_in_to_gpu_pass0_cpu(self.handle, f16(posCamera), radius, int(useParts), int(multiThreaded)),
              "streamInToGPUPass0CPU")

    def streamInToGPUPass1GPU(self, multiThreaded=True):
        check(self.L.vh_chunk_grid_stream_in_to_gpu_pass1_gpu(self.handle, int(multiThreaded)), "streamInToGPUPass1GPU")

    def streamOutToCPU(self, posCamera, radius, useParts=True):
        return _scalar_out(C.c_uint32, "streamOutToCPU", self.L.vh_chunk_grid_stream_out_to_cpu, self.handle, f16(posCamera), radius, int(useParts))

    def streamInToGPU(self, posCamera, radius, useParts=True):
        return _scalar_out(C.c_uint32, "streamInToGPU", self.L.vh_chunk_grid_stream_in_to_gpu, self.handle, f16(posCamera), radius, int(useParts))

    def streamOutToCPUAll(self):
        check(self.L.vh_chunk_grid_stream_out_to_cpu_all(self.handle), "streamOutToCPUAll")

    def streamInToGPUAll(self, posCamera, radius, useParts=True):
        return _scalar_out(C.c_uint32, "streamInToGPUAll", self.L.vh_chunk_grid_stream_in_to_gpu_all, self.handle, f16(posCamera), radius, int(useParts))

    def getBitMaskGPU(self):
        return _struct_out(C.c_void_p, "getBitMaskGPU", self.L.vh_chunk_grid_get_bit_mask_gpu, self.handle)

    def downloadBitMasks(self):
        """-> (host copy, device copy, host copy marked dirty): both copies of the bit mask with the pipeline drained and
        before any upload of the host's copy (read-only; for tests)"""
        n, dirty = C.c_uint32(), C.c_int32()
        check(self.L.vh_chunk_grid_debug_download_bit_masks(self.handle, None, None, 0, C.byref(n), C.byref(dirty)), "downloadBitMasks")
        host, dev = np.zeros(n.value, dtype=np.uint32), np.zeros(n.value, dtype=np.uint32)
        check(self.L.vh_chunk_grid_debug_download_bit_masks(self.handle, host.ctypes.data, dev.ctypes.data, n.value, C.byref(n), C.byref(dirty)),
              "downloadBitMasks")
        return host, dev, bool(dirty.value)

    def reset(self):
        check(self.L.vh_chunk_grid_reset(self.handle), "reset")

    def debugCheckForDuplicates(self):
        check(self.L.vh_chunk_grid_debug_check_for_duplicates(self.handle), "debugCheckForDuplicates")

    def getStatistics(self):
        out = (C.c_uint32 * 3)()
        check(self.L.vh_chunk_grid_get_statistics(self.handle, out), "getStatistics")
        return dict(chunks=out[0], blocks=out[1], bits=out[2])

    def getNumFailedInserts(self):
        return _scalar_out(C.c_uint32, "getNumFailedInserts", self.L.vh_chunk_grid_get_num_failed_inserts, self.handle)

    def downloadHostBlocks(self):
        n = C.c_uint32()
        check(self.L.vh_chunk_grid_download_host_blocks(self.handle, None, None, 0, C.byref(n)), "downloadHostBlocks")
        descs = np.zeros(n.value, dtype=T.DESC_DTYPE)
        blocks = np.zeros((n.value, T.SDF_BLOCK_VOXELS), dtype=T.VOXEL_DTYPE)
        if n.value:
            check(self.L.vh_chunk_grid_download_host_blocks(self.handle, descs.ctypes.data, blocks.ctypes.data, n.value, C.byref(n)),
                  "downloadHostBlocks")
        return descs, blocks

    def saveToFile(self, filename, camPos, radius):
        check(self.L.vh_chunk_grid_save_to_file(self.handle, filename.encode(), f16(camPos), radius), "saveToFile")

    def loadFromFile(self, filename, camPos, radius):
        check(self.L.vh_chunk_grid_load_from_file(self.handle, filename.encode(), f16(camPos), radius), "loadFromFile")
