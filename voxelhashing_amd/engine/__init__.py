"""Python mirror of the reference host classes over the C ABI:

    CUDASceneRepHashSDF   (DepthSensingCUDA/Source/CUDASceneRepHashSDF.h:28)
    CUDARayCastSDF        (DepthSensingCUDA/Source/CUDARayCastSDF.h:13)
    CUDASceneRepChunkGrid (DepthSensingCUDA/Source/CUDASceneRepChunkGrid.h:152)

Same method names and argument meaning as the reference (camelCase kept), so
tests read like the reference's frame loop (DepthSensing.cpp:720-924).  All
compute happens in libvoxelhashing_amd.so on the GPU; this package only marshals.

One module per subsystem; this file only gathers their public names (DESIGN.md section 1 has their table).
"""
from .. import canonical
from .. import vhtypes as T
from ..lib import DeviceBuffer, VhError, check, download, f16, load
from .chunk_grid import CUDASceneRepChunkGrid
from .frame_loop import Reconstruction
from .frames import DepthFrame, image_op, ingest_frame, synth_frame
from .launchers import LauncherScene
from .marching_cubes import CUDAMarchingCubesHashSDF, LiveMesh, live_mesh_digest
from .mesh import (mesh_cluster, mesh_cluster_default_scale_log2, mesh_cluster_key, mesh_components, mesh_components_filter,
                   mesh_normals_default_scale_log2, mesh_save_ply, mesh_smooth, mesh_vertex_normals, mesh_weld, mesh_weld_appends, mesh_weld_key)
from .raycast import CUDARayCastSDF
from .render import PhongLighting, RGBDRenderer, phong_light_from_render_state, view_resolve_depth, write_png_rgba8
from .scene import CUDASceneRepHashSDF, cut_region_transform, deintegrate_rule, extract_from_block_list, resample_voxel_transforms
from .sensor import CUDARGBDSensor
from .tracking import CUDACameraTrackingMultiRes, CUDACameraTrackingMultiResRGBD
