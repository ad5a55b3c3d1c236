"""ctypes binding of the C ABI declared in include/tinybvh_amd.h.

The shared library is built in-tree (tinybvh_amd/csrc/Makefile ->
tinybvh_amd/libtinybvh_amd.so).  There is no CPU fallback: if the library is missing or a
symbol is absent, importing this module raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TBVH_LIB_OVERRIDE") or os.path.join(_HERE, "libtinybvh_amd.so")   # override: A/B builds in tools/

# every symbol include/tinybvh_amd.h declares: name -> (restype, argtypes)
_u64, _u32, _vp, _i = C.c_uint64, C.c_uint32, C.c_void_p, C.c_int
_pp = C.POINTER(C.c_void_p)


class BuildParams(C.Structure):
    _fields_ = [("bins", _u32), ("max_leaf_tris", _u32), ("threads", _u32), ("flags", _u32)]


class Mesh(C.Structure):   # tbvh_mesh
    _fields_ = [("verts", C.c_void_p), ("n_verts", C.c_uint64), ("stride_bytes", C.c_uint32), ("on_device", C.c_uint32),
                ("indices", C.c_void_p), ("n_tris", C.c_uint64)]


class AlphaTexture(C.Structure):   # tbvh_alpha_texture
    _fields_ = [("texels", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32)]


class OmmSource(C.Structure):   # tbvh_omm_source
    _fields_ = [("uv", C.c_void_p), ("n_uv", C.c_uint64), ("uv_stride_bytes", C.c_uint32), ("on_device", C.c_uint32), ("indices", C.c_void_p),
                ("n_tris", C.c_uint64), ("tri_texture", C.c_void_p), ("textures", C.POINTER(AlphaTexture)), ("n_textures", C.c_uint32)]


class VoxelizeParams(C.Structure):   # tbvh_voxelize_params
    _fields_ = [("bmin", C.c_float * 3), ("maxSize", C.c_float), ("ext", C.c_float * 3), ("color", C.c_uint32), ("max_hits_per_ray", C.c_uint32)]


class VoxelizeStats(C.Structure):   # tbvh_voxelize_stats
    _fields_ = [("rounds", C.c_uint32), ("reserved", C.c_uint32), ("records", C.c_uint64), ("rays_cut", C.c_uint64), ("bricks", C.c_uint64)]


class SceneGraphDesc(C.Structure):   # tbvh_scenegraph_desc
    _fields_ = [("flags", C.c_uint32), ("n_nodes", C.c_uint64), ("parent", C.c_void_p), ("visit_order", C.c_void_p), ("translation", C.c_void_p), ("rotation", C.c_void_p),
                ("scale", C.c_void_p), ("matrix", C.c_void_p), ("local_transform", C.c_void_p), ("n_weights", C.c_void_p), ("weights", C.c_void_p),
                ("n_samplers", C.c_uint64), ("sampler_interpolation", C.c_void_p), ("sampler_type", C.c_void_p), ("sampler_key_offset", C.c_void_p),
                ("sampler_value_offset", C.c_void_p), ("key_times", C.c_void_p), ("key_values", C.c_void_p), ("n_animations", C.c_uint64), ("n_channels", C.c_uint64),
                ("channel_animation", C.c_void_p), ("channel_sampler", C.c_void_p), ("channel_node", C.c_void_p), ("channel_target", C.c_void_p),
                ("n_instances", C.c_uint64), ("node_of_instance", C.c_void_p), ("n_skin_uses", C.c_uint64), ("skin_mesh_node", C.c_void_p),
                ("skin_joint_offset", C.c_void_p), ("skin_joint_node", C.c_void_p), ("skin_inverse_bind", C.c_void_p)]


class Camera(C.Structure):
    _fields_ = [("eye", C.c_float * 3), ("p1", C.c_float * 3), ("p2", C.c_float * 3), ("p3", C.c_float * 3),
                ("width", _u32), ("height", _u32), ("spp_x", _u32), ("spp_y", _u32)]


class WfParams(C.Structure):
    _fields_ = [("light_pos", C.c_float * 3), ("light_color", C.c_float * 3), ("sky_lo", C.c_float * 3), ("sky_hi", C.c_float * 3),
                ("eps", C.c_float), ("max_depth", _u32), ("seed", _u32), ("clear", _u32), ("light_size", C.c_float * 2), ("flags", _u32), ("sample_index", _u32)]


class WfStats(C.Structure):
    _fields_ = [("extend_rays", _u64 * 8), ("shadow_rays", _u64 * 8), ("frame_ms", C.c_float)]


class ViewerParams(C.Structure):   # tbvh_viewer_params
    _fields_ = [("mode", _u32), ("max_rounds", _u32), ("light_dir", C.c_float * 3), ("flags", _u32)]


class ViewerStats(C.Structure):   # tbvh_viewer_stats
    _fields_ = [("rays", _u64 * 8), ("shadow_rays", _u64), ("frame_ms", C.c_float)]


SYMBOLS = {
    "tbvh_debug_wide_copy_bvh2": (_i, [_i, _vp, _u64, _vp, _u64, _vp, _u64, _u32, _vp, _u64, C.POINTER(_u64), _vp, _u64, C.POINTER(_u64)]),
    "tbvh_wavefront_create": (_i, [_vp, _u32, _u32, _pp]),
    "tbvh_wavefront_destroy": (None, [_vp]),
    "tbvh_wavefront_render": (_i, [_vp, _vp, _vp, C.POINTER(Camera), C.POINTER(WfParams), C.POINTER(WfStats)]),
    "tbvh_wavefront_read": (_i, [_vp, _vp]),
    "tbvh_wavefront_set_blas_vertices": (_i, [_vp, _vp, _u64]),
    "tbvh_wavefront_finalize": (_i, [_vp, C.c_float, _vp]),
    "tbvh_wavefront_set_blue_noise": (_i, [_vp, _vp, _u64]),
    "tbvh_abi_version": (_i, []),
    "tbvh_last_error": (C.c_char_p, []),
    "tbvh_device_count": (_i, []),
    "tbvh_init": (_i, [_i, _pp]),
    "tbvh_shutdown": (None, [_vp]),
    "tbvh_synchronize": (_i, [_vp]),
    "tbvh_set_stream": (_i, [_vp, _vp]),
    "tbvh_context_set_overlap": (_i, [_vp, _i]),
    "tbvh_debug_overlap_stats": (_i, [_vp, _vp]),
    "tbvh_debug_lane_script": (_i, [_vp, _u64, _vp]),
    "tbvh_debug_set_overlap_depth": (_i, [_vp, _i]),
    "tbvh_debug_set_probe_memory": (_i, [_vp, _i]),
    "tbvh_debug_probe_memory_stats": (_i, [_vp, _vp]),
    "tbvh_debug_runahead_script": (_i, [_vp, _u64, _i, _vp]),
    "tbvh_debug_launch_plan": (_i, [_vp, _u32, _vp, _u32]),
    "tbvh_debug_tlas_plan": (_i, [_vp, _u32, _vp, _u32]),
    "tbvh_debug_tlas_state": (_i, [_vp, _vp, _vp]),
    "tbvh_debug_packet_cull": (_i, [_vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp]),
    "tbvh_debug_tri_test_flat": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp]),
    "tbvh_set_timing": (_i, [_vp, _i]),
    "tbvh_upload_bvh_gpu": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _pp]),
    "tbvh_upload_bvh4_gpu": (_i, [_vp, _vp, _u64, _pp]),
    "tbvh_upload_cwbvh": (_i, [_vp, _vp, _u64, _vp, _u64, _pp]),
    "tbvh_upload_tlas": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _pp, _u64, _pp]),
    "tbvh_update_tlas": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64]),
    "tbvh_update_bvh_gpu": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64]),
    "tbvh_update_bvh4_gpu": (_i, [_vp, _vp, _u64]),
    "tbvh_update_cwbvh": (_i, [_vp, _vp, _u64, _vp, _u64]),
    "tbvh_rebuild_tlas_device": (_i, [_vp, _vp, _i, _vp, _u64]),
    "tbvh_refit": (_i, [_vp, _vp, _u64, _i]),
    "tbvh_set_triangle_test": (_i, [_vp, _i, _vp, _u64, _i]),
    "tbvh_scene_triangle_test": (_i, [_vp]),
    "tbvh_host_tri_test": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tbvh_debug_tri_test_batch": (_i, [_i, _i, _vp, _vp, _u64, _vp, _vp, _vp]),
    "tbvh_set_opacity_micromaps": (_i, [_vp, _vp, _u32, _u64, _i]),
    "tbvh_scene_download": (_i, [_vp, _i, _vp, _u64, _vp]),
    "tbvh_build_device": (_i, [_vp, _vp, _u64, _i, _i, _u32, _vp]),
    "tbvh_build_device_ploc": (_i, [_vp, _vp, _u64, _i, _i, _u32, _vp]),
    "tbvh_build_device_sah": (_i, [_vp, _vp, _u64, _i, _i, _u32, _vp]),
    "tbvh_build_bvh2_sah_device": (_i, [_vp, C.POINTER(Mesh), _u32, _vp, _u64, _vp, _u64, _i, C.POINTER(_u64)]),
    "tbvh_host_build_bvh2_sah": (_i, [C.POINTER(Mesh), _u32, _vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    "tbvh_build_bvh2_sah_device_aabbs": (_i, [_vp, _vp, _u64, _i, _u32, _vp, _u64, _vp, _u64, _i, C.POINTER(_u64)]),
    "tbvh_host_build_bvh2_sah_aabbs": (_i, [_vp, _u64, _u32, _vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    "tbvh_host_build_bvh2_sah_spheres": (_i, [_vp, _u64, _u32, _vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    "tbvh_host_build_tlas_sah": (_i, [_vp, _u64, _vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    "tbvh_build_device_custom_spheres_sah": (_i, [_vp, _vp, _u64, _i, _u32, C.POINTER(_vp)]),
    "tbvh_build_bvh2_sbvh_device": (_i, [_vp, C.POINTER(Mesh), _u32, _vp, _u64, _vp, _u64, _i, C.POINTER(_u64), C.POINTER(_u64), _vp]),
    "tbvh_host_build_bvh2_sbvh": (_i, [C.POINTER(Mesh), _u32, _vp, _u64, _vp, _u64, C.POINTER(_u64), C.POINTER(_u64), _vp]),
    "tbvh_build_device_sbvh": (_i, [_vp, _vp, _u64, _i, _i, _u32, _vp]),
    "tbvh_build_device_sbvh_mesh": (_i, [_vp, C.POINTER(Mesh), _i, _u32, _vp]),
    "tbvh_convert_bvh2_device": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _i, _i, _vp]),
    "tbvh_tlas_download": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp]),
    "tbvh_free_scene": (None, [_vp]),
    "tbvh_scene_layout": (_i, [_vp]),
    "tbvh_scene_device_bytes": (_u64, [_vp]),
    "tbvh_debug_scene_bytes": (_i, [_vp, _vp]),
    "tbvh_intersect": (_i, [_vp, _vp, _u64, _u32]),
    "tbvh_occluded": (_i, [_vp, _vp, _u64, _u32, _vp]),
    "tbvh_intersect_sharded": (_i, [_vp, _u32, _vp, _u64, _u32]),
    "tbvh_occluded_sharded": (_i, [_vp, _u32, _vp, _u64, _u32, _vp]),
    "tbvh_intersect_sharded_device": (_i, [_vp, _u32, _vp, _vp, _i, C.c_float, _vp, _vp]),
    "tbvh_occluded_sharded_device": (_i, [_vp, _u32, _vp, _vp, _vp, _vp, _vp]),
    "tbvh_wavefront_set_band": (_i, [_vp, _u32, _u32]),
    "tbvh_debug_wavefront_queues": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tbvh_wavefront_render_sharded": (_i, [_vp, _vp, _vp, _u32, C.POINTER(Camera), _vp, _vp, _vp]),
    "tbvh_wavefront_read_sharded": (_i, [_vp, _u32, _vp]),
    "tbvh_shard_range": (None, [_u64, _u32, _u32, C.POINTER(_u64), C.POINTER(_u64)]),
    "tbvh_intersect_device": (_i, [_vp, _vp, _u64]),
    "tbvh_occluded_device": (_i, [_vp, _vp, _u64, _vp]),
    "tbvh_intersect_device_fresh": (_i, [_vp, _vp, _u64, C.c_float]),
    "tbvh_reset_hits_device": (_i, [_vp, _vp, _u64, C.c_float]),
    "tbvh_time_last_ms": (C.c_float, [_vp]),
    "tbvh_debug_coherent_schedule": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_uint32)]),
    "tbvh_time_history": (C.c_int, [_vp, C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32)]),
    "tbvh_measure_copy_bandwidth": (_i, [_vp, _u64, _u32, C.POINTER(C.c_double)]),
    "tbvh_measure_read_bandwidth": (_i, [_vp, _u64, _u32, C.POINTER(C.c_double)]),
    "tbvh_measure_valu_issue": (_i, [_vp, _u32, C.POINTER(C.c_double)]),
    "tbvh_measure_link_bandwidth": (_i, [_vp, _u64, _u32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "tbvh_scene_get_schedule_hint": (_i, [_vp, _vp]),
    "tbvh_scene_set_schedule_hint": (_i, [_vp, _vp]),
    "tbvh_pinned_malloc": (_i, [_vp, _u64, _pp]),
    "tbvh_pinned_free": (_i, [_vp, _vp]),
    "tbvh_set_variant": (_i, [_vp, _i]),
    "tbvh_debug_stats": (_i, [_vp, _vp, _i]),
    "tbvh_debug_last_probe": (_i, [_vp, _vp]),
    "tbvh_debug_set_flags": (_i, [_vp, _u32]),
    "tbvh_debug_set_sah_small_subtree": (_i, [_vp, _u32]),
    "tbvh_debug_set_sah_one_group": (_i, [_vp, _u32]),
    "tbvh_debug_get_sah_thresholds": (_i, [_vp, C.POINTER(_u32)]),
    "tbvh_tlas_set_builder": (_i, [_vp, _i]),
    "tbvh_debug_device_allocations": (_i, [C.POINTER(_u64)]),
    "tbvh_debug_lbvh_topology": (_i, [_vp, _u64, _i, _vp]),
    "tbvh_debug_lbvh_ordered": (_i, [_vp, _u64, _i, _vp, _vp]),
    "tbvh_debug_build_scratch_bytes": (_i, [_u32, _u64, _u64, _vp]),
    "tbvh_cwbvh_set_hybrid": (_i, [_vp, C.c_int64]),
    "tbvh_bin_rays_device": (_i, [_vp, _vp, _vp, _u64, C.POINTER(C.c_float), _u32, _u32, _vp]),
    "tbvh_generate_primary_device": (_i, [_vp, C.POINTER(Camera), _vp, _u64, _u64]),
    "tbvh_generate_bounce_device": (_i, [_vp, _vp, _vp, _vp, _u64, _u32]),
    "tbvh_generate_shadow_device": (_i, [_vp, _vp, _vp, _u64, C.POINTER(C.c_float), C.c_float]),
    "tbvh_device_malloc": (_i, [_vp, _u64, _pp]),
    "tbvh_device_free": (_i, [_vp, _vp]),
    "tbvh_copy_to_device": (_i, [_vp, _vp, _vp, _u64]),
    "tbvh_copy_from_device": (_i, [_vp, _vp, _vp, _u64]),
    "tbvh_host_build": (_i, [_vp, _u64, _i, C.POINTER(BuildParams), _pp]),
    "tbvh_host_build_tlas": (_i, [_vp, _u64, _vp, _u64, _pp]),
    "tbvh_host_free": (None, [_vp]),
    "tbvh_cwbvh_file_write": (_i, [C.c_char_p, _vp, _u64, _vp, _u64, _u64, _vp]),
    "tbvh_cwbvh_file_read": (_i, [C.c_char_p, _u64, _pp, C.POINTER(_u64)]),
    "tbvh_host_layout": (_i, [_vp]),
    "tbvh_host_blob": (_vp, [_vp, _i]),
    "tbvh_host_blob_count": (_u64, [_vp, _i]),
    "tbvh_upload_host": (_i, [_vp, _vp, _vp, _u64, _pp]),
    # BVH_Double scenes (capi_double.hip)
    "tbvh_upload_bvh_double": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _pp]),
    "tbvh_upload_tlas_double": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _pp, _u64, _pp]),
    "tbvh_intersect_ex_device": (_i, [_vp, _vp, _u64]),
    "tbvh_occluded_ex_device": (_i, [_vp, _vp, _u64, _vp]),
    "tbvh_intersect_ex": (_i, [_vp, _vp, _u64]),
    "tbvh_occluded_ex": (_i, [_vp, _vp, _u64, _vp]),
    "tbvh_host_build_double": (_i, [_vp, _u64, _pp]),
    "tbvh_host_build_tlas_double": (_i, [_vp, _u64, _vp, _u64, _pp]),
    # ... that move (capi_double.hip, kernels_double_anim.hip)
    "tbvh_rebuild_tlas_double_device": (_i, [_vp, _vp, _i]),
    "tbvh_update_tlas_double": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64]),
    "tbvh_tlas_double_download": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp]),
    "tbvh_double_download": (_i, [_vp, _vp, _u64, _vp]),
    "tbvh_refit_double": (_i, [_vp, _vp, _u64, _i]),
    # ... over custom geometry: spheres {pos, r} (capi_double.hip, the sphere forms of kernels_double.hip)
    "tbvh_upload_custom_spheres_double": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _pp]),
    "tbvh_host_build_custom_spheres_double": (_i, [_vp, _u64, _pp]),
    "tbvh_build_device_custom_spheres_double": (_i, [_vp, _vp, _u64, _i, _pp]),
    "tbvh_rebuild_custom_spheres_double_device": (_i, [_vp, _vp, _u64, _i]),
    "tbvh_custom_spheres_double_download": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _vp]),
    # VoxelSet scenes (capi_voxel.hip)
    "tbvh_upload_voxelset": (_i, [_vp, _vp, _vp, _u64, _vp, _pp]),
    "tbvh_host_build_voxelset": (_i, [_vp, _u32, _u32, _u32, _pp]),
    "tbvh_upload_voxelset_dense": (_i, [_vp, _vp, _u32, _u32, _u32, _pp]),
    # editing voxel sets, GetNormal (capi_voxel_edit.hip, voxel_edit_host.cpp)
    "tbvh_voxelset_create": (_i, [_vp, _u64, _pp]),
    "tbvh_voxelset_reserve": (_i, [_vp, _u64]),
    "tbvh_voxelset_capacity": (_i, [_vp, _vp, _vp]),
    "tbvh_voxelset_set": (_i, [_vp, _vp, _u64, _i]),
    "tbvh_voxelset_update_top_grid": (_i, [_vp]),
    "tbvh_voxelset_download": (_i, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "tbvh_host_voxelset_create": (_i, [_pp]),
    "tbvh_host_voxelset_set": (_i, [_vp, _vp, _u64]),
    "tbvh_host_voxelset_update_top_grid": (_i, [_vp]),
    "tbvh_voxel_normals_device": (_i, [_vp, _vp, _vp, _u32, _u64, _vp]),
    "tbvh_voxel_normals": (_i, [_vp, _vp, _vp, _u32, _u64, _vp]),
    "tbvh_voxelize_device": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "tbvh_host_voxel_normals": (_i, [_vp, _u64, _vp, _u32, _u64, _vp]),
    # custom-geometry sphere BLASes (capi_custom.hip)
    "tbvh_upload_custom_spheres": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _pp]),
    "tbvh_host_build_custom_spheres": (_i, [_vp, _u64, _pp]),
    "tbvh_build_device_custom_spheres": (_i, [_vp, _vp, _u64, _i, _i, _u32, _u32, _pp]),
    "tbvh_rebuild_custom_spheres_device": (_i, [_vp, _vp, _u64, _i]),
    "tbvh_refit_custom_spheres": (_i, [_vp, _vp, _u64, _i]),
    "tbvh_custom_spheres_download": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _vp]),
    "tbvh_custom_spheres_bounds": (_i, [_vp, _vp]),
    # sphere-overlap queries (capi_sphere.hip)
    "tbvh_intersect_spheres": (_i, [_vp, _vp, _u64, _vp, _u64, _vp]),
    "tbvh_intersect_spheres_device": (_i, [_vp, _vp, _u64, _vp, _u64, _vp]),
    # indexed / strided triangle meshes (tbvh_mesh)
    "tbvh_upload_bvh_gpu_mesh": (_i, [_vp, _vp, _u64, _vp, _u64, C.POINTER(Mesh), _pp]),
    "tbvh_update_bvh_gpu_mesh": (_i, [_vp, _vp, _u64, _vp, _u64, C.POINTER(Mesh)]),
    "tbvh_host_build_mesh": (_i, [C.POINTER(Mesh), _i, C.POINTER(BuildParams), _pp]),
    "tbvh_upload_host_mesh": (_i, [_vp, _vp, C.POINTER(Mesh), _pp]),
    "tbvh_build_device_mesh": (_i, [_vp, C.POINTER(Mesh), _i, _u32, _i, _u32, _pp]),
    "tbvh_convert_bvh2_device_mesh": (_i, [_vp, _vp, _u64, _vp, _u64, C.POINTER(Mesh), _i, _i, _pp]),
    "tbvh_refit_mesh": (_i, [_vp, C.POINTER(Mesh)]),
    "tbvh_intersect_spheres_mesh": (_i, [_vp, _vp, _u64, C.POINTER(Mesh), _vp]),
    "tbvh_intersect_spheres_mesh_device": (_i, [_vp, _vp, _u64, C.POINTER(Mesh), _vp]),
    "tbvh_flatten_mesh_device": (_i, [_vp, C.POINTER(Mesh), _vp]),
    # skinned / morph-target meshes posed on the device (capi_pose.hip)
    "tbvh_pose_create_skin": (_i, [_vp, _vp, _u64, _vp, _vp, _u32, _i, _pp]),
    "tbvh_pose_create_morph": (_i, [_vp, _vp, _u64, _u32, _i, _pp]),
    "tbvh_pose_set_skin": (_i, [_vp, _vp, _u32, _i]),
    "tbvh_pose_set_morph": (_i, [_vp, _vp, _u32, _i]),
    "tbvh_pose_vertices": (_i, [_vp, _pp, C.POINTER(_u64)]),
    "tbvh_pose_refit": (_i, [_vp, _vp]),
    "tbvh_pose_download": (_i, [_vp, _vp, _u64]),
    "tbvh_pose_free": (None, [_vp]),
    # the animated scene graph (capi_scenegraph.hip, scenegraph_host.cpp)
    "tbvh_scenegraph_create": (_i, [_vp, C.POINTER(SceneGraphDesc), _pp]),
    "tbvh_scenegraph_advance": (_i, [_vp, C.c_float]),
    "tbvh_scenegraph_advance_animation": (_i, [_vp, _u32, C.c_float]),
    "tbvh_scenegraph_update_nodes": (_i, [_vp]),
    "tbvh_scenegraph_set_time": (_i, [_vp, _u32, C.c_float]),
    "tbvh_scenegraph_reset": (_i, [_vp, _u32]),
    "tbvh_scenegraph_set_local": (_i, [_vp, _u32, _vp]),
    "tbvh_scenegraph_instance_transforms": (_i, [_vp, _pp, C.POINTER(_u64)]),
    "tbvh_scenegraph_joint_matrices": (_i, [_vp, _u32, _pp, C.POINTER(_u32)]),
    "tbvh_scenegraph_morph_weights": (_i, [_vp, _u32, _pp, C.POINTER(_u32)]),
    "tbvh_scenegraph_download": (_i, [_vp, _i, _vp, _u64]),
    "tbvh_scenegraph_free": (None, [_vp]),
    "tbvh_debug_scenegraph_array": (_i, [_vp, _i, _pp]),
    "tbvh_debug_scenegraph_step": (_i, [_vp, _i, C.c_float]),
    "tbvh_host_scenegraph_create": (_i, [C.POINTER(SceneGraphDesc), _pp]),
    "tbvh_host_scenegraph_advance": (_i, [_vp, C.c_float]),
    "tbvh_host_scenegraph_advance_animation": (_i, [_vp, _u32, C.c_float]),
    "tbvh_host_scenegraph_update_nodes": (_i, [_vp]),
    "tbvh_host_scenegraph_set_time": (_i, [_vp, _u32, C.c_float]),
    "tbvh_host_scenegraph_reset": (_i, [_vp, _u32]),
    "tbvh_host_scenegraph_set_local": (_i, [_vp, _u32, _vp]),
    "tbvh_debug_host_scenegraph_set_trs": (_i, [_vp, _vp, _u64]),
    "tbvh_debug_host_scenegraph_check_chains": (_i, [_vp, C.POINTER(_u64)]),
    "tbvh_host_scenegraph_instance_transforms": (_i, [_vp, _pp, C.POINTER(_u64)]),
    "tbvh_host_scenegraph_joint_matrices": (_i, [_vp, _u32, _pp, C.POINTER(_u32)]),
    "tbvh_host_scenegraph_morph_weights": (_i, [_vp, _u32, _pp, C.POINTER(_u32)]),
    "tbvh_host_scenegraph_download": (_i, [_vp, _i, _vp, _u64]),
    "tbvh_host_scenegraph_free": (None, [_vp]),
    "tbvh_host_pose_skin": (_i, [_vp, _u64, _vp, _vp, _vp, _u32, _vp]),
    "tbvh_host_pose_morph": (_i, [_vp, _u64, _u32, _vp, _vp]),
    # opacity micromaps baked from alpha textures (capi_omm.hip)
    "tbvh_bake_opacity_micromaps": (_i, [_vp, C.POINTER(OmmSource), _u32, _vp]),
    "tbvh_bake_set_opacity_micromaps": (_i, [_vp, C.POINTER(OmmSource), _u32]),
    "tbvh_host_bake_opacity_micromaps": (_i, [C.POINTER(OmmSource), _u32, _vp]),
    # hits resolved to shading data (capi_shade.hip)
    "tbvh_shading_create": (_i, [_vp, _vp, _u32, _vp, _u32, _i, _pp]),
    "tbvh_shading_set_fat_tris": (_i, [_vp, _u32, _vp, _u64, _i]),
    "tbvh_shading_fat_tris": (_i, [_vp, _u32, _pp, C.POINTER(_u64)]),
    "tbvh_shading_download_fat_tris": (_i, [_vp, _u32, _vp, _u64]),
    "tbvh_shading_free": (None, [_vp]),
    "tbvh_shade_hits": (_i, [_vp, _vp, _vp, _u64, _u32, _vp]),
    "tbvh_shade_hits_device": (_i, [_vp, _vp, _vp, _u64, _u32, _vp]),
    "tbvh_shade_continue_device": (_i, [_vp, _vp, _u32, _vp, _u64, _vp]),
    "tbvh_pose_attach_fat_tris": (_i, [_vp, _vp, _u32, _vp, _vp, _u64, _i]),
    "tbvh_host_pose_skin_normals": (_i, [_u64, _vp, _vp, _vp, _u32, _vp, _vp]),
    "tbvh_host_pose_morph_normals": (_i, [_vp, _u64, _u32, _vp]),
    "tbvh_host_pose_update_fat_tris": (_i, [_vp, _u64, _vp, _vp, _u64, _vp, _i]),
    "tbvh_host_shade_hits": (_i, [_vp, _u32, _vp, _u32, _vp, _vp, _u32, _vp, _u64, _vp, _u64, _u32, _vp]),
    # a viewer frame lit and finished on the device (capi_viewer.hip)
    "tbvh_sky_create": (_i, [_vp, _vp, _u32, _u32, _i, _pp]),
    "tbvh_sky_free": (None, [_vp]),
    "tbvh_sky_sample_device": (_i, [_vp, _vp, _u64, _vp]),
    "tbvh_host_sky_sample": (_i, [_vp, _u32, _u32, _vp, _u64, _vp]),
    "tbvh_host_sky_prepare": (_i, [_vp, _u64, _vp, _i]),
    "tbvh_viewer_generate_device": (_i, [_vp, C.POINTER(Camera), _vp, _u64, _u64]),
    "tbvh_viewer_shadow_rays_device": (_i, [_vp, _vp, _u32, _u64, _vp, _vp]),
    "tbvh_viewer_light_device": (_i, [_vp, _u32, _vp, _vp, _vp, _u32, _vp, _vp, _u64, _vp, _vp]),
    "tbvh_viewer_pack_device": (_i, [_vp, _vp, _u64, _vp]),
    "tbvh_host_viewer_generate": (_i, [C.POINTER(Camera), _vp, _u64, _u64]),
    "tbvh_host_viewer_continue": (_i, [_vp, _u32, _u32, _vp, _u32, _vp, _u64, _vp, C.POINTER(_u64)]),
    "tbvh_host_viewer_shadow_rays": (_i, [_vp, _u32, _u64, _vp, _vp]),
    "tbvh_host_viewer_light": (_i, [_u32, _vp, _u32, _u32, _vp, _u32, _vp, _vp, _u64, _vp, _vp]),
    "tbvh_host_viewer_pack": (_i, [_vp, _u64, _vp]),
    "tbvh_viewer_create": (_i, [_vp, _u32, _u32, _pp]),
    "tbvh_viewer_destroy": (None, [_vp]),
    "tbvh_viewer_render": (_i, [_vp, _vp, _vp, _vp, C.POINTER(Camera), C.POINTER(ViewerParams), C.POINTER(ViewerStats)]),
    "tbvh_viewer_read_pixels": (_i, [_vp, _vp]),
    "tbvh_viewer_read_rgb": (_i, [_vp, _vp]),
    "tbvh_viewer_rays": (_i, [_vp, _pp]),
    "tbvh_debug_viewer_math": (_i, [_i, _vp, _vp, _u64, _vp]),
}


def _load() -> C.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `make -C tinybvh_amd/csrc` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback."
        )
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the ABI and the header disagree
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


class TbvhError(RuntimeError):
    def __init__(self, code: int, where: str):
        msg = lib.tbvh_last_error()
        super().__init__(f"{where}: error {code}: {msg.decode() if msg else ''}")
        self.code = code


def check(code: int, where: str) -> None:
    if code != 0:
        raise TbvhError(code, where)
