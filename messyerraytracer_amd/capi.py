"""ctypes binding of the C-ABI in include/mrt_hip.h (libmrt_hip.so).

This is plumbing for tests and bench.py; the product is the shared library.
There is no fallback: if the library is missing or fails to load, importing
callers get an ImportError / MrtError, never a CPU path.
"""
import ctypes as C
import os

import numpy as np

from . import types as T

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MRT_LIB_PATH", os.path.join(HERE, "libmrt_hip.so"))  # override: A/B builds in tools/

MRT_OK = 0
ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_NO_SCENE, ERR_PENDING, ERR_NOT_PENDING, ERR_OOM, ERR_UNSUPPORTED, ERR_BAD_BVH = range(1, 10)
MODE_NEAREST, MODE_ANY_HIT = 0, 1
FLAG_COHERENT, FLAG_RAYS_ON_DEVICE, FLAG_HITS_ON_DEVICE, FLAG_HOST_LAYOUT, FLAG_BOOL_OUT, FLAG_FORCE_SORT, FLAG_TOKEN_OUT, FLAG_ASYNC = (1 << i for i in range(8))
TOKEN_MISS = 0xFFFFFFFF
BUILD_TRIS_ON_DEVICE, BUILD_SAFE_HANDOFF, BUILD_BLAS_ON_DEVICE, BUILD_PLOC, BUILD_SAH, BUILD_INSTANCES_ON_DEVICE = 1, 2, 4, 8, 16, 32
TLAS_FORMS = {"radix": 0, "ploc": BUILD_PLOC, "sah": BUILD_SAH}  # update_instances_device(form=...)
KERNEL_AUTO, KERNEL_LANE, KERNEL_PACKET = 0, 1, 2   # (3 and 4: retired experiments, ids not reused)
KERNEL_PACKET_ASM, KERNEL_LANE_PERSISTENT, KERNEL_LANE4_PERSISTENT, KERNEL_LANE8_PERSISTENT, KERNEL_PACKET_DUAL, KERNEL_PACKET_ROWS, KERNEL_PACKET_QUAD = 5, 6, 7, 8, 9, 10, 11
KERNEL_TWO_LEVEL, KERNEL_TWO_LEVEL_PACKET, KERNEL_TWO_LEVEL_PERSISTENT, KERNEL_TWO_LEVEL_PERSISTENT8 = 100, 101, 102, 103  # reported only

# every entry point include/mrt_hip.h declares (tests check they are all exported)
SYMBOLS = [
    "mrt_create", "mrt_destroy", "mrt_last_error", "mrt_status_string", "mrt_version", "mrt_set_stream",
    "mrt_synchronize", "mrt_make_triangles", "mrt_pack_host_triangles", "mrt_bvh2_build", "mrt_bvh2_save", "mrt_bvh2_load", "mrt_upload_scene",
    "mrt_build_scene_device", "mrt_flatten_instances", "mrt_build_instanced_scene_device", "mrt_refit_scene", "mrt_refit_instanced_scene", "mrt_upload_two_level_scene", "mrt_refit_two_level_scene", "mrt_update_instances", "mrt_update_instances_device", "mrt_two_level_prepare_host", "mrt_two_level_host_arrays", "mrt_two_level_free_host", "mrt_scene_prepare_host", "mrt_scene_host_arrays", "mrt_scene_free_host", "mrt_debug_snapshot", "mrt_is_available", "mrt_scene_info", "mrt_cast", "mrt_submit", "mrt_collect", "mrt_has_pending",
    "mrt_camera_look", "mrt_camera_perspective", "mrt_camera_orthographic", "mrt_generate_grid", "mrt_cast_grid", "mrt_cast_tiled",
    "mrt_cast_shadows", "mrt_cast_grid_shadows", "mrt_cast_reflections", "mrt_cast_grid_reflections", "mrt_cast_hemisphere", "mrt_cast_grid_hemisphere", "mrt_cast_bounce", "mrt_cast_grid_bounce",
    "mrt_upload_shade_data", "mrt_clear_shade_data", "mrt_resolve_surfaces", "mrt_resolve_grid_surfaces",
    "mrt_upload_textures", "mrt_clear_textures",
    "mrt_upload_panorama", "mrt_clear_panorama",
    "mrt_shade_channels", "mrt_shade_grid_channels", "mrt_finish_color", "mrt_image_to_rgba8",
    "mrt_halton_jitter", "mrt_accum_begin_frame", "mrt_accum_end_frame", "mrt_accumulate",
    "mrt_denoise_spatial", "mrt_denoise_temporal", "mrt_composite_reflections", "mrt_resolve_reflections", "mrt_reflection_guides",
    "mrt_svgf_guides", "mrt_svgf_temporal", "mrt_svgf_variance", "mrt_svgf_atrous", "mrt_svgf_modulate", "mrt_svgf_frame",
    "mrt_cast_gbuffer_reflections", "mrt_reflection_image",
    "mrt_shadow_lights", "mrt_light_surfaces", "mrt_light_grid_surfaces",
    "mrt_cast_selected_shadows", "mrt_cast_grid_selected_shadows", "mrt_light_selected_surfaces", "mrt_light_grid_selected_surfaces",
    "mrt_build_emitters", "mrt_clear_emitters", "mrt_emitter_info", "mrt_emitter_table", "mrt_cast_emitter_shadows", "mrt_cast_grid_emitter_shadows",
    "mrt_light_emitter_surfaces", "mrt_light_grid_emitter_surfaces", "mrt_path_step_emitters", "mrt_path_grid_step_emitters",
    "mrt_path_init", "mrt_path_step", "mrt_path_grid_step", "mrt_path_finish", "mrt_expand_tokens",
    "mrt_expand_grid_tokens", "mrt_token_bytes", "mrt_morton_keys",
    "mrt_kernel_name", "mrt_struct_size", "mrt_get_stats", "mrt_last_kernel_variant", "mrt_schedule_counts", "mrt_debug_sort_order", "mrt_kernel_available", "mrt_device_alloc", "mrt_device_free", "mrt_memcpy_h2d", "mrt_memcpy_d2h",
    "mrt_group_create", "mrt_group_destroy", "mrt_group_size", "mrt_group_context", "mrt_group_last_error", "mrt_group_row_block",
    "mrt_group_upload_scene", "mrt_group_upload_two_level_scene", "mrt_group_cast_grid",
]


class MrtError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"mrt status {status}: {msg}")
        self.status = status


class Options(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("kernel", C.c_uint32), ("count_visits", C.c_uint32),
                ("sort_threshold", C.c_uint32), ("grid_tile", C.c_uint32), ("tile_w_log2", C.c_uint32),
                ("xcd_swizzle", C.c_uint32), ("stack_override", C.c_uint32), ("tile_order", C.c_uint32),
                ("sort_key", C.c_uint32), ("refill", C.c_uint32), ("leaf_wait", C.c_uint32),
                ("extra_lds", C.c_uint32), ("packet_wg", C.c_uint32), ("packet_cull", C.c_uint32), ("tile_schedule", C.c_uint32)]


class Camera(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("fwd", C.c_float * 3), ("right", C.c_float * 3), ("up", C.c_float * 3),
                ("half_w", C.c_float), ("half_h", C.c_float), ("t_min", C.c_float), ("t_max", C.c_float),
                ("kind", C.c_uint32), ("inv_w", C.c_float), ("inv_h", C.c_float), ("jitter_x", C.c_float), ("jitter_y", C.c_float),
                ("reserved", C.c_uint32 * 3)]


class Hemisphere(C.Structure):
    """mrt_hemisphere"""
    _fields_ = [("n_samples", C.c_uint32), ("frame", C.c_uint32), ("first_draw", C.c_uint32), ("t_max", C.c_float),
                ("d_select", C.c_void_p)]


class Bounce(C.Structure):
    """mrt_bounce"""
    _fields_ = [("frame", C.c_uint32), ("first_draw", C.c_uint32), ("t_max", C.c_float), ("metallic", C.c_float),
                ("roughness", C.c_float), ("d_select", C.c_void_p), ("d_surface", C.c_void_p), ("d_out_lobe", C.c_void_p)]


LOBE_NONE, LOBE_DIFFUSE, LOBE_SPECULAR = 0, 1, 2


class LightSelect(C.Structure):
    """mrt_light_select (types.LIGHT_SELECT)"""
    _fields_ = [("frame", C.c_uint32), ("select_draw", C.c_uint32), ("d_select", C.c_void_p), ("d_out_light", C.c_void_p)]


class EmitterSelect(C.Structure):
    """mrt_emitter_select (types.EMITTER_SELECT)"""
    _fields_ = [("frame", C.c_uint32), ("draw", C.c_uint32), ("d_select", C.c_void_p), ("d_out_emitter", C.c_void_p)]


EMITTER_ACCUMULATE = 1


class ShadeData(C.Structure):
    """mrt_shade_data"""
    _fields_ = [("struct_size", C.c_uint32), ("n_tris", C.c_uint32), ("n_materials", C.c_uint32), ("flags", C.c_uint32),
                ("materials", C.c_void_p), ("material_ids", C.c_void_p), ("normals9", C.c_void_p), ("uvs6", C.c_void_p)]


class SurfaceOut(C.Structure):
    """mrt_surface_out"""
    _fields_ = [("d_rows", C.c_void_p), ("d_bounce_surface", C.c_void_p), ("d_out_hits", C.c_void_p)]


class Texture(C.Structure):
    """mrt_texture"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("format", C.c_uint32), ("reserved", C.c_uint32), ("pixels", C.c_void_p)]


class TextureSet(C.Structure):
    """mrt_texture_set"""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("n_textures", C.c_uint32), ("n_bindings", C.c_uint32),
                ("n_tangent_tris", C.c_uint32), ("reserved", C.c_uint32), ("textures", C.c_void_p), ("bindings", C.c_void_p),
                ("tangents12", C.c_void_p)]


class Panorama(C.Structure):
    """mrt_panorama"""
    _fields_ = [("pixels", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("energy", C.c_float), ("flags", C.c_uint32)]


CHANNEL_COLOR, CHANNEL_NORMAL, CHANNEL_DEPTH, CHANNEL_BARYCENTRIC, CHANNEL_POSITION, CHANNEL_PRIM_ID, CHANNEL_HIT_MASK, CHANNEL_ALBEDO, \
    CHANNEL_WIREFRAME, CHANNEL_UV, CHANNEL_FRESNEL, CHANNEL_COUNT = range(12)   # RayImage::Channel


class ChannelOut(C.Structure):
    """mrt_channel_out"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("inv_depth_range", C.c_float), ("inv_pos_range", C.c_float),
                ("d_rgba", C.c_void_p * CHANNEL_COUNT), ("d_rgba8", C.c_void_p * CHANNEL_COUNT)]


class AccumState(C.Structure):
    """mrt_accum_state"""
    _fields_ = [("struct_size", C.c_uint32), ("aa_enabled", C.c_uint32), ("max_samples", C.c_int32), ("count", C.c_uint32),
                ("pixels", C.c_uint64), ("prev_origin", C.c_float * 3), ("prev_basis", C.c_float * 9),
                ("jitter_x", C.c_float), ("jitter_y", C.c_float), ("sample_index", C.c_uint32), ("accumulate", C.c_uint32),
                ("n_prior", C.c_uint32), ("reserved", C.c_uint32)]


ACCUM_SRC_RGBA, ACCUM_SRC_LIT, ACCUM_SRC_PATH_STATE = 0, 1, 2


class LightOut(C.Structure):
    """mrt_light_out"""
    _fields_ = [("d_rgba", C.c_void_p)]


class PathStepDesc(C.Structure):
    """mrt_path_step_desc"""
    _fields_ = [("frame", C.c_uint32), ("bounce", C.c_uint32), ("max_bounces", C.c_uint32), ("reserved", C.c_uint32),
                ("d_direct", C.c_void_p), ("d_state", C.c_void_p), ("env", C.c_void_p), ("d_out_select", C.c_void_p),
                ("d_out_lobe", C.c_void_p), ("d_active_count", C.c_void_p)]


SHADE_ARRAYS_ON_DEVICE = 1
TEXTURES_ON_DEVICE = 1
TEXEL_RGBA8, TEXEL_RGBA32F = 0, 1
PANORAMA_ON_DEVICE = 1
PANORAMA_MAX_DIM = 16384
STRUCT_LIGHT_SELECT = 34   # mrt_struct_size index (33: not a struct)
STRUCT_EMITTER_SELECT, STRUCT_EMITTER64 = 36, 38   # mrt_struct_size indices (35, 37: not structs)
STRUCT_SVGF_PARAMS = 32   # mrt_struct_size index (31: not a struct); the struct and the calls: svgf.py
STRUCT_GBUFFER = 30   # mrt_struct_size index (29: not a struct); the struct and the calls: gbuffer.py
STRUCT_DENOISE_PARAMS = 28   # mrt_struct_size index (27: not a struct); the struct and the calls: denoise.py
STRUCT_ACCUM_STATE = 26   # mrt_struct_size index (25: not a struct)
STRUCT_CHANNEL_OUT = 24   # mrt_struct_size index (23: not a struct)
STRUCT_PANORAMA = 22   # mrt_struct_size index (21: not a struct)
STRUCT_TEXTURE, STRUCT_MATERIAL_TEXTURES, STRUCT_TEXTURE_SET = 18, 19, 20   # mrt_struct_size indices (17: not a struct)
STRUCT_PATH_STATE, STRUCT_PATH_STEP_DESC = 15, 16   # mrt_struct_size indices (14: not a struct)
STRUCT_SHADE_LIGHT, STRUCT_ENVIRONMENT, STRUCT_LIGHT_OUT = 11, 12, 13   # mrt_struct_size indices
STRUCT_MATERIAL, STRUCT_SHADE_DATA, STRUCT_SURFACE64, STRUCT_SURFACE_OUT = 6, 7, 8, 9   # mrt_struct_size indices


class Stats(C.Structure):
    _fields_ = [("rays_cast", C.c_uint64), ("tri_tests", C.c_uint64), ("bvh_nodes_visited", C.c_uint64),
                ("hits", C.c_uint64), ("last_trace_ms", C.c_float), ("last_sort_ms", C.c_float),
                ("last_h2d_ms", C.c_float), ("last_d2h_ms", C.c_float), ("last_kernel_launches", C.c_uint32),
                ("max_stack_depth", C.c_uint32), ("dead_pops", C.c_uint64), ("detected_grid_w", C.c_uint32), ("reserved", C.c_uint32),
                ("last_build_ms", C.c_float), ("last_kernel", C.c_uint32),
                ("wave_node_fetches", C.c_uint64), ("wave_tri_fetches", C.c_uint64), ("leaf_box_checks", C.c_uint64),
                ("fetch_wait_cycles", C.c_uint64), ("wave_cycles", C.c_uint64), ("waves", C.c_uint64)]


class TwoLevelArrays(C.Structure):
    """mrt_two_level_arrays"""
    _fields_ = [("nodes", C.c_void_p), ("n_nodes", C.c_uint32), ("n_tlas_nodes", C.c_uint32),
                ("tri_hot", C.c_void_p), ("tri_cold", C.c_void_p), ("n_tris", C.c_uint32),
                ("instances", C.c_void_p), ("n_instances", C.c_uint32), ("depth", C.c_uint32)]


class SceneHostArrays(C.Structure):
    """mrt_flat_scene_arrays"""
    _fields_ = [("nodes", C.c_void_p), ("n_nodes", C.c_uint32), ("tri_hot", C.c_void_p), ("tri_cold", C.c_void_p), ("n_tris", C.c_uint32),
                ("nodes4", C.c_void_p), ("n_nodes4", C.c_uint32), ("stack4", C.c_uint32),
                ("nodes8", C.c_void_p), ("n_nodes8", C.c_uint32), ("stack8", C.c_uint32), ("leaf_box", C.c_void_p),
                ("depth", C.c_uint32), ("bounds_lo", C.c_float * 3), ("bounds_hi", C.c_float * 3)]


SNAP_COUNT = len(T.SNAPSHOT_ARRAYS)


class SnapshotInfo(C.Structure):
    """mrt_debug_snapshot_info"""
    _fields_ = [("struct_size", C.c_uint32), ("two_level", C.c_uint32), ("n_nodes", C.c_uint32), ("n_tris", C.c_uint32),
                ("n_nodes4", C.c_uint32), ("n_nodes8", C.c_uint32), ("depth", C.c_uint32), ("stack_depth", C.c_uint32),
                ("stack4", C.c_uint32), ("stack8", C.c_uint32), ("n_tlas_nodes", C.c_uint32), ("tlas_cap", C.c_uint32),
                ("n_instances", C.c_uint32), ("bounds_lo", C.c_float * 3), ("bounds_hi", C.c_float * 3), ("scene_abs_max", C.c_float),
                ("elem_bytes", C.c_uint32 * SNAP_COUNT), ("count", C.c_uint64 * SNAP_COUNT)]


_lib = None


def load():
    """Loads libmrt_hip.so; raises ImportError if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(the HIP extension is the product; there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    L.mrt_last_error.restype = C.c_char_p
    L.mrt_status_string.restype = C.c_char_p
    L.mrt_version.restype = C.c_uint32
    L.mrt_struct_size.restype = C.c_uint32
    L.mrt_struct_size.argtypes = [C.c_uint32]
    L.mrt_kernel_name.restype = C.c_char_p
    L.mrt_kernel_name.argtypes = [C.c_uint32]
    L.mrt_token_bytes.restype = C.c_uint32
    L.mrt_token_bytes.argtypes = [C.c_void_p]
    L.mrt_last_kernel_variant.restype = C.c_char_p
    L.mrt_last_kernel_variant.argtypes = [C.c_void_p]
    L.mrt_create.argtypes = [C.c_int, C.POINTER(Options), C.POINTER(C.c_void_p)]
    L.mrt_destroy.argtypes = [C.c_void_p]
    L.mrt_destroy.restype = None
    L.mrt_last_error.argtypes = [C.c_void_p]
    L.mrt_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.mrt_synchronize.argtypes = [C.c_void_p]
    L.mrt_make_triangles.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.mrt_pack_host_triangles.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.mrt_bvh2_build.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32]
    L.mrt_bvh2_save.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    L.mrt_bvh2_load.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    L.mrt_upload_scene.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    L.mrt_build_scene_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    L.mrt_flatten_instances.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.mrt_build_instanced_scene_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
    L.mrt_refit_scene.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    L.mrt_refit_instanced_scene.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
    L.mrt_refit_two_level_scene.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
    L.mrt_upload_two_level_scene.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
    L.mrt_update_instances.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.mrt_update_instances_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    L.mrt_two_level_prepare_host.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    L.mrt_two_level_host_arrays.argtypes = [C.c_void_p, C.POINTER(TwoLevelArrays)]
    L.mrt_two_level_free_host.argtypes = [C.c_void_p]
    L.mrt_two_level_free_host.restype = None
    L.mrt_scene_prepare_host.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p)]
    L.mrt_scene_host_arrays.argtypes = [C.c_void_p, C.POINTER(SceneHostArrays)]
    L.mrt_scene_free_host.argtypes = [C.c_void_p]
    L.mrt_scene_free_host.restype = None
    L.mrt_debug_snapshot.argtypes = [C.c_void_p, C.POINTER(SnapshotInfo), C.POINTER(C.c_void_p)]
    L.mrt_is_available.argtypes = [C.c_void_p]
    L.mrt_scene_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.mrt_cast.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32]
    L.mrt_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32]
    L.mrt_collect.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.mrt_has_pending.argtypes = [C.c_void_p]
    L.mrt_camera_look.argtypes = [C.POINTER(Camera), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32, C.c_uint32, C.c_float]
    L.mrt_camera_perspective.argtypes = [C.POINTER(Camera), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32, C.c_uint32, C.c_float]
    L.mrt_camera_orthographic.argtypes = [C.POINTER(Camera), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32, C.c_uint32, C.c_float]
    L.mrt_generate_grid.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.mrt_cast_grid.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                C.c_void_p, C.c_uint32, C.c_int, C.c_uint32]
    L.mrt_cast_shadows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p,
                                   C.c_uint32, C.c_uint32]
    L.mrt_cast_grid_shadows.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                        C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
    L.mrt_cast_reflections.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_float, C.c_void_p,
                                       C.c_void_p, C.c_uint32, C.c_uint32]
    L.mrt_cast_grid_reflections.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                            C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    L.mrt_cast_hemisphere.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(Hemisphere), C.c_void_p, C.c_void_p,
                                      C.c_uint32, C.c_int, C.c_uint32]
    L.mrt_cast_grid_hemisphere.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                           C.POINTER(Hemisphere), C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_uint32]
    L.mrt_cast_bounce.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(Bounce), C.c_void_p, C.c_void_p,
                                  C.c_uint32, C.c_uint32]
    L.mrt_cast_grid_bounce.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                       C.POINTER(Bounce), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    L.mrt_upload_shade_data.argtypes = [C.c_void_p, C.POINTER(ShadeData)]
    L.mrt_clear_shade_data.argtypes = [C.c_void_p]
    L.mrt_upload_textures.argtypes = [C.c_void_p, C.POINTER(TextureSet)]
    L.mrt_clear_textures.argtypes = [C.c_void_p]
    L.mrt_upload_panorama.argtypes = [C.c_void_p, C.POINTER(Panorama)]
    L.mrt_clear_panorama.argtypes = [C.c_void_p]
    L.mrt_resolve_surfaces.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(SurfaceOut), C.c_uint32]
    L.mrt_resolve_grid_surfaces.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                            C.POINTER(SurfaceOut), C.c_uint32]
    L.mrt_shadow_lights.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.mrt_light_surfaces.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p,
                                     C.c_void_p, C.POINTER(LightOut), C.c_uint32]
    L.mrt_light_grid_surfaces.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(LightOut), C.c_uint32]
    L.mrt_cast_selected_shadows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(LightSelect), C.c_void_p, C.c_uint32,
                                            C.c_void_p, C.c_uint32, C.c_uint32]
    L.mrt_cast_grid_selected_shadows.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                                 C.POINTER(LightSelect), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
    L.mrt_light_selected_surfaces.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.POINTER(LightOut), C.c_uint32]
    L.mrt_light_grid_selected_surfaces.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(LightOut),
                                                   C.c_uint32]
    L.mrt_build_emitters.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    L.mrt_clear_emitters.argtypes = [C.c_void_p]
    L.mrt_emitter_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.mrt_emitter_table.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.mrt_cast_emitter_shadows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(EmitterSelect), C.c_void_p, C.c_uint32,
                                           C.c_uint32]
    L.mrt_cast_grid_emitter_shadows.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                                C.POINTER(EmitterSelect), C.c_void_p, C.c_uint32, C.c_uint32]
    L.mrt_light_emitter_surfaces.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(EmitterSelect), C.c_void_p,
                                             C.c_uint32, C.POINTER(LightOut), C.c_uint32]
    L.mrt_light_grid_emitter_surfaces.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                                  C.c_void_p, C.POINTER(EmitterSelect), C.c_void_p, C.c_uint32, C.POINTER(LightOut), C.c_uint32]
    L.mrt_path_step_emitters.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(PathStepDesc), C.c_void_p,
                                         C.c_uint32]
    L.mrt_path_grid_step_emitters.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                              C.c_void_p, C.POINTER(PathStepDesc), C.c_void_p, C.c_uint32]
    L.mrt_path_init.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
    L.mrt_path_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(PathStepDesc), C.c_uint32]
    L.mrt_path_grid_step.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                     C.POINTER(PathStepDesc), C.c_uint32]
    L.mrt_path_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32]
    L.mrt_shade_channels.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(ChannelOut), C.c_uint32]
    L.mrt_shade_grid_channels.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                          C.POINTER(ChannelOut), C.c_uint32]
    L.mrt_finish_color.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
    L.mrt_image_to_rgba8.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32]
    L.mrt_halton_jitter.argtypes = [C.c_uint32, C.POINTER(C.c_float)]
    L.mrt_accum_begin_frame.argtypes = [C.POINTER(AccumState), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.mrt_accum_end_frame.argtypes = [C.POINTER(AccumState), C.c_uint64]
    L.mrt_accumulate.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
    L.mrt_cast_tiled.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.mrt_expand_tokens.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
    L.mrt_expand_grid_tokens.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.c_void_p, C.c_void_p, C.c_void_p]
    L.mrt_morton_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.mrt_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
    L.mrt_schedule_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.mrt_debug_sort_order.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.mrt_device_alloc.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
    L.mrt_device_free.argtypes = [C.c_void_p, C.c_void_p]
    L.mrt_memcpy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.mrt_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.mrt_group_create.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(Options), C.POINTER(C.c_void_p)]
    L.mrt_group_destroy.argtypes = [C.c_void_p]
    L.mrt_group_destroy.restype = None
    L.mrt_group_size.argtypes = [C.c_void_p]
    L.mrt_group_context.argtypes = [C.c_void_p, C.c_int]
    L.mrt_group_context.restype = C.c_void_p
    L.mrt_group_last_error.argtypes = [C.c_void_p]
    L.mrt_group_last_error.restype = C.c_char_p
    L.mrt_group_row_block.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.mrt_group_row_block.restype = None
    L.mrt_group_upload_scene.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    L.mrt_group_upload_two_level_scene.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
    L.mrt_group_cast_grid.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_uint32]
    _lib = L
    return L


def _np(a):
    return a.ctypes.data_as(C.c_void_p)


def _optr(x):
    """_ptr, or a null pointer for None (optional arguments)"""
    return None if x is None else _ptr(x)


def hemisphere_desc(n_samples, frame, first_draw, t_max, d_select=None):
    """mrt_hemisphere from its fields (d_select: device pointer / tensor or None)"""
    sel = _optr(d_select)
    return Hemisphere(n_samples, frame, first_draw, t_max, None if sel is None else sel.value)


def bounce_desc(frame, first_draw, t_max, metallic=0.0, roughness=0.5, d_select=None, d_surface=None, d_out_lobe=None):
    """mrt_bounce from its fields (d_select, d_surface, d_out_lobe: device pointers / tensors or None)"""
    v = [None if x is None else _ptr(x).value for x in (d_select, d_surface, d_out_lobe)]
    return Bounce(frame, first_draw, t_max, metallic, roughness, v[0], v[1], v[2])


def light_select_desc(frame, select_draw, d_out_light, d_select=None):
    """mrt_light_select from its fields (d_out_light, d_select: device pointers / tensors; d_select or None)"""
    return LightSelect(frame, select_draw, None if d_select is None else _ptr(d_select).value, _ptr(d_out_light).value)


def emitter_select_desc(frame, draw, d_out_emitter, d_select=None):
    """mrt_emitter_select from its fields (d_out_emitter, d_select: device pointers / tensors; d_select or None)"""
    return EmitterSelect(frame, draw, None if d_select is None else _ptr(d_select).value, _ptr(d_out_emitter).value)


def surface_out(d_rows=None, d_bounce_surface=None, d_out_hits=None):
    """mrt_surface_out from its fields (device pointers / tensors or None)"""
    v = [None if x is None else _ptr(x).value for x in (d_rows, d_bounce_surface, d_out_hits)]
    return SurfaceOut(v[0], v[1], v[2])


def channel_out(inv_depth_range, inv_pos_range, rgba=None, rgba8=None):
    """mrt_channel_out from its fields: rgba / rgba8 map a CHANNEL_* value to the device pointer / tensor of that channel's float / byte
    plane (a channel in neither is not selected)"""
    d = ChannelOut(C.sizeof(ChannelOut), 0, inv_depth_range, inv_pos_range)
    for planes, field in ((rgba, d.d_rgba), (rgba8, d.d_rgba8)):
        for c, x in (planes or {}).items():
            field[c] = None if x is None else _ptr(x).value
    return d


def shadow_lights(lights) -> np.ndarray:
    """mrt_shadow_lights: the shadow half (T.LIGHT) of each T.SHADE_LIGHT row, for cast_shadows"""
    lights = np.ascontiguousarray(lights, dtype=T.SHADE_LIGHT).reshape(-1)
    out = np.zeros(lights.shape[0], T.LIGHT)
    st = load().mrt_shadow_lights(_np(lights) if lights.shape[0] else None, lights.shape[0], _np(out) if lights.shape[0] else None)
    if st != 0:
        raise MrtError(st, "mrt_shadow_lights")
    return out


def _ptr(x):
    """numpy array -> host pointer; int -> raw (device) pointer; torch tensor -> data_ptr()."""
    if isinstance(x, np.ndarray):
        return _np(x)
    if isinstance(x, int):
        return C.c_void_p(x)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    raise TypeError(type(x))


# ---- host-side helpers (no device needed) ---------------------------------------
def make_triangles(verts9, ids=None, layers=None) -> np.ndarray:
    v = np.ascontiguousarray(verts9, dtype=np.float32).reshape(-1, 9)
    out = np.zeros(v.shape[0], dtype=T.TRI64)
    ids_a = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint32)
    lay_a = None if layers is None else np.ascontiguousarray(layers, dtype=np.uint32)
    rc = load().mrt_make_triangles(_np(v), None if ids_a is None else _np(ids_a), None if lay_a is None else _np(lay_a),
                                   v.shape[0], _np(out))
    if rc:
        raise MrtError(rc, "mrt_make_triangles")
    return out


def bvh2_build(verts4: np.ndarray, n_threads: int = 0):
    v4 = np.ascontiguousarray(verts4, dtype=np.float32)
    n = v4.shape[0] // 3
    nodes = np.zeros(2 * n + 2, dtype=T.NODE32)
    prim_idx = np.zeros(n, dtype=np.uint32)
    used = C.c_uint32(0)
    rc = load().mrt_bvh2_build(_np(v4), n, _np(nodes), _np(prim_idx), C.byref(used), n_threads)
    if rc:
        raise MrtError(rc, "mrt_bvh2_build")
    return nodes[:used.value].copy(), prim_idx, used.value


def bvh2_save(path: str, nodes: np.ndarray, prim_idx: np.ndarray) -> None:
    """BVH cache file (the counterpart of tinybvh::BVH::Save, tiny_bvh.h:1747-1758)."""
    nodes = np.ascontiguousarray(nodes)
    prim_idx = np.ascontiguousarray(prim_idx, dtype=np.uint32)
    assert nodes.dtype == T.NODE32
    rc = load().mrt_bvh2_save(os.fsencode(path), _np(nodes), nodes.shape[0], _np(prim_idx), prim_idx.shape[0])
    if rc:
        raise MrtError(rc, "mrt_bvh2_save")


def bvh2_load(path: str, n_tris: int):
    """Load a BVH saved for exactly n_tris triangles (BVH::Load, tiny_bvh.h:1770-1799); MrtError(ERR_BAD_BVH)
    if the file is for another triangle count, another version, or damaged."""
    nodes = np.zeros(2 * n_tris, dtype=T.NODE32)
    prim_idx = np.zeros(n_tris, dtype=np.uint32)
    used = C.c_uint32(0)
    rc = load().mrt_bvh2_load(os.fsencode(path), n_tris, _np(nodes), _np(prim_idx), C.byref(used))
    if rc:
        raise MrtError(rc, "mrt_bvh2_load")
    return nodes[:used.value].copy(), prim_idx, used.value


def _copy_rows(ptr, count, dtype):
    """count rows of dtype at a host pointer, copied into a numpy array (None for a null pointer)"""
    if not ptr:
        return None
    dtype = np.dtype(dtype)
    if count == 0:
        return np.zeros((0,) + dtype.shape, dtype=dtype.base)
    buf = (C.c_char * (count * dtype.itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype.base).reshape((count,) + dtype.shape).copy()


def prepare_scene_host(tris, nodes, prim_idx) -> dict:
    """mrt_scene_prepare_host: the arrays upload_scene would upload (8-wide layout included), as numpy copies.  No device."""
    tris = np.ascontiguousarray(tris)
    nodes = np.ascontiguousarray(nodes)
    prim_idx = np.ascontiguousarray(prim_idx, dtype=np.uint32)
    assert tris.dtype == T.TRI64 and nodes.dtype == T.NODE32
    L = load()
    h = C.c_void_p()
    rc = L.mrt_scene_prepare_host(_np(tris), tris.shape[0], _np(nodes), nodes.shape[0], _np(prim_idx), C.byref(h))
    if rc:
        raise MrtError(rc, "mrt_scene_prepare_host")
    try:
        a = SceneHostArrays()
        rc = L.mrt_scene_host_arrays(h, C.byref(a))
        if rc:
            raise MrtError(rc, "mrt_scene_host_arrays")
        return dict(two_level=0, n_nodes=a.n_nodes, n_tris=a.n_tris, n_nodes4=a.n_nodes4, n_nodes8=a.n_nodes8, depth=a.depth,
                    stack4=a.stack4, stack8=a.stack8, bounds_lo=np.array(a.bounds_lo[:], np.float32), bounds_hi=np.array(a.bounds_hi[:], np.float32),
                    nodes=_copy_rows(a.nodes, a.n_nodes, T.WIDE64), tri_hot=_copy_rows(a.tri_hot, a.n_tris, T.TRI_HOT),
                    tri_cold=_copy_rows(a.tri_cold, a.n_tris, T.TRI_COLD), nodes4=_copy_rows(a.nodes4, a.n_nodes4, T.NODE4),
                    nodes8=_copy_rows(a.nodes8, a.n_nodes8, T.NODE8), leaf_box=_copy_rows(a.leaf_box, a.n_tris, np.dtype(("<f4", 8))),
                    slot_src=prim_idx.copy())
    finally:
        L.mrt_scene_free_host(h)


def two_level_prepare_host(verts9, instances, n_threads: int = 1) -> dict:
    """mrt_two_level_prepare_host + mrt_two_level_host_arrays: the arrays upload_two_level_scene uploads, as numpy copies.  No device."""
    verts9 = np.ascontiguousarray(verts9, dtype=np.float32)
    instances = np.ascontiguousarray(instances)
    assert instances.dtype == T.INSTANCE
    L = load()
    h = C.c_void_p()
    rc = L.mrt_two_level_prepare_host(_np(verts9), verts9.size // 9, _np(instances), instances.shape[0], n_threads, C.byref(h))
    if rc:
        raise MrtError(rc, "mrt_two_level_prepare_host")
    try:
        a = TwoLevelArrays()
        rc = L.mrt_two_level_host_arrays(h, C.byref(a))
        if rc:
            raise MrtError(rc, "mrt_two_level_host_arrays")
        return dict(two_level=1, n_nodes=a.n_nodes, n_tlas_nodes=a.n_tlas_nodes, tlas_cap=2 * a.n_instances, n_tris=a.n_tris,
                    n_instances=a.n_instances, depth=a.depth, nodes=_copy_rows(a.nodes, a.n_nodes, T.WIDE64),
                    tri_hot=_copy_rows(a.tri_hot, a.n_tris, T.TRI_HOT), tri_cold=_copy_rows(a.tri_cold, a.n_tris, T.TRI_COLD),
                    instances=_copy_rows(a.instances, a.n_instances, T.DEV_INSTANCE))
    finally:
        L.mrt_two_level_free_host(h)


def kernel_available(kernel_id: int) -> bool:
    """Whether this build of libmrt_hip.so contains the kernel (KERNEL_PACKET_QUAD: only with MRT_WITH_QUAD=1)."""
    return bool(load().mrt_kernel_available(C.c_uint32(kernel_id)))


def kernel_name(kernel_id: int) -> str:
    return load().mrt_kernel_name(kernel_id).decode()


def halton_jitter(sample_index):
    """mrt_halton_jitter: (jitter_x, jitter_y) of frame sample_index of a progressive render"""
    j = (C.c_float * 2)()
    rc = load().mrt_halton_jitter(sample_index, j)
    if rc:
        raise MrtError(rc, "mrt_halton_jitter")
    return np.float32(j[0]), np.float32(j[1])


def accum_state(aa_enabled=True, max_samples=256) -> AccumState:
    """A fresh mrt_accum_state: the two settings, every persistent word zero"""
    st = AccumState()
    st.struct_size, st.aa_enabled, st.max_samples = C.sizeof(AccumState), int(bool(aa_enabled)), max_samples
    return st


def accum_begin_frame(st, origin, basis):
    """mrt_accum_begin_frame: the motion reset, then st.sample_index and st.jitter_x / jitter_y of the frame (basis: 3x3 row-major)"""
    o = (C.c_float * 3)(*np.asarray(origin, dtype=np.float32).reshape(3))
    b = (C.c_float * 9)(*np.asarray(basis, dtype=np.float32).reshape(9))
    rc = load().mrt_accum_begin_frame(C.byref(st), o, b)
    if rc:
        raise MrtError(rc, "mrt_accum_begin_frame")
    return st


def accum_end_frame(st, pixels):
    """mrt_accum_end_frame: st.accumulate and st.n_prior of the frame of `pixels` pixels just rendered"""
    rc = load().mrt_accum_end_frame(C.byref(st), pixels)
    if rc:
        raise MrtError(rc, "mrt_accum_end_frame")
    return st


def camera_look(origin, forward, grid_w, grid_h, fov_degrees) -> Camera:
    cam = Camera()
    o = (C.c_float * 3)(*origin)
    f = (C.c_float * 3)(*forward)
    rc = load().mrt_camera_look(C.byref(cam), o, f, grid_w, grid_h, fov_degrees)
    if rc:
        raise MrtError(rc, "mrt_camera_look")
    return cam


def ray_camera(origin, basis, width, height, param, ortho=False, jitter=(0.5, 0.5)) -> Camera:
    """RayCamera::setup (ray_camera.h:50-76): basis = 3x3 row-major camera basis; param = vertical fov in degrees
    (perspective) or Camera3D::size (orthographic); jitter = sub-pixel offset of generate_rays_tile_jittered."""
    cam = Camera()
    o = (C.c_float * 3)(*origin)
    b = (C.c_float * 9)(*np.asarray(basis, dtype=np.float32).reshape(9))
    fn = load().mrt_camera_orthographic if ortho else load().mrt_camera_perspective
    rc = fn(C.byref(cam), o, b, width, height, param)
    if rc:
        raise MrtError(rc, "mrt_camera_orthographic" if ortho else "mrt_camera_perspective")
    cam.jitter_x, cam.jitter_y = jitter
    return cam


class Context:
    """mrt_ctx wrapper: one per GPU, externally serialised (SURVEY 8(b) threading)."""

    def __init__(self, device: int = 0, kernel: int = KERNEL_AUTO, count_visits: bool = False,
                 sort_threshold: int = 0, grid_tile: int = 0, tile_w_log2: int = 0, xcd_swizzle: int = 0,
                 stack_override: int = 0, tile_order: int = 0, sort_key: int = 0, refill: int = 0,
                 leaf_wait: int = 0, extra_lds: int = 0, packet_wg: int = 0, packet_cull: int = 0, tile_schedule: int = 0):
        self.L = load()
        opts = Options()
        opts.struct_size = C.sizeof(Options)
        opts.kernel = kernel
        opts.count_visits = int(count_visits)
        opts.sort_threshold = sort_threshold
        opts.grid_tile = grid_tile
        opts.tile_w_log2 = tile_w_log2
        opts.xcd_swizzle = xcd_swizzle
        opts.stack_override = stack_override
        opts.tile_order = tile_order
        opts.sort_key = sort_key
        opts.refill = refill
        opts.leaf_wait = leaf_wait
        opts.extra_lds = extra_lds
        opts.packet_wg = packet_wg
        opts.packet_cull = packet_cull
        opts.tile_schedule = tile_schedule
        self.h = C.c_void_p()
        rc = self.L.mrt_create(device, C.byref(opts), C.byref(self.h))
        if rc:
            raise MrtError(rc, self.L.mrt_status_string(rc).decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.mrt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise MrtError(rc, self.L.mrt_last_error(self.h).decode() or self.L.mrt_status_string(rc).decode())

    def set_stream(self, stream_ptr: int):
        self._chk(self.L.mrt_set_stream(self.h, C.c_void_p(stream_ptr)))

    def synchronize(self):
        self._chk(self.L.mrt_synchronize(self.h))

    def build_scene_device(self, tris, n_tris=None, on_device=False, safe_handoff=False, ploc=False, sah=False):
        """BVH built on the device from mrt_tri64 triangles (numpy array, or a device pointer with on_device): the radix tree,
        PLOC (ploc) or the host builder's binned-SAH tree (sah)."""
        if isinstance(tris, np.ndarray):
            tris = np.ascontiguousarray(tris)
            assert tris.dtype == T.TRI64
            n_tris = tris.shape[0]
        flags = (BUILD_TRIS_ON_DEVICE if on_device else 0) | (BUILD_SAFE_HANDOFF if safe_handoff else 0) | (BUILD_PLOC if ploc else 0) | (BUILD_SAH if sah else 0)
        self._chk(self.L.mrt_build_scene_device(self.h, _ptr(tris), n_tris, flags))

    def flatten_instances(self, verts9, instances, d_out, n_mesh_tris=None, on_device=False):
        """instances: numpy array of types.INSTANCE; verts9: (n,3,3) float32 mesh-space vertices (or a device pointer)."""
        if isinstance(verts9, np.ndarray):
            verts9 = np.ascontiguousarray(verts9, dtype=np.float32)
            n_mesh_tris = verts9.size // 9
        instances = np.ascontiguousarray(instances)
        assert instances.dtype == T.INSTANCE
        self._chk(self.L.mrt_flatten_instances(self.h, _ptr(verts9), n_mesh_tris, _np(instances), instances.shape[0],
                                               BUILD_TRIS_ON_DEVICE if on_device else 0, _ptr(d_out)))

    def build_instanced_scene_device(self, verts9, instances, n_mesh_tris=None, on_device=False):
        if isinstance(verts9, np.ndarray):
            verts9 = np.ascontiguousarray(verts9, dtype=np.float32)
            n_mesh_tris = verts9.size // 9
        instances = np.ascontiguousarray(instances)
        assert instances.dtype == T.INSTANCE
        self._chk(self.L.mrt_build_instanced_scene_device(self.h, _ptr(verts9), n_mesh_tris, _np(instances), instances.shape[0],
                                                          BUILD_TRIS_ON_DEVICE if on_device else 0))

    def refit_scene(self, tris, n_tris=None, on_device=False):
        """New mrt_tri64 triangles (numpy array, or a device pointer with on_device) for the resident flat scene's tree: the same
        count and order as the array the scene came from; the tree keeps its shape and gets new boxes."""
        if isinstance(tris, np.ndarray):
            tris = np.ascontiguousarray(tris)
            assert tris.dtype == T.TRI64
            n_tris = tris.shape[0]
        self._chk(self.L.mrt_refit_scene(self.h, _ptr(tris), n_tris, BUILD_TRIS_ON_DEVICE if on_device else 0))

    def refit_instanced_scene(self, verts9, instances, n_mesh_tris=None, on_device=False):
        """The scene of build_instanced_scene_device with new mesh vertices and / or new transforms (same meshes and instances)."""
        if isinstance(verts9, np.ndarray):
            verts9 = np.ascontiguousarray(verts9, dtype=np.float32)
            n_mesh_tris = verts9.size // 9
        instances = np.ascontiguousarray(instances)
        assert instances.dtype == T.INSTANCE
        self._chk(self.L.mrt_refit_instanced_scene(self.h, _ptr(verts9), n_mesh_tris, _np(instances), instances.shape[0],
                                                   BUILD_TRIS_ON_DEVICE if on_device else 0))

    def upload_two_level_scene(self, verts9, instances, blas_on_device=False, sah=False):
        """SceneTLAS::build_tlas: one BLAS per distinct mesh, a TLAS over the instances (nothing is flattened)."""
        verts9 = np.ascontiguousarray(verts9, dtype=np.float32)
        instances = np.ascontiguousarray(instances)
        assert instances.dtype == T.INSTANCE
        self._chk(self.L.mrt_upload_two_level_scene(self.h, _np(verts9), verts9.size // 9, _np(instances), instances.shape[0],
                                                    (BUILD_BLAS_ON_DEVICE if blas_on_device else 0) | (BUILD_SAH if sah else 0)))

    def refit_two_level_scene(self, verts9, instances, n_mesh_tris=None, on_device=False, instances_on_device=False, n_instances=None):
        """The two-level scene of upload_two_level_scene with new mesh vertices (numpy array, or a device pointer with on_device)
        and the instances as given (same meshes and count; transforms and layers may change): every BLAS is refit, the TLAS rebuilt.
        instances_on_device: instances is a device pointer (an int, with n_instances) and the TLAS is built on the device."""
        if isinstance(verts9, np.ndarray):
            verts9 = np.ascontiguousarray(verts9, dtype=np.float32)
            n_mesh_tris = verts9.size // 9
        if not instances_on_device:
            instances = np.ascontiguousarray(instances)
            assert instances.dtype == T.INSTANCE
            n_instances = instances.shape[0]
        flags = (BUILD_TRIS_ON_DEVICE if on_device else 0) | (BUILD_INSTANCES_ON_DEVICE if instances_on_device else 0)
        self._chk(self.L.mrt_refit_two_level_scene(self.h, _ptr(verts9), n_mesh_tris, _ptr(instances), n_instances, flags))

    def update_instances(self, instances):
        """SceneTLAS::refit_tlas: the same instances with new transforms."""
        instances = np.ascontiguousarray(instances)
        assert instances.dtype == T.INSTANCE
        self._chk(self.L.mrt_update_instances(self.h, _np(instances), instances.shape[0]))

    def update_instances_device(self, instances, on_device=False, form="radix", n_instances=None):
        """update_instances with the top level built on the device, in the form "radix", "ploc" or "sah".  instances: a numpy array
        of types.INSTANCE (staged with one copy), or with on_device a device pointer (an int, with n_instances)."""
        if not on_device:
            instances = np.ascontiguousarray(instances)
            assert instances.dtype == T.INSTANCE
            n_instances = instances.shape[0]
        flags = TLAS_FORMS[form] | (BUILD_INSTANCES_ON_DEVICE if on_device else 0)
        self._chk(self.L.mrt_update_instances_device(self.h, _ptr(instances), n_instances, flags))

    def upload_scene(self, tris, nodes, prim_idx):
        tris = np.ascontiguousarray(tris)
        nodes = np.ascontiguousarray(nodes)
        prim_idx = np.ascontiguousarray(prim_idx, dtype=np.uint32)
        assert tris.dtype == T.TRI64 and nodes.dtype == T.NODE32
        self._chk(self.L.mrt_upload_scene(self.h, _np(tris), tris.shape[0], _np(nodes), nodes.shape[0], _np(prim_idx)))

    def is_available(self) -> bool:
        return bool(self.L.mrt_is_available(self.h))

    def debug_snapshot(self, arrays=True) -> dict:
        """mrt_debug_snapshot: the scalars of the resident scene and (arrays=True) every array it has, copied to numpy arrays named
        as types.SNAPSHOT_ARRAYS; an array the scene does not have is None.  Reads only."""
        info = SnapshotInfo()
        info.struct_size = C.sizeof(SnapshotInfo)
        self._chk(self.L.mrt_debug_snapshot(self.h, C.byref(info), None))
        out = {k: getattr(info, k) for k, _ in SnapshotInfo._fields_[1:13]}
        out["bounds_lo"] = np.array(info.bounds_lo[:], np.float32)
        out["bounds_hi"] = np.array(info.bounds_hi[:], np.float32)
        out["scene_abs_max"] = np.float32(info.scene_abs_max)
        out["counts"] = {name: int(info.count[a]) for a, (name, _) in enumerate(T.SNAPSHOT_ARRAYS)}
        if not arrays:
            return out
        bufs = (C.c_void_p * SNAP_COUNT)()
        for a, (name, dt) in enumerate(T.SNAPSHOT_ARRAYS):
            n = int(info.count[a])
            assert info.elem_bytes[a] == dt.itemsize, name
            out[name] = np.zeros((n,) + dt.shape, dtype=dt.base) if n else None
            bufs[a] = out[name].ctypes.data if n else None
        self._chk(self.L.mrt_debug_snapshot(self.h, C.byref(info), bufs))
        return out

    def scene_info(self):
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._chk(self.L.mrt_scene_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(n_tris=a.value, n_wide_nodes=b.value, stack_need=c.value)

    def cast(self, rays, hits=None, count=None, query_mask=0xFFFFFFFF, mode=MODE_NEAREST, flags=0):
        """rays / hits: numpy arrays (host) or ints / torch tensors (device, with the matching flag)."""
        if count is None:
            count = rays.shape[0]
        if hits is None:
            if flags & FLAG_BOOL_OUT:
                hits = np.zeros(count, dtype=np.uint8)
            elif flags & FLAG_TOKEN_OUT:
                hits = self._token_array(count)
            elif flags & FLAG_HOST_LAYOUT:
                hits = np.zeros(count, dtype=T.HOST_HIT44)
            else:
                hits = np.zeros(count, dtype=T.HIT32)
        if isinstance(rays, np.ndarray):
            rays = np.ascontiguousarray(rays)
        self._chk(self.L.mrt_cast(self.h, _ptr(rays), _ptr(hits), count, query_mask, mode, flags))
        return hits

    def submit(self, rays, count=None, query_mask=0xFFFFFFFF, mode=MODE_NEAREST, flags=0):
        if count is None:
            count = rays.shape[0]
        self._keep = rays  # caller must keep rays alive until collect (gpu_ray_caster.cpp:542)
        self._chk(self.L.mrt_submit(self.h, _ptr(rays), count, query_mask, mode, flags))
        self._pending = (count, mode, flags)

    def collect(self, hits=None, count=None):
        pc, mode, flags = getattr(self, "_pending", (0, 0, 0))
        if count is None:
            count = pc
        if hits is None:
            if flags & FLAG_BOOL_OUT:
                hits = np.zeros(count, dtype=np.uint8)
            elif flags & FLAG_TOKEN_OUT:
                hits = self._token_array(count)
            elif flags & FLAG_HOST_LAYOUT:
                hits = np.zeros(count, dtype=T.HOST_HIT44)
            else:
                hits = np.zeros(count, dtype=T.HIT32)
        self._chk(self.L.mrt_collect(self.h, _ptr(hits), count))
        return hits

    def has_pending(self) -> bool:
        return bool(self.L.mrt_has_pending(self.h))

    def generate_grid(self, cam, grid_w, grid_h, y0, y1, d_rays):
        self._chk(self.L.mrt_generate_grid(self.h, C.byref(cam), grid_w, grid_h, y0, y1, _ptr(d_rays)))

    def cast_grid(self, cam, grid_w, grid_h, y0=0, y1=None, hits=None, query_mask=0xFFFFFFFF, mode=MODE_NEAREST, flags=0):
        y1 = grid_h if y1 is None else y1
        n = grid_w * (y1 - y0)
        if hits is None:
            hits = np.zeros(n, dtype=np.uint8) if (flags & FLAG_BOOL_OUT) else (self._token_array(n) if (flags & FLAG_TOKEN_OUT) else np.zeros(n, dtype=T.HIT32))
        self._chk(self.L.mrt_cast_grid(self.h, C.byref(cam), grid_w, grid_h, y0, y1, _ptr(hits), query_mask, mode, flags))
        return hits

    def cast_tiled(self, d_rays, d_hits, grid_w, rows, query_mask=0xFFFFFFFF, mode=MODE_NEAREST):
        self._chk(self.L.mrt_cast_tiled(self.h, _ptr(d_rays), _ptr(d_hits), grid_w, rows, query_mask, mode))

    @staticmethod
    def _lights(lights):
        lights = np.ascontiguousarray(lights, dtype=T.LIGHT)
        return lights, (_np(lights) if lights.shape[0] else None)

    def cast_shadows(self, d_rays, d_hits, count, lights, d_mask, query_mask=0xFFFFFFFF, flags=0):
        """Shadow rays for the hit records of a cast (device pointers / tensors: mrt_ray32 + mrt_hit32, or mrt_host_ray60 +
        mrt_host_hit44 with FLAG_HOST_LAYOUT); lights: types.LIGHT array on the host.  d_mask[l * count + i] = 1 lit, 0 shadowed."""
        lights, lp = self._lights(lights)
        self._chk(self.L.mrt_cast_shadows(self.h, _ptr(d_rays), _ptr(d_hits), count, lp, lights.shape[0], _ptr(d_mask),
                                          query_mask, flags))

    def cast_grid_shadows(self, cam, grid_w, grid_h, d_hits, lights, d_mask, y0=0, y1=None, query_mask=0xFFFFFFFF, flags=0):
        """The same for rows [y0, y1) of a grid cast by cast_grid (d_hits: its mrt_hit32 records on the device)."""
        y1 = grid_h if y1 is None else y1
        lights, lp = self._lights(lights)
        self._chk(self.L.mrt_cast_grid_shadows(self.h, C.byref(cam), grid_w, grid_h, y0, y1, _ptr(d_hits), lp, lights.shape[0],
                                               _ptr(d_mask), query_mask, flags))

    def cast_selected_shadows(self, d_rays, d_hits, count, lights, d_mask, d_out_light, frame=0, select_draw=256, d_select=None,
                              query_mask=0xFFFFFFFF, flags=0):
        """One shadow ray per record, to the light the record draws uniformly from its own stream (draw select_draw; the path tracer:
        types.path_select_draw(bounce)).  d_rays / d_hits / lights as for cast_shadows; d_mask and d_out_light one byte per record: 1 lit
        / 0 shadowed, and the light selected or types.LIGHT_NONE; d_select: optional byte per record (0 = selects no light)."""
        lights, lp = self._lights(lights)
        desc = light_select_desc(frame, select_draw, d_out_light, d_select)
        self._chk(self.L.mrt_cast_selected_shadows(self.h, _ptr(d_rays), _ptr(d_hits), count, C.byref(desc), lp, lights.shape[0],
                                                   _ptr(d_mask), query_mask, flags))

    def cast_grid_selected_shadows(self, cam, grid_w, grid_h, d_hits, lights, d_mask, d_out_light, frame=0, select_draw=256, d_select=None,
                                   y0=0, y1=None, query_mask=0xFFFFFFFF, flags=0):
        """The same for rows [y0, y1) of a grid cast by cast_grid (d_hits: its mrt_hit32 records on the device; the bytes indexed by the
        record within the band); the random stream of a pixel is seeded from its index in the whole grid."""
        y1 = grid_h if y1 is None else y1
        lights, lp = self._lights(lights)
        desc = light_select_desc(frame, select_draw, d_out_light, d_select)
        self._chk(self.L.mrt_cast_grid_selected_shadows(self.h, C.byref(cam), grid_w, grid_h, y0, y1, _ptr(d_hits), C.byref(desc), lp,
                                                        lights.shape[0], _ptr(d_mask), query_mask, flags))

    def cast_reflections(self, d_rays, d_hits, count, d_out_hits, max_distance, d_select=None, d_out_rays=None,
                         query_mask=0xFFFFFFFF, flags=0):
        """Mirror-reflection rays for the hit records of a cast, traced closest-hit (device pointers / tensors: mrt_ray32 + mrt_hit32,
        or mrt_host_ray60 + mrt_host_hit44 with FLAG_HOST_LAYOUT).  d_out_hits: the records, in the input layout; d_select: optional
        byte per record (0 = no ray); d_out_rays: optional, the rays made, in the input layout."""
        self._chk(self.L.mrt_cast_reflections(self.h, _ptr(d_rays), _ptr(d_hits), count, _optr(d_select), max_distance,
                                              _ptr(d_out_hits), _optr(d_out_rays), query_mask, flags))

    def cast_grid_reflections(self, cam, grid_w, grid_h, d_hits, d_out_hits, max_distance, d_select=None, d_out_rays=None,
                              y0=0, y1=None, query_mask=0xFFFFFFFF, flags=0):
        """The same for rows [y0, y1) of a grid cast by cast_grid (d_hits: its mrt_hit32 records on the device)."""
        y1 = grid_h if y1 is None else y1
        self._chk(self.L.mrt_cast_grid_reflections(self.h, C.byref(cam), grid_w, grid_h, y0, y1, _ptr(d_hits), _optr(d_select),
                                                   max_distance, _ptr(d_out_hits), _optr(d_out_rays), query_mask, flags))

    def cast_hemisphere(self, d_rays, d_hits, count, d_out, n_samples=1, frame=0, first_draw=1, t_max=1e30, mode=MODE_NEAREST,
                        d_select=None, d_out_rays=None, query_mask=0xFFFFFFFF, flags=0):
        """Cosine-weighted hemisphere rays for the hit records of a cast (device pointers / tensors: mrt_ray32 + mrt_hit32, or
        mrt_host_ray60 + mrt_host_hit44 with FLAG_HOST_LAYOUT), n_samples per record, entry = sample * count + record.  MODE_ANY_HIT
        (ambient occlusion): d_out one byte per entry, 1 - occluded.  MODE_NEAREST (a diffuse bounce): d_out one record per entry in the
        input layout, d_out_rays (optional) the rays made.  d_select: optional byte per record (0 = no ray)."""
        desc = hemisphere_desc(n_samples, frame, first_draw, t_max, d_select)
        self._chk(self.L.mrt_cast_hemisphere(self.h, _ptr(d_rays), _ptr(d_hits), count, C.byref(desc), _ptr(d_out), _optr(d_out_rays),
                                             query_mask, mode, flags))

    def cast_grid_hemisphere(self, cam, grid_w, grid_h, d_hits, d_out, n_samples=1, frame=0, first_draw=1, t_max=1e30,
                             mode=MODE_NEAREST, d_select=None, d_out_rays=None, y0=0, y1=None, query_mask=0xFFFFFFFF, flags=0):
        """The same for rows [y0, y1) of a grid cast by cast_grid (d_hits: its mrt_hit32 records on the device); the random stream of a
        pixel is seeded from its index in the whole grid."""
        y1 = grid_h if y1 is None else y1
        desc = hemisphere_desc(n_samples, frame, first_draw, t_max, d_select)
        self._chk(self.L.mrt_cast_grid_hemisphere(self.h, C.byref(cam), grid_w, grid_h, y0, y1, _ptr(d_hits), C.byref(desc), _ptr(d_out),
                                                  _optr(d_out_rays), query_mask, mode, flags))

    def cast_bounce(self, d_rays, d_hits, count, d_out_hits, frame=0, first_draw=0, t_max=1e30, metallic=0.0, roughness=0.5,
                    d_select=None, d_surface=None, d_out_lobe=None, d_out_rays=None, query_mask=0xFFFFFFFF, flags=0):
        """The path tracer's bounce for the hit records of a cast (device pointers / tensors: mrt_ray32 + mrt_hit32, or mrt_host_ray60 +
        mrt_host_hit44 with FLAG_HOST_LAYOUT): one closest-hit ray per record, GGX-specular or cosine-diffuse by the lobe draw.
        d_out_hits one record per entry in the input layout, d_out_rays (optional) the rays made.  d_select: optional byte per record
        (0 = no ray); d_surface: optional {metallic, roughness} float pairs per record (else the two constants); d_out_lobe: optional
        byte per record, LOBE_*."""
        desc = bounce_desc(frame, first_draw, t_max, metallic, roughness, d_select, d_surface, d_out_lobe)
        self._chk(self.L.mrt_cast_bounce(self.h, _ptr(d_rays), _ptr(d_hits), count, C.byref(desc), _ptr(d_out_hits), _optr(d_out_rays),
                                         query_mask, flags))

    def cast_grid_bounce(self, cam, grid_w, grid_h, d_hits, d_out_hits, frame=0, first_draw=0, t_max=1e30, metallic=0.0, roughness=0.5,
                         d_select=None, d_surface=None, d_out_lobe=None, d_out_rays=None, y0=0, y1=None, query_mask=0xFFFFFFFF, flags=0):
        """The same for rows [y0, y1) of a grid cast by cast_grid (d_hits: its mrt_hit32 records on the device; d_select, d_surface and
        d_out_lobe indexed by the record within the band); the random stream of a pixel is seeded from its index in the whole grid."""
        y1 = grid_h if y1 is None else y1
        desc = bounce_desc(frame, first_draw, t_max, metallic, roughness, d_select, d_surface, d_out_lobe)
        self._chk(self.L.mrt_cast_grid_bounce(self.h, C.byref(cam), grid_w, grid_h, y0, y1, _ptr(d_hits), C.byref(desc), _ptr(d_out_hits),
                                              _optr(d_out_rays), query_mask, flags))

    def upload_shade_data(self, n_tris, materials=None, material_ids=None, normals9=None, uvs6=None, on_device=False):
        """Makes the shade data of the context resident (mrt_upload_shade_data).  materials: a host array of T.MATERIAL or None; the
        three per-triangle arrays, each optional: numpy arrays (uint32 [n_tris], float32 [n_tris, 9], float32 [n_tris, 6]) or, with
        on_device, device pointers / tensors.  Indexed by the prim_id a record carries; replaced by the next upload."""
        mats = None if materials is None else np.ascontiguousarray(materials, dtype=T.MATERIAL)
        keep = [mats]
        ptrs = []
        for a, dt in ((material_ids, np.uint32), (normals9, np.float32), (uvs6, np.float32)):
            if a is not None and not on_device:
                a = np.ascontiguousarray(a, dtype=dt)
                keep.append(a)
            ptrs.append(None if a is None else _ptr(a).value)
        d = ShadeData(C.sizeof(ShadeData), n_tris, 0 if mats is None else mats.shape[0], SHADE_ARRAYS_ON_DEVICE if on_device else 0,
                      None if mats is None or mats.shape[0] == 0 else _np(mats).value, ptrs[0], ptrs[1], ptrs[2])
        self._chk(self.L.mrt_upload_shade_data(self.h, C.byref(d)))

    def clear_shade_data(self):
        self._chk(self.L.mrt_clear_shade_data(self.h))

    def upload_textures(self, textures=(), bindings=None, tangents12=None, n_tangent_tris=None, on_device=False):
        """Makes a texture set resident (mrt_upload_textures).  textures: [height, width, 4] numpy arrays, uint8 (RGBA8) or float32
        (RGBA32F), or with on_device (width, height, format, device pointer / tensor) tuples; bindings: a host array of
        T.MATERIAL_TEXTURES indexed by the material id, or None; tangents12: float32 [n, 12] indexed by prim_id, or with on_device a
        device pointer / tensor and n_tangent_tris, or None.  While a set is resident the two resolves sample it."""
        keep, tex = [], (Texture * max(len(textures), 1))()
        for k, im in enumerate(textures):
            if on_device:
                w, h, fmt, ptr = im
                tex[k] = Texture(w, h, fmt, 0, _ptr(ptr).value)
            else:
                im = np.ascontiguousarray(im)
                if im.ndim != 3 or im.shape[2] != 4 or im.dtype not in (np.uint8, np.float32):
                    raise ValueError("a texture is a [height, width, 4] array of uint8 or float32")
                keep.append(im)
                tex[k] = Texture(im.shape[1], im.shape[0], TEXEL_RGBA8 if im.dtype == np.uint8 else TEXEL_RGBA32F, 0, _np(im).value)
        bind = None if bindings is None else np.ascontiguousarray(bindings, dtype=T.MATERIAL_TEXTURES)
        n_tan, tan_ptr = 0, None
        if tangents12 is not None:
            if on_device:
                n_tan, tan_ptr = int(n_tangent_tris), _ptr(tangents12).value
            else:
                tan = np.ascontiguousarray(tangents12, dtype=np.float32).reshape(-1, 12)
                keep.append(tan)
                n_tan, tan_ptr = tan.shape[0], (_np(tan).value if tan.shape[0] else None)
        d = TextureSet(C.sizeof(TextureSet), TEXTURES_ON_DEVICE if on_device else 0, len(textures), 0 if bind is None else bind.shape[0],
                       n_tan, 0, C.cast(tex, C.c_void_p).value if len(textures) else None,
                       None if bind is None or bind.shape[0] == 0 else _np(bind).value, tan_ptr)
        self._chk(self.L.mrt_upload_textures(self.h, C.byref(d)))

    def clear_textures(self):
        self._chk(self.L.mrt_clear_textures(self.h))

    def upload_panorama(self, pixels, energy=1.0, on_device=False, size=None):
        """Makes an equirectangular panorama resident (mrt_upload_panorama).  pixels: a [height, width, 4] float32 numpy array, top row
        first, or with on_device a device pointer / tensor and size = (width, height).  While one is resident the lighting calls
        with an environment and the path steps sample it for the sky of a miss (and the lighting calls for a hit's ambient factor)."""
        if on_device:
            (w, h), ptr, keep = size, _ptr(pixels).value, None
        else:
            keep = np.ascontiguousarray(pixels, dtype=np.float32)
            if keep.ndim != 3 or keep.shape[2] != 4:
                raise ValueError("a panorama is a [height, width, 4] array of float32")
            (h, w), ptr = keep.shape[:2], _np(keep).value
        d = Panorama(ptr, w, h, energy, PANORAMA_ON_DEVICE if on_device else 0)
        self._chk(self.L.mrt_upload_panorama(self.h, C.byref(d)))

    def clear_panorama(self):
        self._chk(self.L.mrt_clear_panorama(self.h))

    def resolve_surfaces(self, d_rays, d_hits, count, d_rows=None, d_bounce_surface=None, d_out_hits=None, flags=0):
        """The shading surface of every hit record of a cast (device pointers / tensors: mrt_ray32 + mrt_hit32, or mrt_host_ray60 +
        mrt_host_hit44 with FLAG_HOST_LAYOUT) against the resident shade data.  Outputs, each optional, at least one: d_rows one
        T.SURFACE64 per record; d_bounce_surface {metallic, roughness} float pairs, cast_bounce's d_surface; d_out_hits the records in
        the input layout with the shading normal in place of the normal."""
        out = surface_out(d_rows, d_bounce_surface, d_out_hits)
        self._chk(self.L.mrt_resolve_surfaces(self.h, _ptr(d_rays), _ptr(d_hits), count, C.byref(out), flags))

    def resolve_grid_surfaces(self, cam, grid_w, grid_h, d_hits, d_rows=None, d_bounce_surface=None, d_out_hits=None, y0=0, y1=None,
                              flags=0):
        """The same for rows [y0, y1) of a grid cast by cast_grid (d_hits: its mrt_hit32 records on the device; the outputs indexed by
        the record within the band)."""
        y1 = grid_h if y1 is None else y1
        out = surface_out(d_rows, d_bounce_surface, d_out_hits)
        self._chk(self.L.mrt_resolve_grid_surfaces(self.h, C.byref(cam), grid_w, grid_h, y0, y1, _ptr(d_hits), C.byref(out), flags))

    @staticmethod
    def _shade_lights(lights, env):
        lights = np.ascontiguousarray(lights, dtype=T.SHADE_LIGHT).reshape(-1)
        env = None if env is None else np.ascontiguousarray(env, dtype=T.ENVIRONMENT).reshape(1)
        return lights, (_np(lights) if lights.shape[0] else None), env, (None if env is None else _np(env))

    def light_surfaces(self, d_rays, d_hits, d_rows, count, lights, d_rgba, d_mask=None, env=None, flags=0):
        """Direct light (Cook-Torrance over all lights) on the rows resolve_surfaces wrote, for the records of a cast (device pointers /
        tensors: mrt_ray32 + mrt_hit32, or mrt_host_ray60 + mrt_host_hit44 with FLAG_HOST_LAYOUT).  lights: T.SHADE_LIGHT array on the
        host; d_mask: optional, what cast_shadows wrote for shadow_lights(lights); env: optional T.ENVIRONMENT row (sky for a miss,
        ambient and emission for a hit).  d_rgba: 4 floats per record."""
        lights, lp, env, ep = self._shade_lights(lights, env)
        out = LightOut(_ptr(d_rgba).value)
        self._chk(self.L.mrt_light_surfaces(self.h, _ptr(d_rays), _ptr(d_hits), _ptr(d_rows), count, lp, lights.shape[0], _optr(d_mask),
                                            ep, C.byref(out), flags))

    def light_grid_surfaces(self, cam, grid_w, grid_h, d_hits, d_rows, lights, d_rgba, d_mask=None, env=None, y0=0, y1=None, flags=0):
        """The same for rows [y0, y1) of a grid cast by cast_grid (d_hits: its mrt_hit32 records on the device; d_rows, d_mask and d_rgba
        indexed by the record within the band)."""
        y1 = grid_h if y1 is None else y1
        lights, lp, env, ep = self._shade_lights(lights, env)
        out = LightOut(_ptr(d_rgba).value)
        self._chk(self.L.mrt_light_grid_surfaces(self.h, C.byref(cam), grid_w, grid_h, y0, y1, _ptr(d_hits), _ptr(d_rows), lp,
                                                 lights.shape[0], _optr(d_mask), ep, C.byref(out), flags))

    def light_selected_surfaces(self, d_rays, d_hits, d_rows, count, lights, d_light, d_rgba, d_mask=None, env=None, flags=0):
        """Direct light of the one light each record selected, scaled by the number of lights: light_surfaces' arguments, with d_light
        one byte per record (cast_selected_shadows' d_out_light) and d_mask one byte per record (its d_mask) or None.  With env=None
        d_rgba is what path_step takes as d_direct."""
        lights, lp, env, ep = self._shade_lights(lights, env)
        out = LightOut(_ptr(d_rgba).value)
        self._chk(self.L.mrt_light_selected_surfaces(self.h, _ptr(d_rays), _ptr(d_hits), _ptr(d_rows), count, lp, lights.shape[0],
                                                     _ptr(d_light), _optr(d_mask), ep, C.byref(out), flags))

    def light_grid_selected_surfaces(self, cam, grid_w, grid_h, d_hits, d_rows, lights, d_light, d_rgba, d_mask=None, env=None, y0=0, y1=None,
                                     flags=0):
        """The same for rows [y0, y1) of a grid cast by cast_grid (every per-record array indexed by the record within the band)."""
        y1 = grid_h if y1 is None else y1
        lights, lp, env, ep = self._shade_lights(lights, env)
        out = LightOut(_ptr(d_rgba).value)
        self._chk(self.L.mrt_light_grid_selected_surfaces(self.h, C.byref(cam), grid_w, grid_h, y0, y1, _ptr(d_hits), _ptr(d_rows), lp,
                                                          lights.shape[0], _ptr(d_light), _optr(d_mask), ep, C.byref(out), flags))

    def build_emitters(self, tris, n_tris=None, on_device=False):
        """Builds the resident emitter table from the scene's world-space triangles (T.TRI64 rows on the host, or a device pointer with
        on_device and n_tris) and the resident shade data; returns (number of emitters, sum of their integer weights)."""
        if isinstance(tris, np.ndarray):
            tris = np.ascontiguousarray(tris, dtype=T.TRI64)
            n_tris = tris.shape[0]
        self._chk(self.L.mrt_build_emitters(self.h, _ptr(tris) if n_tris else None, n_tris, BUILD_TRIS_ON_DEVICE if on_device else 0))
        return self.emitter_info()

    def clear_emitters(self):
        self._chk(self.L.mrt_clear_emitters(self.h))

    def emitter_info(self):
        n, total = C.c_uint32(0), C.c_uint32(0)
        self._chk(self.L.mrt_emitter_info(self.h, C.byref(n), C.byref(total)))
        return n.value, total.value

    def emitter_table(self):
        """The resident table: (rows [n] T.EMITTER64, cdf [n] uint32)."""
        n = self.emitter_info()[0]
        rows, cdf = np.zeros(n, T.EMITTER64), np.zeros(n, np.uint32)
        self._chk(self.L.mrt_emitter_table(self.h, _np(rows), _np(cdf), n))
        return rows, cdf

    def cast_emitter_shadows(self, d_rays, d_hits, count, d_mask, d_out_emitter, frame=0, draw=512, d_select=None, query_mask=0xFFFFFFFF,
                             flags=0):
        """One shadow ray per record, to a point of the emitter the record samples from the resident table (draws draw .. draw + 2 of its
        stream; the path tracer: types.path_emitter_draw(bounce)).  d_mask one byte per record: 1 lit / 0 shadowed; d_out_emitter one
        uint32 per record: the emitter or types.EMITTER_NONE; d_select: optional byte per record (0 = samples no emitter)."""
        desc = emitter_select_desc(frame, draw, d_out_emitter, d_select)
        self._chk(self.L.mrt_cast_emitter_shadows(self.h, _ptr(d_rays), _ptr(d_hits), count, C.byref(desc), _ptr(d_mask), query_mask, flags))

    def cast_grid_emitter_shadows(self, cam, grid_w, grid_h, d_hits, d_mask, d_out_emitter, frame=0, draw=512, d_select=None, y0=0, y1=None,
                                  query_mask=0xFFFFFFFF, flags=0):
        """The same for rows [y0, y1) of a grid cast by cast_grid; the stream of a pixel is seeded from its index in the whole grid."""
        y1 = grid_h if y1 is None else y1
        desc = emitter_select_desc(frame, draw, d_out_emitter, d_select)
        self._chk(self.L.mrt_cast_grid_emitter_shadows(self.h, C.byref(cam), grid_w, grid_h, y0, y1, _ptr(d_hits), C.byref(desc), _ptr(d_mask),
                                                       query_mask, flags))

    def light_emitter_surfaces(self, d_rays, d_hits, d_rows, count, d_emitter, d_rgba, d_mask=None, frame=0, draw=512, accumulate=False, flags=0):
        """The diffuse term of the emitter point each record sampled (d_emitter, d_mask: what cast_emitter_shadows wrote with the same
        frame and draw).  accumulate: added to what d_rgba holds, else written."""
        desc = emitter_select_desc(frame, draw, d_emitter)
        out = LightOut(_ptr(d_rgba).value)
        self._chk(self.L.mrt_light_emitter_surfaces(self.h, _ptr(d_rays), _ptr(d_hits), _ptr(d_rows), count, C.byref(desc), _optr(d_mask),
                                                    EMITTER_ACCUMULATE if accumulate else 0, C.byref(out), flags))

    def light_grid_emitter_surfaces(self, cam, grid_w, grid_h, d_hits, d_rows, d_emitter, d_rgba, d_mask=None, frame=0, draw=512,
                                    accumulate=False, y0=0, y1=None, flags=0):
        """The same for rows [y0, y1) of a grid cast by cast_grid (every per-record array indexed by the record within the band)."""
        y1 = grid_h if y1 is None else y1
        desc = emitter_select_desc(frame, draw, d_emitter)
        out = LightOut(_ptr(d_rgba).value)
        self._chk(self.L.mrt_light_grid_emitter_surfaces(self.h, C.byref(cam), grid_w, grid_h, y0, y1, _ptr(d_hits), _ptr(d_rows), C.byref(desc),
                                                         _optr(d_mask), EMITTER_ACCUMULATE if accumulate else 0, C.byref(out), flags))

    def path_step_emitters(self, d_rays, d_hits, d_rows, count, d_direct, d_state, env, d_out_select, d_prev_lobe, frame=0, bounce=0,
                           max_bounces=4, d_out_lobe=None, d_active_count=None, flags=0):
        """path_step for a loop that samples emitters: from bounce 1 on the emission of a hit is added only where d_prev_lobe (the lobe
        bytes of the step before; None at bounce 0; may be d_out_lobe) says the ray came from the specular lobe."""
        desc, env = self._path_desc(frame, bounce, max_bounces, d_direct, d_state, env, d_out_select, d_out_lobe, d_active_count)
        self._chk(self.L.mrt_path_step_emitters(self.h, _ptr(d_rays), _ptr(d_hits), _ptr(d_rows), count, C.byref(desc), _optr(d_prev_lobe), flags))

    def path_grid_step_emitters(self, cam, grid_w, grid_h, d_hits, d_rows, d_direct, d_state, env, d_out_select, d_prev_lobe, frame=0, bounce=0,
                                max_bounces=4, d_out_lobe=None, d_active_count=None, y0=0, y1=None, flags=0):
        """The same for rows [y0, y1) of a grid cast by cast_grid (every per-record array indexed by the record within the band)."""
        y1 = grid_h if y1 is None else y1
        desc, env = self._path_desc(frame, bounce, max_bounces, d_direct, d_state, env, d_out_select, d_out_lobe, d_active_count)
        self._chk(self.L.mrt_path_grid_step_emitters(self.h, C.byref(cam), grid_w, grid_h, y0, y1, _ptr(d_hits), _ptr(d_rows), C.byref(desc),
                                                     _optr(d_prev_lobe), flags))

    def path_init(self, d_state, count, flags=0):
        """Every T.PATH_STATE entry to throughput 1, active, radiance 0."""
        self._chk(self.L.mrt_path_init(self.h, _ptr(d_state), count, flags))

    @staticmethod
    def _path_desc(frame, bounce, max_bounces, d_direct, d_state, env, d_out_select, d_out_lobe, d_active_count):
        env = np.ascontiguousarray(env, dtype=T.ENVIRONMENT).reshape(1)
        desc = PathStepDesc(frame, bounce, max_bounces, 0, _ptr(d_direct).value, _ptr(d_state).value, _np(env).value,
                            _ptr(d_out_select).value, _optr(d_out_lobe).value if d_out_lobe is not None else None,
                            _optr(d_active_count).value if d_active_count is not None else None)
        return desc, env

    def path_step(self, d_rays, d_hits, d_rows, count, d_direct, d_state, env, d_out_select, frame=0, bounce=0, max_bounces=4,
                  d_out_lobe=None, d_active_count=None, flags=0):
        """One bounce of the path tracer's per-pixel state for the records of a cast (device pointers / tensors: mrt_ray32 + mrt_hit32,
        or mrt_host_ray60 + mrt_host_hit44 with FLAG_HOST_LAYOUT; the records with the shading normal, resolve_surfaces' d_out_hits):
        radiance and throughput of d_state advanced in place from d_rows and d_direct (light_surfaces with env=None), Russian roulette,
        d_out_select for the cast_bounce that follows.  env: T.ENVIRONMENT row; d_active_count: optional zeroed word."""
        desc, env = self._path_desc(frame, bounce, max_bounces, d_direct, d_state, env, d_out_select, d_out_lobe, d_active_count)
        self._chk(self.L.mrt_path_step(self.h, _ptr(d_rays), _ptr(d_hits), _ptr(d_rows), count, C.byref(desc), flags))

    def path_grid_step(self, cam, grid_w, grid_h, d_hits, d_rows, d_direct, d_state, env, d_out_select, frame=0, bounce=0, max_bounces=4,
                       d_out_lobe=None, d_active_count=None, y0=0, y1=None, flags=0):
        """The same for rows [y0, y1) of a grid cast by cast_grid (every per-record array indexed by the record within the band)."""
        y1 = grid_h if y1 is None else y1
        desc, env = self._path_desc(frame, bounce, max_bounces, d_direct, d_state, env, d_out_select, d_out_lobe, d_active_count)
        self._chk(self.L.mrt_path_grid_step(self.h, C.byref(cam), grid_w, grid_h, y0, y1, _ptr(d_hits), _ptr(d_rows), C.byref(desc), flags))

    def path_finish(self, d_state, count, d_rgba, tonemap_mode=0, flags=0):
        """The frame's last pass: tone mapping (0 linear, 1 Reinhard, 2 Hable, 3 ACES, 4 AgX) and gamma 2.2 of every entry's radiance,
        4 floats per entry with alpha 1."""
        self._chk(self.L.mrt_path_finish(self.h, _ptr(d_state), count, tonemap_mode, _ptr(d_rgba), flags))

    def shade_channels(self, d_rays, d_hits, count, inv_depth_range, inv_pos_range, rgba=None, rgba8=None, flags=0):
        """The renderer's channels besides COLOR for the records of a cast (device pointers / tensors: mrt_ray32 + mrt_hit32, or
        mrt_host_ray60 + mrt_host_hit44 with FLAG_HOST_LAYOUT) against the resident shade data and textures.  rgba / rgba8: dicts from a
        CHANNEL_* value to that channel's plane, 4 floats / 4 bytes per record; a channel in either is shaded."""
        out = channel_out(inv_depth_range, inv_pos_range, rgba, rgba8)
        self._chk(self.L.mrt_shade_channels(self.h, _ptr(d_rays), _ptr(d_hits), count, C.byref(out), flags))

    def shade_grid_channels(self, cam, grid_w, grid_h, d_hits, inv_depth_range, inv_pos_range, rgba=None, rgba8=None, y0=0, y1=None, flags=0):
        """The same for rows [y0, y1) of a grid cast by cast_grid (d_hits: its mrt_hit32 records on the device; the planes indexed by
        the record within the band)."""
        y1 = grid_h if y1 is None else y1
        out = channel_out(inv_depth_range, inv_pos_range, rgba, rgba8)
        self._chk(self.L.mrt_shade_grid_channels(self.h, C.byref(cam), grid_w, grid_h, y0, y1, _ptr(d_hits), C.byref(out), flags))

    def finish_color(self, d_lit_rgba, count, d_rgba=None, d_rgba8=None, tonemap_mode=0, flags=0):
        """The last pass of a lit frame (what light_surfaces wrote with an environment): tone mapping and gamma 2.2 on the hits, the sky
        as it is on the misses, alpha 1; d_rgba (may be d_lit_rgba) 4 floats per record, d_rgba8 its 8-bit image, at least one."""
        self._chk(self.L.mrt_finish_color(self.h, _ptr(d_lit_rgba), count, tonemap_mode, _optr(d_rgba), _optr(d_rgba8), flags))

    def image_to_rgba8(self, d_rgba, count, d_rgba8, flags=0):
        """The 8-bit image of a float plane: 4 bytes per record."""
        self._chk(self.L.mrt_image_to_rgba8(self.h, _ptr(d_rgba), count, _ptr(d_rgba8), flags))

    def accumulate(self, source_kind, d_source, count, d_accum, n_prior, d_rgba8=None, tonemap_mode=0, flags=0):
        """One frame into the running mean of a progressive render: d_accum (4 floats per pixel) takes the sample when n_prior == 0, else
        acc + (s - acc) * (1 / (n_prior + 1)); d_rgba8 (optional) the mean's 8-bit image.  source_kind: ACCUM_SRC_RGBA (4 floats per
        pixel as they are), ACCUM_SRC_LIT (a lit frame, finished as finish_color would) or ACCUM_SRC_PATH_STATE (T.PATH_STATE entries,
        finished as path_finish would)."""
        self._chk(self.L.mrt_accumulate(self.h, source_kind, _ptr(d_source), count, tonemap_mode, n_prior, _ptr(d_accum), _optr(d_rgba8), flags))

    def expand_tokens(self, d_rays, d_tokens, d_hits, count, flags=0, stream=None):
        """Device pointers; enqueued on `stream` (raw hipStream_t) or the context's stream, not waited for."""
        self._chk(self.L.mrt_expand_tokens(self.h, _ptr(d_rays), _ptr(d_tokens), _ptr(d_hits), count, flags,
                                           C.c_void_p(stream) if stream else None))

    def expand_grid_tokens(self, cam, grid_w, grid_h, y0, y1, d_tokens, d_hits, stream=None):
        self._chk(self.L.mrt_expand_grid_tokens(self.h, C.byref(cam), grid_w, grid_h, y0, y1, _ptr(d_tokens), _ptr(d_hits),
                                                C.c_void_p(stream) if stream else None))

    def morton_keys(self, d_rays, count, d_keys):
        self._chk(self.L.mrt_morton_keys(self.h, _ptr(d_rays), count, _ptr(d_keys)))

    def stats(self) -> dict:
        s = Stats()
        self._chk(self.L.mrt_get_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in Stats._fields_}

    def schedule_counts(self) -> dict:
        """mrt_schedule_counts: casts planned under the tile schedule, those launched in a measured order, sorts queued"""
        c = (C.c_uint64 * 3)()
        self._chk(self.L.mrt_schedule_counts(self.h, c))
        return dict(scheduled=int(c[0]), ordered=int(c[1]), sorts=int(c[2]))

    def debug_sort_order(self, count) -> np.ndarray:
        """mrt_debug_sort_order: the order in which the last sorted cast of `count` rays walked them"""
        out = np.zeros(count, dtype=np.uint32)
        self._chk(self.L.mrt_debug_sort_order(self.h, _np(out), count))
        return out

    def _token_array(self, count):
        """host array for `count` hit tokens: uint32[count] (flat scene) or uint32[count, 2] (two-level: {triangle, instance})"""
        words = self.token_bytes() // 4
        return np.zeros(count if words == 1 else (count, words), dtype=np.uint32)

    def token_bytes(self) -> int:
        """Bytes per hit token (MRT_FLAG_TOKEN_OUT): 4 for a flat scene, 8 ({triangle, instance}) for a two-level one."""
        return int(self.L.mrt_token_bytes(self.h))

    def last_kernel_variant(self) -> str:
        """The instantiation that ran the last blocking cast, as rocprofv3 spells kernel names."""
        return self.L.mrt_last_kernel_variant(self.h).decode()

    def device_alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._chk(self.L.mrt_device_alloc(self.h, nbytes, C.byref(p)))
        return p.value

    def device_free(self, ptr: int):
        self._chk(self.L.mrt_device_free(self.h, C.c_void_p(ptr)))

    def h2d(self, d_ptr: int, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        self._chk(self.L.mrt_memcpy_h2d(self.h, C.c_void_p(d_ptr), _np(arr), arr.nbytes))

    def d2h(self, arr: np.ndarray, d_ptr: int):
        self._chk(self.L.mrt_memcpy_d2h(self.h, _np(arr), C.c_void_p(d_ptr), arr.nbytes))


class Group:
    """mrt_group wrapper: several devices of one node driven from this process (rows of a grid sharded over them)."""

    def __init__(self, devices, **opts_kw):
        self.L = load()
        opts = Options()
        opts.struct_size = C.sizeof(Options)
        for k, v in opts_kw.items():
            setattr(opts, k, v)
        devs = (C.c_int * len(devices))(*devices)
        self.h = C.c_void_p()
        rc = self.L.mrt_group_create(len(devices), devs, C.byref(opts), C.byref(self.h))
        if rc:
            raise MrtError(rc, self.L.mrt_status_string(rc).decode())

    def _chk(self, rc):
        if rc:
            raise MrtError(rc, self.L.mrt_group_last_error(self.h).decode() or self.L.mrt_status_string(rc).decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.mrt_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self) -> int:
        return self.L.mrt_group_size(self.h)

    def upload(self, scene: "Scene"):
        tris, nodes, prim_idx = np.ascontiguousarray(scene.tris), np.ascontiguousarray(scene.nodes), np.ascontiguousarray(scene.prim_idx, dtype=np.uint32)
        self._chk(self.L.mrt_group_upload_scene(self.h, _np(tris), tris.shape[0], _np(nodes), nodes.shape[0], _np(prim_idx)))

    def upload_two_level_scene(self, verts9, instances, blas_on_device=False, sah=False):
        verts9 = np.ascontiguousarray(verts9, dtype=np.float32)
        instances = np.ascontiguousarray(instances)
        self._chk(self.L.mrt_group_upload_two_level_scene(self.h, _np(verts9), verts9.size // 9, _np(instances), instances.shape[0],
                                                          (BUILD_BLAS_ON_DEVICE if blas_on_device else 0) | (BUILD_SAH if sah else 0)))

    def cast_grid(self, cam, grid_w, grid_h, hits=None, query_mask=0xFFFFFFFF, mode=MODE_NEAREST, flags=0):
        if hits is None:
            hits = np.zeros(grid_w * grid_h, dtype=np.uint8 if (flags & FLAG_BOOL_OUT) else T.HIT32)
        self._chk(self.L.mrt_group_cast_grid(self.h, C.byref(cam), grid_w, grid_h, _ptr(hits), query_mask, mode, flags))
        return hits


def group_row_block(member: int, n_members: int, rows: int):
    y0, y1 = C.c_uint32(), C.c_uint32()
    load().mrt_group_row_block(member, n_members, rows, C.byref(y0), C.byref(y1))
    return y0.value, y1.value


class Scene:
    """Host-side scene: Triangle ctor -> 8-bin SAH BVH2, i.e. what RayScene::build
    hands to upload_scene (src/accel/ray_scene.h:62-86)."""

    def __init__(self, verts9, ids=None, layers=None, n_threads: int = 0):
        self.tris = make_triangles(verts9, ids, layers)
        self.verts4 = T.verts4_from_verts9(verts9)
        self.nodes, self.prim_idx, self.used_nodes = bvh2_build(self.verts4, n_threads)

    def upload(self, ctx: Context):
        ctx.upload_scene(self.tris, self.nodes, self.prim_idx)

    def save_bvh(self, path: str) -> None:
        bvh2_save(path, self.nodes, self.prim_idx)

    @classmethod
    def with_cached_bvh(cls, verts9, path: str, ids=None, layers=None, n_threads: int = 0):
        """The scene with its BVH taken from the cache file if it fits, else built (and saved)."""
        self = cls.__new__(cls)
        self.tris = make_triangles(verts9, ids, layers)
        self.verts4 = T.verts4_from_verts9(verts9)
        try:
            self.nodes, self.prim_idx, self.used_nodes = bvh2_load(path, self.tris.shape[0])
        except MrtError:
            self.nodes, self.prim_idx, self.used_nodes = bvh2_build(self.verts4, n_threads)
            bvh2_save(path, self.nodes, self.prim_idx)
        return self
