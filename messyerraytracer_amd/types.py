"""numpy mirrors of the PODs in include/mrt_hip.h.

Device layouts == GLSL std430 structs of the reference
(src/api/gpu_types.h:44-126, src/gpu/gpu_structs.h:41-47); host layouts == the
reference's Ray / Intersection / Triangle at precision=single
(src/core/ray.h:25-51, src/core/intersection.h:16-40, src/core/triangle.h:22-39).
"""
import numpy as np

RAY32 = np.dtype([("origin", "<f4", 3), ("t_max", "<f4"), ("direction", "<f4", 3), ("t_min", "<f4")])
HIT32 = np.dtype([("t", "<f4"), ("prim_id", "<i4"), ("bary_u", "<f4"), ("bary_v", "<f4"),
                  ("normal", "<f4", 3), ("hit_layers", "<u4")])
TRI64 = np.dtype([("v0", "<f4", 3), ("id", "<u4"), ("edge1", "<f4", 3), ("layers", "<u4"),
                  ("edge2", "<f4", 3), ("pad2", "<f4"), ("normal", "<f4", 3), ("pad3", "<f4")])
NODE32 = np.dtype([("aabb_min", "<f4", 3), ("left_first", "<u4"), ("aabb_max", "<f4", 3), ("tri_count", "<u4")])
WIDE64 = np.dtype([("left_min", "<f4", 3), ("left_idx", "<u4"), ("left_max", "<f4", 3), ("right_idx", "<u4"),
                   ("right_min", "<f4", 3), ("left_count", "<u4"), ("right_max", "<f4", 3), ("right_count", "<u4")])
HOST_RAY60 = np.dtype([("origin", "<f4", 3), ("direction", "<f4", 3), ("inv_direction", "<f4", 3),
                       ("dir_sign", "<i4", 3), ("t_min", "<f4"), ("t_max", "<f4"), ("flags", "<u4")])
HOST_HIT44 = np.dtype([("t", "<f4"), ("position", "<f4", 3), ("normal", "<f4", 3), ("u", "<f4"), ("v", "<f4"),
                       ("prim_id", "<u4"), ("hit_layers", "<u4")])
HOST_TRI80 = np.dtype([("v0", "<f4", 3), ("v1", "<f4", 3), ("v2", "<f4", 3), ("edge1", "<f4", 3),
                       ("edge2", "<f4", 3), ("normal", "<f4", 3), ("id", "<u4"), ("layers", "<u4")])

INSTANCE = np.dtype([("first_tri", "<u4"), ("n_tris", "<u4"), ("layers", "<u4"), ("reserved", "<u4"),
                     ("basis", "<f4", 9), ("origin", "<f4", 3)])  # mrt_instance

LIGHT = np.dtype([("type", "<u4"), ("cast_shadows", "<u4"), ("position", "<f4", 3), ("direction", "<f4", 3)])  # mrt_light
LIGHT_DIRECTIONAL, LIGHT_POINT, LIGHT_SPOT = 0, 1, 2
MAX_LIGHTS = 16

# shading surfaces (mrt_upload_shade_data, mrt_resolve_surfaces)
MATERIAL = np.dtype([("albedo", "<f4", 3), ("metallic", "<f4"), ("roughness", "<f4"), ("specular", "<f4"), ("emission", "<f4", 3),
                     ("emission_energy", "<f4"), ("flags", "<u4"), ("reserved", "<u4")])  # mrt_material
SURFACE64 = np.dtype([("normal", "<f4", 3), ("n_dot_v", "<f4"), ("albedo", "<f4", 3), ("metallic", "<f4"), ("emission", "<f4", 3),
                      ("roughness", "<f4"), ("uv", "<f4", 2), ("specular", "<f4"), ("material", "<u4")])  # mrt_surface64
DEFAULT_MATERIAL = 0xFFFFFFFF
assert MATERIAL.itemsize == 48 and SURFACE64.itemsize == 64

# resident textures (mrt_upload_textures)
MATERIAL_TEXTURES = np.dtype([("albedo_texture", "<u4"), ("normal_texture", "<u4"), ("normal_scale", "<f4"), ("reserved", "<u4")])  # mrt_material_textures
NO_TEXTURE, TEXTURE_MAX_DIM = 0xFFFFFFFF, 16384
assert MATERIAL_TEXTURES.itemsize == 16

# direct light on resolved surfaces (mrt_light_surfaces)
SHADE_LIGHT = np.dtype([("type", "<u4"), ("cast_shadows", "<u4"), ("position", "<f4", 3), ("direction", "<f4", 3), ("color", "<f4", 3),
                        ("range", "<f4"), ("attenuation", "<f4"), ("spot_angle", "<f4"), ("spot_angle_attenuation", "<f4"),
                        ("reserved", "<u4")])  # mrt_shade_light: mrt_light, then the rest of LightData
ENVIRONMENT = np.dtype([("sky_zenith", "<f4", 3), ("sky_horizon", "<f4", 3), ("sky_ground", "<f4", 3), ("ambient", "<f4", 3),
                        ("ambient_energy", "<f4"), ("reserved", "<u4", 3)])  # mrt_environment
assert SHADE_LIGHT.itemsize == 64 and ENVIRONMENT.itemsize == 64

# the path tracer's per-pixel state (mrt_path_init, mrt_path_step, mrt_path_finish)
PATH_STATE = np.dtype([("throughput", "<f4", 3), ("active", "<u4"), ("radiance", "<f4", 3), ("reserved", "<u4")])  # mrt_path_state
PATH_MAX_FRAME, PATH_MAX_BOUNCES = 999999, 32
assert PATH_STATE.itemsize == 32

# next-event estimation with one light per record (mrt_cast_selected_shadows, mrt_light_selected_surfaces)
LIGHT_SELECT = np.dtype([("frame", "<u4"), ("select_draw", "<u4"), ("d_select", "<u8"), ("d_out_light", "<u8")])  # mrt_light_select
LIGHT_NONE = 0xFF
assert LIGHT_SELECT.itemsize == 24


def path_select_draw(bounce):
    """MRT_PATH_SELECT_DRAW: the draw of a pixel's stream that selects bounce b's light"""
    return 256 + int(bounce)


# emissive triangles as light sources (mrt_build_emitters, mrt_cast_emitter_shadows, mrt_light_emitter_surfaces)
EMITTER_SELECT = np.dtype([("frame", "<u4"), ("draw", "<u4"), ("d_select", "<u8"), ("d_out_emitter", "<u8")])  # mrt_emitter_select
EMITTER64 = np.dtype([("v0", "<f4", 3), ("q", "<u4"), ("edge1", "<f4", 3), ("prim_id", "<u4"), ("edge2", "<f4", 3), ("area", "<f4"),
                      ("radiance", "<f4", 3), ("material", "<u4")])  # mrt_emitter64
EMITTER_NONE = 0xFFFFFFFF
MAX_EMITTERS = 1 << 20
assert EMITTER_SELECT.itemsize == 24 and EMITTER64.itemsize == 64


def path_emitter_draw(bounce):
    """MRT_PATH_EMITTER_DRAW: the first of the three draws of a pixel's stream that bounce b's emitter sample takes"""
    return 512 + 4 * int(bounce)


# rows of the device layouts (csrc/mrt_internal.h), as mrt_debug_snapshot and the host preparations return them
TRI_HOT = np.dtype([("v0", "<f4", 3), ("id", "<u4"), ("e1", "<f4", 3), ("layers", "<u4"), ("e2", "<f4", 3), ("flags", "<u4")])
TRI_COLD = np.dtype([("normal", "<f4", 3), ("pad", "<u4")])
NODE4 = np.dtype([("box", "<f4", (4, 6)), ("ref", "<u4", 4), ("n_children", "<u4"), ("pad", "<u4", 3)])
NODE8 = np.dtype([("org", "<f4", 3), ("exp", "u1", 3), ("n_children", "u1"), ("qlo", "u1", (3, 8)), ("qhi", "u1", (3, 8)),
                  ("ref", "<u4", 8), ("pad", "<u4", 8)])
DEV_INSTANCE = np.dtype([("inv", "<f4", 12), ("basis", "<f4", 9), ("root", "<u4"), ("id_base", "<u4"), ("layers", "<u4"),
                         ("flags", "<u4"), ("index", "<u4"), ("root8", "<u4"), ("pad", "<u4", 5)])
# mrt_debug_snapshot: array index -> (name, row dtype)
SNAPSHOT_ARRAYS = [("nodes", WIDE64), ("tri_hot", TRI_HOT), ("tri_cold", TRI_COLD), ("nodes4", NODE4), ("nodes8", NODE8),
                   ("leaf_box", np.dtype(("<f4", 8))), ("slot_src", np.dtype("<u4")), ("parent", np.dtype("<u4")),
                   ("rows", np.dtype(("<u4", 16))), ("rows4", np.dtype(("<u4", 16))), ("instances", DEV_INSTANCE)]

assert INSTANCE.itemsize == 64 and LIGHT.itemsize == 32
assert TRI_HOT.itemsize == 48 and TRI_COLD.itemsize == 16 and NODE4.itemsize == 128 and NODE8.itemsize == 128 and DEV_INSTANCE.itemsize == 128
assert RAY32.itemsize == 32 and HIT32.itemsize == 32 and TRI64.itemsize == 64
assert NODE32.itemsize == 32 and WIDE64.itemsize == 64
assert HOST_RAY60.itemsize == 60 and HOST_HIT44.itemsize == 44 and HOST_TRI80.itemsize == 80

FLT_MAX = np.float32(3.4028234663852886e38)
NO_HIT = 0xFFFFFFFF


def verts4_from_verts9(verts9: np.ndarray) -> np.ndarray:
    """(n,3,3) float32 vertices -> (3n,4) bvhvec4 array (w = 0), the input of
    tinybvh::BVH::Build (src/accel/tinybvh_adapter.h:42-55)."""
    v = np.ascontiguousarray(verts9, dtype=np.float32).reshape(-1, 3)
    out = np.zeros((v.shape[0], 4), dtype=np.float32)
    out[:, :3] = v
    return out
