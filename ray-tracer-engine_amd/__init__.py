"""ray-tracer-engine_amd -- Python host binding of the MI355X-native ray-tracing
hot path (C ABI: include/rt_engine.h, library: csrc/librt_engine.so).

This package is plumbing around the C ABI: ctypes structures that mirror the
reference's kernel-argument types (/root/reference/kernel.cu:38-40, 225-262,
265-358, 1246-1261; sprite.h:11-47), a `Scene` wrapper over the device-resident
scene, and helpers to build the default scene of the reference
(kernel.cu:1189-1192, 1695-1712). PyTorch is used only for device buffers,
streams and torch.distributed.

There is NO CPU fallback: if the HIP library is missing or no GPU is present the
render calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RT_ENGINE_LIB") or os.path.join(_HERE, "csrc", "librt_engine.so")   # env: tuning builds only

# torch bundles a HIP runtime with the same soname as /opt/rocm's; it has to be
# in the process first so that the engine binds to that single runtime.
try:  # pragma: no cover - exercised implicitly
    import torch  # noqa: F401
except Exception:  # torch is optional for pure-host helpers
    torch = None

RT_MAX_LIGHTS = 8
RT_MAX_SPP = 16
RT_MAX_REFLECT_DEPTH = 8
RT_STATS_COUNT = 24
STAT_NAMES = ("primary_tests", "shadow_tests", "cull_tests", "hit_pixels", "unshadowed",
              "wave_test_slots", "list_entries", "list_overflows",
              "cyc_ray_setup", "cyc_primary_cull", "cyc_primary_tests", "cyc_shade_sky", "cyc_beam_bound",
              "cyc_shadow_cull", "cyc_sample_dirs", "cyc_shadow_tests",
              "clusters", "waves_lt5us", "waves_lt10us", "waves_lt20us", "waves_lt40us", "waves_lt80us", "waves_lt160us",
              "waves_ge160us")


class RtError(RuntimeError):
    pass


# ----------------------------------------------------------------------------
# ctypes mirrors of include/rt_engine.h
# ----------------------------------------------------------------------------
class Vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class Ray(C.Structure):
    _fields_ = [("Org", Vec3), ("Dir", Vec3)]


class Camera(C.Structure):
    _fields_ = [("Org", Vec3), ("Dir", Vec3), ("aspect", C.c_float),
                ("Camyaw", C.c_float), ("Campitch", C.c_float)]


class Light(C.Structure):
    _fields_ = [("pos", Vec3), ("size", C.c_float), ("r", C.c_float), ("g", C.c_float), ("b", C.c_float)]


class Sphere(C.Structure):
    _fields_ = [("vptr_slot", C.c_void_p), ("orgin", Vec3), ("reflective", C.c_uint8),
                ("pad_", C.c_uint8 * 3), ("radius", C.c_float), ("tail_pad_", C.c_uint32)]


class Plane(C.Structure):
    _fields_ = [("vptr_slot", C.c_void_p), ("orgin", Vec3), ("reflective", C.c_uint8), ("pad_", C.c_uint8 * 3),
                ("normal", Vec3), ("tail_pad_", C.c_uint32)]


class Cube(C.Structure):
    _fields_ = [("vptr_slot", C.c_void_p), ("orgin", Vec3), ("normals", Vec3 * 3), ("bounds", Vec3 * 2)]


class Vec2(C.Structure):
    _fields_ = [("u", C.c_float), ("v", C.c_float)]


class Triangle(C.Structure):
    _fields_ = [("points", Vec3 * 3), ("normal", Vec3), ("vecNormal", Vec3 * 3), ("vt", Vec2 * 3)]


class BvhBox(C.Structure):
    _fields_ = [("bvhbox", C.POINTER(Cube)), ("d_bvhbox", C.POINTER(Cube)), ("indexes", C.POINTER(C.c_int)),
                ("d_indexes", C.POINTER(C.c_int)), ("length", C.c_int)]


class Mesh(C.Structure):
    _fields_ = [("d_tri_arr", C.POINTER(Triangle)), ("h_tri_arr", C.POINTER(Triangle)), ("poly_count", C.c_int),
                ("bvhbox_count", C.c_int), ("bvhLayer_count", C.c_int), ("has_normals", C.c_uint8),
                ("h_box", C.POINTER(BvhBox)), ("d_box", C.POINTER(BvhBox)), ("indexes", C.POINTER(C.c_int))]


class Buffer(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_float)), ("size", C.c_int)]


class Sprite(C.Structure):
    _fields_ = [("rBuff", C.POINTER(Buffer)), ("gBuff", C.POINTER(Buffer)), ("bBuff", C.POINTER(Buffer)),
                ("width", C.c_int), ("height", C.c_int)]


class Skybox(C.Structure):
    _fields_ = [("box", C.POINTER(Sphere)), ("skyboxTex", C.POINTER(Sprite))]


class Object(C.Structure):
    _fields_ = [("sphere_count", C.c_int), ("plane_count", C.c_int), ("cube_count", C.c_int),
                ("depth", C.c_int), ("s1", C.POINTER(Sphere)), ("d_spheres", C.POINTER(Sphere)),
                ("c1", C.POINTER(Cube)), ("d_cubes", C.POINTER(Cube)), ("planes", C.POINTER(Plane)),
                ("d_planes", C.POINTER(Plane)), ("mesh1", C.POINTER(Mesh)), ("texture", C.POINTER(Sprite)),
                ("mat", C.c_void_p), ("tot_mesh", C.c_void_p), ("meshes", C.c_int)]


class LaunchOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("rgba", C.c_void_p), ("y0", C.c_int), ("y1", C.c_int),
                ("spp", C.c_int), ("sample_base", C.c_int), ("sample_total", C.c_int),
                ("accumulate", C.c_int), ("resolve", C.c_int), ("cull", C.c_int), ("tile", C.c_int),
                ("stats", C.c_void_p), ("force_slow_path", C.c_int), ("profile", C.c_int),
                ("interleave_count", C.c_int), ("interleave_index", C.c_int), ("interleave_rows", C.c_int),
                ("packed24", C.c_void_p), ("table_lds", C.c_int), ("fast", C.c_int), ("reflect_depth", C.c_int)]


# G-buffer outputs (rt_frame_desc.aov_*): name -> (dtype name, components per pixel)
AOV_NAMES = ("depth", "normal", "id", "albedo")
_AOV_LAYOUT = {"depth": ("float32", 1), "normal": ("float32", 4), "id": ("int32", 2), "albedo": ("float32", 4)}


class Material(C.Structure):
    """rt_material (material, kernel.cu:213-224): only reflectivness is implemented."""
    _fields_ = [("reflectivness", C.c_float), ("transperancy", C.c_float), ("roughness", C.c_float)]


class MaterialEx(C.Structure):
    """rt_material_ex: a material with transparency and an index of refraction (16 bytes)."""
    _fields_ = [("reflectivness", C.c_float), ("transperancy", C.c_float), ("roughness", C.c_float), ("ior", C.c_float)]


class ReflectStats(C.Structure):
    _fields_ = [("bvh_build_ms", C.c_double), ("bvh_nodes", C.c_int), ("bvh_depth", C.c_int), ("bvh_leaves", C.c_int),
                ("depth", C.c_int), ("queue", C.c_int * (RT_MAX_REFLECT_DEPTH + 1)),
                ("pass_ms", C.c_float * (RT_MAX_REFLECT_DEPTH + 2)), ("timed", C.c_int)]


RT_HIT_NONE, RT_HIT_TRIANGLE, RT_HIT_SPHERE, RT_HIT_PLANE, RT_HIT_CUBE = -1, 0, 1, 2, 3
RT_QUERY_NEAREST, RT_QUERY_OCCLUDED, RT_QUERY_SHADE = 0, 1, 2
RT_MAX_QUERY_RAYS = 1 << 26
_QUERY_MODES = {"nearest": RT_QUERY_NEAREST, "occluded": RT_QUERY_OCCLUDED, "shade": RT_QUERY_SHADE}
RT_REFLECT_SPHERES, RT_REFLECT_SCENE = 0, 1     # rt_scene_set_reflect_scope
_REFLECT_SCOPES = {"spheres": RT_REFLECT_SPHERES, "scene": RT_REFLECT_SCENE}
RT_REFLECT_SAMPLES_ONE, RT_REFLECT_SAMPLES_MANY = 0, 1     # rt_scene_set_reflect_samples
_REFLECT_SAMPLES = {"one": RT_REFLECT_SAMPLES_ONE, "many": RT_REFLECT_SAMPLES_MANY}
_ROUGH_KINDS = {"sphere": RT_HIT_SPHERE, "plane": RT_HIT_PLANE, "cube": RT_HIT_CUBE}   # Scene.set_roughness
RT_GLASS_PLAIN, RT_GLASS_FRESNEL = 0, 1     # rt_scene_set_glass_model
_GLASS_MODELS = {"plain": RT_GLASS_PLAIN, "fresnel": RT_GLASS_FRESNEL}


class Hit(C.Structure):
    """rt_hit: castRay's outputs for one ray (64 bytes)."""
    _fields_ = [("t", C.c_float), ("kind", C.c_int), ("index", C.c_int), ("u", C.c_float), ("v", C.c_float),
                ("tx", C.c_float), ("ty", C.c_float), ("normal", Vec3), ("new_org", Vec3), ("pad_", C.c_uint32 * 3)]


class RayQuery(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int), ("n", C.c_int), ("cull", C.c_int),
                ("rays", C.c_void_p), ("hits", C.c_void_p), ("occluded", C.c_void_p), ("rgba", C.c_void_p),
                ("packed", C.c_void_p)]


class FrameDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int), ("height", C.c_int),
                ("aspect", C.c_float), ("cam", Camera), ("pixels", C.c_void_p), ("opts", LaunchOpts),
                ("aov_depth", C.c_void_p), ("aov_normal", C.c_void_p), ("aov_id", C.c_void_p), ("aov_albedo", C.c_void_p)]


class DenoiseDesc(C.Structure):
    """rt_denoise_desc."""
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int), ("height", C.c_int),
                ("rgba_in", C.c_void_p), ("depth", C.c_void_p), ("normal", C.c_void_p), ("albedo", C.c_void_p),
                ("id", C.c_void_p), ("rgba_out", C.c_void_p), ("pixels", C.c_void_p),
                ("iterations", C.c_int), ("normal_shift", C.c_int), ("sigma_depth", C.c_float),
                ("sigma_colour", C.c_float), ("demodulate", C.c_int), ("variant", C.c_int)]


class VDenoiseDesc(C.Structure):
    """rt_vdenoise_desc."""
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int), ("height", C.c_int),
                ("rgba_in", C.c_void_p), ("depth", C.c_void_p), ("normal", C.c_void_p), ("albedo", C.c_void_p),
                ("id", C.c_void_p), ("rgba_out", C.c_void_p), ("pixels", C.c_void_p),
                ("moments", C.c_void_p), ("variance_out", C.c_void_p),
                ("iterations", C.c_int), ("normal_shift", C.c_int), ("sigma_depth", C.c_float),
                ("sigma_colour", C.c_float), ("sigma_floor", C.c_float), ("min_history", C.c_int),
                ("spatial_boost", C.c_float), ("demodulate", C.c_int), ("variant", C.c_int)]


class TemporalDesc(C.Structure):
    """rt_temporal_desc."""
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int), ("height", C.c_int),
                ("aspect", C.c_float), ("cam", Camera), ("prev_aspect", C.c_float), ("prev_cam", Camera),
                ("rgba_in", C.c_void_p), ("depth", C.c_void_p), ("normal", C.c_void_p), ("id", C.c_void_p),
                ("prev_rgba", C.c_void_p), ("prev_depth", C.c_void_p), ("prev_normal", C.c_void_p),
                ("prev_id", C.c_void_p), ("prev_moments", C.c_void_p),
                ("rgba_out", C.c_void_p), ("moments_out", C.c_void_p), ("pixels", C.c_void_p),
                ("reset", C.c_int), ("max_history", C.c_int), ("depth_tolerance", C.c_float),
                ("normal_cos_min", C.c_float), ("variant", C.c_int)]


class TMotionDesc(C.Structure):
    """rt_tmotion_desc: rt_temporal_desc's fields, then the motion and the clamp."""
    _fields_ = TemporalDesc._fields_ + [("sphere_motion", C.c_void_p), ("n_sphere_motion", C.c_int),
                                        ("cube_motion", C.c_void_p), ("n_cube_motion", C.c_int),
                                        ("clamp", C.c_int), ("clamp_slack", C.c_float), ("clamp_history", C.c_int)]


class UpsampleDesc(C.Structure):
    """rt_upsample_desc."""
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int), ("height", C.c_int),
                ("lo_width", C.c_int), ("lo_height", C.c_int),
                ("rgba_lo", C.c_void_p), ("depth_lo", C.c_void_p), ("normal_lo", C.c_void_p), ("albedo_lo", C.c_void_p),
                ("id_lo", C.c_void_p),
                ("depth", C.c_void_p), ("normal", C.c_void_p), ("albedo", C.c_void_p), ("id", C.c_void_p),
                ("base", C.c_void_p), ("rgba_out", C.c_void_p), ("pixels", C.c_void_p), ("source", C.c_void_p),
                ("sphere_select", C.c_void_p), ("n_sphere_select", C.c_int),
                ("plane_select", C.c_void_p), ("n_plane_select", C.c_int),
                ("cube_select", C.c_void_p), ("n_cube_select", C.c_int),
                ("use_tables", C.c_int), ("normal_shift", C.c_int), ("sigma_depth", C.c_float),
                ("demodulate", C.c_int), ("variant", C.c_int)]


class IndirectDesc(C.Structure):
    """rt_indirect_desc."""
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int), ("height", C.c_int),
                ("aspect", C.c_float), ("cam", Camera),
                ("depth", C.c_void_p), ("normal", C.c_void_p), ("id", C.c_void_p), ("albedo", C.c_void_p),
                ("rgba_in", C.c_void_p), ("rgba_out", C.c_void_p), ("pixels", C.c_void_p),
                ("rays", C.c_int), ("ray_base", C.c_int), ("seed", C.c_uint32), ("strength", C.c_float),
                ("cull", C.c_int), ("variant", C.c_int)]


RT_INDIRECT_MAX_RAYS = 16


class DisplayDesc(C.Structure):
    """rt_display_desc."""
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int), ("height", C.c_int),
                ("rgba_in", C.c_void_p), ("id", C.c_void_p), ("rgba_out", C.c_void_p), ("pixels", C.c_void_p),
                ("state", C.c_void_p), ("histogram_out", C.c_void_p),
                ("meter", C.c_int), ("exposure", C.c_float), ("key", C.c_float), ("min_exposure", C.c_float),
                ("max_exposure", C.c_float), ("meter_low", C.c_int), ("meter_high", C.c_int), ("adapt", C.c_float),
                ("meter_sky", C.c_int), ("curve", C.c_int), ("white", C.c_float), ("transfer", C.c_int),
                ("variant", C.c_int)]


RT_DISPLAY_BINS = 512
RT_DISPLAY_METER_MANUAL, RT_DISPLAY_METER_AUTO, RT_DISPLAY_METER_LAGGED = 0, 1, 2
RT_DISPLAY_CLIP, RT_DISPLAY_REINHARD, RT_DISPLAY_ACES = 0, 1, 2
RT_DISPLAY_LINEAR, RT_DISPLAY_SRGB = 0, 1
_DISPLAY_METERS = {"manual": RT_DISPLAY_METER_MANUAL, "auto": RT_DISPLAY_METER_AUTO, "lagged": RT_DISPLAY_METER_LAGGED}
_DISPLAY_CURVES = {"clip": RT_DISPLAY_CLIP, "reinhard": RT_DISPLAY_REINHARD, "aces": RT_DISPLAY_ACES}
_DISPLAY_TRANSFERS = {"linear": RT_DISPLAY_LINEAR, "srgb": RT_DISPLAY_SRGB}


class BloomDesc(C.Structure):
    """rt_bloom_desc."""
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int), ("height", C.c_int),
                ("rgba_in", C.c_void_p), ("state", C.c_void_p), ("rgba_out", C.c_void_p), ("pixels", C.c_void_p),
                ("glow_out", C.c_void_p),
                ("levels", C.c_int), ("threshold", C.c_float), ("limit", C.c_float), ("spread", C.c_float),
                ("strength", C.c_float), ("variant", C.c_int)]


RT_BLOOM_MAX_LEVELS = 8
RT_BLOOM_MAX_EVENTS = 16


class IndirectPathsOpts(C.Structure):
    """rt_indirect_paths_opts."""
    _fields_ = [("struct_size", C.c_uint32), ("bounces", C.c_int)]


RT_INDIRECT_MAX_BOUNCES = 4


class ViewListsInfo(C.Structure):
    """rt_view_lists_info."""
    _fields_ = [("read", C.c_int), ("block_w", C.c_int), ("block_h", C.c_int), ("blocks_x", C.c_int), ("blocks_y", C.c_int),
                ("blocks", C.c_int), ("overflowed", C.c_int), ("not_built", C.c_int), ("longest", C.c_int), ("mean", C.c_float)]


class LightVerdictsInfo(C.Structure):
    """rt_light_verdicts_info."""
    _fields_ = [("state", C.c_int), ("slot", C.c_int), ("tiles_x", C.c_int), ("tiles_y", C.c_int), ("unwritten", C.c_int),
                ("nothing", C.c_longlong), ("clear", C.c_longlong)]


class ShadowCountsInfo(C.Structure):
    """rt_shadow_counts_info."""
    _fields_ = [("state", C.c_int), ("slot", C.c_int), ("tiles_x", C.c_int), ("tiles_y", C.c_int), ("records", C.c_int),
                ("tagged", C.c_longlong), ("tiles_tagged", C.c_longlong), ("tagged_all", C.c_longlong)]


class PrimaryRecordsInfo(C.Structure):
    """rt_primary_records_info."""
    _fields_ = [("state", C.c_int), ("slot", C.c_int), ("tiles_x", C.c_int), ("tiles_y", C.c_int), ("tile_w", C.c_int),
                ("tiles_recorded", C.c_longlong), ("hit_pixels", C.c_longlong), ("miss_pixels", C.c_longlong)]


class CompactLaunchInfo(C.Structure):
    """rt_compact_launch_info."""
    _fields_ = [("compact", C.c_int), ("n_unsettled", C.c_uint), ("n_streamed", C.c_uint), ("run", C.c_uint), ("workgroups", C.c_uint), ("ahead", C.c_int),
                ("rebuilds", C.c_ulonglong), ("list_built", C.c_int), ("tiles_x", C.c_int), ("tiles_y", C.c_int),
                ("list_n_unsettled", C.c_uint), ("list_n_streamed", C.c_uint)]


class TileSummariesInfo(C.Structure):
    """rt_tile_summaries_info."""
    _fields_ = [("state", C.c_int), ("slot", C.c_int), ("tiles_x", C.c_int), ("tiles_y", C.c_int),
                ("settled", C.c_longlong), ("settled_no_miss", C.c_longlong)]


RT_PRIMARY_MISS, RT_PRIMARY_NONE = 0xff, 0xfe
RT_TILE_SETTLED, RT_TILE_NO_MISS, RT_TILE_GROUPS_SHIFT = 1, 2, 8


def decode_primary_records(dwords):
    """uint32 records -> (entry uint8: position in the tile's view list, RT_PRIMARY_MISS, RT_PRIMARY_NONE; texel int64)."""
    d = np.asarray(dwords, dtype=np.uint32)
    return (d & np.uint32(0xff)).astype(np.uint8), (d >> np.uint32(8)).astype(np.int64)


def encode_primary_records(entry, texel):
    """The inverse of decode_primary_records (texel < 2^24)."""
    return (np.asarray(entry).astype(np.uint32) & np.uint32(0xff)) | (np.asarray(texel).astype(np.uint32) << np.uint32(8))


def tiles_to_pixels(a, tile_w):
    """[tiles_y, tiles_x, 64] (lane = row in tile * tile_w + column in tile) -> [tiles_y * 64 / tile_w, tiles_x * tile_w], the
    launch's grid of pixels in local rows."""
    ty, tx, _ = a.shape
    th = 64 // tile_w
    return a.reshape(ty, tx, th, tile_w).transpose(0, 2, 1, 3).reshape(ty * th, tx * tile_w)


def pixels_to_tiles(a, tile_w):
    """The inverse of tiles_to_pixels."""
    th = 64 // tile_w
    ty, tx = a.shape[0] // th, a.shape[1] // tile_w
    return np.ascontiguousarray(a.reshape(ty, th, tx, tile_w).transpose(0, 2, 1, 3)).reshape(ty, tx, 64)


RT_VIEW_CAP = 64
RT_VIEW_SLOT = 1 + RT_VIEW_CAP + RT_VIEW_CAP // 4 + RT_VIEW_CAP // 4    # 16-byte records per block
RT_VIEW_OVERFLOW, RT_VIEW_NOT_BUILT = 1, 2

RT_DENOISE_MAX_ITERATIONS = 6
RT_DENOISE_MAX_NORMAL_SHIFT = 8
RT_TEMPORAL_MAX_HISTORY = 256

_lib = None


def load_library():
    """dlopen the HIP extension. Raises if it has not been built: the product
    path never substitutes a CPU implementation."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RtError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      "or `make -C ray-tracer-engine_amd/csrc` (there is no CPU fallback)")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    fp = C.POINTER(C.c_float)
    sig = {
        "rt_abi_version": (ci, []),
        "rt_last_error": (C.c_char_p, []),
        "rt_device_count": (ci, []),
        "rt_set_soft_errors": (ci, [ci]),
        "rt_check": (None, [ci, C.c_char_p, C.c_char_p, ci]),
        "rt_managed_alloc": (vp, [C.c_size_t]),
        "rt_managed_free": (None, [vp]),
        "rt_launch_raytrace": (ci, [vp, ci, ci, cf, C.POINTER(Object), C.POINTER(Light), ci, Camera,
                                    C.POINTER(Skybox), vp]),
        "rt_launch_raytrace_ex": (ci, [vp, ci, ci, cf, C.POINTER(Object), C.POINTER(Light), ci, Camera,
                                       C.POINTER(Skybox), vp, C.POINTER(LaunchOpts)]),
        "rt_invalidate_textures": (None, []),
        "rt_on_start": (None, []),
        "rt_update": (None, []),
        "rt_config_set_sphere_count": (ci, [ci]),
        "rt_config_set_seed": (ci, [C.c_uint]),
        "rt_config_set_assets": (ci, [C.c_char_p, C.c_char_p, C.c_char_p]),
        "rt_config_camera": (C.POINTER(Camera), []),
        "rt_config_lights": (C.POINTER(Light), [C.POINTER(ci)]),
        "rt_default_aspect": (cf, []),
        "rt_last_frame_ms": (C.c_double, []),
        "rt_offscreen_resize": (ci, [ci, ci]),
        "rt_offscreen_pixels": (C.POINTER(C.c_uint32), []),
        "rt_offscreen_width": (ci, []),
        "rt_offscreen_height": (ci, []),
        "rt_offscreen_write_ppm": (ci, [C.c_char_p]),
        "rt_sphere_init": (None, [C.POINTER(Sphere), cf, cf, cf, cf]),
        "rt_generate_spheres": (ci, [C.POINTER(Sphere), ci, C.c_uint]),
        "rt_mesh_from_obj_text": (C.POINTER(Mesh), [C.c_char_p]),
        "rt_mesh_load_obj": (C.POINTER(Mesh), [C.c_char_p]),
        "rt_mesh_free": (None, [C.POINTER(Mesh)]),
        "rt_scene_set_mesh": (ci, [vp, C.POINTER(Mesh)]),
        "rt_plane_init": (None, [C.POINTER(Plane), cf, cf, cf, cf, cf, cf]),
        "rt_cube_init": (None, [C.POINTER(Cube), cf, cf, cf, cf, cf, cf]),
        "rt_scene_set_planes": (ci, [vp, C.POINTER(Plane), ci]),
        "rt_scene_set_cubes": (ci, [vp, C.POINTER(Cube), ci]),
        "rt_msvc_rand_sequence": (ci, [C.c_uint, C.POINTER(ci), ci]),
        "rt_synth_texture_size": (ci, [ci, C.POINTER(ci), C.POINTER(ci)]),
        "rt_synth_texture": (ci, [ci, fp, fp, fp]),
        "rt_load_ppm": (ci, [C.c_char_p, C.POINTER(fp), C.POINTER(fp), C.POINTER(fp), C.POINTER(ci), C.POINTER(ci)]),
        "rt_free_planes": (None, [fp, fp, fp]),
        "rt_sample_offset": (ci, [ci, ci, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "rt_scene_create": (vp, []),
        "rt_scene_destroy": (None, [vp]),
        "rt_scene_set_spheres": (ci, [vp, C.POINTER(Sphere), ci]),
        "rt_scene_set_texture": (ci, [vp, fp, fp, fp, ci, ci]),
        "rt_scene_set_sky": (ci, [vp, C.POINTER(Sphere), fp, fp, fp, ci, ci]),
        "rt_scene_set_lights": (ci, [vp, C.POINTER(Light), ci]),
        "rt_scene_set_tile_order": (ci, [vp, ci]),
        "rt_scene_set_view_lists": (ci, [vp, ci]),
        "rt_scene_set_light_verdicts": (ci, [vp, ci]),
        "rt_debug_light_verdicts": (ci, [vp, C.POINTER(LightVerdictsInfo), C.POINTER(C.c_uint64), C.c_size_t]),
        "rt_debug_shim_scene": (vp, []),
        "rt_debug_shadow_counts": (ci, [vp, C.POINTER(ShadowCountsInfo), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.c_size_t]),
        "rt_debug_set_shadow_counts": (ci, [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.c_size_t]),
        "rt_debug_primary_records": (ci, [vp, C.POINTER(PrimaryRecordsInfo), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.c_size_t]),
        "rt_debug_set_primary_records": (ci, [vp, C.POINTER(C.c_uint32), C.c_size_t]),
        "rt_debug_tile_summaries": (ci, [vp, C.POINTER(TileSummariesInfo), C.POINTER(C.c_uint32), C.c_size_t]),
        "rt_debug_set_tile_summaries": (ci, [vp, C.POINTER(C.c_uint32), C.c_size_t]),
        "rt_scene_set_compact_launch": (ci, [vp, ci]),
        "rt_debug_compact_launch": (ci, [vp, C.POINTER(CompactLaunchInfo), C.POINTER(C.c_uint32), C.c_size_t]),
        "rt_debug_set_compact_run": (ci, [vp, ci, ci, ci]),
        "rt_debug_compact_order": (ci, [vp, C.POINTER(C.c_uint32), C.c_size_t]),
        "rt_scene_view_lists_info": (ci, [vp, C.POINTER(ViewListsInfo), fp, C.c_size_t]),
        "rt_debug_view_lists_host": (ci, [C.POINTER(Sphere), ci, C.POINTER(FrameDesc), C.POINTER(ViewListsInfo), fp, C.c_size_t, fp]),
        "rt_debug_tile_order": (ci, [C.POINTER(C.c_uint), ci, ci, ci, C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_uint)]),
        "rt_scene_render": (ci, [vp, C.POINTER(FrameDesc), vp]),
        "rt_graph_capture": (vp, [vp, C.POINTER(FrameDesc), ci, vp, vp]),
        "rt_graph_launch": (ci, [vp, vp]),
        "rt_graph_set_camera": (ci, [vp, C.POINTER(Camera)]),
        "rt_graph_destroy": (None, [vp]),
        "rt_debug_math": (ci, [ci, fp, fp, fp, ci]),
        "rt_debug_launch_floor": (ci, [ci, ci, C.POINTER(ci), ci, ci, ci, ci, fp]),
        "rt_debug_intersect": (ci, [C.POINTER(Sphere), C.POINTER(Ray), ci, C.POINTER(ci), fp]),
        "rt_debug_light": (ci, [C.POINTER(Sphere), ci, C.POINTER(Vec3), C.POINTER(Vec3), C.POINTER(Light), ci, fp, fp]),
        "rt_debug_shortcuts": (ci, [ci, C.c_uint, C.c_longlong, C.POINTER(C.c_ulonglong)]),
        "rt_debug_light_prepass": (ci, [C.POINTER(Vec3), C.POINTER(Light), ci, fp, fp, C.POINTER(ci)]),
        "rt_debug_occluder_lists": (ci, [C.POINTER(Sphere), ci, C.POINTER(Light), C.POINTER(ci), fp, C.POINTER(ci), ci]),
        "rt_debug_sphere_beam_slopes": (ci, [C.POINTER(Sphere), ci, C.POINTER(Light), fp, fp]),
        "rt_debug_sphere_beam_slope": (C.c_double, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double]),
        "rt_debug_beam_sine": (C.c_double, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "rt_debug_occluder_lists_device": (ci, [C.POINTER(Sphere), ci, C.POINTER(Light), C.POINTER(ci), fp, C.POINTER(ci), ci]),
        "rt_debug_occluder_lists_ex": (ci, [C.POINTER(Sphere), ci, C.POINTER(Light), C.POINTER(ci), fp, C.POINTER(ci), ci,
                                            C.POINTER(ci), C.POINTER(ci)]),
        "rt_multi_create": (vp, [ci]),
        "rt_multi_create_ex": (ci, [C.POINTER(ci), ci, ci, C.POINTER(vp)]),
        "rt_multi_destroy": (None, [vp]),
        "rt_multi_device_count": (ci, [vp]),
        "rt_multi_transport": (ci, [vp]),
        "rt_multi_scene": (vp, [vp, ci, C.POINTER(ci)]),
        "rt_multi_set_spheres": (ci, [vp, C.POINTER(Sphere), ci]),
        "rt_multi_set_planes": (ci, [vp, C.POINTER(Plane), ci]),
        "rt_multi_set_cubes": (ci, [vp, C.POINTER(Cube), ci]),
        "rt_multi_set_mesh": (ci, [vp, C.POINTER(Mesh)]),
        "rt_multi_set_texture": (ci, [vp, fp, fp, fp, ci, ci]),
        "rt_multi_set_sky": (ci, [vp, C.POINTER(Sphere), fp, fp, fp, ci, ci]),
        "rt_multi_set_lights": (ci, [vp, C.POINTER(Light), ci]),
        "rt_multi_render": (ci, [vp, C.POINTER(FrameDesc), vp]),
        "rt_multi_sync": (ci, [vp]),
        "rt_multi_stream_wait": (ci, [vp, vp]),
        "rt_multi_note": (C.c_char_p, [vp]),
        "rt_multi_gathers": (C.c_ulonglong, [vp]),
        "rt_config_object": (C.POINTER(Object), []),
        "rt_multi_frame": (vp, [vp]),
        "rt_multi_download": (ci, [vp, vp]),
        "rt_config_set_gpus": (ci, [ci]),
        "rt_assemble_rows24": (ci, [vp, vp, ci, ci, ci, ci, vp]),
        "rt_scene_set_materials": (ci, [vp, C.POINTER(Material), ci]),
        "rt_scene_set_reflect_timing": (ci, [vp, ci]),
        "rt_scene_reflect_stats": (ci, [vp, C.POINTER(ReflectStats)]),
        "rt_debug_sphere_bvh": (ci, [C.POINTER(Sphere), ci, fp, C.POINTER(ci), C.POINTER(ci), ci, C.POINTER(ci), C.POINTER(ci)]),
        "rt_debug_bvh_cast": (ci, [C.POINTER(Sphere), ci, C.POINTER(Ray), ci, ci, C.POINTER(ci), fp, C.POINTER(ci)]),
        "rt_debug_reflect": (ci, [C.POINTER(Vec3), C.POINTER(Vec3), ci, C.POINTER(Vec3)]),
        "rt_scene_set_materials_ex": (ci, [vp, C.POINTER(MaterialEx), ci]),
        "rt_debug_refract": (ci, [C.POINTER(Vec3), C.POINTER(Vec3), fp, ci, C.POINTER(Vec3)]),
        "rt_debug_transmit": (ci, [C.POINTER(Sphere), fp, C.POINTER(Ray), ci, C.POINTER(Ray), C.POINTER(ci)]),
        "rt_scene_trace_rays": (ci, [vp, C.POINTER(RayQuery), vp]),
        "rt_scene_primary_rays": (ci, [vp, C.POINTER(FrameDesc), vp, vp]),
        "rt_denoise_desc_init": (None, [C.POINTER(DenoiseDesc)]),
        "rt_scene_denoise": (ci, [vp, C.POINTER(DenoiseDesc), vp]),
        "rt_scene_set_denoise_timing": (ci, [vp, ci]),
        "rt_scene_denoise_times": (ci, [vp, fp, ci, C.POINTER(ci)]),
        "rt_vdenoise_desc_init": (None, [C.POINTER(VDenoiseDesc)]),
        "rt_scene_denoise_variance": (ci, [vp, C.POINTER(VDenoiseDesc), vp]),
        "rt_scene_set_vdenoise_timing": (ci, [vp, ci]),
        "rt_scene_vdenoise_times": (ci, [vp, fp, ci, C.POINTER(ci)]),
        "rt_debug_copy16": (ci, [vp, vp, C.c_size_t, vp]),
        "rt_temporal_desc_init": (None, [C.POINTER(TemporalDesc)]),
        "rt_scene_temporal": (ci, [vp, C.POINTER(TemporalDesc), vp]),
        "rt_view_terms": (ci, [ci, ci, cf, C.POINTER(Camera), fp]),
        "rt_tmotion_desc_init": (None, [C.POINTER(TMotionDesc)]),
        "rt_scene_temporal_motion": (ci, [vp, C.POINTER(TMotionDesc), vp]),
        "rt_scene_set_temporal_timing": (ci, [vp, ci]),
        "rt_scene_temporal_times": (ci, [vp, fp, ci, C.POINTER(ci)]),
        "rt_upsample_desc_init": (None, [C.POINTER(UpsampleDesc)]),
        "rt_scene_upsample": (ci, [vp, C.POINTER(UpsampleDesc), vp]),
        "rt_scene_set_upsample_timing": (ci, [vp, ci]),
        "rt_scene_upsample_times": (ci, [vp, fp, ci, C.POINTER(ci)]),
        "rt_scene_set_reflect_scope": (ci, [vp, ci]),
        "rt_scene_set_reflect_samples": (ci, [vp, ci]),
        "rt_scene_set_plane_materials": (ci, [vp, C.POINTER(Material), ci]),
        "rt_scene_set_cube_materials": (ci, [vp, C.POINTER(Material), ci]),
        "rt_scene_set_roughness": (ci, [vp, ci, fp, ci]),
        "rt_scene_set_emission": (ci, [vp, ci, fp, ci]),
        "rt_scene_set_gloss_seed": (ci, [vp, C.c_uint]),
        "rt_debug_gloss": (ci, [C.POINTER(Vec3), C.POINTER(Vec3), fp, C.POINTER(C.c_uint), C.POINTER(ci), ci,
                                C.POINTER(Vec3), C.POINTER(ci)]),
        "rt_debug_gloss_key": (ci, [C.POINTER(C.c_uint)] * 4 + [ci, C.POINTER(C.c_uint)]),
        "rt_debug_reflect_entry_size": (ci, []),
        "rt_scene_set_glass_model": (ci, [vp, ci]),
        "rt_debug_fresnel": (ci, [fp, fp, ci, fp]),
        "rt_debug_glass_choice": (ci, [C.POINTER(Sphere), fp, fp, C.POINTER(C.c_uint), C.POINTER(ci), C.POINTER(Ray), ci,
                                       C.POINTER(Ray), C.POINTER(ci), fp, fp, C.POINTER(ci)]),
        "rt_indirect_desc_init": (None, [C.POINTER(IndirectDesc)]),
        "rt_scene_indirect": (ci, [vp, C.POINTER(IndirectDesc), vp]),
        "rt_scene_set_indirect_timing": (ci, [vp, ci]),
        "rt_scene_indirect_times": (ci, [vp, fp, ci, C.POINTER(ci)]),
        "rt_debug_indirect_dir": (ci, [C.POINTER(Vec3), C.POINTER(C.c_uint), ci, C.POINTER(Vec3), C.POINTER(ci)]),
        "rt_debug_indirect_counts": (ci, [vp, C.POINTER(ci), ci, C.POINTER(ci)]),
        "rt_indirect_paths_opts_init": (None, [C.POINTER(IndirectPathsOpts)]),
        "rt_scene_indirect_paths": (ci, [vp, C.POINTER(IndirectDesc), C.POINTER(IndirectPathsOpts), vp]),
        "rt_debug_indirect_path_counts": (ci, [vp, C.POINTER(ci), ci, C.POINTER(ci)]),
        "rt_debug_indirect_path_key": (ci, [C.POINTER(C.c_uint), ci, ci, C.POINTER(C.c_uint)]),
        "rt_debug_reflect_dispatch": (ci, [vp, C.POINTER(ci), ci]),
        "rt_display_desc_init": (None, [C.POINTER(DisplayDesc)]),
        "rt_display_transfer_table": (ci, [fp]),
        "rt_scene_display": (ci, [vp, C.POINTER(DisplayDesc), vp]),
        "rt_scene_set_display_timing": (ci, [vp, ci]),
        "rt_scene_display_times": (ci, [vp, fp, ci, C.POINTER(ci)]),
        "rt_bloom_desc_init": (None, [C.POINTER(BloomDesc)]),
        "rt_scene_bloom": (ci, [vp, C.POINTER(BloomDesc), vp]),
        "rt_scene_set_bloom_timing": (ci, [vp, ci]),
        "rt_scene_bloom_times": (ci, [vp, fp, ci, C.POINTER(ci)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)   # AttributeError here = header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _check(rc, what):
    if rc != 0:
        raise RtError(f"{what} failed (status {rc}): {load_library().rt_last_error().decode(errors='replace')}")


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


# ----------------------------------------------------------------------------
# default scene of the reference (kernel.cu:1189-1192, 1695-1712, 261, 1701)
# ----------------------------------------------------------------------------
def view_terms(width, height, aspect, cam):
    """rt_view_terms: the origin of a view's primary rays, then cos_pitch, sin_pitch, cos_yaw, sin_yaw (7 float32)."""
    import numpy as np
    out = np.zeros(7, dtype=np.float32)
    cam = _copy_camera(cam)
    _check(load_library().rt_view_terms(width, height, aspect, C.byref(cam), _fptr(out)), "rt_view_terms")
    return out


def _copy_camera(cam) -> Camera:
    c = Camera()
    C.memmove(C.byref(c), C.byref(cam), C.sizeof(Camera))
    return c


def default_camera() -> Camera:
    return Camera(Vec3(4, 3, 10), Vec3(0, 0, 1), 0.0, 180.0, -20.0)


def default_lights():
    arr = (Light * 3)()
    arr[0] = Light(Vec3(20, 20, 20), 20, 1, 0, 0)
    arr[1] = Light(Vec3(0, 20, -20), 20, 0, 0, 1)
    arr[2] = Light(Vec3(0, 20, 0), 20, 0, 1, 0)
    return arr


def default_aspect() -> float:
    return float(load_library().rt_default_aspect())


def generate_spheres(n: int, seed: int = 1):
    arr = (Sphere * max(n, 1))()
    _check(load_library().rt_generate_spheres(arr, n, seed), "rt_generate_spheres")
    return arr


def synth_texture(kind: int):
    """(r, g, b) float32 planes [H, W] of the deterministic stand-in textures."""
    lib = load_library()
    w, h = C.c_int(), C.c_int()
    _check(lib.rt_synth_texture_size(kind, C.byref(w), C.byref(h)), "rt_synth_texture_size")
    planes = [np.empty((h.value, w.value), dtype=np.float32) for _ in range(3)]
    _check(lib.rt_synth_texture(kind, *[_fptr(p) for p in planes]), "rt_synth_texture")
    return planes


def mesh_from_obj_text(text: str):
    """rt_mesh* (reference layout) from OBJ text; raises on failure."""
    lib = load_library()
    m = lib.rt_mesh_from_obj_text(text.encode())
    if not m:
        raise RtError("rt_mesh_from_obj_text: " + lib.rt_last_error().decode(errors="replace"))
    return m


def sky_sphere(size: float = 10000.0) -> Sphere:
    s = Sphere()
    load_library().rt_sphere_init(C.byref(s), 0.0, 0.0, 0.0, size)
    return s


def band_rows(height: int, rank: int, world: int):
    """Contiguous row band [y0, y1) of `rank` out of `world`.
    Bands differ by at most one row; every row belongs to exactly one rank."""
    base, rem = divmod(height, world)
    y0 = rank * base + min(rank, rem)
    return y0, y0 + base + (1 if rank < rem else 0)


def interleaved_rows(height: int, rank: int, world: int, block: int = 16):
    """Global row indices owned by `rank` when row blocks of `block` rows are dealt
    round-robin over `world` ranks (balanced multi-GPU split), in local-row order."""
    rows = []
    k = rank
    while k * block < height:
        rows.extend(range(k * block, min((k + 1) * block, height)))
        k += world
    return rows


def _view_info_dict(info) -> dict:
    return {k: getattr(info, k) for k, _ in ViewListsInfo._fields_}


def unpack_view_lists(buf, blocks):
    """Per block of a view-list table (float32 [blocks * RT_VIEW_SLOT, 4]): (count, flags, entries float32 [count, 4],
    positions int32 [count], bounds float32 [count])."""
    out = []
    slots = np.ascontiguousarray(buf, dtype=np.float32).reshape(blocks, RT_VIEW_SLOT, 4)
    for b in range(blocks):
        count, flags = (int(v) for v in slots[b, 0].view(np.int32)[:2])
        pos = slots[b, 1 + RT_VIEW_CAP:1 + RT_VIEW_CAP + RT_VIEW_CAP // 4].reshape(-1).view(np.int32)[:count].copy()
        lbs = slots[b, 1 + RT_VIEW_CAP + RT_VIEW_CAP // 4:].reshape(-1)[:count].copy()
        out.append((count, flags, slots[b, 1:1 + count].copy(), pos, lbs))
    return out


def view_lists_host(spheres, n, fd, want_lists=True, want_beams=False) -> dict:
    """The host builder's view lists for a sphere list and a frame description (no GPU): the summary of
    Scene.view_lists_info plus 'lists' and 'beams' (float32 [blocks, 4]: unit axis, slope or -1)."""
    lib = load_library()
    info = ViewListsInfo()
    _check(lib.rt_debug_view_lists_host(spheres, n, C.byref(fd), C.byref(info), None, 0, None), "rt_debug_view_lists_host")
    buf = np.zeros((info.blocks * RT_VIEW_SLOT, 4), dtype=np.float32) if want_lists else None
    beams = np.zeros((info.blocks, 4), dtype=np.float32) if want_beams else None
    if want_lists or want_beams:
        _check(lib.rt_debug_view_lists_host(spheres, n, C.byref(fd), C.byref(info), _fptr(buf) if want_lists else None,
                                            buf.shape[0] if want_lists else 0, _fptr(beams) if want_beams else None),
               "rt_debug_view_lists_host")
    d = _view_info_dict(info)
    if want_lists:
        d["lists"] = unpack_view_lists(buf, info.blocks)
    if want_beams:
        d["beams"] = beams
    return d


def debug_tile_order(cost, tiles_x, tiles_y, via_configs=False):
    """rt_debug_tile_order as is: (status, key uint32 [nb], start uint32 [nb], perm uint32 [tiles_x * tiles_y]) as the
    device sorts the tile durations cost (uint32, row-major); the arrays hold 0xffffffff where nothing was written."""
    cost = np.ascontiguousarray(cost, dtype=np.uint32).reshape(-1)
    n = max(tiles_x, 0) * max(tiles_y, 0)
    if cost.size != n:
        raise RtError(f"debug_tile_order: {cost.size} durations for {tiles_x} x {tiles_y} tiles")
    nb = -(-max(tiles_x, 0) // 16) * -(-max(tiles_y, 0) // 16)
    key, start, perm = (np.full(k, 0xffffffff, dtype=np.uint32) for k in (nb, nb, n))
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint))
    rc = load_library().rt_debug_tile_order(up(cost), tiles_x, tiles_y, 1 if via_configs else 0, up(key), up(start), up(perm))
    return rc, key, start, perm


class Scene:
    """Device-resident scene (rt_scene). Keeps the host arrays it was built from
    so tests can hand exactly the same inputs to the oracle."""

    def __init__(self):
        self.lib = load_library()
        self.handle = self.lib.rt_scene_create()
        if not self.handle:
            raise RtError("rt_scene_create failed")
        self.spheres = None
        self.n_spheres = 0
        self.texture = None
        self.sky = None
        self.sky_box = None
        self.lights = None
        self.n_lights = 0
        self.planes, self.n_planes = None, 0
        self.cubes, self.n_cubes = None, 0
        self.materials = self.plane_materials = self.cube_materials = None
        self.emission = {}                # set_emission's host mirror: {RT_HIT_*: float32 [n, 3]} (emission_term)

    def close(self):
        if self.handle:
            self.lib.rt_scene_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_spheres(self, spheres, n):
        _check(self.lib.rt_scene_set_spheres(self.handle, spheres, n), "rt_scene_set_spheres")
        if n != self.n_spheres:           # the library cleared the materials: so does their host mirror (upsample_select)
            self.materials = None
            self.emission.pop(RT_HIT_SPHERE, None)
        self.spheres, self.n_spheres = spheres, n

    def set_planes(self, planes, n):
        _check(self.lib.rt_scene_set_planes(self.handle, planes, n), "rt_scene_set_planes")
        if n != self.n_planes:
            self.plane_materials = None
            self.emission.pop(RT_HIT_PLANE, None)
        self.planes, self.n_planes = planes, n

    def set_cubes(self, cubes, n):
        _check(self.lib.rt_scene_set_cubes(self.handle, cubes, n), "rt_scene_set_cubes")
        if n != self.n_cubes:
            self.cube_materials = None
            self.emission.pop(RT_HIT_CUBE, None)
        self.cubes, self.n_cubes = cubes, n

    def set_mesh(self, mesh):
        _check(self.lib.rt_scene_set_mesh(self.handle, mesh), "rt_scene_set_mesh")
        self.mesh = mesh

    def set_texture(self, planes):
        planes = [np.ascontiguousarray(p, dtype=np.float32) for p in planes]
        h, w = planes[0].shape
        _check(self.lib.rt_scene_set_texture(self.handle, *[_fptr(p) for p in planes], w, h), "rt_scene_set_texture")
        self.texture = planes

    def set_sky(self, box: Sphere, planes):
        planes = [np.ascontiguousarray(p, dtype=np.float32) for p in planes]
        h, w = planes[0].shape
        _check(self.lib.rt_scene_set_sky(self.handle, C.byref(box), *[_fptr(p) for p in planes], w, h), "rt_scene_set_sky")
        self.sky, self.sky_box = planes, box

    def set_lights(self, lights, n):
        _check(self.lib.rt_scene_set_lights(self.handle, lights, n), "rt_scene_set_lights")
        self.lights, self.n_lights = lights, n

    def set_materials(self, reflectivity):
        """One material per sphere: an array of floats (reflectivness k in [0, 1]) or of Material; None clears them."""
        if reflectivity is None or len(reflectivity) == 0:
            _check(self.lib.rt_scene_set_materials(self.handle, None, 0), "rt_scene_set_materials")
            self.materials = None
            return
        n = len(reflectivity)
        mats = (Material * n)()
        for i, m in enumerate(reflectivity):
            if isinstance(m, Material):
                mats[i] = m
            else:
                mats[i].reflectivness = float(m)
        _check(self.lib.rt_scene_set_materials(self.handle, mats, n), "rt_scene_set_materials")
        self.materials = mats

    def set_materials_ex(self, reflectivity=None, transparency=None, ior=None):
        """One rt_material_ex per sphere: per-sphere arrays of reflectivness k, transperancy tau and ior (a missing array
        is all 0), or a list of MaterialEx as the first argument; all None (or empty) clears the materials."""
        if reflectivity is not None and len(reflectivity) > 0 and isinstance(reflectivity[0], MaterialEx):
            n = len(reflectivity)
            mats = (MaterialEx * n)(*reflectivity)
        else:
            given = [a for a in (reflectivity, transparency, ior) if a is not None]
            if not given or all(len(a) == 0 for a in given):
                _check(self.lib.rt_scene_set_materials_ex(self.handle, None, 0), "rt_scene_set_materials_ex")
                self.materials = None
                return
            n = len(given[0])
            if any(len(a) != n for a in given):
                raise RtError("set_materials_ex: reflectivity, transparency and ior differ in length")
            mats = (MaterialEx * n)()
            for field, a in (("reflectivness", reflectivity), ("transperancy", transparency), ("ior", ior)):
                if a is not None:
                    for i, v in enumerate(a):
                        setattr(mats[i], field, float(v))
        _check(self.lib.rt_scene_set_materials_ex(self.handle, mats, n), "rt_scene_set_materials_ex")
        self.materials = mats

    def set_reflect_scope(self, scope):
        """"spheres" (default): reflective frames refuse planes, cubes and a mesh; "scene": they cast, shade and
        reflect over every kind of primitive. Also takes RT_REFLECT_SPHERES / RT_REFLECT_SCENE."""
        if isinstance(scope, str):
            if scope not in _REFLECT_SCOPES:
                raise RtError(f"unknown reflect scope {scope!r} (one of {tuple(_REFLECT_SCOPES)})")
            scope = _REFLECT_SCOPES[scope]
        _check(self.lib.rt_scene_set_reflect_scope(self.handle, int(scope)), "rt_scene_set_reflect_scope")

    def set_reflect_samples(self, mode):
        """"one" (default): reflective frames take one sample per pixel and refuse spp > 1, sample ranges and
        accumulate; "many": they take spp, sample_base, sample_total, accumulate and resolve=-1 as plain frames do
        (DESIGN.md 6h). Also takes RT_REFLECT_SAMPLES_ONE / RT_REFLECT_SAMPLES_MANY."""
        if isinstance(mode, str):
            if mode not in _REFLECT_SAMPLES:
                raise RtError(f"unknown reflect sampling mode {mode!r} (one of {tuple(_REFLECT_SAMPLES)})")
            mode = _REFLECT_SAMPLES[mode]
        _check(self.lib.rt_scene_set_reflect_samples(self.handle, int(mode)), "rt_scene_set_reflect_samples")

    def _set_kind_materials(self, entry, reflectivity):
        fn = getattr(self.lib, entry)
        if reflectivity is None or len(reflectivity) == 0:
            _check(fn(self.handle, None, 0), entry)
            return None
        n = len(reflectivity)
        mats = (Material * n)()
        for i, m in enumerate(reflectivity):
            if isinstance(m, Material):
                mats[i] = m
            else:
                mats[i].reflectivness = float(m)
        _check(fn(self.handle, mats, n), entry)
        return mats

    def set_plane_materials(self, reflectivity):
        """One material per plane (floats k in [0, 1], or Material); None clears them. Read under the "scene" scope."""
        self.plane_materials = self._set_kind_materials("rt_scene_set_plane_materials", reflectivity)

    def set_cube_materials(self, reflectivity):
        """One material per cube (floats k in [0, 1], or Material); None clears them. Read under the "scene" scope."""
        self.cube_materials = self._set_kind_materials("rt_scene_set_cube_materials", reflectivity)

    def set_roughness(self, kind, values):
        """Roughness per primitive of one kind ("sphere", "plane" or "cube"; also RT_HIT_SPHERE / _PLANE / _CUBE): one
        float in [0, 1] per primitive of that list; None (or empty) clears the kind's table. The mirror continuation of
        a hit with roughness > 0 is jittered inside a ball of that radius; the draws are a function of
        the pixel, the sample index and set_gloss_seed. The plane and cube tables are read under the "scene" scope."""
        if isinstance(kind, str):
            if kind not in _ROUGH_KINDS:
                raise RtError(f"unknown roughness kind {kind!r} (one of {tuple(_ROUGH_KINDS)})")
            kind = _ROUGH_KINDS[kind]
        if values is None or len(values) == 0:
            _check(self.lib.rt_scene_set_roughness(self.handle, int(kind), None, 0), "rt_scene_set_roughness")
            return
        v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
        _check(self.lib.rt_scene_set_roughness(self.handle, int(kind), _fptr(v), v.shape[0]), "rt_scene_set_roughness")

    def set_emission(self, kind, values):
        """Emission per primitive of one kind ("sphere", "plane" or "cube"; also RT_HIT_SPHERE / _PLANE / _CUBE): an
        [n, 3] array, one finite colour >= 0 per primitive of that list; None (or empty) clears the kind's table. A gather
        hit of indirect / indirect_paths on an emitter adds its colour to what the hit is shaded with;
        nothing else reads the tables -- emission_term is what the primary ray sees. Host state: the next indirect call
        uploads it. A list set again with another count clears its table."""
        if isinstance(kind, str):
            if kind not in _ROUGH_KINDS:
                raise RtError(f"unknown emission kind {kind!r} (one of {tuple(_ROUGH_KINDS)})")
            kind = _ROUGH_KINDS[kind]
        if values is None or len(values) == 0:
            _check(self.lib.rt_scene_set_emission(self.handle, int(kind), None, 0), "rt_scene_set_emission")
            self.emission.pop(int(kind), None)
            return
        v = np.ascontiguousarray(values, dtype=np.float32)
        if v.ndim != 2 or v.shape[1] != 3:
            raise RtError(f"set_emission: values must have shape [n, 3], not {tuple(v.shape)}")
        _check(self.lib.rt_scene_set_emission(self.handle, int(kind), _fptr(v), v.shape[0]), "rt_scene_set_emission")
        self.emission[int(kind)] = v.copy()

    def emission_term(self, frame):
        """What the primary ray itself sees of an emitter: float32 [rows, W, 4] on the device of frame["aov"]["id"], rgb
        the set_emission entry of the id guide's (kind, index), a = 0; zero for sky, triangles and kinds without a
        table. Plain indexing, no kernel. The caller adds it after the denoiser, so that an emitter glows in the picture
        -- outside the pass, where the demodulated upsample of a half-resolution pipeline would divide it by albedo."""
        import torch
        ids = (frame.get("aov") or {}).get("id")
        if ids is None:
            raise RtError(f"emission_term needs the G-buffer output 'id': render with aov={AOV_NAMES}")
        kind, index = ids[..., 0].long(), ids[..., 1].long()
        out = torch.zeros(tuple(ids.shape[:2]) + (4,), dtype=torch.float32, device=ids.device)
        for k, v in self.emission.items():
            m = kind == k
            out[..., :3][m] = torch.from_numpy(v).to(ids.device)[index[m]]
        return out

    def set_gloss_seed(self, seed: int):
        """The seed of the glossy draws (default 0; taken modulo 2^32). One sample per frame with set_gloss_seed(frame)
        into Scene.temporal(colour=...) accumulates a glossy lobe over frames."""
        _check(self.lib.rt_scene_set_gloss_seed(self.handle, int(seed) & 0xffffffff), "rt_scene_set_gloss_seed")

    def set_glass_model(self, model):
        """How a glass sphere continues a ray: "plain" (the default: always through the sphere) or "fresnel" -- a hit
        reflects with the dielectric reflectance of its angle and index and goes through otherwise, by a draw of the
        pixel, the sample index and set_gloss_seed; roughness on a glass sphere then frosts it. Also
        takes RT_GLASS_PLAIN / RT_GLASS_FRESNEL."""
        if isinstance(model, str):
            if model not in _GLASS_MODELS:
                raise RtError(f"unknown glass model {model!r} (one of {tuple(_GLASS_MODELS)})")
            model = _GLASS_MODELS[model]
        _check(self.lib.rt_scene_set_glass_model(self.handle, int(model)), "rt_scene_set_glass_model")

    def set_reflect_timing(self, on: bool):
        _check(self.lib.rt_scene_set_reflect_timing(self.handle, 1 if on else 0), "rt_scene_set_reflect_timing")

    def reflect_stats(self) -> dict:
        """What the last reflective frame did (waits for it): BVH, queue length per bounce, pass times if timed."""
        st = ReflectStats()
        _check(self.lib.rt_scene_reflect_stats(self.handle, C.byref(st)), "rt_scene_reflect_stats")
        d = st.depth
        return {"bvh_build_ms": st.bvh_build_ms, "bvh_nodes": st.bvh_nodes, "bvh_depth": st.bvh_depth,
                "bvh_leaves": st.bvh_leaves, "depth": d, "queue": list(st.queue)[:d],
                "pass_ms": list(st.pass_ms)[:d + 2] if st.timed else None}

    def set_tile_order(self, mode: int):
        """1 (default): launches start their longest tiles first (durations of earlier frames); 0: grid order."""
        _check(self.lib.rt_scene_set_tile_order(self.handle, mode), "rt_scene_set_tile_order")

    def set_view_lists(self, mode: int):
        """1 (default): the tiles of a frame walk their block's per-view candidate list; 0: every tile culls for itself."""
        _check(self.lib.rt_scene_set_view_lists(self.handle, mode), "rt_scene_set_view_lists")

    def set_light_verdicts(self, mode: int):
        """1 (default): launches of a resting view skip the lights an earlier launch of the same inputs found to add
        nothing to a tile, and the occluder search of those it found clear; 0: every launch evaluates every light."""
        _check(self.lib.rt_scene_set_light_verdicts(self.handle, mode), "rt_scene_set_light_verdicts")

    def _read_back(self, fn: str, info_cls, wanted, make) -> dict:
        """An 'info, then buffers' read-back: `fn` with null buffers fills the info struct, whose fields are the dict;
        where wanted(info), make(info) gives the buffer arguments of a second call and a callable for the entries
        they become."""
        call = getattr(self.lib, fn)
        info = info_cls()
        _check(call(self.handle, C.byref(info), *[None] * (len(call.argtypes) - 3), 0), fn)
        d = {k: getattr(info, k) for k, _ in info_cls._fields_}
        if wanted(info):
            args, entries = make(info)
            _check(call(self.handle, C.byref(info), *args), fn)
            d.update(entries())
        return d

    def light_verdicts(self, want_words: bool = False) -> dict:
        """What the last frame launch did with light verdicts (waits for the table's writer): state 0 nothing / 1 wrote
        / 2 read, slot, tiles_x, tiles_y, unwritten, nothing, clear; with want_words also 'words', uint64 [tiles_y,
        tiles_x]: two bits per (group, light) at 16 * group + 2 * light."""
        def make(i):
            buf = np.zeros(i.tiles_x * i.tiles_y, dtype=np.uint64)
            return (buf.ctypes.data_as(C.POINTER(C.c_uint64)), buf.size), lambda: {"words": buf.reshape(i.tiles_y, i.tiles_x)}
        return self._read_back("rt_debug_light_verdicts", LightVerdictsInfo, lambda i: want_words and i.state, make)

    def shadow_counts(self, want_tables: bool = False) -> dict:
        """The shadow counts behind the last launch's light verdicts (waits for the table's writer): state, slot, tiles_x,
        tiles_y, records (per tile), tagged, tiles_tagged, tagged_all (over all of the scene's tables); with want_tables also 'tags', uint8 [tiles_y, tiles_x, 4]
        (byte r: 0x80 | group << 3 | light of record r, 0 = free) and 'counts', uint8 [tiles_y, tiles_x, records, 64]."""
        def make(i):
            n = i.tiles_x * i.tiles_y
            tags = np.zeros(n, dtype=np.uint32)
            counts = np.zeros((n, i.records, 64), dtype=np.uint8)
            return ((tags.ctypes.data_as(C.POINTER(C.c_uint32)), counts.ctypes.data_as(C.POINTER(C.c_uint8)), n),
                    lambda: {"tags": tags.view(np.uint8).reshape(i.tiles_y, i.tiles_x, 4),
                             "counts": counts.reshape(i.tiles_y, i.tiles_x, i.records, 64)})
        return self._read_back("rt_debug_shadow_counts", ShadowCountsInfo, lambda i: want_tables and i.state, make)

    def set_shadow_counts(self, tags=None, counts=None):
        """Tests: overwrites the record tags (uint8 [tiles_y, tiles_x, 4]) and / or the records (uint8 [tiles_y, tiles_x,
        records, 64]) of the table that the last launch wrote or read."""
        n = 0
        tp = cp = None
        if tags is not None:
            tags = np.ascontiguousarray(tags, dtype=np.uint8)
            n = tags.size // 4
            tp = tags.ctypes.data_as(C.POINTER(C.c_uint32))
        if counts is not None:
            counts = np.ascontiguousarray(counts, dtype=np.uint8)
            n = counts.shape[0] * counts.shape[1]
            cp = counts.ctypes.data_as(C.POINTER(C.c_uint8))
        _check(self.lib.rt_debug_set_shadow_counts(self.handle, tp, cp, n), "rt_debug_set_shadow_counts")

    def primary_records(self, want_tables: bool = False) -> dict:
        """The primary records behind the last launch's light verdicts (waits for the table's writer): state, slot, tiles_x,
        tiles_y, tile_w, tiles_recorded, hit_pixels, miss_pixels; with want_tables also 'dwords', uint32 [tiles_y, tiles_x,
        64] (see decode_primary_records; lane = row in tile * tile_w + column in tile) and 'positions', int32 of the same
        shape: the sphere-table position a pixel's entry resolves to, -1 a miss, -2 no record or outside the frame."""
        def make(i):
            n = 64 * i.tiles_x * i.tiles_y
            dwords = np.zeros(n, dtype=np.uint32)
            pos = np.zeros(n, dtype=np.int32)
            return ((dwords.ctypes.data_as(C.POINTER(C.c_uint32)), pos.ctypes.data_as(C.POINTER(C.c_int32)), n),
                    lambda: {"dwords": dwords.reshape(i.tiles_y, i.tiles_x, 64), "positions": pos.reshape(i.tiles_y, i.tiles_x, 64)})
        return self._read_back("rt_debug_primary_records", PrimaryRecordsInfo, lambda i: want_tables and i.state, make)

    def set_primary_records(self, dwords):
        """Tests: overwrites the primary records (uint32 [tiles_y, tiles_x, 64]) of the table that the last launch wrote or
        read."""
        dwords = np.ascontiguousarray(dwords, dtype=np.uint32)
        _check(self.lib.rt_debug_set_primary_records(self.handle, dwords.ctypes.data_as(C.POINTER(C.c_uint32)), dwords.size),
               "rt_debug_set_primary_records")

    def tile_summaries(self, want_tables: bool = False) -> dict:
        """The tile summaries behind the last launch's light verdicts (waits for the table's writer): state, slot, tiles_x,
        tiles_y, settled, settled_no_miss; with want_tables also 'dwords', uint32 [tiles_y, tiles_x]: RT_TILE_SETTLED,
        RT_TILE_NO_MISS and the tile's group count (saturating) at RT_TILE_GROUPS_SHIFT."""
        def make(i):
            dwords = np.zeros(i.tiles_x * i.tiles_y, dtype=np.uint32)
            return (dwords.ctypes.data_as(C.POINTER(C.c_uint32)), dwords.size), lambda: {"dwords": dwords.reshape(i.tiles_y, i.tiles_x)}
        return self._read_back("rt_debug_tile_summaries", TileSummariesInfo, lambda i: want_tables and i.state, make)

    def set_tile_summaries(self, dwords):
        """Tests: overwrites the tile summaries (uint32 [tiles_y, tiles_x]) of the table that the last launch wrote or
        read."""
        dwords = np.ascontiguousarray(dwords, dtype=np.uint32)
        _check(self.lib.rt_debug_set_tile_summaries(self.handle, dwords.ctypes.data_as(C.POINTER(C.c_uint32)), dwords.size),
               "rt_debug_set_tile_summaries")

    def set_compact_launch(self, on: int):
        """1 (default): a resting view's reading launches start one workgroup per tile that still computes and one per run
        of settled tiles, once the table's run list is built and its counts have arrived; 0: one per tile. Same frames."""
        _check(self.lib.rt_scene_set_compact_launch(self.handle, on), "rt_scene_set_compact_launch")

    def set_compact_run(self, run: int = 64, ahead: int = 1, min_percent: int = 0):
        """Profiles and tests: settled tiles per workgroup of the compact launches whose run lists are built from now on,
        whether those workgroups lie behind (0) or ahead of (1) the tiles that keep their wave, and the share of streamed
        tiles (percent) below which a launch keeps the full grid -- the library's default is 25, this call's is 0."""
        _check(self.lib.rt_debug_set_compact_run(self.handle, run, ahead, min_percent), "rt_debug_set_compact_run")

    def compact_order(self, tiles: int):
        """Tests: the order the last launch's run list was built from, uint32 [tiles]: (tile_y << 16) | tile_x."""
        order = np.zeros(tiles, dtype=np.uint32)
        _check(self.lib.rt_debug_compact_order(self.handle, order.ctypes.data_as(C.POINTER(C.c_uint32)), order.size), "rt_debug_compact_order")
        return order

    def compact_launch(self, want_list: bool = False) -> dict:
        """The last frame launch's geometry (compact, n_unsettled, n_streamed, run, workgroups), the run lists built so far
        (rebuilds) and, where the table that launch wrote or read has a run list (list_built; waits for its build), the
        list's header (tiles_x, tiles_y, list_n_unsettled, list_n_streamed) and with want_list its entries 'list',
        uint32 [tiles]: (tile_y << 16) | tile_x."""
        info = CompactLaunchInfo()
        _check(self.lib.rt_debug_compact_launch(self.handle, C.byref(info), None, 0), "rt_debug_compact_launch")
        out = {name: getattr(info, name) for name, _ in CompactLaunchInfo._fields_}
        if want_list and info.list_built:
            lst = np.zeros(info.tiles_x * info.tiles_y, dtype=np.uint32)
            _check(self.lib.rt_debug_compact_launch(self.handle, C.byref(info), lst.ctypes.data_as(C.POINTER(C.c_uint32)), lst.size),
                   "rt_debug_compact_launch")
            out["list"] = lst
        return out

    def view_lists_info(self, want_lists: bool = False) -> dict:
        """What the last launch read (waits for the lists' build): read, block size, blocks, overflowed and not-built
        blocks, longest and mean list; with want_lists also 'lists' (see unpack_view_lists)."""
        def make(i):
            buf = np.zeros((i.blocks * RT_VIEW_SLOT, 4), dtype=np.float32)
            return (_fptr(buf), buf.shape[0]), lambda: {"lists": unpack_view_lists(buf, i.blocks)}
        return self._read_back("rt_scene_view_lists_info", ViewListsInfo, lambda i: want_lists and i.read, make)

    @classmethod
    def default(cls, n_spheres: int = 1024, seed: int = 1) -> "Scene":
        s = cls()
        s.set_spheres(generate_spheres(n_spheres, seed), n_spheres)
        s.set_texture(synth_texture(0))
        s.set_sky(sky_sphere(), synth_texture(1))
        s.set_lights(default_lights(), 3)
        return s

    def frame_desc(self, width, height, *, pixels=0, rgba=0, cam=None, aspect=None, y0=0, y1=0, spp=1,
                   sample_base=0, sample_total=0, accumulate=False, resolve=0, cull=True, tile=0,
                   stats=0, force_slow=False, profile=False, interleave=None, packed24=0, table_lds=False, fast=False,
                   reflect_depth=0, aov_depth=0, aov_normal=0, aov_id=0, aov_albedo=0) -> FrameDesc:
        fd = FrameDesc()
        fd.struct_size = C.sizeof(FrameDesc)
        fd.width, fd.height = width, height
        fd.aspect = default_aspect() if aspect is None else aspect
        fd.cam = cam if cam is not None else default_camera()
        fd.pixels = pixels
        o = fd.opts
        o.struct_size = C.sizeof(LaunchOpts)
        o.rgba = rgba
        o.y0, o.y1 = y0, y1
        o.spp, o.sample_base, o.sample_total = spp, sample_base, sample_total
        o.accumulate = 1 if accumulate else 0
        o.resolve = resolve
        o.cull = 1 if cull else 0
        o.tile = tile
        o.stats = stats
        o.force_slow_path = 1 if force_slow else 0
        o.profile = 1 if profile else 0
        if interleave is not None:          # (count, index, block_rows)
            o.interleave_count, o.interleave_index, o.interleave_rows = interleave
        o.packed24 = packed24
        o.table_lds = 1 if table_lds else 0
        o.fast = 1 if fast else 0
        o.reflect_depth = reflect_depth
        fd.aov_depth, fd.aov_normal, fd.aov_id, fd.aov_albedo = aov_depth, aov_normal, aov_id, aov_albedo
        return fd

    def render_raw(self, fd: FrameDesc, stream=0):
        _check(self.lib.rt_scene_render(self.handle, C.byref(fd), stream), "rt_scene_render")

    def render(self, width, height, *, y0=0, y1=0, want_rgba=True, want_stats=False, want_packed24=False, stream=None,
               aov=(), **kw):
        """Render rows [y0,y1) into fresh torch CUDA tensors and return
        {'packed': int32 [rows, W], 'rgba': float32 [rows, W, 4], 'stats': dict}. `aov`: names out of AOV_NAMES
        ("depth", "normal", "id", "albedo"); out['aov'] then maps each to its G-buffer of the frame's primary rays:
        depth float32 [rows, W], normal float32 [rows, W, 4], id int32 [rows, W, 2] (kind, index), albedo float32
        [rows, W, 4] (rt_frame_desc.aov_*)."""
        aov = (aov,) if isinstance(aov, str) else tuple(aov or ())
        for name in aov:
            if name not in _AOV_LAYOUT:
                raise RtError(f"unknown G-buffer output {name!r} (one of {AOV_NAMES})")
        import torch
        if not torch.cuda.is_available():
            raise RtError("no GPU visible: the ray-tracing path has no CPU fallback")
        rows = (y1 if y1 else height) - y0
        if kw.get("interleave") is not None:
            cnt, idx, blk = kw["interleave"]
            rows = len(interleaved_rows(rows, idx, cnt, blk or 16))   # blocks are dealt from the band's first row
        packed = torch.empty((rows, width), dtype=torch.int32, device="cuda")
        rgba = torch.empty((rows, width, 4), dtype=torch.float32, device="cuda") if want_rgba else None
        stats = torch.zeros(RT_STATS_COUNT, dtype=torch.int64, device="cuda") if want_stats else None
        st = torch.cuda.current_stream() if stream is None else stream
        p24 = torch.zeros((rows, width * 3 // 4), dtype=torch.int32, device="cuda") if want_packed24 else None
        aovs = {}
        for name in aov:
            dt, comps = _AOV_LAYOUT[name]
            shape = (rows, width) if comps == 1 else (rows, width, comps)
            aovs[name] = torch.empty(shape, dtype=getattr(torch, dt), device="cuda")
        fd = self.frame_desc(width, height, pixels=packed.data_ptr(), rgba=rgba.data_ptr() if want_rgba else 0,
                             y0=y0, y1=y1, stats=stats.data_ptr() if want_stats else 0,
                             packed24=p24.data_ptr() if want_packed24 else 0,
                             **{f"aov_{k}": v.data_ptr() for k, v in aovs.items()}, **kw)
        self.render_raw(fd, st.cuda_stream)
        out = {"packed": packed, "rgba": rgba}
        if aov:
            out["aov"] = aovs
        if want_packed24:
            out["packed24"] = p24     # [rows, 3*width/4] int32: bytes B,G,R per pixel (rt_launch_opts.packed24)
        if want_stats:
            out["stats"] = dict(zip(STAT_NAMES, stats.cpu().tolist()))
        return out

    # ---------------------------------------------------------------- ray queries
    def query(self, mode, n, *, rays=0, hits=0, occluded=0, rgba=0, packed=0, cull=-1) -> RayQuery:
        q = RayQuery()
        q.struct_size = C.sizeof(RayQuery)
        q.mode = _QUERY_MODES.get(mode, mode) if isinstance(mode, str) else mode
        q.n, q.cull = n, cull
        q.rays, q.hits, q.occluded, q.rgba, q.packed = rays, hits, occluded, rgba, packed
        return q

    def trace_rays_raw(self, q: RayQuery, stream=0) -> int:
        """rt_scene_trace_rays as is: returns the status."""
        return self.lib.rt_scene_trace_rays(self.handle, C.byref(q), stream)

    def trace_rays(self, rays, mode="nearest", cull=True, stream=None):
        """Cast a CUDA float32 tensor of rays, shape (n, 6) = Org, Dir (directions used as given). Returns a dict of
        tensors: nearest -> t, kind, index, uv, txy, normal, new_org (castRay's hit record; kind -1 / t = inf on a
        miss); occluded -> occluded (int32 0/1, castLightRay's any-hit); shade -> rgba (n, 4), packed (n,) int32 (the
        colour rayTrace gives the ray: the frame's pixel for its own primary ray)."""
        import torch
        if not torch.cuda.is_available():
            raise RtError("no GPU visible: the ray queries have no CPU fallback")
        if not (rays.is_cuda and rays.dtype == torch.float32 and rays.dim() == 2 and rays.shape[1] == 6):
            raise RtError("rays must be a CUDA float32 tensor of shape (n, 6)")
        rays = rays.contiguous()
        n = rays.shape[0]
        m = _QUERY_MODES[mode]
        st = torch.cuda.current_stream() if stream is None else stream
        out = {}
        kw = {}
        if m == RT_QUERY_NEAREST:
            hits = torch.empty((n, 16), dtype=torch.int32, device=rays.device)
            kw["hits"] = hits.data_ptr()
        elif m == RT_QUERY_OCCLUDED:
            occ = torch.empty(n, dtype=torch.int32, device=rays.device)
            kw["occluded"] = occ.data_ptr()
        else:
            rgba = torch.empty((n, 4), dtype=torch.float32, device=rays.device)
            packed = torch.empty(n, dtype=torch.int32, device=rays.device)
            kw["rgba"], kw["packed"] = rgba.data_ptr(), packed.data_ptr()
        q = self.query(m, n, rays=rays.data_ptr(), cull=1 if cull else 0, **kw)
        _check(self.trace_rays_raw(q, st.cuda_stream), "rt_scene_trace_rays")
        if m == RT_QUERY_NEAREST:
            f = hits.view(torch.float32)
            out = {"t": f[:, 0], "kind": hits[:, 1], "index": hits[:, 2], "uv": f[:, 3:5], "txy": f[:, 5:7],
                   "normal": f[:, 7:10], "new_org": f[:, 10:13]}
        elif m == RT_QUERY_OCCLUDED:
            out = {"occluded": occ}
        else:
            out = {"rgba": rgba, "packed": packed}
        return out

    def primary_rays(self, width, height, *, y0=0, y1=0, cam=None, aspect=None, stream=None):
        """The reference's primary rays of rows [y0, y1) as the frame kernel forms them: (rows, width, 6) CUDA float32."""
        import torch
        if not torch.cuda.is_available():
            raise RtError("no GPU visible: the ray queries have no CPU fallback")
        rows = (y1 if y1 else height) - y0
        rays = torch.empty((rows, width, 6), dtype=torch.float32, device="cuda")
        fd = self.frame_desc(width, height, cam=cam, aspect=aspect, y0=y0, y1=y1)
        st = torch.cuda.current_stream() if stream is None else stream
        _check(self.lib.rt_scene_primary_rays(self.handle, C.byref(fd), rays.data_ptr(), st.cuda_stream),
               "rt_scene_primary_rays")
        return rays

    def pick(self, width, height, x, y, **kw):
        """What is under pixel (x, y) of a width x height frame: (kind, index), kind RT_HIT_* (-1: sky)."""
        hit = self.trace_rays(self.primary_rays(width, height, y0=y, y1=y + 1, **kw)[0, x:x + 1], "nearest")
        return int(hit["kind"][0]), int(hit["index"][0])

    # ---------------------------------------------------------------- what the post passes below share
    def _desc(self, cls, init, plain, optional=None, flags=None):
        """A `cls` after self.lib.<init>: `plain` assigned as it is, `optional` where not None, `flags` (where not
        None) as 0 / 1."""
        d = cls()
        getattr(self.lib, init)(C.byref(d))
        for k, v in plain.items():
            setattr(d, k, v)
        for k, v in (optional or {}).items():
            if v is not None:
                setattr(d, k, v)
        for k, v in (flags or {}).items():
            if v is not None:
                setattr(d, k, 1 if v else 0)
        return d

    @staticmethod
    def _need_gpu(what):
        """torch, or RtError where no GPU is visible."""
        import torch
        if not torch.cuda.is_available():
            raise RtError(f"no GPU visible: {what} has no CPU fallback")
        return torch

    @staticmethod
    def _guides(frame, colour, need, message):
        """The frame's G-buffer outputs, or RtError(message) without a colour or one of the guides `need`."""
        aov = frame.get("aov") or {}
        if colour is None or any(k not in aov for k in need):
            raise RtError(message)
        return aov

    @staticmethod
    def _cuda_colour(torch, name, rgba, rows, width):
        if tuple(rgba.shape) != (rows, width, 4) or rgba.dtype != torch.float32 or not rgba.is_cuda:
            raise RtError(f"{name}: the colour must be a CUDA float32 tensor of the guides' shape [rows, W, 4]")
        return rgba.contiguous()

    @staticmethod
    def _stream(torch, stream):
        return torch.cuda.current_stream() if stream is None else stream

    @staticmethod
    def _new(torch, want, like, shape, dtype):
        """A new tensor on `like`'s device, or None."""
        return torch.empty(shape, dtype=dtype, device=like.device) if want else None

    @staticmethod
    def _ptr(t):
        return t.data_ptr() if t is not None else 0

    @classmethod
    def _prev(cls, history):
        """temporal_desc's prev_* of a history."""
        if history is None:
            return {}
        return dict(prev_cam=history["cam"], prev_aspect=history["aspect"], prev_rgba=history["rgba"].data_ptr(),
                    prev_depth=history["depth"].data_ptr(), prev_normal=history["normal"].data_ptr(),
                    prev_id=history["id"].data_ptr(), prev_moments=cls._ptr(history.get("moments")))

    def _set_pass_timing(self, name, on):
        fn = f"rt_scene_set_{name}_timing"
        _check(getattr(self.lib, fn)(self.handle, 1 if on else 0), fn)

    def _pass_times(self, name, cap):
        fn = f"rt_scene_{name}_times"
        ms = (C.c_float * cap)()
        n = C.c_int()
        _check(getattr(self.lib, fn)(self.handle, ms, cap, C.byref(n)), fn)
        return list(ms)[: n.value]

    # ---------------------------------------------------------------- the denoiser
    def denoise_desc(self, width, height, *, rgba_in=0, depth=0, normal=0, albedo=0, id=0, rgba_out=0, pixels=0,
                     iterations=None, normal_shift=None, sigma_depth=None, sigma_colour=None, demodulate=None,
                     variant=0) -> DenoiseDesc:
        """rt_denoise_desc with rt_denoise_desc_init's defaults where an argument is None."""
        return self._desc(DenoiseDesc, "rt_denoise_desc_init",
                          dict(width=width, height=height, rgba_in=rgba_in, depth=depth, normal=normal, albedo=albedo,
                               id=id, rgba_out=rgba_out, pixels=pixels),
                          dict(iterations=iterations, normal_shift=normal_shift, sigma_depth=sigma_depth,
                               sigma_colour=sigma_colour, variant=variant),
                          dict(demodulate=demodulate))

    def denoise_raw(self, d: DenoiseDesc, stream=0) -> int:
        """rt_scene_denoise as is: returns the status."""
        return self.lib.rt_scene_denoise(self.handle, C.byref(d), stream)

    def _denoise(self, variance, frame, history, want_packed, want_variance, stream, **knobs):
        """denoise (variance False: no history, rows and width from the colour as it is) and denoise_variance."""
        torch = self._need_gpu("the denoiser")
        rgba = frame.get("rgba") if history is None else history.get("rgba")
        moments = None if history is None else history.get("moments")
        demodulate = knobs["demodulate"]
        need = ("depth", "normal", "id") + (() if demodulate is not None and not demodulate else ("albedo",))
        colour = "a colour (the frame's rgba or the history's)" if variance else "the frame's rgba"
        aov = self._guides(frame, rgba, need, f"{'denoise_variance' if variance else 'denoise'} needs {colour} and the "
                           f"G-buffer outputs {need}: render with want_rgba=True and aov={AOV_NAMES}")
        if variance:
            if history is not None and moments is None:
                raise RtError("denoise_variance: the history carries no moments (Scene.temporal(..., want_moments=True))")
            rows, width = aov["depth"].shape[0], aov["depth"].shape[1]
            if tuple(rgba.shape) != (rows, width, 4):
                raise RtError("denoise_variance: the colour is not of the guides' shape [rows, W, 4]")
        else:
            rows, width = rgba.shape[0], rgba.shape[1]
        out = torch.empty_like(rgba)
        packed = self._new(torch, want_packed, rgba, (rows, width), torch.int32)
        var = self._new(torch, want_variance, rgba, (rows, width), torch.float32)
        st = self._stream(torch, stream)
        args = dict(rgba_in=rgba.data_ptr(), depth=aov["depth"].data_ptr(), normal=aov["normal"].data_ptr(),
                    albedo=self._ptr(aov.get("albedo")), id=aov["id"].data_ptr(), rgba_out=out.data_ptr(),
                    pixels=self._ptr(packed), **knobs)
        if variance:
            d = self.vdenoise_desc(width, rows, moments=self._ptr(moments), variance_out=self._ptr(var), **args)
            _check(self.denoise_variance_raw(d, st.cuda_stream), "rt_scene_denoise_variance")
            return {"rgba": out, "packed": packed, "variance": var}
        _check(self.denoise_raw(self.denoise_desc(width, rows, **args), st.cuda_stream), "rt_scene_denoise")
        return {"rgba": out, "packed": packed}

    def denoise(self, frame, *, iterations=None, normal_shift=None, sigma_depth=None, sigma_colour=None,
                demodulate=None, want_packed=True, variant=0, stream=None):
        """Filter a frame that render(..., aov=("depth", "normal", "id", "albedo")) returned with the edge-avoiding
        a-trous filter of rt_scene_denoise (None: the default of rt_denoise_desc_init; demodulate=False needs no
        albedo). Returns {'rgba': float32 [rows, W, 4], 'packed': int32 [rows, W] or None} as new tensors; the frame's
        own tensors are not written. Enqueued on `stream` (default: the current stream); no host wait."""
        return self._denoise(False, frame, None, want_packed, False, stream, iterations=iterations,
                             normal_shift=normal_shift, sigma_depth=sigma_depth, sigma_colour=sigma_colour,
                             demodulate=demodulate, variant=variant)

    # ---------------------------------------------------------------- the variance-guided denoiser
    def vdenoise_desc(self, width, height, *, rgba_in=0, depth=0, normal=0, albedo=0, id=0, rgba_out=0, pixels=0,
                      moments=0, variance_out=0, iterations=None, normal_shift=None, sigma_depth=None, sigma_colour=None,
                      sigma_floor=None, min_history=None, spatial_boost=None, demodulate=None, variant=0) -> VDenoiseDesc:
        """rt_vdenoise_desc with rt_vdenoise_desc_init's defaults where an argument is None."""
        return self._desc(VDenoiseDesc, "rt_vdenoise_desc_init",
                          dict(width=width, height=height, rgba_in=rgba_in, depth=depth, normal=normal, albedo=albedo,
                               id=id, rgba_out=rgba_out, pixels=pixels, moments=moments, variance_out=variance_out),
                          dict(iterations=iterations, normal_shift=normal_shift, sigma_depth=sigma_depth,
                               sigma_colour=sigma_colour, sigma_floor=sigma_floor, min_history=min_history,
                               spatial_boost=spatial_boost, variant=variant),
                          dict(demodulate=demodulate))

    def denoise_variance_raw(self, d: VDenoiseDesc, stream=0) -> int:
        """rt_scene_denoise_variance as is: returns the status."""
        return self.lib.rt_scene_denoise_variance(self.handle, C.byref(d), stream)

    def denoise_variance(self, frame, history=None, *, iterations=None, normal_shift=None, sigma_depth=None,
                         sigma_colour=None, sigma_floor=None, min_history=None, spatial_boost=None, demodulate=None,
                         want_packed=True, want_variance=True, variant=0, stream=None):
        """Filter with the variance-guided a-trous filter of rt_scene_denoise_variance. The guides and the albedo are
        those of `frame` (render(..., aov=("depth", "normal", "id", "albedo"))). With `history` (what Scene.temporal
        returned for that frame) the colour, its history length and the luminance moments come from it; without, the
        colour is the frame's own and every pixel's variance is the spatial estimate. None: the default of
        rt_vdenoise_desc_init. Returns {'rgba': float32 [rows, W, 4], 'packed': int32 [rows, W] or None, 'variance':
        float32 [rows, W] or None} as new tensors; neither the frame's nor the history's tensors are written.
        Enqueued on `stream` (default: the current stream); no host wait."""
        return self._denoise(True, frame, history, want_packed, want_variance, stream, iterations=iterations,
                             normal_shift=normal_shift, sigma_depth=sigma_depth, sigma_colour=sigma_colour,
                             sigma_floor=sigma_floor, min_history=min_history, spatial_boost=spatial_boost,
                             demodulate=demodulate, variant=variant)

    def set_vdenoise_timing(self, on: bool):
        self._set_pass_timing("vdenoise", on)

    def vdenoise_times(self):
        """Device ms of every launch of the last timed variance-guided call (waits for it): variants 0 and 2: the pack
        pass, the spatial-estimate pass, then the iterations; variant 1: the initial variance, then the iterations."""
        return self._pass_times("vdenoise", RT_DENOISE_MAX_ITERATIONS + 2)

    # ---------------------------------------------------------------- temporal accumulation
    def temporal_desc(self, width, height, *, cam=None, aspect=None, prev_cam=None, prev_aspect=None, rgba_in=0, depth=0,
                      normal=0, id=0, prev_rgba=0, prev_depth=0, prev_normal=0, prev_id=0, prev_moments=0, rgba_out=0,
                      moments_out=0, pixels=0, reset=False, max_history=None, depth_tolerance=None, normal_cos_min=None,
                      variant=0) -> TemporalDesc:
        """rt_temporal_desc with rt_temporal_desc_init's defaults where an argument is None (cam / aspect: the
        default view; prev_cam / prev_aspect: the current ones)."""
        aspect = default_aspect() if aspect is None else aspect
        cam = _copy_camera(cam if cam is not None else default_camera())
        return self._desc(TemporalDesc, "rt_temporal_desc_init",
                          dict(width=width, height=height, aspect=aspect, cam=cam,
                               prev_aspect=aspect if prev_aspect is None else prev_aspect,
                               prev_cam=_copy_camera(prev_cam if prev_cam is not None else cam),
                               rgba_in=rgba_in, depth=depth, normal=normal, id=id, prev_rgba=prev_rgba,
                               prev_depth=prev_depth, prev_normal=prev_normal, prev_id=prev_id, prev_moments=prev_moments,
                               rgba_out=rgba_out, moments_out=moments_out, pixels=pixels),
                          dict(max_history=max_history, depth_tolerance=depth_tolerance, normal_cos_min=normal_cos_min,
                               variant=variant),
                          dict(reset=bool(reset)))

    def temporal_raw(self, d: TemporalDesc, stream=0) -> int:
        """rt_scene_temporal as is: returns the status."""
        return self.lib.rt_scene_temporal(self.handle, C.byref(d), stream)

    def _temporal(self, motion, frame, history, cam, aspect, colour, want_moments, want_packed, stream, **knobs):
        """temporal (motion None) and temporal_motion (motion: (sphere_motion, cube_motion, the clamp's arguments))."""
        import contextlib
        torch = self._need_gpu("temporal accumulation")
        name = "temporal" if motion is None else "temporal_motion"
        rgba = frame.get("rgba") if colour is None else colour
        need = ("depth", "normal", "id")
        aov = self._guides(frame, rgba, need, f"{name} needs the frame's rgba (or colour=) and the G-buffer outputs "
                           f"{need}: render with want_rgba=True and aov={need}")
        rows, width = aov["depth"].shape[0], aov["depth"].shape[1]
        rgba = self._cuda_colour(torch, name, rgba, rows, width)
        now = {} if motion is None else dict(zip(("spheres", "cubes"), self._object_origins()))
        if history is not None:
            if tuple(history["rgba"].shape) != (rows, width, 4):
                raise RtError(f"{name}: the history is of another size (pass history=None after a resize)")
            if want_moments and history.get("moments") is None:
                raise RtError(f"{name}: want_moments needs a history with moments")
            for k in now:
                if history.get(k) is not None and history[k].shape != now[k].shape:
                    raise RtError(f"temporal_motion: the scene has {now[k].shape[0]} {k}, the history {history[k].shape[0]} "
                                  "(pass history=None after adding or removing objects)")
        cam = _copy_camera(cam if cam is not None else default_camera())
        aspect = default_aspect() if aspect is None else aspect
        st = self._stream(torch, stream)
        # temporal_motion allocates (and uploads its tables) on `stream`, temporal on the current stream
        with torch.cuda.stream(st) if motion is not None else contextlib.nullcontext():
            out = torch.empty_like(rgba)
            moments = self._new(torch, want_moments, rgba, (rows, width, 2), torch.float32)
            packed = self._new(torch, want_packed, rgba, (rows, width), torch.int32)
            tables = {} if motion is None else self._motion_tables(torch, history, now, rgba.device, *motion[:2])
        args = dict(cam=cam, aspect=aspect, rgba_in=rgba.data_ptr(), depth=aov["depth"].data_ptr(),
                    normal=aov["normal"].data_ptr(), id=aov["id"].data_ptr(), rgba_out=out.data_ptr(),
                    moments_out=self._ptr(moments), pixels=self._ptr(packed), reset=history is None,
                    **knobs, **self._prev(history))
        if motion is None:
            _check(self.temporal_raw(self.temporal_desc(width, rows, **args), st.cuda_stream), "rt_scene_temporal")
        else:
            for k, m in tables.items():
                args[k], args["n_" + k] = m.data_ptr(), m.shape[0]
            d = self.temporal_motion_desc(width, rows, **args, **motion[2])
            _check(self.temporal_motion_raw(d, st.cuda_stream), "rt_scene_temporal_motion")
        return {"rgba": out, "moments": moments, "packed": packed, "depth": aov["depth"], "normal": aov["normal"],
                "id": aov["id"], "cam": cam, "aspect": aspect, **now}

    def temporal(self, frame, history=None, *, cam=None, aspect=None, colour=None, max_history=None,
                 depth_tolerance=None, normal_cos_min=None, want_moments=True, want_packed=True, variant=0, stream=None):
        """Blend a frame that render(..., aov=("depth", "normal", "id")) returned with camera `cam` and `aspect` into
        `history`, what the previous call returned (None: no history is read -- the first frame, or after objects or
        lights moved, which temporal_motion below follows instead). `colour`: an rgba tensor to accumulate instead of the frame's own, from another render of the
        same view (a jittered sample_base = k, sample_total = m frame, which cannot carry guides). Returns the new
        history {'rgba': float32 [rows, W, 4] (accumulated colour, history length), 'moments': float32 [rows, W, 2]
        or None, 'packed': int32 [rows, W] or None, 'depth', 'normal', 'id': the frame's guide tensors (not copied),
        'cam', 'aspect'} as new tensors; neither the frame's nor the history's tensors are written. Enqueued on
        `stream` (default: the current stream); no host wait."""
        return self._temporal(None, frame, history, cam, aspect, colour, want_moments, want_packed, stream,
                              max_history=max_history, depth_tolerance=depth_tolerance, normal_cos_min=normal_cos_min,
                              variant=variant)

    # ------------------------------------------- temporal accumulation over moving objects
    def temporal_motion_desc(self, width, height, *, sphere_motion=0, n_sphere_motion=0, cube_motion=0, n_cube_motion=0,
                             clamp=None, clamp_slack=None, clamp_history=None, **kw) -> TMotionDesc:
        """rt_tmotion_desc: temporal_desc's arguments, then the motion arrays (device addresses) and the clamp, with
        rt_tmotion_desc_init's defaults where an argument is None."""
        t = self.temporal_desc(width, height, **kw)
        return self._desc(TMotionDesc, "rt_tmotion_desc_init",
                          dict({k: getattr(t, k) for k, _ in TemporalDesc._fields_[1:]}, sphere_motion=sphere_motion,
                               n_sphere_motion=n_sphere_motion, cube_motion=cube_motion, n_cube_motion=n_cube_motion),
                          dict(clamp_slack=clamp_slack, clamp_history=clamp_history), dict(clamp=clamp))

    def temporal_motion_raw(self, d: TMotionDesc, stream=0) -> int:
        """rt_scene_temporal_motion as is: returns the status."""
        return self.lib.rt_scene_temporal_motion(self.handle, C.byref(d), stream)

    def _object_origins(self):
        """Host copies, float32 [n, 3]: the sphere centres and each cube's bounds[0] as the scene holds them now."""
        sp = np.zeros((self.n_spheres or 0, 3), dtype=np.float32)
        for i in range(sp.shape[0]):
            o = self.spheres[i].orgin
            sp[i] = (o.x, o.y, o.z)
        cu = np.zeros((getattr(self, "n_cubes", 0) or 0, 3), dtype=np.float32)
        for i in range(cu.shape[0]):
            o = self.cubes[i].bounds[0]
            cu[i] = (o.x, o.y, o.z)
        return sp, cu

    @staticmethod
    def _motion_tables(torch, history, now, device, sphere_motion, cube_motion):
        """{'sphere_motion', 'cube_motion': CUDA float32 [n, 4]}: per kind the displacements given, else those inferred
        from the positions the history carries; no entry without a history, where nothing moved or for an empty table."""
        tables = {}
        for k, arg, m in (("spheres", "sphere_motion", sphere_motion), ("cubes", "cube_motion", cube_motion)):
            if m is None and history is not None and history.get(k) is not None:
                m = (now[k] - history[k]).astype(np.float32)
                if not m.any():
                    m = None                                   # nothing moved: no table
            if m is None or history is None:
                continue
            if not torch.is_tensor(m):
                m = np.asarray(m, dtype=np.float32)
                if m.ndim != 2 or m.shape[1] not in (3, 4):
                    raise RtError("temporal_motion: a displacement array is [n, 3] or [n, 4]")
                m4 = np.zeros((m.shape[0], 4), dtype=np.float32)
                m4[:, :m.shape[1]] = m
                m = torch.from_numpy(m4).to(device)
            if m.dtype != torch.float32 or not m.is_cuda or m.ndim != 2 or m.shape[1] != 4 or not m.is_contiguous():
                raise RtError("temporal_motion: a displacement tensor must be a contiguous CUDA float32 [n, 4]")
            if m.shape[0]:
                tables[arg] = m
        return tables

    def temporal_motion(self, frame, history=None, *, cam=None, aspect=None, colour=None, sphere_motion=None,
                        cube_motion=None, clamp=None, clamp_slack=None, clamp_history=None, max_history=None,
                        depth_tolerance=None, normal_cos_min=None, want_moments=True, want_packed=True, variant=0,
                        stream=None):
        """Scene.temporal for a scene whose spheres and cubes were moved (set_spheres / set_cubes) and whose lights may
        have moved since `history` was made. The returned history is temporal's dict plus 'spheres' and 'cubes': host
        copies, float32 [n, 3], of the sphere centres and of each cube's bounds[0] at the time of this call. With
        sphere_motion / cube_motion None the displacements are now - history[...] in binary32 (a history from
        Scene.temporal carries no positions: nothing moved); an object count that differs from the history's raises
        RtError: start over with history=None. An explicit displacement array -- numpy [n, 3] or [n, 4], or a CUDA
        float32 tensor [n, 4] -- overrides the inferred one. clamp / clamp_slack / clamp_history: rt_tmotion_desc's
        (None: its defaults). Enqueued on `stream` (default: the current stream); inferred or numpy displacements
        are uploaded first, which is the only host wait."""
        motion = (sphere_motion, cube_motion, dict(clamp=clamp, clamp_slack=clamp_slack, clamp_history=clamp_history))
        return self._temporal(motion, frame, history, cam, aspect, colour, want_moments, want_packed, stream,
                              max_history=max_history, depth_tolerance=depth_tolerance, normal_cos_min=normal_cos_min,
                              variant=variant)

    # ---------------------------------------------------------------- guided upsampling
    def upsample_desc(self, width, height, lo_width, lo_height, *, rgba_lo=0, depth_lo=0, normal_lo=0, albedo_lo=0,
                      id_lo=0, depth=0, normal=0, albedo=0, id=0, base=0, rgba_out=0, pixels=0, source=0,
                      sphere_select=0, n_sphere_select=0, plane_select=0, n_plane_select=0, cube_select=0,
                      n_cube_select=0, use_tables=False, normal_shift=None, sigma_depth=None, demodulate=None,
                      variant=0) -> UpsampleDesc:
        """rt_upsample_desc with rt_upsample_desc_init's defaults where an argument is None."""
        return self._desc(UpsampleDesc, "rt_upsample_desc_init",
                          dict(width=width, height=height, lo_width=lo_width, lo_height=lo_height, rgba_lo=rgba_lo,
                               depth_lo=depth_lo, normal_lo=normal_lo, albedo_lo=albedo_lo, id_lo=id_lo, depth=depth,
                               normal=normal, albedo=albedo, id=id, base=base, rgba_out=rgba_out, pixels=pixels,
                               source=source, sphere_select=sphere_select, n_sphere_select=n_sphere_select,
                               plane_select=plane_select, n_plane_select=n_plane_select, cube_select=cube_select,
                               n_cube_select=n_cube_select),
                          dict(normal_shift=normal_shift, sigma_depth=sigma_depth, variant=variant),
                          dict(use_tables=bool(use_tables), demodulate=demodulate))

    def upsample_raw(self, d: UpsampleDesc, stream=0) -> int:
        """rt_scene_upsample as is: returns the status."""
        return self.lib.rt_scene_upsample(self.handle, C.byref(d), stream)

    def upsample(self, hi, lo, *, colour=None, base=True, select=None, normal_shift=None, sigma_depth=None,
                 demodulate=None, want_packed=True, want_source=True, variant=0, stream=None):
        """Bring a low-resolution colour to the resolution of `hi`. `hi` and `lo` are frames of one view as
        render(..., aov=("depth", "normal", "id", "albedo")) returned them (demodulate=False needs no albedo).
        `colour`: an rgba tensor of lo's size to upsample instead of lo["rgba"]. `base`: True passes hi["rgba"] (what
        a pixel that is not upsampled takes), False or None none (the plain bilinear mean), or a tensor of hi's size.
        `select`: None = every hit pixel is upsampled; or a dict with any of "sphere", "plane", "cube", each a sequence
        (or uint8 CUDA tensor) with a non-zero entry per object whose pixels are. Returns {'rgba': float32
        [H, W, 4], 'packed': int32 [H, W] or None, 'source': uint8 [H, W] or None} as new tensors; no input is
        written. Enqueued on `stream` (default: the current stream); no host wait."""
        torch = self._need_gpu("the upsampler")
        ha, la = hi.get("aov") or {}, lo.get("aov") or {}
        rgba_lo = lo.get("rgba") if colour is None else colour
        demod = demodulate is None or bool(demodulate)
        need = ("depth", "normal", "id") + (("albedo",) if demod else ())
        if rgba_lo is None or any(k not in ha or k not in la for k in need):
            raise RtError(f"upsample needs lo's rgba (or colour=) and the G-buffer outputs {need} of both frames: render "
                          f"with want_rgba=True and aov={AOV_NAMES}")
        H, W = ha["depth"].shape[0], ha["depth"].shape[1]
        h, w = la["depth"].shape[0], la["depth"].shape[1]
        if tuple(rgba_lo.shape) != (h, w, 4) or rgba_lo.dtype != torch.float32 or not rgba_lo.is_cuda:
            raise RtError("upsample: the colour must be a CUDA float32 tensor of lo's guides' shape [h, w, 4]")
        rgba_lo = rgba_lo.contiguous()
        if base is True:
            base = hi.get("rgba")
            if base is None:
                raise RtError("upsample: base=True needs hi's rgba")
        elif base is False:
            base = None
        if base is not None:
            if tuple(base.shape) != (H, W, 4) or base.dtype != torch.float32 or not base.is_cuda:
                raise RtError("upsample: base must be a CUDA float32 tensor of hi's shape [H, W, 4]")
            base = base.contiguous()
        dev = rgba_lo.device
        tables, keep = {}, []
        if select is not None:
            for kind in ("sphere", "plane", "cube"):
                t = select.get(kind)
                if t is None or len(t) == 0:
                    continue
                if not isinstance(t, torch.Tensor):
                    t = torch.tensor([1 if v else 0 for v in t], dtype=torch.uint8)
                t = t.to(device=dev, dtype=torch.uint8).contiguous()
                keep.append(t)
                tables[f"{kind}_select"], tables[f"n_{kind}_select"] = t.data_ptr(), t.numel()
        out = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
        packed = self._new(torch, want_packed, rgba_lo, (H, W), torch.int32)
        source = self._new(torch, want_source, rgba_lo, (H, W), torch.uint8)
        st = self._stream(torch, stream)
        d = self.upsample_desc(W, H, w, h, rgba_lo=rgba_lo.data_ptr(), depth_lo=la["depth"].data_ptr(),
                               normal_lo=la["normal"].data_ptr(), albedo_lo=la["albedo"].data_ptr() if demod else 0,
                               id_lo=la["id"].data_ptr(), depth=ha["depth"].data_ptr(), normal=ha["normal"].data_ptr(),
                               albedo=ha["albedo"].data_ptr() if demod else 0, id=ha["id"].data_ptr(),
                               base=self._ptr(base), rgba_out=out.data_ptr(), pixels=self._ptr(packed),
                               source=self._ptr(source), use_tables=select is not None,
                               normal_shift=normal_shift, sigma_depth=sigma_depth, demodulate=demod, variant=variant,
                               **tables)
        _check(self.upsample_raw(d, st.cuda_stream), "rt_scene_upsample")
        for t in keep:                    # the tables stay allocated until the stream has run the pass
            t.record_stream(st)
        return {"rgba": out, "packed": packed, "source": source}

    def upsample_select(self):
        """The tables render_upscaled passes: per kind, 1 where the object's material has k > 0 or tau > 0."""
        def table(mats):
            return [1 if (m.reflectivness > 0 or m.transperancy > 0) else 0 for m in mats] if mats is not None else []
        return {"sphere": table(self.materials), "plane": table(self.plane_materials), "cube": table(self.cube_materials)}

    def render_upscaled(self, width, height, factor=2, reflect_depth=1, *, variant=0, want_parts=False, **kw):
        """A reflective frame traced at reduced resolution: the plain frame (reflect_depth = 0) with guides at
        width x height, the reflective frame with guides at width // factor x height // factor with the same camera
        and aspect, and rt_scene_upsample without demodulation, the plain frame as base and tables built from the
        materials -- every pixel that shows neither mirror nor glass is the full-resolution frame's, bit for bit.
        `kw` goes to both renders (cam, aspect, cull, ...). Returns upsample's dict; with want_parts also 'hi' and
        'lo', the two frames."""
        if factor < 1 or width // factor < 1 or height // factor < 1:
            raise RtError("render_upscaled: factor must be >= 1 and leave a low-resolution frame of at least 1 x 1")
        guides = ("depth", "normal", "id")
        hi = self.render(width, height, aov=guides, **kw)
        lo = self.render(width // factor, height // factor, aov=guides, reflect_depth=reflect_depth, **kw)
        out = self.upsample(hi, lo, base=True, select=self.upsample_select(), demodulate=False, variant=variant,
                            stream=kw.get("stream"))
        if want_parts:
            out["hi"], out["lo"] = hi, lo
        return out

    def set_upsample_timing(self, on: bool):
        self._set_pass_timing("upsample", on)

    def upsample_times(self):
        """Device ms of the last timed upsample call (waits for it): a list of at most one."""
        return self._pass_times("upsample", 1)

    def set_temporal_timing(self, on: bool):
        self._set_pass_timing("temporal", on)

    def temporal_times(self):
        """Device ms of the last timed temporal call's launch (waits for it): a list of at most one value."""
        return self._pass_times("temporal", 1)

    def set_denoise_timing(self, on: bool):
        self._set_pass_timing("denoise", on)

    def denoise_times(self):
        """Device ms of every launch of the last timed denoise call (waits for it): variants 0 and 2: the pack pass, then
        the iterations; variant 1: the iterations."""
        return self._pass_times("denoise", RT_DENOISE_MAX_ITERATIONS + 1)

    # ---------------------------------------------------------------- the bloom pass
    def bloom_desc(self, width, height, *, rgba_in=0, state=0, rgba_out=0, pixels=0, glow_out=0, levels=None,
                   threshold=None, limit=None, spread=None, strength=None, variant=0) -> BloomDesc:
        """rt_bloom_desc with rt_bloom_desc_init's defaults where an argument is None."""
        return self._desc(BloomDesc, "rt_bloom_desc_init",
                          dict(width=width, height=height, rgba_in=rgba_in, state=state, rgba_out=rgba_out, pixels=pixels,
                               glow_out=glow_out),
                          dict(levels=levels, threshold=threshold, limit=limit, spread=spread, strength=strength,
                               variant=variant))

    def bloom_raw(self, d: BloomDesc, stream=0) -> int:
        """rt_scene_bloom as is: returns the status."""
        return self.lib.rt_scene_bloom(self.handle, C.byref(d), stream)

    def bloom(self, frame, state=None, *, levels=None, threshold=None, limit=None, spread=None, strength=None,
              want_rgba=True, want_packed=True, want_glow=False, variant=0, stream=None):
        """Spread the light above a luminance threshold over its neighbourhood, on the linear colour ahead of `display`
        (rt_scene_bloom; None: the default of rt_bloom_desc_init). `frame`: a frame dict (its "rgba") or a bare CUDA
        float32 [H, W, 4] tensor. `state`: None, or the "state" a display call returned: threshold and limit are then
        on the scale that call exposes at; it is read on the device and not written. Returns {'rgba': float32 [H, W, 4]
        or None, 'pixels': int32 [H, W] or None, 'glow': float32 [H, W, 4] or None (the glare alone, before
        `strength`)} as new tensors; the frame is not written. Enqueued on `stream` (default: the current stream); no
        host wait."""
        for name, value in (("levels", levels), ("variant", variant)):
            if value is not None and (isinstance(value, bool) or not isinstance(value, int)):
                raise RtError(f"bloom: {name} must be an int, not {value!r}")
        for name, value in (("threshold", threshold), ("limit", limit), ("spread", spread), ("strength", strength)):
            if value is not None and (isinstance(value, bool) or not isinstance(value, (int, float))):
                raise RtError(f"bloom: {name} must be a number, not {value!r}")
        if not (want_rgba or want_packed or want_glow):
            raise RtError("bloom: want_rgba, want_packed and want_glow are all false: nothing to do")
        torch = self._need_gpu("the bloom pass")
        rgba = frame.get("rgba") if isinstance(frame, dict) else frame
        if (not isinstance(rgba, torch.Tensor) or rgba.dim() != 3 or rgba.shape[2] != 4 or rgba.dtype != torch.float32
                or not rgba.is_cuda):
            raise RtError("bloom: the colour must be a CUDA float32 tensor of shape [H, W, 4] (or a frame with such an rgba)")
        rgba = rgba.contiguous()
        H, W = rgba.shape[0], rgba.shape[1]
        if state is not None and (not isinstance(state, torch.Tensor) or tuple(state.shape) != (4,)
                                  or state.dtype != torch.float32 or state.device != rgba.device
                                  or not state.is_contiguous()):
            raise RtError("bloom: state must be a contiguous float32 tensor of shape [4] beside the colour")
        st = self._stream(torch, stream)
        out = self._new(torch, want_rgba, rgba, (H, W, 4), torch.float32)
        packed = self._new(torch, want_packed, rgba, (H, W), torch.int32)
        glow = self._new(torch, want_glow, rgba, (H, W, 4), torch.float32)
        d = self.bloom_desc(W, H, rgba_in=rgba.data_ptr(), state=self._ptr(state), rgba_out=self._ptr(out),
                            pixels=self._ptr(packed), glow_out=self._ptr(glow), levels=levels, threshold=threshold,
                            limit=limit, spread=spread, strength=strength, variant=variant)
        _check(self.bloom_raw(d, st.cuda_stream), "rt_scene_bloom")
        rgba.record_stream(st)            # a contiguous copy stays allocated until the stream has run the pass
        return {"rgba": out, "pixels": packed, "glow": glow}

    def set_bloom_timing(self, on: bool):
        self._set_pass_timing("bloom", on)

    def bloom_times(self):
        """Device ms of every launch of the last timed bloom call (waits for it), 2 * levels of them: the downsamples
        from the frame on, the upsamples from the coarsest level on, the combine."""
        return self._pass_times("bloom", RT_BLOOM_MAX_EVENTS)

    # ---------------------------------------------------------------- one-bounce global illumination
    def indirect_desc(self, width, height, *, cam=None, aspect=None, depth=0, normal=0, id=0, albedo=0, rgba_in=0,
                      rgba_out=0, pixels=0, rays=None, ray_base=None, seed=None, strength=None, cull=None,
                      variant=0) -> IndirectDesc:
        """rt_indirect_desc with rt_indirect_desc_init's defaults where an argument is None (cam / aspect: the default
        view)."""
        return self._desc(IndirectDesc, "rt_indirect_desc_init",
                          dict(width=width, height=height, aspect=default_aspect() if aspect is None else aspect,
                               cam=_copy_camera(cam if cam is not None else default_camera()), depth=depth, normal=normal,
                               id=id, albedo=albedo, rgba_in=rgba_in, rgba_out=rgba_out, pixels=pixels),
                          dict(rays=rays, ray_base=ray_base, seed=seed, strength=strength, cull=cull, variant=variant))

    def indirect_raw(self, d: IndirectDesc, stream=0) -> int:
        """rt_scene_indirect as is: returns the status."""
        return self.lib.rt_scene_indirect(self.handle, C.byref(d), stream)

    def indirect(self, frame, *, cam=None, aspect=None, colour="frame", rays=None, ray_base=None, seed=None,
                 strength=None, modulate=True, cull=True, variant=0, want_packed=False, stream=None):
        """Add one-bounce indirect diffuse light to a frame that render(..., aov=("depth", "normal", "id", "albedo"))
        returned with camera `cam` and `aspect`: per surface pixel `rays` hashed cosine-distributed gather rays (ray
        indices ray_base .. ray_base + rays - 1 under `seed`), each shaded as trace_rays(..., "shade") shades it, their
        mean times `strength` and -- with `modulate` -- the pixel's albedo. `colour`: "frame" adds the term to
        frame["rgba"], None returns the term alone, or a CUDA float32 tensor of the guides' shape to add it to.
        modulate=False needs no albedo. None: the default of rt_indirect_desc_init. Returns {'rgba': float32
        [rows, W, 4], and with want_packed 'packed': int32 [rows, W]} as new tensors; no input is written. Enqueued on
        `stream` (default: the current stream)."""
        return self._indirect("indirect", lambda d, st: _check(self.indirect_raw(d, st), "rt_scene_indirect"), frame, cam,
                              aspect, colour, rays, ray_base, seed, strength, modulate, cull, variant, want_packed, stream)

    def _indirect(self, name, call, frame, cam, aspect, colour, rays, ray_base, seed, strength, modulate, cull, variant,
                  want_packed, stream):
        """The body of indirect and indirect_paths: `name` is the method's, call(d, stream) runs its entry."""
        torch = self._need_gpu("the indirect pass")
        need = ("depth", "normal", "id") + (("albedo",) if modulate else ())
        aov = frame.get("aov") or {}
        if any(k not in aov for k in need):
            raise RtError(f"{name} needs the G-buffer outputs {need}: render with aov={AOV_NAMES}")
        rows, width = aov["depth"].shape[0], aov["depth"].shape[1]
        if isinstance(colour, str):
            if colour != "frame":
                raise RtError(f'{name}: colour is "frame", None or a tensor')
            colour = frame.get("rgba")
            if colour is None:
                raise RtError(f'{name}: colour="frame" needs the frame\'s rgba (render with want_rgba=True)')
        if colour is not None:
            colour = self._cuda_colour(torch, name, colour, rows, width)
        like = aov["depth"]
        out = torch.empty((rows, width, 4), dtype=torch.float32, device=like.device)
        packed = self._new(torch, want_packed, like, (rows, width), torch.int32)
        st = self._stream(torch, stream)
        d = self.indirect_desc(width, rows, cam=cam, aspect=aspect, depth=aov["depth"].data_ptr(),
                               normal=aov["normal"].data_ptr(), id=aov["id"].data_ptr(),
                               albedo=aov["albedo"].data_ptr() if modulate else 0, rgba_in=self._ptr(colour),
                               rgba_out=out.data_ptr(), pixels=self._ptr(packed), rays=rays, ray_base=ray_base, seed=seed,
                               strength=strength, cull=1 if cull else 0, variant=variant)
        call(d, st.cuda_stream)
        res = {"rgba": out}
        if want_packed:
            res["packed"] = packed
        return res

    def set_indirect_timing(self, on: bool):
        self._set_pass_timing("indirect", on)

    def indirect_times(self):
        """Device ms of every launch of the last timed indirect call (waits for it): variant 1: the kernel; variant 0:
        per group of at most 4 rays the cast, shade and resolve passes."""
        return self._pass_times("indirect", 3 * ((RT_INDIRECT_MAX_RAYS + 3) // 4))

    def indirect_counts(self):
        """The queue lengths of the last variant-0 indirect call (waits for it), one per group of rays: the gather rays
        that hit something."""
        return self._indirect_counts("rt_debug_indirect_counts", 4)

    def _indirect_counts(self, fn, cap):
        cnt = (C.c_int * cap)()
        n = C.c_int()
        _check(getattr(self.lib, fn)(self.handle, cnt, cap, C.byref(n)), fn)
        return list(cnt)[: n.value]

    # ---------------------------------------------------------------- multi-bounce global illumination
    def indirect_paths_opts(self, bounces=None) -> IndirectPathsOpts:
        """rt_indirect_paths_opts with rt_indirect_paths_opts_init's default where `bounces` is None."""
        return self._desc(IndirectPathsOpts, "rt_indirect_paths_opts_init", {}, dict(bounces=bounces))

    def indirect_paths_raw(self, d: IndirectDesc, o: IndirectPathsOpts = None, stream=0) -> int:
        """rt_scene_indirect_paths as is (o None: NULL, the defaults): returns the status."""
        self._paths_bounces = o.bounces if o is not None else self.indirect_paths_opts().bounces   # for indirect_path_counts
        return self.lib.rt_scene_indirect_paths(self.handle, C.byref(d), C.byref(o) if o is not None else None, stream)

    def indirect_paths(self, frame, *, bounces=None, cam=None, aspect=None, colour="frame", rays=None, ray_base=None,
                       seed=None, strength=None, modulate=True, cull=True, variant=0, want_packed=False, stream=None):
        """Scene.indirect whose gather rays are diffuse paths of at most `bounces` shaded surface hits (1 ..
        RT_INDIRECT_MAX_BOUNCES; None: the default of rt_indirect_paths_opts_init, 2): a hit lit directly spawns the
        next cosine-distributed ray with the hit's texel as its weight. Every other keyword as indirect's, the same
        dict returned; bounces=1 is indirect itself, launch for launch."""
        def call(d, st):
            _check(self.indirect_paths_raw(d, self.indirect_paths_opts(bounces), st), "rt_scene_indirect_paths")
        return self._indirect("indirect_paths", call, frame, cam, aspect, colour, rays, ray_base, seed, strength, modulate,
                              cull, variant, want_packed, stream)

    def indirect_path_counts(self):
        """The queue lengths of the last variant-0 indirect_paths call with bounces > 1 (waits for it): per group of
        rays a list with, per bounce, the paths that entered its shade pass. [] after any other indirect call."""
        cnt = self._indirect_counts("rt_debug_indirect_path_counts", ((RT_INDIRECT_MAX_RAYS + 3) // 4) * RT_INDIRECT_MAX_BOUNCES)
        b = getattr(self, "_paths_bounces", 0)    # the C entry reports counts[group * bounces + b]
        if not cnt or b < 1 or len(cnt) % b:
            return []
        return [cnt[g:g + b] for g in range(0, len(cnt), b)]

    def indirect_paths_times(self):
        """Device ms of every launch of the last timed indirect or indirect_paths call (set_indirect_timing; waits for
        it): variant 1: the kernel; variant 0: per group of at most 4 rays the cast pass, the shade pass (bounces = 1)
        or one shade-and-continue pass per bounce, and the resolve pass."""
        return self._pass_times("indirect", (2 + RT_INDIRECT_MAX_BOUNCES) * ((RT_INDIRECT_MAX_RAYS + 3) // 4))

    # ---------------------------------------------------------------- the display transform
    def display_desc(self, width, height, *, rgba_in=0, id=0, rgba_out=0, pixels=0, state=0, histogram_out=0, meter=None,
                     exposure=None, key=None, min_exposure=None, max_exposure=None, meter_low=None, meter_high=None,
                     adapt=None, meter_sky=None, curve=None, white=None, transfer=None, variant=0) -> DisplayDesc:
        """rt_display_desc with rt_display_desc_init's defaults where an argument is None."""
        return self._desc(DisplayDesc, "rt_display_desc_init",
                          dict(width=width, height=height, rgba_in=rgba_in, id=id, rgba_out=rgba_out, pixels=pixels,
                               state=state, histogram_out=histogram_out),
                          dict(meter=meter, exposure=exposure, key=key, min_exposure=min_exposure,
                               max_exposure=max_exposure, meter_low=meter_low, meter_high=meter_high, adapt=adapt,
                               curve=curve, white=white, transfer=transfer, variant=variant),
                          dict(meter_sky=meter_sky))

    def display_raw(self, d: DisplayDesc, stream=0) -> int:
        """rt_scene_display as is: returns the status."""
        return self.lib.rt_scene_display(self.handle, C.byref(d), stream)

    def display(self, frame, state=None, *, meter="auto", exposure=None, key=None, window=None, limits=None, adapt=None,
                meter_sky=None, curve="aces", white=None, transfer="srgb", want_rgba=True, want_packed=True,
                want_histogram=False, variant=0, stream=None):
        """Show a float colour: meter it, expose it, run it through a tone curve and pack it (rt_scene_display; None:
        the default of rt_display_desc_init). `frame`: a frame dict (its "rgba", and its id guide where it has one: sky
        pixels are then not metered unless meter_sky) or a bare CUDA float32 [H, W, 4] tensor. `state`: the "state" an
        earlier call returned, or None for a zeroed one; it is updated in place. meter: "auto" (this frame's own
        exposure), "lagged" (the state's exposure, the frame read once; its histogram resolves the next one) or
        "manual" (`exposure`; no state). window: (meter_low, meter_high) in 1/1024ths; limits: (min_exposure,
        max_exposure). Returns {'rgba': float32 [H, W, 4] or None, 'pixels': int32 [H, W] or None, 'state': float32
        [4] or None, 'histogram': int32 [RT_DISPLAY_BINS] or None} as new tensors but the state; the frame is not
        written. Enqueued on `stream` (default: the current stream); no host wait."""
        for name, value, table in (("meter", meter, _DISPLAY_METERS), ("curve", curve, _DISPLAY_CURVES),
                                   ("transfer", transfer, _DISPLAY_TRANSFERS)):
            if value not in table:
                raise RtError(f"display: {name} must be one of {sorted(table)}, not {value!r}")
        for name, pair in (("window", window), ("limits", limits)):
            if pair is not None and len(pair) != 2:
                raise RtError(f"display: {name} must be a pair")
        torch = self._need_gpu("the display transform")
        rgba, ids = frame, None
        if isinstance(frame, dict):
            rgba, ids = frame.get("rgba"), (frame.get("aov") or {}).get("id")
        if (not isinstance(rgba, torch.Tensor) or rgba.dim() != 3 or rgba.shape[2] != 4 or rgba.dtype != torch.float32
                or not rgba.is_cuda):
            raise RtError("display: the colour must be a CUDA float32 tensor of shape [H, W, 4] (or a frame with such an rgba)")
        rgba = rgba.contiguous()
        H, W = rgba.shape[0], rgba.shape[1]
        metering = meter != "manual"
        if ids is not None and metering:
            if tuple(ids.shape) != (H, W, 2) or ids.dtype != torch.int32 or ids.device != rgba.device:
                raise RtError("display: the id guide must be an int32 tensor of shape [H, W, 2] beside the colour")
            ids = ids.contiguous()
        st = self._stream(torch, stream)
        if metering:
            if state is None:
                with torch.cuda.stream(st):           # cleared on the stream the pass runs on
                    state = torch.zeros(4, dtype=torch.float32, device=rgba.device)
            elif (not isinstance(state, torch.Tensor) or tuple(state.shape) != (4,) or state.dtype != torch.float32
                  or state.device != rgba.device or not state.is_contiguous()):
                raise RtError("display: state must be a contiguous float32 tensor of shape [4] beside the colour")
        else:
            state = None
        out = self._new(torch, want_rgba, rgba, (H, W, 4), torch.float32)
        packed = self._new(torch, want_packed, rgba, (H, W), torch.int32)
        hist = None
        if want_histogram and metering:               # a call that meters nothing writes none: zeros then
            with torch.cuda.stream(st):
                hist = torch.zeros(RT_DISPLAY_BINS, dtype=torch.int32, device=rgba.device)
        low, high = window if window is not None else (None, None)
        lo_e, hi_e = limits if limits is not None else (None, None)
        d = self.display_desc(W, H, rgba_in=rgba.data_ptr(), id=self._ptr(ids) if metering else 0, rgba_out=self._ptr(out),
                              pixels=self._ptr(packed), state=self._ptr(state), histogram_out=self._ptr(hist),
                              meter=_DISPLAY_METERS[meter], exposure=exposure, key=key, min_exposure=lo_e,
                              max_exposure=hi_e, meter_low=low, meter_high=high, adapt=adapt, meter_sky=meter_sky,
                              curve=_DISPLAY_CURVES[curve], white=white, transfer=_DISPLAY_TRANSFERS[transfer],
                              variant=variant)
        _check(self.display_raw(d, st.cuda_stream), "rt_scene_display")
        rgba.record_stream(st)            # a contiguous copy stays allocated until the stream has run the pass
        return {"rgba": out, "pixels": packed, "state": state, "histogram": hist}

    def set_display_timing(self, on: bool):
        self._set_pass_timing("display", on)

    def display_times(self):
        """Device ms of every launch of the last timed display call (waits for it): "auto": metering, resolve, apply;
        "lagged": the fused pass, resolve; "manual": the apply pass."""
        return self._pass_times("display", 3)
