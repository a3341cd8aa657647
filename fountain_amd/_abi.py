"""ctypes mirror of include/fountain_hip.h (the C ABI of the MI355X path-tracing core).

Only layout lives here: every struct below must match the header field for field
(tests/test_abi.py checks sizes and that the shared library exports each declared symbol).
"""
import ctypes as C
from collections import namedtuple

c_f = C.c_float
c_u32 = C.c_uint32
c_i32 = C.c_int32
c_u64 = C.c_uint64

FTN_OK = 0
FTN_ERR_INVALID_ARGUMENT = -1
FTN_ERR_NO_DEVICE = -2
FTN_ERR_OUT_OF_MEMORY = -3
FTN_ERR_NAN_RADIANCE = -4
FTN_ERR_UNSUPPORTED = -5
FTN_ERR_BVH_TOO_DEEP = -6
FTN_ERR_INTERNAL = -7

FTN_SHAPE_TRIANGLE, FTN_SHAPE_SPHERE = 0, 1
FTN_MAT_MATTE, FTN_MAT_METAL, FTN_MAT_MIRROR, FTN_MAT_PLASTIC, FTN_MAT_GLASS = range(5)
FTN_LIGHT_POINT, FTN_LIGHT_DISTANT, FTN_LIGHT_INFINITE = range(3)
FTN_SAMPLER_TILE_SERIAL, FTN_SAMPLER_INDEXED = 0, 1
FTN_INTEGRATOR_PATH, FTN_INTEGRATOR_DIRECT_LIGHTING, FTN_INTEGRATOR_WHITTED = 0, 1, 2
FTN_PIPELINE_AUTO, FTN_PIPELINE_MEGAKERNEL, FTN_PIPELINE_WAVEFRONT = 0, 1, 2


class ftn_transform(C.Structure):
    _fields_ = [("m", c_f * 16), ("inv", c_f * 16)]


class ftn_pixel(C.Structure):
    _fields_ = [("xyz", c_f * 3), ("filter_weight_sum", c_f)]


class ftn_bvh_node(C.Structure):
    _fields_ = [("bmin", c_f * 3), ("bmax", c_f * 3), ("idx", c_u32), ("n_prims", C.c_uint16),
                ("axis", C.c_uint8), ("is_leaf", C.c_uint8)]


class ftn_prim(C.Structure):
    _fields_ = [("shape_kind", c_u32), ("shape_index", c_u32), ("material", c_i32), ("area_emit", c_i32)]


class ftn_mesh(C.Structure):
    _fields_ = [("has_normals", c_u32), ("has_uvs", c_u32), ("flip_normals", c_u32), ("reverse_orientation", c_u32), ("has_tangents", c_u32)]


class ftn_sphere(C.Structure):
    _fields_ = [("object_to_world", ftn_transform), ("world_to_object", ftn_transform),
                ("radius", c_f), ("z_min", c_f), ("z_max", c_f), ("theta_min", c_f), ("theta_max", c_f),
                ("phi_max", c_f), ("reverse_orientation", c_u32), ("_pad", c_u32)]


class ftn_material(C.Structure):
    _fields_ = [("type", c_u32), ("remap_roughness", c_u32), ("a", c_f * 3), ("b", c_f * 3),
                ("s0", c_f), ("s1", c_f), ("s2", c_f), ("_pad", c_f)]


class ftn_light(C.Structure):
    _fields_ = [("type", c_u32), ("envmap", c_i32), ("rgb", c_f * 3), ("v", c_f * 3),
                ("light_to_world", ftn_transform)]


class ftn_envmap(C.Structure):
    _fields_ = [("width", c_u32), ("height", c_u32), ("texels", C.POINTER(c_f))]


FTN_TEX_CONSTANT, FTN_TEX_UV, FTN_TEX_CHECKERBOARD, FTN_TEX_IMAGE = range(4)
FTN_WRAP_REPEAT, FTN_WRAP_BLACK, FTN_WRAP_CLAMP = range(3)


class ftn_texture(C.Structure):
    _fields_ = [("kind", c_u32), ("is_float", c_u32), ("value", c_f * 3), ("tex1", c_i32), ("tex2", c_i32), ("image", c_i32),
                ("su", c_f), ("sv", c_f), ("du", c_f), ("dv", c_f)]


class ftn_image(C.Structure):
    _fields_ = [("width", c_u32), ("height", c_u32), ("wrap", c_u32), ("_pad", c_u32), ("texels", C.POINTER(c_f))]


class ftn_material_textures(C.Structure):
    _fields_ = [("a", c_i32), ("b", c_i32), ("s0", c_i32), ("s1", c_i32), ("s2", c_i32), ("_pad", c_i32 * 3)]


class ftn_scene_desc(C.Structure):
    _fields_ = [
        ("n_prims", c_u32), ("prims", C.POINTER(ftn_prim)),
        ("n_triangles", c_u32), ("tri_indices", C.POINTER(c_u32)), ("tri_mesh", C.POINTER(c_u32)),
        ("n_vertices", c_u32), ("P", C.POINTER(c_f)), ("N", C.POINTER(c_f)), ("UV", C.POINTER(c_f)),
        ("n_meshes", c_u32), ("meshes", C.POINTER(ftn_mesh)),
        ("n_spheres", c_u32), ("spheres", C.POINTER(ftn_sphere)),
        ("n_materials", c_u32), ("materials", C.POINTER(ftn_material)),
        ("n_area_emit", c_u32), ("area_emit", C.POINTER(c_f)),
        ("n_lights", c_u32), ("lights", C.POINTER(ftn_light)),
        ("n_envmaps", c_u32), ("envmaps", C.POINTER(ftn_envmap)),
        ("n_textures", c_u32), ("textures", C.POINTER(ftn_texture)), ("material_textures", C.POINTER(ftn_material_textures)),
        ("n_images", c_u32), ("images", C.POINTER(ftn_image)),
        ("S", C.POINTER(c_f)),
    ]


class ftn_camera_desc(C.Structure):
    _fields_ = [("camera_to_world", ftn_transform), ("raster_to_camera", ftn_transform),
                ("shutter_open", c_f), ("shutter_close", c_f), ("lens_radius", c_f), ("focal_dist", c_f),
                ("dx_camera", c_f * 3), ("dy_camera", c_f * 3)]


class ftn_film_desc(C.Structure):
    _fields_ = [("full_resolution", c_i32 * 2), ("crop", c_i32 * 4), ("filter_radius", c_f * 2)]


class ftn_sampler_desc(C.Structure):
    _fields_ = [("kind", c_u32), ("samples_per_pixel", c_u32), ("seed", c_u64),
                ("first_sample", c_u32), ("sample_count", c_u32)]


class ftn_integrator_desc(C.Structure):
    _fields_ = [("kind", c_u32), ("max_depth", c_u32), ("rr_threshold", c_f), ("_pad", c_u32)]


class ftn_tile_range(C.Structure):
    _fields_ = [("first", c_u32), ("stride", c_u32), ("count", c_u32), ("_pad", c_u32)]


class ftn_render_options(C.Structure):
    _fields_ = [("pipeline", c_u32), ("device", c_i32), ("count_traffic", c_u32), ("_pad", c_u32)]


class ftn_stats(C.Structure):
    _fields_ = [("rays_closest", c_u64), ("rays_any", c_u64), ("nodes_visited", c_u64), ("prims_tested", c_u64),
                ("camera_samples", c_u64), ("spill_samples", c_u64), ("kernel_ms", C.c_double),
                ("trace_ms", C.c_double), ("trace_launches", c_u64), ("nodes_visited_any", c_u64),
                ("prims_tested_any", c_u64), ("mis_rays_any_hit", c_u64), ("quad_records", c_u64), ("quad_records_any", c_u64),
                ("any_ms", C.c_double), ("any_launches", c_u64), ("shade_ms", C.c_double), ("shade_launches", c_u64), ("sort_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ftn_scene_memory(C.Structure):
    _fields_ = [(k, c_u64) for k in ("nodes", "quad", "oct", "fat", "geom", "srec", "indexed_attributes", "prim_class", "lights", "textures", "other", "total")]


class ftn_gbuffer_pixel(C.Structure):
    """include/fountain_hip_gbuffer.h: per-pixel sums of the first-hit G-buffer (w = box filter weight)."""
    _fields_ = [("albedo", c_f * 3), ("normal", c_f * 3), ("position", c_f * 3), ("depth", c_f), ("hit_weight", c_f), ("weight", c_f)]


FTN_GBUFFER_ABI_VERSION = 1  # include/fountain_hip_gbuffer.h (an extension with a version of its own; FTN_ABI_VERSION is unchanged)


FTN_IDMATTE_SLOTS = 8


class ftn_idmatte_pixel(C.Structure):
    """include/fountain_hip_idmatte.h: a pixel's table of (id, weight) in first-seen order, and what did not enter it."""
    _fields_ = [("id", c_u32 * FTN_IDMATTE_SLOTS), ("weight", c_f * FTN_IDMATTE_SLOTS), ("overflow", c_f), ("miss", c_f), ("total", c_f), ("n_used", c_u32)]


FTN_IDMATTE_ABI_VERSION = 1  # include/fountain_hip_idmatte.h (an extension with a version of its own; FTN_ABI_VERSION is unchanged)
FTN_IDMATTE_RESOLVED_WORDS = 20
FTN_IDMATTE_SELECT_OVERFLOW, FTN_IDMATTE_SELECT_MISS = 1, 2


class ftn_ao_options(C.Structure):
    """include/fountain_hip_ao.h: occlusion rays per recorded surface (1 .. 64) and their t_max (> 0, +inf allowed)."""
    _fields_ = [("rays", c_u32), ("radius", c_f), ("_pad", c_u32 * 2)]


class ftn_ao_pixel(C.Structure):
    """include/fountain_hip_ao.h: per-pixel sums of the ambient-occlusion pass (w = box filter weight)."""
    _fields_ = [("open", c_f), ("bent", c_f * 3), ("hit_weight", c_f), ("weight", c_f), ("_pad", c_f * 2)]


FTN_AO_ABI_VERSION = 1       # include/fountain_hip_ao.h (an extension with a version of its own; FTN_ABI_VERSION is unchanged)
FTN_AO_MAX_RAYS = 64


class ftn_lightpass_pixel(C.Structure):
    """include/fountain_hip_lightpass.h: per-pixel sums of the light-group pass (w = box filter weight)."""
    _fields_ = [("lit", c_f * 3), ("unshadowed", c_f * 3), ("hit_weight", c_f), ("weight", c_f)]


FTN_LIGHTPASS_ABI_VERSION = 1       # include/fountain_hip_lightpass.h (an extension with a version of its own; FTN_ABI_VERSION is unchanged)
FTN_LIGHTPASS_MAX_GROUPS = 16


class ftn_motion_pixel(C.Structure):
    """include/fountain_hip_motion.h: per-pixel sums of the previous-position pass (w = box filter weight)."""
    _fields_ = [("prev_position", c_f * 3), ("prev_normal", c_f * 3), ("hit_weight", c_f), ("weight", c_f)]


FTN_MOTION_ABI_VERSION = 1   # include/fountain_hip_motion.h (an extension with a version of its own; FTN_ABI_VERSION is unchanged)


class ftn_denoise_params(C.Structure):
    """include/fountain_hip_denoise.h: parameters of the a-trous denoiser (ftn_denoise_params_default fills the defaults)."""
    _fields_ = [("levels", C.c_int32), ("flags", c_u32), ("sigma_color", c_f), ("sigma_normal", c_f), ("sigma_plane", c_f),
                ("albedo_eps", c_f), ("color_eps", c_f), ("reserved", c_u32)]


FTN_DENOISE_DEMODULATE = 1
FTN_DENOISE_MAX_LEVELS = 10
FTN_DENOISE_ABI_VERSION = 1  # include/fountain_hip_denoise.h (an extension with a version of its own)


class ftn_denoise_guided_params(C.Structure):
    """include/fountain_hip_denoise_guided.h: parameters of the variance-guided a-trous denoiser (ftn_denoise_guided_params_default)."""
    _fields_ = [("levels", C.c_int32), ("flags", c_u32), ("sigma_variance", c_f), ("sigma_normal", c_f), ("sigma_plane", c_f),
                ("albedo_eps", c_f), ("rel_eps", c_f), ("reserved", c_u32)]


FTN_DENOISE_GUIDED_ABI_VERSION = 1  # include/fountain_hip_denoise_guided.h (an extension with a version of its own)


class ftn_moment_pixel(C.Structure):
    """include/fountain_hip_moments.h: per-pixel sums of the squares of the samples' radiance (box filter weight 1)."""
    _fields_ = [("sq", c_f * 3), ("sq_y", c_f)]


FTN_MOMENTS_ABI_VERSION = 1  # include/fountain_hip_moments.h (an extension with a version of its own)


class ftn_adaptive_params(C.Structure):
    """include/fountain_hip_adaptive.h: the schedule and criterion of per-tile adaptive sampling (ftn_adaptive_params_default fills them)."""
    _fields_ = [("min_samples", c_u32), ("step_samples", c_u32), ("threshold", c_f), ("abs_floor", c_f)]


class ftn_adaptive_info(C.Structure):
    """include/fountain_hip_adaptive.h: what an adaptive call did (rounds, tiles, tiles that reached N, samples in the crop)."""
    _fields_ = [("rounds", c_u32), ("tiles", c_u32), ("tiles_at_max", c_u32), ("_pad", c_u32), ("pixel_samples", c_u64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "_pad"}


FTN_ADAPTIVE_ABI_VERSION = 1  # include/fountain_hip_adaptive.h (an extension with a version of its own)


class ftn_temporal_pixel(C.Structure):
    """include/fountain_hip_temporal.h: one pixel of temporal history (accumulated colour, history length, accumulated variances)."""
    _fields_ = [("u", c_f * 3), ("n", c_f), ("nu", c_f * 4)]


class ftn_temporal_params(C.Structure):
    """include/fountain_hip_temporal.h: parameters of temporal accumulation (ftn_temporal_params_default fills the defaults)."""
    _fields_ = [("flags", c_u32), ("alpha_min", c_f), ("normal_tol", c_f), ("plane_tol", c_f), ("albedo_eps", c_f), ("albedo_tol", c_f),
                ("reserved", c_u32 * 2)]


FTN_TEMPORAL_ABI_VERSION = 1  # include/fountain_hip_temporal.h (an extension with a version of its own)

class ftn_filter_desc(C.Structure):
    """include/fountain_hip_filter.h: a reconstruction filter (ftn_filter_init fills the defaults of a kind)."""
    _fields_ = [("kind", c_u32), ("radius", c_f * 2), ("param", c_f * 2), ("reserved", c_u32 * 3)]


FTN_FILTER_BOX, FTN_FILTER_TRIANGLE, FTN_FILTER_GAUSSIAN, FTN_FILTER_MITCHELL, FTN_FILTER_SINC = range(5)
FTN_FILTER_TABLE_WIDTH = 16
FTN_FILTER_MAX_RADIUS = 8.0
FTN_FILTER_ABI_VERSION = 1  # include/fountain_hip_filter.h (an extension with a version of its own)



class ftn_display_params(C.Structure):
    """include/fountain_hip_display.h: parameters of the display stage (ftn_display_params_default fills the defaults)."""
    _fields_ = [("tonemap", c_u32), ("transfer", c_u32), ("flags", c_u32), ("reserved", c_u32), ("ev", c_f), ("key", c_f), ("white", c_f),
                ("gamma", c_f), ("p_lo", c_f), ("p_hi", c_f), ("min_ev", c_f), ("max_ev", c_f)]


class ftn_display_info(C.Structure):
    """include/fountain_hip_display.h: what ftn_display_exposure found (the scale, the window's mean log2 luminance, the four counts)."""
    _fields_ = [("scale", c_f), ("flags", c_u32), ("avg_log2", C.c_double), ("count_bins", c_u32), ("count_invalid", c_u32),
                ("count_below", c_u32), ("count_above", c_u32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


FTN_DISPLAY_TONEMAP_LINEAR, FTN_DISPLAY_TONEMAP_REINHARD, FTN_DISPLAY_TONEMAP_ACES, FTN_DISPLAY_TONEMAP_HABLE = range(4)
FTN_DISPLAY_TRANSFER_SRGB, FTN_DISPLAY_TRANSFER_GAMMA, FTN_DISPLAY_TRANSFER_LINEAR = range(3)
FTN_DISPLAY_DITHER, FTN_DISPLAY_AUTO_EXPOSURE = 1, 2
FTN_DISPLAY_INFO_EMPTY = 1
FTN_DISPLAY_HIST_BINS, FTN_DISPLAY_HIST_INVALID, FTN_DISPLAY_HIST_BELOW, FTN_DISPLAY_HIST_ABOVE, FTN_DISPLAY_HIST_WORDS = 384, 384, 385, 386, 388
FTN_PNG_GAMA = 1
FTN_DISPLAY_ABI_VERSION = 1  # include/fountain_hip_display.h (an extension with a version of its own)


class ftn_bloom_params(C.Structure):
    """include/fountain_hip_bloom.h: parameters of the bloom stage (ftn_bloom_params_default fills the defaults)."""
    _fields_ = [("levels", c_i32), ("flags", c_u32), ("strength", c_f), ("scatter", c_f), ("threshold", c_f), ("knee", c_f), ("clamp_max", c_f),
                ("reserved", c_u32)]


FTN_BLOOM_KARIS = 1
FTN_BLOOM_MAX_LEVELS = 12
FTN_BLOOM_ABI_VERSION = 1    # include/fountain_hip_bloom.h (an extension with a version of its own)

class ftn_vectorblur_params(C.Structure):
    """include/fountain_hip_vectorblur.h: parameters of the vector-blur stage (ftn_vectorblur_params_default fills the defaults)."""
    _fields_ = [("taps", c_i32), ("flags", c_u32), ("shutter", c_f), ("max_radius", c_f), ("depth_extent", c_f), ("reserved", c_u32 * 3)]


FTN_VECTORBLUR_MAX_TAPS = 64
FTN_VECTORBLUR_MAX_RADIUS = 16
FTN_VECTORBLUR_ABI_VERSION = 1    # include/fountain_hip_vectorblur.h (an extension with a version of its own)


class ftn_metrics_params(C.Structure):
    """include/fountain_hip_metrics.h: parameters of the measuring stage (ftn_metrics_params_default fills the defaults)."""
    _fields_ = [("flags", c_u32), ("peak", c_f), ("rel_eps", c_f), ("reserved", c_u32)]


class ftn_metrics_totals(C.Structure):
    """include/fountain_hip_metrics.h: what the device writes (the eight sums SE, AE, REL, SM, SE_r, SE_g, SE_b, SSIM; the largest
    difference and its pixel; the counts)."""
    _fields_ = [("sum", C.c_double * 8), ("max_abs", C.c_double), ("max_abs_index", C.c_uint64), ("n_pixels", C.c_uint64),
                ("n_nonfinite", C.c_uint64), ("n_different", C.c_uint64), ("n_ssim_windows", C.c_uint64)]


class ftn_metrics_result(C.Structure):
    """include/fountain_hip_metrics.h: what ftn_metrics_resolve makes of the totals."""
    _fields_ = [("mse", C.c_double), ("rmse", C.c_double), ("mae", C.c_double), ("rel_mse", C.c_double), ("smape", C.c_double),
                ("psnr", C.c_double), ("ssim", C.c_double), ("mse_rgb", C.c_double * 3), ("max_abs", C.c_double),
                ("max_abs_index", C.c_uint64), ("n_pixels", C.c_uint64), ("n", C.c_uint64), ("n_nonfinite", C.c_uint64),
                ("n_different", C.c_uint64), ("n_ssim_windows", C.c_uint64)]


FTN_METRICS_SSIM = 1
FTN_METRICS_TILE, FTN_METRICS_SUMS, FTN_METRICS_SSIM_TAPS = 16, 8, 11
FTN_METRICS_ABI_VERSION = 1  # include/fountain_hip_metrics.h (an extension with a version of its own)

FTN_SUBDIV_MAX_LEVELS = 10
FTN_SUBDIV_MAX_FACES = 1 << 26
FTN_SUBDIV_ABI_VERSION = 1   # include/fountain_hip_subdiv.h (an extension with a version of its own)


class ftn_subdiv_info(C.Structure):
    """include/fountain_hip_subdiv.h: the counts of every level of a Loop subdivision (ftn_loop_subdivide_info fills them)."""
    _fields_ = [("levels", c_i32), ("max_valence", c_i32), ("n_vertices", c_u32 * (FTN_SUBDIV_MAX_LEVELS + 1)), ("n_faces", c_u32 * (FTN_SUBDIV_MAX_LEVELS + 1)),
                ("n_edges", c_u32 * (FTN_SUBDIV_MAX_LEVELS + 1)), ("n_boundary", c_u32 * (FTN_SUBDIV_MAX_LEVELS + 1))]


FTN_ABI_VERSION = 3          # include/fountain_hip.h; Backend() refuses a product library that reports another one

# Expected sizes (bytes) -- asserted against the header by the C side's static_asserts and tests/test_abi.py
SIZES = {
    "ftn_transform": 128, "ftn_pixel": 16, "ftn_bvh_node": 32, "ftn_prim": 16, "ftn_mesh": 20,
    "ftn_sphere": 288, "ftn_material": 48, "ftn_light": 160, "ftn_envmap": 16, "ftn_camera_desc": 296,
    "ftn_film_desc": 32, "ftn_sampler_desc": 24, "ftn_integrator_desc": 16, "ftn_tile_range": 16,
    "ftn_render_options": 16, "ftn_stats": 152, "ftn_scene_memory": 96, "ftn_texture": 48, "ftn_image": 24, "ftn_material_textures": 32,
    "ftn_gbuffer_pixel": 48, "ftn_idmatte_pixel": 80, "ftn_ao_options": 16, "ftn_ao_pixel": 32, "ftn_lightpass_pixel": 32, "ftn_motion_pixel": 32, "ftn_denoise_params": 32, "ftn_denoise_guided_params": 32, "ftn_moment_pixel": 16, "ftn_adaptive_params": 16, "ftn_adaptive_info": 24,
    "ftn_temporal_pixel": 32, "ftn_temporal_params": 32, "ftn_filter_desc": 32, "ftn_display_params": 48, "ftn_display_info": 32,
    "ftn_bloom_params": 32, "ftn_vectorblur_params": 32, "ftn_subdiv_info": 184,
    "ftn_metrics_params": 16, "ftn_metrics_totals": 112, "ftn_metrics_result": 136,
}

# Every function the header declares (name -> None); used by the symbol-export test.
DECLARED_FUNCTIONS = [
    "ftn_transform_identity", "ftn_transform_translate", "ftn_transform_scale", "ftn_transform_rotate",
    "ftn_transform_look_at", "ftn_transform_from_flat", "ftn_transform_mul", "ftn_transform_inverse",
    "ftn_transform_perspective", "ftn_transform_point", "ftn_transform_vector", "ftn_transform_normal",
    "ftn_transform_swaps_handedness", "ftn_transform_points", "ftn_transform_normals",
    "ftn_sphere_init", "ftn_camera_perspective", "ftn_film_init",
    "ftn_film_sample_bounds", "ftn_film_tile_count", "ftn_film_resolve", "ftn_scene_create",
    "ftn_scene_destroy", "ftn_bvh_build", "ftn_bvh_quads", "ftn_bvh_octs", "ftn_scene_info", "ftn_scene_get_nodes", "ftn_scene_get_lights",
    "ftn_intersect", "ftn_intersect_test", "ftn_intersect_full", "ftn_render", "ftn_render_device",
    "ftn_last_error", "ftn_device_count", "ftn_version", "ftn_abi_version", "ftn_scene_memory_info", "ftn_test_math",
    "ftn_pbrt_load", "ftn_pbrt_destroy", "ftn_pbrt_scene", "ftn_pbrt_camera", "ftn_pbrt_film",
    "ftn_pbrt_samples_per_pixel", "ftn_pbrt_film_name", "ftn_pbrt_last_error", "ftn_ply_load",
    "ftn_test_mipmap_level", "ftn_test_texture_eval", "ftn_test_bsdf", "ftn_test_light", "ftn_test_interaction", "ftn_test_camera", "ftn_test_material", "ftn_film_resolve_device", "ftn_exr_write", "ftn_exr_read", "ftn_imageio_last_error", "ftn_image_inverse_gamma",
]

# ftn_test_bsdf (the BSDF test hook): floats per input / output row, the BxDFType bits of `flags`, the argument types
FTN_TEST_BSDF_IN, FTN_TEST_BSDF_OUT = 17, 16
BSDF_REFLECTION, BSDF_TRANSMISSION, BSDF_DIFFUSE, BSDF_GLOSSY, BSDF_SPECULAR, BSDF_ALL = 1, 2, 4, 8, 16, 31
TEST_BSDF_ARGTYPES = [C.c_void_p, c_i32, c_u32, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
# ftn_test_light (the light test hook): floats per input / output row, the argument types
FTN_TEST_LIGHT_IN, FTN_TEST_LIGHT_OUT = 15, 24
TEST_LIGHT_ARGTYPES = [C.c_void_p, c_i32, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
# ftn_test_interaction / ftn_test_camera (the surface-interaction and camera test hooks): floats per input / output row, the argument types
FTN_TEST_INTERACTION_IN, FTN_TEST_INTERACTION_OUT = 32, 68
TEST_INTERACTION_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
FTN_TEST_CAMERA_IN, FTN_TEST_CAMERA_OUT = 8, 20
TEST_CAMERA_ARGTYPES = [C.c_void_p, c_u32, C.c_void_p, C.c_size_t, C.c_void_p]
# ftn_test_material (the textured-material test hook): floats per input / output row, the argument types
FTN_TEST_MATERIAL_IN, FTN_TEST_MATERIAL_OUT = 6, 16
TEST_MATERIAL_ARGTYPES = [C.c_void_p, c_i32, C.c_void_p, C.c_size_t, C.c_void_p]

# The functions of fountain_hip.h that api.py calls with declared types, name without the backend's prefix -> (argument types, result
# type); Backend() applies them once.  CORE_TWINS are the ones the oracle's orc_* twins get as well; the rest exist in the product
# library alone.  Every other function of the header is called with ctypes' default conversions (some, such as scene_create, intersect*
# and render, differ between the backends).
CORE_PROTOTYPES = {
    "last_error": (None, C.c_char_p),
    "transform_scale": ([c_f, c_f, c_f, C.c_void_p], C.c_int),
    "transform_rotate": ([c_f, C.c_void_p, C.c_void_p], C.c_int),
    "transform_perspective": ([c_f, c_f, c_f, C.c_void_p], C.c_int),
    "sphere_init": ([C.c_void_p, C.c_void_p, C.c_int, c_f, c_f, c_f, c_f, C.c_void_p], C.c_int),
    "camera_perspective": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_f, c_f, c_f, C.c_void_p], C.c_int),
    "test_interaction": (TEST_INTERACTION_ARGTYPES, C.c_int),
    "test_camera": (TEST_CAMERA_ARGTYPES, C.c_int),
    "pbrt_load": ([C.c_char_p, C.POINTER(C.c_void_p)], C.c_int),
    "pbrt_destroy": ([C.c_void_p], None),
    "pbrt_scene": ([C.c_void_p], C.POINTER(ftn_scene_desc)),
    "pbrt_camera": ([C.c_void_p], C.POINTER(ftn_camera_desc)),
    "pbrt_film": ([C.c_void_p], C.POINTER(ftn_film_desc)),
    "pbrt_samples_per_pixel": ([C.c_void_p], C.c_int),
    "pbrt_film_name": ([C.c_void_p], C.c_char_p),
    "pbrt_last_error": (None, C.c_char_p),
    "ply_load": ([C.c_char_p] + [C.c_void_p] * 8, C.c_int),
    "film_resolve_device": ([C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p], C.c_int),
    "exr_write": ([C.c_char_p, C.c_void_p, c_u32, c_u32], C.c_int),
    "exr_read": ([C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "imageio_last_error": (None, C.c_char_p),
}
CORE_TWINS = ("last_error", "transform_scale", "transform_rotate", "transform_perspective", "sphere_init", "camera_perspective",
              "test_interaction", "test_camera")

# The extension headers, one table each: every function the header declares, name -> (argument types, result type).  They are kept
# apart from DECLARED_FUNCTIONS, which mirrors fountain_hip.h alone: the reference has none of these calls, so none has an orc_* twin.
# X_FUNCTIONS is the sorted list of a table's names; EXTENSIONS at the end of this file is the registry _nontwin.bind works from.
_VP = C.c_void_p
_RENDER_ARGS = [_VP] * 8                                    # scene, camera, film, filter, sampler, integrator, tiles, options

# include/fountain_hip_gbuffer.h
GBUFFER_PROTOTYPES = {
    "ftn_render_gbuffer": ([_VP] * 8, C.c_int),
    "ftn_render_gbuffer_device": ([_VP] * 9, C.c_int),
    "ftn_gbuffer_resolve": ([_VP, C.c_size_t, _VP], C.c_int),
    "ftn_gbuffer_resolve_device": ([_VP, C.c_size_t, _VP, _VP], C.c_int),
    "ftn_gbuffer_abi_version": ([], C.c_int),
}
GBUFFER_FUNCTIONS = sorted(GBUFFER_PROTOTYPES)

# include/fountain_hip_denoise.h and include/fountain_hip_denoise_guided.h (whose calls take var4 after gb12)
DENOISE_PROTOTYPES = {
    "ftn_denoise_params_default": ([_VP], None),
    "ftn_denoise": ([_VP, _VP, c_i32, c_i32, _VP, _VP, c_i32], C.c_int),
    "ftn_denoise_workspace_size": ([c_i32, c_i32, _VP], C.c_int),
    "ftn_denoise_device": ([_VP, _VP, c_i32, c_i32, _VP, _VP, _VP, _VP], C.c_int),
    "ftn_denoise_cpu": ([_VP, _VP, c_i32, c_i32, _VP, _VP], C.c_int),
    "ftn_denoise_abi_version": ([], C.c_int),
}
DENOISE_FUNCTIONS = sorted(DENOISE_PROTOTYPES)
DENOISE_GUIDED_PROTOTYPES = {
    "ftn_denoise_guided_params_default": ([_VP], None),
    "ftn_denoise_guided": ([_VP] * 3 + [c_i32, c_i32, _VP, _VP, c_i32], C.c_int),
    "ftn_denoise_guided_workspace_size": ([c_i32, c_i32, _VP], C.c_int),
    "ftn_denoise_guided_device": ([_VP] * 3 + [c_i32, c_i32, _VP, _VP, _VP, _VP], C.c_int),
    "ftn_denoise_guided_cpu": ([_VP] * 3 + [c_i32, c_i32, _VP, _VP], C.c_int),
    "ftn_denoise_guided_abi_version": ([], C.c_int),
}
DENOISE_GUIDED_FUNCTIONS = sorted(DENOISE_GUIDED_PROTOTYPES)

# include/fountain_hip_moments.h
MOMENTS_PROTOTYPES = {
    "ftn_render_moments": ([_VP] * 10, C.c_int),
    "ftn_render_moments_device": ([_VP] * 11, C.c_int),
    "ftn_moments_resolve": ([_VP, _VP, C.c_size_t, _VP], C.c_int),
    "ftn_moments_resolve_device": ([_VP, _VP, C.c_size_t, _VP, _VP], C.c_int),
    "ftn_moments_abi_version": ([], C.c_int),
}
MOMENTS_FUNCTIONS = sorted(MOMENTS_PROTOTYPES)

# include/fountain_hip_adaptive.h
ADAPTIVE_PROTOTYPES = {
    "ftn_adaptive_params_default": ([_VP], None),
    "ftn_render_adaptive": ([_VP] * 13, C.c_int),
    "ftn_render_adaptive_device": ([_VP] * 14, C.c_int),
    "ftn_adaptive_converged": ([_VP, _VP, C.c_size_t, _VP, _VP], C.c_int),
    "ftn_adaptive_abi_version": ([], C.c_int),
}
ADAPTIVE_FUNCTIONS = sorted(ADAPTIVE_PROTOTYPES)

# include/fountain_hip_temporal.h
_TEMPORAL = [_VP] * 5 + [c_i32, c_i32] + [_VP] * 7     # rgb, gb12, var4, camera, film, w, h, the previous three, params, the outputs
TEMPORAL_PROTOTYPES = {
    "ftn_temporal_params_default": ([_VP], None),
    "ftn_temporal_accumulate": (_TEMPORAL + [c_i32], C.c_int),
    "ftn_temporal_accumulate_device": (_TEMPORAL + [_VP], C.c_int),
    "ftn_temporal_accumulate_cpu": (_TEMPORAL, C.c_int),
    "ftn_temporal_abi_version": ([], C.c_int),
}
TEMPORAL_FUNCTIONS = sorted(TEMPORAL_PROTOTYPES)

# include/fountain_hip_filter.h
FILTER_PROTOTYPES = {
    "ftn_filter_init": ([c_u32, C.c_void_p], C.c_int),
    "ftn_filter_table": ([C.c_void_p, C.c_void_p], C.c_int),
    "ftn_render_filtered": (_RENDER_ARGS + [C.c_void_p, C.c_void_p], C.c_int),
    "ftn_render_filtered_device": (_RENDER_ARGS + [C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "ftn_filter_accumulate_samples": ([C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 6, C.c_int),
    "ftn_pbrt_filter": ([C.c_void_p, C.c_void_p], C.c_int),
    "ftn_filter_abi_version": ([], C.c_int),
}
FILTER_FUNCTIONS = sorted(FILTER_PROTOTYPES)

# include/fountain_hip_display.h
_IMG = [C.c_void_p, c_i32, c_i32]
DISPLAY_PROTOTYPES = {
    "ftn_display_params_default": ([C.c_void_p], None),
    "ftn_display_histogram": (_IMG + [C.c_void_p, c_i32], C.c_int),
    "ftn_display_histogram_device": (_IMG + [C.c_void_p, C.c_void_p], C.c_int),
    "ftn_display_histogram_cpu": (_IMG + [C.c_void_p], C.c_int),
    "ftn_display_exposure": ([C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "ftn_display_encode": (_IMG + [C.c_void_p, c_f, C.c_void_p, C.c_void_p, c_i32], C.c_int),
    "ftn_display_encode_device": (_IMG + [C.c_void_p, c_f, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "ftn_display_encode_cpu": (_IMG + [C.c_void_p, c_f, C.c_void_p, C.c_void_p], C.c_int),
    "ftn_display": (_IMG + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_i32], C.c_int),
    "ftn_png_write": ([C.c_char_p, C.c_void_p, c_u32, c_u32, c_u32], C.c_int),
    "ftn_display_abi_version": ([], C.c_int),
}
DISPLAY_FUNCTIONS = sorted(DISPLAY_PROTOTYPES)

# include/fountain_hip_bloom.h
BLOOM_PROTOTYPES = {
    "ftn_bloom_params_default": ([C.c_void_p], None),
    "ftn_bloom": (_IMG + [C.c_void_p, C.c_void_p, c_i32], C.c_int),
    "ftn_bloom_workspace_size": ([c_i32, c_i32, c_i32, C.c_void_p], C.c_int),
    "ftn_bloom_device": (_IMG + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "ftn_bloom_cpu": (_IMG + [C.c_void_p, C.c_void_p], C.c_int),
    "ftn_bloom_abi_version": ([], C.c_int),
}
BLOOM_FUNCTIONS = sorted(BLOOM_PROTOTYPES)

# include/fountain_hip_vectorblur.h
_BLUR = [C.c_void_p, C.c_void_p, C.c_void_p, c_i32, c_i32, C.c_void_p]      # rgb, motion2, gb12, w, h, params
VECTORBLUR_PROTOTYPES = {
    "ftn_vectorblur_params_default": ([C.c_void_p], None),
    "ftn_vectorblur": (_BLUR + [C.c_void_p, c_i32], C.c_int),
    "ftn_vectorblur_workspace_size": ([c_i32, c_i32, C.c_void_p], C.c_int),
    "ftn_vectorblur_device": (_BLUR + [C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "ftn_vectorblur_cpu": (_BLUR + [C.c_void_p], C.c_int),
    "ftn_vectorblur_velocities_cpu": (_BLUR[1:] + [C.c_void_p], C.c_int),
    "ftn_vectorblur_abi_version": ([], C.c_int),
}
VECTORBLUR_FUNCTIONS = sorted(VECTORBLUR_PROTOTYPES)

# include/fountain_hip_metrics.h
_PAIR = [C.c_void_p, C.c_void_p, c_i32, c_i32, C.c_void_p]      # test, ref, w, h, params
METRICS_PROTOTYPES = {
    "ftn_metrics_params_default": ([C.c_void_p], None),
    "ftn_metrics_workspace_size": ([c_i32, c_i32, c_u32, C.c_void_p], C.c_int),
    "ftn_metrics_ssim_weights": ([C.c_void_p], C.c_int),
    "ftn_metrics": (_PAIR + [C.c_void_p] * 5 + [c_i32], C.c_int),
    "ftn_metrics_device": (_PAIR + [C.c_void_p] * 6, C.c_int),
    "ftn_metrics_resolve": ([C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "ftn_metrics_cpu": (_PAIR + [C.c_void_p] * 5, C.c_int),
    "ftn_metrics_abi_version": ([], C.c_int),
}
METRICS_FUNCTIONS = sorted(METRICS_PROTOTYPES)

# include/fountain_hip_subdiv.h
_CAGE = [C.c_void_p, c_i32, C.c_void_p, c_i32, c_i32]      # P, n_vertices, indices, n_faces, levels
SUBDIV_PROTOTYPES = {
    "ftn_loop_subdivide_info": ([C.c_void_p, c_i32, c_i32, c_i32, C.c_void_p], C.c_int),
    "ftn_loop_subdivide": (_CAGE + [C.c_void_p, C.c_void_p, C.c_void_p, c_i32], C.c_int),
    "ftn_loop_subdivide_cpu": (_CAGE + [C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "ftn_subdiv_abi_version": ([], C.c_int),
}
SUBDIV_FUNCTIONS = sorted(SUBDIV_PROTOTYPES)

# include/fountain_hip_idmatte.h
_STRINGS = C.POINTER(C.c_char_p)
IDMATTE_PROTOTYPES = {
    "ftn_render_idmatte": ([C.c_void_p] * 7 + [C.c_size_t, C.c_void_p, C.c_void_p], C.c_int),
    "ftn_render_idmatte_device": ([C.c_void_p] * 7 + [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "ftn_idmatte_resolve": ([C.c_void_p, C.c_size_t, C.c_void_p], C.c_int),
    "ftn_idmatte_resolve_device": ([C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p], C.c_int),
    "ftn_idmatte_select": ([C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, c_u32, C.c_void_p], C.c_int),
    "ftn_idmatte_select_device": ([C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, c_u32, C.c_void_p, C.c_void_p], C.c_int),
    "ftn_exr_write_channels": ([C.c_char_p, c_i32, c_i32, c_i32, _STRINGS, C.POINTER(C.c_void_p), c_i32, _STRINGS, _STRINGS], C.c_int),
    "ftn_idmatte_abi_version": ([], C.c_int),
}
IDMATTE_FUNCTIONS = sorted(IDMATTE_PROTOTYPES)

# include/fountain_hip_ao.h
AO_PROTOTYPES = {
    "ftn_render_ao": ([C.c_void_p] * 9, C.c_int),
    "ftn_render_ao_device": ([C.c_void_p] * 10, C.c_int),
    "ftn_ao_resolve": ([C.c_void_p, C.c_size_t, c_u32, C.c_void_p], C.c_int),
    "ftn_ao_resolve_device": ([C.c_void_p, C.c_size_t, c_u32, C.c_void_p, C.c_void_p], C.c_int),
    "ftn_ao_rays": ([C.c_void_p, C.c_void_p, C.c_size_t, c_f, C.c_void_p], C.c_int),
    "ftn_ao_abi_version": ([], C.c_int),
}
AO_FUNCTIONS = sorted(AO_PROTOTYPES)

# include/fountain_hip_lightpass.h
LIGHTPASS_PROTOTYPES = {
    "ftn_render_lightpass": ([C.c_void_p] * 7 + [c_u32] + [C.c_void_p] * 2, C.c_int),
    "ftn_render_lightpass_device": ([C.c_void_p] * 7 + [c_u32] + [C.c_void_p] * 3, C.c_int),
    "ftn_lightpass_resolve": ([C.c_void_p, C.c_size_t, C.c_void_p], C.c_int),
    "ftn_lightpass_resolve_device": ([C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p], C.c_int),
    "ftn_lightpass_compose": ([C.c_void_p, C.c_void_p, c_u32, C.c_void_p, C.c_size_t, C.c_void_p], C.c_int),
    "ftn_lightpass_compose_device": ([C.c_void_p, C.c_void_p, c_u32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p], C.c_int),
    "ftn_lightpass_terms": ([C.c_void_p, C.c_void_p, C.c_size_t, c_u32, C.c_void_p, C.c_void_p], C.c_int),
    "ftn_lightpass_abi_version": ([], C.c_int),
}
LIGHTPASS_FUNCTIONS = sorted(LIGHTPASS_PROTOTYPES)

# include/fountain_hip_motion.h
_TEMPORAL_MOTION = [C.c_void_p] * 6 + [c_i32, c_i32] + [C.c_void_p] * 7
MOTION_PROTOTYPES = {
    "ftn_render_motion": ([C.c_void_p] * 9, C.c_int),
    "ftn_render_motion_device": ([C.c_void_p] * 10, C.c_int),
    "ftn_motion_resolve": ([C.c_void_p, C.c_size_t, C.c_void_p], C.c_int),
    "ftn_motion_resolve_device": ([C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p], C.c_int),
    "ftn_motion_vectors": ([C.c_void_p] * 5 + [c_i32, c_i32, C.c_void_p, c_i32], C.c_int),
    "ftn_motion_vectors_device": ([C.c_void_p] * 5 + [c_i32, c_i32, C.c_void_p, C.c_void_p], C.c_int),
    "ftn_motion_vectors_cpu": ([C.c_void_p] * 5 + [c_i32, c_i32, C.c_void_p], C.c_int),
    "ftn_temporal_accumulate_motion": (_TEMPORAL_MOTION + [c_i32], C.c_int),
    "ftn_temporal_accumulate_motion_device": (_TEMPORAL_MOTION + [C.c_void_p], C.c_int),
    "ftn_temporal_accumulate_motion_cpu": (_TEMPORAL_MOTION, C.c_int),
    "ftn_motion_abi_version": ([], C.c_int),
}
MOTION_FUNCTIONS = sorted(MOTION_PROTOTYPES)


# One extension header as _nontwin.bind needs it: the header's file, its ABI-version function and the version this binding was written
# for, its prototypes, and the words of the two refusals -- `what` names the extension where the library reports another version,
# `no_twin` is the sentence the oracle backend is refused with.
Extension = namedtuple("Extension", "header abi_version_fn abi_version prototypes what no_twin")

EXTENSIONS = {
    "gbuffer": Extension("fountain_hip_gbuffer.h", "ftn_gbuffer_abi_version", FTN_GBUFFER_ABI_VERSION, GBUFFER_PROTOTYPES, "G-buffer",
                          "the G-buffer pass has no oracle twin: the reference renders no G-buffer"),
    "denoise": Extension("fountain_hip_denoise.h", "ftn_denoise_abi_version", FTN_DENOISE_ABI_VERSION, DENOISE_PROTOTYPES, "denoise",
                          "the denoiser has no oracle twin: the reference has no denoiser"),
    "denoise_guided": Extension("fountain_hip_denoise_guided.h", "ftn_denoise_guided_abi_version", FTN_DENOISE_GUIDED_ABI_VERSION, DENOISE_GUIDED_PROTOTYPES, "guided denoise",
                                 "the denoiser has no oracle twin: the reference has no denoiser"),
    "moments": Extension("fountain_hip_moments.h", "ftn_moments_abi_version", FTN_MOMENTS_ABI_VERSION, MOMENTS_PROTOTYPES, "moments",
                          "the moments pass has no oracle twin: the reference keeps no second moments"),
    "adaptive": Extension("fountain_hip_adaptive.h", "ftn_adaptive_abi_version", FTN_ADAPTIVE_ABI_VERSION, ADAPTIVE_PROTOTYPES, "adaptive",
                           "adaptive sampling has no oracle twin: the reference has no adaptive sampling"),
    "temporal": Extension("fountain_hip_temporal.h", "ftn_temporal_abi_version", FTN_TEMPORAL_ABI_VERSION, TEMPORAL_PROTOTYPES, "temporal",
                           "temporal accumulation has no oracle twin: the reference renders single frames"),
    "filter": Extension("fountain_hip_filter.h", "ftn_filter_abi_version", FTN_FILTER_ABI_VERSION, FILTER_PROTOTYPES, "filter",
                         "the filtered film has no oracle twin: the reference's only filter is the box"),
    "display": Extension("fountain_hip_display.h", "ftn_display_abi_version", FTN_DISPLAY_ABI_VERSION, DISPLAY_PROTOTYPES, "display",
                          "the display stage has no oracle twin: the reference writes linear OpenEXR files only"),
    "bloom": Extension("fountain_hip_bloom.h", "ftn_bloom_abi_version", FTN_BLOOM_ABI_VERSION, BLOOM_PROTOTYPES, "bloom",
                        "the bloom stage has no oracle twin: the reference writes linear OpenEXR files only"),
    "vectorblur": Extension("fountain_hip_vectorblur.h", "ftn_vectorblur_abi_version", FTN_VECTORBLUR_ABI_VERSION, VECTORBLUR_PROTOTYPES, "vector-blur",
                             "the vector-blur stage has no oracle twin: the reference renders single frames without a shutter"),
    "metrics": Extension("fountain_hip_metrics.h", "ftn_metrics_abi_version", FTN_METRICS_ABI_VERSION, METRICS_PROTOTYPES, "metrics",
                          "the measuring stage has no oracle twin: the reference compares no images"),
    "subdiv": Extension("fountain_hip_subdiv.h", "ftn_subdiv_abi_version", FTN_SUBDIV_ABI_VERSION, SUBDIV_PROTOTYPES, "subdivision",
                         ""),
    "idmatte": Extension("fountain_hip_idmatte.h", "ftn_idmatte_abi_version", FTN_IDMATTE_ABI_VERSION, IDMATTE_PROTOTYPES, "ID-matte",
                          "the ID-matte pass has no oracle twin: the reference renders no mattes"),
    "ao": Extension("fountain_hip_ao.h", "ftn_ao_abi_version", FTN_AO_ABI_VERSION, AO_PROTOTYPES, "ambient-occlusion",
                     "the ambient-occlusion pass has no oracle twin: the reference has no such integrator"),
    "lightpass": Extension("fountain_hip_lightpass.h", "ftn_lightpass_abi_version", FTN_LIGHTPASS_ABI_VERSION, LIGHTPASS_PROTOTYPES, "light-pass",
                            "the light-group pass has no oracle twin: the reference has no light AOVs"),
    "motion": Extension("fountain_hip_motion.h", "ftn_motion_abi_version", FTN_MOTION_ABI_VERSION, MOTION_PROTOTYPES, "motion",
                         "the previous-position pass has no oracle twin: the reference renders single frames"),
}
