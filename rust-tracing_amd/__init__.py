"""ctypes bindings of the two shared libraries of this package.

  librt_amd.so   csrc/  — the HIP renderer behind the C ABI of include/rt_amd.h (the product)
  librt_host.so  host/  — the reference's host-side surface (scene builders, BVH build, camera, output stage)
                          behind include/rt_host.h

Python is plumbing here: tests and bench.py use it to hold device memory (torch), to launch one process per
GPU (torch.distributed) and to call the C ABI.  Nothing in this module computes pixels, and there is no
fallback: if librt_amd.so is missing or has no GPU to run on, calls raise.

The package directory is named ``rust-tracing_amd`` (not importable with a plain ``import`` statement); load it
with ``importlib.import_module("rust-tracing_amd")``.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

_PKG_DIR = Path(__file__).resolve().parent
LIB_DIR = _PKG_DIR / "lib"

RT_ABI_VERSION = 2
RT_TILE_W = 8
RT_TILE_H = 8
RT_OUT_FRAME = 0
RT_OUT_TILES = 1

# rt_hittable_kind
RT_HITTABLE_NONE, RT_HITTABLE_SPHERE, RT_HITTABLE_QUAD, RT_HITTABLE_LIST, RT_HITTABLE_TRANSLATE, \
    RT_HITTABLE_ROTATE_Y, RT_HITTABLE_BVH, RT_HITTABLE_CONSTANT_MEDIUM = range(8)
# rt_material_kind
RT_MATERIAL_LAMBERTIAN, RT_MATERIAL_METAL, RT_MATERIAL_DIELECTRIC, RT_MATERIAL_DIFFUSE_LIGHT, \
    RT_MATERIAL_ISOTROPIC = range(1, 6)
# rt_texture_kind
RT_TEXTURE_SOLID, RT_TEXTURE_CHECKER, RT_TEXTURE_IMAGE, RT_TEXTURE_NOISE = range(1, 5)


class Vec3(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("z", C.c_double)]

    def tuple(self):
        return (self.x, self.y, self.z)


class Aabb(C.Structure):
    _fields_ = [("lo", C.c_double * 3), ("hi", C.c_double * 3)]


class Ref(C.Structure):
    _fields_ = [("kind", C.c_int32), ("index", C.c_int32)]


class Sphere(C.Structure):
    _fields_ = [("center", Vec3), ("radius", C.c_double), ("center_vec", Vec3), ("is_moving", C.c_int32),
                ("material", C.c_int32)]


class Quad(C.Structure):
    _fields_ = [("q", Vec3), ("u", Vec3), ("v", Vec3), ("w", Vec3), ("normal", Vec3), ("d", C.c_double),
                ("material", C.c_int32), ("_pad", C.c_int32)]


class List(C.Structure):
    _fields_ = [("first", C.c_int32), ("count", C.c_int32)]


class Translate(C.Structure):
    _fields_ = [("object", Ref), ("offset", Vec3)]


class RotateY(C.Structure):
    _fields_ = [("object", Ref), ("sin_theta", C.c_double), ("cos_theta", C.c_double)]


class BvhNode(C.Structure):
    _fields_ = [("bbox", Aabb), ("is_leaf", C.c_int32), ("left", C.c_int32), ("right", C.c_int32),
                ("object", Ref), ("_pad", C.c_int32)]


class Bvh(C.Structure):
    _fields_ = [("root", C.c_int32), ("_pad", C.c_int32)]


class ConstantMedium(C.Structure):
    _fields_ = [("boundary", Ref), ("neg_inv_density", C.c_double), ("phase_material", C.c_int32),
                ("_pad", C.c_int32)]


class Material(C.Structure):
    _fields_ = [("kind", C.c_int32), ("texture", C.c_int32), ("albedo", Vec3), ("fuzz", C.c_double),
                ("ir", C.c_double)]


class Texture(C.Structure):
    _fields_ = [("kind", C.c_int32), ("even", C.c_int32), ("odd", C.c_int32), ("image", C.c_int32),
                ("perlin", C.c_int32), ("_pad", C.c_int32), ("color", Vec3), ("inv_scale", C.c_double),
                ("scale", C.c_double)]


class Perlin(C.Structure):
    _fields_ = [("ranvec", Vec3 * 256), ("perm_x", C.c_int32 * 256), ("perm_y", C.c_int32 * 256),
                ("perm_z", C.c_int32 * 256)]


class Image(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("rgb", C.POINTER(C.c_uint8))]


class SceneDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("_pad", C.c_uint32), ("world", Ref),
                ("n_spheres", C.c_int32), ("n_quads", C.c_int32), ("n_lists", C.c_int32),
                ("n_list_items", C.c_int32), ("n_translates", C.c_int32), ("n_rotates", C.c_int32),
                ("n_bvh_nodes", C.c_int32), ("n_bvhs", C.c_int32), ("n_media", C.c_int32),
                ("n_materials", C.c_int32), ("n_textures", C.c_int32), ("n_perlins", C.c_int32),
                ("n_images", C.c_int32), ("_pad2", C.c_int32),
                ("spheres", C.POINTER(Sphere)), ("quads", C.POINTER(Quad)), ("lists", C.POINTER(List)),
                ("list_items", C.POINTER(Ref)), ("translates", C.POINTER(Translate)),
                ("rotates", C.POINTER(RotateY)), ("bvh_nodes", C.POINTER(BvhNode)), ("bvhs", C.POINTER(Bvh)),
                ("media", C.POINTER(ConstantMedium)), ("materials", C.POINTER(Material)),
                ("textures", C.POINTER(Texture)), ("perlins", C.POINTER(Perlin)), ("images", C.POINTER(Image))]


class Camera(C.Structure):
    _fields_ = [("image_width", C.c_int32), ("image_height", C.c_int32), ("samples_per_pixel", C.c_int32),
                ("max_depth", C.c_int32), ("background", Vec3), ("center", Vec3), ("pixel00_loc", Vec3),
                ("pixel_delta_u", Vec3), ("pixel_delta_v", Vec3), ("defocus_angle", C.c_double),
                ("defocus_disk_u", Vec3), ("defocus_disk_v", Vec3)]


class RenderParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("sample_begin", C.c_int32), ("sample_end", C.c_int32),
                ("max_depth", C.c_int32), ("accumulate", C.c_int32), ("shard_index", C.c_int32),
                ("shard_count", C.c_int32), ("out_layout", C.c_int32), ("device", C.c_int32)]


class View(C.Structure):
    """rt_view: one camera of rt_render_views with its seed."""
    _fields_ = [("camera", Camera), ("seed", C.c_uint64)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("samples", "rays", "node_visits", "sphere_tests", "quad_tests",
                                          "medium_visits", "rng_draws", "noise_evals", "image_lookups",
                                          "instance_enters")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class SceneStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("node_bytes", "sphere_bytes", "quad_bytes", "instance_bytes",
                                          "medium_bytes", "material_bytes", "texture_bytes", "perlin_bytes",
                                          "image_bytes")] + \
               [(n, C.c_uint32) for n in ("n_nodes", "n_spheres", "n_quads", "n_instances", "n_media",
                                          "max_instance_depth", "lds_nodes", "lds_bytes", "ordered",
                                          "stack_entries")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class SceneOptions(C.Structure):
    _fields_ = [("scene", C.c_int32), ("bvh_policy", C.c_int32), ("scene_seed", C.c_uint64),
                ("image_width", C.c_int64), ("aspect_ratio", C.c_double), ("samples_per_pixel", C.c_int32),
                ("max_depth", C.c_int32), ("earth_image", C.c_char_p)]


RT_WALK_DEFAULT, RT_WALK_REFERENCE_ORDER, RT_WALK_AUTO, RT_WALK_OWN_TREES = -1, 0, 1, 2
RT_COMM_ID_BYTES = 128


class SceneCreateOptions(C.Structure):
    """rt_scene_options (per-scene options of rt_scene_create_ex)."""
    _fields_ = [("struct_size", C.c_uint32), ("walk", C.c_int32), ("leaf_max", C.c_int32), ("refit", C.c_int32),
                ("use_lds", C.c_int32), ("th_prim", C.c_int32), ("th_other", C.c_int32), ("th_shade", C.c_int32),
                ("th_box", C.c_int32), ("th_new", C.c_int32), ("sample_buffer_bytes", C.c_int64), ("reserved_pool", C.c_int32),
                ("flat_max", C.c_int32), ("start_shortcut", C.c_int32), ("defer_instances", C.c_int32),
                ("seq_lookahead", C.c_int32), ("slow_min", C.c_int32), ("slow_age", C.c_int32), ("wide", C.c_int32),
                ("quad_filter", C.c_int32), ("medium_first", C.c_int32)]


def _params(cls, init, c_name, kw, *, sized=True, convert=None):
    """The body of every *_params(**kw) below: a `cls` filled by the library's `init` (with the struct's size where it takes one),
    then the given fields, each through its entry in `convert` if it has one."""
    p = cls()
    if sized:
        _check(getattr(amd_lib(), init)(C.byref(p), C.sizeof(p)), init)
    else:
        getattr(amd_lib(), init)(C.byref(p))
    for k, v in kw.items():
        if k not in dict(cls._fields_):
            raise TypeError(f"{c_name} has no field {k}")
        setattr(p, k, convert[k](v) if convert and k in convert else v)
    return p


def scene_options(**kw) -> "SceneCreateOptions":
    """rt_scene_options_init, then the given fields (walk=, leaf_max=, flat_max=, refit=, use_lds=, th_*=, sample_buffer_bytes=,
    start_shortcut=, defer_instances=, seq_lookahead=, slow_min=, slow_age=, quad_filter=, medium_first=)."""
    return _params(SceneCreateOptions, "rt_scene_options_init", "rt_scene_options", kw, sized=False)


class AdaptiveParams(C.Structure):
    """rt_adaptive_params (rt_render_adaptive)."""
    _fields_ = [("struct_size", C.c_uint32), ("min_spp", C.c_int32), ("batch_spp", C.c_int32), ("_pad", C.c_int32),
                ("rel_threshold", C.c_double), ("abs_threshold", C.c_double)]


class AdaptiveResult(C.Structure):
    _fields_ = [("samples", C.c_int64), ("launches", C.c_int32), ("converged", C.c_int32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


def adaptive_params(**kw) -> "AdaptiveParams":
    """rt_adaptive_params_init_sized, then the given fields (min_spp=, batch_spp=, rel_threshold=, abs_threshold=)."""
    return _params(AdaptiveParams, "rt_adaptive_params_init_sized", "rt_adaptive_params", kw)


class DenoiseParams(C.Structure):
    """rt_denoise_params (rt_denoise_device)."""
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_int32), ("sigma", C.c_double), ("eps", C.c_double)]


def denoise_params(**kw) -> "DenoiseParams":
    """rt_denoise_params_init_sized, then the given fields (iterations=, sigma=, eps=)."""
    return _params(DenoiseParams, "rt_denoise_params_init_sized", "rt_denoise_params", kw)


class DenoiseAlbedoParams(C.Structure):
    """rt_denoise_albedo_params (rt_denoise_albedo_device)."""
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_int32), ("sigma", C.c_double), ("eps", C.c_double),
                ("sigma_albedo", C.c_double), ("albedo_floor", C.c_double)]


def denoise_albedo_params(**kw) -> "DenoiseAlbedoParams":
    """rt_denoise_albedo_params_init_sized, then the given fields (iterations=, sigma=, eps=, sigma_albedo=, albedo_floor=)."""
    return _params(DenoiseAlbedoParams, "rt_denoise_albedo_params_init_sized", "rt_denoise_albedo_params", kw)


class DenoiseGuidedParams(C.Structure):
    """rt_denoise_guided_params (rt_denoise_guided_device and its _mean, _mean_spatial and _views forms)."""
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_int32), ("sigma", C.c_double), ("eps", C.c_double),
                ("sigma_albedo", C.c_double), ("albedo_floor", C.c_double), ("sigma_edge", C.c_double)]


def denoise_guided_params(**kw) -> "DenoiseGuidedParams":
    """rt_denoise_guided_params_init_sized, then the given fields (iterations=, sigma=, eps=, sigma_albedo=, albedo_floor=, sigma_edge=)."""
    return _params(DenoiseGuidedParams, "rt_denoise_guided_params_init_sized", "rt_denoise_guided_params", kw)


class DenoiseSpatialParams(C.Structure):
    """rt_denoise_spatial_params (rt_denoise_mean_spatial_device, rt_denoise_albedo_mean_spatial_device)."""
    _fields_ = [("struct_size", C.c_uint32), ("spatial_below", C.c_int32), ("window_radius", C.c_int32)]


def denoise_spatial_params(**kw) -> "DenoiseSpatialParams":
    """rt_denoise_spatial_params_init_sized, then the given fields (spatial_below=, window_radius=)."""
    return _params(DenoiseSpatialParams, "rt_denoise_spatial_params_init_sized", "rt_denoise_spatial_params", kw)


RT_TONEMAP_CLAMP, RT_TONEMAP_REINHARD, RT_TONEMAP_ACES = range(3)
TONEMAP_OPS = {"clamp": RT_TONEMAP_CLAMP, "reinhard": RT_TONEMAP_REINHARD, "aces": RT_TONEMAP_ACES}


class TonemapParams(C.Structure):
    """rt_tonemap_params (rt_tonemap_device, rth_tonemap)."""
    _fields_ = [("struct_size", C.c_uint32), ("op", C.c_int32), ("exposure", C.c_double), ("auto_key", C.c_double),
                ("delta", C.c_double), ("white", C.c_double)]


def _tonemap_op(v):
    if isinstance(v, str):
        if v not in TONEMAP_OPS:
            raise RtError(f"tonemap_params: no operator {v!r} (clamp, reinhard, aces)")
        return TONEMAP_OPS[v]
    return v


def tonemap_params(**kw) -> "TonemapParams":
    """rt_tonemap_params_init_sized, then the given fields (op= a number or "clamp" / "reinhard" / "aces", exposure=, auto_key=,
    delta=, white=)."""
    return _params(TonemapParams, "rt_tonemap_params_init_sized", "rt_tonemap_params", kw, convert={"op": _tonemap_op})


RT_METRICS_SUMS, RT_METRICS_MEANS = 0, 1
METRICS_FORMS = {"sums": RT_METRICS_SUMS, "means": RT_METRICS_MEANS}
FRAME_ERROR_FIELDS = ("count", "mse", "rmse", "rel_mse", "mae", "bias", "max_abs", "psnr")
FRAME_NOISE_FIELDS = ("count", "mean_var", "noise", "max_noise")


class FrameErrorParams(C.Structure):
    """rt_frame_error_params (rt_frame_error_device, rth_frame_error)."""
    _fields_ = [("struct_size", C.c_uint32), ("_pad", C.c_int32), ("eps", C.c_double), ("peak", C.c_double)]


def frame_error_params(**kw) -> "FrameErrorParams":
    """rt_frame_error_params_init_sized, then the given fields (eps=, peak=)."""
    return _params(FrameErrorParams, "rt_frame_error_params_init_sized", "rt_frame_error_params", kw)


class FrameNoiseParams(C.Structure):
    """rt_frame_noise_params (rt_frame_noise_device, rth_frame_noise)."""
    _fields_ = [("struct_size", C.c_uint32), ("_pad", C.c_int32), ("eps", C.c_double)]


def frame_noise_params(**kw) -> "FrameNoiseParams":
    """rt_frame_noise_params_init_sized, then the given fields (eps=)."""
    return _params(FrameNoiseParams, "rt_frame_noise_params_init_sized", "rt_frame_noise_params", kw)


class BloomParams(C.Structure):
    """rt_bloom_params (rt_bloom_device, rth_bloom)."""
    _fields_ = [("struct_size", C.c_uint32), ("levels", C.c_int32), ("threshold", C.c_double), ("strength", C.c_double)]


def bloom_params(**kw) -> "BloomParams":
    """rt_bloom_params_init_sized, then the given fields (levels=, threshold=, strength=)."""
    return _params(BloomParams, "rt_bloom_params_init_sized", "rt_bloom_params", kw)


RT_ROBUST_MEAN, RT_ROBUST_TRIM, RT_ROBUST_MEDIAN, RT_ROBUST_GINI = 0, 1, 2, 3
RT_ROBUST_MAX_BLOCKS = 32
ROBUST_MODES = {"mean": RT_ROBUST_MEAN, "trim": RT_ROBUST_TRIM, "median": RT_ROBUST_MEDIAN, "gini": RT_ROBUST_GINI}


class RobustParams(C.Structure):
    """rt_robust_params (rt_robust_device, rth_robust)."""
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("trim", C.c_int32), ("gain", C.c_double)]


def _robust_mode(v):
    if isinstance(v, str):
        if v not in ROBUST_MODES:
            raise RtError(f"robust_params: no mode {v!r} (mean, trim, median, gini)")
        return ROBUST_MODES[v]
    return v


def robust_params(**kw) -> "RobustParams":
    """rt_robust_params_init_sized, then the given fields (mode= an RT_ROBUST_* value or one of "mean", "trim", "median", "gini";
    trim=, gain=)."""
    return _params(RobustParams, "rt_robust_params_init_sized", "rt_robust_params", kw, convert={"mode": _robust_mode})


class UpsampleParams(C.Structure):
    """rt_upsample_params (rt_upsample_device, rth_upsample)."""
    _fields_ = [("struct_size", C.c_uint32), ("factor", C.c_int32), ("sigma_edge", C.c_double), ("sigma_albedo", C.c_double),
                ("albedo_floor", C.c_double)]


def upsample_params(**kw) -> "UpsampleParams":
    """rt_upsample_params_init_sized, then the given fields (factor=, sigma_edge=, sigma_albedo=, albedo_floor=)."""
    return _params(UpsampleParams, "rt_upsample_params_init_sized", "rt_upsample_params", kw)


class DebugNode(C.Structure):
    _fields_ = [("lo", C.c_double * 3), ("hi", C.c_double * 3), ("lo32", C.c_float * 3), ("hi32", C.c_float * 3),
                ("prim_lo", C.c_double * 3), ("prim_hi", C.c_double * 3), ("skip", C.c_uint32), ("kind", C.c_uint32),
                ("no_bbox", C.c_uint32), ("a", C.c_uint32), ("b", C.c_uint32), ("_pad", C.c_uint32)]


class RtError(RuntimeError):
    pass


# every symbol include/rt_amd.h declares: name -> (restype, argtypes)
RT_AMD_SYMBOLS = {
    "rt_device_count": (C.c_int, []),
    "rt_scene_create": (C.c_int, [C.POINTER(SceneDesc), C.c_int, C.POINTER(C.c_void_p)]),
    "rt_scene_destroy": (None, [C.c_void_p]),
    "rt_scene_get_stats": (C.c_int, [C.c_void_p, C.POINTER(SceneStats)]),
    "rt_render": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.POINTER(C.c_double)]),
    "rt_render_device": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.c_void_p, C.c_void_p]),
    "rt_render_device_counted": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.c_void_p,
                                           C.c_void_p, C.POINTER(Counters)]),
    "rt_out_size": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "rt_tiles_to_frame_device": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_resolve_rgb8_device": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_scene_options_init": (None, [C.c_void_p]),
    "rt_scene_options_init_sized": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rt_scene_create_ex": (C.c_int, [C.POINTER(SceneDesc), C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "rt_resolve_rgb8_values_device": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_tiles_to_frame_rgb8_device": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_device_malloc": (C.c_int, [C.c_int, C.c_int64, C.POINTER(C.c_void_p)]),
    "rt_device_free": (C.c_int, [C.c_int, C.c_void_p]),
    "rt_device_download": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "rt_device_upload": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "rt_comm_get_unique_id": (C.c_int, [C.c_void_p]),
    "rt_comm_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "rt_comm_create_all": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p)]),
    "rt_comm_adopt": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "rt_comm_destroy": (None, [C.c_void_p]),
    "rt_comm_rank": (C.c_int, [C.c_void_p]),
    "rt_comm_size": (C.c_int, [C.c_void_p]),
    "rt_gather_tiles_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "rt_last_error": (C.c_char_p, []),
    "rt_version": (C.c_char_p, []),
    "rt_adaptive_params_init_sized": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rt_render_pixels_device": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.c_void_p, C.c_int32,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_render_adaptive": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_render_adaptive_device": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_resolve_rgb8_spp_device": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_render_views_device": (C.c_int, [C.c_void_p, C.POINTER(View), C.c_int32, C.POINTER(RenderParams), C.c_void_p, C.c_void_p]),
    "rt_render_views": (C.c_int, [C.c_void_p, C.POINTER(View), C.c_int32, C.POINTER(RenderParams), C.c_void_p]),
    "rt_render_mean_device": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_render_mean": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.c_void_p, C.c_void_p]),
    "rt_resolve_rgba8_device": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_denoise_params_init_sized": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rt_denoise_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "rt_denoise_device": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_render_moments_device": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_render_moments": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.c_void_p, C.c_void_p]),
    "rt_albedo_materials": (C.c_int, [C.POINTER(SceneDesc), C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "rt_scene_create_albedo": (C.c_int, [C.POINTER(SceneDesc), C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "rt_denoise_albedo_params_init_sized": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rt_denoise_albedo_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "rt_denoise_albedo_device": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_surface_id_tables": (C.c_int, [C.POINTER(SceneDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_scene_create_surface_ids": (C.c_int, [C.POINTER(SceneDesc), C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "rt_denoise_guided_params_init_sized": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rt_denoise_guided_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "rt_denoise_guided_device": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                           C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_render_mean_moments_device": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p]),
    "rt_render_mean_moments": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_denoise_mean_device": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "rt_denoise_albedo_mean_device": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_denoise_spatial_params_init_sized": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rt_denoise_mean_spatial_device": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_denoise_albedo_mean_spatial_device": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_render_views_moments_device": (C.c_int, [C.c_void_p, C.POINTER(View), C.c_int32, C.POINTER(RenderParams), C.c_void_p, C.c_void_p,
                                                 C.c_void_p]),
    "rt_render_views_moments": (C.c_int, [C.c_void_p, C.POINTER(View), C.c_int32, C.POINTER(RenderParams), C.c_void_p, C.c_void_p]),
    "rt_denoise_views_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "rt_denoise_albedo_views_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "rt_denoise_views_device": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_denoise_albedo_views_device": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_denoise_guided_mean_device": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_denoise_guided_mean_spatial_device": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_denoise_guided_views_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "rt_denoise_guided_views_device": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                                 C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_robust_params_init_sized": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rt_robust_device": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_bloom_params_init_sized": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rt_bloom_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "rt_bloom_device": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_camera_scaled": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "rt_upsample_params_init_sized": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rt_upsample_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "rt_upsample_device": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_tonemap_params_init_sized": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rt_tonemap_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "rt_tonemap_device": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "rt_log_average_luminance_device": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p,
                                                  C.c_void_p]),
    "rt_film_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "rt_film_device": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_camera_cube_faces": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "rt_panorama_tables": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p]),
    "rt_panorama_device": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "rt_frame_error_params_init_sized": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rt_frame_noise_params_init_sized": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rt_metrics_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "rt_frame_error_device": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "rt_frame_noise_device": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
}

# every symbol include/rt_amd_debug.h declares (test and tuning hooks; not part of the drop-in boundary)
RT_AMD_DEBUG_SYMBOLS = {
    "rt_debug_eval": (C.c_int, [C.c_int32, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                C.POINTER(C.c_double), C.c_int]),
    "rt_debug_box_tests": (C.c_int, [C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_double,
                                     C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_int]),
    "rt_debug_quad_filter_tests": (C.c_int, [C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_double,
                                             C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_int]),
    "rt_debug_compiled_nodes": (C.c_int, [C.POINTER(SceneDesc), C.c_int32, C.POINTER(DebugNode), C.c_int64,
                                          C.POINTER(C.c_int64)]),
    "rt_debug_stage_profile": (C.c_int, [C.POINTER(C.c_uint64)]),
    "rt_debug_visit_stats": (C.c_int, [C.POINTER(C.c_uint64)]),
    "rt_debug_last_launch": (C.c_int, [C.POINTER(C.c_uint32)]),
    "rt_debug_last_kernel": (C.c_int, [C.POINTER(C.c_uint32)]),
    "rt_debug_last_start": (C.c_int, [C.POINTER(C.c_uint32)]),
    "rt_debug_adaptive_step": (C.c_int, [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double,
                                         C.c_double, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_int]),
    "rt_debug_wide_layout": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "rt_debug_wide_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_debug_wide_visits": (C.c_int, [C.c_void_p, C.c_int]),
    "rt_debug_scene_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_debug_set_traversal": (C.c_int, [C.c_int32, C.c_int32]),
    "rt_debug_set_walk_shortcuts": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "rt_debug_set_start_inline": (C.c_int, [C.c_int32]),
    "rt_debug_set_bloom_fused": (C.c_int, [C.c_int32]),
    "rt_debug_set_robust_form": (C.c_int, [C.c_int32]),
    "rt_debug_set_upsample_form": (C.c_int, [C.c_int32]),
    "rt_debug_ordered_layout": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_debug_ordered_layout_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_debug_set_tuning": (C.c_int, [C.c_int32] * 6),
}

RT_DEBUG_LOG, RT_DEBUG_SIN, RT_DEBUG_ACOS, RT_DEBUG_ATAN2, RT_DEBUG_POW5, RT_DEBUG_SQRT, RT_DEBUG_DIV, \
    RT_DEBUG_MUL_ADD, RT_DEBUG_RNG_RANDOM, RT_DEBUG_RNG_RANGE, RT_DEBUG_F32_ABOVE, RT_DEBUG_F32_BELOW, RT_DEBUG_RNG_UNNEXT = range(1, 14)
RT_DEBUG_REJECT_SPHERE_VERDICTS, RT_DEBUG_REJECT_SPHERE_COORDS, RT_DEBUG_REJECT_DISK_VERDICTS, RT_DEBUG_REJECT_DISK_COORDS = range(14, 18)


def debug_box_tests(rays, boxes, tmin, tmax, device=0):
    """rt_debug_box_tests: per (ray, box) pair: does the exact f64 test enter? the conservative f32 test of the
    reference-order walk? the packed pair test of the ordered walk (both slots must agree)?"""
    import numpy as np
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
    boxes = np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 6)
    n = rays.shape[0]
    assert boxes.shape[0] == n
    exact = np.zeros(n, dtype=np.uint8); f32 = np.zeros(n, dtype=np.uint8)
    _check(amd_lib().rt_debug_box_tests(n, rays.ctypes.data_as(C.POINTER(C.c_double)),
                                        boxes.ctypes.data_as(C.POINTER(C.c_double)), tmin, tmax,
                                        exact.ctypes.data_as(C.POINTER(C.c_uint8)), f32.ctypes.data_as(C.POINTER(C.c_uint8)),
                                        device), "rt_debug_box_tests")
    assert (((f32 >> 1) & 1) == ((f32 >> 2) & 1)).all(), "the two slots of the pair test disagree on the same box"
    return exact.astype(bool), (f32 & 1).astype(bool), ((f32 >> 1) & 1).astype(bool)


def debug_quad_filter_tests(rays, quads, tmin, tmax, device=0):
    """rt_debug_quad_filter_tests: per (ray, quad = Q, u, v) pair: does the exact f64 Quad::hit accept within [tmin, tmax]? does the
    quad stage's conservative f32 filter keep the quad (both slots of the pair record must agree)?  does it claim alpha and beta are
    certainly inside [0, 1] — and are they, where the exact test evaluates them?"""
    import numpy as np
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
    quads = np.ascontiguousarray(quads, dtype=np.float64).reshape(-1, 9)
    n = rays.shape[0]
    assert quads.shape[0] == n
    exact = np.zeros(n, dtype=np.uint8); keep = np.zeros(n, dtype=np.uint8)
    _check(amd_lib().rt_debug_quad_filter_tests(n, rays.ctypes.data_as(C.POINTER(C.c_double)), quads.ctypes.data_as(C.POINTER(C.c_double)),
                                                tmin, tmax, exact.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                keep.ctypes.data_as(C.POINTER(C.c_uint8)), device), "rt_debug_quad_filter_tests")
    assert ((keep & 1) == ((keep >> 1) & 1)).all() and ((keep >> 2 & 1) == (keep >> 3 & 1)).all(), "the two slots of the pair record disagree on the same quad"
    # exact verdict | the filter keeps the quad | the filter says alpha, beta are certainly inside | the exact alpha, beta are inside
    # (True where the exact test did not get that far)
    return exact.astype(bool), (keep & 1).astype(bool), (keep >> 2 & 1).astype(bool), (keep >> 4 & 1).astype(bool)


def debug_compiled_nodes(host_scene, refit=True):
    """rt_debug_compiled_nodes: the records the device walks for this scene (runs on the CPU)."""
    n = C.c_int64()
    _check(amd_lib().rt_debug_compiled_nodes(C.byref(host_scene.desc), 1 if refit else 0, None, 0, C.byref(n)),
           "rt_debug_compiled_nodes")
    buf = (DebugNode * n.value)()
    _check(amd_lib().rt_debug_compiled_nodes(C.byref(host_scene.desc), 1 if refit else 0, buf, n.value, C.byref(n)),
           "rt_debug_compiled_nodes")
    return buf


class DebugOrdered(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("cap_nodes", "cap_spheres", "cap_quads", "cap_instances", "cap_steps", "cap_media",
                                         "n_nodes", "n_spheres", "n_quads", "n_instances", "n_steps", "n_media")] + \
               [(n, C.c_uint32) for n in ("ordered", "root", "stack_entries", "_pad")] + \
               [("nodes", C.c_void_p), ("spheres", C.c_void_p), ("quads", C.c_void_p), ("instances", C.c_void_p),
                ("steps", C.c_void_p), ("media", C.c_void_p)]


def debug_ordered_layout(host_scene, **option_fields) -> dict:
    """rt_debug_ordered_layout_ex: the scene compiler's ordered layout (numpy arrays), no device needed; leaf_max= / flat_max= as
    rt_scene_options has them."""
    import numpy as np
    io = DebugOrdered()
    opts = scene_options(**option_fields) if option_fields else None
    call = lambda: amd_lib().rt_debug_ordered_layout_ex(C.addressof(host_scene.desc), C.addressof(opts) if opts is not None else None, C.addressof(io))
    _check(call(), "rt_debug_ordered_layout")
    nodes = np.zeros((max(io.n_nodes, 1), 16), dtype=np.uint32)
    spheres = np.zeros((max(io.n_spheres, 1), 9)); quads = np.zeros((max(io.n_quads, 1), 10))
    insts = np.zeros((max(io.n_instances, 1), 8))
    steps = np.zeros((max(io.n_steps, 1), 28), dtype=np.uint32); media = np.zeros(max(io.n_media, 1), dtype=np.uint32)
    io.cap_nodes, io.cap_spheres, io.cap_quads, io.cap_instances = len(nodes), len(spheres), len(quads), len(insts)
    io.cap_steps, io.cap_media = len(steps), len(media)
    io.nodes, io.spheres, io.quads, io.instances = (a.ctypes.data for a in (nodes, spheres, quads, insts))
    io.steps, io.media = steps.ctypes.data, media.ctypes.data
    _check(call(), "rt_debug_ordered_layout")
    return {"ordered": bool(io.ordered), "root": int(io.root), "stack_entries": int(io.stack_entries),
            "nodes": nodes[:io.n_nodes], "spheres": spheres[:io.n_spheres], "quads": quads[:io.n_quads],
            "instances": insts[:io.n_instances], "steps": steps[:io.n_steps], "media": media[:io.n_media]}


def debug_wide_layout(host_scene, **option_fields) -> dict:
    """rt_debug_wide_layout: structure check of the four-child layout (CPU)."""
    buf = (C.c_uint64 * 6)()
    opts = scene_options(**option_fields) if option_fields else None
    _check(amd_lib().rt_debug_wide_layout(C.addressof(host_scene.desc), C.addressof(opts) if opts is not None else None, buf), "rt_debug_wide_layout")
    return dict(zip(("records", "found", "primitives", "stack_entries", "violations", "deepest"), (int(x) for x in buf)))


class DebugWide(C.Structure):
    _fields_ = [("cap_records", C.c_int64), ("cap_steps", C.c_int64), ("n_records", C.c_int64), ("n_steps", C.c_int64),
                ("wide", C.c_uint32), ("table_bytes", C.c_uint32), ("box_extent", C.c_float), ("_pad", C.c_uint32),
                ("boxes", C.c_void_p), ("refs", C.c_void_p), ("bounds", C.c_void_p), ("global_image", C.c_void_p),
                ("lds_image", C.c_void_p), ("step_boxes", C.c_void_p)]


class DebugPlanLevel(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("lds_level", "features", "threads", "aux_in_lds", "world_in_lds", "stack_off", "seq_off", "aux_off",
                                          "world_off", "prof_off", "dynamic_lds_bytes", "dynamic_lds_bytes_counted")]


class DebugPlanBytes(C.Structure):
    _fields_ = [("bytes", C.c_uint64), ("digest", C.c_uint64)]


PLAN_IMAGES = ("oimage", "lds_image", "aux_image", "mats")  # what scene creation builds; then the tables it uploads as they are
PLAN_TABLES = ("nodes", "oseq", "spheres", "quads", "insts", "media", "texs", "perlins", "images", "texels", "lut")
PLAN_SCALARS = ("features", "parks_colours", "has_instances", "ordered", "wide", "o_root", "n_oseq", "o_stack", "n_nodes", "o_start_stage",
                "o_start_prim", "o_start_end", "o_start_rest", "o_start_slot", "o_start_direct", "box_extent", "lds_level", "lds_off_node_b",
                "lds_off_spheres", "lds_off_quads", "lds_off_qfilt", "lds_prefix_bytes", "aux_bytes", "aux_off")


class DebugPlan(C.Structure):
    _fields_ = [("cap_" + n, C.c_int64) for n in PLAN_IMAGES + ("insts",)] + [(n, C.c_void_p) for n in PLAN_IMAGES + ("insts",)] + \
               [(n, C.c_uint32) for n in PLAN_SCALARS[:15]] + [("box_extent", C.c_float)] + [(n, C.c_uint32) for n in PLAN_SCALARS[16:21]] + \
               [("lds_prefix_bytes", C.c_uint32 * 4), ("aux_bytes", C.c_uint32), ("aux_off", C.c_uint32 * 5), ("stats", SceneStats),
                ("level", DebugPlanLevel * 2), ("image_bytes", DebugPlanBytes * 4), ("table_bytes", DebugPlanBytes * 11)]


class DebugWideCases(C.Structure):
    _fields_ = [("n", C.c_int64), ("rays", C.c_void_p), ("tmin", C.c_void_p), ("tmax", C.c_void_p), ("todo", C.c_void_p),
                ("boxes", C.c_void_p), ("refs", C.c_void_p), ("global_image", C.c_void_p), ("lds_image", C.c_void_p),
                ("n_records", C.c_int64), ("record", C.c_void_p), ("extent", C.c_float), ("lds", C.c_int32),
                ("enter", C.c_void_p), ("leave", C.c_void_p), ("hit", C.c_void_p), ("chosen", C.c_void_p),
                ("degenerate", C.c_void_p), ("exact", C.c_void_p)]


def debug_wide_records(host_scene, **option_fields) -> dict:
    """rt_debug_wide_records: the four-child records of the scene as the device sees them (numpy arrays; CPU only).  boxes (n, 4, 3, 2)
    f32 and bounds (n, 4, 3, 2) f64 = [record, slot, axis, lo / hi]; refs (n, 4); the two packed images as bytes; the sequence's boxes."""
    import numpy as np
    io = DebugWide()
    opts = scene_options(**option_fields) if option_fields else None
    call = lambda: amd_lib().rt_debug_wide_records(C.addressof(host_scene.desc), C.addressof(opts) if opts is not None else None, C.addressof(io))
    _check(call(), "rt_debug_wide_records")
    n, ns = int(io.n_records), int(io.n_steps)
    boxes = np.zeros((max(n, 1), 4, 3, 2), dtype=np.float32); refs = np.zeros((max(n, 1), 4), dtype=np.uint32)
    bounds = np.zeros((max(n, 1), 4, 3, 2)); glob = np.zeros((max(n, 1), 256), dtype=np.uint8); lds = np.zeros(max(n, 1) * 208, dtype=np.uint8)
    steps = np.zeros((max(ns, 1), 3, 2), dtype=np.float32)
    io.cap_records, io.cap_steps = max(n, 1), max(ns, 1)
    io.boxes, io.refs, io.bounds, io.global_image, io.lds_image, io.step_boxes = (a.ctypes.data for a in (boxes, refs, bounds, glob, lds, steps))
    _check(call(), "rt_debug_wide_records")
    assert (int(io.n_records), int(io.n_steps)) == (n, ns)
    return {"wide": bool(io.wide), "box_extent": float(io.box_extent), "table_bytes": int(io.table_bytes), "boxes": boxes[:n], "refs": refs[:n],
            "bounds": bounds[:n], "global_image": glob[:n], "lds_image": lds[:n * 208], "step_boxes": steps[:ns]}


def debug_scene_plan(host_scene, options: "SceneCreateOptions | None" = None, **option_fields) -> dict:
    """rt_debug_scene_plan: what rt_scene_create_ex would decide and upload for this scene under these options (CPU only).  The layout's
    scalars by name (box_extent a float, lds_prefix_bytes and aux_off lists); "stats" as DeviceScene.stats(); "levels": {0: ...,
    lds_level: ...}, a launch at either LDS level; "sizes" and "digests" (64-bit FNV-1a) of the four images and the eleven tables by name
    (PLAN_IMAGES, PLAN_TABLES); the four images and the instance table as uint8 arrays."""
    import numpy as np
    io = DebugPlan()
    if option_fields:
        assert options is None
        options = scene_options(**option_fields)
    call = lambda: amd_lib().rt_debug_scene_plan(C.addressof(host_scene.desc), C.addressof(options) if options is not None else None, C.addressof(io))
    _check(call(), "rt_debug_scene_plan")
    sized = dict(zip(PLAN_IMAGES, (int(b.bytes) for b in io.image_bytes)), insts=int(io.table_bytes[PLAN_TABLES.index("insts")].bytes))
    bufs = {n: np.zeros(max(size, 1), dtype=np.uint8) for n, size in sized.items()}
    for n, a in bufs.items():
        setattr(io, "cap_" + n, a.size)
        setattr(io, n, a.ctypes.data)
    _check(call(), "rt_debug_scene_plan")
    out = {n: (list(getattr(io, n)) if n in ("lds_prefix_bytes", "aux_off") else float(io.box_extent) if n == "box_extent" else int(getattr(io, n)))
           for n in PLAN_SCALARS}
    out["stats"] = io.stats.as_dict()
    out["levels"] = {int(v.lds_level): {n: int(getattr(v, n)) for n, _ in DebugPlanLevel._fields_} for v in io.level}
    named = list(zip(PLAN_IMAGES, io.image_bytes)) + list(zip(PLAN_TABLES, io.table_bytes))
    out["sizes"] = {n: int(b.bytes) for n, b in named}
    out["digests"] = {n: f"{int(b.digest):016x}" for n, b in named}
    out.update({n: a[:sized[n]] for n, a in bufs.items()})
    return out


def debug_wide_visits(rays, tmin, tmax, todo, boxes=None, refs=None, records=None, record=None, extent=0.0, lds=0, device=0) -> dict:
    """rt_debug_wide_visits: one visit of a four-child record per case, as the render kernels make it.  Either boxes (n, 4, 3, 2) f64
    (+ refs (n, 4)), or records = what debug_wide_records returned and record (n,) = the record each case visits.  Returns enter,
    leave (n, 4) f32; hit, exact (n, 4) bool; chosen (n,) int8 (-1: none); degenerate (n,) bool."""
    import numpy as np
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
    n = rays.shape[0]
    tmin = np.ascontiguousarray(np.broadcast_to(np.asarray(tmin, dtype=np.float64), (n,)))
    tmax = np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, dtype=np.float64), (n,)))
    todo = np.ascontiguousarray(np.broadcast_to(np.asarray(todo, dtype=np.uint8), (n,)))
    io = DebugWideCases(n=n, rays=rays.ctypes.data, tmin=tmin.ctypes.data, tmax=tmax.ctypes.data, todo=todo.ctypes.data, extent=extent, lds=lds)
    keep = []
    if boxes is not None:
        boxes = np.ascontiguousarray(boxes, dtype=np.float64).reshape(n, 24)
        io.boxes = boxes.ctypes.data
        if refs is not None:
            refs = np.ascontiguousarray(refs, dtype=np.uint32).reshape(n, 4)
            io.refs = refs.ctypes.data
    else:
        glob = np.ascontiguousarray(records["global_image"], dtype=np.uint8); ldsi = np.ascontiguousarray(records["lds_image"], dtype=np.uint8)
        record = np.ascontiguousarray(record, dtype=np.uint32).reshape(n)
        assert ldsi.size == glob.shape[0] * 208
        io.global_image, io.lds_image, io.n_records, io.record = glob.ctypes.data, ldsi.ctypes.data, glob.shape[0], record.ctypes.data
        keep += [glob, ldsi]
    enter = np.zeros((n, 4), dtype=np.float32); leave = np.zeros((n, 4), dtype=np.float32)
    hit = np.zeros(n, dtype=np.uint8); chosen = np.zeros(n, dtype=np.int8); deg = np.zeros(n, dtype=np.uint8); exact = np.zeros(n, dtype=np.uint8)
    io.enter, io.leave, io.hit, io.chosen, io.degenerate, io.exact = (a.ctypes.data for a in (enter, leave, hit, chosen, deg, exact))
    _check(amd_lib().rt_debug_wide_visits(C.addressof(io), device), "rt_debug_wide_visits")
    bits = lambda m: ((m[:, None] >> np.arange(4, dtype=np.uint8)) & 1).astype(bool)
    return {"enter": enter, "leave": leave, "hit": bits(hit), "chosen": chosen, "degenerate": deg.astype(bool), "exact": bits(exact)}


def debug_last_launch() -> dict:
    """rt_debug_last_launch: how this thread's last render was launched (render-kernel launches, LDS level, workgroup threads,
    workgroups)."""
    buf = (C.c_uint32 * 4)()
    _check(amd_lib().rt_debug_last_launch(buf), "rt_debug_last_launch")
    return {"launches": int(buf[0]), "lds_level": int(buf[1]), "threads": int(buf[2]), "grid": int(buf[3])}


# the render kernels' feature masks (rt_kernels.h) and job modes, as rt_debug_last_kernel reports them
RT_FEAT_SPHERES_SOLID, RT_FEAT_QUADS_FRAMES, RT_FEAT_QUADS_FRAMES_MEDIA, RT_FEAT_SPHERES_QUADS_TEXTURES, RT_FEAT_ALL = 1, 6, 14, 19, 31
RT_JOBS_DENSE, RT_JOBS_LIST, RT_JOBS_VIEWS = 0, 1, 2


def debug_last_kernel() -> dict:
    """rt_debug_last_kernel: which render kernel this thread's last render ran (feature mask, LDS level, own trees?, four-child
    records?, small tables in the LDS?, job mode, ids_ok, workgroup threads)."""
    buf = (C.c_uint32 * 8)()
    _check(amd_lib().rt_debug_last_kernel(buf), "rt_debug_last_kernel")
    return dict(zip(("features", "lds_level", "ordered", "wide", "aux", "jobs", "ids_ok", "threads"), (int(x) for x in buf)))


def debug_last_start() -> dict:
    """rt_debug_last_start: how the queries of this thread's last render started (the start shortcut's stage, its leaf's primitives
    [first, end), whether the launch asked for the inline start test) and `ran_inline`: whether the kernel it ran has that test."""
    buf = (C.c_uint32 * 4)()
    _check(amd_lib().rt_debug_last_start(buf), "rt_debug_last_start")
    k = debug_last_kernel()
    out = dict(zip(("stage", "first", "end", "start_inline"), (int(x) for x in buf)))
    out["ran_inline"] = int(out["start_inline"] == 1 and k["features"] == RT_FEAT_SPHERES_SOLID and k["ordered"] == 1)
    return out


def debug_adaptive_step(pixels, sums, sums_sq, n, rel, abs, *, last=False, spp=None, list_out=None, device=0):
    """rt_debug_adaptive_step: one convergence step over `pixels` (uint32, a multiple of 64 entries) on chosen sums (n_pixels x 3).
    `spp` (int32, n_pixels) and `list_out` (uint32, as long as the list) are the caller's pre-filled arrays (default: -1 / zeros);
    returns (survivor count, list_out, spp) — copies, the arguments are not written."""
    import numpy as np
    pixels = np.ascontiguousarray(pixels, dtype=np.uint32)
    sums = np.ascontiguousarray(sums, dtype=np.float64).reshape(-1, 3)
    sums_sq = np.ascontiguousarray(sums_sq, dtype=np.float64).reshape(-1, 3)
    n_pixels = sums.shape[0]
    assert sums_sq.shape[0] == n_pixels
    spp = np.full(n_pixels, -1, dtype=np.int32) if spp is None else np.array(spp, dtype=np.int32)
    list_out = np.zeros(pixels.size, dtype=np.uint32) if list_out is None else np.array(list_out, dtype=np.uint32)
    assert spp.size == n_pixels and list_out.size == pixels.size
    count = C.c_uint32(0)
    _check(amd_lib().rt_debug_adaptive_step(pixels.size, C.c_void_p(pixels.ctypes.data), n_pixels, C.c_void_p(sums.ctypes.data),
                                            C.c_void_p(sums_sq.ctypes.data), int(n), 1 if last else 0, float(rel), float(abs),
                                            C.c_void_p(spp.ctypes.data), C.c_void_p(list_out.ctypes.data), C.byref(count), device),
           "rt_debug_adaptive_step")
    return int(count.value), list_out, spp


def debug_stage_profile() -> dict:
    """rt_debug_stage_profile: per stage {rounds, lanes (mean active per round), cycles} of the last counted render."""
    buf = (C.c_uint64 * 36)()
    _check(amd_lib().rt_debug_stage_profile(buf), "rt_debug_stage_profile")
    out = {}
    for i, name in enumerate(("box", "sphere", "quad", "other", "shade", "newjob", "shade.rebuild", "shade.sample", "shade.texture",
                              "shade.material", "end.products", "end.newjob")):
        rounds, lanes, cycles = int(buf[3 * i]), int(buf[3 * i + 1]), int(buf[3 * i + 2])
        out[name] = {"rounds": rounds, "mean_active_lanes": lanes / rounds if rounds else 0.0, "cycles": cycles}
    return out


def debug_visit_stats() -> dict:
    """rt_debug_visit_stats: the last counted render's visits of four-child records — first visits, revisits of a record set aside
    with b = 1..3 children left by what the walk went on with (inner record / leaf or instance / nothing), and the two kinds of entry
    set aside."""
    buf = (C.c_uint64 * 12)()
    _check(amd_lib().rt_debug_visit_stats(buf), "rt_debug_visit_stats")
    out = {"first": int(buf[0])}
    for b in (1, 2, 3):
        for o, name in enumerate(("inner", "leaf", "none")):
            out[f"revisit{b}.{name}"] = int(buf[1 + 3 * (b - 1) + o])
    out["push.record"] = int(buf[10])
    out["push.child"] = int(buf[11])
    return out


def debug_eval(op, a, b=None, device=0):
    """rt_debug_eval: one device-side scalar function over arrays (test hook)."""
    import numpy as np
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = np.empty_like(a)
    bp = None
    if b is not None:
        b = np.ascontiguousarray(b, dtype=np.float64)
        assert b.shape == a.shape
        bp = b.ctypes.data_as(C.POINTER(C.c_double))
    _check(amd_lib().rt_debug_eval(op, a.size, a.ctypes.data_as(C.POINTER(C.c_double)), bp,
                                   out.ctypes.data_as(C.POINTER(C.c_double)), device), "rt_debug_eval")
    return out

# every symbol include/rt_host.h declares
RT_HOST_SYMBOLS = {
    "rth_scene_build": (C.c_int, [C.POINTER(SceneOptions), C.POINTER(C.c_void_p)]),
    "rth_scene_destroy": (None, [C.c_void_p]),
    "rth_scene_desc": (C.POINTER(SceneDesc), [C.c_void_p]),
    "rth_scene_camera": (C.POINTER(Camera), [C.c_void_p]),
    "rth_scene_camera_look": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(Camera)]),
    "rth_scene_look": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "rth_scene_orbit_look_from": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_double)]),
    "rth_resolve_rgb8": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_uint8)]),
    "rth_tonemap": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rth_log_average_luminance": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.c_void_p]),
    "rth_film": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "rth_bloom": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rth_upsample": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                               C.c_void_p]),
    "rth_robust": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rth_panorama": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "rth_frame_error": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "rth_frame_noise": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rth_read_pfm": (C.c_int, [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_int64]),
    "rth_write_png": (C.c_int, [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_uint8)]),
    "rth_write_hdr": (C.c_int, [C.c_char_p, C.c_int32, C.c_int32, C.c_void_p]),
    "rth_write_pfm": (C.c_int, [C.c_char_p, C.c_int32, C.c_int32, C.c_void_p]),
    "rth_write_png16": (C.c_int, [C.c_char_p, C.c_int32, C.c_int32, C.c_void_p]),
    "rth_synthetic_earth": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_uint8)]),
    "rth_load_image": (C.c_int, [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint8),
                                 C.c_int64]),
    "rth_last_error": (C.c_char_p, []),
}


def _bind(lib, table):
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        fn.restype = restype
        fn.argtypes = argtypes
    return lib


_host_lib = None
_amd_lib = None


def host_lib():
    """librt_host.so (CPU only)."""
    global _host_lib
    if _host_lib is None:
        path = LIB_DIR / "librt_host.so"
        if not path.exists():
            raise RtError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        _host_lib = _bind(C.CDLL(str(path)), RT_HOST_SYMBOLS)
    return _host_lib


def amd_lib():
    """librt_amd.so (HIP).  Loading works without a GPU; rendering does not."""
    global _amd_lib
    if _amd_lib is None:
        path = Path(os.environ.get("RT_AMD_LIB", LIB_DIR / "librt_amd.so"))  # RT_AMD_LIB: tuning builds only
        if not path.exists():
            raise RtError(f"{path} is missing: the HIP renderer is not built and there is no fallback; "
                          "run `python -c 'import __graft_entry__ as g; g.build()'`")
        _amd_lib = _bind(_bind(C.CDLL(str(path), mode=C.RTLD_GLOBAL), RT_AMD_SYMBOLS), RT_AMD_DEBUG_SYMBOLS)
    return _amd_lib


def _check(rc, where):
    if rc != 0:
        raise RtError(f"{where} failed ({rc}): {amd_lib().rt_last_error().decode(errors='replace')}")


class HostScene:
    """A scene built by the host library: the reference's `main` up to the call of render()
    (scene function -> BVHNode::new -> Camera), described as rt_scene_desc + rt_camera."""

    def __init__(self, scene: int, *, scene_seed: int = 1, width: int = 0, aspect: float = 0.0, spp: int = 0,
                 depth: int = 0, earth_image: str | None = None, bvh: str = "reference"):
        lib = host_lib()
        self._earth = earth_image.encode() if earth_image else None
        opts = SceneOptions(scene=scene, bvh_policy=1 if bvh == "sah" else 0, scene_seed=scene_seed,
                            image_width=width, aspect_ratio=aspect, samples_per_pixel=spp, max_depth=depth,
                            earth_image=self._earth)
        handle = C.c_void_p()
        if lib.rth_scene_build(C.byref(opts), C.byref(handle)) != 0:
            raise RtError(lib.rth_last_error().decode(errors="replace"))
        self._handle = handle
        self.desc = lib.rth_scene_desc(handle).contents
        self.camera = lib.rth_scene_camera(handle).contents
        # the records live in the C object: keep it alive for as long as either view is referenced
        self.desc._owner = self
        self.camera._owner = self

    @property
    def width(self):
        return self.camera.image_width

    @property
    def height(self):
        return self.camera.image_height

    def close(self):
        if getattr(self, "_handle", None):
            host_lib().rth_scene_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def camera_look(host_scene: HostScene, look_from=None, look_at=None) -> Camera:
    """rth_scene_camera_look: the scene's camera with look_from and / or look_at replaced (None: the scene's own)."""
    def vec(v):
        return None if v is None else (C.c_double * 3)(*[float(x) for x in v])
    cam = Camera()
    lib = host_lib()
    if lib.rth_scene_camera_look(host_scene._handle, vec(look_from), vec(look_at), C.byref(cam)) != 0:
        raise RtError(lib.rth_last_error().decode(errors="replace"))
    return cam


def scene_look(host_scene: HostScene):
    """rth_scene_look: the scene's own (look_from, look_at, vup), each a tuple of three floats."""
    f, a, u = (C.c_double * 3)(), (C.c_double * 3)(), (C.c_double * 3)()
    lib = host_lib()
    if lib.rth_scene_look(host_scene._handle, f, a, u) != 0:
        raise RtError(lib.rth_last_error().decode(errors="replace"))
    return tuple(f), tuple(a), tuple(u)


def orbit_look_from(host_scene: HostScene, k: int, n: int):
    """rth_scene_orbit_look_from: the scene's look_from turned about the axis through look_at along vup by 360 k / n degrees (what
    `rtrace --orbit n` gives view k)."""
    out = (C.c_double * 3)()
    lib = host_lib()
    if lib.rth_scene_orbit_look_from(host_scene._handle, k, n, out) != 0:
        raise RtError(lib.rth_last_error().decode(errors="replace"))
    return tuple(out)


def orbit_views(host_scene: HostScene, n: int, seed: int = 1, of: "int | None" = None):
    """The n views of `rtrace --orbit n --seed seed`: a ctypes array of View, view k with seed + k.  With `of` > n they are the
    first n of an `of`-view orbit, steps of 360 / of degrees: an arc, for a scene that is open to one side only."""
    views = (View * n)()
    for k in range(n):
        views[k].camera = camera_look(host_scene, orbit_look_from(host_scene, k, n if of is None else of))
        views[k].seed = seed + k
    return views


def _view_array(views):
    if isinstance(views, C.Array) and views._type_ is View:
        return views
    arr = (View * len(views))()
    for k, v in enumerate(views):
        if isinstance(v, View):
            arr[k] = v
        else:  # (camera, seed)
            arr[k].camera, arr[k].seed = v[0], v[1]
    return arr


def render_params(*, seed=1, sample_begin=0, sample_end=0, max_depth=0, accumulate=False, shard_index=0,
                  shard_count=1, out_layout=RT_OUT_FRAME, device=0) -> RenderParams:
    return RenderParams(seed=seed, sample_begin=sample_begin, sample_end=sample_end, max_depth=max_depth,
                        accumulate=1 if accumulate else 0, shard_index=shard_index, shard_count=shard_count,
                        out_layout=out_layout, device=device)


def out_size(width, height, out_layout=RT_OUT_FRAME, shard_index=0, shard_count=1) -> int:
    n = int(amd_lib().rt_out_size(width, height, out_layout, shard_index, shard_count))
    if n < 0:
        raise RtError(f"rt_out_size: invalid arguments (size {width}x{height}, layout {out_layout}, "
                      f"shard {shard_index} of {shard_count})")
    return n


def _frame_arg(who, name, a, shape):
    """a caller's array that a host-buffer render writes in place: float64, C-contiguous, writable and of this shape"""
    import numpy as np
    if a is None or a.shape != shape or a.dtype != np.float64 or not a.flags["C_CONTIGUOUS"] or not a.flags["WRITEABLE"]:
        raise RtError(f"{who}: `{name}` must be a writable C-contiguous float64 array of shape {shape}")


class DeviceScene:
    """rt_scene handle: the compiled scene resident in one GPU's HBM."""

    def __init__(self, host_scene: HostScene, device: int = 0, options: "SceneCreateOptions | None" = None, albedo: bool = False,
                 surface_ids: bool = False, **option_fields):
        """albedo=True: rt_scene_create_albedo, the scene whose render is the first-hit albedo frame (render it with
        albedo_camera(camera): a miss then contributes (1, 1, 1)).  surface_ids=True: rt_scene_create_surface_ids, the scene whose
        render is the first-hit surface-ID frame (render it with surface_id_camera(camera): a miss then contributes (0, 0, 0))."""
        lib = amd_lib()
        self.host_scene = host_scene  # keeps desc memory alive during create
        self.device = device
        self.albedo = bool(albedo)
        self.surface_ids = bool(surface_ids)
        if albedo and surface_ids:
            raise RtError("DeviceScene: albedo and surface_ids are two scenes of a description: give one of them")
        handle = C.c_void_p()
        if option_fields:
            assert options is None
            options = scene_options(**option_fields)
        if surface_ids:
            _check(lib.rt_scene_create_surface_ids(C.byref(host_scene.desc), device, C.byref(options) if options is not None else None,
                                                   C.byref(handle)), "rt_scene_create_surface_ids")
        elif albedo:
            _check(lib.rt_scene_create_albedo(C.byref(host_scene.desc), device, C.byref(options) if options is not None else None,
                                              C.byref(handle)), "rt_scene_create_albedo")
        elif options is None:
            _check(lib.rt_scene_create(C.byref(host_scene.desc), device, C.byref(handle)), "rt_scene_create")
        else:
            _check(lib.rt_scene_create_ex(C.byref(host_scene.desc), device, C.byref(options), C.byref(handle)), "rt_scene_create_ex")
        self._handle = handle

    def stats(self) -> dict:
        st = SceneStats()
        _check(amd_lib().rt_scene_get_stats(self._handle, C.byref(st)), "rt_scene_get_stats")
        return st.as_dict()

    def render(self, params: RenderParams, camera: Camera | None = None, out=None):
        """rt_render: host buffer out (numpy float64, flat: out_size(...) values).  `out`: the array to write (with params.accumulate:
        the running sums this call adds to, so it is required then); returned."""
        import numpy as np
        cam = camera if camera is not None else self.host_scene.camera
        n = out_size(cam.image_width, cam.image_height, params.out_layout, params.shard_index, params.shard_count)
        if out is None:
            if params.accumulate:
                raise RtError("render: params.accumulate adds to running sums: pass them as `out`")
            out = np.zeros(n, dtype=np.float64)
        _frame_arg("render", "out", out, (n,))
        _check(amd_lib().rt_render(self._handle, C.byref(cam), C.byref(params),
                                   out.ctypes.data_as(C.POINTER(C.c_double))), "rt_render")
        return out

    def render_device(self, params: RenderParams, d_out_ptr: int, stream: int = 0, camera: Camera | None = None):
        """rt_render_device: `d_out_ptr` is a device pointer (e.g. torch tensor .data_ptr()), `stream` a hipStream_t."""
        cam = camera if camera is not None else self.host_scene.camera
        _check(amd_lib().rt_render_device(self._handle, C.byref(cam), C.byref(params), C.c_void_p(d_out_ptr),
                                          C.c_void_p(stream)), "rt_render_device")

    def render_device_counted(self, params: RenderParams, d_out_ptr: int, stream: int = 0,
                              camera: Camera | None = None) -> dict:
        cam = camera if camera is not None else self.host_scene.camera
        cnt = Counters()
        _check(amd_lib().rt_render_device_counted(self._handle, C.byref(cam), C.byref(params),
                                                  C.c_void_p(d_out_ptr), C.c_void_p(stream), C.byref(cnt)),
               "rt_render_device_counted")
        return cnt.as_dict()

    def render_views(self, params: RenderParams, views, out=None):
        """rt_render_views: every view's frame from one launch, as an (n_views, h, w, 3) float64 array.  `views`: View records (or
        (camera, seed) pairs); view v equals render() under that camera with seed = that seed (params.seed is ignored).  `out`: the
        array to write (with params.accumulate: the running sums this call adds to, so it is required then); returned."""
        import numpy as np
        arr = _view_array(views)
        n = len(arr)
        h, w = (arr[0].camera.image_height, arr[0].camera.image_width) if n else (0, 0)
        if out is None:
            if params.accumulate:
                raise RtError("render_views: params.accumulate adds to running sums: pass them as `out`")
            out = np.zeros((n, h, w, 3), dtype=np.float64)
        _frame_arg("render_views", "out", out, (n, h, w, 3))
        _check(amd_lib().rt_render_views(self._handle, arr, n, C.byref(params), C.c_void_p(out.ctypes.data)), "rt_render_views")
        return out

    def render_views_device(self, params: RenderParams, views, d_out_ptr: int, stream: int = 0):
        """rt_render_views_device: `d_out_ptr` is device memory for n_views frames of 3 w h doubles, view-major; enqueued on
        `stream` without synchronising (the view records are copied during the call)."""
        arr = _view_array(views)
        _check(amd_lib().rt_render_views_device(self._handle, arr, len(arr), C.byref(params), C.c_void_p(d_out_ptr),
                                                C.c_void_p(stream)), "rt_render_views_device")

    def render_robust(self, params: RenderParams, blocks: int, camera: Camera | None = None, **robust_kw):
        """A firefly-robust frame: `blocks` sub-frames of this camera under the seeds params.seed + k, each of the samples
        [0, spp / blocks) — spp is params.sample_end or, if that is 0, the camera's samples_per_pixel, and `blocks` must divide it —
        from ONE rt_render_views_device launch, combined on the device by rt_robust_device with robust_params(**robust_kw).  Returns
        (mean, m2), two (h, w, 3) float64 frames: with samples = blocks they are what denoise_mean takes."""
        import torch
        cam = camera if camera is not None else self.host_scene.camera
        spp = params.sample_end if params.sample_end > 0 else cam.samples_per_pixel
        if not 1 <= blocks <= RT_ROBUST_MAX_BLOCKS:
            raise RtError(f"render_robust: blocks must be from 1 to {RT_ROBUST_MAX_BLOCKS}")
        if params.sample_begin != 0 or params.accumulate:
            raise RtError("render_robust: the sub-frames start at sample 0 and are not accumulated")
        if spp % blocks != 0:
            raise RtError(f"render_robust: blocks = {blocks} does not divide the sample count {spp}")
        rp = robust_params(**robust_kw)
        sub = RenderParams.from_buffer_copy(params)
        sub.sample_end = spp // blocks
        h, w = cam.image_height, cam.image_width
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream().cuda_stream
            d_stack = torch.empty((blocks, h, w, 3), dtype=torch.float64, device="cuda")
            d_out = torch.empty((2, h, w, 3), dtype=torch.float64, device="cuda")
            self.render_views_device(sub, [(cam, params.seed + k) for k in range(blocks)], d_stack.data_ptr(), stream)
            robust_device(w, h, blocks, d_stack.data_ptr(), sub.sample_end, d_out[0].data_ptr(), d_m2_out_ptr=d_out[1].data_ptr(), params=rp,
                          stream=stream)
            torch.cuda.synchronize()
            out = d_out.cpu().numpy()
        return out[0], out[1]

    def panorama_views(self, face_size: int, guard: int = 1, center=None, seed: int = 1):
        """The six views render_panorama launches: the cube-face cameras about `center` (None: the scene camera's centre), face f with
        seed + f."""
        cams = cube_face_cameras(self.host_scene.camera, center, face_size, guard)
        return _view_array([(cams[f], seed + f) for f in range(6)])

    def render_panorama(self, width: int, height: "int | None" = None, center=None, face_size: "int | None" = None, guard: int = 1,
                        spp: "int | None" = None, seed: int = 1):
        """A full 360 x 180 degree equirectangular frame of the scene seen from `center` (None: the scene camera's centre): the six
        cube faces (face_size pixels wide, default width // 4 + 2 * guard — the cube's texel density at the equator) under seeds
        seed + f from ONE rt_render_views_device launch of `spp` samples (None: the camera's samples_per_pixel), resampled on the device
        by rt_panorama_device.  `height` defaults to width // 2.  Returns the (height, width, 3) float64 frame of means: what bloom,
        tonemap and film take with spp = 1."""
        import torch
        height = width // 2 if height is None else height
        face_size = width // 4 + 2 * guard if face_size is None else face_size
        views = self.panorama_views(face_size, guard, center, seed)
        n = spp if spp is not None else self.host_scene.camera.samples_per_pixel
        tables = panorama_tables(width, height)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream().cuda_stream
            d_tables = torch.from_numpy(tables).cuda()
            d_faces = torch.empty((6, face_size, face_size, 3), dtype=torch.float64, device="cuda")
            d_out = torch.empty((height, width, 3), dtype=torch.float64, device="cuda")
            self.render_views_device(render_params(sample_end=n), views, d_faces.data_ptr(), stream)
            panorama_device(width, height, d_tables.data_ptr(), d_faces.data_ptr(), face_size, guard, n, d_out.data_ptr(), stream=stream)
            torch.cuda.synchronize()
            return d_out.cpu().numpy()

    def render_views_moments(self, params: RenderParams, views, sum=None, sum_sq=None):
        """rt_render_views_moments: (sum, sum_sq), two (n_views, h, w, 3) float64 arrays from one launch: `sum` is render_views' array,
        sum_sq[v] what render_moments gives as sum_sq under view v's camera and seed.  With params.accumulate both running arrays are
        required and continued in place."""
        import numpy as np
        arr = _view_array(views)
        n = len(arr)
        h, w = (arr[0].camera.image_height, arr[0].camera.image_width) if n else (0, 0)
        if sum is None and sum_sq is None:
            if params.accumulate:
                raise RtError("render_views_moments: params.accumulate adds to running sums: pass them as `sum` and `sum_sq`")
            sum, sum_sq = np.zeros((n, h, w, 3), dtype=np.float64), np.zeros((n, h, w, 3), dtype=np.float64)
        _frame_arg("render_views_moments", "sum", sum, (n, h, w, 3))
        _frame_arg("render_views_moments", "sum_sq", sum_sq, (n, h, w, 3))
        _check(amd_lib().rt_render_views_moments(self._handle, arr, n, C.byref(params), C.c_void_p(sum.ctypes.data),
                                                 C.c_void_p(sum_sq.ctypes.data)), "rt_render_views_moments")
        return sum, sum_sq

    def render_views_moments_device(self, params: RenderParams, views, d_sum_ptr: int, d_sum_sq_ptr: int, stream: int = 0):
        """rt_render_views_moments_device: two device buffers of n_views frames of 3 w h doubles, view-major (sums, sums of squares);
        enqueued on `stream` without synchronising (the view records are copied during the call)."""
        arr = _view_array(views)
        _check(amd_lib().rt_render_views_moments_device(self._handle, arr, len(arr), C.byref(params), C.c_void_p(d_sum_ptr),
                                                        C.c_void_p(d_sum_sq_ptr or None), C.c_void_p(stream)), "rt_render_views_moments_device")

    def render_mean(self, params: RenderParams, camera: Camera | None = None, mean=None, rgba8: bool = False):
        """rt_render_mean: the samples of params' range folded into a running mean, m += (c - m) / (s + 1) per sample s (the reference's
        live_render, src/renderer.rs:114).  `mean`: the (h, w, 3) float64 frame to continue — required when params.sample_begin > 0,
        which is also the number of samples already in it — written and returned.  With rgba8, returns (mean, (h, w, 4) uint8): the
        display frame color_to_rgb(mean) with alpha 255."""
        import numpy as np
        cam = camera if camera is not None else self.host_scene.camera
        h, w = cam.image_height, cam.image_width
        if mean is None:
            if params.sample_begin > 0:
                raise RtError("render_mean: params.sample_begin > 0 continues a running mean: pass it as `mean`")
            mean = np.zeros((h, w, 3), dtype=np.float64)
        _frame_arg("render_mean", "mean", mean, (h, w, 3))
        frame = np.zeros((h, w, 4), dtype=np.uint8) if rgba8 else None
        _check(amd_lib().rt_render_mean(self._handle, C.byref(cam), C.byref(params), C.c_void_p(mean.ctypes.data),
                                        C.c_void_p(frame.ctypes.data) if rgba8 else None), "rt_render_mean")
        return (mean, frame) if rgba8 else mean

    def render_mean_device(self, params: RenderParams, d_mean_ptr: int, d_rgba8_ptr: int = 0, stream: int = 0,
                           camera: Camera | None = None):
        """rt_render_mean_device: `d_mean_ptr` is a device frame of 3 w h doubles holding the mean of the first params.sample_begin
        samples (not read when that is 0); `d_rgba8_ptr`, if not 0, 4 w h device bytes for the display frame.  Enqueued on `stream`."""
        cam = camera if camera is not None else self.host_scene.camera
        _check(amd_lib().rt_render_mean_device(self._handle, C.byref(cam), C.byref(params), C.c_void_p(d_mean_ptr),
                                               C.c_void_p(d_rgba8_ptr or None), C.c_void_p(stream)), "rt_render_mean_device")

    def render_mean_moments(self, params: RenderParams, camera: Camera | None = None, mean=None, m2=None, rgba8: bool = False):
        """rt_render_mean_moments: render_mean with Welford's M2 beside the mean, M2 += (c - m) * (c - m') per sample (m the mean before
        the sample, m' after it).  `mean`, `m2`: the (h, w, 3) float64 frames to continue — both required when params.sample_begin > 0
        — written and returned: (mean, m2), or (mean, m2, (h, w, 4) uint8) with rgba8."""
        import numpy as np
        cam = camera if camera is not None else self.host_scene.camera
        h, w = cam.image_height, cam.image_width
        if mean is None and m2 is None:
            if params.sample_begin > 0:
                raise RtError("render_mean_moments: params.sample_begin > 0 continues running frames: pass them as `mean` and `m2`")
            mean, m2 = np.zeros((h, w, 3), dtype=np.float64), np.zeros((h, w, 3), dtype=np.float64)
        _frame_arg("render_mean_moments", "mean", mean, (h, w, 3))
        _frame_arg("render_mean_moments", "m2", m2, (h, w, 3))
        frame = np.zeros((h, w, 4), dtype=np.uint8) if rgba8 else None
        _check(amd_lib().rt_render_mean_moments(self._handle, C.byref(cam), C.byref(params), C.c_void_p(mean.ctypes.data),
                                                C.c_void_p(m2.ctypes.data), C.c_void_p(frame.ctypes.data) if rgba8 else None),
               "rt_render_mean_moments")
        return (mean, m2, frame) if rgba8 else (mean, m2)

    def render_mean_moments_device(self, params: RenderParams, d_mean_ptr: int, d_m2_ptr: int, d_rgba8_ptr: int = 0, stream: int = 0,
                                   camera: Camera | None = None):
        """rt_render_mean_moments_device: render_mean_device with `d_m2_ptr`, a second device frame of 3 w h doubles holding M2 of the
        first params.sample_begin samples (not read when that is 0).  Enqueued on `stream`."""
        cam = camera if camera is not None else self.host_scene.camera
        _check(amd_lib().rt_render_mean_moments_device(self._handle, C.byref(cam), C.byref(params), C.c_void_p(d_mean_ptr), C.c_void_p(d_m2_ptr),
                                                       C.c_void_p(d_rgba8_ptr or None), C.c_void_p(stream)), "rt_render_mean_moments_device")

    def render_until(self, noise: float, *, max_spp: int, pass_spp: int = 1, min_samples: int = 16, seed: int = 1, camera: Camera | None = None,
                     eps: "float | None" = None):
        """Refines a running mean and M2 on the device in passes of `pass_spp` samples (the last one cut at max_spp), each a
        render_mean_moments_device over the next sample range, and evaluates frame_noise_device (means form) after every pass.  Stops at
        the first pass with samples >= min_samples and noise <= `noise`, or at max_spp.  Returns (mean, m2, samples, noise): the two
        (h, w, 3) float64 frames — bit for bit render_mean_moments' over [0, samples) —, the sample count reached and the last pass's
        noise.  `eps`: frame_noise_params' (None: its default)."""
        import torch
        if max_spp < 1 or pass_spp < 1:
            raise RtError("render_until: max_spp and pass_spp must be at least 1")
        cam = camera if camera is not None else self.host_scene.camera
        h, w = cam.image_height, cam.image_width
        np_params = frame_noise_params(**({} if eps is None else {"eps": eps}))
        with torch.cuda.device(self.device):
            d_mean = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
            d_m2 = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
            d_out4 = torch.zeros(4, dtype=torch.float64, device="cuda")
            d_ws = torch.empty(metrics_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
            stream = torch.cuda.current_stream().cuda_stream
            samples, level = 0, float("inf")
            while samples < max_spp:
                end = min(samples + pass_spp, max_spp)
                self.render_mean_moments_device(render_params(seed=seed, sample_begin=samples, sample_end=end), d_mean.data_ptr(), d_m2.data_ptr(),
                                                stream=stream, camera=cam)
                samples = end
                frame_noise_device(w, h, RT_METRICS_MEANS, d_mean.data_ptr(), d_m2.data_ptr(), samples, d_out4.data_ptr(), d_ws.data_ptr(),
                                   params=np_params, stream=stream)
                level = float(d_out4.cpu()[2])  # (the download waits for the pass and the reduction; this loop hands no frame to the host, so it is its only wait)
                if samples >= min_samples and level <= noise:
                    break
            return d_mean.cpu().numpy(), d_m2.cpu().numpy(), samples, level

    def render_moments(self, params: RenderParams, camera: Camera | None = None, sum=None, sum_sq=None):
        """rt_render_moments: (sum, sum_sq), two (h, w, 3) float64 frames: the per-pixel sums rt_render gives and the in-order sums of
        the samples' squares.  With params.accumulate both running frames are required and continued in place."""
        import numpy as np
        cam = camera if camera is not None else self.host_scene.camera
        h, w = cam.image_height, cam.image_width
        if sum is None and sum_sq is None:
            if params.accumulate:
                raise RtError("render_moments: params.accumulate adds to running sums: pass them as `sum` and `sum_sq`")
            sum, sum_sq = np.zeros((h, w, 3), dtype=np.float64), np.zeros((h, w, 3), dtype=np.float64)
        _frame_arg("render_moments", "sum", sum, (h, w, 3))
        _frame_arg("render_moments", "sum_sq", sum_sq, (h, w, 3))
        _check(amd_lib().rt_render_moments(self._handle, C.byref(cam), C.byref(params), C.c_void_p(sum.ctypes.data),
                                           C.c_void_p(sum_sq.ctypes.data)), "rt_render_moments")
        return sum, sum_sq

    def render_moments_device(self, params: RenderParams, d_sum_ptr: int, d_sum_sq_ptr: int, stream: int = 0, camera: Camera | None = None):
        """rt_render_moments_device: two device frames of 3 w h doubles (sums, sums of squares); enqueued on `stream`."""
        cam = camera if camera is not None else self.host_scene.camera
        _check(amd_lib().rt_render_moments_device(self._handle, C.byref(cam), C.byref(params), C.c_void_p(d_sum_ptr),
                                                  C.c_void_p(d_sum_sq_ptr), C.c_void_p(stream)), "rt_render_moments_device")

    def render_pixels_device(self, params: RenderParams, d_pixels_ptr: int, n_pixels: int, d_sum_ptr: int,
                             d_sum_sq_ptr: int = 0, stream: int = 0, camera: Camera | None = None):
        """rt_render_pixels_device: the samples of params' range for the n_pixels entries (uint32 pixel indices, device memory) onto
        a device frame of sums (and of squared sums, if d_sum_sq_ptr is not 0)."""
        cam = camera if camera is not None else self.host_scene.camera
        _check(amd_lib().rt_render_pixels_device(self._handle, C.byref(cam), C.byref(params), C.c_void_p(d_pixels_ptr), n_pixels,
                                                 C.c_void_p(d_sum_ptr), C.c_void_p(d_sum_sq_ptr or None), C.c_void_p(stream)),
               "rt_render_pixels_device")

    def render_adaptive(self, params: RenderParams, *, min_spp=16, batch_spp=16, rel=0.02, abs=1e-3, camera: Camera | None = None):
        """rt_render_adaptive: returns (sum (h, w, 3), spp (h, w), sum_sq (h, w, 3), result dict); the maximum spp is the
        params' sample_end (the camera's spp when 0)."""
        import numpy as np
        cam = camera if camera is not None else self.host_scene.camera
        h, w = cam.image_height, cam.image_width
        a = adaptive_params(min_spp=min_spp, batch_spp=batch_spp, rel_threshold=rel, abs_threshold=abs)
        total = np.zeros((h, w, 3), dtype=np.float64)
        sq = np.zeros((h, w, 3), dtype=np.float64)
        spp = np.zeros((h, w), dtype=np.int32)
        res = AdaptiveResult()
        _check(amd_lib().rt_render_adaptive(self._handle, C.byref(cam), C.byref(params), C.byref(a), C.c_void_p(total.ctypes.data),
                                            C.c_void_p(spp.ctypes.data), C.c_void_p(sq.ctypes.data), C.byref(res)),
               "rt_render_adaptive")
        return total, spp, sq, res.as_dict()

    def render_adaptive_device(self, params: RenderParams, adaptive: AdaptiveParams, d_sum_ptr: int, d_spp_ptr: int,
                               d_sum_sq_ptr: int = 0, stream: int = 0, camera: Camera | None = None) -> dict:
        """rt_render_adaptive_device: device buffers of 3 w h doubles (sums, optionally squared sums) and w h int32 (spp)."""
        cam = camera if camera is not None else self.host_scene.camera
        res = AdaptiveResult()
        _check(amd_lib().rt_render_adaptive_device(self._handle, C.byref(cam), C.byref(params), C.byref(adaptive), C.c_void_p(d_sum_ptr),
                                                   C.c_void_p(d_spp_ptr), C.c_void_p(d_sum_sq_ptr or None), C.c_void_p(stream),
                                                   C.byref(res)), "rt_render_adaptive_device")
        return res.as_dict()

    def close(self):
        if getattr(self, "_handle", None):
            amd_lib().rt_scene_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def tiles_to_frame_device(width, height, shard_count, d_gathered_ptr: int, d_frame_ptr: int, stream: int = 0):
    _check(amd_lib().rt_tiles_to_frame_device(width, height, shard_count, C.c_void_p(d_gathered_ptr),
                                              C.c_void_p(d_frame_ptr), C.c_void_p(stream)),
           "rt_tiles_to_frame_device")


def resolve_rgb8_device(width, height, spp, d_frame_ptr: int, d_rgb8_ptr: int, stream: int = 0):
    _check(amd_lib().rt_resolve_rgb8_device(width, height, spp, C.c_void_p(d_frame_ptr), C.c_void_p(d_rgb8_ptr),
                                            C.c_void_p(stream)), "rt_resolve_rgb8_device")


def resolve_rgb8_values_device(n_values, spp, d_sum_ptr: int, d_rgb8_ptr: int, stream: int = 0):
    _check(amd_lib().rt_resolve_rgb8_values_device(n_values, spp, C.c_void_p(d_sum_ptr), C.c_void_p(d_rgb8_ptr),
                                                   C.c_void_p(stream)), "rt_resolve_rgb8_values_device")


def resolve_rgb8_spp_device(width, height, d_sum_ptr: int, d_spp_ptr: int, d_rgb8_ptr: int, stream: int = 0):
    _check(amd_lib().rt_resolve_rgb8_spp_device(width, height, C.c_void_p(d_sum_ptr), C.c_void_p(d_spp_ptr), C.c_void_p(d_rgb8_ptr),
                                                C.c_void_p(stream)), "rt_resolve_rgb8_spp_device")


def resolve_rgba8_device(width, height, d_mean_ptr: int, d_rgba8_ptr: int, stream: int = 0):
    """rt_resolve_rgba8_device: color_to_rgb(mean) with alpha 255 over a device frame of means (4 bytes per pixel)."""
    _check(amd_lib().rt_resolve_rgba8_device(width, height, C.c_void_p(d_mean_ptr), C.c_void_p(d_rgba8_ptr), C.c_void_p(stream)),
           "rt_resolve_rgba8_device")


def _workspace_bytes(symbol, what, *args) -> int:
    n = int(getattr(amd_lib(), symbol)(*args))
    if n < 0:
        raise RtError(f"{symbol}: no workspace for {what}")
    return n


def _frame_end(device, inputs, out_shape, rgba8_shape, ws_bytes, call, out_dtype="float64"):
    """The device work of the blocking frame-end wrappers, on `device`: uploads `inputs` (numpy arrays; None stays None), allocates the
    output, `ws_bytes` of workspace and, with rgba8_shape, the display frame, makes the *_device call on the current stream —
    call(the inputs' device pointers (0 for None), output, workspace, display frame or 0, stream) —, synchronises and downloads:
    the output, or (output, display frame) with rgba8_shape."""
    import torch
    with torch.cuda.device(device):
        d_in = [torch.from_numpy(a).cuda() if a is not None else None for a in inputs]
        d_out = torch.empty(out_shape, dtype=getattr(torch, out_dtype), device="cuda")
        d_ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        d_rgba = torch.empty(rgba8_shape, dtype=torch.uint8, device="cuda") if rgba8_shape else None
        call([t.data_ptr() if t is not None else 0 for t in d_in], d_out.data_ptr(), d_ws.data_ptr(), d_rgba.data_ptr() if rgba8_shape else 0,
             torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        return (out, d_rgba.cpu().numpy()) if rgba8_shape else out


def _denoise_call(symbol, *args):
    """One rt_denoise*_device call, `args` in the header's order.  Where the binding takes a pointer, a device address goes as a
    C.c_void_p (0: null) and a params struct by reference (None: null); the return code is checked under the symbol's name."""
    fn = getattr(amd_lib(), symbol)

    def pointer(a):
        return C.byref(a) if isinstance(a, C.Structure) else C.c_void_p(a or None) if a is not None else None
    _check(fn(*[pointer(a) if t is C.c_void_p else a for t, a in zip(fn.argtypes, args)]), symbol)


def _spatial_split(kw):
    """The keywords of a *_mean_spatial wrapper: (denoise_spatial_params of spatial_below= and window_radius=, every other keyword)."""
    kw = dict(kw)
    return denoise_spatial_params(**{k: kw.pop(k) for k in ("spatial_below", "window_radius") if k in kw}), kw


def _denoise_blocking(who, frames, rank, shape_error, make_params, kw, ws_bytes, call, *, optional=(), spp_map=None, copy=False, rgba8=False,
                      device=0):
    """The body of every blocking denoise wrapper: checks the shapes, builds the params, uploads, runs, downloads.  `frames`: the float64
    inputs in the order `call` finds their device pointers in (contiguous views, or with `copy` copies); all of one shape, of `rank`
    dimensions, (h, w, 3) or (n_views, h, w, 3), else `shape_error`; a None is a null pointer at an index in `optional` and refused
    elsewhere.  `spp_map`: an (h, w) int32 map, whose pointer follows the frames'.  `size` is (w, h) or (w, h, n_views):
    ws_bytes(*size) sizes the workspace, and call(size, input pointers, output, workspace, keywords) makes the *_device call, the
    keywords being d_rgba8_ptr=, params= (make_params(**kw)) and stream=.  Returns the filtered means, or (means, display bytes)
    with rgba8."""
    import numpy as np
    inputs = [None if a is None else np.array(a, dtype=np.float64, order="C") if copy else np.ascontiguousarray(a, dtype=np.float64) for a in frames]
    given = [a for a in inputs if a is not None]
    if any(a is None and i not in optional for i, a in enumerate(inputs)) or given[0].ndim != rank or given[0].shape[-1] != 3 or \
            any(a.shape != given[0].shape for a in given):
        raise RtError(f"{who}: {shape_error}")
    dims = given[0].shape[:-1]  # (h, w) or (n_views, h, w)
    if spp_map is not None:
        spp_map = np.ascontiguousarray(spp_map, dtype=np.int32)
        if spp_map.shape != dims:
            raise RtError(f"{who}: `spp_map` must have shape {dims}")
    params = make_params(**kw)
    size = (dims[-1], dims[-2]) + dims[:-2]
    return _frame_end(device, inputs + [spp_map], dims + (3,), rgba8 and dims + (4,), ws_bytes(*size),
                      lambda d, out, ws, rgba, stream: call(size, d, out, ws, dict(d_rgba8_ptr=rgba, params=params, stream=stream)))


def denoise_workspace_bytes(width, height) -> int:
    return _workspace_bytes("rt_denoise_workspace_bytes", f"a {width}x{height} frame", width, height)


def denoise_device(width, height, d_sum_ptr: int, d_sum_sq_ptr: int, spp: int, d_mean_out_ptr: int, d_workspace_ptr: int, *,
                   d_spp_ptr: int = 0, d_rgba8_ptr: int = 0, params: "DenoiseParams | None" = None, stream: int = 0):
    """rt_denoise_device: the variance-guided à-trous filter over device frames of sums and sums of squares (3 w h doubles each) with
    the uniform sample count `spp` or, if d_spp_ptr is not 0, a device map of w h int32.  Writes 3 w h doubles of filtered means and,
    if d_rgba8_ptr is not 0, 4 w h display bytes; `d_workspace_ptr`: denoise_workspace_bytes(w, h) device bytes.  Enqueued on `stream`."""
    _denoise_call("rt_denoise_device", width, height, d_sum_ptr, d_sum_sq_ptr, spp, d_spp_ptr, params, d_mean_out_ptr, d_rgba8_ptr, d_workspace_ptr, stream)


def denoise(sum, sum_sq, spp, *, spp_map=None, rgba8=False, device=0, **kw):
    """Uploads (h, w, 3) frames of sums and sums of squares (and an (h, w) int32 spp map, if given), runs rt_denoise_device with
    denoise_params(**kw) and downloads: the (h, w, 3) float64 filtered means, or (means, (h, w, 4) uint8) with rgba8."""
    return _denoise_blocking("denoise", [sum, sum_sq], 3, "`sum` and `sum_sq` must be (h, w, 3) frames of one shape", denoise_params, kw,
                             denoise_workspace_bytes,
                             lambda size, d, out, ws, tail: denoise_device(*size, d[0], d[1], int(spp), out, ws, d_spp_ptr=d[2], **tail),
                             spp_map=spp_map, rgba8=rgba8, device=device)


def albedo_materials(host_scene):
    """rt_albedo_materials (GPU-free): (materials, textures), ctypes arrays of Material (n_materials entries) and Texture (the
    description's textures, then one SOLID per metal or dielectric) — the tables of the scene's albedo scene."""
    desc = host_scene.desc
    mats = (Material * max(1, desc.n_materials))()
    texs = (Texture * max(1, desc.n_textures + desc.n_materials))()
    n = C.c_int32(0)
    _check(amd_lib().rt_albedo_materials(C.byref(desc), C.addressof(mats), C.addressof(texs), C.byref(n)), "rt_albedo_materials")
    return (Material * desc.n_materials).from_buffer_copy(mats), (Texture * n.value).from_buffer_copy(texs)


def albedo_camera(camera: Camera) -> Camera:
    """The camera an albedo scene is rendered with: `camera` with background (1, 1, 1), so that a miss demodulates to the background."""
    cam = Camera.from_buffer_copy(camera)
    cam.background = Vec3(1.0, 1.0, 1.0)
    return cam


def denoise_albedo_workspace_bytes(width, height) -> int:
    return _workspace_bytes("rt_denoise_albedo_workspace_bytes", f"a {width}x{height} frame", width, height)


def denoise_albedo_device(width, height, d_sum_ptr: int, d_sum_sq_ptr: int, spp: int, d_albedo_sum_ptr: int, albedo_spp: int,
                          d_mean_out_ptr: int, d_workspace_ptr: int, *, d_spp_ptr: int = 0, d_rgba8_ptr: int = 0,
                          params: "DenoiseAlbedoParams | None" = None, stream: int = 0):
    """rt_denoise_albedo_device: rt_denoise_device with a device frame of albedo sums (3 w h doubles, `albedo_spp` samples of the
    albedo scene) beside the moments; `d_workspace_ptr`: denoise_albedo_workspace_bytes(w, h) device bytes.  Enqueued on `stream`."""
    _denoise_call("rt_denoise_albedo_device", width, height, d_sum_ptr, d_sum_sq_ptr, spp, d_spp_ptr, d_albedo_sum_ptr, albedo_spp, params,
                 d_mean_out_ptr, d_rgba8_ptr, d_workspace_ptr, stream)


def denoise_albedo(sum, sum_sq, spp, albedo_sum, albedo_spp, *, spp_map=None, rgba8=False, device=0, **kw):
    """Uploads (h, w, 3) frames of sums, sums of squares and albedo sums (and an (h, w) int32 spp map, if given), runs
    rt_denoise_albedo_device with denoise_albedo_params(**kw) and downloads: the (h, w, 3) float64 filtered means, or
    (means, (h, w, 4) uint8) with rgba8."""
    return _denoise_blocking("denoise_albedo", [sum, sum_sq, albedo_sum], 3, "`sum`, `sum_sq` and `albedo_sum` must be (h, w, 3) frames of one shape",
                             denoise_albedo_params, kw, denoise_albedo_workspace_bytes,
                             lambda size, d, out, ws, tail: denoise_albedo_device(*size, d[0], d[1], int(spp), d[2], int(albedo_spp), out, ws,
                                                                                  d_spp_ptr=d[3], **tail),
                             spp_map=spp_map, rgba8=rgba8, device=device)


RT_SURFACE_ID_COLOURS = 26


def surface_id_tables(host_scene):
    """rt_surface_id_tables (GPU-free): (spheres, quads, media, materials, textures), ctypes arrays — the description's spheres, quads
    and media with their material rewritten to the surface's palette entry, and the 26 DIFFUSE_LIGHT materials and SOLID textures of
    the palette: the tables of the scene's surface-ID scene."""
    desc = host_scene.desc
    sph = (Sphere * max(1, desc.n_spheres))()
    qua = (Quad * max(1, desc.n_quads))()
    med = (ConstantMedium * max(1, desc.n_media))()
    mats = (Material * RT_SURFACE_ID_COLOURS)()
    texs = (Texture * RT_SURFACE_ID_COLOURS)()
    _check(amd_lib().rt_surface_id_tables(C.byref(desc), C.addressof(sph), C.addressof(qua), C.addressof(med), C.addressof(mats),
                                          C.addressof(texs)), "rt_surface_id_tables")
    return ((Sphere * desc.n_spheres).from_buffer_copy(sph), (Quad * desc.n_quads).from_buffer_copy(qua),
            (ConstantMedium * desc.n_media).from_buffer_copy(med), mats, texs)


def surface_id_camera(camera: Camera) -> Camera:
    """The camera a surface-ID scene is rendered with: `camera` with background (0, 0, 0), which is no palette colour."""
    cam = Camera.from_buffer_copy(camera)
    cam.background = Vec3(0.0, 0.0, 0.0)
    return cam


def denoise_guided_workspace_bytes(width, height, with_albedo) -> int:
    return _workspace_bytes("rt_denoise_guided_workspace_bytes", f"a {width}x{height} frame", width, height, 1 if with_albedo else 0)


def denoise_guided_device(width, height, d_sum_ptr: int, d_sum_sq_ptr: int, spp: int, d_albedo_sum_ptr: int, albedo_spp: int, d_edge_sum_ptr: int,
                          edge_spp: int, d_mean_out_ptr: int, d_workspace_ptr: int, *, d_spp_ptr: int = 0, d_rgba8_ptr: int = 0,
                          params: "DenoiseGuidedParams | None" = None, stream: int = 0):
    """rt_denoise_guided_device: rt_denoise_albedo_device (d_albedo_sum_ptr 0: rt_denoise_device) with a device frame of edge-guide sums
    (3 w h doubles, `edge_spp` samples, e.g. of the surface-ID scene) beside its inputs; `d_workspace_ptr`:
    denoise_guided_workspace_bytes(w, h, d_albedo_sum_ptr != 0) device bytes.  Enqueued on `stream`."""
    _denoise_call("rt_denoise_guided_device", width, height, d_sum_ptr, d_sum_sq_ptr, spp, d_spp_ptr, d_albedo_sum_ptr, albedo_spp, d_edge_sum_ptr,
                 edge_spp, params, d_mean_out_ptr, d_rgba8_ptr, d_workspace_ptr, stream)


def denoise_guided(sum, sum_sq, spp, edge_sum, edge_spp, *, albedo_sum=None, albedo_spp=0, spp_map=None, rgba8=False, device=0, **kw):
    """Uploads (h, w, 3) frames of sums, sums of squares and edge-guide sums (and albedo sums and an (h, w) int32 spp map, if given),
    runs rt_denoise_guided_device with denoise_guided_params(**kw) and downloads: the (h, w, 3) float64 filtered means, or
    (means, (h, w, 4) uint8) with rgba8."""
    return _denoise_blocking("denoise_guided", [sum, sum_sq, edge_sum, albedo_sum], 3,
                             "`sum`, `sum_sq`, `edge_sum` and `albedo_sum` must be (h, w, 3) frames of one shape", denoise_guided_params, kw,
                             lambda w, h: denoise_guided_workspace_bytes(w, h, albedo_sum is not None),
                             lambda size, d, out, ws, tail: denoise_guided_device(*size, d[0], d[1], int(spp), d[3], int(albedo_spp), d[2], int(edge_spp),
                                                                                  out, ws, d_spp_ptr=d[4], **tail),
                             optional=(3,), spp_map=spp_map, rgba8=rgba8, device=device)


def denoise_views_workspace_bytes(width, height, n_views) -> int:
    return _workspace_bytes("rt_denoise_views_workspace_bytes", f"{n_views} frames of {width}x{height}", width, height, n_views)


def denoise_albedo_views_workspace_bytes(width, height, n_views) -> int:
    return _workspace_bytes("rt_denoise_albedo_views_workspace_bytes", f"{n_views} frames of {width}x{height}", width, height, n_views)


def denoise_views_device(width, height, n_views, d_sum_ptr: int, d_sum_sq_ptr: int, spp: int, d_mean_out_ptr: int, d_workspace_ptr: int, *,
                         d_rgba8_ptr: int = 0, params: "DenoiseParams | None" = None, stream: int = 0):
    """rt_denoise_views_device: denoise_device over a stack of n_views frames in one set of launches; every buffer is view-major
    (n_views frames of 3 w h doubles; d_rgba8_ptr, if not 0, n_views frames of 4 w h bytes), `spp` is uniform, `d_workspace_ptr`:
    denoise_views_workspace_bytes(w, h, n_views) device bytes.  View v equals denoise_device on view v's frames.  Enqueued on `stream`."""
    _denoise_call("rt_denoise_views_device", width, height, n_views, d_sum_ptr, d_sum_sq_ptr, spp, params, d_mean_out_ptr, d_rgba8_ptr, d_workspace_ptr,
                 stream)


def denoise_albedo_views_device(width, height, n_views, d_sum_ptr: int, d_sum_sq_ptr: int, spp: int, d_albedo_sum_ptr: int, albedo_spp: int,
                                d_mean_out_ptr: int, d_workspace_ptr: int, *, d_rgba8_ptr: int = 0,
                                params: "DenoiseAlbedoParams | None" = None, stream: int = 0):
    """rt_denoise_albedo_views_device: denoise_albedo_device over a stack of n_views frames in one set of launches, the albedo sums
    view-major as well; `d_workspace_ptr`: denoise_albedo_views_workspace_bytes(w, h, n_views) device bytes.  Enqueued on `stream`."""
    _denoise_call("rt_denoise_albedo_views_device", width, height, n_views, d_sum_ptr, d_sum_sq_ptr, spp, d_albedo_sum_ptr, albedo_spp, params,
                 d_mean_out_ptr, d_rgba8_ptr, d_workspace_ptr, stream)


def denoise_views(sum, sum_sq, spp, *, rgba8=False, device=0, **kw):
    """Uploads (n_views, h, w, 3) stacks of sums and sums of squares (what render_views_moments returns), runs rt_denoise_views_device
    with denoise_params(**kw) and downloads: the (n_views, h, w, 3) float64 filtered means, or (means, (n_views, h, w, 4) uint8) with rgba8."""
    return _denoise_blocking("denoise_views", [sum, sum_sq], 4, "the frames must be (n_views, h, w, 3) arrays of one shape", denoise_params, kw, denoise_views_workspace_bytes,
                             lambda size, d, out, ws, tail: denoise_views_device(*size, d[0], d[1], int(spp), out, ws, **tail),
                             rgba8=rgba8, device=device)


def denoise_albedo_views(sum, sum_sq, spp, albedo_sum, albedo_spp, *, rgba8=False, device=0, **kw):
    """denoise_views with an (n_views, h, w, 3) stack of albedo sums (render_views of the albedo scene): rt_denoise_albedo_views_device
    with denoise_albedo_params(**kw)."""
    return _denoise_blocking("denoise_albedo_views", [sum, sum_sq, albedo_sum], 4, "the frames must be (n_views, h, w, 3) arrays of one shape", denoise_albedo_params, kw,
                             denoise_albedo_views_workspace_bytes,
                             lambda size, d, out, ws, tail: denoise_albedo_views_device(*size, d[0], d[1], int(spp), d[2], int(albedo_spp), out, ws, **tail),
                             rgba8=rgba8, device=device)


def denoise_mean_device(width, height, d_mean_ptr: int, d_m2_ptr: int, samples: int, d_mean_out_ptr: int, d_workspace_ptr: int, *,
                        d_rgba8_ptr: int = 0, params: "DenoiseParams | None" = None, stream: int = 0):
    """rt_denoise_mean_device: denoise_device over device frames of running means and of M2 (3 w h doubles each, what
    render_mean_moments_device keeps) after `samples` samples of every pixel; `d_workspace_ptr`: denoise_workspace_bytes(w, h) device
    bytes.  Enqueued on `stream`."""
    _denoise_call("rt_denoise_mean_device", width, height, d_mean_ptr, d_m2_ptr, samples, params, d_mean_out_ptr, d_rgba8_ptr, d_workspace_ptr, stream)


def denoise_albedo_mean_device(width, height, d_mean_ptr: int, d_m2_ptr: int, samples: int, d_albedo_mean_ptr: int, d_mean_out_ptr: int,
                               d_workspace_ptr: int, *, d_rgba8_ptr: int = 0, params: "DenoiseAlbedoParams | None" = None, stream: int = 0):
    """rt_denoise_albedo_mean_device: denoise_mean_device with a device frame of albedo means (3 w h doubles: render_mean_device of the
    albedo scene) beside them; `d_workspace_ptr`: denoise_albedo_workspace_bytes(w, h) device bytes.  Enqueued on `stream`."""
    _denoise_call("rt_denoise_albedo_mean_device", width, height, d_mean_ptr, d_m2_ptr, samples, d_albedo_mean_ptr, params, d_mean_out_ptr,
                 d_rgba8_ptr, d_workspace_ptr, stream)


def denoise_mean(mean, m2, samples, *, rgba8=False, device=0, **kw):
    """Uploads (h, w, 3) frames of running means and of M2 after `samples` samples, runs rt_denoise_mean_device with denoise_params(**kw)
    and downloads: the (h, w, 3) float64 filtered means, or (means, (h, w, 4) uint8) with rgba8."""
    return _denoise_blocking("denoise_mean", [mean, m2], 3, "the frames must be (h, w, 3) and of one shape", denoise_params, kw, denoise_workspace_bytes,
                             lambda size, d, out, ws, tail: denoise_mean_device(*size, d[0], d[1], int(samples), out, ws, **tail),
                             copy=True, rgba8=rgba8, device=device)


def denoise_albedo_mean(mean, m2, samples, albedo_mean, *, rgba8=False, device=0, **kw):
    """denoise_mean with an (h, w, 3) frame of albedo means beside the two: rt_denoise_albedo_mean_device with denoise_albedo_params(**kw)."""
    if albedo_mean is None:
        raise RtError("denoise_albedo_mean: `albedo_mean` is required")
    return _denoise_blocking("denoise_albedo_mean", [mean, m2, albedo_mean], 3, "the frames must be (h, w, 3) and of one shape", denoise_albedo_params, kw, denoise_albedo_workspace_bytes,
                             lambda size, d, out, ws, tail: denoise_albedo_mean_device(*size, d[0], d[1], int(samples), d[2], out, ws, **tail),
                             copy=True, rgba8=rgba8, device=device)


def denoise_mean_spatial_device(width, height, d_mean_ptr: int, d_m2_ptr: int, samples: int, d_mean_out_ptr: int, d_workspace_ptr: int, *,
                                d_rgba8_ptr: int = 0, spatial: "DenoiseSpatialParams | None" = None, params: "DenoiseParams | None" = None,
                                stream: int = 0):
    """rt_denoise_mean_spatial_device: denoise_mean_device that, for frames of fewer than spatial.spatial_below samples (default 2),
    takes the variance from the spread of the neighbouring pixels' means; `d_m2_ptr` may then be 0.  Enqueued on `stream`."""
    _denoise_call("rt_denoise_mean_spatial_device", width, height, d_mean_ptr, d_m2_ptr, samples, spatial, params, d_mean_out_ptr, d_rgba8_ptr,
                 d_workspace_ptr, stream)


def denoise_albedo_mean_spatial_device(width, height, d_mean_ptr: int, d_m2_ptr: int, samples: int, d_albedo_mean_ptr: int, d_mean_out_ptr: int,
                                       d_workspace_ptr: int, *, d_rgba8_ptr: int = 0, spatial: "DenoiseSpatialParams | None" = None,
                                       params: "DenoiseAlbedoParams | None" = None, stream: int = 0):
    """rt_denoise_albedo_mean_spatial_device: denoise_mean_spatial_device with a device frame of albedo means beside the two;
    `d_workspace_ptr`: denoise_albedo_workspace_bytes(w, h) device bytes.  Enqueued on `stream`."""
    _denoise_call("rt_denoise_albedo_mean_spatial_device", width, height, d_mean_ptr, d_m2_ptr, samples, d_albedo_mean_ptr, spatial, params,
                 d_mean_out_ptr, d_rgba8_ptr, d_workspace_ptr, stream)


def denoise_mean_spatial(mean, m2, samples, *, rgba8=False, device=0, **kw):
    """denoise_mean through rt_denoise_mean_spatial_device: `m2` may be None where samples < spatial_below; spatial_below= and
    window_radius= go to denoise_spatial_params, every other keyword to denoise_params."""
    spatial, kw = _spatial_split(kw)
    return _denoise_blocking("denoise_mean_spatial", [mean, m2], 3, "the frames must be (h, w, 3) and of one shape", denoise_params, kw, denoise_workspace_bytes,
                             lambda size, d, out, ws, tail: denoise_mean_spatial_device(*size, d[0], d[1], int(samples), out, ws, spatial=spatial, **tail),
                             optional=(1,), copy=True, rgba8=rgba8, device=device)


def denoise_albedo_mean_spatial(mean, m2, samples, albedo_mean, *, rgba8=False, device=0, **kw):
    """denoise_mean_spatial with an (h, w, 3) frame of albedo means beside the two: rt_denoise_albedo_mean_spatial_device."""
    if albedo_mean is None:
        raise RtError("denoise_albedo_mean_spatial: `albedo_mean` is required")
    spatial, kw = _spatial_split(kw)
    return _denoise_blocking("denoise_albedo_mean_spatial", [mean, m2, albedo_mean], 3, "the frames must be (h, w, 3) and of one shape", denoise_albedo_params, kw,
                             denoise_albedo_workspace_bytes,
                             lambda size, d, out, ws, tail: denoise_albedo_mean_spatial_device(*size, d[0], d[1], int(samples), d[2], out, ws,
                                                                                               spatial=spatial, **tail),
                             optional=(1,), copy=True, rgba8=rgba8, device=device)


def denoise_guided_mean_device(width, height, d_mean_ptr: int, d_m2_ptr: int, samples: int, d_albedo_mean_ptr: int, d_edge_mean_ptr: int,
                               d_mean_out_ptr: int, d_workspace_ptr: int, *, d_rgba8_ptr: int = 0, params: "DenoiseGuidedParams | None" = None,
                               stream: int = 0):
    """rt_denoise_guided_mean_device: denoise_albedo_mean_device (d_albedo_mean_ptr 0: denoise_mean_device) with a device frame of
    edge-guide means (3 w h doubles: render_mean_device of the surface-ID scene) beside its inputs; `d_workspace_ptr`:
    denoise_guided_workspace_bytes(w, h, d_albedo_mean_ptr != 0) device bytes.  Enqueued on `stream`."""
    _denoise_call("rt_denoise_guided_mean_device", width, height, d_mean_ptr, d_m2_ptr, samples, d_albedo_mean_ptr, d_edge_mean_ptr, params,
                 d_mean_out_ptr, d_rgba8_ptr, d_workspace_ptr, stream)


def denoise_guided_mean_spatial_device(width, height, d_mean_ptr: int, d_m2_ptr: int, samples: int, d_albedo_mean_ptr: int, d_edge_mean_ptr: int,
                                       d_mean_out_ptr: int, d_workspace_ptr: int, *, d_rgba8_ptr: int = 0,
                                       spatial: "DenoiseSpatialParams | None" = None, params: "DenoiseGuidedParams | None" = None, stream: int = 0):
    """rt_denoise_guided_mean_spatial_device: denoise_guided_mean_device that, for frames of fewer than spatial.spatial_below samples,
    takes the variance from the spread of the neighbouring pixels of the same surface; `d_m2_ptr` may then be 0.  Enqueued on `stream`."""
    _denoise_call("rt_denoise_guided_mean_spatial_device", width, height, d_mean_ptr, d_m2_ptr, samples, d_albedo_mean_ptr, d_edge_mean_ptr, spatial,
                 params, d_mean_out_ptr, d_rgba8_ptr, d_workspace_ptr, stream)


def denoise_guided_views_workspace_bytes(width, height, n_views, with_albedo) -> int:
    return _workspace_bytes("rt_denoise_guided_views_workspace_bytes", f"{n_views} frames of {width}x{height}", width, height, n_views,
                            1 if with_albedo else 0)


def denoise_guided_views_device(width, height, n_views, d_sum_ptr: int, d_sum_sq_ptr: int, spp: int, d_albedo_sum_ptr: int, albedo_spp: int,
                                d_edge_sum_ptr: int, edge_spp: int, d_mean_out_ptr: int, d_workspace_ptr: int, *, d_rgba8_ptr: int = 0,
                                params: "DenoiseGuidedParams | None" = None, stream: int = 0):
    """rt_denoise_guided_views_device: denoise_guided_device over a stack of n_views frames in one set of launches, every buffer
    view-major; `d_workspace_ptr`: denoise_guided_views_workspace_bytes(w, h, n_views, d_albedo_sum_ptr != 0) device bytes.  View v
    equals denoise_guided_device on view v's frames.  Enqueued on `stream`."""
    _denoise_call("rt_denoise_guided_views_device", width, height, n_views, d_sum_ptr, d_sum_sq_ptr, spp, d_albedo_sum_ptr, albedo_spp, d_edge_sum_ptr,
                 edge_spp, params, d_mean_out_ptr, d_rgba8_ptr, d_workspace_ptr, stream)


def denoise_guided_mean(mean, m2, samples, edge_mean, *, albedo_mean=None, rgba8=False, device=0, **kw):
    """Uploads (h, w, 3) frames of running means, of M2 after `samples` samples and of edge-guide means (and of albedo means, if given),
    runs rt_denoise_guided_mean_device with denoise_guided_params(**kw) and downloads: the (h, w, 3) float64 filtered means, or
    (means, (h, w, 4) uint8) with rgba8."""
    if m2 is None:
        raise RtError("denoise_guided_mean: `m2` is required")
    if edge_mean is None:
        raise RtError("denoise_guided_mean: `edge_mean` is required")
    return _denoise_blocking("denoise_guided_mean", [mean, m2, edge_mean, albedo_mean], 3, "the frames must be (h, w, 3) and of one shape", denoise_guided_params, kw,
                             lambda w, h: denoise_guided_workspace_bytes(w, h, albedo_mean is not None),
                             lambda size, d, out, ws, tail: denoise_guided_mean_device(*size, d[0], d[1], int(samples), d[3], d[2], out, ws, **tail),
                             optional=(3,), copy=True, rgba8=rgba8, device=device)


def denoise_guided_mean_spatial(mean, m2, samples, edge_mean, *, albedo_mean=None, rgba8=False, device=0, **kw):
    """denoise_guided_mean through rt_denoise_guided_mean_spatial_device: `m2` may be None where samples < spatial_below; spatial_below=
    and window_radius= go to denoise_spatial_params, every other keyword to denoise_guided_params."""
    spatial, kw = _spatial_split(kw)
    if edge_mean is None:
        raise RtError("denoise_guided_mean_spatial: `edge_mean` is required")
    return _denoise_blocking("denoise_guided_mean_spatial", [mean, m2, edge_mean, albedo_mean], 3, "the frames must be (h, w, 3) and of one shape", denoise_guided_params, kw,
                             lambda w, h: denoise_guided_workspace_bytes(w, h, albedo_mean is not None),
                             lambda size, d, out, ws, tail: denoise_guided_mean_spatial_device(*size, d[0], d[1], int(samples), d[3], d[2], out, ws,
                                                                                               spatial=spatial, **tail),
                             optional=(1, 3), copy=True, rgba8=rgba8, device=device)


def denoise_guided_views(sum, sum_sq, spp, edge_sum, edge_spp, *, albedo_sum=None, albedo_spp=0, rgba8=False, device=0, **kw):
    """Uploads (n_views, h, w, 3) stacks of sums, sums of squares and edge-guide sums (render_views of the surface-ID scene; and of
    albedo sums, if given), runs rt_denoise_guided_views_device with denoise_guided_params(**kw) and downloads: the (n_views, h, w, 3)
    float64 filtered means, or (means, (n_views, h, w, 4) uint8) with rgba8."""
    if edge_sum is None:
        raise RtError("denoise_guided_views: `edge_sum` is required")
    return _denoise_blocking("denoise_guided_views", [sum, sum_sq, edge_sum, albedo_sum], 4, "the frames must be (n_views, h, w, 3) arrays of one shape", denoise_guided_params, kw,
                             lambda w, h, n: denoise_guided_views_workspace_bytes(w, h, n, albedo_sum is not None),
                             lambda size, d, out, ws, tail: denoise_guided_views_device(*size, d[0], d[1], int(spp), d[3], int(albedo_spp), d[2],
                                                                                        int(edge_spp), out, ws, **tail),
                             optional=(3,), rgba8=rgba8, device=device)


def tonemap_workspace_bytes(width, height) -> int:
    return _workspace_bytes("rt_tonemap_workspace_bytes", f"a {width}x{height} frame", width, height)


def tonemap_device(width, height, d_values_ptr: int, spp: int, *, d_spp_ptr: int = 0, d_rgb8_ptr: int = 0, d_rgba8_ptr: int = 0,
                   d_workspace_ptr: int = 0, params: "TonemapParams | None" = None, stream: int = 0):
    """rt_tonemap_device: exposure, tone curve, gamma and quantisation over a device frame of 3 w h doubles — sums with the uniform
    sample count `spp` or, if d_spp_ptr is not 0, a device map of w h int32; means with spp = 1 — into 3 w h bytes at d_rgb8_ptr, 4 w h
    bytes at d_rgba8_ptr, or both.  With params.auto_key > 0 the exposure comes from the frame's log-average luminance, reduced in
    `d_workspace_ptr` (tonemap_workspace_bytes(w, h) device bytes).  Enqueued on `stream`."""
    _check(amd_lib().rt_tonemap_device(width, height, C.c_void_p(d_values_ptr), spp, C.c_void_p(d_spp_ptr or None),
                                       C.byref(params) if params is not None else None, C.c_void_p(d_rgb8_ptr or None),
                                       C.c_void_p(d_rgba8_ptr or None), C.c_void_p(d_workspace_ptr or None), C.c_void_p(stream)), "rt_tonemap_device")


def log_average_luminance_device(width, height, d_values_ptr: int, spp: int, d_out4_ptr: int, d_workspace_ptr: int, *, d_spp_ptr: int = 0,
                                 delta: float = 1e-4, stream: int = 0):
    """rt_log_average_luminance_device: log_mean, Lavg, count and 0 of a device frame into four device doubles.  Enqueued on `stream`."""
    _check(amd_lib().rt_log_average_luminance_device(width, height, C.c_void_p(d_values_ptr), spp, C.c_void_p(d_spp_ptr or None), delta,
                                                     C.c_void_p(d_out4_ptr), C.c_void_p(d_workspace_ptr), C.c_void_p(stream)),
           "rt_log_average_luminance_device")


def _tonemap_frame(who, values, spp_map):
    import numpy as np
    values = np.ascontiguousarray(values, dtype=np.float64)
    if values.ndim != 3 or values.shape[2] != 3:
        raise RtError(f"{who}: `values` must be an (h, w, 3) frame")
    h, w = values.shape[:2]
    if spp_map is not None:
        spp_map = np.ascontiguousarray(spp_map, dtype=np.int32)
        if spp_map.shape != (h, w):
            raise RtError(f"{who}: `spp_map` must have shape {(h, w)}")
    return values, spp_map, w, h


def tonemap(values, spp, *, spp_map=None, rgba8=False, device=0, **kw):
    """Uploads an (h, w, 3) frame of sums (with `spp`, or an (h, w) int32 spp map) or of means (spp = 1), runs rt_tonemap_device with
    tonemap_params(**kw) and downloads the (h, w, 3) uint8 frame, or (rgb8, (h, w, 4) uint8) with rgba8."""
    values, spp_map, w, h = _tonemap_frame("tonemap", values, spp_map)
    params = tonemap_params(**kw)
    return _frame_end(device, [values, spp_map], (h, w, 3), rgba8 and (h, w, 4), tonemap_workspace_bytes(w, h),
                      lambda d, rgb, ws, rgba, stream: tonemap_device(w, h, d[0], int(spp), d_spp_ptr=d[1], d_rgb8_ptr=rgb, d_rgba8_ptr=rgba,
                                                                      d_workspace_ptr=ws, params=params, stream=stream), out_dtype="uint8")


def log_average_luminance(values, spp, *, spp_map=None, delta=1e-4, device=0):
    """Uploads a frame as tonemap() takes it, runs rt_log_average_luminance_device and downloads (log_mean, Lavg, count, 0.0)."""
    values, spp_map, w, h = _tonemap_frame("log_average_luminance", values, spp_map)
    out4 = _frame_end(device, [values, spp_map], (4,), None, tonemap_workspace_bytes(w, h),
                      lambda d, out, ws, rgba, stream: log_average_luminance_device(w, h, d[0], int(spp), out, ws, d_spp_ptr=d[1], delta=delta,
                                                                                    stream=stream))
    return tuple(float(x) for x in out4)


def tonemap_host(values, spp, *, spp_map=None, rgba8=False, **kw):
    """rth_tonemap (librt_host, CPU): the bytes rt_tonemap_device gives, from the same shared functions and the same reduction tree."""
    import numpy as np
    values, spp_map, w, h = _tonemap_frame("tonemap_host", values, spp_map)
    params = tonemap_params(**kw)
    rgb = np.zeros((h, w, 3), dtype=np.uint8)
    rgba = np.zeros((h, w, 4), dtype=np.uint8) if rgba8 else None
    if host_lib().rth_tonemap(w, h, values.ctypes.data, int(spp), spp_map.ctypes.data if spp_map is not None else None, C.byref(params),
                              rgb.ctypes.data, rgba.ctypes.data if rgba8 else None) != 0:
        raise RtError(host_lib().rth_last_error().decode(errors="replace"))
    return (rgb, rgba) if rgba8 else rgb


def log_average_luminance_host(values, spp, *, spp_map=None, delta=1e-4):
    """rth_log_average_luminance (librt_host, CPU): (log_mean, Lavg, count, 0.0), bit for bit the device's."""
    import numpy as np
    values, spp_map, w, h = _tonemap_frame("log_average_luminance_host", values, spp_map)
    out = np.zeros(4, dtype=np.float64)
    if host_lib().rth_log_average_luminance(w, h, values.ctypes.data, int(spp), spp_map.ctypes.data if spp_map is not None else None, delta,
                                            out.ctypes.data) != 0:
        raise RtError(host_lib().rth_last_error().decode(errors="replace"))
    return tuple(float(x) for x in out)


# frame metrics (include/rt_amd.h "frame metrics")
def _metrics_form(v):
    if isinstance(v, str):
        if v not in METRICS_FORMS:
            raise RtError(f"frame_noise: no form {v!r} (sums, means)")
        return METRICS_FORMS[v]
    return int(v)


def metrics_workspace_bytes(width, height) -> int:
    return _workspace_bytes("rt_metrics_workspace_bytes", f"a {width}x{height} frame", width, height)


def frame_error_device(width, height, d_values_ptr: int, spp: int, d_ref_ptr: int, ref_spp: int, d_out8_ptr: int, d_workspace_ptr: int, *,
                       d_spp_ptr: int = 0, params: "FrameErrorParams | None" = None, stream: int = 0):
    """rt_frame_error_device: count, mse, rmse, rel_mse, mae, bias, max_abs and psnr of a device frame (sums with `spp` or the device map
    d_spp_ptr; means with spp = 1) against a reference frame (sums with ref_spp; means with 1) into eight device doubles, reduced in
    `d_workspace_ptr` (metrics_workspace_bytes(w, h) device bytes).  Enqueued on `stream`."""
    _check(amd_lib().rt_frame_error_device(width, height, C.c_void_p(d_values_ptr or None), spp, C.c_void_p(d_spp_ptr or None),
                                           C.c_void_p(d_ref_ptr or None), ref_spp, C.byref(params) if params is not None else None,
                                           C.c_void_p(d_out8_ptr or None), C.c_void_p(d_workspace_ptr or None), C.c_void_p(stream)),
           "rt_frame_error_device")


def frame_noise_device(width, height, form, d_a_ptr: int, d_b_ptr: int, n: int, d_out4_ptr: int, d_workspace_ptr: int, *, d_spp_ptr: int = 0,
                       params: "FrameNoiseParams | None" = None, stream: int = 0):
    """rt_frame_noise_device: count, mean_var, noise and max_noise of a device frame's moments — form "sums": sums and sums of squares with
    the count `n` or the device map d_spp_ptr; "means": running means and M2 after n samples — into four device doubles, reduced in
    `d_workspace_ptr` (metrics_workspace_bytes(w, h) device bytes).  Enqueued on `stream`."""
    _check(amd_lib().rt_frame_noise_device(width, height, _metrics_form(form), C.c_void_p(d_a_ptr or None), C.c_void_p(d_b_ptr or None), n,
                                           C.c_void_p(d_spp_ptr or None), C.byref(params) if params is not None else None,
                                           C.c_void_p(d_out4_ptr or None), C.c_void_p(d_workspace_ptr or None), C.c_void_p(stream)),
           "rt_frame_noise_device")


def _metrics_frames(who, first, second, spp_map):
    import numpy as np
    first, spp_map, w, h = _tonemap_frame(who, first, spp_map)
    second = np.ascontiguousarray(second, dtype=np.float64)
    if second.shape != first.shape:
        raise RtError(f"{who}: both frames must have shape {first.shape}")
    return first, second, spp_map, w, h


def frame_error(values, spp, ref, ref_spp, *, spp_map=None, device=0, **kw) -> dict:
    """Uploads an (h, w, 3) frame as tonemap() takes it and a reference frame of the same shape (sums with ref_spp, or means with 1), runs
    rt_frame_error_device with frame_error_params(**kw) and downloads the eight values as a dict (FRAME_ERROR_FIELDS; count an int)."""
    values, ref, spp_map, w, h = _metrics_frames("frame_error", values, ref, spp_map)
    params = frame_error_params(**kw)
    out = _frame_end(device, [values, ref, spp_map], (8,), None, metrics_workspace_bytes(w, h),
                     lambda d, out, ws, rgba, stream: frame_error_device(w, h, d[0], int(spp), d[1], int(ref_spp), out, ws, d_spp_ptr=d[2],
                                                                         params=params, stream=stream))
    return _metrics_dict(FRAME_ERROR_FIELDS, out)


def frame_noise(a, b, n, *, form="sums", spp_map=None, device=0, **kw) -> dict:
    """Uploads two (h, w, 3) frames of moments — form "sums": sums and sums of squares with the count n or an (h, w) int32 map; "means":
    running means and M2 after n samples —, runs rt_frame_noise_device with frame_noise_params(**kw) and downloads the four values as a
    dict (FRAME_NOISE_FIELDS; count an int)."""
    a, b, spp_map, w, h = _metrics_frames("frame_noise", a, b, spp_map)
    params, form = frame_noise_params(**kw), _metrics_form(form)
    out = _frame_end(device, [a, b, spp_map], (4,), None, metrics_workspace_bytes(w, h),
                     lambda d, out, ws, rgba, stream: frame_noise_device(w, h, form, d[0], d[1], int(n), out, ws, d_spp_ptr=d[2], params=params,
                                                                         stream=stream))
    return _metrics_dict(FRAME_NOISE_FIELDS, out)


def _metrics_dict(fields, out):
    d = {k: float(x) for k, x in zip(fields, out)}
    d["count"] = int(d["count"])
    return d


def frame_error_host(values, spp, ref, ref_spp, *, spp_map=None, **kw) -> dict:
    """rth_frame_error (librt_host, CPU): the eight values rt_frame_error_device gives, bit for bit."""
    import numpy as np
    values, ref, spp_map, w, h = _metrics_frames("frame_error_host", values, ref, spp_map)
    params = frame_error_params(**kw)
    out = np.zeros(8, dtype=np.float64)
    if host_lib().rth_frame_error(w, h, values.ctypes.data, int(spp), spp_map.ctypes.data if spp_map is not None else None, ref.ctypes.data,
                                  int(ref_spp), C.byref(params), out.ctypes.data) != 0:
        raise RtError(host_lib().rth_last_error().decode(errors="replace"))
    return _metrics_dict(FRAME_ERROR_FIELDS, out)


def frame_noise_host(a, b, n, *, form="sums", spp_map=None, **kw) -> dict:
    """rth_frame_noise (librt_host, CPU): the four values rt_frame_noise_device gives, bit for bit."""
    import numpy as np
    a, b, spp_map, w, h = _metrics_frames("frame_noise_host", a, b, spp_map)
    params = frame_noise_params(**kw)
    out = np.zeros(4, dtype=np.float64)
    if host_lib().rth_frame_noise(w, h, _metrics_form(form), a.ctypes.data, b.ctypes.data, int(n),
                                  spp_map.ctypes.data if spp_map is not None else None, C.byref(params), out.ctypes.data) != 0:
        raise RtError(host_lib().rth_last_error().decode(errors="replace"))
    return _metrics_dict(FRAME_NOISE_FIELDS, out)


# film output (include/rt_amd.h "film output"): the formats, and the (trailing shape, dtype) of a frame in each
RT_FILM_RGBE, RT_FILM_F32, RT_FILM_RGB16 = 0, 1, 2
_FILM_LAYOUT = {RT_FILM_RGBE: ((4,), "uint8"), RT_FILM_F32: ((3,), "float32"), RT_FILM_RGB16: ((3,), "uint16")}


def _film_format(v):
    if isinstance(v, str):
        if v.lower() not in ("rgbe", "f32", "rgb16"):
            raise RtError(f"film: no format {v!r} (rgbe, f32, rgb16)")
        return ("rgbe", "f32", "rgb16").index(v.lower())
    return int(v)


def film_bytes(width, height, format) -> int:
    """rt_film_bytes: the bytes of a w x h frame in `format` (a number or "rgbe" / "f32" / "rgb16"); an RtError where the call refuses."""
    n = int(amd_lib().rt_film_bytes(width, height, _film_format(format)))
    if n < 0:
        raise RtError(f"rt_film_bytes: no {width}x{height} frame in format {format!r}")
    return n


def film_device(width, height, d_values_ptr: int, spp: int, format, d_out_ptr: int, *, d_spp_ptr: int = 0, d_workspace_ptr: int = 0,
                params: "TonemapParams | None" = None, stream: int = 0):
    """rt_film_device: the tone-mapping stage's value over a device frame, as tonemap_device takes it, written in `format` to
    film_bytes(w, h, format) device bytes at d_out_ptr.  With params.auto_key > 0 the exposure comes from the frame's log-average
    luminance, reduced in `d_workspace_ptr` (tonemap_workspace_bytes(w, h) device bytes).  Enqueued on `stream`."""
    _check(amd_lib().rt_film_device(width, height, C.c_void_p(d_values_ptr), spp, C.c_void_p(d_spp_ptr or None),
                                    C.byref(params) if params is not None else None, _film_format(format), C.c_void_p(d_out_ptr or None),
                                    C.c_void_p(d_workspace_ptr or None), C.c_void_p(stream)), "rt_film_device")


def film(values, spp, format, *, spp_map=None, device=0, **kw):
    """Uploads a frame as tonemap() takes it, runs rt_film_device with tonemap_params(**kw) and downloads the frame in `format`:
    (h, w, 4) uint8 R, G, B, E for "rgbe", (h, w, 3) float32 for "f32", (h, w, 3) uint16 for "rgb16"."""
    values, spp_map, w, h = _tonemap_frame("film", values, spp_map)
    params, fmt = tonemap_params(**kw), _film_format(format)
    film_bytes(w, h, fmt)
    tail, dtype = _FILM_LAYOUT[fmt]
    return _frame_end(device, [values, spp_map], (h, w) + tail, None, tonemap_workspace_bytes(w, h),
                      lambda d, out, ws, rgba, stream: film_device(w, h, d[0], int(spp), fmt, out, d_spp_ptr=d[1], d_workspace_ptr=ws, params=params,
                                                                   stream=stream), out_dtype=dtype)


def film_host(values, spp, format, *, spp_map=None, **kw):
    """rth_film (librt_host, CPU): the bytes rt_film_device gives, from the same shared encoders and the same reduction tree."""
    import numpy as np
    values, spp_map, w, h = _tonemap_frame("film_host", values, spp_map)
    params, fmt = tonemap_params(**kw), _film_format(format)
    tail, dtype = _FILM_LAYOUT.get(fmt, ((4,), "uint8"))  # (a format out of range is refused below, by the library)
    out = np.zeros((h, w) + tail, dtype=dtype)
    if host_lib().rth_film(w, h, values.ctypes.data, int(spp), spp_map.ctypes.data if spp_map is not None else None, C.byref(params), fmt,
                           out.ctypes.data) != 0:
        raise RtError(host_lib().rth_last_error().decode(errors="replace"))
    return out


def _write_film(symbol, path, frame, channels, dtype):
    import numpy as np
    frame = np.ascontiguousarray(frame, dtype=dtype)
    if frame.ndim != 3 or frame.shape[2] != channels:
        raise RtError(f"{symbol}: the frame must have shape (h, w, {channels})")
    h, w, _ = frame.shape
    if getattr(host_lib(), symbol)(os.fsencode(path), w, h, frame.ctypes.data) != 0:
        raise RtError(host_lib().rth_last_error().decode(errors="replace"))


def write_hdr(path, rgbe):
    """rth_write_hdr: an (h, w, 4) uint8 frame of R, G, B, E bytes ("rgbe") as a Radiance .hdr picture."""
    _write_film("rth_write_hdr", path, rgbe, 4, "uint8")


def write_pfm(path, rgb_f32):
    """rth_write_pfm: an (h, w, 3) float32 frame ("f32") as a colour PFM."""
    _write_film("rth_write_pfm", path, rgb_f32, 3, "float32")


def read_pfm(path):
    """rth_read_pfm: a colour PFM of either byte order as an (h, w, 3) float64 frame, row 0 on top, each value the file's f32 widened;
    an RtError for a file the reader refuses."""
    import numpy as np
    lib = host_lib()
    w, h = C.c_int32(0), C.c_int32(0)
    if lib.rth_read_pfm(os.fsencode(path), C.byref(w), C.byref(h), None, 0) != 0:
        raise RtError(lib.rth_last_error().decode(errors="replace"))
    out = np.zeros((h.value, w.value, 3), dtype=np.float64)
    if lib.rth_read_pfm(os.fsencode(path), C.byref(w), C.byref(h), out.ctypes.data, out.size) != 0:
        raise RtError(lib.rth_last_error().decode(errors="replace"))
    return out


def write_png16(path, rgb16):
    """rth_write_png16: an (h, w, 3) uint16 frame ("rgb16") as a PNG with 16 bits per sample."""
    _write_film("rth_write_png16", path, rgb16, 3, "uint16")


def bloom_workspace_bytes(width, height) -> int:
    return _workspace_bytes("rt_bloom_workspace_bytes", f"a {width}x{height} frame", width, height)


def bloom_device(width, height, d_values_ptr: int, spp: int, d_mean_out_ptr: int, d_workspace_ptr: int, *, d_spp_ptr: int = 0,
                 params: "BloomParams | None" = None, stream: int = 0):
    """rt_bloom_device: the bright pass, the a-trous levels and the glow added back, over a device frame of 3 w h doubles — sums with the
    uniform sample count `spp` or, if d_spp_ptr is not 0, a device map of w h int32; means with spp = 1 — into the 3 w h doubles of MEANS
    at d_mean_out_ptr, working in `d_workspace_ptr` (bloom_workspace_bytes(w, h) device bytes).  Enqueued on `stream`."""
    _check(amd_lib().rt_bloom_device(width, height, C.c_void_p(d_values_ptr or None), spp, C.c_void_p(d_spp_ptr or None),
                                     C.byref(params) if params is not None else None, C.c_void_p(d_mean_out_ptr or None),
                                     C.c_void_p(d_workspace_ptr or None), C.c_void_p(stream)), "rt_bloom_device")


def bloom(values, spp, *, spp_map=None, device=0, **kw):
    """Uploads an (h, w, 3) frame of sums (with `spp`, or an (h, w) int32 spp map) or of means (spp = 1), runs rt_bloom_device with
    bloom_params(**kw) and downloads the (h, w, 3) float64 frame of bloomed means."""
    values, spp_map, w, h = _tonemap_frame("bloom", values, spp_map)
    params = bloom_params(**kw)
    return _frame_end(device, [values, spp_map], (h, w, 3), None, bloom_workspace_bytes(w, h),
                      lambda d, out, ws, rgba, stream: bloom_device(w, h, d[0], int(spp), out, ws, d_spp_ptr=d[1], params=params, stream=stream))


def bloom_host(values, spp, *, spp_map=None, **kw):
    """rth_bloom (librt_host, CPU): the frame rt_bloom_device gives, bit for bit, from the same shared functions in the same order."""
    import numpy as np
    values, spp_map, w, h = _tonemap_frame("bloom_host", values, spp_map)
    params = bloom_params(**kw)
    out = np.zeros((h, w, 3), dtype=np.float64)
    if host_lib().rth_bloom(w, h, values.ctypes.data, int(spp), spp_map.ctypes.data if spp_map is not None else None, C.byref(params),
                            out.ctypes.data) != 0:
        raise RtError(host_lib().rth_last_error().decode(errors="replace"))
    return out


def robust_device(width, height, blocks, d_stack_ptr: int, spp: int, d_mean_out_ptr: int, *, d_m2_out_ptr: int = 0,
                  params: "RobustParams | None" = None, stream: int = 0):
    """rt_robust_device: the median of means over `blocks` device frames of 3 w h doubles at d_stack_ptr, block after block — sums with
    the uniform per-block count `spp`, or means with spp = 1 — into the 3 w h doubles of MEANS at d_mean_out_ptr and, if d_m2_out_ptr is
    not 0, the winsorised second moments there.  One launch, enqueued on `stream`; no workspace."""
    _check(amd_lib().rt_robust_device(width, height, blocks, C.c_void_p(d_stack_ptr or None), spp, C.byref(params) if params is not None else None,
                                      C.c_void_p(d_mean_out_ptr or None), C.c_void_p(d_m2_out_ptr or None), C.c_void_p(stream)), "rt_robust_device")


def _robust_stack(who, stack):
    import numpy as np
    stack = np.ascontiguousarray(stack, dtype=np.float64)
    if stack.ndim != 4 or stack.shape[3] != 3 or stack.size == 0:
        raise RtError(f"{who}: stack must be (blocks, h, w, 3), not {stack.shape}")
    return stack


def robust(stack, spp, *, m2=False, device=0, **kw):
    """Uploads a (blocks, h, w, 3) stack of sums (with the per-block count `spp`) or of means (spp = 1), runs rt_robust_device with
    robust_params(**kw) and downloads the (h, w, 3) float64 frame of robust means — with m2=True, (mean, m2)."""
    stack = _robust_stack("robust", stack)
    params = robust_params(**kw)
    k, h, w, _ = stack.shape
    import torch
    with torch.cuda.device(device):
        d_stack = torch.from_numpy(stack).cuda()
        d_out = torch.empty((2 if m2 else 1, h, w, 3), dtype=torch.float64, device="cuda")
        robust_device(w, h, k, d_stack.data_ptr(), int(spp), d_out[0].data_ptr(), d_m2_out_ptr=d_out[1].data_ptr() if m2 else 0, params=params,
                      stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
    return (out[0], out[1]) if m2 else out[0]


def robust_host(stack, spp, *, m2=False, **kw):
    """rth_robust (librt_host, CPU): what rt_robust_device gives, bit for bit, from the same per-value body."""
    import numpy as np
    stack = _robust_stack("robust_host", stack)
    params = robust_params(**kw)
    k, h, w, _ = stack.shape
    mean = np.zeros((h, w, 3), dtype=np.float64)
    second = np.zeros((h, w, 3), dtype=np.float64) if m2 else None
    if host_lib().rth_robust(w, h, k, stack.ctypes.data, int(spp), C.byref(params), mean.ctypes.data, second.ctypes.data if m2 else None) != 0:
        raise RtError(host_lib().rth_last_error().decode(errors="replace"))
    return (mean, second) if m2 else mean


def camera_scaled(camera: Camera, factor: int) -> Camera:
    """rt_camera_scaled (GPU-free): the camera of the small frame — ceil(w / factor) x ceil(h / factor) pixels, each covering a
    factor x factor block of `camera`'s."""
    out = Camera()
    _check(amd_lib().rt_camera_scaled(C.byref(camera), int(factor), C.byref(out)), "rt_camera_scaled")
    return out


def cube_face_cameras(like: Camera, center=None, face_size: int = 0, guard: int = 1):
    """rt_camera_cube_faces (GPU-free): a ctypes array of the six square pinhole cameras of a cube map about `center` (None: like's
    centre), faces +X, -X, +Y, -Y, +Z, -Z, each `face_size` pixels wide with `guard` texels beyond the 90 degrees on every side;
    samples_per_pixel, max_depth and background are like's."""
    out = (Camera * 6)()
    c = None if center is None else (C.c_double * 3)(*[float(x) for x in center])
    _check(amd_lib().rt_camera_cube_faces(C.byref(like), c, int(face_size), int(guard), out), "rt_camera_cube_faces")
    return out


def panorama_tables(width, height):
    """rt_panorama_tables (GPU-free): the 2 w + 2 h float64 of a w x h equirectangular frame — (sin, cos) of every column's longitude,
    then of every row's latitude.  Data for panorama_device / panorama_host, reusable for every frame of that size."""
    import numpy as np
    n = 2 * width + 2 * height if width > 0 and height > 0 and width * height < 1 << 27 else 1
    t = np.zeros(n, dtype=np.float64)
    _check(amd_lib().rt_panorama_tables(int(width), int(height), t.ctypes.data), "rt_panorama_tables")
    return t


def panorama_device(width, height, d_tables_ptr: int, d_faces_ptr: int, face_size: int, guard: int, spp: int, d_mean_out_ptr: int, *,
                    stream: int = 0):
    """rt_panorama_device: the six device frames of 3 F F doubles at d_faces_ptr, face after face — sums with the count `spp`, or means
    with spp = 1 — resampled through the device copy of panorama_tables(w, h) at d_tables_ptr into the 3 w h doubles of MEANS at
    d_mean_out_ptr.  One launch, enqueued on `stream`; no workspace."""
    _check(amd_lib().rt_panorama_device(width, height, C.c_void_p(d_tables_ptr or None), C.c_void_p(d_faces_ptr or None), face_size, guard, spp,
                                        C.c_void_p(d_mean_out_ptr or None), C.c_void_p(stream)), "rt_panorama_device")


def _panorama_inputs(who, width, height, faces, tables):
    import numpy as np
    faces = np.ascontiguousarray(faces, dtype=np.float64)
    if faces.ndim != 4 or faces.shape[0] != 6 or faces.shape[1] != faces.shape[2] or faces.shape[3] != 3:
        raise RtError(f"{who}: faces must be (6, F, F, 3), not {faces.shape}")
    tables = panorama_tables(width, height) if tables is None else np.ascontiguousarray(tables, dtype=np.float64)
    if tables.shape != (2 * width + 2 * height,):
        raise RtError(f"{who}: tables must hold 2 * width + 2 * height values")
    return faces, tables


def panorama(width, height, faces, guard, spp, *, tables=None, device=0):
    """Uploads a (6, F, F, 3) stack of cube faces (sums with the count `spp`, or means with spp = 1) and the tables (None:
    panorama_tables(width, height)), runs rt_panorama_device and downloads the (height, width, 3) float64 frame of means."""
    faces, tables = _panorama_inputs("panorama", width, height, faces, tables)
    F = faces.shape[1]
    return _frame_end(device, [tables, faces], (height, width, 3), None, 0,
                      lambda d, out, ws, rgba, stream: panorama_device(width, height, d[0], d[1], F, int(guard), int(spp), out, stream=stream))


def panorama_host(width, height, faces, guard, spp, *, tables=None):
    """rth_panorama (librt_host, CPU): what rt_panorama_device gives, bit for bit, from the same per-pixel body and the same tables."""
    import numpy as np
    faces, tables = _panorama_inputs("panorama_host", width, height, faces, tables)
    out = np.zeros((height, width, 3), dtype=np.float64)
    if host_lib().rth_panorama(width, height, tables.ctypes.data, faces.ctypes.data, faces.shape[1], int(guard), int(spp), out.ctypes.data) != 0:
        raise RtError(host_lib().rth_last_error().decode(errors="replace"))
    return out


def upsample_workspace_bytes(width, height, factor) -> int:
    return _workspace_bytes("rt_upsample_workspace_bytes", f"a {width}x{height} frame at factor {factor}", width, height, factor)


def upsample_device(width, height, d_low_ptr: int, spp: int, d_mean_out_ptr: int, d_workspace_ptr: int, *, d_albedo_sum_ptr: int = 0,
                    albedo_spp: int = 0, d_edge_sum_ptr: int = 0, edge_spp: int = 0, d_rgba8_ptr: int = 0,
                    params: "UpsampleParams | None" = None, stream: int = 0):
    """rt_upsample_device: the low device frame at d_low_ptr (3 lw lh doubles, lw = ceil(width / factor): sums with the count `spp`, or
    means with spp = 1) brought to the FULL size width x height under the full-size guide frames given (3 w h doubles of sums each, with
    their counts), into the 3 w h doubles at d_mean_out_ptr and, if d_rgba8_ptr is not 0, 4 w h display bytes; `d_workspace_ptr`:
    upsample_workspace_bytes(w, h, factor) device bytes.  Enqueued on `stream`."""
    _check(amd_lib().rt_upsample_device(width, height, C.c_void_p(d_low_ptr or None), spp, C.c_void_p(d_albedo_sum_ptr or None), albedo_spp,
                                        C.c_void_p(d_edge_sum_ptr or None), edge_spp, C.byref(params) if params is not None else None,
                                        C.c_void_p(d_mean_out_ptr or None), C.c_void_p(d_rgba8_ptr or None), C.c_void_p(d_workspace_ptr or None),
                                        C.c_void_p(stream)), "rt_upsample_device")


def _upsample_frames(who, low, size, factor, albedo_sum, edge_sum):
    import numpy as np
    w, h = int(size[0]), int(size[1])
    low = np.ascontiguousarray(low, dtype=np.float64)
    if w < 1 or h < 1 or factor < 1:
        raise RtError(f"{who}: the full size and the factor must be positive")
    lw, lh = (w + factor - 1) // factor, (h + factor - 1) // factor
    if low.shape != (lh, lw, 3):
        raise RtError(f"{who}: `low` must be an ({lh}, {lw}, 3) frame for a {w}x{h} frame at factor {factor}")
    guides = []
    for name, g in (("albedo_sum", albedo_sum), ("edge_sum", edge_sum)):
        if g is not None:
            g = np.ascontiguousarray(g, dtype=np.float64)
            if g.shape != (h, w, 3):
                raise RtError(f"{who}: `{name}` must be an ({h}, {w}, 3) frame")
        guides.append(g)
    return low, guides[0], guides[1], w, h


def upsample(low, spp, size, *, albedo_sum=None, albedo_spp=0, edge_sum=None, edge_spp=0, rgba8=False, device=0, **kw):
    """Uploads the low (lh, lw, 3) frame (sums with `spp`, or means with spp = 1) and the full-size (h, w, 3) guide frames of sums given,
    runs rt_upsample_device with upsample_params(**kw) for the full size `size` = (w, h) and downloads: the (h, w, 3) float64 frame, or
    (frame, (h, w, 4) uint8) with rgba8."""
    params = upsample_params(**kw)
    low, albedo_sum, edge_sum, w, h = _upsample_frames("upsample", low, size, params.factor, albedo_sum, edge_sum)
    return _frame_end(device, [low, albedo_sum, edge_sum], (h, w, 3), rgba8 and (h, w, 4), upsample_workspace_bytes(w, h, params.factor),
                      lambda d, out, ws, rgba, stream: upsample_device(w, h, d[0], int(spp), out, ws, d_albedo_sum_ptr=d[1], albedo_spp=int(albedo_spp),
                                                                       d_edge_sum_ptr=d[2], edge_spp=int(edge_spp), d_rgba8_ptr=rgba, params=params,
                                                                       stream=stream))


def upsample_host(low, spp, size, *, albedo_sum=None, albedo_spp=0, edge_sum=None, edge_spp=0, rgba8=False, **kw):
    """rth_upsample (librt_host, CPU): what rt_upsample_device gives, bit for bit, from the same shared functions in the same order."""
    import numpy as np
    params = upsample_params(**kw)
    low, albedo_sum, edge_sum, w, h = _upsample_frames("upsample_host", low, size, params.factor, albedo_sum, edge_sum)
    out = np.zeros((h, w, 3), dtype=np.float64)
    rgba = np.zeros((h, w, 4), dtype=np.uint8) if rgba8 else None
    if host_lib().rth_upsample(w, h, low.ctypes.data, int(spp), albedo_sum.ctypes.data if albedo_sum is not None else None, int(albedo_spp),
                               edge_sum.ctypes.data if edge_sum is not None else None, int(edge_spp), C.byref(params), out.ctypes.data,
                               rgba.ctypes.data if rgba8 else None) != 0:
        raise RtError(host_lib().rth_last_error().decode(errors="replace"))
    return (out, rgba) if rgba8 else out


def tiles_to_frame_rgb8_device(width, height, shard_count, d_gathered_ptr: int, d_frame_ptr: int, stream: int = 0):
    _check(amd_lib().rt_tiles_to_frame_rgb8_device(width, height, shard_count, C.c_void_p(d_gathered_ptr),
                                                   C.c_void_p(d_frame_ptr), C.c_void_p(stream)),
           "rt_tiles_to_frame_rgb8_device")


class Comm:
    """rt_comm: one RCCL communicator handle of this rank (include/rt_amd.h "frame-end gather")."""

    def __init__(self, handle):
        self._handle = handle

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * RT_COMM_ID_BYTES)()
        _check(amd_lib().rt_comm_get_unique_id(buf), "rt_comm_get_unique_id")
        return bytes(buf)

    @classmethod
    def create(cls, unique_id: bytes, rank: int, n_ranks: int, device: int) -> "Comm":
        assert len(unique_id) == RT_COMM_ID_BYTES
        buf = (C.c_uint8 * RT_COMM_ID_BYTES).from_buffer_copy(unique_id)
        h = C.c_void_p()
        _check(amd_lib().rt_comm_create(buf, rank, n_ranks, device, C.byref(h)), "rt_comm_create")
        return cls(h)

    rank = property(lambda self: amd_lib().rt_comm_rank(self._handle))
    size = property(lambda self: amd_lib().rt_comm_size(self._handle))

    def gather_tiles(self, width, height, elem_bytes, d_tiles_ptr: int, d_gathered_ptr: int, root: int = 0, stream: int = 0):
        _check(amd_lib().rt_gather_tiles_device(self._handle, width, height, elem_bytes, C.c_void_p(d_tiles_ptr),
                                                C.c_void_p(d_gathered_ptr), root, C.c_void_p(stream)), "rt_gather_tiles_device")

    def close(self):
        if getattr(self, "_handle", None):
            amd_lib().rt_comm_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def resolve_rgb8_host(width, height, spp, sums):
    """color_to_rgb(sum / spp) on the host (librt_host; src/renderer.rs:55-58)."""
    import numpy as np
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    out = np.zeros(width * height * 3, dtype=np.uint8)
    if host_lib().rth_resolve_rgb8(width, height, spp, sums.ctypes.data_as(C.POINTER(C.c_double)),
                                   out.ctypes.data_as(C.POINTER(C.c_uint8))) != 0:
        raise RtError(host_lib().rth_last_error().decode(errors="replace"))
    return out.reshape(height, width, 3)


def write_png(path, rgb8):
    import numpy as np
    rgb8 = np.ascontiguousarray(rgb8, dtype=np.uint8)
    h, w, _ = rgb8.shape
    if host_lib().rth_write_png(os.fsencode(path), w, h, rgb8.ctypes.data_as(C.POINTER(C.c_uint8))) != 0:
        raise RtError(host_lib().rth_last_error().decode(errors="replace"))
