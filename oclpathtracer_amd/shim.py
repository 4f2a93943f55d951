"""ctypes binding of libptshim.so -- the C ABI declared in include/pt_shim.h.

This is the only way Python reaches the hot path; there is no Python/NumPy/torch fallback.
If the library is missing, ``load()`` raises: build it with ``__graft_entry__.build()``
(``make -C oclpathtracer_amd/csrc``).
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PT_SHIM_LIB lets an experiment point at an alternative build of the same ABI (A/B kernel variants)
LIB_PATH = os.environ.get("PT_SHIM_LIB") or os.path.join(_HERE, "libptshim.so")

PT_OK = 0
PT_ERR_INVALID, PT_ERR_NO_DEVICE, PT_ERR_OOM, PT_ERR_HIP, PT_ERR_NOT_FOUND, PT_ERR_ARGS, PT_ERR_RANGE, PT_ERR_TRAVERSAL = range(1, 9)
PT_INFO_NAME, PT_INFO_BOARD, PT_INFO_VENDOR, PT_INFO_VERSION = range(4)
PT_OPT_BATCH_FRAMES, PT_OPT_CHUNK_FRAMES, PT_OPT_PROFILE_RETURN_TIME = 0, 1, 2   # (3 is not assigned)
PT_OPT_QUAD_FILTER, PT_OPT_ACCEL, PT_OPT_BVH_TALLY, PT_OPT_PRIMARY_MASKS, PT_OPT_BVH_STACK_LIMIT, PT_OPT_RENDER_LANES, PT_OPT_CHECKPOINT, PT_OPT_BVH_BUILD_COUNT = 4, 5, 6, 7, 8, 9, 10, 11
PT_OPT_SECONDARY_MASKS = 12
PT_OPT_DENOISE_TILE = 13   # pt_denoise: 0 = auto, 1 = global gathers, 2 = an LDS halo tile at steps 1 and 2 (identical bits)
PT_OPT_REPROJECT_FORM = 14   # pt_reproject: 0 = auto, 1 = one kernel over the records, 2 = a prepare pass first (identical bits)
PT_OPT_DENOISE_SPATIAL_FORM = 15   # pt_denoise_spatial's pool pass: 0 = auto, 1 = global gathers, 2 = an LDS tile with halo 3 (identical bits)
PT_SHIM_ABI_VERSION = 2  # include/pt_shim.h; load() refuses a library of another version
PT_MAX_ARG_SIZE = 64
PT_MAX_ARG_COUNT = 64
PT_STAT_SAMPLES, PT_STAT_RAYS, PT_STAT_WORDS = 0, 1, 16
PT_STAT_BVH_NODES, PT_STAT_BVH_TRIS, PT_STAT_BVH_STEPS, PT_STAT_BVH_TRI_STEPS, PT_STAT_BVH_MAX_STACK, PT_STAT_CARRIED, PT_STAT_BVH_GRAZING = 2, 3, 4, 5, 6, 7, 8
PT_PROF_TRACE, PT_PROF_FOLD = 0, 1
PT_STREAM_LEGACY = 1  # hipStreamLegacy: how a caller names the legacy default stream to pt_device_set_stream
PT_QUERY_CLOSEST, PT_QUERY_OCCLUDED = 0, 1  # pt_intersect_rays modes

_c = ctypes
_H = _c.c_void_p  # opaque handles


class LaunchArg(_c.Structure):
    """pt_launch_arg (mirrors Launcher::Args, Adl/AdlKernel.h:133-140)."""

    _fields_ = [
        ("is_buffer", _c.c_int32),
        ("read_only", _c.c_int32),
        ("size", _c.c_uint64),
        ("buffer", _H),
        ("data", _c.c_ubyte * PT_MAX_ARG_SIZE),
    ]


class RenderParams(_c.Structure):
    """pt_render_params."""

    _fields_ = [
        ("width", _c.c_int32), ("height", _c.c_int32),
        ("frame_begin", _c.c_int32), ("frame_count", _c.c_int32),
        ("max_bounces", _c.c_int32), ("num_triangles", _c.c_int32), ("num_materials", _c.c_int32),
        ("stripe_rows", _c.c_int32), ("n_ranks", _c.c_int32), ("rank", _c.c_int32),
        ("reserved", _c.c_int32 * 6),
    ]


class _CameraLens(_c.Structure):
    _fields_ = [("lens_radius", _c.c_float), ("focus_distance", _c.c_float)]


class _CameraTail(_c.Union):
    """the six trailing words of pt_camera: the thin lens' two floats laid over the first two of ``reserved``"""

    _anonymous_ = ("lens",)
    _fields_ = [("lens", _CameraLens), ("reserved", _c.c_int32 * 6)]


class Camera(_c.Structure):
    """pt_camera (64 bytes): eye, center, up, vertical field of view in degrees; the thin lens (``lens_radius``, ``focus_distance``:
    offsets 40 and 44, both 0 = the pinhole) and four reserved words, which must be 0.  ``reserved`` is the view of all six trailing
    words, as before the lens: ``reserved[0]`` and ``reserved[1]`` are the bits of the two floats."""

    _anonymous_ = ("tail",)
    _fields_ = [
        ("eye", _c.c_float * 3), ("center", _c.c_float * 3), ("up", _c.c_float * 3),
        ("fov_y_deg", _c.c_float),
        ("tail", _CameraTail),
    ]


class Ray(_c.Structure):
    """pt_ray (32 bytes): the arguments of getRay -- origin, tmax (a hit counts at 0 < t < min(tmax, 1e20)), direction (any
    length; normalised on the device as getRay does), reserved."""

    _fields_ = [("origin", _c.c_float * 3), ("tmax", _c.c_float), ("dir", _c.c_float * 3), ("reserved", _c.c_int32)]


class Hit(_c.Structure):
    """pt_hit (48 bytes): t, triangle, u, v | hit point, material | normal, reserved.  A miss: t = +inf, tri = -1."""

    _fields_ = [
        ("t", _c.c_float), ("tri", _c.c_int32), ("u", _c.c_float), ("v", _c.c_float),
        ("p", _c.c_float * 3), ("material", _c.c_int32),
        ("n", _c.c_float * 3), ("reserved", _c.c_int32),
    ]


class AoParams(_c.Structure):
    """pt_ao_params (64 bytes): image, frames, triangles, K occlusion rays per hit, their radius, the value of a pixel never hit,
    image sharding as RenderParams; reserved must be 0."""

    _fields_ = [
        ("width", _c.c_int32), ("height", _c.c_int32),
        ("frame_begin", _c.c_int32), ("frame_count", _c.c_int32),
        ("num_triangles", _c.c_int32), ("rays_per_sample", _c.c_int32),
        ("radius", _c.c_float), ("miss_value", _c.c_float),
        ("stripe_rows", _c.c_int32), ("n_ranks", _c.c_int32), ("rank", _c.c_int32),
        ("reserved", _c.c_int32 * 5),
    ]


class DirectParams(_c.Structure):
    """pt_direct_params (64 bytes): image, frames, triangles, materials, lights in the list, K light samples per hit, image
    sharding as RenderParams; reserved must be 0."""

    _fields_ = [
        ("width", _c.c_int32), ("height", _c.c_int32),
        ("frame_begin", _c.c_int32), ("frame_count", _c.c_int32),
        ("num_triangles", _c.c_int32), ("num_materials", _c.c_int32), ("num_lights", _c.c_int32),
        ("light_samples", _c.c_int32),
        ("stripe_rows", _c.c_int32), ("n_ranks", _c.c_int32), ("rank", _c.c_int32),
        ("reserved", _c.c_int32 * 5),
    ]


PT_FEATURE_ALBEDO, PT_FEATURE_NORMAL, PT_FEATURE_DEPTH, PT_FEATURE_EMISSION = 1, 2, 4, 8


class FeatureParams(_c.Structure):
    """pt_feature_params (64 bytes): image, frames (frame_begin only numbers them), triangles, materials, image sharding as
    RenderParams; reserved must be 0."""

    _fields_ = [
        ("width", _c.c_int32), ("height", _c.c_int32),
        ("frame_begin", _c.c_int32), ("frame_count", _c.c_int32),
        ("num_triangles", _c.c_int32), ("num_materials", _c.c_int32),
        ("stripe_rows", _c.c_int32), ("n_ranks", _c.c_int32), ("rank", _c.c_int32),
        ("reserved", _c.c_int32 * 7),
    ]


class IndirectParams(_c.Structure):
    """pt_indirect_params (64 bytes): DirectParams' fields (K light samples per vertex) and the path's depth max_bounces; reserved
    must be 0."""

    _fields_ = [
        ("width", _c.c_int32), ("height", _c.c_int32),
        ("frame_begin", _c.c_int32), ("frame_count", _c.c_int32),
        ("num_triangles", _c.c_int32), ("num_materials", _c.c_int32), ("num_lights", _c.c_int32),
        ("light_samples", _c.c_int32),
        ("stripe_rows", _c.c_int32), ("n_ranks", _c.c_int32), ("rank", _c.c_int32),
        ("max_bounces", _c.c_int32),
        ("reserved", _c.c_int32 * 4),
    ]


class BvhInfo(_c.Structure):
    """pt_bvh_info (64 bytes): what pt_bvh_snapshot says about the LBVH of the prepared scene."""

    _fields_ = [
        ("records", _c.c_uint32), ("num_big", _c.c_int32), ("num_triangles", _c.c_int32),
        ("grid_min", _c.c_float * 3), ("grid_step", _c.c_float * 3),
        ("reserved", _c.c_int32 * 7),
    ]


PT_BVH_SNAPSHOT_BIG_MAX = 64


class Roulette(_c.Structure):
    """pt_roulette (16 bytes): the Russian roulette of pt_render_indirect_rr -- played from vertex first_bounce on (counted from 1), with
    survival probability min(largest channel of the throughput, max_survival); reserved must be 0."""

    _fields_ = [("first_bounce", _c.c_int32), ("max_survival", _c.c_float), ("reserved", _c.c_int32 * 2)]


NO_ROULETTE = Roulette(65535, 1.0)   # what an entry point that takes a pt_roulette gets for none: a first bounce no path reaches


class Ris(_c.Structure):
    """pt_ris (16 bytes): resampled light sampling -- candidates (M, 1 .. 32) drawn from the light table per light sample, one of which
    is kept in proportion to its unshadowed contribution; reserved must be 0."""

    _fields_ = [("candidates", _c.c_int32), ("reserved", _c.c_int32 * 3)]


class Environment(_c.Structure):
    """pt_environment (16 bytes): the octahedral sky map of pt_render_direct_env / pt_render_indirect_env -- size (N, a power of two in
    1 .. 2048) and env_samples (Ke, 0 .. 256, per vertex); reserved must be 0."""

    _fields_ = [("size", _c.c_int32), ("env_samples", _c.c_int32), ("reserved", _c.c_int32 * 2)]


class RadianceParams(_c.Structure):
    """pt_radiance_params (64 bytes): the rays (their number, the id of the first), the sample range of every ray, the scene's counts
    and K as IndirectParams, the path's depth, reset != 0 = the moments start from zeros; reserved must be 0."""

    _fields_ = [
        ("num_rays", _c.c_uint32), ("first_ray", _c.c_uint32),
        ("sample_begin", _c.c_int32), ("sample_count", _c.c_int32),
        ("num_triangles", _c.c_int32), ("num_materials", _c.c_int32), ("num_lights", _c.c_int32),
        ("light_samples", _c.c_int32),
        ("max_bounces", _c.c_int32), ("reset", _c.c_int32),
        ("reserved", _c.c_int32 * 6),
    ]


assert _c.sizeof(RadianceParams) == 64


class PixelMoments(_c.Structure):
    """pt_pixel_moments (56 bytes): per channel the sum and the sum of squares of a pixel's finite samples, their number, and the
    number of samples rejected for a NaN or an infinity."""

    _fields_ = [("sum", _c.c_double * 3), ("sum2", _c.c_double * 3), ("n", _c.c_uint32), ("rejected", _c.c_uint32)]


# the same record for numpy: what every reader of a moments buffer decodes it through
MOMENTS_DTYPE = np.dtype([("sum", np.float64, 3), ("sum2", np.float64, 3), ("n", np.uint32), ("rejected", np.uint32)])
assert MOMENTS_DTYPE.itemsize == _c.sizeof(PixelMoments) == 56


class NoiseSummary(_c.Structure):
    """pt_noise_summary (48 bytes): the first record of pt_moments_resolve's summary buffer."""

    _fields_ = [("var_sum", _c.c_double), ("se2_sum", _c.c_double), ("mean2_sum", _c.c_double),
                ("pixels", _c.c_uint64), ("samples", _c.c_uint64), ("rejected", _c.c_uint64)]

class AdaptiveRule(_c.Structure):
    """pt_adaptive_rule (32 bytes): a pixel is listed while it has received fewer than max_samples samples and has fewer than
    min_samples finite ones or a squared standard error of its mean above tol2 * (its squared mean + floor2); reserved must be 0."""

    _fields_ = [("tol2", _c.c_double), ("floor2", _c.c_double), ("min_samples", _c.c_uint32), ("max_samples", _c.c_uint32),
                ("reserved", _c.c_uint32 * 2)]


class PixelSlot(_c.Structure):
    """pt_pixel_slot (8 bytes): a local pixel and the number of its next frame.  A list is 16 bytes {count, reserved[3]}, then slots."""

    _fields_ = [("pixel", _c.c_uint32), ("frame", _c.c_uint32)]


PT_PIXEL_LIST_HEADER = 16


class DenoiseParams(_c.Structure):
    """pt_denoise_params (64 bytes): the whole image, the a-trous levels (0 .. 8; level i has step 1 << i), the squarings of the normal
    weight (0 .. 8), the four sigmas and the two eps (finite, > 0); reserved must be 0."""

    _fields_ = [
        ("width", _c.c_int32), ("height", _c.c_int32), ("levels", _c.c_int32), ("normal_squarings", _c.c_int32),
        ("sigma_l", _c.c_float), ("sigma_z", _c.c_float), ("sigma_a", _c.c_float), ("sigma_e", _c.c_float),
        ("eps_l", _c.c_float), ("eps_z", _c.c_float),
        ("reserved", _c.c_int32 * 6),
    ]


assert _c.sizeof(DenoiseParams) == 64


class DenoiseSpatialParams(_c.Structure):
    """pt_denoise_spatial_params (32 bytes): a pixel with 1 <= n < below takes the pooled variance of its 7 x 7 neighbourhood (>= 0;
    0 and 1 name no pixel); reserved must be 0."""

    _fields_ = [("below", _c.c_int32), ("reserved", _c.c_int32 * 7)]


assert _c.sizeof(DenoiseSpatialParams) == 32


class ReprojectParams(_c.Structure):
    """pt_reproject_params (64 bytes): the whole image, the cap on the history length taken over (>= 0), the relative depth tolerance
    (finite, > 0), the least cosine between the mean normals (in [0, 1]), the least sum of surviving bilinear weights (in [0, 1)) and
    the largest squared relative standard error of a tap's mean (finite, >= 0; 0 = no noise test); reserved must be 0."""

    _fields_ = [
        ("width", _c.c_int32), ("height", _c.c_int32), ("max_history", _c.c_int32),
        ("tol_z", _c.c_float), ("cos_min", _c.c_float), ("min_weight", _c.c_float), ("max_noise", _c.c_float),
        ("reserved", _c.c_int32 * 9),
    ]


assert _c.sizeof(ReprojectParams) == 64

# every symbol include/pt_shim.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "pt_last_error": (_c.c_char_p, []),
    "pt_abi_version": (_c.c_int, []),
    "pt_init": (_c.c_int, []),
    "pt_quit": (None, []),
    "pt_device_count": (_c.c_int, []),
    "pt_device_create": (_c.c_int, [_c.c_int, _c.POINTER(_H)]),
    "pt_device_destroy": (_c.c_int, [_H]),
    "pt_device_info": (_c.c_int, [_H, _c.c_int, _c.c_char_p]),
    "pt_device_max_alloc": (_c.c_uint64, [_H]),
    "pt_device_mem_size": (_c.c_uint64, [_H]),
    "pt_device_used_memory": (_c.c_uint64, [_H]),
    "pt_device_peak_memory": (_c.c_uint64, [_H]),
    "pt_device_workspace_memory": (_c.c_uint64, [_H]),
    "pt_device_reserve_staging": (_c.c_int, [_H, _c.c_size_t]),
    "pt_device_num_cus": (_c.c_int, [_H]),
    "pt_device_set_stream": (_c.c_int, [_H, _c.c_void_p]),
    "pt_device_get_stream": (_c.c_void_p, [_H]),
    "pt_device_wait_stream": (_c.c_int, [_H, _c.c_void_p]),
    "pt_device_wait_hip_event": (_c.c_int, [_H, _c.c_void_p]),
    "pt_event_wait_on": (_c.c_int, [_H, _c.c_void_p]),
    "pt_sync": (_c.c_int, [_H]),
    "pt_flush": (_c.c_int, [_H]),
    "pt_device_set_option": (_c.c_int, [_H, _c.c_int, _c.c_int64]),
    "pt_device_get_option": (_c.c_int64, [_H, _c.c_int]),
    "pt_buffer_alloc": (_c.c_int, [_H, _c.c_size_t, _c.POINTER(_H)]),
    "pt_buffer_wrap": (_c.c_int, [_H, _c.c_void_p, _c.c_size_t, _c.POINTER(_H)]),
    "pt_buffer_free": (_c.c_int, [_H]),
    "pt_buffer_size": (_c.c_size_t, [_H]),
    "pt_buffer_device_ptr": (_c.c_void_p, [_H]),
    "pt_buffer_address": (_c.c_void_p, [_H]),
    "pt_buffer_write": (_c.c_int, [_H, _c.c_void_p, _c.c_size_t, _c.c_size_t, _H]),
    "pt_buffer_read": (_c.c_int, [_H, _c.c_void_p, _c.c_size_t, _c.c_size_t, _H]),
    "pt_buffer_copy": (_c.c_int, [_H, _H, _c.c_size_t, _c.c_size_t, _c.c_size_t, _H]),
    "pt_buffer_map": (_c.c_void_p, [_H, _c.c_size_t, _c.c_int]),
    "pt_buffer_unmap": (_c.c_int, [_H, _c.c_void_p]),
    "pt_host_alloc": (_c.c_int, [_c.c_size_t, _c.POINTER(_c.c_void_p)]),
    "pt_host_free": (_c.c_int, [_c.c_void_p]),
    "pt_event_create": (_c.c_int, [_H, _c.POINTER(_H)]),
    "pt_event_destroy": (_c.c_int, [_H]),
    "pt_event_wait": (_c.c_int, [_H]),
    "pt_event_is_complete": (_c.c_int, [_H]),
    "pt_event_elapsed_ns": (_c.c_int, [_H, _c.POINTER(_c.c_uint64)]),
    "pt_kernel_get": (_c.c_int, [_H, _c.c_char_p, _c.c_char_p, _c.POINTER(_H)]),
    "pt_launch_2d": (_c.c_int, [_H, _H, _c.POINTER(LaunchArg), _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _H,
                                _c.POINTER(_c.c_float)]),
    "pt_local_rows": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "pt_render_frames": (_c.c_int, [_H, _H, _H, _H, _c.POINTER(RenderParams), _H, _H]),
    "pt_camera_reference": (None, [_c.POINTER(Camera)]),
    "pt_camera_derive": (_c.c_int, [_c.POINTER(Camera), _c.POINTER(_c.c_float)]),
    "pt_render_frames_camera": (_c.c_int, [_H, _H, _H, _H, _c.POINTER(RenderParams), _c.POINTER(Camera), _H, _H]),
    "pt_intersect_rays": (_c.c_int, [_H, _H, _c.c_int, _H, _H, _c.c_size_t, _c.c_int, _H]),
    "pt_camera_rays": (_c.c_int, [_H, _c.POINTER(Camera), _c.c_int, _c.c_int, _c.c_int, _H, _H]),
    "pt_occluded_rays": (_c.c_int, [_H, _H, _c.c_int, _H, _H, _c.c_size_t, _H]),
    "pt_render_ao": (_c.c_int, [_H, _H, _H, _H, _c.POINTER(AoParams), _c.POINTER(Camera), _H]),
    "pt_render_direct": (_c.c_int, [_H, _H, _H, _H, _H, _H, _c.POINTER(DirectParams), _c.POINTER(Camera), _H]),
    "pt_render_features": (_c.c_int, [_H, _H, _H, _H, _H, _H, _H, _c.POINTER(FeatureParams), _c.POINTER(Camera), _H]),
    "pt_render_indirect": (_c.c_int, [_H, _H, _H, _H, _H, _H, _c.POINTER(IndirectParams), _c.POINTER(Camera), _H]),
    "pt_light_counts": (_c.c_int, [_H, _H, _c.c_int, _c.c_int, _H, _H]),
    "pt_render_indirect_mis": (_c.c_int, [_H, _H, _H, _H, _H, _H, _H, _c.POINTER(IndirectParams), _c.POINTER(Camera), _H]),
    "pt_light_table_bytes": (_c.c_size_t, [_c.c_int]),
    "pt_light_table": (_c.c_int, [_H, _H, _c.c_int, _H, _c.c_int, _H, _c.c_int, _H, _H, _H]),
    "pt_render_direct_power": (_c.c_int, [_H, _H, _H, _H, _H, _H, _H, _H, _c.POINTER(DirectParams), _c.POINTER(Camera), _H]),
    "pt_render_indirect_power": (_c.c_int, [_H, _H, _H, _H, _c.c_int, _H, _H, _H, _H, _H, _c.POINTER(IndirectParams), _c.POINTER(Camera), _H]),
    "pt_render_indirect_rr": (_c.c_int, [_H, _H, _H, _H, _c.c_int, _H, _H, _H, _H, _H, _c.POINTER(IndirectParams), _c.POINTER(Roulette),
                                         _c.POINTER(Camera), _H]),
    "pt_sample_moments": (_c.c_int, [_H, _H, _H, _c.c_uint32, _c.c_int32, _c.c_int, _H]),
    "pt_moments_summary_bytes": (_c.c_size_t, [_c.c_uint32]),
    "pt_moments_resolve": (_c.c_int, [_H, _H, _c.c_uint32, _H, _H, _H]),
    "pt_adaptive_list_bytes": (_c.c_size_t, [_c.c_uint32]),
    "pt_adaptive_select": (_c.c_int, [_H, _H, _c.c_uint32, _c.POINTER(AdaptiveRule), _H, _H]),
    "pt_render_indirect_pixels": (_c.c_int, [_H, _H, _H, _H, _c.c_int, _H, _H, _H, _H, _H, _H, _c.c_uint32, _c.POINTER(IndirectParams),
                                             _c.POINTER(Roulette), _c.POINTER(Camera), _H]),
    "pt_render_direct_ris": (_c.c_int, [_H, _H, _H, _H, _H, _H, _H, _H, _c.POINTER(DirectParams), _c.POINTER(Ris), _c.POINTER(Camera), _H]),
    "pt_render_indirect_ris": (_c.c_int, [_H, _H, _H, _H, _c.c_int, _H, _H, _H, _H, _H, _c.POINTER(IndirectParams), _c.POINTER(Roulette),
                                          _c.POINTER(Ris), _c.POINTER(Camera), _H]),
    "pt_render_indirect_pixels_ris": (_c.c_int, [_H, _H, _H, _H, _c.c_int, _H, _H, _H, _H, _H, _H, _c.c_uint32, _c.POINTER(IndirectParams),
                                                 _c.POINTER(Roulette), _c.POINTER(Ris), _c.POINTER(Camera), _H]),
    "pt_sample_moments_pixels": (_c.c_int, [_H, _H, _H, _H, _c.c_uint32, _c.c_int32, _H]),
    "pt_env_table_bytes": (_c.c_size_t, [_c.c_int]),
    "pt_env_table": (_c.c_int, [_H, _H, _c.c_int, _H, _H]),
    "pt_render_direct_env": (_c.c_int, [_H, _H, _H, _H, _H, _H, _H, _H, _H, _H, _c.POINTER(DirectParams), _c.POINTER(Environment),
                                        _c.POINTER(Camera), _H]),
    "pt_render_indirect_env": (_c.c_int, [_H, _H, _H, _H, _H, _H, _H, _H, _H, _H, _H, _c.POINTER(IndirectParams), _c.POINTER(Roulette),
                                          _c.POINTER(Environment), _c.POINTER(Camera), _H]),
    "pt_radiance_rays": (_c.c_int, [_H, _H, _H, _H, _c.c_int, _H, _H, _H, _H, _H, _H, _c.POINTER(RadianceParams), _c.POINTER(Roulette), _H]),
    "pt_denoise_scratch_bytes": (_c.c_size_t, [_c.c_int32, _c.c_int32]),
    "pt_denoise": (_c.c_int, [_H, _H, _H, _H, _H, _H, _H, _H, _c.POINTER(DenoiseParams), _H]),
    "pt_denoise_spatial": (_c.c_int, [_H, _H, _H, _H, _H, _H, _H, _H, _c.POINTER(DenoiseParams), _c.POINTER(DenoiseSpatialParams), _H]),
    "pt_reproject_scratch_bytes": (_c.c_size_t, [_c.c_int32, _c.c_int32]),
    "pt_reproject": (_c.c_int, [_H, _H, _H, _H, _H, _H, _H, _H, _H, _c.POINTER(ReprojectParams), _c.POINTER(Camera), _c.POINTER(Camera), _H]),
    "pt_profile_enable": (_c.c_int, [_H, _c.c_int]),
    "pt_profile_query": (_c.c_int, [_H, _c.c_int, _c.POINTER(_c.c_double), _c.POINTER(_c.c_uint64)]),
    "pt_bvh_snapshot": (_c.c_int, [_H, _c.POINTER(BvhInfo), _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "pt_primary_mask_snapshot": (_c.c_int, [_H, _c.POINTER(_c.c_uint32), _c.c_void_p, _c.c_size_t]),
    "pt_secondary_mask_snapshot": (_c.c_int, [_H, _c.POINTER(_c.c_uint32), _c.c_void_p, _c.c_size_t]),
    "pt_profile_query_union": (_c.c_int, [_H, _c.c_int, _c.POINTER(_c.c_double)]),
    "pt_profile_reset": (_c.c_int, [_H]),
    "pt_assemble_stripes": (_c.c_int, [_H, _H, _H, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _H]),
    "pt_assemble_stripes_on": (_c.c_int, [_H, _H, _H, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p]),
    "pt_tonemap_ppm": (_c.c_int, [_H, _H, _H, _c.c_size_t, _H]),
}


class ShimError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__("pt_shim error %d: %s" % (code, message))
        self.code = code


_lib = None


def load():
    """Load libptshim.so and declare every entry point.  Raises if the library is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ShimError(PT_ERR_NO_DEVICE, "libptshim.so is not built (run __graft_entry__.build()); "
                                              "there is no CPU fallback for the hot path")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError here = ABI drift; do not mask it
            fn.restype = res
            fn.argtypes = args
        if lib.pt_abi_version() != PT_SHIM_ABI_VERSION:
            raise ShimError(PT_ERR_INVALID, "libptshim.so speaks ABI version %d, this binding %d: rebuild (__graft_entry__.build())"
                            % (lib.pt_abi_version(), PT_SHIM_ABI_VERSION))
        _lib = lib
    return _lib


def check(rc: int) -> None:
    if rc != PT_OK:
        raise ShimError(rc, load().pt_last_error().decode("utf-8", "replace"))
