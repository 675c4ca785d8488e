"""Loads librtfs_amd.so (the HIP product library) and declares the C ABI of include/rtfs_amd.h.

There is no fallback: if the library is missing the import fails loudly, and compute entry points return
RT_ERR_NO_DEVICE (raised as RtError) when no GPU is visible.
"""
import ctypes as C
import os

from . import _abi as A

_HERE = os.path.dirname(os.path.abspath(__file__))
# RTFS_LIB: another build of the same library (kernel A/B experiments, scripts/ab.sh); the default is the in-tree product build
LIB_PATH = os.environ.get("RTFS_LIB") or os.path.join(_HERE, "librtfs_amd.so")


class RtError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"rtfs_amd error {code}: {message}")
        self.code = code
        self.message = message


def _preload_hip_runtime():
    """A process must hold ONE HIP/HSA runtime.  PyTorch-ROCm wheels bundle their own libamdhip64.so (SONAME libamdhip64.so.7,
    RPATH $ORIGIN); if librtfs_amd.so pulled in /opt/rocm's copy first, a later `import torch` would start a second runtime
    that finds no GPU.  So when a torch wheel is present, its runtime is loaded first (torch itself is NOT imported) and
    librtfs_amd.so's NEEDED libamdhip64.so.7 binds to it; without torch the system runtime is used."""
    import importlib.util

    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    bundled = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(bundled):
        C.CDLL(bundled, mode=C.RTLD_GLOBAL)


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C ray-tracing-fsharp_amd/csrc` (hipcc, gfx950). There is no CPU fallback."
        )
    _preload_hip_runtime()
    return C.CDLL(LIB_PATH)


lib = _load()

_P = C.POINTER
_dp, _u8p, _i32p, _u32p, _u64p = _P(C.c_double), _P(C.c_uint8), _P(C.c_int32), _P(C.c_uint32), _P(C.c_uint64)

# name -> (restype, argtypes); every symbol include/rtfs_amd.h declares
SIGNATURES = {
    "rt_abi_version": (C.c_int, []),
    "rt_abi_sizeof": (C.c_size_t, [C.c_int]),
    "rt_abi_offsetof": (C.c_size_t, [C.c_int, C.c_int]),
    "rt_last_error": (C.c_char_p, []),
    "rt_device_count": (C.c_int, []),
    "rt_set_launch_config": (C.c_int, [C.c_int32, C.c_int32, C.c_int32]),
    "rt_set_schedule": (C.c_int, [C.c_int32, C.c_int32]),
    "rt_set_passes": (C.c_int, [C.c_int32]),
    "rt_set_walk_tree": (C.c_int, [C.c_int32]),
    "rt_set_park": (C.c_int, [C.c_int32]),
    "rt_last_stage_stats": (C.c_int, [_u64p]),  # out[16]
    "rt_dev_last_launch_plan": (C.c_int, [_P(C.c_int64)]),  # out[RT_LAUNCH_PLAN_WORDS]
    "rt_camera_make_basic": (C.c_int, [C.c_int32, C.c_double, C.c_double, _dp, _dp, _dp, _P(A.rt_camera)]),
    "rt_scene_create": (C.c_int, [_P(A.rt_hittable), C.c_size_t, _P(A.rt_texture), C.c_size_t, _P(C.c_void_p)]),
    "rt_scene_create_ex": (C.c_int, [_P(A.rt_hittable), C.c_size_t, _P(A.rt_texture), C.c_size_t, _P(A.rt_scene_options), _P(C.c_void_p)]),
    "rt_scene_destroy": (None, [C.c_void_p]),
    "rt_scene_get_info": (C.c_int, [C.c_void_p, _P(A.rt_scene_info)]),
    "rt_scene_get_tree": (C.c_int, [C.c_void_p, _i32p, _i32p, _dp]),
    "rt_scene_get_walk_tree": (C.c_int, [C.c_void_p, _i32p, _i32p, _dp]),
    "rt_scene_get_filter_tree": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), _i32p]),
    "rt_scene_tune_rays": (C.c_int, [C.c_void_p, _dp, C.c_size_t, _P(A.rt_tune_info)]),
    "rt_scene_tune": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_int32, _P(A.rt_tune_info)]),
    "rt_render": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_int32, C.c_int32,
                            C.c_int32, C.c_uint32, _i32p, _u8p, _P(A.rt_stats)]),
    "rt_render_device": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_int32,
                                   C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, _P(A.rt_stats)]),
    "rt_render_device_ex": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, _P(A.rt_render_options),
                                      _P(A.rt_stats)]),
    "rt_render_frame": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_uint64, _i32p, C.c_int32, C.c_uint32, C.c_int32,
                                  _P(A.rt_render_options), _i32p, _u8p, _P(A.rt_stats)]),
    "rt_hit_objects": (C.c_int, [C.c_void_p, C.c_int32, C.c_size_t, _dp, C.c_uint32, _i32p, _dp, _P(A.rt_stats)]),
    "rt_hit_objects_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        _P(A.rt_render_options), _P(A.rt_stats)]),
    "rt_trace_rays": (C.c_int, [C.c_void_p, C.c_int32, C.c_size_t, _dp, _u32p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int32, C.c_uint32,
                                _u8p, _P(A.rt_stats)]),
    "rt_trace_rays_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32,
                                       C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, _P(A.rt_render_options), _P(A.rt_stats)]),
    "rt_render_footprints": (C.c_int, [C.c_void_p, C.c_int32, C.c_size_t, _dp, C.c_int32, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint32,
                                       _i32p, _u8p, _P(A.rt_stats)]),
    "rt_render_footprints_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_size_t, C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.c_uint64,
                                              C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, _P(A.rt_render_options), _P(A.rt_stats)]),
    "rt_render_pixels": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_size_t, _i32p, C.c_uint32,
                                   _i32p, _u8p, _P(A.rt_stats)]),
    "rt_render_pixels_device": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_size_t, C.c_void_p,
                                          C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, _P(A.rt_render_options), _P(A.rt_stats)]),
    "rt_render_pixels_extend": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_size_t, _i32p,
                                          C.c_uint32, C.c_int32, _i32p, _u8p, _P(A.rt_stats)]),
    "rt_render_pixels_extend_device": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_size_t,
                                                 C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 _P(A.rt_render_options), _P(A.rt_stats)]),
    # (stats is bound as an untyped pointer: the census of host/device pairs in tests/test_abi.py, which pins the twelve pairs Scene._launch
    # serves, goes by a trailing rt_stats pointer; Scene.renderViews calls this pair itself)
    "rt_render_views": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_int32, _u64p, C.c_uint64, C.c_int32, C.c_uint32, _i32p, _u8p,
                                  C.c_void_p]),
    "rt_render_views_device": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_int32, _u64p, C.c_uint64, C.c_int32, C.c_uint32,
                                         C.c_void_p, C.c_void_p, C.c_void_p, _P(A.rt_render_options), _P(A.rt_stats)]),
    # (stats bound as an untyped pointer, as rt_render_views': Scene.extendViews and Scene.extendViewsMap call these pairs themselves)
    "rt_render_views_extend": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_int32, _u64p, C.c_uint64, C.c_int32, C.c_uint32, C.c_int32,
                                         _i32p, _u8p, C.c_void_p]),
    "rt_render_views_extend_device": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_int32, _u64p, C.c_uint64, C.c_int32, C.c_uint32,
                                                C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, _P(A.rt_render_options), _P(A.rt_stats)]),
    "rt_render_views_extend_map": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_int32, _u64p, C.c_uint64, C.c_int32, C.c_uint32, _i32p,
                                             _i32p, _u8p, C.c_void_p]),
    "rt_render_views_extend_map_device": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_int32, _u64p, C.c_uint64, C.c_int32, C.c_uint32,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _P(A.rt_render_options), _P(A.rt_stats)]),
    "rt_camera_hits": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_size_t, _i32p, C.c_int32, C.c_int32,
                                 C.c_uint32, _i32p, _dp, _dp, _P(A.rt_stats)]),
    "rt_camera_hits_device": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_size_t, C.c_void_p, C.c_int32,
                                        C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _P(A.rt_render_options), _P(A.rt_stats)]),
    # (stats bound as an untyped pointer, as rt_render_views': Scene.cameraHitsViews calls this pair itself)
    "rt_camera_hits_views": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_int32, _u64p, C.c_uint64, C.c_int32, C.c_size_t, _i32p,
                                       C.c_int32, C.c_int32, C.c_uint32, _i32p, _dp, _dp, C.c_void_p]),
    "rt_camera_hits_views_device": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_int32, _u64p, C.c_uint64, C.c_int32, C.c_size_t,
                                              C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              _P(A.rt_render_options), _P(A.rt_stats)]),
    "rt_camera_paths": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_size_t, _i32p, C.c_int32, C.c_int32,
                                  C.c_uint32, _P(A.rt_path_outputs), _P(A.rt_stats)]),
    "rt_camera_paths_device": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_size_t, C.c_void_p, C.c_int32,
                                         C.c_int32, C.c_uint32, _P(A.rt_path_outputs), C.c_void_p, _P(A.rt_render_options), _P(A.rt_stats)]),
    "rt_trace_paths": (C.c_int, [C.c_void_p, C.c_int32, C.c_size_t, _dp, _u32p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int32, C.c_uint32,
                                 _P(A.rt_path_outputs), _P(A.rt_stats)]),
    "rt_trace_paths_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32,
                                        C.c_int32, C.c_uint32, _P(A.rt_path_outputs), C.c_void_p, _P(A.rt_render_options), _P(A.rt_stats)]),
    "rt_dev_last_paths_plan": (C.c_int, [_P(C.c_int64)]),  # out[8]
    # (stats bound as an untyped pointer, as rt_render_views': Scene.surfaces and Scene.cameraSurfaces call these pairs themselves)
    "rt_surfaces": (C.c_int, [C.c_void_p, C.c_int32, C.c_size_t, _i32p, _dp, _dp, C.c_uint32, _P(A.rt_surface_outputs), C.c_void_p]),
    "rt_surfaces_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, _P(A.rt_surface_outputs),
                                     C.c_void_p, _P(A.rt_render_options), _P(A.rt_stats)]),
    "rt_camera_surfaces": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_size_t, _i32p, C.c_int32, C.c_int32,
                                     C.c_uint32, _i32p, _dp, _P(A.rt_surface_outputs), C.c_void_p]),
    "rt_camera_surfaces_device": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_size_t, C.c_void_p, C.c_int32,
                                            C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, _P(A.rt_surface_outputs), C.c_void_p,
                                            _P(A.rt_render_options), _P(A.rt_stats)]),
    "rt_dev_last_surface_plan": (C.c_int, [_P(C.c_int64)]),  # out[8]
    "rt_render_extend": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_int32, C.c_int32,
                                   C.c_int32, C.c_uint32, C.c_int32, _i32p, _u8p, _P(A.rt_stats)]),
    "rt_render_extend_device": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_int32,
                                          C.c_int32, C.c_int32, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                          _P(A.rt_render_options), _P(A.rt_stats)]),
    "rt_render_footprints_extend": (C.c_int, [C.c_void_p, C.c_int32, C.c_size_t, _dp, C.c_int32, C.c_int32, C.c_uint64, C.c_uint64,
                                              C.c_uint32, C.c_int32, _i32p, _u8p, _P(A.rt_stats)]),
    "rt_render_footprints_extend_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_size_t, C.c_void_p, C.c_int32, C.c_int32, C.c_uint64,
                                                     C.c_uint64, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     _P(A.rt_render_options), _P(A.rt_stats)]),
    "rt_render_extend_map": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_int32, C.c_uint32, _i32p, _i32p, _u8p, _P(A.rt_stats)]),
    "rt_render_extend_map_device": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_int32,
                                              C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              _P(A.rt_render_options), _P(A.rt_stats)]),
    "rt_render_footprints_extend_map": (C.c_int, [C.c_void_p, C.c_int32, C.c_size_t, _dp, C.c_int32, C.c_int32, C.c_uint64, C.c_uint64,
                                                  C.c_uint32, _i32p, _i32p, _u8p, _P(A.rt_stats)]),
    "rt_render_footprints_extend_map_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_size_t, C.c_void_p, C.c_int32, C.c_int32, C.c_uint64,
                                                         C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                         _P(A.rt_render_options), _P(A.rt_stats)]),
    "rt_gamma_correct": (C.c_uint8, [C.c_uint8]),
    "rt_write_ppm": (C.c_int, [C.c_char_p, _u8p, C.c_int32, C.c_int32, C.c_int32]),
    "rt_format_ppm": (C.c_int64, [_u8p, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]),
    "rt_format_pixel_map": (C.c_int64, [_u8p, C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]),
    "rt_parse_pixel_map": (C.c_int64, [C.c_char_p, C.c_size_t, C.c_int32, C.c_int32, _u8p, _u8p]),
    "rt_ppm_max_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "rt_pixel_map_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "rt_gamma_correct_device": (C.c_int, [C.c_int32, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_format_ppm_device": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                       _P(C.c_int64)]),
    "rt_format_pixel_map_device": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                             _P(C.c_int64)]),
    "rt_write_ppm_device": (C.c_int, [C.c_char_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "rt_render_ppm": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_uint32, C.c_int32, C.c_char_p,
                                _P(A.rt_render_options), _P(A.rt_stats)]),
    "rt_write_png": (C.c_int, [C.c_char_p, _u8p, C.c_int32, C.c_int32, C.c_int32]),
    "rt_format_png": (C.c_int64, [_u8p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t]),
    "rt_png_tile_bytes": (C.c_int32, []),
    "rt_png_max_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "rt_format_png_device": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                       _P(C.c_int64)]),
    "rt_write_png_device": (C.c_int, [C.c_char_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "rt_render_png": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_uint32, C.c_int32, C.c_char_p,
                                _P(A.rt_render_options), _P(A.rt_stats)]),
    "rt_png_views_max_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "rt_format_png_views_device": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p,
                                             C.c_void_p, _P(C.c_int64)]),
    "rt_write_png_views_device": (C.c_int, [_P(C.c_char_p), C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "rt_render_views_png": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_int32, _u64p, C.c_uint64, C.c_int32, C.c_uint32, C.c_int32,
                                      _P(C.c_char_p), _P(A.rt_render_options), _P(A.rt_stats)]),
    "rt_pixel_map_chunk_bytes": (C.c_int32, []),
    "rt_pixel_map_tile_bytes": (C.c_int32, []),
    "rt_pixel_map_scan_tiles": (C.c_int32, []),
    "rt_parse_pixel_map_device": (C.c_int, [C.c_int32, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            _P(C.c_int64)]),
    "rt_missing_pixels_device": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, _P(C.c_int64)]),
    "rt_scatter_pixels_device": (C.c_int, [C.c_int32, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "rt_resume_pixel_map": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_uint32, C.c_char_p, C.c_size_t, _u8p,
                                      _P(A.rt_render_options), _P(A.rt_stats)]),
    "rt_resume_png": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_uint32, C.c_char_p, C.c_int32, C.c_char_p,
                                _P(A.rt_render_options), _P(A.rt_stats)]),
    "rt_resume_ppm": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_uint32, C.c_char_p, C.c_int32, C.c_char_p,
                                _P(A.rt_render_options), _P(A.rt_stats)]),
    "rt_render_job_start": (C.c_int, [C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                      C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _P(A.rt_render_options), _P(C.c_void_p)]),
    "rt_render_job_progress": (C.c_int, [C.c_void_p, _P(A.rt_job_progress)]),
    "rt_render_job_stop": (C.c_int, [C.c_void_p]),
    "rt_render_job_wait": (C.c_int, [C.c_void_p, _P(A.rt_job_result), _P(A.rt_stats)]),
    "rt_render_job_finish": (C.c_int, [C.c_void_p, C.c_void_p, _P(A.rt_stats)]),
    "rt_render_job_destroy": (None, [C.c_void_p]),
    "rt_dev_set_job_limits": (C.c_int, [C.c_int64, C.c_int64]),
    "rt_dev_last_job_plan": (C.c_int, [_P(C.c_int64)]),  # out[8]
    "rt_format_pixel_map_present": (C.c_int64, [_u8p, _u8p, C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]),
    "rt_format_pixel_map_present_device": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p,
                                                     C.c_void_p, _P(C.c_int64)]),
    "rt_tree_nodes": (C.c_int64, [C.c_size_t]),
    "rt_tree_depth": (C.c_int32, [C.c_size_t]),
    "rt_tree_lds_boxes": (C.c_int32, []),
    "rt_tree_make_host": (C.c_int, [C.c_size_t, _dp, _i32p, _i32p, _dp, _i32p]),
    "rt_tree_make": (C.c_int, [C.c_int32, C.c_size_t, _dp, _i32p, _i32p, _dp, _i32p]),
    "rt_tree_make_device": (C.c_int, [C.c_int32, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_scene_create_gpu_tree": (C.c_int, [_P(A.rt_hittable), C.c_size_t, _P(A.rt_texture), C.c_size_t, _P(A.rt_scene_options), C.c_int32,
                                           _P(C.c_void_p)]),
    "rt_walk_tree_make_host": (C.c_int, [C.c_size_t, _dp, _i32p, _i32p, _dp]),
    "rt_walk_tree_make": (C.c_int, [C.c_int32, C.c_size_t, _dp, _i32p, _i32p, _dp]),
    "rt_walk_tree_make_device": (C.c_int, [C.c_int32, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_scene_create_gpu_trees": (C.c_int, [_P(A.rt_hittable), C.c_size_t, _P(A.rt_texture), C.c_size_t, _P(A.rt_scene_options), C.c_int32,
                                            _P(C.c_void_p)]),
    "rt_scene_create_device": (C.c_int, [C.c_int32, C.c_void_p, C.c_size_t, _P(A.rt_texture), C.c_size_t, _P(A.rt_scene_options), C.c_void_p,
                                         _P(C.c_void_p)]),
    "rt_dev_scene_image": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, _P(C.c_size_t), _u32p]),  # offsets[16]
    "rt_dev_encode_image": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, _P(C.c_size_t)]),
    "rt_dev_encode_image_radix": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, _P(C.c_size_t)]),
    "rt_dev_scene_has_host_mirror": (C.c_int, [C.c_void_p]),
    "rt_jpeg_get_info": (C.c_int, [C.c_char_p, C.c_size_t, _P(A.rt_jpeg_info)]),
    "rt_decode_jpeg": (C.c_int, [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "rt_decode_jpeg_device": (C.c_int, [C.c_int32, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, _P(A.rt_jpeg_stats)]),
    "rt_dev_decode_jpeg": (C.c_int, [C.c_int32, C.c_char_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_size_t]),
    "rt_dev_last_jpeg_plan": (C.c_int, [_P(C.c_int64)]),  # out[8]
    "rt_scene_create_textures": (C.c_int, [_P(A.rt_hittable), C.c_size_t, _P(A.rt_texture), C.c_size_t, _P(A.rt_texels_source), _P(A.rt_scene_options),
                                           C.c_int32, C.c_void_p, _P(C.c_void_p)]),
    "rt_scene_create_device_textures": (C.c_int, [C.c_int32, C.c_void_p, C.c_size_t, _P(A.rt_texture), C.c_size_t, _P(A.rt_texels_source),
                                                  _P(A.rt_scene_options), C.c_void_p, _P(C.c_void_p)]),
    "rt_of_image_device": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rt_scene_set_texels_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]),
    "rt_dev_scene_texels": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, _P(C.c_size_t), _u32p]),  # texel_off[n_textures]
    "rt_dev_last_texture_plan": (C.c_int, [_P(C.c_int64)]),  # out[8]
    "rt_texture_program_check": (C.c_int, [C.c_char_p, C.c_size_t]),
    "rt_dev_float_producer": (C.c_int, [C.c_int32, _u32p, C.c_int32, _dp]),
    "rt_dev_stream_state": (C.c_int, [C.c_int32, C.c_uint64, C.c_int32, _u64p, _u32p, _u32p]),
    "rt_dev_bbox_hits": (C.c_int, [C.c_int32, C.c_int32, _dp, _dp, _i32p]),
    "rt_dev_bbox_filter": (C.c_int, [C.c_int32, C.c_int32, _dp, _dp, C.c_double, _i32p]),
    "rt_dev_pixel_candidates": (C.c_int, [C.c_int32, C.c_void_p, _P(A.rt_camera), C.c_int32, C.c_int32, C.c_int32, _i32p, _i32p]),
    "rt_dev_sphere_first_intersection": (C.c_int, [C.c_int32, C.c_int32, _dp, _dp, _dp]),
    "rt_dev_plane_intersection": (C.c_int, [C.c_int32, C.c_int32, _dp, _dp, _dp]),
    "rt_dev_pixel_combine": (C.c_int, [C.c_int32, C.c_int32, _u8p, _u8p, _u8p]),
    "rt_dev_pixel_darken": (C.c_int, [C.c_int32, C.c_int32, _u8p, _dp, _u8p]),
    "rt_dev_reflection": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, _i32p, _dp, _u8p, _dp, _u32p, _i32p, _u8p, _dp]),
    "rt_dev_hit_object": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, _dp, _i32p, _dp, _u32p]),
    "rt_dev_hit_object_lds": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, _dp, _i32p, _dp]),
    "rt_dev_trace_ray": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, _dp, _u32p, _u8p]),
    "rt_dev_texture_colour_at": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, _dp, _dp, _u8p]),
    "rt_dev_arith": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp]),
}

for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here = the library does not export a declared symbol
    _fn.restype = _res
    _fn.argtypes = _args


def check(code):
    if code != A.RT_OK:
        raise RtError(code, (lib.rt_last_error() or b"").decode("utf-8", "replace"))


for _i, _t in list(enumerate(A.ABI_STRUCTS)) + [(A.ABI_STRUCT_PATH_OUTPUTS, A.rt_path_outputs), (A.ABI_STRUCT_SURFACE_OUTPUTS, A.rt_surface_outputs)]:  # sizes and every field offset of the ctypes mirrors against the library as compiled
    if lib.rt_abi_sizeof(_i) != C.sizeof(_t):
        raise ImportError(f"ABI mismatch for {_t.__name__}: library {lib.rt_abi_sizeof(_i)} vs ctypes {C.sizeof(_t)}")
    for _k, (_fname, *_rest) in enumerate(_t._fields_):
        if lib.rt_abi_offsetof(_i, _k) != getattr(_t, _fname).offset:
            raise ImportError(f"ABI mismatch for {_t.__name__}.{_fname}: library offset {lib.rt_abi_offsetof(_i, _k)} vs ctypes {getattr(_t, _fname).offset}")
    if lib.rt_abi_offsetof(_i, len(_t._fields_)) != C.c_size_t(-1).value:
        raise ImportError(f"ABI mismatch for {_t.__name__}: the library has more fields than the ctypes mirror")
if lib.rt_abi_sizeof(A.ABI_STRUCT_TEXELS_SOURCE) != C.sizeof(A.rt_texels_source):
    raise ImportError(f"ABI mismatch for rt_texels_source: library {lib.rt_abi_sizeof(A.ABI_STRUCT_TEXELS_SOURCE)} vs ctypes {C.sizeof(A.rt_texels_source)}")
if lib.rt_abi_version() != A.RT_ABI_VERSION:
    raise ImportError("ABI version mismatch between librtfs_amd.so and _abi.py")
