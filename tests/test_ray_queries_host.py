"""The ray-list entry points (rt_hit_objects, rt_trace_rays and their device variants) without a GPU: they are declared and
bound, every argument error is reported before any device call and writes nothing, n = 0 is a no-op, and the Python
wrappers refuse wrong shapes and dtypes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("rt_hit_objects", "rt_hit_objects_device", "rt_trace_rays", "rt_trace_rays_device")


def _scene(rt):
    P, S, H, Tex, Px = rt.Point.make, rt.SphereStyle, rt.Hittable, rt.Texture.Colour, rt.Pixel
    return rt.Scene.make([H.Sphere(rt.Sphere.make(S.LambertReflection(0.8, Tex(Px(200, 100, 50))), P(0.0, 0.0, 3.0), 1.0))])


def test_prototypes_and_version(rt):
    from ray_tracing_fsharp_amd import _lib
    header = open(os.path.join(ROOT, "include", "rtfs_amd.h")).read()
    assert "#define RT_ABI_VERSION 7" in header
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES
    assert rt.lib.rt_abi_version() == 7 == rt._abi.RT_ABI_VERSION


def _hit_calls(rt, s, n, rays, hit, strike):
    L = rt.lib
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    yield lambda: L.rt_hit_objects(s, 0, n, rays.ctypes.data_as(C.POINTER(C.c_double)) if rays is not None else None, 0,
                                   hit.ctypes.data_as(C.POINTER(C.c_int32)) if hit is not None else None,
                                   strike.ctypes.data_as(C.POINTER(C.c_double)) if strike is not None else None, None)
    yield lambda: L.rt_hit_objects_device(s, 0, n, p(rays), 0, p(hit), p(strike), None, None, None)


def _trace_calls(rt, s, n, rays, rng, colour, depth):
    L = rt.lib
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    yield lambda: L.rt_trace_rays(s, 0, n, rays.ctypes.data_as(C.POINTER(C.c_double)) if rays is not None else None,
                                  rng.ctypes.data_as(C.POINTER(C.c_uint32)) if rng is not None else None, 1, 0, 0, depth, 0,
                                  colour.ctypes.data_as(C.POINTER(C.c_uint8)) if colour is not None else None, None)
    yield lambda: L.rt_trace_rays_device(s, 0, n, p(rays), p(rng), 1, 0, 0, depth, 0, p(colour), None, None, None)


def test_invalid_arguments_are_refused_before_any_device_call(rt):
    A = rt._abi
    scene = _scene(rt)
    n = 5
    rays = np.full((n, 6), 1.0)
    hit, strike = np.full(n, 77, np.int32), np.full((n, 3), 7.0)
    rng, colour = np.full((n, 4), 9, np.uint32), np.full((n, 3), 3, np.uint8)
    S = scene.handle
    cases = []
    cases += list(_hit_calls(rt, None, n, rays, hit, strike))                                  # NULL scene
    cases += list(_hit_calls(rt, S, n, None, hit, strike))                                     # NULL rays
    cases += list(_hit_calls(rt, S, n, rays, None, strike))                                    # NULL hit_index
    cases += list(_trace_calls(rt, None, n, rays, rng, colour, 3))
    cases += list(_trace_calls(rt, S, n, None, rng, colour, 3))
    cases += list(_trace_calls(rt, S, n, rays, rng, None, 3))                                  # NULL colour
    cases += list(_hit_calls(rt, S, 2**31, rays, hit, strike))                                 # n > INT32_MAX
    cases += list(_trace_calls(rt, S, 2**31, rays, rng, colour, 3))
    cases += list(_trace_calls(rt, S, n, rays, rng, colour, -1))                               # bounce_depth < 0
    assert len(cases) == 18
    for call in cases:
        assert call() == A.RT_ERR_INVALID_ARGUMENT
        # nothing written
        assert (hit == 77).all() and (strike == 7.0).all() and (rng == 9).all() and (colour == 3).all()
    # options: an unset struct_size and settings out of range are refused as well
    bad = A.rt_render_options(block_threads=100)
    unset = A.rt_render_options(); unset.struct_size = 0
    for opt in (bad, unset):
        assert rt.lib.rt_hit_objects_device(scene.handle, 0, n, rays.ctypes.data_as(C.c_void_p), 0, hit.ctypes.data_as(C.c_void_p),
                                            None, None, C.byref(opt), None) == A.RT_ERR_INVALID_ARGUMENT
    assert (hit == 77).all()


def test_no_rays_is_a_no_op(rt):
    A = rt._abi
    scene = _scene(rt)
    st = A.rt_stats(rays=5, kernel_ms=3.0)
    for call in list(_hit_calls(rt, scene.handle, 0, None, None, None)) + list(_trace_calls(rt, scene.handle, 0, None, None, None, 0)):
        assert call() == A.RT_OK
    assert rt.lib.rt_hit_objects(scene.handle, 0, 0, None, 0, None, None, C.byref(st)) == A.RT_OK
    assert st.rays == 0 and st.kernel_ms == 0.0
    hit, strike = scene.hitObject(np.zeros((0, 6)))
    assert hit.shape == (0,) and strike.shape == (0, 3)
    col, g = scene.traceRays(np.zeros((0, 6)), 5, rng=np.zeros((0, 4), np.uint32))
    assert col.shape == (0, 3) and g.shape == (0, 4)


def test_without_a_gpu_the_queries_fail_loudly(rt):
    if rt.device_count() > 0:
        pytest.skip("a GPU is visible")
    scene = _scene(rt)
    for fn in (lambda: scene.hitObject(np.ones((3, 6))), lambda: scene.traceRays(np.ones((3, 6)), 4)):
        with pytest.raises(rt.RtError) as e:
            fn()
        assert e.value.code == rt._abi.RT_ERR_NO_DEVICE


def test_python_wrappers_check_shapes_and_dtypes(rt):
    scene = _scene(rt)
    with pytest.raises(TypeError):
        scene.hitObject(np.ones((3, 6), np.float32))
    with pytest.raises(TypeError):
        scene.hitObject([[0.0] * 6])
    with pytest.raises(ValueError):
        scene.hitObject(np.ones((3, 5)))
    with pytest.raises(ValueError):
        scene.hitObject(np.ones(6))
    with pytest.raises(TypeError):
        scene.traceRays(np.ones((3, 6), np.int64), 4)
    with pytest.raises(ValueError):
        scene.traceRays(np.ones((3, 7)), 4)
    with pytest.raises(TypeError):
        scene.traceRays(np.ones((3, 6)), 4, rng=np.ones((3, 4), np.int64))
    with pytest.raises(ValueError):
        scene.traceRays(np.ones((3, 6)), 4, rng=np.ones((2, 4), np.uint32))
    with pytest.raises(ValueError):
        scene.traceRays(np.ones((3, 6)), 4, rng=np.ones((3, 3), np.uint32))
    with pytest.raises(rt.RtError) as e:
        scene.traceRays(np.ones((3, 6)), -1)
    assert e.value.code == rt._abi.RT_ERR_INVALID_ARGUMENT


def build_ray_query_smoke(tmp_path):
    exe = str(tmp_path / "ray_query_smoke")
    libdir = os.path.join(ROOT, "ray-tracing-fsharp_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "ray_query_smoke.c"),
                           "-L", libdir, "-lrtfs_amd", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    return exe


def test_c_program_checks_the_ray_query_arguments(rt, tmp_path):
    """tests/c/ray_query_smoke.c from C99: the argument checks hold without a GPU (with one, test_gpu_ray_queries compares its
    answers with the oracle)."""
    out = subprocess.run([build_ray_query_smoke(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ray queries: argument checks ok" in out.stdout
