"""The extension entry points (rt_render_extend, rt_render_footprints_extend and their device variants) without a GPU: declared
and bound, every argument error reported before any device call with nothing written, target == samples_done and empty shards
no-ops, the Python wrappers' own checks, and tests/c/extend_smoke.c from C99."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("rt_render_extend", "rt_render_extend_device", "rt_render_footprints_extend", "rt_render_footprints_extend_device")
W, H = 3, 2
COLS, ROWS = 2 * W + 1, 2 * H + 1


def _scene(rt):
    P, S, Hit, Tex, Px = rt.Point.make, rt.SphereStyle, rt.Hittable, rt.Texture.Colour, rt.Pixel
    return rt.Scene.make([Hit.Sphere(rt.Sphere.make(S.LambertReflection(0.8, Tex(Px(200, 100, 50))), P(0.0, 0.0, 3.0), 1.0))])


def _camera(rt, spp):
    cam = rt.Camera.makeBasic(spp, 1.0, 1.5, rt.Point.make(0.0, 0.0, -1.0), rt.Vector.unitise(rt.Vector.make(0.0, 0.0, 1.0)), rt.Vector.make(0.0, 1.0, 0.0))
    return dataclasses.replace(cam, BounceDepth=5)


def test_prototypes_and_version(rt):
    from ray_tracing_fsharp_amd import _lib
    header = open(os.path.join(ROOT, "include", "rtfs_amd.h")).read()
    assert "#define RT_ABI_VERSION 7" in header  # added symbols only
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES
    assert rt.lib.rt_abi_version() == 7 == rt._abi.RT_ABI_VERSION
    # the extension calls take the base calls' arguments with samples_done in front of the buffers
    for base, ext in (("rt_render", "rt_render_extend"), ("rt_render_device_ex", "rt_render_extend_device"),
                      ("rt_render_footprints", "rt_render_footprints_extend"), ("rt_render_footprints_device", "rt_render_footprints_extend_device")):
        (res_b, args_b), (res_e, args_e) = _lib.SIGNATURES[base], _lib.SIGNATURES[ext]
        at = args_b.index(C.c_uint32) + 1  # behind `flags`
        assert res_e is res_b and args_e == args_b[:at] + [C.c_int32] + args_b[at:]
    # the structs these calls share with the base calls are the library's, field for field
    for which, t in ((2, rt._abi.rt_camera), (4, rt._abi.rt_stats), (5, rt._abi.rt_render_options)):
        assert rt.lib.rt_abi_sizeof(which) == C.sizeof(t)
        for k, (fname, *_r) in enumerate(t._fields_):
            assert rt.lib.rt_abi_offsetof(which, k) == getattr(t, fname).offset
    assert "[77]" in header and "first_sample" in header  # rt_dev_last_launch_plan's new word


def _frame_calls(rt, s, cam, accum, rgb, done, n_rows=ROWS, options=None):
    L = rt.lib
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    camp = C.byref(cam) if cam is not None else None
    if options is None:
        yield lambda: L.rt_render_extend(s, camp, W, H, 1, 0, 0, 1, n_rows, 0, done, accum.ctypes.data_as(C.POINTER(C.c_int32)) if accum is not None else None,
                                         rgb.ctypes.data_as(C.POINTER(C.c_uint8)) if rgb is not None else None, None)
    yield lambda: L.rt_render_extend_device(s, camp, W, H, 1, 0, 0, 1, n_rows, 0, done, p(accum), p(rgb), None,
                                            C.byref(options) if options is not None else None, None)


def _list_calls(rt, s, n, fp, accum, rgb, spp, done, depth=3, options=None):
    L = rt.lib
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    if options is None:
        yield lambda: L.rt_render_footprints_extend(s, 0, n, fp.ctypes.data_as(C.POINTER(C.c_double)) if fp is not None else None, spp, depth, 1, 0, 0, done,
                                                    accum.ctypes.data_as(C.POINTER(C.c_int32)) if accum is not None else None,
                                                    rgb.ctypes.data_as(C.POINTER(C.c_uint8)) if rgb is not None else None, None)
    yield lambda: L.rt_render_footprints_extend_device(s, 0, n, p(fp), spp, depth, 1, 0, 0, done, p(accum), p(rgb), None,
                                                       C.byref(options) if options is not None else None, None)


def test_invalid_arguments_are_refused_before_any_device_call(rt):
    A = rt._abi
    scene = _scene(rt)
    S = scene.handle
    cam = _camera(rt, 40).to_abi()
    accum, rgb = np.full((ROWS, COLS, 4), 77, np.int32), np.full((ROWS, COLS, 3), 3, np.uint8)
    n = ROWS * COLS
    fp = np.full((n, 12), 1.0)
    bad = A.rt_render_options(block_threads=100)
    unset = A.rt_render_options(); unset.struct_size = 0
    low = _camera(rt, 20).to_abi()
    cases = []
    for done in (0, 11, -5):                                                    # samples_done < 12
        cases += list(_frame_calls(rt, S, cam, accum, rgb, done))
        cases += list(_list_calls(rt, S, n, fp, accum, rgb, 40, done))
    cases += list(_frame_calls(rt, S, low, accum, rgb, 21))                     # target < samples_done
    cases += list(_list_calls(rt, S, n, fp, accum, rgb, 20, 21))
    cases += list(_frame_calls(rt, S, cam, None, rgb, 12))                      # NULL accum with pixels to do
    cases += list(_list_calls(rt, S, n, fp, None, rgb, 40, 12))
    cases += list(_frame_calls(rt, None, cam, accum, rgb, 12))                  # NULL scene
    cases += list(_list_calls(rt, None, n, fp, accum, rgb, 40, 12))
    cases += list(_frame_calls(rt, S, None, accum, rgb, 12))                    # what the base calls reject: NULL camera, rows past the image,
    cases += list(_frame_calls(rt, S, cam, accum, rgb, 12, n_rows=ROWS + 1))    # NULL footprints, a negative depth, too many footprints
    cases += list(_list_calls(rt, S, n, None, accum, rgb, 40, 12))
    cases += list(_list_calls(rt, S, n, fp, accum, rgb, 40, 12, depth=-1))
    cases += list(_list_calls(rt, S, 2**31, fp, accum, rgb, 40, 12))
    for o in (bad, unset, A.rt_render_options(passes=3), A.rt_render_options(chunk_pixels=65)):  # bad options
        cases += list(_frame_calls(rt, S, cam, accum, rgb, 12, options=o))
        cases += list(_list_calls(rt, S, n, fp, accum, rgb, 40, 12, options=o))
    assert len(cases) == 42
    for i, call in enumerate(cases):
        assert call() == A.RT_ERR_INVALID_ARGUMENT, i
        assert rt.lib.rt_last_error()
        assert (accum == 77).all() and (rgb == 3).all()  # nothing written


def test_nothing_to_add_is_a_no_op(rt):
    A = rt._abi
    scene = _scene(rt)
    S = scene.handle
    cam = _camera(rt, 40).to_abi()
    accum, rgb = np.full((ROWS, COLS, 4), 77, np.int32), np.full((ROWS, COLS, 3), 3, np.uint8)
    n = ROWS * COLS
    fp = np.full((n, 12), 1.0)
    calls = list(_frame_calls(rt, S, cam, accum, rgb, 40)) + list(_list_calls(rt, S, n, fp, accum, rgb, 40, 40))          # target == samples_done
    calls += list(_frame_calls(rt, S, cam, None, None, 12, n_rows=0)) + list(_list_calls(rt, S, 0, None, None, None, 40, 12))  # empty shards
    calls += list(_frame_calls(rt, S, cam, accum, rgb, 40, options=A.rt_render_options(passes=1)))
    for call in calls:
        assert call() == A.RT_OK
    assert (accum == 77).all() and (rgb == 3).all()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for call in (lambda st: rt.lib.rt_render_extend(S, C.byref(cam), W, H, 1, 0, 0, 1, ROWS, 0, 40, accum.ctypes.data_as(C.POINTER(C.c_int32)), None, st),
                 lambda st: rt.lib.rt_render_extend_device(S, C.byref(cam), W, H, 1, 0, 0, 1, 0, 0, 12, None, None, None, None, st),
                 lambda st: rt.lib.rt_render_footprints_extend(S, 0, 0, None, 40, 3, 1, 0, 0, 12, None, None, st),
                 lambda st: rt.lib.rt_render_footprints_extend_device(S, 0, n, p(fp), 40, 3, 1, 0, 0, 40, p(accum), None, None, None, st)):
        st = A.rt_stats(rays=5, samples=9, pixels=4, pixels_early=2, kernel_ms=3.0)
        assert call(C.byref(st)) == A.RT_OK
        assert st.rays == 0 and st.samples == 0 and st.pixels == 0 and st.pixels_early == 0 and st.kernel_ms == 0.0
    res = scene.extend_rows(W, H, _camera(rt, 40), accum, 40)
    assert np.array_equal(res.accum, accum) and res.accum is not accum and res.stats["samples"] == 0 and res.stats is scene.last_stats
    res = scene.renderFootprints(fp, 40, 3, extend=(accum.reshape(-1, 4), 40))
    assert np.array_equal(res.accum, accum.reshape(-1, 4)) and res.stats["pixels"] == 0


def test_without_a_gpu_the_extension_fails_loudly(rt):
    if rt.device_count() > 0:
        pytest.skip("a GPU is visible")
    scene = _scene(rt)
    accum = np.full((ROWS, COLS, 4), 12, np.int32)
    with pytest.raises(rt.RtError) as e:
        scene.extend_rows(W, H, _camera(rt, 40), accum, 12)
    assert e.value.code == rt._abi.RT_ERR_NO_DEVICE and (accum == 12).all()
    with pytest.raises(rt.RtError) as e:
        scene.renderFootprints(np.ones((3, 12)), 40, 3, extend=(np.full((3, 4), 12, np.int32), 12))
    assert e.value.code == rt._abi.RT_ERR_NO_DEVICE


def test_python_wrappers_check_shapes_and_dtypes(rt):
    scene = _scene(rt)
    cam = _camera(rt, 40)
    for bad in (np.zeros((ROWS, COLS, 4), np.int64), np.zeros((ROWS, COLS + 1, 4), np.int32), np.zeros((ROWS * COLS, 4), np.int32), [[0] * 4]):
        with pytest.raises(ValueError):
            scene.extend_rows(W, H, cam, bad, 12)
    with pytest.raises(ValueError):  # options belong to the device entry
        scene.extend_rows(W, H, cam, np.zeros((ROWS, COLS, 4), np.int32), 12, options=rt._abi.rt_render_options(passes=2))
    with pytest.raises(TypeError):
        scene.renderFootprints(np.ones((3, 12)), 40, 3, extend=(np.zeros((3, 4), np.int64), 12))
    with pytest.raises(ValueError):
        scene.renderFootprints(np.ones((3, 12)), 40, 3, extend=(np.zeros((4, 4), np.int32), 12))
    for done, spp in ((11, 40), (41, 40)):
        with pytest.raises(rt.RtError) as e:
            scene.extend_rows(W, H, _camera(rt, spp), np.zeros((ROWS, COLS, 4), np.int32), done)
        assert e.value.code == rt._abi.RT_ERR_INVALID_ARGUMENT


def build_extend_smoke(tmp_path):
    exe = str(tmp_path / "extend_smoke")
    libdir = os.path.join(ROOT, "ray-tracing-fsharp_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "extend_smoke.c"),
                           "-L", libdir, "-lrtfs_amd", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    return exe


def test_c_program_checks_the_extension_arguments(rt, tmp_path):
    """tests/c/extend_smoke.c from C99: the argument checks hold without a GPU (with one, test_gpu_extend holds its frame to the oracle)."""
    out = subprocess.run([build_extend_smoke(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "extend: argument checks ok" in out.stdout


def test_the_cpp_host_mirror_declares_the_two_calls(tmp_path):
    """host/RayTracing.hpp: Scene::extendRows and Scene::extendFootprints compile against the header (g++ only, nothing is run)."""
    src = tmp_path / "use.cpp"
    src.write_text('#include "RayTracing.hpp"\n'
                   "std::vector<uint8_t> f(RayTracing::Scene &s, const RayTracing::Camera &c, std::vector<int32_t> &a, const std::vector<double> &fp) {\n"
                   "    auto r = s.extendRows(3, 2, c, a, 12); auto q = s.extendFootprints(fp, 40, 5, a, 12, 1, 7); r.insert(r.end(), q.begin(), q.end()); return r; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "ray-tracing-fsharp_amd", "host"), str(src)])
