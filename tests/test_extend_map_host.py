"""The extension-by-map entry points (rt_render_extend_map, rt_render_footprints_extend_map and their device variants) without a
GPU: declared and bound, every argument error reported before any device call with nothing written, empty shards no-ops, the
Python wrappers' own checks, the item -> (pixel, offset) lookup of pass B's map variant driven exhaustively on a CPU
(tests/c/extend_map_lookup_table.cpp over csrc/rt_extend_map.h), and tests/c/extend_map_smoke.c from C99."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("rt_render_extend_map", "rt_render_extend_map_device", "rt_render_footprints_extend_map", "rt_render_footprints_extend_map_device")
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
    # the four *_extend* signatures with `int32_t samples_done` replaced by the map, in the same position: an int32 pointer for
    # the host variants, a device pointer for the device variants
    for ext, host in (("rt_render_extend", True), ("rt_render_extend_device", False),
                      ("rt_render_footprints_extend", True), ("rt_render_footprints_extend_device", False)):
        (res_e, args_e), (res_m, args_m) = _lib.SIGNATURES[ext], _lib.SIGNATURES[ext.replace("_extend", "_extend_map")]
        at = args_e.index(C.c_uint32) + 1  # behind `flags`
        assert args_e[at] is C.c_int32
        assert res_m is res_e and args_m == args_e[:at] + [C.POINTER(C.c_int32) if host else C.c_void_p] + args_e[at + 1:]
    assert "[78]" in header


def _frame_calls(rt, s, cam, accum, rgb, targets, n_rows=ROWS, options=None):
    L = rt.lib
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None  # noqa: E731
    camp = C.byref(cam) if cam is not None else None
    if options is None:
        yield lambda: L.rt_render_extend_map(s, camp, W, H, 1, 0, 0, 1, n_rows, 0, i32(targets), i32(accum),
                                             rgb.ctypes.data_as(C.POINTER(C.c_uint8)) if rgb is not None else None, None)
    yield lambda: L.rt_render_extend_map_device(s, camp, W, H, 1, 0, 0, 1, n_rows, 0, p(targets), p(accum), p(rgb), None,
                                                C.byref(options) if options is not None else None, None)


def _list_calls(rt, s, n, fp, accum, rgb, targets, cap, depth=3, options=None):
    L = rt.lib
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None  # noqa: E731
    if options is None:
        yield lambda: L.rt_render_footprints_extend_map(s, 0, n, fp.ctypes.data_as(C.POINTER(C.c_double)) if fp is not None else None, cap, depth, 1, 0, 0,
                                                        i32(targets), i32(accum), rgb.ctypes.data_as(C.POINTER(C.c_uint8)) if rgb is not None else None, None)
    yield lambda: L.rt_render_footprints_extend_map_device(s, 0, n, p(fp), cap, depth, 1, 0, 0, p(targets), p(accum), p(rgb), None,
                                                           C.byref(options) if options is not None else None, None)


def test_invalid_arguments_are_refused_before_any_device_call(rt):
    A = rt._abi
    scene = _scene(rt)
    S = scene.handle
    cam = _camera(rt, 40).to_abi()
    accum, rgb = np.full((ROWS, COLS, 4), 77, np.int32), np.full((ROWS, COLS, 3), 3, np.uint8)
    n = ROWS * COLS
    targets = np.full(n, 40, np.int32)
    fp = np.full((n, 12), 1.0)
    bad = A.rt_render_options(block_threads=100)
    unset = A.rt_render_options(); unset.struct_size = 0
    cases = []
    for cap in (11, 1, 0, -3, 8000001):                                              # cap < 12, cap > 8000000
        cases += list(_frame_calls(rt, S, _camera(rt, cap).to_abi(), accum, rgb, targets))
        cases += list(_list_calls(rt, S, n, fp, accum, rgb, targets, cap))
    cases += list(_frame_calls(rt, S, cam, accum, rgb, None))                        # NULL targets with pixels to do
    cases += list(_list_calls(rt, S, n, fp, accum, rgb, None, 40))
    cases += list(_frame_calls(rt, S, cam, None, rgb, targets))                      # NULL accum with pixels to do
    cases += list(_list_calls(rt, S, n, fp, None, rgb, targets, 40))
    cases += list(_frame_calls(rt, None, cam, accum, rgb, targets))                  # NULL scene
    cases += list(_list_calls(rt, None, n, fp, accum, rgb, targets, 40))
    cases += list(_frame_calls(rt, S, None, accum, rgb, targets))                    # what the base calls reject: NULL camera, rows past the image,
    cases += list(_frame_calls(rt, S, cam, accum, rgb, targets, n_rows=ROWS + 1))    # NULL footprints, a negative depth, too many footprints
    cases += list(_list_calls(rt, S, n, None, accum, rgb, targets, 40))
    cases += list(_list_calls(rt, S, n, fp, accum, rgb, targets, 40, depth=-1))
    cases += list(_list_calls(rt, S, 2**31, fp, accum, rgb, targets, 40))
    for o in (bad, unset, A.rt_render_options(passes=3), A.rt_render_options(chunk_pixels=65)):  # bad options
        cases += list(_frame_calls(rt, S, cam, accum, rgb, targets, options=o))
        cases += list(_list_calls(rt, S, n, fp, accum, rgb, targets, 40, options=o))
    assert len(cases) == 20 + 12 + 10 + 8
    for i, call in enumerate(cases):
        assert call() == A.RT_ERR_INVALID_ARGUMENT, i
        assert rt.lib.rt_last_error()
        assert (accum == 77).all() and (rgb == 3).all() and (targets == 40).all()  # nothing written


def test_empty_shards_are_no_ops(rt):
    A = rt._abi
    scene = _scene(rt)
    S = scene.handle
    cam = _camera(rt, 40).to_abi()
    calls = list(_frame_calls(rt, S, cam, None, None, None, n_rows=0)) + list(_list_calls(rt, S, 0, None, None, None, None, 40))
    calls += list(_frame_calls(rt, S, cam, None, None, None, n_rows=0, options=A.rt_render_options(passes=1)))
    for call in calls:
        assert call() == A.RT_OK
    for call in (lambda st: rt.lib.rt_render_extend_map(S, C.byref(cam), W, H, 1, 0, 0, 1, 0, 0, None, None, None, st),
                 lambda st: rt.lib.rt_render_extend_map_device(S, C.byref(cam), W, H, 1, 0, 0, 1, 0, 0, None, None, None, None, None, st),
                 lambda st: rt.lib.rt_render_footprints_extend_map(S, 0, 0, None, 40, 3, 1, 0, 0, None, None, None, st),
                 lambda st: rt.lib.rt_render_footprints_extend_map_device(S, 0, 0, None, 40, 3, 1, 0, 0, None, None, None, None, None, st)):
        st = A.rt_stats(rays=5, samples=9, pixels=4, pixels_early=2, kernel_ms=3.0)
        assert call(C.byref(st)) == A.RT_OK
        assert st.rays == 0 and st.samples == 0 and st.pixels == 0 and st.pixels_early == 0 and st.kernel_ms == 0.0
    res = scene.extend_rows_map(W, H, _camera(rt, 40), np.zeros((0, COLS, 4), np.int32), np.zeros((0, COLS), np.int32))
    assert res.accum.shape == (0, COLS, 4) and res.stats["samples"] == 0 and res.stats is scene.last_stats
    res = scene.renderFootprints(np.zeros((0, 12)), 40, 3, extend_map=(np.zeros((0, 4), np.int32), np.zeros(0, np.int32)))
    assert res.accum.shape == (0, 4) and res.stats["pixels"] == 0


def test_without_a_gpu_the_map_fails_loudly(rt):
    if rt.device_count() > 0:
        pytest.skip("a GPU is visible")
    scene = _scene(rt)
    accum, targets = np.full((ROWS, COLS, 4), 12, np.int32), np.full((ROWS, COLS), 40, np.int32)
    with pytest.raises(rt.RtError) as e:
        scene.extend_rows_map(W, H, _camera(rt, 40), accum, targets)
    assert e.value.code == rt._abi.RT_ERR_NO_DEVICE and (accum == 12).all()
    with pytest.raises(rt.RtError) as e:
        scene.renderFootprints(np.ones((3, 12)), 40, 3, extend_map=(np.full((3, 4), 12, np.int32), np.full(3, 40, np.int32)))
    assert e.value.code == rt._abi.RT_ERR_NO_DEVICE


def test_python_wrappers_check_shapes_and_dtypes(rt):
    scene = _scene(rt)
    cam = _camera(rt, 40)
    good_acc, good_t = np.zeros((ROWS, COLS, 4), np.int32), np.zeros((ROWS, COLS), np.int32)
    for bad in (np.zeros((ROWS, COLS, 4), np.int64), np.zeros((ROWS, COLS + 1, 4), np.int32), np.zeros((ROWS * COLS, 4), np.int32), [[0] * 4]):
        with pytest.raises(ValueError):
            scene.extend_rows_map(W, H, cam, bad, good_t)
    for bad in (np.zeros((ROWS, COLS), np.int64), np.zeros((ROWS, COLS + 1), np.int32), np.zeros(ROWS * COLS, np.int32), np.zeros((ROWS - 1, COLS), np.int32), 40):
        with pytest.raises(ValueError):
            scene.extend_rows_map(W, H, cam, good_acc, bad)
    with pytest.raises(ValueError):  # options belong to the device entry
        scene.extend_rows_map(W, H, cam, good_acc, good_t, options=rt._abi.rt_render_options(passes=2))
    with pytest.raises(TypeError):
        scene.renderFootprints(np.ones((3, 12)), 40, 3, extend_map=(np.zeros((3, 4), np.int64), np.zeros(3, np.int32)))
    for bad_acc, bad_t in ((np.zeros((4, 4), np.int32), np.zeros(3, np.int32)), (np.zeros((3, 4), np.int32), np.zeros(4, np.int32)),
                           (np.zeros((3, 4), np.int32), np.zeros(3, np.int64)), (np.zeros((3, 4), np.int32), np.zeros((3, 1), np.int32))):
        with pytest.raises(ValueError):
            scene.renderFootprints(np.ones((3, 12)), 40, 3, extend_map=(bad_acc, bad_t))
    with pytest.raises(ValueError):  # one kind of extension at a time
        scene.renderFootprints(np.ones((3, 12)), 40, 3, extend=(np.zeros((3, 4), np.int32), 12), extend_map=(np.zeros((3, 4), np.int32), np.zeros(3, np.int32)))
    with pytest.raises(rt.RtError) as e:
        scene.extend_rows_map(W, H, _camera(rt, 11), good_acc, good_t)
    assert e.value.code == rt._abi.RT_ERR_INVALID_ARGUMENT


# ---- the lookup: item -> (pixel, offset) over a range's prefix sums ------------------------------------------------------------
BIG = 2000  # "large" beside 1: enough items that the search crosses every pixel boundary; the arithmetic is the same up to 8e6 a pixel


def _patterns(npx):
    yield [1] * npx                                            # all 1
    yield [1] * (npx // 2) + [BIG] + [1] * (npx - npx // 2 - 1)  # one large among 1s
    yield [BIG] + [1] * (npx - 1)                              # large first
    yield [1] * (npx - 1) + [BIG]                              # large last


def test_every_item_finds_its_pixel_and_offset(tmp_path):
    exe = str(tmp_path / "extend_map_lookup_table")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-o", exe, os.path.join(ROOT, "tests", "c", "extend_map_lookup_table.cpp")])
    cases = [p for npx in range(1, 65) for p in _patterns(npx)]
    cases.append([1] * 63 + [8000000])          # the widest range at the largest count a pixel can have
    cases.append([8000000] + [1] * 63)
    cases += [[0, 3, 0, 0, 2], [2, 0, 0, 5, 0]]  # pixels with nothing to add own no item (the list never holds one; the search does not care)
    text = "".join("lookup %d %s\n" % (len(c), " ".join(map(str, c))) for c in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases) == 64 * 4 + 4
    for c, line in zip(cases, out):
        got = {k: int(v) for k, v in (kv.split("=") for kv in line.split())}
        assert got["npx"] == len(c) and got["total"] == sum(c), (c[:4], got)
        assert got["wrong"] == 0 and got["uncovered"] == 0, (len(c), got)  # every item right; each pixel's offsets 0 .. n2-1 exactly once
        assert got["reads"] <= 6 and got["outside"] == 0, (len(c), got)    # at most six reads of the starts, none past the range


def build_extend_map_smoke(tmp_path):
    exe = str(tmp_path / "extend_map_smoke")
    libdir = os.path.join(ROOT, "ray-tracing-fsharp_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "extend_map_smoke.c"),
                           "-L", libdir, "-lrtfs_amd", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    return exe


def test_c_program_checks_the_map_arguments(rt, tmp_path):
    """tests/c/extend_map_smoke.c from C99: the argument checks hold without a GPU (with one, test_gpu_extend_map holds its frame to the oracle)."""
    out = subprocess.run([build_extend_map_smoke(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "extend_map: argument checks ok" in out.stdout


def test_the_cpp_host_mirror_declares_the_two_calls(tmp_path):
    """host/RayTracing.hpp: Scene::extendRowsMap and Scene::extendFootprintsMap compile against the header (g++ only, nothing is run)."""
    src = tmp_path / "use.cpp"
    src.write_text('#include "RayTracing.hpp"\n'
                   "std::vector<uint8_t> f(RayTracing::Scene &s, const RayTracing::Camera &c, std::vector<int32_t> &a, const std::vector<int32_t> &t, const std::vector<double> &fp) {\n"
                   "    auto r = s.extendRowsMap(3, 2, c, a, t); auto q = s.extendFootprintsMap(fp, 40, 5, a, t, 1, 7); r.insert(r.end(), q.begin(), q.end()); return r; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "ray-tracing-fsharp_amd", "host"), str(src)])
