"""The pixel-list entry points (rt_render_pixels, rt_render_pixels_extend and their device variants) without a GPU: they are
declared and bound, every argument error -- a host list with an entry outside the frame included -- is reported before any device
call and writes nothing, n = 0 is a no-op, the Python wrapper refuses wrong shapes and dtypes, the C consumer builds, and the launch
plan treats a pixel list as the footprint list of the same length run by the pixel-list kernels."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("rt_render_pixels", "rt_render_pixels_device", "rt_render_pixels_extend", "rt_render_pixels_extend_device")
MAX_W, MAX_H = 4, 3
FRAME = (2 * MAX_W + 1) * (2 * MAX_H + 1)


def _scene(rt):
    P, S, H, Tex, Px = rt.Point.make, rt.SphereStyle, rt.Hittable, rt.Texture.Colour, rt.Pixel
    return rt.Scene.make([H.Sphere(rt.Sphere.make(S.LambertReflection(0.8, Tex(Px(200, 100, 50))), P(0.0, 0.0, 3.0), 1.0))])


def _camera(rt, spp=20, depth=3):
    cam = rt.Camera.makeBasic(spp, 1.0, 9.0 / 7.0, rt.Point.make(0.0, 0.0, -1.0), rt.Vector.unitise(rt.Vector.make(0.0, 0.0, 1.0)), rt.Vector.make(0.0, 1.0, 0.0))
    return dataclasses.replace(cam, BounceDepth=depth)


def test_prototypes_and_version(rt):
    from ray_tracing_fsharp_amd import _lib
    header = open(os.path.join(ROOT, "include", "rtfs_amd.h")).read()
    assert "#define RT_ABI_VERSION 7" in header
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES
    assert rt.lib.rt_abi_version() == 7 == rt._abi.RT_ABI_VERSION
    assert "4 pixel list" in header  # rt_dev_last_launch_plan's kinds
    assert "Scene.fs:157-194" in header and "Scene.fs:219,226" in header


def _calls(rt, s, cam, n, px, accum, rgb, max_w=MAX_W, max_h=MAX_H, done=12, options=None):
    """The four entry points with the same arguments (the host variants take no options)."""
    L = rt.lib
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None  # noqa: E731
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)) if a is not None else None  # noqa: E731
    c = C.byref(cam) if cam is not None else None
    o = C.byref(options) if options is not None else None
    if options is None:
        yield lambda: L.rt_render_pixels(s, c, max_w, max_h, 1, 0, n, i32(px), 0, i32(accum), u8(rgb), None)
        yield lambda: L.rt_render_pixels_extend(s, c, max_w, max_h, 1, 0, n, i32(px), 0, done, i32(accum), u8(rgb), None)
    yield lambda: L.rt_render_pixels_device(s, c, max_w, max_h, 1, 0, n, p(px), 0, p(accum), p(rgb), None, o, None)
    yield lambda: L.rt_render_pixels_extend_device(s, c, max_w, max_h, 1, 0, n, p(px), 0, done, p(accum), p(rgb), None, o, None)


def test_invalid_arguments_are_refused_before_any_device_call(rt):
    A = rt._abi
    scene = _scene(rt)
    n = 5
    px = np.array([0, 7, FRAME - 1, 7, 30], np.int32)
    accum, rgb = np.full((n, 4), 77, np.int32), np.full((n, 3), 3, np.uint8)
    S = scene.handle
    cam = _camera(rt).to_abi()
    bad = A.rt_render_options(block_threads=100)
    unset = A.rt_render_options(); unset.struct_size = 0

    def with_cam(**kw):
        c = _camera(rt).to_abi()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    cases = []
    cases += list(_calls(rt, None, cam, n, px, accum, rgb))                           # NULL scene
    cases += list(_calls(rt, S, None, n, px, accum, rgb))                             # NULL camera
    cases += list(_calls(rt, S, cam, n, px, accum, rgb, max_w=0))                     # geometry
    cases += list(_calls(rt, S, cam, n, px, accum, rgb, max_h=-2))
    cases += list(_calls(rt, S, cam, n, px, accum, rgb, max_w=(1 << 20) + 1))
    cases += list(_calls(rt, S, cam, n, px, accum, rgb, max_w=40000, max_h=40000))    # a frame of more than INT32_MAX pixels
    cases += list(_calls(rt, S, cam, n, px, accum, rgb, max_w=1 << 20, max_h=512))    # ... just above: 2097153 * 1025
    cases += list(_calls(rt, S, with_cam(samples_per_pixel=0), n, px, accum, rgb))    # camera
    cases += list(_calls(rt, S, with_cam(samples_per_pixel=8000001), n, px, accum, rgb))
    cases += list(_calls(rt, S, with_cam(bounce_depth=-1), n, px, accum, rgb))
    cases += list(_calls(rt, S, with_cam(bounce_depth=0x1000000), n, px, accum, rgb))
    cases += list(_calls(rt, S, cam, n, None, accum, rgb))                            # NULL pixels
    cases += list(_calls(rt, S, cam, n, px, None, rgb))                               # NULL accum
    cases += list(_calls(rt, S, cam, 2**31, px, accum, rgb))                          # n > INT32_MAX
    cases += list(_calls(rt, S, cam, n, px, accum, rgb, options=bad))                 # settings out of range
    cases += list(_calls(rt, S, cam, n, px, accum, rgb, options=unset))               # struct_size not set
    cases += list(_calls(rt, S, cam, n, px, accum, rgb, options=A.rt_render_options(passes=3)))
    cases += list(_calls(rt, S, cam, n, px, accum, rgb, options=A.rt_render_options(chunk_pixels=65)))
    assert len(cases) == 14 * 4 + 4 * 2
    # what check_extend rejects: the two extend variants
    for done in (0, 11, 21):  # below 12; above the target (20)
        cases += list(_calls(rt, S, cam, n, px, accum, rgb, done=done))[1::2]
    # a HOST list with an entry outside the frame: the two host variants
    for entry in (-1, FRAME, -2**31, 2**31 - 1):
        lst = px.copy()
        lst[3] = entry
        cases += list(_calls(rt, S, cam, n, lst, accum, rgb))[:2]
    assert len(cases) == 64 + 6 + 8
    for i, call in enumerate(cases):
        assert call() == A.RT_ERR_INVALID_ARGUMENT, i
        assert rt.lib.rt_last_error()
        assert (accum == 77).all() and (rgb == 3).all()  # nothing written
    assert (2 * (1 << 20) + 1) * 1025 > 2**31 - 1 >= FRAME


def test_an_empty_list_is_a_no_op(rt):
    A = rt._abi
    scene, cam = _scene(rt), _camera(rt).to_abi()
    for call in _calls(rt, scene.handle, cam, 0, None, None, None):
        assert call() == A.RT_OK
    L, S = rt.lib, scene.handle
    for call in (lambda st: L.rt_render_pixels(S, C.byref(cam), MAX_W, MAX_H, 1, 0, 0, None, 0, None, None, C.byref(st)),
                 lambda st: L.rt_render_pixels_device(S, C.byref(cam), MAX_W, MAX_H, 1, 0, 0, None, 0, None, None, None, None, C.byref(st)),
                 lambda st: L.rt_render_pixels_extend(S, C.byref(cam), MAX_W, MAX_H, 1, 0, 0, None, 0, 12, None, None, C.byref(st)),
                 lambda st: L.rt_render_pixels_extend_device(S, C.byref(cam), MAX_W, MAX_H, 1, 0, 0, None, 0, 12, None, None, None, None, C.byref(st))):
        st = A.rt_stats(rays=5, samples=9, pixels=4, kernel_ms=3.0)
        assert call(st) == A.RT_OK
        assert st.rays == 0 and st.samples == 0 and st.pixels == 0 and st.kernel_ms == 0.0
    res = scene.renderPixels(MAX_W, MAX_H, _camera(rt), np.zeros(0, np.int32))
    assert res.accum.shape == (0, 4) and res.accum.dtype == np.int32 and res.rgb.shape == (0, 3) and res.rgb.dtype == np.uint8
    assert res.stats["pixels"] == 0 and res.stats is scene.last_stats
    # an extension with nothing to add (target == samples_done) is one too: the buffer comes back as it was
    accum = np.full((3, 4), 77, np.int32)
    res = scene.renderPixels(MAX_W, MAX_H, _camera(rt, spp=20), np.array([1, 2, 3], np.int32), extend=(accum, 20))
    assert np.array_equal(res.accum, accum) and res.stats["pixels"] == 0


def test_without_a_gpu_the_render_fails_loudly(rt):
    if rt.device_count() > 0:
        pytest.skip("a GPU is visible")
    scene = _scene(rt)
    with pytest.raises(rt.RtError) as e:
        scene.renderPixels(MAX_W, MAX_H, _camera(rt), np.array([0, 5, 9], np.int32))
    assert e.value.code == rt._abi.RT_ERR_NO_DEVICE
    with pytest.raises(rt.RtError) as e:
        scene.renderPixels(MAX_W, MAX_H, _camera(rt), np.array([0, 5, 9], np.int32), extend=(np.full((3, 4), 12, np.int32), 12))
    assert e.value.code == rt._abi.RT_ERR_NO_DEVICE


def test_python_wrapper_checks_shapes_and_dtypes(rt):
    scene, cam = _scene(rt), _camera(rt)
    with pytest.raises(TypeError):
        scene.renderPixels(MAX_W, MAX_H, cam, np.ones(3, np.int64))
    with pytest.raises(TypeError):
        scene.renderPixels(MAX_W, MAX_H, cam, np.ones(3, np.uint32))
    with pytest.raises(TypeError):
        scene.renderPixels(MAX_W, MAX_H, cam, np.ones(3, np.float64))
    with pytest.raises(TypeError):
        scene.renderPixels(MAX_W, MAX_H, cam, [0, 1, 2])
    with pytest.raises(ValueError):
        scene.renderPixels(MAX_W, MAX_H, cam, np.ones((3, 1), np.int32))
    with pytest.raises(ValueError):
        scene.renderPixels(MAX_W, MAX_H, cam, np.ones((2, 2), np.int32))
    with pytest.raises(ValueError):
        scene.renderPixels(MAX_W, MAX_H, cam, np.array(3, np.int32))
    with pytest.raises(ValueError):  # options belong to the device entry
        scene.renderPixels(MAX_W, MAX_H, cam, np.ones(3, np.int32), options=rt._abi.rt_render_options(passes=2))
    with pytest.raises(TypeError):   # extend's accum
        scene.renderPixels(MAX_W, MAX_H, cam, np.ones(3, np.int32), extend=(np.ones((3, 4), np.int64), 12))
    with pytest.raises(ValueError):
        scene.renderPixels(MAX_W, MAX_H, cam, np.ones(3, np.int32), extend=(np.ones((2, 4), np.int32), 12))
    with pytest.raises(ValueError):
        scene.renderPixels(MAX_W, MAX_H, cam, np.ones(3, np.int32), extend=(np.ones((3, 3), np.int32), 12))
    for px in ([0, -1, 2], [0, FRAME, 2]):  # the library's own refusals arrive as RtError
        with pytest.raises(rt.RtError) as e:
            scene.renderPixels(MAX_W, MAX_H, cam, np.array(px, np.int32))
        assert e.value.code == rt._abi.RT_ERR_INVALID_ARGUMENT
    with pytest.raises(rt.RtError) as e:
        scene.renderPixels(MAX_W, MAX_H, cam, np.ones(3, np.int32), extend=(np.ones((3, 4), np.int32), 11))
    assert e.value.code == rt._abi.RT_ERR_INVALID_ARGUMENT


def build_pixels_smoke(tmp_path):
    exe = str(tmp_path / "pixels_smoke")
    libdir = os.path.join(ROOT, "ray-tracing-fsharp_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "pixels_smoke.c"),
                           "-L", libdir, "-lrtfs_amd", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    return exe


def test_c_program_checks_the_pixel_list_arguments(rt, tmp_path):
    """tests/c/pixels_smoke.c from C99: the argument checks hold without a GPU (with one, test_gpu_pixels compares its pixels with
    the oracle's frame)."""
    out = subprocess.run([build_pixels_smoke(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pixels: argument checks ok" in out.stdout


PLAN_PROBE = r"""
#include "rt_launch_plan.h"
#include <cstdio>
#include <initializer_list>
// a pixel list against the footprint list of the same length: the same decisions field for field, the pixel-list kernels
int main() {
    int bad = 0, seen = 0, two = 0;
    const unsigned long long lengths[] = {1, 7, 1001, 19999, 300001};
    for (int first : {0, 12})
    for (int tex = 0; tex < 2; ++tex) for (int big = 0; big < 2; ++big) for (int count = 0; count < 2; ++count)
    for (int spp : {1, 3, 40, 80, 300}) for (int passes = 0; passes < 3; ++passes) for (int block : {0, 256, 512, 768, 1024}) for (int chunk : {0, 1, 64})
    for (unsigned long long n : lengths) {
        if (first != 0 && spp <= first) continue; // (an extension needs samples to add: the entry points make a no-op of the rest)
        rtp::SceneSize sc; sc.lds_total = big ? 400000 : 30000; sc.lds32_total = big ? 300000 : 20000; sc.n_nodes = big ? 5199 : 99;
        sc.n_objects = big ? 2602 : 52; sc.tex = tex;
        rtp::Settings st{}; st.passes = passes; st.block = block; st.chunk = chunk;
        rtp::Job fp; fp.kind = rtp::Job::FOOTPRINTS; fp.n = n; fp.spp = spp; fp.first_sample = first;
        rtp::Job px = fp; px.kind = rtp::Job::PIXELS;
        rtp::LaunchPlan a = rtp::plan_begin(sc, st, count, fp, 256), b = rtp::plan_begin(sc, st, count, px, 256);
        rtp::plan_finish(a, 2); rtp::plan_finish(b, 2);
        auto same = [&](const rtp::Pass &x, const rtp::Pass &y, int shift) {
            return y.mode == x.mode + shift && x.lds == y.lds && x.count == y.count && x.tex == y.tex && x.block == y.block && x.grid == y.grid && x.lds_bytes == y.lds_bytes &&
                   x.chunk == y.chunk && x.park == y.park && x.park_l == y.park_l && x.park_l_lds == y.park_l_lds && x.lds_node_bytes == y.lds_node_bytes &&
                   x.lds_node_thr == y.lds_node_thr && x.k == y.k && x.total_waves == y.total_waves && x.yield_lanes == y.yield_lanes && x.leaf_wait == y.leaf_wait &&
                   x.refill_lanes == y.refill_lanes;
        };
        const int want_block = block == 256 ? 256 : 1024;
        bool ok = px.pixels() && px.list() && px.pixel_count() == n && px.extend() == (first != 0) &&
                  a.two_pass == b.two_pass && a.pixels == b.pixels && b.pixels == n && a.waves == b.waves && a.pool_bytes == b.pool_bytes &&
                  a.pairs_bytes == b.pairs_bytes && a.list_bytes == b.list_bytes && a.sort_bytes == b.sort_bytes && (a.error != nullptr) == (b.error != nullptr) &&
                  a.one.mode == 6 && b.one.mode == 11 && same(a.one, b.one, 5) && b.one.block == want_block;
        if (ok && b.two_pass && !b.error) {
            ok = a.b.mode == 8 && b.b.mode == 13 && same(a.b, b.b, 5);
            if (first == 0) ok = ok && a.a.mode == 7 && b.a.mode == 12 && same(a.a, b.a, 5);
            else ok = ok && b.a.grid == 0 && b.a.chunk == 0 && a.a.grid == 0; // an extension: no pass A
            ++two;
        }
        if (first != 0) ok = ok && b.two_pass && !b.error; // an extension is pass B alone
        ++seen;
        if (!ok) { ++bad; std::printf("differs: first %d tex %d big %d count %d spp %d passes %d block %d chunk %d n %llu\n", first, tex, big, count, spp, passes, block, chunk, n); }
    }
    std::printf("pixel-list plans: %d of %d differ, %d in two passes\n", bad, seen, two);
    return bad != 0 || two == 0 || two == seen;
}
"""


def test_a_pixel_list_is_planned_as_the_footprint_list_of_the_same_length(tmp_path):
    """rt_launch_plan.h on the CPU: for every combination of scene size, settings and list length a pixel list gets the plan of the
    footprint list of as many pixels -- hence of a one-row frame: unit sizes, fused or two passes, placement, pools, workspace -- field
    for field, with modes 11 / 12 / 13 in place of 6 / 7 / 8, a block of 512 or 768 threads running as 1024; and again as an extension
    from 12 samples (pass B alone)."""
    src, exe = tmp_path / "plan_probe.cpp", str(tmp_path / "plan_probe")
    src.write_text(PLAN_PROBE)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "ray-tracing-fsharp_amd", "csrc"), str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    assert "pixel-list plans: 0 of" in out.stdout
