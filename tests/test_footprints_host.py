"""The footprint entry points (rt_render_footprints and its device variant) without a GPU: they are declared and bound, every
argument error is reported before any device call and writes nothing, n = 0 is a no-op, the Python wrapper refuses wrong shapes
and dtypes, and the launch plan treats a footprint list as a frame of n pixels run by the footprint kernels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("rt_render_footprints", "rt_render_footprints_device")


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
    assert "3 footprint list" in header  # rt_dev_last_launch_plan's kinds


def _calls(rt, s, n, fp, accum, rgb, spp=8, depth=3, options=None):
    L = rt.lib
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    if options is None:
        yield lambda: L.rt_render_footprints(s, 0, n, fp.ctypes.data_as(C.POINTER(C.c_double)) if fp is not None else None, spp, depth, 1, 0, 0,
                                             accum.ctypes.data_as(C.POINTER(C.c_int32)) if accum is not None else None,
                                             rgb.ctypes.data_as(C.POINTER(C.c_uint8)) if rgb is not None else None, None)
    yield lambda: L.rt_render_footprints_device(s, 0, n, p(fp), spp, depth, 1, 0, 0, p(accum), p(rgb), None,
                                                C.byref(options) if options is not None else None, None)


def test_invalid_arguments_are_refused_before_any_device_call(rt):
    A = rt._abi
    scene = _scene(rt)
    n = 5
    fp = np.full((n, 12), 1.0)
    accum, rgb = np.full((n, 4), 77, np.int32), np.full((n, 3), 3, np.uint8)
    S = scene.handle
    bad = A.rt_render_options(block_threads=100)
    unset = A.rt_render_options(); unset.struct_size = 0
    cases = []
    cases += list(_calls(rt, None, n, fp, accum, rgb))                   # NULL scene
    cases += list(_calls(rt, S, n, None, accum, rgb))                    # NULL footprints
    cases += list(_calls(rt, S, n, fp, None, rgb))                       # NULL accum
    cases += list(_calls(rt, S, 2**31, fp, accum, rgb))                  # n > INT32_MAX
    cases += list(_calls(rt, S, n, fp, accum, rgb, spp=0))               # samples_per_pixel < 1
    cases += list(_calls(rt, S, n, fp, accum, rgb, spp=-4))
    cases += list(_calls(rt, S, n, fp, accum, rgb, depth=-1))            # bounce_depth < 0
    cases += list(_calls(rt, S, n, fp, accum, rgb, depth=0x1000000))     # bounce_depth > 0xFFFFFF
    cases += list(_calls(rt, S, n, fp, accum, rgb, options=bad))         # settings out of range
    cases += list(_calls(rt, S, n, fp, accum, rgb, options=unset))       # struct_size not set
    cases += list(_calls(rt, S, n, fp, accum, rgb, options=A.rt_render_options(passes=3)))
    cases += list(_calls(rt, S, n, fp, accum, rgb, options=A.rt_render_options(chunk_pixels=65)))
    assert len(cases) == 20
    for call in cases:
        assert call() == A.RT_ERR_INVALID_ARGUMENT
        assert rt.lib.rt_last_error()
        assert (accum == 77).all() and (rgb == 3).all()  # nothing written


def test_no_footprints_is_a_no_op(rt):
    A = rt._abi
    scene = _scene(rt)
    for call in _calls(rt, scene.handle, 0, None, None, None):
        assert call() == A.RT_OK
    st = A.rt_stats(rays=5, samples=9, pixels=4, kernel_ms=3.0)
    assert rt.lib.rt_render_footprints(scene.handle, 0, 0, None, 8, 3, 1, 0, 0, None, None, C.byref(st)) == A.RT_OK
    assert st.rays == 0 and st.samples == 0 and st.pixels == 0 and st.kernel_ms == 0.0
    st = A.rt_stats(rays=5, samples=9, pixels=4, kernel_ms=3.0)
    assert rt.lib.rt_render_footprints_device(scene.handle, 0, 0, None, 8, 3, 1, 0, 0, None, None, None, None, C.byref(st)) == A.RT_OK
    assert st.rays == 0 and st.samples == 0 and st.pixels == 0 and st.kernel_ms == 0.0
    res = scene.renderFootprints(np.zeros((0, 12)), 8, 3)
    assert res.accum.shape == (0, 4) and res.accum.dtype == np.int32 and res.rgb.shape == (0, 3) and res.rgb.dtype == np.uint8
    assert res.stats["pixels"] == 0 and res.stats is scene.last_stats


def test_without_a_gpu_the_render_fails_loudly(rt):
    if rt.device_count() > 0:
        pytest.skip("a GPU is visible")
    scene = _scene(rt)
    with pytest.raises(rt.RtError) as e:
        scene.renderFootprints(np.ones((3, 12)), 8, 3)
    assert e.value.code == rt._abi.RT_ERR_NO_DEVICE


def test_python_wrapper_checks_shapes_and_dtypes(rt):
    scene = _scene(rt)
    with pytest.raises(TypeError):
        scene.renderFootprints(np.ones((3, 12), np.float32), 8, 3)
    with pytest.raises(TypeError):
        scene.renderFootprints(np.ones((3, 12), np.int64), 8, 3)
    with pytest.raises(TypeError):
        scene.renderFootprints([[0.0] * 12], 8, 3)
    with pytest.raises(ValueError):
        scene.renderFootprints(np.ones((3, 6)), 8, 3)
    with pytest.raises(ValueError):
        scene.renderFootprints(np.ones(12), 8, 3)
    with pytest.raises(ValueError):
        scene.renderFootprints(np.ones((3, 4, 3)), 8, 3)
    with pytest.raises(ValueError):  # options belong to the device entry
        scene.renderFootprints(np.ones((3, 12)), 8, 3, options=rt._abi.rt_render_options(passes=2))
    for spp, depth in ((0, 3), (8, -1)):
        with pytest.raises(rt.RtError) as e:
            scene.renderFootprints(np.ones((3, 12)), spp, depth)
        assert e.value.code == rt._abi.RT_ERR_INVALID_ARGUMENT


def build_footprint_smoke(tmp_path):
    exe = str(tmp_path / "footprint_smoke")
    libdir = os.path.join(ROOT, "ray-tracing-fsharp_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "footprint_smoke.c"),
                           "-L", libdir, "-lrtfs_amd", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    return exe


def test_c_program_checks_the_footprint_arguments(rt, tmp_path):
    """tests/c/footprint_smoke.c from C99: the argument checks hold without a GPU (with one, test_gpu_footprints compares its
    pixels with the oracle's composition)."""
    out = subprocess.run([build_footprint_smoke(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "footprints: argument checks ok" in out.stdout


PLAN_PROBE = r"""
#include "rt_launch_plan.h"
#include <cstdio>
#include <initializer_list>
// a footprint list against the frame of as many pixels (one row, 2 * max_w + 1 columns): the same decisions, the footprint kernels
int main() {
    int bad = 0;
    const int widths[] = {0, 3, 500, 9999, 150000};
    for (int tex = 0; tex < 2; ++tex) for (int big = 0; big < 2; ++big) for (int count = 0; count < 2; ++count)
    for (int spp : {1, 3, 40, 80, 300}) for (int passes = 0; passes < 3; ++passes) for (int block : {0, 256, 512, 1024}) for (int chunk : {0, 1, 64})
    for (int mw : widths) {
        rtp::SceneSize sc; sc.lds_total = big ? 400000 : 30000; sc.lds32_total = big ? 300000 : 20000; sc.n_nodes = big ? 5199 : 99;
        sc.n_objects = big ? 2602 : 52; sc.tex = tex;
        rtp::Settings st{}; st.passes = passes; st.block = block == 512 ? 1024 : block; st.chunk = chunk;
        rtp::Job frame; frame.n_rows = 1; frame.max_w = mw; frame.spp = spp;
        rtp::Job list; list.kind = rtp::Job::FOOTPRINTS; list.n = 2ull * mw + 1; list.spp = spp;
        rtp::Settings sl = st; sl.block = block;
        rtp::LaunchPlan a = rtp::plan_begin(sc, st, count, frame, 256), b = rtp::plan_begin(sc, sl, count, list, 256);
        rtp::plan_finish(a, 2); rtp::plan_finish(b, 2);
        auto same = [&](const rtp::Pass &x, const rtp::Pass &y, int mode) {
            return y.mode == mode && x.lds == y.lds && x.count == y.count && x.tex == y.tex && x.block == y.block && x.grid == y.grid && x.lds_bytes == y.lds_bytes &&
                   x.chunk == y.chunk && x.park == y.park && x.park_l == y.park_l && x.park_l_lds == y.park_l_lds && x.lds_node_bytes == y.lds_node_bytes &&
                   x.k == y.k && x.total_waves == y.total_waves && x.yield_lanes == y.yield_lanes && x.leaf_wait == y.leaf_wait && x.refill_lanes == y.refill_lanes;
        };
        const int want_block = block == 256 ? 256 : 1024;
        bool ok = a.two_pass == b.two_pass && a.pixels == b.pixels && b.pixels == list.n && a.waves == b.waves && a.pool_bytes == b.pool_bytes &&
                  a.pairs_bytes == b.pairs_bytes && a.list_bytes == b.list_bytes && a.sort_bytes == b.sort_bytes && (a.error != nullptr) == (b.error != nullptr) &&
                  same(a.one, b.one, 6) && b.one.block == want_block;
        if (ok && b.two_pass && !b.error) ok = same(a.a, b.a, 7) && same(a.b, b.b, 8);
        if (!ok) { ++bad; std::printf("differs: tex %d big %d count %d spp %d passes %d block %d chunk %d max_w %d\n", tex, big, count, spp, passes, block, chunk, mw); }
    }
    std::printf("footprint plans: %d differ\n", bad);
    return bad != 0;
}
"""


def test_a_footprint_list_is_planned_as_a_frame_of_n_pixels(tmp_path):
    """rt_launch_plan.h on the CPU: for every combination of scene size, settings and list length a footprint list gets the plan of
    a one-row frame of as many pixels -- unit sizes, fused or two passes, placement, pools, workspace -- with modes 6 / 7 / 8 in
    place of 0 / 1 / 2, and a block of 512 threads runs as 1024."""
    src, exe = tmp_path / "plan_probe.cpp", str(tmp_path / "plan_probe")
    src.write_text(PLAN_PROBE)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "ray-tracing-fsharp_amd", "csrc"), str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    assert "footprint plans: 0 differ" in out.stdout
