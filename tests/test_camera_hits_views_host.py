"""rt_camera_hits_views and rt_camera_hits_views_device without a GPU: they are declared and bound, every refusal the header lists comes
with its status and its exact message before any device call and writes nothing, an argument error wins over a missing device, the two
no-ops, a valid call without a device fails loudly, and the Python wrapper refuses what it can see and shapes its outputs [K, n, n_samples]."""
import ctypes as C
import os

import numpy as np
import pytest

from test_views_host import _camera, _cams, _scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_W, MAX_H = 4, 3
FRAME = (2 * MAX_W + 1) * (2 * MAX_H + 1)
K = 3
ENTRY_POINTS = ("rt_camera_hits_views", "rt_camera_hits_views_device")


def test_prototypes_and_version(rt):
    from ray_tracing_fsharp_amd import _lib, raytracing
    header = open(os.path.join(ROOT, "include", "rtfs_amd.h")).read()
    assert "#define RT_ABI_VERSION 7" in header
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES
    assert rt.lib.rt_abi_version() == 7 == rt._abi.RT_ABI_VERSION
    assert len(raytracing._ROUTED) == 12 and "rt_camera_hits_views" not in raytracing._ROUTED  # (Scene.cameraHitsViews calls the pair itself)
    assert "7 camera hits over a batch of views" in header and "6 batch of views" in header  # rt_dev_last_launch_plan's kinds
    section = header[header.index("Camera hits over a batch of views"):header.index("int rt_camera_hits_views(")]
    assert "Scene.fs:62-91" in section and "Scene.fs:129-143" in section
    assert "ONE list shared by all views" in header and "RT_ERR_UNSUPPORTED: the batch kernels" in header
    assert hasattr(rt.Scene, "cameraHitsViews")


def _calls(rt, s, cams, k, n, px, hit, strike, rays, max_w=MAX_W, max_h=MAX_H, seeds=None, first=2, per=3, options=None, device=0):
    """Both entry points with the same arguments (the host variant takes no options)."""
    L = rt.lib
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None  # noqa: E731
    f64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None  # noqa: E731
    o = C.byref(options) if options is not None else None
    if options is None:
        yield lambda: L.rt_camera_hits_views(s, cams, k, max_w, max_h, seeds, 1, device, n, i32(px), first, per, 0, i32(hit), f64(strike), f64(rays), None)
    yield lambda: L.rt_camera_hits_views_device(s, cams, k, max_w, max_h, seeds, 1, device, n, p(px), first, per, 0, p(hit), p(strike), p(rays), None, o, None)


def test_invalid_arguments_are_refused_before_any_device_call(rt):
    A = rt._abi
    scene = _scene(rt)
    S = scene.handle
    n, per = 5, 3
    px = np.array([0, 7, FRAME - 1, 7, 30], np.int32)
    hit, strike, rays = np.full((K, n, per), 77, np.int32), np.full((K, n, per, 3), 7.5), np.full((K, n, per, 6), 7.5)
    bad = A.rt_render_options(block_threads=100)
    unset = A.rt_render_options(); unset.struct_size = 0
    spp, depth = "samples_per_pixel", "bounce_depth"
    slots = "more than INT32_MAX output slots (n * n_samples)"
    refusals = [
        (dict(s=None), "scene is NULL"),
        (dict(k=-1), "n_views must be >= 0"),
        (dict(cams=None), "cameras is NULL"),
        (dict(max_w=0), "max_width_coord and max_height_coord must be positive"),                    # geometry
        (dict(max_h=-2), "max_width_coord and max_height_coord must be positive"),
        (dict(max_w=(1 << 20) + 1), "image too large"),
        (dict(max_w=40000, max_h=40000), "a pixel list indexes frames of at most INT32_MAX pixels"),
        (dict(cams=_cams(rt, K, {(1, spp): 0})), "samples_per_pixel must be >= 1"),                  # a camera: the first offending view reports
        (dict(cams=_cams(rt, K, {(2, spp): 8000001})), "samples_per_pixel too large for int32 sums (255*spp)"),
        (dict(cams=_cams(rt, K, {(0, depth): -1})), "bounce_depth must be >= 0"),
        (dict(cams=_cams(rt, K, {(2, depth): 0x1000000, (1, spp): 0})), "samples_per_pixel must be >= 1"),  # (view 1 comes before view 2)
        (dict(cams=_cams(rt, K, {(2, depth): 0x1000000})), "bounce_depth too large"),
        (dict(first=-1), "sample_first must be >= 0"),                                               # the sample range
        (dict(per=0), "n_samples must be >= 1"),
        (dict(per=-4), "n_samples must be >= 1"),
        (dict(first=7999998, per=3), "sample_first + n_samples exceeds 8000000"),
        (dict(n=2**31, per=1), slots),                                                               # one view's slots
        (dict(n=2**63, per=2), slots),
        (dict(n=715827883, per=1), "more than INT32_MAX output slots (n_views * n * n_samples)"),    # the batch's: 3 * 715827883 = 2^31 + 1
        (dict(n=2**31 // (K * 7) + 1, per=7), "more than INT32_MAX output slots (n_views * n * n_samples)"),
        (dict(hit=None), "hit_index is NULL"),
        (dict(n=FRAME + 1, px=None), "pixels is NULL and n exceeds the frame's pixels"),
        (dict(options=bad), "block_threads must be 0, 256, 512, 768 or 1024"),
        (dict(options=unset), "rt_render_options.struct_size is not set"),
        (dict(options=A.rt_render_options(chunk_pixels=65)), "chunk_pixels must be in [0, 64]"),
    ]
    count = 0
    for device in (0, 99):  # an argument error wins over a device that does not exist
        for kw, message in refusals:
            args = dict(s=S, cams=_cams(rt), k=K, n=n, px=px, hit=hit, strike=strike, rays=rays, device=device)
            args.update(kw)
            for call in _calls(rt, args.pop("s"), args.pop("cams"), args.pop("k"), args.pop("n"), args.pop("px"), args.pop("hit"), args.pop("strike"),
                               args.pop("rays"), **args):
                assert call() == A.RT_ERR_INVALID_ARGUMENT, (kw, device)
                assert rt.lib.rt_last_error().decode() == message, (kw, device)
                assert (hit == 77).all() and (strike == 7.5).all() and (rays == 7.5).all()  # nothing written
                count += 1
    assert count == 2 * (22 * 2 + 3)
    # a HOST list with an entry outside the frame: the host variant refuses it on the host
    for entry in (-1, FRAME, -2**31, 2**31 - 1):
        lst = px.copy()
        lst[3] = entry
        assert next(iter(_calls(rt, S, _cams(rt), K, n, lst, hit, strike, rays, device=99)))() == A.RT_ERR_INVALID_ARGUMENT
        assert rt.lib.rt_last_error().decode() == "the pixel list has an entry outside the frame"
        assert (hit == 77).all() and (strike == 7.5).all() and (rays == 7.5).all()
    assert 3 * 715827883 == 2**31 + 1 and K * 7 * (2**31 // (K * 7) + 1) > 2**31 - 1 >= 7 * (2**31 // (K * 7) + 1)


def test_no_views_or_no_entries_is_a_no_op(rt):
    A = rt._abi
    scene = _scene(rt)
    L, S = rt.lib, scene.handle
    px = np.array([0, 7], np.int32)
    for k, n, cams, lst in ((0, 2, None, px), (0, 2, _cams(rt), px), (K, 0, _cams(rt), None), (0, 0, None, None)):
        for call in _calls(rt, S, cams, k, n, lst, None, None, None, device=99):  # (no device is asked for)
            assert call() == A.RT_OK, (k, n)
        i32 = lst.ctypes.data_as(C.POINTER(C.c_int32)) if lst is not None else None
        ptr = lst.ctypes.data_as(C.c_void_p) if lst is not None else None
        for call in (lambda st: L.rt_camera_hits_views(S, cams, k, MAX_W, MAX_H, None, 1, 0, n, i32, 0, 1, 0, None, None, None, C.byref(st)),
                     lambda st: L.rt_camera_hits_views_device(S, cams, k, MAX_W, MAX_H, None, 1, 0, n, ptr, 0, 1, 0, None, None, None, None, None, C.byref(st))):
            st = A.rt_stats(rays=5, samples=9, pixels=4, kernel_ms=3.0)
            assert call(st) == A.RT_OK
            assert st.rays == 0 and st.samples == 0 and st.pixels == 0 and st.kernel_ms == 0.0
    # an empty list is still checked for every view
    assert L.rt_camera_hits_views(S, _cams(rt), K, MAX_W, MAX_H, None, 1, 0, 0, None, 0, 0, 0, None, None, None, None) == A.RT_ERR_INVALID_ARGUMENT
    res = scene.cameraHitsViews(MAX_W, MAX_H, [], np.array([0, 7], np.int32), n_samples=3)
    assert res.hit_index.shape == (0, 2, 3) and res.strike.shape == (0, 2, 3, 3) and res.rays.shape == (0, 2, 3, 6) and res.stats["pixels"] == 0
    res = scene.cameraHitsViews(MAX_W, MAX_H, [_camera(rt)] * K, np.zeros(0, np.int32), n_samples=2, strike=False)
    assert res.hit_index.shape == (K, 0, 2) and res.hit_index.dtype == np.int32 and res.strike is None and res.rays.shape == (K, 0, 2, 6)
    assert res.rays.dtype == np.float64 and res.stats is scene.last_stats


def test_without_a_gpu_a_valid_batch_fails_loudly(rt):
    """A valid call -- the limits themselves included: sample_first + n_samples == 8000000, the whole frame without a list, cameras that
    differ in samples_per_pixel and bounce_depth, NULL strike and rays_out -- is past the argument checks and asks for the device."""
    if rt.device_count() > 0:
        pytest.skip("a GPU is visible")
    A = rt._abi
    scene = _scene(rt)
    cams = _cams(rt, K, {(1, "samples_per_pixel"): 7, (2, "bounce_depth"): 9})
    hit = np.full((K, FRAME, 2), 77, np.int32)
    for call in _calls(rt, scene.handle, cams, K, FRAME, None, hit, None, None, first=7999998, per=2):
        assert call() == A.RT_ERR_NO_DEVICE
        assert (hit == 77).all()
    for px in (np.array([0, 5, 9], np.int32), None):
        with pytest.raises(rt.RtError) as e:
            scene.cameraHitsViews(MAX_W, MAX_H, [_camera(rt), _camera(rt, spp=3)], px, seeds=[4, 5])
        assert e.value.code == A.RT_ERR_NO_DEVICE


def test_python_wrapper_checks_seeds_shapes_and_dtypes(rt):
    scene, cam = _scene(rt), _camera(rt)
    px = np.ones(3, np.int32)
    for seeds in ([1], [1, 2, 3], ()):
        with pytest.raises(ValueError, match="one seed per camera"):
            scene.cameraHitsViews(MAX_W, MAX_H, [cam, cam], px, seeds=seeds)
    for bad in (np.ones(3, np.int64), np.ones(3, np.uint32), np.ones(3, np.float64), [0, 1, 2]):
        with pytest.raises(TypeError):
            scene.cameraHitsViews(MAX_W, MAX_H, [cam, cam], bad)
    for bad in (np.ones((3, 1), np.int32), np.ones((2, 3), np.int32), np.array(3, np.int32)):  # (one list for all views: [n], never [K, n])
        with pytest.raises(ValueError):
            scene.cameraHitsViews(MAX_W, MAX_H, [cam, cam], bad)
    with pytest.raises(ValueError):  # options belong to the device entry
        scene.cameraHitsViews(MAX_W, MAX_H, [cam], px, options=rt._abi.rt_render_options(chunk_pixels=8))
    with pytest.raises(ValueError):  # n is for pixels=None
        scene.cameraHitsViews(MAX_W, MAX_H, [cam], px, n=3)
    with pytest.raises(TypeError):
        scene.cameraHitsViews(MAX_W, MAX_H, [cam], px, n_samples=2.0)
    # the library's own refusals arrive as RtError, and nothing as large as the refused batch is allocated first
    refused = [dict(pixels=np.array([0, -1, 2], np.int32)), dict(pixels=None, n=FRAME + 1), dict(pixels=px, sample_first=-1), dict(pixels=px, n_samples=0),
               dict(pixels=None, n=FRAME, n_samples=2**31 // (2 * FRAME) + 1)]
    for kw in refused:
        with pytest.raises(rt.RtError) as e:
            scene.cameraHitsViews(MAX_W, MAX_H, [cam, cam], kw.pop("pixels"), **kw)
        assert e.value.code == rt._abi.RT_ERR_INVALID_ARGUMENT


def build_camera_hits_views_smoke(tmp_path):
    import subprocess
    exe = str(tmp_path / "camera_hits_views_smoke")
    libdir = os.path.join(ROOT, "ray-tracing-fsharp_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "camera_hits_views_smoke.c"),
                           "-L", libdir, "-lrtfs_amd", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    return exe


def test_c_program_checks_the_batch_arguments(rt, tmp_path):
    """tests/c/camera_hits_views_smoke.c from C99: the argument checks hold without a GPU (with one, test_gpu_camera_hits_views compares
    what its one launch prints with single calls)."""
    import subprocess
    out = subprocess.run([build_camera_hits_views_smoke(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "camera hits views: argument checks ok" in out.stdout
