"""The device output stage as far as it goes without a GPU: the seven entry points are declared, exported and bound; the two length
functions against the oracle's own formatters; every refusal -- made before a device is entered, so it is tested here -- with its
status, its message and the proof that nothing was written; numpy inputs still take the host route, byte for byte; and the C consumer.
Expected bytes come from oracle.format_ppm / oracle.format_pixel_map, never from the library's host functions alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_ppm_max_bytes", "rt_pixel_map_bytes", "rt_gamma_correct_device", "rt_format_ppm_device", "rt_format_pixel_map_device",
       "rt_write_ppm_device", "rt_render_ppm")


def test_the_seven_symbols_are_declared_exported_and_bound(rt):
    from ray_tracing_fsharp_amd import _lib

    header = open(os.path.join(ROOT, "include", "rtfs_amd.h")).read()
    declared = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/rtfs_amd.h"
        assert hasattr(_lib.lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert "#define RT_ABI_VERSION 7" in header and rt.lib.rt_abi_version() == 7  # symbols only: no struct, field or symbol changed


def _images():
    rng = np.random.default_rng(16)
    return [rng.integers(0, 256, (r, c, 3), dtype=np.uint8) for r, c in ((1, 1), (1, 7), (7, 1), (13, 11), (3, 2))]


def test_ppm_max_bytes_bounds_the_oracle_text(rt, orc):
    for img in _images():
        for gamma in (False, True):
            assert rt.lib.rt_ppm_max_bytes(img.shape[0], img.shape[1]) >= len(orc.format_ppm(img, gamma=gamma))
    rng = np.random.default_rng(17)
    for r, c in ((1, 1), (13, 11), (3, 2)):  # every byte three digits: the bound is reached
        img = rng.integers(100, 256, (r, c, 3), dtype=np.uint8)
        assert rt.lib.rt_ppm_max_bytes(r, c) == len(orc.format_ppm(img, gamma=False))
    assert rt.lib.rt_ppm_max_bytes(1601, 2401) == 46128028
    assert rt.lib.rt_ppm_max_bytes(1, 2**31 - 1) == len(b"P3\n2147483647 1\n255\n") + 12 * (2**31 - 1) - 1


def test_pixel_map_bytes_is_the_oracle_length(rt, orc):
    for rows in (1, 2, 9, 10, 11, 12, 99, 100, 101, 102):
        for cols in (1, 2, 10, 11, 100, 101, 1000, 1001):
            assert rt.lib.rt_pixel_map_bytes(rows, cols) == len(orc.format_pixel_map(np.zeros((rows, cols, 3), np.uint8))), (rows, cols)


@pytest.mark.parametrize("fn", ["rt_ppm_max_bytes", "rt_pixel_map_bytes"])
def test_length_functions_refuse_bad_sizes(rt, fn):
    A = rt._abi
    for rows, cols, text in ((0, 3, "rows and cols must be positive"), (3, -1, "rows and cols must be positive"),
                             (65536, 65536, "an image of more than INT32_MAX pixels"), (2, 2**30, "an image of more than INT32_MAX pixels")):
        assert getattr(rt.lib, fn)(rows, cols) == -A.RT_ERR_INVALID_ARGUMENT
        assert rt.lib.rt_last_error().decode() == text


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


FORMAT_REFUSALS = (  # (d_rgb given, rows, cols, d_out given, capacity) -> message
    ((False, 2, 3, True, 256), "d_rgb is NULL"),
    ((True, 0, 3, True, 256), "rows and cols must be positive"),
    ((True, 2, -3, True, 256), "rows and cols must be positive"),
    ((True, 65536, 65536, True, 256), "an image of more than INT32_MAX pixels"),
    ((True, 2, 3, True, 0), "d_out is given but out_capacity is 0"),
    ((False, 0, 3, True, 0), "d_rgb is NULL"),  # two faults: the first one found decides
)


@pytest.mark.parametrize("which", ["ppm", "map"])
@pytest.mark.parametrize("case, text", FORMAT_REFUSALS)
def test_format_calls_refuse_before_any_device(rt, which, case, text):
    """The pointers are host arrays: a refused call must not touch them (and no device is needed to find that out)."""
    A = rt._abi
    has_rgb, rows, cols, has_out, cap = case
    rgb = np.full(18, 7, np.uint8)
    out = np.full(256, 0x5A, np.uint8)
    d_len = np.full(1, -7, np.int64)
    length = C.c_int64(-7)
    head = (99, _ptr(rgb) if has_rgb else None, rows, cols)  # device 99: a bad index would be reported only after the arguments
    tail = (_ptr(out) if has_out else None, cap, _ptr(d_len), None, C.byref(length))
    rc = rt.lib.rt_format_ppm_device(*head, 1, *tail) if which == "ppm" else rt.lib.rt_format_pixel_map_device(*head, *tail)
    assert rc == A.RT_ERR_INVALID_ARGUMENT and rt.lib.rt_last_error().decode() == text
    assert length.value == -7 and d_len[0] == -7 and (out == 0x5A).all() and (rgb == 7).all()


def test_gamma_write_and_render_refusals(rt, tmp_path):
    A = rt._abi
    rgb = np.full(18, 7, np.uint8)
    out = np.full(18, 0x5A, np.uint8)
    err = lambda: rt.lib.rt_last_error().decode()  # noqa: E731
    assert rt.lib.rt_gamma_correct_device(99, 18, None, _ptr(out), None) == A.RT_ERR_INVALID_ARGUMENT and err() == "d_in is NULL"
    assert rt.lib.rt_gamma_correct_device(99, 18, _ptr(rgb), None, None) == A.RT_ERR_INVALID_ARGUMENT and err() == "d_out is NULL"
    assert rt.lib.rt_gamma_correct_device(99, 0, None, None, None) == A.RT_OK
    good, bad = str(tmp_path / "x.ppm").encode(), str(tmp_path / "missing" / "x.ppm").encode()
    w = rt.lib.rt_write_ppm_device
    assert w(None, 99, _ptr(rgb), 2, 3, 1, None) == A.RT_ERR_INVALID_ARGUMENT and err() == "path is NULL"
    assert w(good, 99, None, 2, 3, 1, None) == A.RT_ERR_INVALID_ARGUMENT and err() == "d_rgb is NULL"
    assert w(good, 99, _ptr(rgb), 2, 0, 1, None) == A.RT_ERR_INVALID_ARGUMENT and err() == "rows and cols must be positive"
    assert w(good, 99, _ptr(rgb), 65536, 65536, 1, None) == A.RT_ERR_INVALID_ARGUMENT and err() == "an image of more than INT32_MAX pixels"
    assert not os.path.exists(good)  # refused before the file is opened
    assert w(bad, 99, _ptr(rgb), 2, 3, 1, None) == A.RT_ERR_IO and err() == "cannot open " + bad.decode()
    assert (out == 0x5A).all() and (rgb == 7).all()

    objs, cam, mw, mh = rt.sample_images.config1_empty()
    scene, cam_abi = rt.Scene.make(objs), cam.to_abi()
    st = A.rt_stats()
    C.memset(C.byref(st), 0x55, C.sizeof(st))
    r = rt.lib.rt_render_ppm

    def call(scene_h=scene.handle, camera=cam_abi, w_=3, h_=2, path=good, options=None):
        return r(scene_h, C.byref(camera) if camera is not None else None, w_, h_, 5, 99, 0, 1, path, C.byref(options) if options is not None else None,
                 C.byref(st))

    # rt_render's own check list, in rt_render_device_ex's order (scene, camera, geometry, options), then the path
    assert call(scene_h=None) == A.RT_ERR_INVALID_ARGUMENT and err() == "scene is NULL"
    assert call(camera=None) == A.RT_ERR_INVALID_ARGUMENT and err() == "camera is NULL"
    assert call(w_=0) == A.RT_ERR_INVALID_ARGUMENT and err() == "max_width_coord and max_height_coord must be positive"
    assert call(h_=(1 << 20) + 1) == A.RT_ERR_INVALID_ARGUMENT and err() == "image too large"
    no_samples = cam.to_abi()
    no_samples.samples_per_pixel = 0
    assert call(camera=no_samples) == A.RT_ERR_INVALID_ARGUMENT and err() == "samples_per_pixel must be >= 1"
    deep = cam.to_abi()
    deep.bounce_depth = -1
    assert call(camera=deep) == A.RT_ERR_INVALID_ARGUMENT and err() == "bounce_depth must be >= 0"
    opt = A.rt_render_options()
    opt.struct_size = C.sizeof(opt)
    opt.block_threads = 100
    assert call(options=opt) == A.RT_ERR_INVALID_ARGUMENT
    assert call(path=None) == A.RT_ERR_INVALID_ARGUMENT and err() == "path is NULL"
    assert call(w_=1 << 20, h_=1 << 20) == A.RT_ERR_INVALID_ARGUMENT and err() == "an image of more than INT32_MAX pixels"
    assert not os.path.exists(good)
    assert call(path=bad) == A.RT_ERR_IO and err() == "cannot open " + bad.decode()
    assert bytes(st)[:8] == b"\x55" * 8


def test_without_a_device_valid_calls_say_so(rt, tmp_path):
    """After the argument checks: RT_ERR_NO_DEVICE, never a fallback to the host formatter."""
    if rt.device_count() > 0:
        pytest.skip("a GPU is visible")
    A = rt._abi
    rgb = np.full(18, 7, np.uint8)
    out = np.full(256, 0x5A, np.uint8)
    length = C.c_int64(-7)
    path = str(tmp_path / "x.ppm").encode()
    assert rt.lib.rt_format_ppm_device(0, _ptr(rgb), 2, 3, 1, _ptr(out), 256, None, None, C.byref(length)) == A.RT_ERR_NO_DEVICE
    assert rt.lib.rt_format_pixel_map_device(0, _ptr(rgb), 2, 3, _ptr(out), 256, None, None, C.byref(length)) == A.RT_ERR_NO_DEVICE
    assert rt.lib.rt_format_ppm_device(0, _ptr(rgb), 2, 3, 1, None, 0, None, None, C.byref(length)) == A.RT_ERR_NO_DEVICE  # length only
    assert rt.lib.rt_gamma_correct_device(0, 18, _ptr(rgb), _ptr(out), None) == A.RT_ERR_NO_DEVICE
    assert rt.lib.rt_write_ppm_device(path, 0, _ptr(rgb), 2, 3, 1, None) == A.RT_ERR_NO_DEVICE
    assert "no CPU fallback" in rt.lib.rt_last_error().decode()
    objs, cam, mw, mh = rt.sample_images.config1_empty()
    with pytest.raises(rt.RtError) as e:
        rt.Scene.make(objs).renderPpm(3, 2, cam, str(tmp_path / "y.ppm"))
    assert e.value.code == A.RT_ERR_NO_DEVICE
    assert length.value == -7 and (out == 0x5A).all()


def test_numpy_inputs_keep_the_host_route(rt, orc, tmp_path):
    for img in _images():
        for gamma in (False, True):
            want = orc.format_ppm(img, gamma=gamma)
            assert rt.ImageOutput.formatPpm(gamma, img) == want
            path = str(tmp_path / "host.ppm")
            ticks = []
            rt.ImageOutput.writePpm(gamma, ticks.append, img, path)
            assert open(path, "rb").read() == want and len(ticks) == img.shape[0] * img.shape[1]
        assert rt.ImageOutput.formatPixelMap(img) == orc.format_pixel_map(img)
        corrected = rt.PixelOutput.correctImage(img)
        assert corrected.dtype == np.uint8 and corrected.shape == img.shape
        assert corrected.tolist() == [[[orc.gamma_correct(int(b)) for b in px] for px in row] for row in img]


def build_output_smoke(tmp_path):
    exe = str(tmp_path / "output_smoke")
    libdir = os.path.join(ROOT, "ray-tracing-fsharp_amd")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "output_smoke.c"),
                           "-L", libdir, "-lrtfs_amd", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    return exe


def test_c_program_checks_the_output_refusals(rt, tmp_path):
    """tests/c/output_smoke.c from C99 -pedantic: host arithmetic and refusals hold without a GPU (with one, test_gpu_output.py holds what it
    formats against the golden text)."""
    out = subprocess.run([build_output_smoke(tmp_path), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "output: refusals ok" in out.stdout
