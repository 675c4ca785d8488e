"""Resuming from a pixel map, as far as it goes without a GPU: every refusal of rt_parse_pixel_map_device, rt_missing_pixels_device,
rt_scatter_pixels_device, rt_resume_pixel_map and rt_resume_png / rt_resume_ppm (the argument checks come before the device check, so
they run here, and write nothing), RT_ERR_NO_DEVICE for what remains, and csrc/rt_pixel_map.h's chunked parse driven on a CPU against
the sequential reader -- plainly and under the sanitizers -- on the records of pixel_map_cases.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pixel_map_cases as pmc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_parse_pixel_map_device", "rt_missing_pixels_device", "rt_scatter_pixels_device", "rt_resume_pixel_map", "rt_resume_png", "rt_resume_ppm",
       "rt_pixel_map_chunk_bytes", "rt_pixel_map_tile_bytes", "rt_pixel_map_scan_tiles")
S = 0x5A  # the sentinel every output is filled with


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _err(rt):
    return rt.lib.rt_last_error().decode()


def test_the_symbols_are_declared_exported_and_bound(rt):
    from ray_tracing_fsharp_amd import _lib

    header = open(os.path.join(ROOT, "include", "rtfs_amd.h")).read()
    declared = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/rtfs_amd.h"
        assert hasattr(_lib.lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert "#define RT_ABI_VERSION 7" in header and rt.lib.rt_abi_version() == 7  # symbols only
    consts = open(os.path.join(ROOT, "ray-tracing-fsharp_amd", "csrc", "rt_pixel_map.h")).read()
    chunk, block = (int(re.search(rf"#define {n} (\d+)", consts).group(1)) for n in ("RPM_CHUNK_BYTES", "RPM_BLOCK"))
    assert rt.lib.rt_pixel_map_chunk_bytes() == chunk and rt.lib.rt_pixel_map_tile_bytes() == chunk * block
    assert rt.lib.rt_pixel_map_scan_tiles() == int(re.search(r"#define RPM_SCAN_THREADS (\d+)", consts).group(1))


PARSE_REFUSALS = (  # (data given, n_bytes, rows, cols, rgb given, present given) -> status, message
    ((False, 8, 2, 3, True, True), "RT_ERR_INVALID_ARGUMENT", "the pixel map's bytes are NULL"),
    ((True, 8, 0, 3, True, True), "RT_ERR_INVALID_ARGUMENT", "rows and cols must be positive"),
    ((True, 8, 2, -3, True, True), "RT_ERR_INVALID_ARGUMENT", "rows and cols must be positive"),
    ((True, 8, 65536, 65536, True, True), "RT_ERR_INVALID_ARGUMENT", "an image of more than INT32_MAX pixels"),
    ((True, 8, 2, 3, False, True), "RT_ERR_INVALID_ARGUMENT", "d_rgb is NULL"),
    ((True, 8, 2, 3, True, False), "RT_ERR_INVALID_ARGUMENT", "d_present is NULL"),
    ((True, (1 << 31), 2, 3, True, True), "RT_ERR_UNSUPPORTED", "a pixel map of more than INT32_MAX bytes"),
    ((True, (1 << 31), 2, 3, False, True), "RT_ERR_INVALID_ARGUMENT", "d_rgb is NULL"),  # two faults: the first one found decides
)


@pytest.mark.parametrize("case, status, text", PARSE_REFUSALS)
def test_parse_refuses_before_any_device(rt, case, status, text):
    has_data, n, rows, cols, has_rgb, has_present = case
    data = np.frombuffer(b",\nabc,1\n", np.uint8).copy()
    rgb, present, d_count = np.full(18, S, np.uint8), np.full(6, S, np.uint8), np.full(1, -7, np.int64)
    count = C.c_int64(-7)
    rc = rt.lib.rt_parse_pixel_map_device(99, _ptr(data) if has_data else None, n, rows, cols, _ptr(rgb) if has_rgb else None,
                                          _ptr(present) if has_present else None, _ptr(d_count), None, C.byref(count))
    assert rc == getattr(rt._abi, status) and _err(rt) == text
    assert count.value == -7 and d_count[0] == -7 and (rgb == S).all() and (present == S).all()


MISSING_REFUSALS = (  # (present given, rows, cols, pixels given, capacity)
    ((False, 2, 3, True, 6), "d_present is NULL"),
    ((True, 0, 3, True, 6), "rows and cols must be positive"),
    ((True, 65536, 65536, True, 6), "an image of more than INT32_MAX pixels"),
    ((True, 2, 3, True, 0), "d_pixels is given but capacity is 0"),
)


@pytest.mark.parametrize("case, text", MISSING_REFUSALS)
def test_missing_pixels_refuses_before_any_device(rt, case, text):
    has_present, rows, cols, has_pixels, cap = case
    present, pixels, d_n = np.zeros(6, np.uint8), np.full(6, -7, np.int32), np.full(1, -7, np.int64)
    n = C.c_int64(-7)
    rc = rt.lib.rt_missing_pixels_device(99, _ptr(present) if has_present else None, rows, cols, _ptr(pixels) if has_pixels else None, cap, _ptr(d_n), None,
                                         C.byref(n))
    assert rc == rt._abi.RT_ERR_INVALID_ARGUMENT and _err(rt) == text
    assert n.value == -7 and d_n[0] == -7 and (pixels == -7).all()


SCATTER_REFUSALS = (  # (n, pixels given, list given, rows, cols, frame given)
    ((2, False, True, 2, 3, True), "d_pixels is NULL"),
    ((2, True, False, 2, 3, True), "d_rgb_list is NULL"),
    (((1 << 31), True, True, 2, 3, True), "more than INT32_MAX list entries"),
    ((2, True, True, 2, 0, True), "rows and cols must be positive"),
    ((2, True, True, 65536, 65536, True), "an image of more than INT32_MAX pixels"),
    ((2, True, True, 2, 3, False), "d_rgb_frame is NULL"),
    ((0, False, False, 2, 3, False), "d_rgb_frame is NULL"),
)


@pytest.mark.parametrize("case, text", SCATTER_REFUSALS)
def test_scatter_pixels_refuses_before_any_device(rt, case, text):
    n, has_pixels, has_list, rows, cols, has_frame = case
    pixels, lst, frame = np.array([1, 4], np.int32), np.full(6, 9, np.uint8), np.full(18, S, np.uint8)
    rc = rt.lib.rt_scatter_pixels_device(99, n, _ptr(pixels) if has_pixels else None, _ptr(lst) if has_list else None, rows, cols,
                                         _ptr(frame) if has_frame else None, None)
    assert rc == rt._abi.RT_ERR_INVALID_ARGUMENT and _err(rt) == text
    assert (frame == S).all()


def test_an_empty_scatter_is_a_no_op_without_a_device(rt):
    frame = np.full(18, S, np.uint8)
    assert rt.lib.rt_scatter_pixels_device(99, 0, None, None, 2, 3, _ptr(frame), None) == rt._abi.RT_OK and (frame == S).all()


def _scene_and_camera(rt):
    objs, cam, _, _ = rt.sample_images.config1_empty()
    return rt.Scene.make(objs), cam.to_abi()


def test_resume_refusals(rt, tmp_path):
    A = rt._abi
    scene, cam_abi = _scene_and_camera(rt)
    data = b",\nabc"
    rgb = np.full(7 * 5 * 3, S, np.uint8)
    st = A.rt_stats()
    C.memset(C.byref(st), 0x55, C.sizeof(st))

    def call(scene_h=scene.handle, camera=cam_abi, w_=3, h_=2, data_=data, n=len(data), out=rgb, options=None):
        return rt.lib.rt_resume_pixel_map(scene_h, C.byref(camera) if camera is not None else None, w_, h_, 5, 99, 0, data_, n, out.ctypes.data_as(C.POINTER(C.c_uint8)) if out is not None else None,
                                          options, C.byref(st))

    # rt_render's check list in its order, then the map, then the frame a pixel list can index, then this call's buffer and the size
    assert call(scene_h=None) == A.RT_ERR_INVALID_ARGUMENT and _err(rt) == "scene is NULL"
    assert call(camera=None) == A.RT_ERR_INVALID_ARGUMENT and _err(rt) == "camera is NULL"
    assert call(w_=0) == A.RT_ERR_INVALID_ARGUMENT and _err(rt) == "max_width_coord and max_height_coord must be positive"
    assert call(h_=(1 << 20) + 1) == A.RT_ERR_INVALID_ARGUMENT and _err(rt) == "image too large"
    bad_cam = type(cam_abi).from_buffer_copy(cam_abi)
    bad_cam.samples_per_pixel = 0
    assert call(camera=bad_cam) == A.RT_ERR_INVALID_ARGUMENT and _err(rt) == "samples_per_pixel must be >= 1"
    bad_cam.samples_per_pixel, bad_cam.bounce_depth = 4, -1
    assert call(camera=bad_cam) == A.RT_ERR_INVALID_ARGUMENT and _err(rt) == "bounce_depth must be >= 0"
    opts = A.rt_render_options()
    opts.struct_size = 0
    assert call(options=C.byref(opts)) == A.RT_ERR_INVALID_ARGUMENT and _err(rt) == "rt_render_options.struct_size is not set"
    assert call(data_=None) == A.RT_ERR_INVALID_ARGUMENT and _err(rt) == "the pixel map's bytes are NULL"
    assert call(w_=1 << 20, h_=1 << 20) == A.RT_ERR_INVALID_ARGUMENT and _err(rt) == "a pixel list indexes frames of at most INT32_MAX pixels"
    assert call(out=None) == A.RT_ERR_INVALID_ARGUMENT and _err(rt) == "rgb_out is NULL"
    assert call(n=1 << 31) == A.RT_ERR_UNSUPPORTED and _err(rt) == "a pixel map of more than INT32_MAX bytes"
    assert (rgb == S).all() and bytes(st)[:8] == b"\x55" * 8


@pytest.mark.parametrize("fn, ext", [("rt_resume_png", "png"), ("rt_resume_ppm", "ppm")])
def test_resume_file_refusals(rt, tmp_path, fn, ext):
    A = rt._abi
    scene, cam_abi = _scene_and_camera(rt)
    spill = tmp_path / "spill.bin"
    spill.write_bytes(b",\nabc")
    good_map, no_map = str(spill).encode(), str(tmp_path / "missing.bin").encode()
    good, bad = str(tmp_path / f"x.{ext}").encode(), str(tmp_path / "missing" / f"x.{ext}").encode()
    st = A.rt_stats()
    C.memset(C.byref(st), 0x55, C.sizeof(st))

    def call(scene_h=scene.handle, camera=cam_abi, w_=3, h_=2, map_path=good_map, path=good):
        return getattr(rt.lib, fn)(scene_h, C.byref(camera) if camera is not None else None, w_, h_, 5, 99, 0, map_path, 1, path, None, C.byref(st))

    # rt_render_png's order: the arguments, then both files (RT_ERR_IO before any device work), then the device
    assert call(scene_h=None) == A.RT_ERR_INVALID_ARGUMENT and _err(rt) == "scene is NULL"
    assert call(camera=None) == A.RT_ERR_INVALID_ARGUMENT and _err(rt) == "camera is NULL"
    assert call(w_=0) == A.RT_ERR_INVALID_ARGUMENT and _err(rt) == "max_width_coord and max_height_coord must be positive"
    assert call(map_path=None) == A.RT_ERR_INVALID_ARGUMENT and _err(rt) == "map_path is NULL"
    assert call(path=None) == A.RT_ERR_INVALID_ARGUMENT and _err(rt) == "out_path is NULL"
    assert call(w_=1 << 20, h_=1 << 20) == A.RT_ERR_INVALID_ARGUMENT
    if ext == "png":
        assert call(w_=13500, h_=13500) == A.RT_ERR_UNSUPPORTED
    assert call(map_path=no_map) == A.RT_ERR_IO and _err(rt) == "cannot open " + no_map.decode()
    assert not os.path.exists(good)  # an unreadable map: the output is not even created
    assert call(path=bad) == A.RT_ERR_IO and _err(rt) == "cannot open " + bad.decode()
    assert call(map_path=str(tmp_path).encode()) == A.RT_ERR_IO  # a directory opens, and cannot be read
    assert bytes(st)[:8] == b"\x55" * 8 and spill.read_bytes() == b",\nabc"


def test_without_a_device_valid_calls_say_so(rt, tmp_path):
    """After the argument checks: RT_ERR_NO_DEVICE, never a fallback to the host reader."""
    if rt.device_count() > 0:
        pytest.skip("a GPU is visible")
    A = rt._abi
    data = np.frombuffer(b",\nabc,1\n", np.uint8).copy()
    rgb, present, pixels = np.full(18, S, np.uint8), np.full(6, S, np.uint8), np.full(6, -7, np.int32)
    count = C.c_int64(-7)
    assert rt.lib.rt_parse_pixel_map_device(0, _ptr(data), 8, 2, 3, _ptr(rgb), _ptr(present), None, None, C.byref(count)) == A.RT_ERR_NO_DEVICE
    assert rt.lib.rt_parse_pixel_map_device(0, None, 0, 2, 3, _ptr(rgb), _ptr(present), None, None, C.byref(count)) == A.RT_ERR_NO_DEVICE  # an empty map
    assert rt.lib.rt_missing_pixels_device(0, _ptr(present), 2, 3, _ptr(pixels), 6, None, None, C.byref(count)) == A.RT_ERR_NO_DEVICE
    assert rt.lib.rt_scatter_pixels_device(0, 2, _ptr(pixels), _ptr(rgb), 2, 3, _ptr(rgb), None) == A.RT_ERR_NO_DEVICE
    assert "no CPU fallback" in _err(rt)
    assert count.value == -7 and (rgb == S).all() and (present == S).all() and (pixels == -7).all()
    objs, cam, _, _ = rt.sample_images.config1_empty()
    scene = rt.Scene.make(objs)
    with pytest.raises(rt.RtError) as e:
        scene.resume(3, 2, cam, b",\nabc")
    assert e.value.code == A.RT_ERR_NO_DEVICE
    spill = tmp_path / "spill.bin"
    spill.write_bytes(b",\nabc")
    for method, name in ((scene.resumePng, "y.png"), (scene.resumePpm, "y.ppm")):
        with pytest.raises(rt.RtError) as e:
            method(3, 2, cam, str(spill), str(tmp_path / name))
        assert e.value.code == A.RT_ERR_NO_DEVICE


def test_read_pixel_map_keeps_its_host_route(rt, orc, tmp_path):
    """ImageOutput.readPixelMap is existing behaviour: numpy results from the host reader, with or without a GPU."""
    for name, rows, cols, data in pmc.small_files()[:8]:
        path = tmp_path / "spill.bin"
        path.write_bytes(data)
        rgb, present = rt.ImageOutput.readPixelMap(str(path), rows, cols)
        n, orgb, opresent = pmc.expected(orc, data, rows, cols)
        assert isinstance(rgb, np.ndarray) and np.array_equal(rgb, orgb) and np.array_equal(present, opresent), name


# ---- the header alone ------------------------------------------------------------------------------------------------------------------
def _table_cases():
    return ([(r, c, d, True) for _, r, c, d in pmc.small_files()] + [(r, c, d, False) for _, r, c, d in pmc.long_files()] +
            [(f[1], f[2], f[3], True) for f in pmc.malformed_files()])


def test_the_cases_are_what_they_claim(orc):
    """Every case is accepted by the reference reader (the malformed ones refused), and the variants do what their names say."""
    for name, rows, cols, data in pmc.small_files() + pmc.long_files():
        n, rgb, present = pmc.expected(orc, data, rows, cols)
        assert n > 0 and present.any(), name
        if name.endswith("duplicated"):
            assert n > int(present.sum()), name
        if name.endswith("dropped") and n > 2:
            whole = [d for m, _, _, d in pmc.small_files() + pmc.long_files() if m == name.replace("dropped", "whole")][0]
            assert int(pmc.expected(orc, whole, rows, cols)[2].sum()) > int(present.sum()), name
    for f in pmc.malformed_files():
        assert pmc.expected(orc, f[3], f[1], f[2])[0] == -1, f[0]
    assert any(len(d) > 2 * 4096 for _, _, _, d in pmc.long_files())


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_the_chunked_parse_is_the_sequential_reader(tmp_path, sanitize):
    """tests/c/pixel_map_scan_table.cpp: csrc/rt_pixel_map.h's maps, scan and owner-computes re-walk against rth::parse_pixel_map -- count,
    record starts, rgb and present -- for every chunk size from 1 to twice the device's and two tile sizes; a stand-alone program, built once
    plainly and once with -fsanitize=address,undefined.  (rt_scene.h reads the HIP headers, so the host compiler is hipcc's, host only.)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe, cases = str(tmp_path / "pixel_map_scan_table"), str(tmp_path / "cases.bin")
    pmc.write_table_input(cases, _table_cases())
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-O1"] + flags +
                          ["-o", exe, os.path.join(ROOT, "tests", "c", "pixel_map_scan_table.cpp")])
    out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split() == ["composition", "ok", "short_strings", "ok", "overflow", "ok", "cases", "ok", f"({len(_table_cases())})"]
