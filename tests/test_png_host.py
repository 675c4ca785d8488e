"""Png.write (ImageOutput.fs:214-251) as far as it goes without a GPU: the host formatter rt_format_png / rt_write_png, the length
functions, every refusal of the device calls, the Python Png paths for numpy images, csrc/rt_png.h driven alone under the sanitizers, and
the C consumer.  Skia's bytes cannot be reproduced, so the PIXELS are held: every file must be a valid PNG that the tests' own decoder and
PIL (png_cases.decode) turn back into exactly oracle.gamma_correct of the image, or the image itself when gamma is off."""
import ctypes as C
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import png_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_format_png", "rt_write_png", "rt_png_max_bytes", "rt_png_tile_bytes", "rt_format_png_device", "rt_write_png_device", "rt_render_png")
SENTINEL = 0xA5


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def host_png(rt, img, gamma=False):
    """rt_format_png into a buffer of rt_png_max_bytes + 64 sentinel bytes: the file; nothing behind its length is touched."""
    img = np.ascontiguousarray(img, np.uint8)
    rows, cols = img.shape[0], img.shape[1]
    cap = rt.lib.rt_png_max_bytes(rows, cols)
    assert cap > 0
    buf = np.full(cap + 64, SENTINEL, np.uint8)
    n = rt.lib.rt_format_png(_u8(img), rows, cols, int(gamma), buf.ctypes.data, cap)
    assert 68 < n <= cap, rt.lib.rt_last_error()
    assert (buf[n:] == SENTINEL).all(), "bytes at or beyond the length were written"
    assert rt.lib.rt_format_png(_u8(img), rows, cols, int(gamma), None, 0) == n  # the length-only call
    return buf[:n].tobytes()


def check_file(rt, orc, data, img, gamma, block_types=None):
    """A valid PNG of exactly the expected pixels, made of one byte-aligned block per tile."""
    px, idat = pc.decode(data)
    want = pc.expected_pixels(orc, img, gamma)
    assert px.shape == want.shape and np.array_equal(px, want)
    T = rt.lib.rt_png_tile_bytes()
    types = pc.tile_block_types(idat, img.shape[0] * (1 + 3 * img.shape[1]), T)
    if block_types is not None:
        assert types == block_types
    return types


def test_the_seven_symbols_are_declared_exported_and_bound(rt):
    from ray_tracing_fsharp_amd import _lib

    header = open(os.path.join(ROOT, "include", "rtfs_amd.h")).read()
    declared = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/rtfs_amd.h"
        assert hasattr(_lib.lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert "#define RT_ABI_VERSION 7" in header and rt.lib.rt_abi_version() == 7  # symbols only
    consts = open(os.path.join(ROOT, "ray-tracing-fsharp_amd", "csrc", "rt_launch_consts.h")).read()
    assert int(re.search(r"#define RTO_PNG_TILE_BYTES (\d+)", consts).group(1)) == rt.lib.rt_png_tile_bytes()


# ---- decoding ------------------------------------------------------------------------------------------------------------------------
def _decoding_images():
    return [("golden-2x3", pc.GOLDEN_IMAGE), ("every-byte", pc.every_byte_image())] + list(pc.golden_frames())


@pytest.mark.parametrize("gamma", [False, True])
@pytest.mark.parametrize("name", [n for n, _ in _decoding_images()])
def test_files_decode_to_their_pixels(rt, orc, name, gamma):
    img = dict(_decoding_images())[name]
    check_file(rt, orc, host_png(rt, img, gamma), img, gamma)


def test_the_container_is_the_one_the_header_defines(rt):
    data = host_png(rt, pc.GOLDEN_IMAGE)
    names = [n for n, _ in pc.chunks(data)]
    assert names == [b"IHDR", b"IDAT", b"IEND"]
    assert pc.chunks(data)[0][1] == (3).to_bytes(4, "big") + (2).to_bytes(4, "big") + bytes([8, 2, 0, 0, 0])
    raw = zlib.decompress(pc.chunks(data)[1][1])
    assert raw[0] == 1 and raw[10] == 1  # every row is filter type 1 (Sub)
    assert list(raw[1:10]) == [255, 0, 0, 1, 255, 0, 0, 1, 255]  # x[j] - x[j-3] mod 256


# ---- shapes, runs, histograms --------------------------------------------------------------------------------------------------------
T0 = 16384  # the cases are generated for the intended tile size; the first test holds the library to it


def test_tile_bytes_is_the_value_the_cases_are_built_for(rt):
    assert rt.lib.rt_png_tile_bytes() == T0


@pytest.mark.parametrize("name", [n for n, _ in pc.shape_cases(T0)])
def test_shapes(rt, orc, name):
    img = dict(pc.shape_cases(T0))[name]
    gamma = img.shape[1] % 2 == 1
    check_file(rt, orc, host_png(rt, img, gamma), img, gamma)


@pytest.mark.parametrize("name", [n for n, _ in pc.run_cases(T0)])
def test_runs(rt, orc, name):
    img = dict(pc.run_cases(T0))[name]
    data = host_png(rt, img)
    types = check_file(rt, orc, data, img, False)
    if name == "tile-of-one-run":
        assert len(types) == 3 and types[1] != 0 and len(data) < 68 + 2 * (T0 + 5) + 64  # the middle tile is a handful of bytes
    if name == "run-lengths":  # 4 bytes and more of one value are cheaper than their literals
        assert len(data) < 68 + 700


@pytest.mark.parametrize("name", [n for n, _, _ in pc.histogram_cases(T0)])
def test_histograms(rt, orc, name):
    img, want_type = {n: (i, t) for n, i, t in pc.histogram_cases(T0)}[name]
    data = host_png(rt, img)
    types = check_file(rt, orc, data, img, False)
    assert len(types) == 1 and (want_type is None or types[0] == want_type)
    body = pc.decode(data)[1][2:]
    if name == "uniform":
        assert len(data) == rt.lib.rt_png_max_bytes(1, img.shape[1])
    if name == "no-match":  # a dynamic block without a distance code: HDIST = 1 (the field 0), and the decoders above accepted it
        assert types[0] == 2 and body[1] & 31 == 0
    if name == "single-literal":  # 16384 equal bytes: a literal, 63 matches of 258 and one of 129 -- under 40 bytes of deflate
        assert types[0] != 0 and len(data) < 68 + 40


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------
def test_capacity_rule(rt):
    A = rt._abi
    img = pc.noise(13, 11, 3)
    data = host_png(rt, img)
    n = len(data)
    buf = np.full(n + 64, SENTINEL, np.uint8)
    assert rt.lib.rt_format_png(_u8(img), 13, 11, 0, buf.ctypes.data, n - 1) == -A.RT_ERR_INVALID_ARGUMENT
    assert rt.lib.rt_last_error().decode() == f"out_capacity {n - 1} below the {n} bytes needed"
    assert (buf == SENTINEL).all()
    assert rt.lib.rt_format_png(_u8(img), 13, 11, 0, buf.ctypes.data, 1) == -A.RT_ERR_INVALID_ARGUMENT and (buf == SENTINEL).all()
    assert rt.lib.rt_format_png(_u8(img), 13, 11, 0, buf.ctypes.data, n) == n  # exactly the length
    assert buf[:n].tobytes() == data and (buf[n:] == SENTINEL).all()


def test_max_bytes_is_met_by_an_all_stored_image_and_never_passed(rt):
    T = rt.lib.rt_png_tile_bytes()
    for rows, cols in ((1, 1), (2, 3), (37, 211), (1, 5461), (2, 5461), (3, 5461)):
        flen = rows * (1 + 3 * cols)
        assert rt.lib.rt_png_max_bytes(rows, cols) == 68 + flen + 5 * -(-flen // T)
    img = pc.noise(37, 211, 9)  # noise: no code beats 8 bits a byte, every tile is stored
    data = host_png(rt, img)
    assert len(data) == rt.lib.rt_png_max_bytes(37, 211)
    assert set(pc.tile_block_types(pc.decode(data)[1], 37 * (1 + 3 * 211), T)) == {0}
    assert rt.lib.rt_png_max_bytes(1601, 2401) == 68 + 1601 * 7204 + 5 * -(-1601 * 7204 // T)


def test_a_black_image_is_a_twentieth_of_its_raw_size(rt, orc):
    """Derivable: a row is the literals 1 and 0 and a match -- under fixed codes 8 + 8 + 13 bits for 193 bytes."""
    img = np.zeros((64, 64, 3), np.uint8)
    for gamma in (False, True):
        data = host_png(rt, img, gamma)
        check_file(rt, orc, data, img, gamma)
        assert len(data) * 20 <= img.size


def test_length_functions_and_host_calls_refuse_bad_sizes(rt, tmp_path):
    A = rt._abi
    err = lambda: rt.lib.rt_last_error().decode()  # noqa: E731
    rgb = np.full(18, 7, np.uint8)
    out = np.full(256, 0x5A, np.uint8)
    for rows, cols, text in ((0, 3, "rows and cols must be positive"), (3, -1, "rows and cols must be positive"),
                             (65536, 65536, "an image of more than INT32_MAX pixels")):
        assert rt.lib.rt_png_max_bytes(rows, cols) == -A.RT_ERR_INVALID_ARGUMENT and err() == text
        assert rt.lib.rt_format_png(_u8(rgb), rows, cols, 0, out.ctypes.data, 256) == -A.RT_ERR_INVALID_ARGUMENT and err() == text
        assert rt.lib.rt_write_png(str(tmp_path / "x.png").encode(), _u8(rgb), rows, cols, 0) == A.RT_ERR_INVALID_ARGUMENT and err() == text
    # the worst-case IDAT must fit a 31-bit chunk length
    assert rt.lib.rt_png_max_bytes(23000, 31000) > 0
    for rows, cols in ((27000, 27000), (1, 2**31 - 1), (2**31 - 1, 1)):
        assert rt.lib.rt_png_max_bytes(rows, cols) == -A.RT_ERR_UNSUPPORTED and err() == "an image whose PNG data may pass 2^31 - 1 bytes"
        assert rt.lib.rt_format_png(_u8(rgb), rows, cols, 0, out.ctypes.data, 256) == -A.RT_ERR_UNSUPPORTED
        assert rt.lib.rt_write_png(str(tmp_path / "x.png").encode(), _u8(rgb), rows, cols, 0) == A.RT_ERR_UNSUPPORTED
    assert rt.lib.rt_format_png(None, 2, 3, 0, out.ctypes.data, 256) == -A.RT_ERR_INVALID_ARGUMENT
    assert rt.lib.rt_write_png(None, _u8(rgb), 2, 3, 0) == A.RT_ERR_INVALID_ARGUMENT
    bad = str(tmp_path / "missing" / "x.png").encode()
    assert rt.lib.rt_write_png(bad, _u8(rgb), 2, 3, 0) == A.RT_ERR_IO and err() == "cannot open " + bad.decode()
    assert (out == 0x5A).all() and (rgb == 7).all() and not os.path.exists(tmp_path / "x.png")


# ---- compression against zlib itself ---------------------------------------------------------------------------------------------------
def _zlib_sizes(orc, img, gamma):
    px = pc.expected_pixels(orc, img, gamma).astype(np.int16)
    sub = px.copy()
    sub[:, 1:] -= px[:, :-1]
    raw = b"".join(b"\x01" + (row & 255).astype(np.uint8).tobytes() for row in sub)
    rle = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return len(rle.compress(raw) + rle.flush()), len(zlib.compress(raw, 6))


def test_compression_of_the_golden_frames_against_zlib(rt, orc):
    """The IDAT payload against zlib.compressobj(6, strategy=Z_RLE) over the same Sub-filtered bytes (and, printed, zlib's default
    strategy).  zlib pays no per-tile sync marker and may merge tables over larger blocks; the golden frames are one tile each, so the
    margin is this encoder's 5-byte final block, its marker and its code-length layout.  Measured with the host formatter (gamma on),
    IDAT bytes here / Z_RLE / default:
        oracle_config2_small_seed2  5730 / 5722 / 5426   +0.14 %
        oracle_all_materials_seed0  5007 / 4998 / 5081   +0.18 %
        oracle_final_thumb_seed7    3365 / 3358 / 3353   +0.21 %
        oracle_earth_thumb_seed3     850 /  842 /  789   +0.95 %
    The largest measured excess over Z_RLE is 0.95 % (8 bytes of 842); the bound asserted is twice that, 1.9 %
    (scripts/png_measure.py --sizes, profiles/r17/png_sizes.json)."""
    for name, img in pc.golden_frames():
        idat = len(pc.decode(host_png(rt, img, True))[1])
        z_rle, z_default = _zlib_sizes(orc, img, True)
        print(f"{name}: idat {idat} Z_RLE {z_rle} default {z_default} excess {idat / z_rle - 1:+.4f}")
        assert idat <= z_rle * (1 + PNG_EXCESS_BOUND), name


PNG_EXCESS_BOUND = 0.019  # twice the largest measured excess, 0.0095 (profiles/r17/png_sizes.json)


# ---- the device calls without a device -------------------------------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


FORMAT_REFUSALS = (  # (d_rgb given, rows, cols, d_out given, capacity) -> status name, message
    ((False, 2, 3, True, 256), "RT_ERR_INVALID_ARGUMENT", "d_rgb is NULL"),
    ((True, 0, 3, True, 256), "RT_ERR_INVALID_ARGUMENT", "rows and cols must be positive"),
    ((True, 2, -3, True, 256), "RT_ERR_INVALID_ARGUMENT", "rows and cols must be positive"),
    ((True, 65536, 65536, True, 256), "RT_ERR_INVALID_ARGUMENT", "an image of more than INT32_MAX pixels"),
    ((True, 2, 3, True, 0), "RT_ERR_INVALID_ARGUMENT", "d_out is given but out_capacity is 0"),
    ((True, 27000, 27000, True, 256), "RT_ERR_UNSUPPORTED", "an image whose PNG data may pass 2^31 - 1 bytes"),
    ((False, 27000, 27000, True, 0), "RT_ERR_INVALID_ARGUMENT", "d_rgb is NULL"),  # two faults: the first one found decides
)


@pytest.mark.parametrize("case, status, text", FORMAT_REFUSALS)
def test_format_png_device_refuses_before_any_device(rt, case, status, text):
    has_rgb, rows, cols, has_out, cap = case
    rgb = np.full(18, 7, np.uint8)
    out = np.full(256, 0x5A, np.uint8)
    d_len = np.full(1, -7, np.int64)
    length = C.c_int64(-7)
    rc = rt.lib.rt_format_png_device(99, _ptr(rgb) if has_rgb else None, rows, cols, 1, _ptr(out) if has_out else None, cap, _ptr(d_len), None,
                                     C.byref(length))
    assert rc == getattr(rt._abi, status) and rt.lib.rt_last_error().decode() == text
    assert length.value == -7 and d_len[0] == -7 and (out == 0x5A).all() and (rgb == 7).all()


def test_write_and_render_refusals(rt, tmp_path):
    A = rt._abi
    rgb = np.full(18, 7, np.uint8)
    err = lambda: rt.lib.rt_last_error().decode()  # noqa: E731
    good, bad = str(tmp_path / "x.png").encode(), str(tmp_path / "missing" / "x.png").encode()
    w = rt.lib.rt_write_png_device
    assert w(None, 99, _ptr(rgb), 2, 3, 1, None) == A.RT_ERR_INVALID_ARGUMENT and err() == "path is NULL"
    assert w(good, 99, None, 2, 3, 1, None) == A.RT_ERR_INVALID_ARGUMENT and err() == "d_rgb is NULL"
    assert w(good, 99, _ptr(rgb), 2, 0, 1, None) == A.RT_ERR_INVALID_ARGUMENT and err() == "rows and cols must be positive"
    assert w(good, 99, _ptr(rgb), 27000, 27000, 1, None) == A.RT_ERR_UNSUPPORTED
    assert not os.path.exists(good)  # refused before the file is opened
    assert w(bad, 99, _ptr(rgb), 2, 3, 1, None) == A.RT_ERR_IO and err() == "cannot open " + bad.decode()
    assert (rgb == 7).all()

    objs, cam, mw, mh = rt.sample_images.config1_empty()
    scene, cam_abi = rt.Scene.make(objs), cam.to_abi()
    st = A.rt_stats()
    C.memset(C.byref(st), 0x55, C.sizeof(st))

    def call(scene_h=scene.handle, camera=cam_abi, w_=3, h_=2, path=good):
        return rt.lib.rt_render_png(scene_h, C.byref(camera) if camera is not None else None, w_, h_, 5, 99, 0, 1, path, None, C.byref(st))

    # rt_render_ppm's check list in its order: scene, camera, geometry, then the path, the pixel count and the PNG's own limit
    assert call(scene_h=None) == A.RT_ERR_INVALID_ARGUMENT and err() == "scene is NULL"
    assert call(camera=None) == A.RT_ERR_INVALID_ARGUMENT and err() == "camera is NULL"
    assert call(w_=0) == A.RT_ERR_INVALID_ARGUMENT and err() == "max_width_coord and max_height_coord must be positive"
    assert call(h_=(1 << 20) + 1) == A.RT_ERR_INVALID_ARGUMENT and err() == "image too large"
    assert call(path=None) == A.RT_ERR_INVALID_ARGUMENT and err() == "path is NULL"
    assert call(w_=1 << 20, h_=1 << 20) == A.RT_ERR_INVALID_ARGUMENT and err() == "an image of more than INT32_MAX pixels"
    assert call(w_=13500, h_=13500) == A.RT_ERR_UNSUPPORTED
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
    path = str(tmp_path / "x.png").encode()
    assert rt.lib.rt_format_png_device(0, _ptr(rgb), 2, 3, 1, _ptr(out), 256, None, None, C.byref(length)) == A.RT_ERR_NO_DEVICE
    assert rt.lib.rt_format_png_device(0, _ptr(rgb), 2, 3, 1, None, 0, None, None, C.byref(length)) == A.RT_ERR_NO_DEVICE  # length only
    assert rt.lib.rt_write_png_device(path, 0, _ptr(rgb), 2, 3, 1, None) == A.RT_ERR_NO_DEVICE
    assert "no CPU fallback" in rt.lib.rt_last_error().decode()
    objs, cam, mw, mh = rt.sample_images.config1_empty()
    with pytest.raises(rt.RtError) as e:
        rt.Scene.make(objs).renderPng(3, 2, cam, str(tmp_path / "y.png"))
    assert e.value.code == A.RT_ERR_NO_DEVICE
    assert length.value == -7 and (out == 0x5A).all()


# ---- Python ----------------------------------------------------------------------------------------------------------------------------
def test_python_png_of_numpy_images(rt, orc, tmp_path):
    for img in (pc.GOLDEN_IMAGE, pc.noise(13, 11, 4), pc.golden_frames()[2][1]):
        for gamma in (False, True):
            data = rt.Png.format(gamma, img)
            assert data == host_png(rt, img, gamma)
            path = str(tmp_path / "host.png")
            ticks = []
            rt.Png.write(gamma, ticks.append, img, path)
            assert open(path, "rb").read() == data
            assert len(ticks) == img.shape[0] * img.shape[1] - 1 and set(ticks) <= {1.0}  # ImageOutput.fs:230-241
    with pytest.raises(rt.RtError):
        rt.Png.format(False, np.zeros((0, 3, 3), np.uint8))


# ---- the header alone, and the C consumer ----------------------------------------------------------------------------------------------
def test_png_header_alone_under_the_sanitizers(tmp_path):
    """tests/c/png_host_table.cpp over csrc/rt_png.h: the combiners against straight-line CRC-32 and Adler-32 over split buffers, the code
    builder's Kraft sums and length limits, the token rule -- a stand-alone program, built with -fsanitize=address,undefined."""
    exe = str(tmp_path / "png_host_table")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "c", "png_host_table.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split() == ["checksums", "ok", "code_builder", "ok", "token_rule", "ok", "sizes", "ok"]


def build_png_smoke(tmp_path):
    exe = str(tmp_path / "png_smoke")
    libdir = os.path.join(ROOT, "ray-tracing-fsharp_amd")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "png_smoke.c"),
                           "-L", libdir, "-lrtfs_amd", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    return exe


def test_c_program_formats_on_the_host_and_checks_the_refusals(rt, orc, tmp_path):
    out = subprocess.run([build_png_smoke(tmp_path), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "png: refusals ok" in out.stdout
    lines = dict(line.split(" ", 1) for line in out.stdout.splitlines() if line.split(" ", 1)[0] in ("host", "device"))
    data = bytes.fromhex(lines["host"])
    assert data == host_png(rt, pc.GOLDEN_IMAGE) == (tmp_path / "c_write.png").read_bytes()
    check_file(rt, orc, data, pc.GOLDEN_IMAGE, False)
