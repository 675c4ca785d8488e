"""Render jobs without a GPU (include/rtfs_amd.h "Render jobs"): the calls declared and bound, every refusal of rt_render_job_start
reported before any device call with nothing written, RT_RENDER_COUNTERS unsupported, and the partial spill's host formatter
rt_format_pixel_map_present against a literal restatement of ImageOutput.fs:145-155 restricted to the present pixels, against
rt_format_pixel_map when all are present, and through rt_parse_pixel_map back to the mask and the present pixels' bytes."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOB_CALLS = ("rt_render_job_start", "rt_render_job_progress", "rt_render_job_stop", "rt_render_job_wait", "rt_render_job_finish",
             "rt_dev_set_job_limits", "rt_dev_last_job_plan", "rt_format_pixel_map_present_device")
W, H = 3, 2
COLS, ROWS = 2 * W + 1, 2 * H + 1


def _scene(rt):
    P, S, Hit, Tex, Px = rt.Point.make, rt.SphereStyle, rt.Hittable, rt.Texture.Colour, rt.Pixel
    return rt.Scene.make([Hit.Sphere(rt.Sphere.make(S.LambertReflection(0.8, Tex(Px(200, 100, 50))), P(0.0, 0.0, 3.0), 1.0))])


def _camera(rt, spp=40):
    cam = rt.Camera.makeBasic(spp, 1.0, 1.5, rt.Point.make(0.0, 0.0, -1.0), rt.Vector.unitise(rt.Vector.make(0.0, 0.0, 1.0)), rt.Vector.make(0.0, 1.0, 0.0))
    return dataclasses.replace(cam, BounceDepth=5)


def test_prototypes_and_version(rt):
    from ray_tracing_fsharp_amd import _lib
    header = open(os.path.join(ROOT, "include", "rtfs_amd.h")).read()
    assert "#define RT_ABI_VERSION 7" in header  # added symbols and structs only
    for name in JOB_CALLS:
        assert f"int {name}(" in header and hasattr(_lib.lib, name) and name in _lib.SIGNATURES, name
    assert "void rt_render_job_destroy(" in header and "int64_t rt_format_pixel_map_present(" in header
    assert "typedef struct rt_render_job rt_render_job;" in header
    assert rt.lib.rt_abi_version() == 7 == rt._abi.RT_ABI_VERSION
    # every call cites the reference's watched render and its eager spill
    for name in JOB_CALLS + ("rt_render_job_destroy", "rt_format_pixel_map_present"):
        doc = header[:header.index(f" {name}(")].rsplit("/*", 1)[1]
        assert "Scene.fs:196-236" in doc and "ImageOutput.fs:131-161" in doc, name
    assert C.sizeof(rt._abi.rt_job_progress) == 24 and C.sizeof(rt._abi.rt_job_result) == 32


def _start(rt, scene, cam, accum, rgb, present, out, *, w=W, h=H, row_first=0, row_stride=1, n_rows=ROWS, flags=0, options=None, device=0):
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    return rt.lib.rt_render_job_start(scene, C.byref(cam) if cam is not None else None, w, h, 1, device, row_first, row_stride, n_rows, flags, p(accum), p(rgb),
                                      p(present), None, C.byref(options) if options is not None else None, C.byref(out) if out is not None else None)


def test_every_refusal_of_start_comes_before_the_device_and_writes_nothing(rt):
    A = rt._abi
    scene = _scene(rt)
    S = scene.handle
    cam = _camera(rt).to_abi()
    accum, rgb, present = np.full((ROWS, COLS, 4), 77, np.int32), np.full((ROWS, COLS, 3), 3, np.uint8), np.full((ROWS, COLS), 9, np.uint8)
    out = C.c_void_p(0x5A5A)
    unset = A.rt_render_options(); unset.struct_size = 0
    big = 1 << 15  # (2 * big + 1)^2 > INT32_MAX pixels: rt_render_job_finish lists pixels as int32
    refused = [
        dict(scene=None), dict(cam=None), dict(w=0), dict(h=-1), dict(w=(1 << 20) + 1),
        dict(cam=_camera(rt, 0).to_abi()), dict(cam=_camera(rt, 8000001).to_abi()), dict(cam=dataclasses.replace(_camera(rt), BounceDepth=-1).to_abi()),
        dict(row_stride=0), dict(row_first=-1), dict(n_rows=-1), dict(n_rows=ROWS + 1), dict(row_first=1, row_stride=2, n_rows=3),
        dict(accum=None), dict(present=None), dict(out=None),
        dict(options=A.rt_render_options(block_threads=100)), dict(options=unset), dict(options=A.rt_render_options(passes=3)),
        dict(options=A.rt_render_options(chunk_pixels=65)),
        dict(w=big, h=big, n_rows=1),
        # ... and in front of a device index nobody has
        dict(accum=None, device=99), dict(present=None, device=-1),
    ]
    for i, kw in enumerate(refused):
        args = dict(scene=S, cam=cam, accum=accum, rgb=rgb, present=present, out=out)
        args.update(kw)
        rc = _start(rt, args.pop("scene"), args.pop("cam"), args.pop("accum"), args.pop("rgb"), args.pop("present"), args.pop("out"), **args)
        assert rc == A.RT_ERR_INVALID_ARGUMENT, (i, kw, rc, rt.lib.rt_last_error())
        assert rt.lib.rt_last_error()
        assert out.value == 0x5A5A and (accum == 77).all() and (rgb == 3).all() and (present == 9).all()
    # there is no counting variant
    assert _start(rt, S, cam, accum, rgb, present, out, flags=A.RT_RENDER_COUNTERS) == A.RT_ERR_UNSUPPORTED
    assert b"counting" in rt.lib.rt_last_error() and out.value == 0x5A5A
    # ... but a bad argument is still what is reported first
    assert _start(rt, S, cam, None, rgb, present, out, flags=A.RT_RENDER_COUNTERS) == A.RT_ERR_INVALID_ARGUMENT
    # the other calls refuse a NULL job and structs whose size is not set
    L = rt.lib
    pr, res = A.rt_job_progress(), A.rt_job_result()
    assert L.rt_render_job_progress(None, C.byref(pr)) == A.RT_ERR_INVALID_ARGUMENT
    assert L.rt_render_job_stop(None) == A.RT_ERR_INVALID_ARGUMENT
    assert L.rt_render_job_wait(None, C.byref(res), None) == A.RT_ERR_INVALID_ARGUMENT
    assert L.rt_render_job_finish(None, None, None) == A.RT_ERR_INVALID_ARGUMENT
    L.rt_render_job_destroy(None)
    assert L.rt_dev_set_job_limits(-2, 0) == A.RT_ERR_INVALID_ARGUMENT and L.rt_dev_set_job_limits(0, -2) == A.RT_ERR_INVALID_ARGUMENT
    assert L.rt_dev_set_job_limits(-1, -1) == A.RT_OK
    assert L.rt_dev_last_job_plan(None) == A.RT_ERR_INVALID_ARGUMENT
    if rt.device_count() == 0:  # a good call gets as far as the device, and no further
        assert _start(rt, S, cam, accum, rgb, present, out) == A.RT_ERR_NO_DEVICE
        assert out.value == 0x5A5A and (accum == 77).all() and (rgb == 3).all() and (present == 9).all()


def test_the_device_formatter_refuses_before_the_device(rt):
    A = rt._abi
    rgb, present, outb = np.zeros((2, 3, 3), np.uint8), np.ones((2, 3), np.uint8), np.full(64, 5, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    f = rt.lib.rt_format_pixel_map_present_device
    n = C.c_int64(-7)
    for args in ((None, p(present), 2, 3, p(outb), 64), (p(rgb), None, 2, 3, p(outb), 64), (p(rgb), p(present), 0, 3, p(outb), 64),
                 (p(rgb), p(present), 2, -1, p(outb), 64), (p(rgb), p(present), 1 << 16, 1 << 16, p(outb), 64), (p(rgb), p(present), 2, 3, p(outb), 0)):
        assert f(0, *args, None, None, C.byref(n)) == A.RT_ERR_INVALID_ARGUMENT, args
        assert n.value == -7 and (outb == 5).all()
    if rt.device_count() == 0:
        assert f(0, p(rgb), p(present), 2, 3, p(outb), 64, None, None, C.byref(n)) == A.RT_ERR_NO_DEVICE


def test_c_program_checks_the_job_arguments(rt, tmp_path):
    """tests/c/render_job_smoke.c from C99: the argument checks and the host formatter hold without a GPU (with one, test_gpu_render_job
    runs its job)."""
    import subprocess
    exe = str(tmp_path / "render_job_smoke")
    libdir = os.path.join(ROOT, "ray-tracing-fsharp_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "render_job_smoke.c"),
                           "-L", libdir, "-lrtfs_amd", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "render job: argument checks ok" in out.stdout


# ---- rt_format_pixel_map_present ------------------------------------------------------------------------------------------------------
def _write_ascii_int(out: bytearray, i: int) -> None:  # ImageOutput.fs:115-129, line for line
    places, tmp, pow_ = 0, i, 1
    while tmp > 0:
        tmp //= 10
        pow_ *= 10
        places += 1
    pow_ //= 10
    while pow_ > 0:
        out.append(((i // pow_) % 10) + 48)
        pow_ //= 10


def _resume_literal(pixels, present) -> bytes:  # ImageOutput.fs:145-155 over the pixels that are there
    out = bytearray()
    for row_num, row in enumerate(pixels):
        for col_num, pixel in enumerate(row):
            if not present[row_num][col_num]:
                continue
            _write_ascii_int(out, row_num)
            out.append(44)
            _write_ascii_int(out, col_num)
            out.append(10)
            out.append(int(pixel[0])); out.append(int(pixel[1])); out.append(int(pixel[2]))
    return bytes(out)


def _masks(rows, cols):
    n = rows * cols
    one = np.zeros(n, bool); one[n // 2] = True
    checker = (np.add.outer(np.arange(rows), np.arange(cols)) % 2 == 0)
    prefix = np.arange(n) < (n * 2) // 3
    return {"none": np.zeros((rows, cols), bool), "all": np.ones((rows, cols), bool), "one": one.reshape(rows, cols), "checkerboard": checker,
            "prefix": prefix.reshape(rows, cols)}


@pytest.mark.parametrize("shape", [(1, 1), (1, 11), (13, 7)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_partial_spill_is_the_references_records_of_the_present_pixels(rt, shape):
    rows, cols = shape
    rng = np.random.default_rng(rows * 100 + cols)
    rgb = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    rgb[0, 0] = (10, 44, 48)  # colour bytes that look like a terminator, a separator and a digit
    whole = rt.ImageOutput.formatPixelMap(rgb)
    for name, mask in _masks(rows, cols).items():
        got = rt.ImageOutput.formatPixelMapPresent(rgb, mask)
        assert got == _resume_literal(rgb, mask), name
        if mask.all():
            assert got == whole
        # a capacity one byte short writes nothing and still answers the length
        if got:
            buf = np.full(len(got), 0xEE, np.uint8)
            u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))  # noqa: E731
            pr = np.ascontiguousarray(mask, np.uint8)
            assert rt.lib.rt_format_pixel_map_present(u8(rgb), u8(pr), rows, cols, buf.ctypes.data_as(C.c_char_p), len(got) - 1) == len(got)
            assert (buf == 0xEE).all()
        # and the reader gives the mask and the present pixels' bytes back
        back, present = np.full((rows, cols, 3), 0xAB, np.uint8), np.full((rows, cols), 7, np.uint8)
        u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))  # noqa: E731
        assert rt.lib.rt_parse_pixel_map(got, len(got), rows, cols, u8(back), u8(present)) == int(mask.sum()), name
        assert np.array_equal(present.astype(bool), mask), name
        assert np.array_equal(back[mask], rgb[mask]) and (back[~mask] == 0xAB).all(), name
    assert rt.lib.rt_format_pixel_map_present(None, None, rows, cols, None, 0) == -rt._abi.RT_ERR_INVALID_ARGUMENT
