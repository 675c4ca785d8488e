"""PNG files of a batch of views as far as they go without a GPU: the batch layout of csrc/rt_png.h driven alone by
tests/c/png_views_table.cpp and held against a straightforward loop (with three wrong layouts that the table must catch),
rt_png_views_max_bytes, every refusal of rt_format_png_views_device, rt_write_png_views_device and rt_render_views_png before any device
call, and the Python routes for numpy batches.  The expected bytes are always rt_format_png per image (test_png_host.host_png)."""
import ctypes as C
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import png_cases as pc
from test_png_host import T0, host_png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("rt_png_views_max_bytes", "rt_format_png_views_device", "rt_write_png_views_device", "rt_render_views_png")
HEAD, TAIL, IDAT_EXTRA = 43, 25, 11  # rt_png.h's HEAD_BYTES, TAIL_BYTES, IDAT_EXTRA: the container of test_png_host.py's files
KS = (1, 2, 3, 1025)
SIZES = ((1, 1), (5, 3), (16, 341), (17, 341))  # rows x cols: 4, 80, 16384 (exactly one tile) and 17408 (a full tile and 1024 more) filtered bytes


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_the_four_symbols_are_declared_exported_and_bound(rt):
    from ray_tracing_fsharp_amd import _lib

    header = open(os.path.join(ROOT, "include", "rtfs_amd.h")).read()
    declared = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/rtfs_amd.h"
        assert hasattr(_lib.lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert "#define RT_ABI_VERSION 7" in header and rt.lib.rt_abi_version() == 7  # symbols only


# ---- the layout ------------------------------------------------------------------------------------------------------------------------
def _build_table(tmp, mutant=0, sanitize=False):
    exe = str(tmp / f"png_views_table_{mutant}{'_san' if sanitize else ''}")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", f"-DRTP_VIEWS_MUTANT={mutant}", *flags, "-o", exe,
                           os.path.join(HERE, "c", "png_views_table.cpp")])
    return exe


def _batches():
    """(K, rows, cols, bytes[K][tiles]) for every K and size, the tile byte counts random between a Huffman tile's few bytes and a stored tile's."""
    rng = np.random.default_rng(35)
    out = []
    for k in KS:
        for rows, cols in SIZES:
            tiles = -(-rows * (1 + 3 * cols) // T0)
            out.append((k, rows, cols, rng.integers(6, T0 + 6, (k, tiles)).tolist()))
    return out


def _run_table(exe, batches):
    lines = [" ".join(str(x) for x in (k, rows, cols, *[b for image in counts for b in image])) for k, rows, cols, counts in batches]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = []
    for line in out.stdout.splitlines():
        d = dict(kv.split("=") for kv in line.split())
        got.append({k: ([int(x) for x in v.split(",")] if k in ("entry", "start", "end", "idat", "tile", "go") else int(v)) for k, v in d.items()})
    assert len(got) == len(batches)
    return got


def _expected(k, rows, cols, counts):
    """The same batch by a loop over the files: each is its head, its tiles and its tail, and the next begins where it ends."""
    tiles = -(-rows * (1 + 3 * cols) // T0)
    at, entry, start, end, idat, tile = 0, [], [], [], [], []
    for v in range(k):
        start.append(at)
        at += HEAD
        for t in range(tiles):
            entry.append(v * (tiles + 1) + t)  # an image's tiles, then one entry for what lies between it and the next
            tile.append(at)
            at += counts[v][t]
        idat.append(sum(counts[v]) + IDAT_EXTRA)
        at += TAIL
        end.append(at)
    return dict(tiles=tiles, entries=k * (tiles + 1), total=at, entry=entry, start=start + [at], end=end, idat=idat, tile=tile, go=[0, 1, 1, 0])


def _mismatches(got, batches):
    bad = []
    for g, (k, rows, cols, counts) in zip(got, batches):
        want = _expected(k, rows, cols, counts)
        bad += [(k, rows, cols, key) for key in want if g[key] != want[key]]
        if g["start"][-1] != sum(e - s for s, e in zip(g["start"][:-1], g["end"])):  # offsets[K] is the sum of the files' lengths
            bad.append((k, rows, cols, "sum of lengths"))
    return bad


def test_the_layout_table_against_a_straightforward_loop(tmp_path):
    batches = _batches()
    assert [-(-r * (1 + 3 * c) // T0) for r, c in SIZES] == [1, 1, 1, 2] and 2 * 1025 > 1024
    got = _run_table(_build_table(tmp_path, sanitize=True), batches)  # a stand-alone program: the sanitizers see all of it
    assert _mismatches(got, batches) == []
    for g in got:  # the capacity decision at total - 1, total, total + 1, and with no buffer
        assert g["go"] == [0, 1, 1, 0]


@pytest.mark.parametrize("mutant, what", [(1, "start"), (2, "entry"), (3, "idat")])
def test_each_wrong_layout_is_caught_by_the_table(tmp_path, mutant, what):
    """1: the head charged to the wrong entry; 2: image v's entries begun one early; 3: the IDAT length taken from the batch's total.
    CPU builds of the test's own -- nothing like them runs on a GPU."""
    batches = _batches()
    bad = _mismatches(_run_table(_build_table(tmp_path, mutant), batches), batches)
    assert any(key == what for _, _, _, key in bad), bad
    assert all(k > 1 for k, _, _, _ in bad)  # a batch of one image is the single image's layout under every mutant


# ---- sizes -----------------------------------------------------------------------------------------------------------------------------
def test_views_max_bytes_is_k_times_one_images(rt):
    A = rt._abi
    f = rt.lib.rt_png_views_max_bytes
    err = lambda: rt.lib.rt_last_error().decode()  # noqa: E731
    for k in (0,) + KS + (64,):
        for rows, cols in SIZES + ((41, 71),):
            assert f(k, rows, cols) == k * rt.lib.rt_png_max_bytes(rows, cols)
    assert f(2, 1601, 2401) == 2 * rt.lib.rt_png_max_bytes(1601, 2401)
    assert f(64, 41, 71) == 64 * (68 + 41 * 214 + 5)
    assert f(-1, 2, 3) == -A.RT_ERR_INVALID_ARGUMENT and err() == "n_views must be >= 0"
    for rows, cols, text in ((0, 3, "rows and cols must be positive"), (3, -1, "rows and cols must be positive"),
                             (65536, 65536, "an image of more than INT32_MAX pixels")):
        assert f(2, rows, cols) == -A.RT_ERR_INVALID_ARGUMENT and err() == text
    assert f(2, 27000, 27000) == -A.RT_ERR_UNSUPPORTED and err() == "an image whose PNG data may pass 2^31 - 1 bytes"
    # the batch's own bound: n_views * rows * cols <= INT32_MAX
    assert f(3, 20001, 40001) == -A.RT_ERR_INVALID_ARGUMENT and err() == "a batch of views holds at most INT32_MAX pixels"
    assert f(2**31 - 1, 1, 1) == (2**31 - 1) * (68 + 4 + 5) and f(2**30, 1, 3) == -A.RT_ERR_INVALID_ARGUMENT
    assert f(3, 23000, 31000) == 3 * rt.lib.rt_png_max_bytes(23000, 31000) > 2**32  # (2,139,000,000 pixels: just inside the bound)


# ---- the device calls without a device ---------------------------------------------------------------------------------------------------
FORMAT_REFUSALS = (  # (d_rgb given, n_views, rows, cols, d_out given, capacity) -> status name, message
    ((True, -1, 2, 3, True, 256), "RT_ERR_INVALID_ARGUMENT", "n_views must be >= 0"),
    ((False, 2, 2, 3, True, 256), "RT_ERR_INVALID_ARGUMENT", "d_rgb is NULL"),
    ((True, 2, 0, 3, True, 256), "RT_ERR_INVALID_ARGUMENT", "rows and cols must be positive"),
    ((True, 2, 2, -3, True, 256), "RT_ERR_INVALID_ARGUMENT", "rows and cols must be positive"),
    ((True, 0, 0, 3, False, 0), "RT_ERR_INVALID_ARGUMENT", "rows and cols must be positive"),
    ((True, 1, 65536, 65536, True, 256), "RT_ERR_INVALID_ARGUMENT", "an image of more than INT32_MAX pixels"),
    ((True, 3, 20001, 40001, True, 256), "RT_ERR_INVALID_ARGUMENT", "a batch of views holds at most INT32_MAX pixels"),
    ((True, 2, 2, 3, True, 0), "RT_ERR_INVALID_ARGUMENT", "d_out is given but out_capacity is 0"),
    ((True, 1, 27000, 27000, True, 256), "RT_ERR_UNSUPPORTED", "an image whose PNG data may pass 2^31 - 1 bytes"),
    ((False, 2, 27000, 27000, True, 0), "RT_ERR_INVALID_ARGUMENT", "d_rgb is NULL"),  # several faults: the first one found decides
)


@pytest.mark.parametrize("case, status, text", FORMAT_REFUSALS)
def test_format_png_views_device_refuses_before_any_device(rt, case, status, text):
    has_rgb, k, rows, cols, has_out, cap = case
    rgb = np.full(36, 7, np.uint8)
    out = np.full(256, 0x5A, np.uint8)
    d_off = np.full(4, -7, np.int64)
    offsets = (C.c_int64 * 4)(-7, -7, -7, -7)
    rc = rt.lib.rt_format_png_views_device(99, _ptr(rgb) if has_rgb else None, k, rows, cols, 1, _ptr(out) if has_out else None, cap, _ptr(d_off), None, offsets)
    assert rc == getattr(rt._abi, status) and rt.lib.rt_last_error().decode() == text
    assert list(offsets) == [-7] * 4 and (d_off == -7).all() and (out == 0x5A).all() and (rgb == 7).all()


def test_no_views_is_ok_without_a_device(rt, tmp_path):
    A = rt._abi
    offsets = (C.c_int64 * 2)(-7, -7)
    out = np.full(16, 0x5A, np.uint8)
    assert rt.lib.rt_format_png_views_device(99, None, 0, 2, 3, 1, _ptr(out), 16, None, None, offsets) == A.RT_OK
    assert list(offsets) == [0, -7] and (out == 0x5A).all()
    assert rt.lib.rt_format_png_views_device(99, None, 0, 2, 3, 1, None, 0, None, None, None) == A.RT_OK
    paths = (C.c_char_p * 1)(str(tmp_path / "x.png").encode())
    assert rt.lib.rt_write_png_views_device(paths, 99, None, 0, 2, 3, 1, None) == A.RT_OK
    assert not os.path.exists(tmp_path / "x.png")


def _scene(rt):
    P, S, H, Tex, Px = rt.Point.make, rt.SphereStyle, rt.Hittable, rt.Texture.Colour, rt.Pixel
    return rt.Scene.make([H.Sphere(rt.Sphere.make(S.LambertReflection(0.8, Tex(Px(200, 100, 50))), P(0.0, 0.0, 3.0), 1.0))])


def _camera(rt, spp=20, depth=3):
    cam = rt.Camera.makeBasic(spp, 1.0, 9.0 / 7.0, rt.Point.make(0.0, 0.0, -1.0), rt.Vector.unitise(rt.Vector.make(0.0, 0.0, 1.0)), rt.Vector.make(0.0, 1.0, 0.0))
    return dataclasses.replace(cam, BounceDepth=depth)


def test_write_and_render_refusals(rt, tmp_path):
    A = rt._abi
    INV = A.RT_ERR_INVALID_ARGUMENT
    err = lambda: rt.lib.rt_last_error().decode()  # noqa: E731
    rgb = np.full(36, 7, np.uint8)
    names = [str(tmp_path / f"v{v}.png").encode() for v in range(3)]
    good, hole = (C.c_char_p * 3)(*names), (C.c_char_p * 3)(names[0], None, names[2])
    w = rt.lib.rt_write_png_views_device
    assert w(good, 99, _ptr(rgb), -1, 2, 3, 1, None) == INV and err() == "n_views must be >= 0"
    assert w(good, 99, None, 2, 2, 3, 1, None) == INV and err() == "d_rgb is NULL"
    assert w(good, 99, _ptr(rgb), 2, 2, 0, 1, None) == INV and err() == "rows and cols must be positive"
    assert w(good, 99, _ptr(rgb), 3, 20001, 40001, 1, None) == INV and err() == "a batch of views holds at most INT32_MAX pixels"
    assert w(good, 99, _ptr(rgb), 1, 27000, 27000, 1, None) == A.RT_ERR_UNSUPPORTED
    assert w(None, 99, _ptr(rgb), 2, 2, 3, 1, None) == INV and err() == "paths is NULL"
    assert w(hole, 99, _ptr(rgb), 2, 2, 3, 1, None) == INV and err() == "paths[1] is NULL"
    assert (rgb == 7).all() and not any(os.path.exists(n) for n in names)

    scene = _scene(rt)
    st = A.rt_stats()
    C.memset(C.byref(st), 0x55, C.sizeof(st))
    cams = (A.rt_camera * 3)(*[_camera(rt).to_abi() for _ in range(3)])
    other = (A.rt_camera * 3)(_camera(rt).to_abi(), _camera(rt, spp=21).to_abi(), _camera(rt).to_abi())

    def call(scene_h=scene.handle, cameras=cams, k=3, w_=4, h_=3, paths=good, options=None):
        return rt.lib.rt_render_views_png(scene_h, cameras, k, w_, h_, None, 5, 99, 0, 1, paths, C.byref(options) if options is not None else None, C.byref(st))

    # rt_render_views' check list in its order, then the paths and the PNG's own limit
    assert call(scene_h=None) == INV and err() == "scene is NULL"
    assert call(k=-1) == INV and err() == "n_views must be >= 0"
    assert call(cameras=None) == INV and err() == "cameras is NULL"
    assert call(w_=0) == INV and err() == "max_width_coord and max_height_coord must be positive"
    assert call(h_=(1 << 20) + 1) == INV and err() == "image too large"
    assert call(cameras=other) == INV and err() == "the cameras of a batch must share samples_per_pixel and bounce_depth"
    assert call(w_=20000, h_=10000) == INV and err() == "a batch of views holds at most INT32_MAX pixels"
    assert call(options=A.rt_render_options(passes=3)) == INV and err() == "passes must be 0 (auto), 1 (fused) or 2 (two-pass)"
    assert call(paths=None) == INV and err() == "paths is NULL"
    assert call(paths=hole) == INV and err() == "paths[1] is NULL"
    assert call(k=1, w_=13500, h_=13500) == A.RT_ERR_UNSUPPORTED and err() == "an image whose PNG data may pass 2^31 - 1 bytes"
    assert bytes(st)[:8] == b"\x55" * 8 and not any(os.path.exists(n) for n in names)
    # no view: RT_OK with zeroed stats, and still no file
    assert call(cameras=None, k=0) == A.RT_OK and st.pixels == 0 and st.samples == 0 and not any(os.path.exists(n) for n in names)


def test_a_scene_with_a_texture_program_is_unsupported(rt, tmp_path):
    from ray_tracing_fsharp_amd import texprog as T
    A = rt._abi
    tp = rt.Texture.Program(T.PX * 10.0, T.PY, T.PZ)
    scene = rt.Scene.make([rt.Hittable.Sphere(rt.Sphere.make(rt.SphereStyle.LightSource(tp), rt.Point.make(8.0, 0.0, 0.0), 1.0))])
    paths = [str(tmp_path / f"v{v}.png") for v in range(2)]
    with pytest.raises(rt.RtError) as e:
        scene.renderViewsPng(4, 3, [_camera(rt)] * 2, paths)
    assert e.value.code == A.RT_ERR_UNSUPPORTED and "a batch of views does not take a scene that holds a texture program" in str(e.value)
    assert not any(os.path.exists(p) for p in paths)


def test_without_a_device_valid_calls_say_so(rt, tmp_path):
    """After the argument checks: RT_ERR_NO_DEVICE, never a fallback to the host formatter."""
    if rt.device_count() > 0:
        pytest.skip("a GPU is visible")
    A = rt._abi
    rgb = np.full(36, 7, np.uint8)
    out = np.full(256, 0x5A, np.uint8)
    offsets = (C.c_int64 * 3)(-7, -7, -7)
    names = [str(tmp_path / f"v{v}.png") for v in range(2)]
    paths = (C.c_char_p * 2)(*[n.encode() for n in names])
    assert rt.lib.rt_format_png_views_device(0, _ptr(rgb), 2, 2, 3, 1, _ptr(out), 256, None, None, offsets) == A.RT_ERR_NO_DEVICE
    assert rt.lib.rt_format_png_views_device(0, _ptr(rgb), 2, 2, 3, 1, None, 0, None, None, offsets) == A.RT_ERR_NO_DEVICE  # offsets only
    assert rt.lib.rt_write_png_views_device(paths, 0, _ptr(rgb), 2, 2, 3, 1, None) == A.RT_ERR_NO_DEVICE
    assert "no CPU fallback" in rt.lib.rt_last_error().decode()
    with pytest.raises(rt.RtError) as e:
        _scene(rt).renderViewsPng(4, 3, [_camera(rt)] * 2, names)
    assert e.value.code == A.RT_ERR_NO_DEVICE
    assert list(offsets) == [-7] * 3 and (out == 0x5A).all() and not any(os.path.exists(n) for n in names)


# ---- Python ----------------------------------------------------------------------------------------------------------------------------
def test_python_views_of_numpy_batches(rt, orc, tmp_path):
    batch = np.stack([pc.noise(5, 3, 1), np.full((5, 3, 3), 90, np.uint8), pc.noise(5, 3, 2)])
    for gamma in (False, True):
        files = rt.Png.formatViews(gamma, batch)
        assert files == [rt.Png.format(gamma, image) for image in batch] == [host_png(rt, image, gamma) for image in batch]
        for data, image in zip(files, batch):
            assert np.array_equal(pc.decode(data)[0], pc.expected_pixels(orc, image, gamma))
        paths = [tmp_path / f"g{int(gamma)}_{v}.png" for v in range(3)]
        rt.Png.writeViews(gamma, batch, paths)
        assert [p.read_bytes() for p in paths] == files
    assert rt.Png.formatViews(True, np.zeros((0, 5, 3, 3), np.uint8)) == []
    with pytest.raises(ValueError, match=r"\[K, rows, cols, 3\]"):
        rt.Png.formatViews(False, batch[0])
    with pytest.raises(ValueError, match="one path per view"):
        rt.Png.writeViews(False, batch, [tmp_path / "only.png"])
    with pytest.raises(ValueError, match="one path per view"):
        _scene(rt).renderViewsPng(4, 3, [_camera(rt)] * 2, [tmp_path / "only.png"])
