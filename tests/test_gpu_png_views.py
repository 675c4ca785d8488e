"""PNG files of a batch of views on the device -- rt_format_png_views_device, rt_write_png_views_device, rt_render_views_png and their Python
and C callers.  File v must equal the host formatter's bytes for image v (rt_format_png, test_png_host.host_png) byte for byte, and every
file is decoded by the tests' own decoder (png_cases.decode) to oracle.gamma_correct of its image.  Every output buffer is allocated 64
bytes larger than the capacity the call is given, behind `out_offset` more, and filled with a sentinel; nothing in front of the buffer and
nothing at or beyond the total may be written."""
import ctypes as C
import dataclasses
import functools
import os
import subprocess

import numpy as np
import pytest

import png_cases as pc
import scenes
from test_png_host import ROOT, T0, host_png

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
SLACK = 64


def _torch():
    return pytest.importorskip("torch")


def _format(rt, batch, gamma=False, *, capacity=None, in_offset=0, out_offset=0, want_offsets=True, stream=None, no_out=False):
    """One rt_format_png_views_device call on raw pointers: (rc, host offsets or None, d_offsets, the whole output allocation, out_offset)."""
    torch = _torch()
    batch = np.ascontiguousarray(batch, np.uint8)
    k, rows, cols = batch.shape[:3]
    capacity = int(rt.lib.rt_png_views_max_bytes(k, rows, cols)) if capacity is None else capacity
    src = torch.empty(batch.size + in_offset, dtype=torch.uint8, device="cuda")
    src[in_offset:] = torch.from_numpy(batch.reshape(-1)).cuda()
    out = torch.full((out_offset + capacity + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_off = torch.full((k + 1,), -7, dtype=torch.int64, device="cuda")
    offsets = (C.c_int64 * (k + 1))(*([-7] * (k + 1)))
    st = (stream or torch.cuda.current_stream()).cuda_stream
    rc = rt.lib.rt_format_png_views_device(0, src.data_ptr() + in_offset, k, rows, cols, int(gamma), None if no_out else out.data_ptr() + out_offset,
                                           0 if no_out else capacity, d_off.data_ptr(), st, offsets if want_offsets else None)
    torch.cuda.synchronize()
    return rc, (list(offsets) if want_offsets else None), d_off.cpu().tolist(), out.cpu().numpy(), out_offset


def _want(rt, batch, gamma):
    files = [host_png(rt, image, gamma) for image in batch]
    return files, [0] + np.cumsum([len(f) for f in files]).tolist()


def _assert_exact(result, files, at):
    rc, offsets, d_offsets, buf, off = result
    assert rc == 0
    assert d_offsets == at and (offsets is None or offsets == at)
    assert (buf[:off] == SENTINEL).all(), "bytes in front of the buffer were written"
    for v, want in enumerate(files):
        got = buf[off + at[v]:off + at[v + 1]].tobytes()
        if got != want:
            first = next(i for i in range(len(want)) if got[i] != want[i])
            raise AssertionError(f"file {v}: byte {first} of {len(want)} differs: got {got[max(0, first - 12):first + 12].hex()}, want {want[max(0, first - 12):first + 12].hex()}")
    assert (buf[off + at[-1]:] == SENTINEL).all(), "bytes at or beyond the total were written"


def _decodes(orc, files, batch, gamma):
    for data, image in zip(files, batch):
        assert np.array_equal(pc.decode(data)[0], pc.expected_pixels(orc, image, gamma))


# ---- 1: K = 1 is the existing call -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows, cols", [(5, 3), (17, 341)])
def test_one_image_is_the_existing_call(rt, orc, rows, cols):
    img = pc.noise(rows, cols, 11)
    want = host_png(rt, img, True)
    assert -(-rows * (1 + 3 * cols) // T0) == (2 if rows == 17 else 1)
    result = _format(rt, img[None], True)
    _assert_exact(result, [want], [0, len(want)])
    assert result[1] == [0, len(want)]
    _decodes(orc, [want], [img], True)


# ---- 2: images that differ in tile size and block type --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _three_images():
    """17 x 341 (stride 1024: a full tile of 16,384 filtered bytes and a second of 1,024): noise (stored blocks), one constant colour (one long
    run: a compressed block of a few bytes), and one whose top 16 rows are constant and whose last row is noise."""
    mixed = np.full((17, 341, 3), 200, np.uint8)
    mixed[16] = pc.noise(1, 341, 22)[0]
    batch = np.stack([pc.noise(17, 341, 21), np.full((17, 341, 3), (90, 14, 201), np.uint8), mixed])
    batch.setflags(write=False)
    return batch


@pytest.mark.parametrize("gamma", [False, True])
def test_images_that_differ_in_tile_size_and_block_type(rt, orc, gamma):
    batch = _three_images()
    files, at = _want(rt, batch, gamma)
    assert len(files[0]) == rt.lib.rt_png_max_bytes(17, 341) and len(files[1]) < 68 + 200 and len(files[1]) < len(files[2]) < len(files[0])
    _assert_exact(_format(rt, batch, gamma), files, at)
    _decodes(orc, files, batch, gamma)


# ---- 3: runs and the halo stop at an image's edge -------------------------------------------------------------------------------------------
def _shared_edges():
    """K = 4 at 5 x 3 (45 colour bytes an image: images 1..3 start 1, 2 and 3 mod 4 into the batch).  Image v ends in the bytes image v + 1
    begins with, and the bytes on both sides of every boundary are equal: a run or a Sub halo that crossed would change the tokens."""
    rng = np.random.default_rng(33)
    batch = rng.integers(0, 256, (4, 5, 3, 3), dtype=np.uint8)
    flat = batch.reshape(4, 45)
    for v in range(3):
        edge = rng.integers(1, 256, 1, dtype=np.uint8)[0]
        flat[v, 36:] = edge      # the last row of image v: one value ...
        flat[v + 1, :9] = edge   # ... which the first row of image v + 1 goes on with
    return batch


def test_runs_and_the_halo_stop_at_an_images_edge(rt, orc):
    batch = _shared_edges()
    flat = batch.reshape(-1)
    assert all(flat[45 * v - 9:45 * v + 9].min() == flat[45 * v - 9:45 * v + 9].max() for v in (1, 2, 3))
    for gamma in (False, True):
        files, at = _want(rt, batch, gamma)
        _assert_exact(_format(rt, batch, gamma), files, at)
        _decodes(orc, files, batch, gamma)
        for off in (1, 2, 3):  # d_rgb and d_out 1..3 bytes into their allocations
            _assert_exact(_format(rt, batch, gamma, in_offset=off, out_offset=(off * 3) % 4), files, at)


# ---- 4: more scan entries than the scanning workgroup has threads ----------------------------------------------------------------------------
def test_more_scan_entries_than_the_scanning_workgroup_has_threads(rt, orc):
    k = 1025
    v = np.arange(k)
    batch = np.stack([v % 256, v // 256 * 50 + 3, (v * 7) % 256], axis=1).astype(np.uint8).reshape(k, 1, 1, 3)
    assert len({tuple(p) for p in batch.reshape(k, 3)}) == k > 1024
    files, at = _want(rt, batch, True)
    _assert_exact(_format(rt, batch, True), files, at)
    _decodes(orc, files[::97] + files[-1:], np.concatenate([batch[::97], batch[-1:]]), True)  # (every file is compared above; a sample is decoded)


# ---- 5: the capacity rule ------------------------------------------------------------------------------------------------------------------
def test_capacity_rule(rt):
    A = rt._abi
    batch = _three_images()
    files, at = _want(rt, batch, True)
    total = at[-1]
    rc, offsets, d_offsets, buf, _ = _format(rt, batch, True, capacity=total - 1)  # one byte less: refused on the device, nothing written
    assert rc == A.RT_ERR_INVALID_ARGUMENT and rt.lib.rt_last_error().decode() == f"out_capacity {total - 1} below the {total} bytes needed"
    assert offsets == at and d_offsets == at and (buf == SENTINEL).all()
    rc, offsets, d_offsets, buf, _ = _format(rt, batch, True, capacity=total - 1, want_offsets=False)  # nobody to tell: RT_OK and the same evidence
    assert rc == A.RT_OK and d_offsets == at and (buf == SENTINEL).all()
    _assert_exact(_format(rt, batch, True, capacity=total), files, at)  # exactly the total: the sentinel beyond it intact
    rc, offsets, d_offsets, buf, _ = _format(rt, batch, True, no_out=True)  # d_out = NULL: the offsets alone
    assert rc == A.RT_OK and offsets == at and d_offsets == at and (buf == SENTINEL).all()


# ---- 6: streams ----------------------------------------------------------------------------------------------------------------------------
def test_two_batches_in_flight_and_the_current_device_untouched(rt, orc):
    """Without `offsets` the call does not synchronise: two batches are enqueued on two streams behind one another, then both are waited for."""
    torch = _torch()
    prev = torch.cuda.current_device()
    batches = [_three_images(), _shared_edges()]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    held = []
    for batch in batches:
        k, rows, cols = batch.shape[:3]
        src = torch.from_numpy(np.array(batch, np.uint8)).cuda()
        cap = int(rt.lib.rt_png_views_max_bytes(k, rows, cols))
        out = torch.full((cap + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
        d_off = torch.full((k + 1,), -7, dtype=torch.int64, device="cuda")
        held.append((src, out, d_off, cap))
    torch.cuda.synchronize()
    for (src, out, d_off, cap), batch, s in zip(held, batches, streams):
        k, rows, cols = batch.shape[:3]
        assert rt.lib.rt_format_png_views_device(0, src.data_ptr(), k, rows, cols, 1, out.data_ptr(), cap, d_off.data_ptr(), s.cuda_stream, None) == 0
    for s in streams:
        s.synchronize()
    assert torch.cuda.current_device() == prev
    for (src, out, d_off, cap), batch in zip(held, batches):
        files, at = _want(rt, batch, True)
        _assert_exact((0, None, d_off.cpu().tolist(), out.cpu().numpy(), 0), files, at)


# ---- 7: the pipeline -----------------------------------------------------------------------------------------------------------------------
W, H, SPP, DEPTH = 4, 2, 20, 12  # a 9 x 5 frame


@functools.lru_cache(maxsize=None)
def _views(rt):
    """small_final's spheres, its own camera and two moved aside: (scene, cameras)."""
    objs, cam, _, _ = scenes.small_final()
    cam = dataclasses.replace(cam, BounceDepth=DEPTH, SamplesPerPixel=SPP)
    a = cam.to_abi()
    eye, xo, xd, yd = (np.array(list(v)) for v in (a.view_origin, a.xaxis_origin, a.xaxis_dir, a.yaxis_dir))
    cams = [cam] + [scenes.free_camera(eye + s * xd, xo + s * xd, xd + 0.05 * yd, yd - 0.03 * xd, a.viewport_width, a.viewport_height, SPP, DEPTH) for s in (0.4, -0.3)]
    return rt.Scene.make(objs), cams


@functools.lru_cache(maxsize=None)
def _rendered(rt, seeds):
    """rt_render_views' rgb for the arguments of the pipeline tests: per-view seeds, or (seeds None) one seed, 5.  Computed once, never written to."""
    scene, cams = _views(rt)
    rgb = scene.renderViews(W, H, cams, seeds=seeds, seed=5).rgb
    rgb.setflags(write=False)
    return rgb


@pytest.mark.parametrize("seeds", [(3, 4, 9), None])
@pytest.mark.parametrize("gamma", [True, False])
def test_render_views_png_writes_the_rendered_views(rt, orc, tmp_path, seeds, gamma):
    A = rt._abi
    scene, cams = _views(rt)
    rgb = _rendered(rt, seeds)
    assert rgb.shape == (3, 5, 9, 3) and len({rgb[v].tobytes() for v in range(3)}) == 3
    files, _ = _want(rt, rgb, gamma)
    names = [str(tmp_path / f"view{v}.png").encode() for v in range(3)]
    abi = (A.rt_camera * 3)(*[c.to_abi() for c in cams])
    keys = None if seeds is None else (C.c_uint64 * 3)(*seeds)
    st = A.rt_stats()
    assert rt.lib.rt_render_views_png(scene.handle, abi, 3, W, H, keys, 5, 0, 0, int(gamma), (C.c_char_p * 3)(*names), None, C.byref(st)) == 0, rt.lib.rt_last_error()
    assert [open(n, "rb").read() for n in names] == files
    _decodes(orc, files, rgb, gamma)
    assert st.pixels == 3 * 45 and st.samples > 0 and st.total_ms >= st.kernel_ms > 0


def test_write_png_views_device_of_a_device_render(rt, orc, tmp_path):
    torch = _torch()
    A = rt._abi
    scene, cams = _views(rt)
    rgb = _rendered(rt, (3, 4, 9))
    files, _ = _want(rt, rgb, True)
    abi = (A.rt_camera * 3)(*[c.to_abi() for c in cams])
    d_accum = torch.zeros((3, 5, 9, 4), dtype=torch.int32, device="cuda")
    d_rgb = torch.zeros((3, 5, 9, 3), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert rt.lib.rt_render_views_device(scene.handle, abi, 3, W, H, (C.c_uint64 * 3)(3, 4, 9), 5, 0, 0, d_accum.data_ptr(), d_rgb.data_ptr(), st, None, None) == 0
    names = [str(tmp_path / f"device{v}.png").encode() for v in range(3)]
    assert rt.lib.rt_write_png_views_device((C.c_char_p * 3)(*names), 0, d_rgb.data_ptr(), 3, 5, 9, 1, st) == 0
    assert [open(n, "rb").read() for n in names] == files
    # an unwritable paths[1]: RT_ERR_IO naming it, and paths[0] is written
    bad = [str(tmp_path / "bad0.png").encode(), str(tmp_path / "missing" / "bad1.png").encode(), str(tmp_path / "bad2.png").encode()]
    assert rt.lib.rt_write_png_views_device((C.c_char_p * 3)(*bad), 0, d_rgb.data_ptr(), 3, 5, 9, 1, st) == A.RT_ERR_IO
    assert rt.lib.rt_last_error().decode() == "cannot open " + bad[1].decode()
    assert open(bad[0], "rb").read() == files[0] and not os.path.exists(bad[2])
    assert rt.lib.rt_render_views_png(scene.handle, abi, 3, W, H, (C.c_uint64 * 3)(3, 4, 9), 5, 0, 0, 1, (C.c_char_p * 3)(*bad), None, None) == A.RT_ERR_IO
    assert rt.lib.rt_last_error().decode() == "cannot open " + bad[1].decode() and open(bad[0], "rb").read() == files[0]
    torch.cuda.synchronize()


# ---- 8: Python tensors ---------------------------------------------------------------------------------------------------------------------
def test_python_tensor_routes(rt, orc, tmp_path):
    torch = _torch()
    batch = _shared_edges()
    t = torch.from_numpy(np.array(batch, np.uint8)).cuda()
    for gamma in (False, True):
        files, at = _want(rt, batch, gamma)
        data, offsets = rt.Png.formatViewsDevice(gamma, t)
        assert data.dtype == torch.uint8 and data.is_cuda and data.numel() == rt.lib.rt_png_views_max_bytes(4, 5, 3)
        assert offsets.dtype == torch.int64 and offsets.is_cuda and offsets.cpu().tolist() == at
        assert data[: at[-1]].cpu().numpy().tobytes() == b"".join(files)
        assert rt.Png.formatViews(gamma, t) == files == rt.Png.formatViews(gamma, batch)
        paths = [tmp_path / f"t{int(gamma)}_{v}.png" for v in range(4)]
        rt.Png.writeViews(gamma, t, paths)
        assert [p.read_bytes() for p in paths] == files
    with pytest.raises(ValueError):
        rt.Png.formatViews(False, t[0])
    with pytest.raises(TypeError):
        rt.Png.formatViews(False, t.to(torch.int32))
    scene, cams = _views(rt)
    rgb = _rendered(rt, (3, 4, 9))
    paths = [tmp_path / f"scene{v}.png" for v in range(3)]
    stats = scene.renderViewsPng(W, H, cams, paths, gammaCorrect=True, seeds=(3, 4, 9), seed=5)
    assert [p.read_bytes() for p in paths] == _want(rt, rgb, True)[0]
    assert stats["pixels"] == 3 * 45 and stats["total_ms"] >= stats["kernel_ms"] > 0


# ---- 9: the C program ----------------------------------------------------------------------------------------------------------------------
def test_c_program_encodes_three_golden_images(rt, orc, tmp_path):
    exe = str(tmp_path / "png_views_smoke")
    libdir = os.path.join(ROOT, "ray-tracing-fsharp_amd")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "png_views_smoke.c"),
                           "-L", libdir, "-lrtfs_amd", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "png views: encoded on the GPU" in out.stdout
    lines = dict(line.split(" ", 1) for line in out.stdout.splitlines() if line.startswith("file"))
    batch = np.stack([pc.GOLDEN_IMAGE, pc.GOLDEN_IMAGE[:, :, ::-1], 255 - pc.GOLDEN_IMAGE])  # the image, channel-reversed, negative
    files, _ = _want(rt, batch, False)
    assert [bytes.fromhex(lines[f"file{v}"]) for v in range(3)] == files == [(tmp_path / f"c_view{v}.png").read_bytes() for v in range(3)]
    _decodes(orc, files, batch, False)
