"""Png.write on the device -- rt_format_png_device, rt_write_png_device, rt_render_png and their Python and C callers.  The device bytes
must equal the host formatter's (rt_format_png) byte for byte, and the file is decoded by the tests' own decoder and PIL
(png_cases.decode) to oracle.gamma_correct of the image: never held to the library's host function alone.  Every output buffer is
allocated 64 bytes larger than the capacity the call is given, behind `out_offset` more, and filled with a sentinel; nothing in front of
the buffer and nothing at or beyond the reported length may be written."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import png_cases as pc
from test_png_host import T0, build_png_smoke, check_file, host_png

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
SLACK = 64


def _torch():
    return pytest.importorskip("torch")


def _format(rt, img, gamma=False, *, capacity=None, in_offset=0, out_offset=0, want_length=True, stream=None):
    """One rt_format_png_device call on raw pointers: (rc, host length or None, d_length, the whole output allocation, out_offset)."""
    torch = _torch()
    rows, cols = img.shape[0], img.shape[1]
    capacity = int(rt.lib.rt_png_max_bytes(rows, cols)) if capacity is None else capacity
    src = torch.empty(img.size + in_offset, dtype=torch.uint8, device="cuda")
    src[in_offset:] = torch.from_numpy(np.array(img, np.uint8).reshape(-1)).cuda()
    out = torch.full((out_offset + capacity + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_len = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    length = C.c_int64(-7)
    st = (stream or torch.cuda.current_stream()).cuda_stream
    rc = rt.lib.rt_format_png_device(0, src.data_ptr() + in_offset, rows, cols, int(gamma), out.data_ptr() + out_offset, capacity, d_len.data_ptr(), st,
                                     C.byref(length) if want_length else None)
    torch.cuda.synchronize()
    return rc, (length.value if want_length else None), int(d_len.item()), out.cpu().numpy(), out_offset


def _assert_exact(result, want):
    rc, length, d_length, buf, off = result
    assert rc == 0
    assert d_length == len(want) and (length is None or length == len(want))
    assert (buf[:off] == SENTINEL).all(), "bytes in front of the buffer were written"
    got = buf[off:off + len(want)].tobytes()
    if got != want:
        first = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError(f"byte {first} of {len(want)} differs: got {got[max(0, first - 12):first + 12].hex()}, want {want[max(0, first - 12):first + 12].hex()}")
    assert (buf[off + len(want):] == SENTINEL).all(), "bytes at or beyond the needed length were written"


def _device_equals_host_and_decodes(rt, orc, img, gamma):
    want = host_png(rt, img, gamma)
    _assert_exact(_format(rt, img, gamma), want)
    check_file(rt, orc, want, img, gamma)  # the very bytes the device wrote


# ---- every case of the host file ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", [False, True])
def test_golden_and_every_byte_images(rt, orc, gamma):
    for img in (pc.GOLDEN_IMAGE, pc.every_byte_image()) + tuple(i for _, i in pc.golden_frames()):
        _device_equals_host_and_decodes(rt, orc, img, gamma)


@pytest.mark.parametrize("name", [n for n, _ in pc.shape_cases(T0)])
def test_shapes(rt, orc, name):
    img = dict(pc.shape_cases(T0))[name]
    _device_equals_host_and_decodes(rt, orc, img, img.shape[1] % 2 == 1)


@pytest.mark.parametrize("name", [n for n, _ in pc.run_cases(T0)])
def test_runs(rt, orc, name):
    _device_equals_host_and_decodes(rt, orc, dict(pc.run_cases(T0))[name], False)


@pytest.mark.parametrize("name", [n for n, _, _ in pc.histogram_cases(T0)])
def test_histograms(rt, orc, name):
    _device_equals_host_and_decodes(rt, orc, {n: i for n, i, _ in pc.histogram_cases(T0)}[name], False)


# ---- alignment, capacity -------------------------------------------------------------------------------------------------------------
def test_any_byte_alignment_of_image_and_output(rt, orc):
    img = pc.golden_frames()[3][1]  # Huffman tiles: bits are OR-ed into words at every alignment
    noisy = pc.noise(3, 1825, 8)    # stored tiles, two of them
    for image in (img, noisy):
        want = host_png(rt, image, True)
        for in_offset in range(4):
            for out_offset in range(4):
                _assert_exact(_format(rt, image, True, in_offset=in_offset, out_offset=out_offset), want)


def test_capacity_rule(rt):
    torch = _torch()
    A = rt._abi
    img = pc.golden_frames()[1][1]
    want = host_png(rt, img)
    n = len(want)
    _assert_exact(_format(rt, img, capacity=n), want)  # exactly the needed length
    rc, length, d_length, buf, _ = _format(rt, img, capacity=n - 1)  # one byte less: refused on the device, nothing written
    assert rc == A.RT_ERR_INVALID_ARGUMENT and rt.lib.rt_last_error().decode() == f"out_capacity {n - 1} below the {n} bytes needed"
    assert length == n and d_length == n and (buf == SENTINEL).all()
    rc, length, d_length, buf, _ = _format(rt, img, capacity=n - 1, want_length=False)  # nobody to tell: RT_OK and the same evidence
    assert rc == A.RT_OK and d_length == n and (buf == SENTINEL).all()
    rc, length, d_length, buf, _ = _format(rt, img, capacity=1)
    assert rc == A.RT_ERR_INVALID_ARGUMENT and length == n and (buf == SENTINEL).all()
    # d_out = NULL: the length alone
    src = torch.from_numpy(np.array(img, np.uint8)).cuda()
    d_len = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    length = C.c_int64(-7)
    st = torch.cuda.current_stream().cuda_stream
    rc = rt.lib.rt_format_png_device(0, src.data_ptr(), img.shape[0], img.shape[1], 0, None, 0, d_len.data_ptr(), st, C.byref(length))
    assert rc == A.RT_OK and length.value == n and int(d_len.item()) == n


# ---- streams -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mostly_constant_image():
    """2400 x 2400, constant but for a sprinkle of pixels and one noisy band: 17,282,400 filtered bytes = 1055 tiles, more than the scanning
    workgroup's RTO_SCAN_THREADS = 1024, so the scan makes its second trip; nearly all runs, so both sides are quick."""
    rng = np.random.default_rng(24)
    img = np.full((2400, 2400, 3), 90, np.uint8)
    ys, xs = rng.integers(0, 2400, 4000), rng.integers(0, 2400, 4000)
    img[ys, xs] = rng.integers(0, 256, (4000, 3), dtype=np.uint8)
    img[1200:1203] = rng.integers(0, 256, (3, 2400, 3), dtype=np.uint8)
    img.setflags(write=False)
    return img


def test_two_streams_in_flight_and_the_current_device_untouched(rt, orc):
    """Without `length` the call does not synchronise: two calls are enqueued on two streams behind one another, then both are waited for."""
    torch = _torch()
    prev = torch.cuda.current_device()
    images = [pc.golden_frames()[0][1], pc.noise(201, 301, 2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    held = []
    for img in images:
        src = torch.from_numpy(np.array(img, np.uint8)).cuda()
        cap = int(rt.lib.rt_png_max_bytes(img.shape[0], img.shape[1]))
        out = torch.full((cap + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
        d_len = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        held.append((src, out, d_len))
    torch.cuda.synchronize()
    for (src, out, d_len), img, s in zip(held, images, streams):
        assert rt.lib.rt_format_png_device(0, src.data_ptr(), img.shape[0], img.shape[1], 1, out.data_ptr(), out.numel() - SLACK, d_len.data_ptr(),
                                           s.cuda_stream, None) == 0
    for s in streams:
        s.synchronize()
    assert torch.cuda.current_device() == prev
    for (src, out, d_len), img in zip(held, images):
        _assert_exact((0, None, int(d_len.item()), out.cpu().numpy(), 0), host_png(rt, img, True))


def test_more_tiles_than_the_scanning_workgroup_has_threads(rt, orc):
    img = _mostly_constant_image()
    assert -(-2400 * 7201 // T0) > 1024
    want = host_png(rt, img, True)
    assert len(want) < img.size // 50
    _assert_exact(_format(rt, img, True), want)
    px, _ = pc.decode(want)
    assert np.array_equal(px, pc.expected_pixels(orc, img, True))


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small_frame(rt):
    """A small catalogue scene and rt_render's rgb of it: (objects, camera, max_w, max_h, rgb).  Computed once, never written to."""
    objs, cam, w, h = rt.sample_images.config3_final(seed=2024, spp=40, depth=50, pixels=12)
    rgb = rt.Scene.make(objs).render_rows(w, h, cam, seed=1).rgb
    rgb.setflags(write=False)
    return objs, cam, w, h, rgb


@pytest.mark.parametrize("gamma", [True, False])
def test_render_png_writes_the_rendered_frame(rt, orc, tmp_path, gamma):
    objs, cam, w, h, rgb = _small_frame(rt)
    path = str(tmp_path / "frame.png")
    stats = rt.Scene.make(objs).renderPng(w, h, cam, path, gammaCorrect=gamma, seed=1)
    data = open(path, "rb").read()
    assert np.array_equal(pc.decode(data)[0], pc.expected_pixels(orc, rgb, gamma))  # rt_render's rgb after gamma
    assert data == host_png(rt, rgb, gamma)
    assert stats["pixels"] == rgb.shape[0] * rgb.shape[1] and stats["samples"] > 0 and stats["total_ms"] >= stats["kernel_ms"] > 0


def test_write_png_device_of_a_device_render(rt, orc, tmp_path):
    torch = _torch()
    A = rt._abi
    objs, cam, w, h, rgb = _small_frame(rt)
    rows, cols = rgb.shape[0], rgb.shape[1]
    scene, cam_abi = rt.Scene.make(objs), cam.to_abi()
    d_accum = torch.zeros((rows, cols, 4), dtype=torch.int32, device="cuda")
    d_rgb = torch.zeros((rows, cols, 3), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert rt.lib.rt_render_device(scene.handle, C.byref(cam_abi), w, h, 1, 0, 0, 1, rows, 0, d_accum.data_ptr(), d_rgb.data_ptr(), st, None) == 0
    path = str(tmp_path / "device.png")
    assert rt.lib.rt_write_png_device(path.encode(), 0, d_rgb.data_ptr(), rows, cols, 1, st) == 0
    data = open(path, "rb").read()
    assert np.array_equal(pc.decode(data)[0], pc.expected_pixels(orc, rgb, True)) and data == host_png(rt, rgb, True)
    # an unopenable path: RT_ERR_IO with no device work -- the image pointer is one the device could not read
    bad = str(tmp_path / "missing" / "x.png").encode()
    host_rgb = np.full(rows * cols * 3, 7, np.uint8)
    assert rt.lib.rt_write_png_device(bad, 0, host_rgb.ctypes.data, rows, cols, 1, st) == A.RT_ERR_IO
    assert rt.lib.rt_last_error().decode() == "cannot open " + bad.decode()
    assert rt.lib.rt_render_png(scene.handle, C.byref(cam_abi), w, h, 1, 0, 0, 1, bad, None, None) == A.RT_ERR_IO
    torch.cuda.synchronize()


def test_c_program_encodes_the_golden_image(rt, orc, tmp_path):
    out = subprocess.run([build_png_smoke(tmp_path), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "png: encoded on the GPU" in out.stdout
    lines = dict(line.split(" ", 1) for line in out.stdout.splitlines() if line.split(" ", 1)[0] in ("host", "device"))
    want = host_png(rt, pc.GOLDEN_IMAGE)
    assert bytes.fromhex(lines["device"]) == want == (tmp_path / "c_device.png").read_bytes()
    check_file(rt, orc, want, pc.GOLDEN_IMAGE, False)
    assert pc.decode((tmp_path / "c_render.png").read_bytes())[0].shape == (3, 3, 3)


# ---- Python tensors ------------------------------------------------------------------------------------------------------------------
def test_python_tensor_routes(rt, orc, tmp_path):
    torch = _torch()
    img = pc.golden_frames()[2][1]
    t = torch.from_numpy(np.array(img, np.uint8)).cuda()
    for gamma in (False, True):
        want = host_png(rt, img, gamma)
        assert rt.Png.format(gamma, t) == want == rt.Png.format(gamma, img)
        data, length = rt.Png.formatDevice(gamma, t)
        assert data.dtype == torch.uint8 and data.is_cuda and data.numel() == rt.lib.rt_png_max_bytes(*img.shape[:2]) and length.dtype == torch.int64
        assert int(length) == len(want) and data[: int(length)].cpu().numpy().tobytes() == want
        path = str(tmp_path / "tensor.png")
        ticks = []
        rt.Png.write(gamma, ticks.append, t, path)
        assert open(path, "rb").read() == want and len(ticks) == img.shape[0] * img.shape[1] - 1
        assert np.array_equal(pc.decode(want)[0], pc.expected_pixels(orc, img, gamma))
    with pytest.raises(ValueError):
        rt.Png.format(False, t[:, :, :2])
    with pytest.raises(TypeError):
        rt.Png.format(False, t.to(torch.int32))
