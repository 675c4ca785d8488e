"""The output stage on the device -- rt_format_ppm_device, rt_format_pixel_map_device, rt_gamma_correct_device, rt_write_ppm_device,
rt_render_ppm and their Python, C and driver callers -- byte for byte against the oracle's own formatters (oracle.format_ppm,
oracle.format_pixel_map, oracle.gamma_correct) and the reference's golden PPM text; never against the library's host functions alone.
Every output buffer is allocated 64 bytes larger than the capacity the call is given and filled with a sentinel; the bytes at and
beyond the reported length must be the sentinel still."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5
SLACK = 64
GOLDEN_IMAGE = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255]], [[255, 255, 0], [255, 255, 255], [0, 0, 0]]], np.uint8)  # TestPpmOutput.fs:12-46


def _golden_text():
    return open(os.path.join(ROOT, "tests", "golden", "PpmOutputExample.txt"), "rb").read().replace(b"\r\n", b"\n")


def _torch():
    return pytest.importorskip("torch")


def _digits_image(rows, cols, seed):
    """Random bytes with one, two and three decimal digits about a third each, so that pixel lengths really vary."""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 3, (rows, cols, 3))
    lo = np.array([0, 10, 100])[kind]
    hi = np.array([10, 100, 256])[kind]
    return (lo + (rng.random((rows, cols, 3)) * (hi - lo)).astype(np.int64)).astype(np.uint8)


def _format(rt, which, img, gamma=False, *, capacity=None, in_offset=0, out_offset=0, want_length=True, stream=None):
    """One device format call on raw pointers.  Returns (rc, host length or None, d_length, the whole output allocation as numpy,
    out_offset): the output buffer starts out_offset bytes into an allocation of out_offset + capacity + SLACK sentinel bytes."""
    torch = _torch()
    rows, cols = img.shape[0], img.shape[1]
    need = rt.lib.rt_ppm_max_bytes(rows, cols) if which == "ppm" else rt.lib.rt_pixel_map_bytes(rows, cols)
    capacity = int(need) if capacity is None else capacity
    src = torch.empty(img.size + in_offset, dtype=torch.uint8, device="cuda")
    src[in_offset:] = torch.from_numpy(np.ascontiguousarray(img).reshape(-1)).cuda()
    out = torch.full((out_offset + capacity + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_len = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    length = C.c_int64(-7)
    st = (stream or torch.cuda.current_stream()).cuda_stream
    head = (0, src.data_ptr() + in_offset, rows, cols)
    tail = (out.data_ptr() + out_offset, capacity, d_len.data_ptr(), st, C.byref(length) if want_length else None)
    rc = rt.lib.rt_format_ppm_device(*head, int(gamma), *tail) if which == "ppm" else rt.lib.rt_format_pixel_map_device(*head, *tail)
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
        raise AssertionError(f"byte {first} of {len(want)} differs: got {got[max(0, first - 12):first + 12]!r}, want {want[max(0, first - 12):first + 12]!r}")
    assert (buf[off + len(want):] == SENTINEL).all(), "bytes at or beyond the needed length were written"


def _expect(orc, which, img, gamma=False):
    return orc.format_ppm(img, gamma=gamma) if which == "ppm" else orc.format_pixel_map(img)


# ---- golden file, separators ---------------------------------------------------------------------------------------------------------
def test_golden_ppm_example(rt, orc):
    want = _golden_text()
    assert want == orc.format_ppm(GOLDEN_IMAGE, gamma=False) and len(want) == 62
    _assert_exact(_format(rt, "ppm", GOLDEN_IMAGE), want)


@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (2, 1), (1, 64), (64, 1)])
@pytest.mark.parametrize("which", ["ppm", "map"])
def test_separators_at_every_edge(rt, orc, shape, which):
    img = _digits_image(*shape, seed=shape[0] * 100 + shape[1])
    want = _expect(orc, which, img)
    if which == "ppm":
        assert not want.endswith((b" ", b"\n")) and want.count(b"\n") == 3 + shape[0] - 1
    _assert_exact(_format(rt, which, img), want)


# ---- digits and gamma ----------------------------------------------------------------------------------------------------------------
def _every_byte_image():
    v = np.arange(256, dtype=np.int64)
    return np.stack([v, (v * 7 + 3) % 256, 255 - v], axis=1).astype(np.uint8).reshape(16, 16, 3)  # each channel a permutation of 0..255


@pytest.mark.parametrize("gamma", [False, True])
def test_every_byte_value_in_every_channel(rt, orc, gamma):
    img = _every_byte_image()
    for ch in range(3):
        assert sorted(img[:, :, ch].reshape(-1).tolist()) == list(range(256))
    _assert_exact(_format(rt, "ppm", img, gamma), orc.format_ppm(img, gamma=gamma))
    _assert_exact(_format(rt, "map", img), orc.format_pixel_map(img))


def test_gamma_correct_device_out_of_place_and_in_place(rt, orc):
    torch = _torch()
    want = np.array([orc.gamma_correct(b) for b in range(256)], np.uint8)
    st = torch.cuda.current_stream().cuda_stream
    for offset in (0, 1, 2, 3):  # any alignment; source and destination misaligned alike, and differently
        for out_offset in (offset, (offset + 1) % 4):
            src = torch.full((256 + offset + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
            src[offset:offset + 256] = torch.arange(256, dtype=torch.int32, device="cuda").to(torch.uint8)
            before = src.cpu().numpy().copy()
            dst = torch.full((256 + out_offset + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
            assert rt.lib.rt_gamma_correct_device(0, 256, src.data_ptr() + offset, dst.data_ptr() + out_offset, st) == 0
            torch.cuda.synchronize()
            got = dst.cpu().numpy()
            assert (got[out_offset:out_offset + 256] == want).all()
            assert (got[:out_offset] == SENTINEL).all() and (got[out_offset + 256:] == SENTINEL).all()
            assert (src.cpu().numpy() == before).all()
        assert rt.lib.rt_gamma_correct_device(0, 256, src.data_ptr() + offset, src.data_ptr() + offset, st) == 0  # in place
        torch.cuda.synchronize()
        got = src.cpu().numpy()
        assert (got[offset:offset + 256] == want).all() and (got[:offset] == SENTINEL).all() and (got[offset + 256:] == SENTINEL).all()
    t = torch.from_numpy(_every_byte_image()).cuda()
    assert (rt.PixelOutput.correctImage(t).cpu().numpy() == want[_every_byte_image()]).all()
    for n in (1, 5, 4099):  # fewer bytes than a dword; a ragged tail behind many dwords
        src = torch.from_numpy((np.arange(n) % 256).astype(np.uint8)).cuda()
        dst = torch.full((n + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert rt.lib.rt_gamma_correct_device(0, n, src.data_ptr(), dst.data_ptr(), st) == 0
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        assert (got[:n] == want[np.arange(n) % 256]).all() and (got[n:] == SENTINEL).all()


# ---- tile boundaries -----------------------------------------------------------------------------------------------------------------
WIDTHS = sorted({(1 << k) + d for k in range(6, 17) for d in (-1, 0, 1)})


@pytest.mark.parametrize("which", ["ppm", "map"])
def test_one_row_images_around_every_power_of_two(rt, orc, which):
    """1 x p for p = 2^k - 1, 2^k, 2^k + 1, k = 6..16: a tile is 1024 pixels, so these end inside the first tile, on a tile's last pixel, on
    the first pixel of the next, and run to 65 tiles."""
    for p in WIDTHS:
        img = _digits_image(1, p, seed=p)
        _assert_exact(_format(rt, which, img, gamma=(p % 2 == 1)), _expect(orc, which, img, gamma=(p % 2 == 1)))


@pytest.mark.parametrize("which", ["ppm", "map"])
def test_more_tile_sums_than_the_scanning_workgroup_has_threads(rt, orc, which):
    """1025 x 1025 = 1,050,625 pixels = 1027 tiles of 1024: the one scanning workgroup (1024 threads) makes a second trip, which begins at
    2^20 pixels -- the only threshold of the scan, and this image is past it."""
    img = _digits_image(1025, 1025, seed=1025)
    _assert_exact(_format(rt, which, img, gamma=True), _expect(orc, which, img, gamma=True))


@pytest.mark.parametrize("shape", [(12, 103), (101, 11), (2, 1002)])
def test_pixel_map_digit_counts_change_in_both_coordinates(rt, orc, shape):
    """9 -> 10, 99 -> 100 and 999 -> 1000 in rows and columns, and the EMPTY digits of row 0 and column 0 (ImageOutput.fs:115-129)."""
    img = _digits_image(*shape, seed=shape[1])
    want = orc.format_pixel_map(img)
    assert want[:2] == b",\n" and len(want) == rt.lib.rt_pixel_map_bytes(*shape)
    _assert_exact(_format(rt, "map", img), want)


# ---- alignment, capacity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["ppm", "map"])
def test_any_byte_alignment_of_image_and_output(rt, orc, which):
    img = _digits_image(37, 53, seed=37)
    want = _expect(orc, which, img, gamma=True)
    for in_offset, out_offset in ((1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (1, 3), (2, 2), (3, 1)):
        _assert_exact(_format(rt, which, img, gamma=True, in_offset=in_offset, out_offset=out_offset), want)


@pytest.mark.parametrize("which", ["ppm", "map"])
def test_capacity_rule(rt, orc, which):
    torch = _torch()
    A = rt._abi
    img = _digits_image(37, 53, seed=53)
    want = _expect(orc, which, img)
    n = len(want)
    _assert_exact(_format(rt, which, img, capacity=n), want)  # exactly the needed length
    rc, length, d_length, buf, _ = _format(rt, which, img, capacity=n - 1)  # one byte less: refused on the device, nothing written
    assert rc == A.RT_ERR_INVALID_ARGUMENT and rt.lib.rt_last_error().decode() == f"out_capacity {n - 1} below the {n} bytes needed"
    assert length == n and d_length == n and (buf == SENTINEL).all()
    rc, length, d_length, buf, _ = _format(rt, which, img, capacity=n - 1, want_length=False)  # nobody to tell: RT_OK and the same evidence
    assert rc == A.RT_OK and d_length == n and (buf == SENTINEL).all()
    rc, length, d_length, buf, _ = _format(rt, which, img, capacity=1)
    assert rc == A.RT_ERR_INVALID_ARGUMENT and length == n and (buf == SENTINEL).all()
    # d_out = NULL: the lengths alone
    src = torch.from_numpy(img).cuda()
    d_len = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    length = C.c_int64(-7)
    st = torch.cuda.current_stream().cuda_stream
    if which == "ppm":
        rc = rt.lib.rt_format_ppm_device(0, src.data_ptr(), 37, 53, 0, None, 0, d_len.data_ptr(), st, C.byref(length))
    else:
        rc = rt.lib.rt_format_pixel_map_device(0, src.data_ptr(), 37, 53, None, 0, d_len.data_ptr(), st, C.byref(length))
    assert rc == A.RT_OK and length.value == n and int(d_len.item()) == n


# ---- streams -------------------------------------------------------------------------------------------------------------------------
def test_two_streams_in_flight_and_the_current_device_untouched(rt, orc):
    torch = _torch()
    prev = torch.cuda.current_device()
    images = [_digits_image(201, 301, seed=1), _digits_image(150, 407, seed=2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    held = []
    for img, s in zip(images, streams):
        src = torch.from_numpy(img).cuda()
        cap = int(rt.lib.rt_ppm_max_bytes(img.shape[0], img.shape[1]))
        out = torch.full((cap + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
        d_len = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        held.append((src, out, d_len))
    torch.cuda.synchronize()
    for (src, out, d_len), img, s in zip(held, images, streams):
        assert rt.lib.rt_format_ppm_device(0, src.data_ptr(), img.shape[0], img.shape[1], 1, out.data_ptr(), out.numel() - SLACK, d_len.data_ptr(),
                                           s.cuda_stream, None) == 0
    for s in streams:
        s.synchronize()
    assert torch.cuda.current_device() == prev
    for (src, out, d_len), img in zip(held, images):
        _assert_exact((0, None, int(d_len.item()), out.cpu().numpy(), 0), orc.format_ppm(img, gamma=True))


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _smoke_frame(rt, orc):
    """smoke()'s scene and the oracle's render of it: (objects, camera, max_w, max_h, oracle rgb).  Computed once, never written to."""
    objs, cam, w, h = rt.sample_images.config3_final(seed=2024, spp=40, depth=50, pixels=12)
    _, rgb, _ = orc.OracleScene(objs).render_rows(w, h, cam.to_abi(), seed=1, threads=4)
    rgb.setflags(write=False)
    return objs, cam, w, h, rgb


@pytest.mark.parametrize("gamma", [True, False])
def test_render_ppm_writes_the_oracle_frame(rt, orc, tmp_path, gamma):
    objs, cam, w, h, rgb = _smoke_frame(rt, orc)
    path = str(tmp_path / "frame.ppm")
    stats = rt.Scene.make(objs).renderPpm(w, h, cam, path, gammaCorrect=gamma, seed=1)
    assert open(path, "rb").read() == orc.format_ppm(rgb, gamma=gamma)
    assert stats["pixels"] == rgb.shape[0] * rgb.shape[1] and stats["samples"] > 0 and stats["total_ms"] >= stats["kernel_ms"] > 0


def test_write_ppm_device_of_a_device_render(rt, orc, tmp_path):
    torch = _torch()
    objs, cam, w, h, rgb = _smoke_frame(rt, orc)
    rows, cols = rgb.shape[0], rgb.shape[1]
    scene, cam_abi = rt.Scene.make(objs), cam.to_abi()
    d_accum = torch.zeros((rows, cols, 4), dtype=torch.int32, device="cuda")
    d_rgb = torch.zeros((rows, cols, 3), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert rt.lib.rt_render_device(scene.handle, C.byref(cam_abi), w, h, 1, 0, 0, 1, rows, 0, d_accum.data_ptr(), d_rgb.data_ptr(), st, None) == 0
    path = str(tmp_path / "device.ppm")
    assert rt.lib.rt_write_ppm_device(path.encode(), 0, d_rgb.data_ptr(), rows, cols, 1, st) == 0
    assert open(path, "rb").read() == orc.format_ppm(rgb, gamma=True)


def test_driver_writes_the_same_file_by_both_routes(rt, tmp_path):
    host = os.path.join(ROOT, "ray-tracing-fsharp_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s"])
    outs = []
    for extra in ((), ("--host-output",)):
        path = tmp_path / f"driver{len(outs)}.ppm"
        r = subprocess.run([os.path.join(host, "rtfs_render"), "glass", str(path), "--scale", "20", "--spp", "20", "--seed", "8", *extra],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs.append((path.read_bytes(), r.stdout.replace(str(path), "PATH"), r.stderr.split(", kernel")[0]))
    assert outs[0] == outs[1] and outs[0][0].startswith(b"P3\n")


def test_c_program_formats_the_golden_image(rt, orc, tmp_path):
    from test_output_host import build_output_smoke

    out = subprocess.run([build_output_smoke(tmp_path), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "output: formatted on the GPU" in out.stdout
    lines = dict(line.split(" ", 1) for line in out.stdout.splitlines() if line.split(" ", 1)[0] in ("ppm", "map", "gamma"))
    assert bytes.fromhex(lines["ppm"]) == _golden_text()
    assert bytes.fromhex(lines["map"]) == orc.format_pixel_map(GOLDEN_IMAGE)
    assert list(bytes.fromhex(lines["gamma"])) == [orc.gamma_correct(int(b)) for b in GOLDEN_IMAGE.reshape(-1)]
    assert (tmp_path / "c_write.ppm").read_bytes() == _golden_text()
    assert (tmp_path / "c_render.ppm").read_bytes().startswith(b"P3\n3 3\n255\n")


# ---- Python tensors ------------------------------------------------------------------------------------------------------------------
def test_python_tensor_routes(rt, orc, tmp_path):
    torch = _torch()
    img = _digits_image(45, 67, seed=45)
    t = torch.from_numpy(img).cuda()
    for gamma in (False, True):
        want = orc.format_ppm(img, gamma=gamma)
        assert rt.ImageOutput.formatPpm(gamma, t) == want == rt.ImageOutput.formatPpm(gamma, t.cpu().numpy())
        text, length = rt.ImageOutput.formatPpmDevice(gamma, t)
        assert text.dtype == torch.uint8 and text.is_cuda and text.numel() == rt.lib.rt_ppm_max_bytes(45, 67) and length.dtype == torch.int64
        assert int(length) == len(want) and text[: int(length)].cpu().numpy().tobytes() == want
        path = str(tmp_path / "tensor.ppm")
        ticks = []
        rt.ImageOutput.writePpm(gamma, ticks.append, t, path)
        assert open(path, "rb").read() == want and len(ticks) == 45 * 67
    assert rt.ImageOutput.formatPixelMap(t) == orc.format_pixel_map(img)
    with pytest.raises(ValueError):
        rt.ImageOutput.formatPpm(False, t[:, :, :2])
    with pytest.raises(TypeError):
        rt.ImageOutput.formatPpm(False, t.to(torch.int32))
