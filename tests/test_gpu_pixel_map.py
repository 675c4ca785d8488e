"""Resuming from a pixel map on the device -- rt_parse_pixel_map_device, rt_missing_pixels_device, rt_scatter_pixels_device,
rt_resume_pixel_map, rt_resume_png / rt_resume_ppm and their Python callers.  The parse is held to the oracle's reader
(oracle.parse_pixel_map) byte for byte, the list and the scatter to numpy, a resumed frame to rt_render's rgb.  Every device buffer has
GUARD sentinel bytes in front of and behind it, and d_rgb is sentinel-filled: what the map does not name must be the sentinel still."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import pixel_map_cases as pmc
import scenes

pytestmark = pytest.mark.gpu

S = 0xA5
GUARD = 64
SEED = 11


def _torch():
    return pytest.importorskip("torch")


def _guarded(torch, n, fill=S, offset=0, dtype=None):
    """A device allocation of GUARD + offset + n + GUARD items filled with `fill`; the buffer proper begins at item GUARD + offset."""
    return torch.full((GUARD + offset + n + GUARD,), fill, dtype=dtype or torch.uint8, device="cuda")


def _parse(rt, data, rows, cols, *, offset=0, want_count=True, stream=None, sync=True):
    """One raw rt_parse_pixel_map_device call.  Returns (rc, host count or None, d_count, rgb allocation, present allocation) as numpy."""
    torch = _torch()
    data = bytes(data)
    src = _guarded(torch, len(data), offset=offset)
    if data:
        src[GUARD + offset:GUARD + offset + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    npx = rows * cols
    rgb, present = _guarded(torch, npx * 3, offset=offset), _guarded(torch, npx, offset=(offset * 3) % 4)
    d_count = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    count = C.c_int64(-7)
    st = (stream or torch.cuda.current_stream()).cuda_stream
    rc = rt.lib.rt_parse_pixel_map_device(0, src.data_ptr() + GUARD + offset if data else None, len(data), rows, cols, rgb.data_ptr() + GUARD + offset,
                                          present.data_ptr() + GUARD + (offset * 3) % 4, d_count.data_ptr(), st, C.byref(count) if want_count else None)
    if not sync:
        return rc, count, d_count, rgb, present, src
    torch.cuda.synchronize()
    return rc, (count.value if want_count else None), int(d_count.item()), rgb.cpu().numpy(), present.cpu().numpy()


def _assert_parse(orc, result, data, rows, cols, offset=0, what=""):
    """The device's answer is the oracle reader's: count, present in full, rgb where present, the sentinel everywhere else."""
    rc, count, d_count, rgb, present = result
    n, orgb, opresent = pmc.expected(orc, data, rows, cols)
    assert n >= 0, what
    assert rc == 0 and d_count == n and (count is None or count == n), (what, rc, count, d_count, n)
    npx, p_off = rows * cols, (offset * 3) % 4
    assert np.array_equal(present[GUARD + p_off:GUARD + p_off + npx], opresent.reshape(-1).astype(np.uint8)), what
    want = np.where(opresent.reshape(-1, 1), orgb.reshape(-1, 3), S).astype(np.uint8).reshape(-1)
    assert np.array_equal(rgb[GUARD + offset:GUARD + offset + npx * 3], want), what
    for buf, lo, hi in ((rgb, GUARD + offset, GUARD + offset + npx * 3), (present, GUARD + p_off, GUARD + p_off + npx)):
        assert (buf[:lo] == S).all() and (buf[hi:] == S).all(), f"{what}: bytes outside the buffer were written"


def _assert_untouched(result, rt, want_count=True):
    rc, count, d_count, rgb, present = result
    assert rc == (rt._abi.RT_ERR_INVALID_ARGUMENT if want_count else 0)
    assert d_count == -rt._abi.RT_ERR_INVALID_ARGUMENT and (count is None or count == -7)
    assert (rgb == S).all() and (present == S).all()


def _file_of_length(length, rows, cols, seed):
    """Records in range whose bytes are exactly `length` long: the last record's row is padded with leading zeros."""
    rng = random.Random(seed)
    out, size = [], 0
    while size + 40 < length:
        rec = pmc.random_records(rng, rows, cols, 1, zeros=(0, 0, 1))[0]
        out.append(rec)
        size += len(rec)
    last = pmc.random_records(rng, rows, cols, 1, zeros=(0,))[0]
    if length - size < len(last):
        last = pmc.record(0, 0, b"9,9")  # five bytes
    data = b"".join(out) + b"0" * (length - size - len(last)) + last
    assert len(data) == length
    return data


# ---- the parse -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (2, 1), (1, 64), (64, 1), (12, 103), (101, 11), (2, 1002)])
def test_shapes_and_digit_counts(rt, orc, shape):
    rows, cols = shape
    rng = np.random.default_rng(rows * 1000 + cols)
    img = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    data = orc.format_pixel_map(img)  # the writer's own bytes: every pixel, zero as no digits
    _assert_parse(orc, _parse(rt, data, rows, cols), data, rows, cols)
    recs = pmc.random_records(random.Random(rows + cols), rows, cols, min(rows * cols, 40), zeros=pmc.LEADING_ZEROS)
    _assert_parse(orc, _parse(rt, b"".join(recs), rows, cols), b"".join(recs), rows, cols)


def test_the_record_cases(rt, orc):
    for name, rows, cols, data in pmc.small_files() + pmc.long_files():
        _assert_parse(orc, _parse(rt, data, rows, cols), data, rows, cols, what=name)


def test_file_sizes_at_the_chunk_and_the_tile(rt, orc):
    chunk, tile = rt.lib.rt_pixel_map_chunk_bytes(), rt.lib.rt_pixel_map_tile_bytes()
    for length in (5, chunk - 1, chunk, chunk + 1, tile - 1, tile, tile + 1, 2 * tile, 3 * tile + 7):
        data = _file_of_length(length, 33, 49, length)
        _assert_parse(orc, _parse(rt, data, 33, 49), data, 33, 49, what=length)
    _assert_parse(orc, _parse(rt, b"", 3, 4), b"", 3, 4, what="empty")  # clears present, counts 0


def test_more_tiles_than_the_scanning_workgroup_has_threads(rt, orc):
    rows, cols = 600, 700
    img = np.random.default_rng(5).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    data = orc.format_pixel_map(img)[:-2]  # and a torn tail: the last record is incomplete
    assert len(data) > rt.lib.rt_pixel_map_scan_tiles() * rt.lib.rt_pixel_map_tile_bytes()
    result = _parse(rt, data, rows, cols)
    assert result[1] == rows * cols - 1
    _assert_parse(orc, result, data, rows, cols)


def test_every_truncation_of_a_three_record_file(rt, orc):
    data = pmc.record(1, 2, b"7,8") + pmc.record(0, 0, b"\n\n\n", zeros=(0, 1)) + pmc.record(2, 10, b"123", terms=(b"A", b"\xff"))
    for cut in range(len(data) + 1):
        _assert_parse(orc, _parse(rt, data[:cut], 3, 11), data[:cut], 3, 11, what=cut)


def test_a_300_zero_run_across_a_tile_boundary(rt, orc):
    tile = rt.lib.rt_pixel_map_tile_bytes()
    for lead in (tile - 150, tile - 1, tile - 299, 2 * tile - 10):
        head = _file_of_length(lead, 9, 9, lead)
        data = head + pmc.record(4, 5, b"0,0", zeros=(300, 300)) + pmc.record(8, 8, b"abc")
        assert len(head) < tile * ((lead // tile) + 1) < len(head) + 300
        _assert_parse(orc, _parse(rt, data, 9, 9), data, 9, 9, what=lead)


def test_colour_bytes_that_look_like_syntax(rt, orc):
    data = pmc.record(0, 1, b"7,8") + pmc.record(1, 0, b",\n0") + pmc.record(1, 1, b"000") + pmc.record(0, 0, b"\n\n\n")
    result = _parse(rt, data, 2, 2)
    _assert_parse(orc, result, data, 2, 2)
    assert result[3][GUARD + 3:GUARD + 6].tobytes() == b"7,8" and result[1] == 4


def test_of_duplicates_the_later_record_wins(rt, orc):
    rng = random.Random(3)
    recs = pmc.random_records(rng, 20, 30, 400)
    later = [pmc.other_colour(r) for r in recs]
    data = b"".join(recs + later[::-1])  # every pixel twice, the copies thousands of bytes (and many workgroups) apart
    result = _parse(rt, data, 20, 30)
    _assert_parse(orc, result, data, 20, 30)
    n, rgb_first, _ = pmc.expected(orc, b"".join(recs), 20, 30)
    got = result[3][GUARD:GUARD + 1800].reshape(20, 30, 3)
    named = pmc.expected(orc, data, 20, 30)[2]
    assert result[1] == 800 and (got[named] != rgb_first[named]).any(axis=1).all()  # no pixel kept its earlier record
    data = b"".join(r for pair in zip(recs, later) for r in pair)  # and side by side, inside one chunk or two
    _assert_parse(orc, _parse(rt, data, 20, 30), data, 20, 30)


@pytest.mark.parametrize("want_count", [True, False])
def test_a_record_outside_the_image_refuses_the_whole_map(rt, orc, want_count):
    for name, rows, cols, data, good, bad, at in pmc.malformed_files():
        assert pmc.expected(orc, data, rows, cols)[0] == -1
        _assert_untouched(_parse(rt, data, rows, cols, want_count=want_count), rt, want_count)
    name, rows, cols, data, good, bad, at = pmc.malformed_files()[-1]  # the bad record last -- and incomplete: a torn tail, accepted
    assert at == len(good)
    for cut in (1, 2, 3):
        _assert_parse(orc, _parse(rt, data[:-cut], rows, cols, want_count=want_count), data[:-cut], rows, cols, what=cut)


def test_a_run_of_eleven_nines_is_malformed(rt):
    for name, rows, cols, data, good, bad, at in pmc.overflow_files():
        _assert_untouched(_parse(rt, data, rows, cols), rt)
    _assert_untouched(_parse(rt, b"0" * 5000 + b"4294967296,\nabc", 2, 2), rt)  # 2^32: no wrap back into the image


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_any_alignment_of_the_data_and_the_outputs(rt, orc, offset):
    tile = rt.lib.rt_pixel_map_tile_bytes()
    for length in (7, tile + 5, 2 * tile + 1):
        data = _file_of_length(length, 33, 49, length + offset)
        _assert_parse(orc, _parse(rt, data, 33, 49, offset=offset), data, 33, 49, offset=offset, what=(offset, length))


def test_two_streams_in_flight(rt, orc):
    torch = _torch()
    files = [(_file_of_length(20000 + 13 * i, 33, 49, i), 33, 49) for i in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    pending = []
    for _ in range(3):
        for (data, rows, cols), st in zip(files, streams):
            with torch.cuda.stream(st):
                pending.append((data, rows, cols, _parse(rt, data, rows, cols, want_count=False, stream=st, sync=False)))
    torch.cuda.synchronize()
    for data, rows, cols, (rc, _, d_count, rgb, present, _src) in pending:
        _assert_parse(orc, (rc, None, int(d_count.item()), rgb.cpu().numpy(), present.cpu().numpy()), data, rows, cols)


# ---- the missing pixels and the scatter ---------------------------------------------------------------------------------------------------
def _presence_maps():
    rng = np.random.default_rng(8)
    rows, cols = 67, 131  # 8777 pixels: three tiles, the last one ragged
    n = rows * cols
    maps = {"none": np.ones(n, np.uint8), "all": np.zeros(n, np.uint8), "every-second": (np.arange(n) % 2).astype(np.uint8),
            "first": np.ones(n, np.uint8), "last": np.ones(n, np.uint8), "random": (rng.random(n) < 0.7).astype(np.uint8) * 3}
    maps["first"][0] = 0
    maps["last"][-1] = 0
    return rows, cols, maps


def _missing(rt, present, rows, cols, capacity, *, offset=0, want_n=True, pixels=True):
    torch = _torch()
    src = _guarded(torch, present.size, offset=offset)
    src[GUARD + offset:GUARD + offset + present.size] = torch.from_numpy(present).cuda()
    out = _guarded(torch, capacity, fill=-7, dtype=torch.int32)
    d_n = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    n = C.c_int64(-7)
    rc = rt.lib.rt_missing_pixels_device(0, src.data_ptr() + GUARD + offset, rows, cols, out.data_ptr() + 4 * GUARD if pixels else None, capacity, d_n.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream, C.byref(n) if want_n else None)
    torch.cuda.synchronize()
    return rc, n.value, int(d_n.item()), out.cpu().numpy()


@pytest.mark.parametrize("name", ["none", "all", "every-second", "first", "last", "random"])
def test_missing_pixels_is_numpys_answer(rt, name):
    rows, cols, maps = _presence_maps()
    present = maps[name]
    want = np.flatnonzero(present == 0).astype(np.int32)
    for offset in (0, 1):
        rc, n, d_n, out = _missing(rt, present, rows, cols, present.size, offset=offset)
        assert rc == 0 and n == d_n == want.size
        assert np.array_equal(out[GUARD:GUARD + want.size], want) and (out[:GUARD] == -7).all() and (out[GUARD + want.size:] == -7).all()
    rc, n, d_n, out = _missing(rt, present, rows, cols, 0, pixels=False)  # the length only
    assert rc == 0 and n == d_n == want.size and (out == -7).all()


def test_missing_pixels_capacity_rule(rt):
    rows, cols, maps = _presence_maps()
    present = maps["random"]
    want = np.flatnonzero(present == 0).astype(np.int32)
    rc, n, d_n, out = _missing(rt, present, rows, cols, want.size)  # exactly enough
    assert rc == 0 and np.array_equal(out[GUARD:GUARD + want.size], want) and (out[GUARD + want.size:] == -7).all()
    rc, n, d_n, out = _missing(rt, present, rows, cols, want.size - 1)  # one short: found on the device, nothing written, the length reported
    assert rc == rt._abi.RT_ERR_INVALID_ARGUMENT and n == d_n == want.size and (out == -7).all()
    rc, n, d_n, out = _missing(rt, present, rows, cols, want.size - 1, want_n=False)
    assert rc == 0 and d_n == want.size and (out == -7).all()


def _scatter(rt, pixels, lst, rows, cols):
    torch = _torch()
    frame = _guarded(torch, rows * cols * 3, offset=1)
    px = torch.from_numpy(np.ascontiguousarray(pixels, np.int32)).cuda()
    src = _guarded(torch, lst.size, fill=0, offset=3)
    src[GUARD + 3:GUARD + 3 + lst.size] = torch.from_numpy(lst.reshape(-1)).cuda()
    rc = rt.lib.rt_scatter_pixels_device(0, len(pixels), px.data_ptr(), src.data_ptr() + GUARD + 3, rows, cols, frame.data_ptr() + GUARD + 1,
                                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = frame.cpu().numpy()
    assert (got[:GUARD + 1] == S).all() and (got[GUARD + 1 + rows * cols * 3:] == S).all()
    return rc, got[GUARD + 1:GUARD + 1 + rows * cols * 3].reshape(-1, 3)


def test_scatter_pixels_is_numpys_answer(rt):
    rows, cols, maps = _presence_maps()
    rng = np.random.default_rng(9)
    for name in ("all", "every-second", "first", "last", "random"):
        pixels = rng.permutation(np.flatnonzero(maps[name] == 0)).astype(np.int32)
        lst = rng.integers(0, 256, (pixels.size, 3), dtype=np.uint8)
        rc, got = _scatter(rt, pixels, lst, rows, cols)
        want = np.full((rows * cols, 3), S, np.uint8)
        want[pixels] = lst
        assert rc == 0 and np.array_equal(got, want), name
    pixels = np.array([5, 9, 5, 5, 9, 0], np.int32)  # duplicates: the last in list order wins
    lst = (np.arange(18, dtype=np.uint8) + 1).reshape(6, 3)
    rc, got = _scatter(rt, pixels, lst, rows, cols)
    assert rc == 0 and got[5].tolist() == [10, 11, 12] and got[9].tolist() == [13, 14, 15] and got[0].tolist() == [16, 17, 18]
    assert (np.delete(got, [0, 5, 9], axis=0) == S).all()


def test_a_malformed_list_scatters_nothing(rt):
    rows, cols, _ = _presence_maps()
    lst = np.full((4, 3), 9, np.uint8)
    for bad in (rows * cols, -1, 2**31 - 1):
        for at in (0, 2, 3):
            pixels = np.array([1, 2, 3, 4], np.int32)
            pixels[at] = bad
            rc, got = _scatter(rt, pixels, lst, rows, cols)
            assert rc == 0 and (got == S).all()


# ---- resume ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _frame(rt, name):
    """(scene, camera, w, h, rt_render's rgb [rows, cols, 3], the frame's records in the writer's order): rendered once, shared, never changed."""
    import oracle as orc
    objs, cam, w, h = {"small_final": scenes.small_final, "all_materials": scenes.all_materials}[name]()
    scene = rt.Scene.make(objs)
    rgb = scene.render_rows(w, h, cam, seed=SEED, device=0).rgb
    rgb.setflags(write=False)
    return scene, cam, w, h, rgb, tuple(pmc.map_of(orc, rgb))


def _partial_maps(recs):
    """(name, bytes, pixels named): whole, empty, cut in half (mid-record), every third record dropped, shuffled with duplicates."""
    n = len(recs)
    whole = b"".join(recs)
    half = whole[:len(whole) // 2]
    done, size = 0, 0
    while size + len(recs[done]) <= len(half):
        size += len(recs[done])
        done += 1
    rng = random.Random(4)
    some = rng.sample(range(n), n // 2)
    shuffled = some + rng.sample(some, 100)
    return [("whole", whole, n), ("empty", b"", 0), ("half", half, done), ("dropped", b"".join(r for i, r in enumerate(recs) if i % 3 != 2), n - n // 3),
            ("shuffled", b"".join(recs[i] for i in shuffled), len(some))]


@pytest.mark.parametrize("name", ["small_final", "all_materials"])
def test_resume_is_the_uninterrupted_frame(rt, name):
    scene, cam, w, h, rgb, recs = _frame(rt, name)
    for what, data, named in _partial_maps(recs):
        got = scene.resume(w, h, cam, data, seed=SEED)
        assert np.array_equal(got, rgb), what
        assert scene.last_stats["pixels"] == len(recs) - named, what
        if what == "whole":
            assert scene.last_stats["samples"] == 0 and scene.last_stats["kernel_ms"] == 0.0 and scene.last_stats["total_ms"] > 0.0


@pytest.mark.parametrize("variant", ["tuned", "reference"])
def test_resume_after_tuning_and_on_the_reference_tree(rt, variant):
    _, cam, w, h, rgb, recs = _frame(rt, "small_final")
    scene = rt.Scene.make(scenes.small_final()[0], walk_tree="reference" if variant == "reference" else None)
    if variant == "tuned":
        assert scene.tune(w, h, cam, seed=SEED, device=0)["tuned"] == 1
    for what, data, named in _partial_maps(recs)[2:4]:
        assert np.array_equal(scene.resume(w, h, cam, data, seed=SEED, counters=(what == "half")), rgb), what
        assert scene.last_stats["pixels"] == len(recs) - named


def test_a_map_from_another_seed_keeps_its_named_pixels(rt, orc):
    scene, cam, w, h, rgb, recs = _frame(rt, "all_materials")
    other = scene.render_rows(w, h, cam, seed=SEED + 1, device=0).rgb
    assert (other != rgb).any()
    keep = list(range(0, len(recs), 2))
    got = scene.resume(w, h, cam, b"".join(pmc.map_of(orc, other, keep)), seed=SEED)
    named = np.zeros(len(recs), bool)
    named[keep] = True
    want = np.where(named.reshape(rgb.shape[0], rgb.shape[1], 1), other, rgb)
    assert np.array_equal(got, want) and scene.last_stats["pixels"] == len(recs) - len(keep)


def test_a_malformed_map_is_refused_before_anything_is_rendered(rt):
    scene, cam, w, h, rgb, recs = _frame(rt, "small_final")
    data = b"".join(recs[:50]) + pmc.record(rgb.shape[0], 0, b"abc") + b"".join(recs[50:60])
    out = np.full(rgb.shape, S, np.uint8)
    st = rt._abi.rt_stats()
    C.memset(C.byref(st), 0x55, C.sizeof(st))
    cam_abi = cam.to_abi()
    rc = rt.lib.rt_resume_pixel_map(scene.handle, C.byref(cam_abi), w, h, SEED, 0, 0, data, len(data), out.ctypes.data_as(C.POINTER(C.c_uint8)), None, C.byref(st))
    assert rc == rt._abi.RT_ERR_INVALID_ARGUMENT and "outside the image" in rt.lib.rt_last_error().decode()
    assert (out == S).all() and bytes(st)[:8] == b"\x55" * 8


@pytest.mark.parametrize("gamma", [False, True])
def test_resume_png_and_ppm_are_the_frames_files(rt, tmp_path, gamma):
    scene, cam, w, h, rgb, recs = _frame(rt, "small_final")
    spill = tmp_path / "spill.bin"
    spill.write_bytes(_partial_maps(recs)[2][1])
    st = scene.resumePng(w, h, cam, str(spill), str(tmp_path / "out.png"), gammaCorrect=gamma, seed=SEED)
    assert (tmp_path / "out.png").read_bytes() == rt.Png.format(gamma, np.asarray(rgb))
    assert st["pixels"] == len(recs) - _partial_maps(recs)[2][2]
    scene.resumePpm(w, h, cam, str(spill), str(tmp_path / "out.ppm"), gammaCorrect=gamma, seed=SEED)
    assert (tmp_path / "out.ppm").read_bytes() == rt.ImageOutput.formatPpm(gamma, np.asarray(rgb))
    scene.resumePpm(w, h, cam, str(spill), str(spill), gammaCorrect=gamma, seed=SEED)  # the two paths may name one file
    assert spill.read_bytes() == rt.ImageOutput.formatPpm(gamma, np.asarray(rgb))


# ---- the Python tensor routes ------------------------------------------------------------------------------------------------------------
def test_python_tensor_routes(rt, orc):
    torch = _torch()
    scene, cam, w, h, rgb, recs = _frame(rt, "small_final")
    rows, cols = rgb.shape[0], rgb.shape[1]
    what, data, named = _partial_maps(recs)[3]
    t = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    pixels, present = rt.ImageOutput.parsePixelMap(t, rows, cols)
    n, orgb, opresent = pmc.expected(orc, data, rows, cols)
    assert pixels.is_cuda and present.dtype == torch.bool and np.array_equal(pixels.cpu().numpy(), orgb) and np.array_equal(present.cpu().numpy(), opresent)
    missing = rt.ImageOutput.missingPixels(present)
    assert missing.dtype == torch.int32 and np.array_equal(missing.cpu().numpy(), np.flatnonzero(~opresent.reshape(-1)))
    res = scene.renderPixels(w, h, cam, missing, seed=SEED)
    flat = pixels.reshape(-1, 3)
    assert rt.lib.rt_scatter_pixels_device(0, missing.numel(), missing.data_ptr(), res.rgb.data_ptr(), rows, cols, flat.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream) == 0
    assert np.array_equal(pixels.cpu().numpy(), rgb)
    assert rt.ImageOutput.missingPixels(torch.ones((rows, cols), dtype=torch.uint8, device="cuda")).numel() == 0
    empty_rgb, empty_present = rt.ImageOutput.parsePixelMap(torch.empty(0, dtype=torch.uint8, device="cuda"), 2, 3)
    assert not empty_present.any() and not empty_rgb.any()
    with pytest.raises(rt.RtError):
        rt.ImageOutput.parsePixelMap(torch.from_numpy(np.frombuffer(b"2,0\nabc", np.uint8).copy()).cuda(), 2, 3)
