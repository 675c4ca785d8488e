"""Scene.renderPixels -- rt_render_pixels, rt_render_pixels_extend and their device variants, the render kernel's pixel-list modes --
against the ORACLE's whole frame (OracleScene.render_rows) gathered at the listed indices, bit for bit, never against the library's
own rt_render: scattered shuffled lists with duplicates at every sample count around the adaptive rule's edges, LDS-resident,
global-memory and textured scenes, both kernel variants, the whole frame as a list with its statistics and counters, the pixels where
pixel_candidates matters, every launch setting with the plan the library reports, list sizes around a wave, extensions and buffers
that are not what the arguments say, the device entry on streams, device lists with entries outside the frame, and the C consumer."""
import ctypes as C
import dataclasses
import functools
import subprocess

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

DEPTH = 12
SEED = 5
EARLY = 11  # Count of a pixel that stopped early, at every spp >= 10
SPPS = (1, 2, 3, 9, 10, 11, 12, 40)
SIZES = {"all_materials": (71, 41), "many_spheres": (35, 21), "earth_thumb": (65, 37), "small_final": (49, 33), "free": (49, 33)}
COUNTERS = ("rays", "aabb_tests", "prim_tests", "reflections")


@functools.lru_cache(maxsize=None)
def _frame(name):
    """(objects, camera at BounceDepth 12, max_w, max_h) at the scene's default size"""
    if name == "earth_thumb":
        objs, cam, w, h = scenes.earth_thumb(scenes.golden("earthmap_rgb")["rgb"])
    elif name == "free":  # small_final's spheres under a hand-made camera: viewport off-centre, axes 84 degrees apart
        objs, cam, w, h = scenes.small_final()
        a = cam.to_abi()
        eye, xo, xd, yd = (np.array(list(v)) for v in (a.view_origin, a.xaxis_origin, a.xaxis_dir, a.yaxis_dir))
        cam = scenes.free_camera(eye, xo + xd * (0.3 * a.viewport_width) - yd * (0.2 * a.viewport_height), xd + 0.1 * yd, yd, a.viewport_width,
                                 a.viewport_height, 40, DEPTH)
        scenes.require_clear_eye(cam, w, h)
    else:
        objs, cam, w, h = getattr(scenes, name)()
    assert (2 * w + 1, 2 * h + 1) == SIZES[name]
    return objs, dataclasses.replace(cam, BounceDepth=DEPTH), w, h


def _cam(name, spp):
    return dataclasses.replace(_frame(name)[1], SamplesPerPixel=spp)


def _n(name):
    return SIZES[name][0] * SIZES[name][1]


@functools.lru_cache(maxsize=None)
def _scene(rt, name, walk_tree=None):
    return rt.Scene.make(_frame(name)[0], walk_tree=walk_tree)


@functools.lru_cache(maxsize=None)
def _oracle_scene(orc, name):
    return orc.OracleScene(_frame(name)[0])


@functools.lru_cache(maxsize=None)
def _oracle(orc, name, spp):
    """The oracle's whole frame at spp, flat: (accum [rows*cols, 4], rgb [rows*cols, 3], stats); computed once, never written to."""
    _, _, w, h = _frame(name)
    acc, rgb, st = _oracle_scene(orc, name).render_rows(w, h, _cam(name, spp).to_abi(), seed=SEED, threads=16)
    acc, rgb = acc.reshape(-1, 4), rgb.reshape(-1, 3)
    acc.setflags(write=False); rgb.setflags(write=False)
    return acc, rgb, st


@functools.lru_cache(maxsize=None)
def _sub(name):
    """SUB: every 7th global index, the four corners and the centre, shuffled (not row-major), its first 10 entries once more."""
    cols, rows = SIZES[name]
    n = rows * cols
    idx = sorted(set(range(0, n, 7)) | {0, cols - 1, n - cols, n - 1, (rows // 2) * cols + cols // 2})
    idx = np.random.default_rng(2024).permutation(np.array(idx, np.int32))
    out = np.concatenate([idx, idx[:10]]).astype(np.int32)
    out.setflags(write=False)
    return out


def _render(rt, name, px, spp, **kw):
    _, _, w, h = _frame(name)
    return _scene(rt, name, kw.pop("walk_tree", None)).renderPixels(w, h, _cam(name, spp), px, seed=SEED, **kw)


def _assert_equals_oracle(got, orc, name, px, spp, what=()):
    want_acc, want_rgb, _ = _oracle(orc, name, spp)
    px = np.asarray(px)
    acc = got.accum if isinstance(got.accum, np.ndarray) else got.accum.cpu().numpy()
    rgb = got.rgb if isinstance(got.rgb, np.ndarray) else got.rgb.cpu().numpy()
    assert np.array_equal(acc, want_acc[px]), (name, spp) + tuple(what)
    assert np.array_equal(rgb, want_rgb[px]), (name, spp) + tuple(what)


# ---- 1 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["all_materials", "many_spheres", "earth_thumb"])
def test_equals_the_frames_pixels(rt, orc, name):
    px = _sub(name)
    assert _scene(rt, name).info()["lds_resident"] == (0 if name == "many_spheres" else 1)
    assert not np.array_equal(px[:-10], np.sort(px[:-10])) and len(px) == len(set(px.tolist())) + 10
    want = _oracle(orc, name, 40)[0][px]  # both branches of the decision, and pass B, are exercised: a condition on the EXPECTED values
    early, full = float((want[:, 0] == EARLY).mean()), float((want[:, 0] == 40).mean())
    print(f"{name}: {early:.2f} of SUB stops early, {full:.2f} runs all 40 samples, of {len(px)}")
    assert early >= 0.05 and full >= 0.05 and abs(early + full - 1.0) < 1e-12
    for spp in SPPS:
        for counters in (False, True):
            got = _render(rt, name, px, spp, counters=counters)
            _assert_equals_oracle(got, orc, name, px, spp, (counters,))
            assert np.array_equal(got.accum[-10:], got.accum[:10]) and np.array_equal(got.rgb[-10:], got.rgb[:10])  # the duplicates
            assert got.stats["pixels"] == len(px) and got.stats["samples"] == int(got.accum[:, 0].sum())


# ---- 2 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["many_spheres", "all_materials"])
def test_the_whole_frame_as_a_list(rt, orc, name):
    n, cols = _n(name), SIZES[name][0]
    _, _, w, h = _frame(name)
    want_acc, _, want_st = _oracle(orc, name, 40)
    every = np.arange(n, dtype=np.int32)
    for px in (every, every[::-1].copy()):
        for counters in (False, True):
            got = _render(rt, name, px, 40, counters=counters)
            _assert_equals_oracle(got, orc, name, px, 40, (counters,))
            st = got.stats
            assert st["samples"] == want_st["samples"] == int(want_acc[:, 0].sum()) and st["pixels"] == n
            assert st["pixels_early"] == want_st["pixels_early"] == int((want_acc[:, 0] == EARLY).sum())
            assert st["kernel_ms"] > 0.0 and st["total_ms"] >= st["kernel_ms"]
    # the counting variant over BoundingBoxTree.make's own tree: the frame's four counters, in any order
    frame = _render(rt, name, every[::-1].copy(), 40, counters=True, walk_tree="reference").stats
    for key in COUNTERS:
        assert frame[key] == want_st[key] > 0, (name, key)
    # one full image row given as a list: the oracle's statistics of that row
    r = 2 * h - 6
    _, _, row_st = _oracle_scene(orc, name).render_rows(w, h, _cam(name, 40).to_abi(), seed=SEED, row_first=r, n_rows=1, threads=16)
    got = _render(rt, name, np.arange(r * cols, (r + 1) * cols, dtype=np.int32), 40, counters=True, walk_tree="reference")
    for key in COUNTERS + ("samples", "pixels_early"):
        assert got.stats[key] == row_st[key], (name, key)
    # SUB (each entry once) and its complement: their counters add up to the frame's
    sub = _sub(name)[:-10]
    rest = np.setdiff1d(every, sub).astype(np.int32)
    a = _render(rt, name, sub, 40, counters=True, walk_tree="reference")
    b = _render(rt, name, rest, 40, counters=True, walk_tree="reference")
    _assert_equals_oracle(a, orc, name, sub, 40)
    _assert_equals_oracle(b, orc, name, rest, 40)
    assert len(sub) + len(rest) == n
    for key in COUNTERS + ("samples", "pixels_early"):
        assert a.stats[key] + b.stats[key] == want_st[key], (name, key)


# ---- 3 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small_final", "free"])
def test_edges_where_pixel_candidates_matter(rt, orc, name):
    cols, rows = SIZES[name]
    _, _, w, h = _frame(name)
    r, c = np.divmod(np.arange(rows * cols), cols)
    # the border, and the two rows (h - r - 1 in {0, -1}) and two columns (c - w in {-1, 0}) that straddle the viewport's axes
    keep = (r == 0) | (r == rows - 1) | (c == 0) | (c == cols - 1) | (r == h - 1) | (r == h) | (c == w - 1) | (c == w)
    px = np.flatnonzero(keep).astype(np.int32)
    assert len(px) == 2 * cols + 2 * (rows - 2) + 2 * (cols - 2) + 2 * (rows - 4)
    want = _oracle(orc, name, 40)[0][px]
    assert len(np.unique(want, axis=0)) > 20
    timed, counting = _render(rt, name, px, 40), _render(rt, name, px, 40, counters=True)
    assert np.array_equal(timed.accum, counting.accum) and np.array_equal(timed.rgb, counting.rgb)
    _assert_equals_oracle(timed, orc, name, px, 40)
    _assert_equals_oracle(counting, orc, name, px, 40)


# ---- 4 -----------------------------------------------------------------------------------------------------------------------
def _tiled(name, tile=8):
    cols, rows = SIZES[name]
    out = [r * cols + c for r0 in range(0, rows, tile) for c0 in range(0, cols, tile)
           for r in range(r0, min(r0 + tile, rows)) for c in range(c0, min(c0 + tile, cols))]
    assert sorted(out) == list(range(rows * cols))
    return np.array(out, np.int32)


SETTINGS = (dict(passes=1), dict(passes=2), dict(block_threads=256), dict(block_threads=1024), dict(chunk_pixels=1), dict(chunk_pixels=16),
            dict(chunk_pixels=64), dict(park_lanes=-1), dict(passes=2, block_threads=256, chunk_pixels=64))


def test_launch_settings_do_not_change_results(rt, orc):
    torch = pytest.importorskip("torch")
    A = rt._abi
    name = "all_materials"
    px = _tiled(name)[:2048]  # two passes have a list to order
    assert _n(name) == 2911 and len(px) == 2048
    want = _oracle(orc, name, 40)[0][px]
    assert 0 < int((want[:, 0] == 40).sum()) < 2048
    d_px = torch.from_numpy(px).cuda()
    for opt in SETTINGS:
        for counters in (False, True):
            got = _render(rt, name, d_px, 40, counters=counters, options=A.rt_render_options(**opt))
            _assert_equals_oracle(got, orc, name, px, 40, (opt, counters))
            plan = rt.hooks.last_launch_plan()
            i, o = plan["in"], plan["out"]
            assert i["kind"] == 4 and i["n"] == 2048 and i["spp"] == 40 and i["first_sample"] == 0 and i["map"] == 0
            if "passes" in opt:
                assert i["s_passes"] == opt["passes"]
            two = i["s_passes"] == 2  # (2048 pixels with 29 samples in phase 2: fused unless two passes are asked for)
            assert o["two_pass"] == (1 if two else 0) and o["error"] == 0 and o["q_mode"] == 11
            if two:
                assert (o["A_mode"], o["B_mode"]) == (12, 13) and o["A_grid"] > 0 and o["B_grid"] > 0 and o["list"] >= 4 * 2048
            else:
                assert o["F_mode"] == 11 and o["F_grid"] > 0
            if "block_threads" in opt:
                assert o["q_block"] == opt["block_threads"]
            if "chunk_pixels" in opt:
                assert (o["A_chunk"] if two else o["F_chunk"]) == opt["chunk_pixels"]
            assert got.stats["pixels"] == 2048 and got.stats["samples"] == int(want[:, 0].sum())
    # a block of 512 or 768 threads runs as 1024
    for block in (512, 768):
        got = _render(rt, name, d_px, 40, options=A.rt_render_options(block_threads=block))
        _assert_equals_oracle(got, orc, name, px, 40, (block,))
        assert rt.hooks.last_launch_plan()["out"]["q_block"] == 1024


# ---- 5 -----------------------------------------------------------------------------------------------------------------------
def test_sizes_around_a_wave(rt, orc):
    for name in ("all_materials", "many_spheres"):
        for n in (1, 63, 64, 65):
            px = _sub(name)[:n]
            for counters in (False, True):
                got = _render(rt, name, px, 12, counters=counters)
                _assert_equals_oracle(got, orc, name, px, 12, (n, counters))
                assert got.stats["pixels"] == n


# ---- 6 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["all_materials", "many_spheres", "earth_thumb"])
def test_extension_equals_the_oracle_at_the_target(rt, orc, name):
    px = _sub(name)
    for a in (12, 13, 40):
        bases = {c: _render(rt, name, px, a, counters=c) for c in (False, True)}
        for b in (a, a + 1, 64):
            want_acc = _oracle(orc, name, b)[0][px]
            direct = _render(rt, name, px, b, counters=True)  # (itself held to the oracle: its counters are what the two halves must add up to)
            _assert_equals_oracle(direct, orc, name, px, b)
            for counters in (False, True):
                base = bases[counters]
                got = _render(rt, name, px, b, counters=counters, extend=(base.accum, a))
                assert np.array_equal(got.accum, want_acc), (name, a, b, counters)
                if b == a:  # nothing to add: a no-op by contract (zeroed stats, rgb not written); the buffer IS the render at b
                    assert got.stats["pixels"] == 0 and got.stats["samples"] == 0
                    continue
                _assert_equals_oracle(got, orc, name, px, b, (a, counters))
                st = got.stats
                assert st["pixels"] == len(px) and st["pixels_early"] == int((want_acc[:, 0] == EARLY).sum())
                assert st["samples"] == int(want_acc[:, 0].sum()) - int(base.accum[:, 0].sum()) == (b - a) * int((want_acc[:, 0] == b).sum())
                for key in COUNTERS:
                    if counters:
                        assert base.stats[key] + st[key] == direct.stats[key] and st["rays"] > 0, (name, a, b, key)
                    else:
                        assert st[key] == 0


def _raw_extend(rt, name, px, accum, rgb, done, to):
    _, _, w, h = _frame(name)
    cam = _cam(name, to).to_abi()
    return rt.lib.rt_render_pixels_extend(_scene(rt, name).handle, C.byref(cam), w, h, SEED, 0, len(px), px.ctypes.data_as(C.POINTER(C.c_int32)), 0, done,
                                          accum.ctypes.data_as(C.POINTER(C.c_int32)), rgb.ctypes.data_as(C.POINTER(C.c_uint8)), None)


def test_a_malformed_buffer_is_refused_and_left_unchanged(rt, orc):
    torch = pytest.importorskip("torch")
    A = rt._abi
    name = "all_materials"
    _, _, w, h = _frame(name)
    px = np.array(_sub(name))
    good = np.array(_render(rt, name, px, 12).accum)
    assert np.array_equal(good, _oracle(orc, name, 12)[0][px])
    cont, final = np.flatnonzero(good[:, 0] == 12), np.flatnonzero(good[:, 0] == EARLY)
    cases = [(int(cont[len(cont) // 2]), 10, 12), (int(final[-1]), 10, 12), (int(cont[0]), 12, 13), (int(cont[0]), 12, 14)]  # (entry, its Count, samples_done)
    for entry, count, done in cases:
        bad = good.copy()
        bad[entry, 0] = count
        accum, rgb = bad.copy(), np.full((len(px), 3), 0xA5, np.uint8)
        assert _raw_extend(rt, name, px, accum, rgb, done, 40) == A.RT_ERR_INVALID_ARGUMENT and rt.lib.rt_last_error()
        assert np.array_equal(accum, bad) and (rgb == 0xA5).all()
        with pytest.raises(rt.RtError) as e:
            _render(rt, name, px, 40, extend=(bad, done))
        assert e.value.code == A.RT_ERR_INVALID_ARGUMENT
        # the device variant: with stats it reports the buffer, without it cannot -- either way nothing is written
        for stats in (True, False):
            d_px, d_acc = torch.from_numpy(px).cuda(), torch.from_numpy(bad).cuda()
            d_rgb = torch.full((len(px), 3), 0xA5, dtype=torch.uint8, device="cuda")
            cam, st = _cam(name, 40).to_abi(), A.rt_stats()
            rc = rt.lib.rt_render_pixels_extend_device(_scene(rt, name).handle, C.byref(cam), w, h, SEED, 0, len(px), d_px.data_ptr(), 0, done, d_acc.data_ptr(),
                                                       d_rgb.data_ptr(), torch.cuda.current_stream().cuda_stream, None, C.byref(st) if stats else None)
            torch.cuda.synchronize()
            assert rc == (A.RT_ERR_INVALID_ARGUMENT if stats else A.RT_OK)
            assert np.array_equal(d_acc.cpu().numpy(), bad) and bool((d_rgb == 0xA5).all())
    # the right arguments still work afterwards
    accum, rgb = good.copy(), np.full((len(px), 3), 0xA5, np.uint8)
    assert _raw_extend(rt, name, px, accum, rgb, 12, 40) == A.RT_OK
    assert np.array_equal(accum, _oracle(orc, name, 40)[0][px]) and np.array_equal(rgb, _oracle(orc, name, 40)[1][px])


# ---- 7 -----------------------------------------------------------------------------------------------------------------------
def test_device_entry_on_streams(rt, orc):
    torch = pytest.importorskip("torch")
    name = "all_materials"
    lists = [np.array(_sub(name)), _tiled(name)[100:1500], np.array(_sub(name)[::-1]), _tiled(name)[::3].copy()]
    prev = torch.cuda.current_device()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = []
    for k, px in enumerate(lists):  # four launches in flight on two streams
        with torch.cuda.stream(streams[k % 2]):
            t = torch.from_numpy(px).to("cuda", non_blocking=False)
            got.append((t, _render(rt, name, t, 40, stats=False)))
            assert _scene(rt, name).last_stats is None and got[-1][1].stats is None
    torch.cuda.synchronize()
    assert torch.cuda.current_device() == prev
    for px, (_, g) in zip(lists, got):
        assert g.accum.dtype == torch.int32 and g.rgb.dtype == torch.uint8 and g.accum.is_cuda and tuple(g.accum.shape) == (len(px), 4)
        _assert_equals_oracle(g, orc, name, px, 40)
    # an extension in place on a stream, with statistics
    with torch.cuda.stream(streams[1]):
        t = torch.from_numpy(lists[1]).cuda()
        base = _render(rt, name, t, 12).accum
        g = _render(rt, name, t, 40, extend=(base, 12))
    assert g.accum is base and g.stats["kernel_ms"] > 0.0 and g.stats["pixels"] == len(lists[1])
    _assert_equals_oracle(g, orc, name, lists[1], 40)
    assert rt.hooks.last_launch_plan()["in"]["kind"] == 4 and rt.hooks.last_launch_plan()["in"]["first_sample"] == 12
    assert rt.hooks.last_launch_plan()["out"]["B_mode"] == 13
    assert torch.cuda.current_device() == prev


@pytest.mark.parametrize("name", ["all_materials", "many_spheres"])
def test_a_device_list_with_entries_outside_the_frame_renders_nothing(rt, orc, name):
    torch = pytest.importorskip("torch")
    A = rt._abi
    _, _, w, h = _frame(name)
    good = np.array(_sub(name))
    n = len(good)
    bad = good.copy()
    bad[3], bad[n // 2] = -1, _n(name)
    base = np.array(_render(rt, name, good, 12).accum)  # what an extension would continue
    S = _scene(rt, name).handle
    for opt in (None, A.rt_render_options(passes=2), A.rt_render_options(passes=1, chunk_pixels=1)):
        for flags in (0, A.RT_RENDER_COUNTERS):
            for stats in (True, False):
                for extend in (False, True):
                    d_px = torch.from_numpy(bad).cuda()
                    before = base if extend else np.full((n, 4), 0x5A5A5A5A, np.int32)
                    d_acc = torch.from_numpy(before).cuda()
                    d_rgb = torch.full((n, 3), 0xA5, dtype=torch.uint8, device="cuda")
                    cam, st = _cam(name, 40).to_abi(), A.rt_stats()
                    stream = torch.cuda.current_stream().cuda_stream
                    if extend:
                        rc = rt.lib.rt_render_pixels_extend_device(S, C.byref(cam), w, h, SEED, 0, n, d_px.data_ptr(), flags, 12, d_acc.data_ptr(), d_rgb.data_ptr(),
                                                                   stream, C.byref(opt) if opt is not None else None, C.byref(st) if stats else None)
                    else:
                        rc = rt.lib.rt_render_pixels_device(S, C.byref(cam), w, h, SEED, 0, n, d_px.data_ptr(), flags, d_acc.data_ptr(), d_rgb.data_ptr(), stream,
                                                            C.byref(opt) if opt is not None else None, C.byref(st) if stats else None)
                    torch.cuda.synchronize()
                    assert rc == (A.RT_ERR_INVALID_ARGUMENT if stats else A.RT_OK), (flags, stats, extend)
                    if stats:
                        assert b"outside the frame" in rt.lib.rt_last_error()
                    assert np.array_equal(d_acc.cpu().numpy(), before) and bool((d_rgb == 0xA5).all()), (flags, stats, extend)
    # the wrapper raises; the valid list still renders afterwards
    with pytest.raises(rt.RtError) as e:
        _render(rt, name, torch.from_numpy(bad).cuda(), 40)
    assert e.value.code == A.RT_ERR_INVALID_ARGUMENT
    _assert_equals_oracle(_render(rt, name, torch.from_numpy(good).cuda(), 40), orc, name, good, 40)


# ---- 8 -----------------------------------------------------------------------------------------------------------------------
def test_c_program_renders_a_list(rt, orc, tmp_path):
    from test_gpu_ray_queries import _smoke_scene
    from test_pixels_host import build_pixels_smoke
    out = subprocess.run([build_pixels_smoke(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pixels: argument checks ok" in out.stdout and "pixels: rendered 10 list entries on the GPU" in out.stdout
    rows = np.array([[int(x) for x in ln.split()[2:]] for ln in out.stdout.splitlines() if ln.startswith("pixel ")])
    assert rows.shape == (10, 8)
    max_w, max_h = 12, 7  # pixels_smoke.c's frame and camera
    cam = rt.Camera.makeBasic(24, 1.0, 25.0 / 15.0, rt.Point.make(0.0, 0.5, -2.0), rt.Vector.unitise(rt.Vector.make(0.0, 0.0, 1.0)), rt.Vector.make(0.0, 1.0, 0.0))
    cam = dataclasses.replace(cam, BounceDepth=10)
    acc, rgb, _ = orc.OracleScene(_smoke_scene(rt)).render_rows(max_w, max_h, cam.to_abi(), seed=5, threads=4)
    px = rows[:, 0]
    assert px[9] == px[2] and px[0] == 25 * 15 - 1 and px[1] == 0
    assert np.array_equal(rows[:, 1:5], acc.reshape(-1, 4)[px]) and np.array_equal(rows[:, 5:], rgb.reshape(-1, 3)[px])
