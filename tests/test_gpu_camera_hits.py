"""Scene.cameraHits -- rt_camera_hits, rt_camera_hits_device, the render kernel's mode 14 -- against the answer composed from the
oracle's pieces (tests/camera_hit_cases.py; itself held to the oracle's traceOnce and to the literal restatement by
test_camera_hits_host.py), bit for bit in hit_index, strike and rays_out, NaNs by position; never against the library's own
rt_hit_objects.  Both kernel variants, LDS-resident and global-memory scenes, the pixels where the candidates matter, sample ranges,
lists in any order with duplicates, sizes around a wave, every launch setting, NULL outputs, the counters, the device entry on
streams, device lists with entries outside the frame, a camera whose every ray fails Ray.make', and the C consumer."""
import ctypes as C
import dataclasses
import functools
import subprocess

import numpy as np
import pytest

import camera_hit_cases as cases
import scenes

pytestmark = pytest.mark.gpu

DEPTH = 12
SEED = 5
SIZES = {"all_materials": (71, 41), "many_spheres": (35, 21), "small_final": (49, 33), "free": (49, 33), "lights": (35, 21)}
SENTINEL_I, SENTINEL_F = 0x5A5A5A5A, 7.5


@functools.lru_cache(maxsize=None)
def _frame(name):
    """(objects, camera at BounceDepth 12, max_w, max_h): tests/test_gpu_pixels.py's scenes and sizes"""
    if name == "free":  # small_final's spheres under a hand-made camera: viewport off-centre, axes 84 degrees apart
        objs, cam, w, h = scenes.small_final()
        a = cam.to_abi()
        eye, xo, xd, yd = (np.array(list(v)) for v in (a.view_origin, a.xaxis_origin, a.xaxis_dir, a.yaxis_dir))
        cam = scenes.free_camera(eye, xo + xd * (0.3 * a.viewport_width) - yd * (0.2 * a.viewport_height), xd + 0.1 * yd, yd, a.viewport_width,
                                 a.viewport_height, 40, DEPTH)
        scenes.require_clear_eye(cam, w, h)
    elif name == "lights":  # test_camera_hits_host.py's light sources with sky between them: rays that hit nothing
        import ray_tracing_fsharp_amd as rt
        from test_camera_hits_host import _basic_camera, _lights
        objs, cam, w, h = _lights(rt)[0], _basic_camera(rt, 1, 35.0 / 21.0), 17, 10
    else:
        objs, cam, w, h = getattr(scenes, name)()
    assert (2 * w + 1, 2 * h + 1) == SIZES[name]
    return objs, dataclasses.replace(cam, BounceDepth=DEPTH), w, h


def _n(name):
    return SIZES[name][0] * SIZES[name][1]


@functools.lru_cache(maxsize=None)
def _scene(rt, name, walk_tree=None):
    return rt.Scene.make(_frame(name)[0], walk_tree=walk_tree)


@functools.lru_cache(maxsize=None)
def _oracle_scene(orc, name):
    return orc.OracleScene(_frame(name)[0])


_SLOTS = {}  # (name, g, s) -> (hit, strike [3], ray [6], counters [2]): every slot is composed once and never written to


def _expected(orc, name, px, first, per, cam=None) -> cases.Expected:
    """The composer's answer for the list px and samples first .. first + per - 1 (cam: another camera, not cached)."""
    _, fcam, w, h = _frame(name)
    px = np.asarray(px, np.int64)
    if cam is not None:
        return cases.compose(orc, _oracle_scene(orc, name), cam.to_abi(), w, h, SEED, px, first, per)
    for s in range(first, first + per):
        todo = sorted({int(g) for g in px if (name, int(g), s) not in _SLOTS})
        if todo:
            e = cases.compose(orc, _oracle_scene(orc, name), fcam.to_abi(), w, h, SEED, todo, s, 1)
            for i, g in enumerate(todo):
                _SLOTS[(name, g, s)] = (e.hit[i, 0], e.strike[i, 0], e.rays[i, 0], e.counters[i, 0])
    got = [[_SLOTS[(name, int(g), s)] for s in range(first, first + per)] for g in px]
    n = len(px)
    pick = lambda k, shape, dt: np.array([[slot[k] for slot in row] for row in got], dt).reshape((n, per) + shape)  # noqa: E731
    return cases.Expected(pick(0, (), np.int32), pick(1, (3,), np.float64), pick(2, (6,), np.float64), pick(3, (2,), np.int64))


def _np(a):
    return None if a is None else (a if isinstance(a, np.ndarray) else a.cpu().numpy())


def _assert_equals(got, want, what=()):
    assert np.array_equal(_np(got.hit_index), want.hit), what
    if got.strike is not None:
        assert cases.same_f64(_np(got.strike), want.strike), what
    if got.rays is not None:
        assert cases.same_f64(_np(got.rays), want.rays), what


def _hits(rt, name, px, first=0, per=1, **kw):
    _, cam, w, h = _frame(name)
    scene, cam = _scene(rt, name, kw.pop("walk_tree", None)), kw.pop("camera", cam)
    return scene.cameraHits(w, h, cam, px, sample_first=first, n_samples=per, seed=SEED, **kw)


@functools.lru_cache(maxsize=None)
def _sub(name, step=7):
    """Every step-th global index, the four corners and the centre, shuffled (not row-major), its first 10 entries once more."""
    cols, rows = SIZES[name]
    n = rows * cols
    idx = sorted(set(range(0, n, step)) | {0, cols - 1, n - cols, n - 1, (rows // 2) * cols + cols // 2})
    idx = np.random.default_rng(2024).permutation(np.array(idx, np.int32))
    out = np.concatenate([idx, idx[:10]]).astype(np.int32)
    out.setflags(write=False)
    return out


# ---- 1 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["all_materials", "many_spheres", "small_final", "free", "lights"])
def test_both_variants_equal_the_composer(rt, orc, name):
    n = _n(name)
    assert _scene(rt, name).info()["lds_resident"] == (0 if name == "many_spheres" else 1)
    want = _expected(orc, name, np.arange(n), 0, 2)
    kinds = set(want.hit.ravel().tolist())
    print(f"{name}: {len(kinds)} different answers over {2 * n} slots, {int((want.hit == -1).sum())} see nothing")
    assert len(kinds) >= {"all_materials": 9, "lights": 7}.get(name, 20) and (want.hit >= -1).all()
    assert (-1 in kinds) == (name == "lights")  # (the other scenes are closed by a dome)
    for counters in (False, True):
        got = _hits(rt, name, None, 0, 2, counters=counters)  # no list: entry i is pixel i
        _assert_equals(got, want, (name, counters))
        st = got.stats
        assert st["pixels"] == n and st["samples"] == 2 * n and st["reflections"] == 0 and st["pixels_early"] == 0
        assert st["kernel_ms"] > 0.0 and st["total_ms"] >= st["kernel_ms"]
        assert st["rays"] == (2 * n if counters else 0)
        plan = rt.hooks.last_launch_plan()
        assert plan["in"]["kind"] == 5 and plan["in"]["n"] == n and plan["in"]["spp"] == 2 and plan["in"]["first_sample"] == 0
        assert plan["out"]["q_mode"] == plan["out"]["F_mode"] == 14 and plan["out"]["two_pass"] == 0 and plan["out"]["q_count"] == int(counters)
        assert plan["out"]["F_chunk"] == (plan["in"]["s_chunk"] or 32) and plan["out"]["F_park"] == 0 and plan["out"]["q_lds"] == (0 if name == "many_spheres" else 1)
    # the strike point lies on the ray, |direction| = 1, and the origin is the eye
    eye = np.array(list(_frame(name)[1].to_abi().view_origin))
    assert np.array_equal(want.rays[..., :3], np.broadcast_to(eye, want.rays[..., :3].shape))
    assert np.allclose(np.linalg.norm(want.rays[..., 3:], axis=-1), 1.0, atol=1e-12)


# ---- 2 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["all_materials", "many_spheres"])
def test_sample_ranges(rt, orc, name):
    px = _sub(name, 13)
    for first in (0, 11, 37):
        for per in (1, 2, 12):
            want = _expected(orc, name, px, first, per)
            for counters in (False, True):
                got = _hits(rt, name, px, first, per, counters=counters)
                _assert_equals(got, want, (name, first, per, counters))
                assert got.hit_index.shape == (len(px), per) and got.strike.shape == (len(px), per, 3) and got.rays.shape == (len(px), per, 6)
                assert np.array_equal(got.hit_index[-10:], got.hit_index[:10]) and cases.same_f64(got.rays[-10:], got.rays[:10])  # the duplicates
                assert rt.hooks.last_launch_plan()["in"]["first_sample"] == first and rt.hooks.last_launch_plan()["in"]["spp"] == per
    # samples 0 .. 11 in one call are the twelve single-sample calls side by side
    whole = _hits(rt, name, px, 0, 12)
    singles = [_hits(rt, name, px, s, 1) for s in range(12)]
    assert np.array_equal(whole.hit_index, np.concatenate([r.hit_index for r in singles], axis=1))
    assert cases.same_f64(whole.strike, np.concatenate([r.strike for r in singles], axis=1))
    assert cases.same_f64(whole.rays, np.concatenate([r.rays for r in singles], axis=1))
    # different samples of a pixel are different rays
    assert not np.array_equal(whole.rays[:, 0], whole.rays[:, 1])


# ---- 3 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["all_materials", "many_spheres"])
def test_lists(rt, orc, name):
    n = _n(name)
    every = np.arange(n, dtype=np.int32)
    rng = np.random.default_rng(7)
    scattered = rng.integers(0, n, 500).astype(np.int32)  # with repeats
    scattered[100:110] = scattered[:10]
    assert len(set(scattered.tolist())) < 500
    lists = [("reversed", every[::-1].copy()), ("scattered", scattered)] + [(f"n={k}", np.array(_sub(name)[:k])) for k in (1, 63, 64, 65)]
    for label, px in lists:
        want = _expected(orc, name, px, 5, 3)
        for counters in (False, True):
            got = _hits(rt, name, px, 5, 3, counters=counters)
            _assert_equals(got, want, (name, label, counters))
            assert got.stats["pixels"] == len(px) and got.stats["samples"] == 3 * len(px)
    # no list: the first k pixels of the frame
    for k in (1, 63, 64, 65, n):
        want = _expected(orc, name, every[:k], 5, 3)
        for counters in (False, True):
            _assert_equals(_hits(rt, name, None, 5, 3, n=k, counters=counters), want, (name, "NULL", k, counters))


# ---- 4 -----------------------------------------------------------------------------------------------------------------------
SETTINGS = (dict(block_threads=256), dict(block_threads=1024), dict(chunk_pixels=1), dict(chunk_pixels=7), dict(chunk_pixels=64),
            dict(yield_lanes=1, refill_lanes=1), dict(yield_lanes=64, refill_lanes=64), dict(yield_lanes=1, refill_lanes=64),
            dict(yield_lanes=64, refill_lanes=1), dict(block_threads=256, chunk_pixels=7, yield_lanes=1, refill_lanes=64), dict(blocks_per_cu=1))


@pytest.mark.parametrize("name", ["all_materials", "many_spheres"])
def test_launch_settings_do_not_change_results(rt, orc, name):
    torch = pytest.importorskip("torch")
    A = rt._abi
    px = np.array(_sub(name))
    d_px = torch.from_numpy(px).cuda()
    for per in (2, 12):
        want = _expected(orc, name, px, 3, per)
        for opt in SETTINGS:
            for counters in (False, True):
                got = _hits(rt, name, d_px, 3, per, counters=counters, options=A.rt_render_options(**opt))
                _assert_equals(got, want, (name, per, opt, counters))
                o = rt.hooks.last_launch_plan()["out"]
                assert o["q_mode"] == 14 and o["F_grid"] > 0 and ("block_threads" not in opt or o["q_block"] == opt["block_threads"])
                if "chunk_pixels" in opt:
                    assert o["F_chunk"] == opt["chunk_pixels"]
                if "yield_lanes" in opt:
                    assert (o["F_yield"], o["F_refill"]) == (opt["yield_lanes"], opt["refill_lanes"])
    # a block of 512 or 768 threads runs as 1024
    for block in (512, 768):
        got = _hits(rt, name, d_px, 3, 2, options=A.rt_render_options(block_threads=block))
        _assert_equals(got, _expected(orc, name, px, 3, 2), (block,))
        assert rt.hooks.last_launch_plan()["out"]["q_block"] == 1024


# ---- 5 -----------------------------------------------------------------------------------------------------------------------
def test_null_outputs(rt, orc):
    torch = pytest.importorskip("torch")
    name = "all_materials"
    px = np.array(_sub(name))
    want = _expected(orc, name, px, 1, 2)
    for arg in (px, torch.from_numpy(px).cuda()):
        for strike in (True, False):
            for rays in (True, False):
                for counters in (False, True):
                    got = _hits(rt, name, arg, 1, 2, strike=strike, rays=rays, counters=counters)
                    assert (got.strike is not None) == strike and (got.rays is not None) == rays
                    _assert_equals(got, want, (strike, rays, counters))


# ---- 6 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small_final", "many_spheres"])
def test_counters_are_the_references(rt, orc, name):
    """Over BoundingBoxTree.make's own tree the counting variant makes the oracle's box tests and primitive tests, slot for slot in sum."""
    px = np.array(_sub(name))
    want = _expected(orc, name, px, 2, 3)
    got = _hits(rt, name, px, 2, 3, counters=True, walk_tree="reference")
    _assert_equals(got, want)
    st = got.stats
    assert st["rays"] == int((want.hit != -2).sum()) == 3 * len(px)
    assert st["aabb_tests"] == int(want.counters[..., 0].sum()) > 0 and st["prim_tests"] == int(want.counters[..., 1].sum()) > 0
    assert st["reflections"] == 0 and st["pixels"] == len(px) and st["samples"] == 3 * len(px)
    timed = _hits(rt, name, px, 2, 3, walk_tree="reference").stats
    assert timed["rays"] == timed["aabb_tests"] == timed["prim_tests"] == 0 and timed["samples"] == 3 * len(px)


# ---- 7 -----------------------------------------------------------------------------------------------------------------------
def test_device_entry_on_streams(rt, orc):
    torch = pytest.importorskip("torch")
    name = "all_materials"
    n = _n(name)
    lists = [np.array(_sub(name)), np.arange(n, dtype=np.int32)[::-1].copy(), np.array(_sub(name, 13)), None]
    prev = torch.cuda.current_device()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = []
    for k, px in enumerate(lists):  # four launches in flight on two non-default streams, none waited for
        with torch.cuda.stream(streams[k % 2]):
            t = torch.from_numpy(px).cuda() if px is not None else None
            got.append((t, _hits(rt, name, t, 2, 3, stats=False, tensors=True)))
            assert _scene(rt, name).last_stats is None and got[-1][1].stats is None
    torch.cuda.synchronize()
    assert torch.cuda.current_device() == prev
    for px, (_, g) in zip(lists, got):
        m = n if px is None else len(px)
        assert g.hit_index.dtype == torch.int32 and g.strike.dtype == torch.float64 and g.hit_index.is_cuda and tuple(g.rays.shape) == (m, 3, 6)
        _assert_equals(g, _expected(orc, name, np.arange(n) if px is None else px, 2, 3))
    # with statistics, on a stream
    with torch.cuda.stream(streams[1]):
        g = _hits(rt, name, torch.from_numpy(lists[0]).cuda(), 2, 3)
    assert g.stats["kernel_ms"] > 0.0 and g.stats["pixels"] == len(lists[0])
    _assert_equals(g, _expected(orc, name, lists[0], 2, 3))
    assert torch.cuda.current_device() == prev


# ---- 8 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["all_materials", "many_spheres"])
def test_a_device_list_with_entries_outside_the_frame_writes_nothing(rt, orc, name):
    torch = pytest.importorskip("torch")
    A = rt._abi
    _, cam, w, h = _frame(name)
    good = np.array(_sub(name))
    n, per = len(good), 2
    S = _scene(rt, name).handle
    abi = cam.to_abi()
    for entries in ((-1,), (_n(name),), (-1, _n(name))):
        bad = good.copy()
        for k, e in enumerate(entries):
            bad[3 + k * (n // 2)] = e
        for opt in (None, A.rt_render_options(chunk_pixels=1), A.rt_render_options(chunk_pixels=64, block_threads=256)):
            for flags in (0, A.RT_RENDER_COUNTERS):
                for stats in (True, False):
                    d_px = torch.from_numpy(bad).cuda()
                    d_hit = torch.full((n, per), SENTINEL_I, dtype=torch.int32, device="cuda")
                    d_strike = torch.full((n, per, 3), SENTINEL_F, dtype=torch.float64, device="cuda")
                    d_rays = torch.full((n, per, 6), SENTINEL_F, dtype=torch.float64, device="cuda")
                    st = A.rt_stats()
                    rc = rt.lib.rt_camera_hits_device(S, C.byref(abi), w, h, SEED, 0, n, d_px.data_ptr(), 0, per, flags, d_hit.data_ptr(), d_strike.data_ptr(),
                                                      d_rays.data_ptr(), torch.cuda.current_stream().cuda_stream, C.byref(opt) if opt is not None else None,
                                                      C.byref(st) if stats else None)
                    torch.cuda.synchronize()
                    assert rc == (A.RT_ERR_INVALID_ARGUMENT if stats else A.RT_OK), (entries, flags, stats)
                    if stats:
                        assert b"outside the frame" in rt.lib.rt_last_error()
                    assert bool((d_hit == SENTINEL_I).all()) and bool((d_strike == SENTINEL_F).all()) and bool((d_rays == SENTINEL_F).all()), (entries, flags, stats)
    # the wrapper raises; the valid list is still answered afterwards
    with pytest.raises(rt.RtError) as e:
        _hits(rt, name, torch.from_numpy(bad).cuda(), 0, per)
    assert e.value.code == A.RT_ERR_INVALID_ARGUMENT
    _assert_equals(_hits(rt, name, torch.from_numpy(good).cuda(), 0, per), _expected(orc, name, good, 0, per))


# ---- 9 -----------------------------------------------------------------------------------------------------------------------
def test_a_camera_whose_rays_cannot_be_made(rt, orc):
    """rt_render's checks admit a camera with viewport_width = viewport_height = 0 and xaxis_origin = eye: every end point is the eye,
    Ray.make' gives ValueNone for every sample, and every slot is -2 with NaNs -- no ray is made, nothing is walked."""
    name = "small_final"
    a = _frame(name)[1].to_abi()
    eye = np.array(list(a.view_origin))
    cam = scenes.free_camera(eye, eye, list(a.xaxis_dir), list(a.yaxis_dir), 0.0, 0.0, 40, DEPTH)
    px = np.array(_sub(name))
    want = _expected(orc, name, px, 0, 3, cam=cam)
    assert (want.hit == -2).all() and np.isnan(want.strike).all() and np.isnan(want.rays).all()
    for counters in (False, True):
        got = _hits(rt, name, px, 0, 3, camera=cam, counters=counters)
        _assert_equals(got, want, (counters,))
        assert got.stats["rays"] == 0 and got.stats["aabb_tests"] == 0 and got.stats["samples"] == 3 * len(px)


# ---- 10 ----------------------------------------------------------------------------------------------------------------------
def test_c_program_asks_once(rt, orc, tmp_path):
    from test_camera_hits_host import build_camera_hits_smoke
    from test_gpu_ray_queries import _smoke_scene
    out = subprocess.run([build_camera_hits_smoke(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "camera hits: argument checks ok" in out.stdout and "camera hits: 30 slots answered on the GPU" in out.stdout
    rows = [ln.split()[1:] for ln in out.stdout.splitlines() if ln.startswith("slot ")]
    assert len(rows) == 30
    px = np.array([int(r[1]) for r in rows[::3]])
    assert px[9] == px[2] and px[0] == 25 * 15 - 1 and px[1] == 0 and [int(r[2]) for r in rows[:3]] == [4, 5, 6]
    hit = np.array([int(r[3]) for r in rows], np.int32).reshape(10, 3)
    f64 = np.array([[int(x, 16) for x in r[4:]] for r in rows], np.uint64).view(np.float64).reshape(10, 3, 9)
    max_w, max_h = 12, 7  # camera_hits_smoke.c's frame and camera
    cam = rt.Camera.makeBasic(24, 1.0, 25.0 / 15.0, rt.Point.make(0.0, 0.5, -2.0), rt.Vector.unitise(rt.Vector.make(0.0, 0.0, 1.0)), rt.Vector.make(0.0, 1.0, 0.0))
    cam = dataclasses.replace(cam, BounceDepth=10)
    want = cases.compose(orc, orc.OracleScene(_smoke_scene(rt)), cam.to_abi(), max_w, max_h, 5, px, 4, 3)
    assert np.array_equal(hit, want.hit) and cases.same_f64(f64[..., :3], want.strike) and cases.same_f64(f64[..., 3:], want.rays)
    assert len(set(hit.ravel().tolist())) >= 3
