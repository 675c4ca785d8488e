"""Scene.cameraHitsViews -- rt_camera_hits_views, rt_camera_hits_views_device, the camera_hits_views kernels -- against the answer
composed per view from the oracle's pieces (tests/camera_hit_cases.compose) and, where breadth matters more than independence, against
K single rt_camera_hits calls (an entry point already held to the composer by test_gpu_camera_hits.py).  Bit for bit in hit_index,
strike and rays, NaNs by position, no tolerance anywhere: every view against the composer in both kernel variants; rays that hit
nothing and a scene beyond the LDS under a shuffled list with duplicates; units against view ends (more views than a wave has lanes,
units shorter than the chunk, a default chunk above n); NULL outputs with sentinels beyond the buffers; two streams; a malformed device
list; one view whose rays cannot be made; a scene with a texture program; the C consumer."""
import ctypes as C
import dataclasses
import functools
import subprocess

import numpy as np
import pytest

import camera_hit_cases as cases
import scenes
from test_gpu_camera_hits import DEPTH, _frame, _sub
from test_gpu_views import _cameras

pytestmark = pytest.mark.gpu

SENTINEL_I, SENTINEL_F = 0x5A5A5A5A, 7.5
VIEWS_1, SEEDS_1 = (0, 1, 2, 1), (5, 5, 9, 6)  # test 1's batch: views 1 and 3 are one camera under two seeds


def _np(a):
    return None if a is None else (a if isinstance(a, np.ndarray) else a.cpu().numpy())


@functools.lru_cache(maxsize=None)
def _scene(rt, name):
    return rt.Scene.make(_frame(name)[0])


@functools.lru_cache(maxsize=None)
def _oracle_scene(orc, name):
    return orc.OracleScene(_frame(name)[0])


@functools.lru_cache(maxsize=None)
def _composed_1(orc):
    """Test 1's expected values: small_final at its own size, the whole frame, samples 0 and 1, per view -- computed once, never written to."""
    cams, w, h = _cameras("small_final")
    n = (2 * w + 1) * (2 * h + 1)
    return [cases.compose(orc, _oracle_scene(orc, "small_final"), cams[v].to_abi(), w, h, s, np.arange(n), 0, 2) for v, s in zip(VIEWS_1, SEEDS_1)]


def _assert_views(got, wants, what=()):
    """got: CameraHits with a leading [K] axis; wants: per view an Expected (the composer's) or a CameraHits (a single call's)."""
    hit, strike, rays = _np(got.hit_index), _np(got.strike), _np(got.rays)
    assert hit.shape[0] == len(wants), what
    for v, want in enumerate(wants):
        w_hit, w_strike, w_rays = (want.hit, want.strike, want.rays) if isinstance(want, cases.Expected) else (_np(want.hit_index), _np(want.strike), _np(want.rays))
        assert np.array_equal(hit[v], w_hit), (v,) + tuple(what)
        if strike is not None:
            assert cases.same_f64(strike[v], w_strike), (v,) + tuple(what)
        if rays is not None:
            assert cases.same_f64(rays[v], w_rays), (v,) + tuple(what)


def _singles(scene, w, h, cams, seeds, px, first, per, **kw):
    return [scene.cameraHits(w, h, c, px, sample_first=first, n_samples=per, seed=s, **kw) for c, s in zip(cams, seeds)]


# ---- 1 -----------------------------------------------------------------------------------------------------------------------
def test_every_view_equals_the_composer(rt, orc):
    cams, w, h = _cameras("small_final")
    n = (2 * w + 1) * (2 * h + 1)
    assert n == 49 * 33
    wants = _composed_1(orc)
    assert np.array_equal(wants[1].rays[..., :3], wants[3].rays[..., :3]) and not np.array_equal(wants[1].rays, wants[3].rays)  # one camera, two seeds
    assert not np.array_equal(wants[1].hit, wants[3].hit)
    scene = _scene(rt, "small_final")
    for counters in (False, True):
        got = scene.cameraHitsViews(w, h, [cams[v] for v in VIEWS_1], seeds=SEEDS_1, sample_first=0, n_samples=2, counters=counters)
        assert got.hit_index.shape == (4, n, 2) and got.strike.shape == (4, n, 2, 3) and got.rays.shape == (4, n, 2, 6)
        _assert_views(got, wants, (counters,))
        assert not np.array_equal(got.hit_index[1], got.hit_index[3]) and not cases.same_f64(got.rays[1], got.rays[3])
        st = got.stats
        assert st["pixels"] == 4 * n and st["samples"] == 4 * n * 2 and st["reflections"] == 0 and st["pixels_early"] == 0
        assert st["kernel_ms"] > 0.0 and st["total_ms"] >= st["kernel_ms"]
        made = sum(int((e.hit != -2).sum()) for e in wants)
        assert made == 4 * n * 2 and st["rays"] == (made if counters else 0)
        plan = rt.hooks.last_launch_plan()
        assert plan["in"]["kind"] == 7 and plan["in"]["n"] == n and plan["in"]["n_views"] == 4 and plan["in"]["spp"] == 2 and plan["in"]["first_sample"] == 0
        assert plan["out"]["q_mode"] == plan["out"]["F_mode"] == 14 and plan["out"]["two_pass"] == 0 and plan["out"]["q_count"] == int(counters)
        assert plan["out"]["F_chunk"] == (plan["in"]["s_chunk"] or 32) and plan["out"]["F_park"] == 0 and plan["out"]["q_lds"] == 1


# ---- 2 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lights", "many_spheres"])
def test_rays_that_hit_nothing_and_a_scene_beyond_the_lds(rt, orc, name):
    _, cam, w, h = _frame(name)
    a = cam.to_abi()
    eye, xo, xd, yd = (np.array(list(v)) for v in (a.view_origin, a.xaxis_origin, a.xaxis_dir, a.yaxis_dir))
    aside = scenes.free_camera(eye + 0.4 * xd, xo + 0.4 * xd, xd + 0.05 * yd, yd - 0.03 * xd, a.viewport_width, a.viewport_height, 40, DEPTH)
    scenes.require_clear_eye(aside, w, h)
    cams, seeds = [cam, aside], (5, 8)
    px = np.array(_sub(name))
    wants = [cases.compose(orc, _oracle_scene(orc, name), c.to_abi(), w, h, s, px, 3, 3) for c, s in zip(cams, seeds)]
    if name == "lights":
        assert all((e.hit == -1).any() and (e.hit >= 0).any() for e in wants)  # sky between the light sources, in both views
    scene = _scene(rt, name)
    assert scene.info()["lds_resident"] == (0 if name == "many_spheres" else 1)
    for counters in (False, True):
        got = scene.cameraHitsViews(w, h, cams, px, seeds=seeds, sample_first=3, n_samples=3, counters=counters)
        _assert_views(got, wants, (name, counters))
        assert np.array_equal(got.hit_index[:, -10:], got.hit_index[:, :10]) and cases.same_f64(got.rays[:, -10:], got.rays[:, :10])  # the duplicates
        plan = rt.hooks.last_launch_plan()
        assert plan["in"]["kind"] == 7 and plan["in"]["first_sample"] == 3 and plan["out"]["q_lds"] == (0 if name == "many_spheres" else 1)
        assert got.stats["pixels"] == 2 * len(px) and got.stats["samples"] == 2 * len(px) * 3


# ---- 3 -----------------------------------------------------------------------------------------------------------------------
def _many_cameras(k):
    cams, _, _ = _cameras("small_final")
    return [cams[v % 3] for v in range(k)], [100 + v for v in range(k)]


def test_units_against_view_ends_in_tiny_frames(rt, orc):
    """3 x 3 frames, the smallest there are, 70 views: more views than a wave has lanes, every unit shorter than a 64-entry chunk, a
    default chunk (10 at 7 samples, 64 at 1) above n."""
    torch = pytest.importorskip("torch")
    A = rt._abi
    w = h = 1
    k = 70
    cams, seeds = _many_cameras(k)
    scene = _scene(rt, "small_final")
    lists = (None, np.array([8, 0, 4, 4, 2], np.int32))
    composed = False
    for px in lists:
        n = 9 if px is None else len(px)
        d_px = None if px is None else torch.from_numpy(px).cuda()
        for per in (1, 7):
            wants = _singles(scene, w, h, cams, seeds, d_px, 2, per, tensors=True, stats=False)  # (70 launches, none waited for)
            for chunk in (0, 1, 64):
                got = scene.cameraHitsViews(w, h, cams, d_px, seeds=seeds, sample_first=2, n_samples=per, tensors=True,
                                            options=A.rt_render_options(chunk_pixels=chunk))
                assert tuple(got.hit_index.shape) == (k, n, per)
                _assert_views(got, wants, (n, per, chunk))
                plan = rt.hooks.last_launch_plan()
                assert plan["in"]["kind"] == 7 and plan["in"]["n_views"] == k and plan["in"]["n"] == n
                assert plan["out"]["F_chunk"] == (chunk or (64 if per == 1 else 10)) and (chunk == 1 or plan["out"]["F_chunk"] > n)
            if px is not None and per == 7:  # one case against the composer itself
                for v in (0, 1, 69):
                    e = cases.compose(orc, _oracle_scene(orc, "small_final"), cams[v].to_abi(), w, h, seeds[v], px, 2, per)
                    assert np.array_equal(_np(got.hit_index)[v], e.hit) and cases.same_f64(_np(got.strike)[v], e.strike) and cases.same_f64(_np(got.rays)[v], e.rays)
                composed = True
    assert composed


def test_units_against_view_ends_at_every_block(rt):
    """9 x 7 frames, 5 views, the whole frame (n = 63): units of 5 (thirteen a view, the last one of 3 entries) and of 64 (one short unit
    a view), at blocks of 256, 512 (runs as 1024) and 1024 threads, both variants."""
    pytest.importorskip("torch")
    A = rt._abi
    w, h, k = 4, 3, 5
    cams, seeds = _many_cameras(k)
    scene = _scene(rt, "small_final")
    wants = _singles(scene, w, h, cams, seeds, None, 0, 3)
    for chunk in (5, 64):
        for block in (256, 512, 1024):
            for counters in (False, True):
                got = scene.cameraHitsViews(w, h, cams, None, seeds=seeds, n_samples=3, tensors=True, counters=counters,
                                            options=A.rt_render_options(chunk_pixels=chunk, block_threads=block))
                _assert_views(got, wants, (chunk, block, counters))
                o = rt.hooks.last_launch_plan()["out"]
                assert o["q_block"] == (256 if block == 256 else 1024) and o["F_chunk"] == chunk and o["q_count"] == int(counters)


# ---- 4 -----------------------------------------------------------------------------------------------------------------------
def test_null_outputs_and_nothing_beyond_the_buffers(rt):
    torch = pytest.importorskip("torch")
    A = rt._abi
    w, h, k, per = 4, 3, 3, 2
    cams, seeds = _many_cameras(k)
    scene = _scene(rt, "small_final")
    px = np.array([62, 0, 31, 8, 54, 31, 17], np.int32)
    n = len(px)
    whole = scene.cameraHitsViews(w, h, cams, px, seeds=seeds, n_samples=per)
    _assert_views(whole, _singles(scene, w, h, cams, seeds, px, 0, per))
    abi = (A.rt_camera * k)(*[c.to_abi() for c in cams])
    keys = (C.c_uint64 * k)(*seeds)
    d_px = torch.from_numpy(px).cuda()
    slots, pad = k * n * per, 64
    for strike in (True, False):
        for rays in (True, False):
            d_hit = torch.full((slots + pad,), SENTINEL_I, dtype=torch.int32, device="cuda")
            d_strike = torch.full((slots * 3 + pad,), SENTINEL_F, dtype=torch.float64, device="cuda")
            d_rays = torch.full((slots * 6 + pad,), SENTINEL_F, dtype=torch.float64, device="cuda")
            st = A.rt_stats()
            rc = rt.lib.rt_camera_hits_views_device(scene.handle, abi, k, w, h, keys, 0, 0, n, d_px.data_ptr(), 0, per, 0, d_hit.data_ptr(),
                                                    d_strike.data_ptr() if strike else None, d_rays.data_ptr() if rays else None,
                                                    torch.cuda.current_stream().cuda_stream, None, C.byref(st))
            torch.cuda.synchronize()
            assert rc == A.RT_OK and st.pixels == k * n and st.samples == slots
            assert np.array_equal(d_hit[:slots].cpu().numpy().reshape(k, n, per), whole.hit_index) and bool((d_hit[slots:] == SENTINEL_I).all())
            if strike:
                assert cases.same_f64(d_strike[:slots * 3].cpu().numpy().reshape(k, n, per, 3), whole.strike)
            if rays:
                assert cases.same_f64(d_rays[:slots * 6].cpu().numpy().reshape(k, n, per, 6), whole.rays)
            assert bool((d_strike[slots * 3 if strike else 0:] == SENTINEL_F).all()) and bool((d_rays[slots * 6 if rays else 0:] == SENTINEL_F).all())
            # ... and the wrapper, on both routes
            for arg in (px, d_px):
                got = scene.cameraHitsViews(w, h, cams, arg, seeds=seeds, n_samples=per, strike=strike, rays=rays)
                assert (got.strike is not None) == strike and (got.rays is not None) == rays
                assert np.array_equal(_np(got.hit_index), whole.hit_index)
                assert not strike or cases.same_f64(_np(got.strike), whole.strike)
                assert not rays or cases.same_f64(_np(got.rays), whole.rays)


# ---- 5 -----------------------------------------------------------------------------------------------------------------------
def test_device_entry_on_two_streams(rt, orc):
    torch = pytest.importorskip("torch")
    cams, w, h = _cameras("small_final")
    n = (2 * w + 1) * (2 * h + 1)
    wants = _composed_1(orc)
    scene = _scene(rt, "small_final")
    prev = torch.cuda.current_device()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = []
    for i in range(2):  # two batches in flight on two non-default streams, none waited for: test 1's, and its views in reverse
        order = list(range(4)) if i == 0 else [3, 2, 1, 0]
        with torch.cuda.stream(streams[i]):
            g = scene.cameraHitsViews(w, h, [cams[VIEWS_1[v]] for v in order], seeds=[SEEDS_1[v] for v in order], n_samples=2, tensors=True, stats=False)
            assert g.stats is None and scene.last_stats is None
            got.append((order, g))
    torch.cuda.synchronize()
    assert torch.cuda.current_device() == prev
    for order, g in got:
        assert g.hit_index.dtype == torch.int32 and g.strike.dtype == g.rays.dtype == torch.float64 and g.hit_index.is_cuda
        assert tuple(g.hit_index.shape) == (4, n, 2) and tuple(g.rays.shape) == (4, n, 2, 6)
        _assert_views(g, [wants[v] for v in order], (order,))
    with torch.cuda.stream(streams[1]):  # with statistics, on a stream
        g = scene.cameraHitsViews(w, h, [cams[v] for v in VIEWS_1], seeds=SEEDS_1, n_samples=2, tensors=True)
    assert g.stats["kernel_ms"] > 0.0 and g.stats["pixels"] == 4 * n
    _assert_views(g, wants)
    assert torch.cuda.current_device() == prev


# ---- 6 -----------------------------------------------------------------------------------------------------------------------
def test_a_malformed_device_list_writes_nothing_in_any_view(rt):
    torch = pytest.importorskip("torch")
    A = rt._abi
    cams, w, h = _cameras("small_final")
    k, per = 3, 2
    good = np.array(_sub("small_final"))
    n = len(good)
    scene = _scene(rt, "small_final")
    abi = (A.rt_camera * k)(*[c.to_abi() for c in cams])
    for entry in (-1, 49 * 33):
        bad = good.copy()
        bad[n // 2] = entry
        for opt in (None, A.rt_render_options(chunk_pixels=1), A.rt_render_options(chunk_pixels=64, block_threads=256)):
            for flags in (0, A.RT_RENDER_COUNTERS):
                for stats in (True, False):
                    d_px = torch.from_numpy(bad).cuda()
                    d_hit = torch.full((k, n, per), SENTINEL_I, dtype=torch.int32, device="cuda")
                    d_strike = torch.full((k, n, per, 3), SENTINEL_F, dtype=torch.float64, device="cuda")
                    d_rays = torch.full((k, n, per, 6), SENTINEL_F, dtype=torch.float64, device="cuda")
                    st = A.rt_stats()
                    rc = rt.lib.rt_camera_hits_views_device(scene.handle, abi, k, w, h, None, 5, 0, n, d_px.data_ptr(), 0, per, flags, d_hit.data_ptr(),
                                                            d_strike.data_ptr(), d_rays.data_ptr(), torch.cuda.current_stream().cuda_stream,
                                                            C.byref(opt) if opt is not None else None, C.byref(st) if stats else None)
                    torch.cuda.synchronize()
                    assert rc == (A.RT_ERR_INVALID_ARGUMENT if stats else A.RT_OK), (entry, flags, stats)
                    if stats:
                        assert b"outside the frame" in rt.lib.rt_last_error()
                    assert bool((d_hit == SENTINEL_I).all()) and bool((d_strike == SENTINEL_F).all()) and bool((d_rays == SENTINEL_F).all()), (entry, flags, stats)
        # the host variant refuses before any device call
        with pytest.raises(rt.RtError) as e:
            scene.cameraHitsViews(w, h, list(cams), bad, seed=5, n_samples=per)
        assert e.value.code == A.RT_ERR_INVALID_ARGUMENT and b"outside the frame" in rt.lib.rt_last_error()
    # the wrapper raises on the device route; the valid list is still answered afterwards
    with pytest.raises(rt.RtError) as e:
        scene.cameraHitsViews(w, h, list(cams), torch.from_numpy(bad).cuda(), seed=5, n_samples=per)
    assert e.value.code == A.RT_ERR_INVALID_ARGUMENT
    got = scene.cameraHitsViews(w, h, list(cams), torch.from_numpy(good).cuda(), seed=5, n_samples=per)
    _assert_views(got, _singles(scene, w, h, cams, (5, 5, 5), good, 0, per))


# ---- 7 -----------------------------------------------------------------------------------------------------------------------
def test_one_view_whose_rays_cannot_be_made(rt):
    """test_a_camera_whose_rays_cannot_be_made's camera (viewport 0 x 0 at the eye: Ray.make' gives ValueNone for every sample) as view
    1 of 3: that slice is all -2 and NaN, the views around it are their single calls."""
    name = "small_final"
    _, cam, w, h = _frame(name)
    a = cam.to_abi()
    eye = np.array(list(a.view_origin))
    blind = scenes.free_camera(eye, eye, list(a.xaxis_dir), list(a.yaxis_dir), 0.0, 0.0, 40, DEPTH)
    other = _cameras(name)[0][1]
    cams, seeds = [cam, blind, other], (5, 5, 7)
    px = np.array(_sub(name))
    scene = _scene(rt, name)
    wants = _singles(scene, w, h, cams, seeds, px, 0, 3)
    assert (wants[0].hit_index >= -1).all() and (wants[2].hit_index >= -1).all()
    for counters in (False, True):
        got = scene.cameraHitsViews(w, h, cams, px, seeds=seeds, n_samples=3, counters=counters)
        assert (got.hit_index[1] == -2).all() and np.isnan(got.strike[1]).all() and np.isnan(got.rays[1]).all()
        _assert_views(got, wants, (counters,))
        assert got.stats["rays"] == (2 * 3 * len(px) if counters else 0) and got.stats["samples"] == 3 * 3 * len(px)


# ---- 8 -----------------------------------------------------------------------------------------------------------------------
def test_a_scene_with_a_texture_program_is_accepted(rt):
    """The scene rt_render_views refuses (tests/test_views_host.py): nothing is shaded here, so the batch takes it, as rt_camera_hits does."""
    import texture_cases as tc
    from ray_tracing_fsharp_amd import texprog as T
    from test_views_host import MAX_H, MAX_W, _camera
    tp = rt.Texture.Program(T.PX * 10.0, T.PY, T.PZ)
    objs = [tc.wear(0, rt.ParameterisedTexture.Program(1.0, 2.0, 3.0)),
            rt.Hittable.Sphere(rt.Sphere.make(rt.SphereStyle.LightSource(tp), rt.Point.make(8.0, 0.0, 0.0), 1.0))]
    scene = rt.Scene.make(objs)
    with pytest.raises(rt.RtError) as e:
        scene.renderViews(MAX_W, MAX_H, [_camera(rt)] * 2)
    assert e.value.code == rt._abi.RT_ERR_UNSUPPORTED
    cams, seeds = [_camera(rt), _camera(rt, spp=7, depth=5)], (3, 4)
    wants = _singles(scene, MAX_W, MAX_H, cams, seeds, None, 1, 2)
    for counters in (False, True):
        got = scene.cameraHitsViews(MAX_W, MAX_H, cams, seeds=seeds, sample_first=1, n_samples=2, counters=counters)
        _assert_views(got, wants, (counters,))


# ---- 9 -----------------------------------------------------------------------------------------------------------------------
def test_c_program_asks_once(rt, tmp_path):
    from test_camera_hits_views_host import build_camera_hits_views_smoke
    from test_gpu_ray_queries import _smoke_scene
    out = subprocess.run([build_camera_hits_views_smoke(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "camera hits views: argument checks ok" in out.stdout and "camera hits views: 36 slots answered on the GPU" in out.stdout
    rows = [ln.split()[1:] for ln in out.stdout.splitlines() if ln.startswith("slot ")]
    assert len(rows) == 36
    k, n, per, max_w, max_h = 3, 6, 2, 4, 3  # camera_hits_views_smoke.c's batch, frame and cameras
    assert [int(r[1]) for r in rows] == [i // (n * per) for i in range(36)] and [int(r[3]) for r in rows[:2]] == [4, 5]
    px = np.array([int(r[2]) for r in rows[:n * per:per]], np.int32)
    assert px[5] == px[1] and px[0] == 9 * 7 - 1 and px[2] == 0
    hit = np.array([int(r[4]) for r in rows], np.int32).reshape(k, n, per)
    f64 = np.array([[int(x, 16) for x in r[5:]] for r in rows], np.uint64).view(np.float64).reshape(k, n, per, 9)
    scene = rt.Scene.make(_smoke_scene(rt))
    origins, seeds = ((0.0, 0.5, -2.0), (1.0, 0.5, -2.0), (-1.5, 1.0, -2.5)), (5, 5, 11)
    for v in range(k):
        cam = rt.Camera.makeBasic(24 + v, 1.0, 9.0 / 7.0, rt.Point.make(*origins[v]), rt.Vector.unitise(rt.Vector.make(0.0, 0.0, 1.0)), rt.Vector.make(0.0, 1.0, 0.0))
        want = scene.cameraHits(max_w, max_h, dataclasses.replace(cam, BounceDepth=10 + v), px, sample_first=4, n_samples=per, seed=seeds[v])
        assert np.array_equal(hit[v], want.hit_index) and cases.same_f64(f64[v, ..., :3], want.strike) and cases.same_f64(f64[v, ..., 3:], want.rays), v
    assert len(set(hit.ravel().tolist())) >= 3
