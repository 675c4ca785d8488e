"""Scene.renderViews -- rt_render_views and rt_render_views_device, the render_views kernels -- against the ORACLE's frame for each view's
camera and seed (OracleScene.render_rows), bit for bit in every PixelStats word and every rgb byte, never against the library's own
rt_render: views of different cost mixed in one wave and one pass-B list at every sample count around the adaptive rule's edges, fused
and in two passes, both kernel variants with their counters; tiny views (more views than a wave has lanes, one-pixel units) at every
unit size and block; one view, repeated views and seeds; the global-memory, the textured and a non-default-schedule route; the device
entry on streams and into a caller's tensor; and a view's slice continued by extend_rows."""
import ctypes as C
import dataclasses
import functools
import types

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

DEPTH = 12
EARLY = 11  # Count of a pixel that stopped early, at every spp >= 10
SPPS = (1, 2, 3, 9, 10, 11, 12, 40)
COUNTERS = ("rays", "aabb_tests", "prim_tests", "reflections")
P, V = scenes.P, scenes.V


@functools.lru_cache(maxsize=None)
def _objects(name):
    if name == "earth_thumb":
        return scenes.earth_thumb(scenes.golden("earthmap_rgb")["rgb"])
    return getattr(scenes, name)()


@functools.lru_cache(maxsize=None)
def _cameras(name):
    """The views of a scene, at BounceDepth 12: (cameras, max_w, max_h)"""
    import ray_tracing_fsharp_amd as rt
    objs, cam, w, h = _objects(name)
    cam = dataclasses.replace(cam, BounceDepth=DEPTH)
    a = cam.to_abi()
    eye, xo, xd, yd = (np.array(list(v)) for v in (a.view_origin, a.xaxis_origin, a.xaxis_dir, a.yaxis_dir))
    if name == "small_final":
        # the scene's own; test_gpu_pixels.py's off-centre "free" camera (pixel_candidates answers RTD_CAND_WALK for some pixels); one
        # turned to the sky from above the spheres, where every pixel stops early
        free = scenes.free_camera(eye, xo + xd * (0.3 * a.viewport_width) - yd * (0.2 * a.viewport_height), xd + 0.1 * yd, yd, a.viewport_width,
                                  a.viewport_height, 40, DEPTH)
        scenes.require_clear_eye(free, w, h)
        sky = dataclasses.replace(rt.Camera.makeBasic(40, 1.0, (2 * w + 1) / (2 * h + 1), P(0.0, 30.0, 0.0), scenes.unit(0.0, 1.0, 0.0), V(0.0, 0.0, 1.0)),
                                  BounceDepth=DEPTH)
        return (cam, free, sky), w, h
    # the scene's own and one moved aside and tilted
    other = scenes.free_camera(eye + 0.4 * xd, xo + 0.4 * xd, xd + 0.05 * yd, yd - 0.03 * xd, a.viewport_width, a.viewport_height, 40, DEPTH)
    scenes.require_clear_eye(other, w, h)
    return (cam, other), w, h


def _cam(cam, spp):
    return dataclasses.replace(cam, SamplesPerPixel=spp)


@functools.lru_cache(maxsize=None)
def _scene(rt, name):
    return rt.Scene.make(_objects(name)[0])


@functools.lru_cache(maxsize=None)
def _oracle_scene(orc, name):
    return orc.OracleScene(_objects(name)[0])


@functools.lru_cache(maxsize=None)
def _oracle(orc, name, view, spp, seed, size=None):
    """The oracle's frame of view `view` of the scene at spp and seed: (accum [rows, cols, 4], rgb [rows, cols, 3], stats); computed
    once, never written to.  size: (max_w, max_h) other than the scene's own."""
    cams, w, h = _cameras(name)
    if size is not None:
        w, h = size
    acc, rgb, st = _oracle_scene(orc, name).render_rows(w, h, _cam(cams[view], spp).to_abi(), seed=seed, threads=16)
    acc.setflags(write=False); rgb.setflags(write=False)
    return acc, rgb, st


def _np(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def _assert_views(got, orc, name, views, spp, seeds, size=None, what=()):
    acc, rgb = _np(got.accum), _np(got.rgb)
    assert acc.shape[0] == rgb.shape[0] == len(views)
    for i, (view, seed) in enumerate(zip(views, seeds)):
        want_acc, want_rgb, _ = _oracle(orc, name, view, spp, seed, size)
        assert acc[i].shape == want_acc.shape and rgb[i].shape == want_rgb.shape
        assert np.array_equal(acc[i], want_acc), (name, i, view, spp, seed) + tuple(what)
        assert np.array_equal(rgb[i], want_rgb), (name, i, view, spp, seed) + tuple(what)


def _render(rt, name, views, spp, seeds, size=None, **kw):
    cams, w, h = _cameras(name)
    if size is not None:
        w, h = size
    return _scene(rt, name).renderViews(w, h, [_cam(cams[v], spp) for v in views], seeds=seeds, **kw)


def _tensor_accum(torch, k, w, h):
    return torch.full((k, 2 * h + 1, 2 * w + 1, 4), -7, dtype=torch.int32, device="cuda")


# ---- 1 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", SPPS)
def test_mixed_views_in_one_wave_and_one_list(rt, orc, spp):
    """small_final at 49 x 33: 1,617 pixels a view, no multiple of 64; the scene's own camera, the off-centre one and the sky, seeds (5, 5, 9)."""
    torch = pytest.importorskip("torch")
    A = rt._abi
    name, views, seeds = "small_final", (0, 1, 2), (5, 5, 9)
    cams, w, h = _cameras(name)
    assert (2 * w + 1, 2 * h + 1) == (49, 33)
    want = [_oracle(orc, name, v, spp, s) for v, s in zip(views, seeds)]
    if spp >= 12:  # the sky stops early everywhere; the other views do not
        assert (want[2][0][..., 0] == EARLY).all() and 0 < int((want[0][0][..., 0] == spp).sum()) < 1617 and (want[1][0][..., 0] == spp).any()
    for passes in (1, 2):
        for counters in (False, True):
            got = _render(rt, name, views, spp, seeds, counters=counters, accum=_tensor_accum(torch, 3, w, h), options=A.rt_render_options(passes=passes))
            _assert_views(got, orc, name, views, spp, seeds, what=(passes, counters))
            plan = rt.hooks.last_launch_plan()
            n2 = spp - (2 * min(5, spp // 2) + 1)
            assert plan["in"]["kind"] == 6 and plan["in"]["n"] == 3 and plan["in"]["n_rows"] == 33 and plan["in"]["s_passes"] == passes
            assert plan["out"]["two_pass"] == (1 if passes == 2 and n2 > 0 else 0) and plan["out"]["error"] == 0
            st = got.stats
            assert st["pixels"] == 3 * 1617 and st["kernel_ms"] > 0.0
            assert st["samples"] == sum(x[2]["samples"] for x in want) == sum(int(x[0][..., 0].sum()) for x in want)
            assert st["pixels_early"] == sum(x[2]["pixels_early"] for x in want)
            for key in COUNTERS:
                if not counters:
                    assert st[key] == 0
                elif key != "aabb_tests":  # (the box-test count is the reference's only when the reference's tree is walked)
                    assert st[key] == sum(x[2][key] for x in want), (key, passes)
    if spp == 40:  # under counters with the reference's own tree, the fourth counter too
        rt.set_walk_tree("reference")
        try:
            scene = rt.Scene.make(_objects(name)[0])
        finally:
            rt.set_walk_tree("sah")
        got = scene.renderViews(w, h, [_cam(cams[v], spp) for v in views], seeds=seeds, counters=True)
        _assert_views(got, orc, name, views, spp, seeds, what=("reference tree",))
        for key in COUNTERS:
            assert got.stats[key] == sum(x[2][key] for x in want), key


# ---- 2 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,k", [((2, 1), 9), ((1, 1), 70)])
def test_tiny_views(rt, orc, size, k):
    """5 x 3 frames with K = 9, and the smallest frame the library takes, 3 x 3, with K = 70: more views than a wave has lanes, and with
    chunk_pixels = 1 one-pixel units.  (rt_render refuses max_width_coord = 0, so a 1 x 1 frame does not exist.)"""
    torch = pytest.importorskip("torch")
    A = rt._abi
    name, spp = "small_final", 40
    w, h = size
    views = [(0, 1)[i % 2] for i in range(k)]  # the scene's own camera and the off-centre one, in turn
    seeds = [3 + i for i in range(k)]
    for chunk in (1, 7, 64):
        for block, runs_as in ((256, 256), (1024, 1024), (512, 1024)):
            for passes in (1, 2):
                if block == 512 and (chunk != 7 or passes != 2):
                    continue
                got = _render(rt, name, views, spp, seeds, size=size, accum=_tensor_accum(torch, k, w, h),
                              options=A.rt_render_options(chunk_pixels=chunk, block_threads=block, passes=passes))
                _assert_views(got, orc, name, views, spp, seeds, size=size, what=(chunk, block, passes))
                o = rt.hooks.last_launch_plan()["out"]
                assert o["q_block"] == runs_as and o["two_pass"] == passes - 1 and (o["A_chunk"] if passes == 2 else o["F_chunk"]) == chunk
                assert got.stats["pixels"] == k * (2 * w + 1) * (2 * h + 1)
    # and through arrays, with the plan's own settings
    got = _render(rt, name, views, spp, seeds, size=size)
    _assert_views(got, orc, name, views, spp, seeds, size=size, what=("arrays",))


# ---- 3 -----------------------------------------------------------------------------------------------------------------------
def test_degenerate_and_repeated_views(rt, orc):
    name, spp = "small_final", 40
    cams, w, h = _cameras(name)
    # K = 1 is the frame
    got = _render(rt, name, (0,), spp, (5,))
    _assert_views(got, orc, name, (0,), spp, (5,))
    assert got.accum.shape == (1, 33, 49, 4) and got.stats["pixels"] == 1617
    # the same camera twice: equal seeds give equal views, different seeds each the oracle's frame for its seed
    got = _render(rt, name, (1, 1), spp, (9, 9))
    _assert_views(got, orc, name, (1, 1), spp, (9, 9))
    assert np.array_equal(got.accum[0], got.accum[1]) and np.array_equal(got.rgb[0], got.rgb[1])
    got = _render(rt, name, (1, 1, 0), spp, (9, 5, 5))
    _assert_views(got, orc, name, (1, 1, 0), spp, (9, 5, 5))
    assert not np.array_equal(got.accum[0], got.accum[1])
    # seeds=None: `seed` for every view
    got = _scene(rt, name).renderViews(w, h, [_cam(cams[v], spp) for v in (0, 1, 2)], seed=5)
    _assert_views(got, orc, name, (0, 1, 2), spp, (5, 5, 5))
    got = _scene(rt, name).renderViews(w, h, [_cam(cams[1], spp)])  # (seed 0)
    _assert_views(got, orc, name, (1,), spp, (0,))


# ---- 4 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,resident,tex", [("many_spheres", 0, 0), ("earth_thumb", 1, 1)])
def test_every_scene_route(rt, orc, name, resident, tex):
    """The global-memory scene the GPU tests pad past the LDS (35 x 21) and the textured earth_thumb (65 x 37), two cameras each."""
    torch = pytest.importorskip("torch")
    A = rt._abi
    cams, w, h = _cameras(name)
    info = _scene(rt, name).info()
    assert info["lds_resident"] == resident and (info["n_textures"] > 0) == bool(tex)
    views, seeds, spp = (0, 1, 0), (5, 6, 7), 40
    for passes in (1, 2):
        for counters in (False, True):
            got = _render(rt, name, views, spp, seeds, counters=counters, accum=_tensor_accum(torch, 3, w, h), options=A.rt_render_options(passes=passes))
            _assert_views(got, orc, name, views, spp, seeds, what=(passes, counters))
            o = rt.hooks.last_launch_plan()["out"]
            assert o["q_tex"] == tex and o["two_pass"] == passes - 1
    got = _render(rt, name, views, 12, seeds)
    _assert_views(got, orc, name, views, 12, seeds)


def test_a_non_default_schedule(rt, orc):
    torch = pytest.importorskip("torch")
    A = rt._abi
    name, views, seeds, spp = "small_final", (0, 1, 2), (5, 5, 9), 40
    _, w, h = _cameras(name)
    for passes in (1, 2):
        got = _render(rt, name, views, spp, seeds, accum=_tensor_accum(torch, 3, w, h), options=A.rt_render_options(yield_lanes=20, passes=passes))
        _assert_views(got, orc, name, views, spp, seeds, what=("yield 20", passes))
        assert rt.hooks.last_launch_plan()["in"]["s_yield"] == 20


# ---- 5 -----------------------------------------------------------------------------------------------------------------------
def test_streams_and_tensors(rt, orc):
    torch = pytest.importorskip("torch")
    A = rt._abi
    name, spp = "small_final", 40
    cams, w, h = _cameras(name)
    scene = _scene(rt, name)
    prev = torch.cuda.current_device()
    # the device variant on a non-null stream with stats == NULL, through the C ABI itself
    views, seeds = (0, 1, 2), (5, 5, 9)
    s0 = torch.cuda.Stream()
    with torch.cuda.stream(s0):
        d_acc = _tensor_accum(torch, 3, w, h)
        d_rgb = torch.zeros((3, 33, 49, 3), dtype=torch.uint8, device="cuda")
    abi = (A.rt_camera * 3)(*[_cam(cams[v], spp).to_abi() for v in views])
    keys = (C.c_uint64 * 3)(*seeds)
    assert s0.cuda_stream != 0
    rc = rt.lib.rt_render_views_device(scene.handle, abi, 3, w, h, keys, 0, 0, 0, d_acc.data_ptr(), d_rgb.data_ptr(), s0.cuda_stream, None, None)
    assert rc == A.RT_OK
    s0.synchronize()
    _assert_views(types.SimpleNamespace(accum=d_acc, rgb=d_rgb), orc, name, views, spp, seeds, what=("raw",))
    # two batches in flight on two streams, two passes each
    batches = [((0, 1, 2), (5, 5, 9)), ((2, 1, 0, 1), (9, 9, 5, 5))]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = []
    for (vs, sd), st in zip(batches, streams):
        with torch.cuda.stream(st):
            acc = _tensor_accum(torch, len(vs), w, h)
            got.append(_render(rt, name, vs, spp, sd, accum=acc, stats=False, options=A.rt_render_options(passes=2)))
            assert got[-1].accum is acc and got[-1].stats is None and scene.last_stats is None
    torch.cuda.synchronize()
    assert torch.cuda.current_device() == prev
    for (vs, sd), g in zip(batches, got):
        assert g.rgb.is_cuda and g.rgb.dtype == torch.uint8 and tuple(g.rgb.shape) == (len(vs), 33, 49, 3)
        _assert_views(g, orc, name, vs, spp, sd)
    # the torch route into a caller's tensor, with statistics
    acc = _tensor_accum(torch, 2, w, h)
    g = _render(rt, name, (1, 0), spp, (9, 5), accum=acc)
    assert g.accum is acc and g.stats["kernel_ms"] > 0.0 and g.stats["pixels"] == 2 * 1617
    _assert_views(g, orc, name, (1, 0), spp, (9, 5))


# ---- 6 -----------------------------------------------------------------------------------------------------------------------
def test_a_views_slice_is_a_frames_buffer(rt, orc):
    """View 1's slice of a batch at 12 samples, continued by extend_rows with cameras[1] to 40, equals the oracle at 40."""
    torch = pytest.importorskip("torch")
    name, views, seeds = "small_final", (0, 1, 2), (5, 5, 9)
    cams, w, h = _cameras(name)
    base = _render(rt, name, views, 12, seeds, accum=_tensor_accum(torch, 3, w, h))
    _assert_views(base, orc, name, views, 12, seeds)
    want_acc, want_rgb, _ = _oracle(orc, name, 1, 40, 5)
    ext = _scene(rt, name).extend_rows(w, h, _cam(cams[1], 40), base.accum[1], 12, seed=5)
    assert ext.accum.data_ptr() == base.accum[1].data_ptr()  # in place: the slice IS the buffer
    assert np.array_equal(_np(ext.accum), want_acc) and np.array_equal(_np(ext.rgb), want_rgb)
    # the neighbours are untouched
    for i in (0, 2):
        assert np.array_equal(_np(base.accum[i]), _oracle(orc, name, views[i], 12, seeds[i])[0])
    # and through arrays
    arr = _render(rt, name, views, 12, seeds)
    ext = _scene(rt, name).extend_rows(w, h, _cam(cams[1], 40), arr.accum[1], 12, seed=5)
    assert np.array_equal(ext.accum, want_acc) and np.array_equal(ext.rgb, want_rgb)
