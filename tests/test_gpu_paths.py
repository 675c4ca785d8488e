"""Scene.cameraPaths / Scene.tracePaths -- rt_camera_paths, rt_trace_paths, their device variants, paths_kernel -- against the answer
composed from the oracle's pieces (tests/path_cases.py; itself held to the oracle's PixelStats, the oracle's traceRay and the literal
restatement by tests/test_path_cases.py).  Every comparison is device against composer, bit for bit, NaNs by position."""
import ctypes as C
import dataclasses
import functools
import subprocess

import numpy as np
import pytest

import path_cases as pc
import scenes

pytestmark = pytest.mark.gpu

SEED = pc.FRAME_SEED
GUARD = 64  # sentinel bytes in front of and behind every raw buffer


@functools.lru_cache(maxsize=None)
def _scene(rt, name, walk_tree=None):
    return rt.Scene.make(pc.frame(name).objs, walk_tree=walk_tree)


def _np(a):
    return None if a is None else (a if isinstance(a, np.ndarray) else a.cpu().numpy())


def _gather(p: pc.Paths, n_px_frame_samples, px, first, per):
    """The frame fixture's slots for list px and samples first .. first + per - 1, as Paths over the list's slots."""
    spp = n_px_frame_samples
    idx = (np.asarray(px, np.int64)[:, None] * spp + np.arange(first, first + per)[None, :]).reshape(-1)
    return pc.Paths(*[a[idx] for a in p[:9]], p.counters)


def _check(got, want: pc.Paths, k, what=()):
    """Every output of a CameraPaths / TracePaths against the composer's, records cut or padded to k."""
    n = len(want.n_vertices)
    assert np.array_equal(_np(got.n_vertices).reshape(n), want.n_vertices), what
    assert np.array_equal(_np(got.end).reshape(n), want.end), what
    assert np.array_equal(_np(got.colour).reshape(n, 3), want.colour), what
    if getattr(got, "first_ray", None) is not None:
        assert pc.same_f64(_np(got.first_ray).reshape(n, 6), want.first_ray), what
    if got.hit_index is not None:
        hi, sk, ca, ra = pc.truncate(want, k)
        assert np.array_equal(_np(got.hit_index).reshape(n, k), hi), what
        assert pc.same_f64(_np(got.strike).reshape(n, k, 3), sk), what
        assert np.array_equal(_np(got.colour_after).reshape(n, k, 3), ca), what
        assert pc.same_f64(_np(got.ray_after).reshape(n, k, 6), ra), what


def _want_summary(want: pc.Paths, n, per):
    return pc.summary(want.n_vertices, want.end, want.colour, want.colour_after[:, 0], n, per)


def _opts(rt, **kw):
    return rt._abi.rt_render_options(**kw)


# ---- 1. the whole all_materials frame: lanes are refilled ---------------------------------------------------------------------------
@pytest.mark.parametrize("counters", [False, True])
def test_whole_frame_every_output(rt, orc, counters):
    f = pc.frame("all_materials")
    scene = _scene(rt, "all_materials")
    n = (2 * f.w + 1) * (2 * f.h + 1)
    per, want = f.spp, f.paths
    for _ in range(4):
        got = scene.cameraPaths(f.w, f.h, f.cam, None, n_samples=per, max_vertices=f.depth + 1, summary=True, seed=SEED, tensors=True, counters=counters,
                                options=_opts(rt, block_threads=256, blocks_per_cu=1))
        plan = rt.hooks.last_paths_plan()
        if plan["slots"] > plan["grid"] * plan["block"]:
            break
        per *= 2  # a device with more lanes than slots: more samples, until lanes have to be refilled
        want = pc.camera_paths(orc, f.oracle, f.cam_abi, f.w, f.h, SEED, np.arange(n), 0, per)
    assert plan["slots"] == n * per > plan["grid"] * plan["block"] and plan["block"] == 256 and plan["counting"] == int(counters)
    _check(got, want, f.depth + 1)
    assert np.array_equal(_np(got.summary), _want_summary(want, n, per))
    assert got.stats["pixels"] == n and got.stats["samples"] == n * per
    if counters:
        assert (got.stats["rays"], got.stats["prim_tests"], got.stats["reflections"]) == (want.counters[0], want.counters[2], want.counters[3])
        assert got.stats["reflections"] == int(want.n_vertices.sum())
    # the path colours of the samples a render takes are the render's PixelStats, from the device
    acc = _np(scene.renderPixels(f.w, f.h, f.cam, np.arange(n, dtype=np.int32), seed=SEED).accum).astype(np.int64)
    col = _np(got.colour).astype(np.int64)[:, :f.spp]
    taken = np.arange(f.spp)[None, :] < acc[:, 0:1]
    assert np.array_equal((col * taken[:, :, None]).sum(1), acc[:, 1:])


# ---- 2. truncation, with sentinel bytes around every buffer --------------------------------------------------------------------------
def _guarded(nbytes):
    raw = np.full(nbytes + 2 * GUARD, 0xA5, np.uint8)
    return raw, raw[GUARD:GUARD + nbytes]


def _raw_camera_paths(rt, scene, f, px, first, per, k, summary=True):
    """rt_camera_paths on guarded host buffers -> dict of arrays; asserts the guards."""
    A = rt._abi
    n = len(px) if px is not None else (2 * f.w + 1) * (2 * f.h + 1)
    slots, recs = n * per, n * per * max(k, 1)  # (K == 0: the record buffers are given all the same, and must stay untouched)
    sizes = {"n_vertices": slots * 4, "end": slots * 4, "colour": slots * 3, "first_ray": slots * 48, "hit_index": recs * 4, "strike": recs * 24,
             "colour_after": recs * 3, "ray_after": recs * 48, "summary": n * 64 if summary else 0}
    bufs = {name: _guarded(sz) for name, sz in sizes.items()}
    out = A.rt_path_outputs(max_vertices=k, **{name: (b[1].ctypes.data if sizes[name] else None) for name, b in bufs.items()})
    st = A.rt_stats()
    pxp = px.ctypes.data_as(C.POINTER(C.c_int32)) if px is not None else None
    rc = rt.lib.rt_camera_paths(scene.handle, C.byref(f.cam_abi), f.w, f.h, SEED, 0, n, pxp, first, per, 0, C.byref(out), C.byref(st))
    assert rc == A.RT_OK, rt.lib.rt_last_error()
    for name, (raw, view) in bufs.items():
        assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + sizes[name]:] == 0xA5).all(), name
    dt = {"n_vertices": np.int32, "end": np.int32, "colour": np.uint8, "first_ray": np.float64, "hit_index": np.int32, "strike": np.float64,
          "colour_after": np.uint8, "ray_after": np.float64, "summary": np.int32}
    return {name: bufs[name][1].view(dt[name]) for name in bufs}


@pytest.mark.parametrize("k", [0, 1, 4])
def test_truncation_keeps_the_per_slot_outputs_and_the_first_records(rt, k):
    f = pc.frame("all_materials")
    n = (2 * f.w + 1) * (2 * f.h + 1)
    got = _raw_camera_paths(rt, _scene(rt, "all_materials"), f, None, 0, f.spp, k)
    want = f.paths
    assert np.array_equal(got["n_vertices"], want.n_vertices) and np.array_equal(got["end"], want.end)  # not capped by K
    assert np.array_equal(got["colour"].reshape(-1, 3), want.colour) and pc.same_f64(got["first_ray"].reshape(-1, 6), want.first_ray)
    assert np.array_equal(got["summary"].reshape(n, 16), _want_summary(want, n, f.spp))
    if k == 0:
        for name in ("hit_index", "strike", "colour_after", "ray_after"):
            assert (got[name].view(np.uint8) == 0xA5).all(), name  # K == 0 ignores the per-record pointers
    else:
        hi, sk, ca, ra = pc.truncate(want, k)
        assert np.array_equal(got["hit_index"].reshape(-1, k), hi) and pc.same_f64(got["strike"].reshape(-1, k, 3), sk)
        assert np.array_equal(got["colour_after"].reshape(-1, k, 3), ca) and pc.same_f64(got["ray_after"].reshape(-1, k, 6), ra)
        assert (want.n_vertices > k).any()


# ---- 3. sizes around a wave -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 7, 499])
def test_wave_edges(rt, orc, first):
    f = pc.frame("all_materials")
    scene = _scene(rt, "all_materials")
    cols = 2 * f.w + 1
    for count in (1, 63, 64, 65, 129):
        for px, per in ((np.array([20 * cols + 35], np.int32), count), ((np.arange(count, dtype=np.int32) * 17 + 400), 1)):
            want = pc.camera_paths(orc, f.oracle, f.cam_abi, f.w, f.h, SEED, px, first, per)
            got = scene.cameraPaths(f.w, f.h, f.cam, px, sample_first=first, n_samples=per, max_vertices=5, summary=True, seed=SEED)
            _check(got, want, 5, (count, per))
            assert np.array_equal(got.summary, _want_summary(want, len(px), per)), (count, per)
            assert got.n_vertices.shape == (len(px), per) and got.strike.shape == (len(px), per, 5, 3)


# ---- 4. lists ---------------------------------------------------------------------------------------------------------------------------
def test_lists_in_any_order_with_duplicates(rt):
    f = pc.frame("all_materials")
    scene = _scene(rt, "all_materials")
    n = (2 * f.w + 1) * (2 * f.h + 1)
    idx = np.random.default_rng(4).permutation(np.arange(0, n, 5, dtype=np.int32))
    shuffled = np.concatenate([idx, idx[:40], np.array([0, n - 1, 0], np.int32)]).astype(np.int32)
    for px, first, per in ((shuffled, 3, 9), (np.arange(100, 700, dtype=np.int32), 0, 24)):
        got = scene.cameraPaths(f.w, f.h, f.cam, px, sample_first=first, n_samples=per, max_vertices=6, summary=True, seed=SEED)
        want = _gather(f.paths, f.spp, px, first, per)
        _check(got, want, 6)
        assert np.array_equal(got.summary, _want_summary(want, len(px), per))  # duplicates: their own sixteen words each
    a = scene.cameraPaths(f.w, f.h, f.cam, None, n_samples=2, max_vertices=3, seed=SEED)
    b = scene.cameraPaths(f.w, f.h, f.cam, np.arange(n, dtype=np.int32), n_samples=2, max_vertices=3, seed=SEED)
    for x, y in zip(a[:8], b[:8]):
        assert x.tobytes() == y.tobytes()


# ---- 5. routes ----------------------------------------------------------------------------------------------------------------------------
def _route_case(name):
    f = pc.frame(name)
    n = (2 * f.w + 1) * (2 * f.h + 1)
    if name == "small_final":  # LDS-resident, depth 50: 200 pixels x 8 samples
        return f, np.random.default_rng(6).choice(n, 200, replace=False).astype(np.int32), 8
    return f, np.arange(n, dtype=np.int32), f.spp  # many_spheres: the whole frame x 12, from global memory


@pytest.mark.parametrize("name,resident", [("small_final", 1), ("many_spheres", 0)])
@pytest.mark.parametrize("variant", ["plain", "tuned", "reference"])
def test_routes(rt, name, resident, variant):
    f, px, per = _route_case(name)
    want = _gather(f.paths, f.spp, px, 0, per)
    scene = _scene(rt, name) if variant == "plain" else rt.Scene.make(f.objs, walk_tree="reference" if variant == "reference" else None)
    if variant == "tuned":
        scene.tune(f.w, f.h, f.cam, seed=SEED, device=0)
    for counters in (False, True):
        got = scene.cameraPaths(f.w, f.h, f.cam, px, n_samples=per, max_vertices=f.depth + 1, summary=True, seed=SEED, counters=counters)
        plan = rt.hooks.last_paths_plan()
        assert plan["lds_resident"] == (0 if counters else resident) and plan["counting"] == int(counters)
        _check(got, want, f.depth + 1, (name, variant, counters))
        assert np.array_equal(got.summary, _want_summary(want, len(px), per))
    if variant == "reference" and len(px) == len(f.paths.n_vertices) // f.spp:  # the oracle's tree: its box tests too
        assert [got.stats[k] for k in ("rays", "aabb_tests", "prim_tests", "reflections")] == f.paths.counters.tolist()


def test_textured_scene(rt, orc):
    objs, cam, w, h = scenes.earth_thumb(scenes.golden("earthmap_rgb")["rgb"])
    cam = dataclasses.replace(cam, BounceDepth=8)
    px = np.random.default_rng(9).choice((2 * w + 1) * (2 * h + 1), 100, replace=False).astype(np.int32)
    want = pc.camera_paths(orc, orc.OracleScene(objs), cam.to_abi(), w, h, SEED, px, 0, 4)
    scene = rt.Scene.make(objs)
    for counters in (False, True):
        got = scene.cameraPaths(w, h, cam, px, n_samples=4, max_vertices=9, seed=SEED, counters=counters)
        assert rt.hooks.last_paths_plan()["textured"] == 1
        _check(got, want, 9)
    assert (want.n_vertices >= 1).any()


def test_a_scene_without_a_dome_misses(rt):
    objs, cam, w, h = pc.lights_scene()
    want = pc.lights_paths()
    got = rt.Scene.make(objs).cameraPaths(w, h, cam, None, n_samples=cam.SamplesPerPixel, max_vertices=2, summary=True, seed=SEED)
    _check(got, want, 2)
    assert (got.end == pc.MISS).any() and np.array_equal(got.summary, _want_summary(want, (2 * w + 1) * (2 * h + 1), cam.SamplesPerPixel))


def test_a_viewport_through_the_eye_has_no_ray(rt):
    objs, cam, w, h = pc.no_ray_scene()
    want = pc.no_ray_camera_paths()
    got = rt.Scene.make(objs).cameraPaths(w, h, cam, None, n_samples=cam.SamplesPerPixel, max_vertices=3, summary=True, seed=SEED)
    _check(got, want, 3)
    assert (got.end == pc.NO_RAY).any() and np.array_equal(got.summary, _want_summary(want, 25, cam.SamplesPerPixel))


@pytest.mark.parametrize("seed", range(12))
def test_random_scenes(rt, orc, seed):
    objs, cam, w, h = scenes.random_scene(700 + seed)
    n = (2 * w + 1) * (2 * h + 1)
    want = pc.camera_paths(orc, orc.OracleScene(objs), cam.to_abi(), w, h, SEED, np.arange(n), 0, 4)
    k = cam.BounceDepth + 1
    for walk_tree in (None, "reference"):
        scene = rt.Scene.make(objs, walk_tree=walk_tree)
        for counters in (False, True):
            got = scene.cameraPaths(w, h, cam, None, n_samples=4, max_vertices=k, summary=True, seed=SEED, counters=counters)
            _check(got, want, k, (seed, walk_tree, counters))
            assert np.array_equal(got.summary, _want_summary(want, n, 4))


# ---- 6. settings never change a result ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["all_materials", "many_spheres"])
def test_settings_never_change_a_result(rt, name):
    import torch
    f = pc.frame(name)
    n = (2 * f.w + 1) * (2 * f.h + 1)
    px = np.arange(0, n, 3, dtype=np.int32)
    want = _gather(f.paths, f.spp, px, 0, f.spp)
    scene, tpx = _scene(rt, name), torch.from_numpy(px).cuda()
    for kw in (dict(block_threads=256), dict(block_threads=512), dict(block_threads=1024), dict(chunk_pixels=1), dict(chunk_pixels=7),
               dict(chunk_pixels=64), dict(blocks_per_cu=1), dict(block_threads=256, chunk_pixels=7, blocks_per_cu=1)):
        got = scene.cameraPaths(f.w, f.h, f.cam, tpx, n_samples=f.spp, max_vertices=4, summary=True, seed=SEED, options=_opts(rt, **kw))
        plan = rt.hooks.last_paths_plan()
        assert plan["block"] == (256 if kw.get("block_threads") == 256 else 1024) and plan["chunk"] == kw.get("chunk_pixels", 64)
        _check(got, want, 4, kw)
        assert np.array_equal(_np(got.summary), _want_summary(want, len(px), f.spp)), kw


# ---- 7. ray paths -----------------------------------------------------------------------------------------------------------------------
def test_ray_paths(rt, orc):
    rays, states, want = pc.ray_fixture()
    f = pc.frame("all_materials")
    scene = _scene(rt, "all_materials")
    for counters in (False, True):
        got = scene.tracePaths(rays, pc.RAY_DEPTH, rng=states, max_vertices=pc.RAY_DEPTH + 1, counters=counters)
        _check(got, want, pc.RAY_DEPTH + 1)
        assert np.array_equal(got.rng, want.rng) and (got.end == pc.NO_RAY).sum() == 4
    assert [got.stats[k] for k in ("rays", "prim_tests", "reflections")] == want.counters[[0, 2, 3]].tolist()
    assert got.stats["pixels"] == got.stats["samples"] == len(rays)
    colour, adv = scene.traceRays(rays, pc.RAY_DEPTH, rng=states)  # rt_trace_rays on the device: the same colours and states
    assert np.array_equal(got.colour, colour) and np.array_equal(got.rng, adv)
    keyed = pc.ray_paths(orc, f.oracle, rays, 3, rng=None, seed=77, stream_base=1 << 33, sample=5)
    got = scene.tracePaths(rays, 3, seed=77, stream_base=1 << 33, sample=5, max_vertices=2)
    _check(got, keyed, 2)
    assert got.rng is None and np.array_equal(got.colour, scene.traceRays(rays, 3, seed=77, stream_base=1 << 33, sample=5)[0])


# ---- 8. the summary ---------------------------------------------------------------------------------------------------------------------
def test_summary_is_the_reduction_and_the_renders_pixel_stats(rt):
    f = pc.frame("all_materials")
    scene = _scene(rt, "all_materials")
    n = (2 * f.w + 1) * (2 * f.h + 1)
    px = np.concatenate([np.arange(0, n, 2), np.array([7, 7, 7])]).astype(np.int32)
    got = scene.cameraPaths(f.w, f.h, f.cam, px, n_samples=f.spp, max_vertices=1, summary=True, seed=SEED)
    assert np.array_equal(got.summary, pc.summary(got.n_vertices, got.end, got.colour, got.colour_after[:, :, 0], len(px), f.spp))  # of its own outputs
    assert np.array_equal(got.summary, _want_summary(_gather(f.paths, f.spp, px, 0, f.spp), len(px), f.spp))                          # of the composer's
    only = scene.cameraPaths(f.w, f.h, f.cam, px, n_samples=f.spp, max_vertices=0, records=False, first_ray=False, summary=True, seed=SEED)
    assert np.array_equal(only.summary, got.summary) and only.hit_index is None
    acc = scene.renderPixels(f.w, f.h, f.cam, px, seed=SEED).accum
    full = acc[:, 0] == f.spp
    assert full.any() and (~full).any() and np.array_equal(got.summary[full, 12:16], acc[full])
    assert np.array_equal(got.summary[-1], got.summary[-2]) and np.array_equal(got.summary[-1], got.summary[-3])


# ---- 9. the device variants ---------------------------------------------------------------------------------------------------------------
def test_device_variants_on_a_stream_and_a_malformed_list(rt):
    import torch
    A = rt._abi
    f = pc.frame("all_materials")
    scene = _scene(rt, "all_materials")
    n = (2 * f.w + 1) * (2 * f.h + 1)
    px = np.arange(0, n, 4, dtype=np.int32)
    want = _gather(f.paths, f.spp, px, 2, 5)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = scene.cameraPaths(f.w, f.h, f.cam, torch.from_numpy(px).cuda(), sample_first=2, n_samples=5, max_vertices=4, summary=True, seed=SEED, stats=False)
        rays, states, rwant = pc.ray_fixture()
        rgot = scene.tracePaths(torch.from_numpy(rays.copy()).cuda(), pc.RAY_DEPTH, rng=torch.from_numpy(states.view(np.int32).copy()).cuda(), max_vertices=3, stats=False)
    stream.synchronize()
    assert got.stats is None and scene.last_stats is None
    _check(got, want, 4)
    assert np.array_equal(_np(got.summary), _want_summary(want, len(px), 5))
    _check(rgot, rwant, 3)
    assert np.array_equal(_np(rgot.rng).view(np.uint32), rwant.rng)
    # a device list with an entry outside the frame: nothing is written; reported when stats is given
    for entry in (-1, n, 2**31 - 1):
        bad = px.copy()
        bad[len(bad) // 2] = entry
        tpx = torch.from_numpy(bad).cuda()
        slots = len(bad) * 3
        bufs = {"n_vertices": torch.full((slots,), 0x5A5A5A5A, dtype=torch.int32, device="cuda"), "end": torch.full((slots,), 0x5A5A5A5A, dtype=torch.int32, device="cuda"),
                "colour": torch.full((slots, 3), 0x5A, dtype=torch.uint8, device="cuda"), "first_ray": torch.full((slots, 6), 7.5, dtype=torch.float64, device="cuda"),
                "hit_index": torch.full((slots, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda"), "strike": torch.full((slots, 2, 3), 7.5, dtype=torch.float64, device="cuda"),
                "colour_after": torch.full((slots, 2, 3), 0x5A, dtype=torch.uint8, device="cuda"), "ray_after": torch.full((slots, 2, 6), 7.5, dtype=torch.float64, device="cuda"),
                "summary": torch.full((len(bad), 16), 0x5A5A5A5A, dtype=torch.int32, device="cuda")}
        before = {k: v.clone() for k, v in bufs.items()}
        out = A.rt_path_outputs(max_vertices=2, **{k: v.data_ptr() for k, v in bufs.items()})
        st = A.rt_stats()
        for stats in (None, C.byref(st)):
            rc = rt.lib.rt_camera_paths_device(scene.handle, C.byref(f.cam_abi), f.w, f.h, SEED, 0, len(bad), tpx.data_ptr(), 0, 3, 0, C.byref(out),
                                               torch.cuda.current_stream().cuda_stream, None, stats)
            torch.cuda.synchronize()
            assert rc == (A.RT_OK if stats is None else A.RT_ERR_INVALID_ARGUMENT), entry
            for k in bufs:
                assert torch.equal(bufs[k], before[k]), (entry, k)
        assert b"outside the frame" in rt.lib.rt_last_error()


def test_c_program_traces_paths_on_the_gpu(rt, orc, tmp_path):
    """tests/c/paths_smoke.c's one launch of each family, against the composer."""
    from test_paths_smoke import build_paths_smoke, smoke_case
    out = subprocess.run([build_paths_smoke(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(line.split(":", 1) for line in out.stdout.splitlines() if ":" in line)
    cam_want, ray_want = smoke_case(rt, orc)
    assert [int(x) for x in lines["camera n_vertices"].split()] == cam_want.n_vertices.tolist()
    assert [int(x) for x in lines["camera end"].split()] == cam_want.end.tolist()
    assert [int(x) for x in lines["camera colour"].split()] == cam_want.colour.reshape(-1).tolist()
    assert [int(x) for x in lines["rays n_vertices"].split()] == ray_want.n_vertices.tolist()
    assert [int(x) for x in lines["rays colour"].split()] == ray_want.colour.reshape(-1).tolist()
