"""rt_render_views_extend(_device) and rt_render_views_extend_map(_device) without a GPU: they are declared and bound, every refusal comes
with its status and its message before any device call and writes nothing, the no-ops are no-ops, the Python wrappers refuse what they
can see, a C consumer links and is refused the same way, and the launch plan treats the extension of a batch as the FRAME extension of
as many pixels run by pass B's views kernel, with the workspace the batch's ordering needs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import texture_cases as tc
from test_views_host import FRAME, K, MAX_H, MAX_W, _camera, _cams, _scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("rt_render_views_extend", "rt_render_views_extend_device", "rt_render_views_extend_map", "rt_render_views_extend_map_device")
ROWS, COLS = 2 * MAX_H + 1, 2 * MAX_W + 1


def test_prototypes_and_bindings(rt):
    from ray_tracing_fsharp_amd import _lib, raytracing
    A = rt._abi
    header = open(os.path.join(ROOT, "include", "rtfs_amd.h")).read()
    assert "#define RT_ABI_VERSION 7" in header and rt.lib.rt_abi_version() == 7 == A.RT_ABI_VERSION
    for name in NAMES:
        assert f"int {name}(" in header
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES
        assert name not in raytracing._ROUTED
    assert len(raytracing._ROUTED) == 12
    # every symbol the header declares is bound
    declared = set(re.findall(r"^(?:int|int64_t|size_t|uint8_t|const char \*|void)\s*\*?(rt_\w+)\(", header, re.M))
    assert set(NAMES) <= declared and declared <= set(_lib.SIGNATURES), declared - set(_lib.SIGNATURES)
    # the device signature is the host's plus stream and options in front of stats
    for base in ("rt_render_views_extend", "rt_render_views_extend_map"):
        host, dev = _lib.SIGNATURES[base][1], _lib.SIGNATURES[base + "_device"][1]
        assert len(dev) == len(host) + 2 and dev[-3] is C.c_void_p and dev[-2] is C.POINTER(A.rt_render_options)
        for h, d in zip(host[:-1], dev[:-3]):  # (buffers: typed pointers on the host, untyped ones on the device)
            assert h is d or (d is C.c_void_p and hasattr(h, "_type_")), base
    # the argument order: rt_render_views' with the extension's extra argument where rt_render_extend(_map) puts it (behind flags)
    views = _lib.SIGNATURES["rt_render_views"][1]
    assert _lib.SIGNATURES["rt_render_views_extend"][1] == views[:9] + [C.c_int32] + views[9:]
    assert _lib.SIGNATURES["rt_render_views_extend_map"][1] == views[:9] + [C.POINTER(C.c_int32)] + views[9:]
    assert "Scene.fs:157-236" in header.split("Continuing a batch of views")[1].split("Output side")[0]


def _calls(rt, s, cams, k, accum, rgb, done=12, targets=None, mapped=False, max_w=MAX_W, max_h=MAX_H, options=None, stats=None):
    """Host and device entry point of the uniform pair (or, mapped, of the pair by map) with the same arguments."""
    L = rt.lib
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None  # noqa: E731
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)) if a is not None else None  # noqa: E731
    o = C.byref(options) if options is not None else None
    st = C.byref(stats) if stats is not None else None
    if mapped:
        if options is None:
            yield lambda: L.rt_render_views_extend_map(s, cams, k, max_w, max_h, None, 1, 0, 0, i32(targets), i32(accum), u8(rgb), st)
        yield lambda: L.rt_render_views_extend_map_device(s, cams, k, max_w, max_h, None, 1, 0, 0, p(targets), p(accum), p(rgb), None, o, st)
    else:
        if options is None:
            yield lambda: L.rt_render_views_extend(s, cams, k, max_w, max_h, None, 1, 0, 0, done, i32(accum), u8(rgb), st)
        yield lambda: L.rt_render_views_extend_device(s, cams, k, max_w, max_h, None, 1, 0, 0, done, p(accum), p(rgb), None, o, st)


def test_every_refusal_comes_before_any_device_call_with_its_message(rt):
    A = rt._abi
    scene = _scene(rt)
    S = scene.handle
    accum, rgb = np.full((K, FRAME, 4), 77, np.int32), np.full((K, FRAME, 3), 3, np.uint8)
    targets = np.full((K, FRAME), 20, np.int32)
    cams = _cams(rt)  # 20 spp
    unset = A.rt_render_options(); unset.struct_size = 0
    INV = A.RT_ERR_INVALID_ARGUMENT
    share = "the cameras of a batch must share samples_per_pixel and bounce_depth"
    cases = []
    for m in (False, True):
        kw = dict(mapped=m, targets=targets)
        cases += [  # (calls, message): check_views' own, in its order
            (_calls(rt, None, cams, K, accum, rgb, **kw), "scene is NULL"),
            (_calls(rt, S, None, K, accum, rgb, **kw), "cameras is NULL"),
            (_calls(rt, S, cams, K, None, rgb, **kw), "accum is NULL"),
            (_calls(rt, S, cams, -1, accum, rgb, **kw), "n_views must be >= 0"),
            (_calls(rt, S, _cams(rt, changed={(2, "samples_per_pixel"): 21}), K, accum, rgb, **kw), share),
            (_calls(rt, S, _cams(rt, changed={(1, "bounce_depth"): 4}), K, accum, rgb, **kw), share),
            (_calls(rt, S, cams, K, accum, rgb, max_w=20000, max_h=10000, **kw), "a batch of views holds at most INT32_MAX pixels"),
            (_calls(rt, S, _cams(rt, 1), 1, accum, rgb, max_w=1 << 20, max_h=512, **kw), "a batch of views holds at most INT32_MAX pixels"),
            (_calls(rt, S, cams, K, accum, rgb, options=A.rt_render_options(block_threads=100), **kw), "block_threads must be 0, 256, 512, 768 or 1024"),
            (_calls(rt, S, cams, K, accum, rgb, options=unset, **kw), "rt_render_options.struct_size is not set"),
        ]
    too_few = "samples_done must be >= 12 (below, firstTrial differs and Count cannot tell a stopped pixel from a finished one)"
    cases += [  # the extension's own, behind the batch's
        (_calls(rt, S, cams, K, accum, rgb, done=11), too_few),
        (_calls(rt, S, cams, K, accum, rgb, done=0), too_few),
        (_calls(rt, S, cams, K, accum, rgb, done=21), "the target samples_per_pixel is below samples_done"),
        (_calls(rt, S, cams, K, accum, rgb, mapped=True, targets=None), "targets is NULL"),
        (_calls(rt, S, _cams(rt, changed={(v, "samples_per_pixel"): 11 for v in range(K)}), K, accum, rgb, mapped=True, targets=targets),
         "a map's samples_per_pixel (the bound on every target) must be >= 12 (a buffer rendered below cannot be continued)"),
        # the batch's checks come first: a bad option beside a bad samples_done is the option's refusal
        (_calls(rt, S, cams, K, accum, rgb, done=11, options=A.rt_render_options(passes=3)), "passes must be 0 (auto), 1 (fused) or 2 (two-pass)"),
    ]
    n = 0
    for calls, message in cases:
        for call in calls:
            assert call() == INV, message
            assert rt.lib.rt_last_error().decode() == message
            assert (accum == 77).all() and (rgb == 3).all()  # nothing written
            n += 1
    assert n == 2 * (8 * 2 + 2) + 5 * 2 + 1


def test_a_scene_with_a_texture_program_is_unsupported(rt):
    from ray_tracing_fsharp_amd import texprog as T
    A = rt._abi
    tp = rt.Texture.Program(T.PX * 10.0, T.PY, T.PZ)
    objs = [tc.wear(0, rt.ParameterisedTexture.Program(1.0, 2.0, 3.0)),
            rt.Hittable.Sphere(rt.Sphere.make(rt.SphereStyle.LightSource(tp), rt.Point.make(8.0, 0.0, 0.0), 1.0))]
    scene = rt.Scene.make(objs)
    accum, rgb = np.full((K, FRAME, 4), 77, np.int32), np.full((K, FRAME, 3), 3, np.uint8)
    targets = np.full((K, FRAME), 20, np.int32)
    for m in (False, True):
        for call in _calls(rt, scene.handle, _cams(rt), K, accum, rgb, mapped=m, targets=targets):
            assert call() == A.RT_ERR_UNSUPPORTED
            assert rt.lib.rt_last_error().decode() == "a batch of views does not take a scene that holds a texture program"
            assert (accum == 77).all() and (rgb == 3).all()
    with pytest.raises(rt.RtError) as e:
        scene.extendViews(MAX_W, MAX_H, [_camera(rt)] * K, accum.reshape(K, ROWS, COLS, 4), 12)
    assert e.value.code == A.RT_ERR_UNSUPPORTED
    # an argument error is still reported first
    assert next(iter(_calls(rt, scene.handle, _cams(rt), -1, accum, rgb)))() == A.RT_ERR_INVALID_ARGUMENT


def test_the_no_ops(rt):
    A = rt._abi
    scene = _scene(rt)
    S = scene.handle
    accum, rgb = np.full((K, FRAME, 4), 77, np.int32), np.full((K, FRAME, 3), 3, np.uint8)
    n = 0
    # no views (uniform and by map), and a target equal to samples_done (the cameras stand at 20)
    for calls in (lambda st: _calls(rt, S, None, 0, None, None, stats=st), lambda st: _calls(rt, S, None, 0, None, None, mapped=True, stats=st),
                  lambda st: _calls(rt, S, _cams(rt), K, accum, rgb, done=20, stats=st)):
        for call in calls(None):
            assert call() == A.RT_OK
        st = A.rt_stats(rays=5, samples=9, pixels=4, pixels_early=2, kernel_ms=3.0)
        for call in calls(st):
            st.rays, st.samples, st.pixels, st.pixels_early, st.kernel_ms = 5, 9, 4, 2, 3.0
            assert call() == A.RT_OK
            assert st.rays == 0 and st.samples == 0 and st.pixels == 0 and st.pixels_early == 0 and st.kernel_ms == 0.0
            n += 1
    assert n == 6 and (accum == 77).all() and (rgb == 3).all()
    got = scene.extendViews(MAX_W, MAX_H, [], np.zeros((0, ROWS, COLS, 4), np.int32), 12)
    assert got.accum.shape == (0, ROWS, COLS, 4) and got.rgb.shape == (0, ROWS, COLS, 3) and got.stats["pixels"] == 0 and got.stats["samples"] == 0
    got = scene.extendViewsMap(MAX_W, MAX_H, [], np.zeros((0, ROWS, COLS, 4), np.int32), np.zeros((0, ROWS, COLS), np.int32))
    assert got.accum.shape == (0, ROWS, COLS, 4) and got.stats["pixels"] == 0
    before = np.full((2, ROWS, COLS, 4), 77, np.int32)
    got = scene.extendViews(MAX_W, MAX_H, [_camera(rt)] * 2, before, 20)  # target == samples_done: a copy comes back, untouched
    assert got.accum is not before and (got.accum == 77).all() and got.stats["samples"] == 0 and got.stats["pixels"] == 0


def test_the_wrappers_refuse_what_they_can_see(rt):
    scene, cam = _scene(rt), _camera(rt)
    acc = np.zeros((2, ROWS, COLS, 4), np.int32)
    tg = np.zeros((2, ROWS, COLS), np.int32)
    with pytest.raises(ValueError, match="one seed per camera"):
        scene.extendViews(MAX_W, MAX_H, [cam, cam], acc, 12, seeds=[1])
    with pytest.raises(ValueError, match="one seed per camera"):
        scene.extendViewsMap(MAX_W, MAX_H, [cam, cam], acc, tg, seeds=[1, 2, 3])
    with pytest.raises(ValueError, match="options apply to the device entry point"):
        scene.extendViews(MAX_W, MAX_H, [cam, cam], acc, 12, options=rt._abi.rt_render_options(passes=1))
    for bad in (acc[:1], acc.astype(np.int64), acc.reshape(2, ROWS * COLS, 4), [1, 2]):
        with pytest.raises(ValueError, match=r"accum must be an int32 array \[2, 7, 9, 4\]"):
            scene.extendViews(MAX_W, MAX_H, [cam, cam], bad, 12)
        with pytest.raises(ValueError, match=r"accum must be an int32 array \[2, 7, 9, 4\]"):
            scene.extendViewsMap(MAX_W, MAX_H, [cam, cam], bad, tg)
    for bad in (tg[:1], tg.astype(np.int64), tg.reshape(2, ROWS * COLS), None):
        with pytest.raises(ValueError, match=r"targets must be an int32 array \[2, 7, 9\]"):
            scene.extendViewsMap(MAX_W, MAX_H, [cam, cam], acc, bad)
    with pytest.raises(rt.RtError) as e:  # (the library's own refusal, through the wrapper)
        scene.extendViews(MAX_W, MAX_H, [cam, cam], acc, 11)
    assert e.value.code == rt._abi.RT_ERR_INVALID_ARGUMENT and "samples_done must be >= 12" in str(e.value)
    assert (acc == 0).all()


def test_c_program_is_refused_the_same_way(rt, tmp_path):
    """tests/c/views_extend_smoke.c from C99: it links against the library and checks refusals and no-ops only -- it launches nothing."""
    src = os.path.join(ROOT, "tests", "c", "views_extend_smoke.c")
    text = open(src).read()
    assert "hipLaunch" not in text and "rt_render_views(" not in text and "rt_render(" not in text
    exe = str(tmp_path / "views_extend_smoke")
    libdir = os.path.join(ROOT, "ray-tracing-fsharp_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-L", libdir, "-lrtfs_amd", f"-Wl,-rpath,{libdir}",
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "views extend: argument checks ok" in out.stdout


# ---- the plan ------------------------------------------------------------------------------------------------------------------
IN_ORDER = ("kind", "lds_total", "lds32_total", "n_nodes", "n_obj", "has_tex", "s_block", "s_chunk", "s_bpc", "s_yield", "s_refill", "s_passes", "s_park",
            "count", "n_views", "n_rows", "max_w", "spp", "cu_count", "per_cu", "first_sample", "map")
FRAME_KIND, VIEWS_KIND = 0, 6
SHAPES = ((64, 41, 35), (3, 33, 24), (9, 3, 2), (70, 1, 0), (1, 801, 600), (512, 41, 35), (4097, 3, 1))
PASS_WORDS = ("mode", "lds_bytes", "chunk", "park", "park_l", "park_l_lds", "lds_node_bytes", "lds_node_thr", "yield", "leaf_wait", "refill", "k", "total_waves")


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("views_extend") / "views_extend_plan_table")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-o", exe, os.path.join(HERE, "c", "views_extend_plan_table.cpp")])

    def plans(inputs):
        lines = ["plan " + " ".join(str(int(i.get(k, 0))) for k in IN_ORDER) for i in inputs]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [{k: int(v) for k, v in (kv.split("=") for kv in line.split())} for line in out]

    return plans


def _job(**kw):
    i = dict(kind=VIEWS_KIND, lds_total=136000, lds32_total=89000, n_nodes=969, n_obj=488, has_tex=0, n_views=64, n_rows=41, max_w=35, spp=100, cu_count=256, per_cu=1,
             first_sample=12, map=0)
    i.update(kw)
    return i


def test_the_extension_of_a_batch_is_the_frame_extension_of_as_many_pixels(planner):
    jobs = []
    for spp in (13, 40, 100, 500):
        for k, n_rows, max_w in SHAPES:
            for mapped in (0, 1):
                for first in ((12,) if mapped else (12, spp - 1)):
                    for extra in ({}, {"s_passes": 1}, {"s_chunk": 7}, {"s_chunk": 1}, {"s_block": 256}, {"count": 1}, {"has_tex": 1},
                                  {"lds32_total": 400000, "lds_total": 600000}):
                        jobs.append(_job(spp=spp, n_views=k, n_rows=n_rows, max_w=max_w, map=mapped, first_sample=first, **extra))
    views = planner(jobs)
    frames = planner([dict(j, kind=FRAME_KIND) for j in jobs])
    for j, v, f in zip(jobs, views, frames):
        px = j["n_views"] * j["n_rows"] * (2 * j["max_w"] + 1)
        assert v["error"] == 0 and f["error"] == 0 and v["extend"] == 1 and v["pixels"] == f["pixels"] == px
        # two passes forced (whatever `passes` asks), pass A's words zero: nothing of it is launched
        assert v["two_pass"] == 1 and f["two_pass"] == 1
        assert all(v[f"A_{w}"] == 0 for w in PASS_WORDS + ("grid", "views")), j
        # pass B: the views kernel, mode 2, or 9 under a map
        assert v["B_views"] == 1 and f["B_views"] == 0 and v["B_mode"] == f["B_mode"] == (9 if j["map"] else 2)
        # every pass-B word, the pass decision and the pools are the FRAME extension's
        same = ["q_lds", "q_count", "q_block", "q_mode", "q_tex", "q_lds_bytes", "two_pass", "list", "pool", "waves", "B_grid"] + [f"B_{w}" for w in PASS_WORDS]
        assert {w: v[w] for w in same} == {w: f[w] for w in same}, j
        assert v["B_grid"] == j["cu_count"] * j["per_cu"] and v["list"] == (px * 4 + 15) // 16 * 16
        # the workspace the ordering needs: pairs for every batch pixel, a key per (view, cost bucket) and view_end; the frame's has neither
        buckets = 64 if j["n_views"] <= 4096 else 1
        assert v["pairs"] == (px * 8 + 15) // 16 * 16 and v["sort"] == (j["n_views"] * (buckets + 1) * 4 + 15) // 16 * 16
        assert f["pairs"] == 0 and f["sort"] == 0


def test_a_batchs_extension_runs_at_blocks_of_256_or_1024(planner):
    for mapped in (0, 1):
        got = planner([_job(s_block=b, map=mapped) for b in (0, 256, 512, 768, 1024)])
        assert [g["q_block"] for g in got] == [g["B_block"] for g in got] == [1024, 256, 1024, 1024, 1024]
        at_1024 = planner([_job(kind=FRAME_KIND, s_block=1024, map=mapped)])[0]
        for g in (got[2], got[3]):  # 512 and 768 run as 1024: the frame extension's words at 1024
            assert {w: g[f"B_{w}"] for w in PASS_WORDS} == {w: at_1024[f"B_{w}"] for w in PASS_WORDS}


def test_a_fresh_batch_and_a_frames_extension_are_planned_as_before(planner):
    """With the extension's fields unused a batch keeps its plan (pairs, keys and view_end as tests/test_views_host.py holds them), and a
    FRAME's extension still has no pairs and nothing to sort."""
    fresh = planner([_job(first_sample=0, s_passes=2)])[0]
    assert fresh["extend"] == 0 and fresh["two_pass"] == 1 and fresh["A_grid"] > 0 and fresh["pairs"] == (64 * 41 * 71 * 8 + 15) // 16 * 16
    frame = planner([_job(kind=FRAME_KIND)])[0]
    assert frame["extend"] == 1 and frame["pairs"] == 0 and frame["sort"] == 0 and frame["B_views"] == 0
