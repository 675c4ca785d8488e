"""rt_render_views and rt_render_views_device without a GPU: they are declared and bound, every refusal the header lists comes with its
status and its message before any device call and writes nothing, n_views = 0 is a no-op, the Python wrapper refuses what it can see,
and the launch plan treats a batch of views as a frame of as many pixels run by the views kernels -- while the plans of every other
kind stay what they were."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import texture_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
MAX_W, MAX_H = 4, 3
FRAME = (2 * MAX_W + 1) * (2 * MAX_H + 1)
K = 3


def _scene(rt):
    P, S, H, Tex, Px = rt.Point.make, rt.SphereStyle, rt.Hittable, rt.Texture.Colour, rt.Pixel
    return rt.Scene.make([H.Sphere(rt.Sphere.make(S.LambertReflection(0.8, Tex(Px(200, 100, 50))), P(0.0, 0.0, 3.0), 1.0))])


def _camera(rt, spp=20, depth=3):
    cam = rt.Camera.makeBasic(spp, 1.0, 9.0 / 7.0, rt.Point.make(0.0, 0.0, -1.0), rt.Vector.unitise(rt.Vector.make(0.0, 0.0, 1.0)), rt.Vector.make(0.0, 1.0, 0.0))
    return dataclasses.replace(cam, BounceDepth=depth)


def _cams(rt, k=K, changed=None):
    """k cameras as the C array the entry points take; changed: (view, field) -> value"""
    arr = (rt._abi.rt_camera * k)(*[_camera(rt).to_abi() for _ in range(k)])
    for (v, field), value in (changed or {}).items():
        setattr(arr[v], field, value)
    return arr


def test_prototypes_and_version(rt):
    from ray_tracing_fsharp_amd import _lib, raytracing
    header = open(os.path.join(ROOT, "include", "rtfs_amd.h")).read()
    assert "#define RT_ABI_VERSION 7" in header
    for name in ("rt_render_views", "rt_render_views_device"):
        assert f"int {name}(" in header
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES
    assert rt.lib.rt_abi_version() == 7 == rt._abi.RT_ABI_VERSION
    assert len(raytracing._ROUTED) == 12 and "rt_render_views" not in raytracing._ROUTED  # (Scene.renderViews calls the pair itself)
    assert "6 batch of views" in header  # rt_dev_last_launch_plan's kinds
    assert "Scene.fs:157-236" in header and "RT_ERR_UNSUPPORTED: the batch kernels" in header


def _calls(rt, s, cams, k, accum, rgb, max_w=MAX_W, max_h=MAX_H, seeds=None, options=None):
    """Both entry points with the same arguments (the host variant takes no options)."""
    L = rt.lib
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None  # noqa: E731
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)) if a is not None else None  # noqa: E731
    o = C.byref(options) if options is not None else None
    if options is None:
        yield lambda: L.rt_render_views(s, cams, k, max_w, max_h, seeds, 1, 0, 0, i32(accum), u8(rgb), None)
    yield lambda: L.rt_render_views_device(s, cams, k, max_w, max_h, seeds, 1, 0, 0, p(accum), p(rgb), None, o, None)


def test_every_refusal_comes_before_any_device_call_with_its_message(rt):
    A = rt._abi
    scene = _scene(rt)
    S = scene.handle
    accum, rgb = np.full((K, FRAME, 4), 77, np.int32), np.full((K, FRAME, 3), 3, np.uint8)
    cams = _cams(rt)
    unset = A.rt_render_options(); unset.struct_size = 0
    INV = A.RT_ERR_INVALID_ARGUMENT
    share = "the cameras of a batch must share samples_per_pixel and bounce_depth"
    cases = [  # (calls, status, message)
        (_calls(rt, None, cams, K, accum, rgb), INV, "scene is NULL"),
        (_calls(rt, S, None, K, accum, rgb), INV, "cameras is NULL"),
        (_calls(rt, S, cams, K, None, rgb), INV, "accum is NULL"),
        (_calls(rt, S, cams, -1, accum, rgb), INV, "n_views must be >= 0"),
        (_calls(rt, S, cams, -2**31, accum, rgb), INV, "n_views must be >= 0"),
        (_calls(rt, S, cams, K, accum, rgb, max_w=0), INV, "max_width_coord and max_height_coord must be positive"),
        (_calls(rt, S, cams, K, accum, rgb, max_h=-2), INV, "max_width_coord and max_height_coord must be positive"),
        (_calls(rt, S, cams, K, accum, rgb, max_w=(1 << 20) + 1), INV, "image too large"),
        # any camera rt_render rejects, wherever it stands in the batch
        (_calls(rt, S, _cams(rt, changed={(0, "samples_per_pixel"): 0}), K, accum, rgb), INV, "samples_per_pixel must be >= 1"),
        (_calls(rt, S, _cams(rt, changed={(2, "samples_per_pixel"): 8000001}), K, accum, rgb), INV, "samples_per_pixel too large for int32 sums (255*spp)"),
        (_calls(rt, S, _cams(rt, changed={(1, "bounce_depth"): -1}), K, accum, rgb), INV, "bounce_depth must be >= 0"),
        (_calls(rt, S, _cams(rt, changed={(2, "bounce_depth"): 0x1000000}), K, accum, rgb), INV, "bounce_depth too large"),
        # cameras that do not all share the sample count and the depth
        (_calls(rt, S, _cams(rt, changed={(2, "samples_per_pixel"): 21}), K, accum, rgb), INV, share),
        (_calls(rt, S, _cams(rt, changed={(1, "bounce_depth"): 4}), K, accum, rgb), INV, share),
        # n_views * rows * cols > INT32_MAX: 3 views of 40001 x 20001, and one pixel too many
        (_calls(rt, S, cams, K, accum, rgb, max_w=20000, max_h=10000), INV, "a batch of views holds at most INT32_MAX pixels"),
        (_calls(rt, S, _cams(rt, 1), 1, accum, rgb, max_w=1 << 20, max_h=512), INV, "a batch of views holds at most INT32_MAX pixels"),
        # bad options
        (_calls(rt, S, cams, K, accum, rgb, options=A.rt_render_options(block_threads=100)), INV, "block_threads must be 0, 256, 512, 768 or 1024"),
        (_calls(rt, S, cams, K, accum, rgb, options=unset), INV, "rt_render_options.struct_size is not set"),
        (_calls(rt, S, cams, K, accum, rgb, options=A.rt_render_options(passes=3)), INV, "passes must be 0 (auto), 1 (fused) or 2 (two-pass)"),
        (_calls(rt, S, cams, K, accum, rgb, options=A.rt_render_options(chunk_pixels=65)), INV, "chunk_pixels must be in [0, 64]"),
    ]
    n = 0
    for calls, status, message in cases:
        for call in calls:
            assert call() == status, message
            assert rt.lib.rt_last_error().decode() == message
            assert (accum == 77).all() and (rgb == 3).all()  # nothing written
            n += 1
    assert n == 16 * 2 + 4
    assert 3 * 40001 * 20001 > 2**31 - 1 and (2 * (1 << 20) + 1) * 1025 > 2**31 - 1 >= K * FRAME


def test_a_scene_with_a_texture_program_is_unsupported(rt):
    from ray_tracing_fsharp_amd import texprog as T
    A = rt._abi
    tp = rt.Texture.Program(T.PX * 10.0, T.PY, T.PZ)
    objs = [tc.wear(0, rt.ParameterisedTexture.Program(1.0, 2.0, 3.0)),
            rt.Hittable.Sphere(rt.Sphere.make(rt.SphereStyle.LightSource(tp), rt.Point.make(8.0, 0.0, 0.0), 1.0))]
    scene = rt.Scene.make(objs)
    accum, rgb = np.full((K, FRAME, 4), 77, np.int32), np.full((K, FRAME, 3), 3, np.uint8)
    for call in _calls(rt, scene.handle, _cams(rt), K, accum, rgb):
        assert call() == A.RT_ERR_UNSUPPORTED
        assert rt.lib.rt_last_error().decode() == "a batch of views does not take a scene that holds a texture program"
        assert (accum == 77).all() and (rgb == 3).all()
    with pytest.raises(rt.RtError) as e:
        scene.renderViews(MAX_W, MAX_H, [_camera(rt)] * 2)
    assert e.value.code == A.RT_ERR_UNSUPPORTED
    # an argument error is still reported first
    assert next(iter(_calls(rt, scene.handle, _cams(rt), -1, accum, rgb)))() == A.RT_ERR_INVALID_ARGUMENT


def test_no_views_is_a_no_op(rt):
    A = rt._abi
    scene = _scene(rt)
    L, S = rt.lib, scene.handle
    for call in _calls(rt, S, None, 0, None, None):
        assert call() == A.RT_OK
    for call in (lambda st: L.rt_render_views(S, None, 0, MAX_W, MAX_H, None, 1, 0, 0, None, None, C.byref(st)),
                 lambda st: L.rt_render_views_device(S, None, 0, MAX_W, MAX_H, None, 1, 0, 0, None, None, None, None, C.byref(st))):
        st = A.rt_stats(rays=5, samples=9, pixels=4, kernel_ms=3.0)
        assert call(st) == A.RT_OK
        assert st.rays == 0 and st.samples == 0 and st.pixels == 0 and st.kernel_ms == 0.0
    got = scene.renderViews(MAX_W, MAX_H, [])
    assert got.accum.shape == (0, 2 * MAX_H + 1, 2 * MAX_W + 1, 4) and got.rgb.shape == (0, 2 * MAX_H + 1, 2 * MAX_W + 1, 3)
    assert got.stats["pixels"] == 0 and got.stats["samples"] == 0


def test_the_wrapper_refuses_what_it_can_see(rt):
    scene, cam = _scene(rt), _camera(rt)
    with pytest.raises(ValueError, match="one seed per camera"):
        scene.renderViews(MAX_W, MAX_H, [cam, cam], seeds=[1])
    with pytest.raises(ValueError, match="options apply to the device entry point"):
        scene.renderViews(MAX_W, MAX_H, [cam], options=rt._abi.rt_render_options(passes=1))
    with pytest.raises(ValueError, match="accum must be a contiguous int32 tensor"):
        scene.renderViews(MAX_W, MAX_H, [cam], accum=np.zeros((1, 7, 9, 4), np.int32))
    with pytest.raises(rt.RtError) as e:  # (the library's own refusal, through the wrapper)
        scene.renderViews(MAX_W, MAX_H, [cam, dataclasses.replace(cam, SamplesPerPixel=21)])
    assert e.value.code == rt._abi.RT_ERR_INVALID_ARGUMENT and "share samples_per_pixel" in str(e.value)


# ---- the plan ------------------------------------------------------------------------------------------------------------------
IN_ORDER = ("kind", "lds_total", "lds32_total", "n_nodes", "n_obj", "has_tex", "s_block", "s_chunk", "s_bpc", "s_yield", "s_refill", "s_passes", "s_park",
            "count", "n_views", "n_rows", "max_w", "spp", "cu_count", "per_cu")
FRAME_KIND, VIEWS_KIND = 0, 6


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("views") / "views_plan_table")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-o", exe, os.path.join(HERE, "c", "views_plan_table.cpp")])

    def plans(inputs):
        lines = ["plan " + " ".join(str(int(i.get(k, 0))) for k in IN_ORDER) for i in inputs]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [{k: int(v) for k, v in (kv.split("=") for kv in line.split())} for line in out]

    return plans


def _job(**kw):
    i = dict(kind=VIEWS_KIND, lds_total=136000, lds32_total=89000, n_nodes=969, n_obj=488, has_tex=0, n_views=64, n_rows=41, max_w=35, spp=100, cu_count=256, per_cu=1)
    i.update(kw)
    return i


def _units(n_views, ppv, chunk):
    return n_views * -(-ppv // chunk)


def test_a_batch_is_planned_as_a_frame_of_as_many_pixels_and_runs_the_views_kernels(planner):
    jobs = []
    for spp in (1, 9, 12, 40, 100, 500):
        for k, n_rows, max_w in ((64, 41, 35), (3, 33, 24), (9, 3, 2), (70, 1, 0), (1, 801, 600), (512, 41, 35)):
            for extra in ({}, {"s_passes": 1}, {"s_passes": 2}, {"s_chunk": 7}, {"s_block": 256}, {"count": 1}, {"has_tex": 1}, {"lds32_total": 400000, "lds_total": 600000}):
                jobs.append(_job(spp=spp, n_views=k, n_rows=n_rows, max_w=max_w, **extra))
    views = planner(jobs)
    frames = planner([dict(j, kind=FRAME_KIND) for j in jobs])
    seen_two = set()
    for j, v, f in zip(jobs, views, frames):
        ppv = j["n_rows"] * (2 * j["max_w"] + 1)
        assert v["error"] == 0 and v["pixels"] == f["pixels"] == j["n_views"] * ppv
        passes = "AB" if v["two_pass"] else "F"
        seen_two.add(v["two_pass"])
        # the views kernels are chosen, for every pass; a frame never gets them
        assert all(v[f"{p}_views"] == 1 for p in passes) and all(f[f"{p}_views"] == 0 for p in ("AB" if f["two_pass"] else "F"))
        # the pass decision, the modes, the unit sizes, the LDS words, the pools, the workspace: the frame's
        same = ["q_lds", "q_count", "q_block", "q_mode", "q_tex", "q_lds_bytes", "two_pass", "pairs", "list"]
        if v["two_pass"]:
            same += ["pool", "waves"]  # (sized by the full grid; a fused launch sizes both by its own grid: below)
        for p in passes:
            same += [f"{p}_{w}" for w in ("mode", "lds_bytes", "chunk", "park", "park_l", "park_l_lds", "lds_node_bytes", "lds_node_thr", "yield", "leaf_wait",
                                          "refill", "k", "total_waves")]
        assert {w: v[w] for w in same} == {w: f[w] for w in same}, j
        assert v["q_mode"] == 0 and (not v["two_pass"] or (v["A_mode"], v["B_mode"]) == (1, 2))
        # the grid: sized by the units of rt_views_plan.h (every view ends with a short unit), capped by the full grid as the frame's is
        full = j["cu_count"] * j["per_cu"]
        wpb = v["q_block"] // 64
        first = "A" if v["two_pass"] else "F"
        assert v[f"{first}_grid"] == min(full, -(-_units(j["n_views"], ppv, v[f"{first}_chunk"]) // wpb)), j
        assert v[f"{first}_grid"] >= f[f"{first}_grid"]
        if not v["two_pass"]:
            assert v["waves"] == v["F_grid"] * wpb and f["waves"] == f["F_grid"] * wpb and v["pool"] * f["F_grid"] == f["pool"] * v["F_grid"]
        if v["two_pass"]:
            assert v["B_grid"] == f["B_grid"] == full
            buckets = 64 if j["n_views"] <= 4096 else 1
            assert v["sort"] == (j["n_views"] * (buckets + 1) * 4 + 15) // 16 * 16
    assert seen_two == {0, 1}


def test_a_batch_runs_at_blocks_of_256_or_1024(planner):
    got = planner([_job(s_block=b) for b in (0, 256, 512, 768, 1024)])
    assert [g["q_block"] for g in got] == [1024, 256, 1024, 1024, 1024]
    frames = planner([_job(kind=FRAME_KIND, s_block=b) for b in (0, 256, 512, 768, 1024)])
    assert [g["q_block"] for g in frames] == [1024, 256, 512, 768, 1024]  # a frame's own blocks are untouched


def test_plans_of_all_other_kinds_are_untouched():
    """The recorded plans of every other kind are compared word for word by tests/test_launch_plan*.py, test_extend_host.py,
    test_pixels_host.py and test_camera_hits_host.py, which this change leaves as they are; here: the planner's text still says that a job
    is a batch only when its kind is VIEWS, and the table of modes is not grown."""
    plan = open(os.path.join(ROOT, "ray-tracing-fsharp_amd", "csrc", "rt_launch_plan.h")).read()
    assert "enum Kind { FRAME, TRACE, HIT, FOOTPRINTS, PIXELS, CAMERA_HITS, VIEWS }" in plan
    assert "bool views() const { return kind == VIEWS; }" in plan
    modes = open(os.path.join(ROOT, "ray-tracing-fsharp_amd", "csrc", "rt_modes.h")).read()
    assert "MODE_COUNT = 15" in modes and "VIEWS" not in modes
