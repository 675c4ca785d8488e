"""rt_camera_paths / rt_trace_paths and their device variants without a GPU: the prototypes are declared and bound, the new struct's
layout, every argument error is reported before any device call and writes nothing, the no-ops, the wrappers' shapes, and the plan of
the path kernel (tests/c/paths_plan_table.cpp over csrc/rt_paths_plan.h)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_camera_hits_host import _camera, _scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
ENTRY_POINTS = ("rt_camera_paths", "rt_camera_paths_device", "rt_trace_paths", "rt_trace_paths_device", "rt_dev_last_paths_plan")
MAX_W, MAX_H = 4, 3
FRAME = (2 * MAX_W + 1) * (2 * MAX_H + 1)
LDS_BYTES = 163840
FIELDS = ("n_vertices", "end", "colour", "first_ray", "hit_index", "strike", "colour_after", "ray_after", "summary")


def test_prototypes_struct_and_version(rt):
    from ray_tracing_fsharp_amd import _lib
    A = rt._abi
    header = open(os.path.join(ROOT, "include", "rtfs_amd.h")).read()
    assert "#define RT_ABI_VERSION 7" in header and rt.lib.rt_abi_version() == 7 == A.RT_ABI_VERSION
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header and hasattr(_lib.lib, name) and name in _lib.SIGNATURES
    assert "#define RT_PATH_SUMMARY_WORDS 16" in header and A.RT_PATH_SUMMARY_WORDS == 16
    assert (A.RT_PATH_MISS, A.RT_PATH_STOPPED, A.RT_PATH_BOUNCE_LIMIT, A.RT_PATH_NO_RAY) == (0, 1, 2, 3)
    for k, name in enumerate(("RT_PATH_MISS", "RT_PATH_STOPPED", "RT_PATH_BOUNCE_LIMIT", "RT_PATH_NO_RAY")):
        assert f"{name} = {k}" in header
    which, t = A.ABI_STRUCT_PATH_OUTPUTS, A.rt_path_outputs
    assert rt.lib.rt_abi_sizeof(which) == C.sizeof(t) == 80
    for k, (fname, _) in enumerate(t._fields_):
        assert rt.lib.rt_abi_offsetof(which, k) == getattr(t, fname).offset
    assert rt.lib.rt_abi_offsetof(which, len(t._fields_)) == C.c_size_t(-1).value
    assert [f for f, _ in t._fields_] == ["struct_size", "max_vertices"] + list(FIELDS)
    assert hasattr(rt.Scene, "cameraPaths") and hasattr(rt.Scene, "tracePaths") and hasattr(rt, "CameraPaths") and hasattr(rt, "TracePaths")
    assert rt.hooks.last_paths_plan() is None or rt.device_count() > 0


class Bufs:
    """Sentinel-filled outputs for n list entries x per samples x k records."""

    def __init__(self, rt, n, per, k, camera=True):
        slots, recs = n * per, n * per * max(k, 1)
        self.arrays = {"n_vertices": np.full(slots, 77, np.int32), "end": np.full(slots, 77, np.int32), "colour": np.full(slots * 3, 77, np.uint8),
                       "first_ray": np.full(slots * 6, 7.5), "hit_index": np.full(recs, 77, np.int32), "strike": np.full(recs * 3, 7.5),
                       "colour_after": np.full(recs * 3, 77, np.uint8), "ray_after": np.full(recs * 6, 7.5), "summary": np.full(n * 16, 77, np.int32)}
        if not camera:
            del self.arrays["first_ray"], self.arrays["summary"]
        self.out = rt._abi.rt_path_outputs(max_vertices=k, **{f: a.ctypes.data for f, a in self.arrays.items()})

    def untouched(self):
        return all((a == (7.5 if a.dtype == np.float64 else 77)).all() for a in self.arrays.values())


def _camera_calls(rt, s, cam, n, px, out, max_w=MAX_W, max_h=MAX_H, first=2, per=3, options=None):
    L = rt.lib
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None  # noqa: E731
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    c = C.byref(cam) if cam is not None else None
    o = C.byref(out) if out is not None else None
    if options is None:
        yield lambda: L.rt_camera_paths(s, c, max_w, max_h, 1, 0, n, i32(px), first, per, 0, o, None)
    yield lambda: L.rt_camera_paths_device(s, c, max_w, max_h, 1, 0, n, p(px), first, per, 0, o, None, C.byref(options) if options is not None else None, None)


def _ray_calls(rt, s, n, rays, out, depth=3, options=None):
    L = rt.lib
    f64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None  # noqa: E731
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    o = C.byref(out) if out is not None else None
    if options is None:
        yield lambda: L.rt_trace_paths(s, 0, n, f64(rays), None, 1, 0, 0, depth, 0, o, None)
    yield lambda: L.rt_trace_paths_device(s, 0, n, p(rays), None, 1, 0, 0, depth, 0, o, None, C.byref(options) if options is not None else None, None)


def test_invalid_arguments_are_refused_before_any_device_call(rt):
    A = rt._abi
    scene = _scene(rt)
    S = scene.handle
    n, per, k = 5, 3, 2
    px = np.array([0, 7, FRAME - 1, 7, 30], np.int32)
    cam = _camera(rt).to_abi()
    b = Bufs(rt, n, per, k)
    rb = Bufs(rt, n, 1, k, camera=False)
    rays = np.ones((n, 6))

    def with_cam(**kw):
        c = _camera(rt).to_abi()
        for key, v in kw.items():
            setattr(c, key, v)
        return c

    def with_out(base, **kw):
        o = A.rt_path_outputs()
        C.memmove(C.byref(o), C.byref(base), C.sizeof(o))
        for key, v in kw.items():
            setattr(o, key, v)
        return o

    nothing = A.rt_path_outputs(max_vertices=k)
    records_only_k0 = with_out(nothing, max_vertices=0, hit_index=b.arrays["hit_index"].ctypes.data)  # K == 0 ignores them: every output NULL
    calls = []
    # rt_camera_hits' refusals
    calls += list(_camera_calls(rt, None, cam, n, px, b.out))
    calls += list(_camera_calls(rt, S, None, n, px, b.out))
    calls += list(_camera_calls(rt, S, cam, n, px, b.out, max_w=0))
    calls += list(_camera_calls(rt, S, cam, n, px, b.out, max_w=40000, max_h=40000))
    calls += list(_camera_calls(rt, S, with_cam(samples_per_pixel=0), n, px, b.out))
    calls += list(_camera_calls(rt, S, with_cam(bounce_depth=-1), n, px, b.out))
    calls += list(_camera_calls(rt, S, cam, n, px, b.out, first=-1))
    calls += list(_camera_calls(rt, S, cam, n, px, b.out, per=0))
    calls += list(_camera_calls(rt, S, cam, n, px, b.out, first=7999998, per=3))
    calls += list(_camera_calls(rt, S, cam, 2**30, px, b.out, per=2))
    calls += list(_camera_calls(rt, S, cam, FRAME + 1, None, b.out))
    calls += list(_camera_calls(rt, S, cam, n, px, b.out, options=A.rt_render_options(block_threads=100)))
    calls += list(_camera_calls(rt, S, cam, n, px, b.out, options=A.rt_render_options(chunk_pixels=65)))
    calls += list(_camera_calls(rt, S, cam, n, px, b.out, options=A.rt_render_options(passes=3)))
    for entry in (-1, FRAME, -2**31, 2**31 - 1):  # a HOST list with an entry outside the frame: the host variant
        lst = px.copy()
        lst[3] = entry
        calls += list(_camera_calls(rt, S, cam, n, lst, b.out))[:1]
    # the added refusals
    calls += list(_camera_calls(rt, S, cam, n, px, None))                                                 # out NULL
    calls += list(_camera_calls(rt, S, cam, n, px, with_out(b.out, struct_size=0)))                       # another struct_size
    calls += list(_camera_calls(rt, S, cam, n, px, with_out(b.out, struct_size=C.sizeof(b.out) + 8)))
    calls += list(_camera_calls(rt, S, cam, n, px, with_out(b.out, struct_size=C.sizeof(b.out) - 8)))
    calls += list(_camera_calls(rt, S, cam, n, px, nothing))                                              # every output NULL
    calls += list(_camera_calls(rt, S, cam, n, px, records_only_k0))
    calls += list(_camera_calls(rt, S, cam, n, px, with_out(b.out, max_vertices=-1)))                     # K < 0
    calls += list(_camera_calls(rt, S, cam, 2**20, None, with_out(b.out, max_vertices=2**10), max_w=1000, max_h=1000, per=2))  # slots * K = 2^31
    calls += list(_camera_calls(rt, S, with_cam(bounce_depth=2**20 - 1), 4, None, b.out, first=0, per=2**11))  # n_samples * (depth + 1) = 2^31, with a summary
    calls += list(_ray_calls(rt, None, n, rays, rb.out))
    calls += list(_ray_calls(rt, S, n, None, rb.out))
    calls += list(_ray_calls(rt, S, n, rays, None))
    calls += list(_ray_calls(rt, S, n, rays, rb.out, depth=-1))
    calls += list(_ray_calls(rt, S, n, rays, rb.out, depth=0x1000000))
    calls += list(_ray_calls(rt, S, 2**31, rays, rb.out))
    calls += list(_ray_calls(rt, S, 2**21, rays, with_out(rb.out, max_vertices=2**10)))                   # slots * K = 2^31
    calls += list(_ray_calls(rt, S, n, rays, with_out(rb.out, first_ray=b.arrays["first_ray"].ctypes.data)))  # camera paths only
    calls += list(_ray_calls(rt, S, n, rays, with_out(rb.out, summary=b.arrays["summary"].ctypes.data)))
    calls += list(_ray_calls(rt, S, n, rays, with_out(rb.out, struct_size=4)))
    calls += list(_ray_calls(rt, S, n, rays, A.rt_path_outputs(max_vertices=1)))
    calls += list(_ray_calls(rt, S, n, rays, rb.out, options=A.rt_render_options(blocks_per_cu=9)))
    assert len(calls) == 11 * 2 + 3 + 4 + 9 * 2 + 11 * 2 + 1
    for i, call in enumerate(calls):
        assert call() == A.RT_ERR_INVALID_ARGUMENT, i
        assert rt.lib.rt_last_error()
        assert b.untouched() and rb.untouched(), i
    assert 2**20 * 2 * 2**10 == 2**31 and (2**20 - 1 + 1) * 2**11 == 2**31


def test_the_limits_themselves_are_admitted(rt):
    """slots * K == INT32_MAX-ish, n_samples * (depth + 1) just inside, K == 0 with per-slot outputs, a summary alone: past the argument
    checks, so without a GPU the call gets as far as asking for the device."""
    if rt.device_count() > 0:
        pytest.skip("a GPU is visible")
    A = rt._abi
    scene, cam = _scene(rt), _camera(rt).to_abi()
    b = Bufs(rt, 5, 3, 2)
    px = np.array([0, 7, FRAME - 1, 7, 30], np.int32)
    only_summary = A.rt_path_outputs(max_vertices=0, summary=b.arrays["summary"].ctypes.data)
    k0 = A.rt_path_outputs(max_vertices=0, end=b.arrays["end"].ctypes.data, hit_index=b.arrays["hit_index"].ctypes.data)
    for out in (b.out, only_summary, k0):
        for call in _camera_calls(rt, scene.handle, cam, 5, px, out):
            assert call() == A.RT_ERR_NO_DEVICE
    rb = Bufs(rt, 5, 1, 2, camera=False)
    for call in _ray_calls(rt, scene.handle, 5, np.ones((5, 6)), rb.out):
        assert call() == A.RT_ERR_NO_DEVICE
    assert b.untouched() and rb.untouched()


def test_an_empty_list_is_a_no_op(rt):
    A = rt._abi
    scene, cam = _scene(rt), _camera(rt).to_abi()
    L, S = rt.lib, scene.handle
    out = A.rt_path_outputs(max_vertices=3, end=1)  # (never dereferenced: no slot)
    for call in (lambda st: L.rt_camera_paths(S, C.byref(cam), MAX_W, MAX_H, 1, 0, 0, None, 0, 1, 0, C.byref(out), st),
                 lambda st: L.rt_camera_paths_device(S, C.byref(cam), MAX_W, MAX_H, 1, 0, 0, None, 0, 1, 0, C.byref(out), None, None, st),
                 lambda st: L.rt_trace_paths(S, 0, 0, None, None, 1, 0, 0, 3, 0, C.byref(out), st),
                 lambda st: L.rt_trace_paths_device(S, 0, 0, None, None, 1, 0, 0, 3, 0, C.byref(out), None, None, st)):
        assert call(None) == A.RT_OK
        st = A.rt_stats(rays=5, samples=9, pixels=4, kernel_ms=3.0)
        assert call(C.byref(st)) == A.RT_OK
        assert st.rays == 0 and st.samples == 0 and st.pixels == 0 and st.kernel_ms == 0.0
    # an empty list is still checked
    assert L.rt_camera_paths(S, C.byref(cam), MAX_W, MAX_H, 1, 0, 0, None, 0, 0, 0, C.byref(out), None) == A.RT_ERR_INVALID_ARGUMENT
    assert L.rt_camera_paths(S, C.byref(cam), MAX_W, MAX_H, 1, 0, 0, None, 0, 1, 0, None, None) == A.RT_ERR_INVALID_ARGUMENT
    res = scene.cameraPaths(MAX_W, MAX_H, _camera(rt), np.zeros(0, np.int32), n_samples=3, max_vertices=4, summary=True)
    assert res.n_vertices.shape == (0, 3) and res.colour.shape == (0, 3, 3) and res.first_ray.shape == (0, 3, 6)
    assert res.hit_index.shape == (0, 3, 4) and res.strike.shape == (0, 3, 4, 3) and res.ray_after.shape == (0, 3, 4, 6) and res.summary.shape == (0, 16)
    assert res.stats["pixels"] == 0 and res.stats is scene.last_stats
    res = scene.tracePaths(np.zeros((0, 6)), 3, max_vertices=2, records=False)
    assert res.n_vertices.shape == (0,) and res.hit_index is None and res.rng is None


def test_python_wrappers_check_and_refuse(rt):
    scene, cam = _scene(rt), _camera(rt)
    with pytest.raises(TypeError):
        scene.cameraPaths(MAX_W, MAX_H, cam, np.ones(3, np.int64))
    with pytest.raises(TypeError):
        scene.cameraPaths(MAX_W, MAX_H, cam, np.ones(3, np.int32), max_vertices=2.0)
    with pytest.raises(ValueError):
        scene.cameraPaths(MAX_W, MAX_H, cam, np.ones(3, np.int32), n=3)
    with pytest.raises(ValueError):  # options belong to the device entry
        scene.cameraPaths(MAX_W, MAX_H, cam, np.ones(3, np.int32), options=rt._abi.rt_render_options(chunk_pixels=8))
    for kw in (dict(pixels=np.array([0, FRAME, 2], np.int32)), dict(pixels=np.ones(3, np.int32), max_vertices=-1), dict(pixels=np.ones(3, np.int32), n_samples=0),
               dict(pixels=None, n=FRAME + 1)):
        with pytest.raises(rt.RtError) as e:
            scene.cameraPaths(MAX_W, MAX_H, cam, kw.pop("pixels"), **kw)
        assert e.value.code == rt._abi.RT_ERR_INVALID_ARGUMENT
    with pytest.raises(rt.RtError) as e:
        scene.tracePaths(np.ones((4, 6)), -1)
    assert e.value.code == rt._abi.RT_ERR_INVALID_ARGUMENT
    if rt.device_count() == 0:
        with pytest.raises(rt.RtError) as e:
            scene.cameraPaths(MAX_W, MAX_H, cam, None)
        assert e.value.code == rt._abi.RT_ERR_NO_DEVICE


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------
IN_ORDER = ("lds_total", "lds32_total", "n_nodes", "n_obj", "has_tex", "s_block", "s_chunk", "s_bpc", "s_yield", "s_refill", "s_passes", "s_park",
            "count", "slots", "cu_count", "per_cu")
SMALL = dict(lds_total=30000, lds32_total=20000, n_nodes=99, n_obj=52)       # LDS-resident
BIG = dict(lds_total=400000, lds32_total=300000, n_nodes=5199, n_obj=2602)   # global memory
MANY = dict(lds_total=30000, lds32_total=20000, n_nodes=99, n_obj=16384)     # fits, but past the node loop's 14-bit queue entries


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_paths") / "paths_plan_table")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-o", exe, os.path.join(HERE, "c", "paths_plan_table.cpp")])

    def plans(inputs):
        lines = ["plan " + " ".join(str(int(i.get(k, 0))) for k in IN_ORDER) for i in inputs]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [{k: int(v) for k, v in (kv.split("=") for kv in line.split())} for line in out]

    return plans


def test_the_plan_table(planner):
    cu = 256
    table = [
        # (inputs, block, grid, chunk, lds_bytes, lds)
        (dict(SMALL, slots=69864, cu_count=cu, per_cu=1), 1024, 69, 64, 20000, 1),            # fewer blocks than the device holds: what the slots need
        (dict(SMALL, slots=69864, cu_count=cu, per_cu=4, s_block=256, s_bpc=1), 256, 256, 64, 20000, 1),  # blocks_per_cu caps the occupancy
        (dict(SMALL, slots=10**7, cu_count=cu, per_cu=4, s_block=256), 256, 1024, 64, 20000, 1),
        (dict(SMALL, slots=10**7, cu_count=cu, per_cu=2, s_block=512), 1024, 512, 64, 20000, 1),  # 512 and 768 run as 1024
        (dict(SMALL, slots=10**7, cu_count=cu, per_cu=2, s_block=768, s_chunk=7), 1024, 512, 7, 20000, 1),
        (dict(SMALL, slots=10**7, cu_count=cu, per_cu=1, count=1), 1024, 256, 64, 0, 0),         # the counting variant: global memory
        (dict(BIG, slots=10**7, cu_count=cu, per_cu=1, has_tex=1), 1024, 256, 64, 0, 0),          # not resident
        (dict(MANY, slots=10**7, cu_count=cu, per_cu=1), 1024, 256, 64, 0, 0),
        (dict(BIG, slots=1, cu_count=cu, per_cu=1, s_chunk=1), 1024, 1, 1, 0, 0),
        (dict(SMALL, slots=1025, cu_count=cu, per_cu=1, s_bpc=8), 1024, 2, 64, 20000, 1),
        (dict(SMALL, slots=2**31 - 1, cu_count=304, per_cu=2, s_bpc=1), 1024, 304, 64, 20000, 1),
    ]
    got = planner([t[0] for t in table])
    for (inp, block, grid, chunk, lds_bytes, lds), g in zip(table, got):
        assert (g["error"], g["block"], g["grid"], g["chunk"], g["lds_bytes"], g["lds"]) == (0, block, grid, chunk, lds_bytes, lds), inp
        assert g["counting"] == inp.get("count", 0) and g["tex"] == inp.get("has_tex", 0) and g["slots"] == inp["slots"]
        assert g["lds_bytes"] <= LDS_BYTES and g["grid"] * g["block"] < inp["slots"] + g["block"]
    bad = planner([dict(SMALL, slots=5, cu_count=cu, per_cu=1, s_block=300), dict(SMALL, slots=5, cu_count=cu, per_cu=1, s_chunk=65)])
    assert [b["error"] for b in bad] == [1, 1]
