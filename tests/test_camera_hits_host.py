"""rt_camera_hits / rt_camera_hits_device without a GPU.  First the yardstick itself: tests/camera_hit_cases.py composes the expected
answer from the oracle's pieces, and is held here to the oracle's own Scene.traceOnce (through whole-frame renders of a scene of light
sources) and to the literal restatement of the F# lines.  Then the library: the prototypes are declared and bound, every argument
error is reported before any device call and writes nothing, the no-ops, the wrapper's refusals, the C consumer's host half, and the
launch plan of the camera-hit job (tests/c/camera_hits_plan_table.cpp)."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import camera_hit_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
ENTRY_POINTS = ("rt_camera_hits", "rt_camera_hits_device")
MAX_W, MAX_H = 4, 3
FRAME = (2 * MAX_W + 1) * (2 * MAX_H + 1)
LDS_BYTES = 163840


# ---- the composer, held to the oracle and to the literal restatement ---------------------------------------------------------------
def _lights(rt):
    """Light sources only, distinct non-black colours: bounded spheres, an unbounded sphere and a plane, with sky left over."""
    P, S, PS, H, Tex, Px = rt.Point.make, rt.SphereStyle, rt.InfinitePlaneStyle, rt.Hittable, rt.Texture.Colour, rt.Pixel
    unit = lambda x, y, z: rt.Vector.unitise(rt.Vector.make(x, y, z))  # noqa: E731
    objs = [H.Sphere(rt.Sphere.make(S.LightSource(Tex(Px(200, 10, 10))), P(-1.2, 0.2, 3.0), 0.8)),
            H.Sphere(rt.Sphere.make(S.LightSource(Tex(Px(10, 200, 10))), P(0.6, 0.0, 2.5), 0.5)),
            H.Sphere(rt.Sphere.make(S.LightSource(Tex(Px(10, 10, 200))), P(1.5, 0.9, 4.0), 0.7)),
            H.Sphere(rt.Sphere.make(S.LightSource(Tex(Px(220, 220, 30))), P(0.4, 0.3, 5.0), 1.6)),  # partly behind the others
            H.UnboundedSphere(rt.Sphere.make(S.LightSource(Tex(Px(30, 220, 220))), P(-2.5, 2.0, 6.0), 1.5)),
            H.InfinitePlane(rt.InfinitePlane.make(PS.LightSource(Tex(Px(120, 60, 240))), P(0.0, -1.0, 0.0), unit(0.0, 1.0, 0.0)))]
    colours = np.array([[200, 10, 10], [10, 200, 10], [10, 10, 200], [220, 220, 30], [30, 220, 220], [120, 60, 240]], np.int32)
    return objs, colours


def _basic_camera(rt, spp, aspect, depth=3, focal=1.0):
    cam = rt.Camera.makeBasic(spp, focal, aspect, rt.Point.make(0.0, 0.5, -1.0), rt.Vector.unitise(rt.Vector.make(0.0, 0.0, 1.0)), rt.Vector.make(0.0, 1.0, 0.0))
    return dataclasses.replace(cam, BounceDepth=depth)


def test_the_composer_is_the_oracles_trace_once(rt, orc):
    """At one sample per pixel Scene.renderPixel takes sample 0 alone (firstTrial = 0: Count = 1), and in a scene of light sources the
    sample's colour is the colour of the object its camera ray hits, or Black: the oracle's frame gives hit_index for every pixel."""
    objs, colours = _lights(rt)
    w, h = 17, 10  # 35 x 21
    cam = _basic_camera(rt, 1, 35.0 / 21.0)
    o = orc.OracleScene(objs)
    for seed in (0, 9):
        acc, _, _ = o.render_rows(w, h, cam.to_abi(), seed=seed, threads=4)
        acc = acc.reshape(-1, 4)
        assert (acc[:, 0] == 1).all()
        want = cases.compose(orc, o, cam.to_abi(), w, h, seed, np.arange(35 * 21), 0, 1)
        hit = want.hit[:, 0]
        assert (hit >= -1).all() and set(hit.tolist()) == {-1, 0, 1, 2, 3, 4, 5}  # every object and the sky are seen
        expect = np.where((hit >= 0)[:, None], colours[np.maximum(hit, 0)], 0)
        assert np.array_equal(acc[:, 1:], expect)
        assert not np.isnan(want.strike[hit >= 0]).any() and np.isnan(want.strike[hit < 0]).all() and not np.isnan(want.rays).any()


def test_the_composer_is_the_literal_restatement(rt, orc):
    import fsharp_literal as L
    from test_oracle_vs_literal import literal_camera, to_literal
    objs, _ = _lights(rt)
    w, h = 2, 1  # 5 x 3
    cam = _basic_camera(rt, 7, 5.0 / 3.0, focal=3.0)  # (a narrow view: the bounded spheres fill a frame this coarse)
    lits = to_literal(objs)
    for i, d in enumerate(lits):
        d["index"] = i
    scene, lcam, stream_for = L.scene_make(lits), literal_camera(cam), L.make_stream_for(11)
    first, per = 3, 4
    want = cases.compose(orc, orc.OracleScene(objs), cam.to_abi(), w, h, 11, np.arange(15), first, per)
    seen = set()
    for g in range(15):
        r, c = divmod(g, 5)
        row, col = h - r - 1, c - w
        for k in range(per):
            rand = stream_for(g, first + k)
            r1, r2 = rand.GetTwo()                                                     # Scene.fs:129
            landingPoint = ((float(col) + r1) * lcam["vw"]) / float(w)                 # Scene.fs:131-132
            pointOnXAxis = L.walk_along(L.Ray(lcam["xo"], lcam["xd"]), landingPoint)
            walkDistance = ((float(row) + r2) * lcam["vh"]) / float(h)                 # Scene.fs:136-137
            endPoint = L.walk_along_ray(pointOnXAxis, lcam["yd"], walkDistance)
            ray = L.ray_make_prime(lcam["eye"], L.v_diff(endPoint, lcam["eye"]))       # Scene.fs:142-143
            assert ray is not None
            assert cases.same_f64(want.rays[g, k], list(ray.Origin) + list(ray.Vector))
            things = L.hit_object(scene, ray)
            if things is None:
                assert want.hit[g, k] == -1 and np.isnan(want.strike[g, k]).all()
            else:
                assert want.hit[g, k] == things[0]["index"] and cases.same_f64(want.strike[g, k], things[1])
            seen.add(int(want.hit[g, k]))
    assert len(seen) >= 4 and seen & {0, 1, 2, 3} and seen & {4, 5}  # through the tree and through the unbounded objects


# ---- the library ---------------------------------------------------------------------------------------------------------------------
def _scene(rt):
    P, S, H, Tex, Px = rt.Point.make, rt.SphereStyle, rt.Hittable, rt.Texture.Colour, rt.Pixel
    return rt.Scene.make([H.Sphere(rt.Sphere.make(S.LambertReflection(0.8, Tex(Px(200, 100, 50))), P(0.0, 0.0, 3.0), 1.0))])


def _camera(rt, spp=20, depth=3):
    return _basic_camera(rt, spp, 9.0 / 7.0, depth)


def test_prototypes_and_version(rt):
    from ray_tracing_fsharp_amd import _lib
    header = open(os.path.join(ROOT, "include", "rtfs_amd.h")).read()
    assert "#define RT_ABI_VERSION 7" in header
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES
    assert rt.lib.rt_abi_version() == 7 == rt._abi.RT_ABI_VERSION
    assert "5 camera hits" in header  # rt_dev_last_launch_plan's kinds
    assert "Scene.fs:129-143" in header and "Scene.fs:62-91" in header
    assert hasattr(rt.Scene, "cameraHits") and hasattr(rt, "CameraHits")


def _calls(rt, s, cam, n, px, hit, strike, rays, max_w=MAX_W, max_h=MAX_H, first=2, per=3, options=None):
    """The two entry points with the same arguments (the host variant takes no options)."""
    L = rt.lib
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None  # noqa: E731
    f64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None  # noqa: E731
    c = C.byref(cam) if cam is not None else None
    o = C.byref(options) if options is not None else None
    if options is None:
        yield lambda: L.rt_camera_hits(s, c, max_w, max_h, 1, 0, n, i32(px), first, per, 0, i32(hit), f64(strike), f64(rays), None)
    yield lambda: L.rt_camera_hits_device(s, c, max_w, max_h, 1, 0, n, p(px), first, per, 0, p(hit), p(strike), p(rays), None, o, None)


def test_invalid_arguments_are_refused_before_any_device_call(rt):
    A = rt._abi
    scene = _scene(rt)
    n, per = 5, 3
    px = np.array([0, 7, FRAME - 1, 7, 30], np.int32)
    hit, strike, rays = np.full((n, per), 77, np.int32), np.full((n, per, 3), 7.5), np.full((n, per, 6), 7.5)
    S = scene.handle
    cam = _camera(rt).to_abi()
    bad = A.rt_render_options(block_threads=100)
    unset = A.rt_render_options(); unset.struct_size = 0

    def with_cam(**kw):
        c = _camera(rt).to_abi()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    a = (n, px, hit, strike, rays)
    cases_ = []
    cases_ += list(_calls(rt, None, cam, *a))                                    # NULL scene
    cases_ += list(_calls(rt, S, None, *a))                                      # NULL camera
    cases_ += list(_calls(rt, S, cam, *a, max_w=0))                              # geometry
    cases_ += list(_calls(rt, S, cam, *a, max_h=-2))
    cases_ += list(_calls(rt, S, cam, *a, max_w=(1 << 20) + 1))
    cases_ += list(_calls(rt, S, cam, *a, max_w=40000, max_h=40000))             # a frame of more than INT32_MAX pixels
    cases_ += list(_calls(rt, S, cam, *a, max_w=1 << 20, max_h=512))             # ... just above: 2097153 * 1025
    cases_ += list(_calls(rt, S, with_cam(samples_per_pixel=0), *a))             # camera: rt_render's checks
    cases_ += list(_calls(rt, S, with_cam(samples_per_pixel=8000001), *a))
    cases_ += list(_calls(rt, S, with_cam(bounce_depth=-1), *a))
    cases_ += list(_calls(rt, S, with_cam(bounce_depth=0x1000000), *a))
    cases_ += list(_calls(rt, S, cam, *a, first=-1))                             # the sample range
    cases_ += list(_calls(rt, S, cam, *a, per=0))
    cases_ += list(_calls(rt, S, cam, *a, per=-4))
    cases_ += list(_calls(rt, S, cam, *a, first=7999998, per=3))                 # first + per = 8000001
    cases_ += list(_calls(rt, S, cam, *a, first=2**31 - 1, per=2**31 - 1))
    cases_ += list(_calls(rt, S, cam, 2**31, px, hit, strike, rays, per=1))      # n * n_samples > INT32_MAX
    cases_ += list(_calls(rt, S, cam, 2**30, px, hit, strike, rays, per=2))
    cases_ += list(_calls(rt, S, cam, 2**63, px, hit, strike, rays, per=2))      # (a product that wraps in 64 bits)
    cases_ += list(_calls(rt, S, cam, 715827883, px, hit, strike, rays, per=3))  # 2^31 + 1
    cases_ += list(_calls(rt, S, cam, n, px, None, strike, rays))                # NULL hit_index with work to do
    cases_ += list(_calls(rt, S, cam, FRAME + 1, None, hit, strike, rays))       # no list, more entries than the frame has pixels
    assert len(cases_) == 22 * 2
    cases_ += list(_calls(rt, S, cam, *a, options=bad))                          # settings out of range
    cases_ += list(_calls(rt, S, cam, *a, options=unset))                        # struct_size not set
    cases_ += list(_calls(rt, S, cam, *a, options=A.rt_render_options(passes=3)))
    cases_ += list(_calls(rt, S, cam, *a, options=A.rt_render_options(chunk_pixels=65)))
    # a HOST list with an entry outside the frame: the host variant
    for entry in (-1, FRAME, -2**31, 2**31 - 1):
        lst = px.copy()
        lst[3] = entry
        cases_ += list(_calls(rt, S, cam, n, lst, hit, strike, rays))[:1]
    assert len(cases_) == 44 + 4 + 4
    for i, call in enumerate(cases_):
        assert call() == A.RT_ERR_INVALID_ARGUMENT, i
        assert rt.lib.rt_last_error()
        assert (hit == 77).all() and (strike == 7.5).all() and (rays == 7.5).all()  # nothing written
    assert 8000000 == 7999998 + 2 and 715827883 * 3 == 2**31 + 1 and 2**30 * 2 > 2**31 - 1


def test_the_limits_themselves_are_admitted(rt):
    """sample_first + n_samples == 8000000, n == rows*cols without a list, NULL strike and rays_out: past the argument checks, so
    without a GPU the call gets as far as asking for the device."""
    if rt.device_count() > 0:
        pytest.skip("a GPU is visible")
    A = rt._abi
    scene, cam = _scene(rt), _camera(rt).to_abi()
    hit = np.full((FRAME, 2), 77, np.int32)
    i32 = hit.ctypes.data_as(C.POINTER(C.c_int32))
    assert rt.lib.rt_camera_hits(scene.handle, C.byref(cam), MAX_W, MAX_H, 1, 0, FRAME, None, 7999998, 2, 0, i32, None, None, None) == A.RT_ERR_NO_DEVICE
    assert (hit == 77).all()


def test_an_empty_list_is_a_no_op(rt):
    A = rt._abi
    scene, cam = _scene(rt), _camera(rt).to_abi()
    for call in _calls(rt, scene.handle, cam, 0, None, None, None, None):
        assert call() == A.RT_OK
    L, S = rt.lib, scene.handle
    for call in (lambda st: L.rt_camera_hits(S, C.byref(cam), MAX_W, MAX_H, 1, 0, 0, None, 0, 1, 0, None, None, None, C.byref(st)),
                 lambda st: L.rt_camera_hits_device(S, C.byref(cam), MAX_W, MAX_H, 1, 0, 0, None, 0, 1, 0, None, None, None, None, None, C.byref(st))):
        st = A.rt_stats(rays=5, samples=9, pixels=4, kernel_ms=3.0)
        assert call(st) == A.RT_OK
        assert st.rays == 0 and st.samples == 0 and st.pixels == 0 and st.kernel_ms == 0.0
    res = scene.cameraHits(MAX_W, MAX_H, _camera(rt), np.zeros(0, np.int32), n_samples=3)
    assert res.hit_index.shape == (0, 3) and res.hit_index.dtype == np.int32
    assert res.strike.shape == (0, 3, 3) and res.rays.shape == (0, 3, 6) and res.strike.dtype == res.rays.dtype == np.float64
    assert res.stats["pixels"] == 0 and res.stats is scene.last_stats
    res = scene.cameraHits(MAX_W, MAX_H, _camera(rt), None, n=0, strike=False, rays=False)
    assert res.hit_index.shape == (0, 1) and res.strike is None and res.rays is None
    # an empty list is still checked: a bad sample range is refused
    assert L.rt_camera_hits(S, C.byref(cam), MAX_W, MAX_H, 1, 0, 0, None, 0, 0, 0, None, None, None, None) == A.RT_ERR_INVALID_ARGUMENT


def test_without_a_gpu_the_query_fails_loudly(rt):
    if rt.device_count() > 0:
        pytest.skip("a GPU is visible")
    scene = _scene(rt)
    for px in (np.array([0, 5, 9], np.int32), None):
        with pytest.raises(rt.RtError) as e:
            scene.cameraHits(MAX_W, MAX_H, _camera(rt), px)
        assert e.value.code == rt._abi.RT_ERR_NO_DEVICE


def test_python_wrapper_checks_shapes_and_dtypes(rt):
    scene, cam = _scene(rt), _camera(rt)
    for bad in (np.ones(3, np.int64), np.ones(3, np.uint32), np.ones(3, np.float64), [0, 1, 2]):
        with pytest.raises(TypeError):
            scene.cameraHits(MAX_W, MAX_H, cam, bad)
    for bad in (np.ones((3, 1), np.int32), np.ones((2, 2), np.int32), np.array(3, np.int32)):
        with pytest.raises(ValueError):
            scene.cameraHits(MAX_W, MAX_H, cam, bad)
    with pytest.raises(ValueError):  # options belong to the device entry
        scene.cameraHits(MAX_W, MAX_H, cam, np.ones(3, np.int32), options=rt._abi.rt_render_options(chunk_pixels=8))
    with pytest.raises(ValueError):  # n is for pixels=None
        scene.cameraHits(MAX_W, MAX_H, cam, np.ones(3, np.int32), n=3)
    with pytest.raises(TypeError):
        scene.cameraHits(MAX_W, MAX_H, cam, np.ones(3, np.int32), n_samples=2.0)
    # the library's own refusals arrive as RtError
    refused = [dict(pixels=np.array([0, -1, 2], np.int32)), dict(pixels=np.array([0, FRAME, 2], np.int32)), dict(pixels=None, n=FRAME + 1),
               dict(pixels=np.ones(3, np.int32), sample_first=-1), dict(pixels=np.ones(3, np.int32), n_samples=0),
               dict(pixels=np.ones(3, np.int32), sample_first=7999999, n_samples=2), dict(pixels=None, n=FRAME, n_samples=2**31 // FRAME + 1)]
    for kw in refused:
        with pytest.raises(rt.RtError) as e:
            scene.cameraHits(MAX_W, MAX_H, cam, kw.pop("pixels"), **kw)
        assert e.value.code == rt._abi.RT_ERR_INVALID_ARGUMENT


def build_camera_hits_smoke(tmp_path):
    exe = str(tmp_path / "camera_hits_smoke")
    libdir = os.path.join(ROOT, "ray-tracing-fsharp_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "camera_hits_smoke.c"),
                           "-L", libdir, "-lrtfs_amd", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    return exe


def test_c_program_checks_the_camera_hit_arguments(rt, tmp_path):
    """tests/c/camera_hits_smoke.c from C99: the argument checks hold without a GPU (with one, test_gpu_camera_hits compares what its
    one launch prints with the oracle)."""
    out = subprocess.run([build_camera_hits_smoke(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "camera hits: argument checks ok" in out.stdout


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
IN_ORDER = ("kind", "lds_total", "lds32_total", "n_nodes", "n_obj", "has_tex", "s_block", "s_chunk", "s_bpc", "s_yield", "s_refill",
            "s_passes", "s_park", "count", "log", "n_rows", "max_w", "spp", "n", "cu_count", "per_cu", "first_sample")
HIT, CAMERA_HITS = 2, 5
SMALL = dict(lds_total=30000, lds32_total=20000, n_nodes=99, n_obj=52)          # LDS-resident
TIGHT = dict(lds_total=140000, lds32_total=138000, n_nodes=969, n_obj=487)      # resident with 16-entry units; 64-entry units do not fit
BIG = dict(lds_total=400000, lds32_total=300000, n_nodes=5199, n_obj=2602)      # global memory


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_camera_hits") / "camera_hits_plan_table")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-o", exe, os.path.join(HERE, "c", "camera_hits_plan_table.cpp")])

    def plans(inputs):
        lines = ["plan " + " ".join(str(int(i.get(k, 0))) for k in IN_ORDER) for i in inputs]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [{k: int(v) for k, v in (kv.split("=") for kv in line.split())} for line in out]

    return plans


def test_the_other_kinds_are_planned_as_recorded(planner):
    """With the new kind unused the probe reproduces tests/golden/launch_plans.json word for word (as launch_plan_table.cpp does)."""
    import json
    with open(os.path.join(HERE, "golden", "launch_plans.json")) as f:
        table = json.load(f)["rows"]
    got = planner([dict(r["in"], first_sample=0) for r in table])
    assert len(table) > 100 and all(r["out"] == g for r, g in zip(table, got))


def test_camera_hits_plan(planner):
    """For LDS-resident and global scenes, n_samples in {1, 12, 500}, both variants, every block and unit setting and list lengths from
    1 to a frame: one launch of mode 14 whose LDS bytes fit, whose scratch is 6 words per entry of a unit, which parks nothing, and whose
    grid is that of the rt_hit_objects job of the same ray count."""
    seen = {"lds": set(), "chunk": set(), "grid": set()}
    for scene in (SMALL, TIGHT, BIG):
        for count in (0, 1):
            for per in (1, 12, 500):
                for block in (0, 256, 512, 768, 1024):
                    for chunk in (0, 1, 7, 64):
                        for n in (1, 63, 64, 65, 1001, 19999, 1201 * 801):
                            if n * per > 2**31 - 1:
                                continue
                            base = dict(scene, count=count, s_block=block, s_chunk=chunk, cu_count=256, per_cu=2)
                            cam, hit = planner([dict(base, kind=CAMERA_HITS, n=n, spp=per, first_sample=37), dict(base, kind=HIT, n=n * per)])
                            what = (scene["n_obj"], count, per, block, chunk, n)
                            assert cam["two_pass"] == 0 and cam["error"] == 0 and cam["q_mode"] == cam["F_mode"] == 14 and cam["q_tex"] == 0, what
                            assert cam["q_block"] == hit["q_block"] == (256 if block == 256 else 1024), what
                            assert cam["q_lds"] == hit["q_lds"] and cam["q_count"] == count, what  # residency is the render's decision, as for a ray list
                            assert scene is TIGHT or cam["q_lds"] == (1 if scene is SMALL else 0), what
                            assert cam["F_lds_bytes"] <= LDS_BYTES and cam["q_lds_bytes"] == cam["F_lds_bytes"], what
                            assert cam["F_grid"] == hit["F_grid"] > 0 and cam["waves"] == hit["waves"], what
                            assert cam["F_park"] == cam["F_park_l"] == cam["F_park_l_lds"] == cam["pool"] == 0, what
                            assert 1 <= cam["F_chunk"] <= 64 and (chunk == 0 or cam["F_chunk"] == chunk), what
                            waves = cam["q_block"] // 64
                            image = 0 if not cam["q_lds"] else (scene["lds_total"] if count else scene["lds32_total"])
                            assert cam["F_lds_bytes"] == image + waves * 6 * cam["F_chunk"] * 4 + cam["F_lds_node_bytes"], what
                            assert (cam["F_lds_node_bytes"] > 0) == (not cam["q_lds"] and not count), what  # the timed hybrid keeps the tree's top in LDS
                            for k in ("F_yield", "F_leaf_wait", "F_refill", "F_lds_node_thr"):
                                assert cam[k] == hit[k], what
                            seen["lds"].add(cam["q_lds"]); seen["chunk"].add(cam["F_chunk"]); seen["grid"].add(cam["F_grid"])
    # the default unit: about a wave's worth of items -- 64 entries at one sample, 6 at twelve, 1 at five hundred -- narrower where the
    # scene leaves the LDS no room
    pick = lambda scene, per, count=0: planner([dict(scene, kind=CAMERA_HITS, n=5000, spp=per, count=count, cu_count=256, per_cu=2)])[0]["F_chunk"]  # noqa: E731
    assert [pick(SMALL, p) for p in (1, 2, 12, 63, 64, 500)] == [64, 32, 6, 2, 1, 1]
    assert pick(TIGHT, 1) == 64 and pick(TIGHT, 1, count=1) == 32 and pick(TIGHT, 12, count=1) == 6 and pick(BIG, 1) == 64
    assert seen["lds"] == {0, 1} and len(seen["chunk"]) >= 5 and len(seen["grid"]) >= 5
