"""Surface records without a GPU.  First the yardstick: tests/surface_cases.py composes the expected answer from the oracle's pieces, and
is held here to the line-by-line restatement of Sphere.reflection / InfinitePlane.reflection on White rays, shown to catch the mistakes a
kernel of this kind makes (seeded mutants), and its case set held to the coverage it claims (conditions, with the census of three camera
frames asserted so that a changed scene cannot quietly empty a class).  Then the library: prototypes, every refusal before any device
call, the limits admitted, n = 0, the loud failure without a GPU, the wrapper's shape and dtype checks, and the C consumer's host half."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import camera_hit_cases as chc
import fsharp_literal as L
import reflection_cases as rc
import scenes
import surface_cases as sc
import texture_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("normal", "surface_origin", "cap_band", "plane", "ordinary")
WITNESSES = ("tex", "planes")
SEED = 5


# ---- the shared case set -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def witness(orc, kind, cluster=False):
    objs = rc.witness(kind, cluster)
    return objs, orc.OracleScene(objs), sc.SceneTable(objs)


@functools.lru_cache(maxsize=None)
def frame(orc, name):
    """(objs, camera, w, h, OracleScene, SceneTable, camera_hit_cases.compose of sample 0 of every pixel at seed 5)."""
    if name == "all_materials":
        objs, cam, w, h = scenes.all_materials()
    elif name == "mostly_textured":
        objs, cam, w, h = texture_cases.mostly_textured_scene()
    elif name == "earth_thumb":
        objs, cam, w, h = scenes.earth_thumb(scenes.golden("earthmap_rgb")["rgb"])
    else:
        from test_camera_hits_host import _basic_camera, _lights
        objs, (w, h) = _lights(rc.rt)[0], (17, 10)
        cam = _basic_camera(rc.rt, 1, 35.0 / 21.0)
    osc = orc.OracleScene(objs)
    hits = chc.compose(orc, osc, cam.to_abi(), w, h, SEED, np.arange((2 * w + 1) * (2 * h + 1)), 0, 1)
    return objs, cam, w, h, osc, sc.SceneTable(objs), hits


def frame_surfaces(orc, name, mutant=None):
    _, _, _, _, osc, table, hits = frame(orc, name)
    return sc.compose(orc, osc, table, hits.hit.reshape(-1), hits.strike.reshape(-1, 3), hits.rays.reshape(-1, 6), mutant=mutant)


@functools.lru_cache(maxsize=None)
def raw_roots(orc):
    arrays, hit, strike, rays = sc.raw_roots_scene()
    _, osc = scenes.raw_scene_pair(orc, *arrays)
    return arrays, osc, sc.SceneTable(arrays=arrays), hit, strike, rays


# ---- the composer against the literal restatement -------------------------------------------------------------------------------------
def _literal_record(s, ray, strike):
    """(normal or None, inside, colour, tint) of one slot, statement for statement Sphere.fs:150-200 / InfinitePlane.fs:43-99."""
    light = {"Ray": L.Ray(tuple(ray[:3]), tuple(ray[3:])), "Colour": (255, 255, 255)}
    rand = L.FloatProducer(123456789, 362436069, 521288629, 88675123)
    if s["kind"] == "plane":
        colour = L.texture_colour_at(strike, s["tex"]) if "tex" in s else s["rgb"]
        got = L.plane_reflection(s, light, strike, rand)
        return s["normal"], False, colour, light["Colour"] if got is None else got
    centre, radius = s["centre"], s["radius"]
    flipped = L.f_compare(radius, 0.0) == "Less"
    normal = L.ray_make_prime(strike, L.v_diff(strike, centre))
    d = L.v_diff(centre, light["Ray"].Origin)
    c = L.f_compare(L.v_dot(d, d), radius * radius)
    inside = (c in ("Equal", "Less")) != flipped
    n = None if normal is None else (L.v_scale(-1.0, normal.Vector) if inside else normal.Vector)
    if s["style"] == "LightSourceCap":
        lower = centre[0] + (radius - (radius / 4.0))
        colour = s["rgb"] if L.f_compare(strike[0], lower) == "Greater" else (0, 0, 0)
    else:
        colour = L.texture_colour_at(strike, s["tex"])
    if normal is None:
        return None, inside, colour, None
    got = L.sphere_reflection(s, light, strike, rand)
    return n, inside, colour, light["Colour"] if got is None else got


@pytest.mark.parametrize("kind", WITNESSES)
@pytest.mark.parametrize("cls", CLASSES)
def test_the_composer_is_the_literal_restatement(orc, kind, cls):
    from test_oracle_vs_literal import to_literal
    objs, osc, table = witness(orc, kind)
    v = rc.vertices(orc, cls).spread(120)
    want = sc.compose(orc, osc, table, v.idx, v.strike, v.rays)
    lits = to_literal(objs)
    for k in range(len(v)):
        n, inside, colour, tint = _literal_record(lits[int(v.idx[k])], v.rays[k].tolist(), tuple(v.strike[k].tolist()))
        assert bool(want.inside[k]) == inside, (cls, k)
        assert tuple(want.colour[k]) == tuple(colour), (cls, k)
        if n is None:
            assert np.isnan(want.normal[k]).all()
            continue
        assert sc.same_f64(want.normal[k], n), (cls, k)
        assert tuple(want.tint[k]) == tuple(tint), (cls, k)


# ---- seeded mutants --------------------------------------------------------------------------------------------------------------------
def _case_set(orc, mutant=None):
    """Every answer of the case set (the GPU tests compare the library with exactly these)."""
    out = {}
    for kind in WITNESSES:
        _, osc, table = witness(orc, kind)
        for cls in CLASSES:
            v = rc.vertices(orc, cls).spread(2000)
            out[kind, cls] = sc.compose(orc, osc, table, v.idx, v.strike, v.rays, mutant=mutant)
    for name in ("all_materials", "mostly_textured", "earth_thumb", "lights"):
        out[name] = frame_surfaces(orc, name, mutant)
    _, osc, table, hit, strike, rays = raw_roots(orc)
    out["raw_roots"] = sc.compose(orc, osc, table, hit, strike, rays, mutant=mutant)
    return out


@functools.lru_cache(maxsize=None)
def _right(orc):
    return _case_set(orc)


@pytest.mark.parametrize("mutant,output", [("normal_not_flipped", "normal"), ("flipped_dropped", "inside"), ("cap_ge", "colour"), ("cap_coordinate_1", "colour"),
                                           ("darken_emitters", "tint"), ("plane_normal_towards_ray", "normal"), ("uv_for_colour_root", "uv")])
def test_a_seeded_mutant_is_caught(orc, mutant, output):
    right, wrong = _right(orc), _case_set(orc, mutant)
    caught = {k: sc.differs(right[k], wrong[k]) for k in right}
    assert any(output in d for d in caught.values()), (mutant, caught)
    assert set(sc.MUTANTS) == {"normal_not_flipped", "flipped_dropped", "cap_ge", "cap_coordinate_1", "darken_emitters", "plane_normal_towards_ray",
                               "uv_for_colour_root"}


# ---- coverage conditions ---------------------------------------------------------------------------------------------------------------
def test_the_vertex_classes_cover_what_they_claim(orc):
    _, osc, table = witness(orc, "tex")
    z = table.zoo
    v = rc.concat([rc.vertices(orc, cls).spread(2000) for cls in CLASSES])
    e = sc.compose(orc, osc, table, v.idx, v.strike, v.rays)
    sphere = ~z.is_plane[v.idx]
    for sign in (1.0, -1.0):  # inside and outside slots on spheres of both radius signs
        m = sphere & (np.sign(z.r[v.idx]) == sign)
        assert (e.inside[m] == 1).sum() >= 50 and (e.inside[m] == 0).sum() >= 50, sign
    assert (e.cap == rc.GT).sum() >= 50 and (e.cap == rc.LT).sum() >= 50 and (e.cap == rc.EQ).sum() >= 50  # both sides of the band, and in it
    assert set(z.style[v.idx][~sphere].tolist()) == {0, 1, 2, 3}  # every plane style
    assert set(z.style[v.idx][sphere].tolist()) == set(range(7))
    assert e.textured.sum() >= 200 and (~e.textured).sum() >= 200
    assert rc.A.RT_TEXTURE_CHECKERED in {int(table.root_kind[i]) for i in v.idx[e.textured]}
    # Checkered, image and ramp roots, and a COLOUR root: the vertices above, the frames below and the scene made by hand between them
    _, _, rtable, rhit, _, _ = raw_roots(orc)
    assert {rc.A.RT_TEXTURE_UV_RAMP, rc.A.RT_TEXTURE_COLOUR, rc.A.RT_TEXTURE_CHECKERED} <= {int(rtable.root_kind[i]) for i in rhit}
    assert rtable.emitter[rhit].sum() >= 100 and (rtable.zoo.albedo[rhit][rtable.emitter[rhit]] != 1.0).all()


def test_the_three_frames_hold_what_the_census_found(orc):
    A = rc.A
    # all_materials, 71 x 41
    objs, cam, w, h, _, table, hits = frame(orc, "all_materials")
    e = frame_surfaces(orc, "all_materials")
    hit = hits.hit.reshape(-1)
    z = table.zoo
    assert (2 * w + 1, 2 * h + 1) == (71, 41) and len(hit) == 2911 and (hit >= 0).all()  # no miss
    sphere = ~z.is_plane[hit]
    assert set(z.style[hit][sphere].tolist()) == set(range(7)) and set(z.style[hit][~sphere].tolist()) == {1, 2, 3}
    assert int(e.inside.sum()) == 90  # the dome
    assert ((e.cap == rc.GT).sum(), (e.cap == rc.LT).sum(), (e.cap == rc.EQ).sum()) == (2, 14, 0)
    tex = np.flatnonzero(e.textured)
    assert len(tex) == 26 and tex.min() >= 1024 and tex.max() < 2048  # all in the second 1024-slot tile
    assert {int(table.root_kind[i]) for i in hit[tex]} == {A.RT_TEXTURE_CHECKERED, A.RT_TEXTURE_IMAGE}
    # mostly_textured, 57 x 29: every slot textured, so the first tile's list is exactly full
    objs, cam, w, h, _, table, hits = frame(orc, "mostly_textured")
    e = frame_surfaces(orc, "mostly_textured")
    assert (2 * w + 1, 2 * h + 1) == (57, 29) and len(e.textured) == 1653 and e.textured.all()
    assert {int(table.root_kind[i]) for i in hits.hit.reshape(-1)} == {A.RT_TEXTURE_CHECKERED}
    # earth_thumb, 65 x 37
    objs, cam, w, h, _, table, hits = frame(orc, "earth_thumb")
    e = frame_surfaces(orc, "earth_thumb")
    assert (2 * w + 1, 2 * h + 1) == (65, 37) and len(e.textured) == 2405
    assert int(e.textured.sum()) == 204 and int(e.inside.sum()) == 2201
    assert {int(table.root_kind[i]) for i in hits.hit.reshape(-1)[e.textured]} == {A.RT_TEXTURE_IMAGE}
    # lights, 35 x 21: misses
    _, _, _, _, _, _, hits = frame(orc, "lights")
    e = frame_surfaces(orc, "lights")
    miss = hits.hit.reshape(-1) < 0
    assert miss.sum() > 50 and np.isnan(e.normal[miss]).all() and not e.colour[miss].any() and not np.isnan(e.normal[~miss]).any()


def test_a_no_surface_slot_and_a_failed_normal(orc):
    _, osc, table = witness(orc, "planes")
    z = table.zoo
    i = int(z.spheres(rc.A.RT_SPHERE_LAMBERT_REFLECTION, where=(z.albedo == 0.5) & (z.r > 0.0) & (table.rgb.max(axis=1) > 100))[0])
    c, r = z.c[i], abs(z.r[i])
    p = c + np.array([r, 0.0, 0.0])
    ray = np.concatenate([p + np.array([1.0, 0.0, 0.0]), [-1.0, 0.0, 0.0]])
    hit = np.array([i, -1, -2, i, i, i], np.int32)
    strike = np.array([p, p, p, [np.nan, 0.0, 0.0], p, c])
    rays = np.tile(ray, (6, 1))
    rays[4, 1] = np.inf
    e = sc.compose(orc, osc, table, hit, strike, rays)
    assert not np.isnan(e.normal[0]).any() and e.tint[0].any()
    for k in (1, 2, 3, 4):
        assert np.isnan(e.normal[k]).all() and np.isnan(e.uv[k]).all() and e.inside[k] == 0 and not e.colour[k].any() and not e.tint[k].any()
    # a strike at the centre: Ray.make' gives ValueNone, the normal is NaN, the rest stays defined
    assert np.isnan(e.normal[5]).all() and e.colour[5].any() and e.tint[5].any()


# ---- the library ---------------------------------------------------------------------------------------------------------------------
ENTRY_POINTS = ("rt_surfaces", "rt_surfaces_device", "rt_camera_surfaces", "rt_camera_surfaces_device", "rt_dev_last_surface_plan")
MAX_W, MAX_H = 4, 3
FRAME = (2 * MAX_W + 1) * (2 * MAX_H + 1)


def _scene(rt):
    P, S, H, Tex, Px = rt.Point.make, rt.SphereStyle, rt.Hittable, rt.Texture.Colour, rt.Pixel
    return rt.Scene.make([H.Sphere(rt.Sphere.make(S.LambertReflection(0.8, Tex(Px(200, 100, 50))), P(0.0, 0.0, 3.0), 1.0)),
                          H.Sphere(rt.Sphere.make(S.LightSource(Tex(Px(20, 10, 250))), P(3.0, 0.0, 3.0), 1.0))])


def _camera(rt, spp=20, depth=3):
    from test_camera_hits_host import _basic_camera
    return _basic_camera(rt, spp, 9.0 / 7.0, depth)


def test_prototypes_and_struct(rt):
    from ray_tracing_fsharp_amd import _lib
    A = rt._abi
    header = open(os.path.join(ROOT, "include", "rtfs_amd.h")).read()
    assert "#define RT_ABI_VERSION 7" in header and rt.lib.rt_abi_version() == 7
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES
    t, which = A.rt_surface_outputs, A.ABI_STRUCT_SURFACE_OUTPUTS
    assert which == 13 and rt.lib.rt_abi_sizeof(which) == C.sizeof(t) == 48
    for k, (fname, _) in enumerate(t._fields_):
        assert rt.lib.rt_abi_offsetof(which, k) == getattr(t, fname).offset
    assert rt.lib.rt_abi_offsetof(which, len(t._fields_)) == C.c_size_t(-1).value
    assert [f for f, _ in t._fields_] == ["struct_size", "normal", "inside", "colour", "tint", "uv"]
    assert rt.lib.rt_abi_sizeof(14) == 0 and rt.lib.rt_abi_sizeof(8) == 0
    assert hasattr(rt.Scene, "surfaces") and hasattr(rt.Scene, "cameraSurfaces") and rt.Surfaces._fields == ("normal", "inside", "colour", "tint", "uv", "stats")
    assert "Sphere.fs:150-200" in header and "InfinitePlane.fs:43-99" in header
    w = (C.c_int64 * 8)(*([7] * 8))
    assert rt.lib.rt_dev_last_surface_plan(w) == A.RT_OK and rt.lib.rt_dev_last_surface_plan(None) == A.RT_ERR_INVALID_ARGUMENT


class _Bufs:
    def __init__(self, n):
        self.hit = np.zeros(n, np.int32)
        self.strike, self.rays = np.full((n, 3), 1.5), np.full((n, 6), 2.5)
        self.normal, self.inside = np.full((n, 3), 7.5), np.full(n, 77, np.uint8)
        self.colour, self.tint, self.uv = np.full((n, 3), 77, np.uint8), np.full((n, 3), 77, np.uint8), np.full((n, 2), 7.5)

    def out(self, rt, **kw):
        p = lambda a: a.ctypes.data  # noqa: E731
        o = rt._abi.rt_surface_outputs(normal=p(self.normal), inside=p(self.inside), colour=p(self.colour), tint=p(self.tint), uv=p(self.uv))
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def untouched(self):
        return ((self.normal == 7.5).all() and (self.inside == 77).all() and (self.colour == 77).all() and (self.tint == 77).all() and (self.uv == 7.5).all()
                and (self.strike == 1.5).all())


def _surface_calls(rt, s, n, hit, strike, rays, out, options=None):
    Lb = rt.lib
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None  # noqa: E731
    f64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None  # noqa: E731
    o = C.byref(out) if out is not None else None
    opt = C.byref(options) if options is not None else None
    if options is None:
        yield lambda: Lb.rt_surfaces(s, 0, n, i32(hit), f64(strike), f64(rays), 0, o, None)
    yield lambda: Lb.rt_surfaces_device(s, 0, n, p(hit), p(strike), p(rays), 0, o, None, opt, None)


def _camera_calls(rt, s, cam, n, px, hit, strike, out, max_w=MAX_W, max_h=MAX_H, first=2, per=3, options=None):
    Lb = rt.lib
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None  # noqa: E731
    f64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None  # noqa: E731
    c = C.byref(cam) if cam is not None else None
    o = C.byref(out) if out is not None else None
    opt = C.byref(options) if options is not None else None
    if options is None:
        yield lambda: Lb.rt_camera_surfaces(s, c, max_w, max_h, 1, 0, n, i32(px), first, per, 0, i32(hit), f64(strike), o, None)
    yield lambda: Lb.rt_camera_surfaces_device(s, c, max_w, max_h, 1, 0, n, p(px), first, per, 0, p(hit), p(strike), o, None, opt, None)


def test_invalid_arguments_are_refused_before_any_device_call(rt):
    A = rt._abi
    scene = _scene(rt)
    S = scene.handle
    n = 5
    b = _Bufs(n)
    out = b.out(rt)
    bad = A.rt_render_options(block_threads=100)
    unset = A.rt_render_options(); unset.struct_size = 0
    empty = A.rt_surface_outputs()
    calls = []
    calls += list(_surface_calls(rt, None, n, b.hit, b.strike, b.rays, out))              # NULL scene
    calls += list(_surface_calls(rt, S, n, None, b.strike, b.rays, out))                  # NULL inputs with work to do
    calls += list(_surface_calls(rt, S, n, b.hit, None, b.rays, out))
    calls += list(_surface_calls(rt, S, n, b.hit, b.strike, None, out))
    calls += list(_surface_calls(rt, S, n, b.hit, b.strike, b.rays, None))                # NULL out
    calls += list(_surface_calls(rt, S, n, b.hit, b.strike, b.rays, b.out(rt, struct_size=40)))
    calls += list(_surface_calls(rt, S, n, b.hit, b.strike, b.rays, b.out(rt, struct_size=0)))
    calls += list(_surface_calls(rt, S, n, b.hit, b.strike, b.rays, empty))               # every output NULL
    calls += list(_surface_calls(rt, S, 2**31, b.hit, b.strike, b.rays, out))             # the ray lists' bound
    calls += list(_surface_calls(rt, S, 2**63, b.hit, b.strike, b.rays, out))
    assert len(calls) == 20
    calls += list(_surface_calls(rt, S, n, b.hit, b.strike, b.rays, out, options=bad))
    calls += list(_surface_calls(rt, S, n, b.hit, b.strike, b.rays, out, options=unset))
    for entry in (2, -3, 2**31 - 1, -2**31):                                              # a HOST list with an index outside [-2, n_hittables)
        lst = b.hit.copy()
        lst[3] = entry
        calls += list(_surface_calls(rt, S, n, lst, b.strike, b.rays, out))[:1]
    assert len(calls) == 26
    # the camera route: rt_camera_hits' refusals (hit_index and strike may be NULL here) and the outputs'
    cam = _camera(rt).to_abi()
    per = 3
    px = np.array([0, 7, FRAME - 1, 7, 30], np.int32)
    cb = _Bufs(n * per)
    cout = cb.out(rt)

    def with_cam(**kw):
        c = _camera(rt).to_abi()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    a = (n, px, cb.hit, cb.strike)
    calls += list(_camera_calls(rt, None, cam, *a, cout))
    calls += list(_camera_calls(rt, S, None, *a, cout))
    calls += list(_camera_calls(rt, S, cam, *a, cout, max_w=0))
    calls += list(_camera_calls(rt, S, cam, *a, cout, max_w=40000, max_h=40000))
    calls += list(_camera_calls(rt, S, with_cam(samples_per_pixel=0), *a, cout))
    calls += list(_camera_calls(rt, S, with_cam(bounce_depth=-1), *a, cout))
    calls += list(_camera_calls(rt, S, cam, *a, cout, first=-1))
    calls += list(_camera_calls(rt, S, cam, *a, cout, per=0))
    calls += list(_camera_calls(rt, S, cam, *a, cout, first=7999998, per=3))
    calls += list(_camera_calls(rt, S, cam, 2**30, px, cb.hit, cb.strike, cout, per=2))
    calls += list(_camera_calls(rt, S, cam, FRAME + 1, None, cb.hit, cb.strike, cout))
    calls += list(_camera_calls(rt, S, cam, *a, None))
    calls += list(_camera_calls(rt, S, cam, *a, cb.out(rt, struct_size=44)))
    calls += list(_camera_calls(rt, S, cam, *a, empty))
    calls += list(_camera_calls(rt, S, cam, *a, cout, options=bad))
    for entry in (-1, FRAME):
        lst = px.copy()
        lst[3] = entry
        calls += list(_camera_calls(rt, S, cam, n, lst, cb.hit, cb.strike, cout))[:1]
    assert len(calls) == 26 + 14 * 2 + 1 + 2
    for i, call in enumerate(calls):
        assert call() == A.RT_ERR_INVALID_ARGUMENT, i
        assert rt.lib.rt_last_error()
        assert b.untouched() and cb.untouched() and (cb.hit == 0).all(), i  # nothing written


def test_n_zero_is_a_no_op(rt):
    A = rt._abi
    scene = _scene(rt)
    S, Lb = scene.handle, rt.lib
    b = _Bufs(1)
    out = b.out(rt)
    cam = _camera(rt).to_abi()
    calls = (lambda st: Lb.rt_surfaces(S, 0, 0, None, None, None, 0, C.byref(out), st),
             lambda st: Lb.rt_surfaces_device(S, 0, 0, None, None, None, A.RT_RENDER_COUNTERS, C.byref(out), None, None, st),
             lambda st: Lb.rt_camera_surfaces(S, C.byref(cam), MAX_W, MAX_H, 1, 0, 0, None, 0, 1, 0, None, None, C.byref(out), st),
             lambda st: Lb.rt_camera_surfaces_device(S, C.byref(cam), MAX_W, MAX_H, 1, 0, 0, None, 0, 1, 0, None, None, C.byref(out), None, None, st))
    for call in calls:
        assert call(None) == A.RT_OK
        st = A.rt_stats(rays=5, samples=9, pixels=4, kernel_ms=3.0)
        assert call(C.byref(st)) == A.RT_OK
        assert st.rays == 0 and st.samples == 0 and st.pixels == 0 and st.kernel_ms == 0.0
    assert b.untouched()
    # an empty list is still checked
    assert Lb.rt_surfaces(S, 0, 0, None, None, None, 0, None, None) == A.RT_ERR_INVALID_ARGUMENT
    assert Lb.rt_camera_surfaces(S, C.byref(cam), MAX_W, MAX_H, 1, 0, 0, None, 0, 0, 0, None, None, C.byref(out), None) == A.RT_ERR_INVALID_ARGUMENT
    res = scene.surfaces(np.zeros(0, np.int32), np.zeros((0, 3)), np.zeros((0, 6)), uv=True)
    assert res.normal.shape == (0, 3) and res.inside.shape == (0,) and res.colour.shape == res.tint.shape == (0, 3) and res.uv.shape == (0, 2)
    assert res.normal.dtype == res.uv.dtype == np.float64 and res.inside.dtype == res.colour.dtype == res.tint.dtype == np.uint8
    assert res.stats["samples"] == 0 and res.stats is scene.last_stats
    hits, res = scene.cameraSurfaces(MAX_W, MAX_H, _camera(rt), None, n=0, n_samples=2, strike=False, tint=False)
    assert hits.hit_index.shape == (0, 2) and hits.strike is None and hits.rays is None and res.tint is None and res.uv is None and res.normal.shape == (0, 2, 3)


def test_past_the_checks_the_call_asks_for_the_device(rt):
    """The limits themselves are admitted -- NULL hit_index and strike on the camera route, a single output, -1 and -2 entries,
    sample_first + n_samples == 8000000, RT_RENDER_COUNTERS -- and without a GPU the failure is loud: RT_ERR_NO_DEVICE, nothing written.
    (With a GPU the same calls succeed: tests/test_gpu_surfaces.py.)"""
    A = rt._abi
    scene, cam = _scene(rt), _camera(rt).to_abi()
    S, Lb = scene.handle, rt.lib
    want = A.RT_OK if rt.device_count() > 0 else A.RT_ERR_NO_DEVICE
    b = _Bufs(4)
    b.hit[:] = (0, -1, -2, 1)
    only_inside = A.rt_surface_outputs(inside=b.inside.ctypes.data)
    i32, f64 = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double)))
    assert Lb.rt_surfaces(S, 0, 4, i32(b.hit), f64(b.strike), f64(b.rays), A.RT_RENDER_COUNTERS, C.byref(only_inside), None) == want
    cb = _Bufs(FRAME * 2)
    only_normal = A.rt_surface_outputs(normal=cb.normal.ctypes.data)
    assert Lb.rt_camera_surfaces(S, C.byref(cam), MAX_W, MAX_H, 1, 0, FRAME, None, 7999998, 2, 0, None, None, C.byref(only_normal), None) == want
    if want != A.RT_OK:
        assert b.untouched() and cb.untouched()
        for call in (lambda: scene.surfaces(b.hit, b.strike, b.rays), lambda: scene.cameraSurfaces(MAX_W, MAX_H, _camera(rt), np.array([0, 5, 9], np.int32)),
                     lambda: scene.cameraSurfaces(MAX_W, MAX_H, _camera(rt))):
            with pytest.raises(rt.RtError) as e:
                call()
            assert e.value.code == A.RT_ERR_NO_DEVICE


def test_python_wrapper_checks_shapes_and_dtypes(rt):
    scene, cam = _scene(rt), _camera(rt)
    hit, strike, rays = np.zeros(3, np.int32), np.zeros((3, 3)), np.zeros((3, 6))
    for bad in (np.zeros(3, np.int64), np.zeros(3, np.float64), [0, 1, 2]):
        with pytest.raises(TypeError):
            scene.surfaces(bad, strike, rays)
    with pytest.raises(TypeError):
        scene.surfaces(hit, strike.astype(np.float32), rays)
    with pytest.raises(TypeError):
        scene.surfaces(hit, strike, rays.astype(np.float32))
    for bad_strike, bad_rays in ((np.zeros((3, 2)), rays), (strike, np.zeros((3, 3))), (np.zeros((4, 3)), rays), (strike, np.zeros((2, 6))), (np.zeros(9), rays)):
        with pytest.raises(ValueError):
            scene.surfaces(hit, bad_strike, bad_rays)
    with pytest.raises(ValueError):
        scene.surfaces(np.zeros((3, 1), np.int32), strike, rays)
    with pytest.raises(ValueError):  # options belong to the device entry
        scene.surfaces(hit, strike, rays, options=rt._abi.rt_render_options(chunk_pixels=8))
    with pytest.raises(ValueError):
        scene.cameraSurfaces(MAX_W, MAX_H, cam, np.ones(3, np.int32), n=3)
    with pytest.raises(TypeError):
        scene.cameraSurfaces(MAX_W, MAX_H, cam, np.ones(3, np.int64))
    with pytest.raises(TypeError):
        scene.cameraSurfaces(MAX_W, MAX_H, cam, np.ones(3, np.int32), n_samples=2.0)
    refused = [lambda: scene.surfaces(np.array([0, 2, 0], np.int32), strike, rays), lambda: scene.surfaces(np.array([0, -3, 0], np.int32), strike, rays),
               lambda: scene.surfaces(hit, strike, rays, normal=False, inside=False, colour=False, tint=False),
               lambda: scene.cameraSurfaces(MAX_W, MAX_H, cam, np.array([0, FRAME, 2], np.int32)),
               lambda: scene.cameraSurfaces(MAX_W, MAX_H, cam, np.ones(3, np.int32), n_samples=0),
               lambda: scene.cameraSurfaces(MAX_W, MAX_H, cam, np.ones(3, np.int32), normal=False, inside=False, colour=False, tint=False)]
    for call in refused:
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == rt._abi.RT_ERR_INVALID_ARGUMENT


def build_surfaces_smoke(tmp_path):
    exe = str(tmp_path / "surfaces_smoke")
    libdir = os.path.join(ROOT, "ray-tracing-fsharp_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "surfaces_smoke.c"),
                           "-L", libdir, "-lrtfs_amd", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    return exe


def test_c_program_checks_the_surface_arguments(rt, tmp_path):
    """tests/c/surfaces_smoke.c from C99: the argument checks hold without a GPU (with one, test_gpu_surfaces compares the frame it
    prints with the composer's)."""
    out = subprocess.run([build_surfaces_smoke(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "surfaces: argument checks ok" in out.stdout
