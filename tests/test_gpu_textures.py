"""Texture.colourAt on the device (texture_colour_at_inline, csrc/rt_device.h) against the oracle, on the families of
tests/texture_cases.py -- which tests/test_texture_model.py holds to the line-by-line restatement on the CPU -- through every route that
evaluates a texture: the unit hook (the out-of-line copy), Hittable.reflection with TEX = true, and stage_tex of the render kernel,
reached by ray lists (scene in the LDS, partly in it, in global memory; 16-bit and full-width queue entries) and by frames whose
hits are mostly textured (fused and two-pass launches, every setting of the park pool).  Everything is compared exactly: (u, v) as
bit patterns, colours and generator states as bytes.

Run time: 7 s for the 50 tests on one MI355X, most of it the host's side of the padded scenes (the families are a few thousand points each).
"""
import numpy as np
import pytest

import scenes
import texture_cases as tc
from ray_tracing_fsharp_amd import _abi as A
from test_gpu_parity import _render_both, _same_f64, _scene_pair
from test_gpu_ray_queries import _oracle_trace

pytestmark = pytest.mark.gpu

FAMILY_NAMES = sorted(tc.FAMILIES)


def _pair(rt, orc, case, extra=()):
    """The case's scene on both sides: from the host mirror's objects where the case has them (then plain spheres can be added),
    from the ABI arrays otherwise (then they are appended to the arrays)."""
    if case.objs is not None:
        return _scene_pair(rt, orc, list(case.objs) + list(extra))
    if not extra:
        return scenes.raw_scene_pair(orc, *case.arrays())
    more, n_more, _, _, _ = tc.flatten_hittables(list(extra))
    hs = (A.rt_hittable * (case.n + n_more))(*(list(case.hs[: case.n]) + list(more[:n_more])))
    return scenes.raw_scene_pair(orc, hs, case.n + n_more, case.tex, case.ntex, case.keep)


def _first_difference(a, b):
    bad = np.flatnonzero(np.any(a != b, axis=1))
    return f"{bad.size} differ, first at {bad[0]}: device {a[bad[0]]}, oracle {b[bad[0]]}" if bad.size else "equal"


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_texture_hook_equals_the_oracle(rt, orc, family):
    """rt_dev_texture_colour_at: (u, v) bit for bit, and the colour, at every point of every query."""
    for case in tc.FAMILIES[family]():
        s, o = _pair(rt, orc, case)
        for q in case.queries:
            uv1, c1 = rt.hooks.texture_colour_at(s, q.texture, q.points)
            uv2, c2 = o.texture_colour_at(q.texture, q.points)
            where = f"{family}/{case.name}/texture {q.texture}"
            assert np.array_equal(c1, c2), f"{where}: colours {_first_difference(c1, c2)}"
            assert _same_f64(uv1, uv2), f"{where}: (u, v) differs"


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_reflection_of_the_wearers_equals_the_oracle(rt, orc, family):
    """rt_dev_reflection (the TEX = true reflection, which calls the out-of-line copy) with the query points as strike points."""
    rng = np.random.default_rng(17)
    for case in tc.FAMILIES[family]():
        s, o = _pair(rt, orc, case)
        for q in case.queries:
            n = len(q.points)
            rays = scenes.random_rays(n, 300 + q.hittable, origin_scale=2.0)
            rays[:, :3] += q.points
            col = rng.integers(0, 256, size=(n, 3), dtype=np.uint8)
            col[: n // 4] = 255  # white light shows the texture's own colour
            st = rng.integers(1, 2 ** 31 - 1, size=(n, 4), dtype=np.uint32)
            idx = np.full(n, q.hittable)
            a1, c1, r1, g1 = rt.hooks.reflection(s, idx, rays, col, q.points, st)
            a2, c2, r2, g2 = o.reflection(idx, rays, col, q.points, st)
            where = f"{family}/{case.name}/hittable {q.hittable}"
            assert np.array_equal(a1, a2), f"{where}: absorbed"
            assert np.array_equal(c1, c2), f"{where}: colours {_first_difference(c1, c2)}"
            assert _same_f64(r1, r2), f"{where}: outgoing ray"
            assert np.array_equal(g1, g2), f"{where}: rng state"


def _plain_field(n, seed):
    """n small plain Lambert spheres in a 30-unit cube far from the wearers: they only make the scene larger."""
    rng = np.random.default_rng(seed)
    c = np.array([0.0, 0.0, 600.0]) + rng.uniform(-15.0, 15.0, (n, 3))
    return [scenes.H.Sphere(scenes.rt.Sphere.make(scenes.S.LambertReflection(0.7, scenes.Tex(scenes.Px(90, 120, 60))), scenes.P(*c[i]), float(rng.uniform(0.05, 0.3))))
            for i in range(n)]


def _trace_both(rt, orc, family, padding, want_lds):
    rng = np.random.default_rng(23 + padding)
    field = _plain_field(padding, seed=padding) if padding else []
    for case in tc.FAMILIES[family]():
        s, o = _pair(rt, orc, case, field)
        assert s.info()["lds_resident"] == want_lds, (case.name, s.info())
        rays = np.concatenate([q.rays for q in case.queries])
        st = rng.integers(1, 2 ** 31 - 1, size=(len(rays), 4), dtype=np.uint32)
        for depth in (0, 3):
            want, g2 = _oracle_trace(orc, o, rays, depth, st)  # the oracle takes Ray.make' of the caller's rays
            for counters in (False, True):
                got, g1 = s.traceRays(rays, depth, rng=st, counters=counters)
                where = f"{family}/{case.name}/+{padding}/depth {depth}/{'counting' if counters else 'timed'}"
                assert np.array_equal(got, want), f"{where}: colours {_first_difference(got, want)}"
                assert np.array_equal(g1, g2), f"{where}: rng states"


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_traced_rays_at_the_wearers_scene_in_lds(rt, orc, family):
    """rt_trace_rays with the caller's generator states, rays aimed at the textured objects, bounce depths 0 and 3: stage_tex of the
    render kernel, timed and counting variants, the scene LDS-resident."""
    _trace_both(rt, orc, family, 0, 1)


@pytest.mark.parametrize("padding", [900, 1700, 17000])
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_traced_rays_at_the_wearers_scene_beyond_the_lds(rt, orc, family, padding):
    """The same with the scene padded by plain spheres to the sizes of test_tree_partly_in_lds: hybrid and global placements of the
    tree, 16-bit and (17000) full-width queue entries -- the texture records and texels are read through the global-memory view."""
    _trace_both(rt, orc, family, padding, 0)


def _frames(s, w, h, cam, seed):
    """The frame under every launch shape the issue names: passes 1 and 2, park_lanes -1 (never park), 1, default and 256, counting
    and timed variants -- per call, through rt_render_options."""
    for passes in (1, 2):
        for park in (-1, 1, 0, 256):
            for counters in (True, False):
                res = s.render_frame(w, h, cam, seed=seed, devices=(0,), counters=counters, options=A.rt_render_options(passes=passes, park_lanes=park))
                yield f"passes {passes}, park_lanes {park}, {'counting' if counters else 'timed'}", res


def test_mostly_textured_frame_under_every_park_setting(rt, orc):
    """A frame where nearly every hit evaluates a texture (a Checkered ground and every texture-carrying style), so that stage_tex's
    own park pool fills and its "pool full" branch runs; all launch shapes equal each other and the oracle."""
    objs, cam, w, h = tc.mostly_textured_scene()
    res, acc, rgb, st = _render_both(rt, orc, objs, cam, w, h, seed=9)
    assert np.array_equal(res.accum, acc) and np.array_equal(res.rgb, rgb)
    for k in ("rays", "prim_tests", "reflections", "samples", "pixels_early"):
        assert res.stats[k] == st[k], k
    s = rt.Scene.make(objs)
    # the share of textured hits, from the oracle: primary rays of the frame's pixels that strike a parameterised texture first
    hit, _, _ = orc.OracleScene(objs).hit_object(_primary_rays(cam, w, h))
    textured = np.array([o.kind != A.RT_HITTABLE_INFINITE_PLANE and o.sphere.Style.texture is not None and o.sphere.Style.texture.param is not None for o in objs])
    assert (hit >= 0).all() and textured[hit].mean() > 0.8
    for name, frame in _frames(s, w, h, cam, 9):
        assert np.array_equal(frame.accum, acc) and np.array_equal(frame.rgb, rgb), name
        assert frame.stats[0]["samples"] == st["samples"], name


def _primary_rays(cam, w, h):
    import candidate_cases as cc
    return cc.camera_rays(cam, w, h, cc.all_pixels(w, h), np.array([[0.5, 0.5]])).reshape(-1, 6)


def test_texels_are_copied_at_creation(rt, orc):
    """rt_texture.texels is "copied by rt_scene_create": overwriting the caller's buffers after creation and before the first render
    (the device copy is made lazily, at the first launch) changes nothing."""
    case = next(tc.family_images())
    s, o = scenes.raw_scene_pair(orc, *case.arrays())
    q = case.queries[5]  # the 257 x 3 image
    _, want = o.texture_colour_at(q.texture, q.points)
    rays = np.concatenate([x.rays for x in case.queries])
    st = np.random.default_rng(4).integers(1, 2 ** 31 - 1, size=(len(rays), 4), dtype=np.uint32)
    want_traced, _ = _oracle_trace(orc, o, rays, 2, st)
    saved = [img.copy() for img in case.keep]
    try:
        for img in case.keep:
            img[...] = 255 - img
        _, got = rt.hooks.texture_colour_at(s, q.texture, q.points)
        traced, _ = s.traceRays(rays, 2, rng=st)
    finally:
        for img, old in zip(case.keep, saved):
            img[...] = old
    assert len(case.keep) >= 8 and np.array_equal(got, want) and np.array_equal(traced, want_traced)
    # and a frame: the earth scene's texel buffers overwritten before its first render
    case = list(tc.family_images())[1]
    cam = scenes.dataclasses.replace(rt.Camera.makeBasic(12, 4.0, 2.0, scenes.P(8.0, 0.3, -1.8), scenes.unit(0.0, 0.0, 1.0), scenes.V(0.0, 1.0, 0.0)), BounceDepth=4)
    acc, rgb, _ = orc.OracleScene(case.objs).render_rows(16, 8, cam.to_abi(), seed=2, threads=8)
    fresh = rt.Scene.make(case.objs)
    saved = [img.copy() for img in fresh._keep]
    try:
        for img in fresh._keep:
            img[...] = 7
        res = fresh.render_rows(16, 8, cam, seed=2)
    finally:
        for img, old in zip(fresh._keep, saved):
            img[...] = old
    assert np.array_equal(res.accum, acc) and np.array_equal(res.rgb, rgb)
    assert np.any(rgb != 200, axis=-1).mean() > 0.25  # the map is in the frame (the sky is grey 200)
