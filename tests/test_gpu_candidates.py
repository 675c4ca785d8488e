"""The timed kernel's per-pixel candidate walk (pixel_candidates, csrc/rt_device.h) on the device, under cameras filled in by hand
(tests/candidate_cases.py): the device's sets equal the numpy model's -- which tests/test_candidates_model.py holds to the exact
BoundingBox.hits on the CPU -- for scenes in and beyond the LDS, and whole renders with such cameras equal the counting variant
and the oracle bit for bit."""
import numpy as np
import pytest

import candidate_cases as cc
import scenes
from test_gpu_parity import _assert_render_equal, _render_both

pytestmark = pytest.mark.gpu


def _assert_hook_equals_model(rt, s, cam, mw, mh, rc, name):
    got = rt.hooks.pixel_candidates(s, cam, mw, mh, rc)
    want, walk = cc.model(s, cam, mw, mh, rc)
    assert np.array_equal(got[:, 0] == -2, walk), f"{name}: walk flags differ at {np.flatnonzero((got[:, 0] == -2) != walk)[:5]}"
    differ = np.flatnonzero(np.any(got[~walk] != want[~walk], axis=1))
    assert differ.size == 0, f"{name}: {differ.size} pixels differ, first {rc[~walk][differ[0]]}: device {got[~walk][differ[0]]}, model {want[~walk][differ[0]]}"
    return want, walk


@pytest.mark.parametrize("family", sorted(cc.FAMILIES))
def test_device_candidates_equal_the_model(rt, family):
    """Same Leaves in the same order, same fall-back to walking, pixel for pixel, on every camera family."""
    for name, objs, cam, mw, mh, rc in cc.FAMILIES[family]():
        s = rt.Scene.make(objs)
        assert s.info()["lds_resident"] == 1
        _assert_hook_equals_model(rt, s, cam, mw, mh, rc, name)


def _far_field(n, seed, centre=(0.0, 0.0, 300.0)):
    """n small Lambert spheres in a 30-unit cube far from the family scenes: enough objects to leave the LDS (and, from 16384
    objects, the 16-bit queue entries), few enough in the cameras' reach that pixels stay on the candidate path."""
    rng = np.random.default_rng(seed)
    c = np.asarray(centre) + rng.uniform(-15.0, 15.0, (n, 3))
    return [cc._lambert(c[i], float(rng.uniform(0.05, 0.3))) for i in range(n)]


@pytest.mark.parametrize("n", [900, 1700, 17000])
def test_device_candidates_beyond_the_lds(rt, orc, n):
    """Scenes that do not fit the LDS (the sizes of test_tree_partly_in_lds; 17000 objects take full-width queue entries, two
    candidates at most): the hook runs the global-memory view of the timed kernel; device == model, and the model's sets contain
    every Leaf a test ray of the pixel hits exactly."""
    field = _far_field(n, seed=n)
    kept = counts = 0
    for fam in ("off_centre", "eye"):
        for name, objs, cam, mw, mh, rc in list(cc.FAMILIES[fam]())[:4]:
            s = rt.Scene.make(list(objs) + field)
            assert s.info()["lds_resident"] == 0
            cand, walk = _assert_hook_equals_model(rt, s, cam, mw, mh, rc, f"{n}/{name}")
            reach, ids = cc.reachable_leaves(orc, s, cam, mw, mh, rc[~walk], seed=n)
            for i, row in enumerate(cand[~walk]):
                assert set(ids[reach[i]].tolist()) <= set(row[row >= 0].tolist()), (n, name, rc[~walk][i])
            kept += int((~walk).sum())
            counts = max(counts, int((cand >= 0).sum(axis=1).max()))
    assert kept > 20
    assert counts >= (2 if n >= 16384 else 3)  # pixels with a second queue word: its decoding is checked too


def test_regression_eye_plane_hole(rt, orc):
    """The camera of the eye-plane hole (eye 0, axes x and y, vw = vh = 1, one coordinate, xaxis_origin (-0.25, -0.25, 0.05)) and a
    large light source (radius 6) centred on the corner ray of pixel (0, 0) at distance 12: every corner of that pixel's pyramid but one lies
    in front of the plane through the eye normal to their sum, the light's box lies wholly behind it, and the pixel's rays do hit
    the light.  Before the guard the timed kernel dropped it from the pixel's candidates (black where the oracle sees light)."""
    cam = scenes.free_camera((0.0, 0.0, 0.0), (-0.25, -0.25, 0.05), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1.0, 1.0, 100, 5)
    g0 = np.array([-0.25, -0.25, 0.05])
    objs = [scenes.H.Sphere(scenes.rt.Sphere.make(scenes.S.LightSource(scenes.Tex(scenes.Px(250, 240, 200))), scenes.P(*(g0 / np.linalg.norm(g0) * 12.0)), 6.0)),
            cc._lambert((3.0, 1.0, 4.0), 1.0)]
    s = rt.Scene.make(objs)
    cand = rt.hooks.pixel_candidates(s, cam, 1, 1, np.array([[0, 0]], np.int32))
    assert 0 in cand[0].tolist() or cand[0, 0] == -2
    res, acc, rgb, st = _render_both(rt, orc, objs, cam, 1, 1, seed=1)  # (a seed whose rays of that pixel reach the light)
    _assert_render_equal(res, acc, rgb, st)
    assert rgb[0, 1].any()  # pixel (row 0, col 0) -- image row maxH - row - 1 = 0, column col + maxW = 1 -- sees the light


@pytest.mark.parametrize("seed", range(24))
def test_free_camera_fuzz(rt, orc, seed):
    """random_scene-style objects around a free camera from families (a)-(d), 1-4 coordinate images, 20-60 samples per pixel:
    timed == counting == oracle, bit for bit, counters included."""
    name, objs, cam, mw, mh = cc.free_camera_render_case(seed)
    _assert_render_equal(*_render_both(rt, orc, objs, cam, mw, mh, seed=seed))


@pytest.mark.parametrize("passes", [1, 2])
def test_free_camera_render_beyond_the_lds(rt, orc, passes):
    """A free camera (off-grid viewport, skewed axes) over a scene that does not fit the LDS, fused and two-pass launches."""
    name, objs, cam, mw, mh, _ = list(cc.family_axes(seed=77))[5]
    objs = list(objs) + _far_field(1000, seed=5, centre=(0.0, 0.0, 40.0))
    objs.append(scenes.H.UnboundedSphere(scenes.rt.Sphere.make(scenes.S.LightSource(scenes.Tex(scenes.Px(200, 210, 255))), scenes.P(0.0, 0.0, 0.0), 500.0)))
    assert rt.Scene.make(objs).info()["lds_resident"] == 0
    try:
        rt.set_passes(passes)
        _assert_render_equal(*_render_both(rt, orc, objs, cam, mw, mh, seed=passes))
    finally:
        rt.set_passes(0)
