"""The closest-hit rule of Scene.hitObject (csrc/rt_device.h: `unbounded_tests`, inlined by hit_object, the rt_dev_hit_object_lds
kernel, the render and trace kernel's shading stage, the ray-query kernel and the camera-hits kernel; `leaf_test_object_exact` for
the Leaves) and `plane_intersection`, against the oracle with no tolerance, on the scenes and rays of tests/closest_hit_cases.py:
pairs of hits a hair's breadth inside and outside the 1e-8 band of `Float.compare a bestFloat`, exact ties, hits below t = 1e-4, at
t = 2^14 (where the band is exact equality) and at t * t = +inf, in every shape of the unbounded list, with and without a tree,
resident in LDS and padded past it.  Routes: the three unit hooks, Scene.hitObject timed and counting under three schedules,
Scene.traceRays at depth 0 (the colour names the winner) and at depth 1 off a mirror, renders fused and in two passes, camera hits.
tests/test_closest_hit_cases.py holds the oracle to the literal restatement on the same rays."""
import ctypes as C

import numpy as np
import pytest

import camera_hit_cases
import closest_hit_cases as chc
from test_gpu_sphere_arms import COUNTERS, SCHEDULES

pytestmark = pytest.mark.gpu

GROUPS = {c: [("class", c, r) for r in range(5)] for c in chc.CLASSES}
GROUPS["leaf_leaf_single_duo"] = [k for k in chc.RESIDENT if k[0] in ("leaf_leaf", "single", "duo")]
GROUPS["unbounded_only"] = [k for k in chc.RESIDENT if k[0] == "unbounded_only"]
GROUPS["at_infinity"] = [k for k in chc.RESIDENT if k[0] == "infinity"]
GROUPS["mirror"] = [("mirror",)]
GROUPS.update({chc.label(k): [k] for k in chc.PADDED})
assert sorted(k for g in GROUPS.values() for k in g) == sorted(chc.RESIDENT + [("mirror",)] + chc.PADDED)
_PAIRS, _WANT = {}, {}


def _pair(rt, orc, key):
    if key not in _PAIRS:
        b = chc.scene(key)
        _PAIRS[key] = (rt.Scene.make(b.objs), orc.OracleScene(b.objs), b)
        assert _PAIRS[key][0].info()["lds_resident"] == (0 if b.padded else 1), key
    return _PAIRS[key]


def _same_f64(a, b):
    return camera_hit_cases.same_f64(a, b)


def _expected(rt, orc, key):
    """[(label, rays, which, made rays, oracle hit, strike (NaN where none), counters)] of a scene's lists, computed once."""
    if key not in _WANT:
        _, o, b = _pair(rt, orc, key)
        out = []
        for label, rays, which in chc.ray_lists(key):
            made = np.array([orc.ray_make(r[:3], r[3:]) for r in rays])  # (no vector of these lists is zero)
            hit, strike, cnt = o.hit_object(made)
            strike = np.where((hit >= 0)[:, None], strike, np.nan)
            m = which >= len(b.crafted()) - len(b)  # the crafted rays whose winner the class states (the mirror's first legs have none)
            assert np.array_equal(hit[m], b.want[which[m] - (len(b.crafted()) - len(b))]), label
            for a in (made, hit, strike, cnt):
                a.setflags(write=False)
            out.append((label, rays, which, made, hit, strike, cnt))
        _WANT[key] = out
    return _WANT[key]


def _opts(rt, sched):
    return rt._abi.rt_render_options(**sched) if sched else None


def _assert_placement(rt, b):
    assert rt.hooks.last_launch_plan()["out"]["q_lds"] == (0 if b.padded else 1), b.name


def test_plane_intersection_hook(rt, orc):
    """rt_dev_plane_intersection on every class of InfinitePlane.intersection, in lists of 64 and 65 rays per class and one of 4096
    rays over all classes."""
    cls = chc.plane_classes()
    for name, (rays, planes) in cls.items():
        for n in (64, 65):
            pick = np.arange(n) % len(rays)
            assert _same_f64(rt.hooks.plane_intersection(rays[pick], planes[pick]), orc.plane_intersection(rays[pick], planes[pick])), (name, n)
    rays, planes = np.concatenate([r for r, _ in cls.values()]), np.concatenate([p for _, p in cls.values()])
    pick = np.arange(4096) % len(rays)
    want = orc.plane_intersection(rays[pick], planes[pick])
    assert len(rays) <= 4096 and 0.2 < np.isnan(want).mean() < 0.8
    assert _same_f64(rt.hooks.plane_intersection(rays[pick], planes[pick]), want)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_unit_hooks(rt, orc, group):
    """rt_dev_hit_object on every list of every scene, rt_dev_hit_object_lds on those of the resident ones: hit index and strike; the
    counting hook's Hittable.hits calls per ray."""
    for key in GROUPS[group]:
        s, _, b = _pair(rt, orc, key)
        for label, _, _, made, hit, strike, cnt in _expected(rt, orc, key):
            h0, s0, c0 = rt.hooks.hit_object(s, made)
            assert np.array_equal(h0, hit), (label, np.flatnonzero(h0 != hit)[:8])
            assert _same_f64(np.where((h0 >= 0)[:, None], s0, np.nan), strike), label
            assert np.array_equal(c0[:, 1], cnt[:, 1]), label
            if not b.padded:
                h1, s1 = rt.hooks.hit_object_lds(s, made)
                assert np.array_equal(h1, hit), (label, np.flatnonzero(h1 != hit)[:8])
                assert _same_f64(np.where((h1 >= 0)[:, None], s1, np.nan), strike), label


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_scene_hit_object(rt, orc, group):
    """Scene.hitObject, the timed kernel and the counting one, under the three schedules: hit index and strike point of every ray of
    every list; the counting launch's rays and Hittable.hits calls are the oracle's sums."""
    import torch

    for key in GROUPS[group]:
        s, _, b = _pair(rt, orc, key)
        for label, rays, _, _, hit, strike, cnt in _expected(rt, orc, key):
            r = torch.from_numpy(np.array(rays)).cuda()
            for sched in SCHEDULES:
                for counters in (False, True):
                    hi, sk = s.hitObject(r, counters=counters, options=_opts(rt, sched))
                    hi = hi.cpu().numpy()
                    assert np.array_equal(hi, hit), (label, sched, counters, np.flatnonzero(hi != hit)[:8])
                    assert _same_f64(sk.cpu().numpy(), strike), (label, sched, counters)
                    if counters:
                        st = s.last_stats
                        assert st["rays"] == len(rays) and st["prim_tests"] == int(cnt[:, 1].sum()), (label, sched, st)
            _assert_placement(rt, b)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_trace_rays_name_the_winner(rt, orc, group):
    """Scene.traceRays at depth 0 (depth 1 in the mirror scene, whose second legs are the crafted rays): every object is a light of
    its own colour, so the colour IS the winner -- the oracle's, and for the crafted rays the one the class states.  Colours and
    final generator states, both variants, three schedules."""
    import torch

    depth = 1 if group == "mirror" else 0
    for key in GROUPS[group]:
        s, o, b = _pair(rt, orc, key)
        first = len(b.crafted()) - len(b)
        for i, (label, rays, which, made, hit, _, _) in enumerate(_expected(rt, orc, key)):
            g0 = np.random.default_rng(70 + i).integers(1, 2 ** 32, size=(len(rays), 4), dtype=np.uint32)
            wc, wg = o.trace_ray(depth, made, g0)
            if depth == 0:
                named = hit >= 0
                assert (hit < b.n_core).all() and np.array_equal(wc[named], np.array([chc.colour_of(k) for k in hit[named]], np.uint8).reshape(-1, 3)), label
                assert (wc[~named] == 0).all()
                want = b.want[which[which >= first] - first]
                m = which >= first
            else:  # a first leg's colour is its second leg's winner's
                m = (which >= 0) & (which < first)
                want = b.want[which[m]]
            assert m.any() and np.array_equal(wc[m], np.array([chc.colour_of(k) if k >= 0 else (0, 0, 0) for k in want], np.uint8).reshape(-1, 3)), label
            r, g = torch.from_numpy(np.array(rays)).cuda(), torch.from_numpy(g0.view(np.int32)).cuda()
            for sched in SCHEDULES:
                for counters in (False, True):
                    c, gg = s.traceRays(r, depth, rng=g, counters=counters, options=_opts(rt, sched))
                    assert np.array_equal(c.cpu().numpy(), wc), (label, sched, counters, np.flatnonzero((c.cpu().numpy() != wc).any(axis=1))[:8])
                    assert np.array_equal(gg.cpu().numpy().view(np.uint32), wg), (label, sched, counters)
            _assert_placement(rt, b)


@pytest.mark.parametrize("name", chc.FRAMES)
def test_frame_classes(rt, orc, name):
    """33 x 17 px at 12 spp, every camera ray in the class: rt_render fused and in two passes under the three schedules, both
    variants (PixelStats, rgb bytes, the counting variant's job counters); rt_camera_hits against the answer composed from the
    oracle's pieces (tests/camera_hit_cases.py): object ids, strike points -- the depths -- and rays of all 12 samples."""
    import torch

    objs, cam, w, h = chc.frame(name)
    s, o = rt.Scene.make(objs), orc.OracleScene(objs)
    acc, rgb, st = o.render_rows(w, h, cam.to_abi(), seed=5, threads=8)
    assert (2 * w + 1, 2 * h + 1) == (33, 17)
    A, lib = rt._abi, rt.lib
    for passes in (1, 2):
        for sched in SCHEDULES:
            for counters in (False, True):
                a = torch.zeros((2 * h + 1, 2 * w + 1, 4), dtype=torch.int32, device="cuda:0")
                g = torch.zeros((2 * h + 1, 2 * w + 1, 3), dtype=torch.uint8, device="cuda:0")
                got, opt, camabi = A.rt_stats(), A.rt_render_options(passes=passes, **sched), cam.to_abi()
                rt._lib.check(lib.rt_render_device_ex(s.handle, C.byref(camabi), w, h, 5, 0, 0, 1, 2 * h + 1, A.RT_RENDER_COUNTERS if counters else 0,
                                                      C.c_void_p(a.data_ptr()), C.c_void_p(g.data_ptr()), None, C.byref(opt), C.byref(got)))
                assert np.array_equal(a.cpu().numpy(), acc) and np.array_equal(g.cpu().numpy(), rgb), (name, passes, sched, counters)
                if counters:
                    got = got.as_dict()
                    assert {k: got[k] for k in COUNTERS} == {k: st[k] for k in COUNTERS}, (name, passes, sched)
    px = np.arange(33 * 17, dtype=np.int32)
    want = camera_hit_cases.compose(orc, o, cam.to_abi(), w, h, 5, px, 0, 12)
    assert (want.hit == (0 if name == "tiny" else -1)).all()
    if name == "tiny":
        t = np.linalg.norm(want.strike - want.rays[..., :3], axis=-1)
        assert (t >= 9e-5 * (1.0 - 1e-12)).all() and (t < 1e-4).all()  # the farther plane's depth
    for counters in (False, True):
        got = s.cameraHits(w, h, cam, px, sample_first=0, n_samples=12, seed=5, counters=counters)
        assert np.array_equal(np.asarray(got.hit_index), want.hit), (name, counters)
        assert _same_f64(np.asarray(got.strike), want.strike) and _same_f64(np.asarray(got.rays), want.rays), (name, counters)
        if counters:
            assert got.stats["prim_tests"] == int(want.counters[..., 1].sum())
