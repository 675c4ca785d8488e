"""The two sphere-test sites of the render kernel (csrc/rt_device.h: `sphere_first_intersection` in the unbounded tests,
`leaf_test_object_exact` in the leaf pass) and `unitise` against the oracle, with no tolerance, on the rays of
tests/sphere_arm_cases.py: the Equal arm of the discriminant runs behind a wave-uniform guard (and the unit hook's +inf
fix-up of the square root behind another), so the rays that need them are placed at chosen lanes of chosen waves (none, lane 0 alone, lane 63 alone, every second
lane, all 64) in lists of 64, 65 and 192 rays, under the default schedule and under yield 64 / refill 64 and yield 1 / refill 1.
Routes: Scene.hitObject timed and counting, Scene.traceRays at depth 2 (bounce rays that START on the tangent point's surface),
one 33 x 17 px render fused and in two passes.  Scenes: (a) resident in LDS, (b) padded past it, (c) the reflection zoo, and (a)
with a sphere of radius 1e160 (every discriminant +inf), unbounded and bounded."""
import numpy as np
import pytest

import sphere_arm_cases as sac

pytestmark = pytest.mark.gpu

SCHEDULES = (dict(), dict(yield_lanes=64, refill_lanes=64), dict(yield_lanes=1, refill_lanes=1))
SCENES = {"base": (sac.base_objects, "base"), "padded": (sac.padded_objects, "base"), "zoo": (sac.zoo_objects, "zoo"),
          "inf_unbounded": (lambda: sac.inf_objects(False), "base"), "inf_bounded": (lambda: sac.inf_objects(True), "base")}
COUNTERS = ("rays", "prim_tests", "reflections", "samples", "pixels_early")
_PAIRS = {}


def _pair(rt, orc, name):
    if name not in _PAIRS:
        objs = SCENES[name][0]()
        _PAIRS[name] = (rt.Scene.make(objs), orc.OracleScene(objs), objs)
    return _PAIRS[name]


def _lists(name):
    cls = sac.classes(SCENES[name][1])
    if name in ("base", "padded"):
        return sac.all_lists(cls)
    return sac.all_lists(cls, sizes=(192,))  # the other scenes: every pattern once per rare class


def _same_f64(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def _made(orc, raw):
    ok, made = np.zeros(len(raw), bool), np.zeros_like(raw)
    for i, r in enumerate(raw):
        m = orc.ray_make(r[:3], r[3:])
        if m is not None:
            ok[i], made[i] = True, m
    return made, ok


def _opts(rt, sched):
    return rt._abi.rt_render_options(**sched) if sched else None


def _assert_placement(rt, name):
    plan = rt.hooks.last_launch_plan()
    if name == "padded":
        assert plan["out"]["q_lds"] == 0, plan  # the LDS = false kernels
    elif name in ("base", "inf_unbounded"):
        assert plan["out"]["q_lds"] == 1, plan


@pytest.mark.parametrize("name", sorted(SCENES))
def test_hit_object_in_every_lane_pattern(rt, orc, name):
    """Scene.hitObject, the timed kernel and the counting one: hit index and strike point of every ray of every list are the
    oracle's, bit for bit, and the counting launch's rays and Hittable.hits calls are the oracle's sums."""
    import torch

    s, o, objs = _pair(rt, orc, name)
    lists = _lists(name)
    raw = np.concatenate([r for _, r, _ in lists])
    made, ok = _made(orc, raw)
    assert ok.all()
    hit, strike, cnt = o.hit_object(made)
    assert (hit >= 0).mean() > 0.3 and ((hit < 0).any() or name == "zoo")  # (the zoo is closed in by its planes)
    at = 0
    for label, rays, rare in lists:
        n = len(rays)
        wh, ws, wc = hit[at:at + n], strike[at:at + n], cnt[at:at + n]
        at += n
        ws = np.where((wh >= 0)[:, None], ws, np.nan)
        r = torch.from_numpy(rays).cuda()
        for sched in SCHEDULES:
            for counters in (False, True):
                hi, sk = s.hitObject(r, counters=counters, options=_opts(rt, sched))
                assert np.array_equal(hi.cpu().numpy(), wh), (name, label, sched, counters, np.flatnonzero(hi.cpu().numpy() != wh)[:8], rare[:8])
                assert _same_f64(sk.cpu().numpy(), ws), (name, label, sched, counters)
                if counters:
                    st = s.last_stats
                    assert st["rays"] == n and st["prim_tests"] == int(wc[:, 1].sum()), (name, label, sched, st)
        _assert_placement(rt, name)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_trace_rays_that_bounce_off_the_tangent_point(rt, orc, name):
    """Scene.traceRays at depth 2: the first hit is found as above; the bounce then starts ON the surface it left (its own sphere's
    discriminant is b^2 to rounding: Equal when it leaves at a grazing angle) and goes through both sites and `unitise` again.
    Colours and final generator states are the oracle's."""
    import torch

    s, o, objs = _pair(rt, orc, name)
    lists = [l for l in _lists(name) if l[0].endswith("/192") or l[0].endswith("/65")]
    for i, (label, rays, rare) in enumerate(lists):
        made, ok = _made(orc, rays)
        g0 = np.random.default_rng(900 + i).integers(1, 2 ** 32, size=(len(rays), 4), dtype=np.uint32)
        wc, wg = o.trace_ray(2, made, g0)
        r, g = torch.from_numpy(rays).cuda(), torch.from_numpy(g0.view(np.int32)).cuda()
        for sched in SCHEDULES:
            for counters in (False, True):
                c, gg = s.traceRays(r, 2, rng=g, counters=counters, options=_opts(rt, sched))
                assert np.array_equal(c.cpu().numpy(), wc), (name, label, sched, counters)
                assert np.array_equal(gg.cpu().numpy().view(np.uint32), wg), (name, label, sched, counters)
    assert len(lists) >= 20


@pytest.mark.parametrize("name", ["base", "padded", "inf_bounded", "inf_unbounded"])
def test_a_small_render_fused_and_in_two_passes(rt, orc, name):
    """33 x 17 px at 12 spp: every PixelStats and rgb byte by the timed kernel, fused and in two passes, under the three schedules;
    the counting variant's PixelStats and its four job counters besides."""
    import ctypes as C

    import torch

    s, o, objs = _pair(rt, orc, name)
    cam, w, h = sac.camera()
    acc, rgb, st = o.render_rows(w, h, cam.to_abi(), seed=5, threads=8)
    assert (2 * w + 1, 2 * h + 1) == (33, 17) and st["rays"] > 33 * 17 * 12
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


def test_unitise_of_an_infinite_squared_norm(rt):
    """inv_sqrt_above_tol / sqrt_above_tol (the hook of test_normal_range_sqrt_and_reciprocal) with +inf operands -- what `unitise`
    sees for a vector whose squared norm overflows -- in no lane of a wave, in one (the first, the last), in every second and in
    all, among ordinary operands: 1 / sqrt(+inf) = +0.0 and sqrt(+inf) = +inf as the host computes them, and no neighbour changed."""
    rng = np.random.default_rng(8)
    for n in (64, 65, 192, 4096):
        for pattern in sac.PATTERNS:
            x = np.exp(rng.uniform(np.log(1e-8), np.log(1e300), n))
            x[sac.rare_lanes(pattern, n)] = np.inf
            with np.errstate(divide="ignore"):
                want_sqrt = np.sqrt(x)
                want_inv = 1.0 / want_sqrt
            got_sqrt, got_inv = rt.hooks.arith(5, x), rt.hooks.arith(6, x)
            assert _same_f64(got_sqrt, want_sqrt), (n, pattern)
            assert _same_f64(got_inv, want_inv) and not np.signbit(got_inv[np.isinf(x)]).any(), (n, pattern)
