"""The TIMED kernel variant (no counters: the one bench.py times) held to the CPU oracle under the settings and placements that
decide its control flow and can never change a pixel: the lane scheduler's thresholds (yield_lanes, refill_lanes, the derived
leaf_wait, park_lanes, blocks_per_cu) at the ends of their ranges, and what csrc/rt_launch_plan.h picks for a launch (Lambert pool
in LDS at 32..64 entries or in global memory, hybrid node bytes, unit width, fused or two passes).  tests/test_launch_plan.py sees a
threshold that moved; it cannot see a kernel that is wrong at a placement the plan rightly chose.  Here every launch is rendered
and compared with the oracle, every placement a case names is ASSERTED from the plan the library reports for that launch
(rt_dev_last_launch_plan, hooks.last_launch_plan), and that plan is fed back to the CPU planner, which must decide the same on every
field.  Settings travel with the call (rt_render_options); nothing here touches a process-wide default."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import scenes
import texture_cases
from test_launch_plan import IN_ORDER, planner  # noqa: F401  (the CPU planner behind a text interface, built the same way)

gpu = pytest.mark.gpu

YIELD, REFILL, PARK, PASSES = (1, 2, 59, 60, 64), (1, 64), (-1, 1, 2, 0, 256), (1, 2)
# yield 59 gives leaf_wait = 64 exactly, 60 and 64 give it clamped; park -1 never parks, 0 is the default, 1 a pool of one entry.
# (yield_lanes, refill_lanes, park_lanes, passes): every pair of values of any two settings occurs (test_the_list_covers_every_pair)
PAIRS = (
    (1, 1, -1, 1), (1, 64, 1, 1), (1, 1, 2, 2), (1, 64, 0, 2), (1, 1, 256, 1),
    (2, 64, -1, 1), (2, 1, 1, 2), (2, 64, 2, 2), (2, 1, 0, 1), (2, 64, 256, 1),
    (59, 1, -1, 2), (59, 64, 1, 2), (59, 1, 2, 1), (59, 64, 0, 1), (59, 1, 256, 2),
    (60, 64, -1, 2), (60, 1, 1, 1), (60, 64, 2, 1), (60, 1, 0, 2), (60, 64, 256, 2),
    (64, 1, -1, 1), (64, 64, 1, 1), (64, 1, 2, 2), (64, 64, 0, 2), (64, 1, 256, 1),
)
CORNERS = ((1, 1, 0, 0), (1, 64, 0, 0), (64, 1, 0, 0), (64, 64, 0, 0))  # (yield, refill) at the default pool and pass choice
SCHEDULES = {name: PAIRS + CORNERS for name in ("small_final", "all_materials", "mostly_textured", "spheres_1300", "spheres_17000")}
COUNTERS = ("rays", "prim_tests", "reflections", "samples", "pixels_early")


def test_the_list_covers_every_pair():
    """No GPU: the committed list per scene holds every pair of values of the four scheduler settings and the four (yield, refill)
    corners at default park and passes, so that nobody thins it unseen."""
    values = (YIELD, REFILL, PARK, PASSES)
    assert set(SCHEDULES) == {"small_final", "all_materials", "mostly_textured", "spheres_1300", "spheres_17000"}
    for name, rows in SCHEDULES.items():
        assert len(set(rows)) == len(rows), name
        for a, b in itertools.combinations(range(4), 2):
            missing = set(itertools.product(values[a], values[b])) - {(r[a], r[b]) for r in rows}
            assert not missing, (name, a, b, sorted(missing))
        for y, r in itertools.product((1, 64), (1, 64)):
            assert (y, r, 0, 0) in rows, (name, y, r)


# ---- plumbing ----------------------------------------------------------------------------------------------------------------
def _knobs():
    """conftest.py's stress knobs change what fits where: placement assertions are skipped under them, pixel comparisons never."""
    return any(os.environ.get(k) for k in ("RTFS_BLOCK", "RTFS_CHUNK", "RTFS_PASSES"))


_ORACLE = {}


def _oracle(orc, key, objs, cam, w, h, seed, **rows):
    """The oracle frame, once per (scene, camera, seed)."""
    if key not in _ORACLE:
        _ORACLE[key] = orc.OracleScene(objs).render_rows(w, h, cam.to_abi(), seed=seed, threads=16, **rows)
    return _ORACLE[key]


class Launches:
    """Renders and ray lists with per-call options; keeps the plan the library reports for each."""

    def __init__(self, rt):
        self.rt, self.plans = rt, []

    def _plan(self):
        plan = self.rt.hooks.last_launch_plan()
        assert plan is not None
        self.plans.append(plan)
        return plan

    def render(self, s, cam, w, h, seed, counters=False, row_first=0, n_rows=None, **opt):
        import torch

        A, lib = self.rt._abi, self.rt.lib
        rows, cols = 2 * h + 1, 2 * w + 1
        n_rows = rows - row_first if n_rows is None else n_rows
        accum = torch.zeros((n_rows, cols, 4), dtype=torch.int32, device="cuda:0")
        rgb = torch.zeros((n_rows, cols, 3), dtype=torch.uint8, device="cuda:0")
        st, o, camabi = A.rt_stats(), A.rt_render_options(**opt), cam.to_abi()
        self.rt._lib.check(lib.rt_render_device_ex(s.handle, C.byref(camabi), w, h, seed, 0, row_first, 1, n_rows, A.RT_RENDER_COUNTERS if counters else 0,
                                                   C.c_void_p(accum.data_ptr()), C.c_void_p(rgb.data_ptr()), None, C.byref(o), C.byref(st)))
        plan = self._plan()
        assert plan["in"]["count"] == int(counters) and plan["in"]["kind"] == 0
        return accum.cpu().numpy(), rgb.cpu().numpy(), st.as_dict(), plan

    def stage_stats(self):
        ss = (C.c_uint64 * 16)()
        assert self.rt.lib.rt_last_stage_stats(ss) == 0
        return list(ss)

    def check_against(self, planner):  # noqa: F811
        """Every plan the device reported, recomputed by the CPU planner from the reported inputs: equal on every field."""
        assert self.plans
        got = planner([p["in"] for p in self.plans])
        wrong = [(p["in"], {k: (p["out"].get(k), g.get(k)) for k in set(p["out"]) | set(g) if p["out"].get(k) != g.get(k)})
                 for p, g in zip(self.plans, got) if p["out"] != g]
        assert not wrong, wrong[:3]


def _passes_of(plan):
    return [p for p in "FAB" if f"{p}_grid" in plan["out"]]


def _opts(y, r, park, passes, **more):
    return dict(yield_lanes=y, refill_lanes=r, park_lanes=park, passes=passes, **more)


def _assert_schedule(plan, y, r, park):
    """The launch ran at the thresholds asked for (not under the stress knobs' either: these are not among them)."""
    for p in _passes_of(plan):
        o = plan["out"]
        assert (o[f"{p}_yield"], o[f"{p}_refill"], o[f"{p}_leaf_wait"]) == (y, r, min(64, y + 5)), (p, o)
        assert o[f"{p}_park"] == (0 if park < 0 else (park or 96)) and (o[f"{p}_park_l"] > 0) == (park >= 0), (p, o)


def _schedule_scene(rt, name):
    """(objects, camera, w, h, seed, placement check).  The placement check reads the reported plan of a TIMED launch."""
    def resident(plan, park):
        o, i = plan["out"], plan["in"]
        assert o["q_lds"] == 1 and i["n_obj"] < 16384, o
        for p in _passes_of(plan):
            assert o[f"{p}_lds_node_bytes"] == 0, o

    if name == "small_final":
        objs, cam, w, h = scenes.small_final()

        def check(plan, park):  # LDS-resident, the Lambert pool in LDS and full-sized: 64 entries beside the narrow units of the two
            resident(plan, park)  # passes, 62 beside the fused kernel's 16-pixel units (89296 B of scene + 18432 B of scratch leave 62.6 x 896 B)
            assert plan["out"]["q_tex"] == 0
            for p in _passes_of(plan):
                cap, in_lds = plan["out"][f"{p}_park_l"], plan["out"][f"{p}_park_l_lds"]
                full = ({"F": 62, "A": 64, "B": 64}[p], 1)  # (a tuned tree is smaller: under RTFS_TUNE=1 the fused pool may reach 64 too)
                ok = (cap, in_lds) == full or (os.environ.get("RTFS_TUNE") == "1" and 62 <= cap <= 64 and in_lds == 1)
                assert ok if park >= 0 else (cap, in_lds) == (0, 0), plan["out"]
        return objs, cam, w, h, 21, check
    if name == "all_materials":
        objs, cam, w, h = scenes.all_materials()

        def check(plan, park):  # every style: the general pool and stage_slow; its two parameterised textures: the TEX variants
            resident(plan, park)
            assert plan["out"]["q_tex"] == 1
        return objs, cam, w, h, 22, check
    if name == "mostly_textured":
        objs, cam, w, h = texture_cases.mostly_textured_scene()

        def check(plan, park):  # the TEX variants, stage_tex and pool_t() behind a Lambert pool that is in LDS
            resident(plan, park)
            assert plan["out"]["q_tex"] == 1
            for p in _passes_of(plan):
                assert plan["out"][f"{p}_park_l_lds"] == (1 if park >= 0 else 0), plan["out"]
        return objs, cam, w, h, 23, check
    n = {"spheres_1300": 1300, "spheres_17000": 17000}[name]
    objs, cam, w, h = scenes.many_spheres(n=n, seed=40 + n % 7, spp=20, depth=10, pixels=12)

    def check(plan, park):  # beyond the LDS: node_loop_hyb16 below 16384 objects (16-bit queue entries), node_loop_glb32 from there on
        o, i = plan["out"], plan["in"]
        assert o["q_lds"] == 0 and (i["n_obj"] >= 16384) == (n == 17000), (o, i)
        for p in _passes_of(plan):
            assert 0 < o[f"{p}_lds_node_bytes"] <= 64 * i["n_nodes"], o
    return objs, cam, w, h, 24, check


# ---- a. the ends of the schedule, per placement --------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_schedule_ends_leave_every_pixel_alone(rt, orc, planner, name):  # noqa: F811
    """The timed kernel at the ends of yield_lanes, refill_lanes and park_lanes, fused and in two passes, against the oracle: every
    PixelStats and every rgb byte.  The four (yield, refill) corners also render the counting variant, whose job counters must be
    the oracle's.  The first launch is Scene.render_rows at the defaults (under RTFS_TUNE=1 that tunes the scene first)."""
    objs, cam, w, h, seed, placement = _schedule_scene(rt, name)
    s, L = rt.Scene.make(objs), Launches(rt)
    acc, rgb, st = _oracle(orc, name, objs, cam, w, h, seed)
    first = s.render_rows(w, h, cam, seed=seed)
    assert np.array_equal(first.accum, acc) and np.array_equal(first.rgb, rgb), "defaults"
    for y, r, park, passes in SCHEDULES[name]:
        a, g, _, plan = L.render(s, cam, w, h, seed, **_opts(y, r, park, passes))
        print(name, (y, r, park, passes), {k: v for k, v in plan["out"].items() if k[0] in "FAB" and k[2:] in ("chunk", "park", "park_l", "park_l_lds", "lds_node_bytes", "leaf_wait")})
        _assert_schedule(plan, y, r, park)
        if passes:
            assert plan["out"]["two_pass"] == passes - 1, plan
        if not _knobs():
            placement(plan, park)
        assert np.array_equal(a, acc) and np.array_equal(g, rgb), (name, y, r, park, passes)
        if (y, r, park, passes) in CORNERS:
            a, g, cst, _ = L.render(s, cam, w, h, seed, counters=True, **_opts(y, r, park, passes))
            assert np.array_equal(a, acc) and np.array_equal(g, rgb), (name, y, r, "counted")
            assert {k: cst[k] for k in COUNTERS} == {k: st[k] for k in COUNTERS}, (name, y, r)
    L.check_against(planner)


@gpu
@pytest.mark.parametrize("name", ["small_final", "spheres_1300"])
def test_grid_block_and_unit_singles(rt, orc, planner, name):  # noqa: F811
    """blocks_per_cu 1 and 8 (never rendered before), every block size with a whole wave yielding and refilling at once, units of
    1 and 64 pixels with every lane yielding and refilling alone: timed against the oracle, counted for the job counters."""
    objs, cam, w, h, seed, placement = _schedule_scene(rt, name)
    s, L = rt.Scene.make(objs), Launches(rt)
    acc, rgb, st = _oracle(orc, name, objs, cam, w, h, seed)
    singles = [dict(blocks_per_cu=1), dict(blocks_per_cu=8)]
    singles += [dict(block_threads=b, yield_lanes=64, refill_lanes=64) for b in (256, 512, 768, 1024)]
    singles += [dict(chunk_pixels=c, yield_lanes=1, refill_lanes=1) for c in (1, 64)]
    for opt in singles:
        a, g, _, plan = L.render(s, cam, w, h, seed, **opt)
        o, i = plan["out"], plan["in"]
        assert (i["s_bpc"], i["s_block"], i["s_chunk"]) == (opt.get("blocks_per_cu", 0), opt.get("block_threads", 0), opt.get("chunk_pixels", 0))
        if "blocks_per_cu" in opt:  # the grid is what the setting allows, whatever the occupancy query answered
            units = -(-i["n_rows"] * (2 * i["max_w"] + 1) // o["F_chunk"])
            assert o["F_grid"] == min(i["cu_count"] * min(i["per_cu"], opt["blocks_per_cu"]), -(-units // (o["q_block"] // 64))), plan
        if "block_threads" in opt:
            assert o["q_block"] == opt["block_threads"] and (o["F_yield"], o["F_refill"], o["F_leaf_wait"]) == (64, 64, 64), plan
        if "chunk_pixels" in opt:
            assert o["F_chunk"] == opt["chunk_pixels"] and (o["F_yield"], o["F_refill"], o["F_leaf_wait"]) == (1, 1, 6), plan
        assert np.array_equal(a, acc) and np.array_equal(g, rgb), (name, opt)
        a, g, cst, _ = L.render(s, cam, w, h, seed, counters=True, **opt)
        assert np.array_equal(a, acc) and np.array_equal(g, rgb), (name, opt, "counted")
        assert {k: cst[k] for k in COUNTERS} == {k: st[k] for k in COUNTERS}, (name, opt)
    L.check_against(planner)


# ---- b. ray lists ----------------------------------------------------------------------------------------------------------------
def _same_f64(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def _list_rays(cam, n, seed):
    """Rays as a caller hands them over: most from the camera's eye into its view, some from anywhere; vectors of any length, a few
    that Ray.make' refuses."""
    rng = np.random.default_rng(seed)
    eye, fwd = np.array(cam.abi.view_origin[:]), np.array(cam.abi.view_dir[:])
    raw = np.concatenate([np.concatenate([np.tile(eye, (n - n // 4, 1)), fwd + rng.normal(size=(n - n // 4, 3)) * 0.4], axis=1),
                          scenes.random_rays(n // 4, seed + 1, origin_scale=4.0)])
    raw[:, 3:] *= (10.0 ** rng.uniform(-3.0, 3.0, len(raw)))[:, None]
    raw[:6, 3:] = 0.0
    return raw


def _made(orc, raw):
    ok = np.zeros(len(raw), bool)
    made = np.zeros_like(raw)
    for i, r in enumerate(raw):
        m = orc.ray_make(r[:3], r[3:])
        if m is not None:
            ok[i], made[i] = True, m
    return made[ok], ok


@gpu
@pytest.mark.parametrize("name", ["small_final", "spheres_1300", "mostly_textured"])
def test_ray_lists_at_the_schedule_corners(rt, orc, planner, name):  # noqa: F811
    """rt_trace_rays_device (depth 0 and 12) and rt_hit_objects_device at the four (yield, refill) corners x park {-1, 1, default},
    on an LDS-resident scene, a hybrid one and a textured one: colours, final generator states, hit indices and strike points are
    the oracle's, bit for bit."""
    import torch

    A = rt._abi
    objs, cam, _, _, seed, _ = _schedule_scene(rt, name)
    s, o, L = rt.Scene.make(objs), orc.OracleScene(objs), Launches(rt)
    raw = _list_rays(cam, 6000, seed)
    made, ok = _made(orc, raw)
    g0 = np.random.default_rng(seed).integers(1, 2**32, size=(len(raw), 4), dtype=np.uint32)
    want_hit, want_strike = np.full(len(raw), -2, np.int32), np.full((len(raw), 3), np.nan)
    want_hit[ok], want_strike[ok] = o.hit_object(made)[:2]
    want = {}
    for depth in (0, 12):
        col, g = np.zeros((len(raw), 3), np.uint8), g0.copy()
        col[ok], g[ok] = o.trace_ray(depth, made, g0[ok])
        want[depth] = (col, g)
    assert (want_hit == -2).sum() == (~ok).sum() >= 6 and np.mean(want_hit >= 0) > 0.2 and len(np.unique(want[12][0], axis=0)) > 20
    r, g = torch.from_numpy(raw).cuda(), torch.from_numpy(g0.view(np.int32)).cuda()
    for (y, rf), park in itertools.product(itertools.product((1, 64), (1, 64)), (-1, 1, 0)):
        opt = A.rt_render_options(yield_lanes=y, refill_lanes=rf, park_lanes=park)
        for depth in (0, 12):
            c, gg = s.traceRays(r, depth, rng=g, options=opt)
            plan = L._plan()
            assert plan["in"]["kind"] == 1 and plan["out"]["F_mode"] == 4 and plan["out"]["q_tex"] == int(name == "mostly_textured"), plan
            _assert_schedule(plan, y, rf, park)
            assert np.array_equal(c.cpu().numpy(), want[depth][0]), (name, y, rf, park, depth)
            assert np.array_equal(gg.cpu().numpy().view(np.uint32), want[depth][1]), (name, y, rf, park, depth)
        hi, sk = s.hitObject(r, options=opt)
        plan = L._plan()
        assert plan["in"]["kind"] == 2 and plan["out"]["F_mode"] == 5 and (plan["out"]["F_yield"], plan["out"]["F_refill"]) == (y, rf), plan
        if not _knobs():
            assert plan["out"]["q_lds"] == int(name != "spheres_1300") and (plan["out"]["F_lds_node_bytes"] > 0) == (name == "spheres_1300"), plan
        assert np.array_equal(hi.cpu().numpy(), want_hit) and _same_f64(sk.cpu().numpy(), want_strike), (name, y, rf, park)
    L.check_against(planner)


# ---- c. the Lambert pool's placements, timed ------------------------------------------------------------------------------------
def _band_scene(rt, n, textured, spp=14, pixels=14):
    """scenes.many_spheres(seed=6) in the band where the timed image (184 B per sphere) leaves the LDS room for a Lambert pool of
    64 entries per wave, of fewer, or of none; `textured` puts a parameterised texture on one Lambert sphere, which makes every
    launch the TEX variant (test_tree_partly_in_lds does the same)."""
    objs, cam, w, h = scenes.many_spheres(n=n, seed=6, spp=spp, depth=8, pixels=pixels)
    objs = list(objs)
    if textured:
        chk = rt.ParameterisedTexture.Checkered(rt.ParameterisedTexture.UvRamp("u", 40, "v"), rt.ParameterisedTexture.Colour(rt.Pixel(20, 60, 20)), 30.0)
        centre = rt.Point.make(0.0, 1.0, 2.0)
        objs[3] = rt.Hittable.Sphere(rt.Sphere.make(rt.SphereStyle.LambertReflection(0.8, rt.ParameterisedTexture.toTexture((0.9, centre), chk)), centre, 0.9))
    return objs, cam, w, h


# name: (spheres, textured, pixels, passes, which pass, (capacity test, in LDS) expected of that pass)
POOL_CASES = {
    "lds_64": (450, False, 14, 1, "F", (lambda c: c == 64, 1)),
    "lds_between": (520, False, 14, 1, "F", (lambda c: c == 54, 1)),  # 95728 B of scene + 18432 B of scratch leave 55.4 x 896 B
    "lds_32": (630, False, 14, 1, "F", (lambda c: c == 32, 1)),
    "global_scene_resident": (640, False, 14, 1, "F", (lambda c: c == 64, 0)),
    "pass_a_narrowed": (600, False, 360, 2, "A", (lambda c: c == 44, 1)),  # 923 kpx: wide enough for 32-pixel units in pass A; 110448 B + 13312 B leave 44.7 x 896 B
    "tex_lds": (450, True, 14, 1, "F", (lambda c: c == 64, 1)),
    "tex_global": (640, True, 14, 1, "F", (lambda c: c == 64, 0)),
}


@gpu
@pytest.mark.parametrize("case", sorted(POOL_CASES))
def test_lambert_pool_placements(rt, orc, planner, case):  # noqa: F811
    """The Lambert pool where the plan puts it -- 64 entries in LDS, fewer, exactly 32, in global memory beside an LDS-resident
    scene, beside a pass A narrowed to 16-pixel units so that it fits, and behind both forms of pool_t() in the TEX variant -- each
    placement asserted from the reported plan, each rendered by the timed kernel at the default schedule and at yield 64 / refill
    64, where a whole wave shades at once and more lanes want to park than the pool has room for (stage_shade's `rank < room`
    false branches).

    NOT asserted: that the `rank < room` false branch is reached.  It was meant to be read off rt_last_stage_stats of a counting
    render with the same options, as "lanes shaded per shade stage exceed the pool's capacity".  That mean cannot serve: a wave
    has 64 lanes, so no mean exceeds a pool of 64 entries; and at refill 64 new items are handed out only when all lanes are
    idle, shaded together once, and then only the survivors of each generation come back, so the mean is 32..35 lanes whatever
    the capacity (measured at 520 spheres, 14 spp: 27228 lanes in 805 stages, capacity 54; at 630 spheres: 27775 in 864,
    capacity 32).  The statistics of the product build count the lanes parked in the GENERAL pool and the lanes through
    stage_slow, none through stage_lamb or into the Lambert pool, and the counting variant's schedule is not the timed one's
    anyway.  The figures are printed; NOTES.md records this as a deviation from what the test was asked to assert."""
    n, textured, pixels, passes, which, (cap_ok, in_lds) = POOL_CASES[case]
    objs, cam, w, h = _band_scene(rt, n, textured, pixels=pixels)
    s, L = rt.Scene.make(objs), Launches(rt)
    acc, rgb, st = _oracle(orc, ("band", n, textured, pixels), objs, cam, w, h, 9)  # (no Scene.render_rows here: a tuned tree is smaller, and the sizes are the case)
    for sched in (dict(), dict(yield_lanes=64, refill_lanes=64)):
        a, g, _, plan = L.render(s, cam, w, h, 9, passes=passes, **sched)
        o = plan["out"]
        cap = o.get(f"{which}_park_l")
        print(case, sched, {k: v for k, v in o.items() if k[0] in "FAB" and k[2:] in ("chunk", "park", "park_l", "park_l_lds", "lds_bytes")})
        if not _knobs():
            assert o["q_lds"] == 1 and o["q_tex"] == int(textured) and o["two_pass"] == passes - 1, plan
            assert cap_ok(cap) and o[f"{which}_park_l_lds"] == in_lds, plan
            if case == "pass_a_narrowed":  # without the pool, pass A's units would be 32 pixels wide: they fit the LDS, the pool beside them does not
                assert o["A_chunk"] == 16 and plan["in"]["lds32_total"] + 16 * 13 * 32 * 4 <= 163840 < plan["in"]["lds32_total"] + 16 * 13 * 32 * 4 + 16 * 56 * 32, plan
        assert np.array_equal(a, acc) and np.array_equal(g, rgb), (case, sched)
        if sched:
            a, g, cst, cplan = L.render(s, cam, w, h, 9, counters=True, passes=passes, **sched)
            ss = L.stage_stats()
            assert np.array_equal(a, acc) and {k: cst[k] for k in COUNTERS} == {k: st[k] for k in COUNTERS}, case
            print(case, "Lambert pool, counting render: shade stages", ss[3], "lanes shaded", ss[5], "per stage", ss[5] / max(1, ss[3]), "timed capacity", cap)
            print(case, "general pool, counting render: lanes parked", ss[11], "lanes through stage_slow", ss[10], "in", ss[9], "stages")
    L.check_against(planner)


# ---- d. widened fused units, timed -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("pixels,spp,chunk,pool", [(400, 16, 32, (42, 1)), (800, 4, 64, (64, 0))])
def test_widened_fused_units(rt, orc, planner, pixels, spp, chunk, pool):  # noqa: F811
    """Config 3's scene at 1201x801 / 16 spp (32-pixel units, a Lambert pool of 42 entries in LDS beside them) and 2401x1601 / 4 spp
    (64-pixel units, the pool in global memory): the whole frame by the timed kernel against the oracle, at the default schedule
    and at yield 64 / refill 64; the unit width and the pool are asserted from the reported plan."""
    import time

    objs, cam, w, h = rt.sample_images.config3_final(seed=2024, spp=spp, depth=50, pixels=pixels)
    assert (2 * w + 1, 2 * h + 1) == {400: (1201, 801), 800: (2401, 1601)}[pixels]
    s, L = rt.Scene.make(objs), Launches(rt)
    t0 = time.time()
    acc, rgb, st = _oracle(orc, ("config3", pixels, spp), objs, cam, w, h, 2024)
    print(f"oracle {2 * w + 1}x{2 * h + 1} at {spp} spp: {time.time() - t0:.1f} s, {st['rays']} rays")
    for sched in (dict(), dict(yield_lanes=64, refill_lanes=64)):  # (no Scene.render_rows here: a tuned tree is smaller, and the sizes are the case)
        a, g, _, plan = L.render(s, cam, w, h, 2024, **sched)
        o = plan["out"]
        if not _knobs():
            assert o["q_lds"] == 1 and o["two_pass"] == 0 and o["F_chunk"] == chunk and (o["F_park_l"], o["F_park_l_lds"]) == pool, plan
        assert np.array_equal(a, acc) and np.array_equal(g, rgb), (pixels, sched)
    a, g, cst, _ = L.render(s, cam, w, h, 2024, counters=True)
    assert np.array_equal(a, acc) and {k: cst[k] for k in COUNTERS} == {k: st[k] for k in COUNTERS}
    L.check_against(planner)


# ---- the device's plan against the CPU planner, live ----------------------------------------------------------------------------
@gpu
def test_the_reported_plan_is_the_cpu_planners(rt, planner):  # noqa: F811
    """Every kind of launch -- fused, two passes, counted, a row block, an empty shard, the tune probe, both ray lists -- reports
    through rt_dev_last_launch_plan the inputs the library gathered (scene sizes, resolved settings, CU count, the occupancy
    answer) and the decisions it executed; the CPU planner, given those inputs, decides the same on every field.  The reported
    inputs are themselves checked against what the caller asked for."""
    import torch

    A = rt._abi
    objs, cam, w, h = scenes.small_final(spp=40, pixels=12)
    s, L = rt.Scene.make(objs), Launches(rt)
    rows = 2 * h + 1
    info = s.info()
    for counters, opt in itertools.product((False, True), (dict(), dict(passes=2), dict(passes=1, block_threads=256, chunk_pixels=8, blocks_per_cu=2),
                                                            dict(yield_lanes=61, refill_lanes=3, park_lanes=-1), dict(park_lanes=7, passes=2, block_threads=512))):
        _, _, st, plan = L.render(s, cam, w, h, 1, counters=counters, **opt)
        i, o = plan["in"], plan["out"]
        assert (i["n_nodes"], i["n_obj"], i["has_tex"]) == (info["walk_tree_nodes"], info["n_bounded"] + info["n_unbounded"], 0)
        assert (i["n_rows"], i["max_w"], i["spp"], i["log"], i["n"]) == (rows, w, 40, 0, 0) and i["cu_count"] > 0 and i["per_cu"] >= 1
        want = dict(s_block=0, s_chunk=0, s_bpc=0, s_yield=0, s_refill=0, s_passes=0, s_park=0)
        want.update({{"block_threads": "s_block", "chunk_pixels": "s_chunk", "blocks_per_cu": "s_bpc", "yield_lanes": "s_yield", "refill_lanes": "s_refill",
                      "passes": "s_passes", "park_lanes": "s_park"}[k]: v for k, v in opt.items()})
        if not _knobs():
            assert {k: i[k] for k in want} == want, (i, opt)
        assert st["pixels"] == rows * (2 * w + 1) and o["error"] == 0
        for p in _passes_of(plan):
            assert o[f"{p}_lds_bytes"] <= 163840 and o[f"{p}_grid"] <= i["cu_count"] * i["per_cu"], plan
    _, _, _, plan = L.render(s, cam, w, h, 1, row_first=3, n_rows=5)
    assert plan["in"]["n_rows"] == 5
    _, _, _, plan = L.render(s, cam, w, h, 1, row_first=0, n_rows=0)
    assert plan["in"]["n_rows"] == 0 and plan["out"]["F_grid"] == 0
    s.tune(w, h, cam, seed=1)
    plan = L._plan()
    assert plan["in"]["log"] == 1 and plan["out"]["F_mode"] == 3 and plan["in"]["n_nodes"] == info["walk_tree_nodes"]
    r = torch.from_numpy(_list_rays(cam, 5000, 3)).cuda()
    for opt in (None, A.rt_render_options(block_threads=256, chunk_pixels=16), A.rt_render_options(block_threads=512, park_lanes=-1)):
        s.traceRays(r, 5, seed=2, options=opt)
        plan = L._plan()
        assert (plan["in"]["kind"], plan["in"]["n"], plan["out"]["F_mode"]) == (1, 5000, 4)
        s.hitObject(r, counters=True, options=opt)
        plan = L._plan()
        assert (plan["in"]["kind"], plan["in"]["n"], plan["in"]["count"], plan["out"]["F_mode"], plan["out"]["F_park"]) == (2, 5000, 1, 5, 0)
    assert len(IN_ORDER) == len(rt.hooks.PLAN_INPUTS) and tuple(IN_ORDER) == tuple(rt.hooks.PLAN_INPUTS)
    L.check_against(planner)
