"""Hittable.Reflection on the device against the oracle, bit for bit, on the vertex classes of tests/reflection_cases.py (material,
incidence and generator edges; tests/test_reflection_model.py pins the oracle on them to the line-by-line restatement and holds the
classes to their coverage conditions).  Three ways in:

* the hook (`rt.hooks.reflection`, the general `reflection`) on every class, plain and textured zoo;
* Scene.traceRays with the classes' rays and generator states, so that each ray's first vertex is the class's vertex, at depth 0,
  1, 2 and 8, in two witness scenes (an image-textured light sphere around the textured zoo: the TEX kernels; six coloured light
  planes around the plain zoo: the non-TEX kernels), LDS-resident and not, counting and timed variant, parked and unparked,
  256 and 1024 threads: `reflection_fast`, `lambert_inside` + `lambert_bounce`, `stage_slow` over the park pool and `stage_tex`
  feeding `texPre`, each against the oracle and not merely against each other;
* Scene.renderFootprints with du = dv = 0 and base = the class's ray, fused and two-pass: the same routes under the frame scheduler.

There is no tolerance anywhere in this file.

NaN rays.  For sinO in (1, 1 + 1e-8] Float.compare says Equal, sqrt(1 - sinO^2) is NaN and Ray.overwriteWithMake accepts the NaN
vector (|v|^2 = NaN is not within 1e-8 of 0): the outgoing ray has a finite origin (the strike) and a NaN direction, and misses
everything.  Why each loop that ray enters ends, read from csrc/rt_device.h (a NaN origin never arises: origins are strikes):
  node_loop_lds32, node_loop_hyb16, node_loop_glb32 -- rcp(NaN) and every fma of the filter are NaN; v_max3/v_min3 and v_max(0, .)
    drop NaN operands, so tn = 0 and tf = NaN, and `v_cmp_nlt` is true: a hit.  Hit or miss, a stepping lane's position is
    REPLACED by one of its record's two links, both of which lead forward in pre-order (on_hit: the next record, on_miss: the
    end of the subtree), so the pre-order rank rises with every visit and reaches `end` after at most n_nodes visits.  A full
    queue only makes the lane sit out until the leaf pass has popped an entry; the loop itself leaves when no more than `stop`
    lanes can step.
  node_loop_lds and node_step (counting variant) -- 1 / NaN = NaN, the products are NaN, v_max_f64 / v_min_f64 (fmax / fmin) keep
    the other operand: tMin = 0, tMax = +inf, a hit; the same forward links.
  the leaf pass (leaf_test, leaf_test_object, leaf_test_object_exact) -- straight-line code: b, disc and both roots are NaN,
    `fpos` fails, t = NaN, t * t compares neither below nor equal to bestF: no candidate, so the exact box test of the sliver
    (three divisions, no loop) is not even entered.  sqrt_core / rcp_core are fma chains without a loop.
  unbounded_tests -- one pass over the unbounded objects; plane and sphere intersections return NaN, `t == t` fails.
  the retry loops (random_unit; the Lambert / fuzz loops of `reflection` and lambert_bounce) -- never entered by a NaN ray, which
    hits nothing; and were one entered, `unitise` fails only for |v|^2 within 1e-8 of 0, which NaN is not: NaN ends such a loop.
So a NaN ray walks the whole tree once, tests every leaf the filter queues, and its path ends Black.  The classes whose outgoing
rays can be NaN (reflection_cases.NAN_CLASSES) have test functions of their own below."""
import ctypes
import functools

import numpy as np
import pytest

import footprint_cases as fc
import reflection_cases as rc
from test_gpu_ray_queries import _oracle_trace

pytestmark = pytest.mark.gpu

NAMES = [name for name, _ in rc.CLASSES]
FINITE = [name for name in NAMES if name not in rc.NAN_CLASSES]
WITNESSES = [("tex", False), ("planes", False), ("tex", True), ("planes", True)]
DEPTHS = [0, 1, 2, 8]
HOTPINK = (205, 105, 180)


def _same_f64(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


@functools.lru_cache(maxsize=None)
def _zoo_pair(rt, orc, textured):
    objs = rc.zoo(textured).objs
    return rt.Scene.make(objs), orc.OracleScene(objs)


@functools.lru_cache(maxsize=None)
def _witness_pair(rt, orc, kind, cluster):
    objs = rc.witness(kind, cluster)
    return rt.Scene.make(objs), orc.OracleScene(objs)


def _hook(rt, orc, name):
    v = rc.vertices(orc, name)
    for textured in (False, True):
        s, o = _zoo_pair(rt, orc, textured)
        a1, c1, r1, g1 = rt.hooks.reflection(s, v.idx, v.rays, v.colour, v.strike, v.state)
        a2, c2, r2, g2 = o.reflection(v.idx, v.rays, v.colour, v.strike, v.state)
        for what, x, y in (("absorbed", a1, a2), ("colour", c1, c2), ("rng state", g1, g2)):
            bad = np.flatnonzero((x != y).reshape(len(v), -1).any(axis=1))
            assert not len(bad), f"{name}: {what} differs at {len(bad)} vertices, first {bad[:5]}, objects {v.idx[bad[:5]]}, tags {v.tag[bad[:5]]}"
        bad = np.flatnonzero([not _same_f64(p, q) for p, q in zip(r1, r2)]) if not _same_f64(r1, r2) else []
        assert not len(bad), f"{name}: outgoing ray differs at {len(bad)} vertices, first {bad[:5]}, objects {v.idx[bad[:5]]}, tags {v.tag[bad[:5]]}"
    return len(v), int(np.isnan(r2).any(axis=1).sum())  # (the outgoing rays do not depend on the textures: r2 is either zoo's)


@pytest.mark.parametrize("name", FINITE)
def test_hook_equals_the_oracle(rt, orc, name):
    n, nans = _hook(rt, orc, name)
    assert n >= rc.LEAST.get(name, 1500) and nans == 0


@pytest.mark.parametrize("name", rc.NAN_CLASSES)
def test_hook_equals_the_oracle_where_outgoing_rays_are_nan(rt, orc, name):
    n, nans = _hook(rt, orc, name)
    print(f"{name}: {nans} NaN outgoing rays of {n}")
    assert n >= 1500 and nans >= (50 if name == "tir" else 1)


@functools.lru_cache(maxsize=None)
def _route_vertices(orc, nan):
    return rc.concat([rc.vertices(orc, name) for name in (rc.NAN_CLASSES if nan else FINITE)])


def _options(rt):
    A = rt._abi
    return [None, A.rt_render_options(park_lanes=0), A.rt_render_options(park_lanes=-1), A.rt_render_options(park_lanes=8),
            A.rt_render_options(block_threads=256), A.rt_render_options(block_threads=1024)]


def _assert_route(rt, label, opt):
    """The launch was the variant its label names, read from the launch plan the library executed: TEX or non-TEX kernel, scene
    in the LDS or not (as rt_scene_info said, at the default block), counting or timed, the block asked for, and a park pool of
    the capacity asked for (none for park_lanes -1, which is what tells the unparked route from the default one, whatever the
    process default is).  In the counting variant, which keeps stage statistics, the
    routes were also TAKEN: lanes went through stage_slow (the zoo's first vertices include every style that reflection_fast does
    not shade), and lanes were parked exactly where there is a pool -- a wave's first L_SLOW lane always finds room in an empty
    pool of capacity >= 1.  (The statistics count the general pool only; the textured pool feeds stage_tex and is not counted.)"""
    kind, cluster, _, counters, _ = label
    plan = rt.hooks.last_launch_plan()["out"]
    park, block = (0, 0) if opt is None else (opt.park_lanes, opt.block_threads)
    assert (plan["q_tex"], plan["q_count"], plan["two_pass"]) == (int(kind == "tex"), int(counters), 0), (label, plan)
    if not cluster or block != 256:  # (residency is decided at the block that runs: beside a quarter of the waves the cluster may fit)
        assert plan["q_lds"] == int(not cluster), (label, plan)
    assert block == 0 or plan["q_block"] == block, (label, plan)
    assert (plan["F_park"] == 0) if park == -1 else (plan["F_park"] == park if park else plan["F_park"] > 0), (label, plan)
    if counters:
        ss = (ctypes.c_uint64 * 16)()
        assert rt.lib.rt_last_stage_stats(ss) == 0
        slow_stages, slow_lanes, parked = ss[9], ss[10], ss[11]
        assert slow_stages > 0 and slow_lanes >= slow_stages, (label, list(ss))
        assert (parked > 0) == (park != -1) and parked <= slow_lanes, (label, list(ss))


def _routes(rt, orc, kind, cluster, depth, nan):
    torch = pytest.importorskip("torch")
    v = _route_vertices(orc, nan)
    s, o = _witness_pair(rt, orc, kind, cluster)
    assert s.info()["lds_resident"] == (0 if cluster else 1)
    want_c, want_g = _oracle_trace(orc, o, v.rays, depth, v.state)
    if depth == 0:  # one vertex and no more: the path is absorbed there or ends HotPink, and the generator is the hook's afterwards
        a, _, _, g = _zoo_pair(rt, orc, kind == "tex")[1].reflection(v.idx, v.rays, v.colour, v.strike, v.state)
        assert np.array_equal(want_g, g) and (want_c[a == 0] == HOTPINK).all()
    elif depth == 8:
        assert len(np.unique(want_c, axis=0)) > 50  # the witness shows where the rays went
    c, g = s.traceRays(v.rays, depth, rng=v.state)  # the host entry point, process defaults
    assert np.array_equal(c, want_c) and np.array_equal(g, want_g), (kind, cluster, depth, "host entry")
    rays, states = torch.from_numpy(v.rays).cuda(), torch.from_numpy(v.state.view(np.int32)).cuda()
    for counters in (False, True):
        for opt in _options(rt):
            c, g = s.traceRays(rays, depth, rng=states, counters=counters, options=opt)
            c, g = c.cpu().numpy(), g.cpu().numpy().view(np.uint32)
            label = (kind, cluster, depth, counters, None if opt is None else (opt.park_lanes, opt.block_threads))
            _assert_route(rt, label, opt)
            bad = np.flatnonzero((c != want_c).any(axis=1) | (g != want_g).any(axis=1))
            assert not len(bad), f"{label}: {len(bad)} rays differ, first {bad[:5]}, objects {v.idx[bad[:5]]}, tags {v.tag[bad[:5]]}"
    return len(v)


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("kind,cluster", WITNESSES)
def test_routes_equal_the_oracle(rt, orc, kind, cluster, depth):
    assert _routes(rt, orc, kind, cluster, depth, nan=False) >= 9000


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("kind,cluster", WITNESSES)
def test_routes_equal_the_oracle_where_outgoing_rays_are_nan(rt, orc, kind, cluster, depth):
    assert _routes(rt, orc, kind, cluster, depth, nan=True) >= 4500


def _render(rt, orc, kind, names, per_class=400, spp=24, depth=8, seed=11):
    torch = pytest.importorskip("torch")
    A = rt._abi
    v = rc.concat([rc.vertices(orc, name).spread(per_class) for name in names])
    fp = np.zeros((len(v), 12))
    fp[:, :6] = v.rays  # du = dv = 0: every sample of the pixel is the class's ray, with its own generator
    s, o = _witness_pair(rt, orc, kind, False)
    want = fc.compose(orc, o, fp, spp, depth, seed)
    assert (want.accum[:, 0] == spp).sum() >= 50 and want.early.sum() >= 50
    t = torch.from_numpy(fp).cuda()
    for passes in (1, 2):
        for counters in (False, True):
            got = s.renderFootprints(t, spp, depth, seed=seed, counters=counters, options=A.rt_render_options(passes=passes))
            assert rt.hooks.last_launch_plan()["out"]["two_pass"] == passes - 1
            assert np.array_equal(got.accum.cpu().numpy(), want.accum), (kind, names, passes, counters)
            assert np.array_equal(got.rgb.cpu().numpy(), want.rgb), (kind, names, passes, counters)


@pytest.mark.parametrize("kind", ["tex", "planes"])
def test_footprint_renders_equal_the_oracle(rt, orc, kind):
    _render(rt, orc, kind, ("surface_origin", "normal"))


@pytest.mark.parametrize("kind", ["tex", "planes"])
def test_footprint_renders_equal_the_oracle_where_outgoing_rays_are_nan(rt, orc, kind):
    _render(rt, orc, kind, ("tir",))
