"""GPU parity tests proper: the HIP path, called through the C ABI, against the CPU oracle on the same seeded inputs.
Bar: bit-exact (integer sums, bytes, indices, and every double the unit hooks return)."""
import dataclasses
import os

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu


def _same_f64(a, b):
    """Bit-for-bit equality of doubles, NaN (= ValueNone) positions included."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def test_device_present(rt):
    assert rt.device_count() >= 1


# ---- arithmetic the contract relies on -------------------------------------------------------------------------
@pytest.mark.parametrize("op", [0, 1, 2, 3])
def test_ieee_division_sqrt_rint_bit_exact(rt, orc, op):
    rng = np.random.default_rng(100 + op)
    a = np.concatenate([rng.normal(size=200000) * 10.0 ** rng.integers(-30, 30, size=200000), [0.0, -0.0, 1.0, 0.5, 1.5, 2.5, 254.5, 1e-310, np.inf]])
    b = np.concatenate([rng.normal(size=200000) * 10.0 ** rng.integers(-30, 30, size=200000), [1.0, 3.0, 7.0, 255.0, 1e300, 1e-300, 0.1, 3.0, 2.0]])
    if op == 1:
        a = np.abs(a)
    assert _same_f64(rt.hooks.arith(op, a, b), orc.arith(op, a, b))


def test_pow5_is_the_correctly_rounded_power(rt, orc):
    """Math.Pow(x, 5.0) (Sphere.fs:290): the device's double-double x^5 equals the oracle's binary128 x^5 bit for bit on
    the range Glass uses ((1 - cos) in [0, 2]); the C runtime's pow (what .NET calls) is within 1 ulp of both and equal
    on > 99.8 % of inputs (measured 99.92 %: glibc's pow is not always correctly rounded)."""
    rng = np.random.default_rng(9)
    x = np.concatenate([rng.random(1000000) * 2.0, rng.random(100000) * 1e-3, [0.0, 1.0, 2.0, 0.5, 1e-200, 1.0 - 2 ** -53, -1e-17]])
    dev, ref, crt = rt.hooks.arith(4, x), orc.arith(4, x), orc.arith(5, x)
    assert _same_f64(dev, ref)
    assert np.mean(dev == crt) > 0.998
    assert np.all(np.abs(dev - crt) <= np.spacing(np.abs(crt)))


def test_normal_range_sqrt_and_reciprocal(rt):
    """rt_device.h's sqrt_above_tol / inv_sqrt_above_tol (the compiler's own expansions minus their rescaling of denormal and
    huge operands) against the host's correctly rounded sqrt and division: 40 M operands log-uniform over [1e-8, 1e300],
    plus the places rounding is touchiest (perfect squares and their neighbours, values just above the 1e-8 tolerance,
    powers of two) and the special values (+inf, NaN)."""
    rng = np.random.default_rng(21)
    special = np.array([1e-8, 1.0000000000000002e-8, 1.0, 2.0, 4.0, 0.25, 2.0 ** -26, 2.0 ** 600, 1e300, np.inf, np.nan, 3.0, 0.1])
    ints = rng.integers(1, 2 ** 26, 200000).astype(np.float64)
    squares = ints * ints
    near = np.concatenate([squares, np.nextafter(squares, np.inf), np.nextafter(squares, 0.0)])
    for chunk in range(8):
        x = np.exp(rng.uniform(np.log(1e-8), np.log(1e300), 5000000))
        if chunk == 0:
            x = np.concatenate([x, special, near, 2.0 ** rng.integers(-26, 1000, 4000).astype(np.float64), 1.0 + rng.random(1000000)])
        with np.errstate(invalid="ignore", divide="ignore"):
            want_sqrt = np.sqrt(x)
            want_inv = 1.0 / want_sqrt
        assert _same_f64(rt.hooks.arith(5, x), want_sqrt)
        assert _same_f64(rt.hooks.arith(6, x), want_inv)


# ---- unit hooks --------------------------------------------------------------------------------------------------
def test_float_producer_and_stream_state(rt, orc):
    assert _same_f64(rt.hooks.float_producer((1, 2, 3, 4), 1000), orc.float_producer((1, 2, 3, 4), 1000))
    rng = np.random.default_rng(3)
    px = rng.integers(0, 2 ** 40, size=5000, dtype=np.uint64)
    sm = rng.integers(0, 5000, size=5000, dtype=np.uint32)
    for seed in (0, 1, 2 ** 63 + 12345):
        assert np.array_equal(rt.hooks.stream_state(seed, px, sm), orc.stream_state(seed, px, sm))


def test_pixel_ops_exhaustive(rt, orc):
    a = np.repeat(np.arange(256, dtype=np.uint8), 256)
    b = np.tile(np.arange(256, dtype=np.uint8), 256)
    A3, B3 = np.stack([a, b, a], 1), np.stack([b, a, b], 1)
    assert np.array_equal(rt.hooks.pixel_combine(A3, B3), orc.pixel_combine(A3, B3))
    alb = np.linspace(0.0, 1.0, len(a))
    assert np.array_equal(rt.hooks.pixel_darken(A3, alb), orc.pixel_darken(A3, alb))
    half = np.full(len(a), 0.5)
    assert np.array_equal(rt.hooks.pixel_darken(A3, half), orc.pixel_darken(A3, half))  # x.5 ties: half-to-even


def test_bbox_hits_incl_axis_aligned_rays(rt, orc):
    rays = scenes.random_rays(100000, 11)
    rng = np.random.default_rng(12)
    lo = rng.normal(size=(100000, 3)) * 2
    boxes = np.concatenate([lo, lo + np.abs(rng.normal(size=(100000, 3)))], axis=1)
    # axis-aligned directions give +-inf inverse directions and NaN products (BoundingBox.fs:25-28)
    rays[:3000, 3:] = np.eye(3)[rng.integers(0, 3, 3000)] * rng.choice([-1.0, 1.0], size=(3000, 1))
    rays[:1000, :3] = boxes[:1000, :3]  # origins exactly on a box corner
    boxes[50000:51000, :3], boxes[50000:51000, 3:] = boxes[50000:51000, 3:].copy(), boxes[50000:51000, :3].copy()  # inverted boxes
    assert np.array_equal(rt.hooks.bbox_hits(rays, boxes), orc.bbox_hits(rays, boxes))


def test_single_precision_filter_never_loses_a_hit(rt):
    """The timed node loop's filter (csrc/rt_device.h) against the exact BoundingBox.hits, both on the device: exact hit => filter hit,
    for the loop's own instruction forms (bit 1) and the compiled form (bit 2), on the cases of tests/filter_cases.py -- rays through
    faces / edges / corners, origins on faces and corners, axis-aligned / denormal / non-unit directions, inverted and flat boxes,
    coordinates from 1e-3 to 1e6, origins 1e13 away, NaN and infinite rays and boxes -- and with the margin's scale enlarged as a
    whole tree's would be.  (The CPU model of the same filter is held to the ORACLE's exact test in tests/test_filter_conservative.py.)"""
    import filter_cases as fc
    n = 200_000
    hits = 0
    for name, rays, boxes in fc.classes(n, seed=31337):
        for bmax in (0.0, 2000.0):
            out = rt.hooks.bbox_filter(rays, boxes, bmax=bmax)
            exact, loop, compiled = (out & 1) != 0, (out & 2) != 0, (out & 4) != 0
            lost = exact & ~(loop & compiled)
            assert not lost.any(), f"{name} (bmax {bmax}): the filter lost {int(lost.sum())} of {int(exact.sum())} hits, first at {int(np.flatnonzero(lost)[0])}"
            if np.isfinite(rays).all() and np.isfinite(boxes).all():
                assert np.array_equal(loop, compiled), name  # the two forms differ only in how NaN operands fall through min/max
        hits += int(exact.sum())
        if name.startswith(("random_scale2_", "random_scale10_")):  # it IS a filter: ordinary boxes the exact test rejects, it rejects
            assert int((loop & ~exact).sum()) <= n // 2000, name
    assert hits > 4_000_000


def test_sphere_and_plane_intersection(rt, orc):
    rays = scenes.random_rays(200000, 21)
    rng = np.random.default_rng(22)
    sph = np.concatenate([rng.normal(size=(200000, 3)) * 3, rng.normal(size=(200000, 1)) * 2], axis=1)
    sph[:2000, 3] = np.linalg.norm(sph[:2000, :3] - rays[:2000, :3], axis=1)  # origin on the surface: roots near 0 and the 1e-8 band
    assert _same_f64(rt.hooks.sphere_first_intersection(rays, sph), orc.sphere_first_intersection(rays, sph))
    n = rng.normal(size=(200000, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    pl = np.concatenate([rng.normal(size=(200000, 3)) * 3, n], axis=1)
    assert _same_f64(rt.hooks.plane_intersection(rays, pl), orc.plane_intersection(rays, pl))


def test_sphere_roots_across_magnitudes(rt, orc):
    """The device picks Sphere.firstIntersection's root without the reference's `Float.compare i1 i2` (rt_device.h explains why
    that is the same double); the oracle keeps the literal control flow.  4 M cases built to sit where the argument is
    delicate: origins 1e3..1e13 away (the sqrt is absorbed into b, roots differ by 0 or 1 ulp), tangent rays (discriminant in and
    around the 1e-8 band), origins on, just inside and just outside the surface, tiny and huge radii, rays pointing away."""
    rng = np.random.default_rng(314)
    n = 4_000_000
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    c = rng.normal(size=(n, 3)) * 3.0
    r = np.exp(rng.uniform(np.log(1e-3), np.log(1e4), n)) * rng.choice([-1.0, 1.0], n, p=[0.1, 0.9])
    dist = np.exp(rng.uniform(np.log(1e-3), np.log(1e13), n))
    # aim point: centre + offset perpendicular-ish with |offset| around |r| (inside, tangent, outside)
    off = rng.normal(size=(n, 3))
    off -= np.sum(off * d, axis=1, keepdims=True) * d
    off /= np.linalg.norm(off, axis=1, keepdims=True)
    frac = rng.choice([0.0, 0.5, 0.999999, 1.0, 1.000001, 1.5], n)
    frac = np.where(rng.random(n) < 0.3, 1.0 + rng.normal(size=n) * 1e-9, frac)
    aim = c + off * (np.abs(r) * frac)[:, None]
    o = aim - d * dist[:, None] * rng.choice([1.0, -1.0], n, p=[0.8, 0.2])[:, None]
    k = n // 10
    o[:k] = c[:k] + d[:k] * np.abs(r[:k])[:, None] * (1.0 + rng.choice([0.0, 1e-9, -1e-9, 1e-7, -1e-7], k))[:, None]  # on / near the surface
    rays = np.concatenate([o, d], axis=1)
    sph = np.concatenate([c, r[:, None]], axis=1)
    got, want = rt.hooks.sphere_first_intersection(rays, sph), orc.sphere_first_intersection(rays, sph)
    assert _same_f64(got, want)
    assert 0.2 < np.isfinite(want).mean() < 0.9


def _with_tree(rt, kind, fn):
    before = rt.get_walk_tree()
    rt.set_walk_tree(kind)
    try:
        return fn()
    finally:
        rt.set_walk_tree(before)


def _scene_pair(rt, orc, objs):
    return rt.Scene.make(objs), orc.OracleScene(objs)


def test_hit_object_indices_strikes_and_counters(rt, orc):
    for objs, *_ in (scenes.all_materials(), scenes.small_final()):
        s, o = _scene_pair(rt, orc, objs)
        rays = scenes.random_rays(60000, 31, origin_scale=4.0)
        rays[:20000, :3] = [13.0, 2.0, -3.0]
        h1, s1, c1 = rt.hooks.hit_object(s, rays)
        h2, s2, c2 = o.hit_object(rays)
        assert np.array_equal(h1, h2)
        assert _same_f64(s1, s2)
        assert np.array_equal(c1[:, 1], c2[:, 1])  # Hittable.hits calls per ray: the same leaves whatever tree is walked
        if rt.get_walk_tree() == "reference":
            assert np.array_equal(c1[:, 0], c2[:, 0])  # BoundingBox.hits calls per ray
        else:
            assert c1[:, 0].sum() < c2[:, 0].sum() or len(objs) < 40


def test_hit_object_through_the_hand_written_node_loop(rt, orc):
    """The timed kernel variant walks the tree with node_loop_lds (assembly) on the LDS image; the hooks above run the compiled
    C++ on the global image.  Same rays through both and through the oracle -- including what renders almost never produce:
    axis-aligned directions (infinite inverse directions, NaN products), origins exactly on box planes and corners, rays along
    box edges, and origins far outside the scene."""
    rng = np.random.default_rng(2718)
    for objs in (scenes.small_final()[0], scenes.all_materials()[0], scenes.many_spheres(n=300, seed=5)[0]):
        s, o = _scene_pair(rt, orc, objs)
        assert s.info()["lds_resident"] == 1
        skip, prim, boxes = s.walk_tree()
        n = 120000
        rays = scenes.random_rays(n, 99, origin_scale=5.0)
        k = 20000
        rays[:k, 3:] = np.eye(3)[rng.integers(0, 3, k)] * rng.choice([-1.0, 1.0], size=(k, 1))       # axis-aligned
        two = np.eye(3)[rng.integers(0, 3, k)] + np.eye(3)[rng.integers(0, 3, k)] * rng.choice([-1.0, 1.0], size=(k, 1))
        ok = np.linalg.norm(two, axis=1) > 0.5
        two[~ok] = [1.0, 1.0, 0.0]
        rays[k:2 * k, 3:] = two / np.linalg.norm(two, axis=1, keepdims=True)                              # in a coordinate plane: one infinite inverse
        if len(boxes):
            b = boxes[rng.integers(0, len(boxes), 3 * k)]                                               # (minx,maxx,miny,maxy,minz,maxz)
            corner = np.stack([b[:, 0 + rng.integers(0, 2)], b[:, 2 + rng.integers(0, 2)], b[:, 4 + rng.integers(0, 2)]], axis=1)
            rays[:k, :3] = corner[:k]                                                                   # axis-aligned ray from a box corner
            rays[2 * k:3 * k, :3] = corner[k:2 * k]                                                     # any direction from a box corner
            rays[3 * k:4 * k, 1] = b[2 * k:, 2]                                                         # origin on a box's y-min plane (the floor of the small spheres)
        rays[4 * k:5 * k, :3] *= 1e6                                                                    # far away
        h1, s1 = rt.hooks.hit_object_lds(s, rays)
        h0, s0, _ = rt.hooks.hit_object(s, rays)
        h2, s2, _ = o.hit_object(rays)
        assert np.array_equal(h1, h2) and _same_f64(s1, s2)
        assert np.array_equal(h0, h2) and _same_f64(s0, s2)
        assert 0.05 < np.mean(h2 >= 0) <= 1.0


def test_leaf_box_is_implied_by_the_sphere_hit(rt, orc):
    """The timed variant's leaf pass does not evaluate a Leaf's own BoundingBox.hits (Scene.fs:41) when Sphere.firstIntersection has
    found a hit from its Greater branch in a scene of moderate extent -- the claim proved above leaf_test_object_exact in
    csrc/rt_device.h.  Rays aimed where the claim is thinnest: tangent to a sphere AT one of the six points where it touches its box
    (offsets from 1 ulp to 1e-7 either way, so the discriminant crosses the 1e-8 band and the ray crosses the box face), origins
    inside a sphere a few ulps to 1e-6 under a pole and leaving at shallow angles, origins ON the surface (what every bounce
    produces), at the poles too.  Three scenes: one inside the claim's bounds with small spheres spread over +-300, the final scene's
    own scale, and one outside the bounds (radii 20 to 60), where the box test is evaluated for every candidate.  The device's two
    routes and the oracle must name the same object and the same strike point for every ray."""
    P, S, H, Px, Tex = scenes.P, scenes.S, scenes.H, scenes.Px, scenes.Tex
    rng = np.random.default_rng(4242)

    def scene_of(n, spread, rlo, rhi):
        objs, placed = [], []
        while len(objs) < n:
            c = rng.uniform(-spread, spread, 3)
            r = float(np.exp(rng.uniform(np.log(rlo), np.log(rhi))))
            if all(np.linalg.norm(c - c2) > r + r2 + 0.01 for c2, r2 in placed):
                placed.append((c, r))
                style = [S.LambertReflection(0.5, Tex(Px(200, 100, 50))), S.Glass(1.0, Tex(Px(255, 255, 255)), 1.5), S.PureReflection(0.9, Tex(Px(180, 180, 180)))][len(objs) % 3]
                objs.append(H.Sphere(rt.Sphere.make(style, P(*c), r)))
        objs.append(H.UnboundedSphere(rt.Sphere.make(S.LightSource(Tex(Px(255, 255, 255))), P(0.0, 0.0, 0.0), 5000.0)))
        return objs, placed

    for n_sph, spread, rlo, rhi, expect in ((60, 300.0, 0.05, 1.0, 1), (60, 11.0, 0.2, 1.0, 1), (12, 150.0, 20.0, 60.0, 0)):
        objs, placed = scene_of(n_sph, spread, rlo, rhi)
        s, o = _scene_pair(rt, orc, objs)
        info = s.info()
        assert info["lds_resident"] == 1 and info["leaf_box_implied"] == expect
        n = 240_000
        which = rng.integers(0, len(placed), n)
        c = np.array([placed[i][0] for i in which])
        r = np.array([placed[i][1] for i in which])
        axis = rng.integers(0, 3, n)
        sign = rng.choice([-1.0, 1.0], n)
        e = np.eye(3)[axis] * sign[:, None]                       # the pole's outward normal
        pole = c + e * r[:, None]
        tang = rng.normal(size=(n, 3))
        tang -= np.sum(tang * e, axis=1, keepdims=True) * e       # a direction in the box face's plane
        tang /= np.linalg.norm(tang, axis=1, keepdims=True)
        mag = np.exp(rng.uniform(np.log(1e-16), np.log(1e-6), n)) * rng.choice([-1.0, 1.0, 0.0], n, p=[0.45, 0.45, 0.1])
        rays = np.zeros((n, 6))
        k = n // 4
        # (1) tangent at a pole, shifted along the normal by +-mag * r, started 0.1..30 away
        aim = pole + e * (mag * r)[:, None]
        dist = rng.uniform(0.1, 30.0, n)
        rays[:, :3] = aim - tang * dist[:, None]
        rays[:, 3:] = tang
        # (2) origin inside, just under a pole, leaving at a shallow angle through (or beside) the pole region
        sl = slice(k, 2 * k)
        depth = np.exp(rng.uniform(np.log(1e-16), np.log(1e-6), n))
        tilt = np.exp(rng.uniform(np.log(1e-9), np.log(1e-2), n)) * rng.choice([-1.0, 1.0], n)
        d2 = tang + e * tilt[:, None]
        d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
        rays[sl, :3] = (pole - e * (depth * r)[:, None])[sl]
        rays[sl, 3:] = d2[sl]
        # (3) origin ON the surface at a random point (and at a pole for a third of them), any direction: self-hits at t ~ 0 and
        #     true second hits through the sphere
        sl = slice(2 * k, 3 * k)
        q = rng.normal(size=(n, 3)); q /= np.linalg.norm(q, axis=1, keepdims=True)
        q = np.where((rng.random(n) < 0.33)[:, None], e, q)
        rays[sl, :3] = (c + q * r[:, None])[sl]
        dd = rng.normal(size=(n, 3)); dd /= np.linalg.norm(dd, axis=1, keepdims=True)
        rays[sl, 3:] = dd[sl]
        # (4) tangent anywhere on the silhouette (not only at poles), offsets across the 1e-8 band
        sl = slice(3 * k, n)
        t2 = np.cross(q, dd); t2 /= np.linalg.norm(t2, axis=1, keepdims=True)
        rays[sl, :3] = (c + q * (r * (1.0 + mag))[:, None] - t2 * dist[:, None])[sl]
        rays[sl, 3:] = t2[sl]
        rays[:, 3:] /= np.linalg.norm(rays[:, 3:], axis=1, keepdims=True)
        h1, s1 = rt.hooks.hit_object_lds(s, rays)
        h0, s0, _ = rt.hooks.hit_object(s, rays)
        h2, s2, _ = o.hit_object(rays)
        assert np.array_equal(h0, h2) and _same_f64(s0, s2)
        assert np.array_equal(h1, h2) and _same_f64(s1, s2)
        bounded = (h2 >= 0) & (h2 < n_sph)
        assert 0.2 < np.mean(bounded) < 0.98  # the rays do hit, and do miss, the spheres they graze


def test_pixel_candidates_contain_every_leaf_a_camera_ray_can_hit(rt):
    """The timed kernel walks the tree once per PIXEL for all of its camera rays (pixel_candidates, csrc/rt_device.h): the Leaves the
    pyramid of the pixel's rays can touch.  The set must contain every Leaf whose box any camera ray of the pixel hits under the exact
    BoundingBox.hits -- here checked with rays through the four corners of the pixel's patch of the viewport (jitter 0 and 1, both
    attainable: FloatProducer is inclusive at both ends), its edges, and random points, built with Scene.traceOnce's own arithmetic
    (Scene.fs:129-144), against every Leaf box of the scene with the DEVICE's exact box test.  Cameras: the final scene's own, one
    inside the sphere field looking along the rows (many boxes in reach, the fall-back to walking must show), one looking straight
    down an axis, and the every-material scene's."""
    rng = np.random.default_rng(777)
    cases = []
    objs, cam, w, h = scenes.small_final(pixels=60)
    cases.append((objs, cam, w, h))
    P, V = scenes.P, scenes.V
    low = dataclasses.replace(rt.Camera.makeBasic(10, 1.0, 1.5, P(-10.5, 0.3, 0.45), scenes.unit(1.0, -0.01, 0.0), V(0.0, 1.0, 0.0)), BounceDepth=5)
    cases.append((objs, low, 45, 30))
    axis = dataclasses.replace(rt.Camera.makeBasic(10, 2.0, 1.0, P(0.5, 30.0, 0.5), scenes.unit(0.0, -1.0, 0.0), V(0.0, 0.0, 1.0)), BounceDepth=5)
    cases.append((objs, axis, 40, 40))
    objs2, cam2, w2, h2 = scenes.all_materials(pixels=40)
    cases.append((objs2, cam2, w2, h2))
    walked = total = nonempty = 0
    for objs, cam, w, h in cases:
        s = rt.Scene.make(objs)
        if s.info()["lds_resident"] != 1:
            continue
        _, prim, boxes = s.walk_tree()
        leaf = prim >= 0
        lb = boxes[leaf][:, [0, 2, 4, 1, 3, 5]]  # (minx,maxx,miny,maxy,minz,maxz) -> (min xyz, max xyz)
        lp = prim[leaf]
        npx = 1500
        rows = rng.integers(-h - 1, h, npx)       # row = maxH - r - 1 for r in [0, 2 maxH]
        cols = rng.integers(-w, w + 1, npx)
        cand = rt.hooks.pixel_candidates(s, cam, w, h, np.stack([rows, cols], axis=1))
        a = cam.to_abi()
        eye, xo, xd, yd = (np.array(list(v)) for v in (a.view_origin, a.xaxis_origin, a.xaxis_dir, a.yaxis_dir))
        jit = np.concatenate([np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0], [0.5, 0.0], [1.0, 0.5], [0.5, 1.0], [0.0, 0.5]]), rng.random((8, 2))])
        for i in range(npx):
            total += 1
            if cand[i, 0] == -2:
                walked += 1
                continue
            lx = ((cols[i] + jit[:, 0]) * a.viewport_width) / float(w)        # Scene.fs:131-133
            ly = ((rows[i] + jit[:, 1]) * a.viewport_height) / float(h)       # Scene.fs:135-137
            end = (xo[None, :] + xd[None, :] * lx[:, None]) + yd[None, :] * ly[:, None]
            d = end - eye[None, :]
            d = d * (1.0 / np.sqrt(np.sum(d * d, axis=1)))[:, None]
            rays = np.concatenate([np.tile(eye, (len(jit), 1)), d], axis=1)
            hit = rt.hooks.bbox_hits(np.repeat(rays, len(lb), axis=0), np.tile(lb, (len(rays), 1))).reshape(len(rays), len(lb)).any(axis=0)
            reach = set(int(x) for x in lp[hit])
            have = set(int(x) for x in cand[i] if x >= 0)
            assert reach <= have, (i, rows[i], cols[i], sorted(reach), sorted(have))
            nonempty += bool(have)
    assert total > 4000 and nonempty > 300 and 0 < walked < total // 2


def test_leaf_queue_of_the_node_loop_under_pressure(rt, orc):
    """The timed variant's node loop queues hit Leaves (two 16-bit entries per lane) and stops a lane only when its queue is full.
    Rays that run through dozens of overlapping Leaf boxes -- a skewer of nested and overlapping spheres, exact duplicates among them
    (the tie rule decides between equal t^2) -- fill the queues over and over; rays from inside, from far away, and ones that miss."""
    P, S, H, Px, Tex = scenes.P, scenes.S, scenes.H, scenes.Px, scenes.Tex
    rng = np.random.default_rng(31)
    objs = []
    for i in range(70):  # along the z axis: nested shells and overlapping neighbours
        c = P(0.02 * float(rng.normal()), 0.02 * float(rng.normal()), 0.25 * i)
        r = float(rng.uniform(0.2, 3.0)) * (-1.0 if i % 11 == 0 else 1.0)
        objs.append(H.Sphere(rt.Sphere.make(S.LambertReflection(0.5, Tex(Px(9, 9, 9))), c, r)))
        if i % 6 == 0:
            objs.append(H.Sphere(rt.Sphere.make(S.PureReflection(0.5, Tex(Px(1, 2, 3))), c, r)))  # the same sphere twice
    for i in range(60):  # and a cloud around it
        objs.append(H.Sphere(rt.Sphere.make(S.Glass(0.9, Tex(Px(7, 7, 7)), 1.5), P(float(rng.uniform(-6, 6)), float(rng.uniform(-6, 6)), float(rng.uniform(0, 18))), float(rng.uniform(0.1, 1.0)))))
    objs.append(H.UnboundedSphere(rt.Sphere.make(S.LightSource(Tex(Px(200, 200, 255))), P(0.0, 0.0, 0.0), 500.0)))
    n = 60000
    rays = scenes.random_rays(n, 5, origin_scale=4.0)
    k = n // 4
    rays[:k, :3] = np.stack([0.05 * rng.normal(size=k), 0.05 * rng.normal(size=k), rng.uniform(-30, -3, k)], 1)  # down the skewer
    d = np.stack([0.01 * rng.normal(size=k), 0.01 * rng.normal(size=k), np.ones(k)], 1)
    rays[:k, 3:] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[k:2 * k, :3] = np.stack([0.3 * rng.normal(size=k), 0.3 * rng.normal(size=k), rng.uniform(0, 17, k)], 1)  # from inside the shells
    for tree in ("sah", "reference"):
        s, o = rt.Scene.make(objs, walk_tree=tree), orc.OracleScene(objs)
        assert s.info()["lds_resident"] == 1
        if tree == "sah":
            s.tune_rays(rays[::7])  # a thinned tree: more Leaves per Branch, longer runs of consecutive Leaf hits
        h1, s1 = rt.hooks.hit_object_lds(s, rays)
        h0, s0, c0 = rt.hooks.hit_object(s, rays)
        h2, s2, c2 = o.hit_object(rays)
        assert np.array_equal(h1, h2) and _same_f64(s1, s2)
        assert np.array_equal(h0, h2) and _same_f64(s0, s2) and np.array_equal(c0[:, 1], c2[:, 1])
        assert c2[:k, 1].mean() > 25  # the skewer rays really do meet dozens of Leaf boxes each
    # and whole renders of the same scene (queue + lane scheduler + shading), counting variant against timed variant against oracle
    cam = dataclasses.replace(rt.Camera.makeBasic(40, 1.0, 1.0, P(0.0, 0.0, -8.0), scenes.unit(0.0, 0.0, 1.0), scenes.V(0.0, 1.0, 0.0)), BounceDepth=12)
    _assert_render_equal(*_render_both(rt, orc, objs, cam, 12, 12, seed=3))


def test_reflection_every_style(rt, orc):
    """Ordinary materials, random rays against unrelated strike points, random generator states.  The edges -- near-normal and grazing
    incidence, total internal reflection at its threshold (NaN rays included), origins on the surface, the LightSourceCap band, extreme
    material parameters, chosen generator values, the retry loops, and the timed kernel's own routes to the same arithmetic -- are in
    tests/test_gpu_reflection.py (cases: tests/reflection_cases.py)."""
    objs, *_ = scenes.all_materials()
    s, o = _scene_pair(rt, orc, objs)
    rng = np.random.default_rng(41)
    n_per = 4000
    for idx, h in enumerate(objs):
        rays = scenes.random_rays(n_per, 50 + idx, origin_scale=2.0)
        if h.sphere is not None:
            c, r = np.array(h.sphere.Centre), abs(h.sphere.Radius)
            d = rng.normal(size=(n_per, 3))
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            strike = c + r * d
            rays[: n_per // 2, :3] = c + 0.3 * r * rng.normal(size=(n_per // 2, 3)) / 2  # half the rays start inside
            rays[-50:, 3:] = -d[-50:]  # along the normal: degenerate plane (Sphere.fs:72-75, 121-124)
            rays[-50:, :3] = strike[-50:] + d[-50:]
        else:
            p0, nn = np.array(h.plane.Point), np.array(h.plane.Normal)
            t = rng.normal(size=(n_per, 3))
            strike = p0 + t - np.outer(t @ nn, nn)
            rays[-50:, 3:] = -nn
        col = rng.integers(0, 256, size=(n_per, 3), dtype=np.uint8)
        st = rng.integers(1, 2 ** 31 - 1, size=(n_per, 4), dtype=np.uint32)
        a1, c1, r1, g1 = rt.hooks.reflection(s, np.full(n_per, idx), rays, col, strike, st)
        a2, c2, r2, g2 = o.reflection(np.full(n_per, idx), rays, col, strike, st)
        assert np.array_equal(a1, a2), f"absorbed differs for hittable {idx}"
        assert np.array_equal(c1, c2), f"colour differs for hittable {idx}"
        assert _same_f64(r1, r2), f"outgoing ray differs for hittable {idx}"
        assert np.array_equal(g1, g2), f"rng state differs for hittable {idx}"


def test_device_trig_is_the_correctly_rounded_value(rt, orc):
    """Math.Acos / Math.Sin / Math.Atan2 of the texture maps: the device's double-double route (csrc/rt_trig.h, OCML seed + one
    Newton step) against the oracle's binary128 route, bit for bit, on 3 x 400k operands incl. the ends of acos' domain, arguments
    next to multiples of pi/2, tiny and huge ratios and every special case.  (tests/test_trig_cr.py pins both to mpmath on the CPU.)"""
    rng = np.random.default_rng(77)
    n = 400000
    x = np.concatenate([rng.uniform(-1, 1, n), 1 - 10.0 ** rng.uniform(-16, -1, 20000), -1 + 10.0 ** rng.uniform(-16, -1, 20000),
                        [0.0, -0.0, 1.0, -1.0, 1.0000000000000002, -2.0, np.nan, np.inf, 1 - 2.0 ** -53, -1 + 2.0 ** -53]])
    assert _same_f64(rt.hooks.arith(7, x), orc.arith(7, x))
    a = np.concatenate([rng.uniform(-100, 100, n), rng.uniform(-1e5, 1e5, 50000), np.arange(1, 20000) * (np.pi / 2),
                        rng.choice([-1.0, 1.0], 5000) * 10.0 ** rng.uniform(-300, 0, 5000), [0.0, -0.0, np.nan, np.inf, -np.inf, 5e-324, 1048575.5]])
    got, want = rt.hooks.arith(8, a), orc.arith(8, a)
    assert _same_f64(got, want)  # bit patterns, so the signs of zeros too (the sign of a NaN is not compared)
    y = np.concatenate([rng.normal(size=n), rng.normal(size=30000) * 10.0 ** rng.uniform(-200, 200, 30000),
                        [0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.inf, -np.inf, 1.0, -1.0, np.nan, 1.0]])
    xx = np.concatenate([rng.normal(size=n), rng.normal(size=30000) * 10.0 ** rng.uniform(-200, 200, 30000),
                         [1.0, 1.0, -1.0, -1.0, 0.0, -0.0, 0.0, -0.0, np.inf, np.inf, -np.inf, -np.inf, np.inf, -np.inf, 1.0, np.nan]])
    assert _same_f64(rt.hooks.arith(9, y, xx), orc.arith(9, y, xx))


def test_texture_lookup(rt, orc):
    objs, *_ = scenes.all_materials()
    s, o = _scene_pair(rt, orc, objs)
    rng = np.random.default_rng(61)
    for tex, centre, radius in ((2, (1.1, 0.0, 1.0), 0.5), (3, (1.6, 1.2, 2.0), 0.3)):
        d = rng.normal(size=(100000, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        d[:6] = np.concatenate([np.eye(3), -np.eye(3)])  # the poles and the seam of the map (TestSphere.fs:197-204's points)
        pts = np.array(centre) + radius * d
        uv1, c1 = rt.hooks.texture_colour_at(s, tex, pts)
        uv2, c2 = o.texture_colour_at(tex, pts)
        # Math.Acos / Math.Atan2 / Math.Sin are the correctly rounded values on both sides (csrc/rt_trig.h: double-double here,
        # binary128 in the oracle), so (u, v) -- and every truncated texel or ramp index -- is the same bit for bit
        assert _same_f64(uv1, uv2)
        assert np.array_equal(c1, c2)


def test_trace_ray_paths(rt, orc):
    for (objs, cam, w, h), depth in ((scenes.all_materials(), 12), (scenes.small_final(), 50), (scenes.small_final(), 0)):
        s, o = _scene_pair(rt, orc, objs)
        rays = scenes.random_rays(30000, 71, origin_scale=0.5)
        rays[:, :3] += [0.0, 0.5, -1.0]
        st = np.random.default_rng(72).integers(1, 2 ** 31 - 1, size=(30000, 4), dtype=np.uint32)
        c1, g1 = rt.hooks.trace_ray(s, depth, rays, st)
        c2, g2 = o.trace_ray(depth, rays, st)
        assert np.array_equal(c1, c2)
        assert np.array_equal(g1, g2)


# ---- whole renders ------------------------------------------------------------------------------------------------
def _render_both(rt, orc, objs, cam, w, h, seed, **shard):
    """The HIP render (the counting kernel variant, and -- asserted equal to it -- the plain variant the bench times, whose
    node loop is hand-written assembly) and the oracle's."""
    s, o = _scene_pair(rt, orc, objs)
    res = s.render_rows(w, h, cam, seed=seed, counters=True, **shard)
    plain = s.render_rows(w, h, cam, seed=seed, counters=False, **shard)
    assert np.array_equal(plain.accum, res.accum) and np.array_equal(plain.rgb, res.rgb), "kernel variants disagree"
    assert plain.stats["samples"] == res.stats["samples"] and plain.stats["pixels_early"] == res.stats["pixels_early"]
    acc, rgb, st = o.render_rows(w, h, cam.to_abi(), seed=seed, threads=8, **shard)
    return res, acc, rgb, st


def _assert_render_equal(res, acc, rgb, st):
    assert np.array_equal(res.accum, acc), f"{np.count_nonzero(np.any(res.accum != acc, axis=-1))} pixels differ"
    assert np.array_equal(res.rgb, rgb)
    for k in ("rays", "prim_tests", "reflections", "samples", "pixels", "pixels_early"):
        assert res.stats[k] == st[k], k
    if scenes.rt.get_walk_tree() == "reference":  # the default walks a surface-area tree over the same leaves: fewer box tests
        assert res.stats["aabb_tests"] == st["aabb_tests"]


def test_config1_empty_scene_is_black_with_one_sample(rt, orc):
    objs, cam, w, h = rt.sample_images.config1_empty()
    res, acc, rgb, st = _render_both(rt, orc, objs, cam, w, h, seed=1)
    _assert_render_equal(res, acc, rgb, st)
    assert res.accum.shape == (101, 201, 4)
    assert np.all(res.accum[..., 0] == 1) and np.all(res.accum[..., 1:] == 0)


@pytest.mark.parametrize("seed", [0, 12345])
def test_all_materials_render(rt, orc, seed):
    objs, cam, w, h = scenes.all_materials()
    _assert_render_equal(*_render_both(rt, orc, objs, cam, w, h, seed=seed))


@pytest.mark.parametrize("spp", [1, 2, 3, 9, 10, 11, 12, 40])
def test_adaptive_sampling_counts(rt, orc, spp):
    """Scene.renderPixel (Scene.fs:172-194): firstTrial = min 5 (spp/2); spp=2 takes 3 samples; counts are 2k+1 or spp."""
    objs, cam, w, h = scenes.all_materials(spp=spp, pixels=8)
    res, acc, rgb, st = _render_both(rt, orc, objs, cam, w, h, seed=5)
    _assert_render_equal(res, acc, rgb, st)
    k = min(5, spp // 2)
    assert set(np.unique(res.accum[..., 0])) <= {2 * k + 1, max(2 * k + 1, spp)}


def test_config2_three_lambert_reduced(rt, orc):
    objs, cam, w, h = rt.sample_images.config2_three_lambert(spp=30, pixels=27)
    _assert_render_equal(*_render_both(rt, orc, objs, cam, w, h, seed=2))


def test_config2_full_size_equals_the_oracle(rt, orc):
    """BASELINE config 2 whole (801x451 px, 100 spp, 50 bounces): every PixelStats and every counter."""
    objs, cam, w, h = rt.sample_images.config2_three_lambert()
    _assert_render_equal(*_render_both(rt, orc, objs, cam, w, h, seed=2024))


def test_config3_final_scene_rows(rt, orc):
    """BASELINE config 3 at FULL geometry (2401x1601, 500 spp, depth 50): three image rows through sky, horizon, spheres."""
    objs, cam, w, h = rt.sample_images.config3_final()
    for row in (100, 640, 1000):
        _assert_render_equal(*_render_both(rt, orc, objs, cam, w, h, seed=2024, row_first=row, row_stride=1, n_rows=1))


def test_hot_pink_when_bounce_limit_is_hit(rt, orc):
    """Scene.fs:98,114: a path still alive after depth+1 hits returns HotPink; two facing mirrors make every path do so."""
    P, H, PS = rt.Point.make, rt.Hittable, rt.InfinitePlaneStyle
    up = rt.Vector.unitise(rt.Vector.make(0.0, 0.0, 1.0))
    objs = [H.InfinitePlane(rt.InfinitePlane.make(PS.PureReflection(1.0, rt.Colour.White), P(0.0, 0.0, 5.0), up)),
            H.InfinitePlane(rt.InfinitePlane.make(PS.PureReflection(1.0, rt.Colour.White), P(0.0, 0.0, -5.0), up))]
    cam = dataclasses.replace(rt.Camera.makeBasic(3, 1.0, 1.0, P(0.0, 0.0, 0.0), up, rt.Vector.make(0.0, 1.0, 0.0)), BounceDepth=7)
    res, acc, rgb, st = _render_both(rt, orc, objs, cam, 4, 4, seed=3)
    _assert_render_equal(res, acc, rgb, st)
    assert np.all(res.rgb == np.array(rt.Colour.HotPink, np.uint8))
    assert res.stats["rays"] == res.stats["samples"] * 8


@pytest.mark.parametrize("name", ["spheres", "shiny-floor", "fuzzy-floor", "inside-sphere", "total-refraction", "glass", "moved-camera", "textured-sphere"])
def test_reference_catalogue_thumbnails(rt, orc, name):
    """The reference's own SampleImages scenes (SampleImages.fs:59-810; inside-sphere: :263-411) at thumbnail size, 20 spp."""
    objs, cam, w, h = rt.sample_images.get(name)()
    cam = dataclasses.replace(cam, SamplesPerPixel=20)
    w, h = max(1, w // 20), max(1, h // 20)
    _assert_render_equal(*_render_both(rt, orc, objs, cam, w, h, seed=8))


def test_sharding_does_not_change_pixels(rt):
    """Streams are keyed by the GLOBAL pixel index: interleaved shards reassemble to the single-call frame."""
    objs, cam, w, h = scenes.all_materials(pixels=14)
    s = rt.Scene.make(objs)
    full = s.render_rows(w, h, cam, seed=77)
    for world in (2, 3, 8):
        out = np.zeros_like(full.accum)
        for rank in range(world):
            part = s.render_rows(w, h, cam, seed=77, row_first=rank, row_stride=world)
            out[rank::world] = part.accum
        assert np.array_equal(out, full.accum)


def test_launch_configs_agree(rt):
    objs, cam, w, h = scenes.small_final(spp=24, pixels=10)
    s = rt.Scene.make(objs)
    base = s.render_rows(w, h, cam, seed=4).accum
    try:
        for block, chunk in ((256, 8), (512, 64), (1024, 16), (1024, 1)):
            rt.set_launch_config(block, chunk)
            assert np.array_equal(s.render_rows(w, h, cam, seed=4).accum, base), (block, chunk)
    finally:
        rt.set_launch_config(0, 0)


def test_seed_changes_the_image_and_same_seed_repeats(rt):
    objs, cam, w, h = scenes.all_materials(pixels=10)
    s = rt.Scene.make(objs)
    a, b, c = (s.render_rows(w, h, cam, seed=x).accum for x in (1, 1, 2))
    assert np.array_equal(a, b) and not np.array_equal(a, c)


def test_monte_carlo_energy_property_full_size(rt):
    """Size-independent property at BASELINE config 2's full size (801x451, 100 spp, depth 50): every Count is 11 or
    100, sums are bounded by 255*Count, sky pixels (dome seen directly) are exactly the dome colour and stop early."""
    objs, cam, w, h = rt.sample_images.config2_three_lambert()
    s = rt.Scene.make(objs)
    res = s.render_rows(w, h, cam, seed=6, counters=True)
    cnt = res.accum[..., 0]
    assert set(np.unique(cnt)) <= {11, 100}
    assert np.all(res.accum[..., 1:] <= 255 * cnt[..., None]) and np.all(res.accum[..., 1:] >= 0)
    top = res.accum[0]
    assert np.all(top[:, 0] == 11) and np.all(top[:, 1:] == 200 * 11)
    assert res.stats["samples"] == int(cnt.sum()) and res.stats["pixels_early"] == int((cnt == 11).sum())
    assert res.stats["rays"] >= res.stats["samples"]


# ---- committed golden fixtures and the device-buffer path -----------------------------------------------------------
@pytest.mark.parametrize("name", ["oracle_all_materials_seed0", "oracle_final_thumb_seed7", "oracle_config2_small_seed2", "oracle_earth_thumb_seed3"])
def test_hip_reproduces_the_committed_fixtures(rt, name):
    from test_oracle_render import FIXTURES, KEYS

    g = scenes.golden(name)
    objs, cam, w, h = FIXTURES[name](rt)
    for kind in ("sah", "reference"):
        res = _with_tree(rt, kind, lambda: rt.Scene.make(objs)).render_rows(w, h, cam, seed=int(g["seed"]), counters=True)
        assert np.array_equal(res.accum, g["accum"]) and np.array_equal(res.rgb, g["rgb"])
        want = dict(zip(KEYS, g["stats"].tolist()))
        for k in KEYS:  # the box-test count is the reference tree's; the default tree needs fewer
            assert res.stats[k] == want[k] or (k == "aabb_tests" and kind == "sah" and res.stats[k] < want[k]), (kind, k)


def test_config5_mixed_scene_thumbnail(rt, orc):
    """BASELINE config 5 geometry (final scene + earth-textured sphere + Dielectric sphere + mirror InfinitePlane), thumbnail."""
    earth = scenes.golden("earthmap_rgb")["rgb"]
    objs, cam, w, h = rt.sample_images.config5_mixed(earth, spp=30, pixels=14)
    _assert_render_equal(*_render_both(rt, orc, objs, cam, w, h, seed=13))


def test_device_buffer_path_and_frame_assembly(rt):
    """rt_render_device into a torch CUDA tensor on torch's current stream + gather_frame (world = 1), as bench.py uses it."""
    import torch

    from ray_tracing_fsharp_amd import distributed as rtd

    objs, cam, w, h = scenes.small_final(spp=24, pixels=10)
    s = rt.Scene.make(objs)
    want = s.render_rows(w, h, cam, seed=5).accum
    frame = rtd.render_frame(s, cam, w, h, seed=5, rank=0, world=1, device=0)
    torch.cuda.synchronize()
    assert np.array_equal(frame.cpu().numpy(), want)
    # an interleaved shard rendered into a padded buffer, as rank 1 of 3 would
    first, stride, n = rtd.shard_rows(2 * h + 1, 1, 3)
    local = torch.zeros(((2 * h + 1 + 2) // 3, 2 * w + 1, 4), dtype=torch.int32, device="cuda:0")
    st = rtd.render_shard_device(s, cam, w, h, 5, 0, first, stride, n, local, stream=torch.cuda.current_stream().cuda_stream, want_stats=True)
    assert np.array_equal(local[:n].cpu().numpy(), want[1::3]) and st["pixels"] == n * (2 * w + 1)


def test_full_size_config3_properties(rt):
    """BASELINE config 3 at full size (2401x1601, 500 spp, 50 bounces), through size-independent properties: Count is 11 or
    500 everywhere, sums bounded by 255*Count, samples = sum of Counts, sky rows are the dome colour exactly, the counters
    are those of the committed run (deterministic in the seed), and two launches give identical frames."""
    objs, cam, w, h = rt.sample_images.config3_final()
    s = rt.Scene.make(objs)
    a = s.render_rows(w, h, cam, seed=2024, counters=True)
    b = s.render_rows(w, h, cam, seed=2024)
    assert np.array_equal(a.accum, b.accum)
    cnt = a.accum[..., 0].astype(np.int64)
    assert set(np.unique(cnt)) <= {11, 500}
    assert np.all(a.accum[..., 1:] >= 0) and np.all(a.accum[..., 1:] <= 255 * cnt[..., None])
    assert a.stats["samples"] == int(cnt.sum()) and a.stats["pixels_early"] == int((cnt == 11).sum())
    assert np.all(a.accum[0, :, 0] == 11) and np.all(a.accum[0, :, 1:] == np.array([200, 200, 255]) * 11)
    assert a.stats["rays"] == a.stats["reflections"]  # the scene is closed: every ray hits something
    assert (a.stats["rays"], a.stats["prim_tests"], a.stats["samples"]) == (3503018818, 11481871042, 1079590420)
    if rt.get_walk_tree() == "reference":
        assert a.stats["aabb_tests"] == 98205213022  # BoundingBoxTree.make's tree: 28.0 box tests per ray
    else:
        lo = 0.5 if os.environ.get("RTFS_TUNE") == "1" else 0.7  # the surface-area tree over the same leaves; thinner still when tuned
        assert lo * 98205213022 < a.stats["aabb_tests"] < 0.92 * 98205213022
        rt.set_walk_tree("reference")
        try:
            c = rt.Scene.make(objs).render_rows(w, h, cam, seed=2024, counters=True)
        finally:
            rt.set_walk_tree("sah")
        assert np.array_equal(c.accum, a.accum) and c.stats["aabb_tests"] == 98205213022
        assert all(c.stats[k] == a.stats[k] for k in ("rays", "prim_tests", "reflections", "samples", "pixels_early"))


def test_walk_trees_agree_and_reference_tree_counts_match_oracle(rt, orc):
    """rt_set_walk_tree: the surface-area tree and BoundingBoxTree.make's own give the same PixelStats and the same
    rays / leaf tests / reflections / samples; walking the reference's tree, the box-test count equals the oracle's too."""
    for (objs, cam, w, h), seed in ((scenes.all_materials(), 4), (scenes.small_final(spp=30, pixels=24), 9), (scenes.many_spheres(), 2)):
        acc, rgb, st = orc.OracleScene(objs).render_rows(w, h, cam.to_abi(), seed=seed, threads=8)
        got = {}
        for kind in ("sah", "reference"):
            s = _with_tree(rt, kind, lambda: rt.Scene.make(objs))
            assert s.info()["walk_tree"] == {"sah": 0, "reference": 1}[kind] or (kind == "sah" and s.info()["n_bounded"] < 3)
            got[kind] = s.render_rows(w, h, cam, seed=seed, counters=True)
            assert np.array_equal(got[kind].accum, acc) and np.array_equal(got[kind].rgb, rgb)
            for k in ("rays", "prim_tests", "reflections", "samples", "pixels", "pixels_early"):
                assert got[kind].stats[k] == st[k], (kind, k)
        assert got["reference"].stats["aabb_tests"] == st["aabb_tests"]
        assert got["sah"].stats["aabb_tests"] <= st["aabb_tests"]
    rays = scenes.random_rays(40000, 77, origin_scale=4.0)
    objs, *_ = scenes.small_final()
    h2, s2, c2 = orc.OracleScene(objs).hit_object(rays)
    for kind in ("sah", "reference"):
        s = _with_tree(rt, kind, lambda: rt.Scene.make(objs))
        h1, s1, c1 = rt.hooks.hit_object(s, rays)
        assert np.array_equal(h1, h2) and _same_f64(s1, s2) and np.array_equal(c1[:, 1], c2[:, 1])
        assert np.array_equal(c1[:, 0], c2[:, 0]) == (kind == "reference")


def test_exact_ties_go_to_the_reference_walk_order(rt, orc):
    """Scene.fs:47's strict `<`: of several spheres hit at exactly the same t^2 the reference keeps the one its depth-first walk
    meets first.  Coincident spheres (same centre and radius, different colours and styles) among others, in shuffled
    input order: whichever tree the device walks, the winner -- hence every pixel -- is the oracle's."""
    S, H, P, Px, Tex = scenes.S, scenes.H, scenes.P, scenes.Px, scenes.Tex
    rng = np.random.default_rng(5)
    objs = []
    for c, r in ((P(0.0, 0.0, 2.0), 0.6), (P(1.0, 0.3, 2.5), 0.5), (P(-1.2, -0.2, 3.0), 0.7)):
        for k in range(5):  # five coincident copies each
            col = Px(*(int(x) for x in rng.integers(40, 256, 3)))
            st = [S.LightSource(Tex(col)), S.LambertReflection(0.8, Tex(col)), S.PureReflection(0.9, Tex(col)), S.Glass(0.9, Tex(col), 1.5),
                  S.FuzzedReflection(0.7, Tex(col), 0.2)][k]
            objs.append(H.Sphere(scenes.rt.Sphere.make(st, c, r)))
    for _ in range(12):
        objs.append(H.Sphere(scenes.rt.Sphere.make(S.LambertReflection(0.6, Tex(Px(*(int(x) for x in rng.integers(0, 256, 3))))),
                                                   P(*rng.uniform(-2.5, 2.5, 2), float(rng.uniform(1.0, 4.0))), float(rng.uniform(0.1, 0.4)))))
    objs.append(H.UnboundedSphere(scenes.rt.Sphere.make(S.LightSource(Tex(Px(210, 220, 255))), P(0.0, 0.0, 0.0), 100.0)))
    import dataclasses
    cam = dataclasses.replace(scenes.rt.Camera.makeBasic(16, 1.0, 1.5, P(0.0, 0.0, -1.0), scenes.unit(0.0, 0.0, 1.0), scenes.V(0.0, 1.0, 0.0)), BounceDepth=10)
    for trial in range(4):
        order = rng.permutation(len(objs))
        shuffled = [objs[i] for i in order]
        acc, rgb, st = orc.OracleScene(shuffled).render_rows(30, 20, cam.to_abi(), seed=trial, threads=8)
        for kind in ("sah", "reference"):
            s = _with_tree(rt, kind, lambda: rt.Scene.make(shuffled))
            res = s.render_rows(30, 20, cam, seed=trial, counters=True)
            assert np.array_equal(res.accum, acc), (trial, kind)
            assert res.stats["prim_tests"] == st["prim_tests"] and res.stats["rays"] == st["rays"]


def test_very_high_sample_count_takes_the_exact_division_path(rt, orc):
    """A unit of 16 pixels x 300 000 samples has more than 2^22 items: the sample -> pixel mapping falls back from the float
    reciprocal (rt_device.h div_uniform) to integer division.  Few pixels, so the oracle still finishes in seconds."""
    import dataclasses
    objs, cam, w, h = scenes.all_materials(spp=300000, depth=6, pixels=1)
    for passes in (1, 2):
        rt.set_passes(passes)
        try:
            res = rt.Scene.make(objs).render_rows(w, h, cam, seed=23, counters=True)
        finally:
            rt.set_passes(0)
        acc, rgb, st = orc.OracleScene(objs).render_rows(w, h, cam.to_abi(), seed=23, threads=8)
        assert np.array_equal(res.accum, acc) and res.stats["samples"] == st["samples"] and res.stats["rays"] == st["rays"]
        assert res.accum[..., 0].max() == 300000


def test_order_of_bounded_objects_does_not_change_a_pixel(rt):
    """Permuting the bounded spheres changes both trees (the reference's and the walked one) and the object ranks, not one sum."""
    objs, cam, w, h = scenes.small_final(seed=11, spp=24, depth=30, pixels=20)
    base = rt.Scene.make(objs).render_rows(w, h, cam, seed=4, counters=True)
    rng = np.random.default_rng(8)
    bounded = [i for i, o in enumerate(objs) if o.kind == 0]
    for _ in range(4):
        perm = list(range(len(objs)))
        for dst, src in zip(bounded, rng.permutation(bounded)):
            perm[dst] = int(src)
        res = rt.Scene.make([objs[i] for i in perm]).render_rows(w, h, cam, seed=4, counters=True)
        assert np.array_equal(res.accum, base.accum)
        assert all(res.stats[k] == base.stats[k] for k in ("rays", "prim_tests", "reflections", "samples"))


def test_six_thousand_spheres_binned_tree_build(rt, orc):
    """Above 4096 leaves per node the surface-area build switches from a full sweep to 32 centroid bins (rt_scene.h): same bar."""
    objs, cam, w, h = scenes.many_spheres(n=6000, seed=4, spp=8, depth=6, pixels=8)
    s = _with_tree(rt, "sah", lambda: rt.Scene.make(objs))
    assert s.info()["walk_tree"] == 0 and s.info()["lds_resident"] == 0
    res = s.render_rows(w, h, cam, seed=17, counters=True)
    acc, rgb, st = orc.OracleScene(objs).render_rows(w, h, cam.to_abi(), seed=17, threads=8)
    assert np.array_equal(res.accum, acc) and np.array_equal(res.rgb, rgb)
    assert all(res.stats[k] == st[k] for k in ("rays", "prim_tests", "reflections", "samples")) and res.stats["aabb_tests"] < st["aabb_tests"]
    plain = s.render_rows(w, h, cam, seed=17)
    assert np.array_equal(plain.accum, acc) and np.array_equal(plain.rgb, rgb)


def _cpu_quota():
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            return max(1, int(int(q) / int(per)))
    except (OSError, ValueError):
        pass
    return os.cpu_count() or 1


def test_full_size_config3_equals_the_oracle(rt, orc):
    """The metric's own frame -- BASELINE config 3, 2401x1601 px, 500 spp, 50 bounces, 3.5e9 rays -- against the oracle, whole:
    every one of the 3,844,001 PixelStats, and the ray / leaf-test / reflection / sample counts (the box-test count under the
    reference's tree is pinned by test_full_size_config3_properties).  The oracle needs ~45 s on the GPU box's 16 CPUs."""
    objs, cam, w, h = rt.sample_images.config3_final()
    res = rt.Scene.make(objs).render_rows(w, h, cam, seed=2024, counters=True)
    acc, rgb, st = orc.OracleScene(objs).render_rows(w, h, cam.to_abi(), seed=2024, threads=min(32, _cpu_quota()))
    assert np.array_equal(res.accum, acc)
    assert np.array_equal(res.rgb, rgb)
    for k in ("rays", "prim_tests", "reflections", "samples", "pixels", "pixels_early"):
        assert res.stats[k] == st[k], k
    assert st["aabb_tests"] == 98205213022 and st["rays"] == 3503018818


def test_scene_larger_than_lds_uses_the_global_memory_kernel(rt, orc):
    """2600 spheres flatten to ~350 KB > 160 KiB of LDS: the LDS=false variant of the render kernel, same bit-exact bar."""
    objs, cam, w, h = scenes.many_spheres()
    s = rt.Scene.make(objs)
    info = s.info()
    assert info["lds_resident"] == 0 and info["scene_bytes"] > 163840 and info["n_nodes"] == 2 * 2600 - 1
    res = s.render_rows(w, h, cam, seed=31, counters=True)
    acc, rgb, st = orc.OracleScene(objs).render_rows(w, h, cam.to_abi(), seed=31, threads=8)
    _assert_render_equal(res, acc, rgb, st)
    plain = s.render_rows(w, h, cam, seed=31)  # the timed variant: filter records, the tree's upper levels in LDS, the rest from global memory
    assert np.array_equal(plain.accum, acc) and np.array_equal(plain.rgb, rgb)


@pytest.mark.parametrize("n,textured", [(900, False), (1300, True), (1700, False), (4000, True), (17000, False)])
@pytest.mark.parametrize("passes", [1, 2])
def test_tree_partly_in_lds(rt, orc, n, textured, passes):
    """Scenes that do not fit the LDS keep the first records of their depth-ordered filter tree there (node_loop_glb32): sizes where
    the whole tree still fits (900), where the split falls in the lower levels (1300, 1700), where it falls high (4000), and beyond the
    16384 objects a 14-bit queue entry can name (17000); fused and two-pass launches (their LDS budgets differ); as built and tuned
    (the tuner reorders and thins the tree, so the split moves).  Timed variant against the oracle, every pixel."""
    objs, cam, w, h = scenes.many_spheres(n=n, seed=40 + n % 7, spp=20, depth=10, pixels=12)
    objs = list(objs)
    chk = rt.ParameterisedTexture.Checkered(rt.ParameterisedTexture.UvRamp("u", 40, "v"), rt.ParameterisedTexture.Colour(rt.Pixel(20, 60, 20)), 30.0)
    centre = rt.Point.make(0.0, 1.0, 2.0)  # with one parameterised texture the launches below are the textured kernel variants
    if textured:
        objs[3] = rt.Hittable.Sphere(rt.Sphere.make(rt.SphereStyle.LambertReflection(0.8, rt.ParameterisedTexture.toTexture((0.9, centre), chk)), centre, 0.9))
    s = rt.Scene.make(objs)
    assert s.info()["lds_resident"] == 0
    acc, rgb, st = orc.OracleScene(objs).render_rows(w, h, cam.to_abi(), seed=5, threads=8)
    try:
        rt.set_passes(passes)
        plain = s.render_rows(w, h, cam, seed=5)
        assert np.array_equal(plain.accum, acc) and np.array_equal(plain.rgb, rgb), "as built"
        s.tune(w, h, cam, seed=5)
        tuned = s.render_rows(w, h, cam, seed=5)
        assert np.array_equal(tuned.accum, acc) and np.array_equal(tuned.rgb, rgb), "tuned"
        counted = s.render_rows(w, h, cam, seed=5, counters=True)
        assert np.array_equal(counted.accum, acc) and all(counted.stats[k] == st[k] for k in ("rays", "prim_tests", "reflections", "samples"))
    finally:
        rt.set_passes(0)


@pytest.mark.parametrize("seed", range(40))
def test_random_scenes_fuzz(rt, orc, seed):
    """Random small scenes (every style, both radius signs, planes, parameterised textures, cameras inside objects, bounce depths
    from 0): exact."""
    objs, cam, w, h = scenes.random_scene(1000 + seed)
    _assert_render_equal(*_render_both(rt, orc, objs, cam, w, h, seed=seed))


def test_edge_shards_and_extremes(rt, orc):
    """Empty shards (more ranks than rows), a one-row image, one-pixel-wide units, spp far above the pixel count, depth 0."""
    objs, cam, w, h = scenes.all_materials(pixels=3)
    s, o = rt.Scene.make(objs), orc.OracleScene(objs)
    rows = 2 * h + 1
    empty = s.render_rows(w, h, cam, seed=1, row_first=rows + 5, row_stride=rows + 9, n_rows=0)
    assert empty.accum.shape[0] == 0 and empty.stats["samples"] == 0
    one = s.render_rows(w, h, cam, seed=1, row_first=rows - 1, row_stride=1, n_rows=1, counters=True)
    acc, rgb, st = o.render_rows(w, h, cam.to_abi(), seed=1, row_first=rows - 1, row_stride=1, n_rows=1)
    _assert_render_equal(one, acc, rgb, st)
    big = dataclasses.replace(cam, SamplesPerPixel=3000, BounceDepth=0)
    try:
        rt.set_launch_config(256, 1)
        res = s.render_rows(1, 1, big, seed=2, counters=True)
    finally:
        rt.set_launch_config(0, 0)
    acc, rgb, st = o.render_rows(1, 1, big.to_abi(), seed=2, threads=4)
    _assert_render_equal(res, acc, rgb, st)
    assert set(np.unique(res.accum[..., 0])) <= {11, 3000}


def test_config5_full_geometry_row(rt, orc):
    """BASELINE config 5 at full geometry (2401x1601, 2000 spp): one image row through the textured sphere and the mirror plane."""
    earth = scenes.golden("earthmap_rgb")["rgb"]
    objs, cam, w, h = rt.sample_images.config5_mixed(earth)
    assert cam.SamplesPerPixel == 2000 and (w, h) == (1200, 800)
    s, o = rt.Scene.make(objs), orc.OracleScene(objs)
    assert s.info()["texel_bytes"] >= 1024 * 512 * 3
    res = s.render_rows(w, h, cam, seed=5, row_first=700, row_stride=1, n_rows=1, counters=True)
    acc, rgb, st = o.render_rows(w, h, cam.to_abi(), seed=5, row_first=700, row_stride=1, n_rows=1, threads=8)
    _assert_render_equal(res, acc, rgb, st)
    assert set(np.unique(res.accum[..., 0])) <= {11, 2000}


def test_config5_whole_frame_at_100_spp(rt, orc):
    """BASELINE config 5's scene and image size, whole frame, at 100 of its 2000 samples per pixel (the oracle then needs ~15 s):
    earth-textured sphere, Dielectric sphere, mirror InfinitePlane, the 485 spheres: every PixelStats and every counter."""
    earth = scenes.golden("earthmap_rgb")["rgb"]
    objs, cam, w, h = rt.sample_images.config5_mixed(earth, spp=100)
    res = rt.Scene.make(objs).render_rows(w, h, cam, seed=5, counters=True)
    acc, rgb, st = orc.OracleScene(objs).render_rows(w, h, cam.to_abi(), seed=5, threads=min(32, _cpu_quota()))
    _assert_render_equal(res, acc, rgb, st)
    assert res.stats["pixels"] == (2 * w + 1) * (2 * h + 1)
    # the textured kernel that is timed (no counters): the same frame
    timed = rt.Scene.make(objs).render_rows(w, h, cam, seed=5)
    assert np.array_equal(timed.accum, acc) and np.array_equal(timed.rgb, rgb)


@pytest.mark.parametrize("chunk", [0, 1, 5, 64])
def test_two_pass_rendering_equals_fused(rt, orc, chunk):
    """rt_set_passes: phase 1 + decision as one launch, a cost-ordered list, phase 2 as another (used for small shards) gives
    the very same integers as the fused kernel and the oracle, counters included."""
    objs, cam, w, h = scenes.small_final(spp=30, pixels=10)
    s = rt.Scene.make(objs)
    acc, rgb, st = orc.OracleScene(objs).render_rows(w, h, cam.to_abi(), seed=6, threads=8)
    try:
        rt.set_launch_config(0, chunk)
        for passes in (1, 2):
            rt.set_passes(passes)
            _assert_render_equal(s.render_rows(w, h, cam, seed=6, counters=True), acc, rgb, st)
        objs2, cam2, w2, h2 = scenes.all_materials(pixels=9)
        rt.set_passes(2)
        res = rt.Scene.make(objs2).render_rows(w2, h2, cam2, seed=8, row_first=1, row_stride=2, counters=True)
        acc2, rgb2, st2 = orc.OracleScene(objs2).render_rows(w2, h2, cam2.to_abi(), seed=8, row_first=1, row_stride=2, threads=8)
        _assert_render_equal(res, acc2, rgb2, st2)
    finally:
        rt.set_passes(0)
        rt.set_launch_config(0, 0)
