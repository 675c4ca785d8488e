"""Textures built to sit where Texture.colourAt on the device (texture_colour_at_inline, csrc/rt_device.h) is most likely to go wrong,
and the points / rays to evaluate them at.  Shared by tests/test_texture_model.py (the oracle against the line-by-line restatement in
tests/fsharp_literal.py, on the CPU) and tests/test_gpu_textures.py (the device against the oracle, through every route that evaluates
a texture).  No GPU and no oracle in here.

Every case is a scene: hittables that wear textures, as the ABI arrays rt_scene_create takes.  Cases the host mirror can express are
built from its objects (ParameterisedTexture -> flatten_hittables, so that route is exercised too) and keep them in `objs`; the others
(shared children, chosen record numbers) are raw rt_texture records and `objs` is None.  A query names a hittable, the texture id it
wears, points to evaluate that texture at (the hook and the strike points of Hittable.reflection) and rays that hit the hittable (for
Scene.traceRay; their strike points are the device's own).

Scene layout: wearer i sits at (8 i, 0, 0) with radius 1 unless the family says otherwise, far enough apart that a ray aimed at one
from 3 radii away meets no other; a plain grey LightSource shell of radius 2000 around everything gives bounced paths a colour.
"""
import ctypes as C
import dataclasses
from typing import List, Optional

import numpy as np

import ray_tracing_fsharp_amd as rt
import scenes
from ray_tracing_fsharp_amd import _abi as A
from ray_tracing_fsharp_amd.raytracing import flatten_hittables

P = rt.Point.make
S, PS, H, PT, Px = rt.SphereStyle, rt.InfinitePlaneStyle, rt.Hittable, rt.ParameterisedTexture, rt.Pixel
PI = np.pi
SPACING = 8.0


@dataclasses.dataclass
class Query:
    hittable: int        # index into the scene's hittables
    texture: int         # the rt_texture id it wears
    points: np.ndarray   # [n, 3]
    rays: np.ndarray     # [m, 6] origin, vector: aimed at the hittable
    on_map: bool = True  # the points were built ON the texture's map sphere (the 99 % condition of test_texture_model applies)


@dataclasses.dataclass
class Case:
    name: str
    hs: object           # (rt_hittable * n)
    n: int
    tex: object          # (rt_texture * ntex)
    ntex: int
    keep: list           # texel arrays the records point at
    objs: Optional[list]
    queries: List[Query]

    def arrays(self):
        return self.hs, self.n, self.tex, self.ntex, self.keep


def colour_of(k):
    """Distinct colours, none black (the device's answer when a descent is cut short), none equal to the sky's grey."""
    k = int(k)
    return Px(1 + (k * 37) % 251, 1 + (k * 101 + 7) % 253, 3 + (k % 250))


def sky():
    return H.UnboundedSphere(rt.Sphere.make(S.LightSource(rt.Texture.Colour(Px(200, 200, 200))), P(0.0, 0.0, 0.0), 2000.0))


def centre_of(i):
    return np.array([SPACING * i, 0.0, 0.0])


def plane_map(radius, centre, u, v):
    """Sphere.planeMap (Sphere.fs:47-52) in numpy: the point of the map sphere that planeMapInverse sends (near) (u, v)."""
    theta, phi = np.asarray(v) * PI, np.asarray(u) * PI * 2.0 - PI
    return np.asarray(centre) + np.stack([radius * np.cos(phi) * np.sin(theta), -radius * np.cos(theta), -radius * np.sin(phi) * np.sin(theta)], axis=-1)


def uniform_uv(rng, n, u=(0.0, 1.0), v=(0.0, 1.0)):
    return rng.uniform(u[0], u[1], n), rng.uniform(v[0], v[1], n)


def rays_at_sphere(rng, centre, radius, n):
    """Rays from 3 radii out that hit the sphere (aimed at a point of it, a little off the normal)."""
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t = rng.normal(size=(n, 3)) * 0.3
    o = np.asarray(centre) + 3.0 * abs(radius) * d
    target = np.asarray(centre) + abs(radius) * (d + t) / np.linalg.norm(d + t, axis=1, keepdims=True)
    return np.concatenate([o, target - o], axis=1)


def rays_at_points(centre, points, rng):
    """Rays from outside the sphere around `centre` towards `points` on it."""
    n = points - np.asarray(centre)
    o = np.asarray(centre) + 3.0 * n + rng.normal(size=n.shape) * 0.2 * np.linalg.norm(n, axis=1, keepdims=True)
    return np.concatenate([o, points - o], axis=1)


# ---- records by hand -------------------------------------------------------------------------------------------------------
def rec_colour(p):
    r = A.rt_texture()
    r.kind, r.even, r.odd, r.map_radius = A.RT_TEXTURE_COLOUR, -1, -1, 1.0
    r.rgb[:] = tuple(p)
    return r


def rec_checkered(even, odd, grid):
    r = rec_colour((0, 0, 0))
    r.kind, r.even, r.odd, r.grid_size = A.RT_TEXTURE_CHECKERED, int(even), int(odd), float(grid)
    return r


def rec_ramp(src, const=(0, 0, 0)):
    r = rec_colour(const)
    r.kind = A.RT_TEXTURE_UV_RAMP
    r.ramp_src[:] = tuple(src)
    return r


def rec_image(img, keep):
    img = np.ascontiguousarray(img, np.uint8)
    keep.append(img)
    r = rec_colour((0, 0, 0))
    r.kind, r.height, r.width, r.texels = A.RT_TEXTURE_IMAGE, img.shape[0], img.shape[1], img.ctypes.data
    return r


def set_map(r, radius, centre):
    r.map_radius = float(radius)
    r.map_centre[:] = tuple(float(c) for c in centre)
    return r


def raw_sphere(style, centre, radius, texture, albedo=0.9, rgb=(9, 9, 9), kind=A.RT_HITTABLE_SPHERE):
    h = A.rt_hittable()
    h.kind, h.style, h.radius, h.albedo, h.fuzz, h.ior, h.prob, h.texture = kind, style, float(radius), albedo, 0.2, 1.5, 0.5, int(texture)
    h.point[:] = tuple(float(c) for c in centre)
    h.rgb[:] = rgb
    return h


def raw_case(name, hittables, records, keep, queries):
    hs = (A.rt_hittable * len(hittables))(*hittables)
    tex = (A.rt_texture * len(records))(*records)
    return Case(name, hs, len(hittables), tex, len(records), keep, None, queries)


def mirror_case(name, objs, queries_for):
    """objs: host-mirror hittables; queries_for(hs) -> queries, given the flattened hittables (which carry the texture ids)."""
    hs, n, tex, ntex, keep = flatten_hittables(objs)
    return Case(name, hs, n, tex, ntex, keep, list(objs), queries_for(hs))


def synthetic_image(h, w, salt=0):
    """Texel (x, y) -> a colour that is a one-to-one function of (x, y) (and never black)."""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.stack([x & 255, (y & 255) ^ (salt & 255), 1 + ((x >> 8) | ((y >> 8) << 2)) + 4 * (salt % 60)], axis=-1).astype(np.uint8)


STYLES = (lambda t: S.LightSource(t), lambda t: S.LambertReflection(0.9, t), lambda t: S.PureReflection(0.95, t))


def wear(i, param, style=None, radius=1.0, map_radius=None, map_centre=None):
    c = centre_of(i)
    t = PT.toTexture((radius if map_radius is None else map_radius, P(*(c if map_centre is None else map_centre))), param)
    return H.Sphere(rt.Sphere.make((style or STYLES[i % 3])(t), P(*c), radius))


def sphere_queries(hs, n_wearers, rng, n_points, uv=None):
    out = []
    for i in range(n_wearers):
        c, r = centre_of(i), hs[i].radius
        u, v = uv(i) if uv else uniform_uv(rng, n_points)
        pts = plane_map(r, c, u, v)
        out.append(Query(i, hs[i].texture, pts, rays_at_points(c, pts[: max(1, len(pts) // 2)], rng)))
    return out


# ---- chains ----------------------------------------------------------------------------------------------------------------
def chain_grid(k, depth):
    """Level k of `depth` (0 = the root): distinct per level.  Ordinary levels (odd = the deeper level, even = this level's leaf) take
    pi (1 + (k + 1) / (4 depth)): sin(g u) sin(g v) > 0 below u, v < 1 / (1 + (k + 1) / (4 depth)), so a point with v < 0.45 descends
    until its u crosses that threshold -- exits spread over all levels for u in (0.8, 1).  Every 7th level from the third is turned
    round (even = the deeper level) with g = 2 pi (1 + (k + 1) / (100 depth)): negative, hence deeper, for u in (0.55, 0.95), v in
    (0.05, 0.45); positive, hence out, for u, v < 0.45."""
    turned = k % 7 == 2
    return turned, (2.0 * PI * (1.0 + (k + 1) / (100.0 * depth)) if turned else PI * (1.0 + (k + 1) / (4.0 * depth)))


def chain_param(depth):
    node = PT.Colour(colour_of(depth))
    for k in range(depth - 1, -1, -1):
        turned, g = chain_grid(k, depth)
        leaf = PT.Colour(colour_of(k))
        node = PT.Checkered(node, leaf, g) if turned else PT.Checkered(leaf, node, g)
    return node


def chain_uv(rng, n):
    """60 % ride the chain down (u in (0.55, 0.95): those above 0.8 leave at an ordinary level on the way, the rest reach the last
    leaf), 15 % leave at the first turned level, 25 % anywhere on the sphere."""
    a, b = int(n * 0.6), int(n * 0.15)
    u = np.concatenate([rng.uniform(0.55, 0.95, a), rng.uniform(0.05, 0.45, b), rng.uniform(0.0, 1.0, n - a - b)])
    v = np.concatenate([rng.uniform(0.05, 0.45, a), rng.uniform(0.05, 0.45, b), rng.uniform(0.0, 1.0, n - a - b)])
    return u, v


CHAIN_DEPTHS = (1, 2, 15, 16, 17, 40, 126)


def family_chains(seed=1):
    rng = np.random.default_rng(seed)
    for depth in CHAIN_DEPTHS:
        style = STYLES[1] if depth in (16, 40) else STYLES[0]
        objs = [wear(0, chain_param(depth), style), sky()]
        yield mirror_case(f"depth{depth}", objs, lambda hs: sphere_queries(hs, 1, rng, 0, uv=lambda i: chain_uv(rng, 1200)))
    # 253 Checkered records over ONE leaf (254 records: the most a scene holds): odd = the record below, even = up to four further down
    depth = 253
    recs = [rec_colour(colour_of(depth))]
    for k in range(1, depth + 1):
        recs.append(rec_checkered(max(0, k - 1 - k % 5), k - 1, PI * (1.0 + k / (4.0 * depth))))
    set_map(recs[depth], 1.0, centre_of(0))
    hitt = [raw_sphere(A.RT_SPHERE_LIGHT_SOURCE, centre_of(0), 1.0, depth), flatten_hittables([sky()])[0][0]]
    pts = plane_map(1.0, centre_of(0), *chain_uv(rng, 400))
    yield raw_case("depth253_shared", hitt, recs, [], [Query(0, depth, pts, rays_at_points(centre_of(0), pts[:200], rng))])


# ---- trees -----------------------------------------------------------------------------------------------------------------
def family_trees(seed=2):
    rng = np.random.default_rng(seed)
    count = [0]

    def leaf():
        k = count[0]
        count[0] += 1
        if k % 3 == 0:
            return PT.Colour(colour_of(k))
        if k % 3 == 1:
            return PT.UvRamp(*[("u", "v", 1 + k)[(k // 3 + j) % 3] for j in range(3)])
        return PT.Image(synthetic_image(2 + k % 3, 3 + k % 4, salt=k))

    def node(d):
        # the grid doubles from level to level (and differs a little from node to node): the signs of sin(g u) sin(g v) at the six
        # levels are then independent of each other, and every one of the 64 leaves owns a fair share of the sphere
        return leaf() if d == 0 else PT.Checkered(node(d - 1), node(d - 1), PI * 2.0 ** (7 - d) * float(rng.uniform(1.0, 1.02)))

    objs = [wear(0, node(6), STYLES[1]), sky()]
    yield mirror_case("balanced6", objs, lambda hs: sphere_queries(hs, 1, rng, 4000))


# ---- images ----------------------------------------------------------------------------------------------------------------
IMAGE_SIZES = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (3, 257))  # (height, width): 1x1, 1xN, Nx1, 2x2, 3x5, 257x3 (width x height)


def seam_uv(rng, n):
    """uniform, plus the seam (u next to 0 and 1), the poles (v next to 0 and 1) and texel boundaries"""
    u, v = uniform_uv(rng, n)
    k = n // 8
    u[:k] = rng.choice([0.0, 1.0, 1e-17, 1.0 - 2.0 ** -53, 0.5, 0.25], k)
    v[k:2 * k] = rng.choice([0.0, 1.0, 1e-9, 1.0 - 1e-9, 0.5], k)
    u[2 * k:3 * k] = rng.integers(0, 257, k) / 256.0
    v[3 * k:4 * k] = rng.integers(0, 5, k) / 4.0
    return u, v


def family_images(seed=3):
    rng = np.random.default_rng(seed)
    params = [PT.Image(synthetic_image(h, w, salt=i)) for i, (h, w) in enumerate(IMAGE_SIZES)]
    # an image as a leaf below two Checkered levels
    params.append(PT.Checkered(PT.Checkered(PT.Image(synthetic_image(5, 9, salt=9)), PT.Colour(colour_of(1)), 7.0), PT.Image(synthetic_image(4, 3, salt=11)), 5.0))
    objs = [wear(i, p) for i, p in enumerate(params)] + [sky()]
    yield mirror_case("synthetic", objs, lambda hs: sphere_queries(hs, len(params), rng, 0, uv=lambda i: seam_uv(rng, 1200)))
    earth = scenes.golden("earthmap_rgb")["rgb"]
    # the earth map BEHIND a small image (a nonzero, 16-byte padded texel offset), through ofImage's row reversal
    objs = [wear(0, PT.Image(synthetic_image(3, 3))), wear(1, PT.ofImage(earth), STYLES[0]), wear(2, PT.Image(synthetic_image(1, 2, salt=3))), sky()]
    yield mirror_case("earth", objs, lambda hs: sphere_queries(hs, 3, rng, 0, uv=lambda i: seam_uv(rng, 3000 if i == 1 else 300)))


# ---- ramps -----------------------------------------------------------------------------------------------------------------
def family_ramps(seed=4):
    rng = np.random.default_rng(seed)
    combos = [(a, b, c) for a in range(3) for b in range(3) for c in range(3)]  # rt_ramp_source per channel
    params = [PT.UvRamp(*[(10 + 9 * i + j, "u", "v")[s] for j, s in enumerate(combo)]) for i, combo in enumerate(combos)]
    objs = [wear(i, p) for i, p in enumerate(params)] + [sky()]
    yield mirror_case("all27", objs, lambda hs: sphere_queries(hs, len(params), rng, 0, uv=lambda i: seam_uv(rng, 320)))


# ---- grids -----------------------------------------------------------------------------------------------------------------
GRIDS = (0.0, -0.0, -7.5, -1e-300, 1e-300, 1.0, PI, 2.0 * PI, 3.0 * PI, 10.0 * PI, 1000.0 * PI, 499999.5, 5e5, -5e5)


def family_grids(seed=5):
    rng = np.random.default_rng(seed)
    params = [PT.Checkered(PT.Colour(colour_of(2 * i)), PT.Colour(colour_of(2 * i + 1)), g) for i, g in enumerate(GRIDS)]
    objs = [wear(i, p) for i, p in enumerate(params)] + [sky()]

    def uv(i):
        u, v = seam_uv(rng, 600)
        g = abs(GRIDS[i])
        if g >= 1.0:  # points next to the lines sin(g u) = 0, where the sign -- and the 1e-8 band of Float.compare -- decides
            k = rng.integers(0, max(1, int(g / PI)) + 1, 200)
            u[-200:] = np.clip(k * PI / g + rng.choice([0.0, 1e-12, -1e-12, 1e-9, -1e-9, 1e-7, -1e-7], 200), 0.0, 1.0)
        return u, v
    yield mirror_case("grids", objs, lambda hs: sphere_queries(hs, len(params), rng, 0, uv=uv))


# ---- maps ------------------------------------------------------------------------------------------------------------------
def axis_points(radius):
    """(+-r, +-0, +-0), (+-0, +-r, +-0), (+-0, +-0, +-r): the poles and the seam with both signs of every zero."""
    out = []
    for axis in range(3):
        for s in (1.0, -1.0):
            for z1 in (0.0, -0.0):
                for z2 in (0.0, -0.0):
                    p = [z1, z2]
                    p.insert(axis, s * radius)
                    out.append(p)
    return np.array(out)


def nudged(points):
    """every point with ONE coordinate moved by -2, -1, 1 or 2 ulps: just inside and just outside the map sphere"""
    out = []
    for axis in range(3):
        for steps in (-2, -1, 1, 2):
            q = points.copy()
            x = q[:, axis]
            for _ in range(abs(steps)):
                x = np.nextafter(x, np.inf if steps > 0 else -np.inf)
            q[:, axis] = x
            out.append(q)
    return np.concatenate(out)


def map_param(salt):
    return PT.Checkered(PT.Image(synthetic_image(5, 7, salt=salt)), PT.UvRamp("u", "v", 40 + salt), 6.0)


def family_maps(seed=6):
    rng = np.random.default_rng(seed)
    # (a) the map sphere AT the origin (so that the signs of zero coordinates survive the subtraction of the centre), radii 1 and 0.375:
    #     poles, seam, random points, and all of them nudged by ulps.  One wearer per texture kind at the root.
    for radius in (1.0, 0.375):
        params = [map_param(1), PT.Image(synthetic_image(3, 257)), PT.UvRamp("u", "v", "u"), PT.Image(synthetic_image(1, 1, salt=5))]
        objs = [H.Sphere(rt.Sphere.make(STYLES[i % 3](PT.toTexture((radius, P(0.0, 0.0, 0.0)), p)), P(*centre_of(i)), 1.0)) for i, p in enumerate(params)] + [sky()]

        def queries(hs, radius=radius, n=len(params)):
            base = np.concatenate([axis_points(radius), plane_map(radius, (0.0, 0.0, 0.0), *seam_uv(rng, 80))])
            pts = np.concatenate([base, nudged(base)])
            return [Query(i, hs[i].texture, pts, rays_at_sphere(rng, centre_of(i), 1.0, 300), on_map=False) for i in range(n)]
        yield mirror_case(f"origin_r{radius:g}", objs, queries)
    # (b) a texture built for one (radius, centre), worn by a sphere with another; negative, tiny, huge and zero map radii
    maps = [(1.0, (0.3, 0.2, -0.1)), (2.5, None), (0.5, None), (-1.0, None), (-0.25, (0.0, 0.5, 0.0)), (1e-300, None), (1e-310, None),
            (1e300, None), (0.0, None), (-0.0, None), (5e-324, None)]
    objs = []
    for i, (mr, off) in enumerate(maps):
        mc = centre_of(i) + (np.zeros(3) if off is None else np.array(off))
        objs.append(wear(i, map_param(i), map_radius=mr, map_centre=mc))
    objs.append(sky())

    def queries(hs):
        out = []
        for i, (mr, off) in enumerate(maps):
            c = centre_of(i)
            d = rng.normal(size=(300, 3))
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            pts = np.concatenate([c + d, c + axis_points(1.0), c + np.zeros((1, 3)), c + d * abs(mr) if np.isfinite(abs(mr)) and 1e-3 < abs(mr) < 10 else c + d * 0.5])
            out.append(Query(i, hs[i].texture, pts, rays_at_sphere(rng, c, 1.0, 300), on_map=False))
        return out
    yield mirror_case("foreign", objs, queries)


# ---- ids -------------------------------------------------------------------------------------------------------------------
ID_WEARERS = (0, 126, 127, 128, 253)


def family_ids(seed=7):
    rng = np.random.default_rng(seed)
    keep, recs = [], []
    for k in range(254):  # record k: a colour (k % 3 == 0, and 1), a Checkered over the two records before it (k % 3 == 1), a ramp
        if k % 3 == 0 or k < 2:
            recs.append(rec_colour(colour_of(k)))
        elif k % 3 == 1:
            recs.append(rec_checkered(k - 1, k - 2, 2.0 + k / 16.0))
        else:
            recs.append(rec_ramp((A.RT_RAMP_U, A.RT_RAMP_CONST, A.RT_RAMP_V), (0, 1 + k, 0)))
    hitt, queries = [], []
    for i, k in enumerate(ID_WEARERS):
        set_map(recs[k], 1.0, centre_of(i))
        hitt.append(raw_sphere((A.RT_SPHERE_LIGHT_SOURCE, A.RT_SPHERE_LAMBERT_REFLECTION, A.RT_SPHERE_GLASS)[i % 3], centre_of(i), 1.0, k))
        pts = plane_map(1.0, centre_of(i), *uniform_uv(rng, 600))
        queries.append(Query(i, k, pts, rays_at_points(centre_of(i), pts[:300], rng)))
    hitt.append(flatten_hittables([sky()])[0][0])
    yield raw_case("ids254", hitt, recs, keep, queries)


# ---- wearers ---------------------------------------------------------------------------------------------------------------
def family_wearers(seed=8):
    rng = np.random.default_rng(seed)
    styles = [lambda t: S.LightSource(t), lambda t: S.PureReflection(0.9, t), lambda t: S.FuzzedReflection(0.85, t, 0.3),
              lambda t: S.LambertReflection(0.8, t), lambda t: S.Dielectric(0.9, t, 1.4, 0.6), lambda t: S.Glass(0.95, t, 1.5)]
    objs = [wear(i, map_param(20 + i), st) for i, st in enumerate(styles)]
    n = len(objs)

    def tex_for(i, radius):
        return PT.toTexture((radius, P(*centre_of(i))), map_param(30 + i))
    objs.append(H.UnboundedSphere(rt.Sphere.make(S.LambertReflection(0.9, tex_for(n, 1.0)), P(*centre_of(n)), 1.0)))
    objs.append(H.UnboundedSphere(rt.Sphere.make(S.Glass(0.95, tex_for(n + 1, -0.8), 1.0 / 1.5), P(*centre_of(n + 1)), -0.8)))
    plane_at = np.array([0.0, -6.0, 0.0])
    objs.append(H.InfinitePlane(rt.InfinitePlane.make(PS.LightSource(PT.toTexture((1.0, P(0.0, 0.0, 0.0)), map_param(40))), P(*plane_at), scenes.unit(0.0, 1.0, 0.0))))
    objs.append(sky())

    def queries(hs):
        out = sphere_queries(hs, n + 2, rng, 700)
        t = rng.normal(size=(700, 3)) * 20.0
        t[:, 1] = 0.0
        pts = plane_at + t
        o = pts[:350] + np.array([0.0, 2.0, 0.0]) + rng.normal(size=(350, 3)) * 0.3
        out.append(Query(n + 2, hs[n + 2].texture, pts, np.concatenate([o, pts[:350] - o], axis=1), on_map=False))
        return out
    yield mirror_case("styles", objs, queries)


FAMILIES = {"chains": family_chains, "trees": family_trees, "images": family_images, "ramps": family_ramps, "grids": family_grids,
            "maps": family_maps, "ids": family_ids, "wearers": family_wearers}


# ---- a frame whose hits are mostly textured (for stage_tex's own park pool) ----------------------------------------------------
def mostly_textured_scene(spp=16, depth=6, pixels=14):
    """The wearers of every style on a Checkered ground sphere, seen from above (no sky in the frame): every primary hit, and nearly
    every later one, evaluates a texture."""
    case = next(family_wearers())
    objs = [o for o in case.objs if o.kind != A.RT_HITTABLE_INFINITE_PLANE]
    ground_c = P(24.0, -1001.0, 0.0)
    ground = PT.Checkered(PT.UvRamp("u", 90, "v"), PT.Checkered(PT.Colour(colour_of(5)), PT.Colour(colour_of(6)), 40000.0), 9000.0)
    objs.insert(0, H.Sphere(rt.Sphere.make(S.LambertReflection(0.8, PT.toTexture((1000.0, ground_c), ground)), ground_c, 1000.0)))
    aspect = 2.0
    cam = dataclasses.replace(rt.Camera.makeBasic(spp, 1.6, aspect, P(24.0, 9.0, -2.0), scenes.unit(0.0, -4.0, 1.0), rt.Vector.make(0.0, 1.0, 0.0)), BounceDepth=depth)
    return objs, cam, int(aspect * pixels), pixels


def texels_of(t):
    """The [height, width, 3] texels an IMAGE record points at."""
    n = t.height * t.width * 3
    return np.frombuffer(C.string_at(t.texels, n), np.uint8).reshape(t.height, t.width, 3)
