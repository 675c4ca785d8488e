"""Path vertices built to sit where Hittable.Reflection (csrc/rt_device.h `reflection`, `reflection_fast`, `lambert_inside` +
`lambert_bounce`; Sphere.fs:150-300, InfinitePlane.fs:43-99) is thinnest, a scene that holds every material at the edges of its
parameters, and xorshift128 states whose next draws are chosen values.  Shared by tests/test_reflection_model.py (the oracle
against the line-by-line restatement, and the coverage conditions) and tests/test_gpu_reflection.py (the device against the
oracle: the hook, Scene.traceRays and Scene.renderFootprints through every launch variant).

A vertex is (object index, incoming ray, strike, colour, rng state).  The strike is `o + d * t` with t from the oracle's own
hitObject for that ray, as the kernel produces it; poles are reached exactly by axis-aligned rays at spheres whose centre and
radius make that arithmetic exact.  A candidate whose ray does not meet its object first is dropped, so the incoming ray of every
vertex, traced, has the vertex as its first hit.  Directions are fixed points of Ray.make' (unitised until they no longer
change), so a traced ray is the hook's ray bit for bit.

Out of scope, because the reference divides by zero, converts out of range or throws there: ior <= 0 or non-finite, albedo
outside [0, 1], non-finite geometry.  Bounded spheres of negative radius are in the zoo (their inverted boxes are walked) but no
ray hits them (BoundingBox.hits of an inverted box), so no vertex lies on one.

`probe` restates in numpy the few values of `reflection` that the classes aim at and the coverage conditions count (inside
decision, normal, the haveV2 decision, sinO): every product and sum rounded on its own, as the device and the oracle do.
"""
import functools

import numpy as np

import scenes
from fsharp_literal import pow5

rt = scenes.rt
A = rt._abi
P, S, PS, H, Tex, Px = scenes.P, scenes.S, scenes.PS, scenes.H, scenes.Tex, scenes.Px
TOL = 0.00000001
M32 = 0xFFFFFFFF
GT, EQ, LT = 0, 1, 2

ALBEDO = [0.0, 1.0, 0.5, 1.0 / 3.0, 2.0 ** -60, 1.0 - 2.0 ** -53]
FUZZ = [0.0, 1e-9, 1.0, 1.0 + 2.0 ** -52, 2.0, 10.0, -0.5]
IOR = [1.0, 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -52, 1.5, 1.0 / 1.5, 0.7, 2.4, 0.01, 100.0, 1e9]


# ---- the generator, backwards ------------------------------------------------------------------------------------------------
def _bswap(u):
    u = np.asarray(u, np.uint64)
    return ((u & 0xFF) << 24) | ((u & 0xFF00) << 8) | ((u >> 8) & 0xFF00) | ((u >> 24) & 0xFF)


def attainable(r):
    """The value FloatProducer.Get can return nearest to r: u / 4294967295.0 for an integer u in [0, 2^32)."""
    return attainable_int(r).astype(np.float64) / 4294967295.0


def attainable_int(r):
    return np.clip(np.rint(np.asarray(r, np.float64) * 4294967295.0), 0, M32).astype(np.uint64)


def _un_t(u):
    """x with T(x) = u, T(x) = t ^ (t >> 8), t = x ^ (x << 11) (generateInt32, Float.fs:14-20): both steps are unit-triangular
    over GF(2), (I + S)^-1 = I + S + S^2 + ... with the shift's powers vanishing at 32 bits."""
    t = u ^ (u >> 8) ^ (u >> 16) ^ (u >> 24)
    return (t ^ (t << 11) ^ (t << 22)) & M32


def states_for(r, w=None):
    """[n, 4] uint32 states whose next three Get() are attainable(r[:, 0..2]); w [n]: the free fourth word (non-zero)."""
    u = _bswap(attainable_int(np.asarray(r, np.float64).reshape(-1, 3)))  # the three generateInt32 outputs
    n = len(u)
    w = np.full(n, 0x9E3779B9, np.uint64) if w is None else np.asarray(w, np.uint64) | 1
    o1, o2, o3 = u[:, 0], u[:, 1], u[:, 2]
    x = _un_t(o1 ^ w ^ (w >> 19))  # o1 = w ^ (w >> 19) ^ T(x); then the state is (y, z, w, o1)
    y = _un_t(o2 ^ o1 ^ (o1 >> 19))
    z = _un_t(o3 ^ o2 ^ (o2 >> 19))
    return np.stack([x, y, z, w], axis=1).astype(np.uint32)


def state_for(r1, r2, r3, w=0x9E3779B9):
    return states_for([[r1, r2, r3]], [w])[0]


def step(state):
    """One generateInt32 on [n, 4] uint32 states -> (new states, outputs)."""
    s = state.astype(np.uint64)
    t = (s[:, 0] ^ (s[:, 0] << 11)) & M32
    w = s[:, 3]
    nw = (w ^ (w >> 19) ^ (t ^ (t >> 8))) & M32
    return np.stack([s[:, 1], s[:, 2], w, nw], axis=1).astype(np.uint32), nw


def draws(state_in, state_out, limit=64):
    """How many Get() lead from state_in to state_out, per row (-1: more than `limit`)."""
    cur = np.array(state_in, np.uint32)
    out = np.full(len(cur), -1, np.int64)
    for k in range(limit + 1):
        hit = (out < 0) & (cur == state_out).all(axis=1)
        out[hit] = k
        cur, _ = step(cur)
    return out


def first_draw(state):
    return _bswap(step(np.array(state, np.uint32))[1]).astype(np.float64) / 4294967295.0


PROB = [0.0, 1.0, 0.5, -0.1, 1.1, float(attainable(0.3)), float(attainable(0.7))]


# ---- the zoo -------------------------------------------------------------------------------------------------------------------
GEOMETRIES = [  # (bounded, radius, region: centre near 0 or near 1e3)
    (True, 0.5, 0), (False, 0.5, 0), (False, -0.5, 0), (True, 0.5, 1), (False, -0.5, 1), (True, 1e-3, 0), (False, 1e-3, 1),
    (False, -1e-3, 0), (True, 1e-3, 1), (True, 1000.0, 0), (False, 1000.0, 0), (False, -1000.0, 1), (True, 1000.0, 1), (True, -0.5, 0)]
PLANE_CENTRE, PLANE_DISTANCE = np.array([500.0, 500.0, 500.0]), 4000.0


class Zoo:
    """objs: the Hittables; per object kind (RT_HITTABLE_*), style, c (centre, or the plane's point), r, nrm (planes), albedo,
    fuzz, ior, prob."""

    def __init__(self, objs):
        self.objs = objs
        n = len(objs)
        self.kind, self.style = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.c, self.nrm, self.r = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
        self.albedo, self.fuzz, self.ior, self.prob = np.zeros(n), np.zeros(n), np.ones(n), np.zeros(n)
        for i, h in enumerate(objs):
            self.kind[i] = h.kind
            if h.plane is not None:
                st = h.plane.Style
                self.c[i], self.nrm[i] = h.plane.Point, h.plane.Normal
            else:
                st = h.sphere.Style
                self.c[i], self.r[i] = h.sphere.Centre, h.sphere.Radius
            self.style[i], self.albedo[i], self.fuzz[i], self.ior[i], self.prob[i] = st.style, st.albedo, st.fuzz, st.ior, st.prob
        self.is_plane = self.kind == A.RT_HITTABLE_INFINITE_PLANE

    def spheres(self, *styles, where=None):
        m = ~self.is_plane & np.isin(self.style, styles)
        if where is not None:
            m &= where
        return np.flatnonzero(m)

    def planes(self, *styles, where=None):
        m = self.is_plane & np.isin(self.style, styles)
        if where is not None:
            m &= where
        return np.flatnonzero(m)


def _fibonacci(n):
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    s = np.sqrt(1.0 - z * z)
    return np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1)


@functools.lru_cache(maxsize=None)
def zoo(textured=False):
    """Every sphere style on every geometry, every plane style, parameters cycling through the lists above.  textured: every fifth
    sphere that carries a Texture wears a checkered UV ramp instead of its colour (same geometry, so the same vertices)."""
    rng = np.random.default_rng(2024)
    chk = rt.ParameterisedTexture.Checkered(rt.ParameterisedTexture.UvRamp("u", 40, "v"), rt.ParameterisedTexture.UvRamp(200, "u", "v"), 30.0)
    objs = []

    def col():
        return Px(*(int(x) for x in rng.choice([0, 1, 128, 200, 254, 255], 3)))

    def place(region):
        k = len(objs)
        base = 1000.0 if region else 0.0
        return P(base + 8.0 * (k % 6 - 3), base + 8.0 * ((k // 6) % 6 - 3), base + 8.0 * (k // 36))

    def tex(c, r):
        plain = Tex(col())  # drawn either way: the two zoos differ in nothing else
        if textured and len(objs) % 5 == 0:
            return rt.ParameterisedTexture.toTexture((abs(r), c), chk)
        return plain

    def add(style, geometry, j, ior_shift=0, fuzz=None):
        bounded, r, region = geometry
        c = place(region)
        al, fz = ALBEDO[j % 6], FUZZ[j % 7] if fuzz is None else fuzz
        ior, prob = IOR[(j + ior_shift) % 10], PROB[(3 * j + 1) % 7]
        st = [lambda: S.LightSource(tex(c, r)), lambda: S.LightSourceCap(col()), lambda: S.PureReflection(al, tex(c, r)),
              lambda: S.FuzzedReflection(al, tex(c, r), fz), lambda: S.LambertReflection(al, tex(c, r)),
              lambda: S.Dielectric(al, tex(c, r), ior, prob), lambda: S.Glass(al, tex(c, r), ior)][style]()
        objs.append((H.Sphere if bounded else H.UnboundedSphere)(rt.Sphere.make(st, c, r)))

    j = 0
    for style, rounds in ((0, 1), (1, 1), (2, 1), (3, 1), (4, 1), (5, 2), (6, 2)):
        for rnd in range(rounds):
            for g in GEOMETRIES:
                add(style, g, j, ior_shift=5 * rnd + style)
                j += 1
    for g in ((True, 0.5, 0), (False, -0.5, 0), (False, 0.5, 1), (True, 1000.0, 0)):  # fuzz = 1.0 where a pole is exact
        add(3, g, j, fuzz=1.0)
        j += 1
    # planes: tangent to a sphere around the zoo, so that next to its own tangent point every plane is the nearest; the six
    # axis planes first (exact normals), normals pointing inwards and outwards in turn
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    axis_styles = [PS.LambertReflection(0.5, col()), PS.FuzzedReflection(1.0, col(), 1.0), PS.PureReflection(1.0 / 3.0, col()),
                   PS.LambertReflection(1.0, col()), PS.FuzzedReflection(0.5, col(), 1.0), PS.LightSource(Tex(col()))]
    for m, st in zip(axes, axis_styles):
        objs.append(H.InfinitePlane(rt.InfinitePlane.make(st, P(*(PLANE_CENTRE + PLANE_DISTANCE * m)), scenes.V(*m))))
    for k, m in enumerate(_fibonacci(20)):
        if np.max(np.abs(axes @ m)) > np.cos(np.radians(18.0)):
            continue  # too close to an axis plane's tangent point
        al, fz = ALBEDO[k % 6], FUZZ[k % 7]
        st = [PS.LightSource(Tex(col())), PS.PureReflection(al, col()), PS.LambertReflection(al, col()), PS.FuzzedReflection(al, col(), fz)][k % 4]
        nrm = scenes.unit(*(m if k % 3 else -m))
        objs.append(H.InfinitePlane(rt.InfinitePlane.make(st, P(*(PLANE_CENTRE + PLANE_DISTANCE * m)), nrm)))
    return Zoo(objs)


def witness(kind, cluster=False):
    """The zoo inside something that shows where a ray left it.  "tex": the textured zoo in an UnboundedSphere LightSource with a
    64 x 128 image of random texels (the TEX kernels); "planes": the plain zoo inside six LightSource planes of different colours,
    no parameterised texture anywhere (the non-TEX kernels).  cluster: 1000 small Lambert spheres far off, which take the scene
    out of the LDS.  The zoo's objects come first, so a vertex's object index holds in every witness."""
    rng = np.random.default_rng(77)
    if kind == "tex":
        img = rt.ParameterisedTexture.Image(rng.integers(0, 256, size=(64, 128, 3), dtype=np.uint8))
        centre = P(*PLANE_CENTRE)
        extra = [H.UnboundedSphere(rt.Sphere.make(S.LightSource(rt.ParameterisedTexture.toTexture((30000.0, centre), img)), centre, 30000.0))]
        objs = list(zoo(True).objs)
    else:
        cols = [Px(255, 40, 40), Px(40, 255, 40), Px(40, 40, 255), Px(255, 255, 40), Px(40, 255, 255), Px(255, 40, 255)]
        extra = [H.InfinitePlane(rt.InfinitePlane.make(PS.LightSource(Tex(c)), P(*(PLANE_CENTRE + 20000.0 * m)), scenes.V(*(-m))))
                 for m, c in zip(np.concatenate([np.eye(3), -np.eye(3)]), cols)]
        objs = list(zoo(False).objs)
    if cluster:
        g = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(10), indexing="ij"), -1).reshape(-1, 3)
        for x, y, z in g:
            st = S.LambertReflection(0.5, Tex(Px(*(int(v) for v in rng.integers(0, 256, 3)))))
            extra.append(H.Sphere(rt.Sphere.make(st, P(9000.0 + 10.0 * x, 9000.0 + 10.0 * y, 9000.0 + 10.0 * z), 0.3)))
    return objs + extra


# ---- numpy restatements -------------------------------------------------------------------------------------------------------
def dot3(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def unitise(v):
    """Vector.unitise without its tolerance test (callers pass vectors of length ~1): 1.0 / sqrt(dot) times each component."""
    with np.errstate(all="ignore"):
        f = 1.0 / np.sqrt(dot3(v, v))
    return f[:, None] * v


def settle(d):
    """Towards a fixed point of Ray.make' (a few directions creep by an ulp per round for a long time: _hits drops what is left)."""
    for _ in range(16):
        d = unitise(d)
    return d


def fcmp(a, b):
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(a - b) < TOL, EQ, np.where(a < b, LT, GT))


class Probe:
    pass


def probe(z, idx, rays, strike):
    """What `reflection` decides on before it draws anything, per vertex: cmp (the inside/outside Float.compare), inside, n (the
    normal as used), have_v2, cos_d / cos_g (incomingCos as Dielectric and Glass form it), index, sin_o (both forms), lower/cap (the
    LightSourceCap comparison)."""
    p = Probe()
    o, d = rays[:, :3], rays[:, 3:]
    c, r, plane = z.c[idx], z.r[idx], z.is_plane[idx]
    with np.errstate(all="ignore"):
        co = c - o
        p.cmp = fcmp(dot3(co, co), r * r)
        flipped = ~(np.abs(r - 0.0) < TOL) & (r < 0.0)
        p.inside = ((p.cmp != GT) != flipped) & ~plane
        n = unitise(strike - c)
        n = np.where(p.inside[:, None], -1.0 * n, n)
        p.n = np.where(plane[:, None], z.nrm[idx], n)
        coefficient = dot3(p.n, d)
        w = d - coefficient[:, None] * p.n
        p.have_v2 = ~(np.abs(dot3(w, w) - 0.0) < TOL)
        p.cos_d, p.cos_g = dot3(d, p.n), dot3(-1.0 * d, p.n)
        p.index = np.where(p.inside, 1.0 / z.ior[idx], z.ior[idx])
        p.sin_o_d = np.sqrt(1.0 - p.cos_d * p.cos_d) / p.index
        p.sin_o_g = np.sqrt(1.0 - p.cos_g * p.cos_g) / p.index
        p.sin_o = np.where(z.style[idx] == A.RT_SPHERE_GLASS, p.sin_o_g, p.sin_o_d)
        p.lower = c[:, 0] + (r - (r / 4.0))
        p.cap = fcmp(strike[:, 0], p.lower)
    return p


def glass_reflection_prob(z, idx, pr, other_side=False):
    """Sphere.fs:283-289 with the restatement's own pow5 (exact fifth power, rounded once), per vertex.  other_side: with Schlick's
    term of the other side of the surface (sr = ior inside, 1 / ior outside) -- the same real number, a few ulp away as rounded."""
    out = np.zeros(len(idx))
    for k, (i, inside, cos) in enumerate(zip(idx, pr.inside, pr.cos_g)):
        sr = 1.0 / z.ior[i] if bool(inside) != other_side else z.ior[i]
        param = (1.0 - sr) / (1.0 + sr)
        param = param * param
        out[k] = param + (1.0 - param) * pow5(1.0 - float(cos))
    return out


# ---- vertices -------------------------------------------------------------------------------------------------------------------
class Vertices:
    def __init__(self, name, idx, rays, strike, colour, state, tag):
        self.name, self.idx, self.rays, self.strike, self.colour, self.state, self.tag = name, idx, rays, strike, colour, state, tag

    def __len__(self):
        return len(self.idx)

    def take(self, sel):
        return Vertices(self.name, self.idx[sel], self.rays[sel], self.strike[sel], self.colour[sel], self.state[sel], self.tag[sel])

    def spread(self, k):
        """k vertices spread evenly over the class (all of it if it has no more)."""
        return self if len(self) <= k else self.take(np.linspace(0, len(self) - 1, k).astype(np.int64))


def concat(vs, name="all"):
    return Vertices(name, *(np.concatenate([getattr(v, f) for v in vs]) for f in ("idx", "rays", "strike", "colour", "state", "tag")))


def _tangent(rng, u):
    t = np.cross(u, rng.normal(size=u.shape))
    bad = np.linalg.norm(t, axis=1) < 1e-3
    t[bad] = np.cross(u[bad], np.roll(u[bad], 1, axis=1) + 0.5)
    return t / np.linalg.norm(t, axis=1, keepdims=True)


def _poles(rng, n):
    """(u, tau): axis poles and an axis tangent, exact."""
    k = rng.integers(0, 3, n)
    u = np.eye(3)[k] * rng.choice([-1.0, 1.0], (n, 1))
    return u, np.eye(3)[(k + 1) % 3] * rng.choice([-1.0, 1.0], (n, 1))


def _random_units(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _sphere_rays(z, rng, idx, u, tau, a, b, lfrac=None):
    """Rays that arrive at c + |r| u with direction a u + b tau (a = d.u < 0: from outside, > 0: from inside), from a point a
    fraction of min(|r|, 0.2) before the surface (outside) or of the chord (inside)."""
    n = len(idx)
    c, r = z.c[idx], np.abs(z.r[idx])
    d = settle(a[:, None] * u + b[:, None] * tau)
    lfrac = rng.uniform(0.2, 0.8, n) if lfrac is None else lfrac
    length = np.where(a > 0.0, 2.0 * r * a, np.minimum(r, 0.2)) * lfrac
    p = c + r[:, None] * u
    return np.concatenate([p - d * length[:, None], d], axis=1)


def _plane_rays(z, rng, idx, a, b, length):
    """Rays that arrive near the plane's point (within 20) with d.n = a."""
    n = len(idx)
    nrm = z.nrm[idx]
    tau, e2 = _tangent(rng, nrm), _tangent(rng, nrm)
    p = z.c[idx] + rng.uniform(-20.0, 20.0, (n, 1)) * tau + rng.uniform(-20.0, 20.0, (n, 1)) * e2
    d = settle(a[:, None] * nrm + b[:, None] * _tangent(rng, nrm))
    return np.concatenate([p - d * length[:, None], d], axis=1)


def _random_states(rng, n):
    return rng.integers(1, 2 ** 32, size=(n, 4), dtype=np.uint32)


def _colours(rng, n):
    c = rng.integers(0, 256, size=(n, 3), dtype=np.uint8)
    c[rng.random(n) < 0.2] = 255  # a path's first vertex arrives White
    return c


def _hits(osc, idx, rays):
    """(keep, strike): the ray meets its object first and is what Ray.make' makes of it."""
    hit, strike, _ = osc.hit_object(rays)
    return (hit == idx) & (unitise(rays[:, 3:]) == rays[:, 3:]).all(axis=1), strike


def _finish(name, osc, rng, idx, rays, state=None, tag=None, keep=None, strike=None):
    n = len(idx)
    if keep is None:
        keep, strike = _hits(osc, idx, rays)
    state = _random_states(rng, n) if state is None else state
    tag = np.zeros(n, np.int32) if tag is None else np.asarray(tag, np.int32)
    v = Vertices(name, np.asarray(idx, np.int32), rays, strike, _colours(rng, n), state, tag)
    return v.take(np.flatnonzero(keep))


def _log10u(rng, lo, hi, n):
    return 10.0 ** rng.uniform(lo, hi, n)


MIRRORS = (A.RT_SPHERE_PURE_REFLECTION, A.RT_SPHERE_FUZZED_REFLECTION, A.RT_SPHERE_DIELECTRIC, A.RT_SPHERE_GLASS)
ALL_SPHERE_STYLES = tuple(range(7))


def _edge_first_draws(rng, n):
    """First draws for Dielectric / Glass vertices of the geometric classes: 0.0, 1.0 or anything."""
    st = _random_states(rng, n)
    pick = rng.integers(0, 3, n)
    r = np.where(pick == 0, 0.0, 1.0)
    fixed = states_for(np.stack([r, rng.random(n), rng.random(n)], axis=1), rng.integers(1, 2 ** 32, n))
    return np.where((pick < 2)[:, None], fixed, st)


def class_normal(z, osc, n, seed):
    """d = -+n exactly at the six poles and tilted by 10^U(-12, -3), from outside and from inside: the haveV2 decision
    (|d - (d.n) n|^2 against 1e-8 -- a tilt of 1e-4) is crossed.  tag: 0 exact pole, 1 tilted pole, 2 tilted anywhere."""
    rng = np.random.default_rng(seed)
    idx = rng.choice(np.concatenate([z.spheres(*MIRRORS)] * 3 + [z.spheres(*ALL_SPHERE_STYLES)]), n)
    tag = rng.integers(0, 3, n)
    u, tau = _poles(rng, n)
    ru = _random_units(rng, n)
    u = np.where((tag == 2)[:, None], ru, u)
    tau = np.where((tag == 2)[:, None], _tangent(rng, ru), tau)
    eps = np.where(tag == 0, 0.0, _log10u(rng, -12, -3, n))
    side = rng.choice([-1.0, 1.0], n)
    rays = _sphere_rays(z, rng, idx, u, tau, side * np.cos(eps), np.sin(eps), lfrac=np.full(n, 0.5))
    return _finish("normal", osc, rng, idx, rays, state=_edge_first_draws(rng, n), tag=tag)


def class_grazing(z, osc, n, seed):
    """cosI = +-10^U(-12, -2), and exactly 0 at a pole (tag 1)."""
    rng = np.random.default_rng(seed)
    idx = rng.choice(np.concatenate([z.spheres(*MIRRORS)] * 2 + [z.spheres(*ALL_SPHERE_STYLES)]), n)
    tag = (rng.random(n) < 0.15).astype(np.int32)
    u, tau = _poles(rng, n)
    ru = _random_units(rng, n)
    u = np.where((tag == 0)[:, None], ru, u)
    tau = np.where((tag == 0)[:, None], _tangent(rng, ru), tau)
    a = np.where(tag == 1, 0.0, _log10u(rng, -12, -2, n) * rng.choice([-1.0, 1.0], n, p=[0.7, 0.3]))
    rays = _sphere_rays(z, rng, idx, u, tau, a, np.sqrt(1.0 - a * a))
    return _finish("grazing", osc, rng, idx, rays, state=_edge_first_draws(rng, n), tag=tag)


def class_tir(z, osc, n, seed):
    """Refraction towards the thinner side (inside hits of ior > 1, outside hits of ior < 1) with sinI / index at 1 +- k ulp, k <= 4
    (tag = k, the best of 24 tries each, measured on the settled ray and the oracle's strike) and at 1 +- 10^U(-12, -6) (tag 9).
    For sinO in (1, 1 + 1e-8] Float.compare says Equal and the outgoing ray is NaN.  First draw 0.0 (Dielectric refracts unless
    prob < 0) or 1.0 (Glass refracts)."""
    rng = np.random.default_rng(seed)
    tries = 24
    ok = np.abs(z.ior - 1.0) > 1e-3
    idx = rng.choice(z.spheres(A.RT_SPHERE_DIELECTRIC, A.RT_SPHERE_GLASS, where=ok & ~((z.kind == A.RT_HITTABLE_SPHERE) & (z.r < 0))), n)
    flipped = z.r[idx] < 0.0
    logical_inside = z.ior[idx] > 1.0
    geometric_inside = logical_inside != flipped
    index = np.where(logical_inside, 1.0 / z.ior[idx], z.ior[idx])
    tag = np.where(rng.random(n) < 0.4, rng.integers(0, 5, n), 9)
    sign = rng.choice([-1.0, 1.0], n)
    delta = np.where(tag == 9, sign * _log10u(rng, -12, -6, n), sign * tag * 2.0 ** -52)
    # candidates: the k-ulp vertices 24 times each with the target moved by up to 6 ulp, everything else once
    rep = np.where(tag == 9, 1, tries)
    src = np.repeat(np.arange(n), rep)
    jitter = np.where(tag[src] == 9, 0.0, rng.uniform(-6.0, 6.0, len(src)) * 2.0 ** -52)
    sin_i = index[src] * (1.0 + delta[src] + jitter)
    u = _random_units(rng, n)[src]
    tau = _tangent(rng, u)
    a = np.where(geometric_inside[src], 1.0, -1.0) * np.sqrt(1.0 - sin_i * sin_i)
    rays = _sphere_rays(z, rng, idx[src], u, tau, a, sin_i, lfrac=np.full(len(src), 0.5))
    keep, strike = _hits(osc, idx[src], rays)
    got = probe(z, idx[src], rays, strike).sin_o
    miss = np.where(keep & np.isfinite(got), np.abs(got - (1.0 + delta[src])), np.inf)
    best = np.zeros(n, np.int64)
    start = np.concatenate([[0], np.cumsum(rep)[:-1]])
    for i in range(n):
        best[i] = start[i] + int(np.argmin(miss[start[i]:start[i] + rep[i]]))
    first = np.where(z.style[idx] == A.RT_SPHERE_GLASS, 1.0, 0.0)
    state = states_for(np.stack([first, rng.random(n), rng.random(n)], axis=1), rng.integers(1, 2 ** 32, n))
    return _finish("tir", osc, rng, idx, rays[best], state=state, tag=tag, keep=keep[best], strike=strike[best])


SURFACE_DELTAS = [0.0, 5e-9, -5e-9, 2e-8, -2e-8, 1e-6, -1e-6]


def class_surface_origin(z, osc, n, seed):
    """The ray starts on the surface, as every second vertex of a path through glass does: |c - o|^2 - r^2 in {0, +-k ulp(r^2),
    +-5e-9, +-2e-8, +-1e-6} as nearly as an origin near that centre can give it, both radius signs, aimed across the sphere.
    tag: index into SURFACE_DELTAS, or 10 + k for the ulp targets."""
    rng = np.random.default_rng(seed)
    idx = rng.choice(z.spheres(*ALL_SPHERE_STYLES), n)
    c, r = z.c[idx], np.abs(z.r[idx])
    r2 = z.r[idx] * z.r[idx]
    k = rng.integers(-4, 5, n)
    tag = np.where(rng.random(n) < 0.3, 10 + np.abs(k), rng.integers(0, len(SURFACE_DELTAS), n))
    delta = np.where(tag >= 10, k * np.spacing(r2), np.array(SURFACE_DELTAS)[np.minimum(tag, len(SURFACE_DELTAS) - 1)])
    u = _random_units(rng, n)
    pole = rng.random(n) < 0.3
    u[pole] = _poles(rng, int(pole.sum()))[0]

    def err(rho):
        co = c - (c + rho[:, None] * u)
        return (dot3(co, co) - r2) - delta

    rho = np.sqrt(np.maximum(r2 + delta, 0.0))
    for _ in range(3):
        rho = np.where(rho > 0.0, rho - err(rho) / np.where(rho > 0.0, 2.0 * rho, 1.0), 0.0)
    best, best_err = rho.copy(), np.abs(err(rho))
    for s in range(-3, 4):
        cand = rho + s * np.spacing(rho)
        e = np.abs(err(cand))
        better = e < best_err
        best, best_err = np.where(better, cand, best), np.where(better, e, best_err)
    o = c + best[:, None] * u
    a = -rng.uniform(0.2, 1.0, n) * np.where(r > 1.0, 0.2 / (2.0 * r), 1.0)  # across the sphere, a chord of at most 0.2 through a huge one
    a[pole & (rng.random(n) < 0.5) & (r <= 1.0)] = -1.0
    d = settle(a[:, None] * u + np.sqrt(1.0 - a * a)[:, None] * _tangent(rng, u))
    return _finish("surface_origin", osc, rng, idx, np.concatenate([o, d], axis=1), state=_edge_first_draws(rng, n), tag=tag)


CAP_DELTAS = [5e-9, -5e-9, 2e-8, -2e-8]


def class_cap_band(z, osc, n, seed):
    """LightSourceCap: strike.x - lower in {0, +-k ulp, +-5e-9, +-2e-8}, lower = c.x + (r - r / 4), both radius signs.  The ray
    runs in the plane x = lower + delta (d.x = 0), so the strike's x is the origin's, exactly.  tag: 10 + k (ulps, k = 0..4) or
    the index into CAP_DELTAS."""
    rng = np.random.default_rng(seed)
    idx = rng.choice(z.spheres(A.RT_SPHERE_LIGHT_SOURCE_CAP), n)
    c, r = z.c[idx], z.r[idx]
    lower = c[:, 0] + (r - (r / 4.0))
    k = rng.integers(-4, 5, n)
    tag = np.where(rng.random(n) < 0.45, 10 + np.abs(k), rng.integers(0, len(CAP_DELTAS), n))
    x0 = lower + np.array(CAP_DELTAS)[np.minimum(tag, len(CAP_DELTAS) - 1)]
    ulps = lower.copy()
    for s in range(1, 5):
        ulps = np.where(np.abs(k) >= s, np.nextafter(ulps, np.where(k > 0, np.inf, -np.inf)), ulps)
    x0 = np.where(tag >= 10, ulps, x0)
    circle = np.sqrt(np.maximum(r * r - (x0 - c[:, 0]) ** 2, 0.0))
    phi = np.where(rng.random(n) < 0.3, rng.integers(0, 4, n) * (np.pi / 2), rng.uniform(0, 2 * np.pi, n))
    w = np.stack([np.zeros(n), np.rint(np.cos(phi) * 1e15) / 1e15, np.rint(np.sin(phi) * 1e15) / 1e15], axis=1)
    inside = rng.random(n) < 0.5
    length = rng.uniform(0.1, 0.5, n) * np.minimum(np.abs(r), 0.2)
    dist = np.where(inside, circle - np.minimum(length, circle), circle + length)
    o = np.stack([x0, c[:, 1] + w[:, 1] * dist, c[:, 2] + w[:, 2] * dist], axis=1)
    d = settle(np.where(inside[:, None], w, -w))
    return _finish("cap_band", osc, rng, idx, np.concatenate([o, d], axis=1), tag=tag)


def class_plane(z, osc, n, seed):
    """Planes: exact normal incidence (tag 0: d = -+n), tilted by 10^U(-12, -3) (1), anything from the front or the back (2), and
    |d.n| = 10^U(-7, -1) (3).  d.n > 0 is a hit from the back."""
    rng = np.random.default_rng(seed)
    idx = rng.choice(z.planes(0, 1, 2, 3), n)
    tag = rng.integers(0, 4, n)
    side = rng.choice([-1.0, 1.0], n)
    eps = _log10u(rng, -12, -3, n)
    graze = _log10u(rng, -7, -1, n)
    anyc = rng.uniform(0.05, 1.0, n)
    a = side * np.select([tag == 0, tag == 1, tag == 2], [np.ones(n), np.cos(eps), anyc], graze)
    b = np.select([tag == 0, tag == 1], [np.zeros(n), np.sin(eps)], np.sqrt(1.0 - a * a))
    rays = _plane_rays(z, rng, idx, a, b, rng.uniform(0.05, 2.0, n))
    return _finish("plane", osc, rng, idx, rays, tag=tag)


def class_rng_edges(z, osc, n, seed):
    """Dielectric with the first draw r in {0.0, 1.0, prob, its attainable neighbours} (tag 0..4: 0.0, 1.0, at, below, above; at a
    prob that no draw attains, the nearest), Glass with r at reflectionProb's two attainable neighbours (tag 5 below-or-at, 6
    above), reflectionProb formed with the restatement's pow5 from the settled ray and the oracle's strike."""
    rng = np.random.default_rng(seed)
    idx = np.concatenate([rng.choice(z.spheres(A.RT_SPHERE_DIELECTRIC), n - n // 3), rng.choice(z.spheres(A.RT_SPHERE_GLASS), n // 3)])
    u = _random_units(rng, n)
    a = rng.uniform(0.2, 1.0, n) * rng.choice([-1.0, 1.0], n)
    rays = _sphere_rays(z, rng, idx, u, _tangent(rng, u), a, np.sqrt(1.0 - a * a))
    keep, strike = _hits(osc, idx, rays)
    sel = np.flatnonzero(keep)
    idx, rays, strike = idx[sel], rays[sel], strike[sel]
    m = len(idx)
    glass = z.style[idx] == A.RT_SPHERE_GLASS
    tag = np.where(glass, rng.integers(5, 7, m), rng.integers(0, 5, m))
    pr = probe(z, idx, rays, strike)
    thr = z.prob[idx].copy()
    thr[glass] = glass_reflection_prob(z, idx[glass], _take_probe(pr, glass))
    at = attainable_int(thr).astype(np.int64)
    lo = np.where(at.astype(np.float64) / 4294967295.0 <= thr, at, at - 1)  # the largest attainable value <= thr (or 0)
    lo = np.clip(lo, 0, M32)
    ui = np.select([tag == 0, tag == 1, tag == 2, tag == 3, tag == 4, tag == 5], [0, M32, at, np.clip(at - 1, 0, M32), np.clip(at + 1, 0, M32), lo],
                   np.clip(lo + 1, 0, M32))
    r1 = ui.astype(np.float64) / 4294967295.0
    state = states_for(np.stack([r1, rng.random(m), rng.random(m)], axis=1), rng.integers(1, 2 ** 32, m))
    return _finish("rng_edges", osc, rng, idx, rays, state=state, tag=tag, keep=np.ones(m, bool), strike=strike)


def schlick_terms(ior):
    """(outside, inside): ((1 - sr) / (1 + sr))^2 for sr = ior and sr = 1 / ior, as the host forms them once per material."""
    inv = 1.0 / ior
    po, pi = (1.0 - ior) / (1.0 + ior), (1.0 - inv) / (1.0 + inv)
    return po * po, pi * pi


def class_schlick(z, osc, n, seed):
    """Glass, with an attainable first draw BETWEEN reflectionProb as formed with Schlick's term of the vertex's own side and as
    formed with the other side's: the two terms are the same real number and differ by a few ulp as rounded, so only a draw inside
    that gap tells them apart.  cosI is aimed at the value where reflectionProb meets a draw, 48 tries each a few ulp apart, and a
    vertex is kept where the two decisions differ (measured on the settled ray and the oracle's strike, with the restatement's
    pow5).  Spheres of positive radius whose two terms differ; from outside and from inside.  tag: 1 if the draw reflects with
    the right term and refracts with the other, 0 the other way round."""
    rng = np.random.default_rng(seed)
    tries = 48
    differ = np.array([len(set(schlick_terms(i))) == 2 for i in z.ior])
    idx = rng.choice(z.spheres(A.RT_SPHERE_GLASS, where=differ & (z.r > 0.0) & (z.ior < 1e6)), n)
    inside = rng.random(n) < 0.6
    term = np.array([schlick_terms(z.ior[i])[int(s)] for i, s in zip(idx, inside)])
    cos0 = rng.uniform(0.15, 0.9, n)
    y = 1.0 - cos0
    u_draw = attainable_int(term + (1.0 - term) * (y * y * y * y * y))
    r1 = u_draw.astype(np.float64) / 4294967295.0
    x = (r1 - term) / (1.0 - term)
    for _ in range(4):  # the fifth root of x by Newton's rule from 1 - cos0, which is within 1e-6 of it (the draws are 2.3e-10 apart):
        y = y - (y * y * y * y * y - x) / (5.0 * (y * y * y * y))  # + - * / only, so the class is the same on every host
    cos = 1.0 - y  # where reflectionProb = r1, to a few ulp
    src = np.repeat(np.arange(n), tries)
    cos_try = cos[src] + rng.integers(-8, 9, len(src)) * 2.0 ** -54
    uu = _random_units(rng, n)[src]
    a = np.where(inside[src], 1.0, -1.0) * cos_try
    with np.errstate(invalid="ignore"):
        rays = _sphere_rays(z, rng, idx[src], uu, _tangent(rng, uu), a, np.sqrt(1.0 - a * a), lfrac=np.full(len(src), 0.5))
    keep, strike = _hits(osc, idx[src], rays)
    pr = probe(z, idx[src], rays, strike)
    keep &= (pr.inside == inside[src]) & np.isfinite(pr.cos_g)
    own, other = np.full(len(src), np.nan), np.full(len(src), np.nan)
    own[keep] = glass_reflection_prob(z, idx[src][keep], _take_probe(pr, keep))
    other[keep] = glass_reflection_prob(z, idx[src][keep], _take_probe(pr, keep), other_side=True)
    told_apart = keep & ((r1[src] < own) != (r1[src] < other))
    first = np.full(n, -1, np.int64)
    for j in np.flatnonzero(told_apart)[::-1]:
        first[src[j]] = j
    sel = first[first >= 0]
    m = len(sel)
    state = states_for(np.stack([r1[src][sel], rng.random(m), rng.random(m)], axis=1), rng.integers(1, 2 ** 32, m))
    tag = (r1[src][sel] < own[sel]).astype(np.int32)
    return _finish("schlick", osc, rng, idx[src][sel], rays[sel], state=state, tag=tag, keep=np.ones(m, bool), strike=strike[sel])


def _take_probe(pr, sel):
    q = Probe()
    for k, v in vars(pr).items():
        setattr(q, k, v[sel])
    return q


ABOVE_HALF = 2147483648.0 / 4294967295.0  # the attainable value just above 0.5: 2 r - 1 = 2.3e-10


def _against(v):
    """The first triple whose unit vector is -v to within 1e-9, v = +-e_k: r = 0.0 (v_k > 0) or 1.0 on that axis, just above 0.5
    on the others."""
    k = np.argmax(np.abs(v), axis=1)
    r = np.full((len(v), 3), ABOVE_HALF)
    r[np.arange(len(v)), k] = np.where(v[np.arange(len(v)), k] > 0.0, 0.0, 1.0)
    return r


def class_retries(z, osc, n, seed):
    """The retry loops, reached on purpose.  tag 0: a first triple with every |2 r - 1| < 5e-5 (random_unit retries) on every
    style that draws a unit vector.  tag 1: a first triple that makes offset = -n at an axis pole: a sphere Lambert draws again, a
    plane Lambert ends Black.  tag 2: the same against fuzz = 1.0 with the mirrored ray = n (normal incidence at a pole): the
    fuzz loop draws again, on spheres and planes."""
    rng = np.random.default_rng(seed)
    third = n // 3
    lam, fuz = A.RT_SPHERE_LAMBERT_REFLECTION, A.RT_SPHERE_FUZZED_REFLECTION
    # tag 0
    n_s = third // 2
    idx = rng.choice(z.spheres(lam, fuz), n_s)
    u = _random_units(rng, n_s)
    a = rng.uniform(0.1, 1.0, n_s) * rng.choice([-1.0, 1.0], n_s)
    rays0 = _sphere_rays(z, rng, idx, u, _tangent(rng, u), a, np.sqrt(1.0 - a * a))
    pidx = rng.choice(z.planes(A.RT_PLANE_LAMBERT_REFLECTION, A.RT_PLANE_FUZZED_REFLECTION), third - n_s)
    a = rng.uniform(0.1, 1.0, third - n_s) * rng.choice([-1.0, 1.0], third - n_s)
    rays0 = np.concatenate([rays0, _plane_rays(z, rng, pidx, a, np.sqrt(1.0 - a * a), rng.uniform(0.05, 2.0, third - n_s))])
    idx0 = np.concatenate([idx, pidx])
    state0 = states_for(0.5 + rng.uniform(-2.4e-5, 2.4e-5, (third, 3)), rng.integers(1, 2 ** 32, third))
    # tags 1 and 2: axis-aligned rays at poles of spheres, and at axis planes
    parts = []
    axis_plane = np.max(np.abs(z.nrm), axis=1) == 1.0
    fuzz_one = z.fuzz == 1.0
    for tag, sph, pln in ((1, z.spheres(lam), z.planes(A.RT_PLANE_LAMBERT_REFLECTION, where=axis_plane)),
                          (2, z.spheres(fuz, where=fuzz_one), z.planes(A.RT_PLANE_FUZZED_REFLECTION, where=axis_plane & fuzz_one))):
        n_s = third // 2
        idx = rng.choice(sph, n_s)
        u, tau = _poles(rng, n_s)
        side = rng.choice([-1.0, 1.0], n_s)
        rays = _sphere_rays(z, rng, idx, u, tau, side, np.zeros(n_s), lfrac=np.full(n_s, 0.5))
        pidx = rng.choice(pln, third - n_s)
        side = rng.choice([-1.0, 1.0], third - n_s)
        prays = _plane_rays(z, rng, pidx, side, np.zeros(third - n_s), rng.choice([0.25, 0.5, 1.0, 2.0], third - n_s))
        idx, rays = np.concatenate([idx, pidx]), np.concatenate([rays, prays])
        keep, strike = _hits(osc, idx, rays)
        against = probe(z, idx, rays, strike).n if tag == 1 else -rays[:, 3:]
        against = np.where(np.isfinite(against), against, 1.0)
        state = states_for(_against(against), rng.integers(1, 2 ** 32, len(idx)))
        parts.append(_finish("retries", osc, rng, idx, rays, state=state, tag=np.full(len(idx), tag), keep=keep, strike=strike))
    return concat([_finish("retries", osc, rng, idx0, rays0, state=state0, tag=np.zeros(third))] + parts, "retries")


def class_ordinary(z, osc, n, seed):
    """Random vertices over the whole zoo, from both sides: the control."""
    rng = np.random.default_rng(seed)
    sph, pln = z.spheres(*ALL_SPHERE_STYLES), z.planes(0, 1, 2, 3)
    n_s = n * 3 // 4
    idx = rng.choice(sph, n_s)
    u = _random_units(rng, n_s)
    a = rng.uniform(0.01, 1.0, n_s) * rng.choice([-1.0, 1.0], n_s)
    rays = _sphere_rays(z, rng, idx, u, _tangent(rng, u), a, np.sqrt(1.0 - a * a))
    pidx = rng.choice(pln, n - n_s)
    a = rng.uniform(0.01, 1.0, n - n_s) * rng.choice([-1.0, 1.0], n - n_s)
    prays = _plane_rays(z, rng, pidx, a, np.sqrt(1.0 - a * a), rng.uniform(0.05, 2.0, n - n_s))
    return _finish("ordinary", osc, rng, np.concatenate([idx, pidx]), np.concatenate([rays, prays]))


CLASSES = [("normal", class_normal), ("grazing", class_grazing), ("tir", class_tir), ("surface_origin", class_surface_origin),
           ("cap_band", class_cap_band), ("plane", class_plane), ("rng_edges", class_rng_edges), ("retries", class_retries),
           ("ordinary", class_ordinary), ("schlick", class_schlick)]
# the classes in which some outgoing rays are NaN: tir by construction; grazing and ordinary through ior = 1 -+ 2^-52, where sinI = 1
# (a hit of a 1e-3 sphere through the Equal arm of its discriminant is as good as tangent) gives sinO = 1 + 2^-52
NAN_CLASSES = ("tir", "grazing", "ordinary")
CANDIDATES = {"schlick": 3000}     # each tried 48 times: the gap between the two terms is a few ulp wide
LEAST = {"schlick": 400}           # vertices a class must keep (default 1500)
PER_CLASS = 3000                   # candidates; about 2000 of them meet their object first


@functools.lru_cache(maxsize=None)
def oracle_zoo(orc):
    return orc.OracleScene(zoo().objs)


@functools.lru_cache(maxsize=None)
def vertices(orc, name):
    fn = dict(CLASSES)[name]
    return fn(zoo(), oracle_zoo(orc), CANDIDATES.get(name, PER_CLASS), 1000 + [c for c, _ in CLASSES].index(name))
