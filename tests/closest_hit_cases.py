"""Scenes and rays whose closest hit is known by construction, aimed at the seam between Scene.hitObject's two rules (Scene.fs:62-91):
a Leaf replaces the best hit when `a < bestFloat` (strict, a = t * t), an UnboundedObject -- taken in array order, after the tree --
only when `Float.compare a bestFloat = Less`, that is a < bestFloat AND |a - bestFloat| >= 1e-8.  And the rays on which the two
guards of InfinitePlane.intersection (InfinitePlane.fs:125-136) decide the result.

Shared by tests/test_closest_hit_cases.py (no GPU: the numpy model of the rule and its mutants, the oracle against the model and the
literal restatement, the coverage conditions) and tests/test_gpu_closest_hit.py (the device against the oracle, bit for bit).

Stations.  Rays run along the six half-axes (axis a, sign s) from dyadic origins with unit axis vectors, so Ray.make' is the
identity and every t below is exact or known to an ulp.  Half-axis g has its own dyadic T in {1, 2, 4, 8, 16, 32}; its stations lie on
a lattice spaced 4 apart, at b = 128 (g + 1) + 4 i, c = -128 (g + 1) - 4 j in the two other axes (b, c) = (a + 1, a + 2) mod 3, which
keeps every sphere of one half-axis out of reach of the rays of the others, and every coordinate inside +-1000 (the timed kernel's
box_implied scenes).  A station's `earlier` object is hit at t = T, its `later` one -- later in Scene.hitObject's order: a Leaf comes
before every UnboundedObject, and those come in array order -- at t_l with t_l^2 - T^2 = delta:

  tie             delta = 0 exactly                                   the earlier one is kept
  inside_nearer   delta = -0.8e-8                                     the earlier one, although the later one is nearer
  outside_nearer  delta = -1.2e-8                                     the later one
  inside_farther  delta = +0.8e-8                                     the earlier one
  tiny            t = 2^-14 (1 + g / 8) < 1e-4, later one at t / 4    the earlier one: any two such hits are "Equal"
  far_tie         T = 2^14, equal t                                   the earlier one
  far_ulp         T = 2^14, later t the next double below             the later one: ulp(t^2) > 1e-8, the band is exact equality
  at_infinity     the only objects hit are at t = 1e160 / t = +inf    none (-1): a = +inf is never Less than bestFloat = +inf

A plane faces its half-axis' rays (one per half-axis; the planes of the other axes are parallel to these rays and answer None, those
of the opposite half-axis lie behind the origin); an unbounded sphere is one per station, its near pole where the plane would be.
Pairs (earlier, later): (leaf, plane), (leaf, usphere), (plane, plane), (plane, usphere), (usphere, plane), and (leaf, leaf) -- two
bounded spheres whose poles differ by the inside_nearer delta, where the strict rule makes the NEARER one win: the contrast.
Every object is a LightSource with a colour of its own, so Scene.traceRays at depth 0 names the winner."""
import dataclasses
import functools

import numpy as np

import fsharp_literal as L
import scenes

rt = scenes.rt
A = rt._abi
P, V, S, PS, H, Tex, Px = scenes.P, scenes.V, scenes.S, scenes.PS, scenes.H, scenes.Tex, scenes.Px
TOL = 0.00000001
INF = np.inf

HALF_AXES = ((0, 1.0), (0, -1.0), (1, 1.0), (1, -1.0), (2, 1.0), (2, -1.0))
T_OF = (1.0, 2.0, 4.0, 8.0, 16.0, 32.0)
T_FAR = 16384.0
N_STATIONS = 14
DELTA = {"tie": 0.0, "inside_nearer": -0.8e-8, "outside_nearer": -1.2e-8, "inside_farther": 0.8e-8}
BAND = tuple(DELTA)
CLASSES = BAND + ("tiny", "far_tie", "far_ulp")          # the classes that have pairs; at_infinity has scenes of its own
PAIRS = ("leaf_plane", "leaf_usphere", "plane_plane", "plane_usphere", "usphere_plane")
PAIRS_UU = PAIRS[2:]                                     # both members in the unbounded list
EXPECT = {"tie": "earlier", "inside_nearer": "earlier", "outside_nearer": "later", "inside_farther": "earlier", "tiny": "earlier",
          "far_tie": "earlier", "far_ulp": "later"}
SHAPE = {"tie": "grouped", "inside_nearer": "grouped", "outside_nearer": "split", "inside_farther": "split", "tiny": "grouped",
         "far_tie": "split", "far_ulp": "grouped"}       # how a class' scenes order their unbounded list
HUGE = 1e160


def colour_of(k):
    """Object k's own colour (no channel 0, so a product with White keeps it)."""
    return (1 + k % 251, 1 + (k // 251) % 251, 7)


def _light(k, plane=False):
    return (PS if plane else S).LightSource(Tex(Px(*colour_of(k))))


# ---- geometry ---------------------------------------------------------------------------------------------------------------------
def _at(g, i, j, along):
    """The point of half-axis g's station (i, j) at signed distance `along` from the origin level."""
    a, s = HALF_AXES[g]
    p = [0.0, 0.0, 0.0]
    p[a] = s * along
    p[(a + 1) % 3] = 128.0 * (g + 1) + 4.0 * i
    p[(a + 2) % 3] = -128.0 * (g + 1) - 4.0 * j
    return p


def station_ray(g, i, j=0, back=0.0):
    a, s = HALF_AXES[g]
    d = [0.0, 0.0, 0.0]
    d[a] = s
    return _at(g, i, j, -back) + d


def times_of(cls, g):
    """(t of the earlier object, t of the later one) on half-axis g."""
    if cls in DELTA:
        t = T_OF[g]
        return t, t + DELTA[cls] / (2.0 * t)  # (t + d / 2t)^2 = t^2 + d + d^2 / 4t^2, the last term below 1e-16
    if cls == "tiny":
        t = 2.0 ** -14 * (1.0 + g / 8.0)
        return t, t / 4.0
    if cls == "far_tie":
        return T_FAR, T_FAR
    if cls == "far_ulp":
        return T_FAR, float(np.nextafter(T_FAR, 0.0))
    raise ValueError(cls)


class Builder:
    """Collects a scene: the bounded spheres first, then the unbounded list in the order its shape asks for."""

    def __init__(self):
        self.bounded, self.early, self.late, self.filler = [], [], [], []   # entries: (key, kind, geometry)
        self.rays, self.keys = [], []                                         # keys: (pair, earlier key, later key, expect)
        self.stations = []                                                    # (g, i, j) of each ray

    @staticmethod
    def _centre(t):
        """Distance of a unit sphere's centre whose near pole is at t: t + 1, rounded so that the pole is not beyond t (at T = 2^14
        the next double below T + 1 puts the pole two ulps below T)."""
        c = t + 1.0
        return float(np.nextafter(c, 0.0)) if c - 1.0 > t else c

    def leaf(self, key, g, i, j, t):
        self.bounded.append((key, "leaf", (_at(g, i, j, self._centre(t)), 1.0)))

    def usphere(self, where, key, g, i, j, t):
        where.append((key, "usphere", (_at(g, i, j, self._centre(t)), 1.0)))

    def plane(self, where, key, g, t):
        a, s = HALF_AXES[g]
        p, n = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
        p[a], n[a] = s * t, -s
        where.append((key, "plane", (p, n)))

    def pair(self, pair, cls, g, n_i=N_STATIONS, n_j=1, t_pair=None, expect=None):
        """Half-axis g hosts `pair` at n_i x n_j stations."""
        te, tl = t_pair or times_of(cls, g)
        early, late = [], []
        for i in range(n_i):
            for j in range(n_j):
                ke, kl = (g, i, j, "e"), (g, i, j, "l")
                if pair == "leaf_leaf":  # list order alternates, so that both visit orders of the pair's two Leaves occur
                    for key, t in ((ke, te), (kl, tl)) if (i + j) % 2 == 0 else ((kl, tl), (ke, te)):
                        self.leaf(key, g, i, j, t)
                else:
                    first, second = pair.split("_")
                    if first == "leaf":
                        self.leaf(ke, g, i, j, te)
                    elif first == "usphere":
                        self.usphere(early, ke, g, i, j, te)
                    else:
                        ke = (g, "plane", "e")
                    if second == "usphere":
                        self.usphere(late, kl, g, i, j, tl)
                    else:
                        kl = (g, "plane", "l")
                self.rays.append(station_ray(g, i, j))
                self.stations.append((g, i, j))
                self.keys.append((pair, ke, kl, expect or ("later" if pair == "leaf_leaf" else EXPECT[cls])))
        if pair.startswith("plane_"):
            self.plane(early, (g, "plane", "e"), g, te)
        if pair.endswith("_plane"):
            self.plane(late, (g, "plane", "l"), g, tl)
        self.early.append(early)
        self.late.append(late)

    def finish(self, name, cls, shape, pad=0, extra_rays=None, cls_of=None):
        if shape == "grouped":
            unbounded = [x for e, l in zip(self.early, self.late) for x in e + l] + self.filler
        else:  # split: every earlier object, eight far-away spheres that no ray meets, every later object
            far = [(("far", k), "usphere", ([-700.0 - 8.0 * k, -700.0, -700.0], 1.0)) for k in range(8)]
            unbounded = [x for e in self.early for x in e] + far + self.filler + [x for l in self.late for x in l]
        entries = self.bounded + unbounded
        objs, index = [], {}
        for k, (key, kind, (p, q)) in enumerate(entries):
            index[key] = k
            if kind == "plane":
                objs.append(H.InfinitePlane(rt.InfinitePlane.make(_light(k, True), P(*p), V(*q))))
            else:
                objs.append((H.Sphere if kind == "leaf" else H.UnboundedSphere)(rt.Sphere.make(_light(k), P(*p), q)))
        n_core = len(objs)
        if pad:
            objs += padding(pad)
        rays = np.array(self.rays, np.float64).reshape(-1, 6)
        e_idx = np.array([index[k[1]] for k in self.keys], np.int32)
        l_idx = np.array([index[k[2]] for k in self.keys], np.int32)
        pair = np.array([k[0] for k in self.keys])
        want_later = np.array([k[3] == "later" for k in self.keys], bool)
        out = Built(name, cls, objs, n_core, len(self.bounded), rays, pair, e_idx, l_idx, want_later, extra_rays, cls_of)
        out.index = index
        return out


def padding(n=1300):
    """Far-away bounded spheres that take a scene past the LDS limit (tests/sphere_arm_cases.py's kind): the LDS = false kernels.
    Every coordinate is positive, every ray of this module runs at a negative one: none is ever met."""
    rng = np.random.default_rng(17)
    return [H.Sphere(rt.Sphere.make(S.LambertReflection(0.5, Tex(Px(*(int(x) for x in rng.integers(30, 256, 3))))),
                                    P(*(900.0 + rng.uniform(0, 60, 3))), float(rng.uniform(0.05, 0.3)))) for _ in range(n)]


class Built:
    """A scene and its crafted rays.  rays [n, 6]; pair [n]; earlier / later [n]: the two objects of each ray's station; want [n]:
    the object the class says wins (-1: none).  `kept` marks the candidates whose computed a = t * t land in the class."""

    def __init__(self, name, cls, objs, n_core, n_bounded, rays, pair, earlier, later, want_later, extra_rays=None, cls_of=None):
        self.name, self.cls, self.objs, self.n_core, self.n_bounded = name, cls, objs, n_core, n_bounded
        self.padded = len(objs) > n_core
        core = objs[:n_core]
        self.order = hit_order(core)
        self.candidates = len(rays)
        cls_of = np.full(len(rays), cls) if cls_of is None else np.asarray(cls_of)  # each ray's class
        keep = np.zeros(len(rays), bool)
        for c in sorted(set(cls_of.tolist())):
            m = cls_of == c
            keep[m] = in_class(c, core, rays[m], earlier[m], later[m])
        self.cls_of = cls_of[keep]
        self.rays, self.pair, self.earlier, self.later = rays[keep], pair[keep], earlier[keep], later[keep]
        self.want = np.where(want_later[keep], self.later, self.earlier).astype(np.int32)
        if cls == "at_infinity":
            self.want = np.full(len(self.rays), -1, np.int32)
        self.extra = np.zeros((0, 6)) if extra_rays is None else np.asarray(extra_rays, np.float64)  # rays with no class of their own
        for a in (self.rays, self.pair, self.earlier, self.later, self.want, self.extra):
            a.setflags(write=False)

    def __len__(self):
        return len(self.rays)

    def ts(self, rays=None):
        """[n, n_core] in Scene.hitObject's order (self.order): the t of every object for every ray, NaN for none."""
        return ts_of(self.objs[:self.n_core], self.rays if rays is None else rays)[:, self.order]

    def model(self, rule="reference", rays=None):
        """The model's winner as an object index."""
        w = winner(self.ts(rays), self.n_bounded, rule)
        return np.where(w >= 0, self.order[np.maximum(w, 0)], -1).astype(np.int32)

    def unbounded_position(self, idx):
        """Positions of the objects idx in the unbounded list (-1 for a bounded one)."""
        unb = np.array([h.kind != A.RT_HITTABLE_SPHERE for h in self.objs])
        return np.where(unb[idx], (np.cumsum(unb) - 1)[idx], -1)

    def crafted(self):
        """The rays that the lists scatter among fillers."""
        return self.rays

    @property
    def n_unbounded(self):
        return sum(h.kind != A.RT_HITTABLE_SPHERE for h in self.objs)


# ---- the numpy model ----------------------------------------------------------------------------------------------------------------
def plane_t(rays, planes):
    """InfinitePlane.intersection in the operation order of `plane_intersection` (csrc/rt_device.h): den = n . d, every product and
    sum rounded on its own; None (NaN) when |den - 0| < 1e-8; t = (n . (p - o)) / den; None unless t > 1e-8.  -> (t, den, raw t)."""
    o, d, p, n = rays[:, :3], rays[:, 3:], planes[:, :3], planes[:, 3:]
    with np.errstate(all="ignore"):
        den = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]
        w = p - o
        raw = ((n[:, 0] * w[:, 0] + n[:, 1] * w[:, 1]) + n[:, 2] * w[:, 2]) / den
        none = (np.abs(den - 0.0) < TOL) | ~(raw > TOL)
        return np.where(none, np.nan, raw), den, raw


def sphere_t(rays, sph):
    """Sphere.firstIntersection (Sphere.fs:349-386), arm by arm."""
    o, d, c, r = rays[:, :3], rays[:, 3:], sph[:, :3], sph[:, 3]
    with np.errstate(all="ignore"):
        diff = o - c
        b = (d[:, 0] * diff[:, 0] + d[:, 1] * diff[:, 1]) + d[:, 2] * diff[:, 2]
        cc = ((diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]) - r * r
        disc = b * b - cc
        equal = np.abs(disc - 0.0) < TOL
        less = ~equal & (disc < 0.0)
        s = np.sqrt(disc)
        i1, i2 = s - b, -(b + s)
        p1, p2 = i1 > TOL, i2 > TOL
        both = np.where(~(np.abs(i1 - i2) < TOL) & ~(i1 < i2), i2, i1)  # Float.compare i1 i2 = Greater -> i2
        ip = np.where(p1 & p2, both, np.where(p1, i1, np.where(p2, i2, np.nan)))
        ip = np.where(equal, -b, np.where(less, np.nan, ip))
        return np.where(ip > TOL, ip, np.nan)


def ts_of(objs, rays):
    """[n_rays, n_objects]: Hittable.hits of every object for every ray (NaN: None).  A Leaf's box test (Scene.fs:41) is left out:
    every ray of this module that meets a bounded sphere runs through its centre or is checked against the oracle alone."""
    rays = np.asarray(rays, np.float64).reshape(-1, 6)
    out = np.full((len(rays), len(objs)), np.nan)
    for k, h in enumerate(objs):
        if h.plane is not None:
            out[:, k] = plane_t(rays, np.tile(np.array([*h.plane.Point, *h.plane.Normal], np.float64), (len(rays), 1)))[0]
        else:
            out[:, k] = sphere_t(rays, np.tile(np.array([*h.sphere.Centre, h.sphere.Radius], np.float64), (len(rays), 1)))
    return out


def hit_order(objs):
    """Object indices in the order Scene.hitObject meets them: the Leaves as BoundingBoxTree.make's tree lists them left to right
    (Scene.fs:30-60; the tree by tests/fsharp_literal.py's tree_make), then the UnboundedObjects in array order."""
    boxes = [(k, L.sphere_box({"centre": tuple(h.sphere.Centre), "radius": h.sphere.Radius})) for k, h in enumerate(objs) if h.kind == A.RT_HITTABLE_SPHERE]
    leaves, todo = [], [L.tree_make(boxes)] if boxes else []
    while todo:
        t = todo.pop()
        if t[0] == "Leaf":
            leaves.append(t[1])
        else:
            todo += [t[2], t[1]]
    return np.array(leaves + [k for k, h in enumerate(objs) if h.kind != A.RT_HITTABLE_SPHERE], np.int64)


def _less(a, b):
    """Float.compare a b = Less (Float.fs:90-96)."""
    with np.errstate(invalid="ignore"):
        return ~(np.abs(a - b) < TOL) & (a < b)


RULES = ("reference", "strict", "nearest", "last_equal", "compare_in_leaves", "accept_infinite")


def winner(ts, n_bounded, rule="reference"):
    """Scene.hitObject (Scene.fs:30-91) on ts [n_rays, n_objects], whose columns are in hit_order: column of the hit, -1 for none.
    reference: a Leaf is taken when a < bestFloat, an UnboundedObject when Float.compare a bestFloat = Less.  The mutants:
    strict `<` everywhere; nearest: argmin t; last_equal: an UnboundedObject also when "Equal"; compare_in_leaves: Float.compare for
    the Leaves too; accept_infinite: an UnboundedObject with a = +inf while nothing is hit yet."""
    ts = np.asarray(ts, np.float64)
    n, m = ts.shape
    if rule == "nearest":
        some = ~np.isnan(ts)
        return np.where(some.any(axis=1), np.argmin(np.where(some, ts, INF), axis=1), -1)
    best, best_f = np.full(n, -1), np.full(n, INF)
    for k in range(m):
        t = ts[:, k]
        with np.errstate(all="ignore"):
            a = t * t
            if k < n_bounded:
                take = _less(a, best_f) if rule == "compare_in_leaves" else a < best_f
            elif rule == "strict":
                take = a < best_f
            elif rule == "last_equal":
                take = (np.abs(a - best_f) < TOL) | (a < best_f)
            else:
                take = _less(a, best_f)
                if rule == "accept_infinite":
                    take = take | ((best < 0) & np.isposinf(a))
        take = take & ~np.isnan(t)
        best, best_f = np.where(take, k, best), np.where(take, a, best_f)
    return best


def in_class(cls, objs, rays, earlier, later):
    """Whether each candidate's computed t and a = t * t land in its class."""
    ts = ts_of(objs, rays)
    rows = np.arange(len(rays))
    te, tl = ts[rows, earlier], ts[rows, later]
    with np.errstate(all="ignore"):
        d = tl * tl - te * te
        if cls == "tie" or cls == "far_tie":
            return d == 0.0
        if cls == "inside_nearer":
            return (d > -0.9e-8) & (d < -0.7e-8)
        if cls == "outside_nearer":
            return (d > -1.3e-8) & (d < -1.1e-8)
        if cls == "inside_farther":
            return (d > 0.7e-8) & (d < 0.9e-8)
        if cls == "outside_farther":
            return (d > 1.1e-8) & (d < 1.3e-8)
        if cls == "tiny":
            return (tl > TOL) & (te < 1e-4) & (te == 4.0 * tl)
        if cls == "far_ulp":
            return (tl < te) & (te - tl <= 2.0 * np.spacing(tl)) & (d <= -TOL)
        if cls == "at_infinity":  # something is hit at t * t = +inf, and nothing else is hit at all
            a = ts * ts
            return np.isposinf(a).any(axis=1) & (np.isnan(ts) | np.isposinf(a)).all(axis=1)
    raise ValueError(cls)


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
def _pulled_back(cls, b):
    """The two just-outside classes as fillers: a ray started T / 2 farther back meets both objects of its station T / 2 later,
    which turns a difference of -+0.8e-8 in t^2 into -+1.2e-8 -- the same scene, the other side of the band."""
    if cls not in ("inside_nearer", "inside_farther"):
        return None
    return [station_ray(g, i, j, back=T_OF[g] / 2.0) for g, i, j in b.stations]


@functools.lru_cache(maxsize=None)
def class_scene(cls, rot, pad=0):
    """Class `cls`: half-axis g hosts pair (g + rot) mod 5; the five rotations give every pair every half-axis."""
    b = Builder()
    for g in range(6):
        b.pair(PAIRS[(g + rot) % 5], cls, g)
    return b.finish(f"{'padded/' if pad else ''}{cls}/r{rot}", cls, SHAPE[cls], pad, _pulled_back(cls, b))


@functools.lru_cache(maxsize=None)
def leaf_leaf_scene(pad=0):
    """(leaf, leaf): two bounded spheres per station, the later-listed role 0.8e-8 nearer in t^2.  28 stations per half-axis."""
    b = Builder()
    for g in range(6):
        b.pair("leaf_leaf", "inside_nearer", g, n_i=28)
    return b.finish(f"{'padded/' if pad else ''}leaf_leaf", "inside_nearer", "grouped", pad)


@functools.lru_cache(maxsize=None)
def unbounded_only_scene(cls, rot, n_i=N_STATIONS):
    """n_bounded = 0: no tree, w.best < 0 when the unbounded tests begin.  n_i = 1 (`duo`): one station per half-axis, so that the
    pair of half-axis 0 holds the first two positions of the unbounded list and the pair of half-axis 5 the last two."""
    b = Builder()
    for g in range(6):
        b.pair(PAIRS_UU[(g + rot) % 3], cls, g, n_i=n_i)
    return b.finish(f"{'duo' if n_i == 1 else 'unbounded_only'}/{cls}/r{rot}", cls, "grouped" if n_i == 1 else SHAPE[cls])


@functools.lru_cache(maxsize=None)
def single_scene(cls):
    """A list of ONE unbounded object: (leaf, plane) on the +z half-axis alone, 9 x 8 stations."""
    b = Builder()
    b.pair("leaf_plane", cls, 4, n_i=9, n_j=8)
    return b.finish(f"single/{cls}", cls, "grouped")


def _infinity_rays():
    rng = np.random.default_rng(23)
    o = np.concatenate([rng.uniform(-3.0, 3.0, (108, 3)), np.zeros((108, 3))])
    return np.concatenate([o, rng.normal(size=(216, 3))], axis=1)  # oblique ones; Ray.make' unitises them


@functools.lru_cache(maxsize=None)
def infinity_scene(tree, pad=0):
    """at_infinity: a plane at t = 1e160 in front of every half-axis (t * t = +inf) and an unbounded sphere of radius 1e160 around
    everything (RadiusSquared, the discriminant and t are +inf).  tree: bounded spheres BEHIND every station, so that a tree is
    walked and nothing in it is hit.  No ray hits anything."""
    b = Builder()
    for g in range(6):
        b.plane(b.filler, (g, "plane", "l"), g, HUGE)
        for i in range(N_STATIONS):
            if tree:
                b.leaf((g, i, 0, "e"), g, i, 0, -T_OF[g] - 2.0)
            b.rays.append(station_ray(g, i))
            b.keys.append(("infinite", (g, "plane", "l"), (g, "plane", "l"), "later"))
    b.filler.append((("huge",), "usphere", ([0.0, 0.0, 0.0], HUGE)))
    out = b.finish(f"{'padded/' if pad else ''}at_infinity/{'tree' if tree else 'bare'}", "at_infinity", "split", pad, _infinity_rays())
    return out


MIRROR_T, MIRROR_BACK = 4.0, 2.0


@functools.lru_cache(maxsize=None)
def mirror_scene():
    """A PureReflection(1.0, White) mirror plane at z = -2 behind the +z half-axis, 16 x 16 stations of (leaf, usphere), station
    (i, j) of band class j // 4.  A ray from z = -1 along -z meets the mirror alone, comes back along +z from the strike point (the
    reflection of an incoming ray along the normal is the exact flip), and on that leg the Leaf's pole is at t = 6 and the unbounded
    sphere's differs from it by the class' delta in t^2.  Built.rays are the FIRST legs; Built.bounce the second legs."""
    g, t = 4, MIRROR_T + MIRROR_BACK
    b = Builder()
    cls_of = []
    for j in range(16):
        cls = BAND[j // 4]
        for i in range(16):
            ke, kl = (g, i, j, "e"), (g, i, j, "l")
            b.leaf(ke, g, i, j, MIRROR_T)
            b.usphere(b.filler, kl, g, i, j, (t + DELTA[cls] / (2.0 * t)) - MIRROR_BACK)
            b.rays.append(station_ray(g, i, j, back=MIRROR_BACK))
            b.stations.append((g, i, j))
            b.keys.append(("leaf_usphere", ke, kl, EXPECT[cls]))
            cls_of.append(cls)
    b.early.append([(("mirror",), "plane", ([0.0, 0.0, -MIRROR_BACK], [0.0, 0.0, 1.0]))])
    b.late.append([])
    out = b.finish("mirror", "mirror", "split", cls_of=cls_of)
    k = out.index[("mirror",)]
    out.objs[k] = H.InfinitePlane(rt.InfinitePlane.make(PS.PureReflection(1.0, rt.Colour.White), P(0.0, 0.0, -MIRROR_BACK), V(0.0, 0.0, 1.0)))
    out.mirror = k
    first = np.array(out.rays)
    first[:, 2], first[:, 5] = -1.0, -1.0
    first.setflags(write=False)
    out.first_leg = first
    out.crafted = lambda: np.concatenate([out.first_leg, out.rays])
    return out


RESIDENT = ([("class", c, r) for c in CLASSES for r in range(5)] + [("leaf_leaf",)] + [("unbounded_only", c, r) for c in BAND[:3] for r in range(3)]
            + [("duo", c, r) for c in BAND[1:3] for r in range(3)] + [("single", c) for c in BAND[1:3]] + [("infinity", False), ("infinity", True)])
PADDED = [("class", c, 0, "pad") for c in CLASSES] + [("leaf_leaf", "pad"), ("infinity", True, "pad")]
N_PAD = 1300


def scene(key) -> Built:
    pad = N_PAD if key[-1] == "pad" else 0
    if key[0] == "class":
        return class_scene(key[1], key[2], pad)
    if key[0] == "leaf_leaf":
        return leaf_leaf_scene(pad)
    if key[0] == "unbounded_only":
        return unbounded_only_scene(key[1], key[2])
    if key[0] == "duo":
        return unbounded_only_scene(key[1], key[2], 1)
    if key[0] == "single":
        return single_scene(key[1])
    if key[0] == "infinity":
        return infinity_scene(key[1], pad)
    if key[0] == "mirror":
        return mirror_scene()
    raise KeyError(key)


def label(key):
    return "/".join(str(k) for k in key)


# ---- fillers and lists -----------------------------------------------------------------------------------------------------------------
def ordinary(b: Built, n, seed):
    """Oblique hits and misses: from around a station's ray towards points near its spheres; vectors of any length."""
    rng = np.random.default_rng(seed)
    sph = np.array([[*h.sphere.Centre, h.sphere.Radius] for h in b.objs[:b.n_core] if h.sphere is not None and abs(h.sphere.Radius) < 100.0])
    if not len(sph):  # planes alone: towards anywhere
        o = rng.uniform(-40.0, 40.0, (n, 3))
        return np.concatenate([o, rng.normal(size=(n, 3)) * (10.0 ** rng.uniform(-2.0, 2.0, (n, 1)))], axis=1)
    c = sph[rng.integers(0, len(sph), n)]
    aim = c[:, :3] + rng.normal(size=(n, 3)) * rng.choice([0.3, 0.9, 1.5], (n, 1))
    o = c[:, :3] + rng.normal(size=(n, 3)) * 6.0
    return np.concatenate([o, (aim - o) * (10.0 ** rng.uniform(-2.0, 2.0, (n, 1)))], axis=1)


SIZES = (64, 65, 192)


@functools.lru_cache(maxsize=None)
def ray_lists(key):
    """[(label, rays [n, 6], crafted [n]: index into the scene's crafted rays or -1)]: lists of 64, 65 and 192 rays in which the
    crafted rays sit among fillers (oblique ordinary rays, the pulled-back rays of the two just-outside classes, the scene's other
    rays) at shuffled positions; the longest holds every crafted ray that fits."""
    b = scene(key)
    crafted = b.crafted()
    out = []
    for n in SIZES + ((len(crafted) + 64,) if len(crafted) > 160 else ()):
        rng = np.random.default_rng(n + len(crafted))
        fill = np.concatenate([ordinary(b, n, n), b.extra]) if len(b.extra) else ordinary(b, n, n)
        rays = fill[rng.choice(len(fill), n)]
        which = np.full(n, -1, np.int64)
        k = min(len(crafted), n // 2 if n < 192 else n - 32)
        pos, pick = rng.permutation(n)[:k], rng.permutation(len(crafted))[:k]
        rays[pos], which[pos] = crafted[pick], pick
        rays.setflags(write=False)
        out.append((f"{label(key)}/{n}", rays, which))
    return out


# ---- frame classes: they hold for every camera ray ------------------------------------------------------------------------------------
def frame(name):
    """(objects, camera, max_w, max_h) at 33 x 17 px and 12 spp.  tiny: the camera origin 9e-5 in front of two parallel planes listed
    far-first, the nearer one at 2e-5; focal length 64, so every ray meets them at less than 1.004 times those distances, both t
    stay below 1e-4 and the two hits are "Equal": the first listed, farther plane is every sample's colour.  at_infinity: the only
    object is a plane at 1e160: t * t = +inf for every ray, never accepted, every sample is black."""
    cam = rt.Camera.makeBasic(12, 64.0, 33.0 / 17.0, P(0.0, 0.0, 0.0), scenes.unit(0.0, 0.0, 1.0), V(0.0, 1.0, 0.0))
    cam = dataclasses.replace(cam, BounceDepth=2)
    zs = {"tiny": (9e-5, 2e-5), "at_infinity": (HUGE,)}[name]
    objs = [H.InfinitePlane(rt.InfinitePlane.make(_light(k, True), P(0.0, 0.0, z), V(0.0, 0.0, -1.0))) for k, z in enumerate(zs)]
    return objs, cam, 16, 8


FRAMES = ("tiny", "at_infinity")


# ---- InfinitePlane.intersection at its guards ---------------------------------------------------------------------------------------------
def _axis_frames(n):
    """n (normal axis, other axis, sign, k) combinations: the classes below repeat over them."""
    out = []
    for k in range(n):
        a = k % 3
        out.append((a, (a + 1 + (k // 3) % 2) % 3, -1.0 if (k // 6) % 2 else 1.0, 1.0 + (k // 12)))
    return out


def _plane_case(n_vec, d_vec, o_vec, p_vec):
    return [*o_vec, *d_vec], [*p_vec, *n_vec]


@functools.lru_cache(maxsize=None)
def plane_classes():
    """{name: (rays [n, 6], planes [n, 6] = point, normal)}, each of at least 64 rays.  What each class must answer is stated in
    tests/test_closest_hit_cases.py against plane_t."""
    rng = np.random.default_rng(41)
    out = {}

    def build(name, fn, n=72):
        rows = [fn(*f, idx) for idx, f in enumerate(_axis_frames(n))]
        out[name] = (np.array([r[0] for r in rows], np.float64), np.array([r[1] for r in rows], np.float64))

    def e(a, v=1.0):
        x = [0.0, 0.0, 0.0]
        x[a] = v
        return x

    def mix(a, va, b, vb):
        x = [0.0, 0.0, 0.0]
        x[a], x[b] = va, vb
        return x

    # the denominator n . d exactly +0.0: the ray lies in a plane parallel to the plane; the plane k in front or behind
    build("den_zero", lambda a, b, s, k, i: _plane_case(e(a, s), e(b), e(a, 0.5 * i), e(a, 0.5 * i + s * k)))
    # -0.0: three products -0.0 (a zero vector against an all-negative normal)
    build("den_negative_zero", lambda a, b, s, k, i: _plane_case([-1.0, -1.0, -k], [0.0, 0.0, 0.0], e(a, 1.0 * i), e(b, s * k)))
    for name, den in (("den_inside", 0.9e-8), ("den_outside", 1.1e-8)):
        # n = e_a, d = (den along a, 1 along b): n . d = +-den exactly; the plane 1e-6 k away on either side
        build(name + "_pos", lambda a, b, s, k, i, den=den: _plane_case(e(a), mix(a, den, b, 1.0), e(b, 1.0 * i), mix(a, s * 1e-6 * k, b, 1.0 * i)))
        build(name + "_neg", lambda a, b, s, k, i, den=den: _plane_case(e(a), mix(a, -den, b, 1.0), e(b, 1.0 * i), mix(a, s * 1e-6 * k, b, 1.0 * i)))
    for name, t in (("t_inside", 0.9e-8), ("t_outside", 1.1e-8)):
        # a unit ray straight at the plane, t away; the origin at a dyadic coordinate up to 6, so that t is good to 1e-15
        build(name, lambda a, b, s, k, i, t=t: _plane_case(e(a, -s), e(a, s), e(a, s * 0.25 * (i % 24)), e(a, s * (0.25 * (i % 24) + t))))
    build("t_zero", lambda a, b, s, k, i: _plane_case(e(a, -s if i % 2 else s), e(a, s), mix(a, 0.5 * i, b, k), mix(a, 0.5 * i, b, -k)))  # the origin on the plane
    build("t_negative", lambda a, b, s, k, i: _plane_case(e(a, -s), e(a, s), e(a, s * i), e(a, s * (i - 2.0 ** (-(i % 40)) * k))))
    build("t_huge", lambda a, b, s, k, i: _plane_case(e(a, -s), e(a, s), e(b, 1.0 * i), e(a, s * HUGE * k)))  # t = k 1e160, t * t = +inf
    build("t_overflow", lambda a, b, s, k, i: _plane_case(e(a, -s), mix(a, s * 1e-3 / k, b, 1.0), e(b, 1.0 * i), e(a, s * 1e308)))  # 1e308 / 1e-3 = +inf
    n = 96
    o, d, p, nv = rng.normal(size=(n, 3)) * 3.0, rng.normal(size=(n, 3)), rng.normal(size=(n, 3)) * 3.0, rng.normal(size=(n, 3))
    scale = 10.0 ** rng.uniform(-3.0, 3.0, (n, 2))
    out["non_unit"] = (np.concatenate([o, d * scale[:, :1]], axis=1), np.concatenate([p, nv * scale[:, 1:]], axis=1))
    for name, sc in (("coordinates_1e-3", 1e-3), ("coordinates_1e6", 1e6)):
        o, p = rng.normal(size=(n, 3)) * sc, rng.normal(size=(n, 3)) * sc
        d, nv = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
        d, nv = d / np.linalg.norm(d, axis=1, keepdims=True), nv / np.linalg.norm(nv, axis=1, keepdims=True)
        out[name] = (np.concatenate([o, d], axis=1), np.concatenate([p, nv], axis=1))
    # NaN, +inf and -inf in each of the twelve operands, over three ordinary cases each (108 rays)
    rays, planes = [], []
    for case in range(3):
        o, d, p, nv = rng.normal(size=3), rng.normal(size=3), rng.normal(size=3), rng.normal(size=3)
        for slot in range(12):
            for bad in (np.nan, np.inf, -np.inf):
                row = np.concatenate([o, d, p, nv])
                row[slot] = bad
                rays.append(row[:6])
                planes.append(row[6:])
    out["non_finite"] = (np.array(rays), np.array(planes))
    for r, p in out.values():
        r.setflags(write=False)
        p.setflags(write=False)
    return out
