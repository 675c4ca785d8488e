"""Rays whose arm of Sphere.firstIntersection's `Float.compare disc 0.0` (Sphere.fs:357-380) is known, scenes that send them through
both sphere-test sites of the render kernel (csrc/rt_device.h: `sphere_first_intersection` for the unbounded objects, the hooks and
`hit_object`; `leaf_test_object_exact` for the leaf pass), and the lane patterns in which a wave can hold them.  The Equal arm
(|disc| < 1e-8) runs behind a wave-uniform guard there and the root is taken without its +inf fix-up: a guard can be wrong by being
taken for one lane only, for all, or not at all, so the rare rays are placed at chosen lanes of chosen waves.

Shared by tests/test_sphere_arm_cases.py (no GPU: the arms restated in numpy, the cases against the oracle, the coverage conditions)
and tests/test_gpu_sphere_arms.py (the device against the oracle).

A tangent candidate of a sphere (centre c, radius r): origin c - k e_a + (r + e) e_b, direction e_a, for k = 1..39 and the three
axis pairs (a, b) = (x, y), (y, z), (z, x).  Then b = -k, |o - c|^2 = k^2 + (r + e)^2 and disc = b^2 - (|o - c|^2 - r^2) = -(2 r e + e^2):
  eq0           e = 0              disc == 0 exactly                     Equal, hit at t = k
  equal_pos     e = -0.45e-8 / r   disc about +0.9e-8                    Equal, hit at t = k
  equal_neg     e = +0.45e-8 / r   disc about -0.9e-8                    Equal, hit at t = k
  greater_edge  e = -0.55e-8 / r   disc about +1.1e-8                    Greater, just outside the band: the nearer root
  less_edge     e = +0.55e-8 / r   disc about -1.1e-8                    Less, just outside the band: none
  equal_behind  the three Equal classes with the direction reversed: b = +k, so -b is not positive: none
`disc_of` restates the discriminant in the operation order of `sphere_first_intersection`; a candidate that does not land in its
arm is dropped (tests/test_sphere_arm_cases.py holds every class to at most a tenth dropped and at least 64 kept).
"""
import dataclasses
import functools

import numpy as np

import reflection_cases
import scenes

rt = scenes.rt
P, V, S, PS, H, Tex, Px = scenes.P, scenes.V, scenes.S, scenes.PS, scenes.H, scenes.Tex, scenes.Px
TOL = 0.00000001
K = np.arange(1, 40, dtype=np.float64)
AXES = ((0, 1), (1, 2), (2, 0))  # (direction axis, offset axis)
TANGENT = {"eq0": 0.0, "equal_pos": -0.45e-8, "equal_neg": 0.45e-8, "greater_edge": -0.55e-8, "less_edge": 0.55e-8}  # e * r
EQUAL = ("eq0", "equal_pos", "equal_neg")
RARE = EQUAL + ("equal_behind",)   # what the Equal guard is taken for
HUGE_RADIUS = 1e160                # radius^2 = +inf: every ray's discriminant is +inf


# ---- scenes ------------------------------------------------------------------------------------------------------------------
def base_objects():
    """(a): two unbounded spheres with an InfinitePlane between them in array order (both positions of the unbounded list, the kind
    branch both ways in one loop), five bounded spheres (a walk tree and a leaf pass)."""
    return [
        H.UnboundedSphere(rt.Sphere.make(S.LambertReflection(0.5, Tex(Px(200, 200, 200))), P(0.0, -1000.0, 0.0), 1000.0)),
        H.InfinitePlane(rt.InfinitePlane.make(PS.LightSource(Tex(Px(255, 200, 90))), P(0.0, 0.0, 5000.0), V(0.0, 0.0, -1.0))),
        H.UnboundedSphere(rt.Sphere.make(S.LightSource(Tex(Px(180, 200, 255))), P(0.0, 0.0, 0.0), 2000.0)),
        H.Sphere(rt.Sphere.make(S.LambertReflection(0.8, Tex(Px(220, 60, 60))), P(3.0, 0.2, -2.0), 0.2)),
        H.Sphere(rt.Sphere.make(S.PureReflection(0.9, Tex(Px(230, 230, 230))), P(-4.0, 1.0, 3.0), 1.0)),
        H.Sphere(rt.Sphere.make(S.Glass(1.0, Tex(rt.Colour.White), 1.5), P(6.0, 1.0, 5.0), 1.0)),
        H.Sphere(rt.Sphere.make(S.FuzzedReflection(0.7, Tex(Px(60, 220, 60)), 0.3), P(-2.0, 0.2, -5.0), 0.2)),
        H.Sphere(rt.Sphere.make(S.LambertReflection(0.6, Tex(Px(60, 60, 220))), P(0.0, 1.0, 12.0), 1.0)),
    ]


BASE_TARGETS = (0, 2, 3, 4, 5, 6, 7)  # every object of (a) but the plane is a sphere to aim at


def padded_objects(n=1300):
    """(b): (a) followed by far-away spheres past the LDS limit (scenes.many_spheres' kind of padding): the LDS = false kernels."""
    rng = np.random.default_rng(17)
    pad = []
    for i in range(n):
        c = P(900.0 + float(rng.uniform(0, 60)), 900.0 + float(rng.uniform(0, 60)), 900.0 + float(rng.uniform(0, 60)))
        st = S.LambertReflection(0.5, Tex(Px(*(int(x) for x in rng.integers(30, 256, 3))))) if i % 2 else S.PureReflection(0.9, Tex(Px(200, 200, 200)))
        pad.append(H.Sphere(rt.Sphere.make(st, c, float(rng.uniform(0.05, 0.3)))))
    return base_objects() + pad


def inf_objects(bounded):
    """(a) and a sphere of radius 1e160, whose RadiusSquared is +inf and so is every discriminant against it: an unbounded one (the
    third of the list), or a bounded one (the scene then leaves box_implied, and every ray's leaf pass meets it)."""
    huge = rt.Sphere.make(S.LambertReflection(0.5, Tex(Px(9, 9, 9))), P(1.0, 2.0, 3.0), HUGE_RADIUS)
    return base_objects() + [(H.Sphere if bounded else H.UnboundedSphere)(huge)]


def zoo_objects():
    """(c): tests/reflection_cases.py's zoo (flipped / negative-radius and radius-1e-3 spheres, bounded and unbounded)."""
    return list(reflection_cases.zoo().objs)


def zoo_targets():
    z = reflection_cases.zoo()
    small = np.flatnonzero(~z.is_plane & (np.abs(z.r) == 1e-3))
    flipped = np.flatnonzero(~z.is_plane & (z.r == -0.5))
    return tuple(int(i) for i in np.concatenate([small[:6], flipped[:4]]))


def camera(spp=12, depth=8):
    cam = rt.Camera.makeBasic(spp, 1.0, 33.0 / 17.0, P(0.5, 1.2, -9.0), scenes.unit(0.0, -0.05, 1.0), V(0.0, 1.0, 0.0))
    return dataclasses.replace(cam, BounceDepth=depth), 16, 8  # 33 x 17 px


# ---- rays ---------------------------------------------------------------------------------------------------------------------
def spheres_of(objs):
    """[n, 4] centre and radius per object (NaN rows for planes)."""
    out = np.full((len(objs), 4), np.nan)
    for i, h in enumerate(objs):
        if h.sphere is not None:
            out[i] = [*h.sphere.Centre, h.sphere.Radius]
    return out


def disc_of(rays, sph):
    """Sphere.firstIntersection's discriminant and b, every product and sum rounded on its own in the order of
    `sphere_first_intersection`: diff = o - c; b = d . diff; cc = diff . diff - r * r; disc = b * b - cc."""
    o, d, c, r = rays[:, :3], rays[:, 3:], sph[:, :3], sph[:, 3]
    with np.errstate(all="ignore"):
        diff = o - c
        b = (d[:, 0] * diff[:, 0] + d[:, 1] * diff[:, 1]) + d[:, 2] * diff[:, 2]
        dd = (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]
        cc = dd - r * r
        return b * b - cc, b


def arm_of(disc):
    """"equal" / "greater" / "less" as Float.compare disc 0.0 says (a NaN is Greater)."""
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(disc) < TOL, "equal", np.where(disc < 0.0, "less", "greater"))


def _tangent_candidates(sph, targets, er, reverse=False):
    rays, idx = [], []
    for t in targets:
        c, r = sph[t, :3], abs(sph[t, 3])
        for a, b in AXES:
            o = np.tile(c, (len(K), 1))
            o[:, a] = c[a] - K
            o[:, b] = c[b] + (r + er / r)
            d = np.zeros((len(K), 3))
            d[:, a] = -1.0 if reverse else 1.0
            rays.append(np.concatenate([o, d], axis=1))
            idx += [t] * len(K)
    return np.concatenate(rays), np.asarray(idx, np.int32)


class Cases:
    """rays [n, 6], target [n] (the object aimed at), kept / candidates."""

    def __init__(self, name, rays, target, candidates):
        self.name, self.rays, self.target, self.candidates = name, rays, target, candidates

    def __len__(self):
        return len(self.rays)


def tangent_class(objs, targets, name):
    """The class `name` over the target spheres of `objs`; candidates outside their arm are dropped."""
    sph = spheres_of(objs)
    if name == "equal_behind":
        parts = [_tangent_candidates(sph, targets, TANGENT[k], reverse=True) for k in EQUAL]
        rays, idx = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    else:
        rays, idx = _tangent_candidates(sph, targets, TANGENT[name])
    disc, b = disc_of(rays, sph[idx])
    arm = arm_of(disc)
    keep = {"eq0": disc == 0.0, "equal_pos": (arm == "equal") & (disc > 0.0), "equal_neg": (arm == "equal") & (disc < 0.0),
            "greater_edge": (arm == "greater") & (disc < 2e-8), "less_edge": (arm == "less") & (disc > -2e-8),
            "equal_behind": (arm == "equal") & ~(-b > TOL)}[name]
    return Cases(name, rays[keep], idx[keep], len(rays))


def ordinary(objs, targets, n, seed):
    """Hits and misses to fill the waves: from around the scene towards points near the targets; directions of any length."""
    rng = np.random.default_rng(seed)
    sph = spheres_of(objs)
    t = rng.choice(np.asarray(targets), n)
    c, r = sph[t, :3], np.abs(sph[t, 3])
    aim = c + rng.normal(size=(n, 3)) * (np.minimum(r, 3.0) * rng.choice([0.3, 0.9, 1.5], n))[:, None]
    o = np.stack([rng.uniform(-12, 12, n), rng.uniform(0.5, 6.0, n), rng.uniform(-12, 12, n)], axis=1)
    far = np.abs(sph[t, 3]) > 100.0  # the huge ones: from anywhere towards anywhere
    aim[far] = rng.normal(size=(int(far.sum()), 3)) * 20.0
    v = (aim - o) * (10.0 ** rng.uniform(-2.0, 2.0, n))[:, None]
    return Cases("ordinary", np.concatenate([o, v], axis=1), t.astype(np.int32), n)


@functools.lru_cache(maxsize=None)
def classes(scene="base"):
    """{name: Cases} of a scene: "base" (also the rays of the padded and the +inf scenes, whose first objects are (a)'s) or "zoo"."""
    objs, targets = (base_objects(), BASE_TARGETS) if scene == "base" else (zoo_objects(), zoo_targets())
    out = {k: tangent_class(objs, targets, k) for k in tuple(TANGENT) + ("equal_behind",)}
    if scene == "zoo":  # around the zoo's own spheres
        rng = np.random.default_rng(5)
        sph = spheres_of(objs)
        t = rng.choice(np.flatnonzero(~np.isnan(sph[:, 3])), 600)
        aim = sph[t, :3] + rng.normal(size=(600, 3)) * np.minimum(np.abs(sph[t, 3:4]), 2.0) * 0.8
        o = aim + rng.normal(size=(600, 3)) * 3.0
        out["ordinary"] = Cases("ordinary", np.concatenate([o, aim - o], axis=1), t.astype(np.int32), 600)
    else:
        out["ordinary"] = ordinary(objs, targets, 600, 3)
    return out


# ---- lane patterns -------------------------------------------------------------------------------------------------------------
PATTERNS = ("none", "lane0", "lane63", "alternate", "all")
SIZES = (64, 65, 192)


def rare_lanes(pattern, n):
    """bool [n]: which positions of a ray list hold a rare ray, wave by wave (64 positions): none, exactly one at lane 0, exactly
    one at lane 63 (or the wave's last lane, if it is shorter), every second lane, all."""
    m = np.zeros(n, bool)
    for first in range(0, n, 64):
        last = min(first + 64, n) - 1
        if pattern == "lane0":
            m[first] = True
        elif pattern == "lane63":
            m[last] = True
        elif pattern == "alternate":
            m[first:last + 1:2] = True
        elif pattern == "all":
            m[first:last + 1] = True
    return m


def ray_list(cls, rare, pattern, n, seed):
    """A list of n rays: rays of class `rare` where rare_lanes says, fillers (ordinary hits and misses and the two classes just
    outside the band) elsewhere.  -> (rays [n, 6], is_rare [n])."""
    rng = np.random.default_rng(seed)
    m = rare_lanes(pattern, n)
    fill = np.concatenate([cls["ordinary"].rays, cls["greater_edge"].rays, cls["less_edge"].rays])
    rays = fill[rng.choice(len(fill), n)]
    rays[m] = cls[rare].rays[rng.choice(len(cls[rare]), int(m.sum()))]
    return rays, m


def all_lists(cls, sizes=SIZES, patterns=PATTERNS, rare=RARE):
    """[(label, rays, is_rare)]: every rare class in every lane pattern at every list size."""
    out = []
    for r_i, r in enumerate(rare):
        for p_i, p in enumerate(patterns):
            for n in sizes:
                rays, m = ray_list(cls, r, p, n, 1000 * r_i + 10 * p_i + n)
                out.append((f"{r}/{p}/{n}", rays, m))
    return out
