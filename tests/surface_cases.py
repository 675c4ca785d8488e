"""What rt_surfaces / rt_camera_surfaces must answer, composed from the oracle's pieces and the numpy restatements and never from the
library.  Per slot (hit_index, strike, the incoming ray):

    normal, inside, the cap comparison   reflection_cases.probe: `reflection`'s decisions, every product rounded on its own;
                                         normal is NaN where fsharp_literal.ray_make_prime(strike, strike - centre) gives None
    colour                               the hittable's Pixel, OracleScene.texture_colour_at(texture, strike), or the cap rule
    uv                                   that same call's, where the texture's root record is not COLOUR; NaN elsewhere
    tint                                 INDEPENDENTLY, OracleScene.reflection(idx, ray, White, strike, any state)'s colour

and the composer itself asserts that tint is colour on the slots Reflection absorbs and fsharp_literal.pixel_darken(albedo, colour) on
the others.  A slot with hit_index < 0 or a strike / origin that is not finite has no surface: NaN normal and uv, zeros elsewhere.

`compose(..., mutant=NAME)` plants one of the MUTANTS -- the mistakes a kernel of this kind makes; tests/test_surface_cases.py shows that
each changes the answer on the case set, i.e. that the cases would catch it."""
from typing import NamedTuple

import numpy as np

import fsharp_literal as L
import reflection_cases as rc

rt = rc.rt
A = rt._abi

MUTANTS = ("normal_not_flipped", "flipped_dropped", "cap_ge", "cap_coordinate_1", "darken_emitters", "plane_normal_towards_ray", "uv_for_colour_root")


class Expected(NamedTuple):
    normal: np.ndarray    # [n, 3] float64
    inside: np.ndarray    # [n] uint8
    colour: np.ndarray    # [n, 3] uint8
    tint: np.ndarray      # [n, 3] uint8
    uv: np.ndarray        # [n, 2] float64
    textured: np.ndarray  # [n] bool: the slot's colour is Texture.colourAt on a parameterised texture whose root is not COLOUR
    cap: np.ndarray       # [n] int: reflection_cases' GT / EQ / LT of the cap comparison on LightSourceCap slots, -1 elsewhere


class SceneTable:
    """Per object of a scene: what flatten_hittables hands the library, plus reflection_cases.Zoo's arrays."""

    def __init__(self, objs=None, arrays=None):
        """objs: host-mirror Hittables; or arrays = (rt_hittable array, n, rt_texture array, ntex, keep) for a scene made by hand."""
        hs, n, tex, ntex, keep = rt.raytracing.flatten_hittables(objs) if arrays is None else arrays
        self._keep = (hs, tex, keep)
        self.n = n
        z = self.zoo = rc.Zoo([])  # reflection_cases.probe's view of the objects, filled from the records
        z.kind = np.array([hs[i].kind for i in range(n)], np.int32)
        z.style = np.array([hs[i].style for i in range(n)], np.int32)
        z.is_plane = z.kind == A.RT_HITTABLE_INFINITE_PLANE
        z.c = np.array([list(hs[i].point) for i in range(n)], np.float64).reshape(n, 3)
        z.nrm = np.array([list(hs[i].normal) for i in range(n)], np.float64).reshape(n, 3)
        z.r = np.where(z.is_plane, 0.0, np.array([hs[i].radius for i in range(n)], np.float64))
        z.albedo, z.fuzz = np.array([hs[i].albedo for i in range(n)], np.float64), np.array([hs[i].fuzz for i in range(n)], np.float64)
        z.ior, z.prob = np.array([hs[i].ior for i in range(n)], np.float64), np.array([hs[i].prob for i in range(n)], np.float64)
        self.rgb = np.array([[hs[i].rgb[0], hs[i].rgb[1], hs[i].rgb[2]] for i in range(n)], np.uint8).reshape(n, 3)
        carries = np.where(z.is_plane, z.style == A.RT_PLANE_LIGHT_SOURCE, z.style != A.RT_SPHERE_LIGHT_SOURCE_CAP)  # the styles that hold a Texture
        self.texture = np.where(carries, np.array([hs[i].texture for i in range(n)], np.int32), -1).astype(np.int32)
        self.root_kind = np.array([tex[int(t)].kind if t >= 0 else -1 for t in self.texture], np.int32)
        cap = ~z.is_plane & (z.style == A.RT_SPHERE_LIGHT_SOURCE_CAP)
        self.emitter = np.where(z.is_plane, z.style == A.RT_PLANE_LIGHT_SOURCE, (z.style == A.RT_SPHERE_LIGHT_SOURCE) | cap)
        self.cap = cap


def same_f64(a, b):
    """Bit for bit, NaNs compared by position."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def no_surface(hit, strike, rays):
    return (np.asarray(hit) < 0) | ~np.isfinite(strike).all(axis=1) | ~np.isfinite(rays[:, :3]).all(axis=1)


def compose(orc, oracle_scene, table: SceneTable, hit, strike, rays, mutant=None) -> Expected:
    """hit [n] int32, strike [n, 3], rays [n, 6] (origin, unit direction; only the origin matters to the answer)."""
    assert mutant is None or mutant in MUTANTS
    hit = np.asarray(hit, np.int32).reshape(-1)
    strike, rays = np.asarray(strike, np.float64).reshape(-1, 3), np.asarray(rays, np.float64).reshape(-1, 6)
    n = len(hit)
    normal, uv = np.full((n, 3), np.nan), np.full((n, 2), np.nan)
    inside, colour, tint = np.zeros(n, np.uint8), np.zeros((n, 3), np.uint8), np.zeros((n, 3), np.uint8)
    textured, cap = np.zeros(n, bool), np.full(n, -1, np.int64)
    sel = np.flatnonzero(~no_surface(hit, strike, rays))
    if len(sel) == 0:
        return _frozen(Expected(normal, inside, colour, tint, uv, textured, cap))
    idx, sk, ry = hit[sel], strike[sel], rays[sel]
    z = table.zoo
    pr = rc.probe(z, idx, ry, sk)
    plane = z.is_plane[idx]
    ins, nrm = pr.inside.copy(), pr.n.copy()
    if mutant == "normal_not_flipped":
        nrm = np.where((ins & ~plane)[:, None], -1.0 * nrm, nrm)  # (undoes the flip: -1.0 * x twice is x, bit for bit)
    if mutant == "flipped_dropped":
        ins = (pr.cmp != rc.GT) & ~plane
        with np.errstate(all="ignore"):
            n0 = rc.unitise(sk - z.c[idx])
        nrm = np.where(plane[:, None], z.nrm[idx], np.where(ins[:, None], -1.0 * n0, n0))
    if mutant == "plane_normal_towards_ray":
        towards = plane & (rc.dot3(nrm, ry[:, 3:]) > 0.0)
        nrm = np.where(towards[:, None], -1.0 * nrm, nrm)
    for k in np.flatnonzero(~plane):  # Sphere.normal: Ray.make' strike (strike - centre); ValueNone -> the reference throws, NaN here
        if L.ray_make_prime(tuple(sk[k]), L.v_diff(tuple(sk[k]), tuple(z.c[idx[k]]))) is None:
            nrm[k] = np.nan
    normal[sel], inside[sel] = nrm, ins.astype(np.uint8)

    # colour
    col = table.rgb[idx].copy()
    tx = table.texture[idx]
    u = np.full((len(sel), 2), np.nan)
    for t in np.unique(tx[tx >= 0]):
        m = tx == t
        got_uv, got_col = oracle_scene.texture_colour_at(int(t), sk[m])
        col[m] = got_col
        kind = table.root_kind[idx][m][0]
        if kind != A.RT_TEXTURE_COLOUR or mutant == "uv_for_colour_root":
            u[m] = got_uv if kind != A.RT_TEXTURE_COLOUR else np.array([L.plane_map_inverse(*_map_of(table, int(t)))(tuple(p)) for p in sk[m]]).reshape(-1, 2)
    is_tex = (tx >= 0) & (table.root_kind[idx] != A.RT_TEXTURE_COLOUR)
    is_cap = table.cap[idx]
    capcmp = pr.cap
    if mutant == "cap_coordinate_1":
        capcmp = rc.fcmp(sk[:, 1], pr.lower)
    lit = (capcmp == rc.GT) | ((capcmp == rc.EQ) if mutant == "cap_ge" else False)
    col[is_cap & ~lit] = 0
    colour[sel], uv[sel], textured[sel] = col, u, is_tex
    cap[sel] = np.where(is_cap, pr.cap, -1)

    # tint, independently: what Hittable.Reflection leaves a White LightRay with
    unit = ry.copy()
    bad_dir = ~np.isfinite(unit[:, 3:]).all(axis=1)
    unit[bad_dir, 3:] = (0.0, 0.0, 1.0)  # (the direction cannot matter to the colour; the oracle wants a ray)
    have_n = ~np.isnan(nrm).any(axis=1)
    white = np.full((len(sel), 3), 255, np.uint8)
    state = np.tile(np.array([[123456789, 362436069, 521288629, 88675123]], np.uint32), (len(sel), 1))
    tn = np.zeros((len(sel), 3), np.uint8)
    if have_n.any():
        absorbed, tcol, _, _ = oracle_scene.reflection(idx[have_n], unit[have_n], white[have_n], sk[have_n], state[have_n])
        tn[have_n] = tcol
        assert np.array_equal(absorbed != 0, table.emitter[idx[have_n]])
    albedo = z.albedo[idx]
    darkened = np.array([L.pixel_darken(float(a), tuple(int(v) for v in c)) for a, c in zip(albedo, col)], np.uint8).reshape(-1, 3)
    want = np.where(table.emitter[idx][:, None], col, darkened)
    if mutant is None:
        assert np.array_equal(tn[have_n], want[have_n]), "tint is colour on absorbed slots, Pixel.darken albedo colour on the others"
        tn[~have_n] = want[~have_n]  # (the reference throws there: the rule above stands in)
    else:
        tn = want  # (a kernel with the mistake forms its tint from its own colour)
    if mutant == "darken_emitters":
        tn = darkened
    tint[sel] = tn
    return _frozen(Expected(normal, inside, colour, tint, uv, textured, cap))


def _map_of(table, t):
    tex = table._keep[1][t]
    return float(tex.map_radius), tuple(float(v) for v in tex.map_centre)


def _frozen(e):
    for a in e:
        a.setflags(write=False)
    return e


def differs(a: Expected, b: Expected):
    """The outputs in which two answers differ."""
    out = []
    if not same_f64(a.normal, b.normal):
        out.append("normal")
    if not same_f64(a.uv, b.uv):
        out.append("uv")
    for f in ("inside", "colour", "tint"):
        if not np.array_equal(getattr(a, f), getattr(b, f)):
            out.append(f)
    return out


def raw_roots_scene():
    """A scene made by hand for what the host mirror cannot express: spheres that wear a COLOUR root record (the library takes the record's
    Pixel and fills no uv), a ramp and a Checkered root beside them, and EMITTERS with an albedo other than 1 (Reflection never darkens
    them): a LightSource sphere, a LightSourceCap and a LightSource plane.  -> (arrays for scenes.raw_scene_pair, hit, strike, rays)."""
    import texture_cases as tc
    keep = []
    recs = [tc.rec_colour((10, 200, 30)), tc.rec_ramp((1, 2, 0), (0, 0, 77)), tc.rec_colour((250, 1, 2)), tc.rec_colour((3, 4, 5))]
    recs.append(tc.rec_checkered(2, 3, 30.0))
    centres = [np.array([8.0 * i, 0.0, 0.0]) for i in range(5)]
    for k, t in ((0, 0), (1, 1), (4, 2)):
        tc.set_map(recs[k], 1.0, centres[t])
    hs = [tc.raw_sphere(A.RT_SPHERE_LAMBERT_REFLECTION, centres[0], 1.0, 0, albedo=0.5),   # COLOUR root, darkened
          tc.raw_sphere(A.RT_SPHERE_LIGHT_SOURCE, centres[1], 1.0, 1, albedo=0.25),        # ramp root on an emitter with albedo 0.25
          tc.raw_sphere(A.RT_SPHERE_PURE_REFLECTION, centres[2], 1.0, 4, albedo=0.75),     # Checkered root over two COLOUR leaves
          tc.raw_sphere(A.RT_SPHERE_LIGHT_SOURCE_CAP, centres[3], 1.0, -1, albedo=0.5, rgb=(200, 100, 50)),
          tc.raw_sphere(A.RT_SPHERE_LIGHT_SOURCE, centres[4], 1.0, 0, albedo=0.5, kind=A.RT_HITTABLE_UNBOUNDED_SPHERE)]
    pl = A.rt_hittable()
    pl.kind, pl.style, pl.albedo, pl.texture = A.RT_HITTABLE_INFINITE_PLANE, A.RT_PLANE_LIGHT_SOURCE, 0.5, -1
    pl.point[:], pl.normal[:], pl.rgb[:] = (0.0, -50.0, 0.0), (0.0, 1.0, 0.0), (90, 180, 240)
    hs.append(pl)
    arrays = ((A.rt_hittable * len(hs))(*hs), len(hs), (A.rt_texture * len(recs))(*recs), len(recs), keep)
    rng = np.random.default_rng(33)
    hit, strike, rays = [], [], []
    for i in range(5):
        u = rng.normal(size=(40, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        p = centres[i] + u
        o = centres[i] + 3.0 * u + rng.normal(size=u.shape) * 0.1
        d = p - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        hit.append(np.full(40, i, np.int32)); strike.append(p); rays.append(np.concatenate([o, d], axis=1))
    p = np.stack([rng.uniform(-20, 20, 40), np.full(40, -50.0), rng.uniform(-20, 20, 40)], axis=1)
    o = p + np.array([0.0, 5.0, 0.0])
    hit.append(np.full(40, 5, np.int32)); strike.append(p); rays.append(np.concatenate([o, np.tile([0.0, -1.0, 0.0], (40, 1))], axis=1))
    return arrays, np.concatenate(hit), np.concatenate(strike), np.concatenate(rays)
