"""The oracle's Texture.colourAt (paramColourAt / textureColourAt, oracle/oracle.cpp) on the families of tests/texture_cases.py, before
tests/test_gpu_textures.py uses it to judge the device:

* where the reference evaluates a point, the oracle equals tests/fsharp_literal.py's line-by-line restatement (Texture.fs:50-72,
  Sphere.fs:55-61): (u, v) bit for bit and the colour -- the recursion at every depth, the image orientation, and that the ROOT's map
  is the one used at every level;
* where the reference throws (a NaN or out-of-range texel index, a NaN ramp byte), the oracle equals the rule in the header comment of
  texel_index / ramp_byte (csrc/rt_device.h), restated here in numpy;
* the split cannot hide a failure: outside the `maps` family and the plane wearer, at least 99 % of the points are ones the literal
  evaluates.

And rt_scene_create's checks on texture records, through the raw ABI (host only)."""
import ctypes as C
import math

import numpy as np
import pytest

import fsharp_literal as L
import scenes
import texture_cases as tc
from ray_tracing_fsharp_amd import _abi as A


class _Strict(list):
    """F# arrays throw on a negative index (Python's wrap round); rows and images of the literal are wrapped in this."""

    def __getitem__(self, i):
        if not 0 <= i < len(self):
            raise IndexError(i)
        return list.__getitem__(self, i)


def _ramp_closure(src, const):
    def closure(x, y):  # RayTracing.App/SampleImages.fs:606-627: byte (float x * 255.0) per ramped channel
        return ("Colour", tuple(int(x * 255.0) & 0xFF if s == A.RT_RAMP_U else int(y * 255.0) & 0xFF if s == A.RT_RAMP_V else c for s, c in zip(src, const)))
    return closure


def literal_of(tex, ident, memo):
    """Record `ident` of an rt_texture array -> the literal's tagged tuples (shared children stay shared)."""
    if ident in memo:
        return memo[ident]
    t = tex[ident]
    if t.kind == A.RT_TEXTURE_COLOUR:
        out = ("Colour", tuple(t.rgb))
    elif t.kind == A.RT_TEXTURE_CHECKERED:
        out = ("Checkered", literal_of(tex, t.even, memo), literal_of(tex, t.odd, memo), t.grid_size)
    elif t.kind == A.RT_TEXTURE_IMAGE:
        out = ("Image", _Strict(_Strict(tuple(int(c) for c in px) for px in row) for row in tc.texels_of(t)))
    else:
        out = ("Arbitrary", _ramp_closure(tuple(t.ramp_src), tuple(t.rgb)))
    memo[ident] = out
    return out


def literal_colours(tex, ident, points):
    """-> (evaluated [n] bool, uv [n, 2], colour [n, 3]) by fsharp_literal.param_colour_at through ParameterisedTexture.toTexture."""
    root = tex[ident]
    inner = L.plane_map_inverse(root.map_radius, tuple(root.map_centre)) if root.map_radius != 0.0 else None
    cache = {}

    def interpret(p):  # pure, and called once per level by the literal: evaluated once per point
        key = tuple(c.hex() for c in p)  # not p itself: -0.0 == 0.0
        if key not in cache:
            cache[key] = inner(p)
        return cache[key]
    texture = L.to_texture(interpret, literal_of(tex, ident, {}))
    ok, uv, col = np.zeros(len(points), bool), np.full((len(points), 2), np.nan), np.zeros((len(points), 3), np.uint8)
    for i, p in enumerate(points):
        p = tuple(float(c) for c in p)
        try:
            if inner is None:
                raise ZeroDivisionError  # 1.0 / 0.0 is an infinity in F#; the point then has no finite map coordinates anyway
            col[i] = L.texture_colour_at(p, texture)
            if root.kind != A.RT_TEXTURE_COLOUR:
                uv[i] = interpret(p)
            ok[i] = True
        except (ValueError, OverflowError, IndexError, ZeroDivisionError):  # int NaN / an index out of range: the reference throws
            pass
    return ok, uv, col


def _texel_index(v, n):
    """texel_index's header comment (csrc/rt_device.h): `int (v * float (n - 1))`; NaN and negative products take texel 0, products
    beyond the last texel take the last one."""
    with np.errstate(invalid="ignore"):
        t = v * float(n - 1)
        return np.where(np.isnan(t) | (t < 0.0), 0, np.where(t >= n - 1, n - 1, np.trunc(np.nan_to_num(t, posinf=0.0)))).astype(np.int64)


def _ramp_byte(v):
    with np.errstate(invalid="ignore"):
        t = v * 255.0
        return np.where(np.isnan(t), 0, np.trunc(np.nan_to_num(t)).astype(np.int64) & 0xFF).astype(np.uint8)


def leaf_records(orc, tex, ident, uv):
    """The descent of Texture.fs:56-62 on the records, for ANY (u, v): the record each point ends at (a NaN sine is "not Less": odd).
    Math.Sin is the oracle's correctly rounded one."""
    x, y = uv[:, 0], uv[:, 1]
    cur = np.full(len(uv), ident)
    for _ in range(len(tex) + 1):
        pending = False
        for k in np.unique(cur):
            t, sel = tex[int(k)], cur == k
            if t.kind == A.RT_TEXTURE_CHECKERED:
                with np.errstate(invalid="ignore"):
                    sine = orc.arith(8, t.grid_size * x[sel]) * orc.arith(8, t.grid_size * y[sel])
                    less = ~(np.abs(sine - 0.0) < L.TOL) & (sine < 0.0)  # Float.compare sine 0.0 = Less (Float.fs:90-96)
                cur[sel] = np.where(less, t.even, t.odd)
                pending = True
        if not pending:
            return cur
    raise AssertionError("descent did not end")


def rule_colours(orc, tex, ident, uv):
    """The defined behaviour for ANY (u, v), NaN included: the descent, then texel_index and ramp_byte as their comments state them."""
    out = np.zeros((len(uv), 3), np.uint8)
    if tex[ident].kind == A.RT_TEXTURE_COLOUR:  # ParameterisedTexture.toTexture's Colour case: no map is evaluated
        out[:] = tuple(tex[ident].rgb)
        return out
    x, y = uv[:, 0], uv[:, 1]
    cur = leaf_records(orc, tex, ident, uv)
    for k in np.unique(cur):
        t, sel = tex[int(k)], cur == k
        if t.kind == A.RT_TEXTURE_IMAGE:
            out[sel] = tc.texels_of(t)[_texel_index(y[sel], t.height), _texel_index(1.0 - x[sel], t.width)]
        elif t.kind == A.RT_TEXTURE_UV_RAMP:
            for ch in range(3):
                out[sel, ch] = _ramp_byte(x[sel]) if t.ramp_src[ch] == A.RT_RAMP_U else _ramp_byte(y[sel]) if t.ramp_src[ch] == A.RT_RAMP_V else t.rgb[ch]
        else:
            out[sel] = tuple(t.rgb)
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("family", sorted(tc.FAMILIES))
def test_oracle_equals_the_literal_and_the_stated_rule(orc, family):
    for case in tc.FAMILIES[family]():
        _, o = scenes.raw_scene_pair(orc, *case.arrays())
        for q in case.queries:
            where = f"{family}/{case.name}/hittable {q.hittable}"
            uv, col = o.texture_colour_at(q.texture, q.points)
            ok, luv, lcol = literal_colours(case.tex, q.texture, q.points)
            if case.tex[q.texture].kind != A.RT_TEXTURE_COLOUR:
                assert np.array_equal(_bits(uv[ok]), _bits(luv[ok])), f"{where}: (u, v) differs from the literal"
            bad = np.flatnonzero(ok & np.any(col != lcol, axis=1))
            assert bad.size == 0, f"{where}: {bad.size} colours differ from the literal, first at {q.points[bad[0]]}: {col[bad[0]]} vs {lcol[bad[0]]}"
            if q.on_map:
                assert ok.mean() >= 0.99, f"{where}: the literal evaluates only {ok.mean():.3%} of the points"
            # every point, the reference's throws included, against the rule as stated (for the points above this is a second,
            # vectorised statement of the same function)
            want = rule_colours(orc, case.tex, q.texture, uv)
            bad = np.flatnonzero(np.any(col != want, axis=1))
            assert bad.size == 0, f"{where}: {bad.size} colours differ from the stated rule, first at {q.points[bad[0]]} uv {uv[bad[0]]}: {col[bad[0]]} vs {want[bad[0]]}"


def test_the_families_reach_what_they_are_for(orc):
    """The inputs do what their families claim: chains are descended to the last leaf (and left at most levels on the way), every
    leaf of the balanced tree is reached, the maps family holds points the reference throws on, every id resolves differently."""
    for case in tc.family_chains():
        depth = 253 if case.objs is None else int(case.name[5:])
        _, o = scenes.raw_scene_pair(orc, *case.arrays())
        q = case.queries[0]
        _, col = o.texture_colour_at(q.texture, q.points)
        seen = {tuple(c) for c in col.tolist()}
        assert tuple(tc.colour_of(depth)) in seen, case.name
        assert (col == np.array(tc.colour_of(depth), np.uint8)).all(axis=1).mean() > 0.25, case.name
        if case.objs is not None:
            leaves = {tuple(tc.colour_of(k)) for k in range(depth + 1)}
            assert seen <= leaves and len(seen) >= min(depth + 1, 0.6 * depth), (case.name, len(seen))
        hit, _, _ = o.hit_object(q.rays)
        assert (hit == q.hittable).all(), case.name
    case = next(tc.family_trees())
    _, o = scenes.raw_scene_pair(orc, *case.arrays())
    q = case.queries[0]
    uv, _ = o.texture_colour_at(q.texture, q.points)
    leaves = set(leaf_records(orc, case.tex, q.texture, uv).tolist())
    assert len(leaves) == 64
    thrown = 0
    for case in tc.family_maps():
        for q in case.queries:
            ok, _, _ = literal_colours(case.tex, q.texture, q.points)
            thrown += int((~ok).sum())
    assert thrown > 2000
    case = next(tc.family_ids())
    _, o = scenes.raw_scene_pair(orc, *case.arrays())
    firsts = [tuple(o.texture_colour_at(q.texture, q.points[:1])[1][0]) for q in case.queries]
    assert [q.texture for q in case.queries] == list(tc.ID_WEARERS) and len(set(firsts)) == len(firsts)


# ---- rt_scene_create on texture records (build_scene, csrc/rt_scene.h; the contract is include/rtfs_amd.h) -------------------------
def _create(rt, hitt, recs):
    hs = (A.rt_hittable * max(1, len(hitt)))(*hitt)
    tex = (A.rt_texture * max(1, len(recs)))(*recs)
    out = C.c_void_p()
    rc = rt.lib.rt_scene_create(hs, len(hitt), tex, len(recs), C.byref(out))
    msg = rt.lib.rt_last_error().decode() if rc else ""
    if rc == A.RT_OK:
        return rc, rt.Scene(out.value, [hs, tex]), msg
    assert not out.value
    return rc, None, msg


def test_texture_records_are_checked_at_creation(rt):
    wearer = tc.raw_sphere(A.RT_SPHERE_LAMBERT_REFLECTION, (0.0, 0.0, 0.0), 1.0, 0)
    leaf = tc.rec_colour((1, 2, 3))
    # Checkered children "must be < own index" (rtfs_amd.h): equal, above, negative -> RT_ERR_INVALID_ARGUMENT
    for even, odd in ((1, 0), (0, 1), (2, 0), (0, 2), (-1, 0), (0, -1), (-2 ** 31, 0)):
        rc, _, msg = _create(rt, [wearer], [leaf, tc.rec_checkered(even, odd, 3.0), leaf])
        assert rc == A.RT_ERR_INVALID_ARGUMENT and "smaller indices" in msg, (even, odd, rc, msg)
    assert _create(rt, [wearer], [tc.rec_checkered(0, 0, 3.0)])[0] == A.RT_ERR_INVALID_ARGUMENT  # record 0 can have no children
    # grid sizes: |g| <= 5e5 accepted (rt_trig.h reduces below 2^20 exactly), beyond it and NaN -> RT_ERR_UNSUPPORTED
    for g, want in ((5e5, A.RT_OK), (-5e5, A.RT_OK), (0.0, A.RT_OK), (-0.0, A.RT_OK), (1e-300, A.RT_OK), (math.nextafter(5e5, math.inf), A.RT_ERR_UNSUPPORTED),
                    (-math.nextafter(5e5, math.inf), A.RT_ERR_UNSUPPORTED), (math.nan, A.RT_ERR_UNSUPPORTED), (math.inf, A.RT_ERR_UNSUPPORTED)):
        rc, _, msg = _create(rt, [wearer], [leaf, tc.rec_checkered(0, 0, g)])
        assert rc == want and (rc == A.RT_OK or "grid size" in msg), (g, rc, msg)
    # images: NULL texels, non-positive sizes -> RT_ERR_INVALID_ARGUMENT
    keep = []
    good = tc.rec_image(tc.synthetic_image(2, 3), keep)
    assert _create(rt, [wearer], [good])[0] == A.RT_OK
    for field, value in (("texels", None), ("width", 0), ("height", 0), ("width", -1), ("height", -3)):
        bad = tc.rec_image(tc.synthetic_image(2, 3), keep)
        setattr(bad, field, value)
        rc, _, msg = _create(rt, [wearer], [bad])
        assert rc == A.RT_ERR_INVALID_ARGUMENT and "image" in msg, (field, value, rc, msg)
    # ramp sources are rt_ramp_source: 3 is none of them -> RT_ERR_INVALID_ARGUMENT
    for ch in range(3):
        src = [A.RT_RAMP_U, A.RT_RAMP_V, A.RT_RAMP_CONST]
        assert _create(rt, [wearer], [tc.rec_ramp(src)])[0] == A.RT_OK
        src[ch] = 3
        rc, _, msg = _create(rt, [wearer], [tc.rec_ramp(src)])
        assert rc == A.RT_ERR_INVALID_ARGUMENT and "ramp" in msg, (ch, rc, msg)
    # a kind that is none of rt_texture_kind stands for a closure -> RT_ERR_UNSUPPORTED
    bad = tc.rec_colour((1, 1, 1))
    bad.kind = 4
    assert _create(rt, [wearer], [bad])[0] == A.RT_ERR_UNSUPPORTED


def test_texture_count_limit_and_ids(rt):
    """254 records are accepted, 255 refused with RT_ERR_UNSUPPORTED (an id rides in 8 bits of an object's record, 0 = none);
    a hittable may wear any id below the count and none at or above it."""
    recs = [tc.rec_colour(tc.colour_of(k)) for k in range(255)]
    for wears in (0, 127, 128, 253):
        rc, s, _ = _create(rt, [tc.raw_sphere(A.RT_SPHERE_LIGHT_SOURCE, (0.0, 0.0, 0.0), 1.0, wears)], recs[:254])
        assert rc == A.RT_OK and s.info()["n_textures"] == 254 and s.info()["texel_bytes"] == 0
    rc, _, msg = _create(rt, [tc.raw_sphere(A.RT_SPHERE_LIGHT_SOURCE, (0.0, 0.0, 0.0), 1.0, 254)], recs[:254])
    assert rc == A.RT_ERR_INVALID_ARGUMENT and "texture index" in msg
    rc, _, msg = _create(rt, [tc.raw_sphere(A.RT_SPHERE_LIGHT_SOURCE, (0.0, 0.0, 0.0), 1.0, 0)], recs)
    assert rc == A.RT_ERR_UNSUPPORTED and "254" in msg
    rc, _, msg = _create(rt, [], recs)  # the limit is on the records, worn or not
    assert rc == A.RT_ERR_UNSUPPORTED
    # the deepest chain a scene can hold is accepted, through the mirror (126: children are not shared) and raw (253)
    for case in tc.family_chains():
        s, _ = scenes.raw_scene_pair(None, *case.arrays())
        assert s.info()["n_textures"] == case.ntex
    with pytest.raises(rt.RtError) as e:
        rt.Scene.make([tc.wear(0, tc.chain_param(127))])
    assert e.value.code == A.RT_ERR_UNSUPPORTED


def test_styles_that_carry_a_pixel_refuse_a_texture_id(rt):
    """"sphere styles with a texture only" (rt_hittable.texture), and the plane LightSource (InfinitePlane.fs:5): LightSourceCap and
    the three Pixel-carrying plane styles -> RT_ERR_INVALID_ARGUMENT; every other style accepts the id."""
    recs = [tc.rec_colour((5, 6, 7))]
    for kind in (A.RT_HITTABLE_SPHERE, A.RT_HITTABLE_UNBOUNDED_SPHERE):
        for style in range(A.RT_SPHERE_GLASS + 1):
            rc, _, msg = _create(rt, [tc.raw_sphere(style, (0.0, 0.0, 0.0), 1.0, 0, kind=kind)], recs)
            assert rc == (A.RT_ERR_INVALID_ARGUMENT if style == A.RT_SPHERE_LIGHT_SOURCE_CAP else A.RT_OK), (kind, style, msg)
    for style in range(A.RT_PLANE_FUZZED_REFLECTION + 1):
        h = tc.raw_sphere(style, (0.0, 0.0, 0.0), 0.0, 0, kind=A.RT_HITTABLE_INFINITE_PLANE)
        h.normal[:] = (0.0, 1.0, 0.0)
        rc, _, msg = _create(rt, [h], recs)
        assert rc == (A.RT_OK if style == A.RT_PLANE_LIGHT_SOURCE else A.RT_ERR_INVALID_ARGUMENT), (style, msg)
        assert rc == A.RT_OK or "carries a Pixel" in msg


def test_scene_info_reports_textures_and_padded_texel_bytes(rt):
    """texel_bytes counts the blob as stored: every image padded to a multiple of 16 bytes."""
    keep = []
    sizes = [(1, 1), (1, 7), (3, 5), (2, 8), (3, 257), (16, 1)]  # 3, 21, 45, 48, 2313, 48 bytes
    recs = [tc.rec_image(tc.synthetic_image(h, w, salt=i), keep) for i, (h, w) in enumerate(sizes)] + [tc.rec_colour((1, 1, 1))]
    rc, s, _ = _create(rt, [tc.raw_sphere(A.RT_SPHERE_LIGHT_SOURCE, (0.0, 0.0, 0.0), 1.0, 4)], recs)
    assert rc == A.RT_OK
    info = s.info()
    assert info["n_textures"] == 7
    assert info["texel_bytes"] == sum((h * w * 3 + 15) // 16 * 16 for h, w in sizes) == 16 + 32 + 48 + 48 + 2320 + 48
    for case in tc.family_images():
        s, _ = scenes.raw_scene_pair(None, *case.arrays())
        images = [t for t in case.tex[: case.ntex] if t.kind == A.RT_TEXTURE_IMAGE]
        assert len(images) > 1 and s.info()["texel_bytes"] == sum((t.height * t.width * 3 + 15) // 16 * 16 for t in images)
