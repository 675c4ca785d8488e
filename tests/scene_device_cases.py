"""Named record sets for Scene.make on the device (rt_scene_create_device): each the smallest that can go wrong at its edge.

CASES: name -> () -> (records, textures): valid scenes.  REFUSALS: the same for record sets that every route refuses.  records: a numpy array
of rt_hittable (rt.HITTABLE_DTYPE); textures: None, or (the ctypes rt_texture array, its count, what it points into) -- the arguments of
rt.TextureTable.  Nothing here touches a device or needs more of the package than its ABI mirror, so the script that records the parent's
scenes (tests/golden/make_scene_images_parent.py) runs these cases on a library from before the device route existed."""
import numpy as np

import ray_tracing_fsharp_amd as rt
from ray_tracing_fsharp_amd import _abi as A

import scenes

DT = np.dtype(A.rt_hittable)  # (= rt.HITTABLE_DTYPE, which tests/test_scene_device_host.py holds to it)


def spheres(centres, radii, style=A.RT_SPHERE_LAMBERT_REFLECTION, kind=A.RT_HITTABLE_SPHERE):
    centres = np.asarray(centres, np.float64).reshape(-1, 3)
    r = np.zeros(len(centres), DT)
    r["kind"], r["style"], r["point"], r["radius"] = kind, style, centres, radii
    r["albedo"], r["fuzz"], r["ior"], r["prob"], r["texture"] = 0.8, 0.25, 1.5, 0.6, -1
    r["rgb"] = (np.arange(len(centres))[:, None] * [7, 13, 29] + [40, 80, 120]) % 256
    return r


def planes(points, normals, style=A.RT_PLANE_LAMBERT_REFLECTION):
    points = np.asarray(points, np.float64).reshape(-1, 3)
    r = np.zeros(len(points), DT)
    r["kind"], r["style"], r["point"], r["normal"] = A.RT_HITTABLE_INFINITE_PLANE, style, points, normals
    r["albedo"], r["fuzz"], r["texture"], r["rgb"] = 0.7, 0.3, -1, (200, 180, 160)
    return r


def random_spheres(n, seed, spread=20.0):
    rng = np.random.default_rng(seed)
    r = spheres(rng.uniform(-spread, spread, (n, 3)), rng.uniform(0.05, 0.4, n))
    r["style"] = rng.integers(0, 7, n)
    r["ior"] = rng.uniform(0.7, 2.0, n)
    return r


def from_objects(objs):
    hs, n, tex, ntex, keep = rt.raytracing.flatten_hittables(objs)
    return np.frombuffer(hs, dtype=DT, count=n).copy(), ((tex, ntex, keep) if ntex else None)


def _interleaved():
    """bounded and unbounded in turn, so that a partition that is not stable on either side shows in the object table"""
    s = random_spheres(9, 3, 4.0)
    out = np.zeros(17, DT)
    out[0::2] = s
    out[1::4] = planes(np.arange(12.0).reshape(4, 3), (0.0, 1.0, 0.0))
    u = spheres(np.arange(12.0).reshape(4, 3) - 5.0, [50.0, -30.0, 70.0, 90.0], kind=A.RT_HITTABLE_UNBOUNDED_SPHERE)
    out[3::4] = u
    return out, None


def _flipped():
    r = random_spheres(7, 5, 3.0)
    r["radius"][[1, 4]] *= -1.0  # inverted boxes
    r["style"][1] = A.RT_SPHERE_GLASS
    return r, None


def _tiny_radii():
    r = random_spheres(8, 6, 3.0)
    r["radius"][:6] = [0.0, -0.0, 9e-9, -9e-9, 2e-8, -2e-8]  # either side of Float.compare's 1e-8
    return r, None


def _ior_styles():
    r = random_spheres(6, 7, 3.0)
    r["style"] = [A.RT_SPHERE_DIELECTRIC, A.RT_SPHERE_GLASS] * 3
    r["ior"] = [1.5, 1.5, 1.0 / 1.5, 1.0 / 1.5, 1.0, 2.4]
    return r, None


def _counted(n_spheres, n_planes=0, seed=9):
    def make():
        r = random_spheres(n_spheres, seed, 60.0)
        if n_planes:
            r = np.concatenate([r, planes(np.zeros((n_planes, 3)) + np.arange(n_planes)[:, None], (0.0, 0.0, 1.0))])
        return r, None
    return make


PEEL_DEPTH = 53


def _peel():
    """64 identical spheres of radius 0.5 (tests/walk_tree_cases.py `peel`): every split of a sweep costs the same, so the surface-area build
    peels one box per level down to depth 48 and halves from there -- PEEL_DEPTH levels, the deep, unbalanced end of the depth scan and of
    the order by depth (tests/test_scene_device_host.py holds the case to that depth)."""
    return spheres(np.tile([1.0, 2.0, 3.0], (64, 1)), 0.5), None


def _earth():
    """tests/scenes.py earth_thumb: an image texture with its texels"""
    return from_objects(scenes.earth_thumb(scenes.golden("earthmap_rgb")["rgb"])[0])


def _radius(r_big):
    def make():
        r = random_spheres(5, 12, 2.0)
        r["radius"][2] = r_big
        return r, None
    return make


def _coordinate(x):
    def make():
        r = random_spheres(5, 13, 2.0)
        r["point"][3] = (x, 0.0, 0.0)
        r["radius"][3] = 0.25
        return r, None
    return make


def _infinite_radius():
    r = random_spheres(5, 14, 2.0)
    r["radius"][1] = np.inf  # ordered but not finite: the reference tree is walked
    return r, None


def _nan_centre():
    r = random_spheres(5, 15, 2.0)
    r["point"][2, 1] = np.nan  # no order: the host's ground
    return r, None


def _all_materials():
    return from_objects(scenes.all_materials()[0])


def _final():
    return from_objects(scenes.small_final()[0])  # 485 objects


def _many():
    return from_objects(scenes.many_spheres()[0])


def _random(seed):
    return lambda: from_objects(scenes.random_scene(seed)[0])


CASES = {
    "empty": lambda: (np.zeros(0, DT), None),
    "planes-only": lambda: (planes([[0, -1, 0], [0, 0, 9], [4, 0, 0]], [[0, 1, 0], [0, 0, -1], [-1, 0, 0]]), None),
    "spheres-1": lambda: (random_spheres(1, 1), None),
    "spheres-2": lambda: (random_spheres(2, 1), None),
    "spheres-3": lambda: (random_spheres(3, 1), None),
    "all-materials": _all_materials,
    "final-485": _final,
    "many-spheres": _many,
    "random-3": _random(3),
    "random-8": _random(8),
    "interleaved": _interleaved,
    "flipped": _flipped,
    "tiny-radii": _tiny_radii,
    "ior-styles": _ior_styles,
    "objects-16383": _counted(5000, 11383),
    "objects-16384": _counted(5000, 11384),
    "spheres-1026": _counted(1026),
    "spheres-2049": _counted(2049),
    "spheres-4097": _counted(4097),
    "peel-64": _peel,
    "earth-thumb": _earth,
    "radius-100": _radius(100.0),
    "radius-above-100": _radius(np.nextafter(100.0, np.inf)),
    "coordinate-1000": _coordinate(999.75),       # the box reaches 1000.0 exactly
    "coordinate-beyond-1000": _coordinate(999.76),
    "infinite-radius": _infinite_radius,
    "nan-centre": _nan_centre,
}
RENDERED = ("all-materials", "final-485", "interleaved", "flipped", "spheres-1026", "objects-16384")


def _bad(field, index, value, n=9, second=None):
    def make():
        r = random_spheres(n, 21, 3.0)
        r[field][index] = value
        if second is not None:
            f2, i2, v2 = second
            r[f2][i2] = v2
        return r, None
    return make


def _texture_on_pixel_style():
    rec, tex = from_objects(scenes.all_materials()[0])
    rec = rec.copy()
    cap = int(np.flatnonzero((rec["kind"] == A.RT_HITTABLE_SPHERE) & (rec["style"] == A.RT_SPHERE_LIGHT_SOURCE_CAP))[0])
    rec["texture"][cap] = 0
    return rec, tex


def _too_many_textures():
    t = (A.rt_texture * 255)()
    for r in t:
        r.kind, r.even, r.odd, r.map_radius = A.RT_TEXTURE_COLOUR, -1, -1, 1.0
    return random_spheres(4, 22), (t, 255, [])


REFUSALS = {
    "bad-kind-at-5": _bad("kind", 5, 7),
    "two-bad-smaller-wins": _bad("style", 6, 9, second=("kind", 2, 3)),
    "bad-style": _bad("style", 3, 7),
    "bad-plane-style": lambda: (np.concatenate([random_spheres(3, 23), planes([[0, 0, 0]], [[0, 1, 0]], style=4)]), None),
    "texture-out-of-range": _bad("texture", 4, 0),
    "kind-and-texture-on-one": _bad("texture", 1, 5, second=("kind", 1, 9)),
    "texture-on-pixel-style": _texture_on_pixel_style,
    "textures-255": _too_many_textures,
}


# ---- the routes, from records ----
def create(entry, records, textures=None, walk_tree=None, device=None):
    """rt_scene_create_ex / rt_scene_create_gpu_tree(s) (with `device`) from records -> (status, rt.Scene or None, rt_last_error())"""
    import ctypes as C
    tex, ntex, keep = textures or (None, 0, [])
    opt = None if walk_tree is None else A.rt_scene_options({"sah": A.RT_WALK_TREE_SAH, "reference": A.RT_WALK_TREE_REFERENCE}[walk_tree])
    out = C.c_void_p()
    rec = np.ascontiguousarray(records)
    ptr = rec.ctypes.data_as(C.POINTER(A.rt_hittable)) if len(rec) else None
    args = [ptr, len(rec), tex, ntex, C.byref(opt) if opt is not None else None] + ([] if device is None else [int(device)]) + [C.byref(out)]
    code = getattr(rt.lib, entry)(*args)
    return code, (rt.Scene(out.value, list(keep)) if code == A.RT_OK else None), (rt.lib.rt_last_error() or b"").decode()


def digest(*arrays):
    import hashlib
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()


def scene_record(scene):
    """What the getters expose of a scene, as recorded in tests/golden/scene_images_parent.json: rt_scene_get_info, and digests of
    rt_scene_get_filter_tree and rt_scene_get_walk_tree (Branch boxes with either zero as +0.0)."""
    fb, fl = scene.filter_tree()
    skip, prim, boxes = scene.walk_tree()
    return {"info": {k: int(v) for k, v in scene.info().items()}, "filter_tree": digest(fb, fl), "walk_tree": digest(skip, prim, boxes + 0.0)}
