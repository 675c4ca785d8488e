"""Small seeded scenes shared by the parity tests: every material, planes, textures, negative radii."""
import dataclasses

import numpy as np

import ray_tracing_fsharp_amd as rt
from ray_tracing_fsharp_amd import sample_images as si

P, V = rt.Point.make, rt.Vector.make
S, PS, H = rt.SphereStyle, rt.InfinitePlaneStyle, rt.Hittable
Tex = rt.Texture.Colour
Px = rt.Pixel


def unit(x, y, z):
    return rt.Vector.unitise(V(x, y, z))


def checker_image(h=16, w=32, seed=5):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def all_materials(spp=24, depth=12, pixels=20):
    """Every SphereStyle and InfinitePlaneStyle, bounded + unbounded, a hollow (negative radius) unbounded shell,
    a checkered UV-ramp texture, an image texture on a light; 16:9 like the reference's small scenes."""
    aspect = 16.0 / 9.0
    cam = dataclasses.replace(rt.Camera.makeBasic(spp, 1.0, aspect, P(0.0, 0.3, -1.0), unit(0.0, -0.05, 1.0), V(0.0, 1.0, 0.0)), BounceDepth=depth)
    chk = rt.ParameterisedTexture.Checkered(rt.ParameterisedTexture.UvRamp("u", 0, "v"), rt.ParameterisedTexture.UvRamp(100, "u", "v"), 50.0)
    img = rt.ParameterisedTexture.Image(checker_image())
    objs = [
        H.Sphere(rt.Sphere.make(S.LambertReflection(0.9, Tex(Px(25, 50, 120))), P(0.0, 0.0, 1.0), 0.5)),
        H.Sphere(rt.Sphere.make(S.PureReflection(0.95, rt.ParameterisedTexture.toTexture((0.5, P(1.1, 0.0, 1.0)), chk)), P(1.1, 0.0, 1.0), 0.5)),
        H.Sphere(rt.Sphere.make(S.Glass(0.95, Tex(rt.Colour.White), 1.5), P(-1.1, 0.0, 1.0), 0.5)),
        H.UnboundedSphere(rt.Sphere.make(S.Glass(1.0, Tex(rt.Colour.White), 1.0 / 1.5), P(-1.1, 0.0, 1.0), -0.4)),
        H.Sphere(rt.Sphere.make(S.FuzzedReflection(0.8, Tex(Px(255, 100, 0)), 0.3), P(0.5, 0.9, 1.6), 0.35)),
        H.Sphere(rt.Sphere.make(S.Dielectric(0.9, Tex(Px(200, 255, 200)), 1.4, 0.7), P(-0.5, 0.9, 1.6), 0.35)),
        H.Sphere(rt.Sphere.make(S.LightSourceCap(Px(255, 240, 200)), P(0.0, 1.9, 1.2), 0.4)),
        H.Sphere(rt.Sphere.make(S.LightSource(rt.ParameterisedTexture.toTexture((0.3, P(1.6, 1.2, 2.0)), img)), P(1.6, 1.2, 2.0), 0.3)),
        H.Sphere(rt.Sphere.make(S.Glass(1.0, Tex(rt.Colour.White), 1.5), P(0.2, -0.1, 0.2), -0.15)),  # bounded negative radius: never hit
        H.InfinitePlane(rt.InfinitePlane.make(PS.FuzzedReflection(0.85, Px(255, 200, 200), 0.4), P(0.0, -0.5, 0.0), unit(0.0, 1.0, 0.0))),
        H.InfinitePlane(rt.InfinitePlane.make(PS.PureReflection(0.8, rt.Colour.White), P(0.0, 0.0, 4.0), unit(0.3, 0.0, -1.0))),
        H.InfinitePlane(rt.InfinitePlane.make(PS.LambertReflection(0.7, Px(120, 220, 120)), P(-3.0, 0.0, 0.0), unit(1.0, 0.0, 0.0))),
        H.InfinitePlane(rt.InfinitePlane.make(PS.LightSource(Tex(Px(90, 90, 160))), P(0.0, 0.0, -5.0), unit(0.0, 0.0, 1.0))),
        H.UnboundedSphere(rt.Sphere.make(S.LightSource(Tex(Px(200, 200, 200))), P(0.0, 0.0, 0.0), 200.0)),
    ]
    return objs, cam, int(aspect * float(pixels)), pixels


def small_final(seed=7, spp=40, depth=50, pixels=16):
    """The RTIOW final scene (config 3) at thumbnail size: same geometry and tree, few pixels."""
    return si.config3_final(seed=seed, spp=spp, depth=depth, pixels=pixels)


def random_rays(n, seed, origin_scale=3.0):
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(n, 3)) * origin_scale
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], axis=1)


def earth_thumb(earthmap_rows_top_first, spp=30, pixels=18):
    """SampleImages.earth (SampleImages.fs:962-1010) at thumbnail size, with the committed decoded texels."""
    objs, cam, w, h = si.earth(earthmap_rows_top_first)
    cam = dataclasses.replace(cam, SamplesPerPixel=spp)
    aspect = 16.0 / 9.0
    return objs, cam, int(aspect * float(pixels)), pixels


def golden(name):
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))


def many_spheres(n=2600, seed=11, spp=12, depth=8, pixels=10):
    """A scene whose flattened image (about 136 B per sphere) exceeds the 160 KiB LDS budget, so rt_render must take the
    global-memory variant of the kernel.  Mixed materials, a Lambert floor and a light dome."""
    rng = np.random.default_rng(seed)
    aspect = 16.0 / 9.0
    cam = dataclasses.replace(rt.Camera.makeBasic(spp, 1.0, aspect, P(0.0, 1.5, -6.0), unit(0.0, -0.2, 1.0), V(0.0, 1.0, 0.0)), BounceDepth=depth)
    objs = []
    for i in range(n):
        c = P(float(rng.uniform(-8, 8)), float(rng.uniform(0.1, 3.0)), float(rng.uniform(-2, 14)))
        r = float(rng.uniform(0.05, 0.3))
        col = Px(*(int(x) for x in rng.integers(30, 256, 3)))
        k = i % 5
        st = (S.LambertReflection(float(rng.uniform(0.3, 1.0)), Tex(col)) if k < 2 else
              S.FuzzedReflection(float(rng.uniform(0.5, 1.0)), Tex(col), float(rng.uniform(0.0, 0.5))) if k == 2 else
              S.Glass(1.0, Tex(rt.Colour.White), 1.5) if k == 3 else S.PureReflection(0.9, Tex(col)))
        objs.append(H.Sphere(rt.Sphere.make(st, c, r)))
    objs.append(H.UnboundedSphere(rt.Sphere.make(S.LambertReflection(0.5, Tex(Px(200, 200, 200))), P(0.0, -1000.0, 0.0), 1000.0)))
    objs.append(H.UnboundedSphere(rt.Sphere.make(S.LightSource(Tex(Px(220, 220, 255))), P(0.0, 0.0, 0.0), 3000.0)))
    return objs, cam, int(aspect * float(pixels)), pixels


def random_scene(seed, pixels=6):
    """A small random scene for fuzzing: every style can appear, bounded or unbounded, radii of both signs, planes in any
    orientation, camera anywhere (possibly inside objects), textures now and then."""
    rng = np.random.default_rng(seed)
    u = lambda a, b: float(rng.uniform(a, b))  # noqa: E731
    col = lambda: Px(*(int(x) for x in rng.integers(0, 256, 3)))  # noqa: E731
    chk = rt.ParameterisedTexture.Checkered(rt.ParameterisedTexture.UvRamp("u", int(rng.integers(0, 256)), "v"),
                                            rt.ParameterisedTexture.Colour(col()), u(5.0, 60.0))

    def tex(c, r):
        if rng.random() < 0.15:
            return rt.ParameterisedTexture.toTexture((abs(r), c), chk)
        return Tex(col())

    objs = []
    for _ in range(int(rng.integers(1, 9))):
        c = P(u(-2, 2), u(-1, 2), u(0, 5))
        r = u(0.1, 1.2) * (-1.0 if rng.random() < 0.15 else 1.0)
        k = int(rng.integers(0, 7))
        st = [S.LightSource(tex(c, r)), S.LightSourceCap(col()), S.PureReflection(u(0, 1), tex(c, r)), S.FuzzedReflection(u(0, 1), tex(c, r), u(0, 1)),
              S.LambertReflection(u(0, 1), tex(c, r)), S.Dielectric(u(0, 1), tex(c, r), u(0.7, 2.0), u(0, 1)), S.Glass(u(0.5, 1), tex(c, r), u(0.7, 2.0))][k]
        objs.append((H.UnboundedSphere if rng.random() < 0.3 else H.Sphere)(rt.Sphere.make(st, c, r)))
    for _ in range(int(rng.integers(0, 3))):
        n = rng.normal(size=3)
        k = int(rng.integers(0, 4))
        st = [PS.LightSource(Tex(col())), PS.PureReflection(u(0, 1), col()), PS.LambertReflection(u(0, 1), col()), PS.FuzzedReflection(u(0, 1), col(), u(0, 1))][k]
        objs.append(H.InfinitePlane(rt.InfinitePlane.make(st, P(u(-3, 3), u(-3, 3), u(-3, 6)), unit(*n))))
    if rng.random() < 0.7:
        objs.append(H.UnboundedSphere(rt.Sphere.make(S.LightSource(Tex(col())), P(0.0, 0.0, 0.0), u(20.0, 300.0))))
    rng.shuffle(objs)
    d = rng.normal(size=3)
    cam = dataclasses.replace(rt.Camera.makeBasic(int(rng.integers(1, 30)), u(0.5, 3.0), u(0.8, 2.0), P(u(-1, 1), u(-0.5, 1.5), u(-3, 1)), unit(*d), V(0.0, 1.0, 0.05)),
                              BounceDepth=int(rng.integers(0, 25)))
    return list(objs), cam, int(rng.integers(2, pixels + 1)), int(rng.integers(2, pixels + 1))


def free_camera(eye, xaxis_origin, xd, yd, vw, vh, spp, depth):
    """A Camera record (Camera.fs:3-28) filled in by hand, as an F# caller may build it: any eye, any viewport origin, any two unit
    axes (not necessarily orthogonal, either handedness).  Scene.traceOnce reads only the eye, ViewportXAxis, the direction of
    ViewportYAxis and the viewport's size (Scene.fs:129-144); View.Vector and FocalLength are set but unused.  xd and yd are
    unitised here (UnitVector in F#)."""
    from ray_tracing_fsharp_amd import _abi as A
    xd, yd = (np.asarray(v, np.float64) / np.sqrt(np.dot(np.asarray(v, np.float64), np.asarray(v, np.float64))) for v in (xd, yd))
    a = A.rt_camera()
    a.view_origin[:] = [float(x) for x in eye]
    n = np.cross(xd, yd)
    nn = float(np.sqrt(np.dot(n, n)))
    a.view_dir[:] = [float(x) for x in (n / nn if nn > 0 else xd)]
    a.xaxis_origin[:] = [float(x) for x in xaxis_origin]
    a.xaxis_dir[:] = [float(x) for x in xd]
    a.yaxis_origin[:] = [float(x) for x in xaxis_origin]
    a.yaxis_dir[:] = [float(x) for x in yd]
    a.viewport_width, a.viewport_height = float(vw), float(vh)
    a.focal_length = 1.0
    a.samples_per_pixel, a.bounce_depth = int(spp), int(depth)
    return rt.Camera(a, SamplesPerPixel=int(spp), BounceDepth=int(depth))


def _point_segment_distance(p, a, b):
    ab = b - a
    den = float(np.dot(ab, ab))
    t = 0.0 if den == 0.0 else min(1.0, max(0.0, float(np.dot(p - a, ab)) / den))
    return float(np.linalg.norm(p - (a + t * ab)))


def viewport_distance(camera, max_w, max_h):
    """Distance from the eye to the part of the viewport that the image's camera rays go through: the parallelogram
    xo + lx * xd + ly * yd with lx in [-maxW, maxW + 1] * vw / maxW and ly in [-maxH - 1, maxH] * vh / maxH (Scene.fs:129-144;
    row = maxH - r - 1, col = c - maxW)."""
    a = camera.abi
    eye, xo, xd, yd = (np.array(list(v), np.float64) for v in (a.view_origin, a.xaxis_origin, a.xaxis_dir, a.yaxis_dir))
    lx = np.array([-max_w, max_w + 1], np.float64) * a.viewport_width / max_w
    ly = np.array([-max_h - 1, max_h], np.float64) * a.viewport_height / max_h
    corner = lambda i, j: xo + xd * lx[i] + yd * ly[j]  # noqa: E731
    c = [corner(0, 0), corner(1, 0), corner(1, 1), corner(0, 1)]
    best = min(_point_segment_distance(eye, c[q], c[(q + 1) % 4]) for q in range(4))
    # the interior: the foot of the perpendicular from the eye onto the viewport's plane, if it falls inside the parallelogram
    g = np.array([[xd @ xd, xd @ yd], [xd @ yd, yd @ yd]])
    if abs(np.linalg.det(g)) > 1e-12:
        u, v = np.linalg.solve(g, np.array([xd @ (eye - xo), yd @ (eye - xo)]))
        if lx[0] <= u <= lx[1] and ly[0] <= v <= ly[1]:
            best = min(best, float(np.linalg.norm(xo + xd * u + yd * v - eye)))
    return best


def require_clear_eye(camera, max_w, max_h, clearance=1e-3):
    """Refuses a camera whose viewport patch comes within `clearance` of the eye: closer than 1e-4 Ray.make' returns ValueNone
    and the reference throws (Scene.fs:142-144)."""
    d = viewport_distance(camera, max_w, max_h)
    if not d >= clearance:
        raise ValueError(f"the viewport passes {d:.3g} from the eye")
    return camera


def raw_scene_pair(orc, hs, n, tex, ntex, keep):
    """(rt.Scene, OracleScene) from the ABI arrays themselves -- for scenes the host mirror cannot express (texture records with
    shared children, chosen record numbers); both sides are handed the same bytes.  orc=None: the product scene alone."""
    import ctypes as C
    from ray_tracing_fsharp_amd._lib import check
    out = C.c_void_p()
    check(rt.lib.rt_scene_create(hs, n, tex, ntex, C.byref(out)))
    s = rt.Scene(out.value, keep)
    if orc is None:
        return s, None
    o = object.__new__(orc.OracleScene)
    o._keep = keep
    h = C.c_void_p()
    orc._check(orc.lib.orc_scene_create(hs, n, tex, ntex, C.byref(h)))
    o._h = h
    return s, o
