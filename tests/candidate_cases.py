"""Cameras built to sit where the timed kernel's per-pixel candidate walk (pixel_candidates, csrc/rt_device.h) is most likely to go
wrong, and a bit-exact numpy model of that walk.  Shared by tests/test_candidates_model.py (the model against the oracle's exact
BoundingBox.hits) and tests/test_gpu_candidates.py (the device's candidates against the model, and renders).

The property under test is ONE inclusion, for every pixel whose rays do not walk the tree: the Leaves whose boxes some camera ray
of the pixel hits (BoundingBox.fs:30-94, exactly) are among the pixel's candidates.  Camera.makeBasic gives every pixel a pyramid
whose corners all lie in front of the plane through the eye normal to their sum; the cameras here (Camera records filled in by
hand, as an F# caller may build them) do not.
"""
import dataclasses

import numpy as np

import ray_tracing_fsharp_amd as rt
import scenes

F32 = np.float32
P = rt.Point.make
S, H, Tex, Px = rt.SphereStyle, rt.Hittable, rt.Texture.Colour, rt.Pixel

# the jitters of a pixel's test rays: the 4 corners and 4 edge midpoints of its patch (FloatProducer reaches 0 and 1), then random
CORNER_JITTER = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0], [0.5, 0.0], [1.0, 0.5], [0.5, 1.0], [0.0, 0.5]])


def all_pixels(max_w, max_h):
    """(row, col) of every pixel of the image in the reference's coordinates (row = maxH - r - 1, col = c - maxW)."""
    r, c = np.meshgrid(np.arange(2 * max_h + 1), np.arange(2 * max_w + 1), indexing="ij")
    return np.stack([(max_h - r - 1).ravel(), (c - max_w).ravel()], axis=1).astype(np.int32)


def camera_arrays(cam):
    a = cam.abi
    return (np.array(list(a.view_origin), np.float64), np.array(list(a.xaxis_origin), np.float64), np.array(list(a.xaxis_dir), np.float64),
            np.array(list(a.yaxis_dir), np.float64), float(a.viewport_width), float(a.viewport_height))


def camera_rays(cam, max_w, max_h, row_col, jitter):
    """[n_pixels, n_jitter, 6] camera rays with Scene.traceOnce's arithmetic (Scene.fs:129-144), the direction unitised as
    Vector.unitise does it (1 / sqrt |v|^2, then the product)."""
    eye, xo, xd, yd, vw, vh = camera_arrays(cam)
    rows = row_col[:, 0].astype(np.float64)[:, None]
    cols = row_col[:, 1].astype(np.float64)[:, None]
    lx = ((cols + jitter[None, :, 0]) * vw) / float(max_w)
    ly = ((rows + jitter[None, :, 1]) * vh) / float(max_h)
    end = (xo + xd * lx[..., None]) + yd * ly[..., None]
    d = end - eye
    dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    d = d * (1.0 / np.sqrt(dd))[..., None]
    return np.concatenate([np.broadcast_to(eye, d.shape), d], axis=-1)


def reachable_leaves(orc, scene, cam, max_w, max_h, row_col, n_random=8, seed=0, chunk=200_000):
    """For every pixel: the hittable indices of the Leaves some of its test rays hit under the oracle's exact BoundingBox.hits
    (as a boolean [n_pixels, n_leaves] matrix over `leaf_ids`)."""
    _, prim, boxes = scene.walk_tree()
    leaf = prim >= 0
    lb = boxes[leaf][:, [0, 2, 4, 1, 3, 5]]  # (minx,maxx,miny,maxy,minz,maxz) -> (min xyz, max xyz)
    leaf_ids = prim[leaf]
    rng = np.random.default_rng(seed)
    jit = np.concatenate([CORNER_JITTER, rng.random((n_random, 2))])
    rays = camera_rays(cam, max_w, max_h, row_col, jit).reshape(-1, 6)
    n_l = len(lb)
    hit = np.zeros(len(rays) * n_l, bool)
    for s0 in range(0, len(hit), chunk):
        idx = np.arange(s0, min(len(hit), s0 + chunk))
        hit[idx] = orc.bbox_hits(rays[idx // n_l], lb[idx % n_l]).astype(bool)
    return hit.reshape(len(row_col), len(jit), n_l).any(axis=1), leaf_ids


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _f32(x):
    return np.asarray(x, np.float64).astype(F32)


def _outside_plane(n, c, h):
    """outside_plane (csrc/rt_device.h) in single precision, operation for operation (no fused multiply-adds)."""
    ax, ay, az = np.abs(n[0]), np.abs(n[1]), np.abs(n[2])
    s = ((n[0] * c[0] + n[1] * c[1]) + n[2] * c[2]) + ((ax * h[0] + ay * h[1]) + az * h[2])
    m = F32(2.0 ** -18) * ((ax * (np.abs(c[0]) + h[0]) + ay * (np.abs(c[1]) + h[1])) + az * (np.abs(c[2]) + h[2]))
    return s < -m


def pyramid(cam, max_w, max_h, row_col, legacy_gc=False):
    """The per-pixel set-up of pixel_candidates: the four side planes (float32 [4, 3, n]), the eye-plane normal (float32 [3, n]; zero
    where it is left out) and the pixels whose pyramid is degenerate.  Double precision, operation for operation as compiled
    with -ffp-contract=off.  legacy_gc: the eye plane always used (the kernel before the front-corner guard)."""
    eye, xo, xd, yd, vw, vh = camera_arrays(cam)
    rows = row_col[:, 0].astype(np.float64)
    cols = row_col[:, 1].astype(np.float64)
    g = []
    for q in range(4):
        jx, jy = (1.0 if q in (1, 2) else 0.0), (1.0 if q >= 2 else 0.0)
        lx = ((cols + jx) * vw) / float(max_w)
        ly = ((rows + jy) * vh) / float(max_h)
        g.append([((xo[a] + xd[a] * lx) + yd[a] * ly) - eye[a] for a in range(3)])
    gc = [(g[0][a] + g[1][a]) + (g[2][a] + g[3][a]) for a in range(3)]

    def dot(u, v):
        return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]

    if legacy_gc:
        front = np.ones(len(rows), bool)
    else:
        front = np.ones(len(rows), bool)
        for q in range(4):
            scale = (np.abs(g[q][0] * gc[0]) + np.abs(g[q][1] * gc[1])) + np.abs(g[q][2] * gc[2])
            front &= dot(g[q], gc) > 2.0 ** -30 * scale
    gcf = np.stack([_f32(np.where(front, gc[a], 0.0)) for a in range(3)])
    degenerate = np.zeros(len(rows), bool)
    n = np.zeros((4, 3, len(rows)), F32)
    for q in range(4):
        u, v = g[q], g[(q + 1) & 3]
        nq = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
        sgn = dot(nq, gc)
        degenerate |= ~(sgn != 0.0)
        with np.errstate(all="ignore"):
            sc1 = np.where(sgn < 0.0, -1.0, 1.0) / ((np.abs(nq[0]) + np.abs(nq[1])) + np.abs(nq[2]))
            for a in range(3):
                n[q, a] = _f32(sc1 * nq[a])
    return n, gcf, degenerate, front


def model(scene, cam, max_w, max_h, row_col, legacy_gc=False):
    """pixel_candidates over the scene's filter tree (Scene.filter_tree: the timed kernel's float32 records, links and hittables),
    vectorised over pixels, one node visit per step.  Returns (cand [n, 4] hittable indices in push order, -1 padded; walk [n] bool), as
    rt.hooks.pixel_candidates reports them (walk <=> its row starts with -2).  Fall-back to walking: a degenerate pyramid, more
    than four Leaves (16-bit queue entries: fewer than 16384 objects) or more than two (full-width entries)."""
    boxes, links = scene.filter_tree()
    info = scene.info()
    limit = 4 if info["n_bounded"] + info["n_unbounded"] < 16384 else 2
    row_col = np.asarray(row_col, np.int32).reshape(-1, 2)
    npx = len(row_col)
    with np.errstate(all="ignore"):
        n, gcf, degenerate, _ = pyramid(cam, max_w, max_h, row_col, legacy_gc)
        eye = camera_arrays(cam)[0]
        lo, hi = boxes[:, 0::2].astype(F32), boxes[:, 1::2].astype(F32)
        c = ((0.5 * (lo.astype(np.float64) + hi.astype(np.float64))) - eye).astype(F32)  # [nodes, 3]
        h = F32(0.5) * np.abs(hi - lo) + F32(1e-30)
        h = h + F32(2.0 ** -22) * (np.abs(lo) + np.abs(hi))
        cand = np.full((npx, 4), -1, np.int32)
        count = np.zeros(npx, np.int32)
        walk = degenerate.copy()
        off = np.where(walk, len(boxes), 0)
        idx = np.flatnonzero(off < len(boxes))
        while idx.size:  # one node visit per pixel per step (the records are in depth order: a walk jumps back and forth)
            k = off[idx]
            ck, hk = c[k].T, h[k].T
            miss = np.zeros(idx.size, bool)
            for q in range(4):
                miss |= _outside_plane(n[q][:, idx], ck, hk)
            miss |= _outside_plane(gcf[:, idx], ck, hk)
            off[idx] = np.where(miss, links[k, 1], links[k, 0])
            leaf = ~miss & (links[k, 2] != 0)
            take, obj = idx[leaf], links[k[leaf], 4]
            over = count[take] >= limit
            walk[take[over]] = True
            off[take[over]] = len(boxes)
            take, obj = take[~over], obj[~over]
            cand[take, count[take]] = obj
            count[take] += 1
            idx = idx[off[idx] < len(boxes)]
    cand[walk] = -1
    return cand, walk


# ---- scenes and cameras -----------------------------------------------------------------------------------------------------
def _lambert(c, r, col=(200, 120, 80)):
    return H.Sphere(rt.Sphere.make(S.LambertReflection(0.8, Tex(Px(*col))), P(*(float(x) for x in c)), float(r)))


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def spheres_on_pixel_rays(rng, cam, max_w, max_h, n, dist, rad):
    """n spheres centred on rays through the corners, edge points and interiors of random pixels (and just outside them), at
    distances `dist` (a range) from the eye, radii `rad` times that distance."""
    row_col = all_pixels(max_w, max_h)
    pick = row_col[rng.integers(0, len(row_col), n)]
    jit = np.where(rng.random((n, 2)) < 0.6, rng.integers(0, 2, (n, 2)).astype(np.float64), rng.uniform(-0.2, 1.2, (n, 2)))
    objs = []
    for i in range(n):
        r = camera_rays(cam, max_w, max_h, pick[i:i + 1], jit[i:i + 1])[0, 0]
        t = float(np.exp(rng.uniform(np.log(dist[0]), np.log(dist[1]))))
        objs.append(_lambert(r[:3] + r[3:] * t, t * float(rng.uniform(*rad)), tuple(int(x) for x in rng.integers(30, 256, 3))))
    return objs


def _frame(rng, eye, f, ratio, max_w, max_h, fx, fy, rotate=True, yd_angle=90.0, mirror=False, behind=False):
    """A viewport at distance f from the eye, normal along the frame's z, the perpendicular's foot moved off the pixel grid by the
    fractions (fx, fy) of a pixel; vw = ratio * f.  Optionally rotated, sheared (angle between the axes), mirrored, behind."""
    rot = _rotation(rng) if rotate else np.eye(3)
    vw = ratio * f
    vh = vw * float(rng.uniform(0.5, 1.5)) if rotate else vw
    pw, ph = vw / max_w, vh / max_h
    ex, ez = rot[:, 0], rot[:, 2]
    a = np.radians(yd_angle)
    ey = rot @ np.array([np.cos(a), np.sin(a), 0.0])
    if mirror:
        ey = -ey
    normal = -ez if behind else ez
    xo = eye + normal * f - ex * (fx * pw) - ey * (fy * ph)
    return xo, ex, ey, vw, vh


def family_off_centre(seed=1):
    """(a) the perpendicular's foot off the pixel grid by 1/4, 1/3, 1e-6 and 1 - 1e-6 of a pixel, 1-3 coordinate images, vw / focal
    from 0.1 to 100 (single pixels subtend up to ~170 degrees), spheres on the pixels' corner rays near and far; and the example of
    the eye-plane hole: eye 0, axes x and y, vw = vh = 1, one coordinate, xaxis_origin (-0.25, -0.25, 0.05), a box of half extent
    0.2 on the corner ray of pixel (0, 0) at distance 10."""
    rng = np.random.default_rng(seed)
    cam = scenes.free_camera((0.0, 0.0, 0.0), (-0.25, -0.25, 0.05), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1.0, 1.0, 20, 5)
    g0 = np.array([-0.25, -0.25, 0.05])
    objs = [_lambert(g0 / np.linalg.norm(g0) * 10.0, 0.2)] + spheres_on_pixel_rays(rng, cam, 1, 1, 6, (1.0, 20.0), (0.005, 0.05))
    yield "example", objs, cam, 1, 1, all_pixels(1, 1)
    for frac in (0.25, 1.0 / 3.0, 1e-6, 1.0 - 1e-6):
        for ratio in (0.1, 1.0, 10.0, 100.0):
            mw, mh = int(rng.integers(1, 4)), int(rng.integers(1, 4))
            eye = rng.normal(size=3) * 2.0
            f = float(np.exp(rng.uniform(np.log(0.05), np.log(2.0))))
            xo, xd, yd, vw, vh = _frame(rng, eye, f, ratio, mw, mh, frac, frac * float(rng.choice([1.0, -1.0, 0.5])))
            cam = scenes.require_clear_eye(scenes.free_camera(eye, xo, xd, yd, vw, vh, 20, 5), mw, mh)
            objs = spheres_on_pixel_rays(rng, cam, mw, mh, 10, (0.5, 30.0), (0.003, 0.06))
            yield f"frac{frac:.3g}_ratio{ratio:g}", objs, cam, mw, mh, all_pixels(mw, mh)


def family_axes(seed=2):
    """(b) unit axes 5 to 175 degrees apart, mirrored handedness, a viewport behind the eye."""
    rng = np.random.default_rng(seed)
    for angle in (5.0, 30.0, 60.0, 120.0, 150.0, 175.0):
        for mirror, behind in ((False, False), (True, False), (False, True), (True, True)):
            mw, mh = int(rng.integers(1, 4)), int(rng.integers(1, 4))
            eye = rng.normal(size=3)
            f = float(rng.uniform(0.2, 2.0))
            ratio = float(np.exp(rng.uniform(np.log(0.1), np.log(30.0))))
            xo, xd, yd, vw, vh = _frame(rng, eye, f, ratio, mw, mh, float(rng.random()), float(rng.random()), yd_angle=angle, mirror=mirror, behind=behind)
            cam = scenes.require_clear_eye(scenes.free_camera(eye, xo, xd, yd, vw, vh, 20, 5), mw, mh)
            objs = spheres_on_pixel_rays(rng, cam, mw, mh, 10, (0.5, 20.0), (0.003, 0.05))
            yield f"angle{angle:g}_mirror{int(mirror)}_behind{int(behind)}", objs, cam, mw, mh, all_pixels(mw, mh)


def family_flat(seed=3):
    """(c) flat and near-flat pyramids: the eye exactly in the viewport's plane (axes x and y, plane z = 0.05, so the eye's z is
    exactly the plane's), then 1, 4 and 1000 ulps off it; xd parallel to yd; xd within 1e-12 rad of yd."""
    rng = np.random.default_rng(seed)
    z0 = 0.05
    for ulps in (0, 1, -1, 4, -4, 1000, -1000):
        ez = z0
        for _ in range(abs(ulps)):
            ez = float(np.nextafter(ez, np.inf if ulps > 0 else -np.inf))
        for mw, mh in ((1, 1), (2, 3)):
            eye = np.array([-3.5, 0.3, ez])  # left of the image, in (or next to) its plane
            cam = scenes.require_clear_eye(scenes.free_camera(eye, (0.0, 0.0, z0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1.0, 1.0, 20, 5), mw, mh)
            # spheres along the fan of rays, one in, just above, just below or above the plane
            # (few of them: a flat pyramid reaches everything in its plane, and more than four Leaves send the pixel to the walk)
            objs = spheres_on_pixel_rays(rng, cam, mw, mh, 2, (0.5, 20.0), (0.002, 0.03))
            objs.append(_lambert((float(rng.uniform(-2, 5)), float(rng.uniform(-2, 3)), z0 + float(rng.choice([0.0, 1e-9, -1e-9, 0.05]))), float(rng.uniform(0.01, 0.2))))
            yield f"in_plane_ulps{ulps:+d}_{mw}x{mh}", objs, cam, mw, mh, all_pixels(mw, mh)
    for tilt in (0.0, 1e-12, 1e-9):
        for k in range(2):
            mw, mh = int(rng.integers(1, 4)), int(rng.integers(1, 4))
            rot = _rotation(rng)
            xd = rot[:, 0]
            yd = np.cos(tilt) * rot[:, 0] + np.sin(tilt) * rot[:, 1]
            eye = rng.normal(size=3)
            xo = eye + rot[:, 2] * float(rng.uniform(0.3, 2.0)) - xd * 0.37
            cam = scenes.require_clear_eye(scenes.free_camera(eye, xo, xd, yd, float(rng.uniform(0.5, 3)), float(rng.uniform(0.5, 3)), 20, 5), mw, mh)
            objs = spheres_on_pixel_rays(rng, cam, mw, mh, 5, (0.5, 20.0), (0.002, 0.05))
            yield f"parallel_axes_tilt{tilt:g}_{k}", objs, cam, mw, mh, all_pixels(mw, mh)


def _cluster(rng, centre, n, spread, rad):
    return [_lambert(np.asarray(centre) + rng.normal(size=3) * spread, float(rng.uniform(*rad)), tuple(int(x) for x in rng.integers(30, 256, 3)))
            for _ in range(n)]


def family_eye(seed=4):
    """(d) the eye at distance 10, 990-1010 (across RTD_IMPLIED_DD = 1e6 = 1000^2), 1e4 and 1e6 from a small sphere field, and inside
    a sphere and inside a Branch box; off-grid viewports aimed at the field so that it covers a few pixels."""
    rng = np.random.default_rng(seed)
    for dist in (10.0, 990.0, 999.9, 1000.1, 1010.0, 1e4, 1e6):
        mw, mh = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        centre = rng.normal(size=3)
        objs = _cluster(rng, centre, 7, 0.6, (0.1, 0.5))
        rot = _rotation(rng)
        eye = centre - rot[:, 2] * dist
        f = float(rng.uniform(0.5, 2.0))
        vw = f * 3.0 / dist
        pw, ph = vw / mw, vw / mh
        xo = eye + rot[:, 2] * f - rot[:, 0] * (float(rng.random()) * pw) - rot[:, 1] * (float(rng.random()) * ph)
        cam = scenes.require_clear_eye(scenes.free_camera(eye, xo, rot[:, 0], rot[:, 1], vw, vw, 20, 5), mw, mh)
        yield f"dist{dist:g}", objs, cam, mw, mh, all_pixels(mw, mh)
    for inside in ("sphere", "branch"):
        for k in range(3):
            mw, mh = int(rng.integers(1, 4)), int(rng.integers(1, 4))
            objs = _cluster(rng, (0.0, 0.0, 0.0), 9, 1.0, (0.2, 0.6))
            if inside == "sphere":
                objs.append(_lambert((0.1, -0.05, 0.02), 0.8))
                eye = np.array([0.1, -0.05, 0.02]) + rng.normal(size=3) * 0.1
            else:  # between the spheres of the field: inside the boxes above them, outside every sphere
                eye = rng.normal(size=3) * 0.3
                objs = [o for o in objs if np.linalg.norm(np.array(list(o.sphere.Centre)) - eye) > abs(o.sphere.Radius) + 0.05]
            rot = _rotation(rng)
            f = float(rng.uniform(0.3, 1.0))
            xo, xd, yd, vw, vh = _frame(rng, eye, f, float(rng.uniform(0.5, 20.0)), mw, mh, float(rng.random()), float(rng.random()))
            cam = scenes.require_clear_eye(scenes.free_camera(eye, xo, xd, yd, vw, vh, 20, 5), mw, mh)
            yield f"inside_{inside}_{k}", objs, cam, mw, mh, all_pixels(mw, mh)


def family_controls(seed=5, npx=1500):
    """(e) the four Camera.makeBasic cameras of test_pixel_candidates_contain_every_leaf_a_camera_ray_can_hit, on sampled pixels."""
    rng = np.random.default_rng(seed)
    objs, cam, w, h = scenes.small_final(pixels=60)
    V = scenes.V
    low = dataclasses.replace(rt.Camera.makeBasic(10, 1.0, 1.5, P(-10.5, 0.3, 0.45), scenes.unit(1.0, -0.01, 0.0), V(0.0, 1.0, 0.0)), BounceDepth=5)
    axis = dataclasses.replace(rt.Camera.makeBasic(10, 2.0, 1.0, P(0.5, 30.0, 0.5), scenes.unit(0.0, -1.0, 0.0), V(0.0, 0.0, 1.0)), BounceDepth=5)
    objs2, cam2, w2, h2 = scenes.all_materials(pixels=40)
    for name, (o, c, mw, mh) in (("final", (objs, cam, w, h)), ("low", (objs, low, 45, 30)), ("axis", (objs, axis, 40, 40)), ("all_materials", (objs2, cam2, w2, h2))):
        rc = np.stack([rng.integers(-mh - 1, mh, npx), rng.integers(-mw, mw + 1, npx)], axis=1).astype(np.int32)
        yield name, o, c, mw, mh, rc


FAMILIES = {"off_centre": family_off_centre, "axes": family_axes, "flat": family_flat, "eye": family_eye, "controls": family_controls}


def free_camera_render_case(seed):
    """A render-sized case for the fuzz: random_scene-style objects around a free camera from one of the families (a)-(d), a
    1-4 coordinate image, 20-60 samples per pixel."""
    rng = np.random.default_rng(seed)
    fam = ["off_centre", "axes", "flat", "eye"][seed % 4]
    cases = list(FAMILIES[fam](seed=1000 + seed))
    name, objs, cam, mw, mh, _ = cases[int(rng.integers(0, len(cases)))]
    extra, ecam, _, _ = scenes.random_scene(seed)
    objs = list(objs) + [o for o in extra if o.kind != rt._abi.RT_HITTABLE_SPHERE or rng.random() < 0.5]
    mw, mh = min(max(mw, int(rng.integers(1, 5))), 4), min(max(mh, int(rng.integers(1, 5))), 4)
    cam = scenes.require_clear_eye(dataclasses.replace(cam, SamplesPerPixel=int(rng.integers(20, 61)), BounceDepth=int(rng.integers(2, 12))), mw, mh)
    return f"{fam}/{name}", objs, cam, mw, mh
