"""Footprints (Scene.renderFootprints) for the tests and their expected values, composed from what the oracle already has: the
stream state of (seed, stream_base + i, s), FloatProducer.GetTwo, the footprint's vector in numpy float64 -- every product and sum
rounded on its own -- orc.ray_make, one batched OracleScene.trace_ray, and Scene.renderPixel's rule in integers as
fsharp_literal.render_pixel applies it (mean = //, difference = L1)."""
import math

import numpy as np

from fsharp_literal import FloatProducer


def equirect(width, height, eye):
    """A 360-degree panorama from `eye`, [width * height, 12]: pixel (row, col) spans longitude col .. col+1 of `width` over
    [-pi, pi) and latitude row .. row+1 of `height` from +pi/2 down; base is the direction of its corner, du and dv the direction
    differences to the next column and row, so that samples jitter inside the pixel."""
    def direction(row, col):
        lon = col * (2.0 * math.pi / width) - math.pi
        lat = 0.5 * math.pi - row * (math.pi / height)
        return np.stack([np.cos(lat) * np.sin(lon), np.sin(lat), np.cos(lat) * np.cos(lon)], axis=-1)

    row, col = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    base = direction(row, col)
    du = direction(row, col + 1.0) - base
    dv = direction(row + 1.0, col) - base
    origin = np.broadcast_to(np.asarray(eye, np.float64), base.shape)
    return np.ascontiguousarray(np.concatenate([origin, base, du, dv], axis=-1).reshape(-1, 12))


def pinhole(camera, max_w, max_h):
    """The footprints of a Camera record's own pixels, [(2 max_h + 1) * (2 max_w + 1), 12], rows top first as a frame has them:
    origin = eye, base = xo + xd * (col * vw / max_w) + yd * (row * vh / max_h) - eye, du = xd * vw / max_w, dv = yd * vh / max_h."""
    c = camera.to_abi()
    eye, xo, xd, yd = (np.array(v[:], np.float64) for v in (c.view_origin, c.xaxis_origin, c.xaxis_dir, c.yaxis_dir))
    vw, vh = c.viewport_width, c.viewport_height
    out = []
    for r in range(2 * max_h + 1):
        row = max_h - r - 1
        for col in range(-max_w, max_w + 1):
            base = xo + xd * (col * vw / max_w) + yd * (row * vh / max_h) - eye
            out.append(np.concatenate([eye, base, xd * vw / max_w, yd * vh / max_h]))
    return np.ascontiguousarray(np.array(out, np.float64))


class Composed:
    """accum [n, 4] int32, rgb [n, 3] uint8, early (pixels whose two means agree), and the samples that were taken: raw rays
    [m, 6] (origin, vector) with their generator states after GetTwo [m, 4], in no particular order."""

    def __init__(self, accum, rgb, early, rays, states):
        self.accum, self.rgb, self.early, self.rays, self.states = accum, rgb, early, rays, states


def compose(orc, oracle_scene, footprints, spp, depth, seed, stream_base=0, index=None):
    """What rt_render_footprints must give for `footprints`; index: the pixels' list indices (default 0 .. n-1), so that a subset
    of a long list can be composed on its own."""
    fp = np.asarray(footprints, np.float64).reshape(-1, 12)
    n = len(fp)
    index = np.arange(n, dtype=np.uint64) if index is None else np.asarray(index, np.uint64)
    k = min(5, spp // 2)
    n1 = 2 * k + 1
    n2 = max(spp - n1, 0)
    total = n1 + n2
    pixel = np.repeat(index + np.uint64(stream_base), total)
    sample = np.tile(np.arange(total, dtype=np.uint32), n)
    states = orc.stream_state(seed, pixel, sample)
    r = np.zeros((n * total, 2), np.float64)
    for j, s in enumerate(states):
        g = FloatProducer(*(int(x) for x in s))
        r[j] = g.GetTwo()
        states[j] = (g.x, g.y, g.z, g.w)
    f = np.repeat(fp, total, axis=0)
    r1, r2 = r[:, 0:1], r[:, 1:2]
    vector = (f[:, 3:6] + r1 * f[:, 6:9]) + r2 * f[:, 9:12]
    raw = np.concatenate([f[:, 0:3], vector], axis=1)
    made = np.zeros((n * total, 6), np.float64)
    ok = np.zeros(n * total, bool)
    for j in range(n * total):
        m = orc.ray_make(raw[j, :3], raw[j, 3:])
        if m is not None:
            ok[j] = True
            made[j] = m
    colour = np.zeros((n * total, 3), np.int64)  # Ray.make' gave ValueNone: Black
    if ok.any():
        colour[ok] = oracle_scene.trace_ray(depth, made[ok], states[ok])[0]
    colour = colour.reshape(n, total, 3)
    first, both = colour[:, :k + 1].sum(axis=1), colour[:, :n1].sum(axis=1)
    difference = np.abs(both // n1 - first // (k + 1)).sum(axis=1)
    early = difference == 0
    go_on = ~early & (n2 > 0)
    count = np.where(go_on, n1 + n2, n1)
    sums = np.where(go_on[:, None], colour.sum(axis=1), both)
    accum = np.concatenate([count[:, None], sums], axis=1).astype(np.int32)
    rgb = (sums // count[:, None]).astype(np.uint8)
    taken = (np.arange(total)[None, :] < count[:, None]).reshape(-1)
    return Composed(accum, rgb, early, raw[taken], states[taken])
