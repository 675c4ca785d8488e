"""What rt_camera_hits must answer, composed from the oracle's own pieces and never from the library: for list entry g and sample s

    state = orc.stream_state(seed, g, s);  (r1, r2) = orc.float_producer(state, 2)            -- the stream keyed (seed, g, s), GetTwo
    landingPoint = ((float col + r1) * vw) / float maxW;  walkDistance = ((float row + r2) * vh) / float maxH   -- Scene.fs:131-137, in
                                                                                                 numpy float64, in the order written
    pointOnXAxis = orc.ray_walk_along((xo, xd), landingPoint);  endPoint = orc.ray_walk_along((pointOnXAxis, yd), walkDistance)
    ray = orc.ray_make(eye, endPoint - eye)                                                    -- Ray.make' (Scene.fs:142-143)
    OracleScene.hit_object(ray)                                                                -- Scene.hitObject, with its counters

with row = maxH - r - 1 and col = c - maxW for g = r * cols + c (Scene.fs:219,226)."""
from typing import NamedTuple

import numpy as np


class Expected(NamedTuple):
    hit: np.ndarray       # [n, n_samples] int32: index into the scene's objects, -1 none, -2 Ray.make' gave ValueNone
    strike: np.ndarray    # [n, n_samples, 3] float64, NaN where hit < 0
    rays: np.ndarray      # [n, n_samples, 6] float64: origin, unit direction; NaN where hit == -2
    counters: np.ndarray  # [n, n_samples, 2] int64: the oracle's box tests and primitive tests of the slot's hitObject (0 at -2)


def camera_rays(orc, cam_abi, max_w, max_h, seed, pixels, sample_first, n_samples):
    """The camera rays alone: [n, n_samples, 6] float64, NaN where Ray.make' gave ValueNone."""
    pixels = np.asarray(pixels, np.int64)
    cols = 2 * max_w + 1
    eye, xo, xd, yd = (tuple(float(x) for x in v) for v in (cam_abi.view_origin, cam_abi.xaxis_origin, cam_abi.xaxis_dir, cam_abi.yaxis_dir))
    vw, vh = np.float64(cam_abi.viewport_width), np.float64(cam_abi.viewport_height)
    n = len(pixels)
    g = np.repeat(pixels, n_samples)
    s = np.tile(np.arange(sample_first, sample_first + n_samples, dtype=np.int64), n)
    states = orc.stream_state(seed, g.astype(np.uint64), s.astype(np.uint32))
    out = np.full((n * n_samples, 6), np.nan)
    eye_v = np.array(eye, np.float64)
    with np.errstate(all="ignore"):
        for i in range(n * n_samples):
            r, c = divmod(int(g[i]), cols)
            row, col = max_h - r - 1, c - max_w
            r1, r2 = orc.float_producer(states[i], 2)
            landing = ((np.float64(col) + r1) * vw) / np.float64(max_w)
            on_x = orc.ray_walk_along(xo + xd, float(landing))
            walk = ((np.float64(row) + r2) * vh) / np.float64(max_h)
            end = orc.ray_walk_along(tuple(on_x) + yd, float(walk))
            made = orc.ray_make(eye, tuple(np.array(end, np.float64) - eye_v))
            if made is not None:
                out[i] = made
    return out.reshape(n, n_samples, 6)


def compose(orc, oracle_scene, cam_abi, max_w, max_h, seed, pixels, sample_first=0, n_samples=1) -> Expected:
    rays = camera_rays(orc, cam_abi, max_w, max_h, seed, pixels, sample_first, n_samples)
    n = rays.shape[0]
    flat = rays.reshape(-1, 6)
    ok = ~np.isnan(flat[:, 0])
    hit = np.full(len(flat), -2, np.int32)
    strike = np.full((len(flat), 3), np.nan)
    counters = np.zeros((len(flat), 2), np.int64)
    if ok.any():
        h, sp, c = oracle_scene.hit_object(flat[ok])
        hit[ok], strike[ok], counters[ok] = h, sp, c
    strike[hit < 0] = np.nan
    out = Expected(hit.reshape(n, n_samples), strike.reshape(n, n_samples, 3), rays, counters.reshape(n, n_samples, 2))
    for a in out:
        a.setflags(write=False)
    return out


def same_f64(a, b):
    """Bit for bit, NaNs compared by position."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))
