"""What rt_camera_paths / rt_trace_paths must answer, composed from the oracle's own pieces and never from the library.  A path is

    {Ray = ray; Colour = White};  while bounces <= maxCount:
        OracleScene.hit_object(ray)                                  -- Scene.hitObject; ValueNone: MISS, Black
        OracleScene.reflection(index, ray, colour, strike, rng)      -- Hittable.Reflection; absorbed != 0 is ValueSome c: STOPPED, c
        bounces += 1
    BOUNCE_LIMIT, HotPink                                            -- Scene.traceRay, Scene.fs:93-114

vectorised over the slots that are still alive.  A camera path starts with camera_hit_cases.camera_rays' ray and the generator of the
stream (seed, g, s) advanced by the two draws of GetTwo; a ray path with orc.ray_make of the caller's (origin, vector) and the caller's
state, or the stream (seed, stream_base + i, sample) from its beginning."""
import atexit
import functools
from typing import NamedTuple

import numpy as np

from camera_hit_cases import camera_rays, same_f64  # noqa: F401  (same_f64: NaN-aware bit equality, for the tests)

MISS, STOPPED, BOUNCE_LIMIT, NO_RAY = 0, 1, 2, 3
SUMMARY_WORDS = 16
WHITE, BLACK, HOTPINK = (255, 255, 255), (0, 0, 0), (205, 105, 180)  # Pixel.fs:61-66


class Paths(NamedTuple):
    """Flat over the slots; records [slots, K, ...] with K = the longest path of the batch (truncate() cuts or pads to a caller's K)."""
    n_vertices: np.ndarray    # [slots] int32
    end: np.ndarray           # [slots] int32
    colour: np.ndarray        # [slots, 3] uint8
    first_ray: np.ndarray     # [slots, 6] float64, NaN at NO_RAY
    rng: np.ndarray           # [slots, 4] uint32: the generator after the path
    hit_index: np.ndarray     # [slots, K] int32, -1 past the end
    strike: np.ndarray        # [slots, K, 3] float64, NaN past the end
    colour_after: np.ndarray  # [slots, K, 3] uint8, 0 past the end
    ray_after: np.ndarray     # [slots, K, 6] float64, NaN past the end and where Reflection gave ValueSome
    counters: np.ndarray      # [4] int64: hitObject calls, box tests, primitive tests, reflections


def xorshift_steps(state, steps):
    """`steps` steps of xorshift128 (Float.fs:14-47) on states [n, 4] uint32: what `steps` calls of Get() leave behind."""
    s = np.array(state, np.uint32).reshape(-1, 4).copy()
    for _ in range(steps):
        x, w = s[:, 0], s[:, 3]
        t = x ^ (x << np.uint32(11))
        nw = w ^ (w >> np.uint32(19)) ^ (t ^ (t >> np.uint32(8)))
        s = np.stack([s[:, 1], s[:, 2], s[:, 3], nw], 1).astype(np.uint32)
    return s


def trace(orc, oracle_scene, rays, rng, max_count, mutant=None):
    """Scene.traceRay for rays [n, 6] (NaN rows: Ray.make' gave ValueNone) and generator states [n, 4].  mutant: one of the three
    deliberate mistakes tests/test_path_cases.py must catch ("colour_before", "limit_ge", "miss_keeps_colour")."""
    rays = np.array(rays, np.float64).reshape(-1, 6)
    n = len(rays)
    rng = np.array(rng, np.uint32).reshape(n, 4).copy()
    cap = max_count + 1
    nv = np.zeros(n, np.int32)
    end = np.full(n, NO_RAY, np.int32)
    colour = np.zeros((n, 3), np.uint8)
    hit_index = np.full((n, cap), -1, np.int32)
    strike = np.full((n, cap, 3), np.nan)
    colour_after = np.zeros((n, cap, 3), np.uint8)
    ray_after = np.full((n, cap, 6), np.nan)
    counters = np.zeros(4, np.int64)
    live = np.flatnonzero(~np.isnan(rays[:, 0]))
    cur_ray = rays.copy()
    cur_col = np.full((n, 3), 255, np.uint8)
    bounces = 0
    limit_reached = (lambda b: b >= max_count) if mutant == "limit_ge" else (lambda b: b > max_count)
    while len(live) and not limit_reached(bounces):
        hit, sp, cnt = oracle_scene.hit_object(cur_ray[live])
        counters[0] += len(live)
        counters[1] += int(cnt[:, 0].astype(np.int64).sum())
        counters[2] += int(cnt[:, 1].astype(np.int64).sum())
        missed = hit < 0
        gone = live[missed]
        end[gone] = MISS
        colour[gone] = cur_col[gone] if mutant == "miss_keeps_colour" else 0
        live, hit, sp = live[~missed], hit[~missed], sp[~missed]
        if not len(live):
            break
        counters[3] += len(live)
        absorbed, col, ray, g = oracle_scene.reflection(hit, cur_ray[live], cur_col[live], sp, rng[live])
        j = bounces
        hit_index[live, j] = hit
        strike[live, j] = sp
        colour_after[live, j] = cur_col[live] if mutant == "colour_before" else col
        ab = absorbed != 0
        ray_after[live, j] = np.where(ab[:, None], np.nan, ray)
        nv[live] += 1
        rng[live] = g
        cur_ray[live] = ray
        cur_col[live] = col
        stopped = live[ab]
        end[stopped] = STOPPED
        colour[stopped] = colour_after[stopped, j]  # ValueSome c: the path's result IS the vertex's colour_after
        live = live[~ab]
        bounces += 1
    end[live] = BOUNCE_LIMIT
    colour[live] = HOTPINK
    k = max(int(nv.max()) if n else 0, 1)
    out = Paths(nv, end, colour, rays, rng, hit_index[:, :k], strike[:, :k], colour_after[:, :k], ray_after[:, :k], counters)
    for a in out:
        a.setflags(write=False)
    return out


def camera_paths(orc, oracle_scene, cam_abi, max_w, max_h, seed, pixels, sample_first=0, n_samples=1, mutant=None):
    """Slots i * n_samples + (s - sample_first), as the library numbers them."""
    pixels = np.asarray(pixels, np.int64)
    rays = camera_rays(orc, cam_abi, max_w, max_h, seed, pixels, sample_first, n_samples).reshape(-1, 6)
    g = np.repeat(pixels, n_samples)
    s = np.tile(np.arange(sample_first, sample_first + n_samples, dtype=np.int64), len(pixels))
    states = orc.stream_state(seed, g.astype(np.uint64), s.astype(np.uint32))
    advanced = xorshift_steps(states, 2)  # GetTwo
    if len(states):  # the cross-check the composer carries with it: the third draw of the stream is the first of the advanced state
        assert orc.float_producer(states[0], 3)[2] == orc.float_producer(advanced[0], 1)[0]
        assert orc.float_producer(states[-1], 3)[2] == orc.float_producer(advanced[-1], 1)[0]
    return trace(orc, oracle_scene, rays, advanced, int(cam_abi.bounce_depth), mutant)


def ray_paths(orc, oracle_scene, rays, bounce_depth, rng=None, seed=0, stream_base=0, sample=0):
    rays = np.array(rays, np.float64).reshape(-1, 6)
    n = len(rays)
    made = np.full((n, 6), np.nan)
    for i in range(n):
        m = orc.ray_make(tuple(rays[i, :3]), tuple(rays[i, 3:]))
        if m is not None:
            made[i] = m
    if rng is None:
        rng = orc.stream_state(seed, (np.arange(n, dtype=np.uint64) + np.uint64(stream_base)), np.full(n, sample, np.uint32))
    return trace(orc, oracle_scene, made, rng, bounce_depth)


def truncate(p: Paths, k):
    """The records as a call with max_vertices = k stores them: (hit_index, strike, colour_after, ray_after), [slots, k, ...]."""
    n, have = p.hit_index.shape
    out = (np.full((n, k), -1, np.int32), np.full((n, k, 3), np.nan), np.zeros((n, k, 3), np.uint8), np.full((n, k, 6), np.nan))
    m = min(k, have)
    for dst, src in zip(out, (p.hit_index, p.strike, p.colour_after, p.ray_after)):
        dst[:, :m] = src[:, :m]
    return out


def summary(n_vertices, end, colour, colour_after0, n_entries, n_samples):
    """The sixteen words per list entry from per-slot values; colour_after0 [slots, 3]: colour_after of vertex 0 (ignored where the
    path has no vertex)."""
    nv = np.asarray(n_vertices, np.int64).reshape(n_entries, n_samples)
    e = np.asarray(end).reshape(n_entries, n_samples)
    col = np.asarray(colour, np.int64).reshape(n_entries, n_samples, 3)
    c0 = np.asarray(colour_after0, np.int64).reshape(n_entries, n_samples, 3)
    out = np.zeros((n_entries, SUMMARY_WORDS), np.int64)
    out[:, 0] = n_samples
    out[:, 1] = nv.sum(1)
    out[:, 2] = nv.max(1) if n_samples else 0
    for kind in range(4):
        out[:, 3 + kind] = (e == kind).sum(1)
    has = nv >= 1
    out[:, 7] = has.sum(1)
    out[:, 8:11] = (c0 * has[:, :, None]).sum(1)
    out[:, 12] = n_samples
    out[:, 13:16] = col.sum(1)
    return out.astype(np.int32)


# ---- the fixtures the CPU and the GPU tests share: composed once per process, never written to ------------------------------------------
FRAME_SEED = 5


class Frame(NamedTuple):
    objs: list
    cam: object
    cam_abi: object
    w: int
    h: int
    spp: int
    depth: int
    oracle: object
    paths: Paths   # the whole frame, samples [0, spp), seed FRAME_SEED


@functools.lru_cache(maxsize=None)
def frame(name):
    """all_materials (41 x 71, 24 samples, depth 12), small_final (33 x 49, 40, depth 50: LDS-resident), many_spheres (21 x 35, 12,
    depth 8: too large for the LDS)."""
    import oracle as orc
    import scenes
    objs, cam, w, h = {"all_materials": scenes.all_materials, "small_final": scenes.small_final, "many_spheres": scenes.many_spheres}[name]()
    o = orc.OracleScene(objs)
    n_px = (2 * w + 1) * (2 * h + 1)
    paths = camera_paths(orc, o, cam.to_abi(), w, h, FRAME_SEED, np.arange(n_px), 0, cam.SamplesPerPixel)
    return Frame(objs, cam, cam.to_abi(), w, h, cam.SamplesPerPixel, cam.BounceDepth, o, paths)


atexit.register(frame.cache_clear)  # (the oracle scenes go before the interpreter takes the oracle's library apart)


def lights_scene():
    """A scene without a dome (light sources only, sky left over): test_camera_hits_host's."""
    import ray_tracing_fsharp_amd as rt
    from test_camera_hits_host import _basic_camera, _lights
    return _lights(rt)[0], _basic_camera(rt, 12, 35.0 / 21.0), 8, 5


@functools.lru_cache(maxsize=None)
def lights_paths():
    import oracle as orc
    objs, cam, w, h = lights_scene()
    return camera_paths(orc, orc.OracleScene(objs), cam.to_abi(), w, h, FRAME_SEED, np.arange((2 * w + 1) * (2 * h + 1)), 0, cam.SamplesPerPixel)


def no_ray_scene():
    """A hand-made camera whose viewport passes through the eye: the samples that land within 1e-4 of it have no ray (Ray.make')."""
    import scenes
    objs, cam, _, _ = scenes.all_materials(spp=8, depth=4)
    cam = scenes.free_camera((0.0, 1.0, -3.0), (0.0, 1.0, -3.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 4e-4, 4e-4, 8, 4)
    return objs, cam, 2, 2


@functools.lru_cache(maxsize=None)
def no_ray_camera_paths():
    import oracle as orc
    objs, cam, w, h = no_ray_scene()
    return camera_paths(orc, orc.OracleScene(objs), cam.to_abi(), w, h, FRAME_SEED, np.arange((2 * w + 1) * (2 * h + 1)), 0, cam.SamplesPerPixel)


RAY_DEPTH = 6


@functools.lru_cache(maxsize=None)
def ray_fixture():
    """(rays [1000 + zero vectors, 6], states, the composed paths with those states) in all_materials."""
    import oracle as orc
    import scenes
    rays = scenes.random_rays(1000, 23)
    rays = np.concatenate([rays[:500], np.zeros((3, 6)), rays[500:], np.array([[1.0, 2.0, 3.0, 0.0, 0.0, 0.0]])])
    states = np.random.default_rng(8).integers(1, 2**31 - 1, size=(len(rays), 4), dtype=np.int64).astype(np.uint32)
    rays.setflags(write=False)
    states.setflags(write=False)
    return rays, states, ray_paths(orc, frame("all_materials").oracle, rays, RAY_DEPTH, rng=states)
