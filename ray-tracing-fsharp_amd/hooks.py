"""numpy wrappers over the rt_dev_* device unit hooks (include/rtfs_amd.h): each runs ONE device function of the
path on the GPU so the reference's unit tests can be replayed against the code the render kernel inlines."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import check, lib
from .raytracing import Scene, _f64, _i32, _u8, _u32, _u64


def _c(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def float_producer(state, n, device=0):
    out = np.zeros(n, np.float64)
    check(lib.rt_dev_float_producer(device, (C.c_uint32 * 4)(*[int(s) for s in state]), n, _f64(out)))
    return out


def stream_state(seed, pixel, sample, device=0):
    pixel, sample = _c(pixel, np.uint64), _c(sample, np.uint32)
    out = np.zeros((len(pixel), 4), np.uint32)
    check(lib.rt_dev_stream_state(device, int(seed), len(pixel), _u64(pixel), _u32(sample), _u32(out)))
    return out


def bbox_hits(rays, boxes, device=0):
    rays, boxes = _c(rays, np.float64).reshape(-1, 6), _c(boxes, np.float64).reshape(-1, 6)
    out = np.zeros(len(rays), np.int32)
    check(lib.rt_dev_bbox_hits(device, len(rays), _f64(rays), _f64(boxes), _i32(out)))
    return out


def bbox_filter(rays, boxes, bmax=0.0, device=0):
    """bit 0: BoundingBox.hits, exactly; bit 1: the timed node loop's single-precision filter (its own instructions); bit 2: the same
    filter as compiled C++.  The filter must say 'hit' wherever the exact test does."""
    rays, boxes = _c(rays, np.float64).reshape(-1, 6), _c(boxes, np.float64).reshape(-1, 6)
    out = np.zeros(len(rays), np.int32)
    check(lib.rt_dev_bbox_filter(device, len(rays), _f64(rays), _f64(boxes), float(bmax), _i32(out)))
    return out


def sphere_first_intersection(rays, spheres, device=0):
    rays, spheres = _c(rays, np.float64).reshape(-1, 6), _c(spheres, np.float64).reshape(-1, 4)
    out = np.zeros(len(rays), np.float64)
    check(lib.rt_dev_sphere_first_intersection(device, len(rays), _f64(rays), _f64(spheres), _f64(out)))
    return out


def plane_intersection(rays, planes, device=0):
    rays, planes = _c(rays, np.float64).reshape(-1, 6), _c(planes, np.float64).reshape(-1, 6)
    out = np.zeros(len(rays), np.float64)
    check(lib.rt_dev_plane_intersection(device, len(rays), _f64(rays), _f64(planes), _f64(out)))
    return out


def pixel_combine(a, b, device=0):
    a, b = _c(a, np.uint8).reshape(-1, 3), _c(b, np.uint8).reshape(-1, 3)
    out = np.zeros_like(a)
    check(lib.rt_dev_pixel_combine(device, len(a), _u8(a), _u8(b), _u8(out)))
    return out


def pixel_darken(p, albedo, device=0):
    p, albedo = _c(p, np.uint8).reshape(-1, 3), _c(albedo, np.float64)
    out = np.zeros_like(p)
    check(lib.rt_dev_pixel_darken(device, len(p), _u8(p), _f64(albedo), _u8(out)))
    return out


def arith(op, a, b=None, device=0):
    a = _c(a, np.float64)
    bb = _c(b, np.float64) if b is not None else None
    out = np.zeros_like(a)
    check(lib.rt_dev_arith(device, op, len(a), _f64(a), _f64(bb) if bb is not None else None, _f64(out)))
    return out


def reflection(scene: Scene, index, ray_in, colour_in, strike, rng_state, device=0):
    index = _c(index, np.int32)
    ray_in, strike = _c(ray_in, np.float64).reshape(-1, 6), _c(strike, np.float64).reshape(-1, 3)
    colour_in = _c(colour_in, np.uint8).reshape(-1, 3)
    rng = _c(rng_state, np.uint32).reshape(-1, 4).copy()
    n = len(index)
    absorbed, col, ray = np.zeros(n, np.int32), np.zeros((n, 3), np.uint8), np.zeros((n, 6), np.float64)
    check(lib.rt_dev_reflection(device, scene.handle, n, _i32(index), _f64(ray_in), _u8(colour_in), _f64(strike), _u32(rng),
                                _i32(absorbed), _u8(col), _f64(ray)))
    return absorbed, col, ray, rng


def hit_object(scene: Scene, rays, device=0):
    rays = _c(rays, np.float64).reshape(-1, 6)
    n = len(rays)
    hit, strike, cnt = np.zeros(n, np.int32), np.zeros((n, 3), np.float64), np.zeros((n, 2), np.uint32)
    check(lib.rt_dev_hit_object(device, scene.handle, n, _f64(rays), _i32(hit), _f64(strike), _u32(cnt)))
    return hit, strike, cnt


def hit_object_lds(scene: Scene, rays, device=0):
    """Scene.hitObject through the timed kernel variant's route: scene in LDS, hand-written node loop."""
    rays = _c(rays, np.float64).reshape(-1, 6)
    n = len(rays)
    hit, strike = np.zeros(n, np.int32), np.zeros((n, 3), np.float64)
    check(lib.rt_dev_hit_object_lds(device, scene.handle, n, _f64(rays), _i32(hit), _f64(strike)))
    return hit, strike


def pixel_candidates(scene: Scene, camera, max_w, max_h, row_col, device=0):
    """The Leaves the camera rays of each pixel can reach, as the timed kernel finds them once per pixel: [n, 4] hittable indices,
    -1 padded; a row starting with -2 means "these rays walk the tree"."""
    import ctypes as C
    rc = _c(row_col, np.int32).reshape(-1, 2)
    out = np.zeros((len(rc), 4), np.int32)
    cam = camera.to_abi()
    check(lib.rt_dev_pixel_candidates(device, scene.handle, C.byref(cam), int(max_w), int(max_h), len(rc), _i32(rc), _i32(out)))
    return out


def trace_ray(scene: Scene, bounce_depth, rays, rng_state, device=0):
    rays = _c(rays, np.float64).reshape(-1, 6)
    rng = _c(rng_state, np.uint32).reshape(-1, 4).copy()
    col = np.zeros((len(rays), 3), np.uint8)
    check(lib.rt_dev_trace_ray(device, scene.handle, int(bounce_depth), len(rays), _f64(rays), _u32(rng), _u8(col)))
    return col, rng


def texture_colour_at(scene: Scene, texture, points, device=0):
    points = _c(points, np.float64).reshape(-1, 3)
    uv, col = np.zeros((len(points), 2), np.float64), np.zeros((len(points), 3), np.uint8)
    check(lib.rt_dev_texture_colour_at(device, scene.handle, int(texture), len(points), _f64(points), _f64(uv), _u8(col)))
    return uv, col


# rt_dev_last_launch_plan's words, under the names tests/c/launch_plan_table.cpp reads and prints
PLAN_INPUTS = ("kind", "lds_total", "lds32_total", "n_nodes", "n_obj", "has_tex", "s_block", "s_chunk", "s_bpc", "s_yield", "s_refill",
               "s_passes", "s_park", "count", "log", "n_rows", "max_w", "spp", "n", "cu_count", "per_cu")
PLAN_HEAD = ("q_lds", "q_count", "q_block", "q_mode", "q_tex", "q_lds_bytes", "two_pass", "pairs", "list", "sort", "pool", "waves", "error")
PLAN_PASS = ("mode", "grid", "lds_bytes", "chunk", "park", "park_l", "park_l_lds", "lds_node_bytes", "lds_node_thr", "yield", "leaf_wait",
             "refill", "k", "total_waves")
PLAN_WORDS = 80


PATHS_PLAN = ("block", "grid", "chunk", "lds_bytes", "lds_resident", "counting", "textured", "slots")


def last_paths_plan():
    """The plan (csrc/rt_paths_plan.h) of the calling thread's last path launch (cameraPaths / tracePaths), or None before the first."""
    w = (C.c_int64 * 8)()
    check(lib.rt_dev_last_paths_plan(w))
    return dict(zip(PATHS_PLAN, w)) if w[0] else None


SURFACE_PLAN = ("slots", "tile", "grid", "block", "program", "texture_phase", "textured", "reserved")


def last_surface_plan():
    """The plan (csrc/rt_surface_plan.h) of the calling thread's last surface launch (Scene.surfaces / Scene.cameraSurfaces), or None
    before the first.  textured: the slots the texture phase evaluated, -1 when no statistics were asked for."""
    w = (C.c_int64 * 8)()
    check(lib.rt_dev_last_surface_plan(w))
    return dict(zip(SURFACE_PLAN, w)) if w[0] else None


def last_launch_plan():
    """The launch plan (csrc/rt_launch_plan.h) of the calling thread's last launch as the library executed it: {"in": the planner's
    inputs, "out": its decisions}, keyed as launch_plan_table.cpp's lines are (F_ for a fused or ray-list launch, A_ and B_ for a
    two-pass one; an extension reports both, A_ all zeros).  None before this thread's first launch."""
    w = (C.c_int64 * PLAN_WORDS)()
    check(lib.rt_dev_last_launch_plan(w))
    if not w[0]:
        return None
    at = 1
    inp = dict(zip(PLAN_INPUTS, w[at:at + len(PLAN_INPUTS)]))
    at += len(PLAN_INPUTS)
    out = dict(zip(PLAN_HEAD, w[at:at + len(PLAN_HEAD)]))
    at += len(PLAN_HEAD)
    for name in "FAB":
        if (name == "F") != bool(out["two_pass"]) and not out["error"]:
            out.update({f"{name}_{k}": v for k, v in zip(PLAN_PASS, w[at:at + len(PLAN_PASS)])})
        at += len(PLAN_PASS)
    inp["first_sample"] = w[at]  # word 77: 0 = a fresh render, else the samples_done of an extension (pass B alone: A_ words 0)
                                 # (camera hits, kind 5: sample_first)
    inp["map"] = w[at + 1]       # word 78: 1 = an extension by map (first_sample is then 12, spp the cap, B_mode 9 or 10)
    if inp["kind"] == 7:         # camera hits over a batch of views: kind 5's words (n: the list's entries), and word 79: the views
        inp["n_views"] = w[at + 2]
    return {"in": inp, "out": out}


def scene_image(scene: Scene, device=0):
    """rt_dev_scene_image: (the image bytes as `device` holds them, the 16 offset words: SceneOffsets' thirteen, then zeros)."""
    size, offsets = C.c_size_t(0), np.zeros(16, np.uint32)
    check(lib.rt_dev_scene_image(scene.handle, device, None, 0, C.byref(size), _u32(offsets)))
    out = np.zeros(size.value, np.uint8)
    check(lib.rt_dev_scene_image(scene.handle, device, out.ctypes.data, out.size, C.byref(size), _u32(offsets)))
    return out, offsets


def encode_image(scene: Scene, device=0, digit_bits=8):
    """rt_dev_encode_image(_radix): the device encoder alone on the scene's own walk tree, object table and hittables -> the image bytes.
    digit_bits: the width of a pass of the order by depth (8 in the product)."""
    size = C.c_size_t(0)
    check(lib.rt_dev_encode_image_radix(device, scene.handle, digit_bits, None, 0, C.byref(size)))
    out = np.zeros(size.value, np.uint8)
    check(lib.rt_dev_encode_image_radix(device, scene.handle, digit_bits, out.ctypes.data, out.size, C.byref(size)))
    return out


def scene_has_host_mirror(scene: Scene) -> bool:
    return bool(lib.rt_dev_scene_has_host_mirror(scene.handle))


def scene_texels(scene: Scene, device=0):
    """rt_dev_scene_texels: (the texel blob as `device` holds it, every record's texel_off as uint32 -- 0xFFFFFFFF: not an image)."""
    size = C.c_size_t(0)
    offs = np.zeros(max(1, scene.info()["n_textures"]), np.uint32)
    check(lib.rt_dev_scene_texels(scene.handle, device, None, 0, C.byref(size), _u32(offs)))
    out = np.zeros(size.value, np.uint8)
    check(lib.rt_dev_scene_texels(scene.handle, device, out.ctypes.data if out.size else None, out.size, C.byref(size), _u32(offs)))
    return out, offs[:scene.info()["n_textures"]]


TEXTURE_PLAN = ("textures", "images", "device_sourced", "jpeg_sourced", "blob_bytes", "launches", "bytes_host_to_device", "bytes_device_to_host")


def texture_plan() -> dict:
    """rt_dev_last_texture_plan: the calling thread's last Scene.make with ofImageDevice / ofJpeg textures, and what was launched and
    copied since (set_image, the lazy fetch of the host's texels)."""
    w = (C.c_int64 * 8)()
    check(lib.rt_dev_last_texture_plan(w))
    return dict(zip(TEXTURE_PLAN, w))


JPEG_PLAN = ("subsequence_bytes", "subsequences", "rounds", "decodes", "blocks", "boundaries")


def decode_jpeg(data: bytes, subsequence_bytes=0, device=0, out=None):
    """rt_dev_decode_jpeg: the device decode with subsequences of subsequence_bytes (0: the default) into `out`, a uint8 torch tensor on
    the device (made from the header when None) -> (status, out).  The status is returned, not raised: refusals are what the hook tests."""
    import torch

    from .raytracing import LoadImage
    data = bytes(data)
    if out is None:
        i = LoadImage.info(data)
        out = torch.empty((i["height"], i["width"], 3), dtype=torch.uint8, device=torch.device("cuda", device))
    return int(lib.rt_dev_decode_jpeg(device, data, len(data), subsequence_bytes, out.data_ptr(), out.numel())), out


def last_jpeg_plan():
    """The plan of the calling thread's last device decode of a JPEG, or None before the first."""
    w = (C.c_int64 * 8)()
    check(lib.rt_dev_last_jpeg_plan(w))
    return dict(zip(JPEG_PLAN, w)) if w[0] else None
