"""What surface records cost, on one GPU, on the bench frame (2401x1601, one sample per pixel, tuned tree) for the config-3 scene (no
parameterised texture) and the earth scene (a textured globe), tensors on the device, events on the stream (rt_stats.kernel_ms):

  hits      rt_camera_hits_device with strike, no rays_out: the camera-hits kernel alone (the parent's entry point, the same kernel)
  both      rt_camera_surfaces_device, every output but uv / every output: the camera-hits kernel + surface_kernel
  surface   both - hits, and rt_surfaces_device over the frame's own hits with a ray array (its list check included)
  floor     the bytes surface_kernel must read and write for the outputs requested / 6.3 TB/s (the achievable HBM rate), as a ratio

and for texture_cases.mostly_textured_scene at --tex-pixels: the time per textured slot and the phase-2 lane occupancy
(textured slots / (64 x phase-2 wave iterations), the iterations counted from the hits: ceil(list length / 64) per tile).
Medians and min..max of --reps runs after --warmup; no threshold is set.

usage: python scripts/surfaces_measure.py [--pixels 800] [--tex-pixels 400] [--reps 9] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM = 6.3e12  # bytes/s


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    return [fn() for _ in range(reps)]


def textured_mask(rt, objs, hit):
    """Per slot: does its colour go through phase 2 (rt_surface_plan.h's predicate, from the records)?"""
    A = rt._abi
    hs, n, tex, ntex, keep = rt.raytracing.flatten_hittables(objs)
    phase = np.zeros(n + 1, bool)
    for i in range(n):
        plane = hs[i].kind == A.RT_HITTABLE_INFINITE_PLANE
        carries = hs[i].style == A.RT_PLANE_LIGHT_SOURCE if plane else hs[i].style != A.RT_SPHERE_LIGHT_SOURCE_CAP
        phase[i] = carries and hs[i].texture >= 0 and tex[hs[i].texture].kind != A.RT_TEXTURE_COLOUR
    return phase[np.where(hit < 0, n, hit)]


def floor_ms(slots, outputs, ray_array):
    per = 4 + 24 + (24 if ray_array else 0) + sum({"normal": 24, "inside": 1, "colour": 3, "tint": 3, "uv": 16}[o] for o in outputs)
    return slots * per / HBM * 1e3, per


def measure_scene(rt, torch, name, objs, cam, w, h, args):
    scene = rt.Scene.make(objs)
    scene.tune(w, h, cam, seed=1, device=0)
    n = (2 * w + 1) * (2 * h + 1)
    out = {"scene": name, "frame": [2 * w + 1, 2 * h + 1], "slots": n}
    hits_ms = timed(lambda: scene.cameraHits(w, h, cam, seed=1, rays=False, tensors=True, device=0).stats["kernel_ms"], args.reps, args.warmup)
    out["camera_hits_kernel_ms"] = spread(hits_ms)
    base = scene.cameraHits(w, h, cam, seed=1, rays=False, tensors=True, device=0)
    rays = torch.zeros((n, 6), dtype=torch.float64, device="cuda:0")
    rays[:, :3] = torch.tensor(list(cam.to_abi().view_origin), dtype=torch.float64, device="cuda:0")
    hit, strike = base.hit_index.reshape(-1), base.strike.reshape(-1, 3)
    tex = textured_mask(rt, objs, hit.cpu().numpy())
    out["textured_slots"] = int(tex.sum())
    for label, kw in (("normal_inside", dict(colour=False, tint=False, uv=False)), ("all_but_uv", dict(uv=False)), ("all", dict(uv=True))):
        outputs = [o for o in ("normal", "inside", "colour", "tint", "uv") if kw.get(o, True)]
        both = timed(lambda: scene.cameraSurfaces(w, h, cam, seed=1, tensors=True, device=0, **kw)[1].stats["kernel_ms"], args.reps, args.warmup)
        alone = timed(lambda: scene.surfaces(hit, strike, rays, **kw).stats["kernel_ms"], args.reps, args.warmup)
        fl_cam, per_cam = floor_ms(n, outputs, False)
        fl_ray, per_ray = floor_ms(n, outputs, True)
        inside = [b - statistics.median(hits_ms) for b in both]
        out[label] = {"outputs": outputs, "camera_surfaces_kernel_ms": spread(both), "surface_kernel_inside_ms": spread(inside),
                      "surfaces_over_ray_array_kernel_ms": spread(alone), "bytes_per_slot": {"camera_route": per_cam, "ray_array": per_ray},
                      "floor_ms": {"camera_route": round(fl_cam, 4), "ray_array": round(fl_ray, 4)},
                      "ratio_to_floor": {"camera_route": round(statistics.median(inside) / fl_cam, 2), "ray_array": round(statistics.median(alone) / fl_ray, 2)}}
    return out


def measure_textured(rt, torch, args):
    import texture_cases
    objs, cam, w, h = texture_cases.mostly_textured_scene(pixels=args.tex_pixels)
    scene = rt.Scene.make(objs)
    n = (2 * w + 1) * (2 * h + 1)
    base = scene.cameraHits(w, h, cam, seed=1, rays=False, tensors=True, device=0)
    hit, strike = base.hit_index.reshape(-1), base.strike.reshape(-1, 3)
    rays = torch.zeros((n, 6), dtype=torch.float64, device="cuda:0")
    rays[:, :3] = torch.tensor(list(cam.to_abi().view_origin), dtype=torch.float64, device="cuda:0")
    tex = textured_mask(rt, objs, hit.cpu().numpy())
    tiles = -(-n // 1024)
    per_tile = np.add.reduceat(tex.astype(np.int64), np.arange(0, n, 1024))
    iterations = int(np.sum(-(-per_tile // 64)))
    with_tex = timed(lambda: scene.surfaces(hit, strike, rays, uv=True).stats["kernel_ms"], args.reps, args.warmup)
    without = timed(lambda: scene.surfaces(hit, strike, rays, colour=False, tint=False).stats["kernel_ms"], args.reps, args.warmup)
    assert rt.hooks.last_surface_plan()["texture_phase"] == 0
    t = int(tex.sum())
    # the same evaluation at the lane occupancy the hits have: what phase 2 is there to avoid (waves of 64 consecutive slots with >= 1 textured one)
    per_wave = np.add.reduceat(tex.astype(np.int64), np.arange(0, n, 64))
    return {"scene": "mostly_textured", "frame": [2 * w + 1, 2 * h + 1], "slots": n, "tiles": tiles, "textured_slots": t,
            "kernel_ms_all_outputs": spread(with_tex), "kernel_ms_normal_inside_only": spread(without),
            "ns_per_textured_slot": round((statistics.median(with_tex) - statistics.median(without)) * 1e6 / max(t, 1), 3),
            "phase2_wave_iterations": iterations, "phase2_lane_occupancy": round(t / (64.0 * max(iterations, 1)), 4),
            "occupancy_without_the_list": round(t / (64.0 * max(int((per_wave > 0).sum()), 1)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pixels", type=int, default=800)
    ap.add_argument("--tex-pixels", type=int, default=400)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r33", "surfaces_measure.json"))
    args = ap.parse_args()
    import torch

    import ray_tracing_fsharp_amd as rt
    import scenes
    res = {"reps": args.reps, "warmup": args.warmup, "hbm_bytes_per_s": HBM, "device": torch.cuda.get_device_name(0), "scenes": []}
    objs, cam, w, h = rt.sample_images.config3_final(seed=2024, spp=500, depth=50, pixels=args.pixels)
    res["scenes"].append(measure_scene(rt, torch, "config3_final", objs, cam, w, h, args))
    objs, cam, _, _ = rt.sample_images.earth(scenes.golden("earthmap_rgb")["rgb"])
    res["scenes"].append(measure_scene(rt, torch, "earth", objs, cam, w, h, args))
    res["textured"] = measure_textured(rt, torch, args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
