"""What a batch of views gains over one launch per view (rt_render_views_device against rt_render_device_ex), on one GPU.

  (a) small frames   K views (config 2, the three Lambert spheres, its camera turned round the y axis in K steps) of a 71x41 frame at 100 spp,
                     depth 50: ONE rt_render_views_device call
                     against K rt_render_device_ex calls enqueued back to back on one stream, all with stats == NULL; each leg is timed
                     by the host clock around one stream synchronise, the legs alternate after a warm-up.  The batch's views are
                     checked against the K frames before anything is timed.  One extra launch of each leg with statistics gives the
                     device time between the events (for the K calls: summed), and one with the counting variant the stage cycles.
  (b) overhead       K = 1 at the bench frame (config 3, 2401x1601 at 500 spp, tuned tree) through the views kernels against
                     rt_render_device_ex: kernel_ms of alternating repetitions -- the price of the variant.

usage: python scripts/views_measure.py [--views 64] [--reps 9] [--bench-reps 3] [--out FILE]"""
import argparse
import ctypes as C
import dataclasses
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def turntable(rt, cam, k):
    """k cameras: the scene's camera (eye and view direction) turned round the y axis in k equal steps"""
    a = cam.to_abi()
    eye, view = np.array(list(a.view_origin)), np.array(list(a.view_dir))
    aspect = a.viewport_width / a.viewport_height
    cams = []
    for i in range(k):
        t = 2.0 * math.pi * i / k
        rot = np.array([[math.cos(t), 0.0, math.sin(t)], [0.0, 1.0, 0.0], [-math.sin(t), 0.0, math.cos(t)]])
        e, v = rot @ eye, rot @ view
        c = rt.Camera.makeBasic(cam.SamplesPerPixel, a.focal_length, aspect, rt.Point.make(*map(float, e)), rt.Vector.unitise(rt.Vector.make(*map(float, v))),
                                rt.Vector.make(0.0, 1.0, 0.0))
        cams.append(dataclasses.replace(c, BounceDepth=cam.BounceDepth))
    return cams


def stats_of(values):
    return {"runs": [round(v, 3) for v in values], "median": round(float(np.median(values)), 3), "min": round(min(values), 3), "max": round(max(values), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--pixels", type=int, default=20, help="maxHeightCoord of the small frames: 20 is 71x41")
    ap.add_argument("--spp", type=int, default=100)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--bench-reps", type=int, default=3)
    ap.add_argument("--bench-pixels", type=int, default=800)
    ap.add_argument("--bench-spp", type=int, default=500)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import ray_tracing_fsharp_amd as rt

    A, L = rt._abi, rt.lib
    if rt.device_count() < 1:
        raise SystemExit("views_measure.py needs a GPU")
    out = {}

    # ---- (a) ----
    objs, cam, w, h = rt.sample_images.config2_three_lambert(spp=args.spp, depth=args.depth, pixels=args.pixels)
    rows, cols = 2 * h + 1, 2 * w + 1
    k = args.views
    cams = turntable(rt, cam, k)
    seeds = [args.seed + i for i in range(k)]
    scene = rt.Scene.make(objs)
    stream = torch.cuda.Stream()
    st_handle = stream.cuda_stream
    with torch.cuda.stream(stream):
        batch = torch.zeros((k, rows, cols, 4), dtype=torch.int32, device="cuda")
        batch_rgb = torch.zeros((k, rows, cols, 3), dtype=torch.uint8, device="cuda")
        single = torch.zeros((k, rows, cols, 4), dtype=torch.int32, device="cuda")
        single_rgb = torch.zeros((k, rows, cols, 3), dtype=torch.uint8, device="cuda")
    stream.synchronize()
    abi = (A.rt_camera * k)(*[c.to_abi() for c in cams])
    keys = (C.c_uint64 * k)(*seeds)

    def run_batch(stats=None, flags=0):
        rt._lib.check(L.rt_render_views_device(scene.handle, abi, k, w, h, keys, 0, 0, flags, batch.data_ptr(), batch_rgb.data_ptr(), st_handle, None,
                                               C.byref(stats) if stats is not None else None))

    def run_singles(stats=None, flags=0):
        total = {"kernel_ms": 0.0}
        for i in range(k):
            s = A.rt_stats() if stats else None
            rt._lib.check(L.rt_render_device_ex(scene.handle, C.byref(abi[i]), w, h, seeds[i], 0, 0, 1, rows, flags, single[i].data_ptr(), single_rgb[i].data_ptr(),
                                                st_handle, None, C.byref(s) if s is not None else None))
            if s is not None:
                total["kernel_ms"] += s.kernel_ms
        return total

    def timed(fn):
        stream.synchronize()
        t0 = time.perf_counter()
        fn()
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(2):  # warm-up of both legs
        timed(run_batch); timed(run_singles)
    if not (torch.equal(batch, single) and torch.equal(batch_rgb, single_rgb)):
        raise SystemExit("the batch's views differ from the K frames")
    ms = {"batch": [], "singles": []}
    for _ in range(args.reps):
        ms["batch"].append(timed(run_batch))
        ms["singles"].append(timed(run_singles))
    s = A.rt_stats()
    run_batch(s)
    plan = rt.hooks.last_launch_plan()
    batch_kernel_ms = s.kernel_ms
    singles_kernel_ms = run_singles(True)["kernel_ms"]
    plan1 = rt.hooks.last_launch_plan()
    # the counting variant: rays and samples (equal by the contract), and where the waves' cycles go
    s = A.rt_stats()
    run_batch(s, A.RT_RENDER_COUNTERS)
    words = (C.c_uint64 * 16)()
    rt._lib.check(L.rt_last_stage_stats(words))
    stage_batch = [int(x) for x in words]  # include/rtfs_amd.h, rt_last_stage_stats: [12..15] cycles in refill / slow / walk / shade
    out["small_frames"] = {
        "frame": [cols, rows], "views": k, "spp": args.spp, "depth": args.depth, "pixels": k * rows * cols,
        "wall_ms": {name: stats_of(v) for name, v in ms.items()},
        "speedup_median": round(float(np.median(ms["singles"]) / np.median(ms["batch"])), 3),
        "kernel_ms_between_events": {"batch": round(batch_kernel_ms, 3), "singles_summed": round(singles_kernel_ms, 3)},
        "samples": int(s.samples), "rays": int(s.rays),
        "Gray_per_s_wall": {name: round(s.rays / (float(np.median(v)) * 1e-3) / 1e9, 2) for name, v in ms.items()},
        "plan": {"batch": {"two_pass": plan["out"]["two_pass"], "block": plan["out"]["q_block"], "waves": plan["out"]["waves"],
                           "chunk": plan["out"].get("A_chunk", plan["out"].get("F_chunk")), "chunk_b": plan["out"].get("B_chunk")},
                 "single": {"two_pass": plan1["out"]["two_pass"], "block": plan1["out"]["q_block"], "waves": plan1["out"]["waves"],
                            "chunk": plan1["out"].get("A_chunk", plan1["out"].get("F_chunk"))}},
        "counting_variant_stage_stats_batch": stage_batch,
    }
    print(json.dumps(out["small_frames"]), flush=True)

    # ---- (b) ----
    if args.bench_reps > 0:
        objs, cam, w, h = rt.sample_images.config3_final(seed=args.seed, spp=args.bench_spp, depth=args.depth, pixels=args.bench_pixels)
        rows, cols = 2 * h + 1, 2 * w + 1
        scene = rt.Scene.make(objs)
        scene.tune(w, h, cam, seed=args.seed ^ 0x5EED, device=0)
        with torch.cuda.stream(stream):
            fa = torch.zeros((1, rows, cols, 4), dtype=torch.int32, device="cuda")
            fb = torch.zeros((rows, cols, 4), dtype=torch.int32, device="cuda")
        abi1 = (A.rt_camera * 1)(cam.to_abi())

        def views_leg():
            s = A.rt_stats()
            rt._lib.check(L.rt_render_views_device(scene.handle, abi1, 1, w, h, None, args.seed, 0, 0, fa.data_ptr(), None, st_handle, None, C.byref(s)))
            return s.kernel_ms

        def frame_leg():
            s = A.rt_stats()
            rt._lib.check(L.rt_render_device_ex(scene.handle, C.byref(abi1[0]), w, h, args.seed, 0, 0, 1, rows, 0, fb.data_ptr(), None, st_handle, None, C.byref(s)))
            return s.kernel_ms

        views_leg(); frame_leg()  # warm-up
        if not torch.equal(fa[0], fb):
            raise SystemExit("K = 1 differs from the frame")
        kms = {"views": [], "frame": []}
        for _ in range(args.bench_reps):
            kms["views"].append(views_leg())
            kms["frame"].append(frame_leg())
        out["one_view_at_the_bench_frame"] = {"frame": [cols, rows], "spp": args.bench_spp, "kernel_ms": {n: stats_of(v) for n, v in kms.items()},
                                              "views_over_frame_median": round(float(np.median(kms["views"]) / np.median(kms["frame"])), 4)}
        print(json.dumps(out["one_view_at_the_bench_frame"]), flush=True)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
