"""What continuing a batch of views in one launch gains over one extension per view (rt_render_views_extend_device against
rt_render_extend_device), on one GPU.

  (a) small frames   the batch of scripts/views_measure.py -- K views of config 2 at 71x41, depth 50, seeds 2024 + v -- rendered at 16 spp, then
                     continued to 100: ONE rt_render_views_extend_device call against K rt_render_extend_device calls enqueued back to back
                     on one stream, all with stats == NULL; each leg is timed by the host clock around one stream synchronise (the restore
                     of the 16-spp buffer is enqueued and waited for BEFORE the clock starts), the legs alternate after a warm-up.  The two
                     outputs are compared with each other and with K frames rendered at 100 before anything is timed.
  (b) by map         the same with per-VIEW targets drawn from {16, 40, 100}: ONE rt_render_views_extend_map_device call against K
                     rt_render_extend_map_device calls.
  (c) overhead       K = 1 at the bench frame (config 3, 2401x1601, tuned tree), 100 -> 500 spp, through the views kernel against
                     rt_render_extend_device: kernel_ms of alternating repetitions -- the price of the variant.

usage: python scripts/views_extend_measure.py [--views 64] [--reps 9] [--bench-reps 3] [--out FILE]"""
import argparse
import ctypes as C
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from views_measure import stats_of, turntable  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--pixels", type=int, default=20, help="maxHeightCoord of the small frames: 20 is 71x41")
    ap.add_argument("--first", type=int, default=16)
    ap.add_argument("--spp", type=int, default=100)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--bench-reps", type=int, default=3)
    ap.add_argument("--bench-pixels", type=int, default=800)
    ap.add_argument("--bench-first", type=int, default=100)
    ap.add_argument("--bench-spp", type=int, default=500)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import ray_tracing_fsharp_amd as rt

    A, L = rt._abi, rt.lib
    check = rt._lib.check
    if rt.device_count() < 1:
        raise SystemExit("views_extend_measure.py needs a GPU")
    out = {}

    objs, cam, w, h = rt.sample_images.config2_three_lambert(spp=args.spp, depth=args.depth, pixels=args.pixels)
    rows, cols = 2 * h + 1, 2 * w + 1
    k = args.views
    cams = turntable(rt, cam, k)  # at the target count
    seeds = [args.seed + i for i in range(k)]
    scene = rt.Scene.make(objs)
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream
    abi = (A.rt_camera * k)(*[c.to_abi() for c in cams])
    abi_first = (A.rt_camera * k)(*[dataclasses.replace(c, SamplesPerPixel=args.first).to_abi() for c in cams])
    keys = (C.c_uint64 * k)(*seeds)
    with torch.cuda.stream(stream):
        start = torch.zeros((k, rows, cols, 4), dtype=torch.int32, device="cuda")
        full = torch.zeros((k, rows, cols, 4), dtype=torch.int32, device="cuda")
        full_rgb = torch.zeros((k, rows, cols, 3), dtype=torch.uint8, device="cuda")
        batch, single = torch.zeros_like(start), torch.zeros_like(start)
        batch_rgb, single_rgb = torch.zeros_like(full_rgb), torch.zeros_like(full_rgb)
        check(L.rt_render_views_device(scene.handle, abi_first, k, w, h, keys, 0, 0, 0, start.data_ptr(), None, sh, None, None))
        check(L.rt_render_views_device(scene.handle, abi, k, w, h, keys, 0, 0, 0, full.data_ptr(), full_rgb.data_ptr(), sh, None, None))
        # per-view targets of the map legs
        per_view = np.random.default_rng(args.seed).choice(np.array([args.first, 40, args.spp], np.int32), size=k).astype(np.int32)
        targets = torch.from_numpy(np.broadcast_to(per_view[:, None, None], (k, rows, cols)).copy()).cuda()
    stream.synchronize()

    def restore(buf):
        with torch.cuda.stream(stream):
            buf.copy_(start)

    def batch_uniform(stats=None, flags=0):
        check(L.rt_render_views_extend_device(scene.handle, abi, k, w, h, keys, 0, 0, flags, args.first, batch.data_ptr(), batch_rgb.data_ptr(), sh, None,
                                              C.byref(stats) if stats is not None else None))

    def singles_uniform(stats=False):
        total = 0.0
        for i in range(k):
            s = A.rt_stats() if stats else None
            check(L.rt_render_extend_device(scene.handle, C.byref(abi[i]), w, h, seeds[i], 0, 0, 1, rows, 0, args.first, single[i].data_ptr(), single_rgb[i].data_ptr(),
                                            sh, None, C.byref(s) if s is not None else None))
            total += s.kernel_ms if s is not None else 0.0
        return total

    def batch_map(stats=None):
        check(L.rt_render_views_extend_map_device(scene.handle, abi, k, w, h, keys, 0, 0, 0, targets.data_ptr(), batch.data_ptr(), batch_rgb.data_ptr(), sh, None,
                                                  C.byref(stats) if stats is not None else None))

    def singles_map(stats=False):
        total = 0.0
        for i in range(k):
            s = A.rt_stats() if stats else None
            check(L.rt_render_extend_map_device(scene.handle, C.byref(abi[i]), w, h, seeds[i], 0, 0, 1, rows, 0, targets[i].data_ptr(), single[i].data_ptr(),
                                                single_rgb[i].data_ptr(), sh, None, C.byref(s) if s is not None else None))
            total += s.kernel_ms if s is not None else 0.0
        return total

    def timed(fn, buf):
        restore(buf)
        stream.synchronize()
        t0 = time.perf_counter()
        fn()
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def leg(name, run_batch, run_singles, want=None):
        for _ in range(2):  # warm-up of both legs
            timed(run_batch, batch); timed(run_singles, single)
        if not (torch.equal(batch, single) and torch.equal(batch_rgb, single_rgb)):
            raise SystemExit(f"{name}: the batch's views differ from the K extended frames")
        if want is not None and not (torch.equal(batch, want[0]) and torch.equal(batch_rgb, want[1])):
            raise SystemExit(f"{name}: the continued batch differs from the K frames rendered at the target")
        ms = {"batch": [], "singles": []}
        for _ in range(args.reps):
            ms["batch"].append(timed(run_batch, batch))
            ms["singles"].append(timed(run_singles, single))
        restore(batch); stream.synchronize()
        s = A.rt_stats()
        run_batch(s)
        plan = rt.hooks.last_launch_plan()
        restore(single); stream.synchronize()
        singles_kernel = run_singles(True)
        out[name] = {
            "frame": [cols, rows], "views": k, "from": args.first, "to": args.spp, "depth": args.depth, "pixels": k * rows * cols,
            "samples_added": int(s.samples), "pixels_final": int(s.pixels_early),
            "wall_ms": {n: stats_of(v) for n, v in ms.items()},
            "speedup_median": round(float(np.median(ms["singles"]) / np.median(ms["batch"])), 3),
            "kernel_ms_between_events": {"batch": round(s.kernel_ms, 3), "singles_summed": round(singles_kernel, 3)},
            "plan_batch": {"block": plan["out"]["q_block"], "chunk_b": plan["out"]["B_chunk"], "mode_b": plan["out"]["B_mode"], "waves": plan["out"]["waves"],
                           "pairs": plan["out"]["pairs"], "sort": plan["out"]["sort"]},
        }
        print(json.dumps({name: out[name]}), flush=True)

    leg("uniform", batch_uniform, singles_uniform, want=(full, full_rgb))
    out["map_targets_per_view"] = {str(t): int((per_view == t).sum()) for t in sorted(set(per_view.tolist()))}
    leg("map", batch_map, singles_map)

    # ---- (c) ----
    if args.bench_reps > 0:
        objs, cam, w, h = rt.sample_images.config3_final(seed=args.seed, spp=args.bench_spp, depth=args.depth, pixels=args.bench_pixels)
        rows, cols = 2 * h + 1, 2 * w + 1
        scene = rt.Scene.make(objs)
        scene.tune(w, h, cam, seed=args.seed ^ 0x5EED, device=0)
        abi1 = (A.rt_camera * 1)(cam.to_abi())
        first1 = (A.rt_camera * 1)(dataclasses.replace(cam, SamplesPerPixel=args.bench_first).to_abi())
        with torch.cuda.stream(stream):
            base = torch.zeros((1, rows, cols, 4), dtype=torch.int32, device="cuda")
            fa, fb = torch.zeros_like(base), torch.zeros_like(base)
            check(L.rt_render_views_device(scene.handle, first1, 1, w, h, None, args.seed, 0, 0, base.data_ptr(), None, sh, None, None))
        stream.synchronize()

        def views_leg():
            with torch.cuda.stream(stream):
                fa.copy_(base)
            s = A.rt_stats()
            check(L.rt_render_views_extend_device(scene.handle, abi1, 1, w, h, None, args.seed, 0, 0, args.bench_first, fa.data_ptr(), None, sh, None, C.byref(s)))
            return s.kernel_ms

        def frame_leg():
            with torch.cuda.stream(stream):
                fb.copy_(base)
            s = A.rt_stats()
            check(L.rt_render_extend_device(scene.handle, C.byref(abi1[0]), w, h, args.seed, 0, 0, 1, rows, 0, args.bench_first, fb.data_ptr(), None, sh, None, C.byref(s)))
            return s.kernel_ms

        views_leg(); frame_leg()  # warm-up
        if not torch.equal(fa, fb):
            raise SystemExit("K = 1 differs from the frame's extension")
        kms = {"views": [], "frame": []}
        for _ in range(args.bench_reps):
            kms["views"].append(views_leg())
            kms["frame"].append(frame_leg())
        out["one_view_at_the_bench_frame"] = {"frame": [cols, rows], "from": args.bench_first, "to": args.bench_spp, "kernel_ms": {n: stats_of(v) for n, v in kms.items()},
                                              "views_over_frame_median": round(float(np.median(kms["views"]) / np.median(kms["frame"])), 4)}
        print(json.dumps({"one_view_at_the_bench_frame": out["one_view_at_the_bench_frame"]}), flush=True)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
