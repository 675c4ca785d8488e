"""What camera hits over a batch of views gain over one launch per view (rt_camera_hits_views_device against rt_camera_hits_device), on one GPU.

  (a) small frames   K views (config 2, the three Lambert spheres, its camera turned round the y axis in K steps, as scripts/views_measure.py)
                     of a 71x41 frame, whole frames (no list), n_samples = 1, all three outputs: ONE rt_camera_hits_views_device call
                     against K rt_camera_hits_device calls enqueued back to back on one stream, all with stats == NULL, in this process
                     and on this library; each leg is timed by the host clock around one stream synchronise, the legs alternate after a
                     warm-up, medians of --reps (>= 7) runs.  The batch's outputs are compared with the K calls' before anything is
                     timed.  One extra launch of each leg with statistics gives the time between the launch's own events (for the K
                     calls: summed).
  (b) overhead       K = 1 at the bench frame (config 3, 2401x1601, tuned tree, n_samples = 1) through the views kernel against
                     rt_camera_hits_device: kernel_ms of alternating repetitions -- the price of the variant.

usage: python scripts/camera_hits_views_measure.py [--views 64] [--reps 9] [--bench-reps 7] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from views_measure import stats_of, turntable  # noqa: E402


def same(torch, a, b):
    """bit for bit (doubles as their words: NaNs compare by pattern)"""
    return torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--pixels", type=int, default=20, help="maxHeightCoord of the small frames: 20 is 71x41")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--bench-reps", type=int, default=7)
    ap.add_argument("--bench-pixels", type=int, default=800)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import ray_tracing_fsharp_amd as rt

    A, L = rt._abi, rt.lib
    if rt.device_count() < 1:
        raise SystemExit("camera_hits_views_measure.py needs a GPU")
    out = {}
    stream = torch.cuda.Stream()
    st_handle = stream.cuda_stream

    def buffers(lead):
        with torch.cuda.stream(stream):
            b = (torch.zeros(lead, dtype=torch.int32, device="cuda"), torch.zeros(lead + (3,), dtype=torch.float64, device="cuda"),
                 torch.zeros(lead + (6,), dtype=torch.float64, device="cuda"))
        stream.synchronize()
        return b

    def timed(fn):
        stream.synchronize()
        t0 = time.perf_counter()
        fn()
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e3

    # ---- (a) ----
    objs, cam, w, h = rt.sample_images.config2_three_lambert(spp=100, depth=50, pixels=args.pixels)
    rows, cols = 2 * h + 1, 2 * w + 1
    n, k = rows * cols, args.views
    cams = turntable(rt, cam, k)
    seeds = [args.seed + i for i in range(k)]
    scene = rt.Scene.make(objs)
    batch, single = buffers((k, n, 1)), buffers((k, n, 1))
    abi = (A.rt_camera * k)(*[c.to_abi() for c in cams])
    keys = (C.c_uint64 * k)(*seeds)

    def run_batch(stats=None):
        rt._lib.check(L.rt_camera_hits_views_device(scene.handle, abi, k, w, h, keys, 0, 0, n, None, 0, 1, 0, batch[0].data_ptr(), batch[1].data_ptr(),
                                                    batch[2].data_ptr(), st_handle, None, C.byref(stats) if stats is not None else None))

    def run_singles(stats=False):
        total = 0.0
        for i in range(k):
            s = A.rt_stats() if stats else None
            rt._lib.check(L.rt_camera_hits_device(scene.handle, C.byref(abi[i]), w, h, seeds[i], 0, n, None, 0, 1, 0, single[0][i].data_ptr(),
                                                  single[1][i].data_ptr(), single[2][i].data_ptr(), st_handle, None, C.byref(s) if s is not None else None))
            if s is not None:
                total += s.kernel_ms
        return total

    for _ in range(2):  # warm-up of both legs
        timed(run_batch); timed(run_singles)
    if not all(same(torch, a, b) for a, b in zip(batch, single)):
        raise SystemExit("the batch's views differ from the K calls")
    ms = {"batch": [], "singles": []}
    for _ in range(args.reps):
        ms["batch"].append(timed(run_batch))
        ms["singles"].append(timed(run_singles))
    s = A.rt_stats()
    run_batch(s)
    plan = rt.hooks.last_launch_plan()
    singles_kernel_ms = run_singles(True)
    plan1 = rt.hooks.last_launch_plan()
    out["small_frames"] = {
        "frame": [cols, rows], "views": k, "n_samples": 1, "slots": k * n, "outputs": ["hit_index", "strike", "rays_out"],
        "wall_ms": {name: stats_of(v) for name, v in ms.items()},
        "speedup_median": round(float(np.median(ms["singles"]) / np.median(ms["batch"])), 3),
        "kernel_ms_between_events": {"batch": round(s.kernel_ms, 4), "singles_summed": round(singles_kernel_ms, 4)},
        "plan": {"batch": {"kind": plan["in"]["kind"], "block": plan["out"]["q_block"], "grid": plan["out"]["F_grid"], "chunk": plan["out"]["F_chunk"],
                           "lds": plan["out"]["q_lds"]},
                 "single": {"kind": plan1["in"]["kind"], "block": plan1["out"]["q_block"], "grid": plan1["out"]["F_grid"], "chunk": plan1["out"]["F_chunk"],
                            "lds": plan1["out"]["q_lds"]}},
    }
    print(json.dumps(out["small_frames"]), flush=True)

    # ---- (b) ----
    if args.bench_reps > 0:
        objs, cam, w, h = rt.sample_images.config3_final(seed=args.seed, spp=500, depth=50, pixels=args.bench_pixels)
        rows, cols = 2 * h + 1, 2 * w + 1
        n = rows * cols
        scene = rt.Scene.make(objs)
        scene.tune(w, h, cam, seed=args.seed ^ 0x5EED, device=0)
        fa, fb = buffers((1, n, 1)), buffers((n, 1))
        abi1 = (A.rt_camera * 1)(cam.to_abi())

        def views_leg():
            s = A.rt_stats()
            rt._lib.check(L.rt_camera_hits_views_device(scene.handle, abi1, 1, w, h, None, args.seed, 0, n, None, 0, 1, 0, fa[0].data_ptr(), fa[1].data_ptr(),
                                                        fa[2].data_ptr(), st_handle, None, C.byref(s)))
            return s.kernel_ms

        def single_leg():
            s = A.rt_stats()
            rt._lib.check(L.rt_camera_hits_device(scene.handle, C.byref(abi1[0]), w, h, args.seed, 0, n, None, 0, 1, 0, fb[0].data_ptr(), fb[1].data_ptr(),
                                                  fb[2].data_ptr(), st_handle, None, C.byref(s)))
            return s.kernel_ms

        views_leg(); single_leg()  # warm-up
        if not all(same(torch, a[0], b) for a, b in zip(fa, fb)):
            raise SystemExit("K = 1 differs from rt_camera_hits_device")
        kms = {"views": [], "single": []}
        for _ in range(args.bench_reps):
            kms["views"].append(views_leg())
            kms["single"].append(single_leg())
        out["one_view_at_the_bench_frame"] = {"frame": [cols, rows], "n_samples": 1, "kernel_ms": {name: stats_of(v) for name, v in kms.items()},
                                              "views_over_single_median": round(float(np.median(kms["views"]) / np.median(kms["single"])), 4)}
        print(json.dumps(out["one_view_at_the_bench_frame"]), flush=True)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
