"""What the path records cost, on one GPU, on the bench frame (config 3, 2401x1601, tuned tree).  Nothing here is a bar.

  (a) no stage scheduler   rt_trace_paths_device with `colour` alone against rt_trace_rays_device, on the SAME device rays (the frame's
                           camera rays at one sample, from rt_camera_hits_device's rays_out), alternating, medians of --reps
  (b) the two routes       the frame's summary alone at --summary-samples samples (16: 61.5 M slots): ms and paths/s with the scene in
                           LDS (the filter loop) and with the global-memory route forced (RTFS_PATHS_ROUTE=global), alternating
  (c) records              max_vertices 0 against 8, every per-record output, at about 1 M slots

Colours of (a) and summaries of (b) are checked for equality before anything is reported.

usage: python scripts/paths_measure.py [--pixels 800] [--reps 7] [--summary-samples 16] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pixels", type=int, default=800)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--summary-samples", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import ray_tracing_fsharp_amd as rt
    from ray_tracing_fsharp_amd import _abi as A
    from ray_tracing_fsharp_amd._lib import check

    objs, cam, w, h = rt.sample_images.config3_final(seed=args.seed, spp=500, depth=50, pixels=args.pixels)
    rows, cols = 2 * h + 1, 2 * w + 1
    n = rows * cols
    scene = rt.Scene.make(objs)
    scene.tune(w, h, cam, seed=args.seed ^ 0x5EED, device=0)
    stream = torch.cuda.current_stream().cuda_stream
    result = {"frame": [cols, rows], "tuned": True, "reps": args.reps}

    def med(xs):
        return float(np.median(xs))

    # ---- (a) the same rays through rt_trace_rays_device and rt_trace_paths_device
    d_rays = scene.cameraHits(w, h, cam, None, n_samples=1, seed=args.seed, strike=False, rays=True, tensors=True).rays.reshape(n, 6).contiguous()
    col_a = torch.empty((n, 3), dtype=torch.uint8, device="cuda")
    col_b = torch.empty((n, 3), dtype=torch.uint8, device="cuda")
    out_b = A.rt_path_outputs(max_vertices=0, colour=col_b.data_ptr())

    def rays_call():
        st = A.rt_stats()
        check(rt.lib.rt_trace_rays_device(scene.handle, 0, n, d_rays.data_ptr(), None, args.seed, 0, 0, cam.BounceDepth, 0, col_a.data_ptr(), stream, None, C.byref(st)))
        return st.kernel_ms

    def paths_call():
        st = A.rt_stats()
        check(rt.lib.rt_trace_paths_device(scene.handle, 0, n, d_rays.data_ptr(), None, args.seed, 0, 0, cam.BounceDepth, 0, C.byref(out_b), stream, None, C.byref(st)))
        return st.kernel_ms

    rays_call(), paths_call()
    equal = bool(torch.equal(col_a, col_b))
    ka, kb = [], []
    for _ in range(args.reps):
        ka.append(rays_call())
        kb.append(paths_call())
    result["trace_rays_vs_paths"] = {"rays": n, "colours_equal": equal, "kernel_ms_trace_rays": sorted(ka), "kernel_ms_trace_paths": sorted(kb),
                                     "median_trace_rays": med(ka), "median_trace_paths": med(kb), "ratio_paths_over_rays": med(kb) / med(ka),
                                     "plan": rt.hooks.last_paths_plan()}
    print(json.dumps(result["trace_rays_vs_paths"]), flush=True)
    del col_a, col_b

    # ---- (b) the frame's summary, LDS route against the global route forced
    per = args.summary_samples

    cam_abi = cam.to_abi()

    def summary_call(route):  # the summary ALONE: no per-slot output is asked for
        words = torch.empty((n, A.RT_PATH_SUMMARY_WORDS), dtype=torch.int32, device="cuda")
        out = A.rt_path_outputs(max_vertices=0, summary=words.data_ptr())
        st = A.rt_stats()
        if route == "global":
            os.environ["RTFS_PATHS_ROUTE"] = "global"
        try:
            check(rt.lib.rt_camera_paths_device(scene.handle, C.byref(cam_abi), w, h, args.seed, 0, n, None, 0, per, 0, C.byref(out), stream, None, C.byref(st)))
        finally:
            os.environ.pop("RTFS_PATHS_ROUTE", None)
        return (words, st.kernel_ms), rt.hooks.last_paths_plan()

    (s_lds, p_lds), (s_glb, p_glb) = summary_call("lds"), summary_call("global")
    equal = bool(torch.equal(s_lds[0], s_glb[0]))
    kl, kg = [], []
    for _ in range(args.reps):
        kl.append(summary_call("lds")[0][1])
        kg.append(summary_call("global")[0][1])
    slots = n * per
    result["summary_routes"] = {"n_samples": per, "slots": slots, "summaries_equal": equal, "plan_lds": p_lds, "plan_global": p_glb,
                                "kernel_ms_lds": sorted(kl), "kernel_ms_global": sorted(kg), "median_lds": med(kl), "median_global": med(kg),
                                "paths_per_s_lds": slots / (med(kl) * 1e-3), "paths_per_s_global": slots / (med(kg) * 1e-3),
                                "spread_lds": max(kl) - min(kl), "spread_global": max(kg) - min(kg),
                                "mean_vertices": float(s_lds[0][:, 1].sum().item()) / slots}
    print(json.dumps(result["summary_routes"]), flush=True)
    del s_lds, s_glb

    # ---- (c) records: K = 0 against K = 8 at about 1 M slots
    px = torch.arange(0, n, max(1, n // 62500), dtype=torch.int32, device="cuda")[:62500].contiguous()
    k0, k8 = [], []
    for _ in range(args.reps + 1):
        k0.append(scene.cameraPaths(w, h, cam, px, n_samples=16, max_vertices=0, records=False, first_ray=False, seed=args.seed).stats["kernel_ms"])
        k8.append(scene.cameraPaths(w, h, cam, px, n_samples=16, max_vertices=8, seed=args.seed).stats["kernel_ms"])
    result["records"] = {"slots": int(px.numel()) * 16, "kernel_ms_k0": sorted(k0[1:]), "kernel_ms_k8": sorted(k8[1:]), "median_k0": med(k0[1:]), "median_k8": med(k8[1:])}
    print(json.dumps(result["records"]), flush=True)

    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if result["trace_rays_vs_paths"]["colours_equal"] and equal else 1


if __name__ == "__main__":
    sys.exit(main())
