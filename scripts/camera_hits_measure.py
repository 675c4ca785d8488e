"""What rt_camera_hits saves a caller, on one GPU: the first hit of every pixel sample of the bench frame (config 3, 2401x1601, tuned
tree), strike and rays_out not asked for, at n_samples 1, 4 and 16 --

  (a) library   rt_camera_hits_device over the whole frame (no list): nothing is uploaded
  (b) caller    what could be done before this entry point: the same rays composed OUTSIDE the library -- the stream keying and
                Scene.traceOnce's ray arithmetic (Scene.fs:129-143) restated in numpy, in the order written -- uploaded (48 bytes a
                ray) and passed to rt_hit_objects_device, which walks the tree from the root for every ray

The hit indices of (b) are checked against (a)'s before anything is timed.  Reported per n_samples: kernel_ms of both (median of
--reps), the bytes uploaded, the host's time to compose, the upload and the wall time of one call of each.  No threshold is set.

usage: python scripts/camera_hits_measure.py [--pixels 800] [--reps 5] [--samples 1 4 16] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def get_two(seed, g, s):
    """GetTwo of the stream keyed (seed, g, s) for arrays g, s: the keying of include/rtfs_amd.h, xorshift128, byte reversal."""
    with np.errstate(over="ignore"):
        k = mix64(np.uint64(seed) + GOLDEN)
        hp = mix64(k ^ (g.astype(np.uint64) * np.uint64(0xD1B54A32D192ED03) + np.uint64(0x8CB92BA72F3D8DD7)))
        s64 = s.astype(np.uint64)
        a = mix64(hp + (np.uint64(2) * s64 + np.uint64(1)) * GOLDEN)
        b = mix64(hp + (np.uint64(2) * s64 + np.uint64(2)) * GOLDEN)
    m = np.uint64(2147483647)
    x = ((a & np.uint64(0xFFFFFFFF)) % m).astype(np.uint32)
    y = ((a >> np.uint64(32)) % m).astype(np.uint32)
    z = ((b & np.uint64(0xFFFFFFFF)) % m).astype(np.uint32)
    w = ((b >> np.uint64(32)) % m).astype(np.uint32)
    w[(x == 0) & (y == 0) & (z == 0) & (w == 0)] = 1
    out = []
    for _ in range(2):
        t = x ^ (x << np.uint32(11))
        x, y, z = y, z, w
        w = w ^ (w >> np.uint32(19)) ^ (t ^ (t >> np.uint32(8)))
        out.append(w.byteswap().astype(np.float64) / np.float64(0xFFFFFFFF))
    return out


def compose(cam, max_w, max_h, seed, n_samples):
    """rays [rows*cols*n_samples, 6] (origin, vector: Ray.make' is rt_hit_objects'), samples innermost"""
    rows, cols = 2 * max_h + 1, 2 * max_w + 1
    g = np.repeat(np.arange(rows * cols, dtype=np.int64), n_samples)
    s = np.tile(np.arange(n_samples, dtype=np.int64), rows * cols)
    r1, r2 = get_two(seed, g, s)
    r, c = np.divmod(g, cols)
    row, col = (max_h - r - 1).astype(np.float64), (c - max_w).astype(np.float64)
    eye, xo, xd, yd = (np.array(list(v), np.float64) for v in (cam.view_origin, cam.xaxis_origin, cam.xaxis_dir, cam.yaxis_dir))
    landing = ((col + r1) * np.float64(cam.viewport_width)) / np.float64(max_w)
    walk = ((row + r2) * np.float64(cam.viewport_height)) / np.float64(max_h)
    rays = np.empty((len(g), 6), np.float64)
    for a in range(3):
        on_x = xo[a] + (xd[a] * landing)
        end = on_x + (yd[a] * walk)
        rays[:, a] = eye[a]
        rays[:, 3 + a] = end - eye[a]
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pixels", type=int, default=800)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import ray_tracing_fsharp_amd as rt
    from ray_tracing_fsharp_amd import _abi as A
    from ray_tracing_fsharp_amd._lib import check

    objs, cam, w, h = rt.sample_images.config3_final(seed=args.seed, spp=500, depth=50, pixels=args.pixels)
    rows, cols = 2 * h + 1, 2 * w + 1
    scene = rt.Scene.make(objs)
    scene.tune(w, h, cam, seed=args.seed ^ 0x5EED, device=0)
    result = {"frame": [cols, rows], "tuned": True, "reps": args.reps, "legs": []}
    for per in args.samples:
        t0 = time.perf_counter()
        rays = compose(cam.to_abi(), w, h, args.seed, per)
        t_compose = time.perf_counter() - t0
        t0 = time.perf_counter()
        d_rays = torch.from_numpy(rays).cuda()
        torch.cuda.synchronize()
        t_upload = time.perf_counter() - t0

        def library():
            return scene.cameraHits(w, h, cam, None, n_samples=per, seed=args.seed, strike=False, rays=False, tensors=True)

        hit_b = torch.empty(len(rays), dtype=torch.int32, device="cuda")

        def caller():  # (no strike either: like for like)
            st = A.rt_stats()
            check(rt.lib.rt_hit_objects_device(scene.handle, 0, len(rays), d_rays.data_ptr(), 0, hit_b.data_ptr(), None,
                                               torch.cuda.current_stream().cuda_stream, None, C.byref(st)))
            return st.kernel_ms

        lib, _ = library(), caller()  # warm-up, and the check: equal outputs first
        torch.cuda.synchronize()
        equal = bool(torch.equal(lib.hit_index.reshape(-1), hit_b))
        leg = {"n_samples": per, "slots": rows * cols * per, "outputs_equal": equal, "bytes_uploaded_library": 0, "bytes_uploaded_caller": int(rays.nbytes),
               "caller_compose_s": round(t_compose, 3), "caller_upload_s": round(t_upload, 3)}
        if not equal:
            leg["error"] = "the two routes disagree; nothing timed"
            result["legs"].append(leg)
            continue
        k_lib, k_call, w_lib, w_call = [], [], [], []
        for _ in range(args.reps):  # alternating
            t0 = time.perf_counter(); library(); torch.cuda.synchronize(); w_lib.append(time.perf_counter() - t0)
            k_lib.append(scene.last_stats["kernel_ms"])
            t0 = time.perf_counter(); ms = caller(); torch.cuda.synchronize(); w_call.append(time.perf_counter() - t0)
            k_call.append(ms)
        leg.update(kernel_ms_library=sorted(k_lib), kernel_ms_caller=sorted(k_call), kernel_ms_library_median=float(np.median(k_lib)),
                   kernel_ms_caller_median=float(np.median(k_call)), wall_ms_library_median=1e3 * float(np.median(w_lib)),
                   wall_ms_caller_call_median=1e3 * float(np.median(w_call)),
                   wall_ms_caller_with_compose_and_upload=1e3 * (float(np.median(w_call)) + t_compose + t_upload))
        result["legs"].append(leg)
        print(json.dumps(leg), flush=True)
        del rays, d_rays, hit_b, lib
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if all(leg["outputs_equal"] for leg in result["legs"]) else 1


if __name__ == "__main__":
    sys.exit(main())
