"""What reading a pixel map back costs by each route, on one GPU: the bench frame's map (config 3, 2401x1601, tuned tree; the image a real
render at a reduced sample count; the map rt_format_pixel_map's bytes of it) --

  (a) host route      rt_parse_pixel_map on one host thread (the code every caller ran before), plus the upload of its rgb
  (b) parse kernels   rt_parse_pixel_map_device alone, between two events on the stream: the memset of the scratch and five launches; bytes
                      moved, bytes/s and the share of the 6.3 TB/s streaming rate
  (c) device route    upload of the map's bytes (from pageable host memory), then (b), until the count is on the host
  (d) resume          rt_resume_pixel_map of the map with every second row missing, against rt_render of the whole frame and against
                      rt_render_pixels of the same list alone, at the image's sample count

The results of both routes are compared before anything is timed.  Warm-up first, medians of --reps, the routes alternating.  The one
comparison that is asked for is (c) against (a) in the same run; no threshold is set: the figures go to profiles/ and NOTES.md.

usage: python scripts/pixel_map_measure.py [--pixels 800] [--spp 20] [--reps 7] [--out FILE]"""
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

STREAM_RATE = 6.3e12  # bytes/s a streaming kernel achieves on an MI355X


def median_ms(xs):
    return 1e3 * float(np.median(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pixels", type=int, default=800)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--spp", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import ray_tracing_fsharp_amd as rt
    from ray_tracing_fsharp_amd import _abi as A
    from ray_tracing_fsharp_amd._lib import check

    lib = rt.lib
    u8p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    objs, cam, w, h = rt.sample_images.config3_final(seed=args.seed, spp=args.spp, depth=50, pixels=args.pixels)
    rows, cols = 2 * h + 1, 2 * w + 1
    npx = rows * cols
    scene = rt.Scene.make(objs)
    scene.tune(w, h, cam, seed=args.seed ^ 0x5EED, device=0)
    cam_abi = cam.to_abi()
    st = A.rt_stats()
    accum = np.zeros((rows, cols, 4), np.int32)
    frame = np.zeros((rows, cols, 3), np.uint8)
    check(lib.rt_render(scene.handle, C.byref(cam_abi), w, h, args.seed, 0, 0, 1, rows, 0, accum.ctypes.data_as(i32p), frame.ctypes.data_as(u8p), C.byref(st)))
    n_map = int(lib.rt_pixel_map_bytes(rows, cols))
    map_buf = C.create_string_buffer(n_map)
    assert lib.rt_format_pixel_map(frame.ctypes.data_as(u8p), rows, cols, map_buf, n_map) == n_map
    map_np = np.frombuffer(map_buf, np.uint8, n_map)

    stream = torch.cuda.current_stream().cuda_stream
    d_map = torch.empty(n_map, dtype=torch.uint8, device="cuda")
    d_rgb = torch.zeros((rows, cols, 3), dtype=torch.uint8, device="cuda")
    d_present = torch.zeros((rows, cols), dtype=torch.uint8, device="cuda")
    d_count = torch.zeros((), dtype=torch.int64, device="cuda")
    host_rgb = np.zeros((rows, cols, 3), np.uint8)
    host_present = np.zeros((rows, cols), np.uint8)
    map_t = torch.from_numpy(map_np)  # pageable host memory

    def host_route():
        t0 = time.perf_counter()
        n = lib.rt_parse_pixel_map(map_buf, n_map, rows, cols, host_rgb.ctypes.data_as(u8p), host_present.ctypes.data_as(u8p))
        t1 = time.perf_counter()
        d_rgb.copy_(torch.from_numpy(host_rgb))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return int(n), t1 - t0, t2 - t1

    def parse_kernels():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        check(lib.rt_parse_pixel_map_device(0, d_map.data_ptr(), n_map, rows, cols, d_rgb.data_ptr(), d_present.data_ptr(), d_count.data_ptr(), stream, None))
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3

    def device_route():
        n = C.c_int64(0)
        t0 = time.perf_counter()
        d_map.copy_(map_t)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        check(lib.rt_parse_pixel_map_device(0, d_map.data_ptr(), n_map, rows, cols, d_rgb.data_ptr(), d_present.data_ptr(), None, stream, C.byref(n)))
        t2 = time.perf_counter()
        return n.value, t1 - t0, t2 - t1

    # equal results first
    n_host, _, _ = host_route()
    d_rgb.zero_()
    n_dev, _, _ = device_route()
    equal = (n_host == n_dev == npx and np.array_equal(d_rgb.cpu().numpy(), host_rgb) and np.array_equal(d_present.cpu().numpy(), host_present)
             and np.array_equal(host_rgb, frame))
    result = {"frame": [cols, rows], "image_spp": args.spp, "reps": args.reps, "map_bytes": n_map, "records": npx, "results_equal": bool(equal)}
    if not equal:
        result["error"] = "the two routes disagree; nothing timed"
    else:
        for _ in range(2):  # warm-up
            host_route(); parse_kernels(); device_route()
        a_parse, a_up, b_all, c_up, c_parse = [], [], [], [], []
        for _ in range(args.reps):  # alternating
            _, tp, tu = host_route(); a_parse.append(tp); a_up.append(tu)
            b_all.append(parse_kernels())
            _, tu, tp = device_route(); c_up.append(tu); c_parse.append(tp)
        tile = lib.rt_pixel_map_tile_bytes()
        n_tiles = (n_map + tile - 1) // tile
        # the map read by the three tile kernels and once more record by record, by both record passes; the winner words zeroed, claimed, read by the
        # store pass and by the finish; rgb and present written; a 24-byte map per tile written and scanned, an 8-byte entry written and read twice
        moved = 3 * n_map + 2 * n_map + 4 * 4 * npx + 3 * npx + npx + n_tiles * (2 * 24 + 3 * 8)
        k = float(np.median(b_all))
        result["a_host_route"] = {"rt_parse_pixel_map_ms": median_ms(a_parse), "upload_rgb_ms": median_ms(a_up),
                                  "total_ms": median_ms([x + y for x, y in zip(a_parse, a_up)])}
        result["b_parse_kernels"] = {"memset_and_five_kernels_ms": 1e3 * k, "all_runs_ms": sorted(1e3 * x for x in b_all), "bytes_moved": moved,
                                     "bytes_per_s": moved / k, "share_of_streaming_rate": moved / k / STREAM_RATE, "streaming_floor_ms": 1e3 * moved / STREAM_RATE}
        result["c_device_route"] = {"upload_map_ms": median_ms(c_up), "parse_to_count_ms": median_ms(c_parse),
                                    "total_ms": median_ms([x + y for x, y in zip(c_up, c_parse)])}
        result["c_faster_than_a"] = result["c_device_route"]["total_ms"] < result["a_host_route"]["total_ms"]
        result["a_over_c"] = result["a_host_route"]["total_ms"] / result["c_device_route"]["total_ms"]

        # (d) every second row missing
        digits = lambda v: len(str(v)) if v else 0  # noqa: E731  (writeAsciiInt: no digit for 0)
        col_digits = sum(digits(c) for c in range(cols))
        row_end = np.cumsum([cols * (digits(r) + 5) + col_digits for r in range(rows)])  # the map is row-major: a row is one byte range
        assert row_end[-1] == n_map
        raw = map_buf.raw
        half = b"".join(raw[(row_end[r - 1] if r else 0):row_end[r]] for r in range(0, rows, 2))
        keep = np.repeat(np.arange(rows) % 2 == 0, cols)
        missing = np.flatnonzero(~keep).astype(np.int32)
        out = np.zeros((rows, cols, 3), np.uint8)
        l_accum, l_rgb = np.zeros((missing.size, 4), np.int32), np.zeros((missing.size, 3), np.uint8)
        d_res, d_full, d_list, k_res, k_full, k_list = [], [], [], [], [], []
        for i in range(min(args.reps, 5) + 1):  # (the first round warms up)
            t0 = time.perf_counter()
            check(lib.rt_resume_pixel_map(scene.handle, C.byref(cam_abi), w, h, args.seed, 0, 0, half, len(half), out.ctypes.data_as(u8p), None, C.byref(st)))
            t1 = time.perf_counter(); kr = st.kernel_ms
            check(lib.rt_render(scene.handle, C.byref(cam_abi), w, h, args.seed, 0, 0, 1, rows, 0, accum.ctypes.data_as(i32p), host_rgb.ctypes.data_as(u8p), C.byref(st)))
            t2 = time.perf_counter(); kf = st.kernel_ms
            check(lib.rt_render_pixels(scene.handle, C.byref(cam_abi), w, h, args.seed, 0, missing.size, missing.ctypes.data_as(i32p), 0, l_accum.ctypes.data_as(i32p),
                                       l_rgb.ctypes.data_as(u8p), C.byref(st)))
            t3 = time.perf_counter()
            if i:
                d_res.append(t1 - t0); d_full.append(t2 - t1); d_list.append(t3 - t2); k_res.append(kr); k_full.append(kf); k_list.append(st.kernel_ms)
        result["d_resume_half"] = {"map_bytes": len(half), "pixels_missing": int(missing.size), "frame_equal": bool(np.array_equal(out, frame)),
                                   "rt_resume_pixel_map_ms": median_ms(d_res), "rt_render_whole_frame_ms": median_ms(d_full),
                                   "rt_render_pixels_same_list_ms": median_ms(d_list), "kernel_ms": {"resume": float(np.median(k_res)),
                                   "whole_frame": float(np.median(k_full)), "same_list": float(np.median(k_list))}}
    text = json.dumps(result, indent=1)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if result["results_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
