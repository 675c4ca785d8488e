"""What the output stage costs by each route, on one GPU: the bench frame (config 3, 2401x1601, tuned tree), gamma on, the image a real
render at a reduced sample count so that the digit counts are a frame's --

  (a) host route      device-to-host copy of rgb, then rt_format_ppm on one host thread (the code every caller ran before)
  (b) device kernels  rt_format_ppm_device alone, between two events on the stream: sums, scan, scatter; and the length-only call
                      (sums and scan) to tell the scatter's share; bytes moved, bytes/s, share of the 6.3 TB/s streaming rate, and the
                      three kernel boundaries at the 1.45 - 1.9 us each that the microarchitecture notes price them at
  (c) device route    (b) and the device-to-host copy of exactly the text (to pageable host memory, as rt_write_ppm_device does it, and
                      to pinned memory), the copy reported apart from the kernels
  (d) file writes     rt_write_ppm of the host rgb against rt_write_ppm_device of the device rgb, into the same directory
  (e) end to end      rt_render + rt_write_ppm against rt_render_ppm, wall clock, at the bench configuration

The bytes of both routes are compared before anything is timed.  Warm-up first, medians of --reps, the two routes alternating.  No
threshold is set: the figures go to profiles/ and NOTES.md.

usage: python scripts/output_measure.py [--pixels 800] [--spp 20] [--bench-spp 500] [--reps 7] [--dir DIR] [--out FILE]"""
import argparse
import ctypes as C
import dataclasses
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_RATE = 6.3e12       # bytes/s a streaming kernel achieves on an MI355X
BOUNDARY_US = (1.45, 1.9)  # one dependent kernel boundary on a stream: trivial kernels, real streaming kernels


def median_ms(xs):
    return 1e3 * float(np.median(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pixels", type=int, default=800)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--spp", type=int, default=20)
    ap.add_argument("--bench-spp", type=int, default=500)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dir", default=None, help="directory for the files of (d) and (e); default: a temporary one")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import ray_tracing_fsharp_amd as rt
    from ray_tracing_fsharp_amd import _abi as A
    from ray_tracing_fsharp_amd._lib import check

    lib = rt.lib
    objs, cam, w, h = rt.sample_images.config3_final(seed=args.seed, spp=args.bench_spp, depth=50, pixels=args.pixels)
    rows, cols = 2 * h + 1, 2 * w + 1
    scene = rt.Scene.make(objs)
    scene.tune(w, h, cam, seed=args.seed ^ 0x5EED, device=0)
    low = dataclasses.replace(cam, SamplesPerPixel=args.spp)
    low_abi, cam_abi = low.to_abi(), cam.to_abi()
    stream = torch.cuda.current_stream().cuda_stream
    d_accum = torch.zeros((rows, cols, 4), dtype=torch.int32, device="cuda")
    d_rgb = torch.zeros((rows, cols, 3), dtype=torch.uint8, device="cuda")
    st = A.rt_stats()
    check(lib.rt_render_device(scene.handle, C.byref(low_abi), w, h, args.seed, 0, 0, 1, rows, 0, d_accum.data_ptr(), d_rgb.data_ptr(), stream, C.byref(st)))

    cap = int(lib.rt_ppm_max_bytes(rows, cols))
    host_text = C.create_string_buffer(cap + 1)
    d_text = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros((), dtype=torch.int64, device="cuda")
    pinned = torch.empty(cap, dtype=torch.uint8).pin_memory()
    u8p = C.POINTER(C.c_uint8)

    def host_route():
        t0 = time.perf_counter()
        rgb = d_rgb.cpu().numpy()
        t1 = time.perf_counter()
        n = lib.rt_format_ppm(rgb.ctypes.data_as(u8p), rows, cols, 1, host_text, cap + 1)
        t2 = time.perf_counter()
        return rgb, int(n), t1 - t0, t2 - t1

    def device_kernels(with_out=True):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        check(lib.rt_format_ppm_device(0, d_rgb.data_ptr(), rows, cols, 1, d_text.data_ptr() if with_out else None, cap if with_out else 0, d_len.data_ptr(),
                                       stream, None))
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3

    def device_route(pin):
        t0 = time.perf_counter()
        check(lib.rt_format_ppm_device(0, d_rgb.data_ptr(), rows, cols, 1, d_text.data_ptr(), cap, d_len.data_ptr(), stream, None))
        n = int(d_len)  # waits for the kernels
        t1 = time.perf_counter()
        if pin:
            pinned[:n].copy_(d_text[:n], non_blocking=True)
            torch.cuda.synchronize()
            text = pinned[:n]
        else:
            text = d_text[:n].cpu()
        t2 = time.perf_counter()
        return text, n, t1 - t0, t2 - t1

    # equal bytes first
    rgb, n_host, _, _ = host_route()
    text, n_dev, _, _ = device_route(False)
    equal = n_host == n_dev and host_text.raw[:n_host] == text.numpy().tobytes()
    result = {"frame": [cols, rows], "image_spp": args.spp, "gamma": True, "reps": args.reps, "text_bytes": n_dev, "rgb_bytes": rows * cols * 3,
              "outputs_equal": bool(equal)}
    if not equal:
        result["error"] = "the two routes disagree; nothing timed"
    else:
        for _ in range(2):  # warm-up
            host_route(); device_kernels(); device_kernels(False); device_route(False); device_route(True)
        a_copy, a_fmt, b_all, b_len, c_k, c_copy, c_kp, c_copyp = [], [], [], [], [], [], [], []
        for _ in range(args.reps):  # alternating
            _, _, tc, tf = host_route(); a_copy.append(tc); a_fmt.append(tf)
            b_all.append(device_kernels()); b_len.append(device_kernels(False))
            _, _, tk, tc = device_route(False); c_k.append(tk); c_copy.append(tc)
            _, _, tk, tc = device_route(True); c_kp.append(tk); c_copyp.append(tc)
        n_tiles = (rows * cols + 1023) // 1024
        moved = 2 * rows * cols * 3 + n_dev + 3 * 8 * n_tiles  # rgb read by the sums and by the scatter, the text, the tile array written, scanned, read
        k = float(np.median(b_all))
        result["a_host_route"] = {"copy_rgb_ms": median_ms(a_copy), "rt_format_ppm_ms": median_ms(a_fmt),
                                  "total_ms": median_ms([x + y for x, y in zip(a_copy, a_fmt)])}
        result["b_device_kernels"] = {"three_kernels_ms": 1e3 * k, "all_runs_ms": sorted(1e3 * x for x in b_all), "sums_and_scan_ms": median_ms(b_len),
                                      "bytes_moved": moved, "bytes_per_s": moved / k, "share_of_streaming_rate": moved / k / STREAM_RATE,
                                      "streaming_floor_ms": 1e3 * moved / STREAM_RATE,
                                      "three_boundaries_priced_us": [3 * BOUNDARY_US[0], 3 * BOUNDARY_US[1]]}
        result["c_device_route"] = {"pageable": {"launch_to_length_ms": median_ms(c_k), "copy_text_ms": median_ms(c_copy),
                                                 "total_ms": median_ms([x + y for x, y in zip(c_k, c_copy)])},
                                    "pinned": {"launch_to_length_ms": median_ms(c_kp), "copy_text_ms": median_ms(c_copyp),
                                               "total_ms": median_ms([x + y for x, y in zip(c_kp, c_copyp)])}}
        result["c_faster_than_a"] = result["c_device_route"]["pageable"]["total_ms"] < result["a_host_route"]["total_ms"]

        with tempfile.TemporaryDirectory(dir=args.dir) as d:
            p_host, p_dev = os.path.join(d, "host.ppm").encode(), os.path.join(d, "device.ppm").encode()
            d_host, d_dev = [], []
            for i in range(args.reps + 1):  # (the first round warms up)
                t0 = time.perf_counter(); check(lib.rt_write_ppm(p_host, rgb.ctypes.data_as(u8p), rows, cols, 1)); t1 = time.perf_counter()
                check(lib.rt_write_ppm_device(p_dev, 0, d_rgb.data_ptr(), rows, cols, 1, stream)); t2 = time.perf_counter()
                if i:
                    d_host.append(t1 - t0); d_dev.append(t2 - t1)
            same = open(p_host, "rb").read() == open(p_dev, "rb").read()
            result["d_file_writes"] = {"rt_write_ppm_ms": median_ms(d_host), "rt_write_ppm_device_ms": median_ms(d_dev), "files_equal": bool(same)}

            accum = np.zeros((rows, cols, 4), np.int32)
            rgb_e = np.zeros((rows, cols, 3), np.uint8)
            e_host, e_dev, k_host, k_dev = [], [], [], []
            for i in range(min(args.reps, 5) + 1):
                t0 = time.perf_counter()
                check(lib.rt_render(scene.handle, C.byref(cam_abi), w, h, args.seed, 0, 0, 1, rows, 0, accum.ctypes.data_as(C.POINTER(C.c_int32)),
                                    rgb_e.ctypes.data_as(u8p), C.byref(st)))
                check(lib.rt_write_ppm(p_host, rgb_e.ctypes.data_as(u8p), rows, cols, 1))
                t1 = time.perf_counter()
                kh = st.kernel_ms
                check(lib.rt_render_ppm(scene.handle, C.byref(cam_abi), w, h, args.seed, 0, 0, 1, p_dev, None, C.byref(st)))
                t2 = time.perf_counter()
                if i:
                    e_host.append(t1 - t0); e_dev.append(t2 - t1); k_host.append(kh); k_dev.append(st.kernel_ms)
            same = open(p_host, "rb").read() == open(p_dev, "rb").read()
            result["e_end_to_end"] = {"spp": args.bench_spp, "rt_render_then_rt_write_ppm_ms": median_ms(e_host), "rt_render_ppm_ms": median_ms(e_dev),
                                      "kernel_ms_host_route": float(np.median(k_host)), "kernel_ms_device_route": float(np.median(k_dev)),
                                      "files_equal": bool(same)}
    text = json.dumps(result, indent=1)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if result["outputs_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
