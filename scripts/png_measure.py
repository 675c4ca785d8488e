"""What Png.write costs and how large its files are.

  --sizes   (no GPU) the host formatter rt_format_png over the four golden frames of tests/golden/, gamma on: IDAT bytes against
            zlib.compressobj(6, strategy=Z_RLE) and zlib's default strategy over the same Sub-filtered bytes, the block types chosen, and
            what a per-row adaptive filter choice could save at most (every row filtered by the best of the five types under zlib's
            default strategy -- an upper bound on the gain, not an encoder).  --frame FILE.npy adds a frame of one's own (bench.py
            --dump-outputs writes rgb.npy).
  default   on one GPU, the bench frame (config 3, 2401x1601, tuned tree), gamma on, the image a real render at a reduced sample count --
            (a) host route      device-to-host copy of rgb, then rt_format_png on one host thread
            (b) device kernels  rt_format_png_device between two events on the stream: four launches; and the length-only call (sums and
                                scan alone), which splits the time into sums + scan and scatter + finish.  Events cannot be placed between
                                the launches from outside the library: the per-kernel times come from a kernel trace of this script
                                (rocprofv3 --kernel-trace --stats -- python scripts/png_measure.py)
            (c) sizes           the file beside the P3 text's, and against zlib as under --sizes
            (d) end to end      rt_render_png beside rt_render_ppm, wall clock, at the bench configuration
The bytes of both routes are compared before anything is timed.  Warm-up first, medians of --reps.  No threshold is set: the figures go
to profiles/ and NOTES.md.

usage: python scripts/png_measure.py [--sizes] [--frame FILE.npy] [--pixels 800] [--spp 20] [--bench-spp 500] [--reps 7] [--out FILE]"""
import argparse
import ctypes as C
import dataclasses
import json
import os
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median_ms(xs):
    return 1e3 * float(np.median(xs))


def sub_filtered(px):
    d = px.astype(np.int16)
    d[:, 1:] -= px[:, :-1].astype(np.int16)
    return b"".join(b"\x01" + (row & 255).astype(np.uint8).tobytes() for row in d)


def best_filter_bound(px):
    """Every row under the filter type whose row compresses best on its own (zlib default): a bound on what adaptive filtering could gain."""
    rows = px.shape[0]
    flat = px.reshape(rows, -1).astype(np.int16)
    out = []
    for r in range(rows):
        cur, up = flat[r], flat[r - 1] if r else np.zeros_like(flat[0])
        left = np.concatenate([np.zeros(3, np.int16), cur[:-3]])
        upleft = np.concatenate([np.zeros(3, np.int16), up[:-3]])
        p = left + up - upleft
        pa, pb, pc = abs(p - left), abs(p - up), abs(p - upleft)
        paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
        cands = [cur, cur - left, cur - up, cur - (left + up) // 2, cur - paeth]
        rows_b = [bytes([t]) + (c & 255).astype(np.uint8).tobytes() for t, c in enumerate(cands)]
        out.append(min(rows_b, key=lambda b: len(zlib.compress(b, 6))))
    return len(zlib.compress(b"".join(out), 6))


def sizes_of(rt, name, rgb):
    import png_cases as pc

    lut = np.array([rt.lib.rt_gamma_correct(b) for b in range(256)], np.uint8)
    data = rt.Png.format(True, rgb)
    px, idat = pc.decode(data)
    assert np.array_equal(px, lut[rgb])
    raw = sub_filtered(px)
    rle = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    z_rle, z_default = len(rle.compress(raw) + rle.flush()), len(zlib.compress(raw, 6))
    small = len(raw) <= 4 << 20  # (the block walk feeds a decoder byte by byte)
    types = pc.tile_block_types(idat, len(raw), rt.lib.rt_png_tile_bytes()) if small else None
    return {"name": name, "shape": [int(rgb.shape[0]), int(rgb.shape[1])], "file_bytes": len(data), "idat_bytes": len(idat), "filtered_bytes": len(raw),
            "zlib_rle_bytes": z_rle, "zlib_default_bytes": z_default, "excess_over_zlib_rle": len(idat) / z_rle - 1.0,
            "excess_over_zlib_default": len(idat) / z_default - 1.0,
            "tiles_stored_fixed_dynamic": [types.count(t) for t in (0, 1, 2)] if types else None,
            "best_row_filter_zlib_default_bytes": best_filter_bound(px) if small else None,
            "ppm_text_bytes": len(rt.ImageOutput.formatPpm(True, rgb))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", action="store_true")
    ap.add_argument("--frame", default=None)
    ap.add_argument("--pixels", type=int, default=800)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--spp", type=int, default=20)
    ap.add_argument("--bench-spp", type=int, default=500)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import ray_tracing_fsharp_amd as rt
    from ray_tracing_fsharp_amd import _abi as A
    from ray_tracing_fsharp_amd._lib import check

    lib = rt.lib
    ok = True
    if args.sizes:
        import png_cases as pc

        frames = list(pc.golden_frames())
        if args.frame:
            frames.append((os.path.basename(args.frame), np.ascontiguousarray(np.load(args.frame), np.uint8)))
        result = {"gamma": True, "tile_bytes": int(lib.rt_png_tile_bytes()), "measured_on": "host formatter (rt_format_png), no GPU",
                  "frames": [sizes_of(rt, n, f) for n, f in frames]}
        result["largest_excess_over_zlib_rle"] = max(f["excess_over_zlib_rle"] for f in result["frames"])
    else:
        import torch

        objs, cam, w, h = rt.sample_images.config3_final(seed=args.seed, spp=args.bench_spp, depth=50, pixels=args.pixels)
        rows, cols = 2 * h + 1, 2 * w + 1
        scene = rt.Scene.make(objs)
        scene.tune(w, h, cam, seed=args.seed ^ 0x5EED, device=0)
        low_abi, cam_abi = dataclasses.replace(cam, SamplesPerPixel=args.spp).to_abi(), cam.to_abi()
        stream = torch.cuda.current_stream().cuda_stream
        d_accum = torch.zeros((rows, cols, 4), dtype=torch.int32, device="cuda")
        d_rgb = torch.zeros((rows, cols, 3), dtype=torch.uint8, device="cuda")
        st = A.rt_stats()
        check(lib.rt_render_device(scene.handle, C.byref(low_abi), w, h, args.seed, 0, 0, 1, rows, 0, d_accum.data_ptr(), d_rgb.data_ptr(), stream, C.byref(st)))
        cap = int(lib.rt_png_max_bytes(rows, cols))
        host_file = np.empty(cap, np.uint8)
        d_file = torch.empty(cap, dtype=torch.uint8, device="cuda")
        d_len = torch.zeros((), dtype=torch.int64, device="cuda")
        u8p = C.POINTER(C.c_uint8)

        def host_route():
            t0 = time.perf_counter()
            rgb = d_rgb.cpu().numpy()
            t1 = time.perf_counter()
            n = lib.rt_format_png(rgb.ctypes.data_as(u8p), rows, cols, 1, host_file.ctypes.data, cap)
            t2 = time.perf_counter()
            return rgb, int(n), t1 - t0, t2 - t1

        def device_kernels(with_out=True):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            check(lib.rt_format_png_device(0, d_rgb.data_ptr(), rows, cols, 1, d_file.data_ptr() if with_out else None, cap if with_out else 0,
                                           d_len.data_ptr(), stream, None))
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e-3

        rgb, n_host, _, _ = host_route()
        device_kernels()
        n_dev = int(d_len)
        equal = n_host == n_dev and host_file[:n_host].tobytes() == d_file[:n_dev].cpu().numpy().tobytes()
        ok = bool(equal)
        result = {"frame": [cols, rows], "image_spp": args.spp, "gamma": True, "reps": args.reps, "outputs_equal": ok,
                  "tiles": -(-rows * (1 + 3 * cols) // int(lib.rt_png_tile_bytes()))}
        if not equal:
            result["error"] = "the two routes disagree; nothing timed"
        else:
            for _ in range(2):
                device_kernels(); device_kernels(False)
            a_copy, a_fmt, b_all, b_len = [], [], [], []
            for i in range(args.reps):
                if i < 3:  # (the host formatter takes a while: three runs)
                    _, _, tc, tf = host_route(); a_copy.append(tc); a_fmt.append(tf)
                b_all.append(device_kernels()); b_len.append(device_kernels(False))
            result["a_host_route"] = {"copy_rgb_ms": median_ms(a_copy), "rt_format_png_ms": median_ms(a_fmt)}
            result["b_device_kernels"] = {"four_launches_ms": median_ms(b_all), "all_runs_ms": sorted(1e3 * x for x in b_all),
                                          "sums_and_scan_ms": median_ms(b_len), "scatter_and_finish_ms": median_ms(b_all) - median_ms(b_len)}
            result["c_sizes"] = sizes_of(rt, "bench frame at %d spp" % args.spp, rgb)
            with tempfile.TemporaryDirectory() as d:
                p_png, p_ppm = os.path.join(d, "frame.png").encode(), os.path.join(d, "frame.ppm").encode()
                e_png, e_ppm, k_png, k_ppm = [], [], [], []
                for i in range(min(args.reps, 5) + 1):  # (the first round warms up)
                    t0 = time.perf_counter()
                    check(lib.rt_render_ppm(scene.handle, C.byref(cam_abi), w, h, args.seed, 0, 0, 1, p_ppm, None, C.byref(st)))
                    t1 = time.perf_counter()
                    kp = st.kernel_ms
                    check(lib.rt_render_png(scene.handle, C.byref(cam_abi), w, h, args.seed, 0, 0, 1, p_png, None, C.byref(st)))
                    t2 = time.perf_counter()
                    if i:
                        e_ppm.append(t1 - t0); e_png.append(t2 - t1); k_ppm.append(kp); k_png.append(st.kernel_ms)
                result["d_end_to_end"] = {"spp": args.bench_spp, "rt_render_ppm_ms": median_ms(e_ppm), "rt_render_png_ms": median_ms(e_png),
                                          "kernel_ms_ppm": float(np.median(k_ppm)), "kernel_ms_png": float(np.median(k_png)),
                                          "ppm_file_bytes": os.path.getsize(p_ppm), "png_file_bytes": os.path.getsize(p_png)}
    text = json.dumps(result, indent=1)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
