"""What encoding a batch of views in one call gains over one encode per view (rt_format_png_views_device against rt_format_png_device), on one GPU.

The batch is README.md's: K = 64 views (config 2, the three Lambert spheres, its camera turned round the y axis in K steps) of a 71x41
frame rendered at 100 spp, depth 50, gamma on.  The bytes of both routes are compared with the host formatter's before anything is timed.
  (a) batch encode     ONE rt_format_png_views_device call between two events on the stream (four launches)
  (b) single encodes   K rt_format_png_device calls back to back on the slices, between the same two events (4 K launches); this is code
                       the parent already has, measured in the same process as (a), the legs alternating after a warm-up
  (c) file routes      wall clock, files included: rt_render_views_png against rt_render_views_device followed by K rt_write_png_device calls
  (d) one large image  the bench frame (config 3, 2401x1601, rendered at a reduced sample count) with K = 1 against rt_format_png_device:
                       what the generality costs a single large image
Events cannot be placed between the launches from outside the library: the per-kernel times come from a kernel trace of this script
(rocprofv3 --kernel-trace --stats -- python scripts/png_views_measure.py), a run of its own with no counters collected in it.  No
threshold is set: the figures go to profiles/ and NOTES.md.

usage: python scripts/png_views_measure.py [--views 64] [--reps 15] [--file-reps 7] [--bench-pixels 800] [--bench-image-spp 20] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from views_measure import stats_of, turntable  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--pixels", type=int, default=20, help="maxHeightCoord of the small frames: 20 is 71x41")
    ap.add_argument("--spp", type=int, default=100)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--file-reps", type=int, default=7)
    ap.add_argument("--bench-pixels", type=int, default=800)
    ap.add_argument("--bench-image-spp", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import ray_tracing_fsharp_amd as rt
    from ray_tracing_fsharp_amd._lib import check

    A, L = rt._abi, rt.lib
    if rt.device_count() < 1:
        raise SystemExit("png_views_measure.py needs a GPU")
    stream = torch.cuda.current_stream().cuda_stream

    def between_events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    # ---- the batch ----
    objs, cam, w, h = rt.sample_images.config2_three_lambert(spp=args.spp, depth=args.depth, pixels=args.pixels)
    rows, cols = 2 * h + 1, 2 * w + 1
    k = args.views
    cams = turntable(rt, cam, k)
    seeds = [args.seed + i for i in range(k)]
    scene = rt.Scene.make(objs)
    abi = (A.rt_camera * k)(*[c.to_abi() for c in cams])
    keys = (C.c_uint64 * k)(*seeds)
    d_accum = torch.zeros((k, rows, cols, 4), dtype=torch.int32, device="cuda")
    d_rgb = torch.zeros((k, rows, cols, 3), dtype=torch.uint8, device="cuda")

    def render():
        check(L.rt_render_views_device(scene.handle, abi, k, w, h, keys, 0, 0, 0, d_accum.data_ptr(), d_rgb.data_ptr(), stream, None, None))

    render()
    torch.cuda.synchronize()
    image_bytes = rows * cols * 3
    cap1, cap = int(L.rt_png_max_bytes(rows, cols)), int(L.rt_png_views_max_bytes(k, rows, cols))
    d_files = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_offsets = torch.zeros(k + 1, dtype=torch.int64, device="cuda")
    d_singles = torch.zeros((k, cap1), dtype=torch.uint8, device="cuda")
    d_lengths = torch.zeros(k, dtype=torch.int64, device="cuda")

    def batch_encode():
        check(L.rt_format_png_views_device(0, d_rgb.data_ptr(), k, rows, cols, 1, d_files.data_ptr(), cap, d_offsets.data_ptr(), stream, None))

    def single_encodes():
        for v in range(k):
            check(L.rt_format_png_device(0, d_rgb.data_ptr() + v * image_bytes, rows, cols, 1, d_singles.data_ptr() + v * cap1, cap1,
                                         d_lengths.data_ptr() + 8 * v, stream, None))

    batch_encode(); single_encodes()
    torch.cuda.synchronize()
    host = [rt.Png.format(True, image) for image in d_rgb.cpu().numpy()]
    at = d_offsets.cpu().tolist()
    files = d_files[: at[-1]].cpu().numpy().tobytes()
    singles, lengths = d_singles.cpu().numpy(), d_lengths.cpu().tolist()
    equal = [files[a:b] for a, b in zip(at[:-1], at[1:])] == host == [singles[v, : lengths[v]].tobytes() for v in range(k)]
    out = {"views": k, "frame": [cols, rows], "spp": args.spp, "gamma": True, "reps": args.reps, "outputs_equal": bool(equal),
           "tiles_per_image": -(-rows * (1 + 3 * cols) // int(L.rt_png_tile_bytes())), "files_bytes": at[-1], "rgb_bytes": k * image_bytes}
    if not equal:
        out["error"] = "the routes disagree; nothing timed"
    else:
        for _ in range(3):  # warm-up of both legs
            between_events(batch_encode); between_events(single_encodes)
        ms = {"batch": [], "singles": []}
        for _ in range(args.reps):
            ms["batch"].append(between_events(batch_encode))
            ms["singles"].append(between_events(single_encodes))
        out["a_batch_encode_ms"] = stats_of(ms["batch"])
        out["b_single_encodes_ms"] = stats_of(ms["singles"])
        out["b_over_a"] = round(out["b_single_encodes_ms"]["median"] / out["a_batch_encode_ms"]["median"], 2)

        # ---- (c) the file routes, wall clock ----
        with tempfile.TemporaryDirectory() as d:
            names = [os.path.join(d, f"view{v}.png").encode() for v in range(k)]
            paths = (C.c_char_p * k)(*names)
            st = A.rt_stats()

            def batch_files():
                check(L.rt_render_views_png(scene.handle, abi, k, w, h, keys, 0, 0, 0, 1, paths, None, C.byref(st)))

            def single_files():
                render()
                for v in range(k):
                    check(L.rt_write_png_device(names[v], 0, d_rgb.data_ptr() + v * image_bytes, rows, cols, 1, stream))

            def wall(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            wall(batch_files)
            same = [open(n, "rb").read() for n in names] == host
            wall(single_files)
            same = same and [open(n, "rb").read() for n in names] == host
            out["c_files_equal"] = bool(same)
            fm = {"batch": [], "singles": []}
            for _ in range(args.file_reps):
                fm["batch"].append(wall(batch_files))
                fm["singles"].append(wall(single_files))
            out["c_render_views_png_ms"] = stats_of(fm["batch"])
            out["c_render_then_k_write_png_device_ms"] = stats_of(fm["singles"])
            out["c_render_kernel_ms_in_batch_call"] = round(float(st.kernel_ms), 3)

        # ---- (d) one large image ----
        objs3, cam3, w3, h3 = rt.sample_images.config3_final(seed=args.seed, spp=args.bench_image_spp, depth=50, pixels=args.bench_pixels)
        rows3, cols3 = 2 * h3 + 1, 2 * w3 + 1
        scene3 = rt.Scene.make(objs3)
        big_accum = torch.zeros((rows3, cols3, 4), dtype=torch.int32, device="cuda")
        big = torch.zeros((rows3, cols3, 3), dtype=torch.uint8, device="cuda")
        check(L.rt_render_device(scene3.handle, C.byref(cam3.to_abi()), w3, h3, args.seed, 0, 0, 1, rows3, 0, big_accum.data_ptr(), big.data_ptr(), stream, None))
        cap3 = int(L.rt_png_max_bytes(rows3, cols3))
        f_views, f_one = torch.zeros(cap3, dtype=torch.uint8, device="cuda"), torch.zeros(cap3, dtype=torch.uint8, device="cuda")
        o_views, o_one = torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros((), dtype=torch.int64, device="cuda")

        def big_views():
            check(L.rt_format_png_views_device(0, big.data_ptr(), 1, rows3, cols3, 1, f_views.data_ptr(), cap3, o_views.data_ptr(), stream, None))

        def big_one():
            check(L.rt_format_png_device(0, big.data_ptr(), rows3, cols3, 1, f_one.data_ptr(), cap3, o_one.data_ptr(), stream, None))

        big_views(); big_one()
        torch.cuda.synchronize()
        n3 = int(o_one)
        out["d_frame"] = [cols3, rows3]
        out["d_outputs_equal"] = bool(o_views.cpu().tolist() == [0, n3] and torch.equal(f_views[:n3], f_one[:n3]))
        for _ in range(2):
            between_events(big_views); between_events(big_one)
        bm = {"views": [], "one": []}
        for _ in range(args.reps):
            bm["views"].append(between_events(big_views))
            bm["one"].append(between_events(big_one))
        out["d_views_k1_ms"] = stats_of(bm["views"])
        out["d_format_png_device_ms"] = stats_of(bm["one"])
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if out.get("outputs_equal") and out.get("c_files_equal") and out.get("d_outputs_equal") else 1


if __name__ == "__main__":
    sys.exit(main())
