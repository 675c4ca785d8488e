"""What decoding a baseline JPEG costs by each route, on one GPU:

  host    rt_decode_jpeg on one host thread (sequential; the route without a GPU)
  device  rt_decode_jpeg_device from the file's bytes in host memory to the bitmap in device memory, waited for (stats given): the header
          parse, the upload of the entropy-coded bytes, every launch, the reads of the round counts

for tests/golden/earthmap.jpg (1024x512, 4:4:4) and -- where PIL is there to make them -- that map enlarged to 4096x2048 and 8192x4096 and
encoded at 4:2:0 and 4:4:4, quality 90.  The device route also runs through the hook at 64, 128, 256, 512 and 1024 bytes a subsequence,
with the rounds and the subsequence decodes of each.  Both routes' bitmaps are compared (and, with PIL, held to PIL's) before anything is
timed.  Warm-up first, medians of --reps, the routes alternating.  No threshold is set: the figures go to profiles/ and NOTES.md.  The
time per kernel (per stage: clean, rounds, place, DC, IDCT, colour) comes from runs of their own under `rocprofv3 --kernel-trace -- python
scripts/jpeg_measure.py --once FILE`, summed by scripts/jpeg_kernel_times.py: a profiler slows the host, so the two are kept apart.

usage: python scripts/jpeg_measure.py [--reps 7] [--out FILE] [--small]      (--small: the earth map alone)"""
import argparse
import ctypes as C
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (64, 128, 256, 512, 1024)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--once", default=None, help="decode this file once on the device at the default size and exit (for a profiler)")
    args = ap.parse_args()

    import torch

    import ray_tracing_fsharp_amd as rt
    from ray_tracing_fsharp_amd import _abi as A

    lib = rt.lib
    earth = open(os.path.join(ROOT, "tests", "golden", "earthmap.jpg"), "rb").read()
    if args.once:
        data = earth if args.once == "earth" else open(args.once, "rb").read()
        for _ in range(3):
            t = rt.LoadImage.fromBytes(data, device=0, tensor=True)
        torch.cuda.synchronize()
        print(tuple(t.shape), rt.hooks.last_jpeg_plan())
        return 0
    files = [("earthmap 1024x512 4:4:4", earth, np.load(os.path.join(ROOT, "tests", "golden", "earthmap_rgb.npz"))["rgb"])]
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None and not args.small:
        src = Image.fromarray(files[0][2])
        for w, h in ((4096, 2048), (8192, 4096)):
            big = src.resize((w, h), Image.BICUBIC)
            for name, sub in (("4:2:0", 2), ("4:4:4", 0)):
                b = io.BytesIO()
                big.save(b, "JPEG", quality=90, subsampling=sub)
                files.append((f"enlarged {w}x{h} {name}", b.getvalue(), np.asarray(Image.open(io.BytesIO(b.getvalue())).convert("RGB"))))
    result = {"reps": args.reps, "pil": Image is not None, "default_subsequence_bytes": None, "files": []}
    for name, data, want in files:
        shape = want.shape
        host_out = np.zeros(shape, np.uint8)
        d_out = torch.zeros(shape, dtype=torch.uint8, device="cuda:0")
        stats = A.rt_jpeg_stats()

        def host_route():
            t0 = time.perf_counter()
            rc = lib.rt_decode_jpeg(data, len(data), host_out.ctypes.data, host_out.size)
            return rc, time.perf_counter() - t0

        def device_route(S=None):
            t0 = time.perf_counter()
            if S is None:
                rc = lib.rt_decode_jpeg_device(0, data, len(data), d_out.data_ptr(), d_out.numel(), None, C.byref(stats))
            else:
                rc = lib.rt_dev_decode_jpeg(0, data, len(data), S, d_out.data_ptr(), d_out.numel())
            return rc, time.perf_counter() - t0

        rc_h, _ = host_route()
        rc_d, _ = device_route()
        equal = rc_h == 0 and rc_d == 0 and np.array_equal(host_out, want) and np.array_equal(d_out.cpu().numpy(), want)
        entry = {"file": name, "bytes": len(data), "info": rt.LoadImage.info(data), "results_equal_libjpeg": bool(equal)}
        result["files"].append(entry)
        if not equal:
            entry["error"] = f"host {rc_h}, device {rc_d}: the routes or PIL disagree; nothing timed"
            continue
        result["default_subsequence_bytes"] = int(stats.subsequence_bytes)
        for _ in range(2):  # warm-up
            host_route(); device_route()
        th, td, per = [], [], {S: [] for S in SIZES}
        plans = {}
        for _ in range(args.reps):  # alternating
            th.append(host_route()[1])
            td.append(device_route()[1])
            for S in SIZES:
                per[S].append(device_route(S)[1])
                plans[S] = rt.hooks.last_jpeg_plan()
        entry["host_ms"] = {"median": 1e3 * float(np.median(th)), "all": sorted(1e3 * x for x in th)}
        entry["device_ms"] = {"median": 1e3 * float(np.median(td)), "all": sorted(1e3 * x for x in td)}
        entry["host_over_device"] = float(np.median(th) / np.median(td))
        entry["by_subsequence_bytes"] = {str(S): {"median_ms": 1e3 * float(np.median(per[S])), "subsequences": plans[S]["subsequences"],
                                                  "rounds": plans[S]["rounds"], "decodes": plans[S]["decodes"]} for S in SIZES}
    text = json.dumps(result, indent=1)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if all(e["results_equal_libjpeg"] for e in result["files"]) else 1


if __name__ == "__main__":
    sys.exit(main())
