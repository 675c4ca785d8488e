"""What a pixel list costs next to the frame it is taken from (rt_render_pixels_device against rt_render_device), on one GPU.

The bench frame (config 3, 2401x1601 at 500 spp, tuned tree) four ways, alternating after a warm-up, kernel_ms of each repetition:
  (a) frame       rt_render_device of the whole frame
  (b) row-major   the whole frame as a list, indices 0 .. rows*cols-1
  (c) tiled       the same pixels ordered in 8x8 tiles
  (d) crop        a centred crop holding a quarter of the pixels (half the rows x half the columns), row-major
and, from one extra launch of each with the counting variant, the samples traced -- (d)'s share of the frame's samples is what its
time is to be compared with.  (b), (c) and (d) are checked against (a)'s pixels before anything is timed.

usage: python scripts/pixel_list_measure.py [--pixels 800] [--spp 500] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def tiled(rows, cols, tile=8):
    r, c = np.divmod(np.arange(rows * cols, dtype=np.int64), cols)
    key = ((r // tile) * ((cols + tile - 1) // tile) + c // tile) * (tile * tile) + (r % tile) * tile + c % tile
    return np.argsort(key, kind="stable").astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pixels", type=int, default=800)
    ap.add_argument("--spp", type=int, default=500)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import ray_tracing_fsharp_amd as rt
    from ray_tracing_fsharp_amd import distributed as rtd

    objs, cam, w, h = rt.sample_images.config3_final(seed=args.seed, spp=args.spp, depth=args.depth, pixels=args.pixels)
    rows, cols = 2 * h + 1, 2 * w + 1
    n = rows * cols
    scene = rt.Scene.make(objs)
    scene.tune(w, h, cam, seed=args.seed ^ 0x5EED, device=0)
    r0, c0 = rows // 4, cols // 4
    crop = (np.arange(r0, r0 + rows // 2, dtype=np.int64)[:, None] * cols + np.arange(c0, c0 + cols // 2, dtype=np.int64)[None, :]).reshape(-1).astype(np.int32)
    lists = {"row-major": np.arange(n, dtype=np.int32), "tiled": tiled(rows, cols), "crop": crop}
    d_lists = {k: torch.from_numpy(v).cuda() for k, v in lists.items()}
    frame = torch.zeros((rows, cols, 4), dtype=torch.int32, device="cuda")

    def leg(name, counters=False):
        if name == "frame":
            return rtd.render_shard_device(scene, cam, w, h, args.seed, 0, 0, 1, rows, frame, counters=counters, want_stats=True), None
        res = scene.renderPixels(w, h, cam, d_lists[name], seed=args.seed, counters=counters)
        return res.stats, res.accum

    legs = ("frame", "row-major", "tiled", "crop")
    # warm-up, and the check: every list entry is that pixel of the frame
    leg("frame")
    flat = frame.reshape(-1, 4)
    for name in legs[1:]:
        _, acc = leg(name)
        if not torch.equal(acc, flat[d_lists[name].long()]):
            raise SystemExit(f"{name}: the list's pixels differ from the frame's")
    out = {"frame": [cols, rows], "spp": args.spp, "pixels": {k: int(len(v)) for k, v in lists.items()}, "kernel_ms": {k: [] for k in legs}, "plan": {}}
    out["pixels"]["frame"] = n
    for _ in range(args.reps):
        for name in legs:
            st, _ = leg(name)
            out["kernel_ms"][name].append(round(st["kernel_ms"], 3))
            p = rt.hooks.last_launch_plan()
            out["plan"][name] = {"kind": p["in"]["kind"], "two_pass": p["out"]["two_pass"], "q_mode": p["out"]["q_mode"]}
    out["samples"] = {name: leg(name, counters=True)[0]["samples"] for name in legs}
    out["rays"] = {name: leg(name, counters=True)[0]["rays"] for name in legs}
    out["mean_ms"] = {k: round(float(np.mean(v)), 3) for k, v in out["kernel_ms"].items()}
    out["spread_ms"] = {k: round(float(np.max(v) - np.min(v)), 3) for k, v in out["kernel_ms"].items()}
    out["crop_share_of_samples"] = round(out["samples"]["crop"] / out["samples"]["frame"], 4)
    out["crop_share_of_time"] = round(out["mean_ms"]["crop"] / out["mean_ms"]["frame"], 4)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
