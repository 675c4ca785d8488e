"""What extending by map costs (NOTES.md "Extending by map"): on the bench frame (config 3, tuned tree) rendered at --base samples,
alternating, `kernel_ms` from HIP events around each launch:
  extend   rt_render_extend base -> --spp (pass B's uniform kernel: the baseline, with the spread of its repeats),
  uniform  rt_render_extend_map with every target --spp (the same samples through the per-pixel variant),
  sparse   rt_render_extend_map with every --every-th pixel to --spp and the others left.
The uniform map must equal the extension word for word, and the sparse map must equal it on the pixels it continues and the base
on the others.  One JSON line per figure on stdout, then a summary line with the time per added sample."""
import argparse
import dataclasses
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import ray_tracing_fsharp_amd as rt  # noqa: E402
from ray_tracing_fsharp_amd import distributed as dist  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=500)
    ap.add_argument("--base", type=int, default=12)
    ap.add_argument("--every", type=int, default=4)
    ap.add_argument("--pixels", type=int, default=800)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--chunk", type=int, default=0, help="pixels per range of pass B for all three (0: the plan's; a small one keeps the Lambert pool in LDS "
                    "at its full size under the map's larger scratch too, which separates that effect from the lookup's)")
    a = ap.parse_args()
    if rt.device_count() < 1:
        raise SystemExit("needs a GPU")
    objs, cam, w, h = rt.sample_images.config3_final(seed=a.seed, spp=a.spp, depth=50, pixels=a.pixels)
    rows, cols = 2 * h + 1, 2 * w + 1
    scene = rt.Scene.make(objs)
    scene.tune(w, h, cam, seed=1, device=0)
    at = lambda spp: dataclasses.replace(cam, SamplesPerPixel=spp)  # noqa: E731

    base = torch.zeros((rows, cols, 4), dtype=torch.int32, device="cuda:0")
    dist.render_shard_device(scene, at(a.base), w, h, 1, 0, 0, 1, rows, base, want_stats=True)
    uniform = torch.full((rows, cols), a.spp, dtype=torch.int32, device="cuda:0")
    sparse = torch.zeros((rows, cols), dtype=torch.int32, device="cuda:0")
    sparse.view(-1)[::a.every] = a.spp
    picked = (sparse > 0)

    def plan():
        o = rt.hooks.last_launch_plan()["out"]
        return {"B_mode": o["B_mode"], "B_chunk": o["B_chunk"], "B_lds_bytes": o["B_lds_bytes"], "B_grid": o["B_grid"], "B_park_l": o["B_park_l"],
                "B_park_l_lds": o["B_park_l_lds"]}

    opt = rt._abi.rt_render_options(chunk_pixels=a.chunk) if a.chunk else None

    def run(what):
        t = base.clone()
        if what == "extend":
            return scene.extend_rows(w, h, at(a.spp), t, a.base, seed=1, options=opt)
        return scene.extend_rows_map(w, h, at(a.spp), t, uniform if what == "uniform" else sparse, seed=1, options=opt)

    full = run("extend").accum.clone()  # warm-up of every kernel the timed window uses, and the frames to compare with
    run("uniform"); run("sparse")
    ms = {"extend": [], "uniform": [], "sparse": []}
    added = {}
    for rep in range(a.reps):
        for what in ("extend", "uniform", "sparse"):
            res = run(what)
            if what == "sparse":
                ok = bool(torch.equal(res.accum[picked], full[picked]) and torch.equal(res.accum[~picked], base[~picked]))
            else:
                ok = bool(torch.equal(res.accum, full))
            ms[what].append(res.stats["kernel_ms"])
            added[what] = res.stats["samples"]
            print(json.dumps(dict({"what": what, "rep": rep, "kernel_ms": res.stats["kernel_ms"], "samples_added": res.stats["samples"],
                                   "pixels_final": res.stats["pixels_early"], "equal": ok}, **plan())), flush=True)
            if not ok:
                raise SystemExit(f"{what}: the result differs")
    out = {"what": "summary", "base": a.base, "spp": a.spp, "every": a.every, "chunk": a.chunk, "pixels": rows * cols}
    for what, v in ms.items():
        out[what] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "samples_added": added[what],
                     "ns_per_sample": statistics.median(v) * 1e6 / max(1, added[what])}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
