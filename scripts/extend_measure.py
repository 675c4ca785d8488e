"""What extending a frame costs (NOTES.md "Extending a frame"): the bench frame (config 3, tuned tree) rendered directly at the target,
and as render(a) + extend(a -> target) for each a of --from, alternating, `kernel_ms` from HIP events around each launch.  Every
extended frame must equal the direct one word for word.  With --tail one more launch of each through the counting variant gives
the span from the mean wave's end to the last wave's (rt_last_stage_stats): the unordered list's tail against the ordered one's.
One JSON line per figure on stdout."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import ray_tracing_fsharp_amd as rt  # noqa: E402
from ray_tracing_fsharp_amd import distributed as dist  # noqa: E402


def stage_tail_ms():
    ss = (C.c_uint64 * 16)()
    rt.lib.rt_last_stage_stats(ss)
    lifetimes, span, waves = ss[6], ss[7], ss[8]  # 100 MHz ticks
    return {"span_ms": span / 1e5, "mean_wave_ms": lifetimes / max(1, waves) / 1e5, "tail_ms": (span - lifetimes / max(1, waves)) / 1e5, "waves": waves}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=500)
    ap.add_argument("--from", dest="starts", type=int, nargs="+", default=[100, 12])
    ap.add_argument("--pixels", type=int, default=800)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--tail", action="store_true")
    a = ap.parse_args()
    if rt.device_count() < 1:
        raise SystemExit("needs a GPU")
    import dataclasses
    objs, cam, w, h = rt.sample_images.config3_final(seed=a.seed, spp=a.spp, depth=50, pixels=a.pixels)
    rows, cols = 2 * h + 1, 2 * w + 1
    scene = rt.Scene.make(objs)
    scene.tune(w, h, cam, seed=1, device=0)
    at = lambda spp: dataclasses.replace(cam, SamplesPerPixel=spp)  # noqa: E731
    buf = lambda: torch.zeros((rows, cols, 4), dtype=torch.int32, device="cuda:0")  # noqa: E731

    def render(spp, counters=False):
        t = buf()
        st = dist.render_shard_device(scene, at(spp), w, h, 1, 0, 0, 1, rows, t, counters=counters, want_stats=True)
        return t, st

    direct, _ = render(a.spp)  # warm-up of every kernel the timed window uses, and the frame to compare with
    for s in a.starts:
        t, _ = render(s)
        scene.extend_rows(w, h, at(a.spp), t, s, seed=1)
    for rep in range(a.reps):
        t, st = render(a.spp)
        print(json.dumps({"what": "render", "spp": a.spp, "rep": rep, "kernel_ms": st["kernel_ms"], "samples": st["samples"]}), flush=True)
        for s in a.starts:
            t, st0 = render(s)
            res = scene.extend_rows(w, h, at(a.spp), t, s, seed=1)
            print(json.dumps({"what": "render+extend", "from": s, "to": a.spp, "rep": rep, "render_ms": st0["kernel_ms"], "extend_ms": res.stats["kernel_ms"],
                              "sum_ms": st0["kernel_ms"] + res.stats["kernel_ms"], "samples_added": res.stats["samples"],
                              "pixels_final": res.stats["pixels_early"], "equal_to_direct": bool(torch.equal(res.accum, direct))}), flush=True)
    if a.tail:
        _, st = render(a.spp, counters=True)
        print(json.dumps(dict({"what": "tail, direct render (counting variant: pass A, ordering, pass B)", "kernel_ms": st["kernel_ms"]}, **stage_tail_ms())), flush=True)
        for s in a.starts:
            t, _ = render(s)
            res = scene.extend_rows(w, h, at(a.spp), t, s, seed=1, counters=True)
            print(json.dumps(dict({"what": "tail, extend (counting variant: pass B over the unordered list)", "from": s, "kernel_ms": res.stats["kernel_ms"]},
                                  **stage_tail_ms())), flush=True)


if __name__ == "__main__":
    main()
