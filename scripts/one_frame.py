"""One launch of the render kernel on the bench workload (config 3), for rocprofv3 --pmc passes.
usage: python scripts/one_frame.py [--block B] [--chunk C] [--pixels P] [--spp S] [--launches L]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import ray_tracing_fsharp_amd as rt  # noqa: E402
from ray_tracing_fsharp_amd import distributed as rtd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--block", type=int, default=0)
ap.add_argument("--chunk", type=int, default=0)
ap.add_argument("--pixels", type=int, default=800)
ap.add_argument("--spp", type=int, default=500)
ap.add_argument("--depth", type=int, default=50)
ap.add_argument("--launches", type=int, default=1)
ap.add_argument("--counters", action="store_true")
ap.add_argument("--park", type=int, default=0, help="park pool entries per wave; -1 = never park")
ap.add_argument("--passes", type=int, default=0)
ap.add_argument("--yield-lanes", type=int, default=0)
ap.add_argument("--refill-lanes", type=int, default=0)
ap.add_argument("--no-tune", action="store_true", help="skip rt_scene_tune")
ap.add_argument("--grid", type=int, default=11, help="the scene's recipe over a larger grid (sample_images.randomSpheres): 16 -> 1026 spheres, 26 -> 2705")
ap.add_argument("--stage-stats", action="store_true", help="print rt_last_stage_stats of a timed launch too (a -DRTD_STAGE_CLOCKS build fills the cycle sums)")
ap.add_argument("--census-dump", metavar="FILE", help="a -DRTD_STAGE_CLOCKS build only: write the stage statistics and the census' execution counts "
                "(rt_diag_census) of the launches as JSON, the input of scripts/instruction_census.py table")
a = ap.parse_args()
rt.set_launch_config(a.block, a.chunk)
rt.set_park(a.park)
rt.set_passes(a.passes)
rt.set_schedule(a.yield_lanes, a.refill_lanes)
objs, cam, w, h = rt.sample_images.config3_final(spp=a.spp, depth=a.depth, pixels=a.pixels)
if a.grid != 11:
    import dataclasses
    objs, cam, w, h = rt.sample_images.randomSpheres(2024, a.spp, a.pixels, grid=a.grid)
    cam = dataclasses.replace(cam, BounceDepth=a.depth)
scene = rt.Scene.make(objs)
if not a.no_tune:
    scene.tune(w, h, cam, seed=2024)
rows, cols = 2 * h + 1, 2 * w + 1
local = torch.zeros((rows, cols, 4), dtype=torch.int32, device="cuda:0")
if a.census_dump:
    import ctypes
    cz = (ctypes.c_uint64 * 52)()
    if not hasattr(rt.lib, "rt_diag_census"):
        sys.exit("--census-dump needs a -DRTD_STAGE_CLOCKS build (RTFS_LIB): this library has no rt_diag_census")
    rt.lib.rt_diag_census.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int32, ctypes.c_int32]
    rt.lib.rt_diag_census(cz, 52, 1)  # the tuning probe's launches are not the frame's
for _ in range(a.launches):
    st = rtd.render_shard_device(scene, cam, w, h, 2024, 0, 0, 1, rows, local, counters=a.counters, want_stats=True)
    print({k: st[k] for k in ("kernel_ms", "rays", "aabb_tests", "prim_tests", "samples")}, flush=True)
    if a.counters or a.stage_stats or a.census_dump:
        import ctypes
        ss = (ctypes.c_uint64 * 16)()
        rt.lib.rt_last_stage_stats(ss)
        names = ("refill_stages", "node_trips", "leaf_stages", "shade_stages", "lanes_refilled", "lanes_shaded", "wave_ticks", "span_ticks", "waves", "slow_stages", "slow_lanes", "parked_lanes", "cyc_refill", "cyc_slow", "cyc_walk", "cyc_shade")
        print(dict(zip(names, list(ss))), flush=True)
        if a.census_dump:
            import json
            if rt.lib.rt_diag_census(cz, 52, 0) != 0:
                sys.exit("rt_diag_census failed")
            cn = ("turns", "lamb_batches", "lamb_lanes", "new_refills", "new_items", "unpark_lambert", "unpark_general", "store_blocks_lambert", "store_lanes_lambert",
                  "store_blocks_general", "light_batches", "light_lanes", "miss_lanes", "ranges", "flushes", "leaf_lanes")
            d = {"launches": a.launches, "kernel_ms": st["kernel_ms"], "stage_stats": dict(zip(names, list(ss))), "census": dict(zip(cn, list(cz)[:16]))}
            d["census"]["slow_lanes_by_style"] = list(cz)[16:24]
            d["census"]["slow_batches_by_style"] = list(cz)[24:32]
            d["census"].update(zip(("random_unit_retries", "lambert_bounce_retries", "sliver_lanes", "sliver_blocks"), list(cz)[32:36]))
            d["census"].update(zip(("refill_stages", "walk_entries", "leaf_passes", "shade_stages", "refill_lanes", "shade_lanes", "slow_stages", "slow_lanes", "loop_trips", "loop_lanes",
                                    "unpark_lambert_batches", "unpark_general_batches"), list(cz)[36:48]))
            # lanes that took an arm behind a wave-uniform guard (rt_device.h, RTD_ANY_LANE); every launch since the reset, not pass B alone
            d["census"].update(zip(("equal_arm_lanes_unbounded", "equal_arm_lanes_leaf"), list(cz)[48:50]))
            d["census"]["guarded_arms"] = sum(list(cz)[48:50])
            json.dump(d, open(a.census_dump, "w"), indent=1)
