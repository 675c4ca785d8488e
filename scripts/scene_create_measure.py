"""What creating a scene costs on each route, wall time, for n = 485 (the final scene's bounded spheres), 1e4, 1e5 and 1e6 spheres of a
final-scene-like input (scripts/tree_measure.py's "tied" spheres), walk tree "sah":

  ex            rt_scene_create_ex: everything on the host
  gpu_trees     rt_scene_create_gpu_trees of this build: both trees on the device, the rest on the host
  ex_parent, gpu_trees_parent
                the same two routes of another build of the library (--parent-lib: the parent commit's librtfs_amd.so), loaded into the same
                process, each alternating with this build's route: pair k is one parent run, then one run of this build.  These two routes
                run the host's build_scene / encode_image, which this build states through csrc/rt_scene_plan.h: the pairs say whether
                that costs anything
  parent        the parent's rt_scene_create_gpu_trees again, its runs alternating with `device`
  device        rt_scene_create_device from a tensor that is already resident: nothing of the scene passes through the host
  stages        of `device`: the reference tree alone (rt_tree_make_device) and the walk tree alone (rt_walk_tree_make_device) over the same
                boxes, already on the device; `rest` is the median of device less the two -- check, partition, ranks, encode, allocations
  crossover     ex against device over a ladder of sizes: the first size from which device stays faster (reported, not required)

Before anything is timed the device-made scene is compared with gpu_trees' (rt_scene_get_info and the image).  Every run is kept.  Required
of the figures (and asserted here): at 1e5 and 1e6 `device` is faster than `parent` in every alternating pair.

usage: python scripts/scene_create_measure.py [--sizes 485,10000,100000,1000000] [--reps 5] [--parent-lib FILE] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tree_measure import boxes_of, hittables, spheres  # noqa: E402

LADDER = [485, 1024, 2048, 4096, 8192, 16384, 32768, 65536]


def timed(fn, reps, after=None):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append(round(1e3 * (time.perf_counter() - t0), 4))
        if after:
            after(r)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="485,10000,100000,1000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25", "scene_create_measure.json"))
    args = ap.parse_args()
    import torch

    import ray_tracing_fsharp_amd as rt
    A = rt._abi
    lib = rt.lib
    parent = None
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        assert parent.rt_abi_version() == A.RT_ABI_VERSION
        parent.rt_scene_destroy.argtypes = [C.c_void_p]
        parent.rt_scene_create_gpu_trees.argtypes = lib.rt_scene_create_gpu_trees.argtypes
        parent.rt_scene_create_ex.argtypes = lib.rt_scene_create_ex.argtypes
    opt = A.rt_scene_options(A.RT_WALK_TREE_SAH)
    where = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(where).cuda_stream
    res = {"device_name": torch.cuda.get_device_name(0), "unit": "ms, wall time, every run", "sizes": {}, "crossover": {}}

    def routes(n):
        sp = spheres("tied", n)
        hs = hittables(A, sp)
        t = torch.from_numpy(np.frombuffer(hs, np.uint8).reshape(n, -1).copy()).to(where)
        boxes = torch.from_numpy(boxes_of(sp)).to(where)
        torch.cuda.synchronize()
        destroy = lambda h: lib.rt_scene_destroy(h)  # noqa: E731

        def ex(which=lib):
            out = C.c_void_p()
            assert which.rt_scene_create_ex(hs, n, None, 0, C.byref(opt), C.byref(out)) == 0
            return out

        def trees(which=lib):
            out = C.c_void_p()
            assert which.rt_scene_create_gpu_trees(hs, n, None, 0, C.byref(opt), 0, C.byref(out)) == 0
            return out

        def device():
            out = C.c_void_p()
            assert lib.rt_scene_create_device(0, t.data_ptr(), n, None, 0, C.byref(opt), stream, C.byref(out)) == 0, lib.rt_last_error()
            return out
        return hs, t, boxes, destroy, ex, trees, device

    for n in (int(s) for s in args.sizes.split(",")):
        hs, t, boxes, destroy, ex, trees, device = routes(n)
        reps = args.reps if n < 1000000 else min(args.reps, 3)
        # the same scene first
        a, b = rt.Scene(trees().value, []), rt.Scene(device().value, [])
        assert a.info() == b.info() and np.array_equal(rt.hooks.scene_image(a)[0], rt.hooks.scene_image(b)[0]), n
        del a, b
        row = {}
        timed(device, 1, destroy)  # warm
        if parent is None:
            row["ex"] = timed(ex, 1 if n >= 1000000 else reps, destroy)
            row["gpu_trees"] = timed(trees, reps, destroy)
            row["device"] = timed(device, reps, destroy)
        else:
            pdestroy = lambda h: parent.rt_scene_destroy(h)  # noqa: E731
            timed(lambda: trees(parent), 1, pdestroy)
            for key, route, k in (("ex", ex, 1 if n >= 1000000 else reps), ("gpu_trees", trees, reps)):
                row[key + "_parent"], row[key] = [], []
                for _ in range(k):  # alternating pairs
                    row[key + "_parent"] += timed(lambda: route(parent), 1, pdestroy)
                    row[key] += timed(route, 1, destroy)
            row["parent"], row["device"] = [], []
            for _ in range(reps):  # alternating pairs
                row["parent"] += timed(lambda: trees(parent), 1, pdestroy)
                row["device"] += timed(device, 1, destroy)
            row["device_faster_in_every_pair"] = all(d < p for d, p in zip(row["device"], row["parent"]))
        nn = int(lib.rt_tree_nodes(n))
        skip, prim = torch.empty(nn, dtype=torch.int32, device=where), torch.empty(nn, dtype=torch.int32, device=where)
        nb, order = torch.empty((nn, 6), dtype=torch.float64, device=where), torch.empty(n, dtype=torch.int32, device=where)
        tree = lambda: lib.rt_tree_make_device(0, n, boxes.data_ptr(), skip.data_ptr(), prim.data_ptr(), nb.data_ptr(), order.data_ptr(), stream)  # noqa: E731
        walk = lambda: lib.rt_walk_tree_make_device(0, n, boxes.data_ptr(), skip.data_ptr(), prim.data_ptr(), nb.data_ptr(), stream)  # noqa: E731
        tree(), walk()
        row["stage_tree"], row["stage_walk_tree"] = timed(tree, reps), timed(walk, reps)
        med = lambda v: float(np.median(v))  # noqa: E731
        row["stage_rest_median"] = round(med(row["device"]) - med(row["stage_tree"]) - med(row["stage_walk_tree"]), 4)
        row["share_of_device_median"] = {k: round(med(row[v]) / med(row["device"]), 3) for k, v in (("tree", "stage_tree"), ("walk_tree", "stage_walk_tree"))}
        res["sizes"][str(n)] = row
        print(n, {k: (round(med(v), 3) if isinstance(v, list) else v) for k, v in row.items()}, flush=True)
    first = None
    for n in LADDER:
        hs, t, boxes, destroy, ex, trees, device = routes(n)
        timed(device, 1, destroy)
        e, d = float(np.median(timed(ex, 3, destroy))), float(np.median(timed(device, 3, destroy)))
        res["crossover"][str(n)] = {"ex": round(e, 4), "device": round(d, 4)}
        first = (first if first is not None else n) if d < e else None
    res["crossover"]["device_stays_faster_from"] = first
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("crossover", res["crossover"], flush=True)
    if parent is not None:
        for n in ("100000", "1000000"):
            if n in res["sizes"]:
                assert res["sizes"][n]["device_faster_in_every_pair"], (n, res["sizes"][n]["parent"], res["sizes"][n]["device"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
