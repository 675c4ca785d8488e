"""What the surface-area walk tree costs on the host and on one GPU, and what creating a scene costs with both trees from the device -- for
n = 485 (the final scene's bounded spheres), 1e4, 1e5 and 1e6 boxes of a final-scene-like input (scripts/tree_measure.py's "tied" spheres):

  host        rt_walk_tree_make_host, wall time (SahBuilder without probe rays: one thread)
  device      rt_walk_tree_make_device, wall time, boxes and outputs already on the device (the call waits for the stream once per level of
              nodes above 4096 boxes, so wall time is the honest figure): warmed, repeated, all runs kept
  create      wall time of rt_scene_create_ex, rt_scene_create_gpu_tree and rt_scene_create_gpu_trees, walk tree "sah"
  parent      rt_scene_create_gpu_tree of another build of the library (--parent-lib: the parent commit's librtfs_amd.so), in a fresh process
  crossover   host and device build over a ladder of sizes; the first size from which the device build stays faster

The host and the device leg alternate.  The device's tree is compared with the host's before anything is timed.  No threshold is set: the
figures go to profiles/ and DESIGN.md.

usage: python scripts/walk_tree_measure.py [--sizes 485,10000,100000,1000000] [--reps 5] [--parent-lib FILE] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tree_measure import boxes_of, hittables, spheres  # noqa: E402

LADDER = [64, 256, 1024, 2048, 4096, 4097, 8192, 16384, 32768, 65536]


def create_ms(fn, A, hs, n, device, reps, destroy):
    out, ts = C.c_void_p(), []
    opt = A.rt_scene_options(A.RT_WALK_TREE_SAH)
    for _ in range(reps):
        t0 = time.perf_counter()
        rc = fn(hs, n, None, 0, C.byref(opt), C.byref(out)) if device is None else fn(hs, n, None, 0, C.byref(opt), device, C.byref(out))
        ts.append(1e3 * (time.perf_counter() - t0))
        assert rc == 0, rc
        destroy(out)
    return sorted(ts)


def parent_leg(args):
    """In a fresh process: the other library alone, through the structs of this checkout (the ABI version is the same)."""
    import ray_tracing_fsharp_amd._abi as A  # noqa: F401  (loads this checkout's library too; only the other one is called)
    lib = C.CDLL(os.path.abspath(args.parent_lib))
    assert lib.rt_abi_version() == A.RT_ABI_VERSION
    lib.rt_scene_destroy.argtypes = [C.c_void_p]
    res = {}
    for n in args.sizes:
        hs = hittables(A, spheres("tied", n))
        reps = args.reps if n < 1000000 else min(args.reps, 3)
        create_ms(lib.rt_scene_create_gpu_tree, A, hs, C.c_size_t(n), 0, 1, lib.rt_scene_destroy)  # warm
        res[str(n)] = create_ms(lib.rt_scene_create_gpu_tree, A, hs, C.c_size_t(n), 0, reps, lib.rt_scene_destroy)
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=[485, 10000, 100000, 1000000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-leg", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.parent_leg:
        return parent_leg(args)

    import torch

    import ray_tracing_fsharp_amd as rt
    from ray_tracing_fsharp_amd._lib import check
    A, lib = rt._abi, rt.lib
    result = {"cpus": len(os.sched_getaffinity(0)), "reps": args.reps, "cases": {}, "ladder": {}}
    ok = True
    i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)

    def legs(n, reps):
        b = boxes_of(spheres("tied", n))
        host = rt.walk_tree_make_host(b)
        d = torch.from_numpy(b).cuda()
        dev = [t.cpu().numpy() for t in rt.walk_tree_make(d)]
        equal = np.array_equal(host[0], dev[0]) and np.array_equal(host[1], dev[1]) and bool((host[2] == dev[2]).all())
        if not equal:
            return None
        nn = 2 * n - 1
        outs = [torch.empty(nn, dtype=torch.int32, device="cuda"), torch.empty(nn, dtype=torch.int32, device="cuda"), torch.empty((nn, 6), dtype=torch.float64, device="cuda")]
        h_outs = [np.zeros(nn, np.int32), np.zeros(nn, np.int32), np.zeros((nn, 6))]
        stream = torch.cuda.current_stream().cuda_stream
        hs_, ds_ = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            check(lib.rt_walk_tree_make_host(n, b.ctypes.data_as(f64), h_outs[0].ctypes.data_as(i32), h_outs[1].ctypes.data_as(i32), h_outs[2].ctypes.data_as(f64)))
            hs_.append(1e3 * (time.perf_counter() - t0))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            check(lib.rt_walk_tree_make_device(0, n, d.data_ptr(), *[o.data_ptr() for o in outs], stream))
            ds_.append(1e3 * (time.perf_counter() - t0))
        return sorted(hs_), sorted(ds_)

    for n in args.sizes:
        reps = args.reps if n < 1000000 else min(args.reps, 3)
        got = legs(n, reps)
        case = {"n": n, "results_equal": got is not None}
        result["cases"][str(n)] = case
        if got is None:
            ok = False
            case["error"] = "the device build differs from the host builder; nothing timed"
            continue
        case["host_build_ms"], case["device_build_ms"] = got
        hs = hittables(A, spheres("tied", n))
        create_ms(lib.rt_scene_create_gpu_trees, A, hs, n, 0, 1, lib.rt_scene_destroy)  # warm
        case["create_host_ms"] = create_ms(lib.rt_scene_create_ex, A, hs, n, None, reps, lib.rt_scene_destroy)
        case["create_gpu_tree_ms"] = create_ms(lib.rt_scene_create_gpu_tree, A, hs, n, 0, reps, lib.rt_scene_destroy)
        case["create_gpu_trees_ms"] = create_ms(lib.rt_scene_create_gpu_trees, A, hs, n, 0, reps, lib.rt_scene_destroy)
        print(n, {k: (v[len(v) // 2] if isinstance(v, list) else v) for k, v in case.items()}, flush=True)
    cross = None
    for n in LADDER:
        got = legs(n, args.reps)
        if got is None:
            ok = False
            continue
        h, d = got[0][len(got[0]) // 2], got[1][len(got[1]) // 2]
        result["ladder"][str(n)] = {"host_build_ms": h, "device_build_ms": d}
        cross = (cross if cross is not None else n) if d < h else None
    result["crossover_boxes"] = cross
    print("crossover", cross, flush=True)
    if args.parent_lib:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent-leg", "--parent-lib", args.parent_lib, "--sizes", ",".join(map(str, args.sizes)),
                              "--reps", str(args.reps)], capture_output=True, text=True, timeout=900)
        if out.returncode != 0:
            ok = False
            result["parent_error"] = out.stderr[-2000:]
        else:
            result["parent_create_gpu_tree_ms"] = json.loads(out.stdout.strip().splitlines()[-1])
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
