"""What BoundingBoxTree.make's tree costs on the host and on one GPU, and what share of scene creation it is -- for n = 485, 1e4, 1e5 and 1e6
boxes of a final-scene-like input (every Min.y tied at 0.0) and of a random one:

  host        rt_tree_make_host, wall time (TreeBuilder on the CPUs this process may use)
  device      rt_tree_make_device between two events on the stream, boxes and outputs already on the device: warmed, repeated, all runs kept
  staged      rt_tree_make, wall time: device allocation, the copy of the boxes in, the build, the copies of the four arrays out
  create      rt_scene_create_ex against rt_scene_create_gpu_tree, wall time, under both walk trees; by difference: the tree's share,
              the surface-area build (sah minus reference), and the rest (ranks, object table, encode_image)
  parent      rt_scene_create_ex of another checkout (--parent-root: the parent commit's tree, built), in a fresh process

The host and the device leg alternate inside one call.  The device's four arrays are compared with the host's before anything is timed.
No threshold is set: the figures go to profiles/ and DESIGN.md.

usage: python scripts/tree_measure.py [--sizes 485,10000,100000,1000000] [--reps 5] [--parent-root DIR] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spheres(kind, n, seed=7):
    """[n, 4] centre and radius: "tied" as the final scene's small spheres sit on the floor (centre.y = radius: Min.y = 0.0), else random."""
    rng = np.random.default_rng(seed + n)
    side = max(11.0, float(np.sqrt(n)))
    r = rng.uniform(0.05, 0.4, n)
    c = np.stack([rng.uniform(-side, side, n), r if kind == "tied" else rng.uniform(0, 4, n), rng.uniform(-side, side, n)], 1)
    return np.concatenate([c, r[:, None]], 1)


def boxes_of(sp):
    b = np.empty((len(sp), 6))
    b[:, 0::2] = sp[:, :3] + (-sp[:, 3:4])
    b[:, 1::2] = sp[:, :3] + sp[:, 3:4]
    return b


def hittables(A, sp):
    hs = (A.rt_hittable * len(sp))()
    raw = np.frombuffer(hs, np.uint8).reshape(len(sp), C.sizeof(A.rt_hittable))
    proto = A.rt_hittable()
    proto.kind, proto.style, proto.texture, proto.albedo = A.RT_HITTABLE_SPHERE, A.RT_SPHERE_LAMBERT_REFLECTION, -1, 0.5
    raw[:] = np.frombuffer(proto, np.uint8)
    off_p, off_r = A.rt_hittable.point.offset, A.rt_hittable.radius.offset
    raw[:, off_p:off_p + 24] = np.ascontiguousarray(sp[:, :3]).view(np.uint8).reshape(len(sp), 24)
    raw[:, off_r:off_r + 8] = np.ascontiguousarray(sp[:, 3:4]).view(np.uint8).reshape(len(sp), 8)
    return hs


def create_ms(lib, A, hs, n, walk, device, reps):
    out, ts = C.c_void_p(), []
    opt = A.rt_scene_options(walk)
    for _ in range(reps):
        t0 = time.perf_counter()
        rc = (lib.rt_scene_create_ex(hs, n, None, 0, C.byref(opt), C.byref(out)) if device is None
              else lib.rt_scene_create_gpu_tree(hs, n, None, 0, C.byref(opt), device, C.byref(out)))
        ts.append(time.perf_counter() - t0)
        assert rc == 0, rc
        lib.rt_scene_destroy(out)
    return ts


def parent_leg(args):
    """In a fresh process, the package of the other checkout: rt_scene_create_ex alone."""
    sys.path.insert(0, os.path.abspath(args.parent_root))
    import ray_tracing_fsharp_amd as rt
    A = rt._abi
    res = {}
    for kind in ("tied", "random"):
        for n in args.sizes:
            hs = hittables(A, spheres(kind, n))
            reps = args.reps if n < 1000000 else min(args.reps, 3)
            res[f"{kind}-{n}"] = {w: sorted(1e3 * x for x in create_ms(rt.lib, A, hs, n, k, None, reps))
                                  for w, k in (("sah", A.RT_WALK_TREE_SAH), ("reference", A.RT_WALK_TREE_REFERENCE))}
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=[485, 10000, 100000, 1000000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--parent-leg", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.parent_leg:
        return parent_leg(args)
    sys.path.insert(0, ROOT)

    import torch

    import ray_tracing_fsharp_amd as rt
    from ray_tracing_fsharp_amd._lib import check
    A, lib = rt._abi, rt.lib
    med = lambda xs: 1e3 * float(np.median(xs))  # noqa: E731
    result = {"cpus": len(os.sched_getaffinity(0)), "omp_num_threads": os.environ.get("OMP_NUM_THREADS"), "reps": args.reps, "lds_boxes": int(lib.rt_tree_lds_boxes()),
              "cases": {}}
    ok = True
    for kind in ("tied", "random"):
        for n in args.sizes:
            sp = spheres(kind, n)
            b = boxes_of(sp)
            reps = args.reps if n < 1000000 else min(args.reps, 3)
            host = rt.tree_make_host(b)
            d = torch.from_numpy(b).cuda()
            dev = rt.tree_make(d)
            equal = all(np.ascontiguousarray(x).tobytes() == t.cpu().numpy().tobytes() for x, t in zip(host, dev))
            case = {"n": n, "depth": int(lib.rt_tree_depth(n)), "results_equal": bool(equal)}
            result["cases"][f"{kind}-{n}"] = case
            if not equal:
                ok = False
                case["error"] = "the device build differs from the host builder; nothing timed"
                continue
            nn = 2 * n - 1
            outs = [torch.empty(nn, dtype=torch.int32, device="cuda"), torch.empty(nn, dtype=torch.int32, device="cuda"),
                    torch.empty((nn, 6), dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")]
            h_outs = [np.zeros(nn, np.int32), np.zeros(nn, np.int32), np.zeros((nn, 6)), np.zeros(n, np.int32)]
            stream = torch.cuda.current_stream().cuda_stream
            i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)

            def host_leg():
                t0 = time.perf_counter()
                check(lib.rt_tree_make_host(n, b.ctypes.data_as(f64), h_outs[0].ctypes.data_as(i32), h_outs[1].ctypes.data_as(i32), h_outs[2].ctypes.data_as(f64),
                                            h_outs[3].ctypes.data_as(i32)))
                return time.perf_counter() - t0

            def device_leg():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                check(lib.rt_tree_make_device(0, n, d.data_ptr(), *[o.data_ptr() for o in outs], stream))
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) * 1e-3

            def staged_leg():
                t0 = time.perf_counter()
                check(lib.rt_tree_make(0, n, b.ctypes.data_as(f64), h_outs[0].ctypes.data_as(i32), h_outs[1].ctypes.data_as(i32), h_outs[2].ctypes.data_as(f64),
                                       h_outs[3].ctypes.data_as(i32)))
                return time.perf_counter() - t0

            device_leg(); device_leg(); staged_leg()  # warm-up (the host leg needs none beyond the comparison above)
            th, td, ts = [], [], []
            for _ in range(reps):  # alternating
                th.append(host_leg()); td.append(device_leg()); ts.append(staged_leg())
            case["host_ms"] = {"median": med(th), "all": sorted(1e3 * x for x in th)}
            case["device_events_ms"] = {"median": med(td), "all": sorted(1e3 * x for x in td)}
            case["staged_ms"] = {"median": med(ts), "all": sorted(1e3 * x for x in ts)}
            case["host_over_device"] = med(th) / med(td)
            case["host_over_staged"] = med(th) / med(ts)
            # scene creation, the two routes alternating, under both walk trees
            hs = hittables(A, sp)
            cr = {}
            for wname, walk in (("sah", A.RT_WALK_TREE_SAH), ("reference", A.RT_WALK_TREE_REFERENCE)):
                create_ms(lib, A, hs, n, walk, 0, 1)  # warm-up
                a_t, b_t = [], []
                for _ in range(reps):
                    a_t += create_ms(lib, A, hs, n, walk, None, 1)
                    b_t += create_ms(lib, A, hs, n, walk, 0, 1)
                cr[wname] = {"rt_scene_create_ex_ms": med(a_t), "rt_scene_create_gpu_tree_ms": med(b_t), "ex_all": sorted(1e3 * x for x in a_t),
                             "gpu_tree_all": sorted(1e3 * x for x in b_t)}
            case["create"] = cr
            ex_sah, gt_ref, gt_sah = cr["sah"]["rt_scene_create_ex_ms"], cr["reference"]["rt_scene_create_gpu_tree_ms"], cr["sah"]["rt_scene_create_gpu_tree_ms"]
            # By difference, from the device route's figures (they spread least): what is not the tree is the same host code on both routes.
            # Ranks, the object table and encode_image are one figure: nothing inside build_scene is timed.
            rest, sah = gt_ref - med(ts), gt_sah - gt_ref
            case["split_by_difference_ms"] = {
                "device_route": {"tree_kernels": med(td), "tree_copies_and_staging": med(ts) - med(td), "sah_build": sah, "ranks_table_encode_image": rest,
                                 "total": gt_sah},
                "host_route": {"tree": ex_sah - sah - rest, "sah_build": sah, "ranks_table_encode_image": rest, "total": ex_sah}}
            print(f"{kind}-{n}: host {med(th):.3f} ms, device {med(td):.3f} ms, staged {med(ts):.3f} ms, create ex {ex_sah:.3f} / gpu tree {gt_sah:.3f} ms", flush=True)
    if args.parent_root:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent-leg", "--parent-root", args.parent_root, "--sizes", ",".join(map(str, args.sizes)),
                              "--reps", str(args.reps)], capture_output=True, text=True)
        result["parent_rt_scene_create_ex_ms"] = json.loads(out.stdout.strip().splitlines()[-1]) if out.returncode == 0 else {"error": out.stderr[-400:]}
    else:
        result["parent_rt_scene_create_ex_ms"] = "not measured"
    text = json.dumps(result, indent=1)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
