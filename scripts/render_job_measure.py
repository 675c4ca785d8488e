"""Render jobs on one MI355X: what polling and publishing cost, how fast a stop lands, what finishing costs (NOTES.md round 28).

  * an unstopped job's kernel_ms against rt_render_device_ex's, same build, on the bench frame and on the 41x71 fixture frame
    (medians of `--reps`, the two routes alternating);
  * stop latency: wall time from rt_render_job_stop to the end of rt_render_job_wait, the stop issued at about half of the frame's
    progress, beside the plan (the most a wave may still have in flight: one unit in pass A, two ranges of B_chunk pixels in pass B);
  * rt_render_job_finish after that stop against the share of a plain render the absent pixels would take.

usage: python scripts/render_job_measure.py [--reps 7] [--out profiles/r28/render_job_measure.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28", "render_job_measure.json"))
    args = ap.parse_args()

    import torch

    import ray_tracing_fsharp_amd as rt
    import scenes
    from ray_tracing_fsharp_amd._lib import check

    A, lib = rt._abi, rt.lib
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def frame(which):
        if which == "bench":
            objs, cam, w, h = rt.sample_images.config3_final(seed=2024, spp=500, depth=50, pixels=800)
            scene = rt.Scene.make(objs)
            scene.tune(w, h, cam, seed=2024 ^ 0x5EED, device=0)
            return scene, cam, w, h, 2024
        objs, cam, w, h = scenes.all_materials()
        return rt.Scene.make(objs), cam, w, h, 0

    def plain(scene, cam, w, h, seed, accum, rgb):
        st = A.rt_stats()
        check(lib.rt_render_device_ex(scene.handle, C.byref(cam.to_abi()), w, h, seed, 0, 0, 1, 2 * h + 1, 0, accum.data_ptr(), rgb.data_ptr(), stream, None,
                                      C.byref(st)))
        return st.kernel_ms

    def launch_plan():
        words = (C.c_int64 * 96)()
        check(lib.rt_dev_last_launch_plan(words))
        return list(words)

    out = {"reps": args.reps, "device": torch.cuda.get_device_name(0)}
    for which in ("bench", "all_materials_41x71"):
        scene, cam, w, h, seed = frame("bench" if which == "bench" else "small")
        rows, cols = 2 * h + 1, 2 * w + 1
        accum = torch.empty((rows, cols, 4), dtype=torch.int32, device=dev)
        rgb = torch.empty((rows, cols, 3), dtype=torch.uint8, device=dev)
        ref_a, ref_c = torch.empty_like(accum), torch.empty_like(rgb)
        plain(scene, cam, w, h, seed, ref_a, ref_c)  # warm: kernels loaded, pools set up
        with scene.render_job(w, h, cam, seed=seed, accum=accum, rgb=rgb) as job:
            job.wait()
            same = bool(torch.equal(accum, ref_a) and torch.equal(rgb, ref_c))
            plan = job.plan()
        t_plain, t_job = [], []
        for _ in range(args.reps):  # the routes alternating
            t_plain.append(plain(scene, cam, w, h, seed, ref_a, ref_c))
            with scene.render_job(w, h, cam, seed=seed, accum=accum, rgb=rgb) as job:
                t_job.append(job.wait()["stats"]["kernel_ms"])
        entry = {"pixels": rows * cols, "job_plan": plan, "job_equals_plain": same,
                 "plain_kernel_ms": t_plain, "job_kernel_ms": t_job,  # (the job's covers its finishing kernels too)
                 "plain_median_ms": statistics.median(t_plain), "job_median_ms": statistics.median(t_job)}
        entry["job_over_plain"] = entry["job_median_ms"] / entry["plain_median_ms"]
        if which == "bench":
            # stop at about half of the frame's progress; then finish
            stops = []
            for _ in range(args.reps):
                with scene.render_job(w, h, cam, seed=seed, accum=accum, rgb=rgb) as job:
                    deadline = time.monotonic() + 10.0
                    while job.progress()["pixels_final"] < rows * cols // 2 and time.monotonic() < deadline:
                        pass
                    at = job.progress()["pixels_final"]
                    t0 = time.perf_counter()
                    job.stop()
                    res = job.wait()
                    latency = (time.perf_counter() - t0) * 1e3
                    t1 = time.perf_counter()
                    fin = job.finish()
                    fin_wall = (time.perf_counter() - t1) * 1e3
                    stops.append({"progress_at_stop": at, "n_present": res["n_present"], "stop_to_wait_end_ms": latency,
                                  "job_kernel_ms": res["stats"]["kernel_ms"], "samples_traced": res["stats"]["samples"],
                                  "finish_pixels": fin["pixels"], "finish_kernel_ms": fin["kernel_ms"], "finish_wall_ms": fin_wall,
                                  "finished_equals_plain": bool(torch.equal(accum, ref_a) and torch.equal(rgb, ref_c)), "plan": job.plan()})
            entry["stops"] = stops
            entry["stop_latency_median_ms"] = statistics.median(s["stop_to_wait_end_ms"] for s in stops)
            entry["finish_kernel_median_ms"] = statistics.median(s["finish_kernel_ms"] for s in stops)
            entry["finish_wall_median_ms"] = statistics.median(s["finish_wall_ms"] for s in stops)
            entry["absent_fraction_median"] = statistics.median(1.0 - s["n_present"] / (rows * cols) for s in stops)
            entry["plain_share_of_absent_ms"] = entry["absent_fraction_median"] * entry["plain_median_ms"]
            # a stop from a second thread while this one waits (the mid-flight test's shape), at the first sign of progress
            with scene.render_job(w, h, cam, seed=seed, accum=accum, rgb=rgb) as job:
                while job.progress()["pixels_final"] == 0:
                    pass
                th = threading.Thread(target=job.stop)
                th.start()
                res = job.wait()
                th.join()
                entry["early_stop_fraction_present"] = res["n_present"] / (rows * cols)
            plain(scene, cam, w, h, seed, ref_a, ref_c)
            lp = launch_plan()
            entry["plain_launch_plan"] = {"two_pass": lp[28], "A_chunk": lp[35 + 14 + 3], "B_chunk": lp[35 + 28 + 3], "total_waves": lp[35 + 28 + 13]}
        out[which] = entry
        print(which, json.dumps({k: v for k, v in entry.items() if not isinstance(v, list)}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
