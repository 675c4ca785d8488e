"""Render jobs on the GPU (rt_render_job_*, Scene.render_job / render_watch; DESIGN.md "Render jobs"), held to the committed oracle
fixtures, to the oracle computed here for a scene beyond the LDS, and -- on the bench frame -- to rt_render_device of the same build:
  * by budget (rt_dev_set_job_limits), deterministic: the present set is the model's from rt_dev_last_job_plan, every present pixel is the
    frame's bit for bit, every absent one zero, the counts agree, and rt_render_job_finish gives the whole frame;
  * the polled word itself: a job stopped while it waits behind another render renders nothing;
  * mid-flight: a stop from a second thread while the first sits in wait(), whatever it catches;
  * the partial spill against the host formatter, and through rt_resume_pixel_map back to the frame;
  * Scene.render_watch and the C consumer."""
import ctypes as C
import functools
import json
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EARLY = 11  # Count of a pixel that stopped after phase 1 (spp >= 12 in every frame here)
FIXTURES = {
    "all_materials": ("oracle_all_materials_seed0", lambda: scenes.all_materials(), (71, 41)),
    "final_thumb": ("oracle_final_thumb_seed7", lambda: scenes.small_final(), (49, 33)),
    "earth_thumb": ("oracle_earth_thumb_seed3", lambda: scenes.earth_thumb(scenes.golden("earthmap_rgb")["rgb"]), (65, 37)),
}
MANY = dict(spp=24, pixels=14)  # scenes.many_spheres: beyond the LDS; 49 x 29


@functools.lru_cache(maxsize=None)
def _frame(name):
    """(objects, camera, max_w, max_h, seed)"""
    if name == "many_spheres":
        return scenes.many_spheres(**MANY) + (11,)
    fixture, build, size = FIXTURES[name]
    objs, cam, w, h = build()
    assert (2 * w + 1, 2 * h + 1) == size
    return objs, cam, w, h, int(scenes.golden(fixture)["seed"])


@functools.lru_cache(maxsize=None)
def _scene(rt, name):
    return rt.Scene.make(_frame(name)[0])


@functools.lru_cache(maxsize=None)
def _want(orc, name):
    """The expected frame, (accum [rows, cols, 4], rgb [rows, cols, 3]): the committed fixture, or the oracle's frame computed once."""
    if name == "many_spheres":
        objs, cam, w, h, seed = _frame(name)
        acc, rgb, _ = orc.OracleScene(objs).render_rows(w, h, cam.to_abi(), seed=seed, threads=16)
    else:
        g = scenes.golden(FIXTURES[name][0])
        acc, rgb = np.array(g["accum"]), np.array(g["rgb"])
    acc.setflags(write=False); rgb.setflags(write=False)
    return acc, rgb


def _job(rt, name, *, passes=0, chunk=0, block=0, limits=(-1, -1), shard=(0, 1), fill=None, use_options=True):
    """A job of the frame (or of its rows shard[0]::shard[1]) into torch buffers, pre-filled with `fill` if given."""
    import torch
    from ray_tracing_fsharp_amd._lib import check
    objs, cam, w, h, seed = _frame(name)
    rows, cols = 2 * h + 1, 2 * w + 1
    n_rows = len(range(shard[0], rows, shard[1]))
    dev = torch.device("cuda", 0)
    mk = ((lambda s, t: torch.full(s, fill if t == torch.int32 else fill & 0xFF, dtype=t, device=dev)) if fill is not None else
          (lambda s, t: torch.empty(s, dtype=t, device=dev)))
    accum, rgb, present = mk((n_rows, cols, 4), torch.int32), mk((n_rows, cols, 3), torch.uint8), mk((n_rows, cols), torch.uint8)
    opts = rt._abi.rt_render_options(passes=passes, chunk_pixels=chunk, block_threads=block) if use_options else None
    check(rt.lib.rt_dev_set_job_limits(*limits))
    return _scene(rt, name).render_job(w, h, cam, seed=seed, row_first=shard[0], row_stride=shard[1], n_rows=n_rows, accum=accum, rgb=rgb,
                                       present=present, options=opts)


def _check_partial(job, res, want_acc, want_rgb, limits, what):
    """Everything the issue asks of a waited job; returns (plan, present)."""
    plan = job.plan()
    present = job.present.cpu().numpy().reshape(-1)
    acc, rgb = job.accum.cpu().numpy().reshape(-1, 4), job.rgb.cpu().numpy().reshape(-1, 3)
    want_acc, want_rgb = want_acc.reshape(-1, 4), want_rgb.reshape(-1, 3)
    n = present.size
    units_a = -(-n // plan["chunk"])
    assert plan["units_a"] == units_a and plan["chunk"] >= 1, what
    done_a = units_a if limits[0] < 0 else min(units_a, limits[0])
    assert plan["done_a"] == done_a, (what, plan)
    in_prefix = np.arange(n) // plan["chunk"] < done_a
    cont = want_acc[:, 0] != EARLY  # the pixels pass A hands to pass B
    if plan["passes"] == 1:
        assert plan["n_list"] == 0 and plan["done_b"] == 0, (what, plan)
        assert np.array_equal(present, in_prefix), what  # the model's set, exactly
    else:
        n_list = int((in_prefix & cont).sum())  # the live list: the continuing pixels of the rendered units
        done_b = n_list if limits[1] < 0 else min(n_list, limits[1])
        assert plan["n_list"] == n_list and plan["done_b"] == done_b, (what, plan, n_list, done_b)
        # the model's set, as far as the list's order (cost buckets: not part of the contract) lets it be named: nothing outside the
        # prefix, every early-stopping pixel inside it, and exactly done_b of its continuing ones
        assert not present[~in_prefix].any() and present[in_prefix & ~cont].all() and int(present[in_prefix & cont].sum()) == done_b, what
    assert np.array_equal(acc[present], want_acc[present]) and np.array_equal(rgb[present], want_rgb[present]), what
    assert not acc[~present].any() and not rgb[~present].any(), what
    assert res["n_present"] == int(present.sum()) == job.progress()["pixels_final"], what
    assert res["pixels_total"] == n and res["complete"] == bool(present.all()) and job.progress()["state"] == 2, what
    assert res["stats"]["pixels"] == res["n_present"] and res["stats"]["samples"] >= int(acc[:, 0].sum()), what
    return plan, present


def _check_finished(job, want_acc, want_rgb, what):
    job.finish()
    assert np.array_equal(job.accum.cpu().numpy(), want_acc) and np.array_equal(job.rgb.cpu().numpy(), want_rgb), what
    assert bool(job.present.all()) and job.progress()["pixels_final"] == want_acc.shape[0] * want_acc.shape[1], what


def _sweep(rt, orc, name, passes, chunk, limit_as, limit_bs_of, **kw):
    want_acc, want_rgb = _want(orc, name)
    shard = kw.get("shard", (0, 1))
    want_acc, want_rgb = want_acc[shard[0]::shard[1]], want_rgb[shard[0]::shard[1]]
    with _job(rt, name, passes=passes, chunk=chunk, **kw) as job:  # no budget: the whole frame, and the plan's numbers
        res = job.wait()
        plan, _ = _check_partial(job, res, want_acc, want_rgb, (-1, -1), (name, passes, chunk, "whole"))
        assert res["complete"] and not res["stop_requested"]
        assert np.array_equal(job.accum.cpu().numpy(), want_acc) and np.array_equal(job.rgb.cpu().numpy(), want_rgb)
        assert job.finish()["pixels"] == 0  # a complete job renders nothing
    assert plan["passes"] == passes
    units_a, flat = plan["units_a"], want_acc.reshape(-1, 4)
    runs = 0
    for limit_a in limit_as(units_a):
        n_list = int((flat[: limit_a * plan["chunk"], 0] != EARLY).sum())
        for limit_b in (limit_bs_of(n_list) if passes == 2 else (-1,)):
            what = (name, passes, chunk, limit_a, limit_b)
            with _job(rt, name, passes=passes, chunk=chunk, limits=(limit_a, limit_b), **kw) as job:
                res = job.wait()
                _check_partial(job, res, want_acc, want_rgb, (limit_a, limit_b), what)
                _check_finished(job, want_acc, want_rgb, what)
            runs += 1
    return runs


ALL_A = lambda u: sorted({0, 1, u // 2, u - 1, u})  # noqa: E731
ALL_B = lambda m: sorted({0, 1, m // 2, m})  # noqa: E731


@pytest.mark.parametrize("chunk", [16, 64])
@pytest.mark.parametrize("passes", [1, 2])
def test_a_budget_stops_the_job_at_exactly_the_models_prefix(rt, orc, passes, chunk):
    runs = _sweep(rt, orc, "all_materials", passes, chunk, ALL_A, ALL_B)
    assert runs >= (5 if passes == 1 else 8)  # (limit_a = 0 leaves an empty list, limit_a = 1 may: one run each)


@pytest.mark.parametrize("name", ["final_thumb", "earth_thumb", "many_spheres"])
def test_other_scenes_textured_and_beyond_the_lds(rt, orc, name):
    info = _scene(rt, name).info()
    assert info["lds_resident"] == (0 if name == "many_spheres" else 1)
    for passes in (1, 2):
        _sweep(rt, orc, name, passes, 16, lambda u: (u // 2,), lambda m: (m // 2,))


def test_an_interleaved_shard_a_small_block_and_prefilled_buffers(rt, orc):
    mid = lambda u: (1, u // 2)  # noqa: E731
    for passes in (1, 2):
        _sweep(rt, orc, "all_materials", passes, 16, mid, lambda m: (m // 2,), shard=(1, 2))
        _sweep(rt, orc, "all_materials", passes, 16, mid, lambda m: (m // 2,), block=256)
        _sweep(rt, orc, "all_materials", passes, 64, mid, lambda m: (0, m // 2), fill=-1)  # 0xFF in every byte: absent pixels are ZEROED


# ---- the bench frame --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bench(rt):
    """bench.py's frame (config 3, 2401 x 1601, 500 spp, tuned) and rt_render_device's render of it, on the GPU: computed once."""
    import torch
    from ray_tracing_fsharp_amd._lib import check
    objs, cam, w, h = rt.sample_images.config3_final(seed=2024, spp=500, depth=50, pixels=800)
    scene = rt.Scene.make(objs)
    scene.tune(w, h, cam, seed=2024 ^ 0x5EED, device=0)
    rows, cols = 2 * h + 1, 2 * w + 1
    dev = torch.device("cuda", 0)
    accum, rgb = torch.empty((rows, cols, 4), dtype=torch.int32, device=dev), torch.empty((rows, cols, 3), dtype=torch.uint8, device=dev)
    check(rt.lib.rt_render_device(scene.handle, C.byref(cam.to_abi()), w, h, 2024, 0, 0, 1, rows, 0, accum.data_ptr(), rgb.data_ptr(),
                                  torch.cuda.current_stream(dev).cuda_stream, None))
    torch.cuda.synchronize(dev)
    return scene, cam, w, h, accum, rgb


def _measurement(key, value):
    """Figures the tests observe, for profiles/r28: appended to $RTFS_JOB_MEASURE when that names a file (never read back here)."""
    path = os.environ.get("RTFS_JOB_MEASURE")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({key: value}) + "\n")


def test_the_polled_word_a_job_stopped_behind_another_render_renders_nothing(rt, orc):
    import torch
    from ray_tracing_fsharp_amd._lib import check
    scene, cam, w, h, _, _ = _bench(rt)
    want_acc, want_rgb = _want(orc, "all_materials")
    dev = torch.device("cuda", 0)
    rows, cols = 2 * h + 1, 2 * w + 1
    spare_a, spare_c = torch.empty((rows, cols, 4), dtype=torch.int32, device=dev), torch.empty((rows, cols, 3), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    # the bench frame (about 0.1 s) goes first on the stream; the job behind it cannot start before it ends
    check(rt.lib.rt_render_device(scene.handle, C.byref(cam.to_abi()), w, h, 2024, 0, 0, 1, rows, 0, spare_a.data_ptr(), spare_c.data_ptr(),
                                  torch.cuda.current_stream(dev).cuda_stream, None))
    with _job(rt, "all_materials", fill=-1, use_options=False) as job:
        job.stop()
        assert job.progress()["state"] == 1
        res = job.wait()
        assert res["stop_requested"] and not res["complete"] and res["n_present"] == 0
        assert not job.present.any() and not job.accum.any() and not job.rgb.any()
        assert job.progress() == {"state": 2, "pixels_total": want_acc.shape[0] * want_acc.shape[1], "pixels_final": 0}
        _check_finished(job, want_acc, want_rgb, "stopped before it began")
    # and a job nobody stops, with no budget and no options, is rt_render_device's frame byte for byte
    with _job(rt, "all_materials", fill=-1, use_options=False) as job:
        res = job.wait()
        assert res["complete"] and not res["stop_requested"] and res["n_present"] == res["pixels_total"]
        assert np.array_equal(job.accum.cpu().numpy(), want_acc) and np.array_equal(job.rgb.cpu().numpy(), want_rgb) and bool(job.present.all())


def test_a_stop_in_mid_flight_from_a_second_thread(rt):
    """The bench frame takes about 0.1 s (README) and the host reacts within that, so the stop lands inside the frame:
    0 < n_present < pixels_total.  Whatever it catches, the partial frame is exact and finish() completes it."""
    import torch
    scene, cam, w, h, ref_acc, ref_rgb = _bench(rt)
    dev = torch.device("cuda", 0)
    rows, cols = 2 * h + 1, 2 * w + 1
    accum = torch.empty((rows, cols, 4), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    with scene.render_job(w, h, cam, seed=2024, accum=accum) as job:
        polls, deadline = [], time.monotonic() + 10.0
        while time.monotonic() < deadline:  # the only polling loop: bounded by the deadline
            polls.append(job.progress()["pixels_final"])
            if polls[-1] > 0:
                break
        assert polls[-1] > 0, "no progress within 10 s"
        stopper = threading.Thread(target=job.stop)
        t0 = time.perf_counter()
        stopper.start()
        res = job.wait()  # (the stop arrives while this thread waits)
        latency_ms = (time.perf_counter() - t0) * 1e3
        stopper.join()
        polls.append(job.progress()["pixels_final"])
        assert all(a <= b for a, b in zip(polls, polls[1:])) and polls[-1] == res["n_present"] <= res["pixels_total"]
        present = job.present
        print(f"mid-flight: {res['n_present']} of {res['pixels_total']} pixels present, stop -> end of wait {latency_ms:.2f} ms")
        _measurement("mid_flight", {"n_present": res["n_present"], "pixels_total": res["pixels_total"], "stop_to_wait_end_ms": latency_ms,
                                    "plan": job.plan()})
        assert res["stop_requested"] and int(present.sum()) == res["n_present"]
        assert torch.equal(job.accum[present], ref_acc[present]) and torch.equal(job.rgb[present], ref_rgb[present])
        assert not job.accum[~present].any() and not job.rgb[~present].any()
        job.finish()
        assert torch.equal(job.accum, ref_acc) and torch.equal(job.rgb, ref_rgb) and bool(job.present.all())
        assert 0 < res["n_present"] < res["pixels_total"]


# ---- the partial spill ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", [1, 2])
def test_the_partial_spill_on_the_device_is_the_host_formatters(rt, orc, passes):
    import torch
    A = rt._abi
    want_acc, want_rgb = _want(orc, "all_materials")
    objs, cam, w, h, seed = _frame("all_materials")
    rows, cols = want_rgb.shape[:2]
    with _job(rt, "all_materials", passes=passes, chunk=16, limits=(70, 300)) as job:
        job.wait()
        present, rgb = job.present.cpu().numpy(), job.rgb.cpu().numpy()
        assert 0 < present.sum() < present.size
        got = job.pixel_map()
        assert got == rt.ImageOutput.formatPixelMapPresent(rgb, present) and len(got) > 0
        # the reference's reader gives the present pixels back, and the resume path completes the frame from them
        back, there = np.zeros_like(rgb), np.zeros((rows, cols), np.uint8)
        u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))  # noqa: E731
        assert rt.lib.rt_parse_pixel_map(got, len(got), rows, cols, u8(back), u8(there)) == int(present.sum())
        assert np.array_equal(there.astype(bool), present)
        assert np.array_equal(_scene(rt, "all_materials").resume(w, h, cam, got, seed=seed), want_rgb)
        # a capacity one byte short is found on the device: the length is reported, nothing is written
        t_rgb, t_pr = job.rgb.contiguous(), job.present.to(torch.uint8).contiguous()
        out = torch.full((len(got),), 0xEE, dtype=torch.uint8, device=t_rgb.device)
        d_n = torch.zeros((), dtype=torch.int64, device=t_rgb.device)
        n = C.c_int64(0)
        stream = torch.cuda.current_stream(t_rgb.device).cuda_stream
        rc = rt.lib.rt_format_pixel_map_present_device(0, t_rgb.data_ptr(), t_pr.data_ptr(), rows, cols, out.data_ptr(), len(got) - 1, d_n.data_ptr(), stream, C.byref(n))
        assert rc == A.RT_ERR_INVALID_ARGUMENT and n.value == len(got) == int(d_n.item()) and bool((out == 0xEE).all())
        # without the host's count the call does not wait and reports through d_bytes alone
        assert rt.lib.rt_format_pixel_map_present_device(0, t_rgb.data_ptr(), t_pr.data_ptr(), rows, cols, out.data_ptr(), len(got) - 1, d_n.data_ptr(), stream, None) == A.RT_OK
        assert int(d_n.item()) == len(got) and bool((out == 0xEE).all())
        # the length alone, and with every pixel present rt_format_pixel_map's bytes
        assert rt.lib.rt_format_pixel_map_present_device(0, t_rgb.data_ptr(), t_pr.data_ptr(), rows, cols, None, 0, None, stream, C.byref(n)) == A.RT_OK
        assert n.value == len(got)
        job.finish()
        assert job.pixel_map() == rt.ImageOutput.formatPixelMap(want_rgb)


# ---- Python ---------------------------------------------------------------------------------------------------------------------
def test_render_watch_ticks_rows_and_its_map_resumes_to_the_frame(rt, orc):
    want_acc, want_rgb = _want(orc, "all_materials")
    objs, cam, w, h, seed = _frame("all_materials")
    rows = want_rgb.shape[0]
    scene = _scene(rt, "all_materials")
    ticks = []
    rgb, present, spill = scene.render_watch(lambda x: ticks.append(x), lambda: False, w, h, cam, seed=seed)
    assert ticks == [1.0] * rows and present.all() and np.array_equal(rgb, want_rgb) and spill == rt.ImageOutput.formatPixelMap(want_rgb)
    ticks.clear()
    rgb, present, spill = scene.render_watch(lambda x: ticks.append(x), lambda: len(ticks) >= 1, w, h, cam, seed=seed)
    assert len(ticks) <= rows and all(t == 1.0 for t in ticks) and len(ticks) == int(present.sum()) // want_rgb.shape[1]
    assert np.array_equal(rgb[present], want_rgb[present]) and not rgb[~present].any()
    assert spill == rt.ImageOutput.formatPixelMapPresent(rgb, present)
    assert np.array_equal(scene.resume(w, h, cam, spill, seed=seed), want_rgb)
    # the array route: the job's own buffers, arrays out, a given array filled
    mine = np.full(want_acc.shape, -1, np.int32)
    rt.lib.rt_dev_set_job_limits(5, -1)
    with scene.render_job(w, h, cam, seed=seed, accum=mine) as job:
        res = job.wait()
        assert isinstance(job.rgb, np.ndarray) and isinstance(job.present, np.ndarray) and 0 < res["n_present"] < res["pixels_total"]
        assert np.array_equal(mine, job.accum) and not mine[~job.present].any()
        job.finish()
        assert np.array_equal(mine, want_acc) and np.array_equal(job.rgb, want_rgb)


def build_render_job_smoke(tmp_path):
    exe = str(tmp_path / "render_job_smoke")
    libdir = os.path.join(ROOT, "ray-tracing-fsharp_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "render_job_smoke.c"),
                           "-L", libdir, "-lrtfs_amd", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    return exe


def test_c_program_runs_a_job_on_the_gpu(rt, tmp_path):
    out = subprocess.run([build_render_job_smoke(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "render job: argument checks ok" in out.stdout and "render job: 48 of 375 pixels before the budget, the frame finished on the GPU" in out.stdout
