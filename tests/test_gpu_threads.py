"""The library from many host threads at once ("Ownership": a scene handle may be used from any thread;
rt_last_error() and rt_last_stage_stats() are per thread).  A caller renders like the reference's Async.Parallel rows
(ImageOutput.fs:142): row blocks of one scene forced from whichever pool thread asks first.

Every call must return RT_OK and every result must equal, bit for bit, the serial result -- which is itself held to the CPU oracle
here or by the serial tests.  Concurrent renders of one scene call the ABI directly, never Scene.render_rows (conftest.py's
RTFS_TUNE wrapper tunes a scene on first use, which must not race its renders); no rt_set_* setter is called (they would change
every thread's defaults): launch settings travel in rt_render_options."""
import collections
import ctypes as C
import os
import random
import threading
import time

import numpy as np
import pytest

import scenes
from test_gpu_ray_queries import _oracle_hits, _oracle_trace, _same_f64
from test_oracle_render import FIXTURES

pytestmark = pytest.mark.gpu

A = scenes.rt._abi
lib = scenes.rt.lib
N_THREADS = 8


def _flat(rt, objs):
    return rt.raytracing.flatten_hittables(objs)


def _scene(rt, flat, walk_tree=-1):
    """A fresh handle (no device copy yet: its first render uploads it)."""
    hs, n, tex, ntex, keep = flat
    out = C.c_void_p()
    opt = A.rt_scene_options(walk_tree)
    rt._lib.check(lib.rt_scene_create_ex(hs, n, tex, ntex, C.byref(opt), C.byref(out)))
    return rt.Scene(out.value, keep)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _render(s, cam, w, h, seed, first=0, n_rows=None, flags=0):
    """rt_render (host buffers, synchronous) -> (status, accum, rgb, stats)."""
    rows, cols = 2 * h + 1, 2 * w + 1
    n_rows = rows - first if n_rows is None else n_rows
    accum = np.zeros((n_rows, cols, 4), np.int32)
    rgb = np.zeros((n_rows, cols, 3), np.uint8)
    st = A.rt_stats()
    camabi = cam.to_abi()
    rc = lib.rt_render(s.handle, C.byref(camabi), w, h, seed, 0, first, 1, n_rows, flags, _p(accum, C.c_int32), _p(rgb, C.c_uint8), C.byref(st))
    return rc, accum, rgb, st


def _last_error():
    return (lib.rt_last_error() or b"").decode("utf-8", "replace")


def _run_threads(n, body):
    """n threads released together by a barrier; the first exception of any of them is raised in the caller."""
    barrier = threading.Barrier(n)
    errors = []

    def run(t):
        try:
            barrier.wait()
            body(t)
        except BaseException as e:  # noqa: BLE001 (re-raised below)
            errors.append(e)
            barrier.abort()

    threads = [threading.Thread(target=run, args=(t,)) for t in range(n)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    if errors:
        raise errors[0]


# ---- 1. one scene, row blocks from many threads ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["oracle_all_materials_seed0", "oracle_final_thumb_seed7", "oracle_earth_thumb_seed3"])
def test_row_blocks_of_one_scene_from_8_threads(rt, name):
    """INTEGRATION.md's shim: each thread renders a disjoint block of rows of the SAME scene handle with host rt_render.  A new
    handle every round, so the lazy device upload (device_scene) is raced as well.  The frame equals one whole-frame call and the
    oracle's (the committed fixture)."""
    g = scenes.golden(name)
    objs, cam, w, h = FIXTURES[name](rt)
    seed = int(g["seed"])
    flat = _flat(rt, objs)
    rc, whole, whole_rgb, _ = _render(_scene(rt, flat), cam, w, h, seed)
    assert rc == A.RT_OK, _last_error()
    assert np.array_equal(whole, g["accum"]) and np.array_equal(whole_rgb, g["rgb"])
    rows = 2 * h + 1
    bounds = np.linspace(0, rows, N_THREADS + 1).astype(int)
    for _ in range(3):
        s = _scene(rt, flat)
        acc = np.zeros_like(whole)
        rgb = np.zeros_like(whole_rgb)
        codes = [None] * N_THREADS

        def body(t):
            first, n = int(bounds[t]), int(bounds[t + 1] - bounds[t])
            codes[t], acc[first:first + n], rgb[first:first + n], _ = _render(s, cam, w, h, seed, first, n)
            codes[t] = (codes[t], _last_error())

        _run_threads(N_THREADS, body)
        assert all(c[0] == A.RT_OK for c in codes), codes
        assert np.array_equal(acc, whole) and np.array_equal(rgb, whole_rgb)


# ---- 2. many instantiations at once ----------------------------------------------------------------------------------------
def _ray_inputs(n, seed):
    rays = scenes.random_rays(n, seed, origin_scale=4.0)
    rng = np.random.default_rng(seed).integers(1, 2**32, size=(n, 4), dtype=np.uint64).astype(np.uint32)
    return rays, rng


def test_many_instantiations_from_8_threads(rt, orc):
    """A table of (scene, entry point, options) jobs -- LDS-resident scenes of very different LDS sizes on the same kernel
    instantiation (the dynamic-LDS attribute belongs to the function, which all threads share), fused and two-pass launches at
    every block size, counters on and off, hybrid and global-memory scenes, a textured scene, hit queries and ray traces through
    the host and the device (torch, stream-ordered) variants -- run by 8 threads, each its own seeded shuffle of the table three
    times, device calls on a stream of its own with stats=None.  One synchronisation at the end, then every result is compared
    with its serial result; the serial results are compared with the oracle."""
    import torch

    defs = {  # name -> (objs, cam, w, h, seed)
        "lds_big": scenes.small_final(pixels=6) + (5,),               # the final scene's 485 spheres: most of the LDS
        "lds_small": scenes.many_spheres(n=30, seed=11, pixels=6) + (6,),  # 30 spheres: a few KiB of it
        "hybrid": scenes.many_spheres(n=1700, seed=12, pixels=4) + (7,),
        "global": scenes.many_spheres(n=17000, seed=13, pixels=3) + (8,),
        "tex": scenes.all_materials(pixels=6) + (9,),
    }
    sc = {k: _scene(rt, _flat(rt, v[0])) for k, v in defs.items()}
    info = {k: s.info() for k, s in sc.items()}
    if not (os.environ.get("RTFS_BLOCK") or os.environ.get("RTFS_CHUNK")):  # (the stress knobs of conftest.py change what fits)
        assert [info[k]["lds_resident"] for k in defs] == [1, 1, 0, 0, 1]
    assert info["lds_big"]["n_textures"] == info["lds_small"]["n_textures"] == 0 < info["tex"]["n_textures"]
    assert info["lds_big"]["scene_bytes"] > 10 * info["lds_small"]["scene_bytes"]

    # serial expectations, held to the oracle
    frame = {}
    for k, (objs, cam, w, h, seed) in defs.items():
        rc, acc, rgb, _ = _render(sc[k], cam, w, h, seed)
        assert rc == A.RT_OK, _last_error()
        oacc, orgb, _ = orc.OracleScene(objs).render_rows(w, h, cam.to_abi(), seed=seed, threads=4)
        assert np.array_equal(acc, oacc) and np.array_equal(rgb, orgb), k
        frame[k] = acc
    ray_scenes = ("lds_big", "lds_small", "hybrid", "tex")
    rays = {k: _ray_inputs(384, 40 + i) for i, k in enumerate(ray_scenes)}
    depth = 6
    hits, traces = {}, {}
    for k in ray_scenes:
        o = orc.OracleScene(defs[k][0])
        r, g = rays[k]
        hits[k] = sc[k].hitObject(r)
        want_h, want_s, _ = _oracle_hits(orc, o, r)
        assert np.array_equal(hits[k][0], want_h) and _same_f64(hits[k][1], want_s), k
        traces[k] = sc[k].traceRays(r, depth, rng=g)
        want_c, want_g = _oracle_trace(orc, o, r, depth, g)
        assert np.array_equal(traces[k][0], want_c) and np.array_equal(traces[k][1], want_g), k
    d_rays = {k: (torch.from_numpy(rays[k][0]).cuda(), torch.from_numpy(rays[k][1].view(np.int32)).cuda()) for k in ray_scenes}
    cams = {k: defs[k][1].to_abi() for k in defs}
    torch.cuda.synchronize()

    # the table: (tag, kind, scene, options kw, flags); "A"/"B": the same instantiation at two LDS sizes
    table = []
    for k in ("lds_big", "lds_small"):
        tag = "A" if k == "lds_big" else "B"
        table += [(tag, "dev", k, {}, 0)] * 10
        for kw in (dict(passes=2), dict(block_threads=256), dict(block_threads=512), dict(block_threads=768),
                   dict(block_threads=768, passes=2), dict(block_threads=256, passes=2), dict(passes=1, park_lanes=-1)):
            table.append(("", "dev", k, kw, 0))
        table += [("", "dev", k, {}, A.RT_RENDER_COUNTERS), ("", "dev", k, dict(passes=2), A.RT_RENDER_COUNTERS)]
        table.append(("", "host", k, {}, 0))
    table += [("", "dev", "hybrid", {}, 0), ("", "dev", "hybrid", dict(passes=2), 0), ("", "dev", "hybrid", {}, A.RT_RENDER_COUNTERS),
              ("", "dev", "global", {}, 0), ("", "dev", "global", {}, A.RT_RENDER_COUNTERS),
              ("", "dev", "tex", {}, 0), ("", "dev", "tex", dict(passes=2, block_threads=512), 0), ("", "dev", "tex", {}, A.RT_RENDER_COUNTERS),
              ("", "host", "tex", {}, 0)]
    for k in ray_scenes:
        table += [("", "hit", k, {}, 0), ("", "hit_dev", k, dict(block_threads=256), 0), ("", "hit_dev", k, {}, A.RT_RENDER_COUNTERS),
                  ("", "trace", k, {}, 0), ("", "trace_dev", k, {}, 0), ("", "trace_dev", k, dict(block_threads=256), A.RT_RENDER_COUNTERS)]
    reps = 3

    log = [[] for _ in range(N_THREADS)]  # per thread: (tag, t0, t1, status, message)
    results = [[] for _ in range(N_THREADS)]  # per thread: (job, output objects)
    streams = [torch.cuda.Stream() for _ in range(N_THREADS)]

    def run_job(t, job, stream):
        tag, kind, k, kw, flags = job
        objs, cam, w, h, seed = defs[k]
        opt = A.rt_render_options(**kw) if kw else None
        rows, cols = 2 * h + 1, 2 * w + 1
        t0 = time.perf_counter()
        rc, out = A.RT_OK, None
        try:
            if kind == "dev":
                out = torch.zeros((rows, cols, 4), dtype=torch.int32, device="cuda:0")
                t0 = time.perf_counter()
                rc = lib.rt_render_device_ex(sc[k].handle, C.byref(cams[k]), w, h, seed, 0, 0, 1, rows, flags, C.c_void_p(out.data_ptr()), None,
                                             C.c_void_p(stream.cuda_stream), C.byref(opt) if opt else None, None)
            elif kind == "host":
                rc, out, _, _ = _render(sc[k], cam, w, h, seed, flags=flags)
            elif kind == "hit":
                out = sc[k].hitObject(rays[k][0])
            elif kind == "trace":
                out = sc[k].traceRays(rays[k][0], depth, rng=rays[k][1])
            elif kind == "hit_dev":
                out = sc[k].hitObject(d_rays[k][0], counters=bool(flags), stats=False, options=opt)
            else:
                out = sc[k].traceRays(d_rays[k][0], depth, rng=d_rays[k][1], counters=bool(flags), stats=False, options=opt)
        except rt.RtError as e:
            rc = e.code
        t1 = time.perf_counter()
        log[t].append((tag, t0, t1, rc, _last_error() if rc != A.RT_OK else ""))
        results[t].append((job, out))

    def body(t):
        order = random.Random(1000 + t)
        with torch.cuda.stream(streams[t]):
            for _ in range(reps):
                jobs = list(table)
                order.shuffle(jobs)
                for job in jobs:
                    run_job(t, job, streams[t])

    _run_threads(N_THREADS, body)
    torch.cuda.synchronize()

    bad = collections.Counter((rc, msg) for calls in log for _, _, _, rc, msg in calls if rc != A.RT_OK)
    assert not bad, f"calls that failed: {dict(bad)}"
    for t in range(N_THREADS):
        assert len(results[t]) == reps * len(table)
        for (tag, kind, k, kw, flags), out in results[t]:
            where = (t, kind, k, kw, flags)
            if kind in ("dev", "host"):
                got = out.cpu().numpy() if kind == "dev" else out
                assert np.array_equal(got, frame[k]), where
            elif kind in ("hit", "hit_dev"):
                h_, s_ = (out[0].cpu().numpy(), out[1].cpu().numpy()) if kind == "hit_dev" else out
                assert np.array_equal(h_, hits[k][0]) and _same_f64(s_, hits[k][1]), where
            else:
                c_, g_ = (out[0].cpu().numpy(), out[1].cpu().numpy().view(np.uint32)) if kind == "trace_dev" else out
                assert np.array_equal(c_, traces[k][0]) and np.array_equal(g_, traces[k][1]), where
    # guard against a vacuous pass: launches of the two LDS sizes on the same instantiation were really in flight together
    spans = {tag: [(t, t0, t1) for t, calls in enumerate(log) for tg, t0, t1, _, _ in calls if tg == tag] for tag in "AB"}
    overlaps = sum(1 for ta, a0, a1 in spans["A"] for tb, b0, b1 in spans["B"] if ta != tb and a0 < b1 and b0 < a1)
    assert overlaps >= 20, f"only {overlaps} overlapping host-side calls of the two LDS sizes"


# ---- 3. errors and diagnostics belong to each thread -----------------------------------------------------------------------
def test_errors_and_stage_stats_belong_to_each_thread(rt):
    """Two threads make different failing calls in a loop while two others render: each failing thread reads its own message
    every time, the rendering threads never see a message, and rt_last_stage_stats()[8] (waves launched) is their own job's."""
    import torch

    big = scenes.small_final(pixels=6)
    small = scenes.many_spheres(n=30, seed=11, pixels=6)
    sb, ss = _scene(rt, _flat(rt, big[0])), _scene(rt, _flat(rt, small[0]))
    opt256 = A.rt_render_options(block_threads=256)
    bad_opt = A.rt_render_options(block_threads=100)

    def good(s, job, opt):
        objs, cam, w, h = job
        rows, cols = 2 * h + 1, 2 * w + 1
        out = torch.zeros((rows, cols, 4), dtype=torch.int32, device="cuda:0")
        st = A.rt_stats()
        camabi = cam.to_abi()
        rc = lib.rt_render_device_ex(s.handle, C.byref(camabi), w, h, 3, 0, 0, 1, rows, A.RT_RENDER_COUNTERS, C.c_void_p(out.data_ptr()), None,
                                     None, C.byref(opt) if opt else None, C.byref(st))
        stage = (C.c_uint64 * 16)()
        assert lib.rt_last_stage_stats(stage) == A.RT_OK
        return rc, out.cpu().numpy(), stage[8], st.rays

    want = {"big": good(sb, big, None), "small": good(ss, small, opt256)}
    assert want["big"][0] == want["small"][0] == A.RT_OK
    assert want["big"][2] != want["small"][2] > 0  # different wave counts: a mix-up would show
    rounds = 150
    seen = [None] * 4

    def body(t):
        camabi = big[1].to_abi()
        out = torch.zeros((13, 19, 4), dtype=torch.int32, device="cuda:0")
        msgs = set()
        for i in range(rounds if t < 2 else rounds // 5):
            if t == 0:
                rc = lib.rt_render_device_ex(sb.handle, C.byref(camabi), 9, 6, 3, 0, 0, 1, 13, 0, C.c_void_p(out.data_ptr()), None, None, C.byref(bad_opt), None)
                assert rc == A.RT_ERR_INVALID_ARGUMENT and _last_error() == "block_threads must be 0, 256, 512, 768 or 1024", (rc, _last_error())
            elif t == 1:
                rc = lib.rt_render_device_ex(sb.handle, C.byref(camabi), 9, 6, 3, 99, 0, 1, 13, 0, C.c_void_p(out.data_ptr()), None, None, None, None)
                assert rc == A.RT_ERR_INVALID_ARGUMENT and _last_error() == "device index out of range", (rc, _last_error())
            else:
                got = good(sb, big, None) if t == 2 else good(ss, small, opt256)
                assert got[0] == A.RT_OK and _last_error() == "", (t, _last_error())
                ref = want["big" if t == 2 else "small"]
                assert np.array_equal(got[1], ref[1]) and got[2] == ref[2] and got[3] == ref[3], t
            msgs.add(_last_error())
        seen[t] = msgs

    _run_threads(4, body)
    assert seen == [{"block_threads must be 0, 256, 512, 768 or 1024"}, {"device index out of range"}, {""}, {""}]


# ---- 4. tuning one scene while others render -------------------------------------------------------------------------------
def test_tune_one_scene_while_others_render(rt):
    """rt_scene_tune of scene A (which holds a device copy: the tune replaces it after a device-wide wait) while three threads
    render scenes B and C.  A is never rendered during its tune (the header forbids it).  Afterwards A equals the oracle's
    fixture and B and C never changed."""
    g = scenes.golden("oracle_final_thumb_seed7")
    a_objs, a_cam, aw, ah = FIXTURES["oracle_final_thumb_seed7"](rt)
    seed_a = int(g["seed"])
    b = scenes.all_materials(pixels=8)
    c = scenes.many_spheres(n=1700, seed=12, pixels=4)
    sb, scn = _scene(rt, _flat(rt, b[0])), _scene(rt, _flat(rt, c[0]))
    want_b, want_c = _render(sb, b[1], b[2], b[3], 2)[1], _render(scn, c[1], c[2], c[3], 3)[1]
    a_flat = _flat(rt, a_objs)
    done = threading.Event()
    out = {"tunes": [], "renders": [[] for _ in range(3)]}

    def body(t):
        if t == 0:
            try:
                for _ in range(3):
                    s = _scene(rt, a_flat, A.RT_WALK_TREE_SAH)  # (tunable whatever the process default)
                    rc, acc, _, _ = _render(s, a_cam, aw, ah, seed_a)
                    assert rc == A.RT_OK and np.array_equal(acc, g["accum"]), _last_error()
                    info = A.rt_tune_info()
                    rc = lib.rt_scene_tune(s.handle, C.byref(a_cam.to_abi()), aw, ah, seed_a, 0, C.byref(info))
                    assert rc == A.RT_OK and info.tuned == 1, (rc, _last_error())
                    rc, acc, rgb, _ = _render(s, a_cam, aw, ah, seed_a)
                    out["tunes"].append((rc, np.array_equal(acc, g["accum"]) and np.array_equal(rgb, g["rgb"])))
            finally:
                done.set()
        else:
            while not done.is_set():
                if t % 2:
                    rc, acc, _, _ = _render(sb, b[1], b[2], b[3], 2)
                    out["renders"][t - 1].append(rc == A.RT_OK and np.array_equal(acc, want_b))
                else:
                    rc, acc, _, _ = _render(scn, c[1], c[2], c[3], 3)
                    out["renders"][t - 1].append(rc == A.RT_OK and np.array_equal(acc, want_c))

    _run_threads(4, body)
    assert out["tunes"] == [(A.RT_OK, True)] * 3
    assert all(r and all(r) for r in out["renders"]), [len(r) for r in out["renders"]]


# ---- 5. rt_render_frame from two threads -----------------------------------------------------------------------------------
def test_render_frame_from_two_threads(rt):
    """rt_render_frame on one GPU listed twice (devices = [0, 0]) from two threads at once, under the peer-copy and host gathers
    (not RCCL: two threads' groups on one communicator are serialised by the library, but a one-GPU box cannot race them)."""
    objs, cam, w, h = scenes.all_materials(pixels=11)
    s = _scene(rt, _flat(rt, objs))
    want = s.render_frame(w, h, cam, seed=12, devices=(0,), gather=A.RT_GATHER_HOST)
    got = [[] for _ in range(2)]

    def body(t):
        for i in range(6):
            gather = A.RT_GATHER_PEER if (i + t) % 2 else A.RT_GATHER_HOST
            r = s.render_frame(w, h, cam, seed=12, devices=(0, 0), gather=gather)
            got[t].append(np.array_equal(r.accum, want.accum) and np.array_equal(r.rgb, want.rgb))

    _run_threads(2, body)
    assert got == [[True] * 6] * 2
