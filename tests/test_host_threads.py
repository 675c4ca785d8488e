"""The host half of the boundary from many threads at once, and in a process that cannot start threads (no GPU involved).

include/rtfs_amd.h promises that no exception crosses the boundary and that rt_last_error() is per thread; INTEGRATION.md that a
scene handle may be used from any thread.  Scene builds and rt_scene_tune_rays start threads of their own (csrc/rt_scene.h: the
reference tree from 4096 leaves, the probe-count build from 48), so they are run here from 16 threads at once, and once in a
child process whose thread stacks cannot be mapped: every tree must equal a serial build's, bit for bit."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import scenes

rt = scenes.rt
A = rt._abi
check = rt._lib.check
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _threaded_objs():  # test_host_scene.py::test_flattened_tree_equals_the_pointer_tree[threaded]
    objs = scenes.many_spheres(n=40000, seed=8)[0]
    objs[100:140] = [objs[100]] * 40
    return objs


def _create(flat, walk_tree=-1):
    """rt_scene_create_ex on pre-flattened input (the Python flattening would hold the GIL and serialise the threads)."""
    hs, n, tex, ntex, keep = flat
    out = C.c_void_p()
    opt = A.rt_scene_options(walk_tree)
    check(rt.lib.rt_scene_create_ex(hs, n, tex, ntex, C.byref(opt), C.byref(out)))
    return rt.Scene(out.value, keep)


def _snapshot(s):
    return {"info": s.info(), "tree": s.tree(), "walk": s.walk_tree(), "filter": s.filter_tree()}


def _same(a, b):
    if a["info"] != b["info"]:
        return False
    for k in ("tree", "walk", "filter"):
        if not all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(a[k], b[k])):
            return False
    return True


def _run_threads(n, body):
    """n threads released together by a barrier; the first exception of any of them is raised here."""
    barrier = threading.Barrier(n)
    errors = []

    def run(t):
        try:
            barrier.wait()
            body(t)
        except BaseException as e:  # noqa: BLE001 (re-raised in the caller's thread)
            errors.append(e)
            barrier.abort()

    threads = [threading.Thread(target=run, args=(t,)) for t in range(n)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    if errors:
        raise errors[0]


def test_scenes_built_from_16_threads_equal_serial_builds():
    earth = scenes.golden("earthmap_rgb")["rgb"]
    sources = {
        "threaded": (_threaded_objs(), -1),                                      # threaded reference tree, binned SAH build
        "n6000": (scenes.many_spheres(n=6000, seed=3)[0], -1),                   # the same, above the 4096-leaf threshold
        "all_materials": (scenes.all_materials()[0], -1),
        "earth": (scenes.earth_thumb(earth)[0], -1),                             # textured
        "reference": (scenes.many_spheres(n=6000, seed=3)[0], A.RT_WALK_TREE_REFERENCE),  # walk tree chosen per scene
    }
    flats = {k: (rt.raytracing.flatten_hittables(objs), walk) for k, (objs, walk) in sources.items()}
    want = {k: _snapshot(_create(f, walk)) for k, (f, walk) in flats.items()}
    assert want["reference"]["info"]["walk_tree"] == A.RT_WALK_TREE_REFERENCE and want["n6000"]["info"]["walk_tree"] == A.RT_WALK_TREE_SAH
    plan = ["threaded"] * 3 + ["n6000"] * 4 + ["reference"] * 3 + ["all_materials"] * 3 + ["earth"] * 3
    got = [None] * len(plan)

    def body(t):
        f, walk = flats[plan[t]]
        got[t] = _snapshot(_create(f, walk))

    _run_threads(len(plan), body)
    for t, k in enumerate(plan):
        assert _same(got[t], want[k]), (t, k)


def test_tune_rays_on_different_scenes_from_8_threads():
    """rt_scene_tune_rays puts the upper subtrees of its build on threads of its own; eight scenes tuned at once (each thread its
    own scene and rays) give the trees of serial tunes."""
    final = rt.raytracing.flatten_hittables(rt.sample_images.config3_final()[0])
    big = rt.raytracing.flatten_hittables(scenes.many_spheres(n=6000, seed=3)[0])
    jobs = [(final if t % 2 == 0 else big, scenes.random_rays(4000 + 500 * t, 20 + t, origin_scale=8.0)) for t in range(8)]

    def tuned(flat, rays):
        s = _create(flat)
        info = s.tune_rays(rays)
        return info, _snapshot(s)

    want = [tuned(f, r) for f, r in jobs]
    assert all(info["tuned"] == 1 for info, _ in want)
    got = [None] * len(jobs)

    def body(t):
        got[t] = tuned(*jobs[t])

    _run_threads(len(jobs), body)
    for t in range(len(jobs)):
        assert got[t][0] == want[t][0] | {"build_ms": got[t][0]["build_ms"]}, t
        assert _same(got[t][1], want[t][1]), t


def test_last_error_belongs_to_the_calling_thread():
    """Argument checks made before any device call, with a message that names the thread's own index; 16 threads each fail
    200 times, read rt_last_error() after every call and must find their own message, never another thread's."""
    objs = scenes.all_materials()[0]
    n_threads, rounds = 16, 200
    bad = []
    for t in range(n_threads):
        hs, n, tex, ntex, keep = rt.raytracing.flatten_hittables(objs * 2)
        hs[t].style = 99  # -> "hittable <t>: bad style"
        bad.append((hs, n, tex, ntex, keep))
    lines = []

    def body(t):
        hs, n, tex, ntex, _ = bad[t]
        want = f"hittable {t}: bad style"
        out = C.c_void_p()
        for i in range(rounds):
            if i % 2:
                assert rt.lib.rt_scene_create(hs, n, tex, ntex, C.byref(out)) == A.RT_ERR_INVALID_ARGUMENT
                msg = rt.lib.rt_last_error().decode()
                assert msg == want, (t, msg)
            else:
                opt = A.rt_scene_options(walk_tree=3 + t)  # not a creation option
                assert rt.lib.rt_scene_create_ex(hs, n, tex, ntex, C.byref(opt), C.byref(out)) == A.RT_ERR_INVALID_ARGUMENT
                msg = rt.lib.rt_last_error().decode()
                assert msg.startswith("walk_tree must be"), (t, msg)
        lines.append(t)

    _run_threads(n_threads, body)
    assert sorted(lines) == list(range(n_threads))


# The child of test_a_process_that_cannot_start_threads: RLIMIT_STACK is 1 GiB (set before exec, so glibc takes it as the default
# thread stack), and after the imports RLIMIT_AS leaves 512 MiB: no thread stack can be mapped, the heap still has room.  Only
# host entry points are called (the import checks the ABI; scene builds, rt_scene_tune_rays and the tree getters touch no GPU).
_CHILD = r"""
import ctypes as C, os, resource, sys, threading
import numpy as np
sys.path[:0] = [sys.argv[1], os.path.join(sys.argv[1], "tests")]
import scenes
rt = scenes.rt
A = rt._abi
objs = scenes.many_spheres(n=6000, seed=3)[0]
flat = rt.raytracing.flatten_hittables(objs)
rays = scenes.random_rays(5000, 21, origin_scale=8.0)
huge = np.zeros(6_000_000 * C.sizeof(A.rt_hittable), np.uint8)  # (kind 0: spheres) counted in VmSize, pages never touched
vm = [int(l.split()[1]) * 1024 for l in open("/proc/self/status") if l.startswith("VmSize:")][0]
resource.setrlimit(resource.RLIMIT_AS, (vm + (512 << 20), resource.getrlimit(resource.RLIMIT_AS)[1]))
try:
    threading.Thread(target=lambda: None).start()
    print("SKIP: a thread still started under RLIMIT_STACK 1 GiB / RLIMIT_AS VmSize + 512 MiB", flush=True)
    sys.exit(0)
except RuntimeError:
    print("child: starting a thread is refused", flush=True)
hs, n, tex, ntex, keep = flat
out = C.c_void_p()
rc = rt.lib.rt_scene_create(hs, n, tex, ntex, C.byref(out))
print(f"child: 6000-sphere rt_scene_create -> {rc}", flush=True)
assert rc == A.RT_OK, rt.lib.rt_last_error()
s = rt.Scene(out.value, keep)
r = np.ascontiguousarray(rays)
ti = A.rt_tune_info()
rc = rt.lib.rt_scene_tune_rays(s.handle, r.ctypes.data_as(C.POINTER(C.c_double)), r.shape[0], C.byref(ti))
print(f"child: rt_scene_tune_rays -> {rc}, tuned {ti.tuned}", flush=True)
assert rc == A.RT_OK, rt.lib.rt_last_error()
np.savez(sys.argv[2], *s.tree(), *s.walk_tree(), *s.filter_tree())
big = C.c_void_p()
rc = rt.lib.rt_scene_create(huge.ctypes.data_as(C.POINTER(A.rt_hittable)), 6_000_000, None, 0, C.byref(big))
msg = rt.lib.rt_last_error().decode()
print(f"child: 6e6-hittable rt_scene_create -> {rc} ({msg})", flush=True)
assert rc == A.RT_ERR_HOST and not big.value, (rc, msg)
print("child: ok", flush=True)
"""


def _limits():
    import resource

    resource.setrlimit(resource.RLIMIT_STACK, (1 << 30, resource.getrlimit(resource.RLIMIT_STACK)[1]))


def test_a_process_that_cannot_start_threads(tmp_path):
    """Thread creation refused (EAGAIN): the tree builders build on the calling thread -- the same trees as a normal build -- and a
    build whose host copies exceed the address space returns RT_ERR_HOST.  Before, std::system_error escaped rt_scene_create and
    std::terminate killed the process (SIGABRT)."""
    import resource

    hard = resource.getrlimit(resource.RLIMIT_STACK)[1]
    if hard != resource.RLIM_INFINITY and hard < (1 << 30):
        pytest.skip(f"the hard RLIMIT_STACK ({hard}) is below the 1 GiB the child needs")
    out = tmp_path / "child.npz"
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    p = subprocess.run([sys.executable, "-s", "-c", _CHILD, ROOT, str(out)], preexec_fn=_limits, env=env, capture_output=True,
                       text=True, timeout=300)
    report = f"exit {p.returncode}\n--- stdout\n{p.stdout}--- stderr\n{p.stderr[-3000:]}"
    if p.returncode == 0 and p.stdout.startswith("SKIP:"):
        pytest.skip(p.stdout.strip())
    assert p.returncode == 0 and p.stdout.rstrip().endswith("child: ok"), report
    s = rt.Scene.make(scenes.many_spheres(n=6000, seed=3)[0])
    assert s.tune_rays(scenes.random_rays(5000, 21, origin_scale=8.0))["tuned"] == 1
    want = [*s.tree(), *s.walk_tree(), *s.filter_tree()]
    got = np.load(out)
    assert len(got.files) == len(want)
    for i, w in enumerate(want):
        g = got[f"arr_{i}"]
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8)), i
