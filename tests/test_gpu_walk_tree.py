"""The tree the device walks built on the GPU (csrc/rt_walk_kernels.h) against the host builder (rt_walk_tree_make_host): every case of
tests/walk_tree_cases.py through rt_walk_tree_make (arrays, staged) and rt_walk_tree_make_device (tensors, in place) -- skip and prim
identical, boxes equal as numbers, the two device routes byte for byte, a second build byte for byte; NULL outputs; the refusal of a
coordinate that is not finite; two builds in flight on two streams; and rt_scene_create_gpu_trees against rt_scene_create_ex -- the same
scene, the same frame, the same counters, before and after rt_scene_tune_rays."""
import ctypes as C

import numpy as np
import pytest

import scenes
import walk_tree_cases as wc

pytestmark = pytest.mark.gpu
rt = scenes.rt
P, S, H, Px, Tex = scenes.P, scenes.S, scenes.H, scenes.Px, scenes.Tex
NOT_FINITE = b"a box coordinate is not finite: a scene never builds the walk tree over such boxes; nothing was written"

_HOST = {}


def host(name):  # the yardstick, once per case, shared and left unchanged
    if name not in _HOST:
        _HOST[name] = rt.walk_tree_make_host(wc.case(name)[0])
    return _HOST[name]


def same_tree(a, b):  # skip and prim identical, boxes equal as numbers (the two zeros compare equal)
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2].shape == b[2].shape and bool((a[2] == b[2]).all())


def to_numpy(ts):
    return tuple(t.cpu().numpy() for t in ts)


def as_bytes(arrays):
    return [np.ascontiguousarray(x).tobytes() for x in arrays]


@pytest.mark.parametrize("name", wc.names())
def test_device_build_equals_the_host_builder(name):
    import torch
    boxes, _ = wc.case(name)
    arrays = rt.walk_tree_make(boxes)
    assert same_tree(arrays, host(name)), "rt_walk_tree_make"
    d = torch.from_numpy(boxes).cuda()
    tensors = rt.walk_tree_make(d)
    assert all(t.is_cuda for t in tensors)
    assert same_tree(to_numpy(tensors), host(name)), "rt_walk_tree_make_device"
    assert as_bytes(to_numpy(tensors)) == as_bytes(arrays)  # the same bytes through both routes
    assert as_bytes(to_numpy(rt.walk_tree_make(d))) == as_bytes(arrays)  # and from a second build


def _p(a, t):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


@pytest.mark.parametrize("name", ["lattice-65", f"tied_y-{wc.SWEEP + 1}", f"zeros_raw-{2 * wc.SWEEP + 3}"])
def test_null_outputs_are_honoured(name):
    import torch
    boxes, _ = wc.case(name)
    n, nn = len(boxes), 2 * len(boxes) - 1
    ref = rt.walk_tree_make(boxes)
    assert same_tree(ref, host(name))
    for keep in range(3):  # one output at a time, the others NULL
        outs = [np.full(nn, -7, np.int32), np.full(nn, -7, np.int32), np.full((nn, 6), -7.0)]
        args = [o if k == keep else None for k, o in enumerate(outs)]
        rt._lib.check(rt.lib.rt_walk_tree_make(0, n, _p(boxes, C.c_double), _p(args[0], C.c_int32), _p(args[1], C.c_int32), _p(args[2], C.c_double)))
        assert outs[keep].tobytes() == np.ascontiguousarray(ref[keep]).tobytes()
        d = torch.from_numpy(boxes).cuda()
        t = [torch.full((nn,), -7, dtype=torch.int32, device="cuda"), torch.full((nn,), -7, dtype=torch.int32, device="cuda"),
             torch.full((nn, 6), -7.0, dtype=torch.float64, device="cuda")]
        ptr = [x.data_ptr() if k == keep else None for k, x in enumerate(t)]
        rt._lib.check(rt.lib.rt_walk_tree_make_device(0, n, d.data_ptr(), *ptr, torch.cuda.current_stream().cuda_stream))
        assert t[keep].cpu().numpy().tobytes() == np.ascontiguousarray(ref[keep]).tobytes()
    rt._lib.check(rt.lib.rt_walk_tree_make(0, n, _p(boxes, C.c_double), None, None, None))  # nothing asked for: nothing written


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("n", [9, wc.SWEEP, 2 * wc.SWEEP + 3])
def test_a_coordinate_that_is_not_finite_is_refused_on_the_device_and_sentinels_stay(n, bad):
    import torch
    A = rt._abi
    boxes = wc.tree_cases.make("random", n)[0].copy()
    boxes[n // 2, 4] = bad
    nn = 2 * n - 1
    outs = [np.full(nn, -7, np.int32), np.full(nn, -7, np.int32), np.full((nn, 6), -7.0)]
    rc = rt.lib.rt_walk_tree_make(0, n, _p(boxes, C.c_double), _p(outs[0], C.c_int32), _p(outs[1], C.c_int32), _p(outs[2], C.c_double))
    assert rc == A.RT_ERR_INVALID_ARGUMENT and rt.lib.rt_last_error() == NOT_FINITE
    assert all((o == -7).all() for o in outs)
    d = torch.from_numpy(boxes).cuda()
    t = [torch.full((nn,), -7, dtype=torch.int32, device="cuda"), torch.full((nn,), -7, dtype=torch.int32, device="cuda"),
         torch.full((nn, 6), -7.0, dtype=torch.float64, device="cuda")]
    rc = rt.lib.rt_walk_tree_make_device(0, n, d.data_ptr(), *[x.data_ptr() for x in t], torch.cuda.current_stream().cuda_stream)
    assert rc == A.RT_ERR_INVALID_ARGUMENT and rt.lib.rt_last_error() == NOT_FINITE
    assert all(bool((x == -7).all()) for x in t)
    with pytest.raises(rt.RtError):
        rt.walk_tree_make(boxes)


def test_argument_checks_come_first():
    import torch
    A = rt._abi
    assert rt.lib.rt_walk_tree_make(0, 3, None, None, None, None) == A.RT_ERR_INVALID_ARGUMENT
    assert rt.lib.rt_walk_tree_make(0, 4500001, _p(np.zeros(6), C.c_double), None, None, None) == A.RT_ERR_UNSUPPORTED
    assert rt.lib.rt_walk_tree_make(0, 0, None, None, None, None) == A.RT_OK
    d = torch.zeros(16, dtype=torch.float64, device="cuda")
    assert rt.lib.rt_walk_tree_make_device(0, 2, d.data_ptr() + 4, None, None, None, None) == A.RT_ERR_INVALID_ARGUMENT
    assert rt.lib.rt_walk_tree_make_device(0, 2, d.data_ptr(), d.data_ptr() + 2, None, None, None) == A.RT_ERR_INVALID_ARGUMENT
    assert rt.lib.rt_walk_tree_make_device(0, 2, None, None, None, None, None) == A.RT_ERR_INVALID_ARGUMENT
    assert rt.lib.rt_walk_tree_make_device(0, 0, None, None, None, None, None) == A.RT_OK


def test_two_builds_of_different_sizes_in_flight_on_two_streams():
    """Scratch is stream-ordered: two host threads, each with a stream of its own, build at once."""
    import threading

    import torch
    names = ["tied_y-20011", wc.OUTLIER]
    dev = [torch.from_numpy(wc.case(nm)[0]).cuda() for nm in names]
    torch.cuda.synchronize()
    got, streams = [None, None], [torch.cuda.Stream(), torch.cuda.Stream()]

    def work(k):
        with torch.cuda.stream(streams[k]):
            for _ in range(3):
                got[k] = rt.walk_tree_make(dev[k])

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    for k, nm in enumerate(names):
        assert same_tree(to_numpy(got[k]), host(nm)), nm


def test_the_callers_current_device_is_left_as_it_was():
    import torch
    before = torch.cuda.current_device()
    rt.walk_tree_make(wc.case("random-65")[0], device=0)
    assert torch.cuda.current_device() == before


# ---- rt_scene_create_gpu_trees: the same scene ----------------------------------------------------------------------------------------
def _spheres(n, seed):
    rng = np.random.default_rng(seed)
    objs = []
    for i in range(n):
        c = P(float(rng.uniform(-9, 9)), float(rng.uniform(0, 4)), float(rng.uniform(-3, 15)))
        objs.append(H.Sphere(rt.Sphere.make(S.LambertReflection(0.5, Tex(Px(9, 9, 9))), c, float(rng.uniform(0.05, 0.4)))))
    objs.insert(n // 2, H.UnboundedSphere(rt.Sphere.make(S.LightSource(Tex(Px(1, 2, 3))), P(0.0, 0.0, 0.0), 500.0)))
    return objs


def _case(which):
    """(objects, camera, w, h)"""
    if which == "many2600":
        return scenes.many_spheres()
    _, cam, w, h = scenes.many_spheres(n=8)
    if which == "random5000":  # above 4096: the binned arm at the root
        return _spheres(5000, 4), cam, w, h
    if which == "two":
        return _spheres(2, 5), cam, w, h
    objs = _spheres(40, 6)  # "infinite": one infinite radius: the host builders' scene
    objs[7] = H.Sphere(rt.Sphere.make(S.LambertReflection(0.5, Tex(Px(9, 9, 9))), P(0.5, 1.0, 2.0), float("inf")))
    return objs, cam, w, h


def _same_scene(a, b):
    assert a.info() == b.info()
    for x, y in zip(a.tree(), b.tree()):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), "tree"
    (sa, pa, ba), (sb, pb, bb) = a.walk_tree(), b.walk_tree()
    assert np.array_equal(sa, sb) and np.array_equal(pa, pb) and ba.shape == bb.shape and bool((ba == bb).all()), "walk_tree"
    (fa, la), (fb, lb) = a.filter_tree(), b.filter_tree()
    assert np.array_equal(la, lb) and fa.shape == fb.shape and bool((fa == fb).all()), "filter_tree"


def _same_frame(a, b, cam, w, h):
    ra = a.render_rows(w, h, cam, seed=2, device=0, counters=True)
    rb = b.render_rows(w, h, cam, seed=2, device=0, counters=True)
    assert ra.accum.tobytes() == rb.accum.tobytes() and ra.rgb.tobytes() == rb.rgb.tobytes()
    for k in ("rays", "aabb_tests", "prim_tests", "reflections", "samples", "pixels_early"):
        assert ra.stats[k] == rb.stats[k], k


@pytest.mark.parametrize("which", ["many2600", "random5000"])
def test_scene_with_both_trees_from_the_device_is_the_same_scene(which):
    objs, cam, w, h = _case(which)
    a, b = rt.Scene.make(objs, walk_tree="sah"), rt.Scene.make(objs, walk_tree="sah", walk_tree_device=0)
    assert a.info()["n_bounded"] == {"many2600": 2600, "random5000": 5000}[which]
    _same_scene(a, b)
    _same_frame(a, b, cam, w, h)
    rng = np.random.default_rng(9)
    rays = np.concatenate([rng.uniform(-6, 6, (4000, 3)) + np.array([0.0, 2.0, 4.0]), rng.normal(size=(4000, 3))], 1)
    ta, tb = a.tune_rays(rays), b.tune_rays(rays)
    assert {k: v for k, v in ta.items() if not k.endswith("_ms")} == {k: v for k, v in tb.items() if not k.endswith("_ms")}  # (all but the times)
    _same_scene(a, b)
    _same_frame(a, b, cam, w, h)


@pytest.mark.parametrize("which,walk", [("many2600", "reference"), ("two", "sah"), ("infinite", "sah")])
def test_the_host_builder_routes_give_the_same_scene_too(which, walk):
    objs, cam, w, h = _case(which)
    a, b = rt.Scene.make(objs, walk_tree=walk), rt.Scene.make(objs, walk_tree=walk, walk_tree_device=0)
    _same_scene(a, b)
    for x, y in zip(a.walk_tree(), b.walk_tree()):  # the host builders' own trees: bit for bit
        assert x.tobytes() == y.tobytes()
    _same_frame(a, b, cam, w, h)
