"""BoundingBoxTree.make's tree built on the GPU (csrc/rt_tree_kernels.h) against the host builder: every case of tests/tree_cases.py through
rt_tree_make (arrays, staged) and rt_tree_make_device (tensors, in place), all four outputs equal and the boxes by their bits; NULL outputs;
the NaN refusal; two builds in flight on two streams; and rt_scene_create_gpu_tree against rt_scene_create_ex -- the same scene."""
import ctypes as C

import numpy as np
import pytest

import scenes
import tree_cases

pytestmark = pytest.mark.gpu
rt = scenes.rt
P, S, H, Px, Tex = scenes.P, scenes.S, scenes.H, scenes.Px, scenes.Tex

_HOST = {}


def host(name):  # the yardstick, once per case, shared and left unchanged
    if name not in _HOST:
        _HOST[name] = rt.tree_make_host(tree_cases.case(name)[0])
    return _HOST[name]


def same_bits(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2].shape == b[2].shape
            and np.array_equal(np.ascontiguousarray(a[2]).view(np.uint64), np.ascontiguousarray(b[2]).view(np.uint64)) and np.array_equal(a[3], b[3]))


def to_numpy(ts):
    return tuple(t.cpu().numpy() for t in ts)


@pytest.mark.parametrize("name", tree_cases.names())
def test_device_build_equals_the_host_builder(name):
    import torch
    boxes, _ = tree_cases.case(name)
    arrays = rt.tree_make(boxes)
    assert same_bits(arrays, host(name)), "rt_tree_make"
    tensors = rt.tree_make(torch.from_numpy(boxes).cuda())
    assert all(t.is_cuda for t in tensors)
    assert same_bits(to_numpy(tensors), host(name)), "rt_tree_make_device"
    assert [x.tobytes() for x in to_numpy(tensors)] == [x.tobytes() for x in arrays]  # the same bytes through both routes


def _p(a, t):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


@pytest.mark.parametrize("name", ["lattice-65", f"tied_y-{tree_cases.S + 1}", f"zeros_raw-{2 * tree_cases.S + 3}"])
def test_null_outputs_are_honoured(name):
    import torch
    boxes, _ = tree_cases.case(name)
    n, nn, ref = len(boxes), 2 * len(boxes) - 1, host(name)
    for keep in range(4):  # one output at a time, the other three NULL
        outs = [np.full(nn, -7, np.int32), np.full(nn, -7, np.int32), np.full((nn, 6), -7.0), np.full(n, -7, np.int32)]
        args = [o if k == keep else None for k, o in enumerate(outs)]
        rt._lib.check(rt.lib.rt_tree_make(0, n, _p(boxes, C.c_double), _p(args[0], C.c_int32), _p(args[1], C.c_int32), _p(args[2], C.c_double), _p(args[3], C.c_int32)))
        assert outs[keep].tobytes() == np.ascontiguousarray(ref[keep]).tobytes()
        d = torch.from_numpy(boxes).cuda()
        t = [torch.full((nn,), -7, dtype=torch.int32, device="cuda"), torch.full((nn,), -7, dtype=torch.int32, device="cuda"),
             torch.full((nn, 6), -7.0, dtype=torch.float64, device="cuda"), torch.full((n,), -7, dtype=torch.int32, device="cuda")]
        ptr = [x.data_ptr() if k == keep else None for k, x in enumerate(t)]
        rt._lib.check(rt.lib.rt_tree_make_device(0, n, d.data_ptr(), *ptr, torch.cuda.current_stream().cuda_stream))
        assert t[keep].cpu().numpy().tobytes() == np.ascontiguousarray(ref[keep]).tobytes()
    rt._lib.check(rt.lib.rt_tree_make(0, n, _p(boxes, C.c_double), None, None, None, None))  # nothing asked for: nothing written


@pytest.mark.parametrize("n", [9, tree_cases.S, 2 * tree_cases.S + 3])
def test_nan_is_refused_on_the_device_and_sentinels_stay(n):
    import torch
    A = rt._abi
    boxes, _ = tree_cases.make("random", n)
    boxes[n // 2, 4] = np.nan
    nn = 2 * n - 1
    outs = [np.full(nn, -7, np.int32), np.full(nn, -7, np.int32), np.full((nn, 6), -7.0), np.full(n, -7, np.int32)]
    rc = rt.lib.rt_tree_make(0, n, _p(boxes, C.c_double), _p(outs[0], C.c_int32), _p(outs[1], C.c_int32), _p(outs[2], C.c_double), _p(outs[3], C.c_int32))
    assert rc == A.RT_ERR_INVALID_ARGUMENT and rt.lib.rt_last_error() == b"a box coordinate is NaN: it has no order; nothing was written"
    assert all((o == -7).all() for o in outs)
    d = torch.from_numpy(boxes).cuda()
    t = [torch.full((nn,), -7, dtype=torch.int32, device="cuda"), torch.full((nn,), -7, dtype=torch.int32, device="cuda"),
         torch.full((nn, 6), -7.0, dtype=torch.float64, device="cuda"), torch.full((n,), -7, dtype=torch.int32, device="cuda")]
    rc = rt.lib.rt_tree_make_device(0, n, d.data_ptr(), *[x.data_ptr() for x in t], torch.cuda.current_stream().cuda_stream)
    assert rc == A.RT_ERR_INVALID_ARGUMENT and rt.lib.rt_last_error() == b"a box coordinate is NaN: it has no order; nothing was written"
    assert all(bool((x == -7).all()) for x in t)
    with pytest.raises(rt.RtError):
        rt.tree_make(boxes)


def test_two_builds_of_different_sizes_in_flight_on_two_streams():
    """Scratch is stream-ordered: two host threads, each with a stream of its own, build at once."""
    import threading

    import torch
    names = ["tied_y-20011", f"lattice-{tree_cases.S - 1}"]
    dev = [torch.from_numpy(tree_cases.case(nm)[0]).cuda() for nm in names]
    torch.cuda.synchronize()
    got, streams = [None, None], [torch.cuda.Stream(), torch.cuda.Stream()]

    def work(k):
        with torch.cuda.stream(streams[k]):
            for _ in range(3):
                got[k] = rt.tree_make(dev[k])

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    for k, nm in enumerate(names):
        assert same_bits(to_numpy(got[k]), host(nm)), nm


def test_the_callers_current_device_is_left_as_it_was():
    import torch
    before = torch.cuda.current_device()
    rt.tree_make(tree_cases.case("random-65")[0], device=0)
    assert torch.cuda.current_device() == before


# ---- rt_scene_create_gpu_tree: the same scene ---------------------------------------------------------------------------------------
def _spheres(n, seed, negative=False):  # tests/test_walk_tree.py's
    rng = np.random.default_rng(seed)
    objs = []
    for i in range(n):
        c = P(float(rng.uniform(-9, 9)), float(rng.uniform(0, 4)), float(rng.uniform(-3, 15)))
        r = float(rng.uniform(0.05, 0.4)) * (-1.0 if negative and i % 7 == 0 else 1.0)
        objs.append(H.Sphere(rt.Sphere.make(S.LambertReflection(0.5, Tex(Px(9, 9, 9))), c, r)))
    objs.insert(n // 2, H.UnboundedSphere(rt.Sphere.make(S.LightSource(Tex(Px(1, 2, 3))), P(0.0, 0.0, 0.0), 500.0)))
    return objs


def _scene_objects(which):
    if which == "final":
        return rt.sample_images.config3_final(seed=2024, spp=40, depth=50, pixels=12)[0]
    if which == "negative700":
        return _spheres(700, 3, negative=True)
    if which == "random9000":
        return _spheres(9000, 4)
    if which == "two":
        return _spheres(2, 5)
    objs = _spheres(40, 6)  # "nan": one NaN box coordinate: the host builder's tree
    objs[7] = H.Sphere(rt.Sphere.make(S.LambertReflection(0.5, Tex(Px(9, 9, 9))), P(float("nan"), 1.0, 2.0), 0.3))
    return objs


@pytest.mark.parametrize("walk", ["sah", "reference"])
@pytest.mark.parametrize("which", ["final", "negative700", "random9000", "two", "nan"])
def test_scene_with_the_device_tree_is_the_same_scene(which, walk):
    objs = _scene_objects(which)
    a, b = rt.Scene.make(objs, walk_tree=walk), rt.Scene.make(objs, walk_tree=walk, tree_device=0)
    assert a.info() == b.info()
    if which == "final":
        assert a.info()["n_bounded"] == 485
    for get in ("tree", "walk_tree", "filter_tree"):
        for x, y in zip(getattr(a, get)(), getattr(b, get)()):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), get


@pytest.mark.parametrize("walk", ["sah", "reference"])
def test_a_small_render_is_the_same(walk):
    objs, cam, w, h = rt.sample_images.config2_three_lambert(spp=30, pixels=27)
    a = rt.Scene.make(objs, walk_tree=walk).render_rows(w, h, cam, seed=2, device=0)
    b = rt.Scene.make(objs, walk_tree=walk, tree_device=0).render_rows(w, h, cam, seed=2, device=0)
    assert np.array_equal(a.accum, b.accum) and np.array_equal(a.rgb, b.rgb)
    objs, cam, w, h = rt.sample_images.config3_final(seed=2024, spp=8, depth=50, pixels=12)
    a = rt.Scene.make(objs, walk_tree=walk).render_rows(w, h, cam, seed=1, device=0)
    b = rt.Scene.make(objs, walk_tree=walk, tree_device=0).render_rows(w, h, cam, seed=1, device=0)
    assert np.array_equal(a.accum, b.accum) and np.array_equal(a.rgb, b.rgb)
