"""The tree entry points' contract without a GPU (include/rtfs_amd.h, "BoundingBoxTree.make's tree on the device"): every refusal with its
message, before any device call; n = 0; RT_ERR_NO_DEVICE where there is no GPU; rt_tree_nodes and rt_tree_depth; and Scene.make with a
tree_device raises the no-device error before anything else."""
import ctypes as C

import numpy as np
import pytest

import tree_cases
import tree_model


def _msg(rt):
    return (rt.lib.rt_last_error() or b"").decode()


def _outs(n, fill=-7):
    nn = max(2 * n - 1, 0)
    return np.full(nn, fill, np.int32), np.full(nn, fill, np.int32), np.full((nn, 6), float(fill)), np.full(n, fill, np.int32)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def test_nodes_and_depth(rt):
    assert [rt.lib.rt_tree_nodes(n) for n in (0, 1, 2, 3, 485)] == [0, 1, 3, 5, 969]
    assert [rt.lib.rt_tree_depth(n) for n in (0, 1, 2, 3, 4, 485, 100000, 1000000, 4500000)] == [0, 1, 2, 3, 4, 11, 19, 22, 25]
    for n in list(range(1, 70)) + [2047, 2048, 2049, 4099, 20011]:
        assert rt.lib.rt_tree_depth(n) == tree_model.depth(n) == len(tree_model.plan(n))
    assert rt.lib.rt_tree_lds_boxes() == tree_cases.S


def test_refusals_of_the_host_builder_and_of_the_staging_call(rt):
    A = rt._abi
    b = np.zeros((3, 6))
    skip, prim, nb, order = _outs(3)
    for call in (lambda n, boxes: rt.lib.rt_tree_make_host(n, boxes, _p(skip, C.c_int32), _p(prim, C.c_int32), _p(nb, C.c_double), _p(order, C.c_int32)),
                 lambda n, boxes: rt.lib.rt_tree_make(0, n, boxes, _p(skip, C.c_int32), _p(prim, C.c_int32), _p(nb, C.c_double), _p(order, C.c_int32))):
        assert call(3, None) == A.RT_ERR_INVALID_ARGUMENT and _msg(rt) == "boxes is NULL"
        assert call(4500001, _p(b, C.c_double)) == A.RT_ERR_UNSUPPORTED and _msg(rt) == "more than 4,500,000 boxes (the scene's own limit)"
        assert call(0, None) == A.RT_OK  # a no-op, with or without a GPU
    assert (skip == -7).all() and (prim == -7).all() and (nb == -7.0).all() and (order == -7).all()  # nothing was written


def test_nan_is_refused_by_the_host_builder_and_nothing_is_written(rt):
    A = rt._abi
    b, _ = tree_cases.make("random", 9)
    b[4, 3] = np.nan
    skip, prim, nb, order = _outs(9)
    assert rt.lib.rt_tree_make_host(9, _p(b, C.c_double), _p(skip, C.c_int32), _p(prim, C.c_int32), _p(nb, C.c_double), _p(order, C.c_int32)) == A.RT_ERR_INVALID_ARGUMENT
    assert _msg(rt) == "a box coordinate is NaN: it has no order; nothing was written"
    assert (skip == -7).all() and (prim == -7).all() and (nb == -7.0).all() and (order == -7).all()
    with pytest.raises(rt.RtError) as e:
        rt.tree_make_host(b)
    assert e.value.code == A.RT_ERR_INVALID_ARGUMENT


def test_refusals_of_the_device_call_come_before_any_device_call(rt):
    """Misaligned addresses are never dereferenced: the checks run first, with or without a GPU."""
    A = rt._abi
    ok = 4096
    f = rt.lib.rt_tree_make_device
    assert f(0, 3, None, ok, ok, ok, ok, None) == A.RT_ERR_INVALID_ARGUMENT and _msg(rt) == "d_boxes is NULL"
    assert f(0, 3, ok + 4, ok, ok, ok, ok, None) == A.RT_ERR_INVALID_ARGUMENT and _msg(rt) == "d_boxes is not 8-byte aligned"
    assert f(0, 3, ok, ok, ok, ok + 4, ok, None) == A.RT_ERR_INVALID_ARGUMENT and _msg(rt) == "d_node_boxes is not 8-byte aligned"
    assert f(0, 3, ok, ok + 2, ok, ok, ok, None) == A.RT_ERR_INVALID_ARGUMENT and _msg(rt) == "d_skip is not 4-byte aligned"
    assert f(0, 3, ok, ok, ok + 1, ok, ok, None) == A.RT_ERR_INVALID_ARGUMENT and _msg(rt) == "d_prim is not 4-byte aligned"
    assert f(0, 3, ok, ok, ok, ok, ok + 3, None) == A.RT_ERR_INVALID_ARGUMENT and _msg(rt) == "d_order is not 4-byte aligned"
    assert f(0, 4500001, ok, ok, ok, ok, ok, None) == A.RT_ERR_UNSUPPORTED and _msg(rt) == "more than 4,500,000 boxes (the scene's own limit)"
    assert f(0, 4500001, ok + 4, ok, ok, ok, ok, None) == A.RT_ERR_INVALID_ARGUMENT  # an invalid argument is reported first
    assert f(0, 0, None, None, None, None, None, None) == A.RT_OK


def test_wrapper_refuses_what_is_not_a_box_array(rt):
    for bad in (np.zeros((3, 5)), np.zeros((3, 6), np.float32), np.zeros(6)):
        with pytest.raises(ValueError, match="boxes must be float64"):
            rt.tree_make_host(bad)
        with pytest.raises(ValueError, match="boxes must be float64"):
            rt.tree_make(bad)
    empty = rt.tree_make_host(np.zeros((0, 6)))
    assert [len(x) for x in empty] == [0, 0, 0, 0]


def test_without_a_gpu_the_device_routes_say_so(rt):
    if rt.device_count() > 0:
        return  # (tests/test_gpu_tree.py is this machine's part)
    A = rt._abi
    b, _ = tree_cases.make("random", 9)
    with pytest.raises(rt.RtError) as e:
        rt.tree_make(b)
    assert e.value.code == A.RT_ERR_NO_DEVICE
    assert rt.lib.rt_tree_make_device(0, 9, 4096, None, None, None, None, None) == A.RT_ERR_NO_DEVICE
    # Scene.make with a tree_device: the no-device error before anything else, a faulty scene included
    objs, cam, w, h = rt.sample_images.config2_three_lambert(spp=30, pixels=27)
    with pytest.raises(rt.RtError) as e:
        rt.Scene.make(objs, tree_device=0)
    assert e.value.code == A.RT_ERR_NO_DEVICE and "no HIP device visible" in e.value.message
    hs = (A.rt_hittable * 1)()
    hs[0].kind = 7
    out = C.c_void_p()
    assert rt.lib.rt_scene_create_gpu_tree(hs, 1, None, 0, None, 0, C.byref(out)) == A.RT_ERR_NO_DEVICE
    assert rt.lib.rt_scene_create_gpu_tree(hs, 1, None, 0, None, 0, None) == A.RT_ERR_INVALID_ARGUMENT and _msg(rt) == "out is NULL"
    assert rt.Scene.make(objs, tree_device=None).info()["n_nodes"] >= 1  # None: today's route
