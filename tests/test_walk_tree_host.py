"""The surface-area build of the tree the device walks, without a GPU: the numpy model of the rules (tests/walk_tree_model.py, written from
csrc/rt_walk_plan.h's comment) against the host builder through rt_walk_tree_make_host on every case of tests/walk_tree_cases.py -- skip
and prim identical, boxes equal as numbers; every Branch box the union of its leaves; prim a permutation; the case list really reaches
the three arms on both sides of 4096; four mutants of the model, each caught by a named case; the refusals; Scene.make's walk tree is this
builder's tree over its leaf boxes in rank order; and the recorded trees of the commit before csrc/rt_walk_plan.h existed
(tests/golden/walk_trees_parent.json), which hold the refactored SahBuilder to the unrefactored one."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import scenes
import walk_tree_cases as wc
import walk_tree_model as wm

rt = scenes.rt
HERE = os.path.dirname(os.path.abspath(__file__))

_HOST, _MODEL = {}, {}


def host(name):  # once per case, shared and left unchanged
    if name not in _HOST:
        _HOST[name] = rt.walk_tree_make_host(wc.case(name)[0])
    return _HOST[name]


def model(name):
    if name not in _MODEL:
        _MODEL[name] = wm.build(wc.case(name)[0])
    return _MODEL[name]


def same_tree(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2].shape == b[2].shape and bool((a[2] == b[2]).all())


def depth_of(skip):
    up, depth = [], 0
    for i, s in enumerate(skip.tolist()):
        while up and i >= up[-1]:
            up.pop()
        up.append(s)
        depth = max(depth, len(up))
    return depth


@pytest.mark.parametrize("name", wc.names())
def test_model_equals_the_host_builder(name):
    boxes, _ = wc.case(name)
    n = len(boxes)
    skip, prim, nb = host(name)
    assert len(skip) == rt.lib.rt_tree_nodes(n) == 2 * n - 1
    assert same_tree(model(name)[:3], host(name))
    assert sorted(prim[prim >= 0].tolist()) == list(range(n))  # a permutation of the boxes
    # every Leaf holds its box, every Branch the union of its two children (so of its leaves): from the last node to the first
    leaf = prim >= 0
    assert bool((nb[leaf] == boxes[prim[leaf]]).all())
    lo, hi = nb[:, 0::2].copy(), nb[:, 1::2].copy()
    for me in range(len(skip) - 1, -1, -1):
        if prim[me] < 0:
            l, r = me + 1, skip[me + 1]
            assert skip[r] == skip[me]
            assert bool((lo[me] == np.minimum(lo[l], lo[r])).all()) and bool((hi[me] == np.maximum(hi[l], hi[r])).all())
        else:
            assert skip[me] == me + 1


def test_the_cases_reach_all_three_arms_on_both_sides_of_the_threshold():
    """The depths and node sizes are the host builder's own (the model's counters say which arm made them)."""
    # identical spheres whose costs are exact: every split costs the same, one box is peeled per level until the depth guard halves
    assert depth_of(host("peel-64")[0]) == 53 == model("peel-64")[3]["depth"]
    assert depth_of(host("peel-4096")[0]) == 48 + 12 == model("peel-4096")[3]["depth"]  # 47 peels leave 4049 boxes at depth 48
    for n in (wc.SWEEP - 1, wc.SWEEP, wc.SWEEP + 1):
        assert depth_of(host(f"random-{n}")[0]) in (15, 16), n
    assert depth_of(host("random-20011")[0]) == 18
    assert model(f"random-{wc.SWEEP}")[3]["binned"] == 0 and model(f"random-{wc.SWEEP + 1}")[3]["binned"] >= 1
    assert model("random-20011")[3]["binned"] >= 3 and model("random-20011")[3]["median_above"] == []
    out = model(wc.OUTLIER)[3]
    assert out["binned"] == 47 and out["median_above"] == [4208]  # one outlier peeled per binned level, then the median arm above 4096
    assert depth_of(host(wc.OUTLIER)[0]) >= 48 + 12
    assert model(f"identical-{2 * wc.SWEEP + 3}")[3]["median_above"] == [2 * wc.SWEEP + 3, wc.SWEEP + 1, wc.SWEEP + 2]  # no winning axis: halved at once, twice
    assert model("identical-20011")[3]["binned"] == 0


def test_uniform_random_spheres_at_1e5_are_21_deep():
    assert depth_of(rt.walk_tree_make_host(wc.tree_cases.make("random", 100000)[0])[0]) == 21


# mutant of the model -> a named case that must catch it
MUTANTS = {
    "the last minimum instead of the first": (dict(last_min=True), "identical-5"),
    "31 bins": (dict(bins=31), f"random-{wc.SWEEP + 1}"),
    "weight 2i instead of 2i - 1": (dict(weight_off=0), "random-63"),
    "no clamp of inverted extents": (dict(clamp=False), "zeros_raw-63"),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_each_mutant_of_the_model_is_caught_by_a_named_case(mutant):
    kw, name = MUTANTS[mutant]
    boxes, _ = wc.case(name)
    assert not same_tree(wm.build(boxes, **kw)[:3], host(name)), f"{name} does not tell '{mutant}' from the host builder"
    assert same_tree(model(name)[:3], host(name))


def _p(a, t):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def test_refusals_come_before_anything_is_written():
    A = rt._abi
    assert rt.lib.rt_walk_tree_make_host(3, None, None, None, None) == A.RT_ERR_INVALID_ARGUMENT
    assert rt.lib.rt_walk_tree_make_host(4500001, _p(np.zeros(6), C.c_double), None, None, None) == A.RT_ERR_UNSUPPORTED
    assert rt.lib.rt_walk_tree_make_host(0, None, None, None, None) == A.RT_OK
    for bad in (np.nan, np.inf, -np.inf):
        boxes = wc.case("random-65")[0].copy()
        boxes[31, 3] = bad
        outs = [np.full(129, -7, np.int32), np.full(129, -7, np.int32), np.full((129, 6), -7.0)]
        rc = rt.lib.rt_walk_tree_make_host(65, _p(boxes, C.c_double), _p(outs[0], C.c_int32), _p(outs[1], C.c_int32), _p(outs[2], C.c_double))
        assert rc == A.RT_ERR_INVALID_ARGUMENT
        assert rt.lib.rt_last_error() == b"rt_walk_tree_make_host: a box coordinate is not finite: a scene never builds the walk tree over such boxes; nothing was written" \
            or rt.lib.rt_last_error() == b"a box coordinate is not finite: a scene never builds the walk tree over such boxes; nothing was written"
        assert all((o == -7).all() for o in outs)
    with pytest.raises(ValueError):
        rt.walk_tree_make_host(np.zeros((3, 5)))
    boxes = wc.case("lattice-65")[0]
    for keep in range(3):  # one output at a time
        outs = [np.full(129, -7, np.int32), np.full(129, -7, np.int32), np.full((129, 6), -7.0)]
        args = [o if k == keep else None for k, o in enumerate(outs)]
        rt._lib.check(rt.lib.rt_walk_tree_make_host(65, _p(boxes, C.c_double), _p(args[0], C.c_int32), _p(args[1], C.c_int32), _p(args[2], C.c_double)))
        assert outs[keep].tobytes() == np.ascontiguousarray(host("lattice-65")[keep]).tobytes()


def _scene_walk_tree(name):
    sp = wc.case(name)[1]
    return rt.Scene.make(wc.sphere_objects(rt, scenes, sp), walk_tree="sah")


@pytest.mark.parametrize("name", [n for n in wc.sphere_names() if len(wc.case(n)[0]) >= 3])
def test_scene_make_walks_this_builders_tree_over_its_leaf_boxes_in_rank_order(name):
    s = _scene_walk_tree(name)
    skip, prim, nb = s.tree()  # BoundingBoxTree.make's tree: its Leaves in pre-order are the ranks; prim = the hittable's index
    leaf = prim >= 0
    by_rank, hittable_of_rank = np.ascontiguousarray(nb[leaf]), prim[leaf]
    o_skip, o_prim, o_nb = rt.walk_tree_make_host(by_rank)
    o_prim = np.where(o_prim >= 0, hittable_of_rank[np.maximum(o_prim, 0)], -1).astype(np.int32)
    w_skip, w_prim, w_nb = s.walk_tree()
    assert w_skip.tobytes() == o_skip.tobytes() and w_prim.tobytes() == o_prim.tobytes() and w_nb.tobytes() == o_nb.tobytes()


def test_the_host_builder_still_makes_the_trees_recorded_before_the_refactor():
    with open(os.path.join(HERE, "golden", "walk_trees_parent.json")) as f:
        want = json.load(f)
    assert sorted(want) == sorted(wc.sphere_names())
    for name in wc.sphere_names():
        skip, prim, _ = _scene_walk_tree(name).walk_tree()
        got = hashlib.sha256(skip.astype("<i4").tobytes() + prim.astype("<i4").tobytes()).hexdigest()
        assert got == want[name], name
