"""BoundingBoxTree.make's tree over the named box sets of tests/tree_cases.py, without a GPU: the numpy model of the level-by-level build
(tests/tree_model.py, written from csrc/rt_tree_plan.h's rules) against the host builder through rt_tree_make_host BIT FOR BIT, against the
literal restatement of BoundingBoxTree.fs by VALUE (Python's min / max break a tie between -0.0 and +0.0 their own way, so `==` there and
bits against the host), and against Scene.make(...).tree() for the sets spheres can express.  Then three mutants of the model, each of
which a named case must catch: the cases are only worth something if they can tell these apart."""
import sys

import numpy as np
import pytest

import scenes
import fsharp_literal as fl
import tree_cases
import tree_model

rt = scenes.rt
P, S, H, Px, Tex = scenes.P, scenes.S, scenes.H, scenes.Px, scenes.Tex


def same_bits(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2].shape == b[2].shape
            and np.array_equal(np.ascontiguousarray(a[2]).view(np.uint64), np.ascontiguousarray(b[2]).view(np.uint64)) and np.array_equal(a[3], b[3]))


_MODEL = {}


def model(name):  # computed once per case, shared and left unchanged
    if name not in _MODEL:
        _MODEL[name] = tree_model.build(tree_cases.case(name)[0])
    return _MODEL[name]


def literal_arrays(boxes):
    """fsharp_literal.tree_make flattened to pre-order (skip, prim, boxes, order)."""
    tree = fl.tree_make([(i, ((r[0], r[2], r[4]), (r[1], r[3], r[5]))) for i, r in enumerate(boxes.tolist())])
    skip, prim, nb, order = [], [], [], []

    def walk(t):
        me = len(skip)
        skip.append(0)
        if t[0] == "Leaf":
            prim.append(t[1]); nb.append(t[2]); order.append(t[1])
        else:
            prim.append(-1); nb.append(t[3])
            walk(t[1]); walk(t[2])
        skip[me] = len(skip)
    walk(tree)
    flat = np.array([[b[0][0], b[1][0], b[0][1], b[1][1], b[0][2], b[1][2]] for b in nb], np.float64).reshape(-1, 6)
    return np.array(skip, np.int32), np.array(prim, np.int32), flat, np.array(order, np.int32)


@pytest.mark.parametrize("name", tree_cases.names())
def test_model_equals_the_host_builder_bit_for_bit(name):
    boxes, _ = tree_cases.case(name)
    host = rt.tree_make_host(boxes)
    assert len(host[0]) == rt.lib.rt_tree_nodes(len(boxes)) == 2 * len(boxes) - 1
    assert same_bits(model(name), host)
    assert sorted(host[3].tolist()) == list(range(len(boxes)))
    assert np.array_equal(host[1][host[1] >= 0], host[3])  # order: the Leaves in pre-order


@pytest.mark.parametrize("name", tree_cases.names())
def test_model_equals_the_literal_restatement_by_value(name):
    boxes, _ = tree_cases.case(name)
    sys.setrecursionlimit(100000)
    lit, m = literal_arrays(boxes), model(name)
    for k in range(4):
        assert np.array_equal(lit[k], m[k]), ("skip", "prim", "boxes", "order")[k]


@pytest.mark.parametrize("name", [n for n in tree_cases.names() if tree_cases.case(n)[1] is not None])
def test_model_equals_scene_make_for_what_spheres_can_express(name):
    _, spheres = tree_cases.case(name)
    style = S.LambertReflection(0.5, Tex(Px(9, 9, 9)))
    objs = [H.Sphere(rt.Sphere.make(style, P(float(c[0]), float(c[1]), float(c[2])), float(c[3]))) for c in spheres]
    skip, prim, nb = rt.Scene.make(objs, walk_tree="reference").tree()
    m = model(name)
    assert np.array_equal(skip, m[0]) and np.array_equal(prim, m[1]) and np.array_equal(nb.view(np.uint64), m[2].view(np.uint64))


# mutant of the model -> a named case that must catch it (found by running every case of at most 100 boxes against each mutant)
MUTANTS = {
    "ties broken by box index instead of position": (dict(tie="index"), "tied_y-9"),
    "left size c/2": (dict(left="half"), "random-3"),
    "the last minimum axis instead of the first": (dict(axis="last"), "lattice-4"),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_each_mutant_of_the_model_is_caught_by_a_named_case(mutant):
    kw, name = MUTANTS[mutant]
    boxes, _ = tree_cases.case(name)
    assert not same_bits(tree_model.build(boxes, **kw), rt.tree_make_host(boxes)), f"{name} does not tell '{mutant}' from the host builder"
    assert same_bits(tree_model.build(boxes), rt.tree_make_host(boxes))


def test_the_zero_cases_do_hold_both_zeros_in_branch_boxes():
    """What makes the bit comparison worth having: some Branch box of the zero cases carries -0.0 and some +0.0."""
    for name in ("zeros_sphere-65", "zeros_raw-65"):
        nb = model(name)[2]
        zero = nb == 0.0
        assert (np.signbit(nb) & zero).any() and (~np.signbit(nb) & zero).any()
