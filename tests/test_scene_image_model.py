"""tests/scene_image_model.py -- the difference-array depth, the stable order by depth, the outward rounding, the ranks and the record
layout as the device route computes them -- held to rt_scene_create_ex on every case of tests/scene_device_cases.py, and three mutants of
it each caught by at least one case: the cases can tell a wrong order within a depth, a wrong rounding and a wrong rank apart.  No GPU."""
import numpy as np
import pytest

import scene_device_cases as sc
from scene_image_model import model


def compare(rt, name, walk, mutant=None):
    """-> the list of what differs between the model and the library's scene"""
    records, textures = sc.CASES[name]()
    code, scene, text = sc.create("rt_scene_create_ex", records, textures, walk)
    assert code == 0, text
    m = model(records, scene.tree(), scene.walk_tree(), mutant)
    fb, fl = scene.filter_tree()
    info = scene.info()
    bad = [k for k, v in m["info"].items() if info[k] != v]
    if not np.array_equal(fb.view(np.uint32), m["filter_boxes"].view(np.uint32)):
        bad.append("filter_boxes")
    if not np.array_equal(fl, m["filter_links"]):
        bad.append("filter_links")
    return bad


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_the_model_is_the_host_scene(rt, name):
    for walk in ("sah", "reference"):
        assert compare(rt, name, walk) == [], walk


@pytest.mark.parametrize("mutant", ["unstable", "nearest", "input-rank"])
def test_each_mutant_is_caught_by_a_case(rt, mutant):
    caught = [name for name in sorted(sc.CASES) if compare(rt, name, "sah", mutant)]
    assert caught, mutant
