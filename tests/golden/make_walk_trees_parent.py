"""Writes tests/golden/walk_trees_parent.json: one SHA-256 of the skip and prim bytes of Scene.make(..., walk_tree="sah").walk_tree() per
sphere case of tests/walk_tree_cases.py.  Run it on the commit BEFORE csrc/rt_walk_plan.h existed (the parent of the commit that added this
file), with that commit's library built: the fixture then holds the refactored host builder to the trees the unrefactored one made.

    python tests/golden/make_walk_trees_parent.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import scenes  # noqa: E402
import walk_tree_cases as wc  # noqa: E402


def digest(skip, prim):
    return hashlib.sha256(skip.astype("<i4").tobytes() + prim.astype("<i4").tobytes()).hexdigest()


def main():
    out = {}
    for name in wc.sphere_names():
        sp = wc.case(name)[1]
        skip, prim, _ = scenes.rt.Scene.make(wc.sphere_objects(scenes.rt, scenes, sp), walk_tree="sah").walk_tree()
        out[name] = digest(skip, prim)
    with open(os.path.join(HERE, "walk_trees_parent.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} cases")


if __name__ == "__main__":
    main()
